// Second-stage few-shot ROI box head, the kernels that are not convolutions:
//   * level-routed 7x7 ROIAlign over the five FPN levels            (modeling/poolers.py:11-42,93-124)
//   * GroupNorm(32, C) + LeakyReLU(0.2) over [R][7][7][C] ROI maps  (roi_heads/box_head/box_head.py:43-66)
//   * arg-max over shots, softmax, BoxCoder.decode, clip            (box_head.py:239-252, box_head/inference.py:46-118,
//                                                                    modeling/box_coder.py:50-95)
// All HBM-bound.  The convolutions / fully connected layers of the head run on the implicit-GEMM kernels.
#include "osd_common.h"
#include "gn_act_rois.h"
#include "../../include/oneshotdet_hip_box_modes.h"

namespace {

inline int grid_for(long long work, int threads) {
  long long g = (work + threads - 1) / threads;
  return (int)(g < 1 ? 1 : (g > 1048576 ? 1048576 : g));
}

template <typename T> struct Chunk;
template <> struct Chunk<float> {
  static constexpr int E = 4;
  float v[4];
  __device__ __forceinline__ void load(const float* p) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  }
  __device__ __forceinline__ void store(float* p) const {
    f32x4 t = {v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4*>(p) = t;
  }
};
template <> struct Chunk<__bf16> {
  static constexpr int E = 8;
  float v[8];
  __device__ __forceinline__ void load(const __bf16* p) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
  }
  __device__ __forceinline__ void store(__bf16* p) const {
    bf16x8 t;
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = (__bf16)v[e];
    *reinterpret_cast<bf16x8*>(p) = t;
  }
};

struct PoolLevels {
  const void* x[OSD_MAX_ROI_LEVELS];
  int h[OSD_MAX_ROI_LEVELS];
  int w[OSD_MAX_ROI_LEVELS];
  float scale[OSD_MAX_ROI_LEVELS];
  int n_levels;
};

// LevelMapper (poolers.py:33-42) with BoxList.area's "+1" (bounding_box.py:226-236)
__device__ __forceinline__ int map_level(float x1, float y1, float x2, float y2, int k_min, int k_max) {
  const float area = (x2 - x1 + 1.f) * (y2 - y1 + 1.f);
  const float s = sqrtf(area);
  float lv = floorf(4.f + log2f(s / 224.f + 1e-6f));
  lv = fminf(fmaxf(lv, (float)k_min), (float)k_max);
  return (int)lv - k_min;
}

// One workgroup per ROI.  The 49 output cells x C channels are walked as (cell, 16-byte channel chunk) items, chunk
// fastest, so the four bilinear taps of a sample are contiguous channel runs of the NHWC level map.  Arithmetic and
// accumulation order of csrc/cuda/ROIAlign_cuda.cu:11-122 (w1*v1 + w2*v2 + w3*v3 + w4*v4 per sample, samples in
// (iy, ix) order, one division by the sample count).  ROIs past counts[image] give zero rows.
// (Tried: staging the ROI's pixel patch, one 64-channel slab per workgroup, in LDS before the taps - bit-identical, but
// 5 % slower end to end, 996 vs 1045 images/s: the vector L1 already serves the repeated taps, and the staged version
// pays a barrier, an LDS round trip and 4x the workgroups.)
// `sets_per_image`: ROI set (boxes / counts row) j reads image j / sets_per_image of the level maps — 1 for the per-pair entry, the
// class sweep's K for osd_roi_pool_levels_sweep (include/oneshotdet_hip.h); one body for both kernels.
template <typename T>
__device__ __forceinline__ void roi_pool_levels_body(const PoolLevels& lv, const float* __restrict__ boxes,
                                                     const int32_t* __restrict__ counts, T* __restrict__ y, int c, int max_rois,
                                                     int pool, int sampling, int y_stride, int32_t* __restrict__ level_out,
                                                     int sets_per_image) {
  constexpr int E = Chunk<T>::E;
  const int roi = blockIdx.x;
  const int img = roi / max_rois, ri = roi % max_rois;
  const int chunks = c / E;
  const int items = pool * pool * chunks;
  T* yr = y + (size_t)roi * pool * pool * y_stride;
  const bool live = counts == nullptr || ri < counts[img];
  if (!live) {
    Chunk<T> z;
#pragma unroll
    for (int e = 0; e < E; ++e) z.v[e] = 0.f;
    for (int it = threadIdx.x; it < items; it += blockDim.x) z.store(yr + (size_t)(it / chunks) * y_stride + (it % chunks) * E);
    if (level_out && threadIdx.x == 0) level_out[roi] = -1;
    return;
  }
  const float* bx = boxes + (size_t)roi * 4;
  const float x1 = bx[0], y1 = bx[1], x2 = bx[2], y2 = bx[3];
  const int k_min = 3, k_max = 3 + lv.n_levels - 1;     // -log2(scales[0]) .. -log2(scales[-1]) (poolers.py:73-75)
  const int l = map_level(x1, y1, x2, y2, k_min, k_max);
  if (level_out && threadIdx.x == 0) level_out[roi] = l;
  const int h = lv.h[l], w = lv.w[l];
  const float scale = lv.scale[l];
  const T* x = reinterpret_cast<const T*>(lv.x[l]) + (size_t)(img / sets_per_image) * h * w * c;
  const float rsw = x1 * scale, rsh = y1 * scale, rew = x2 * scale, reh = y2 * scale;
  const float roi_w = fmaxf(rew - rsw, 1.f), roi_h = fmaxf(reh - rsh, 1.f);
  const float bin_h = roi_h / (float)pool, bin_w = roi_w / (float)pool;
  const int gh = sampling > 0 ? sampling : (int)ceilf(roi_h / pool);
  const int gw = sampling > 0 ? sampling : (int)ceilf(roi_w / pool);
  const float count = (float)(gh * gw);
  for (int it = threadIdx.x; it < items; it += blockDim.x) {
    const int cell = it / chunks, ch = (it % chunks) * E;
    const int py = cell / pool, px = cell % pool;
    float acc[E];
#pragma unroll
    for (int e = 0; e < E; ++e) acc[e] = 0.f;
    if (gh <= 2 && gw <= 2) {
      // separable bilinear weights: the cell's samples are merged per axis first (equal pixel indices summed), so the
      // sampling-ratio-2 cell reads 3 x 3 (or fewer) taps instead of 16 — this kernel is bound by its tap loads
      int iyv[4], ixv[4];
      float wyv[4], wxv[4];
      int ny = 0, nx = 0;
      auto axis = [](float v0, int size, int* idx, float* wt, int& n) {
        float v = v0;
        if (v < -1.0f || v > (float)size) return;
        if (v <= 0.f) v = 0.f;
        int lo = (int)v, hi;
        if (lo >= size - 1) { hi = lo = size - 1; v = (float)lo; } else { hi = lo + 1; }
        const float fr = v - lo;
        const int ids[2] = {lo, hi};
        const float ws[2] = {1.f - fr, fr};
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          bool found = false;
#pragma unroll
          for (int q = 0; q < 4; ++q)
            if (q < n && idx[q] == ids[t]) { wt[q] += ws[t]; found = true; }
          if (!found) { idx[n] = ids[t]; wt[n] = ws[t]; ++n; }
        }
      };
      for (int iy = 0; iy < gh; ++iy) axis(rsh + py * bin_h + (iy + .5f) * bin_h / (float)gh, h, iyv, wyv, ny);
      for (int ix = 0; ix < gw; ++ix) axis(rsw + px * bin_w + (ix + .5f) * bin_w / (float)gw, w, ixv, wxv, nx);
      for (int a = 0; a < ny; ++a)
        for (int b = 0; b < nx; ++b) {
          Chunk<T> v;
          v.load(x + ((size_t)iyv[a] * w + ixv[b]) * c + ch);
          const float wgt = wyv[a] * wxv[b];
#pragma unroll
          for (int e = 0; e < E; ++e) acc[e] += wgt * v.v[e];
        }
      Chunk<T> o;
#pragma unroll
      for (int e = 0; e < E; ++e) o.v[e] = acc[e] / count;
      o.store(yr + (size_t)cell * y_stride + ch);
      continue;
    }
    for (int iy = 0; iy < gh; ++iy) {
      const float yy = rsh + py * bin_h + (iy + .5f) * bin_h / (float)gh;
      for (int ix = 0; ix < gw; ++ix) {
        const float xx = rsw + px * bin_w + (ix + .5f) * bin_w / (float)gw;
        float yv = yy, xv = xx;
        if (yv < -1.0f || yv > (float)h || xv < -1.0f || xv > (float)w) continue;
        if (yv <= 0.f) yv = 0.f;
        if (xv <= 0.f) xv = 0.f;
        int yl = (int)yv, xl = (int)xv, yh, xh;
        if (yl >= h - 1) { yh = yl = h - 1; yv = (float)yl; } else { yh = yl + 1; }
        if (xl >= w - 1) { xh = xl = w - 1; xv = (float)xl; } else { xh = xl + 1; }
        const float ly = yv - yl, lx = xv - xl, hy = 1.f - ly, hx = 1.f - lx;
        const float w1 = hy * hx, w2 = hy * lx, w3 = ly * hx, w4 = ly * lx;
        Chunk<T> v1, v2, v3, v4;
        v1.load(x + ((size_t)yl * w + xl) * c + ch);
        v2.load(x + ((size_t)yl * w + xh) * c + ch);
        v3.load(x + ((size_t)yh * w + xl) * c + ch);
        v4.load(x + ((size_t)yh * w + xh) * c + ch);
#pragma unroll
        for (int e = 0; e < E; ++e) acc[e] += w1 * v1.v[e] + w2 * v2.v[e] + w3 * v3.v[e] + w4 * v4.v[e];
      }
    }
    Chunk<T> o;
#pragma unroll
    for (int e = 0; e < E; ++e) o.v[e] = acc[e] / count;
    o.store(yr + (size_t)cell * y_stride + ch);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void roi_pool_levels_kernel(PoolLevels lv, const float* __restrict__ boxes,
                                                              const int32_t* __restrict__ counts, T* __restrict__ y, int c,
                                                              int max_rois, int pool, int sampling, int y_stride,
                                                              int32_t* __restrict__ level_out) {
  roi_pool_levels_body<T>(lv, boxes, counts, y, c, max_rois, pool, sampling, y_stride, level_out, 1);
}

template <typename T>
__global__ __launch_bounds__(256) void roi_pool_levels_sweep_kernel(PoolLevels lv, const float* __restrict__ boxes,
                                                                    const int32_t* __restrict__ counts, T* __restrict__ y, int c,
                                                                    int max_rois, int pool, int sampling, int y_stride,
                                                                    int32_t* __restrict__ level_out, int sets_per_image) {
  roi_pool_levels_body<T>(lv, boxes, counts, y, c, max_rois, pool, sampling, y_stride, level_out, sets_per_image);
}

// (GroupNorm(groups, C) + LeakyReLU(slope) of one ROI map per workgroup: gn_act_rois.h, shared with the query gallery's entry.)

// Per ROI: arg-max over the shots of each class logit and the box deltas that go with it (box_head.py:239-252),
// softmax over the two logits (inference.py:66), BoxCoder.decode of the class-1 deltas (box_coder.py:50-95), clip to
// the image (bounding_box.py:214-219).  pred: [shots][n*max_rois][pstride], columns 0..1 = logits, 2..9 = deltas.
// scores: class-1 probability, or -1 (= dropped by osd_rank_sort_gather) for ROIs past counts[image] and for
// probabilities that do not exceed `score_thresh` (inference.py:136).
// MODE = FEW_SHOT.SECOND_STAGE_CLS_LOSS (include/oneshotdet_hip_box_modes.h).  The one-logit modes ('focal_loss', 'mse_loss'):
// column 0 = the logit, 1..8 = deltas, score = sigmoid(logit) (inference.py:61-64,67-69); with several shots all 8 deltas come from
// the shot with the largest logit (the reference itself fails there, box_head.py:246-253, and the Python layer refuses it).
template <typename T, int MODE>
__device__ __forceinline__ void box_decode_body(const T* __restrict__ pred, const float* __restrict__ rois,
                                                const int32_t* __restrict__ counts, float* __restrict__ scores,
                                                float* __restrict__ boxes, float* __restrict__ logits_out,
                                                float* __restrict__ reg_out, int n, int max_rois, int shots, int pstride, float wx,
                                                float wy, float ww, float wh, float clip, float img_h, float img_w,
                                                float score_thresh, const float* __restrict__ img_hw) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * max_rois) return;
  const int img = i / max_rois, ri = i % max_rois;
  if (img_hw) {      // per-image true sizes of a padded batch
    img_h = img_hw[2 * img];
    img_w = img_hw[2 * img + 1];
  }
  const size_t shot_stride = (size_t)n * max_rois * pstride;
  const T* p0 = pred + (size_t)i * pstride;
  float d[8];
  float prob;
  if constexpr (MODE == OSD_BOX_CLS_CE) {
    float l[2];
    int arg[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      l[j] = to_f32(p0[j]);
      arg[j] = 0;
      for (int s = 1; s < shots; ++s) {
        const float v = to_f32(p0[s * shot_stride + j]);
        if (v > l[j]) { l[j] = v; arg[j] = s; }
      }
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int k = 0; k < 4; ++k) d[4 * j + k] = to_f32(p0[arg[j] * shot_stride + 2 + 4 * j + k]);
    if (logits_out) {
      logits_out[2 * (size_t)i] = l[0];
      logits_out[2 * (size_t)i + 1] = l[1];
    }
    const float m = fmaxf(l[0], l[1]);
    const float e0 = expf(l[0] - m), e1 = expf(l[1] - m);
    prob = e1 / (e0 + e1);
  } else {
    float l = to_f32(p0[0]);
    int arg = 0;
    for (int s = 1; s < shots; ++s) {
      const float v = to_f32(p0[s * shot_stride]);
      if (v > l) { l = v; arg = s; }
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) d[k] = to_f32(p0[arg * shot_stride + 1 + k]);
    if (logits_out) logits_out[i] = l;
    prob = 1.f / (1.f + expf(-l));
  }
  if (reg_out)
#pragma unroll
    for (int k = 0; k < 8; ++k) reg_out[8 * (size_t)i + k] = d[k];
  const float* b = rois + (size_t)i * 4;
  const float bw = b[2] - b[0] + 1.f, bh = b[3] - b[1] + 1.f;
  const float cx = b[0] + 0.5f * bw, cy = b[1] + 0.5f * bh;
  const float dx = d[4] / wx, dy = d[5] / wy;
  const float dw = fminf(d[6] / ww, clip), dh = fminf(d[7] / wh, clip);
  const float pcx = dx * bw + cx, pcy = dy * bh + cy;
  const float pw = expf(dw) * bw, ph = expf(dh) * bh;
  float ox1 = pcx - 0.5f * pw, oy1 = pcy - 0.5f * ph;
  float ox2 = pcx + 0.5f * pw - 1.f, oy2 = pcy + 0.5f * ph - 1.f;
  ox1 = fminf(fmaxf(ox1, 0.f), img_w - 1.f);
  oy1 = fminf(fmaxf(oy1, 0.f), img_h - 1.f);
  ox2 = fminf(fmaxf(ox2, 0.f), img_w - 1.f);
  oy2 = fminf(fmaxf(oy2, 0.f), img_h - 1.f);
  const bool live = (counts == nullptr || ri < counts[img]) && prob > score_thresh;
  scores[i] = live ? prob : -1.f;
  float* o = boxes + (size_t)i * 4;
  o[0] = ox1; o[1] = oy1; o[2] = ox2; o[3] = oy2;
}

// 'ce_loss', the config of record: the launch osd_box_decode has always made
template <typename T>
__global__ void box_decode_kernel(const T* __restrict__ pred, const float* __restrict__ rois, const int32_t* __restrict__ counts,
                                  float* __restrict__ scores, float* __restrict__ boxes, float* __restrict__ logits_out,
                                  float* __restrict__ reg_out, int n, int max_rois, int shots, int pstride, float wx,
                                  float wy, float ww, float wh, float clip, float img_h, float img_w, float score_thresh,
                                  const float* __restrict__ img_hw) {
  box_decode_body<T, OSD_BOX_CLS_CE>(pred, rois, counts, scores, boxes, logits_out, reg_out, n, max_rois, shots, pstride, wx, wy, ww,
                                     wh, clip, img_h, img_w, score_thresh, img_hw);
}

// the one-logit modes: the score is the same sigmoid in both, so one instantiation serves them
template <typename T>
__global__ void box_decode_sigmoid_kernel(const T* __restrict__ pred, const float* __restrict__ rois,
                                          const int32_t* __restrict__ counts, float* __restrict__ scores, float* __restrict__ boxes,
                                          float* __restrict__ logits_out, float* __restrict__ reg_out, int n, int max_rois,
                                          int shots, int pstride, float wx, float wy, float ww, float wh, float clip, float img_h,
                                          float img_w, float score_thresh, const float* __restrict__ img_hw) {
  box_decode_body<T, OSD_BOX_CLS_FOCAL>(pred, rois, counts, scores, boxes, logits_out, reg_out, n, max_rois, shots, pstride, wx, wy,
                                        ww, wh, clip, img_h, img_w, score_thresh, img_hw);
}

// add_gt_proposals (modeling/rpn/fcos/inference.py:139-160): per image the kept proposals followed by the ground-truth
// boxes with score 1 (cat_boxlist((proposal, gt_box))); rows past the new count are zero.
__global__ void append_gt_kernel(const float* __restrict__ boxes, const float* __restrict__ scores,
                                 const int32_t* __restrict__ counts, const float* __restrict__ gt, const int32_t* __restrict__ gt_count,
                                 float* __restrict__ out_boxes, float* __restrict__ out_scores, int32_t* __restrict__ out_counts,
                                 int n, int cap, int max_gt, int out_cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n * out_cap) return;
  const int img = i / out_cap, r = i % out_cap;
  const int c = min(counts[img], cap), g = min(gt_count[img], max_gt);
  float b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f, sc = 0.f;
  if (r < c) {
    const float* s = boxes + ((size_t)img * cap + r) * 4;
    b0 = s[0]; b1 = s[1]; b2 = s[2]; b3 = s[3];
    sc = scores[(size_t)img * cap + r];
  } else if (r < c + g) {
    const float* s = gt + ((size_t)img * max_gt + (r - c)) * 4;
    b0 = s[0]; b1 = s[1]; b2 = s[2]; b3 = s[3];
    sc = 1.f;
  }
  float* o = out_boxes + (size_t)i * 4;
  o[0] = b0; o[1] = b1; o[2] = b2; o[3] = b3;
  out_scores[i] = sc;
  if (r == 0) out_counts[img] = c + g;
}

}  // namespace

#define OSD_STREAM(s) reinterpret_cast<hipStream_t>(s)

extern "C" int osd_append_gt_boxes(const float* boxes, const float* scores, const int32_t* counts, const float* gt_boxes,
                                   const int32_t* gt_count, float* out_boxes, float* out_scores, int32_t* out_counts, int n,
                                   int cap, int max_gt, void* stream) {
  if (!boxes || !scores || !counts || !gt_boxes || !gt_count || !out_boxes || !out_scores || !out_counts || cap < 0 || max_gt < 0)
    return osd_fail(OSD_ERR_INVALID_ARG, "append_gt_boxes: bad args");
  const int out_cap = cap + max_gt;
  if (n == 0 || out_cap == 0) return OSD_OK;
  hipLaunchKernelGGL(append_gt_kernel, dim3(grid_for((long long)n * out_cap, 256)), dim3(256), 0, OSD_STREAM(stream), boxes,
                     scores, counts, gt_boxes, gt_count, out_boxes, out_scores, out_counts, n, cap, max_gt, out_cap);
  return osd_check_launch("append_gt_boxes");
}

extern "C" int osd_roi_pool_levels(int n_levels, const void* const* xs, const int32_t* hs, const int32_t* ws,
                                   const float* scales, const float* boxes, const int32_t* counts, void* y, int n, int c,
                                   int max_rois, int pool, int sampling_ratio, int y_stride, int32_t* level_out,
                                   int dtype, void* stream) {
  if (n_levels < 1 || n_levels > OSD_MAX_ROI_LEVELS || !xs || !hs || !ws || !scales || !boxes || !y)
    return osd_fail(OSD_ERR_INVALID_ARG, "roi_pool_levels: bad args");
  const int e = dtype == OSD_BF16 ? 8 : 4;
  if (c % e != 0 || y_stride < c || y_stride % e != 0 || pool < 1)
    return osd_fail(OSD_ERR_INVALID_ARG, "roi_pool_levels: channels %d / stride %d must be multiples of %d", c, y_stride, e);
  if (n * max_rois == 0) return OSD_OK;
  PoolLevels lv;
  lv.n_levels = n_levels;
  for (int l = 0; l < n_levels; ++l) {
    if (!xs[l]) return osd_fail(OSD_ERR_INVALID_ARG, "roi_pool_levels: null level %d", l);
    lv.x[l] = xs[l]; lv.h[l] = hs[l]; lv.w[l] = ws[l]; lv.scale[l] = scales[l];
  }
  if (dtype == OSD_F32)
    hipLaunchKernelGGL(roi_pool_levels_kernel<float>, dim3(n * max_rois), dim3(256), 0, OSD_STREAM(stream), lv, boxes, counts,
                       (float*)y, c, max_rois, pool, sampling_ratio, y_stride, level_out);
  else if (dtype == OSD_BF16)
    hipLaunchKernelGGL(roi_pool_levels_kernel<__bf16>, dim3(n * max_rois), dim3(256), 0, OSD_STREAM(stream), lv, boxes, counts,
                       (__bf16*)y, c, max_rois, pool, sampling_ratio, y_stride, level_out);
  else
    return osd_fail(OSD_ERR_INVALID_ARG, "bad dtype %d", dtype);
  return osd_check_launch("roi_pool_levels");
}

// the class sweep's pooling: sets_per_image ROI sets read one image's maps
extern "C" int osd_roi_pool_levels_sweep(int n_levels, const void* const* xs, const int32_t* hs, const int32_t* ws,
                                         const float* scales, const float* boxes, const int32_t* counts, void* y, int n_sets,
                                         int sets_per_image, int c, int max_rois, int pool, int sampling_ratio, int y_stride,
                                         int32_t* level_out, int dtype, void* stream) {
  if (n_levels < 1 || n_levels > OSD_MAX_ROI_LEVELS || !xs || !hs || !ws || !scales || !boxes || !y || n_sets < 0 || max_rois < 0)
    return osd_fail(OSD_ERR_INVALID_ARG, "roi_pool_levels_sweep: bad args");
  if (sets_per_image < 1 || n_sets % sets_per_image != 0)
    return osd_fail(OSD_ERR_INVALID_ARG, "roi_pool_levels_sweep: %d ROI sets are no multiple of %d sets per image", n_sets,
                    sets_per_image);
  const int e = dtype == OSD_BF16 ? 8 : 4;
  if (c % e != 0 || y_stride < c || y_stride % e != 0 || pool < 1)
    return osd_fail(OSD_ERR_INVALID_ARG, "roi_pool_levels_sweep: channels %d / stride %d must be multiples of %d", c, y_stride, e);
  if (dtype != OSD_F32 && dtype != OSD_BF16) return osd_fail(OSD_ERR_INVALID_ARG, "bad dtype %d", dtype);
  for (int l = 0; l < n_levels; ++l)
    if (!xs[l]) return osd_fail(OSD_ERR_INVALID_ARG, "roi_pool_levels_sweep: null level %d", l);
  if ((long long)n_sets * max_rois > 0x7fffffffLL) return osd_fail(OSD_ERR_INVALID_ARG, "roi_pool_levels_sweep: too many ROIs");
  if (n_sets * max_rois == 0) return OSD_OK;
  PoolLevels lv;
  lv.n_levels = n_levels;
  for (int l = 0; l < n_levels; ++l) { lv.x[l] = xs[l]; lv.h[l] = hs[l]; lv.w[l] = ws[l]; lv.scale[l] = scales[l]; }
  if (dtype == OSD_F32)
    hipLaunchKernelGGL(roi_pool_levels_sweep_kernel<float>, dim3(n_sets * max_rois), dim3(256), 0, OSD_STREAM(stream), lv, boxes,
                       counts, (float*)y, c, max_rois, pool, sampling_ratio, y_stride, level_out, sets_per_image);
  else
    hipLaunchKernelGGL(roi_pool_levels_sweep_kernel<__bf16>, dim3(n_sets * max_rois), dim3(256), 0, OSD_STREAM(stream), lv, boxes,
                       counts, (__bf16*)y, c, max_rois, pool, sampling_ratio, y_stride, level_out, sets_per_image);
  return osd_check_launch("roi_pool_levels_sweep");
}

extern "C" int osd_groupnorm_act_rois(const void* x, const void* addend, const float* gamma, const float* beta, void* y,
                                      int n_samples, int hw, int c, int groups, float eps, float slope, int rois_per_add,
                                      int add_stride, int add_offset, int dtype, void* stream) {
  if (!x || !gamma || !beta || !y) return osd_fail(OSD_ERR_INVALID_ARG, "groupnorm_act_rois: null argument");
  if (const int rc = gn_act_rois_shape("groupnorm_act_rois", hw, c, groups)) return rc;
  if (addend && rois_per_add < 1) return osd_fail(OSD_ERR_INVALID_ARG, "groupnorm_act_rois: rois_per_add");
  if (n_samples == 0) return OSD_OK;
  if (dtype == OSD_F32)
    hipLaunchKernelGGL((gn_act_rois_kernel<float, 49, false>), dim3(n_samples), dim3(c / 2), 0, OSD_STREAM(stream), (const float*)x,
                       (const float*)addend, gamma, beta, (float*)y, c, groups, eps, slope, rois_per_add, add_stride,
                       add_offset, (const int32_t*)nullptr, 0, 0);
  else if (dtype == OSD_BF16)
    hipLaunchKernelGGL((gn_act_rois_kernel<__bf16, 49, false>), dim3(n_samples), dim3(c / 2), 0, OSD_STREAM(stream),
                       (const __bf16*)x, (const __bf16*)addend, gamma, beta, (__bf16*)y, c, groups, eps, slope, rois_per_add,
                       add_stride, add_offset, (const int32_t*)nullptr, 0, 0);
  else
    return osd_fail(OSD_ERR_INVALID_ARG, "bad dtype %d", dtype);
  return osd_check_launch("groupnorm_act_rois");
}

extern "C" int osd_box_decode_opt(const void* pred, const float* rois, const int32_t* counts, float* scores, float* boxes,
                                  float* logits_out, float* reg_out, int n, int max_rois, int shots, int pred_stride,
                                  const float* reg_weights, float img_h, float img_w, const float* img_hw, float score_thresh,
                                  int dtype, int cls_loss, void* stream) {
  if (cls_loss != OSD_BOX_CLS_CE && cls_loss != OSD_BOX_CLS_FOCAL && cls_loss != OSD_BOX_CLS_MSE)
    return osd_fail(OSD_ERR_INVALID_ARG, "box_decode: cls_loss %d (OSD_BOX_CLS_CE / _FOCAL / _MSE)", cls_loss);
  const bool ce = cls_loss == OSD_BOX_CLS_CE;
  if (!pred || !rois || !scores || !boxes || !reg_weights || shots < 1 || pred_stride < (ce ? 10 : 9))
    return osd_fail(OSD_ERR_INVALID_ARG, "box_decode: bad args");
  if (n * max_rois == 0) return OSD_OK;
  const float clip = 4.135166556742356f;   // log(1000/16), box_coder.py:19
  // the softmax kernel and the sigmoid kernel share their argument list: one launch, templated on the kernel and its element type
  auto launch = [&](auto kernel, auto* p) {
    hipLaunchKernelGGL(kernel, dim3(grid_for((long long)n * max_rois, 256)), dim3(256), 0, OSD_STREAM(stream), p, rois, counts, scores,
                       boxes, logits_out, reg_out, n, max_rois, shots, pred_stride, reg_weights[0], reg_weights[1], reg_weights[2],
                       reg_weights[3], clip, img_h, img_w, score_thresh, img_hw);
  };
  if (dtype == OSD_F32)
    launch(ce ? box_decode_kernel<float> : box_decode_sigmoid_kernel<float>, (const float*)pred);
  else if (dtype == OSD_BF16)
    launch(ce ? box_decode_kernel<__bf16> : box_decode_sigmoid_kernel<__bf16>, (const __bf16*)pred);
  else
    return osd_fail(OSD_ERR_INVALID_ARG, "bad dtype %d", dtype);
  return osd_check_launch("box_decode");
}

extern "C" int osd_box_decode(const void* pred, const float* rois, const int32_t* counts, float* scores, float* boxes,
                              float* logits_out, float* reg_out, int n, int max_rois, int shots, int pred_stride,
                              const float* reg_weights, float img_h, float img_w, const float* img_hw, float score_thresh,
                              int dtype, void* stream) {
  return osd_box_decode_opt(pred, rois, counts, scores, boxes, logits_out, reg_out, n, max_rois, shots, pred_stride, reg_weights,
                            img_h, img_w, img_hw, score_thresh, dtype, OSD_BOX_CLS_CE, stream);
}
