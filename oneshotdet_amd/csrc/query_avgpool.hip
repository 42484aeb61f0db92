// Global-average query pooling (FEW_SHOT.SUPP_ROIALIGN False): nn.AdaptiveAvgPool2d((1, 1)) of every query feature map
// (generalized_rcnn.py:87-94, 302-303) followed by batch_pooling's mean over the shots of a target image (:100-104), and its
// backward.  A translation unit of its own: nothing here is shared with (or can change the code generation of) the ROIAlign
// pooling in elementwise.hip / backward.hip.
//
// Forward, two launches for all levels.  (1) One workgroup per (level, query map, pixel chunk) sums its chunk over 16-byte
// channel loads into an fp32 partial in the caller's workspace.  (2) One thread per (level, target image, 4 channels) sums a
// map's partials in chunk order, divides by h * w, and averages the maps of the shots.  The chunking depends on (h, w) alone,
// so every sum is taken in an order fixed by (h, w, shots): the result does not depend on the batch size, the stream or timing.
#include "osd_common.h"

#define OSD_STREAM(s) reinterpret_cast<hipStream_t>(s)
#define OSD_DISPATCH_DTYPE(dtype, CALL_F32, CALL_BF16)                            \
  do {                                                                           \
    if ((dtype) == OSD_F32) { CALL_F32; }                                        \
    else if ((dtype) == OSD_BF16) { CALL_BF16; }                                 \
    else return osd_fail(OSD_ERR_INVALID_ARG, "bad dtype %d", (int)(dtype));     \
  } while (0)

namespace {

constexpr int kAvgLevels = 8;
constexpr int kAvgThreads = 256;
constexpr int kAvgMinChunk = 64;     // pixels: the smallest chunk a map is cut into ...
constexpr int kAvgMaxChunks = 16;    // ... and at most this many chunks per map (52 x 52 -> 16 chunks of 169 pixels)
constexpr int kBwdPerThread = 4;     // 16-byte stores per thread of the backward

// chunks of a map of hw pixels, and pixels per chunk (the last may be shorter): a function of hw only
inline int avg_chunks(int hw) { const int n = (hw + kAvgMinChunk - 1) / kAvgMinChunk; return n < kAvgMaxChunks ? n : kAvgMaxChunks; }
inline int avg_chunk_px(int hw) { const int n = avg_chunks(hw); return (hw + n - 1) / n; }

struct AvgFwdLevels {
  const void* x[kAvgLevels];
  float* y[kAvgLevels];
  int hw[kAvgLevels];
  int chunks[kAvgLevels];
  int chunk_px[kAvgLevels];
  int block0[kAvgLevels + 1];       // first workgroup of each level in the partial-sum launch; block0[n_levels] = grid size
  long long part0[kAvgLevels];      // first float of each level's partials in the workspace
  int n_levels;
};

struct AvgBwdLevels {
  const float* dq[kAvgLevels];
  void* out[kAvgLevels];
  int hw[kAvgLevels];
  int block0[kAvgLevels + 1];
  int n_levels;
};

template <typename T> struct Vec16;
template <> struct Vec16<float> {
  static constexpr int N = 4;
  __device__ __forceinline__ static void add(const float* p, float* acc) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += t[e];
  }
  __device__ __forceinline__ static void store(float* p, const float* v) {
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  }
};
template <> struct Vec16<__bf16> {
  static constexpr int N = 8;
  __device__ __forceinline__ static void add(const __bf16* p, float* acc) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += (float)t[e];
  }
  __device__ __forceinline__ static void store(__bf16* p, const float* v) {
    bf16x8 t;
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = from_f32<__bf16>(v[e]);
    *reinterpret_cast<bf16x8*>(p) = t;
  }
};

// V fp32 values as 16-byte stores
template <int V> __device__ __forceinline__ void store_f32(float* p, const float* v) {
  Vec16<float>::store(p, v);
  if constexpr (V == 8) Vec16<float>::store(p + 4, v + 4);
}

__device__ __forceinline__ int level_of(const int* block0, int n_levels, int blk) {
  int l = 0;
  while (l + 1 < n_levels && blk >= block0[l + 1]) ++l;
  return l;
}

// (1) part[l][n][j][c] = sum of map n's pixels in chunk j.  The workgroup's threads are (pixel slot ps, 16-byte channel group g);
// slot ps sums pixels p0 + ps, p0 + ps + P, ... in order; the P slots are then added in slot order through LDS.
template <typename T>
__global__ void __launch_bounds__(kAvgThreads) query_avgpool_partial_kernel(AvgFwdLevels L, float* __restrict__ part, int c) {
  constexpr int V = Vec16<T>::N;
  __shared__ float red[kAvgThreads * V];
  const int lvl = level_of(L.block0, L.n_levels, blockIdx.x);
  const int rem = blockIdx.x - L.block0[lvl];
  const int nch = L.chunks[lvl], hw = L.hw[lvl];
  const int n = rem / nch, j = rem - n * nch;
  const int p0 = j * L.chunk_px[lvl];
  const int p1 = min(hw, p0 + L.chunk_px[lvl]);
  const int G = c / V;                                       // 16-byte channel groups per pixel
  const int P = G >= kAvgThreads ? 1 : kAvgThreads / G;      // pixel slots
  const int GW = G >= kAvgThreads ? kAvgThreads : G;         // channel groups per pass
  const T* x = reinterpret_cast<const T*>(L.x[lvl]) + (size_t)n * hw * c;
  float* out = part + L.part0[lvl] + ((size_t)n * nch + j) * c;
  const int t = threadIdx.x;
  for (int g0 = 0; g0 < G; g0 += GW) {
    const int g = g0 + t % GW, ps = t / GW;
    const bool active = ps < P && g < G;
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    if (active) {
      const T* src = x + (size_t)g * V;
#pragma unroll 4
      for (int p = p0 + ps; p < p1; p += P) Vec16<T>::add(src + (size_t)p * c, acc);
    }
    if (P == 1) {          // (uniform) one slot: no reduction
      if (active) store_f32<V>(out + g * V, acc);
      continue;
    }
    // P > 1 means G < kAvgThreads: this is the only pass
    if (active) {
#pragma unroll
      for (int e = 0; e < V; ++e) red[(ps * G + g) * V + e] = acc[e];
    }
    __syncthreads();
    if (t < G) {
      float s[V];
#pragma unroll
      for (int e = 0; e < V; ++e) s[e] = red[t * V + e];
      for (int q = 1; q < P; ++q) {
#pragma unroll
        for (int e = 0; e < V; ++e) s[e] += red[(q * G + t) * V + e];
      }
      store_f32<V>(out + t * V, s);
    }
  }
}

// (2) y[l][b][c] = (sum_k (sum_j part[l][b * shots + k][j][c]) / (h * w)) / shots
__global__ void __launch_bounds__(kAvgThreads) query_avgpool_finalize_kernel(AvgFwdLevels L, const float* __restrict__ part, int batch,
                                                                              int shots, int c) {
  const int c4 = c / 4;
  const int per_level = batch * c4;
  const int i = blockIdx.x * kAvgThreads + threadIdx.x;
  if (i >= per_level * L.n_levels) return;
  const int lvl = i / per_level, r = i - lvl * per_level;
  const int b = r / c4, ch = (r - b * c4) * 4;
  const int nch = L.chunks[lvl];
  const float area = (float)L.hw[lvl];
  float s[4] = {0.f, 0.f, 0.f, 0.f};
  for (int k = 0; k < shots; ++k) {
    const float* src = part + L.part0[lvl] + (size_t)(b * shots + k) * nch * c + ch;
    float m[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int j = 0; j < nch; ++j) Vec16<float>::add(src + (size_t)j * c, m);
#pragma unroll
    for (int e = 0; e < 4; ++e) s[e] += m[e] / area;
  }
  const float fs = (float)shots;
  const float y[4] = {s[0] / fs, s[1] / fs, s[2] / fs, s[3] / fs};
  Vec16<float>::store(L.y[lvl] + (size_t)b * c + ch, y);
}

// outs[l][n][p][c] = dqs[l][n / shots][c] / (h * w) / shots: a write-only stream of 16-byte stores
template <typename T>
__global__ void __launch_bounds__(kAvgThreads) query_avgpool_bwd_kernel(AvgBwdLevels L, int maps, int shots, int c) {
  constexpr int V = Vec16<T>::N;
  const int lvl = level_of(L.block0, L.n_levels, blockIdx.x);
  const int hw = L.hw[lvl];
  const int G = c / V;
  const int per_map = hw * G;
  const int nvec = maps * per_map;
  const float area = (float)hw, fs = (float)shots;
  const float* dq = L.dq[lvl];
  T* out = reinterpret_cast<T*>(L.out[lvl]);
  const int v0 = (blockIdx.x - L.block0[lvl]) * (kAvgThreads * kBwdPerThread) + threadIdx.x;
#pragma unroll
  for (int it = 0; it < kBwdPerThread; ++it) {
    const int v = v0 + it * kAvgThreads;
    if (v >= nvec) break;
    const int n = v / per_map;
    const int g = v % G;
    const float* src = dq + (size_t)(n / shots) * c + g * V;
    float d[V];
#pragma unroll
    for (int e = 0; e < V; ++e) d[e] = 0.f;
    Vec16<float>::add(src, d);
    if constexpr (V == 8) Vec16<float>::add(src + 4, d + 4);
#pragma unroll
    for (int e = 0; e < V; ++e) d[e] = d[e] / area / fs;
    Vec16<T>::store(out + (size_t)v * V, d);
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// shared argument checks of the three entry points; fills the per-level tables of the forward
int avg_levels_setup(const char* what, int n_levels, const int32_t* hs, const int32_t* ws, int maps, int c, AvgFwdLevels* L,
                     long long* part_floats) {
  if (n_levels < 1 || n_levels > kAvgLevels || !hs || !ws || maps < 0 || c < 1)
    return osd_fail(OSD_ERR_INVALID_ARG, "%s: bad arguments", what);
  if (c % 8 != 0) return osd_fail(OSD_ERR_UNSUPPORTED, "%s: c = %d is not a multiple of 8", what, c);
  long long floats = 0, blocks = 0;
  for (int l = 0; l < n_levels; ++l) {
    if (hs[l] < 1 || ws[l] < 1) return osd_fail(OSD_ERR_INVALID_ARG, "%s: bad level %d (%d x %d)", what, l, hs[l], ws[l]);
    const long long hw = (long long)hs[l] * ws[l];
    if (hw * c * (long long)maps >= (1LL << 31))
      return osd_fail(OSD_ERR_UNSUPPORTED, "%s: level %d has %lld elements (at most 2^31 - 1)", what, l, hw * c * maps);
    const int nch = avg_chunks((int)hw);
    if (L) {
      L->hw[l] = (int)hw;
      L->chunks[l] = nch;
      L->chunk_px[l] = avg_chunk_px((int)hw);
      L->block0[l] = (int)blocks;
      L->part0[l] = floats;
    }
    blocks += (long long)maps * nch;
    floats += (long long)maps * nch * c;
  }
  if (blocks >= (1LL << 31)) return osd_fail(OSD_ERR_UNSUPPORTED, "%s: too many maps", what);
  if (L) {
    L->block0[n_levels] = (int)blocks;
    L->n_levels = n_levels;
  }
  if (part_floats) *part_floats = floats;
  return OSD_OK;
}

}  // namespace

extern "C" int64_t osd_query_avgpool_workspace_bytes(int n_levels, const int32_t* hs, const int32_t* ws, int maps, int c) {
  long long floats = 0;
  const int rc = avg_levels_setup("query_avgpool_workspace_bytes", n_levels, hs, ws, maps, c, nullptr, &floats);
  return rc != OSD_OK ? (int64_t)rc : (int64_t)floats * (int64_t)sizeof(float);
}

extern "C" int osd_query_avgpool_levels(int n_levels, const void* const* xs, const int32_t* hs, const int32_t* ws, int batch,
                                        int shots, int c, float* const* ys, float* workspace, int64_t workspace_bytes, int dtype,
                                        void* stream) {
  if (!xs || !ys || batch < 0 || shots < 1) return osd_fail(OSD_ERR_INVALID_ARG, "query_avgpool_levels: bad arguments");
  if (dtype != OSD_F32 && dtype != OSD_BF16) return osd_fail(OSD_ERR_INVALID_ARG, "query_avgpool_levels: bad dtype %d", dtype);
  if ((long long)batch * shots >= (1LL << 31)) return osd_fail(OSD_ERR_UNSUPPORTED, "query_avgpool_levels: batch too large");
  AvgFwdLevels L;
  long long floats = 0;
  int rc = avg_levels_setup("query_avgpool_levels", n_levels, hs, ws, batch * shots, c, &L, &floats);
  if (rc != OSD_OK) return rc;
  for (int l = 0; l < n_levels; ++l) {
    if (!xs[l] || !ys[l]) return osd_fail(OSD_ERR_INVALID_ARG, "query_avgpool_levels: null pointer at level %d", l);
    if (!aligned16(xs[l]) || !aligned16(ys[l]))
      return osd_fail(OSD_ERR_UNSUPPORTED, "query_avgpool_levels: level %d is not 16-byte aligned", l);
    L.x[l] = xs[l];
    L.y[l] = ys[l];
  }
  if (batch == 0) return OSD_OK;
  if (!workspace || workspace_bytes < floats * (long long)sizeof(float))
    return osd_fail(OSD_ERR_WORKSPACE, "query_avgpool_levels: the workspace needs %lld bytes, got %lld", floats * (long long)sizeof(float),
                    (long long)workspace_bytes);
  if (!aligned16(workspace)) return osd_fail(OSD_ERR_UNSUPPORTED, "query_avgpool_levels: workspace is not 16-byte aligned");
  const long long threads = (long long)n_levels * batch * (c / 4);
  if (threads >= (1LL << 31)) return osd_fail(OSD_ERR_UNSUPPORTED, "query_avgpool_levels: batch too large");
  const int blocks = L.block0[n_levels];
  OSD_DISPATCH_DTYPE(dtype,
      hipLaunchKernelGGL(query_avgpool_partial_kernel<float>, dim3(blocks), dim3(kAvgThreads), 0, OSD_STREAM(stream), L, workspace, c),
      hipLaunchKernelGGL(query_avgpool_partial_kernel<__bf16>, dim3(blocks), dim3(kAvgThreads), 0, OSD_STREAM(stream), L, workspace, c));
  rc = osd_check_launch("query_avgpool_partial");
  if (rc != OSD_OK) return rc;
  hipLaunchKernelGGL(query_avgpool_finalize_kernel, dim3(cdiv((int)threads, kAvgThreads)), dim3(kAvgThreads), 0, OSD_STREAM(stream), L,
                     workspace, batch, shots, c);
  return osd_check_launch("query_avgpool_finalize");
}

extern "C" int osd_query_avgpool_levels_bwd(int n_levels, const float* const* dqs, const int32_t* hs, const int32_t* ws, int batch,
                                            int shots, int c, void* const* outs, int dtype, void* stream) {
  if (!dqs || !outs || batch < 0 || shots < 1) return osd_fail(OSD_ERR_INVALID_ARG, "query_avgpool_levels_bwd: bad arguments");
  if (dtype != OSD_F32 && dtype != OSD_BF16) return osd_fail(OSD_ERR_INVALID_ARG, "query_avgpool_levels_bwd: bad dtype %d", dtype);
  if ((long long)batch * shots >= (1LL << 31)) return osd_fail(OSD_ERR_UNSUPPORTED, "query_avgpool_levels_bwd: batch too large");
  const int maps = batch * shots;
  int rc = avg_levels_setup("query_avgpool_levels_bwd", n_levels, hs, ws, maps, c, nullptr, nullptr);
  if (rc != OSD_OK) return rc;
  const int V = dtype == OSD_BF16 ? 8 : 4;
  AvgBwdLevels L;
  long long blocks = 0;
  for (int l = 0; l < n_levels; ++l) {
    if (!dqs[l] || !outs[l]) return osd_fail(OSD_ERR_INVALID_ARG, "query_avgpool_levels_bwd: null pointer at level %d", l);
    if (!aligned16(dqs[l]) || !aligned16(outs[l]))
      return osd_fail(OSD_ERR_UNSUPPORTED, "query_avgpool_levels_bwd: level %d is not 16-byte aligned", l);
    L.dq[l] = dqs[l];
    L.out[l] = outs[l];
    L.hw[l] = hs[l] * ws[l];
    L.block0[l] = (int)blocks;
    const long long nvec = (long long)maps * L.hw[l] * (c / V);
    blocks += (nvec + kAvgThreads * kBwdPerThread - 1) / (kAvgThreads * kBwdPerThread);
  }
  if (blocks >= (1LL << 31)) return osd_fail(OSD_ERR_UNSUPPORTED, "query_avgpool_levels_bwd: too many maps");
  L.block0[n_levels] = (int)blocks;
  L.n_levels = n_levels;
  if (batch == 0) return OSD_OK;
  OSD_DISPATCH_DTYPE(dtype,
      hipLaunchKernelGGL(query_avgpool_bwd_kernel<float>, dim3((int)blocks), dim3(kAvgThreads), 0, OSD_STREAM(stream), L, maps, shots, c),
      hipLaunchKernelGGL(query_avgpool_bwd_kernel<__bf16>, dim3((int)blocks), dim3(kAvgThreads), 0, OSD_STREAM(stream), L, maps, shots, c));
  return osd_check_launch("query_avgpool_levels_bwd");
}
