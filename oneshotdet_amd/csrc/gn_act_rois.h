// GroupNorm + LeakyReLU over [R][7][7][C] ROI maps with an optional addend map, shared by its two entries: osd_groupnorm_act_rois
// (box_head.hip: the addend row of a sample follows from its number) and osd_groupnorm_act_rois_gallery (gallery.hip: it goes through
// an index table).  ONE kernel templated on the indexing; the plain instantiation has no table and no branch on one.
#ifndef OSD_GN_ACT_ROIS_H
#define OSD_GN_ACT_ROIS_H

#include "osd_common.h"

namespace {

// two adjacent channels (even index) as one 4- / 8-byte access
__device__ __forceinline__ void load2(const float* p, float& a, float& b) {
  const f32x2 t = *reinterpret_cast<const f32x2*>(p);
  a = t[0]; b = t[1];
}
__device__ __forceinline__ void load2(const __bf16* p, float& a, float& b) {
  const uint32_t u = *reinterpret_cast<const uint32_t*>(p);
  a = __uint_as_float(u << 16);
  b = __uint_as_float(u & 0xffff0000u);
}
__device__ __forceinline__ void store2(float* p, float a, float b) {
  f32x2 t = {a, b};
  *reinterpret_cast<f32x2*>(p) = t;
}
__device__ __forceinline__ void store2(__bf16* p, float a, float b) {
  typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
  bf16x2 t = {(__bf16)a, (__bf16)b};
  *reinterpret_cast<bf16x2*>(p) = t;
}

// v += the thread's two channels of every pixel of one addend map
template <typename T, int HW>
__device__ __forceinline__ void gn_add_map(const T* __restrict__ as, int c, float (&v0)[HW], float (&v1)[HW]) {
#pragma unroll
  for (int p = 0; p < HW; ++p) {
    float a0, a1;
    load2(as + (size_t)p * c, a0, a1);
    v0[p] += a0;
    v1[p] += a1;
  }
}

// GroupNorm(groups, C) + LeakyReLU(slope) of one ROI map [hw][C] per workgroup (hw = 49): the whole sample sits in
// registers, so mean and the centred second moment are two exact passes over registers and HBM is read once.
// Thread t owns channels (2t, 2t+1) of every pixel; a group's channels are CPG/2 adjacent lanes.  `addend` (optional):
// [n_add][hw][C], row of this sample = sample / rois_per_add * add_stride + add_offset — the query half of the
// concatenated 1x1 conv (box_head.py:146-148), which is the same for every ROI of an image, added before the statistics.
// INDEXED: the row is add_index[sample / rois_per_add] * add_stride + add_offset instead (one table entry per ROI set: the same in
// every lane of the workgroup); a row outside [0, n_add) is never used as an address (row 0 is read in its place) and the sample's output is NaN.
// INDEXED launches are a 2-D grid (ROI within its set, set), so the set, and with it the table entry, follows from the workgroup's id
// without a division and is fetched first: its latency passes under the 49 loads of x.
// (The plain launches pass no table: add_index = null, n_add = 0, n_samples = 0, all unread.)
template <typename T, int HW, bool INDEXED>
__global__ __launch_bounds__(256) void gn_act_rois_kernel(const T* __restrict__ x, const T* __restrict__ addend,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta,
                                                          T* __restrict__ y, int c, int groups, float eps, float slope,
                                                          int rois_per_add, int add_stride, int add_offset,
                                                          const int32_t* __restrict__ add_index, int n_add, int n_samples) {
  int sample = blockIdx.x;
  // INDEXED: never an address outside the addend (row 0 stands in for a row that is)
  bool inside = true;
  size_t arow = 0;
  if constexpr (INDEXED) {
    const int idx = add_index[blockIdx.y];
    sample += blockIdx.y * rois_per_add;
    if (sample >= n_samples) return;            // the last set may be short
    const long long r = (long long)idx * add_stride + add_offset;
    inside = idx >= 0 && r >= 0 && r < (long long)n_add;               // workgroup-uniform
    arow = inside ? (size_t)r : 0;
  }
  const int t = threadIdx.x;                 // blockDim.x == c / 2
  const int cpg = c / groups;                // channels per group (even)
  const int lanes = cpg / 2;                 // lanes per group: power of two <= 64
  const T* xs = x + (size_t)sample * HW * c + 2 * t;
  float v0[HW], v1[HW];
#pragma unroll
  for (int p = 0; p < HW; ++p) load2(xs + (size_t)p * c, v0[p], v1[p]);
  if constexpr (INDEXED) {
    gn_add_map<T, HW>(addend + arow * HW * c + 2 * t, c, v0, v1);
  } else if (addend) {
    gn_add_map<T, HW>(addend + ((size_t)(sample / rois_per_add) * add_stride + add_offset) * HW * c + 2 * t, c, v0, v1);
  }
  float s = 0.f;
#pragma unroll
  for (int p = 0; p < HW; ++p) s += v0[p] + v1[p];
  for (int m = 1; m < lanes; m <<= 1) s += __shfl_xor(s, m);
  const float inv_n = 1.f / (float)(HW * cpg);
  const float mean = s * inv_n;
  float q = 0.f;
#pragma unroll
  for (int p = 0; p < HW; ++p) {
    const float d0 = v0[p] - mean, d1 = v1[p] - mean;
    q += d0 * d0 + d1 * d1;
  }
  for (int m = 1; m < lanes; m <<= 1) q += __shfl_xor(q, m);
  float rstd = rsqrtf(q * inv_n + eps);
  if constexpr (INDEXED) rstd = inside ? rstd : __builtin_nanf("");      // a row outside the addend: the whole sample is NaN
  const float a0 = gamma[2 * t] * rstd, a1 = gamma[2 * t + 1] * rstd;
  const float b0 = beta[2 * t] - mean * a0, b1 = beta[2 * t + 1] - mean * a1;
  T* ys = y + (size_t)sample * HW * c + 2 * t;
#pragma unroll
  for (int p = 0; p < HW; ++p) {
    float o0 = fmaf(v0[p], a0, b0), o1 = fmaf(v1[p], a1, b1);
    o0 = o0 >= 0.f ? o0 : o0 * slope;
    o1 = o1 >= 0.f ? o1 : o1 * slope;
    store2(ys + (size_t)p * c, o0, o1);
  }
}

// the shape rule both entries share: 7x7 maps, a power-of-two number (<= 64) of lanes per group, whole waves
inline int gn_act_rois_shape(const char* what, int hw, int c, int groups) {
  if (hw != 49) return osd_fail(OSD_ERR_UNSUPPORTED, "%s: hw %d (only 7x7 ROI maps)", what, hw);
  const int cpg = groups > 0 ? c / groups : 0;
  const int lanes = cpg / 2;
  if (groups < 1 || c % groups != 0 || cpg % 2 != 0 || lanes < 1 || lanes > 64 || (lanes & (lanes - 1)) != 0 || c > 512 ||
      (c / 2) % 64 != 0)
    return osd_fail(OSD_ERR_UNSUPPORTED, "%s: c %d groups %d", what, c, groups);
  return OSD_OK;
}

}  // namespace

#endif /* OSD_GN_ACT_ROIS_H */
