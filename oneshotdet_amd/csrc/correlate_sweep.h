// The class sweep's correlation walk, shared by its two entries: osd_correlate_levels_sweep (class_sweep.hip: the staged query vectors
// are the rows b*K + k of qs) and osd_correlate_levels_gallery (gallery.hip: they are rows of a gallery, picked through a slot table).
// The two differ in how a workgroup fills its LDS and in nothing else, so the walk is ONE kernel templated on the staging; the sweep's
// instantiation has no slot table, no gallery size and no branch on either: it compiles to what it compiled to as a kernel of its own.
#ifndef OSD_CORRELATE_SWEEP_H
#define OSD_CORRELATE_SWEEP_H

#include "osd_common.h"

namespace {

constexpr int kGroup = OSD_CLASS_SWEEP_GROUP;
// G = 8: a thread keeps its channel chunk of all G vectors in registers (G * 8 fp32 = 64 VGPRs for bf16; the kernel compiles to
// 136 VGPRs = 3 waves per SIMD for bf16, 98 = 4 for fp32, no scratch), and a workgroup stages G * 4c bytes = 8 KiB of LDS at
// c = 256, a twentieth of a CU's 160 KiB, so LDS never limits the occupancy.  A larger G buys little: the traffic at K = 20 is 23 maps at G = 8, 22 at G = 10 and 21 at G = 20, against 40.
constexpr int kSweepLevels = 6;
constexpr int kSweepMaxC = 2048;      // G * 4c <= 64 KiB of LDS

template <typename T> struct Chunk;
template <> struct Chunk<float> {
  static constexpr int N = 4;
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
  static constexpr int N = 8;
  float v[8];
  __device__ __forceinline__ void load(const __bf16* p) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (float)t[i];
  }
  __device__ __forceinline__ void store(__bf16* p) const {
    bf16x8 t;
#pragma unroll
    for (int i = 0; i < 8; ++i) t[i] = (__bf16)v[i];
    *reinterpret_cast<bf16x8*>(p) = t;
  }
};

struct SweepLevels {
  const void* x[kSweepLevels];
  const float* q[kSweepLevels];
  void* y[kSweepLevels];
  int hw[kSweepLevels];
  int bx[kSweepLevels];        // slabs per (image, group) at this level
  int begin[kSweepLevels];     // first workgroup of this level
  int n_levels;
};

// the products of one loaded chunk with the kg staged vectors: v * q in fp32, then the store conversion (correlate_levels_kernel's
// `v *= q; store`), one 16-byte store per category slot
template <typename T>
__device__ __forceinline__ void sweep_store(const Chunk<T>& v, const float (&qv)[kGroup][Chunk<T>::N], int kg, T* y0, size_t row,
                                            long long off) {
  constexpr int E = Chunk<T>::N;
#pragma unroll
  for (int g = 0; g < kGroup; ++g) {
    if (g < kg) {       // wave-uniform
      Chunk<T> o;
#pragma unroll
      for (int e = 0; e < E; ++e) o.v[e] = v.v[e] * qv[g][e];
      o.store(y0 + g * row + off);
    }
  }
}

// A workgroup = (level, image, slab, group of up to kGroup category slots); the groups of one slab are adjacent workgroups, so the
// ceil(K/G) reads of a slab come close together in time.  Level table and slab walk as correlate_levels_kernel (elementwise.hip).
// SLOTS = false: the staged vector of output row r = img*classes + k is q[r].  SLOTS = true: it is q[slots[r]], a row of a gallery of
// n_gallery vectors; a slot outside [0, n_gallery) stages NaNs instead of loading (its output row is NaN), so no table, however
// wrong, makes the kernel read outside the gallery.  The slot is one value per staged vector: loaded and checked wave-uniformly.
// (The sweep's launches pass no table: slots = null, n_gallery = 0, both unread.)
template <typename T, bool SLOTS>
__global__ void __launch_bounds__(256) correlate_sweep_kernel(SweepLevels L, int c, int classes, int groups,
                                                              const int32_t* __restrict__ slots, int n_gallery) {
  constexpr int E = Chunk<T>::N;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* qs = reinterpret_cast<float*>(smem);
  const int b = blockIdx.x;
  int lvl = 0;
#pragma unroll
  for (int i = 1; i < kSweepLevels; ++i)
    if (i < L.n_levels && b >= L.begin[i]) lvl = i;
  const void* xv = L.x[0]; const float* q = L.q[0]; void* yv = L.y[0];
  int hw = L.hw[0], bx = L.bx[0], beg = L.begin[0];
#pragma unroll
  for (int i = 1; i < kSweepLevels; ++i)
    if (lvl == i) { xv = L.x[i]; q = L.q[i]; yv = L.y[i]; hw = L.hw[i]; bx = L.bx[i]; beg = L.begin[i]; }
  const int local = b - beg;
  const int grp = local % groups, rest = local / groups;
  const int img = rest / bx, slab = rest - img * bx;
  const int k0 = grp * kGroup;
  const int kg = min(kGroup, classes - k0);          // >= 1: groups = ceil(classes / kGroup)
  const size_t row0 = (size_t)img * classes + k0;    // first output row (and query row / slot table row) of this group
  if constexpr (SLOTS) {
    for (int g = 0; g < kg; ++g) {
      const int slot = slots[row0 + g];                                   // the same address in every lane
      const bool inside = (unsigned)slot < (unsigned)n_gallery;
      const float* qg = q + (size_t)(inside ? slot : 0) * c;
      for (int i = threadIdx.x; i < c; i += blockDim.x) qs[g * c + i] = inside ? qg[i] : __builtin_nanf("");
    }
  } else {
    for (int i = threadIdx.x; i < kg * c; i += blockDim.x) qs[i] = q[row0 * c + i];
  }
  __syncthreads();
  const int cch = c / E;
  const long long total = (long long)hw * cch;
  const size_t row = (size_t)hw * c;                 // elements per map
  const T* xi = reinterpret_cast<const T*>(xv) + (size_t)img * row;
  T* y0 = reinterpret_cast<T*>(yv) + row0 * row;
  const long long stride = (long long)bx * blockDim.x;
  long long i = slab * (long long)blockDim.x + threadIdx.x;
  // the host makes bx * 256 a multiple of the chunks per pixel: a thread's channel chunk is loop invariant
  const int cc = (int)(i % cch);
  float qv[kGroup][E];
#pragma unroll
  for (int g = 0; g < kGroup; ++g)
#pragma unroll
    for (int e = 0; e < E; ++e) qv[g][e] = g < kg ? qs[g * c + cc * E + e] : 0.f;
  for (; i + stride < total; i += 2 * stride) {
    Chunk<T> v0, v1;
    v0.load(xi + i * E);
    v1.load(xi + (i + stride) * E);
    sweep_store<T>(v0, qv, kg, y0, row, i * E);
    sweep_store<T>(v1, qv, kg, y0, row, (i + stride) * E);
  }
  if (i < total) {
    Chunk<T> v;
    v.load(xi + i * E);
    sweep_store<T>(v, qv, kg, y0, row, i * E);
  }
}

// The argument rules and the level table both entries share (`what` names the entry in the error text).  -> OSD_OK with *blocks_out
// workgroups to launch (0: nothing to do), or the error.
inline int correlate_sweep_plan(const char* what, int n_levels, const void* const* xs, const float* const* qs, void* const* ys,
                                const int32_t* hws, int n, int classes, int c, int dtype, SweepLevels* L, long long* blocks_out) {
  *blocks_out = 0;
  if (n_levels < 1 || n_levels > kSweepLevels || !xs || !qs || !ys || !hws)
    return osd_fail(OSD_ERR_INVALID_ARG, "%s: 1..%d levels, no null array", what, kSweepLevels);
  if (n < 0 || classes < 1) return osd_fail(OSD_ERR_INVALID_ARG, "%s: n %d, classes %d", what, n, classes);
  if (dtype != OSD_F32 && dtype != OSD_BF16) return osd_fail(OSD_ERR_INVALID_ARG, "%s: bad dtype", what);
  const int e = dtype == OSD_BF16 ? 8 : 4;
  if (c < e || c % e != 0 || c > kSweepMaxC || 256 % (c / e) != 0)
    return osd_fail(OSD_ERR_INVALID_ARG, "%s: bad channel count %d", what, c);
  if (n == 0) return OSD_OK;
  const int groups = (classes + kGroup - 1) / kGroup;
  L->n_levels = 0;
  long long blocks = 0;
  for (int i = 0; i < n_levels; ++i) {
    if (hws[i] <= 0) continue;
    if (!xs[i] || !qs[i] || !ys[i]) return osd_fail(OSD_ERR_INVALID_ARG, "%s: null tensor at level %d", what, i);
    const long long chunks = (long long)hws[i] * (c / e);
    int bx = (int)((chunks + 256LL * 8 - 1) / (256LL * 8));     // as correlate_levels: >= 8 loaded chunks per thread on a large level
    if (bx < 1) bx = 1;
    if (bx > 1024) bx = 1024;
    const int k = L->n_levels++;
    L->x[k] = xs[i]; L->q[k] = qs[i]; L->y[k] = ys[i]; L->hw[k] = hws[i]; L->bx[k] = bx; L->begin[k] = (int)blocks;
    blocks += (long long)bx * n * groups;
    if (blocks > 0x7fffffffLL) return osd_fail(OSD_ERR_INVALID_ARG, "%s: grid too large", what);
  }
  if (L->n_levels == 0) return OSD_OK;
  for (int k = L->n_levels; k < kSweepLevels; ++k) { L->x[k] = L->x[0]; L->q[k] = L->q[0]; L->y[k] = L->y[0]; L->hw[k] = 0; L->bx[k] = 1; L->begin[k] = 0x7fffffff; }
  *blocks_out = blocks;
  return OSD_OK;
}

}  // namespace

#endif /* OSD_CORRELATE_SWEEP_H */
