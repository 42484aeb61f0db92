// Query augmentation groups (FEW_SHOT.SUPP_AUG, SUPP_AUG_METHOD 'avg' / 'max'): the query pyramid arrives as groups of
// A = NUM_SUPP_AUG + 1 consecutive maps (a support crop and its augmentations, feat.split(A, dim=0)) and every group is merged
// into one map before any pooling (generalized_rcnn.py:280-288), and the backward of that merge.  A translation unit of its own,
// modelled on query_avgpool.hip: the levels travel in a by-value struct, level_of() dispatches workgroups to levels, every load and
// store is 16 bytes wide.  One launch per direction for all levels; plain vector loads and stores only (no atomics, no workspace,
// no memset): every output element is written exactly once by the thread that owns it, so the result depends on nothing but the
// inputs.
#include "osd_common.h"
#include "../../include/oneshotdet_hip_supp_aug.h"

#define OSD_STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int kAugLevels = 8;
constexpr int kAugMax = 8;           // members of a group at most
constexpr int kAugThreads = 256;
constexpr int kAugPerThread = 4;     // 16-byte output vectors per thread (of the merged map: a thread reads / writes A times as many)

struct AugLevels {
  const void* x[kAugLevels];        // [groups * aug, hw, c]
  const void* dy[kAugLevels];       // backward only: [groups, hw, c]
  void* out[kAugLevels];            // forward: y [groups, hw, c]; backward: dx [groups * aug, hw, c]
  int per_map[kAugLevels];          // 16-byte vectors of one map: hw * (c / V)
  int block0[kAugLevels + 1];       // first workgroup of each level; block0[n_levels] = grid size
  int n_levels;
};

template <typename T> struct Vec16;
template <> struct Vec16<float> {
  static constexpr int N = 4;
  __device__ __forceinline__ static void load(const float* p, float* v) {
    const f32x4 t = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = t[e];
  }
  __device__ __forceinline__ static void store(float* p, const float* v) {
    *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
  }
};
template <> struct Vec16<__bf16> {
  static constexpr int N = 8;
  __device__ __forceinline__ static void load(const __bf16* p, float* v) {
    const bf16x8 t = *reinterpret_cast<const bf16x8*>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (float)t[e];
  }
  __device__ __forceinline__ static void store(__bf16* p, const float* v) {
    bf16x8 t;
#pragma unroll
    for (int e = 0; e < 8; ++e) t[e] = from_f32<__bf16>(v[e]);
    *reinterpret_cast<bf16x8*>(p) = t;
  }
};

__device__ __forceinline__ int level_of(const int* block0, int n_levels, int blk) {
  int l = 0;
  while (l + 1 < n_levels && blk >= block0[l + 1]) ++l;
  return l;
}

// y[l][g][p][c] = mean / max over a of x[l][g * aug + a][p][c].  avg: the members are added in member order in fp32, the sum is
// divided by aug (a true division) and rounded once to T.  max: exact in either dtype (a bf16 is a float).
template <typename T, int METHOD>
__global__ void __launch_bounds__(kAugThreads) supp_aug_reduce_kernel(AugLevels L, int groups, int aug) {
  constexpr int V = Vec16<T>::N;
  const int lvl = level_of(L.block0, L.n_levels, blockIdx.x);
  const int per = L.per_map[lvl];
  const int nvec = groups * per;
  const float fa = (float)aug;
  const T* x = reinterpret_cast<const T*>(L.x[lvl]);
  T* y = reinterpret_cast<T*>(L.out[lvl]);
  const int v0 = (blockIdx.x - L.block0[lvl]) * (kAugThreads * kAugPerThread) + threadIdx.x;
#pragma unroll
  for (int it = 0; it < kAugPerThread; ++it) {
    const int v = v0 + it * kAugThreads;
    if (v >= nvec) break;
    const int g = v / per, r = v - g * per;
    const T* src = x + ((size_t)g * aug * per + r) * V;
    float acc[V], m[V];
    Vec16<T>::load(src, acc);
    for (int a = 1; a < aug; ++a) {
      Vec16<T>::load(src + (size_t)a * per * V, m);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        if constexpr (METHOD == OSD_SUPP_AUG_AVG) acc[e] += m[e];
        else acc[e] = m[e] > acc[e] ? m[e] : acc[e];
      }
    }
    if constexpr (METHOD == OSD_SUPP_AUG_AVG) {
#pragma unroll
      for (int e = 0; e < V; ++e) acc[e] = acc[e] / fa;
    }
    Vec16<T>::store(y + (size_t)v * V, acc);
  }
}

// dx[l][g * aug + a][p][c]: avg, dy / aug for every member; max, the whole dy for the LOWEST member index that attains the maximum
// of the saved x and 0 for the others (torch.max(dim=1)'s backward on the CPU).  Every element of dx is written, once.
template <typename T, int METHOD>
__global__ void __launch_bounds__(kAugThreads) supp_aug_reduce_bwd_kernel(AugLevels L, int groups, int aug) {
  constexpr int V = Vec16<T>::N;
  const int lvl = level_of(L.block0, L.n_levels, blockIdx.x);
  const int per = L.per_map[lvl];
  const int nvec = groups * per;
  const float fa = (float)aug;
  const T* x = reinterpret_cast<const T*>(L.x[lvl]);
  const T* dy = reinterpret_cast<const T*>(L.dy[lvl]);
  T* dx = reinterpret_cast<T*>(L.out[lvl]);
  const int v0 = (blockIdx.x - L.block0[lvl]) * (kAugThreads * kAugPerThread) + threadIdx.x;
#pragma unroll
  for (int it = 0; it < kAugPerThread; ++it) {
    const int v = v0 + it * kAugThreads;
    if (v >= nvec) break;
    const int g = v / per, r = v - g * per;
    const size_t first = ((size_t)g * aug * per + r) * V;      // member 0's vector; member a's is a * per * V further on
    float d[V], o[V];
    Vec16<T>::load(dy + (size_t)v * V, d);
    if constexpr (METHOD == OSD_SUPP_AUG_AVG) {
#pragma unroll
      for (int e = 0; e < V; ++e) o[e] = d[e] / fa;
      for (int a = 0; a < aug; ++a) Vec16<T>::store(dx + first + (size_t)a * per * V, o);
    } else {
      float best[V], m[V];
      int arg[V];
      Vec16<T>::load(x + first, best);
#pragma unroll
      for (int e = 0; e < V; ++e) arg[e] = 0;
      for (int a = 1; a < aug; ++a) {
        Vec16<T>::load(x + first + (size_t)a * per * V, m);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          if (m[e] > best[e]) {      // strictly greater: a tie stays with the lower index
            best[e] = m[e];
            arg[e] = a;
          }
        }
      }
      for (int a = 0; a < aug; ++a) {
#pragma unroll
        for (int e = 0; e < V; ++e) o[e] = arg[e] == a ? d[e] : 0.f;
        Vec16<T>::store(dx + first + (size_t)a * per * V, o);
      }
    }
  }
}

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// the argument checks of both entry points, in the order the header documents; fills L (dy only when dys is given)
int aug_setup(const char* what, int n_levels, const void* const* xs, const void* const* dys, void* const* outs, const int32_t* hw,
              int groups, int aug, int c, int dtype, int method, AugLevels* L) {
  if (!xs || !outs || !hw) return osd_fail(OSD_ERR_INVALID_ARG, "%s: null pointer", what);
  if (aug < 2 || aug > kAugMax) return osd_fail(OSD_ERR_INVALID_ARG, "%s: aug = %d (2 .. %d members per group)", what, aug, kAugMax);
  if (n_levels < 1 || n_levels > kAugLevels)
    return osd_fail(OSD_ERR_INVALID_ARG, "%s: n_levels = %d (1 .. %d)", what, n_levels, kAugLevels);
  if (dtype != OSD_F32 && dtype != OSD_BF16) return osd_fail(OSD_ERR_INVALID_ARG, "%s: bad dtype %d", what, dtype);
  if (method != OSD_SUPP_AUG_AVG && method != OSD_SUPP_AUG_MAX) return osd_fail(OSD_ERR_INVALID_ARG, "%s: bad method %d", what, method);
  if (groups < 0 || c < 1) return osd_fail(OSD_ERR_INVALID_ARG, "%s: bad arguments (groups %d, c %d)", what, groups, c);
  const int V = dtype == OSD_BF16 ? 8 : 4;
  if (c % V != 0)
    return osd_fail(OSD_ERR_UNSUPPORTED, "%s: c = %d is not a multiple of %d (one 16-byte group of the dtype)", what, c, V);
  L->n_levels = 0;
  if (groups == 0) return OSD_OK;      // a no-op: the callers return before the launch, the level pointers may be those of empty tensors
  long long blocks = 0;
  for (int l = 0; l < n_levels; ++l) {
    if (!xs[l] || !outs[l] || (dys && !dys[l])) return osd_fail(OSD_ERR_INVALID_ARG, "%s: null pointer at level %d", what, l);
    if (hw[l] < 1) return osd_fail(OSD_ERR_INVALID_ARG, "%s: bad level %d (%d pixels)", what, l, hw[l]);
    if (!aligned16(xs[l]) || !aligned16(outs[l]) || (dys && !aligned16(dys[l])))
      return osd_fail(OSD_ERR_UNSUPPORTED, "%s: level %d is not 16-byte aligned", what, l);
    const long long elems = (long long)groups * aug * hw[l] * c;
    if (elems >= (1LL << 31)) return osd_fail(OSD_ERR_UNSUPPORTED, "%s: level %d has %lld elements (at most 2^31 - 1)", what, l, elems);
    L->x[l] = xs[l];
    L->dy[l] = dys ? dys[l] : nullptr;
    L->out[l] = outs[l];
    L->per_map[l] = hw[l] * (c / V);
    L->block0[l] = (int)blocks;
    const long long nvec = (long long)groups * L->per_map[l];
    blocks += (nvec + kAugThreads * kAugPerThread - 1) / (kAugThreads * kAugPerThread);
  }
  if (blocks >= (1LL << 31)) return osd_fail(OSD_ERR_UNSUPPORTED, "%s: too many maps", what);
  L->block0[n_levels] = (int)blocks;
  L->n_levels = n_levels;
  return OSD_OK;
}

}  // namespace

#define OSD_AUG_LAUNCH(KERNEL)                                                                                                   \
  do {                                                                                                                           \
    const dim3 grid(L.block0[n_levels]), block(kAugThreads);                                                                     \
    if (dtype == OSD_F32 && method == OSD_SUPP_AUG_AVG)                                                                          \
      hipLaunchKernelGGL((KERNEL<float, OSD_SUPP_AUG_AVG>), grid, block, 0, OSD_STREAM(stream), L, groups, aug);                 \
    else if (dtype == OSD_F32)                                                                                                   \
      hipLaunchKernelGGL((KERNEL<float, OSD_SUPP_AUG_MAX>), grid, block, 0, OSD_STREAM(stream), L, groups, aug);                 \
    else if (method == OSD_SUPP_AUG_AVG)                                                                                         \
      hipLaunchKernelGGL((KERNEL<__bf16, OSD_SUPP_AUG_AVG>), grid, block, 0, OSD_STREAM(stream), L, groups, aug);                \
    else                                                                                                                         \
      hipLaunchKernelGGL((KERNEL<__bf16, OSD_SUPP_AUG_MAX>), grid, block, 0, OSD_STREAM(stream), L, groups, aug);                \
  } while (0)

extern "C" int osd_supp_aug_reduce_levels(int n_levels, const void* const* x, void* const* y, const int32_t* hw, int groups, int aug,
                                          int c, int dtype, int method, void* stream) {
  AugLevels L;
  const int rc = aug_setup("supp_aug_reduce_levels", n_levels, x, nullptr, y, hw, groups, aug, c, dtype, method, &L);
  if (rc != OSD_OK) return rc;
  if (groups == 0) return OSD_OK;
  OSD_AUG_LAUNCH(supp_aug_reduce_kernel);
  return osd_check_launch("supp_aug_reduce_levels");
}

extern "C" int osd_supp_aug_reduce_levels_bwd(int n_levels, const void* const* x, const void* const* dy, void* const* dx,
                                              const int32_t* hw, int groups, int aug, int c, int dtype, int method, void* stream) {
  if (!dy) return osd_fail(OSD_ERR_INVALID_ARG, "supp_aug_reduce_levels_bwd: null pointer");
  AugLevels L;
  const int rc = aug_setup("supp_aug_reduce_levels_bwd", n_levels, x, dy, dx, hw, groups, aug, c, dtype, method, &L);
  if (rc != OSD_OK) return rc;
  if (groups == 0) return OSD_OK;
  OSD_AUG_LAUNCH(supp_aug_reduce_bwd_kernel);
  return osd_check_launch("supp_aug_reduce_levels_bwd");
}
