// conv_pred_bwd — data gradient AND weight gradient of an FCOS prediction conv (3x3 / stride 1 / pad 1, Cout <= 4, Cin a multiple
// of 256, bf16) over all FPN levels in ONE launch (gfx950):
//     G[q][tap * 4 + co] = dy[q - (tap / 3 - 1, tap % 3 - 1)][co]     (the nine shifted dy vectors of pixel q side by side; columns
//                                                                      >= 36, channels >= cout and taps outside the map are zero)
//     dX[q][ci]          = sum_k G[q][k] * Wd[ci][k]                   (K = 64, Wd from osd_pred_dgrad_pack)
//     T[k][ci]           = sum_q G[q][k] * X[q][ci]                    (dw[co][tap][ci] += T[tap * 4 + co][ci]; db[co] += sum_q G[q][16 + co])
// osd_pred_dy_gather writes G to memory (128 bytes per pixel) for two GEMM launches to read back; here a workgroup builds a tile of
// G in LDS from dy (1 MB, cache resident) and uses it for both products, so the launch reads X once and writes dX once.
//
// A workgroup (4 waves) owns a run of consecutive pixels of G's row order — the levels one after the other, the images one
// after the other within a level; the grid is sized so that all workgroups are resident — and walks it in tiles of TP pixels;
// every row finds its level by itself, so a tile may cross image and level boundaries.  A wave owns 64 of the workgroup's
// 256 input channels (blockIdx.y = the 256-channel group) for both products:
//   * dX^T[ci][q] = Wd[ci][k] * G^T[k][q] with v_mfma_f32_16x16x32_bf16, two K steps: Wd's fragments stay in registers for the
//     whole launch, G's are row reads of the tile (K contiguous); an accumulator lane holds 4 consecutive channels of one pixel,
//     and the channel order of the M tiles gives it 8 (one 16-byte store; four lanes write 64 contiguous bytes of a pixel row).
//   * T = G^T X: both operands are pixel-major, the reduction runs over pixels, so both fragments are transposed LDS reads
//     (ds_read_b64_tr_b16) with the k-slot map of conv_wgrad.hip: rows (4g + j | 16 + 4g + j - 4) of a 32-pixel step.  X is staged
//     per WAVE ([64 pixels][64 channels], loaded to registers one stage ahead): the staging needs no workgroup barrier.
//     T (48 x 64 per wave) stays in accumulator registers over all tiles; at the end every workgroup stores its 9 * cout real
//     rows, and a second small launch adds the partials in workgroup order into dw / db: no atomics, no memset, same bits every run.
// LDS image of G and of an X stage: 128-byte rows, 16-byte chunk c of row r at chunk c ^ 2 * ((r >> 1) & 3): the 8 rows x 32 bytes a
// half-wave takes in a transposed read cover the 64 banks once, and so do the 16 x 16 bytes of a row read's lane group.
#include "osd_common.h"

#include <stdlib.h>

#define OSD_STREAM(s) reinterpret_cast<hipStream_t>(s)

namespace {

constexpr int kLevels = 6;       // = kPredLevels of conv_wgrad.hip
constexpr int kG = 64;           // columns of G (36 used)
constexpr int TP = 128;          // pixels per G tile
constexpr int SP = 64;           // pixels per X stage (two 32-pixel MFMA steps)

struct PredBwdLevels {
  const void* x[kLevels];
  const void* dy[kLevels];
  int H[kLevels], W[kLevels], npix[kLevels], begin[kLevels];
  int n_levels;
};

__device__ __attribute__((aligned(16))) unsigned g_pb_zero[4];

typedef __attribute__((address_space(3))) bf16x4* lds_bf4_ptr;

__device__ __forceinline__ int pb_swz(int row) { return ((row >> 1) & 3) << 1; }
__device__ __forceinline__ int pb_off(int row, int chunk) { return row * 128 + ((chunk ^ pb_swz(row)) << 4); }

template <bool DG, bool WG>
__global__ void __launch_bounds__(256, 2) pred_bwd_kernel(PredBwdLevels L, const __bf16* __restrict__ wd, __bf16* __restrict__ dx,
                                                          float* __restrict__ part, float* __restrict__ part_b, int cin, int cout,
                                                          int dy_stride, int tot, int ppw) {
  __shared__ __attribute__((aligned(16))) char s_g[TP * 128];
  __shared__ __attribute__((aligned(16))) char s_x[4 * SP * 128];
  __shared__ const char* s_row[TP];
  __shared__ float s_b[4][4];

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cg = blockIdx.y;
  const int p0 = blockIdx.x * ppw, p1 = min(tot, p0 + ppw);
  const int g4 = lane >> 4, l16 = lane & 15;

  // Wd fragments (A operand of dX^T = Wd G^T): M tile i, row r <-> channel (i >> 1) * 32 + (r >> 2) * 8 + (i & 1) * 4 + (r & 3)
  bf16x8 wa[4][2];
  if constexpr (DG) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ci = cg * 256 + wave * 64 + (i >> 1) * 32 + (l16 >> 2) * 8 + (i & 1) * 4 + (l16 & 3);
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) wa[i][ks] = *reinterpret_cast<const bf16x8*>(wd + (size_t)ci * kG + ks * 32 + g4 * 8);
    }
  }
  f32x4 acc[3][4];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};

  char* sx = s_x + wave * (SP * 128);
  bf16x8 xr[8];
  auto load_stage = [&](int s) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const char* rp = s_row[s * SP + i * 8 + (lane >> 3)];
      const char* src = rp != nullptr ? rp + wave * 128 + (lane & 7) * 16 : reinterpret_cast<const char*>(g_pb_zero);
      xr[i] = *reinterpret_cast<const bf16x8*>(src);
    }
  };

  for (int t0 = p0; t0 < p1; t0 += TP) {
    const int rows = min(TP, p1 - t0);
    __syncthreads();                       // the previous tile's readers of s_g / s_row are done
    // ---- G tile + the X row pointers (the arithmetic of pred_dy_gather_kernel; one 16-byte chunk = two taps x four channels) ----
#pragma unroll
    for (int it = 0; it < TP * 8 / 256; ++it) {
      const int idx = it * 256 + tid;
      const int px = idx >> 3, c8 = idx & 7;
      const bool valid = px < rows;
      const int q_all = valid ? t0 + px : p0;
      int lvl = 0;
#pragma unroll
      for (int i = 1; i < kLevels; ++i)
        if (i < L.n_levels && q_all >= L.begin[i]) lvl = i;
      const void* dyv = L.dy[0];
      const void* xv = L.x[0];
      int H = L.H[0], W = L.W[0], beg = L.begin[0];
#pragma unroll
      for (int i = 1; i < kLevels; ++i)
        if (lvl == i) { dyv = L.dy[i]; xv = L.x[i]; H = L.H[i]; W = L.W[i]; beg = L.begin[i]; }
      const __bf16* __restrict__ dy = reinterpret_cast<const __bf16*>(dyv);
      const int q = q_all - beg, HW = H * W;
      const int img = q / HW, rem = q - img * HW, qy = rem / W, qx = rem - qy * W;
      bf16x8 out;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int t = 2 * c8 + h;
        const int py = qy - t / 3 + 1, pxx = qx - t % 3 + 1;
        const bool ok = valid && t < 9 && (unsigned)py < (unsigned)H && (unsigned)pxx < (unsigned)W;
        const bf16x4* src = ok ? reinterpret_cast<const bf16x4*>(dy + ((size_t)(img * H + py) * W + pxx) * dy_stride)
                               : reinterpret_cast<const bf16x4*>(g_pb_zero);
        const bf16x4 v = *src;
#pragma unroll
        for (int co = 0; co < 4; ++co) out[h * 4 + co] = co < cout ? v[co] : (__bf16)0.f;
      }
      if (c8 == 2) {                        // the centre tap: the bias gradient's column sums
#pragma unroll
        for (int co = 0; co < 4; ++co) bsum[co] += (float)out[co];
      }
      *reinterpret_cast<bf16x8*>(s_g + pb_off(px, c8)) = out;
      if (c8 == 0)
        s_row[px] = valid ? reinterpret_cast<const char*>(xv) + ((size_t)q * cin + cg * 256) * 2 : nullptr;
    }
    __syncthreads();
    const int nst = (rows + SP - 1) / SP;
    if constexpr (WG) load_stage(0);        // in flight during the data gradient

    // ---- data gradient: dX^T tile by tile of 16 pixels ----
    if constexpr (DG) {
      for (int n = 0; n * 16 < rows; ++n) {
        const int row = n * 16 + l16;
        const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(s_g + pb_off(row, g4));
        const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(s_g + pb_off(row, 4 + g4));
        f32x4 d[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          d[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[i][0], b0, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
          d[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wa[i][1], b1, d[i], 0, 0, 0);
        }
        if (row < rows) {
          __bf16* o = dx + (size_t)(t0 + row) * cin + cg * 256 + wave * 64 + g4 * 8;
#pragma unroll
          for (int h = 0; h < 2; ++h) {
            bf16x8 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) { v[e] = (__bf16)d[2 * h][e]; v[4 + e] = (__bf16)d[2 * h + 1][e]; }
            *reinterpret_cast<bf16x8*>(o + h * 32) = v;
          }
        }
      }
    }

    // ---- weight gradient: T += G^T X over the tile's pixels, X stage by stage through the wave's own LDS buffer ----
    if constexpr (WG) {
#pragma unroll
      for (int s = 0; s < TP / SP; ++s) {
        if (s < nst) {
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");      // the previous stage's reads precede these writes
#pragma unroll
          for (int i = 0; i < 8; ++i) *reinterpret_cast<bf16x8*>(sx + pb_off(i * 8 + (lane >> 3), lane & 7)) = xr[i];
          if (s + 1 < nst) load_stage(s + 1);
          __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
          __builtin_amdgcn_wave_barrier();
          const int q4 = l16 >> 2, pp = l16 & 3, h8 = (pp & 1) * 8;
#pragma unroll
          for (int kk = 0; kk < SP / 32; ++kk) {
            if (s * SP + kk * 32 < rows) {
              const int rs1 = kk * 32 + 4 * g4 + q4, rs2 = rs1 + 16;
              const int rg1 = s * SP + rs1, rg2 = rg1 + 16;
              bf16x8 af[3], bfr[4];
#pragma unroll
              for (int i = 0; i < 3; ++i) {
                const int chunk = 2 * i + (pp >> 1);
                const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf4_ptr)(s_g + pb_off(rg1, chunk) + h8));
                const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf4_ptr)(s_g + pb_off(rg2, chunk) + h8));
#pragma unroll
                for (int e = 0; e < 4; ++e) { af[i][e] = lo[e]; af[i][e + 4] = hi[e]; }
              }
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                const int chunk = 2 * j + (pp >> 1);
                const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf4_ptr)(sx + pb_off(rs1, chunk) + h8));
                const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf4_ptr)(sx + pb_off(rs2, chunk) + h8));
#pragma unroll
                for (int e = 0; e < 4; ++e) { bfr[j][e] = lo[e]; bfr[j][e + 4] = hi[e]; }
              }
#pragma unroll
              for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
            }
          }
        }
      }
    }
  }

  if constexpr (WG) {
    // the workgroup's partial T: the 9 * cout real rows, in dw's [co][tap] order
    const int rows_real = 9 * cout;
    float* pp = part + ((size_t)blockIdx.x * gridDim.y + cg) * rows_real * 256 + wave * 64 + l16;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int grow = 16 * i + 4 * g4 + e, tap = grow >> 2, co = grow & 3;
        if (tap < 9 && co < cout) {
#pragma unroll
          for (int j = 0; j < 4; ++j) pp[(co * 9 + tap) * 256 + 16 * j] = acc[i][j][e];
        }
      }
    if (cg == 0) {                           // bias partials: lanes, then waves, in a fixed order
#pragma unroll
      for (int co = 0; co < 4; ++co) {
        float v = bsum[co];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
        if (lane == 0) s_b[wave][co] = v;
      }
      __syncthreads();
      if (tid < 4) part_b[(size_t)blockIdx.x * 4 + tid] = (s_b[0][tid] + s_b[1][tid]) + (s_b[2][tid] + s_b[3][tid]);
    }
  }
}

// dw[co][tap][ci] += the partials of all workgroups, db[co] += the bias partials: 16 elements x 16 slices of the workgroup list per
// block, every slice summed in its order, the 16 slice sums added in their order by one thread (plain load + store: same bits every run)
__global__ void __launch_bounds__(256) pred_bwd_reduce_kernel(const float* __restrict__ part, const float* __restrict__ part_b,
                                                              float* __restrict__ dw, float* __restrict__ db, int nwg, int groups,
                                                              int cin, int cout) {
  __shared__ float s[16][17];
  const int e = threadIdx.x & 15, sl = threadIdx.x >> 4;
  const int n = cout * 9 * cin;                       // a multiple of 16
  const bool bias = (int)blockIdx.x == n / 16;
  const int per = (nwg + 15) / 16;
  const int b0 = sl * per, b1 = min(nwg, b0 + per);
  const int i = blockIdx.x * 16 + e;
  const float* p;
  size_t stride;
  bool on;
  if (!bias) {
    const int ci = i % cin, ct = i / cin;
    p = part + ((size_t)(ci >> 8) * 9 * cout + ct) * 256 + (ci & 255);
    stride = (size_t)groups * 9 * cout * 256;
    on = true;
  } else {
    p = part_b + e;
    stride = 4;
    on = e < cout;
  }
  // sixteen independent loads in flight per thread, the ragged end of a slice as loads of its first row whose values are dropped: the
  // launch sits on the backward pass's critical chain, and every dependent round costs a memory latency there
  float a[16];
#pragma unroll
  for (int u = 0; u < 16; ++u) a[u] = 0.f;
  if (on) {
    for (int b = b0; b < b1; b += 16) {
      float v[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const bool ok = b + u < b1;
        v[u] = p[(size_t)(ok ? b + u : b0) * stride];
        if (!ok) v[u] = 0.f;
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) a[u] += v[u];
    }
  }
  s[sl][e] = (((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))) + (((a[8] + a[9]) + (a[10] + a[11])) + ((a[12] + a[13]) + (a[14] + a[15])));
  __syncthreads();
  if (sl == 0 && on) {
    float t = 0.f;
#pragma unroll
    for (int k = 0; k < 16; ++k) t += s[k][e];
    if (!bias) dw[i] += t;
    else db[e] += t;
  }
}

// pixels per workgroup and the number of workgroups: two resident workgroups per CU share out the pixels evenly (a multiple of the
// 16-pixel MFMA tile each), `groups` 256-channel groups per pixel run.  Not below 272 pixels (the benchmark's share): a workgroup's
// fixed cost — Wd's fragments, the store of its partial T and its share of the reduce — is paid per workgroup
void pred_bwd_plan(long long tot, int groups, int* ppw, int* nwg) {
  static int target = -1;        // OSD_PRED_BWD_WGS: workgroups of the launch (measurement)
  if (target < 0) { const char* e = getenv("OSD_PRED_BWD_WGS"); target = e ? atoi(e) : 0; if (target < 1) target = 512; }
  int t = target / groups;
  if (t < 1) t = 1;
  long long p = ((tot + t - 1) / t + 15) / 16 * 16;
  if (p < 272) p = 272;
  *ppw = (int)p;
  *nwg = (int)((tot + p - 1) / p);
}

int pred_bwd_check(const osd_conv_desc* d, int n_seg, const int32_t* ns, const int32_t* hs, const int32_t* ws, long long* tot_out) {
  if (!d || !ns || !hs || !ws || n_seg < 1 || n_seg > kLevels) return osd_fail(OSD_ERR_INVALID_ARG, "pred_bwd: bad arguments (1..%d levels)", kLevels);
  if (d->dtype != OSD_F32 && d->dtype != OSD_BF16) return osd_fail(OSD_ERR_INVALID_ARG, "pred_bwd: bad dtype");
  if (d->dtype != OSD_BF16) return osd_fail(OSD_ERR_UNSUPPORTED, "pred_bwd: bf16 only");
  if (d->cout < 1 || d->cout > 4 || d->r != 3 || d->s != 3 || d->stride_h != 1 || d->stride_w != 1 || d->pad_h != 1 || d->pad_w != 1 ||
      d->cin <= 0 || d->cin % 256 != 0 || d->out_stride < 4 || d->out_stride % 4 != 0)
    return osd_fail(OSD_ERR_UNSUPPORTED, "pred_bwd: 3x3 / stride 1 / pad 1, cout <= 4, cin %% 256 == 0, dy rows of >= 4 channels");
  long long tot = 0;
  for (int i = 0; i < n_seg; ++i) {
    if (ns[i] <= 0 || hs[i] <= 0 || ws[i] <= 0) return osd_fail(OSD_ERR_INVALID_ARG, "pred_bwd: bad segment %d", i);
    const long long npix = (long long)ns[i] * hs[i] * ws[i];
    if (npix > 0x7fffffffLL / d->out_stride) return osd_fail(OSD_ERR_INVALID_ARG, "pred_bwd: bad segment %d", i);
    tot += npix;
  }
  if (tot > 0x7fffffffLL / 8) return osd_fail(OSD_ERR_INVALID_ARG, "pred_bwd: too many pixels");
  *tot_out = tot;
  return OSD_OK;
}

}  // namespace

extern "C" int64_t osd_pred_bwd_workspace_bytes(int n_seg, const int32_t* ns, const int32_t* hs, const int32_t* ws, int cin, int cout) {
  if (n_seg < 1 || n_seg > kLevels || !ns || !hs || !ws || cin <= 0 || cin % 256 != 0 || cout < 1 || cout > 4) return 0;
  long long tot = 0;
  for (int i = 0; i < n_seg; ++i) tot += (long long)ns[i] * hs[i] * ws[i];
  if (tot <= 0) return 0;
  int ppw, nwg;
  pred_bwd_plan(tot, cin / 256, &ppw, &nwg);
  return (int64_t)nwg * (cin / 256) * 9 * cout * 256 * 4 + (int64_t)nwg * 4 * 4 + 256;
}

extern "C" int osd_conv2d_pred_bwd(const osd_conv_desc* d, int n_seg, const void* const* xs, const void* const* dys, const int32_t* ns,
                                   const int32_t* hs, const int32_t* ws, const void* wd_packed, void* dx, float* dw, float* db,
                                   void* workspace, int flags, void* stream) {
  long long tot = 0;
  int rc = pred_bwd_check(d, n_seg, ns, hs, ws, &tot);
  if (rc) return rc;
  if (flags != OSD_PRED_BWD_BOTH && flags != OSD_PRED_BWD_DGRAD && flags != OSD_PRED_BWD_WGRAD)
    return osd_fail(OSD_ERR_INVALID_ARG, "pred_bwd: bad flags %d", flags);
  const bool dg = flags != OSD_PRED_BWD_WGRAD, wg = flags != OSD_PRED_BWD_DGRAD;
  if (!dys || (wg && (!xs || !dw || !workspace)) || (dg && (!wd_packed || !dx))) return osd_fail(OSD_ERR_INVALID_ARG, "pred_bwd: null argument");
  if (((size_t)wd_packed | (size_t)dx | (size_t)workspace) & 15) return osd_fail(OSD_ERR_INVALID_ARG, "pred_bwd: wd_packed, dx and workspace must be 16-byte aligned");
  PredBwdLevels L;
  L.n_levels = n_seg;
  long long beg = 0;
  for (int i = 0; i < kLevels; ++i) {
    const int j = i < n_seg ? i : 0;
    if (!dys[j] || (wg && !xs[j])) return osd_fail(OSD_ERR_INVALID_ARG, "pred_bwd: null segment %d", j);
    if (((size_t)dys[j] & 7) || (wg && ((size_t)xs[j] & 15))) return osd_fail(OSD_ERR_INVALID_ARG, "pred_bwd: segment %d: dy must be 8-byte, x 16-byte aligned", j);
    const long long npix = (long long)ns[j] * hs[j] * ws[j];
    L.x[i] = wg ? xs[j] : nullptr; L.dy[i] = dys[j]; L.H[i] = hs[j]; L.W[i] = ws[j];
    L.npix[i] = i < n_seg ? (int)npix : 0; L.begin[i] = i < n_seg ? (int)beg : 0x7fffffff;
    if (i < n_seg) beg += npix;
  }
  const int groups = d->cin / 256;
  int ppw, nwg;
  pred_bwd_plan(tot, groups, &ppw, &nwg);
  float* part = static_cast<float*>(workspace);
  float* part_b = wg ? part + (size_t)nwg * groups * 9 * d->cout * 256 : nullptr;
  hipStream_t st = OSD_STREAM(stream);
  const dim3 grid(nwg, groups);
#define OSD_PB_LAUNCH(DG, WG)                                                                                                        \
  hipLaunchKernelGGL((pred_bwd_kernel<DG, WG>), grid, dim3(256), 0, st, L, (const __bf16*)wd_packed, (__bf16*)dx, part, part_b, d->cin, \
                     d->cout, d->out_stride, (int)tot, ppw)
  if (dg && wg) OSD_PB_LAUNCH(true, true);
  else if (dg) OSD_PB_LAUNCH(true, false);
  else OSD_PB_LAUNCH(false, true);
#undef OSD_PB_LAUNCH
  rc = osd_check_launch("pred_bwd");
  if (rc || !wg) return rc;
  const int n = d->cout * 9 * d->cin;
  hipLaunchKernelGGL(pred_bwd_reduce_kernel, dim3(n / 16 + (db ? 1 : 0)), dim3(256), 0, st, (const float*)part, (const float*)part_b, dw, db,
                     nwg, groups, d->cin, d->cout);
  return osd_check_launch("pred_bwd(reduce)");
}
