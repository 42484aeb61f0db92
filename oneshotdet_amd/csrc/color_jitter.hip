// color_jitter.hip — the reference's colour jitter of support crops (data/datasets/coco.py:286-294, NUM_SUPP_AUG = 3) for gfx950: the
// four PIL ImageEnhance steps Color, Brightness, Contrast, Sharpness, each Image.blend(degenerate, image, factor), on uint8 RGB
// [H][W][3] images that are already on the device.  Pillow: Convert.c rgb2l (the grey image), Blend.c ImagingBlend, ImageStat mean
// (Contrast's grey level), Filter.c ImagingFilter3x3 with ImageFilter.SMOOTH (Sharpness's degenerate).  Restated in
// tests/color_jitter_ref.py, which is bit-exact against Pillow and against a fixture recorded through the reference's method; these
// kernels are bit-exact too: integer luma and mean, and the float steps are Pillow's float32 operations one by one, each rounded on
// its own: floating-point contraction is switched off for this translation unit (the pragma below).  hipcc's __fmul_rn / __fadd_rn
// are plain `*` and `+` compiled under the header's contraction mode, so a product and a sum written with them DO fuse into one
// v_fma_f32 (one rounding instead of two, measured: 26 of 1056 bytes off by 1 or 2); mul_rn / add_rn here are compiled under the pragma.
//
// Two launches per chunk of kJitterMaxImages images, grid (tiles, images), the table by value in the kernarg segment as in
// transforms.hip.  The first launch writes one 64-bit integer sum of L(brightness image) per workgroup into that workgroup's own slot;
// the second re-reduces an image's slots (integers: any order gives the same sum), stages the contrast image of a 32 x 8 tile and its
// one-pixel halo in LDS, and writes the sharpened pixels.  No atomics, no memset, no host read-back: every slot that is read has been
// written by the first launch, so the result does not depend on what the workspace held.
#include "osd_common.h"
#include "../../include/oneshotdet_hip_color_jitter.h"
#include <cmath>
#include <cstddef>

#pragma clang fp contract(off)

namespace {

__device__ __forceinline__ float mul_rn(float a, float b) { return a * b; }
__device__ __forceinline__ float add_rn(float a, float b) { return a + b; }

constexpr int kJitterMaxImages = OSD_COLOR_JITTER_MAX_IMAGES;
constexpr int kThreads = 256;
constexpr int kSumPixels = 2048;            // pixels per workgroup (= per slot) of the first launch
constexpr int kTileW = 32, kTileH = 8;      // pixels per workgroup of the second launch; kTileW * kTileH == kThreads
constexpr int kHaloW = kTileW + 2, kHaloH = kTileH + 2;

struct JitterEntry {
  const unsigned char* src;      // RGB uint8 [h][w][3]
  unsigned char* dst;            // RGB uint8 [h][w][3]
  long long* slots;              // n_slots partial sums of L(brightness image)
  int h, w, n_slots, tiles_x;
  float f[4];                    // Color, Brightness, Contrast, Sharpness
};
struct JitterTable { JitterEntry im[kJitterMaxImages]; };

// the table entry of this workgroup's image, read with scalar loads from the kernarg segment (see transforms.hip: image_entry)
__device__ __forceinline__ JitterEntry jitter_entry(int idx) {
  typedef const __attribute__((address_space(4))) char* kcp;
  typedef unsigned long long u64;
  kcp b = (kcp)__builtin_amdgcn_kernarg_segment_ptr() + (size_t)idx * sizeof(JitterEntry);
#define OSD_CJF(type, field) (*reinterpret_cast<const __attribute__((address_space(4))) type*>(b + offsetof(JitterEntry, field)))
  JitterEntry e;
  e.src = (const unsigned char*)OSD_CJF(u64, src); e.dst = (unsigned char*)OSD_CJF(u64, dst); e.slots = (long long*)OSD_CJF(u64, slots);
  e.h = OSD_CJF(int, h); e.w = OSD_CJF(int, w); e.n_slots = OSD_CJF(int, n_slots); e.tiles_x = OSD_CJF(int, tiles_x);
  e.f[0] = OSD_CJF(float, f[0]); e.f[1] = OSD_CJF(float, f[1]); e.f[2] = OSD_CJF(float, f[2]); e.f[3] = OSD_CJF(float, f[3]);
#undef OSD_CJF
  return e;
}

// Convert.c rgb2l
__device__ __forceinline__ int luma(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Blend.c ImagingBlend on one byte: d + f * (x - d) in float32, the product and the sum rounded separately; a factor in [0, 1] cannot
// leave 0..255 and is truncated, any other is clipped first
__device__ __forceinline__ int blend(int d, int x, float f) {
  const float t = add_rn((float)d, mul_rn(f, (float)(x - d)));
  if (f >= 0.0f && f <= 1.0f) return (int)t & 255;
  return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

// ImageEnhance.Color then ImageEnhance.Brightness on one pixel
__device__ __forceinline__ void color_brightness(const unsigned char* __restrict__ p, float f_color, float f_bright, int* px) {
  const int r = p[0], g = p[1], b = p[2];
  const int l = luma(r, g, b);
  px[0] = blend(0, blend(l, r, f_color), f_bright);
  px[1] = blend(0, blend(l, g, f_color), f_bright);
  px[2] = blend(0, blend(l, b, f_color), f_bright);
}

// sum over the workgroup, every thread gets it; `red` holds kThreads values
__device__ __forceinline__ long long block_sum(long long v, long long* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = kThreads / 2; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  const long long total = red[0];
  __syncthreads();
  return total;
}

// first launch: slots[blockIdx.x] = sum of L(brightness image) over pixels [blockIdx.x * kSumPixels, + kSumPixels)
__global__ __launch_bounds__(kThreads) void jitter_sums_kernel(JitterTable) {
  __shared__ long long red[kThreads];
  const JitterEntry e = jitter_entry(blockIdx.y);
  if ((int)blockIdx.x >= e.n_slots) return;
  const long long n = (long long)e.h * e.w;
  const long long base = (long long)blockIdx.x * kSumPixels;
  long long acc = 0;
  for (int k = 0; k < kSumPixels / kThreads; ++k) {
    const long long i = base + k * kThreads + (int)threadIdx.x;
    if (i < n) {
      int px[3];
      color_brightness(e.src + (size_t)i * 3, e.f[0], e.f[1], px);
      acc += luma(px[0], px[1], px[2]);
    }
  }
  const long long total = block_sum(acc, red);
  if (threadIdx.x == 0) e.slots[blockIdx.x] = total;
}

// second launch: one 32 x 8 tile per workgroup
__global__ __launch_bounds__(kThreads) void jitter_apply_kernel(JitterTable) {
  __shared__ long long red[kThreads];
  __shared__ unsigned int tile[kHaloH][kHaloW];       // the contrast image: r | g << 8 | b << 16
  const JitterEntry e = jitter_entry(blockIdx.y);
  const int h = e.h, w = e.w;
  const int tiles_y = (h + kTileH - 1) / kTileH;
  if ((long long)blockIdx.x >= (long long)e.tiles_x * tiles_y) return;
  // ImageEnhance.Contrast's grey level: int(mean(L) + 0.5) = (2 S + N) / (2 N) in integers
  long long acc = 0;
  for (int s = threadIdx.x; s < e.n_slots; s += kThreads) acc += e.slots[s];
  const long long sum = block_sum(acc, red);
  const long long n = (long long)h * w;
  const int mean = (int)((2 * sum + n) / (2 * n));
  const int ty = (int)(blockIdx.x / (unsigned)e.tiles_x), tx = (int)(blockIdx.x - (unsigned)ty * (unsigned)e.tiles_x);
  const int y0 = ty * kTileH - 1, x0 = tx * kTileW - 1;
  for (int t = threadIdx.x; t < kHaloH * kHaloW; t += kThreads) {
    const int ly = t / kHaloW, lx = t - ly * kHaloW;
    const int y = y0 + ly, x = x0 + lx;
    unsigned int v = 0;
    if ((unsigned)y < (unsigned)h && (unsigned)x < (unsigned)w) {
      int px[3];
      color_brightness(e.src + ((size_t)y * w + x) * 3, e.f[0], e.f[1], px);
      v = (unsigned)blend(mean, px[0], e.f[2]) | ((unsigned)blend(mean, px[1], e.f[2]) << 8) | ((unsigned)blend(mean, px[2], e.f[2]) << 16);
    }
    tile[ly][lx] = v;
  }
  __syncthreads();
  const int ly = threadIdx.x / kTileW + 1, lx = threadIdx.x % kTileW + 1;
  const int y = y0 + ly, x = x0 + lx;
  if (y >= h || x >= w) return;
  const unsigned int c = tile[ly][lx];
  unsigned char* o = e.dst + ((size_t)y * w + x) * 3;
  if (y < 1 || x < 1 || y >= h - 1 || x >= w - 1) {       // Filter.c copies the border: the blend of a byte with itself
    o[0] = (unsigned char)(c & 255); o[1] = (unsigned char)((c >> 8) & 255); o[2] = (unsigned char)((c >> 16) & 255);
    return;
  }
  // ImageFilter.SMOOTH: (1 1 1 / 1 5 1 / 1 1 1) / 13, float32 weights, accumulated from 0.5 in float32 and truncated.  The exact value
  // is an integer / 13 + 0.5, never within 0.03 of an integer, so the order of accumulation cannot change the byte.
  const float k = 1.0f / 13.0f, kc = 5.0f / 13.0f;      // float32 quotients, as Filter.c divides the kernel by its scale
  float ss[3] = {0.5f, 0.5f, 0.5f};
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
    for (int dx = -1; dx <= 1; ++dx) {
      const unsigned int v = tile[ly + dy][lx + dx];
      const float wgt = (dy == 0 && dx == 0) ? kc : k;
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) ss[ch] = add_rn(ss[ch], mul_rn((float)((v >> (8 * ch)) & 255), wgt));
    }
  }
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    int s = (int)ss[ch];
    s = s < 0 ? 0 : (s > 255 ? 255 : s);
    o[ch] = (unsigned char)blend(s, (int)((c >> (8 * ch)) & 255), e.f[3]);          // ImageEnhance.Sharpness
  }
}

inline size_t al256(size_t v) { return (v + 255) & ~(size_t)255; }
inline long long n_slots_of(int h, int w) { return ((long long)h * w + kSumPixels - 1) / kSumPixels; }

}  // namespace

extern "C" int64_t osd_color_jitter_workspace_bytes(int n_images, const int32_t* hs, const int32_t* ws) {
  if (n_images <= 0 || !hs || !ws) return 0;
  size_t total = 0;
  for (int i = 0; i < n_images; ++i) {
    if (hs[i] <= 0 || ws[i] <= 0) return 0;
    total += al256((size_t)n_slots_of(hs[i], ws[i]) * sizeof(long long));
  }
  return (int64_t)total;
}

extern "C" int osd_color_jitter_batch(int n_images, const uint8_t* const* srcs_rgb_hwc, const int32_t* hs, const int32_t* ws,
                                      const float* factors, uint8_t* const* dsts_rgb_hwc, void* workspace, void* stream) {
  if (n_images < 0) return osd_fail(OSD_ERR_INVALID_ARG, "color_jitter: n_images %d", n_images);
  if (!srcs_rgb_hwc || !hs || !ws || !factors || !dsts_rgb_hwc || !workspace)
    return osd_fail(OSD_ERR_INVALID_ARG, "color_jitter: null argument");
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return osd_fail(OSD_ERR_INVALID_ARG, "color_jitter: workspace not 8-byte aligned");
  // every check before any launch
  for (int i = 0; i < n_images; ++i) {
    if (!srcs_rgb_hwc[i] || !dsts_rgb_hwc[i]) return osd_fail(OSD_ERR_INVALID_ARG, "color_jitter: null image %d", i);
    if (hs[i] <= 0 || ws[i] <= 0) return osd_fail(OSD_ERR_INVALID_ARG, "color_jitter: bad size %d x %d of image %d", hs[i], ws[i], i);
    if (dsts_rgb_hwc[i] == srcs_rgb_hwc[i])
      return osd_fail(OSD_ERR_INVALID_ARG, "color_jitter: image %d in place (the sharpness step reads a pixel's neighbours)", i);
    for (int k = 0; k < 4; ++k) {
      const float f = factors[i * 4 + k];
      if (!(f >= 0.0f) || std::isinf(f))
        return osd_fail(OSD_ERR_INVALID_ARG, "color_jitter: factor %d of image %d is negative or not finite", k, i);
    }
  }
  for (int i = 0; i < n_images; ++i)
    if ((long long)hs[i] * ws[i] > 0x7fffffffLL)
      return osd_fail(OSD_ERR_UNSUPPORTED, "color_jitter: image %d has 2^31 pixels or more", i);
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  char* p = static_cast<char*>(workspace);
  for (int base = 0; base < n_images; base += kJitterMaxImages) {
    const int cnt = n_images - base < kJitterMaxImages ? n_images - base : kJitterMaxImages;
    JitterTable tab;
    long long max_slots = 1, max_tiles = 1;
    for (int j = 0; j < kJitterMaxImages; ++j) {
      JitterEntry& e = tab.im[j];
      if (j >= cnt) { e = tab.im[0]; continue; }      // never indexed: the grid's y extent is cnt
      const int i = base + j;
      e.src = srcs_rgb_hwc[i]; e.dst = dsts_rgb_hwc[i];
      e.h = hs[i]; e.w = ws[i];
      e.n_slots = (int)n_slots_of(e.h, e.w);
      e.tiles_x = cdiv(e.w, kTileW);
      for (int k = 0; k < 4; ++k) e.f[k] = factors[i * 4 + k];
      e.slots = reinterpret_cast<long long*>(p);      // workspace slices in the layout osd_color_jitter_workspace_bytes sums up
      p += al256((size_t)e.n_slots * sizeof(long long));
      const long long tiles = (long long)e.tiles_x * cdiv(e.h, kTileH);
      if (e.n_slots > max_slots) max_slots = e.n_slots;
      if (tiles > max_tiles) max_tiles = tiles;
    }
    hipLaunchKernelGGL(jitter_sums_kernel, dim3((unsigned)max_slots, cnt), dim3(kThreads), 0, st, tab);
    int rc = osd_check_launch("color_jitter: sums");
    if (rc) return rc;
    hipLaunchKernelGGL(jitter_apply_kernel, dim3((unsigned)max_tiles, cnt), dim3(kThreads), 0, st, tab);
    rc = osd_check_launch("color_jitter");
    if (rc) return rc;
  }
  return OSD_OK;
}
