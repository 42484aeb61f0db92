/*
 * oneshotdet_hip_color_jitter.h — C-ABI of liboneshotdet_hip.so, fifth part: the colour jitter of support crops (FEW_SHOT.SUPP_AUG with
 * NUM_SUPP_AUG = 3, config/defaults.py).  Same conventions as oneshotdet_hip.h (raw device pointers, caller-allocated outputs,
 * asynchronous on `stream`, 0 = OK / negative = OSD_ERR_*); paths relative to the reference's maskrcnn_benchmark/.  The ABI version is
 * unchanged.
 *
 * With NUM_SUPP_AUG = 3 every support is four rows: the crop, its horizontal flip, the colour-jittered crop and the colour-jittered flip
 * (data/datasets/coco.py:447-452).  The jitter (coco.py:286-294) is four PIL ImageEnhance steps in a row — Color, Brightness, Contrast,
 * Sharpness — each Image.blend(degenerate, image, factor) with its own factor; every step yields a uint8 image that the next one reads.
 * All of it is integer or float32 arithmetic on bytes and is reproduced bit for bit:
 *   L(a)            = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16                        (convert("L"))
 *   blend(d, x, f)  = t = float32(d) + float32(f * float32(x - d)), product and sum rounded separately; for 0 <= f <= 1 the byte is
 *                     trunc(t), otherwise 0 where t <= 0, 255 where t >= 255, trunc(t) elsewhere   (ImagingBlend)
 *   Color           b1 = blend(L(a) on all three channels, a, f0)
 *   Brightness      b2 = blend(0, b1, f1)
 *   Contrast        b3 = blend(m, b2, f2), m = (2*S + N) / (2*N) in integers, S = sum of L(b2) over the image, N = H*W  (int(mean + 0.5))
 *   Sharpness       out = blend(smooth(b3), b3, f3); smooth = the 3x3 kernel (1 1 1 / 1 5 1 / 1 1 1) / 13 with float32 weights, + 0.5,
 *                   truncated and clipped, on interior pixels; border pixels (and every pixel of an image with H < 3 or W < 3) are copies.
 */
#ifndef ONESHOTDET_HIP_COLOR_JITTER_H
#define ONESHOTDET_HIP_COLOR_JITTER_H

#include "oneshotdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define OSD_COLOR_JITTER_MAX_IMAGES 16 /* images per launch pair: a longer list is worked off in chunks of this many */

/* Bytes of `workspace` osd_color_jitter_batch needs for these images (64-bit partial sums for the Contrast step of coco.py:286-294, one
 * slot per workgroup of the first launch); 0 for n_images <= 0, a null array or a non-positive size. */
int64_t osd_color_jitter_workspace_bytes(int n_images, const int32_t* hs, const int32_t* ws);

/* The colour jitter of coco.py:286-294 on n_images dense uint8 RGB images: srcs_rgb_hwc[i] [hs[i], ws[i], 3] -> dsts_rgb_hwc[i], same
 * shape.  The three tables of pointers and sizes and `factors` are HOST arrays; factors[i*4 + 0..3] are image i's Color, Brightness,
 * Contrast and Sharpness factors as float32.  Two launches per OSD_COLOR_JITTER_MAX_IMAGES images: integer sums of L(b2), one slot per
 * workgroup, then everything else; the mean never leaves the device, there are no atomics and no memset, and the result does not depend
 * on what `workspace` (device memory, 8-byte aligned) held.  Argument checks, all before anything is launched: n_images < 0, a null table,
 * `factors` or workspace, a workspace that is not 8-byte aligned, per image a null pointer, a size < 1, a factor that is NaN, infinite or
 * negative, dsts[i] == srcs[i] (the Sharpness step reads a pixel's neighbours, so in place is refused): OSD_ERR_INVALID_ARG; an image of
 * 2^31 pixels or more: OSD_ERR_UNSUPPORTED.  n_images == 0 returns 0 and launches nothing. */
int osd_color_jitter_batch(int n_images, const uint8_t* const* srcs_rgb_hwc, const int32_t* hs, const int32_t* ws, const float* factors,
                           uint8_t* const* dsts_rgb_hwc, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ONESHOTDET_HIP_COLOR_JITTER_H */
