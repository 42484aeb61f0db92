/*
 * oneshotdet_hip_pred_bwd.h — C-ABI of liboneshotdet_hip.so, eighth part: the backward pass of an FCOS prediction conv
 * (rpn/fcos/fcos.py:50-61,91-97: cls_logits + centerness, bbox_pred) as ONE launch over all FPN levels.  The gathered matrix
 * G [pixels][64] of osd_pred_dy_gather (oneshotdet_hip.h) is built tile by tile in LDS and never reaches memory: the launch reads x
 * once and writes dx once.  Same conventions as oneshotdet_hip.h (raw device pointers, asynchronous on `stream`, 0 = OK / negative =
 * OSD_ERR_*).  The ABI version is unchanged.
 */
#ifndef ONESHOTDET_HIP_PRED_BWD_H
#define ONESHOTDET_HIP_PRED_BWD_H

#include "oneshotdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `flags` of osd_conv2d_pred_bwd: both gradients, the data gradient only, the weight + bias gradient only */
#define OSD_PRED_BWD_BOTH 0
#define OSD_PRED_BWD_DGRAD 1
#define OSD_PRED_BWD_WGRAD 2

/* Bytes of the workspace osd_conv2d_pred_bwd needs for these levels (the per-workgroup partial weight gradients: 9 * cout rows of
 * cin fp32 values per workgroup, no initialisation needed).  0 for arguments the launch refuses. */
int64_t osd_pred_bwd_workspace_bytes(int n_seg, const int32_t* ns, const int32_t* hs, const int32_t* ws, int cin, int cout);

/* Backward of a 3x3 / stride 1 / pad 1 conv with cout <= 4 and cin % 256 == 0 in bf16 over n_seg <= 6 levels (desc: dtype, cin,
 * cout, r, s, stride, pad, out_stride = channels stored per dy pixel, a multiple of 4; n / h / w are taken from ns / hs / ws, HOST
 * arrays):
 *   xs[l]  [ns[l]][hs[l]][ws[l]][cin]         the conv's input (dense NHWC, 16-byte aligned)
 *   dys[l] [ns[l]][hs[l]][ws[l]][out_stride]  the gradient of its output (8-byte aligned; channels >= cout are ignored)
 *   wd_packed [cin][64]                       the weights as osd_pred_dgrad_pack writes them
 *   dx [sum_l ns hs ws][cin]                  WRITTEN: the data gradient, the levels one after the other (rows in G's order), rounded
 *                                             once from the fp32 sum over the 64 columns of G
 *   dw [cout][3][3][cin] fp32, db [cout] fp32 ADDED TO (db may be null): the weight and bias gradient summed over the levels
 * The weight gradient is accumulated per workgroup in registers over all its pixels, stored to `workspace` and added into dw / db
 * by a second launch in workgroup order: no atomics, the same bits every run.  flags = OSD_PRED_BWD_DGRAD ignores xs, dw, db and
 * workspace (they may be null); OSD_PRED_BWD_WGRAD ignores wd_packed and dx.  Either half computes the bits the fused launch does.
 * OSD_ERR_UNSUPPORTED: fp32, another geometry, cout > 4, cin % 256 != 0, out_stride % 4 != 0.  OSD_ERR_INVALID_ARG: n_seg outside
 * 1..6, a null or misaligned pointer the flags need, an empty level, bad flags or dtype.  Nothing is launched then. */
int osd_conv2d_pred_bwd(const osd_conv_desc* desc, int n_seg, const void* const* xs, const void* const* dys, const int32_t* ns,
                        const int32_t* hs, const int32_t* ws, const void* wd_packed, void* dx, float* dw, float* db, void* workspace,
                        int flags, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ONESHOTDET_HIP_PRED_BWD_H */
