/*
 * oneshotdet_hip_solver.h — C-ABI of liboneshotdet_hip.so, fifth part: the optimiser update with its learning rate read from device
 * memory, so that a captured update (hipGraph) follows a learning-rate schedule (solver/lr_scheduler.py:10-52, WarmupMultiStepLR)
 * without being captured again.  Same conventions as oneshotdet_hip.h (raw device pointers, asynchronous on `stream`, 0 = OK /
 * negative = OSD_ERR_*); paths relative to the reference's maskrcnn_benchmark/.  The ABI version is unchanged.
 *
 * The solver block: 8 bytes of device memory, 8-byte aligned,
 *   struct { float lr; int32_t first_step; }
 * lr is the rate of the weight group (a table entry's lr_mult makes the bias group's, solver/build.py:8-26); first_step != 0: the
 * momentum buffer is not read (buf = g), as with the by-value entries' first_step.
 */
#ifndef ONESHOTDET_HIP_SOLVER_H
#define ONESHOTDET_HIP_SOLVER_H

#include "oneshotdet_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Write the solver block: one workgroup, one lane, two plain stores.  Stream-ordered like any launch — the values travel as
 * kernel arguments, so the caller keeps no staging buffer alive — and meant to run BETWEEN graph launches, never inside a captured
 * graph (its arguments would be baked in like the by-value entries').  Exactly the block's 8 bytes are written.
 * OSD_ERR_INVALID_ARG for a null block or one that is not 8-byte aligned; nothing is launched then. */
int osd_solver_set(void* block, float lr, int first_step, void* stream);

/* osd_sgd_momentum_multi with (lr, first_step) read from the solver block: every workgroup loads the block once (a wave-uniform
 * load) and then runs the by-value entry's update — the same code, so the same bits for the same rate.  Arguments as
 * osd_sgd_momentum_multi's, `float lr, ..., int first_step` replaced by `const void* solver_block`.  OSD_ERR_INVALID_ARG for a null
 * or misaligned block; nothing is launched then. */
int osd_sgd_momentum_multi_dev(const void* table, const int32_t* block_entry, int n_blocks, float* params, const float* grads,
                               float* momentum_buf, const void* solver_block, float momentum, void* stream);

/* osd_sgd_momentum_pack_multi with (lr, first_step) read from the solver block, as above. */
int osd_sgd_momentum_pack_multi_dev(const void* table, const int32_t* block_entry, int n_blocks, float* params, float* grads,
                                    float* momentum_buf, const float* scales, void* packed, int dtype,
                                    const void* solver_block, float momentum, int zero_grads, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ONESHOTDET_HIP_SOLVER_H */
