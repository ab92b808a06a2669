/* romp_hip_smpl_grad.h -- the backward of the SMPL layer of libromp_hip.so: an addition to the C ABI of romp_hip.h (same
 * conventions, same ABI version 7; the symbol is listed in romp_amd/lib.py SMPL_GRAD_EXPORTS: a host that must run on an
 * older library looks it up by name). */
#ifndef ROMP_HIP_SMPL_GRAD_H
#define ROMP_HIP_SMPL_GRAD_H
#include "romp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Vector-Jacobian product of smpl_forward(ctx, betas, n_betas, thetas, N, root_align, verts, joints):
 *   grad_betas[n]  = d( sum grad_verts . verts + sum grad_joints . joints ) / d betas[n]      (N, n_betas)
 *   grad_thetas[n] = the same with respect to thetas[n]                                          (N, 72)
 * betas / thetas: the inputs of the forward (device, float32).  grad_verts (N,6890,3) and grad_joints (N,71,3): device,
 * float32, contiguous; NULL stands for zeros.  grad_betas / grad_thetas: device outputs, every element written; either
 * may be NULL (not wanted).  The Rodrigues formula differentiated is the forward's own, the 1e-8 added to every component
 * of the axis-angle vector included: the gradient is finite at thetas = 0.
 * The call recomputes what it needs from betas / thetas: it reads nothing an earlier smpl_forward left in the context,
 * so forwards of other batches may run on the context between a forward and its backward.  It keeps its own grow-only
 * scratch in the context (about 220 KB per person; freed by smpl_ctx_destroy).  Growing it frees and reallocates, which
 * waits for the device like smpl_forward's own growth; calls on one context must not overlap in time.
 * All work is enqueued on `stream`; no host synchronisation when the scratch is large enough.  No float atomics: every
 * reduction is a sum of per-tile partials in a fixed order, so equal inputs give equal bits.
 * Returns ROMP_OK or a status of romp_hip.h with romp_last_error() set (NULL ctx / betas / thetas, N < 0, n_betas not the
 * context's: ROMP_EINVAL before any device call).  N == 0: ROMP_OK, nothing done. */
int  smpl_backward(smpl_ctx* ctx, const float* betas, int n_betas, const float* thetas, int N, int root_align,
                   const float* grad_verts, const float* grad_joints, float* grad_betas, float* grad_thetas,
                   void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ROMP_HIP_SMPL_GRAD_H */
