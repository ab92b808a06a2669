/* romp_hip_fit_clip.h -- temporal smoothness terms for the device fitter of romp_hip_fit.h, and the acceleration metric of a
 * tracked clip: an addition to the C ABI of romp_hip.h (same conventions, same ABI version 7; the symbols are listed in
 * romp_amd/lib.py FIT_CLIP_EXPORTS: a host that must run on an older library looks them up by name).  A step of a clip fit is
 *   smpl_forward -> romp_fit_reproject -> romp_fit_temporal (joints, cam; accumulate) -> smpl_backward
 *   -> romp_fit_temporal (betas, rotations; accumulate) -> romp_fit_adam : the step of romp_hip_fit.h plus two launches.
 * Both entries: int status plus romp_last_error(); every argument check before any device call; N == 0 returns ROMP_OK and
 * launches nothing; enqueued on `stream`, no host synchronisation; no atomics, every sum in a fixed order, so equal inputs give
 * equal bits; float64 arithmetic on the float32 inputs, rounded once when stored; each output element has one owning thread.
 *
 * LINKS.  A row is one person in one frame.  prev (N) and next (N), device int32, name the row of the same track in the
 * neighbouring frame, -1 for none.  A link (p -> n) exists iff  prev[n] == p,  0 <= p < N,  p != n  and  next[p] == n.  The
 * kernels test all four before they read row p; an entry that fails them is never used as an index, so no content of the tables
 * makes a kernel read outside its arrays.  Rows may come in any order.  A row reads its neighbours within two links: a NaN in a
 * row reaches those and no other chain. */
#ifndef ROMP_HIP_FIT_CLIP_H
#define ROMP_HIP_FIT_CLIP_H
#include "romp_hip_fit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ROMP_CLIP_MAX_SEGMENTS 4    /* linear blocks of one romp_fit_temporal call */

/* One linear block of romp_fit_temporal: a (N, cols) float32 tensor on the device, contiguous, and its gradient. */
typedef struct romp_clip_segment {
    const float* x;           /* (N, cols) */
    float* grad;              /* (N, cols): the gradient of  sum_n (w_vel Lvel[n] + w_acc Lacc[n])  with respect to x */
    const float* col_w;       /* (cols) per-column weights, or NULL = ones */
    int32_t cols;             /* >= 1 */
    float w_vel, w_acc;       /* >= 0 */
    float sigma_vel, sigma_acc;   /* <= 0: rho(e) = e; > 0: Geman-McClure sigma^2 e / (sigma^2 + e), as romp_fit_reproject */
    int32_t accumulate;       /* 0: every element of grad is written; != 0: every element becomes float(double(old) + g) */
} romp_clip_segment;

/* Velocity and acceleration terms of up to ROMP_CLIP_MAX_SEGMENTS tensors, and a first-order term on the joint rotations,
 * over the links of one clip, with their gradients, in one launch.
 *   segments_host: n_segments entries on the HOST, read before the call returns (NULL only with n_segments == 0).
 *   With pv = the row linked to n from behind, nx = the row n links to, both by the link rule above:
 *     v_n = x[n] - x[pv],              e_v(n) = sum_c col_w[c] v_n[c]^2,   Lvel[n] = rho(e_v(n))    needs (pv -> n)
 *     a_n = x[pv] - 2 x[n] + x[nx],    e_a(n) = sum_c col_w[c] a_n[c]^2,   Lacc[n] = rho(e_a(n))    needs (pv -> n), (n -> nx)
 *   A term without its links is exactly 0.  rho' = 1, or sigma^4 / (sigma^2 + e)^2.  The gradient of row n gathers the up to
 *   five terms that contain it:
 *     g[n,c] = 2 col_w[c] ( w_vel ( rho'(e_v(n)) v_n[c] - rho'(e_v(nx)) v_nx[c] )
 *                         + w_acc ( rho'(e_a(pv)) a_pv[c] - 2 rho'(e_a(n)) a_n[c] + rho'(e_a(nx)) a_nx[c] ) )
 *   The wave that owns (row, segment) recomputes its neighbours' e itself; nothing is read from another wave.
 *   poses (N,72) or NULL: the rotation block.  R_j(n) = the SMPL layer's Rodrigues matrix of columns 3j..3j+2
 *   (angle = |rv + 1e-8|, differentiable at zero),  e_r(n) = sum_j joint_w[j] |R_j(n) - R_j(pv)|_F^2  (= 4 sum_j w_j (1 - cos
 *   phi_j): no axis-angle wrap),  Lrot[n] = rho(e_r(n)) with sigma_rot; joint_w (24) or NULL = ones.  grad_poses (N,72) =
 *   w_rot * the gradient of sum_n Lrot[n] from the links (pv -> n) and (n -> nx); accumulate_poses as a segment's accumulate.
 *   term_w (N), device, or NULL = ones: the terms of row m (Lvel[m], Lacc[m], Lrot[m]) enter every objective above multiplied by
 *   term_w[m], so the gradients are those of  sum_m term_w[m] (...)[m]  (the backward of a node whose output is loss[m]).
 *   loss (N, L), L = 2 n_segments + (poses ? 1 : 0): Lvel, Lacc per segment, then Lrot; UNWEIGHTED.  loss_history or NULL:
 *   the same L numbers are also written to loss_history[(history_row * N + n) * L + 0..L-1].
 * One wave per (row, block), four waves to a workgroup; lanes stride over the columns, and over joints x 9 matrix elements
 * for the rotations.  Returns ROMP_OK, or ROMP_EINVAL before any device call (a NULL prev / next / loss, a NULL table with
 * n_segments > 0, n_segments outside 0..ROMP_CLIP_MAX_SEGMENTS, no block at all, a segment without x or grad, cols < 1, a
 * negative or NaN weight, poses without grad_poses, N < 0, history_row < 0). */
int  romp_fit_temporal(const romp_clip_segment* segments_host, int n_segments, const int32_t* prev, const int32_t* next, int N,
                       const float* term_w, const float* poses, const float* joint_w, float w_rot, float sigma_rot, float* grad_poses,
                       int accumulate_poses, float* loss, float* loss_history, int history_row, void* stream);

/* Acceleration and acceleration error of 3-D joints along the links (compute_accel / compute_error_accel,
 * evaluation_matrix.py:424-465), one launch.
 *   joints (N,J,3), gt (N,J,3) or NULL: device, float32, contiguous; vis (N) uint8 or NULL (= all visible), device.
 *   joint_inds_host as in romp_fit_reproject: K distinct indices < J on the HOST, NULL = 0..K-1; 1 <= K <= J <=
 *   ROMP_FIT_MAX_JOINTS.
 *   A row n is valid when the links (pv -> n) and (n -> nx) exist and, with vis, vis[pv], vis[n] and vis[nx] are all non-zero
 *   (the rows the reference's np.roll mask keeps).  There
 *     value[n] = mean_k | J[pv] - 2 J[n] + J[nx] |                                         without gt
 *     value[n] = mean_k | (J[pv] - 2 J[n] + J[nx]) - (G[pv] - 2 G[n] + G[nx]) |            with gt
 *   over the K picked joints, |.| the Euclidean norm, in the units of the joints, and valid[n] = 1.  Every other row:
 *   value[n] = 0, valid[n] = 0.
 * One wave per row, four to a workgroup, lanes over the joints.  Returns ROMP_OK, or ROMP_EINVAL before any device call (a
 * NULL joints / prev / next / value / valid, N < 0, K outside 1..J, J > ROMP_FIT_MAX_JOINTS, a repeated or out-of-range
 * index). */
int  romp_clip_accel(const float* joints, int N, int J, const float* gt, const uint8_t* vis, int K,
                     const int32_t* joint_inds_host, const int32_t* prev, const int32_t* next, float* value, uint8_t* valid,
                     void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ROMP_HIP_FIT_CLIP_H */
