/* romp_hip_fit.h -- fitting the SMPL layer to 2-D keypoints with libromp_hip.so: an addition to the C ABI of romp_hip.h (same
 * conventions, same ABI version 7; the symbols are listed in romp_amd/lib.py FIT_EXPORTS: a host that must run on an older
 * library looks them up by name).  One step of a fit is  smpl_forward -> romp_fit_reproject -> smpl_backward (grad_verts =
 * NULL) -> romp_fit_adam : the layer's own launches plus two. */
#ifndef ROMP_HIP_FIT_H
#define ROMP_HIP_FIT_H
#include "romp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ROMP_FIT_MAX_JOINTS   256   /* J of romp_fit_reproject (the index table travels with the launch) */
#define ROMP_FIT_MAX_SEGMENTS 8     /* parameter tensors of one romp_fit_adam call */

/* Reprojection loss of K picked joints against 2-D keypoints, and its gradients, in one launch.
 *   joints (N,J,3), cam (N,3), targets (N,K,2), conf (N,K) or NULL (= ones): device, float32, contiguous.
 *   joint_inds_host: K distinct indices < J on the HOST (read before the call returns); keypoint k belongs to joint
 *   joint_inds_host[k]; NULL stands for 0..K-1.  1 <= K <= J <= ROMP_FIT_MAX_JOINTS.
 *   mode 0: the weak-perspective camera of batch_orth_proj, cam = (s, c1, c2):  u = s x + c1,  v = s y + c2.
 *   mode 1: BEV's perspective_projection as romp_bev_project_verts computes it, cam = cam_trans:  p = X + cam,
 *           u = p.x / (p.z + 1e-6) * focal / half,  v likewise (443.4 and 256 in BEV); no clamp of the depth.
 *           focal and half are ignored in mode 0.
 *   r = (u, v) - target,  e = |r|^2,  term = conf^2 rho(e);  rho(e) = e for sigma <= 0, else Geman-McClure
 *   sigma^2 e / (sigma^2 + e).  The distance is SQUARED, unlike the reference's batch_kp_2d_l2_loss
 *   (keypoints_loss.py:37), whose unsquared norm has no gradient at a perfect fit.
 *   A keypoint is visible when conf > 0 and both target coordinates are > -1.99 (keypoints_loss.py:24; a NaN fails the
 *   comparison, so a NaN target or conf is invisible); an invisible keypoint contributes nothing.
 *   loss[n] = sum over visible terms / (n_visible + 1e-4), the reference's normaliser (keypoints_loss.py:38).
 * Outputs (device, float32): loss (N); grad_joints (N,J,3) = d loss[n] / d joints[n], every element written (zeros at joints
 * not picked and at invisible keypoints); grad_cam (N,3) = d loss[n] / d cam[n]; loss_history or NULL: the loss is also
 * written to loss_history[history_row * N + n], so a loop keeps its curve on the device.
 * One wave per person (four to a workgroup), lanes over the joints, float64 arithmetic on the float32 inputs, the sums
 * reduced across lanes in a fixed order: no atomics, equal inputs give equal bits.  Enqueued on `stream`, no host
 * synchronisation.  Returns ROMP_OK, or ROMP_EINVAL with romp_last_error() set before any device call (a NULL joints / cam /
 * targets / loss / grad_joints / grad_cam, N < 0, K < 1, K > J, J > ROMP_FIT_MAX_JOINTS, a repeated or out-of-range index,
 * a mode other than 0 / 1, history_row < 0).  N == 0: ROMP_OK, nothing launched. */
int  romp_fit_reproject(const float* joints, int N, int J, const float* cam, const float* targets, const float* conf, int K,
                        const int32_t* joint_inds_host, int mode, float focal, float half, float sigma,
                        float* loss, float* grad_joints, float* grad_cam, float* loss_history, int history_row,
                        void* stream);

/* One parameter tensor of a fit: (rows, cols) float32 on the device, contiguous. */
typedef struct romp_fit_segment {
    float* param;             /* updated in place */
    const float* grad;        /* gradient of the data term */
    float* m;                 /* Adam's first moment, updated in place (zeros before step 1) */
    float* v;                 /* Adam's second moment, likewise */
    const float* prior_ref;   /* (rows, cols) or NULL = zeros */
    const float* prior_w;     /* (cols) per-column weights of the L2 prior, or NULL = no prior */
    int32_t rows, cols;
} romp_fit_segment;

/* One Adam step for all parameter tensors of a fit in one launch.  For every element of every segment
 *   g = grad + 2 prior_w[c] (param - prior_ref)           (the gradient of  sum_c prior_w[c] (param - prior_ref)^2)
 *   m = beta1 m + (1 - beta1) g,   v = beta2 v + (1 - beta2) g^2
 *   param -= (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
 * which is torch.optim.Adam (amsgrad off, no weight decay) with the prior's gradient added; `step` counts from 1.
 * segments_host: n_segments entries on the HOST, read before the call returns.  One thread per element, float64 arithmetic
 * on the float32 state.  Enqueued on `stream`, no host synchronisation, no atomics.  Returns ROMP_OK, or ROMP_EINVAL before
 * any device call (NULL table, n_segments outside 1..ROMP_FIT_MAX_SEGMENTS, a NULL param / grad / m / v, rows < 0,
 * cols < 1, step < 1).  No element at all: ROMP_OK, nothing launched. */
int  romp_fit_adam(const romp_fit_segment* segments_host, int n_segments, float lr, float beta1, float beta2, float eps,
                   int step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ROMP_HIP_FIT_H */
