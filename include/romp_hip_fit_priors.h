/* romp_hip_fit_priors.h -- SMPLify's pose priors and 3-D joint targets for the device fitter of romp_hip_fit.h: an addition to
 * the C ABI of romp_hip.h (same conventions, same ABI version 7; the symbols are listed in romp_amd/lib.py FIT_PRIOR_EXPORTS: a
 * host that must run on an older library looks them up by name).  A step of a fit with every term on is
 *   smpl_forward -> romp_fit_reproject -> romp_fit_joints3d (accumulate) -> smpl_backward -> romp_fit_pose_prior (accumulate)
 *   -> romp_fit_adam : the step of romp_hip_fit.h plus two launches.
 * Both entries: int status plus romp_last_error(); every argument check before any device call; N == 0 returns ROMP_OK and
 * launches nothing; enqueued on `stream`, no host synchronisation; no atomics, every sum in a fixed order, so equal inputs give
 * equal bits; float64 arithmetic on the float32 inputs, rounded once when stored.  The arithmetic of a person does not depend
 * on the other persons: a NaN in one person's inputs stays in that person's outputs. */
#ifndef ROMP_HIP_FIT_PRIORS_H
#define ROMP_HIP_FIT_PRIORS_H
#include "romp_hip_fit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ROMP_FIT_MAX_GAUSSIANS 16   /* M of romp_fit_pose_prior */
#define ROMP_FIT_MAX_POSE_DIM  69   /* D of romp_fit_pose_prior: the body pose without the global orientation */

/* The max-mixture pose prior (MaxMixturePrior.merged_log_likelihood, prior_loss.py:232-247) and the joint-angle prior
 * (angle_prior, prior_loss.py:106-111) of a 72-column pose, with their gradient, in one launch.
 *   poses (N,72), means (M,D), precisions (M,D,D), offsets (M): device, float32, contiguous.  1 <= D <= 69,
 *   0 <= M <= ROMP_FIT_MAX_GAUSSIANS.  Every precisions[m] MUST BE SYMMETRIC (the kernel reads P[k][i] where the formula has
 *   P[i][k], so that the lanes of a wave read one contiguous row); an unsymmetric matrix gives the result of its transpose
 *   in the gradient.
 *   x = poses[n, 3:3+D],  d_m = x - means[m],  q_m = 0.5 d_m^T P_m d_m + offsets[m]   (offsets[m] = -log(nll_weights[m]),
 *   prior_loss.py:207-214, 240).  loss[n,0] = min_m q_m;  best[n] (or NULL) = the lowest m that attains it.
 *   M == 0 or means == NULL: the mixture is off, loss[n,0] = 0, best[n] = -1.  Otherwise precisions and offsets are required.
 *   loss[n,1] = sum over (column, sign) = (55,+1), (58,-1), (12,-1), (15,-1) of exp(2 s theta): angle_prior's exp(s theta)^2,
 *   its indices moved to the 72-column vector (left elbow, right elbow, left knee, right knee).
 *   loss is UNWEIGHTED; loss_history or NULL: the same two numbers are also written to loss_history[(history_row * N + n) * 2
 *   + 0..1].
 *   grad_poses (N,72): g = w_gmm * P_best d_best on columns 3..3+D-1, plus w_angle * 2 s exp(2 s theta) on the four angle
 *   columns, zero elsewhere.  accumulate == 0: every element is written (zeros where no term acts); accumulate != 0: every
 *   element becomes float(double(old) + g).  Each element has exactly one owning thread.
 * One workgroup of eight waves per person, one mixture component per wave and round; the winner is chosen across the waves
 * through the LDS and its wave stores the gradient.  Returns ROMP_OK, or ROMP_EINVAL with romp_last_error() set before any
 * device call (a NULL poses / loss / grad_poses, means without precisions or offsets, N < 0, D outside 1..69, M outside
 * 0..ROMP_FIT_MAX_GAUSSIANS, history_row < 0). */
int  romp_fit_pose_prior(const float* poses, int N, const float* means, const float* precisions, const float* offsets, int M,
                         int D, float w_gmm, float w_angle, float* loss, int32_t* best, float* grad_poses, int accumulate,
                         float* loss_history, int history_row, void* stream);

/* The distance of K picked joints to 3-D targets under the rule of calc_mpjpe / align_by_parts (keypoints_loss.py:64-82), and
 * its gradients, in one launch.
 *   joints (N,J,3), trans (N,3) or NULL, targets (N,K,3), conf (N,K) or NULL (= ones): device, float32, contiguous.
 *   joint_inds_host as in romp_fit_reproject: K distinct indices < J on the HOST, NULL = 0..K-1; 1 <= K <= J <=
 *   ROMP_FIT_MAX_JOINTS.  P_k = joints[n, ind_k] (+ trans[n]),  T_k = targets[n,k].
 *   Keypoint k is visible when conf > 0, T_k.x != -2 (keypoints_loss.py:71) and no coordinate of T_k is NaN.
 *   n_align > 0: align_inds_host holds n_align distinct indices into the K SELECTED keypoints (the convention of
 *   evaluation.eval_points(align_inds=...)); the mean of the prediction over them is subtracted from every prediction, and
 *   the mean of the targets from every target (align_by_parts).  Unlike the reference, which would average the -2 mark in:
 *   if any alignment keypoint is invisible the person's term is zero, loss 0 and no gradient.
 *   r_k = the difference of the (aligned) prediction and target, e = |r_k|^2, term = conf^2 rho(e), rho as in
 *   romp_fit_reproject (e, or Geman-McClure sigma^2 e / (sigma^2 + e) for sigma > 0).
 *   loss[n] = sum over visible terms / (n_visible + 1e-4), UNWEIGHTED; also written to loss_history[history_row * N + n].
 *   grad_joints (N,J,3) = weight * d loss[n] / d joints[n]: with g_k the gradient with respect to the aligned prediction of
 *   keypoint k, joint j gets g_j - [j in A] (1/|A|) sum_k g_k; zeros at joints not picked and at invisible keypoints.
 *   grad_trans (N,3) = weight * the sum of the joint gradients; exact zeros when n_align > 0.  NULL iff trans is NULL.
 *   accumulate as in romp_fit_pose_prior, for both gradient outputs.
 * One wave per person (four to a workgroup), lanes over the joints.  Returns ROMP_OK, or ROMP_EINVAL before any device call
 * (a NULL joints / targets / loss / grad_joints, grad_trans without trans or trans without grad_trans, N < 0, K outside 1..J,
 * J > ROMP_FIT_MAX_JOINTS, a repeated or out-of-range index in either table, n_align outside 0..K, n_align > 0 without a
 * table, history_row < 0). */
int  romp_fit_joints3d(const float* joints, int N, int J, const float* trans, const float* targets, const float* conf, int K,
                       const int32_t* joint_inds_host, const int32_t* align_inds_host, int n_align, float sigma, float weight,
                       float* loss, float* grad_joints, float* grad_trans, int accumulate, float* loss_history, int history_row,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ROMP_HIP_FIT_PRIORS_H */
