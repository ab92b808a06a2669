/* romp_hip_fit_scene.h -- scene terms for the device fitter of romp_hip_fit.h: the depth order of the persons of one image and
 * their interpenetration, the cross-person counterpart of romp_hip_fit_clip.h.  An addition to the C ABI of romp_hip.h (same
 * conventions, same ABI version 7; the symbol is listed in romp_amd/lib.py FIT_SCENE_EXPORTS: a host that must run on an older
 * library looks it up by name).  A step of a scene fit is
 *   smpl_forward -> romp_fit_reproject -> romp_fit_scene (joints, cam; accumulate) -> smpl_backward -> romp_fit_adam :
 * the step of romp_hip_fit.h plus one launch.
 * int status plus romp_last_error(); every argument check before any device call; N == 0 returns ROMP_OK and launches nothing;
 * enqueued on `stream`, no host synchronisation; no atomics, every sum in a fixed order, so equal inputs give equal bits;
 * float64 arithmetic on the float32 inputs, rounded once when stored; each output element has one owning thread.
 *
 * SCENES.  A row is one person in one image.  offsets (N + 1) and members (N), device int32, group the rows by image: scene g
 * is members[offsets[g] .. offsets[g + 1] - 1], in that order (romp_amd.scene.scene_groups builds both on the device).  A
 * member entry is used only after  0 <= offsets[g] <= offsets[g + 1] <= N  and  0 <= member < N  have been tested; an entry that
 * fails is skipped and never used as an index, so no content of the tables makes the kernel read outside its arrays.  The
 * scene of row n is the first valid group with an entry equal to n, at the first such position; its partners are the other
 * valid entries of that group that are not n.  A row in no group has no partner.  A row reads the rows of its own scene: a
 * NaN in a row reaches that scene and no other. */
#ifndef ROMP_HIP_FIT_SCENE_H
#define ROMP_HIP_FIT_SCENE_H
#include "romp_hip_fit.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ROMP_SCENE_MAX_SPHERES 64   /* entries of the sphere table of one romp_fit_scene call */
#define ROMP_SCENE_PIECEWISE 0      /* depth_loss_type 'Piecewise' of the reference */
#define ROMP_SCENE_LOG       1      /* 'Log' */

/* One proxy sphere of the body: centre (1 - a) J[p] + a J[q] in the frame of the joints, radius r > 0 in their units. */
typedef struct romp_scene_sphere {
    int32_t p, q;             /* joint indices, 0 .. J-1; p == q puts the sphere on a joint */
    float a, r;               /* finite; r > 0 */
} romp_scene_sphere;

/* The depth-order term and the collision term of every scene, with their gradients, in one launch.
 *   joints (N,J,3), cam (N,3): device, float32, contiguous.  The translation of row n:
 *     camera_mode 1 (perspective): t = cam (BEV's cam_trans);
 *     camera_mode 0 (weak), cam = (s, c1, c2): t = 2 (c1 / s, c2 / s, 1 / s)  (convert_cam_to_3d_trans, utils.py:303-307).
 *   Both terms' gradients are chained back to cam through this map.
 *   DEPTH ORDER (relative_depth_loss, loss_funcs/relative_loss.py:46-99, on z = t.z).  depth_ids (N) device int32, a negative
 *   entry = unlabelled; NULL: the term is off and loss[n,0] = 0.  For every pair i < j (positions in member order) of labelled
 *   rows of a scene, d = z_j - z_i and k = id_j - id_i:
 *     k == 0: d^2, always active;   k < 0: softplus(d), active iff d - k thresh > 0;   k > 0: softplus(-d), active iff
 *     d - k thresh < 0 (both strict);  kind ROMP_SCENE_LOG: every pair is active.  softplus(x) = max(x, 0) + log1p(exp(-|x|)).
 *   A = the number of active pairs of the scene.  loss[n,0] = (1 / 2A) sum of the active pairs that contain n; with A == 0
 *   every row of the scene gets 0 and no gradient.  The rows of a scene sum to the reference's mean over the image, and the
 *   sum over all rows divided by the number of scenes with A > 0 is the reference's scalar.  A is constant under the gradient.
 *   COLLISION (the sphere proxies of SMPLify, Bogo et al. 2016, eq. 7, between DIFFERENT persons of a scene).  spheres_host: S
 *   entries on the HOST, read and checked before the call returns; they travel with the launch as kernel arguments, so the
 *   caller keeps no device copy.  S == 0: the term is off, loss[n,1] = 0, joints and grad_joints are not touched (may be NULL).
 *   Sphere s of row n has the centre  c = (1 - a) J[n,p] + a J[n,q] + t_n  and  sigma = r / 3 * radius_scale[n]
 *   (radius_scale (N) device or NULL = ones).
 *     loss[n,1] = 1/2 sum_{m != n in the scene} sum_{s,u} exp(-|c_{n,s} - c_{m,u}|^2 / (sigma_{n,s}^2 + sigma_{m,u}^2)),
 *   so the rows of a scene sum to its energy; a row alone in its scene, or in none, gets exactly 0.
 *   term_w (N) device, or NULL = ones: the gradients are those of
 *     w_depth sum_m term_w[m] loss[m,0] + w_col sum_m term_w[m] loss[m,1]
 *   (the backward of a node whose outputs are the losses).  The depth part goes onto grad_cam, the collision part onto
 *   grad_joints (N,J,3), through the affine centres, and onto grad_cam.  accumulate_joints / accumulate_cam: 0: every element
 *   of the gradient is written; != 0: every element becomes float(double(old) + g).
 *   loss (N,2) or NULL: (depth, collision), UNWEIGHTED.  loss_history or NULL: the same two numbers are also written to
 *   loss_history[(history_row * N + n) * 2 + 0..1].
 * One workgroup of 256 threads per row.  The row finds its scene by a scan of the tables; its threads stride over the pairs
 * of the scene for A and over its partners for its own depth sum; in the collision term a lane owns one of the row's spheres,
 * the partners are split over the four waves and combined in LDS in wave order, and one thread per joint gathers the
 * spheres on it in table order.  Every row recomputes its own side of a pair; nothing is read from another workgroup.
 * Returns ROMP_OK, or ROMP_EINVAL before any device call (a NULL cam / offsets / members / grad_cam; S > 0 with a NULL
 * joints / grad_joints / spheres_host; neither term on (depth_ids NULL and S == 0); a negative or NaN weight or threshold; S
 * outside 0..ROMP_SCENE_MAX_SPHERES; a sphere joint index outside 0..J-1, a non-finite a or r, r <= 0; J < 1 or
 * J > ROMP_FIT_MAX_JOINTS with S > 0; kind or camera_mode outside {0, 1}; N < 0; history_row < 0; both weights zero and no
 * loss output). */
int  romp_fit_scene(const float* joints, int N, int J, const float* cam, int camera_mode, const int32_t* offsets,
                    const int32_t* members, const int32_t* depth_ids, float w_depth, float dist_thresh, int kind,
                    const romp_scene_sphere* spheres_host, int S, const float* radius_scale, float w_col, const float* term_w,
                    float* grad_joints, int accumulate_joints, float* grad_cam, int accumulate_cam, float* loss,
                    float* loss_history, int history_row, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ROMP_HIP_FIT_SCENE_H */
