/* romp_hip_eval.h -- benchmark scoring on the device: an addition to the C ABI of romp_hip.h (same conventions, same
 * status codes, same ABI version 7; the symbols are listed in romp_amd/lib.py EVAL_EXPORTS).  Every pointer is a device
 * pointer, everything is enqueued on `stream`, nothing synchronises, nothing allocates, no atomics: two calls on the
 * same inputs write identical bytes. */
#ifndef ROMP_HIP_EVAL_H
#define ROMP_HIP_EVAL_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ROMP_EVAL_NORM_FROBENIUS 0   /* sqrt of the sum of squares over the valid joints */
#define ROMP_EVAL_NORM_SPECTRAL  1   /* largest singular value of the (valid joints, 2) difference: what the reference's
                                        literal np.linalg.norm(d, 2) returns for a matrix */
#define ROMP_EVAL_ACC_TAIL 5         /* doubles after the (sum, count) pairs of a romp_eval_accumulate accumulator */

/* simple_romp/evaluation/RH_evaluation/matching.py match_2d_greedy(valid=None) for B images in one launch, one wave per
 * image.  pred_kp2d (Np,J,2), gt_kp2d (Ng,J,2) float32, gt_valid (Ng,J) uint8; image b owns the rows
 * [pred_offsets[b], pred_offsets[b+1]) and [gt_offsets[b], gt_offsets[b+1]) (offsets: B+1 int32 each, non-decreasing).
 *   error(p,g) = float32 norm (`norm`, above) of pred[p] - gt[g] over g's valid joints;
 *   repeat: take the unconsumed pair of least error (ties: lowest p*G + g) and consume it; IoU of the two boxes over ALL
 *   J joints with the reference's +1 widths, in float32; both free and IoU >= iou_thresh: a match; else IoU < iou_thresh:
 *   one false-positive event, nothing assigned; else the next pair;
 *   until every g is assigned, or matches + false-positive events reach the image's number of preds, or every pair is
 *   consumed (the reference spins there).
 * gt_of_pred (Np) / pred_of_gt (Ng) int32: GLOBAL row numbers, -1 = false positive / miss; every row of every image is
 * written.  max_pred / max_gt: the caller's caps on one image's counts; the pair table (max_pred*max_gt errors and the
 * boxes) lives in LDS and one that 64 KiB cannot hold is ROMP_EINVAL.  An image whose counts exceed the caps is never
 * truncated: all its rows are -1 and over_cap[b] (B int32, may be null) is 1, else 0. */
int  romp_eval_match2d(const float* pred_kp2d, const int32_t* pred_offsets, const float* gt_kp2d, const uint8_t* gt_valid,
                       const int32_t* gt_offsets, int B, int J, int max_pred, int max_gt, float iou_thresh, int norm,
                       int32_t* gt_of_pred, int32_t* pred_of_gt, int32_t* over_cap, void* stream);

/* Per ground-truth row g with p = pred_of_gt[g] (null: p = g), over pred (Np,P,3) and target (Ng,P,3) float32, one
 * workgroup per row, moments / decomposition / error sums in float64:
 *   mpjpe[g]     compute_mpjpe(sample_wise=True): mean distance after subtracting from each side its own mean over
 *                align_inds (n_align int32, null/0: no alignment); with vis (Ng,P) uint8: sum(err*vis) / sum(vis)
 *   mpjpe_all[g] sum(err*vis) / P (vis null: equals mpjpe): eval_cmu_panoptic.py's per-person figure
 *   pa_mpjpe[g]  batch_compute_similarity_transform_torch fitted on the points with point_mask[i] != 0 (P uint8, null:
 *                all), then the mean distance over those points
 *   sRt (Ng,13)  scale, R row-major, t of   aligned = scale * R x + t
 *   aligned (Ng,P,3)  the transform applied to ALL P points of pred[p]
 * Every output may be null.  p outside [0,Np) (-1: a miss) gives NaN in every output of the row.  K of rank 2 or 1
 * (planar, collinear, P = 2) is decomposed without dividing by a vanishing singular value; var1 = 0 gives a non-finite
 * row as in the reference, and so does a point_mask that selects no point.  pred[p] == target[g] bit for bit gives scale 1,
 * R = I, t = 0 and errors of exactly 0.  P < 2: ROMP_EINVAL. */
int  romp_eval_points(const float* pred, int Np, const float* target, int Ng, int P, const int32_t* pred_of_gt,
                      const int32_t* align_inds, int n_align, const uint8_t* vis, const uint8_t* point_mask,
                      float* mpjpe, float* mpjpe_all, float* pa_mpjpe, float* sRt, float* aligned, void* stream);

/* Folds one call's rows into the caller's float64 accumulator of 2*n_metrics + ROMP_EVAL_ACC_TAIL doubles (the caller
 * zeroes it once): per metric k of metrics (n_metrics,Ng) float32  acc[2k] += sum of the finite rows, acc[2k+1] += their
 * number; then += misses (pred_of_gt < 0), false positives (gt_of_pred < 0), Ng, Np, images over the cap (over_cap (B),
 * may be null).  One workgroup, a fixed order. */
int  romp_eval_accumulate(const float* metrics, int n_metrics, int Ng, const int32_t* pred_of_gt, const int32_t* gt_of_pred,
                          int Np, const int32_t* over_cap, int B, double* acc, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ROMP_HIP_EVAL_H */
