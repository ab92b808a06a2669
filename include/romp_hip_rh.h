/* romp_hip_rh.h -- the Relative Human benchmark scored on the device: an addition to the C ABI of romp_hip.h next to
 * romp_hip_eval.h (same conventions, same status codes, same ABI version 7; the symbols are listed in romp_amd/lib.py
 * RH_EXPORTS).  Every pointer is a device pointer, everything is enqueued on `stream`, nothing synchronises, nothing
 * allocates, no atomics: all sums are integers (or exact, below) folded in a fixed order, so two calls on the same inputs
 * write identical bytes.  A call that returns ROMP_EINVAL has launched nothing and written nothing; romp_last_error() says
 * why. */
#ifndef ROMP_HIP_RH_H
#define ROMP_HIP_RH_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* One image's row of int32 counts written by romp_rh_score. */
#define ROMP_RH_EQ_PAIRS     0   /* pairs of equal depth id */
#define ROMP_RH_EQ_CORRECT   1   /*   ... with |dist| < dr_thresh */
#define ROMP_RH_ORD_PAIRS    2   /* pairs of different depth id (the reference's "close" and "far" together) */
#define ROMP_RH_ORD_CORRECT  3   /*   ... with dist beyond dr_thresh on the side of the id difference */
#define ROMP_RH_AGE_PAIRS    4   /* + 2*a, a = 0..3: pairs with at least one member of age a */
#define ROMP_RH_AGE_CORRECT  5   /* + 2*a: the correct ones among them */
#define ROMP_RH_MISSED      12   /* ground-truth rows without a prediction */
#define ROMP_RH_MISSED_AGE  13   /* + a, a = 0..3: those of age a */
#define ROMP_RH_MATCHED     17   /* ground-truth rows with a prediction */
#define ROMP_RH_UNSCORED    18   /* matched rows with fewer than 2 visible joints (pckh == -1) */
#define ROMP_RH_OVER_CAP    19   /* 1: the image holds more than max_gt rows; every other count of the row is then 0 */
#define ROMP_RH_COUNTS      20
/* The accumulator of romp_rh_accumulate: the ROMP_RH_COUNTS columns summed over the images, then */
#define ROMP_RH_ACC_PCKH_SUM 20  /* sum of pckh over the rows with pckh >= 0 */
#define ROMP_RH_ACC_N_GT     21
#define ROMP_RH_ACC_N_PRED   22
#define ROMP_RH_ACC_FALSE_POS 23 /* predictions without a ground-truth row (gt_of_pred < 0) */
#define ROMP_RH_ACC          24

/* simple_romp/evaluation/RH_evaluation/evaluation.py _calc_matched_PCKh_ (:71-88), _calc_relative_depth_error_weak_ (:37-69)
 * and the counting of get_results (:101-123) for the B images of a call in one launch, one wave per image.
 * pred_kp2d (Np,J,2) float32, pred_depth (Np) float32, gt_kp2d (Ng,J,2) float32 (a missing joint is (-2,-2)), gt_depth_id
 * (Ng) int32 (-1: none), gt_age (Ng) int32, pred_of_gt (Ng) int32 as romp_eval_match2d writes it (global row of pred, < 0
 * or >= Np: a miss); image b owns the rows [gt_offsets[b], gt_offsets[b+1]) (B+1 int32, clamped to [0, Ng]).
 * Per ground-truth row g of an image (rows outside every image are not written):
 *   a joint is visible when both of ITS GROUND-TRUTH COORDINATES are > -1; scale = the diagonal of the visible joints' box;
 *   correct = the visible joints with |pred - gt| / scale < pck_thresh, all in float32 (scale 0: inf or NaN, not correct);
 *   pckh[g] (Ng float32) = float32(correct) / float32(visible); -1 with fewer than 2 visible joints; NaN for a miss;
 *   correct_visible[g] (Ng,2 int32) = (correct, visible); (0, visible) with fewer than 2; (0, 0) for a miss.
 * Per image: counts[b] (B, ROMP_RH_COUNTS int32), above.  The pairs are the unordered pairs (i < j, ascending row order)
 * of the matched rows with gt_depth_id != -1: dist = pred_depth[p_j] - pred_depth[p_i] in float32, did = id_j - id_i;
 * did == 0: correct when |dist| < dr_thresh; did < 0: when dist < -dr_thresh; did > 0: when dist > dr_thresh.  An age
 * outside 0..3 counts in the totals only.  The compacted rows live in LDS: max_gt is the caller's cap on one image's rows
 * (1..4096); an image over it is never truncated: its rows are NaN / (0,0), its counts 0 and ROMP_RH_OVER_CAP 1.
 * pckh and correct_visible may be null; Np = 0 or Ng = 0 need no pointers to those rows.
 * ROMP_EINVAL: B <= 0, J <= 0, Np < 0, Ng < 0, max_gt outside 1..4096, a null gt_offsets or counts, a null input that has rows. */
int  romp_rh_score(const float* pred_kp2d, const float* pred_depth, int Np, const float* gt_kp2d, const int32_t* gt_depth_id,
                   const int32_t* gt_age, const int32_t* pred_of_gt, int Ng, const int32_t* gt_offsets, int B, int J, int max_gt,
                   float dr_thresh, float pck_thresh, float* pckh, int32_t* correct_visible, int32_t* counts, void* stream);

/* Folds one call into the caller's accumulator of ROMP_RH_ACC doubles (the caller zeroes it once): the columns of counts
 * (B, ROMP_RH_COUNTS), the sum of pckh (Ng, may be null when Ng = 0) over the rows >= 0, Ng, Np, and the rows of gt_of_pred
 * (Np int32, from romp_eval_match2d) that are < 0.  One workgroup, a fixed order.  Every addend is an integer or a float32
 * quotient c/v of integers 0 <= c <= v <= J: a multiple of 2^-29 for J <= 64, so the float64 sums are exact up to 2^24 rows
 * and do not depend on how a dataset is cut into calls.  ROMP_EINVAL: a null acc, B < 0, Ng < 0, Np < 0, a null array that has rows. */
int  romp_rh_accumulate(const int32_t* counts, int B, const float* pckh, int Ng, const int32_t* gt_of_pred, int Np, double* acc,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ROMP_HIP_RH_H */
