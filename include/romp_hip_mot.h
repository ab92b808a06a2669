/* romp_hip_mot.h -- tracking scores on the device: HOTA, CLEAR-MOT and Identity (IDF1) for many clips in one call each.  An
 * addition to the C ABI of romp_hip.h (same conventions, same ABI version 7; the symbols are listed in romp_amd/lib.py MOT_EXPORTS:
 * a host that must run on an older library looks them up by name).  The definitions are TrackEval's (metrics/hota.py, clear.py,
 * identity.py); romp_amd/tracking_metrics.py `score_clip_host` is their host mirror.
 * Every entry: int status plus romp_last_error(); every argument check before any device call (ROMP_EINVAL launches nothing);
 * enqueued on `stream`, no host synchronisation; no atomics, every sum in a fixed order, so equal inputs give equal bits.  All
 * arithmetic is float64 on the float32 boxes, compiled without fused multiply-adds.
 *
 * Layout.  One call scores S clips holding F frames in all; clip s owns the frames clip_frames[s] .. clip_frames[s+1]-1.  Frame f
 * owns the ground-truth rows gt_off[f] .. gt_off[f+1]-1 and the predicted rows pred_off[f] .. pred_off[f+1]-1 (at most
 * ROMP_TRACK_MAX_DET rows per frame and side).  A row carries an id, dense per clip: 0 .. n_gt_ids[s]-1 and 0 .. n_pred_ids[s]-1 (at
 * most ROMP_TRACK_MAX_CAPACITY each).  A row whose id is negative (or not below that count) is UNUSED: it is nobody, counts for
 * nothing and has similarity 0 -- so the padded (T, capacity) output of romp_track_frames is a valid prediction side as it is.  An id
 * may own at most one row of a frame.  n_pred_ids may be an upper bound: an id that never occurs changes no score (n_gt_ids enters
 * ML and must be exact).  The similarity is ragged: frame f owns the row-major (gt rows x pred rows) block at sim_off[f].
 *
 * These numbers live in ONE block of int64 words that romp_mot_pack checks and writes on the HOST; the caller uploads a copy, and
 * every device entry takes both: the host block (checked again, sizes the launches) and the device copy (read by the kernels).
 *   words 0..15   magic, S, F, words, gt rows, pred rows, similarity elements, gt table ints, pred table ints, id-pair elements,
 *                 the largest n_gt_ids * n_pred_ids of a clip, the largest block of a frame, 0...
 *   then          clip_frames[S+1]  n_gt_ids[S]  n_pred_ids[S]  gt_table_off[S+1]  pred_table_off[S+1]  pair_off[S+1]
 *                 frame_clip[F]  gt_off[F+1]  pred_off[F+1]  sim_off[F+1]
 * Workspace: ONE caller-owned device buffer of romp_mot_workspace_bytes, 8-byte aligned, shared by the entries below (so they run
 * one after the other on one stream): the presence tables (frame x id -> row of the frame or -1) that romp_mot_tables writes and
 * romp_mot_hota / romp_mot_identity read, the id-pair matrix, the cost matrices of the frames, the matches of the frames.
 *
 * Launches: romp_mot_boxes 1, romp_mot_tables 1, romp_mot_similarity 1, romp_mot_hota 4, romp_mot_clear 1, romp_mot_identity 2. */
#ifndef ROMP_HIP_MOT_H
#define ROMP_HIP_MOT_H
#include "romp_hip.h"
#include "romp_hip_track.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ROMP_MOT_ALPHAS     19       /* HOTA's localisation thresholds 0.05 .. 0.95 */
#define ROMP_MOT_MAX_CLIPS  65535
#define ROMP_MOT_MAX_FRAMES (1 << 20)
#define ROMP_MOT_HOTA_OUT   7        /* per clip and alpha: TP, FN, FP, LocA_sum, and the sums of AssA, AssRe, AssPr before / max(1, TP) */
#define ROMP_MOT_CLEAR_OUT  12       /* per clip: CLR_TP, CLR_FN, CLR_FP, IDSW, MT, PT, ML, Frag, CLR_Frames, MOTP_sum, gt dets, tracker dets */
#define ROMP_MOT_ID_OUT     3        /* per clip: IDTP, IDFN, IDFP */

/* HOST only.  Checks the layout (all arrays on the host, the offsets starting at 0 and not decreasing, the caps above, 1 <= S <=
 * ROMP_MOT_MAX_CLIPS, 0 <= F <= ROMP_MOT_MAX_FRAMES) and returns the number of int64 words of the block, written to `block` when it
 * is not NULL (then block_words must be at least that number).  ROMP_EINVAL otherwise. */
int  romp_mot_pack(int S, int F, const int32_t* clip_frames, const int32_t* gt_off, const int32_t* pred_off, const int32_t* n_gt_ids,
                   const int32_t* n_pred_ids, int64_t* block, int block_words);

/* HOST only.  Bytes of the workspace of a block. */
int  romp_mot_workspace_bytes(const int64_t* block, int64_t* bytes);

/* The box of a set of 2-D joints as the reference's pj2ds_to_bbox has it: kp2d (N, J, 2) float32 -> boxes (N, 4) float64 = left, top,
 * width, height: the min / max over the joints, the half extents about the centre enlarged by (enlarge_x, enlarge_y). */
int  romp_mot_boxes(const float* kp2d, int N, int J, double enlarge_x, double enlarge_y, double* boxes, void* stream);

/* The presence tables of the workspace from the ids (int32 per row, device).  One workgroup per frame. */
int  romp_mot_tables(const int64_t* block, const int64_t* block_dev, const int32_t* gt_ids, const int32_t* pred_ids, void* workspace,
                     void* stream);

/* The IoU blocks.  gt_boxes (gt rows, 4) float32 = x, y, w, h.  Predictions: pred_boxes (pred rows, 4) float32, or -- pred_boxes NULL
 * -- pred_kp2d (pred rows, J, 2) float32, boxed as romp_mot_boxes does.  IoU = intersection / union, 0 where the union is 0; an IoU
 * with 1 - IoU > max_iou is set to 0; a pair with an unused row is 0, and so is a pair with a box that has a NaN or infinite
 * coordinate (given as a box; joints are boxed with fmin / fmax, which pass over a NaN).  Also rowsum[gt rows] and colsum[pred rows] of each block,
 * summed in index order.  One workgroup per frame, one thread per pair. */
int  romp_mot_similarity(const int64_t* block, const int64_t* block_dev, const float* gt_boxes, const int32_t* gt_ids,
                         const float* pred_boxes, const float* pred_kp2d, int J, double enlarge_x, double enlarge_y,
                         const int32_t* pred_ids, double max_iou, double* sim, double* rowsum, double* colsum, void* stream);

/* HOTA.  alphas_host[ROMP_MOT_ALPHAS] on the HOST (read before return).  out (S, ROMP_MOT_ALPHAS, ROMP_MOT_HOTA_OUT) float64.
 * (a) one thread per id pair of a clip walks the frames through the tables: potential[g, k], the presence counts, A[g, k];
 * (b) one wave per frame: cost = -A * sim, wave_assign with limit 0, the matched column and its similarity per row, TP and LocA_sum
 *     per alpha (similarity >= alpha - eps);
 * (c) one thread per id pair walks the frames again: the 19 match counts in registers, its AssA / AssRe / AssPr terms, summed per
 *     workgroup in a fixed order;
 * (d) one workgroup per clip adds the workgroups of (c) and the frames of (b) in order. */
int  romp_mot_hota(const int64_t* block, const int64_t* block_dev, const int32_t* gt_ids, const int32_t* pred_ids, const double* sim,
                   const double* rowsum, const double* colsum, const double* alphas_host, void* workspace, double* out, void* stream);

/* CLEAR.  One wave per clip walks its frames in order (state in LDS: the id each ground-truth id was last matched to, ever and in
 * the previous scored frame; presence, match and fragment counts), one wave_assign per frame on
 * -(1000 [k is the id g had in the previous frame] + sim), 0 where sim < threshold - eps; pairs of score > eps are kept.
 * out (S, ROMP_MOT_CLEAR_OUT) float64. */
int  romp_mot_clear(const int64_t* block, const int64_t* block_dev, const int32_t* gt_ids, const int32_t* pred_ids, const double* sim,
                    double threshold, void* workspace, double* out, void* stream);

/* Identity.  pm[g, k] = frames with both present and sim >= threshold (one thread per id pair), then one wave per clip:
 * IDTP = the optimum of wave_assign on -pm with limit 0, IDFN = gt dets - IDTP, IDFP = tracker dets - IDTP.
 * out (S, ROMP_MOT_ID_OUT) float64. */
int  romp_mot_identity(const int64_t* block, const int64_t* block_dev, const int32_t* gt_ids, const int32_t* pred_ids, const double* sim,
                       double threshold, void* workspace, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ROMP_HIP_MOT_H */
