/* romp_hip_track.h -- ByteTrack-3D association of BEV's video mode on the device: an addition to the C ABI of romp_hip.h (same
 * conventions, same ABI version 7; the symbols are listed in romp_amd/lib.py TRACK_EXPORTS: a host that must run on an older
 * library looks them up by name).  A frame of a video is
 *   romp_track_frames (one launch) -> romp_oneeuro_smooth_frames (one launch) -> one download of the count and the ids.
 * Every entry: int status plus romp_last_error(); every argument check before any device call (ROMP_EINVAL launches nothing);
 * enqueued on `stream`, no host synchronisation; no atomics, every sum in a fixed order, so equal inputs give equal bits.  All
 * tracker arithmetic is float64 on the float32 inputs, compiled without fused multiply-adds.
 *
 * The tracker is romp_amd/tracker.py `Tracker.update`, decision for decision (the mirror of the reference's
 * byte_tracker_3dcenter.py:21-160): float32 strong / weak split, batch Kalman prediction of the confirmed and the lost tracks
 * (lost ones coast with mean[7] = 0), three association rounds (pool x strong at match_thresh; still-tracked x strong AGAIN at
 * twice that, only when some weak detection exists; tentative x leftover at three times), kf_correct / absorb, births (confirmed
 * only on frame 1), the lost-track timeout (a timed-out track leaves the lost list one frame later), the tracked and lost lists
 * rebuilt in the order of union / minus, duplicate removal (a live and a lost track closer than dup_thresh in (x, y): the
 * younger by frame - born goes; at equal age the live one) and nearest_detection (first minimum over all rows of the frame).
 *
 * Non-finite input (the host tracker raises on it): a row with a NaN or infinite coordinate stays alone.  Every distance to it is
 * not comparable, which the assignment takes as a forbidden pair; with a strong score it begins a tentative track that nothing
 * matches and that is removed a frame later, as a far-away detection would; and it is never reported as the nearest detection of
 * a finite track, at whichever row it stands.  A NaN score is neither strong nor weak: the row takes part in no association.
 *
 * State: ONE caller-owned device buffer of romp_track_state_bytes(capacity) bytes, 8-byte aligned:
 *   int32 header[32]   [0] capacity  [1] frame id  [2] last id  [3] number tracked  [4] number lost  [5] overflow count
 *                      [6] max_time_lost  [7] 0  [8] det_thresh (float32 bits)  [9] low_thresh (float32 bits)  [10..15] 0
 *                      [16..17] match_thresh (float64)  [18..19] dup_thresh (float64)  [20..31] 0
 *   int32 rows[ROMP_TRACK_MAX_FRAMES]   the row counts of the frames of the running multi-frame call
 *   table              capacity records of ROMP_TRACK_SLOT_BYTES: float64 mean[8], float64 covariance[8][8], float32 score, int32
 *                      state (0 free, 1 tracked, 2 lost, 3 removed), confirmed, id, frame, born, hits, dropped (the track has been
 *                      on the host's removed list: once lost again it is forgotten at once, as minus(lost, removed) has it)
 *   int32 tracked[capacity], lost[capacity]   the two ordered lists, as table slots
 *   float64 cost[capacity][ROMP_TRACK_MAX_DET]   workspace of the cost matrices
 * A record whose state is 0 is free.  A track is begun in the lowest free slot. */
#ifndef ROMP_HIP_TRACK_H
#define ROMP_HIP_TRACK_H
#include "romp_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ROMP_TRACK_MAX_DET      256   /* detections of one frame */
#define ROMP_TRACK_MAX_CAPACITY 512   /* table slots */
#define ROMP_TRACK_MAX_FRAMES   1024  /* frames of one call */
#define ROMP_TRACK_SLOT_BYTES   608
#define ROMP_TRACK_RECORD       14    /* float64 per track of romp_track_list */

/* Bytes of the state buffer, or ROMP_EINVAL unless 1 <= capacity <= ROMP_TRACK_MAX_CAPACITY. */
int  romp_track_state_bytes(int capacity);

/* Clear the state (one memset and one small upload on `stream`).  first_id: the id before the first one given out, the
 * per-instance stand-in for the host's class-wide Track.last_id.  ROMP_EINVAL: NULL state, capacity out of range, first_id < 0,
 * a threshold that is NaN or negative, max_time_lost < 0. */
int  romp_track_init(void* state, int capacity, int first_id, float det_thresh, float low_thresh, double match_thresh,
                     int max_time_lost, double dup_thresh, void* stream);

/* T frames in ONE launch of one workgroup.  points (sum N, 4) float32 and scores (sum N) float32 on the device, the rows of
 * frame t after those of frame t-1; frame_rows_host[T] on the HOST, read before return, each 0..ROMP_TRACK_MAX_DET.  A frame with
 * 0 rows is skipped: the frame id does not advance, out_count[t] = 0.
 * Outputs, device int32: out_count[T]; out_ids, out_rows, out_slots [T * capacity], entry k of frame t at t * capacity + k:
 * the id, the ABSOLUTE row in `points` and the table slot of the k-th confirmed track, in the order of the tracked list.  The
 * entries from out_count[t] to capacity - 1 are filled with id -1, row 0, slot -1.
 * oneeuro_flags (or NULL): when a track is begun in a slot, 0.f is written to oneeuro_flags[slot * oneeuro_stride] -- the
 * `initialised` word of the filter state of romp_oneeuro_smooth, so the table slot doubles as the filter slot.  In a call of
 * several frames that write must not reach back to the frames in which the slot's earlier track was still reported: then the
 * word is set to -(t + 1) instead ("afresh from frame t of this call on"; -(t + 1.5): and afresh at the start of the call too),
 * which romp_oneeuro_smooth_frames applies and clears; run it on the same outputs before the next romp_track_frames.  A slot takes
 * one such hand-over per call: one that would need a second is passed over for the rest of the call (the only way in which one
 * T-frame call can differ from T one-frame calls, and then only in slot numbers; without oneeuro_flags there is none).
 * A full table: the detection that should begin a track is left without one on that frame, header[5] goes up by one, nothing
 * else changes.
 * `capacity` in the output layout is the one the state was initialised with (header[0], read on the device).  ROMP_EINVAL: a NULL
 * pointer other than oneeuro_flags, T outside 1..ROMP_TRACK_MAX_FRAMES, an entry of frame_rows_host out of range, oneeuro_stride < 1
 * with flags given. */
int  romp_track_frames(void* state, const float* points, const float* scores, const int32_t* frame_rows_host, int T,
                       int32_t* out_count, int32_t* out_ids, int32_t* out_rows, int32_t* out_slots, float* oneeuro_flags,
                       int oneeuro_stride, void* stream);

/* The exact assignment of one association round on its own: cost (n, m) float64 on the device; pair_of_row[n] int32, the column of
 * each row or -1.  Minimises the sum of (cost - limit) over the chosen pairs: the optimum of lapjv(cost, extend_cost=True,
 * cost_limit=limit), i.e. of tracker.assign's (n+m)^2 matrix padded with limit / 2.  Shortest augmenting paths on n x (m + 1)
 * columns, the last one "stay unassigned" at cost `limit` and never full; ONE wave, columns across lanes, the minimum of a step
 * by a cross-lane reduction (lowest column wins a tie).  1 <= n <= 512, 1 <= m <= 512, limit finite, else ROMP_EINVAL. */
int  romp_track_assign(const double* cost, int n, int m, double limit, int32_t* pair_of_row, void* stream);

/* The tracks in list order: records (capacity, ROMP_TRACK_RECORD) float64 = id, state, confirmed, frame, born, score, mean[8];
 * the tracked list first, then the lost list; count[2] int32 = number tracked, number lost.  Rows past their sum are not
 * written. */
int  romp_track_list(const void* state, double* records, int32_t* count, void* stream);

/* The OneEuro filters of romp_oneeuro_smooth for what romp_track_frames reported, T frames in ONE launch: one workgroup per
 * table slot walks the frames, and where its slot is entry k of frame t it filters detection row out_rows[t * capacity + k] of
 * thetas_in (rows, 72) / betas_in (rows, n_betas) / cam_in (rows, 3) into row t * capacity + k of thetas_out / betas_out /
 * cam_out ((T * capacity, .) rows; rows that report nobody are not written).  state: the filter state of romp_oneeuro_smooth
 * with `capacity` slots, whose `initialised` words romp_track_frames has marked (above).  The counts are read on the device.
 * The same device code as romp_oneeuro_smooth: equal bits. */
int  romp_oneeuro_smooth_frames(float* state, int T, int capacity, const int32_t* out_count, const int32_t* out_rows,
                                const int32_t* out_slots, int n_betas, float smooth_coeff, const float* thetas_in,
                                const float* betas_in, const float* cam_in, float* thetas_out, float* betas_out, float* cam_out,
                                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ROMP_HIP_TRACK_H */
