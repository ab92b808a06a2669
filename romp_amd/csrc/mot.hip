// mot.hip -- tracking scores on the device: HOTA, CLEAR-MOT and Identity for many clips (include/romp_hip_mot.h).
//
// The mirror of romp_amd/tracking_metrics.py `score_clip_host` (itself written from TrackEval's metrics/hota.py, clear.py and
// identity.py).  Every exact assignment -- one per frame for HOTA and CLEAR, one per clip for Identity -- is wave_assign of assign.h
// on cost = -score with limit 0: a rectangular linear_sum_assignment(-score), since a pair of score 0 and no pair contribute the same
// to every count.  All arithmetic is float64 on the float32 boxes; this file is compiled with -ffp-contract=off (romp_amd/build.py).
// No atomics: a sum is a loop in index order, or per-lane partial sums in index order joined by a fixed shuffle tree.
#include <float.h>
#include <string.h>
#include "common.h"
#include "../../include/romp_hip_mot.h"
#include "assign.h"

namespace romp {

constexpr int MAXD = ROMP_TRACK_MAX_DET, NA = ROMP_MOT_ALPHAS, NT = 256, NTERM = 3 * NA;
constexpr int64_t MAGIC = 0x4d4f5431;                                  // "MOT1"
enum { B_MAGIC = 0, B_S, B_F, B_WORDS, B_GT_ROWS, B_PRED_ROWS, B_SIM, B_GTAB, B_PTAB, B_PAIRS, B_MAX_PAIRS, B_MAX_BLOCK, B_HEAD = 16 };

struct Meta {
    int S, F;
    const int64_t *clip_frames, *n_gt, *n_pred, *gtab_off, *ptab_off, *pair_off, *frame_clip, *gt_off, *pred_off, *sim_off;
};

__host__ __device__ inline int64_t block_words(int64_t S, int64_t F) { return B_HEAD + (S + 1) + 2 * S + 3 * (S + 1) + F + 3 * (F + 1); }

__host__ __device__ inline Meta view(const int64_t* b) {
    Meta m;
    m.S = (int)b[B_S]; m.F = (int)b[B_F];
    const int64_t S = m.S, F = m.F;
    const int64_t* p = b + B_HEAD;
    m.clip_frames = p; p += S + 1;
    m.n_gt = p; p += S;
    m.n_pred = p; p += S;
    m.gtab_off = p; p += S + 1;
    m.ptab_off = p; p += S + 1;
    m.pair_off = p; p += S + 1;
    m.frame_clip = p; p += F;
    m.gt_off = p; p += F + 1;
    m.pred_off = p; p += F + 1;
    m.sim_off = p;
    return m;
}

// the workspace: float64 parts first, then the int32 parts
struct Work {
    double *A, *cost, *match_sim, *frame_loc, *partial;
    int *gtab, *ptab, *match_col, *frame_tp, *frame_cnt;
    int nblk;
    size_t bytes;
};

inline Work carve(const int64_t* b, void* ws) {
    Work w;
    const size_t S = (size_t)b[B_S], F = (size_t)b[B_F];
    w.nblk = (int)((b[B_MAX_PAIRS] + NT - 1) / NT);
    double* d = (double*)ws;
    w.A = d; d += b[B_PAIRS];
    w.cost = d; d += b[B_SIM];
    w.match_sim = d; d += b[B_GT_ROWS];
    w.frame_loc = d; d += F * NA;
    w.partial = d; d += S * (size_t)w.nblk * NTERM;
    int* i = (int*)d;
    w.gtab = i; i += b[B_GTAB];
    w.ptab = i; i += b[B_PTAB];
    w.match_col = i; i += b[B_GT_ROWS];
    w.frame_tp = i; i += F * NA;
    w.frame_cnt = i; i += F * 2;
    w.bytes = (((char*)i - (char*)ws) + 7) / 8 * 8;
    return w;
}

// is this a block romp_mot_pack wrote?  (the sizes it leads to are then within the caps)
static const char* bad_block(const int64_t* b) {
    if (!b) return "NULL block";
    if (b[B_MAGIC] != MAGIC) return "not a block of romp_mot_pack";
    const int64_t S = b[B_S], F = b[B_F];
    if (S < 1 || S > ROMP_MOT_MAX_CLIPS || F < 0 || F > ROMP_MOT_MAX_FRAMES || b[B_WORDS] != block_words(S, F)) return "S, F or the word count";
    const Meta m = view(b);
    if (m.clip_frames[0] != 0 || m.clip_frames[S] != F || m.gt_off[0] != 0 || m.pred_off[0] != 0 || m.sim_off[0] != 0 ||
        m.gtab_off[0] != 0 || m.ptab_off[0] != 0 || m.pair_off[0] != 0)
        return "an offset list does not start at 0 or end at F";
    int64_t max_pairs = 0, max_block = 0;
    for (int64_t s = 0; s < S; ++s) {
        const int64_t T = m.clip_frames[s + 1] - m.clip_frames[s], G = m.n_gt[s], K = m.n_pred[s];
        if (T < 0 || G < 0 || G > MAXC || K < 0 || K > MAXC) return "a clip's frame range or id count";
        if (m.gtab_off[s + 1] != m.gtab_off[s] + T * G || m.ptab_off[s + 1] != m.ptab_off[s] + T * K || m.pair_off[s + 1] != m.pair_off[s] + G * K)
            return "a table offset";
        for (int64_t f = m.clip_frames[s]; f < m.clip_frames[s + 1]; ++f)
            if (m.frame_clip[f] != s) return "frame_clip";
        if (G * K > max_pairs) max_pairs = G * K;
    }
    for (int64_t f = 0; f < F; ++f) {
        const int64_t n = m.gt_off[f + 1] - m.gt_off[f], k = m.pred_off[f + 1] - m.pred_off[f];
        if (n < 0 || n > MAXD || k < 0 || k > MAXD) return "a frame's row count";
        if (m.sim_off[f + 1] != m.sim_off[f] + n * k) return "a similarity offset";
        if (n * k > max_block) max_block = n * k;
    }
    if (b[B_GT_ROWS] != m.gt_off[F] || b[B_PRED_ROWS] != m.pred_off[F] || b[B_SIM] != m.sim_off[F] || b[B_GTAB] != m.gtab_off[S] ||
        b[B_PTAB] != m.ptab_off[S] || b[B_PAIRS] != m.pair_off[S] || b[B_MAX_PAIRS] != max_pairs || b[B_MAX_BLOCK] != max_block)
        return "a total";
    return nullptr;
}

__device__ __forceinline__ bool valid_id(int id, int n) { return id >= 0 && id < n; }

// per-lane partial sums joined in a fixed order
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// how many of ids[0..n) are valid (the same value in every lane)
__device__ __forceinline__ int wave_count_valid(int lane, const int32_t* __restrict__ ids, int n, int limit) {
    int c = 0;
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        c += __popcll(__ballot(i < n && valid_id(ids[i], limit)));
    }
    return c;
}

// A box with a NaN or infinite coordinate is similar to nothing (iou_host gives 0 there: numpy's minimum and maximum hand a NaN on,
// fmin and fmax would drop it and score the rest of the box)
__device__ __forceinline__ bool finite_box(const double* b) { return isfinite(b[0]) && isfinite(b[1]) && isfinite(b[2]) && isfinite(b[3]); }

__device__ __forceinline__ void box_of_joints(const float* __restrict__ kp, int J, double ex, double ey, double* box) {
    double x0 = (double)kp[0], x1 = x0, y0 = (double)kp[1], y1 = y0;
    for (int j = 1; j < J; ++j) {
        const double x = (double)kp[2 * j], y = (double)kp[2 * j + 1];
        x0 = fmin(x0, x); x1 = fmax(x1, x); y0 = fmin(y0, y); y1 = fmax(y1, y);
    }
    const double cx = (x1 + x0) / 2, cy = (y1 + y0) / 2;
    const double hx = (cx - x0) * ex, hy = (cy - y0) * ey;
    box[0] = cx - hx; box[1] = cy - hy; box[2] = hx * 2; box[3] = hy * 2;
}

__global__ __launch_bounds__(NT) void mot_boxes_kernel(const float* __restrict__ kp2d, int N, int J, double ex, double ey, double* __restrict__ boxes) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < N) box_of_joints(kp2d + (size_t)i * J * 2, J, ex, ey, boxes + (size_t)i * 4);
}

__global__ __launch_bounds__(64) void mot_tables_kernel(const int64_t* __restrict__ blk, const int32_t* __restrict__ gt_ids,
                                                        const int32_t* __restrict__ pred_ids, int* __restrict__ gtab, int* __restrict__ ptab) {
    const Meta M = view(blk);
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= M.F) return;
    const int s = (int)M.frame_clip[f], t = f - (int)M.clip_frames[s], G = (int)M.n_gt[s], K = (int)M.n_pred[s];
    int* g = gtab + M.gtab_off[s] + (int64_t)t * G;
    int* p = ptab + M.ptab_off[s] + (int64_t)t * K;
    for (int i = lane; i < G; i += 64) g[i] = -1;
    for (int i = lane; i < K; i += 64) p[i] = -1;
    __syncthreads();
    const int64_t go = M.gt_off[f], po = M.pred_off[f];
    const int n = (int)(M.gt_off[f + 1] - go), m = (int)(M.pred_off[f + 1] - po);
    for (int r = lane; r < n; r += 64) {
        const int id = gt_ids[go + r];
        if (valid_id(id, G)) g[id] = r;
    }
    for (int c = lane; c < m; c += 64) {
        const int id = pred_ids[po + c];
        if (valid_id(id, K)) p[id] = c;
    }
}

__global__ __launch_bounds__(NT) void mot_similarity_kernel(const int64_t* __restrict__ blk, const float* __restrict__ gt_boxes,
                                                            const int32_t* __restrict__ gt_ids, const float* __restrict__ pred_boxes,
                                                            const float* __restrict__ pred_kp2d, int J, double ex, double ey,
                                                            const int32_t* __restrict__ pred_ids, double max_iou, double* __restrict__ sim,
                                                            double* __restrict__ rowsum, double* __restrict__ colsum) {
    __shared__ double gb[MAXD * 4], pb[MAXD * 4];
    __shared__ unsigned char gv[MAXD], pv[MAXD];
    const Meta M = view(blk);
    const int f = blockIdx.x, tid = threadIdx.x;
    if (f >= M.F) return;
    const int s = (int)M.frame_clip[f], G = (int)M.n_gt[s], K = (int)M.n_pred[s];
    const int64_t go = M.gt_off[f], po = M.pred_off[f], so = M.sim_off[f];
    const int n = (int)(M.gt_off[f + 1] - go), m = (int)(M.pred_off[f + 1] - po);
    for (int r = tid; r < n; r += NT) {
        for (int k = 0; k < 4; ++k) gb[4 * r + k] = (double)gt_boxes[(go + r) * 4 + k];
        gv[r] = valid_id(gt_ids[go + r], G) && finite_box(gb + 4 * r);
    }
    for (int c = tid; c < m; c += NT) {
        if (pred_boxes) for (int k = 0; k < 4; ++k) pb[4 * c + k] = (double)pred_boxes[(po + c) * 4 + k];
        else box_of_joints(pred_kp2d + (po + c) * J * 2, J, ex, ey, pb + 4 * c);
        pv[c] = valid_id(pred_ids[po + c], K) && finite_box(pb + 4 * c);
    }
    __syncthreads();
    for (int idx = tid; idx < n * m; idx += NT) {
        const int r = idx / m, c = idx - r * m;
        double v = 0.;
        if (gv[r] && pv[c]) {
            const double* a = gb + 4 * r, *b = pb + 4 * c;
            const double iw = fmin(a[0] + a[2], b[0] + b[2]) - fmax(a[0], b[0]), ih = fmin(a[1] + a[3], b[1] + b[3]) - fmax(a[1], b[1]);
            const double inter = iw > 0. && ih > 0. ? iw * ih : 0.;
            const double uni = (a[2] * a[3] + b[2] * b[3]) - inter;
            if (uni > 0.) v = inter / uni;
            if (1. - v > max_iou) v = 0.;
        }
        sim[so + idx] = v;
    }
    __syncthreads();                                                   // (the block reads back what it wrote)
    for (int r = tid; r < n; r += NT) {
        double a = 0.;
        for (int c = 0; c < m; ++c) a += sim[so + r * m + c];
        rowsum[go + r] = a;
    }
    for (int c = tid; c < m; c += NT) {
        double a = 0.;
        for (int r = 0; r < n; ++r) a += sim[so + r * m + c];
        colsum[po + c] = a;
    }
}

// One thread per id pair (g, k) of a clip walks the clip's frames through the presence tables.
// IDENT false: HOTA's first pass, out = A[g, k].  IDENT true: out = -pm[g, k], the cost of Identity's assignment.
template <bool IDENT>
__global__ __launch_bounds__(NT) void mot_pair_walk_kernel(const int64_t* __restrict__ blk, const int* __restrict__ gtab, const int* __restrict__ ptab,
                                                           const double* __restrict__ sim, const double* __restrict__ rowsum,
                                                           const double* __restrict__ colsum, double threshold, double* __restrict__ out) {
    const Meta M = view(blk);
    const int s = blockIdx.y;
    const int G = (int)M.n_gt[s], K = (int)M.n_pred[s];
    const int p = blockIdx.x * NT + threadIdx.x;
    if (p >= G * K) return;
    const int g = p / K, k = p - g * K;
    const int f0 = (int)M.clip_frames[s], T = (int)M.clip_frames[s + 1] - f0;
    const int* gt = gtab + M.gtab_off[s] + g;
    const int* pt = ptab + M.ptab_off[s] + k;
    double acc = 0.;
    int gc = 0, tc = 0;
    for (int t = 0; t < T; ++t) {
        const int gr = gt[(int64_t)t * G], pr = pt[(int64_t)t * K];
        gc += gr >= 0; tc += pr >= 0;
        if (gr >= 0 && pr >= 0) {
            const int f = f0 + t;
            const int m = (int)(M.pred_off[f + 1] - M.pred_off[f]);
            const double v = sim[M.sim_off[f] + (int64_t)gr * m + pr];
            if (IDENT) acc += v >= threshold ? 1. : 0.;
            else {
                const double den = (colsum[M.pred_off[f] + pr] + rowsum[M.gt_off[f] + gr]) - v;
                if (den > DBL_EPSILON) acc += v / den;
            }
        }
    }
    if (IDENT) out[M.pair_off[s] + p] = -acc;
    else out[M.pair_off[s] + p] = gc + tc > 0 ? acc / (((double)gc + (double)tc) - acc) : 0.;
}

struct Thresholds { double v[NA]; };                                   // alpha - eps

__global__ __launch_bounds__(64) void mot_hota_frame_kernel(const int64_t* __restrict__ blk, const int32_t* __restrict__ gt_ids,
                                                            const int32_t* __restrict__ pred_ids, const double* __restrict__ sim,
                                                            const double* __restrict__ A, Thresholds th, double* __restrict__ cost,
                                                            int* __restrict__ match_col, double* __restrict__ match_sim,
                                                            int* __restrict__ frame_tp, double* __restrict__ frame_loc, int* __restrict__ frame_cnt) {
    __shared__ SolveLds L;
    __shared__ int pair[MAXC];
    const Meta M = view(blk);
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= M.F) return;
    const int s = (int)M.frame_clip[f], G = (int)M.n_gt[s], K = (int)M.n_pred[s];
    const int64_t go = M.gt_off[f], po = M.pred_off[f], so = M.sim_off[f];
    const int n = (int)(M.gt_off[f + 1] - go), m = (int)(M.pred_off[f + 1] - po);
    const int ngv = wave_count_valid(lane, gt_ids + go, n, G), npv = wave_count_valid(lane, pred_ids + po, m, K);
    int tp[NA];
    double loc[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) { tp[a] = 0; loc[a] = 0.; }
    const bool solve = ngv > 0 && npv > 0;
    if (solve) {
        const double* Ac = A + M.pair_off[s];
        for (int idx = lane; idx < n * m; idx += 64) {
            const int r = idx / m, c = idx - r * m;
            const int gi = gt_ids[go + r], ki = pred_ids[po + c];
            cost[so + idx] = valid_id(gi, G) && valid_id(ki, K) ? -(Ac[gi * K + ki] * sim[so + idx]) : 0.;
        }
        __syncthreads();
        wave_assign(lane, cost + so, m, n, m, 0., L, pair);
    }
    for (int r0 = 0; r0 < n; r0 += 64) {
        const int r = r0 + lane;
        bool ok = false;
        int c = -1;
        double v = 0.;
        if (solve && r < n) {
            c = pair[r];
            ok = c >= 0 && valid_id(gt_ids[go + r], G) && valid_id(pred_ids[po + c], K);
            if (ok) v = sim[so + r * m + c];
        }
        if (r < n) { match_col[go + r] = ok ? c : -1; match_sim[go + r] = v; }
#pragma unroll
        for (int a = 0; a < NA; ++a) {
            const bool hit = ok && v >= th.v[a];
            tp[a] += __popcll(__ballot(hit));
            loc[a] += hit ? v : 0.;
        }
    }
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const double l = wave_sum(loc[a]);
        if (lane == 0) { frame_tp[(size_t)f * NA + a] = tp[a]; frame_loc[(size_t)f * NA + a] = l; }
    }
    if (lane == 0) { frame_cnt[2 * (size_t)f] = ngv; frame_cnt[2 * (size_t)f + 1] = npv; }
}

__global__ __launch_bounds__(NT) void mot_hota_pairs_kernel(const int64_t* __restrict__ blk, const int* __restrict__ gtab, const int* __restrict__ ptab,
                                                            const int* __restrict__ match_col, const double* __restrict__ match_sim, Thresholds th,
                                                            int nblk, double* __restrict__ partial) {
    __shared__ double red[NT / 64][NTERM];
    const Meta M = view(blk);
    const int s = blockIdx.y, tid = threadIdx.x;
    const int G = (int)M.n_gt[s], K = (int)M.n_pred[s];
    const int p = blockIdx.x * NT + tid;
    int cnt[NA];
#pragma unroll
    for (int a = 0; a < NA; ++a) cnt[a] = 0;
    int gc = 0, tc = 0;
    if (p < G * K) {
        const int g = p / K, k = p - g * K;
        const int f0 = (int)M.clip_frames[s], T = (int)M.clip_frames[s + 1] - f0;
        const int* gt = gtab + M.gtab_off[s] + g;
        const int* pt = ptab + M.ptab_off[s] + k;
        for (int t = 0; t < T; ++t) {
            const int gr = gt[(int64_t)t * G], pr = pt[(int64_t)t * K];
            gc += gr >= 0; tc += pr >= 0;
            if (gr >= 0 && pr >= 0) {
                const int64_t row = M.gt_off[f0 + t] + gr;
                if (match_col[row] == pr) {
                    const double v = match_sim[row];
#pragma unroll
                    for (int a = 0; a < NA; ++a) cnt[a] += v >= th.v[a];
                }
            }
        }
    }
#pragma unroll
    for (int a = 0; a < NA; ++a) {
        const double c = (double)cnt[a];
        const double ta = c * (c / fmax(1., ((double)gc + (double)tc) - c));
        const double tr = c * (c / fmax(1., (double)gc));
        const double tq = c * (c / fmax(1., (double)tc));
        const double sa = wave_sum(ta), sr = wave_sum(tr), sq = wave_sum(tq);
        if ((tid & 63) == 0) { red[tid >> 6][3 * a] = sa; red[tid >> 6][3 * a + 1] = sr; red[tid >> 6][3 * a + 2] = sq; }
    }
    __syncthreads();
    if (tid < NTERM) {
        double v = 0.;
        for (int w = 0; w < NT / 64; ++w) v += red[w][tid];
        partial[((size_t)s * nblk + blockIdx.x) * NTERM + tid] = v;
    }
}

__global__ __launch_bounds__(64) void mot_hota_reduce_kernel(const int64_t* __restrict__ blk, const int* __restrict__ frame_tp,
                                                             const double* __restrict__ frame_loc, const int* __restrict__ frame_cnt,
                                                             const double* __restrict__ partial, int nblk, double* __restrict__ out) {
    const Meta M = view(blk);
    const int s = blockIdx.x, a = threadIdx.x;
    if (a >= NA) return;
    const int G = (int)M.n_gt[s], K = (int)M.n_pred[s];
    const int used = (G * K + NT - 1) / NT;                            // the workgroups of (c) that held pairs of this clip
    double tp = 0., fn = 0., fp = 0., loc = 0., sa = 0., sr = 0., sq = 0.;
    for (int64_t f = M.clip_frames[s]; f < M.clip_frames[s + 1]; ++f) {
        const int t = frame_tp[f * NA + a];
        tp += t; fn += frame_cnt[2 * f] - t; fp += frame_cnt[2 * f + 1] - t;
        loc += frame_loc[f * NA + a];
    }
    for (int b = 0; b < used; ++b) {
        const double* q = partial + ((size_t)s * nblk + b) * NTERM + 3 * a;
        sa += q[0]; sr += q[1]; sq += q[2];
    }
    double* o = out + ((size_t)s * NA + a) * ROMP_MOT_HOTA_OUT;
    o[0] = tp; o[1] = fn; o[2] = fp; o[3] = loc; o[4] = sa; o[5] = sr; o[6] = sq;
}

__global__ __launch_bounds__(64) void mot_clear_kernel(const int64_t* __restrict__ blk, const int32_t* __restrict__ gt_ids,
                                                       const int32_t* __restrict__ pred_ids, const double* __restrict__ sim, double threshold,
                                                       double* __restrict__ cost, double* __restrict__ out) {
    __shared__ SolveLds L;
    __shared__ int pair[MAXC], prev[MAXC], prevf[MAXC], newf[MAXC], gcnt[MAXC], mcnt[MAXC], frag[MAXC];
    const Meta M = view(blk);
    const int s = blockIdx.x, lane = threadIdx.x;
    const int G = (int)M.n_gt[s], K = (int)M.n_pred[s];
    for (int g = lane; g < G; g += 64) { prev[g] = -1; prevf[g] = -1; gcnt[g] = 0; mcnt[g] = 0; frag[g] = 0; }
    wave_sync();
    const double th = threshold - DBL_EPSILON;
    double tp = 0., fn = 0., fp = 0., idsw = 0., gdets = 0., pdets = 0., motp = 0.;
    for (int64_t f = M.clip_frames[s]; f < M.clip_frames[s + 1]; ++f) {
        const int64_t go = M.gt_off[f], po = M.pred_off[f], so = M.sim_off[f];
        const int n = (int)(M.gt_off[f + 1] - go), m = (int)(M.pred_off[f + 1] - po);
        const int ngv = wave_count_valid(lane, gt_ids + go, n, G), npv = wave_count_valid(lane, pred_ids + po, m, K);
        gdets += ngv; pdets += npv;
        if (ngv == 0) { fp += npv; continue; }
        if (npv == 0) {
            fn += ngv;
            for (int r = lane; r < n; r += 64) {
                const int gi = gt_ids[go + r];
                if (valid_id(gi, G)) gcnt[gi] += 1;
            }
            wave_sync();
            continue;
        }
        for (int idx = lane; idx < n * m; idx += 64) {
            const int r = idx / m, c = idx - r * m;
            const int gi = gt_ids[go + r], ki = pred_ids[po + c];
            double sc = 0.;
            if (valid_id(gi, G) && valid_id(ki, K)) {
                const double v = sim[so + idx];
                sc = (prevf[gi] == ki ? 1000. : 0.) + v;
                if (v < th) sc = 0.;
            }
            cost[so + idx] = -sc;
        }
        for (int g = lane; g < G; g += 64) newf[g] = -1;
        __syncthreads();
        wave_assign(lane, cost + so, m, n, m, 0., L, pair);
        int nmatch = 0, nsw = 0;
        for (int r0 = 0; r0 < n; r0 += 64) {
            const int r = r0 + lane;
            bool matched = false, sw = false;
            if (r < n) {
                const int gi = gt_ids[go + r], c = pair[r];
                if (valid_id(gi, G)) {
                    gcnt[gi] += 1;
                    const int ki = c >= 0 ? pred_ids[po + c] : -1;
                    if (valid_id(ki, K) && -cost[so + r * m + c] > DBL_EPSILON) {
                        matched = true;
                        sw = prev[gi] >= 0 && prev[gi] != ki;
                        mcnt[gi] += 1; prev[gi] = ki; newf[gi] = ki;
                        motp += sim[so + r * m + c];
                    }
                }
            }
            nmatch += __popcll(__ballot(matched));
            nsw += __popcll(__ballot(sw));
        }
        wave_sync();
        for (int g = lane; g < G; g += 64) {
            frag[g] += prevf[g] < 0 && newf[g] >= 0;
            prevf[g] = newf[g];
        }
        wave_sync();
        tp += nmatch; fn += ngv - nmatch; fp += npv - nmatch; idsw += nsw;
    }
    int mt = 0, ge = 0, fr = 0;
    for (int g = lane; g < G; g += 64) {
        if (gcnt[g] > 0) {
            const double ratio = (double)mcnt[g] / (double)gcnt[g];
            mt += ratio > 0.8; ge += ratio >= 0.2;
        }
        if (frag[g] > 0) fr += frag[g] - 1;
    }
    mt = wave_sum(mt); ge = wave_sum(ge); fr = wave_sum(fr);
    motp = wave_sum(motp);
    if (lane == 0) {
        double* o = out + (size_t)s * ROMP_MOT_CLEAR_OUT;
        o[0] = tp; o[1] = fn; o[2] = fp; o[3] = idsw; o[4] = mt; o[5] = ge - mt; o[6] = G - ge; o[7] = fr;
        o[8] = (double)(M.clip_frames[s + 1] - M.clip_frames[s]); o[9] = motp; o[10] = gdets; o[11] = pdets;
    }
}

__global__ __launch_bounds__(64) void mot_identity_kernel(const int64_t* __restrict__ blk, const int32_t* __restrict__ gt_ids,
                                                          const int32_t* __restrict__ pred_ids, const double* __restrict__ cost,
                                                          double* __restrict__ out) {
    __shared__ SolveLds L;
    __shared__ int pair[MAXC];
    const Meta M = view(blk);
    const int s = blockIdx.x, lane = threadIdx.x;
    const int G = (int)M.n_gt[s], K = (int)M.n_pred[s];
    const double* c = cost + M.pair_off[s];
    double idtp = 0.;
    if (G > 0 && K > 0) {
        wave_assign(lane, c, K, G, K, 0., L, pair);
        for (int g = lane; g < G; g += 64)
            if (pair[g] >= 0) idtp += -c[g * K + pair[g]];             // (whole numbers: exact in any order)
        idtp = wave_sum(idtp);
    }
    const int64_t f0 = M.clip_frames[s], f1 = M.clip_frames[s + 1];
    const int64_t g0 = M.gt_off[f0], g1 = M.gt_off[f1], p0 = M.pred_off[f0], p1 = M.pred_off[f1];
    int ng = 0, np = 0;
    for (int64_t i = g0 + lane; i < g1; i += 64) ng += valid_id(gt_ids[i], G);
    for (int64_t i = p0 + lane; i < p1; i += 64) np += valid_id(pred_ids[i], K);
    ng = wave_sum(ng); np = wave_sum(np);
    if (lane == 0) {
        double* o = out + (size_t)s * ROMP_MOT_ID_OUT;
        o[0] = idtp; o[1] = ng - idtp; o[2] = np - idtp;
    }
}

}  // namespace romp

using namespace romp;

#define MOT_BLOCK(name)                                                                             \
    do {                                                                                            \
        const char* _why = bad_block(block);                                                        \
        ROMP_REQUIRE(!_why, name ": bad block (%s)", _why);                                         \
        ROMP_REQUIRE(block_dev, name ": NULL device copy of the block");                            \
    } while (0)

extern "C" {

int romp_mot_pack(int S, int F, const int32_t* clip_frames, const int32_t* gt_off, const int32_t* pred_off, const int32_t* n_gt_ids,
                  const int32_t* n_pred_ids, int64_t* block, int block_words_given) {
    ROMP_REQUIRE(clip_frames && gt_off && pred_off && n_gt_ids && n_pred_ids, "romp_mot_pack: NULL argument");
    ROMP_REQUIRE(S >= 1 && S <= ROMP_MOT_MAX_CLIPS && F >= 0 && F <= ROMP_MOT_MAX_FRAMES, "romp_mot_pack: S %d outside 1..%d or F %d outside 0..%d",
                 S, ROMP_MOT_MAX_CLIPS, F, ROMP_MOT_MAX_FRAMES);
    ROMP_REQUIRE(clip_frames[0] == 0 && clip_frames[S] == F && gt_off[0] == 0 && pred_off[0] == 0,
                 "romp_mot_pack: clip_frames must run from 0 to F, the row offsets start at 0");
    for (int s = 0; s < S; ++s) {
        ROMP_REQUIRE(clip_frames[s + 1] >= clip_frames[s] && clip_frames[s + 1] <= F, "romp_mot_pack: clip_frames decreases at clip %d", s);
        ROMP_REQUIRE(n_gt_ids[s] >= 0 && n_gt_ids[s] <= MAXC && n_pred_ids[s] >= 0 && n_pred_ids[s] <= MAXC,
                     "romp_mot_pack: clip %d has %d / %d ids, outside 0..%d", s, n_gt_ids[s], n_pred_ids[s], MAXC);
    }
    for (int f = 0; f < F; ++f) {
        const int64_t n = (int64_t)gt_off[f + 1] - gt_off[f], k = (int64_t)pred_off[f + 1] - pred_off[f];
        ROMP_REQUIRE(n >= 0 && n <= MAXD && k >= 0 && k <= MAXD, "romp_mot_pack: frame %d has %lld / %lld rows, outside 0..%d", f, (long long)n,
                     (long long)k, MAXD);
    }
    const int64_t words = block_words(S, F);
    if (!block) return (int)words;
    ROMP_REQUIRE(block_words_given >= words, "romp_mot_pack: the block needs %lld words, %d given", (long long)words, block_words_given);
    memset(block, 0, 8 * (size_t)words);
    block[B_MAGIC] = MAGIC; block[B_S] = S; block[B_F] = F; block[B_WORDS] = words;
    int64_t* w = block + B_HEAD;                                       // (the arrays in the order of view())
    int64_t* q_clip = w; w += S + 1;
    int64_t* q_ng = w; w += S;
    int64_t* q_np = w; w += S;
    int64_t* q_gtab = w; w += S + 1;
    int64_t* q_ptab = w; w += S + 1;
    int64_t* q_pair = w; w += S + 1;
    int64_t* q_fc = w; w += F;
    int64_t* q_go = w; w += F + 1;
    int64_t* q_po = w; w += F + 1;
    int64_t* q_so = w;
    int64_t max_pairs = 0, max_block = 0;
    for (int s = 0; s <= S; ++s) q_clip[s] = clip_frames[s];
    for (int s = 0; s < S; ++s) {
        const int64_t T = clip_frames[s + 1] - clip_frames[s], G = n_gt_ids[s], K = n_pred_ids[s];
        q_ng[s] = G; q_np[s] = K;
        q_gtab[s + 1] = q_gtab[s] + T * G; q_ptab[s + 1] = q_ptab[s] + T * K; q_pair[s + 1] = q_pair[s] + G * K;
        for (int f = clip_frames[s]; f < clip_frames[s + 1]; ++f) q_fc[f] = s;
        if (G * K > max_pairs) max_pairs = G * K;
    }
    for (int f = 0; f <= F; ++f) { q_go[f] = gt_off[f]; q_po[f] = pred_off[f]; }
    for (int f = 0; f < F; ++f) {
        const int64_t nk = (q_go[f + 1] - q_go[f]) * (q_po[f + 1] - q_po[f]);
        q_so[f + 1] = q_so[f] + nk;
        if (nk > max_block) max_block = nk;
    }
    block[B_GT_ROWS] = q_go[F]; block[B_PRED_ROWS] = q_po[F]; block[B_SIM] = q_so[F]; block[B_GTAB] = q_gtab[S]; block[B_PTAB] = q_ptab[S];
    block[B_PAIRS] = q_pair[S]; block[B_MAX_PAIRS] = max_pairs; block[B_MAX_BLOCK] = max_block;
    const char* why = bad_block(block);
    ROMP_REQUIRE(!why, "romp_mot_pack: inconsistent layout (%s)", why);
    return (int)words;
}

int romp_mot_workspace_bytes(const int64_t* block, int64_t* bytes) {
    const char* why = bad_block(block);
    ROMP_REQUIRE(!why, "romp_mot_workspace_bytes: bad block (%s)", why);
    ROMP_REQUIRE(bytes, "romp_mot_workspace_bytes: NULL argument");
    *bytes = (int64_t)carve(block, nullptr).bytes + 8;
    return ROMP_OK;
}

int romp_mot_boxes(const float* kp2d, int N, int J, double enlarge_x, double enlarge_y, double* boxes, void* stream) {
    ROMP_REQUIRE(kp2d && boxes && N >= 1 && J >= 1 && enlarge_x > 0. && enlarge_y > 0. && enlarge_x < 1e300 && enlarge_y < 1e300,
                 "romp_mot_boxes: bad arguments (N, J >= 1, enlarge > 0 and finite)");
    hipLaunchKernelGGL(mot_boxes_kernel, dim3((N + NT - 1) / NT), dim3(NT), 0, (hipStream_t)stream, kp2d, N, J, enlarge_x, enlarge_y, boxes);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_mot_tables(const int64_t* block, const int64_t* block_dev, const int32_t* gt_ids, const int32_t* pred_ids, void* workspace,
                    void* stream) {
    MOT_BLOCK("romp_mot_tables");
    ROMP_REQUIRE(workspace && (gt_ids || !block[B_GT_ROWS]) && (pred_ids || !block[B_PRED_ROWS]), "romp_mot_tables: NULL argument");
    if (!block[B_F]) return ROMP_OK;
    const Work w = carve(block, workspace);
    hipLaunchKernelGGL(mot_tables_kernel, dim3((unsigned)block[B_F]), dim3(64), 0, (hipStream_t)stream, block_dev, gt_ids, pred_ids, w.gtab, w.ptab);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_mot_similarity(const int64_t* block, const int64_t* block_dev, const float* gt_boxes, const int32_t* gt_ids, const float* pred_boxes,
                        const float* pred_kp2d, int J, double enlarge_x, double enlarge_y, const int32_t* pred_ids, double max_iou, double* sim,
                        double* rowsum, double* colsum, void* stream) {
    MOT_BLOCK("romp_mot_similarity");
    ROMP_REQUIRE(((gt_boxes && gt_ids && rowsum) || !block[B_GT_ROWS]) && ((pred_ids && colsum) || !block[B_PRED_ROWS]) && (sim || !block[B_SIM]),
                 "romp_mot_similarity: NULL argument");
    ROMP_REQUIRE(!block[B_PRED_ROWS] || (pred_boxes != nullptr) != (pred_kp2d != nullptr), "romp_mot_similarity: give pred_boxes or pred_kp2d, one of them");
    ROMP_REQUIRE(pred_boxes || !block[B_PRED_ROWS] || (J >= 1 && enlarge_x > 0. && enlarge_y > 0. && enlarge_x < 1e300 && enlarge_y < 1e300),
                 "romp_mot_similarity: J %d < 1 or an enlargement that is not positive and finite", J);
    ROMP_REQUIRE(max_iou >= 0. && max_iou <= 1., "romp_mot_similarity: max_iou outside 0..1");
    if (!block[B_F]) return ROMP_OK;
    hipLaunchKernelGGL(mot_similarity_kernel, dim3((unsigned)block[B_F]), dim3(NT), 0, (hipStream_t)stream, block_dev, gt_boxes, gt_ids, pred_boxes,
                       pred_kp2d, J, enlarge_x, enlarge_y, pred_ids, max_iou, sim, rowsum, colsum);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

#define MOT_SCORE_ARGS(name)                                                                                              \
    MOT_BLOCK(name);                                                                                                      \
    ROMP_REQUIRE(workspace && out && (gt_ids || !block[B_GT_ROWS]) && (pred_ids || !block[B_PRED_ROWS]) && (sim || !block[B_SIM]), \
                 name ": NULL argument")

int romp_mot_hota(const int64_t* block, const int64_t* block_dev, const int32_t* gt_ids, const int32_t* pred_ids, const double* sim,
                  const double* rowsum, const double* colsum, const double* alphas_host, void* workspace, double* out, void* stream) {
    MOT_SCORE_ARGS("romp_mot_hota");
    ROMP_REQUIRE(alphas_host && (rowsum || !block[B_GT_ROWS]) && (colsum || !block[B_PRED_ROWS]), "romp_mot_hota: NULL argument");
    Thresholds th;
    for (int a = 0; a < NA; ++a) {
        ROMP_REQUIRE(alphas_host[a] > 0. && alphas_host[a] <= 1. && (a == 0 || alphas_host[a] > alphas_host[a - 1]),
                     "romp_mot_hota: the alphas must increase within (0, 1]");
        th.v[a] = alphas_host[a] - DBL_EPSILON;
    }
    const Work w = carve(block, workspace);
    hipStream_t st = (hipStream_t)stream;
    const unsigned S = (unsigned)block[B_S], F = (unsigned)block[B_F];
    if (w.nblk)
        hipLaunchKernelGGL(mot_pair_walk_kernel<false>, dim3(w.nblk, S), dim3(NT), 0, st, block_dev, w.gtab, w.ptab, sim, rowsum, colsum, 0., w.A);
    if (F)
        hipLaunchKernelGGL(mot_hota_frame_kernel, dim3(F), dim3(64), 0, st, block_dev, gt_ids, pred_ids, sim, w.A, th, w.cost, w.match_col,
                           w.match_sim, w.frame_tp, w.frame_loc, w.frame_cnt);
    if (w.nblk)
        hipLaunchKernelGGL(mot_hota_pairs_kernel, dim3(w.nblk, S), dim3(NT), 0, st, block_dev, w.gtab, w.ptab, w.match_col, w.match_sim, th, w.nblk,
                           w.partial);
    hipLaunchKernelGGL(mot_hota_reduce_kernel, dim3(S), dim3(64), 0, st, block_dev, w.frame_tp, w.frame_loc, w.frame_cnt, w.partial, w.nblk, out);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_mot_clear(const int64_t* block, const int64_t* block_dev, const int32_t* gt_ids, const int32_t* pred_ids, const double* sim,
                   double threshold, void* workspace, double* out, void* stream) {
    MOT_SCORE_ARGS("romp_mot_clear");
    ROMP_REQUIRE(threshold > 0. && threshold <= 1., "romp_mot_clear: threshold outside (0, 1]");
    const Work w = carve(block, workspace);
    hipLaunchKernelGGL(mot_clear_kernel, dim3((unsigned)block[B_S]), dim3(64), 0, (hipStream_t)stream, block_dev, gt_ids, pred_ids, sim, threshold,
                       w.cost, out);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_mot_identity(const int64_t* block, const int64_t* block_dev, const int32_t* gt_ids, const int32_t* pred_ids, const double* sim,
                      double threshold, void* workspace, double* out, void* stream) {
    MOT_SCORE_ARGS("romp_mot_identity");
    ROMP_REQUIRE(threshold > 0. && threshold <= 1., "romp_mot_identity: threshold outside (0, 1]");
    const Work w = carve(block, workspace);
    hipStream_t st = (hipStream_t)stream;
    const unsigned S = (unsigned)block[B_S];
    if (w.nblk)
        hipLaunchKernelGGL(mot_pair_walk_kernel<true>, dim3(w.nblk, S), dim3(NT), 0, st, block_dev, w.gtab, w.ptab, sim, nullptr, nullptr, threshold,
                           w.A);
    hipLaunchKernelGGL(mot_identity_kernel, dim3(S), dim3(64), 0, st, block_dev, gt_ids, pred_ids, w.A, out);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

}  // extern "C"
