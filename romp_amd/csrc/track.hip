// track.hip -- ByteTrack-3D association of BEV's video mode on the device (include/romp_hip_track.h).
//
// The mirror of romp_amd/tracker.py `Tracker.update` (itself the mirror of the reference's byte_tracker_3dcenter.py:21-160 and
// kalman_filter_3dcenter.py), decision for decision: one workgroup of four waves walks the frames of a call in order.  The
// parallel parts of a frame (prediction, cost matrices, corrections, duplicate test, nearest detection) use the whole workgroup
// between barriers; the ordered lists are built by wave 0 with ballots, so their order is the one union / minus give on the host;
// the assignment of a round is solved by wave 0 alone (wave_assign), columns across lanes, with no workgroup barrier inside.
// All arithmetic is float64 on the float32 inputs; this file is compiled with -ffp-contract=off (romp_amd/build.py) so that a
// sum of squares is the one numpy forms.  No atomics.
#include <string.h>
#include "common.h"
#include "../../include/romp_hip_track.h"
#include "assign.h"                                                    // wave_sync, SolveLds, wave_assign (shared with mot.hip)

namespace romp {

constexpr int MAXD = ROMP_TRACK_MAX_DET, MAXT = 1024, NT = 256;
constexpr int T_FREE = 0, T_TRACKED = 1, T_LOST = 2, T_REMOVED = 3;
constexpr double POS_W = 1. / 20, VEL_W = 1. / 160;      // kalman_filter_3dcenter.py:33-34

struct Slot {
    double mean[8], cov[64];
    float score;
    int state, confirmed, id, frame, born, hits, dropped;
};
static_assert(sizeof(Slot) == ROMP_TRACK_SLOT_BYTES, "the documented record size");

// header words (int32)
enum { H_CAP = 0, H_FRAME, H_LAST_ID, H_NTRACKED, H_NLOST, H_OVERFLOW, H_MAX_LOST, H_DET = 8, H_LOW = 9, H_MATCH = 16, H_DUP = 18, H_WORDS = 32 };

// the state buffer: header | row counts of a multi-frame call | table | tracked list | lost list | cost workspace
__host__ __device__ inline size_t off_rows() { return 4 * H_WORDS; }
__host__ __device__ inline size_t off_table() { return off_rows() + 4 * (size_t)MAXT; }
__host__ __device__ inline size_t off_tracked(int cap) { return off_table() + sizeof(Slot) * (size_t)cap; }
__host__ __device__ inline size_t off_lost(int cap) { return off_tracked(cap) + 4 * (size_t)cap; }
__host__ __device__ inline size_t off_cost(int cap) { return off_lost(cap) + 4 * (size_t)cap; }
__host__ __device__ inline size_t state_bytes(int cap) { return off_cost(cap) + 8 * (size_t)cap * MAXD; }

// ordered compaction by one wave: out[base ...] = f(i) for the i in 0..n-1 with f(i) >= 0, in the order of i; returns the new end
template <class F>
__device__ __forceinline__ int wave_compact(int lane, int n, int* out, int base, F f) {
    wave_sync();
    for (int i0 = 0; i0 < n; i0 += 64) {
        const int i = i0 + lane;
        const int v = i < n ? f(i) : -1;
        const unsigned long long m = __ballot(v >= 0);
        if (v >= 0) out[base + __popcll(m & ((1ull << lane) - 1ull))] = v;
        base += __popcll(m);
    }
    wave_sync();
    return base;
}

// ---------------------------------------------------------------------------------------------- the Kalman filter
__device__ void kf_start(Slot& s, const double* z) {                   // initiate (:36-66)
    const double sp = 2 * POS_W * z[3], sv = 10 * VEL_W * z[3];
    for (int i = 0; i < 8; ++i) s.mean[i] = i < 4 ? z[i] : 0.;
    for (int i = 0; i < 64; ++i) s.cov[i] = 0.;
    for (int i = 0; i < 8; ++i) s.cov[i * 9] = i < 4 ? sp * sp : sv * sv;
}

__device__ void kf_predict(Slot& s) {                                  // multi_predict (:131-164); a lost track coasts with vh = 0
    double m[8], P[64], Q[64];
    for (int i = 0; i < 8; ++i) m[i] = s.mean[i];
    for (int i = 0; i < 64; ++i) P[i] = s.cov[i];
    if (s.state != T_TRACKED) m[7] = 0.;
    const double qp = (POS_W * m[3]) * (POS_W * m[3]), qv = (VEL_W * m[3]) * (VEL_W * m[3]);
    for (int i = 0; i < 8; ++i)
        for (int l = 0; l < 8; ++l) {                                  // F P F^T, F = [[I, I], [0, I]]
            double a = P[i * 8 + l];
            if (l < 4) a += P[i * 8 + l + 4];
            if (i < 4) {
                a += P[(i + 4) * 8 + l];
                if (l < 4) a += P[(i + 4) * 8 + l + 4];
            }
            Q[i * 8 + l] = a;
        }
    for (int i = 0; i < 8; ++i) Q[i * 9] += i < 4 ? qp : qv;
    for (int i = 0; i < 4; ++i) m[i] = m[i] + m[i + 4];
    for (int i = 0; i < 8; ++i) s.mean[i] = m[i];
    for (int i = 0; i < 64; ++i) s.cov[i] = Q[i];
}

__device__ void kf_correct(Slot& s, const double* z) {                 // update (:166-194)
    double m[8], P[64], S[16], X[32];                                  // X (4,8): S X = (P H^T)^T, K = X^T
    for (int i = 0; i < 8; ++i) m[i] = s.mean[i];
    for (int i = 0; i < 64; ++i) P[i] = s.cov[i];
    const double r = (POS_W * m[3]) * (POS_W * m[3]);
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) S[a * 4 + b] = P[a * 8 + b] + (a == b ? r : 0.);
    for (int a = 0; a < 4; ++a)
        for (int i = 0; i < 8; ++i) X[a * 8 + i] = P[i * 8 + a];
    double A[16];
    for (int i = 0; i < 16; ++i) A[i] = S[i];
    for (int k = 0; k < 4; ++k) {                                      // LU with partial pivoting, as LAPACK's gesv
        int piv = k;
        double big = fabs(A[k * 4 + k]);
        for (int a = k + 1; a < 4; ++a)
            if (fabs(A[a * 4 + k]) > big) { big = fabs(A[a * 4 + k]); piv = a; }
        if (piv != k) {
            for (int b = 0; b < 4; ++b) { const double t = A[k * 4 + b]; A[k * 4 + b] = A[piv * 4 + b]; A[piv * 4 + b] = t; }
            for (int i = 0; i < 8; ++i) { const double t = X[k * 8 + i]; X[k * 8 + i] = X[piv * 8 + i]; X[piv * 8 + i] = t; }
        }
        for (int a = k + 1; a < 4; ++a) {
            const double f = A[a * 4 + k] / A[k * 4 + k];
            for (int b = k + 1; b < 4; ++b) A[a * 4 + b] -= f * A[k * 4 + b];
            for (int i = 0; i < 8; ++i) X[a * 8 + i] -= f * X[k * 8 + i];
        }
    }
    for (int k = 3; k >= 0; --k)
        for (int i = 0; i < 8; ++i) {
            double t = X[k * 8 + i];
            for (int b = k + 1; b < 4; ++b) t -= A[k * 4 + b] * X[b * 8 + i];
            X[k * 8 + i] = t / A[k * 4 + k];
        }
    double inn[4];
    for (int a = 0; a < 4; ++a) inn[a] = z[a] - m[a];
    for (int i = 0; i < 8; ++i) {
        double t = 0.;
        for (int a = 0; a < 4; ++a) t += inn[a] * X[a * 8 + i];
        s.mean[i] = m[i] + t;
    }
    double KS[32];                                                     // (8,4) = K S
    for (int i = 0; i < 8; ++i)
        for (int b = 0; b < 4; ++b) {
            double t = 0.;
            for (int a = 0; a < 4; ++a) t += X[a * 8 + i] * S[a * 4 + b];
            KS[i * 4 + b] = t;
        }
    for (int i = 0; i < 8; ++i)
        for (int l = 0; l < 8; ++l) {
            double t = 0.;
            for (int b = 0; b < 4; ++b) t += KS[i * 4 + b] * X[b * 8 + l];
            s.cov[i * 8 + l] = P[i * 8 + l] - t;
        }
}

__device__ __forceinline__ void absorb(Slot& s, const double* z, float score, int frame) {   // STrack.update / re_activate
    kf_correct(s, z);
    s.hits = s.state == T_TRACKED ? s.hits + 1 : 0;
    s.state = T_TRACKED; s.confirmed = 1; s.frame = frame; s.score = score;
}

__device__ __forceinline__ double dist4(const double* a, const double* b) {
    const double d0 = a[0] - b[0], d1 = a[1] - b[1], d2 = a[2] - b[2], d3 = a[3] - b[3];
    return sqrt(((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3);
}

struct FrameLds {
    SolveLds solve;
    double pts[MAXD * 4];
    float sc[MAXD];
    int tracked[MAXC], lost[MAXC], pool[MAXC], tent[MAXC], still[MAXC], pair[MAXC], live[MAXC], newlost[MAXC], lostnew[MAXC],
        freeslot[MAXC], reset_at[MAXC];
    int det[MAXD], rest[MAXD], birth[MAXD];
    unsigned char used[MAXC], reported[MAXC], fresh0[MAXC], kill_live[MAXC], kill_lost[MAXC], timedout[MAXC], keep[MAXC], detused[MAXD], restused[MAXD];
    int n[16];
};

// one association round on rows[0..n) (table slots) x cols[0..m) (rows of the frame); pair[r] = index into cols or -1
__device__ void match_round(FrameLds& L, Slot* tab, double* W, const int* rows, int n, const int* cols, int m, double limit,
                            int frame, unsigned char* colused) {
    const int tid = threadIdx.x;
    if (n == 0 || m == 0) {                                            // (assign: everything stays unmatched)
        for (int r = tid; r < n; r += NT) L.pair[r] = -1;
        __syncthreads();
        return;
    }
    for (int idx = tid; idx < n * m; idx += NT) {
        const int r = idx / m, c = idx - r * m;
        W[idx] = dist4(tab[rows[r]].mean, L.pts + 4 * cols[c]);
    }
    __syncthreads();
    if (tid < 64) wave_assign(tid, W, m, n, m, limit, L.solve, L.pair);
    __syncthreads();
    for (int r = tid; r < n; r += NT) {
        const int c = L.pair[r];
        if (c >= 0) {
            absorb(tab[rows[r]], L.pts + 4 * cols[c], L.sc[cols[c]], frame);
            if (colused) colused[c] = 1;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(NT) void track_frames_kernel(unsigned char* __restrict__ state, const float* __restrict__ points,
                                                          const float* __restrict__ scores, int T, int single_rows,
                                                          int32_t* __restrict__ out_count, int32_t* __restrict__ out_ids,
                                                          int32_t* __restrict__ out_rows, int32_t* __restrict__ out_slots,
                                                          float* __restrict__ flags, int stride) {
    __shared__ FrameLds L;
    const int tid = threadIdx.x;
    int* hdr = (int*)state;
    const int cap = hdr[H_CAP];
    if (cap < 1 || cap > MAXC) return;                                 // not a state of romp_track_init
    Slot* tab = (Slot*)(state + off_table());
    int* g_tracked = (int*)(state + off_tracked(cap)), *g_lost = (int*)(state + off_lost(cap));
    const int* g_rows = (const int*)(state + off_rows());
    double* W = (double*)(state + off_cost(cap));
    int frame = hdr[H_FRAME], last_id = hdr[H_LAST_ID], n_tracked = hdr[H_NTRACKED], n_lost = hdr[H_NLOST], overflow = hdr[H_OVERFLOW];
    const int max_lost = hdr[H_MAX_LOST];
    const float det_th = __int_as_float(hdr[H_DET]), low_th = __int_as_float(hdr[H_LOW]);
    const double match = *(const double*)(hdr + H_MATCH), dup = *(const double*)(hdr + H_DUP);
    for (int s = tid; s < cap; s += NT) {
        L.used[s] = tab[s].state != T_FREE;
        L.reported[s] = 0;
        L.fresh0[s] = 0;
        L.reset_at[s] = -1;
        if (s < n_tracked) L.tracked[s] = g_tracked[s];
        if (s < n_lost) L.lost[s] = g_lost[s];
    }
    __syncthreads();
    int row0 = 0;
    for (int t = 0; t < T; ++t) {
        const int N = T == 1 ? single_rows : g_rows[t];
        int nout = 0;
        if (N > 0) {
            ++frame;
            for (int i = tid; i < N; i += NT) {
                for (int k = 0; k < 4; ++k) L.pts[4 * i + k] = (double)points[(size_t)(row0 + i) * 4 + k];
                L.sc[i] = scores[row0 + i];
            }
            __syncthreads();
            // ---- strong / weak detections (float32 comparisons), confirmed / tentative tracks, the pool = confirmed + lost
            if (tid < 64) {
                const int ns = wave_compact(tid, N, L.det, 0, [&](int i) { return L.sc[i] > det_th ? i : -1; });
                int weak = 0;
                for (int i0 = 0; i0 < N; i0 += 64) {
                    const int i = i0 + tid;
                    weak |= __ballot(i < N && L.sc[i] > low_th && L.sc[i] < det_th) != 0ull;
                }
                const int nconf = wave_compact(tid, n_tracked, L.pool, 0, [&](int k) { return tab[L.tracked[k]].confirmed ? L.tracked[k] : -1; });
                const int ntent = wave_compact(tid, n_tracked, L.tent, 0, [&](int k) { return tab[L.tracked[k]].confirmed ? -1 : L.tracked[k]; });
                const int npool = wave_compact(tid, n_lost, L.pool, nconf, [&](int k) { return L.lost[k]; });
                if (tid == 0) { L.n[0] = ns; L.n[1] = weak; L.n[2] = ntent; L.n[3] = npool; }
            }
            __syncthreads();
            const int ns = L.n[0], any_weak = L.n[1], ntent = L.n[2], npool = L.n[3];
            for (int r = tid; r < npool; r += NT) kf_predict(tab[L.pool[r]]);
            for (int c = tid; c < MAXD; c += NT) { L.detused[c] = 0; L.restused[c] = 0; }
            __syncthreads();
            // ---- round 1: pool x strong
            match_round(L, tab, W, L.pool, npool, L.det, ns, match, frame, L.detused);
            if (tid < 64) {
                const int nstill = wave_compact(tid, npool, L.still, 0,
                                                [&](int r) { return L.pair[r] < 0 && tab[L.pool[r]].state == T_TRACKED ? L.pool[r] : -1; });
                const int nrest = wave_compact(tid, ns, L.rest, 0, [&](int c) { return L.detused[c] ? -1 : L.det[c]; });
                if (tid == 0) { L.n[4] = nstill; L.n[5] = nrest; }
            }
            __syncthreads();
            const int nstill = L.n[4], nrest = L.n[5];
            // ---- round 2: the still-tracked x the STRONG detections again, only when some weak one exists (kept quirk)
            match_round(L, tab, W, L.still, nstill, L.det, any_weak ? ns : 0, match * 2, frame, nullptr);
            for (int r = tid; r < nstill; r += NT)
                if (L.pair[r] < 0) tab[L.still[r]].state = T_LOST;
            if (tid < 64) {
                const int nnl = wave_compact(tid, nstill, L.newlost, 0, [&](int r) { return L.pair[r] < 0 ? L.still[r] : -1; });
                if (tid == 0) L.n[6] = nnl;
            }
            __syncthreads();
            const int nnewlost = L.n[6];
            // ---- round 3: tentative x leftover; an unmatched tentative track is removed
            match_round(L, tab, W, L.tent, ntent, L.rest, nrest, match * 3, frame, L.restused);
            for (int r = tid; r < ntent; r += NT)
                if (L.pair[r] < 0) tab[L.tent[r]].state = T_REMOVED;
            // ---- births in the free slots, lowest first
            if (tid < 64) {
                const int nb = wave_compact(tid, nrest, L.birth, 0, [&](int c) { return L.restused[c] ? -1 : L.rest[c]; });
                const int nfree = wave_compact(tid, cap, L.freeslot, 0,
                                               [&](int s) { return !L.used[s] && !(flags && L.reported[s] && L.reset_at[s] >= 0) ? s : -1; });
                if (tid == 0) { L.n[7] = nb; L.n[8] = nfree; }
            }
            __syncthreads();
            const int nb = L.n[7], nok = min(nb, L.n[8]);
            for (int k = tid; k < nok; k += NT) {
                const int slot = L.freeslot[k], i = L.birth[k];
                Slot& s = tab[slot];
                kf_start(s, L.pts + 4 * i);
                s.score = L.sc[i];
                s.state = T_TRACKED; s.confirmed = frame == 1; s.id = last_id + k + 1; s.frame = frame; s.born = frame; s.hits = 0; s.dropped = 0;
                L.used[slot] = 1;
                // the filter of this slot starts afresh: at once, or -- if the slot's earlier track was reported in this call -- from frame t on
                // (-(t + 1): with the history it has up to there; -(t + 1.5): afresh at the start of the call as well)
                if (L.reported[slot]) {
                    L.reset_at[slot] = t; L.reported[slot] = 0;
                    if (flags) flags[(size_t)slot * stride] = -((float)(t + 1) + (L.fresh0[slot] ? 0.5f : 0.f));
                } else if (L.reset_at[slot] < 0) {
                    L.fresh0[slot] = 1;
                    if (flags) flags[(size_t)slot * stride] = 0.f;
                }
            }
            last_id += nok;
            overflow += nb - nok;
            // ---- lost tracks past the buffer are removed (they leave the lost list one frame later)
            for (int k = tid; k < n_lost; k += NT) {
                Slot& s = tab[L.lost[k]];
                const bool out = frame - s.frame > max_lost;
                if (out) s.state = T_REMOVED;
                L.timedout[k] = out;
            }
            __syncthreads();
            // ---- live = tracked that still are + births + revived;  lost = (lost - live) + newly lost, minus the once-removed
            if (tid < 64) {
                int nl = wave_compact(tid, n_tracked, L.live, 0, [&](int k) { return tab[L.tracked[k]].state == T_TRACKED ? L.tracked[k] : -1; });
                nl = wave_compact(tid, nok, L.live, nl, [&](int k) { return L.freeslot[k]; });
                nl = wave_compact(tid, n_lost, L.live, nl, [&](int k) { return tab[L.lost[k]].state == T_TRACKED ? L.lost[k] : -1; });
                int nlo = wave_compact(tid, n_lost, L.lostnew, 0, [&](int k) {
                    const Slot& s = tab[L.lost[k]];
                    return s.state != T_TRACKED && !s.dropped ? L.lost[k] : -1; });
                nlo = wave_compact(tid, nnewlost, L.lostnew, nlo, [&](int k) { return tab[L.newlost[k]].dropped ? -1 : L.newlost[k]; });
                if (tid == 0) { L.n[9] = nl; L.n[10] = nlo; }
            }
            __syncthreads();
            const int nl = L.n[9], nlo = L.n[10];
            for (int k = tid; k < n_lost; k += NT)
                if (L.timedout[k]) tab[L.lost[k]].dropped = 1;
            // ---- duplicates: a live and a lost track closer than dup in (x, y): the younger one goes
            for (int a = tid; a < nl; a += NT) {
                const Slot& sa = tab[L.live[a]];
                const int age = sa.frame - sa.born;
                bool kill = false;
                for (int b = 0; b < nlo; ++b) {
                    const Slot& sb = tab[L.lostnew[b]];
                    const double dx = sa.mean[0] - sb.mean[0], dy = sa.mean[1] - sb.mean[1];
                    if (sqrt(dx * dx + dy * dy) < dup && !(age > sb.frame - sb.born)) kill = true;
                }
                L.kill_live[a] = kill;
            }
            for (int b = tid; b < nlo; b += NT) {
                const Slot& sb = tab[L.lostnew[b]];
                const int age = sb.frame - sb.born;
                bool kill = false;
                for (int a = 0; a < nl; ++a) {
                    const Slot& sa = tab[L.live[a]];
                    const double dx = sa.mean[0] - sb.mean[0], dy = sa.mean[1] - sb.mean[1];
                    if (sqrt(dx * dx + dy * dy) < dup && sa.frame - sa.born > age) kill = true;
                }
                L.kill_lost[b] = kill;
            }
            for (int s = tid; s < cap; s += NT) L.keep[s] = 0;
            __syncthreads();
            if (tid < 64) {
                const int nt2 = wave_compact(tid, nl, L.tracked, 0, [&](int a) { return L.kill_live[a] ? -1 : L.live[a]; });
                const int nl2 = wave_compact(tid, nlo, L.lost, 0, [&](int b) { return L.kill_lost[b] ? -1 : L.lostnew[b]; });
                const int no = wave_compact(tid, nt2, L.pool, 0, [&](int k) { return tab[L.tracked[k]].confirmed ? L.tracked[k] : -1; });
                if (tid == 0) { L.n[11] = nt2; L.n[12] = nl2; L.n[13] = no; }
            }
            __syncthreads();
            n_tracked = L.n[11]; n_lost = L.n[12]; nout = L.n[13];
            for (int k = tid; k < n_tracked; k += NT) L.keep[L.tracked[k]] = 1;
            for (int k = tid; k < n_lost; k += NT) L.keep[L.lost[k]] = 1;
            // ---- what is reported: the confirmed tracks, each with the nearest detection of the frame (first minimum).  A row with a
            // non-finite coordinate is at no comparable distance, wherever it stands: it is never the nearest of a finite track
            for (int k = tid; k < nout; k += NT) {
                const int slot = L.pool[k];
                const Slot& s = tab[slot];
                double bd = INFINITY;
                int bi = 0;
                for (int i = 0; i < N; ++i) {
                    const double d = dist4(L.pts + 4 * i, s.mean);
                    if (d < bd) { bd = d; bi = i; }
                }
                out_ids[(size_t)t * cap + k] = s.id;
                out_rows[(size_t)t * cap + k] = row0 + bi;
                out_slots[(size_t)t * cap + k] = slot;
                L.reported[slot] = 1;
            }
            __syncthreads();
            for (int s = tid; s < cap; s += NT)
                if (L.used[s] && !L.keep[s]) { L.used[s] = 0; tab[s].state = T_FREE; }
            __syncthreads();
        }
        if (tid == 0) out_count[t] = nout;
        for (int k = nout + tid; k < cap; k += NT) {
            out_ids[(size_t)t * cap + k] = -1; out_rows[(size_t)t * cap + k] = 0; out_slots[(size_t)t * cap + k] = -1;
        }
        row0 += N;
    }
    for (int s = tid; s < cap; s += NT) {
        g_tracked[s] = s < n_tracked ? L.tracked[s] : -1;              // (the tails too: the state is a function of the frames seen, not of how calls cut them)
        g_lost[s] = s < n_lost ? L.lost[s] : -1;
    }
    if (tid == 0) { hdr[H_FRAME] = frame; hdr[H_LAST_ID] = last_id; hdr[H_NTRACKED] = n_tracked; hdr[H_NLOST] = n_lost; hdr[H_OVERFLOW] = overflow; }
}

__global__ __launch_bounds__(64) void track_assign_kernel(const double* __restrict__ cost, int n, int m, double limit, int32_t* __restrict__ pair_of_row) {
    __shared__ SolveLds L;
    __shared__ int pair[MAXC];
    wave_assign(threadIdx.x, cost, m, n, m, limit, L, pair);
    for (int r = threadIdx.x; r < n; r += 64) pair_of_row[r] = pair[r];
}

__global__ __launch_bounds__(NT) void track_list_kernel(const unsigned char* __restrict__ state, double* __restrict__ records, int32_t* __restrict__ count) {
    const int* hdr = (const int*)state;
    const int cap = hdr[H_CAP];
    if (cap < 1 || cap > MAXC) return;
    const Slot* tab = (const Slot*)(state + off_table());
    const int* g_tracked = (const int*)(state + off_tracked(cap)), *g_lost = (const int*)(state + off_lost(cap));
    const int nt = hdr[H_NTRACKED], nl = hdr[H_NLOST];
    if (threadIdx.x == 0) { count[0] = nt; count[1] = nl; }
    for (int k = threadIdx.x; k < nt + nl; k += NT) {
        const Slot& s = tab[k < nt ? g_tracked[k] : g_lost[k - nt]];
        double* r = records + (size_t)k * ROMP_TRACK_RECORD;
        r[0] = s.id; r[1] = s.state; r[2] = s.confirmed; r[3] = s.frame; r[4] = s.born; r[5] = s.score;
        for (int i = 0; i < 8; ++i) r[6 + i] = s.mean[i];
    }
}

}  // namespace romp

using namespace romp;

extern "C" {

int romp_track_state_bytes(int capacity) {
    ROMP_REQUIRE(capacity >= 1 && capacity <= MAXC, "romp_track_state_bytes: capacity %d outside 1..%d", capacity, MAXC);
    return (int)state_bytes(capacity);
}

int romp_track_init(void* state, int capacity, int first_id, float det_thresh, float low_thresh, double match_thresh, int max_time_lost,
                    double dup_thresh, void* stream) {
    ROMP_REQUIRE(state && capacity >= 1 && capacity <= MAXC && first_id >= 0 && det_thresh >= 0.f && low_thresh >= 0.f &&
                 match_thresh >= 0. && match_thresh < 1e300 && dup_thresh >= 0. && dup_thresh < 1e300 && max_time_lost >= 0,
                 "romp_track_init: bad arguments (capacity 1..%d, first_id >= 0, thresholds >= 0 and finite)", MAXC);
    int32_t h[H_WORDS] = {0};
    h[H_CAP] = capacity; h[H_LAST_ID] = first_id; h[H_MAX_LOST] = max_time_lost;
    memcpy(h + H_DET, &det_thresh, 4); memcpy(h + H_LOW, &low_thresh, 4);
    memcpy(h + H_MATCH, &match_thresh, 8); memcpy(h + H_DUP, &dup_thresh, 8);
    ROMP_HIP_CHECK(hipMemsetAsync(state, 0, state_bytes(capacity), (hipStream_t)stream));
    ROMP_HIP_CHECK(hipMemcpyAsync(state, h, sizeof(h), hipMemcpyHostToDevice, (hipStream_t)stream));   // (pageable source: staged before return)
    return ROMP_OK;
}

int romp_track_frames(void* state, const float* points, const float* scores, const int32_t* frame_rows_host, int T, int32_t* out_count,
                      int32_t* out_ids, int32_t* out_rows, int32_t* out_slots, float* oneeuro_flags, int oneeuro_stride, void* stream) {
    ROMP_REQUIRE(state && points && scores && frame_rows_host && out_count && out_ids && out_rows && out_slots,
                 "romp_track_frames: NULL argument");
    ROMP_REQUIRE(T >= 1 && T <= MAXT, "romp_track_frames: T %d outside 1..%d", T, MAXT);
    ROMP_REQUIRE(!oneeuro_flags || oneeuro_stride >= 1, "romp_track_frames: oneeuro_stride %d", oneeuro_stride);
    for (int t = 0; t < T; ++t)
        ROMP_REQUIRE(frame_rows_host[t] >= 0 && frame_rows_host[t] <= MAXD, "romp_track_frames: frame %d has %d rows, outside 0..%d", t,
                     frame_rows_host[t], MAXD);
    hipStream_t st = (hipStream_t)stream;
    if (T > 1)                                                         // the row counts ride in the state (pageable source: staged before return); T == 1: in the launch
        ROMP_HIP_CHECK(hipMemcpyAsync((unsigned char*)state + off_rows(), frame_rows_host, 4 * (size_t)T, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(track_frames_kernel, dim3(1), dim3(NT), 0, st, (unsigned char*)state, points, scores, T, frame_rows_host[0], out_count,
                       out_ids, out_rows, out_slots, oneeuro_flags, oneeuro_stride);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_track_assign(const double* cost, int n, int m, double limit, int32_t* pair_of_row, void* stream) {
    ROMP_REQUIRE(cost && pair_of_row && n >= 1 && n <= MAXC && m >= 1 && m <= MAXC && limit > -1e300 && limit < 1e300,
                 "romp_track_assign: bad arguments (1 <= n, m <= %d, a finite limit)", MAXC);
    hipLaunchKernelGGL(track_assign_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, cost, n, m, limit, pair_of_row);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_track_list(const void* state, double* records, int32_t* count, void* stream) {
    ROMP_REQUIRE(state && records && count, "romp_track_list: NULL argument");
    hipLaunchKernelGGL(track_list_kernel, dim3(1), dim3(NT), 0, (hipStream_t)stream, (const unsigned char*)state, records, count);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

}  // extern "C"
