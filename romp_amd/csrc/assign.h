// assign.h -- the exact assignment solver of one wave, shared by track.hip (the association rounds of the tracker) and mot.hip (the
// per-frame and per-clip matchings of the tracking scores).  Float64; include it only in files compiled with -ffp-contract=off.
#pragma once
#include "common.h"
#include "../../include/romp_hip_track.h"

namespace romp {

constexpr int MAXC = ROMP_TRACK_MAX_CAPACITY;
constexpr double BIG = 1e300;

// lanes of ONE wave exchange values through the LDS: the LDS serves a wave's accesses in order, the fence keeps the compiler from moving them
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct SolveLds {
    double u[MAXC], v[MAXC + 1], minv[MAXC + 1];
    int way[MAXC + 1], p[MAXC + 1];
    unsigned char used[MAXC + 8];
};

// Exact assignment by shortest augmenting paths, rows entered one at a time.  Columns 0..m-1 are the real ones, column m is "stay
// unassigned": it costs `limit`, is never full and so ends every path that reaches it.  Minimises the sum over rows of (cost of
// the pair, or limit) = the sum of (cost - limit) over the pairs + n limit: the optimum of the reference's padded square matrix.
// A lane owns the columns j with j % 64 == lane (v, minv, way, used of a column are touched by that lane only); u and p are shared.
__device__ void wave_assign(int lane, const double* __restrict__ cost, int ld, int n, int m, double limit, SolveLds& L, int* pair) {
    const int M1 = m + 1;
    for (int j = lane; j < M1; j += 64) { L.v[j] = 0.; L.p[j] = -1; }
    for (int r = lane; r < n; r += 64) { L.u[r] = 0.; pair[r] = -1; }
    wave_sync();
    for (int i = 0; i < n; ++i) {
        for (int j = lane; j < M1; j += 64) { L.minv[j] = BIG; L.way[j] = -1; L.used[j] = 0; }
        int j0 = -1;
        for (int step = 0; step <= M1; ++step) {                     // (a path uses a column at most once)
            const int i0 = j0 < 0 ? i : L.p[j0];
            const double ui0 = L.u[i0];
            if (j0 >= 0 && (j0 & 63) == lane) L.used[j0] = 1;
            double best = BIG;
            int bj = M1;
            for (int j = lane; j < M1; j += 64) {
                if (!L.used[j]) {
                    const double c = (j < m ? cost[(size_t)i0 * ld + j] : limit) - ui0 - L.v[j];
                    double mv = L.minv[j];
                    if (c < mv) { mv = c; L.minv[j] = c; L.way[j] = j0; }
                    if (mv < best) { best = mv; bj = j; }
                }
            }
#pragma unroll
            for (int off = 32; off; off >>= 1) {                      // minimum over the wave, the lowest column on a tie
                const double ob = __shfl_xor(best, off);
                const int oj = __shfl_xor(bj, off);
                if (ob < best || (ob == best && oj < bj)) { best = ob; bj = oj; }
            }
            int j1 = bj;
            if (j1 >= M1) { j1 = m; best = 0.; }                      // nothing comparable left (NaN costs): stay unassigned
            wave_sync();
            for (int j = lane; j < M1; j += 64) {
                if (L.used[j]) { L.u[L.p[j]] += best; L.v[j] -= best; }
                else L.minv[j] -= best;
            }
            if (lane == 0) L.u[i] += best;
            wave_sync();
            j0 = j1;
            if (j0 == m || L.p[j0] < 0) break;
        }
        if (lane == 0) {                                              // augment along way[]
            while (j0 >= 0) {
                const int j1 = L.way[j0];
                const int r = j1 < 0 ? i : L.p[j1];
                if (j0 < m) { L.p[j0] = r; pair[r] = j0; }
                else pair[r] = -1;
                j0 = j1;
            }
        }
        wave_sync();
    }
}

}  // namespace romp
