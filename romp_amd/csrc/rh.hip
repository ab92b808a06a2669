// rh.hip -- the Relative Human benchmark on the device (include/romp_hip_rh.h): per matched person PCKh, per image the
// depth-relation counts (equal / ordered, per age group) and the missed persons, and a float64 running accumulator.
//
// Reference: simple_romp/evaluation/RH_evaluation/evaluation.py _calc_matched_PCKh_ :71-88, _calc_relative_depth_error_weak_
// :37-69, get_results :101-123; the matching before it is romp_eval_match2d (eval.hip).
//
// score_kernel: one wave per image.  Lanes stride over the image's ground-truth rows (PCKh, misses), compact the matched
// rows that carry a depth id into LDS in ascending row order (ballot + popcount, no atomics), then stride over the
// n (n - 1) / 2 pairs.  Every count is an integer folded across the wave by shuffles: the outputs are deterministic.
// accumulate_kernel: one workgroup, one column after the other.
#include "common.h"
#include "../../include/romp_hip_rh.h"
#include <math.h>

namespace romp {

constexpr int RH_MAX_GT = 4096;                                    // 12 bytes of LDS a row; n (n - 1) / 2 stays far inside int32
constexpr int RH_ACC_THREADS = 256, RH_ACC_WAVES = RH_ACC_THREADS / 64;
constexpr int RH_N_SUMS = ROMP_RH_OVER_CAP;                        // the counts a wave folds: every column before the flag

__device__ __forceinline__ int wave_sum(int v) {
    for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// first member i of pair k among the pairs (i < j) of n rows listed row by row: the largest i with start(i) <= k,
// start(i) = i (2n - i - 1) / 2.  The float64 root is a first guess; the two loops make it exact.
__device__ __forceinline__ int pair_row(int k, int n) {
    const double t = 2.0 * n - 1.0;
    int i = (int)((t - sqrt(fmax(t * t - 8.0 * (double)k, 0.0))) * 0.5);
    i = min(max(i, 0), n - 2);
    while (i > 0 && i * (2 * n - i - 1) / 2 > k) --i;
    while (i < n - 2 && (i + 1) * (2 * n - i - 2) / 2 <= k) ++i;
    return i;
}

__global__ __launch_bounds__(64) void score_kernel(const float* __restrict__ pkp, const float* __restrict__ pdepth, int Np,
                                                   const float* __restrict__ gkp, const int32_t* __restrict__ gdid,
                                                   const int32_t* __restrict__ gage, const int32_t* __restrict__ pred_of_gt, int Ng,
                                                   const int32_t* __restrict__ goff, int J, int max_gt, float dr_thresh,
                                                   float pck_thresh, float* __restrict__ pckh, int32_t* __restrict__ cv,
                                                   int32_t* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float* s_depth = (float*)lds_raw;                              // (max_gt) predicted depth of a compacted row
    int32_t* s_id = (int32_t*)(s_depth + max_gt);                  // (max_gt) its depth id
    int32_t* s_age = s_id + max_gt;                                // (max_gt) its age
    const int b = blockIdx.x, lane = threadIdx.x;
    const int g0 = min(max(goff[b], 0), Ng), g1 = min(max(goff[b + 1], g0), Ng);
    const int G = g1 - g0;
    int32_t* row = counts + (size_t)b * ROMP_RH_COUNTS;
    if (G > max_gt) {                                              // flagged, never truncated
        const float nan = __builtin_nanf("");
        for (int i = lane; i < G; i += 64) {
            if (pckh) pckh[g0 + i] = nan;
            if (cv) { cv[2 * (size_t)(g0 + i)] = 0; cv[2 * (size_t)(g0 + i) + 1] = 0; }
        }
        if (lane < ROMP_RH_COUNTS) row[lane] = lane == ROMP_RH_OVER_CAP ? 1 : 0;
        return;
    }
    int c[RH_N_SUMS];
#pragma unroll
    for (int k = 0; k < RH_N_SUMS; ++k) c[k] = 0;

    // the rows: PCKh of a matched one, the missed ones by age, and the compaction of those that take part in the pairs
    int n = 0;                                                     // the same in every lane
    for (int base = 0; base < G; base += 64) {
        const int i = base + lane;
        bool take = false;
        float depth = 0.f;
        int did = -1, age = -1;
        if (i < G) {
            const int g = g0 + i, p = pred_of_gt[g];
            age = gage[g];
            if (p < 0 || p >= Np) {
                ++c[ROMP_RH_MISSED];
#pragma unroll
                for (int a = 0; a < 4; ++a) c[ROMP_RH_MISSED_AGE + a] += age == a;      // (constant indices: c stays in registers)
                if (pckh) pckh[g] = __builtin_nanf("");
                if (cv) { cv[2 * (size_t)g] = 0; cv[2 * (size_t)g + 1] = 0; }
            } else {
                const float* a = pkp + (size_t)p * J * 2;
                const float* t = gkp + (size_t)g * J * 2;
                float x1 = INFINITY, x2 = -INFINITY, y1 = INFINITY, y2 = -INFINITY;
                int visible = 0;
                for (int j = 0; j < J; ++j) {
                    const float x = t[2 * j], y = t[2 * j + 1];
                    if (x > -1.f && y > -1.f) {
                        ++visible;
                        x1 = fminf(x1, x); x2 = fmaxf(x2, x); y1 = fminf(y1, y); y2 = fmaxf(y2, y);
                    }
                }
                int correct = 0;
                float value = -1.f;
                if (visible >= 2) {
                    const float w = x2 - x1, h = y2 - y1;
                    const float scale = sqrtf(w * w + h * h);
                    for (int j = 0; j < J; ++j) {
                        const float x = t[2 * j], y = t[2 * j + 1];
                        if (x > -1.f && y > -1.f) {
                            const float dx = x - a[2 * j], dy = y - a[2 * j + 1];
                            if (sqrtf(dx * dx + dy * dy) / scale < pck_thresh) ++correct;      // 0/0 and x/0: not correct
                        }
                    }
                    value = (float)correct / (float)visible;
                } else {
                    ++c[ROMP_RH_UNSCORED];
                }
                ++c[ROMP_RH_MATCHED];
                if (pckh) pckh[g] = value;
                if (cv) { cv[2 * (size_t)g] = correct; cv[2 * (size_t)g + 1] = visible; }
                did = gdid[g];
                take = did != -1;
                depth = pdepth[p];
            }
        }
        const unsigned long long mask = __ballot(take);
        if (take) {
            const int at = n + __popcll(mask & ((1ull << lane) - 1ull));
            s_depth[at] = depth; s_id[at] = did; s_age[at] = age;
        }
        n += __popcll(mask);
    }
    __syncthreads();

    // the pairs
    const int n_pairs = n * (n - 1) / 2;
    for (int k = lane; k < n_pairs; k += 64) {
        const int i = pair_row(k, n);
        const int j = i + 1 + (k - i * (2 * n - i - 1) / 2);
        const float dist = s_depth[j] - s_depth[i];
        const int did = s_id[j] - s_id[i];
        const bool ok = did == 0 ? fabsf(dist) < dr_thresh : (did < 0 ? dist < -dr_thresh : dist > dr_thresh);
        if (did == 0) { ++c[ROMP_RH_EQ_PAIRS]; c[ROMP_RH_EQ_CORRECT] += ok; }
        else { ++c[ROMP_RH_ORD_PAIRS]; c[ROMP_RH_ORD_CORRECT] += ok; }
        const int ai = s_age[i], aj = s_age[j];
#pragma unroll
        for (int a = 0; a < 4; ++a)
            if (ai == a || aj == a) { ++c[ROMP_RH_AGE_PAIRS + 2 * a]; c[ROMP_RH_AGE_CORRECT + 2 * a] += ok; }
    }
#pragma unroll
    for (int k = 0; k < RH_N_SUMS; ++k) c[k] = wave_sum(c[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < RH_N_SUMS; ++k) row[k] = c[k];
        row[ROMP_RH_OVER_CAP] = 0;
    }
}

// the sum of one value per thread: wave shuffle -> LDS -> the waves' sums in index order; every thread gets it
__device__ __forceinline__ double rh_block_sum(double x, double* s_part) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int m = 32; m >= 1; m >>= 1) x += __shfl_down(x, m, 64);
    if (lane == 0) s_part[wave] = x;
    __syncthreads();
    double s = 0.0;
    for (int w = 0; w < RH_ACC_WAVES; ++w) s += s_part[w];
    __syncthreads();                                               // s_part is free for the next sum
    return s;
}

__global__ __launch_bounds__(RH_ACC_THREADS) void rh_accumulate_kernel(const int32_t* __restrict__ counts, int B,
                                                                        const float* __restrict__ pckh, int Ng,
                                                                        const int32_t* __restrict__ gt_of_pred, int Np,
                                                                        double* __restrict__ acc) {
    __shared__ double s_part[RH_ACC_WAVES];
    const int tid = threadIdx.x;
    for (int k = 0; k < ROMP_RH_COUNTS; ++k) {
        double v = 0.0;
        for (int b = tid; b < B; b += RH_ACC_THREADS) v += (double)counts[(size_t)b * ROMP_RH_COUNTS + k];
        v = rh_block_sum(v, s_part);
        if (tid == 0) acc[k] += v;
    }
    double s = 0.0, fp = 0.0;
    for (int i = tid; i < Ng; i += RH_ACC_THREADS) {
        const float x = pckh[i];
        if (x >= 0.f) s += (double)x;                              // not the -1 rows, not the NaN of a miss
    }
    for (int i = tid; i < Np; i += RH_ACC_THREADS) fp += gt_of_pred[i] < 0 ? 1.0 : 0.0;
    s = rh_block_sum(s, s_part);
    fp = rh_block_sum(fp, s_part);
    if (tid == 0) {
        acc[ROMP_RH_ACC_PCKH_SUM] += s;
        acc[ROMP_RH_ACC_N_GT] += (double)Ng;
        acc[ROMP_RH_ACC_N_PRED] += (double)Np;
        acc[ROMP_RH_ACC_FALSE_POS] += fp;
    }
}

}  // namespace romp

using namespace romp;

extern "C" {

int romp_rh_score(const float* pred_kp2d, const float* pred_depth, int Np, const float* gt_kp2d, const int32_t* gt_depth_id,
                  const int32_t* gt_age, const int32_t* pred_of_gt, int Ng, const int32_t* gt_offsets, int B, int J, int max_gt,
                  float dr_thresh, float pck_thresh, float* pckh, int32_t* correct_visible, int32_t* counts, void* stream) {
    ROMP_REQUIRE(gt_offsets && counts && B > 0 && J > 0 && Np >= 0 && Ng >= 0,
                 "romp_rh_score: bad arguments (B %d, J %d, Np %d, Ng %d)", B, J, Np, Ng);
    ROMP_REQUIRE(max_gt >= 1 && max_gt <= RH_MAX_GT, "romp_rh_score: max_gt %d outside 1..%d", max_gt, RH_MAX_GT);
    ROMP_REQUIRE(Ng == 0 || (gt_kp2d && gt_depth_id && gt_age && pred_of_gt), "romp_rh_score: null ground truth with %d rows", Ng);
    ROMP_REQUIRE(Np == 0 || (pred_kp2d && pred_depth), "romp_rh_score: null predictions with %d rows", Np);
    const size_t lds = (sizeof(float) + 2 * sizeof(int32_t)) * (size_t)max_gt;
    hipLaunchKernelGGL(score_kernel, dim3(B), dim3(64), lds, (hipStream_t)stream, pred_kp2d, pred_depth, Np, gt_kp2d, gt_depth_id,
                       gt_age, pred_of_gt, Ng, gt_offsets, J, max_gt, dr_thresh, pck_thresh, pckh, correct_visible, counts);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_rh_accumulate(const int32_t* counts, int B, const float* pckh, int Ng, const int32_t* gt_of_pred, int Np, double* acc,
                       void* stream) {
    ROMP_REQUIRE(acc && B >= 0 && Ng >= 0 && Np >= 0 && (counts || B == 0) && (pckh || Ng == 0) && (gt_of_pred || Np == 0),
                 "romp_rh_accumulate: bad arguments (B %d, Ng %d, Np %d)", B, Ng, Np);
    hipLaunchKernelGGL(rh_accumulate_kernel, dim3(1), dim3(RH_ACC_THREADS), 0, (hipStream_t)stream, counts, B, pckh, Ng, gt_of_pred,
                       Np, acc);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

}  // extern "C"
