// fit_priors.hip -- SMPLify's pose priors and 3-D joint targets for the device fitter (include/romp_hip_fit_priors.h): each
// term with its gradient in one launch, beside the two launches of fit.hip.  Like those, both kernels move little (the eight
// 69 x 69 precisions are 152 KB and stay in the L2) and are bound by latency; what they buy is the launch count of a step.
//   fit_pose_prior_kernel  one workgroup of eight waves per person; in a round wave w takes component m = 8 round + w.
//                          Lane i owns the pose columns 3 + i and 67 + i (i < 5): P is symmetric, so it accumulates
//                          sum_k P[k][i] d_k, one contiguous row per k across the lanes, d_k broadcast from the LDS.  A wave
//                          keeps P d of its best component in registers; the waves' (q, m) meet in the LDS, every thread picks
//                          the same winner (lowest q, then lowest m), and the winning wave stores all 72 columns.
//   fit_joints3d_kernel    one wave per person, four to a workgroup, lane l owns joints l, l + 64, ... as fit_reproject_kernel;
//                          a first pass finds the alignment means, a second the residuals.
// Arithmetic is float64 on the float32 inputs, rounded once when stored; sums run in a fixed order (xor butterflies, serial
// loops), no atomics.
#include "common.h"
#include "../../include/romp_hip_fit_priors.h"
#include <math.h>

namespace romp {

constexpr int PRIOR_WAVES = 8;                                 // mixture components per round
constexpr int PRIOR_D = ROMP_FIT_MAX_POSE_DIM;
constexpr int J3D_WAVES = 4;                                   // persons per workgroup
constexpr int J3D_ITERS = ROMP_FIT_MAX_JOINTS / 64;            // joints per lane

// joint -> keypoint (-1: not picked) and whether the joint's keypoint is in the alignment set
struct j3d_pick { int16_t j2k[ROMP_FIT_MAX_JOINTS]; uint8_t aligned[ROMP_FIT_MAX_JOINTS]; };

__device__ __forceinline__ double wave_sum64(double x) {
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

// the angle prior's (column, sign) pairs: prior_loss.py:111 with the global orientation's three columns put back
__device__ __forceinline__ double angle_sign(int c) { return c == 55 ? 1.0 : (c == 58 || c == 12 || c == 15) ? -1.0 : 0.0; }

__device__ __forceinline__ void put(float* p, double g, int accumulate) { *p = (float)(accumulate ? (double)*p + g : g); }

__global__ __launch_bounds__(64 * PRIOR_WAVES) void fit_pose_prior_kernel(
        const float* __restrict__ poses, const float* __restrict__ means, const float* __restrict__ precisions,
        const float* __restrict__ offsets, int M, int D, float w_gmm, float w_angle, float* __restrict__ loss,
        int32_t* __restrict__ best, float* __restrict__ grad_poses, int accumulate, float* __restrict__ history) {
    __shared__ double s_d[PRIOR_WAVES][PRIOR_D + 3];           // d of the wave's component
    __shared__ double s_q[PRIOR_WAVES];
    __shared__ int s_m[PRIOR_WAVES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const size_t n = blockIdx.x;
    const float* x = poses + n * 72;
    const bool own0 = lane < D, own1 = lane + 64 < D;          // the lane's two columns of the D
    const double x0 = own0 ? (double)x[3 + lane] : 0.0, x1 = own1 ? (double)x[67 + lane] : 0.0;
    double best_q = 0, pd0 = 0, pd1 = 0;                        // the wave's best component: q and its share of P d
    int best_m = -1;
    const int rounds = (M + PRIOR_WAVES - 1) / PRIOR_WAVES;     // the same for every wave: the barriers below are uniform
    for (int r = 0; r < rounds; ++r) {
        const int m = r * PRIOR_WAVES + wave;
        const bool on = m < M;
        const float* mu = means + (size_t)(on ? m : 0) * D;
        const double d0 = on && own0 ? x0 - (double)mu[lane] : 0.0, d1 = on && own1 ? x1 - (double)mu[lane + 64] : 0.0;
        s_d[wave][lane] = d0;
        if (lane < PRIOR_D + 3 - 64) s_d[wave][lane + 64] = d1;
        __syncthreads();
        if (on) {
            const float* P = precisions + (size_t)m * D * D;
            double a0 = 0, a1 = 0;
#pragma unroll 4
            for (int k = 0; k < D; ++k) {
                const double dk = s_d[wave][k];
                const float* row = P + (size_t)k * D;
                if (own0) a0 += (double)row[lane] * dk;
                if (own1) a1 += (double)row[lane + 64] * dk;
            }
            const double q = 0.5 * wave_sum64(d0 * a0 + d1 * a1) + (double)offsets[m];
            if (best_m < 0 || q < best_q) { best_q = q; best_m = m; pd0 = a0; pd1 = a1; }   // m rises: the lowest m keeps a tie
        }
        __syncthreads();
    }
    if (lane == 0) { s_q[wave] = best_q; s_m[wave] = best_m; }
    __syncthreads();
    int win = 0, win_m = -1;                                    // mixture off: wave 0 writes
    double win_q = 0;
    for (int w = 0; w < PRIOR_WAVES; ++w) {
        const int m = s_m[w];
        if (m < 0) continue;
        const double q = s_q[w];
        if (win_m < 0 || q < win_q || (q == win_q && m < win_m)) { win = w; win_m = m; win_q = q; }
    }
    if (wave != win) return;
    const double wg = win_m >= 0 ? (double)w_gmm : 0.0, wa = (double)w_angle;
    float* g = grad_poses + n * 72;
    {   // column 3 + lane: the lane's first column of the D, which also holds the four angle columns (12, 15, 55, 58)
        const int c = 3 + lane;
        const double s = angle_sign(c);
        double v = own0 ? wg * pd0 : 0.0;
        if (s != 0.0) v += wa * 2.0 * s * exp(2.0 * s * (double)x[c]);
        put(g + c, v, accumulate);
    }
    if (lane < 5) put(g + 67 + lane, own1 ? wg * pd1 : 0.0, accumulate);
    if (lane < 3) put(g + lane, 0.0, accumulate);
    if (lane == 0) {
        const float lg = (float)(win_m >= 0 ? win_q : 0.0);
        const float la = (float)(exp(2.0 * (double)x[55]) + exp(-2.0 * (double)x[58]) + exp(-2.0 * (double)x[12]) + exp(-2.0 * (double)x[15]));
        loss[n * 2] = lg; loss[n * 2 + 1] = la;
        if (history) { history[n * 2] = lg; history[n * 2 + 1] = la; }
        if (best) best[n] = win_m;
    }
}

__global__ __launch_bounds__(64 * J3D_WAVES) void fit_joints3d_kernel(
        const float* __restrict__ joints, int N, int J, const float* __restrict__ trans, const float* __restrict__ targets,
        const float* __restrict__ conf, int K, j3d_pick pick, int n_align, float sigma, float weight, float* __restrict__ loss,
        float* __restrict__ grad_joints, float* __restrict__ grad_trans, int accumulate, float* __restrict__ history) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * J3D_WAVES + (threadIdx.x >> 6);
    if (n >= N) return;                                        // whole waves leave; no barrier below
    const double t0 = trans ? (double)trans[(size_t)n * 3] : 0.0, t1 = trans ? (double)trans[(size_t)n * 3 + 1] : 0.0,
                 t2 = trans ? (double)trans[(size_t)n * 3 + 2] : 0.0;
    const double s2 = sigma > 0.f ? (double)sigma * (double)sigma : 0.0;
    // pass 1: the lane's keypoints, their visibility, and the sums over the alignment set
    double px[J3D_ITERS], py[J3D_ITERS], pz[J3D_ITERS], w[J3D_ITERS];          // prediction - target; conf^2, 0: invisible
    double mx = 0, my = 0, mz = 0, hidden = 0;
#pragma unroll
    for (int it = 0; it < J3D_ITERS; ++it) {
        px[it] = py[it] = pz[it] = w[it] = 0;
        const int j = lane + 64 * it;
        if (j >= J) continue;
        const int k = pick.j2k[j];
        if (k < 0) continue;
        const size_t nk = (size_t)n * K + k;
        const float tx = targets[nk * 3], ty = targets[nk * 3 + 1], tz = targets[nk * 3 + 2];
        const float cf = conf ? conf[nk] : 1.f;
        const bool vis = cf > 0.f && tx != -2.f && tx == tx && ty == ty && tz == tz;
        if (!vis) { if (pick.aligned[j]) hidden += 1; continue; }
        const float* X = joints + ((size_t)n * J + j) * 3;
        px[it] = ((double)X[0] + t0) - (double)tx; py[it] = ((double)X[1] + t1) - (double)ty; pz[it] = ((double)X[2] + t2) - (double)tz;
        w[it] = (double)cf * (double)cf;
        if (pick.aligned[j]) { mx += px[it]; my += py[it]; mz += pz[it]; }
    }
    bool off = false;
    if (n_align > 0) {                                         // mean(prediction) - mean(target) over the alignment set
        off = wave_sum64(hidden) > 0;
        mx = wave_sum64(mx) / n_align; my = wave_sum64(my) / n_align; mz = wave_sum64(mz) / n_align;
    }
    // pass 2: residuals, the loss and the unnormalised gradients
    double a_loss = 0, a_cnt = 0, sx = 0, sy = 0, sz = 0;
#pragma unroll
    for (int it = 0; it < J3D_ITERS; ++it) {
        if (!(w[it] > 0) || off) { px[it] = py[it] = pz[it] = 0; continue; }
        const double rx = px[it] - mx, ry = py[it] - my, rz = pz[it] - mz, e = rx * rx + ry * ry + rz * rz;
        double rho = e, drho = 1;
        if (s2 > 0) { const double q = s2 / (s2 + e); rho = q * e; drho = q * q; }
        const double c = 2 * w[it] * drho;
        px[it] = c * rx; py[it] = c * ry; pz[it] = c * rz;
        a_loss += w[it] * rho; a_cnt += 1;
        sx += px[it]; sy += py[it]; sz += pz[it];
    }
    a_loss = wave_sum64(a_loss); a_cnt = wave_sum64(a_cnt); sx = wave_sum64(sx); sy = wave_sum64(sy); sz = wave_sum64(sz);
    const double inv = 1.0 / (a_cnt + 1e-4), gw = (double)weight * inv;
    const double ax = n_align > 0 ? sx / n_align : 0.0, ay = n_align > 0 ? sy / n_align : 0.0, az = n_align > 0 ? sz / n_align : 0.0;
#pragma unroll
    for (int it = 0; it < J3D_ITERS; ++it) {
        const int j = lane + 64 * it;
        if (j >= J) continue;
        const bool al = pick.aligned[j] && !off;
        float* g = grad_joints + ((size_t)n * J + j) * 3;
        put(g, (px[it] - (al ? ax : 0.0)) * gw, accumulate);
        put(g + 1, (py[it] - (al ? ay : 0.0)) * gw, accumulate);
        put(g + 2, (pz[it] - (al ? az : 0.0)) * gw, accumulate);
    }
    if (lane == 0) {
        const float l = (float)(a_loss * inv);
        loss[n] = l;
        if (history) history[n] = l;
        if (grad_trans) {
            const bool z = n_align > 0;
            put(grad_trans + (size_t)n * 3, z ? 0.0 : sx * gw, accumulate);
            put(grad_trans + (size_t)n * 3 + 1, z ? 0.0 : sy * gw, accumulate);
            put(grad_trans + (size_t)n * 3 + 2, z ? 0.0 : sz * gw, accumulate);
        }
    }
}

}  // namespace romp

using namespace romp;

extern "C" int romp_fit_pose_prior(const float* poses, int N, const float* means, const float* precisions, const float* offsets,
                                   int M, int D, float w_gmm, float w_angle, float* loss, int32_t* best, float* grad_poses,
                                   int accumulate, float* loss_history, int history_row, void* stream) {
    ROMP_REQUIRE(poses && loss && grad_poses, "romp_fit_pose_prior: null argument");
    ROMP_REQUIRE(N >= 0, "romp_fit_pose_prior: N %d", N);
    ROMP_REQUIRE(D >= 1 && D <= ROMP_FIT_MAX_POSE_DIM, "romp_fit_pose_prior: D %d (1..%d)", D, ROMP_FIT_MAX_POSE_DIM);
    ROMP_REQUIRE(M >= 0 && M <= ROMP_FIT_MAX_GAUSSIANS, "romp_fit_pose_prior: M %d (0..%d)", M, ROMP_FIT_MAX_GAUSSIANS);
    ROMP_REQUIRE(history_row >= 0, "romp_fit_pose_prior: history_row %d", history_row);
    if (!means) M = 0;                                         // the mixture is off
    ROMP_REQUIRE(M == 0 || (precisions && offsets), "romp_fit_pose_prior: means without precisions or offsets");
    if (N == 0) return ROMP_OK;
    float* hist = loss_history ? loss_history + (size_t)history_row * N * 2 : nullptr;
    hipLaunchKernelGGL(fit_pose_prior_kernel, dim3(N), dim3(64 * PRIOR_WAVES), 0, (hipStream_t)stream, poses, means, precisions,
                       offsets, M, D, w_gmm, w_angle, loss, best, grad_poses, accumulate, hist);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

extern "C" int romp_fit_joints3d(const float* joints, int N, int J, const float* trans, const float* targets, const float* conf,
                                 int K, const int32_t* joint_inds_host, const int32_t* align_inds_host, int n_align, float sigma,
                                 float weight, float* loss, float* grad_joints, float* grad_trans, int accumulate,
                                 float* loss_history, int history_row, void* stream) {
    ROMP_REQUIRE(joints && targets && loss && grad_joints, "romp_fit_joints3d: null argument");
    ROMP_REQUIRE(!trans == !grad_trans, "romp_fit_joints3d: trans and grad_trans go together (both or neither)");
    ROMP_REQUIRE(N >= 0 && K >= 1 && K <= J && J <= ROMP_FIT_MAX_JOINTS, "romp_fit_joints3d: N %d, K %d, J %d (N >= 0, 1 <= K <= J <= %d)",
                 N, K, J, ROMP_FIT_MAX_JOINTS);
    ROMP_REQUIRE(n_align >= 0 && n_align <= K, "romp_fit_joints3d: n_align %d (0..K = %d)", n_align, K);
    ROMP_REQUIRE(n_align == 0 || align_inds_host, "romp_fit_joints3d: n_align %d without align_inds", n_align);
    ROMP_REQUIRE(history_row >= 0, "romp_fit_joints3d: history_row %d", history_row);
    j3d_pick pick;
    int k2j[ROMP_FIT_MAX_JOINTS];
    for (int j = 0; j < ROMP_FIT_MAX_JOINTS; ++j) { pick.j2k[j] = -1; pick.aligned[j] = 0; }
    for (int k = 0; k < K; ++k) {
        const int j = joint_inds_host ? joint_inds_host[k] : k;
        ROMP_REQUIRE(j >= 0 && j < J, "romp_fit_joints3d: joint_inds[%d] = %d is outside 0..%d", k, j, J - 1);
        ROMP_REQUIRE(pick.j2k[j] < 0, "romp_fit_joints3d: joint %d is picked twice (keypoints %d and %d)", j, (int)pick.j2k[j], k);
        pick.j2k[j] = (int16_t)k;
        k2j[k] = j;
    }
    for (int a = 0; a < n_align; ++a) {
        const int k = align_inds_host[a];
        ROMP_REQUIRE(k >= 0 && k < K, "romp_fit_joints3d: align_inds[%d] = %d is outside 0..%d", a, k, K - 1);
        ROMP_REQUIRE(!pick.aligned[k2j[k]], "romp_fit_joints3d: keypoint %d is in align_inds twice", k);
        pick.aligned[k2j[k]] = 1;
    }
    if (N == 0) return ROMP_OK;
    float* hist = loss_history ? loss_history + (size_t)history_row * N : nullptr;
    hipLaunchKernelGGL(fit_joints3d_kernel, dim3((N + J3D_WAVES - 1) / J3D_WAVES), dim3(64 * J3D_WAVES), 0, (hipStream_t)stream,
                       joints, N, J, trans, targets, conf, K, pick, n_align, sigma, weight, loss, grad_joints, grad_trans, accumulate,
                       hist);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}
