// fit.hip -- fitting the SMPL layer to 2-D keypoints (include/romp_hip_fit.h): the reprojection loss with its gradients in
// one launch, and one Adam step for all parameter tensors of a fit in one launch.  Both kernels move a few kilobytes and are
// bound by latency; what they buy is the launch count of a fitting step (the layer's own launches plus these two).
//   fit_reproject_kernel  one wave per person, four waves to a workgroup; lane l owns joints l, l + 64, ... (J <= 256, so at
//                         most four, kept in registers until the visible count is known); the loss, the three camera sums
//                         and the count are reduced with a xor butterfly, the same order on every run.
//   fit_adam_kernel       one thread per element of up to eight (rows, cols) tensors; the segment table is a launch argument.
// Arithmetic is float64 on the float32 inputs (a residual is a difference of nearly equal numbers; at these sizes the cost
// is nothing), rounded once when stored.
#include "common.h"
#include "../../include/romp_hip_fit.h"
#include <math.h>

namespace romp {

constexpr int FIT_WAVES = 4;                                   // persons per workgroup
constexpr int FIT_ITERS = ROMP_FIT_MAX_JOINTS / 64;            // joints per lane

struct fit_pick { int16_t j2k[ROMP_FIT_MAX_JOINTS]; };         // joint -> keypoint, -1: not picked
struct fit_table { romp_fit_segment seg[ROMP_FIT_MAX_SEGMENTS]; int32_t first[ROMP_FIT_MAX_SEGMENTS + 1]; };

__device__ __forceinline__ double wave_sum(double x) {
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

__global__ __launch_bounds__(64 * FIT_WAVES) void fit_reproject_kernel(
        const float* __restrict__ joints, int N, int J, const float* __restrict__ cam, const float* __restrict__ targets,
        const float* __restrict__ conf, int K, fit_pick pick, int mode, float focal, float half, float sigma,
        float* __restrict__ loss, float* __restrict__ grad_joints, float* __restrict__ grad_cam, float* __restrict__ history) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * FIT_WAVES + (threadIdx.x >> 6);
    if (n >= N) return;                                        // whole waves leave; no barrier below
    const double c0 = cam[(size_t)n * 3], c1 = cam[(size_t)n * 3 + 1], c2 = cam[(size_t)n * 3 + 2];
    const double fh_f = (double)focal, fh_h = (double)half;
    const double s2 = sigma > 0.f ? (double)sigma * (double)sigma : 0.0;
    // per joint of this lane: the unnormalised gradient of the joint; camera sums and loss per lane
    double gx[FIT_ITERS], gy[FIT_ITERS], gz[FIT_ITERS];
    double a_loss = 0, a0 = 0, a1 = 0, a2 = 0, a_cnt = 0;
#pragma unroll
    for (int it = 0; it < FIT_ITERS; ++it) {
        gx[it] = gy[it] = gz[it] = 0;
        const int j = lane + 64 * it;
        if (j >= J) continue;
        const int k = pick.j2k[j];
        if (k < 0) continue;
        const size_t nk = (size_t)n * K + k;
        const float tu = targets[nk * 2], tv = targets[nk * 2 + 1];
        const float cf = conf ? conf[nk] : 1.f;
        if (!(cf > 0.f) || !(tu > -1.99f) || !(tv > -1.99f)) continue;
        const float* X = joints + ((size_t)n * J + j) * 3;
        const double x = X[0], y = X[1], z = X[2];
        double u, v, zz = 1, px = 0, py = 0;
        if (mode == 0) {
            u = c0 * x + c1; v = c0 * y + c2;
        } else {
            px = x + c0; py = y + c1; zz = z + c2 + 1e-6;
            u = px / zz * fh_f / fh_h; v = py / zz * fh_f / fh_h;
        }
        const double ru = u - (double)tu, rv = v - (double)tv, e = ru * ru + rv * rv, w = (double)cf * (double)cf;
        double rho = e, drho = 1;
        if (s2 > 0) { const double q = s2 / (s2 + e); rho = q * e; drho = q * q; }
        const double gu = 2 * w * drho * ru, gv = 2 * w * drho * rv;   // d term / d (u, v)
        a_loss += w * rho; a_cnt += 1;
        if (mode == 0) {
            gx[it] = gu * c0; gy[it] = gv * c0;
            a0 += gu * x + gv * y; a1 += gu; a2 += gv;
        } else {
            const double f = fh_f / fh_h / zz;
            gx[it] = gu * f; gy[it] = gv * f; gz[it] = -(gu * u + gv * v) / zz;
            a0 += gx[it]; a1 += gy[it]; a2 += gz[it];
        }
    }
    a_loss = wave_sum(a_loss); a0 = wave_sum(a0); a1 = wave_sum(a1); a2 = wave_sum(a2); a_cnt = wave_sum(a_cnt);
    const double inv = 1.0 / (a_cnt + 1e-4);
#pragma unroll
    for (int it = 0; it < FIT_ITERS; ++it) {
        const int j = lane + 64 * it;
        if (j >= J) continue;
        float* g = grad_joints + ((size_t)n * J + j) * 3;
        g[0] = (float)(gx[it] * inv); g[1] = (float)(gy[it] * inv); g[2] = (float)(gz[it] * inv);
    }
    if (lane == 0) {
        const float l = (float)(a_loss * inv);
        loss[n] = l;
        if (history) history[n] = l;
        grad_cam[(size_t)n * 3] = (float)(a0 * inv); grad_cam[(size_t)n * 3 + 1] = (float)(a1 * inv);
        grad_cam[(size_t)n * 3 + 2] = (float)(a2 * inv);
    }
}

__global__ __launch_bounds__(256) void fit_adam_kernel(fit_table t, int n_seg, int total, double lr_c, double beta1, double beta2,
                                                       double inv_sqrt_c2, double eps) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    int s = 0;
    while (s + 1 < n_seg && i >= t.first[s + 1]) ++s;
    const romp_fit_segment& sg = t.seg[s];
    const int e = i - t.first[s], c = e % sg.cols;
    const double p = sg.param[e];
    double g = sg.grad[e];
    if (sg.prior_w) g += 2.0 * (double)sg.prior_w[c] * (p - (sg.prior_ref ? (double)sg.prior_ref[e] : 0.0));
    const float m = (float)(beta1 * (double)sg.m[e] + (1.0 - beta1) * g);
    const float v = (float)(beta2 * (double)sg.v[e] + (1.0 - beta2) * g * g);
    sg.m[e] = m; sg.v[e] = v;
    sg.param[e] = (float)(p - lr_c * (double)m / (sqrt((double)v) * inv_sqrt_c2 + eps));
}

}  // namespace romp

using namespace romp;

extern "C" int romp_fit_reproject(const float* joints, int N, int J, const float* cam, const float* targets, const float* conf,
                                  int K, const int32_t* joint_inds_host, int mode, float focal, float half, float sigma,
                                  float* loss, float* grad_joints, float* grad_cam, float* loss_history, int history_row,
                                  void* stream) {
    ROMP_REQUIRE(joints && cam && targets && loss && grad_joints && grad_cam, "romp_fit_reproject: null argument");
    ROMP_REQUIRE(N >= 0 && K >= 1 && K <= J && J <= ROMP_FIT_MAX_JOINTS, "romp_fit_reproject: N %d, K %d, J %d (N >= 0, 1 <= K <= J <= %d)",
                 N, K, J, ROMP_FIT_MAX_JOINTS);
    ROMP_REQUIRE(mode == 0 || mode == 1, "romp_fit_reproject: mode %d (0 = weak perspective, 1 = perspective)", mode);
    ROMP_REQUIRE(history_row >= 0, "romp_fit_reproject: history_row %d", history_row);
    fit_pick pick;
    for (int j = 0; j < ROMP_FIT_MAX_JOINTS; ++j) pick.j2k[j] = -1;
    for (int k = 0; k < K; ++k) {
        const int j = joint_inds_host ? joint_inds_host[k] : k;
        ROMP_REQUIRE(j >= 0 && j < J, "romp_fit_reproject: joint_inds[%d] = %d is outside 0..%d", k, j, J - 1);
        ROMP_REQUIRE(pick.j2k[j] < 0, "romp_fit_reproject: joint %d is picked twice (keypoints %d and %d)", j, (int)pick.j2k[j], k);
        pick.j2k[j] = (int16_t)k;
    }
    if (N == 0) return ROMP_OK;
    float* hist = loss_history ? loss_history + (size_t)history_row * N : nullptr;
    hipLaunchKernelGGL(fit_reproject_kernel, dim3((N + FIT_WAVES - 1) / FIT_WAVES), dim3(64 * FIT_WAVES), 0, (hipStream_t)stream,
                       joints, N, J, cam, targets, conf, K, pick, mode, focal, half, sigma, loss, grad_joints, grad_cam, hist);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

extern "C" int romp_fit_adam(const romp_fit_segment* segments_host, int n_segments, float lr, float beta1, float beta2, float eps,
                             int step, void* stream) {
    ROMP_REQUIRE(segments_host && n_segments >= 1 && n_segments <= ROMP_FIT_MAX_SEGMENTS,
                 "romp_fit_adam: %d segments (1..%d) or a null table", n_segments, ROMP_FIT_MAX_SEGMENTS);
    ROMP_REQUIRE(step >= 1, "romp_fit_adam: step %d (counts from 1)", step);
    fit_table t;
    long long total = 0;
    for (int s = 0; s < n_segments; ++s) {
        const romp_fit_segment& sg = segments_host[s];
        ROMP_REQUIRE(sg.param && sg.grad && sg.m && sg.v, "romp_fit_adam: segment %d has a null param / grad / m / v", s);
        ROMP_REQUIRE(sg.rows >= 0 && sg.cols >= 1, "romp_fit_adam: segment %d is %d x %d", s, sg.rows, sg.cols);
        t.seg[s] = sg;
        t.first[s] = (int32_t)total;
        total += (long long)sg.rows * sg.cols;
        ROMP_REQUIRE(total < (1ll << 31), "romp_fit_adam: more than 2^31 elements");
    }
    for (int s = n_segments; s <= ROMP_FIT_MAX_SEGMENTS; ++s) t.first[s] = (int32_t)total;
    for (int s = n_segments; s < ROMP_FIT_MAX_SEGMENTS; ++s) t.seg[s] = romp_fit_segment{nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, 1};
    if (total == 0) return ROMP_OK;
    const double c1 = 1.0 - pow((double)beta1, step), c2 = 1.0 - pow((double)beta2, step);
    hipLaunchKernelGGL(fit_adam_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, t, n_segments,
                       (int)total, (double)lr / c1, (double)beta1, (double)beta2, 1.0 / sqrt(c2), (double)eps);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}
