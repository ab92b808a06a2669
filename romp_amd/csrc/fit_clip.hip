// fit_clip.hip -- temporal smoothness terms for the device fitter and the acceleration metric of a tracked clip
// (include/romp_hip_fit_clip.h).  A row is one person in one frame; two int32 tables name its neighbours in the track.  The data
// is a few KB per row and a launch is bound by latency, so all blocks of a call (up to four linear tensors and the rotations)
// share one launch.
//   fit_temporal_kernel  one wave per (row, block), four to a workgroup.  A linear block: lanes stride over the columns; the
//                        wave recomputes e of its neighbours' terms from the up to five rows it reads, so no wave waits for
//                        another.  The rotation block: the wave puts the 24 Rodrigues matrices of rows pv, n, nx into its own
//                        slice of the LDS, lanes stride over joints x 9 for the two e_r, and lanes 0..23 take one joint each
//                        through the layer's Rodrigues derivative (rodrigues64.h).
//   clip_accel_kernel    one wave per row, lanes over the joints.
// Arithmetic is float64 on the float32 inputs, rounded once when stored; sums run in a fixed order (a lane's columns in
// ascending order, then xor butterflies), no atomics.
#include "common.h"
#include "rodrigues64.h"
#include "../../include/romp_hip_fit_clip.h"
#include <math.h>

namespace romp {

constexpr int CLIP_WAVES = 4;                                  // (row, block) pairs per workgroup
constexpr int CLIP_NJ = 24, CLIP_RE = CLIP_NJ * 9;             // joints of a pose; elements of their matrices

struct clip_args {
    romp_clip_segment seg[ROMP_CLIP_MAX_SEGMENTS];
    int n_seg, blocks, N, L;                                   // blocks = n_seg + (poses ? 1 : 0)
    const int32_t *prev, *next;
    const float *term_w, *poses, *joint_w;                     // term_w (N) or NULL = ones
    float w_rot, sigma_rot;
    float* grad_poses;
    int accumulate_poses;
    float *loss, *history;
};

struct accel_pick { uint8_t on[ROMP_FIT_MAX_JOINTS]; };

// ---- the link rule: every table entry is range-checked before it is used as an index -----------------------------------
// the row linked to n from behind, or -1:  p = prev[n], 0 <= p < N, p != n, next[p] == n.  0 <= n < N is the caller's.
__device__ __forceinline__ int link_prev(const int32_t* __restrict__ prev, const int32_t* __restrict__ next, int N, int n) {
    const int p = prev[n];
    if (p < 0 || p >= N || p == n) return -1;                  // never an index
    return next[p] == n ? p : -1;
}
// the row n links to, or -1: the same rule read from the other end, for the link (n -> x)
__device__ __forceinline__ int link_next(const int32_t* __restrict__ prev, const int32_t* __restrict__ next, int N, int n) {
    const int x = next[n];
    if (x < 0 || x >= N || x == n) return -1;                  // never an index
    return prev[x] == n ? x : -1;
}

__device__ __forceinline__ double clip_sum64(double x) {
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

__device__ __forceinline__ void clip_put(float* p, double g, int accumulate) { *p = (float)(accumulate ? (double)*p + g : g); }

// rho(e) and rho'(e): e and 1, or Geman-McClure for s2 = sigma^2 > 0
__device__ __forceinline__ double clip_rho(double e, double s2, double* d) {
    if (!(s2 > 0)) { *d = 1.0; return e; }
    const double q = s2 / (s2 + e);
    *d = q * q;
    return q * e;
}

__device__ __forceinline__ double sq_sigma(float sigma) { return sigma > 0.f ? (double)sigma * (double)sigma : 0.0; }

// One linear block of row n.  pv, nx, ppv, nnx: the linked rows or -1 (the same for every lane of the wave).
__device__ __forceinline__ void clip_linear(const romp_clip_segment& s, int n, int pv, int nx, int ppv, int nnx, int lane,
                                            double tw_p, double tw_n, double tw_x, float* __restrict__ loss2,
                                            float* __restrict__ hist2) {
    const int C = s.cols;
    const float* xn = s.x + (size_t)n * C;
    const float* xp = s.x + (size_t)(pv >= 0 ? pv : n) * C;    // a missing row stands in as row n and is not used
    const float* xx = s.x + (size_t)(nx >= 0 ? nx : n) * C;
    const float* xpp = s.x + (size_t)(ppv >= 0 ? ppv : n) * C;
    const float* xnn = s.x + (size_t)(nnx >= 0 ? nnx : n) * C;
    const bool vel_n = pv >= 0, vel_x = nx >= 0, acc_p = ppv >= 0, acc_n = pv >= 0 && nx >= 0, acc_x = nnx >= 0;
    double ev_n = 0, ev_x = 0, ea_p = 0, ea_n = 0, ea_x = 0;
    for (int c = lane; c < C; c += 64) {
        const double w = s.col_w ? (double)s.col_w[c] : 1.0;
        const double a = (double)xn[c], p = (double)xp[c], x = (double)xx[c], pp = (double)xpp[c], nn = (double)xnn[c];
        if (vel_n) { const double v = a - p; ev_n += w * v * v; }
        if (vel_x) { const double v = x - a; ev_x += w * v * v; }
        if (acc_p) { const double t = pp - 2 * p + a; ea_p += w * t * t; }
        if (acc_n) { const double t = p - 2 * a + x; ea_n += w * t * t; }
        if (acc_x) { const double t = a - 2 * x + nn; ea_x += w * t * t; }
    }
    ev_n = clip_sum64(ev_n); ev_x = clip_sum64(ev_x); ea_p = clip_sum64(ea_p); ea_n = clip_sum64(ea_n); ea_x = clip_sum64(ea_x);
    const double sv = sq_sigma(s.sigma_vel), sa = sq_sigma(s.sigma_acc);
    double dv_n, dv_x, da_p, da_n, da_x;
    const double l_vel = clip_rho(ev_n, sv, &dv_n), l_acc = clip_rho(ea_n, sa, &da_n);
    clip_rho(ev_x, sv, &dv_x); clip_rho(ea_p, sa, &da_p); clip_rho(ea_x, sa, &da_x);
    dv_n *= tw_n; da_n *= tw_n; dv_x *= tw_x; da_x *= tw_x; da_p *= tw_p;   // a term carries the weight of its own row
    const double wv = (double)s.w_vel, wa = (double)s.w_acc;
    float* g = s.grad + (size_t)n * C;
    for (int c = lane; c < C; c += 64) {
        const double w = s.col_w ? (double)s.col_w[c] : 1.0;
        const double a = (double)xn[c], p = (double)xp[c], x = (double)xx[c], pp = (double)xpp[c], nn = (double)xnn[c];
        double gv = 0, ga = 0;
        if (vel_n) gv += dv_n * (a - p);
        if (vel_x) gv -= dv_x * (x - a);
        if (acc_p) ga += da_p * (pp - 2 * p + a);
        if (acc_n) ga -= 2 * da_n * (p - 2 * a + x);
        if (acc_x) ga += da_x * (a - 2 * x + nn);
        clip_put(g + c, 2 * w * (wv * gv + wa * ga), s.accumulate);
    }
    if (lane == 0) {
        const float lv = (float)(vel_n ? l_vel : 0.0), la = (float)(acc_n ? l_acc : 0.0);
        loss2[0] = lv; loss2[1] = la;
        if (hist2) { hist2[0] = lv; hist2[1] = la; }
    }
}

__global__ __launch_bounds__(64 * CLIP_WAVES) void fit_temporal_kernel(clip_args a) {
    __shared__ double s_R[CLIP_WAVES][3][CLIP_RE];             // the wave's matrices of rows n, pv, nx
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long w = (long long)blockIdx.x * CLIP_WAVES + wave;
    const bool live = w < (long long)a.N * a.blocks;           // a dead wave only meets the barrier
    const int n = live ? (int)(w / a.blocks) : 0, b = live ? (int)(w % a.blocks) : 0;
    int pv = -1, nx = -1;
    if (live) {
        pv = link_prev(a.prev, a.next, a.N, n);
        nx = link_next(a.prev, a.next, a.N, n);
    }
    const double tw_p = a.term_w && pv >= 0 ? (double)a.term_w[pv] : 1.0, tw_n = a.term_w && live ? (double)a.term_w[n] : 1.0,
                 tw_x = a.term_w && nx >= 0 ? (double)a.term_w[nx] : 1.0;
    float* loss = a.loss + (size_t)n * a.L;
    float* hist = a.history ? a.history + (size_t)n * a.L : nullptr;
    if (live && b < a.n_seg) {
        const int ppv = pv >= 0 ? link_prev(a.prev, a.next, a.N, pv) : -1, nnx = nx >= 0 ? link_next(a.prev, a.next, a.N, nx) : -1;
        clip_linear(a.seg[b], n, pv, nx, ppv, nnx, lane, tw_p, tw_n, tw_x, loss + 2 * b, hist ? hist + 2 * b : nullptr);
    }
    const bool rot = live && b == a.n_seg;                     // only with poses: blocks = n_seg + 1
    if (rot) {                                                 // 72 (row, joint) matrices over the lanes, two rounds
        for (int item = lane; item < 3 * CLIP_NJ; item += 64) {
            const int r = item / CLIP_NJ, j = item % CLIP_NJ, row = r == 0 ? n : r == 1 ? pv : nx;
            if (row < 0) continue;
            double R[9];
            Rodrigues64 st;
            rodrigues64(a.poses + (size_t)row * 72 + j * 3, R, st);
            for (int e = 0; e < 9; ++e) s_R[wave][r][j * 9 + e] = R[e];
        }
    }
    __syncthreads();                                           // uniform: every wave of the workgroup gets here
    if (!rot) return;
    double e_n = 0, e_x = 0;
    for (int i = lane; i < CLIP_RE; i += 64) {
        const double wj = a.joint_w ? (double)a.joint_w[i / 9] : 1.0;
        if (pv >= 0) { const double d = s_R[wave][0][i] - s_R[wave][1][i]; e_n += wj * d * d; }
        if (nx >= 0) { const double d = s_R[wave][2][i] - s_R[wave][0][i]; e_x += wj * d * d; }
    }
    e_n = clip_sum64(e_n); e_x = clip_sum64(e_x);
    const double s2 = sq_sigma(a.sigma_rot);
    double d_n, d_x;
    const double l_rot = clip_rho(e_n, s2, &d_n);
    clip_rho(e_x, s2, &d_x);
    d_n *= tw_n; d_x *= tw_x;
    if (lane < CLIP_NJ) {
        const int j = lane;
        const double c = 2 * (double)a.w_rot * (a.joint_w ? (double)a.joint_w[j] : 1.0);
        double R[9], gR[9], g[3];
        Rodrigues64 st;
        rodrigues64(a.poses + (size_t)n * 72 + j * 3, R, st);
        for (int e = 0; e < 9; ++e) {
            double t = 0;
            if (pv >= 0) t += d_n * (s_R[wave][0][j * 9 + e] - s_R[wave][1][j * 9 + e]);
            if (nx >= 0) t -= d_x * (s_R[wave][2][j * 9 + e] - s_R[wave][0][j * 9 + e]);
            gR[e] = c * t;
        }
        rodrigues64_backward(st, gR, g);
        float* out = a.grad_poses + (size_t)n * 72 + j * 3;
        for (int k = 0; k < 3; ++k) clip_put(out + k, g[k], a.accumulate_poses);
    }
    if (lane == 0) {
        const float l = (float)(pv >= 0 ? l_rot : 0.0);
        loss[2 * a.n_seg] = l;
        if (hist) hist[2 * a.n_seg] = l;
    }
}

__global__ __launch_bounds__(64 * CLIP_WAVES) void clip_accel_kernel(
        const float* __restrict__ joints, int N, int J, const float* __restrict__ gt, const uint8_t* __restrict__ vis, int K,
        accel_pick pick, const int32_t* __restrict__ prev, const int32_t* __restrict__ next, float* __restrict__ value,
        uint8_t* __restrict__ valid) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * CLIP_WAVES + (threadIdx.x >> 6);
    if (n >= N) return;                                        // whole waves leave; no barrier below
    const int pv = link_prev(prev, next, N, n), nx = link_next(prev, next, N, n);
    bool ok = pv >= 0 && nx >= 0;
    if (ok && vis) ok = vis[pv] && vis[n] && vis[nx];
    double sum = 0;
    if (ok) {
        for (int j = lane; j < J; j += 64) {
            if (!pick.on[j]) continue;
            const size_t ip = ((size_t)pv * J + j) * 3, in = ((size_t)n * J + j) * 3, ix = ((size_t)nx * J + j) * 3;
            double d[3];
            for (int k = 0; k < 3; ++k) {
                d[k] = (double)joints[ip + k] - 2 * (double)joints[in + k] + (double)joints[ix + k];
                if (gt) d[k] -= (double)gt[ip + k] - 2 * (double)gt[in + k] + (double)gt[ix + k];
            }
            sum += sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
        }
    }
    sum = clip_sum64(sum);
    if (lane == 0) {
        value[n] = ok ? (float)(sum / K) : 0.f;
        valid[n] = ok ? 1 : 0;
    }
}

}  // namespace romp

using namespace romp;

extern "C" int romp_fit_temporal(const romp_clip_segment* segments_host, int n_segments, const int32_t* prev, const int32_t* next,
                                 int N, const float* term_w, const float* poses, const float* joint_w, float w_rot, float sigma_rot, float* grad_poses,
                                 int accumulate_poses, float* loss, float* loss_history, int history_row, void* stream) {
    ROMP_REQUIRE(prev && next && loss, "romp_fit_temporal: null prev, next or loss");
    ROMP_REQUIRE(n_segments >= 0 && n_segments <= ROMP_CLIP_MAX_SEGMENTS, "romp_fit_temporal: n_segments %d (0..%d)", n_segments,
                 ROMP_CLIP_MAX_SEGMENTS);
    ROMP_REQUIRE(n_segments == 0 || segments_host, "romp_fit_temporal: null segment table");
    ROMP_REQUIRE(n_segments > 0 || poses, "romp_fit_temporal: neither a segment nor the rotation block");
    ROMP_REQUIRE(N >= 0, "romp_fit_temporal: N %d", N);
    ROMP_REQUIRE(history_row >= 0, "romp_fit_temporal: history_row %d", history_row);
    ROMP_REQUIRE(!poses || grad_poses, "romp_fit_temporal: poses without grad_poses");
    ROMP_REQUIRE(!poses || w_rot >= 0.f, "romp_fit_temporal: w_rot %g is negative", (double)w_rot);
    clip_args a = {};
    for (int i = 0; i < n_segments; ++i) {
        const romp_clip_segment& s = segments_host[i];
        ROMP_REQUIRE(s.x && s.grad, "romp_fit_temporal: segment %d without x or grad", i);
        ROMP_REQUIRE(s.cols >= 1, "romp_fit_temporal: segment %d has cols %d", i, (int)s.cols);
        ROMP_REQUIRE(s.w_vel >= 0.f && s.w_acc >= 0.f, "romp_fit_temporal: segment %d has a negative weight (%g, %g)", i,
                     (double)s.w_vel, (double)s.w_acc);
        a.seg[i] = s;
    }
    a.n_seg = n_segments; a.blocks = n_segments + (poses ? 1 : 0); a.N = N; a.L = 2 * n_segments + (poses ? 1 : 0);
    const long long groups = ((long long)N * a.blocks + CLIP_WAVES - 1) / CLIP_WAVES;
    ROMP_REQUIRE(groups <= 0x7fffffffLL, "romp_fit_temporal: N %d times %d blocks is beyond one launch", N, a.blocks);
    if (N == 0) return ROMP_OK;
    a.prev = prev; a.next = next; a.term_w = term_w; a.poses = poses; a.joint_w = joint_w; a.w_rot = w_rot; a.sigma_rot = sigma_rot;
    a.grad_poses = grad_poses; a.accumulate_poses = accumulate_poses; a.loss = loss;
    a.history = loss_history ? loss_history + (size_t)history_row * N * a.L : nullptr;
    hipLaunchKernelGGL(fit_temporal_kernel, dim3((unsigned)groups), dim3(64 * CLIP_WAVES), 0, (hipStream_t)stream, a);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

extern "C" int romp_clip_accel(const float* joints, int N, int J, const float* gt, const uint8_t* vis, int K,
                               const int32_t* joint_inds_host, const int32_t* prev, const int32_t* next, float* value,
                               uint8_t* valid, void* stream) {
    ROMP_REQUIRE(joints && prev && next && value && valid, "romp_clip_accel: null argument");
    ROMP_REQUIRE(N >= 0 && K >= 1 && K <= J && J <= ROMP_FIT_MAX_JOINTS, "romp_clip_accel: N %d, K %d, J %d (N >= 0, 1 <= K <= J <= %d)",
                 N, K, J, ROMP_FIT_MAX_JOINTS);
    accel_pick pick;
    for (int j = 0; j < ROMP_FIT_MAX_JOINTS; ++j) pick.on[j] = 0;
    for (int k = 0; k < K; ++k) {
        const int j = joint_inds_host ? joint_inds_host[k] : k;
        ROMP_REQUIRE(j >= 0 && j < J, "romp_clip_accel: joint_inds[%d] = %d is outside 0..%d", k, j, J - 1);
        ROMP_REQUIRE(!pick.on[j], "romp_clip_accel: joint %d is picked twice", j);
        pick.on[j] = 1;
    }
    if (N == 0) return ROMP_OK;
    hipLaunchKernelGGL(clip_accel_kernel, dim3(((unsigned)N + CLIP_WAVES - 1) / CLIP_WAVES), dim3(64 * CLIP_WAVES), 0, (hipStream_t)stream, joints,
                       N, J, gt, vis, K, pick, prev, next, value, valid);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}
