// fit_scene.hip -- scene terms for the device fitter: depth order and inter-person collision (include/romp_hip_fit_scene.h).
// A row is one person in one image; two int32 tables group the rows by image.  The data is a few KB per row and a launch is
// bound by latency, so both terms share one launch.
//   fit_scene_kernel  one workgroup of 256 threads per row.  The row finds its scene by a scan of the tables (every entry
//                     range-checked before use).  Depth: the threads stride over the scene's pair space for the number of
//                     active pairs A, then over the row's partners for its own sum.  Collision: lane s of every wave owns
//                     sphere s of the row; wave w takes partners w, w + 4, ... and puts the partner's spheres into its own
//                     slice of the LDS; the four waves' sums are combined in wave order; thread j gathers joint j's spheres.
// Every row recomputes its own side of a pair, so the row's workgroup is the one owner of loss[n], grad_joints[n] and
// grad_cam[n].  Arithmetic is float64 on the float32 inputs, rounded once when stored; sums run in a fixed order (a thread's
// items in ascending order, xor butterflies, then the waves in order), no atomics.
#include "common.h"
#include "../../include/romp_hip_fit_scene.h"
#include <cmath>
#include <math.h>

namespace romp {

constexpr int SCENE_THREADS = 256, SCENE_WAVES = SCENE_THREADS / 64;
constexpr int SCENE_NONE = 0x7fffffff;

struct scene_args {
    romp_scene_sphere sph[ROMP_SCENE_MAX_SPHERES];
    const float *joints, *cam, *radius_scale, *term_w;
    const int32_t *offsets, *members, *depth_ids;
    float *grad_joints, *grad_cam, *loss, *history;
    int N, J, S, mode, kind, accumulate_joints, accumulate_cam;
    float w_depth, w_col, thresh;
};

__device__ __forceinline__ double scene_sum64(double x) {
    for (int d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
    return x;
}

// the sum of x over the workgroup, the same value in every thread: butterflies, then the waves in order.  Uniform calls only.
__device__ __forceinline__ double scene_block_sum(double x, double* s_red) {
    x = scene_sum64(x);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = x;
    __syncthreads();
    double r = 0;
    for (int w = 0; w < SCENE_WAVES; ++w) r += s_red[w];
    __syncthreads();
    return r;
}

__device__ __forceinline__ int scene_block_min(int x, int* s_min) {
    for (int d = 32; d > 0; d >>= 1) x = min(x, __shfl_xor(x, d));
    if ((threadIdx.x & 63) == 0) s_min[threadIdx.x >> 6] = x;
    __syncthreads();
    int r = s_min[0];
    for (int w = 1; w < SCENE_WAVES; ++w) r = min(r, s_min[w]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ void scene_put(float* p, double g, int accumulate) { *p = (float)(accumulate ? (double)*p + g : g); }

// ---- the table rule: every entry is range-checked before it is used as an index ----------------------------------------
// group g as the half-open range of positions [lo, hi), or false:  0 <= offsets[g] <= offsets[g + 1] <= N.  0 <= g < N is the
// caller's, so offsets[g + 1] lies inside the (N + 1) table.
__device__ __forceinline__ bool scene_group(const int32_t* __restrict__ offsets, int N, int g, int* lo, int* hi) {
    const int a = offsets[g], b = offsets[g + 1];
    if (a < 0 || a > b || b > N) return false;                 // never a range
    *lo = a; *hi = b;
    return true;
}
// the row at position k of the members, or -1:  0 <= member < N.  0 <= k < N is the caller's.
__device__ __forceinline__ int scene_member(const int32_t* __restrict__ members, int N, int k) {
    const int m = members[k];
    return m < 0 || m >= N ? -1 : m;                           // never an index
}

// z of a row's translation and the translation itself
__device__ __forceinline__ double scene_depth(const float* __restrict__ cam, int mode, int m) {
    return mode == 1 ? (double)cam[(size_t)m * 3 + 2] : 2.0 / (double)cam[(size_t)m * 3];
}
__device__ __forceinline__ void scene_trans(const float* __restrict__ cam, int mode, int m, double t[3]) {
    const double c0 = (double)cam[(size_t)m * 3], c1 = (double)cam[(size_t)m * 3 + 1], c2 = (double)cam[(size_t)m * 3 + 2];
    if (mode == 1) { t[0] = c0; t[1] = c1; t[2] = c2; }
    else { t[0] = 2.0 * c1 / c0; t[1] = 2.0 * c2 / c0; t[2] = 2.0 / c0; }
}

__device__ __forceinline__ double scene_softplus(double x) { return fmax(x, 0.0) + log1p(exp(-fabs(x))); }
__device__ __forceinline__ double scene_sigmoid(double x) {
    if (x >= 0) return 1.0 / (1.0 + exp(-x));
    const double e = exp(x);
    return e / (1.0 + e);
}

// The pair (first, second) in member order: d = z2 - z1, k = id2 - id1.  -> active; *f the pair's term, *df its derivative in d.
__device__ __forceinline__ bool scene_pair(double z1, double z2, int id1, int id2, double thresh, int kind, double* f, double* df) {
    const double d = z2 - z1;
    const long long k = (long long)id2 - (long long)id1;
    if (k == 0) { *f = d * d; *df = 2 * d; return true; }
    const double margin = d - (double)k * thresh;
    if (k < 0) {
        if (kind == ROMP_SCENE_PIECEWISE && !(margin > 0)) return false;
        *f = scene_softplus(d); *df = scene_sigmoid(d);
        return true;
    }
    if (kind == ROMP_SCENE_PIECEWISE && !(margin < 0)) return false;
    *f = scene_softplus(-d); *df = -scene_sigmoid(-d);
    return true;
}

__global__ __launch_bounds__(SCENE_THREADS) void fit_scene_kernel(scene_args a) {
    __shared__ double s_red[SCENE_WAVES];
    __shared__ int s_min[SCENE_WAVES];
    __shared__ double s_part[SCENE_WAVES][ROMP_SCENE_MAX_SPHERES][4];   // a wave's partner: centre and sigma^2 per sphere
    __shared__ double s_acc[SCENE_WAVES][ROMP_SCENE_MAX_SPHERES][4];    // a wave's sums per own sphere: energy, gradient
    __shared__ double s_g[ROMP_SCENE_MAX_SPHERES][3];                   // the gradient of the row's sphere centres
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = blockIdx.x, N = a.N;

    // ---- the scene of row n: the first position that names it, then the first valid group that holds the position
    int pos = SCENE_NONE;
    for (int k = tid; k < N; k += SCENE_THREADS)
        if (a.members[k] == n) { pos = k; break; }             // a thread's positions ascend: its first is its smallest
    pos = scene_block_min(pos, s_min);
    int grp = SCENE_NONE;
    if (pos != SCENE_NONE)
        for (int g = tid; g < N; g += SCENE_THREADS) {
            int lo, hi;
            if (scene_group(a.offsets, N, g, &lo, &hi) && lo <= pos && pos < hi) { grp = g; break; }
        }
    grp = scene_block_min(grp, s_min);
    int lo = 0, hi = 0;                                        // no scene: an empty range, no partner
    if (grp != SCENE_NONE) scene_group(a.offsets, N, grp, &lo, &hi);
    const int P = hi - lo;
    const double tw_n = a.term_w ? (double)a.term_w[n] : 1.0;

    // ---- depth order
    double l_depth = 0, g_z = 0;                               // loss[n,0]; the gradient of the objective in z_n
    if (a.depth_ids && a.depth_ids[n] >= 0 && P > 1) {
        const double thresh = (double)a.thresh;
        double count = 0;                                      // exact: whole numbers below 2^53
        const long long pairs = (long long)P * P;
        for (long long idx = tid; idx < pairs; idx += SCENE_THREADS) {
            const int i = (int)(idx / P), j = (int)(idx % P);
            if (i >= j) continue;
            const int mi = scene_member(a.members, N, lo + i), mj = scene_member(a.members, N, lo + j);
            if (mi < 0 || mj < 0) continue;
            const int idi = a.depth_ids[mi], idj = a.depth_ids[mj];
            if (idi < 0 || idj < 0) continue;
            double f, df;
            if (scene_pair(scene_depth(a.cam, a.mode, mi), scene_depth(a.cam, a.mode, mj), idi, idj, thresh, a.kind, &f, &df)) count += 1.0;
        }
        count = scene_block_sum(count, s_red);
        const int id_n = a.depth_ids[n];
        const double z_n = scene_depth(a.cam, a.mode, n);
        double sum = 0, gsum = 0;
        for (int k = lo + tid; k < hi; k += SCENE_THREADS) {
            const int m = scene_member(a.members, N, k);
            if (m < 0 || m == n) continue;
            const int id_m = a.depth_ids[m];
            if (id_m < 0) continue;
            const double z_m = scene_depth(a.cam, a.mode, m);
            const bool first = pos < k;                        // n is the pair's first row: d = z_m - z_n
            double f, df;
            if (!(first ? scene_pair(z_n, z_m, id_n, id_m, thresh, a.kind, &f, &df) : scene_pair(z_m, z_n, id_m, id_n, thresh, a.kind, &f, &df)))
                continue;
            const double tw_m = a.term_w ? (double)a.term_w[m] : 1.0;
            sum += f;
            gsum += (tw_n + tw_m) * (first ? -df : df);
        }
        sum = scene_block_sum(sum, s_red);
        gsum = scene_block_sum(gsum, s_red);
        if (count > 0) {
            l_depth = sum / (2 * count);
            g_z = (double)a.w_depth * gsum / (2 * count);
        }
    }

    // ---- collision
    double l_col = 0, g_t[3] = {0, 0, 0};                      // loss[n,1]; the gradient in t_n (thread 0 holds it)
    if (a.S > 0) {
        const int S = a.S, J = a.J;
        const bool own = lane < S;
        double c[3] = {0, 0, 0}, s2 = 0;                       // lane s: the centre and sigma^2 of sphere s of row n
        if (own) {
            const romp_scene_sphere sp = a.sph[lane];
            const float *jp = a.joints + ((size_t)n * J + sp.p) * 3, *jq = a.joints + ((size_t)n * J + sp.q) * 3;
            double t[3];
            scene_trans(a.cam, a.mode, n, t);
            const double al = (double)sp.a, sg = (double)sp.r / 3.0 * (a.radius_scale ? (double)a.radius_scale[n] : 1.0);
            for (int x = 0; x < 3; ++x) c[x] = (1.0 - al) * (double)jp[x] + al * (double)jq[x] + t[x];
            s2 = sg * sg;
        }
        double e_sum = 0, g[3] = {0, 0, 0};
        for (int k0 = lo; k0 < hi; k0 += SCENE_WAVES) {        // uniform: every wave of the workgroup meets both barriers
            const int k = k0 + wave;
            const int m = k < hi ? scene_member(a.members, N, k) : -1;
            const bool pair = m >= 0 && m != n;
            if (pair && own) {                                 // lane u: sphere u of the partner
                const romp_scene_sphere sp = a.sph[lane];
                const float *jp = a.joints + ((size_t)m * J + sp.p) * 3, *jq = a.joints + ((size_t)m * J + sp.q) * 3;
                double t[3];
                scene_trans(a.cam, a.mode, m, t);
                const double al = (double)sp.a, sg = (double)sp.r / 3.0 * (a.radius_scale ? (double)a.radius_scale[m] : 1.0);
                for (int x = 0; x < 3; ++x) s_part[wave][lane][x] = (1.0 - al) * (double)jp[x] + al * (double)jq[x] + t[x];
                s_part[wave][lane][3] = sg * sg;
            }
            __syncthreads();
            if (pair && own) {
                const double tw = 0.5 * (tw_n + (a.term_w ? (double)a.term_w[m] : 1.0));
                for (int u = 0; u < S; ++u) {
                    const double dx = c[0] - s_part[wave][u][0], dy = c[1] - s_part[wave][u][1], dz = c[2] - s_part[wave][u][2];
                    const double den = s2 + s_part[wave][u][3];
                    const double e = exp(-(dx * dx + dy * dy + dz * dz) / den);
                    const double q = -2.0 * tw * e / den;
                    e_sum += e;
                    g[0] += q * dx; g[1] += q * dy; g[2] += q * dz;
                }
            }
            __syncthreads();
        }
        if (own) {
            s_acc[wave][lane][0] = e_sum;
            for (int x = 0; x < 3; ++x) s_acc[wave][lane][1 + x] = g[x];
        }
        __syncthreads();
        double e_row = 0;
        if (wave == 0 && own) {
            double gs[3] = {0, 0, 0};
            for (int w = 0; w < SCENE_WAVES; ++w) {
                e_row += s_acc[w][lane][0];
                for (int x = 0; x < 3; ++x) gs[x] += s_acc[w][lane][1 + x];
            }
            for (int x = 0; x < 3; ++x) s_g[lane][x] = (double)a.w_col * gs[x];
        }
        if (wave == 0) l_col = 0.5 * scene_sum64(e_row);       // whole wave: the lanes without a sphere add 0
        __syncthreads();
        if (tid < J) {                                         // joint tid gathers its spheres in table order
            double gj[3] = {0, 0, 0};
            for (int s = 0; s < S; ++s) {
                const romp_scene_sphere sp = a.sph[s];
                const double al = (double)sp.a;
                if (sp.p == tid) for (int x = 0; x < 3; ++x) gj[x] += (1.0 - al) * s_g[s][x];
                if (sp.q == tid) for (int x = 0; x < 3; ++x) gj[x] += al * s_g[s][x];
            }
            float* out = a.grad_joints + ((size_t)n * J + tid) * 3;
            for (int x = 0; x < 3; ++x) scene_put(out + x, gj[x], a.accumulate_joints);
        }
        if (tid == 0)
            for (int s = 0; s < S; ++s)
                for (int x = 0; x < 3; ++x) g_t[x] += s_g[s][x];
    }

    if (tid == 0) {
        g_t[2] += g_z;
        double gc[3];
        if (a.mode == 1) { gc[0] = g_t[0]; gc[1] = g_t[1]; gc[2] = g_t[2]; }
        else {                                                 // t = 2 (c1 / s, c2 / s, 1 / s)
            const double s = (double)a.cam[(size_t)n * 3], c1 = (double)a.cam[(size_t)n * 3 + 1], c2 = (double)a.cam[(size_t)n * 3 + 2];
            gc[0] = -2.0 * (c1 * g_t[0] + c2 * g_t[1] + g_t[2]) / (s * s);
            gc[1] = 2.0 * g_t[0] / s;
            gc[2] = 2.0 * g_t[1] / s;
        }
        for (int x = 0; x < 3; ++x) scene_put(a.grad_cam + (size_t)n * 3 + x, gc[x], a.accumulate_cam);
        const float ld = (float)l_depth, lc = (float)l_col;
        if (a.loss) { a.loss[(size_t)n * 2] = ld; a.loss[(size_t)n * 2 + 1] = lc; }
        if (a.history) { a.history[(size_t)n * 2] = ld; a.history[(size_t)n * 2 + 1] = lc; }
    }
}

}  // namespace romp

using namespace romp;

extern "C" int romp_fit_scene(const float* joints, int N, int J, const float* cam, int camera_mode, const int32_t* offsets,
                              const int32_t* members, const int32_t* depth_ids, float w_depth, float dist_thresh, int kind,
                              const romp_scene_sphere* spheres_host, int S, const float* radius_scale, float w_col,
                              const float* term_w, float* grad_joints, int accumulate_joints, float* grad_cam, int accumulate_cam,
                              float* loss, float* loss_history, int history_row, void* stream) {
    ROMP_REQUIRE(cam && offsets && members && grad_cam, "romp_fit_scene: null cam, offsets, members or grad_cam");
    ROMP_REQUIRE(S >= 0 && S <= ROMP_SCENE_MAX_SPHERES, "romp_fit_scene: S %d (0..%d)", S, ROMP_SCENE_MAX_SPHERES);
    ROMP_REQUIRE(S == 0 || (joints && grad_joints && spheres_host), "romp_fit_scene: spheres without joints, grad_joints or the table");
    ROMP_REQUIRE(depth_ids || S > 0, "romp_fit_scene: neither depth labels nor spheres");
    ROMP_REQUIRE(N >= 0, "romp_fit_scene: N %d", N);
    ROMP_REQUIRE(S == 0 || (J >= 1 && J <= ROMP_FIT_MAX_JOINTS), "romp_fit_scene: J %d (1..%d)", J, ROMP_FIT_MAX_JOINTS);
    ROMP_REQUIRE(camera_mode == 0 || camera_mode == 1, "romp_fit_scene: camera_mode %d", camera_mode);
    ROMP_REQUIRE(kind == ROMP_SCENE_PIECEWISE || kind == ROMP_SCENE_LOG, "romp_fit_scene: kind %d", kind);
    ROMP_REQUIRE(w_depth >= 0.f && w_col >= 0.f, "romp_fit_scene: a negative or NaN weight (%g, %g)", (double)w_depth, (double)w_col);
    ROMP_REQUIRE(dist_thresh >= 0.f, "romp_fit_scene: dist_thresh %g", (double)dist_thresh);
    ROMP_REQUIRE(history_row >= 0, "romp_fit_scene: history_row %d", history_row);
    ROMP_REQUIRE(loss || w_depth > 0.f || w_col > 0.f, "romp_fit_scene: both weights are zero and there is no loss output");
    scene_args a = {};
    for (int s = 0; s < S; ++s) {
        const romp_scene_sphere& sp = spheres_host[s];
        ROMP_REQUIRE(sp.p >= 0 && sp.p < J && sp.q >= 0 && sp.q < J, "romp_fit_scene: sphere %d names joints %d, %d outside 0..%d", s,
                     (int)sp.p, (int)sp.q, J - 1);
        ROMP_REQUIRE(std::isfinite(sp.a) && std::isfinite(sp.r) && sp.r > 0.f, "romp_fit_scene: sphere %d has a = %g, r = %g (finite, r > 0)", s,
                     (double)sp.a, (double)sp.r);
        a.sph[s] = sp;
    }
    if (N == 0) return ROMP_OK;
    a.joints = joints; a.cam = cam; a.radius_scale = radius_scale; a.term_w = term_w;
    a.offsets = offsets; a.members = members; a.depth_ids = depth_ids;
    a.grad_joints = grad_joints; a.grad_cam = grad_cam; a.loss = loss;
    a.history = loss_history ? loss_history + (size_t)history_row * N * 2 : nullptr;
    a.N = N; a.J = J; a.S = S; a.mode = camera_mode; a.kind = kind;
    a.accumulate_joints = accumulate_joints; a.accumulate_cam = accumulate_cam;
    a.w_depth = w_depth; a.w_col = w_col; a.thresh = dist_thresh;
    hipLaunchKernelGGL(fit_scene_kernel, dim3((unsigned)N), dim3(SCENE_THREADS), 0, (hipStream_t)stream, a);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}
