// eval.hip -- benchmark scoring on the device (include/romp_hip_eval.h): greedy 2-D matching of predictions to ground
// truth, per-person MPJPE / Procrustes-aligned MPJPE over 2 .. 6890 points, and a float64 running accumulator.
//
// Reference: simple_romp/evaluation/RH_evaluation/matching.py match_2d_greedy :51-171, get_bbx_overlap :7-49;
// romp/lib/evaluation/evaluation_matrix.py batch_compute_similarity_transform_torch :252-303, compute_mpjpe :306-322,
// compute_error_verts :105-122; romp/lib/loss_funcs/keypoints_loss.py align_by_parts :64-68, calc_mpjpe :70-82,
// calc_pampjpe :84-93; simple_romp/evaluation/eval_cmu_panoptic.py :300-311.
//
// match2d_kernel: one wave per image, the pair table in LDS, every lane takes the same decisions from shuffled minima.
// points_kernel: one workgroup per ground-truth row; three passes over the row (means, centred moments, aligned error),
// each reduced wave-shuffle -> LDS -> a fixed-order sum, all in float64; thread 0 finds the rotation as the top eigenvector
// of Horn's 4x4 matrix of K by Jacobi rotations, which never divides by a vanishing singular value.  No atomics anywhere: the outputs are deterministic.
#include "common.h"
#include "../../include/romp_hip_eval.h"
#include <math.h>

namespace romp {

constexpr int EVAL_LDS_BYTES = 64 * 1024;
constexpr int PT_THREADS = 256, PT_WAVES = PT_THREADS / 64;

static size_t match_lds_bytes(int max_pred, int max_gt) {
    return sizeof(float) * ((size_t)max_pred * max_gt + 4 * (size_t)max_pred + 4 * (size_t)max_gt) +
           sizeof(int32_t) * ((size_t)max_pred + max_gt);
}

__device__ __forceinline__ void box_of(const float* __restrict__ kp, int J, float* box) {      // x1, x2, y1, y2 over all joints
    float x1 = kp[0], x2 = kp[0], y1 = kp[1], y2 = kp[1];
    for (int j = 1; j < J; ++j) {
        const float x = kp[2 * j], y = kp[2 * j + 1];
        x1 = fminf(x1, x); x2 = fmaxf(x2, x); y1 = fminf(y1, y); y2 = fmaxf(y2, y);
    }
    box[0] = x1; box[1] = x2; box[2] = y1; box[3] = y2;
}

__device__ __forceinline__ float box_iou(const float* a, const float* b) {                      // get_bbx_overlap, float32
    const float xl = fmaxf(a[0], b[0]), yt = fmaxf(a[2], b[2]), xr = fminf(a[1], b[1]), yb = fminf(a[3], b[3]);
    const float inter = fmaxf(0.f, xr - xl + 1.f) * fmaxf(0.f, yb - yt + 1.f);
    const float a1 = (a[1] - a[0] + 1.f) * (a[3] - a[2] + 1.f), a2 = (b[1] - b[0] + 1.f) * (b[3] - b[2] + 1.f);
    return inter / (a1 + a2 - inter);
}

__global__ __launch_bounds__(64) void match2d_kernel(const float* __restrict__ pkp, const int32_t* __restrict__ poff,
                                                     const float* __restrict__ gkp, const uint8_t* __restrict__ gvalid,
                                                     const int32_t* __restrict__ goff, int J, int max_pred, int max_gt,
                                                     float iou_thresh, int norm, int32_t* __restrict__ gt_of_pred,
                                                     int32_t* __restrict__ pred_of_gt, int32_t* __restrict__ over_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    float* err = (float*)lds_raw;                                 // (P, G), +inf once consumed
    float* pbox = err + (size_t)max_pred * max_gt;                // (max_pred, 4)
    float* gbox = pbox + 4 * (size_t)max_pred;                    // (max_gt, 4)
    int32_t* p_to_g = (int32_t*)(gbox + 4 * (size_t)max_gt);      // (max_pred) local g or -1
    int32_t* g_to_p = p_to_g + max_pred;                          // (max_gt)
    const int b = blockIdx.x, lane = threadIdx.x;
    const int p0 = poff[b], g0 = goff[b];
    const int P = max(poff[b + 1] - p0, 0), G = max(goff[b + 1] - g0, 0);
    const bool over = P > max_pred || G > max_gt;
    if (over_cap && lane == 0) over_cap[b] = over ? 1 : 0;
    if (over || P == 0 || G == 0) {
        for (int i = lane; i < P; i += 64) gt_of_pred[p0 + i] = -1;
        for (int i = lane; i < G; i += 64) pred_of_gt[g0 + i] = -1;
        return;
    }
    for (int i = lane; i < P; i += 64) { box_of(pkp + (size_t)(p0 + i) * J * 2, J, pbox + 4 * i); p_to_g[i] = -1; }
    for (int i = lane; i < G; i += 64) { box_of(gkp + (size_t)(g0 + i) * J * 2, J, gbox + 4 * i); g_to_p[i] = -1; }
    const int n = P * G;
    for (int i = lane; i < n; i += 64) {
        const int p = i / G, g = i - p * G;
        const float* a = pkp + (size_t)(p0 + p) * J * 2;
        const float* c = gkp + (size_t)(g0 + g) * J * 2;
        const uint8_t* v = gvalid + (size_t)(g0 + g) * J;
        float sxx = 0.f, syy = 0.f, sxy = 0.f;
        for (int j = 0; j < J; ++j)
            if (v[j]) {
                const float dx = a[2 * j] - c[2 * j], dy = a[2 * j + 1] - c[2 * j + 1];
                sxx += dx * dx; syy += dy * dy; sxy += dx * dy;
            }
        float e;
        if (norm == ROMP_EVAL_NORM_SPECTRAL) {
            const float h = 0.5f * (sxx + syy), d = 0.5f * (sxx - syy);
            e = sqrtf(h + sqrtf(d * d + sxy * sxy));
        } else {
            e = sqrtf(sxx + syy);
        }
        err[i] = e;
    }
    __syncthreads();

    int n_match = 0, n_fp = 0;                                    // the same in every lane
    while (n_match < G && n_match + n_fp < P) {
        float bv = INFINITY;
        int bi = 0x7fffffff;
        for (int i = lane; i < n; i += 64) {
            const float v = err[i];
            if (v < bv) { bv = v; bi = i; }
        }
        for (int m = 1; m < 64; m <<= 1) {
            const float ov = __shfl_xor(bv, m, 64);
            const int oi = __shfl_xor(bi, m, 64);
            if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (bi == 0x7fffffff) break;                               // every pair consumed: the reference would spin here
        const int p = bi / G, g = bi - p * G;
        const float iou = box_iou(pbox + 4 * p, gbox + 4 * g);
        const bool is_free = p_to_g[p] < 0 && g_to_p[g] < 0;
        __syncthreads();                                           // every lane has read the table and the flags
        if (lane == 0) err[bi] = INFINITY;
        if (is_free && iou >= iou_thresh) {
            if (lane == 0) { p_to_g[p] = g; g_to_p[g] = p; }
            ++n_match;
        } else if (iou < iou_thresh) {
            ++n_fp;
        }
        __syncthreads();
    }
    for (int i = lane; i < P; i += 64) gt_of_pred[p0 + i] = p_to_g[i] < 0 ? -1 : g0 + p_to_g[i];
    for (int i = lane; i < G; i += 64) pred_of_gt[g0 + i] = g_to_p[i] < 0 ? -1 : p0 + g_to_p[i];
}

// ------------------------------------------------------------------------------------------------ per-row metrics
template <int N>
__device__ __forceinline__ void block_sum(double (&v)[N], double (*s_part)[PT_WAVES], double* s_out) {
    // wave shuffle -> LDS -> thread k adds the waves' sums of element k in index order; every thread then reads s_out[0..N)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double x = v[k];
        for (int m = 32; m >= 1; m >>= 1) x += __shfl_down(x, m, 64);
        if (lane == 0) s_part[k][wave] = x;
    }
    __syncthreads();
    if (threadIdx.x < N) {
        double x = 0.0;
        for (int w = 0; w < PT_WAVES; ++w) x += s_part[threadIdx.x][w];
        s_out[threadIdx.x] = x;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = s_out[k];
    __syncthreads();                                              // s_part / s_out are free for the next reduction
}

// The proper rotation R that maximises trace(R K), K = X1 X2^T row-major -- what evaluation_matrix.py :281-289 builds as
// V Z U^T with Z33 = sign det(U V^T) -- as the unit quaternion of the largest eigenvalue of Horn's symmetric 4x4 matrix of K,
// found by cyclic Jacobi rotations.  Nothing is divided by a singular value, so K of rank 2 (planar sets; R is still
// unique) and of rank 1 (collinear sets, P = 2; some maximiser) need no special case, and the reflection fix is built in:
// only proper rotations are searched.  Jacobi skips an off-diagonal element that is exactly zero, so a symmetric K
// (pred == target) keeps the eigenvector (1,0,0,0) and gives R = I exactly.
__device__ void procrustes_rotation(const double* K, double* R) {
    const double Sxx = K[0], Sxy = K[1], Sxz = K[2], Syx = K[3], Syy = K[4], Syz = K[5], Szx = K[6], Szy = K[7], Szz = K[8];
    double a[4][4] = {{Sxx + Syy + Szz, Syz - Szy, Szx - Sxz, Sxy - Syx},
                      {Syz - Szy, Sxx - Syy - Szz, Sxy + Syx, Szx + Sxz},
                      {Szx - Sxz, Sxy + Syx, -Sxx + Syy - Szz, Syz + Szy},
                      {Sxy - Syx, Szx + Sxz, Syz + Szy, -Sxx - Syy + Szz}};
    double v[4][4];                                                // v[r][c]: component r of eigenvector c
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) v[r][c] = r == c ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        double off = 0.0, diag = 0.0;
        for (int p = 0; p < 4; ++p) {
            diag += a[p][p] * a[p][p];
            for (int q = p + 1; q < 4; ++q) off += a[p][q] * a[p][q];
        }
        if (!(off > 1e-34 * diag)) break;                          // converged (or not finite: the row is non-finite anyway)
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                const double apq = a[p][q];
                if (apq == 0.0) continue;
                const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
                const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 4; ++k) {                      // A <- A J
                    const double akp = a[k][p], akq = a[k][q];
                    a[k][p] = c * akp - s * akq; a[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 4; ++k) {                      // A <- J^T A
                    const double apk = a[p][k], aqk = a[q][k];
                    a[p][k] = c * apk - s * aqk; a[q][k] = s * apk + c * aqk;
                }
                a[p][q] = 0.0; a[q][p] = 0.0;
                for (int k = 0; k < 4; ++k) {
                    const double vkp = v[k][p], vkq = v[k][q];
                    v[k][p] = c * vkp - s * vkq; v[k][q] = s * vkp + c * vkq;
                }
            }
    }
    int m = 0;
    for (int c = 1; c < 4; ++c)
        if (a[c][c] > a[m][m]) m = c;
    double w = v[0][m], x = v[1][m], y = v[2][m], z = v[3][m];
    const double n = sqrt(w * w + x * x + y * y + z * z);
    w /= n; x /= n; y /= n; z /= n;
    R[0] = w * w + x * x - y * y - z * z; R[1] = 2.0 * (x * y - w * z);         R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z);         R[4] = w * w - x * x + y * y - z * z; R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y);         R[7] = 2.0 * (y * z + w * x);         R[8] = w * w - x * x - y * y + z * z;
}

__global__ __launch_bounds__(PT_THREADS) void points_kernel(const float* __restrict__ pred, int Np, const float* __restrict__ target,
                                                            int P, const int32_t* __restrict__ pred_of_gt,
                                                            const int32_t* __restrict__ align_inds, int n_align,
                                                            const uint8_t* __restrict__ vis, const uint8_t* __restrict__ point_mask,
                                                            float* __restrict__ mpjpe, float* __restrict__ mpjpe_all,
                                                            float* __restrict__ pa_mpjpe, float* __restrict__ sRt,
                                                            float* __restrict__ aligned) {
    __shared__ double s_part[14][PT_WAVES];
    __shared__ double s_out[14];
    __shared__ double s_tf[13];                                    // scale, R, t
    const int g = blockIdx.x, tid = threadIdx.x;
    const int p = pred_of_gt ? pred_of_gt[g] : g;
    if (p < 0 || p >= Np) {                                        // a miss: NaN everywhere
        const float nan = __builtin_nanf("");
        if (tid == 0) {
            if (mpjpe) mpjpe[g] = nan;
            if (mpjpe_all) mpjpe_all[g] = nan;
            if (pa_mpjpe) pa_mpjpe[g] = nan;
        }
        if (sRt && tid < 13) sRt[(size_t)g * 13 + tid] = nan;
        if (aligned)
            for (int i = tid; i < 3 * P; i += PT_THREADS) aligned[(size_t)g * P * 3 + i] = nan;
        return;
    }
    const float* x1 = pred + (size_t)p * P * 3;
    const float* x2 = target + (size_t)g * P * 3;
    const uint8_t* vrow = vis ? vis + (size_t)g * P : nullptr;

    // pass 1: the means -- of the align_inds points (MPJPE) and of the masked points (Procrustes)
    double m[13];
    for (int k = 0; k < 13; ++k) m[k] = 0.0;
    for (int i = tid; i < n_align; i += PT_THREADS) {
        const int j = align_inds[i];
        if (j >= 0 && j < P)
            for (int c = 0; c < 3; ++c) { m[c] += (double)x1[3 * j + c]; m[3 + c] += (double)x2[3 * j + c]; }
    }
    for (int i = tid; i < P; i += PT_THREADS)
        if (!point_mask || point_mask[i]) {
            for (int c = 0; c < 3; ++c) { m[6 + c] += (double)x1[3 * i + c]; m[9 + c] += (double)x2[3 * i + c]; }
            m[12] += 1.0;
        }
    block_sum<13>(m, s_part, s_out);
    double a1[3], a2[3], mu1[3], mu2[3];
    const double n_pts = m[12];
    for (int c = 0; c < 3; ++c) {
        a1[c] = n_align > 0 ? m[c] / n_align : 0.0;
        a2[c] = n_align > 0 ? m[3 + c] / n_align : 0.0;
        mu1[c] = m[6 + c] / n_pts;
        mu2[c] = m[9 + c] / n_pts;
    }

    // pass 2: centred moments (about the means: no cancellation far from the origin) K = X1 X2^T and var1, kept per
    // coordinate and summed exactly as K's diagonal is, so that pred == target gives scale = 1 exactly; the MPJPE sums
    double q[14];
    for (int k = 0; k < 14; ++k) q[k] = 0.0;
    for (int i = tid; i < P; i += PT_THREADS) {
        double u[3], w[3];
        for (int c = 0; c < 3; ++c) { u[c] = (double)x1[3 * i + c]; w[c] = (double)x2[3 * i + c]; }
        const double dx = (u[0] - a1[0]) - (w[0] - a2[0]), dy = (u[1] - a1[1]) - (w[1] - a2[1]), dz = (u[2] - a1[2]) - (w[2] - a2[2]);
        const double vv = vrow ? (vrow[i] ? 1.0 : 0.0) : 1.0;
        q[12] += sqrt(dx * dx + dy * dy + dz * dz) * vv;
        q[13] += vv;
        if (!point_mask || point_mask[i]) {
            for (int c = 0; c < 3; ++c) { u[c] -= mu1[c]; w[c] -= mu2[c]; }
            for (int r = 0; r < 3; ++r) {
                q[9 + r] = fma(u[r], u[r], q[9 + r]);
                for (int c = 0; c < 3; ++c) q[r * 3 + c] = fma(u[r], w[c], q[r * 3 + c]);
            }
        }
    }
    block_sum<14>(q, s_part, s_out);
    if (tid == 0) {
        if (mpjpe) mpjpe[g] = (float)(q[12] / q[13]);
        if (mpjpe_all) mpjpe_all[g] = (float)(q[12] / (double)P);
        double R[9];
        procrustes_rotation(q, R);
        double tr = 0.0;                                           // trace(R K), rows in order
        for (int r = 0; r < 3; ++r) tr += (R[r * 3] * q[r] + R[r * 3 + 1] * q[3 + r]) + R[r * 3 + 2] * q[6 + r];
        const double scale = tr / ((q[9] + q[10]) + q[11]);
        s_tf[0] = scale;
        for (int k = 0; k < 9; ++k) s_tf[1 + k] = R[k];
        for (int r = 0; r < 3; ++r)
            s_tf[10 + r] = mu2[r] - scale * (R[r * 3] * mu1[0] + R[r * 3 + 1] * mu1[1] + R[r * 3 + 2] * mu1[2]);
    }
    __syncthreads();
    if (sRt && tid < 13) sRt[(size_t)g * 13 + tid] = (float)s_tf[tid];
    if (!pa_mpjpe && !aligned) return;

    // pass 3: aligned = scale R x + t, its distance to the target over the masked points
    const double sc = s_tf[0];
    double e[1] = {0.0};
    for (int i = tid; i < P; i += PT_THREADS) {
        const double u0 = (double)x1[3 * i], u1 = (double)x1[3 * i + 1], u2 = (double)x1[3 * i + 2];
        double y[3];
        for (int r = 0; r < 3; ++r) y[r] = sc * (s_tf[1 + r * 3] * u0 + s_tf[2 + r * 3] * u1 + s_tf[3 + r * 3] * u2) + s_tf[10 + r];
        if (aligned)
            for (int r = 0; r < 3; ++r) aligned[((size_t)g * P + i) * 3 + r] = (float)y[r];
        if (!point_mask || point_mask[i]) {
            const double dx = y[0] - (double)x2[3 * i], dy = y[1] - (double)x2[3 * i + 1], dz = y[2] - (double)x2[3 * i + 2];
            e[0] += sqrt(dx * dx + dy * dy + dz * dz);
        }
    }
    block_sum<1>(e, s_part, s_out);
    if (pa_mpjpe && tid == 0) pa_mpjpe[g] = (float)(e[0] / n_pts);
}

// ------------------------------------------------------------------------------------------------ accumulator
constexpr int ACC_MAX_METRICS = 8;

__global__ __launch_bounds__(PT_THREADS) void accumulate_kernel(const float* __restrict__ metrics, int n_metrics, int Ng,
                                                                const int32_t* __restrict__ pred_of_gt,
                                                                const int32_t* __restrict__ gt_of_pred, int Np,
                                                                const int32_t* __restrict__ over_cap, int B, double* __restrict__ acc) {
    __shared__ double s_part[2][PT_WAVES];
    __shared__ double s_out[2];
    const int tid = threadIdx.x;
    for (int k = 0; k < n_metrics; ++k) {
        double v[2] = {0.0, 0.0};
        for (int i = tid; i < Ng; i += PT_THREADS) {
            const float x = metrics[(size_t)k * Ng + i];
            if (isfinite(x)) { v[0] += (double)x; v[1] += 1.0; }
        }
        block_sum<2>(v, s_part, s_out);
        if (tid == 0) { acc[2 * k] += v[0]; acc[2 * k + 1] += v[1]; }
    }
    double c[2] = {0.0, 0.0};
    for (int i = tid; i < Ng; i += PT_THREADS) c[0] += pred_of_gt[i] < 0 ? 1.0 : 0.0;
    for (int i = tid; i < Np; i += PT_THREADS) c[1] += gt_of_pred[i] < 0 ? 1.0 : 0.0;
    block_sum<2>(c, s_part, s_out);
    double o[2] = {0.0, 0.0};
    if (over_cap)
        for (int i = tid; i < B; i += PT_THREADS) o[0] += over_cap[i] ? 1.0 : 0.0;
    block_sum<2>(o, s_part, s_out);
    if (tid == 0) {
        double* tail = acc + 2 * n_metrics;
        tail[0] += c[0]; tail[1] += c[1]; tail[2] += (double)Ng; tail[3] += (double)Np; tail[4] += o[0];
    }
}

}  // namespace romp

using namespace romp;

extern "C" {

int romp_eval_match2d(const float* pred_kp2d, const int32_t* pred_offsets, const float* gt_kp2d, const uint8_t* gt_valid,
                      const int32_t* gt_offsets, int B, int J, int max_pred, int max_gt, float iou_thresh, int norm,
                      int32_t* gt_of_pred, int32_t* pred_of_gt, int32_t* over_cap, void* stream) {
    ROMP_REQUIRE(pred_offsets && gt_offsets && B > 0 && J > 0 && max_pred > 0 && max_gt > 0,
                 "romp_eval_match2d: bad arguments (B %d, J %d, caps %d x %d)", B, J, max_pred, max_gt);
    ROMP_REQUIRE(norm == ROMP_EVAL_NORM_FROBENIUS || norm == ROMP_EVAL_NORM_SPECTRAL, "romp_eval_match2d: norm %d", norm);
    const size_t lds = match_lds_bytes(max_pred, max_gt);
    ROMP_REQUIRE(lds <= (size_t)EVAL_LDS_BYTES, "romp_eval_match2d: a %d x %d pair table needs %zu bytes of LDS, %d available",
                 max_pred, max_gt, lds, EVAL_LDS_BYTES);
    hipLaunchKernelGGL(match2d_kernel, dim3(B), dim3(64), lds, (hipStream_t)stream, pred_kp2d, pred_offsets, gt_kp2d, gt_valid,
                       gt_offsets, J, max_pred, max_gt, iou_thresh, norm, gt_of_pred, pred_of_gt, over_cap);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_eval_points(const float* pred, int Np, const float* target, int Ng, int P, const int32_t* pred_of_gt,
                     const int32_t* align_inds, int n_align, const uint8_t* vis, const uint8_t* point_mask,
                     float* mpjpe, float* mpjpe_all, float* pa_mpjpe, float* sRt, float* aligned, void* stream) {
    ROMP_REQUIRE(P >= 2, "romp_eval_points: P = %d, a similarity transform needs at least 2 points", P);
    ROMP_REQUIRE(Np >= 0 && Ng >= 0 && n_align >= 0 && (n_align == 0 || align_inds), "romp_eval_points: bad arguments");
    if (Ng == 0) return ROMP_OK;
    ROMP_REQUIRE(target && (pred || Np == 0), "romp_eval_points: null points");
    hipLaunchKernelGGL(points_kernel, dim3(Ng), dim3(PT_THREADS), 0, (hipStream_t)stream, pred, Np, target, P, pred_of_gt,
                       align_inds, n_align, vis, point_mask, mpjpe, mpjpe_all, pa_mpjpe, sRt, aligned);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_eval_accumulate(const float* metrics, int n_metrics, int Ng, const int32_t* pred_of_gt, const int32_t* gt_of_pred,
                         int Np, const int32_t* over_cap, int B, double* acc, void* stream) {
    ROMP_REQUIRE(acc && n_metrics >= 0 && n_metrics <= ACC_MAX_METRICS && Ng >= 0 && Np >= 0 && B >= 0 &&
                 (metrics || n_metrics == 0 || Ng == 0) && (pred_of_gt || Ng == 0) && (gt_of_pred || Np == 0),
                 "romp_eval_accumulate: bad arguments");
    hipLaunchKernelGGL(accumulate_kernel, dim3(1), dim3(PT_THREADS), 0, (hipStream_t)stream, metrics, n_metrics, Ng, pred_of_gt,
                       gt_of_pred, Np, over_cap, B, acc);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

}  // extern "C"
