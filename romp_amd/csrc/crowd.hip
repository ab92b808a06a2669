// crowd.hip -- BEV's long-image "crowd" mode (simple_romp/bev/main.py:184-258, bev/split2process.py) on the device: a wide frame
// is cut into overlapping square-ish crops of a virtually zero-padded frame, all crops go through one batched network call, and
// the per-crop people are merged into one full-frame result.
//
//  * crowd_preprocess_kernel: padding_image_overlap + the crop cut + img_preprocess (utils.py:16-30) for every crop in one launch:
//    each crop gets its own centred square pad and cubic tables (cv_cubic.h, bit-exact with the single-frame path).  The frame is
//    read where it lies; the padded frame is never built.
//
//  * the merge, four kernels on the caller's stream:
//    crowd_crop_kernel     one workgroup per crop: exclude_boudary_subjects (tolerance 0), the projection with the crop's own
//                          offsets [0, ch, 0, cw, ch, cw], conf-based suppressing_redundant_prediction_via_projection, remove_outlier
//                          (scale_thresh 1), then convert_crop_cam_params2full_image;
//    crowd_list_kernel     one workgroup: the crop-stage survivors as a row-ordered list (collect_outputs keeps crop order);
//    crowd_project_kernel  the full-frame projection with padding_image_overlap's pad info;
//    crowd_pairs_kernel    the global conf-based suppression over all survivor pairs, spread over workgroups (the removal is an OR
//                          over pairs, so no ordering is needed);
//    crowd_outlier_kernel  one workgroup: remove_outlier (scale_thresh 0.5) over what is left, and the keep mask.
//    Arithmetic follows the reference's float32 torch ops one by one (no contraction into FMAs); the thresholds the reference
//    computes in double are computed in double on the host and rounded to float32, as torch rounds a Python scalar.
#include <math.h>

#include "common.h"
#include "cv_cubic.h"

namespace romp {

constexpr int CROWD_CHUNK = 64;        // crops per launch (their parameters travel as kernel arguments)
constexpr int CJ = 71;                 // joints per person
constexpr float CROWD_TAN_FOV = 0.57735026918962573f;

struct CropWindows {                   // crop c: window of the FRAME starting at (y0, x0), h x w (may reach into the zero padding)
    int y0[CROWD_CHUNK], x0[CROWD_CHUNK], h[CROWD_CHUNK], w[CROWD_CHUNK];
};

struct CropMerge {                     // per-crop constants of the merge (split2process.py / post_parser.py)
    float drop_hi[CROWD_CHUNK];        // cam_x >  drop_hi: beyond the overlap with the next crop (+inf: last crop)
    float drop_lo[CROWD_CHUNK];        // cam_x <  drop_lo: beyond the overlap with the previous crop (-inf: crops 0 and 1)
    float nms_thr[CROWD_CHUNK];        // nms_thresh * max(ch, cw) / 640
    float pad[CROWD_CHUNK];            // max(ch, cw): the projection's square size
    float scale[CROWD_CHUNK];          // max(crop w, crop h) / max(H, W)
    float shift[CROWD_CHUNK];          // mean(left, right) / (W / 2) - 1 (frame coordinates)
};

__global__ __launch_bounds__(256) void crowd_preprocess_kernel(const unsigned char* __restrict__ src, int H, int W, CropWindows t,
                                                               int c_base, float* __restrict__ dst_all, int S) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S * S) return;
    const int c = blockIdx.y;
    const int y0 = t.y0[c], x0 = t.x0[c], h = t.h[c], w = t.w[c];
    const int side = max(h, w), top = (side - h) / 2, left = (side - w) / 2;
    const int ylo = max(0, -y0), yhi = max(ylo, min(h, H - y0));     // the window's pixels that lie in the frame
    const int xlo = max(0, -x0), xhi = max(xlo, min(w, W - x0));
    float* dst = dst_all + ((size_t)(c_base + c) * S * S + i) * 3;
    cv_cubic_pixel(src, (size_t)W * 3, y0, x0, ylo, yhi, xlo, xhi, side, top, left, i % S, i / S, S, dst);
}

// denormalize_cam_params_to_trans (bev/post_parser.py:114-128)
__device__ __forceinline__ void crowd_trans(const float* c, float* tr) {
#pragma clang fp contract(off)
    const float depth = 1.f / (c[0] * CROWD_TAN_FOV + 1e-3f);
    tr[0] = c[2] * depth * CROWD_TAN_FOV; tr[1] = c[1] * depth * CROWD_TAN_FOV; tr[2] = depth;
}

// perspective_projection (focal 443.4, normalised by 256) + convert_proejection_from_input_to_orgimg for one joint
__device__ __forceinline__ void crowd_project(const float* j, const float* tr, float pad, float top, float left, float* out) {
#pragma clang fp contract(off)
    const float z = (j[2] + tr[2]) + 1e-6f;
    float x = (j[0] + tr[0]) / z * 443.4f, y = (j[1] + tr[1]) / z * 443.4f;
    x /= 256.f; y /= 256.f;
    out[0] = (x + 1.f) * pad / 2.f - left;
    out[1] = (y + 1.f) * pad / 2.f - top;
}

// mean over the joints of the pixel distance of persons a and b (pj2d_dist_mat), normalised by the larger scale
__device__ __forceinline__ float crowd_pair_dist(const float* __restrict__ pj, int a, int b, float sa, float sb) {
#pragma clang fp contract(off)
    const float2* pa = (const float2*)(pj + (size_t)a * CJ * 2);
    const float2* pb = (const float2*)(pj + (size_t)b * CJ * 2);
    float d = 0.f;
    for (int k = 0; k < CJ; ++k) {
        const float2 u = pa[k], v = pb[k];
        const float dx = u.x - v.x, dy = u.y - v.y;
        d += sqrtf(dx * dx + dy * dy);
    }
    return d / CJ / fmaxf(sa, sb);
}

// Order-keeping compaction by one workgroup: out[0..m) = val(r) for the r in [0, n) with pred(r); returns m in every thread.
// May run in place (out[k] = f(out[k])): a chunk reads all its entries before it writes, and writes never pass its reads.
template <class Pred, class Val>
__device__ int crowd_block_compact(int n, Pred pred, Val val, int* out, int* s_wave /* [blockDim/64 + 1] */) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
    int total = 0;
    for (int base = 0; base < n; base += blockDim.x) {
        const int r = base + tid;
        const bool p = r < n && pred(r);
        const int v = p ? val(r) : 0;
        const unsigned long long mask = __ballot(p);
        if (lane == 0) s_wave[wave] = __popcll(mask);
        __syncthreads();
        int before = total;
        for (int k = 0; k < wave; ++k) before += s_wave[k];
        int chunk = 0;
        for (int k = 0; k < nw; ++k) chunk += s_wave[k];
        if (p) out[before + __popcll(mask & ((1ull << lane) - 1ull))] = v;
        total += chunk;
        __syncthreads();
    }
    return total;
}

// remove_outlier (bev/post_parser.py:200-222) over the m >= 3 persons list[0..m): marks flag[row] = mark for the outliers.
// mean[k]: mean distance of person k to the others without the row's smallest and largest entry (sorted()[1:-1]).
__device__ void crowd_outlier(const int* __restrict__ list, int m, const float* __restrict__ trans, const float* __restrict__ cam,
                              float rel_thresh, float scale_thresh, float* __restrict__ mean, int* __restrict__ flag, int mark,
                              float* s_red) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    for (int k = tid; k < m; k += blockDim.x) {
        const float* ta = trans + (size_t)list[k] * 3;
        float sum = 0.f, mn = 3.4e38f, mx = -1.f;
        for (int q = 0; q < m; ++q) {
            const float* tb = trans + (size_t)list[q] * 3;
            const float dx = ta[0] - tb[0], dy = ta[1] - tb[1], dz = ta[2] - tb[2];
            const float d = sqrtf(dx * dx + dy * dy + dz * dz);
            sum += d; mn = fminf(mn, d); mx = fmaxf(mx, d);
        }
        mean[k] = (sum - mn - mx) / (float)(m - 2);
    }
    __syncthreads();
    float part = 0.f;
    for (int k = tid; k < m; k += blockDim.x) part += mean[k];
    s_red[tid] = part;
    __syncthreads();
    for (int s = blockDim.x / 2; s > 0; s >>= 1) {
        if (tid < s) s_red[tid] += s_red[tid + s];
        __syncthreads();
    }
    const float tot = s_red[0];
    for (int k = tid; k < m; k += blockDim.x) {
        const float rel = mean[k] / ((tot - mean[k]) / (float)(m - 1));
        const int row = list[k];
        if (rel > rel_thresh && cam[(size_t)row * 3] < scale_thresh) flag[row] = mark;
    }
    __syncthreads();
}

// Crop stage, one workgroup per crop.  flag[row]: 0 alive, 1 boundary-excluded, 2 suppressed, 3 outlier.  The crop-space
// projection and translation go to pj / trans (the full-frame stage overwrites them); cam_full gets the converted camera.
__global__ __launch_bounds__(256) void crowd_crop_kernel(const float* __restrict__ joints, const float* __restrict__ cam,
                                                         const float* __restrict__ conf, const int* __restrict__ offsets, int N,
                                                         int c_base, CropMerge t, float rel_thresh, float* __restrict__ cam_full,
                                                         float* __restrict__ trans, float* __restrict__ pj, int* __restrict__ flag,
                                                         int* __restrict__ list, float* __restrict__ mean) {
#pragma clang fp contract(off)
    __shared__ int s_wave[5];
    __shared__ float s_red[256];
    const int cl = blockIdx.x, c = c_base + cl, tid = threadIdx.x;
    const int o0 = min(max(offsets[c], 0), N), o1 = min(max(offsets[c + 1], o0), N), n = o1 - o0;
    if (n == 0) return;
    const float drop_hi = t.drop_hi[cl], drop_lo = t.drop_lo[cl], scale = t.scale[cl], shift = t.shift[cl], pad = t.pad[cl];
    for (int r = tid; r < n; r += blockDim.x) {
        const int row = o0 + r;
        const float* cm = cam + (size_t)row * 3;
        flag[row] = (cm[2] > drop_hi || cm[2] < drop_lo) ? 1 : 0;         // exclude_boudary_subjects, both sides
        crowd_trans(cm, trans + (size_t)row * 3);
        float* cf = cam_full + (size_t)row * 3;                           // convert_crop_cam_params2full_image
        cf[0] = cm[0] * scale; cf[1] = cm[1] * scale; cf[2] = cm[2] * scale + shift;
    }
    __syncthreads();
    for (int i = tid; i < n * CJ; i += blockDim.x) {
        const int row = o0 + i / CJ, k = i % CJ;
        crowd_project(joints + ((size_t)row * CJ + k) * 3, trans + (size_t)row * 3, pad, 0.f, 0.f, pj + ((size_t)row * CJ + k) * 2);
    }
    int* lst = list + o0;
    float* mn = mean + o0;
    const int m1 = crowd_block_compact(n, [&](int r) { return flag[o0 + r] == 0; }, [&](int r) { return o0 + r; }, lst, s_wave);
    __syncthreads();
    if (m1 > 1) {                                                         // suppressing_redundant_prediction_via_projection
        const float thr = t.nms_thr[cl];
        for (int p = tid; p < m1 * m1; p += blockDim.x) {
            const int a = p / m1, b = p % m1;
            if (a >= b) continue;
            const int ra = lst[a], rb = lst[b];
            const float d = crowd_pair_dist(pj, ra, rb, cam[(size_t)ra * 3] * 2.f, cam[(size_t)rb * 3] * 2.f);
            if (d < thr) atomicExch(&flag[conf[ra] < conf[rb] ? ra : rb], 2);
        }
    }
    __syncthreads();
    const int m2 = crowd_block_compact(m1, [&](int k) { return flag[lst[k]] == 0; }, [&](int k) { return lst[k]; }, lst, s_wave);
    __syncthreads();
    if (m2 >= 3) crowd_outlier(lst, m2, trans, cam, rel_thresh, 1.f, mn, flag, 3, s_red);
}

// The crop-stage survivors, row-ordered, and the reset of the flags for the full-frame stage.
__global__ __launch_bounds__(1024) void crowd_list_kernel(int N, int* __restrict__ flag, int* __restrict__ keep1,
                                                          int* __restrict__ list, int* __restrict__ count) {
    __shared__ int s_wave[17];
    for (int r = threadIdx.x; r < N; r += blockDim.x) keep1[r] = flag[r] == 0;
    __syncthreads();
    const int m = crowd_block_compact(N, [&](int r) { return keep1[r] != 0; }, [](int r) { return r; }, list, s_wave);
    for (int r = threadIdx.x; r < N; r += blockDim.x) flag[r] = 0;
    if (threadIdx.x == 0) count[0] = m;
}

// Full-frame projection of every row (pad info of padding_image_overlap: top, left, square size).
__global__ __launch_bounds__(256) void crowd_project_kernel(const float* __restrict__ joints, const float* __restrict__ cam_full,
                                                            int N, float top, float pad, float* __restrict__ trans,
                                                            float* __restrict__ pj) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N * CJ) return;
    const int row = i / CJ;
    float tr[3];
    crowd_trans(cam_full + (size_t)row * 3, tr);
    if (i % CJ == 0)
        for (int k = 0; k < 3; ++k) trans[(size_t)row * 3 + k] = tr[k];
    crowd_project(joints + (size_t)i * 3, tr, pad, top, 0.f, pj + (size_t)i * 2);
}

// Global conf-based suppression: every survivor pair (a < b in row order), grid-stride.
__global__ __launch_bounds__(256) void crowd_pairs_kernel(const float* __restrict__ pj, const float* __restrict__ cam_full,
                                                          const float* __restrict__ conf, const int* __restrict__ list,
                                                          const int* __restrict__ count, float thr, int* __restrict__ flag) {
    const long long m = count[0];
    for (long long p = (long long)blockIdx.x * blockDim.x + threadIdx.x; p < m * m; p += (long long)gridDim.x * blockDim.x) {
        const int a = (int)(p / m), b = (int)(p % m);
        if (a >= b) continue;
        const int ra = list[a], rb = list[b];
        const float d = crowd_pair_dist(pj, ra, rb, cam_full[(size_t)ra * 3] * 2.f, cam_full[(size_t)rb * 3] * 2.f);
        if (d < thr) atomicExch(&flag[conf[ra] < conf[rb] ? ra : rb], 1);
    }
}

// remove_outlier (scale_thresh 0.5) over the survivors of the global suppression; keep[row] for every row.
__global__ __launch_bounds__(1024) void crowd_outlier_kernel(int N, const float* __restrict__ trans, const float* __restrict__ cam_full,
                                                             float rel_thresh, const int* __restrict__ keep1, int* __restrict__ flag,
                                                             int* __restrict__ list, const int* __restrict__ count,
                                                             float* __restrict__ mean, int* __restrict__ keep) {
    __shared__ int s_wave[17];
    __shared__ float s_red[1024];
    const int m1 = count[0];
    const int m = crowd_block_compact(m1, [&](int k) { return flag[list[k]] == 0; }, [&](int k) { return list[k]; }, list, s_wave);
    __syncthreads();
    if (m >= 3) crowd_outlier(list, m, trans, cam_full, rel_thresh, 0.5f, mean, flag, 2, s_red);
    for (int r = threadIdx.x; r < N; r += blockDim.x) keep[r] = keep1[r] && flag[r] == 0;
}

}  // namespace romp

using namespace romp;

namespace {

bool crops_valid(const int32_t* crops_host, int K, int H, int W, int pad_length, const char* who) {
    for (int c = 0; c < K; ++c) {
        const int32_t* b = crops_host + 4 * c;                            // left, right, top, bottom in the padded frame
        if (!(b[0] >= 0 && b[0] < b[1] && b[1] <= W + 2 * pad_length && b[2] >= 0 && b[2] < b[3] && b[3] <= H)) {
            romp::set_error("%s: crop %d = [%d, %d, %d, %d] is not inside the %d x %d padded frame", who, c, b[0], b[1], b[2], b[3],
                            H, W + 2 * pad_length);
            return false;
        }
    }
    return true;
}

}  // namespace

extern "C" {

int romp_preprocess_crops(const unsigned char* bgr_u8, int H, int W, int pad_length, int K, const int32_t* crops_host,
                          float* out_rgb_f32, int out_size, float* pad_info_host, void* stream) {
    ROMP_REQUIRE(bgr_u8 && crops_host && out_rgb_f32 && H > 0 && W > 0 && pad_length >= 0 && K > 0 && out_size > 0,
                 "romp_preprocess_crops: bad arguments");
    if (!crops_valid(crops_host, K, H, W, pad_length, "romp_preprocess_crops")) return ROMP_EINVAL;
    const int total = out_size * out_size;
    for (int c0 = 0; c0 < K; c0 += CROWD_CHUNK) {
        const int n = K - c0 < CROWD_CHUNK ? K - c0 : CROWD_CHUNK;
        CropWindows t = {};
        for (int c = 0; c < n; ++c) {
            const int32_t* b = crops_host + 4 * (c0 + c);
            t.x0[c] = b[0] - pad_length; t.y0[c] = b[2]; t.w[c] = b[1] - b[0]; t.h[c] = b[3] - b[2];
            if (pad_info_host) {                                          // padding_image of the crop: top, bottom, left, right, h, w
                const int side = t.h[c] > t.w[c] ? t.h[c] : t.w[c];
                const int top = (side - t.h[c]) / 2, left = (side - t.w[c]) / 2;
                float* pi = pad_info_host + 6 * (c0 + c);
                pi[0] = (float)top; pi[1] = (float)(top + t.h[c]); pi[2] = (float)left; pi[3] = (float)(left + t.w[c]);
                pi[4] = (float)t.h[c]; pi[5] = (float)t.w[c];
            }
        }
        hipLaunchKernelGGL(crowd_preprocess_kernel, dim3((total + 255) / 256, n), dim3(256), 0, (hipStream_t)stream, bgr_u8, H, W, t, c0,
                           out_rgb_f32, out_size);
        ROMP_HIP_CHECK(hipGetLastError());
    }
    return ROMP_OK;
}

int romp_bev_crowd_merge(const float* joints, const float* cam, const float* center_confs, const int32_t* offsets, int N,
                         int capacity, int K, const int32_t* crops_host, int H, int W, int pad_length, double nms_thresh,
                         float relative_scale_thresh, float* cam_full, float* cam_trans, float* pj2d_org, int32_t* keep,
                         int32_t* workspace, void* stream) {
    ROMP_REQUIRE(joints && cam && center_confs && offsets && crops_host && cam_full && cam_trans && pj2d_org && keep && workspace &&
                 K > 0 && N >= 0 && H > 0 && W > 0 && pad_length >= 0, "romp_bev_crowd_merge: bad arguments");
    ROMP_REQUIRE(N <= capacity, "romp_bev_crowd_merge: %d rows but capacity %d", N, capacity);
    if (!crops_valid(crops_host, K, H, W, pad_length, "romp_bev_crowd_merge")) return ROMP_EINVAL;
    if (N == 0) return ROMP_OK;
    hipStream_t st = (hipStream_t)stream;
    int* flag = workspace;                                                // workspace: 4 * capacity + 4 int32
    int* keep1 = flag + capacity;
    int* list = keep1 + capacity;
    float* mean = (float*)(list + capacity);
    int* count = (int*)(mean + capacity);
    const double maxhw = (double)(H > W ? H : W);
    ROMP_HIP_CHECK(hipMemsetD32Async((hipDeviceptr_t)flag, 1, N, st));       // rows outside every crop's range are dropped
    for (int c0 = 0; c0 < K; c0 += CROWD_CHUNK) {
        const int n = K - c0 < CROWD_CHUNK ? K - c0 : CROWD_CHUNK;
        CropMerge t = {};
        for (int c = 0; c < n; ++c) {
            const int cid = c0 + c;
            const int32_t* b = crops_host + 4 * cid;
            const int cw = b[1] - b[0], ch = b[3] - b[2], side = cw > ch ? cw : ch;
            // drop_boundary_ratio = (this_right - next_left) / fh / 2, compared as float32 (main.py:214-228)
            const int32_t* next = crops_host + 4 * (cid + 1);
            const int32_t* prev = crops_host + 4 * (cid - 1);
            t.drop_hi[c] = cid != K - 1 ? (float)(1.0 - (double)(b[1] - next[0]) / H / 2) : INFINITY;
            t.drop_lo[c] = cid >= 2 ? (float)((double)(prev[1] - b[0]) / H / 2 - 1.0) : -INFINITY;
            t.nms_thr[c] = (float)(nms_thresh * side / 640);
            t.pad[c] = (float)side;
            t.scale[c] = (float)((double)side / maxhw);
            t.shift[c] = (float)(((double)(b[0] - pad_length) + (double)(b[1] - pad_length)) / 2 / ((double)W / 2) - 1);
        }
        hipLaunchKernelGGL(crowd_crop_kernel, dim3(n), dim3(256), 0, st, joints, cam, center_confs, (const int*)offsets, N, c0, t,
                           relative_scale_thresh, cam_full, cam_trans, pj2d_org, flag, list, mean);
        ROMP_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(crowd_list_kernel, dim3(1), dim3(1024), 0, st, N, flag, keep1, list, count);
    ROMP_HIP_CHECK(hipGetLastError());
    // padding_image_overlap's pad info [(w-h)//2, w-(w-h)//2, 0, w, h, w] (Python floor division)
    const int d = W - H, top = d >= 0 ? d / 2 : -((-d + 1) / 2);
    hipLaunchKernelGGL(crowd_project_kernel, dim3((N * CJ + 255) / 256), dim3(256), 0, st, joints, cam_full, N, (float)top,
                       (float)maxhw, cam_trans, pj2d_org);
    ROMP_HIP_CHECK(hipGetLastError());
    const long long pairs = (long long)N * N;
    const int grid = (int)(pairs / 256 + 1 < 2048 ? pairs / 256 + 1 : 2048);
    hipLaunchKernelGGL(crowd_pairs_kernel, dim3(grid), dim3(256), 0, st, pj2d_org, cam_full, center_confs, list, count,
                       (float)(nms_thresh * maxhw / 640), flag);
    ROMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(crowd_outlier_kernel, dim3(1), dim3(1024), 0, st, N, cam_trans, cam_full, relative_scale_thresh, keep1, flag,
                       list, count, mean, keep);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

}  // extern "C"
