// smpl_shared.h -- what the SMPL forward (smpl.hip) and its backward (smpl_grad.hip) share: the sizes, the kinematic-tree
// tables, the per-person pose prologue, the posedirs chunk loads of the skinning kernel and the context.
#pragma once
#include "common.h"

struct smpl_grad_scratch;                               // smpl_grad.hip: the backward's own buffers

namespace romp {

constexpr int NV = 6890, NJ = 24, NPF = 207, NJOUT = 71, NREG = 26, NPICK = 21;
constexpr int PB = 16;                                 // persons per workgroup in the skinning kernel
constexpr int NT = (NV + 63) / 64;                    // 108 vertex tiles
constexpr int MAXLV = NJ;

typedef float f2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ f2 pk_fma(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }   // v_pk_fma_f32

struct Parents { int p[NJ]; };
// joints ordered by depth in the kinematic tree: level l = order[start[l] .. start[l + 1])
struct Levels { int n; int start[MAXLV + 1]; int order[NJ]; };

// ---- kernel A: per-person pose prologue ---------------------------------------------------------
// pose_feat is written in the layout the skinning kernel stages: [person group][207][PB]
template <int NB>
__global__ __launch_bounds__(64) void smpl_pose_kernel(const float* __restrict__ betas,
                                                        const float* __restrict__ thetas,
                                                        const float* __restrict__ Jt, const float* __restrict__ Js,
                                                        const int* __restrict__ sched, float* __restrict__ pose_feat,
                                                        float* __restrict__ Amat, float* __restrict__ joints) {
    __shared__ float sR[NJ][9], sJ[NJ][3], sG[NJ][12];
    const int n = blockIdx.x, lane = threadIdx.x;
    if (lane < NJ) {
        const float* r = thetas + (size_t)n * 72 + lane * 3;
        const float rx0 = r[0], ry0 = r[1], rz0 = r[2];
        float jt[3], js[3][NB], bt[NB];                      // every load of the prologue in flight before the first use
#pragma unroll
        for (int l = 0; l < NB; ++l) bt[l] = betas[(size_t)n * NB + l];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            jt[k] = Jt[lane * 3 + k];
#pragma unroll
            for (int l = 0; l < NB; ++l) js[k][l] = Js[(lane * 3 + k) * NB + l];
        }
        const float ex = rx0 + 1e-8f, ey = ry0 + 1e-8f, ez = rz0 + 1e-8f;     // smpl.py:206
        const float angle = sqrtf(ex * ex + ey * ey + ez * ez);
        const float rx = rx0 / angle, ry = ry0 / angle, rz = rz0 / angle;
        float sn, cs;
        sincosf(angle, &sn, &cs);
        const float oc = 1.f - cs;
        // K = [[0,-rz,ry],[rz,0,-rx],[-ry,rx,0]];  R = I + sin K + (1-cos) K K   (smpl.py:217-221)
        const float kk00 = -(rz * rz) - ry * ry, kk11 = -(rz * rz) - rx * rx, kk22 = -(ry * ry) - rx * rx;
        const float kk01 = ry * rx, kk02 = rz * rx, kk12 = rz * ry;
        float R[9];
        R[0] = 1.f + oc * kk00;      R[1] = sn * -rz + oc * kk01; R[2] = sn * ry + oc * kk02;
        R[3] = sn * rz + oc * kk01;  R[4] = 1.f + oc * kk11;      R[5] = sn * -rx + oc * kk12;
        R[6] = sn * -ry + oc * kk02; R[7] = sn * rx + oc * kk12;  R[8] = 1.f + oc * kk22;
#pragma unroll
        for (int e = 0; e < 9; ++e) sR[lane][e] = R[e];
        if (lane >= 1) {
            float* pf = pose_feat + (size_t)(n / PB) * NPF * PB + (n % PB);
#pragma unroll
            for (int e = 0; e < 9; ++e) pf[((lane - 1) * 9 + e) * PB] = R[e] - ((e == 0 || e == 4 || e == 8) ? 1.f : 0.f);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float a = jt[k];
#pragma unroll
            for (int l = 0; l < NB; ++l) a = fmaf(bt[l], js[k][l], a);
            sJ[lane][k] = a;
        }
    }
    __syncthreads();
    // kinematic chain (smpl.py:269-275): G[i] = G[parent] * [R_i | J_i - J_parent], one tree level per step; five groups of
    // 12 lanes each own one joint of the level (one element of its 3x4 transform per lane)
    const int grp = lane / 12, el = lane % 12, rr = el / 4, cc = el % 4;
    if (lane < 12) sG[0][lane] = (cc < 3) ? sR[0][rr * 3 + cc] : sJ[0][rr];
    __syncthreads();
    const int n_lv = sched[0];
    for (int lv = 1; lv < n_lv; ++lv) {
        const int q1 = sched[1 + lv + 1];
        for (int q = sched[1 + lv] + grp; q < q1 && grp < 5; q += 5) {
            const int i = sched[1 + (MAXLV + 1) + q], p = sched[1 + (MAXLV + 1) + NJ + i];
            float v;
            if (cc < 3) {
                v = sG[p][rr * 4 + 0] * sR[i][0 * 3 + cc];
                v = fmaf(sG[p][rr * 4 + 1], sR[i][1 * 3 + cc], v);
                v = fmaf(sG[p][rr * 4 + 2], sR[i][2 * 3 + cc], v);
            } else {
                v = sG[p][rr * 4 + 0] * (sJ[i][0] - sJ[p][0]);
                v = fmaf(sG[p][rr * 4 + 1], sJ[i][1] - sJ[p][1], v);
                v = fmaf(sG[p][rr * 4 + 2], sJ[i][2] - sJ[p][2], v);
                v += sG[p][rr * 4 + 3];
            }
            sG[i][el] = v;
        }
        __syncthreads();
    }
    // posed joints + relative transforms A = G - pad(G [J;0])   (smpl.py:280-288)
    for (int idx = lane; idx < NJ * 12; idx += 64) {
        const int j = idx / 12, e = idx % 12, r = e / 4, c = e % 4;
        float v = sG[j][e];
        if (c == 3) {
            joints[((size_t)n * NJOUT + j) * 3 + r] = v;
            const float t = sG[j][r * 4 + 0] * sJ[j][0] + sG[j][r * 4 + 1] * sJ[j][1] + sG[j][r * 4 + 2] * sJ[j][2];
            v -= t;
        }
        Amat[(size_t)n * NJ * 12 + idx] = v;
    }
}

// ---- the pose-blend quarter of the skinning kernel: 4 waves on the SAME 64 vertices and PB persons, each wave a quarter
// of the 207 terms in register chunks of 13
constexpr int SKIN_WAVES = 4, KQ = (NPF + SKIN_WAVES - 1) / SKIN_WAVES;   // 52 terms per wave
constexpr int PPW = PB / SKIN_WAVES;                                      // persons finished per wave
constexpr int U_FLOATS = SKIN_WAVES * PB * 3 * 64;                        // blend partials, then the vertex tile
constexpr int KC = 13, NCH = KQ / KC;                                     // posedirs terms per register chunk, chunks per wave
static_assert(KQ == KC * NCH, "chunking of the pose-blend quarter");

__device__ __forceinline__ void pd_load(float (&d)[KC][3], const float* __restrict__ pdv, int kbase) {
#pragma unroll
    for (int i = 0; i < KC; ++i) {
        const size_t off = (size_t)min(kbase + i, NPF - 1) * (NV * 3);
        d[i][0] = pdv[off]; d[i][1] = pdv[off + 1]; d[i][2] = pdv[off + 2];
    }
}

__device__ __forceinline__ void pd_blend(f2 (&po)[PB / 2][3], const float (&d)[KC][3], const float (*s_pf)[PB], int kbase) {
#pragma unroll
    for (int i = 0; i < KC; ++i) {
        const int k = kbase + i;
        const bool in = k < NPF;                                  // the last quarter is one term short
        const float d0 = in ? d[i][0] : 0.f, d1 = in ? d[i][1] : 0.f, d2 = in ? d[i][2] : 0.f;
        const f2 dd0{d0, d0}, dd1{d1, d1}, dd2{d2, d2};
        const float* row = s_pf[min(k, NPF - 1)];
#pragma unroll
        for (int p4 = 0; p4 < PB; p4 += 4) {
            const float4 f = *reinterpret_cast<const float4*>(row + p4);
            const f2 fa{f.x, f.y}, fb{f.z, f.w};
            po[p4 / 2][0] = pk_fma(fa, dd0, po[p4 / 2][0]); po[p4 / 2][1] = pk_fma(fa, dd1, po[p4 / 2][1]); po[p4 / 2][2] = pk_fma(fa, dd2, po[p4 / 2][2]);
            po[p4 / 2 + 1][0] = pk_fma(fb, dd0, po[p4 / 2 + 1][0]); po[p4 / 2 + 1][1] = pk_fma(fb, dd1, po[p4 / 2 + 1][1]); po[p4 / 2 + 1][2] = pk_fma(fb, dd2, po[p4 / 2 + 1][2]);
        }
    }
}

}  // namespace romp

struct smpl_ctx {
    int nb = 10;
    int cap = 0;
    romp::Parents par;
    int* sched = nullptr;          // [n_levels, start[MAXLV + 1], order[NJ], parent[NJ]] for the pose kernel
    float* jpart = nullptr;        // (cap, NT, NREG, 3) per-tile joint partial sums
    float *vt = nullptr, *sd = nullptr, *pd = nullptr, *lbsw = nullptr, *reg = nullptr, *Jt = nullptr, *Js = nullptr;
    int* pick = nullptr;
    float *pose_feat = nullptr, *Amat = nullptr, *root = nullptr;
    smpl_grad_scratch* grad = nullptr;   // smpl_backward's grow-only scratch (never touched by the forward)
};

void smpl_grad_release(smpl_ctx* c);     // smpl_grad.hip: frees c->grad (smpl_ctx_destroy)
