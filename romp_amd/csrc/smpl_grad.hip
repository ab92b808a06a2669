// smpl_grad.hip -- backward of the SMPL layer (include/romp_hip_smpl_grad.h): the vector-Jacobian product of smpl_forward
// with respect to betas and thetas, for gradients arriving at the vertices and at the 71 joints.
//
// Like the forward it never materialises v_posed, the expanded weights or the per-vertex transforms; everything is
// recomputed from betas / thetas (nothing the forward left in the context is read):
//   kernel A  (the forward's smpl_pose_kernel, into the backward's own scratch)  pose features, A matrices, posed joints;
//   kernel J  (one workgroup per person)  the gradients that reach the 71 joints BEFORE the root alignment: with
//             root_align the sum of all vertex and joint gradients comes back through joints 45 / 46;
//   kernel B  (64 vertices x PB = 16 persons per workgroup, placed per XCD like the forward's skinning kernel so that the
//             posedirs tile comes from HBM once)  recomputes v_posed and T = W.A per vertex exactly as the forward does,
//             forms gV' (vertex gradient + regressed + picked joints), g_vp = T.R^T gV' and the outer products
//             [gV' x v_posed | gV'], and reduces the tile's 64 vertices to ONE partial row per person:
//               gA   (24 x 12)   sum_v W[v][j] [gV' x vp | gV']       packed-f32 FMAs out of LDS
//               gbeta (n_betas)  sum_v,k S[v][k][l] g_vp[k]           \  one f32 MFMA product per 16 output rows:
//               g_pf (207)       sum_v,k P[f][3v+k] g_vp[k]           /  rows = f (or l), columns = persons, K = 192
//             The tile's posedirs rows are contiguous 768-byte segments: they go from L2 straight into the MFMA's A
//             operand (no LDS), g_vp is the B operand, read from LDS once and kept in registers for all 13 row blocks.
//   kernel C  (one workgroup per person)  sums the 108 partial rows in tile order, walks the context's kinematic tree from
//             the leaves to the root, differentiates the forward's own Rodrigues formula (the 1e-8 included) and applies
//             the pre-regressed J_shapedirs; this per-person part runs in float64 (a few hundred operations).
// No float atomics; every reduction has a fixed order.
#include "smpl_shared.h"
#include "../../include/romp_hip_smpl_grad.h"

struct smpl_grad_scratch {
    int cap = 0;
    float *pose_feat = nullptr, *Amat = nullptr, *jtr = nullptr;   // kernel A's outputs (jtr: posed joints, row stride NJOUT)
    float* gj = nullptr;                                           // (cap, 71, 3) joint gradients before the root alignment
    float* part = nullptr;                                         // (cap, NT, 288 + n_betas + 207) per-tile partial rows
};

namespace romp {

constexpr int NGJ = NJOUT - NJ;                                    // joints 24..70: 21 picked, 26 regressed
constexpr int grad_row(int nb) { return NJ * 12 + nb + NPF; }

// ---- kernel J: joint gradients before the root alignment --------------------------------------------------------------
// joints_out = joints - root, verts_out = verts - root, root = (joints[45] + joints[46]) / 2:
// g_root = -(sum_v gV + sum_j gJ), half of it to each of joints 45 and 46.  NULL inputs stand for zeros.
// Joints 24..44 are vertex picks: their rows are combined per picked vertex for the gather in kernel B.
__global__ __launch_bounds__(256) void smpl_grad_joints_kernel(const float* __restrict__ gverts, const float* __restrict__ gjoints,
                                                                const int* __restrict__ pick, int root_align, float* __restrict__ gj) {
    __shared__ float s_red[3][256];
    const int n = blockIdx.x, tid = threadIdx.x;
    float a0 = 0.f, a1 = 0.f, a2 = 0.f;
    if (root_align) {
        if (gverts)
#pragma unroll 9
            for (int v = tid; v < NV; v += 256) {
                const float* g = gverts + ((size_t)n * NV + v) * 3;
                a0 += g[0]; a1 += g[1]; a2 += g[2];
            }
        if (gjoints && tid < NJOUT) {
            const float* g = gjoints + ((size_t)n * NJOUT + tid) * 3;
            a0 += g[0]; a1 += g[1]; a2 += g[2];
        }
    }
    s_red[0][tid] = a0; s_red[1][tid] = a1; s_red[2][tid] = a2;
    __syncthreads();
    for (int d = 128; d > 0; d >>= 1) {
        if (tid < d) {
            s_red[0][tid] += s_red[0][tid + d]; s_red[1][tid] += s_red[1][tid + d]; s_red[2][tid] += s_red[2][tid + d];
        }
        __syncthreads();
    }
    if (tid < NJOUT * 3) {
        float g = gjoints ? gjoints[(size_t)n * NJOUT * 3 + tid] : 0.f;
        if (root_align && (tid / 3 == 45 || tid / 3 == 46)) g -= 0.5f * s_red[tid % 3][0];
        // picks that name one vertex: the first of them carries the sum (added in index order), the tile kernel reads only that row
        const int i = tid / 3 - NJ;
        if (gjoints && i >= 0 && i < NPICK)
            for (int i2 = i + 1; i2 < NPICK; ++i2)
                if (pick[i2] == pick[i]) g += gjoints[((size_t)n * NJOUT + NJ + i2) * 3 + tid % 3];
        gj[(size_t)n * NJOUT * 3 + tid] = g;
    }
}

// ---- kernel B: per-vertex backward + the tile's partial row -----------------------------------------------------------
constexpr int GVS = 196, OS = 784, WS = NJ;                       // LDS strides: g_vp per person, outer products per person, weights per vertex
constexpr int G_FLOATS = PB * GVS, O_FLOATS = PB * OS, W_FLOATS = 64 * WS;
constexpr int A_FLOATS = 5 * 256 * 4;                              // the A matrices with the staging slack of the forward
constexpr int S_FLOATS = U_FLOATS + A_FLOATS;
static_assert(G_FLOATS + O_FLOATS + W_FLOATS <= S_FLOATS && GVS % 4 == 0 && OS % 4 == 0 && G_FLOATS % 4 == 0, "LDS aliasing of the reduction phase");
constexpr int NFB = (NPF + 15) / 16;                              // 13 blocks of 16 posedirs rows (+ one block for shapedirs)
typedef float f4 __attribute__((ext_vector_type(4)));

template <int NB>
__global__ __launch_bounds__(256, 2) void smpl_grad_tile_kernel(const float* __restrict__ betas, const float* __restrict__ pose_feat,
                                                              const float* __restrict__ Amat, const float* __restrict__ vt,
                                                              const float* __restrict__ sd, const float* __restrict__ pd,
                                                              const float* __restrict__ lbsw, const float* __restrict__ reg,
                                                              const int* __restrict__ pick, const float* __restrict__ gverts,
                                                              const float* __restrict__ gj, int N, int groups,
                                                              float* __restrict__ part) {
    constexpr int ROW = grad_row(NB);
    __shared__ __attribute__((aligned(16))) float s_m[S_FLOATS];  // pose features | A; blend partials | A; then g_vp, outer products, weights
    __shared__ float s_beta[PB][NB];
    __shared__ float s_gj[PB][NGJ * 3];                            // gradients of joints 24..70
    float* s_u = s_m;
    float* s_A = s_m + U_FLOATS;
    static_assert(NPF * PB <= U_FLOATS && 4 * 256 * 4 <= U_FLOATS, "LDS aliasing");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const int tile = (slot / groups) * 8 + xcd, grp = slot % groups;
    if (tile >= NT) return;
    const int p0 = grp * PB;
    const int np = min(PB, N - p0);
    const bool live = tile * 64 + lane < NV;
    const int v = min(tile * 64 + lane, NV - 1);                  // tail lanes recompute the last vertex; their gradient is zero
    const float* pdv = pd + (size_t)v * 3;
    const int k0 = wave * KQ;
    // ---- forward recomputation, as smpl_skin_kernel: staging, the pose-blend quarter of this wave
    float d[2][KC][3];
    pd_load(d[0], pdv, k0);
    constexpr int PF4 = NPF * PB / 4, A4 = PB * NJ * 12 / 4;
    static_assert(PF4 <= 4 * 256 && A4 <= 5 * 256 && PB * NB <= 256, "staging loops");
    const float4* src_pf = reinterpret_cast<const float4*>(pose_feat + (size_t)grp * NPF * PB);
    const float4* src_A = reinterpret_cast<const float4*>(Amat + (size_t)p0 * NJ * 12);
    float4 tpf[4], tA[5];
#pragma unroll
    for (int i = 0; i < 4; ++i) tpf[i] = src_pf[min(tid + 256 * i, PF4 - 1)];
#pragma unroll
    for (int i = 0; i < 5; ++i) tA[i] = src_A[min(tid + 256 * i, A4 - 1)];
    const float tb = (tid < PB * NB && tid / NB < np) ? betas[(size_t)p0 * NB + tid] : 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) reinterpret_cast<float4*>(s_u)[tid + 256 * i] = tpf[i];
#pragma unroll
    for (int i = 0; i < 5; ++i) reinterpret_cast<float4*>(s_A)[tid + 256 * i] = tA[i];
    if (tid < PB * NB) (&s_beta[0][0])[tid] = tb;
    for (int idx = tid; idx < PB * NGJ * 3; idx += 256) {         // rows past N: zeros, never read from memory
        const int p = idx / (NGJ * 3), e = idx % (NGJ * 3);
        (&s_gj[0][0])[idx] = p < np ? gj[((size_t)(p0 + p) * NJOUT + NJ) * 3 + e] : 0.f;
    }
    __syncthreads();
    const float(*s_pf)[PB] = reinterpret_cast<const float(*)[PB]>(s_u);   // [NPF][PB]
    f2 po[PB / 2][3];
#pragma unroll
    for (int p = 0; p < PB / 2; ++p) po[p][0] = po[p][1] = po[p][2] = f2{0.f, 0.f};
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c + 1 < NCH) pd_load(d[(c + 1) & 1], pdv, k0 + (c + 1) * KC);
        pd_blend(po, d[c & 1], s_pf, k0 + c * KC);
    }
    // per-vertex constants of the finishing phase: in flight across the exchange of the partials, as in the forward; the
    // regressor column, the picks that name this vertex and the vertex gradients of this wave's persons leave after the
    // first barrier: issued before it the compiler hoists them above the blend loop, whose 190 registers leave no room
    const float t0 = vt[v * 3 + 0], t1 = vt[v * 3 + 1], t2 = vt[v * 3 + 2];
    float sdv[3][NB];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int l = 0; l < NB; ++l) sdv[k][l] = sd[((size_t)v * 3 + k) * NB + l];
    f2 w[NJ];
#pragma unroll
    for (int j4 = 0; j4 < NJ; j4 += 4) {
        const float4 t = *reinterpret_cast<const float4*>(lbsw + (size_t)v * NJ + j4);
        w[j4] = f2{t.x, t.x}; w[j4 + 1] = f2{t.y, t.y}; w[j4 + 2] = f2{t.z, t.z}; w[j4 + 3] = f2{t.w, t.w};
    }
    __syncthreads();                                              // every wave is done with the pose features: s_u becomes the partials
    float(*s_po)[PB * 3][64] = reinterpret_cast<float(*)[PB * 3][64]>(s_u);
#pragma unroll
    for (int p = 0; p < PB / 2; ++p)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s_po[wave][(2 * p) * 3 + k][lane] = po[p][k].x;
            s_po[wave][(2 * p + 1) * 3 + k][lane] = po[p][k].y;
        }
    float regv[NREG];
#pragma unroll
    for (int r = 0; r < NREG; ++r) regv[r] = reg[(size_t)r * NV + v];
    int ps = -1;                                                  // gather form of the vertex picks: the FIRST pick that names this vertex
#pragma unroll
    for (int i = NPICK - 1; i >= 0; --i) ps = pick[i] == v ? i : ps;
    float gvr[PPW][3];
#pragma unroll
    for (int pp = 0; pp < PPW; ++pp) {
        const int p = wave * PPW + pp;
        const bool ok = live && p < np && gverts != nullptr;      // no gradient row past N is ever read
        const float* g = gverts + ((size_t)(p0 + min(p, np - 1)) * NV + v) * 3;
        gvr[pp][0] = ok ? g[0] : 0.f; gvr[pp][1] = ok ? g[1] : 0.f; gvr[pp][2] = ok ? g[2] : 0.f;
    }
    __syncthreads();
    // ---- this wave's persons: v_posed and T as in the forward, then gV', g_vp
    float vpq[PPW][3], gq[PPW][3], gvp[PPW][3];
#pragma unroll
    for (int pp = 0; pp < PPW; ++pp) {
        const int p = wave * PPW + pp;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f;
#pragma unroll
        for (int l = 0; l < NB; ++l) {
            const float bb = s_beta[p][l];
            a0 = fmaf(bb, sdv[0][l], a0); a1 = fmaf(bb, sdv[1][l], a1); a2 = fmaf(bb, sdv[2][l], a2);
        }
        float q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)
            q[k] = (s_po[0][p * 3 + k][lane] + s_po[1][p * 3 + k][lane]) + (s_po[2][p * 3 + k][lane] + s_po[3][p * 3 + k][lane]);
        vpq[pp][0] = q[0] + (t0 + a0); vpq[pp][1] = q[1] + (t1 + a1); vpq[pp][2] = q[2] + (t2 + a2);
        f2 T[6];
#pragma unroll
        for (int e = 0; e < 6; ++e) T[e] = f2{0.f, 0.f};
        const float* Ap = s_A + p * NJ * 12;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {              // T = W @ A
            const float4 a0v = *reinterpret_cast<const float4*>(Ap + j * 12);
            const float4 a1v = *reinterpret_cast<const float4*>(Ap + j * 12 + 4);
            const float4 a2v = *reinterpret_cast<const float4*>(Ap + j * 12 + 8);
            T[0] = pk_fma(w[j], f2{a0v.x, a0v.y}, T[0]); T[1] = pk_fma(w[j], f2{a0v.z, a0v.w}, T[1]);
            T[2] = pk_fma(w[j], f2{a1v.x, a1v.y}, T[2]); T[3] = pk_fma(w[j], f2{a1v.z, a1v.w}, T[3]);
            T[4] = pk_fma(w[j], f2{a2v.x, a2v.y}, T[4]); T[5] = pk_fma(w[j], f2{a2v.z, a2v.w}, T[5]);
            // a compiler fence every 8 joints (and per person below): without them the LDS reads of all four persons are
            // issued ahead of the arithmetic and the kernel spills (measured at compile time: 120 spilled registers)
            if (j % 8 == 7) asm volatile("" ::: "memory");
        }
        // gV' = gV + sum_r reg[r][v] gJ[45 + r] + sum_{pick_i = v} gJ[24 + i]
        float gx = gvr[pp][0], gy = gvr[pp][1], gz = gvr[pp][2];
        const float* gjp = s_gj[p];
#pragma unroll
        for (int r = 0; r < NREG; ++r) {
            gx = fmaf(regv[r], gjp[(NPICK + r) * 3 + 0], gx); gy = fmaf(regv[r], gjp[(NPICK + r) * 3 + 1], gy);
            gz = fmaf(regv[r], gjp[(NPICK + r) * 3 + 2], gz);
        }
        {                                                         // one combined row per picked vertex (kernel J): no control flow here
            const float* gp = gjp + max(ps, 0) * 3;
            const float p0v = gp[0], p1v = gp[1], p2v = gp[2];
            gx += ps >= 0 ? p0v : 0.f; gy += ps >= 0 ? p1v : 0.f; gz += ps >= 0 ? p2v : 0.f;
        }
        const bool ok = live && p < np;                           // idle tail lanes and phantom persons add zero to every partial
        gx = ok ? gx : 0.f; gy = ok ? gy : 0.f; gz = ok ? gz : 0.f;
        gq[pp][0] = gx; gq[pp][1] = gy; gq[pp][2] = gz;
        gvp[pp][0] = fmaf(T[0].x, gx, fmaf(T[2].x, gy, T[4].x * gz));     // g_vp = T.R^T gV'
        gvp[pp][1] = fmaf(T[0].y, gx, fmaf(T[2].y, gy, T[4].y * gz));
        gvp[pp][2] = fmaf(T[1].x, gx, fmaf(T[3].x, gy, T[5].x * gz));
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            gvp[pp][k] = ok ? gvp[pp][k] : 0.f;
            vpq[pp][k] = ok ? vpq[pp][k] : 0.f;
        }
        asm volatile("" ::: "memory");
    }
    __syncthreads();                                              // partials and A are consumed: the reduction operands take their place
    float* s_g = s_m;                                             // [PB][GVS]   g_vp, 192 per person
    float* s_o = s_m + G_FLOATS;                                  // [PB][OS]    [gV' x vp | gV'], 12 per vertex
    float* s_w = s_o + O_FLOATS;                                  // [64][WS]    skinning weights of the tile (zero rows for idle lanes)
#pragma unroll
    for (int pp = 0; pp < PPW; ++pp) {
        const int p = wave * PPW + pp;
#pragma unroll
        for (int k = 0; k < 3; ++k) s_g[p * GVS + 3 * lane + k] = gvp[pp][k];
        float4* o = reinterpret_cast<float4*>(s_o + p * OS + lane * 12);
#pragma unroll
        for (int r = 0; r < 3; ++r)
            o[r] = float4{gq[pp][r] * vpq[pp][0], gq[pp][r] * vpq[pp][1], gq[pp][r] * vpq[pp][2], gq[pp][r]};
    }
    if (wave == 0) {
#pragma unroll
        for (int j4 = 0; j4 < NJ; j4 += 4)
            *reinterpret_cast<float4*>(s_w + lane * WS + j4) =
                live ? float4{w[j4].x, w[j4 + 1].x, w[j4 + 2].x, w[j4 + 3].x} : float4{0.f, 0.f, 0.f, 0.f};
    }
    __syncthreads();
    // ---- g_pf and gbeta: out[row][person] = sum_{i<192} M[row][i] g_vp[person][i] on the f32 MFMA (16 rows x 16 persons x 4).
    // Lane (m = lane % 16, kq = lane / 16) holds four consecutive i = 16 s + 4 kq + t of both operands, MFMA t of step s
    // uses element t: both operands are 16-byte reads, and any order of the reduction index is as good as another.
    {
        const int m = lane & 15, kq = lane >> 4;
        f4 bq[12];
#pragma unroll
        for (int s = 0; s < 12; ++s) bq[s] = *reinterpret_cast<const f4*>(s_g + m * GVS + 16 * s + 4 * kq);
#pragma unroll 1
        for (int fb = wave; fb < NFB + 1; fb += SKIN_WAVES) {
            f4 a[12];
            if (fb < NFB && tile < NT - 1) {                      // whole 768-byte row segments: one address, constant offsets
                const float* rowp = pd + (size_t)min(fb * 16 + m, NPF - 1) * (NV * 3) + tile * 192 + 4 * kq;
#pragma unroll
                for (int s = 0; s < 12; ++s) {                    // rows are 82 680 bytes long: 8-byte alignment only
                    const float2 lo = *reinterpret_cast<const float2*>(rowp + 16 * s), hi = *reinterpret_cast<const float2*>(rowp + 16 * s + 2);
                    a[s] = f4{lo.x, lo.y, hi.x, hi.y};
                }
            } else if (fb < NFB) {                                // the last tile ends at the row's end: zeros past it
                const float* row = pd + (size_t)min(fb * 16 + m, NPF - 1) * (NV * 3);
#pragma unroll
                for (int s = 0; s < 12; ++s)
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int c = tile * 192 + 16 * s + 4 * kq + t;
                        a[s][t] = c < NV * 3 ? row[min(c, NV * 3 - 1)] : 0.f;
                    }
            } else {                                              // shapedirs: rows = the betas, element (l, i) = S[3 v0 + i][l]
#pragma unroll
                for (int s = 0; s < 12; ++s)
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int c = tile * 192 + 16 * s + 4 * kq + t;
                        a[s][t] = (m < NB && c < NV * 3) ? sd[(size_t)min(c, NV * 3 - 1) * NB + min(m, NB - 1)] : 0.f;
                    }
            }
            f4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};   // two chains: the dependent latency exceeds the issue interval
#pragma unroll
            for (int s = 0; s < 12; s += 2)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s][t], bq[s][t], acc0, 0, 0, 0);
                    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s + 1][t], bq[s + 1][t], acc1, 0, 0, 0);
                }
            const f4 acc = acc0 + acc1;
            if (m < np) {                                         // result column = person m, rows 4 kq .. 4 kq + 3 of the block
                float* pr = part + ((size_t)(p0 + m) * NT + tile) * ROW;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = 4 * kq + i;
                    if (fb < NFB) {
                        if (fb * 16 + r < NPF) pr[NJ * 12 + NB + fb * 16 + r] = acc[i];
                    } else if (r < NB) {
                        pr[NJ * 12 + r] = acc[i];
                    }
                }
            }
        }
    }
    // ---- gA[j] = sum_v W[v][j] [gV' x vp | gV']: thread = (person, 3 joints, half of the 12 elements)
    {
        const int p = tid >> 4, sub = tid & 15, jb = sub >> 1, eh = sub & 1;
        const float* so = s_o + p * OS + eh * 6;
        const float* sw = s_w + jb * 3;
        f2 acc[3][3];
#pragma unroll
        for (int jj = 0; jj < 3; ++jj) acc[jj][0] = acc[jj][1] = acc[jj][2] = f2{0.f, 0.f};
#pragma unroll 4
        for (int vv = 0; vv < 64; ++vv) {
            const f2 o0 = *reinterpret_cast<const f2*>(so + vv * 12), o1 = *reinterpret_cast<const f2*>(so + vv * 12 + 2),
                     o2 = *reinterpret_cast<const f2*>(so + vv * 12 + 4);
#pragma unroll
            for (int jj = 0; jj < 3; ++jj) {
                const float ww = sw[vv * WS + jj];
                const f2 w2{ww, ww};
                acc[jj][0] = pk_fma(w2, o0, acc[jj][0]); acc[jj][1] = pk_fma(w2, o1, acc[jj][1]); acc[jj][2] = pk_fma(w2, o2, acc[jj][2]);
            }
        }
        if (p < np) {
            float* pr = part + ((size_t)(p0 + p) * NT + tile) * ROW;
#pragma unroll
            for (int jj = 0; jj < 3; ++jj)
#pragma unroll
                for (int e2 = 0; e2 < 3; ++e2)
                {                                                 // (rows have an odd length: no 8-byte stores)
                    pr[(jb * 3 + jj) * 12 + eh * 6 + e2 * 2] = acc[jj][e2].x;
                    pr[(jb * 3 + jj) * 12 + eh * 6 + e2 * 2 + 1] = acc[jj][e2].y;
                }
        }
    }
}

// ---- kernel C: per-person epilogue ------------------------------------------------------------------------------------
// Sums the tile partials in tile order, then the chain rule through A = [G.R | G.t - G.R J], the kinematic tree
// G_j = G_parent [R_j | J_j - J_parent] (children before parents: parents[j] < j), Rodrigues and J = Jt + Js.beta.
constexpr int PERSON_THREADS = 512;
template <int NB>
__global__ __launch_bounds__(PERSON_THREADS) void smpl_grad_person_kernel(const float* __restrict__ betas, const float* __restrict__ thetas,
                                                                const float* __restrict__ Jt, const float* __restrict__ Js,
                                                                const int* __restrict__ sched, const float* __restrict__ Amat,
                                                                const float* __restrict__ gj,
                                                                const float* __restrict__ part, float* __restrict__ gbetas,
                                                                float* __restrict__ gthetas) {
    constexpr int ROW = grad_row(NB);
    static_assert(ROW <= PERSON_THREADS && NT % 27 == 0, "one partial-row element per thread");
    __shared__ double s_row[ROW];
    __shared__ double s_R[NJ][9], s_J[NJ][3], s_GR[NJ][9], s_gG[NJ][12], s_grel[NJ][3], s_gJ[NJ][3];
    __shared__ int s_par[NJ];
    const int n = blockIdx.x, tid = threadIdx.x;
    const int* par = sched + 1 + (MAXLV + 1) + NJ;
    if (tid < NJ) s_par[tid] = par[tid];
    if (tid < ROW) {                                              // 27 loads in flight at a time, added in tile order
        const float* src = part + (size_t)n * NT * ROW + tid;
        double acc = 0.0;
#pragma unroll 27
        for (int t = 0; t < NT; ++t) acc += (double)src[(size_t)t * ROW];
        s_row[tid] = acc;
    }
    double rv[3] = {0, 0, 0}, ev[3] = {0, 0, 0}, angle = 1, sn = 0, cs = 1, K[9] = {0}, K2[9] = {0};
    if (tid < NJ) {
        const int j = tid;
        for (int k = 0; k < 3; ++k) {
            rv[k] = (double)thetas[(size_t)n * 72 + j * 3 + k];
            ev[k] = rv[k] + 1e-8;
        }
        angle = sqrt(ev[0] * ev[0] + ev[1] * ev[1] + ev[2] * ev[2]);
        const double dx = rv[0] / angle, dy = rv[1] / angle, dz = rv[2] / angle;
        sincos(angle, &sn, &cs);
        K[0] = 0; K[1] = -dz; K[2] = dy; K[3] = dz; K[4] = 0; K[5] = -dx; K[6] = -dy; K[7] = dx; K[8] = 0;
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) K2[r * 3 + c] = K[r * 3] * K[c] + K[r * 3 + 1] * K[3 + c] + K[r * 3 + 2] * K[6 + c];
        for (int e = 0; e < 9; ++e) s_R[j][e] = ((e == 0 || e == 4 || e == 8) ? 1.0 : 0.0) + sn * K[e] + (1.0 - cs) * K2[e];
        for (int k = 0; k < 3; ++k) {
            double a = (double)Jt[j * 3 + k];
            for (int l = 0; l < NB; ++l) a += (double)betas[(size_t)n * NB + l] * (double)Js[(j * 3 + k) * NB + l];
            s_J[j][k] = a;
        }
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) s_GR[j][r * 3 + c] = (double)Amat[(size_t)n * NJ * 12 + j * 12 + r * 4 + c];
    }
    __syncthreads();
    if (tid < NJ) {
        // A = [G.R | G.t - G.R J]:  gG.R = gA.R - gA.t J^T,  gG.t = gA.t + gJ_j,  gJrest_j = -G.R^T gA.t
        const int j = tid;
        for (int r = 0; r < 3; ++r) {
            const double gt = s_row[j * 12 + r * 4 + 3];
            for (int c = 0; c < 3; ++c) s_gG[j][r * 4 + c] = s_row[j * 12 + r * 4 + c] - gt * s_J[j][c];
            s_gG[j][r * 4 + 3] = gt + (double)gj[((size_t)n * NJOUT + j) * 3 + r];
        }
        for (int c = 0; c < 3; ++c)
            s_gJ[j][c] = -(s_GR[j][c] * s_row[j * 12 + 3] + s_GR[j][3 + c] * s_row[j * 12 + 7] + s_GR[j][6 + c] * s_row[j * 12 + 11]);
    }
    __syncthreads();
    // the tree, children before parents: gG_p.R += gG_j.R R_j^T + gG_j.t rel_j^T,  gG_p.t += gG_j.t; twelve lanes, one
    // element of the parent's 3x4 each; siblings are added in descending order
    for (int j = NJ - 1; j >= 1; --j) {
        const int p = s_par[j];
        if (tid < 12) {
            const int r = tid / 4, c = tid % 4;
            double a;
            if (c < 3)
                a = s_gG[j][r * 4] * s_R[j][c * 3] + s_gG[j][r * 4 + 1] * s_R[j][c * 3 + 1] + s_gG[j][r * 4 + 2] * s_R[j][c * 3 + 2] +
                    s_gG[j][r * 4 + 3] * (s_J[j][c] - s_J[p][c]);
            else
                a = s_gG[j][r * 4 + 3];
            s_gG[p][tid] += a;
        }
        __syncthreads();
    }
    if (tid < NJ) {
        const int j = tid, p = s_par[j];
        double gR[9], grel[3];
        for (int a = 0; a < 3; ++a) {
            for (int c = 0; c < 3; ++c)
                gR[a * 3 + c] = j ? s_GR[p][a] * s_gG[j][c] + s_GR[p][3 + a] * s_gG[j][4 + c] + s_GR[p][6 + a] * s_gG[j][8 + c]
                                  : s_gG[j][a * 4 + c];
            grel[a] = j ? s_GR[p][a] * s_gG[j][3] + s_GR[p][3 + a] * s_gG[j][7] + s_GR[p][6 + a] * s_gG[j][11] : s_gG[j][a * 4 + 3];
            s_grel[j][a] = grel[a];
        }
        if (j >= 1)
            for (int e = 0; e < 9; ++e) gR[e] += s_row[NJ * 12 + NB + (j - 1) * 9 + e];      // pose_feat = R - I
        // R = I + sin K(d) + (1 - cos) K(d)^2,  d = rv / angle,  angle = |rv + 1e-8|
        double gs = 0, goc = 0;
        for (int e = 0; e < 9; ++e) { gs += gR[e] * K[e]; goc += gR[e] * K2[e]; }
        double gang = cs * gs + sn * goc;
        double gK[9];
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) {
                double t = 0;                                         // (G K^T + K^T G)[r][c]
                for (int k = 0; k < 3; ++k) t += gR[r * 3 + k] * K[c * 3 + k] + K[k * 3 + r] * gR[k * 3 + c];
                gK[r * 3 + c] = sn * gR[r * 3 + c] + (1.0 - cs) * t;
            }
        const double gd[3] = {gK[7] - gK[5], gK[2] - gK[6], gK[3] - gK[1]};
        gang -= (gd[0] * rv[0] + gd[1] * rv[1] + gd[2] * rv[2]) / (angle * angle);
        if (gthetas)
            for (int k = 0; k < 3; ++k) gthetas[(size_t)n * 72 + j * 3 + k] = (float)(gd[k] / angle + gang * ev[k] / angle);
    }
    __syncthreads();
    if (tid < NJ) {
        // rel_j = J_j - J_parent: gJrest_j += g_rel_j, and minus the g_rel of every child (gather form, ascending)
        const int j = tid;
        double a[3] = {s_gJ[j][0] + s_grel[j][0], s_gJ[j][1] + s_grel[j][1], s_gJ[j][2] + s_grel[j][2]};
        for (int c = j + 1; c < NJ; ++c)
            if (s_par[c] == j) { a[0] -= s_grel[c][0]; a[1] -= s_grel[c][1]; a[2] -= s_grel[c][2]; }
        s_gJ[j][0] = a[0]; s_gJ[j][1] = a[1]; s_gJ[j][2] = a[2];   // (only this thread reads or writes row j)
    }
    __syncthreads();
    if (tid < NB && gbetas) {
        double a = s_row[NJ * 12 + tid];
        for (int e = 0; e < NJ * 3; ++e) a += (double)Js[e * NB + tid] * (&s_gJ[0][0])[e];
        gbetas[(size_t)n * NB + tid] = (float)a;
    }
}

}  // namespace romp

using namespace romp;

static void grad_free(smpl_grad_scratch* g) {
    float* ptrs[] = {g->pose_feat, g->Amat, g->jtr, g->gj, g->part};
    for (float* p : ptrs)
        if (p) hipFree(p);
    g->pose_feat = g->Amat = g->jtr = g->gj = g->part = nullptr;
    g->cap = 0;
}

void smpl_grad_release(smpl_ctx* c) {
    if (!c || !c->grad) return;
    grad_free(c->grad);
    delete c->grad;
    c->grad = nullptr;
}

// grow-only; `st`: the stream of the call that will use the buffers (the clears are ordered on it)
static int grad_reserve(smpl_ctx* c, int N, hipStream_t st) {
    if (!c->grad) c->grad = new smpl_grad_scratch();
    smpl_grad_scratch* g = c->grad;
    if (N <= g->cap) return ROMP_OK;
    grad_free(g);
    const size_t cap = (size_t)(N + PB - 1) / PB * PB;            // whole person groups, as the forward's staging buffers
    ROMP_HIP_CHECK(hipMalloc((void**)&g->pose_feat, cap * NPF * 4));
    ROMP_HIP_CHECK(hipMalloc((void**)&g->Amat, cap * NJ * 12 * 4));
    ROMP_HIP_CHECK(hipMalloc((void**)&g->jtr, cap * NJOUT * 3 * 4));
    ROMP_HIP_CHECK(hipMalloc((void**)&g->gj, cap * NJOUT * 3 * 4));
    ROMP_HIP_CHECK(hipMalloc((void**)&g->part, cap * NT * (size_t)grad_row(c->nb) * 4));
    ROMP_HIP_CHECK(hipMemsetAsync(g->pose_feat, 0, cap * NPF * 4, st));   // rows of a partial last group stay finite
    ROMP_HIP_CHECK(hipMemsetAsync(g->Amat, 0, cap * NJ * 12 * 4, st));
    g->cap = (int)cap;
    return ROMP_OK;
}

extern "C" int smpl_backward(smpl_ctx* c, const float* betas, int n_betas, const float* thetas, int N, int root_align,
                             const float* grad_verts, const float* grad_joints, float* grad_betas, float* grad_thetas,
                             void* stream) {
    ROMP_REQUIRE(c && betas && thetas && N >= 0, "smpl_backward: bad arguments");
    ROMP_REQUIRE(n_betas == c->nb, "smpl_backward: n_betas %d but context was built with %d", n_betas, c->nb);
    if (N == 0 || (!grad_betas && !grad_thetas)) return ROMP_OK;
    hipStream_t st = (hipStream_t)stream;
    int rc = grad_reserve(c, N, st);
    if (rc) return rc;
    smpl_grad_scratch* g = c->grad;
    if (c->nb == 10)
        hipLaunchKernelGGL(smpl_pose_kernel<10>, dim3(N), dim3(64), 0, st, betas, thetas, c->Jt, c->Js, c->sched, g->pose_feat, g->Amat, g->jtr);
    else
        hipLaunchKernelGGL(smpl_pose_kernel<11>, dim3(N), dim3(64), 0, st, betas, thetas, c->Jt, c->Js, c->sched, g->pose_feat, g->Amat, g->jtr);
    ROMP_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(smpl_grad_joints_kernel, dim3(N), dim3(256), 0, st, grad_verts, grad_joints, c->pick, root_align, g->gj);
    ROMP_HIP_CHECK(hipGetLastError());
    const int groups = (N + PB - 1) / PB;
    const dim3 grid(8 * ((NT + 7) / 8) * groups);
    if (c->nb == 10)
        hipLaunchKernelGGL(smpl_grad_tile_kernel<10>, grid, dim3(256), 0, st, betas, g->pose_feat, g->Amat, c->vt, c->sd, c->pd,
                           c->lbsw, c->reg, c->pick, grad_verts, g->gj, N, groups, g->part);
    else
        hipLaunchKernelGGL(smpl_grad_tile_kernel<11>, grid, dim3(256), 0, st, betas, g->pose_feat, g->Amat, c->vt, c->sd, c->pd,
                           c->lbsw, c->reg, c->pick, grad_verts, g->gj, N, groups, g->part);
    ROMP_HIP_CHECK(hipGetLastError());
    if (c->nb == 10)
        hipLaunchKernelGGL(smpl_grad_person_kernel<10>, dim3(N), dim3(PERSON_THREADS), 0, st, betas, thetas, c->Jt, c->Js, c->sched, g->Amat,
                           g->gj, g->part, grad_betas, grad_thetas);
    else
        hipLaunchKernelGGL(smpl_grad_person_kernel<11>, dim3(N), dim3(PERSON_THREADS), 0, st, betas, thetas, c->Jt, c->Js, c->sched, g->Amat,
                           g->gj, g->part, grad_betas, grad_thetas);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}
