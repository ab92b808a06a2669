// render.hip -- Sim3DR mesh renderer on the device (the only native component next to
// the hot path; `--render_mesh` pays ~10x the network time for it on the host in the reference).
//
// Reference: simple_romp/vis_human/sim3drender/lib/rasterize_kernel.cpp  _get_normal :171-229,
// get_point_weight :56-85, _rasterize :233-300; simple_romp/vis_human/sim3drender/renderer.py
// Sim3DR.render :64-118 (lighting), __call__ :120-133.
//
// The reference is sequential (triangles in index order, strict `>` z-test, colour written on every
// accepted fragment).  With alpha == 1 (the only value its Python passes) the final colour of a pixel is
// the colour of the fragment with the greatest depth, ties going to the LOWEST triangle index, where -0.0
// and +0.0 are EQUAL depths as they are for the reference's `>` (and a NaN depth, or one not above -1e8, is
// no fragment) -- an order-free statement, so the device runs two passes: (1) one thread per triangle scans
// its bounding box and atomicMax-es a 64-bit key {orderable depth, ~triangle} per pixel, the depth's zero
// taken as +0.0 in the key only; (2) one thread per pixel recomputes the winner's barycentric weights (and,
// for the maps, its values: a -0.0 stays a -0.0 there) and writes the truncated uint8 colour.  Every float
// expression keeps the reference's operation order with contraction off, so the image is BIT-IDENTICAL to
// the C++ one.
// Vertex normals: the reference accumulates face normals onto vertices in triangle order; here one thread
// per vertex walks its (triangle, corner) incidence list in ascending order -- the same additions in the
// same order.  Lighting: one workgroup per mesh (min / max reductions of norm_vertices in LDS).
//
// Batches (Sim3DR.__call__, renderer.py:120-133): N meshes of one topology are painted one after the other,
// each with a fresh z-buffer.  With alpha == 1 the pixel takes the colour of the HIGHEST mesh index that
// covers it, and inside that mesh the rule above -- so the key grows to {mesh in the top m bits, orderable
// depth, ~triangle in the low 32-m bits}, m = ceil(log2 N), and one launch of each kernel paints all N
// meshes (N = 1, m = 0 is the single-mesh key).  The kernels below take the mesh as a grid dimension.
//
// View transform (vis_human/vis_utils.py:26-51, rotate_view_weak_perspective): Rx then Ry as two rounded
// steps, bbox centre 0.5*(min+max), scale 1/(expand_ratio*max|xy/(w/2,h/2)|); three launches, no host sync.
#include "common.h"
#include "../../include/romp_hip_views.h"
#include "../../include/romp_hip_maps.h"
#include "../../include/romp_hip_canvases.h"

#pragma clang fp contract(off)

namespace romp {

__device__ __forceinline__ void vertex_normal(const float* __restrict__ v, const int32_t* __restrict__ tri,
                                              const int32_t* __restrict__ adj_off, const int32_t* __restrict__ adj_ent, int i,
                                              float* __restrict__ out) {
    float nx = 0.f, ny = 0.f, nz = 0.f;
    for (int e = adj_off[i]; e < adj_off[i + 1]; ++e) {
        const int t = adj_ent[e] / 3;
        const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
        const float v1x = v[3 * b] - v[3 * a], v1y = v[3 * b + 1] - v[3 * a + 1], v1z = v[3 * b + 2] - v[3 * a + 2];
        const float v2x = v[3 * c] - v[3 * a], v2y = v[3 * c + 1] - v[3 * a + 1], v2z = v[3 * c + 2] - v[3 * a + 2];
        nx += v1y * v2z - v1z * v2y;
        ny += v1z * v2x - v1x * v2z;
        nz += v1x * v2y - v1y * v2x;
    }
    float det = sqrtf(nx * nx + ny * ny + nz * nz);
    if (det <= 0.f) det = 1e-6f;
    out[3 * i] = nx / det; out[3 * i + 1] = ny / det; out[3 * i + 2] = nz / det;
}

// grid.y walks the meshes (v / out: n x nver x 3)
__global__ void sim3dr_normal_kernel(const float* __restrict__ v, const int32_t* __restrict__ tri,
                                     const int32_t* __restrict__ adj_off, const int32_t* __restrict__ adj_ent, int nver, int n,
                                     float* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nver) return;
    for (int mesh = blockIdx.y; mesh < n; mesh += gridDim.y)
        vertex_normal(v + (size_t)mesh * nver * 3, tri, adj_off, adj_ent, i, out + (size_t)mesh * nver * 3);
}

struct LightCfg {
    float ambient[3];          // intensity_ambient * color, already rounded to float32 as numpy does (renderer.py:83)
    float i_dir, i_spec;       // 0: term switched off
    float color_dir[3], light_pos[3], view_pos[3];
    int spec_exp;              // specular_exp >= 1 (renderer.py:110); 1: the reference default
};

__device__ __forceinline__ float clip01(float x) { return fminf(fmaxf(x, 0.f), 1.f); }

// renderer.py:19-24 (norm_vertices) + :77-110.  One workgroup per mesh (v / nrm / light: n x nver x 3);
// ambient: n x 3 per-mesh ambient terms (device), or null for cfg.ambient.  texture: n x nver x 3 per-vertex colours, or
// null; with it the output is texture * light (renderer.py:124: one rounded multiply of the clipped light), without it
// the clipped light itself.  cfg.spec_exp = e: each component of v2v * reflection is raised to e before the three are
// summed (renderer.py:110).  e = 1 multiplies nothing; e >= 2 is t * t * ... * t, e - 1 rounded multiplies from left to
// right: numpy's square for e = 2, within rounding of its powf for e > 2 (not bit for bit).
// rows: mesh m takes its ambient term and texture from row rows[m] (romp_sim3dr_render_canvases), or from row m for null.
__global__ __launch_bounds__(1024) void sim3dr_light_kernel(const float* __restrict__ v, const float* __restrict__ nrm, int nver,
                                                             LightCfg cfg, const float* __restrict__ ambient,
                                                             const float* __restrict__ texture, const int32_t* __restrict__ rows,
                                                             float* __restrict__ light) {
    __shared__ float red[3][1024];
    __shared__ float s_min[3], s_max1, s_max3[3];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * nver * 3;
    v += base; nrm += base; light += base;
    const size_t row = rows ? (size_t)rows[blockIdx.x] : (size_t)blockIdx.x;
    if (texture) texture += row * nver * 3;
    const float amb[3] = {ambient ? ambient[3 * row] : cfg.ambient[0], ambient ? ambient[3 * row + 1] : cfg.ambient[1],
                          ambient ? ambient[3 * row + 2] : cfg.ambient[2]};
    float m[3] = {3.4e38f, 3.4e38f, 3.4e38f};
    for (int i = tid; i < nver; i += 1024)
        for (int k = 0; k < 3; ++k) m[k] = fminf(m[k], v[3 * i + k]);
    for (int k = 0; k < 3; ++k) red[k][tid] = m[k];
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) for (int k = 0; k < 3; ++k) red[k][tid] = fminf(red[k][tid], red[k][tid + s]);
        __syncthreads();
    }
    if (tid < 3) s_min[tid] = red[tid][0];
    __syncthreads();
    float mx = -3.4e38f;                                          // vertices.max() after the shift
    for (int i = tid; i < nver; i += 1024)
        for (int k = 0; k < 3; ++k) mx = fmaxf(mx, v[3 * i + k] - s_min[k]);
    red[0][tid] = mx;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) red[0][tid] = fmaxf(red[0][tid], red[0][tid + s]);
        __syncthreads();
    }
    if (tid == 0) s_max1 = red[0][0];
    __syncthreads();
    float m3[3] = {-3.4e38f, -3.4e38f, -3.4e38f};                 // vertices.max(0) after /max, *2
    for (int i = tid; i < nver; i += 1024)
        for (int k = 0; k < 3; ++k) m3[k] = fmaxf(m3[k], ((v[3 * i + k] - s_min[k]) / s_max1) * 2.f);
    __syncthreads();
    for (int k = 0; k < 3; ++k) red[k][tid] = m3[k];
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if (tid < s) for (int k = 0; k < 3; ++k) red[k][tid] = fmaxf(red[k][tid], red[k][tid + s]);
        __syncthreads();
    }
    if (tid < 3) s_max3[tid] = red[tid][0] / 2.f;
    __syncthreads();
    for (int i = tid; i < nver; i += 1024) {
        float vn[3], n[3], l[3];
        for (int k = 0; k < 3; ++k) {
            vn[k] = ((v[3 * i + k] - s_min[k]) / s_max1) * 2.f - s_max3[k];
            n[k] = nrm[3 * i + k];
            l[k] = amb[k];
        }
        if (cfg.i_dir > 0.f) {
            float d[3];
            for (int k = 0; k < 3; ++k) d[k] = cfg.light_pos[k] - vn[k];
            const float dl = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
            for (int k = 0; k < 3; ++k) d[k] = d[k] / dl;
            const float cs = n[0] * d[0] + n[1] * d[1] + n[2] * d[2];
            const float cc = clip01(cs);
            for (int k = 0; k < 3; ++k) l[k] += cfg.i_dir * (cfg.color_dir[k] * cc);
            if (cfg.i_spec > 0.f) {
                float e[3];
                for (int k = 0; k < 3; ++k) e[k] = cfg.view_pos[k] - vn[k];
                const float el = sqrtf(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
                float spe = 0.f;
                for (int k = 0; k < 3; ++k) {
                    const float r = (2.f * cs) * n[k] - d[k];
                    const float t1 = (e[k] / el) * r;
                    float t = t1;
                    for (int p = 1; p < cfg.spec_exp; ++p) t = t * t1;
                    spe = k == 0 ? t : spe + t;
                }
                spe = cs != 0.f ? clip01(spe) : 0.f;
                for (int k = 0; k < 3; ++k) l[k] += (cfg.i_spec * cfg.color_dir[k]) * clip01(spe);
            }
        }
        for (int k = 0; k < 3; ++k) {
            const float lk = clip01(l[k]);
            light[3 * i + k] = texture ? texture[3 * i + k] * lk : lk;
        }
    }
}

// rasterize_kernel.cpp:56-85
__device__ __forceinline__ void point_weight(float px, float py, float p0x, float p0y, float p1x, float p1y, float p2x, float p2y,
                                             float& w0, float& w1, float& w2) {
    const float v0x = p2x - p0x, v0y = p2y - p0y, v1x = p1x - p0x, v1y = p1y - p0y, v2x = px - p0x, v2y = py - p0y;
    const float d00 = v0x * v0x + v0y * v0y, d01 = v0x * v1x + v0y * v1y, d02 = v0x * v2x + v0y * v2y;
    const float d11 = v1x * v1x + v1y * v1y, d12 = v1x * v2x + v1y * v2y;
    const float den = d00 * d11 - d01 * d01;
    const float inv = den == 0.f ? 0.f : 1.f / den;
    const float u = (d11 * d02 - d01 * d12) * inv;
    const float vv = (d00 * d12 - d01 * d02) * inv;
    w0 = 1.f - u - vv; w1 = vv; w2 = u;
}

__device__ __forceinline__ unsigned orderable(float d) {
    const unsigned u = __float_as_uint(d);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// Key of mesh `mesh` (of 2^mbits), depth d, triangle t: later meshes win, then greater depth, then lower t.
// orderable() tells -0.0 from +0.0, the reference's `>` does not: both zeros take the key of +0.0.
__device__ __forceinline__ unsigned long long raster_key(int mesh, int mbits, float d, int t) {
    const unsigned long long top = mbits ? (unsigned long long)mesh << (64 - mbits) : 0ull;
    const unsigned long long tmask = (1ull << (32 - mbits)) - 1ull;
    const unsigned od = orderable(d == 0.f ? 0.f : d);
    return top | ((unsigned long long)od << (32 - mbits)) | (tmask - (unsigned)t);
}

__device__ __forceinline__ void raster_triangle(const float* __restrict__ v, const int32_t* __restrict__ tri, int t, int mesh,
                                                int mbits, int h, int w, unsigned long long* __restrict__ keys) {
    const int a = tri[3 * t], b = tri[3 * t + 1], c = tri[3 * t + 2];
    const float p0x = v[3 * a], p0y = v[3 * a + 1], z0 = v[3 * a + 2];
    const float p1x = v[3 * b], p1y = v[3 * b + 1], z1 = v[3 * b + 2];
    const float p2x = v[3 * c], p2y = v[3 * c + 1], z2 = v[3 * c + 2];
    const int x_min = max((int)ceilf(fminf(p0x, fminf(p1x, p2x))), 0);
    const int x_max = min((int)floorf(fmaxf(p0x, fmaxf(p1x, p2x))), w - 1);
    const int y_min = max((int)ceilf(fminf(p0y, fminf(p1y, p2y))), 0);
    const int y_max = min((int)floorf(fmaxf(p0y, fmaxf(p1y, p2y))), h - 1);
    if (x_max < x_min || y_max < y_min) return;
    for (int y = y_min; y <= y_max; ++y)
        for (int x = x_min; x <= x_max; ++x) {
            float w0, w1, w2;
            point_weight((float)x, (float)y, p0x, p0y, p1x, p1y, p2x, p2y, w0, w1, w2);
            if (w2 >= 0.f && w1 >= 0.f && w0 > 0.f) {
                const float d = w0 * z0 + w1 * z1 + w2 * z2;
                if (d > -1e8f) atomicMax(&keys[(size_t)y * w + x], raster_key(mesh, mbits, d, t));
            }
        }
}

// grid.y walks the meshes (v: n x nver x 3); ntri <= 2^(32 - mbits), n <= 2^mbits (checked by the callers)
__global__ void sim3dr_raster_kernel(const float* __restrict__ v, const int32_t* __restrict__ tri, int ntri, int n, int nver,
                                     int mbits, int h, int w, unsigned long long* __restrict__ keys) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntri) return;
    for (int mesh = blockIdx.y; mesh < n; mesh += gridDim.y)
        raster_triangle(v + (size_t)mesh * nver * 3, tri, t, mesh, mbits, h, w, keys);
}

// rasterize_kernel.cpp:280-289: the colour of triangle t of one mesh (v, col: nver x 3 / nver x c) at pixel (x, y) -> px[0..c)
__device__ __forceinline__ void paint_pixel(const float* __restrict__ v, const int32_t* __restrict__ tri, const float* __restrict__ col,
                                            int t, int x, int y, int c, unsigned char* __restrict__ px) {
    const int a = tri[3 * t], b = tri[3 * t + 1], cc = tri[3 * t + 2];
    float w0, w1, w2;
    point_weight((float)x, (float)y, v[3 * a], v[3 * a + 1], v[3 * b], v[3 * b + 1], v[3 * cc], v[3 * cc + 1], w0, w1, w2);
    const float alpha = 1.f;
    for (int k = 0; k < c; ++k) {
        const float pc = w0 * col[c * a + k] + w1 * col[c * b + k] + w2 * col[c * cc + k];
        px[k] = (unsigned char)((1 - alpha) * px[k] + alpha * 255 * pc);      // rasterize_kernel.cpp:287-288
    }
}

// v: n x nver x 3, col: n x nver x c; the winning mesh and triangle come out of the key
__global__ void sim3dr_resolve_kernel(const float* __restrict__ v, const int32_t* __restrict__ tri, const float* __restrict__ col,
                                      const unsigned long long* __restrict__ keys, int nver, int mbits, int h, int w, int c,
                                      int reverse, unsigned char* __restrict__ image) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= h * w) return;
    const unsigned long long key = keys[i];
    if (key == 0ull) return;                                              // no fragment: orderable(d > -1e8) is never 0
    const unsigned long long tmask = (1ull << (32 - mbits)) - 1ull;
    const int t = (int)(tmask - (key & tmask));
    const size_t mesh = mbits ? (size_t)(key >> (64 - mbits)) : 0;
    const int x = i % w, y = i / w;
    const int row = reverse ? (h - 1 - y) : y;
    paint_pixel(v + mesh * nver * 3, tri, col + mesh * nver * c, t, x, y, c, image + ((size_t)row * w + x) * c);
}

// ---- many canvases in one pass (romp_hip_canvases.h) -------------------------------------------------------
// Canvas c of C paints the slots [lo, lo + count) of v with a fresh z-buffer per slot: romp_sim3dr_render_batch on that
// slice, the mesh index in the key counted from lo and mesh_bits(count) key bits for it.  The range is read from the
// device offsets by every thread that needs it (two wave-uniform loads), clamped to [0, n]; a decreasing pair is empty.
__device__ __forceinline__ void canvas_range(const int32_t* __restrict__ off, int c, int n, int& lo, int& count, int& mbits) {
    lo = min(max(off[c], 0), n);
    count = max(min(max(off[c + 1], 0), n) - lo, 0);
    mbits = count <= 1 ? 0 : 32 - __clz(count - 1);                        // ceil(log2 count), mesh_bits() of the host
}

// grid.x: triangles, grid.z walks the canvases, grid.y the slots of a canvas (keys: C x h x w)
__global__ void sim3dr_raster_canvases_kernel(const float* __restrict__ v, const int32_t* __restrict__ tri, int ntri, int n, int nver,
                                              const int32_t* __restrict__ off, int C, int h, int w,
                                              unsigned long long* __restrict__ keys) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ntri) return;
    for (int c = blockIdx.z; c < C; c += gridDim.z) {
        int lo, count, mbits;
        canvas_range(off, c, n, lo, count, mbits);
        for (int m = blockIdx.y; m < count; m += gridDim.y)
            raster_triangle(v + (size_t)(lo + m) * nver * 3, tri, t, m, mbits, h, w, keys + (size_t)c * h * w);
    }
}

// one thread per pixel of all canvases (image: C x h x w x 3, col: n x nver x 3): 64-bit pixel and byte indices
__global__ __launch_bounds__(256) void sim3dr_resolve_canvases_kernel(const float* __restrict__ v, const int32_t* __restrict__ tri,
                                                                      const float* __restrict__ col,
                                                                      const unsigned long long* __restrict__ keys,
                                                                      const int32_t* __restrict__ off, int C, int n, int nver, int h,
                                                                      int w, unsigned char* __restrict__ image) {
    const size_t hw = (size_t)h * w, total = hw * C;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const unsigned long long key = keys[i];
        if (key == 0ull) continue;
        const size_t c = i / hw, p = i - c * hw;
        int lo, count, mbits;
        canvas_range(off, (int)c, n, lo, count, mbits);
        const unsigned long long tmask = (1ull << (32 - mbits)) - 1ull;
        const int t = (int)(tmask - (key & tmask));
        const size_t mesh = (size_t)lo + (mbits ? (size_t)(key >> (64 - mbits)) : 0);
        paint_pixel(v + mesh * nver * 3, tri, col + mesh * nver * 3, t, (int)(p % w), (int)(p / w), 3, image + i * 3);
    }
}

// Dense maps (romp_hip_maps.h): what the resolve pass decides per pixel, kept instead of painted.  One thread per pixel,
// the key decoded and the weights recomputed exactly as in sim3dr_resolve_kernel; background values where key == 0, so
// every byte of every non-null output is written.  C floats per pixel of attr_map are one store of C dwords: a wave
// writes 64 * C * 4 contiguous bytes, as it does 768 for bary_map.  person_pixels: one integer atomicAdd per distinct mesh
// of a wave (neighbouring pixels mostly share the mesh), so no thread leaves before the count.  vert_visible: racing
// stores of the same byte.  No float atomics: the outputs do not depend on the order of execution.
template <int C>
__global__ __launch_bounds__(256) void sim3dr_maps_kernel(const float* __restrict__ v, const int32_t* __restrict__ tri,
                                                          const unsigned long long* __restrict__ keys, int nver, int mbits,
                                                          int h, int w, const int32_t* __restrict__ mesh_ids,
                                                          const float* __restrict__ attrs, float attr_bg,
                                                          const uint8_t* __restrict__ vert_labels, int32_t* __restrict__ person_map,
                                                          int32_t* __restrict__ tri_map, float* __restrict__ bary_map,
                                                          float* __restrict__ attr_map, uint8_t* __restrict__ label_map,
                                                          uint8_t* __restrict__ vert_visible, int32_t* __restrict__ person_pixels) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool inside = i < (size_t)h * w;
    const unsigned long long key = inside ? keys[i] : 0ull;
    int mesh = -1, t = -1;
    if (key != 0ull) {                                                    // no fragment: orderable(d > -1e8) is never 0
        const unsigned long long tmask = (1ull << (32 - mbits)) - 1ull;
        t = (int)(tmask - (key & tmask));
        mesh = mbits ? (int)(key >> (64 - mbits)) : 0;
    }
    if (inside) {
        float w0 = 0.f, w1 = 0.f, w2 = 0.f;
        int a = 0, b = 0, cc = 0;
        if (t >= 0) {
            const float* vm = v + (size_t)mesh * nver * 3;
            const int x = (int)(i % w), y = (int)(i / w);
            a = tri[3 * t]; b = tri[3 * t + 1]; cc = tri[3 * t + 2];
            point_weight((float)x, (float)y, vm[3 * a], vm[3 * a + 1], vm[3 * b], vm[3 * b + 1], vm[3 * cc], vm[3 * cc + 1], w0, w1, w2);
        }
        if (person_map) person_map[i] = t < 0 ? -1 : (mesh_ids ? mesh_ids[mesh] : mesh);
        if (tri_map) tri_map[i] = t;
        if (bary_map) { bary_map[3 * i] = w0; bary_map[3 * i + 1] = w1; bary_map[3 * i + 2] = w2; }
        if (attr_map) {
            const float* am = attrs + (size_t)max(mesh, 0) * nver * C;
            float val[C];
            for (int k = 0; k < C; ++k)
                val[k] = t < 0 ? attr_bg : (w0 * am[C * a + k] + w1 * am[C * b + k]) + w2 * am[C * cc + k];
            for (int k = 0; k < C; ++k) attr_map[C * i + k] = val[k];
        }
        if (label_map) {
            int corner = a;                                               // the greatest weight, the lowest corner on ties
            float best = w0;
            if (w1 > best) { best = w1; corner = b; }
            if (w2 > best) corner = cc;
            label_map[i] = t < 0 ? (uint8_t)255 : vert_labels[corner];
        }
        if (vert_visible && t >= 0) {
            uint8_t* vis = vert_visible + (size_t)mesh * nver;
            vis[a] = 1; vis[b] = 1; vis[cc] = 1;
        }
    }
    if (person_pixels) {
        unsigned long long todo = __ballot(mesh >= 0);
        while (todo) {                                                    // wave-uniform: todo is the same in every lane
            const int leader = __ffsll((long long)todo) - 1;
            const int m = __shfl(mesh, leader);
            const unsigned long long same = __ballot(mesh == m);
            if ((int)(threadIdx.x & (warpSize - 1)) == leader) atomicAdd(&person_pixels[m], __popcll(same));
            todo &= ~same;
        }
    }
}


// ---- rotate_view_weak_perspective (vis_utils.py:26-51) ---------------------------------------------------
struct ViewCfg {
    float rx[9], ry[9];        // row-major, float32 of float64 cos / sin (vis_utils.py:10-24)
    float half[2];             // rendered_image_center: w / 2, h / 2
    float expand_ratio;
};

// work[0..2]: orderable(min) (atomicMin), work[3..5]: ~orderable(max) (atomicMin), work[6]: ~bits(max |xy / half|); all
// start at 0xFFFFFFFF.
__device__ __forceinline__ float from_orderable(unsigned u) { return __uint_as_float((u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u); }

__device__ __forceinline__ void rotate3(const float* r, float x, float y, float z, float& ox, float& oy, float& oz) {
    ox = x * r[0] + y * r[1] + z * r[2];                                   // einsum('bij,kj->bik'): out_k = sum_j v_j r[k][j]
    oy = x * r[3] + y * r[4] + z * r[5];
    oz = x * r[6] + y * r[7] + z * r[8];
}

template <int NV>
__device__ __forceinline__ void block_min_u32(unsigned (&val)[NV], unsigned* __restrict__ dst) {
    __shared__ unsigned red[NV][256];
    const int tid = threadIdx.x;
    for (int k = 0; k < NV; ++k) red[k][tid] = val[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) for (int k = 0; k < NV; ++k) red[k][tid] = min(red[k][tid], red[k][tid + s]);
        __syncthreads();
    }
    if (tid < NV) atomicMin(&dst[tid], red[tid][0]);
}

__global__ __launch_bounds__(256) void view_rotate_kernel(const float* __restrict__ v, long long count, ViewCfg cfg,
                                                          float* __restrict__ out, unsigned* __restrict__ work) {
    unsigned acc[6] = {~0u, ~0u, ~0u, ~0u, ~0u, ~0u};
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        float a[3], b[3];
        rotate3(cfg.rx, v[3 * i], v[3 * i + 1], v[3 * i + 2], a[0], a[1], a[2]);
        rotate3(cfg.ry, a[0], a[1], a[2], b[0], b[1], b[2]);
        for (int k = 0; k < 3; ++k) {
            out[3 * i + k] = b[k];
            acc[k] = min(acc[k], orderable(b[k]));
            acc[3 + k] = min(acc[3 + k], ~orderable(b[k]));
        }
    }
    block_min_u32<6>(acc, work);
}

__device__ __forceinline__ void view_center(const unsigned* __restrict__ work, float (&c)[3]) {
    for (int k = 0; k < 3; ++k) c[k] = 0.5f * (from_orderable(work[k]) + from_orderable(~work[3 + k]));
}

__global__ __launch_bounds__(256) void view_extent_kernel(const float* __restrict__ rot, long long count, ViewCfg cfg,
                                                          unsigned* __restrict__ work) {
    float c[3];
    view_center(work, c);
    unsigned acc[1] = {~0u};
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256)
        for (int k = 0; k < 2; ++k) acc[0] = min(acc[0], ~__float_as_uint(fabsf((rot[3 * i + k] - c[k]) / cfg.half[k])));
    block_min_u32<1>(acc, work + 6);
}

__global__ __launch_bounds__(256) void view_apply_kernel(float* __restrict__ out, long long count, ViewCfg cfg,
                                                         const unsigned* __restrict__ work, float* __restrict__ center_scale) {
    float c[3];
    view_center(work, c);
    const float scale = 1.f / (cfg.expand_ratio * __uint_as_float(~work[6]));   // 1 / t is t.reciprocal() * 1 in torch
    if (blockIdx.x == 0 && threadIdx.x < 4) center_scale[threadIdx.x] = threadIdx.x < 3 ? c[threadIdx.x] : scale;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256)
        for (int k = 0; k < 3; ++k) {
            float a = (out[3 * i + k] - c[k]) * scale;
            if (k < 2) a = a + cfg.half[k];
            out[3 * i + k] = a;
        }
}

// ---- turntable (romp_hip_canvases.h): K views of one scene with one shared fit -------------------------------
constexpr int kTurnViews = 128;                                            // views per launch: their cos / sin travel as kernel arguments

struct TurnCfg {
    float cs[kTurnViews][4];   // cos, sin of the azimuth, cos, sin of the tilt: float32 of float64 cos / sin
    float half[2];
    float expand_ratio;
};

__global__ __launch_bounds__(256) void turntable_bounds_kernel(const float* __restrict__ v, long long count, unsigned* __restrict__ work) {
    unsigned acc[6] = {~0u, ~0u, ~0u, ~0u, ~0u, ~0u};
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256)
        for (int k = 0; k < 3; ++k) {
            acc[k] = min(acc[k], orderable(v[3 * i + k]));
            acc[3 + k] = min(acc[3 + k], ~orderable(v[3 * i + k]));
        }
    block_min_u32<6>(acc, work);
}

// Rx(tilt) . (Ry(azimuth) . a), two rounded steps with the full matrices (their 0 and 1 entries multiply too)
__device__ __forceinline__ void turn_rotate(const float* cs, const float (&a)[3], float (&r)[3]) {
    const float ry[9] = {cs[0], 0.f, cs[1], 0.f, 1.f, 0.f, -cs[1], 0.f, cs[0]};
    const float rx[9] = {1.f, 0.f, 0.f, 0.f, cs[2], -cs[3], 0.f, cs[3], cs[2]};
    float b[3];
    rotate3(ry, a[0], a[1], a[2], b[0], b[1], b[2]);
    rotate3(rx, b[0], b[1], b[2], r[0], r[1], r[2]);
}

// grid.y: the views of this launch; work[6] gathers the extent of all of them
__global__ __launch_bounds__(256) void turntable_extent_kernel(const float* __restrict__ v, long long count, TurnCfg cfg,
                                                               unsigned* __restrict__ work) {
    float c[3];
    view_center(work, c);
    const float cs[4] = {cfg.cs[blockIdx.y][0], cfg.cs[blockIdx.y][1], cfg.cs[blockIdx.y][2], cfg.cs[blockIdx.y][3]};
    unsigned acc[1] = {~0u};
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const float a[3] = {v[3 * i] - c[0], v[3 * i + 1] - c[1], v[3 * i + 2] - c[2]};
        float r[3];
        turn_rotate(cs, a, r);
        for (int k = 0; k < 2; ++k) acc[0] = min(acc[0], ~__float_as_uint(fabsf(r[k] / cfg.half[k])));
    }
    block_min_u32<1>(acc, work + 6);
}

// grid.y: the views k0 + blockIdx.y; out (K,n,nver,3); order (K,n): the mesh in slot j of view k (clamped to [0, n)), or null
__global__ __launch_bounds__(256) void turntable_apply_kernel(const float* __restrict__ v, int n, int nver, TurnCfg cfg, int k0,
                                                              const int32_t* __restrict__ order, const unsigned* __restrict__ work,
                                                              float* __restrict__ out, float* __restrict__ center_scale) {
    float c[3];
    view_center(work, c);
    const float scale = 1.f / (cfg.expand_ratio * __uint_as_float(~work[6]));
    if (k0 == 0 && blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x < 4) center_scale[threadIdx.x] = threadIdx.x < 3 ? c[threadIdx.x] : scale;
    const float cs[4] = {cfg.cs[blockIdx.y][0], cfg.cs[blockIdx.y][1], cfg.cs[blockIdx.y][2], cfg.cs[blockIdx.y][3]};
    const long long count = (long long)n * nver, k = k0 + (long long)blockIdx.y;
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const long long j = i / nver, p = i - j * nver;
        const long long src = order ? (long long)min(max(order[k * n + j], 0), n - 1) : j;
        const float* s = v + (src * nver + p) * 3;
        const float a[3] = {s[0] - c[0], s[1] - c[1], s[2] - c[2]};
        float r[3];
        turn_rotate(cs, a, r);
        float* o = out + (k * count + i) * 3;
        o[0] = r[0] * scale + cfg.half[0];
        o[1] = r[1] * scale + cfg.half[1];
        o[2] = r[2] * scale;
    }
}

}  // namespace romp

using namespace romp;

namespace {

LightCfg light_cfg(const float* cfg_host, int spec_exp = 1) {
    LightCfg c;
    c.spec_exp = spec_exp;
    for (int k = 0; k < 3; ++k) {
        c.ambient[k] = cfg_host[k]; c.color_dir[k] = cfg_host[5 + k]; c.light_pos[k] = cfg_host[8 + k]; c.view_pos[k] = cfg_host[11 + k];
    }
    c.i_dir = cfg_host[3]; c.i_spec = cfg_host[4];
    return c;
}

int mesh_bits(int n) {                                                     // ceil(log2 n)
    int m = 0;
    while ((1ll << m) < n) ++m;
    return m;
}

constexpr int kMaxGridY = 65535;

// romp_sim3dr_render_batch (textures = null, spec_exp = 1) and romp_sim3dr_render_batch_tex: normals, light, raster, resolve
int render_batch(const char* who, unsigned char* image, int h, int w, const float* verts, int n, int nver, const int32_t* tris,
                 int ntri, const int32_t* adj_off, const int32_t* adj_ent, const float* ambient, const float* cfg_host,
                 const float* textures, int spec_exp, float* normals, float* light, unsigned long long* keys, void* stream) {
    ROMP_REQUIRE(image && verts && tris && adj_off && adj_ent && ambient && cfg_host && normals && light && keys && n > 0 &&
                 nver > 0 && ntri > 0 && h > 0 && w > 0, "%s: bad arguments", who);
    const int mbits = mesh_bits(n);
    ROMP_REQUIRE((long long)ntri <= (1ll << (32 - mbits)),
                 "%s: %d meshes leave %d key bits for the triangle index, %d triangles do not fit", who, n, 32 - mbits, ntri);
    hipStream_t st = (hipStream_t)stream;
    const unsigned gy = (unsigned)std::min(n, kMaxGridY);
    hipLaunchKernelGGL(sim3dr_normal_kernel, dim3((nver + 255) / 256, gy), dim3(256), 0, st, verts, tris, adj_off, adj_ent, nver, n,
                       normals);
    hipLaunchKernelGGL(sim3dr_light_kernel, dim3(n), dim3(1024), 0, st, verts, normals, nver, light_cfg(cfg_host, spec_exp), ambient,
                       textures, (const int32_t*)nullptr, light);
    ROMP_HIP_CHECK(hipMemsetAsync(keys, 0, (size_t)h * w * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(sim3dr_raster_kernel, dim3((ntri + 63) / 64, gy), dim3(64), 0, st, verts, tris, ntri, n, nver, mbits, h, w,
                       keys);
    hipLaunchKernelGGL(sim3dr_resolve_kernel, dim3((h * w + 255) / 256), dim3(256), 0, st, verts, tris, light, keys, nver, mbits, h,
                       w, 3, 0, image);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

}  // namespace

extern "C" {

int romp_sim3dr_normals(const float* verts, const int32_t* tris, const int32_t* adj_off, const int32_t* adj_ent, int nver,
                        float* normals, void* stream) {
    ROMP_REQUIRE(verts && tris && adj_off && adj_ent && normals && nver > 0, "romp_sim3dr_normals: bad arguments");
    hipLaunchKernelGGL(sim3dr_normal_kernel, dim3((nver + 255) / 256), dim3(256), 0, (hipStream_t)stream, verts, tris, adj_off,
                       adj_ent, nver, 1, normals);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_sim3dr_light(const float* verts, const float* normals, int nver, const float* cfg_host, float* light, void* stream) {
    ROMP_REQUIRE(verts && normals && cfg_host && light && nver > 0, "romp_sim3dr_light: bad arguments");
    hipLaunchKernelGGL(sim3dr_light_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, verts, normals, nver, light_cfg(cfg_host),
                       (const float*)nullptr, (const float*)nullptr, (const int32_t*)nullptr, light);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_sim3dr_light_tex(const float* verts, const float* normals, int nver, const float* cfg_host, int specular_exp,
                          const float* texture, float* light, void* stream) {
    ROMP_REQUIRE(verts && normals && cfg_host && light && nver > 0, "romp_sim3dr_light_tex: bad arguments");
    ROMP_REQUIRE(specular_exp >= 1, "romp_sim3dr_light_tex: specular_exp must be an integer >= 1, got %d", specular_exp);
    hipLaunchKernelGGL(sim3dr_light_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, verts, normals, nver,
                       light_cfg(cfg_host, specular_exp), (const float*)nullptr, texture, (const int32_t*)nullptr, light);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_sim3dr_rasterize(unsigned char* image, const float* verts, const int32_t* tris, const float* colors, int ntri, int h,
                          int w, int c, int reverse, unsigned long long* keys, void* stream) {
    ROMP_REQUIRE(image && verts && tris && colors && keys && ntri > 0 && h > 0 && w > 0 && c > 0 && c <= 4,
                 "romp_sim3dr_rasterize: bad arguments");
    hipStream_t st = (hipStream_t)stream;
    ROMP_HIP_CHECK(hipMemsetAsync(keys, 0, (size_t)h * w * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(sim3dr_raster_kernel, dim3((ntri + 63) / 64), dim3(64), 0, st, verts, tris, ntri, 1, 0, 0, h, w, keys);
    hipLaunchKernelGGL(sim3dr_resolve_kernel, dim3((h * w + 255) / 256), dim3(256), 0, st, verts, tris, colors, keys, 0, 0, h, w, c,
                       reverse, image);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_sim3dr_render_batch(unsigned char* image, int h, int w, const float* verts, int n, int nver, const int32_t* tris,
                             int ntri, const int32_t* adj_off, const int32_t* adj_ent, const float* ambient,
                             const float* cfg_host, float* normals, float* light, unsigned long long* keys, void* stream) {
    return render_batch("romp_sim3dr_render_batch", image, h, w, verts, n, nver, tris, ntri, adj_off, adj_ent, ambient, cfg_host,
                        nullptr, 1, normals, light, keys, stream);
}

int romp_sim3dr_render_batch_tex(unsigned char* image, int h, int w, const float* verts, int n, int nver, const int32_t* tris,
                                 int ntri, const int32_t* adj_off, const int32_t* adj_ent, const float* ambient,
                                 const float* cfg_host, const float* textures, int specular_exp, float* normals, float* light,
                                 unsigned long long* keys, void* stream) {
    ROMP_REQUIRE(specular_exp >= 1, "romp_sim3dr_render_batch_tex: specular_exp must be an integer >= 1, got %d", specular_exp);
    return render_batch("romp_sim3dr_render_batch_tex", image, h, w, verts, n, nver, tris, ntri, adj_off, adj_ent, ambient,
                        cfg_host, textures, specular_exp, normals, light, keys, stream);
}

int romp_view_weak_perspective(const float* verts, int n, int nver, double rx, double ry, int img_h, int img_w,
                               double expand_ratio, float* out, float* center_scale, unsigned* work, void* stream) {
    ROMP_REQUIRE(verts && out && center_scale && work && n > 0 && nver > 0 && img_h > 0 && img_w > 0 && expand_ratio > 0,
                 "romp_view_weak_perspective: bad arguments");
    ViewCfg cfg;
    const double ax = rx * (M_PI / 180.0), ay = ry * (M_PI / 180.0);          // np.radians
    const double mx[9] = {1, 0, 0, 0, std::cos(ax), -std::sin(ax), 0, std::sin(ax), std::cos(ax)};
    const double my[9] = {std::cos(ay), 0, std::sin(ay), 0, 1, 0, -std::sin(ay), 0, std::cos(ay)};
    for (int k = 0; k < 9; ++k) { cfg.rx[k] = (float)mx[k]; cfg.ry[k] = (float)my[k]; }
    cfg.half[0] = (float)(img_w / 2.0); cfg.half[1] = (float)(img_h / 2.0);
    cfg.expand_ratio = (float)expand_ratio;                                  // a python float times a float32 tensor: float32
    const long long count = (long long)n * nver;
    const unsigned grid = (unsigned)std::min<long long>((count + 255) / 256, 1024);
    hipStream_t st = (hipStream_t)stream;
    ROMP_HIP_CHECK(hipMemsetAsync(work, 0xFF, 7 * sizeof(unsigned), st));
    hipLaunchKernelGGL(view_rotate_kernel, dim3(grid), dim3(256), 0, st, verts, count, cfg, out, work);
    hipLaunchKernelGGL(view_extent_kernel, dim3(grid), dim3(256), 0, st, out, count, cfg, work);
    hipLaunchKernelGGL(view_apply_kernel, dim3(grid), dim3(256), 0, st, out, count, cfg, (const unsigned*)work, center_scale);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_sim3dr_render_canvases(unsigned char* images, int C, int h, int w, const float* verts, int n, int nver,
                                const int32_t* canvas_off, const int32_t* tris, int ntri, const int32_t* adj_off,
                                const int32_t* adj_ent, const float* ambient, const float* cfg_host, const float* textures,
                                const int32_t* rows, int specular_exp, float* normals, float* light, unsigned long long* keys,
                                void* stream) {
    ROMP_REQUIRE(images && verts && canvas_off && tris && adj_off && adj_ent && ambient && cfg_host && normals && light && keys &&
                 C > 0 && n > 0 && nver > 0 && ntri > 0 && h > 0 && w > 0, "romp_sim3dr_render_canvases: bad arguments");
    ROMP_REQUIRE(specular_exp >= 1, "romp_sim3dr_render_canvases: specular_exp must be an integer >= 1, got %d", specular_exp);
    const int mbits = mesh_bits(n);                                          // of all slots: no canvas holds more
    ROMP_REQUIRE((long long)ntri <= (1ll << (32 - mbits)),
                 "romp_sim3dr_render_canvases: %d meshes leave %d key bits for the triangle index, %d triangles do not fit", n,
                 32 - mbits, ntri);
    hipStream_t st = (hipStream_t)stream;
    const size_t pixels = (size_t)C * h * w;
    hipLaunchKernelGGL(sim3dr_normal_kernel, dim3((nver + 255) / 256, (unsigned)std::min(n, kMaxGridY)), dim3(256), 0, st, verts, tris,
                       adj_off, adj_ent, nver, n, normals);
    hipLaunchKernelGGL(sim3dr_light_kernel, dim3(n), dim3(1024), 0, st, verts, normals, nver, light_cfg(cfg_host, specular_exp), ambient,
                       textures, rows, light);
    ROMP_HIP_CHECK(hipMemsetAsync(keys, 0, pixels * sizeof(unsigned long long), st));
    const unsigned gy = (unsigned)std::min((n + C - 1) / C, kMaxGridY);     // an even split fills it; a fuller canvas strides
    hipLaunchKernelGGL(sim3dr_raster_canvases_kernel, dim3((ntri + 63) / 64, gy, (unsigned)std::min(C, kMaxGridY)), dim3(64), 0, st,
                       verts, tris, ntri, n, nver, canvas_off, C, h, w, keys);
    const unsigned gx = (unsigned)std::min<size_t>((pixels + 255) / 256, 1u << 22);
    hipLaunchKernelGGL(sim3dr_resolve_canvases_kernel, dim3(gx), dim3(256), 0, st, verts, tris, light,
                       (const unsigned long long*)keys, canvas_off, C, n, nver, h, w, images);
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_view_turntable(const float* verts, int n, int nver, int K, const double* azimuth_deg, const double* tilt_deg,
                        const int32_t* order, int img_h, int img_w, double expand_ratio, float* out, float* center_scale,
                        unsigned* work, void* stream) {
    ROMP_REQUIRE(verts && azimuth_deg && tilt_deg && out && center_scale && work && n > 0 && nver > 0 && K > 0 && img_h > 0 &&
                 img_w > 0 && expand_ratio > 0, "romp_view_turntable: bad arguments");
    TurnCfg cfg;
    cfg.half[0] = (float)(img_w / 2.0); cfg.half[1] = (float)(img_h / 2.0);
    cfg.expand_ratio = (float)expand_ratio;
    const long long count = (long long)n * nver;
    const unsigned grid = (unsigned)std::min<long long>((count + 255) / 256, 1024);
    hipStream_t st = (hipStream_t)stream;
    ROMP_HIP_CHECK(hipMemsetAsync(work, 0xFF, 7 * sizeof(unsigned), st));
    hipLaunchKernelGGL(turntable_bounds_kernel, dim3(grid), dim3(256), 0, st, verts, count, work);
    for (int pass = 0; pass < 2; ++pass)                                     // every view's extent before any view is scaled
        for (int k0 = 0; k0 < K; k0 += kTurnViews) {
            const int kc = std::min(K - k0, kTurnViews);
            for (int k = 0; k < kc; ++k) {
                const double az = azimuth_deg[k0 + k] * (M_PI / 180.0), ti = tilt_deg[k0 + k] * (M_PI / 180.0);   // np.radians
                cfg.cs[k][0] = (float)std::cos(az); cfg.cs[k][1] = (float)std::sin(az);
                cfg.cs[k][2] = (float)std::cos(ti); cfg.cs[k][3] = (float)std::sin(ti);
            }
            if (pass == 0)
                hipLaunchKernelGGL(turntable_extent_kernel, dim3(grid, kc), dim3(256), 0, st, verts, count, cfg, work);
            else
                hipLaunchKernelGGL(turntable_apply_kernel, dim3(grid, kc), dim3(256), 0, st, verts, n, nver, cfg, k0, order,
                                   (const unsigned*)work, out, center_scale);
        }
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

int romp_sim3dr_maps(const float* verts, int n, int nver, const int32_t* tris, int ntri, int h, int w, const int32_t* mesh_ids,
                     const float* attrs, int c, float attr_bg, const uint8_t* vert_labels, int32_t* person_map, int32_t* tri_map,
                     float* bary_map, float* attr_map, uint8_t* label_map, uint8_t* vert_visible, int32_t* person_pixels,
                     unsigned long long* keys, int keys_ready, void* stream) {
    ROMP_REQUIRE(verts && tris && keys && n > 0 && nver > 0 && ntri > 0 && h > 0 && w > 0, "romp_sim3dr_maps: bad arguments");
    ROMP_REQUIRE(!attr_map || (attrs && c >= 1 && c <= 4), "romp_sim3dr_maps: attr_map needs attrs of 1 to 4 channels, got c = %d", c);
    ROMP_REQUIRE(!label_map || vert_labels, "romp_sim3dr_maps: label_map needs vert_labels");
    const int mbits = mesh_bits(n);
    ROMP_REQUIRE((long long)ntri <= (1ll << (32 - mbits)),
                 "romp_sim3dr_maps: %d meshes leave %d key bits for the triangle index, %d triangles do not fit", n, 32 - mbits,
                 ntri);
    hipStream_t st = (hipStream_t)stream;
    if (!keys_ready) {
        ROMP_HIP_CHECK(hipMemsetAsync(keys, 0, (size_t)h * w * sizeof(unsigned long long), st));
        hipLaunchKernelGGL(sim3dr_raster_kernel, dim3((ntri + 63) / 64, (unsigned)std::min(n, kMaxGridY)), dim3(64), 0, st, verts, tris,
                           ntri, n, nver, mbits, h, w, keys);
    }
    if (vert_visible) ROMP_HIP_CHECK(hipMemsetAsync(vert_visible, 0, (size_t)n * nver, st));
    if (person_pixels) ROMP_HIP_CHECK(hipMemsetAsync(person_pixels, 0, (size_t)n * sizeof(int32_t), st));
    const dim3 grid((unsigned)(((size_t)h * w + 255) / 256));
#define ROMP_MAPS_LAUNCH(C)                                                                                                       \
    hipLaunchKernelGGL(sim3dr_maps_kernel<C>, grid, dim3(256), 0, st, verts, tris, (const unsigned long long*)keys, nver, mbits, h, \
                       w, mesh_ids, attrs, attr_bg, vert_labels, person_map, tri_map, bary_map, attr_map, label_map, vert_visible,  \
                       person_pixels)
    switch (attr_map ? c : 1) {
        case 1: ROMP_MAPS_LAUNCH(1); break;
        case 2: ROMP_MAPS_LAUNCH(2); break;
        case 3: ROMP_MAPS_LAUNCH(3); break;
        default: ROMP_MAPS_LAUNCH(4); break;
    }
#undef ROMP_MAPS_LAUNCH
    ROMP_HIP_CHECK(hipGetLastError());
    return ROMP_OK;
}

}  // extern "C"
