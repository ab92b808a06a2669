/* romp_hip_canvases.h -- many canvases in one pass: the batched Sim3DR render over C canvases of one size and the
 * K-view turntable transform of libromp_hip.so.  Additions to the C ABI of romp_hip.h and romp_hip_views.h (same
 * conventions, same ABI version 7; the symbols are listed in romp_amd/lib.py CANVAS_EXPORTS: a host that must run on an
 * older library looks them up by name). */
#ifndef ROMP_HIP_CANVASES_H
#define ROMP_HIP_CANVASES_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* romp_sim3dr_render_batch_tex for C canvases at once.  images (C,h,w,3) uint8, painted in place.  verts (n,nver,3): n
 * slots of one topology; the slots canvas_off[c] .. canvas_off[c+1]-1 are painted onto canvas c in slot order, each with
 * a fresh z-buffer.  canvas_off: C+1 int32 on the DEVICE, ascending; each value is clamped to [0, n] and a decreasing
 * pair is an empty canvas, so no offset can make a kernel read or write outside the buffers.  A canvas without slots
 * keeps its bytes and its keys are 0.
 * Slot j is lit with ambient[rows[j]] and coloured with textures[rows[j]] (rows: n int32 on the device, every value a
 * valid row of ambient / textures -- not checked), or with row j for rows = NULL; textures = NULL: the light alone.
 * cfg_host, specular_exp, and the scratch normals / light (n,nver,3) as for romp_sim3dr_render_batch_tex; keys: C*h*w
 * 64-bit words.
 * Afterwards the bytes of images[c] and the words of keys[c] are those romp_sim3dr_render_batch_tex writes for the
 * slice of canvas c alone, the key with ceil(log2 count_c) mesh bits (computed on the device) and the mesh index counted
 * from the slice's first slot: romp_sim3dr_maps(verts + slice, count_c, ..., keys + c*h*w, keys_ready = 1) may follow.
 * The host cannot see the counts, so it checks the conservative ntri <= 2^(32 - ceil(log2 n)) (EINVAL otherwise, like a
 * null pointer, a size < 1 or specular_exp < 1: before any launch).
 * Five launches whatever C and n are (normals, light, key clear, raster, resolve), no host sync, 64-bit pixel and byte
 * indices, no float atomics. */
int  romp_sim3dr_render_canvases(unsigned char* images, int C, int h, int w, const float* verts, int n, int nver,
                                 const int32_t* canvas_off, const int32_t* tris, int ntri, const int32_t* adj_off,
                                 const int32_t* adj_ent, const float* ambient, const float* cfg_host, const float* textures,
                                 const int32_t* rows, int specular_exp, float* normals, float* light, unsigned long long* keys,
                                 void* stream);
/* A turntable: K views of the scene verts (n,nver,3) with ONE fit, all in float32.  c0 = 0.5 * (min + max) of the
 * unrotated points; a = v - c0; r_k = Rx(tilt_k) . (Ry(azimuth_k) . a), two rounded steps: the spin about the vertical
 * axis first, then the tilt (romp_view_weak_perspective tilts first: its ground plane would wobble).  Matrices: float32
 * of float64 cos / sin of the angles in degrees (host arrays of K doubles); a rotation is (x*m0 + y*m1) + z*m2.
 * scale = 1 / (float32(expand_ratio) * max over all views and points of |r_k.xy / (img_w/2, img_h/2)|): one scale for all
 * views.  out (K,n,nver,3): out[k][j] = r_k[order[k*n + j]] * scale, xy += (img_w/2, img_h/2); order (K,n) int32 on the
 * device (values clamped to [0, n)), or NULL for the mesh index j.  center_scale[4] = c0 xyz, scale.  work: 7 unsigned
 * of scratch.  Three launches for K <= 128 (two more per further 128 views), no host sync. */
int  romp_view_turntable(const float* verts, int n, int nver, int K, const double* azimuth_deg, const double* tilt_deg,
                         const int32_t* order, int img_h, int img_w, double expand_ratio, float* out, float* center_scale,
                         unsigned* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ROMP_HIP_CANVASES_H */
