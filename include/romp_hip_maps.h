/* romp_hip_maps.h -- dense per-pixel maps of the Sim3DR rasterizer of libromp_hip.so: an addition to the C ABI of
 * romp_hip.h (same conventions, same ABI version 7; the symbol is listed in romp_amd/lib.py MAP_EXPORTS). */
#ifndef ROMP_HIP_MAPS_H
#define ROMP_HIP_MAPS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* What Sim3DR.__call__ (renderer.py:128-135, rasterize_kernel.cpp _rasterize) decides per pixel, kept instead of
 * painted.  verts (n,nver,3), tris (ntri,3): n meshes of one topology painted in index order onto an h x w canvas,
 * each with a fresh z-buffer.  A pixel's winner is the highest mesh that covers it, inside that mesh the fragment of
 * greatest depth, the lowest triangle on equal depth (-0.0 and +0.0 are equal; a NaN depth or one not above -1e8 is no
 * fragment) -- the very winner whose colour romp_sim3dr_render_batch writes.
 * Every output pointer may be null; every byte of a non-null output is written by the call:
 *   person_map (h,w) int32      mesh_ids[mesh] (mesh_ids null: mesh); background -1
 *   tri_map    (h,w) int32      winning triangle; -1
 *   bary_map   (h,w,3) float32  (w0,w1,w2) of get_point_weight at the pixel; 0
 *   attr_map   (h,w,c) float32  (w0*a0 + w1*a1) + w2*a2 of attrs (n,nver,c), 1 <= c <= 4 (affine in screen space, as
 *                               the reference's depth buffer; attrs = verts z reproduces that buffer); attr_bg
 *   label_map  (h,w) uint8      vert_labels[corner of greatest weight, lowest corner on ties] (vert_labels (nver,)); 255
 *   vert_visible (n,nver) uint8 1 iff the vertex is a corner of a triangle that wins at least one pixel
 *   person_pixels (n,) int32    pixels each mesh wins
 * attr_map needs attrs, label_map needs vert_labels (EINVAL otherwise).  keys: h*w 64-bit words.  keys_ready = 0: they
 * are scratch, cleared and filled here by the rasterizer of romp_sim3dr_render_batch.  keys_ready = 1: the caller
 * states that romp_sim3dr_render_batch / romp_sim3dr_rasterize has just filled them for these very verts, tris, h, w
 * (n = 1 for romp_sim3dr_rasterize); no raster pass runs.  ntri <= 2^(32 - ceil(log2 n)) (EINVAL otherwise, before
 * anything is written).  No host sync, no float atomics: the outputs are deterministic. */
int  romp_sim3dr_maps(const float* verts, int n, int nver, const int32_t* tris, int ntri, int h, int w,
                      const int32_t* mesh_ids, const float* attrs, int c, float attr_bg, const uint8_t* vert_labels,
                      int32_t* person_map, int32_t* tri_map, float* bary_map, float* attr_map, uint8_t* label_map,
                      uint8_t* vert_visible, int32_t* person_pixels,
                      unsigned long long* keys, int keys_ready, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ROMP_HIP_MAPS_H */
