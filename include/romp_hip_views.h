/* romp_hip_views.h -- batched Sim3DR rendering and the bird / side mesh views of libromp_hip.so: additions to the C ABI
 * of romp_hip.h (same conventions, same ABI version 7; the symbols are listed in romp_amd/lib.py VIEW_EXPORTS). */
#ifndef ROMP_HIP_VIEWS_H
#define ROMP_HIP_VIEWS_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Sim3DR.__call__ (renderer.py:120-133) for n meshes of one topology: verts (n,nver,3) painted in index order onto
 * image (h,w,3) uint8 in place, each with a fresh z-buffer, in a fixed number of launches whatever n is.  ambient
 * (n,3): intensity_ambient * colour of each mesh as float32; cfg_host[14] as for romp_sim3dr_light (its ambient
 * entries are not read).  Scratch: normals, light (n,nver,3) floats, keys h*w 64-bit words.  The key holds
 * ceil(log2 n) mesh bits, so ntri <= 2^(32 - ceil(log2 n)) (EINVAL otherwise). */
int  romp_sim3dr_render_batch(unsigned char* image, int h, int w, const float* verts, int n, int nver, const int32_t* tris,
                              int ntri, const int32_t* adj_off, const int32_t* adj_ent, const float* ambient,
                              const float* cfg_host, float* normals, float* light, unsigned long long* keys, void* stream);
/* rotate_view_weak_perspective (vis_human/vis_utils.py:26-51) with bbox3D_center / scale computed: verts (n,nver,3)
 * rotated by Rx(rx degrees) then Ry(ry degrees), centred on the bbox of all n*nver points and scaled so that the
 * largest |xy| / (img_w/2, img_h/2) is 1 / expand_ratio, then shifted by (img_w/2, img_h/2) -> out (n,nver,3).
 * center_scale[4] = bbox centre xyz, scale.  work: 7 unsigned of scratch.  No host sync. */
int  romp_view_weak_perspective(const float* verts, int n, int nver, double rx, double ry, int img_h, int img_w,
                                double expand_ratio, float* out, float* center_scale, unsigned* work, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ROMP_HIP_VIEWS_H */
