/* romp_hip_views.h -- batched Sim3DR rendering and the bird / side mesh views of libromp_hip.so: additions to the C ABI
 * of romp_hip.h (same conventions, same ABI version 7; the symbols are listed in romp_amd/lib.py VIEW_EXPORTS, the two
 * *_tex entries, added later, in TEXTURE_EXPORTS: a host that must run on an older library looks them up by name). */
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
/* romp_sim3dr_light (romp_hip.h) with a per-vertex texture and a specular exponent: light_out (nver,3) =
 * texture * light, one rounded float32 multiply of the clipped light (Sim3DR.render(texture=...), renderer.py:124), or
 * the light itself for texture = NULL.  specular_exp: an integer >= 1 (EINVAL otherwise), the power each component of
 * v2v * reflection is raised to before the three are summed (renderer.py:110), formed as specular_exp - 1 rounded
 * multiplies from left to right: exact for 1, numpy's square for 2, within rounding of numpy's powf above.
 * texture = NULL with specular_exp = 1 writes the bytes romp_sim3dr_light writes. */
int  romp_sim3dr_light_tex(const float* verts, const float* normals, int nver, const float* cfg_host, int specular_exp,
                           const float* texture, float* light_out, void* stream);
/* romp_sim3dr_render_batch with per-vertex colours: textures (n,nver,3) float32 or NULL, specular_exp as above; mesh i
 * is painted with textures[i] * light_i, light_i lit with ambient[i].  The same four launches (normals, light, raster,
 * resolve), the same scratch, and keys filled exactly as romp_sim3dr_render_batch fills them (romp_sim3dr_maps with
 * keys_ready = 1 may follow).  textures = NULL, specular_exp = 1: the bytes of romp_sim3dr_render_batch. */
int  romp_sim3dr_render_batch_tex(unsigned char* image, int h, int w, const float* verts, int n, int nver, const int32_t* tris,
                                  int ntri, const int32_t* adj_off, const int32_t* adj_ent, const float* ambient,
                                  const float* cfg_host, const float* textures, int specular_exp, float* normals, float* light,
                                  unsigned long long* keys, void* stream);
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
