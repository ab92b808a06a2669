"""Mesh visualisation glue -- mirror of ``simple_romp/vis_human/main.py`` for the Sim3DR renderer
(``setup_renderer`` :11-21, ``rendering_romp_bev_results`` :23-113, items 'mesh', 'mesh_bird_view',
'mesh_side_view') and of ``vis_utils.mesh_color_left2right`` (:147-153).  The view transform and the
rasterization run on the device (renderer.py here); pyrender / open3d back-ends and the cv2 overlays
(pj2d, j3d, center_conf, tracking) are not part of the MI355X path."""
import numpy as np
import torch

from .renderer import Sim3DR, view_weak_perspective

# vis_utils.py:128-141 -- the palette persons are coloured with, left to right in the image
color_table_default = np.array([
    [0.4, 0.6, 1], [0.8, 0.7, 1], [0.1, 0.9, 1], [0.8, 0.9, 1], [1, 0.6, 0.4], [1, 0.7, 0.8], [1, 0.9, 0.1],
    [1, 0.9, 0.8], [0.9, 1, 1], [0.9, 0.7, 0.4], [0.8, 0.7, 1], [0.8, 0.9, 1], [0.9, 0.3, 0.1], [0.7, 1, 0.6],
    [0.7, 0.4, 0.6], [0.3, 0.5, 1]])[:, ::-1]


def setup_renderer(name='sim3dr', **kwargs):
    if name != 'sim3dr':
        raise NotImplementedError("renderer '%s': only 'sim3dr' runs on the MI355X path" % name)
    return Sim3DR(**kwargs)


def mesh_color_left2right(trans, color_table=None):
    """Colour index = rank of the person's x translation (vis_utils.py:147-153)."""
    order = torch.sort(trans[:, 0].cpu()).indices.numpy()
    inds = np.arange(len(trans))
    inds[order] = np.arange(len(trans))
    table = color_table_default if color_table is None else color_table
    return np.array([table[i % len(table)] for i in inds])


# show_items drawn on the device, in the order rendering_romp_bev_results appends their panels
DEVICE_ITEMS = ('mesh', 'mesh_bird_view', 'mesh_side_view')


def rendering_romp_bev_results(renderer, outputs, image, rendering_cfgs, alpha=1, keys=None):
    """main.py:23-113 for renderer 'sim3dr': persons painted far to near.  `outputs['rendered_image']` =
    [frame | mesh | bird view | side view], the panels of `rendering_cfgs['items']` in this fixed order whatever
    order the items are listed in.  'mesh': onto the frame.  The views: the meshes in camera space
    (verts + cam_trans, z negated), rotated and fitted by view_weak_perspective, onto a white h x h canvas.
    As in the reference, the side view is fitted to the frame's (h, w), not to the h x h canvas it is drawn on:
    for a frame wider than high its centre lies at x = w / 2, right of the canvas centre (kept, not fixed).
    `keys`: an int64 device tensor of h*w words the 'mesh' panel rasterizes into, for `dense_maps(..., keys=keys)`."""
    triangles = outputs['smpl_face'].cpu().numpy().astype(np.int32)
    cam_trans = outputs['cam_trans']
    if rendering_cfgs['mesh_color'] == 'identity':
        mesh_colors = mesh_color_left2right(cam_trans)
    elif rendering_cfgs['mesh_color'] == 'same':
        mesh_colors = np.array([[.9, .9, .8] for _ in range(len(cam_trans))])
    else:
        raise ValueError(rendering_cfgs['mesh_color'])
    items = rendering_cfgs['items']
    unsupported = [it for it in items if it not in DEVICE_ITEMS]
    if unsupported:
        raise NotImplementedError('show_items %s need OpenCV drawing (pj2d / j3d / center_conf / tracking), which is not on the '
                                  'device path' % unsupported)
    h, w = image.shape[:2]
    result_image = [image]
    depth_order = torch.sort(cam_trans[:, 2].cpu(), descending=True).indices
    colors = mesh_colors[depth_order.numpy()]
    if 'mesh' in items:
        vertices = outputs['verts_camed_org'][depth_order.to(outputs['verts_camed_org'].device)].clone()
        vertices[:, :, 2] = vertices[:, :, 2] * -1
        result_image.append(renderer(vertices, triangles, np.ascontiguousarray(image), mesh_colors=colors, keys=keys))
    views = [(it, rx, ry, shape) for it, rx, ry, shape in (('mesh_bird_view', -90, 0, (h, h)), ('mesh_side_view', 0, -90, (h, w)))
             if it in items]
    if views:
        verts = outputs['verts']
        verts_tran = (verts + cam_trans.to(verts.device).unsqueeze(1))[depth_order.to(verts.device)].float()
        verts_tran[:, :, 2] = verts_tran[:, :, 2] * -1
        background = torch.full((h, h, 3), 255, dtype=torch.uint8, device=verts_tran.device)
        for _, rx, ry, shape in views:
            view = view_weak_perspective(verts_tran, rx, ry, shape, expand_ratio=1.2)[0] if len(verts_tran) else verts_tran
            result_image.append(renderer(view, triangles, background, mesh_colors=colors))
    outputs['rendered_image'] = np.concatenate(result_image, 1)
    return outputs


def mesh_panel_keys(image_shape, device):
    """The tensor the 'mesh' panel and `dense_maps` share: one raster pass serves both."""
    return torch.empty(int(image_shape[0]) * int(image_shape[1]), dtype=torch.int64, device=device)


def dense_maps(renderer, outputs, image_shape, vert_labels, keys=None):
    """[romp_amd] `--dense_maps`: what the 'mesh' panel shows, per pixel and per vertex instead of as colours.  The geometry
    is that panel's: `verts_camed_org` with z negated, persons painted far to near by cam_trans[:, 2] (the depth_order of
    rendering_romp_bev_results), so a pixel belongs to the person the panel shows there.  Adds to `outputs` (device tensors;
    h, w = image_shape[:2], N persons):
      person_map (h,w) int32: the row of the result the pixel shows, -1 on the background;
      part_map (h,w) uint8: the body part, `vert_labels` (SMPL.part_labels, 0..23) at the nearest corner of the winning
        triangle, 255 on the background;
      depth_map (h,w) float32: camera-space z, (verts + cam_trans)[..., 2], interpolated affinely in screen space as the
        reference's depth buffer is; +inf on the background;
      verts_visible (N,6890) bool: the vertex is a corner of a triangle that shows in at least one pixel;
      person_pixels (N,) int32: the pixels each person shows in.
    `keys`: the tensor rendering_romp_bev_results(..., keys=keys) has just filled drawing the 'mesh' panel of this frame."""
    triangles = outputs['smpl_face'].cpu().numpy().astype(np.int32)
    cam_trans = outputs['cam_trans']
    org = outputs['verts_camed_org']
    depth_order = torch.sort(cam_trans[:, 2].cpu(), descending=True).indices
    order = depth_order.to(org.device)
    vertices = org[order].clone()
    vertices[:, :, 2] = vertices[:, :, 2] * -1
    verts = outputs['verts']
    cam_z = (verts + cam_trans.to(verts.device).unsqueeze(1))[order.to(verts.device)][:, :, 2:].float()
    m = renderer.maps(vertices, triangles, image_shape, mesh_ids=depth_order.int(), attrs=cam_z, attr_bg=float('inf'),
                      vert_labels=vert_labels, want=('person_map', 'attr_map', 'label_map', 'vert_visible', 'person_pixels'), keys=keys)
    visible = torch.empty_like(m['vert_visible'], dtype=torch.bool)
    visible[order] = m['vert_visible'].bool()                          # paint order -> result rows
    pixels = torch.empty_like(m['person_pixels'])
    pixels[order] = m['person_pixels']
    outputs.update({'person_map': m['person_map'], 'part_map': m['label_map'], 'depth_map': m['attr_map'][:, :, 0],
                    'verts_visible': visible, 'person_pixels': pixels})
    return outputs
