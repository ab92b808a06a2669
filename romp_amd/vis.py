"""Mesh visualisation glue -- mirror of ``simple_romp/vis_human/main.py`` for the Sim3DR renderer
(``setup_renderer`` :11-21, ``rendering_romp_bev_results`` :23-113, items 'mesh', 'mesh_bird_view',
'mesh_side_view', 'rotate_mesh'), of ``vis_utils.rendering_mesh_rotating_view`` (:101-125, the turntable) and of ``vis_utils.mesh_color_left2right`` (:147-153) and ``mesh_color_trackID`` (:238-241).  The view transform and the
rasterization run on the device (renderer.py here); pyrender / open3d back-ends and the cv2 overlays
(pj2d, j3d, center_conf, tracking) are not part of the MI355X path."""
import numpy as np
import torch

from .renderer import Sim3DR, turntable_views, view_weak_perspective

# vis_utils.py:128-141 -- the palette persons are coloured with, left to right in the image
color_table_default = np.array([
    [0.4, 0.6, 1], [0.8, 0.7, 1], [0.1, 0.9, 1], [0.8, 0.9, 1], [1, 0.6, 0.4], [1, 0.7, 0.8], [1, 0.9, 0.1],
    [1, 0.9, 0.8], [0.9, 1, 1], [0.9, 0.7, 0.4], [0.8, 0.7, 1], [0.8, 0.9, 1], [0.9, 0.3, 0.1], [0.7, 1, 0.6],
    [0.7, 0.4, 0.6], [0.3, 0.5, 1]])[:, ::-1]


# vis_utils.py:155-236 -- the 79 colours persons are coloured with by track id (the detection-toolkit colour list), float32
tracking_color_list = np.array(
    [[0.000, 0.447, 0.741], [0.850, 0.325, 0.098], [0.929, 0.694, 0.125], [0.494, 0.184, 0.556], [0.466, 0.674, 0.188],
     [0.301, 0.745, 0.933], [0.635, 0.078, 0.184], [0.300, 0.300, 0.300], [0.600, 0.600, 0.600], [1.000, 0.000, 0.000],
     [1.000, 0.500, 0.000], [0.749, 0.749, 0.000], [0.000, 1.000, 0.000], [0.000, 0.000, 1.000], [0.667, 0.000, 1.000]]
    + [[r, g, 0.000] for r in (0.333, 0.667, 1.000) for g in (0.333, 0.667, 1.000)]
    + [[r, g, 0.500] for r in (0.000, 0.333, 0.667, 1.000) for g in (0.000, 0.333, 0.667, 1.000)][1:]
    + [[r, g, 1.000] for r in (0.000, 0.333, 0.667, 1.000) for g in (0.000, 0.333, 0.667, 1.000)][1:-1]
    + [[x, 0.000, 0.000] for x in (0.167, 0.333, 0.500, 0.667, 0.833, 1.000)]
    + [[0.000, x, 0.000] for x in (0.167, 0.333, 0.500, 0.667, 0.833, 1.000)]
    + [[0.000, 0.000, x] for x in (0.167, 0.333, 0.500, 0.667, 0.833, 1.000)]
    + [[x, x, x] for x in (0.000, 0.143, 0.286, 0.429, 0.571, 0.714, 0.857, 1.000)], np.float32)

# [romp_amd] mesh_color 'part': one colour per SMPL body part (SMPL.part_labels, 0..23), picked by hand so that the rows
# are distinct and consecutive labels contrast; all in [0, 1]
part_palette = np.array([
    [0.90, 0.30, 0.30], [0.30, 0.75, 0.45], [0.35, 0.45, 0.90], [0.95, 0.80, 0.25], [0.70, 0.35, 0.85], [0.25, 0.80, 0.85],
    [0.95, 0.55, 0.20], [0.55, 0.85, 0.30], [0.90, 0.40, 0.70], [0.35, 0.60, 0.60], [0.65, 0.50, 0.35], [0.50, 0.55, 0.95],
    [0.80, 0.20, 0.45], [0.20, 0.60, 0.30], [0.60, 0.70, 1.00], [0.75, 0.65, 0.10], [0.45, 0.25, 0.65], [0.10, 0.55, 0.70],
    [1.00, 0.70, 0.55], [0.40, 0.65, 0.15], [1.00, 0.65, 0.90], [0.60, 0.85, 0.80], [0.85, 0.75, 0.60], [0.75, 0.80, 1.00]], np.float32)

MESH_COLOR_MODES = ('identity', 'same', 'track_id', 'part')


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


def mesh_color_trackID(track_ids, color_table=None):
    """Colour = the table's row track id modulo its length (vis_utils.py:238-241): stable while a person keeps the id."""
    table = tracking_color_list if color_table is None else color_table
    return np.array([table[tid % len(table)] for tid in track_ids])


# show_items drawn on the device, in the order rendering_romp_bev_results appends their panels ('rotate_mesh' is no panel:
# its frames go to outputs['rotate_mesh_frames'])
DEVICE_ITEMS = ('mesh', 'mesh_bird_view', 'mesh_side_view', 'rotate_mesh')


def _mesh_colors(mode, cam_trans, track_ids=None, part_labels=None):
    """(mesh_colors (n,3), part_colors (V,3) or None) of one frame's persons for a `mesh_color` mode."""
    part_colors = None
    if mode == 'identity' or (mode == 'track_id' and track_ids is None):
        mesh_colors = mesh_color_left2right(cam_trans)
    elif mode == 'track_id':
        mesh_colors = mesh_color_trackID(track_ids.cpu().numpy() if torch.is_tensor(track_ids) else np.asarray(track_ids))
        mesh_colors = mesh_colors.reshape(len(cam_trans), 3)
    elif mode == 'same':
        mesh_colors = np.array([[.9, .9, .8] for _ in range(len(cam_trans))])
    elif mode == 'part':
        if part_labels is None:
            raise ValueError("mesh_color 'part' needs rendering_cfgs['part_labels'], the (V,) part label of every vertex")
        mesh_colors = np.ones((len(cam_trans), 3))
        labels = part_labels.cpu().numpy() if torch.is_tensor(part_labels) else np.asarray(part_labels)
        part_colors = part_palette[labels.reshape(-1).astype(np.int64)]                    # (V,3): the same for every person
    else:
        raise ValueError(mode)
    return mesh_colors, part_colors


def rendering_romp_bev_results(renderer, outputs, image, rendering_cfgs, alpha=1, keys=None):
    """main.py:23-113 for renderer 'sim3dr': persons painted far to near.  `outputs['rendered_image']` =
    [frame | mesh | bird view | side view], the panels of `rendering_cfgs['items']` in this fixed order whatever
    order the items are listed in.  'mesh': onto the frame.  The views: the meshes in camera space
    (verts + cam_trans, z negated), rotated and fitted by view_weak_perspective, onto a white h x h canvas.
    As in the reference, the side view is fitted to the frame's (h, w), not to the h x h canvas it is drawn on:
    for a frame wider than high its centre lies at x = w / 2, right of the canvas centre (kept, not fixed).
    `rendering_cfgs['mesh_color']`, for every panel: 'identity' colours persons left to right and 'same' alike, as the
    reference's values do without tracking; [romp_amd] 'track_id' by `outputs['track_ids']` (mesh_color_trackID; what
    the reference's 'identity' does once track ids exist), left to right when there are none; [romp_amd] 'part' paints
    every vertex with part_palette[rendering_cfgs['part_labels']] (the (V,) labels of SMPL.part_labels) under white
    ambient light.
    [romp_amd] 'rotate_mesh' (advertised by the reference's --show_items, drawn there by pyrender only): no panel; the
    turntable of the scene, `rendering_mesh_rotating_view` of the meshes in camera space onto white s x s canvases,
    s = rendering_cfgs.get('rotate_size', 512), as outputs['rotate_mesh_frames'] (K,s,s,3) uint8, K = 96 frames.
    `keys`: an int64 device tensor of h*w words the 'mesh' panel rasterizes into, for `dense_maps(..., keys=keys)`."""
    triangles = outputs['smpl_face'].cpu().numpy().astype(np.int32)
    cam_trans = outputs['cam_trans']
    mesh_colors, part_colors = _mesh_colors(rendering_cfgs['mesh_color'], cam_trans, outputs.get('track_ids'),
                                            rendering_cfgs.get('part_labels'))
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
        result_image.append(renderer(vertices, triangles, np.ascontiguousarray(image), mesh_colors=colors,
                                     vert_colors=_per_person(part_colors, vertices), keys=keys))
    views = [(it, rx, ry, shape) for it, rx, ry, shape in (('mesh_bird_view', -90, 0, (h, h)), ('mesh_side_view', 0, -90, (h, w)))
             if it in items]
    if views or 'rotate_mesh' in items:
        verts = outputs['verts']
        verts_tran = (verts + cam_trans.to(verts.device).unsqueeze(1))[depth_order.to(verts.device)].float()
        verts_tran[:, :, 2] = verts_tran[:, :, 2] * -1
        background = torch.full((h, h, 3), 255, dtype=torch.uint8, device=verts_tran.device)
        for _, rx, ry, shape in views:
            view = view_weak_perspective(verts_tran, rx, ry, shape, expand_ratio=1.2)[0] if len(verts_tran) else verts_tran
            result_image.append(renderer(view, triangles, background, mesh_colors=colors, vert_colors=_per_person(part_colors, view)))
        if 'rotate_mesh' in items:
            size = int(rendering_cfgs.get('rotate_size', 512))
            outputs['rotate_mesh_frames'] = rendering_mesh_rotating_view(renderer, verts_tran, triangles, (size, size), colors,
                                                                         vert_colors=_per_person(part_colors, verts_tran))
    outputs['rendered_image'] = np.concatenate(result_image, 1)
    return outputs


def turntable_angles(pause=24, step=5):
    """vis_utils.py:101-110: the azimuths of the reference's rotating view in degrees: `pause` frames at 0, then the running sum
    of 4 * (90 // step) steps of `step` degrees -- 96 frames by default, the last one at 360."""
    return np.concatenate([np.zeros(pause), np.cumsum(np.ones(4 * (90 // step)) * step)])


def rendering_mesh_rotating_view(renderer, verts_tran, triangles, canvas_hw, mesh_colors, vert_colors=None, azimuths=None, tilt=-20.):
    """[romp_amd] vis_utils.rendering_mesh_rotating_view (:101-125, pyrender only there) on the device: the turntable of the
    scene verts_tran (n,V,3) (device tensor, camera space with z negated as for the bird view: greater z is nearer) on white
    canvas_hw = (h, w) canvases -> (K,h,w,3) uint8 numpy, one frame per azimuth (default `turntable_angles()`: 96 frames).
    Every view spins the scene about its bbox centre by the azimuth, tilts it by `tilt` degrees (-20 looks down on the scene the
    way the reference's camera, raised by 20 degrees, does) and uses ONE scale (`turntable_views`), so the scene does not
    breathe while it turns.  Per view the persons are painted far to near: slots ascending by the z of the person's rotated
    centroid, the lower index first on ties.  Person i keeps mesh_colors[i % len(mesh_colors)] and vert_colors[i] ((n,V,3) or
    None) in every view.  One view transform and one `render_canvases` call: the launches do not grow with K or n, and all
    frames come back in one download."""
    h, w = int(canvas_hw[0]), int(canvas_hw[1])
    az = turntable_angles() if azimuths is None else np.asarray(azimuths, np.float64).reshape(-1)
    K, n = len(az), len(verts_tran)
    white = np.full((h, w, 3), 255, np.uint8)
    if n == 0 or K == 0:
        return np.broadcast_to(white, (K, h, w, 3)).copy()
    verts = verts_tran.float()
    dev = verts.device
    # the z of Rx(tilt) . Ry(azimuth) . centroid per view: (K,n), float64 (the bbox centre shifts every person alike)
    cen = verts.double().mean(1)
    ang = torch.from_numpy(np.radians(az)).to(dev)
    ct, st = float(np.cos(np.radians(tilt))), float(np.sin(np.radians(tilt)))
    z = cen[None, :, 1] * st + (cen[None, :, 2] * torch.cos(ang)[:, None] - cen[None, :, 0] * torch.sin(ang)[:, None]) * ct
    order = torch.argsort(z, dim=1, stable=True)
    views = turntable_views(verts, az, float(tilt), (h, w), expand_ratio=1.2, order=order)[0]
    palette = np.asarray(mesh_colors).reshape(-1, 3)
    return renderer.render_canvases(views.reshape(K * n, verts.shape[1], 3), triangles, white, np.arange(K + 1) * n,
                                    mesh_colors=palette[np.arange(n) % len(palette)], vert_colors=vert_colors,
                                    rows=order.reshape(-1))


def render_mesh_frames(renderer, verts_camed_org, cam_trans, batch_ids, frames, triangles, mesh_color='identity', track_ids=None,
                       part_labels=None):
    """[romp_amd] The 'mesh' panel of `rendering_romp_bev_results` for the B same-sized frames of a batch in one render call
    and one download: frames (B,h,w,3) uint8 (numpy or device), persons verts_camed_org (N,V,3) (device, already projected to
    their frames) with cam_trans (N,3) and batch_ids (N,) ascending frame indices, as `forward_batch` returns them.  Per frame
    the persons are painted far to near (cam_trans[:, 2] descending, z negated) and coloured as that function colours them in
    an image of its own: `mesh_color` 'identity' is left to right WITHIN the frame.  -> (B,h,w,3) uint8 numpy; a frame without
    persons comes back unchanged.  (cam_trans and batch_ids, a few floats per person, are read back to order the persons.)"""
    B = len(frames)
    ct = (cam_trans.detach() if torch.is_tensor(cam_trans) else torch.from_numpy(np.asarray(cam_trans))).cpu().float()
    ids = (batch_ids.detach().cpu().numpy() if torch.is_tensor(batch_ids) else np.asarray(batch_ids)).reshape(-1).astype(np.int64)
    tids = None if track_ids is None else (track_ids.cpu().numpy() if torch.is_tensor(track_ids) else np.asarray(track_ids)).reshape(-1)
    perm, colors, offsets, part_colors = [], [], [0], None
    for b in range(B):
        idx = np.nonzero(ids == b)[0]
        if len(idx):
            mesh_colors, part_colors = _mesh_colors(mesh_color, ct[idx], None if tids is None else tids[idx], part_labels)
            depth_order = torch.sort(ct[idx][:, 2], descending=True).indices.numpy()
            perm.append(idx[depth_order])
            colors.append(np.asarray(mesh_colors)[depth_order])
        offsets.append(offsets[-1] + len(idx))
    if not perm:
        return renderer.render_canvases(verts_camed_org[:0], triangles, frames, offsets)
    perm = torch.from_numpy(np.concatenate(perm))
    vertices = verts_camed_org[perm.to(verts_camed_org.device)].clone()
    vertices[:, :, 2] = vertices[:, :, 2] * -1
    return renderer.render_canvases(vertices, triangles, frames, offsets, mesh_colors=np.concatenate(colors),
                                    vert_colors=_per_person(part_colors, vertices))


def _per_person(part_colors, verts):
    """part_colors (V,3) numpy -> (n,V,3) on the device of verts (n,V,3), or None."""
    if part_colors is None:
        return None
    return torch.from_numpy(part_colors).to(verts.device).unsqueeze(0).expand(len(verts), -1, -1).contiguous()


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
