"""BEV on the MI355X -- mirror of ``simple_romp/bev/main.py`` (``bev_settings`` :27-87, ``BEV`` :91-181)
and of the device-side steps of ``BEVv1.forward`` (bev/model.py:232-250) for BASELINE config 4.

    from romp_amd import bev
    model = bev.BEV(bev.bev_settings([]), state_dict=..., smpla_model=..., smil_model=...)
    outputs = model(bgr_image)         # dict of numpy arrays, or None

Network (HRNet-32 + BEV head), 3-D center parsing, per-person regression, SMPL-A / SMIL meshes,
perspective projection, projection-based duplicate suppression and outlier removal
(bev/post_parser.py:68-136,167-222) all run in libromp_hip.so.  Video mode (``-t``): ByteTrack-3D association on the host
(tracker.py) or, with ``--device_tracker``, on the device (tracking.py) + OneEuro filters on the device (temporal.py); ``--render_mesh``: the Sim3DR rasteriser (renderer.py).
Crowd mode (``--crowd``, bev/main.py:184-258, bev/split2process.py): a frame with W / H >= 2 is cut into overlapping crops that
go through ONE batched pre-processing launch (csrc/crowd.hip), the network in chunks of ``max_batch``, one SMPL-A / SMIL call
and a device merge (boundary exclusion, per-crop and full-frame suppression / outlier removal).  The reference turns crowd mode
on by default; here it stays off unless asked for.  One deviation: where the reference raises because a crop before a crop
with people has no detections, an empty crop here simply contributes nobody.
"""
import argparse
import ctypes as C
import os.path as osp
import sys

import numpy as np
import torch
from torch import nn

from . import lib as L
from .bev_plan import DEPTH, MAP, build_bev_hrnet32, cam3dmap_anchor
from .net import RangeGuard, RompNet
from .smpl import SMPL
from .utils import convert_tensor2numpy, determine_device, img_preprocess_device


def bev_settings(input_args=sys.argv[1:]):
    """bev/main.py:27-87 (model_id 2 defaults; rendering / crowd / temporal flags kept for
    compatibility, the options they enable are outside the MI355X hot path)."""
    p = argparse.ArgumentParser(description='BEV on MI355X')
    p.add_argument('-m', '--mode', type=str, default='image')
    p.add_argument('--model_id', type=int, default=2)
    p.add_argument('-i', '--input', type=str, default=None)
    p.add_argument('-o', '--save_path', type=str, default=osp.join(osp.expanduser('~'), 'BEV_results'))
    p.add_argument('--crowd', action='store_true',
                   help='process a frame with width / height >= 2 as overlapping crops (sliding window) and merge their people; '
                        '[romp_amd] off by default, the reference defaults it to on')
    p.add_argument('--GPU', type=int, default=0)
    p.add_argument('--overlap_ratio', type=float, default=0.8)
    p.add_argument('--center_thresh', type=float, default=0.1)
    p.add_argument('--nms_thresh', type=float, default=20)
    p.add_argument('--relative_scale_thresh', type=float, default=1.6)
    p.add_argument('--show_largest', action='store_true')
    p.add_argument('--show_patch_results', action='store_true',
                   help='[romp_amd] accepted for compatibility, not supported: no per-crop renderings are written')
    p.add_argument('--calc_smpl', action='store_false')
    p.add_argument('--render_mesh', action='store_true',
                   help='[romp_amd] off by default (the reference defaults to on, with --show_items mesh,mesh_bird_view)')
    p.add_argument('--renderer', type=str, default='sim3dr')
    p.add_argument('--show_items', type=str, default='mesh',
                   help='any of mesh, mesh_bird_view, mesh_side_view (panels in that order) and rotate_mesh (a 96-frame turntable of '
                        'the scene, returned as rotate_mesh_frames); the cv2 overlays are not supported')
    p.add_argument('--rotate_size', type=int, default=512, help='[romp_amd] side of the square frames of --show_items rotate_mesh')
    p.add_argument('--mesh_color', type=str, default='identity', choices=['identity', 'same', 'track_id', 'part'],
                   help='[romp_amd] how --render_mesh colours the meshes: identity: per person, left to right (default); same: one colour; '
                        'track_id: per person by track id, stable across frames with -t; part: per vertex by SMPL body part')
    p.add_argument('-sc', '--smooth_coeff', type=float, default=3.)
    p.add_argument('--show', action='store_true')
    p.add_argument('--smpl_path', type=str, default=osp.join(osp.expanduser('~'), '.romp', 'SMPLA_NEUTRAL.pth'))
    p.add_argument('--smil_path', type=str, default=osp.join(osp.expanduser('~'), '.romp', 'smil_packed_info.pth'))
    p.add_argument('--model_path', type=str, default=osp.join(osp.expanduser('~'), '.romp', 'BEV.pth'))
    p.add_argument('-t', '--temporal_optimize', action='store_true')
    p.add_argument('--device_tracker', action='store_true',
                   help='[romp_amd] with -t: ByteTrack-3D association on the device too (tracking.py): two launches and one download per '
                        'frame instead of three downloads and the host tracker; same results while a source has seen at most 256 track '
                        'ids (beyond that the host filter bank clears all its filters, the device one never does)')
    p.add_argument('--max_batch', type=int, default=32)
    p.add_argument('--conv_math', type=str, default='f16x2', choices=['f32', 'bf16x3', 'f16x2', 'all'],
                   help='[romp_amd] f32 MFMA only, or also the f32-accurate split-precision kernels (f16x2: 2 fp16 pieces; bf16x3; chosen by autotune)')
    p.add_argument('--dense_maps', action='store_true',
                   help='[romp_amd] also return per-pixel maps of the mesh panel (person_map, part_map, depth_map) and per-person '
                        'verts_visible / person_pixels, computed on the device (vis.dense_maps)')
    args = p.parse_args(input_args)
    if not torch.cuda.is_available():
        args.GPU = -1
    if args.dense_maps:
        args.calc_smpl = True
    if args.crowd:                                                          # bev/main.py:79-83
        args.center_thresh, args.nms_thresh, _, args.overlap_ratio = LONG_CONF[args.model_id]
        args.relative_scale_thresh = LONG_CONF[MODEL_ID][2]                 # (indexed with the module-global model id, as there)
    return args


MODEL_ID = 2                                                                # bev/main.py:24-25
LONG_CONF = {1: [0.12, 20, 1.5, 0.46], 2: [0.08, 20, 1.6, 0.8]}           # center_thresh, nms_thresh, relative_scale_thresh, overlap


def crowd_pad_length(h, overlap_ratio):
    """padding_image_overlap (bev/split2process.py:6-21): zero columns added on each side of the frame."""
    return int(h * overlap_ratio)


def crowd_pad_info(h, w):
    """padding_image_overlap's image_pad_info, on the unpadded size: the square-padding convention of the full frame."""
    top = (w - h) // 2
    return [float(top), float(w - top), 0., float(w), float(h), float(w)]


def crowd_split_plan(h, w_pad, overlap_ratio):
    """get_image_split_plan (bev/split2process.py:23-37) on the padded width -> (K,4) int32 left, right, top, bottom.  The last
    crop's left is w_pad - h, its right the one left over from the previous step (so it is narrower than h)."""
    slide_time = int(np.ceil((w_pad / h - 1) / (1 - overlap_ratio))) + 1
    move_step = (1 - overlap_ratio) * h
    boxes = []
    for ind in range(slide_time):
        if ind == slide_time - 1:
            left = w_pad - h
        else:
            left = move_step * ind
            right = left + h
        boxes.append([left, right, 0, h])
    return np.array(boxes).astype(np.int32)


TAN_FOV = float(np.tan(np.radians(60 / 2.)))


def denormalize_cam_params_to_trans(normed_cams):
    """bev/post_parser.py:114-128 (positive_constrain False): (scale, ty, tx) -> camera-space translation."""
    depth = (1. / (normed_cams[:, 0] * TAN_FOV + 1e-3)).unsqueeze(1)
    return torch.cat([torch.flip(normed_cams[:, 1:], [1]) * depth * TAN_FOV, depth], 1)


class CenterMap3D(object):
    """bev/post_parser.py:19-66 -- parse configuration + the device parse."""

    def __init__(self, conf_thresh):
        self.size, self.max_person, self.conf_thresh = 128, 64, conf_thresh

    def parse_3dcentermap(self, center_maps):
        """center_maps (B,64,128,128) device tensor -> [batch_ids (N), center_zyxs (N,3), scores (N)]
        (int64 / int64 / float32), batch-major and score-descending; empty tensors if nobody."""
        lib = L.load()
        dev = center_maps.device
        if dev.type != 'cuda':
            raise L.RompHipError('3-D center parsing runs on the HIP device only (no CPU fallback)')
        cm = center_maps.contiguous().float()
        B = cm.shape[0]
        cap = B * self.max_person
        bids = torch.empty(cap, device=dev, dtype=torch.int32)
        czyx = torch.empty(cap, 3, device=dev, dtype=torch.int32)
        conf = torch.empty(cap, device=dev, dtype=torch.float32)
        ws = torch.empty(lib.romp_bev_workspace_ints(B, self.max_person), device=dev, dtype=torch.int32)
        n = C.c_int32(0)
        with torch.cuda.device(dev):
            L.check(lib.romp_bev_parse(L.ptr(cm), B, float(self.conf_thresh), self.max_person, C.byref(n), L.ptr(bids),
                                       L.ptr(czyx), L.ptr(conf), L.ptr(ws), L.stream_ptr(dev)))
        N = n.value
        return [bids[:N].long(), czyx[:N].long(), conf[:N]]


class BEVv1(object):
    """Device-side BEVv1 (bev/model.py:104-250): network program + parse + per-person regression."""

    def __init__(self, state_dict, device, center_thresh=0.1, max_batch=32, bf16x3=False):
        self.device = torch.device(device)
        self.net = RompNet(state_dict, self.device, max_batch=max_batch, builder=build_bev_hrnet32,
                           out_shapes=((DEPTH, MAP, MAP), (3, DEPTH, MAP, MAP)), bf16x3=bf16x3)
        self.centermap_parser = CenterMap3D(center_thresh)
        self.range_guard = RangeGuard(self.net)                # default-on, as in ROMP (net.RangeGuard)
        f = lambda k: state_dict[k].detach().float()
        dv = lambda t: t.contiguous().to(self.device)
        self.emb = dv(f('position_embeddings.weight'))
        self.w1t, self.b1 = dv(f('transformer.0.weight').t()), dv(f('transformer.0.bias'))      # [in][out]
        self.w2t, self.b2 = dv(f('transformer.3.weight').t()), dv(f('transformer.3.bias'))
        self.w3t, self.b3 = dv(f('transformer.6.weight').t()), dv(f('transformer.6.bias'))
        self.anchors = (C.c_float * DEPTH)(*cam3dmap_anchor(60, MAP).tolist())

    def localization(self, images):
        """coarse2fine_localization: -> center_maps_3d (B,64,128,128), cam_maps_3d (B,3,64,128,128)."""
        return self.net.forward_nhwc(images)

    @torch.no_grad()
    def __call__(self, images):
        """images (B,512,512,3) float on device -> dict like BEVv1.forward (:247-249) or None."""
        lib = L.load()
        net = self.net
        c3d, cam3d = self.localization(images)
        bids, czyx, confs = self.centermap_parser.parse_3dcentermap(c3d)
        # range guard: the parse has just synchronised on the count, so the network is done -- one 4-byte read of its saturation
        # counter; if it moved, the whole call again on the exact-f32 program (whose front-view features the regression then reads)
        if self.range_guard.enabled and self.range_guard.check(net.saturated):
            net = self.net.f32_twin()
            c3d, cam3d = net.forward_nhwc(images)
            self.range_guard.warn(images)
            bids, czyx, confs = self.centermap_parser.parse_3dcentermap(c3d)
        N = bids.shape[0]
        if N == 0:
            print('No person detected!')
            return None
        dev = self.device
        f32 = dict(device=dev, dtype=torch.float32)
        out = {'params_pred': torch.empty(N, 146, **f32), 'cam': torch.empty(N, 3, **f32),
               'smpl_thetas': torch.empty(N, 72, **f32), 'smpl_betas': torch.empty(N, 11, **f32),
               'cam_trans': torch.empty(N, 3, **f32)}
        cam_czyx = torch.empty(N, 3, device=dev, dtype=torch.int32)
        b32, z32 = bids.int().contiguous(), czyx.int().contiguous()
        P = net.program
        feat_ptr = net.buffer_ptr(P.fv_buf) + 4 * P.fv_coff
        with torch.cuda.device(dev):
            L.check(lib.romp_bev_regress(L.ptr(cam3d), C.c_void_p(feat_ptr), P.fv_cstride, N, L.ptr(b32), L.ptr(z32),
                                         self.anchors, L.ptr(self.emb), L.ptr(self.w1t), L.ptr(self.b1), L.ptr(self.w2t),
                                         L.ptr(self.b2), L.ptr(self.w3t), L.ptr(self.b3), L.ptr(out['params_pred']),
                                         L.ptr(cam_czyx), L.ptr(out['cam']), L.ptr(out['smpl_thetas']),
                                         L.ptr(out['smpl_betas']), L.ptr(out['cam_trans']), L.stream_ptr(dev)))
        out.update({'cam_czyx': cam_czyx.float(), 'center_map_3d': c3d, 'cam_maps_3d': cam3d, 'pred_batch_ids': bids,
                    'pred_czyxs': czyx, 'center_confs': confs})
        return out


class SMPLA_parser(nn.Module):
    """bev/post_parser.py:255-278: SMPL-A for adults, SMIL for betas[:,10] > 0.8, always root-aligned."""

    def __init__(self, smpla_path, smil_path):
        super(SMPLA_parser, self).__init__()
        self.smil_model = SMPL(smil_path, model_type='smpl')
        self.smpl_model = SMPL(smpla_path, model_type='smpla')
        self.baby_thresh = 0.8

    def forward(self, betas=None, thetas=None, root_align=True):
        baby_mask = betas[:, 10] > self.baby_thresh
        if baby_mask.sum() > 0:
            adult_mask = ~baby_mask
            n = len(thetas)
            verts = torch.zeros(n, 6890, 3, device=thetas.device)
            joints = torch.zeros(n, 71, 3, device=thetas.device)
            verts[baby_mask], joints[baby_mask], face = self.smil_model(betas[baby_mask, :10].contiguous(),
                                                                        thetas[baby_mask].contiguous(), root_align=root_align)
            if adult_mask.sum() > 0:
                verts[adult_mask], joints[adult_mask], face = self.smpl_model(betas[adult_mask].contiguous(),
                                                                              thetas[adult_mask].contiguous(),
                                                                              root_align=root_align)
        else:
            verts, joints, face = self.smpl_model(betas, thetas, root_align=root_align)
        return verts, joints, face


class BEV(nn.Module):
    def __init__(self, settings, state_dict=None, smpla_model=None, smil_model=None):
        super(BEV, self).__init__()
        self.settings = settings
        if settings.GPU == -1:
            raise L.RompHipError('romp_amd.bev needs a HIP device; there is no CPU fallback')
        self.tdevice = determine_device(settings.GPU)
        if state_dict is None:
            state_dict = torch.load(settings.model_path, map_location='cpu')
        self.model = BEVv1(state_dict, self.tdevice, center_thresh=settings.center_thresh,
                           max_batch=getattr(settings, 'max_batch', 32),
                           bf16x3=getattr(settings, 'conv_math', 'f16x2'))
        if settings.calc_smpl or settings.crowd:                           # (crowd mode merges on the meshes' joints)
            self.smpl_parser = SMPLA_parser(smpla_model if smpla_model is not None else settings.smpl_path,
                                            smil_model if smil_model is not None else settings.smil_path).to(self.tdevice)
        self.result_keys = ['smpl_thetas', 'smpl_betas', 'cam', 'cam_trans', 'params_pred', 'center_confs', 'pred_batch_ids']
        if settings.temporal_optimize:                                                      # bev/main.py:117-121
            self.OE_filters = {}
            if not settings.show_largest and getattr(settings, 'device_tracker', False):
                self.device_smoothers = {}                                                  # signal_ID -> tracking.TrackedSmoother
            elif not settings.show_largest:
                from .tracker import Tracker
                self.tracker = Tracker(det_thresh=0.12, low_conf_det_thresh=0.05, track_buffer=60, match_thresh=300, frame_rate=30)
        if settings.render_mesh:                                                            # bev/main.py:112-114
            from .vis import setup_renderer
            self.renderer = setup_renderer(name=getattr(settings, 'renderer', 'sim3dr'), device=self.tdevice)
            self.visualize_items = getattr(settings, 'show_items', 'mesh').split(',')
        elif getattr(settings, 'dense_maps', False):
            from .vis import setup_renderer
            self.renderer = setup_renderer(device=self.tdevice)

    def temporal_optimization(self, outputs, signal_ID, image_scale=128, depth_scale=30):
        """bev/main.py:260-287: ByteTrack-3D association on the host (tracker.py), OneEuro filters on the device (temporal.py).
        Returns None when no confirmed track is seen in the frame."""
        from .temporal import OneEuroBank
        if signal_ID not in self.OE_filters:                                                # check_filter_state (utils.py:246-255)
            if len(self.OE_filters) > 100:
                self.OE_filters.clear()
            self.OE_filters[signal_ID] = OneEuroBank(self.tdevice, getattr(self.settings, 'smooth_coeff', 3.), outputs['smpl_betas'].shape[1])
        bank = self.OE_filters[signal_ID]
        if self.settings.show_largest:
            max_id = int(torch.argmax(outputs['cam'][:, 0]))
            th, be, ca = (outputs[k][max_id:max_id + 1].contiguous().clone() for k in ('smpl_thetas', 'smpl_betas', 'cam'))
            outputs['smpl_thetas'], outputs['smpl_betas'], outputs['cam'] = bank.smooth([0], th, be, ca)
            return outputs
        if getattr(self.settings, 'device_tracker', False):
            return BEV._temporal_optimization_device(self, outputs, signal_ID, image_scale, depth_scale)
        cams = outputs['cam'].cpu().numpy()
        cam_trans = outputs['cam_trans'].cpu().numpy()
        det_confs = outputs['center_confs'].cpu().numpy()
        tracking_points = np.concatenate([(cams[:, [2, 1]] + 1) * image_scale, cam_trans[:, [2]] * depth_scale,
                                          cams[:, [0]] * image_scale / 2], 1)
        tracked_ids, results_inds = self.tracker.update(tracking_points, det_confs)
        if len(tracked_ids) == 0:
            return None
        rows = torch.as_tensor(results_inds, dtype=torch.long, device=self.tdevice)
        for key in self.result_keys:
            outputs[key] = outputs[key][rows].contiguous()
        outputs['smpl_thetas'], outputs['smpl_betas'], outputs['cam'] = bank.smooth(tracked_ids, outputs['smpl_thetas'],
                                                                                    outputs['smpl_betas'], outputs['cam'])
        outputs['track_ids'] = np.array(tracked_ids).astype(np.int32)
        return outputs

    def _temporal_optimization_device(self, outputs, signal_ID, image_scale=128, depth_scale=30):
        """--device_tracker: the association on the device as well (tracking.py): the tracking points are built there, one launch
        tracks, one launch filters, every other entry is gathered with the padded device rows, and ONE download (count and ids) tells
        how far to narrow them.  Each signal_ID has its own tracker state, ids counted from 1."""
        from .tracking import TrackedSmoother, bev_tracking_points
        if signal_ID not in self.device_smoothers:
            if len(self.device_smoothers) > 100:
                self.device_smoothers.clear()
            self.device_smoothers[signal_ID] = TrackedSmoother(self.tdevice, getattr(self.settings, 'smooth_coeff', 3.), outputs['smpl_betas'].shape[1],
                                                               det_thresh=0.12, low_conf_det_thresh=0.05, track_buffer=60, match_thresh=300,
                                                               frame_rate=30)
        sm = self.device_smoothers[signal_ID]
        points = bev_tracking_points(outputs['cam'], outputs['cam_trans'], image_scale, depth_scale)
        buf, _, _, rows, _, th, be, ca = sm.run(points, outputs['center_confs'].float(), outputs['smpl_thetas'], outputs['smpl_betas'], outputs['cam'])
        rows = rows[0].long()
        gathered = {key: outputs[key][rows] for key in self.result_keys if key not in ('smpl_thetas', 'smpl_betas', 'cam')}
        counts, ids = sm.download(buf, 1, sm.capacity)                                      # the one synchronisation
        n = int(counts[0])
        if n == 0:
            return None
        for key, v in gathered.items():
            outputs[key] = v[:n]
        outputs['smpl_thetas'], outputs['smpl_betas'], outputs['cam'] = th[:n], be[:n], ca[:n]
        outputs['track_ids'] = ids[0, :n].astype(np.int32)
        return outputs

    @torch.no_grad()
    def forward_batch(self, images, pad_infos=None):
        """[extension] images (B,512,512,3) float on device -> dict of device tensors or None.
        With `pad_infos` (B,6) the per-image post-processing of process_normal_image (bev/main.py:168-180)
        runs too: projection, duplicate suppression, outlier removal (rows of dropped persons removed)."""
        out = self.model(images)
        if out is None:
            return None
        res = {k: out[k] for k in self.result_keys}
        if self.settings.calc_smpl:
            verts, joints, face = self.smpl_parser(res['smpl_betas'], res['smpl_thetas'])
            res.update({'verts': verts, 'joints': joints})
            if pad_infos is not None:
                res = self._postprocess(res, images.shape[0], pad_infos)
        return res

    def _postprocess(self, res, B, pad_infos):
        lib = L.load()
        dev = self.tdevice
        N = res['cam'].shape[0]
        counts = torch.bincount(res['pred_batch_ids'], minlength=B)
        offsets = torch.zeros(B + 1, dtype=torch.int32, device=dev)
        offsets[1:] = torch.cumsum(counts, 0).int()
        pads = torch.as_tensor(pad_infos, dtype=torch.float32).reshape(B, 6).to(dev).contiguous()
        pj = torch.empty(N, 71, 2, device=dev)
        pjo = torch.empty(N, 71, 2, device=dev)
        tr = torch.empty(N, 3, device=dev)
        keep = torch.empty(N, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            L.check(lib.romp_bev_postprocess(L.ptr(res['joints'].contiguous()), L.ptr(res['cam'].contiguous()), L.ptr(offsets),
                                             B, L.ptr(pads), float(self.settings.nms_thresh),
                                             float(self.settings.relative_scale_thresh), L.ptr(pj), L.ptr(pjo), L.ptr(tr),
                                             L.ptr(keep), L.stream_ptr(dev)))
        res.update({'cam_trans': tr, 'pj2d': pjo, 'pj2d_org': pjo})       # the reference aliases pj2d to pj2d_org
        mask = keep.bool()
        mask_np = None
        out = {}
        for k, v in res.items():                        # remove_subjects (bev/post_parser.py:154-165): every per-person entry
            if torch.is_tensor(v) and v.shape[:1] == (N,) and k != 'smpl_face':
                v = v[mask]
            elif isinstance(v, np.ndarray) and v.shape[:1] == (N,):
                mask_np = mask.cpu().numpy() if mask_np is None else mask_np
                v = v[mask_np]
            out[k] = v
        return out

    @torch.no_grad()
    def process_long_image(self, full_image, show_patch_results=False):
        """bev/main.py:184-258: BGR uint8 HxWx3 frame -> dict of device tensors (the merged people of all crops) or None.
        show_patch_results is not supported (ignored)."""
        lib = L.load()
        dev = self.tdevice
        H, W = full_image.shape[:2]
        pad_length = crowd_pad_length(H, self.settings.overlap_ratio)
        crops = np.ascontiguousarray(crowd_split_plan(H, W + 2 * pad_length, self.settings.overlap_ratio), np.int32)
        K = crops.shape[0]
        crops_c = crops.ctypes.data_as(C.POINTER(C.c_int32))
        img = torch.from_numpy(np.ascontiguousarray(full_image)).to(dev)
        assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3
        inputs = torch.empty(K, 512, 512, 3, device=dev, dtype=torch.float32)
        with torch.cuda.device(dev):
            L.check(lib.romp_preprocess_crops(L.ptr(img), H, W, pad_length, K, crops_c, L.ptr(inputs), 512, None,
                                              L.stream_ptr(dev)))
        parts = []
        step = self.model.net.max_batch
        for s in range(0, K, step):                                         # the network in chunks of max_batch crops
            out = self.model(inputs[s:s + step])
            if out is not None:
                part = {k: out[k] for k in self.result_keys}
                part['pred_batch_ids'] = out['pred_batch_ids'] + s          # -> crop index
                parts.append(part)
        if not parts:
            return None
        res = {k: torch.cat([p[k] for p in parts]) if len(parts) > 1 else parts[0][k] for k in self.result_keys}
        crop_ids = res.pop('pred_batch_ids')
        N = crop_ids.shape[0]
        verts, joints, face = self.smpl_parser(res['smpl_betas'], res['smpl_thetas'])
        offsets = torch.zeros(K + 1, dtype=torch.int32, device=dev)
        offsets[1:] = torch.cumsum(torch.bincount(crop_ids, minlength=K), 0).int()
        f32 = dict(device=dev, dtype=torch.float32)
        cam, trans, pjo = torch.empty(N, 3, **f32), torch.empty(N, 3, **f32), torch.empty(N, 71, 2, **f32)
        keep = torch.empty(N, dtype=torch.int32, device=dev)
        ws = torch.empty(4 * N + 4, dtype=torch.int32, device=dev)
        joints, crop_cam, confs = joints.contiguous(), res['cam'].contiguous(), res['center_confs'].contiguous()
        with torch.cuda.device(dev):
            L.check(lib.romp_bev_crowd_merge(L.ptr(joints), L.ptr(crop_cam), L.ptr(confs), L.ptr(offsets), N, N, K, crops_c, H, W,
                                             pad_length, float(self.settings.nms_thresh),
                                             float(self.settings.relative_scale_thresh), L.ptr(cam), L.ptr(trans), L.ptr(pjo),
                                             L.ptr(keep), L.ptr(ws), L.stream_ptr(dev)))
        rows = torch.nonzero(keep).squeeze(1)                               # the one host synchronisation of the merge
        n = rows.shape[0]
        if n == 0:
            return None
        out = {k: res[k][rows] for k in ('smpl_thetas', 'smpl_betas')}
        out.update({'cam': cam[rows], 'cam_trans': trans[rows], 'params_pred': res['params_pred'][rows],
                    'center_confs': res['center_confs'][rows],
                    'pred_batch_ids': torch.zeros(n, dtype=torch.int64, device=dev),   # every crop was a B = 1 forward there
                    'verts': verts[rows], 'joints': joints[rows], 'pj2d_org': pjo[rows], 'smpl_face': face})
        return out

    def forward(self, image, signal_ID=0, **kwargs):
        """bev/main.py:139-181: BGR uint8 HxWx3 -> dict of numpy arrays or None.  With --crowd, a frame with W / H >= 2 takes
        process_long_image (no tracking / filtering, no --show_largest there, as in the reference)."""
        if self.settings.crowd and image.shape[1] / image.shape[0] >= 2:
            res = self.process_long_image(image)
            if res is None:
                return None
            H, W = image.shape[:2]
            return convert_tensor2numpy(self._visualize(res, image, crowd_pad_info(H, W)))
        input_image, image_pad_info = img_preprocess_device(image, self.tdevice)
        if not (self.settings.temporal_optimize or self.settings.render_mesh or getattr(self.settings, 'dense_maps', False)):
            res = self.forward_batch(input_image, image_pad_info.reshape(1, 6))
            return None if res is None else convert_tensor2numpy(res)
        out = self.model(input_image)
        if out is None:
            return None
        res = {k: out[k] for k in self.result_keys}
        if self.settings.temporal_optimize:                                                 # bev/main.py:162-166
            res = self.temporal_optimization(res, signal_ID)
            if res is None:
                return None
            res['cam_trans'] = denormalize_cam_params_to_trans(res['cam'])
        if self.settings.calc_smpl:
            verts, joints, face = self.smpl_parser(res['smpl_betas'], res['smpl_thetas'])
            res.update({'verts': verts, 'joints': joints, 'smpl_face': face})
            res = self._postprocess(res, 1, image_pad_info.reshape(1, 6))
            res = self._visualize(res, image, image_pad_info)
        return convert_tensor2numpy(res)

    def _visualize(self, res, image, pad_info):
        """--render_mesh (bev/main.py:147-150) and --dense_maps on the meshes of one frame; with both, the 'mesh' panel's raster
        pass serves the maps too.  The part labels are the adult model's (SMPL-A) table for every person, infants included:
        SMIL shares SMPL's topology, so one table indexes every mesh; a per-person SMIL table is not kept."""
        dense = getattr(self.settings, 'dense_maps', False)
        if not (self.settings.render_mesh or dense):
            return res
        from .vis import dense_maps, mesh_panel_keys, rendering_romp_bev_results
        res['verts_camed_org'] = self._verts_camed_org(res['verts'], res['cam_trans'], pad_info)
        keys = None
        if self.settings.render_mesh:
            keys = mesh_panel_keys(image.shape, self.tdevice) if dense and 'mesh' in self.visualize_items else None
            cfgs = {'mesh_color': getattr(self.settings, 'mesh_color', 'identity'), 'items': self.visualize_items,
                    'renderer': getattr(self.settings, 'renderer', 'sim3dr'), 'part_labels': self.smpl_parser.smpl_model.part_labels,
                    'rotate_size': getattr(self.settings, 'rotate_size', 512)}
            res = rendering_romp_bev_results(self.renderer, res, image, cfgs, keys=keys)
        if dense:
            res = dense_maps(self.renderer, res, image.shape, self.smpl_parser.smpl_model.part_labels, keys=keys)
        return res

    def _verts_camed_org(self, verts, cam_trans, pad_info):
        lib = L.load()
        v = verts.contiguous().float()
        org = torch.empty_like(v)
        pad_c = (C.c_float * 6)(*[float(x) for x in pad_info])
        with torch.cuda.device(self.tdevice):
            L.check(lib.romp_bev_project_verts(L.ptr(v), v.shape[0], v.shape[1], L.ptr(cam_trans.contiguous().float()), pad_c,
                                               L.ptr(org), L.stream_ptr(self.tdevice)))
        return org
