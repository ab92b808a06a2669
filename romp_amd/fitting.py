"""[romp_amd] Fitting the SMPL layer to 2-D keypoints on the device (include/romp_hip_fit.h, csrc/fit.hip).

The reference has no counterpart: it regresses the parameters and stops.  A ROMP / BEV result can be refined here against a
detector's keypoints or annotations, with the project's own camera conventions:

  ``reprojection_loss``  an autograd node around ``romp_fit_reproject`` (loss and gradients in one launch); composes with
                         ``romp_amd.smpl.SMPL`` and any torch optimiser.
  ``KeypointFitter``     the whole loop without autograd and without a host round trip: per step ``smpl_forward``,
                         ``romp_fit_reproject``, ``smpl_backward`` (joint gradients only) and ``romp_fit_adam``, i.e. the
                         layer's own launches plus two.
  ``refine_outputs``     the same for the dict a ``ROMP`` / ``BEV`` forward returns and keypoints in original-image pixels.

The loss, per person:  sum over visible keypoints of conf^2 rho(|proj(joint) - keypoint|^2) / (n_visible + 1e-4), with
rho(e) = e or, for sigma > 0, Geman-McClure sigma^2 e / (sigma^2 + e).  The visibility rule (conf > 0, both coordinates
> -1.99) and the normaliser are the reference's (loss_funcs/keypoints_loss.py:24,38); the distance is squared, unlike the
reference's unsquared norm, which has no gradient at a perfect fit.  camera 'weak': cam = (s, c1, c2), u = s x + c1,
v = s y + c2 (batch_orth_proj); 'perspective': cam = cam_trans, p = X + cam, u = p.x / (p.z + 1e-6) * focal / half
(BEV's perspective_projection, as ``romp_bev_project_verts``).  Coordinates are the network's normalised frame (-1..1).
"""
import ctypes as C

import numpy as np
import torch

from . import lib as L

CAMERAS = {'weak': 0, 'perspective': 1}


def _mode(camera):
    if camera not in CAMERAS:
        raise ValueError("camera must be 'weak' or 'perspective', not %r" % (camera,))
    return CAMERAS[camera]


def _inds(joint_inds, K):
    """-> ctypes int32 array of K joint indices, or None.  The C side checks range and repeats."""
    if joint_inds is None:
        return None
    idx = [int(i) for i in (joint_inds.tolist() if hasattr(joint_inds, 'tolist') else joint_inds)]
    if len(idx) != K:
        raise ValueError('joint_inds names %d joints for %d keypoints' % (len(idx), K))
    return (C.c_int32 * K)(*idx)


def _f32(t, dev):
    return torch.as_tensor(t).to(dev).float().contiguous()


def _reproject(joints, cam, kp2d, conf, inds_c, mode, focal, half, sigma, loss, gj, gc, history=None, row=0):
    dev = joints.device
    if dev.type != 'cuda':
        raise L.RompHipError('the reprojection loss runs on the HIP device only (no CPU fallback); move the tensors to "cuda:N"')
    N, J = joints.shape[:2]
    K = kp2d.shape[1]
    with torch.cuda.device(dev):
        L.check(L.load().romp_fit_reproject(L.ptr(joints), N, J, L.ptr(cam), L.ptr(kp2d), L.ptr(conf), K, inds_c, mode,
                                            float(focal), float(half), float(sigma), L.ptr(loss), L.ptr(gj), L.ptr(gc),
                                            L.ptr(history), int(row), L.stream_ptr(dev)))


class _ReprojectFunction(torch.autograd.Function):
    """romp_fit_reproject as an autograd node: the forward launch leaves both gradients, the backward scales them."""

    @staticmethod
    def forward(ctx, joints, cam, kp2d, conf, inds_c, mode, focal, half, sigma):
        loss = torch.empty(joints.shape[0], device=joints.device, dtype=torch.float32)
        gj, gc = torch.empty_like(joints), torch.empty_like(cam)
        _reproject(joints, cam, kp2d, conf, inds_c, mode, focal, half, sigma, loss, gj, gc)
        ctx.save_for_backward(gj, gc)
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        gj, gc = ctx.saved_tensors
        g = grad_loss.to(gj.device).float()
        need_j, need_c = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        return (gj * g[:, None, None] if need_j else None, gc * g[:, None] if need_c else None,
                None, None, None, None, None, None, None)


def reprojection_loss(joints, cam, kp2d, conf=None, joint_inds=None, sigma=0., camera='weak', focal=443.4, half=256.):
    """joints (N,J,3), cam (N,3), kp2d (N,K,2) in the normalised frame, conf (N,K) or None, joint_inds: K distinct joint
    indices or None (= the first K joints) -> loss (N,), differentiable in joints and cam."""
    dev = joints.device
    joints, cam, kp2d = _f32(joints, dev), _f32(cam, dev), _f32(kp2d, dev)
    conf = None if conf is None else _f32(conf, dev)
    if joints.dim() != 3 or joints.shape[2] != 3 or cam.shape != (joints.shape[0], 3) or kp2d.dim() != 3 or \
            kp2d.shape[0] != joints.shape[0] or kp2d.shape[2] != 2 or (conf is not None and conf.shape != kp2d.shape[:2]):
        raise ValueError('reprojection_loss: joints (N,J,3), cam (N,3), kp2d (N,K,2), conf (N,K)')
    inds_c = _inds(joint_inds, kp2d.shape[1])
    return _ReprojectFunction.apply(joints, cam, kp2d, conf, inds_c, _mode(camera), focal, half, sigma)


class KeypointFitter(object):
    """Adam on (betas, poses, cam) against 2-D keypoints, every step on the device:

        fitter = KeypointFitter(smpl, camera='weak', steps=30, lr=0.02)
        res = fitter.fit(betas0, poses0, cam0, kp2d, conf)       # dict: betas, poses, cam, verts, joints, loss_history

    smpl: a ``romp_amd.smpl.SMPL`` on the device.  The priors are L2 with per-column weights, added to the gradient inside the
    Adam launch:  w_betas |betas|^2  keeps the shape small,  w_pose |poses - poses0|^2  holds the pose near the start, the
    global orientation (columns 0-2) excepted.  Each weight is a number or a vector with one entry per column.
    ``loss_history`` (steps + 1, N) holds the data term before every step and after the last; it stays on the device."""

    def __init__(self, smpl, camera='weak', steps=30, lr=0.02, sigma=0., w_betas=1e-4, w_pose=1e-4, root_align=False,
                 focal=443.4, half=256., betas=(0.9, 0.999), eps=1e-8):
        self.smpl, self.camera, self.mode = smpl, camera, _mode(camera)
        self.steps, self.lr, self.sigma = int(steps), float(lr), float(sigma)
        self.w_betas, self.w_pose, self.root_align = w_betas, w_pose, bool(root_align)
        self.focal, self.half, self.adam_betas, self.eps = float(focal), float(half), (float(betas[0]), float(betas[1])), float(eps)
        if self.steps < 0:
            raise ValueError('steps must not be negative')

    @staticmethod
    def _weights(w, cols, dev, free=0):
        """A prior weight as a (cols,) device vector, the first `free` columns zero when it was given as a number."""
        if w is None:
            return None
        if np.ndim(w) == 0 and not torch.is_tensor(w):
            out = torch.full((cols,), float(w), dtype=torch.float32)
            out[:free] = 0
            return out.to(dev)
        out = _f32(w, dev).reshape(-1)
        if out.numel() != cols:
            raise ValueError('a prior weight vector needs %d entries, got %d' % (cols, out.numel()))
        return out

    def start(self, betas0, poses0, cam0, kp2d, conf=None, joint_inds=None):
        """The buffers of one fit and its two halves of a step (``_FitRun``); ``fit`` drives it."""
        return _FitRun(self, betas0, poses0, cam0, kp2d, conf, joint_inds)

    def fit(self, betas0, poses0, cam0, kp2d, conf=None, joint_inds=None):
        """betas0 (N,n_betas), poses0 (N,72), cam0 (N,3) (`cam` or `cam_trans`, by the camera), kp2d (N,K,2) in the normalised
        frame, conf (N,K) or None, joint_inds: K joint indices of the 71 or None (= the first K).  The inputs are not changed.
        -> dict(betas, poses, cam, verts, joints, loss_history (steps + 1, N)), device tensors; nothing is downloaded."""
        run = self.start(betas0, poses0, cam0, kp2d, conf, joint_inds)
        for s in range(self.steps):
            run.evaluate(s)
            run.update(s + 1)
        run.evaluate(self.steps)
        return {'betas': run.betas, 'poses': run.poses, 'cam': run.cam, 'verts': run.verts, 'joints': run.joints,
                'loss_history': run.history}


class _FitRun(object):
    """Device buffers of one KeypointFitter.fit and the two halves of a step.  evaluate(row): smpl_forward and
    romp_fit_reproject (loss into history[row], joint and camera gradients); update(step): smpl_backward from the joint
    gradients alone and romp_fit_adam over betas, poses and cam (step counts from 1)."""

    def __init__(self, fitter, betas0, poses0, cam0, kp2d, conf, joint_inds):
        self.fitter, smpl = fitter, fitter.smpl
        self.dev = dev = smpl.shapedirs.device
        self.ctx = smpl._context()                                   # raises without a HIP device
        self.h = L.load()
        self.betas, self.poses, self.cam = (_f32(t, dev).detach().clone() for t in (betas0, poses0, cam0))
        self.kp2d = _f32(kp2d, dev)
        self.conf = None if conf is None else _f32(conf, dev)
        N, nb = self.betas.shape
        if self.poses.shape != (N, 72) or self.cam.shape != (N, 3) or self.kp2d.dim() != 3 or self.kp2d.shape[0] != N or \
                self.kp2d.shape[2] != 2 or (self.conf is not None and self.conf.shape != self.kp2d.shape[:2]):
            raise ValueError('fit: betas (N,n_betas), poses (N,72), cam (N,3), kp2d (N,K,2), conf (N,K)')
        self.N, self.nb = N, nb
        self.inds_c = _inds(joint_inds, self.kp2d.shape[1])
        f32 = dict(device=dev, dtype=torch.float32)
        self.verts, self.joints = torch.empty(N, 6890, 3, **f32), torch.empty(N, 71, 3, **f32)
        self.loss, self.gj, self.gc = torch.empty(N, **f32), torch.empty(N, 71, 3, **f32), torch.empty(N, 3, **f32)
        self.gb, self.gp = torch.empty_like(self.betas), torch.empty_like(self.poses)
        self.history = torch.empty(fitter.steps + 1, N, **f32)
        self.state = torch.zeros(2, N * (nb + 72 + 3), **f32)        # Adam's m and v of the three tensors
        self.poses_ref = self.poses.clone()
        self.wb = fitter._weights(fitter.w_betas, nb, dev)
        self.wp = fitter._weights(fitter.w_pose, 72, dev, free=3)
        self.segs, at = (L.FitSegment * 3)(), 0
        for i, (p, g, ref, w) in enumerate(((self.betas, self.gb, None, self.wb), (self.poses, self.gp, self.poses_ref, self.wp),
                                            (self.cam, self.gc, None, None))):
            n = p.numel()
            m, v = self.state[0, at:at + n], self.state[1, at:at + n]
            at += n
            self.segs[i] = L.FitSegment(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(),
                                        None if ref is None or w is None else ref.data_ptr(), None if w is None else w.data_ptr(),
                                        N, p.shape[1])

    def evaluate(self, row):
        f, ra = self.fitter, int(self.fitter.root_align)
        with torch.cuda.device(self.dev):
            L.check(self.h.smpl_forward(self.ctx, L.ptr(self.betas), self.nb, L.ptr(self.poses), self.N, ra, L.ptr(self.verts),
                                        L.ptr(self.joints), L.stream_ptr(self.dev)))
        _reproject(self.joints, self.cam, self.kp2d, self.conf, self.inds_c, f.mode, f.focal, f.half, f.sigma, self.loss, self.gj,
                   self.gc, self.history, row)

    def update(self, step):
        f, ra = self.fitter, int(self.fitter.root_align)
        with torch.cuda.device(self.dev):
            st = L.stream_ptr(self.dev)
            L.check(self.h.smpl_backward(self.ctx, L.ptr(self.betas), self.nb, L.ptr(self.poses), self.N, ra, None, L.ptr(self.gj),
                                         L.ptr(self.gb), L.ptr(self.gp), st))
            L.check(self.h.romp_fit_adam(self.segs, 3, f.lr, f.adam_betas[0], f.adam_betas[1], f.eps, int(step), st))


def keypoints_to_input_frame(kp2d_org, pad_info):
    """Original-image pixels -> the network's normalised frame: the inverse of convert_proejection_from_input_to_orgimg
    (post_parser.py:81-88), x = (x_org + left) * 2 / max(h, w) - 1, y with `top`.  pad_info = top, bottom, left, right, h, w."""
    top, _, left, _, h, w = [float(v) for v in pad_info]
    size = max(h, w)
    off = torch.tensor([left, top], dtype=torch.float32, device=kp2d_org.device)
    return (kp2d_org + off) * (2. / size) - 1.


def refine_outputs(model, outputs, kp2d_org, conf=None, joint_inds=None, pad_info=None, **fit_args):
    """Refine the result dict of a ``ROMP`` / ``BEV`` forward against keypoints in original-image pixels.

    outputs: the dict of ``forward`` / ``forward_batch`` (numpy arrays or tensors) with smpl_betas, smpl_thetas and cam
    (ROMP) or cam_trans (BEV); kp2d_org (N,K,2), conf (N,K) or None, row for row with the dict's persons (matching detections
    to annotations is the caller's job: ``evaluation.match_2d_greedy``).  pad_info: the (top, bottom, left, right, h, w) of the
    frame's pre-processing; None means a 512 x 512 frame without padding.  fit_args go to ``KeypointFitter``.

    ROMP is fitted with the weak-perspective camera `cam`; BEV with the perspective camera `cam_trans`, always root-aligned,
    infants (betas[:, 10] > 0.8) on the SMIL layer as in BEV's own parser (one host read of that mask, as there); BEV's `cam`
    stays the network's.  Returns a copy of
    the dict, device tensors, with smpl_thetas, smpl_betas, cam / cam_trans, verts, joints, pj2d, pj2d_org rewritten (by
    ``romp_project`` / ``romp_bev_project_verts``) and fit_loss (N,2): the loss before and after."""
    from .post_parser import body_mesh_projection2image
    parser = getattr(model, 'smpl_parser', None)
    if parser is None:
        raise L.RompHipError('refine_outputs needs a model built with calc_smpl')
    is_bev = hasattr(parser, 'smil_model')                            # bev.SMPLA_parser; post_parser.SMPL_parser has one layer
    dev = model.tdevice
    pad = [0., 512., 0., 512., 512., 512.] if pad_info is None else [float(v) for v in np.asarray(pad_info).reshape(-1)]
    betas, thetas = _f32(outputs['smpl_betas'], dev), _f32(outputs['smpl_thetas'], dev)
    kp = keypoints_to_input_frame(_f32(kp2d_org, dev), pad)
    conf = None if conf is None else _f32(conf, dev)
    N = betas.shape[0]
    out = dict(outputs)
    if not is_bev:
        fitter = KeypointFitter(parser.smpl_model, camera='weak', **dict(dict(root_align=model.settings.root_align), **fit_args))
        res = fitter.fit(betas, thetas, _f32(outputs['cam'], dev), kp, conf, joint_inds)
        proj = body_mesh_projection2image(res['joints'], res['cam'], input2org_offsets=pad)
        out.update({'smpl_betas': res['betas'], 'smpl_thetas': res['poses'], 'cam': res['cam'], 'cam_trans': proj['cam_trans'],
                    'verts': res['verts'], 'joints': res['joints'], 'pj2d': proj['pj2d'], 'pj2d_org': proj['pj2d_org'],
                    'fit_loss': res['loss_history'][[0, -1]].t().contiguous()})
        return out
    trans = _f32(outputs['cam_trans'], dev)
    args = dict(dict(root_align=True), **fit_args)
    baby = (betas[:, 10] > parser.baby_thresh).cpu() if betas.shape[1] == 11 else torch.zeros(N, dtype=torch.bool)
    groups = [(parser.smpl_model, torch.nonzero(~baby).squeeze(1), betas.shape[1])]
    if bool(baby.any()):
        groups.append((parser.smil_model, torch.nonzero(baby).squeeze(1), 10))
    new = {'smpl_betas': betas.clone(), 'smpl_thetas': thetas.clone(), 'cam_trans': trans.clone(),
           'verts': torch.empty(N, 6890, 3, device=dev), 'joints': torch.empty(N, 71, 3, device=dev),
           'fit_loss': torch.empty(N, 2, device=dev)}
    for layer, rows, nb in groups:
        if rows.numel() == 0:
            continue
        rows = rows.to(dev)
        res = KeypointFitter(layer, camera='perspective', **args).fit(betas[rows][:, :nb], thetas[rows], trans[rows], kp[rows],
                                                                      None if conf is None else conf[rows], joint_inds)
        new['smpl_betas'][rows, :nb] = res['betas']
        for key, val in (('smpl_thetas', res['poses']), ('cam_trans', res['cam']), ('verts', res['verts']), ('joints', res['joints']),
                         ('fit_loss', res['loss_history'][[0, -1]].t())):
            new[key][rows] = val
    org = torch.empty(N, 71, 3, device=dev)
    pad_c = (C.c_float * 6)(*pad)
    if N:
        with torch.cuda.device(dev):
            L.check(L.load().romp_bev_project_verts(L.ptr(new['joints']), N, 71, L.ptr(new['cam_trans']), pad_c, L.ptr(org), L.stream_ptr(dev)))
    pj = org[:, :, :2].contiguous()
    out.update(new)
    out.update({'pj2d': pj, 'pj2d_org': pj})                          # BEV aliases pj2d to pj2d_org (bev.py _postprocess)
    return out
