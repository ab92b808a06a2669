"""[romp_amd] Fitting the SMPL layer to 2-D keypoints on the device (include/romp_hip_fit.h, csrc/fit.hip), with SMPLify's pose
priors and 3-D joint targets as further terms (include/romp_hip_fit_priors.h, csrc/fit_priors.hip).

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

  ``PosePrior``          SMPLify's Gaussian mixture over the body pose (MaxMixturePrior, loss_funcs/prior_loss.py:160-247).
  ``pose_prior_loss``    autograd node around ``romp_fit_pose_prior``: the max-mixture term and the joint-angle prior.
  ``joints3d_loss``      autograd node around ``romp_fit_joints3d``: the distance to 3-D targets under the rule of calc_mpjpe /
                         align_by_parts (loss_funcs/keypoints_loss.py:64-82), squared and normalised as the 2-D term.
``KeypointFitter`` takes all three as further terms of its objective, one launch each per step.

Given the ``links`` of a tracked clip (``romp_amd.clip.clip_links``) ``KeypointFitter`` also ties a row to the rows of the same
track in the neighbouring frames: velocity and acceleration terms on joints, camera and betas and a first-order term on the
joint rotations (include/romp_hip_fit_clip.h, csrc/fit_clip.hip), two more launches per step.  ``romp_amd.clip`` holds the
links, the autograd nodes of these terms and ``refine_clip``.

Given the ``scene`` tables of a ``forward_batch`` (``romp_amd.scene.scene_groups``) ``KeypointFitter`` ties the persons of one
image together: a depth-order term from depth-layer labels and a sphere-proxy collision term between different persons
(include/romp_hip_fit_scene.h, csrc/fit_scene.hip), one more launch per step.  ``romp_amd.scene`` holds the tables, the sphere
table, the autograd nodes of these terms and ``refine_scene``.
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


class PosePrior(object):
    """SMPLify's Gaussian-mixture pose prior as romp_fit_pose_prior reads it (include/romp_hip_fit_priors.h).

    means (M,D), covars (M,D,D), weights (M,): the mixture over the body pose (D = 69 in SMPLify's gmm_08.pkl).  Built in
    float64 as MaxMixturePrior builds it (prior_loss.py:202-212): precisions = inv(covars), made symmetric as (P + P^T) / 2,
    nll_weights = weights / ((2 pi)^(69/2) * sqrtdet / min sqrtdet); kept as the float32 device tensors ``means`` (M,D),
    ``precisions`` (M,D,D) and ``offsets`` (M,) = -log(nll_weights)."""

    def __init__(self, means, covars, weights, device=None):
        means, covars, weights = (np.asarray(torch.as_tensor(a).detach().cpu().numpy(), dtype=np.float64) for a in (means, covars, weights))
        if means.ndim != 2 or covars.shape != (means.shape[0], means.shape[1], means.shape[1]) or weights.shape != (means.shape[0],):
            raise ValueError('PosePrior: means (M,D), covars (M,D,D), weights (M,)')
        if not 1 <= means.shape[1] <= 69 or not 1 <= means.shape[0] <= 16:
            raise ValueError('PosePrior: 1 <= D <= 69 and 1 <= M <= 16, got D %d, M %d' % (means.shape[1], means.shape[0]))
        prec = np.stack([np.linalg.inv(c) for c in covars])
        prec = 0.5 * (prec + prec.transpose(0, 2, 1))
        sqrdets = np.array([np.sqrt(np.linalg.det(c)) for c in covars])
        nll_weights = weights / ((2 * np.pi) ** (69 / 2.) * (sqrdets / sqrdets.min()))
        self._set(torch.from_numpy(means), torch.from_numpy(prec), torch.from_numpy(-np.log(nll_weights)), device)

    def _set(self, means, precisions, offsets, device):
        dev = torch.device('cpu' if device is None else device)
        self.means, self.precisions, self.offsets = (_f32(t, dev) for t in (means, precisions, offsets))
        return self

    @classmethod
    def from_file(cls, path, device=None):
        """SMPLify's gmm_XX.pkl (a pickled dict with means, covars, weights; latin1 encoding) or an .npz with the same keys."""
        gmm = np.load(path, allow_pickle=True, encoding='latin1')    # numpy unpickles what is neither .npy nor .npz
        return cls(gmm['means'], gmm['covars'], gmm['weights'], device)

    def to(self, device):
        return PosePrior.__new__(PosePrior)._set(self.means, self.precisions, self.offsets, device)

    def sliced(self, D):
        """The prior of the first D pose parameters: means[:, :D] and precisions[:, :D, :D], as merged_log_likelihood slices
        them for a shorter pose (prior_loss.py:233-237)."""
        return PosePrior.__new__(PosePrior)._set(self.means[:, :D], self.precisions[:, :D, :D], self.offsets, self.means.device)


def _pose_prior(poses, prior, w_gmm, w_angle, loss, best, gp, accumulate, history=None, row=0):
    dev = poses.device
    if dev.type != 'cuda':
        raise L.RompHipError('the pose prior runs on the HIP device only (no CPU fallback); move the tensors to "cuda:N"')
    M, D = (0, 69) if prior is None else prior.means.shape
    with torch.cuda.device(dev):
        L.check(L.load().romp_fit_pose_prior(L.ptr(poses), poses.shape[0], L.ptr(None if prior is None else prior.means),
                                             L.ptr(None if prior is None else prior.precisions),
                                             L.ptr(None if prior is None else prior.offsets), M, D, float(w_gmm), float(w_angle),
                                             L.ptr(loss), L.ptr(best), L.ptr(gp), int(accumulate), L.ptr(history), int(row),
                                             L.stream_ptr(dev)))


def _joints3d(joints, trans, targets, conf, inds_c, align_c, sigma, weight, loss, gj, gt, accumulate, history=None, row=0):
    dev = joints.device
    if dev.type != 'cuda':
        raise L.RompHipError('the 3-D joint loss runs on the HIP device only (no CPU fallback); move the tensors to "cuda:N"')
    N, J = joints.shape[:2]
    with torch.cuda.device(dev):
        L.check(L.load().romp_fit_joints3d(L.ptr(joints), N, J, L.ptr(trans), L.ptr(targets), L.ptr(conf), targets.shape[1], inds_c,
                                           align_c, 0 if align_c is None else len(align_c), float(sigma), float(weight), L.ptr(loss),
                                           L.ptr(gj), L.ptr(gt), int(accumulate), L.ptr(history), int(row), L.stream_ptr(dev)))


def _links(links, N, dev):
    """(prev, next) of ``romp_amd.clip.clip_links`` -> two contiguous int32 (N,) tensors on the device of the fit."""
    if not isinstance(links, (tuple, list)) or len(links) != 2:
        raise ValueError('links must be the pair (prev, next) of romp_amd.clip.clip_links')
    prev, nxt = (torch.as_tensor(t).to(dev).to(torch.int32).contiguous() for t in links)
    if prev.shape != (N,) or nxt.shape != (N,):
        raise ValueError('links: prev and next need one entry per row (%d), got %s and %s' % (N, tuple(prev.shape), tuple(nxt.shape)))
    return prev, nxt


def _clip_segment(x, grad, col_w=None, w_vel=0., w_acc=0., sigma_vel=0., sigma_acc=0., accumulate=0):
    """One linear block of romp_fit_temporal: x and grad (N, ...) float32 device tensors, read as (N, cols)."""
    return L.ClipSegment(x.data_ptr(), grad.data_ptr(), None if col_w is None else col_w.data_ptr(), int(np.prod(x.shape[1:])),
                         float(w_vel), float(w_acc), float(sigma_vel), float(sigma_acc), int(accumulate))


def _temporal(segs, links, N, loss, poses=None, joint_w=None, w_rot=0., sigma_rot=0., gp=None, accumulate=0, history=None, row=0,
              term_w=None):
    """romp_fit_temporal: segs a ctypes array of ``L.ClipSegment`` (or None), links = (prev, next) on the device."""
    dev = loss.device
    if dev.type != 'cuda':
        raise L.RompHipError('the temporal terms run on the HIP device only (no CPU fallback); move the tensors to "cuda:N"')
    with torch.cuda.device(dev):
        L.check(L.load().romp_fit_temporal(segs, 0 if segs is None else len(segs), L.ptr(links[0]), L.ptr(links[1]), int(N),
                                           L.ptr(term_w), L.ptr(poses), L.ptr(joint_w), float(w_rot), float(sigma_rot), L.ptr(gp),
                                           int(accumulate), L.ptr(loss), L.ptr(history), int(row), L.stream_ptr(dev)))


def _fit_scene(joints, cam, mode, groups, depth_ids, w_depth, thresh, kind, table, radius_scale, w_col, term_w, gj, acc_j, gc, acc_c,
               loss, history=None, row=0):
    """romp_fit_scene: groups = (offsets, members) on the device, table a ctypes array of ``L.SceneSphere`` (or None: no
    collision term; joints and gj may be None then), depth_ids int32 (N,) or None (no depth term)."""
    dev = cam.device
    if dev.type != 'cuda':
        raise L.RompHipError('the scene terms run on the HIP device only (no CPU fallback); move the tensors to "cuda:N"')
    N, J = cam.shape[0], 0 if joints is None else joints.shape[1]
    with torch.cuda.device(dev):
        L.check(L.load().romp_fit_scene(L.ptr(joints), int(N), int(J), L.ptr(cam), int(mode), L.ptr(groups[0]), L.ptr(groups[1]),
                                        L.ptr(depth_ids), float(w_depth), float(thresh), int(kind), table,
                                        0 if table is None else len(table), L.ptr(radius_scale), float(w_col), L.ptr(term_w), L.ptr(gj),
                                        int(acc_j), L.ptr(gc), int(acc_c), L.ptr(loss), L.ptr(history), int(row), L.stream_ptr(dev)))


def _pair(w, name):
    """A (velocity, acceleration) weight pair; a number stands for the velocity weight alone."""
    vel, acc = (w, 0.) if np.ndim(w) == 0 else w
    vel, acc = float(vel), float(acc)
    if not (vel >= 0 and acc >= 0):
        raise ValueError('%s must not be negative' % name)
    return vel, acc


def _align(align_inds):
    """-> ctypes int32 array of the alignment keypoints, or None.  The C side checks range and repeats."""
    if align_inds is None:
        return None
    idx = [int(i) for i in (align_inds.tolist() if hasattr(align_inds, 'tolist') else align_inds)]
    return (C.c_int32 * len(idx))(*idx) if idx else None


def _prior_on(prior, dev):
    """The prior's tensors on the device of the fit, contiguous."""
    if prior is None:
        return None
    if not isinstance(prior, PosePrior):
        raise ValueError('pose_prior must be a romp_amd.fitting.PosePrior')
    return prior.to(dev)


class _PosePriorFunction(torch.autograd.Function):
    """romp_fit_pose_prior as an autograd node.  The two losses have gradients of their own, so the forward launches once per
    term (the angle term with the mixture off) and leaves both; the backward scales them."""

    @staticmethod
    def forward(ctx, poses, prior):
        N = poses.shape[0]
        loss = torch.zeros(N, 2, device=poses.device, dtype=torch.float32)
        g_angle = torch.empty_like(poses)
        _pose_prior(poses, None, 0., 1., loss, None, g_angle, 0)
        gmm, g_gmm = loss[:, 0], None                                # zeros without a mixture
        if prior is not None:
            both, g_gmm = torch.empty_like(loss), torch.empty_like(poses)
            _pose_prior(poses, prior, 1., 0., both, None, g_gmm, 0)
            gmm = both[:, 0]
        ctx.has_gmm = g_gmm is not None
        ctx.save_for_backward(*([g_angle, g_gmm] if ctx.has_gmm else [g_angle]))
        return gmm.clone(), loss[:, 1].clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_gmm, grad_angle):
        if not ctx.needs_input_grad[0]:
            return None, None
        g = ctx.saved_tensors[0] * grad_angle.to(ctx.saved_tensors[0].device).float()[:, None]
        if ctx.has_gmm:
            g = g + ctx.saved_tensors[1] * grad_gmm.to(g.device).float()[:, None]
        return g, None


def pose_prior_loss(poses, prior=None):
    """poses (N,72), prior: a ``PosePrior`` or None (mixture off) -> (gmm (N,), angle (N,)), both unweighted and differentiable
    in poses: the max-mixture negative log-likelihood of poses[:, 3:3+D] and the joint-angle prior of the elbows and knees."""
    dev = poses.device
    poses = _f32(poses, dev)
    if poses.dim() != 2 or poses.shape[1] != 72:
        raise ValueError('pose_prior_loss: poses (N,72)')
    return _PosePriorFunction.apply(poses, _prior_on(prior, dev))


class _Joints3dFunction(torch.autograd.Function):
    """romp_fit_joints3d as an autograd node: the forward launch leaves both gradients, the backward scales them."""

    @staticmethod
    def forward(ctx, joints, trans, targets, conf, inds_c, align_c, sigma):
        loss = torch.empty(joints.shape[0], device=joints.device, dtype=torch.float32)
        gj, gt = torch.empty_like(joints), None if trans is None else torch.empty_like(trans)
        _joints3d(joints, trans, targets, conf, inds_c, align_c, sigma, 1., loss, gj, gt, 0)
        ctx.has_trans = gt is not None
        ctx.save_for_backward(*([gj, gt] if ctx.has_trans else [gj]))
        return loss

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        gj = ctx.saved_tensors[0]
        g = grad_loss.to(gj.device).float()
        need_j, need_t = ctx.needs_input_grad[0], ctx.has_trans and ctx.needs_input_grad[1]
        return (gj * g[:, None, None] if need_j else None, ctx.saved_tensors[1] * g[:, None] if need_t else None,
                None, None, None, None, None)


def joints3d_loss(joints, targets, conf=None, joint_inds=None, align_inds=None, sigma=0., trans=None):
    """joints (N,J,3), targets (N,K,3) in the frame of the joints (plus trans (N,3) when given), conf (N,K) or None, joint_inds:
    K distinct joint indices or None (= the first K joints), align_inds: indices into the K keypoints whose mean is taken off
    predictions and targets alike, or None -> loss (N,), differentiable in joints and trans."""
    dev = joints.device
    joints, targets = _f32(joints, dev), _f32(targets, dev)
    conf = None if conf is None else _f32(conf, dev)
    trans = None if trans is None else _f32(trans, dev)
    if joints.dim() != 3 or joints.shape[2] != 3 or targets.dim() != 3 or targets.shape[0] != joints.shape[0] or targets.shape[2] != 3 or \
            (conf is not None and conf.shape != targets.shape[:2]) or (trans is not None and trans.shape != (joints.shape[0], 3)):
        raise ValueError('joints3d_loss: joints (N,J,3), targets (N,K,3), conf (N,K), trans (N,3)')
    return _Joints3dFunction.apply(joints, trans, targets, conf, _inds(joint_inds, targets.shape[1]), _align(align_inds), sigma)


class KeypointFitter(object):
    """Adam on (betas, poses, cam) against 2-D keypoints, every step on the device:

        fitter = KeypointFitter(smpl, camera='weak', steps=30, lr=0.02)
        res = fitter.fit(betas0, poses0, cam0, kp2d, conf)       # dict: betas, poses, cam, verts, joints, loss_history

    smpl: a ``romp_amd.smpl.SMPL`` on the device.  The priors are L2 with per-column weights, added to the gradient inside the
    Adam launch:  w_betas |betas|^2  keeps the shape small,  w_pose |poses - poses0|^2  holds the pose near the start, the
    global orientation (columns 0-2) excepted.  Each weight is a number or a vector with one entry per column.
    ``loss_history`` (steps + 1, N) holds the 2-D data term before every step and after the last; it stays on the device.

    SMPLify's terms (include/romp_hip_fit_priors.h), all off by default, each one more launch per step:
    ``pose_prior`` (a ``PosePrior``) with ``w_gmm`` > 0 adds  w_gmm * min_m (0.5 d^T P_m d + offset_m)  over the body pose;
    ``w_angle`` > 0 adds  w_angle * sum exp(2 s theta)  over elbows and knees; both come with ``prior_history``
    (steps + 1, N, 2), unweighted.  ``joints3d`` (N,K,3) given to ``fit`` adds  w_3d * (the loss of ``joints3d_loss``)  with
    ``sigma_3d`` and ``align_inds``, and ``loss3d_history`` (steps + 1, N), unweighted.  With the perspective camera the targets
    are camera-space points (the joints plus cam); with the weak camera they are in the frame of the joints.  ``kp2d`` may be
    None when ``joints3d`` is given: the 2-D launch is skipped and ``loss_history`` is zeros.

    Temporal smoothness terms (include/romp_hip_fit_clip.h), all off by default; they act when ``fit`` is given ``links``, the
    (prev, next) row tables of ``romp_amd.clip.clip_links``, and tie a row to the rows of the same track in the neighbouring
    frames.  Each (vel, acc) pair weighs  sum_n rho(|x[n] - x[prev n]|^2)  and  sum_n rho(|x[prev n] - 2 x[n] + x[next n]|^2);
    a number stands for vel alone.
    ``w_smooth_joints`` on the 71 joints the layer returns (213 columns; ``smooth_joint_inds`` picks joints, three columns of
    weight one per picked joint).  These joints are in the BODY frame -- the layer's output before any camera -- so the term
    smooths the articulated motion only; the motion of the root through the scene is the camera segment's business:
    ``w_smooth_cam`` on the three camera columns.  ``w_smooth_betas``: velocity only, one shape per track.
    ``w_smooth_pose`` weighs  sum_n rho(sum_j joint_w[j] |R_j(n) - R_j(prev n)|_F^2)  over the 24 joint rotations (``joint_w``
    (24,) or None = ones), first order, free of the axis-angle wrap.  ``sigma_smooth`` > 0 makes rho Geman-McClure for all of
    them.  With any of them on a step gains two launches (joints and camera before ``smpl_backward``, betas and rotations
    after it) and the result ``smooth_history`` (steps + 1, N, L), unweighted: (vel, acc) columns for joints, cam and betas,
    then one for the rotations, each present when its term is on.

    Scene terms (include/romp_hip_fit_scene.h), all off by default; they act when ``fit`` is given ``scene``, the (offsets,
    members) row tables of ``romp_amd.scene.scene_groups``, and tie the persons of one image together.  ``w_depth_order``
    weighs the depth-order term of ``romp_amd.scene.depth_order_loss`` on the ``depth_ids`` given to ``fit`` (``depth_loss_type``
    'piecewise' or 'log', ``dist_thresh``); ``w_collision`` weighs ``romp_amd.scene.collision_loss`` with the table ``spheres``
    (a ``BodySpheres``; None = ``body_spheres`` of the layer) and ``fit``'s ``radius_scale``.  The translation of a row is cam
    with the perspective camera and 2 (c1 / s, c2 / s, 1 / s) with the weak one.  With either on a step gains one launch
    (after the 2-D, 3-D and temporal ones, before ``smpl_backward``) and the result ``scene_history`` (steps + 1, N, 2),
    unweighted: (depth, collision)."""

    def __init__(self, smpl, camera='weak', steps=30, lr=0.02, sigma=0., w_betas=1e-4, w_pose=1e-4, root_align=False,
                 focal=443.4, half=256., betas=(0.9, 0.999), eps=1e-8, pose_prior=None, w_gmm=0., w_angle=0., w_3d=1., sigma_3d=0.,
                 align_inds=None, w_smooth_pose=0., joint_w=None, w_smooth_joints=(0., 0.), smooth_joint_inds=None,
                 w_smooth_cam=(0., 0.), w_smooth_betas=0., sigma_smooth=0., w_depth_order=0., depth_loss_type='piecewise',
                 dist_thresh=0.3, w_collision=0., spheres=None):
        self.smpl, self.camera, self.mode = smpl, camera, _mode(camera)
        self.steps, self.lr, self.sigma = int(steps), float(lr), float(sigma)
        self.w_betas, self.w_pose, self.root_align = w_betas, w_pose, bool(root_align)
        self.focal, self.half, self.adam_betas, self.eps = float(focal), float(half), (float(betas[0]), float(betas[1])), float(eps)
        self.pose_prior, self.w_gmm, self.w_angle = pose_prior, float(w_gmm), float(w_angle)
        self.w_3d, self.sigma_3d, self.align_inds = float(w_3d), float(sigma_3d), align_inds
        if self.steps < 0:
            raise ValueError('steps must not be negative')
        if self.w_gmm < 0 or self.w_angle < 0 or self.w_3d < 0:
            raise ValueError('w_gmm, w_angle and w_3d must not be negative')
        self.w_smooth_pose, self.joint_w, self.sigma_smooth = float(w_smooth_pose), joint_w, float(sigma_smooth)
        self.w_smooth_joints, self.w_smooth_cam = _pair(w_smooth_joints, 'w_smooth_joints'), _pair(w_smooth_cam, 'w_smooth_cam')
        self.w_smooth_betas, self.smooth_joint_inds = float(w_smooth_betas), smooth_joint_inds
        if not (self.w_smooth_pose >= 0 and self.w_smooth_betas >= 0):
            raise ValueError('w_smooth_pose and w_smooth_betas must not be negative')
        self.smooth_on = max(self.w_smooth_pose, self.w_smooth_betas, *(self.w_smooth_joints + self.w_smooth_cam)) > 0
        self.w_depth_order, self.w_collision, self.dist_thresh = float(w_depth_order), float(w_collision), float(dist_thresh)
        self.depth_loss_type, self.spheres = depth_loss_type, spheres
        if not (self.w_depth_order >= 0 and self.w_collision >= 0 and self.dist_thresh >= 0):
            raise ValueError('w_depth_order, w_collision and dist_thresh must not be negative')
        if str(depth_loss_type).lower() not in ('piecewise', 'log'):
            raise ValueError("depth_loss_type must be 'piecewise' or 'log', not %r" % (depth_loss_type,))
        self.scene_on = max(self.w_depth_order, self.w_collision) > 0

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

    def start(self, betas0, poses0, cam0, kp2d, conf=None, joint_inds=None, joints3d=None, conf3d=None, joint_inds3d=None, links=None,
              scene=None, depth_ids=None, radius_scale=None, fixed=None):
        """The buffers of one fit and its two halves of a step (``_FitRun``); ``fit`` drives it."""
        return _FitRun(self, betas0, poses0, cam0, kp2d, conf, joint_inds, joints3d, conf3d, joint_inds3d, links, scene, depth_ids,
                       radius_scale, fixed)

    def fit(self, betas0, poses0, cam0, kp2d, conf=None, joint_inds=None, joints3d=None, conf3d=None, joint_inds3d=None, links=None,
            scene=None, depth_ids=None, radius_scale=None, fixed=None):
        """betas0 (N,n_betas), poses0 (N,72), cam0 (N,3) (`cam` or `cam_trans`, by the camera), kp2d (N,K,2) in the normalised
        frame (None: no 2-D term, joints3d is needed then), conf (N,K) or None, joint_inds: K joint indices of the 71 or None
        (= the first K); joints3d (N,K3,3) or None, conf3d (N,K3) or None, joint_inds3d likewise.  The inputs are not changed.
        -> dict(betas, poses, cam, verts, joints, loss_history (steps + 1, N)), device tensors; nothing is downloaded; with the
        prior terms on also prior_history (steps + 1, N, 2), with joints3d also loss3d_history (steps + 1, N).
        links: (prev, next), the row tables of ``romp_amd.clip.clip_links``, or None; with links and a smoothness weight above
        zero the rows of a track are fitted together and smooth_history (steps + 1, N, L) is returned too.
        scene: (offsets, members), the row tables of ``romp_amd.scene.scene_groups``, or None; with scene and a scene weight above
        zero the persons of an image are fitted together and scene_history (steps + 1, N, 2) is returned too.  depth_ids (N,)
        integer depth layers, -1 = unlabelled (None: no depth term); radius_scale (N,) or None = ones.  fixed: (joints (F,71,3),
        cam (F,3)) or None: F further rows that take part in the scenes but are not fitted (persons on another layer); the
        tables, depth_ids and radius_scale then cover N + F rows, the fitted ones first."""
        run = self.start(betas0, poses0, cam0, kp2d, conf, joint_inds, joints3d, conf3d, joint_inds3d, links, scene, depth_ids,
                         radius_scale, fixed)
        for s in range(self.steps):
            run.evaluate(s)
            run.update(s + 1)
        run.evaluate(self.steps)
        run.prior(self.steps, accumulate=0)                           # the prior's last row; its gradient is not used
        run.smooth_params(self.steps, accumulate=0)                   # likewise
        out = {'betas': run.betas, 'poses': run.poses, 'cam': run.cam, 'verts': run.verts, 'joints': run.joints,
               'loss_history': run.history}
        if run.smooth_on:
            out['smooth_history'] = torch.cat([h for h in (run.hist_eval, run.hist_upd) if h is not None], 2)
        if run.scene_on:
            out['scene_history'] = run.hist_scene[:, :run.N]
        if run.prior_on:
            out['prior_history'] = run.prior_history
        if run.targets3d is not None:
            out['loss3d_history'] = run.history3d
        return out


class _FitRun(object):
    """Device buffers of one KeypointFitter.fit and the two halves of a step.  evaluate(row): smpl_forward and
    romp_fit_reproject (loss into history[row], joint and camera gradients); update(step): smpl_backward from the joint
    gradients alone and romp_fit_adam over betas, poses and cam (step counts from 1).  With 3-D targets evaluate also runs
    romp_fit_joints3d onto the same gradients; with a prior term on update runs romp_fit_pose_prior between its two launches
    (losses into prior_history[the row of the last evaluate]).  With links and a smoothness term on, evaluate ends with
    romp_fit_temporal over the joints and the camera, onto the gradients smpl_backward and romp_fit_adam read, and update runs
    it over the betas and the rotations between smpl_backward and romp_fit_adam.  With scene tables and a scene term on,
    evaluate ends with romp_fit_scene over the joints and the camera, onto the same gradients."""

    def __init__(self, fitter, betas0, poses0, cam0, kp2d, conf, joint_inds, joints3d=None, conf3d=None, joint_inds3d=None, links=None,
                 scene=None, depth_ids=None, radius_scale=None, fixed=None):
        self.fitter, smpl = fitter, fitter.smpl
        self.dev = dev = smpl.shapedirs.device
        self.ctx = smpl._context()                                   # raises without a HIP device
        self.h = L.load()
        self.betas, self.poses, self.cam = (_f32(t, dev).detach().clone() for t in (betas0, poses0, cam0))
        if kp2d is None and joints3d is None:
            raise ValueError('fit: kp2d or joints3d is needed')
        self.kp2d = None if kp2d is None else _f32(kp2d, dev)
        self.conf = None if conf is None or kp2d is None else _f32(conf, dev)
        N, nb = self.betas.shape
        if self.poses.shape != (N, 72) or self.cam.shape != (N, 3) or (self.kp2d is not None and (
                self.kp2d.dim() != 3 or self.kp2d.shape[0] != N or self.kp2d.shape[2] != 2 or
                (self.conf is not None and self.conf.shape != self.kp2d.shape[:2]))):
            raise ValueError('fit: betas (N,n_betas), poses (N,72), cam (N,3), kp2d (N,K,2), conf (N,K)')
        self.N, self.nb = N, nb
        self.inds_c = None if self.kp2d is None else _inds(joint_inds, self.kp2d.shape[1])
        f32 = dict(device=dev, dtype=torch.float32)
        self.verts, self.joints = torch.empty(N, 6890, 3, **f32), torch.empty(N, 71, 3, **f32)
        self.loss, self.gj = torch.empty(N, **f32), torch.empty(N, 71, 3, **f32)
        # without a 2-D term nothing writes the gradient of a weak camera: it is zero, and Adam leaves the camera where it is
        self.gc = torch.empty(N, 3, **f32) if self.kp2d is not None else torch.zeros(N, 3, **f32)
        self.gb, self.gp = torch.empty_like(self.betas), torch.empty_like(self.poses)
        self.history = torch.empty(fitter.steps + 1, N, **f32) if self.kp2d is not None else torch.zeros(fitter.steps + 1, N, **f32)
        self.targets3d = self.conf3d = self.inds3d_c = self.align_c = self.history3d = None
        if joints3d is not None:
            self.targets3d = _f32(joints3d, dev)
            self.conf3d = None if conf3d is None else _f32(conf3d, dev)
            if self.targets3d.dim() != 3 or self.targets3d.shape[0] != N or self.targets3d.shape[2] != 3 or \
                    (self.conf3d is not None and self.conf3d.shape != self.targets3d.shape[:2]):
                raise ValueError('fit: joints3d (N,K,3), conf3d (N,K)')
            self.inds3d_c, self.align_c = _inds(joint_inds3d, self.targets3d.shape[1]), _align(fitter.align_inds)
            self.loss3d, self.history3d = torch.empty(N, **f32), torch.empty(fitter.steps + 1, N, **f32)
        self.pose_prior = _prior_on(fitter.pose_prior, dev) if fitter.w_gmm > 0 else None
        self.prior_on = self.pose_prior is not None or fitter.w_angle > 0
        if self.prior_on:
            self.loss_prior, self.prior_history = torch.empty(N, 2, **f32), torch.empty(fitter.steps + 1, N, 2, **f32)
        self.row = 0
        self.scene_on = scene is not None and (fitter.w_collision > 0 or (fitter.w_depth_order > 0 and depth_ids is not None))
        if self.scene_on:                                            # before anything below takes the buffers' addresses
            self._scene_setup(scene, depth_ids, radius_scale, fixed, f32)
        self.smooth_on = links is not None and fitter.smooth_on
        self.seg_eval = self.seg_upd = self.hist_eval = self.hist_upd = None
        if self.smooth_on:
            self._smooth_setup(links, f32)
        # A step is bound by the host issuing its launches, so a fit with nothing but the old four entries keeps the old two
        # methods, test for test (profiles/fit_prior_latency.txt holds that step against the parent commit's).
        if self.kp2d is not None and self.targets3d is None and not self.prior_on and not self.smooth_on and not self.scene_on:
            self.evaluate, self.update = self._evaluate_2d, self._update_2d
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

    def _scene_setup(self, scene, depth_ids, radius_scale, fixed, f32):
        """The tables and buffers of the romp_fit_scene launch of a step.  With F fixed rows the joints, the camera and their
        gradients become the first N rows of (N + F)-row buffers whose tail holds the fixed rows, so one launch reads both."""
        from . import scene as S                                     # (scene imports this module: resolved at call time)
        BodySpheres, _groups, _kind, body_spheres = S.BodySpheres, S._groups, S._kind, S.body_spheres
        f, N, dev = self.fitter, self.N, self.dev
        NT = N
        if fixed is not None:
            fj, fc = (_f32(t, dev) for t in fixed)
            if fj.dim() != 3 or fj.shape[1:] != (71, 3) or fc.shape != (fj.shape[0], 3):
                raise ValueError('fit: fixed = (joints (F,71,3), cam (F,3))')
            NT = N + fj.shape[0]
            self.joints_all, self.cam_all = torch.cat([self.joints, fj]), torch.cat([self.cam, fc])
            self.gj_all, self.gc_all = torch.zeros(NT, 71, 3, **f32), torch.zeros(NT, 3, **f32)
            self.joints, self.cam, self.gj, self.gc = self.joints_all[:N], self.cam_all[:N], self.gj_all[:N], self.gc_all[:N]
        else:
            self.joints_all, self.cam_all, self.gj_all, self.gc_all = self.joints, self.cam, self.gj, self.gc
        self.scene = _groups(scene, NT, dev)
        self.depth_ids = None
        if depth_ids is not None and f.w_depth_order > 0:
            self.depth_ids = torch.as_tensor(depth_ids).to(dev).to(torch.int32).contiguous()
            if self.depth_ids.shape != (NT,):
                raise ValueError('fit: depth_ids needs one entry per row (%d), got %s' % (NT, tuple(self.depth_ids.shape)))
        self.sphere_table = None
        if f.w_collision > 0:
            spheres = body_spheres(f.smpl) if f.spheres is None else f.spheres
            if not isinstance(spheres, BodySpheres) or not len(spheres):
                raise ValueError('spheres must be a non-empty romp_amd.scene.BodySpheres')
            self.sphere_table = spheres.table()
        self.radius_scale = None if radius_scale is None or self.sphere_table is None else _f32(radius_scale, dev).reshape(-1)
        if self.radius_scale is not None and self.radius_scale.shape != (NT,):
            raise ValueError('fit: radius_scale needs one entry per row (%d)' % NT)
        self.scene_kind = _kind(f.depth_loss_type)
        self.loss_scene, self.hist_scene = torch.empty(NT, 2, **f32), torch.empty(f.steps + 1, NT, 2, **f32)

    def _scene(self, row):
        """romp_fit_scene on the current joints and camera: the losses into scene_history[row], the gradients onto those of the
        joints (always written earlier in the step) and into or onto that of the camera."""
        f = self.fitter
        cam_written = self.kp2d is not None or (self.targets3d is not None and f.mode == 1) or \
            (self.seg_eval is not None and max(f.w_smooth_cam) > 0)
        _fit_scene(self.joints_all if self.sphere_table is not None else None, self.cam_all, f.mode, self.scene, self.depth_ids,
                   f.w_depth_order, f.dist_thresh, self.scene_kind, self.sphere_table, self.radius_scale, f.w_collision, None,
                   self.gj_all if self.sphere_table is not None else None, 1, self.gc_all, int(cam_written), self.loss_scene,
                   self.hist_scene, row)

    def _smooth_setup(self, links, f32):
        """The segment tables and loss buffers of the two romp_fit_temporal launches of a step."""
        f, N, dev, rows = self.fitter, self.N, self.dev, self.fitter.steps + 1
        self.links = _links(links, N, dev)
        sig = f.sigma_smooth
        self.col_w = None
        if f.smooth_joint_inds is not None:
            idx = torch.as_tensor([int(i) for i in f.smooth_joint_inds], dtype=torch.long)
            if idx.numel() == 0 or int(idx.min()) < 0 or int(idx.max()) >= 71:
                raise ValueError('smooth_joint_inds must name joints 0..70')
            picked = torch.zeros(71, 3, dtype=torch.float32)
            picked[idx] = 1.
            self.col_w = picked.reshape(213).to(dev)
        # gj is always written earlier in the step (by the 2-D or the 3-D term); gc only when one of them has a camera gradient
        cam_written = self.kp2d is not None or (self.targets3d is not None and f.mode == 1)
        segs = []
        if max(f.w_smooth_joints) > 0:
            segs.append(_clip_segment(self.joints, self.gj, self.col_w, f.w_smooth_joints[0], f.w_smooth_joints[1], sig, sig, 1))
        if max(f.w_smooth_cam) > 0:
            segs.append(_clip_segment(self.cam, self.gc, None, f.w_smooth_cam[0], f.w_smooth_cam[1], sig, sig, int(cam_written)))
        if segs:
            self.seg_eval = (L.ClipSegment * len(segs))(*segs)
            self.loss_eval, self.hist_eval = torch.empty(N, 2 * len(segs), **f32), torch.empty(rows, N, 2 * len(segs), **f32)
        self.rot_on = f.w_smooth_pose > 0
        self.joint_w = None
        if self.rot_on and f.joint_w is not None:
            self.joint_w = _f32(f.joint_w, dev).reshape(-1)
            if self.joint_w.numel() != 24:
                raise ValueError('joint_w needs 24 entries, got %d' % self.joint_w.numel())
        if f.w_smooth_betas > 0:
            self.seg_upd = (L.ClipSegment * 1)(_clip_segment(self.betas, self.gb, None, f.w_smooth_betas, 0., sig, sig, 1))
        cols = 2 * (self.seg_upd is not None) + self.rot_on
        if cols:
            self.loss_upd, self.hist_upd = torch.empty(N, cols, **f32), torch.empty(rows, N, cols, **f32)

    def smooth_params(self, row, accumulate):
        """romp_fit_temporal on the current betas and rotations: the losses into smooth_history[row], the gradients into (or
        onto) those of betas and poses.  Nothing when both terms are off."""
        if self.hist_upd is not None:
            f = self.fitter
            if self.seg_upd is not None:
                self.seg_upd[0].accumulate = int(accumulate)
            _temporal(self.seg_upd, self.links, self.N, self.loss_upd, self.poses if self.rot_on else None, self.joint_w,
                      f.w_smooth_pose, f.sigma_smooth, self.gp if self.rot_on else None, accumulate, self.hist_upd, row)

    def _evaluate_2d(self, row):
        f, ra = self.fitter, int(self.fitter.root_align)
        with torch.cuda.device(self.dev):
            L.check(self.h.smpl_forward(self.ctx, L.ptr(self.betas), self.nb, L.ptr(self.poses), self.N, ra, L.ptr(self.verts),
                                        L.ptr(self.joints), L.stream_ptr(self.dev)))
        _reproject(self.joints, self.cam, self.kp2d, self.conf, self.inds_c, f.mode, f.focal, f.half, f.sigma, self.loss, self.gj,
                   self.gc, self.history, row)

    def _update_2d(self, step):
        f, ra = self.fitter, int(self.fitter.root_align)
        with torch.cuda.device(self.dev):
            st = L.stream_ptr(self.dev)
            L.check(self.h.smpl_backward(self.ctx, L.ptr(self.betas), self.nb, L.ptr(self.poses), self.N, ra, None, L.ptr(self.gj),
                                         L.ptr(self.gb), L.ptr(self.gp), st))
            L.check(self.h.romp_fit_adam(self.segs, 3, f.lr, f.adam_betas[0], f.adam_betas[1], f.eps, int(step), st))

    def evaluate(self, row):
        f = self.fitter
        if self.kp2d is not None:
            self._evaluate_2d(row)
        else:
            with torch.cuda.device(self.dev):
                L.check(self.h.smpl_forward(self.ctx, L.ptr(self.betas), self.nb, L.ptr(self.poses), self.N, int(f.root_align),
                                            L.ptr(self.verts), L.ptr(self.joints), L.stream_ptr(self.dev)))
        if self.targets3d is not None:                               # perspective: camera-space targets, trans = cam
            cam = f.mode == 1
            _joints3d(self.joints, self.cam if cam else None, self.targets3d, self.conf3d, self.inds3d_c, self.align_c, f.sigma_3d,
                      f.w_3d, self.loss3d, self.gj, self.gc if cam else None, int(self.kp2d is not None), self.history3d, row)
        if self.seg_eval is not None:
            _temporal(self.seg_eval, self.links, self.N, self.loss_eval, history=self.hist_eval, row=row)
        if self.scene_on:
            self._scene(row)
        self.row = row

    def update(self, step):
        f, ra = self.fitter, int(self.fitter.root_align)
        with torch.cuda.device(self.dev):
            st = L.stream_ptr(self.dev)
            L.check(self.h.smpl_backward(self.ctx, L.ptr(self.betas), self.nb, L.ptr(self.poses), self.N, ra, None, L.ptr(self.gj),
                                         L.ptr(self.gb), L.ptr(self.gp), st))
            if self.prior_on:
                self.prior(self.row, accumulate=1)
            self.smooth_params(self.row, accumulate=1)
            L.check(self.h.romp_fit_adam(self.segs, 3, f.lr, f.adam_betas[0], f.adam_betas[1], f.eps, int(step), st))

    def prior(self, row, accumulate):
        """romp_fit_pose_prior on the current poses: the losses into prior_history[row], the gradient into (or onto) that of the
        poses.  Nothing when both prior terms are off."""
        if self.prior_on:
            f = self.fitter
            _pose_prior(self.poses, self.pose_prior, f.w_gmm, f.w_angle, self.loss_prior, None, self.gp, accumulate,
                        self.prior_history, row)


def keypoints_to_input_frame(kp2d_org, pad_info):
    """Original-image pixels -> the network's normalised frame: the inverse of convert_proejection_from_input_to_orgimg
    (post_parser.py:81-88), x = (x_org + left) * 2 / max(h, w) - 1, y with `top`.  pad_info = top, bottom, left, right, h, w."""
    top, _, left, _, h, w = [float(v) for v in pad_info]
    size = max(h, w)
    off = torch.tensor([left, top], dtype=torch.float32, device=kp2d_org.device)
    return (kp2d_org + off) * (2. / size) - 1.


def refine_outputs(model, outputs, kp2d_org, conf=None, joint_inds=None, pad_info=None, joints3d=None, conf3d=None, joint_inds3d=None,
                   **fit_args):
    """Refine the result dict of a ``ROMP`` / ``BEV`` forward against keypoints in original-image pixels.

    outputs: the dict of ``forward`` / ``forward_batch`` (numpy arrays or tensors) with smpl_betas, smpl_thetas and cam
    (ROMP) or cam_trans (BEV); kp2d_org (N,K,2), conf (N,K) or None, row for row with the dict's persons (matching detections
    to annotations is the caller's job: ``evaluation.match_2d_greedy``).  pad_info: the (top, bottom, left, right, h, w) of the
    frame's pre-processing; None means a 512 x 512 frame without padding.  fit_args go to ``KeypointFitter``, its pose_prior,
    w_gmm, w_angle, w_3d, sigma_3d and align_inds among them.  joints3d (N,K3,3), conf3d (N,K3), joint_inds3d: 3-D targets, in
    the frame of the joints for ROMP and in camera space (joints + cam_trans) for BEV; kp2d_org may be None then.

    ROMP is fitted with the weak-perspective camera `cam`; BEV with the perspective camera `cam_trans`, always root-aligned,
    infants (betas[:, 10] > 0.8) on the SMIL layer as in BEV's own parser (one host read of that mask, as there); BEV's `cam`
    stays the network's; the mixture prior describes adults, so the infants are fitted without it (their prior_history[..., 0]
    is zero) and keep the angle prior.  Returns a copy of
    the dict, device tensors, with smpl_thetas, smpl_betas, cam / cam_trans, verts, joints, pj2d, pj2d_org rewritten (by
    ``romp_project`` / ``romp_bev_project_verts``) and fit_loss (N,2): the 2-D loss before and after; with a prior term on
    also prior_history (steps + 1, N, 2), with joints3d also loss3d_history (steps + 1, N)."""
    return _refine(model, outputs, kp2d_org, conf, joint_inds, pad_info, joints3d, conf3d, joint_inds3d, None, fit_args)


def _refine(model, outputs, kp2d_org, conf, joint_inds, pad_info, joints3d, conf3d, joint_inds3d, link_fn, fit_args, scene_fn=None):
    """``refine_outputs``; link_fn(rows) -> the (prev, next) of the rows fitted together (rows: device indices into the dict's
    persons, None = all of them), or link_fn = None for unrelated rows (``romp_amd.clip.refine_clip`` supplies it).
    scene_fn(rows, new) -> the scene arguments of ``KeypointFitter.fit`` for those rows (new: the BEV results so far, its
    joints and cam_trans the network's for the rows not fitted yet), or None (``romp_amd.scene.refine_scene`` supplies it)."""
    from .post_parser import body_mesh_projection2image
    parser = getattr(model, 'smpl_parser', None)
    if parser is None:
        raise L.RompHipError('refine_outputs needs a model built with calc_smpl')
    is_bev = hasattr(parser, 'smil_model')                            # bev.SMPLA_parser; post_parser.SMPL_parser has one layer
    dev = model.tdevice
    pad = [0., 512., 0., 512., 512., 512.] if pad_info is None else [float(v) for v in np.asarray(pad_info).reshape(-1)]
    betas, thetas = _f32(outputs['smpl_betas'], dev), _f32(outputs['smpl_thetas'], dev)
    kp = None if kp2d_org is None else keypoints_to_input_frame(_f32(kp2d_org, dev), pad)
    conf = None if conf is None else _f32(conf, dev)
    joints3d, conf3d = (None if t is None else _f32(t, dev) for t in (joints3d, conf3d))
    extra = ('prior_history', 'loss3d_history', 'smooth_history', 'scene_history')
    scene_of = (lambda rows, new: {}) if scene_fn is None else scene_fn
    N = betas.shape[0]
    out = dict(outputs)
    links_of = (lambda rows: None) if link_fn is None else link_fn
    if not is_bev:
        fitter = KeypointFitter(parser.smpl_model, camera='weak', **dict(dict(root_align=model.settings.root_align), **fit_args))
        res = fitter.fit(betas, thetas, _f32(outputs['cam'], dev), kp, conf, joint_inds, joints3d, conf3d, joint_inds3d,
                         links=links_of(None), **scene_of(None, None))
        proj = body_mesh_projection2image(res['joints'], res['cam'], input2org_offsets=pad)
        out.update({'smpl_betas': res['betas'], 'smpl_thetas': res['poses'], 'cam': res['cam'], 'cam_trans': proj['cam_trans'],
                    'verts': res['verts'], 'joints': res['joints'], 'pj2d': proj['pj2d'], 'pj2d_org': proj['pj2d_org'],
                    'fit_loss': res['loss_history'][[0, -1]].t().contiguous()})
        out.update({k: res[k] for k in extra if k in res})
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
    if scene_fn is not None:                                          # a group's fixed rows: the network's joints until they are fitted
        new['joints'] = _f32(outputs['joints'], dev).clone()
    pick = lambda t, rows: None if t is None else t[rows]
    for layer, rows, nb in groups:
        if rows.numel() == 0:
            continue
        rows = rows.to(dev)
        group_args = dict(args, pose_prior=None) if layer is parser.smil_model else args
        res = KeypointFitter(layer, camera='perspective', **group_args).fit(
            betas[rows][:, :nb], thetas[rows], trans[rows], pick(kp, rows), pick(conf, rows), joint_inds, pick(joints3d, rows),
            pick(conf3d, rows), joint_inds3d, links=links_of(rows), **scene_of(rows, new))
        new['smpl_betas'][rows, :nb] = res['betas']
        for key in extra:                                             # (steps + 1, n, ...) of this group into (steps + 1, N, ...)
            if key in res:
                if key not in new:
                    new[key] = torch.zeros((res[key].shape[0], N) + tuple(res[key].shape[2:]), device=dev)
                new[key][:, rows] = res[key]
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
