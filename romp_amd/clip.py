"""[romp_amd] Tracked clips on the device: the rows of one track tied together in a fit (include/romp_hip_fit_clip.h,
csrc/fit_clip.hip).

A row is one person in one frame.  ``DeviceTracker`` / ``smooth_batch`` give every row a track id; ``clip_links`` turns the
ids into two row tables, and everything else here reads those:

  ``clip_links``                (track_ids, frame_ids) -> (prev, next): for every row the row of the same track in the
                                neighbouring frame, -1 for none.  Torch ops on the inputs' device, no download.
  ``temporal_loss``             autograd node around ``romp_fit_temporal``: velocity (order 1) or acceleration (order 2) of any
                                (N, cols) tensor along the links.
  ``rotation_smoothness_loss``  autograd node around the same entry: the chordal distance of consecutive joint rotations.
  ``refine_clip``               ``fitting.refine_outputs`` for a clip: ``KeypointFitter`` with its smoothness terms on.

The link rule: a link (p -> n) exists iff prev[n] == p, 0 <= p < N, p != n and next[p] == n; the kernels test it before they
read row p, so a table with stale or inconsistent entries acts as one with fewer links.  Rows may come in any order; the
frame-major order of ``forward_batch`` is the common one.  ``romp_amd.evaluation.accel`` / ``accel_error`` score a clip along
the same links."""
import torch

from . import fitting as F
from . import lib as L


def clip_links(track_ids, frame_ids, max_gap=1):
    """track_ids (N,), frame_ids (N,): integer tensors (or anything torch.as_tensor takes) -> (prev, next), int32 (N,) on the
    inputs' device.  Rows are ordered by (track, frame) with two stable sorts; consecutive rows of one track are linked iff
    1 <= frame gap <= max_gap, so two rows of one (track, frame) pair are never linked to each other, and a track seen again
    after more than max_gap frames starts a new chain."""
    track = torch.as_tensor(track_ids).reshape(-1).to(torch.int64)
    frame = torch.as_tensor(frame_ids, device=track.device).reshape(-1).to(torch.int64)
    if track.shape != frame.shape:
        raise ValueError('clip_links: one track id and one frame id per row, got %d and %d' % (track.numel(), frame.numel()))
    N, dev = track.numel(), track.device
    prev = torch.full((N,), -1, dtype=torch.int32, device=dev)
    nxt = torch.full((N,), -1, dtype=torch.int32, device=dev)
    if N < 2:
        return prev, nxt
    by_frame = torch.argsort(frame, stable=True)
    order = by_frame[torch.argsort(track[by_frame], stable=True)]   # rows by (track, frame); equal pairs keep their row order
    t, f = track[order], frame[order]
    gap = f[1:] - f[:-1]
    linked = (t[1:] == t[:-1]) & (gap >= 1) & (gap <= int(max_gap))
    none = torch.full((N - 1,), -1, dtype=torch.int32, device=dev)
    rows = order.to(torch.int32)
    prev[order[1:]] = torch.where(linked, rows[:-1], none)       # order is a permutation: every row is written at most once
    nxt[order[:-1]] = torch.where(linked, rows[1:], none)
    return prev, nxt


class _TemporalFunction(torch.autograd.Function):
    """romp_fit_temporal with one linear block as an autograd node.  loss[n] reads the rows linked to n, so the backward is a
    second launch with the incoming gradient as the per-row weights of the terms."""

    @staticmethod
    def forward(ctx, x, prev, nxt, col_w, order, sigma):
        N = x.shape[0]
        loss = torch.empty(N, 2, device=x.device, dtype=torch.float32)
        F._temporal((L.ClipSegment * 1)(F._clip_segment(x, torch.empty_like(x), col_w, 1., 1., sigma, sigma, 0)), (prev, nxt), N, loss)
        ctx.order, ctx.sigma, ctx.col_w = order, sigma, col_w
        ctx.save_for_backward(x, prev, nxt)
        return loss[:, order - 1].clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None, None
        x, prev, nxt = ctx.saved_tensors
        g, scratch = torch.empty_like(x), torch.empty(x.shape[0], 2, device=x.device, dtype=torch.float32)
        seg = F._clip_segment(x, g, ctx.col_w, float(ctx.order == 1), float(ctx.order == 2), ctx.sigma, ctx.sigma, 0)
        F._temporal((L.ClipSegment * 1)(seg), (prev, nxt), x.shape[0], scratch, term_w=grad_loss.to(x.device).float().contiguous())
        return g, None, None, None, None, None


def temporal_loss(x, links, order=1, col_w=None, sigma=0.):
    """x (N, ...) read as (N, cols), links = (prev, next) of ``clip_links``, col_w (cols,) or None (= ones) -> loss (N,),
    differentiable in x.  order 1: rho(sum_c col_w[c] (x[n] - x[prev n])[c]^2), zero at a row without a link from behind;
    order 2: rho(sum_c col_w[c] (x[prev n] - 2 x[n] + x[next n])[c]^2), zero at a row without both links.  rho(e) = e, or for
    sigma > 0 Geman-McClure sigma^2 e / (sigma^2 + e)."""
    if order not in (1, 2):
        raise ValueError('temporal_loss: order must be 1 (velocity) or 2 (acceleration), not %r' % (order,))
    dev = x.device
    x = F._f32(x, dev)
    if x.dim() < 2 or x[0].numel() < 1:
        raise ValueError('temporal_loss: x (N, cols)')
    prev, nxt = F._links(links, x.shape[0], dev)
    col_w = None if col_w is None else F._f32(col_w, dev).reshape(-1)
    if col_w is not None and col_w.numel() != x[0].numel():
        raise ValueError('temporal_loss: col_w needs %d entries, got %d' % (x[0].numel(), col_w.numel()))
    return _TemporalFunction.apply(x, prev, nxt, col_w, int(order), float(sigma))


class _RotationFunction(torch.autograd.Function):
    """The rotation block of romp_fit_temporal as an autograd node, in the way of ``_TemporalFunction``."""

    @staticmethod
    def forward(ctx, poses, prev, nxt, joint_w, sigma):
        N = poses.shape[0]
        loss = torch.empty(N, 1, device=poses.device, dtype=torch.float32)
        F._temporal(None, (prev, nxt), N, loss, poses, joint_w, 1., sigma, torch.empty_like(poses), 0)
        ctx.sigma, ctx.joint_w = sigma, joint_w
        ctx.save_for_backward(poses, prev, nxt)
        return loss[:, 0].clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        poses, prev, nxt = ctx.saved_tensors
        g, scratch = torch.empty_like(poses), torch.empty(poses.shape[0], 1, device=poses.device, dtype=torch.float32)
        F._temporal(None, (prev, nxt), poses.shape[0], scratch, poses, ctx.joint_w, 1., ctx.sigma, g, 0,
                    term_w=grad_loss.to(poses.device).float().contiguous())
        return g, None, None, None, None


def rotation_smoothness_loss(poses, links, joint_w=None, sigma=0.):
    """poses (N,72), links = (prev, next), joint_w (24,) or None (= ones) -> loss (N,), differentiable in poses:
    rho(sum_j joint_w[j] |R_j(n) - R_j(prev n)|_F^2) with R_j the layer's own Rodrigues matrix of columns 3j..3j+2, which is
    4 sum_j joint_w[j] (1 - cos phi_j) for the angle phi_j between the two rotations: no axis-angle wrap.  Zero at a row
    without a link from behind."""
    dev = poses.device
    poses = F._f32(poses, dev)
    if poses.dim() != 2 or poses.shape[1] != 72:
        raise ValueError('rotation_smoothness_loss: poses (N,72)')
    prev, nxt = F._links(links, poses.shape[0], dev)
    joint_w = None if joint_w is None else F._f32(joint_w, dev).reshape(-1)
    if joint_w is not None and joint_w.numel() != 24:
        raise ValueError('rotation_smoothness_loss: joint_w needs 24 entries, got %d' % joint_w.numel())
    return _RotationFunction.apply(poses, prev, nxt, joint_w, float(sigma))


def refine_clip(model, outputs, track_ids, frame_ids, kp2d_org, conf=None, joint_inds=None, pad_info=None, joints3d=None, conf3d=None,
                joint_inds3d=None, max_gap=1, **fit_args):
    """``fitting.refine_outputs`` for a tracked clip: outputs is the dict of a ``forward_batch`` over the clip's frames (or
    the rows of several calls stacked), track_ids (N,) and frame_ids (N,) name each row's track and frame, and fit_args carry
    the smoothness weights of ``KeypointFitter`` (w_smooth_pose, w_smooth_joints, w_smooth_cam, w_smooth_betas, sigma_smooth)
    among the rest.  One pad_info serves the clip: its frames share one size.  The links come from ``clip_links(track_ids,
    frame_ids, max_gap)``.  For BEV the adults and the infants are fitted separately, as in ``refine_outputs``, and the links
    are computed inside each group, so a track whose age class flips is cut there.  Returns what ``refine_outputs`` returns,
    plus smooth_history (steps + 1, N, L) when a smoothness term is on."""
    dev = model.tdevice
    track = torch.as_tensor(track_ids).reshape(-1).to(dev)
    frame = torch.as_tensor(frame_ids).reshape(-1).to(dev)

    def links_of(rows):
        return clip_links(track, frame, max_gap) if rows is None else clip_links(track[rows], frame[rows], max_gap)

    return F._refine(model, outputs, kp2d_org, conf, joint_inds, pad_info, joints3d, conf3d, joint_inds3d, links_of, fit_args)
