"""[romp_amd] Whole scenes on the device: the persons of one image tied together in a fit (include/romp_hip_fit_scene.h,
csrc/fit_scene.hip).

A row is one person in one image.  ``forward_batch`` gives every row the index of its image; ``scene_groups`` turns those into
two row tables, and everything else here reads them:

  ``scene_groups``      batch_ids -> (offsets, members): scene g is members[offsets[g]:offsets[g + 1]].  Torch ops on the
                        inputs' device, no download.
  ``depth_order_loss``  autograd node around ``romp_fit_scene``: the reference's relative_depth_loss (loss_funcs/
                        relative_loss.py:46-99) spread over the rows, from depth-layer labels ("A stands in front of B").
  ``collision_loss``    autograd node around the same entry: SMPLify's sphere-proxy interpenetration penalty (Bogo et al. 2016,
                        eq. 7) between different persons of a scene.
  ``BodySpheres``       the sphere table; ``body_spheres(smpl)`` derives a default one from a layer's own template.
  ``refine_scene``      ``fitting.refine_outputs`` for the persons of a ``forward_batch``, fitted together.

The table rule: a member entry is used only after 0 <= offsets[g] <= offsets[g + 1] <= N and 0 <= member < N have been tested;
the kernel skips an entry that fails, so stale or padded tables act as tables with fewer members."""
import numpy as np
import torch

from . import fitting as F
from . import lib as L

KINDS = {'piecewise': 0, 'log': 1}


def _kind(kind):
    k = str(kind).lower()
    if k not in KINDS:
        raise ValueError("depth_loss_type must be 'piecewise' or 'log', not %r" % (kind,))
    return KINDS[k]


def scene_groups(batch_ids):
    """batch_ids (N,): an integer tensor (or anything torch.as_tensor takes) with the image of every row -> (offsets (N + 1,),
    members (N,)), int32 on the inputs' device.  Group g is members[offsets[g]:offsets[g + 1]]; groups are ordered by image id,
    the rows of a group ascend; the groups past the last distinct image are empty; rows with a negative id belong to no scene
    and appear in no group (members is padded with -1).  One stable sort, a cumsum and a scatter of fixed output shape: the
    number of distinct images is never read on the host, so the tables always have N + 1 and N entries."""
    ids = torch.as_tensor(batch_ids).reshape(-1).to(torch.int64)
    N, dev = ids.numel(), ids.device
    if N == 0:
        return torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev)
    valid = ids >= 0
    key = torch.where(valid, ids, torch.full_like(ids, torch.iinfo(torch.int64).max))
    order = torch.argsort(key, stable=True)                      # valid rows first, by image, rows ascending inside an image
    skey, svalid = key[order], valid[order]
    first = torch.ones(N, dtype=torch.bool, device=dev)
    first[1:] = skey[1:] != skey[:-1]
    group = torch.cumsum((first & svalid).to(torch.int64), 0) - 1        # the group of every sorted position (valid ones)
    counts = torch.zeros(N, dtype=torch.int64, device=dev)
    counts.scatter_add_(0, group.clamp(min=0), svalid.to(torch.int64))   # an invalid position adds 0
    offsets = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(counts, 0)
    members = torch.where(svalid, order, torch.full_like(order, -1))
    return offsets.to(torch.int32), members.to(torch.int32)


def _groups(groups, N, dev):
    """(offsets, members) of ``scene_groups`` -> two contiguous int32 tensors on the device of the fit."""
    if not isinstance(groups, (tuple, list)) or len(groups) != 2:
        raise ValueError('scene must be the pair (offsets, members) of romp_amd.scene.scene_groups')
    offsets, members = (torch.as_tensor(t).to(dev).to(torch.int32).contiguous() for t in groups)
    if offsets.shape != (N + 1,) or members.shape != (N,):
        raise ValueError('scene: offsets needs %d entries and members %d, got %s and %s' % (N + 1, N, tuple(offsets.shape), tuple(members.shape)))
    return offsets, members


class BodySpheres(object):
    """The sphere table of ``romp_fit_scene``: sphere s has the centre (1 - a[s]) J[p[s]] + a[s] J[q[s]] and the radius r[s] in
    the units of the joints; at most 64 entries.  Held on the host: the table travels with the launch."""

    def __init__(self, p, q, a, r):
        as_list = lambda v, t: [t(x) for x in (v.tolist() if hasattr(v, 'tolist') else v)]
        self.p, self.q, self.a, self.r = as_list(p, int), as_list(q, int), as_list(a, float), as_list(r, float)
        if not len(self.p) == len(self.q) == len(self.a) == len(self.r):
            raise ValueError('BodySpheres: p, q, a and r need one entry per sphere')
        if len(self.p) > 64:
            raise ValueError('BodySpheres: at most 64 spheres, got %d' % len(self.p))

    def __len__(self):
        return len(self.p)

    def table(self):
        """-> ctypes array of ``lib.SceneSphere`` (None when empty).  The C side checks ranges and finiteness."""
        if not len(self):
            return None
        return (L.SceneSphere * len(self))(*[L.SceneSphere(p, q, a, r) for p, q, a, r in zip(self.p, self.q, self.a, self.r)])


R_MIN, R_MAX = 0.03, 0.15


def body_spheres(smpl):
    """The default table of a layer, from its own template and nothing else (v_template, J_regressor, lbs_weights, parents),
    computed in float64 on the host, deterministic.  With Jt = J_regressor v_template (the 24 rest joints) and part j = the
    vertices whose greatest skinning weight is joint j (``smpl.part_labels``):
      radius[j] = the mean distance of part j's template vertices to the segment from Jt[j] to the mean of its children's rest
                  joints (to the point Jt[j] for a leaf), clamped to [0.03, 0.15] (metres on SMPL; a part without vertices, or
                  with a non-finite mean, gets 0.03);
      24 spheres on the joints: (p, q, a, r) = (j, j, 0, radius[j]);
      23 spheres at the middle of the bones: (parent[j], j, 0.5, radius[parent[j]]) for every joint j with a parent.
    47 spheres in all; the indices are those of the first 24 of the layer's 71 joints."""
    v = smpl.v_template.detach().double().cpu().numpy()
    Jt = smpl.J_regressor.detach().double().cpu().numpy() @ v
    parents = [int(x) for x in smpl.parents.cpu().tolist()]
    labels = smpl.part_labels.cpu().numpy()
    radius = []
    for j in range(24):
        pts = v[labels == j]
        kids = [c for c in range(24) if parents[c] == j]
        a, b = Jt[j], (Jt[kids].mean(0) if kids else Jt[j])
        ab = b - a
        den = float(ab @ ab)
        t = np.clip((pts - a) @ ab / den, 0., 1.) if den > 0 else np.zeros(len(pts))
        dist = np.linalg.norm(pts - (a + t[:, None] * ab), axis=1)
        mean = float(dist.mean()) if len(pts) else R_MIN
        radius.append(float(np.clip(mean, R_MIN, R_MAX)) if np.isfinite(mean) else R_MIN)
    p, q, a, r = list(range(24)), list(range(24)), [0.] * 24, list(radius)
    for j in range(24):
        if 0 <= parents[j] < 24 and parents[j] != j:
            p.append(parents[j]), q.append(j), a.append(0.5), r.append(radius[parents[j]])
    return BodySpheres(p, q, a, r)


def _spheres(spheres):
    if not isinstance(spheres, BodySpheres):
        raise ValueError('spheres must be a romp_amd.scene.BodySpheres')
    return spheres


class _SceneFunction(torch.autograd.Function):
    """romp_fit_scene as an autograd node with one of its terms on.  loss[n] reads the rows of n's scene, so the backward is a
    second launch with the incoming gradient as the per-row weights of the terms."""

    @staticmethod
    def forward(ctx, joints, cam, offsets, members, depth_ids, thresh, kind, table, radius_scale, mode, col):
        N = cam.shape[0]
        loss = torch.empty(N, 2, device=cam.device, dtype=torch.float32)
        gj = None if table is None else torch.empty_like(joints)
        F._fit_scene(joints, cam, mode, (offsets, members), depth_ids, 0., thresh, kind, table, radius_scale, 0., None, gj, 0,
                     torch.empty_like(cam), 0, loss)
        ctx.args = (thresh, kind, table, mode, col)
        ctx.save_for_backward(*[t for t in (joints, cam, offsets, members, depth_ids, radius_scale) if t is not None])
        ctx.have = [t is not None for t in (joints, cam, offsets, members, depth_ids, radius_scale)]
        return loss[:, col].clone()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_loss):
        saved = list(ctx.saved_tensors)
        joints, cam, offsets, members, depth_ids, radius_scale = (saved.pop(0) if h else None for h in ctx.have)
        thresh, kind, table, mode, col = ctx.args
        gj, gc = None if table is None else torch.empty_like(joints), torch.empty_like(cam)
        F._fit_scene(joints, cam, mode, (offsets, members), depth_ids, float(col == 0), thresh, kind, table, radius_scale,
                     float(col == 1), grad_loss.to(cam.device).float().contiguous(), gj, 0, gc, 0, None)
        return (gj if ctx.needs_input_grad[0] else None, gc if ctx.needs_input_grad[1] else None) + (None,) * 9


def depth_order_loss(depth_or_cam, depth_ids, groups, dist_thresh=0.3, kind='piecewise', camera=None):
    """depth_or_cam: with camera None the depths z (N,); with camera 'perspective' cam_trans (N,3), z = its third column; with
    'weak' cam (N,3) = (s, c1, c2), z = 2 / s.  depth_ids (N,) integer depth layers, -1 = unlabelled; groups = (offsets,
    members) of ``scene_groups`` -> loss (N,), differentiable in depth_or_cam.  Over the pairs i < j of a scene's labelled
    rows, d = z_j - z_i, k = id_j - id_i: d^2 when k == 0, softplus(d) when k < 0, softplus(-d) when k > 0; 'piecewise' counts
    the last two only while the order is violated by the margin (d - k dist_thresh > 0, < 0), 'log' always.  With A active
    pairs in the scene, loss[n] = (1 / 2A) * the sum of the active pairs that contain n: a scene's rows sum to the reference's
    mean over the image, and loss.sum() / (number of scenes with A > 0) is the reference's scalar."""
    dev = depth_or_cam.device
    x = F._f32(depth_or_cam, dev)
    if camera is None:
        if x.dim() != 1:
            raise ValueError('depth_order_loss: depths (N,) without a camera, cam (N,3) with one')
        cam, mode = torch.stack([torch.zeros_like(x), torch.zeros_like(x), x], 1), 1
    else:
        mode = F._mode(camera)
        if x.dim() != 2 or x.shape[1] != 3:
            raise ValueError('depth_order_loss: cam (N,3)')
        cam = x
    N = cam.shape[0]
    offsets, members = _groups(groups, N, dev)
    ids = torch.as_tensor(depth_ids).to(dev).to(torch.int32).contiguous()
    if ids.shape != (N,):
        raise ValueError('depth_order_loss: one depth id per row (%d), got %s' % (N, tuple(ids.shape)))
    return _SceneFunction.apply(None, cam.contiguous(), offsets, members, ids, float(dist_thresh), _kind(kind), None, None, mode, 0)


def collision_loss(joints, cam, groups, spheres, radius_scale=None, camera='perspective'):
    """joints (N,J,3), cam (N,3) (`cam_trans`, or (s, c1, c2) with camera 'weak': t = 2 (c1 / s, c2 / s, 1 / s)), groups =
    (offsets, members), spheres: a ``BodySpheres``, radius_scale (N,) or None (= ones; below one for children) -> loss (N,),
    differentiable in joints and cam:  loss[n] = 1/2 sum over the other rows m of n's scene and all sphere pairs (s, u) of
    exp(-|c_ns - c_mu|^2 / (sigma_ns^2 + sigma_mu^2)),  c = the sphere centre plus t,  sigma = r / 3 * radius_scale."""
    dev = joints.device
    joints, cam = F._f32(joints, dev), F._f32(cam, dev)
    if joints.dim() != 3 or joints.shape[2] != 3 or cam.shape != (joints.shape[0], 3):
        raise ValueError('collision_loss: joints (N,J,3), cam (N,3)')
    N = joints.shape[0]
    offsets, members = _groups(groups, N, dev)
    table = _spheres(spheres).table()
    if table is None:
        raise ValueError('collision_loss: the sphere table is empty')
    scale = None if radius_scale is None else F._f32(radius_scale, dev).reshape(-1)
    if scale is not None and scale.shape != (N,):
        raise ValueError('collision_loss: radius_scale needs one entry per row (%d)' % N)
    return _SceneFunction.apply(joints, cam, offsets, members, None, 0., 0, table, scale, F._mode(camera), 1)


def refine_scene(model, outputs, batch_ids, kp2d_org, conf=None, joint_inds=None, pad_info=None, depth_ids=None, radius_scale=None,
                 **fit_args):
    """``fitting.refine_outputs`` for the persons of a ``forward_batch``, fitted together: outputs is the dict of the call,
    batch_ids (N,) the image of every row (its `reorganize_idx`), depth_ids (N,) the depth layers (-1 = unlabelled) or None,
    radius_scale (N,) or None, and fit_args carry ``KeypointFitter``'s w_depth_order, depth_loss_type, dist_thresh, w_collision
    and spheres among the rest.  The scenes come from ``scene_groups(batch_ids)``.  One pad_info serves all images.

    For BEV the adults and the infants sit on different layers and are fitted one after the other, as in ``refine_outputs``,
    but both stay in one scene: each group's fit sees the rows of the other group as FIXED rows (``fit(..., fixed=...)``) --
    the adults against the infants as the network placed them, then the infants against the fitted adults -- so the depth
    order and the collision term still tie an infant to the adult who holds it.  The sphere table of a group's fit is that
    layer's own (or ``spheres``) and is applied to the fixed rows too.  Returns what ``refine_outputs`` returns, plus
    scene_history (steps + 1, N, 2) when a scene term is on."""
    dev = model.tdevice
    ids = torch.as_tensor(batch_ids).reshape(-1).to(dev)
    labels = None if depth_ids is None else torch.as_tensor(depth_ids).reshape(-1).to(dev)
    scale = None if radius_scale is None else F._f32(radius_scale, dev).reshape(-1)
    N = ids.numel()

    def scene_of(rows, new):
        if rows is None:
            return dict(scene=scene_groups(ids), depth_ids=labels, radius_scale=scale)
        keep = torch.zeros(N, dtype=torch.bool, device=dev)
        keep[rows] = True
        rest = torch.nonzero(~keep).squeeze(1)
        order = torch.cat([rows, rest])                               # the fitted rows first, the fixed ones behind them
        fixed = None if rest.numel() == 0 else (new['joints'][rest], new['cam_trans'][rest])
        return dict(scene=scene_groups(ids[order]), depth_ids=None if labels is None else labels[order],
                    radius_scale=None if scale is None else scale[order], fixed=fixed)

    return F._refine(model, outputs, kp2d_org, conf, joint_inds, pad_info, None, None, None, None, fit_args, scene_of)
