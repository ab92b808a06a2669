"""The differentiable SMPL layer, CPU part (include/romp_hip_smpl_grad.h, csrc/smpl_grad.hip): the exported symbol, its
argument checks (they return before any HIP call), and `smpl_torch`, the torch restatement of
oracle.romp_oracle.smpl_forward whose float64 autograd is the reference of tests/test_gpu_smpl_grad.py.  The restatement is
pinned here against the oracle itself in float64."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from oracle import romp_oracle as O
from romp_amd.synthetic import make_smpl_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN = torch.tensor([-1] + list(range(23)))                 # every joint the child of the one before
STAR = torch.tensor([-1] + [0] * 23)                         # every joint a child of the root


def batch_rodrigues_torch(rv):
    """oracle.romp_oracle.batch_rodrigues (smpl.py:191-222): the 1e-8 goes onto every component before the norm."""
    angle = ((rv + 1e-8) ** 2).sum(1, keepdim=True).sqrt()
    d = rv / angle
    c, s = torch.cos(angle)[:, :, None], torch.sin(angle)[:, :, None]
    rx, ry, rz = d[:, 0], d[:, 1], d[:, 2]
    z = torch.zeros_like(rx)
    K = torch.stack([z, -rz, ry, rz, z, -rx, -ry, rx, z], 1).reshape(-1, 3, 3)
    return torch.eye(3, dtype=rv.dtype, device=rv.device)[None] + s * K + (1 - c) * (K @ K)


def smpl_torch(model, betas, poses, root_align=False, dtype=torch.float64):
    """oracle.romp_oracle.smpl_forward line by line in torch (differentiable in betas and poses), with the model dict's own
    kintree_table.  Runs where betas lives: the tests use it on the CPU, scripts/smpl_grad_latency.py also on the device.  -> verts (N,6890,3), joints (N,71,3)."""
    dev = betas.device
    g = lambda k: model[k].to(device=dev, dtype=dtype)
    betas, poses = betas.to(dtype), poses.to(dtype)
    N = betas.shape[0]
    sdirs = g('smpla_shapedirs' if betas.shape[1] == 11 else 'shapedirs')
    v_t, pdirs, Jreg, W = g('v_template'), g('posedirs'), g('J_regressor'), g('weights')
    parents = [int(p) for p in model['kintree_table'].tolist()]
    v_shaped = v_t[None] + torch.einsum('bl,mkl->bmk', betas, sdirs)
    J = torch.einsum('bik,ji->bjk', v_shaped, Jreg)
    R = batch_rodrigues_torch(poses.reshape(-1, 3)).reshape(N, 24, 3, 3)
    pose_feat = (R[:, 1:] - torch.eye(3, dtype=dtype, device=dev)).reshape(N, 207)
    v_posed = (pose_feat @ pdirs).reshape(N, 6890, 3) + v_shaped
    rel = torch.cat([J[:, :1], J[:, 1:] - J[:, parents[1:]]], 1)
    bottom = torch.tensor([0, 0, 0, 1], dtype=dtype, device=dev).expand(N, 24, 1, 4)
    T = torch.cat([torch.cat([R, rel[..., None]], 3), bottom], 2)                  # (N,24,4,4)
    G = [T[:, 0]]
    for i in range(1, 24):
        G.append(G[parents[i]] @ T[:, i])
    G = torch.stack(G, 1)
    J_tr = G[:, :, :3, 3]
    Jh = torch.cat([J, torch.zeros(N, 24, 1, dtype=dtype, device=dev)], 2)[..., None]
    A = torch.cat([G[..., :3], G[..., 3:] - G @ Jh], 3)
    Tv = (W @ A.reshape(N, 24, 16)).reshape(N, 6890, 4, 4)
    vh = torch.cat([v_posed, torch.ones(N, 6890, 1, dtype=dtype, device=dev)], 2)[..., None]
    verts = (Tv @ vh)[:, :, :3, 0]
    j21 = verts[:, model['extra_joints_index'].long().to(dev)]
    j9 = torch.einsum('bik,ji->bjk', verts, g('J_regressor_extra9'))
    j17 = torch.einsum('bik,ji->bjk', verts, g('J_regressor_h36m17'))
    joints = torch.cat([J_tr, j21, j9, j17], 1)
    if root_align:
        root = joints[:, [45, 46]].mean(1, keepdim=True)
        joints, verts = joints - root, verts - root
    return verts, joints


_MODELS = {}


def model_for(n_betas, tree=None):
    """The synthetic model (cached per n_betas), with another kinematic tree put into the dict if asked for."""
    if n_betas not in _MODELS:
        _MODELS[n_betas] = make_smpl_model(0, n_betas=n_betas)
    m = dict(_MODELS[n_betas])
    if tree is not None:
        m['kintree_table'] = tree.clone()
    return m


# ------------------------------------------------------------------------------------------------ the C seam
def test_smpl_grad_symbols_exported():
    from romp_amd import lib
    header = open(os.path.join(ROOT, 'include', 'romp_hip_smpl_grad.h')).read()
    declared = re.findall(r'^\s*(?:int|void)\s+(\w+)\s*\(', header, re.M)
    assert declared == lib.SMPL_GRAD_EXPORTS == ['smpl_backward']
    others = (lib.EXPORTS + lib.VIEW_EXPORTS + lib.MAP_EXPORTS + lib.TEXTURE_EXPORTS + lib.EVAL_EXPORTS + lib.RH_EXPORTS +
              lib.CANVAS_EXPORTS)
    assert not set(declared) & set(others)
    h = lib.load()
    assert h.romp_abi_version() == 7 == lib.ABI_VERSION
    for n in declared:
        assert getattr(h, n).restype is ctypes.c_int and len(getattr(h, n).argtypes) == 11, n


def test_smpl_backward_rejects_bad_arguments_before_any_device_call():
    from romp_amd import lib
    h = lib.load()
    buf = (ctypes.c_float * 128)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    rc = h.smpl_backward(None, p, 10, p, 1, 0, None, None, p, p, None)          # NULL context
    assert rc == -1 and b'smpl_backward' in h.romp_last_error()
    rc = h.smpl_backward(None, None, 10, None, 0, 0, None, None, None, None, None)
    assert rc == -1 and h.romp_last_error()
    # a negative N fails the same check, which never looks behind the (here meaningless) context pointer
    rc = h.smpl_backward(p, p, 10, p, -1, 0, None, None, p, p, None)
    assert rc == -1 and b'smpl_backward' in h.romp_last_error()


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('tree', ['model', 'chain', 'star'])
@pytest.mark.parametrize('root_align', [False, True])
@pytest.mark.parametrize('n_betas', [10, 11])
def test_restatement_equals_the_oracle_in_float64(n_betas, root_align, tree):
    model = model_for(n_betas, {'model': None, 'chain': CHAIN, 'star': STAR}[tree])
    g = torch.Generator().manual_seed(7 + n_betas)
    betas = torch.randn(3, n_betas, generator=g, dtype=torch.float64)
    poses = 0.4 * torch.randn(3, 72, generator=g, dtype=torch.float64)
    poses[1] = 0                                                  # one all-zero row: R = I through the 1e-8
    poses[2, 3:6] = torch.tensor([3.1, 0.2, -0.1], dtype=torch.float64)
    vo, jo, _ = O.smpl_forward(model, betas.numpy(), poses.numpy(), root_align=root_align, dtype=np.float64)
    vt, jt = smpl_torch(model, betas, poses, root_align=root_align, dtype=torch.float64)
    ev, ej = float(np.abs(vt.numpy() - vo).max()), float(np.abs(jt.numpy() - jo).max())
    print(f'n_betas {n_betas} root_align {root_align} tree {tree}: verts {ev:.2e} joints {ej:.2e}')
    assert ev <= 1e-12 and ej <= 1e-12


def test_restatement_gradient_is_finite_at_zero_and_near_pi():
    model = model_for(10)
    betas = torch.zeros(2, 10, dtype=torch.float64, requires_grad=True)
    poses = torch.zeros(2, 72, dtype=torch.float64)
    poses[1, 6:9] = torch.tensor([3.1, 0.2, -0.1], dtype=torch.float64)
    poses.requires_grad_(True)
    v, j = smpl_torch(model, betas, poses)
    (v.sum() + (j ** 2).sum()).backward()
    assert torch.isfinite(betas.grad).all() and torch.isfinite(poses.grad).all()
    assert float(poses.grad.abs().max()) > 0
