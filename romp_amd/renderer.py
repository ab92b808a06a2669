"""Sim3DR mesh renderer on the HIP device -- drop-in for ``simple_romp/vis_human/sim3drender``
(``renderer.py``: ``Sim3DR``, ``rasterize``, ``get_normal``; the Cython extension ``Sim3DR_Cython`` is
replaced by ``romp_sim3dr_*`` in libromp_hip.so, csrc/render.hip) and ``vis_utils.rotate_view_weak_perspective``
(``view_weak_perspective``).  Images are bit-identical to the reference's (tests/test_render.py, test_render_views.py).  No CPU path: a missing HIP device / extension raises.
Per-vertex colours (``render(texture=...)``, ``__call__(vert_colors=...)``) and ``specular_exp`` 2 are bit-identical too; a
larger exponent is formed by repeated multiplication, within one grey level of numpy's powf (tests/test_gpu_render_texture.py).
"""
import ctypes as C

import numpy as np
import torch

from . import lib as L


def _to_ctype(arr):
    return arr if arr.flags.c_contiguous else arr.copy(order='C')


def convert_type(obj):
    """renderer.py:27-30."""
    if isinstance(obj, (tuple, list)):
        return np.array(obj, dtype=np.float32)[None, :]
    return obj


class _Topology(object):
    """Triangles on the device + the vertex -> (triangle, corner) incidence lists in ascending order."""

    def __init__(self, triangles, nver, device):
        tri = np.ascontiguousarray(triangles, np.int32)
        flat = tri.reshape(-1).astype(np.int64)
        order = np.argsort(flat, kind='stable').astype(np.int32)           # stable: ascending corner index per vertex
        counts = np.bincount(flat, minlength=nver)
        off = np.zeros(nver + 1, np.int32)
        off[1:] = np.cumsum(counts)
        self.ntri, self.nver = tri.shape[0], nver
        self.tri = torch.from_numpy(tri).to(device)
        self.adj_off = torch.from_numpy(off).to(device)
        self.adj_ent = torch.from_numpy(order).to(device)


_topologies = {}


def _topology(triangles, nver, device):
    tri = np.ascontiguousarray(triangles, np.int32)
    key = (tri.shape, nver, str(device), hash(tri.tobytes()))
    if key not in _topologies:
        if len(_topologies) > 8:
            _topologies.clear()
        _topologies[key] = _Topology(tri, nver, device)
    return _topologies[key]


def _device(device=None):
    if not torch.cuda.is_available():
        raise L.RompHipError('romp_amd.renderer needs a HIP device; there is no CPU fallback')
    return torch.device(device if device is not None else 'cuda:%d' % torch.cuda.current_device())


def _verts_dev(verts_list, dev):
    """(n,V,3) float32 on the device from a device tensor, an array or a list of (V,3) arrays."""
    if torch.is_tensor(verts_list):
        return verts_list.to(dev, torch.float32).contiguous()
    if len(verts_list) == 0:
        return torch.empty((0, 0, 3), dtype=torch.float32, device=dev)
    return torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(v, np.float32) for v in verts_list]))).to(dev)


def _keys(keys, h, w, dev):
    """The rasterizer's h*w 64-bit words: the caller's tensor (checked) or a fresh one."""
    if keys is None:
        return torch.empty(h * w, dtype=torch.int64, device=dev)
    if not (torch.is_tensor(keys) and keys.dtype == torch.int64 and keys.device == dev and keys.is_contiguous() and keys.numel() == h * w):
        raise ValueError('keys must be a contiguous int64 tensor of %d x %d words on %s' % (h, w, dev))
    return keys


def _dev_array(x, dtype, dev):
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    return t.to(dev, dtype).contiguous()


def get_normal(vertices, triangles, device=None):
    """renderer.py:32-37: per-vertex normals (numpy in, numpy out)."""
    dev = _device(device)
    lib = L.load()
    v = torch.from_numpy(np.ascontiguousarray(vertices, np.float32)).to(dev)
    topo = _topology(triangles, v.shape[0], dev)
    out = torch.empty_like(v)
    L.check(lib.romp_sim3dr_normals(L.ptr(v), L.ptr(topo.tri), L.ptr(topo.adj_off), L.ptr(topo.adj_ent), v.shape[0], L.ptr(out),
                                    L.stream_ptr(dev)))
    return out.cpu().numpy()


def _rasterize_dev(image_dev, v_dev, topo, colors_dev, reverse, keys):
    h, w, c = image_dev.shape
    L.check(L.load().romp_sim3dr_rasterize(L.ptr(image_dev), L.ptr(v_dev), L.ptr(topo.tri), L.ptr(colors_dev), topo.ntri, h, w, c,
                                           int(bool(reverse)), L.ptr(keys), L.stream_ptr(image_dev.device)))


def rasterize(vertices, triangles, colors, bg=None, height=None, width=None, channel=None, reverse=False, device=None):
    """renderer.py:39-62: z-buffer rasterization of per-vertex colours onto `bg` (modified in place and
    returned, like the reference)."""
    if bg is None:
        assert height is not None and width is not None and channel is not None
        bg = np.zeros((height, width, channel), dtype=np.uint8)
    dev = _device(device)
    img = torch.from_numpy(np.ascontiguousarray(bg)).to(dev)
    v = torch.from_numpy(np.ascontiguousarray(vertices, np.float32)).to(dev)
    col = torch.from_numpy(np.ascontiguousarray(colors, np.float32)).to(dev)
    keys = torch.empty(img.shape[0] * img.shape[1], dtype=torch.int64, device=dev)
    _rasterize_dev(img, v, _topology(triangles, v.shape[0], dev), col, reverse, keys)
    bg[...] = img.cpu().numpy()
    return bg


class Sim3DR(object):
    """renderer.py:64-133.  `__call__(verts_list, triangles, bg, mesh_colors)` paints the meshes one after the
    other (each with a fresh z-buffer) onto a copy of `bg` and returns the uint8 image.  Meshes of one topology go
    through romp_sim3dr_render_batch together: the number of launches does not grow with the number of meshes.
    `specular_exp`: any integer >= 1 (the reference default is 1); the device raises v2v * reflection to it by repeated
    multiplication, which is numpy's result for 1 and 2 and within rounding of it above."""

    def __init__(self, **kwargs):
        self.intensity_ambient = convert_type(kwargs.get('intensity_ambient', 0.66))
        self.intensity_directional = convert_type(kwargs.get('intensity_directional', 0.36))
        self.intensity_specular = convert_type(kwargs.get('intensity_specular', 0.1))
        self.specular_exp = kwargs.get('specular_exp', 1)
        self.color_directional = convert_type(kwargs.get('color_directional', (1, 1, 1)))
        self.light_pos = convert_type(kwargs.get('light_pos', (0, 0, -5)))
        self.view_pos = convert_type(kwargs.get('view_pos', (0, 0, 5)))
        self.device = kwargs.get('device', None)
        self.max_canvases = int(kwargs.get('max_canvases', 32))            # [romp_amd] canvases per render_canvases launch set
        if self.max_canvases < 1:
            raise ValueError('max_canvases must be >= 1, got %d' % self.max_canvases)
        e = self.specular_exp
        if isinstance(e, bool) or not isinstance(e, (int, np.integer)) or e < 1:
            raise NotImplementedError('specular_exp must be an integer >= 1 on the device path (it multiplies repeatedly; '
                                      'a fractional or smaller exponent is not supported), got %r' % (e,))
        self.specular_exp = int(e)

    def update_light_pos(self, light_pos):
        self.light_pos = convert_type(light_pos)

    def _light_cfg(self, color):
        """The 14 floats of romp_sim3dr_light.  The ambient term is formed exactly as renderer.py:83 does: a
        float64 product added into a float32 zero buffer."""
        amb = np.zeros((1, 3), np.float32)
        if self.intensity_ambient > 0:
            amb += self.intensity_ambient * np.array(color)
        i_dir = np.float32(self.intensity_directional) if self.intensity_directional > 0 else np.float32(0)
        i_spec = np.float32(self.intensity_specular) if self.intensity_specular > 0 else np.float32(0)
        cfg = np.concatenate([amb.reshape(3), [i_dir, i_spec], np.asarray(self.color_directional, np.float32).reshape(3),
                              np.asarray(self.light_pos, np.float32).reshape(3), np.asarray(self.view_pos, np.float32).reshape(3)])
        return (C.c_float * 14)(*[float(x) for x in cfg.astype(np.float32)])

    def _render_dev(self, img, v, topo, color, keys, light, texture=None):
        lib = L.load()
        st = L.stream_ptr(img.device)
        normal = torch.empty_like(v)
        L.check(lib.romp_sim3dr_normals(L.ptr(v), L.ptr(topo.tri), L.ptr(topo.adj_off), L.ptr(topo.adj_ent), topo.nver, L.ptr(normal), st))
        if texture is None and self.specular_exp == 1:
            L.check(lib.romp_sim3dr_light(L.ptr(v), L.ptr(normal), topo.nver, self._light_cfg(color), L.ptr(light), st))
        else:
            L.check(lib.romp_sim3dr_light_tex(L.ptr(v), L.ptr(normal), topo.nver, self._light_cfg(color), self.specular_exp,
                                              L.ptr(texture), L.ptr(light), st))
        _rasterize_dev(img, v, topo, light, False, keys)

    def render(self, vertices, triangles, bg, color=np.array([[1, 0.6, 0.4]]), texture=None):
        """renderer.py:76-118 for one mesh (numpy in; `bg` is modified in place and returned).  `texture`: (V,3) floats, one
        colour per vertex (taken as float32): the mesh is painted with texture * light, light lit with `color` as the
        ambient colour.  The reference scales the caller's `texture` array in place (`texture *= light`); this one leaves
        it untouched."""
        dev = _device(self.device)
        img = torch.from_numpy(np.ascontiguousarray(bg)).to(dev)
        v = torch.from_numpy(np.ascontiguousarray(vertices, np.float32)).to(dev)
        if texture is not None:
            texture = _dev_array(texture, torch.float32, dev)
            if tuple(texture.shape) != tuple(v.shape):
                raise ValueError('texture must be %s like the vertices, got %s' % (tuple(v.shape), tuple(texture.shape)))
        keys = torch.empty(img.shape[0] * img.shape[1], dtype=torch.int64, device=dev)
        self._render_dev(img, v, _topology(triangles, v.shape[0], dev), color, keys, torch.empty_like(v), texture)
        bg[...] = img.cpu().numpy()
        return bg

    def _ambient(self, colors):
        """The ambient term of `_light_cfg` for every row of `colors` (n,3): the same float64 product rounded into float32."""
        amb = np.zeros((len(colors), 3), np.float32)
        if self.intensity_ambient > 0:
            amb += self.intensity_ambient * np.array(colors)
        return amb

    def _render_batch(self, img, verts, topo, colors, keys, textures=None):
        """Meshes verts (n,V,3) (device) painted in index order onto img (h,w,3) (device, in place): one fixed set of launches.
        textures: (n,V,3) float32 (device) per-vertex colours or None.  Without them and with specular_exp 1 this is
        romp_sim3dr_render_batch, as before; otherwise romp_sim3dr_render_batch_tex, the same launches.
        Returns `keys`, which now hold every pixel's winner: `maps(..., keys=keys)` reads them instead of rasterizing again."""
        dev = img.device
        n = verts.shape[0]
        amb = torch.from_numpy(self._ambient(colors)).pin_memory().to(dev, non_blocking=True)   # no stream sync
        normals, light = torch.empty_like(verts), torch.empty_like(verts)
        lib = L.load()
        with torch.cuda.device(dev):
            if textures is None and self.specular_exp == 1:
                L.check(lib.romp_sim3dr_render_batch(L.ptr(img), img.shape[0], img.shape[1], L.ptr(verts), n, topo.nver, L.ptr(topo.tri),
                                                     topo.ntri, L.ptr(topo.adj_off), L.ptr(topo.adj_ent), L.ptr(amb),
                                                     self._light_cfg(colors[:1]), L.ptr(normals), L.ptr(light), L.ptr(keys),
                                                     L.stream_ptr(dev)))
            else:
                L.check(lib.romp_sim3dr_render_batch_tex(L.ptr(img), img.shape[0], img.shape[1], L.ptr(verts), n, topo.nver,
                                                         L.ptr(topo.tri), topo.ntri, L.ptr(topo.adj_off), L.ptr(topo.adj_ent), L.ptr(amb),
                                                         self._light_cfg(colors[:1]), L.ptr(textures), self.specular_exp,
                                                         L.ptr(normals), L.ptr(light), L.ptr(keys), L.stream_ptr(dev)))
        return keys

    def __call__(self, verts_list, triangles, bg, mesh_colors=np.array([[1, 0.6, 0.4]]), vert_colors=None, keys=None):
        """`bg`: numpy (h,w,3) uint8, or a device tensor (a canvas made on the device); neither is modified.  `vert_colors`:
        (n,V,3) floats, numpy or a device tensor, one colour per vertex: mesh i is painted with vert_colors[i] * light_i, its
        light lit with row i of `mesh_colors` as the ambient colour -- what `render(color=..., texture=...)` paints for each
        mesh in turn, in one batched call; None: light_i alone, as the reference.  `keys`: an int64
        device tensor of h*w words to rasterize into (default: a fresh one); with one topology and at least one mesh it holds
        the winners of this very picture afterwards, for `maps(..., keys=keys)`."""
        dev = _device(self.device)
        if torch.is_tensor(bg):
            img = bg.to(dev, torch.uint8).clone(memory_format=torch.contiguous_format)
        else:
            img = torch.from_numpy(np.ascontiguousarray(bg)).to(dev)        # a copy: the reference returns bg.copy()
        if img.dim() != 3 or img.shape[2] != 3:
            raise ValueError('Sim3DR paints (h, w, 3) images, got %s' % (tuple(img.shape),))
        keys = _keys(keys, img.shape[0], img.shape[1], dev)
        verts_dev = _verts_dev(verts_list, dev)
        n = len(verts_dev)
        if vert_colors is not None:
            vert_colors = _dev_array(vert_colors, torch.float32, dev)
            if vert_colors.dim() != 3 or vert_colors.shape[0] != n or (n and tuple(vert_colors.shape) != tuple(verts_dev.shape)):
                raise ValueError('vert_colors must be (n, V, 3) like the vertices %s, got %s'
                                 % (tuple(verts_dev.shape), tuple(vert_colors.shape)))
        if n == 0:
            return img.cpu().numpy()
        palette = np.asarray(mesh_colors)
        colors = palette[np.arange(n) % len(palette)]
        if len(np.shape(triangles)) == 2:                                    # one topology: every mesh in one batch
            self._render_batch(img, verts_dev, _topology(triangles, verts_dev.shape[1], dev), colors, keys, vert_colors)
        else:
            for ind in range(n):
                self._render_batch(img, verts_dev[ind:ind + 1], _topology(triangles[ind], verts_dev.shape[1], dev), colors[ind:ind + 1],
                                   keys, None if vert_colors is None else vert_colors[ind:ind + 1])
        return img.cpu().numpy()

    def render_canvases(self, verts, triangles, canvases, offsets, mesh_colors=np.array([[1, 0.6, 0.4]]), vert_colors=None, rows=None,
                        keys=None, return_tensor=False):
        """[romp_amd] `__call__` for C canvases of one size at once (romp_sim3dr_render_canvases, include/romp_hip_canvases.h):
        the slots offsets[c] .. offsets[c+1]-1 of verts (n,V,3) (ONE topology `triangles`) are painted in slot order onto a copy
        of canvases[c], what `__call__(verts[slice], triangles, canvases[c], ...)` paints, byte for byte, in five launches
        whatever C and n are, and all canvases come back in one download.
        `canvases`: (C,h,w,3) uint8, numpy or a device tensor, or one (h,w,3) canvas for all C = len(offsets) - 1; not modified.
        `offsets`: (C+1,) ascending, an array (host) or an int32 device tensor such as `evaluation.batch_offsets(batch_ids, B)`
        (no host sync then).  The device clamps each offset to [0, n]; a decreasing pair is an empty canvas, which keeps its bytes.
        Colours: without `rows`, slot j is lit with mesh_colors[j % len(mesh_colors)] and painted with vert_colors[j]
        ((n,V,3) or None), as in `__call__` on all n slots; with `rows` (n,) ints, slot j takes row rows[j] of mesh_colors (R,3)
        and of vert_colors (R,V,3): a person who sits in a different slot on every canvas keeps one row.
        `keys`: a contiguous int64 device tensor of C*h*w words to rasterize into; keys[c] then holds what `__call__` leaves for
        canvas c's slice (for `maps(verts[slice], ..., keys=keys[c])`).
        More than `max_canvases` canvases (constructor, default 32) are rendered in chunks of that many so that the key scratch
        stays bounded: host offsets let a chunk take its own slots only; with device offsets every chunk lights all n slots.
        Returns (C,h,w,3) uint8: numpy, or the device tensor with return_tensor=True."""
        dev = _device(self.device)
        off_dev = off_host = None
        if torch.is_tensor(offsets) and offsets.is_cuda:
            off_dev = offsets.to(dev, torch.int32).contiguous().reshape(-1)
            ncan = off_dev.numel() - 1
        else:
            off_host = np.asarray(offsets.cpu() if torch.is_tensor(offsets) else offsets).astype(np.int64).reshape(-1)
            ncan = len(off_host) - 1
        if ncan < 0:
            raise ValueError('offsets must hold C + 1 values, got none')
        if torch.is_tensor(canvases):
            img = canvases.to(dev, torch.uint8)
        else:
            img = torch.from_numpy(np.ascontiguousarray(canvases)).to(dev)
        if img.dim() == 3:
            img = img.unsqueeze(0).expand(ncan, -1, -1, -1)
        if img.dim() != 4 or img.shape[3] != 3 or img.shape[0] != ncan:
            raise ValueError('render_canvases paints %d canvases (C, h, w, 3), got %s' % (ncan, tuple(img.shape)))
        img = img.clone(memory_format=torch.contiguous_format)             # a copy: the input is not modified
        h, w = int(img.shape[1]), int(img.shape[2])
        verts_dev = _verts_dev(verts, dev)
        n = len(verts_dev)
        if n and (verts_dev.dim() != 3 or verts_dev.shape[2] != 3):
            raise ValueError('render_canvases takes (n, V, 3) vertices, got %s' % (tuple(verts_dev.shape),))
        if n and len(np.shape(triangles)) != 2:
            raise ValueError('render_canvases needs one triangle table (ntri, 3) for all meshes, got a list of topologies')
        if keys is not None and not (torch.is_tensor(keys) and keys.dtype == torch.int64 and keys.device == dev and keys.is_contiguous()
                                     and keys.numel() == ncan * h * w):
            raise ValueError('keys must be a contiguous int64 tensor of %d x %d x %d words on %s' % (ncan, h, w, dev))
        palette = np.asarray(mesh_colors).reshape(-1, 3)                   # (dtype kept: `_ambient` rounds as `__call__` does)
        if rows is None:
            nrow = n
            colors = palette[np.arange(n) % len(palette)]
        else:
            nrow = len(palette)
            colors = palette
            if not torch.is_tensor(rows):
                r = np.asarray(rows).reshape(-1)
                if len(r) != n or (n and (r.min() < 0 or r.max() >= nrow)):
                    raise ValueError('rows must hold %d indices into the %d rows of mesh_colors' % (n, nrow))
            rows = _dev_array(rows, torch.int32, dev).reshape(-1)
            if rows.numel() != n:
                raise ValueError('rows must hold %d indices, got %d' % (n, rows.numel()))
            rows = rows.clamp(0, max(nrow - 1, 0))                          # a device tensor is not read back: clamped instead
        if vert_colors is not None:
            vert_colors = _dev_array(vert_colors, torch.float32, dev)
            if vert_colors.dim() != 3 or vert_colors.shape[0] != nrow or (n and tuple(vert_colors.shape[1:]) != tuple(verts_dev.shape[1:])):
                raise ValueError('vert_colors must be (%d, V, 3) like the vertices %s, got %s'
                                 % (nrow, tuple(verts_dev.shape), tuple(vert_colors.shape)))
        if keys is not None and (n == 0 or ncan == 0):
            keys.zero_()
        if n == 0 or ncan == 0:
            return img if return_tensor else img.cpu().numpy()
        topo = _topology(triangles, verts_dev.shape[1], dev)
        amb = torch.from_numpy(self._ambient(colors)).pin_memory().to(dev, non_blocking=True)   # no stream sync
        if off_dev is None:
            off_host = np.clip(off_host, 0, n)
            off_dev = torch.from_numpy(off_host.astype(np.int32)).pin_memory().to(dev, non_blocking=True)
        step = self.max_canvases
        scratch = keys.view(ncan, h * w) if keys is not None else torch.empty((min(ncan, step), h * w), dtype=torch.int64, device=dev)
        lib = L.load()
        cfg = self._light_cfg(colors[:1])
        with torch.cuda.device(dev):
            for c0 in range(0, ncan, step):
                c1 = min(c0 + step, ncan)
                lo, hi, off = 0, n, off_dev[c0:c1 + 1]
                if off_host is not None and ncan > step:                    # this chunk's slots only
                    lo, hi = int(off_host[c0:c1 + 1].min()), int(off_host[c0:c1 + 1].max())
                    if hi <= lo:
                        if keys is not None:
                            scratch[c0:c1].zero_()
                        continue
                    off = torch.from_numpy((off_host[c0:c1 + 1] - lo).astype(np.int32)).pin_memory().to(dev, non_blocking=True)
                v = verts_dev[lo:hi]
                normals, light = torch.empty_like(v), torch.empty_like(v)
                if rows is None:
                    a, tex, rw = amb[lo:hi], (None if vert_colors is None else vert_colors[lo:hi]), None
                else:
                    a, tex, rw = amb, vert_colors, rows[lo:hi]
                k = scratch[c0:c1] if keys is not None else scratch[:c1 - c0]
                L.check(lib.romp_sim3dr_render_canvases(L.ptr(img[c0:c1]), c1 - c0, h, w, L.ptr(v), hi - lo, topo.nver, L.ptr(off),
                                                        L.ptr(topo.tri), topo.ntri, L.ptr(topo.adj_off), L.ptr(topo.adj_ent), L.ptr(a),
                                                        cfg, L.ptr(tex), L.ptr(rw), self.specular_exp, L.ptr(normals), L.ptr(light),
                                                        L.ptr(k), L.stream_ptr(dev)))
        return img if return_tensor else img.cpu().numpy()

    MAPS = ('person_map', 'tri_map', 'bary_map', 'attr_map', 'label_map', 'vert_visible', 'person_pixels')

    def maps(self, verts_list, triangles, image_shape, mesh_ids=None, attrs=None, attr_bg=0., vert_labels=None, want=None, keys=None):
        """What `__call__` decides per pixel, kept instead of painted (romp_sim3dr_maps, include/romp_hip_maps.h): the meshes
        verts_list (n,V,3) of ONE topology are painted in index order onto an image_shape[:2] = (h, w) canvas, each with a
        fresh z-buffer, so a pixel's winner is the highest mesh that covers it, inside that mesh the fragment of greatest
        depth, the lowest triangle on equal depth -- the fragment whose colour `__call__` shows.  Returns a dict of device
        tensors, the names of `want` (default: every map the inputs allow):
          person_map (h,w) int32: mesh_ids[mesh] (default: the mesh index), -1 on the background;
          tri_map (h,w) int32: the winning triangle, -1;
          bary_map (h,w,3) float32: its weights (w0,w1,w2) at the pixel, 0;
          attr_map (h,w,c) float32: (w0*a0 + w1*a1) + w2*a2 of the per-vertex attribute attrs (n,V,c), c <= 4 ((n,V): c = 1),
            attr_bg on the background.  The interpolation is affine in screen space, as the reference's depth buffer is, not
            perspective-correct: attrs = verts[..., 2:] reproduces that buffer, camera-space z gives metric depth, template
            coordinates a canonical-surface map;
          label_map (h,w) uint8: vert_labels (V,) at the winner's corner of greatest weight (the lowest corner on ties), 255;
          vert_visible (n,V) uint8: 1 iff the vertex is a corner of a triangle that wins at least one pixel;
          person_pixels (n,) int32: the number of pixels each mesh wins.
        Numpy or device input, as in `__call__`.  `keys`: the tensor a `__call__(..., keys=keys)` on these very meshes,
        triangles and canvas size has just filled: the raster pass is not run again.  No mesh: all background, no launch."""
        dev = _device(self.device)
        h, w = int(image_shape[0]), int(image_shape[1])
        verts = _verts_dev(verts_list, dev)
        if verts.dim() != 3 or verts.shape[2] != 3:
            raise ValueError('Sim3DR.maps takes (n, V, 3) vertices, got %s' % (tuple(verts.shape),))
        n, nver = verts.shape[:2]
        if n and len(np.shape(triangles)) != 2:
            raise ValueError('Sim3DR.maps needs one triangle table (ntri, 3) for all meshes, got a list of topologies')
        if attrs is not None:
            attrs = _dev_array(attrs, torch.float32, dev)
            attrs = attrs.unsqueeze(-1) if attrs.dim() == 2 else attrs
            if attrs.dim() != 3 or tuple(attrs.shape[:2]) != (n, nver) or not 1 <= attrs.shape[2] <= 4:
                raise ValueError('attrs must be (%d, %d, c) with 1 <= c <= 4, got %s' % (n, nver, tuple(attrs.shape)))
        if vert_labels is not None:
            vert_labels = _dev_array(vert_labels, torch.uint8, dev).reshape(-1)
            if n and vert_labels.numel() != nver:
                raise ValueError('vert_labels must hold %d labels, got %d' % (nver, vert_labels.numel()))
        if mesh_ids is not None:
            mesh_ids = _dev_array(mesh_ids, torch.int32, dev).reshape(-1)
            if mesh_ids.numel() != n:
                raise ValueError('mesh_ids must hold %d ids, got %d' % (n, mesh_ids.numel()))
        if want is None:
            want = [m for m in self.MAPS if (m != 'attr_map' or attrs is not None) and (m != 'label_map' or vert_labels is not None)]
        want = list(want)
        unknown = [m for m in want if m not in self.MAPS]
        if unknown:
            raise ValueError('unknown maps %s (known: %s)' % (unknown, ', '.join(self.MAPS)))
        if 'attr_map' in want and attrs is None:
            raise ValueError('attr_map needs attrs')
        if 'label_map' in want and vert_labels is None:
            raise ValueError('label_map needs vert_labels')
        c = attrs.shape[2] if attrs is not None else 1
        spec = {'person_map': ((h, w), torch.int32, -1), 'tri_map': ((h, w), torch.int32, -1), 'bary_map': ((h, w, 3), torch.float32, 0.),
                'attr_map': ((h, w, c), torch.float32, float(attr_bg)), 'label_map': ((h, w), torch.uint8, 255),
                'vert_visible': ((n, nver), torch.uint8, 0), 'person_pixels': ((n,), torch.int32, 0)}
        if n == 0:
            return {m: torch.full(spec[m][0], spec[m][2], dtype=spec[m][1], device=dev) for m in want}
        topo = _topology(triangles, nver, dev)
        ready = keys is not None
        keys = _keys(keys, h, w, dev)
        out = {m: torch.empty(spec[m][0], dtype=spec[m][1], device=dev) for m in want}
        with torch.cuda.device(dev):
            L.check(L.load().romp_sim3dr_maps(L.ptr(verts), n, nver, L.ptr(topo.tri), topo.ntri, h, w, L.ptr(mesh_ids), L.ptr(attrs), c,
                                              float(attr_bg), L.ptr(vert_labels), *[L.ptr(out.get(m)) for m in self.MAPS], L.ptr(keys),
                                              int(ready), L.stream_ptr(dev)))
        return out


def view_weak_perspective(verts, rx, ry, img_shape, expand_ratio=1.2):
    """vis_utils.py:26-51 (rotate_view_weak_perspective, bbox3D_center / scale computed) on the device, no host sync:
    verts (N,V,3) device tensor -> (verts rotated by Rx(rx) then Ry(ry) degrees, centred and scaled into the
    img_shape = (h, w) canvas, (N,V,3); bbox centre (3,); scale ()) as float32 device tensors."""
    v = verts.float().contiguous()
    dev = v.device
    h, w = img_shape
    out = torch.empty_like(v)
    center_scale = torch.empty(4, dtype=torch.float32, device=dev)
    work = torch.empty(7, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(L.load().romp_view_weak_perspective(L.ptr(v), v.shape[0], v.shape[1], float(rx), float(ry), int(h), int(w),
                                                    float(expand_ratio), L.ptr(out), L.ptr(center_scale), L.ptr(work), L.stream_ptr(dev)))
    return out, center_scale[:3], center_scale[3]


def turntable_views(verts, azimuths, tilts, img_shape, expand_ratio=1.2, order=None):
    """[romp_amd] K views of one scene for a turntable (romp_view_turntable, include/romp_hip_canvases.h), no host sync: verts
    (n,V,3) device tensor, centred on its bbox centre c0, spun by azimuths[k] degrees about the vertical axis and THEN tilted by
    tilts[k] degrees about the horizontal one (a number: the same tilt for every view), scaled by ONE scale for all views so that
    the largest |xy| / (w/2, h/2) of any view is 1 / expand_ratio, and shifted to the centre of the img_shape = (h, w) canvas.
    `order` (K,n) ints: slot j of view k holds mesh order[k, j] (the painter's order of that view); None: the mesh index.
    -> (views (K,n,V,3), c0 (3,), scale ()) float32 device tensors."""
    v = verts.float().contiguous()
    dev = v.device
    h, w = img_shape
    az = np.ascontiguousarray(np.asarray(azimuths, np.float64).reshape(-1))
    K = len(az)
    if v.dim() != 3 or v.shape[2] != 3 or v.shape[0] < 1 or v.shape[1] < 1 or K < 1:
        raise ValueError('turntable_views takes (n, V, 3) vertices and K >= 1 angles, got %s and %d' % (tuple(v.shape), K))
    ti = np.ascontiguousarray(np.broadcast_to(np.asarray(tilts, np.float64).reshape(-1), (K,)))
    n, nver = int(v.shape[0]), int(v.shape[1])
    if order is not None:
        order = _dev_array(order, torch.int32, dev)
        if tuple(order.shape) != (K, n):
            raise ValueError('order must be (%d, %d), got %s' % (K, n, tuple(order.shape)))
    out = torch.empty((K, n, nver, 3), dtype=torch.float32, device=dev)
    center_scale = torch.empty(4, dtype=torch.float32, device=dev)
    work = torch.empty(7, dtype=torch.int32, device=dev)
    dp = C.POINTER(C.c_double)
    with torch.cuda.device(dev):
        L.check(L.load().romp_view_turntable(L.ptr(v), n, nver, K, az.ctypes.data_as(dp), ti.ctypes.data_as(dp), L.ptr(order), int(h),
                                             int(w), float(expand_ratio), L.ptr(out), L.ptr(center_scale), L.ptr(work),
                                             L.stream_ptr(dev)))
    return out, center_scale[:3], center_scale[3]
