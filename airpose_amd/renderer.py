"""The reference's utils/renderer.py Renderer (pyrender, trimesh, an off-screen GL context, one mesh at a time on the CPU) as one
hand-written gfx950 pass over the whole batch: Renderer.

summaries() of the reference trainers (copenet_twoview.py:445-500 and the same method of copenet_singleview.py, hmr.py, muhmr.py and
the copenet_real trainers; bundle_adj.py:232-239 and aircapfit.py:115-122 for the AirPose+ fits) calls Renderer.visualize_tb on
vertices that are already on the GPU.  apg_render_overlay (csrc/render.hip, include/airpose_grad.h) casts one ray per pixel against
the posed meshes on the device and composites over the images; nothing moves to the host.  There is no fallback: a missing library is
an error.

pyrender is absent here, so two things are UNPINNED: the half-pixel convention (a pixel's ray goes through
its centre, GL's convention) and the shading, which is a stand-in without pyrender's specular lobe -- ambient 0.5 (the scene's) plus
3 (1 - 0.2) / pi of Lambert term (three unit directional lights along the view axis on a material of metallic factor 0.2).  The
geometry -- which face a pixel shows, at which depth -- is pinned by the contract in include/airpose_grad.h.
"""
import math

import numpy as np
import torch

from . import _native_grad as G
from . import _stream_metric as S

AMBIENT = 0.5
DIFFUSE = 3.0 * (1.0 - 0.2) / math.pi
ZNEAR, ZFAR = 0.05, 100.0                # pyrender's defaults


def vertex_face_table(faces, num_vertices):
    """(offsets (V + 1), entries) int32: the faces of vertex v are entries[offsets[v]:offsets[v + 1]], ascending; a face is listed
    once per distinct vertex it uses"""
    f = np.asarray(faces, np.int64)
    idx = np.arange(f.shape[0], dtype=np.int64)
    keep1 = f[:, 1] != f[:, 0]
    keep2 = (f[:, 2] != f[:, 0]) & (f[:, 2] != f[:, 1])
    v = np.concatenate([f[:, 0], f[keep1, 1], f[keep2, 2]])
    k = np.concatenate([idx, idx[keep1], idx[keep2]])
    order = np.lexsort((k, v))
    offsets = np.zeros(num_vertices + 1, np.int64)
    np.cumsum(np.bincount(v, minlength=num_vertices), out=offsets[1:])
    return offsets.astype(np.int32), k[order].astype(np.int32)


def make_grid(images, nrow=8, padding=2):
    """torchvision.utils.make_grid's layout on an (n, C, H, W) tensor: rows of nrow images, `padding` pixels of 0 around and between
    them; one image comes back as it is"""
    n, C, H, W = images.shape
    if n == 1:
        return images[0]
    xmaps = min(int(nrow), n)
    ymaps = (n + xmaps - 1) // xmaps
    h, w = H + padding, W + padding
    grid = images.new_zeros((C, h * ymaps + padding, w * xmaps + padding))
    for k in range(n):
        y, x = divmod(k, xmaps)
        grid[:, y * h + padding:y * h + padding + H, x * w + padding:x * w + padding + W] = images[k]
    return grid


class Renderer(object):
    """Renderer(focal_length=[1475, 1475], img_res=[224, 224], center=None, faces=None): both reference constructors (copenet's has no
    `center` and uses img_res // 2, which center=None gives; copenet_real's passes (cx, cy)).  img_res is (width, height).

    faces: the mesh's (F, 3) integer array or tensor (SMPLX(...).faces as it is); validated once here.

    visualize_tb(vertices (n, V, 3), camera_translation (n, 3), camera_rotation (n, 3, 3), images (n, 3, H, W), nrow=5,
                 color=(0.8, 0.3, 0.3, 1.0), padding=2) -> (3, Hg, Wg) grid on the inputs' device; rows of the last three past n
        are ignored, as the reference's loop ignores them
        (copenet_real's variant is color=(0.3, 0.3, 0.8, 1.0), padding=0)
    __call__(vertices (V, 3), camera_translation (3), camera_rotation (3, 3), image (H, W, 3), color=...) -> (H, W, 3)
    render(vertices, camera_translation=None, camera_rotation=None, images=None, color=...) -> rgb (n, 3, H, W), depth (n, H, W),
        face (n, H, W) int32; None is a zero translation, the identity, a black background

    CUDA float tensors only; a call runs on the current stream and never synchronises the host.  The workspace (the z-buffer is in
    it) is kept per (device, n, V) and shared by all calls of this object, so two calls of one Renderer on different streams must
    be ordered by the caller; use one Renderer per stream to overlap them.
    """

    def __init__(self, focal_length=[1475, 1475], img_res=[224, 224], center=None, faces=None):
        if faces is None:
            raise RuntimeError("Renderer: faces is required (the mesh's (F, 3) vertex indices)")
        self.focal_length = [float(focal_length[0]), float(focal_length[1])]
        self.img_res = [int(img_res[0]), int(img_res[1])]
        if self.img_res[0] < 1 or self.img_res[1] < 1:
            raise RuntimeError("Renderer: img_res must be positive, got %s" % (img_res,))
        self.camera_center = [self.img_res[0] // 2, self.img_res[1] // 2] if center is None else [float(center[0]), float(center[1])]
        f = faces.detach().cpu().numpy() if torch.is_tensor(faces) else np.asarray(faces)
        if f.dtype.kind not in "iu":
            raise RuntimeError("Renderer: faces must be integers, got %s" % f.dtype)
        if f.ndim != 2 or f.shape[1] != 3 or f.shape[0] < 1:
            raise RuntimeError("Renderer: faces must be (F, 3) with F >= 1, got %s" % (tuple(f.shape),))
        f = f.astype(np.int64)
        if f.min() < 0 or f.max() >= 1 << 24:
            raise RuntimeError("Renderer: faces must index vertices 0 .. 2^24 - 1, got %d .. %d" % (f.min(), f.max()))
        self.faces = f.astype(np.int32)
        self._max_index = int(f.max())
        self._tables = {}                # (device, V) -> faces, csr offsets, csr entries on the device
        self._ws = {}                    # (device, n, V) -> workspace

    def _table(self, dev, V):
        key = (dev, V)
        if key not in self._tables:
            if self._max_index >= V:
                raise RuntimeError("Renderer: faces index vertex %d, the vertices given are %d" % (self._max_index, V))
            off, ent = vertex_face_table(self.faces, V)
            self._tables[key] = tuple(torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (self.faces, off, ent))
        return self._tables[key]

    def render(self, vertices, camera_translation=None, camera_rotation=None, images=None, color=(0.8, 0.3, 0.3, 1.0),
               ambient=AMBIENT, diffuse=DIFFUSE, want_depth=True, want_face=True):
        if not torch.is_tensor(vertices) or vertices.dim() != 3 or vertices.shape[2] != 3 or vertices.shape[1] < 1:
            raise RuntimeError("Renderer: vertices must be an (n, V, 3) tensor, got %s" % (
                tuple(vertices.shape) if torch.is_tensor(vertices) else type(vertices).__name__,))
        n, V = vertices.shape[0], vertices.shape[1]
        W, H = self.img_res
        given = [(vertices, (n, V, 3), "vertices"), (camera_translation, (n, 3), "camera_translation"),
                 (camera_rotation, (n, 3, 3), "camera_rotation"), (images, (n, 3, H, W), "images")]
        for x, shape, name in given:                     # what every tensor must be first, then where it must live
            if x is not None:
                S.check_what("Renderer", x, shape, name)
        v = S.check_where("Renderer", vertices, None, "vertices", "the vertices")
        dev = v.device
        t, R, bg = (None if x is None else S.check_where("Renderer", x, dev, name, "the vertices") for x, _, name in given[1:])
        L = G.lib()
        with torch.cuda.device(dev):
            faces, off, ent = self._table(dev, V)
            F = faces.shape[0]
            rgb = torch.empty(n, 3, H, W, device=dev, dtype=torch.float32)
            depth = torch.empty(n, H, W, device=dev, dtype=torch.float32) if want_depth else None
            face = torch.empty(n, H, W, device=dev, dtype=torch.int32) if want_face else None
            nbytes = L.apg_render_workspace_bytes(n, H, W, V, F)
            if nbytes < 0:
                raise RuntimeError("Renderer: n = %d, %d x %d, V = %d, F = %d is outside apg_render_overlay's limits" % (n, H, W, V, F))
            ws = self._ws.get((dev, n, V))
            if ws is None or ws.numel() * 8 < nbytes:
                ws = self._ws[(dev, n, V)] = torch.empty((nbytes + 7) // 8, device=dev, dtype=torch.int64)
            vp = G.vp
            G.check(L.apg_render_overlay(n, V, F, H, W, vp(v), vp(faces), vp(off), vp(ent), ent.numel(), vp(R), vp(t),
                                         self.focal_length[0], self.focal_length[1], float(self.camera_center[0]),
                                         float(self.camera_center[1]), ZNEAR, ZFAR, vp(bg), float(color[0]), float(color[1]),
                                         float(color[2]), float(ambient), float(diffuse), vp(rgb), vp(depth), vp(face), vp(ws),
                                         ws.numel() * 8, G.stream(dev)), "apg_render_overlay")
        return rgb, depth, face

    def visualize_tb(self, vertices, camera_translation, camera_rotation, images, nrow=5, color=(0.8, 0.3, 0.3, 1.0), padding=2):
        # the reference walks range(vertices.shape[0]) and its callers pass translations and rotations for the whole batch beside
        # the four sampled meshes (copenet_twoview.py:464-467): rows past the meshes are ignored here as well
        n = vertices.shape[0] if torch.is_tensor(vertices) and vertices.dim() == 3 else None
        rows = lambda x: x[:n] if n is not None and torch.is_tensor(x) and x.dim() >= 1 and x.shape[0] > n else x
        rgb, _, _ = self.render(vertices, rows(camera_translation), rows(camera_rotation), rows(images), color=color,
                                want_depth=False, want_face=False)
        return make_grid(rgb, nrow, padding)

    def __call__(self, vertices, camera_translation, camera_rotation, image, color=(0.8, 0.3, 0.3, 1.0)):
        if not torch.is_tensor(image) or image.dim() != 3 or image.shape[2] != 3:
            raise RuntimeError("Renderer: image must be an (H, W, 3) tensor")
        if not torch.is_tensor(vertices) or vertices.dim() != 2:
            raise RuntimeError("Renderer: vertices must be a (V, 3) tensor")
        rgb, _, _ = self.render(vertices[None], camera_translation[None], camera_rotation[None], image.permute(2, 0, 1)[None],
                                color=color, want_depth=False, want_face=False)
        return rgb[0].permute(1, 2, 0)
