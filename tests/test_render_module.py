"""airpose_amd.Renderer (airpose_amd/renderer.py): the reference's utils/renderer.py interface on apg_render_overlay.  The pixels are
judged in test_render_fp64.py; here: visualize_tb's grid layout against a known-answer layout, __call__ against the batched form,
SMPLX(...).faces taken as it is, the workspace kept between calls, and what is refused."""
import numpy as np
import pytest
import torch

import render_util as RU


def _scene(n, H, W, dev):
    v, f = RU.two_ellipsoids()
    verts = torch.from_numpy(np.stack([v + np.float32([0.1 * k, 0, 0]) for k in range(n)])).to(dev)
    t = torch.tensor([[0.0, 0.0, 3.0 + 0.2 * k] for k in range(n)], device=dev)
    R = torch.from_numpy(np.stack([RU.rot((0, 1, 0), 0.3 * k) for k in range(n)]).astype(np.float32)).to(dev)
    images = torch.from_numpy(RU.background(n, H, W, 5)).to(dev)
    return verts, t, R, images, f


def _known_grid(imgs, nrow, padding):
    """make_grid's layout written cell by cell: image k sits at row k // cols, column k % cols of cells of (H + padding) x (W + padding),
    offset by `padding`; everything else is 0; one image comes back as it is"""
    n, C, H, W = imgs.shape
    if n == 1:
        return imgs[0]
    cols = min(nrow, n)
    rows = -(-n // cols)
    out = np.zeros((C, rows * (H + padding) + padding, cols * (W + padding) + padding), np.float32)
    for k in range(n):
        r, c = k // cols, k % cols
        out[:, padding + r * (H + padding):padding + r * (H + padding) + H, padding + c * (W + padding):padding + c * (W + padding) + W] = imgs[k]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n,nrow,kw", [(7, 5, {}), (7, 5, dict(color=(0.3, 0.3, 0.8, 1.0), padding=0)), (4, 2, dict(padding=3)),
                                       (3, 8, {}), (1, 5, {})])
def test_visualize_tb_grid_layout(n, nrow, kw):
    from airpose_amd import Renderer
    dev = torch.device("cuda", 0)
    H, W = 30, 44
    verts, t, R, images, f = _scene(n, H, W, dev)
    r = Renderer(focal_length=[40.0, 40.0], img_res=[W, H], faces=f)
    grid = r.visualize_tb(verts, t, R, images, nrow=nrow, **kw)
    rgb, depth, face = r.render(verts, t, R, images, color=kw.get("color", (0.8, 0.3, 0.3, 1.0)))
    assert grid.device == verts.device and grid.dtype == torch.float32
    want = _known_grid(rgb.cpu().numpy(), nrow, kw.get("padding", 2))
    assert tuple(grid.shape) == want.shape
    assert np.array_equal(grid.cpu().numpy().view(np.int32), want.view(np.int32))
    shown = (face >= 0)
    assert 0.05 < float(shown.float().mean()) < 0.9
    # where nothing is shown the image's bits
    assert torch.equal(rgb.permute(0, 2, 3, 1)[~shown], images.permute(0, 2, 3, 1)[~shown])
    assert torch.equal(depth > 0, shown)
    # the reference's callers pass translations and rotations for the whole batch beside the sampled meshes: the rest is ignored
    more = lambda x: torch.cat([x, x[:1].expand(3, *x.shape[1:])])
    assert torch.equal(r.visualize_tb(verts, more(t), more(R), more(images), nrow=nrow, **kw), grid)


@pytest.mark.gpu
def test_call_takes_hwc_and_equals_the_batched_form():
    from airpose_amd import Renderer
    dev = torch.device("cuda", 0)
    H, W = 30, 44
    verts, t, R, images, f = _scene(3, H, W, dev)
    r = Renderer(focal_length=[40.0, 40.0], img_res=[W, H], center=[20.5, 16.25], faces=torch.from_numpy(f))
    assert r.camera_center == [20.5, 16.25]
    rgb, _, _ = r.render(verts, t, R, images, color=(0.3, 0.3, 0.8, 1.0))
    for k in range(3):
        one = r(verts[k], t[k], R[k], images[k].permute(1, 2, 0), color=(0.3, 0.3, 0.8, 1.0))
        assert tuple(one.shape) == (H, W, 3)
        assert torch.equal(one, rgb[k].permute(1, 2, 0))
    # None is the identity / zero / black
    posed = torch.einsum("nij,nvj->nvi", R, verts) + t[:, None]
    a, _, fa = r.render(posed)
    b, _, fb = r.render(posed, torch.zeros_like(t), torch.eye(3, device=dev).expand(3, 3, 3).contiguous(), torch.zeros_like(images))
    assert torch.equal(a, b) and torch.equal(fa, fb)


@pytest.mark.gpu
def test_smplx_faces_are_accepted_as_given_and_the_workspace_is_reused(smplx_model):
    from airpose_amd import Renderer, smplx
    dev = torch.device("cuda", 0)
    body = smplx.SMPLX(model_data=smplx_model)
    r = Renderer(img_res=[64, 48], focal_length=[100.0, 100.0], faces=body.faces)
    assert r.camera_center == [32, 24]
    V = int(np.asarray(smplx_model["v_template"]).shape[0])
    verts = torch.from_numpy(np.asarray(smplx_model["v_template"], np.float32))[None].to(dev).repeat(2, 1, 1)
    t = torch.tensor([[0.0, 0.0, 2.5], [0.1, 0.0, 3.0]], device=dev)
    R = torch.eye(3, device=dev).expand(2, 3, 3).contiguous()
    images = torch.from_numpy(RU.background(2, 48, 64, 9)).to(dev)
    rgb1, d1, f1 = r.render(verts, t, R, images)
    ws = r._ws[(verts.device, 2, V)]
    ptr = ws.data_ptr()
    rgb2, d2, f2 = r.render(verts, t, R, images)
    assert r._ws[(verts.device, 2, V)].data_ptr() == ptr and len(r._ws) == 1 and len(r._tables) == 1
    assert torch.equal(rgb1, rgb2) and torch.equal(d1, d2) and torch.equal(f1, f2)
    assert int(f1.max()) < body.faces.shape[0] and float((f1 >= 0).float().mean()) > 0.01


def test_package_table_equals_the_restated_one():
    from airpose_amd.renderer import vertex_face_table
    f = np.concatenate([RU.two_ellipsoids()[1], np.int32([[3, 3, 9], [5, 7, 5], [8, 8, 8]])])
    off, ent = vertex_face_table(f, 1100)
    vv, ff = RU.vertex_faces(f)
    assert np.array_equal(ent, ff) and np.array_equal(off, np.concatenate([[0], np.cumsum(np.bincount(vv, minlength=1100))]))
    assert len(ent) == 3 * len(f) - 4                    # the repeated indices are listed once


def test_refusals_on_the_cpu():
    import airpose_amd
    from airpose_amd.renderer import Renderer
    assert airpose_amd.Renderer is Renderer
    v, f = RU.two_ellipsoids()
    r = Renderer(img_res=[44, 30], faces=f)
    V = len(v)
    with pytest.raises(RuntimeError, match="CUDA"):
        r.render(torch.zeros(1, V, 3))
    with pytest.raises(RuntimeError, match="CUDA"):
        r.visualize_tb(torch.zeros(2, V, 3), torch.zeros(2, 3), torch.zeros(2, 3, 3), torch.zeros(2, 3, 30, 44))
    with pytest.raises(RuntimeError, match="vertices"):
        r.render(torch.zeros(V, 3))
    with pytest.raises(RuntimeError, match="camera_translation"):
        r.render(torch.zeros(2, V, 3), torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="floating"):
        r.render(torch.zeros(2, V, 3, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="image"):
        r(torch.zeros(V, 3), torch.zeros(3), torch.eye(3), torch.zeros(3, 30, 44))
    for bad, what in ((None, "required"), (f.astype(np.float32), "integers"), (f[:, :2], r"\(F, 3\)"), (f.reshape(-1), r"\(F, 3\)"),
                      (-f, "index"), (np.zeros((0, 3), np.int32), r"\(F, 3\)")):
        with pytest.raises(RuntimeError, match=what):
            Renderer(faces=bad)
    with pytest.raises(RuntimeError, match="img_res"):
        Renderer(img_res=[0, 10], faces=f)


@pytest.mark.gpu
def test_refusals_on_the_gpu():
    from airpose_amd import Renderer
    dev = torch.device("cuda", 0)
    v, f = RU.two_ellipsoids()
    r = Renderer(img_res=[44, 30], faces=f)
    with pytest.raises(RuntimeError, match="index vertex"):
        r.render(torch.zeros(1, len(v) - 1, 3, device=dev))
    with pytest.raises(RuntimeError, match="images"):
        r.render(torch.zeros(1, len(v), 3, device=dev), images=torch.zeros(1, 3, 44, 30, device=dev))
    with pytest.raises(RuntimeError, match="CUDA"):
        r.render(torch.zeros(1, len(v), 3, device=dev), torch.zeros(1, 3))
