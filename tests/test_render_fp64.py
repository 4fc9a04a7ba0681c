"""Pixel-wise fp64 ground truth for apg_render_overlay (airpose_amd/csrc/render.hip): the mesh overlay behind airpose_amd.Renderer.

The reference (render_util.py) evaluates the contract of include/airpose_grad.h by brute force over pixels x faces in fp64 on exactly
the fp32 inputs and gives, per pixel, the set of acceptable answers; the derivation of every bar is in render_util.py's docstring.  No
pixel is left out of a check; ambiguity only widens what is accepted, and in every case at most 1 % of the pixels may have more than
one acceptable answer (asserted on the CPU).

CPU part: that cap; the fp32 emulation of the kernels' sequence is accepted on every case; each mutation of it is rejected on at least
one case (the exact lattice for the two that only differ on exact ties and zeros).
GPU part: the exact lattice (coverage of every pixel centre on edges and vertices, depth == 2.0, lowest face, reversed winding draws
nothing); every tolerance case; a NaN vertex; a full-size frame whose 40 x 40 window equals the render of the window alone bit for
bit and is judged in fp64.  Every GPU call runs twice into fresh buffers between NaN guard bands: bit-equal, guards untouched, inputs
unchanged (render_util.gpu_render).

The full-size windows are placed on the CPU (the leftmost point of each mesh's outline) and are cases like the others: the cap, the
emulation and the GPU judgement apply to them.
"""
import numpy as np
import pytest

import render_util as RU

CAP = 0.01


def _dev():
    import torch
    return torch.device("cuda", 0)


# ------------------------------------------------------------------------------------------------ CPU
@pytest.mark.parametrize("name", RU.CASE_NAMES)
def test_at_most_one_percent_of_the_pixels_are_ambiguous_and_the_emulation_is_accepted(name):
    case = RU.tolerance_cases()[name]
    for k in range(case["n"]):
        sc = RU.scan(case, k)
        print("%s[%d]: ambiguous %.4f %%, covered by a sure face %.1f %%" % (name, k, 100 * sc["ambiguous"], 100 * sc["covered"]))
        assert sc["ambiguous"] <= CAP
        if k == 0:
            assert sc["covered"] >= case["cover"]
        bad = RU.judge(case, k, *RU.emulate(case, k))
        assert RU.accepted(bad), (name, k, bad)


def test_case_names_are_the_cases():
    assert tuple(sorted(RU.tolerance_cases())) == tuple(sorted(RU.CASE_NAMES))


def test_lattice_on_the_cpu_inclusive_covers_exactly_and_exclusive_leaves_332_holes():
    case, cols, rows = RU.lattice_case()
    covered, want_face = RU.lattice_expected(case, cols, rows)
    region = np.zeros_like(covered)
    region[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1] = True
    assert (covered == region).all()
    face, depth, _ = RU.emulate(case, 0)                                  # fp32
    assert ((face >= 0) == region).all() and (depth[region] == 2.0).all() and (depth[~region] == 0).all()
    assert (face == want_face).all()
    g = RU.geometry(case, 0)                                               # fp64: w_k <= 0 for some face, exactly
    dx, dy = RU.rays(case)
    X, Y = np.tile(dx, case["H"]), np.repeat(dy, case["W"])
    w = [X[:, None] * n[:, 0] + Y[:, None] * n[:, 1] + n[:, 2] for n in g["n"]]
    inc = ((w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0) & (g["det"] < 0)).any(1).reshape(case["H"], case["W"])
    exc = ((w[0] < 0) & (w[1] < 0) & (w[2] < 0) & (g["det"] < 0)).any(1).reshape(case["H"], case["W"])
    assert (inc == region).all()
    assert int((region & ~exc).sum()) == 332
    face_x, _, _ = RU.emulate(case, 0, "exclusive_edge")
    assert int((region & (face_x < 0)).sum()) == 332


def _rejected_somewhere(mutation, names):
    for name in names:
        case = RU.tolerance_cases()[name]
        for k in range(case["n"]):
            if not RU.accepted(RU.judge(case, k, *RU.emulate(case, k, mutation))):
                return True
    return False


@pytest.mark.parametrize("mutation,names", [("no_culling", ("near_inside_culled",)), ("farthest_wins", ("ellipsoids_45x67_n1_null",)),
                                            ("no_half_pixel", ("ellipsoids_45x67_n1_null",)),
                                            ("centre_swapped", ("ellipsoids_45x67_n1_null",))])
def test_mutations_are_rejected_by_the_fp64_reference(mutation, names):
    assert _rejected_somewhere(mutation, names)


@pytest.mark.parametrize("mutation", ["exclusive_edge", "tie_to_higher_face"])
def test_mutations_that_differ_on_exact_ties_are_rejected_by_the_lattice(mutation):
    case, cols, rows = RU.lattice_case()
    covered, want_face = RU.lattice_expected(case, cols, rows)
    face, _, _ = RU.emulate(case, 0, mutation)
    assert not (face == want_face).all()


def test_every_mutation_is_tried():
    tried = {"no_culling", "farthest_wins", "no_half_pixel", "centre_swapped", "exclusive_edge", "tie_to_higher_face"}
    assert tried == set(RU.MUTATIONS)


# ------------------------------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_gpu_exact_lattice():
    case, cols, rows = RU.lattice_case()
    covered, want_face = RU.lattice_expected(case, cols, rows)
    rgb, depth, face = RU.gpu_render(case, _dev())
    assert ((face[0] >= 0) == covered).all()
    assert (depth[0][covered] == 2.0).all() and (depth[0][~covered] == 0).all()
    assert (face[0] == want_face).all()
    assert np.array_equal(rgb[0][:, ~covered].view(np.int32), case["bg"][0][:, ~covered].view(np.int32))
    rev, _, _ = RU.lattice_case(reverse=True)
    rgb, depth, face = RU.gpu_render(rev, _dev())
    assert np.array_equal(rgb.view(np.int32), rev["bg"].view(np.int32))
    assert (depth.view(np.int32) == 0).all() and (face == -1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", RU.CASE_NAMES)
def test_gpu_every_pixel_is_an_acceptable_answer(name):
    case = RU.tolerance_cases()[name]
    rgb, depth, face = RU.gpu_render(case, _dev())
    for k in range(case["n"]):
        bad = RU.judge(case, k, face[k], depth[k], rgb[k])
        print(name, k, bad, "shown %.1f %%" % (100 * (face[k] >= 0).mean()))
        assert RU.accepted(bad), (name, k, bad)
        assert (face[k] >= 0).mean() >= (case["cover"] if k == 0 else 0.0)


@pytest.mark.gpu
def test_gpu_black_background_and_optional_outputs():
    case = dict(RU.tolerance_cases()["ellipsoids_45x67_n1_null"], bg=None)
    case["name"] = "ellipsoids_45x67_n1_null_black"
    rgb, depth, face = RU.gpu_render(case, _dev())
    assert RU.accepted(RU.judge(case, 0, face[0], depth[0], rgb[0]))
    only, none_d, none_f = RU.gpu_once(case, _dev(), want_depth=False, want_face=False)
    assert none_d is None and none_f is None and np.array_equal(only.view(np.int32), rgb.view(np.int32))


@pytest.mark.gpu
def test_gpu_a_nan_vertex_removes_exactly_the_faces_that_use_it():
    base = RU.tolerance_cases()["ellipsoids_48x64_n3_null"]
    bad_vertex = int(base["faces"][len(base["faces"]) // 3, 1])
    verts = base["verts"].copy()
    verts[:, bad_vertex, 1] = np.nan
    with_nan = dict(base, verts=verts, name="nan_vertex")
    keep = ~(base["faces"] == bad_vertex).any(1)
    assert 0 < (~keep).sum() < 16
    without = dict(base, faces=np.ascontiguousarray(base["faces"][keep]), name="nan_vertex_faces_removed")
    a, b = RU.gpu_render(with_nan, _dev()), RU.gpu_render(without, _dev())
    assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32))       # rgb
    assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32))       # depth
    old_index = np.concatenate([np.nonzero(keep)[0], [-1]])               # the face indices of `without` in the full table
    assert np.array_equal(a[2], old_index[b[2]])
    assert (a[2] >= 0).mean() > 0.1
    for k in range(base["n"]):                                            # and it is a right answer for the remaining faces
        assert RU.accepted(RU.judge(without, k, b[2][k], b[1][k], b[0][k]))


@pytest.mark.gpu
def test_gpu_full_size_window_equals_the_window_alone_and_the_fp64_reference():
    """the windows are cases of their own (placed on the CPU from the fp64 projection: the 1 % cap and the emulation are asserted
    for them with the other cases, and the GPU render of each alone is judged there); here the full frame must show the same bits"""
    full = RU.full_size_case()
    S = RU.WINDOW
    rgb, depth, face = RU.gpu_render(full, _dev())
    assert 0.005 < (face >= 0).mean() < 0.5
    for k in range(full["n"]):
        win, i0, j0 = RU.window_case(full, k)
        wrgb, wdepth, wface = RU.gpu_render(win, _dev())
        shown = (wface[0] >= 0).mean()
        assert 0.1 < shown < 0.9, shown                                    # the window lies across the silhouette
        assert np.array_equal(wface[0], face[k, i0:i0 + S, j0:j0 + S])
        assert np.array_equal(wdepth[0].view(np.int32), np.ascontiguousarray(depth[k, i0:i0 + S, j0:j0 + S]).view(np.int32))
        assert np.array_equal(wrgb[0].view(np.int32), np.ascontiguousarray(rgb[k, :, i0:i0 + S, j0:j0 + S]).view(np.int32))
        bad = RU.judge(RU.tolerance_cases()[win["name"]], 0, wface[0], wdepth[0], wrgb[0])
        print("window", k, (i0, j0), bad, "shown %.1f %%" % (100 * shown))
        assert RU.accepted(bad), bad
