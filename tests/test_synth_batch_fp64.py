"""apg_synth_batch and apg_synth_crops (airpose_amd/csrc/synth_batch.hip) through the C ABI against the restatement of
aerialpeople_crop.__getitem__ in synth_batch_util.py: frames of 120 x 160, margin 20, a canvas of 96 x 128 (origin "region") or the
frame itself (origin "frame"), n in {1, 5}, V in {1, 67, 10475}, J in {22, 127}, joints at z >= 2, and the planted boxes of
synth_batch_util.PLANTED.  Every output is pre-filled with NaN / -77 and must be overwritten.

Exact: crops, crop_info, status, the flips; intr and extr are copies bit for bit; bb[..., 2] is bit for bit the scale
ap_preprocess_crops writes for the same box; the images, scales and pads of apg_synth_crops are bit for bit ap_preprocess_crops' on the
same boxes; a shuffled suffix row is bit for bit the unshuffled row of camera flip ^ s; two calls give the same bits.
bb[..., :2]: real_batch_util.bb_bar (half an ulp at bb + 1 from the divide, half an ulp at bb from the subtract).
The fp32 chains, with u = 2^-24 (one rounding of v is at most u |v|) and a factor 1 + 2^-20 for the second order; each bar is per
element, computed in fp64 from the chain's own exact fp32 inputs (synth_batch_util.rigid_bar, project_bar, crop_bar, rodrigues_bar):
  transforms       X = fl(fl(fl(a + b) + c) + t), a = fl(R0 x), b = fl(R1 y), c = fl(R2 z), from the records:
                   u (|a| + |b| + |c| + |a + b| + |a + b + c| + |X|); orient_rel the same without t
  projection       j = fl(fl(f fl(x / z)) + c) from the kernel's own joints_rel: u (2 |f x / z| + |j|)
  j2d_crop         r = fl(s fl(j - fl(fl(b + 1) c))) from the kernel's own j2d and bb: u (s (2 |(b + 1) c| + |j - (b + 1) c|) + |r|)
  smplpose_rotmat  lbs.batch_rodrigues with sinf / cosf taken as 4 ulp: |k| ds + 5.5 u |s k| + |kk| dc + 12 u c1 |kk| + u (|I + s k| + |R|)
                   (the derivation is rodrigues_bar's docstring)
The projection and the crop pixels are held to fp64 on the kernel's OWN upstream outputs, so each chain answers for its own roundings
only; that those upstream outputs are right is the transforms' and bb's own check, and `differs` compares every output with the
restatement end to end at 1e-3.  Beside each error the test prints the error of the same chain evaluated in numpy fp32 on the host
(the floor) and whether the kernel is bit-equal to that evaluation.  Measured on the CPU (tests/test_synth_batch_abi.py asserts it
for its shapes, this file for every shape): the floor's worst element reaches between 0.12 (the rotations at n = 1) and 0.96 (the
vertices at V = 10475) of its bar, so no bar is wider than 9 times the floor (16 times is the limit).  On an MI355X the kernel is
that evaluation bit for bit in every chain but the rotations (the device's sinf / cosf are not numpy's), which reach 0.13 .. 0.24 of
their bar.

The hostile test runs apg_synth_batch ONLY, which reads no frame: it copies `crops` to the host and asserts the invariant for every
row; nothing that reads a frame is launched from those boxes.  Everywhere else the fixture checks the boxes on the host before the
first apg_synth_crops launch."""
import numpy as np
import pytest
import torch

import real_batch_util as RU
import synth_batch_util as U
from loss_util import dev  # noqa: F401  (the fixture of the GPU tests)

F32_OUT = {"bb": (3,), "intr": (3, 3), "extr": (4, 4), "verts_rel": ("V", 3), "joints_rel": ("J", 3), "orient_rel": (3, 3),
           "trans_rel": (3,), "j2d": ("J", 2), "j2d_crop": ("J", 2)}
ORDER = ("crops", "crop_info", "status", "flip", "bb", "intr", "extr", "verts_rel", "joints_rel", "orient_rel", "trans_rel", "j2d",
         "j2d_crop", "pose_rotmat")
IN_ORDER = ("bb", "intr", "extr", "smplpose", "smpl_vertices_wrt_origin", "smpl_joints_wrt_origin", "smplorient_rotmat_wrt_origin", "smpltrans")


def canvas_of(origin):
    return (U.HC, U.WC) if origin == "region" else (U.H, U.W)


def run_batch(dev, rec, index, origin="region", seed=U.SEED, epoch=0, jitter=True, shuffle=True, margin=U.MARGIN):
    """one apg_synth_batch call -> dict of device tensors, all pre-filled"""
    from airpose_amd import _native_grad as G
    n, V, J = rec["bb"].shape[0], rec["smpl_vertices_wrt_origin"].shape[2], rec["smpl_joints_wrt_origin"].shape[2]
    Hc, Wc = canvas_of(origin)
    f32 = lambda *s: torch.full(s, float("nan"), device=dev, dtype=torch.float32)          # (nothing may be left as it was)
    i32 = lambda *s: torch.full(s, -77, device=dev, dtype=torch.int32)
    dims = {"V": V, "J": J}
    o = dict(crops=i32(2, n, 4), crop_info=i32(2, n, 2, 2), status=i32(2, n), flip=i32(n), pose_rotmat=f32(n, 21, 3, 3))
    o.update({k: f32(2, n, *[dims.get(d, d) for d in tail]) for k, tail in F32_OUT.items()})
    ins = [torch.from_numpy(np.ascontiguousarray(index)).to(dev)] + [torch.from_numpy(np.ascontiguousarray(rec[k])).to(dev) for k in IN_ORDER]
    with torch.cuda.device(dev):
        G.check(G.lib().apg_synth_batch(n, V, J, U.H, U.W, Hc, Wc, int(margin), U.ORIGINS[origin], int(jitter), int(shuffle), U.FOCAL[0],
                                        U.FOCAL[1], seed, epoch, *[G.vp(t) for t in ins], *[G.vp(o[k]) for k in ORDER], G.stream(dev)),
                "apg_synth_batch")
    return o


def check_invariant(crops, Hc, Wc):
    y0, y1, x0, x1 = np.asarray(crops).reshape(-1, 4).T.astype(np.int64)
    assert (0 <= y0).all() and (y0 < y1).all() and (y1 <= Hc).all(), crops
    assert (0 <= x0).all() and (x0 < x1).all() and (x1 <= Wc).all(), crops


def run_crops(dev, frames, o, bgr=True):
    """one apg_synth_crops call on the boxes and flips of `o` (device tensors), AFTER the boxes have been checked on the host"""
    from airpose_amd import _native_grad as G
    n, Hc, Wc = frames.shape[1], frames.shape[2], frames.shape[3]
    check_invariant(o["crops"].cpu().numpy(), Hc, Wc)
    assert set(o["flip"].cpu().tolist()) <= {0, 1}
    im = torch.full((2, n, 3, 224, 224), float("nan"), device=dev, dtype=torch.float32)
    scale = torch.full((2, n), float("nan"), device=dev, dtype=torch.float32)
    pad = torch.full((2, n, 2), -77, device=dev, dtype=torch.int32)
    with torch.cuda.device(dev):
        G.check(G.lib().apg_synth_crops(n, Hc, Wc, int(bgr), G.vp(frames), G.vp(o["crops"]), G.vp(o["flip"]), G.vp(im), G.vp(scale),
                                        G.vp(pad), G.stream(dev)), "apg_synth_crops")
    return dict(im=im, scale=scale, pad=pad)


def frames_for(dev, n, origin):
    Hc, Wc = canvas_of(origin)
    g = torch.Generator().manual_seed(4400 + n)
    return torch.randint(0, 256, (2, n, Hc, Wc, 3), generator=g, dtype=torch.uint8).to(dev)


def host(o):
    return {k: v.cpu().numpy() for k, v in o.items()}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype == np.float32 else a


@pytest.fixture(scope="module")
def outputs(dev):
    """every shape once (origin "region", jitter and shuffle on), copied to the host; the tests share them and leave them unchanged"""
    got = {}
    for n in U.NS:
        for V in U.VS:
            for J in U.JS:
                rec, index = U.case(n, V, J)
                got[n, V, J] = host(run_batch(dev, rec, index))
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("J", U.JS)
@pytest.mark.parametrize("V", U.VS)
@pytest.mark.parametrize("n", U.NS)
def test_against_the_restatement(outputs, n, V, J):
    rec, index = U.case(n, V, J)
    got = outputs[n, V, J]
    ref, r32 = U.ref_batch(rec, index), U.ref_batch(rec, index, dtype=np.float32)
    for k, v in got.items():                                 # every element was overwritten
        assert not (np.isnan(v).any() if v.dtype == np.float32 else (v == -77).any()), k
    for k in U.INT_KEYS:
        assert np.array_equal(got[k], ref[k]), k
    for k in ("intr", "extr"):
        assert np.array_equal(bits(got[k]), bits(ref[k].astype(np.float32))), k
    assert U.differs(got, ref) == []
    # bb
    err, bar = np.abs(got["bb"][..., :2].astype(np.float64) - ref["bb"][..., :2]), RU.bb_bar(ref["bb"][..., :2])
    print("n %d V %d J %d: bb worst err / bar %.3f, bit-equal to the fp32 evaluation: %s" % (
        n, V, J, float((err / bar).max()), np.array_equal(bits(got["bb"]), bits(r32["bb"]))))
    assert (err <= bar).all()
    assert np.array_equal(bits(got["bb"][..., 2]), bits(ref["scale"].astype(np.float32)))
    # the fp32 chains
    floors = {c: U.worst(e, b) for c, e, b in U.chain_checks(rec, r32, ref)}
    for chain, err, bar in U.chain_checks(rec, got, ref):
        same = np.array_equal(bits(got[chain]), bits(r32[chain]))
        print("n %d V %d J %d: %s worst err / bar %.3f (largest bar %.2e), the fp32 evaluation's %.3f, bit-equal to it: %s" % (
            n, V, J, chain, U.worst(err, bar), float(bar.max()), floors[chain], same))
        assert (err <= bar).all(), chain
        assert floors[chain] >= 1 / 16, chain                # (the bar is at most 16 times the host floor)


@pytest.mark.gpu
def test_the_inputs_tell_the_mutants_apart(outputs):
    rec, index = U.case(5, 67, 22)
    got = outputs[5, 67, 22]
    for m in U.MUTATIONS:
        bad = U.differs(got, U.ref_batch(rec, index, mut=m))
        print("%s: %s" % (m, ", ".join(bad)))
        assert bad, m
    for m in U.EQUIVALENT:                                   # (synth_batch_util's docstring: why this one cannot differ)
        assert U.differs(got, U.ref_batch(rec, index, mut=m)) == [], m


@pytest.mark.gpu
@pytest.mark.parametrize("origin,jitter", [("frame", True), ("region", False), ("frame", False)])
def test_the_other_origin_and_no_jitter(dev, origin, jitter):
    rec, index = U.case(5, 67, 22)
    got = host(run_batch(dev, rec, index, origin=origin, jitter=jitter))
    ref = U.ref_batch(rec, index, origin=origin, jitter=jitter)
    for k in U.INT_KEYS:
        assert np.array_equal(got[k], ref[k]), k
    assert U.differs(got, ref) == []
    assert np.array_equal(bits(got["bb"][..., 2]), bits(ref["scale"].astype(np.float32)))


@pytest.mark.gpu
@pytest.mark.parametrize("origin", ["region", "frame"])
@pytest.mark.parametrize("n", U.NS)
def test_images_are_preprocess_crops_and_the_shuffle_is_a_row_choice(dev, n, origin):
    """shuffle off: im, scale and pad of apg_synth_crops against ap_preprocess_crops per camera on the same boxes, bit for bit, and
    bb[..., 2] against that scale; shuffle on: every suffix row of every output is the unshuffled row of camera flip ^ s, bit for bit"""
    from airpose_amd import utils
    rec, index = U.case(n, 67, 22)
    frames = frames_for(dev, n, origin)
    plain = run_batch(dev, rec, index, origin=origin, shuffle=False)
    plain.update(run_crops(dev, frames, plain))
    assert not bool(plain["flip"].any())
    for bgr in (True, False):
        mine = plain if bgr else run_crops(dev, frames, plain, bgr=False)
        for c in (0, 1):
            im, scale, pad = utils.preprocess_crops(frames[c], plain["crops"][c], bgr=bgr)
            assert torch.equal(mine["im"][c].view(torch.int32), im.view(torch.int32)), (bgr, c)
            assert torch.equal(mine["scale"][c].view(torch.int32), scale.view(torch.int32)) and torch.equal(mine["pad"][c], pad)
            assert torch.equal(plain["bb"][c, :, 2].view(torch.int32), scale.view(torch.int32))
    assert not torch.equal(plain["im"][0], plain["im"][1])
    mixed = run_batch(dev, rec, index, origin=origin, shuffle=True)
    mixed.update(run_crops(dev, frames, mixed))
    flip = mixed["flip"].cpu().numpy()
    assert np.array_equal(flip, U.ref_batch(rec, index, origin=origin, boxes_only=True)["flip"]) and (n == 1 or set(flip.tolist()) == {0, 1})
    p, m = host(plain), host(mixed)
    for k in m:
        if k in ("flip", "pose_rotmat"):
            continue
        for s in (0, 1):
            for i in range(n):
                assert np.array_equal(bits(m[k][s, i]), bits(p[k][flip[i] ^ s, i])), (k, s, i)
    assert np.array_equal(bits(m["pose_rotmat"]), bits(p["pose_rotmat"]))


@pytest.mark.gpu
@pytest.mark.parametrize("margin", [20, 0])
@pytest.mark.parametrize("origin", ["region", "frame"])
def test_hostile_boxes_keep_the_box_invariant(dev, origin, margin):
    """boxes outside the frame, inverted, negative, INT_MIN / INT_MAX: the box kernel alone, `crops` on the host, the invariant for
    every row, then the boxes and the status bits against the restatement.  margin = 0 adds the crops that only the widening keeps"""
    rec, index = U.hostile()
    got = host(run_batch(dev, rec, index, origin=origin, margin=margin))
    check_invariant(got["crops"], *canvas_of(origin))
    ref = U.ref_batch(rec, index, origin=origin, margin=margin, boxes_only=True)
    for k in U.INT_KEYS:
        assert np.array_equal(got[k], ref[k]), k
    seen = int(np.bitwise_or.reduce(got["status"].ravel()))
    assert seen & U.CLAMPED and seen & U.WIDENED and (origin == "frame" or seen & U.OUTSIDE)
    assert np.isfinite(got["bb"]).all() and not np.isnan(got["j2d_crop"]).any()


@pytest.mark.gpu
def test_two_calls_give_the_same_bits(dev):
    rec, index = U.case(5, 10475, 127)
    frames = frames_for(dev, 5, "region")
    runs = []
    for _ in range(2):
        o = run_batch(dev, rec, index)
        o.update(run_crops(dev, frames, o))
        runs.append(host(o))
    for k in runs[0]:
        assert np.array_equal(bits(runs[0][k]), bits(runs[1][k])), k


@pytest.mark.gpu
def test_draws_depend_on_seed_epoch_and_index_alone(dev, outputs):
    rec, index = U.case(5, 67, 22)
    base = outputs[5, 67, 22]
    for kw in (dict(epoch=1), dict(seed=U.SEED + 1), dict(seed=U.SEED ^ (1 << 40))):
        other = host(run_batch(dev, rec, index, **kw))
        ref = U.ref_batch(rec, index, **kw)
        assert all(np.array_equal(other[k], ref[k]) for k in U.INT_KEYS), kw
        assert not np.array_equal(other["crops"], base["crops"]), kw
    # the same samples in another batch order, and alone: the same rows
    perm = np.asarray([3, 0, 4, 2, 1])
    shuffled = host(run_batch(dev, {k: v[perm] for k, v in rec.items()}, index[perm]))
    for k, v in shuffled.items():
        if k in ("flip", "pose_rotmat"):
            assert np.array_equal(bits(v), bits(base[k][perm])), k
        else:
            assert np.array_equal(bits(v), bits(base[k][:, perm])), k
    alone = host(run_batch(dev, {k: v[2:3] for k, v in rec.items()}, index[2:3]))
    assert np.array_equal(alone["crops"], base["crops"][:, 2:3]) and np.array_equal(alone["flip"], base["flip"][2:3])
