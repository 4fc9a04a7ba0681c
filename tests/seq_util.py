"""Shared by tests/test_seq_abi.py, test_seq_fp64.py and test_seq_module.py: the fp64 restatement of what apg_seq_init and
apg_seq_export (airpose_amd/csrc/seq_fit.hip) compute, the seeded and conditioned inputs, and the per-element bar.  CPU only.

PARITY UNPINNED, as in oracle/fitting_ref.py: human_body_prior (VPoser V02_05) and pytorch3d 0.3.0 are absent here, so each piece is
restated from its published source --
  * VPoser's encoder (human_body_prior/models/vposer_model.py) from the UNFOLDED state dict: BatchNorm1d(63) - Linear(63, 512) -
    LeakyReLU(0.01) - BatchNorm1d(512) - Dropout - Linear(512, 512) - Linear(512, 512) - NormalDistDecoder (mu, logvar heads), in eval
    mode (running statistics, eps 1e-5, Dropout = identity); encode(x).mean = mu.  The kernel receives loss_real.fold_encoder's two
    affine maps, so the fold is checked as well;
  * pytorch3d.transforms.axis_angle_to_quaternion (sin(t / 2) / t -> 1/2 - t^2 / 48 below 1e-6), quaternion_to_matrix,
    matrix_to_rotation_6d (the first two ROWS);
  * copenet_real.py:105-106 (both detectors' confidences zeroed where they lie more than 100 px apart) and bundle_adj.py:200 (a frame
    is robust iff its AlphaPose confidences sum to more than 14).
The export side uses the oracle's own fitting_ref.vposer_decode and rotation_6d_to_matrix, a general fp64 inverse for cam1_wrt_cam0
(the kernel's rigid shortcut is what gets checked) and smplx_ref's LBS on fit_util.full_model()."""
import functools
import os
import re

import torch
import torch.nn.functional as F

import fit_util as FU
from conftest import REPO
from oracle import fitting_ref as Fr
from oracle import smplx_ref

HEADER = os.path.join(REPO, "include", "airpose_grad.h")
R = int(re.search(r"#define\s+APG_SEQ_ROWS\s+(\d+)", open(HEADER).read()).group(1))       # frames per workgroup
SIZES = tuple(sorted({1, 2, 3, R - 1, R, R + 1, 2 * R + 1, 33} - {0}))
DECODERS = ("body", "all-branch")                            # fit_util._decoder_targets
AGREEMENT_PX, ROBUST_CONF = 100.0, 14.0
INIT_SEED, EXPORT_SEED, VPOSER_SEED = 4100, 80, 4177         # recorded: the seeds of every case (RESEED where one broke a condition)
RESEED = {}                                                  # L -> seed of the init inputs
INIT_KINDS, EXPORT_KINDS = ("z", "phi"), ("thetas", "root_rot", "smpl_wrt_cam", "cam1_wrt_cam0")
INIT_MUTATIONS = ("sixd_from_columns", "logvar_rows", "encoder_on_view1", "bn_eps_dropped", "agreement_ge", "robust_ge",
                  "filter_one_detector", "mask_from_openpose")
EXPORT_MUTATIONS = ("t1_t0inv", "inverse_minus_R_t")
MESH_MUTATIONS = ("hands_at_pca_mean",)
FRAME_EDGE, FRAME_ZERO_ANGLES, FRAME_ZERO_CONF, FRAME_EXACT_14 = 0, 1, 2, 3     # special frames, where L has them


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def encoder_state():
    """a seeded VPoser encoder state dict (fp32 values as fp64): nn.Linear's init, BatchNorm statistics away from (0, 1)"""
    g = torch.Generator().manual_seed(VPOSER_SEED)
    uni = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    sd = {}

    def lin(name, o, i):
        b = 1.0 / i ** 0.5
        sd[name + ".weight"], sd[name + ".bias"] = (uni(o, i) * 2 - 1) * b, (uni(o) * 2 - 1) * b

    def bn(name, n, spread):
        sd[name + ".weight"], sd[name + ".bias"] = 1.0 + 0.2 * rnd(n), 0.1 * rnd(n)
        sd[name + ".running_mean"], sd[name + ".running_var"] = spread * 0.2 * rnd(n), spread * spread * (0.5 + uni(n))
    bn("encoder_net.1", 63, 0.4)
    lin("encoder_net.2", 512, 63)
    bn("encoder_net.4", 512, 0.5)
    lin("encoder_net.6", 512, 512)
    lin("encoder_net.7", 512, 512)
    lin("encoder_net.8.mu", 32, 512)
    lin("encoder_net.8.logvar", 32, 512)
    return {k: v.float().double() for k, v in sd.items()}


def state_dict(vp):
    """ONE VPoser state dict: the seeded encoder and the decoder `vp` (w1 .. b3) under the published names, fp32"""
    sd = {k: v.float() for k, v in encoder_state().items()}
    for i, n in zip((0, 3, 5), (1, 2, 3)):
        sd["decoder_net.%d.weight" % i], sd["decoder_net.%d.bias" % i] = vp["w%d" % n].float(), vp["b%d" % n].float()
    sd["encoder_net.1.num_batches_tracked"] = torch.tensor(7)               # (an entry that is ignored)
    return sd


def init_seed(L):
    return RESEED.get(L, INIT_SEED + L)


@functools.lru_cache(maxsize=None)
def init_case(L):
    """the inputs of apg_seq_init for a sequence of L frames, fp32 values as fp64: angles0/1 (L,22,3), trans0/1 (L,3), det
    (2,L,2,24,3).  Root angles in [0.05, 3.0] rad; detector distances away from 100 px; confidence sums away from 14.  Special
    frames where L has them: 0 carries the representable edge (dx, dy) = (60, 80) at view 1, joint 5; 1 has angles = 0 in both
    views; 2 has all confidences 0; 3 has AlphaPose confidences that are multiples of 0.25 and sum to exactly 14, all kept."""
    g = torch.Generator().manual_seed(init_seed(L))
    uni = lambda *s: torch.rand(*s, generator=g, dtype=torch.float64)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    c = {}
    for v in (0, 1):
        a = 0.4 * rnd(L, 22, 3)
        axis = F.normalize(rnd(L, 3), dim=1)
        a[:, 0] = axis * (0.05 + 2.95 * uni(L, 1))
        if L > FRAME_ZERO_ANGLES:
            a[FRAME_ZERO_ANGLES] = 0.0
        c["angles%d" % v] = a
        c["trans%d" % v] = torch.tensor([0.0, 0.2, 8.0], dtype=torch.float64) + rnd(L, 3)
    det = torch.zeros(2, L, 2, 24, 3, dtype=torch.float64)
    pos = 600.0 + 250.0 * rnd(2, L, 24, 2)
    # the second detector: half the joints within 3 .. 97 px, half 103 .. 300 px away
    far = uni(2, L, 24) < 0.5
    dist = torch.where(far, 103.0 + 197.0 * uni(2, L, 24), 3.0 + 94.0 * uni(2, L, 24))
    ang = 6.283185307179586 * uni(2, L, 24)
    det[:, :, 0, :, :2] = pos
    det[:, :, 1, :, :2] = pos + dist.unsqueeze(-1) * torch.stack([torch.cos(ang), torch.sin(ang)], -1)
    det[..., 2] = uni(2, L, 2, 24)
    det[1, FRAME_EDGE, 0, 5, :2] = torch.tensor([400.0, 300.0], dtype=torch.float64)
    det[1, FRAME_EDGE, 1, 5, :2] = torch.tensor([340.0, 220.0], dtype=torch.float64)
    if L > FRAME_ZERO_CONF:
        det[:, FRAME_ZERO_CONF, :, :, 2] = 0.0
    if L > FRAME_EXACT_14:
        det[:, FRAME_EXACT_14, 1, :, :2] = det[:, FRAME_EXACT_14, 0, :, :2] + 5.0
        q = torch.zeros(2, 24, dtype=torch.float64)
        q[0, :16], q[1, :8], q[1, 8:12] = 0.5, 0.25, 1.0                    # 8 + 2 + 4 = 14
        det[:, FRAME_EXACT_14, 1, :, 2] = q
    c["det"] = det
    return {k: v.float().double() for k, v in c.items()}


@functools.lru_cache(maxsize=None)
def export_case(L, decoder):
    """(vp, prm) of fit_util.make_problem(L, EXPORT_SEED, decoder, ..): a conditioned decoder with its state z, phi0/1, tau0/1"""
    vp, prm, _ = FU.make_problem(L, EXPORT_SEED, decoder, "rot")
    return vp, prm


# ------------------------------------------------------------------------------------------------ the reference
def encode_mean(sd, x, eps=1e-5, head="mu"):
    """VPoser.encode(x).mean from the unfolded state dict, in x's dtype"""
    p = lambda k: sd["encoder_net." + k].to(x.dtype)
    bn = lambda t, k, e: (t - p(k + ".running_mean")) / torch.sqrt(p(k + ".running_var") + e) * p(k + ".weight") + p(k + ".bias")
    h = F.leaky_relu(F.linear(bn(x, "1", eps), p("2.weight"), p("2.bias")), 0.01)
    h = F.linear(F.linear(bn(h, "4", eps), p("6.weight"), p("6.bias")), p("7.weight"), p("7.bias"))
    return F.linear(h, p("8.%s.weight" % head), p("8.%s.bias" % head))


def axis_angle_to_matrix(a):
    """pytorch3d 0.3.0: axis_angle_to_quaternion, then quaternion_to_matrix; (N,3) -> (N,3,3)"""
    t = a.norm(dim=-1, keepdim=True)
    small = t.abs() < 1e-6
    k = torch.where(small, 0.5 - t * t / 48, torch.sin(0.5 * t) / torch.where(small, torch.ones_like(t), t))
    q = torch.cat([torch.cos(0.5 * t), a * k], -1)
    r, i, j, k = q.unbind(-1)
    two_s = 2.0 / (q * q).sum(-1)
    o = torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r),
                     two_s * (i * j + k * r), 1 - two_s * (i * i + k * k), two_s * (j * k - i * r),
                     two_s * (i * k - j * r), two_s * (j * k + i * r), 1 - two_s * (i * i + j * j)), -1)
    return o.reshape(a.shape[:-1] + (3, 3))


def ref_init(case, dtype=torch.float64, mut=None, agreement_px=AGREEMENT_PX, robust_conf=ROBUST_CONF):
    """what apg_seq_init returns, in `dtype`: z (L,32), phi (2,L,6), tau (2,L,3), j2d (2,L,2,24,3), robust (L,) int32"""
    c = {k: v.to(dtype) for k, v in case.items()}
    sd = encoder_state()
    L = c["angles0"].shape[0]
    x = c["angles1" if mut == "encoder_on_view1" else "angles0"][:, 1:22].reshape(L, 63)
    z = encode_mean(sd, x, eps=0.0 if mut == "bn_eps_dropped" else 1e-5, head="logvar" if mut == "logvar_rows" else "mu")
    phi = []
    for v in (0, 1):
        M = axis_angle_to_matrix(c["angles%d" % v][:, 0])
        phi.append((M[:, :, :2].transpose(1, 2) if mut == "sixd_from_columns" else M[:, :2, :]).reshape(L, 6))
    det = c["det"]
    d = det[:, :, 0, :, :2] - det[:, :, 1, :, :2]
    dist = torch.sqrt(d[..., 0] ** 2 + d[..., 1] ** 2)
    apart = dist >= agreement_px if mut == "agreement_ge" else dist > agreement_px
    j2d = det.clone()
    j2d[:, :, 0, :, 2] = torch.where(apart, torch.zeros_like(dist), det[:, :, 0, :, 2])
    if mut != "filter_one_detector":
        j2d[:, :, 1, :, 2] = torch.where(apart, torch.zeros_like(dist), det[:, :, 1, :, 2])
    s = j2d[:, :, 0 if mut == "mask_from_openpose" else 1, :, 2].sum((0, 2))
    robust = (s >= robust_conf if mut == "robust_ge" else s > robust_conf).to(torch.int32)
    return dict(z=z, phi=torch.stack(phi), tau=torch.stack([c["trans0"], c["trans1"]]), j2d=j2d, robust=robust)


def ref_export(vp, prm, dtype=torch.float64, mut=None):
    """what apg_seq_export returns, in `dtype`: thetas (L,63), root_rot (2,L,3,3), smpl_wrt_cam (2,L,4,4), cam1_wrt_cam0 (L,4,4)"""
    vp = {k: v.to(dtype) for k, v in vp.items()}
    p = {k: v.to(dtype) for k, v in prm.items()}
    L = p["z"].shape[0]
    with torch.no_grad():
        thetas = Fr.vposer_decode(vp, p["z"])[0].reshape(L, 63)
        Rv = torch.stack([Fr.rotation_6d_to_matrix(p["phi%d" % v]) for v in (0, 1)])
    tau = torch.stack([p["tau0"], p["tau1"]])
    T = torch.zeros(2, L, 4, 4, dtype=dtype)
    T[:, :, :3, :3], T[:, :, :3, 3], T[:, :, 3, 3] = Rv, tau, 1.0
    if mut == "inverse_minus_R_t":
        inv1 = torch.zeros(L, 4, 4, dtype=dtype)
        inv1[:, :3, :3], inv1[:, 3, 3] = Rv[1].transpose(1, 2), 1.0
        inv1[:, :3, 3] = -torch.einsum("lij,lj->li", Rv[1], tau[1])
        cam = T[0] @ inv1
    elif mut == "t1_t0inv":
        cam = T[1] @ torch.linalg.inv(T[0])
    else:
        cam = T[0] @ torch.linalg.inv(T[1])
    return dict(thetas=thetas, root_rot=Rv, smpl_wrt_cam=T, cam1_wrt_cam0=cam)


def ref_meshes(thetas, betas, T, mut=None):
    """fp64: BodyModel.forward(pose_body = thetas, betas) with root_orient = 0 and zero jaw, eyes and hands, through smplx_ref's LBS on
    fit_util.full_model(), then X' = R X + t per view -> (vertices (2,n,V,3), joints (2,n,127,3))"""
    model = FU.full_model()
    n = thetas.shape[0]
    thetas, betas, T = thetas.double(), betas.double(), T.double()
    if mut == "hands_at_pca_mean":                           # this package's pose2rot=True default: the model file's mean hand pose
        v, j = smplx_ref.smplx_forward_axis_angle(model, betas, thetas, dtype=torch.float64)
    else:
        Rb = smplx_ref.batch_rodrigues(thetas.reshape(-1, 3)).reshape(n, 21, 3, 3)
        v, j = smplx_ref.smplx_forward(model, betas, Rb, dtype=torch.float64)
    move = lambda X, M: torch.einsum("nij,nkj->nki", M[:, :3, :3], X) + M[:, :3, 3].unsqueeze(1)
    return torch.stack([move(v, T[0]), move(v, T[1])]), torch.stack([move(j, T[0]), move(j, T[1])])


# ------------------------------------------------------------------------------------------------ the bar
def scale(ref):
    """|ref| + S per element, S = the largest |ref| of the element's row (the last dimension)"""
    a = ref.abs()
    return a + a.amax(-1, keepdim=True)


def ratio(got, ref):
    """worst |got - ref| / (|ref| + S) (an element whose |ref| + S is 0 counts 0 if it is exactly 0, else inf)"""
    err, sc = (got.double() - ref).abs(), scale(ref)
    q = torch.where(sc > 0, err / torch.where(sc > 0, sc, torch.ones_like(sc)), torch.where(err > 0, float("inf"), 0.0).to(err.dtype))
    return float(q.max())


def exact(got, ref, kinds):
    """the outputs that are copies or discrete: bit-equal as fp32 / equal as integers -> list of the kinds that differ"""
    bad = []
    for k in kinds:
        a, b = got[k], ref[k]
        same = torch.equal(a.to(torch.int32), b.to(torch.int32)) if k == "robust" else \
            torch.equal(a.float().view(torch.int32), b.float().view(torch.int32))
        if not same:
            bad.append(k)
    return bad
