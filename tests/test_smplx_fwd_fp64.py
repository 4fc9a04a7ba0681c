"""Element-wise fp64 ground truth for every kernel of airpose_amd/csrc/smplx.hip: the SMPL-X forward (pose prep and kinematic
chain, skinning, the fused contraction + skinning kernel in its three instantiations, joints / landmarks / projection) and the
stand-alone geometry helpers, through the C ABI of include/airpose_hip.h on the handle of SMPLX._native(dev).  Companion of
test_conv_fwd_fp64.py and test_stem_pool_fp64.py, whose evaluate / check / report / Guarded it reuses.

Kernel -> test
  smplx_prep_kernel                 every LBS test (rotation-matrix inputs: test_lbs_*; 6-D inputs, post transform, in-place
                                    un-scaling, camera centres, input meshes: test_fwd_fused_entry, test_fwd_twoview_entry)
  smplx_skin_kernel<4>              test_lbs_bodies_vertices_modes (mode 0, and every mode under fp32), test_lbs_optional_arguments,
                                    test_lbs_hands_face[4]
  smplx_skin_kernel<8>              test_lbs_hands_face[6]
  smplx_skin_kernel<0>              test_lbs_hands_face[9]
  smplx_lbs_tail_kernel<55, 32>     test_lbs_bodies_vertices_modes (mode 6), test_lbs_default_model
  smplx_lbs_tail_kernel<22, 32>     test_lbs_bodies_vertices_modes (modes 1, 4, 7; mode 8 below 256 bodies), test_lbs_default_model,
                                    test_mode4_leaves_its_counters_at_zero, test_fwd_fused_entry, test_fwd_twoview_entry (A22 form)
  smplx_lbs_tail_kernel<22, 64>     test_lbs_mode8_wide (n >= 256)
  smplx_joints_kernel               every LBS test but mode 4 (packed-record form behind the fused kernel, the generic form else)
  rot6d_kernel                      test_rot6d
  batch_rodrigues_kernel            test_batch_rodrigues[0 | 1]
  rotmat_to_angle_axis_kernel       test_rotmat_to_angle_axis[3 | 4]
  transform_points_kernel           test_transform_points
  projection_kernel                 test_perspective_projection

Reference.  oracle/smplx_ref.smplx_forward(dtype=float64) and oracle/geometry_ref on exactly the fp32 values the kernel receives.
lbs_poly below restates the same polynomial with its intermediates exposed (test_lbs_poly_is_the_oracle holds it to the oracle at
1e-12); it supplies the magnitudes, and its fp32 run is the emulation that the mutations corrupt.

Bars of the LBS path (derived, none measured).  With rotation matrices as inputs every output is a polynomial in the inputs and the
model arrays.  A = the same polynomial on absolute values with every subtraction an addition (blend, rest joints j_template +
j_shapedirs beta, relative joints, chain, A = G [I | -J], weighted bone sum, apply, + transl, post transform, barycentric landmarks);
the one exception is the pose feature R - I, which enters as |R - I|: the inputs are exact, so the subtraction's only error is the
rounding of its result, relative to that result (a one-hot pose feature then has a one-hot magnitude).  A does not change under
re-association or distribution, so one form covers the two-kernel path, the fused kernel, the merged 22-bone table and the bones
with the post transform folded in.  B = the blend's own magnitude sum |coef| |dirs| carried through |sum_k w_k A_k| and |P|.
  |got - ref| <= g(D_rest) A + (g(D_blend) + e_split) (1 + g(D_rest)) B,      g(D) = D u / (1 - D u),  u = 2^-24
(never more than g(D_rest + D_blend) A + e_split B, the form of one gamma for A as a whole: B <= A).  Roundings, from the code:
  D_blend  K + 3 (fp32 MFMA chain over K coefficients, scale / shift epilogue or the template addition), 3 K + 3 in split form (three
           MFMAs per product), + 1 for R - I.  K = 224 (body only, also the fused kernel's 7 steps of 32) or 512 (hands / face).
  D_rest   2 (j_template / j_shapedirs: fp64 sums rounded once, and the fp32 model arrays) + 21 (20 fma and the template addition
           of a rest joint) + 1 (relative joint) + 6 depth (a chain level: three products and three additions; depth = 10)
           + 6 (A's translation) + 6 (post transform composed into a bone, prep kernel) + 2 KB (weighted bone sum: KB = 4, 8 or the
           model's bone count) + 1 (the merged table's re-rounded summed weights) + 6 (apply) + 1 (transl) + 6 (post transform)
           + 3 (barycentric sum) = 113 + 2 KB (121 at four bones).  No form runs all of them; the longest chain bounds every form.
  e_split  3 2^-16 + 2^-32, only in split-bf16 form: hi = rne8(v), lo = rne8(v - hi) leaves |v - (hi + lo)| <= 2^-16 |v| on either
           operand ((1 + 2^-16)^2 - 1 on the product) and the dropped lo lo is at most 2^-8 2^-8 |coef dir|.  With
           ap_smplx_set_blend_precision(fp32) the term is absent and D_blend has K, not 3 K.
  zero     where the bound is 0 the output must be exactly 0 (evaluate()).
Joints 55..75 are vertices: bit-equal to the kernel's own stored vertices on the two-kernel path, the LBS bar on the side-buffer paths.
Tail of the fused / two-view entries: the rotmat output has rot6d's bar; the fp64 LBS reference is evaluated on the kernel's OWN
stored rotmat (and stored translation), so nothing is propagated; with rotmat = NULL the reference takes fp64 rot6d and the bound
grows by A(|R| + dR) - A(|R|), dR = rot6d's bar (a polynomial with non-negative coefficients bounds its own increments).
Projection, d = the LBS bar of the camera-space joint:  |d(x/z)| <= (dx + |x/z| dz) / (|z| - dz), + u |x/z| (division), then
f p + c: two roundings.  |z| >= 1 is asserted on the reference.  pred_pose[:, :3] /= trans_scale is ONE division (prep kernel: t3 /
trans_scale, no reciprocal): one rounding of the fp64 quotient; trans_scale = 0: untouched; every other column never changes.

Bars of the geometry helpers.
  rot6d (derived, Gram-Schmidt)  column b1: 4 u.  b2: (46 / sin + 4) u, sin = the sine of the angle between a1 and a2 (the projection
           a2 - (b1 . a2) b1 carries 13 u |a2| per component, 23 u |a2| in norm, normalising by |a2| sin doubles it at most).  b3 = b1 x
           b2: 11 u + 2 db2.  Independent of |a1|, |a2| (inputs at scales 1e-3 .. 1e3 are included).
  batch_rodrigues (derived, in the angle a; device sinf / cosf taken as 4 ulp)  angle and axis d carry 5 u and 6 u relative (r + 1e-8
           is one rounding of exact inputs); variant 0: u [1 + (5 a + 12 |sin a|) dm + (5 a |sin a| + 4 + 34 (1 - cos a)) dd], dm =
           max |d_i|, dd = max(1, |d|^2); variant 1 (unit quaternion, 8 products of components): u [(20 a + 120) max(1, dm) + 39].
           Both + 2e-8 for the fp64 reference keeping the 1e-8 that fp32 absorbs.
  rotmat_to_angle_axis (derived)  the branch's t = 1 +- t00 +- t11 +- t22 >= 1 in every branch; e = 3 u (1 + |t00| + |t11| + |t22|) / t
           + 4 u per quaternion component beyond the common factor 0.5 / sqrt(t), which cancels in axis x angle; 2 log on the unit
           quaternions is pi-Lipschitz; sqrt, atan2f, division, product: 8 u.  Bar pi (e + 8 u).  The margins (1e-3 from every
           branch condition) are asserted so that fp32 and fp64 take the same branch; the sign of w is that of an exact difference.
  transform_points  g(6) (|M| |v| + |t|).  perspective_projection  d = g(6) (|R| |x| + |t|) (0 without R and t), then the division rule.
No helper needed the 4 x fp32-oracle rule.

Inputs of the LBS path: each body is randn (betas x 2, expression x 1, rotations rot6d_to_rotmat(randn)), one-hot (identity pose,
one coefficient 3.0 at index 0, 9, 10 or 19; or one rotated joint whose feature columns straddle a K step of 32: joints 2, 5, and 23
(224, the body-only K) with hands; or a single matrix entry + 0.5: columns 20, 208 and, with hands, 505 -- each one-hot's column
exceeds 8 x the bar on some vertex, asserted on the CPU), alt (neighbours with translations +4 / -4 and opposite root rotations) or
frame (identity body pose, root rotated by 3.1 rad), mixed within a batch.  Every GPU call runs twice: bit-equal.
Shapes: bodies 1, 31, 32, 33, 64, 65, 77 (7, 8, 9 on the two-kernel path; 255, 256, 257, 300 for mode 8); vertices 24 (the smallest
make_synthetic_model accepts: its joint regressor draws 24 vertices; two vertex groups for sixteen waves), 1024, 1025, 2731 and
the default 10475 once per mode at n = 3; modes 0, 1, 4, 6, 7, 8 x {bf16x2, fp32}.

Finding.  include/airpose_hip.h described the split-bf16 blend as "four-term products"; both the two-kernel GEMM and the fused
kernel run three (hi hi + lo hi + hi lo, the lo lo term dropped: e_split above).  The header now says so.  No kernel bug was found.

CPU self-check (no GPU): smplx_ref.smplx_forward(float32), the fp32 geometry_ref functions and lbs_poly(float32) sit inside every
bar on every family and shape at the small vertex counts; each of MUTATIONS is rejected by the same check.

MEASURED (below) holds the worst err / bound per kernel path on an MI355X; none of it is used as a bar.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_stem_pool_fp64 import Guarded, check, evaluate, report

MEASURED = """
Worst err / bound on an MI355X (256 CUs) per kernel path and blend precision, over every body count, family and vertex count
(python -m pytest tests/test_smplx_fwd_fp64.py -m gpu -s):
  ap_smplx_fwd, body only        V = 24     two-kernel split 0.0241 (joints 0.0241)   fused split 0.0241 (0.0241)   two-kernel fp32 0.0054 (0.0079)
                                 V = 1024   two-kernel split 0.0508 (0.0316)          fused split 0.0508 (0.0316)   two-kernel fp32 0.0078 (0.0078)
                                 V = 1025   two-kernel split 0.0497 (0.0317)          fused split 0.0497 (0.0316)   two-kernel fp32 0.0073 (0.0081)
                                 V = 2731   two-kernel split 0.0577 (0.0483)          fused split 0.0577 (0.0483)   two-kernel fp32 0.0150 (0.0077)
                                 V = 10475  two-kernel split 0.0287 (0.0079)          fused split 0.0287 (0.0079)   two-kernel fp32 0.0070 (0.0053)
  (fused = modes 1, 4, 6, 7, 8: smplx_lbs_tail_kernel<22, 32> and <55, 32>; their maxima agree to the digits shown)
  smplx_lbs_tail_kernel<22, 64>  n = 256, 257, 300: 0.0506 (0.0316); n = 255 (falls back to <22, 32>): 0.0506 (0.0316)
  mode 4, n = 77 then 3, 33, 1   0.0496 (0.0249)
  optional arguments             fused split 0.0476 (0.0316)   two-kernel split 0.0477 (0.0316)
  hands / face, K = 512          smplx_skin_kernel<4> split 0.0327 (0.0159) fp32 0.0061 (0.0063);  <8> split 0.0308 (0.0170) fp32 0.0050
                                 (0.0061);  <0> split 0.0397 (0.0181) fp32 0.0047 (0.0066)
  ap_smplx_fwd_fused             rotmat 0.3921   vertices 0.0262   joints 0.0159   joints2d 0.0131
  ap_smplx_fwd_twoview           rotmat 0.4040   vertices 0.0255   joints 0.0200   joints2d 0.0185   un-scaled translation: exact
  rot6d_kernel 0.5206   batch_rodrigues_kernel variant 0 0.1603, variant 1 0.0240
  rotmat_to_angle_axis_kernel    branch 0 0.1650   1 0.1344   2 0.1763   3 0.0843 (cols = 3 and 4 alike)
  transform_points_kernel 0.2447   projection_kernel  R t 0.2285   t 0.2091   R 0.5688   neither 0.8254 (two roundings of a bar of three)
The split-bf16 blend uses five to six percent of its bar, the fp32 blend one percent; the CPU oracles in fp32 measure the same
(0.006 .. 0.012, rot6d 0.52, projection 0.83).  Vertex joints 55..75 equal the stored vertices bit for bit on the two-kernel path.
The 26 GPU tests take 5.3 s together on the MI355X, none more than 0.6 s; the CPU self-check takes 10 s.
"""

U32 = 2.0 ** -24
E_SPLIT = 3 * 2.0 ** -16 + 2.0 ** -32
MODES = (0, 1, 4, 6, 7, 8)
PRECS = ("bf16x2", "fp32")
N_FUSED = (1, 31, 32, 33, 64, 65, 77)
N_TWO_KERNEL = (7, 8, 9)
N_WIDE = (255, 256, 257, 300)
V_MIN = 24
ANGLES = (0.0, 1e-8, 1e-6, 1e-3, 1.0, 3.1, float(np.float32(math.pi)))
N_GEOM = (1, 255, 256, 257, 55 * 40)
BP_GEOM = ((1, 1), (3, 255), (2, 256), (5, 257), (3, 127))


def g(D):
    return D * U32 / (1.0 - D * U32)


# ------------------------------------------------------------------------------------------------ model and polynomial
_MODELS = {}


def model_of(V=None, max_bones=4):
    """(model dict, fp64 tensors of lbs_poly, their absolute values): built once per (V, max_bones)"""
    key = (V, max_bones)
    if key not in _MODELS:
        from airpose_amd import smplx_model as SM
        md = SM.make_synthetic_model(4321, max_bones=max_bones) if V is None else \
            SM.make_synthetic_model(4321 + V, num_verts=V, num_faces=2 * V, max_bones=max_bones)
        t = lambda a: torch.as_tensor(np.asarray(a, np.float64))
        Vn = md["v_template"].shape[0]
        dirs = torch.cat([t(md["shapedirs"]), t(md["posedirs"]).t().reshape(Vn, 3, -1)], dim=2)       # [V][3][20 + 486]
        parents = [int(p) for p in md["parents"]]
        depth = [0] * len(parents)
        for j in range(1, len(parents)):
            depth[j] = depth[parents[j]] + 1

        def pack(ab):
            f = (lambda x: x.abs()) if ab else (lambda x: x)
            Jreg, vt, sd = f(t(md["J_regressor"])), f(t(md["v_template"])), f(t(md["shapedirs"]))
            return dict(vt=vt, dirs=f(dirs), jt=Jreg @ vt, jsd=torch.einsum("jv,vcl->jcl", Jreg, sd), W=f(t(md["lbs_weights"])),
                        bary=f(t(md["lmk_bary_coords"])), parents=parents,
                        tri=torch.as_tensor(md["faces"][md["lmk_faces_idx"]]).long(), extra=torch.as_tensor(md["extra_joint_verts"]).long())
        _MODELS[key] = dict(md=md, M=pack(False), Mabs=pack(True), depth=max(depth), V=Vn,
                            bones=int((md["lbs_weights"] != 0).sum(1).max()))
    return _MODELS[key]


def lbs_poly(M, c20, pf, R, transl, post, sub=-1.0, mut=None, seed=0):
    """The SMPL-X forward as the polynomial it is.  c20 [n][20], pf [n][54][9] (the pose feature R - I, or its magnitude), R
    [n][55][3][3], transl [n][3] or None, post [n][3][4] or None; sub = -1: the forward, + 1: on magnitudes.  -> dict(verts, joints,
    bverts, bjoints (the blend's own share carried through |T| and |P|), Trot, Prot).  mut: one of MUTATIONS (fp32 emulation)."""
    gen = torch.Generator().manual_seed(9000 + seed)
    n, V = c20.shape[0], M["vt"].shape[0]
    dt = c20.dtype
    Mt = {k: (v.to(dt) if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in M.items()}
    coef = torch.cat([c20, pf.reshape(n, -1)], 1)
    dirs, W, bary = Mt["dirs"], Mt["W"], Mt["bary"]
    if mut == "drop_column":                                 # the heaviest column of one body
        b = int(torch.randint(0, n, (1,), generator=gen))
        coef = coef.clone()
        coef[b, int(coef[b].abs().argmax())] = 0.0
    if mut == "drop_lo":                                     # hi parts only, both operands
        coef, dirs = coef.to(torch.bfloat16).to(dt), dirs.to(torch.bfloat16).to(dt)
    if mut == "neighbour_weights":
        v = int(torch.randint(0, V - 1, (1,), generator=gen))
        W = W.clone()
        W[v] = W[v + 1]
    if mut == "permute_bary":
        l = int(torch.randint(0, bary.shape[0], (1,), generator=gen))
        bary = bary.clone()
        bary[l] = bary[l].roll(1)
    blend = torch.einsum("bk,vck->bvc", coef, dirs)
    vposed = Mt["vt"] + blend
    Jr = Mt["jt"] + torch.einsum("jcl,bl->bjc", Mt["jsd"], c20)
    par = Mt["parents"]
    rel = Jr.clone()
    rel[:, 1:] = Jr[:, 1:] + sub * Jr[:, par[1:]]
    Grot, Gt = [R[:, 0]], [rel[:, 0]]
    for j in range(1, len(par)):
        p = par[j]
        Grot.append(Grot[p] @ R[:, j])
        Gt.append((Grot[p] @ rel[:, j, :, None])[..., 0] + Gt[p])
    Grot, Gt = torch.stack(Grot, 1), torch.stack(Gt, 1)
    At = Gt + sub * (Grot @ Jr[..., None])[..., 0]
    if mut == "neighbour_bones":                             # every body skins with the next body's bone table
        Grot_s, At_s = Grot.roll(-1, 0), At.roll(-1, 0)
    else:
        Grot_s, At_s = Grot, At
    Trot = torch.einsum("vj,bjrc->bvrc", W, Grot_s)
    sk = (Trot @ vposed[..., None])[..., 0] + torch.einsum("vj,bjr->bvr", W, At_s)
    bl = (Trot.abs() @ blend.abs()[..., None])[..., 0]
    lmk = lambda x: torch.einsum("blfi,lf->bli", x[:, Mt["tri"]], bary)
    joints = torch.cat([Gt, sk[:, Mt["extra"]], lmk(sk)], 1)
    bj = torch.cat([torch.zeros_like(Gt), bl[:, Mt["extra"]], lmk(bl)], 1)
    verts = sk
    if transl is not None:
        add = transl.abs() if sub > 0 else transl
        verts, joints = verts + add[:, None], joints + add[:, None]
    Prot = None
    if post is not None:
        Prot, Pt = post[:, :, :3], post[:, :, 3]
        ap = lambda x: (Prot[:, None] @ x[..., None])[..., 0] + Pt[:, None]
        apb = lambda x: (Prot.abs()[:, None] @ x[..., None])[..., 0]
        v2 = ap(verts)
        if mut == "skip_post":                               # the last vertex group of 16 keeps its un-transformed vertices
            v0 = (V - 1) // 16 * 16
            v2[:, v0:] = verts[:, v0:]
        verts, joints, bl, bj = v2, ap(joints), apb(bl), apb(bj)
    return dict(verts=verts, joints=joints, bverts=bl, bjoints=bj, Trot=Trot, Prot=Prot)


def full_rot(inp):
    """[n][55][3][3] fp64: identity where the call passes NULL"""
    n = inp["betas"].shape[0]
    eye = torch.eye(3, dtype=torch.float64).expand(n, 1, 3, 3)
    go = eye if inp.get("go") is None else inp["go"].double().reshape(n, 1, 3, 3)
    ex = eye.expand(n, 33, 3, 3) if inp.get("extra") is None else inp["extra"].double()
    return torch.cat([go, inp["body"].double(), ex], 1)


def c20_of(inp):
    n = inp["betas"].shape[0]
    ex = torch.zeros(n, 10, dtype=torch.float64) if inp.get("expr") is None else inp["expr"].double()
    return torch.cat([inp["betas"].double(), ex], 1)


def d_rest(mo, KB, merged):
    return 2 + 21 + 1 + 6 * mo["depth"] + 6 + 6 + 2 * KB + (1 if merged else 0) + 6 + 1 + 6 + 3


def d_blend(K, split):
    return (3 * K if split else K) + 3 + 1


def lbs_magnitudes(mo, inp, dR=None):
    """fp64 (reference polynomial, magnitude polynomial) of a call; dR [n][55][3][3]: an error bar on the rotations, added to the
    magnitudes of R, of the pose feature and of the post transform's rotation"""
    R = full_rot(inp)
    c20 = c20_of(inp)
    pf = R[:, 1:] - torch.eye(3, dtype=torch.float64)
    post = None if inp.get("post") is None else inp["post"].double()
    tr = None if inp.get("transl") is None else inp["transl"].double()
    ref = lbs_poly(mo["M"], c20, pf.reshape(-1, 54, 9), R, tr, post)
    Ra, pfa, pa = R.abs(), pf.abs(), None if post is None else post.abs()
    if dR is not None:
        Ra, pfa = Ra + dR, pfa + dR[:, 1:]
        if pa is not None:
            pa = pa.clone()
            pa[:, :, :3] += inp["dpost"]
    mag = lbs_poly(mo["Mabs"], c20.abs(), pfa.reshape(-1, 54, 9), Ra, tr, pa, sub=1.0)
    return ref, mag


def lbs_bounds(mo, mag, K, split, KB=4, merged=True):
    """(bound of the vertices, bound of the 127 joints) from the magnitudes"""
    gr, gb = g(d_rest(mo, KB, merged)), g(d_blend(K, split)) + (E_SPLIT if split else 0.0)
    return gr * mag["verts"] + gb * (1 + gr) * mag["bverts"], gr * mag["joints"] + gb * (1 + gr) * mag["bjoints"]


def oracle(mo, inp, dtype):
    """oracle/smplx_ref (+ geometry_ref.transform_smpl for the post transform) on the call's inputs"""
    from oracle import geometry_ref, smplx_ref
    ex = inp.get("extra")
    parts = [None] * 5 if ex is None else [ex[:, 0:1], ex[:, 1:2], ex[:, 2:3], ex[:, 3:18], ex[:, 18:33]]
    cv = lambda x: None if x is None else x.to(dtype)
    v, j = smplx_ref.smplx_forward(mo["md"], cv(inp["betas"]), cv(inp["body"]), cv(inp.get("go")), cv(inp.get("transl")), cv(inp.get("expr")),
                                   cv(parts[0]), cv(parts[1]), cv(parts[2]), cv(parts[3]), cv(parts[4]), dtype=dtype)
    if inp.get("post") is not None:
        P = inp["post"].to(dtype)
        v, j = geometry_ref.transform_smpl(P, v, j)
    return v, j


# ------------------------------------------------------------------------------------------------ inputs
PATTERN = ("randn", "onehot", "alt", "alt", "frame", "onehot")
ONEHOT_BODY = (("c", 0), ("c", 9), ("c", 10), ("c", 19), ("e", 1, 0), ("e", 21, 8), ("r", 2), ("r", 5))
ONEHOT_HANDS = (("e", 54, 8), ("r", 23), ("c", 19), ("e", 1, 0))


def rotmats(x6):
    """fp32 rotation matrices of fp32 6-D vectors [..][6] (fp64 Gram-Schmidt, rounded once)"""
    from oracle import geometry_ref
    return geometry_ref.rot6d_to_rotmat(x6.double().reshape(-1, 6)).float().reshape(*x6.shape[:-1], 3, 3)


def axis_angle_rot(axis, angle):
    from oracle import smplx_ref
    a = torch.as_tensor(axis, dtype=torch.float64)
    return smplx_ref.batch_rodrigues((a / a.norm() * angle).reshape(1, 3), epsilon=0.0)[0].float()


def make_bodies(n, seed, hands=False, expr=True, go=True, transl=True, shift=0):
    """inputs of ap_smplx_fwd for n bodies: body k is PATTERN[(k + shift) % 6]; -> dict of fp32 tensors, "kinds", "onehots" """
    gen = torch.Generator().manual_seed(100 + seed)
    eye = torch.eye(3)
    inp = dict(betas=torch.zeros(n, 10), expr=torch.zeros(n, 10) if expr else None, go=eye.repeat(n, 1, 1, 1) if go else None,
               body=eye.repeat(n, 21, 1, 1), extra=eye.repeat(n, 33, 1, 1) if hands else None,
               transl=torch.zeros(n, 3) if transl else None)
    kinds, onehots, n_one = [], {}, 0
    for k in range(n):
        kind = PATTERN[(k + shift) % len(PATTERN)]
        kinds.append(kind)
        r6 = torch.randn(55, 6, generator=gen)
        b, e, t = torch.randn(10, generator=gen) * 2, torch.randn(10, generator=gen), torch.randn(3, generator=gen)
        if kind == "onehot":
            lst = ONEHOT_HANDS if hands and n_one % 2 == 0 else ONEHOT_BODY
            oh = lst[(n_one // (2 if hands else 1) + seed) % len(lst)]
            n_one += 1
            if oh[0] == "c":
                idx = oh[1] if expr or oh[1] < 10 else oh[1] - 10
                (inp["betas"] if idx < 10 else inp["expr"])[k, idx % 10] = 3.0
            else:
                j = oh[1]
                M3 = eye.clone()
                if oh[0] == "e":
                    M3.view(-1)[oh[2]] += 0.5                # one matrix entry: ONE pose-feature column, 20 + 9 (j - 1) + e
                else:
                    M3 = axis_angle_rot((1.0, 2.0, -1.5), 1.2)
                (inp["body"][k, j - 1:j] if j < 22 else inp["extra"][k, j - 22:j - 21]).copy_(M3[None])
            onehots[k] = oh
            continue
        inp["betas"][k] = b
        if expr:
            inp["expr"][k] = e
        if kind == "frame":
            if go:
                inp["go"][k, 0] = axis_angle_rot((0.3, -1.0, 0.5), 3.1)
        else:
            R = rotmats(r6)
            inp["body"][k] = R[1:22]
            if hands:
                inp["extra"][k] = R[22:]
            if go:
                inp["go"][k, 0] = R[0]
        if transl:
            inp["transl"][k] = t
        if kind == "alt":
            sgn = 1.0 if (k + shift) % len(PATTERN) == 2 else -1.0
            if transl:
                inp["transl"][k] = torch.tensor([4.0, -4.0, 4.0]) * sgn
            if go:
                inp["go"][k, 0] = axis_angle_rot((0.0, 0.0, 1.0), 2.0 * sgn)
    inp["kinds"], inp["onehots"] = kinds, onehots
    return inp


def onehot_margins(mo, inp, ref, bound_v):
    """per one-hot body: the largest (contribution of its heaviest nonzero column) / bar over the vertices; each must exceed 8"""
    out = {}
    R = full_rot(inp)
    pf = (R[:, 1:] - torch.eye(3, dtype=torch.float64)).reshape(len(R), -1)
    coef = torch.cat([c20_of(inp), pf], 1)
    for b in inp["onehots"]:
        col = int(coef[b].abs().argmax())
        assert coef[b, col] != 0
        d = coef[b, col] * mo["M"]["dirs"][:, :, col]
        d = (ref["Trot"][b] @ d[..., None])[..., 0]
        if ref["Prot"] is not None:
            d = (ref["Prot"][b] @ d[..., None])[..., 0]
        out[b] = float((d.abs() / bound_v[b]).max())
    return out


# ------------------------------------------------------------------------------------------------ tail of the fused entries
def proj_bound(j3, dj, fx, fy, c):
    """(reference, bound) of f (x / z) + c for camera-space joints j3 [n][P][3] with bars dj; c [n][2]; asserts |z| >= 1"""
    z, dz = j3[..., 2], dj[..., 2]
    assert float(z.abs().min()) >= 1.0, "a projected point with |z| < 1: %g" % float(z.abs().min())
    out, bnd = [], []
    for i, f in ((0, fx), (1, fy)):
        p = j3[..., i] / z
        dp = (dj[..., i] + p.abs() * dz) / (z.abs() - dz) + U32 * p.abs()
        cc = c[:, None, i].double()
        out.append(f * p + cc)
        bnd.append(abs(f) * dp * (1 + 2 * U32) + U32 * (abs(f) * p.abs()) + U32 * ((abs(f) * p).abs() + cc.abs()))
    return torch.stack(out, -1), torch.stack(bnd, -1)


def rot6d_ref(x6):
    """(fp64 rotation matrices [n][3][3], per-element bar) of fp32 6-D vectors [n][6]"""
    from oracle import geometry_ref
    x = x6.double().reshape(-1, 3, 2)
    a1, a2 = x[:, :, 0], x[:, :, 1]
    cos = (a1 * a2).sum(1) / (a1.norm(dim=1) * a2.norm(dim=1))
    sin = (1 - cos * cos).clamp_min(0).sqrt()
    assert float(sin.min()) > 1e-3, "a1 and a2 nearly parallel: outside the test's domain"
    db2 = (46.0 / sin + 4.0) * U32
    col = torch.stack([torch.full_like(sin, 4 * U32), db2, 11 * U32 + 2 * db2], 1)              # [n][3]: bars of columns b1 b2 b3
    return geometry_ref.rot6d_to_rotmat(x6.double().reshape(-1, 6)), col[:, None, :].expand(-1, 3, -1).contiguous()


def make_pose(n, ld, seed, z0=6.0):
    """pred_pose [n][ld]: translation (z >= z0 - 1.5, alternating x / y signs) | 22 x 6-D | NaN pad;  betas [n][10]"""
    gen = torch.Generator().manual_seed(300 + seed)
    pose = torch.full((n, ld), float("nan"))
    pose[:, 3:135] = torch.randn(n, 132, generator=gen)
    t = torch.rand(n, 3, generator=gen) * 3 - 1.5
    t[:, 2] += z0
    t[1::2, :2] *= -1
    t[::3, 0] += 4.0
    pose[:, :3] = t
    return pose, torch.randn(n, 10, generator=gen) * 2


def tail_case(mo, pose, betas, rot, trans, in_trans=None, dR=None, dpost=None):
    """LBS inputs of a fused-entry call from the rotations `rot` [n][22][3][3] and translations `trans` [n][3] (the kernel's own
    stored values, or a reference's): bodies [n, 2n) are the input meshes (betas 0, the same body rotations, [I | in_trans])"""
    n = rot.shape[0]
    post = torch.cat([rot[:, 0].double(), trans.double()[:, :, None]], 2)
    inp = dict(betas=betas, body=rot[:, 1:], post=post)
    if in_trans is not None:
        pin = torch.cat([torch.eye(3, dtype=torch.float64).expand(n, 3, 3), in_trans.double()[:, :, None]], 2)
        inp = dict(betas=torch.cat([betas, torch.zeros_like(betas)]), body=torch.cat([rot[:, 1:], rot[:, 1:]]), post=torch.cat([post, pin]))
    if dR is not None:
        z33 = torch.zeros(inp["body"].shape[0], 33, 3, 3, dtype=torch.float64)
        rep = 2 if in_trans is not None else 1
        dfull = torch.cat([torch.zeros(n, 1, 3, 3, dtype=torch.float64), dR[:, 1:]], 1).repeat(rep, 1, 1, 1)
        inp["dpost"] = torch.cat([dR[:, 0], torch.zeros_like(dR[:, 0])]) if in_trans is not None else dR[:, 0]
        return inp, torch.cat([dfull, z33], 1)
    return inp, None


def emulate_tail(mo, pose, betas, fx, fy, cc, mut=None):
    """fp32 emulation of ap_smplx_fwd_fused through the fp32 oracles: (rotmat, vertices, joints, joints2d)"""
    from oracle import geometry_ref
    n = pose.shape[0]
    rot = geometry_ref.rot6d_to_rotmat(pose[:, 3:135].reshape(-1, 6)).reshape(n, 22, 3, 3)
    inp = dict(betas=betas, body=rot[:, 1:], post=torch.cat([rot[:, 0], pose[:, :3, None]], 2))
    v, j = oracle(mo, inp, torch.float32)
    if mut == "view0_centre":                                # the second half (view 1) projected with the first half's centres
        cc = torch.cat([cc[:n // 2], cc[:n - n // 2]])
    eye = torch.eye(3).expand(n, 3, 3)
    j2 = geometry_ref.perspective_projection(j, eye, torch.zeros(n, 3), (fx, fy), cc)
    return rot, v, j, j2


# ------------------------------------------------------------------------------------------------ geometry helper references
def geom_axis_angles(n, seed):
    """[n][3] fp32 axis-angle vectors: angles from ANGLES, along +- coordinate axes and along random axes"""
    gen = torch.Generator().manual_seed(500 + seed)
    out = torch.zeros(n, 3)
    ang = torch.zeros(n, dtype=torch.float64)
    for i in range(n):
        a = ANGLES[i % len(ANGLES)]
        k = (i // len(ANGLES)) % 9
        if k < 6:
            ax = torch.zeros(3, dtype=torch.float64)
            ax[k % 3] = 1.0 if k < 3 else -1.0
        else:
            ax = torch.randn(3, generator=gen).double()
            ax /= ax.norm()
        out[i] = (ax * a).float()
        ang[i] = a
    return out, ang


def rodrigues_ref(aa, variant):
    """(fp64 reference, per-element bar [n][3][3]) of batch_rodrigues on fp32 axis-angle vectors"""
    from oracle import geometry_ref, smplx_ref
    r = aa.double()
    ref = smplx_ref.batch_rodrigues(r) if variant == 0 else geometry_ref.batch_rodrigues_quat(r)
    a = (r + 1e-8).norm(dim=1)
    d = r / a[:, None]
    dm, dd = d.abs().max(1)[0], (d * d).sum(1).clamp_min(1.0)
    s, c1 = a.sin().abs(), 1 - a.cos()
    if variant == 0:
        bar = U32 * (1 + (5 * a + 12 * s) * dm + (5 * a * s + 4 + 34 * c1) * dd)
    else:
        bar = U32 * ((20 * a + 120) * dm.clamp_min(1.0) + 39)
    return ref, (bar + 2e-8)[:, None, None].expand(-1, 3, 3).contiguous()


def branch_rotations(n, seed):
    """[n][3][3] fp32 rotations that fall, with a margin of 1e-3, in each of the four trace branches of rotation_matrix_to_quaternion
    (cyclically), plus the identity and angles 1e-4 and 3.1; -> (R, branch [n])"""
    gen = torch.Generator().manual_seed(700 + seed)
    near = {0: (1.0, 0.0, 0.0), 1: (0.0, 1.0, 0.0), 2: (0.0, 0.0, 1.0)}
    Rs, br = [], []
    i = 0
    while len(Rs) < n:
        want = i % 4
        i += 1
        if want < 3:                                         # a turn of 2.2 .. 3.1 rad about an axis near x / y / z
            ax = torch.tensor(near[want], dtype=torch.float64) + 0.25 * torch.randn(3, generator=gen).double()
            ang = (3.1, 2.2 + 0.9 * float(torch.rand(1, generator=gen)))[i % 2]
        else:
            ax = torch.randn(3, generator=gen).double()
            ang = (0.0, 1e-4, 0.3 + 1.2 * float(torch.rand(1, generator=gen)), 1.0)[(i // 4) % 4]
        R = axis_angle_rot(ax, ang) if ang > 0 else torch.eye(3)
        b = angle_axis_branch(R[None])
        if b is None or int(b[0]) != want:
            continue
        Rs.append(R)
        br.append(want)
    return torch.stack(Rs), torch.tensor(br)


def angle_axis_branch(R, margin=1e-3):
    """branch of each fp32 rotation [n][3][3] (0: t22 < eps, t00 > t11; 1: t22 < eps, else; 2: t00 < -t11; 3: else), or None when
    one sits within `margin` of a branch condition"""
    t00, t11, t22 = R[:, 0, 0].double(), R[:, 1, 1].double(), R[:, 2, 2].double()
    low = t22 < 1e-6
    dist = torch.minimum((t22 - 1e-6).abs(), torch.where(low, (t00 - t11).abs(), (t00 + t11).abs()))
    if float(dist.min()) < margin:
        return None
    return torch.where(low, torch.where(t00 > t11, 0, 1), torch.where(t00 < -t11, 2, 3))


def angle_axis_ref(R):
    """(fp64 reference [n][3], per-element bar) of rotation_matrix_to_angle_axis on fp32 rotations; asserts the branch margins"""
    from oracle import geometry_ref
    br = angle_axis_branch(R)
    assert br is not None, "a rotation within 1e-3 of a branch condition"
    t00, t11, t22 = R[:, 0, 0].double(), R[:, 1, 1].double(), R[:, 2, 2].double()
    sg = torch.tensor([[1, -1, -1], [-1, 1, -1], [-1, -1, 1], [1, 1, 1]], dtype=torch.float64)[br]
    t = 1 + sg[:, 0] * t00 + sg[:, 1] * t11 + sg[:, 2] * t22
    assert float(t.min()) >= 1.0 - 1e-5
    e = 3 * U32 * (1 + t00.abs() + t11.abs() + t22.abs()) / t + 4 * U32
    return geometry_ref.rotation_matrix_to_angle_axis(R.double()), (math.pi * (e + 8 * U32))[:, None].expand(-1, 3).contiguous(), br


def make_points(B, P, seed, z0=3.0):
    """points [B][P][3], rt [B][3][4], R [B][3][3], t [B][3], centres [B][2]: signs alternate between neighbouring batches; the
    rotations turn about z (so that z stays >= 1 behind R and t)"""
    gen = torch.Generator().manual_seed(800 + seed)
    pts = torch.randn(B, P, 3, generator=gen)
    pts[..., 2] = pts[..., 2].abs() + z0
    sgn = torch.tensor([1.0 if b % 2 == 0 else -1.0 for b in range(B)])
    R = torch.stack([axis_angle_rot((0.0, 0.0, 1.0), 0.7 * float(s) + 0.1 * b) for b, s in enumerate(sgn)])
    t = torch.stack([torch.tensor([4.0, -4.0, 0.5]) * s for s in sgn]) + torch.tensor([0.0, 0.0, 1.0])
    rt = torch.cat([rotmats(torch.randn(B, 6, generator=gen)), (torch.tensor([4.0, -4.0, 4.0]) * sgn[:, None])[:, :, None]], 2)
    cen = torch.tensor([500.0, -300.0]) * sgn[:, None] + torch.randn(B, 2, generator=gen)
    return pts, rt.contiguous(), R, t, cen


def transform_ref(rt, pts):
    M, v = rt.double(), pts.double()
    ref = (M[:, None, :, :3] @ v[..., None])[..., 0] + M[:, None, :, 3]
    mag = (M[:, None, :, :3].abs() @ v.abs()[..., None])[..., 0] + M[:, None, :, 3].abs()
    return ref, g(6) * mag


def projection_ref(pts, R, t, fx, fy, cen):
    x = pts.double()
    mag = torch.zeros_like(x)
    if R is not None:
        mag = (R.double().abs()[:, None] @ x.abs()[..., None])[..., 0]
        x = (R.double()[:, None] @ x[..., None])[..., 0]
    if t is not None:
        mag = (mag if R is not None else x.abs()) + t.double().abs()[:, None]
        x = x + t.double()[:, None]
    return proj_bound(x, g(6) * mag if (R is not None or t is not None) else mag, fx, fy, cen)


# ------------------------------------------------------------------------------------------------ CPU self-check
MUTATIONS = ("drop_column", "drop_lo", "neighbour_weights", "neighbour_bones", "skip_post", "permute_bary", "view0_centre",
             "negate_branch")
CPU_CASES = [(V_MIN, 9, False), (V_MIN, 33, False), (1025, 7, False), (1025, 9, True)]        # (vertices, bodies, hands / face)


def _emulate_poly(mo, inp, mut=None, seed=0):
    f = lambda x: None if x is None else x.float()
    R = full_rot(inp).float()
    pf = (R[:, 1:] - torch.eye(3)).reshape(-1, 54, 9)
    return lbs_poly(mo["M"], c20_of(inp).float(), pf, R, f(inp.get("transl")), f(inp.get("post")), mut=mut, seed=seed)


def test_lbs_poly_is_the_oracle():
    """lbs_poly (the magnitudes' polynomial, with sub = -1) reproduces oracle/smplx_ref in fp64, hands / face and post transform included"""
    mo = model_of(1025)
    inp = make_bodies(6, 3, hands=True)
    inp["post"] = torch.cat([rotmats(torch.randn(6, 6)), torch.randn(6, 3, 1)], 2)
    ref, mag = lbs_magnitudes(mo, inp)
    v, j = oracle(mo, inp, torch.float64)
    assert float((ref["verts"] - v).abs().max()) < 1e-12 and float((ref["joints"] - j).abs().max()) < 1e-12
    assert bool((mag["verts"] >= ref["verts"].abs()).all()) and bool((mag["bverts"] <= mag["verts"]).all())
    assert d_rest(mo, 4, True) == 121 and d_blend(224, True) == 676 and mo["depth"] == 10


def test_smallest_vertex_count():
    from airpose_amd import smplx_model as SM
    SM.make_synthetic_model(1, num_verts=V_MIN, num_faces=2 * V_MIN)
    with pytest.raises(ValueError):
        SM.make_synthetic_model(1, num_verts=V_MIN - 1, num_faces=2 * V_MIN)


@pytest.mark.parametrize("V,n,hands", CPU_CASES)
def test_cpu_oracles_are_inside_the_bars_and_mutations_are_not(V, n, hands):
    """smplx_ref in fp32 and lbs_poly in fp32 sit inside the bars of both blend precisions (with and without post transform); every
    one-hot column exceeds 8 x the bar; each LBS mutation is rejected under the WIDER of the bars (split, K = 512)."""
    mo = model_of(V)
    ratios = {}
    K = 512 if hands else 224
    for shift in (0, 1, 2):
        inp = make_bodies(n, 10 * V + n + shift, hands=hands, shift=shift)
        if shift == 1:
            inp["post"] = torch.cat([rotmats(torch.randn(n, 6, generator=torch.Generator().manual_seed(shift))),
                                     torch.tensor([4.0, -4.0, 4.0]).repeat(n, 1)[:, :, None] * (1 - 2 * (torch.arange(n) % 2))[:, None, None]], 2)
        ref, mag = lbs_magnitudes(mo, inp)
        v64, j64 = oracle(mo, inp, torch.float64)
        v32, j32 = oracle(mo, inp, torch.float32)
        em = _emulate_poly(mo, inp)
        for split in (False, True):
            bv, bj = lbs_bounds(mo, mag, K, split)
            tag = "split" if split else "fp32"
            check("oracle fp32 V=%d n=%d" % (V, n), "verts/" + tag, v32, v64, bv, ratios)
            check("oracle fp32 V=%d n=%d" % (V, n), "joints/" + tag, j32, j64, bj, ratios)
            check("lbs_poly fp32 V=%d n=%d" % (V, n), "verts/" + tag, em["verts"], v64, bv, ratios)
            check("lbs_poly fp32 V=%d n=%d" % (V, n), "joints/" + tag, em["joints"], j64, bj, ratios)
        marg = onehot_margins(mo, inp, ref, bv)
        assert marg and min(marg.values()) > 8, (V, n, marg)
        if shift != 1:
            continue
        for mut in MUTATIONS[:6]:
            bad = _emulate_poly(mo, inp, mut=mut, seed=7)
            okv, rv, _, _ = evaluate(bad["verts"], v64, bv)
            okj, rj, _, _ = evaluate(bad["joints"], j64, bj)
            assert not (okv and okj), (mut, "the checker accepts this mutation: worst err / bound %.3f / %.3f" % (rv, rj))
            ratios["!" + mut] = max(rv, rj)
    report("emulation V=%d n=%d%s" % (V, n, " hands" if hands else ""), ratios)


def test_cpu_tail_and_geometry_oracles_are_inside_the_bars_and_mutations_are_not():
    """fp32 oracles of the fused entry's tail (rot6d, LBS on the stored rotations, projection) and of every geometry helper against
    their bars; a view projected with the other view's centre and a negated trace branch are rejected."""
    from oracle import geometry_ref, smplx_ref
    ratios = {}
    mo = model_of(V_MIN)
    n, fx, fy = 6, 1475.0, 1400.0
    pose, betas = make_pose(n, 135, 1)
    cc = torch.tensor([500.0, -300.0]) * (1 - 2 * (torch.arange(n) % 2))[:, None] + torch.arange(n)[:, None] * 7.0
    for mut in (None, "view0_centre"):
        rot, v, j, j2 = emulate_tail(mo, pose, betas, fx, fy, cc, mut=mut)
        r64, rbar = rot6d_ref(pose[:, 3:135].reshape(-1, 6))
        inp, _ = tail_case(mo, pose, betas, rot, pose[:, :3])
        ref, mag = lbs_magnitudes(mo, inp)
        bv, bj = lbs_bounds(mo, mag, 224, True)
        p64, pb = proj_bound(ref["joints"], bj, fx, fy, cc)
        if mut is None:
            check("tail", "rotmat", rot.reshape(-1, 3, 3), r64, rbar, ratios)
            check("tail", "verts", v, ref["verts"], bv, ratios)
            check("tail", "joints", j, ref["joints"], bj, ratios)
            check("tail", "joints2d", j2, p64, pb, ratios)
        else:
            ok, r, _, _ = evaluate(j2, p64, pb)
            assert not ok, (mut, r)
            ratios["!" + mut] = r
    for nn in N_GEOM:
        x6 = torch.randn(nn, 6, generator=torch.Generator().manual_seed(nn)) * torch.tensor([1e-3, 1.0, 1e3])[torch.arange(nn) % 3][:, None]
        r64, rbar = rot6d_ref(x6)
        check("rot6d n=%d" % nn, "rot6d", geometry_ref.rot6d_to_rotmat(x6), r64, rbar, ratios)
        aa, _ = geom_axis_angles(nn, nn)
        for variant, fn in ((0, smplx_ref.batch_rodrigues), (1, geometry_ref.batch_rodrigues_quat)):
            ref, bar = rodrigues_ref(aa, variant)
            check("rodrigues n=%d" % nn, "rodrigues%d" % variant, fn(aa), ref, bar, ratios)
        R, br = branch_rotations(nn, nn)
        ref, bar, br2 = angle_axis_ref(R)
        assert torch.equal(br, br2) and (nn < 8 or sorted(set(br.tolist())) == [0, 1, 2, 3])
        got = geometry_ref.rotation_matrix_to_angle_axis(R)
        check("angle_axis n=%d" % nn, "angle_axis", got, ref, bar, ratios)
        if nn >= 8:
            bad = torch.where((br == 1)[:, None], -got, got)
            ok, r, _, _ = evaluate(bad, ref, bar)
            assert not ok, ("negate_branch", r)
            ratios["!negate_branch"] = r
    for B, P in BP_GEOM:
        pts, rt, R, t, cen = make_points(B, P, B * P)
        ref, bar = transform_ref(rt, pts)
        check("transform", "transform", geometry_ref.transform_smpl(rt, pts)[0], ref, bar, ratios)
        for Rr, tt in ((R, t), (None, t), (R, None), (None, None)):
            ref, bar = projection_ref(pts, Rr, tt, 1475.0, 1400.0, cen)
            got = geometry_ref.perspective_projection(pts, torch.eye(3).expand(B, 3, 3) if Rr is None else Rr,
                                                      torch.zeros(B, 3) if tt is None else tt, (1475.0, 1400.0), cen)
            check("projection", "projection", got, ref, bar, ratios)
    report("tail and geometry emulation", ratios)


# ------------------------------------------------------------------------------------------------ GPU side
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


class Body(object):
    """The C ABI on the handle of SMPLX._native(dev); every output in a Guarded buffer; every call twice, bit-equal"""
    _cache = {}

    def __init__(self, dev, mo):
        from airpose_amd import _native as Nn
        from airpose_amd import smplx
        self.Nn, self.L, self.dev, self.mo = Nn, Nn.lib(), dev, mo
        self.S = smplx.SMPLX(model_data=mo["md"])
        self.h = self.S._native(dev)
        self.V, self.mode, self.prec = mo["V"], 1, "bf16x2"

    @classmethod
    def of(cls, dev, V=None, max_bones=4):
        if (V, max_bones) not in cls._cache:
            cls._cache[(V, max_bones)] = cls(dev, model_of(V, max_bones))
        return cls._cache[(V, max_bones)]

    def set(self, mode, prec):
        self.Nn.check(self.L.ap_smplx_set_fused(self.h, mode), "ap_smplx_set_fused")
        self.Nn.check(self.L.ap_smplx_set_blend_precision(self.h, self.Nn.PRECISIONS[prec]), "ap_smplx_set_blend_precision")
        self.mode, self.prec = mode, prec

    def _d(self, t):
        return None if t is None else t.float().contiguous().to(self.dev)

    def _twice(self, what, call, shapes):
        """call(list of Guarded) -> status, twice; -> the fp32 values of the outputs on the CPU (None for a NULL output)"""
        res = []
        for rep in range(2):
            gs = [None if s is None else Guarded(self.dev, "fp32", int(np.prod(s))) for s in shapes]
            self.Nn.check(call(gs), what)
            torch.cuda.synchronize()
            res.append(gs)
        for a, b, s in zip(res[0], res[1], shapes):
            if s is not None:
                a.values(s, what)
                assert torch.equal(a.bits(), b.bits()), (what, "two identical calls differ")
        return [None if s is None else gg.values(s, what).cpu() for gg, s in zip(res[1], shapes)]

    def fwd(self, inp, what):
        n = inp["betas"].shape[0]
        d = {k: self._d(inp.get(k)) for k in ("betas", "expr", "go", "body", "extra", "transl")}
        st = self.Nn.stream_ptr(self.dev)
        call = lambda gs: self.L.ap_smplx_fwd(self.h, n, _p(d["betas"]), _p(d["expr"]), _p(d["go"]), _p(d["body"]), _p(d["extra"]),
                                              _p(d["transl"]), _p(gs[0].out), _p(gs[1].out), st)
        return self._twice(what, call, [(n, self.V, 3), (n, 127, 3)])

    def fused_entry(self, pose, betas, cc, fx, fy, want_rot, what):
        n, ld = pose.shape
        pd, bd, cd = self._d(pose), self._d(betas), self._d(cc)
        st = self.Nn.stream_ptr(self.dev)
        call = lambda gs: self.L.ap_smplx_fwd_fused(self.h, n, _p(pd), ld, _p(bd), _p(cd), fx, fy, _p(gs[0].out), _p(gs[1].out),
                                                    _p(gs[2].out) if gs[2] else None, _p(gs[3].out) if gs[3] else None, st)
        out = self._twice(what, call, [(n, self.V, 3), (n, 127, 3), (n, 127, 2) if cc is not None else None,
                                       (n, 22, 3, 3) if want_rot else None])
        assert torch.equal(pd.view(torch.int32).cpu(), pose.view(torch.int32)), (what, "pred_pose was written")
        return out

    def twoview_entry(self, pose, scale, betas, i0, i1, fx, fy, in_trans, what):
        """-> (outputs, pred_pose after the call)"""
        n2, ld = pose.shape
        B = n2 // 2
        bd, d0, d1, dt = self._d(betas), self._d(i0), self._d(i1), self._d(in_trans)
        st = self.Nn.stream_ptr(self.dev)
        poses = []

        def call(gs):
            poses.append(self._d(pose))                      # a fresh copy per call: the entry divides in place
            return self.L.ap_smplx_fwd_twoview(self.h, B, _p(poses[-1]), ld, scale, _p(bd), _p(d0), _p(d1), fx, fy, _p(dt), _p(gs[0].out),
                                               _p(gs[1].out), _p(gs[2].out) if gs[2] else None, _p(gs[3].out), st)
        out = self._twice(what, call, [((4 if in_trans is not None else 2) * B, self.V, 3), (n2, 127, 3),
                                       (n2, 127, 2) if i0 is not None else None, (n2, 22, 3, 3)])
        assert torch.equal(poses[0].view(torch.int32), poses[1].view(torch.int32)), (what, "two identical calls differ in pred_pose")
        return out, poses[1].cpu()


def plan_of(mo, mode, prec, n, body_only=True, has_transl=True):
    """What api_smplx.hip's smplx_run launches: (fused kernel?, K, split, KB, merged table?)"""
    fused = mode != 0 and prec == "bf16x2" and body_only and mo["bones"] <= 4
    K = 224 if body_only else 512
    return fused, K, prec == "bf16x2", (4 if mo["bones"] <= 4 else 8 if mo["bones"] <= 8 else mo["bones"]), fused and mode != 6


def run_lbs_case(body, inp, modes, precs, ratios, what, body_only=True):
    mo = body.mo
    ref, mag = lbs_magnitudes(mo, inp)
    for prec in precs:
        for mode in modes:
            body.set(mode, prec)
            n = inp["betas"].shape[0]
            fused, K, split, KB, merged = plan_of(mo, mode, prec, n, body_only)
            bv, bj = lbs_bounds(mo, mag, K, split, KB, merged)
            tag = "%s mode %d %s" % (what, mode, prec)
            v, j = body.fwd(inp, tag)
            name = ("fused" if fused else "two-kernel") + ("/split" if split else "/fp32")
            check(tag, "verts " + name, v, ref["verts"], bv, ratios)
            check(tag, "joints " + name, j, ref["joints"], bj, ratios)
            if not fused:                                    # joints 55..75 are vertices: the joints kernel redoes skin_point's arithmetic
                assert torch.equal(j[:, 55:76], v[:, mo["M"]["extra"]]), (tag, "vertex joints differ from the stored vertices")
    body.set(1, "bf16x2")


@gpu
@pytest.mark.parametrize("V", [V_MIN, 1024, 1025, 2731])
def test_lbs_bodies_vertices_modes(dev, V):
    """ap_smplx_fwd body-only at every body count x fused mode x blend precision on a model of V vertices (fp32 forces the two kernels)"""
    body = Body.of(dev, V)
    ratios = {}
    for n in N_FUSED + N_TWO_KERNEL:
        inp = make_bodies(n, 31 * V + n, shift=n % 6)
        modes = MODES if n in N_FUSED else (0, 1)
        run_lbs_case(body, inp, modes, PRECS, ratios, "V=%d n=%d" % (V, n))
    report("ap_smplx_fwd V=%d" % V, ratios)


@gpu
@pytest.mark.parametrize("n", N_WIDE)
def test_lbs_mode8_wide(dev, n):
    """mode 8: 64 bodies per workgroup from 256 bodies on; at 255 the 32-body kernel, still right; modes 1 and 0 beside it"""
    body = Body.of(dev, 1024)
    ratios = {}
    run_lbs_case(body, make_bodies(n, 77 + n, shift=n % 6), (8, 1, 0), PRECS, ratios, "V=1024 n=%d" % n)
    report("ap_smplx_fwd mode 8 n=%d" % n, ratios)


@gpu
def test_lbs_default_model(dev):
    """the 10475-vertex model once per mode and precision at n = 3"""
    body = Body.of(dev, None)
    ratios = {}
    run_lbs_case(body, make_bodies(3, 5, shift=1), MODES, PRECS, ratios, "V=10475 n=3")
    report("ap_smplx_fwd V=10475", ratios)


@gpu
def test_mode4_leaves_its_counters_at_zero(dev):
    """mode 4 at n = 77 and at once n = 3 on the same handle: the second call's joints need every arrival counter back at zero"""
    body = Body.of(dev, 1025)
    ratios = {}
    for n in (77, 3, 33, 1):
        run_lbs_case(body, make_bodies(n, 900 + n, shift=n % 6), (4,), ("bf16x2",), ratios, "counters n=%d" % n)
    report("mode 4 counters", ratios)


@gpu
def test_lbs_optional_arguments(dev):
    """every optional pointer of ap_smplx_fwd given and NULL (extra_pose given: K = 512 and the two-kernel path)"""
    body = Body.of(dev, 1024)
    ratios = {}
    for bits in range(16):
        ex, go, hands, tr = bool(bits & 1), bool(bits & 2), bool(bits & 4), bool(bits & 8)
        inp = make_bodies(3, 40 + bits, hands=hands, expr=ex, go=go, transl=tr, shift=bits % 6)
        run_lbs_case(body, inp, (1, 0), ("bf16x2",), ratios, "expr=%d go=%d extra=%d transl=%d" % (ex, go, hands, tr), body_only=not hands)
    report("ap_smplx_fwd optional arguments", ratios)


@gpu
@pytest.mark.parametrize("max_bones", [4, 6, 9])
def test_lbs_hands_face(dev, max_bones):
    """hands / face / expression (K = 512) on models with up to 4, 6 and 9 bones per vertex: smplx_skin_kernel<4>, <8>, <0>"""
    body = Body.of(dev, 1025, max_bones)
    assert (body.mo["bones"] <= 4, 4 < body.mo["bones"] <= 8, body.mo["bones"] > 8)[(4, 6, 9).index(max_bones)]
    ratios = {}
    for n in (3, 9):
        run_lbs_case(body, make_bodies(n, 60 + n + max_bones, hands=True, shift=n % 6), (1,), PRECS, ratios, "hands n=%d" % n, body_only=False)
        run_lbs_case(body, make_bodies(n, 70 + n + max_bones, shift=1), (1,), PRECS, ratios, "body n=%d" % n)
    report("ap_smplx_fwd hands / face, %d bones" % max_bones, ratios)


def _check_tail(body, what, out, pose_after, betas, cc, fx, fy, in_trans, ratios, pose_in=None):
    """vertices, joints and projection of a fused-entry call against the fp64 LBS on the kernel's own stored rotations and translations"""
    mo = body.mo
    v, j, j2, rot = out
    n = j.shape[0]
    x6 = pose_after[:, 3:135].reshape(-1, 6)
    if rot is not None:
        r64, rbar = rot6d_ref(x6)
        check(what, "rotmat", rot.reshape(-1, 3, 3), r64, rbar, ratios)
        inp, dR = tail_case(mo, None, betas, rot, pose_after[:, :3], in_trans)
    else:                                                    # rotmat = NULL: fp64 rot6d, its bar propagated through the magnitudes
        r64, rbar = rot6d_ref(x6)
        inp, dR = tail_case(mo, None, betas, r64.reshape(n, 22, 3, 3), pose_after[:, :3], in_trans, dR=rbar.reshape(n, 22, 3, 3))
    ref, mag = lbs_magnitudes(mo, inp, dR)
    _, K, split, KB, merged = plan_of(mo, body.mode, body.prec, v.shape[0])
    bv, bj = lbs_bounds(mo, mag, K, split, KB, merged)
    if dR is not None:
        _, mag0 = lbs_magnitudes(mo, {k: x for k, x in inp.items() if k != "dpost"})
        bv, bj = bv + (mag["verts"] - mag0["verts"]), bj + (mag["joints"] - mag0["joints"])
    check(what, "verts", v, ref["verts"], bv, ratios)
    check(what, "joints", j, ref["joints"][:n], bj[:n], ratios)
    if j2 is not None:
        p64, pb = proj_bound(ref["joints"][:n], bj[:n], fx, fy, cc)
        check(what, "joints2d", j2, p64, pb, ratios)


@gpu
@pytest.mark.parametrize("n", [1, 33])
def test_fwd_fused_entry(dev, n):
    """ap_smplx_fwd_fused: pose_ld 135 and 144 (NaN pad), cam_center and rotmat given and NULL, fused modes and the two kernels"""
    body = Body.of(dev, 1025)
    ratios = {}
    fx, fy = 1475.0, 1400.0
    cc = torch.tensor([500.0, -300.0]) * (1 - 2 * (torch.arange(n) % 2))[:, None] + torch.arange(n)[:, None] * 3.0
    for ld in (135, 144):
        pose, betas = make_pose(n, ld, n + ld)
        for mode, prec, use_cc, want_rot in ((1, "bf16x2", True, True), (1, "bf16x2", False, True), (1, "bf16x2", True, False),
                                             (4, "bf16x2", True, True), (7, "bf16x2", True, True), (0, "bf16x2", True, True),
                                             (1, "fp32", True, True)):
            body.set(mode, prec)
            what = "fused entry n=%d ld=%d mode %d %s cc=%d rot=%d" % (n, ld, mode, prec, use_cc, want_rot)
            out = body.fused_entry(pose, betas, cc if use_cc else None, fx, fy, want_rot, what)
            _check_tail(body, what, out, pose, betas, cc, fx, fy, None, ratios)
    body.set(1, "bf16x2")
    report("ap_smplx_fwd_fused n=%d" % n, ratios)


@gpu
@pytest.mark.parametrize("B", [1, 3, 17])
def test_fwd_twoview_entry(dev, B):
    """ap_smplx_fwd_twoview: trans_scale 0 and 0.5 (in place, one division), intrinsics given (centres differ per view and body)
    and NULL, the input meshes given and NULL; nothing but pred_pose[:, :3] ever changes"""
    body = Body.of(dev, 1025)
    ratios = {}
    fx, fy, n2 = 1475.0, 1400.0, 2 * B
    gen = torch.Generator().manual_seed(B)
    intr = torch.eye(3).repeat(2, B, 1, 1)
    intr[..., 0, 0], intr[..., 1, 1] = fx, fy
    intr[0, :, :2, 2] = torch.tensor([500.0, 300.0]) + torch.randn(B, 2, generator=gen) * 20
    intr[1, :, :2, 2] = torch.tensor([-450.0, 350.0]) + torch.randn(B, 2, generator=gen) * 20
    cc = torch.cat([intr[0, :, :2, 2], intr[1, :, :2, 2]])
    in_trans = torch.randn(n2, 3, generator=gen) + torch.tensor([0.0, 0.0, 6.0])
    for ld, scale, use_intr, use_in, mode in ((135, 0.0, True, True, 1), (144, 0.5, True, True, 1), (144, 0.5, False, False, 1),
                                              (135, 0.5, True, False, 4), (144, 0.0, True, True, 0)):
        pose, betas = make_pose(n2, ld, 7 * B + ld, z0=6.0 if scale == 0 else 3.0)          # (z / 0.5 >= 3 behind the un-scaling)
        body.set(mode, "bf16x2")
        what = "twoview B=%d ld=%d scale=%g intr=%d in=%d mode %d" % (B, ld, scale, use_intr, use_in, mode)
        out, after = body.twoview_entry(pose, scale, betas, intr[0] if use_intr else None, intr[1] if use_intr else None, fx, fy,
                                        in_trans if use_in else None, what)
        keep = torch.ones(ld, dtype=torch.bool)
        keep[:3] = scale == 0
        assert torch.equal(after.view(torch.int32)[:, keep], pose.view(torch.int32)[:, keep]), (what, "pred_pose changed outside [:, :3]")
        if scale != 0:
            q = pose[:, :3].double() / scale
            check(what, "un-scaled translation", after[:, :3], q, U32 * q.abs(), ratios)
        _check_tail(body, what, out, after, betas, cc, fx, fy, in_trans if use_in else None, ratios)
    body.set(1, "bf16x2")
    report("ap_smplx_fwd_twoview B=%d" % B, ratios)


def _geom(dev, what, fn, shape):
    """fn(Guarded) -> status, twice; the fp32 values on the CPU"""
    from airpose_amd import _native as Nn
    res = []
    for rep in range(2):
        gg = Guarded(dev, "fp32", int(np.prod(shape)))
        Nn.check(fn(gg), what)
        torch.cuda.synchronize()
        res.append(gg)
    res[0].values(shape, what)
    assert torch.equal(res[0].bits(), res[1].bits()), (what, "two identical calls differ")
    return res[1].values(shape, what).cpu()


@gpu
def test_rot6d(dev):
    from airpose_amd import _native as Nn
    L, st, ratios = Nn.lib(), Nn.stream_ptr(dev), {}
    for n in N_GEOM:
        x6 = torch.randn(n, 6, generator=torch.Generator().manual_seed(n)) * torch.tensor([1e-3, 1.0, 1e3])[torch.arange(n) % 3][:, None]
        xd = x6.to(dev)
        ref, bar = rot6d_ref(x6)
        check("rot6d n=%d" % n, "rot6d", _geom(dev, "ap_rot6d_to_rotmat", lambda gg: L.ap_rot6d_to_rotmat(_p(xd), n, _p(gg.out), st), (n, 3, 3)),
              ref, bar, ratios)
    report("rot6d_kernel", ratios)


@gpu
@pytest.mark.parametrize("variant", [0, 1])
def test_batch_rodrigues(dev, variant):
    from airpose_amd import _native as Nn
    L, st, ratios = Nn.lib(), Nn.stream_ptr(dev), {}
    for n in N_GEOM:
        aa, _ = geom_axis_angles(n, n)
        ad = aa.to(dev)
        ref, bar = rodrigues_ref(aa, variant)
        got = _geom(dev, "ap_batch_rodrigues", lambda gg: L.ap_batch_rodrigues(_p(ad), n, variant, _p(gg.out), st), (n, 3, 3))
        check("rodrigues %d n=%d" % (variant, n), "n=%d" % n, got, ref, bar, ratios)
    report("batch_rodrigues_kernel variant %d" % variant, ratios)


@gpu
@pytest.mark.parametrize("cols", [3, 4])
def test_rotmat_to_angle_axis(dev, cols):
    """every trace branch, the identity, angles 1e-4 and 3.1; cols = 4: the fourth column holds NaN and must not be read"""
    from airpose_amd import _native as Nn
    L, st, ratios = Nn.lib(), Nn.stream_ptr(dev), {}
    for n in N_GEOM:
        R, br = branch_rotations(n, n)
        ref, bar, _ = angle_axis_ref(R)
        Rin = R if cols == 3 else torch.cat([R, torch.full((n, 3, 1), float("nan"))], 2)
        rd = Rin.contiguous().to(dev)
        got = _geom(dev, "ap_rotmat_to_angle_axis", lambda gg: L.ap_rotmat_to_angle_axis(_p(rd), n, cols, _p(gg.out), st), (n, 3))
        for b in sorted(set(br.tolist())):
            check("angle_axis cols=%d n=%d" % (cols, n), "branch %d" % b, got[br == b], ref[br == b], bar[br == b], ratios)
    report("rotmat_to_angle_axis_kernel cols=%d" % cols, ratios)


@gpu
def test_transform_points(dev):
    from airpose_amd import _native as Nn
    L, st, ratios = Nn.lib(), Nn.stream_ptr(dev), {}
    for B, P in BP_GEOM:
        pts, rt, _, _, _ = make_points(B, P, B * P)
        pd, rd = pts.to(dev), rt.to(dev)
        ref, bar = transform_ref(rt, pts)
        got = _geom(dev, "ap_transform_points", lambda gg: L.ap_transform_points(_p(rd), _p(pd), B, P, _p(gg.out), st), (B, P, 3))
        check("transform_points B=%d P=%d" % (B, P), "B=%d P=%d" % (B, P), got, ref, bar, ratios)
    report("transform_points_kernel", ratios)


@gpu
def test_perspective_projection(dev):
    from airpose_amd import _native as Nn
    L, st, ratios = Nn.lib(), Nn.stream_ptr(dev), {}
    fx, fy = 1475.0, 1400.0
    for B, P in BP_GEOM:
        pts, _, R, t, cen = make_points(B, P, B * P)
        pd, cd = pts.to(dev), cen.to(dev)
        for Rr, tt, tag in ((R, t, "R t"), (None, t, "t"), (R, None, "R"), (None, None, "none")):
            Rd, td = (None if Rr is None else Rr.contiguous().to(dev)), (None if tt is None else tt.contiguous().to(dev))
            ref, bar = projection_ref(pts, Rr, tt, fx, fy, cen)
            got = _geom(dev, "ap_perspective_projection",
                        lambda gg: L.ap_perspective_projection(_p(pd), B, P, _p(Rd), _p(td), fx, fy, _p(cd), _p(gg.out), st), (B, P, 2))
            check("projection B=%d P=%d %s" % (B, P, tag), tag, got, ref, bar, ratios)
    report("projection_kernel", ratios)
