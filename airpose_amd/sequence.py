"""AirPose+ on a whole sequence: the network's per-frame outputs and the raw detections in, fitted bodies out -- AirPosePlusSequence.

copenet_real_data/scripts/bundle_adj.py around its optimisation loop (which is AirPosePlusFitter.run, fitting.py):
  prepare   :176-200 and copenet_real/dsets/copenet_real.py:105-106: z = vp_model.encode(pose_body of view 0).mean, the per-view root
            rotation as pytorch3d's 6-D (the first two ROWS of axis_angle_to_matrix), the translations, the detector-agreement filter
            and the robust-frame mask.  One apg_seq_init launch (csrc/seq_fit.hip, include/airpose_grad.h).
  fit       :216-222: windows of `chunk` frames, each an independent AirPosePlusFitter.run with beta = 0 and a fresh Adam.
  export    :404-412, 510-516: vp_model.decode(z)["pose_body"], rotation_6d_to_matrix, the bodies' poses in both cameras and
            cam1_wrt_cam0 (one apg_seq_export launch), then the meshes: SMPLX.forward and utils.transform_smpl.
human_body_prior and pytorch3d are not dependencies: VPoser V02_05's encoder and decoder and pytorch3d 0.3.0's conversions are
restated from their published sources, so parity with them is UNPINNED (as for the fitter's decoder and RealDataLoss's encoder).
There is no CPU path and no fallback: a missing library is an error.

Script quirks reproduced, beside the fitter's own (sigma = 30, loss_beta without gradient, two optimisers switching at iteration
100): the script halves the hip confidences IN PLACE in the array of the whole sequence on every iteration of every window
(:344-345), so window k starts with the hips weighing 2^-(k n_iters) and from the second window on they weigh nothing.
carry_hip_decay=True (the default) reproduces that: window k runs with first_iter = k n_iters and switch_iter = k n_iters +
switch_iter (the hip weight is the only thing that reads the absolute iteration).  carry_hip_decay=False starts every window at
iteration 0.  Each window has a shape vector of its own: `beta` is (n_chunks, 10), as the script writes one result file per window.
"""
import torch

from . import _args as A
from . import _native as N
from . import _native_grad as G
from .fitting import SWITCH_ITER, AirPosePlusFitter
from .loss_real import ENCODER_KEYS, NZ, fold_encoder

NAME = "AirPosePlusSequence"
DECODER_KEYS = {"decoder_net.0.weight": (512, 32), "decoder_net.0.bias": (512,), "decoder_net.3.weight": (512, 512),
                "decoder_net.3.bias": (512,), "decoder_net.5.weight": (126, 512), "decoder_net.5.bias": (126,)}
_DECODER_SHORT = ("w1", "b1", "w2", "b2", "w3", "b3")        # AirPosePlusFitter's names, in DECODER_KEYS' order
PRED_KEYS = {"pred_angles0": (22, 3), "pred_angles1": (22, 3), "pred_smpltrans0": (3,), "pred_smpltrans1": (3,)}
STATE_KEYS = {"z": (NZ,), "phi0": (6,), "phi1": (6,), "tau0": (3,), "tau1": (3,)}
HYPER = ("lr", "sigma", "w_vposer", "w_temporal")
AGREEMENT_PX, ROBUST_CONF = 100.0, 14.0                      # copenet_real.py:105-106, bundle_adj.py:200
MESH_BATCH = 512                                             # bodies per SMPLX.forward call of export


def windows(L, chunk):
    """[k chunk, min((k + 1) chunk, L)) for k = 0 .. ceil(L / chunk) - 1 (bundle_adj.py:216-222)"""
    if int(L) != L or L < 1:
        raise ValueError("%s: a sequence needs at least one frame, got %r" % (NAME, L))
    if int(chunk) != chunk or chunk < 1:
        raise ValueError("%s: chunk must be a positive integer, got %r" % (NAME, chunk))
    return [(a, min(a + int(chunk), int(L))) for a in range(0, int(L), int(chunk))]


def _strip(state_dict):
    return {(k[len("vp_model."):] if k.startswith("vp_model.") else k): v for k, v in state_dict.items()}


class AirPosePlusSequence:
    """AirPosePlusSequence(vposer, body, device=None, chunk=2000)

    vposer: ONE VPoser V02_05 state dict -- the encoder's published keys (loss_real.ENCODER_KEYS) and the decoder's Linear layers
    decoder_net.{0,3,5}.{weight,bias}; an optional `vp_model.` prefix is stripped, other entries are ignored, a missing key or a
    wrong shape is refused by name.  body: an airpose_amd.smplx.SMPLX.  Owns one AirPosePlusFitter (made on first use).

    prepare(pred, detections, agreement_px=100, robust_conf=14) -> (state, data)
      pred: pred_angles0/1 (L, 22, 3) axis-angle and pred_smpltrans0/1 (L, 3), what TwoViewInference(..., want_angles=True)
      returns (further keys are ignored); detections (2 views, L, 2 detectors, 24, 3) = x, y, confidence, detector 0 OpenPose,
      detector 1 AlphaPose.  fp32 CUDA tensors on the object's device; shapes and devices are refused by name.
      state: z (L, 32), phi0/phi1 (L, 6), tau0/tau1 (L, 3); data: j2d (2, L, 2, 24, 3), robust (L,) int32 on the host (the one
      host copy of prepare).
    fit(state, data, intr, extr=None, n_iters=300, switch_iter=100, carry_hip_decay=True, want_loss=False, **hyper) -> result
      intr (2, 4) = fx, fy, cx, cy; extr (2, 3, 4), None = identity (bundle_adj.py:231-235); hyper: lr, sigma, w_vposer, w_temporal
      of AirPosePlusFitter.run.  result: z, phi0, phi1, tau0, tau1 for all L frames, beta (n_chunks, 10), chunks (the windows),
      robust, and with want_loss loss: per window the (n_iters, 4) history.
    export(result, frames=None, want_vertices=True) -> dict
      thetas (L, 63), betas (L, 10) (each frame its window's), root_rot0/1 (L, 3, 3), trans0/1 (L, 3) -- the names of the script's
      .npz -- smpl_wrt_cam0/1 (L, 4, 4), cam1_wrt_cam0 (L, 4, 4): for ALL frames.  With want_vertices also pred_vertices_cam0/1
      (n, V, 3) and pred_j3d_cam0/1 (n, 127, 3), the pipeline's names (MeshMetrics.update and Renderer.visualize_tb take them as
      they are), for the frames of the slice `frames` only, with frames itself under "frames".  frames=None means every frame: a
      7000-frame mesh is 0.9 GB per view, so pass a slice for a long sequence.
    __call__(pred, detections, intr, extr=None, frames=None, want_vertices=True, **fit_args) chains the three.
    """

    def __init__(self, vposer, body, device=None, chunk=2000):
        self.device = A.cuda_device(NAME, device)
        windows(1, chunk)
        self.chunk, self.body = int(chunk), body
        sd = _strip(vposer)
        dec = []
        for k, shape in DECODER_KEYS.items():
            if k not in sd:
                raise KeyError("%s: the vposer state dict has no %r" % (NAME, k))
            t = torch.as_tensor(sd[k]).detach().to(device="cpu", dtype=torch.float32)
            if tuple(t.shape) != shape:
                raise ValueError("%s: vposer[%r] must be %s, got %s" % (NAME, k, shape, tuple(t.shape)))
            dec.append(t.contiguous())
        for k, shape in ENCODER_KEYS.items():
            if k not in sd:
                raise KeyError("%s: the vposer state dict has no %r" % (NAME, k))
            if tuple(torch.as_tensor(sd[k]).shape) != shape:
                raise ValueError("%s: vposer[%r] must be %s, got %s" % (NAME, k, shape, tuple(torch.as_tensor(sd[k]).shape)))
        W1, b1, W2, b2 = fold_encoder(sd)                    # fp64; rounded to fp32 once
        self._enc_host = [t.float().contiguous() for t in (W1, b1, W2[:NZ], b2[:NZ])]
        self._dec_host = dec
        self._enc = self._dec = self._fitter = None

    # ---------------------------------------------------------------------------------------- device state
    def _weights(self):
        if self._enc is None:
            N.require_gpu()
            self._enc = [t.to(self.device) for t in self._enc_host]
            self._dec = [t.to(self.device) for t in self._dec_host]
        return self._enc, self._dec

    @property
    def fitter(self):
        if self._fitter is None:
            self._fitter = AirPosePlusFitter(dict(zip(_DECODER_SHORT, self._dec_host)), self.body, self.device)
        return self._fitter

    def _tensors(self, items):
        """items: (tensor, shape with None = any extent, name) -> fp32 contiguous tensors.  Every item's type and shape are looked at
        first, then every item's device; anything else is refused by name"""
        for t, shape, name in items:
            A.is_tensor(NAME, t, name)
            if not t.is_floating_point():
                raise RuntimeError("%s: %s must be a floating-point tensor, got %s" % (NAME, name, t.dtype))
            if t.dim() != len(shape) or any(s is not None and s != d for s, d in zip(shape, t.shape)):
                raise RuntimeError("%s: %s must be (%s), got %s" % (NAME, name, ", ".join("L" if s is None else str(s) for s in shape),
                                                                    tuple(t.shape)))
        for t, _, name in items:
            A.lives_on(NAME, t, self.device, name, "the fitter")
        return [N.f32c(t.detach()) for t, _, _ in items]

    # ---------------------------------------------------------------------------------------- the three steps
    def prepare(self, pred, detections, agreement_px=AGREEMENT_PX, robust_conf=ROBUST_CONF):
        for k in PRED_KEYS:
            if k not in pred:
                raise RuntimeError("%s: pred has no %r (TwoViewInference(..., want_angles=True) returns it)" % (NAME, k))
        if not torch.is_tensor(pred["pred_angles0"]) or pred["pred_angles0"].dim() < 1:
            raise RuntimeError("%s: pred_angles0 must be a (L, 22, 3) tensor" % NAME)
        L = pred["pred_angles0"].shape[0]
        windows(L, self.chunk)
        got = self._tensors([(pred[k], (L,) + shape, k) for k, shape in PRED_KEYS.items()] + [(detections, (2, L, 2, 24, 3), "detections")])
        p, det = dict(zip(PRED_KEYS, got)), got[-1]
        dev = self.device
        (W1, b1, Wmu, bmu), _ = self._weights()
        z = torch.empty(L, NZ, device=dev)
        phi, tau = torch.empty(2, L, 6, device=dev), torch.empty(2, L, 3, device=dev)
        j2d = torch.empty_like(det)
        robust = torch.empty(L, device=dev, dtype=torch.int32)
        with torch.cuda.device(dev):
            G.check(G.lib().apg_seq_init(L, G.vp(p["pred_angles0"]), G.vp(p["pred_angles1"]), G.vp(p["pred_smpltrans0"]),
                                         G.vp(p["pred_smpltrans1"]), G.vp(det), G.vp(W1), G.vp(b1), G.vp(Wmu), G.vp(bmu),
                                         float(agreement_px), float(robust_conf), G.vp(z), G.vp(phi), G.vp(tau), G.vp(j2d),
                                         G.vp(robust), G.stream(dev)), "apg_seq_init")
        state = {"z": z, "phi0": phi[0], "phi1": phi[1], "tau0": tau[0], "tau1": tau[1]}
        return state, {"j2d": j2d, "robust": robust.cpu()}

    def fit(self, state, data, intr, extr=None, n_iters=300, switch_iter=SWITCH_ITER, carry_hip_decay=True, want_loss=False, **hyper):
        for k in hyper:
            if k not in HYPER:
                raise TypeError("%s.fit: unknown argument %r (the fitter's hyper-parameters are %s)" % (NAME, k, ", ".join(HYPER)))
        for k in STATE_KEYS:
            if k not in state:
                raise RuntimeError("%s: state has no %r" % (NAME, k))
        if not torch.is_tensor(state["z"]) or state["z"].dim() < 1:
            raise RuntimeError("%s: z must be a (L, 32) tensor" % NAME)
        L = state["z"].shape[0]
        wins = windows(L, self.chunk)
        for k in ("j2d", "robust"):
            if k not in data:
                raise RuntimeError("%s: data has no %r" % (NAME, k))
        robust = torch.as_tensor(data["robust"]).to(torch.int32).cpu()
        if robust.shape != (L,):
            raise RuntimeError("%s: robust must be (%d,), got %s" % (NAME, L, tuple(robust.shape)))
        got = self._tensors([(state[k], (L,) + shape, k) for k, shape in STATE_KEYS.items()] +
                            [(data["j2d"], (2, L, 2, 24, 3), "j2d"), (intr, (2, 4), "intr")] + ([] if extr is None else [(extr, (2, 3, 4), "extr")]))
        st, j2d, intr = dict(zip(STATE_KEYS, got)), got[len(STATE_KEYS)], got[len(STATE_KEYS) + 1]
        extr = torch.eye(4, device=self.device)[:3].repeat(2, 1, 1) if extr is None else got[-1]
        if n_iters < 1:
            raise ValueError("%s: n_iters must be at least 1, got %r" % (NAME, n_iters))
        out = {k: torch.empty_like(st[k]) for k in STATE_KEYS}
        betas, losses = [], []
        for k, (a, b) in enumerate(wins):
            first = k * int(n_iters) if carry_hip_decay else 0
            s = {key: st[key][a:b] for key in STATE_KEYS}
            s["beta"] = torch.zeros(10, device=self.device)
            res = self.fitter.run(s, j2d[:, a:b], robust[a:b], intr, extr, n_iters=int(n_iters), first_iter=first,
                                  switch_iter=first + int(switch_iter), want_loss=want_loss, **hyper)
            if want_loss:
                res, hist = res
                losses.append(hist)
            for key in STATE_KEYS:
                out[key][a:b] = res[key]
            betas.append(res["beta"])
        out.update(beta=torch.stack(betas), chunks=wins, robust=robust)
        if want_loss:
            out["loss"] = losses
        return out

    def export(self, result, frames=None, want_vertices=True):
        for k in tuple(STATE_KEYS) + ("beta", "chunks"):
            if k not in result:
                raise RuntimeError("%s: result has no %r" % (NAME, k))
        if not torch.is_tensor(result["z"]) or result["z"].dim() < 1:
            raise RuntimeError("%s: z must be a (L, 32) tensor" % NAME)
        L = result["z"].shape[0]
        wins = [(int(a), int(b)) for a, b in result["chunks"]]
        if not wins or wins[0][0] != 0 or wins[-1][1] != L or any(a >= b for a, b in wins) or \
                any(wins[i][1] != wins[i + 1][0] for i in range(len(wins) - 1)):
            raise RuntimeError("%s: chunks must be consecutive windows covering 0 .. %d, got %s" % (NAME, L, wins))
        got = self._tensors([(result[k], (L,) + shape, k) for k, shape in STATE_KEYS.items()] + [(result["beta"], (len(wins), 10), "beta")])
        st, beta = dict(zip(STATE_KEYS, got)), got[-1]
        if frames is not None and not isinstance(frames, slice):
            raise TypeError("%s: frames must be a slice or None, got %s" % (NAME, type(frames).__name__))
        dev = self.device
        _, dec = self._weights()
        phi, tau = torch.stack([st["phi0"], st["phi1"]]), torch.stack([st["tau0"], st["tau1"]])
        thetas = torch.empty(L, 63, device=dev)
        rr, T, C = torch.empty(2, L, 3, 3, device=dev), torch.empty(2, L, 4, 4, device=dev), torch.empty(L, 4, 4, device=dev)
        with torch.cuda.device(dev):
            G.check(G.lib().apg_seq_export(L, G.vp(st["z"]), G.vp(phi), G.vp(tau), *[G.vp(t) for t in dec], G.vp(thetas), G.vp(rr),
                                           G.vp(T), G.vp(C), G.stream(dev)), "apg_seq_export")
        betas = torch.repeat_interleave(beta, torch.tensor([b - a for a, b in wins], device=dev), dim=0)
        out = {"thetas": thetas, "betas": betas, "root_rot0": rr[0], "root_rot1": rr[1], "trans0": tau[0], "trans1": tau[1],
               "smpl_wrt_cam0": T[0], "smpl_wrt_cam1": T[1], "cam1_wrt_cam0": C}
        if want_vertices:
            sl = slice(None) if frames is None else frames
            out["frames"] = sl
            v, j = self._meshes(thetas[sl], betas[sl], T[:, sl])
            out.update(pred_vertices_cam0=v[0], pred_vertices_cam1=v[1], pred_j3d_cam0=j[0], pred_j3d_cam1=j[1])
        return out

    def _meshes(self, thetas, betas, T):
        """the bodies of `thetas` / `betas` (n frames) in both cameras: BodyModel.forward with root_orient = 0 and its zero defaults
        for jaw, eyes and HANDS (not this package's PCA hand mean) -- lbs.batch_rodrigues (angle = |r + 1e-8|, the fitter's chain) on
        the body pose, the identity everywhere else -- then transform_smpl per view"""
        from . import lbs, utils
        dev, n = self.device, thetas.shape[0]
        V = self.body.num_verts
        verts = [torch.empty(n, V, 3, device=dev) for _ in (0, 1)]
        joints = None
        for a in range(0, n, MESH_BATCH):
            b = min(a + MESH_BATCH, n)
            R = lbs.batch_rodrigues(thetas[a:b].reshape(-1, 3)).reshape(b - a, 21, 3, 3)
            eye = lambda m: torch.eye(3, device=dev).expand(b - a, m, 3, 3).contiguous()
            o = self.body.forward(betas=betas[a:b].contiguous(), body_pose=R, global_orient=eye(1), jaw_pose=eye(1), leye_pose=eye(1),
                                  reye_pose=eye(1), left_hand_pose=eye(15), right_hand_pose=eye(15), pose2rot=False)
            if joints is None:
                joints = [torch.empty(n, o.joints.shape[1], 3, device=dev) for _ in (0, 1)]
            for v in (0, 1):
                verts[v][a:b], joints[v][a:b], _, _ = utils.transform_smpl(T[v, a:b, :3].contiguous(), o.vertices, o.joints)
        if joints is None:
            joints = [torch.empty(0, 127, 3, device=dev) for _ in (0, 1)]
        return verts, joints

    def __call__(self, pred, detections, intr, extr=None, frames=None, want_vertices=True, agreement_px=AGREEMENT_PX,
                 robust_conf=ROBUST_CONF, **fit_args):
        state, data = self.prepare(pred, detections, agreement_px=agreement_px, robust_conf=robust_conf)
        result = self.fit(state, data, intr, extr, **fit_args)
        out = self.export(result, frames=frames, want_vertices=want_vertices)
        out["result"] = result
        return out
