"""fp64 ground truth for apg_grad_norm, apg_grad_scale and apg_adam_step_guarded (airpose_amd/csrc/guard/grad_guard.hip) through the C ABI of
include/airpose_grad.h.  The reference, the bars and how they were counted are in gradnorm_util.py; C = 4096 is the kernels' chunk and
T = 192 the tensors one norm launch carries.

Shapes.  numel in {0, 1, 3, 4, 5, C - 1, C, C + 1, 2 C + 3} in one call; calls of 1, T and T + 1 tensors; one mixed call of 2 T + 5
tensors with empty ones among them.  Gradients as test_optim_fp64 draws them (|g| log-uniform in [1e-8, 1e-1], a tenth exact zeros),
plus the two range cases on C + 1 elements -- every |g| = 1e19 (an fp32 sum overflows; the norm, 6.4e20, is finite) and every
|g| = 1e-30 (fp32 squares flush; the norm, 6.4e-29, is not zero) -- and one case in which eps matters (norm near 1e-5 clipped to 1e-6).
Every call runs twice into fresh buffers (bit-equal), with the gradients between NaN guard bands (a read outside a tensor would make
the norm NaN) and the workspace, per_tensor and the record starting as NaN / garbage.

CPU self-check (no GPU): emulate_norm() / emulate_guarded(), an evaluation of the kernels' exact sequence, stay inside every bar on
the same cases, and each mutation of NORM_MUTATIONS / STEP_MUTATIONS is rejected by at least one case.
"""
import math

import pytest
import torch

import gradnorm_util as U
import test_optim_fp64 as F

C, T = U.C, U.T
INF, NAN = float("inf"), float("nan")


def _cases():
    """name -> (gradients, max_norm): what the CPU emulation and the GPU both run"""
    sizes = U.make_grads(U.SIZES)
    ref = U.reference(sizes, 1.0)["norm"]
    eps_g, eps_max = U.eps_case()
    return {
        "sizes-clipped": (sizes, 0.5 * ref),
        "sizes-above": (sizes, 4.0 * ref),
        "sizes-zero": (sizes, 0.0),
        "sizes-inf": (sizes, INF),
        "all-zero": ([torch.zeros(n) for n in U.SIZES], 1.0),
        "only-empty": ([torch.zeros(0), torch.zeros(0)], 1.0),
        "no-tensor": ([], 0.25),
        "huge": (U.constant_grads(1e19), 1.0),
        "tiny": (U.constant_grads(1e-30), 1e-30),
        "eps": (eps_g, eps_max),
        "one": (U.make_grads((2 * C + 3,), seed=1), 0.01),
        "T": (U.make_grads([s for s in U.mixed_sizes(T)], seed=2), 0.05),
        "T+1": (U.make_grads([s or 7 for s in U.mixed_sizes(T + 1)], seed=3), 0.05),
        "mixed": (U.make_grads(U.mixed_sizes(2 * T + 5), seed=4), 0.1),
    }


CASES = _cases()


def test_cases_are_what_the_docstring_promises():
    ref = lambda k: U.reference(*CASES[k])
    assert 6.3e20 < ref("huge")["norm"] < 6.5e20 and 6.3e-29 < ref("tiny")["norm"] < 6.5e-29
    assert 0.9e-5 < ref("eps")["norm"] < 1.1e-5 and abs(ref("eps")["coef"] - 1.0 / 11.0) < 1e-3
    assert ref("sizes-clipped")["coef"] < 0.51 and ref("sizes-above")["coef"] == 1.0 and ref("sizes-zero")["coef"] == 0.0
    assert ref("sizes-inf")["coef"] == 1.0
    assert len(CASES["T"][0]) == T and len(CASES["T+1"][0]) == T + 1 and len(CASES["mixed"][0]) == 2 * T + 5
    assert sum(g.numel() == 0 for g in CASES["mixed"][0]) > 40 and any(g.numel() == 0 for g in CASES["T"][0])
    assert all(ref(k)["coef"] < 0.9 for k in ("one", "T", "T+1", "mixed", "tiny")), "these cases are meant to clip"


@pytest.mark.parametrize("name", sorted(CASES))
def test_cpu_emulation_is_inside_every_bar(name):
    grads, max_norm = CASES[name]
    got = U.emulate_norm(grads, max_norm)
    assert not U.verify(got, grads, max_norm), U.verify(got, grads, max_norm)
    if name in ("all-zero", "only-empty", "no-tensor"):
        assert got["norm"] == 0.0 and got["coef"] == 1.0


@pytest.mark.parametrize("mut", U.NORM_MUTATIONS)
def test_cpu_norm_mutations_are_rejected(mut):
    caught = [name for name, (grads, max_norm) in sorted(CASES.items()) if U.verify(U.emulate_norm(grads, max_norm, mut=mut), grads, max_norm)]
    print(mut, "rejected by", caught)
    want = dict(fp32_accumulation=("huge", "tiny"), no_eps=("eps",), eps_inside_sqrt=("eps",), no_clamp=("sizes-above",),
                sum_of_norms=("mixed", "sizes-clipped"))[mut]
    assert all(w in caught for w in want), (mut, caught)


def _nonfinite(where, value):
    """the gradients of the non-finite cases: value placed at element 0 of tensor 0, at the last element of a tensor with C + 1
    elements (the one-by-one tail), or in a tensor whose index is beyond T"""
    if where == "first":
        grads = U.make_grads((37, C + 1, 5), seed=5)
        grads[0][0] = value
    elif where == "tail":
        grads = U.make_grads((37, C + 1, 5), seed=5)
        grads[1][C] = value
    else:
        grads = U.make_grads([(5, 64, 3)[i % 3] for i in range(T + 4)], seed=6)
        grads[T + 2][1] = value
    return grads


@pytest.mark.parametrize("value", [INF, -INF, NAN], ids=["inf", "-inf", "nan"])
@pytest.mark.parametrize("where", ["first", "tail", "beyond-T"])
def test_cpu_emulation_of_the_nonfinite_cases(where, value):
    grads = _nonfinite(where, value)
    for skip in (True, False):
        got = U.emulate_norm(grads, 1.0, skip_nonfinite=skip)
        assert not U.verify(got, grads, 1.0, skip_nonfinite=skip), (skip, got)
        assert got["skip"] == int(skip) and (got["coef"] == 1.0 if skip else math.isnan(got["coef"])) and not math.isfinite(got["norm"])


def _step_case():
    call = F.make_call((5, C + 1, 259, 2 * C + 3), (2, 1000, 1, 2), seed=3)
    return call, F.hyper(lr=5e-5, wd=1e-4, amsgrad=True)


def _step_fails(call, h, coef, skip, got):
    """a guarded step's outputs against the rule: skip -> the inputs bit for bit; else test_optim_fp64's bars around the fp64 step on g2"""
    if skip:
        return [] if F.bit_equal(got, U.inputs_of(call, h)) else [("skip", "a skipped step changed p, m, v or vmax")]
    return F.verify(U.clipped_call(call, coef), h, got, "guarded")


def test_cpu_guarded_step_emulation_and_its_mutations():
    call, h = _step_case()
    for coef, skip in ((0.37, 0), (1.0, 0), (1.0, 1)):
        assert not _step_fails(call, h, coef, skip, U.emulate_guarded(call, h, coef, skip))
    assert F.bit_equal(U.emulate_guarded(call, h, 1.0, 0), F.emulate(call, h))           # coef = 1: the unguarded sequence
    assert _step_fails(call, h, 0.37, 0, U.emulate_guarded(call, h, 0.37, 0, mut="coef_after_weight_decay"))
    assert _step_fails(call, h, 1.0, 1, U.emulate_guarded(call, h, 1.0, 1, mut="skip_updates_m"))
    assert set(U.STEP_MUTATIONS) == {"coef_after_weight_decay", "skip_updates_m"}


# ------------------------------------------------------------------------------------------------ the GPU
@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda", 0)


def _twice(grads, max_norm, dev, **kw):
    a = U.run_norm(grads, max_norm, dev, **kw)
    b = U.run_norm(grads, max_norm, dev, **kw)
    assert U.same_record(a, b), "two runs differ"
    assert all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a["g"], b["g"])), "two runs left other gradients"
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_norm_coef_and_per_tensor_against_fp64(dev, name):
    grads, max_norm = CASES[name]
    got = _twice(grads, max_norm, dev)
    ref = U.reference(grads, max_norm)
    print("%-14s norm %.9g (ref %.17g) coef %.9g (ref %.17g) skip %d" % (name, got["norm"], ref["norm"], got["coef"], ref["coef"], got["skip"]))
    fails = U.verify(got, grads, max_norm)
    assert not fails, fails
    if name in ("all-zero", "only-empty", "no-tensor"):
        assert got["norm"] == 0.0 and got["coef"] == 1.0 and got["skip"] == 0
    if name in ("huge", "tiny"):                                              # the range cases do not flag
        assert math.isfinite(got["norm"]) and got["norm"] > 0 and got["skip"] == 0
        assert _twice(grads, max_norm, dev, skip_nonfinite=True)["skip"] == 0
    if name == "sizes-zero":
        assert got["coef"] == 0.0
    # per_tensor is optional
    assert U.same_record(dict(got, per_tensor=None), _twice(grads, max_norm, dev, per_tensor=False))


@pytest.mark.gpu
@pytest.mark.parametrize("off", [1, 2, 3])
def test_pointers_off_a_16_byte_boundary_give_the_same_bits(dev, off):
    for name in ("sizes-clipped", "T+1"):
        grads, max_norm = CASES[name]
        base = _twice(grads, max_norm, dev)
        assert U.same_record(base, _twice(grads, max_norm, dev, off=off)), (name, off)
        mixed = [(off, 0, (off + 1) % 4, 3)[i % 4] for i in range(len(grads))]
        assert U.same_record(base, _twice(grads, max_norm, dev, off=mixed)), (name, mixed[:4])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["sizes-clipped", "sizes-zero", "eps", "mixed"])
def test_scale_is_one_rounded_product_with_the_coef_read_back(dev, name):
    grads, max_norm = CASES[name]
    for off in (0, 1):
        got = _twice(grads, max_norm, dev, scale=True, off=off)
        assert got["coef"] != 1.0
        c = torch.tensor(got["coef"], dtype=torch.float32)
        for i, (g, s) in enumerate(zip(grads, got["g"])):
            assert torch.equal((g * c).view(torch.int32), s.view(torch.int32)), (name, off, i)


@pytest.mark.gpu
def test_scale_with_coef_one_stores_nothing(dev):
    """-0.0 and NaN payloads inside the tensors keep their bits (coef = 1 from max_norm = +inf would otherwise rewrite a signalling
    NaN), as do the guard bands (run_norm checks those)"""
    grads = U.make_grads((37, C + 1, 2 * C + 3), seed=8)
    grads[0][3] = -0.0
    grads[1][C] = -0.0
    odd = torch.tensor([0x7fa00001, -0x00400001], dtype=torch.int32).view(torch.float32)       # a signalling and a negative quiet NaN
    grads[2][5], grads[2][2 * C + 2] = odd[0], odd[1]
    for skip, max_norm in ((True, 1e-3), (False, None)):
        if max_norm is None:                                                  # finite gradients, max_norm above the norm
            grads[2][5], grads[2][2 * C + 2] = -0.0, -0.0
            max_norm = INF
        got = _twice(grads, max_norm, dev, skip_nonfinite=skip, scale=True)
        assert got["coef"] == 1.0 and got["skip"] == int(skip)
        for g, s in zip(grads, got["g"]):
            assert torch.equal(g.view(torch.int32), s.view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("value", [INF, -INF, NAN], ids=["inf", "-inf", "nan"])
@pytest.mark.parametrize("where", ["first", "tail", "beyond-T"])
def test_nonfinite_gradients_flag_skip_and_count(dev, where, value):
    grads = _nonfinite(where, value)
    counters = torch.zeros(2, dtype=torch.int64, device=dev)
    fine = U.make_grads((37, C + 1, 5), seed=5)
    assert _twice(fine, 1.0, dev, skip_nonfinite=True, counters=counters)["skip"] == 0
    got = _twice(grads, 1.0, dev, skip_nonfinite=True, counters=counters)
    assert not U.verify(got, grads, 1.0, skip_nonfinite=True), got
    assert got["skip"] == 1 and got["coef"] == 1.0 and not math.isfinite(got["norm"])
    # a guarded step with this record leaves p, m, v, vmax bit-identical
    call, h = _step_case()
    for ams in (True, False):
        hh = dict(h, amsgrad=ams)
        assert F.bit_equal(U.run_guarded(call, hh, dev, got["record"]), U.inputs_of(call, hh))
    off = _twice(grads, 1.0, dev, skip_nonfinite=False, counters=counters)
    assert not U.verify(off, grads, 1.0, skip_nonfinite=False), off
    assert off["skip"] == 0 and math.isnan(off["coef"]) and not math.isfinite(off["norm"])
    assert counters.cpu().tolist() == [6, 2]                                  # seen counts every call (2 + 2 + 2), skipped the two that set skip


@pytest.mark.gpu
@pytest.mark.parametrize("step", [1, 1000])
@pytest.mark.parametrize("wd", [0.0, 1e-4])
@pytest.mark.parametrize("amsgrad", [True, False])
def test_guarded_step_is_the_plain_step_on_the_clipped_gradient(dev, amsgrad, wd, step):
    """apg_adam_step_guarded == apg_adam_step on g2 = float32(coef) * g, bit for bit: test_optim_fp64's bars carry over as they are"""
    sizes = (1, 3, 4, 5, C - 1, C, C + 1, 2 * C + 3)
    call = F.make_call(sizes, [step] * len(sizes), seed=11)
    h = F.hyper(lr=1e-3, wd=wd, amsgrad=amsgrad)
    grads = [t["g"] for t in call]
    ref = U.reference(grads, 1.0)["norm"]
    for max_norm in (0.3 * ref, INF):
        rec = _twice(grads, max_norm, dev)
        assert (rec["coef"] == 1.0) == (max_norm == INF) and rec["skip"] == 0
        got = U.run_guarded(call, h, dev, rec["record"])
        again = U.run_guarded(call, h, dev, rec["record"])
        want = F.run(U.clipped_call(call, rec["coef"]), h, dev)
        assert F.bit_equal(got, again) and F.bit_equal(got, want), (max_norm, amsgrad, wd, step)
        if max_norm == INF:
            assert F.bit_equal(got, F.run(call, h, dev))
        else:
            assert not F.bit_equal(got, F.run(call, h, dev))                  # the clip did something
