"""The rounding probe nets (tests/rounding_nets.py) on the CPU: every net and
batch that tests/test_gpu_resnet_rounding.py runs meets the exactness and
coverage conditions; the reference's explicit integer round-to-nearest-even is
tied to independent code (torch's bfloat16 / float16 casts in a float64 / float32
emulation of the spec, and oracle/resnet_ref.py with the roundings switched
off); and the comparison rejects every wrong rounding rule a kernel or loader
could follow (reference(mutant) against reference, on rows the GPU tests use).
"""

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_nets as E
import resnet_ref
import rounding_nets as Rn

IDS = [Rn.case_id(a) for a, _ in Rn.ALL_CASES]
TORCH_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}
MUTANT_ROWS = 128  # a prefix of every case's large batch


def test_rne_is_torchs_cast_and_the_wrong_modes_are_wrong():
    rng = np.random.default_rng(5)
    y = np.concatenate([rng.integers(-60000, 60000, 100000).astype(np.float64),
                        rng.standard_normal(50000).astype(np.float32).astype(np.float64) * 8,
                        [0.0, -0.0, 255.5, 256.5, 257.5, 258.5, -2049.0, -2051.0, 2.0 - 2.0 ** -12]])
    y = y[(np.abs(y) > 1e-3) | (y == 0)]
    for dtype, tt in TORCH_DTYPE.items():
        p = Rn.P_BITS[dtype]
        r = Rn.rne(y, p)
        t = torch.from_numpy(y).to(tt).to(torch.float64).numpy()
        assert np.array_equal(r, t) and np.array_equal(np.signbit(r), np.signbit(t))
        inexact, down, up = Rn.classify(y, p)
        assert np.array_equal(inexact, r != y) and down.sum() > 100 and up.sum() > 100
        tr, aw = Rn.rne(y, p, "trunc"), Rn.rne(y, p, "away")
        assert (np.abs(tr) <= np.abs(y)).all() and np.array_equal(tr == y, ~inexact)
        assert np.array_equal(aw != r, down)  # ties to even that went toward zero go away from it


# ------------------------------------------------------------------ conditions
@pytest.mark.parametrize("args,rows", Rn.ALL_CASES, ids=IDS)
def test_conditions_of_every_gpu_case(args, rows):
    """Rn.case asserts per layer, over the master batch of which every GPU
    batch is a prefix: the 2^24-unit bound, that every value is a multiple of
    the unit, normal numbers the dtype holds, fp16 magnitudes <= 2^15, the
    heads' bounds. Re-asserted here: the scales and the coverage conditions."""
    dtype, family, C, R, cin, hid = args
    sd, x, ref = Rn.case(*args)
    assert max(rows) <= len(x)
    Rn.check_scales(ref)
    assert len(ref.layers) == 1 + 2 * R and ref.head_bound < E.SUM_BOUND
    assert all(s.bound_units < E.SUM_BOUND for s in ref.layers)
    if dtype == "fp16":
        assert max(s.max_pre for s in ref.layers) <= Rn.FP16_PRE_MAX
    assert ref.z.std() > 0.1 and ref.logits.std(axis=0).min() > 0
    p = Rn.P_BITS[dtype]
    if family == "R":
        assert not Rn.coverage_failures(ref, dtype)
        kinds = {k for s in ref.layers for k in s.kinds}
        assert kinds == ({"first", "last"} | ({"conv1", "conv2"} if R else set()))
        assert all(0.03 <= s.live <= 0.5 for s in ref.layers), [s.live for s in ref.layers]
        w0, _ = E.fold(sd, "conv_block.conv", "conv_block.norm")
        assert np.abs(w0).max() > Rn.FIRST_WMAX[dtype] / 2 and Rn.representable(w0.astype(np.float64), p)
        for pc, pn in E.conv_layers(sd):  # biases the dtype does not hold
            _, b = E.fold(sd, pc, pn)
            assert not Rn.representable(b.astype(np.float64), p), pc
    elif family == "L":
        cond = Rn.loader_conditions(sd, dtype)
        assert cond["inexact"] >= C and min(cond.values()) >= 4, cond
    else:
        for name in ("policy_head", "value_head"):
            w, _ = E.fold(sd, name + ".conv", name + ".norm")
            w = w[w != 0].astype(np.float64)
            inexact, down, up = Rn.classify(w, p)
            assert inexact.all() and down.any() and up.any(), name


# ------------------------------------------------------------------ links to independent code
def _torch_emulation(sd, x, dtype):
    """The spec in torch: float64 convolutions (exact), the accumulator's
    value checked to fit fp32, rounding by tensor.to(bfloat16 / float16)."""
    tt = TORCH_DTYPE[dtype]

    def cast(t):
        assert torch.equal(t.to(torch.float32).to(torch.float64), t), "the fp32 accumulator would not hold this"
        return t.to(torch.float32).to(tt).to(torch.float64)

    def folded(pc, pn):
        w, b = E.fold(sd, pc, pn)
        return torch.from_numpy(w).to(tt).to(torch.float64), torch.from_numpy(b).to(torch.float64)

    a = torch.from_numpy(np.array(x)).to(torch.float64)
    stored, skip = [], None
    for layer, (pc, pn) in enumerate(E.conv_layers(sd)):
        w, b = folded(pc, pn)
        if layer % 2 == 1:
            skip = a
        y = F.conv2d(a, w, b, padding=1)
        if layer > 0 and layer % 2 == 0:
            y = y + skip
        a = torch.relu(cast(y))
        stored.append(a)
    wp, bp = folded("policy_head.conv", "policy_head.norm")
    wv, bv = folded("value_head.conv", "value_head.norm")
    pol = torch.relu(F.conv2d(a, wp, bp)).flatten(1)
    val = torch.relu(F.conv2d(a, wv, bv)).flatten(1)
    d = lambda k: torch.from_numpy(np.asarray(sd[k])).to(torch.float64)  # noqa: E731
    logits = F.linear(pol, d("policy_head.linear.weight"), d("policy_head.linear.bias"))
    hidden = torch.relu(F.linear(val, d("value_head.linear1.weight"), d("value_head.linear1.bias")))
    z = F.linear(hidden, d("value_head.linear2.weight"), d("value_head.linear2.bias"))[:, 0]
    return stored, logits.numpy(), z.numpy()


@pytest.mark.parametrize("args,rows", Rn.ALL_CASES, ids=IDS)
def test_reference_matches_torch_casts_bit_for_bit(args, rows):
    sd, x, ref = Rn.case(*args)
    n = 32
    keep = []
    got = Rn.forward_rounded(sd, x[:n], args[0], keep=keep)
    assert np.array_equal(got.logits, ref.logits[:n]) and np.array_equal(got.z, ref.z[:n])  # prefix = own batch
    stored, logits, z = _torch_emulation(sd, x[:n], args[0])
    assert len(stored) == len(keep)
    for layer, (mine, theirs) in enumerate(zip(keep, stored)):
        theirs = theirs.numpy().transpose(1, 0, 2, 3).reshape(mine.shape)
        assert np.array_equal(mine, theirs) and not np.signbit(mine).any(), f"conv layer {layer}"
    assert np.array_equal(got.logits, logits) and np.array_equal(got.z, z)


@pytest.mark.parametrize("args", [("bf16", "R", 128, 1, 17, 64), ("fp16", "L", 128, 0, 17, 64),
                                  ("bf16", "H", 256, 0, 17, 64)], ids=Rn.case_id)
def test_without_roundings_the_reference_is_the_fp32_restatement(args):
    """With every rounding switched off these nets stay exact in fp32 (integer
    sums below 2^24; single products of short weights), so forward_rounded
    and oracle/resnet_ref.py compute the same function."""
    sd, x, _ = Rn.case(*args)
    n = 24
    got = Rn.forward_rounded(sd, x[:n], None)
    out = resnet_ref.forward(sd, torch.from_numpy(np.array(x[:n])))
    p, v = E.outputs_of(got)
    dp = np.abs(out["policy"].numpy() - p).max()
    dv = np.abs(out["value"].numpy() - v).max()
    assert dp <= 1e-5 and dv <= 1e-5, (dp, dv)


# ------------------------------------------------------------------ wide-range heads
@pytest.mark.parametrize("which", ["policy", "value"])
def test_wide_range_heads_conditions(which):
    """Rn.wide_heads_case asserts the spread (64-80, < 87), the offset, that
    the maximum sits on action 64 in some rows and on a square in others, and
    |z| in (6, 9]; the float64 expectation, rounded to float32 as a correct
    kernel's outputs are, meets the criteria with room; a row's largest
    probability off by 2^-19 relative (twice its bound) does not."""
    sd, x, ref = Rn.wide_heads_case(which)
    p, v, d = Rn.wide_outputs(ref)
    assert np.isfinite(p).all() and p.min() >= 2.0 ** -126  # normal fp32 numbers
    p32, v32 = p.astype(np.float32), v.astype(np.float32)
    dev = Rn.wide_deviations(p32, v32, ref)
    assert dev["rel_over_bound"] <= 0.1 and dev["sum_err"] <= 1e-5 and dev["value_err"] <= 1e-7, dev
    if which == "policy":
        assert (ref.logits.argmax(1) == 64).any() and (ref.logits.argmax(1) < 64).any()
        bad = p32.copy()
        bad[np.arange(len(bad)), ref.logits.argmax(1)] *= np.float32(1 + 2.0 ** -19)
        assert Rn.wide_deviations(bad, v32, ref)["rel_over_bound"] > 1.0
    n = 16
    out = resnet_ref.forward(sd, torch.from_numpy(np.array(x[:n])))
    assert np.abs(out["policy"].numpy() - p[:n]).max() <= 1e-5 and np.abs(out["value"].numpy() - v[:n]).max() <= 1e-5


# ------------------------------------------------------------------ the tests have teeth
def _applicable(args):
    _, family, _, R, _, _ = args
    if family == "R":
        return ("trunc", "away", "relu_late", "bias16") + (("round_before_skip", "skip_unrounded") if R else ())
    return ("w_trunc", "w_double") if family == "L" else ("head_fp32",)


def test_every_mutant_has_cases():
    seen = {m for a, _ in Rn.ALL_CASES for m in _applicable(a)}
    assert seen == set(Rn.MUTANTS)


@pytest.mark.parametrize("args,rows", Rn.ALL_CASES, ids=IDS)
def test_comparison_rejects_every_wrong_rounding(args, rows):
    """Mutants (rounding_nets.MUTANTS): truncation; round-half-away; a ReLU
    that lets -0 / tiny negatives through; rounding before the skip is added;
    the skip taken from the unrounded value; bias rounded to the dtype (tower
    nets); tower weights truncated, or rounded from the double product (loader
    nets); head-conv weights left in fp32 (head-conv nets). Each must fail
    exact_nets.compare on the first MUTANT_ROWS rows of the case's batch."""
    sd, x, ref = Rn.case(*args)
    n = MUTANT_ROWS
    assert n <= max(rows)
    want = ref.rows(n)
    p0, v0 = E.outputs_of(want)
    d = E.compare(p0, v0, want, "unmutated")
    assert d["policy_steps"] < 0.05 and d["value_steps"] < 0.05  # float32 outputs
    missed = []
    for m in _applicable(args):
        got = Rn.forward_rounded(sd, x[:n], args[0], mut=(m,))
        p, v = E.outputs_of(got)
        try:
            E.compare(p, v, want, m)
        except AssertionError:
            pass
        else:
            missed.append(m)
        if m == "head_fp32":
            # the fp32 folded weights (what the fp32 restatement multiplies
            # with) move at least half the rows by a step or more
            moved_l = (np.abs(got.logits - want.logits).max(1) >= want.step).mean()
            moved_z = (np.abs(got.z - want.z) >= want.step_v).mean()
            assert moved_l >= 0.5 and moved_z >= 0.5, (moved_l, moved_z)
    assert not missed, f"wrong roundings the comparison does not flag: {missed}"
