"""Zero-slack tests of the fused ResNet's 16-bit roundings (csrc/resnet.hip's
pack_relu epilogue and accumulator start, csrc/capi_net.hip's weight loader) on
the rounding probe nets of tests/rounding_nets.py: nets whose fp32 sums are
exact in any order but whose layer results do not fit bf16 / fp16, so what
the kernel stores is one specific rounded number that the integer reference
predicts bit for bit. The kernel must reproduce the reference's logits and
value pre-activation to a quarter of the smallest change one wrong rounding
can cause (exact_nets.compare, unchanged): truncation, round-half-away, a
rounding before the skip is added, a truncating loader, head-conv weights left
in fp32 each fail it (tests/test_cpu_rounding_nets.py shows that on the CPU,
for exactly these cases). Every case runs with one board per workgroup and in
the throughput geometries with a ragged last workgroup, C=128 under both
settings of native.set_c128_four_wave, which must also agree bit for bit.
The terminal summary lists every case's largest deviation in steps (limit
0.25) and the wide-range heads' largest relative error next to its bound."""

import numpy as np
import pytest
import torch

import exact_nets as E
import numerics
import rounding_nets as Rn

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SWITCH = (True, False)  # 4-wave, 8-wave


@pytest.fixture(scope="module")
def om():
    import othello_mcts

    return othello_mcts


@pytest.fixture()
def four_wave(om):
    """Sets the switch for a test and restores the build's default after it."""
    from othello_mcts import native

    default = native.c128_four_wave()
    yield native.set_c128_four_wave
    native.set_c128_four_wave(default)


def _check(out, ref, label, failed):
    def report(d):
        numerics.record(f"resnet rounding {label}",
                        f"policy {d['policy_steps']:.2e} steps (row {d['row']} action {d['action']}), "
                        f"value {d['value_steps']:.2e} steps, |sum p - 1| {d['sum_err']:.1e}")
    try:
        E.compare(out["policy"].cpu().numpy(), out["value"].cpu().numpy(), ref, label, report)
    except AssertionError as e:
        failed.append(str(e))


def _run(om, four_wave, args, rows):
    """One NativeNet per case, used for every row count; every row count and
    geometry runs, the report names all that fail."""
    dtype, _, C, _, _, _ = args
    sd, x, ref = Rn.case(*args)
    net = om.NativeNet(sd, device=0, dtype=dtype)
    failed = []
    for n in rows:
        xs = torch.from_numpy(np.array(x[:n])).to(DEV)
        label = f"{Rn.case_id(args)} rows={n}"
        if C == 128 and n >= 1024:
            out = {}
            for v in SWITCH:
                four_wave(v)
                out[v] = net(xs)
                torch.cuda.synchronize()
                _check(out[v], ref.rows(n), f"{label} four_wave={v}", failed)
            if not all(torch.equal(out[True][k], out[False][k]) for k in ("policy", "value")):
                failed.append(f"{label}: the 4-wave and 8-wave geometries differ")
        else:
            out = net(xs)
            torch.cuda.synchronize()
            _check(out, ref.rows(n), label, failed)
    assert not failed, "\n".join(failed)


def _ids(cases):
    return [Rn.case_id(a) for a, _ in cases]


@pytest.mark.parametrize("args,rows", Rn.TOWER, ids=_ids(Rn.TOWER))
def test_tower_rounding(om, four_wave, args, rows):
    """Family R: every conv layer's result needs rounding (first conv, a
    block's two convs with the skip added before the one rounding, the last
    layer), with ties both ways, inexact negatives and values next to zero on
    either side; biases the dtype does not hold."""
    _run(om, four_wave, args, rows)


@pytest.mark.parametrize("args,rows", Rn.LOADER, ids=_ids(Rn.LOADER))
def test_loader_rounding(om, four_wave, args, rows):
    """Family L: folded fp32 tower weights the dtype does not hold (the
    loader's f32_to_bf16_rne / _Float16 cast, after the double -> float
    cast), ties both ways."""
    _run(om, four_wave, args, rows)


@pytest.mark.parametrize("args,rows", Rn.HEADCONV, ids=_ids(Rn.HEADCONV))
def test_head_conv_rounding(om, four_wave, args, rows):
    """Family H: head 1x1 conv weights the dtype does not hold; the kernel
    multiplies with their dtype-rounded values."""
    _run(om, four_wave, args, rows)


@pytest.mark.parametrize("dtype", Rn.DTYPES)
@pytest.mark.parametrize("which", ["policy", "value"])
def test_wide_range_heads(om, which, dtype):
    """Logit spread 64-80 at an absolute size of +200, the maximum on action
    64 in some rows and on a square in others; |z| up to 9. Expected: float64
    softmax / tanh of the exact logits. Policy: relative error at most
    2^-23 (|o - m| + 8) per probability (rounding_nets.WIDE_REL: derived from
    __expf = exp2 of an fp32 product, not measured), |sum p - 1| <= 1e-5;
    value: |dvalue| <= exact_nets.MIN_QUARTER_STEP."""
    sd, x, ref = Rn.wide_heads_case(which)
    net = om.NativeNet(sd, device=0, dtype=dtype)
    failed = []
    for n in (5, 1027):
        out = net(torch.from_numpy(np.array(x[:n])).to(DEV))
        torch.cuda.synchronize()
        d = Rn.wide_deviations(out["policy"].cpu().numpy(), out["value"].cpu().numpy(), ref.rows(n))
        numerics.record(f"resnet wide-range {which} head {dtype} rows={n}",
                        f"largest relative error of a probability {d['rel']:.2e} = {d['rel_over_bound']:.2f} of its "
                        f"bound {d['bound_at_worst']:.2e}, |sum p - 1| {d['sum_err']:.1e}, "
                        f"|dvalue| {d['value_err']:.1e} (bound {E.MIN_QUARTER_STEP:g})")
        if not (d["rel_over_bound"] <= 1.0 and d["sum_err"] <= 1e-5 and d["value_err"] <= E.MIN_QUARTER_STEP):
            failed.append(f"rows={n}: {d}")
    assert not failed, "\n".join(failed)
