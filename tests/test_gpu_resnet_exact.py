"""Zero-slack tests of the fused ResNet (csrc/resnet.hip) on exact-arithmetic
probe nets (tests/exact_nets.py): integer weights, biases and activations that
bf16 and fp16 hold exactly, heads whose fp32 sums are exact in any order. The
kernel must reproduce the integer reference's logits and value pre-activation
to a quarter of the smallest change one wrong tower unit can cause, so one
misrouted channel, tap, board, row or K-step fails the case. What the nets
prove is addressing and accumulation, not rounding behaviour: which number
is stored is pinned by tests/test_gpu_resnet_rounding.py, how large the
rounding error of a live net is stays with the tolerance tests of
tests/test_gpu_resnet.py. tests/test_cpu_exact_nets.py
asserts the exactness conditions for exactly these cases and that the
comparison rejects the bug classes named there. The terminal summary lists
every case's largest deviation in steps (the limit is 0.25)."""

import numpy as np
import pytest
import torch

import exact_nets as E
import numerics

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = ("bf16", "fp16")


@pytest.fixture(scope="module")
def om():
    import othello_mcts

    return othello_mcts


def _ids(cases):
    return [E.case_id(a) for a, _ in cases]


def _check(out, ref, label):
    torch.cuda.synchronize()

    def report(d):
        numerics.record(f"resnet exact {label}",
                        f"policy {d['policy_steps']:.2e} steps (row {d['row']} action {d['action']}), "
                        f"value {d['value_steps']:.2e} steps, |sum p - 1| {d['sum_err']:.1e}")
    E.compare(out["policy"].cpu().numpy(), out["value"].cpu().numpy(), ref, label, report)


def _run(om, args, rows, twice=False):
    """One NativeNet per dtype, used for every row count of the case. twice:
    the >= 1024-row launch is issued again and must give the same bits."""
    sd, x, ref = E.case(*args)
    failed = []  # every dtype and row count runs: the report names all that fail
    for dtype in DTYPES:
        net = om.NativeNet(sd, device=0, dtype=dtype)
        for n in rows:
            xs = torch.from_numpy(np.array(x[:n])).to(DEV)
            out = net(xs)
            try:
                _check(out, ref.rows(n), f"{E.case_id(args)} {dtype} rows={n}")
            except AssertionError as e:
                failed.append(str(e))
            if twice and n >= 1024:
                again = net(xs)
                torch.cuda.synchronize()
                if not (torch.equal(out["policy"], again["policy"]) and torch.equal(out["value"], again["value"])):
                    failed.append(f"{E.case_id(args)} {dtype} rows={n}: two launches differ")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("args,rows", E.ROUTING, ids=_ids(E.ROUTING))
def test_routing_nets(om, args, rows):
    """Family A at full depth in both geometries: C=128 / 9 blocks (LDS weight
    ring, barrier-free epilogue) at 5 and 1027 rows, C=256 / 19 blocks (the
    register queue across 39 convs) at 3 and 1025; the four phases together
    give every conv2 output channel a non-zero weight. Determinism: the large
    batch is launched twice and the outputs must be bit-identical (the exact
    comparison leaves no room for an intermittent error; this pins which kind
    a failure was)."""
    _run(om, args, rows, twice=True)


@pytest.mark.parametrize("args,rows", E.GEOMETRY, ids=_ids(E.GEOMETRY))
def test_geometry_switch_and_tiny_batches(om, args, rows):
    """1, 2, 4, 7 rows, and 1023 / 1024 on either side of kSmallBatchRows."""
    _run(om, args, rows)


@pytest.mark.parametrize("args,rows", E.DEPTH, ids=_ids(E.DEPTH))
def test_depth_and_input_width(om, args, rows):
    """0, 1 and 2 residual blocks (with none, the first conv's epilogue is the
    tower's last: no next bias, the weight stream runs on into the zero pad
    and the heads take the drained ring as scratch, as after any last layer)
    on 1, 3 and 31 input planes."""
    _run(om, args, rows)


@pytest.mark.parametrize("args,rows", E.HEADS, ids=_ids(E.HEADS))
def test_value_head_hidden_sizes(om, args, rows):
    """Hidden sizes off the 64-unit slices of the k-split value head (1, 33,
    65, 100: the clamped read), one full slice, and the maximum 1024, with 1
    board per workgroup and with 4 (C=128) / 2 (C=256)."""
    _run(om, args, rows)


@pytest.mark.parametrize("args,rows", E.INTEGER, ids=_ids(E.INTEGER))
def test_integer_nets(om, args, rows):
    """Family B: many K entries per output, biases, BatchNorms that fold
    exactly with gamma 2 and 1/2, var 4, non-zero mean and conv bias."""
    _run(om, args, rows)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("args", [a for a, _ in E.GEOMETRY], ids=_ids(E.GEOMETRY))
def test_nothing_written_past_the_batch(om, args, dtype):
    """Output buffers longer than the batch, filled with a sentinel: the rows
    past `rows` stay untouched (ragged last workgroups at 1, 5, 1025, 1027)."""
    sd, x, ref = E.case(*args)
    net = om.NativeNet(sd, device=0, dtype=dtype)
    extra, sentinel = 9, -7.0
    for n in (1, 5, 1025, 1027):
        xs = torch.from_numpy(np.array(x[:n])).to(DEV)
        policy = torch.full((n + extra, 65), sentinel, dtype=torch.float32, device=DEV)
        value = torch.full((n + extra,), sentinel, dtype=torch.float32, device=DEV)
        net._net.forward(xs.data_ptr(), n, policy.data_ptr(), value.data_ptr(),
                         torch.cuda.current_stream(DEV).cuda_stream)
        torch.cuda.synchronize()
        assert (policy[n:] == sentinel).all() and (value[n:] == sentinel).all(), f"rows={n}"
        _check({"policy": policy[:n], "value": value[:n]}, ref.rows(n),
               f"{E.case_id(args)} {dtype} rows={n} (long buffers)")
