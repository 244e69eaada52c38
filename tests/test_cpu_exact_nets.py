"""The exact-arithmetic probe nets (tests/exact_nets.py) on the CPU: the integer
reference agrees with the fp32 torch restatement, every net and batch that
tests/test_gpu_resnet_exact.py runs meets the exactness conditions, and the
comparison rejects every mutation that names a bug class the GPU tests are
meant to catch (reference(mutated net) against reference(net), on the very
inputs of the GPU tests)."""

import numpy as np
import pytest
import torch

import exact_nets as E
import resnet_ref


# ------------------------------------------------------------------ reference link
@pytest.mark.parametrize("args", [("A", 128, 2, 17, 64, 1), ("A", 256, 2, 17, 33, 0),
                                  ("B", 128, 2, 17, 64, 0), ("B", 256, 2, 17, 100, 0)], ids=E.case_id)
def test_forward_exact_matches_fp32_restatement(args):
    sd, x, ref = E.case(*args)
    n = 24
    got = E.forward_exact(sd, x[:n])
    assert np.array_equal(got.logits, ref.logits[:n]) and np.array_equal(got.z, ref.z[:n])  # prefix = own batch
    out = resnet_ref.forward(sd, torch.from_numpy(np.array(x[:n])))
    p, v = E.outputs_of(got)
    dp = np.abs(out["policy"].numpy() - p).max()
    dv = np.abs(out["value"].numpy() - v).max()
    assert dp <= 1e-5 and dv <= 1e-5, (dp, dv)


# ------------------------------------------------------------------ conditions
@pytest.mark.parametrize("args,rows", E.ALL_CASES, ids=[E.case_id(a) for a, _ in E.ALL_CASES])
def test_conditions_of_every_gpu_case(args, rows):
    """E.case asserts, for both 16-bit formats, that every conv folds to the
    intended integers, U <= 256 and the heads' 2^24 bound over the master
    batch, of which every GPU batch is a prefix."""
    sd, x, ref = E.case(*args)
    assert max(rows) <= len(x) and ref.U <= E.U_MAX
    E.check_scales(ref)
    assert all(0.1 <= f <= 0.9 for f in ref.fracs), ref.fracs
    assert (x[1] == 0).all() and (x[2] == 1).all() and np.isin(x, (0.0, 1.0)).all()
    # every tap of every conv layer carries weights
    for pc, pn in E.conv_layers(sd):
        w, _ = E.fold(sd, pc, pn)
        assert (np.abs(w).sum(axis=(0, 1)) > 0).all(), pc
    # the heads' outputs move: no degenerate net
    assert ref.z.std() > 0.1 and ref.logits.std(axis=0).min() > 0


@pytest.mark.parametrize("C,R", [(128, 9), (256, 19)])
def test_routing_phases_cover_every_conv2_channel(C, R):
    live = np.zeros((R, C), bool)
    for phase in range(4):
        sd = E.routing_tower(C, R, 17, phase)
        for l in range(R):
            w = sd[f"residual_blocks.{l}.conv2.weight"]
            assert ((w != 0).sum(axis=(1, 2, 3)) <= 1).all()
            live[l] |= (w != 0).any(axis=(1, 2, 3))
            src = np.abs(sd[f"residual_blocks.{l}.conv1.weight"]).sum(axis=(2, 3)).argmax(1)
            assert sorted(src) == list(range(C))  # a permutation of the channels
    assert live.all()


def test_fold_restates_the_naive_identity_trap():
    """gamma 1 / var 1 folds to 0.999995: the builders' var = float32(1 - 1e-5)
    is what makes the fold exact."""
    sd = E.routing_tower(128, 1, 17, 0)
    bad = dict(sd)
    bad["conv_block.norm.running_var"] = np.ones(128, np.float32)
    w, _ = E.fold(bad, "conv_block.conv", "conv_block.norm")
    assert not np.array_equal(w, np.rint(w))
    with pytest.raises(AssertionError):
        E.tower_exact(bad, E.inputs(17)[:2])


# ------------------------------------------------------------------ the tests have teeth
def _swap(a, i, j, axis=0):
    a = np.array(a, copy=True)
    idx = [slice(None)] * a.ndim
    ii, jj = list(idx), list(idx)
    ii[axis], jj[axis] = i, j
    a[tuple(ii)], a[tuple(jj)] = a[tuple(jj)].copy(), a[tuple(ii)].copy()
    return a


def _zero_tap(pc, ky, kx):
    def f(sd):
        w = np.array(sd[pc + ".weight"], copy=True)
        w[:, :, ky, kx] = 0
        sd[pc + ".weight"] = w
    return f


def _map_weight(pc, g):
    def f(sd):
        sd[pc + ".weight"] = np.ascontiguousarray(g(sd[pc + ".weight"]))
    return f


def _mutations(sd, C):
    """name -> (state dict edit or None, forward_exact keywords, output edit or None)"""
    layers = E.conv_layers(sd)
    m = len(layers) // 2 + (len(layers) // 2) % 2  # a block's second conv: every output channel is read on
    first, mid, last = layers[0], layers[m], layers[-1]
    muts = {}
    for where, (pc, _) in (("first", first), ("middle", mid), ("last", last)):
        muts[f"zero tap dy=-1 of the {where} conv"] = (_zero_tap(pc, 0, 1), {}, None)
        muts[f"zero tap dx=+1 of the {where} conv"] = (_zero_tap(pc, 1, 2), {}, None)
    pc, pn = mid
    muts["exchange dy and dx"] = (_map_weight(pc, lambda w: w.transpose(0, 1, 3, 2)), {}, None)
    muts["mirror taps left to right"] = (_map_weight(pc, lambda w: w[:, :, :, ::-1]), {}, None)
    for d in (1, 4, 8, 16, 32):
        for where, layer, c in (("first", 0, 7), ("middle", m, 40), ("last", len(layers) - 1, C - 33)):
            muts[f"swap output channels {c} and {c + d} of the {where} conv"] = (
                None, {"swap_out": (layer, c, c + d)}, None)

    def chunks(w):
        w = np.array(w, copy=True)
        w[:, 8:16], w[:, 16:24] = w[:, 16:24].copy(), w[:, 8:16].copy()
        return w
    muts["swap input-channel chunks 8-15 and 16-23"] = (_map_weight(pc, chunks), {}, None)
    muts["drop the skip of one block"] = (None, {"drop_skip": (m - 2) // 2}, None)

    def rows(i, j):
        return lambda p, v: (_swap(p, i, j), _swap(v, i, j))
    muts["exchange the outputs of rows 0 and 1"] = (None, {}, rows(0, 1))
    muts["exchange the outputs of rows 0 and boards-per-workgroup"] = (None, {}, rows(0, E.BOARDS_PER_WG[C]))
    muts["swap two squares of policy_head.linear's input"] = (
        lambda sd: sd.__setitem__("policy_head.linear.weight",
                                  _swap(sd["policy_head.linear.weight"], 64 + 9, 64 + 10, 1)), {}, None)
    muts["swap the last two value hidden units"] = (
        lambda sd: sd.__setitem__("value_head.linear2.weight", _swap(sd["value_head.linear2.weight"], -1, -2, 1)),
        {}, None)
    return muts


def _assert_flagged(sd, x, ref, muts):
    p0, v0 = E.outputs_of(ref)
    d = E.compare(p0, v0, ref, "unmutated")  # the comparison passes what it should
    assert d["policy_steps"] < 0.05 and d["value_steps"] < 0.05  # float32 outputs
    missed = []
    for name, (edit, kw, post) in muts.items():
        msd = dict(sd)
        if edit is not None:
            edit(msd)
        p, v = E.outputs_of(E.forward_exact(msd, x, **kw)) if (edit is not None or kw) else (p0, v0)
        if post is not None:
            p, v = post(p, v)
        try:
            E.compare(p, v, ref, name)
        except AssertionError:
            continue
        missed.append(name)
    assert not missed, f"mutations the comparison does not flag: {missed}"


@pytest.mark.parametrize("args,rows", [E.ROUTING[0], E.ROUTING[4]], ids=["c128b9", "c256b19"])
def test_comparison_rejects_every_mutation(args, rows):
    """On the small batch of the GPU tests (5 / 3 rows; the large batch holds
    it as its first rows, so what is flagged here is flagged there)."""
    sd, x, ref = E.case(*args)
    n = min(rows)
    assert n > E.BOARDS_PER_WG[args[1]]
    _assert_flagged(sd, x[:n], ref.rows(n), _mutations(sd, args[1]))


@pytest.mark.parametrize("args,rows", E.INTEGER, ids=["c128", "c256"])
def test_integer_nets_notice_a_lost_or_doubled_kstep(args, rows):
    """Family B: one K-step (one tap x 32 input channels) never counted
    (weights zeroed) or counted twice (weights doubled), in the first tower
    conv and the last; a wrong folded bias; on the 7-row batch."""
    sd, x, ref = E.case(*args)
    layers = E.conv_layers(sd)

    def kstep(pc, factor, ky, kx, cb):
        def f(sd):
            w = np.array(sd[pc + ".weight"], copy=True)
            w[:, 32 * cb:32 * cb + 32, ky, kx] *= factor
            sd[pc + ".weight"] = w
        return f

    def bias(pn):
        def f(sd):
            b = np.array(sd[pn + ".bias"], copy=True)
            b[5] += 1
            sd[pn + ".bias"] = b
        return f
    muts = {}
    for where, (pc, pn) in (("first tower", layers[1]), ("last", layers[-1])):
        muts[f"K-step lost in the {where} conv"] = (kstep(pc, 0.0, 0, 2, 1), {}, None)
        muts[f"K-step doubled in the {where} conv"] = (kstep(pc, 2.0, 2, 0, args[1] // 32 - 1), {}, None)
        muts[f"one folded bias off by one in the {where} conv"] = (bias(pn), {}, None)
    n = min(rows)
    _assert_flagged(sd, x[:n], ref.rows(n), muts)
