"""The fused ResNet's packed-row input path (csrc/resnet.hip, IN == kPacked: the
path of every native search, self-play step, arena match and bench line),
tested at the kernel: bit-packed feature rows (tests/packed_rows.py) go through
oamd_debug_forward_packed, a thin wrapper over the launch the search uses, and
must give
  * the exact probe nets' integer reference (tests/exact_nets.py) to a quarter
    step, as tests/test_gpu_resnet_exact.py asks of the fp32-plane path, and
  * the bits of the fp32-plane path (NativeNet.__call__) on the same planes, in
    a launch of the same row count: both instantiations share everything behind
    a prologue that produces only 0 and 1.
Output buffers are longer than any launch and filled with a sentinel; every row
a launch should not write must keep it. The per-row symmetry cycles through
0..7, so every workgroup decodes boards under different transforms.

What runs only here: the prologue's decode (one 64-bit load per lane, readlane
broadcasts, inverse_transform, the fw - 1 lane clamp, 3 to 31 planes), RowMap
with an evaluation list (the device-side count, the list offset of an nn_batch
split, outputs at policy[list[i]]), the looping grids of the extra rounds, the
all-terminal early exit and invalid rows inside a live workgroup.

Which case reaches which of the 20 packed kernels (5 geometries x bf16 / fp16
x plain / _loop; every case runs both dtypes):
  k_resnet_w8<GeoS<128>>        dense 5 / 1023 rows at C=128 (a, b), the 7-row
                                list and the 512-row second half (c)
  k_resnet_w8_loop<GeoS<128>>   40-row list launches, max_wgs 1 / 3 (d, e)
  k_resnet_w4<GeoW4>            dense 1024 / 1027 rows, four-wave on (a, b),
                                1024-entry lists (c)
  k_resnet_w4_loop<GeoW4>       1024-entry lists, max_wgs 1 / 3, four-wave on (d, e)
  k_resnet_w8<Geo<128>>         dense 1024 / 1027 rows, four-wave off (a)
  k_resnet_w8_loop<Geo<128>>    1024-entry lists, max_wgs 1 / 3, four-wave off (d, e)
  k_resnet_w8<GeoS<256>>        dense 5 / 1023 rows at C=256 (a, b), the 7-row
                                list and the 512-row second half (c)
  k_resnet_w8_loop<GeoS<256>>   40-row list launches, max_wgs 1 / 3 (d, e)
  k_resnet_w8<Geo<256>>         dense 1025 / 1027 rows (a, b), 1024-entry lists (c)
  k_resnet_w8_loop<Geo<256>>    1024-entry lists, max_wgs 1 / 3 (d, e)
test_the_comparison_sees_a_wrong_decode feeds rows packed as a wrong prologue
would read them and requires both comparisons to fail at exactly that row.
The last test ties the packer to the engine: the rows a search really writes
unpack to oamd_engine_features and evaluate to the bits of the callback path.
The terminal summary lists every exact case's deviation in steps (limit 0.25).
"""

import numpy as np
import pytest
import torch

import exact_nets as E
import numerics
import packed_rows as P
import resnet_ref
from test_gpu_resnet import TOL

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = ("bf16", "fp16")
SWITCH = (True, False)  # C=128 throughput launches: 4-wave, 8-wave
SENTINEL = -7.0
EXTRA = 9  # output rows behind the last one any launch may write
N = E.MASTER_ROWS


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


def _switches(C):
    return SWITCH if C == 128 else (None,)


def _set(four_wave, v):
    if v is not None:
        four_wave(v)
    return "" if v is None else f" four_wave={v}"


# ------------------------------------------------------------------ plumbing
class Case:
    """One exact case on the device: the master planes, their packed rows
    (symmetry n mod 8 for row n) and the integer reference."""

    def __init__(self, args):
        self.args = args
        self.id = E.case_id(args)
        self.sd, self.x, self.ref = E.case(*args)
        self.C, self.cin = args[1], args[3]
        self.H = (self.cin - 1) // 2
        self.t = np.arange(N) % 8
        self.x_dev = torch.from_numpy(np.array(self.x)).to(DEV)
        self.feat = self.upload(P.pack(self.x, self.t))
        self.nets = {}

    @staticmethod
    def upload(rows):
        return torch.from_numpy(np.ascontiguousarray(rows).view(np.int64)).to(DEV)

    def net(self, om, dtype):
        if dtype not in self.nets:
            self.nets[dtype] = om.NativeNet(self.sd, device=0, dtype=dtype)
        return self.nets[dtype]

    def feat_with_invalid(self, dead_rows):
        valid = np.ones(N, bool)
        valid[dead_rows] = False
        return self.upload(P.pack(self.x, self.t, valid))


_CASES = {}


def _case(args):
    if args not in _CASES:
        while len(_CASES) >= 2:  # as exact_nets.case keeps two
            _CASES.pop(next(iter(_CASES)))
        _CASES[args] = Case(args)
    return _CASES[args]


def _launch(om, net, feat, H, rows, lst=None, count=0, off=0, max_wgs=0, out_rows=None):
    """oamd_debug_forward_packed into sentinel-filled buffers; (policy, value) as numpy."""
    out_rows = rows + EXTRA if out_rows is None else out_rows
    policy = torch.full((out_rows, 65), SENTINEL, dtype=torch.float32, device=DEV)
    value = torch.full((out_rows,), SENTINEL, dtype=torch.float32, device=DEV)
    om._othello_mcts_impl._debug_forward_packed(
        net._net, feat.data_ptr(), feat.shape[0], H, None if lst is None else [int(v) for v in lst], count, off,
        rows, max_wgs, policy.data_ptr(), value.data_ptr(), out_rows, torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    return policy.cpu().numpy(), value.cpu().numpy()


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _same(a, b):
    return _bits(a[0], b[0]) and _bits(a[1], b[1])


def _subset(ref, idx):
    return E.Reference(ref.logits[idx], ref.z[idx], ref.U, ref.fracs, ref.step, ref.step_v)


def _planes_path(net, planes):
    """The fp32-plane path (kF32) on these planes, as numpy."""
    out = net(planes)
    torch.cuda.synchronize()
    return out["policy"].cpu().numpy(), out["value"].cpu().numpy()


def _verify(case, net, got, entries, label, failed, dead=None, filled=None, exact=True):
    """got = (policy, value) of a launch whose entry i holds master row
    entries[i] (so its output row is entries[i] too), invalid where dead[i];
    only the first `filled` entries are evaluated (the device-side count).
    Live rows: the integer reference to a quarter step and the bits of the
    fp32-plane path on the launch's planes (dead boards zeroed), in a launch of
    the same row count. Dead rows: wholly sentinel, or wholly the all-zero
    board's evaluation (master row 1 in the reference). Every other row of the
    buffers, those of unfilled entries included: sentinel."""
    policy, value = got
    entries = np.asarray(entries, np.int64)
    filled = np.arange(len(entries)) < (len(entries) if filled is None else filled)
    dead = (np.zeros(len(entries), bool) if dead is None else np.asarray(dead, bool)) & filled
    live = ~dead & filled
    touched = np.zeros(len(policy), bool)
    touched[entries[filled]] = True
    if not ((policy[~touched] == SENTINEL).all() and (value[~touched] == SENTINEL).all()):
        bad = np.nonzero(~touched & ((policy != SENTINEL).any(1) | (value != SENTINEL)))[0]
        failed.append(f"{label}: rows outside the launch were written: {bad[:8].tolist()}")
    if len(entries) == 0:
        return
    planes = case.x_dev[torch.from_numpy(entries).to(DEV)]  # a copy
    if dead.any():
        planes[torch.from_numpy(dead).to(DEV)] = 0.0
    fp, fv = _planes_path(net, planes)
    le = entries[live]
    if not (_bits(policy[le], fp[live]) and _bits(value[le], fv[live])):
        n = int(((policy[le] != fp[live]).any(1) | (value[le] != fv[live])).sum())
        failed.append(f"{label}: {n} of {len(le)} live rows differ from the fp32-plane path")
    if exact and len(le):
        def report(d):
            numerics.record(f"resnet packed exact {label}",
                            f"policy {d['policy_steps']:.2e} steps (row {d['row']} action {d['action']}), "
                            f"value {d['value_steps']:.2e} steps, |sum p - 1| {d['sum_err']:.1e}")
        try:
            E.compare(policy[le], value[le], _subset(case.ref, le), label, report)
        except AssertionError as e:
            failed.append(str(e))
    written = []
    for i in np.nonzero(dead)[0]:
        r = entries[i]
        if (policy[r] == SENTINEL).all() and value[r] == SENTINEL:
            continue
        if _bits(policy[r], fp[i]) and _bits(value[r:r + 1], fv[i:i + 1]):
            written.append(r)
        else:
            failed.append(f"{label}: invalid row {r} (entry {i}) is neither untouched nor the all-zero board's")
    if exact and written:
        try:
            E.compare(policy[written], value[written], _subset(case.ref, np.full(len(written), 1)),
                      f"{label} (invalid rows, as the all-zero board)")
        except AssertionError as e:
            failed.append(str(e))


def _untouched(got):
    return bool((got[0] == SENTINEL).all() and (got[1] == SENTINEL).all())


# ------------------------------------------------------------------ (a), (b), (f) dense rows
def _dense(om, four_wave, args, small, large):
    case = _case(args)
    failed = []
    for dtype in DTYPES:
        net = case.net(om, dtype)
        for rows in small:
            label = f"{case.id} {dtype} rows={rows}"
            _verify(case, net, _launch(om, net, case.feat, case.H, rows), np.arange(rows), label, failed)
        for v in _switches(case.C):
            tag = _set(four_wave, v)
            for rows in large:
                label = f"{case.id} {dtype} rows={rows}{tag}"
                got = _launch(om, net, case.feat, case.H, rows)
                _verify(case, net, got, np.arange(rows), label, failed)
                if not _same(got, _launch(om, net, case.feat, case.H, rows)):
                    failed.append(f"{label}: two launches differ")
    assert not failed, "\n".join(failed)


INSTANTIATION_CASES = [a for a, _ in E.ROUTING + E.INTEGER]


@pytest.mark.parametrize("args", INSTANTIATION_CASES, ids=[E.case_id(a) for a in INSTANTIATION_CASES])
def test_every_instantiation_on_dense_rows(om, four_wave, args):
    """(a) The routing nets at full depth (four phases: every conv2 output
    channel carries a non-zero weight) and the integer nets: 5 and 1023 rows in
    the one-board geometry; 1024 and 1027 rows at C=128 under both settings of
    the four-wave switch, 1025 at C=256, in the throughput geometries (ragged
    last workgroups). (f) Every throughput launch is issued twice and must
    repeat its bits."""
    _dense(om, four_wave, args, (5, 1023), (1024, 1027) if args[1] == 128 else (1025,))


WIDTH_CASES = [a for a, _ in E.DEPTH if a[2] in (0, 2) and a[3] in (3, 31)]


@pytest.mark.parametrize("args", WIDTH_CASES, ids=[E.case_id(a) for a in WIDTH_CASES])
def test_input_widths(om, four_wave, args):
    """(b) History 1 (rows of 4 words: 60 lanes of the row load clamp to word
    3) and 15 (all 32 words, 31 planes and the always-zero 32nd channel), with
    no residual block and with two, at 5 and 1027 rows."""
    _dense(om, four_wave, args, (5,), (1027,))


# ------------------------------------------------------------------ (c), (d), (e) lists
LIST_CASES = [("A", 128, 9, 17, 64, 0), ("A", 256, 19, 17, 64, 0)]
LIST_IDS = [E.case_id(a) for a in LIST_CASES]
SKIPPED = (0, 513, 1026)  # master rows the list leaves out


def _permuted_list():
    """1024 of the 1027 master rows in a seeded order."""
    from othello_mcts.synthetic import portable_uniform

    keep = np.array([r for r in range(N) if r not in SKIPPED])
    lst = keep[np.argsort(portable_uniform(20261021, 1, len(keep)), kind="stable")]
    assert len(lst) == 1024 and len(set(lst.tolist())) == 1024 and not np.array_equal(lst, np.sort(lst))
    return lst


@pytest.mark.parametrize("args", LIST_CASES, ids=LIST_IDS)
def test_evaluation_lists(om, args):
    """(c) The launch as enqueue_group_nn issues it: a permuted list that skips
    rows, the device-side count equal to, three short of and at or below the
    list offset, the second launch of an nn_batch split (list_off = 512, rows =
    512), and a 7-entry list through the one-board geometry. Outputs land at
    policy[list[i]] and nowhere else."""
    case = _case(args)
    lst = _permuted_list()
    failed = []
    for dtype in DTYPES:
        net = case.net(om, dtype)

        def run(label, entries, filled=None, **kw):
            got = _launch(om, net, case.feat, case.H, out_rows=N + EXTRA, **kw)
            _verify(case, net, got, entries, f"{case.id} {dtype} {label}", failed, filled=filled)

        run("list full", lst, rows=1024, lst=lst, count=1024)
        run("list count-3", lst, filled=1021, rows=1024, lst=lst, count=1021)
        run("list second half", lst[512:], rows=512, lst=lst, count=1024, off=512)
        run("list second half count-3", lst[512:], filled=509, rows=512, lst=lst, count=1021, off=512)
        seven = lst[[1000, 3, 512, 7, 77, 1023, 0]]
        run("list of 7", seven, rows=7, lst=seven, count=7)
        for count, off, rows in ((0, 0, 1024), (512, 512, 512), (100, 512, 512), (0, 0, 7)):
            got = _launch(om, net, case.feat, case.H, rows, lst=lst, count=count, off=off, out_rows=N + EXTRA)
            if not _untouched(got):
                failed.append(f"{case.id} {dtype} count={count} list_off={off} rows={rows}: something was written")
    assert not failed, "\n".join(failed)


@pytest.mark.parametrize("args", LIST_CASES, ids=LIST_IDS)
def test_looping_grids(om, four_wave, args):
    """(d) The extra rounds' grids over the permuted list: one workgroup that
    takes every board group in turn, three (no divisor of the 256 / 512 / 40
    groups), and grids at and above the group count (the plain kernel), at
    1024 entries (throughput geometries, at C=128 both of them) and at 40
    (one-board geometry). All must give the bits of the regular grid, which is
    checked against the reference."""
    case = _case(args)
    lst = _permuted_list()
    failed = []
    for dtype in DTYPES:
        net = case.net(om, dtype)
        for rows in (1024, 40):
            groups = rows // (E.BOARDS_PER_WG[case.C] if rows >= 1024 else 1)
            for v in _switches(case.C) if rows >= 1024 else (None,):
                label = f"{case.id} {dtype} list rows={rows}{_set(four_wave, v)}"
                kw = dict(rows=rows, lst=lst[:rows], count=rows, out_rows=N + EXTRA)
                base = _launch(om, net, case.feat, case.H, **kw)
                _verify(case, net, base, lst[:rows], label, failed)
                for wgs in (1, 3, groups, groups + 5):
                    if not _same(base, _launch(om, net, case.feat, case.H, max_wgs=wgs, **kw)):
                        failed.append(f"{label}: max_wgs={wgs} differs from the regular grid")
    assert not failed, "\n".join(failed)


def _dead_entries(rows, boards):
    """Invalid launch entries by board group (group g = entries g*boards ..):
    group 1 wholly dead between live groups 0 and 2 (with one workgroup, a
    dead group directly followed by a live one), groups 3 and 4 with one live
    board (the first / the last), groups 5 and 6 dead in a row, the group
    before the last with one live board, the last group dead."""
    groups = rows // boards
    dead = np.zeros((groups, boards), bool)
    dead[[1, 5, 6, groups - 1]] = True
    dead[3, 1:] = True
    dead[4, :-1] = True
    dead[groups - 2, :-1] = True
    return dead.reshape(-1)


@pytest.mark.parametrize("args", LIST_CASES, ids=LIST_IDS)
def test_invalid_rows(om, four_wave, args):
    """(e) Terminal leaves: whole board groups dead, groups with one live
    board, a dead group followed by a live one in the same looping workgroup,
    the last group dead; under the regular grid, one workgroup and three. A
    launch whose rows are all invalid writes nothing."""
    case = _case(args)
    lst = _permuted_list()
    failed = []
    for rows in (1024, 40):
        boards = E.BOARDS_PER_WG[case.C] if rows >= 1024 else 1
        dead = _dead_entries(rows, boards)
        assert dead[boards:2 * boards].all() and not dead[:boards].any() and not dead[2 * boards:3 * boards].any()
        assert dead[-boards:].all() and (boards == 1 or dead[3 * boards:5 * boards].sum() == 2 * (boards - 1))
        feat = case.feat_with_invalid(lst[:rows][dead])
        none = case.feat_with_invalid(np.arange(N))
        for dtype in DTYPES:
            net = case.net(om, dtype)
            for v in _switches(case.C) if rows >= 1024 else (None,):
                tag = _set(four_wave, v)
                kw = dict(rows=rows, lst=lst[:rows], count=rows, out_rows=N + EXTRA)
                for wgs in (0, 1, 3):
                    label = f"{case.id} {dtype} invalid rows={rows} max_wgs={wgs}{tag}"
                    _verify(case, net, _launch(om, net, feat, case.H, max_wgs=wgs, **kw), lst[:rows], label,
                            failed, dead=dead)
                for wgs in (0, 1):
                    if not _untouched(_launch(om, net, none, case.H, max_wgs=wgs, **kw)):
                        failed.append(f"{case.id} {dtype} all invalid rows={rows} max_wgs={wgs}{tag}: rows written")
    assert not failed, "\n".join(failed)


def test_the_comparison_sees_a_wrong_decode(om):
    """The test of the tests, on the device: rows packed as a wrong prologue
    would read them (tests/test_cpu_packed_rows.py's three mutations, each on
    one row of an 8-row launch) fail both comparisons at that row."""
    case = _case(LIST_CASES[0])
    net = case.net(om, "bf16")
    good = P.pack(case.x[:8], case.t[:8])
    wrong_t = good.copy()
    wrong_t[5, 0] = P.meta(case.x[5, 0, 0, 0], (case.t[5] + 3) % 8)
    swapped = good.copy()
    swapped[6, [6, 7]] = good[6, [7, 6]]
    shifted = good.copy()
    shifted[7, 2:-2], shifted[7, -2:] = good[7, 4:], 0
    for name, rows, row in (("symmetry", wrong_t, 5), ("planes", swapped, 6), ("history", shifted, 7)):
        got = _launch(om, net, Case.upload(rows), case.H, 8)
        failed = []
        _verify(case, net, got, np.arange(8), f"mutated {name} (must fail)", failed)
        assert any("fp32-plane path" in f for f in failed) and any("steps" in f for f in failed), (name, failed)
        keep = np.arange(8) != row  # and only there
        ok = _launch(om, net, case.feat, case.H, 8)
        assert _bits(got[0][:8][keep], ok[0][:8][keep]) and not _bits(got[0][row], ok[0][row]), name
    failed = []
    _verify(case, net, _launch(om, net, Case.upload(good), case.H, 8), np.arange(8), f"{case.id} bf16 rows=8", failed)
    assert not failed, failed


def test_entry_refuses_what_would_leave_the_buffers(om):
    """oamd_debug_forward_packed launches nothing unless every row it could
    read or write lies inside both buffers."""
    case = _case(LIST_CASES[0])
    net = case.net(om, "bf16")
    ok = dict(rows=8, lst=list(range(8)), count=8, off=0, out_rows=N)

    def refused(**kw):
        a = {**ok, **kw}
        with pytest.raises(ValueError):
            _launch(om, net, a.pop("feat", case.feat), a.pop("H", case.H), **a)

    refused(lst=[0, 1, 2, 3, 4, 5, 6, N])        # an entry past the features
    refused(lst=[0, 1, 2, 3, 4, 5, 6, 20], out_rows=20)  # ... past the outputs
    refused(lst=[0, 1, 2, -1, 4, 5, 6, 7])
    refused(off=1)                                # list_off + rows > list_len
    refused(rows=9)
    refused(rows=-1)
    refused(count=-1)
    refused(max_wgs=-1)
    refused(off=-1, rows=4)
    refused(H=7)                                  # not the net's history
    refused(H=0)
    refused(H=16)
    refused(lst=None, rows=N + 1, out_rows=N + EXTRA)  # dense rows past the features
    refused(lst=None, rows=30, out_rows=20)
    refused(lst=None, off=1)
    got = _launch(om, net, case.feat, case.H, **ok)
    assert not _untouched(got) and (got[0][8:] == SENTINEL).all()


# ------------------------------------------------------------------ a live net
# TOL is absolute and was set on the reference's golden nets (test_gpu_resnet.py:
# "for the torch-default-init goldens"); the 16-bit tower's value error grows
# with the net's value spread (about an eighth of its standard deviation at
# bf16, whichever the seed), so another seed of the same family can sit on
# either side of it. The nets here are therefore the 1027- and 1025-board
# goldens' own (tests/golden/resnet_large_meta.json), the ones the suite already
# holds to TOL at this batch size.
LIVE_NETS = {128: "c128b9_h8_r1027", 256: "c256b19_h8_r1025"}


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C", sorted(LIVE_NETS))
def test_live_net_packed_equals_planes(om, golden_dir, C, dtype):
    """Dense random weights (every plane bit matters) on the 1027 master rows:
    the packed path gives the bits of the fp32-plane path and stays within the
    tolerances tests/test_gpu_resnet.py sets for these nets against the fp32
    restatement."""
    import json

    from othello_mcts.synthetic import alphazero_state_dict

    meta = json.loads((golden_dir / "resnet_large_meta.json").read_text())[LIVE_NETS[C]]
    assert meta["conv_channels"] == C and meta["history_size"] == 8
    sd = alphazero_state_dict(meta["seed"], 17, C, meta["num_residual_blocks"], meta["value_head_hidden_channels"])
    net = om.NativeNet(sd, device=0, dtype=dtype)
    x = E.inputs(17)
    x_dev = torch.from_numpy(np.array(x)).to(DEV)
    feat = Case.upload(P.pack(x, np.arange(N) % 8))
    policy, value = _launch(om, net, feat, 8, N)
    assert (policy[N:] == SENTINEL).all() and (value[N:] == SENTINEL).all()
    fp, fv = _planes_path(net, x_dev)
    assert _bits(policy[:N], fp) and _bits(value[:N], fv)
    ref = resnet_ref.forward(sd, x_dev)
    dp = np.abs(policy[:N] - ref["policy"].cpu().numpy()).max()
    dv = np.abs(value[:N] - ref["value"].cpu().numpy()).max()
    numerics.record(f"resnet packed live {LIVE_NETS[C]} {dtype}", f"max|dpolicy|={dp:.2e} max|dvalue|={dv:.2e}")
    tp, tv = TOL[dtype]
    assert np.isfinite(policy[:N]).all() and dp <= tp and dv <= tv


# ------------------------------------------------------------------ the engine's own rows
ENGINE_SEEDS = {4: (8, 9), 15: (8, 9)}  # history -> (engine seed, openings seed)
ENGINE_MOVES = 6


@pytest.mark.parametrize("H", [4, 15])
def test_engine_rows_unpack_and_evaluate_as_the_callback_path(om, H):
    """36 games x 2 threads x 16 leaves = 1152 rows per round (the throughput
    geometry), 64 simulations = two rounds of the step API per search, from
    openings of up to 58 plies, a C=128 NativeNet as the callback evaluator.
    Both rounds of a search from a fresh root hold leaves at depth <= 1, which
    are terminal only after a double pass, so the run is six searches with a
    self-play move after each: the reused trees put leaves behind the games'
    last moves. At each round the engine's packed rows unpack to
    oamd_engine_features exactly; where a thread waits for the NN their valid
    bits are oamd_engine_leaf_flags; and the packed launch on them, dense,
    gives the flagged rows the bits of net(features()). A terminal row of a
    waiting thread is untouched or the all-zero board's evaluation. A thread
    waits for the NN this round exactly when one of its 16 rows is flagged
    (k_leaf_flags: flag = pending and valid; a thread whose batch was all
    terminal backed it up at once and is not pending); the rows of the other
    threads are stale and excluded."""
    from othello_mcts.synthetic import alphazero_state_dict

    G, T, B = 36, 2, 16
    rows, C = G * T * B, 1 + 2 * H
    net = om.NativeNet(alphazero_state_dict(43 + H, C, 128, 2, 32), device=0)
    seed, opening_seed = ENGINE_SEEDS[H]
    b = om.BatchedMCTS(G, history_size=H, num_simulations=64, num_threads=T, batch_size=B, dirichlet_epsilon=0.25,
                       seed=seed, node_capacity=1 << 16)
    assert b.rows_per_step == rows
    b.random_openings(58, seed=opening_seed)
    e = b.engine
    impl = om._othello_mcts_impl
    feat = torch.empty((rows, C, 8, 8), dtype=torch.float32, device=DEV)
    packed = torch.zeros((rows, P.feature_words(H)), dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError):
        impl._debug_engine_feature_rows(e, packed.data_ptr(), packed.numel() - 1)
    live_transforms, terminal_rows, live_rows = set(), 0, 0
    for move in range(ENGINE_MOVES):
        b._stream()
        steps = e.search_begin()
        assert steps == 2
        for step in range(steps):
            at = (move, step)
            e.select()
            e.features(feat.data_ptr(), 0, rows)
            impl._debug_engine_feature_rows(e, packed.data_ptr(), packed.numel())
            flags = e.leaf_flags().astype(bool)
            torch.cuda.synchronize()
            words = packed.cpu().numpy().view(np.uint64)
            planes = feat.cpu().numpy()
            assert (words[:, 1] == 0).all(), at
            np.testing.assert_array_equal(P.unpack(words, H), planes, err_msg=f"move, round {at}")
            waiting = np.repeat(flags.reshape(G * T, B).any(1), B)
            valid = P.valid_bits(words)
            assert np.array_equal(valid[waiting], flags[waiting]), at
            out = net(feat)
            policy, value = _launch(om, net, packed, H, rows)
            fp, fv = out["policy"].cpu().numpy(), out["value"].cpu().numpy()
            assert (policy[rows:] == SENTINEL).all() and (value[rows:] == SENTINEL).all(), at
            assert _bits(policy[:rows][flags], fp[flags]) and _bits(value[:rows][flags], fv[flags]), at
            terminal = waiting & ~valid
            for r in np.nonzero(terminal)[0]:
                assert (planes[r] == 0).all(), (at, r)
                untouched = (policy[r] == SENTINEL).all() and value[r] == SENTINEL
                assert untouched or (_bits(policy[r], fp[r]) and _bits(value[r:r + 1], fv[r:r + 1])), (at, r)
            live_transforms |= set(P.transforms(words)[flags].tolist())
            terminal_rows += int(terminal.sum())
            live_rows += int(flags.sum())
            e.set_evaluation(out["policy"].data_ptr(), out["value"].data_ptr(), 0, rows)
        e.backup()
        e.check_health()
        b.selfplay_move(temperature_moves=12, opening_moves=58)
    numerics.record(f"resnet packed engine rows H={H}",
                    f"live rows {live_rows}, terminal rows of waiting threads {terminal_rows}, "
                    f"transforms {sorted(live_transforms)}")
    assert terminal_rows >= 1 and live_rows >= 1 and live_transforms == set(range(8))
