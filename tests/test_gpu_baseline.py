"""The baseline opponents on the device (csrc/baseline.hip k_baseline /
k_baseline_pick through othello_mcts.baseline_moves) against the fixture
tests/golden/baseline.npz (the independent Python reference) and against the
host twin: scores, picks, flags and node counts, on several batch sizes and on
a one-workgroup grid."""

import functools

import numpy as np
import pytest
import torch

import baseline_ref as R
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NONE = -(1 << 31)
SENTINEL = 0x5A5A5A5
N_CASES = 8


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(ROOT / "tests" / "golden" / "baseline.npz")
    return {k: z[k] for k in z.files}


def case(c):
    """(kind, depth, indices of the positions the case holds)."""
    f = fixture()
    idx = np.nonzero(f["group"] == 3)[0] if f["case_late_only"][c] else np.arange(len(f["player"]))
    return int(f["case_kind"][c]), max(1, int(f["case_depth"][c])), idx


def triples(idx):
    f = fixture()
    return [(int(f["player"][i]), int(f["p1"][i]), int(f["p2"][i])) for i in idx]


@functools.lru_cache(maxsize=None)
def host(c):
    """The host twin's outputs of every position of case c (computed once, not modified)."""
    import othello_mcts as om

    kind, depth, idx = case(c)
    return [om.baseline_move(t, kind, depth) for t in triples(idx)]


@functools.lru_cache(maxsize=None)
def device_positions():
    from othello_mcts.endgame import pack_positions

    return pack_positions(triples(range(len(fixture()["player"])))).to(DEV)


@pytest.mark.parametrize("c", range(N_CASES))
def test_device_equals_fixture_and_host(c):
    import othello_mcts as om

    f = fixture()
    kind, depth, idx = case(c)
    want = host(c)
    assert [w["move_scores"] for w in want] == f["move_scores"][c, idx].tolist()
    pos = device_positions()[torch.from_numpy(idx).to(DEV)]
    sizes = sorted({1, min(63, len(idx)), min(64, len(idx)), min(65, len(idx)), len(idx)})
    for n in sizes:
        for wg in (1, 0):
            out = om.baseline_moves(pos[:n], kind, depth, _workgroups=wg)
            assert out.move_scores.shape == (n, 65) and out.move_scores.dtype == torch.int32
            assert out.nodes.dtype == torch.int64
            assert out.move_scores.cpu().tolist() == f["move_scores"][c, idx[:n]].tolist(), (n, wg)
            assert out.action.cpu().tolist() == f["action"][c, idx[:n]].tolist(), (n, wg)
            assert out.score.cpu().tolist() == [w["score"] for w in want[:n]]
            assert out.flags.cpu().tolist() == [w["flags"] for w in want[:n]] == [0] * n
            assert out.nodes.cpu().tolist() == [w["nodes"] for w in want[:n]], (n, wg)
    # the same from a sequence of positions
    out = om.baseline_moves(triples(idx[:3]), kind, depth)
    assert out.action.cpu().tolist() == f["action"][c, idx[:3]].tolist()
    assert om.baseline_moves(pos[:0], kind, depth).action.shape == (0,)


def test_mixed_batch_writes_exactly_its_own_rows():
    import othello_mcts as om
    from othello_mcts._othello_mcts_impl import _baseline_workspace_bytes, _gpu_baseline
    from othello_mcts.endgame import pack_positions

    f = fixture()
    full = (1 << 64) - 1
    root_pass = next(i for i in range(len(f["player"])) if f["move_scores"][0, i, 64] == 0)
    ordinary = triples([0, 40, 70, 100])
    over = (1, full - 0xFF, 0xF0)  # nobody can move
    batch = [ordinary[0], over, (1, ordinary[1][1] | 1, ordinary[1][2] | 1), triples([root_pass])[0], ordinary[1],
             (3, *ordinary[2][1:]), (0, *ordinary[2][1:]), (2, *over[1:]), ordinary[2], ordinary[3]]
    flagged = [2, 5, 6]
    terminal = [1, 7]
    n = len(batch)
    pos = pack_positions(batch).to(DEV)
    for kind, depth, limit in ((om.baseline.GREEDY, 1, 1 << 24), (om.baseline.SEARCH, 3, 1 << 24),
                               (om.baseline.SEARCH, 4, 200)):
        want = [om.baseline_move(t, kind, depth, node_limit=limit) for t in batch]
        if limit == 200:  # binds for some positions, not for others
            assert sum(w["flags"] == om.baseline.FLAG_NODE_LIMIT for w in want) >= 2
            assert sum(w["flags"] == 0 and w["action"] >= 0 for w in want) >= 2
        # one guard row before and after every output
        ms = torch.full((n + 2, 65), SENTINEL, dtype=torch.int32, device=DEV)
        score, action, flags = (torch.full((n + 2,), SENTINEL, dtype=torch.int32, device=DEV) for _ in range(3))
        nodes = torch.full((n + 2,), SENTINEL, dtype=torch.int64, device=DEV)
        ws = torch.empty((_baseline_workspace_bytes(n),), dtype=torch.uint8, device=DEV)
        _gpu_baseline(0, pos.data_ptr(), n, kind, depth, limit, 0, 0, ms[1:].data_ptr(), score[1:].data_ptr(),
                      action[1:].data_ptr(), flags[1:].data_ptr(), nodes[1:].data_ptr(), ws.data_ptr(), 0,
                      torch.cuda.current_stream(DEV).cuda_stream)
        torch.cuda.synchronize()
        for t in (ms, score, action, flags, nodes):
            assert (t[0] == SENTINEL).all() and (t[-1] == SENTINEL).all()
        assert ms[1:-1].cpu().tolist() == [w["move_scores"] for w in want]
        assert score[1:-1].cpu().tolist() == [w["score"] for w in want]
        assert action[1:-1].cpu().tolist() == [w["action"] for w in want]
        assert flags[1:-1].cpu().tolist() == [w["flags"] for w in want]
        assert nodes[1:-1].cpu().tolist() == [w["nodes"] for w in want]
        for i in range(n):
            if i in flagged or i in terminal or want[i]["flags"]:
                assert want[i]["move_scores"] == [NONE] * 65 and want[i]["score"] == NONE and want[i]["action"] == -1
                assert (want[i]["flags"] != 0) == (i not in terminal)
            else:
                assert want[i]["action"] >= 0
        assert [want[i]["flags"] for i in flagged] == [om.baseline.FLAG_INVALID] * 3
        assert want[3]["action"] == 64


@pytest.mark.parametrize("c", range(N_CASES))
def test_keyed_device_pick_equals_the_host_pick(c):
    """Eight events per case. The host search is repeated with the key only
    where two or more actions tie; elsewhere the pick cannot depend on the key
    and must be the fixture's action."""
    import othello_mcts as om

    f = fixture()
    kind, depth, idx = case(c)
    pos = device_positions()[torch.from_numpy(idx).to(DEV)]
    keys = [(0x9E3779B97F4A7C15 * (int(i) + 1) + c) & ((1 << 63) - 1) for i in idx]
    keys_dev = torch.tensor(keys, dtype=torch.int64, device=DEV)
    tied = [len(R.ties(f["move_scores"][c, i].tolist())) >= 2 for i in idx]
    assert any(tied) or kind == om.baseline.SEARCH
    for ev in range(8):
        events = torch.full((len(idx),), ev, dtype=torch.int64, device=DEV) + torch.arange(len(idx), device=DEV) % 3
        out = om.baseline_moves(pos, kind, depth, keys=keys_dev, events=events)
        got = out.action.cpu().tolist()
        assert out.move_scores.cpu().tolist() == f["move_scores"][c, idx].tolist()
        for j, i in enumerate(idx):
            if tied[j]:
                want = om.baseline_move(triples([i])[0], kind, depth, key=keys[j], event=ev + j % 3)["action"]
            else:
                want = int(f["action"][c, i])
            assert got[j] == want, (ev, j)
    # keys without events: event 0
    out = om.baseline_moves(pos, kind, depth, keys=keys_dev)
    zero = om.baseline_moves(pos, kind, depth, keys=keys_dev, events=torch.zeros_like(keys_dev))
    assert torch.equal(out.action, zero.action)
    with pytest.raises(ValueError):
        om.baseline_moves(pos, kind, depth, events=torch.zeros_like(keys_dev))
    with pytest.raises(ValueError):
        om.baseline_moves(pos, kind, depth, keys=keys_dev[:-1])
    with pytest.raises(ValueError):
        om.baseline_moves(pos, kind, depth, keys=keys_dev.cpu())
