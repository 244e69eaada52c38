"""The split endgame solver on the GPU (csrc/solver.hip k_solve_plan /
k_solve_items / k_solve_split_reduce) against the fixture
tests/golden/endgames.npz, against its host twin (same source, so equal node
counts) and against the current solver.

Every device call carries a node limit of 2^24 per item or less, so a traversal
bug ends as a flag. Node totals in the docstrings were computed with the host
twin, which visits the same nodes as the device."""

import functools
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NONE = -128
LIMIT = 1 << 24
KEYS = ("move_scores", "score", "best_action", "flags", "nodes")


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(Path(__file__).parent / "golden" / "endgames.npz")
    return {k: z[k] for k in z.files}


def triples(idx=None):
    f = fixture()
    idx = range(len(f["player"])) if idx is None else idx
    return [(int(f["player"][i]), int(f["p1"][i]), int(f["p2"][i])) for i in idx]


def arrays(s):
    return {k: getattr(s, k).cpu().numpy() for k in KEYS}


@functools.lru_cache(maxsize=None)
def solved_all():
    """The whole fixture in one call on the default grid; shared, read only."""
    import othello_mcts as om

    return arrays(om.solve_endgames(triples(), 12, LIMIT, split=True))


@functools.lru_cache(maxsize=None)
def host_all():
    import othello_mcts as om

    return [om.solve_position(p, 12, LIMIT, split=True) for p in triples()]


def assert_equals_fixture(s, idx):
    f = fixture()
    idx = list(idx)
    assert np.array_equal(s["move_scores"], f["move_scores"][idx])
    assert np.array_equal(s["score"], f["score"][idx])
    assert np.array_equal(s["best_action"], f["best_action"][idx])
    assert not s["flags"].any()


def assert_equals_host(s, host):
    assert s["nodes"].tolist() == [h["nodes"] for h in host]
    assert s["move_scores"].tolist() == [h["move_scores"] for h in host]
    assert s["score"].tolist() == [h["score"] for h in host]
    assert s["best_action"].tolist() == [h["best_action"] for h in host]
    assert s["flags"].tolist() == [h["flags"] for h in host]


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_device_equals_fixture_small_batches(n):
    """The n deepest positions of the fixture (12 empties first). 65
    positions: 3,454,631 nodes."""
    import othello_mcts as om

    f = fixture()
    idx = np.argsort(-f["empties"], kind="stable")[:n].tolist()
    s = om.solve_endgames(triples(idx), 12, LIMIT, split=True)
    s.check()
    assert_equals_fixture(arrays(s), idx)


def test_device_equals_fixture_and_host():
    """All 274 positions in one call (3,535,116 nodes): outputs equal the
    fixture; nodes, move_scores and the rest equal the host twin's per
    position."""
    s = solved_all()
    assert_equals_fixture(s, range(len(s["score"])))
    assert_equals_host(s, host_all())
    assert int(s["nodes"].sum()) == 3535116


def test_one_workgroup_equals_default_grid_and_runs_repeat():
    """274 positions = 4,384 phase A and 70,144 phase B slots through one
    64-lane workgroup, and the default grid a second time: 2 x 3,535,116
    nodes. Every output is identical."""
    import othello_mcts as om

    base = solved_all()
    one = arrays(om.solve_endgames(triples(), 12, LIMIT, _workgroups=1, split=True))
    again = arrays(om.solve_endgames(triples(), 12, LIMIT, split=True))
    for k, v in base.items():
        assert np.array_equal(one[k], v), k
        assert np.array_equal(again[k], v), k


SENTINEL = {torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int32: 0x5A5A5A5A}


class Bracketed:
    """A tensor between two sentinel rows; ``inner`` is the part handed out."""

    def __init__(self, shape, dtype):
        self.dtype = dtype
        self.big = torch.full((shape[0] + 2, *shape[1:]), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.inner = self.big[1:-1]

    def intact(self):
        s = SENTINEL[self.dtype]
        return bool((self.big[0] == s).all()) and bool((self.big[-1] == s).all())


def test_outputs_stay_between_sentinel_rows():
    """65 positions (3,454,631 nodes per call) through the raw entry point
    with every output and the workspace bracketed by sentinel rows; then with
    the optional outputs passed as 0."""
    import othello_mcts as om
    from othello_mcts import _othello_mcts_impl as impl

    f = fixture()
    idx = np.argsort(-f["empties"], kind="stable")[:65].tolist()
    n = len(idx)
    pos = om.endgame.pack_positions(triples(idx)).to(DEV)
    B = {"move_scores": Bracketed((n, 65), torch.int32), "score": Bracketed((n,), torch.int32),
         "best_action": Bracketed((n,), torch.int32), "flags": Bracketed((n,), torch.int32),
         "nodes": Bracketed((n,), torch.int64)}
    ws_bytes = impl._solve_split_workspace_bytes(n)
    assert ws_bytes == 256 + n * (16 * 32 + (16 + 256) * 12) and ws_bytes % 8 == 0
    ws = Bracketed((ws_bytes // 8,), torch.int64)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    for grid in (0, 1, 3):
        for b in B.values():
            b.inner.fill_(SENTINEL[b.dtype])
        impl._gpu_solve_split(0, pos.data_ptr(), n, 12, LIMIT, B["move_scores"].inner.data_ptr(),
                              B["score"].inner.data_ptr(), B["best_action"].inner.data_ptr(),
                              B["flags"].inner.data_ptr(), B["nodes"].inner.data_ptr(), ws.inner.data_ptr(), grid,
                              stream)
        torch.cuda.synchronize()
        assert all(b.intact() for b in B.values()) and ws.intact(), grid
        assert_equals_fixture({k: b.inner.cpu().numpy() for k, b in B.items()}, idx)
        assert B["nodes"].inner.cpu().tolist() == [host_all()[i]["nodes"] for i in idx]
    # optional outputs: only move_scores; the others keep their sentinels
    for b in B.values():
        b.inner.fill_(SENTINEL[b.dtype])
    impl._gpu_solve_split(0, pos.data_ptr(), n, 12, LIMIT, B["move_scores"].inner.data_ptr(), 0, 0, 0, 0,
                          ws.inner.data_ptr(), 0, stream)
    torch.cuda.synchronize()
    assert np.array_equal(B["move_scores"].inner.cpu().numpy(), f["move_scores"][idx])
    assert all(b.intact() for b in B.values()) and ws.intact()
    for k in ("score", "best_action", "flags", "nodes"):
        assert bool((B[k].inner == SENTINEL[B[k].dtype]).all()), k


def test_flagged_rows_leave_their_neighbours_alone():
    """The 36 positions of the fixture with 9 and 10 empties (462,627 nodes),
    interleaved with rows that are refused: too many empties (12 > max 10),
    overlapping discs, player 3, player 0 on a live board; and terminal roots.
    Every row is as on the host."""
    import othello_mcts as om
    from othello_mcts import endgame as E

    f = fixture()
    good = [i for i in range(len(f["player"])) if 9 <= f["empties"][i] <= 10]
    deep = [i for i in range(len(f["player"])) if f["empties"][i] == 12]
    terminal = [i for i in range(len(f["player"])) if f["best_action"][i] < 0]
    rows, want = [], []
    for j, i in enumerate(good):
        rows.append(triples([i])[0])
        want.append(("good", i))
        kind = j % 5
        player, p1, p2 = triples([i])[0]
        if kind == 0:
            rows.append(triples([deep[j % len(deep)]])[0])
            want.append(("flag", E.FLAG_TOO_MANY_EMPTIES))
        elif kind == 1:
            rows.append((player, p1 | 1 << 30, p2 | 1 << 30))
            want.append(("flag", E.FLAG_INVALID))
        elif kind == 2:
            rows.append((3, p1, p2))
            want.append(("flag", E.FLAG_INVALID))
        elif kind == 3:
            rows.append((0, p1, p2))
            want.append(("flag", E.FLAG_INVALID))
        else:
            rows.append(triples([terminal[j % len(terminal)]])[0])
            want.append(("terminal", terminal[j % len(terminal)]))
    assert len(rows) == 72
    s = arrays(om.solve_endgames(rows, 10, LIMIT, split=True))
    for r, (what, v) in enumerate(want):
        if what == "good":
            assert s["flags"][r] == 0 and np.array_equal(s["move_scores"][r], f["move_scores"][v])
            assert s["score"][r] == f["score"][v] and s["best_action"][r] == f["best_action"][v]
            assert s["nodes"][r] == host_all()[v]["nodes"]
        elif what == "flag":
            assert s["flags"][r] == v and (s["move_scores"][r] == NONE).all() and s["score"][r] == NONE
            assert s["best_action"][r] == -1 and s["nodes"][r] == 0
        else:
            assert s["flags"][r] == 0 and (s["move_scores"][r] == NONE).all() and s["score"][r] == f["score"][v]
            assert s["best_action"][r] == -1 and s["nodes"][r] == 0
    assert_equals_host(s, [om.solve_position(p, 10, LIMIT, split=True) for p in rows])


def test_node_limit_flags_and_none_pattern_equal_the_host():
    """node_limit = 1000 per item on the fixture's 12-empties positions: some
    root actions stay within it, some stop in phase A (no phase B then), some
    in phase B: 5 of the 80 root actions keep their score, 84,928 nodes.
    Flags, the NONE pattern and nodes equal the host twin's."""
    import othello_mcts as om
    from othello_mcts import endgame as E

    f = fixture()
    deep = [i for i in range(len(f["player"])) if f["empties"][i] == 12 and f["best_action"][i] >= 0]
    s = arrays(om.solve_endgames(triples(deep), 12, 1000, split=True))
    host = [om.solve_position(p, 12, 1000, split=True) for p in triples(deep)]
    assert_equals_host(s, host)
    assert (s["flags"] == E.FLAG_NODE_LIMIT).all() and (s["score"] == NONE).all() and (s["best_action"] == -1).all()
    legal = f["move_scores"][deep] != NONE
    kept = (s["move_scores"] != NONE)
    assert not (kept & ~legal).any()
    assert np.array_equal(s["move_scores"][kept], f["move_scores"][deep][kept])
    assert 0 < int(kept.sum()) < int(legal.sum())


def test_14_empties_equals_host():
    """16 seeded random-play positions at 14 empties: scores, flags and nodes
    equal the host twin's; 17,708,485 nodes."""
    import othello_mcts as om

    ps = om.endgame.random_play_positions(14, 16, 11)
    s = om.solve_endgames(ps, 14, LIMIT, split=True)
    s.check()
    host = [om.solve_position(p, 14, LIMIT, split=True) for p in ps]
    assert_equals_host(arrays(s), host)
    print("split nodes at 14 empties:", sum(h["nodes"] for h in host))


def test_endgame_move_loss_split_equals_plain():
    """Roots of 8 games of a small net from random openings of up to 52 plies
    (BatchedMCTS.root_positions), played on until 16 recorded moves had a
    root of at most 10 empties (tests/test_gpu_endgame.py finds 30 with at
    most 8 in the same games played to the end): split=True gives the same
    loss, wdl_kept and empties as split=False. Under 10^6 nodes."""
    import othello_mcts as om
    from othello_mcts.synthetic import alphazero_state_dict

    net = om.NativeNet(alphazero_state_dict(4, 5, 128, 0, 32), device=0)
    b = om.BatchedMCTS(8, history_size=2, num_simulations=32, num_threads=1, batch_size=8, dirichlet_epsilon=0.0,
                       seed=12, node_capacity=1 << 14)
    b.random_openings(52, seed=9)
    checked = 0
    for _ in range(70):
        if checked >= 16:
            break
        roots = b.root_positions()
        b.search(net)
        actions = b.selfplay_move(temperature_moves=0)["actions"].clone()
        plain = om.endgame_move_loss(roots, actions, 10, LIMIT)
        split = om.endgame_move_loss(roots, actions, 10, LIMIT, split=True)
        assert all(torch.equal(x, y) for x, y in zip(plain, split))
        a = om.solve_endgames(roots, 10, LIMIT)
        c = om.solve_endgames(roots, 10, LIMIT, split=True)
        assert torch.equal(a.move_scores, c.move_scores) and torch.equal(a.score, c.score)
        assert torch.equal(a.best_action, c.best_action) and torch.equal(a.flags, c.flags)
        checked += int((plain[0] >= 0).sum())
    assert checked >= 16
