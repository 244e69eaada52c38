"""Exact endgame value targets of the replay buffer, the parts that need no
GPU: the numpy restatement (tests/relabel_ref.py) against the fixture
tests/golden/endgames.npz and against the host solver, the optimal policy, the
argument errors raised before a device is touched, and the C ABI's exports."""

import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import endgame_ref as E
import relabel_ref as L

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "othello-alphazero_amd"
BIG = 1 << 40


def relabelled(positions, outcomes, H=1, policy="keep", solve=None, max_empties=12):
    """A RelabelRef fed one game per position (G = 1: ring order = list
    order), before and after relabel_endgames."""
    rng = np.random.default_rng(5)
    ref = L.RelabelRef(1, H, len(positions) + 3, solve=solve or L.table_solver())
    for m in L.games_script(rng, 1, H, [([p], o) for p, o in zip(positions, outcomes)]):
        ref.add(m)
    before = (ref.value.copy(), ref.policy.copy())
    ref.relabel_endgames(max_empties=max_empties, policy=policy)
    return ref, before


def test_initial_position_is_the_fillers_60_empties():
    import othello_mcts as om

    p = om.Position.initial_position()
    assert (p.player(), p.player1_discs(), p.player2_discs()) == L.INITIAL
    assert 64 - L.popcount(L.INITIAL[1] | L.INITIAL[2]) == 60


def test_reference_relabel_equals_fixture_in_the_movers_view():
    f = L.fixture()
    pos = L.replay_positions(f)
    n = len(pos)
    want = np.array([L.mover_score(pos[i][0], int(f["score"][i]), int(f["best_action"][i])) for i in range(n)])
    # the convention, spelled out: only a terminal root with white to move is negated
    player = np.array([p[0] for p in pos])
    terminal_white = (f["best_action"] < 0) & (player == 2)
    assert terminal_white.sum() >= 2 and ((f["best_action"] < 0) & (player == 1)).sum() >= 2
    assert np.array_equal(want, np.where(terminal_white, -f["score"], f["score"]))
    outcomes = [L.disagreeing_outcome(pos[i][0], int(want[i]), i) for i in range(n)]
    # the reference's own search up to 8 empties, the table of its earlier results above
    small = [i for i in range(n) if f["empties"][i] <= 8]
    assert len(small) >= 200
    ref, _ = relabelled([pos[i] for i in small], [outcomes[i] for i in small], solve=E.solve)
    assert np.array_equal(ref.exact_scores(), want[small])
    ref, (v0, _) = relabelled(pos, outcomes)
    assert ref.size == n and np.array_equal(ref.exact_scores(), want)
    live = ref.live_slots()
    assert np.array_equal(ref.value[live], np.sign(want).astype(np.float32))
    assert not (v0[live] == ref.value[live]).any()  # every outcome was chosen to disagree
    assert ref.relabel_counters.tolist() == [n, 0, 0, n]


def test_reference_relabel_equals_the_host_solver():
    import othello_mcts as om

    pos = L.replay_positions()
    ref, _ = relabelled(pos, [1 + i % 3 for i in range(len(pos))])
    got = ref.exact_scores()
    seen = set()
    for i, (player, p1, p2) in enumerate(pos):
        s = om.solve_position((player, p1, p2), 12, BIG)
        assert s["flags"] == 0
        assert got[i] == L.mover_score(player, s["score"], s["best_action"]), i
        if s["best_action"] < 0:
            # the host solver reports black minus white whoever is to move: the mover's view negates it for white
            assert s["score"] == L.popcount(p1) - L.popcount(p2)
            assert got[i] == (s["score"] if player == 1 else -s["score"])
            seen.add(("terminal", player))
        elif s["best_action"] == 64:
            seen.add(("pass", player))
    assert seen == {("terminal", 1), ("terminal", 2), ("pass", 1), ("pass", 2)}


def test_optimal_policy_sits_on_the_argmax_set():
    f = L.fixture()
    pos = L.replay_positions(f)
    ref, (_, p0) = relabelled(pos, [2] * len(pos), policy="optimal")
    ties = 0
    for i, slot in enumerate(ref.live_slots().tolist()):
        row = ref.policy[slot]
        if f["best_action"][i] < 0:  # a terminal root keeps its row
            assert np.array_equal(row, p0[slot])
            continue
        best = f["move_scores"][i] == f["score"][i]
        assert np.array_equal(row != 0, best) and best[f["best_action"][i]]
        assert row.sum(dtype=np.float64) == pytest.approx(1.0, abs=1e-6)
        assert len(set(row[best].tolist())) == 1
        ties += best.sum() > 1
        if f["best_action"][i] == 64:
            assert row[64] == 1.0
    assert ties >= 10


def test_budget_age_order_and_retry_in_the_reference():
    f = L.fixture()
    pos = [p for p, e in zip(L.fixture_positions(f), f["empties"]) if 3 <= e <= 5][:6]
    rng = np.random.default_rng(0)
    ref = L.RelabelRef(1, 1, 4, solve=L.table_solver(f))
    for m in L.games_script(rng, 1, 1, [([p], 2) for p in pos]):  # 6 positions through a ring of 4
        ref.add(m)
    assert ref.head == 2 and ref.size == 4
    ref.relabel_endgames(budget=3, gives_up=lambda *p: p == pos[3])
    assert ref.relabel_counters.tolist() == [2, 1, 1, 3]
    e = ref.exact_scores()
    assert e[1] == L.EXACT_GAVE_UP and e[3] == L.EXACT_UNKNOWN and abs(int(e[0])) <= 64 and abs(int(e[2])) <= 64
    ref.relabel_endgames(budget=3)
    assert ref.relabel_counters.tolist() == [3, 1, 0, 1] and ref.exact_scores()[1] == L.EXACT_GAVE_UP
    ref.relabel_endgames(budget=3, retry=True)
    assert ref.relabel_counters.tolist() == [4, 1, 0, 1] and (np.abs(ref.exact_scores().astype(int)) <= 64).all()
    # an overwritten slot forgets its label
    ref.add(L.games_script(rng, 1, 1, [([None], 3)])[0])
    assert ref.exact_scores().tolist()[-1] == L.EXACT_UNKNOWN and ref.value[ref.live_slots()[-1]] == -1.0


def test_argument_errors_need_no_gpu():
    import othello_mcts as om
    from othello_mcts import _othello_mcts_impl as impl
    from othello_mcts import replay

    assert (replay.EXACT_UNKNOWN, replay.EXACT_GAVE_UP) == (-128, -127)
    with pytest.raises(TypeError, match="Expected a bool for track_exact, but got int."):
        om.ReplayBuffer(2, 2, 8, track_exact=1)
    with pytest.raises(ValueError, match=r"Expected capacity < 2\^31 with track_exact"):
        om.ReplayBuffer(2, 2, 1 << 31, track_exact=True)
    with pytest.raises(ValueError, match="lives on a ROCm GPU"):
        om.ReplayBuffer(2, 2, 8, device="cpu", track_exact=True)

    rb = om.ReplayBuffer.__new__(om.ReplayBuffer)  # no storage: the checks come before it is touched
    rb.track_exact = False
    cases = [
        (dict(max_empties=17), ValueError, r"Expected 0 <= max_empties <= 16, but got 17\."),
        (dict(max_empties=-1), ValueError, r"Expected 0 <= max_empties <= 16, but got -1\."),
        (dict(max_empties=10.0), TypeError, "Expected an int for max_empties, but got float."),
        (dict(node_limit=0), ValueError, r"Expected 1 <= node_limit < 2\^56, but got 0\."),
        (dict(budget=0), ValueError, r"Expected 1 <= budget <= 1048576, but got 0\."),
        (dict(budget=(1 << 20) + 1), ValueError, r"Expected 1 <= budget <= 1048576, but got 1048577\."),
        (dict(budget=True), TypeError, "Expected an int for budget, but got bool."),
        (dict(policy="best"), ValueError, "Expected policy 'keep' or 'optimal', but got 'best'."),
        (dict(policy=1), TypeError, "Expected a str for policy, but got int."),
        (dict(retry=1), TypeError, "Expected a bool for retry, but got int."),
    ]
    for kwargs, exc, msg in cases:
        with pytest.raises(exc, match=msg):
            rb.relabel_endgames(**kwargs)
    with pytest.raises(RuntimeError, match="track_exact=True"):
        rb.relabel_endgames()
    with pytest.raises(RuntimeError, match="track_exact=True"):
        rb.relabel_stats
    with pytest.raises(RuntimeError, match="track_exact=True"):
        rb.exact_scores()
    # the C ABI validates on its own, same messages
    with pytest.raises(ValueError, match=r"Expected 1 <= budget <= 1048576, but got 0\."):
        impl._relabel_workspace_bytes(0)
    # the solver's workspace plus the position list, the slot list and the solver's four outputs
    assert impl._relabel_workspace_bytes(5) == impl._solve_workspace_bytes(5) + 5 * (40 + 4 * (1 + 65 + 3))


def test_abi_exports_the_relabel_functions():
    header = (ROOT / "include" / "othello_mcts_amd.h").read_text()
    declared = set(re.findall(r"\b(oamd_[a-z0-9_]+)\s*\(", header))
    new = {"oamd_replay_add_tracked", "oamd_replay_relabel_workspace_bytes", "oamd_replay_relabel_endgames"}
    assert new <= declared
    lib = ctypes.CDLL(str(PKG / "othello_mcts" / "liboamd.so"))
    assert all(hasattr(lib, n) for n in new)
    assert lib.oamd_abi_version() == 1
    # additive: the view's layout is as it was (15 fields, 104 bytes)
    view = re.search(r"typedef struct oamd_replay_view \{(.*?)\} oamd_replay_view;", header, re.S).group(1)
    assert len(re.findall(r";", re.sub(r"/\*.*?\*/", "", view, flags=re.S))) == 15
    # bad arguments come back as OAMD_INVALID_ARGUMENT without touching a device
    lib.oamd_last_error.restype = ctypes.c_char_p
    n = ctypes.c_int64(0)
    assert lib.oamd_replay_relabel_workspace_bytes(ctypes.c_int64(0), ctypes.byref(n)) != 0
    assert b"budget" in lib.oamd_last_error()
    assert lib.oamd_replay_relabel_endgames(None, None, None, 17, ctypes.c_int64(8), ctypes.c_int64(100), 0, 0, None,
                                            None) != 0
    assert b"max_empties" in lib.oamd_last_error()
    assert lib.oamd_replay_relabel_endgames(None, None, None, 10, ctypes.c_int64(8), ctypes.c_int64(100), 2, 0, None,
                                            None) != 0
    assert b"policy_mode" in lib.oamd_last_error()
    assert lib.oamd_replay_add_tracked(None, None, 1, None, None, None, None, None) != 0
    assert b"exact" in lib.oamd_last_error()
