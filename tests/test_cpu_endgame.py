"""The exact endgame solver on the host (csrc/solver.h through
othello_mcts.solve_position) against the fixture tests/golden/endgames.npz,
which tests/golden/make_endgames.py solved with the independent Python
reference tests/endgame_ref.py (negamax over the oracle's bitboards)."""

import functools
import time

import numpy as np
import pytest

import endgame_ref as R
import oracle as O

NONE = -128
BIG = 1 << 40


@functools.lru_cache(maxsize=None)
def fixture():
    from pathlib import Path

    z = np.load(Path(__file__).parent / "golden" / "endgames.npz")
    return {k: z[k] for k in z.files}


def position(i):
    f = fixture()
    return int(f["player"][i]), int(f["p1"][i]), int(f["p2"][i])


def transform_board(b, t):
    return sum(1 << (63 - O.transform_action(s, t)) for s in range(64) if b >> (63 - s) & 1)


def test_fixture_holds_every_kind_of_position():
    f = fixture()
    n = len(f["player"])
    assert 250 <= n <= 350 and f["move_scores"].shape == (n, 65)
    for bit in (R.ROOT_PASS, R.ROOT_TERMINAL, R.PASS_INSIDE, R.ENDS_WITH_EMPTIES, R.WIPEOUT):
        assert int((f["kinds"] & bit != 0).sum()) >= 5, bit
    for player in (1, 2):
        assert int((f["player"] == player).sum()) >= 5
    for e in (0, 1, 2):
        assert int((f["empties"] == e).sum()) >= 5
    assert set(f["empties"].tolist()) == set(range(13))
    # the stored kinds are what the host solver's own line of perfect play shows
    import othello_mcts as om

    for i in range(n):
        k = R.kinds(*position(i), solver=lambda *p: om.solve_position(p, 12, BIG)["best_action"])
        assert k == int(f["kinds"][i]), i
    # structure of the stored solutions
    for i in range(n):
        ms = f["move_scores"][i]
        legal = ms != NONE
        if f["best_action"][i] < 0:
            assert not legal.any()
        else:
            assert f["score"][i] == ms[legal].max() and f["best_action"][i] == int(np.argmax(ms == f["score"][i]))


def test_reference_alphabeta_equals_exhaustive_minimax():
    f = fixture()
    idx = [i for i in range(len(f["player"])) if f["empties"][i] <= 7]
    assert len(idx) >= 150
    for i in idx:
        ms, score, best = R.solve(*position(i), search=R.minimax)
        assert ms == f["move_scores"][i].tolist() and score == f["score"][i] and best == f["best_action"][i], i
        assert R.solve(*position(i), search=R.alphabeta) == (ms, score, best), i


def test_solve_position_equals_fixture():
    import othello_mcts as om

    f = fixture()
    for i in range(len(f["player"])):
        s = om.solve_position(position(i), 12, BIG)
        assert s["flags"] == 0, i
        assert s["move_scores"] == f["move_scores"][i].tolist(), i
        assert s["score"] == f["score"][i] and s["best_action"] == f["best_action"][i], i
        assert (s["nodes"] == 0) == (f["best_action"][i] < 0)
        # the default limits solve every position up to 12 empties
        assert om.solve_position(position(i)) == s


def test_solve_position_takes_a_position_object():
    import othello_mcts as om

    p = om.Position.initial_position()
    for _ in range(4):
        p = p.apply_action(p.legal_actions()[0])
    s = om.solve_position(p, max_empties=4)
    assert s["flags"] == om.endgame.FLAG_TOO_MANY_EMPTIES and s["score"] == NONE and s["best_action"] == -1
    assert s["move_scores"] == [NONE] * 65 and s["nodes"] == 0
    assert s == om.solve_position((p.player(), p.player1_discs(), p.player2_discs()), max_empties=4)


def test_d4_transforms_permute_move_scores():
    import othello_mcts as om

    f = fixture()
    idx = np.linspace(0, len(f["player"]) - 1, 32).astype(int)
    for i in idx:
        player, p1, p2 = position(i)
        base = om.solve_position((player, p1, p2), 12, BIG)
        for t in range(8):
            s = om.solve_position((player, transform_board(p1, t), transform_board(p2, t)), 12, BIG)
            want = [NONE] * 65
            for a in range(65):
                want[O.transform_action(a, t)] = base["move_scores"][a]
            assert s["move_scores"] == want, (i, t)
            assert s["score"] == base["score"] and s["flags"] == 0


def test_flags():
    import othello_mcts as om
    from othello_mcts import endgame as E

    f = fixture()
    searched = [i for i in range(len(f["player"])) if f["best_action"][i] >= 0]
    for i in searched[::7]:
        e = int(f["empties"][i])
        s = om.solve_position(position(i), max_empties=e - 1)
        assert s["flags"] == E.FLAG_TOO_MANY_EMPTIES and s["score"] == NONE and s["best_action"] == -1
        assert s["move_scores"] == [NONE] * 65 and s["nodes"] == 0
        assert om.solve_position(position(i), max_empties=e)["flags"] == 0
    # a terminal root is never searched, so never too deep
    t = int(np.argmax(f["best_action"] < 0))
    assert om.solve_position(position(t), max_empties=0)["score"] == f["score"][t]
    deep = [i for i in searched if f["empties"][i] == 12]
    t0 = time.perf_counter()
    for i in deep:
        s = om.solve_position(position(i), 12, node_limit=10)
        assert s["flags"] == E.FLAG_NODE_LIMIT and s["score"] == NONE and s["best_action"] == -1
        legal = f["move_scores"][i] != NONE
        # every root action gives up after at most one node past its budget
        assert s["nodes"] <= 11 * int(legal.sum())
        assert all(v == NONE or v == w for v, w in zip(s["move_scores"], f["move_scores"][i].tolist()))
    assert time.perf_counter() - t0 < 1.0  # 10 positions x <= 11 nodes per root action
    player, p1, p2 = position(searched[0])
    s = om.solve_position((player, p1 | 1 << 20, p2 | 1 << 20))
    assert s["flags"] == E.FLAG_INVALID and s["score"] == NONE and s["best_action"] == -1 and s["nodes"] == 0
    for bad_player in (-1, 3, 7):
        assert om.solve_position((bad_player, p1, p2))["flags"] == E.FLAG_INVALID
    # player 0 on a board where a side can move: nobody to search for
    assert om.solve_position((0, p1, p2))["flags"] == E.FLAG_INVALID


def test_argument_errors():
    import othello_mcts as om
    from othello_mcts import _othello_mcts_impl as impl

    p = position(0)
    with pytest.raises(ValueError, match=r"Expected 0 <= max_empties <= 16, but got 17\."):
        om.solve_position(p, max_empties=17)
    with pytest.raises(ValueError, match=r"Expected 0 <= max_empties <= 16, but got -1\."):
        om.solve_position(p, max_empties=-1)
    with pytest.raises(ValueError, match=r"Expected 1 <= node_limit < 2\^56, but got 0\."):
        om.solve_position(p, node_limit=0)
    with pytest.raises(TypeError, match="Expected an int for max_empties, but got float."):
        om.solve_position(p, max_empties=12.0)
    with pytest.raises(TypeError, match="Expected a Position or a"):
        om.solve_position(5)
    # the C ABI validates on its own, same messages
    with pytest.raises(ValueError, match=r"Expected 0 <= max_empties <= 16, but got 17\."):
        impl._host_solve(1, 0, 0, 17, 100)
    with pytest.raises(ValueError, match=r"Expected 1 <= node_limit < 2\^56, but got 0\."):
        impl._host_solve(1, 0, 0, 12, 0)
    with pytest.raises(ValueError, match=r"Expected 0 <= n <= \d+, but got -1\."):
        impl._solve_workspace_bytes(-1)
    assert impl._solve_workspace_bytes(3) == 256 + 3 * 65 * 8
    with pytest.raises(ValueError, match=r"Expected positions as an \(n, 5\) int64 tensor"):
        import torch

        om.solve_endgames(torch.zeros((3, 4), dtype=torch.int64))


def test_build_checks_the_solver_for_scratch():
    """build.py fails when k_solve reports scratch, and keeps the ResNet's
    VGPR rule to resnet.hip."""
    import importlib.util
    from pathlib import Path

    spec = importlib.util.spec_from_file_location("oamd_build_endgame",
                                                  Path(__file__).parents[1] / "othello-alphazero_amd" / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "-Rpass-analysis=kernel-resource-usage" in b.UNITS["solver.hip"]
    assert set(b.RESOURCE_CHECKS) == {"resnet.hip", "solver.hip"}
    remark = ("solver.hip:47:1: remark: Function Name: _ZN4oamd12_GLOBAL__N_17k_solveEPK13oamd_positionlilPiPlPy "
              "[-Rpass-analysis=kernel-resource-usage]\n"
              "solver.hip:47:1: remark:     ScratchSize [bytes/lane]: {} [-Rpass-analysis=kernel-resource-usage]\n")
    b.check_solver_scratch(remark.format(0))
    with pytest.raises(SystemExit, match="scratch"):
        b.check_solver_scratch(remark.format(448))
    with pytest.raises(SystemExit, match="no resource remark"):
        b.check_solver_scratch("")
