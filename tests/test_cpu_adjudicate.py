"""Adjudication by the exact solver without a GPU: the rule on
the host (othello_mcts.adjudicate), the argument checks of every layer, the C
ABI's new entry points and the stub file."""

import ast
import ctypes
import functools
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "othello-alphazero_amd"
FULL = (1 << 64) - 1
NEW_ABI = {"oamd_engine_selfplay_move_adjudicated", "oamd_engine_selfplay_steps_adjudicated",
           "oamd_arena_move_adjudicated", "oamd_arena_play_adjudicated"}


def bits(*squares):
    return sum(1 << (63 - s) for s in squares)


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(Path(__file__).parent / "golden" / "endgames.npz")
    return {k: z[k] for k in z.files}


def position(i):
    f = fixture()
    return int(f["player"][i]), int(f["p1"][i]), int(f["p2"][i])


def code_of(margin):
    return 2 if margin > 0 else (3 if margin < 0 else 1)


# Square 0 is the only empty square, square 2 the only disc of one colour, the
# other colour holds the rest. The side holding the rest has no move (every
# neighbour of square 0 is its own); the other side plays square 0 and flips
# square 1: 3 discs against 61.
LONE, REST = bits(2), FULL & ~bits(0, 2)


def test_rule_on_hand_made_positions():
    import othello_mcts as om

    # the mover must pass: still adjudicated; black holds the rest and ends 61 : 3
    assert om.Position is not None
    assert om.adjudicate((1, REST, LONE), 1) == (2, 58)
    assert om.adjudicate((1, REST, LONE), 16) == (2, 58)
    # white to move (and passing), colours swapped: the solver's +58 for the mover is -58 for black
    assert om.adjudicate((2, LONE, REST), 1) == (3, -58)
    # white to move and moving: black holds the rest, white plays square 0
    assert om.adjudicate((2, REST, LONE), 1) == (2, 58)
    # off, and above K empties
    assert om.adjudicate((1, REST, LONE), 0) is None
    two_empty = (1, REST & ~bits(63), LONE)
    assert om.adjudicate(two_empty, 1) is None and om.adjudicate(two_empty, 2) is not None
    # terminal whatever the side-to-move field says: the board decides, not the solver
    for player in (0, 1, 2):
        assert om.adjudicate((player, FULL & ~bits(0), 0), 8) is None  # one colour only: nobody can move
        assert om.adjudicate((player, FULL >> 32, FULL << 32 & FULL), 8) is None  # full board
    # a Position object works like its triple
    p = om.Position.initial_position()
    assert om.adjudicate(p, 16) is None  # 60 empties


def test_draw_is_code_1_and_sign_follows_the_mover():
    import othello_mcts as om

    f = fixture()
    seen = {"draw": 0, "white": 0, "black": 0}
    for i in np.nonzero((f["empties"] <= 8) & (f["best_action"] >= 0))[0]:
        player, p1, p2 = position(i)
        got = om.adjudicate((player, p1, p2), 8)
        score = int(f["score"][i])
        margin = -score if player == 2 else score
        assert got == (code_of(margin), margin), i
        seen["draw" if margin == 0 else ("white" if player == 2 else "black")] += 1
    assert min(seen.values()) > 0, seen
    draw = int(np.nonzero((f["empties"] <= 8) & (f["best_action"] >= 0) & (f["score"] == 0))[0][0])
    assert om.adjudicate(position(draw), 8) == (1, 0)


@pytest.mark.parametrize("split", [False, True])
def test_consistent_with_solve_position_over_the_fixture(split):
    """Every fixture position with at most 8 empties: None exactly for the
    terminal ones, else solve_position's score seen from black."""
    import othello_mcts as om

    f = fixture()
    idx = np.nonzero(f["empties"] <= 8)[0]
    assert len(idx) > 200
    n_none = 0
    for i in idx:
        player, p1, p2 = position(i)
        s = om.solve_position((player, p1, p2), 8, (1 << 56) - 1, split=split)
        assert s["flags"] == 0
        got = om.adjudicate((player, p1, p2), 8, split=split)
        if s["best_action"] < 0:
            assert got is None, i
            n_none += 1
            continue
        margin = -s["score"] if player == 2 else s["score"]
        assert got == (code_of(margin), margin), i
        # at K below the position's empties the rule does not apply
        e = int(f["empties"][i])
        if e >= 1:
            assert om.adjudicate((player, p1, p2), e - 1, split=split) is None
    assert n_none == int((f["best_action"][idx] < 0).sum()) > 0


def test_argument_errors_before_a_device_is_touched():
    """No engine exists here: the checks come first in every method."""
    import othello_mcts as om
    from othello_mcts.adjudication import check_adjudicate_empties

    for bad in (-1, 17):
        msg = rf"Expected 0 <= adjudicate_empties <= 16, but got {bad}\."
        with pytest.raises(ValueError, match=msg):
            om.adjudicate((1, REST, LONE), bad)
        with pytest.raises(ValueError, match=msg):
            om.BatchedMCTS.selfplay_move(None, adjudicate_empties=bad)
        with pytest.raises(ValueError, match=msg):
            om.BatchedMCTS.selfplay_steps(None, None, 4, adjudicate_empties=bad)
        with pytest.raises(ValueError, match=msg):
            om.Arena.move(None, adjudicate_empties=bad)
        with pytest.raises(ValueError, match=msg):
            om.Arena.play(None, None, None, adjudicate_empties=bad)
        with pytest.raises(ValueError, match=msg):
            om.self_play(None, None, 1, adjudicate_empties=bad)
    with pytest.raises(TypeError, match="Expected an int for adjudicate_empties"):
        om.adjudicate((1, REST, LONE), 8.0)
    with pytest.raises(TypeError, match="Expected an int for adjudicate_empties"):
        om.BatchedMCTS.selfplay_move(None, adjudicate_empties=True)
    with pytest.raises(ValueError, match="needs keep_all=True"):
        om.BatchedMCTS.selfplay_steps(None, None, 2, keep_all=False, adjudicate_empties=8)
    # one move overwrites nothing; off needs nothing
    assert check_adjudicate_empties(8, 1, False) == 8 and check_adjudicate_empties(0, 5, False) == 0
    assert check_adjudicate_empties(16, 64, True) == 16


def test_abi_exports_the_adjudicated_functions():
    header = (ROOT / "include" / "othello_mcts_amd.h").read_text()
    declared = set(re.findall(r"\b(oamd_[a-z0-9_]+)\s*\(", header))
    assert NEW_ABI <= declared
    lib = ctypes.CDLL(str(PKG / "othello_mcts" / "liboamd.so"))
    assert all(hasattr(lib, n) for n in NEW_ABI)
    assert lib.oamd_abi_version() == 1
    lib.oamd_last_error.restype = ctypes.c_char_p
    fin = (ctypes.c_int32 * 4)()
    # OAMD_INVALID_ARGUMENT (1) before any pointer is followed
    for k in (-1, 17):
        assert lib.oamd_engine_selfplay_move_adjudicated(None, None, None, fin, None, None, k, 0, None) == 1
        assert b"max_empties" in lib.oamd_last_error()
        assert lib.oamd_engine_selfplay_steps_adjudicated(None, None, None, 4, 1, None, fin, None, None, k, 0,
                                                          None) == 1
        assert b"max_empties" in lib.oamd_last_error()
        assert lib.oamd_arena_move_adjudicated(None, None, None, None, fin, None, None, k, 0, None) == 1
        assert b"max_empties" in lib.oamd_last_error()
        assert lib.oamd_arena_play_adjudicated(None, None, None, None, None, 8, None, fin, None, None, k, 0,
                                               None) == 1
        assert b"max_empties" in lib.oamd_last_error()
    # several moves into one slice would overwrite the pending positions
    assert lib.oamd_engine_selfplay_steps_adjudicated(None, None, None, 2, 0, None, fin, None, None, 8, 0, None) == 1
    assert b"per_move_outputs" in lib.oamd_last_error()
    # the outcome bits need somewhere to go
    assert lib.oamd_engine_selfplay_move_adjudicated(None, None, None, None, None, None, 8, 0, None) == 1
    assert b"finished" in lib.oamd_last_error()
    experimental = (ROOT / "include" / "othello_mcts_amd_experimental.h").read_text()
    assert re.search(r"\boamd_engine_adjudicate_ms\s*\(", experimental) and hasattr(lib, "oamd_engine_adjudicate_ms")
    assert "oamd_engine_adjudicate_ms" not in header
    # the pinned self-play config did not grow
    assert re.search(r"typedef struct oamd_selfplay_config \{[^}]*int32_t emit_targets;[^}]*\} oamd_selfplay_config;",
                     header)
    body = re.search(r"typedef struct oamd_selfplay_config \{([^}]*)\}", header).group(1)
    assert len(re.findall(r"\b(?:int32_t|float)\s+\w+;", body)) == 4


def test_stub_lists_the_adjudicated_methods():
    import othello_mcts._othello_mcts_impl as impl

    tree = ast.parse(Path(impl.__file__).with_name("_othello_mcts_impl.pyi").read_text())
    engine = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "_Engine")
    stub = {n.name: n for n in engine.body if isinstance(n, ast.FunctionDef)}
    new = {"selfplay_move_adjudicated": 11, "selfplay_steps_adjudicated": 14, "arena_move_adjudicated": 10,
           "arena_play_adjudicated": 12, "adjudicate_ms": 0}
    for name, n_args in new.items():
        assert name in stub and hasattr(impl._Engine, name), name
        assert len(stub[name].args.posonlyargs) + len(stub[name].args.args) == n_args + 1, name  # + self
    # every public method of the extension's engine is in the stub, and the other way round
    real = {n for n in dir(impl._Engine) if not n.startswith("_") and callable(getattr(impl._Engine, n))}
    assert real == {n for n in stub if not n.startswith("_")}


def test_python_layer_names():
    import othello_mcts as om
    from othello_mcts import adjudication, arena, selfplay

    assert selfplay.FIN_ADJUDICATED == adjudication.FIN_ADJUDICATED == arena._ADJUDICATED == 32
    assert selfplay.FIN_SOLVER_FLAG == adjudication.FIN_SOLVER_FLAG == arena._SOLVER_FLAG == 64
    assert adjudication.MARGIN_NONE == -(1 << 31)
    from othello_mcts import replay

    header = (ROOT / "include" / "othello_mcts_amd.h").read_text()
    assert replay.FLAG_SOLVER == 16 and re.search(r"#define OAMD_REPLAY_SOLVER_FLAG 16\b", header)
    assert "adjudicate" in om.__all__
    import torch

    # ArenaResult as before this change (five fields): margin is the disc difference, nothing adjudicated
    r = om.ArenaResult(actions=torch.zeros((0, 3), dtype=torch.int32), result=torch.tensor([1, 0, -1]),
                       a_is_white=torch.tensor([False, True, True]),
                       discs=torch.tensor([[40, 24], [32, 32], [0, 0]]), plies=0)
    assert r.margin.tolist() == [16, 0, 0] and r.adjudicated.tolist() == [False, False, False]
    assert r.margin_a().tolist() == [16, 0, 0]
    r = om.ArenaResult(actions=r.actions, result=torch.tensor([2, 1, 0]), a_is_white=r.a_is_white,
                       discs=torch.tensor([[30, 26], [30, 26], [28, 28]]), plies=0,
                       margin=torch.tensor([-4, 6, 0]), adjudicated=torch.tensor([True, True, True]))
    assert r.margin_a().tolist() == [-4, -6, 0] and r.wdl() == (0, 1, 2)
