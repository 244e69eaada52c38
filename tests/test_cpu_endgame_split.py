"""The split endgame solver on the host (csrc/solver.h solve_host_split through
othello_mcts.solve_position(split=True)) against the fixture
tests/golden/endgames.npz, against the current solver, and its node accounting
on constructed positions. Every call carries a node limit of at most 2^24 per
item; none binds unless the test says so."""

import ast
import ctypes
import functools
import importlib.util
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import endgame_ref as R
import oracle as O

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "othello-alphazero_amd"
NONE = -128
LIMIT = 1 << 24


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(Path(__file__).parent / "golden" / "endgames.npz")
    return {k: z[k] for k in z.files}


def position(i):
    f = fixture()
    return int(f["player"][i]), int(f["p1"][i]), int(f["p2"][i])


@functools.lru_cache(maxsize=None)
def split_all():
    """The whole fixture through the split host solver; shared, read only."""
    import othello_mcts as om

    return [om.solve_position(position(i), 12, LIMIT, split=True) for i in range(len(fixture()["player"]))]


def bits(*actions):
    return sum(1 << (63 - a) for a in actions)


FULL = (1 << 64) - 1


def test_split_equals_fixture():
    """All 274 positions, root passes, terminal roots and wipe-outs among them
    (the fixture's kinds): 3,535,116 nodes."""
    f = fixture()
    for bit in (R.ROOT_PASS, R.ROOT_TERMINAL, R.WIPEOUT):
        assert int((f["kinds"] & bit != 0).sum()) >= 5
    for i, s in enumerate(split_all()):
        assert s["flags"] == 0, i
        assert s["move_scores"] == f["move_scores"][i].tolist(), i
        assert s["score"] == f["score"][i] and s["best_action"] == f["best_action"][i], i
        assert (s["nodes"] == 0) == (f["best_action"][i] < 0)


def test_split_visits_at_most_half_the_nodes():
    """The current solver visits 8,532,650 nodes on the fixture
    (tests/test_gpu_endgame.py); the split solver 3,535,116."""
    total = sum(s["nodes"] for s in split_all())
    print("split node total over the fixture:", total)
    assert total * 2 <= 8532650


def test_constructed_positions_and_their_node_counts():
    """Positions small enough to count by hand. Black (player 1) has every
    disc that is neither white nor empty."""
    import othello_mcts as om

    # L = 64: white at 1, 57 and 30, empties 0, 56 and 31. Whichever black plays, white must pass (Q's mover
    # passes, R is black's again) and black takes the rest, a corner first, ending 64-0. Per root action: Q, the
    # pass, and a phase A item of 3 nodes (after the corner, white's pass, after the last move); L = 64, so phase B
    # is skipped. With phase B the other move of R would add 3 nodes per action.
    white, empty = bits(1, 57, 30), bits(0, 56, 31)
    p = (1, FULL & ~(white | empty), white)
    s = om.solve_position(p, 12, LIMIT, split=True)
    want = [NONE] * 65
    want[0] = want[56] = want[31] = 64
    assert s == {"move_scores": want, "score": 64, "best_action": 0, "flags": 0, "nodes": 15}
    old = om.solve_position(p, 12, LIMIT)
    assert (old["move_scores"], old["score"], old["best_action"]) == (want, 64, 0)
    # the same seen from white's chair: colours swapped, player 2
    s = om.solve_position((2, white, FULL & ~(white | empty)), 12, LIMIT, split=True)
    assert s == {"move_scores": want, "score": 64, "best_action": 0, "flags": 0, "nodes": 15}

    # the game ends at Q: one empty (0), white at 1. Black fills the board: no item, 1 node.
    p = (1, FULL & ~bits(0, 1), bits(1))
    s = om.solve_position(p, 12, LIMIT, split=True)
    want = [NONE] * 65
    want[0] = 64
    assert s == {"move_scores": want, "score": 64, "best_action": 0, "flags": 0, "nodes": 1}

    # Q's mover passes and R has one move: empties 0 and 56, white at 1 and 57. Root action 0: Q (white cannot
    # move), the pass, then the single item 56 of 1 node (the board is full). Root action 56 likewise.
    white, empty = bits(1, 57), bits(0, 56)
    p = (1, FULL & ~(white | empty), white)
    s = om.solve_position(p, 12, LIMIT, split=True)
    want = [NONE] * 65
    want[0] = want[56] = 64
    assert s == {"move_scores": want, "score": 64, "best_action": 0, "flags": 0, "nodes": 6}

    # a root pass whose Q is the opponent's position with two moves: white to move cannot, black has 0 and 56
    s = om.solve_position((2, FULL & ~(white | empty), white), 12, LIMIT, split=True)
    want = [NONE] * 65
    want[64] = -64
    # Q = black to move (1 node, no pass); items 0 and 56: phase A (corner 0 first): after 0, white passes, after
    # 56: 3 nodes, L = 64 for black, phase B skipped
    assert s == {"move_scores": want, "score": -64, "best_action": 64, "flags": 0, "nodes": 4}
    old = om.solve_position((2, FULL & ~(white | empty), white), 12, LIMIT)
    assert (old["move_scores"], old["score"], old["best_action"]) == (want, -64, 64)


def test_found_positions_cover_every_plan_kind():
    """Among the fixture's positions the host twin meets root actions after
    which the game is over and after which the mover passes; their scores are
    the fixture's (test_split_equals_fixture). Found by the oracle's rules."""
    f = fixture()
    ends = passes = 0
    for i in range(len(f["player"])):
        if f["best_action"][i] < 0 or f["empties"][i] > 6:
            continue
        player, p1, p2 = position(i)
        me, opp = (p1, p2) if player == 1 else (p2, p1)
        for a in range(64):
            if f["move_scores"][i][a] == NONE:
                continue
            qme, qopp = R.play(me, opp, a)
            if not O.get_legal_moves(qme, qopp):
                if O.get_legal_moves(qopp, qme):
                    passes += 1
                else:
                    ends += 1
    assert ends >= 5 and passes >= 5


def test_split_equals_current_solver_at_13_empties():
    """16 seeded random-play positions at 13 empties: the current solver
    visits 27,492,148 nodes, the split solver 6,269,333."""
    import othello_mcts as om

    ps = om.endgame.random_play_positions(13, 16, 7)
    total = 0
    for p in ps:
        a = om.solve_position(p, 13, LIMIT, split=True)
        b = om.solve_position(p, 13, 1 << 40)
        assert a["flags"] == 0 and b["flags"] == 0
        assert a["move_scores"] == b["move_scores"] and a["score"] == b["score"]
        assert a["best_action"] == b["best_action"]
        assert a["nodes"] < b["nodes"]
        total += a["nodes"]
    print("split nodes at 13 empties:", total)


def test_flags():
    import othello_mcts as om
    from othello_mcts import endgame as E

    f = fixture()
    searched = [i for i in range(len(f["player"])) if f["best_action"][i] >= 0]
    for i in searched[::7]:
        e = int(f["empties"][i])
        s = om.solve_position(position(i), max_empties=e - 1, node_limit=LIMIT, split=True)
        assert s["flags"] == E.FLAG_TOO_MANY_EMPTIES and s["score"] == NONE and s["best_action"] == -1
        assert s["move_scores"] == [NONE] * 65 and s["nodes"] == 0
        assert om.solve_position(position(i), max_empties=e, node_limit=LIMIT, split=True)["flags"] == 0
    # a terminal root is never searched, so never too deep
    t = int(np.argmax(f["best_action"] < 0))
    s = om.solve_position(position(t), max_empties=0, node_limit=LIMIT, split=True)
    assert s["score"] == f["score"][t] and s["flags"] == 0 and s["nodes"] == 0 and s["best_action"] == -1
    player, p1, p2 = position(searched[0])
    s = om.solve_position((player, p1 | 1 << 20, p2 | 1 << 20), node_limit=LIMIT, split=True)
    assert s["flags"] == E.FLAG_INVALID and s["score"] == NONE and s["best_action"] == -1 and s["nodes"] == 0
    for bad_player in (-1, 3, 7):
        assert om.solve_position((bad_player, p1, p2), node_limit=LIMIT, split=True)["flags"] == E.FLAG_INVALID
    # player 0 on a board where a side can move: nobody to search for
    assert om.solve_position((0, p1, p2), node_limit=LIMIT, split=True)["flags"] == E.FLAG_INVALID


class OverBudget(Exception):
    pass


class SplitRef:
    """DESIGN.md §15's rules written a second time, recursively in Python over the
    oracle's bitboards: the ordered pick, fail-soft alpha-beta with the
    solver's node count, the plan (Q, R, phase A move) and the two phases."""

    CORNERS = 0x8100000000000081
    NEXT_TO_CORNER = 0x42C300000000C342

    def __init__(self, limit):
        self.limit = limit
        self.count = 0

    def visit(self):
        self.count += 1
        if self.count > self.limit:
            raise OverBudget

    def static_pick(self, moves):
        c = moves & self.CORNERS or moves & ~self.NEXT_TO_CORNER or moves
        return 1 << (c.bit_length() - 1)

    def pick(self, me, opp, moves):
        if moves & (moves - 1) == 0 or R.popcount(R.FULL & ~(me | opp)) < 6:
            return self.static_pick(moves)
        counts = {}
        for sq in R.squares(moves):
            counts[sq] = R.popcount(O.get_legal_moves(*R.play(me, opp, sq)))
        fewest = min(counts.values())
        return self.static_pick(sum(1 << (63 - sq) for sq, c in counts.items() if c == fewest))

    def enter(self, me, opp, alpha, beta):
        """Value for `me`, to move at a position just reached."""
        self.visit()
        moves = O.get_legal_moves(me, opp)
        if not moves:
            theirs = O.get_legal_moves(opp, me)
            if not theirs:
                return R.popcount(me) - R.popcount(opp)
            self.visit()  # the position after the pass
            return -self.frame(opp, me, theirs, -beta, -alpha)
        return self.frame(me, opp, moves, alpha, beta)

    def frame(self, me, opp, moves, alpha, beta):
        best = -65
        while moves:
            m = self.pick(me, opp, moves)
            moves ^= m
            v = -self.enter(*R.play(me, opp, 63 - (m.bit_length() - 1)), -beta, -alpha)
            best, alpha = max(best, v), max(alpha, v)
            if alpha >= beta:
                break
        return best


def split_ref(player, p1, p2, limit):
    """(move_scores, flags, nodes) of a live, valid root by SplitRef."""
    me, opp = (p1, p2) if player == 1 else (p2, p1)
    legal = O.get_legal_moves(me, opp)
    ms, nodes, flagged = [NONE] * 65, 0, False
    for a in R.squares(legal) if legal else [64]:
        qme, qopp = R.play(me, opp, a) if a != 64 else (opp, me)
        nodes += 1
        moves, sign = O.get_legal_moves(qme, qopp), -1
        rme, ropp = qme, qopp
        if not moves:
            moves, sign = O.get_legal_moves(qopp, qme), 1
            if not moves:
                ms[a] = R.popcount(qopp) - R.popcount(qme)
                continue
            rme, ropp = qopp, qme
            nodes += 1

        def item(m, alpha):
            ref = SplitRef(limit)
            try:
                return -ref.enter(*R.play(rme, ropp, 63 - (m.bit_length() - 1)), -64, -alpha), ref.count
            except OverBudget:
                return None, ref.count

        first = SplitRef(limit).pick(rme, ropp, moves)
        value, c = item(first, -64)
        nodes += c
        ok = value is not None
        if ok and value < 64:
            lower = value
            for sq in R.squares(moves & ~first):
                v, c = item(1 << (63 - sq), lower)
                nodes += c
                if v is None:
                    ok = False
                elif v > value:
                    value = v
        if ok:
            ms[a] = sign * value
        else:
            flagged = True
    return ms, 2 if flagged else 0, nodes


def test_node_counts_and_limits_equal_the_python_twin():
    """Fixture positions with 5..8 empties (both sides of the ordering
    threshold of 6), unlimited and with node_limit = 10 per item: move_scores,
    the NONE pattern, the flag and the node count equal a recursive Python
    rewrite of the rules (SplitRef). At 12 empties node_limit = 10 stops every
    root action in phase A: Q and 11 nodes each."""
    import othello_mcts as om
    from othello_mcts import endgame as E

    f = fixture()
    idx = [i for i in range(len(f["player"])) if 5 <= f["empties"][i] <= 8 and f["best_action"][i] >= 0]
    assert len(idx) >= 40
    partly = 0
    for i in idx[::2]:
        for limit in (LIMIT, 10):
            ms, flags, nodes = split_ref(*position(i), limit)
            s = om.solve_position(position(i), 12, limit, split=True)
            assert s["move_scores"] == ms and s["flags"] == flags and s["nodes"] == nodes, (i, limit)
            if limit == LIMIT:
                assert ms == f["move_scores"][i].tolist() and s == split_all()[i]
            elif flags:
                assert s["score"] == NONE and s["best_action"] == -1
                partly += any(v != NONE for v in ms)
            else:
                assert s == split_all()[i]
    assert partly >= 3  # some root actions within the budget beside some over it
    deep = [i for i in range(len(f["player"])) if f["empties"][i] == 12 and f["best_action"][i] >= 0]
    assert len(deep) >= 5
    for i in deep:
        s = om.solve_position(position(i), 12, node_limit=10, split=True)
        assert s["flags"] == E.FLAG_NODE_LIMIT and s["score"] == NONE and s["best_action"] == -1
        assert s["move_scores"] == [NONE] * 65
        assert s["nodes"] == 12 * int((f["move_scores"][i] != NONE).sum())


def test_argument_errors():
    import othello_mcts as om
    from othello_mcts import _othello_mcts_impl as impl

    p = position(0)
    with pytest.raises(ValueError, match=r"Expected 0 <= max_empties <= 16, but got 17\."):
        om.solve_position(p, max_empties=17, split=True)
    with pytest.raises(ValueError, match=r"Expected 1 <= node_limit < 2\^56, but got 0\."):
        om.solve_position(p, node_limit=0, split=True)
    with pytest.raises(TypeError, match="Expected an int for max_empties, but got float."):
        om.solve_position(p, max_empties=12.0, split=True)
    with pytest.raises(TypeError, match="Expected a Position or a"):
        om.solve_position(5, split=True)
    # the C ABI validates on its own, same messages
    with pytest.raises(ValueError, match=r"Expected 0 <= max_empties <= 16, but got 17\."):
        impl._host_solve_split(1, 0, 0, 17, 100)
    with pytest.raises(ValueError, match=r"Expected 1 <= node_limit < 2\^56, but got 0\."):
        impl._host_solve_split(1, 0, 0, 12, 0)
    with pytest.raises(ValueError, match=r"Expected 0 <= n <= \d+, but got -1\."):
        impl._solve_split_workspace_bytes(-1)
    # counter block, 16 plans of 32 bytes, 16 + 256 item slots of a word and a score each
    assert impl._solve_split_workspace_bytes(3) == 256 + 3 * (16 * 32 + (16 + 256) * (8 + 4))
    with pytest.raises(ValueError, match=r"Expected 1 <= budget <= 1048576, but got 0\."):
        impl._relabel_split_workspace_bytes(0)
    assert impl._relabel_split_workspace_bytes(5) == impl._solve_split_workspace_bytes(5) + 5 * (40 + 4 * (1 + 65 + 3))
    with pytest.raises(ValueError, match=r"Expected positions as an \(n, 5\) int64 tensor"):
        import torch

        om.solve_endgames(torch.zeros((3, 4), dtype=torch.int64), split=True)


def test_abi_exports_the_split_functions():
    header = (ROOT / "include" / "othello_mcts_amd.h").read_text()
    declared = set(re.findall(r"\b(oamd_[a-z0-9_]+)\s*\(", header))
    new = {"oamd_solve_split_workspace_bytes", "oamd_solve_endgames_split", "oamd_host_solve_endgame_split",
           "oamd_replay_relabel_split_workspace_bytes", "oamd_replay_relabel_endgames_split"}
    assert new <= declared
    experimental = (ROOT / "include" / "othello_mcts_amd_experimental.h").read_text()
    assert re.search(r"\boamd_solve_endgames_split_grid\s*\(", experimental)
    assert "oamd_solve_endgames_split_grid" not in header
    lib = ctypes.CDLL(str(PKG / "othello_mcts" / "liboamd.so"))
    assert all(hasattr(lib, n) for n in new | {"oamd_solve_endgames_split_grid"})
    assert lib.oamd_abi_version() == 1
    # bad arguments come back as OAMD_INVALID_ARGUMENT (1) without touching a device
    lib.oamd_last_error.restype = ctypes.c_char_p
    n = ctypes.c_int64(0)
    i64 = ctypes.c_int64
    assert lib.oamd_solve_split_workspace_bytes(i64(-1), ctypes.byref(n)) == 1
    assert b"Expected 0 <= n" in lib.oamd_last_error()
    assert lib.oamd_solve_split_workspace_bytes(i64(1), None) == 1
    assert lib.oamd_solve_endgames_split(0, None, i64(4), 17, i64(100), None, None, None, None, None, None, None) == 1
    assert b"max_empties" in lib.oamd_last_error()
    assert lib.oamd_solve_endgames_split(0, None, i64(4), 12, i64(0), None, None, None, None, None, None, None) == 1
    assert b"node_limit" in lib.oamd_last_error()
    assert lib.oamd_solve_endgames_split(0, None, i64(-1), 12, i64(100), None, None, None, None, None, None,
                                         None) == 1
    assert b"Expected 0 <= n" in lib.oamd_last_error()
    assert lib.oamd_solve_endgames_split_grid(0, None, i64(4), 12, i64(100), None, None, None, None, None, None, 0,
                                              None) == 1
    assert b"workgroups" in lib.oamd_last_error()
    assert lib.oamd_host_solve_endgame_split(None, 12, i64(100), None, None, None, None, None) == 1
    assert b"position and move_scores" in lib.oamd_last_error()
    assert lib.oamd_replay_relabel_split_workspace_bytes(i64(0), ctypes.byref(n)) == 1
    assert b"budget" in lib.oamd_last_error()
    assert lib.oamd_replay_relabel_endgames_split(None, None, None, 17, i64(8), i64(100), 0, 0, None, None) == 1
    assert b"max_empties" in lib.oamd_last_error()
    assert lib.oamd_replay_relabel_endgames_split(None, None, None, 10, i64(8), i64(100), 2, 0, None, None) == 1
    assert b"policy_mode" in lib.oamd_last_error()
    # the host entry point through ctypes: the fixture's first searched position
    f = fixture()
    i = int(np.argmax(f["best_action"] >= 0))

    class Pos(ctypes.Structure):
        _fields_ = [("player", ctypes.c_int32), ("pad", ctypes.c_int32), ("p1", ctypes.c_uint64),
                    ("p2", ctypes.c_uint64), ("legal", ctypes.c_uint64), ("next_legal", ctypes.c_uint64)]

    pos = Pos(*((position(i)[0], 0) + position(i)[1:] + (0, 0)))
    ms = (ctypes.c_int32 * 65)()
    score = ctypes.c_int32(0)
    assert lib.oamd_host_solve_endgame_split(ctypes.byref(pos), 12, i64(LIMIT), ms, ctypes.byref(score), None, None,
                                             None) == 0
    assert list(ms) == f["move_scores"][i].tolist() and score.value == f["score"][i]


def test_stub_lists_the_split_names():
    import othello_mcts._othello_mcts_impl as impl

    tree = ast.parse(Path(impl.__file__).with_name("_othello_mcts_impl.pyi").read_text())
    names = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
    new = {"_host_solve_split", "_solve_split_workspace_bytes", "_gpu_solve_split", "_relabel_split_workspace_bytes"}
    assert new <= names and all(hasattr(impl, n) for n in new)
    view = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "_ReplayView")
    assert "relabel_split" in {n.name for n in view.body if isinstance(n, ast.FunctionDef)}
    assert hasattr(impl._ReplayView, "relabel_split")


def test_build_checks_the_item_kernel_for_scratch():
    """build.py fails when the split solver's item kernel reports scratch; the
    planning and reducing kernels are not search kernels."""
    spec = importlib.util.spec_from_file_location("oamd_build_endgame_split", PKG / "build.py")
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    remark = ("solver.hip:136:0: remark: Function Name: {} [-Rpass-analysis=kernel-resource-usage]\n"
              "solver.hip:136:0: remark:     ScratchSize [bytes/lane]: {} [-Rpass-analysis=kernel-resource-usage]\n")
    items = "_ZN4oamd12_GLOBAL__N_113k_solve_itemsEPKNS_9SolvePlanEyiPKiPKllPiPlPy"
    solve = "_ZN4oamd12_GLOBAL__N_17k_solveEPK13oamd_positionlilPiPlPy"
    plan = "_ZN4oamd12_GLOBAL__N_112k_solve_planEPK13oamd_positionliPNS_9SolvePlanE"
    b.check_solver_scratch(remark.format(solve, 0) + remark.format(items, 0))
    with pytest.raises(SystemExit, match="k_solve_items.*scratch"):
        b.check_solver_scratch(remark.format(solve, 0) + remark.format(items, 448))
    b.check_solver_scratch(remark.format(solve, 0) + remark.format(plan, 64))
    with pytest.raises(SystemExit, match="no resource remark"):
        b.check_solver_scratch(remark.format(plan, 0))


def test_standalone_check_runs_clean_under_the_sanitizers(tmp_path):
    """tools/solver_split_check.cpp, a program of its own, built with
    -fsanitize=address,undefined: the split host solver against an exhaustive
    minimax (0..8 empties), against solve_host (10..12 empties), the flags and
    the node accounting. No Python runs under a sanitizer."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # build.py's compiler
    exe = tmp_path / "solver_split_check"
    subprocess.run([hipcc, "-O1", "-g", "-x", "hip", "--offload-arch=gfx950", "-Xarch_host",
                    "-fsanitize=address,undefined", "-I", str(PKG / "csrc"),
                    str(ROOT / "tools" / "solver_split_check.cpp"), "-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
    assert re.search(r"[1-9]\d* with L = 64", r.stdout)


def test_host_resources_check_runs_clean_under_the_sanitizers(tmp_path):
    """tools/host_resources_check.cpp, a program of its own, built by the host
    compiler alone with -fsanitize=address,undefined: csrc/host_resources.h
    (the owners of the host layer's device resources and the engine's resource
    sets) over counting HIP stubs. Every creating call of one scenario fails
    once: the call reports it, every set still holds what it held, the retry
    succeeds, and the run ends in the state of the run without a failure;
    nothing is live after destruction or released twice; streams and events
    are created in the order the schedules were measured with. No Python runs
    under a sanitizer."""
    hipcc = Path(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))  # build.py's compiler: its headers
    exe = tmp_path / "host_resources_check"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-D__HIP_PLATFORM_AMD__",
                    "-I", str(hipcc.parent.parent / "include"), "-I", str(PKG / "csrc"),
                    str(ROOT / "tools" / "host_resources_check.cpp"), "-o", str(exe)], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 failures" in r.stdout and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr
    assert re.search(r"([1-9]\d*) creating calls, \1 runs with one of them failing", r.stdout)
