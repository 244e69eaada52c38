"""The baseline opponents on the host (csrc/baseline.h through
othello_mcts.baseline_move) against the fixture tests/golden/baseline.npz,
which tests/golden/make_baseline.py computed with the independent Python
reference tests/baseline_ref.py (unpruned negamax, its own bitboards)."""

import ctypes
import functools
import re

import numpy as np
import pytest
import torch

import baseline_ref as R
from conftest import PKG, ROOT

import othello_mcts as om
from othello_mcts import baseline as B

NONE = -(1 << 31)
KEY = 0x1234_5678_9ABC_DEF1


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(ROOT / "tests" / "golden" / "baseline.npz")
    return {k: z[k] for k in z.files}


def position(i):
    f = fixture()
    return int(f["player"][i]), int(f["p1"][i]), int(f["p2"][i])


def cases():
    """(case index, kind, depth, position index) of every stored case."""
    f = fixture()
    for c, (k, d, late) in enumerate(zip(f["case_kind"], f["case_depth"], f["case_late_only"])):
        for i in range(len(f["player"])):
            if not late or f["group"][i] == 3:
                yield c, int(k), max(1, int(d)), i


def empties(i):
    _, p1, p2 = position(i)
    return 64 - bin(p1 | p2).count("1")


def test_fixture_holds_what_the_tests_rely_on():
    f = fixture()
    n = len(f["player"])
    assert n >= 128 and f["move_scores"].shape == (8, n, 65)
    counts = dict(zip(f["count_names"].tolist(), f["counts"].tolist()))
    assert counts["root_pass"] >= 1 and counts["pass_below_root"] >= 4 and counts["early_terminal"] >= 4
    assert counts["tied_search"] >= 16 and counts["tied3_search"] >= 1
    for g, e in ((0, 44), (1, 30), (2, 18)):
        idx = np.nonzero(f["group"] == g)[0]
        assert len(idx) == 32 and all(empties(i) == e for i in idx)
    late = np.nonzero(f["group"] == 3)[0]
    assert len(late) >= 32 and all(5 <= empties(i) <= 8 for i in late)
    assert [(int(k), int(d)) for k, d in zip(f["case_kind"], f["case_depth"])] == \
        [(0, 0), (1, 0), (2, 1), (2, 2), (2, 3), (2, 4), (2, 6), (2, 8)]
    assert any(f["move_scores"][0, i, 64] == 0 for i in range(n))  # the forced pass is a root action


def test_host_baseline_equals_the_fixture_on_every_case():
    f = fixture()
    seen = 0
    for c, kind, depth, i in cases():
        got = om.baseline_move(position(i), kind, depth)
        want = f["move_scores"][c, i]
        assert got["move_scores"] == want.tolist(), (kind, depth, i)
        assert got["action"] == f["action"][c, i] and got["flags"] == 0
        assert got["score"] == want.max()
        assert (got["nodes"] == 0) == (kind != B.SEARCH)
        seen += 1
    assert seen >= 6 * 128 + 2 * 32


def test_reference_recomputed_live_equals_the_fixture():
    f = fixture()
    for c, kind, depth, i in cases():
        if kind == B.SEARCH and depth > 2:
            continue
        ms = R.move_scores(kind, depth, *position(i))
        assert ms == f["move_scores"][c, i].tolist(), (kind, depth, i)
        assert R.first_max(ms) == f["action"][c, i]


def test_deep_enough_search_gives_the_exact_solvers_scores():
    f = fixture()
    for i in np.nonzero(f["group"] == 3)[0]:
        e = empties(i)
        exact = om.solve_position(position(i), 12, 1 << 40)
        want = [NONE if s == -128 else B.terminal_value(s) for s in exact["move_scores"]]
        for depth in sorted({e, 8, 10}):
            got = om.baseline_move(position(i), B.SEARCH, depth, node_limit=1 << 40)
            assert got["move_scores"] == want, (i, depth)
            assert got["action"] == exact["best_action"]


def tied_case(min_ties):
    f = fixture()
    for c, kind, depth, i in cases():
        if kind == B.SEARCH and len(R.ties(f["move_scores"][c, i].tolist())) >= min_ties:
            return c, kind, depth, i
    raise AssertionError("no such case in the fixture")


def test_pick_without_a_key_is_the_lowest_tied_action():
    f = fixture()
    tied = 0
    for c, kind, depth, i in cases():
        t = R.ties(f["move_scores"][c, i].tolist())
        tied += len(t) >= 2
        assert f["action"][c, i] == t[0]
    assert tied >= 16 + 128  # RANDOM ties every root with two moves


def test_pick_with_keys_reaches_every_tied_action_and_no_other():
    f = fixture()
    c, kind, depth, i = tied_case(3)
    t = R.ties(f["move_scores"][c, i].tolist())
    got = [om.baseline_move(position(i), kind, depth, key=KEY, event=ev)["action"] for ev in range(64)]
    assert set(got) == set(t)
    again = [om.baseline_move(position(i), kind, depth, key=KEY, event=ev)["action"] for ev in range(64)]
    assert again == got
    # every case of two shallow kinds: a keyed pick is a tied action, the scores do not move
    for c, kind, depth, i in cases():
        if kind == B.SEARCH and depth > 1:
            continue
        for ev in (0, 7):
            r = om.baseline_move(position(i), kind, depth, key=KEY + i, event=ev)
            assert r["move_scores"] == f["move_scores"][c, i].tolist()
            assert r["action"] in R.ties(r["move_scores"])


def test_keyed_pick_follows_the_stated_rule_and_the_tensor_form():
    """k = min(nt - 1, int(u * nt)) with u = uniform(stream_key(key, event, 0), 0),
    computed here from csrc/rng.h's constants in Python ints."""
    M = (1 << 64) - 1

    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)

    def uniform(key, event):
        sk = mix((mix(key ^ ((event * 0xD1B54A32D192ED03) & M)) + 0x9E3779B97F4A7C15) & M)
        m = mix((sk + 0x9E3779B97F4A7C15) & M) >> 41
        return np.float32(2 * m + 1) * np.float32(2.0 ** -24)

    f = fixture()
    c, kind, depth, i = tied_case(3)
    ms = f["move_scores"][c, i].tolist()
    t = R.ties(ms)
    keys = [KEY, 1, (1 << 63) - 5, 0]
    for key in keys:
        for ev in range(16):
            k = min(len(t) - 1, int(uniform(key, ev) * np.float32(len(t))))
            assert om.baseline_move(position(i), kind, depth, key=key, event=ev)["action"] == t[k]
    # the Gauntlet's tensor form of the same rule
    K = torch.tensor([k for k in keys for _ in range(16)], dtype=torch.int64)
    E = torch.tensor([ev for _ in keys for ev in range(16)], dtype=torch.int64)
    u = B.stream_uniform(K, E)
    assert u.dtype == torch.float32
    assert u.tolist() == [float(uniform(k, e)) for k, e in zip(K.tolist(), E.tolist())]
    scores = torch.tensor([ms] * len(K), dtype=torch.int32)
    legal = scores != NONE
    want = [om.baseline_move(position(i), kind, depth, key=k, event=e)["action"]
            for k, e in zip(K.tolist(), E.tolist())]
    assert B.pick_actions(scores, legal, K, E).tolist() == want
    assert B.pick_actions(scores, torch.zeros_like(legal), K, E).tolist() == [-1] * len(K)


def test_greedy_scores_are_flip_counts():
    f = fixture()
    for i in range(len(f["player"])):
        player, p1, p2 = position(i)
        me, opp = (p1, p2) if player == 1 else (p2, p1)
        ms = om.baseline_move(position(i), B.GREEDY)["move_scores"]
        legal = om.get_legal_moves(me, opp)
        for a in range(64):
            if legal >> (63 - a) & 1:
                assert ms[a] == bin(om.get_flips(1 << (63 - a), me, opp)).count("1") > 0
            else:
                assert ms[a] == NONE
        assert ms[64] == (0 if legal == 0 else NONE)


def test_flags_and_terminal_roots():
    player, p1, p2 = position(0)
    flagged = {"move_scores": [NONE] * 65, "score": NONE, "action": -1}
    for kind in (B.RANDOM, B.GREEDY, B.SEARCH):
        r = om.baseline_move((player, p1 | 1, p2 | 1), kind, 2)  # overlapping discs
        assert r["flags"] == B.FLAG_INVALID and {k: r[k] for k in flagged} == flagged and r["nodes"] == 0
        assert om.baseline_move((3, p1, p2), kind, 2)["flags"] == B.FLAG_INVALID
        assert om.baseline_move((0, p1, p2), kind, 2)["flags"] == B.FLAG_INVALID  # marked over, but a side can move
        # nobody can move: no action, no flag, whatever `player` says
        for pl in (0, 1, 2):
            r = om.baseline_move((pl, (1 << 64) - 1 - 0xFF, 0xF0), kind, 2)
            assert r["flags"] == 0 and {k: r[k] for k in flagged} == flagged
    r = om.baseline_move(position(0), B.SEARCH, 4, node_limit=10)
    assert r["flags"] == B.FLAG_NODE_LIMIT and {k: r[k] for k in flagged} == flagged and r["nodes"] > 0
    full = om.baseline_move(position(0), B.SEARCH, 4)
    per_action_max = full["nodes"]  # a budget no root action exceeds is no limit
    assert om.baseline_move(position(0), B.SEARCH, 4, node_limit=per_action_max) == full
    # node_limit does not bind the kinds that search nothing
    assert om.baseline_move(position(0), B.GREEDY, node_limit=1)["flags"] == 0


def test_argument_errors():
    p = position(0)
    for kind in (-1, 3, "minimax"):
        with pytest.raises(ValueError):
            om.baseline_move(p, kind)
    for depth in (0, 11, -1):
        with pytest.raises(ValueError, match="depth"):
            om.baseline_move(p, B.SEARCH, depth)
    om.baseline_move(p, B.GREEDY, 0)  # depth is read for SEARCH only
    assert om.baseline_move(p, "search", 2) == om.baseline_move(p, B.SEARCH, 2)
    with pytest.raises(ValueError, match="node_limit"):
        om.baseline_move(p, B.SEARCH, 1, node_limit=0)
    for bad in (dict(kind=1.0), dict(kind=B.SEARCH, depth=True), dict(kind=B.SEARCH, key="k")):
        with pytest.raises(TypeError):
            om.baseline_move(p, **bad)
    with pytest.raises(TypeError):
        om.baseline_move("nope", B.RANDOM)
    with pytest.raises(ValueError):
        om.baseline_moves(torch.zeros((2, 4), dtype=torch.int64), B.RANDOM)
    with pytest.raises(ValueError, match="host baseline"):
        om.baseline_moves(torch.zeros((2, 5), dtype=torch.int64), B.RANDOM)
    assert B.baseline_name("random") == "random" and B.baseline_name(B.GREEDY) == "greedy"
    assert B.baseline_name(B.SEARCH, 4) == "search-4"


def test_c_abi_rejects_bad_arguments_before_any_device():
    lib = ctypes.CDLL(str(PKG / "othello_mcts" / "liboamd.so"))
    pos = (ctypes.c_int64 * 5)(1, 0x0000000810000000, 0x0000001008000000, 0, 0)
    ms = (ctypes.c_int32 * 65)()
    i32 = [ctypes.c_int32() for _ in range(3)]
    nodes = ctypes.c_int64()
    lib.oamd_host_baseline_move.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int64,
                                            ctypes.c_int32, ctypes.c_uint64, ctypes.c_uint64] + [ctypes.c_void_p] * 5
    outs = [ms, *map(ctypes.byref, i32), ctypes.byref(nodes)]

    def host(kind, depth, limit, outs=outs):
        return lib.oamd_host_baseline_move(pos, kind, depth, limit, 0, 0, 0, *outs)

    legal = om.get_legal_moves(pos[1], pos[2])
    assert host(2, 3, 1 << 24) == 0 and legal >> (63 - i32[1].value) & 1 and nodes.value > 0
    assert [m for m in ms if m != NONE] and i32[0].value == max(ms)
    for kind, depth, limit in ((3, 1, 1), (-1, 1, 1), (2, 0, 1), (2, 11, 1), (2, 1, 0)):
        assert host(kind, depth, limit) == 1
    assert host(2, 3, 1 << 24, [None] + outs[1:]) == 1
    assert host(2, 3, 1 << 24, outs[:4] + [None]) == 1
    lib.oamd_baseline_moves.argtypes = [ctypes.c_int32, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int32,
                                        ctypes.c_int32, ctypes.c_int64] + [ctypes.c_void_p] * 8 + \
        [ctypes.c_int32, ctypes.c_void_p]
    fake = ctypes.c_void_p(4096)  # never dereferenced: every call fails its argument checks
    for kind, depth in ((3, 1), (2, 0), (2, 11)):
        assert lib.oamd_baseline_moves(0, fake, 1, kind, depth, 1, None, None, fake, fake, fake, fake, fake, fake, 0,
                                       None) == 1
    assert lib.oamd_baseline_moves(0, fake, 1, 2, 1, 1, None, None, fake, None, fake, fake, fake, fake, 0, None) == 1
    b = ctypes.c_int64()
    assert lib.oamd_baseline_workspace_bytes(10, ctypes.byref(b)) == 0 and b.value >= 10 * 65 * 8
    assert lib.oamd_baseline_workspace_bytes(10, None) == 1


def test_header_symbols_are_exported_and_stubbed():
    header = (ROOT / "include" / "othello_mcts_amd.h").read_text()
    names = set(re.findall(r"\b(oamd_(?:host_)?baseline_[a-z0-9_]+)\s*\(", header))
    assert names == {"oamd_baseline_workspace_bytes", "oamd_baseline_moves", "oamd_host_baseline_move"}
    lib = ctypes.CDLL(str(PKG / "othello_mcts" / "liboamd.so"))
    assert all(hasattr(lib, n) for n in names)
    assert re.search(r"#define OAMD_BASELINE_NONE INT32_MIN", header)
    stub = (PKG / "othello_mcts" / "_othello_mcts_impl.pyi").read_text()
    for n in ("_host_baseline", "_baseline_workspace_bytes", "_gpu_baseline"):
        assert f"def {n}(" in stub
    for n in ("baseline_move", "baseline_moves", "BaselineMoves", "Gauntlet"):
        assert n in om.__all__ and hasattr(om, n)
    from othello_mcts import provenance

    assert {"baseline.h", "baseline.hip"} <= set(provenance.FAMILIES["all"])
