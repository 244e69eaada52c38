"""Given positions without a GPU: the canonical form against the
oracle's positions, board strings, the new surface, the frozen roots of the GPU
tests, and analyze's record assembly against the dict-tree PV walk of
tests/positions_ref.py."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import asym_stub as A
import oracle as O
import positions_ref as R


@functools.lru_cache(maxsize=None)
def chains():
    return A.random_game_chains(40)


@functools.lru_cache(maxsize=None)
def final_positions():
    out = []
    for game in range(40):
        rng = np.random.default_rng(game)
        p = O.initial_position()
        while p.player != 0:
            legal = O.legal_actions(p)
            p = O.apply_action(p, int(legal[int(rng.integers(len(legal)))]))
        out.append(p)
    return out


def fields(p):
    return (p.player(), p.player1_discs(), p.player2_discs(), p.legal_moves(), p.next_legal_moves())


# ------------------------------------------------------------ canonical form
def test_canonical_form_reproduces_every_oracle_position():
    import othello_mcts as om

    cs = chains()
    assert len(cs) == 2411
    passes = terminal = 0
    for c in cs:
        p = c[0]
        passes += p.player != 0 and p.legal == 0
        terminal += p.player == 0
        got = om.canonical_position((p.player, p.p1, p.p2))
        assert fields(got) == (p.player, p.p1, p.p2, p.legal, p.next_legal)
    assert (passes, terminal) == (11, 0)


@pytest.mark.parametrize("player", [1, 2])
def test_final_positions_come_back_terminal(player):
    import othello_mcts as om

    for p in final_positions():
        assert p.player == 0 and p.legal == 0 and p.next_legal == 0
        got = om.canonical_position((player, p.p1, p.p2))
        assert got.is_terminal()
        assert fields(got) == (0, p.p1, p.p2, 0, 0)
    # a position that says terminal stays terminal and carries no moves
    init = O.initial_position()
    assert fields(om.canonical_position((0, init.p1, init.p2))) == (0, init.p1, init.p2, 0, 0)


def test_canonical_form_takes_a_position_and_ignores_its_other_fields():
    import othello_mcts as om

    p = om.Position.initial_position().apply_action(19)
    assert om.canonical_position(p) == p


def test_invalid_positions_are_rejected():
    import othello_mcts as om

    init = O.initial_position()
    with pytest.raises(ValueError, match="overlap"):
        om.canonical_position((1, init.p1 | 1, init.p2 | 1))
    with pytest.raises(ValueError, match="player"):
        om.canonical_position((3, init.p1, init.p2))
    with pytest.raises(ValueError, match="player"):
        om.canonical_position((-1, init.p1, init.p2))


# -------------------------------------------------------------- board strings
def test_board_strings_round_trip():
    import othello_mcts as om

    for c in chains():
        p = om.canonical_position((c[0].player, c[0].p1, c[0].p2))
        text = om.format_board(p)
        assert len(text) == 66 and text[64] == " "
        assert om.parse_board(text) == p
    for p in final_positions():
        t = om.canonical_position((1, p.p1, p.p2))
        assert om.parse_board(om.format_board(t)) == t


def test_board_string_dialects_and_errors():
    import othello_mcts as om

    init = om.Position.initial_position()
    rows = ["--------", "........", "--------", "---OX---", "---*o---", "--------", "--------", "--------"]
    assert om.parse_board("\n".join(rows) + "\n X\n") == init
    assert om.parse_board("".join(rows) + "*") == init
    white = om.parse_board("".join(rows) + "O")
    assert white.player() == 2 and white.legal_moves() == O.get_legal_moves(init.player2_discs(), init.player1_discs())
    # square 0 is a1, the top bit
    assert om.parse_board("X" + "-" * 63 + "X").player1_discs() == 1 << 63
    for bad in ("".join(rows), "".join(rows) + "-", "".join(rows) + "XX", "?" + "".join(rows)[1:] + "X", ""):
        with pytest.raises(ValueError):
            om.parse_board(bad)
    with pytest.raises(TypeError):
        om.parse_board(None)


# -------------------------------------------------------------------- exports
def test_new_symbols_are_exported_and_abi_version_stays():
    import capi_host as H
    import othello_mcts as om

    raw = ctypes.CDLL(str(H.LIB_PATH))
    header = H.HEADER.read_text()
    for name in ("oamd_engine_set_positions", "oamd_engine_principal_variations", "oamd_host_canonical_position"):
        assert hasattr(raw, name), name
        assert name in header
    assert raw.oamd_abi_version() == 1
    for name in ("analyze", "Analysis", "canonical_position", "parse_board", "format_board"):
        assert name in om.__all__ and hasattr(om, name)
    for name in ("set_positions", "principal_variations"):
        assert hasattr(om.BatchedMCTS, name)
    # the host function itself, through ctypes
    fn = raw.oamd_host_canonical_position
    fn.argtypes = [ctypes.POINTER(H.Position), ctypes.POINTER(H.Position)]
    fn.restype = ctypes.c_int
    p = chains()[359][0]  # a pass position
    src, dst = H.Position(p.player, 0, p.p1, p.p2, 0xDEAD, 0xBEEF), H.Position()
    assert fn(ctypes.byref(src), ctypes.byref(dst)) == H.OAMD_OK
    assert dst.tuple() == (p.player, p.p1, p.p2, 0, p.next_legal) and p.next_legal != 0
    src.player = 3
    assert fn(ctypes.byref(src), ctypes.byref(dst)) == H.OAMD_INVALID_ARGUMENT
    src.player, src.player2_discs = 1, p.p1
    assert fn(ctypes.byref(src), ctypes.byref(dst)) == H.OAMD_INVALID_ARGUMENT


# ---------------------------------------------------- the GPU tests' frozen data
def test_frozen_roots_are_what_the_gpu_tests_say():
    cs = chains()
    assert tuple(len(cs[i]) for i in R.ROOT_INDICES) == R.ROOT_LENGTHS
    assert sorted(R.ROOT_LENGTHS)[:2] == [1, 3]  # shorter than H = 4
    for i in R.PASS_ROOTS:
        assert i in R.ROOT_INDICES and cs[i][0].legal == 0 and cs[i][0].player != 0 and len(cs[i]) == 60
    mid = [n for i, n in zip(R.ROOT_INDICES, R.ROOT_LENGTHS) if i not in R.PASS_ROOTS and n > 3]
    assert len(mid) == 4 and all(20 <= n <= 45 for n in mid)


def test_position_keys_are_the_engines_game_keys():
    from othello_mcts.analysis import position_key

    for seed, i in ((0, 0), (17, 2), (2**64 - 1, 300), (12345678901234567890, 7)):
        assert position_key(seed, i) == A.game_key(seed, i)
    assert position_key(17, 0) == A.ROW_KEYS[0]


# ------------------------------------------------------------ record assembly
def _hand_rows():
    """Three hand-made games: a plain line, a tie at the root (actions 19 and 26
    both 7), and an unsearched root. Returns the dict trees and the tensors the
    engine's read-outs would hold."""
    v = np.zeros((3, 65), np.int32)
    q = np.zeros((3, 65), np.float32)
    v[0, [19, 26, 37]] = [5, 9, 2]
    q[0, [19, 26, 37]] = [0.25, -0.5, 0.125]
    v[1, [19, 26, 44]] = [7, 7, 1]
    q[1, [19, 26, 44]] = [0.5, 0.75, -1.0]
    below0 = {26: {"children": [(18, 4, 0.5, {"children": [(10, 3, -0.25, None)]}), (20, 4, 0.0, None)]}}
    below1 = {19: {"children": [(64, 6, -0.125, {"children": [(3, 0, 0.0, None)]})]}}
    trees = [R.root_tree(v[0], q[0], below0), R.root_tree(v[1], q[1], below1), R.root_tree(v[2], q[2])]
    return trees, v, q


def _pv_tensors(trees, max_len):
    n = len(trees)
    pv = {"actions": torch.full((n, max_len), -1, dtype=torch.int32),
          "visits": torch.zeros((n, max_len), dtype=torch.int32),
          "q": torch.zeros((n, max_len), dtype=torch.float32), "length": torch.zeros(n, dtype=torch.int32)}
    for i, t in enumerate(trees):
        line = R.pv_walk(t, max_len)
        pv["length"][i] = len(line)
        for k, (a, nv, qq) in enumerate(line):
            pv["actions"][i, k], pv["visits"][i, k], pv["q"][i, k] = a, nv, qq
    return pv


def test_pv_walk_reference():
    trees, _, _ = _hand_rows()
    assert R.pv_walk(trees[0], 8) == [(26, 9, -0.5), (18, 4, 0.5), (10, 3, -0.25)]
    assert R.pv_walk(trees[0], 2) == [(26, 9, -0.5), (18, 4, 0.5)]
    assert R.pv_walk(trees[1], 8) == [(19, 7, 0.5), (64, 6, -0.125)]  # first of the tie; stops at the 0-visit child
    assert R.pv_walk(trees[2], 8) == []


def test_record_assembly_against_the_pv_reference():
    from othello_mcts import analysis as AN

    trees, v, q = _hand_rows()
    a = AN.empty_analysis(5, 4)
    a.terminal[1] = True
    a.margin[1] = -6
    rows = [0, 2, 4]  # inputs 1 and 3 were terminal / are left alone
    AN.fill_rows(a, rows, torch.from_numpy(v), torch.from_numpy(q), _pv_tensors(trees, 4))
    recs = a.records()
    assert len(recs) == 5 and len(a) == 5
    import json

    json.dumps(recs)
    for row, tree, vi, qi in zip(rows, trees, v, q):
        line = R.pv_walk(tree, 4)
        r = recs[row]
        assert r["pv"] == [x[0] for x in line] and r["pv_visits"] == [x[1] for x in line]
        assert r["pv_q"] == [x[2] for x in line]
        assert r["best_action"] == (line[0][0] if line else -1)
        assert r["visits"] == int(vi.sum())
        assert r["children"] == [{"action": k, "visits": int(vi[k]), "q": float(qi[k])} for k in range(65) if vi[k] > 0]
        want = float(np.float32((vi.astype(np.float64) * qi.astype(np.float64)).sum() / max(1, int(vi.sum()))))
        assert r["value"] == want and not r["terminal"] and "margin" not in r
    assert int(a.best_action[0]) == 26 and int(a.best_action[2]) == 19 and int(a.best_action[4]) == -1
    assert recs[1] == {"terminal": True, "best_action": -1, "value": 0.0, "visits": 0, "children": [], "pv": [],
                       "pv_visits": [], "pv_q": [], "margin": -6}
    assert recs[3]["best_action"] == -1 and recs[3]["pv"] == [] and not recs[3]["terminal"]


def test_history_packing():
    from othello_mcts import analysis as AN

    cs = chains()
    c = cs[80]
    lists = [[(p.player, p.p1, p.p2) for p in c[1:4]], [], [(p.player, p.p1, p.p2) for p in c[1:2]]]
    h, n = AN.pack_history(lists, 3)
    assert h.shape == (3, 3, 5) and n.tolist() == [3, 0, 1]
    assert int(h[0, 2, 1]) & (2**64 - 1) == c[3].p1 and int(h[2, 0, 2]) & (2**64 - 1) == c[1].p2
    assert h[1].abs().sum() == 0 and h[2, 1:].abs().sum() == 0
    h2, n2 = AN.pack_history(h, 3)
    assert torch.equal(h2, h) and n2.tolist() == [3, 3, 3]
    with pytest.raises(ValueError):
        AN.pack_history([[(1, 0, 0)] * 16], 1)
    with pytest.raises(ValueError):
        AN.pack_history(lists, 2)
