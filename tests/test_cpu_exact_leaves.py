"""Exact leaf values without a GPU: the Python reference
tests/exact_leaves_ref.py against the oracle with the setting off, the host
rule against ``solve_position``, the validation of the setters, and the branch
coverage of the fixtures the GPU tests run."""

import ctypes
import functools

import numpy as np
import pytest

import asym_stub as A
import exact_leaves_ref as X
import forced_ref as R
import oracle as O


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ------------------------------------------------- 1. the reference is a yardstick
SHAPES = {
    "T1B8": dict(num_threads=1, batch_size=8, history_size=2, num_simulations=64, dirichlet_epsilon=0.25),
    "T2B8": dict(num_threads=2, batch_size=8, history_size=4, num_simulations=64, dirichlet_epsilon=0.25),
}


@pytest.mark.parametrize("stub", ["equivariant", "asymmetric"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_reference_with_the_setting_off_equals_the_oracle(shape, stub):
    """E = 0 over a whole game from a late position (every ply down to the end,
    so the plies where the rule would act are covered), bit for bit."""
    kw, nn = SHAPES[shape], R.stub_of(stub)
    key = A.game_key(5, 2)
    o = O.OracleMCTS(game_key=key, **kw)
    r = X.ExactMCTS(max_empties=0, game_key=key, **kw)
    for a in X.play_prefix(5, 10):
        o.apply_action(int(a))
        r.apply_action(int(a))
    plies = 0
    while r.position().player != 0:
        assert o.search(nn) == r.search(nn)
        assert o.visit_counts() == r.visit_counts(), plies
        assert np.array_equal(_bits(o.mean_action_values()), _bits(r.mean_action_values())), plies
        assert (o.events(), o.node_count()) == (r.events(), r.node_count()), plies
        fo, po = o.self_play_data()
        fr, pr = r.self_play_data()
        assert np.array_equal(fo, fr) and np.array_equal(_bits(po), _bits(pr)), plies
        a = o.selfplay_action(plies, 2, 1.0)
        assert r.selfplay_action(plies, 2, 1.0) == a
        o.apply_action(a)
        r.apply_action(a)
        plies += 1
    assert plies >= 6
    assert r.counters() == {"solves": 0, "hits": 0, "nodes": 0} and not r.hits


# --------------------------------------------------------------- 2. the host rule
@functools.lru_cache(maxsize=None)
def _positions(empties: int, count: int = 24):
    import othello_mcts as om
    from othello_mcts.endgame import random_play_positions

    pos = random_play_positions(empties, count, seed=100 + empties)
    assert all(not p.is_terminal() for p in pos)
    return om, pos


@pytest.mark.parametrize("empties", range(1, 11))
def test_exact_leaf_value_is_the_sign_of_solve_position(empties):
    om, pos = _positions(empties)
    for p in pos:
        want = int(np.sign(om.solve_position(p, max_empties=empties)["score"]))
        value, nodes = om.exact_leaf_value(p, empties, return_nodes=True)
        assert value == want and nodes >= 1
        assert om.exact_leaf_value(p, 10) == want  # any E at or above the empties
        if empties > 1:
            assert om.exact_leaf_value(p, empties - 1) is None  # above E: no exact leaf


def test_exact_leaf_value_on_positions_whose_mover_must_pass():
    """Found in random play: the side to move has no move, the other side has."""
    import random

    import othello_mcts as om

    rng, found = random.Random(9), []
    while len(found) < 12:
        p = om.Position.initial_position()
        while not p.is_terminal():
            acts = p.legal_actions()
            e = 64 - bin(p.player1_discs() | p.player2_discs()).count("1")
            if acts == [64] and e <= 10:
                found.append(p)
            p = p.apply_action(acts[rng.randrange(len(acts))])
    for p in found:
        e = 64 - bin(p.player1_discs() | p.player2_discs()).count("1")
        assert om.exact_leaf_value(p, max(e, 1)) == int(np.sign(om.solve_position(p, max_empties=10)["score"]))


def test_exact_leaf_value_is_none_on_terminal_positions():
    import random

    import othello_mcts as om

    rng = random.Random(4)
    for _ in range(6):
        p = om.Position.initial_position()
        while not p.is_terminal():
            acts = p.legal_actions()
            p = p.apply_action(acts[rng.randrange(len(acts))])
        assert om.exact_leaf_value(p, 10) is None
        # ... whatever `player` says
        assert om.exact_leaf_value((1, p.player1_discs(), p.player2_discs()), 10) is None
    assert om.exact_leaf_value(om.Position.initial_position(), 10) is None


# ------------------------------------------------------------- 3. setter validation
@pytest.mark.parametrize("e", [-1, 11, 64])
def test_a_value_out_of_range_is_rejected_before_a_device_is_touched(e):
    import othello_mcts as om

    class NoDevice:
        @property
        def engine(self):
            raise AssertionError("the engine was touched")

    with pytest.raises(ValueError, match="max_empties"):
        om.BatchedMCTS.set_exact_leaves(NoDevice(), e)
    with pytest.raises(TypeError):
        om.BatchedMCTS.set_exact_leaves(NoDevice(), 4.0)
    with pytest.raises(ValueError, match="max_empties"):
        om.exact_leaf_value(om.Position.initial_position(), e)
    with pytest.raises(ValueError, match="max_empties"):
        om.exact_leaf_value(om.Position.initial_position(), 0)  # off is no value of the host rule


def test_the_c_rule_rejects_a_bad_value_and_a_bad_position():
    import capi_host as H

    raw = ctypes.CDLL(str(H.LIB_PATH))
    header = H.HEADER.read_text()
    for name in ("oamd_engine_set_exact_leaves", "oamd_engine_exact_leaf_counters", "oamd_engine_exact_leaf_faults",
                 "oamd_exact_leaf_sign", "oamd_exact_leaf_signs"):
        assert hasattr(raw, name), name
        assert name in header
    assert hasattr(raw, "oamd_exact_leaf_sign_nodes")  # the node count: the experimental header
    assert "oamd_exact_leaf_sign_nodes" in (H.HEADER.parent / "othello_mcts_amd_experimental.h").read_text()
    assert raw.oamd_abi_version() == 1

    class Pos(ctypes.Structure):
        _fields_ = [("player", ctypes.c_int32), ("reserved", ctypes.c_int32), ("p1", ctypes.c_uint64),
                    ("p2", ctypes.c_uint64), ("legal", ctypes.c_uint64), ("next_legal", ctypes.c_uint64)]

    fn = raw.oamd_exact_leaf_sign
    fn.argtypes = [ctypes.POINTER(Pos), ctypes.c_int32, ctypes.POINTER(ctypes.c_int32)]
    fn.restype = ctypes.c_int
    sign = ctypes.c_int32(7)
    # black to move fills the last square of a board it owns but for one white disc
    p = Pos(1, 0, ((1 << 64) - 1) & ~0b11, 0b10, 0, 0)
    assert fn(ctypes.byref(p), 1, ctypes.byref(sign)) == 0 and sign.value == 1
    assert fn(ctypes.byref(p), 0, ctypes.byref(sign)) != 0
    assert fn(ctypes.byref(p), 11, ctypes.byref(sign)) != 0
    bad = Pos(1, 0, 3, 1, 0, 0)  # overlapping discs
    assert fn(ctypes.byref(bad), 4, ctypes.byref(sign)) != 0


def test_the_python_setter_forwards_the_value_and_keeps_its_own_copy_in_step():
    """BatchedMCTS.set_exact_leaves on an engine stand-in that refuses a change
    the way the C layer does: the wrapper passes None as 0, and its own
    ``exact_leaves`` (what the Arena looks at) follows only a change the engine
    accepted. The rule itself (exact_setting_change_ok, the engine's
    exact_trees) needs an engine and is tested on the GPU
    (tests/test_gpu_exact_leaves.py test_switched_off_again...)."""
    import othello_mcts as om

    class Engine:  # the state the C engine keeps for the rule
        def __init__(self):
            self.value, self.trees = 0, False

        def set_exact_leaves(self, e):
            if e != self.value and self.trees:
                raise ValueError("exact leaves: the setting cannot change")
            self.value = e

    class Host:
        exact_leaves = 0

        def __init__(self):
            self.engine = Engine()

    h = Host()
    om.BatchedMCTS.set_exact_leaves(h, 4)
    assert (h.exact_leaves, h.engine.value) == (4, 4)
    h.engine.trees = True  # a search ran
    om.BatchedMCTS.set_exact_leaves(h, 4)  # the same value again is fine
    with pytest.raises(ValueError, match="cannot change"):
        om.BatchedMCTS.set_exact_leaves(h, 6)
    with pytest.raises(ValueError, match="cannot change"):
        om.BatchedMCTS.set_exact_leaves(h, None)
    assert h.exact_leaves == 4  # a refused change leaves the Python side as it was
    h.engine.trees = False  # every game was reset
    om.BatchedMCTS.set_exact_leaves(h, None)
    assert (h.exact_leaves, h.engine.value) == (0, 0)


def test_the_arena_rejects_an_engine_that_has_the_setting():
    import torch

    import othello_mcts as om

    class Fake:
        num_games, device = 2, torch.device("cpu")

        def __init__(self, e):
            self.exact_leaves = e

    with pytest.raises(ValueError, match="exact leaves"):
        om.Arena(Fake(0), Fake(4))
    with pytest.raises(ValueError, match="exact leaves"):
        om.Arena(Fake(6), Fake(0))
    arena = om.Arena(Fake(0), Fake(0))
    arena.b.exact_leaves = 4  # set after the arena was made: rejected at the next use
    with pytest.raises(ValueError, match="exact leaves"):
        arena._streams()
    assert not hasattr(om.MCTS, "set_exact_leaves")  # the drop-in gets no setter


# ------------------------------------------------------------ 4. fixture coverage
@functools.lru_cache(maxsize=None)
def _fixture_hits(name: str, stub: str) -> frozenset:
    hits: set = set()
    m = X.run_fixture_on_cpu(name, R.stub_of(stub), hits)
    c = m.counters()
    if "pending" in hits:
        assert c["solves"] > 0 and c["nodes"] >= c["solves"]
    return frozenset(hits)


def test_the_fixtures_cover_the_shapes_and_values_the_rule_asks_for():
    assert {X.FIXTURES[n][2] for n in X.FIXTURES} == {1, 4, 6}
    assert {X.FIXTURES[n][3] for n in X.FIXTURES} == {"1x4", "2x8", "2x16"}
    for name, (seed, start, E, shape, sims, plies) in X.FIXTURES.items():
        assert 8 <= start <= 12 and 64 <= sims <= 200
        m, _ = X.fixture_game(name)
        assert X.empties(m.position()) == start and m.position().player != 0


def test_every_branch_of_the_rule_is_hit_across_the_fixtures():
    hits = set()
    for name in X.FIXTURES:
        got = _fixture_hits(name, "equivariant")
        assert got, name  # a fixture that exercises nothing cannot pass
        hits |= got
    assert hits == set(X.BRANCHES), sorted(set(X.BRANCHES) - hits)


@pytest.mark.parametrize("name", list(X.FIXTURES))
def test_each_fixture_sees_the_feature(name):
    """Every fixture solves leaves, and its searches differ from the same game
    with the setting off (the twin run)."""
    hits: set = set()
    stub = R.stub_of("asymmetric")
    m, plies = X.fixture_game(name, hits=hits)
    seed, start, E, shape, sims, _ = X.FIXTURES[name]
    z = X.ExactMCTS(max_empties=0, history_size=4, num_simulations=sims, dirichlet_epsilon=0.25, game_key=0,
                    **X.SHAPES[shape])
    for a in X.play_prefix(seed, start):
        z.apply_action(int(a))
    changed = 0
    for _ in range(plies):
        if m.position().player == 0:
            break
        m.search(stub)
        z.search(stub)
        changed += m.visit_counts() != z.visit_counts() or m.evals != z.evals
        a = O.legal_actions(m.position())[int(np.argmax(m.visit_counts()))]
        m.apply_action(a)
        z.apply_action(a)
    assert "pending" in hits and m.solves > 0 and changed > 0
    assert m.evals < z.evals  # exact leaves took rows from the net
