"""Exact leaf values on the GPU: the solve kernel's path against
the host rule, the callback path against the Python reference
tests/exact_leaves_ref.py (pinned to the oracle by
tests/test_cpu_exact_leaves.py), and the native schedules against the callback
path."""

import functools

import numpy as np
import pytest
import torch

import asym_stub as A
import exact_leaves_ref as X
import forced_ref as R
import oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F = np.float32
NONE = -128


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _cpu(out):
    return {k: v.cpu().numpy().copy() for k, v in out.items()}


def _callback(stub):
    def nn(features):
        p, v = stub(features.cpu().numpy())
        return {"policy": torch.from_numpy(p), "value": torch.from_numpy(v)}

    return nn


def _engine(seed, G, E, **kw):
    import othello_mcts as om

    kw.setdefault("history_size", 4)
    b = om.BatchedMCTS(G, seed=seed, node_capacity=1 << 16, **kw)
    if E is not None:
        b.set_exact_leaves(E)
    return b


def _play(b, actions):
    for a in actions:
        b.apply_actions(torch.full((b.num_games,), int(a), dtype=torch.int32))


# ------------------------------------------------------ 1. the kernel's solving path
@pytest.mark.parametrize("empties", range(1, 11))
def test_the_solve_kernel_equals_the_host_rule(empties):
    """256 random-play positions at this many empties: sign and node count."""
    import othello_mcts as om
    from othello_mcts.endgame import random_play_positions

    pos = random_play_positions(empties, 256, seed=1000 + empties)
    host = [om.exact_leaf_value(p, empties, return_nodes=True) for p in pos]
    sign, nodes = om.exact_leaf_values(pos, empties, return_nodes=True)
    assert sign.cpu().tolist() == [s for s, _ in host]
    assert nodes.cpu().tolist() == [n for _, n in host]
    assert {s for s, _ in host} <= {-1, 0, 1}
    if empties > 1:  # above E: no exact leaf, nothing searched
        sign, nodes = om.exact_leaf_values(pos[:64], empties - 1, return_nodes=True)
        assert set(sign.cpu().tolist()) == {NONE} and not nodes.cpu().any()


def test_the_solve_kernel_on_pass_and_terminal_positions():
    """Positions whose mover must pass (one root action, the pass), terminal
    ones (no value), and a tail that does not fill the last wave."""
    import random

    import othello_mcts as om

    rng, passes, ends = random.Random(9), [], []
    while len(passes) < 21 or len(ends) < 6:
        p = om.Position.initial_position()
        while not p.is_terminal():
            acts = p.legal_actions()
            if acts == [64] and 64 - bin(p.player1_discs() | p.player2_discs()).count("1") <= 10:
                passes.append(p)
            p = p.apply_action(acts[rng.randrange(len(acts))])
        ends.append(p)
    pos = passes[:21] + ends[:6]  # 27 positions: 6 full waves of 4 and 3 more
    host = [om.exact_leaf_value(p, 10, return_nodes=True) for p in pos]
    assert all(s is not None for s, _ in host[:21]) and all(s is None for s, _ in host[21:])
    sign, nodes = om.exact_leaf_values(pos, 10, return_nodes=True)
    assert sign.cpu().tolist() == [NONE if s is None else s for s, _ in host]
    assert nodes.cpu().tolist() == [n for _, n in host]
    assert om.exact_leaf_values([], 4).numel() == 0


# ------------------------------------------------------------ 2. the callback path
def _check_roots(b, refs, live, tag):
    visits, q = (x.cpu().numpy() for x in b.root_stats())
    for g, r in enumerate(refs):
        if not live[g]:
            continue
        acts = O.legal_actions(r.position())
        assert list(visits[g][acts]) == r.visit_counts(), (tag, g)
        assert np.array_equal(_bits(q[g][acts]), _bits(r.mean_action_values())), (tag, g)
        assert b.engine.game_event(g) == r.events(), (tag, g)
        assert b.root_info(g)["visit_count"] == r.root_visit_count(), (tag, g)
        d = b.self_play_data(g)
        f, p = r.self_play_data()
        assert np.array_equal(np.stack([x.numpy() for x in d["features"]]), f), (tag, g)
        assert np.array_equal(_bits(np.stack([x.numpy() for x in d["policy"]])), _bits(p)), (tag, g)


def _run_fixture(name, stub_name, G=4, seed=21):
    """A fixture of exact_leaves_ref.FIXTURES on G games (the same prefix, each
    game its own key and so its own root noise), move by move with tree reuse;
    the moves are the reference's (the first most visited child)."""
    fseed, start, E, shape, sims, plies = X.FIXTURES[name]
    stub = R.stub_of(stub_name)
    b = _engine(seed, G, E, num_simulations=sims, dirichlet_epsilon=0.25, **X.SHAPES[shape])
    keys = [A.game_key(seed, g) for g in range(G)]
    assert [b.engine.game_key(g) for g in range(G)] == keys
    hits: set = set()
    refs = [X.fixture_game(name, key=k, hits=hits)[0] for k in keys]
    _play(b, X.play_prefix(fseed, start))
    nn = _callback(stub)
    searched = 0
    for ply in range(plies):
        live = [r.position().player != 0 for r in refs]
        if not any(live):
            break
        b.set_active(live)
        evals0 = sum(r.evals for r in refs)
        for g, r in enumerate(refs):
            if live[g]:
                r.search(stub)
        sims_e, evals_e = b.search(nn)
        searched += sum(live)
        assert evals_e == sum(r.evals for r in refs) - evals0, (name, ply)
        assert sims_e == sum(live) * -(-sims // (refs[0].T * refs[0].B)) * refs[0].T * refs[0].B
        _check_roots(b, refs, live, (name, ply))
        want = {k: sum(r.counters()[k] for r in refs) for k in ("solves", "hits", "nodes")}
        assert b.exact_leaf_counters() == want, (name, ply)
        actions = []
        for g, r in enumerate(refs):
            a = O.legal_actions(r.position())[int(np.argmax(r.visit_counts()))] if live[g] else -1
            actions.append(a)
            if live[g]:
                r.apply_action(a)
        b.apply_actions(torch.tensor(actions, dtype=torch.int32))
    assert searched >= 2 * G and "pending" in hits and sum(r.solves for r in refs) > 0
    return hits


@pytest.mark.parametrize("name", ["e1", "e4", "e6"])
def test_callback_search_equals_the_reference(name):
    """The equivariant stub: visit counts, Q bits, 8-fold targets, the events,
    evals and the three counters, ply by ply."""
    _run_fixture(name, "equivariant")


def test_callback_search_with_the_asymmetric_stub():
    hits = _run_fixture("e4_wide", "asymmetric")
    assert "solved_hit" in hits


def test_leaf_flags_report_exact_leaves_as_rows_without_an_evaluation():
    """The step API: after a select, a row that ended at an exact leaf carries
    flag 0 like a terminal one. A root with E + 1 empties and its children
    expanded: every later row of that search is an exact or terminal leaf."""
    E = 4
    b = _engine(3, 2, E, num_simulations=16, num_threads=1, batch_size=4, dirichlet_epsilon=0.0)
    _play(b, _root_prefix(E + 1, 0))
    b._stream()
    steps = b.engine.search_begin()
    feat = torch.empty((b.rows_per_step, 9, 8, 8), dtype=torch.float32, device=DEV)
    pol = torch.full((b.rows_per_step, 65), 1.0 / 65, dtype=torch.float32, device=DEV)
    val = torch.zeros(b.rows_per_step, dtype=torch.float32, device=DEV)
    seen = []
    for _ in range(steps):
        b.engine.select()
        seen.append(b.engine.leaf_flags().copy())
        b.engine.features(feat.data_ptr(), 0, b.rows_per_step)
        b.engine.set_evaluation(pol.data_ptr(), val.data_ptr(), 0, b.rows_per_step)
    b.engine.backup()
    assert seen[0].all()  # the unexpanded root, four times per game
    assert not np.concatenate(seen[1:]).any()
    c = b.exact_leaf_counters()
    assert c["solves"] > 0 and c["solves"] + c["hits"] <= 2 * 12


# ------------------------------------- 3. a root with at most E + 1 empties, fresh tree
@functools.lru_cache(maxsize=None)
def _root_prefix(empties, skip):
    """A random-play prefix to a root with this many empties whose mover has a move."""
    seed = 40
    while True:
        acts = X.play_prefix(seed, empties)
        p = O.initial_position()
        for a in acts:
            p = O.apply_action(p, a)
        if X.empties(p) == empties and O.legal_actions(p) != [64]:
            if skip == 0:
                return acts
            skip -= 1
        seed += 1


@pytest.fixture(scope="module")
def net():
    import othello_mcts as om
    from othello_mcts.synthetic import alphazero_state_dict

    return om.NativeNet(alphazero_state_dict(4, 9, 128, 1, 32), device=0)


@pytest.mark.parametrize("E", [3, 6])
def test_a_root_just_above_the_threshold_is_searched_with_one_evaluation(net, E):
    """Every child of a root with E + 1 empties is an exact leaf or terminal:
    the search evaluates the root and nothing else, and every visited child's
    mean action value is minus the host sign of that child, bit for bit."""
    import othello_mcts as om

    G = 4
    b = _engine(8, G, E, num_simulations=64, num_threads=1, batch_size=1, dirichlet_epsilon=0.25)
    roots = []
    for g in range(G):
        p = O.initial_position()
        for a in _root_prefix(E + 1, g):
            b.apply_action(g, int(a))
            p = O.apply_action(p, a)
        roots.append(p)
    sims, evals = b.search(net)
    assert (sims, evals) == (64 * G, G)
    visits, q = (x.cpu().numpy() for x in b.root_stats())
    exact_children = 0
    for g, p in enumerate(roots):
        acts = O.legal_actions(p)
        assert int(visits[g][acts].sum()) == 63
        for a in acts:
            if visits[g][a] == 0:
                continue
            c = O.apply_action(p, a)
            if c.player == 0:
                mine, theirs = (c.p1, c.p2) if p.player == 1 else (c.p2, c.p1)
                want = F(np.sign(bin(mine).count("1") - bin(theirs).count("1")))
            else:
                s = om.exact_leaf_value((c.player, c.p1, c.p2), E)
                assert s is not None
                want = F(-s) if s else F(0.0)
                exact_children += 1
            assert _bits(q[g][a]) == _bits(want), (g, a, q[g][a], want)
    c = b.exact_leaf_counters()
    assert c["solves"] == exact_children  # one row at a time: each visited leaf solved once
    assert c["solves"] + c["hits"] <= 63 * G and c["nodes"] >= c["solves"]


# --------------------------------------------- 4. native search equals the callback path
SHAPE_NATIVE = dict(num_simulations=64, num_threads=2, batch_size=8, dirichlet_epsilon=0.25)
E_NATIVE, MOVES_NATIVE, START_NATIVE = 6, 6, 12


def _late_engine(G, E, seed=17, start=START_NATIVE, **kw):
    b = _engine(seed, G, E, **{**SHAPE_NATIVE, **kw})
    _play(b, X.play_prefix(7, start))
    return b


def _record(b):
    sims, evals = b.engine.work_counters()
    return {"evals": evals, "sims": sims, **b.exact_leaf_counters()}


def _move_by_move(b, evaluator, moves, **kw):
    outs = []
    for _ in range(moves):
        b.search(evaluator)
        outs.append(_cpu(b.selfplay_move(emit_targets=True, **kw)))
    return {k: np.stack([o[k] for o in outs]) for k in outs[0]}, _record(b)


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


@pytest.fixture(scope="module")
def callback_run(net):
    """8 games from 12 empties, E = 6, 6 x (search + selfplay_move) with the
    native net called as an external evaluator. Computed once."""
    out, rec = _move_by_move(_late_engine(8, E_NATIVE), lambda f: net(f), MOVES_NATIVE)
    assert rec["solves"] > 0 and rec["hits"] > 0
    return out, rec


def test_native_search_equals_the_callback_path(net, callback_run):
    out, rec = _move_by_move(_late_engine(8, E_NATIVE), net, MOVES_NATIVE)
    _same(out, callback_run[0])
    assert rec == callback_run[1]


@pytest.mark.parametrize("free_running", [True, False])
def test_selfplay_steps_equals_move_by_move(net, callback_run, free_running):
    b = _late_engine(8, E_NATIVE)
    b.engine.set_free_running(free_running)
    out = _cpu(b.selfplay_steps(net, MOVES_NATIVE, emit_targets=True, keep_all=True))
    _same(out, callback_run[0])
    assert _record(b) == callback_run[1]


def test_two_pipeline_groups(net):
    """64 games: two pipeline groups, each with its own solve launches."""
    a = _late_engine(64, E_NATIVE)
    out, rec = _move_by_move(a, net, 3)
    for free_running in (True, False):
        b = _late_engine(64, E_NATIVE)
        b.engine.set_free_running(free_running)
        _same(_cpu(b.selfplay_steps(net, 3, emit_targets=True, keep_all=True)), out)
        assert _record(b) == rec
    assert rec["solves"] > 0


def test_with_a_playout_cap_and_adjudication(net):
    def make():
        b = _late_engine(8, E_NATIVE)
        b.set_playout_cap(0.5, 16)
        return b

    outs = []
    a = make()
    for _ in range(MOVES_NATIVE):
        a.search(net)
        outs.append(_cpu(a.selfplay_move(emit_targets=True, adjudicate_empties=8)))
    want = {k: np.stack([o[k] for o in outs]) for k in outs[0]}
    b = make()
    got = _cpu(b.selfplay_steps(net, MOVES_NATIVE, emit_targets=True, keep_all=True, adjudicate_empties=8))
    # (slices of moves that wrote no targets hold what the buffers held before)
    for k in ("actions", "finished", "margin"):
        assert np.array_equal(got[k], want[k]), k
    wrote = (want["finished"] & 128) == 0
    assert np.array_equal(got["policy"][wrote].view(np.uint32), want["policy"][wrote].view(np.uint32))
    assert _record(b) == _record(a) and _record(a)["solves"] > 0
    assert (want["finished"] & 128).any() and (want["finished"] & 32).any()  # fast moves and adjudicated games


def test_one_game_with_two_threads_runs_the_grouped_schedule(net):
    """G = 1, T = 2 would run the thread-split schedule; with exact leaves it
    runs the grouped one, with the callback path's results."""
    a, b = _late_engine(1, 8, start=10), _late_engine(1, 8, start=10)
    for _ in range(3):
        ra = a.search(lambda f: net(f))
        rb = b.search(net)
        assert ra == rb
        for x, y in zip(a.root_stats(), b.root_stats()):
            assert np.array_equal(x.cpu().numpy().view(np.uint32), y.cpu().numpy().view(np.uint32))
        act = a.root_stats()[0].argmax(1).to(torch.int32)  # (no event drawn: both streams stay in step)
        a.apply_actions(act)
        b.apply_actions(act)
    assert a.exact_leaf_counters() == b.exact_leaf_counters() and a.exact_leaf_counters()["solves"] > 0


# ------------------------------------------------------------------- 5. off is off
def test_switched_off_again_is_an_engine_that_never_had_it(net, callback_run):
    plain = _late_engine(8, None)
    again = _engine(17, 8, 4, **SHAPE_NATIVE)
    _play(again, X.play_prefix(7, START_NATIVE))
    again.search(net)  # a tree built under E = 4
    with pytest.raises(ValueError, match="exact leaves"):
        again.set_exact_leaves(None)
    with pytest.raises(ValueError, match="exact leaves"):
        again.set_exact_leaves(6)
    again.reset(0, seed=17)  # one game's reset does not lift the restriction
    with pytest.raises(ValueError, match="exact leaves"):
        again.set_exact_leaves(None)
    again.reset(seed=17)
    again.set_exact_leaves(None)
    plain.reset(seed=17)
    for b in (plain, again):
        _play(b, X.play_prefix(7, START_NATIVE))
    c0 = again.exact_leaf_counters()
    x = _cpu(plain.selfplay_steps(net, MOVES_NATIVE, emit_targets=True, keep_all=True))
    y = _cpu(again.selfplay_steps(net, MOVES_NATIVE, emit_targets=True, keep_all=True))
    _same(x, y)
    assert again.exact_leaf_counters() == c0
    assert plain.exact_leaf_counters() == {"solves": 0, "hits": 0, "nodes": 0}


def test_the_feature_changes_the_search(net, callback_run):
    """... and with the setting on the same games evaluate fewer rows."""
    plain = _late_engine(8, None)
    _, rec = _move_by_move(plain, net, MOVES_NATIVE)
    assert rec["solves"] == 0 and rec["evals"] > callback_run[1]["evals"]


def test_the_arena_rejects_an_engine_with_exact_leaves():
    import othello_mcts as om

    a = _engine(1, 4, None, **SHAPE_NATIVE)
    c = _engine(2, 4, 4, **SHAPE_NATIVE)
    with pytest.raises(ValueError, match="exact leaves"):
        om.Arena(a, c)
    arena = om.Arena(a, _engine(2, 4, None, **SHAPE_NATIVE))
    arena.b.engine.set_exact_leaves(4)  # behind the Python layer's back: the C layer rejects it
    with pytest.raises(ValueError, match="exact leaves"):
        arena.reset()
    arena.b.engine.set_exact_leaves(0)
    arena.reset()
