"""Forced playouts and policy target pruning on the GPU against
the Python reference tests/forced_ref.py (pinned to the oracle by
tests/test_cpu_forced_playouts.py) and, on the native path, against the host
pruning rule."""

import numpy as np
import pytest
import torch

import forced_ref as R
import oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
FIN_FAST = 128
K = R.K


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _cpu(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _callback(stub):
    def nn(features):
        p, v = stub(features.cpu().numpy())
        return {"policy": torch.from_numpy(p), "value": torch.from_numpy(v)}

    return nn


def _engine(seed, G, shape, k=K, prune=True, cap=None):
    import othello_mcts as om

    b = om.BatchedMCTS(G, seed=seed, node_capacity=1 << 16, **shape)
    if k is not None:
        b.set_forced_playouts(k, prune_targets=prune)
    if cap is not None:
        b.set_playout_cap(*cap)
    return b


def _check_root(b, twins, tag):
    """root_stats, root_priors and the event count of every game against its
    reference, by action; entries that are no child hold 0."""
    visits, q = (x.cpu().numpy() for x in b.root_stats())
    priors = b.root_priors().cpu().numpy()
    for g, t in enumerate(twins):
        r = t.r
        acts = O.legal_actions(r.position())
        rest = np.setdiff1d(np.arange(65), acts)
        if r.nch[r.root] == 0:  # (an unsearched root has no children yet)
            acts, rest = [], np.arange(65)
        assert list(visits[g][acts]) == r.visit_counts(), (tag, g)
        assert np.array_equal(_bits(q[g][acts]), _bits(r.mean_action_values())), (tag, g)
        assert np.array_equal(_bits(priors[g][acts]), _bits(r.priors())), (tag, g)
        assert not visits[g][rest].any() and not priors[g][rest].any() and not q[g][rest].any()
        assert b.engine.game_event(g) == r.events(), (tag, g)
        assert b.root_info(g)["visit_count"] == r.root_visit_count()


def _run_case(name, prefix=(), plies=None, prune=True):
    """A case of forced_ref.CASES on the callback path, move by move."""
    seed, G, n_plies, _, shape, cap = R.CASES[name]
    plies = plies or n_plies
    keys, twins, full, stub = R.case_twins(name)
    if prefix:
        twins = [R.Twin(k, shape, prefix=prefix) for k in keys]
    b = _engine(seed, G, shape, prune=prune, cap=cap)
    assert [b.engine.game_key(g) for g in range(G)] == keys
    for a in prefix:
        b.apply_actions(torch.full((G,), a, dtype=torch.int32))
    nn = _callback(stub)
    C = 1 + 2 * shape["history_size"]
    b._targets_f = torch.empty((G, 8, C, 8, 8), dtype=torch.float32, device=DEV)
    b._targets_p = torch.empty((G, 8, 65), dtype=torch.float32, device=DEV)
    guard = R.Guard()
    widths = []
    for ply in range(plies):
        for g, t in enumerate(twins):
            t.search(stub, guard, None if full[g, ply] else cap[1])
        b.search(nn)
        _check_root(b, twins, (name, ply))
        widths.append([t.r.nch[t.r.root] for t in twins])
        b._targets_f.fill_(float("nan"))
        b._targets_p.fill_(float("nan"))
        out = _cpu(b.selfplay_move(emit_targets=True))
        for g, t in enumerate(twins):
            fin = int(out["finished"][g])
            assert fin & 0x7F == 0, (name, ply, g, fin)
            if full[g, ply]:
                f, p = t.r.self_play_data(prune_k=K if prune else None)
                assert not fin & FIN_FAST
                assert np.array_equal(out["features"][g], f), (name, ply, g)
                assert np.array_equal(_bits(out["policy"][g]), _bits(p)), (name, ply, g)
            else:
                assert fin & FIN_FAST
                assert np.isnan(out["features"][g]).all() and np.isnan(out["policy"][g]).all()
            t.engine_move(out["actions"][g])
    return guard, full, np.array(widths)


# ---------------------------------------------------- 1.-3. the callback path
def test_forced_search_and_pruned_targets_equal_the_reference():
    """G = 8, T = 2, B = 8, H = 4, S = 64, eps 0.25, k = 2, 14 plies."""
    guard, _, _ = _run_case("noise")
    guard.check()


def test_forcing_without_noise_and_pruning_that_zeroes_children():
    """T = 1, B = 8, eps 0: the stored priors are the selection's."""
    guard, _, _ = _run_case("plain")
    guard.check(zeroed=True)


def test_forced_search_with_the_asymmetric_stub():
    guard, _, _ = _run_case("asym")
    guard.check()


def test_forcing_under_a_playout_cap_skips_fast_searches():
    """cap (0.5, 16): the reference forces only the full searches; fast moves
    carry bit 7 and write nothing (checked in _run_case)."""
    guard, full, _ = _run_case("cap")
    assert full.any() and (~full).any()
    assert (~full[:, :-1] & full[:, 1:]).any()  # a full search on a tree a fast one grew
    guard.check()


# ------------------------------------------------------ 5. wide and narrow roots
def test_a_root_with_seventeen_children():
    """Every game starts at a root with 17 legal moves: the selection's scan
    and argmax cross DPP rows, and the forced child of the lowest index wins."""
    guard, _, widths = _run_case("noise", prefix=R.WIDE_PREFIX, plies=3)
    assert (widths[0] >= 17).all()
    assert guard.changed > 0 and guard.pruned > 0


def test_a_root_whose_mover_must_pass():
    """One child, taken without scoring: nothing is forced, nothing pruned, the
    target is the pass."""
    guard, _, widths = _run_case("noise", prefix=R.PASS_PREFIX, plies=3)
    assert (widths[0] == 1).all()


# ------------------------------------------------------------- 4. native path
SHAPE_NATIVE = dict(history_size=2, num_simulations=32, num_threads=2, batch_size=8)
G_NATIVE, SEED_NATIVE, MOVES_NATIVE = 16, 5, 12


@pytest.fixture(scope="module")
def net():
    import othello_mcts as om
    from othello_mcts.synthetic import alphazero_state_dict

    return om.NativeNet(alphazero_state_dict(4, 5, 128, 1, 32), device=0)


def _children(info):
    legal = info["legal_moves"]
    if info["num_children"] == 0:
        return []
    return [s for s in range(64) if (legal >> (63 - s)) & 1] or [64]


def _expected_policy(b, g, prune_k):
    """The 8-fold policy target of game g's root from the public queries."""
    import othello_mcts as om

    info = b.root_info(g)
    acts = _children(info)
    visits, q = (x[g].cpu().numpy() for x in b.root_stats())
    priors = b.root_priors()[g].cpu().numpy()
    n = visits[acts].astype(np.int32)
    if prune_k is not None:
        n = om.prune_visit_counts(info["visit_count"], n, q[acts], priors[acts], b.config.c_puct_base,
                                  b.config.c_puct_init, prune_k)
    s = np.float32(max(int(n.sum()), 1))
    pol = np.zeros((8, 65), np.float32)
    for t in range(8):
        for a, x in zip(acts, n):
            pol[t, O.transform_action(a, t)] = np.float32(x) / s
    return pol, visits[acts], n


@pytest.fixture(scope="module")
def move_by_move(net):
    """12 x (search(net) + selfplay_move) with k = 2 and pruning; every recorded
    policy is checked against the host rule on the way. Computed once."""
    b = _engine(SEED_NATIVE, G_NATIVE, SHAPE_NATIVE)
    moves, pruned, zeroed = [], 0, 0
    for _ in range(MOVES_NATIVE):
        b.search(net)
        want = [_expected_policy(b, g, K) for g in range(G_NATIVE)]
        out = {k: v.copy() for k, v in _cpu(b.selfplay_move(emit_targets=True)).items()}
        for g, (pol, raw, n) in enumerate(want):
            assert out["actions"][g] >= 0 and out["finished"][g] & 0xFC == 0
            assert np.array_equal(_bits(out["policy"][g]), _bits(pol)), g
            pruned += bool((n < raw).any())
            zeroed += int(((n == 0) & (raw > 0)).sum())
        moves.append(out)
    assert 2 * pruned >= G_NATIVE * MOVES_NATIVE and zeroed > 0, (pruned, zeroed)
    return {k: np.stack([m[k] for m in moves]) for k in moves[0]}


def test_native_targets_equal_the_host_rule_on_the_queried_root(move_by_move):
    assert move_by_move["policy"].shape == (MOVES_NATIVE, G_NATIVE, 8, 65)
    sums = move_by_move["policy"].sum(-1)
    assert np.allclose(sums, 1.0, atol=1e-5)


@pytest.mark.parametrize("free_running", [True, False])
def test_selfplay_steps_equals_move_by_move(net, move_by_move, free_running):
    b = _engine(SEED_NATIVE, G_NATIVE, SHAPE_NATIVE)
    b.engine.set_free_running(free_running)
    out = _cpu(b.selfplay_steps(net, MOVES_NATIVE, emit_targets=True, keep_all=True))
    for k in ("actions", "finished", "features"):
        assert np.array_equal(out[k], move_by_move[k]), k
    assert np.array_equal(_bits(out["policy"]), _bits(move_by_move["policy"]))


# ---------------------------------------------------------------- 6. off is off
def test_switched_off_again_is_an_engine_that_never_had_it(net, move_by_move):
    plain = _engine(SEED_NATIVE, G_NATIVE, SHAPE_NATIVE, k=None)
    again = _engine(SEED_NATIVE, G_NATIVE, SHAPE_NATIVE, k=2.0)
    again.set_forced_playouts(None)
    a = _cpu(plain.selfplay_steps(net, 6, emit_targets=True, keep_all=True))
    c = _cpu(again.selfplay_steps(net, 6, emit_targets=True, keep_all=True))
    for k in a:
        assert np.array_equal(a[k].view(np.uint32), c[k].view(np.uint32)), k
    # and the feature does change this run
    assert not np.array_equal(a["policy"], move_by_move["policy"][:6])


def test_without_pruning_the_targets_are_the_forced_searchs_raw_counts(net, move_by_move):
    b = _engine(SEED_NATIVE, G_NATIVE, SHAPE_NATIVE, prune=False)
    differs = 0
    for i in range(4):
        b.search(net)
        want = [_expected_policy(b, g, None)[0] for g in range(G_NATIVE)]
        out = _cpu(b.selfplay_move(emit_targets=True))
        # the same forced search as the pruning run: same moves, other targets
        assert np.array_equal(out["actions"], move_by_move["actions"][i])
        for g in range(G_NATIVE):
            assert np.array_equal(_bits(out["policy"][g]), _bits(want[g])), (i, g)
        differs += int((out["policy"] != move_by_move["policy"][i]).any())
    assert differs > 0


# ------------------------------------------------------------- 7. the consumers
def test_arena_rejects_an_engine_with_forced_playouts():
    import othello_mcts as om

    a = _engine(1, 4, SHAPE_NATIVE, k=None)
    c = _engine(2, 4, SHAPE_NATIVE, k=2.0)
    with pytest.raises(ValueError, match="forced playouts"):
        om.Arena(a, c).reset()
    c.set_forced_playouts(None)
    om.Arena(a, c).reset()


def test_replay_buffer_stores_the_pruned_rows(net):
    """ReplayBuffer.add(out) then gather: what the numpy restatement
    (tests/replay_ref.py) holds after the same pruned outputs, bit for bit, and
    the first stored position's 8 rows are the engine's own pruned targets."""
    import othello_mcts as om
    import replay_ref

    G, H = G_NATIVE, SHAPE_NATIVE["history_size"]
    b = _engine(SEED_NATIVE, G, SHAPE_NATIVE)
    b.random_openings(52, seed=9)  # late openings: games finish within the calls
    buf = om.ReplayBuffer(G, H, capacity=1 << 10, device=DEV)
    ref = replay_ref.ReplayRef(G, H, 1 << 10)
    first = None  # the 8 target rows of the first position the ring receives
    slice0 = None
    for _ in range(3):
        out = b.selfplay_steps(net, 12, opening_moves=52, emit_targets=True, keep_all=True)
        buf.add(out)
        o = _cpu(out)
        ref.add(o)
        if slice0 is None:
            assert (o["actions"][0] >= 0).all()
            slice0 = o["policy"][0].copy()  # every game's first staged move
        done = np.argwhere(o["finished"] & 3)
        if first is None and len(done):
            # games commit move by move, in ascending game order within a move
            first = slice0[min((int(i), int(g)) for i, g in done)[1]]
    buf.check()
    assert first is not None and buf.size == ref.size > 0
    f, p, v = buf.gather(torch.arange(8 * buf.size))
    rf, rp, rv = ref.gather(np.arange(8 * ref.size))
    assert np.array_equal(_bits(p.cpu().numpy()), _bits(rp))
    assert np.array_equal(f.cpu().numpy().reshape(rf.shape), rf)
    assert np.array_equal(_bits(p[:8].cpu().numpy()), _bits(first))
