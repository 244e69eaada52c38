"""Playout cap randomization and the free-running call's work budget on the GPU
(DESIGN.md §17)."""

import numpy as np
import pytest
import torch

import oracle as O
import playout_cap_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

FIN_ADJ, FIN_FAST = 32, 128
SHAPE = dict(history_size=2, num_simulations=32, num_threads=2, batch_size=8)  # L = 16: 2 steps, fast 16 = 1 step
FAST, P = 16, 0.5


def _stub(features):
    p, v = O.equivariant_stub(features.cpu().numpy())
    return {"policy": torch.from_numpy(p), "value": torch.from_numpy(v)}


@pytest.fixture(scope="module")
def net():
    import othello_mcts as om
    from othello_mcts.synthetic import alphazero_state_dict

    return om.NativeNet(alphazero_state_dict(4, 5, 128, 1, 32), device=0)


def _engine(seed=5, G=16, cap=(P, FAST), **kw):
    import othello_mcts as om

    b = om.BatchedMCTS(G, seed=seed, node_capacity=1 << 15, **{**SHAPE, **kw})
    if cap is not None:
        b.set_playout_cap(*cap)
    return b


def _cpu(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


# ------------------------------------------------------------------ 1. oracle
def test_capped_searches_and_moves_match_the_oracle():
    """The callback path, move by move: per ply and game the oracle's budget is
    set from the mirrored draw; root visits, actions, and the targets of full
    moves equal the oracle's bit for bit; fast moves carry bit 7 and write no
    targets (a NaN sentinel survives)."""
    import othello_mcts as om

    G, H, plies = 16, 4, 18
    kw = dict(history_size=H, num_simulations=64, num_threads=2, batch_size=8, dirichlet_epsilon=0.25)
    b = om.BatchedMCTS(G, seed=41, node_capacity=1 << 16, **kw)
    b.set_playout_cap(0.5, 16)
    keys = [b.engine.game_key(g) for g in range(G)]
    refs = [R.BudgetedOracle(game_key=k, **kw) for k in keys]
    full = np.array([[R.is_full(k, ply, 0.5) for ply in range(plies)] for k in keys])
    # 18 plies from the initial position finish no game (60 empties)
    assert plies < 60
    assert full.any() and (~full).any()
    assert (~full[:, :-1] & full[:, 1:]).any(), "no full search right after a fast one"
    # target buffers of our own, so a NaN sentinel can be written before each move
    C = 1 + 2 * H
    b._targets_f = torch.empty((G, 8, C, 8, 8), dtype=torch.float32, device=DEV)
    b._targets_p = torch.empty((G, 8, 65), dtype=torch.float32, device=DEV)
    seen = {True: 0, False: 0}
    for ply in range(plies):
        for g, r in enumerate(refs):
            if full[g, ply]:
                r.set_full()
            else:
                r.set_fast(16)
        b.search(_stub)
        sims = [r.search(O.equivariant_stub) for r in refs]
        assert sims == [64 if f else 16 for f in full[:, ply]]
        visits = b.root_stats()[0].cpu().numpy()
        b._targets_f.fill_(float("nan"))
        b._targets_p.fill_(float("nan"))
        out = _cpu(b.selfplay_move(temperature_moves=12, temperature=1.0, opening_moves=0, emit_targets=True))
        for g, r in enumerate(refs):
            acts = O.legal_actions(r.position())
            np.testing.assert_array_equal(visits[g][acts], r.visit_counts(), err_msg=f"ply {ply} game {g} visits")
            a = r.selfplay_action(ply, 12, 1.0)
            assert out["actions"][g] == a, (ply, g)
            fin = int(out["finished"][g])
            assert fin & 0x7F == 0, (ply, g, fin)
            if full[g, ply]:
                f, p = r.self_play_data()
                assert not fin & FIN_FAST
                np.testing.assert_array_equal(out["features"][g], f, err_msg=f"ply {ply} game {g} features")
                np.testing.assert_array_equal(out["policy"][g], p, err_msg=f"ply {ply} game {g} policy")
            else:
                assert fin & FIN_FAST
                assert np.isnan(out["features"][g]).all() and np.isnan(out["policy"][g]).all()
            seen[bool(full[g, ply])] += 1
            r.apply_action(a)
    assert seen[True] > 0 and seen[False] > 0


# ----------------------------------------------------- 2. free == move by move
@pytest.fixture(scope="module")
def move_by_move(net):
    """12 x (search(net) + selfplay_move) under the cap: the reference run of
    tests 2 and 3, computed once."""
    b = _engine()
    moves = []
    for _ in range(12):
        b.search(net)
        moves.append({k: v.copy() for k, v in _cpu(b.selfplay_move(emit_targets=True)).items()})
    return {k: np.stack([m[k] for m in moves]) for k in moves[0]}


def _equal_where_recorded(out, ref, mask):
    """actions / finished everywhere in `mask`; targets where a full move was played"""
    assert (out["actions"][mask] == ref["actions"][mask]).all()
    assert (out["finished"][mask] == ref["finished"][mask]).all()
    rec = mask & (ref["actions"] >= 0) & ((ref["finished"] & (FIN_FAST | 4)) == 0)
    assert rec.any()
    assert np.array_equal(out["features"][rec], ref["features"][rec])
    assert np.array_equal(out["policy"][rec], ref["policy"][rec])


def test_free_running_equals_move_by_move_under_the_cap(net, move_by_move):
    b = _engine()
    out = _cpu(b.selfplay_steps(net, 12, emit_targets=True, keep_all=True))
    fast = (move_by_move["finished"] & FIN_FAST) != 0
    assert fast.any() and (~fast).any()
    _equal_where_recorded(out, move_by_move, np.ones_like(fast))


# ------------------------------------------------------------------ 3. budget
def test_budget_stops_each_game_at_its_own_move(net, move_by_move):
    """sim_budget = 128 over 12 slots: per game the played slots are a prefix,
    equal to the move-by-move run's first moves; the nominal sizes (16 after a
    fast search, 32 after a full one) reach the budget exactly at the prefix's
    last move. 128 / 16 = 8 moves at the most, so 12 slots are never the limit."""
    budget, slots = 128, 12
    b = _engine()
    out = _cpu(b.selfplay_steps(net, slots, emit_targets=True, keep_all=True, sim_budget=budget))
    played = out["actions"] >= 0
    n = played.sum(0)
    lengths = set()
    for g in range(played.shape[1]):
        k = int(n[g])
        assert played[:k, g].all() and not played[k:, g].any()
        assert (out["actions"][k:, g] == -1).all() and (out["finished"][k:, g] == 0).all()
        nominal = np.where(out["finished"][:k, g] & FIN_FAST, 16, 32)
        total = np.cumsum(nominal)
        assert 1 <= k <= 8
        assert total[-1] >= budget and (k == 1 or total[-2] < budget), (g, nominal)
        lengths.add(k)
    assert len(lengths) > 1  # games stop at different moves
    _equal_where_recorded(out, move_by_move, played)


# ------------------------------------------------------------------ 4. p = 1
def test_full_probability_one_is_the_cap_off(net):
    a = _engine(cap=None)
    c = _engine(cap=(1.0, FAST))
    oa = _cpu(a.selfplay_steps(net, 6, emit_targets=True, keep_all=True))
    oc = _cpu(c.selfplay_steps(net, 6, emit_targets=True, keep_all=True))
    for k in oa:
        assert np.array_equal(oa[k], oc[k]), k
    assert not (oc["finished"] & FIN_FAST).any()
    # and switching the cap off again restores the plain engine
    d = _engine()
    d.set_playout_cap()
    od = _cpu(d.selfplay_steps(net, 6, emit_targets=True, keep_all=True))
    for k in oa:
        assert np.array_equal(oa[k], od[k]), k


# --------------------------------------------------------------- 5. consumers
def test_replay_buffer_and_collector_skip_fast_moves(net):
    import othello_mcts as om
    from othello_mcts.selfplay import SelfPlayCollector

    G = 16
    b = _engine(seed=5)
    b.random_openings(40, seed=9)  # late openings: games finish within a few moves
    buf = om.ReplayBuffer(G, SHAPE["history_size"], capacity=1 << 12, device=DEV)
    col = SelfPlayCollector(G)
    samples = 0
    want = 0
    pending = np.zeros(G, np.int64)
    # 16 slots, 256 nominal simulations per game and call: 8 to 16 moves each
    for _ in range(6):
        out = b.selfplay_steps(net, 16, opening_moves=4, emit_targets=True, keep_all=True, sim_budget=256)
        buf.add(out)
        o = _cpu(out)
        for i in range(16):
            samples += len(col.add({k: v[i] for k, v in out.items()})["values"])
            rec = (o["actions"][i] >= 0) & ((o["finished"][i] & FIN_FAST) == 0)
            pending += rec
            done = (o["finished"][i] & 3) != 0
            want += int(pending[done].sum())
            pending[done] = 0
        assert ((o["finished"] & FIN_FAST) != 0).any()
    assert want > 0
    assert buf.size == want and samples == 8 * want
    buf.check()  # raises what the kernels flagged
    assert int(buf.counters[3]) == 0


# ------------------------------------------------------------- 6. adjudication
def test_budget_and_cap_with_adjudication(net):
    b = _engine(seed=5)
    b.random_openings(40, seed=9)
    fins, margins = [], []
    for _ in range(6):
        o = _cpu(b.selfplay_steps(net, 16, opening_moves=4, emit_targets=True, keep_all=True, sim_budget=256,
                                  adjudicate_empties=6))
        fins.append(o["finished"])
        margins.append(o["margin"])
        unplayed = o["actions"] < 0
        assert (o["finished"][unplayed] == 0).all()
        assert (o["margin"][unplayed] == np.iinfo(np.int32).min).all()
    fin, margin = np.concatenate(fins), np.concatenate(margins)
    adj = (fin & FIN_ADJ) != 0
    assert adj.any() and ((fin & FIN_FAST) != 0).any()
    assert ((fin[adj] & 3) != 0).all()  # every adjudicated game has its outcome
    assert (margin[adj] != np.iinfo(np.int32).min).all()


# ------------------------------------------------------------------ 7. errors
def test_errors(net):
    import othello_mcts as om

    b = _engine()
    with pytest.raises(ValueError, match="keep_all"):
        b.selfplay_steps(net, 4, keep_all=False, sim_budget=64)
    a = torch.empty(4 * 16, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="per_move_outputs"):
        b.engine.selfplay_steps_budget(net.handle, 4, 64, 12, 1.0, 0, False, False, a.data_ptr(), a.data_ptr(), 0, 0,
                                       0, False, 0)
    b.engine.set_free_running(False)
    with pytest.raises(ValueError, match="free-running"):
        b.selfplay_steps(net, 4, keep_all=True, sim_budget=64)
    one = om.BatchedMCTS(1, seed=1, node_capacity=1 << 12, **SHAPE)
    with pytest.raises(ValueError, match="thread-split"):
        one.set_playout_cap(0.5, 16)
    with pytest.raises(ValueError, match="free-running"):
        one.selfplay_steps(net, 4, keep_all=True, sim_budget=64)
    for bad in ((0.0, 16), (1.5, 16), (0.5, 0), (0.5, 33)):
        with pytest.raises(ValueError, match="Expected"):
            b.set_playout_cap(*bad)
    with pytest.raises(ValueError, match="together"):
        b.set_playout_cap(0.5)
