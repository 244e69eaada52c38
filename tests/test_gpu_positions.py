"""Search from given positions on the GPU: set_positions against
the oracle's reset_chain, against the native path and against a game replayed
move by move; the mask and the rejections; the device's principal variation
against the slow way; analyze; and the two engine calls through ctypes.

Common shape: G = 8 games, H = 4, T = 2 x B = 4, 64 simulations, eps = 0.25, the
callback path with the asymmetric evaluator (the equivariant stub cannot see a
misplaced history plane). The roots are tests/positions_ref.py's: two chains
shorter than H, two pass positions, four mid-game chains."""

import ctypes
import functools

import numpy as np
import pytest
import torch

import asym_stub as A
import oracle as O
import positions_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
G = 8
KW = dict(history_size=4, num_simulations=64, num_threads=2, batch_size=4, dirichlet_epsilon=0.25)
MASK64 = (1 << 64) - 1


@pytest.fixture(scope="module")
def om():
    import othello_mcts

    assert othello_mcts.device_count() >= 1
    return othello_mcts


def _t(fn):
    def nn(features):
        p, v = fn(features.cpu().numpy())
        return {"policy": torch.from_numpy(p), "value": torch.from_numpy(v)}

    return nn


ASYM = _t(A.asymmetric_stub)
UNIFORM = _t(O.uniform_stub)


@functools.lru_cache(maxsize=None)
def all_chains():
    return A.random_game_chains(40)


def root_chains():
    cs = all_chains()
    return [cs[i] for i in R.ROOT_INDICES]


def triple(p):
    return (p.player, p.p1, p.p2)


def history_of(chain):
    return [triple(p) for p in chain[1:16]]


def moves_of(chain):
    """The actions that lead from the initial position to chain[0]."""
    out = []
    for prev, nxt in zip(chain[:0:-1], chain[-2::-1]):
        new = (nxt.p1 | nxt.p2) & ~(prev.p1 | prev.p2)
        out.append(64 if new == 0 else 64 - new.bit_length())
    return out


def engine(om, seed=77, **over):
    return om.BatchedMCTS(G, seed=seed, node_capacity=1 << 14, **{**KW, **over})


def by_action(position, values, fill=0):
    out = [fill] * 65
    for a, v in zip(O.legal_actions(position), values):
        out[a] = v
    return out


def assert_game_equals_oracle(b, g, ref, tag):
    info = b.root_info(g)
    assert info["visit_counts"] == ref.visit_counts(), tag
    np.testing.assert_allclose(np.array(info["mean_action_values"], np.float32),
                               np.array(ref.mean_action_values(), np.float32), rtol=0, atol=1e-6, err_msg=str(tag))
    return info["visit_counts"]


# ------------------------------------------------------------ 1. oracle parity
@pytest.mark.parametrize("with_history", [True, False])
def test_set_positions_matches_the_oracles_reset_chain(om, with_history):
    """Per game the oracle started from the same chain with the same key: visits
    bit for bit and Q within 1e-6 after the first search and, after the best
    move, after a second one (tree reuse, hist[] moving past the given
    ancestors); the 8-fold targets as well. Without history the planes behind
    the root are zero, as orc_features leaves them for a chain of length 1."""
    chains = root_chains()
    keys = [A.game_key(4242, 100 + g) for g in range(G)]
    b = engine(om)
    b.set_positions([triple(c[0]) for c in chains], history=[history_of(c) for c in chains] if with_history else None,
                    keys=keys)
    refs = []
    for g, c in enumerate(chains):
        r = O.OracleMCTS(game_key=keys[g], **KW)
        r.reset_chain(c[:1 + min(15, len(c) - 1)] if with_history else c[:1])
        refs.append(r)
        assert b.engine.game_key(g) == keys[g]
        assert tuple(b.root_positions()[g].tolist()) == tuple(x - (1 << 64) if x >= 1 << 63 else x for x in
                                                              (c[0].player, c[0].p1, c[0].p2, c[0].legal, c[0].next_legal))
    for mv in range(2):
        sims, evals = b.search(ASYM)
        assert sims == G * 64 and 0 < evals <= sims
        acts = torch.full((G,), -1, dtype=torch.int32)
        for g, r in enumerate(refs):
            r.search(A.asymmetric_stub)
            vc = assert_game_equals_oracle(b, g, r, (with_history, mv, g))
            d = b.self_play_data(g)
            f, p = r.self_play_data()
            np.testing.assert_array_equal(torch.stack(d["features"]).numpy(), f, err_msg=str((mv, g)))
            np.testing.assert_array_equal(torch.stack(d["policy"]).numpy(), p, err_msg=str((mv, g)))
            a = O.legal_actions(r.position())[int(np.argmax(vc))]
            acts[g] = a
            r.apply_action(a)
        b.apply_actions(acts.to(DEV))
        if mv == 0:
            assert all(r.position().player != 0 for r in refs), "a root of the second search is terminal"


# ------------------------------------------------------- 2. native == callback
def test_native_search_after_set_positions_equals_the_callback_search(om):
    """The packed feature rows gathered from given ancestor nodes (native path)
    against the fp32 planes of the same nodes (callback path), same net."""
    from othello_mcts.synthetic import alphazero_state_dict

    net = om.NativeNet(alphazero_state_dict(7, 9, 128, 3, 64), device=0)
    chains = root_chains()
    a, b = engine(om, seed=21), engine(om, seed=21)
    for e in (a, b):
        e.set_positions([triple(c[0]) for c in chains], history=[history_of(c) for c in chains], seed=9)
    for mv in range(2):
        a.search(net)
        b.search(lambda f: net(f))
        va, qa = a.root_stats()
        vb, qb = b.root_stats()
        assert torch.equal(va, vb) and torch.equal(qa, qb), mv
        assert int(va.sum()) > 0
        best = va.argmax(1).to(torch.int32)
        a.apply_actions(best)
        b.apply_actions(best)


# --------------------------------------------------------- 3. set == replayed
@pytest.mark.parametrize("temperature_moves", [3, 21, 45])
def test_a_set_game_equals_the_game_replayed_move_by_move(om, temperature_moves):
    """Engine A replays each root's game with apply_actions from a reset; engine
    B is given the root, its last 15 positions and the move count. Searches,
    self_play_data and two self-play moves agree. The plies are 0, 2, 59, 59,
    20, 39, 37 and 44: temperature_moves = 3, 21 and 45 put the switch from
    sampling to argmax between the two moves of games 1, 4 and 7."""
    chains = root_chains()
    moves = [moves_of(c) for c in chains]
    assert [len(m) for m in moves] == [n - 1 for n in R.ROOT_LENGTHS]
    seed = 31337
    a, b = engine(om), engine(om)
    a.reset(-1, seed)
    b.reset(-1, seed)
    for k in range(max(len(m) for m in moves)):
        a.apply_actions(torch.tensor([m[k] if k < len(m) else -1 for m in moves], dtype=torch.int32, device=DEV))
    b.set_positions([triple(c[0]) for c in chains], history=[history_of(c) for c in chains],
                    ply=[len(m) for m in moves], seed=seed)
    assert torch.equal(a.root_positions(), b.root_positions())
    for g in range(G):
        assert a.engine.game_key(g) == b.engine.game_key(g)
    for mv in range(2):
        a.search(ASYM)
        b.search(ASYM)
        va, qa = a.root_stats()
        vb, qb = b.root_stats()
        assert torch.equal(va, vb) and torch.equal(qa, qb), mv
        for g in range(G):
            da, db = a.self_play_data(g), b.self_play_data(g)
            assert torch.equal(torch.stack(da["features"]), torch.stack(db["features"])), (mv, g)
            assert torch.equal(torch.stack(da["policy"]), torch.stack(db["policy"])), (mv, g)
        oa = a.selfplay_move(temperature_moves=temperature_moves, emit_targets=True)
        oa = {k: v.clone() for k, v in oa.items()}
        ob = b.selfplay_move(temperature_moves=temperature_moves, emit_targets=True)
        for k in ("actions", "finished", "features", "policy"):
            assert torch.equal(oa[k], ob[k]), (mv, k)
        assert bool((oa["actions"] >= 0).all())
        assert torch.equal(a.root_positions(), b.root_positions())


# ------------------------------------------------------ 4. mask and rejection
def test_mask_leaves_other_games_alone_and_rejections_are_named(om):
    chains = root_chains()
    b = engine(om)
    b.random_openings(6, seed=3)
    b.search(ASYM)
    v0, q0 = b.root_stats()
    p0 = b.root_positions()
    assert bool((v0.sum(1) > 0).all())
    b.set_positions([triple(chains[4][0]), triple(chains[2][0])], games=[1, 5])
    v1, q1 = b.root_stats()
    p1 = b.root_positions()
    others = [g for g in range(G) if g not in (1, 5)]
    assert torch.equal(v1[others], v0[others]) and torch.equal(q1[others], q0[others])
    assert torch.equal(p1[others], p0[others])
    assert int(v1[[1, 5]].abs().sum()) == 0
    for g, c in ((1, chains[4]), (5, chains[2])):
        assert [int(x) & MASK64 for x in p1[g, 1:].tolist()] == [c[0].p1, c[0].p2, c[0].legal, c[0].next_legal]
        assert int(p1[g, 0]) & 0xFFFFFFFF == c[0].player
    # one overlapping entry: named, its game untouched, its neighbour set
    good = chains[5][0]
    with pytest.raises(ValueError, match=r"entry 0 \(game 2\).*overlap"):
        b.set_positions([(1, good.p1 | 1 << 20, good.p2 | 1 << 20), triple(good)], games=[2, 3])
    v2, q2 = b.root_stats()
    p2 = b.root_positions()
    assert torch.equal(v2[2], v1[2]) and torch.equal(q2[2], q1[2]) and torch.equal(p2[2], p1[2])
    assert int(v2[3].abs().sum()) == 0
    assert [int(x) & MASK64 for x in p2[3, 1:3].tolist()] == [good.p1, good.p2]
    with pytest.raises(ValueError, match="player"):
        b.set_positions([(3, good.p1, good.p2)], games=[0])
    with pytest.raises(ValueError, match="history"):
        b.set_positions([triple(good)], history=[[(1, 3, 3)]], games=[0])
    with pytest.raises(ValueError, match="ply"):
        b.set_positions([triple(good)], ply=[-1], games=[0])
    v3, _ = b.root_stats()
    assert torch.equal(v3[0], v0[0])
    # the untouched games still search on from their trees
    b.search(ASYM)
    b.check_health()


# ------------------------------------------------------------------- 5. the PV
def slow_pv(b, g, max_len):
    """The line found through the public queries: argmax of the root's visits
    (the first action of equals), apply_action, again."""
    line = []
    while len(line) < max_len:
        info = b.root_info(g)
        vc = info["visit_counts"]
        if info["num_children"] == 0 or max(vc) <= 0:
            break
        k = int(np.argmax(vc))
        legal = info["legal_moves"]
        a = [s for s in range(64) if (legal >> (63 - s)) & 1][k] if legal else 64
        line.append((a, vc[k], np.float32(info["mean_action_values"][k])))
        b.apply_action(g, a)
    return line


@pytest.mark.parametrize("stub,sims", [("asym", 64), ("uniform", 16)])
def test_principal_variations_equal_the_line_found_the_slow_way(om, stub, sims):
    """With the uniform stub at 16 simulations ties are certain (asserted)."""
    nn = ASYM if stub == "asym" else UNIFORM
    chains = root_chains()
    a, b = engine(om, num_simulations=sims), engine(om, num_simulations=sims)
    for e in (a, b):
        e.set_positions([triple(c[0]) for c in chains], history=[history_of(c) for c in chains], seed=5)
    unsearched = a.principal_variations(8)
    assert int(unsearched["length"].abs().sum()) == 0 and bool((unsearched["actions"] == -1).all())
    a.search(nn)
    b.search(nn)
    va, _ = a.root_stats()
    assert torch.equal(va, b.root_stats()[0])
    pv = {k: v.cpu() for k, v in a.principal_variations(8).items()}
    pv2 = {k: v.cpu() for k, v in a.principal_variations(2).items()}
    ties = 0
    for g in range(G):
        line = slow_pv(b, g, 8)
        n = int(pv["length"][g])
        assert n == len(line) and n >= 1, (g, n, line)
        assert pv["actions"][g, :n].tolist() == [x[0] for x in line], g
        assert pv["visits"][g, :n].tolist() == [x[1] for x in line], g
        np.testing.assert_array_equal(pv["q"][g, :n].numpy(), np.array([x[2] for x in line], np.float32))
        assert bool((pv["actions"][g, n:] == -1).all()) and int(pv["visits"][g, n:].abs().sum()) == 0
        k = min(2, n)
        assert int(pv2["length"][g]) == k
        assert pv2["actions"][g, :k].tolist() == pv["actions"][g, :k].tolist()
        assert pv2["visits"][g, :k].tolist() == pv["visits"][g, :k].tolist()
        row = va[g].cpu()
        ties += int((row == row.max()).sum()) > 1
    if stub == "uniform":
        assert ties > 0
    # an inactive game reports no line
    a.set_active([g != 3 for g in range(G)])
    assert int(a.principal_variations(8)["length"][3]) == 0
    with pytest.raises(ValueError):
        a.principal_variations(0)
    with pytest.raises(ValueError):
        a.principal_variations(65)


# ---------------------------------------------------------------- 6. analyze
def test_analyze_does_not_depend_on_the_engine_size_and_equals_the_oracle(om):
    cs = all_chains()
    chains = root_chains() + [cs[150], cs[700]]
    final = cs[59][0]
    while final.player != 0:
        final = O.apply_action(final, O.legal_actions(final)[0])
    inputs = [triple(c[0]) for c in chains[:5]] + [(1, final.p1, final.p2)] + [triple(c[0]) for c in chains[5:]]
    hists = [history_of(c) for c in chains[:5]] + [[]] + [history_of(c) for c in chains[5:]]
    lens = [len(c) for c in chains[:5]] + [0] + [len(c) for c in chains[5:]]
    assert len(inputs) == 11
    kw = dict(history_size=4, num_simulations=64, num_threads=2, batch_size=4, node_capacity=1 << 14)
    small = om.analyze(inputs, ASYM, history=hists, num_games=4, pv_len=8, seed=99, **kw)
    large = om.analyze(inputs, ASYM, history=hists, num_games=16, pv_len=8, seed=99, **kw)
    for name in ("visits", "q", "value", "best_action", "pv", "pv_visits", "pv_q", "pv_len", "terminal", "margin"):
        assert torch.equal(getattr(small, name), getattr(large, name)), name
    from othello_mcts.analysis import position_key

    okw = {**KW, "dirichlet_epsilon": 0.0}
    chain_of = chains[:5] + [None] + chains[5:]
    for i, c in enumerate(chain_of):
        if c is None:
            assert bool(small.terminal[i]) and int(small.best_action[i]) == -1 and int(small.visits[i].sum()) == 0
            assert int(small.margin[i]) == bin(final.p1).count("1") - bin(final.p2).count("1")
            assert int(small.pv_len[i]) == 0
            continue
        r = O.OracleMCTS(game_key=position_key(99, i), **okw)
        r.reset_chain(c[:1 + min(15, lens[i] - 1)])
        r.search(A.asymmetric_stub)
        assert small.visits[i].tolist() == by_action(c[0], r.visit_counts()), i
        np.testing.assert_allclose(small.q[i].numpy(), np.array(by_action(c[0], r.mean_action_values(), 0.0), np.float32),
                                   rtol=0, atol=1e-6)
        assert not bool(small.terminal[i])
        assert int(small.best_action[i]) == int(np.argmax(small.visits[i].numpy())) == int(small.pv[i, 0])
        assert int(small.pv_visits[i, 0]) == int(small.visits[i].max())
    recs = small.records()
    assert len(recs) == 11 and recs[5]["terminal"] and recs[0]["pv"][0] == recs[0]["best_action"]


# ------------------------------------------------ 7. the C ABI from the header
def test_the_two_engine_calls_through_ctypes(om):
    """include/othello_mcts_amd.h's oamd_engine_set_positions and
    oamd_engine_principal_variations bound here from the header alone, on the
    foreign host of tests/capi_host.py: test 1's full-history case."""
    import capi_host as H

    raw = ctypes.CDLL(str(H.LIB_PATH))
    vp, i32, u64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_uint64
    set_positions = raw.oamd_engine_set_positions
    set_positions.argtypes = [vp, vp, vp, i32, vp, vp, vp, vp, u64, vp]
    set_positions.restype = ctypes.c_int
    pvs = raw.oamd_engine_principal_variations
    pvs.argtypes = [vp, i32, vp, vp, vp, vp]
    pvs.restype = ctypes.c_int

    chains = root_chains()
    keys = [A.game_key(777, g) for g in range(G)]
    signed = lambda x: x - (1 << 64) if x >= 1 << 63 else x  # noqa: E731
    pos = torch.tensor([[c[0].player, signed(c[0].p1), signed(c[0].p2), 0, 0] for c in chains], dtype=torch.int64)
    K = 15
    hist = torch.zeros((G, K, 5), dtype=torch.int64)
    hist_len = torch.zeros(G, dtype=torch.int32)
    for g, c in enumerate(chains):
        h = c[1:1 + K]
        hist_len[g] = len(h)
        for k, p in enumerate(h):
            hist[g, k] = torch.tensor([p.player, signed(p.p1), signed(p.p2), 0, 0])
    keys_t = torch.tensor([signed(k) for k in keys], dtype=torch.int64)
    e = H.Engine(G, H.SearchConfig(4, 64, 2, 4, 20000.0, 2.5, 0.25, 0.5), seed=5, node_capacity=1 << 14)
    try:
        e.set_stream()
        dev = [t.to(DEV) for t in (pos, hist, hist_len, keys_t)]
        status = torch.full((G,), 99, dtype=torch.int32, device=DEV)
        # argument errors come back as OAMD_INVALID_ARGUMENT and enqueue nothing
        assert set_positions(e.h, None, None, 0, None, None, None, None, 0, status.data_ptr()) == H.OAMD_INVALID_ARGUMENT
        assert set_positions(e.h, dev[0].data_ptr(), dev[1].data_ptr(), 16, None, None, None, None, 0,
                             status.data_ptr()) == H.OAMD_INVALID_ARGUMENT
        assert set_positions(e.h, dev[0].data_ptr(), None, 3, None, None, None, None, 0,
                             status.data_ptr()) == H.OAMD_INVALID_ARGUMENT
        assert status.cpu().tolist() == [99] * G
        assert set_positions(e.h, dev[0].data_ptr(), dev[1].data_ptr(), K, dev[2].data_ptr(), dev[3].data_ptr(), None,
                             None, 0, status.data_ptr()) == H.OAMD_OK
        assert status.cpu().tolist() == [0] * G
        H.search_dense(e, A.asymmetric_stub)
        L = 8
        out = [torch.empty((G, L), dtype=torch.int32, device=DEV), torch.empty((G, L), dtype=torch.int32, device=DEV),
               torch.empty((G, L), dtype=torch.float32, device=DEV), torch.empty(G, dtype=torch.int32, device=DEV)]
        assert pvs(e.h, 0, *[t.data_ptr() for t in out]) == H.OAMD_INVALID_ARGUMENT
        assert pvs(e.h, L, *[t.data_ptr() for t in out]) == H.OAMD_OK
        acts, visits, qs, length = [t.cpu() for t in out]
        for g, c in enumerate(chains):
            r = O.OracleMCTS(game_key=keys[g], **KW)
            r.reset_chain(c[:1 + min(K, len(c) - 1)])
            r.search(A.asymmetric_stub)
            info = e.root_info(g)
            assert e.game_key(g) == keys[g]
            assert info["visits"] == r.visit_counts(), g
            np.testing.assert_allclose(info["q"], np.array(r.mean_action_values(), np.float32), rtol=0, atol=1e-6)
            k = int(np.argmax(info["visits"]))
            assert int(length[g]) >= 1 and int(acts[g, 0]) == O.legal_actions(c[0])[k]
            assert int(visits[g, 0]) == info["visits"][k] and np.float32(qs[g, 0]) == info["q"][k]
    finally:
        e.destroy()
