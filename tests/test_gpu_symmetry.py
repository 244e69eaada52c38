"""The per-leaf board symmetry of the HIP search against the oracle, with an
evaluator that can see it (tests/asym_stub.py).

Every other oracle / reference comparison of the search evaluates leaves with
oracle.equivariant_stub or uniform_stub, for which the symmetry's three steps
(the draw, csrc/rng.h draw_transform at csrc/tree_search.h select_range; the features
under t, inverse_transform in k_features_f32; the priors read back at
transform_action(a, t) in expand_quads) cancel up to an ulp of fp32 summation
order: a constant draw, a draw at the wrong event or a feature transform and a
prior gather that are not inverses leave those tests green, or fail one only
where such an ulp tips a near-tie (tests/test_cpu_symmetry.py shows the blind
spot on the oracle). Here the evaluator is asymmetric under all seven non-identity
transforms and row-independent to the bit, so every comparison is exact: visit
counts as lists, Q bits, 8-fold targets and feature rows with
assert_array_equal. Reference: search_thread.cpp:59-148, transformation.h:40-116.

All searches take the callback path (host evaluator). The packed ResNet
prologue's own inverse_transform (csrc/resnet.hip) is pinned at the kernel by
tests/test_gpu_resnet_packed.py: packed rows under every symmetry against the
exact nets and, bit for bit, against the fp32-plane path, and the engine's own
rows against k_features_f32.
"""

import numpy as np
import pytest
import torch

import asym_stub as A
import numerics
import oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


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


def _q(values):
    return np.array(values, np.float32)


# ------------------------------------------------------------------- the stub
def test_stub_holds_on_this_host():
    """tests/test_cpu_symmetry.py's two properties of the evaluator on the
    machine the comparisons below run on, over the positions of 8 random games
    (H = 4): rows evaluated 128 at a time (the engine's call) have the bits of
    rows evaluated 8 at a time (the oracle's), and every transform moves the
    policy by >= 1e-3 and the value on the majority of positions."""
    f = A.transformed_stacks(A.random_game_chains(8), 4)
    x = np.ascontiguousarray(f.reshape(-1, *f.shape[2:]))
    for stub in (A.asymmetric_stub_a, A.asymmetric_stub_b):
        big = [stub(x[i:i + 128]) for i in range(0, len(x), 128)]
        small = [stub(x[i:i + 8]) for i in range(0, len(x), 8)]
        for k in (0, 1):
            assert np.concatenate([o[k] for o in big]).tobytes() == np.concatenate([o[k] for o in small]).tobytes()
        min_policy, shares = A.sensitivity(stub, f)
        numerics.record(f"asymmetric stub {'a' if stub is A.asymmetric_stub_a else 'b'} H=4 (8 games)",
                        f"positions={f.shape[0]} min_policy_sensitivity={min_policy:.3e} "
                        f"value_share_t1..7={' '.join(f'{s:.3f}' for s in shares)}")
        assert min_policy >= 1e-3
        assert min(shares) > 0.5, shares


# ------------------------------------------------------------------ row level
@pytest.mark.parametrize("eps", [0.0, 0.25])
@pytest.mark.parametrize("H", [4, 8])
def test_first_round_rows_are_the_roots_under_the_streams_draws(om, H, eps):
    """draw_transform, the event it is taken at and k_features_f32 with no
    search around them: three fresh games, each after its own 6-ply prefix,
    one select. Every root is unexpanded, so row (g, i) is game g's root chain
    under the draw of event i of its stream (oracle.features of the chain; keys
    and prefixes checked in tests/test_cpu_symmetry.py) and every row waits for
    the NN. The search is then finished through the step API with the
    asymmetric stub and each game compared with its oracle."""
    G, T, B = A.ROW_GAMES, A.ROW_THREADS, A.ROW_BATCH
    L, C, sims = T * B, 1 + 2 * H, 4 * T * B
    kw = dict(history_size=H, num_simulations=sims, num_threads=T, batch_size=B, dirichlet_epsilon=eps)
    b = om.BatchedMCTS(G, seed=A.ROW_SEED, node_capacity=1 << 14, **kw)
    assert [b.engine.game_key(g) for g in range(G)] == list(A.ROW_KEYS)
    refs = [O.OracleMCTS(game_key=A.ROW_KEYS[g], **kw) for g in range(G)]
    for k in range(6):
        acts = torch.tensor([A.ROW_PREFIXES[g][k] for g in range(G)], dtype=torch.int32)
        b.apply_actions(acts.to(DEV))
        for g, r in enumerate(refs):
            r.apply_action(A.ROW_PREFIXES[g][k])
    for g, r in enumerate(refs):
        i = b.root_info(g)
        assert (i["player"], i["player1_discs"], i["player2_discs"], i["legal_moves"]) == r.position().tuple()[:4]

    b._stream()
    e = b.engine
    rows = G * L
    feat = torch.empty((rows, C, 8, 8), dtype=torch.float32, device=DEV)
    steps = e.search_begin()
    assert steps == sims // L
    e.select()
    e.features(feat.data_ptr(), 0, rows)
    got = feat.cpu().numpy()
    seen = set()
    for g in range(G):
        ts, expected = A.expected_first_rows(A.ROW_KEYS[g], A.ROW_PREFIXES[g], H, L)
        seen |= set(ts)
        for i in range(L):
            np.testing.assert_array_equal(got[g * L + i], expected[i], err_msg=f"game {g} row {i} t={ts[i]}")
    assert seen == set(range(8))
    assert e.leaf_flags().tolist() == [1] * rows
    numerics.record(f"symmetry rows H={H} eps={eps}", f"rows={rows} transforms seen={sorted(seen)}")

    # finish the search: this round's evaluation, the remaining rounds, backup
    for step in range(steps):
        if step > 0:
            e.select()
            e.features(feat.data_ptr(), 0, rows)
        out = ASYM(feat)
        pol = out["policy"].to(DEV, torch.float32).contiguous()
        val = out["value"].to(DEV, torch.float32).contiguous()
        e.set_evaluation(pol.data_ptr(), val.data_ptr(), 0, rows)
    e.backup()
    e.check_health()
    for g, r in enumerate(refs):
        r.search(A.asymmetric_stub)
        assert b.visit_counts(g) == r.visit_counts(), g
        assert sum(b.visit_counts(g)) == sims - L
        np.testing.assert_array_equal(_q(b.mean_action_values(g)), _q(r.mean_action_values()))


# ---------------------------------------------------------------- single game
def _pair(om, **kw):
    m = om.MCTS(torch_device="cpu", seed=1234, **kw)
    m.set_native_nn(False)
    return m, O.OracleMCTS(game_key=m.game_key(), **kw)


def _compare_move(m, ref, tag):
    """One search of both; visits, Q bits and the 8-fold targets. Returns the visits."""
    m.search(ASYM)
    ref.search(A.asymmetric_stub)
    vc = m.visit_counts()
    assert vc == ref.visit_counts(), tag
    np.testing.assert_array_equal(_q(m.mean_action_values()), _q(ref.mean_action_values()), err_msg=str(tag))
    d = m.self_play_data()
    f, p = ref.self_play_data()
    np.testing.assert_array_equal(torch.stack(d["features"]).numpy(), f, err_msg=str(tag))
    np.testing.assert_array_equal(torch.stack(d["policy"]).numpy(), p, err_msg=str(tag))
    return vc


CASES = {
    # name: (T, B, H, simulations, eps, moves)
    "single_thread": (1, 16, 4, 200, 0.0, 6),
    "two_threads_noise": (2, 16, 8, 200, 0.25, 6),
    "backup_chunks_64_64_16": (3, 48, 8, 288, 0.25, 3),
    "widest_packed_row": (2, 16, 15, 128, 0.25, 3),
    # one round per search: all 1024 selections stop at the unexpanded root, so
    # only the expansion itself is compared (every visit count is 0) ...
    "engine_limit_1024_leaves": (4, 256, 4, 1024, 0.0, 2),
    # ... and with a second round the 1024 leaves descend through its priors
    "engine_limit_1024_leaves_two_rounds": (4, 256, 4, 2048, 0.0, 2),
}


@pytest.mark.parametrize("name", list(CASES))
def test_mcts_matches_oracle_with_asymmetric_stub(om, name):
    """The drop-in MCTS against OracleMCTS(game_key=m.game_key()) at the shapes
    of test_gpu_parity.py's oracle tests, argmax moves with tree reuse."""
    T, B, H, sims, eps, moves = CASES[name]
    m, ref = _pair(om, history_size=H, num_simulations=sims, num_threads=T, batch_size=B, dirichlet_epsilon=eps)
    for mv in range(moves):
        assert not m.position().is_terminal()
        vc = _compare_move(m, ref, (name, mv))
        a = m.position().legal_actions()[int(np.argmax(vc))]
        m.apply_action(a)
        ref.apply_action(a)


def test_mcts_matches_oracle_whole_game_with_asymmetric_stub(om):
    """From the initial position to the end (passes, terminal leaves, all-terminal
    batches, tree reuse over every move), T = 2 x B = 8, H = 3, 96 simulations,
    eps = 0.25."""
    m, ref = _pair(om, history_size=3, num_simulations=96, num_threads=2, batch_size=8, dirichlet_epsilon=0.25)
    moves = 0
    while not m.position().is_terminal():
        vc = _compare_move(m, ref, moves)
        a = m.position().legal_actions()[int(np.argmax(vc))]
        m.apply_action(a)
        ref.apply_action(a)
        moves += 1
    assert moves >= 30
    assert ref.position().player == 0


# -------------------------------------------------------------------- batched
def test_batched_games_match_their_oracles_with_asymmetric_stub(om):
    """Eight games in one engine (the evaluator sees G * L = 128 rows per call,
    the oracles 8), each after 0-8 host-chosen random opening plies, four moves
    with tree reuse: every game equals its own oracle."""
    G, H = 8, 4
    kw = dict(history_size=H, num_simulations=64, num_threads=2, batch_size=8, dirichlet_epsilon=0.25)
    b = om.BatchedMCTS(G, seed=505, node_capacity=1 << 14, **kw)
    refs = [O.OracleMCTS(game_key=b.engine.game_key(g), **kw) for g in range(G)]
    rng = np.random.default_rng(606)
    plies = rng.permutation(9)[:G]  # eight distinct lengths in 0..8
    for k in range(int(plies.max())):
        acts = torch.full((G,), -1, dtype=torch.int32)
        for g, r in enumerate(refs):
            if k < plies[g]:
                legal = O.legal_actions(r.position())
                acts[g] = int(legal[rng.integers(len(legal))])
                r.apply_action(int(acts[g]))
        b.apply_actions(acts.to(DEV))
    for mv in range(4):
        sims, evals = b.search(ASYM)
        assert sims == G * 64 and 0 < evals <= sims
        acts = torch.full((G,), -1, dtype=torch.int32)
        for g, r in enumerate(refs):
            r.search(A.asymmetric_stub)
            info = b.root_info(g)
            vc = r.visit_counts()
            assert info["visit_counts"] == vc, (mv, g)
            np.testing.assert_array_equal(_q(info["mean_action_values"]), _q(r.mean_action_values()))
            d = b.self_play_data(g)
            f, p = r.self_play_data()
            np.testing.assert_array_equal(torch.stack(d["features"]).numpy(), f)
            np.testing.assert_array_equal(torch.stack(d["policy"]).numpy(), p)
            a = O.legal_actions(r.position())[int(np.argmax(vc))]
            acts[g] = a
            r.apply_action(a)
        b.apply_actions(acts.to(DEV))


# ---------------------------------------------------------- self-play driver
def test_selfplay_driver_targets_and_moves_match_oracle_with_asymmetric_stub(om):
    """What test_gpu_selfplay.py's test_selfplay_driver_targets_and_moves_match_oracle
    checks, with the asymmetric evaluator: k_selfplay_move's 8-fold targets equal
    the oracle's self_play_data bit for bit and its action is the oracle's
    restatement of train.py:421-430 drawn from the same event, so the move
    draws and the symmetry draws share one stream correctly."""
    G, H, moves = 16, 4, 18
    kw = dict(history_size=H, num_simulations=64, num_threads=2, batch_size=8, dirichlet_epsilon=0.25)
    b = om.BatchedMCTS(G, seed=41, node_capacity=1 << 16, **kw)
    refs = [O.OracleMCTS(game_key=b.engine.game_key(g), **kw) for g in range(G)]
    for ply in range(moves):
        b.search(ASYM)
        for r in refs:
            r.search(A.asymmetric_stub)
        out = b.selfplay_move(temperature_moves=12, temperature=1.0, opening_moves=0, emit_targets=True)
        acts = out["actions"].cpu().numpy()
        fin = out["finished"].cpu().numpy()
        feats = out["features"].cpu().numpy()
        pols = out["policy"].cpu().numpy()
        for g, r in enumerate(refs):
            f, p = r.self_play_data()
            np.testing.assert_array_equal(feats[g], f, err_msg=f"ply {ply} game {g} features")
            np.testing.assert_array_equal(pols[g], p, err_msg=f"ply {ply} game {g} policy")
            vc = np.array(r.visit_counts())
            a = r.selfplay_action(ply, 12, 1.0)
            assert acts[g] == a, (ply, g, acts[g], a, vc)
            k = O.legal_actions(r.position()).index(a)
            assert vc[k] > 0 if ply < 12 else vc[k] == vc.max()
            assert fin[g] == 0  # 18 plies from the initial position: no game ends
            r.apply_action(a)
