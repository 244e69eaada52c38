"""What tests/test_gpu_symmetry.py rests on, checked without a GPU: the
asymmetric stub (tests/asym_stub.py) gives the same bits for a row however the
rows are batched and reacts to every board transform, the oracle's search
depends on its symmetry draws with it (and provably not with
oracle.equivariant_stub), the draw is uniform over the 8 transforms, and the
rows of a fresh search's first NN calls are predictable from the game key
alone."""

import numpy as np
import pytest

import asym_stub as A
import numerics
import oracle as O

STUBS = {"a": A.asymmetric_stub_a, "b": A.asymmetric_stub_b}


# ------------------------------------------------------------------ positions
@pytest.fixture(scope="module")
def random_games():
    """Every position of 40 seeded random games as its chain (newest first),
    shared by the tests below and not modified."""
    chains = A.random_game_chains(40)
    assert len(chains) > 2000
    return chains


@pytest.fixture(scope="module", params=[4, 8], ids=lambda h: f"H{h}")
def stacks(request, random_games):
    """(H, (positions, 8, C, 8, 8) feature stacks under every transform)."""
    H = request.param
    return H, A.transformed_stacks(random_games, H)


# ------------------------------------------------------------ row independence
@pytest.mark.parametrize("name", ["a", "b"])
def test_stub_rows_do_not_depend_on_the_batch(stacks, name):
    """The engine evaluates G * L rows per call, the oracle B: row i of a
    300-row batch has the bits of the same row evaluated alone, in chunks of 8
    and in chunks of 48."""
    H, f = stacks
    stub = STUBS[name]
    rng = np.random.default_rng(H)
    pick = rng.choice(f.shape[0] * 8, 300, replace=False)
    x = np.ascontiguousarray(f.reshape(-1, *f.shape[2:])[pick])
    pol, val = stub(x)
    assert pol.shape == (300, 65) and pol.dtype == np.float32
    assert val.shape == (300,) and val.dtype == np.float32
    np.testing.assert_allclose(pol.astype(np.float64).sum(1), 1.0, atol=1e-6)
    assert (np.abs(val) < 1).all()
    for chunk in (1, 8, 48):
        for i in range(0, 300, chunk):
            p, v = stub(x[i:i + chunk])
            assert p.tobytes() == pol[i:i + chunk].tobytes(), (chunk, i)
            assert v.tobytes() == val[i:i + chunk].tobytes(), (chunk, i)
    # a strided view of the same rows
    p, v = stub(x[::3])
    assert p.tobytes() == pol[::3].tobytes() and v.tobytes() == val[::3].tobytes()


# ------------------------------------------------------------------ sensitivity
@pytest.mark.parametrize("name", ["a", "b"])
def test_stub_reacts_to_every_transform(stacks, name):
    """Features under t, evaluated and un-transformed as the search does
    (search_thread.cpp:139-148), never give back the t = 0 policy: max-abs
    difference >= 1e-3 for every position and every t in 1..7. The value
    changes on the majority of the positions whose stack t does not fix."""
    H, f = stacks
    stub = STUBS[name]
    n = f.shape[0]
    min_policy, shares = A.sensitivity(stub, f)
    numerics.record(f"asymmetric stub {name} H={H}",
                    f"positions={n} min_policy_sensitivity={min_policy:.3e} "
                    f"value_share_t1..7={' '.join(f'{s:.3f}' for s in shares)}")
    print(f"stub {name} H={H}: positions={n} min policy sensitivity {min_policy:.3e}, value shares {shares}")
    assert min_policy >= 1e-3
    assert min(shares) > 0.5, shares


def test_equivariant_stub_cannot_see_a_transform(stacks):
    """The blind spot at its root: oracle.equivariant_stub's un-transformed
    policy and its value are the t = 0 ones up to fp32 summation order (the
    softmax denominator and the board mean add the same terms permuted), a
    few ulp against the asymmetric stub's >= 1e-3."""
    H, f = stacks
    x = f[::16]
    n = x.shape[0]
    pol, val = O.equivariant_stub(np.ascontiguousarray(x.reshape(-1, *x.shape[2:])))
    pol, val = pol.reshape(n, 8, 65), val.reshape(n, 8)
    for t in range(1, 8):
        np.testing.assert_allclose(A.untransform_policy(pol[:, t], t), pol[:, 0], rtol=1e-6, atol=0)
    assert np.abs(val - val[:, :1]).max() <= 1e-6


# ------------------------------------------------------------------ blind spot
def _searches(stub, key, moves):
    """Four searches with tree reuse; `moves` is filled by the first caller
    (argmax of its visits) and followed by the others."""
    m = O.OracleMCTS(history_size=4, num_simulations=200, num_threads=2, batch_size=8,
                     dirichlet_epsilon=0.0, game_key=key)
    out = []
    for ply in range(4):
        m.search(stub)
        vc = m.visit_counts()
        out.append((vc, np.array(m.mean_action_values(), np.float32).tobytes()))
        if len(moves) == ply:
            moves.append(O.legal_actions(m.position())[int(np.argmax(vc))])
        m.apply_action(moves[ply])
    return out


def test_game_key_matters_only_with_the_asymmetric_stub():
    """eps = 0, so the game key enters a search through the symmetry draws
    alone. Four moves with tree reuse under keys 1..4: with the equivariant
    stub every search has the same visits and Q bits, which is why no test
    that uses it can see the symmetry path; with the asymmetric stub the
    searches differ from the first one on."""
    moves: list[int] = []
    eq = [_searches(O.equivariant_stub, key, moves) for key in (1, 2, 3, 4)]
    assert all(r == eq[0] for r in eq[1:])
    asym = [_searches(A.asymmetric_stub, key, moves) for key in (1, 2, 3, 4)]
    first = [r[0][0] for r in asym]
    assert len({tuple(v) for v in first}) > 1, first
    assert sum(r != asym[0] for r in asym[1:]) == 3
    assert len(moves) == 4


# ------------------------------------------------------------------------ draw
@pytest.mark.parametrize("key", [1, A.ROW_KEYS[0], 0xFFFFFFFFFFFFFFFF])
def test_symmetry_draw_is_uniform(key):
    """mix64(stream_key(key, e, 0)) >> 61 over 80,000 events: each transform
    10,000 +- 500 times (sigma = 94, a 5.3 sigma band)."""
    L = O.lib()
    counts = np.bincount([L.orc_mix64(L.orc_stream_key(key, e, 0)) >> 61 for e in range(80000)], minlength=8)
    assert counts.sum() == 80000 and counts.shape == (8,)
    assert (np.abs(counts - 10000) <= 500).all(), counts


# ----------------------------------------------------------- first NN calls
def test_row_level_fixtures_are_what_the_gpu_test_assumes():
    assert [A.game_key(A.ROW_SEED, g) for g in range(A.ROW_GAMES)] == list(A.ROW_KEYS)
    for key, prefix in zip(A.ROW_KEYS, A.ROW_PREFIXES):
        assert {A.draw(key, e) for e in range(A.ROW_THREADS * A.ROW_BATCH)} == set(range(8))
        chain = A.chain_after(prefix)  # raises nothing: apply_action of an illegal move would give garbage
        p = O.initial_position()
        for a in prefix:
            assert a in O.legal_actions(p)
            p = O.apply_action(p, a)
        assert p.player != 0 and p.tuple() == chain[0].tuple()
        for H in (4, 8):
            assert len({O.features(chain, H, t).tobytes() for t in range(8)}) == 8
    assert len(set(A.ROW_PREFIXES)) == A.ROW_GAMES


@pytest.mark.parametrize("eps", [0.0, 0.25])
@pytest.mark.parametrize("H", [4, 8])
@pytest.mark.parametrize("g", range(A.ROW_GAMES))
def test_first_nn_calls_are_the_root_under_the_first_draws(g, H, eps):
    """A fresh oracle at an unexpanded root: all L selections of the first
    round stop at the root, so row i of the first T NN calls is the root's
    chain under the draw of event i; no Dirichlet event comes before them."""
    key, prefix = A.ROW_KEYS[g], A.ROW_PREFIXES[g]
    T, B = A.ROW_THREADS, A.ROW_BATCH
    m = O.OracleMCTS(history_size=H, num_simulations=4 * T * B, num_threads=T, batch_size=B,
                     dirichlet_epsilon=eps, game_key=key)
    for a in prefix:
        m.apply_action(a)
    assert m.events() == 0
    calls = []

    def spy(features):
        calls.append(features.copy())
        return A.asymmetric_stub(features)

    m.search(spy)
    assert all(c.shape == (B, 1 + 2 * H, 8, 8) for c in calls[:T])
    ts, expected = A.expected_first_rows(key, prefix, H)
    np.testing.assert_array_equal(np.concatenate(calls[:T]), expected)
    assert set(ts) == set(range(8))
    assert sum(m.visit_counts()) == 3 * T * B  # the first round's leaves were all the root


# ----------------------------------------------------------------------- arena
def test_asymmetric_arena_reference_covers_what_the_gpu_test_needs():
    """tests/test_gpu_arena.py's asymmetric case compares against these eight
    matches: they differ from the equivariant ones and keep a forced pass, a
    random tie-break in every game, both sides moving and wins for both colours."""
    import arena_ref as R

    ms = R.reference_matches(0, A.asymmetric_stub_a, A.asymmetric_stub_b)
    games = [R.summary(m) for m in ms]
    assert games != [R.summary(m) for m in R.reference_matches(0)]
    assert sum(g[1] for g in games) >= 1, games
    assert all(g[2] >= 1 for g in games), games
    assert {m["result"] for m in ms} >= {1, 2}, games
    assert all({p["a_moves"] for p in m["plies"]} == {True, False} for m in ms)
