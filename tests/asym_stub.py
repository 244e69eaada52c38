"""A leaf evaluator with no board symmetry, for tests/test_cpu_symmetry.py and
tests/test_gpu_symmetry.py, and the fixed positions and keys both files share.

oracle.equivariant_stub commutes with the eight board transforms: its policy
is a pointwise function of each square's planes and its value a board mean, so
un-transforming its answer gives the untransformed answer up to the order of
two fp32 sums (an ulp) and the search's per-leaf random symmetry
(search_thread.cpp:92, :139-148) cannot be seen through it. asymmetric_stub adds a fixed per-square table without any D4
invariance to the logits and weights the disc planes of the value by a second
one, so a wrong draw, a wrong feature transform or a wrong prior gather
changes the search.

The engine's callback path evaluates G * L rows per call and the oracle B rows
per call; both must get the same bits for the same row. Hence:
  * no operation reduces across rows;
  * float64 throughout; the channel weights and both tables are multiples of
    1/64 and the features 0 / 1, so every logit and the value's argument are
    exact in any summation order;
  * exp and tanh are elementwise on contiguous arrays; the softmax denominator
    is accumulated square by square in a fixed order;
  * one rounding to float32 at the end.
"""

from __future__ import annotations

import numpy as np

import oracle as O


def _table(mult: int, add: int) -> np.ndarray:
    """((mult * s + add) mod 64) / 32 - 1 for s = 0..63: a permutation of the
    multiples of 1/32 in [-1, 1) (mult odd)."""
    s = np.arange(64, dtype=np.int64)
    return ((mult * s + add) % 64).astype(np.float64) / 32.0 - 1.0


def make_asymmetric_stub(policy_table: np.ndarray, value_table: np.ndarray, pass_logit: float = -2.0,
                         reverse_channels: bool = False):
    policy_table = np.ascontiguousarray(policy_table, np.float64).reshape(64)
    value_table = np.ascontiguousarray(value_table, np.float64).reshape(64)
    for tab in (policy_table, value_table):
        assert np.array_equal(tab * 64.0, np.round(tab * 64.0))

    def stub(features: np.ndarray):
        x = np.ascontiguousarray(features, np.float64)
        n, C = x.shape[0], x.shape[1]
        x = x.reshape(n, C, 64)
        w = np.round(np.linspace(-1.0, 1.0, C) * 64.0) / 64.0
        if reverse_channels:
            w = w[::-1].copy()
        logits = np.empty((n, 65), np.float64)
        sq = np.zeros((n, 64), np.float64)
        for c in range(C):  # exact: dyadic weights, 0 / 1 features
            sq += w[c] * x[:, c, :]
        logits[:, :64] = sq + policy_table[None, :]
        logits[:, 64] = pass_logit
        mx = logits[:, 0].copy()
        for k in range(1, 65):
            np.maximum(mx, logits[:, k], out=mx)
        e = np.exp(np.ascontiguousarray(logits - mx[:, None]).reshape(-1)).reshape(n, 65)
        den = e[:, 0].copy()
        for k in range(1, 65):  # fixed order, row by row
            den += e[:, k]
        policy = e / den[:, None]
        z = np.zeros(n, np.float64)
        d = x[:, 1, :] - x[:, 2, :]
        for k in range(64):  # exact
            z += value_table[k] * d[:, k]
        z = z / 16.0 + 0.125 * x[:, 0, 0]
        value = np.tanh(np.ascontiguousarray(z))
        return policy.astype(np.float32), value.astype(np.float32)

    return stub


POLICY_TABLE_A, VALUE_TABLE_A = _table(37, 11), _table(29, 5)
POLICY_TABLE_B, VALUE_TABLE_B = _table(23, 40), _table(51, 17)

asymmetric_stub_a = make_asymmetric_stub(POLICY_TABLE_A, VALUE_TABLE_A)
asymmetric_stub_b = make_asymmetric_stub(POLICY_TABLE_B, VALUE_TABLE_B, pass_logit=-1.5, reverse_channels=True)
asymmetric_stub = asymmetric_stub_a


# ----------------------------------------------------------- shared test data
def draw(key: int, event: int) -> int:
    """The symmetry of the leaf selected at `event` of the game stream `key`
    (DESIGN.md "Random streams"; search_thread.cpp:92)."""
    L = O.lib()
    return int(L.orc_mix64(L.orc_stream_key(key, event, 0)) >> 61)


def chain_after(actions) -> list:
    """Positions from the initial one through `actions`, newest first (the
    order oracle.features takes)."""
    p = O.initial_position()
    chain = [p]
    for a in actions:
        p = O.apply_action(p, int(a))
        chain.insert(0, p)
    return chain


def untransform_policy(policy: np.ndarray, t: int) -> np.ndarray:
    """policy[transform_action(a, t)] for a = 0..64 (search_thread.cpp:139-148)."""
    idx = np.array([O.transform_action(a, t) for a in range(65)])
    return policy[..., idx]


def mix64(z: int) -> int:
    return int(O.lib().orc_mix64(z & 0xFFFFFFFFFFFFFFFF))


def game_key(seed: int, g: int) -> int:
    """Random-stream key of game g of an engine created with `seed` (DESIGN.md "Random streams")."""
    return mix64(seed ^ mix64(g + 0x632BE59BD9B4E019))


# Row-level tests: three games of one engine, each after its own 6-ply prefix
# (legal sequences from the initial position whose 8 transformed feature stacks
# are pairwise distinct), T = 2 x B = 8. ROW_SEED is an engine seed for which
# the first L = 16 draws of every one of its three game keys hit all 8
# transforms (tests/test_cpu_symmetry.py asserts both properties).
ROW_THREADS, ROW_BATCH, ROW_GAMES = 2, 8, 3
ROW_PREFIXES = ((44, 45, 19, 34, 26, 20), (26, 34, 44, 20, 12, 43), (26, 18, 37, 34, 17, 43))
ROW_SEED = 17
ROW_KEYS = (0x38F43D0C36A3EF35, 0x57A34FF08FD0CCF4, 0xE4E4E5B27632DED0)  # game_key(ROW_SEED, g)


def expected_first_rows(key: int, prefix, history_size: int, rows: int = ROW_THREADS * ROW_BATCH):
    """(transforms, features) of the first `rows` leaf rows of a fresh search
    whose root, reached through `prefix`, is unexpanded: every selection stops
    at the root and takes the draw of event i (no Dirichlet event precedes an
    expansion of the root)."""
    chain = chain_after(prefix)
    ts = [draw(key, e) for e in range(rows)]
    return ts, np.stack([O.features(chain, history_size, t) for t in ts])


def random_game_chains(games: int) -> list:
    """Every position of `games` seeded random games as its chain (newest first)."""
    chains = []
    for game in range(games):
        rng = np.random.default_rng(game)
        p = O.initial_position()
        chain = [p]
        while p.player != 0:
            chains.append(list(chain))
            legal = O.legal_actions(p)
            p = O.apply_action(p, int(legal[int(rng.integers(len(legal)))]))
            chain.insert(0, p)
    return chains


def transformed_stacks(chains, history_size: int) -> np.ndarray:
    """(positions, 8, C, 8, 8): every chain's features under every transform."""
    return np.stack([np.stack([O.features(c, history_size, t) for t in range(8)]) for c in chains])


def sensitivity(stub, f: np.ndarray):
    """(minimum over positions and t = 1..7 of the max-abs difference between
    the un-transformed policy of the features under t and the t = 0 policy,
    per-t share of the positions whose stack t moves on which the value
    changes)."""
    n = f.shape[0]
    pol, val = stub(np.ascontiguousarray(f.reshape(-1, *f.shape[2:])))
    pol, val = pol.reshape(n, 8, 65), val.reshape(n, 8)
    min_policy, shares = np.inf, []
    for t in range(1, 8):
        d = np.abs(untransform_policy(pol[:, t], t) - pol[:, 0]).max(axis=1)
        min_policy = min(min_policy, float(d.min()))
        moved = np.array([not np.array_equal(f[i, t], f[i, 0]) for i in range(n)])
        assert moved.sum() > n // 2
        shares.append(float((val[moved, t] != val[moved, 0]).mean()))
    return min_policy, shares
