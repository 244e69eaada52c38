"""Test reference for forced playouts and policy target pruning.

The oracle (oracle/omcts_oracle.c) cannot force playouts, so this module
restates its search in Python, function by function: choose_best_child,
select_leaf, expand_and_backward, and the T x B schedule of orc_mcts_search
with the all-terminal skip. It is built on the primitives oracle.lib() exports
(orc_apply_action, orc_legal_actions, orc_features, orc_transform_action,
orc_stream_key, orc_mix64, orc_gamma); every float is a numpy float32, the
exploration rate uses libm's logf through ctypes, the square roots np.sqrt on
float32 (IEEE, as sqrtf). With ``forced_k = 0`` it must equal OracleMCTS bit for
bit (tests/test_cpu_forced_playouts.py checks that first); ``forced_k > 0`` adds
the forcing rule, and ``prune`` / ``self_play_data(prune_k=...)`` the pruning.

The rule (fp32, in this order):

    forced_c = n_c > 0 and f32(n_c) * f32(n_c) < (k * prob_c) * f32(total)
    ucb_c    = +inf if forced_c else q_c + mult * prob_c / (1 + f32(n_c))

at the root of a search that is not a fast one, with more than one child; prob_c
is the prior of that selection's PUCT line (noised when eps > 0), total the
children's visit sum. Pruning: see ``prune``.
"""

from __future__ import annotations

import ctypes
import ctypes.util

import numpy as np

import oracle as O

F = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m"))
_libm.logf.restype = ctypes.c_float
_libm.logf.argtypes = [ctypes.c_float]
_libm.powf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]


def logf(x) -> np.float32:
    return F(_libm.logf(float(x)))


def explore_rate(n: int, c_base, c_init) -> np.float32:
    """search_thread.cpp:198-203 as the oracle's choose_best_child writes it."""
    return F(logf((F(1 + n) + F(c_base)) / F(c_base)) + F(c_init))


def prune(n_root: int, visits, q, priors, c_base=20000.0, c_init=2.5, k=2.0, hits: set | None = None) -> np.ndarray:
    """Pruned visit counts of a root's children (child order). ``hits`` collects
    the names of the branches taken (for the branch coverage test)."""
    n = [int(x) for x in visits]
    q = [F(x) for x in q]
    p = [F(x) for x in priors]
    hits = hits if hits is not None else set()
    nc = len(n)
    total = sum(n)
    if nc <= 1:
        hits.add("single")
        return np.array(n, np.int32)
    if total == 0:
        hits.add("unvisited")
        return np.array(n, np.int32)
    best = max(range(nc), key=lambda j: (n[j], -j))  # the first of the largest
    if n.count(n[best]) > 1:
        hits.add("tie")
    k = F(k)
    mult = F(explore_rate(n_root, c_base, c_init) * np.sqrt(F(total)))

    def u(j, m):
        return F(q[j] + F(F(mult * p[j]) / F(F(1.0) + F(m))))

    ubest = u(best, n[best])
    out = list(n)
    for j in range(nc):
        if j == best or n[j] <= 0:
            continue
        cap = int(np.sqrt(F(F(k * p[j]) * F(total))))
        m = n[j]
        steps = 0
        stopped = False
        while steps < cap and m > 0:
            if u(j, m - 1) < ubest:
                m -= 1
                steps += 1
            else:
                stopped = True
                break
        if stopped:
            hits.add("puct_stop" if steps else "nothing")
        elif cap > 0 and steps == cap and m > 0:
            hits.add("cap_stop")
        if cap == 0 and n[j] == 1:
            hits.add("one_kept")
        if m < n[j] and m == 1:
            hits.add("one_dropped")
            m = 0
        if m == 0:
            hits.add("zeroed")
        out[j] = m
    return np.array(out, np.int32)


class ForcedMCTS:
    """One game's search, the oracle's semantics, with a forcing factor."""

    def __init__(self, history_size=4, num_simulations=800, num_threads=2, batch_size=16, c_puct_base=20000.0,
                 c_puct_init=2.5, dirichlet_epsilon=0.25, dirichlet_alpha=0.5, game_key=0, forced_k=0.0):
        self.H, self.S, self.T, self.B = history_size, num_simulations, num_threads, batch_size
        self.c_base, self.c_init = F(c_puct_base), F(c_puct_init)
        self.eps, self.alpha = F(dirichlet_epsilon), F(dirichlet_alpha)
        self.key = int(game_key)
        self.forced_k = F(forced_k)
        self.L = O.lib()
        self.reset_position()

    # ------------------------------------------------------------- the tree
    def reset_position(self) -> None:
        self.pos, self.parent, self.first, self.nch = [], [], [], []
        self.N = np.zeros(1024, np.int32)
        self.W = np.zeros(1024, np.float32)
        self.Q = np.zeros(1024, np.float32)
        self.P = np.zeros(1024, np.float32)
        self.count = 0
        self.root = self._new_node(O.initial_position(), -1)
        self.event = 0

    def _new_node(self, pos, parent) -> int:
        i = self.count
        if i == len(self.N):
            for name in ("N", "W", "Q", "P"):
                a = getattr(self, name)
                setattr(self, name, np.concatenate([a, np.zeros_like(a)]))
        self.pos.append(pos)
        self.parent.append(parent)
        self.first.append(-1)
        self.nch.append(0)
        self.N[i], self.W[i], self.Q[i], self.P[i] = 0, 0.0, 0.0, 1.0
        self.count += 1
        return i

    def position(self):
        return self.pos[self.root]

    # ------------------------------------------- search_thread.cpp:192-260
    def _choose_best_child(self, node: int, force: bool) -> int:
        nc, fc = self.nch[node], self.first[node]
        if nc == 1:
            return fc
        sl = slice(fc, fc + nc)
        n, q, p = self.N[sl], self.Q[sl], self.P[sl]
        total = int(n.sum(dtype=np.int64))
        mult = F(explore_rate(int(self.N[node]), self.c_base, self.c_init) * np.sqrt(F(total)))
        prob = p
        at_root = node == self.root
        if at_root and self.noise_eps > 0:
            ev = self.event
            self.event += 1
            noise = np.array([self.L.orc_gamma(self.L.orc_stream_key(self.key, ev, j), float(self.alpha))
                              for j in range(nc)], np.float32)
            noise_sum = F(0.0)
            for x in noise:
                noise_sum = F(noise_sum + x)
            if noise_sum == 0:
                noise_sum = F(1.0)
            pm = F(F(1.0) - self.noise_eps)
            nm = F(self.noise_eps / noise_sum)
            prob = p * pm + noise * nm
        nf = n.astype(np.float32)
        ucb = q + (mult * prob) / (F(1.0) + nf)
        assert ucb.dtype == np.float32
        if at_root and force and self.forced_k > 0:
            forced = (n > 0) & (nf * nf < (self.forced_k * prob) * F(total))
            ucb = np.where(forced, F(np.inf), ucb)
        return fc + int(np.argmax(ucb))  # the first maximum (strict '>' scan)

    # -------------------------------------------- search_thread.cpp:62-79
    def _select_leaf(self, i: int, force: bool) -> None:
        node = self.root
        while not (self.pos[node].player == 0 or self.nch[node] == 0):
            node = self._choose_best_child(node, force)
        self.leaves[i] = node
        x = node
        while x != self.root:
            self.N[x] += 1
            self.W[x] = F(self.W[x] - F(1.0))
            self.Q[x] = F(self.W[x] / F(self.N[x]))
            x = self.parent[x]
        self.N[self.root] += 1
        if self.pos[node].player != 0:
            ev = self.event
            self.event += 1
            self.trans[i] = self.L.orc_mix64(self.L.orc_stream_key(self.key, ev, 0)) >> 61
        else:
            self.trans[i] = 0

    def _chain(self, leaf: int) -> list:
        chain, x = [], leaf
        while x >= 0 and len(chain) < self.H:
            chain.append(self.pos[x])
            x = self.parent[x]
        return chain

    # ------------------------------------------- search_thread.cpp:130-190
    def _expand_and_backward(self, leaf: int, t: int, policy, value) -> None:
        pos = self.pos[leaf]
        if pos.player != 0 and self.nch[leaf] == 0:
            acts = O.legal_actions(pos)
            first = self.count
            for a in acts:
                c = self._new_node(O.apply_action(pos, a), leaf)
                self.P[c] = policy[self.L.orc_transform_action(a, t)]
            self.first[leaf] = first
            self.nch[leaf] = len(acts)
        if pos.player != 0:
            v = F(-F(value))
        else:
            par = self.pos[self.parent[leaf]]
            mine, theirs = (pos.p1, pos.p2) if par.player == 1 else (pos.p2, pos.p1)
            a, b = bin(mine).count("1"), bin(theirs).count("1")
            v = F(1.0 if a > b else (-1.0 if a < b else 0.0))
        x = leaf
        while x != self.root:
            self.W[x] = F(self.W[x] + F(F(1.0) + v))
            self.Q[x] = F(self.W[x] / F(self.N[x]))
            v = F(-v)
            x = self.parent[x]

    # ------------------------------------------------------- the schedule
    def _live(self, th: int) -> bool:
        return any(self.pos[self.leaves[th * self.B + j]].player != 0 for j in range(self.B))

    def _backup_thread(self, th: int) -> None:
        for j in range(self.B):
            i = th * self.B + j
            self._expand_and_backward(self.leaves[i], self.trans[i], self.policy[i], self.value[i])

    def _select_thread(self, th: int, steps: int, sel, pend, force: bool) -> None:
        while sel[th] < steps:
            for j in range(self.B):
                self._select_leaf(th * self.B + j, force)
            sel[th] += 1
            if self._live(th):
                pend[th] = True
                return
            self._backup_thread(th)

    def _evaluate_thread(self, th: int, nn) -> None:
        C = 1 + 2 * self.H
        f = np.zeros((self.B, C, 8, 8), np.float32)
        for j in range(self.B):
            i = th * self.B + j
            if self.pos[self.leaves[i]].player != 0:
                f[j] = O.features(self._chain(self.leaves[i]), self.H, self.trans[i])
        p, v = nn(f)
        self.policy[th * self.B:(th + 1) * self.B] = np.asarray(p, np.float32)
        self.value[th * self.B:(th + 1) * self.B] = np.asarray(v, np.float32)

    def search(self, nn, fast_simulations: int | None = None) -> int:
        """orc_mcts_search. fast_simulations = n: a fast search of a playout cap
        (n simulations, no root noise, no forcing)."""
        fast = fast_simulations is not None
        sims = fast_simulations if fast else self.S
        self.noise_eps = F(0.0) if fast else self.eps
        force = not fast
        T, B = self.T, self.B
        rows = T * B
        steps = (sims + rows - 1) // rows
        self.leaves, self.trans = [0] * rows, [0] * rows
        self.policy = np.zeros((rows, 65), np.float32)
        self.value = np.zeros(rows, np.float32)
        sel, pend = [0] * T, [False] * T
        for t in range(T):
            self._select_thread(t, steps, sel, pend, force)
        while True:
            waiting = [t for t in range(T) if pend[t]]
            if not waiting:
                break
            for t in waiting:
                self._evaluate_thread(t, nn)
            for t in range(T):
                if pend[t]:
                    self._backup_thread(t)
                    pend[t] = False
                    self._select_thread(t, steps, sel, pend, force)
        return steps * rows

    # ---------------------------------------------------------- the queries
    def _children(self):
        r = self.root
        return slice(self.first[r], self.first[r] + self.nch[r]) if self.nch[r] else slice(0, 0)

    def visit_counts(self) -> list[int]:
        return [int(x) for x in self.N[self._children()]]

    def mean_action_values(self) -> np.ndarray:
        return self.Q[self._children()].copy()

    def priors(self) -> np.ndarray:
        return self.P[self._children()].copy()

    def root_visit_count(self) -> int:
        return int(self.N[self.root])

    def node_count(self) -> int:
        return self.count

    def events(self) -> int:
        return self.event

    def pruned_counts(self, k) -> np.ndarray:
        return prune(self.root_visit_count(), self.visit_counts(), self.mean_action_values(), self.priors(),
                     self.c_base, self.c_init, k)

    def self_play_data(self, prune_k=None):
        """mcts.cpp:63-112; prune_k: the targets from the pruned counts."""
        r = self.root
        if self.pos[r].player == 0:
            raise ValueError("Self-play data cannot be generated from a terminal position.")
        if self.nch[r] == 0:
            raise ValueError("The root node has not been expanded yet.")
        acts = O.legal_actions(self.pos[r])
        n = self.visit_counts() if prune_k is None else [int(x) for x in self.pruned_counts(prune_k)]
        s = sum(n) or 1
        C = 1 + 2 * self.H
        f = np.zeros((8, C, 8, 8), np.float32)
        p = np.zeros((8, 65), np.float32)
        chain = self._chain(r)
        for t in range(8):
            f[t] = O.features(chain, self.H, t)
            for i, a in enumerate(acts):
                p[t, self.L.orc_transform_action(a, t)] = F(n[i]) / F(s)
        return f, p

    def apply_action(self, action: int) -> None:
        """mcts.cpp:114-165 (a legal action is the caller's business)."""
        r = self.root
        pos = self.pos[r]
        if self.nch[r] == 0:
            self.root = self._new_node(O.apply_action(pos, action), r)
            return
        idx = 0
        if action != 0 and self.nch[r] > 1:
            idx = bin(pos.legal & ((~0 << (64 - action)) & ((1 << 64) - 1))).count("1")
        self.root = self.first[r] + idx

    def selfplay_action(self, ply: int, temperature_moves: int = 12, temperature: float = 1.0) -> int:
        """orc_mcts_selfplay_action: the driver's move choice from the RAW visit
        counts, one event of the game's stream (not applied). The CPU tests check
        it against the oracle's; the GPU tests apply the engine's own action and
        use this only to keep the event count."""
        r = self.root
        if self.pos[r].player == 0:
            return -1
        acts = O.legal_actions(self.pos[r])
        n = self.visit_counts()
        nc, na = len(n), len(acts)
        ev = self.event
        self.event += 1
        u = F(self.L.orc_uniform(self.L.orc_stream_key(self.key, ev, 0), 0))
        if nc == 0:
            j = min(int(F(u * F(na))), na - 1)
        elif ply < temperature_moves:
            cdf, s = [], F(0.0)
            for x in n:
                s = F(s + F(_libm.powf(float(F(x)), float(F(1.0) / F(temperature)))))
                cdf.append(s)
            if s > 0:
                target = F(u * s)
                j = next((i for i, c in enumerate(cdf) if c > target), nc - 1)
            else:
                j = min(int(F(u * F(nc))), nc - 1)
        else:
            mx = max(n)
            ties = [i for i, x in enumerate(n) if x == mx]
            j = ties[min(int(F(u * F(len(ties)))), len(ties) - 1)]
        return acts[j]


# --------------------------------------------------------------------------
# The cases tests/test_gpu_forced_playouts.py runs on the engine, and the twin
# run that tells whether they can see the feature at all: per game a forced
# reference and an unforced one (forced_k = 0) that follow the same actions.
# Seeds were chosen on the CPU (tests/test_cpu_forced_playouts.py) so that the
# vacuity guards of ``Guard.check`` hold.
# --------------------------------------------------------------------------
K = 2.0
SHAPE_NOISE = dict(history_size=4, num_simulations=64, num_threads=2, batch_size=8, dirichlet_epsilon=0.25)
SHAPE_PLAIN = dict(history_size=4, num_simulations=64, num_threads=1, batch_size=8, dirichlet_epsilon=0.0)
CASES = {
    # name: (engine seed, games, plies, stub name, search shape, playout cap)
    "noise": (41, 8, 14, "equivariant", SHAPE_NOISE, None),
    "plain": (1, 8, 14, "equivariant", SHAPE_PLAIN, None),
    "asym": (41, 4, 14, "asymmetric", SHAPE_NOISE, None),
    "cap": (41, 8, 14, "equivariant", SHAPE_NOISE, (0.5, 16)),
}
# a root with 17 legal moves (the selection's scan over more than one DPP row)
# and one whose mover must pass (a single child, taken without scoring), both
# reached from the initial position (found with the oracle on random games)
WIDE_PREFIX = (19, 18, 37, 45, 17, 43, 53, 54, 34, 29, 20, 26, 38)
PASS_PREFIX = (26, 18, 44, 25, 24, 32, 10, 16)


def stub_of(name: str):
    import asym_stub

    return {"equivariant": O.equivariant_stub, "asymmetric": asym_stub.asymmetric_stub}[name]


class Guard:
    """What the feature changed over a run's full searches."""

    def __init__(self):
        self.searches = self.changed = self.pruned = self.zeroed = 0

    def check(self, zeroed: bool = False) -> None:
        assert self.searches > 0
        assert 4 * self.changed >= self.searches, (self.changed, self.searches)  # forcing moved a quarter of them
        assert 2 * self.pruned >= self.searches, (self.pruned, self.searches)  # pruning took a visit from half
        if zeroed:
            assert self.zeroed > 0


class Twin:
    """One game: the forced reference ``r`` and its unforced twin ``z``."""

    def __init__(self, key: int, shape: dict, k: float = K, prefix=()):
        self.k = k
        self.r = ForcedMCTS(game_key=key, forced_k=k, **shape)
        self.z = ForcedMCTS(game_key=key, **shape)
        for a in prefix:
            self.r.apply_action(int(a))
            self.z.apply_action(int(a))

    def search(self, stub, guard: Guard, fast_simulations: int | None = None) -> None:
        self.r.search(stub, fast_simulations)
        self.z.search(stub, fast_simulations)
        if fast_simulations is None:
            n = np.array(self.r.visit_counts())
            pc = self.r.pruned_counts(self.k)
            guard.searches += 1
            guard.changed += self.r.visit_counts() != self.z.visit_counts()
            guard.pruned += bool((pc < n).any())
            guard.zeroed += int(((pc == 0) & (n > 0)).sum())

    def own_move(self, ply: int) -> int:
        """the reference's own choice (CPU runs), applied to both"""
        a = self.r.selfplay_action(ply)
        self.z.selfplay_action(ply)
        self.r.apply_action(a)
        self.z.apply_action(a)
        return a

    def engine_move(self, action: int) -> None:
        """the engine's action (GPU runs): one event for its draw, no rule restated"""
        for m in (self.r, self.z):
            m.event += 1
            m.apply_action(int(action))


def case_twins(name: str):
    import asym_stub
    import playout_cap_ref

    seed, G, plies, stub, shape, cap = CASES[name]
    keys = [asym_stub.game_key(seed, g) for g in range(G)]
    full = np.ones((G, plies), bool)
    if cap is not None:
        full = np.array([[playout_cap_ref.is_full(k, ply, cap[0]) for ply in range(plies)] for k in keys])
    return keys, [Twin(k, shape) for k in keys], full, stub_of(stub)


def run_case_on_cpu(name: str) -> Guard:
    """The whole case with the reference's own moves."""
    seed, G, plies, _, shape, cap = CASES[name]
    _, twins, full, stub = case_twins(name)
    guard = Guard()
    for ply in range(plies):
        for g, t in enumerate(twins):
            t.search(stub, guard, None if full[g, ply] else cap[1])
            t.own_move(ply)
    return guard
