"""Test reference for exact leaf values.

The rule, on top of the Python restatement of the oracle's search in
tests/forced_ref.py (imported unmodified, ``forced_k = 0``):

1. a child created by an expansion that is not terminal and has at most E
   empties is an exact leaf, *pending*;
2. a node that becomes the root loses its mark;
3. a descent stops at an exact leaf; like a terminal leaf it has no NN row,
   draws no symmetry and is no evaluation;
4. a pending leaf that was selected is solved before its batch is backed up
   (every row that found it pending is solved and counted);
5. its backup expands nothing and gives the path what a terminal leaf whose
   score for the parent's player is -s would give; the node is then *solved*;
6. a batch waits for the evaluation round trip if it holds an NN row or a
   pending leaf; terminal and solved leaves alone are backed up at once.

s comes from the host ``solve_position`` (the sign of its exact score); the
node count of a solve from ``exact_leaf_value(..., return_nodes=True)``, whose
sign must agree. ``hits`` records which branches a run took.
"""

from __future__ import annotations

import numpy as np

import forced_ref as R
import oracle as O

F = np.float32
PLAIN, PENDING = -1, -2  # NodeLink.first_child of a childless node; solved: -4 - s
BRANCHES = ("pending", "solved_hit", "pass_leaf", "double_pending", "skip_solved", "root_cleared")

_solved: dict = {}


def empties(pos) -> int:
    return 64 - bin(pos.p1 | pos.p2).count("1")


def solve(pos, E: int) -> tuple[int, int]:
    """(s, nodes) of an exact leaf: s from solve_position, nodes from the host rule."""
    import othello_mcts as om

    key = (pos.player, pos.p1, pos.p2, E)
    if key not in _solved:
        sol = om.solve_position((pos.player, pos.p1, pos.p2), max_empties=E)
        assert sol["flags"] == 0 and sol["best_action"] >= 0, sol
        s = int(np.sign(sol["score"]))
        value, nodes = om.exact_leaf_value((pos.player, pos.p1, pos.p2), E, return_nodes=True)
        assert value == s, (value, s)
        _solved[key] = (s, int(nodes))
    return _solved[key]


class ExactMCTS(R.ForcedMCTS):
    """One game's search with exact leaves at ``max_empties`` (0 = off)."""

    def __init__(self, max_empties: int = 0, hits: set | None = None, **kw):
        self.E = int(max_empties)
        self.hits = hits if hits is not None else set()
        self.solves = self.solved_hits = self.solver_nodes = self.evals = 0
        super().__init__(forced_k=0.0, **kw)

    # ------------------------------------------------------------- the tree
    def reset_position(self) -> None:
        self.mark = []
        super().reset_position()

    def _new_node(self, pos, parent) -> int:
        i = super()._new_node(pos, parent)
        self.mark.append(PLAIN)
        return i

    def apply_action(self, action: int) -> None:
        super().apply_action(action)
        if self.mark[self.root] != PLAIN:  # rule 2
            self.hits.add("root_cleared")
            self.mark[self.root] = PLAIN

    # ------------------------------------------------------------ selection
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
        m = self.mark[node]
        self.xflag[i] = -1 - m  # 0 none, 1 pending, 2 / 3 / 4 the result
        self.trans[i] = 0
        if m == PENDING:
            self.hits.add("pending")
            if O.legal_actions(self.pos[node]) == [64]:
                self.hits.add("pass_leaf")
            if any(self.xflag[j] == 1 and self.leaves[j] == node and self.live_row[j] for j in range(len(self.leaves))
                   if j != i):
                self.hits.add("double_pending")
        elif m != PLAIN:
            self.hits.add("solved_hit")
            self.solved_hits += 1
        elif self.pos[node].player != 0:
            ev = self.event
            self.event += 1
            self.trans[i] = self.L.orc_mix64(self.L.orc_stream_key(self.key, ev, 0)) >> 61
            self.evals += 1
        self.live_row[i] = True  # selected and not backed up yet

    def _nn_row(self, i: int) -> bool:
        return self.xflag[i] == 0 and self.pos[self.leaves[i]].player != 0

    # --------------------------------------------------------------- backup
    def _backup_row(self, i: int) -> None:
        leaf = self.leaves[i]
        self.live_row[i] = False
        if self.xflag[i] == 0:
            self._expand_and_backward(leaf, self.trans[i], self.policy[i], self.value[i])
            return
        if self.xflag[i] == 1:  # rule 4: every row that found the leaf pending is solved
            s, nodes = solve(self.pos[leaf], self.E)
            self.solves += 1
            self.solver_nodes += nodes
            self.mark[leaf] = -4 - s
        else:
            s = self.xflag[i] - 3
        v = F(-1.0 if s > 0 else (1.0 if s < 0 else 0.0))  # a terminal leaf scoring -s for the parent's player
        x = leaf
        while x != self.root:
            self.W[x] = F(self.W[x] + F(F(1.0) + v))
            self.Q[x] = F(self.W[x] / F(self.N[x]))
            v = F(-v)
            x = self.parent[x]

    def _expand_and_backward(self, leaf: int, t: int, policy, value) -> None:
        first = self.count
        super()._expand_and_backward(leaf, t, policy, value)
        for c in range(first, self.count):  # rule 1, both expansion sites
            p = self.pos[c]
            if self.E > 0 and p.player != 0 and empties(p) <= self.E:
                self.mark[c] = PENDING

    def _backup_thread(self, th: int) -> None:
        for j in range(self.B):
            self._backup_row(th * self.B + j)

    # ------------------------------------------------------------- schedule
    def _live(self, th: int) -> bool:
        rows = range(th * self.B, (th + 1) * self.B)
        live = any(self._nn_row(i) or self.xflag[i] == 1 for i in rows)
        if not live and any(self.xflag[i] >= 2 for i in rows):
            self.hits.add("skip_solved")
        return live

    def _evaluate_thread(self, th: int, nn) -> None:
        C = 1 + 2 * self.H
        f = np.zeros((self.B, C, 8, 8), np.float32)
        for j in range(self.B):
            i = th * self.B + j
            if self._nn_row(i):
                f[j] = O.features(self._chain(self.leaves[i]), self.H, self.trans[i])
        p, v = nn(f)
        self.policy[th * self.B:(th + 1) * self.B] = np.asarray(p, np.float32)
        self.value[th * self.B:(th + 1) * self.B] = np.asarray(v, np.float32)

    def search(self, nn, fast_simulations: int | None = None) -> int:
        rows = self.T * self.B
        self.xflag = [0] * rows
        self.live_row = [False] * rows
        return super().search(nn, fast_simulations)

    def counters(self) -> dict:
        return {"solves": self.solves, "hits": self.solved_hits, "nodes": self.solver_nodes}


# --------------------------------------------------------------------------
# Fixtures: a fixed game prefix played down to few empties (chosen on the CPU,
# tests/test_cpu_exact_leaves.py asserts that the six branches are all hit).
# --------------------------------------------------------------------------
def play_prefix(seed: int, target_empties: int) -> tuple[int, ...]:
    """Actions of seeded uniformly random play from the initial position down
    to ``target_empties`` empties (a game that ends earlier is dropped and the
    next one of the seeded stream taken)."""
    import random

    rng = random.Random(seed)
    while True:
        p, acts = O.initial_position(), []
        while p.player != 0 and empties(p) > target_empties:
            a = rng.choice(O.legal_actions(p))
            acts.append(a)
            p = O.apply_action(p, a)
        if p.player != 0:
            return tuple(acts)


SHAPES = {"1x4": dict(num_threads=1, batch_size=4), "2x8": dict(num_threads=2, batch_size=8),
          "2x16": dict(num_threads=2, batch_size=16)}
# name: (prefix seed, empties at the first searched root, E, shape, simulations, plies searched)
FIXTURES = {
    "e1": (3, 8, 1, "1x4", 64, 6),
    "e4": (5, 10, 4, "2x8", 128, 6),
    "e6": (7, 12, 6, "2x16", 192, 6),
    "e4_wide": (11, 9, 4, "2x16", 128, 5),
}


def fixture_game(name: str, key: int = 0, hits: set | None = None, eps: float = 0.25) -> tuple[ExactMCTS, int]:
    seed, start, E, shape, sims, plies = FIXTURES[name]
    m = ExactMCTS(max_empties=E, hits=hits, history_size=4, num_simulations=sims, dirichlet_epsilon=eps, game_key=key,
                  **SHAPES[shape])
    for a in play_prefix(seed, start):
        m.apply_action(int(a))
    return m, plies


def run_fixture_on_cpu(name: str, stub, hits: set) -> ExactMCTS:
    """The fixture with the reference's own moves (argmax of the visits, the first of the largest)."""
    m, plies = fixture_game(name, hits=hits)
    for _ in range(plies):
        if m.position().player == 0:
            break
        m.search(stub)
        n = m.visit_counts()
        m.apply_action(O.legal_actions(m.position())[int(np.argmax(n))])
    return m
