"""Numpy restatement of the replay buffer's exact endgame value targets
(csrc/replay.hip k_replay_endgame_list / k_replay_endgame_apply, DESIGN.md
§14), built on ``replay_ref.ReplayRef`` (the ring) and ``endgame_ref.solve``
(the independent solver), plus self-play outputs made from given positions.

``RelabelRef`` shares no code with the kernels: candidates are found by a
plain loop over the live positions in age order, and the exact result comes
from the Python negamax. ``solve`` can be replaced by a table of results the
same reference produced earlier (tests/golden/endgames.npz), because the
recursion takes seconds per position from 10 empties on. The reference cannot
count the device solver's nodes, so which positions a ``node_limit`` stops is
an input (``gives_up``), taken by the tests from the host solver.
"""

from __future__ import annotations

from pathlib import Path

import numpy as np

import endgame_ref
import replay_ref
from replay_ref import FIN_NO_TARGETS, FIN_OVERFLOW, FWD, ReplayRef

EXACT_UNKNOWN, EXACT_GAVE_UP = -128, -127
INITIAL = (1, 0x0000000810000000, 0x0000001008000000)  # black to move, 60 empties: never a candidate


def popcount(x: int) -> int:
    return bin(int(x)).count("1")


def mover_score(player: int, score: int, best_action: int) -> int:
    """The solver's score from the view of the side to move: a root with
    actions is scored for its mover already, a terminal root as black minus
    white."""
    return score if best_action >= 0 or player == 1 else -score


def optimal_policy(move_scores, score: int) -> np.ndarray:
    """1/m on the m actions (pass included) whose score is the position's."""
    best = np.asarray(move_scores) == score
    return np.where(best, np.float32(1.0) / np.float32(best.sum()), np.float32(0.0)).astype(np.float32)


def fixture() -> dict[str, np.ndarray]:
    z = np.load(Path(__file__).parent / "golden" / "endgames.npz")
    return {k: z[k] for k in z.files}


def fixture_positions(f=None) -> list[tuple[int, int, int]]:
    f = f or fixture()
    return [(int(a), int(b), int(c)) for a, b, c in zip(f["player"], f["p1"], f["p2"])]


def replay_positions(f=None) -> list[tuple[int, int, int]]:
    """The fixture's positions as replay records can hold them: a record always
    has a side to move, so the fixture's terminal roots (player 0) get black
    and white in turn."""
    return [(player or 1 + i % 2, p1, p2) for i, (player, p1, p2) in enumerate(fixture_positions(f))]


def table_solver(f=None):
    """``endgame_ref.solve`` with the fixture's stored results (which it
    produced) looked up instead of searched again; any other position is
    searched."""
    f = f or fixture()
    table = {p: (f["move_scores"][i].tolist(), int(f["score"][i]), int(f["best_action"][i]))
             for i, p in enumerate(fixture_positions(f))}

    def solve(player, p1, p2):
        key = (int(player), int(p1), int(p2))
        return table[key] if key in table else endgame_ref.solve(*key)

    return solve


class RelabelRef(ReplayRef):
    """``ReplayRef`` with the ``exact`` ring and ``relabel_endgames``."""

    def __init__(self, num_games, history_size, capacity, max_moves=128, solve=endgame_ref.solve) -> None:
        super().__init__(num_games, history_size, capacity, max_moves)
        self.exact = np.full(capacity, EXACT_UNKNOWN, dtype=np.int8)
        self.relabel_counters = np.zeros(4, dtype=np.int64)
        self.solve = solve

    def _add_move(self, out) -> None:
        # the positions this move commits: the staged moves of every game that finishes without an error row
        total = 0
        for g in range(self.G):
            fin, played = int(out["finished"][g]), out["actions"][g] >= 0
            m = int(self.moves[g])
            err = fin & FIN_OVERFLOW or (played and (fin & FIN_NO_TARGETS or m >= self.max_moves))
            if fin & 3 and not err:
                total += m + (1 if played else 0)
        head = self.head
        super()._add_move(out)
        assert self.head == (head + total) % self.capacity
        for j in range(max(0, total - self.capacity), total):  # the slots the commit wrote
            self.exact[(head + j) % self.capacity] = EXACT_UNKNOWN

    def live_slots(self) -> np.ndarray:
        return (self.head - self.size + np.arange(self.size)) % self.capacity

    def exact_scores(self) -> np.ndarray:
        return self.exact[self.live_slots()]

    def relabel_endgames(self, max_empties=10, budget=4096, policy="keep", retry=False, gives_up=None) -> None:
        """``gives_up(player, p1, p2) -> bool``: the positions a node limit
        stops. Overlapping discs always give up."""
        taken = left = 0
        for slot in self.live_slots().tolist():
            e = int(self.exact[slot])
            if e != EXACT_UNKNOWN and not (retry and e == EXACT_GAVE_UP):
                continue
            p1, p2 = int(self.boards[slot, 0]), int(self.boards[slot, 1])
            if 64 - popcount(p1 | p2) > max_empties:
                continue
            if taken == budget:
                left += 1
                continue
            taken += 1
            player = int(self.player[slot]) + 1
            if p1 & p2 or (gives_up is not None and gives_up(player, p1, p2)):
                self.exact[slot] = EXACT_GAVE_UP
                self.relabel_counters[1] += 1
                continue
            move_scores, score, best = self.solve(player, p1, p2)
            s = mover_score(player, score, best)
            self.exact[slot] = s
            self.value[slot] = np.float32(np.sign(s))
            if policy == "optimal" and best >= 0:
                self.policy[slot] = optimal_policy(move_scores, score)
            self.relabel_counters[0] += 1
        self.relabel_counters[2:] = left, taken


def position_move(rng: np.random.Generator, G: int, H: int, records, finished) -> dict[str, np.ndarray]:
    """One move's outputs in the self-play driver's layout. ``records[g]``:
    the ``(player, p1, p2)`` game g moves from (player 1 black, 2 white), or
    None when it sits the move out (action -1). History step 0 holds the
    position; the older steps and the policy are random. Scattered through the
    forward transform, as ``replay_ref.synthetic_move`` does."""
    C = 1 + 2 * H
    boards = rng.integers(0, 1 << 63, size=(G, 2 * H), dtype=np.uint64)
    white = np.zeros(G, dtype=np.int64)
    actions = np.full(G, -1, dtype=np.int32)
    for g, r in enumerate(records):
        if r is not None:
            white[g] = r[0] - 1
            boards[g, 0], boards[g, 1] = np.uint64(r[1]), np.uint64(r[2])
            actions[g] = rng.integers(0, 65)
    p0 = rng.random((G, 65)).astype(np.float32)
    p0[rng.random((G, 65)) < 0.5] = 0.0
    p0 /= np.maximum(p0.sum(1, keepdims=True), np.float32(1e-6))
    bits = replay_ref.board_bits(boards)
    features = np.zeros((G, 8, C, 64), dtype=np.float32)
    policy = np.zeros((G, 8, 65), dtype=np.float32)
    for t in range(8):
        ft, pt = features[:, t], policy[:, t]
        ft[:, 0, :] = white[:, None]
        ft[:, 1:, FWD[t]] = bits
        pt[:, FWD[t]] = p0[:, :64]
        pt[:, 64] = p0[:, 64]
    return {"actions": actions, "finished": np.asarray(finished, dtype=np.int32),
            "features": features.reshape(G, 8, C, 8, 8), "policy": policy}


def games_script(rng: np.random.Generator, G: int, H: int, games) -> list[dict]:
    """Self-play outputs of ``games``: a list of ``(positions, outcome)``, the
    ``(player, p1, p2)`` records of one game in order (None: a filler record,
    the initial position) and its finished code (1 draw, 2 black won, 3 white
    won). Game k runs in lane k % G after the lane's earlier games, so with
    G = 1 the ring holds the records in the order given."""
    lanes = [[] for _ in range(G)]
    for k, (positions, outcome) in enumerate(games):
        assert positions and outcome in (1, 2, 3)
        for n, r in enumerate(positions):
            lanes[k % G].append((INITIAL if r is None else r, outcome if n == len(positions) - 1 else 0))
    moves = []
    for step in range(max(len(lane) for lane in lanes)):
        now = [lane[step] if step < len(lane) else (None, 0) for lane in lanes]
        moves.append(position_move(rng, G, H, [r for r, _ in now], [f for _, f in now]))
    return moves


def disagreeing_outcome(player: int, s: int, k: int) -> int:
    """A finished code whose value for ``player`` differs from sign(s), the
    exact score for that player; ``k`` picks between the two candidates."""
    # value for black of codes 1, 2, 3 is 0, +1, -1; for white it is negated
    want = np.sign(s) * (1 if player == 1 else -1)  # the code that would AGREE, as black's value
    others = [c for c, v in ((1, 0), (2, 1), (3, -1)) if v != want]
    return others[k % 2]
