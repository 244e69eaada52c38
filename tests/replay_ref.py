"""Numpy restatement of the packed replay buffer (csrc/replay.hip): pack,
commit and gather, plus synthetic self-play outputs to feed it with.

The two halves are independent on purpose. ``synthetic_move`` builds the 8
transformed feature / policy slices of a move by SCATTERING through the forward
transform as transformation.h defines it (optional horizontal flip, then t / 2
clockwise rotations). ``ReplayRef.gather`` rebuilds them by INDEXING through
the inverse map, found by search. tests/test_cpu_replay.py pins the pair
against ``SampleBuffer``, which never transforms anything.
"""

from __future__ import annotations

import numpy as np

FIN_NO_TARGETS, FIN_OVERFLOW = 4, 8
FLAG_OVERFLOW, FLAG_NO_TARGETS, FLAG_TOO_LONG, FLAG_BAD_ID = 1, 2, 4, 8
_OUTCOME = np.array([0.0, 0.0, 1.0, -1.0], dtype=np.float32)  # finished bits 0-1 -> outcome for black


def transform_action(a: int, t: int) -> int:
    """transformation.h:40-57: flip the columns when t is odd, then t // 2
    clockwise rotations (row, col) -> (col, 7 - row); the pass stays."""
    if a == 64:
        return 64
    row, col = divmod(a, 8)
    if t & 1:
        col = 7 - col
    for _ in range(t >> 1):
        row, col = col, 7 - row
    return row * 8 + col


# FWD[t][sq] = where square sq goes; INV[t][sq'] = the square shown at sq'
FWD = np.array([[transform_action(s, t) for s in range(64)] for t in range(8)])
INV = np.array([[int(np.nonzero(FWD[t] == s)[0][0]) for s in range(64)] for t in range(8)])


def board_bits(boards: np.ndarray) -> np.ndarray:
    """(..., ) uint64 -> (..., 64) 0/1 by square: square i is bit 63 - i."""
    shifts = np.uint64(63) - np.arange(64, dtype=np.uint64)
    return ((boards[..., None] >> shifts) & np.uint64(1)).astype(np.float32)


def synthetic_move(rng: np.random.Generator, G: int, H: int, actions, finished, player=None) -> dict[str, np.ndarray]:
    """One move's outputs in the self-play driver's layout, from random
    bitboards, a random side to move (or ``player``: 0 black, 1 white per game)
    and a random policy per game."""
    C = 1 + 2 * H
    boards = rng.integers(0, 1 << 63, size=(G, 2 * H), dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, size=(G, 2 * H), dtype=np.uint64)
    boards[rng.random((G, 2 * H)) < 0.15] = 0  # empty history planes, as early in a game
    player = rng.integers(0, 2, size=G) if player is None else np.asarray(player)
    p0 = rng.random((G, 65)).astype(np.float32)
    p0[rng.random((G, 65)) < 0.5] = 0.0
    p0 /= np.maximum(p0.sum(1, keepdims=True), np.float32(1e-6))
    bits = board_bits(boards)  # (G, 2H, 64)
    features = np.zeros((G, 8, C, 64), dtype=np.float32)
    policy = np.zeros((G, 8, 65), dtype=np.float32)
    for t in range(8):
        ft, pt = features[:, t], policy[:, t]  # views
        ft[:, 0, :] = player[:, None]
        ft[:, 1:, FWD[t]] = bits  # square sq is shown at FWD[t][sq]
        pt[:, FWD[t]] = p0[:, :64]
        pt[:, 64] = p0[:, 64]
    return {"actions": np.asarray(actions, dtype=np.int32), "finished": np.asarray(finished, dtype=np.int32),
            "features": features.reshape(G, 8, C, 8, 8), "policy": policy}


def random_script(rng: np.random.Generator, G: int, H: int, n_moves: int, max_len: int = 6) -> list[dict]:
    """n_moves moves of G games: every game plays a random number of moves in
    [1, max_len] and then finishes with a random outcome (draws included),
    sometimes after sitting out a few moves (action -1) first."""
    left = rng.integers(1, max_len + 1, size=G)
    idle = rng.integers(0, 3, size=G) * (rng.random(G) < 0.3)
    moves = []
    for _ in range(n_moves):
        actions = np.full(G, -1, dtype=np.int32)
        finished = np.zeros(G, dtype=np.int32)
        for g in range(G):
            if idle[g] > 0:
                idle[g] -= 1
                continue
            actions[g] = rng.integers(0, 65)
            left[g] -= 1
            if left[g] == 0:
                finished[g] = rng.integers(1, 4)
                left[g] = rng.integers(1, max_len + 1)
                idle[g] = rng.integers(0, 3) * (rng.random() < 0.3)
        moves.append(synthetic_move(rng, G, H, actions, finished))
    return moves


def stack(moves: list[dict]) -> dict[str, np.ndarray]:
    """The selfplay_steps(keep_all=True) layout of consecutive moves."""
    return {k: np.stack([m[k] for m in moves]) for k in moves[0]}


class ReplayRef:
    """What ReplayBuffer must hold and return, in numpy."""

    def __init__(self, num_games: int, history_size: int, capacity: int, max_moves: int = 128) -> None:
        G, H2, M = num_games, 2 * history_size, max_moves
        self.G, self.H, self.capacity, self.max_moves = num_games, history_size, capacity, max_moves
        self.boards = np.zeros((capacity, H2), dtype=np.uint64)
        self.policy = np.zeros((capacity, 65), dtype=np.float32)
        self.value = np.zeros(capacity, dtype=np.float32)
        self.player = np.zeros(capacity, dtype=np.uint8)
        self.stage_boards = np.zeros((G, M, H2), dtype=np.uint64)
        self.stage_policy = np.zeros((G, M, 65), dtype=np.float32)
        self.stage_player = np.zeros((G, M), dtype=np.uint8)
        self.moves = np.zeros(G, dtype=np.int32)
        self.head = self.size = self.games_completed = self.flags = 0

    @staticmethod
    def pack(planes: np.ndarray) -> np.ndarray:
        """(n, 8, 8) planes -> (n,) uint64, square i in bit 63 - i."""
        on = planes.reshape(planes.shape[0], 64) != 0
        weights = np.uint64(1) << (np.uint64(63) - np.arange(64, dtype=np.uint64))
        return (on * weights).sum(axis=1, dtype=np.uint64)

    def add(self, out: dict[str, np.ndarray]) -> None:
        if out["actions"].ndim == 2:
            for i in range(out["actions"].shape[0]):
                self._add_move({k: v[i] for k, v in out.items()})
        else:
            self._add_move(out)

    def _add_move(self, out: dict[str, np.ndarray]) -> None:
        commit = []  # (game, staged moves, outcome for black), ascending game order
        for g in range(self.G):
            fin, played = int(out["finished"][g]), out["actions"][g] >= 0
            m = int(self.moves[g])
            err = (FLAG_OVERFLOW if fin & FIN_OVERFLOW else 0) | \
                (FLAG_NO_TARGETS if played and fin & FIN_NO_TARGETS else 0) | \
                (FLAG_TOO_LONG if played and m >= self.max_moves else 0)
            self.flags |= err
            if played and not err:
                f0 = out["features"][g, 0]  # only the untransformed slice is kept
                self.stage_boards[g, m] = self.pack(f0[1:])
                self.stage_player[g, m] = f0[0, 0, 0] != 0
                self.stage_policy[g, m] = out["policy"][g, 0]
                m += 1
            if fin & 3:
                if err:
                    m = 0  # the game is dropped
                else:
                    commit.append((g, m, _OUTCOME[fin & 3]))
            self.moves[g] = m
        total = sum(n for _, n, _ in commit)
        j = 0
        for g, n, outcome in commit:
            for k in range(n):
                if total - j <= self.capacity:  # else a later position of this commit overwrites it
                    slot = (self.head + j) % self.capacity
                    self.boards[slot] = self.stage_boards[g, k]
                    self.policy[slot] = self.stage_policy[g, k]
                    self.player[slot] = self.stage_player[g, k]
                    self.value[slot] = outcome * np.float32(-1.0 if self.stage_player[g, k] else 1.0)
                j += 1
            self.moves[g] = 0
            self.games_completed += 1
        self.head = (self.head + total) % self.capacity
        self.size = min(self.capacity, self.size + total)

    def gather(self, ids) -> tuple[np.ndarray, np.ndarray, np.ndarray]:
        ids = np.asarray(ids, dtype=np.int64)
        n, C = ids.shape[0], 1 + 2 * self.H
        features = np.zeros((n, C, 64), dtype=np.float32)
        policy = np.zeros((n, 65), dtype=np.float32)
        value = np.zeros(n, dtype=np.float32)
        for i, s in enumerate(ids.tolist()):
            if not 0 <= s < 8 * self.size:
                self.flags |= FLAG_BAD_ID
                continue
            t = s & 7
            slot = (self.head - self.size + (s >> 3)) % self.capacity
            features[i, 0] = self.player[slot]
            features[i, 1:] = board_bits(self.boards[slot])[:, INV[t]]
            policy[i, :64] = self.policy[slot, INV[t]]
            policy[i, 64] = self.policy[slot, 64]
            value[i] = self.value[slot]
        return features.reshape(n, C, 8, 8), policy, value
