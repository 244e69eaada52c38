"""Generate tests/golden/endgames.npz: endgame positions with their exact
solutions from the independent reference (tests/endgame_ref.py over the
oracle's bitboards). Needs neither the GPU nor the package under test.

    python tests/golden/make_endgames.py [--jobs N]

Three sources, all seeded:
  * uniformly random play from the initial position down to E empties,
    E = 0..12 (PER_EMPTIES positions each), the side to move as it falls;
  * random games that ended before the board was full: terminal roots with
    empties left (up to EARLY_TERMINAL of them, at most 12 empties);
  * constructed boards, because random play almost never produces a wipeout
    and rarely a root that must pass: a board full of one colour except for E
    random empties and one or two discs of the other colour, side to move at
    random. Of these, the first N_WIPEOUT whose perfect play ends with one
    side discless and the first N_ROOT_PASS whose root must pass are kept.
    They are not reachable in a game; the solver does not care.

Per position: player, p1, p2, empties, move_scores (65), score, best_action and
`kinds` (bits of endgame_ref: root pass, terminal root, pass inside the line
of perfect play, game ends with empties, wipeout). tests/test_cpu_endgame.py
asserts at least five of each kind, both colours, and E = 0, 1, 2.
"""

from __future__ import annotations

import argparse
import multiprocessing as mp
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
for p in (ROOT / "oracle", ROOT / "tests"):
    sys.path.insert(0, str(p))

import endgame_ref as R  # noqa: E402
import oracle as O  # noqa: E402

SEED = 20260
PER_EMPTIES = {0: 8, 1: 24, 2: 24, 3: 24, 4: 24, 5: 24, 6: 24, 7: 24, 8: 24, 9: 20, 10: 16, 11: 12, 12: 10}
EARLY_TERMINAL, N_WIPEOUT, N_ROOT_PASS = 12, 8, 8


def random_play(rng: np.random.RandomState, empties: int):
    """(player, p1, p2) after random play down to `empties` empties; the second
    value says whether the game ended before (the position is then terminal)."""
    p = O.initial_position()
    while p.player != 0 and R.popcount(R.FULL & ~(p.p1 | p.p2)) > empties:
        acts = O.legal_actions(p)
        p = O.apply_action(p, acts[rng.randint(len(acts))])
    return (p.player, p.p1, p.p2), R.popcount(R.FULL & ~(p.p1 | p.p2)) > empties


def constructed(rng: np.random.RandomState):
    e = rng.randint(2, 9)
    sq = rng.permutation(64)
    empty = sum(1 << int(s) for s in sq[:e])
    few = sum(1 << int(s) for s in sq[e:e + rng.randint(1, 3)])
    many = R.FULL & ~(empty | few)
    p1, p2 = (many, few) if rng.randint(2) else (few, many)
    return 1 + int(rng.randint(2)), p1, p2


def solve_one(pos):
    ms, score, best = R.solve(*pos)
    return ms, score, best, R.kinds(*pos)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    rng = np.random.RandomState(SEED)
    positions, early = [], []
    for e, count in PER_EMPTIES.items():
        got = 0
        while got < count:
            pos, ended = random_play(rng, e)
            if ended:
                if len(early) < EARLY_TERMINAL and R.popcount(R.FULL & ~(pos[1] | pos[2])) <= 12:
                    early.append(pos)
                continue
            positions.append(pos)
            got += 1
    positions += early
    candidates = [constructed(rng) for _ in range(600)]
    with mp.Pool(a.jobs) as pool:
        solved = pool.map(solve_one, positions, chunksize=1)
        cand = pool.map(solve_one, candidates, chunksize=8)
    wipe = [i for i, s in enumerate(cand) if s[3] & R.WIPEOUT and not s[3] & R.ROOT_TERMINAL][:N_WIPEOUT]
    rpass = [i for i, s in enumerate(cand) if s[3] & R.ROOT_PASS and i not in wipe][:N_ROOT_PASS]
    for i in wipe + rpass:
        positions.append(candidates[i])
        solved.append(cand[i])
    n = len(positions)
    out = {
        "player": np.array([p[0] for p in positions], np.int32),
        "p1": np.array([p[1] for p in positions], np.uint64),
        "p2": np.array([p[2] for p in positions], np.uint64),
        "empties": np.array([R.popcount(R.FULL & ~(p[1] | p[2])) for p in positions], np.int32),
        "move_scores": np.array([s[0] for s in solved], np.int32).reshape(n, 65),
        "score": np.array([s[1] for s in solved], np.int32),
        "best_action": np.array([s[2] for s in solved], np.int32),
        "kinds": np.array([s[3] for s in solved], np.int32),
    }
    np.savez_compressed(Path(__file__).with_name("endgames.npz"), **out)
    k = out["kinds"]
    print(n, "positions;", {name: int((k & bit != 0).sum()) for name, bit in
                            (("root_pass", R.ROOT_PASS), ("terminal", R.ROOT_TERMINAL), ("pass_inside", R.PASS_INSIDE),
                             ("ends_with_empties", R.ENDS_WITH_EMPTIES), ("wipeout", R.WIPEOUT))},
          "black", int((out["player"] == 1).sum()), "white", int((out["player"] == 2).sum()),
          "empties", np.bincount(out["empties"]).tolist())


if __name__ == "__main__":
    main()
