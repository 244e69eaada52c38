"""Generate tests/golden/baseline.npz: positions with the baseline opponents'
scores from the independent reference (tests/baseline_ref.py: unpruned negamax
in plain Python). Needs no GPU; the package is used for the seeded positions
only (othello_mcts.endgame.random_play_positions).

    python tests/golden/make_baseline.py [--jobs N]

Positions: PER_GROUP each from random play down to 44, 30 and 18 empties, and
PER_GROUP at 5..8 empties (group 3). Per position and case: move_scores (65)
and the first-maximum action. Cases: RANDOM, GREEDY, SEARCH at depths 1..4 on
every position, SEARCH at depths 6 and 8 on group 3 only (rows of the other
groups hold NONE / -1 there).

The generator asserts what the tests rely on and stores the counts: a root
with a forced pass (more positions are drawn and appended to group 3 until
there is one), cases whose search crosses a pass below the root, cases that
reach a finished game before their depth, and SEARCH cases with tied best
actions.
"""

from __future__ import annotations

import argparse
import multiprocessing as mp
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "othello-alphazero_amd"))

import baseline_ref as R  # noqa: E402

SEED = 2110
PER_GROUP = 32
GROUP_EMPTIES = (44, 30, 18)
LATE_EMPTIES = (5, 6, 7, 8)
# (kind, depth, group 3 only)
CASES = [(R.RANDOM, 0, False), (R.GREEDY, 0, False), (R.SEARCH, 1, False), (R.SEARCH, 2, False),
         (R.SEARCH, 3, False), (R.SEARCH, 4, False), (R.SEARCH, 6, True), (R.SEARCH, 8, True)]


def triple(p):
    return p.player(), p.player1_discs(), p.player2_discs()


def root_pass(pos) -> bool:
    player, p1, p2 = pos
    me, opp = (p1, p2) if player == 1 else (p2, p1)
    return not R.moves_of(me, opp) and bool(R.moves_of(opp, me))


def work(job):
    kind, depth, pos = job
    ms = R.move_scores(kind, depth, *pos)
    return ms, R.first_max(ms), R.STATS["passes"], R.STATS["early_terminals"]


def main() -> None:
    from othello_mcts.endgame import random_play_positions

    ap = argparse.ArgumentParser()
    ap.add_argument("--jobs", type=int, default=8)
    a = ap.parse_args()
    positions, group = [], []
    for g, e in enumerate(GROUP_EMPTIES):
        positions += [triple(p) for p in random_play_positions(e, PER_GROUP, SEED + g)]
        group += [g] * PER_GROUP
    for i, e in enumerate(LATE_EMPTIES):
        positions += [triple(p) for p in random_play_positions(e, PER_GROUP // len(LATE_EMPTIES), SEED + 10 + i)]
        group += [3] * (PER_GROUP // len(LATE_EMPTIES))
    extra_seed = SEED + 100
    while not any(root_pass(p) for p in positions):  # random play rarely leaves a root that must pass
        for p in random_play_positions(6, 64, extra_seed):
            if root_pass(triple(p)):
                positions.append(triple(p))
                group.append(3)
                break
        extra_seed += 1
    n = len(positions)
    group = np.array(group, np.int32)
    jobs = [(k, d, positions[i]) for (k, d, late) in CASES for i in range(n) if not late or group[i] == 3]
    with mp.Pool(a.jobs) as pool:
        done = iter(pool.map(work, jobs, chunksize=1))
    scores = np.full((len(CASES), n, 65), R.NONE, np.int32)
    action = np.full((len(CASES), n), -1, np.int32)
    passes = np.zeros((len(CASES), n), np.int32)
    early = np.zeros((len(CASES), n), np.int32)
    for c, (k, d, late) in enumerate(CASES):
        for i in range(n):
            if late and group[i] != 3:
                continue
            ms, act, np_, ne = next(done)
            scores[c, i], action[c, i], passes[c, i], early[c, i] = ms, act, np_, ne
    search = np.array([k == R.SEARCH for k, _, _ in CASES])
    best = scores.max(2, keepdims=True)
    tied = ((scores == best) & (best != R.NONE)).sum(2)
    counts = {
        "root_pass": int(sum(root_pass(p) for p in positions)),
        "pass_below_root": int((passes[search] > 0).sum()),
        "early_terminal": int((early[search] > 0).sum()),
        "tied_search": int((tied[search] >= 2).sum()),
        "tied3_search": int((tied[search] >= 3).sum()),
    }
    assert counts["root_pass"] >= 1, counts
    assert counts["pass_below_root"] >= 4, counts
    assert counts["early_terminal"] >= 4, counts
    assert counts["tied_search"] >= 16 and counts["tied3_search"] >= 1, counts
    np.savez_compressed(
        Path(__file__).with_name("baseline.npz"),
        player=np.array([p[0] for p in positions], np.int32),
        p1=np.array([p[1] for p in positions], np.uint64),
        p2=np.array([p[2] for p in positions], np.uint64),
        group=group,
        case_kind=np.array([k for k, _, _ in CASES], np.int32),
        case_depth=np.array([d for _, d, _ in CASES], np.int32),
        case_late_only=np.array([late for _, _, late in CASES], np.bool_),
        move_scores=scores, action=action, passes=passes, early_terminals=early,
        count_names=np.array(sorted(counts)), counts=np.array([counts[k] for k in sorted(counts)], np.int32))
    print(n, "positions;", counts)


if __name__ == "__main__":
    main()
