"""The round schedule of k_tree's chain splitting (csrc/tree_search.h search_round, DESIGN.md §7
"Exact endgames"), restated as a small model: per game, virtual threads are
visited cyclically from the round's resume thread; a visit backs up the
thread's waiting batch and selects, re-selecting at once while batches come
back all terminal (search_thread.cpp:102-127); after `budget` re-selections
in a round a chain may stop (at most `cuts` times per search) and the next
round resumes it. The model checks, over random terminal patterns, that the
split schedule performs exactly the unsplit schedule's operations in the same
order and completes within steps + cuts selecting rounds (the extra rounds the
host runs). The GPU test test_chain_split_keeps_every_game_identical checks
the kernel itself against the unsplit callback path.

The adaptive extra-round count (capi.hip pick_extra_rounds) reads back the
cuts each game used, or cuts + 1 when a chain went past the budget with no
cut left (k_tree `over`); the model checks that this report is exactly the
cuts an unlimited search uses whenever it is <= the limit.

The host side of the schedule (csrc/schedule.h: the group split, the rounds
and launches of a search, the extra-round cap and the adaptive controller) is
compiled with g++ and held against bench.py's restatement and the rule of
include/othello_mcts_amd_experimental.h."""

import ctypes
import itertools
import random
import subprocess
import sys
import types
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def run_schedule(T, steps, budget, cuts_max, terminal, report=None):
    """Operations ('S'elect / 'B'ackup, thread, batch) of one search; budget 0
    = the unsplit schedule (steps + 1 rounds). report: a list that receives
    the cuts the search reports (k_tree's cuts_out)."""
    X = cuts_max if budget > 0 else 0
    S = steps + X
    sel = [0] * T
    pend = [False] * T
    rp = cuts = 0
    over = False
    ops = []
    for s in range(S + 1):
        do_select, do_backup = s < S, s > 0
        if s == 0:  # a search's first round starts every thread fresh
            sel, pend, rp, cuts = [0] * T, [False] * T, 0, 0
        chain, cut_at = 0, -1
        for k in range(T):
            if cut_at >= 0:
                break
            t = (rp + k) % T
            if do_backup and pend[t]:
                ops.append(("B", t, sel[t]))
                pend[t] = False
            again = False
            while do_select and not pend[t] and sel[t] < steps:
                if again and budget > 0 and chain >= budget:
                    if cuts < cuts_max:
                        cut_at, cuts = t, cuts + 1
                        break
                    over = True  # no cut left: the chain runs on
                sel[t] += 1
                ops.append(("S", t, sel[t]))
                if terminal(t, sel[t]):
                    ops.append(("B", t, sel[t]))
                    again, chain = True, chain + 1
                else:
                    pend[t] = True
        if budget > 0 and cut_at >= 0:
            rp = cut_at
    if report is not None:
        report.append(cuts_max + 1 if over else cuts)
    return ops, sel, pend


def test_chain_split_schedule_keeps_order_and_completes():
    rng = random.Random(1)
    for _ in range(3000):
        T = rng.choice([1, 2, 3, 4])
        steps = rng.randint(1, 12)
        p = rng.random()
        tab = {(t, k): rng.random() < p for t in range(T) for k in range(1, steps + 1)}
        term = lambda t, k: tab[(t, k)]  # noqa: E731
        ref, _, _ = run_schedule(T, steps, 0, 0, term)
        budget, cuts = rng.randint(1, 8), rng.randint(1, 5)
        ops, sel, pend = run_schedule(T, steps, budget, cuts, term)
        assert ops == ref, (T, steps, budget, cuts)
        assert sel == [steps] * T and not any(pend)


def test_chain_split_needs_the_first_round_reset():
    """A split in a search's first round leaves later threads unvisited: their
    state must still start fresh (the kernel resets every thread at round 0)."""
    term = lambda t, k: True  # noqa: E731  (a terminal root: every batch is terminal)
    ops, sel, pend = run_schedule(2, 10, 1, 3, term)
    assert sel == [10, 10] and ops == run_schedule(2, 10, 0, 0, term)[0]


def test_cut_report_is_the_unlimited_demand():
    """X = cuts_max extra rounds, X from 0 (the adaptive count outside the
    endgame: budget kept, no cut allowed) up: the order of operations never
    changes, and the report is the cuts an unlimited search uses when that is
    <= X, X + 1 otherwise."""
    rng = random.Random(2)
    for _ in range(3000):
        T = rng.choice([1, 2, 3, 4])
        steps = rng.randint(1, 16)
        p = rng.random()
        tab = {(t, k): rng.random() < p for t in range(T) for k in range(1, steps + 1)}
        term = lambda t, k: tab[(t, k)]  # noqa: E731
        budget = rng.randint(1, 6)
        ref, _, _ = run_schedule(T, steps, 0, 0, term)
        need = []
        run_schedule(T, steps, budget, 64, term, need)
        X = rng.randint(0, 6)
        got = []
        ops, sel, pend = run_schedule(T, steps, budget, X, term, got)
        assert ops == ref and sel == [steps] * T and not any(pend)
        assert got[0] == (need[0] if need[0] <= X else X + 1), (T, steps, budget, X, need, got)


# ---------------------------------------------------------------------------
# csrc/schedule.h
# ---------------------------------------------------------------------------
SHIMS = '''#include "schedule.h"
static AdaptiveRounds A;
extern "C" {
int max_pipeline() { return kMaxPipeline; }
int split(int G, int pipeline, int* g0, int* ng) {
    const GroupSplit P = split_groups(G, pipeline);
    for (int k = 0; k < P.K; ++k) g0[k] = P.g0[k], ng[k] = P.ng[k];
    return P.K;
}
int launches(int ng, int L, int nn_batch) { return group_launches(ng, L, nn_batch); }
// the most NN rounds of one search: the thread-split schedule runs no extra rounds
int max_rounds(int G, int T, int B, int sims, int exact, int budget, int cuts) {
    const int steps = search_steps(sims, T * B);
    return steps + (thread_split_shape(G, T) ? 0 : extra_round_cap(exact != 0, budget, cuts, T, steps));
}
void ar_new() { A = AdaptiveRounds(); }
void ar_reset(int on, int min_rounds) { A.reset(on != 0, min_rounds); }
void ar_observe(int x, int used, int empties, int cuts) { A.observe(x, used, empties, cuts); }
int ar_pick(int cap) { return A.pick(cap); }
int ar_threshold() { return A.empties; }
}
'''


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("schedule")
    (d / "s.cpp").write_text(SHIMS)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-shared", "-fPIC", "-I",
                    str(ROOT / "othello-alphazero_amd" / "csrc"), str(d / "s.cpp"), "-o", str(d / "s.so")], check=True)
    return ctypes.CDLL(str(d / "s.so"))


@pytest.fixture(scope="module")
def bench():
    sys.path.insert(0, str(ROOT))
    import bench

    return bench


def test_group_split_matches_bench_and_covers_every_game(lib, bench):
    assert lib.max_pipeline() == 8
    g0, ng = (ctypes.c_int * 8)(), (ctypes.c_int * 8)()
    for G, pipeline in itertools.product(range(1, 301), range(0, 9)):
        K = lib.split(G, pipeline, g0, ng)
        assert K == bench.pipeline_groups(types.SimpleNamespace(games=G, pipeline=pipeline)), (G, pipeline)
        assert g0[0] == 0 and all(ng[k] >= 1 for k in range(K)), (G, pipeline)
        assert all(g0[k + 1] == g0[k] + ng[k] for k in range(K - 1)), (G, pipeline)
        assert g0[K - 1] + ng[K - 1] == G and sum(ng[:K]) == G, (G, pipeline)


def test_group_launches(lib):
    """nn_batch slices a group's ng x L rows into consecutive launches."""
    assert lib.launches(2, 8, 20) == 1 and lib.launches(3, 8, 20) == 2  # 16 and 24 rows
    assert lib.launches(128, 32, 0) == 1 and lib.launches(128, 32, 4096) == 1 and lib.launches(128, 32, 4095) == 2
    assert lib.launches(256, 32, 2048) == 4 and lib.launches(1, 1, 1) == 1


def test_extra_round_cap_matches_bench(lib, bench):
    """steps + the cap == bench.max_search_rounds: round-robin endgames and
    budget 0 run no extra round, nor does the single-game thread split."""
    seen = set()
    for G, T, B, sims, budget, cuts, rr in itertools.product((1, 7, 256), (1, 2, 3, 8, 9), (1, 4, 16),
                                                             (1, 31, 96, 800, 1600), (0, 1, 2, 4), (0, 3, 64),
                                                             (False, True)):
        a = types.SimpleNamespace(games=G, pipeline=0, threads=T, batch=B, sims=sims, chain_budget=budget,
                                  chain_cuts=cuts, round_robin_endgames=rr)
        want = bench.max_search_rounds(a)
        assert lib.max_rounds(G, T, B, sims, not rr, budget, cuts) == want, vars(a)
        seen.add(want - -(-sims // (T * B)))
    assert {0, 3, 64} <= seen and len(seen) > 5  # capped by cuts, and by T x steps / budget
    a = bench.parse_args([])  # the benched shape: 25 + min(64, 2 x 25 / 2)
    assert lib.max_rounds(a.games, a.threads, a.batch, a.sims, 1, a.chain_budget, a.chain_cuts) == 50


def test_adaptive_controller(lib):
    """The control law of the adaptive extra rounds, driven with scripted
    read-backs (x of that search, most cuts used, fewest root empties).

    Two values of the header's prose cannot come out of the rule as the
    engine has always applied it: a search that used cuts first raises the
    endgame threshold to its fewest empties + 3, so the comparison that
    follows always finds it inside the endgame and X becomes chain_cuts;
    `used + min` is only ever reached with used = 0, and `2X + 2 + min` never.
    The rule is kept as it is (scheduling only), and pinned as it is."""
    cuts = 64
    lib.ar_new()
    # nothing observed yet: the minimum, within the cap
    assert lib.ar_pick(50) == 1 and lib.ar_pick(0) == 0
    lib.ar_reset(1, 3)
    assert lib.ar_pick(50) == 3 and lib.ar_pick(2) == 2
    # no cuts outside the endgame: used + min = the minimum
    lib.ar_reset(1, 1)
    lib.ar_observe(1, 0, 40, cuts)
    assert lib.ar_pick(50) == 1 and lib.ar_threshold() == 12
    lib.ar_reset(1, 2)
    lib.ar_observe(2, 0, 13, cuts)
    assert lib.ar_pick(50) == 2
    # fewest empties <= 12: chain_cuts, clamped to the cap
    lib.ar_observe(2, 0, 12, cuts)
    assert lib.ar_pick(50) == 50 and lib.ar_pick(64) == 64 and lib.ar_pick(100) == 64
    assert lib.ar_threshold() == 12
    # cuts used at 30 empties raise the threshold to 33: that search counts as
    # endgame (see the docstring), whether its report is within its X ...
    lib.ar_reset(1, 1)
    lib.ar_observe(3, 2, 30, cuts)
    assert lib.ar_threshold() == 33 and lib.ar_pick(50) == 50
    # ... or above it (a game ran out of cuts: k_tree reports X + 1)
    lib.ar_reset(1, 1)
    lib.ar_observe(3, 4, 30, cuts)
    assert lib.ar_threshold() == 33 and lib.ar_pick(50) == 50
    # the raised threshold holds for roots within it, and a lower root with
    # cuts does not lower it
    lib.ar_observe(50, 1, 20, cuts)
    assert lib.ar_threshold() == 33
    # each cut-free search lowers it by one, down to 12 and no further; roots
    # above it run the minimum again
    for want in range(32, 11, -1):
        lib.ar_observe(1, 0, 60, cuts)
        assert lib.ar_threshold() == want and lib.ar_pick(50) == 1
    for _ in range(3):
        lib.ar_observe(1, 0, 60, cuts)
        assert lib.ar_threshold() == 12
    # the endgame value is chain_cuts, not the cap: a cap below it clamps
    lib.ar_observe(1, 0, 5, 7)
    assert lib.ar_pick(50) == 7 and lib.ar_pick(4) == 4
    # the minimum bounds X from below, the cap bounds the minimum
    lib.ar_reset(1, 5)
    lib.ar_observe(5, 0, 5, 2)
    assert lib.ar_pick(50) == 5 and lib.ar_pick(3) == 3
    # off: always the cap, whatever was observed
    lib.ar_reset(0, 1)
    assert lib.ar_pick(50) == 50
    lib.ar_observe(1, 0, 60, cuts)
    assert lib.ar_pick(37) == 37
    # reset returns to the first state
    lib.ar_observe(3, 2, 30, cuts)
    lib.ar_reset(1, 1)
    assert lib.ar_threshold() == 12 and lib.ar_pick(50) == 1
