// Stand-alone host check of the split endgame solver (csrc/solver.h,
// DESIGN.md §15), meant to be built with -fsanitize=address,undefined and run
// on a CPU, like solver_host_check.cpp:
//
//   hipcc -O1 -g -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -I othello-alphazero_amd/csrc tools/solver_split_check.cpp -o tools/_build/solver_split_check
//   tools/_build/solver_split_check                 # the checks below
//   tools/_build/solver_split_check nodes 12 256    # node counts of both solvers, as JSON
//
// check (default): seeded random-play positions with 0..8 empties: every
// output of solve_host_split against a recursive exhaustive minimax written
// here; positions at 10..12 empties against solve_host; the limits
// (max_empties below the count, node_limit 10, overlapping discs, player 0 on
// a live board); and the node accounting, recomputed here from the plans.
// nodes E COUNT: COUNT seeded random-play positions at E empties (the
// generator of solver_host_check.cpp): total nodes and the largest item of
// the current solver, and total nodes and the largest item of each phase of
// the split solver. These are counts, so any CPU gives the same numbers.

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "bitboard.h"
#include "solver.h"

using namespace oamd;

static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd(uint32_t n) {  // xorshift64*
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return (uint32_t)((g_rng * 0x2545F4914F6CDD1DULL) >> 33) % n;
}

static int empties(const Pos& p) { return popcount64(~(p.p1 | p.p2)); }

// Random play from the initial position down to `e` empties; false when the game ended before.
static bool random_position(int e, Pos* out) {
    Pos p = initial_position();
    while (p.player != 0 && empties(p) > e) {
        int acts[65], n = 0;
        if (!p.legal) acts[n++] = 64;
        for (int s = 0; s < 64; ++s)
            if (p.legal >> (63 - s) & 1) acts[n++] = s;
        p = apply_action(p, acts[rnd((uint32_t)n)]);
    }
    *out = p;
    return empties(p) == e;
}

static int minimax(uint64_t me, uint64_t opp) {
    const uint64_t moves = legal_moves(me, opp);
    if (!moves) {
        if (!legal_moves(opp, me)) return popcount64(me) - popcount64(opp);
        return -minimax(opp, me);
    }
    int best = -65;
    for (int s = 0; s < 64; ++s) {
        const uint64_t m = 1ULL << (63 - s);
        if (!(moves & m)) continue;
        const uint64_t f = flips(m, me, opp);
        best = std::max(best, -minimax(opp & ~f, me | m | f));
    }
    return best;
}

static int fails = 0;
#define EXPECT(cond)                                              \
    do {                                                          \
        if (!(cond)) {                                            \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++fails;                                              \
        }                                                         \
    } while (0)

struct Solved {
    int32_t ms[65], score, best, flags;
    int64_t nodes;
};

static Solved split(const Pos& p, int max_empties, int64_t limit) {
    Solved s;
    solve_host_split(p.player, p.p1, p.p2, max_empties, limit, s.ms, &s.score, &s.best, &s.flags, &s.nodes);
    return s;
}

static Solved plain(const Pos& p, int max_empties, int64_t limit) {
    Solved s;
    solve_host(p.player, p.p1, p.p2, max_empties, limit, s.ms, &s.score, &s.best, &s.flags, &s.nodes);
    return s;
}

// One item of the split solver, searched here: its nodes, status and result.
static int64_t item(const SolvePlan& pl, uint64_t m, int alpha, int64_t limit, int32_t* status, int32_t* result) {
    SolveHostStack st;
    SolveState s;
    solve_begin(s, st, pl.me, pl.opp, solve_action_of(m), alpha, 64, limit);
    while (s.status == kSolveRunning) solve_step_as<true>(s, st, limit);
    *status = s.status;
    *result = s.result;
    return s.nodes;
}

// The accounting of DESIGN.md §15, written out a second time: per root action 1 for Q,
// 1 more when Q's mover passes, plus its items; an item over the limit makes
// the action NONE and stops phase B when it is the phase A item. Also counts
// the kinds of plan met and the largest item of each phase.
struct Tally {
    int64_t nodes = 0, largest_a = 0, largest_b = 0;
    int terminal_q = 0, pass_q = 0, l64 = 0;
};

static void account(const Pos& p, int max_empties, int64_t limit, Tally* t, int32_t* want_none) {
    const SolveRoot r = solve_classify(p.player, p.p1, p.p2, max_empties);
    for (int i = 0; i < kSplitRanks; ++i) {
        const SolvePlan pl = solve_plan(r, i);
        if (pl.kind == kPlanNone) continue;
        t->nodes += pl.qnodes;
        if (pl.kind == kPlanTerminal) {
            ++t->terminal_q;
            continue;
        }
        if (pl.qnodes == 2) ++t->pass_q;
        int32_t status, L, v;
        const uint64_t first = 1ULL << (63 - pl.first);
        int64_t c = item(pl, first, -64, limit, &status, &L);
        t->nodes += c;
        t->largest_a = std::max(t->largest_a, c);
        bool none = status != kSolveDone;
        if (!none && L == 64) ++t->l64;
        if (!none && L < 64) {
            for (uint64_t rest = pl.moves & ~first; rest; rest &= rest - 1) {
                c = item(pl, rest & (0 - rest), L, limit, &status, &v);
                t->nodes += c;
                t->largest_b = std::max(t->largest_b, c);
                if (status != kSolveDone) none = true;
            }
        }
        if (none && want_none) want_none[pl.action] = 1;
    }
}

static int run_check() {
    int positions = 0, terminal = 0, passes = 0, deep = 0, limited = 0;
    Tally all;
    for (int e = 0; e <= 8; ++e) {
        for (int i = 0; i < 24; ++i) {
            Pos p;
            random_position(e, &p);  // a game that ended early is a terminal root with empties: kept
            const Solved s = split(p, 8, 1LL << 40);
            EXPECT(s.flags == 0);
            const uint64_t m1 = legal_moves(p.p1, p.p2), m2 = legal_moves(p.p2, p.p1);
            int32_t want[65], wscore = OAMD_SOLVE_NONE, wbest = -1;
            for (int a = 0; a < 65; ++a) want[a] = OAMD_SOLVE_NONE;
            if (!m1 && !m2) {
                wscore = popcount64(p.p1) - popcount64(p.p2);
                ++terminal;
            } else {
                const uint64_t me = p.player == 1 ? p.p1 : p.p2, opp = p.player == 1 ? p.p2 : p.p1;
                const uint64_t moves = p.player == 1 ? m1 : m2;
                if (!moves) {
                    want[64] = -minimax(opp, me);
                    ++passes;
                }
                for (int sq = 0; sq < 64; ++sq) {
                    const uint64_t m = 1ULL << (63 - sq);
                    if (!(moves & m)) continue;
                    const uint64_t f = flips(m, me, opp);
                    want[sq] = -minimax(opp & ~f, me | m | f);
                }
                for (int a = 0; a < 65; ++a)
                    if (want[a] > wscore) wscore = want[a], wbest = a;
            }
            EXPECT(std::memcmp(s.ms, want, sizeof(want)) == 0);
            EXPECT(s.score == wscore && s.best == wbest);
            Tally t;
            account(p, 8, 1LL << 40, &t, nullptr);
            EXPECT(t.nodes == s.nodes);
            all.nodes += t.nodes;
            all.terminal_q += t.terminal_q;
            all.pass_q += t.pass_q;
            all.l64 += t.l64;
            ++positions;
            if (empties(p) > 0 && (m1 || m2)) {
                // limits: every output of a flagged position is the sentinel
                const Solved f = split(p, empties(p) - 1, 1LL << 40);
                EXPECT(f.flags == OAMD_SOLVE_TOO_MANY_EMPTIES && f.score == OAMD_SOLVE_NONE && f.best == -1 &&
                       f.nodes == 0);
                for (int a = 0; a < 65; ++a) EXPECT(f.ms[a] == OAMD_SOLVE_NONE);
            }
            if (m1 || m2) {
                // node_limit 10 per item: NONE for exactly the root actions with an item over it
                const Solved f = split(p, 8, 10);
                int32_t none[65] = {};
                Tally tl;
                account(p, 8, 10, &tl, none);
                bool any = false;
                for (int a = 0; a < 65; ++a) {
                    any = any || none[a];
                    EXPECT(f.ms[a] == (none[a] ? OAMD_SOLVE_NONE : want[a]));
                }
                EXPECT(f.nodes == tl.nodes);
                EXPECT(f.flags == (any ? OAMD_SOLVE_NODE_LIMIT : 0));
                if (any) {
                    EXPECT(f.score == OAMD_SOLVE_NONE && f.best == -1);
                    ++limited;
                } else {
                    EXPECT(f.score == wscore && f.best == wbest);
                }
            }
            const Pos bad{p.player, 0, p.p1 | 1ULL, p.p2 | 1ULL, 0, 0};
            const Solved f = split(bad, 8, 1LL << 40);
            EXPECT(f.flags == OAMD_SOLVE_INVALID && f.score == OAMD_SOLVE_NONE && f.best == -1 && f.nodes == 0);
            if (m1 || m2) {
                const Pos nobody{0, 0, p.p1, p.p2, 0, 0};
                EXPECT(split(nobody, 8, 1LL << 40).flags == OAMD_SOLVE_INVALID);
            }
        }
    }
    // deeper than the minimax affords: the current solver is the reference
    for (int e = 10; e <= 12; ++e) {
        for (int i = 0; i < 4;) {
            Pos p;
            if (!random_position(e, &p) || p.player == 0) continue;
            const Solved a = split(p, e, 1LL << 40), b = plain(p, e, 1LL << 40);
            EXPECT(a.flags == 0 && b.flags == 0);
            EXPECT(std::memcmp(a.ms, b.ms, sizeof(a.ms)) == 0 && a.score == b.score && a.best == b.best);
            Tally t;
            account(p, e, 1LL << 40, &t, nullptr);
            EXPECT(t.nodes == a.nodes && a.nodes < b.nodes);
            all.nodes += a.nodes;
            ++deep;
            ++i;
        }
    }
    // L = 64 needs a full board of one colour, which random play does not reach. Black has everything but
    // actions 1, 57 and 30 (white) and the empties 0, 56 and 31: whichever black plays, white must pass and black
    // takes the rest, the corner first. Per root action: Q, the pass, and a phase A item of 3 nodes; no phase B.
    {
        const uint64_t white = 1ULL << (63 - 1) | 1ULL << (63 - 57) | 1ULL << (63 - 30);
        const uint64_t empty = 1ULL << 63 | 1ULL << (63 - 56) | 1ULL << (63 - 31);
        const Pos p{1, 0, ~(white | empty), white, 0, 0};
        const Solved s = split(p, 8, 1LL << 40), b = plain(p, 8, 1LL << 40);
        EXPECT(s.flags == 0 && s.score == 64 && s.best == 0 && s.nodes == 15);
        EXPECT(s.ms[0] == 64 && s.ms[56] == 64 && s.ms[31] == 64 && std::memcmp(s.ms, b.ms, sizeof(s.ms)) == 0);
        Tally t;
        account(p, 8, 1LL << 40, &t, nullptr);
        EXPECT(t.nodes == 15 && t.l64 == 3 && t.pass_q == 3);
        all.l64 += t.l64;
    }
    // the plans met at least once
    EXPECT(all.terminal_q > 0 && all.pass_q > 0 && all.l64 > 0 && limited > 0);
    std::printf("solver_split_check: %d positions (%d terminal roots, %d root passes) + %d at 10..12 empties, "
                "%d root actions ending the game, %d with a pass below, %d with L = 64, %d node-limited, "
                "%lld solver nodes, %d failures\n",
                positions, terminal, passes, deep, all.terminal_q, all.pass_q, all.l64, limited,
                (long long)all.nodes, fails);
    return fails ? 1 : 0;
}

static int run_nodes(int e, int count) {
    if (e < 0 || e > kSolveMaxEmpties || count < 1) return 2;
    int64_t plain_total = 0, plain_largest = 0;
    Tally t;
    for (int i = 0; i < count;) {
        Pos p;
        if (!random_position(e, &p) || p.player == 0) continue;
        const SolveRoot r = solve_classify(p.player, p.p1, p.p2, e);
        SolveHostStack st;
        for (int a = 0; a < 65; ++a) {
            if (!solve_is_root_action(r, a)) continue;
            SolveState s;
            solve_begin(s, st, r.me, r.opp, a, 1LL << 50);
            while (s.status == kSolveRunning) solve_step(s, st, 1LL << 50);
            plain_total += s.nodes;
            plain_largest = std::max(plain_largest, (int64_t)s.nodes);
        }
        account(p, e, 1LL << 50, &t, nullptr);
        ++i;
    }
    std::printf("{\"empties\": %d, \"positions\": %d, \"current\": {\"total_nodes\": %lld, \"largest_item\": %lld}, "
                "\"split\": {\"total_nodes\": %lld, \"largest_item_phase_a\": %lld, \"largest_item_phase_b\": %lld}}\n",
                e, count, (long long)plain_total, (long long)plain_largest, (long long)t.nodes,
                (long long)t.largest_a, (long long)t.largest_b);
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "nodes")) return run_nodes(std::atoi(argv[2]), std::atoi(argv[3]));
    return run_check();
}
