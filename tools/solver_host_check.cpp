// Stand-alone host check of the endgame solver (csrc/solver.h + bitboard.h),
// meant to be built with -fsanitize=address,undefined and run on a CPU:
//
//   hipcc -O1 -g -x hip --offload-arch=gfx950 -Xarch_host -fsanitize=address,undefined \
//       -I othello-alphazero_amd/csrc tools/solver_host_check.cpp -o tools/_build/solver_host_check
//   tools/_build/solver_host_check                 # solver == exhaustive minimax, <= 8 empties
//   tools/_build/solver_host_check nodes 12 256    # node counts per root action, as JSON
//
// check (default): seeded random-play positions with 0..8 empties; every
// output of solve_host (move scores, score, best action, flags) is compared
// with a recursive exhaustive minimax written here, and the limits are
// exercised (max_empties below the count, node_limit 10, overlapping discs).
// nodes E COUNT: COUNT seeded random-play positions at E empties; the
// distribution of nodes per root action (the unit node_limit is a budget for)
// and per position. These are counts, so any CPU gives the same numbers.

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

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
#define EXPECT(cond)                                                   \
    do {                                                               \
        if (!(cond)) {                                                 \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);      \
            ++fails;                                                   \
        }                                                              \
    } while (0)

static int run_check() {
    int64_t total_nodes = 0;
    int positions = 0, terminal = 0, passes = 0;
    for (int e = 0; e <= 8; ++e) {
        for (int i = 0; i < 24; ++i) {
            Pos p;
            random_position(e, &p);  // a game that ended early is a terminal root with empties: kept
            int32_t ms[65], score, best, flags;
            int64_t nodes;
            solve_host(p.player, p.p1, p.p2, 8, 1LL << 40, ms, &score, &best, &flags, &nodes);
            EXPECT(flags == 0);
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
                for (int s = 0; s < 64; ++s) {
                    const uint64_t m = 1ULL << (63 - s);
                    if (!(moves & m)) continue;
                    const uint64_t f = flips(m, me, opp);
                    want[s] = -minimax(opp & ~f, me | m | f);
                }
                for (int a = 0; a < 65; ++a)
                    if (want[a] > wscore) wscore = want[a], wbest = a;
            }
            EXPECT(std::memcmp(ms, want, sizeof(ms)) == 0);
            EXPECT(score == wscore && best == wbest);
            total_nodes += nodes;
            ++positions;
            if (empties(p) > 0 && (m1 || m2)) {
                // limits: every output of a flagged position is the sentinel
                solve_host(p.player, p.p1, p.p2, empties(p) - 1, 1LL << 40, ms, &score, &best, &flags, &nodes);
                EXPECT(flags == OAMD_SOLVE_TOO_MANY_EMPTIES && score == OAMD_SOLVE_NONE && best == -1 && nodes == 0);
                for (int a = 0; a < 65; ++a) EXPECT(ms[a] == OAMD_SOLVE_NONE);
            }
            if (empties(p) >= 6 && (m1 || m2)) {
                solve_host(p.player, p.p1, p.p2, 8, 10, ms, &score, &best, &flags, &nodes);
                EXPECT(flags == OAMD_SOLVE_NODE_LIMIT && score == OAMD_SOLVE_NONE && best == -1);
            }
            solve_host(p.player, p.p1 | 1ULL, p.p2 | 1ULL, 8, 1LL << 40, ms, &score, &best, &flags, &nodes);
            EXPECT(flags == OAMD_SOLVE_INVALID && score == OAMD_SOLVE_NONE && best == -1);
        }
    }
    std::printf("solver_host_check: %d positions (%d terminal roots, %d root passes), %lld solver nodes, %d failures\n",
                positions, terminal, passes, (long long)total_nodes, fails);
    return fails ? 1 : 0;
}

static int64_t pct(const std::vector<int64_t>& v, double q) { return v[(size_t)(q * (double)(v.size() - 1))]; }

static int run_nodes(int e, int count) {
    if (e < 0 || e > kSolveMaxEmpties || count < 1) return 2;
    std::vector<int64_t> per_action, per_position;
    for (int i = 0; i < count;) {
        Pos p;
        if (!random_position(e, &p) || p.player == 0) continue;
        const SolveRoot r = solve_classify(p.player, p.p1, p.p2, e);
        SolveHostStack st;
        int64_t sum = 0;
        for (int a = 0; a < 65; ++a) {
            if (!solve_is_root_action(r, a)) continue;
            SolveState s;
            solve_begin(s, st, r.me, r.opp, a, 1LL << 50);
            while (s.status == kSolveRunning) solve_step(s, st, 1LL << 50);
            per_action.push_back(s.nodes);
            sum += s.nodes;
        }
        per_position.push_back(sum);
        ++i;
    }
    std::sort(per_action.begin(), per_action.end());
    std::sort(per_position.begin(), per_position.end());
    int64_t total = 0;
    for (int64_t v : per_position) total += v;
    std::printf("{\"empties\": %d, \"positions\": %d, \"root_actions\": %zu, \"total_nodes\": %lld, "
                "\"nodes_per_root_action\": {\"median\": %lld, \"p90\": %lld, \"p99\": %lld, \"max\": %lld}, "
                "\"nodes_per_position\": {\"median\": %lld, \"p90\": %lld, \"p99\": %lld, \"max\": %lld}}\n",
                e, count, per_action.size(), (long long)total, (long long)pct(per_action, 0.5),
                (long long)pct(per_action, 0.9), (long long)pct(per_action, 0.99), (long long)per_action.back(),
                (long long)pct(per_position, 0.5), (long long)pct(per_position, 0.9),
                (long long)pct(per_position, 0.99), (long long)per_position.back());
    return 0;
}

int main(int argc, char** argv) {
    if (argc >= 4 && !std::strcmp(argv[1], "nodes")) return run_nodes(std::atoi(argv[2]), std::atoi(argv[3]));
    return run_check();
}
