// Stand-alone host check of the baseline opponents (csrc/baseline.h over
// solver.h, rng.h and bitboard.h), meant to be built with
// -fsanitize=address,undefined and run on a CPU:
//
//   hipcc -O1 -g -x hip --offload-arch=gfx950 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//       -I othello-alphazero_amd/csrc tools/baseline_host_check.cpp -o tools/_build/baseline_host_check
//   tools/_build/baseline_host_check
//
// Seeded random-play positions; every output of baseline_host (move scores,
// score, the pick, flags) is compared with an unpruned recursive minimax and a
// static evaluation written here: depth 1..4 at any stage of the game, depth up
// to 8 at 8 or fewer empties, RANDOM and GREEDY everywhere. The flags
// (overlapping discs, a bad player, a node limit that binds), roots where
// nobody can move, the depth cap of 10 on a late position and the keyed pick
// (always a tied action, every tied action reached, k as stated) are exercised.

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "baseline.h"
#include "bitboard.h"

using namespace oamd;

static uint64_t g_rng = 0x9E3779B97F4A7C15ULL;
static uint32_t rnd(uint32_t n) {  // xorshift64*
    g_rng ^= g_rng >> 12;
    g_rng ^= g_rng << 25;
    g_rng ^= g_rng >> 27;
    return (uint32_t)((g_rng * 0x2545F4914F6CDD1DULL) >> 33) % n;
}

static int empties(const Pos& p) { return popcount64(~(p.p1 | p.p2)); }

// Random play from the initial position down to `e` empties (or to the end of the game).
static Pos random_position(int e) {
    Pos p = initial_position();
    while (p.player != 0 && empties(p) > e) {
        int acts[65], n = 0;
        if (!p.legal) acts[n++] = 64;
        for (int s = 0; s < 64; ++s)
            if (p.legal >> (63 - s) & 1) acts[n++] = s;
        p = apply_action(p, acts[rnd((uint32_t)n)]);
    }
    return p;
}

static bool owns(uint64_t side, int action) { return (side >> (63 - action) & 1) != 0; }

static int heuristic(uint64_t me, uint64_t opp) {
    static const int corner[4] = {0, 7, 56, 63}, xsq[4] = {9, 14, 49, 54};
    int h = 10 * (popcount64(legal_moves(me, opp)) - popcount64(legal_moves(opp, me))) + popcount64(me) -
            popcount64(opp);
    for (int i = 0; i < 4; ++i) {
        h += 50 * ((int)owns(me, corner[i]) - (int)owns(opp, corner[i]));
        if (!owns(me | opp, corner[i])) h -= 20 * ((int)owns(me, xsq[i]) - (int)owns(opp, xsq[i]));
    }
    return h;
}

static int minimax(uint64_t me, uint64_t opp, int d) {
    const uint64_t moves = legal_moves(me, opp);
    if (!moves) {
        if (!legal_moves(opp, me)) {
            const int delta = popcount64(me) - popcount64(opp);
            return 4096 * ((delta > 0) - (delta < 0)) + delta;
        }
        return -minimax(opp, me, d);
    }
    if (d == 0) return heuristic(me, opp);
    int best = INT32_MIN;
    for (int s = 0; s < 64; ++s) {
        const uint64_t m = 1ULL << (63 - s);
        if (!(moves & m)) continue;
        const uint64_t f = flips(m, me, opp);
        best = std::max(best, -minimax(opp & ~f, me | m | f, d - 1));
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

static const int64_t kBig = 1LL << 40;

// Expected scores of a position that is neither flagged nor over.
static void expected(const Pos& p, int kind, int depth, int32_t* want) {
    const uint64_t me = p.player == 1 ? p.p1 : p.p2, opp = p.player == 1 ? p.p2 : p.p1;
    const uint64_t moves = legal_moves(me, opp);
    for (int a = 0; a < 65; ++a) want[a] = OAMD_BASELINE_NONE;
    if (!moves) want[64] = kind == OAMD_BASELINE_SEARCH ? -minimax(opp, me, depth) : 0;
    for (int s = 0; s < 64; ++s) {
        const uint64_t m = 1ULL << (63 - s);
        if (!(moves & m)) continue;
        const uint64_t f = flips(m, me, opp);
        want[s] = kind == OAMD_BASELINE_RANDOM   ? 0
                  : kind == OAMD_BASELINE_GREEDY ? popcount64(f)
                                                 : -minimax(opp & ~f, me | m | f, depth - 1);
    }
}

static int cases = 0, tied_cases = 0, passes = 0, terminals = 0;

static void check_position(const Pos& p, int kind, int depth) {
    int32_t ms[65], score, action, flags, want[65];
    int64_t nodes;
    baseline_host(p.player, p.p1, p.p2, kind, depth, kBig, false, 0, 0, ms, &score, &action, &flags, &nodes);
    EXPECT(flags == 0);
    if (!legal_moves(p.p1, p.p2) && !legal_moves(p.p2, p.p1)) {  // nobody can move: no action
        for (int a = 0; a < 65; ++a) EXPECT(ms[a] == OAMD_BASELINE_NONE);
        EXPECT(score == OAMD_BASELINE_NONE && action == -1 && nodes == 0);
        ++terminals;
        return;
    }
    expected(p, kind, depth, want);
    EXPECT(std::memcmp(ms, want, sizeof(ms)) == 0);
    const int32_t best = *std::max_element(want, want + 65);
    int tied[65], nt = 0;
    for (int a = 0; a < 65; ++a)
        if (want[a] == best) tied[nt++] = a;
    EXPECT(score == best && action == tied[0]);
    EXPECT((nodes == 0) == (kind != OAMD_BASELINE_SEARCH));
    passes += want[64] != OAMD_BASELINE_NONE;
    ++cases;
    // the keyed pick: k = min(nt - 1, (int)(u * nt)); over 64 events every tied action and no other
    uint64_t reached = 0, all = 0;
    const uint64_t key = 0xC0FFEEULL * (uint64_t)(cases + 1);
    for (int ev = 0; ev < 64; ++ev) {
        int32_t ms2[65], score2, action2, flags2;
        int64_t nodes2;
        if (kind == OAMD_BASELINE_SEARCH && depth > 2 && ev >= 4) break;  // the search is repeated per event
        baseline_host(p.player, p.p1, p.p2, kind, depth, kBig, true, key, (uint64_t)ev, ms2, &score2, &action2, &flags2,
                      &nodes2);
        int k = (int)(uniform(stream_key(key, (uint64_t)ev, 0), 0) * (float)nt);
        if (k >= nt) k = nt - 1;
        EXPECT(action2 == tied[k] && score2 == score && nodes2 == nodes && flags2 == 0);
        EXPECT(std::memcmp(ms, ms2, sizeof(ms)) == 0);
        reached |= 1ULL << k;
    }
    for (int k = 0; k < nt; ++k) all |= 1ULL << k;
    if (nt >= 2 && nt <= 4 && !(kind == OAMD_BASELINE_SEARCH && depth > 2)) {
        EXPECT(reached == all);  // 64 draws over at most 4 values: a miss has probability < 4 * 0.75^64
        ++tied_cases;
    }
}

static void check_flags(const Pos& p) {
    int32_t ms[65], score, action, flags;
    int64_t nodes;
    for (int kind = 0; kind <= 2; ++kind) {
        baseline_host(p.player, p.p1 | 1ULL, p.p2 | 1ULL, kind, 2, kBig, false, 0, 0, ms, &score, &action, &flags,
                      &nodes);
        EXPECT(flags == OAMD_SOLVE_INVALID && score == OAMD_BASELINE_NONE && action == -1 && nodes == 0);
        for (int a = 0; a < 65; ++a) EXPECT(ms[a] == OAMD_BASELINE_NONE);
        baseline_host(3, p.p1, p.p2, kind, 2, kBig, true, 5, 6, ms, &score, &action, &flags, &nodes);
        EXPECT(flags == OAMD_SOLVE_INVALID && action == -1);
    }
    if (p.player == 0) return;
    baseline_host(0, p.p1, p.p2, OAMD_BASELINE_SEARCH, 2, kBig, false, 0, 0, ms, &score, &action, &flags, &nodes);
    EXPECT(flags == OAMD_SOLVE_INVALID);  // marked over while a side can move
    if (empties(p) >= 12) {
        baseline_host(p.player, p.p1, p.p2, OAMD_BASELINE_SEARCH, 4, 10, false, 0, 0, ms, &score, &action, &flags,
                      &nodes);
        EXPECT(flags == OAMD_SOLVE_NODE_LIMIT && score == OAMD_BASELINE_NONE && action == -1 && nodes > 0);
        for (int a = 0; a < 65; ++a) EXPECT(ms[a] == OAMD_BASELINE_NONE);
        baseline_host(p.player, p.p1, p.p2, OAMD_BASELINE_GREEDY, 4, 1, false, 0, 0, ms, &score, &action, &flags,
                      &nodes);
        EXPECT(flags == 0 && action >= 0);  // nothing is searched: the limit cannot bind
    }
}

int main() {
    for (int e = 0; e <= 60; e += 2) {
        for (int i = 0; i < (e <= 8 ? 12 : 3); ++i) {
            const Pos p = random_position(e);
            check_flags(p);
            check_position(p, OAMD_BASELINE_RANDOM, 1);
            check_position(p, OAMD_BASELINE_GREEDY, 1);
            const int deepest = empties(p) <= 8 ? 8 : 4;
            for (int d = 1; d <= deepest; ++d) check_position(p, OAMD_BASELINE_SEARCH, d);
            if (empties(p) <= 6) check_position(p, OAMD_BASELINE_SEARCH, kBaselineMaxDepth);
        }
    }
    std::printf("baseline_host_check: %d cases (%d root passes, %d with 2..4 ties reached in full), %d terminal roots, "
                "%d failures\n", cases, passes, tied_cases, terminals, fails);
    return fails ? 1 : 0;
}
