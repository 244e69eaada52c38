// Search from positions handed in from outside: k_set_positions
// puts a position and up to 15 of its ancestors at the root of a game,
// k_principal_variations reads the most visited line below every root. Built
// from the game lifecycle's headers like tree.hip, selfplay.hip and arena.hip;
// neither kernel runs inside a search.

#include <hip/hip_runtime.h>

#include "bitboard.h"
#include "engine.h"
#include "kernels.h"
#include "positions.h"
#include "tree_game.h"
#include "wave.h"

namespace oamd {

// One thread per game. A game is validated completely before its first store,
// so a rejected game is left exactly as it was. Accepted: init_game's effect
// (a fresh pool, kActive, event 0, no arena match), then the key and the ply,
// the ancestors as parentless-looking nodes 0 .. n-1 of the pool, oldest first
// (node i's parent is node i-1, the oldest has none: the order in which the
// game itself would have created them), the root as node n, and hist[k] =
// n-1-k (hist[0] the root's parent), which the feature gathers and
// write_targets read.
__global__ __launch_bounds__(64) void k_set_positions(EngineView E, const oamd_position* pos,
                                                      const oamd_position* history, int K, const int32_t* hist_len,
                                                      const uint64_t* keys, const int32_t* ply, const uint8_t* mask,
                                                      uint64_t seed, int32_t* status) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.G) return;
    if (mask && !mask[g]) {
        if (status) status[g] = kSetPosSkipped;
        return;
    }
    const oamd_position in = pos[g];
    const int n = hist_len ? hist_len[g] : K;
    int32_t fault = position_fault(in.player, in.player1_discs, in.player2_discs);
    if (!fault && (n < 0 || n > K)) fault = kSetPosBadHistLen;
    if (!fault && ply && ply[g] < 0) fault = kSetPosBadPly;
    if (!fault && (int64_t)n + 1 > E.cap) fault = kSetPosCapacity;
    const oamd_position* hg = history + (size_t)g * K;  // never read with n = 0
    for (int k = 0; !fault && k < n; ++k) {
        const int32_t f = position_fault(hg[k].player, hg[k].player1_discs, hg[k].player2_discs);
        if (f) fault = f == kSetPosBadPlayer ? kSetPosHistBadPlayer : kSetPosHistOverlap;
    }
    if (status) status[g] = fault;
    if (fault) return;

    init_game(E, g, seed);
    GameState* gs = E.games + g;
    const size_t base = (size_t)g * E.cap;
    if (keys) gs->key = keys[g];
    const Pos root = canonical_position(in.player, in.player1_discs, in.player2_discs);
    gs->ply = ply ? ply[g] : popcount64(root.p1 | root.p2) - 4;
    for (int i = 0; i < n; ++i) {
        const oamd_position& h = hg[n - 1 - i];  // node i: the (n - i)-th position before the root
        const Pos a = canonical_position(h.player, h.player1_discs, h.player2_discs);
        store_link(E.link + base + i, NodeLink{-1, 0, i - 1, a.player});
        store_stat(E.stat + base + i, NodeStat{0, 0.0f, 0.0f, 1.0f});
        store_pos(E.pos + base + i, a);
    }
    store_link(E.link + base + n, NodeLink{-1, 0, n - 1, root.player});
    store_stat(E.stat + base + n, NodeStat{0, 0.0f, 0.0f, 1.0f});
    store_pos(E.pos + base + n, root);
    for (int k = 0; k < 16; ++k) gs->hist[k] = k < n ? n - 1 - k : -1;
    gs->hist_n = n;
    gs->root = n;
    gs->count = n + 1;
}

// One wave per game, lane = child. From the root: the child with the most
// visits (the lowest child index among equals, i.e. the first in
// legal_actions() order), its action, visit count and Q (the child's own
// statistics, as k_root_stats reports the root's children), then down into it;
// until a node without children (unexpanded, terminal or an exact leaf, whose
// mark sits in first_child with n_children 0), a best child without a visit,
// or max_len entries. Reads only; runs between searches.
__global__ __launch_bounds__(64) void k_principal_variations(EngineView E, int max_len, int32_t* pv_actions,
                                                             int32_t* pv_visits, float* pv_q, int32_t* pv_len) {
    const int g = blockIdx.x;
    const int lane = lane_id();
    const GameState* gs = E.games + g;
    const size_t base = (size_t)g * E.cap;
    int32_t* ao = pv_actions + (size_t)g * max_len;
    int32_t* vo = pv_visits + (size_t)g * max_len;
    float* qo = pv_q + (size_t)g * max_len;
    int len = 0;
    int node = gs->root;
    const bool active = (gs->flags & kActive) != 0;
    while (active && len < max_len) {
        const NodeLink lk = load_link(E.link + base + node);
        const int nc = __builtin_amdgcn_readfirstlane(lk.n_children);
        if (nc <= 0 || nc > 64) break;
        const int fc = __builtin_amdgcn_readfirstlane(lk.first_child);
        NodeStat cs{(int)0x80000000, 0.0f, 0.0f, 0.0f};
        if (lane < nc) cs = load_stat(E.stat + base + fc + lane);
        const int mx = wave_max_i(cs.n);
        if (mx <= 0) break;
        const int best = __ffsll((unsigned long long)__ballot(lane < nc && cs.n == mx)) - 1;
        const int action = action_of_child(E.pos[base + node].legal, best);
        if (lane == best) {
            ao[len] = action;
            vo[len] = cs.n;
            qo[len] = cs.q;
        }
        node = fc + best;
        ++len;
    }
    for (int i = len + lane; i < max_len; i += 64) {
        ao[i] = -1;
        vo[i] = 0;
        qo[i] = 0.0f;
    }
    if (lane == 0) pv_len[g] = len;
}

void launch_set_positions(const EngineView& E, const oamd_position* pos, const oamd_position* history, int K,
                          const int32_t* hist_len, const uint64_t* keys, const int32_t* ply, const uint8_t* mask,
                          uint64_t seed, int32_t* status, hipStream_t s) {
    hipLaunchKernelGGL(k_set_positions, dim3(blocks_for(E.G, 64)), dim3(64), 0, s, E, pos, history, K, hist_len, keys,
                       ply, mask, seed, status);
}

void launch_principal_variations(const EngineView& E, int max_len, int32_t* pv_actions, int32_t* pv_visits,
                                 float* pv_q, int32_t* pv_len, hipStream_t s) {
    hipLaunchKernelGGL(k_principal_variations, dim3(E.G), dim3(64), 0, s, E, max_len, pv_actions, pv_visits, pv_q,
                       pv_len);
}

}  // namespace oamd
