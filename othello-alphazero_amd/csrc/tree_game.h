// Game lifecycle on the device: reset, moving the root, the self-play targets
// of a root, random openings, the choice of a move from a searched root and
// the self-play move itself. Device code shared by tree.hip (reset / apply /
// targets), selfplay.hip (k_selfplay_move, k_tree_free) and arena.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "bitboard.h"
#include "engine.h"
#include "exact_leaf.h"
#include "forced.h"
#include "kernels.h"
#include "rng.h"
#include "tree_search.h"
#include "wave.h"

namespace oamd {

// ---------------------------------------------------------------------------
// Game state: reset, moves, root statistics, self-play targets
// ---------------------------------------------------------------------------
__device__ inline void init_game(const EngineView& E, int g, uint64_t seed) {
    GameState* gs = E.games + g;
    const size_t base = (size_t)g * E.cap;
    const Pos p = initial_position();
    store_link(E.link + base, NodeLink{-1, 0, -1, p.player});
    store_stat(E.stat + base, NodeStat{0, 0.0f, 0.0f, 1.0f});
    store_pos(E.pos + base, p);
    gs->root = 0;
    gs->count = 1;
    gs->flags = kActive;
    gs->hist_n = 0;
    gs->key = mix64(seed ^ mix64((uint64_t)g + 0x632BE59BD9B4E019ULL));
    gs->event = 0;
    gs->ply = 0;
    gs->arena = 0;
    for (int k = 0; k < 16; ++k) gs->hist[k] = -1;
}

// Move the root of game g along `action` (mcts.cpp:114-165): into the existing
// child when the root is expanded, else into a fresh node. History = parents.
__device__ inline void move_root(const EngineView& E, int g, int action) {
    GameState* gs = E.games + g;
    const size_t base = (size_t)g * E.cap;
    const int root = gs->root;
    const NodeLink lk = load_link(E.link + base + root);
    int next;
    if (lk.n_children == 0) {
        if ((int64_t)gs->count + 1 > E.cap) {
            gs->flags |= kOverflow;
            return;
        }
        next = gs->count++;
        const Pos p = load_pos(E.pos + base + root, lk.player);
        const Pos c = apply_action(p, action);
        store_link(E.link + base + next, NodeLink{-1, 0, root, c.player});
        store_stat(E.stat + base + next, NodeStat{0, 0.0f, 0.0f, 1.0f});
        store_pos(E.pos + base + next, c);
    } else {
        const uint64_t legal = E.pos[base + root].legal;
        next = lk.first_child + child_index_of(legal, lk.n_children, action);
        // the root is never an exact leaf: a pending or solved mark goes, and
        // the node is an ordinary unexpanded leaf again
        if (E.exact_empties > 0) {
            const NodeLink nl = load_link(E.link + base + next);
            if (nl.n_children == 0 && exact_mark(nl.first_child))
                store_link(E.link + base + next, NodeLink{kMarkPlain, 0, nl.parent, nl.player});
        }
    }
    for (int k = 15; k > 0; --k) gs->hist[k] = gs->hist[k - 1];
    gs->hist[0] = root;
    gs->hist_n = gs->hist_n < 16 ? gs->hist_n + 1 : 16;
    gs->root = next;
    gs->ply += 1;
}

// Visit count of root child `lane` of game g as the policy target counts it
// (0 for lanes past the children): the raw count, or with policy target pruning
// (E.prune_targets, forced.h) the pruned one. The most visited
// child (the first of them) keeps its count; every other child gives back the
// visits PUCT alone would not have spent, judged with the stored priors, the
// root's exploration rate and the children's visit sum as the selection uses
// them. One wave, lane = child.
__device__ __forceinline__ int root_target_count(const EngineView& E, int g) {
    const int lane = lane_id();
    const size_t base = (size_t)g * E.cap;
    const int root = E.games[g].root;
    const NodeLink lk = load_link(E.link + base + root);
    const int nc = lk.n_children;
    NodeStat cs{0, 0.0f, 0.0f, 0.0f};
    if (lane < nc) cs = load_stat(E.stat + base + lk.first_child + lane);
    if (!E.prune_targets || nc <= 1) return cs.n;
    const int total = wave_sum(cs.n);
    if (total == 0) return cs.n;
    const int mx = wave_max_i(lane < nc ? cs.n : (int)0x80000000);
    const int best = __ffsll((unsigned long long)__ballot(lane < nc && cs.n == mx)) - 1;
    const float mult = explore_rate(E, E.stat[base + root].n) * sqrt_count(E, total);
    const float ubest = readlane_f(prune_score(cs.q, mult, cs.p, cs.n), best);
    if (lane < nc && lane != best) return prune_child(cs.n, cs.q, cs.p, mult, ubest, E.forced_k, total);
    return cs.n;
}

// 8-fold self-play targets of the root (mcts.cpp:63-112): features of the root
// under transform t (wave t of the block) and policy[transform(a,t)] = N_a/sum,
// N = n of lane = child, the caller's root_target_count (computed once per root).
__device__ inline void write_targets(const EngineView& E, int g, int t, int n, float* feat_out, float* pol_out) {
    const int lane = lane_id();
    const GameState* gs = E.games + g;
    const size_t base = (size_t)g * E.cap;
    const int root = gs->root;
    const NodeLink lk = load_link(E.link + base + root);
    const NodePos rp = E.pos[base + root];
    const int C = 1 + 2 * E.H;
    float* fo = feat_out + (size_t)t * C * 64;
    const int src = inverse_transform(lane, t);
    fo[lane] = (float)(lk.player - 1);
    for (int h = 0; h < E.H; ++h) {
        int node = -1;
        if (h == 0) node = root;
        else if (h - 1 < gs->hist_n) node = gs->hist[h - 1];
        float b = 0.0f, w = 0.0f;
        if (node >= 0) {
            const NodePos np = E.pos[base + node];
            b = (float)((np.p1 >> (63 - src)) & 1ULL);
            w = (float)((np.p2 >> (63 - src)) & 1ULL);
        }
        fo[(1 + 2 * h) * 64 + lane] = b;
        fo[(2 + 2 * h) * 64 + lane] = w;
    }
    float* po = pol_out + (size_t)t * 65;
    const int nc = lk.n_children;
    int sum = wave_sum(n);
    if (sum == 0) sum = 1;
    po[lane] = 0.0f;
    if (lane == 0) po[64] = 0.0f;
    __builtin_amdgcn_wave_barrier();
    if (nc > 0) {
        if (rp.legal) {
            const int s = lane;
            const bool set = (rp.legal >> (63 - s)) & 1ULL;
            const int j = s == 0 ? 0 : popcount64(rp.legal & (~0ULL << (64 - s)));
            const int nj = __shfl(n, j & 63);
            if (set) po[transform_action(s, t)] = (float)nj / (float)sum;
        } else if (lane == 0) {
            po[64] = (float)n / (float)sum;
        }
    }
}

// ---------------------------------------------------------------------------
// On-device self-play move (train.py:404-452): choose, emit targets, apply,
// restart finished games from a random opening.
// ---------------------------------------------------------------------------
__device__ inline void random_opening(const EngineView& E, int g, int max_moves) {
    // lane-0 sequential: k ~ U{0..max_moves} uniformly random legal plies
    GameState* gs = E.games + g;
    if (max_moves <= 0) return;
    const uint64_t ev = gs->event++;
    const uint64_t key = stream_key(gs->key, ev, 0);
    const int k = (int)(mix64(key) % (uint64_t)(max_moves + 1));
    for (int m = 0; m < k; ++m) {
        const size_t base = (size_t)g * E.cap;
        const int root = gs->root;
        const NodeLink lk = load_link(E.link + base + root);
        if (lk.player == 0) break;
        const NodePos rp = E.pos[base + root];
        const int na = rp.legal ? popcount64(rp.legal) : 1;
        const int pick = (int)(mix64(key + (uint64_t)(m + 1) * kGolden) % (uint64_t)na);
        int action = 64;
        if (rp.legal) {
            uint64_t rem = rp.legal;
            for (int s = 0, c = 0; s < 64; ++s) {
                if ((rem >> (63 - s)) & 1ULL) {
                    if (c == pick) {
                        action = s;
                        break;
                    }
                    ++c;
                }
            }
        }
        move_root(E, g, action);
    }
    gs->ply = 0;
}

constexpr int kFinNoTargets = 4, kFinOverflow = 8;

// The move a game plays from its searched root (one wave; train.py:421-430,
// player.py:250-256): temperature sampling while the game's ply <
// temperature_moves, else argmax of the root visits with a uniform random
// tie-break; uniform over the legal actions when the root is unexpanded. One
// draw from the game's stream at its current event (the caller advances it).
// Shared by the self-play driver and the arena.
__device__ __forceinline__ int choose_root_action(const EngineView& E, const GameState* gs, size_t base,
                                                  const NodeLink& lk, const NodePos& rp, int temperature_moves,
                                                  float temperature) {
    const int lane = lane_id();
    const int nc = lk.n_children;
    const int na = rp.legal ? popcount64(rp.legal) : 1;
    int n = 0;
    if (lane < nc) n = E.stat[base + lk.first_child + lane].n;
    const uint64_t ev = gs->event;
    const float u = uniform(stream_key(gs->key, ev, 0), 0);
    int j = 0;
    if (nc == 0) {
        j = (int)(u * (float)na);  // unexpanded root: uniform over legal actions
        if (j >= na) j = na - 1;
    } else if (gs->ply < temperature_moves) {
        // p ~ N^(1/temperature) (train.py:423-426); cdf search like numpy.random.choice
        const float w = lane < nc ? powf((float)n, 1.0f / temperature) : 0.0f;
        float sum = 0.0f;
        float cdf = 0.0f;
        for (int k = 0; k < nc; ++k) {
            sum += readlane_f(w, k);
            if (k == lane) cdf = sum;
        }
        if (sum > 0.0f) {
            const float target = u * sum;
            const bool above = lane < nc && cdf > target;
            const uint64_t b = __ballot(above);
            j = b ? __ffsll((unsigned long long)b) - 1 : nc - 1;
        } else {
            j = (int)(u * (float)nc);
            if (j >= nc) j = nc - 1;
        }
    } else {
        // argmax with uniform random tie-break (train.py:428-430)
        int m = n;
        m = wave_max_i(m);
        const uint64_t ties = __ballot(lane < nc && n == m);
        const int nt = popcount64(ties);
        int k = (int)(u * (float)nt);
        if (k >= nt) k = nt - 1;
        uint64_t rem = ties;
        for (int x = 0; x < k; ++x) rem &= rem - 1;
        j = __ffsll((unsigned long long)rem) - 1;
    }
    return action_of_child(rp.legal, j);
}

// The pending slot of an adjudicating driver (SelfplayParams::adj_pending):
// the root as an oamd_position, player 0 for a game that ended on the board.
__device__ __forceinline__ void store_pending(oamd_position* slot, int player, const NodePos& p) {
    slot->player = player;
    slot->reserved = 0;
    slot->player1_discs = p.p1;
    slot->player2_discs = p.p2;
    slot->legal_moves = p.legal;
    slot->next_legal_moves = p.next_legal;
}

// Whether the game ends at its new root (node `root`, side to move `player`)
// after a move, as the `finished` code: 1 draw, 2 black won, 3 white won for a
// game over on the board (player 0); kFinAdjudicated when adj_empties > 0 and
// the root has at most that many empties (adjudication, DESIGN.md §16: the
// exact solver finishes it, the outcome bits come from adjudicate.hip); 0 when
// the game goes on. A game that ends leaves its root in *slot (store_pending)
// and its disc counts in discs[0..1], where those are given. Lane 0.
__device__ __forceinline__ int end_of_game(const EngineView& E, size_t base, int root, int player, int adj_empties,
                                           oamd_position* slot, int32_t* discs) {
    if (player != 0 && adj_empties <= 0) return 0;
    const NodePos p2 = E.pos[base + root];
    const int b = popcount64(p2.p1), w = popcount64(p2.p2);
    int fin = kFinAdjudicated;
    if (player == 0) fin = b > w ? 2 : (b < w ? 3 : 1);
    else if (64 - popcount64(p2.p1 | p2.p2) > adj_empties) return 0;
    if (discs) {
        discs[0] = b;
        discs[1] = w;
    }
    if (slot) store_pending(slot, player, p2);
    return fin;
}

// One self-play move of game g (one wave): outputs at index g of the given
// per-move slices. fast: the root's search was a fast one (search_is_fast at
// the ply of the searched root, before the move): the move is chosen and
// applied as ever, but writes no targets and reports kFinFast.
__device__ __forceinline__ void selfplay_move_game(const EngineView& E, const SelfplayParams& sp, int g,
                                                   int32_t* actions, int32_t* finished, float* feat_out,
                                                   float* pol_out, oamd_position* pending, bool fast) {
    const int lane = lane_id();
    GameState* gs = E.games + g;
    const size_t base = (size_t)g * E.cap;
    const int root = gs->root;
    const NodeLink lk = load_link(E.link + base + root);
    const NodePos rp = E.pos[base + root];
    const int nc = lk.n_children;
    // status bits reported with `finished` (selfplay.py): the root had no
    // searched children, so no targets were written (the reference's
    // self_play_data raises, mcts.cpp:69-71); the game's node pool overflowed
    const int status = (lk.player != 0 && nc == 0 ? kFinNoTargets : 0) |
                       (gs->flags & kOverflow ? kFinOverflow : 0);
    int action = -1;
    if (lk.player != 0) {
        const uint64_t ev = gs->event;
        action = choose_root_action(E, gs, base, lk, rp, sp.temperature_moves, sp.temperature);
        if (sp.emit_targets && feat_out && nc > 0 && !fast) {
            const int C = 1 + 2 * E.H;
            const int n = root_target_count(E, g);
            for (int t = 0; t < 8; ++t)
                write_targets(E, g, t, n, feat_out + (size_t)g * 8 * C * 64, pol_out + (size_t)g * 8 * 65);
        }
        if (lane == 0) {
            gs->event = ev + 1;
            move_root(E, g, action);
        }
    }
    __builtin_amdgcn_wave_barrier();
    wait_stores();
    int fin = 0;
    if (lane == 0) {
        const int r2 = gs->root;
        const NodeLink l2 = load_link(E.link + base + r2);
        // only a searched move is adjudicated
        fin = end_of_game(E, base, r2, l2.player, action >= 0 ? sp.adj_empties : 0, pending ? pending + g : nullptr,
                          nullptr);
        if (fin) {
            const uint64_t key = gs->key;
            const uint64_t ev = gs->event;
            init_game(E, g, key ^ mix64(ev + 0xA5A5A5A5ULL));
            random_opening(E, g, sp.opening_moves);
        }
        if (actions) actions[g] = action;
        if (finished) finished[g] = fin | status | (fast && action >= 0 ? kFinFast : 0);
    }
}

}  // namespace oamd
