// On-device arena: batched head-to-head matches between two engines. The
// choice and the application of a move are tree_game.h's (choose_root_action,
// move_root), shared with the self-play driver (selfplay.hip).

#include <hip/hip_runtime.h>

#include "engine.h"
#include "kernels.h"
#include "tree_game.h"
#include "wave.h"

namespace oamd {

// ---------------------------------------------------------------------------
// Arena: match g is game g of two engines, one tree per player as the
// reference's two AlphaZeroPlayers each own an MCTS (player.py:177-259). Per
// ply only the side to move searches (its tree alone carries kActive), the
// chosen action moves both roots (play_game, player.py:74-76), so each side
// keeps its subtree across its own and the opponent's moves.
// ---------------------------------------------------------------------------
// whether engine A's net moves at a position whose side to move is `player`
__device__ __forceinline__ bool arena_a_moves(int arena, int player) { return (player == 1) == (arena == 1); }

__device__ __forceinline__ void arena_set_mover(GameState* ga, GameState* gb, int player) {
    const int fa = ga->flags & ~(int)kActive, fb = gb->flags & ~(int)kActive;
    const bool running = player != 0;
    const bool a = arena_a_moves(ga->arena, player);
    ga->flags = fa | (running && a ? (int)kActive : 0);
    gb->flags = fb | (running && !a ? (int)kActive : 0);
}

// Reset both games of every match, play the opening plies (openings: (G,
// plies) actions, -1 = none) in both trees, and leave kActive in the tree of
// the side to move only. An illegal ply ends the match's opening there.
__global__ void k_arena_begin(EngineView EA, EngineView EB, uint64_t seed_a, uint64_t seed_b, const int32_t* openings,
                              int plies, const uint8_t* a_is_white) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= EA.G) return;
    init_game(EA, g, seed_a);
    init_game(EB, g, seed_b);
    GameState* ga = EA.games + g;
    GameState* gb = EB.games + g;
    const size_t base = (size_t)g * EA.cap;
    for (int k = 0; openings && k < plies; ++k) {
        const int a = openings[(size_t)g * plies + k];
        const int root = ga->root;
        const int player = load_link(EA.link + base + root).player;
        const uint64_t legal = EA.pos[base + root].legal;
        const bool ok = player != 0 && (a == 64 ? legal == 0 : (a >= 0 && a < 64 && ((legal >> (63 - a)) & 1ULL)));
        if (!ok) break;
        move_root(EA, g, a);
        move_root(EB, g, a);
    }
    ga->ply = 0;
    gb->ply = 0;
    ga->arena = gb->arena = a_is_white && a_is_white[g] ? 2 : 1;
    arena_set_mover(ga, gb, load_link(EA.link + base + ga->root).player);
}

// *remaining = matches still running (both roots of an arena match not terminal)
__global__ void k_arena_count(EngineView EA, int32_t* remaining) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= EA.G) return;
    const GameState* ga = EA.games + g;
    if (ga->arena != 0 && load_link(EA.link + (size_t)g * EA.cap + ga->root).player != 0 &&
        (ga->arena & (kArenaDesync | kFinAdjudicated)) == 0)
        atomicAdd(remaining, 1);
}

// One ply of match g (one wave). finished[g] is updated, never cleared: bits
// 0-1 the outcome once the match ends (1 draw, 2 black won, 3 white won, as
// k_selfplay_move reports it), bit 2 a move from an unexpanded root (uniform),
// bit 3 a node pool overflowed, bit 4 the two trees' roots differ (the match
// stops), bit 5 the match was adjudicated at this ply (sp.adj_empties > 0: the
// outcome bits follow from adjudicate.hip). actions[g] = the action played, -1
// when the match is over.
__global__ __launch_bounds__(64) void k_arena_move(EngineView EA, EngineView EB, SelfplayParams sp, int32_t* actions,
                                                   int32_t* finished, int32_t* discs, int32_t* remaining) {
    const int g = (int)blockIdx.x;
    const int lane = lane_id();
    GameState* ga = EA.games + g;
    GameState* gb = EB.games + g;
    const size_t base_a = (size_t)g * EA.cap, base_b = (size_t)g * EB.cap;
    const int arena = ga->arena;
    const NodeLink la = load_link(EA.link + base_a + ga->root);
    const NodeLink lb = load_link(EB.link + base_b + gb->root);
    const NodePos pa = EA.pos[base_a + ga->root];
    const NodePos pb = EB.pos[base_b + gb->root];
    int action = -1;
    if ((arena & 3) == 0 || (arena & (kArenaDesync | kFinAdjudicated)) || la.player == 0) {
        if (lane == 0 && actions) actions[g] = -1;
        return;
    }
    if (la.player != lb.player || pa.p1 != pb.p1 || pa.p2 != pb.p2) {
        if (lane == 0) {
            ga->arena = gb->arena = arena | kArenaDesync;
            arena_set_mover(ga, gb, 0);
            if (actions) actions[g] = -1;
            if (finished) finished[g] |= kArenaDesync;
            if (remaining) atomicSub(remaining, 1);
        }
        return;
    }
    const bool a_moves = arena_a_moves(arena, la.player);
    GameState* gm = a_moves ? ga : gb;
    const int nc = a_moves ? la.n_children : lb.n_children;
    int status = (nc == 0 ? kFinNoTargets : 0) | ((ga->flags | gb->flags) & kOverflow ? kFinOverflow : 0);
    const uint64_t ev = gm->event;
    if (a_moves) action = choose_root_action(EA, ga, base_a, la, pa, sp.temperature_moves, sp.temperature);
    else action = choose_root_action(EB, gb, base_b, lb, pb, sp.temperature_moves, sp.temperature);
    if (lane == 0) {
        gm->event = ev + 1;  // the side that does not move draws nothing
        move_root(EA, g, action);
        move_root(EB, g, action);
    }
    __builtin_amdgcn_wave_barrier();
    wait_stores();
    if (lane == 0) {
        const int r2 = ga->root;
        const NodeLink l2 = load_link(EA.link + base_a + r2);
        status |= (ga->flags | gb->flags) & kOverflow ? kFinOverflow : 0;
        const int fin = end_of_game(EA, base_a, r2, l2.player, sp.adj_empties,
                                    sp.adj_pending ? sp.adj_pending + g : nullptr, discs ? discs + 2 * g : nullptr);
        if (fin) {
            // adjudication: the match stops here, adjudicate.hip reports the exact result
            if (fin & kFinAdjudicated) ga->arena = gb->arena = arena | kFinAdjudicated;
            if (remaining) atomicSub(remaining, 1);
        }
        arena_set_mover(ga, gb, fin & kFinAdjudicated ? 0 : l2.player);
        if (actions) actions[g] = action;
        if (finished && (fin | status)) finished[g] |= fin | status;
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
void launch_arena_begin(const EngineView& EA, const EngineView& EB, uint64_t seed_a, uint64_t seed_b,
                        const int32_t* openings, int plies, const uint8_t* a_is_white, hipStream_t s) {
    if (EA.G != EB.G) return;  // caller validated
    hipLaunchKernelGGL(k_arena_begin, dim3(blocks_for(EA.G, 64)), dim3(64), 0, s, EA, EB, seed_a, seed_b, openings,
                       plies, a_is_white);
}
void launch_arena_count(const EngineView& EA, int32_t* remaining, hipStream_t s) {
    hipLaunchKernelGGL(k_arena_count, dim3(blocks_for(EA.G, 64)), dim3(64), 0, s, EA, remaining);
}
void launch_arena_move(const EngineView& EA, const EngineView& EB, const SelfplayParams& sp, int32_t* actions,
                       int32_t* finished, int32_t* discs, int32_t* remaining, hipStream_t s) {
    if (EA.G != EB.G || EA.G <= 0) return;  // caller validated
    hipLaunchKernelGGL(k_arena_move, dim3(EA.G), dim3(64), 0, s, EA, EB, sp, actions, finished, discs, remaining);
}

}  // namespace oamd
