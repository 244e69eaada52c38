// On-device self-play between searches: random openings and the self-play
// move of a searched game (k_selfplay_move). The move itself is tree_game.h's
// selfplay_move_game, which free-running self-play (tree.hip k_tree_free) runs
// inside its round kernel.

#include <hip/hip_runtime.h>

#include "engine.h"
#include "kernels.h"
#include "tree_game.h"
#include "tree_search.h"
#include "wave.h"

namespace oamd {

__global__ void k_random_openings(EngineView E, int max_moves, uint64_t seed) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.G) return;
    init_game(E, g, seed);
    random_opening(E, g, max_moves);
}

__global__ __launch_bounds__(64) void k_selfplay_move(EngineView E, SelfplayParams sp, int g0,
                                                      int32_t* actions, int32_t* finished,
                                                      float* feat_out, float* pol_out) {
    const int g = g0 + (int)blockIdx.x;
    const int lane = lane_id();
    GameState* gs = E.games + g;
    if (!(gs->flags & kActive)) {
        if (lane == 0) {
            if (actions) actions[g] = -1;
            if (finished) finished[g] = 0;
        }
        return;
    }
    selfplay_move_game(E, sp, g, actions, finished, feat_out, pol_out, sp.adj_pending, search_is_fast(E, gs));
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
void launch_random_openings(const EngineView& E, int max_moves, uint64_t seed, hipStream_t s) {
    hipLaunchKernelGGL(k_random_openings, dim3(blocks_for(E.G, 64)), dim3(64), 0, s, E, max_moves, seed);
}
void launch_selfplay_move(const EngineView& E, const SelfplayParams& sp, int g0, int ng, int32_t* actions,
                          int32_t* finished, float* feat, float* pol, hipStream_t s) {
    if (ng > 0)
        hipLaunchKernelGGL(k_selfplay_move, dim3(ng), dim3(64), 0, s, E, sp, g0, actions, finished, feat, pol);
}

}  // namespace oamd
