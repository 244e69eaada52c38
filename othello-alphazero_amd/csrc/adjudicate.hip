// Adjudication by the exact solver: the apply step.
//
// The self-play driver and the arena (tree_game.h selfplay_move_game,
// arena.hip k_arena_move) end a game whose searched move left a non-terminal root with
// at most K empties and put that root into the pending slot of the move's
// `finished` word; a game that ended on the board leaves its final position
// there with player 0. Slots of moves that ended nothing stay all-zero (the
// caller zeroes the array before the moves), which the solver classifies as a
// terminal position at the cost of one look. After the solver has run over the
// whole array, k_adjudicate_apply turns its scores into the words consumers read:
//
//   slot empty (no discs)     margin = INT32_MIN              (self-play only)
//   player 0 (board-ended)    margin = black - white discs; finished untouched
//   player 1 / 2              margin = score, negated for white;
//                             finished |= outcome of the margin (1 draw,
//                             2 black, 3 white), or kFinSolverFlag alone when
//                             the solver flagged the position
//
// One thread per slot, every word has one writer, nothing depends on the grid.

#include <hip/hip_runtime.h>
#include <limits.h>

#include "bitboard.h"
#include "engine.h"
#include "kernels.h"

namespace oamd {

namespace {

__global__ __launch_bounds__(256) void k_adjudicate_apply(const oamd_position* pending, const int32_t* score,
                                                          const int32_t* flags, int64_t n, int32_t* finished,
                                                          int32_t* margin, int accumulate) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const oamd_position p = pending[i];
    if ((p.player1_discs | p.player2_discs) == 0) {
        if (margin && !accumulate) margin[i] = INT_MIN;
        return;
    }
    if (p.player == 0) {
        if (margin) margin[i] = popcount64(p.player1_discs) - popcount64(p.player2_discs);
        return;
    }
    if (flags[i] != 0) {
        finished[i] |= kFinSolverFlag;
        if (margin) margin[i] = INT_MIN;
        return;
    }
    const int m = p.player == 2 ? -score[i] : score[i];
    finished[i] |= m > 0 ? 2 : (m < 0 ? 3 : 1);
    if (margin) margin[i] = m;
}

}  // namespace

void launch_adjudicate_apply(const oamd_position* pending, const int32_t* score, const int32_t* flags, int64_t n,
                             int32_t* finished, int32_t* margin, int accumulate, hipStream_t s) {
    if (n > 0)
        hipLaunchKernelGGL(k_adjudicate_apply, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pending, score,
                           flags, n, finished, margin, accumulate);
}

}  // namespace oamd
