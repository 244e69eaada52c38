// Launchers of the packed replay buffer's kernels (replay.hip), called by the
// C ABI (capi.hip). The storage itself belongs to the caller: oamd_replay_view
// (include/othello_mcts_amd.h) only points at it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/othello_mcts_amd.h"

namespace oamd {

// counters[] slots of oamd_replay_view
constexpr int kReplayHead = 0, kReplaySize = 1, kReplayGames = 2, kReplayFlags = 3;

// One move of every game: pack and stage the transform-0 slice of the played
// games, then commit the games that finished on this move to the ring in
// ascending game order (two launches, stream order).
void launch_replay_add(const oamd_replay_view& V, const int32_t* actions, const int32_t* finished,
                       const float* features, const float* policy, hipStream_t s);
// n samples: id = 8 * position + transform, positions counted from the oldest.
void launch_replay_gather(const oamd_replay_view& V, const int64_t* ids, int64_t n, float* features,
                          float* policy, float* value, hipStream_t s);

}  // namespace oamd
