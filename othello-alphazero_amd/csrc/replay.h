// Launchers of the packed replay buffer's kernels (replay.hip), called by the
// C ABI (capi.hip). The storage itself belongs to the caller: oamd_replay_view
// (include/othello_mcts_amd.h) only points at it.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/othello_mcts_amd.h"
#include "solver.h"

namespace oamd {

// counters[] slots of oamd_replay_view
constexpr int kReplayHead = 0, kReplaySize = 1, kReplayGames = 2, kReplayFlags = 3;
// relabel_counters[] slots of oamd_replay_relabel_endgames
constexpr int kRelabelSolved = 0, kRelabelGaveUp = 1, kRelabelLeft = 2, kRelabelTaken = 3;

// One move of every game: pack and stage the transform-0 slice of the played
// games, then commit the games that finished on this move to the ring in
// ascending game order (two launches, stream order). exact: the ring's exact
// bytes (a committed slot is reset to OAMD_REPLAY_EXACT_UNKNOWN), or nullptr.
void launch_replay_add(const oamd_replay_view& V, int8_t* exact, const int32_t* actions, const int32_t* finished,
                       const float* features, const float* policy, hipStream_t s);
// n samples: id = 8 * position + transform, positions counted from the oldest.
void launch_replay_gather(const oamd_replay_view& V, const int64_t* ids, int64_t n, float* features,
                          float* policy, float* value, hipStream_t s);


// The caller's relabel workspace for `budget` list rows, widest alignment
// first: the solver's own workspace (the split solver's when `split`), the
// position list, then the int32 arrays (slot list, move_scores, score,
// best_action, flags).
struct RelabelWorkspace {
    void* solver;
    oamd_position* pos;
    int32_t *slots, *move_scores, *score, *best_action, *flags;
    RelabelWorkspace(void* base, int64_t budget, bool split = false) {
        char* p = static_cast<char*>(base);
        solver = p;
        p += split ? solve_split_workspace_bytes(budget) : solve_workspace_bytes(budget);
        pos = reinterpret_cast<oamd_position*>(p);
        p += budget * (int64_t)sizeof(oamd_position);
        slots = reinterpret_cast<int32_t*>(p);
        move_scores = slots + budget;
        score = move_scores + budget * 65;
        best_action = score + budget;
        flags = best_action + budget;
    }
};
inline int64_t relabel_workspace_bytes(int64_t budget, bool split = false) {
    return (split ? solve_split_workspace_bytes(budget) : solve_workspace_bytes(budget)) +
           budget * (int64_t)(sizeof(oamd_position) + (1 + 65 + 3) * sizeof(int32_t));
}
// Exact value targets for the ring's last plies: list the candidates (live
// positions in age order, at most `budget`), solve them, apply the answers
// (list kernel, launch_solve or with `split` launch_solve_split, apply kernel;
// stream order).
void launch_replay_relabel(const oamd_replay_view& V, int8_t* exact, int64_t* relabel_counters, int32_t max_empties,
                           int64_t budget, int64_t node_limit, int32_t policy_mode, int32_t retry, void* workspace,
                           int32_t compute_units, hipStream_t s, bool split = false);

}  // namespace oamd
