// Search-tree kernels: one 64-lane wavefront per game.
//
// The reference runs num_threads CPU threads per game, each selecting
// batch_size leaves under a mutex with virtual loss, sending them through the
// NN and backing them up (search_thread.cpp:47-260). Here a round of a game
// (every thread backs up its previous batch and selects its next one, see
// k_tree) is one wave of k_tree followed by one row block of the NN launch;
// all games of the engine run in the same launches. Lanes parallelise what is parallel inside one game:
// the child scan of PUCT (lane = child), virtual loss and backup (lane = path
// depth), expansion (lane = square), feature gathers (lane = history slot).
// The sequential dependence between the L descents (each sees the previous
// descents' virtual losses) is kept exactly.
//
// Floating point: compiled with -ffp-contract=off and IEEE division/sqrt so
// that every PUCT score, virtual loss and backup is bit-identical to the
// reference's float arithmetic (search_thread.cpp:163-166, 198-249, 270-280).
//
// This unit holds the round kernels (k_tree, k_tree_wide and free-running
// self-play's k_tree_free), the step-API kernels, the game lifecycle and root
// read-outs and the batched bitboards. The search itself is tree_search.h over
// wave.h, the game lifecycle's device functions tree_game.h; selfplay.hip (the
// self-play move) and arena.hip are built from the same headers. The three
// round kernels share one unit on purpose: k_tree_free compiled in a unit
// without k_tree comes out with another register allocation.

#include <hip/hip_runtime.h>

#include "bitboard.h"
#include "engine.h"
#include "kernels.h"
#include "wave.h"

// Diagnostic build only (-DOAMD_TREE_STAMPS, tools/tree_stamps.py): cycle
// sums of k_tree's phases (s_memtime), per wave in LDS (k_tree blocks are one
// wave), added to g_tree_stamps when the wave ends. Nothing else reads them.
#ifdef OAMD_TREE_STAMPS
namespace oamd {
enum TreeStamp {
    kTsWaves, kTsCycles, kTsDescent, kTsLevels, kTsLeaves, kTsPost, kTsBackup, kTsBackedUp, kTsTerminal,
    kTsMaxCycles, kTsBatches, kTsSelect, kTsExpand, kTsPathW, kTsNoise, kTsRefill, kTsCount
};
__device__ unsigned long long g_tree_stamps[kTsCount];
__shared__ unsigned long long ts_acc[kTsCount];
}  // namespace oamd
#define TS_T(v) const unsigned long long v = __builtin_amdgcn_s_memtime()
#define TS_ADD(i, x) do { if (lane_id() == 0) ts_acc[i] += (unsigned long long)(x); } while (0)
#endif

#include "tree_game.h"
#include "tree_search.h"

namespace oamd {

__device__ __forceinline__ void tree_round_kernel(const EngineView& E, int g0, int do_backup, int do_select, int t0,
                                                  int t1, int B, int* cnt_add, int* cnt_reset, int fresh, int budget,
                                                  int max_cuts, int timed, int* cuts_out) {
    const int g = g0 + (int)blockIdx.x;
    const int lane = lane_id();
    if (cnt_reset && blockIdx.x == 0 && lane == 0) *cnt_reset = 0;
    count_launch(E);
    // cuts_out (adaptive extra rounds, capi.hip): [0] the most cuts any game
    // of the launch's group used in this search, [1] the fewest empty squares
    // of an active game's root; reset by the search's first round, set by its
    // final (backup-only) round
    if (cuts_out && fresh && blockIdx.x == 0 && lane == 0) {
        cuts_out[0] = 0;
        cuts_out[1] = 64;
    }
#ifdef OAMD_TREE_STAMPS
    if (lane < kTsCount) ts_acc[lane] = 0;
    __builtin_amdgcn_wave_barrier();
    TS_T(tk0);
#endif
    GameState* gs = E.games + g;
    const size_t base = (size_t)g * E.cap;
    const int flags = gs->flags;
    if (!(flags & kActive)) {
        if (do_select) {
            for (int i = t0 * B; i < t1 * B; ++i) {
                const int r = g * E.L + i;
                if (lane == 0) {
                    E.leaf[r] = -1;
                    E.depth[r] = 0;
                    E.trans[r] = 0;
                    if (E.exact_empties > 0) E.exact[r] = kExactFlagNone;
                }
                write_feature_meta(E, r, 1, 0, false);
            }
        }
        return;
    }
    // a game on a fast search stops selecting after its own steps and idles
    // for the launch's remaining rounds
    const bool fast = search_is_fast(E, gs);
    WaveSearch ws;
    ws.load(gs);
    const int count0 = ws.count;
    const int rp = budget > 0 && !fresh ? gs->resume : t0;  // this round's first thread
    ws.cuts = budget > 0 && !fresh ? gs->cuts : 0;
    search_round(E, g, gs, base, t0, t1, B, do_backup != 0, do_select != 0, fresh != 0, rp, budget, max_cuts, cnt_add,
                 g0 * E.L, fast, ws);
    if (lane == 0) {
        if (budget > 0) {
            gs->resume = ws.cut_at >= 0 ? ws.cut_at : rp;
            // a search that ran out of cuts reports max_cuts + 1 (cuts_out)
            gs->cuts = ws.over ? max_cuts + 1 : ws.cuts;
        }
        if (cuts_out && !do_select) {
            const NodePos& rp = E.pos[base + gs->root];
            atomicMax(cuts_out, ws.cuts);
            atomicMin(cuts_out + 1, 64 - __popcll(rp.p1 | rp.p2));
        }
        ws.publish(gs);
#ifdef OAMD_TREE_STAMPS
        {
            TS_T(tk1);
            ts_acc[kTsWaves] = 1;
            ts_acc[kTsCycles] = tk1 - tk0;
            for (int i = 0; i < kTsCount; ++i) {
                if (i == kTsMaxCycles) atomicMax(&g_tree_stamps[i], tk1 - tk0);
                else atomicAdd(&g_tree_stamps[i], ts_acc[i]);
            }
        }
#endif
        add_counters(E, ws.acc, timed != 0, (unsigned)(ws.count - count0));
    }
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(48))) void k_tree(EngineView E, int g0, int do_backup,
                                                                                int do_select, int t0, int t1, int B,
                                                                                int* cnt_add, int* cnt_reset, int fresh,
                                                                                int budget, int max_cuts, int timed,
                                                                                int* cuts_out) {
    tree_round_kernel(E, g0, do_backup, do_select, t0, t1, B, cnt_add, cnt_reset, fresh, budget, max_cuts, timed,
                      cuts_out);
}

// The same round without the register cap (114 VGPRs, no spills) for launches
// of at most kWideTreeGames games (the single-game drop-in MCTS and other
// small engines): their NN launches leave most CUs free, so a tree wave needs
// no room beside ResNet waves, and its leaves' serial chain is the search's
// critical path.
constexpr int kWideTreeGames = 16;
__global__ __launch_bounds__(64) void k_tree_wide(EngineView E, int g0, int do_backup, int do_select, int t0, int t1,
                                                  int B, int* cnt_add, int* cnt_reset, int fresh, int budget,
                                                  int max_cuts, int timed, int* cuts_out) {
    tree_round_kernel(E, g0, do_backup, do_select, t0, t1, B, cnt_add, cnt_reset, fresh, budget, max_cuts, timed,
                      cuts_out);
}

// ---------------------------------------------------------------------------
// Free-running self-play (oamd_engine_selfplay_steps, capi.hip): every game
// plays `n_moves` moves on its own; a round of this kernel is, per game, one
// round of its current search (search_round) and, in the round that completes
// the search, the move (selfplay_move_game: choice, 8-fold targets, apply,
// restart) and the first round of its next search. Per game the operations
// and their order are exactly those of n x (search + selfplay_move): the
// rounds of one search, then its move, then the next search's rounds (a chain
// cut only moves a round boundary, see k_tree). But no game waits for the
// others at a move: a game whose search needs more rounds (chains near its
// end) lags by those rounds while the others go on, so the group's ResNet
// launches stay full and no extra rounds are needed. The host enqueues rounds
// until `remaining` (games of the group with moves left) reads 0.
// ---------------------------------------------------------------------------
//
// Work budget (sim_budget > 0, per-move outputs only): n_moves
// is the number of output slices and the most moves a game plays; a game
// stops after the move whose search brought the nominal simulations (steps x
// L) of the searches it started in this call to sim_budget or more, so it
// overshoots by less than one search. Every slice of every game is pre-filled
// with action -1 / finished 0 ("nothing played"), and the played moves
// overwrite a prefix of them.
__global__ void k_free_begin(EngineView E, int g0, int ng, int n_moves, int32_t* remaining, int32_t* actions,
                             int32_t* finished, int per_move, int sim_budget) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;  // *remaining zeroed by the caller
    if (i >= ng) return;
    const int g = g0 + i;
    GameState* gs = E.games + g;
    const bool active = (gs->flags & kActive) != 0 && n_moves > 0;
    gs->moves_left = active ? n_moves : 0;
    gs->sims_left = active ? sim_budget : 0;
    gs->fresh = 1;
    if (active) atomicAdd(remaining, 1);
    const bool fill = !active || sim_budget > 0;
    for (int m = 0; fill && m < (per_move ? n_moves : (n_moves > 0 ? 1 : 0)); ++m) {
        if (actions) actions[(size_t)m * E.G + g] = -1;
        if (finished) finished[(size_t)m * E.G + g] = 0;
    }
}

__global__ __launch_bounds__(64) __attribute__((amdgpu_num_vgpr(48))) void k_tree_free(
    EngineView E, int g0, int B, int* cnt_add, int* cnt_reset, int budget, int timed, SelfplayParams sp, int n_moves,
    int per_move, int32_t* actions, int32_t* finished, float* feat_out, float* pol_out, int32_t* remaining,
    int sim_budget) {
    const int g = g0 + (int)blockIdx.x;
    const int lane = lane_id();
    if (cnt_reset && blockIdx.x == 0 && lane == 0) *cnt_reset = 0;
    count_launch(E);
    GameState* gs = E.games + g;
    const size_t base = (size_t)g * E.cap;
    int moves = gs->moves_left;
    if (moves <= 0) return;
    const int T = E.L / B;
    const bool fresh = gs->fresh != 0;
    WaveSearch ws;
    ws.load(gs);
    unsigned grown = 0;  // children created (the node count restarts with a finished game)
    int count0 = ws.count;
    int rp = fresh || budget <= 0 ? 0 : gs->resume;
    ws.cuts = fresh ? 0 : gs->cuts;
    // no extra rounds to budget for: a game may cut its chains any number of times
    constexpr int kNoCap = 0x3FFFFFFF;
    const bool fast = search_is_fast(E, gs);  // this round's search (the ply of its root)
    const bool done = search_round(E, g, gs, base, 0, T, B, true, true, fresh, rp, budget, kNoCap, cnt_add, g0 * E.L,
                                   fast, ws);
    if (done) {
        // the search has returned: publish the wave's state, then the move
        // (k_selfplay_move's), which reads it from memory
        if (lane == 0) ws.publish(gs);
        grown += (unsigned)(ws.count - count0);
        __builtin_amdgcn_wave_barrier();
        wait_stores();
        const size_t slot = per_move ? (size_t)(n_moves - moves) * E.G : 0;
        const size_t C = 1 + 2 * (size_t)E.H;
        selfplay_move_game(E, sp, g, actions ? actions + slot : nullptr, finished ? finished + slot : nullptr,
                           feat_out ? feat_out + slot * 8 * C * 64 : nullptr, pol_out ? pol_out + slot * 8 * 65 : nullptr,
                           sp.adj_pending ? sp.adj_pending + slot : nullptr, fast);
        --moves;
        if (sim_budget > 0) {
            // work budget: the search just played is charged its nominal size;
            // the move that uses the budget up is the game's last of the call
            const int left = __builtin_amdgcn_readfirstlane(gs->sims_left) - search_steps_of(E, fast) * E.L;
            if (lane == 0) gs->sims_left = left;
            if (left <= 0) moves = 0;
        }
        __builtin_amdgcn_wave_barrier();
        wait_stores();  // (a compiler barrier too: the reloads below see the move's stores)
        ws.load(gs);
        count0 = ws.count;
        rp = 0;
        if (moves > 0) {  // the next search's first round, in this same round
            const bool fast2 = search_is_fast(E, gs);  // the new root's ply (and key, after a restart)
            search_round(E, g, gs, base, 0, T, B, true, true, true, 0, budget, kNoCap, cnt_add, g0 * E.L, fast2, ws);
        }
    }
    if (lane == 0) {
        gs->moves_left = moves;
        gs->fresh = 0;
        gs->resume = ws.cut_at >= 0 ? ws.cut_at : rp;
        gs->cuts = ws.cuts;
        ws.publish(gs);
        if (moves == 0 && remaining) atomicSub(remaining, 1);
        add_counters(E, ws.acc, timed != 0, grown + (unsigned)(ws.count - count0));
    }
}

// ---------------------------------------------------------------------------
// Packed -> fp32 features (B, 1+2H, 8, 8) for the external-evaluator path.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float plane_value(const uint64_t* row, int c, int sq_src) {
    if (c == 0) return (float)(row[0] & 1ULL);
    const uint64_t bb = row[1 + c];  // c = 1 + 2h -> word 2 + 2h; c = 2 + 2h -> 3 + 2h
    return (float)((bb >> (63 - sq_src)) & 1ULL);
}

__global__ __launch_bounds__(256) void k_features_f32(EngineView E, float* out, int row_begin,
                                                      int rows) {
    const int rr = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (rr >= rows) return;
    const int p = threadIdx.x & 63;
    const uint64_t* row = E.feat + (size_t)(row_begin + rr) * E.FW;
    const uint64_t meta = row[0];
    const bool valid = (meta >> 16) & 1ULL;
    const int t = (int)((meta >> 8) & 7ULL);
    const int src = inverse_transform(p, t);
    const int C = 1 + 2 * E.H;
    float* o = out + (size_t)rr * C * 64;
    for (int c = 0; c < C; ++c) o[c * 64 + p] = valid ? plane_value(row, c, src) : 0.0f;
}

__global__ __launch_bounds__(256) void k_set_evaluation(EngineView E, const float* policy,
                                                        const float* value, int row_begin,
                                                        int rows) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx < rows * 65) E.policy[(size_t)row_begin * 65 + idx] = policy[idx];
    if (idx < rows) E.value[row_begin + idx] = value[idx];
}

// 1 = the row is a non-terminal leaf of a batch that waits for the NN this
// round (a thread that ran out of batches, or whose last batch was all
// terminal, has none: its rows are stale)
__global__ __launch_bounds__(256) void k_leaf_flags(EngineView E, uint8_t* flags) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= E.G * E.L) return;
    const int g = r / E.L, t = (r % E.L) / E.B;
    const bool pend = (E.tstate[(size_t)g * E.L + t] & kTstatePend) != 0;
    flags[r] = (uint8_t)(pend && ((E.feat[(size_t)r * E.FW] >> 16) & 1ULL));
}

// ---------------------------------------------------------------------------
// Game state (tree_game.h): reset, moves, root statistics, self-play targets
// ---------------------------------------------------------------------------
__global__ void k_reset(EngineView E, int game, uint64_t seed) {
    const int g = game >= 0 ? game : (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (g >= E.G || (game >= 0 && threadIdx.x + blockIdx.x != 0)) return;
    init_game(E, g, seed);
}

__global__ void k_apply_actions(EngineView E, const int32_t* actions) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.G) return;
    const int a = actions[g];
    if (a < 0 || !(E.games[g].flags & kActive)) return;
    move_root(E, g, a);
}

__global__ void k_apply_one(EngineView E, int g, int action) { move_root(E, g, action); }

// Root summary per game: info + visits/q indexed by action.
__global__ __launch_bounds__(64) void k_root_stats(EngineView E, int game_begin,
                                                   oamd_root_info* info, int32_t* visits,
                                                   float* q, int by_action) {
    const int g = game_begin + blockIdx.x;
    const int lane = lane_id();
    const GameState* gs = E.games + g;
    const size_t base = (size_t)g * E.cap;
    const int root = gs->root;
    const NodeLink lk = load_link(E.link + base + root);
    const NodePos rp = E.pos[base + root];
    const int nc = lk.n_children;
    int32_t* vo = visits + (size_t)blockIdx.x * 65;
    float* qo = q + (size_t)blockIdx.x * 65;
    if (by_action) {
        // lane = square; pass in slot 64
        vo[lane] = 0;
        qo[lane] = 0.0f;
        if (lane == 0) {
            vo[64] = 0;
            qo[64] = 0.0f;
        }
        __builtin_amdgcn_wave_barrier();
        if (nc > 0) {
            if (rp.legal) {
                if ((rp.legal >> (63 - lane)) & 1ULL) {
                    const int j = child_index_of(rp.legal, nc, lane);
                    const NodeStat s = load_stat(E.stat + base + lk.first_child + j);
                    vo[lane] = s.n;
                    qo[lane] = s.q;
                }
            } else if (lane == 0) {
                const NodeStat s = load_stat(E.stat + base + lk.first_child);
                vo[64] = s.n;
                qo[64] = s.q;
            }
        }
    } else if (lane < nc) {
        const NodeStat s = load_stat(E.stat + base + lk.first_child + lane);
        vo[lane] = s.n;
        qo[lane] = s.q;
    }
    if (lane == 0) {
        oamd_root_info& I = info[blockIdx.x];
        I.position.player = lk.player;
        I.position.reserved = 0;
        I.position.player1_discs = rp.p1;
        I.position.player2_discs = rp.p2;
        I.position.legal_moves = rp.legal;
        I.position.next_legal_moves = rp.next_legal;
        I.num_children = nc;
        I.visit_count = E.stat[base + root].n;
        I.overflow = (gs->flags & (kOverflow | kDepthCap)) ? gs->flags : 0;
        I.reserved = 0;
        I.node_count = gs->count;
    }
}

// Stored priors of every game's root children by action (lane = square, pass
// in slot 64), 0 where there is no child: the P of k_root_stats' N and Q.
__global__ __launch_bounds__(64) void k_root_priors(EngineView E, float* priors) {
    const int g = blockIdx.x;
    const int lane = lane_id();
    const size_t base = (size_t)g * E.cap;
    const int root = E.games[g].root;
    const NodeLink lk = load_link(E.link + base + root);
    const uint64_t legal = E.pos[base + root].legal;
    const int nc = lk.n_children;
    float* po = priors + (size_t)g * 65;
    float p = 0.0f, pass = 0.0f;
    if (nc > 0) {
        if (legal) {
            if ((legal >> (63 - lane)) & 1ULL) p = E.stat[base + lk.first_child + child_index_of(legal, nc, lane)].p;
        } else {
            pass = E.stat[base + lk.first_child].p;
        }
    }
    po[lane] = p;
    if (lane == 0) po[64] = pass;
}

__global__ __launch_bounds__(512) void k_self_play_data(EngineView E, int g, float* feat_out,
                                                        float* pol_out) {
    write_targets(E, g, threadIdx.x >> 6, root_target_count(E, g), feat_out, pol_out);
}

// Per-game search mask (oamd_engine_set_active): k_tree, k_selfplay_move and
// k_apply_actions leave inactive games alone. active == nullptr: every game.
__global__ void k_set_active(EngineView E, const uint8_t* active) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.G) return;
    GameState* gs = E.games + g;
    const bool on = !active || active[g] != 0;
    gs->flags = (gs->flags & ~(int)kActive) | (on ? (int)kActive : 0);
}

// Games whose node pool overflowed / whose descent hit the depth cap (sticky
// flags since the game's last reset).
__global__ void k_status(EngineView E, int32_t* out) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= E.G) return;
    const int f = E.games[g].flags;
    if (f & kOverflow) atomicAdd(out + 0, 1);
    if (f & kDepthCap) atomicAdd(out + 1, 1);
}

// ---------------------------------------------------------------------------
// Batched bitboards (position.h) — elementwise, one position per lane.
// ---------------------------------------------------------------------------
__global__ void k_legal_moves(const uint64_t* me, const uint64_t* opp, uint64_t* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = legal_moves(me[i], opp[i]);
}

__global__ void k_flips(const uint64_t* mv, const uint64_t* me, const uint64_t* opp, uint64_t* out,
                        int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = flips(mv[i], me[i], opp[i]);
}

__global__ void k_apply_positions(const Pos* in, const int32_t* actions, Pos* out, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = apply_action(in[i], actions[i]);
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
void launch_tree(const EngineView& E, hipStream_t s, bool do_backup, bool do_select, int T, int B,
                 int g0, int ng, int t0, int t1, int* cnt_add, int* cnt_reset, bool fresh, int budget,
                 int max_cuts, bool timed, int* cuts_out) {
    if (ng < 0) ng = E.G - g0;
    if (t1 < 0) t1 = T;
    if (T * B != E.L || t0 < 0 || t1 > T || t0 >= t1) return;  // caller validated; never launch on a mismatched layout
    if (ng > 0 && (do_backup || do_select))
        hipLaunchKernelGGL(ng <= kWideTreeGames ? k_tree_wide : k_tree, dim3(ng), dim3(64), 0, s, E, g0,
                           (int)do_backup, (int)do_select, t0, t1, B, do_select ? cnt_add : nullptr, cnt_reset,
                           (int)fresh, budget, max_cuts, (int)timed, cuts_out);
}
void launch_free_begin(const EngineView& E, int g0, int ng, int n_moves, int32_t* remaining, int32_t* actions,
                       int32_t* finished, int per_move, int sim_budget, hipStream_t s) {
    if (ng > 0)
        hipLaunchKernelGGL(k_free_begin, dim3(blocks_for(ng, 256)), dim3(256), 0, s, E, g0, ng, n_moves, remaining,
                           actions, finished, per_move, sim_budget);
}
void launch_tree_free(const EngineView& E, hipStream_t s, int g0, int ng, int B, int* cnt_add, int* cnt_reset,
                      int budget, bool timed, const SelfplayParams& sp, int n_moves, int per_move, int32_t* actions,
                      int32_t* finished, float* feat, float* pol, int32_t* remaining, int sim_budget) {
    if (ng > 0 && B > 0 && E.L % B == 0)
        hipLaunchKernelGGL(k_tree_free, dim3(ng), dim3(64), 0, s, E, g0, B, cnt_add, cnt_reset, budget, (int)timed, sp,
                           n_moves, per_move, actions, finished, feat, pol, remaining, sim_budget);
}
void launch_features_f32(const EngineView& E, float* out, int row_begin, int rows, hipStream_t s) {
    if (rows > 0) hipLaunchKernelGGL(k_features_f32, dim3(blocks_for(rows, 4)), dim3(256), 0, s, E, out, row_begin, rows);
}
void launch_set_evaluation(const EngineView& E, const float* pol, const float* val, int row_begin,
                           int rows, hipStream_t s) {
    if (rows > 0)
        hipLaunchKernelGGL(k_set_evaluation, dim3(blocks_for((int64_t)rows * 65, 256)), dim3(256), 0, s, E,
                           pol, val, row_begin, rows);
}
void launch_leaf_flags(const EngineView& E, uint8_t* flags, hipStream_t s) {
    hipLaunchKernelGGL(k_leaf_flags, dim3(blocks_for((int64_t)E.G * E.L, 256)), dim3(256), 0, s, E, flags);
}
void launch_reset(const EngineView& E, int game, uint64_t seed, hipStream_t s) {
    if (game >= 0) hipLaunchKernelGGL(k_reset, dim3(1), dim3(1), 0, s, E, game, seed);
    else hipLaunchKernelGGL(k_reset, dim3(blocks_for(E.G, 64)), dim3(64), 0, s, E, -1, seed);
}
void launch_apply_actions(const EngineView& E, const int32_t* actions, hipStream_t s) {
    hipLaunchKernelGGL(k_apply_actions, dim3(blocks_for(E.G, 64)), dim3(64), 0, s, E, actions);
}
void launch_apply_one(const EngineView& E, int g, int action, hipStream_t s) {
    hipLaunchKernelGGL(k_apply_one, dim3(1), dim3(1), 0, s, E, g, action);
}
void launch_root_stats(const EngineView& E, int game_begin, int n_games, oamd_root_info* info,
                       int32_t* visits, float* q, int by_action, hipStream_t s) {
    hipLaunchKernelGGL(k_root_stats, dim3(n_games), dim3(64), 0, s, E, game_begin, info, visits, q, by_action);
}
void launch_root_priors(const EngineView& E, float* priors, hipStream_t s) {
    hipLaunchKernelGGL(k_root_priors, dim3(E.G), dim3(64), 0, s, E, priors);
}
void launch_self_play_data(const EngineView& E, int g, float* feat, float* pol, hipStream_t s) {
    hipLaunchKernelGGL(k_self_play_data, dim3(1), dim3(512), 0, s, E, g, feat, pol);
}
void launch_set_active(const EngineView& E, const uint8_t* active, hipStream_t s) {
    hipLaunchKernelGGL(k_set_active, dim3(blocks_for(E.G, 64)), dim3(64), 0, s, E, active);
}
void launch_status(const EngineView& E, int32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_status, dim3(blocks_for(E.G, 64)), dim3(64), 0, s, E, out);
}
void launch_legal_moves(const uint64_t* me, const uint64_t* opp, uint64_t* out, int64_t n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_legal_moves, dim3(blocks_for(n, 256)), dim3(256), 0, s, me, opp, out, n);
}
void launch_flips(const uint64_t* mv, const uint64_t* me, const uint64_t* opp, uint64_t* out, int64_t n,
                  hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_flips, dim3(blocks_for(n, 256)), dim3(256), 0, s, mv, me, opp, out, n);
}
void launch_apply_positions(const Pos* in, const int32_t* actions, Pos* out, int64_t n, hipStream_t s) {
    if (n > 0) hipLaunchKernelGGL(k_apply_positions, dim3(blocks_for(n, 256)), dim3(256), 0, s, in, actions, out, n);
}

}  // namespace oamd

namespace oamd {
int tree_read_stamps(unsigned long long* out, long long n, int reset) {
#ifdef OAMD_TREE_STAMPS
    if (n > kTsCount) n = kTsCount;
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tree_stamps), (size_t)n * 8, 0, hipMemcpyDeviceToHost) != hipSuccess)
        return -1;
    if (reset) {
        unsigned long long z[kTsCount] = {};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_tree_stamps), z, sizeof(z), 0, hipMemcpyHostToDevice) != hipSuccess)
            return -1;
    }
    return 0;
#else
    (void)out;
    (void)n;
    (void)reset;
    return -2;
#endif
}
}  // namespace oamd
