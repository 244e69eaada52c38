// Exact endgame solver on the device (the split solver §15; the algorithm is solver.h).
//
//   k_solve         work item = one of the n x 65 (position, action) slots; one
//                   lane per item, 64-thread workgroups. Every lane runs the
//                   same solve_step loop on its own searcher, whose stack is
//                   kSolveDepth x 7 words of LDS laid out [level][word][lane].
//                   A lane whose item is done stores the slot's score and its
//                   node word and takes the next slot from a global counter, so
//                   a wave lasts as long as the work. A slot that is no legal
//                   root action (or belongs to a flagged position) stores
//                   OAMD_SOLVE_NONE and costs one classification.
//   k_solve_reduce  one thread per position, after k_solve in stream order:
//                   score, best_action, flags and the node total from the 65
//                   slots (solve_reduce).
//
// Every slot is written by exactly one lane and no kernel reads what the same
// launch wrote, so the outputs do not depend on the grid or on which lane got
// which slot.

#include <hip/hip_runtime.h>

#include "bitboard.h"
#include "solver.h"

namespace oamd {

namespace {

constexpr int kSolveThreads = 64;
constexpr int kStepsPerRound = 32;  // solve_steps between two looks at the item counter
// 16 levels x 7 words x 64 lanes x 4 bytes = 28,672 bytes per workgroup (one
// wave): 5 waves per CU out of 160 KiB of LDS
constexpr int kWavesPerCU = 5;

struct LdsStack {
    uint32_t* base;  // &stack[0][0][lane]
    __device__ __forceinline__ void put(int level, int word, uint32_t v) {
        base[(level * kSolveFrameWords + word) * kSolveThreads] = v;
    }
    __device__ __forceinline__ uint32_t get(int level, int word) const {
        return base[(level * kSolveFrameWords + word) * kSolveThreads];
    }
};

__global__ __launch_bounds__(kSolveThreads) void k_solve(const oamd_position* pos, int64_t n, int32_t max_empties,
                                                         int64_t node_limit, int32_t* move_scores, int64_t* words,
                                                         unsigned long long* counter) {
    __shared__ uint32_t s_stack[kSolveDepth * kSolveFrameWords * kSolveThreads];
    LdsStack st{s_stack + threadIdx.x};
    const unsigned long long total = (unsigned long long)n * 65ULL;
    SolveState s;
    s.status = kSolveDone;
    s.nodes = 0;
    s.result = OAMD_SOLVE_NONE;
    s.sp = 0;
    s.me = s.opp = s.moves = 0;
    s.alpha = s.beta = s.best = s.passed = 0;
    unsigned long long slot = 0;
    bool have = false;  // this lane holds a slot whose result is not stored yet
    bool dry = false;   // the counter ran past the last slot
    for (;;) {
        if (!have && !dry) {
            slot = atomicAdd(counter, 1ULL);
            if (slot >= total) {
                dry = true;
            } else {
                have = true;
                const oamd_position p = pos[slot / 65];
                const int a = (int)(slot % 65);
                const SolveRoot r = solve_classify(p.player, p.player1_discs, p.player2_discs, max_empties);
                if (solve_is_root_action(r, a)) {
                    solve_begin(s, st, r.me, r.opp, a, node_limit);
                } else {
                    s.status = kSolveDone;
                    s.result = OAMD_SOLVE_NONE;
                    s.nodes = 0;
                    s.sp = -1;  // no item: the slot's word is 0
                }
            }
        }
        if (__ballot(have) == 0ULL) break;  // every lane is dry and has stored its last slot
        if (have) {
            for (int k = 0; k < kStepsPerRound; ++k)
                if (s.status == kSolveRunning) solve_step(s, st, node_limit);
            if (s.status != kSolveRunning) {
                move_scores[slot] = s.status == kSolveDone ? s.result : OAMD_SOLVE_NONE;
                words[slot] = s.sp < 0 ? 0LL : (s.nodes | (int64_t)s.status << kSolveStatusShift);
                have = false;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_solve_reduce(const oamd_position* pos, int64_t n, int32_t max_empties,
                                                      const int32_t* move_scores, const int64_t* words,
                                                      int32_t* score, int32_t* best_action, int32_t* flags,
                                                      int64_t* nodes) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const oamd_position p = pos[i];
    solve_reduce(p.player, p.player1_discs, p.player2_discs, max_empties, move_scores + i * 65, words + i * 65,
                 score ? score + i : nullptr, best_action ? best_action + i : nullptr, flags ? flags + i : nullptr,
                 nodes ? nodes + i : nullptr);
}

// ---- split solver ----
//
//   k_solve_plan          one thread per (position, root action rank): the
//                         SolvePlan (solve_plan).
//   k_solve_items         launched once per phase; k_solve's shape (one
//                         searcher per lane, the same LDS stack, refill from a
//                         global counter, uniform step loop) over the phase's
//                         slots: n x 16 plans in phase A, n x 256 (plan, move
//                         rank) slots in phase B, which reads the phase A
//                         results of the earlier launch. Moves are taken by
//                         the ordered pick. A slot without an item stores
//                         OAMD_SOLVE_NONE and a zero word.
//   k_solve_split_reduce  one thread per position: all 65 move_scores, score,
//                         best_action, flags and nodes (solve_reduce_split).
//
// As above every word has one writer per launch and no launch reads what it wrote.

__global__ __launch_bounds__(256) void k_solve_plan(const oamd_position* pos, int64_t n, int32_t max_empties,
                                                    SolvePlan* plan) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * kSplitRanks) return;
    const oamd_position p = pos[t / kSplitRanks];
    plan[t] = solve_plan(solve_classify(p.player, p.player1_discs, p.player2_discs, max_empties),
                         (int)(t % kSplitRanks));
}

__global__ __launch_bounds__(kSolveThreads) void k_solve_items(const SolvePlan* plan, unsigned long long total,
                                                               int32_t phase, const int32_t* a_scores,
                                                               const int64_t* a_words, int64_t node_limit,
                                                               int32_t* out_scores, int64_t* out_words,
                                                               unsigned long long* counter) {
    __shared__ uint32_t s_stack[kSolveDepth * kSolveFrameWords * kSolveThreads];
    LdsStack st{s_stack + threadIdx.x};
    SolveState s;
    s.status = kSolveDone;
    s.nodes = 0;
    s.result = OAMD_SOLVE_NONE;
    s.sp = 0;
    s.me = s.opp = s.moves = 0;
    s.alpha = s.beta = s.best = s.passed = 0;
    unsigned long long slot = 0;
    bool have = false;  // this lane holds a slot whose result is not stored yet
    bool dry = false;   // the counter ran past the last slot
    for (;;) {
        if (!have && !dry) {
            slot = atomicAdd(counter, 1ULL);
            if (slot >= total) {
                dry = true;
            } else {
                have = true;
                const unsigned long long rec = phase ? slot / kSplitRanks : slot;
                const SolvePlan p = plan[rec];
                int alpha;
                const uint64_t m = solve_split_item(p, phase, (int)(slot % kSplitRanks), phase ? a_scores[rec] : 0,
                                                    phase ? a_words[rec] : 0LL, &alpha);
                if (m) {
                    solve_begin(s, st, p.me, p.opp, solve_action_of(m), alpha, 64, node_limit);
                } else {
                    s.status = kSolveDone;
                    s.result = OAMD_SOLVE_NONE;
                    s.nodes = 0;
                    s.sp = -1;  // no item: the slot's word is 0
                }
            }
        }
        if (__ballot(have) == 0ULL) break;  // every lane is dry and has stored its last slot
        if (have) {
            for (int k = 0; k < kStepsPerRound; ++k)
                if (s.status == kSolveRunning) solve_step_as<true>(s, st, node_limit);
            if (s.status != kSolveRunning) {
                out_scores[slot] = s.status == kSolveDone ? s.result : OAMD_SOLVE_NONE;
                out_words[slot] = s.sp < 0 ? 0LL : (s.nodes | (int64_t)s.status << kSolveStatusShift);
                have = false;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_solve_split_reduce(const oamd_position* pos, int64_t n, int32_t max_empties,
                                                            const SolvePlan* plan, const int32_t* a_scores,
                                                            const int64_t* a_words, const int32_t* b_scores,
                                                            const int64_t* b_words, int32_t* move_scores,
                                                            int32_t* score, int32_t* best_action, int32_t* flags,
                                                            int64_t* nodes) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const oamd_position p = pos[i];
    solve_reduce_split(p.player, p.player1_discs, p.player2_discs, max_empties, plan + i * kSplitRanks,
                       a_scores + i * kSplitRanks, a_words + i * kSplitRanks, b_scores + i * kSplitSlots,
                       b_words + i * kSplitSlots, move_scores + i * 65, score ? score + i : nullptr,
                       best_action ? best_action + i : nullptr, flags ? flags + i : nullptr,
                       nodes ? nodes + i : nullptr);
}

}  // namespace

void launch_solve_split(const oamd_position* pos, int64_t n, int32_t max_empties, int64_t node_limit,
                        int32_t* move_scores, int32_t* score, int32_t* best_action, int32_t* flags, int64_t* nodes,
                        void* workspace, int32_t workgroups, int32_t compute_units, hipStream_t s) {
    const SplitWorkspace w(workspace, n);
    (void)hipMemsetAsync(w.counters, 0, 256, s);
    hipLaunchKernelGGL(k_solve_plan, dim3((unsigned)((n * kSplitRanks + 255) / 256)), dim3(256), 0, s, pos, n,
                       max_empties, w.plan);
    const int64_t fill = (int64_t)(workgroups > 0 ? workgroups : compute_units * kWavesPerCU);
    for (int phase = 0; phase < 2; ++phase) {
        const int64_t total = n * (phase ? kSplitSlots : kSplitRanks);
        int64_t blocks = (total + kSolveThreads - 1) / kSolveThreads;
        if (blocks > fill) blocks = fill;
        hipLaunchKernelGGL(k_solve_items, dim3((unsigned)blocks), dim3(kSolveThreads), 0, s, w.plan,
                           (unsigned long long)total, phase, phase ? w.a_scores : nullptr, phase ? w.a_words : nullptr, node_limit,
                           phase ? w.b_scores : w.a_scores, phase ? w.b_words : w.a_words,
                           w.counters + 16 * phase);  // 128 bytes apart
    }
    hipLaunchKernelGGL(k_solve_split_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pos, n, max_empties,
                       w.plan, w.a_scores, w.a_words, w.b_scores, w.b_words, move_scores, score, best_action, flags,
                       nodes);
}

void launch_solve(const oamd_position* pos, int64_t n, int32_t max_empties, int64_t node_limit, int32_t* move_scores,
                  int32_t* score, int32_t* best_action, int32_t* flags, int64_t* nodes, void* workspace,
                  int32_t workgroups, int32_t compute_units, hipStream_t s) {
    unsigned long long* counter = static_cast<unsigned long long*>(workspace);
    int64_t* words = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + 256);
    (void)hipMemsetAsync(counter, 0, 256, s);
    int64_t blocks = (n * 65 + kSolveThreads - 1) / kSolveThreads;
    const int64_t fill = (int64_t)(workgroups > 0 ? workgroups : compute_units * kWavesPerCU);
    if (blocks > fill) blocks = fill;
    hipLaunchKernelGGL(k_solve, dim3((unsigned)blocks), dim3(kSolveThreads), 0, s, pos, n, max_empties, node_limit,
                       move_scores, words, counter);
    if (score || best_action || flags || nodes)
        hipLaunchKernelGGL(k_solve_reduce, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pos, n, max_empties,
                           move_scores, words, score, best_action, flags, nodes);
}

}  // namespace oamd
