// Baseline opponents on the device (the rule is baseline.h).
//
//   k_baseline       k_solve's shape (solver.hip): work item = one of the n x 65
//                    (position, action) slots; one lane per item, 64-thread
//                    workgroups. Every lane runs the same baseline_step loop on
//                    its own searcher, whose stack is kBaselineLevels x 8 words
//                    of LDS laid out [level][word][lane]. A lane whose item is
//                    done stores the slot's score and its node word and takes
//                    the next slot from a global counter. RANDOM and GREEDY
//                    items are done when they begin. A slot that is no legal
//                    root action (or belongs to a flagged position) stores
//                    OAMD_BASELINE_NONE and costs one classification.
//   k_baseline_pick  one thread per position, after k_baseline in stream order:
//                    score, action (the pick), flags and the node total from
//                    the 65 slots (baseline_reduce); resets the row of a
//                    flagged position.
//
// Every slot is written by exactly one lane and no kernel reads what the same
// launch wrote, so the outputs do not depend on the grid or on which lane got
// which slot.

#include <hip/hip_runtime.h>

#include "baseline.h"
#include "bitboard.h"

namespace oamd {

namespace {

constexpr int kBaselineThreads = 64;
constexpr int kBaselineStepsPerRound = 32;  // baseline_steps between two looks at the item counter
// 10 levels x 8 words x 64 lanes x 4 bytes = 20,480 bytes per workgroup (one
// wave): 8 waves per CU out of 160 KiB of LDS
constexpr int kBaselineWavesPerCU = 8;

struct BaselineLdsStack {
    uint32_t* base;  // &stack[0][0][lane]
    __device__ __forceinline__ void put(int level, int word, uint32_t v) {
        base[(level * kBaselineFrameWords + word) * kBaselineThreads] = v;
    }
    __device__ __forceinline__ uint32_t get(int level, int word) const {
        return base[(level * kBaselineFrameWords + word) * kBaselineThreads];
    }
};

__global__ __launch_bounds__(kBaselineThreads) void k_baseline(const oamd_position* pos, int64_t n, int32_t kind,
                                                               int32_t depth, int64_t node_limit,
                                                               int32_t* move_scores, int64_t* words,
                                                               unsigned long long* counter) {
    __shared__ uint32_t s_stack[kBaselineLevels * kBaselineFrameWords * kBaselineThreads];
    BaselineLdsStack st{s_stack + threadIdx.x};
    const unsigned long long total = (unsigned long long)n * 65ULL;
    BaselineState s;
    s.status = kSolveDone;
    s.nodes = 0;
    s.result = OAMD_BASELINE_NONE;
    s.sp = 0;
    s.me = s.opp = s.moves = 0;
    s.alpha = s.beta = s.best = s.passed = s.depth = 0;
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
                const SolveRoot r = baseline_classify(p.player, p.player1_discs, p.player2_discs);
                if (solve_is_root_action(r, a)) {
                    baseline_begin(s, st, r.me, r.opp, a, kind, depth, node_limit);
                } else {
                    s.status = kSolveDone;
                    s.result = OAMD_BASELINE_NONE;
                    s.nodes = 0;
                    s.sp = -1;  // no item: the slot's word is 0
                }
            }
        }
        if (__ballot(have) == 0ULL) break;  // every lane is dry and has stored its last slot
        if (have) {
            for (int k = 0; k < kBaselineStepsPerRound; ++k)
                if (s.status == kSolveRunning) baseline_step(s, st, node_limit);
            if (s.status != kSolveRunning) {
                move_scores[slot] = s.status == kSolveDone ? s.result : OAMD_BASELINE_NONE;
                words[slot] = s.sp < 0 ? 0LL : (s.nodes | (int64_t)s.status << kSolveStatusShift);
                have = false;
            }
        }
    }
}

__global__ __launch_bounds__(256) void k_baseline_pick(const oamd_position* pos, int64_t n, const int64_t* keys,
                                                       const int64_t* events, int32_t* move_scores,
                                                       const int64_t* words, int32_t* score, int32_t* action,
                                                       int32_t* flags, int64_t* nodes) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const oamd_position p = pos[i];
    baseline_reduce(p.player, p.player1_discs, p.player2_discs, keys != nullptr, keys ? (uint64_t)keys[i] : 0ULL,
                    keys && events ? (uint64_t)events[i] : 0ULL, move_scores + i * 65, words + i * 65,
                    score ? score + i : nullptr, action ? action + i : nullptr, flags ? flags + i : nullptr,
                    nodes ? nodes + i : nullptr);
}

}  // namespace

void launch_baseline(const oamd_position* pos, int64_t n, int32_t kind, int32_t depth, int64_t node_limit,
                     const int64_t* keys, const int64_t* events, int32_t* move_scores, int32_t* score,
                     int32_t* action, int32_t* flags, int64_t* nodes, void* workspace, int32_t workgroups,
                     int32_t compute_units, hipStream_t s) {
    unsigned long long* counter = static_cast<unsigned long long*>(workspace);
    int64_t* words = reinterpret_cast<int64_t*>(static_cast<char*>(workspace) + 256);
    (void)hipMemsetAsync(counter, 0, 256, s);
    int64_t blocks = (n * 65 + kBaselineThreads - 1) / kBaselineThreads;
    const int64_t fill = (int64_t)(workgroups > 0 ? workgroups : compute_units * kBaselineWavesPerCU);
    if (blocks > fill) blocks = fill;
    hipLaunchKernelGGL(k_baseline, dim3((unsigned)blocks), dim3(kBaselineThreads), 0, s, pos, n, kind, depth,
                       node_limit, move_scores, words, counter);
    hipLaunchKernelGGL(k_baseline_pick, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pos, n, keys, events,
                       move_scores, words, score, action, flags, nodes);
}

}  // namespace oamd
