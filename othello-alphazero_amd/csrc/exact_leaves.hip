// Exact leaf values on the device (the rule is exact_leaf.h, the
// search's side of it tree_search.h).
//
//   k_solve_leaves     over the rows of a pipeline group (or all rows, the step
//                      API), between a round's tree launch and the next one. A
//                      row whose flag (EngineView::exact) says "pending" ended
//                      at an exact leaf that has no result yet: the kernel
//                      solves the leaf's position and leaves the result in the
//                      flag, where the backup of the next tree launch finds it.
//   k_solve_positions  the same solving path over an array of positions
//                      (oamd_exact_leaf_signs): what the tests compare with
//                      the host rule.
//
// Work item = one (row, root action): a wave holds 4 rows x 16 action ranks (a
// leaf with at most 10 empties has at most 10 moves), lane = 16 * row + rank.
// Every lane runs the solver.h state machine on its item with the window
// [-1, 1] (only the sign is needed); the row's 16 lanes then reduce: the best
// result's sign, the nodes' sum. Items are independent and statically
// assigned, so the result and the node count do not depend on the grid or on
// timing. A wave without a pending row (almost all of them) leaves after one
// load per lane.
//
// The stack: LDS, [level][word][lane] as in solver.hip, but kExactDepth = 10
// levels instead of 16: 10 x 7 words x 64 lanes x 4 bytes = 17,920 bytes per
// wave. That fits in what a ResNet workgroup leaves of a CU's LDS (about 139
// of 160 KB), so a solve wave can be resident on a CU the other pipeline
// group's ResNet launch occupies, like a tree wave; registers cannot hold 70
// words per lane beside the searcher, and scratch would put every push and pop
// on the memory path the ResNet's loads use.

#include <hip/hip_runtime.h>

#include "bitboard.h"
#include "engine.h"
#include "exact_leaf.h"
#include "kernels.h"
#include "solver.h"

namespace oamd {

namespace {

constexpr int kLeafThreads = 64;
constexpr int kLeafRanks = 16;                           // action ranks (lanes) per row
constexpr int kLeafRowsPerWave = kLeafThreads / kLeafRanks;

struct LeafStack {
    uint32_t* base;  // &stack[0][0][lane]
    // a level past the stack cannot be reached below the empties cap; never index past it
    __device__ __forceinline__ void put(int level, int word, uint32_t v) {
        if (level < kExactDepth) base[(level * kSolveFrameWords + word) * kLeafThreads] = v;
    }
    __device__ __forceinline__ uint32_t get(int level, int word) const {
        return level < kExactDepth ? base[(level * kSolveFrameWords + word) * kLeafThreads] : 0u;
    }
};

// The items of one position on the 16 lanes of its row group (`work`: uniform
// over the group). Returns the sign on every lane of the group; *nodes = the
// group's node total. `work` implies exact_solvable (the callers test it).
__device__ __forceinline__ int32_t solve_group(LeafStack& st, bool work, int32_t player, uint64_t p1, uint64_t p2,
                                               int64_t* nodes) {
    const int rank = threadIdx.x & (kLeafRanks - 1);
    int32_t best = -65;
    long long n = 0;
    if (work) {
        const uint64_t me = player == 1 ? p1 : p2, opp = player == 1 ? p2 : p1;
        const int a = exact_root_action(legal_moves(me, opp), rank);
        if (a >= 0) {
            int64_t item_nodes = 0;
            best = exact_solve_item(st, me, opp, a, &item_nodes);
            n = item_nodes;
        }
    }
#pragma unroll
    for (int m = kLeafRanks / 2; m >= 1; m >>= 1) {
        const int32_t ob = __shfl_xor(best, m, kLeafRanks);
        const long long on = __shfl_xor(n, m, kLeafRanks);
        best = ob > best ? ob : best;
        n += on;
    }
    *nodes = n;
    return best == -65 ? 0 : exact_reduce(best);
}

__global__ __launch_bounds__(kLeafThreads) void k_solve_leaves(EngineView E, int row0, int rows) {
    __shared__ uint32_t s_stack[kExactDepth * kSolveFrameWords * kLeafThreads];
    LeafStack st{s_stack + threadIdx.x};
    const int sub = threadIdx.x / kLeafRanks, rank = threadIdx.x & (kLeafRanks - 1);
    const int i = (int)blockIdx.x * kLeafRowsPerWave + sub;
    const bool in = i < rows;
    const int r = row0 + (in ? i : 0);
    const bool pending = in && E.exact[r] == kExactFlagPending;
    if (__ballot(pending) == 0ULL) return;
    int32_t player = 0;
    uint64_t p1 = 0, p2 = 0;
    if (pending) {
        const int node = E.leaf[r];
        if (node >= 0 && (int64_t)node < E.cap) {
            const size_t at = (size_t)(r / E.L) * E.cap + node;
            player = E.link[at].player;
            p1 = E.pos[at].p1;
            p2 = E.pos[at].p2;
        }
    }
    // a pending row whose leaf is no position the solve can take (a bad node
    // index, a corrupted node) stays pending: the backup counts the fault
    // (counter [15], oamd_engine_exact_leaf_faults) and check_health raises
    const bool work = pending && exact_solvable(player, p1, p2);
    int64_t nodes = 0;
    const int32_t s = solve_group(st, work, player, p1, p2, &nodes);
    if (work && rank == 0) {
        E.exact[r] = exact_flag_of_sign(s);
        if (E.counters) {
            atomicAdd(E.counters + 12, 1ULL);
            atomicAdd(E.counters + 14, (unsigned long long)nodes);
        }
    }
}

__global__ __launch_bounds__(kLeafThreads) void k_solve_positions(const oamd_position* pos, int64_t n,
                                                                  int32_t max_empties, int32_t* sign, int64_t* nodes) {
    __shared__ uint32_t s_stack[kExactDepth * kSolveFrameWords * kLeafThreads];
    LeafStack st{s_stack + threadIdx.x};
    const int sub = threadIdx.x / kLeafRanks, rank = threadIdx.x & (kLeafRanks - 1);
    const int64_t i = (int64_t)blockIdx.x * kLeafRowsPerWave + sub;
    bool work = false;
    int32_t player = 0;
    uint64_t p1 = 0, p2 = 0;
    if (i < n) {
        const oamd_position p = pos[i];
        player = p.player;
        p1 = p.player1_discs;
        p2 = p.player2_discs;
        // the rule's own test: a terminal position (whatever `player` says) is no exact leaf
        work = exact_solvable(player, p1, p2) && exact_leaf_position(player, p1, p2, max_empties);
    }
    int64_t total = 0;
    const int32_t s = solve_group(st, work, player, p1, p2, &total);
    if (i < n && rank == 0) {
        sign[i] = work ? s : OAMD_SOLVE_NONE;
        if (nodes) nodes[i] = work ? total : 0;
    }
}

}  // namespace

void launch_solve_leaves(const EngineView& E, int row0, int rows, hipStream_t s) {
    if (rows <= 0 || E.exact_empties <= 0 || row0 < 0 || (int64_t)row0 + rows > (int64_t)E.G * E.L) return;
    hipLaunchKernelGGL(k_solve_leaves, dim3((unsigned)((rows + kLeafRowsPerWave - 1) / kLeafRowsPerWave)),
                       dim3(kLeafThreads), 0, s, E, row0, rows);
}

void launch_solve_positions(const oamd_position* pos, int64_t n, int32_t max_empties, int32_t* sign, int64_t* nodes,
                            hipStream_t s) {
    if (n <= 0) return;
    hipLaunchKernelGGL(k_solve_positions, dim3((unsigned)((n + kLeafRowsPerWave - 1) / kLeafRowsPerWave)),
                       dim3(kLeafThreads), 0, s, pos, n, max_empties, sign, nodes);
}

}  // namespace oamd
