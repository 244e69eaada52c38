// Packed on-device replay buffer: a ring of POSITIONS, each
// 2H bitboards + the side to move + one 65-entry policy + one value, fed by the
// self-play driver's per-move outputs and expanded to the 8 board symmetries
// when a minibatch is gathered.
//
//   k_replay_add     one wave per game: pack the transform-0 feature planes of
//                    the move with wave ballots and stage the record
//   k_replay_commit  one block: move the games that finished on this move from
//                    the staging area into the ring, in ascending game order
//                    (offsets from a prefix sum; no ordering atomics)
//   k_replay_gather  one wave per sample: position id >> 3 under transform
//                    id & 7 as fp32 planes, policy and value
//
// Exact endgame value targets, for a ring that also keeps one
// `exact` byte per slot:
//
//   k_replay_endgame_list   one block: the live positions in age order whose
//                           exact byte asks for it and that have few empties,
//                           ranked by a prefix sum; the first `budget` of them
//                           become a list of oamd_position rows for the solver
//                           (solver.hip, next in stream order)
//   k_replay_endgame_apply  one wave per list row: the solver's answer becomes
//                           the slot's exact byte, value and (optionally) policy
//
// Every kernel reads only what earlier launches wrote (commit and list keep
// their prefix sums in LDS), so no load depends on a store of the same launch.

#include <hip/hip_runtime.h>

#include "bitboard.h"
#include "replay.h"
#include "solver.h"

namespace oamd {

namespace {

constexpr int kCommitThreads = 1024;
constexpr int kCommitWaves = kCommitThreads / 64;
constexpr int kGatherWaves = 4;

// finished word of the self-play driver (tree_game.h selfplay_move_game)
constexpr int kFinOutcome = 3, kFinNoTargets = 4, kFinOverflow = 8, kFinSolverFlag = 64, kFinFast = 128;

__device__ __forceinline__ void raise_flag(int64_t* counters, int bit) {
    // sticky OR: the result does not depend on the order of the updates
    atomicOr(reinterpret_cast<unsigned long long*>(counters + kReplayFlags), (unsigned long long)bit);
}

// Block g = game g. A played game (actions[g] >= 0) stages one record; a game
// in an error row stages nothing, and if it also finished on this move its
// staged moves are dropped (pending = -1, moves = 0). pending[g] = number of
// staged moves to commit for a game that finished on this move, else -1.
// A move that followed a fast search (playout cap, kFinFast) has no targets by
// design: it stages nothing and raises no flag of its own, and the game's
// other moves and its commit go on as ever.
__global__ __launch_bounds__(64) void k_replay_add(oamd_replay_view V, const int32_t* actions,
                                                   const int32_t* finished, const float* feat, const float* pol) {
    const int g = blockIdx.x;
    const int lane = threadIdx.x;
    const int H2 = 2 * V.history_size;
    const int C = 1 + H2;
    const int fin = finished[g];
    const bool played = actions[g] >= 0 && !(fin & kFinFast);
    int m = V.moves[g];
    int err = 0;
    if (fin & kFinOverflow) err |= OAMD_REPLAY_OVERFLOW;
    if (played && (fin & kFinNoTargets)) err |= OAMD_REPLAY_NO_TARGETS;
    if (played && m >= V.max_moves) err |= OAMD_REPLAY_TOO_LONG;
    // an adjudicated game the solver gave no outcome for: the game is over, its moves have no value target
    if (fin & kFinSolverFlag) err |= OAMD_REPLAY_SOLVER_FLAG;
    if (played && !err) {
        const float* f = feat + (size_t)g * 8 * C * 64;  // transform 0: inverse_transform(sq, 0) == sq
        uint64_t mine = 0;
        for (int c = 0; c < H2; ++c) {
            // ballot bit i = square i; the project's boards keep square i in bit 63 - i
            const uint64_t b = __ballot(f[(size_t)(1 + c) * 64 + lane] != 0.0f);
            if (lane == c) mine = __brevll(b);
        }
        const size_t rec = (size_t)g * V.max_moves + m;
        if (lane < H2) V.stage_boards[rec * H2 + lane] = mine;
        const float* p = pol + (size_t)g * 8 * 65;
        V.stage_policy[rec * 65 + lane] = p[lane];
        if (lane == 0) {
            V.stage_policy[rec * 65 + 64] = p[64];
            V.stage_player[rec] = f[0] != 0.0f ? 1 : 0;  // plane 0 = player - 1
        }
        ++m;
    }
    if (lane == 0) {
        if (err) raise_flag(V.counters, err);
        const bool done = (fin & (kFinOutcome | kFinSolverFlag)) != 0;
        V.pending[g] = done && !err ? m : -1;
        V.moves[g] = done && err ? 0 : m;
    }
}

// Inclusive scan of v over the wave.
__device__ __forceinline__ int wave_scan(int v, int lane) {
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d);
        if (lane >= d) v += t;
    }
    return v;
}

// One block. Pass A: T = positions to commit, from all games. Pass B, per
// chunk of 1024 games: exclusive prefix sum of their counts (offsets in LDS),
// then one wave per committing game copies its records: the j-th committed
// position lands in slot (head + j) % capacity. When more than `capacity`
// positions are committed at once, only the last `capacity` are written, so
// no slot has two writers. Value rule of SampleBuffer: the outcome for black
// (bits 0-1: 1 draw, 2 black won, 3 white won), negated when white is to move.
// exact: the ring's exact bytes, or nullptr for a buffer that keeps none.
__global__ __launch_bounds__(kCommitThreads) void k_replay_commit(oamd_replay_view V, const int32_t* finished,
                                                                  int8_t* exact) {
    __shared__ int s_off[kCommitThreads];
    __shared__ int s_n[kCommitThreads];
    __shared__ float s_outcome[kCommitThreads];
    __shared__ int s_wave[kCommitWaves];
    __shared__ long long s_sum[kCommitWaves];
    __shared__ int s_games[kCommitWaves];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int G = V.num_games;
    const int H2 = 2 * V.history_size;
    const int64_t cap = V.capacity;
    const int64_t head = V.counters[kReplayHead];
    const int64_t size = V.counters[kReplaySize];
    const int64_t games0 = V.counters[kReplayGames];

    // pass A
    long long sum = 0;
    int games = 0;
    for (int g = tid; g < G; g += kCommitThreads) {
        const int n = V.pending[g];
        if (n >= 0) {
            sum += n;
            ++games;
        }
    }
    for (int d = 32; d > 0; d >>= 1) {
        sum += __shfl_xor(sum, d);
        games += __shfl_xor(games, d);
    }
    if (lane == 0) {
        s_sum[wave] = sum;
        s_games[wave] = games;
    }
    __syncthreads();
    int64_t T = 0;
    int n_games = 0;
    for (int w = 0; w < kCommitWaves; ++w) {
        T += s_sum[w];
        n_games += s_games[w];
    }
    if (n_games == 0) return;  // uniform: nothing finished on this move

    // pass B
    int64_t carry = 0;
    for (int base = 0; base < G; base += kCommitThreads) {
        const int g = base + tid;
        const int n = g < G ? V.pending[g] : -1;
        const int v = n > 0 ? n : 0;
        const int incl = wave_scan(v, lane);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int woff = 0, chunk = 0;
        for (int w = 0; w < kCommitWaves; ++w) {
            if (w < wave) woff += s_wave[w];
            chunk += s_wave[w];
        }
        s_off[tid] = n >= 0 ? (int)carry + woff + incl - v : -1;
        s_n[tid] = v;
        const int code = g < G ? finished[g] & kFinOutcome : 0;
        s_outcome[tid] = code == 2 ? 1.0f : (code == 3 ? -1.0f : 0.0f);
        __syncthreads();
        const int chunk_games = min(kCommitThreads, G - base);
        for (int i = wave; i < chunk_games; i += kCommitWaves) {
            const int off = s_off[i];
            if (off < 0) continue;
            const int cnt = s_n[i];
            const float outcome = s_outcome[i];
            for (int k = 0; k < cnt; ++k) {
                const int64_t j = (int64_t)off + k;
                if (T - j > cap) continue;  // overwritten by a later position of this commit
                const size_t slot = (size_t)((head + j) % cap);
                const size_t rec = (size_t)(base + i) * V.max_moves + k;
                if (lane < H2) V.boards[slot * H2 + lane] = V.stage_boards[rec * H2 + lane];
                V.policy[slot * 65 + lane] = V.stage_policy[rec * 65 + lane];
                if (lane == 0) {
                    V.policy[slot * 65 + 64] = V.stage_policy[rec * 65 + 64];
                    const uint8_t white = V.stage_player[rec];
                    V.player[slot] = white;
                    V.value[slot] = outcome * (white ? -1.0f : 1.0f);
                    if (exact) exact[slot] = OAMD_REPLAY_EXACT_UNKNOWN;  // the game's outcome, not examined
                }
            }
        }
        if (g < G && n >= 0) V.moves[g] = 0;
        carry += chunk;
        __syncthreads();  // s_wave / s_off are rewritten by the next chunk
    }
    if (tid == 0) {
        V.counters[kReplayHead] = (head + T) % cap;
        V.counters[kReplaySize] = size + T < cap ? size + T : cap;
        V.counters[kReplayGames] = games0 + n_games;
    }
}

// Wave w of block b = sample b * 4 + w. A plane is one coalesced 256-byte store.
__global__ __launch_bounds__(64 * kGatherWaves) void k_replay_gather(oamd_replay_view V, const int64_t* ids,
                                                                    int64_t n, float* feat, float* pol,
                                                                    float* val) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * kGatherWaves + (threadIdx.x >> 6);
    if (i >= n) return;
    const int H2 = 2 * V.history_size;
    const int C = 1 + H2;
    const int64_t size = V.counters[kReplaySize];
    const int64_t s = ids[i];
    float* fo = feat + (size_t)i * C * 64;
    float* po = pol + (size_t)i * 65;
    if (s < 0 || s >= 8 * size) {
        for (int c = 0; c < C; ++c) fo[c * 64 + lane] = 0.0f;
        po[lane] = 0.0f;
        if (lane == 0) {
            po[64] = 0.0f;
            val[i] = 0.0f;
            raise_flag(V.counters, OAMD_REPLAY_BAD_ID);
        }
        return;
    }
    const int t = (int)(s & 7);
    int64_t slot = V.counters[kReplayHead] - size + (s >> 3);  // oldest live position first
    if (slot < 0) slot += V.capacity;
    const int src = inverse_transform(lane, t);
    const uint64_t mine = lane < H2 ? V.boards[(size_t)slot * H2 + lane] : 0ULL;
    fo[lane] = V.player[slot] ? 1.0f : 0.0f;
    for (int c = 0; c < H2; ++c) {
        const uint64_t b = __shfl(mine, c);
        fo[(1 + c) * 64 + lane] = (float)((b >> (63 - src)) & 1ULL);
    }
    const float* p0 = V.policy + (size_t)slot * 65;
    po[lane] = p0[src];
    if (lane == 0) {
        po[64] = p0[64];
        val[i] = V.value[slot];
    }
}

// The solver's cheapest row: overlapping discs, which solve_classify refuses in
// its first test, before any move generation. Its 65 slots cost one
// classification each and no search; apply skips the row by its slot of -1.
__device__ __forceinline__ void put_pad(oamd_position* p) {
    p->player = 1;
    p->reserved = 0;
    p->player1_discs = p->player2_discs = ~0ULL;
    p->legal_moves = p->next_legal_moves = 0;
}

// One block. Live position i (0 = oldest) sits in slot (head - size + i) mod
// capacity. Per chunk of 1024 positions: candidate bit, inclusive scan over the
// wave, per-wave totals in LDS, a running carry: rank = candidates before i.
// Rows rank < budget get the position and its slot; the scan goes on to the
// end, because rc[2] counts what the budget left behind. Rows taken..budget-1
// are padded. Writes the two lists and rc[2], rc[3] only.
__global__ __launch_bounds__(kCommitThreads) void k_replay_endgame_list(oamd_replay_view V, const int8_t* exact,
                                                                        int64_t* rc, int32_t max_empties,
                                                                        int64_t budget, int32_t retry,
                                                                        oamd_position* pos, int32_t* slots) {
    __shared__ int s_wave[kCommitWaves];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int H2 = 2 * V.history_size;
    const int64_t cap = V.capacity;
    const int64_t head = V.counters[kReplayHead];
    const int64_t size = V.counters[kReplaySize];
    int64_t carry = 0;
    for (int64_t base = 0; base < size; base += kCommitThreads) {
        const int64_t i = base + tid;
        int64_t slot = head - size + i;
        if (slot < 0) slot += cap;
        uint64_t b1 = 0, b2 = 0;
        int cand = 0;
        if (i < size) {
            const int8_t e = exact[slot];
            if (e == OAMD_REPLAY_EXACT_UNKNOWN || (retry && e == OAMD_REPLAY_EXACT_GAVE_UP)) {
                b1 = V.boards[(size_t)slot * H2];  // history step 0: black's discs, white's discs
                b2 = V.boards[(size_t)slot * H2 + 1];
                cand = 64 - popcount64(b1 | b2) <= max_empties;
            }
        }
        const int incl = wave_scan(cand, lane);
        if (lane == 63) s_wave[wave] = incl;
        __syncthreads();
        int woff = 0, chunk = 0;
        for (int w = 0; w < kCommitWaves; ++w) {
            if (w < wave) woff += s_wave[w];
            chunk += s_wave[w];
        }
        const int64_t rank = carry + woff + incl - cand;
        if (cand && rank < budget) {
            oamd_position* p = pos + rank;
            p->player = V.player[slot] + 1;
            p->reserved = 0;
            p->player1_discs = b1;
            p->player2_discs = b2;
            p->legal_moves = p->next_legal_moves = 0;
            slots[rank] = (int32_t)slot;
        }
        carry += chunk;
        __syncthreads();  // s_wave is rewritten by the next chunk
    }
    const int64_t taken = carry < budget ? carry : budget;
    for (int64_t r = taken + tid; r < budget; r += kCommitThreads) {
        put_pad(pos + r);
        slots[r] = -1;
    }
    if (tid == 0) {
        rc[kRelabelLeft] = carry - taken;
        rc[kRelabelTaken] = taken;
    }
}

// Wave w of block b = list row b * 4 + w. Lane l owns policy entry l, lane 0
// also entry 64. A flagged row (node limit, invalid record) marks the slot and
// leaves its value and policy alone. A terminal root (best_action -1) reports
// black minus white: negated for white, and no policy to write.
__global__ __launch_bounds__(64 * kGatherWaves) void k_replay_endgame_apply(
    oamd_replay_view V, int8_t* exact, int64_t* rc, int64_t budget, int32_t policy_mode, const int32_t* slots,
    const int32_t* move_scores, const int32_t* score, const int32_t* best_action, const int32_t* flags) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * kGatherWaves + (threadIdx.x >> 6);
    if (r >= budget) return;
    const int32_t slot = slots[r];
    if (slot < 0) return;  // pad row
    if (flags[r] != 0) {
        if (lane == 0) {
            exact[slot] = OAMD_REPLAY_EXACT_GAVE_UP;
            atomicAdd(reinterpret_cast<unsigned long long*>(rc + kRelabelGaveUp), 1ULL);
        }
        return;
    }
    const int32_t sc = score[r];
    const bool searched = best_action[r] >= 0;
    if (policy_mode == OAMD_REPLAY_POLICY_OPTIMAL && searched) {
        const int32_t* ms = move_scores + r * 65;
        const bool mine = ms[lane] == sc;
        const bool pass = ms[64] == sc;
        const int m = popcount64(__ballot(mine)) + (pass ? 1 : 0);
        const float w = 1.0f / (float)m;  // m >= 1: best_action is one of them
        float* p = V.policy + (size_t)slot * 65;
        p[lane] = mine ? w : 0.0f;
        if (lane == 0) p[64] = pass ? w : 0.0f;
    }
    if (lane == 0) {
        const int32_t s = searched || !V.player[slot] ? sc : -sc;
        exact[slot] = (int8_t)s;
        V.value[slot] = s > 0 ? 1.0f : (s < 0 ? -1.0f : 0.0f);
        atomicAdd(reinterpret_cast<unsigned long long*>(rc + kRelabelSolved), 1ULL);
    }
}

}  // namespace

void launch_replay_add(const oamd_replay_view& V, int8_t* exact, const int32_t* actions, const int32_t* finished,
                       const float* features, const float* policy, hipStream_t s) {
    hipLaunchKernelGGL(k_replay_add, dim3(V.num_games), dim3(64), 0, s, V, actions, finished, features, policy);
    hipLaunchKernelGGL(k_replay_commit, dim3(1), dim3(kCommitThreads), 0, s, V, finished, exact);
}

void launch_replay_relabel(const oamd_replay_view& V, int8_t* exact, int64_t* relabel_counters, int32_t max_empties,
                           int64_t budget, int64_t node_limit, int32_t policy_mode, int32_t retry, void* workspace,
                           int32_t compute_units, hipStream_t s, bool split) {
    const RelabelWorkspace w(workspace, budget, split);
    hipLaunchKernelGGL(k_replay_endgame_list, dim3(1), dim3(kCommitThreads), 0, s, V, exact, relabel_counters,
                       max_empties, budget, retry, w.pos, w.slots);
    (split ? launch_solve_split : launch_solve)(w.pos, budget, max_empties, node_limit, w.move_scores, w.score,
                                                w.best_action, w.flags, nullptr, w.solver, 0, compute_units, s);
    const unsigned blocks = (unsigned)((budget + kGatherWaves - 1) / kGatherWaves);
    hipLaunchKernelGGL(k_replay_endgame_apply, dim3(blocks), dim3(64 * kGatherWaves), 0, s, V, exact,
                       relabel_counters, budget, policy_mode, w.slots, w.move_scores, w.score, w.best_action, w.flags);
}

void launch_replay_gather(const oamd_replay_view& V, const int64_t* ids, int64_t n, float* features,
                          float* policy, float* value, hipStream_t s) {
    const unsigned blocks = (unsigned)((n + kGatherWaves - 1) / kGatherWaves);
    hipLaunchKernelGGL(k_replay_gather, dim3(blocks), dim3(64 * kGatherWaves), 0, s, V, ids, n, features, policy,
                       value);
}

}  // namespace oamd
