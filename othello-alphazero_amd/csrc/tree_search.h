// The search of one game by one wave: selection with virtual loss, expansion,
// backup and the round schedule (search_round), with the per-wave state and
// work counters they carry. Everything here is __forceinline__ into the round
// kernels of tree.hip (k_tree, k_tree_wide, k_tree_free); tree_game.h and the
// kernels of selfplay.hip and arena.hip use the small helpers. See tree.hip
// for the mapping of the reference's search onto a wave and for the
// floating-point rules.
#pragma once

#include <hip/hip_runtime.h>

#include "bitboard.h"
#include "engine.h"
#include "exact_leaf.h"
#include "forced.h"
#include "rng.h"
#include "wave.h"

#ifndef OAMD_CHAIN_PRIO
#define OAMD_CHAIN_PRIO 2
#endif

// Phase stamps of the diagnostic build (-DOAMD_TREE_STAMPS): tree.hip, the unit
// that holds k_tree, defines them before it includes this header; in every
// other unit (and in the normal build) they expand to nothing.
#ifndef TS_T
#define TS_T(v) ((void)0)
#define TS_ADD(i, x) ((void)0)
#endif

namespace oamd {

// exploration_rate of search_thread.cpp:198-203, tabulated on the host with
// the host's logf so that it is bit-identical to the CPU reference.
__device__ __forceinline__ float explore_rate(const EngineView& E, int n) {
    if (n >= 0 && n < kExploreTab) return E.explore_tab[n];
    return logf(((float)(1 + n) + E.c_base) / E.c_base) + E.c_init;
}

// sqrt of the children's visit sum: IEEE correctly rounded on the device as on
// the host (HIP's default correctly-rounded fp32 sqrt, -fno-fast-math)
__device__ __forceinline__ float sqrt_count(const EngineView&, int n) { return sqrtf((float)n); }

// Square of the j-th legal action of a position (legal_actions order,
// position.h:308-326), computed by lane = square.
__device__ __forceinline__ int action_of_child(uint64_t legal, int j) {
    if (legal == 0) return 64;
    const int s = lane_id();
    const bool set = (legal >> (63 - s)) & 1ULL;
    const uint64_t before = s == 0 ? 0ULL : (legal & (~0ULL << (64 - s)));
    const bool hit = set && popcount64(before) == j;
    const uint64_t b = __ballot(hit);
    return b ? (__ffsll((unsigned long long)b) - 1) : 64;
}

// Child index of an action in legal_actions order (mcts.cpp:147-153).
__device__ __forceinline__ int child_index_of(uint64_t legal, int n_children, int action) {
    if (action == 0 || n_children <= 1 || action == 64) return 0;
    return popcount64(legal & (~0ULL << (64 - action)));
}

// Packed features of row r (position_iterator.h:24-71, transformation.h:83-116):
// a meta word (leaf player, symmetry, valid; 0 for a terminal leaf: no NN row)
// and the H positions leaf = path[d], its ancestors, then the game history.
// The meta word is written at the leaf; the positions are gathered for up to
// 64 / H leaves at once (flush_ancestors), so the selection loop does not wait
// for a position load per leaf.
__device__ __forceinline__ void write_feature_meta(const EngineView& E, int r, int leaf_player, int t,
                                                   bool valid) {
    if (lane_id() != 0) return;
    uint64_t* row = E.feat + (size_t)r * E.FW;
    row[0] = valid ? ((uint64_t)((leaf_player - 1) & 1) | ((uint64_t)t << 8) | (1ULL << 16)) : 0ULL;
    row[1] = 0;
}

// Node of position h = lane (< H) of a leaf at depth d: path[d - h] for h <= d,
// else hist[h - d - 1]; -1 past the history (a zero plane pair)
__device__ __forceinline__ int feature_ancestor(int d, int p0, int p1, int hist_node, int hist_n) {
    const int lane = lane_id();
    const int idx = d - lane;
    const int from_p0 = __shfl(p0, idx & 63);
    const int from_p1 = __shfl(p1, idx & 63);
    const int hj = lane - d - 1;
    const int from_h = __shfl(hist_node, hj & 63);
    int anc = -1;
    if (idx >= 0) anc = idx < 64 ? from_p0 : from_p1;
    else if (hj < hist_n) anc = from_h;
    return anc;
}

// Position planes of rows r0 .. r0 + n - 1: lane j = (leaf j / H, position
// j % H) holds its node in anc (from feature_ancestor); bit k of `valid` =
// row r0 + k has an NN row. One load round trip for all of them.
__device__ __forceinline__ void flush_ancestors(const EngineView& E, size_t base, int r0, int n, int anc,
                                                uint64_t valid) {
    const int lane = lane_id();
    const int k = lane / E.H, h = lane - k * E.H;
    if (k >= n || !((valid >> k) & 1ULL)) return;
    uint64_t a1 = 0, a2 = 0;
    if (anc >= 0) {
        const NodePos* np = E.pos + base + anc;
        a1 = np->p1;
        a2 = np->p2;
    }
    uint64_t* row = E.feat + (size_t)(r0 + k) * E.FW;
    row[2 + 2 * h] = a1;
    row[3 + 2 * h] = a2;
}

// Append the NN rows of non-terminal leaves among rows c0 + j (bit j of
// `valid`) to the group's evaluation list: one atomic per chunk of <= 64 rows
// reserves the slots, lane j writes row c0 + j. The ResNet launch reads the
// list, so terminal leaves cost it nothing (the reference builds no NN row for
// them, search_thread.cpp:88-90); the list order does not matter, every row's
// evaluation is independent of its place in a launch.
__device__ __forceinline__ void append_rows(const EngineView& E, int* cnt, int list_base, int c0, uint64_t valid) {
    const int n = popcount64(valid);
    if (n == 0) return;
    int slot = 0;
    if (lane_id() == 0) slot = atomicAdd(cnt, n);
    slot = readlane_i(slot, 0);
    const int lane = lane_id();
    if ((valid >> lane) & 1ULL)
        E.rowlist[list_base + slot + popcount64(valid & ((1ULL << lane) - 1ULL))] = c0 + lane;
}

// Per-wave work counters of one k_tree launch.
struct RoundAcc {
    unsigned long long sims = 0, evals = 0, depth_sum = 0;
    unsigned long long scan_sum = 0;  // children scanned over every descent level
    int depth_max = 0;
    unsigned expansions = 0;          // leaves expanded (children = the node count's growth)
    unsigned exact_pending = 0;       // exact leaves selected while pending
    unsigned exact_hits = 0;          // ... and while solved
};

// The search state a wave carries across a round (search_round): read from
// the game's GameState when the round starts, kept in registers, and written
// back by lane 0 when it ends. load() leaves the work counters alone: one
// launch of k_tree_free loads twice (a move lies between two searches).
struct WaveSearch {
    int cut_at;      // the thread whose chain this round stopped, -1: none
    bool over;       // a chain went past the budget with every cut used
    int cuts;        // chains split so far in this search
    bool overflow;   // an expansion found the pool full
    int count;       // nodes allocated in the game's pool
    RoundAcc acc;
    int hist_node;   // lane < 16: entry `lane` of the root's history (-1 for the other lanes)
    int hist_n;      // ... and its valid entries
    uint64_t event;  // the game's next random event

    // resume: the round continues a search whose chains may have been cut
    __device__ __forceinline__ void load(const GameState* gs) {
        event = gs->event;
        hist_n = gs->hist_n;
        hist_node = lane_id() < 16 ? gs->hist[lane_id()] : -1;
        count = gs->count;
        overflow = false;
        cuts = 0;
        over = false;
        cut_at = -1;
    }

    // lane 0. The flag is set atomically like select_range's kDepthCap: a plain
    // read-modify-write of flags read at kernel start could drop that bit
    __device__ __forceinline__ void publish(GameState* gs) const {
        gs->event = event;
        gs->count = count;
        if (overflow) atomicOr(&gs->flags, (int)kOverflow);
    }
};

// ---------------------------------------------------------------------------
// Selection: descents i in [i0, i1) with virtual loss (search_thread.cpp:59-100).
// cnt != nullptr: the non-terminal leaves' rows go to the evaluation list.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void select_range(const EngineView& E, int g, GameState* gs, size_t base,
                                             int i0, int i1, uint64_t& event, int hist_node,
                                             int hist_n, int* cnt, int list_base, bool fast, RoundAcc& acc) {
    const int lane = lane_id();
    const int root = gs->root;
    const uint64_t key = gs->key;
    // the root's link is fixed during one thread's selections (expansions happen
    // in that thread's backup, before this range); its N grows by one per
    // selected leaf (search_thread.cpp:78)
    const NodeLink root_link = load_link(E.link + base + root);
    int root_n = E.stat[base + root].n;
    uint64_t valid_rows = 0;  // bit i - c0: row i is an NN row (chunks of 64 rows from i0)
    int c0 = i0;
    // Root noise vectors drawn ahead: lane s * nz_nc + j holds the noise of
    // child j at event nz_base + s, for as many events as 64 lanes hold (a
    // selection followed by a non-terminal leaf's symmetry draw uses two, one
    // ending in a terminal leaf one); a selection past them draws again.
    // The noise is a function of (game key, event, child) only, so these are
    // the draws of the selections themselves.
    float nz_cache = 0.0f;
    uint64_t nz_base = ~0ULL;
    int nz_nc = 0;
    // feature positions of leaves f0 .. (up to 64 / H of them), flushed together
    const int per_flush = 64 / E.H;
    int f0 = i0, anc_rec = -1;
    uint64_t fvalid = 0;

    for (int i = i0; i < i1; ++i) {
        const int r = g * E.L + i;
        int node = root;
        int d = 0;
        int p0 = lane == 0 ? root : -1;  // path slot `lane`
        int p1 = -1;                     // path slot 64 + lane
        NodeLink lk = root_link;
        // exploration rate of `node` (from its N); for a chosen child it was
        // fetched by the child's lane at the previous level
        float er = explore_rate(E, root_n);
        TS_T(ts0);
        // One dependent memory round trip per level: the stats AND links of all
        // children are loaded together; the chosen child's link, N and
        // exploration rate come from its lane (readlane), not from a second load.
        while (!(lk.player == 0 || lk.n_children == 0) && d < kMaxDepth - 1) {
            const int nc = lk.n_children, fc = lk.first_child;
            acc.scan_sum += (unsigned long long)nc;  // children whose stats this level reads
            int4 cs4 = make_int4(0, 0, 0, 0), cl4 = make_int4(0, 0, 0, 0);
            if (lane < nc) {
                cs4 = *reinterpret_cast<const int4*>(E.stat + base + fc + lane);
                cl4 = *reinterpret_cast<const int4*>(E.link + base + fc + lane);
            }
            // every child lane fetches its own exploration rate now, so the
            // chosen child's is ready for the next level (no dependent table read)
            const float er_child = lane < nc ? explore_rate(E, cs4.x) : 0.0f;
            int best = 0;
            if (nc > 1) {
                const NodeStat cs{cs4.x, __int_as_float(cs4.y), __int_as_float(cs4.z), __int_as_float(cs4.w)};
                const int total = wave_scan_first_n(lane < nc ? cs.n : 0, 0, [](int a, int b) { return a + b; }, nc);
                const float mult = er * sqrt_count(E, total);
                float prob = cs.p;
                if (node == root && !fast && E.eps > 0.0f) {  // a fast search draws no root noise
                    // fresh Dirichlet noise on every root selection (search_thread.cpp:230-249)
                    TS_T(tn0);
                    const int slots = 64 / nc;
                    const uint64_t off = event - nz_base;
                    if (nz_nc != nc || off >= (uint64_t)slots) {
                        TS_T(tr0);
                        nz_base = event;
                        nz_nc = nc;
                        const int sl = lane / nc, j = lane - sl * nc;
                        nz_cache = sl < slots ? gamma_draw(stream_key(key, event + (uint64_t)sl, (uint32_t)j), E.alpha)
                                              : 0.0f;
                        TS_T(tr1);
                        TS_ADD(kTsRefill, tr1 - tr0);
                    }
                    float noise = __shfl(nz_cache, ((int)(event - nz_base) * nc + lane) & 63);
                    if (lane >= nc) noise = 0.0f;
                    event += 1;
                    float nsum = 0.0f;
                    for (int j = 0; j < nc; ++j) nsum += readlane_f(noise, j);
                    if (nsum == 0.0f) nsum = 1.0f;
                    const float pm = 1.0f - E.eps;
                    const float nm = E.eps / nsum;
                    prob = cs.p * pm + noise * nm;
                    TS_T(tn1);
                    TS_ADD(kTsNoise, tn1 - tn0);
                }
                float ucb = cs.q + mult * prob / (1.0f + (float)cs.n);
                // forced playouts (forced.h): at the root of a full
                // search a tried child below its visit floor goes first (the
                // lowest such child: the first-max argmax). Wave-uniform branch,
                // E.forced_k read here from the kernel argument.
                if (node == root && !fast && E.forced_k > 0.0f && forced_playout(cs.n, prob, total, E.forced_k))
                    ucb = __builtin_inff();
                if (lane >= nc) ucb = -__builtin_inff();
                best = wave_argmax_first_n(ucb, nc);
            }  // a single child is taken without scoring (search_thread.cpp:194-196)
            const int child = fc + best;
            const int4 clk4 = make_int4(readlane_i(cl4.x, best), readlane_i(cl4.y, best),
                                        readlane_i(cl4.z, best), readlane_i(cl4.w, best));
            const float er_next = readlane_f(er_child, best);
            ++d;
            if (lane == (d & 63)) {
                if (d < 64) p0 = child;
                else p1 = child;
            }
            node = child;
            lk = NodeLink{clk4.x, clk4.y, clk4.z, clk4.w};
            er = er_next;
        }
        TS_T(ts1);
        TS_ADD(kTsDescent, ts1 - ts0);
        TS_ADD(kTsLevels, d);
        TS_ADD(kTsLeaves, 1);
        TS_ADD(kTsTerminal, lk.player == 0 ? 1 : 0);
        if (d == kMaxDepth - 1 && lk.player != 0 && lk.n_children != 0 && lane == 0)
            atomicOr(&gs->flags, (int)kDepthCap);
        // virtual loss on the path excluding the root (search_thread.cpp:69-76)
        if (lane >= 1 && lane <= d) {
            NodeStat s = load_stat(E.stat + base + p0);
            s.n += 1;
            s.w -= 1.0f;
            s.q = s.w / (float)s.n;
            store_stat(E.stat + base + p0, s);
        }
        if (64 + lane <= d) {
            NodeStat s = load_stat(E.stat + base + p1);
            s.n += 1;
            s.w -= 1.0f;
            s.q = s.w / (float)s.n;
            store_stat(E.stat + base + p1, s);
        }
        root_n += 1;
        if (lane == 0) E.stat[base + root].n = root_n;  // search_thread.cpp:78
        // record the path for the backup
        int* gp = E.path + (size_t)r * kMaxDepth;
        if (lane <= d) gp[lane] = p0;
        if (64 + lane <= d) gp[64 + lane] = p1;
        // exact leaves (exact_leaf.h): a childless node carrying a
        // mark is a terminal-like leaf: no NN row, meta word 0, no symmetry draw,
        // not an evaluation. Its row flag tells the solve kernel (pending) and
        // the backup (the result) what to do. Wave-uniform (lk is). With the
        // setting off no mark exists, so the test needs no look at
        // E.exact_empties, and it is written without a branch on purpose: a
        // loop-invariant branch here makes the compiler clone the selection
        // loop (152 instead of 48 bytes of scratch per lane in k_tree).
        int xflag = kExactFlagNone;
        if (lk.player != 0 && lk.n_children == 0 && exact_mark(lk.first_child)) xflag = exact_flag_of_mark(lk.first_child);
        acc.exact_pending += xflag == kExactFlagPending ? 1 : 0;
        acc.exact_hits += xflag > kExactFlagPending ? 1 : 0;
        const bool valid = lk.player != 0 && xflag == kExactFlagNone;
        int t = 0;
        if (valid) {
            t = draw_transform(key, event);  // search_thread.cpp:92
            event += 1;
        }
        if (lane == 0) {
            E.leaf[r] = node;
            E.depth[r] = d;
            E.trans[r] = t;
            if (E.exact_empties > 0) E.exact[r] = xflag;
        }
        write_feature_meta(E, r, lk.player, t, valid);
        {
            const int anc = feature_ancestor(d, p0, p1, hist_node, hist_n);
            const int k = i - f0;
            const int moved = __shfl(anc, (lane - k * E.H) & 63);
            if (lane >= k * E.H && lane < (k + 1) * E.H) anc_rec = moved;
            fvalid |= (uint64_t)(valid ? 1 : 0) << k;
            if (k == per_flush - 1 || i == i1 - 1) {
                flush_ancestors(E, base, g * E.L + f0, k + 1, anc_rec, fvalid);
                f0 = i + 1;
                fvalid = 0;
            }
        }
        acc.sims += 1;
        acc.evals += valid ? 1 : 0;
        acc.depth_sum += (unsigned long long)d;
        acc.depth_max = d > acc.depth_max ? d : acc.depth_max;
        if (cnt) {
            valid_rows |= (uint64_t)(valid ? 1 : 0) << (i - c0);
            if (i - c0 == 63 || i == i1 - 1) {
                append_rows(E, cnt, list_base, g * E.L + c0, valid_rows);
                valid_rows = 0;
                c0 = i + 1;
            }
        }
        wave_order();  // the next descent reads these statistics
        TS_T(ts2);
        TS_ADD(kTsPost, ts2 - ts1);
    }
}

// ---------------------------------------------------------------------------
// Expansion: the children of one position, four lanes per child.
// The reference computes each child with apply_action (position.h:328-363):
// flips in 8 directions, then the child's legal moves (8 directions), and the
// other side's when those are empty. Lane 4k + q works on child k and on the
// two opposite directions of magnitude {1, 7, 8, 9}[q] (edge masks as
// position.h:155-172); an OR over the child's 4 lanes completes each 8-way
// union. Exactly the same bit operations as bitboard.h's apply_action, 4x
// fewer instructions per expansion than one child per lane (16 children per
// pass; positions with more take a second pass).
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint64_t or_quad(uint64_t x) {
    // quad_perm [1,0,3,2], then [2,3,0,1]: every lane of a quad holds the quad's OR
    uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
    lo |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, 0xB1, 0xF, 0xF, false);
    hi |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, 0xB1, 0xF, 0xF, false);
    lo |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, 0x4E, 0xF, 0xF, false);
    hi |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)hi, 0x4E, 0xF, 0xF, false);
    return (uint64_t)lo | ((uint64_t)hi << 32);
}

// opponent run from seed along << mag and >> mag (run_dir's 6 steps each)
__device__ __forceinline__ void runs_pair(uint64_t seed, uint64_t om, int mag, uint64_t& l, uint64_t& r) {
    l = om & (seed << mag);
    r = om & (seed >> mag);
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        l |= om & (l << mag);
        r |= om & (r >> mag);
    }
}

// The k-th set square (ascending square index = descending bit) of a mask
__device__ __forceinline__ int kth_square(uint64_t mask, int k) {
    // bit-reverse so that square s is bit s, then select the k-th set bit from
    // the bottom by halving
    const uint32_t rlo = __builtin_bitreverse32((uint32_t)(mask >> 32));  // squares 0..31
    const uint32_t rhi = __builtin_bitreverse32((uint32_t)mask);          // squares 32..63
    int pos = 0;
    uint32_t x = rlo;
    int c = __builtin_popcount(rlo);
    if (k >= c) {
        k -= c;
        pos = 32;
        x = rhi;
    }
#pragma unroll
    for (int w = 16; w >= 1; w >>= 1) {
        c = __builtin_popcount(x & ((1u << w) - 1u));
        if (k >= c) {
            k -= c;
            pos += w;
            x >>= w;
        }
    }
    return pos;
}

// Expand position P (not terminal, legal != 0) into children fc .. fc+nc-1 in
// legal_actions order (position.h:308-326), priors policy[transform(a, t)].
// pol_l: entry `lane` of the leaf's policy row (prefetched by backup_range)
__device__ __forceinline__ void expand_quads(const EngineView& E, size_t base, int leaf, const Pos& P, int fc,
                                             int nc, int t, float pol_l, int child_mark) {
    const int lane = lane_id();
    const int q = lane & 3;
    const int mag = q == 0 ? 1 : (q == 1 ? 7 : (q == 2 ? 8 : 9));
    const uint64_t dmask = q == 0 ? kNoLR : (q == 2 ? kNoTB : kNoEdge);
    const bool black = P.player == 1;
    const uint64_t me = black ? P.p1 : P.p2;
    const uint64_t opp = black ? P.p2 : P.p1;
    for (int k0 = 0; k0 < nc; k0 += 16) {
        const int k = k0 + (lane >> 2);
        const int sq = kth_square(P.legal, k < nc ? k : 0);
        const uint64_t move = 1ULL << (63 - sq);
        // flips (position.h:231-262): runs capped by an own disc
        uint64_t l, r;
        runs_pair(move, opp & dmask, mag, l, r);
        uint64_t f = (((l << mag) & me) ? l : 0ULL) | (((r >> mag) & me) ? r : 0ULL);
        f = or_quad(f);
        const uint64_t mine = me | move | f, theirs = opp & ~f;  // the mover's / the opponent's discs
        // the child's side to move is the opponent (position.h:349-362)
        runs_pair(theirs, mine & dmask, mag, l, r);
        uint64_t lg = or_quad((l << mag) | (r >> mag)) & ~(mine | theirs);
        uint64_t nx = 0;
        int player = 3 - P.player;
        if (lg == 0) {  // the child's mover must pass: the other side's moves
            runs_pair(mine, theirs & dmask, mag, l, r);
            nx = or_quad((l << mag) | (r >> mag)) & ~(mine | theirs);
            if (nx == 0) player = 0;
        }
        // the prior of a move (< 64) from the lane holding its transformed entry
        const float prior = __shfl(pol_l, transform_action(sq, t));
        if (q == 0 && k < nc) {
            Pos c;
            c.player = player;
            c.pad_ = 0;
            c.p1 = black ? mine : theirs;
            c.p2 = black ? theirs : mine;
            c.legal = lg;
            c.next_legal = nx;
            const int id = fc + k;
            // a child with few empties is an exact leaf (pending): never expanded
            store_link(E.link + base + id, NodeLink{c.player != 0 ? child_mark : kMarkPlain, 0, leaf, c.player});
            store_stat(E.stat + base + id, NodeStat{0, 0.0f, 0.0f, prior});
            store_pos(E.pos + base + id, c);
        }
    }
}

// ---------------------------------------------------------------------------
// Expansion + backup of leaves [i0, i1) (search_thread.cpp:116-127, 130-190).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void backup_range(const EngineView& E, int g, size_t base, int i0, int i1,
                                             int& count, bool& overflow, unsigned& expansions) {
    const int lane = lane_id();
    TS_T(tb0);
    TS_ADD(kTsBackedUp, i1 - i0);
    // Leaves are processed in order (their backups share path nodes), but
    // everything a leaf needs except the path statistics is independent of
    // the earlier leaves: it is fetched for up to 64 leaves at once, one lane
    // per leaf. A chunk's prefetch starts after every earlier store of the
    // wave has completed, so links are current except for duplicates of a
    // leaf expanded earlier in the same chunk: those are found by a ballot
    // over the chunk's lanes (duplicates never expand again, search_thread.cpp:
    // 133-135, and use only the immutable player / parent of the link).
    for (int c0 = i0; c0 < i1; c0 += 64) {
        const int cend = i1 - c0 < 64 ? i1 - c0 : 64;
        const int cl = lane < cend ? lane : 0;
        const int rl = g * E.L + c0 + cl;
        const int leaf_v = E.leaf[rl];
        const int d_v = E.depth[rl];
        const int t_v = E.trans[rl];
        const float val_v = E.value[rl];
        const int ex_v = E.exact_empties > 0 ? E.exact[rl] : kExactFlagNone;  // exact leaves: the row's flag
        const int4 lk_v = *reinterpret_cast<const int4*>(E.link + base + leaf_v);
        const NodePos pos_v = E.pos[base + leaf_v];
        bool expanded_here = false;  // lane j: leaf j of this chunk expanded its node
        // path and policy row (entry `lane`; the pass's entry 64 is read when used) of the chunk's first
        // leaf; each leaf prefetches the next one's (the ResNet launch that
        // wrote the rows has completed before this kernel started)
        int gp0 = 0, gp1 = 0;
        float pol_l = 0.0f;
        {
            const int* gp = E.path + (size_t)(g * E.L + c0) * kMaxDepth;
            const int d0 = readlane_i(d_v, 0);
            if (lane >= 1 && lane <= d0) gp0 = gp[lane];
            if (64 + lane <= d0) gp1 = gp[64 + lane];
            const float* pr = E.policy + (size_t)(g * E.L + c0) * 65;
            pol_l = pr[lane];
        }
        for (int j = 0; j < cend; ++j) {
            const int r = g * E.L + c0 + j;
            const int leaf = readlane_i(leaf_v, j);
            const int d = readlane_i(d_v, j);
            const int t = readlane_i(t_v, j);
            const NodeLink lk{readlane_i(lk_v.x, j), readlane_i(lk_v.y, j), readlane_i(lk_v.z, j),
                              readlane_i(lk_v.w, j)};
            const int path0 = gp0, path1 = gp1;
            const float polj = pol_l;
            if (j + 1 < cend) {  // next leaf's path and policy row, behind this leaf's work
                const int* gp = E.path + (size_t)(r + 1) * kMaxDepth;
                const int dn = readlane_i(d_v, j + 1);
                if (lane >= 1 && lane <= dn) gp0 = gp[lane];
                if (64 + lane <= dn) gp1 = gp[64 + lane];
                const float* pr = E.policy + (size_t)(r + 1) * 65;
                pol_l = pr[lane];
            }
            const bool already = __ballot(expanded_here && leaf_v == leaf) != 0;
            // an exact leaf is never expanded: the solve kernel left its result
            // in the row's flag. A flag still pending means the kernel did not
            // run or could not take the row: a fault, counted in counter [15]
            // (check_health raises); the leaf stays pending and backs up a draw
            const int ex = readlane_i(ex_v, j);
            TS_T(te0);
            if (ex != kExactFlagNone) {
                if (ex == kExactFlagPending && lane == 0 && E.counters) atomicAdd(E.counters + 15, 1ULL);
                if (lk.first_child == kMarkPending && ex != kExactFlagPending && lane == 0)
                    store_link(E.link + base + leaf, NodeLink{exact_mark_of_flag(ex), 0, lk.parent, lk.player});
            } else if (lk.player != 0 && lk.n_children == 0 && !already) {
                Pos P;
                P.player = lk.player;
                P.pad_ = 0;
                P.p1 = readlane_u64(pos_v.p1, j);
                P.p2 = readlane_u64(pos_v.p2, j);
                P.legal = readlane_u64(pos_v.legal, j);
                P.next_legal = readlane_u64(pos_v.next_legal, j);
                const int nc = P.legal ? popcount64(P.legal) : 1;
                if ((int64_t)count + nc > E.cap) {
                    overflow = true;  // leaf stays a leaf; value still backed up
                } else {
                    const int fc = count;
                    count += nc;
                    ++expansions;
                    // exact leaves (exact_leaf.h): every child of a move has one
                    // empty fewer than P, the child of a pass as many: one
                    // wave-uniform test per expansion gives the children's mark
                    const int child_mark =
                        E.exact_empties > 0 && popcount64(~(P.p1 | P.p2)) - (P.legal ? 1 : 0) <= E.exact_empties
                            ? kMarkPending
                            : kMarkPlain;
                    if (P.legal) {
                        expand_quads(E, base, leaf, P, fc, nc, t, polj, child_mark);
                    } else if (lane == 0) {  // the pass: one child (position.h:382-386)
                        const Pos c = apply_action(P, 64);
                        store_link(E.link + base + fc,
                                   NodeLink{c.player != 0 ? child_mark : kMarkPlain, 0, leaf, c.player});
                        store_stat(E.stat + base + fc, NodeStat{0, 0.0f, 0.0f, E.policy[(size_t)r * 65 + 64]});
                        store_pos(E.pos + base + fc, c);
                    }
                    if (lane == 0) store_link(E.link + base + leaf, NodeLink{fc, nc, lk.parent, lk.player});
                    if (lane == j) expanded_here = true;
                }
            }
            TS_T(te1);
            TS_ADD(kTsExpand, te1 - te0);
            if (d > 0) {
                float v;
                if (ex != kExactFlagNone) {
                    v = exact_parent_value(ex == kExactFlagPending ? 0 : exact_sign_of_flag(ex));
                } else if (lk.player != 0) {
                    v = -readlane_f(val_v, j);
                } else {
                    // terminal: score from the perspective of the parent's player
                    const NodeLink pl = load_link(E.link + base + lk.parent);
                    const uint64_t lp1 = readlane_u64(pos_v.p1, j);
                    const uint64_t lp2 = readlane_u64(pos_v.p2, j);
                    const uint64_t mine = pl.player == 1 ? lp1 : lp2;
                    const uint64_t theirs = pl.player == 1 ? lp2 : lp1;
                    const int a = popcount64(mine), b = popcount64(theirs);
                    v = a > b ? 1.0f : (a < b ? -1.0f : 0.0f);
                }
                // node at depth k receives v * (-1)^(d-k)  (sign flips walking up)
                if (lane >= 1 && lane <= d) {
                    const float vk = ((d - lane) & 1) ? -v : v;
                    NodeStat s = load_stat(E.stat + base + path0);
                    s.w += 1.0f + vk;
                    s.q = s.w / (float)s.n;
                    store_stat(E.stat + base + path0, s);
                }
                if (64 + lane <= d) {
                    const int k = 64 + lane;
                    const float vk = ((d - k) & 1) ? -v : v;
                    NodeStat s = load_stat(E.stat + base + path1);
                    s.w += 1.0f + vk;
                    s.q = s.w / (float)s.n;
                    store_stat(E.stat + base + path1, s);
                }
            }
            wave_order();  // the next leaf's backup reads these statistics
            TS_T(tw1);
            TS_ADD(kTsPathW, tw1 - te1);
        }
    }
    TS_T(tb1);
    TS_ADD(kTsBackup, tb1 - tb0);
}

// Playout cap randomization: the batches per virtual thread
// and the root noise weight of the search of game gs at its current root.
// Off (E.fast_steps == 0): the engine's. On: a search that playout_cap_full
// calls fast runs E.fast_steps batches and draws no root noise. Both are
// wave-uniform (one readfirstlane of the draw), recomputed every round from
// the game's key and ply, which do not change during a search.
__device__ __forceinline__ bool search_is_fast(const EngineView& E, const GameState* gs) {
    if (E.fast_steps <= 0) return false;
    const bool full = playout_cap_full(gs->key, gs->ply, E.full_probability);
    return __builtin_amdgcn_readfirstlane(full ? 0 : 1) != 0;
}
__device__ __forceinline__ int search_steps_of(const EngineView& E, bool fast) { return fast ? E.fast_steps : E.steps; }

// ---------------------------------------------------------------------------
// One round of the search schedule for every game (one wave per game).
//
// The reference runs T threads, each looping lock{select B leaves} -> NN ->
// lock{expand + backup B leaves}, with the calling thread serving NN requests
// FIFO (search_thread.cpp:47-128, mcts.h:220-256). The interleaving it
// produces (measured on the compiled reference, DESIGN.md "Search semantics")
// is a pipelined round-robin: after every thread selected its first batch,
// thread t backs up batch k and immediately selects batch k+1, then thread
// t+1 does the same. Round k of this kernel is therefore, for t = 0..T-1:
//     backup(thread t, batch k-1)   [do_backup]
//     select(thread t, batch k)     [do_select]
// Thread t's rows are consumed by its backup before its selection rewrites
// them. With T = 1 this is exactly the reference's sequential loop. Calling
// with do_backup only after every select gives the lock-step order instead.
// ---------------------------------------------------------------------------
// Capped at 96 VGPRs (amdgpu_num_vgpr counts the unified VGPR+AGPR file in
// units of 2 on gfx950) so that a tree wave fits beside the two 208-VGPR
// k_resnet_w8 waves of every SIMD (512 VGPRs): one pipeline group's tree round
// runs on the CUs that the other group's ResNet launch occupies. The cap costs
// 60 bytes per lane of spills (72 in k_tree_free; DESIGN.md §17 has the
// remarks of this tree and of the one before the playout cap); launches of at most
// kWideTreeGames games run k_tree_wide, the same round uncapped (114 VGPRs).
// Evaluation list (cnt_add != nullptr, the native search): the rows of
// non-terminal leaves this round selects are appended to E.rowlist[g0 * L ..]
// behind the counter *cnt_add; *cnt_reset (the counter of the next round,
// which no launch still reads) is zeroed by the group's first wave.
// Chain splitting (budget > 0, the native search): a thread whose batches
// come back all terminal selects again at once (the reference's order), and
// such a chain can run to the end of the thread's search inside one round,
// holding its pipeline group's NN launch. After `budget` re-selections in a
// round the game stops (at most `max_cuts` times per search) and its next
// round resumes exactly there, visiting the threads cyclically from that
// thread: every game still performs the same operations in the same order,
// only the round boundaries move. Each cut delays the game's remaining visits
// by at most one round, so the host runs max_cuts extra rounds. budget = 0:
// rounds always start at thread 0 (the step API and the single-game split).

// One round of game g's search schedule (see k_tree): virtual threads
// [t0, t1) visited cyclically from rp, each backing up its pending batch and
// selecting its next ones (chain splitting after `budget` re-selections, at
// most `max_cuts` cuts per search; cut_at = the thread whose chain stopped).
// Returns true when the search is complete after this round: every thread
// selected its `steps` batches and none waits for the NN (the reference's
// search has returned, mcts.h:252-255). fast: search_is_fast of this search
// (its batches per thread are search_steps_of, and it draws no root noise).
__device__ __forceinline__ bool search_round(const EngineView& E, int g, GameState* gs, size_t base, int t0,
                                             int t1, int B, bool do_backup, bool do_select, bool fresh, int rp,
                                             int budget, int max_cuts, int* cnt_add, int list_base, bool fast,
                                             WaveSearch& ws) {
    const int lane = lane_id();
    const int nt = t1 - t0;
    int chain = 0;  // re-selections after all-terminal batches in this round
    bool done = true;
    // a search's first round starts every thread fresh, also the ones a split
    // chain keeps it from visiting (their state is read from the next round on)
    // (strided: a search may run up to 1024 virtual threads)
    if (fresh && budget > 0)
        for (int t = t0 + lane; t < t1; t += 64) E.tstate[(size_t)g * E.L + t] = 0;
    for (int k = 0; k < nt && ws.cut_at < 0; ++k) {
        const int t = t0 + (rp - t0 + k) % nt;
        // virtual thread t: batches selected so far in this search, and whether
        // its last batch waits for the NN (a search's first round starts fresh)
        int* ts = E.tstate + (size_t)g * E.L + t;
        const int st = fresh ? 0 : *ts;
        int sel = st & kTstateSel;
        bool pend = (st & kTstatePend) != 0;
        if (do_backup && pend) {
            backup_range(E, g, base, t * B, (t + 1) * B, ws.count, ws.overflow, ws.acc.expansions);
            pend = false;
        }
        // the thread's next batch; one whose leaves are all terminal needs no NN
        // round trip (search_thread.cpp:102) and is backed up at once (:116-127),
        // then the thread selects again, up to `steps` batches per search
        bool again = false;  // the last batch was all terminal and is backed up
        while (do_select && !pend && sel < search_steps_of(E, fast)) {
            if (again && budget > 0 && chain >= budget) {
                if (ws.cuts < max_cuts) {
                    ws.cut_at = t;  // the next round continues this chain
                    ++ws.cuts;
                    break;
                }
                ws.over = true;  // no cut left: the chain runs on in this round
            }
            const unsigned long long ev0 = ws.acc.evals;
            const unsigned xp0 = ws.acc.exact_pending;
            TS_T(tsel0);
            select_range(E, g, gs, base, t * B, (t + 1) * B, ws.event, ws.hist_node, ws.hist_n, cnt_add, list_base, fast,
                         ws.acc);
            TS_T(tsel1);
            TS_ADD(kTsSelect, tsel1 - tsel0);
            TS_ADD(kTsBatches, 1);
            ++sel;
            // the round trip: an NN row, or a pending exact leaf for the solve
            // kernel; terminal and solved leaves alone are "all terminal"
            if (ws.acc.evals != ev0 || ws.acc.exact_pending != xp0 || !E.terminal_skip) {
                pend = true;
            } else {
                backup_range(E, g, base, t * B, (t + 1) * B, ws.count, ws.overflow, ws.acc.expansions);
                again = true;
                ++chain;
#if OAMD_CHAIN_PRIO > 0
                // an all-terminal chain holds its pipeline group's round (and so
                // its NN launch): from its first re-selection on, this wave
                // issues ahead of the other group's ResNet waves (priority 1)
                if (chain == 1) __builtin_amdgcn_s_setprio(OAMD_CHAIN_PRIO);
#endif
            }
        }
        if (lane == 0) *ts = sel | (pend ? kTstatePend : 0);
        done = done && sel >= search_steps_of(E, fast) && !pend;
    }
    return done && ws.cut_at < 0;
}

// The wave's work counters (lane 0): [0..1] this search (reset when a caller
// asks for them), [2..3] cumulative since the engine was created
// (oamd_engine_work_counters), [4..5] the searches that record timing events,
// [6] descent depths summed over every selected leaf, [7] the deepest descent
// (levels below the root; oamd_engine_descent_depths), and the tree kernels'
// algorithmic work (oamd_engine_tree_work): [8] children scanned over every
// descent level, [9] expansions, [10] children created, [11] tree launches
// (lane 0 of each launch's first wave). children: the game's node count
// growth this round (count_grown, no restart in between).
__device__ __forceinline__ void add_counters(const EngineView& E, const RoundAcc& acc, bool timed,
                                             unsigned children) {
    if (!E.counters) return;
    if (acc.sims) {
        atomicAdd(E.counters + 0, acc.sims);
        atomicAdd(E.counters + 1, acc.evals);
        atomicAdd(E.counters + 2, acc.sims);
        atomicAdd(E.counters + 3, acc.evals);
        if (timed) {
            atomicAdd(E.counters + 4, acc.sims);
            atomicAdd(E.counters + 5, acc.evals);
        }
        atomicAdd(E.counters + 6, acc.depth_sum);
        atomicMax(E.counters + 7, (unsigned long long)acc.depth_max);
        atomicAdd(E.counters + 8, acc.scan_sum);
    }
    if (acc.expansions) {
        atomicAdd(E.counters + 9, (unsigned long long)acc.expansions);
        atomicAdd(E.counters + 10, (unsigned long long)children);
    }
    if (acc.exact_hits) atomicAdd(E.counters + 13, (unsigned long long)acc.exact_hits);
}

// counter [11]: one per tree launch (lane 0 of its first wave, before any
// early return of an inactive game)
__device__ __forceinline__ void count_launch(const EngineView& E) {
    if (E.counters && blockIdx.x == 0 && lane_id() == 0) atomicAdd(E.counters + 11, 1ULL);
}

}  // namespace oamd
