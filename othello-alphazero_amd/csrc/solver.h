// Exact endgame solver, written once for the host and gfx950
// like bitboard.h: the CPU entry point (oamd_host_solve_endgame) and the device
// kernels (solver.hip) run the same state machine and count the same nodes.
//
// Semantics: the game ends when neither side can move; the result is the plain
// disc difference (mover minus opponent, no bonus for empties). A work item is
// one (position, legal root action): the position after the action is searched
// by negamax alpha-beta with the full window [-64, 64], so the item's score is
// exact. A forced pass is an action (64) and consumes no empty.
//
// Shape: an explicit stack, no recursion. The frame being searched lives in
// registers (SolveState); solve_step either takes its next move (pushing the
// frame when the child has moves of its own) or, when no move is left, pops the
// parent and hands it the value. A child that must pass is stored with the sides
// already swapped (`passed`), so a pass takes no stack level: level k has made
// k moves since the item's first position, and kSolveDepth levels cover the
// 16-empties cap. The stack is a template parameter: an array on the host,
// [level][word][lane] LDS words on the device.
//
// nodes = positions visited: the position after the root action, every position
// a move leads to, and once more for every position whose mover passes.
#pragma once

#include "../../include/othello_mcts_amd.h"
#include "bitboard.h"

namespace oamd {

constexpr int kSolveMaxEmpties = 16;
// levels stored at most: an item's first position has <= 16 empties (15 after
// a root move), level k has k fewer and is pushed only while its child has an
// empty left, so indices 0..14 are used
constexpr int kSolveDepth = 16;
constexpr int kSolveFrameWords = 7;  // me, opp, moves (2 words each) + the packed window

enum : int32_t { kSolveRunning = 0, kSolveDone = 1, kSolveLimit = 2 };

// Per-slot word of the workspace: node count in the low 56 bits, kSolve* status above.
constexpr int kSolveStatusShift = 56;

struct SolveState {
    uint64_t me, opp;  // discs of the frame's side to move / of the other side
    uint64_t moves;    // moves not tried yet
    int32_t alpha, beta, best;
    int32_t passed;  // the node's mover passed: me/opp are swapped, the window is the parent's
    int32_t sp;      // stack levels below this frame
    int32_t status;
    int32_t result;  // score of the root action for the root's mover
    int64_t nodes;
};

// Host stack: one packed frame per level.
struct SolveHostStack {
    uint32_t w[kSolveDepth][kSolveFrameWords];
    OAMD_HD void put(int level, int word, uint32_t v) { w[level][word] = v; }
    OAMD_HD uint32_t get(int level, int word) const { return w[level][word]; }
};

OAMD_HD int clz64(uint64_t x) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __clzll((long long)x);
#else
    return __builtin_clzll(x);
#endif
}

// Static move order: corners, then everything but the squares next to a
// corner, then those (C and X squares); within a class in action order.
constexpr uint64_t kSolveCorners = 0x8100000000000081ULL;
constexpr uint64_t kSolveNextToCorner = 0x42C300000000C342ULL;

OAMD_HD uint64_t solve_pick(uint64_t moves) {
    uint64_t c = moves & kSolveCorners;
    if (!c) c = moves & ~kSolveNextToCorner;
    if (!c) c = moves;
    return 1ULL << (63 - clz64(c));
}

template <class Stack>
OAMD_HD void solve_push(const SolveState& s, Stack& st) {
    st.put(s.sp, 0, (uint32_t)s.me);
    st.put(s.sp, 1, (uint32_t)(s.me >> 32));
    st.put(s.sp, 2, (uint32_t)s.opp);
    st.put(s.sp, 3, (uint32_t)(s.opp >> 32));
    st.put(s.sp, 4, (uint32_t)s.moves);
    st.put(s.sp, 5, (uint32_t)(s.moves >> 32));
    st.put(s.sp, 6, (uint32_t)(s.alpha + 128) | (uint32_t)(s.beta + 128) << 8 | (uint32_t)(s.best + 128) << 16 |
                        (uint32_t)s.passed << 24);
}

template <class Stack>
OAMD_HD void solve_pop(SolveState& s, const Stack& st) {
    s.me = (uint64_t)st.get(s.sp, 0) | (uint64_t)st.get(s.sp, 1) << 32;
    s.opp = (uint64_t)st.get(s.sp, 2) | (uint64_t)st.get(s.sp, 3) << 32;
    s.moves = (uint64_t)st.get(s.sp, 4) | (uint64_t)st.get(s.sp, 5) << 32;
    const uint32_t w = st.get(s.sp, 6);
    s.alpha = (int32_t)(w & 255) - 128;
    s.beta = (int32_t)(w >> 8 & 255) - 128;
    s.best = (int32_t)(w >> 16 & 255) - 128;
    s.passed = (int32_t)(w >> 24);
}

// A child's value v (for this frame's side to move) arrives.
OAMD_HD void solve_absorb(SolveState& s, int v) {
    if (v > s.best) s.best = v;
    if (v > s.alpha) s.alpha = v;
    if (s.alpha >= s.beta) s.moves = 0;  // cut-off: nothing left to try
}

// The position (cme to move, copp the other side) that the frame in `s` has
// just moved to, searched with the window (alpha, beta) of s's side: either it
// is terminal and its value is absorbed at once, or s is pushed and the child
// becomes the frame in registers. `root`: the child is the item's first
// position and there is no frame to push or to absorb into.
template <class Stack>
OAMD_HD void solve_enter(SolveState& s, Stack& st, uint64_t cme, uint64_t copp, bool root, int64_t node_limit) {
    if (++s.nodes > node_limit) {
        s.status = kSolveLimit;
        return;
    }
    uint64_t cm = 0, pm = 0;
    if (~(cme | copp) != 0) {  // a full board needs no move generation
        cm = legal_moves(cme, copp);
        if (!cm) pm = legal_moves(copp, cme);
    }
    if (!cm && !pm) {
        const int v = popcount64(copp) - popcount64(cme);  // for the side that moved here
        if (root) {
            s.result = v;
            s.status = kSolveDone;
        } else {
            solve_absorb(s, v);
        }
        return;
    }
    if (!cm && ++s.nodes > node_limit) {  // the position after the pass
        s.status = kSolveLimit;
        return;
    }
    if (!root) {
        if (s.sp >= kSolveDepth) {  // unreachable below the empties cap; never index past the stack
            s.status = kSolveLimit;
            return;
        }
        solve_push(s, st);
        ++s.sp;
    }
    const int a = s.alpha, b = s.beta;
    s.best = -65;
    if (cm) {
        s.me = cme;
        s.opp = copp;
        s.moves = cm;
        s.alpha = -b;
        s.beta = -a;
        s.passed = 0;
    } else {  // the child's mover passes: the parent's side moves again, with its own window
        s.me = copp;
        s.opp = cme;
        s.moves = pm;
        s.passed = 1;
    }
}

// Start the item: `me` to move plays `action` (a legal square, or 64 when it
// must pass) on (me, opp).
template <class Stack>
OAMD_HD void solve_begin(SolveState& s, Stack& st, uint64_t me, uint64_t opp, int action, int64_t node_limit) {
    s.sp = 0;
    s.status = kSolveRunning;
    s.result = OAMD_SOLVE_NONE;
    s.nodes = 0;
    s.alpha = -64;
    s.beta = 64;
    s.best = -65;
    s.passed = 0;
    s.moves = 0;
    s.me = me;
    s.opp = opp;
    uint64_t cme = opp, copp = me;
    if (action != 64) {
        const uint64_t m = 1ULL << (63 - action);
        const uint64_t f = flips(m, me, opp);
        cme = opp & ~f;
        copp = me | m | f;
    }
    solve_enter(s, st, cme, copp, true, node_limit);
}

// One step of a running item.
template <class Stack>
OAMD_HD void solve_step(SolveState& s, Stack& st, int64_t node_limit) {
    if (s.moves == 0) {  // the frame is searched: its value for the side that moved into it
        const int v = s.passed ? s.best : -s.best;
        if (s.sp == 0) {
            s.result = v;
            s.status = kSolveDone;
            return;
        }
        --s.sp;
        solve_pop(s, st);
        solve_absorb(s, v);
        return;
    }
    const uint64_t m = solve_pick(s.moves);
    s.moves ^= m;
    const uint64_t f = flips(m, s.me, s.opp);
    solve_enter(s, st, s.opp & ~f, s.me | m | f, false, node_limit);
}

// What the root is, before any search. Returns the OAMD_SOLVE_* flags (0 = to
// be searched or terminal). legal: the mover's squares; pass: it must pass.
struct SolveRoot {
    int32_t flags;
    bool terminal, pass;
    uint64_t me, opp, legal;
};

OAMD_HD SolveRoot solve_classify(int32_t player, uint64_t p1, uint64_t p2, int32_t max_empties) {
    SolveRoot r;
    r.flags = 0;
    r.terminal = r.pass = false;
    r.me = r.opp = r.legal = 0;
    if ((p1 & p2) != 0 || player < 0 || player > 2) {
        r.flags = OAMD_SOLVE_INVALID;
        return r;
    }
    const uint64_t m1 = legal_moves(p1, p2), m2 = legal_moves(p2, p1);
    if (!m1 && !m2) {
        r.terminal = true;
        return r;
    }
    if (player == 0) {  // marked terminal, but somebody can move: no side to search for
        r.flags = OAMD_SOLVE_INVALID;
        return r;
    }
    if (popcount64(~(p1 | p2)) > max_empties) {
        r.flags = OAMD_SOLVE_TOO_MANY_EMPTIES;
        return r;
    }
    r.me = player == 1 ? p1 : p2;
    r.opp = player == 1 ? p2 : p1;
    r.legal = player == 1 ? m1 : m2;
    r.pass = r.legal == 0;
    return r;
}

OAMD_HD bool solve_is_root_action(const SolveRoot& r, int action) {
    if (r.flags || r.terminal) return false;
    return action == 64 ? r.pass : (r.legal >> (63 - action) & 1) != 0;
}

// Position outputs from its 65 slots (move_scores as the items wrote them,
// words = nodes | status << kSolveStatusShift; 0 for a slot that is no action).
OAMD_HD void solve_reduce(int32_t player, uint64_t p1, uint64_t p2, int32_t max_empties, const int32_t* move_scores,
                          const int64_t* words, int32_t* score, int32_t* best_action, int32_t* flags,
                          int64_t* nodes) {
    const SolveRoot r = solve_classify(player, p1, p2, max_empties);
    int32_t fl = r.flags, sc = OAMD_SOLVE_NONE, best = -1;
    int64_t total = 0;
    if (r.terminal) {
        sc = popcount64(p1) - popcount64(p2);
    } else if (!fl) {
        for (int a = 0; a < 65; ++a) {
            if (!solve_is_root_action(r, a)) continue;
            total += words[a] & ((1LL << kSolveStatusShift) - 1);
            if ((words[a] >> kSolveStatusShift) != kSolveDone) fl |= OAMD_SOLVE_NODE_LIMIT;
            if (move_scores[a] > sc) {
                sc = move_scores[a];
                best = a;
            }
        }
        if (fl) {
            sc = OAMD_SOLVE_NONE;
            best = -1;
        }
    }
    if (score) *score = sc;
    if (best_action) *best_action = best;
    if (flags) *flags = fl;
    if (nodes) *nodes = total;
}

// The whole solver for one position on the host.
inline void solve_host(int32_t player, uint64_t p1, uint64_t p2, int32_t max_empties, int64_t node_limit,
                       int32_t* move_scores65, int32_t* score, int32_t* best_action, int32_t* flags,
                       int64_t* nodes) {
    const SolveRoot r = solve_classify(player, p1, p2, max_empties);
    int64_t words[65];
    SolveHostStack st;
    for (int a = 0; a < 65; ++a) {
        move_scores65[a] = OAMD_SOLVE_NONE;
        words[a] = 0;
        if (!solve_is_root_action(r, a)) continue;
        SolveState s;
        solve_begin(s, st, r.me, r.opp, a, node_limit);
        while (s.status == kSolveRunning) solve_step(s, st, node_limit);
        if (s.status == kSolveDone) move_scores65[a] = s.result;
        words[a] = s.nodes | (int64_t)s.status << kSolveStatusShift;
    }
    solve_reduce(player, p1, p2, max_empties, move_scores65, words, score, best_action, flags, nodes);
}

// Device entry points (solver.hip), called by the C ABI. workspace: one counter
// block + one word per slot, solve_workspace_bytes(n). workgroups = 0: enough
// to fill the chip, capped by the slot count.
inline int64_t solve_workspace_bytes(int64_t n) { return 256 + n * 65 * (int64_t)sizeof(int64_t); }
void launch_solve(const oamd_position* pos, int64_t n, int32_t max_empties, int64_t node_limit, int32_t* move_scores,
                  int32_t* score, int32_t* best_action, int32_t* flags, int64_t* nodes, void* workspace,
                  int32_t workgroups, int32_t compute_units, hipStream_t s);

}  // namespace oamd
