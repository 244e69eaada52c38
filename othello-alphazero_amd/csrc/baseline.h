// Baseline opponents, written once for the host and gfx950
// like solver.h: the CPU entry point (oamd_host_baseline_move) and the device
// kernels (baseline.hip) run the same state machine and count the same nodes.
//
// A baseline maps a position with a side to move to one score per root action
// (squares 0..63, 64 = the forced pass) and picks one action from the scores.
//   RANDOM  every root action scores 0
//   GREEDY  a square scores the discs it flips, the pass 0
//   SEARCH  negamax to `depth` disc placements below the root, int32:
//             V(P, d) = T(P)                     neither side can move
//                     = -V(P swapped, d)         the mover cannot move (no depth consumed)
//                     = h(P)                     d == 0
//                     = max_m -V(P.m, d - 1)     otherwise
//             T = 4096 * sgn(delta) + delta, delta = mover's discs minus the other side's
//             h = 10 (M_me - M_opp) + 50 (K_me - K_opp) - 20 (X_me - X_opp) + (D_me - D_opp)
//           score[a] = -V(P.a, depth - 1), score[64] = -V(P swapped, depth).
//
// A work item is one (position, root action), searched by alpha-beta with the
// full window, fail-soft, so the item's score is the exact minimax value; moves
// are taken in solve_pick's static order. The shape is solver.h's: an explicit
// stack, the frame being searched in registers, a passing child stored with
// the sides swapped so that a pass takes no stack level. A frame carries the
// disc placements it may still make (`depth` >= 1); a child with none left is
// evaluated where it is entered and never becomes a frame.
//
// nodes = positions visited (the position after the root action, every position
// a move leads to, once more for every position whose mover passes) plus one
// per static evaluation. RANDOM and GREEDY visit nothing: 0.
#pragma once

#include "../../include/othello_mcts_amd.h"
#include "bitboard.h"
#include "rng.h"
#include "solver.h"

namespace oamd {

constexpr int kBaselineMaxDepth = 10;
// Stack levels: a frame is pushed when its child becomes a frame, i.e. has at
// least one placement left. The first frame of an item has depth - 1 left
// (depth after a root pass), so at most depth - 1 <= 9 frames are ever stored.
constexpr int kBaselineLevels = kBaselineMaxDepth;
// me, opp, moves (2 words each), the window (alpha | beta), best | passed | depth
constexpr int kBaselineFrameWords = 8;
constexpr int32_t kBaselineInf = 8191;    // above every value: |T| <= 4160, |h| < 1000
constexpr int32_t kBaselineBias = 8192;   // packs a value of [-8192, 8191] into 14 bits
constexpr int32_t kBaselineWin = 4096;

struct BaselineState {
    uint64_t me, opp;  // discs of the frame's side to move / of the other side
    uint64_t moves;    // moves not tried yet
    int32_t alpha, beta, best;
    int32_t passed;  // the node's mover passed: me/opp are swapped, the window is the parent's
    int32_t depth;   // disc placements the frame's side may still look ahead, >= 1
    int32_t sp;      // stack levels below this frame
    int32_t status;  // kSolve*
    int32_t result;  // score of the root action for the root's mover
    int64_t nodes;
};

struct BaselineHostStack {
    uint32_t w[kBaselineLevels][kBaselineFrameWords];
    OAMD_HD void put(int level, int word, uint32_t v) { w[level][word] = v; }
    OAMD_HD uint32_t get(int level, int word) const { return w[level][word]; }
};

// Value of a finished game for the side with `mine` discs.
OAMD_HD int32_t baseline_terminal(uint64_t mine, uint64_t theirs) {
    const int32_t d = popcount64(mine) - popcount64(theirs);
    return d > 0 ? kBaselineWin + d : d < 0 ? d - kBaselineWin : 0;
}

// X-squares (actions 9, 14, 49, 54) whose corner (0, 7, 56, 63) is in `empty`.
OAMD_HD uint64_t baseline_open_x(uint64_t empty) {
    return (empty & (1ULL << 63)) >> 9 | (empty & (1ULL << 56)) >> 7 | (empty & (1ULL << 7)) << 7 |
           (empty & 1ULL) << 9;
}

// The static evaluation for the side `me`, whose legal moves are my_moves.
OAMD_HD int32_t baseline_eval(uint64_t me, uint64_t opp, uint64_t my_moves, uint64_t opp_moves) {
    const uint64_t x = baseline_open_x(~(me | opp));
    return 10 * (popcount64(my_moves) - popcount64(opp_moves)) +
           50 * (popcount64(me & kSolveCorners) - popcount64(opp & kSolveCorners)) -
           20 * (popcount64(me & x) - popcount64(opp & x)) + (popcount64(me) - popcount64(opp));
}

template <class Stack>
OAMD_HD void baseline_push(const BaselineState& s, Stack& st) {
    st.put(s.sp, 0, (uint32_t)s.me);
    st.put(s.sp, 1, (uint32_t)(s.me >> 32));
    st.put(s.sp, 2, (uint32_t)s.opp);
    st.put(s.sp, 3, (uint32_t)(s.opp >> 32));
    st.put(s.sp, 4, (uint32_t)s.moves);
    st.put(s.sp, 5, (uint32_t)(s.moves >> 32));
    st.put(s.sp, 6, (uint32_t)(s.alpha + kBaselineBias) | (uint32_t)(s.beta + kBaselineBias) << 16);
    st.put(s.sp, 7, (uint32_t)(s.best + kBaselineBias) | (uint32_t)s.passed << 16 | (uint32_t)s.depth << 20);
}

template <class Stack>
OAMD_HD void baseline_pop(BaselineState& s, const Stack& st) {
    s.me = (uint64_t)st.get(s.sp, 0) | (uint64_t)st.get(s.sp, 1) << 32;
    s.opp = (uint64_t)st.get(s.sp, 2) | (uint64_t)st.get(s.sp, 3) << 32;
    s.moves = (uint64_t)st.get(s.sp, 4) | (uint64_t)st.get(s.sp, 5) << 32;
    const uint32_t w = st.get(s.sp, 6), v = st.get(s.sp, 7);
    s.alpha = (int32_t)(w & 0xFFFF) - kBaselineBias;
    s.beta = (int32_t)(w >> 16) - kBaselineBias;
    s.best = (int32_t)(v & 0xFFFF) - kBaselineBias;
    s.passed = (int32_t)(v >> 16 & 1);
    s.depth = (int32_t)(v >> 20);
}

// A child's value v (for this frame's side to move) arrives.
OAMD_HD void baseline_absorb(BaselineState& s, int32_t v) {
    if (v > s.best) s.best = v;
    if (v > s.alpha) s.alpha = v;
    if (s.alpha >= s.beta) s.moves = 0;  // cut-off: nothing left to try
}

// The position (cme to move, copp the other side) that the frame in `s` has
// just moved to, with `cdepth` placements left and the window of s's side:
// its value is absorbed at once when the game is over there or cdepth is 0;
// otherwise s is pushed and the child becomes the frame in registers. `root`:
// the child is the item's first position, there is no frame to push or to
// absorb into.
template <class Stack>
OAMD_HD void baseline_enter(BaselineState& s, Stack& st, uint64_t cme, uint64_t copp, int32_t cdepth, bool root,
                            int64_t node_limit) {
    if (++s.nodes > node_limit) {
        s.status = kSolveLimit;
        return;
    }
    uint64_t cm = 0, pm = 0;
    if (~(cme | copp) != 0) {  // a full board needs no move generation
        cm = legal_moves(cme, copp);
        if (!cm || cdepth == 0) pm = legal_moves(copp, cme);
    }
    bool leaf = false;
    int32_t v = 0;  // for the side that moved here
    if (!cm && !pm) {
        leaf = true;
        v = baseline_terminal(copp, cme);
    } else {
        if (!cm && ++s.nodes > node_limit) {  // the position after the pass
            s.status = kSolveLimit;
            return;
        }
        if (cdepth == 0) {
            if (++s.nodes > node_limit) {  // the static evaluation
                s.status = kSolveLimit;
                return;
            }
            leaf = true;
            v = baseline_eval(copp, cme, pm, cm);  // h is antisymmetric: a pass changes nothing
        }
    }
    if (leaf) {
        if (root) {
            s.result = v;
            s.status = kSolveDone;
        } else {
            baseline_absorb(s, v);
        }
        return;
    }
    if (!root) {
        if (s.sp >= kBaselineLevels) {  // unreachable below the depth cap; never index past the stack
            s.status = kSolveLimit;
            return;
        }
        baseline_push(s, st);
        ++s.sp;
    }
    const int32_t a = s.alpha, b = s.beta;
    s.best = -kBaselineInf - 1;
    s.depth = cdepth;
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
// must pass) on (me, opp). RANDOM and GREEDY are done here.
template <class Stack>
OAMD_HD void baseline_begin(BaselineState& s, Stack& st, uint64_t me, uint64_t opp, int action, int32_t kind,
                            int32_t depth, int64_t node_limit) {
    s.sp = 0;
    s.status = kSolveRunning;
    s.result = OAMD_BASELINE_NONE;
    s.nodes = 0;
    s.alpha = -kBaselineInf;
    s.beta = kBaselineInf;
    s.best = -kBaselineInf - 1;
    s.passed = 0;
    s.depth = 0;
    s.moves = 0;
    s.me = me;
    s.opp = opp;
    uint64_t f = 0, m = 0;
    if (action != 64) {
        m = 1ULL << (63 - action);
        f = flips(m, me, opp);
    }
    if (kind != OAMD_BASELINE_SEARCH) {
        s.result = kind == OAMD_BASELINE_GREEDY ? popcount64(f) : 0;
        s.status = kSolveDone;
        return;
    }
    if (action != 64)
        baseline_enter(s, st, opp & ~f, me | m | f, depth - 1, true, node_limit);
    else
        baseline_enter(s, st, opp, me, depth, true, node_limit);
}

// One step of a running item.
template <class Stack>
OAMD_HD void baseline_step(BaselineState& s, Stack& st, int64_t node_limit) {
    if (s.moves == 0) {  // the frame is searched: its value for the side that moved into it
        const int32_t v = s.passed ? s.best : -s.best;
        if (s.sp == 0) {
            s.result = v;
            s.status = kSolveDone;
            return;
        }
        --s.sp;
        baseline_pop(s, st);
        baseline_absorb(s, v);
        return;
    }
    const uint64_t m = solve_pick(s.moves);
    s.moves ^= m;
    const uint64_t f = flips(m, s.me, s.opp);
    baseline_enter(s, st, s.opp & ~f, s.me | m | f, s.depth - 1, false, node_limit);
}

// The root as solve_classify sees it, without an empties cap.
OAMD_HD SolveRoot baseline_classify(int32_t player, uint64_t p1, uint64_t p2) {
    return solve_classify(player, p1, p2, 64);
}

// The pick: among the root actions with the maximal score, the lowest without
// a key; with one, the k-th lowest, k = min(nt - 1, (int)(u * nt)), u the
// first uniform of the stream (key, event, 0): choose_root_action's argmax rule.
OAMD_HD int32_t baseline_pick(const int32_t* move_scores65, int32_t best, bool has_key, uint64_t key, uint64_t event) {
    int nt = 0;
    for (int a = 0; a < 65; ++a) nt += move_scores65[a] == best;
    int k = 0;
    if (has_key) {
        const float u = uniform(stream_key(key, event, 0), 0);
        k = (int)(u * (float)nt);
        if (k >= nt) k = nt - 1;
    }
    for (int a = 0; a < 65; ++a)
        if (move_scores65[a] == best && k-- == 0) return a;
    return -1;
}

// Position outputs from its 65 slots (move_scores as the items wrote them,
// words = nodes | status << kSolveStatusShift; 0 for a slot that is no action).
// The row of a flagged position is reset to OAMD_BASELINE_NONE.
OAMD_HD void baseline_reduce(int32_t player, uint64_t p1, uint64_t p2, bool has_key, uint64_t key, uint64_t event,
                             int32_t* move_scores65, const int64_t* words, int32_t* score, int32_t* action,
                             int32_t* flags, int64_t* nodes) {
    const SolveRoot r = baseline_classify(player, p1, p2);
    int32_t fl = r.flags, sc = OAMD_BASELINE_NONE, act = -1;
    int64_t total = 0;
    if (!fl && !r.terminal) {
        for (int a = 0; a < 65; ++a) {
            if (!solve_is_root_action(r, a)) continue;
            total += words[a] & ((1LL << kSolveStatusShift) - 1);
            if ((words[a] >> kSolveStatusShift) != kSolveDone) fl |= OAMD_SOLVE_NODE_LIMIT;
            else if (move_scores65[a] > sc) sc = move_scores65[a];
        }
    }
    if (fl) {
        sc = OAMD_BASELINE_NONE;
        for (int a = 0; a < 65; ++a) move_scores65[a] = OAMD_BASELINE_NONE;
    } else if (!r.terminal) {
        act = baseline_pick(move_scores65, sc, has_key, key, event);
    }
    if (score) *score = sc;
    if (action) *action = act;
    if (flags) *flags = fl;
    if (nodes) *nodes = total;
}

// The whole baseline for one position on the host.
inline void baseline_host(int32_t player, uint64_t p1, uint64_t p2, int32_t kind, int32_t depth, int64_t node_limit,
                          bool has_key, uint64_t key, uint64_t event, int32_t* move_scores65, int32_t* score,
                          int32_t* action, int32_t* flags, int64_t* nodes) {
    const SolveRoot r = baseline_classify(player, p1, p2);
    int64_t words[65];
    BaselineHostStack st;
    for (int a = 0; a < 65; ++a) {
        move_scores65[a] = OAMD_BASELINE_NONE;
        words[a] = 0;
        if (!solve_is_root_action(r, a)) continue;
        BaselineState s;
        baseline_begin(s, st, r.me, r.opp, a, kind, depth, node_limit);
        while (s.status == kSolveRunning) baseline_step(s, st, node_limit);
        if (s.status == kSolveDone) move_scores65[a] = s.result;
        words[a] = s.nodes | (int64_t)s.status << kSolveStatusShift;
    }
    baseline_reduce(player, p1, p2, has_key, key, event, move_scores65, words, score, action, flags, nodes);
}

// Device entry point (baseline.hip), called by the C ABI. workspace: one counter
// block + one word per slot. workgroups = 0: enough to fill the chip, capped by
// the slot count. keys / events: (n) device arrays or nullptr.
inline int64_t baseline_workspace_bytes(int64_t n) { return 256 + n * 65 * (int64_t)sizeof(int64_t); }
void launch_baseline(const oamd_position* pos, int64_t n, int32_t kind, int32_t depth, int64_t node_limit,
                     const int64_t* keys, const int64_t* events, int32_t* move_scores, int32_t* score,
                     int32_t* action, int32_t* flags, int64_t* nodes, void* workspace, int32_t workgroups,
                     int32_t compute_units, hipStream_t s);

}  // namespace oamd
