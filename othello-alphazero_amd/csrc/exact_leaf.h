// Exact leaf values: the rule, once, for the device (tree_search.h,
// exact_leaves.hip) and the host (oamd_exact_leaf_sign). A node with at most E
// empties that is not terminal and not a game's root is never expanded and
// never evaluated by the net: it is solved once (solver.h) and every later
// visit is a terminal-like leaf that carries the sign of the exact result.
#pragma once

#include <stdint.h>

#include "bitboard.h"
#include "solver.h"

namespace oamd {

constexpr int kExactMaxEmpties = 10;
// stack levels of a leaf's solve: an item's first position has <= 10 empties
// (10 after a root pass, 9 after a root move), level k has k fewer and is
// pushed only while its child has an empty left, so indices 0..9 are used
constexpr int kExactDepth = kExactMaxEmpties;

// ---- the empties test -----------------------------------------------------
// A node created by an expansion becomes an exact leaf (pending) when it is
// not terminal and has at most max_empties empties (0 = the feature is off).
OAMD_HD bool exact_leaf_position(int32_t player, uint64_t p1, uint64_t p2, int32_t max_empties) {
    return max_empties > 0 && player != 0 && popcount64(~(p1 | p2)) <= max_empties;
}

// ---- the mark ---------------------------------------------------------------
// NodeLink::first_child of a childless node: -1 plain, -2 pending, -3 / -4 / -5
// solved with s = -1 / 0 / +1 (s: the sign of the exact disc difference for
// the node's side to move). The per-row flag of a selected leaf (EngineView::
// exact) is -1 - mark: 0 none, 1 pending, 2 / 3 / 4 the result s = -1 / 0 / +1.
constexpr int32_t kMarkPlain = -1;
constexpr int32_t kMarkPending = -2;

OAMD_HD bool exact_mark(int32_t first_child) { return first_child <= kMarkPending; }
OAMD_HD int32_t exact_mark_solved(int32_t s) { return -4 - s; }
OAMD_HD int32_t exact_flag_of_mark(int32_t first_child) { return -1 - first_child; }
OAMD_HD int32_t exact_mark_of_flag(int32_t flag) { return -1 - flag; }
constexpr int32_t kExactFlagNone = 0;
constexpr int32_t kExactFlagPending = 1;
OAMD_HD int32_t exact_flag_of_sign(int32_t s) { return 3 + s; }
OAMD_HD int32_t exact_sign_of_flag(int32_t flag) { return flag - 3; }  // flag in 2..4
// what every node on the path receives: the value of a terminal leaf whose
// score for the parent's player is -s
OAMD_HD float exact_parent_value(int32_t s) { return s > 0 ? -1.0f : (s < 0 ? 1.0f : 0.0f); }

// A position the solve can take: a side to move, disjoint discs, at most
// kExactMaxEmpties empties, and somebody can move. A row that carries a mark
// always is one; anything else is a fault (a corrupted row), never searched.
OAMD_HD bool exact_solvable(int32_t player, uint64_t p1, uint64_t p2) {
    if ((player != 1 && player != 2) || (p1 & p2) != 0 || popcount64(~(p1 | p2)) > kExactMaxEmpties) return false;
    return legal_moves(p1, p2) != 0 || legal_moves(p2, p1) != 0;
}

// ---- solving ----------------------------------------------------------------
// Every legal root action of the leaf (the pass when its mover has no move) is
// one item, searched with the window [-1, 1] of the leaf's mover: fail-soft, so
// the item's result is >= 1, 0 or <= -1 exactly when the true score is.
constexpr int kExactAlpha = -1, kExactBeta = 1;
constexpr int64_t kExactNodeLimit = (int64_t)1 << 40;  // never reached below the empties cap

// The k-th root action of a leaf (ascending action; the pass is the only one
// of a mover without moves), -1 past the last.
OAMD_HD int exact_root_action(uint64_t legal, int k) {
    if (!legal) return k == 0 ? 64 : -1;
    const uint64_t m = solve_nth(legal, k);
    return m ? solve_action_of(m) : -1;
}

// One item on a stack of the caller's: its result for the leaf's mover and the nodes it visited.
template <class Stack>
OAMD_HD int32_t exact_solve_item(Stack& st, uint64_t me, uint64_t opp, int action, int64_t* nodes) {
    SolveState s;
    solve_begin(s, st, me, opp, action, kExactAlpha, kExactBeta, kExactNodeLimit);
    while (s.status == kSolveRunning) solve_step(s, st, kExactNodeLimit);
    *nodes = s.nodes;
    return s.status == kSolveDone ? s.result : 0;
}

// The reduction of the items' results to s: the sign of the best one.
OAMD_HD int32_t exact_reduce(int32_t best_result) { return best_result > 0 ? 1 : (best_result < 0 ? -1 : 0); }

// The rule on the host: false when the position is no exact leaf at this
// max_empties (terminal, too many empties, or the feature off); else *sign
// and the nodes of all its items.
inline bool exact_leaf_host(int32_t player, uint64_t p1, uint64_t p2, int32_t max_empties, int32_t* sign,
                            int64_t* nodes) {
    if (max_empties > kExactMaxEmpties) max_empties = kExactMaxEmpties;
    if ((p1 & p2) != 0 || player < 1 || player > 2) return false;
    const uint64_t me = player == 1 ? p1 : p2, opp = player == 1 ? p2 : p1;
    const uint64_t legal = legal_moves(me, opp);
    if (!legal && !legal_moves(opp, me)) return false;  // terminal whatever `player` says
    if (!exact_leaf_position(player, p1, p2, max_empties)) return false;
    SolveHostStack st;
    int32_t best = -65;
    int64_t total = 0;
    for (int k = 0;; ++k) {
        const int a = exact_root_action(legal, k);
        if (a < 0) break;
        int64_t n = 0;
        const int32_t r = exact_solve_item(st, me, opp, a, &n);
        total += n;
        if (r > best) best = r;
    }
    *sign = exact_reduce(best);
    *nodes = total;
    return true;
}

// Changing the setting (rule 7): allowed only while no game holds a tree built
// under another value, i.e. while nothing was searched since the last reset of
// all games. Setting the current value again is always allowed.
OAMD_HD bool exact_setting_change_ok(int32_t current, int32_t wanted, bool trees_built) {
    return wanted == current || !trees_built;
}

}  // namespace oamd
