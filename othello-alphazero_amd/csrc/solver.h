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

// Fastest-first order of the split solver: with at least
// kSolveOrderMinEmpties empties and more than one untried move, the move after
// which the opponent has the fewest legal moves; ties go to the move that
// solve_pick takes first among the tied ones. Recomputed at every pick from
// the untried set, so the frame keeps its 7 words. Otherwise solve_pick.
constexpr int kSolveOrderMinEmpties = 6;

OAMD_HD uint64_t solve_pick_ordered(uint64_t me, uint64_t opp, uint64_t moves) {
    if ((moves & (moves - 1)) == 0 || popcount64(~(me | opp)) < kSolveOrderMinEmpties) return solve_pick(moves);
    uint64_t tied = 0;
    int fewest = 65;
    for (uint64_t rest = moves; rest; rest &= rest - 1) {
        const uint64_t m = rest & (0 - rest);
        const uint64_t f = flips(m, me, opp);
        const int c = popcount64(legal_moves(opp & ~f, me | m | f));
        if (c < fewest) {
            fewest = c;
            tied = 0;
        }
        if (c == fewest) tied |= m;
    }
    return solve_pick(tied);
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
// must pass) on (me, opp); the item is searched with the window (alpha, beta)
// of `me`. The search is fail-soft: a result outside the window is a bound on
// the exact score from that side.
template <class Stack>
OAMD_HD void solve_begin(SolveState& s, Stack& st, uint64_t me, uint64_t opp, int action, int alpha, int beta,
                         int64_t node_limit) {
    s.sp = 0;
    s.status = kSolveRunning;
    s.result = OAMD_SOLVE_NONE;
    s.nodes = 0;
    s.alpha = alpha;
    s.beta = beta;
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

// The full window [-64, 64]: the item's score is exact.
template <class Stack>
OAMD_HD void solve_begin(SolveState& s, Stack& st, uint64_t me, uint64_t opp, int action, int64_t node_limit) {
    solve_begin(s, st, me, opp, action, -64, 64, node_limit);
}

// One step of a running item. Ordered: moves are taken by solve_pick_ordered
// (the split solver) instead of solve_pick.
template <bool Ordered, class Stack>
OAMD_HD void solve_step_as(SolveState& s, Stack& st, int64_t node_limit) {
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
    const uint64_t m = Ordered ? solve_pick_ordered(s.me, s.opp, s.moves) : solve_pick(s.moves);
    s.moves ^= m;
    const uint64_t f = flips(m, s.me, s.opp);
    solve_enter(s, st, s.opp & ~f, s.me | m | f, false, node_limit);
}

template <class Stack>
OAMD_HD void solve_step(SolveState& s, Stack& st, int64_t node_limit) {
    solve_step_as<false>(s, st, node_limit);
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

// ---------------------------------------------------------------------------
// Split solver: the work item is one move of the position one
// ply below the root action, searched with the ordered pick.
//
// For a root action a, Q is the position after a and R is Q, or Q after a pass
// when Q's mover has no move. Game over at Q: no item, the score is the disc
// difference. Otherwise the items are the moves of R's mover: phase A searches
// the ordered pick's first move with the full window and gives L (for R's
// mover); phase B searches every other move with the window (L, 64), all with
// the same L, unless L = 64. Fail-soft: value(R) = max(L, phase B results).
//
// Item space per position: root actions by rank (ascending action, <= 16 below
// the empties cap) x moves of R by rank (<= 16) = kSplitSlots slots.
// nodes = per root action 1 for Q, 1 more when Q's mover passes, plus the
// nodes of its items; node_limit is a budget per item.
// ---------------------------------------------------------------------------
constexpr int kSplitRanks = 16;
constexpr int kSplitSlots = kSplitRanks * kSplitRanks;

enum : int8_t { kPlanNone = 0, kPlanTerminal = 1, kPlanItems = 2 };

// What the planning step writes per (position, root action rank).
struct SolvePlan {
    uint64_t me, opp;  // R: discs of its mover / of the other side
    uint64_t moves;    // R's mover's moves: the items
    int8_t kind;       // kPlan*
    int8_t action;     // the root action (0..64)
    int8_t first;      // the phase A move, as an action (0..63)
    int8_t sign;       // +1 when R's mover is the root's mover (Q's mover passed), else -1
    int8_t qnodes;     // 1 for Q, 2 when Q's mover passes
    int8_t score;      // kPlanTerminal: the root action's score for the root's mover
    int8_t pad[2];
};
static_assert(sizeof(SolvePlan) == 32, "layout");

// The k-th member of `set` in action order (most significant bit first); 0 when there is none.
OAMD_HD uint64_t solve_nth(uint64_t set, int k) {
    for (; set; set &= ~(1ULL << (63 - clz64(set)))) {
        if (k-- == 0) return 1ULL << (63 - clz64(set));
    }
    return 0;
}

OAMD_HD int solve_action_of(uint64_t move) { return clz64(move); }

// The plan of the root action of rank `rank` (kPlanNone when there is none).
OAMD_HD SolvePlan solve_plan(const SolveRoot& r, int rank) {
    SolvePlan p;
    p.me = p.opp = p.moves = 0;
    p.kind = kPlanNone;
    p.action = p.first = p.sign = p.qnodes = p.score = 0;
    p.pad[0] = p.pad[1] = 0;
    if (r.flags || r.terminal) return p;
    uint64_t qme = r.opp, qopp = r.me;  // Q after the root's pass
    if (r.pass) {
        if (rank != 0) return p;
        p.action = 64;
    } else {
        const uint64_t m = solve_nth(r.legal, rank);
        if (!m) return p;
        const uint64_t f = flips(m, r.me, r.opp);
        qme = r.opp & ~f;
        qopp = r.me | m | f;
        p.action = (int8_t)solve_action_of(m);
    }
    uint64_t qm = 0, pm = 0;
    if (~(qme | qopp) != 0) {
        qm = legal_moves(qme, qopp);
        if (!qm) pm = legal_moves(qopp, qme);
    }
    p.qnodes = 1;
    if (!qm && !pm) {
        p.kind = kPlanTerminal;
        p.score = (int8_t)(popcount64(qopp) - popcount64(qme));
        return p;
    }
    p.kind = kPlanItems;
    if (qm) {
        p.me = qme;
        p.opp = qopp;
        p.moves = qm;
        p.sign = -1;
    } else {
        p.me = qopp;
        p.opp = qme;
        p.moves = pm;
        p.sign = 1;
        p.qnodes = 2;
    }
    p.first = (int8_t)solve_action_of(solve_pick_ordered(p.me, p.opp, p.moves));
    return p;
}

// The item of slot `j` of a plan in `phase` (0 = A, 1 = B): the move to search,
// 0 when the slot holds no item. a_score / a_word: the plan's phase A result
// (phase B only). *alpha: the lower bound of the item's window for R's mover.
OAMD_HD uint64_t solve_split_item(const SolvePlan& p, int phase, int j, int32_t a_score, int64_t a_word, int* alpha) {
    *alpha = -64;
    if (p.kind != kPlanItems) return 0;
    const uint64_t first = 1ULL << (63 - p.first);
    if (phase == 0) return first;
    if ((a_word >> kSolveStatusShift) != kSolveDone || a_score >= 64) return 0;
    const uint64_t m = solve_nth(p.moves, j);
    if (m == first) return 0;
    *alpha = a_score;
    return m;
}

// Position outputs from its kSplitRanks plans, their phase A results and the
// kSplitSlots phase B slots (words = nodes | status << kSolveStatusShift; 0
// for a slot that held no item). move_scores65 is written in full.
OAMD_HD void solve_reduce_split(int32_t player, uint64_t p1, uint64_t p2, int32_t max_empties, const SolvePlan* plan,
                                const int32_t* a_scores, const int64_t* a_words, const int32_t* b_scores,
                                const int64_t* b_words, int32_t* move_scores65, int32_t* score, int32_t* best_action,
                                int32_t* flags, int64_t* nodes) {
    const SolveRoot r = solve_classify(player, p1, p2, max_empties);
    const int64_t mask = (1LL << kSolveStatusShift) - 1;
    int32_t fl = r.flags, sc = OAMD_SOLVE_NONE, best = -1;
    int64_t total = 0;
    for (int a = 0; a < 65; ++a) move_scores65[a] = OAMD_SOLVE_NONE;
    if (r.terminal) {
        sc = popcount64(p1) - popcount64(p2);
    } else if (!fl) {
        // ranks ascend with the action, so the first maximum is the lowest action as in solve_reduce
        for (int i = 0; i < kSplitRanks; ++i) {
            const SolvePlan p = plan[i];
            if (p.kind == kPlanNone) break;
            total += p.qnodes;
            int32_t v;
            if (p.kind == kPlanTerminal) {
                v = p.score;
            } else {
                bool done = (a_words[i] >> kSolveStatusShift) == kSolveDone;
                total += a_words[i] & mask;
                int32_t value = a_scores[i];
                if (done && value < 64) {
                    const uint64_t first = 1ULL << (63 - p.first);
                    int j = 0;
                    for (uint64_t rest = p.moves; rest && j < kSplitRanks; rest &= ~(1ULL << (63 - clz64(rest))), ++j) {
                        if ((1ULL << (63 - clz64(rest))) == first) continue;
                        const int64_t w = b_words[i * kSplitRanks + j];
                        total += w & mask;
                        if ((w >> kSolveStatusShift) != kSolveDone) done = false;
                        else if (b_scores[i * kSplitRanks + j] > value) value = b_scores[i * kSplitRanks + j];
                    }
                }
                if (!done) {
                    fl |= OAMD_SOLVE_NODE_LIMIT;
                    continue;
                }
                v = p.sign * value;
            }
            move_scores65[p.action] = v;
            if (v > sc) {
                sc = v;
                best = p.action;
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

// The whole split solver for one position on the host: plan, phase A, phase B, reduce.
inline void solve_host_split(int32_t player, uint64_t p1, uint64_t p2, int32_t max_empties, int64_t node_limit,
                             int32_t* move_scores65, int32_t* score, int32_t* best_action, int32_t* flags,
                             int64_t* nodes) {
    const SolveRoot r = solve_classify(player, p1, p2, max_empties);
    SolvePlan plan[kSplitRanks];
    int32_t a_scores[kSplitRanks] = {}, b_scores[kSplitSlots];
    int64_t a_words[kSplitRanks] = {}, b_words[kSplitSlots];
    SolveHostStack st;
    for (int i = 0; i < kSplitRanks; ++i) plan[i] = solve_plan(r, i);
    for (int phase = 0; phase < 2; ++phase) {
        for (int slot = 0; slot < (phase ? kSplitSlots : kSplitRanks); ++slot) {
            const int i = phase ? slot / kSplitRanks : slot;
            int alpha;
            const uint64_t m = solve_split_item(plan[i], phase, slot % kSplitRanks, a_scores[i], a_words[i], &alpha);
            int32_t sc = OAMD_SOLVE_NONE;
            int64_t w = 0;
            if (m) {
                SolveState s;
                solve_begin(s, st, plan[i].me, plan[i].opp, solve_action_of(m), alpha, 64, node_limit);
                while (s.status == kSolveRunning) solve_step_as<true>(s, st, node_limit);
                if (s.status == kSolveDone) sc = s.result;
                w = s.nodes | (int64_t)s.status << kSolveStatusShift;
            }
            (phase ? b_scores : a_scores)[slot] = sc;
            (phase ? b_words : a_words)[slot] = w;
        }
    }
    solve_reduce_split(player, p1, p2, max_empties, plan, a_scores, a_words, b_scores, b_words, move_scores65, score,
                       best_action, flags, nodes);
}

// Device entry points (solver.hip), called by the C ABI. workspace: one counter
// block + one word per slot, solve_workspace_bytes(n). workgroups = 0: enough
// to fill the chip, capped by the slot count.
inline int64_t solve_workspace_bytes(int64_t n) { return 256 + n * 65 * (int64_t)sizeof(int64_t); }
void launch_solve(const oamd_position* pos, int64_t n, int32_t max_empties, int64_t node_limit, int32_t* move_scores,
                  int32_t* score, int32_t* best_action, int32_t* flags, int64_t* nodes, void* workspace,
                  int32_t workgroups, int32_t compute_units, hipStream_t s);

// The split solver's workspace, widest alignment first: the counter block (one
// counter per phase), the plans, the node words of both phases, their scores.
struct SplitWorkspace {
    unsigned long long* counters;
    SolvePlan* plan;
    int64_t *a_words, *b_words;
    int32_t *a_scores, *b_scores;
    SplitWorkspace(void* base, int64_t n) {
        char* p = static_cast<char*>(base);
        counters = reinterpret_cast<unsigned long long*>(p);
        p += 256;
        plan = reinterpret_cast<SolvePlan*>(p);
        p += n * kSplitRanks * (int64_t)sizeof(SolvePlan);
        a_words = reinterpret_cast<int64_t*>(p);
        p += n * kSplitRanks * (int64_t)sizeof(int64_t);
        b_words = reinterpret_cast<int64_t*>(p);
        p += n * kSplitSlots * (int64_t)sizeof(int64_t);
        a_scores = reinterpret_cast<int32_t*>(p);
        p += n * kSplitRanks * (int64_t)sizeof(int32_t);
        b_scores = reinterpret_cast<int32_t*>(p);
    }
};
inline int64_t solve_split_workspace_bytes(int64_t n) {
    return 256 + n * (kSplitRanks * (int64_t)(sizeof(SolvePlan) + sizeof(int64_t) + sizeof(int32_t)) +
                      kSplitSlots * (int64_t)(sizeof(int64_t) + sizeof(int32_t)));
}
void launch_solve_split(const oamd_position* pos, int64_t n, int32_t max_empties, int64_t node_limit,
                        int32_t* move_scores, int32_t* score, int32_t* best_action, int32_t* flags, int64_t* nodes,
                        void* workspace, int32_t workgroups, int32_t compute_units, hipStream_t s);

}  // namespace oamd
