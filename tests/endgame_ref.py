"""Independent reference for the exact endgame solver: plain Python negamax
over the ORACLE's bitboard functions (oracle/omcts_oracle.c, pinned to the
compiled reference by tests/test_oracle_golden.py). It shares no code with
csrc/solver.h: recursion instead of a state machine, its own move order
(fewest opponent moves first, where the solver uses a static square order),
its own handling of passes.

Two forms: ``minimax`` visits every line, ``alphabeta`` prunes; both are run
with the full window per root action, so every root action's score is exact.

Semantics (include/othello_mcts_amd.h): the game ends when neither side can
move, the result is the plain disc difference mover minus opponent, a forced
pass is action 64, a root where nobody can move is terminal with score black
minus white and best_action -1.
"""

from __future__ import annotations

import oracle as O

NONE = -128
FULL = (1 << 64) - 1


def popcount(x: int) -> int:
    return bin(x).count("1")


def squares(mask: int) -> list[int]:
    """Actions of a move mask in ascending order (square i = bit 63 - i)."""
    return [i for i in range(64) if mask >> (63 - i) & 1]


def play(me: int, opp: int, sq: int) -> tuple[int, int]:
    """(opponent's discs, mover's discs) after the mover plays square sq: the
    pair is in the order (side to move next, other side)."""
    m = 1 << (63 - sq)
    f = O.get_flips(m, me, opp)
    return opp & ~f, me | m | f


def minimax(me: int, opp: int) -> int:
    """Value for `me`, to move, by visiting every line."""
    moves = O.get_legal_moves(me, opp)
    if not moves:
        if not O.get_legal_moves(opp, me):
            return popcount(me) - popcount(opp)
        return -minimax(opp, me)
    return max(-minimax(*play(me, opp, sq)) for sq in squares(moves))


def alphabeta(me: int, opp: int, alpha: int = -64, beta: int = 64) -> int:
    """Value for `me`, to move, exact when it lies inside (alpha, beta)."""
    moves = O.get_legal_moves(me, opp)
    if not moves:
        if not O.get_legal_moves(opp, me):
            return popcount(me) - popcount(opp)
        return -alphabeta(opp, me, -beta, -alpha)
    children = [play(me, opp, sq) for sq in squares(moves)]
    if popcount(FULL & ~(me | opp)) >= 5:
        children.sort(key=lambda c: popcount(O.get_legal_moves(c[0], c[1])))
    best = -65
    for c in children:
        v = -alphabeta(c[0], c[1], -beta, -max(alpha, best))
        if v > best:
            best = v
            if best >= beta:
                break
    return best


def solve(player: int, p1: int, p2: int, search=alphabeta) -> tuple[list[int], int, int]:
    """(move_scores[65], score, best_action) of a position."""
    ms = [NONE] * 65
    m1, m2 = O.get_legal_moves(p1, p2), O.get_legal_moves(p2, p1)
    if not m1 and not m2:
        return ms, popcount(p1) - popcount(p2), -1
    me, opp, moves = (p1, p2, m1) if player == 1 else (p2, p1, m2)
    if not moves:
        ms[64] = -search(opp, me)
    for sq in squares(moves):
        ms[sq] = -search(*play(me, opp, sq))
    score = max(ms)
    return ms, score, ms.index(score)


def apply(player: int, p1: int, p2: int, action: int) -> tuple[int, int, int]:
    """(player, p1, p2) after a legal action; player 0 when the game is over."""
    me, opp = (p1, p2) if player == 1 else (p2, p1)
    if action != 64:
        opp, me = play(me, opp, action)
    p1, p2 = (me, opp) if player == 1 else (opp, me)
    over = not O.get_legal_moves(p1, p2) and not O.get_legal_moves(p2, p1)
    return (0 if over else 3 - player), p1, p2


# kinds of fixture positions (bits of the fixture's `kinds` column)
ROOT_PASS, ROOT_TERMINAL, PASS_INSIDE, ENDS_WITH_EMPTIES, WIPEOUT = 1, 2, 4, 8, 16


def kinds(player: int, p1: int, p2: int, solver=None) -> int:
    """Classify a position by its line of perfect play (best_action at every
    ply, to the end): the root must pass / is terminal, a pass occurs after the
    root's action, the game ends with empties left, one side ends with no
    discs. `solver(player, p1, p2) -> best_action` (default: this module)."""
    solver = solver or (lambda *p: solve(*p)[2])
    k, ply = 0, 0
    while True:
        a = solver(player, p1, p2)
        if a < 0:
            break
        if a == 64:
            k |= ROOT_PASS if ply == 0 else PASS_INSIDE
        player, p1, p2 = apply(player, p1, p2, a)
        ply += 1
    if ply == 0:
        k |= ROOT_TERMINAL
    if FULL & ~(p1 | p2):
        k |= ENDS_WITH_EMPTIES
    if p1 == 0 or p2 == 0:
        k |= WIPEOUT
    return k
