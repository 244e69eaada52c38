"""Independent reference for the baseline opponents (include/othello_mcts_amd.h
OAMD_BASELINE_*): plain Python on integer bitboards with its own move
generation and flips (ray walks square by square), recursion and no pruning.
It shares no code with csrc/baseline.h or the package.

Squares: action a = row * 8 + column is bit 63 - a. ``move_scores(kind, depth,
player, p1, p2)`` gives the 65 scores (NONE where there is no root action),
``first_max`` the lowest action with the maximal score. ``STATS`` counts, for
the last ``move_scores`` call, the passes crossed below the root action and the
finished games met before the depth ran out.
"""

from __future__ import annotations

NONE = -(1 << 31)
RANDOM, GREEDY, SEARCH = 0, 1, 2
DIRS = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]
CORNERS = (0, 7, 56, 63)
X_OF_CORNER = ((9, 0), (14, 7), (49, 56), (54, 63))
STATS = {"passes": 0, "early_terminals": 0}


def bit(a: int) -> int:
    return 1 << (63 - a)


def count(x: int) -> int:
    return bin(x).count("1")


def flipped(a: int, me: int, opp: int) -> int:
    """Discs of opp that a disc of me on the empty square a turns over."""
    r0, c0 = divmod(a, 8)
    out = 0
    for dr, dc in DIRS:
        r, c, run = r0 + dr, c0 + dc, 0
        while 0 <= r < 8 and 0 <= c < 8 and opp & bit(r * 8 + c):
            run |= bit(r * 8 + c)
            r, c = r + dr, c + dc
        if run and 0 <= r < 8 and 0 <= c < 8 and me & bit(r * 8 + c):
            out |= run
    return out


def moves_of(me: int, opp: int) -> list[int]:
    """Legal squares of me, ascending."""
    occupied = me | opp
    near = 0  # empty squares next to a disc of opp: the only candidates
    for a in range(64):
        if opp & bit(a):
            r0, c0 = divmod(a, 8)
            for dr, dc in DIRS:
                r, c = r0 + dr, c0 + dc
                if 0 <= r < 8 and 0 <= c < 8 and not occupied & bit(r * 8 + c):
                    near |= bit(r * 8 + c)
    return [a for a in range(64) if near & bit(a) and flipped(a, me, opp)]


def after(a: int, me: int, opp: int) -> tuple[int, int]:
    """(side to move next, other side) after me plays square a."""
    f = flipped(a, me, opp)
    return opp & ~f, me | bit(a) | f


def terminal_value(me: int, opp: int) -> int:
    d = count(me) - count(opp)
    return 4096 * ((d > 0) - (d < 0)) + d


def heuristic(me: int, opp: int, my_moves: list[int], opp_moves: list[int]) -> int:
    h = 10 * (len(my_moves) - len(opp_moves)) + count(me) - count(opp)
    for c in CORNERS:
        h += 50 * (bool(me & bit(c)) - bool(opp & bit(c)))
    for x, c in X_OF_CORNER:
        if not (me | opp) & bit(c):
            h -= 20 * (bool(me & bit(x)) - bool(opp & bit(x)))
    return h


def value(me: int, opp: int, d: int) -> int:
    """V(P, d) for the side `me`, to move."""
    mine = moves_of(me, opp)
    if not mine:
        theirs = moves_of(opp, me)
        if not theirs:
            STATS["early_terminals"] += 1
            return terminal_value(me, opp)
        STATS["passes"] += 1
        return -value(opp, me, d)
    if d == 0:
        return heuristic(me, opp, mine, moves_of(opp, me))
    return max(-value(*after(a, me, opp), d - 1) for a in mine)


def move_scores(kind: int, depth: int, player: int, p1: int, p2: int) -> list[int]:
    STATS["passes"] = STATS["early_terminals"] = 0
    ms = [NONE] * 65
    me, opp = (p1, p2) if player == 1 else (p2, p1)
    mine = moves_of(me, opp)
    if not mine:
        if not moves_of(opp, me):
            return ms  # nobody can move: no action
        ms[64] = 0 if kind != SEARCH else -value(opp, me, depth)
    for a in mine:
        if kind == RANDOM:
            ms[a] = 0
        elif kind == GREEDY:
            ms[a] = count(flipped(a, me, opp))
        else:
            ms[a] = -value(*after(a, me, opp), depth - 1)
    return ms


def first_max(ms: list[int]) -> int:
    best = max(ms)
    return -1 if best == NONE else ms.index(best)


def ties(ms: list[int]) -> list[int]:
    best = max(ms)
    return [] if best == NONE else [a for a, s in enumerate(ms) if s == best]
