"""Adjudication of running games by the exact endgame solver.

The rule, one for self-play and the arena: after a *searched* move has been
applied, a new root that is not terminal and has at most K =
``adjudicate_empties`` empty squares ends the game there (a mover that must
pass still counts). The root is solved exactly; ``margin`` is the score seen
from black (the solver's score for the mover, negated when white is to move)
and the outcome code is that of a finished game: 2 black won (margin > 0),
3 white won (margin < 0), 1 draw. K = 0 is off.

The device applies it inside ``BatchedMCTS.selfplay_move`` /
``selfplay_steps`` and ``Arena.move`` / ``Arena.play``; ``adjudicate`` is the
same rule on the host, for one position, built on ``solve_position``.
"""

from __future__ import annotations

from .endgame import MAX_EMPTIES, _fields, solve_position

FIN_ADJUDICATED = 32  # finished bit 5: the game was adjudicated at this move
FIN_SOLVER_FLAG = 64  # finished bit 6: the solver flagged the position (never for an engine position)
MARGIN_NONE = -(1 << 31)  # margin of a slot in which no game ended
_NO_LIMIT = (1 << 56) - 1  # with at most 16 empties the solver always finishes


def check_adjudicate_empties(adjudicate_empties, n_moves: int = 1, keep_all: bool = True) -> int:
    """Validate K (and the multi-move form) before anything touches a device."""
    k = adjudicate_empties
    if isinstance(k, bool) or not isinstance(k, int):
        raise TypeError(f"Expected an int for adjudicate_empties, but got {type(k).__name__}.")
    if not 0 <= k <= MAX_EMPTIES:
        raise ValueError(f"Expected 0 <= adjudicate_empties <= {MAX_EMPTIES}, but got {k}.")
    if k > 0 and n_moves > 1 and not keep_all:
        raise ValueError("adjudicate_empties > 0 with n_moves > 1 needs keep_all=True: every move keeps the "
                         "position of the games it adjudicates until the call's resolve step")
    return k


def adjudicate(position, max_empties: int, split: bool = False):
    """``(code, margin)`` of a root the rule adjudicates at K = ``max_empties``,
    ``None`` when it does not apply (K = 0, a terminal position, or more than K
    empties). position: a ``Position`` or ``(player, player1_discs,
    player2_discs)``. Host only."""
    k = check_adjudicate_empties(max_empties)
    player, p1, p2 = _fields(position)
    if k == 0 or 64 - bin(p1 | p2).count("1") > k:
        return None
    s = solve_position((player, p1, p2), k, _NO_LIMIT, split=split)
    if s["flags"]:
        raise ValueError(f"adjudicate: the solver flagged the position (flags {s['flags']})")
    if s["best_action"] < 0:  # neither side can move: the game is over on the board
        return None
    margin = -s["score"] if player == 2 else s["score"]
    return (2 if margin > 0 else (3 if margin < 0 else 1)), margin


__all__ = ["adjudicate", "check_adjudicate_empties", "FIN_ADJUDICATED", "FIN_SOLVER_FLAG", "MARGIN_NONE"]
