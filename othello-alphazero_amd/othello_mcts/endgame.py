"""Exact endgame solver: the last plies of Othello solved by
brute force on bitboards, on the device (csrc/solver.hip) and on the host
(the same code, csrc/solver.h).

The game ends when neither side can move; the result is the plain disc
difference, mover minus opponent. ``move_scores[a]`` is the exact result for the
side to move after action ``a`` (0..63, or 64 when it must pass) and perfect play
by both sides, ``NONE`` (-128) for every other entry; ``score`` is their
maximum and ``best_action`` its first index. A position where neither side can
move is terminal: ``score`` = black minus white, ``best_action`` = -1.

It stands in for the external engine behind the reference's ``EgaroucidPlayer``
(player.py:262-321) as an absolute yardstick: ``endgame_move_loss`` says how
many discs a move gave away against perfect play.

``split=True`` selects the split solver: the work item is one
move of the position one ply below a root action, searched with fastest-first
move ordering, in two phases. Scores, ``best_action`` and flags are the same
wherever no node limit binds; ``nodes`` are fewer and counted per item (1 for
the position after the root action, 1 more when its mover passes, plus the
items), and ``node_limit`` is a budget per item.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Sequence

import torch

from ._othello_mcts_impl import (Position, _gpu_solve, _gpu_solve_split, _host_solve, _host_solve_split,
                                 _solve_split_workspace_bytes, _solve_workspace_bytes)

NONE = -128
# per-position flags (include/othello_mcts_amd.h OAMD_SOLVE_*)
FLAG_TOO_MANY_EMPTIES, FLAG_NODE_LIMIT, FLAG_INVALID = 1, 2, 4
MAX_EMPTIES = 16
# Budget per root action. The largest count seen over 256 random-play positions
# at 12 empties is 1,522,632 nodes (profiles/endgame/host_nodes.json): the
# smallest power of two at least 8 times that. 14 empties needs more (up to
# 25,226,377 seen): pass a node_limit with a larger max_empties.
DEFAULT_NODE_LIMIT = 1 << 24

_FLAG_NAMES = ((FLAG_TOO_MANY_EMPTIES, "more empties than max_empties"),
               (FLAG_NODE_LIMIT, "node_limit exceeded"),
               (FLAG_INVALID, "invalid position"))


def _check_limits(max_empties, node_limit) -> None:
    for name, v in (("max_empties", max_empties), ("node_limit", node_limit)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"Expected an int for {name}, but got {type(v).__name__}.")
    if not 0 <= max_empties <= MAX_EMPTIES:
        raise ValueError(f"Expected 0 <= max_empties <= {MAX_EMPTIES}, but got {max_empties}.")
    if not 1 <= node_limit < 1 << 56:
        raise ValueError(f"Expected 1 <= node_limit < 2^56, but got {node_limit}.")


def _fields(p) -> tuple[int, int, int]:
    """(player, player1_discs, player2_discs) of a Position or of such a triple."""
    if isinstance(p, Position):
        return p.player(), p.player1_discs(), p.player2_discs()
    try:
        player, p1, p2 = (int(x) for x in p)
    except (TypeError, ValueError):
        raise TypeError(f"Expected a Position or a (player, player1_discs, player2_discs) triple, but got "
                        f"{type(p).__name__}.") from None
    if not (0 <= p1 < 1 << 64 and 0 <= p2 < 1 << 64):
        raise ValueError("Expected disc sets in [0, 2^64).")
    return player, p1, p2


def _signed(x: int) -> int:
    return x - (1 << 64) if x >= 1 << 63 else x


def pack_positions(positions: Sequence) -> torch.Tensor:
    """(n, 5) int64 CPU tensor in ``oamd_position`` layout (player in the low
    half of word 0, the two disc sets, two unused words)."""
    rows = []
    for p in positions:
        player, p1, p2 = _fields(p)
        rows.append([player & 0xFFFFFFFF, _signed(p1), _signed(p2), 0, 0])
    return torch.tensor(rows, dtype=torch.int64).reshape(len(rows), 5)


def random_play_positions(empties: int, count: int, seed: int) -> list[Position]:
    """``count`` positions with exactly ``empties`` empty squares and a side to
    move, from seeded uniformly random play from the initial position (games
    that end before are dropped). Host only: benchmark and test input."""
    import random

    rng = random.Random(seed)
    out: list[Position] = []
    while len(out) < count:
        p = Position.initial_position()
        while not p.is_terminal() and 64 - bin(p.player1_discs() | p.player2_discs()).count("1") > empties:
            acts = p.legal_actions()
            p = p.apply_action(acts[rng.randrange(len(acts))])
        if not p.is_terminal():
            out.append(p)
    return out


def solve_position(position, max_empties: int = 12, node_limit: int = DEFAULT_NODE_LIMIT, split: bool = False) -> dict:
    """The host solver for one ``Position`` (or ``(player, player1_discs,
    player2_discs)``); needs no GPU. Returns ``move_scores`` (65 ints),
    ``score``, ``best_action``, ``flags`` and ``nodes``. ``split``: the split
    solver's host twin."""
    _check_limits(max_empties, node_limit)
    player, p1, p2 = _fields(position)
    if not -(1 << 31) <= player < 1 << 31:
        raise ValueError(f"Expected player as an int32, but got {player}.")
    ms, score, best, flags, nodes = (_host_solve_split if split else _host_solve)(player, p1, p2, max_empties,
                                                                                  node_limit)
    return {"move_scores": ms, "score": score, "best_action": best, "flags": flags, "nodes": nodes}


@dataclass
class EndgameSolution:
    """Device tensors of ``solve_endgames``: ``move_scores`` (n, 65) int32,
    ``score``, ``best_action``, ``flags`` (n) int32, ``nodes`` (n) int64."""

    move_scores: torch.Tensor
    score: torch.Tensor
    best_action: torch.Tensor
    flags: torch.Tensor
    nodes: torch.Tensor

    def check(self) -> None:
        """Raise if any position was flagged, with the count per flag (waits
        for the stream)."""
        f = self.flags
        if not bool((f != 0).any()):
            return
        parts = [f"{int((f & bit).ne(0).sum())} x {name}" for bit, name in _FLAG_NAMES if bool((f & bit).ne(0).any())]
        raise RuntimeError(f"solve_endgames: {int((f != 0).sum())} of {f.numel()} positions were not solved: "
                           + ", ".join(parts))


def solve_endgames(positions, max_empties: int = 12, node_limit: int = DEFAULT_NODE_LIMIT,
                   _workgroups: int = 0, split: bool = False) -> EndgameSolution:
    """Solve n positions on the GPU. ``positions``: an ``(n, 5)`` int64 device
    tensor in ``oamd_position`` layout (``BatchedMCTS.root_positions()``), or a
    sequence of ``Position`` objects / ``(player, player1_discs,
    player2_discs)`` triples, packed and uploaded to the current device.
    Enqueued on the current torch stream; nothing waits on the host.
    ``_workgroups`` (tests): that many 64-lane workgroups instead of the
    chip-filling grid; no output depends on it. ``split``: the split solver."""
    _check_limits(max_empties, node_limit)
    if isinstance(positions, torch.Tensor):
        pos = positions
        if pos.dim() != 2 or pos.shape[1] != 5 or pos.dtype != torch.int64:
            raise ValueError(f"Expected positions as an (n, 5) int64 tensor, but got {pos.dtype} of shape "
                             f"{tuple(pos.shape)}.")
        if pos.device.type != "cuda":
            raise ValueError(f"solve_endgames runs on a ROCm GPU, but positions are on '{pos.device}'; "
                             "solve_position is the host solver.")
        pos = pos.contiguous()
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("solve_endgames needs a ROCm GPU; solve_position is the host solver.")
        pos = pack_positions(positions).to(torch.device("cuda", torch.cuda.current_device()))
    if isinstance(_workgroups, bool) or not isinstance(_workgroups, int) or _workgroups < 0:
        raise ValueError(f"Expected _workgroups >= 0, but got {_workgroups!r}.")
    d, n = pos.device, pos.shape[0]
    sol = EndgameSolution(torch.empty((n, 65), dtype=torch.int32, device=d),
                          torch.empty((n,), dtype=torch.int32, device=d),
                          torch.empty((n,), dtype=torch.int32, device=d),
                          torch.empty((n,), dtype=torch.int32, device=d),
                          torch.empty((n,), dtype=torch.int64, device=d))
    if n == 0:
        return sol
    workspace_bytes, solve = (_solve_split_workspace_bytes, _gpu_solve_split) if split else \
        (_solve_workspace_bytes, _gpu_solve)
    ws = torch.empty((workspace_bytes(n),), dtype=torch.uint8, device=d)
    solve(d.index, pos.data_ptr(), n, max_empties, node_limit, sol.move_scores.data_ptr(), sol.score.data_ptr(),
          sol.best_action.data_ptr(), sol.flags.data_ptr(), sol.nodes.data_ptr(), ws.data_ptr(), _workgroups,
          torch.cuda.current_stream(d).cuda_stream)
    # the caching allocator hands a freed block to later work of the same stream only
    return sol


def endgame_move_loss(roots: torch.Tensor, actions: torch.Tensor, max_empties: int = 12,
                      node_limit: int = DEFAULT_NODE_LIMIT, solution: EndgameSolution | None = None,
                      split: bool = False) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """How far the moves ``actions`` (G) played from ``roots`` (G, 5) are from
    perfect play: ``(loss, wdl_kept, empties)``, device tensors of length G.
    ``loss = score - move_scores[action] >= 0`` discs given away, ``wdl_kept``
    = 1 where the move keeps the sign of the exact result, else 0. Both are -1
    where the root has more than ``max_empties`` empties, is terminal, was not
    solved, or ``action < 0``. ``solution``: the roots' solution if the caller
    has it already; otherwise the roots are solved here, by the split solver
    with ``split``. No host wait."""
    if solution is None:
        solution = solve_endgames(roots, max_empties, node_limit, split=split)
    d = roots.device
    a = actions.to(d, torch.int64).reshape(-1)
    if a.shape[0] != roots.shape[0]:
        raise ValueError(f"Expected {roots.shape[0]} actions, but got {a.shape[0]}.")
    # popcount of the occupied squares, byte by byte through a 256-entry table
    occupied = (roots[:, 1] | roots[:, 2]).contiguous().view(torch.uint8).reshape(-1, 8).to(torch.int64)
    table = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64, device=d)
    empties = 64 - table[occupied].sum(1)
    played = torch.gather(solution.move_scores.to(torch.int64), 1, a.clamp(0, 64).unsqueeze(1)).squeeze(1)
    score = solution.score.to(torch.int64)
    ok = (a >= 0) & (a <= 64) & (solution.flags == 0) & (solution.best_action >= 0) & (played != NONE)
    minus = torch.full_like(a, -1)
    loss = torch.where(ok, score - played, minus)
    wdl = torch.where(ok, (torch.sign(played) == torch.sign(score)).to(torch.int64), minus)
    return loss, wdl, empties


__all__ = ["EndgameSolution", "solve_endgames", "solve_position", "endgame_move_loss", "pack_positions",
           "random_play_positions", "NONE",
           "FLAG_TOO_MANY_EMPTIES", "FLAG_NODE_LIMIT", "FLAG_INVALID", "MAX_EMPTIES", "DEFAULT_NODE_LIMIT"]
