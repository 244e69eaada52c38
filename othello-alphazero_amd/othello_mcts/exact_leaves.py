"""Exact leaf values: the rule of ``BatchedMCTS.set_exact_leaves``
on the host and the solve kernel's path on the device.

With ``max_empties = E`` a search never expands and never evaluates a node that
is not terminal, is not the root and has at most E empties: the node is solved
once with the endgame solver's state machine (csrc/solver.h) and every visit
backs up the sign of the exact result. ``exact_leaf_value`` is that sign for
one position, ``exact_leaf_values`` the same for many on the GPU.
"""

from __future__ import annotations

import torch

from ._othello_mcts_impl import _gpu_exact_leaves, _host_exact_leaf
from .endgame import NONE, _fields, pack_positions

MAX_EXACT_EMPTIES = 10


def check_exact_empties(max_empties, allow_off: bool = False) -> int:
    """E as an int in 1..10 (0..10 with ``allow_off``); TypeError / ValueError otherwise."""
    if isinstance(max_empties, bool) or not isinstance(max_empties, int):
        raise TypeError(f"Expected an int for max_empties, but got {type(max_empties).__name__}.")
    low = 0 if allow_off else 1
    if not low <= max_empties <= MAX_EXACT_EMPTIES:
        raise ValueError(f"Expected {low} <= max_empties <= {MAX_EXACT_EMPTIES}, but got {max_empties}.")
    return max_empties


def exact_leaf_value(position, max_empties: int, return_nodes: bool = False):
    """The rule on the host (no GPU): for a ``Position`` (or ``(player,
    player1_discs, player2_discs)``) that the search would make an exact leaf
    at ``max_empties`` (not terminal, at most that many empties), the sign of
    the exact disc difference for the side to move under best play: -1, 0 or
    +1. ``None`` for every other position. ``return_nodes``: ``(value, nodes)``
    with the positions the solve visited (every root action searched with the
    window [-1, 1]), the figure the engine's ``exact_leaf_counters`` sum."""
    e = check_exact_empties(max_empties)
    player, p1, p2 = _fields(position)
    if not 0 <= player <= 2:
        raise ValueError(f"Expected player in 0..2, but got {player}.")
    sign, nodes = _host_exact_leaf(player, p1, p2, e)
    value = None if sign == NONE else sign
    return (value, nodes) if return_nodes else value


def exact_leaf_values(positions, max_empties: int, return_nodes: bool = False):
    """The solve kernel's path over n positions on the GPU: an (n,) int32 device
    tensor of signs, ``NONE`` (-128) where ``exact_leaf_value`` gives None.
    ``positions`` as ``solve_endgames`` takes them. Enqueued on the current
    torch stream. ``return_nodes``: ``(signs, nodes)``, nodes (n,) int64."""
    e = check_exact_empties(max_empties)
    if isinstance(positions, torch.Tensor):
        pos = positions
        if pos.dim() != 2 or pos.shape[1] != 5 or pos.dtype != torch.int64:
            raise ValueError(f"Expected positions as an (n, 5) int64 tensor, but got {pos.dtype} of shape "
                             f"{tuple(pos.shape)}.")
        if pos.device.type != "cuda":
            raise ValueError(f"exact_leaf_values runs on a ROCm GPU, but positions are on '{pos.device}'; "
                             "exact_leaf_value is the host rule.")
        pos = pos.contiguous()
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("exact_leaf_values needs a ROCm GPU; exact_leaf_value is the host rule.")
        pos = pack_positions(positions).to(torch.device("cuda", torch.cuda.current_device()))
    d, n = pos.device, pos.shape[0]
    sign = torch.empty((n,), dtype=torch.int32, device=d)
    nodes = torch.empty((n,), dtype=torch.int64, device=d)
    if n:
        _gpu_exact_leaves(d.index, pos.data_ptr(), n, e, sign.data_ptr(), nodes.data_ptr(),
                          torch.cuda.current_stream(d).cuda_stream)
    return (sign, nodes) if return_nodes else sign


__all__ = ["exact_leaf_value", "exact_leaf_values", "check_exact_empties", "MAX_EXACT_EMPTIES"]
