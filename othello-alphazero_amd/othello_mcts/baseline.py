"""Baseline opponents: fixed classical players for the whole
game, on the device (csrc/baseline.hip) and on the host (the same code,
csrc/baseline.h), and ``Gauntlet``: G matches of one net against one of them.

They stand in for the reference's ``RandomPlayer``, ``GreedyPlayer`` and
``EgaroucidPlayer`` (player.py:121-175, 262-321) as opponents that do not move
from one training run to the next. A baseline gives every root action of a
position (0..63, or 64 when the mover must pass) one int32 score and picks an
action with the maximal score:

``RANDOM``   every action scores 0.
``GREEDY``   a square scores the discs it flips, the pass 0.
``SEARCH``   the exact negamax value ``depth`` (1..10) disc placements deep; a
             pass consumes no depth. A finished game is worth ``4096 * sgn(d) +
             d`` (``terminal_value``), a position at depth 0 ``10 * mobility +
             50 * corners - 20 * X-squares beside an empty corner + discs``,
             each as mover minus other side. With ``depth >=`` the empties the
             scores are ``terminal_value`` of the exact solver's.

Every other ``move_scores`` entry is ``NONE`` (INT32_MIN). The pick is the
lowest action among the tied best ones, or with a key the k-th lowest, ``k =
min(nt - 1, int(u * nt))`` with ``u`` the first uniform of the random stream
``(key, event, 0)``: the argmax rule of the self-play move. A root where
neither side can move has no action (-1), as has a flagged position
(``FLAG_INVALID``, ``FLAG_NODE_LIMIT``). ``nodes`` counts positions visited plus
static evaluations (0 for ``RANDOM`` and ``GREEDY``).

There is no transposition table and the evaluation is a fixed hand-written
one: ``search-D`` is an anchor for Elo scales, not a strong engine.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from ._othello_mcts_impl import _baseline_workspace_bytes, _gpu_baseline, _host_baseline
from .arena import UNFINISHED, ArenaResult, paired_openings
from .batched import BatchedMCTS
from .endgame import DEFAULT_NODE_LIMIT, FLAG_INVALID, FLAG_NODE_LIMIT, _fields, pack_positions

NONE = -(1 << 31)
RANDOM, GREEDY, SEARCH = 0, 1, 2
MAX_DEPTH = 10
_KIND_NAMES = {"random": RANDOM, "greedy": GREEDY, "search": SEARCH}


def terminal_value(discs: int) -> int:
    """The search's value of a finished game with disc difference ``discs``."""
    return 4096 * ((discs > 0) - (discs < 0)) + discs


def _check_kind(kind, depth, node_limit) -> int:
    if isinstance(kind, str):
        if kind not in _KIND_NAMES:
            raise ValueError(f"Expected a baseline kind of {sorted(_KIND_NAMES)}, but got {kind!r}.")
        kind = _KIND_NAMES[kind]
    for name, v in (("kind", kind), ("depth", depth), ("node_limit", node_limit)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"Expected an int for {name}, but got {type(v).__name__}.")
    if kind not in (RANDOM, GREEDY, SEARCH):
        raise ValueError(f"Expected a baseline kind in 0..2, but got {kind}.")
    if kind == SEARCH and not 1 <= depth <= MAX_DEPTH:
        raise ValueError(f"Expected 1 <= depth <= {MAX_DEPTH}, but got {depth}.")
    if not 1 <= node_limit < 1 << 56:
        raise ValueError(f"Expected 1 <= node_limit < 2^56, but got {node_limit}.")
    return kind


def baseline_name(kind, depth: int = 1) -> str:
    """The identity string of a baseline in game records: ``"random"``,
    ``"greedy"`` or ``"search-D"``."""
    kind = _check_kind(kind, depth, 1)
    return ("random", "greedy", f"search-{depth}")[kind]


def baseline_move(position, kind, depth: int = 1, key: int | None = None, event: int = 0,
                  node_limit: int = DEFAULT_NODE_LIMIT) -> dict:
    """The host baseline for one ``Position`` (or ``(player, player1_discs,
    player2_discs)``); needs no GPU. Returns ``move_scores`` (65 ints),
    ``score``, ``action``, ``flags`` and ``nodes``. ``key`` / ``event``: the
    random stream of the tie-break (ints below 2^64); no key: the lowest tied
    action."""
    kind = _check_kind(kind, depth, node_limit)
    for name, v in (("key", 0 if key is None else key), ("event", event)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"Expected an int for {name}, but got {type(v).__name__}.")
        if not -(1 << 63) <= v < 1 << 64:
            raise ValueError(f"Expected {name} as a 64-bit int, but got {v}.")
    player, p1, p2 = _fields(position)
    if not -(1 << 31) <= player < 1 << 31:
        raise ValueError(f"Expected player as an int32, but got {player}.")
    mask = (1 << 64) - 1
    ms, score, action, flags, nodes = _host_baseline(player, p1, p2, kind, depth, node_limit, key is not None,
                                                     (key or 0) & mask, event & mask)
    return {"move_scores": ms, "score": score, "action": action, "flags": flags, "nodes": nodes}


@dataclass
class BaselineMoves:
    """Device tensors of ``baseline_moves``: ``move_scores`` (n, 65) int32,
    ``score``, ``action``, ``flags`` (n) int32, ``nodes`` (n) int64."""

    move_scores: torch.Tensor
    score: torch.Tensor
    action: torch.Tensor
    flags: torch.Tensor
    nodes: torch.Tensor


def _per_position(t, n: int, device, name: str):
    if t is None:
        return None
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"Expected {name} as a tensor or None, but got {type(t).__name__}.")
    if t.dtype != torch.int64 or t.shape != (n,):
        raise ValueError(f"Expected {name} as an ({n},) int64 tensor, but got {t.dtype} of shape {tuple(t.shape)}.")
    if t.device != device:
        raise ValueError(f"Expected {name} on {device}, but got '{t.device}'.")
    return t.contiguous()


def baseline_moves(positions, kind, depth: int = 1, keys=None, events=None, node_limit: int = DEFAULT_NODE_LIMIT,
                   _workgroups: int = 0) -> BaselineMoves:
    """The baseline's scores and pick for n positions on the GPU. ``positions``:
    an ``(n, 5)`` int64 device tensor in ``oamd_position`` layout
    (``BatchedMCTS.root_positions()``), or a sequence of ``Position`` objects /
    triples, packed and uploaded to the current device. ``keys`` / ``events``:
    (n) int64 device tensors or None (no keys: the lowest tied action; keys
    without events: event 0). Enqueued on the current torch stream; nothing
    waits on the host. ``_workgroups`` (tests): that many 64-lane workgroups
    instead of the chip-filling grid; no output depends on it."""
    kind = _check_kind(kind, depth, node_limit)
    if isinstance(positions, torch.Tensor):
        pos = positions
        if pos.dim() != 2 or pos.shape[1] != 5 or pos.dtype != torch.int64:
            raise ValueError(f"Expected positions as an (n, 5) int64 tensor, but got {pos.dtype} of shape "
                             f"{tuple(pos.shape)}.")
        if pos.device.type != "cuda":
            raise ValueError(f"baseline_moves runs on a ROCm GPU, but positions are on '{pos.device}'; "
                             "baseline_move is the host baseline.")
        pos = pos.contiguous()
    else:
        if not torch.cuda.is_available():
            raise RuntimeError("baseline_moves needs a ROCm GPU; baseline_move is the host baseline.")
        pos = pack_positions(positions).to(torch.device("cuda", torch.cuda.current_device()))
    if isinstance(_workgroups, bool) or not isinstance(_workgroups, int) or _workgroups < 0:
        raise ValueError(f"Expected _workgroups >= 0, but got {_workgroups!r}.")
    d, n = pos.device, pos.shape[0]
    keys = _per_position(keys, n, d, "keys")
    events = _per_position(events, n, d, "events")
    if events is not None and keys is None:
        raise ValueError("Expected keys with events (events alone select nothing).")
    out = BaselineMoves(torch.empty((n, 65), dtype=torch.int32, device=d),
                        torch.empty((n,), dtype=torch.int32, device=d),
                        torch.empty((n,), dtype=torch.int32, device=d),
                        torch.empty((n,), dtype=torch.int32, device=d),
                        torch.empty((n,), dtype=torch.int64, device=d))
    if n == 0:
        return out
    ws = torch.empty((_baseline_workspace_bytes(n),), dtype=torch.uint8, device=d)
    _gpu_baseline(d.index, pos.data_ptr(), n, kind, depth, node_limit,
                  0 if keys is None else keys.data_ptr(), 0 if events is None else events.data_ptr(),
                  out.move_scores.data_ptr(), out.score.data_ptr(), out.action.data_ptr(), out.flags.data_ptr(),
                  out.nodes.data_ptr(), ws.data_ptr(), _workgroups, torch.cuda.current_stream(d).cuda_stream)
    # the caching allocator hands a freed block to later work of the same stream only
    return out


def gauntlet_key(seed: int, game: int) -> int:
    """The random stream key of the baseline's tie-breaks in match ``game`` of
    a gauntlet seeded ``seed`` (splitmix64 of the pair), below 2^63."""
    z = (seed * 0x9E3779B97F4A7C15 + game + 1) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return (z ^ (z >> 31)) >> 1


def _s64(x: int) -> int:
    return x - (1 << 64) if x >= 1 << 63 else x


def _lsr(x: torch.Tensor, s: int) -> torch.Tensor:
    return (x >> s) & ((1 << (64 - s)) - 1)


def _mix64(z: torch.Tensor) -> torch.Tensor:
    z = (z ^ _lsr(z, 30)) * _s64(0xBF58476D1CE4E5B9)
    z = (z ^ _lsr(z, 27)) * _s64(0x94D049BB133111EB)
    return z ^ _lsr(z, 31)


def stream_uniform(keys: torch.Tensor, events: torch.Tensor) -> torch.Tensor:
    """csrc/rng.h ``uniform(stream_key(key, event, 0), 0)`` over int64 tensors
    (two's complement, wrapping): float32 in (0, 1)."""
    golden = _s64(0x9E3779B97F4A7C15)
    sk = _mix64(_mix64(keys ^ (events * _s64(0xD1B54A32D192ED03))) + golden)
    m = _lsr(_mix64(sk + golden), 41)
    return (2 * m + 1).to(torch.float32) * 5.9604644775390625e-08


def pick_actions(scores: torch.Tensor, legal: torch.Tensor, keys: torch.Tensor, events: torch.Tensor) -> torch.Tensor:
    """The pick rule of ``baseline_move`` over (G, 65) integer ``scores``
    restricted to the (G, 65) bool ``legal``: (G) int32 actions, -1 for a row
    without a legal action. Tensor operations only, no host wait."""
    sc = scores.to(torch.int64)
    low = torch.full_like(sc, -(1 << 62))
    masked = torch.where(legal, sc, low)
    ties = legal & (masked == masked.max(1, keepdim=True).values)
    nt = ties.sum(1)
    u = stream_uniform(keys, events)
    k = torch.minimum((u * nt.to(torch.float32)).to(torch.int64), nt - 1).clamp(min=0)
    rank = ties.to(torch.int64).cumsum(1) - 1
    hit = ties & (rank == k.unsqueeze(1))
    action = hit.to(torch.int64).argmax(1)
    return torch.where(nt > 0, action, torch.full_like(action, -1)).to(torch.int32)


class Gauntlet:
    """G matches of one net, searched in ``mcts``, against a baseline.

    Per ply the matches whose mover is the net are searched (the others are
    masked out with ``set_active``); the net plays the argmax of its root
    visits, the baseline its pick, ties of both broken by the stream ``(key_g,
    ply)`` with ``key_g = gauntlet_key(seed, g)`` and the pick rule of
    ``baseline_move``; one ``apply_actions`` call moves every tree, so the
    net reuses its subtree across the baseline's moves. There is no
    temperature sampling. ``ply`` counts from 0 at the first move after the
    opening."""

    def __init__(self, mcts: BatchedMCTS, kind, depth: int = 1, seed: int = 0) -> None:
        self.kind = _check_kind(kind, depth, DEFAULT_NODE_LIMIT)
        self.depth = depth
        if isinstance(seed, bool) or not isinstance(seed, int):
            raise TypeError(f"Expected an int for seed, but got {type(seed).__name__}.")
        self.mcts = mcts
        self.seed = seed
        self._reject_settings()
        self.num_games = mcts.num_games
        self.device = mcts.device
        G = self.num_games
        self.keys = torch.tensor([gauntlet_key(seed, g) for g in range(G)], dtype=torch.int64, device=self.device)
        self.net_is_white = torch.zeros(G, dtype=torch.bool)
        self._net_colour = torch.ones(G, dtype=torch.int64, device=self.device)  # 1 black, 2 white
        self._ply = torch.zeros(G, dtype=torch.int64, device=self.device)
        self._flags = torch.zeros(G, dtype=torch.int32, device=self.device)  # baseline flags seen since reset
        self._square_bit = (torch.ones(64, dtype=torch.int64, device=self.device)
                            << (63 - torch.arange(64, device=self.device)))
        self.opening_plies = 0
        self._begun = False
        self.time_baseline = False  # record a device event pair around every baseline_moves call
        self._events: list = []

    def baseline_ms(self) -> float:
        """Device time of the baseline_moves calls since reset() while
        ``time_baseline`` was set (waits for the recorded events)."""
        total = 0.0
        for e0, e1 in self._events:
            e1.synchronize()
            total += e0.elapsed_time(e1)
        return total

    @property
    def baseline_id(self) -> str:
        return baseline_name(self.kind, self.depth)

    def _reject_settings(self) -> None:
        """Matches are played by the plain search without root noise, as the
        arena's are."""
        m = self.mcts
        if getattr(m, "exact_leaves", 0):
            raise ValueError("gauntlet: the engine has exact leaves set (the gauntlet does not use them)")
        if getattr(m, "playout_cap", None) is not None:
            raise ValueError("gauntlet: the engine has a playout cap set (the gauntlet does not use it)")
        if getattr(m, "forced_playouts", None) is not None:
            raise ValueError("gauntlet: the engine has forced playouts set (the gauntlet does not use them)")
        if m.config.dirichlet_epsilon != 0:
            raise ValueError(f"gauntlet: the engine draws root noise (dirichlet_epsilon = "
                             f"{m.config.dirichlet_epsilon}); create it with dirichlet_epsilon=0")

    def reset(self, openings=None, net_is_white=None) -> None:
        """Start G new matches. openings: (G, plies) actions, -1 padded
        (default: 4-ply paired_openings of this gauntlet's seed); net_is_white:
        (G) bools (default: the odd matches)."""
        G = self.num_games
        if openings is None:
            openings = paired_openings(G, 4, self.seed)
        op = np.asarray(openings, dtype=np.int32)
        op = np.ascontiguousarray(op.reshape(G, -1) if op.size else op.reshape(G, 0))
        if net_is_white is None:
            net_is_white = np.arange(G) % 2 == 1
        white = np.ascontiguousarray(np.asarray(net_is_white)).astype(bool).reshape(G)
        from . import Position

        for g in range(G):  # the device plays the plies unchecked
            p = Position.initial_position()
            ended = False
            for a in op[g].tolist():
                if a < 0:
                    ended = True
                    continue
                if ended:
                    raise ValueError(f"opening of match {g}: an action follows the -1 padding")
                p = p.apply_action(int(a))  # raises on an illegal action, as the reference does
        self._reject_settings()
        self.mcts.reset(seed=self.seed)
        op_dev = torch.from_numpy(op).to(self.device)
        for k in range(op.shape[1]):
            self.mcts.apply_actions(op_dev[:, k].contiguous())
        self.net_is_white = torch.from_numpy(white.copy())
        self._net_colour = torch.from_numpy(np.where(white, 2, 1)).to(self.device, torch.int64)
        self._ply.zero_()
        self._flags.zero_()
        self._events = []
        self.opening_plies = op.shape[1]
        self._begun = True

    def move(self, net) -> dict[str, torch.Tensor]:
        """One ply of every running match (device tensors; enqueued only with a
        native net): ``actions`` (G) int32, -1 once a match is over;
        ``net_moved`` (G) bool; ``finished`` (G) bool, the match is over after
        this ply; ``visits`` (G, 65) int32, the root visits by action that the
        net's picks were made from."""
        if not self._begun:
            raise RuntimeError("Gauntlet.move before Gauntlet.reset")
        self._reject_settings()
        m = self.mcts
        roots = m.root_positions()
        player = roots[:, 0] & 0xFFFFFFFF
        running = player != 0
        net_moves = running & (player == self._net_colour)
        m.set_active(net_moves)
        m.search(net, sync=False)  # a native net's search is only enqueued
        m.set_active(None)
        visits, _ = m.root_stats()
        # the root's legal actions: its squares, or the pass when it has none
        legal_sq = (roots[:, 3:4] & self._square_bit.unsqueeze(0)) != 0
        legal = torch.cat([legal_sq, ~legal_sq.any(1, keepdim=True)], 1) & running.unsqueeze(1)
        if self.time_baseline:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        base = baseline_moves(roots, self.kind, self.depth, self.keys, self._ply)
        if self.time_baseline:
            e1.record()
            self._events.append((e0, e1))
        self._flags |= base.flags
        net_action = pick_actions(visits, legal, self.keys, self._ply)
        actions = torch.where(net_moves, net_action, base.action)
        actions = torch.where(running, actions, torch.full_like(actions, -1))
        m.apply_actions(actions)
        self._ply += running.to(torch.int64)
        after = m.root_positions()
        finished = (after[:, 0] & 0xFFFFFFFF) == 0
        return {"actions": actions, "net_moved": net_moves, "finished": finished, "visits": visits}

    def play(self, net, max_plies: int = 128) -> ArenaResult:
        """Play the matches begun by reset() (called here if it was not) to the
        end, at most ``max_plies`` plies; the count of running matches is read
        back every 4 plies. Returns an ``ArenaResult`` whose ``a_is_white``
        means "the net is white": ``records(id_net, gauntlet.baseline_id)``,
        ``wdl()``, ``score_a()`` and ``margin_a()`` are the net's. Raises
        RuntimeError when a node pool overflowed."""
        if not self._begun:
            self.reset()
        G = self.num_games
        rows = []
        done = False
        while len(rows) < max_plies and not done:
            out = self.move(net)
            rows.append(out["actions"].clone())
            if len(rows) % 4 == 0 or len(rows) == max_plies:
                done = bool(out["finished"].all())
        self.mcts.check_health()
        flagged = torch.nonzero(self._flags).flatten().tolist()
        if flagged:
            raise RuntimeError(f"gauntlet: the baseline flagged the root of match(es) {flagged} (flags "
                               f"{self._flags[flagged].tolist()}: {FLAG_NODE_LIMIT} = node limit, {FLAG_INVALID} = "
                               "invalid position)")
        actions = torch.stack(rows).cpu() if rows else torch.empty((0, G), dtype=torch.int32)
        n = actions.shape[0]
        while n > 0 and bool((actions[n - 1] < 0).all()):
            n -= 1
        actions = actions[:n]
        roots = self.mcts.root_positions().cpu()
        over = (roots[:, 0] & 0xFFFFFFFF) == 0
        discs = torch.tensor([[bin(int(r[1]) & (1 << 64) - 1).count("1"), bin(int(r[2]) & (1 << 64) - 1).count("1")]
                              for r in roots.tolist()], dtype=torch.int64).reshape(G, 2)
        diff = discs[:, 0] - discs[:, 1]
        result = torch.where(over, torch.where(diff > 0, 1, torch.where(diff < 0, 2, 0)),
                             torch.full_like(diff, UNFINISHED))
        margin = torch.where(over, diff, torch.zeros_like(diff))
        self._begun = False
        return ArenaResult(actions=actions, result=result, a_is_white=self.net_is_white.clone(), discs=discs,
                           plies=n, margin=margin)


__all__ = ["BaselineMoves", "Gauntlet", "baseline_move", "baseline_moves", "baseline_name", "gauntlet_key",
           "pick_actions", "stream_uniform", "terminal_value", "NONE", "RANDOM", "GREEDY", "SEARCH", "MAX_DEPTH", "FLAG_NODE_LIMIT", "FLAG_INVALID",
           "DEFAULT_NODE_LIMIT"]
