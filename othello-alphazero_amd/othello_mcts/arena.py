"""Batched arena: G head-to-head matches between two nets on one GPU.

The reference measures a new net against an old one with ``play_game``
(player.py:33-95) between two ``AlphaZeroPlayer`` objects (player.py:177-259),
one game at a time and in pairs with the colours swapped (evaluation.py:15-90).
``Arena`` plays G such matches at once: match g is game g of two
``BatchedMCTS`` engines, one tree per player. Per ply only the side to move
searches (with its own net); the chosen action moves both trees, so each side
reuses its subtree across its own and the opponent's moves, as the reference's
players do. A forced pass is an ordinary ply. Move choice is the argmax of the
root visits with a uniform random tie-break (player.py:250-256); the first
``temperature_moves`` plies after the opening may be sampled by temperature.

Deterministic nets without root noise would play nearly the same game G
times, so matches start from openings: matches 2i and 2i + 1 share opening i,
and in the odd one net A plays white.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .adjudication import MARGIN_NONE, check_adjudicate_empties
from .batched import BatchedMCTS
from .native import resolve
from .synthetic import _splitmix_stream

UNFINISHED = -1  # ArenaResult.result of a match still running when play() stopped

# bits of the per-match status word (include/othello_mcts_amd.h oamd_arena_move)
_OUTCOME = 3
_UNEXPANDED = 4
_OVERFLOW = 8
_DESYNC = 16
_ADJUDICATED = 32  # the match was ended by the exact solver (othello_mcts.adjudication)
_SOLVER_FLAG = 64


def paired_openings(num_games: int, plies: int, seed: int = 0, position_cls=None) -> np.ndarray:
    """(num_games, plies) int32 opening actions, -1 padded: opening i =
    ``plies`` uniformly random legal actions from the initial position (a
    splitmix64 stream seeded with (seed, i), as synthetic.random_opening_actions
    draws its plies), shared by matches 2i and 2i + 1."""
    if position_cls is None:
        from . import Position as position_cls  # noqa: N813
    out = np.full((num_games, max(plies, 0)), -1, dtype=np.int32)
    for i in range((num_games + 1) // 2):
        rng = _splitmix_stream((seed * 0x9E3779B97F4A7C15 + i) & 0xFFFFFFFFFFFFFFFF)
        p = position_cls.initial_position()
        for k in range(plies):
            if p.is_terminal():
                break
            legal = p.legal_actions()
            a = legal[next(rng) % len(legal)]
            out[2 * i:2 * i + 2, k] = a
            p = p.apply_action(a)
    return out


@dataclass
class ArenaResult:
    """Outcome of Arena.play (CPU tensors).

    actions (plies, G): the action of every ply after the opening, -1 once a
    match is over; result (G): play_game's return, 0 draw, 1 black won, 2 white
    won (UNFINISHED = -1: still running when play stopped); a_is_white (G) bool;
    discs (G, 2): black and white discs at the end (of an adjudicated match: at
    the adjudicated position); plies: plies played; margin (G): the final score
    seen from black, black minus white discs for a match that ended on the
    board, the exact result of the adjudicated position otherwise (0 for an
    unfinished match); adjudicated (G) bool."""

    actions: torch.Tensor
    result: torch.Tensor
    a_is_white: torch.Tensor
    discs: torch.Tensor
    plies: int
    margin: torch.Tensor = None
    adjudicated: torch.Tensor = None

    def __post_init__(self) -> None:
        if self.adjudicated is None:
            self.adjudicated = torch.zeros(self.result.shape, dtype=torch.bool)
        if self.margin is None:
            self.margin = torch.where(self.result >= 0, self.discs[:, 0] - self.discs[:, 1], 0).to(torch.int64)

    def wdl(self) -> tuple[int, int, int]:
        """(wins, draws, losses) of net A."""
        r = self.result
        a_colour = torch.where(self.a_is_white, 2, 1).to(r.dtype)
        done = r >= 0
        wins = int((done & (r == a_colour)).sum())
        draws = int((r == 0).sum())
        losses = int((done & (r != 0) & (r != a_colour)).sum())
        return wins, draws, losses

    def score_a(self) -> float:
        """(wins + draws / 2) of net A over all G matches."""
        w, d, _ = self.wdl()
        return (w + 0.5 * d) / max(1, self.result.numel())

    def records(self, id_a: str, id_b: str) -> list[dict]:
        """The game records evaluation.py:68-84 writes (player1 = black's id),
        one per finished match: input of the reference's estimate_elo / save_pgn."""
        out = []
        for r, w in zip(self.result.tolist(), self.a_is_white.tolist()):
            if r < 0:
                continue
            out.append({"player1": id_b if w else id_a, "player2": id_a if w else id_b, "result": int(r)})
        return out

    def margin_a(self) -> torch.Tensor:
        """(G) the margin seen from net A (0 for an unfinished match)."""
        return torch.where(self.a_is_white, -self.margin, self.margin)


def _result_from_status(status: torch.Tensor) -> torch.Tensor:
    """finished bits 0-1 (1 draw, 2 black, 3 white; 0 running) -> play_game's 0/1/2, UNFINISHED."""
    o = (status & _OUTCOME).to(torch.int64)
    return torch.where(o == 0, torch.full_like(o, UNFINISHED), o - 1)


class Arena:
    """G matches between net A (searched in ``mcts_a``) and net B (``mcts_b``)."""

    def __init__(self, mcts_a: BatchedMCTS, mcts_b: BatchedMCTS) -> None:
        if mcts_a.num_games != mcts_b.num_games:
            raise ValueError(f"Arena needs two engines with the same number of games, got {mcts_a.num_games} "
                             f"and {mcts_b.num_games}")
        if mcts_a.device != mcts_b.device:
            raise ValueError(f"Arena needs two engines on the same device, got {mcts_a.device} and {mcts_b.device}")
        if mcts_a is mcts_b:
            raise ValueError("Arena needs two different engines (one tree per player)")
        self.a, self.b = mcts_a, mcts_b
        self._reject_exact_leaves()
        self.num_games = mcts_a.num_games
        self.device = mcts_a.device
        G = self.num_games
        self._actions = torch.full((G,), -1, dtype=torch.int32, device=self.device)
        self._status = torch.zeros(G, dtype=torch.int32, device=self.device)
        self._discs = torch.zeros((G, 2), dtype=torch.int32, device=self.device)
        self._remaining = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._margin = torch.full((G,), MARGIN_NONE, dtype=torch.int32, device=self.device)
        self.a_is_white = torch.zeros(G, dtype=torch.bool)
        self.opening_plies = 0
        self.seed = 0
        self._begun = False

    @classmethod
    def create(cls, num_games: int, seed: int = 0, **search_kwargs) -> "Arena":
        """Two engines of ``num_games`` games without root noise, seeded
        ``seed`` (A) and ``seed + 1`` (B); search_kwargs as BatchedMCTS."""
        kw = dict(search_kwargs)
        kw["dirichlet_epsilon"] = 0.0
        arena = cls(BatchedMCTS(num_games, seed=seed, **kw), BatchedMCTS(num_games, seed=seed + 1, **kw))
        arena.seed = seed
        return arena

    def _reject_exact_leaves(self) -> None:
        """Matches are played by the plain search: an engine with exact leaf
        values set (BatchedMCTS.set_exact_leaves) is rejected, as
        the C layer rejects it (and a playout cap, and forced playouts)."""
        for name, m in (("A", self.a), ("B", self.b)):
            if getattr(m, "exact_leaves", 0):
                raise ValueError(f"arena: engine {name} has exact leaves set (the arena does not use them)")

    def _streams(self) -> None:
        self._reject_exact_leaves()
        self.a._stream()
        self.b._stream()

    def reset(self, openings=None, a_is_white=None) -> None:
        """Start G new matches. openings: (G, plies) actions, -1 padded
        (default: 4-ply paired_openings of this arena's seed); a_is_white: (G)
        bools (default: the odd matches)."""
        G = self.num_games
        if openings is None:
            openings = paired_openings(G, 4, self.seed)
        op = np.asarray(openings, dtype=np.int32)
        op = np.ascontiguousarray(op.reshape(G, -1) if op.size else op.reshape(G, 0))
        if a_is_white is None:
            a_is_white = np.arange(G) % 2 == 1
        white = np.ascontiguousarray(np.asarray(a_is_white)).astype(bool).reshape(G)
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
        self._streams()
        op_dev = torch.from_numpy(op).to(self.device)
        white_dev = torch.from_numpy(white.astype(np.uint8)).to(self.device)
        self.a.engine.arena_begin(self.b.engine, op_dev.data_ptr() if op.shape[1] else 0, op.shape[1],
                                  white_dev.data_ptr())
        self._actions.fill_(-1)
        self._status.zero_()
        self._discs.zero_()
        self._remaining.zero_()
        self._margin.fill_(MARGIN_NONE)
        self.a_is_white = torch.from_numpy(white.copy())
        self.opening_plies = op.shape[1]
        self._begun = True

    def search(self, net_a, net_b, sync: bool = True):
        """This ply's two searches: every match searches in the engine of its
        side to move only. Nets: NativeNet, eval-mode AlphaZeroNet or any
        callable evaluator (BatchedMCTS.search). Returns the two engines'
        (simulations, nn_rows), or None with sync=False and native nets."""
        ra = self.a.search(net_a, sync=sync)
        rb = self.b.search(net_b, sync=sync)
        return (ra, rb) if sync else None

    def move(self, temperature_moves: int = 0, temperature: float = 1.0, adjudicate_empties: int = 0,
             split: bool = False) -> dict[str, torch.Tensor]:
        """One ply of every match from the searched roots (device tensors,
        overwritten by the next call): actions (G), -1 once a match is over;
        finished (G): the cumulative status word of oamd_arena_move; discs (G, 2).
        adjudicate_empties = K > 0: a ply that leaves a non-terminal position
        with at most K empties ends the match with its exact result (bit 5 of
        finished; othello_mcts.adjudication), and ``margin`` (G, cumulative) is
        the final score seen from black of every match that has ended since
        reset(), MARGIN_NONE for the others."""
        k = check_adjudicate_empties(adjudicate_empties)
        if not self._begun:
            raise RuntimeError("Arena.move before Arena.reset")
        self._streams()
        if k == 0:
            self.a.engine.arena_move(self.b.engine, temperature_moves, temperature, self._actions.data_ptr(),
                                     self._status.data_ptr(), self._discs.data_ptr(), 0)
            return {"actions": self._actions, "finished": self._status, "discs": self._discs}
        self.a.engine.arena_move_adjudicated(self.b.engine, temperature_moves, temperature, self._actions.data_ptr(),
                                             self._status.data_ptr(), self._discs.data_ptr(), 0, k, bool(split),
                                             self._margin.data_ptr())
        return {"actions": self._actions, "finished": self._status, "discs": self._discs, "margin": self._margin}

    def _native(self, net, mcts):
        return resolve(net, self.device.index, mcts.config.history_size)

    def play(self, net_a, net_b, max_plies: int = 128, temperature_moves: int = 0,
             temperature: float = 1.0, adjudicate_empties: int = 0, split: bool = False) -> ArenaResult:
        """Play the matches begun by reset() (called here if it was not) to the
        end, at most ``max_plies`` plies: one fused call when both nets are
        native, the search / move loop otherwise. Matches still running after
        max_plies have result UNFINISHED. Raises RuntimeError when a node pool
        overflowed, a descent hit the depth cap or the two trees of a match
        disagree, naming the matches. adjudicate_empties / split: as move();
        the result's ``adjudicated`` and ``margin`` say which matches the solver
        ended and by how much."""
        k = check_adjudicate_empties(adjudicate_empties)
        if not self._begun:
            self.reset()
        G = self.num_games
        na, nb = self._native(net_a, self.a), self._native(net_b, self.b)
        if na is not None and nb is not None:
            self._streams()
            actions = torch.empty((max(0, max_plies), G), dtype=torch.int32, device=self.device)
            if k > 0:
                plies = self.a.engine.arena_play_adjudicated(na.handle, self.b.engine, nb.handle, temperature_moves,
                                                             temperature, max_plies, actions.data_ptr(),
                                                             self._status.data_ptr(), self._discs.data_ptr(), k,
                                                             bool(split), self._margin.data_ptr())
            else:
                plies = self.a.engine.arena_play(na.handle, self.b.engine, nb.handle, temperature_moves, temperature,
                                                 max_plies, actions.data_ptr(), self._status.data_ptr(),
                                                 self._discs.data_ptr())
            actions = actions[:plies]
            status = self._status.cpu()
        else:
            rows = []
            status = self._status.cpu()
            while len(rows) < max_plies and bool(((status & (_OUTCOME | _DESYNC | _SOLVER_FLAG)) == 0).any()):
                self.search(net_a, net_b)
                out = self.move(temperature_moves, temperature, k, split)
                rows.append(out["actions"].clone())
                status = out["finished"].cpu()
            actions = torch.stack(rows) if rows else torch.empty((0, G), dtype=torch.int32, device=self.device)
        # trailing plies in which no match moved (the fused call reads the count of running matches late)
        acts = actions.cpu()
        n = acts.shape[0]
        while n > 0 and bool((acts[n - 1] < 0).all()):
            n -= 1
        acts = acts[:n]
        self._raise_on_trouble(status)
        self._begun = False
        result = _result_from_status(status)
        discs = self._discs.cpu().to(torch.int64)
        adjudicated = (status & _ADJUDICATED) != 0
        margin = torch.where(result >= 0, discs[:, 0] - discs[:, 1], 0)
        if k > 0:
            margin = torch.where(adjudicated, self._margin.cpu().to(torch.int64), margin)
        return ArenaResult(actions=acts, result=result, a_is_white=self.a_is_white.clone(), discs=discs, plies=n,
                           margin=margin, adjudicated=adjudicated)

    def _raise_on_trouble(self, status: torch.Tensor) -> None:
        def games(bit):
            return torch.nonzero(status & bit).flatten().tolist()

        if games(_SOLVER_FLAG):
            raise RuntimeError(f"arena: the exact solver flagged the adjudicated position of match(es) "
                               f"{games(_SOLVER_FLAG)}")
        if games(_DESYNC):
            raise RuntimeError(f"arena: the two trees of match(es) {games(_DESYNC)} hold different positions")
        if games(_OVERFLOW):
            raise RuntimeError(f"arena: node pool exhausted in match(es) {games(_OVERFLOW)}; create the engines "
                               "with a larger node_capacity")
        for name, m in (("A", self.a), ("B", self.b)):
            try:
                m.check_health()
            except RuntimeError as e:
                bad = [g for g in range(self.num_games) if m.root_info(g)["overflow"]]
                raise RuntimeError(f"arena, engine {name}, match(es) {bad}: {e}") from None


__all__ = ["Arena", "ArenaResult", "paired_openings", "UNFINISHED"]
