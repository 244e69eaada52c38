"""Search from given positions.

``BatchedMCTS.set_positions`` puts any position, with up to 15 of the positions
before it, at the root of a game; ``BatchedMCTS.principal_variations`` reads the
most visited line below every searched root on the device. ``analyze`` is the
front end over both: n positions through an engine of G games, chunk by chunk,
each position with a random-stream key of its own, so that what it reports for
a position does not depend on G or on the other positions. ``parse_board`` /
``format_board`` read and write the common 64-character board string, and
``canonical_position`` is the form the engine stores (the rule of
``csrc/positions.h``, the same code on the host).
"""

from __future__ import annotations

from dataclasses import dataclass

import torch

from ._othello_mcts_impl import Position, _canonical_position
from .endgame import _fields, _signed

MAX_HISTORY = 15
_MASK64 = (1 << 64) - 1

# status codes of oamd_engine_set_positions (include/othello_mcts_amd.h)
_FAULTS = {
    1: "player outside {0, 1, 2}",
    2: "the two disc sets overlap",
    3: "a history entry's player is outside {0, 1, 2}",
    4: "a history entry's disc sets overlap",
    5: "hist_len outside 0..K",
    6: "ply < 0",
    7: "the node pool cannot hold the history",
}


def set_positions_fault(code: int) -> str:
    return _FAULTS.get(code, f"status {code}")


def canonical_position(position) -> Position:
    """The canonical ``Position`` of a ``Position`` or a ``(player,
    player1_discs, player2_discs)`` triple, from those three fields alone: the
    legal moves as ``apply_action`` would have left them, a side to move without
    a move passing (``legal_actions() == [64]``) when the opponent has one, and
    the position terminal (player 0) when neither side has. ValueError for a
    player outside 0..2 or overlapping disc sets."""
    player, p1, p2 = _fields(position)
    if not -(1 << 31) <= player < 1 << 31:
        raise ValueError(f"Expected player in {{0, 1, 2}}, but got {player}.")
    return _canonical_position(player, p1, p2)


# ------------------------------------------------------------- board strings
_BLACK, _WHITE, _EMPTY = "X*", "O", "-."


def parse_board(text: str) -> Position:
    """A canonical ``Position`` from a board string: 64 squares a1, b1, ... h8
    (``X`` or ``*`` black, ``O`` white, ``-`` or ``.`` empty) and then the side to
    move (``X`` / ``*`` or ``O``); whitespace anywhere is ignored, letters may be
    lower case. ValueError for anything else."""
    if not isinstance(text, str):
        raise TypeError(f"Expected a board string, but got {type(text).__name__}.")
    s = "".join(text.split()).upper()
    if len(s) != 65:
        raise ValueError(f"Expected 64 squares and a side to move, but got {len(s)} characters.")
    p1 = p2 = 0
    for i, c in enumerate(s[:64]):
        if c in _BLACK:
            p1 |= 1 << (63 - i)
        elif c in _WHITE:
            p2 |= 1 << (63 - i)
        elif c not in _EMPTY:
            raise ValueError(f"Unexpected character {c!r} at square {i}.")
    if s[64] in _BLACK:
        player = 1
    elif s[64] in _WHITE:
        player = 2
    else:
        raise ValueError(f"Expected the side to move (X or O), but got {s[64]!r}.")
    return _canonical_position(player, p1, p2)


def format_board(position) -> str:
    """The board string of a position: 64 of ``X`` / ``O`` / ``-``, a space and
    the side to move. ``parse_board`` is its inverse on canonical positions (a
    terminal position is written with ``X`` to move and parses back terminal)."""
    player, p1, p2 = _fields(position)
    sq = "".join("X" if (p1 >> (63 - i)) & 1 else ("O" if (p2 >> (63 - i)) & 1 else "-") for i in range(64))
    return sq + " " + ("O" if player == 2 else "X")


# ------------------------------------------------------------------- packing
def pack_position_rows(positions) -> torch.Tensor:
    """(n, 5) int64 CPU rows in ``oamd_position`` layout from such a tensor or a
    sequence of positions / triples (``endgame.pack_positions``)."""
    if isinstance(positions, torch.Tensor):
        if positions.dim() != 2 or positions.shape[1] != 5 or positions.dtype != torch.int64:
            raise ValueError(f"Expected positions as an (n, 5) int64 tensor, but got {positions.dtype} of shape "
                             f"{tuple(positions.shape)}.")
        return positions.detach().to("cpu").contiguous()
    rows = []
    for p in positions:
        player, p1, p2 = _fields(p)
        rows.append([player & 0xFFFFFFFF, _signed(p1), _signed(p2), 0, 0])
    return torch.tensor(rows, dtype=torch.int64).reshape(len(rows), 5)


def pack_history(history, n: int) -> tuple[torch.Tensor, torch.Tensor]:
    """((n, K, 5) int64 rows, (n) int32 lengths) of the positions before each of
    n roots, newest first: from an (n, K, 5) tensor (every length K) or a list
    of per-position lists of unequal length (K = the longest)."""
    if isinstance(history, torch.Tensor):
        if history.dim() != 3 or history.shape[0] != n or history.shape[2] != 5 or history.dtype != torch.int64:
            raise ValueError(f"Expected history as an ({n}, K, 5) int64 tensor, but got {history.dtype} of shape "
                             f"{tuple(history.shape)}.")
        K = history.shape[1]
        if K > MAX_HISTORY:
            raise ValueError(f"Expected at most {MAX_HISTORY} history positions, but got {K}.")
        return history.detach().to("cpu").contiguous(), torch.full((n,), K, dtype=torch.int32)
    history = list(history)
    if len(history) != n:
        raise ValueError(f"Expected {n} history lists, but got {len(history)}.")
    lens = [len(h) for h in history]
    K = max(lens, default=0)
    if K > MAX_HISTORY:
        raise ValueError(f"Expected at most {MAX_HISTORY} history positions, but got {K}.")
    out = torch.zeros((n, K, 5), dtype=torch.int64)
    for i, h in enumerate(history):
        if lens[i]:
            out[i, : lens[i]] = pack_position_rows(h)
    return out, torch.tensor(lens, dtype=torch.int32)


# ---------------------------------------------------------------------- keys
def _mix64(z: int) -> int:
    z &= _MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def position_key(seed: int, index: int) -> int:
    """The random-stream key ``analyze`` gives input position ``index``: the key
    of game ``index`` of an engine reset with ``seed`` (csrc/rng.h mix64), so it
    depends on neither the engine's size nor the position's chunk."""
    return _mix64((int(seed) & _MASK64) ^ _mix64(int(index) + 0x632BE59BD9B4E019))


# ------------------------------------------------------------------ analysis
@dataclass
class Analysis:
    """Per input position (CPU tensors, n rows): ``visits`` (n, 65) int32 and
    ``q`` (n, 65) fp32 of the root's children by action; ``value`` (n) fp32,
    the root's mean value for the side to move: the visit-weighted mean of its
    children's Q (the engine keeps Q on the edges, each for the player who moves
    along it; a root has no edge of its own), 0 without visits; ``best_action``
    (n) int32, the most visited action, the lowest on ties, -1 for a terminal
    input or an unsearched root; ``pv`` (n, pv_len) int32 padded with -1,
    ``pv_visits``, ``pv_q`` and ``pv_len`` (n): the principal variation, whose
    first action is ``best_action``; ``terminal`` (n) bool and ``margin`` (n)
    int32: black's discs minus white's of a terminal input, 0 elsewhere."""

    visits: torch.Tensor
    q: torch.Tensor
    value: torch.Tensor
    best_action: torch.Tensor
    pv: torch.Tensor
    pv_visits: torch.Tensor
    pv_q: torch.Tensor
    pv_len: torch.Tensor
    terminal: torch.Tensor
    margin: torch.Tensor

    def __len__(self) -> int:
        return self.visits.shape[0]

    def records(self) -> list[dict]:
        """One plain dict per position, ready for ``json.dumps``."""
        out = []
        for i in range(len(self)):
            k = int(self.pv_len[i])
            rec = {"terminal": bool(self.terminal[i]), "best_action": int(self.best_action[i]),
                   "value": float(self.value[i]), "visits": int(self.visits[i].sum()),
                   "children": [{"action": a, "visits": int(self.visits[i, a]), "q": float(self.q[i, a])}
                                for a in range(65) if int(self.visits[i, a]) > 0],
                   "pv": [int(a) for a in self.pv[i, :k]], "pv_visits": [int(v) for v in self.pv_visits[i, :k]],
                   "pv_q": [float(v) for v in self.pv_q[i, :k]]}
            if rec["terminal"]:
                rec["margin"] = int(self.margin[i])
            out.append(rec)
        return out


def empty_analysis(n: int, pv_len: int) -> Analysis:
    return Analysis(torch.zeros((n, 65), dtype=torch.int32), torch.zeros((n, 65), dtype=torch.float32),
                    torch.zeros(n, dtype=torch.float32), torch.full((n,), -1, dtype=torch.int32),
                    torch.full((n, pv_len), -1, dtype=torch.int32), torch.zeros((n, pv_len), dtype=torch.int32),
                    torch.zeros((n, pv_len), dtype=torch.float32), torch.zeros(n, dtype=torch.int32),
                    torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.int32))


def fill_rows(a: Analysis, rows, visits: torch.Tensor, q: torch.Tensor, pv: dict) -> None:
    """Write the engine's read-outs of m games (``root_stats`` and
    ``principal_variations`` rows, any device) into rows ``rows`` of ``a``."""
    idx = torch.as_tensor(list(rows), dtype=torch.int64)
    v = visits.detach().to("cpu", torch.int32)
    qq = q.detach().to("cpu", torch.float32)
    a.visits[idx] = v
    a.q[idx] = qq
    total = v.sum(1)
    mean = (v.to(torch.float64) * qq.to(torch.float64)).sum(1) / total.clamp(min=1).to(torch.float64)
    a.value[idx] = torch.where(total > 0, mean, torch.zeros_like(mean)).to(torch.float32)
    # the first (lowest) action holding the maximum
    best = torch.argmax((v == v.max(1, keepdim=True).values).to(torch.int32), dim=1).to(torch.int32)
    a.best_action[idx] = torch.where(total > 0, best, torch.full_like(best, -1))
    a.pv[idx] = pv["actions"].detach().to("cpu", torch.int32)
    a.pv_visits[idx] = pv["visits"].detach().to("cpu", torch.int32)
    a.pv_q[idx] = pv["q"].detach().to("cpu", torch.float32)
    a.pv_len[idx] = pv["length"].detach().to("cpu", torch.int32)


def analyze(positions, neural_net, *, history=None, num_simulations: int = 800, num_games: int = 256,
            num_threads: int = 2, batch_size: int = 16, pv_len: int = 16, seed: int = 0, mcts=None,
            **search_config) -> Analysis:
    """Search n given positions with ``neural_net`` (a ``NativeNet``, or whatever
    ``BatchedMCTS.search`` takes) and report, per position, the root's visit
    counts and Q by action, its value, the most visited action and the
    principal variation (``Analysis``).

    The positions go through an engine of G games in ceil(n / G) chunks:
    ``set_positions``, ``search``, ``root_stats``, ``principal_variations``.
    ``mcts``: the ``BatchedMCTS`` to use (its configuration stands and the
    search arguments here are ignored); its games are overwritten and nothing is
    restored. Otherwise an engine of ``min(num_games, n)`` games is created from
    the arguments and ``search_config`` (``BatchedMCTS`` keywords;
    ``history_size`` defaults to the net's), with root noise off
    (``dirichlet_epsilon = 0``) unless ``search_config`` sets it.

    ``history``: per position the positions before it, newest first (a list of
    lists, or an (n, K, 5) tensor), K <= 15. Position i searches with the
    random-stream key ``position_key(seed, i)``, so its result depends on
    neither G, nor its chunk, nor the other positions. Terminal inputs (after
    ``canonical_position``) are not searched: ``terminal`` is set, there are no
    visits, ``best_action`` is -1 and ``margin`` holds the final disc margin."""
    from .batched import BatchedMCTS

    pv_len = int(pv_len)
    if not 1 <= pv_len <= 64:
        raise ValueError(f"Expected 1 <= pv_len <= 64, but got {pv_len}.")
    rows = pack_position_rows(positions)
    n = rows.shape[0]
    if history is not None:
        hist, hist_len = pack_history(history, n)
    out = empty_analysis(n, pv_len)
    live = []
    for i in range(n):
        player = int(rows[i, 0]) & 0xFFFFFFFF
        player = player - (1 << 32) if player >= 1 << 31 else player
        c = canonical_position((player, int(rows[i, 1]) & _MASK64, int(rows[i, 2]) & _MASK64))
        if c.is_terminal():
            out.terminal[i] = True
            out.margin[i] = bin(c.player1_discs()).count("1") - bin(c.player2_discs()).count("1")
        else:
            live.append(i)
    if not live:
        return out
    if mcts is None:
        cfg = dict(search_config)
        cfg.setdefault("dirichlet_epsilon", 0.0)
        if "history_size" not in cfg:
            h = getattr(neural_net, "history_size", None)
            cfg["history_size"] = int(h) if isinstance(h, int) else 8
        mcts = BatchedMCTS(max(1, min(int(num_games), len(live))), num_simulations=num_simulations,
                           num_threads=num_threads, batch_size=batch_size, **cfg)
    elif search_config:
        raise ValueError(f"search_config {sorted(search_config)} cannot be applied to a given engine.")
    G = mcts.num_games
    for c0 in range(0, len(live), G):
        chunk = live[c0:c0 + G]
        m = len(chunk)
        ci = torch.tensor(chunk, dtype=torch.int64)
        h = None
        if history is not None:
            h = [hist[i, : int(hist_len[i])] for i in chunk]
        mcts.set_positions(rows[ci], history=h, keys=[position_key(seed, i) for i in chunk], games=range(m))
        # a full chunk set (and so activated) every game
        if m < G:
            mcts.set_active([g < m for g in range(G)])
        mcts.search(neural_net)
        v, q = mcts.root_stats()
        pv = mcts.principal_variations(pv_len)
        fill_rows(out, chunk, v[:m], q[:m], {k: t[:m] for k, t in pv.items()})
    return out


__all__ = ["Analysis", "analyze", "canonical_position", "parse_board", "format_board", "position_key",
           "pack_position_rows", "pack_history", "fill_rows", "empty_analysis", "set_positions_fault", "MAX_HISTORY"]
