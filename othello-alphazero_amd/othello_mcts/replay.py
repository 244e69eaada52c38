"""Packed on-device replay buffer.

``SampleBuffer`` keeps every position as 8 fp32 samples (36,928 bytes at
H = 8) and waits on the host several times per move. ``ReplayBuffer`` keeps the
position itself: 2H bitboards, the side to move, the transform-0 policy and the
value, 16H + 265 bytes (393 at H = 8). The 8 board symmetries are produced when
a minibatch is drawn (``gather``), and ``add`` only enqueues two kernels per
move (csrc/replay.hip): no host read anywhere in the self-play loop.

Sample id ``s`` in ``[0, 8 * size)`` is position ``s >> 3`` under transform
``s & 7``; positions are counted from the oldest live one. An unwrapped
``ReplayBuffer`` of P positions therefore gives the rows of a ``SampleBuffer``
of 8P samples, and a wrapped one gives that buffer's rows rotated to the
oldest-first order.

The storage is plain torch tensors on the engine's device (structure of
arrays), so a checkpoint is ``state_dict()``.

``track_exact=True`` adds one byte per slot (``exact``) and
``relabel_endgames``: the positions with few empties get the exact result of
perfect play (csrc/solver.hip) as their value target instead of the outcome of
the game they came from. Off by default, and then nothing here
behaves, stores or serialises differently.
"""

from __future__ import annotations

import torch

from ._othello_mcts_impl import _relabel_split_workspace_bytes, _relabel_workspace_bytes, _ReplayView
from .endgame import DEFAULT_NODE_LIMIT, _check_limits

# sticky bits of the device counter block (include/othello_mcts_amd.h OAMD_REPLAY_*)
FLAG_OVERFLOW, FLAG_NO_TARGETS, FLAG_TOO_LONG, FLAG_BAD_ID = 1, 2, 4, 8
FLAG_SOLVER = 16  # an adjudicated game whose position the exact solver flagged (finished bit 6)

# codes of the ``exact`` ring (include/othello_mcts_amd.h OAMD_REPLAY_EXACT_*); -64..64 is an exact score
EXACT_UNKNOWN, EXACT_GAVE_UP = -128, -127
MAX_BUDGET = 1 << 20
_POLICY_MODES = {"keep": 0, "optimal": 1}

_RING = ("boards", "policy", "value", "player")
_EXACT = ("exact", "relabel_counters")
_STAGE = ("stage_boards", "stage_policy", "stage_player", "moves")
_DIMS = ("num_games", "history_size", "capacity", "max_moves")


def _check_relabel(max_empties, budget, node_limit, policy, retry) -> None:
    _check_limits(max_empties, node_limit)
    if isinstance(budget, bool) or not isinstance(budget, int):
        raise TypeError(f"Expected an int for budget, but got {type(budget).__name__}.")
    if not isinstance(policy, str):
        raise TypeError(f"Expected a str for policy, but got {type(policy).__name__}.")
    if not isinstance(retry, bool):
        raise TypeError(f"Expected a bool for retry, but got {type(retry).__name__}.")
    if not 1 <= budget <= MAX_BUDGET:
        raise ValueError(f"Expected 1 <= budget <= {MAX_BUDGET}, but got {budget}.")
    if policy not in _POLICY_MODES:
        raise ValueError(f"Expected policy 'keep' or 'optimal', but got {policy!r}.")


def _validate(num_games, history_size, capacity, max_moves) -> None:
    for name, v in (("num_games", num_games), ("history_size", history_size), ("capacity", capacity),
                    ("max_moves", max_moves)):
        if isinstance(v, bool) or not isinstance(v, int):
            raise TypeError(f"Expected an int for {name}, but got {type(v).__name__}.")
    if num_games < 1:
        raise ValueError(f"Expected num_games >= 1, but got {num_games}.")
    if not 1 <= history_size <= 15:
        raise ValueError(f"Expected 1 <= history_size <= 15, but got {history_size}.")
    if capacity < 1:
        raise ValueError(f"Expected capacity >= 1, but got {capacity}.")
    if max_moves < 1:
        raise ValueError(f"Expected max_moves >= 1, but got {max_moves}.")
    if num_games * max_moves >= 1 << 31:
        raise ValueError(f"Expected num_games * max_moves < 2^31, but got {num_games * max_moves}.")


class ReplayBuffer:
    """Ring of ``capacity`` positions fed by the on-device self-play driver.

    ``add(out)`` takes what ``BatchedMCTS.selfplay_move(emit_targets=True)`` or
    ``selfplay_steps(..., emit_targets=True)`` returned (one move, or the stacked
    ``keep_all=True`` moves) and only enqueues work. A game's moves wait in a
    staging area until the game finishes; then they get their value targets
    (``SampleBuffer``'s rule) and move into the ring in ascending game order,
    the oldest positions overwritten. Rows the kernels refuse set sticky flags;
    ``check()`` raises them with ``SampleBuffer``'s messages.
    A move played after a fast search of a playout cap (``FIN_FAST`` in
    ``finished``, ``BatchedMCTS.set_playout_cap``) carries no targets: it is
    skipped, without a flag, and the game's outcome labels its other moves.

    ``track_exact=True``: the ring also keeps ``exact`` (``capacity`` int8:
    ``EXACT_UNKNOWN``, ``EXACT_GAVE_UP`` or the exact disc difference for the
    side to move) and ``relabel_counters``, and ``relabel_endgames`` works."""

    def __init__(self, num_games: int, history_size: int, capacity: int, max_moves: int = 128,
                 device: torch.device | str | None = None, track_exact: bool = False) -> None:
        _validate(num_games, history_size, capacity, max_moves)
        if not isinstance(track_exact, bool):
            raise TypeError(f"Expected a bool for track_exact, but got {type(track_exact).__name__}.")
        if track_exact and capacity >= 1 << 31:
            raise ValueError(f"Expected capacity < 2^31 with track_exact, but got {capacity}.")
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device())
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError(f"ReplayBuffer lives on a ROCm GPU (its kernels run there), but got device '{device}'.")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        self.num_games, self.history_size = num_games, history_size
        self.capacity, self.max_moves = capacity, max_moves
        self.C = 1 + 2 * history_size
        G, H2, M, d = num_games, 2 * history_size, max_moves, device
        # uint64 bitboards, square i = bit 63 - i (allocated through int64: same bytes)
        self.boards = torch.zeros((capacity, H2), dtype=torch.int64, device=d).view(torch.uint64)
        self.policy = torch.zeros((capacity, 65), dtype=torch.float32, device=d)
        self.value = torch.zeros((capacity,), dtype=torch.float32, device=d)
        self.player = torch.zeros((capacity,), dtype=torch.uint8, device=d)
        self.stage_boards = torch.zeros((G, M, H2), dtype=torch.int64, device=d).view(torch.uint64)
        self.stage_policy = torch.zeros((G, M, 65), dtype=torch.float32, device=d)
        self.stage_player = torch.zeros((G, M), dtype=torch.uint8, device=d)
        self.moves = torch.zeros((G,), dtype=torch.int32, device=d)
        self._pending = torch.zeros((G,), dtype=torch.int32, device=d)
        # head, size, games_completed, sticky flags
        self.counters = torch.zeros((4,), dtype=torch.int64, device=d)
        self.track_exact = track_exact
        if track_exact:
            self.exact = torch.full((capacity,), EXACT_UNKNOWN, dtype=torch.int8, device=d)
            # labelled so far, given up so far, left behind by the last call, taken by the last call
            self.relabel_counters = torch.zeros((4,), dtype=torch.int64, device=d)
            self._relabel_ws: dict[int, torch.Tensor] = {}  # workspace per budget
            self._relabel_split_ws: dict[int, torch.Tensor] = {}  # the split solver's, per budget

    # ------------------------------------------------------------------ plumbing
    def _view(self) -> _ReplayView:
        return _ReplayView(self.device.index, self.num_games, self.history_size, self.max_moves, self.capacity,
                           self.boards.data_ptr(), self.policy.data_ptr(), self.value.data_ptr(),
                           self.player.data_ptr(), self.stage_boards.data_ptr(), self.stage_policy.data_ptr(),
                           self.stage_player.data_ptr(), self.moves.data_ptr(), self._pending.data_ptr(),
                           self.counters.data_ptr())

    def _stream(self) -> int:
        return torch.cuda.current_stream(self.device).cuda_stream

    def _input(self, out: dict, key: str, dtype: torch.dtype, tail: tuple, lead: tuple) -> torch.Tensor:
        t = out[key]
        if t.device != self.device or t.dtype != dtype:
            raise ValueError(f"Expected out['{key}'] as {dtype} on {self.device}, but got {t.dtype} on {t.device}.")
        if tuple(t.shape) != lead + tail:
            raise ValueError(f"Expected out['{key}'] of shape {lead + tail}, but got {tuple(t.shape)}.")
        return t.contiguous()

    # ------------------------------------------------------------------ feeding
    def add(self, out: dict[str, torch.Tensor]) -> None:
        """Stage one move of every game, or the ``n`` stacked moves of
        ``selfplay_steps(..., keep_all=True)`` in order. Enqueues only."""
        if "features" not in out:
            raise ValueError("selfplay_move must be called with emit_targets=True")
        G = self.num_games
        a = out["actions"]
        lead = (a.shape[0],) if a.dim() == 2 else ()  # stacked moves of selfplay_steps(keep_all=True)
        actions = self._input(out, "actions", torch.int32, (G,), lead)
        finished = self._input(out, "finished", torch.int32, (G,), lead)
        features = self._input(out, "features", torch.float32, (G, 8, self.C, 8, 8), lead)
        policy = self._input(out, "policy", torch.float32, (G, 8, 65), lead)
        n = lead[0] if lead else 1
        if self.track_exact:
            self._view().add_tracked(self.exact.data_ptr(), n, actions.data_ptr(), finished.data_ptr(),
                                     features.data_ptr(), policy.data_ptr(), self._stream())
        else:
            self._view().add(n, actions.data_ptr(), finished.data_ptr(), features.data_ptr(), policy.data_ptr(),
                             self._stream())

    # ------------------------------------------------------------------ exact endgame targets
    def relabel_endgames(self, max_empties: int = 10, budget: int = 4096, node_limit: int = DEFAULT_NODE_LIMIT,
                         policy: str = "keep", retry: bool = False, split: bool = False) -> None:
        """Give the live positions with at most ``max_empties`` empties their
        exact value target: the sign of the result of perfect play for the side
        to move, from ``solve_endgames``' kernels. Oldest first, at most
        ``budget`` positions per call; a position is examined once (again with
        ``retry`` if the solver gave up on it: ``node_limit``, an invalid
        record). ``policy="optimal"`` also replaces the policy row by the
        uniform distribution over the optimal actions. ``split``: solve with the
        split solver (``solve_endgames(split=True)``; ``node_limit`` is then a
        budget per item). Enqueues only."""
        _check_relabel(max_empties, budget, node_limit, policy, retry)
        if not self.track_exact:
            raise RuntimeError("ReplayBuffer.relabel_endgames needs a buffer created with track_exact=True.")
        cache, workspace_bytes = (self._relabel_split_ws, _relabel_split_workspace_bytes) if split else \
            (self._relabel_ws, _relabel_workspace_bytes)
        ws = cache.get(budget)
        if ws is None:
            ws = torch.empty((workspace_bytes(budget),), dtype=torch.uint8, device=self.device)
            cache[budget] = ws
        view = self._view()
        relabel = view.relabel_split if split else view.relabel
        relabel(self.exact.data_ptr(), self.relabel_counters.data_ptr(), max_empties, budget, node_limit,
                _POLICY_MODES[policy], retry, ws.data_ptr(), self._stream())

    @property
    def relabel_stats(self) -> dict[str, int]:
        """``relabel_counters`` as a dict (waits for the stream): positions
        ``solved`` and ``gave_up`` so far, candidates the last call ``left``
        behind for lack of budget and candidates it ``taken``."""
        if not self.track_exact:
            raise RuntimeError("ReplayBuffer.relabel_stats needs a buffer created with track_exact=True.")
        return dict(zip(("solved", "gave_up", "left", "taken"), self.relabel_counters.tolist()))

    def exact_scores(self) -> torch.Tensor:
        """``exact`` of the live positions, oldest first (a device tensor of
        ``size`` int8; reading the size waits for the stream)."""
        if not self.track_exact:
            raise RuntimeError("ReplayBuffer.exact_scores needs a buffer created with track_exact=True.")
        size, head = self._counters()[:2]
        slots = (head - size + torch.arange(size, device=self.device)) % self.capacity
        return self.exact[slots]

    # ------------------------------------------------------------------ counters
    def _counters(self) -> tuple[int, int, int, int]:
        return self._view().counters(self._stream())

    @property
    def size(self) -> int:
        """Live positions (waits for the stream); ``8 * size`` samples."""
        return self._counters()[0]

    @property
    def head(self) -> int:
        """Ring slot the next position is written to (waits for the stream)."""
        return self._counters()[1]

    @property
    def games_completed(self) -> int:
        """Games committed to the ring so far (waits for the stream)."""
        return self._counters()[2]

    @property
    def nbytes(self) -> int:
        """Device bytes: capacity * (16H + 265) for the ring plus the staging
        area, G * max_moves * (16H + 261) + 8G + 32 (records without the value,
        the per-game move counts and commit scratch, the counter block)."""
        H = self.history_size
        staging = self.num_games * self.max_moves * (16 * H + 261) + 8 * self.num_games + 32
        exact = self.capacity + 32 if self.track_exact else 0  # one byte per slot, the relabel counters
        return self.capacity * (16 * H + 265) + staging + exact

    def check(self) -> None:
        """Raise what the kernels flagged since the buffer was created (waits
        for the stream). The flags are sticky: the buffer stays in error."""
        flags = self._counters()[3]
        if flags & FLAG_OVERFLOW:
            raise RuntimeError("node pool exhausted: the search no longer matches the reference; "
                               "use a larger node_capacity")
        if flags & FLAG_NO_TARGETS:
            raise ValueError("The root node has not been expanded yet.")
        if flags & FLAG_TOO_LONG:
            raise RuntimeError("a game exceeded ReplayBuffer.max_moves")
        if flags & FLAG_SOLVER:
            raise RuntimeError("the exact solver flagged the position of an adjudicated game")
        if flags & FLAG_BAD_ID:
            raise IndexError("ReplayBuffer.gather: a sample id outside [0, 8 * size)")

    # ------------------------------------------------------------------ drawing
    def gather(self, ids: torch.Tensor, out: tuple[torch.Tensor, torch.Tensor, torch.Tensor] | None = None
               ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """(features (n, C, 8, 8), policy (n, 65), value (n,)) fp32 of the
        sample ids (any integer tensor, moved to the device as int64). A bad id
        gives a zero row and an IndexError from ``check()``. ``out``: three
        contiguous fp32 tensors of those shapes to write into."""
        ids = torch.as_tensor(ids)
        if ids.dim() != 1 or ids.dtype.is_floating_point or ids.dtype == torch.bool:
            raise ValueError(f"Expected a 1-D integer tensor of sample ids, but got {ids.dtype} of shape "
                             f"{tuple(ids.shape)}.")
        ids = ids.to(self.device, torch.int64).contiguous()
        n = ids.shape[0]
        shapes = ((n, self.C, 8, 8), (n, 65), (n,))
        if out is None:
            out = tuple(torch.empty(s, dtype=torch.float32, device=self.device) for s in shapes)
        else:
            for t, s in zip(out, shapes):
                if tuple(t.shape) != s or t.dtype != torch.float32 or t.device != self.device or \
                        not t.is_contiguous():
                    raise ValueError(f"Expected a contiguous float32 output of shape {s} on {self.device}.")
        f, p, v = out
        self._view().gather(ids.data_ptr(), n, f.data_ptr(), p.data_ptr(), v.data_ptr(), self._stream())
        return f, p, v

    def sample(self, batch_size: int, generator: torch.Generator | None = None
               ) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``batch_size`` samples drawn uniformly (with replacement) from the
        ``8 * size`` live ones. The ids are drawn on the device against the
        device's own size counter: no host read. An empty buffer gives zero
        rows and an IndexError from ``check()``."""
        if batch_size < 0:
            raise ValueError(f"Expected batch_size >= 0, but got {batch_size}.")
        gen_dev = self.device if generator is None else generator.device
        u = torch.rand((batch_size,), dtype=torch.float64, device=gen_dev, generator=generator).to(self.device)
        n = 8 * self.counters[1]
        ids = torch.minimum((u * n).to(torch.int64), n - 1)
        return self.gather(ids)

    # ------------------------------------------------------------------ persistence
    def state_dict(self) -> dict:
        """CPU copies of the ring, the staging area and the counters, and the
        dimensions (waits for the stream)."""
        sd = {k: getattr(self, k).cpu() for k in self._tensors()}
        sd.update({k: getattr(self, k) for k in _DIMS})
        return sd

    def _tensors(self) -> tuple[str, ...]:
        return _RING + _STAGE + ("counters",) + (_EXACT if self.track_exact else ())

    def load_state_dict(self, sd: dict) -> None:
        for k in _DIMS:
            if k not in sd or int(sd[k]) != getattr(self, k):
                raise ValueError(f"ReplayBuffer.load_state_dict: {k} is {sd.get(k)!r} in the state, but "
                                 f"{getattr(self, k)} in this buffer.")
        for k in _EXACT:
            if (k in sd) != self.track_exact:
                raise ValueError(f"ReplayBuffer.load_state_dict: the state {'has' if k in sd else 'lacks'} {k}, but "
                                 f"this buffer was created with track_exact={self.track_exact}.")
        for k in self._tensors():
            dst = getattr(self, k)
            src = sd[k]
            if tuple(src.shape) != tuple(dst.shape) or src.dtype != dst.dtype:
                raise ValueError(f"ReplayBuffer.load_state_dict: expected {k} as {dst.dtype} of shape "
                                 f"{tuple(dst.shape)}, but got {src.dtype} of shape {tuple(src.shape)}.")
        # the kernels index with these: refuse values outside the ring / the staging area
        head, size = (int(x) for x in sd["counters"][:2])
        if not (0 <= head < self.capacity and 0 <= size <= self.capacity):
            raise ValueError(f"ReplayBuffer.load_state_dict: head {head} / size {size} outside a ring of "
                             f"{self.capacity} positions.")
        if self.num_games and (int(sd["moves"].min()) < 0 or int(sd["moves"].max()) > self.max_moves):
            raise ValueError("ReplayBuffer.load_state_dict: a staged move count outside [0, max_moves].")
        if self.track_exact:
            e = sd["exact"].to(torch.int16)
            if bool(((e > EXACT_GAVE_UP) & ((e < -64) | (e > 64))).any()):
                raise ValueError("ReplayBuffer.load_state_dict: an exact code outside EXACT_UNKNOWN, EXACT_GAVE_UP "
                                 "and [-64, 64].")
            if int(sd["relabel_counters"].min()) < 0:
                raise ValueError("ReplayBuffer.load_state_dict: a negative relabel counter.")
        for k in self._tensors():
            getattr(self, k).copy_(sd[k])


__all__ = ["ReplayBuffer", "FLAG_OVERFLOW", "FLAG_NO_TARGETS", "FLAG_TOO_LONG", "FLAG_BAD_ID",
           "EXACT_UNKNOWN", "EXACT_GAVE_UP", "MAX_BUDGET"]
