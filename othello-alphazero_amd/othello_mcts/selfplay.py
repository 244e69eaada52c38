"""Self-play training data from the on-device driver.

``BatchedMCTS.selfplay_move(emit_targets=True)`` plays one move of every game on
the GPU and emits that move's 8-fold targets (mcts.cpp:63-112). ``SelfPlayCollector``
turns the stream of moves into the samples the reference's ``_self_play``
returns (train.py:404-452) once a game is over: per move, 8 feature tensors
``(1+2H, 8, 8)`` and 8 policy tensors ``(65,)``, and the value target of every
sample = the final outcome (+1 black wins / -1 white wins / 0 draw, by disc
count, train.py:438-445) from the perspective of the player to move at that
step. For a game from the initial position that is exactly the reference's
rule "+outcome for step 0, alternate sign every step, passes included"
(train.py:447-450): players alternate every step, passes included. Games that
start from a random opening get the same perspective rule, which the
alternating form would get wrong when white moves first.

The dict returned by ``add`` / ``drain`` has the reference's keys, so it feeds
``_AlphaZeroDataset`` unchanged:
    dataset.features += data["features"]; dataset.policies += data["policies"];
    dataset.values += data["values"]
"""

from __future__ import annotations

import torch

# BatchedMCTS.selfplay_move "finished" codes (csrc/selfplay.hip k_selfplay_move):
# bits 0-1 outcome of a game that ended with this move, bit 2 no targets were
# written (unexpanded root), bit 3 the game's node pool overflowed
FIN_NONE, FIN_DRAW, FIN_BLACK, FIN_WHITE = 0, 1, 2, 3
FIN_NO_TARGETS, FIN_OVERFLOW = 4, 8
# with adjudicate_empties > 0 (othello_mcts.adjudication): bit 5 the
# game was ended at this move by the exact solver (bits 0-1 carry its exact
# outcome), bit 6 the solver flagged the position (an error)
FIN_ADJUDICATED, FIN_SOLVER_FLAG = 32, 64
# with a playout cap (BatchedMCTS.set_playout_cap): bit 7 the move
# followed a fast search: it was played, but no targets were written for it
FIN_FAST = 128
_OUTCOME_BLACK = {FIN_DRAW: 0.0, FIN_BLACK: 1.0, FIN_WHITE: -1.0}


def outcome_for_black(player1_discs: int, player2_discs: int) -> float:
    """+1 / -1 / 0 by the final disc count (train.py:438-445)."""
    b, w = bin(player1_discs).count("1"), bin(player2_discs).count("1")
    return 1.0 if b > w else (-1.0 if b < w else 0.0)


def value_targets_from_outcome(black_to_move: list[bool], player1_discs: int, player2_discs: int) -> list[float]:
    """One value target per move (the reference repeats it for the move's 8
    samples): the final outcome from the perspective of the side to move at that
    step. From the initial position this is train.py:447-450's alternating rule."""
    v = outcome_for_black(player1_discs, player2_discs)
    return [v if b else -v for b in black_to_move]


class SelfPlayCollector:
    """Accumulates selfplay_move outputs per game; completed games become samples.

    ``device``: where returned sample tensors live ("cpu" like the reference's
    dataset, or a CUDA device to keep them in HBM)."""

    def __init__(self, num_games: int, device: str | torch.device = "cpu") -> None:
        self.num_games = num_games
        self.device = torch.device(device)
        self._moves: list[list[tuple[torch.Tensor, torch.Tensor]]] = [[] for _ in range(num_games)]
        self._ready = {"features": [], "policies": [], "values": []}
        self.games_completed = 0

    def add(self, out: dict[str, torch.Tensor]) -> dict[str, list[torch.Tensor]]:
        """Record one selfplay_move(emit_targets=True) result; return (and clear)
        the samples of every game that finished on this move."""
        if "features" not in out:
            raise ValueError("selfplay_move must be called with emit_targets=True")
        actions = out["actions"].to("cpu")
        finished = out["finished"].to("cpu")
        if actions.shape[0] != self.num_games:
            raise ValueError(f"expected {self.num_games} games, got {actions.shape[0]}")
        # the output buffers are reused by the next move: copy this move's targets
        feats = out["features"].to(self.device, copy=True)
        pols = out["policy"].to(self.device, copy=True)
        bad = (finished & FIN_OVERFLOW) != 0
        if bool(bad.any()):
            raise RuntimeError(f"node pool exhausted in game(s) {bad.nonzero().flatten().tolist()}: the search no "
                               "longer matches the reference; use a larger node_capacity")
        flagged = (finished & FIN_SOLVER_FLAG) != 0
        if bool(flagged.any()):
            raise RuntimeError(f"the exact solver flagged the adjudicated position of game(s) "
                               f"{flagged.nonzero().flatten().tolist()}")
        # a move after a fast search (playout cap) is played but not recorded;
        # the game's outcome still labels its recorded moves
        fast = (finished & FIN_FAST) != 0
        no_targets = (finished & FIN_NO_TARGETS) != 0
        if bool((no_targets & (actions >= 0) & ~fast).any()):
            # the reference's self_play_data raises here (mcts.cpp:69-71)
            raise ValueError("The root node has not been expanded yet.")
        for g in range(self.num_games):
            if int(actions[g]) >= 0 and not bool(fast[g]):  # a searched, expanded root: targets were written
                self._moves[g].append((feats[g], pols[g]))
            fin = int(finished[g]) & 3
            if fin != FIN_NONE:
                self._finish(g, _OUTCOME_BLACK[fin])
        return self.drain()

    def _finish(self, g: int, outcome_black: float) -> None:
        for f8, p8 in self._moves[g]:
            # plane 0 = player - 1: 0 when black is to move (transformation.h:83-116)
            black_to_move = bool(f8[0, 0, 0, 0] == 0)
            v = outcome_black if black_to_move else -outcome_black
            for t in range(8):
                self._ready["features"].append(f8[t])
                self._ready["policies"].append(p8[t])
                self._ready["values"].append(torch.tensor(v, dtype=torch.float32, device=self.device))
        self._moves[g] = []
        self.games_completed += 1

    def drain(self) -> dict[str, list[torch.Tensor]]:
        out = self._ready
        self._ready = {"features": [], "policies": [], "values": []}
        return out

    def pending_moves(self, game: int) -> int:
        return len(self._moves[game])


def self_play(batched, neural_net, games: int, temperature_moves: int = 12, temperature: float = 1.0,
              opening_moves: int = 0, device: str | torch.device = "cpu",
              moves_per_call: int = 16, adjudicate_empties: int = 0,
              split: bool = False, playout_cap: tuple[float, int] | None = None,
              sim_budget: int = 0, forced_playouts: float | None = None,
              exact_leaves: int | None = None) -> dict[str, list[torch.Tensor]]:
    """Play until at least ``games`` games have completed across the batch (each
    slot restarts when its game ends) and return their samples in the
    reference's ``_self_play`` format (train.py:404-452). ``opening_moves=0``
    starts every game from the initial position as train.py does.

    With a native net (NativeNet, or a module ``search`` would convert) the
    moves run ``moves_per_call`` at a time through
    ``BatchedMCTS.selfplay_steps`` (free-running games, one enqueue per call:
    the bench's throughput path); per game the moves are those of the
    move-by-move loop (search + selfplay_move), which any other evaluator
    uses, so the samples of the games completed by a given move are the same
    either way. The last call may play up to ``moves_per_call - 1`` moves past
    the one that completed the requested games (their finished games are
    returned too).

    adjudicate_empties = K > 0: a game ends with the searched move that leaves
    at most K empties, with the exact result of that position as its outcome
    (othello_mcts.adjudication; ``split``: the split solver). The samples then
    hold no position with K or fewer empties except the first searched move
    after a restart whose opening already went that far.

    playout_cap = (full_probability, fast_simulations): sets the engine's
    playout cap for this run (``BatchedMCTS.set_playout_cap``; None leaves the
    engine as it is). Moves after fast searches are played but yield no
    samples. sim_budget = S > 0 (native net, moves_per_call > 1): every call
    gives each game S nominal simulations instead of ``moves_per_call`` moves
    (``BatchedMCTS.selfplay_steps``); ``moves_per_call`` is then the slot count,
    the most moves of a game per call.

    forced_playouts = k: sets the engine's forced playouts with policy target
    pruning for this run (``BatchedMCTS.set_forced_playouts(k)``, DESIGN.md §18;
    None leaves the engine as it is). The policy samples are then the pruned
    targets; nothing else about the samples changes.

    exact_leaves = E: sets the engine's exact leaf values for this run
    (``BatchedMCTS.set_exact_leaves(E)``; None leaves the engine
    as it is). The engine must hold no tree built under another value (a fresh
    engine, or one whose games were all reset)."""
    from .adjudication import check_adjudicate_empties
    from .native import resolve

    check_adjudicate_empties(adjudicate_empties)
    if playout_cap is not None:
        batched.set_playout_cap(*playout_cap)
    if forced_playouts is not None:
        batched.set_forced_playouts(forced_playouts)
    if exact_leaves is not None:
        batched.set_exact_leaves(exact_leaves)
    sim_budget = int(sim_budget)
    if sim_budget < 0:
        raise ValueError(f"Expected sim_budget >= 0, but got {sim_budget}.")

    col = SelfPlayCollector(batched.num_games, device=device)
    data = {"features": [], "policies": [], "values": []}
    native = moves_per_call > 1 and resolve(neural_net, batched.device.index, batched.config.history_size) is not None
    if sim_budget > 0 and not native:
        raise ValueError("sim_budget needs a native net and moves_per_call > 1 (the free-running call).")
    kw = dict(temperature_moves=temperature_moves, temperature=temperature, opening_moves=opening_moves,
              emit_targets=True)
    if adjudicate_empties:
        kw.update(adjudicate_empties=adjudicate_empties, split=split)
    while col.games_completed < games:
        if native:
            out = batched.selfplay_steps(neural_net, moves_per_call, keep_all=True, sim_budget=sim_budget, **kw)
            moves = [{k: v[i] for k, v in out.items()} for i in range(moves_per_call)]
        else:
            batched.search(neural_net)
            moves = [batched.selfplay_move(**kw)]
        for o in moves:
            got = col.add(o)
            for k in data:
                data[k] += got[k]
    return data


__all__ = ["SelfPlayCollector", "self_play", "outcome_for_black", "value_targets_from_outcome",
           "FIN_NO_TARGETS", "FIN_OVERFLOW", "FIN_NONE", "FIN_DRAW", "FIN_BLACK", "FIN_WHITE", "FIN_ADJUDICATED",
           "FIN_SOLVER_FLAG", "FIN_FAST"]
