"""Batched multi-game search: G independent games on one GPU.

The reference searches one game per ``MCTS`` object and plays games one after
another (train.py:394-398). ``BatchedMCTS`` keeps G game trees in HBM and
advances all of them with the same kernel launches (csrc/tree.hip), the NN
evaluating G * num_threads * batch_size leaves per launch. With G = 1 it is
the reference's single-game search; every game follows exactly the
single-game semantics (tested against the oracle game by game).
"""

from __future__ import annotations

import math

import torch

from ._othello_mcts_impl import SearchConfig, _Engine
from .adjudication import check_adjudicate_empties
from .exact_leaves import check_exact_empties
from .native import NativeNet, resolve


def default_node_capacity(num_simulations: int) -> int:
    """Power of two >= 64 searches x num_simulations x 12 nodes, in [2^16, 2^22]
    (observed: ~8.5 children per expansion, games of <= 64 plies; 800 sims ->
    2^20 nodes = 64 MB per game, 1600 sims -> 2^21)."""
    need = 64 * max(1, num_simulations) * 12
    cap = 1 << 16
    while cap < need and cap < (1 << 22):
        cap <<= 1
    return cap


class BatchedMCTS:
    def __init__(
        self,
        num_games: int,
        history_size: int = 8,
        num_simulations: int = 800,
        num_threads: int = 2,
        batch_size: int = 16,
        c_puct_base: float = 20000.0,
        c_puct_init: float = 2.5,
        dirichlet_epsilon: float = 0.25,
        dirichlet_alpha: float = 0.5,
        device: int | None = None,
        seed: int = 0,
        node_capacity: int = 0,
    ) -> None:
        """node_capacity: nodes per game (0 = sized from num_simulations: a whole
        game of 64 searches at ~12 new nodes per simulation, 2^16..2^22). Nodes are
        reclaimed when a game restarts; running out raises (check_health)."""
        if device is None:
            device = torch.cuda.current_device()
        self.device = torch.device("cuda", device)
        self.config = SearchConfig(history_size, num_simulations, num_threads, batch_size, c_puct_base,
                                   c_puct_init, dirichlet_epsilon, dirichlet_alpha)
        if node_capacity == 0:
            node_capacity = default_node_capacity(num_simulations)
        self.node_capacity = node_capacity
        self.engine = _Engine(device, num_games, node_capacity, self.config, seed)
        self.num_games = num_games
        self._actions = torch.empty(num_games, dtype=torch.int32, device=self.device)
        self._finished = torch.empty(num_games, dtype=torch.int32, device=self.device)
        C = 1 + 2 * history_size
        self._targets_f = None
        self._targets_p = None
        self._margin = None
        self._C = C
        self.exact_leaves = 0  # set_exact_leaves
        self.playout_cap = None  # set_playout_cap: (full_probability, fast_simulations)
        self.forced_playouts = None  # set_forced_playouts: (k, prune_targets)

    @property
    def rows_per_step(self) -> int:
        return self.num_games * self.config.num_threads * self.config.batch_size

    def _stream(self) -> int:
        s = torch.cuda.current_stream(self.device).cuda_stream
        self.engine.set_stream(s)
        return s

    def search(self, neural_net, sync: bool = True):
        """Run num_simulations for every active game. Returns (simulations, nn_rows).

        With the native net and ``sync=False`` the search is only enqueued on the
        engine's stream (returns None): a self-play loop then queues the next
        move's kernels while the GPU still runs this one's."""
        self._stream()
        nat = resolve(neural_net, self.device.index, self.config.history_size)
        if nat is not None:
            r = self.engine.search(nat.handle, sync)
            if sync:
                self.engine.check_health()  # raises if a node pool ran out
            return r
        # external evaluator: one call per step over all G * L rows. Each select
        # backs up the previous round thread by thread (the reference's
        # interleaving, csrc/tree.hip k_tree); one backup closes the search.
        rows = self.rows_per_step
        feat = torch.empty((rows, self._C, 8, 8), dtype=torch.float32, device=self.device)
        sims0, evals0 = self.engine.work_counters()
        steps = self.engine.search_begin()
        for _ in range(steps):
            self.engine.select()
            # every row goes to the evaluator; rows of terminal leaves and of
            # threads with no batch waiting this round are never read back
            self.engine.features(feat.data_ptr(), 0, rows)
            out = neural_net(feat)
            pol = out["policy"].detach().to(self.device, torch.float32).contiguous()
            val = out["value"].detach().to(self.device, torch.float32).contiguous()
            self.engine.set_evaluation(pol.data_ptr(), val.data_ptr(), 0, rows)
        self.engine.backup()
        self.engine.check_health()
        sims1, evals1 = self.engine.work_counters()
        # simulations = leaf selections; evaluations = rows of non-terminal
        # leaves (terminal ones need no NN, search_thread.cpp:88-90)
        return sims1 - sims0, evals1 - evals0

    def check_health(self) -> None:
        """Raise RuntimeError if any game's node pool ran out or a descent hit
        the depth cap (waits for the engine's stream). Asynchronous searches
        (sync=False) are checked here or by SelfPlayCollector."""
        self._stream()
        self.engine.check_health()

    def reset(self, game: int = -1, seed: int = 0) -> None:
        self._stream()
        self.engine.reset(game, seed)

    def set_active(self, active=None) -> None:
        """Per-game mask (G bools; None = every game): inactive games are left
        alone by search, selfplay_move and apply_actions. reset() reactivates
        the games it resets."""
        self._stream()
        if active is None:
            self.engine.set_active(0)
            return
        m = torch.as_tensor(active).to(self.device).ne(0).to(torch.uint8).contiguous()
        if m.shape != (self.num_games,):
            raise ValueError(f"Expected {self.num_games} mask entries, but got shape {tuple(m.shape)}.")
        self.engine.set_active(m.data_ptr())

    def set_positions(self, positions, history=None, ply=None, keys=None, games=None, seed: int = 0) -> None:
        """Put given positions at the roots of games.

        ``positions``: an ``(n, 5)`` int64 tensor in ``pack_positions`` layout or a
        sequence of ``Position`` objects / ``(player, player1_discs,
        player2_discs)`` triples; entry i goes to game ``games[i]`` (default
        ``range(n)``, n <= G). Only the player and the two disc sets are read: the
        engine stores ``canonical_position`` of each. ``history``: the positions
        before each root, newest first, as ``(n, K, 5)`` or as a list of
        per-position lists of unequal length (K <= 15); they fill the history
        planes as the game's own earlier roots would. ``ply``: moves played so
        far (default: discs - 4), read by the self-play move's temperature
        schedule and the playout cap. ``keys``: the games' random-stream keys
        (default: the keys ``reset(game, seed)`` gives).

        A game that is set is as after ``reset``: a fresh tree, active, event 0.
        Waits for the engine's stream to read the status back; raises ValueError
        naming the first rejected entry and its fault. Rejected games are left as
        they were, and the accepted games of the same call stay set."""
        from .analysis import pack_history, pack_position_rows, set_positions_fault

        G = self.num_games
        self._stream()
        rows = pack_position_rows(positions)
        n = rows.shape[0]
        if games is None:
            games = list(range(n))
        games = [int(g) for g in games]
        if len(games) != n:
            raise ValueError(f"Expected {n} game indices, but got {len(games)}.")
        if n > G or len(set(games)) != n or any(not 0 <= g < G for g in games):
            raise ValueError(f"Expected at most {G} distinct games in [0, {G}), but got {games}.")
        idx = torch.tensor(games, dtype=torch.int64)
        pos = torch.zeros((G, 5), dtype=torch.int64)
        pos[idx] = rows
        mask = torch.zeros(G, dtype=torch.uint8)
        mask[idx] = 1
        dev = self.device
        hist_d = len_d = ply_d = keys_d = None
        K = 0
        if history is not None:
            hist_n, lens = pack_history(history, n)
            K = hist_n.shape[1]
            if K > 0:
                hist = torch.zeros((G, K, 5), dtype=torch.int64)
                hist[idx] = hist_n
                hl = torch.zeros(G, dtype=torch.int32)
                hl[idx] = lens
                hist_d, len_d = hist.to(dev), hl.to(dev)
        if ply is not None:
            pl = torch.zeros(G, dtype=torch.int32)
            pl[idx] = torch.as_tensor(ply).to("cpu", torch.int32).reshape(n)
            ply_d = pl.to(dev)
        if keys is not None:
            if isinstance(keys, torch.Tensor):
                kn = keys.to("cpu", torch.int64).reshape(n)
            else:
                kn = torch.tensor([(int(k) & 0xFFFFFFFFFFFFFFFF) - ((int(k) & (1 << 63)) << 1) for k in keys],
                                  dtype=torch.int64).reshape(n)
            kk = torch.zeros(G, dtype=torch.int64)
            kk[idx] = kn
            keys_d = kk.to(dev)
        pos_d, mask_d = pos.to(dev), mask.to(dev)
        status = torch.empty(G, dtype=torch.int32, device=dev)
        ptr = lambda t: 0 if t is None else t.data_ptr()  # noqa: E731
        self.engine.set_positions(pos_d.data_ptr(), ptr(hist_d), K, ptr(len_d), ptr(keys_d), ptr(ply_d),
                                  mask_d.data_ptr(), int(seed) & 0xFFFFFFFFFFFFFFFF, status.data_ptr())
        st = status.cpu()[idx]  # the host wait: the inputs above outlive the kernel
        bad = torch.nonzero(st != 0).reshape(-1)
        if bad.numel():
            i = int(bad[0])
            raise ValueError(f"set_positions: entry {i} (game {games[i]}) was rejected: "
                             f"{set_positions_fault(int(st[i]))}"
                             + (f" ({bad.numel()} entries rejected in all)" if bad.numel() > 1 else "") + ".")

    def principal_variations(self, max_len: int = 16) -> dict[str, torch.Tensor]:
        """The most visited line below every root, read on the device (DESIGN.md
        §22): from the root the child with the most visits, the lowest action
        among equals, then the same below it, until a node without children, a
        best child without a visit or ``max_len`` (1..64) entries. Device
        tensors: ``actions`` (G, max_len) int32 padded with -1, ``visits``
        (G, max_len) int32 and ``q`` (G, max_len) fp32 of the chosen children
        (as ``root_stats`` reports a root's), ``length`` (G) int32, 0 for an
        inactive game. Enqueued only."""
        max_len = int(max_len)
        if not 1 <= max_len <= 64:
            raise ValueError(f"Expected 1 <= max_len <= 64, but got {max_len}.")
        self._stream()
        G, d = self.num_games, self.device
        out = {"actions": torch.empty((G, max_len), dtype=torch.int32, device=d),
               "visits": torch.empty((G, max_len), dtype=torch.int32, device=d),
               "q": torch.empty((G, max_len), dtype=torch.float32, device=d),
               "length": torch.empty(G, dtype=torch.int32, device=d)}
        self.engine.principal_variations(max_len, out["actions"].data_ptr(), out["visits"].data_ptr(),
                                         out["q"].data_ptr(), out["length"].data_ptr())
        return out

    def set_playout_cap(self, full_probability: float | None = None, fast_simulations: int | None = None) -> None:
        """Playout cap randomization (KataGo, Wu 2019, section 3.1).
        With a cap set, a game's search at a given ply is a full one
        (num_simulations, root noise, its move recorded) with probability
        ``full_probability``; otherwise a fast one: ``fast_simulations``, no
        root noise, and the move that follows it is played but writes no targets
        and carries FIN_FAST in ``finished``. Which one is a function of the
        game's key and ply alone (``othello_mcts.playout_cap_is_full``), so no
        other random draw of the game moves. ``None`` (both): off, the default.
        The arena does not use the setting and rejects an engine that has it."""
        if full_probability is None and fast_simulations is None:
            self.engine.set_playout_cap(1.0, 0)
            self.playout_cap = None
            return
        if full_probability is None or fast_simulations is None:
            raise ValueError("Expected full_probability and fast_simulations together (or neither: off).")
        p, n = float(full_probability), int(fast_simulations)
        if not 0.0 < p <= 1.0:
            raise ValueError(f"Expected 0 < full_probability <= 1, but got {full_probability}.")
        if not 1 <= n <= self.config.num_simulations:
            raise ValueError(f"Expected 1 <= fast_simulations <= num_simulations ({self.config.num_simulations}), "
                             f"but got {fast_simulations}.")
        self.engine.set_playout_cap(p, n)
        self.playout_cap = (p, n)

    def set_forced_playouts(self, k: float | None = None, prune_targets: bool = True) -> None:
        """Forced playouts and policy target pruning (KataGo, Wu 2019, section 3.2;
        DESIGN.md §18). With ``k`` set, the root of every full search (never a
        fast one of a playout cap) takes a child that has been tried first while
        ``n_c * n_c < (k * prob_c) * total`` (fp32; ``prob_c`` the prior of that
        selection's PUCT line, noised when the root draws noise; ``total`` the
        children's visits with in-flight ones): every tried child keeps a floor
        of ``sqrt(k * prob_c * total)`` visits. With ``prune_targets`` the
        self-play targets are written from ``othello_mcts.prune_visit_counts`` of
        the root instead of the raw counts: the visits PUCT alone would not have
        spent are taken out, and a child left with one is dropped. Visit counts
        and Q as queried, the move choice and ``finished`` do not change; no
        random event is consumed. ``None``: off, the default. KataGo uses k = 2.
        The arena does not use the setting and rejects an engine that has it."""
        if k is None:
            self.engine.set_forced_playouts(0.0, False)
            self.forced_playouts = None
            return
        kf = float(k)
        if not (math.isfinite(kf) and kf > 0.0):
            raise ValueError(f"Expected a finite forced playout factor k > 0, but got {k}.")
        self.engine.set_forced_playouts(kf, bool(prune_targets))
        self.forced_playouts = (kf, bool(prune_targets))

    def set_exact_leaves(self, max_empties: int | None = None) -> None:
        """Exact leaf values. With ``max_empties = E`` in 1..10 a
        search never expands and never evaluates a node below the root that is
        not terminal and has at most E empties: the first visit solves it with
        the exact endgame solver, and every visit backs up the sign of the exact
        result as a terminal leaf would (no NN row, no random event, not an
        evaluation). The root itself is always evaluated and expanded. The
        external-evaluator path, ``search`` with a native net, ``selfplay_steps``
        and every schedule follow the same rule and give the same trees.
        ``None`` (or 0): off, the default. The value may change only while no
        game holds a tree built under another value: before the first search,
        or after ``reset()`` of all games or ``random_openings`` (ValueError
        otherwise). Independent of the playout cap, forced playouts and
        ``adjudicate_empties``. The arena rejects an engine that has it."""
        e = 0 if max_empties is None else check_exact_empties(max_empties, allow_off=True)
        self.engine.set_exact_leaves(e)
        self.exact_leaves = e

    def exact_leaf_counters(self) -> dict[str, int]:
        """Since the engine was created (waits for the engine's stream):
        ``solves`` rows that ended at an exact leaf not solved yet (each one is
        solved), ``hits`` rows that ended at a solved leaf, ``nodes`` positions
        the solves visited."""
        self._stream()
        solves, hits, nodes = self.engine.exact_leaf_counters()
        return {"solves": solves, "hits": hits, "nodes": nodes}

    def root_priors(self) -> torch.Tensor:
        """Stored priors of every game's root children, (G, 65) indexed by action
        like ``root_stats`` (0 where there is no child)."""
        self._stream()
        p = torch.empty((self.num_games, 65), dtype=torch.float32, device=self.device)
        self.engine.root_priors(p.data_ptr())
        return p

    def random_openings(self, max_moves: int = 8, seed: int = 0) -> None:
        self._stream()
        self.engine.random_openings(max_moves, seed)

    def root_info(self, game: int) -> dict:
        self._stream()
        return self.engine.root_info(game)

    def visit_counts(self, game: int) -> list[int]:
        return self.root_info(game)["visit_counts"]

    def mean_action_values(self, game: int) -> list[float]:
        return self.root_info(game)["mean_action_values"]

    def root_stats(self) -> tuple[torch.Tensor, torch.Tensor]:
        """(visits, q) of every game's root children, (G, 65) indexed by action."""
        self._stream()
        v = torch.empty((self.num_games, 65), dtype=torch.int32, device=self.device)
        q = torch.empty((self.num_games, 65), dtype=torch.float32, device=self.device)
        self.engine.root_stats(v.data_ptr(), q.data_ptr(), 0)
        return v, q

    def root_positions(self) -> torch.Tensor:
        """Every game's root as ``oamd_position``: (G, 5) int64 on the device
        (player, the two disc sets, legal moves, the passer's opponent's
        moves), what ``othello_mcts.solve_endgames`` takes. Enqueued only."""
        self._stream()
        info = torch.empty((self.num_games, 8), dtype=torch.int64, device=self.device)  # oamd_root_info: 64 bytes
        self.engine.root_stats(0, 0, info.data_ptr())
        return info[:, :5].contiguous()

    def self_play_data(self, game: int):
        self._stream()
        f, p = self.engine.self_play_data(game)
        return {"features": list(torch.from_numpy(f)), "policy": list(torch.from_numpy(p))}

    def apply_action(self, game: int, action: int) -> None:
        self._stream()
        self.engine.apply_action(game, action)

    def apply_actions(self, actions: torch.Tensor) -> None:
        """actions: (G,) int32 on the engine's device, -1 = leave the game."""
        self._stream()
        a = actions.to(self.device, torch.int32).contiguous()
        self.engine.apply_actions(a.data_ptr())

    def selfplay_move(self, temperature_moves: int = 12, temperature: float = 1.0, opening_moves: int = 0,
                      emit_targets: bool = False, adjudicate_empties: int = 0,
                      split: bool = False) -> dict[str, torch.Tensor]:
        """One self-play move for every game (train.py:404-452 on device): choose the
        move from the root visits, (optionally) emit the 8-fold targets, apply it, and
        restart finished games from a random opening. Returns device tensors.

        adjudicate_empties = K > 0 (othello_mcts.adjudication): a move that leaves
        a non-terminal root with at most K empties ends the game there with the
        exact result (``split``: by the split solver); ``finished`` carries
        FIN_ADJUDICATED and the outcome, and ``out["margin"]`` (G) the exact
        margin seen from black (disc difference for a game that ended on the
        board, MARGIN_NONE where no game ended)."""
        k = check_adjudicate_empties(adjudicate_empties)
        self._stream()
        if emit_targets and self._targets_f is None:
            self._targets_f = torch.empty((self.num_games, 8, self._C, 8, 8), dtype=torch.float32,
                                          device=self.device)
            self._targets_p = torch.empty((self.num_games, 8, 65), dtype=torch.float32, device=self.device)
        f = self._targets_f.data_ptr() if emit_targets else 0
        p = self._targets_p.data_ptr() if emit_targets else 0
        if k > 0:
            if self._margin is None:
                self._margin = torch.empty(self.num_games, dtype=torch.int32, device=self.device)
            self.engine.selfplay_move_adjudicated(temperature_moves, temperature, opening_moves, emit_targets,
                                                  self._actions.data_ptr(), self._finished.data_ptr(), f, p, k,
                                                  bool(split), self._margin.data_ptr())
        else:
            self.engine.selfplay_move(temperature_moves, temperature, opening_moves, emit_targets,
                                      self._actions.data_ptr(), self._finished.data_ptr(), f, p)
        out = {"actions": self._actions, "finished": self._finished}
        if k > 0:
            out["margin"] = self._margin
        if emit_targets:
            out["features"] = self._targets_f
            out["policy"] = self._targets_p
        return out

    def selfplay_steps(self, neural_net, n_moves: int, temperature_moves: int = 12, temperature: float = 1.0,
                       opening_moves: int = 0, emit_targets: bool = False,
                       keep_all: bool = True, adjudicate_empties: int = 0,
                       split: bool = False, sim_budget: int = 0) -> dict[str, torch.Tensor]:
        """n_moves x (search(net) + selfplay_move(...)) in one enqueue, same results
        move for move; each pipeline group chains its searches and moves on its own
        stream, so the per-move join disappears (oamd_engine_selfplay_steps).
        keep_all: outputs shaped (n_moves, G, ...); else only the last move's
        (G, ...), every move writing the same buffers. Native net (or a module
        search() would convert) only. adjudicate_empties / split: as
        selfplay_move, ``out["margin"]`` shaped like ``finished``; with more than
        one move it needs keep_all=True (ValueError otherwise).

        sim_budget = S > 0 (free-running games only, keep_all=True): a work
        budget per game in place of the move count. n_moves is then the number
        of output slices and the most moves a game plays; a game stops after the
        move whose search brought the nominal simulations of the searches it
        started in this call to S or more (it overshoots by less than one
        search). A game's moves fill a prefix of its slices, and the slices it
        did not reach hold action -1 and finished 0. Meant for a playout cap
        (set_playout_cap), where games given the same number of moves would
        finish the call at very different times."""
        k = check_adjudicate_empties(adjudicate_empties, max(0, int(n_moves)), keep_all)
        sim_budget = int(sim_budget)
        if sim_budget < 0:
            raise ValueError(f"Expected sim_budget >= 0, but got {sim_budget}.")
        if sim_budget > 0 and not keep_all:
            raise ValueError("sim_budget needs keep_all=True: games play different numbers of moves in the call.")
        self._stream()
        net = resolve(neural_net, self.device.index, self.config.history_size)
        if net is None:
            raise TypeError("selfplay_steps needs a NativeNet (or an eval-mode AlphaZeroNet)")
        n = max(0, int(n_moves))
        lead = (n,) if keep_all else ()
        actions = torch.empty(lead + (self.num_games,), dtype=torch.int32, device=self.device)
        finished = torch.empty_like(actions)
        feat = pol = None
        if emit_targets:
            feat = torch.empty(lead + (self.num_games, 8, self._C, 8, 8), dtype=torch.float32, device=self.device)
            pol = torch.empty(lead + (self.num_games, 8, 65), dtype=torch.float32, device=self.device)
        fp = feat.data_ptr() if feat is not None else 0
        pp = pol.data_ptr() if pol is not None else 0
        out = {"actions": actions, "finished": finished}
        if k > 0 or sim_budget > 0:
            margin = torch.empty_like(actions) if k > 0 else None
            self.engine.selfplay_steps_budget(net.handle, n, sim_budget, temperature_moves, temperature,
                                              opening_moves, emit_targets, keep_all, actions.data_ptr(),
                                              finished.data_ptr(), fp, pp, k, bool(split),
                                              margin.data_ptr() if k > 0 else 0)
            if k > 0:
                out["margin"] = margin
        else:
            self.engine.selfplay_steps(net.handle, n, temperature_moves, temperature, opening_moves, emit_targets,
                                       keep_all, actions.data_ptr(), finished.data_ptr(), fp, pp)
        if emit_targets:
            out["features"] = feat
            out["policy"] = pol
        return out


__all__ = ["BatchedMCTS", "NativeNet"]
