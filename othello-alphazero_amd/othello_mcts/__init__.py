"""MI355X-native drop-in for the reference's ``othello_mcts`` package.

Same import surface as cpp/src/othello_mcts/__init__.py:1-6 (``MCTS``,
``Position``, ``get_flips``, ``get_legal_moves``), backed by hand-written HIP
kernels for gfx950 behind the C ABI in include/othello_mcts_amd.h. Additive
API: ``BatchedMCTS`` (G games per GPU, on-device self-play driver),
``Arena`` (G head-to-head matches between two nets, one tree per player),
``NativeNet`` (fused bf16/fp16 AlphaZeroNet forward, also from a reference
checkpoint directory via ``load_checkpoint``), ``SelfPlayCollector`` /
``self_play`` (training samples in the reference's ``_self_play`` format) and
the training step beside the engine (``SampleBuffer``, ``train_epoch``,
``alphazero_loss``, ``refresh_native``: train.py:455-521 with the samples kept
in HBM) and ``ReplayBuffer`` / ``train_epoch_replay``: the same samples kept as
packed positions (bitboards, 94 times smaller at H = 8) and expanded to the 8
board symmetries when a minibatch is gathered. ``solve_endgames`` /
``solve_position`` / ``endgame_move_loss`` solve the last plies exactly (GPU
and host) and measure a move against perfect play;
``ReplayBuffer(track_exact=True).relabel_endgames`` uses the same solver to
give the buffer's last plies exact value targets, and ``adjudicate_empties=K``
(self-play, arena; ``adjudicate`` is the rule on the host) ends running games
at K empties with the exact result. ``BatchedMCTS.set_playout_cap`` switches on
playout cap randomization (full searches recorded, fast ones only played:
``FIN_FAST``, ``playout_cap_is_full``), and ``selfplay_steps(sim_budget=...)``
gives every game of a free-running call a work budget instead of a move count.
``BatchedMCTS.set_forced_playouts`` switches on forced playouts at the root of
full searches and policy target pruning (``prune_visit_counts`` is the pruning
rule on the host). ``BatchedMCTS.set_exact_leaves`` makes the search solve
leaves with few empties instead of asking the net (``exact_leaf_value`` is the
rule on the host, ``exact_leaf_values`` the solve kernel's path on the GPU).
``baseline_moves`` / ``baseline_move`` are fixed classical opponents (random,
greedy, a depth-limited alpha-beta search; GPU and host) and ``Gauntlet`` plays
G matches of one net against one of them. ``BatchedMCTS.set_positions`` puts
given positions (with their history) at the roots, ``principal_variations``
reads the most visited lines on the device, and ``analyze`` takes any list of
positions through an engine (``parse_board`` / ``format_board`` for board
strings, ``canonical_position`` is the stored form on the host).

There is no CPU fallback: importing works anywhere the extension was built,
but creating a search object needs a ROCm GPU and raises otherwise.
"""

# The reference imports torch first (its extension links libtorch). We keep the
# same order so user code that relies on it behaves identically.
import torch  # noqa: F401

from ._othello_mcts_impl import (  # noqa: F401
    MCTS,
    Position,
    SearchConfig,
    abi_version,
    device_count,
    get_flips,
    get_legal_moves,
    playout_cap_is_full,
    prune_visit_counts,
)
from .batched import BatchedMCTS  # noqa: E402,F401
from .arena import Arena, ArenaResult, paired_openings  # noqa: E402,F401
from .native import NativeNet, load_checkpoint  # noqa: E402,F401
from .selfplay import FIN_FAST, SelfPlayCollector, self_play  # noqa: E402,F401
from .replay import ReplayBuffer  # noqa: E402,F401
from .endgame import EndgameSolution, endgame_move_loss, solve_endgames, solve_position  # noqa: E402,F401
from .adjudication import adjudicate  # noqa: E402,F401
from .baseline import BaselineMoves, Gauntlet, baseline_move, baseline_moves  # noqa: E402,F401
from .exact_leaves import exact_leaf_value, exact_leaf_values  # noqa: E402,F401
from .analysis import Analysis, analyze, canonical_position, format_board, parse_board, position_key  # noqa: E402,F401
from .training import (  # noqa: E402,F401
    SampleBuffer,
    alphazero_loss,
    refresh_native,
    train_epoch,
    train_epoch_replay,
)

__all__ = [
    "MCTS",
    "Position",
    "get_flips",
    "get_legal_moves",
    "BatchedMCTS",
    "NativeNet",
    "SearchConfig",
    "SelfPlayCollector",
    "load_checkpoint",
    "self_play",
    "SampleBuffer",
    "alphazero_loss",
    "train_epoch",
    "train_epoch_replay",
    "refresh_native",
    "ReplayBuffer",
    "Arena",
    "ArenaResult",
    "paired_openings",
    "EndgameSolution",
    "solve_endgames",
    "solve_position",
    "endgame_move_loss",
    "adjudicate",
    "FIN_FAST",
    "playout_cap_is_full",
    "prune_visit_counts",
    "exact_leaf_value",
    "exact_leaf_values",
    "BaselineMoves",
    "Gauntlet",
    "baseline_move",
    "baseline_moves",
    "Analysis",
    "analyze",
    "canonical_position",
    "parse_board",
    "format_board",
    "position_key",
]
