"""Label noise of self-play value targets in the last plies:
how often the outcome of the game a position came from has another sign than
the position's exact result.

    python tools/relabel_report.py NET --games 256 --sims 800 --empties 10 --out FILE

NET: as tools/endgame_accuracy.py takes it (a checkpoint directory, an .npz
state dict, or live:SEED).

Self-play as training plays it (tools/selfplay_train.py: Dirichlet noise 0.25 /
0.5, temperature for the first 12 moves) into a packed ReplayBuffer with
track_exact=True until --games games have finished. The game-outcome values
are kept aside, relabel_endgames(--empties) replaces them by the exact ones,
and the two are compared per empties count: positions, the share whose
game-outcome sign differs from the exact sign (a drawn game counts as differing
from an exact win or loss), and how the differing ones split. Also the device
time of the relabel calls.
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "othello-alphazero_amd"))

import torch  # noqa: E402

import othello_mcts as om  # noqa: E402
from othello_mcts.replay import EXACT_GAVE_UP, EXACT_UNKNOWN  # noqa: E402

from endgame_accuracy import load_state  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("net")
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--empties", type=int, default=10)
    ap.add_argument("--threads", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--seed", type=int, default=77)
    ap.add_argument("--budget", type=int, default=16384)
    ap.add_argument("--node-limit", type=int, default=om.endgame.DEFAULT_NODE_LIMIT)
    ap.add_argument("--split", action="store_true", help="relabel with the split solver (DESIGN.md §15)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    net = om.NativeNet(load_state(a.net), device=0, dtype=a.dtype)
    G, E = a.games, a.empties
    b = om.BatchedMCTS(G, history_size=net.history_size, num_simulations=a.sims, num_threads=a.threads,
                       batch_size=a.batch, dirichlet_epsilon=0.25, dirichlet_alpha=0.5, seed=a.seed)
    b.reset()
    dev = b.device
    rb = om.ReplayBuffer(G, net.history_size, capacity=G * 256, device=dev, track_exact=True)
    moves = 0
    while rb.games_completed < G:  # one host read per 16 moves
        rb.add(b.selfplay_steps(net, 16, temperature_moves=12, opening_moves=0, emit_targets=True, keep_all=True))
        moves += 16
        print(f"{moves} moves, {rb.games_completed} games finished", file=sys.stderr, flush=True)
    rb.check()
    b.check_health()
    size, games = rb.size, rb.games_completed
    assert rb.head == size, "the ring must not wrap: the rows below are read in place"
    game_value = rb.value[:size].clone()

    events, calls = [], 0
    while True:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        rb.relabel_endgames(E, a.budget, a.node_limit, split=a.split)
        t1.record()
        events.append((t0, t1))
        calls += 1
        stats = rb.relabel_stats
        if stats["left"] == 0:
            break
    torch.cuda.synchronize()
    relabel_ms = [round(t0.elapsed_time(t1), 3) for t0, t1 in events]

    exact = rb.exact[:size].to(torch.int64)
    solved = (exact != EXACT_UNKNOWN) & (exact != EXACT_GAVE_UP)
    occupied = (rb.boards[:size, 0].view(torch.int64) | rb.boards[:size, 1].view(torch.int64)).contiguous()
    table = torch.tensor([bin(i).count("1") for i in range(256)], dtype=torch.int64, device=dev)
    empties = 64 - table[occupied.view(torch.uint8).reshape(-1, 8).to(torch.int64)].sum(1)
    g, x = torch.sign(game_value).to(torch.int64), torch.sign(exact)
    assert bool((torch.sign(rb.value[:size]).to(torch.int64)[solved] == x[solved]).all())
    assert bool((rb.value[:size][~solved] == game_value[~solved]).all())

    def row(mask: torch.Tensor) -> dict:
        n = int(mask.sum())
        differs = mask & (g != x)
        d = int(differs.sum())
        return {"positions": n, "from_drawn_games": int((mask & (g == 0)).sum()),
                "exactly_drawn": int((mask & (x == 0)).sum()),
                "differs": d, "differs_share": round(d / n, 4) if n else None,
                # of the differing ones: the game was drawn / the exact result is a draw / win and loss swapped
                "game_drawn": int((differs & (g == 0)).sum()), "exact_draw": int((differs & (x == 0)).sum()),
                "win_loss_swapped": int((differs & (g * x == -1)).sum())}

    per = [{"empties": e, **row(solved & (empties == e))} for e in range(0, E + 1)]
    report = {"net": a.net, "games_finished": games, "parallel_games": G, "moves_per_game_slot": moves,
              "sims": a.sims, "empties": E, "dtype": a.dtype, "seed": a.seed,
              "command": "python tools/relabel_report.py " + " ".join(sys.argv[1:]),
              "positions_in_buffer": size, "buffer_positions_from_drawn_games": int((g == 0).sum()),
              "all": row(solved), "per_empties": per,
              "relabel_stats": stats, "relabel_calls": calls, "budget": a.budget, "relabel_ms": relabel_ms,
              "node_limit": a.node_limit}
    text = json.dumps(report, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
