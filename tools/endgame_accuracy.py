"""Endgame accuracy of a net's search against exact play: the
absolute yardstick the reference gets from an external solver engine
(EgaroucidPlayer, player.py:262-321), here from the on-device exact solver.

    python tools/endgame_accuracy.py NET --games 256 --sims 800 --empties 12 --out FILE

NET: a reference checkpoint directory (config.json + neural_net.pth), an .npz
state dict (bench_nets/), or live:SEED (a seeded live-statistics 128x10b H = 8
net, othello_mcts.synthetic.live_state_dict).

Self-play as AlphaZeroPlayer plays (player.py:177-259): no Dirichlet noise,
argmax moves, and a few uniformly random opening plies for variety. Per move:
the roots are read (BatchedMCTS.root_positions) and solved before
selfplay_move, and endgame_move_loss judges the move after it. A game that
ends restarts from a new random opening and is simply a new game; the run
stops after --games finished games. Reported per empties count 1..E: positions,
share of exactly optimal moves, share with the win/draw/loss kept, mean disc
loss; plus the solver's nodes and time (device events around the solver calls).
"""

from __future__ import annotations

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "othello-alphazero_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import othello_mcts as om  # noqa: E402
from othello_mcts.native import load_checkpoint  # noqa: E402
from othello_mcts.synthetic import live_state_dict  # noqa: E402


def load_state(spec: str) -> dict:
    if spec.startswith("live:"):
        return live_state_dict(int(spec[5:]), 17, 128, 9, 128)
    p = Path(spec)
    if p.is_dir():
        return load_checkpoint(p)[1]
    z = np.load(p, allow_pickle=False)
    return {k: (np.array(0, dtype=np.int64) if k.endswith("num_batches_tracked")
                else np.ascontiguousarray(z[k], dtype=np.float32)) for k in z.files}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("net")
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--empties", type=int, default=12)
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--threads", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--node-limit", type=int, default=om.endgame.DEFAULT_NODE_LIMIT)
    ap.add_argument("--split", action="store_true", help="solve with the split solver (DESIGN.md §15)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()

    net = om.NativeNet(load_state(a.net), device=0, dtype=a.dtype)
    G, E = a.games, a.empties
    b = om.BatchedMCTS(G, history_size=net.history_size, num_simulations=a.sims, num_threads=a.threads,
                       batch_size=a.batch, dirichlet_epsilon=0.0, seed=a.seed)
    b.random_openings(a.opening_plies, seed=a.seed)
    dev = b.device
    # per empties count: positions, optimal moves, w/d/l kept, discs lost (device, no host read per move)
    stats = torch.zeros((E + 1, 4), dtype=torch.int64, device=dev)
    totals = torch.zeros(3, dtype=torch.int64, device=dev)  # games finished, solver nodes, unsolved roots
    events = []
    moves, finished = 0, 0
    while finished < G:
        for _ in range(8):  # one host read per 8 moves
            roots = b.root_positions()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            sol = om.solve_endgames(roots, E, a.node_limit, split=a.split)
            t1.record()
            events.append((t0, t1))
            b.search(net, sync=False)
            out = b.selfplay_move(temperature_moves=0, opening_moves=a.opening_plies)
            loss, kept, empties = om.endgame_move_loss(roots, out["actions"], E, solution=sol)
            judged = loss >= 0
            e = empties.clamp(0, E)
            row = torch.stack([judged, judged & (loss == 0), judged & (kept == 1), loss.clamp(min=0)], 1).to(torch.int64)
            stats.index_add_(0, e, row)
            totals[0] += ((out["finished"] & 3) != 0).sum()
            totals[1] += sol.nodes.sum()
            totals[2] += ((sol.flags & ~om.endgame.FLAG_TOO_MANY_EMPTIES) != 0).sum()
            moves += 1
        finished = int(totals[0])
        print(f"{moves} moves, {finished} games finished", file=sys.stderr, flush=True)
    b.check_health()
    torch.cuda.synchronize()
    solver_ms = sum(t0.elapsed_time(t1) for t0, t1 in events)
    s = stats.cpu().numpy()
    per = []
    for e in range(1, E + 1):
        n = int(s[e, 0])
        per.append({"empties": e, "positions": n, "optimal": round(s[e, 1] / n, 4) if n else None,
                    "wdl_kept": round(s[e, 2] / n, 4) if n else None,
                    "mean_disc_loss": round(s[e, 3] / n, 4) if n else None})
    n = int(s[1:, 0].sum())
    report = {"net": a.net, "games_finished": finished, "parallel_games": G, "moves_per_game_slot": moves,
              "sims": a.sims, "empties": E, "dtype": a.dtype, "opening_plies": a.opening_plies, "seed": a.seed,
              "command": "python tools/endgame_accuracy.py " + " ".join(sys.argv[1:]),
              "all": {"positions": n, "optimal": round(s[1:, 1].sum() / n, 4), "wdl_kept": round(s[1:, 2].sum() / n, 4),
                      "mean_disc_loss": round(s[1:, 3].sum() / n, 4)} if n else None,
              "per_empties": per, "solver_nodes": int(totals[1]), "solver_ms": round(solver_ms, 1),
              "solver_calls": len(events), "unsolved_roots": int(totals[2]), "node_limit": a.node_limit}
    text = json.dumps(report, indent=1)
    print(text)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
