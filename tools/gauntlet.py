"""A net against a baseline opponent on one MI355X (othello_mcts.Gauntlet): the
reference's evaluation games against RandomPlayer, GreedyPlayer and the
external engine (evaluation.py, player.py:121-175, 262-321), G matches at once,
with the built-in depth-limited search in place of the engine.

The net is a reference checkpoint directory (config.json + neural_net.pth), an
.npz state dict with the reference's keys, or live:SEED (a seeded untrained net
of the shape of --like). Prints W/D/L and the score of the net, plies, wall
time and the share of it spent in the baseline's kernels, and writes them with
the game records (the dicts evaluation.py writes, input of the reference's
estimate_elo / save_pgn; the baseline's id is random, greedy or search-D) as
JSON.

Usage (GPU box):
  python tools/gauntlet.py CHECKPOINT_DIR --baseline search --depth 4 [--games 256] [--sims 800]
                           [--opening-plies 4] [--out gauntlet.json]
"""

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "othello-alphazero_amd"))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import torch  # noqa: E402

import othello_mcts as om  # noqa: E402
from arena import load_state  # noqa: E402  (tools/arena.py)


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("net")
    ap.add_argument("--baseline", default="search", choices=["random", "greedy", "search"])
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--threads", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--like", default=str(ROOT / "bench_nets" / "selfplay_128x10b_h8.npz"),
                    help="the net whose shape live:SEED takes")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    sd = load_state(a.net, load_state(a.like) if a.net.startswith("live:") else None)
    net = om.NativeNet(sd, device=0, dtype=a.dtype)
    mcts = om.BatchedMCTS(a.games, history_size=net.history_size, num_simulations=a.sims, num_threads=a.threads,
                          batch_size=a.batch, dirichlet_epsilon=0.0, seed=a.seed)
    gauntlet = om.Gauntlet(mcts, a.baseline, a.depth, seed=a.seed)
    gauntlet.time_baseline = True
    gauntlet.reset(openings=om.paired_openings(a.games, a.opening_plies, a.seed))
    c0 = mcts.engine.work_counters()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = gauntlet.play(net)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    c1 = mcts.engine.work_counters()
    baseline_ms = gauntlet.baseline_ms()
    sims, evals = c1[0] - c0[0], c1[1] - c0[1]
    w, d, lost = res.wdl()
    moves = int((res.actions >= 0).sum())
    out = {
        "net": a.net, "baseline": gauntlet.baseline_id, "games": a.games, "num_simulations": a.sims,
        "num_threads": a.threads, "batch_size": a.batch, "opening_plies": a.opening_plies, "dtype": a.dtype,
        "seed": a.seed, "wins_net": w, "draws": d, "losses_net": lost, "score_net": res.score_a(),
        "plies": res.plies, "moves": moves, "wall_s": wall, "baseline_moves_device_ms": baseline_ms,
        "baseline_share_of_wall": baseline_ms / 1e3 / wall, "simulations": sims, "nn_rows": evals,
        "simulations_per_s": sims / wall, "device": torch.cuda.get_device_name(0),
        "margin": res.margin.tolist(), "mean_margin_net": float(res.margin_a().float().mean()),
        "net_is_white": res.a_is_white.tolist(), "records": res.records(a.net, gauntlet.baseline_id),
    }
    print(f"{a.net} vs {gauntlet.baseline_id}: {a.games} matches, {a.sims} simulations per move")
    print(f"W/D/L (net) {w}/{d}/{lost}  score {out['score_net']:.3f}  plies {res.plies}  moves {moves}  "
          f"mean margin (net) {out['mean_margin_net']:+.2f}")
    print(f"wall {wall:.2f} s  baseline kernels {baseline_ms:.1f} ms ({100 * out['baseline_share_of_wall']:.2f} % of "
          f"wall)  {sims / wall / 1e6:.3f} M simulations/s")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
