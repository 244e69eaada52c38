"""Head-to-head matches between two nets on one MI355X (othello_mcts.Arena):
the reference's evaluation games (evaluation.py:15-90: play_game between two
AlphaZeroPlayers, in pairs with the colours swapped), G matches at once.

Each net is a reference checkpoint directory (config.json + neural_net.pth,
NativeNet.from_checkpoint), an .npz state dict with the reference's keys, or
live:SEED (a seeded net of the other net's shape, synthetic.live_state_dict).
Prints W/D/L and the score of net A, plies, wall time and simulations/s, and
writes them with the game records (the dicts evaluation.py writes, input of
the reference's estimate_elo / save_pgn) as JSON.

Usage (GPU box):
  python tools/arena.py NET_A NET_B [--games 256] [--sims 800] [--opening-plies 4] [--out FILE.json]
                        [--adjudicate K [--split]]

--adjudicate K: a match ends at the ply that leaves at most K empties, with the
exact result of that position (Arena.play(adjudicate_empties=K), DESIGN.md §16;
--split: by the split solver). The JSON carries margin (seen from black) and
adjudicated per match.
"""

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "othello-alphazero_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import othello_mcts as om  # noqa: E402
from othello_mcts.native import load_checkpoint  # noqa: E402
from othello_mcts.synthetic import live_state_dict, net_config_from_state_dict  # noqa: E402


def load_state(spec: str, like: dict | None = None) -> dict:
    if spec.startswith("live:"):
        if like is None:
            raise SystemExit("live:SEED takes its shape from the other net, which must be a file or directory")
        c = net_config_from_state_dict(like)
        return live_state_dict(int(spec[5:]), c["in_channels"], c["conv_channels"], c["num_residual_blocks"],
                               c["value_head_hidden_channels"])
    p = Path(spec)
    if p.is_dir():
        return load_checkpoint(p)[1]
    z = np.load(p, allow_pickle=False)
    return {k: (np.array(0, dtype=np.int64) if k.endswith("num_batches_tracked")
                else np.ascontiguousarray(z[k], dtype=np.float32)) for k in z.files}


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("net_a")
    ap.add_argument("net_b")
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--sims", type=int, default=800)
    ap.add_argument("--opening-plies", type=int, default=4)
    ap.add_argument("--threads", type=int, default=2)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--temperature-moves", type=int, default=0)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp16"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    ap.add_argument("--adjudicate", type=int, default=0, metavar="K")
    ap.add_argument("--split", action="store_true")
    a = ap.parse_args()

    live_a, live_b = a.net_a.startswith("live:"), a.net_b.startswith("live:")
    sd_a = None if live_a else load_state(a.net_a)
    sd_b = load_state(a.net_b, sd_a)
    if sd_a is None:
        sd_a = load_state(a.net_a, None if live_b else sd_b)
    net_a = om.NativeNet(sd_a, device=0, dtype=a.dtype)
    net_b = om.NativeNet(sd_b, device=0, dtype=a.dtype)
    if net_a.history_size != net_b.history_size:
        raise SystemExit("the two nets have different history sizes: the arena shares one engine configuration")
    arena = om.Arena.create(a.games, seed=a.seed, history_size=net_a.history_size, num_simulations=a.sims,
                            num_threads=a.threads, batch_size=a.batch)
    arena.reset(openings=om.paired_openings(a.games, a.opening_plies, a.seed))
    c0 = [m.engine.work_counters() for m in (arena.a, arena.b)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = arena.play(net_a, net_b, temperature_moves=a.temperature_moves, adjudicate_empties=a.adjudicate,
                     split=a.split)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    c1 = [m.engine.work_counters() for m in (arena.a, arena.b)]
    sims = sum(x[0] - y[0] for x, y in zip(c1, c0))
    evals = sum(x[1] - y[1] for x, y in zip(c1, c0))
    w, d, lost = res.wdl()
    moves = int((res.actions >= 0).sum())
    out = {
        "net_a": a.net_a, "net_b": a.net_b, "games": a.games, "num_simulations": a.sims,
        "num_threads": a.threads, "batch_size": a.batch, "opening_plies": a.opening_plies,
        "temperature_moves": a.temperature_moves, "dtype": a.dtype, "seed": a.seed,
        "wins_a": w, "draws": d, "losses_a": lost, "score_a": res.score_a(), "plies": res.plies, "moves": moves,
        "wall_s": wall, "simulations": sims, "nn_rows": evals, "simulations_per_s": sims / wall,
        "nn_rows_per_s": evals / wall, "device": torch.cuda.get_device_name(0),
        "adjudicate_empties": a.adjudicate, "split": a.split, "margin": res.margin.tolist(),
        "adjudicated": res.adjudicated.tolist(), "mean_margin_a": float(res.margin_a().float().mean()),
        "records": res.records(a.net_a, a.net_b),
    }
    print(f"A {a.net_a} vs B {a.net_b}: {a.games} matches, {a.sims} simulations per move")
    print(f"W/D/L (A) {w}/{d}/{lost}  score {out['score_a']:.3f}  plies {res.plies}  moves {moves}  "
          f"adjudicated {int(res.adjudicated.sum())}  mean margin (A) {out['mean_margin_a']:+.2f}")
    print(f"wall {wall:.2f} s  {sims / wall / 1e6:.3f} M simulations/s  {evals / wall / 1e6:.3f} M NN rows/s")
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
