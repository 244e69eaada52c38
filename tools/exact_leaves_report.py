"""Exact leaf values on self-play: what they buy in move quality
and what they cost or save in throughput.

For E = 0 (off) and a few values of E, from the same seeds and openings, the
bench's self-play trained 128x10b net in bf16 (bench_nets/selfplay_128x10b_h8),
256 games, 800 simulations, T=2 x B=16, history 8. Two passes per setting, each
on a fresh engine:

  accuracy    the machinery of tools/endgame_accuracy.py: play as AlphaZeroPlayer
              does (no root noise, argmax moves, 4 random opening plies) until
              GAMES games have finished; every root with at most 14 empties is
              solved exactly (the split solver) before the move and
              endgame_move_loss judges the move. Reported at 12 and at 14
              empties, where every leaf of the search sits a few plies above
              the exact leaves: positions, share of optimal moves, share with
              the win/draw/loss kept, mean disc loss.
  throughput  free-running selfplay_steps calls with root noise 0.25 from random
              openings (warm-up, then timed, device events around each):
              sustained simulations/s over the timed calls together and of the
              median call, NN rows per finished game, and the three counters
              (solves, hits, solver nodes) per finished game.

The solve kernel's share of the time comes from a kernel trace of one
throughput pass (events around the solve launches would serialise the group
streams they sit on):

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o t -- \
        python tools/exact_leaves_report.py --only-throughput E
    python tools/exact_leaves_report.py --kernel-stats DIR/.../t_kernel_stats.csv

--only-throughput E runs one throughput pass (warm-up and timed calls) and
nothing else; --kernel-stats reduces the trace's per-kernel statistics to the
calls, total and longest duration and share of all kernel time of the solve,
tree and ResNet kernels (profiles/exact_leaves/placement_and_trace.json).

Usage (GPU box): python tools/exact_leaves_report.py [--out OUT.json] [--E 4 6 8 10] [--games 256] [--moves 16]
"""

import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "othello-alphazero_amd"))

import torch  # noqa: E402

import othello_mcts as om  # noqa: E402
from othello_mcts.synthetic import selfplay_state_dict  # noqa: E402

H, SIMS, T, B = 8, 800, 2, 16
WARMUP, TIMED = 2, 5
SOLVE_EMPTIES, NODE_LIMIT = 14, 1 << 27
JUDGED = (12, 14)


def engine(G, E, eps, opening):
    b = om.BatchedMCTS(G, history_size=H, num_simulations=SIMS, num_threads=T, batch_size=B, dirichlet_epsilon=eps,
                       seed=1)
    b.random_openings(opening, seed=2)
    if E:
        b.set_exact_leaves(E)
    return b


def accuracy(net, G, E):
    """tools/endgame_accuracy.py's loop; the rows of 12 and 14 empties."""
    b = engine(G, E, 0.0, 4)
    dev = b.device
    stats = torch.zeros((SOLVE_EMPTIES + 1, 4), dtype=torch.int64, device=dev)
    totals = torch.zeros(2, dtype=torch.int64, device=dev)  # games finished, unsolved roots
    finished = moves = 0
    while finished < G:
        for _ in range(8):  # one host read per 8 moves
            roots = b.root_positions()
            sol = om.solve_endgames(roots, SOLVE_EMPTIES, NODE_LIMIT, split=True)
            b.search(net, sync=False)
            out = b.selfplay_move(temperature_moves=0, opening_moves=4)
            loss, kept, empties = om.endgame_move_loss(roots, out["actions"], SOLVE_EMPTIES, solution=sol)
            judged = loss >= 0
            e = empties.clamp(0, SOLVE_EMPTIES)
            row = torch.stack([judged, judged & (loss == 0), judged & (kept == 1), loss.clamp(min=0)], 1).to(torch.int64)
            stats.index_add_(0, e, row)
            totals[0] += ((out["finished"] & 3) != 0).sum()
            totals[1] += ((sol.flags & ~om.endgame.FLAG_TOO_MANY_EMPTIES) != 0).sum()
            moves += 1
        finished = int(totals[0])
    b.check_health()
    s = stats.cpu().numpy()
    rows = {}
    for e in JUDGED:
        n = int(s[e, 0])
        rows[str(e)] = {"positions": n, "optimal": round(s[e, 1] / n, 4), "wdl_kept": round(s[e, 2] / n, 4),
                        "mean_disc_loss": round(s[e, 3] / n, 4)}
    return {"move_loss_at_empties": rows, "games_finished": finished, "moves_per_game_slot": moves,
            "unsolved_roots": int(totals[1]), "counters": b.exact_leaf_counters()}


def throughput(net, G, E, moves):
    b = engine(G, E, 0.25, 8)
    calls = []
    games = rows = sims = 0
    c0 = b.exact_leaf_counters()
    for i in range(WARMUP + TIMED):
        if i == WARMUP:
            c0 = b.exact_leaf_counters()
        s0, r0 = b.engine.work_counters()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        o = b.selfplay_steps(net, moves, opening_moves=8, emit_targets=True, keep_all=True)
        e1.record()
        torch.cuda.synchronize()
        b.check_health()
        s1, r1 = b.engine.work_counters()
        if i >= WARMUP:
            calls.append((e0.elapsed_time(e1) / 1e3, s1 - s0))
            games += int(((o["finished"] & 3) != 0).sum())
            rows += r1 - r0
            sims += s1 - s0
        del o
    c1 = b.exact_leaf_counters()
    total = sum(c[0] for c in calls)
    med = sorted(calls)[len(calls) // 2]
    per_game = {k: round((c1[k] - c0[k]) / max(games, 1), 1) for k in c1}
    return {"seconds_all": [round(c[0], 4) for c in calls], "simulations": sims,
            "simulations_per_s_sustained": round(sims / total), "simulations_per_s_median_call": round(med[1] / med[0]),
            "games_finished": games, "nn_rows": rows, "nn_rows_per_game": round(rows / max(games, 1), 1),
            "nn_rows_per_simulation": round(rows / sims, 4), "counters_per_game": per_game,
            "counters": {k: c1[k] - c0[k] for k in c1}}


def kernel_shares(stats_csv):
    """rocprofv3's per-kernel statistics -> the solve, tree and ResNet kernels' rows."""
    import csv

    rows = list(csv.DictReader(open(stats_csv)))
    total = sum(float(x["TotalDurationNs"]) for x in rows)
    out = {}
    for x in rows:
        if any(k in x["Name"] for k in ("k_solve_leaves", "k_tree_free", "k_resnet")):
            out[x["Name"][:60]] = {"calls": int(x["Calls"]), "total_ms": round(float(x["TotalDurationNs"]) / 1e6, 2),
                                   "avg_us": round(float(x["AverageNs"]) / 1e3, 2),
                                   "max_us": round(float(x["MaxNs"]) / 1e3, 1),
                                   "share_of_kernel_time": round(float(x["TotalDurationNs"]) / total, 4)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "exact_leaves" / "report.json"))
    ap.add_argument("--E", type=int, nargs="*", default=[4, 6, 8, 10])
    ap.add_argument("--games", type=int, default=256)
    ap.add_argument("--moves", type=int, default=16)
    ap.add_argument("--only-throughput", type=int, default=None, metavar="E")
    ap.add_argument("--kernel-stats", default=None, metavar="CSV")
    a = ap.parse_args()
    if a.kernel_stats:
        print(json.dumps(kernel_shares(a.kernel_stats), indent=1))
        return
    net = om.NativeNet(selfplay_state_dict(), device=0, dtype="bf16")
    if a.only_throughput is not None:
        print(json.dumps({"E": a.only_throughput, **throughput(net, a.games, a.only_throughput, a.moves)}))
        return
    res = {"shape": {"games": a.games, "history_size": H, "num_simulations": SIMS, "num_threads": T, "batch_size": B,
                     "moves_per_call": a.moves, "net": "bench_nets/selfplay_128x10b_h8 (bf16)",
                     "accuracy": "no root noise, argmax moves, 4 opening plies, roots of <= 14 empties solved (split)",
                     "throughput": "root noise 0.25, openings of up to 8 plies, free-running selfplay_steps"},
           "warmup_calls": WARMUP, "timed_calls": TIMED, "device": torch.cuda.get_device_name(0), "runs": {}}
    for E in [0, *a.E]:
        res["runs"][str(E)] = {"accuracy": accuracy(net, a.games, E), "throughput": throughput(net, a.games, E, a.moves)}
        print(E, json.dumps(res["runs"][str(E)]), flush=True)
    off = res["runs"]["0"]["throughput"]["simulations_per_s_sustained"]
    res["sustained_simulations_per_s_over_off"] = {
        k: round(v["throughput"]["simulations_per_s_sustained"] / off, 4) for k, v in res["runs"].items()}
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
