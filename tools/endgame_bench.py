"""Throughput of the exact endgame solver: seeded random-play
positions at 10, 12 and 14 empties on the GPU (warm-up, device events, median
of 5) and the same positions through the host solver on 16 worker processes.

    python tools/endgame_bench.py --out profiles/endgame/solver_bench.json
    python tools/endgame_bench.py --split ...     # the split solver, host twin included

The GPU / CPU ratio is against the SAME algorithm (csrc/solver.h) on 16 CPU
processes of the GPU machine, nothing else; no share of any peak is claimed.
"""

from __future__ import annotations

import argparse
import json
import multiprocessing as mp
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "othello-alphazero_amd"))

CASES = "10:4096,12:4096,14:1024"
NODE_LIMIT = 1 << 30


def _host(args):
    from othello_mcts import solve_position

    triple, empties, split = args
    return solve_position(triple, empties, NODE_LIMIT, split=split)["nodes"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-processes", type=int, default=16)
    ap.add_argument("--host-positions", type=int, default=0, help="0 = all of them")
    ap.add_argument("--cases", default=CASES, help="EMPTIES:POSITIONS,... (a case can be run on its own: one lane "
                    "searches one root action, so a run lasts as long as its largest root action)")
    ap.add_argument("--split", action="store_true", help="the split solver (solve_endgames(split=True))")
    ap.add_argument("--no-host", action="store_true", help="GPU timing only")
    a = ap.parse_args()

    import torch

    import othello_mcts as om
    from othello_mcts import endgame as E

    results = []
    for empties, count in (tuple(int(x) for x in c.split(":")) for c in a.cases.split(",")):
        ps = E.random_play_positions(empties, count, a.seed + empties)
        triples = [(p.player(), p.player1_discs(), p.player2_discs()) for p in ps]
        pos = E.pack_positions(triples).cuda()
        sol = om.solve_endgames(pos, empties, NODE_LIMIT, split=a.split)  # warm-up
        sol.check()
        nodes = int(sol.nodes.sum())
        ms = []
        for _ in range(a.repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            om.solve_endgames(pos, empties, NODE_LIMIT, split=a.split)
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
            print(f"empties {empties}: run {len(ms)} {ms[-1]:.1f} ms", file=sys.stderr, flush=True)
        gpu_s = statistics.median(ms) / 1e3
        r = {"empties": empties, "positions": count, "split": a.split, "nodes": nodes,
             "gpu_ms_runs": [round(x, 3) for x in ms], "gpu_ms_median": round(gpu_s * 1e3, 3),
             "gpu_positions_per_s": round(count / gpu_s, 1), "gpu_nodes_per_s": round(nodes / gpu_s)}
        if a.no_host:
            print(json.dumps(r), flush=True)
            results.append(r)
            continue
        sub = triples[:a.host_positions] if a.host_positions else triples
        with mp.get_context("spawn").Pool(a.host_processes) as pool:
            pool.map(_host, [(t, empties, a.split) for t in sub[:a.host_processes]])  # start the workers
            t = time.perf_counter()
            host_nodes = sum(pool.map(_host, [(t_, empties, a.split) for t_ in sub], chunksize=4))
            host_s = time.perf_counter() - t
        if not a.host_positions:
            assert host_nodes == nodes, (host_nodes, nodes)
        r.update({"host_processes": a.host_processes, "host_positions": len(sub), "host_s": round(host_s, 3),
                  "host_positions_per_s": round(len(sub) / host_s, 1), "host_nodes_per_s": round(host_nodes / host_s),
                  "gpu_over_host_nodes_per_s": round((nodes / gpu_s) / (host_nodes / host_s), 2)})
        print(json.dumps(r), flush=True)
        results.append(r)
    out = {"what": ("split " if a.split else "") + "exact endgame solver, seeded random-play positions; GPU: device events, median of "
                   f"{a.repeats} after a warm-up; host: the same solver on {a.host_processes} processes",
           "command": "python tools/endgame_bench.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "node_limit": NODE_LIMIT, "results": results}
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
