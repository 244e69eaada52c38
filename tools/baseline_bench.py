"""Throughput of the baseline opponents' depth-limited search:
seeded random-play positions at 30 empties, depths 2, 4 and 6, on the GPU
(warm-up, device events, median of 5) and the same positions through the host
twin on 16 worker processes.

    python tools/baseline_bench.py --out profiles/baseline/bench.json

The host figure is the SAME algorithm (csrc/baseline.h) on 16 CPU processes of
the GPU machine, nothing else; no ratio to any peak is claimed. longest_item:
the largest node count of one (position, root action), which one lane searches
alone, so a launch lasts at least that long.
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

NODE_LIMIT = 1 << 30


def _host(args):
    from othello_mcts import baseline_move

    triple, depth = args
    return baseline_move(triple, "search", depth, node_limit=NODE_LIMIT)["nodes"]


def _longest_item(om, pos, depth: int, total: int) -> int:
    """The largest node count of one (position, root action): node_limit is a
    budget per root action, so this is the smallest budget that flags nothing
    (bisected on the device)."""
    lo, hi = 1, total
    while lo < hi:
        mid = (lo + hi) // 2
        if bool(om.baseline_moves(pos, "search", depth, node_limit=mid).flags.any()):
            lo = mid + 1
        else:
            hi = mid
    return lo


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--empties", type=int, default=30)
    ap.add_argument("--positions", type=int, default=4096)
    ap.add_argument("--depths", default="2,4,6")
    ap.add_argument("--host-processes", type=int, default=16)
    ap.add_argument("--host-positions", type=int, default=0, help="0 = all of them")
    ap.add_argument("--no-host", action="store_true", help="GPU timing only")
    a = ap.parse_args()

    import torch

    import othello_mcts as om
    from othello_mcts import endgame as E

    ps = E.random_play_positions(a.empties, a.positions, a.seed + a.empties)
    triples = [(p.player(), p.player1_discs(), p.player2_discs()) for p in ps]
    pos = E.pack_positions(triples).cuda()
    results = []
    for depth in (int(x) for x in a.depths.split(",")):
        out = om.baseline_moves(pos, "search", depth, node_limit=NODE_LIMIT)  # warm-up
        assert not bool(out.flags.any())
        per_position = out.nodes.cpu()
        nodes = int(per_position.sum())
        ms = []
        for _ in range(a.repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            om.baseline_moves(pos, "search", depth, node_limit=NODE_LIMIT)
            t1.record()
            t1.synchronize()
            ms.append(t0.elapsed_time(t1))
            print(f"depth {depth}: run {len(ms)} {ms[-1]:.2f} ms", file=sys.stderr, flush=True)
        gpu_s = statistics.median(ms) / 1e3
        r = {"empties": a.empties, "positions": a.positions, "depth": depth, "nodes": nodes,
             "gpu_ms_runs": [round(x, 3) for x in ms], "gpu_ms_median": round(gpu_s * 1e3, 3),
             "gpu_positions_per_s": round(a.positions / gpu_s, 1), "gpu_nodes_per_s": round(nodes / gpu_s),
             "largest_position_nodes": int(per_position.max()),
             "longest_item_nodes": _longest_item(om, pos, depth, int(per_position.max()))}
        if not a.no_host:
            sub = triples[:a.host_positions] if a.host_positions else triples
            with mp.get_context("spawn").Pool(a.host_processes) as pool:
                pool.map(_host, [(t, depth) for t in sub[:a.host_processes]])  # start the workers
                t = time.perf_counter()
                host_nodes = sum(pool.map(_host, [(t_, depth) for t_ in sub], chunksize=4))
                host_s = time.perf_counter() - t
            if not a.host_positions:
                assert host_nodes == nodes, (host_nodes, nodes)
            r.update({"host_processes": a.host_processes, "host_positions": len(sub), "host_s": round(host_s, 3),
                      "host_positions_per_s": round(len(sub) / host_s, 1),
                      "host_nodes_per_s": round(host_nodes / host_s)})
        print(json.dumps(r), flush=True)
        results.append(r)
    rec = {"what": "baseline opponents, SEARCH: seeded random-play positions; GPU: device events, median of "
                   f"{a.repeats} after a warm-up; host: the same search on {a.host_processes} processes",
           "command": "python tools/baseline_bench.py " + " ".join(sys.argv[1:]),
           "device": torch.cuda.get_device_name(0), "node_limit": NODE_LIMIT, "results": results}
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
