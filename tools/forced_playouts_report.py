"""Forced playouts and policy target pruning on self-play.

One self-play run with the feature on and one with it off, from the same seeds:
256 games, 800 simulations, T=2 x B=16, history 8, root noise 0.25, the net of
a checkpoint directory (the reference's config.json + neural_net.pth; history 8)
or the bench's self-play trained
128x10b net in bf16 (bench_nets/selfplay_128x10b_h8.npz).

Two passes per setting, each on a fresh engine:

  targets     MOVES x (search + selfplay_move), the root queried before every
              move (root_stats, root_priors): the raw visit counts, and with
              the feature on the pruned ones from othello_mcts.prune_visit_counts
              (the rule the device writes its targets with; the written policy
              is checked against it on the way).
  throughput  free-running selfplay_steps calls (warm-up, then timed, device
              events around each): simulations/s of the median call, from the
              engine's work counters.

Reported per setting: the share of visits pruned, the share of visited root
children zeroed, the mean entropy (nats) of the policy target before and after
pruning, the mean number of root children with at least one visit (and with a
nonzero target), and simulations/s; and the on / off simulations/s ratio.
Whether pruned targets train a better net is KataGo's claim and is not measured.

Usage (GPU box): python tools/forced_playouts_report.py [OUT.json] [k] [checkpoint_dir | -] [games] [moves]
"""

import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "othello-alphazero_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import othello_mcts as om  # noqa: E402
from othello_mcts.synthetic import selfplay_state_dict  # noqa: E402

H, SIMS, T, B = 8, 800, 2, 16
WARMUP, TIMED = 2, 5


def engine(G, k):
    b = om.BatchedMCTS(G, history_size=H, num_simulations=SIMS, num_threads=T, batch_size=B, dirichlet_epsilon=0.25,
                       seed=1)
    b.random_openings(8, seed=2)
    if k:
        b.set_forced_playouts(k)
    return b


def entropy(n: np.ndarray) -> float:
    p = n[n > 0].astype(np.float64) / n.sum()
    return float(-(p * np.log(p)).sum())


def targets(net, G, k, moves):
    """Raw and pruned counts of every searched root of `moves` moves."""
    b = engine(G, k)
    acc = dict(roots=0, visits=0, pruned_visits=0, visited=0, zeroed=0, kept=0, h_raw=0.0, h_target=0.0, mismatches=0)
    info = torch.empty((G, 8), dtype=torch.int64, device=b.device)
    for _ in range(moves):
        b.search(net)
        v, q = b.root_stats()
        b.engine.root_stats(0, 0, info.data_ptr())
        v, q, p, word = v.cpu().numpy(), q.cpu().numpy(), b.root_priors().cpu().numpy(), info[:, 5].cpu().numpy()
        legal = info[:, 3].cpu().numpy().astype(np.uint64)
        out = b.selfplay_move(opening_moves=8, emit_targets=True)
        pol = out["policy"][:, 0].cpu().numpy()
        fin = out["finished"].cpu().numpy()
        for g in range(G):
            nc, n_root = int(word[g] & 0xFFFFFFFF), int(word[g] >> 32)
            if nc == 0 or fin[g] & 4:
                continue
            acts = [s for s in range(64) if (int(legal[g]) >> (63 - s)) & 1] or [64]
            raw = v[g][acts].astype(np.int32)
            if raw.sum() == 0:
                continue
            kept = om.prune_visit_counts(n_root, raw, q[g][acts], p[g][acts], k=k) if k else raw
            want = kept.astype(np.float32) / np.float32(kept.sum())
            acc["mismatches"] += int(not np.array_equal(want, pol[g][acts]))
            acc["roots"] += 1
            acc["visits"] += int(raw.sum())
            acc["pruned_visits"] += int(raw.sum() - kept.sum())
            acc["visited"] += int((raw > 0).sum())
            acc["kept"] += int((kept > 0).sum())
            acc["zeroed"] += int(((kept == 0) & (raw > 0)).sum())
            acc["h_raw"] += entropy(raw)
            acc["h_target"] += entropy(kept)
    b.check_health()
    r = acc["roots"]
    return {"roots": r, "written_policy_mismatches": acc["mismatches"],
            "share_of_visits_pruned": acc["pruned_visits"] / acc["visits"],
            "share_of_visited_children_zeroed": acc["zeroed"] / acc["visited"],
            "mean_entropy_raw_counts": acc["h_raw"] / r, "mean_entropy_target": acc["h_target"] / r,
            "mean_children_visited": acc["visited"] / r, "mean_children_in_target": acc["kept"] / r}


def throughput(net, G, k, moves):
    b = engine(G, k)
    calls = []
    for i in range(WARMUP + TIMED):
        s0, _ = b.engine.work_counters()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        o = b.selfplay_steps(net, moves, opening_moves=8, emit_targets=True, keep_all=True)
        e1.record()
        torch.cuda.synchronize()
        b.check_health()
        s1, _ = b.engine.work_counters()
        if i >= WARMUP:
            calls.append((e0.elapsed_time(e1) / 1e3, s1 - s0))
        del o
    calls.sort()
    sec, sims = calls[len(calls) // 2]
    return {"seconds_all": [round(c[0], 4) for c in calls], "median_call_seconds": sec, "median_call_simulations": sims,
            "simulations_per_s": round(sims / sec)}


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "profiles" / "forced_playouts" / "report.json"
    k = float(sys.argv[2]) if len(sys.argv) > 2 else 2.0
    ckpt = sys.argv[3] if len(sys.argv) > 3 and sys.argv[3] != "-" else None
    G = int(sys.argv[4]) if len(sys.argv) > 4 else 256
    moves = int(sys.argv[5]) if len(sys.argv) > 5 else 16
    if ckpt:
        net = om.NativeNet.from_checkpoint(ckpt, device=0, dtype="bf16")
    else:
        net = om.NativeNet(selfplay_state_dict(), device=0, dtype="bf16")
    res = {"shape": {"games": G, "history_size": H, "num_simulations": SIMS, "num_threads": T, "batch_size": B,
                     "dirichlet_epsilon": 0.25, "moves": moves,
                     "net": ckpt or "bench_nets/selfplay_128x10b_h8 (bf16)"},
           "k": k, "warmup_calls": WARMUP, "timed_calls": TIMED, "device": torch.cuda.get_device_name(0), "runs": {}}
    for name, kk in (("off", 0.0), ("on", k)):
        res["runs"][name] = {**targets(net, G, kk, moves), **throughput(net, G, kk, moves)}
        print(name, json.dumps(res["runs"][name]), flush=True)
    res["simulations_per_s_on_over_off"] = round(res["runs"]["on"]["simulations_per_s"] /
                                                 res["runs"]["off"]["simulations_per_s"], 4)
    print("on / off simulations per s", res["simulations_per_s_on_over_off"])
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
