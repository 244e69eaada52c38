"""Minibatch time of the packed ReplayBuffer against the fp32 SampleBuffer
(DESIGN.md §12): both are filled by the same self-play (G = 256, H = 8, a
128x1b net, 16 simulations per move: only the buffers are measured), then the
time to draw one minibatch of 256 random samples is taken for each,

  ReplayBuffer.gather(ids)                      one k_replay_gather launch
  features[idx], policies[idx], values[idx]     SampleBuffer, three index kernels

as the median of per-batch HIP event times over many batches, after checking
that the two give the same rows. The per-move cost of the two ``add`` paths is
reported as well (host clock around a synchronised loop over recorded moves).

Usage (GPU box): python tools/replay_gather_bench.py OUT.json [moves] [batches]
"""

import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "othello-alphazero_amd"))

import torch  # noqa: E402

import othello_mcts as om  # noqa: E402
from othello_mcts.synthetic import alphazero_state_dict  # noqa: E402


def event_times_ms(fn, batches, warmup=20):
    for i in range(warmup):
        fn(i)
    out = []
    for i in range(batches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn(i)
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def main():
    out_path = Path(sys.argv[1])
    moves = int(sys.argv[2]) if len(sys.argv) > 2 else 96
    batches = int(sys.argv[3]) if len(sys.argv) > 3 else 300
    G, H, B = 256, 8, 256
    dev = torch.device("cuda", 0)
    net = om.NativeNet(alphazero_state_dict(4, 17, 128, 1, 32), device=0)
    eng = om.BatchedMCTS(G, history_size=H, num_simulations=16, num_threads=1, batch_size=8, seed=3,
                         node_capacity=1 << 14)
    P = 1 << 15
    sb = om.SampleBuffer(G, 1 + 2 * H, capacity=8 * P, device=dev)
    rb = om.ReplayBuffer(G, H, P, device=dev)
    recorded = []
    for _ in range(moves // 16):
        o = eng.selfplay_steps(net, 16, emit_targets=True, keep_all=True)
        recorded.append(o)
    torch.cuda.synchronize()
    # add paths, per move (the same recorded outputs for both)
    t0 = time.perf_counter()
    for o in recorded:
        for i in range(16):
            sb.add({k: v[i] for k, v in o.items()})
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    for o in recorded:
        rb.add(o)
    t_enqueued = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    rb.check()
    n_moves = 16 * len(recorded)
    size = rb.size
    assert 8 * size == sb.size and size < P and size > 0, (size, sb.size)
    n = 8 * size
    # same rows
    ids = torch.arange(n, device=dev)
    for lo in range(0, n, 1 << 14):
        f, p, v = rb.gather(ids[lo:lo + (1 << 14)])
        hi = lo + f.shape[0]
        assert torch.equal(f, sb.features[lo:hi]) and torch.equal(p, sb.policies[lo:hi])
        assert torch.equal(v, sb.values[lo:hi])
    gen = torch.Generator(device=dev).manual_seed(1)
    idx = [torch.randint(0, n, (B,), device=dev, generator=gen) for _ in range(batches + 20)]
    torch.cuda.synchronize()
    t_gather = event_times_ms(lambda i: rb.gather(idx[i]), batches)
    t_index = event_times_ms(lambda i: (sb.features[idx[i]], sb.policies[idx[i]], sb.values[idx[i]]), batches)
    t_gather2 = event_times_ms(lambda i: rb.gather(idx[i]), batches)
    t_index2 = event_times_ms(lambda i: (sb.features[idx[i]], sb.policies[idx[i]], sb.values[idx[i]]), batches)

    def stats(x):
        q = statistics.quantiles(x, n=10)
        return {"median_ms": round(statistics.median(x), 5), "p10_ms": round(q[0], 5), "p90_ms": round(q[-1], 5)}

    sb_bytes = sum(t.numel() * t.element_size() for t in (sb.features, sb.policies, sb.values, sb._stage_f,
                                                           sb._stage_p, sb._moves))
    rec = {
        "what": "minibatch of 256 random samples, per-batch HIP event time; interleaved A B A B",
        "games": G, "history_size": H, "positions": size, "samples": n, "batch": B, "batches": batches,
        "replay_gather": [stats(t_gather), stats(t_gather2)],
        "sample_buffer_index": [stats(t_index), stats(t_index2)],
        "add_per_move_ms": {
            "moves": n_moves,
            "sample_buffer_add": round(1e3 * (t1 - t0) / n_moves, 4),
            "replay_add_host_enqueue": round(1e3 * (t_enqueued - t1) / n_moves, 4),
            "replay_add_until_done": round(1e3 * (t2 - t1) / n_moves, 4),
        },
        "bytes": {"replay_buffer": rb.nbytes, "sample_buffer_same_capacity": sb_bytes,
                  "ratio": round(sb_bytes / rb.nbytes, 1)},
        "rows_equal": True,
    }
    out_path.parent.mkdir(parents=True, exist_ok=True)
    out_path.write_text(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
