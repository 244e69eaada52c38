"""Train a 128x10b net by self-play on one MI355X, the reference's loop in
miniature (train.py:386-521: self-play games -> 8-fold samples with outcome
values -> SGD epochs; README.md:69-90 hyper-parameters: lr 0.02, momentum 0.9,
L2 1e-4, training batch 256, 800 sims, T=2 x B=16, eps 0.25, alpha 0.5,
temperature for the first 12 moves), with this package's pieces: the
on-device self-play driver (BatchedMCTS.selfplay_steps), the HBM sample buffer
(SampleBuffer), the reference loss (alphazero_loss / train_epoch) and the
native net refreshed after every epoch (refresh_native).

Purpose: a benchmark workload whose priors and values are coherent the way a
trained net's are (trees of a trained net concentrate and
descend deeper than those of any random init). Output: the trained state_dict
as float16 (npz, the reference's keys) + a JSON log of the iterations.

Usage (GPU box): python tools/selfplay_train.py OUT_PREFIX [iterations] [games] [seconds]
                 [packed [exact=K]] [adjudicate=K] [split] [cap=P:N] [budget=S] [forced=K] [exact_leaves=E]

packed: keep the samples in the packed ReplayBuffer (500,000 positions = 4
million samples in 0.2 GB, one add per selfplay_steps call, no host wait in the
self-play phase; minibatches expanded by train_epoch_replay) instead of the
fp32 SampleBuffer (400,000 samples in 1.85 GB, one add per move).

exact=K (with packed): after each self-play phase and before training, the
buffer's positions with at most K empties get the exact result of perfect play
as their value target (ReplayBuffer.relabel_endgames). The
iteration's log line gains relabel_ms (device events around the call) and the
buffer's relabel_stats. split (with exact=K): the split solver does the
relabelling (relabel_endgames(split=True)).

adjudicate=K: self-play games end at the searched move that leaves at most K
empties, with the exact result of that position (selfplay_steps(...,
adjudicate_empties=K); split: by the split solver). The log line
gains adjudicated (games the solver ended in the iteration), resolve_ms (device
events around the resolve step, mean over the iteration's selfplay_steps
calls; reading them waits for each call, a host wait the K = 0 run does not
have) and resolve_share (their sum over the self-play phase).

cap=P:N: playout cap randomization (BatchedMCTS.set_playout_cap(P, N), DESIGN.md
§17): a search is a full one (800 simulations, recorded) with probability P,
else N simulations, played but not recorded. budget=S: every selfplay_steps
call gives each game S nominal simulations instead of 16 moves
(selfplay_steps(sim_budget=S)); the call's slot count is the most moves S buys
(S / N rounded up with a cap, S / 800 without), 64 at the most.

forced=K: forced playouts at the root of full searches with factor K and policy
target pruning (BatchedMCTS.set_forced_playouts(K); KataGo: 2).
exact_leaves=E: the search solves leaves with at most E empties (1..10) instead
of asking the net (BatchedMCTS.set_exact_leaves(E)).

new_positions (packed) is the ring head's advance, valid while one iteration
stores fewer positions than the ring holds; new_games / selfplay_s and
new_positions / selfplay_s are the games/s and stored positions/s of a phase.
"""

import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "othello-alphazero_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import othello_mcts as om  # noqa: E402
from othello_mcts.synthetic import live_state_dict  # noqa: E402


class AZNet(torch.nn.Module):
    """AlphaZeroNet's layers and state_dict keys (neural_net.py:9-172), for
    training here: the reference module itself does not travel to the box."""

    def __init__(self, in_ch=17, C=128, R=9, hid=128):
        super().__init__()
        nn = torch.nn

        def cb():
            m = nn.Module()
            m.conv = nn.Conv2d(in_ch, C, 3, padding=1)
            m.norm = nn.BatchNorm2d(C)
            return m

        def rb():
            m = nn.Module()
            m.conv1, m.norm1 = nn.Conv2d(C, C, 3, padding=1), nn.BatchNorm2d(C)
            m.conv2, m.norm2 = nn.Conv2d(C, C, 3, padding=1), nn.BatchNorm2d(C)
            return m

        self.conv_block = cb()
        self.residual_blocks = nn.ModuleList([rb() for _ in range(R)])
        ph = nn.Module()
        ph.conv, ph.norm, ph.linear = nn.Conv2d(C, 2, 1), nn.BatchNorm2d(2), nn.Linear(128, 65)
        vh = nn.Module()
        vh.conv, vh.norm = nn.Conv2d(C, 1, 1), nn.BatchNorm2d(1)
        vh.linear1, vh.linear2 = nn.Linear(64, hid), nn.Linear(hid, 1)
        self.policy_head, self.value_head = ph, vh

    def forward(self, x):
        h = F.relu(self.conv_block.norm(self.conv_block.conv(x)))
        for b in self.residual_blocks:
            y = F.relu(b.norm1(b.conv1(h)))
            h = F.relu(b.norm2(b.conv2(y)) + h)
        p = F.relu(self.policy_head.norm(self.policy_head.conv(h)))
        p = torch.softmax(self.policy_head.linear(p.flatten(1)), dim=1)
        v = F.relu(self.value_head.norm(self.value_head.conv(h)))
        v = F.relu(self.value_head.linear1(v.flatten(1)))
        v = torch.tanh(self.value_head.linear2(v).squeeze(1))
        return {"policy": p, "value": v}


def main():
    out = Path(sys.argv[1])
    iterations = int(sys.argv[2]) if len(sys.argv) > 2 else 40
    G = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    packed = "packed" in sys.argv[5:]
    exact = [int(w[6:]) for w in sys.argv[5:] if w.startswith("exact=")]
    if exact and not packed:
        raise SystemExit("exact=K needs the packed buffer")
    adjudicate = [int(w[11:]) for w in sys.argv[5:] if w.startswith("adjudicate=")]
    K = adjudicate[0] if adjudicate else 0
    split = "split" in sys.argv[5:]
    if split and not (exact or K):
        raise SystemExit("split needs exact=K or adjudicate=K")
    cap = [w[4:].split(":") for w in sys.argv[5:] if w.startswith("cap=")]
    cap = (float(cap[0][0]), int(cap[0][1])) if cap else None
    budget = [int(w[7:]) for w in sys.argv[5:] if w.startswith("budget=")]
    budget = budget[0] if budget else 0
    forced = [float(w[7:]) for w in sys.argv[5:] if w.startswith("forced=")]
    forced = forced[0] if forced else None
    exact_leaves = [int(w[13:]) for w in sys.argv[5:] if w.startswith("exact_leaves=")]
    exact_leaves = exact_leaves[0] if exact_leaves else 0
    L = 2 * 16
    nominal_min = -(-(cap[1] if cap else 800) // L) * L  # the smallest search's nominal simulations
    slots = min(64, -(-budget // nominal_min)) if budget else 16
    moves_per_iter = 64
    torch.manual_seed(0)
    dev = torch.device("cuda", 0)
    sd0 = live_state_dict(2025, 17, 128, 9, 128)
    model = AZNet().to(dev)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd0.items()})
    native = om.NativeNet(sd0, device=0)
    opt = torch.optim.SGD(model.parameters(), lr=0.02, momentum=0.9)
    b = om.BatchedMCTS(G, history_size=8, num_simulations=800, num_threads=2, batch_size=16,
                       dirichlet_epsilon=0.25, dirichlet_alpha=0.5, seed=77)
    b.reset()
    if cap:
        b.set_playout_cap(*cap)
    if forced:
        b.set_forced_playouts(forced)
    if exact_leaves:
        b.set_exact_leaves(exact_leaves)  # right after the reset: no tree built yet
    if packed:
        buf = om.ReplayBuffer(G, 8, capacity=500_000, device=dev, track_exact=bool(exact))
    else:
        buf = om.SampleBuffer(G, 17, capacity=400_000, device=dev)
    log = []
    t_start = time.time()
    gen = torch.Generator().manual_seed(1)
    for it in range(iterations):
        t0 = time.time()
        games0, size0 = buf.games_completed, (buf.head if packed else buf.size)
        adjudicated = None
        resolve_ms = []
        if K and it == 0:
            b.engine.adjudicate_ms()  # switches the resolve step's events on
        for _ in range(moves_per_iter // 16):  # 16 moves per call: bounded output buffers
            o = b.selfplay_steps(native, slots, temperature_moves=12, opening_moves=0, emit_targets=True,
                                 keep_all=True, adjudicate_empties=K, split=split and K > 0, sim_budget=budget)
            if K:
                n_adj = ((o["finished"] & 32) != 0).sum()  # stays on the device until the phase is over
                adjudicated = n_adj if adjudicated is None else adjudicated + n_adj
                o = {k: v for k, v in o.items() if k != "margin"}
                resolve_ms.append(b.engine.adjudicate_ms()[0])
            if packed:
                buf.add(o)
            else:
                for i in range(slots):
                    buf.add({k: v[i] for k, v in o.items()})
        torch.cuda.synchronize()
        t1 = time.time()
        selfplay_s = round(t1 - t0, 2)
        adj = {}
        if K:
            adj = {"adjudicated": int(adjudicated), "resolve_ms": round(sum(resolve_ms) / len(resolve_ms), 3),
                   "resolve_ms_calls": [round(x, 3) for x in resolve_ms],
                   "resolve_share": round(sum(resolve_ms) / 1e3 / max(t1 - t0, 1e-9), 5)}
        relabel = {}
        if exact:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            buf.relabel_endgames(exact[0], split=split)
            e1.record()
            stats = buf.relabel_stats  # the iteration's one host wait for the relabel
            relabel = {"relabel_ms": round(e0.elapsed_time(e1), 2), "relabel": stats}
            t1 = time.time()  # train_s starts after the relabel
        if packed:
            buf.check()
            n = 8 * buf.size
            losses = om.train_epoch_replay(model, opt, buf, 256, l2_weight=1e-4, generator=gen)
        else:
            n = buf.size
            losses = om.train_epoch(model, opt, buf.features[:n], buf.policies[:n], buf.values[:n], 256,
                                    l2_weight=1e-4, generator=gen)
        model.eval()
        om.refresh_native(native, model)
        torch.cuda.synchronize()
        rec = {"iteration": it, "games": buf.games_completed, "new_games": buf.games_completed - games0,
               "samples": n, "new_positions": ((buf.head - size0) % buf.capacity if packed else (buf.size - size0) // 8),
               "selfplay_s": selfplay_s, "train_s": round(time.time() - t1, 2), **adj, **relabel, **{k: round(v, 4) for k, v in losses.items()}}
        log.append(rec)
        print(json.dumps(rec), flush=True)
        if time.time() - t_start > (float(sys.argv[4]) if len(sys.argv) > 4 else 900.0):
            break
    sd = {k: v.detach().float().cpu().numpy() for k, v in model.state_dict().items()}
    np.savez_compressed(str(out) + ".npz", **{k: (v.astype(np.float16) if v.dtype == np.float32 else v)
                                             for k, v in sd.items()})
    Path(str(out) + ".json").write_text(json.dumps({"iterations": log, "games_per_engine": G,
                                                    "moves_per_iteration": moves_per_iter,
                                                    "buffer": "packed" if packed else "fp32",
                                                    "exact_max_empties": exact[0] if exact else None,
                                                    "exact_split": split and bool(exact),
                                                    "adjudicate_empties": K, "adjudicate_split": split and K > 0,
                                                    "playout_cap": cap, "sim_budget": budget, "slots_per_call": slots,
                                                    "forced_playouts": forced, "exact_leaves": exact_leaves},
                                                   indent=1))


if __name__ == "__main__":
    main()
