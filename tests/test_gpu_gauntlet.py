"""Gauntlet (othello_mcts.baseline): G matches of one net against a baseline
opponent, replayed ply by ply on host Positions: legality, the net's argmax
pick, the baseline's pick against the host twin, the roots after every move,
and play() against the stepped loop."""

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = 8
H = 3
KW = dict(history_size=H, num_simulations=32, num_threads=2, batch_size=8, node_capacity=1 << 15,
          dirichlet_epsilon=0.0)
SEED = 5


@pytest.fixture(scope="module")
def net():
    import othello_mcts as om
    from othello_mcts.synthetic import alphazero_state_dict

    return om.NativeNet(alphazero_state_dict(11, 1 + 2 * H, 128, 2, 32), device=0, dtype="bf16")


def root(m, g):
    i = m.root_info(g)
    return i["player"], i["player1_discs"], i["player2_discs"]


def fields(p):
    return p.player(), p.player1_discs(), p.player2_discs()


@pytest.mark.parametrize("kind,depth,net_white", [("greedy", 1, None), ("search", 2, [True, False] * 4)])
def test_gauntlet_replays_on_the_host(net, kind, depth, net_white):
    import othello_mcts as om
    from othello_mcts import baseline as B

    m = om.BatchedMCTS(G, seed=SEED, **KW)
    gauntlet = om.Gauntlet(m, kind, depth, seed=SEED)
    openings = om.paired_openings(G, 4, SEED)
    gauntlet.reset(net_is_white=net_white)  # the default openings are these
    white = np.arange(G) % 2 == 1 if net_white is None else np.array(net_white)
    assert gauntlet.net_is_white.tolist() == white.tolist()
    pos = []
    for g in range(G):
        p = om.Position.initial_position()
        for a in openings[g]:
            p = p.apply_action(int(a))
        pos.append(p)
        assert root(m, g) == fields(p)
    keys = [B.gauntlet_key(SEED, g) for g in range(G)]
    assert gauntlet.keys.tolist() == keys and len(set(keys)) == G
    played, ply_of = [], [0] * G
    net_plies = base_plies = 0
    while not all(p.is_terminal() for p in pos):
        assert len(played) < 80
        counts = [m.root_info(g)["visit_count"] for g in range(G)]
        out = gauntlet.move(net)
        acts, moved, fin = (out[k].cpu().tolist() for k in ("actions", "net_moved", "finished"))
        visits = out["visits"].cpu().numpy()
        played.append(acts)
        for g in range(G):
            p = pos[g]
            if p.is_terminal():
                assert acts[g] == -1 and not moved[g] and fin[g]
                continue
            assert acts[g] in p.legal_actions(), (len(played), g)
            assert moved[g] == ((p.player() == 2) == bool(white[g]))
            if moved[g]:
                legal = p.legal_actions()
                assert visits[g].sum() == visits[g][legal].sum() >= KW["num_simulations"] // 2
                assert visits[g][acts[g]] == visits[g][legal].max()
                net_plies += 1
            else:
                want = om.baseline_move(p, kind, depth, key=keys[g], event=ply_of[g])
                assert want["flags"] == 0 and acts[g] == want["action"], (len(played), g)
                # the tree of a match whose mover is the baseline was not searched
                assert visits[g].sum() <= counts[g]
                base_plies += 1
            pos[g] = p.apply_action(acts[g])
            ply_of[g] += 1
            assert root(m, g) == fields(pos[g]), (len(played), g)
            assert fin[g] == pos[g].is_terminal()
    assert net_plies > 60 and base_plies > 60
    m.check_health()
    # one more ply moves nothing
    assert (gauntlet.move(net)["actions"].cpu() == -1).all()

    # play() on a fresh gauntlet with the same seed: the same matches
    m2 = om.BatchedMCTS(G, seed=SEED, **KW)
    g2 = om.Gauntlet(m2, kind, depth, seed=SEED)
    g2.reset(net_is_white=net_white)
    res = g2.play(net)
    assert res.plies == len(played) and res.actions.tolist() == played
    discs = [[bin(p.player1_discs()).count("1"), bin(p.player2_discs()).count("1")] for p in pos]
    assert res.discs.tolist() == discs
    assert res.margin.tolist() == [b - w for b, w in discs]
    assert res.result.tolist() == [0 if b == w else 1 if b > w else 2 for b, w in discs]
    assert res.a_is_white.tolist() == white.tolist() and not res.adjudicated.any()
    name = "greedy" if kind == "greedy" else f"search-{depth}"
    assert g2.baseline_id == name
    recs = res.records("net", g2.baseline_id)
    assert len(recs) == G
    for g, r in enumerate(recs):
        assert r["player1"] == (name if white[g] else "net") and r["player2"] == ("net" if white[g] else name)
        assert r["result"] == res.result[g]
    w, d, l = res.wdl()
    net_margin = [(w_ - b) if white[g] else (b - w_) for g, (b, w_) in enumerate(discs)]
    assert (w, d, l) == (sum(x > 0 for x in net_margin), sum(x == 0 for x in net_margin),
                         sum(x < 0 for x in net_margin))
    assert res.margin_a().tolist() == net_margin
    assert res.score_a() == (w + 0.5 * d) / G
    # play() begins new matches by itself, and stops at max_plies with the rest unfinished
    short = g2.play(net, max_plies=3)
    assert short.plies == 3 and (short.result == -1).all()
    if net_white is None:
        assert short.actions.tolist() == played[:3]


def test_gauntlet_rejects_unfit_engines_and_arguments(net):
    import othello_mcts as om

    kw = {k: v for k, v in KW.items() if k != "dirichlet_epsilon"}
    with pytest.raises(ValueError, match="root noise"):
        om.Gauntlet(om.BatchedMCTS(2, dirichlet_epsilon=0.25, **kw), "greedy")
    m = om.BatchedMCTS(2, **KW)
    m.set_exact_leaves(4)
    with pytest.raises(ValueError, match="exact leaves"):
        om.Gauntlet(m, "greedy")
    m.set_exact_leaves(None)
    m.set_playout_cap(0.5, 8)
    with pytest.raises(ValueError, match="playout cap"):
        om.Gauntlet(m, "greedy")
    m.set_playout_cap(None, None)
    m.set_forced_playouts(2.0)
    with pytest.raises(ValueError, match="forced playouts"):
        om.Gauntlet(m, "greedy")
    m.set_forced_playouts(None)
    g = om.Gauntlet(m, "random")
    assert g.baseline_id == "random"
    with pytest.raises(RuntimeError, match="before Gauntlet.reset"):
        g.move(net)
    m.set_forced_playouts(2.0)  # set after the gauntlet was made: caught when matches begin
    with pytest.raises(ValueError, match="forced playouts"):
        g.reset()
    m.set_forced_playouts(None)
    with pytest.raises(ValueError):
        om.Gauntlet(m, "search", 11)
    with pytest.raises(ValueError):
        om.Gauntlet(m, "engine")
    a0 = int(om.paired_openings(2, 1, 0)[0][0])
    with pytest.raises(ValueError, match="padding"):
        g.reset(openings=[[a0, -1, a0], [a0, -1, -1]])
    with pytest.raises(Exception):
        g.reset(openings=[[0, -1], [a0, -1]])  # an illegal opening action
    # random against the net: a finished result with both colours
    g.reset()
    res = g.play(net)
    assert (res.result >= 0).all() and res.a_is_white.tolist() == [False, True]
    assert len(res.records("net", "random")) == 2
