"""On-device arena (othello_mcts.Arena, csrc/arena.hip k_arena_begin /
k_arena_move) against the CPU reference match (tests/arena_ref.py), the fused
call against the step-wise loop, and the per-game search mask."""

import numpy as np
import pytest
import torch

import arena_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _t(fn):
    def ev(features):
        p, v = fn(features.cpu().numpy())
        return {"policy": torch.from_numpy(p), "value": torch.from_numpy(v)}

    return ev


STUB_A, STUB_B = _t(R.stub_a), _t(R.stub_b)


def _root(m, g):
    i = m.root_info(g)
    return i, (i["player"], i["player1_discs"], i["player2_discs"], i["legal_moves"], i["next_legal_moves"])


@pytest.mark.parametrize("temperature_moves", [0, 6])
def test_arena_matches_equal_the_reference_ply_by_ply(temperature_moves):
    """Eight matches with callable evaluators, driven by search / move: before
    every move the mover's root visits and Q equal the oracle's bit for bit and
    the other tree was not touched by the ply's search (the mask); after it
    both roots are the oracle's position; actions, lengths, results and discs
    are the reference's."""
    _matches_equal_the_reference(temperature_moves, R.reference_matches(temperature_moves), STUB_A, STUB_B)


def test_arena_matches_equal_the_reference_with_asymmetric_evaluators():
    """The same, with two evaluators that see the per-leaf board symmetry
    (tests/asym_stub.py; both default stubs are equivariant, so a wrong draw or
    un-transform in either engine's stream is invisible above)."""
    import asym_stub as A

    ref = R.reference_matches(0, A.asymmetric_stub_a, A.asymmetric_stub_b)
    assert ref != R.reference_matches(0)
    _matches_equal_the_reference(0, ref, _t(A.asymmetric_stub_a), _t(A.asymmetric_stub_b))


def _matches_equal_the_reference(temperature_moves, ref, STUB_A, STUB_B):
    import othello_mcts as om

    G = R.MATCHES
    arena = om.Arena.create(G, seed=0, node_capacity=1 << 16, **{k: v for k, v in R.SETUP.items()
                                                                  if k != "dirichlet_epsilon"})
    assert arena.a.config.dirichlet_epsilon == 0.0 and arena.b.config.dirichlet_epsilon == 0.0
    arena.reset(openings=R.openings(), a_is_white=R.swapped())
    for g in range(G):
        assert arena.a.engine.game_key(g) == R.game_key(0, g)
        assert arena.b.engine.game_key(g) == R.game_key(1, g)
    longest = max(len(m["plies"]) for m in ref)
    played = []
    for ply in range(longest):
        live = [g for g in range(G) if ply < len(ref[g]["plies"])]
        before = {g: (_root(arena.a, g), _root(arena.b, g)) for g in range(G)}
        for g in live:
            assert before[g][0][1] == before[g][1][1] == ref[g]["plies"][ply]["before"], (ply, g)
        (sa, _), (sb, _) = arena.search(STUB_A, STUB_B)
        assert sa == 64 * sum(ref[g]["plies"][ply]["a_moves"] for g in live), ply
        assert sb == 64 * sum(not ref[g]["plies"][ply]["a_moves"] for g in live), ply
        va, qa = (x.cpu().numpy() for x in arena.a.root_stats())
        vb, qb = (x.cpu().numpy() for x in arena.b.root_stats())
        for g in range(G):
            ia, ib = _root(arena.a, g)[0], _root(arena.b, g)[0]
            p = ref[g]["plies"][ply] if g in live else None
            idle = [(ia, before[g][0][0]), (ib, before[g][1][0])]
            if p is not None:
                v, q = (va, qa) if p["a_moves"] else (vb, qb)
                assert v[g][p["legal"]].tolist() == p["visits"], (ply, g)
                assert v[g].sum() == sum(p["visits"])
                np.testing.assert_array_equal(q[g][p["legal"]], np.array(p["q"], np.float32), err_msg=f"{ply} {g}")
                idle.pop(0 if p["a_moves"] else 1)
            for now, was in idle:  # the side that does not move (both, once the match is over)
                assert (now["visit_count"], now["node_count"]) == (was["visit_count"], was["node_count"]), (ply, g)
        out = arena.move(temperature_moves=temperature_moves, temperature=1.0)
        acts = out["actions"].cpu().numpy()
        played.append(acts.copy())
        for g in range(G):
            if g in live:
                p = ref[g]["plies"][ply]
                assert acts[g] == p["action"], (ply, g, acts[g], p)
                assert _root(arena.a, g)[1] == _root(arena.b, g)[1] == p["after"], (ply, g)
            else:
                assert acts[g] == -1, (ply, g)
    status = out["finished"].cpu().numpy()
    discs = out["discs"].cpu().numpy()
    assert (status & ~3 == 0).all(), status  # no unexpanded root, overflow or desync
    assert (status & 3).tolist() == [m["result"] + 1 for m in ref]
    assert discs.tolist() == [list(m["discs"]) for m in ref]
    lengths = [int((np.array(played)[:, g] >= 0).sum()) for g in range(G)]
    assert lengths == [len(m["plies"]) for m in ref]
    # everything is over: one more ply searches nothing and moves nothing
    (sa, ea), (sb, eb) = arena.search(STUB_A, STUB_B)
    assert (sa, ea, sb, eb) == (0, 0, 0, 0)
    assert (arena.move()["actions"].cpu().numpy() == -1).all()
    # Arena.play over the same matches gives the same result object
    arena.reset(openings=R.openings(), a_is_white=R.swapped())
    res = arena.play(STUB_A, STUB_B, temperature_moves=temperature_moves)
    assert res.plies == longest and res.actions.shape == (longest, G)
    np.testing.assert_array_equal(res.actions.numpy(), np.array(played))
    assert res.result.tolist() == [m["result"] for m in ref]
    assert res.discs.tolist() == [list(m["discs"]) for m in ref]
    wins = sum((m["result"] == 2) == bool(R.swapped()[g]) and m["result"] != 0 for g, m in enumerate(ref))
    draws = sum(m["result"] == 0 for m in ref)
    assert res.wdl() == (wins, draws, G - wins - draws)


# ------------------------------------------------------------------ native nets
H2 = 3
KW2 = dict(history_size=H2, num_simulations=32, num_threads=2, batch_size=8, node_capacity=1 << 15)
C_KEY = 0x632BE59BD9B4E019


@pytest.fixture(scope="module")
def native_nets():
    import othello_mcts as om
    from othello_mcts.synthetic import alphazero_state_dict

    return (om.NativeNet(alphazero_state_dict(11, 1 + 2 * H2, 128, 2, 32), device=0, dtype="bf16"),
            om.NativeNet(alphazero_state_dict(12, 1 + 2 * H2, 128, 2, 32), device=0, dtype="bf16"))


@pytest.fixture(scope="module")
def stepped_games(native_nets):
    """64 matches played by the search / move loop, with the mover's root
    visits of every ply (shared by the tests below, not modified)."""
    import othello_mcts as om

    net_a, net_b = native_nets
    G = 64
    arena = om.Arena.create(G, seed=7, **KW2)
    ops = om.paired_openings(G, 4, seed=7)
    arena.reset(openings=ops)
    white = arena.a_is_white.numpy().copy()
    actions, visits = [], []
    status = np.zeros(G, np.int32)
    while ((status & 3) == 0).any():
        assert len(actions) < 80
        arena.search(net_a, net_b)
        va = arena.a.root_stats()[0].cpu().numpy()
        vb = arena.b.root_stats()[0].cpu().numpy()
        out = arena.move()
        acts = out["actions"].cpu().numpy().copy()
        status = out["finished"].cpu().numpy().copy()
        actions.append(acts)
        visits.append((va, vb))
    return dict(openings=ops, white=white, actions=np.array(actions), visits=visits, status=status,
                discs=out["discs"].cpu().numpy().copy())


def test_fused_play_equals_the_stepped_loop(native_nets, stepped_games):
    import othello_mcts as om

    net_a, net_b = native_nets
    s = stepped_games
    assert (s["status"] & ~3 == 0).all() and ((s["status"] & 3) != 0).all()
    assert (s["white"] == (np.arange(64) % 2 == 1)).all()
    arena = om.Arena.create(64, seed=7, **KW2)
    arena.reset(openings=s["openings"])
    res = arena.play(net_a, net_b)
    np.testing.assert_array_equal(res.actions.numpy(), s["actions"])
    assert res.plies == len(s["actions"])
    assert res.result.tolist() == ((s["status"] & 3) - 1).tolist()
    assert res.discs.tolist() == s["discs"].tolist()
    assert len(res.records("a", "b")) == 64 and sum(res.wdl()) == 64
    # finished: a search of either engine is a no-op
    assert arena.a.search(net_a) == (0, 0) and arena.b.search(net_b) == (0, 0)
    # reset reactivates: a plain search again covers every game
    arena.a.reset()
    assert arena.a.search(net_a)[0] == 64 * KW2["num_simulations"]


@pytest.mark.parametrize("g", [0, 31, 32, 63])
def test_arena_match_equals_two_single_game_searches(native_nets, stepped_games, g):
    """Match g replayed with two one-game engines holding the same random
    streams (game keys): at every ply the mover's engine, searched with the
    same net, has the arena's recorded visits, and the arena's action lies in
    their argmax set. The mover plays it through selfplay_move (which draws
    the tie-break from the game stream as the arena did, so the streams stay
    aligned for the next searches' symmetry draws) and must choose the same
    action; the other engine applies it."""
    import othello_mcts as om

    net_a, net_b = native_nets
    s = stepped_games

    def single(seed):  # game 0 of this engine gets the key of game g of an engine seeded `seed`
        return om.BatchedMCTS(1, dirichlet_epsilon=0.0,
                              seed=seed ^ R.mix64(g + C_KEY) ^ R.mix64(C_KEY), **KW2)

    ea, eb = single(7), single(8)
    assert ea.engine.game_key(0) == R.game_key(7, g) and eb.engine.game_key(0) == R.game_key(8, g)
    for a in s["openings"][g]:
        ea.apply_action(0, int(a))
        eb.apply_action(0, int(a))
    n = int((s["actions"][:, g] >= 0).sum())
    assert n >= 40
    for ply in range(n):
        player = ea.root_info(0)["player"]
        assert player == eb.root_info(0)["player"] != 0
        a_moves = (player == 1) != bool(s["white"][g])
        mover, net, other = (ea, net_a, eb) if a_moves else (eb, net_b, ea)
        mover.search(net)
        v = mover.root_stats()[0].cpu().numpy()[0]
        rec = s["visits"][ply][0 if a_moves else 1][g]
        np.testing.assert_array_equal(v, rec, err_msg=f"match {g} ply {ply}")
        action = int(s["actions"][ply, g])
        assert v[action] == v.max(), (g, ply)
        mine = int(mover.selfplay_move(temperature_moves=0)["actions"].cpu()[0])
        assert mine == action, (g, ply)
        if ply < n - 1:
            other.apply_action(0, action)
    assert s["status"][g] & 3  # the match ended with that ply


# ------------------------------------------------------------------ mask
def test_idle_engine_and_set_active(native_nets):
    import othello_mcts as om

    net_a, net_b = native_nets
    G = 8
    arena = om.Arena.create(G, seed=3, **KW2)
    arena.reset(openings=np.zeros((G, 0), np.int32), a_is_white=np.zeros(G, bool))
    # black moves first and A is black everywhere: engine B has nothing to search
    assert arena.b.search(net_b, sync=True) == (0, 0)
    assert all(arena.b.root_info(g)["node_count"] == 1 for g in range(G))
    assert arena.a.search(net_a, sync=True)[0] == G * KW2["num_simulations"]
    # a half mask on a plain engine
    m = om.BatchedMCTS(G, dirichlet_epsilon=0.0, seed=5, **KW2)
    mask = np.arange(G) % 2 == 0
    m.set_active(mask)
    sims, evals = m.search(net_a)
    assert sims == int(mask.sum()) * KW2["num_simulations"] and 0 < evals <= sims
    for g in range(G):
        i = m.root_info(g)
        if mask[g]:
            assert i["visit_count"] == KW2["num_simulations"] and i["node_count"] > 1
        else:
            assert (i["visit_count"], i["node_count"], i["num_children"]) == (0, 1, 0)
    # the step-wise path honours the mask too
    sims, _ = m.search(STUB_A)
    assert sims == int(mask.sum()) * KW2["num_simulations"]
    assert all(m.root_info(g)["node_count"] == 1 for g in range(G) if not mask[g])
    m.set_active(None)
    assert m.search(net_a)[0] == G * KW2["num_simulations"]
    with pytest.raises(ValueError):
        m.set_active(np.ones(G + 1, bool))


# ------------------------------------------------------------------ errors
def test_arena_errors_and_unfinished_matches(native_nets):
    import othello_mcts as om
    from othello_mcts.arena import UNFINISHED

    net_a, net_b = native_nets
    with pytest.raises(ValueError):
        om.Arena(om.BatchedMCTS(2, **KW2), om.BatchedMCTS(4, **KW2))
    arena = om.Arena.create(4, seed=1, **KW2)
    with pytest.raises(ValueError):
        arena.reset(openings=[[19, 0, -1, -1]] * 4)  # 0 is not legal after 19
    with pytest.raises(RuntimeError):
        arena.move()  # no match begun
    arena.reset()
    res = arena.play(net_a, net_b, max_plies=10)
    assert res.plies == 10 and res.actions.shape == (10, 4) and (res.actions >= 0).all()
    assert (res.result == UNFINISHED).all() and res.wdl() == (0, 0, 0) and res.records("a", "b") == []
    # the step-wise loop stops at max_plies as well
    arena.reset()
    res2 = arena.play(STUB_A, STUB_B, max_plies=3)
    assert res2.plies == 3 and (res2.result == UNFINISHED).all()
    # the engines must share the stream, the nets must fit their engines
    from othello_mcts.synthetic import alphazero_state_dict

    other = om.NativeNet(alphazero_state_dict(1, 5, 128, 1, 32), device=0)  # history 2, the engines' is 3
    arena.reset()
    with pytest.raises(ValueError):
        arena.a.engine.arena_play(other.handle, arena.b.engine, net_b.handle, 0, 1.0, 4, 0, 0, 0)
