"""Adjudication by the exact solver on the GPU (csrc/tree_game.h
selfplay_move_game, csrc/arena.hip k_arena_move, csrc/adjudicate.hip): every stream is
replayed on the host with Position and othello_mcts.adjudicate, the three
schedules of selfplay_steps against the move-by-move loop, the split solver
against the plain one, the consumers, the arena, and the rows of inactive
games."""

import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
H = 2
KW = dict(history_size=H, num_threads=2, batch_size=8, node_capacity=1 << 15)
ADJ, FLAG, NONE = 32, 64, -(1 << 31)


def empties(p):
    return 64 - bin(p.player1_discs() | p.player2_discs()).count("1")


def discs(p):
    return bin(p.player1_discs()).count("1"), bin(p.player2_discs()).count("1")


def board_code(p):
    b, w = discs(p)
    return 2 if b > w else (3 if b < w else 1)


@pytest.fixture(scope="module")
def net():
    import othello_mcts as om
    from othello_mcts.synthetic import alphazero_state_dict

    return om.NativeNet(alphazero_state_dict(4, 1 + 2 * H, 128, 1, 32), device=0)


def replay_stream(actions, finished, margin, K, split=False):
    """Walk every game of a stream that began at the initial position and
    restarts there (opening_moves = 0) and check each word against the rule.
    Returns the finished games in stream order: (move index, game, margin,
    [black to move? for each of its searched moves], adjudicated?)."""
    import othello_mcts as om

    n, G = actions.shape
    games = []
    for g in range(G):
        p = om.Position.initial_position()
        movers = []
        for i in range(n):
            a, f, m = int(actions[i, g]), int(finished[i, g]), int(margin[i, g])
            assert a >= 0 and not p.is_terminal(), (i, g)
            # no searched move from a root an earlier searched move left at or below K empties
            assert empties(p) > K, (i, g, empties(p))
            assert f & ~(3 | ADJ) == 0, (i, g, f)
            movers.append(p.player() == 1)
            p = p.apply_action(a)
            if f & ADJ:
                assert not p.is_terminal() and empties(p) <= K, (i, g)
                assert om.adjudicate(p, K, split=split) == (f & 3, m), (i, g, f, m)
            elif f & 3:
                assert p.is_terminal(), (i, g)
                assert f & 3 == board_code(p) and m == discs(p)[0] - discs(p)[1], (i, g, f, m)
            else:
                assert not p.is_terminal() and empties(p) > K and m == NONE, (i, g, f, m)
            if f & 3:
                games.append((i, g, m, movers, bool(f & ADJ)))
                p = om.Position.initial_position()
                movers = []
    return sorted(games, key=lambda t: t[:2])


@pytest.fixture(scope="module")
def stream(net):
    """64 moves of 8 games from the initial position at K = 8 (shared, read only)."""
    import othello_mcts as om

    b = om.BatchedMCTS(8, num_simulations=16, seed=21, **KW)
    out = b.selfplay_steps(net, 64, temperature_moves=12, opening_moves=0, emit_targets=True, adjudicate_empties=8)
    torch.cuda.synchronize()
    assert b.engine.status() == (0, 0)
    assert set(out) == {"actions", "finished", "features", "policy", "margin"}
    return out


def test_stream_replays_on_the_host(stream):
    a, f, m = (stream[k].cpu().numpy() for k in ("actions", "finished", "margin"))
    games = replay_stream(a, f, m, 8)
    # from the initial position a game needs at most 60 plies to reach 8
    # empties: within 64 moves every game was adjudicated or ended on the board
    assert len(games) >= 8 and {g for _, g, _, _, _ in games} == set(range(8))
    assert sum(adj for *_, adj in games) >= 8 and int(((f & ADJ) != 0).sum()) == sum(adj for *_, adj in games)


@pytest.fixture(scope="module")
def deep_net():
    """Six blocks: with 64 games the ResNet launches outlast the host's
    enqueue, so the last moves of a multi-move call are still queued when the
    call returns, and a resolve step that did not wait for them would show."""
    import othello_mcts as om
    from othello_mcts.synthetic import alphazero_state_dict

    return om.NativeNet(alphazero_state_dict(4, 1 + 2 * H, 128, 6, 32), device=0)


def late_engine(free=True, pipeline=0, games=16, sims=32):
    import othello_mcts as om

    # trees are kept across a game's moves: the deeper searches of the schedule tests need the room
    b = om.BatchedMCTS(games, num_simulations=sims, seed=5, **{**KW, "node_capacity": 1 << 15 if sims <= 32 else 1 << 18})
    b.random_openings(52, seed=9)  # late openings: games reach 8 empties and restart inside the moves
    b.engine.set_free_running(free)
    if pipeline:
        b.engine.set_pipeline(pipeline)
    return b


PATH_MOVES = 9


@pytest.fixture(scope="module")
def loop_reference(deep_net):
    """9 x (search + selfplay_move(K = 8)) of 64 games from late openings."""
    b = late_engine(games=64, sims=256)
    outs = []
    for _ in range(PATH_MOVES):
        b.search(deep_net, sync=False)
        o = b.selfplay_move(temperature_moves=12, opening_moves=4, emit_targets=True, adjudicate_empties=8)
        outs.append({k: v.clone() for k, v in o.items()})
    torch.cuda.synchronize()
    assert b.engine.status() == (0, 0)
    ref = {k: torch.stack([o[k] for o in outs]) for k in outs[0]}
    fin = ref["finished"].cpu().numpy()
    # adjudications in the first moves (moves after their restarts follow) and in the last two
    per_move = ((fin & ADJ) != 0).sum(axis=1)
    assert per_move[:6].sum() >= 3 and per_move[-2:].sum() >= 1, per_move
    assert (fin[(fin & ADJ) != 0] & 3 != 0).all() and (fin & FLAG == 0).all()
    return ref, b.root_stats()


@pytest.mark.parametrize("path", ["free", "grouped", "single"])
def test_free_running_equals_move_by_move(deep_net, loop_reference, path):
    """selfplay_steps(n, K) on each of its schedules against n x (search +
    selfplay_move(K)): bit for bit, margins and the trees left behind included.
    Two pipeline groups on streams of their own in the first two."""
    ref, (rv, rq) = loop_reference
    b = late_engine(free=path == "free", pipeline=1 if path == "single" else 2, games=64, sims=256)
    out = b.selfplay_steps(deep_net, PATH_MOVES, temperature_moves=12, opening_moves=4, emit_targets=True,
                           adjudicate_empties=8)
    torch.cuda.synchronize()
    assert b.engine.status() == (0, 0)
    for k in ("actions", "finished", "margin", "features", "policy"):
        assert torch.equal(out[k], ref[k]), (path, k)
    v, q = b.root_stats()
    assert torch.equal(v, rv) and torch.equal(q, rq)


def test_openings_at_or_below_k_are_searched_once(net):
    """A root that no searched move produced is searched whatever its empties;
    the move that follows is adjudicated (here every non-terminal result is at
    or below K). Must-pass roots among 64 late openings included."""
    import othello_mcts as om

    G, K = 64, 8
    b = om.BatchedMCTS(G, num_simulations=16, seed=3, **KW)
    b.random_openings(60, seed=4)
    before = [b.root_info(g) for g in range(G)]
    b.search(net, sync=False)
    out = b.selfplay_move(temperature_moves=0, opening_moves=0, adjudicate_empties=K)
    a, f, m = (out[k].cpu().numpy() for k in ("actions", "finished", "margin"))
    seen = {"adjudicated": 0, "board": 0, "on": 0}
    for g, i in enumerate(before):
        p = (i["player"], i["player1_discs"], i["player2_discs"])
        if i["player"] == 0:
            continue
        q = _apply(p, int(a[g]))
        e = 64 - bin(q[1] | q[2]).count("1")
        b1, w1 = bin(q[1]).count("1"), bin(q[2]).count("1")
        if om.get_legal_moves(q[1], q[2]) == 0 and om.get_legal_moves(q[2], q[1]) == 0:  # over on the board
            assert int(f[g]) & (3 | ADJ) == (2 if b1 > w1 else (3 if b1 < w1 else 1)) and int(m[g]) == b1 - w1, g
            seen["board"] += 1
        elif e <= K:
            code, margin = om.adjudicate(q, K)
            assert (int(f[g]) & (3 | ADJ), int(m[g])) == (code | ADJ, margin), g
            seen["adjudicated"] += 1
        else:
            assert int(f[g]) & (3 | ADJ) == 0 and int(m[g]) == NONE, g
            seen["on"] += 1
    assert seen["adjudicated"] >= 4 and seen["on"] >= 4, seen


def _apply(triple, action):
    """(player, p1, p2) after `action` (64 = pass), by the package's bitboards."""
    import othello_mcts as om

    player, p1, p2 = triple
    me, opp = (p1, p2) if player == 1 else (p2, p1)
    if action != 64:
        mv = 1 << (63 - action)
        fl = om.get_flips(mv, me, opp)
        assert fl != 0
        me, opp = me | mv | fl, opp & ~fl
    p1, p2 = (me, opp) if player == 1 else (opp, me)
    return 3 - player, p1, p2


def test_split_equals_plain(net):
    """K = 10: the split solver's words are the plain solver's."""
    outs = []
    for split in (False, True):
        b = late_engine()
        o = b.selfplay_steps(net, 12, temperature_moves=12, opening_moves=4, adjudicate_empties=10, split=split)
        torch.cuda.synchronize()
        outs.append(o)
    for k in ("actions", "finished", "margin"):
        assert torch.equal(outs[0][k], outs[1][k]), k
    f = outs[0]["finished"].cpu().numpy()
    assert int(((f & ADJ) != 0).sum()) >= 3 and (f[(f & ADJ) != 0] & 3 != 0).all()


def forced_line_into_a_pass(K, seed=1):
    """Seeded random playouts until a position P with one legal move a (no
    pass) whose successor Q is not terminal, has at most K empties and a mover
    that must pass. Returns (plies from the initial position to P, a, Q)."""
    import othello_mcts as om

    rng = random.Random(seed)
    for _ in range(20000):
        p, line = om.Position.initial_position(), []
        while not p.is_terminal():
            acts = p.legal_actions()
            a = acts[rng.randrange(len(acts))]
            q = p.apply_action(a)
            if len(acts) == 1 and a != 64 and not q.is_terminal() and q.legal_actions() == [64] and empties(q) <= K:
                return line, a, q
            line.append(a)
            p = q
    raise AssertionError("no forced line into a pass found")


def test_pass_at_the_adjudicated_root(net):
    """The searched (forced) move leaves a root whose mover must pass: it
    counts, and the result is the solver's for the position with the passer
    to move."""
    import othello_mcts as om

    K, G = 8, 8
    line, a, q = forced_line_into_a_pass(K)
    b = om.BatchedMCTS(G, num_simulations=16, seed=8, **KW)
    for ply in line:
        b.apply_actions(torch.full((G,), ply, dtype=torch.int32))
    b.search(net, sync=False)
    out = b.selfplay_move(temperature_moves=0, adjudicate_empties=K)
    code, margin = om.adjudicate(q, K)
    assert out["actions"].tolist() == [a] * G
    assert out["finished"].tolist() == [ADJ | code] * G and out["margin"].tolist() == [margin] * G
    # the games restarted at the initial position
    assert all(b.root_info(g)["player1_discs"] | b.root_info(g)["player2_discs"] ==
               om.Position.initial_position().player1_discs() | om.Position.initial_position().player2_discs()
               for g in range(G))


def test_off_is_the_old_call(net):
    """K = 0 through the new entry points: the old calls' outputs, margin untouched and absent."""
    import othello_mcts as om

    def engine():
        b = om.BatchedMCTS(16, num_simulations=32, seed=5, **KW)
        b.random_openings(58, seed=9)  # roots at and below 8 empties that stay searched
        return b

    old, new = engine(), engine()
    C = 1 + 2 * H
    for _ in range(3):
        old.search(net, sync=False)
        new.search(net, sync=False)
        o = old.selfplay_move(temperature_moves=12, opening_moves=4, emit_targets=True)
        assert "margin" not in o
        acts = torch.empty(16, dtype=torch.int32, device=DEV)
        fin = torch.empty_like(acts)
        margin = torch.full_like(acts, 777)
        feat = torch.empty((16, 8, C, 8, 8), dtype=torch.float32, device=DEV)
        pol = torch.empty((16, 8, 65), dtype=torch.float32, device=DEV)
        new._stream()
        new.engine.selfplay_move_adjudicated(12, 1.0, 4, True, acts.data_ptr(), fin.data_ptr(), feat.data_ptr(),
                                             pol.data_ptr(), 0, False, margin.data_ptr())
        assert torch.equal(acts, o["actions"]) and torch.equal(fin, o["finished"])
        assert torch.equal(feat, o["features"]) and torch.equal(pol, o["policy"])
        assert (margin == 777).all() and (fin & (ADJ | FLAG) == 0).all()
    o = old.selfplay_steps(net, 6, temperature_moves=12, opening_moves=4)
    assert set(o) == {"actions", "finished"}
    acts = torch.empty((6, 16), dtype=torch.int32, device=DEV)
    fin = torch.empty_like(acts)
    margin = torch.full_like(acts, 777)
    new._stream()
    new.engine.selfplay_steps_adjudicated(net.handle, 6, 12, 1.0, 4, False, True, acts.data_ptr(), fin.data_ptr(), 0,
                                          0, 0, False, margin.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(acts, o["actions"]) and torch.equal(fin, o["finished"]) and (margin == 777).all()
    assert int(((fin & 3) != 0).sum()) >= 1 and (fin & (ADJ | FLAG) == 0).all()
    assert new.selfplay_steps(net, 1, adjudicate_empties=0).keys() == {"actions", "finished"}


def test_consumers(stream):
    """The adjudicated move is the move that ended the game: ReplayBuffer and
    SelfPlayCollector store one record per searched move of a finished game,
    valued with the exact sign seen from that record's mover."""
    import othello_mcts as om
    from othello_mcts.selfplay import SelfPlayCollector

    a, f, m = (stream[k].cpu().numpy() for k in ("actions", "finished", "margin"))
    games = replay_stream(a, f, m, 8)
    want_value, want_white = [], []
    for _, _, margin, movers, _ in games:
        s = float(np.sign(margin))
        want_value += [s if black else -s for black in movers]
        want_white += [0 if black else 1 for black in movers]
    assert any(adj for *_, adj in games) and len(want_value) > 8 * 40

    buf = om.ReplayBuffer(8, H, capacity=1024, max_moves=64, device=DEV)
    buf.add({k: stream[k] for k in ("actions", "finished", "features", "policy")})
    buf.check()
    assert buf.games_completed == len(games) and buf.size == len(want_value)
    assert buf.value[:buf.size].tolist() == want_value
    assert buf.player[:buf.size].tolist() == want_white
    # what is still staged belongs to the games running when the stream stopped
    last = {g: i for i, g, *_ in games}
    assert buf.moves.tolist() == [63 - last[g] for g in range(8)]

    col = SelfPlayCollector(8)
    values = []
    for i in range(a.shape[0]):
        got = col.add({k: v[i] for k, v in stream.items()})
        values += [float(v) for v in got["values"]]
    assert col.games_completed == len(games)
    assert values == [v for v in want_value for _ in range(8)]
    assert [col.pending_moves(g) for g in range(8)] == [63 - last[g] for g in range(8)]


def test_sentinel_rows(net):
    """Inactive games: action -1, finished 0, margin INT32_MIN, in the single
    move and in every slice of the multi-move call; the others play what they
    play without the mask."""
    mask = torch.tensor([g % 3 != 1 for g in range(16)])
    full = late_engine()
    part = late_engine()
    part.set_active(mask)
    of = full.selfplay_steps(net, 12, temperature_moves=12, opening_moves=4, adjudicate_empties=8)
    op = part.selfplay_steps(net, 12, temperature_moves=12, opening_moves=4, adjudicate_empties=8)
    torch.cuda.synchronize()
    on = mask.to(DEV)
    for k in ("actions", "finished", "margin"):
        assert torch.equal(of[k][:, on], op[k][:, on]), k
    assert (op["actions"][:, ~on] == -1).all() and (op["finished"][:, ~on] == 0).all()
    assert (op["margin"][:, ~on] == NONE).all()
    assert int(((op["finished"] & ADJ) != 0).sum()) >= 2
    part.search(net, sync=False)
    o = part.selfplay_move(temperature_moves=12, opening_moves=4, adjudicate_empties=8)
    assert (o["actions"][~on] == -1).all() and (o["finished"][~on] == 0).all() and (o["margin"][~on] == NONE).all()
    assert (o["actions"][on] >= 0).all()


# ------------------------------------------------------------------ arena
AKW = dict(history_size=H, num_simulations=16, num_threads=2, batch_size=8, node_capacity=1 << 15)


@pytest.fixture(scope="module")
def nets(net):
    import othello_mcts as om
    from othello_mcts.synthetic import alphazero_state_dict

    return net, om.NativeNet(alphazero_state_dict(6, 1 + 2 * H, 128, 1, 32), device=0)


def replay_matches(openings, res, K):
    """Every match on the host: where it ended and how. Returns per match
    'adjudicated' or 'board'."""
    import othello_mcts as om

    kinds = []
    acts = res.actions.numpy()
    for g in range(acts.shape[1]):
        p = om.Position.initial_position()
        for a in openings[g]:
            if a >= 0:
                p = p.apply_action(int(a))
        n = int((acts[:, g] >= 0).sum())
        assert (acts[:n, g] >= 0).all() and (acts[n:, g] == -1).all(), g  # -1 once the match is over
        for a in acts[:n, g]:
            assert not p.is_terminal() and (K == 0 or empties(p) > K), g
            p = p.apply_action(int(a))
        assert res.discs[g].tolist() == list(discs(p)), g
        if bool(res.adjudicated[g]):
            assert not p.is_terminal() and empties(p) <= K, g
            code, margin = om.adjudicate(p, K)
            assert (int(res.result[g]) + 1, int(res.margin[g])) == (code, margin), g
            kinds.append("adjudicated")
        else:
            assert p.is_terminal(), g
            assert int(res.result[g]) + 1 == board_code(p) and int(res.margin[g]) == discs(p)[0] - discs(p)[1], g
            kinds.append("board")
    return kinds


@pytest.fixture(scope="module")
def arena_k8(nets):
    import othello_mcts as om

    arena = om.Arena.create(16, seed=7, **AKW)
    ops = om.paired_openings(16, 4, seed=7)
    arena.reset(openings=ops)
    res = arena.play(nets[0], nets[1], adjudicate_empties=8)
    return ops, res


def test_arena_replays_on_the_host(arena_k8):
    ops, res = arena_k8
    kinds = replay_matches(ops, res, 8)
    assert kinds.count("adjudicated") >= 8  # a match can end on the board above 8 empties, few do


def test_arena_fused_equals_loop(nets, arena_k8):
    """arena_play against the search / move loop, with the count of running
    matches followed ply by ply: an adjudicated match leaves it once."""
    import othello_mcts as om

    ops, res = arena_k8
    G = 16
    arena = om.Arena.create(G, seed=7, **AKW)
    arena.reset(openings=ops)
    remaining = torch.full((1,), G, dtype=torch.int32, device=DEV)
    rows = []
    for ply in range(res.plies + 2):
        arena.search(nets[0], nets[1], sync=False)
        arena._streams()
        arena.a.engine.arena_move_adjudicated(arena.b.engine, 0, 1.0, arena._actions.data_ptr(),
                                              arena._status.data_ptr(), arena._discs.data_ptr(),
                                              remaining.data_ptr(), 8, False, arena._margin.data_ptr())
        rows.append(arena._actions.cpu().clone())
        running = int(((arena._status.cpu() & 3) == 0).sum())
        assert int(remaining.item()) == running, ply
    acts = torch.stack(rows)
    assert torch.equal(acts[:res.plies], res.actions) and (acts[res.plies:] == -1).all()
    status = arena._status.cpu()
    assert int(remaining.item()) == 0 and (status & 3 != 0).all()
    assert torch.equal(((status & 3) - 1).to(torch.int64), res.result)
    assert torch.equal((status & ADJ) != 0, res.adjudicated)
    assert torch.equal(arena._discs.cpu().to(torch.int64), res.discs)
    assert torch.equal(arena._margin.cpu().to(torch.int64), res.margin)
    # the split solver reports the same matches
    arena.reset(openings=ops)
    res2 = arena.play(nets[0], nets[1], adjudicate_empties=8, split=True)
    for k in ("actions", "result", "discs", "margin", "adjudicated"):
        assert torch.equal(getattr(res2, k), getattr(res, k)), k


def test_arena_result_on_a_mix(nets):
    """K = 1: matches that end on the board (a full board, or nobody can move
    with empties left) beside adjudicated ones; the result object agrees with
    the host replay, and with the feature off the same openings end on the board."""
    import othello_mcts as om

    G = 32
    arena = om.Arena.create(G, seed=11, **AKW)
    ops = om.paired_openings(G, 6, seed=11)
    arena.reset(openings=ops)
    res = arena.play(nets[0], nets[1], adjudicate_empties=1)
    kinds = replay_matches(ops, res, 1)
    assert "adjudicated" in kinds and "board" in kinds, kinds
    assert res.adjudicated.tolist() == [k == "adjudicated" for k in kinds]
    ma = res.margin_a()
    assert res.wdl() == (int((ma > 0).sum()), int((ma == 0).sum()), int((ma < 0).sum()))
    recs = res.records("a", "b")
    assert len(recs) == G and [r["result"] for r in recs] == res.result.tolist()
    assert all((r["player1"] == "b") == bool(w) for r, w in zip(recs, res.a_is_white.tolist()))
    # off: the same openings play to the end on the board
    arena.reset(openings=ops)
    off = arena.play(nets[0], nets[1])
    assert not off.adjudicated.any() and replay_matches(ops, off, 0) == ["board"] * G
    assert torch.equal(off.margin, off.discs[:, 0] - off.discs[:, 1])


def test_arena_off_is_the_old_call(nets):
    """max_empties = 0 through the arena's new entry points: the old bindings'
    outputs ply by ply and for the fused call, the margin buffer untouched."""
    import othello_mcts as om

    G = 16
    ops = om.paired_openings(G, 4, seed=3)

    def arena():
        x = om.Arena.create(G, seed=3, **AKW)
        x.reset(openings=ops)
        return x

    old, new = arena(), arena()
    margin = torch.full((G,), 777, dtype=torch.int32, device=DEV)
    for _ in range(70):
        old.search(nets[0], nets[1], sync=False)
        new.search(nets[0], nets[1], sync=False)
        o = old.move()
        new._streams()
        new.a.engine.arena_move_adjudicated(new.b.engine, 0, 1.0, new._actions.data_ptr(), new._status.data_ptr(),
                                            new._discs.data_ptr(), 0, 0, False, margin.data_ptr())
        assert torch.equal(new._actions, o["actions"]) and torch.equal(new._status, o["finished"])
        assert torch.equal(new._discs, o["discs"])
        if bool((o["finished"] & 3 != 0).all()):
            break
    status = old._status.cpu()
    assert (status & 3 != 0).all() and (status & (ADJ | FLAG) == 0).all() and (margin == 777).all()
    # the fused call
    old.reset(openings=ops)
    res = old.play(nets[0], nets[1])
    new.reset(openings=ops)
    new._streams()
    acts = torch.empty((128, G), dtype=torch.int32, device=DEV)
    plies = new.a.engine.arena_play_adjudicated(nets[0].handle, new.b.engine, nets[1].handle, 0, 1.0, 128,
                                                acts.data_ptr(), new._status.data_ptr(), new._discs.data_ptr(), 0,
                                                False, margin.data_ptr())
    assert plies >= res.plies and torch.equal(acts[:res.plies].cpu(), res.actions) and (acts[res.plies:plies] == -1).all()
    assert torch.equal(((new._status.cpu() & 3) - 1).to(torch.int64), res.result)
    assert torch.equal(new._discs.cpu().to(torch.int64), res.discs) and (margin == 777).all()
    assert not res.adjudicated.any()


def test_replay_refuses_a_word_the_solver_flagged(stream):
    """finished bit 6 (an adjudicated game without an outcome): the buffer sets
    its sticky flag, drops that game's staged moves, and check() raises."""
    import othello_mcts as om

    f = stream["finished"].clone()
    i, g = (int(x) for x in ((f & ADJ) != 0).nonzero()[0])
    f[i, g] = ADJ | FLAG
    buf = om.ReplayBuffer(8, H, capacity=1024, max_moves=64, device=DEV)
    buf.add({"actions": stream["actions"][:i + 1], "finished": f[:i + 1], "features": stream["features"][:i + 1],
             "policy": stream["policy"][:i + 1]})
    assert int(buf.moves[g]) == 0
    others = int(((f[:i + 1] & 3) != 0).sum())
    assert buf.games_completed == others
    with pytest.raises(RuntimeError, match="exact solver flagged"):
        buf.check()
    with pytest.raises(RuntimeError, match="exact solver flagged"):
        from othello_mcts.selfplay import SelfPlayCollector

        SelfPlayCollector(8).add({k: (f if k == "finished" else v)[i] for k, v in stream.items()})
