"""ReplayBuffer (csrc/replay.hip) on the GPU: against SampleBuffer on real
self-play, against the numpy restatement (tests/replay_ref.py, pinned to
SampleBuffer by tests/test_cpu_replay.py) on synthetic shapes, its sticky
errors, train_epoch_replay against train_epoch, and persistence."""

import functools

import numpy as np
import pytest
import torch

import replay_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
G_PLAY, H_PLAY = 16, 2


def to_dev(out):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in out.items()}


def bits(t):
    return t.contiguous().view(torch.int32)


def sample_buffer_rows(sb):
    """SampleBuffer's live rows, oldest first (a full ring is in physical order
    with the oldest row at ``_head``)."""
    n = sb.size
    rows = [sb.features[:n], sb.policies[:n], sb.values[:n]]
    if n == sb.capacity:
        rows = [torch.roll(r, -sb._head, 0) for r in rows]
    return rows


def assert_same_as_sample_buffer(rb, sb):
    size = rb.size
    assert 8 * size == sb.size and rb.games_completed == sb.games_completed
    assert (8 * rb.head) % sb.capacity == sb._head
    f, p, v = rb.gather(torch.arange(8 * size))
    bf, bp, bv = sample_buffer_rows(sb)
    # features and policy bit for bit; values by ==, so a draw's -0.0 counts as 0.0
    assert torch.equal(bits(f), bits(bf))
    assert torch.equal(bits(p), bits(bp))
    assert torch.equal(v, bv)
    rb.check()


def engine_and_net():
    import othello_mcts as om
    from othello_mcts.synthetic import alphazero_state_dict

    net = om.NativeNet(alphazero_state_dict(4, 5, 128, 1, 32), device=0)
    b = om.BatchedMCTS(G_PLAY, history_size=H_PLAY, num_simulations=16, num_threads=1, batch_size=8, seed=3,
                       node_capacity=1 << 14)
    return b, net


@functools.lru_cache(maxsize=None)
def played(P):
    """Real self-play until 3 G games have completed, every move fed to a
    SampleBuffer of 8 P samples and a ReplayBuffer of P positions, compared
    every 8 moves and at the end. Returns the two buffers, which the tests
    that share them only read."""
    import othello_mcts as om

    b, net = engine_and_net()
    sb = om.SampleBuffer(G_PLAY, 1 + 2 * H_PLAY, capacity=8 * P, device=DEV)
    rb = om.ReplayBuffer(G_PLAY, H_PLAY, P, device=DEV)
    moves = 0
    while sb.games_completed < 3 * G_PLAY:
        b.search(net)
        out = b.selfplay_move(emit_targets=True)
        sb.add(out)
        assert rb.add(out) is None  # enqueued only
        moves += 1
        if moves % 8 == 0:
            assert_same_as_sample_buffer(rb, sb)
    assert_same_as_sample_buffer(rb, sb)
    return rb, sb


def test_real_self_play_unwrapped_equals_sample_buffer():
    rb, sb = played(4096)
    assert rb.size < 4096 and rb.head == rb.size and rb.games_completed >= 3 * G_PLAY


def test_real_self_play_wrapped_equals_sample_buffer():
    rb, sb = played(256)
    assert rb.size == 256 and rb.games_completed >= 3 * G_PLAY


def test_real_self_play_stacked_add_equals_sample_buffer():
    """selfplay_steps(keep_all=True): one stacked add per call against the
    SampleBuffer fed slice by slice."""
    import othello_mcts as om

    P, n = 256, 16
    b, net = engine_and_net()
    sb = om.SampleBuffer(G_PLAY, 1 + 2 * H_PLAY, capacity=8 * P, device=DEV)
    rb = om.ReplayBuffer(G_PLAY, H_PLAY, P, device=DEV)
    while sb.games_completed < 3 * G_PLAY:
        o = b.selfplay_steps(net, n, emit_targets=True, keep_all=True)
        rb.add(o)
        for i in range(n):
            sb.add({k: v[i] for k, v in o.items()})
        assert_same_as_sample_buffer(rb, sb)
    assert rb.size == P


# ------------------------------------------------------------------ synthetic shapes
SENTINEL = {torch.float32: 12345.5, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int32: 0x5A5A5A5A, torch.uint8: 0xA5}


class Bracketed:
    """A tensor between two sentinel rows; ``inner`` is the part handed out."""

    def __init__(self, shape, dtype):
        raw = torch.int64 if dtype == torch.uint64 else dtype
        self.raw = raw
        self.big = torch.full((shape[0] + 2, *shape[1:]), SENTINEL[raw], dtype=raw, device=DEV)
        self.inner = self.big[1:-1]
        self.inner.zero_()
        if dtype == torch.uint64:
            self.inner = self.inner.view(torch.uint64)

    def intact(self):
        return bool((self.big[0] == SENTINEL[self.raw]).all()) and bool((self.big[-1] == SENTINEL[self.raw]).all())


def bracket_storage(rb):
    guards = {}
    for name in ("boards", "policy", "value", "player", "stage_boards", "stage_policy", "stage_player", "moves",
                 "_pending", "counters"):
        t = getattr(rb, name)
        guards[name] = Bracketed(tuple(t.shape), t.dtype)
        assert guards[name].inner.shape == t.shape and guards[name].inner.dtype == t.dtype
        setattr(rb, name, guards[name].inner)
    return guards


@pytest.mark.parametrize("H", [1, 8, 15])
@pytest.mark.parametrize("G", [1, 3, 70])
def test_synthetic_shapes_equal_reference(G, H):
    import othello_mcts as om

    rng = np.random.default_rng(1000 * G + H)
    cap, max_moves = 8, 6
    moves = R.random_script(rng, G, H, 30, max_len=max_moves)
    ref = R.ReplayRef(G, H, cap, max_moves=max_moves)
    rb = om.ReplayBuffer(G, H, cap, max_moves=max_moves, device=DEV)
    guards = bracket_storage(rb)
    for out in moves[:10]:  # move by move, then the rest as one stacked call
        ref.add(out)
        rb.add(to_dev(out))
    ref.add(R.stack(moves[10:]))
    rb.add(to_dev(R.stack(moves[10:])))
    assert (rb.size, rb.head, rb.games_completed) == (ref.size, ref.head, ref.games_completed)
    assert ref.size == cap and ref.flags == 0
    rb.check()
    # the ring and the staging area themselves
    assert np.array_equal(rb.boards.cpu().numpy(), ref.boards)
    assert np.array_equal(rb.policy.cpu().numpy().view(np.uint32), ref.policy.view(np.uint32))
    assert np.array_equal(rb.value.cpu().numpy(), ref.value)
    assert np.array_equal(rb.player.cpu().numpy(), ref.player)
    assert np.array_equal(rb.moves.cpu().numpy(), ref.moves)
    for g in range(G):
        m = int(ref.moves[g])
        assert np.array_equal(rb.stage_boards[g, :m].cpu().numpy(), ref.stage_boards[g, :m])
        assert np.array_equal(rb.stage_policy[g, :m].cpu().numpy(), ref.stage_policy[g, :m])
        assert np.array_equal(rb.stage_player[g, :m].cpu().numpy(), ref.stage_player[g, :m])
    # gathers: duplicate and unsorted ids, sizes around the 4-samples-per-block grid
    C = 1 + 2 * H
    for n in (1, 63, 65, 1000):
        ids = rng.integers(0, 8 * cap, size=n)
        outs = [Bracketed(s, torch.float32) for s in ((n, C, 8, 8), (n, 65), (n,))]
        f, p, v = rb.gather(torch.from_numpy(ids), out=tuple(o.inner for o in outs))
        rf, rp, rv = ref.gather(ids)
        assert np.array_equal(f.cpu().numpy().view(np.uint32), rf.view(np.uint32))
        assert np.array_equal(p.cpu().numpy().view(np.uint32), rp.view(np.uint32))
        assert np.array_equal(v.cpu().numpy(), rv)
        assert all(o.intact() for o in outs)
    rb.check()
    assert all(g.intact() for g in guards.values()), [k for k, g in guards.items() if not g.intact()]


# ------------------------------------------------------------------ sticky errors
def test_sticky_errors_raise_sample_buffers_messages():
    import othello_mcts as om

    rng = np.random.default_rng(7)

    def fresh(max_moves=4):
        return om.ReplayBuffer(3, 1, 8, max_moves=max_moves, device=DEV)

    rb = fresh()
    rb.add(to_dev(R.synthetic_move(rng, 3, 1, [2, 3, 4], [0, R.FIN_OVERFLOW, 0])))
    assert rb.moves.tolist() == [1, 0, 1]  # the offending row is not staged, the valid ones are
    with pytest.raises(RuntimeError, match="node pool exhausted: the search no longer matches the reference"):
        rb.check()
    with pytest.raises(RuntimeError, match="node pool exhausted"):  # sticky
        rb.check()

    rb = fresh()
    rb.add(to_dev(R.synthetic_move(rng, 3, 1, [2, 3, -1], [R.FIN_NO_TARGETS, 0, R.FIN_NO_TARGETS])))
    assert rb.moves.tolist() == [0, 1, 0]
    with pytest.raises(ValueError, match="The root node has not been expanded yet."):
        rb.check()

    rb = fresh(max_moves=2)
    for _ in range(2):
        rb.add(to_dev(R.synthetic_move(rng, 3, 1, [2, 3, -1], [0, 0, 0])))
    rb.check()
    rb.add(to_dev(R.synthetic_move(rng, 3, 1, [2, -1, 5], [0, 0, 0])))
    assert rb.moves.tolist() == [2, 2, 1]
    with pytest.raises(RuntimeError, match="a game exceeded ReplayBuffer.max_moves"):
        rb.check()

    rb = fresh()
    rb.add(to_dev(R.synthetic_move(rng, 3, 1, [2, 3, 4], [2, 0, 0])))
    assert rb.size == 1
    f, p, v = rb.gather(torch.tensor([7, 8, -1, 0]))
    assert not f[1:3].any() and not p[1:3].any() and not v[1:3].any()
    assert p[0].any() and p[3].any() and float(v[3]) == 1.0 - 2.0 * float(f[3, 0, 0, 0])  # black won
    with pytest.raises(IndexError, match="sample id outside"):
        rb.check()

    with pytest.raises(ValueError, match="emit_targets=True"):
        fresh().add({"actions": torch.zeros(3, dtype=torch.int32, device=DEV),
                     "finished": torch.zeros(3, dtype=torch.int32, device=DEV)})


# ------------------------------------------------------------------ sampling
def test_sample_draws_live_rows_on_the_device():
    import othello_mcts as om

    rb, sb = played(256)  # wrapped: every slot is live
    bf, bp, bv = sample_buffer_rows(sb)

    def key(f, p, v):
        # rows as exact integers: 0/1 planes against integer weights, plus the value and the policy's bits
        w = torch.arange(1, f[0].numel() + 1, dtype=torch.float64, device=DEV) ** 2
        return (f.flatten(1).double() @ w) * 4 + (v.double() + 1) + bits(p).double().sum(1) * 2 ** -40

    live = key(bf, bp, bv)
    gen = torch.Generator(device=DEV).manual_seed(5)
    f, p, v = rb.sample(512, generator=gen)
    assert f.shape == (512, 1 + 2 * H_PLAY, 8, 8) and p.shape == (512, 65) and v.shape == (512,)
    assert bool(torch.isin(key(f, p, v), live).all())
    assert len(torch.unique(key(f, p, v))) > 256  # all 8 transforms of many positions, not one corner of the ring
    again = rb.sample(512, generator=torch.Generator(device=DEV).manual_seed(5))
    assert all(torch.equal(a, b) for a, b in zip((f, p, v), again))
    f2, _, _ = rb.sample(16, generator=torch.Generator().manual_seed(1))  # a host generator works too
    assert f2.shape[0] == 16 and rb.sample(0)[0].shape[0] == 0
    rb.check()
    empty = om.ReplayBuffer(2, 1, 8, device=DEV)
    f, p, v = empty.sample(4)
    assert not f.any() and not p.any() and not v.any()
    with pytest.raises(IndexError, match="sample id outside"):
        empty.check()


# ------------------------------------------------------------------ training
def test_train_epoch_replay_equals_train_epoch():
    from othello_mcts.training import train_epoch, train_epoch_replay

    rb, sb = played(4096)
    C = 1 + 2 * H_PLAY

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear(C * 64, 66)

        def forward(self, x):
            y = self.lin(x.flatten(1))
            return {"policy": torch.softmax(y[:, :65], 1), "value": torch.tanh(y[:, 65])}

    def run(replay):
        torch.manual_seed(0)
        toy = Toy().to(DEV)
        seen = []
        toy.register_forward_pre_hook(lambda mod, args: seen.append(args[0].clone()))
        opt = torch.optim.SGD(toy.parameters(), lr=0.1, momentum=0.9)
        gen = torch.Generator().manual_seed(42)
        if replay:
            means = train_epoch_replay(toy, opt, rb, 256, generator=gen)
        else:
            n = sb.size
            means = train_epoch(toy, opt, sb.features[:n], sb.policies[:n], sb.values[:n], 256, generator=gen)
        return means, seen

    m_old, seen_old = run(False)
    m_new, seen_new = run(True)
    assert len(seen_old) == len(seen_new) == sb.size // 256 and len(seen_old) > 10
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(seen_old, seen_new))
    assert set(m_old) == set(m_new) == {"total_loss", "policy_loss", "value_loss", "l2_loss"}
    for k in m_old:
        assert m_new[k] == pytest.approx(m_old[k], rel=1e-6), k


# ------------------------------------------------------------------ persistence, footprint
def test_state_dict_round_trip_and_footprint():
    import othello_mcts as om

    G, H, cap, max_moves = 5, 3, 16, 6
    rng = np.random.default_rng(21)
    moves = R.random_script(rng, G, H, 20, max_len=max_moves)
    a = om.ReplayBuffer(G, H, cap, max_moves=max_moves, device=DEV)
    for out in moves[:12]:
        a.add(to_dev(out))
    sd = a.state_dict()
    assert all(t.device.type == "cpu" for t in sd.values() if isinstance(t, torch.Tensor))
    assert int(sd["moves"].sum()) > 0  # games in flight travel with the state
    b = om.ReplayBuffer(G, H, cap, max_moves=max_moves, device=DEV)
    b.load_state_dict(sd)
    ids = torch.from_numpy(rng.integers(0, 8 * a.size, size=300))
    assert (a.size, a.head, a.games_completed) == (b.size, b.head, b.games_completed)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a.gather(ids), b.gather(ids)))
    for out in moves[12:]:  # 8 more moves
        a.add(to_dev(out))
        b.add(to_dev(out))
    ids = torch.arange(8 * a.size)
    assert (a.size, a.head, a.games_completed) == (b.size, b.head, b.games_completed)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a.gather(ids), b.gather(ids)))
    for k in ("boards", "stage_boards", "moves", "counters"):
        assert torch.equal(getattr(a, k).cpu().view(torch.uint8), getattr(b, k).cpu().view(torch.uint8))
    with pytest.raises(ValueError, match="capacity"):
        om.ReplayBuffer(G, H, cap + 1, max_moves=max_moves, device=DEV).load_state_dict(sd)

    def nbytes(*names):
        return sum(getattr(a, n).numel() * getattr(a, n).element_size() for n in names)

    staging = nbytes("stage_boards", "stage_policy", "stage_player", "moves", "_pending", "counters")
    assert staging == G * max_moves * (16 * H + 261) + 8 * G + 32
    assert a.nbytes == cap * (16 * H + 265) + staging
    assert nbytes("boards", "policy", "value", "player") == cap * (16 * H + 265)
    # 393 bytes per position at H = 8, 94 times less than SampleBuffer's 8 fp32 samples
    assert 16 * 8 + 265 == 393 and round(8 * (17 * 64 * 4 + 65 * 4 + 4) / 393) == 94
