"""The numpy restatement of the packed replay buffer (tests/replay_ref.py)
against ``SampleBuffer(device="cpu")``: fed the same synthetic self-play
outputs, the reference's rows for all sample ids are the SampleBuffer's rows
after every move. tests/test_gpu_replay.py then holds ``ReplayBuffer``'s
kernels to this reference. No GPU is used here."""

import numpy as np
import pytest
import torch

import replay_ref as R
from othello_mcts.replay import ReplayBuffer
from othello_mcts.training import SampleBuffer, train_epoch_replay  # noqa: F401  (the new name imports)


def as_torch(out):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in out.items()}


def sample_buffer_rows(buf):
    """The SampleBuffer's live rows, oldest first: once the ring is full its
    rows are in physical order and the oldest one sits at ``buf._head``."""
    n = buf.size
    rows = [buf.features[:n], buf.policies[:n], buf.values[:n]]
    if n == buf.capacity:
        rows = [torch.roll(r, -buf._head, 0) for r in rows]
    return rows


def assert_rows_equal(ref, buf):
    assert 8 * ref.size == buf.size and ref.games_completed == buf.games_completed
    f, p, v = ref.gather(np.arange(8 * ref.size))
    bf, bp, bv = sample_buffer_rows(buf)
    # features and policy bit for bit; values by ==, so a draw's -0.0 counts as 0.0
    assert np.array_equal(f.view(np.uint32), bf.numpy().view(np.uint32))
    assert np.array_equal(p.view(np.uint32), bp.numpy().view(np.uint32))
    assert torch.equal(torch.from_numpy(v), bv)
    assert ref.flags == 0


def scripted_moves(rng, H):
    """G = 3, for a ring of 8 positions: an inactive game, a draw with white to
    move that finishes on the game's first staged move, then two games
    finishing on one move whose 8 positions wrap the ring inside game 2."""
    mv = R.synthetic_move
    return [
        mv(rng, 3, H, [5, -1, 7], [0, 0, 0], player=[0, 0, 0]),
        mv(rng, 3, H, [1, -1, 2], [0, 0, 0], player=[1, 1, 1]),
        mv(rng, 3, H, [3, 64, 4], [0, 1, 0], player=[0, 1, 0]),
        mv(rng, 3, H, [6, -1, 8], [2, 0, 3], player=[1, 0, 1]),
        mv(rng, 3, H, [9, 10, -1], [0, 0, 0]),
        mv(rng, 3, H, [11, 12, 13], [3, 2, 0], player=[1, 0, 1]),
    ]


@pytest.mark.parametrize("capacity", [8, 64])
def test_reference_rows_equal_sample_buffer_rows_after_every_move(capacity):
    rng = np.random.default_rng(11)
    G, H = 3, 2
    moves = scripted_moves(rng, H) + R.random_script(rng, G, H, 40, max_len=6)
    ref = R.ReplayRef(G, H, capacity, max_moves=8)
    buf = SampleBuffer(G, 1 + 2 * H, capacity=8 * capacity, max_moves=8, device="cpu")
    sizes = []
    for out in moves:
        ref.add(out)
        buf.add(as_torch(out))
        assert_rows_equal(ref, buf)
        sizes.append(ref.size)
    assert ref.games_completed > 10
    if capacity == 8:
        # the scripted part: 1 position (the draw), then 8 more wrap the ring
        assert sizes[2] == 1 and sizes[3] == 8 and ref.size == 8
    else:
        assert ref.size == 64 and sizes[3] == 9


def test_draw_with_white_to_move_is_minus_zero_in_both():
    rng = np.random.default_rng(5)
    ref = R.ReplayRef(1, 1, 4, max_moves=4)
    buf = SampleBuffer(1, 3, capacity=32, max_moves=4, device="cpu")
    out = R.synthetic_move(rng, 1, 1, [20], [1], player=[1])
    ref.add(out)
    buf.add(as_torch(out))
    assert_rows_equal(ref, buf)
    v = ref.gather(np.arange(8))[2]
    assert np.all(v == 0.0) and np.all(np.signbit(v)) and bool(torch.signbit(buf.values[:8]).all())


@pytest.mark.parametrize("G,H", [(1, 1), (5, 8), (4, 15)])
def test_reference_other_shapes_and_stacked_moves(G, H):
    rng = np.random.default_rng(100 * G + H)
    moves = R.random_script(rng, G, H, 24, max_len=5)
    ref = R.ReplayRef(G, H, 8, max_moves=6)
    stacked = R.ReplayRef(G, H, 8, max_moves=6)
    buf = SampleBuffer(G, 1 + 2 * H, capacity=64, max_moves=6, device="cpu")
    for out in moves:
        ref.add(out)
        buf.add(as_torch(out))
    assert_rows_equal(ref, buf)
    stacked.add(R.stack(moves))
    ids = np.arange(8 * ref.size)
    assert stacked.size == ref.size and stacked.head == ref.head
    assert all(np.array_equal(a, b) for a, b in zip(ref.gather(ids), stacked.gather(ids)))


def test_reference_flags_what_sample_buffer_raises():
    rng = np.random.default_rng(3)
    cases = [
        ([2, 3], [R.FIN_OVERFLOW, 0], R.FLAG_OVERFLOW, RuntimeError, "node pool exhausted"),
        ([2, 3], [0, R.FIN_NO_TARGETS], R.FLAG_NO_TARGETS, ValueError, "has not been expanded"),
    ]
    for actions, finished, flag, exc, msg in cases:
        ref = R.ReplayRef(2, 1, 8, max_moves=2)
        out = R.synthetic_move(rng, 2, 1, actions, finished)
        ref.add(out)
        assert ref.flags == flag and ref.moves.tolist() == [int(not finished[0]), int(not finished[1])]
        with pytest.raises(exc, match=msg):
            SampleBuffer(2, 3, capacity=64, max_moves=2, device="cpu").add(as_torch(out))
    # an unplayed game may carry the no-targets bit (the driver reports it for any unexpanded root)
    ref = R.ReplayRef(2, 1, 8, max_moves=2)
    ref.add(R.synthetic_move(rng, 2, 1, [-1, 3], [R.FIN_NO_TARGETS, 0]))
    assert ref.flags == 0 and ref.moves.tolist() == [0, 1]
    # a third move of a game with max_moves = 2
    ref = R.ReplayRef(2, 1, 8, max_moves=2)
    buf = SampleBuffer(2, 3, capacity=64, max_moves=2, device="cpu")
    for _ in range(2):
        out = R.synthetic_move(rng, 2, 1, [4, 5], [0, 0])
        ref.add(out)
        buf.add(as_torch(out))
    assert ref.flags == 0 and ref.moves.tolist() == [2, 2]
    out = R.synthetic_move(rng, 2, 1, [4, -1], [0, 0])
    ref.add(out)
    assert ref.flags == R.FLAG_TOO_LONG and ref.moves.tolist() == [2, 2]
    with pytest.raises(RuntimeError, match="exceeded SampleBuffer.max_moves"):
        buf.add(as_torch(out))
    # a bad gather id: a zero row and the flag
    ref = R.ReplayRef(1, 1, 8)
    ref.add(R.synthetic_move(rng, 1, 1, [4], [2]))
    f, p, v = ref.gather([0, 8, -1, 7])
    assert ref.flags == R.FLAG_BAD_ID
    assert not f[1].any() and not f[2].any() and not p[1:3].any() and f[0].any() and p[3].any()


def test_transform_tables_follow_the_definition():
    """t = 0 is the identity, t = 1 flips the columns, t = 2 is one clockwise
    rotation ((row, col) -> (col, 7 - row)); INV undoes FWD."""
    assert R.FWD[0].tolist() == list(range(64))
    assert R.FWD[1][0] == 7 and R.FWD[1][8] == 15
    assert R.FWD[2][1] == 15 and R.FWD[2][8] == 6  # (0,1) -> (1,7); (1,0) -> (0,6)
    for t in range(8):
        assert sorted(R.FWD[t].tolist()) == list(range(64))
        assert (R.FWD[t][R.INV[t]] == np.arange(64)).all()


@pytest.mark.parametrize("kwargs,exc", [
    (dict(num_games=0, history_size=2, capacity=8), ValueError),
    (dict(num_games=2, history_size=0, capacity=8), ValueError),
    (dict(num_games=2, history_size=16, capacity=8), ValueError),
    (dict(num_games=2, history_size=2, capacity=0), ValueError),
    (dict(num_games=2, history_size=2, capacity=8, max_moves=0), ValueError),
    (dict(num_games=1 << 20, history_size=2, capacity=8, max_moves=1 << 11), ValueError),
    (dict(num_games=2.0, history_size=2, capacity=8), TypeError),
    (dict(num_games=2, history_size=2, capacity=8, device="cpu"), ValueError),
])
def test_constructor_validation_needs_no_gpu(kwargs, exc):
    with pytest.raises(exc):
        ReplayBuffer(**kwargs)
