"""The two C=128 throughput geometries of the fused ResNet (csrc/resnet.hip):
k_resnet_w8 (8 waves of 32 channels x 128 positions, LDS weight ring) and
k_resnet_w4 (4 waves of 32 channels x 256 positions, weights queued in
registers), chosen by the process-wide switch
othello_mcts.native.set_c128_four_wave. Same K order, same tile -> position
map, same accumulator start: every output must agree bit for bit between the
two and with the one-board small-batch geometry, the exact probe nets of
tests/exact_nets.py must come out exact under either, and a search that feeds
the kernel through the packed evaluation list must not change."""

import numpy as np
import pytest
import torch

import exact_nets as E

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = ("bf16", "fp16")
SWITCH = (True, False)  # 4-wave, 8-wave


@pytest.fixture(scope="module")
def om():
    import othello_mcts

    return othello_mcts


@pytest.fixture()
def four_wave(om):
    """Sets the switch for a test and restores the build's default after it."""
    from othello_mcts import native

    default = native.c128_four_wave()
    yield native.set_c128_four_wave
    native.set_c128_four_wave(default)


def test_switch_round_trip(om, four_wave):
    from othello_mcts import native

    for v in SWITCH:
        four_wave(v)
        assert native.c128_four_wave() is v
    assert four_wave(True) is False  # returns the previous setting


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R", [1, 2], ids=["128x2b", "128x3b"])
def test_geometries_are_bit_identical(om, four_wave, dtype, R):
    """128x2b: the first conv and one block (the weight queue crosses two layer
    boundaries); 128x3b adds the block -> block boundary. 1024 rows: the
    dispatch threshold; 1027: the last workgroup holds 3 boards and 1 past the
    end. The first 100 rows and the ragged tail, evaluated alone (one board
    per workgroup), give the same bits."""
    from othello_mcts.synthetic import alphazero_state_dict

    net = om.NativeNet(alphazero_state_dict(11, 17, 128, R, 64), device=0, dtype=dtype)
    gen = torch.Generator().manual_seed(128 + R)
    x = (torch.rand((1027, 17, 8, 8), generator=gen) < 0.3).float().to(DEV)
    head = net(x[:100].contiguous())
    tail = net(x[1024:].contiguous())
    for rows in (1024, 1027):
        xs = x[:rows].contiguous()
        out = {}
        for v in SWITCH:
            four_wave(v)
            out[v] = net(xs)
        torch.cuda.synchronize()
        for k in ("policy", "value"):
            assert torch.equal(out[True][k], out[False][k]), (rows, k)
            assert torch.equal(out[True][k][:100], head[k]), (rows, k)
        if rows == 1027:
            for k in ("policy", "value"):
                assert torch.equal(out[True][k][1024:], tail[k]), k


EXACT_CASES = [a for a, _ in E.ROUTING + E.INTEGER if a[1] == 128]


@pytest.mark.parametrize("args", EXACT_CASES, ids=[E.case_id(a) for a in EXACT_CASES])
def test_exact_nets_under_either_geometry(om, four_wave, args):
    """The routing nets (four phases: every conv2 output channel carries a
    non-zero weight) and the integer net at 1024 rows: one misrouted channel,
    tap, board, row or K-step of any of a wave's 16 tiles fails the case."""
    sd, x, ref = E.case(*args)
    xs = torch.from_numpy(np.array(x[:1024])).to(DEV)
    for dtype in DTYPES:
        net = om.NativeNet(sd, device=0, dtype=dtype)
        for v in SWITCH:
            four_wave(v)
            out = net(xs)
            torch.cuda.synchronize()
            E.compare(out["policy"].cpu().numpy(), out["value"].cpu().numpy(), ref.rows(1024),
                      f"{E.case_id(args)} {dtype} four_wave={v}")


def test_search_through_the_evaluation_list(om, four_wave):
    """32 games x (2 threads x 16 leaves) = 1024 list entries per launch, 64
    simulations per search, 24 moves of self-play from late openings (games
    reach their last squares, so some leaves are terminal and the list is not
    full): every search's visits, Q and work counts and every move are the
    same under both geometries, and the guard words behind the engine's
    policy / value buffers stay untouched."""
    from othello_mcts.synthetic import alphazero_state_dict

    net = om.NativeNet(alphazero_state_dict(43, 9, 128, 1, 32), device=0)
    b = om.BatchedMCTS(32, history_size=4, num_simulations=64, num_threads=2, batch_size=16,
                       dirichlet_epsilon=0.25, seed=8, node_capacity=1 << 16)
    assert b.rows_per_step == 1024
    moves = 24  # openings of 0-58 plies: many games reach their last squares within these moves
    got = {}
    for v in SWITCH:
        four_wave(v)
        b.reset(-1, 8)
        b.random_openings(58, seed=9)
        got[v] = []
        for _ in range(moves):
            work = b.search(net)
            visits, q = b.root_stats()
            o = b.selfplay_move(temperature_moves=12, opening_moves=58)
            got[v].append((tuple(work), visits, q, o["actions"].clone(), o["finished"].clone()))
        assert b.engine.eval_guards_intact(), v
    sims = sum(w[0] for w, *_ in got[True])
    evals = sum(w[1] for w, *_ in got[True])
    assert 0 < evals < sims  # some leaves were terminal: the lists had gaps
    for mv, (x, y) in enumerate(zip(got[True], got[False])):
        assert x[0] == y[0], mv
        assert all(torch.equal(s, t) for s, t in zip(x[1:], y[1:])), mv
        assert int(x[1].sum()) > 0, mv
