"""Timing and round accounting of the three native schedules where
test_gpu_async_search_matches_sync does not pin it: pipeline groups of unequal
size whose rows are sliced into several ResNet launches (oamd_engine_set_nn_batch),
for the lock-step search and the free-running self-play call, and the
single-game thread split. The small synthetic net of that test (C=128,
2 blocks, H=4); the counters are nn_timing / tree_timing / round_counts /
nn_busy of the experimental header."""

import pytest
import torch

pytestmark = pytest.mark.gpu

# 7 games over 3 pipeline groups: 2, 2 and 3 games; T=2 x B=4 rows per game;
# 20 rows per launch: 16, 16 and 24 rows -> 1, 1 and 2 launches per round
G, K, T, B, SIMS, NN_BATCH = 7, 3, 2, 4, 32, 20
STEPS = 4  # 32 simulations / (2 x 4)
LAUNCHES_PER_ROUND = 4
ROWS_PER_ROUND = G * T * B


@pytest.fixture(scope="module")
def om():
    import othello_mcts

    return othello_mcts


@pytest.fixture(scope="module")
def net(om):
    from othello_mcts.synthetic import alphazero_state_dict

    return om.NativeNet(alphazero_state_dict(5, 9, 128, 2, 32), device=0)


def _grouped_engine(om, free):
    b = om.BatchedMCTS(G, history_size=4, num_simulations=SIMS, num_threads=T, batch_size=B, seed=9,
                       node_capacity=1 << 14)
    b.random_openings(6, seed=4)
    b.engine.set_pipeline(K)
    b.engine.set_nn_batch(NN_BATCH)
    b.engine.set_chain_split(1, 3)
    b.engine.set_free_running(free)
    b.engine.enable_timing(1)
    return b


def _counters(b):
    ms, nn_launches, rows = b.engine.nn_timing()
    sel, bk, tree_launches = b.engine.tree_timing()
    searches, rounds, finals = b.engine.round_counts()
    busy, busy_launches = b.engine.nn_busy()
    return dict(ms=ms, nn_launches=nn_launches, rows=rows, sel=sel, bk=bk, tree_launches=tree_launches,
                searches=searches, rounds=rounds, finals=finals, busy=busy, busy_launches=busy_launches)


def test_lock_step_unequal_groups_sliced_launches(om, net):
    b = _grouped_engine(om, False)
    for _ in range(3):
        assert b.search(net, sync=False) is None
        b.selfplay_move(temperature_moves=3, emit_targets=False)
    c = _counters(b)
    print(c)
    assert c["searches"] == 3
    # 4 batches per thread + 1..3 extra chain-splitting rounds per search
    assert 3 * (STEPS + 1) <= c["rounds"] <= 3 * (STEPS + 3)
    assert c["nn_launches"] == c["rounds"] * LAUNCHES_PER_ROUND
    assert c["rows"] == c["rounds"] * ROWS_PER_ROUND
    assert c["tree_launches"] == c["rounds"] * K
    assert c["finals"] == c["searches"] * K
    assert 0 < c["busy_launches"] <= c["nn_launches"]
    assert c["ms"] > 0 and c["sel"] > 0 and c["bk"] > 0 and c["busy"] > 0


def test_free_running_unequal_groups_sliced_launches(om, net):
    """One free-running call of 3 moves: only the base chunks (3 x 4 + 1
    rounds) are timed, none of their rounds is a backup-only final round; the
    games equal the lock-step call's."""
    a, ref = _grouped_engine(om, True), _grouped_engine(om, False)
    before = _counters(a)
    assert before["nn_launches"] == 0 and before["searches"] == 0
    oa = a.selfplay_steps(net, 3, temperature_moves=3, opening_moves=0, emit_targets=False)
    oc = ref.selfplay_steps(net, 3, temperature_moves=3, opening_moves=0, emit_targets=False)
    torch.cuda.synchronize()
    c = _counters(a)
    print(c)
    base = 3 * STEPS + 1
    assert c["nn_launches"] == base * LAUNCHES_PER_ROUND
    assert c["rows"] == base * ROWS_PER_ROUND
    assert c["tree_launches"] == base * K
    assert c["finals"] == before["finals"] == 0
    assert c["searches"] == 3 and c["rounds"] >= base
    assert c["busy_launches"] > 0 and c["ms"] > 0 and c["sel"] > 0
    for k in ("actions", "finished"):
        assert torch.equal(oa[k], oc[k]), k
    va, qa = a.root_stats()
    vc, qc = ref.root_stats()
    assert torch.equal(va, vc) and torch.equal(qa, qc)
    assert [a.visit_counts(g) for g in range(G)] == [ref.visit_counts(g) for g in range(G)]


def test_thread_split_accounting(om, net):
    """One game, T=3 virtual threads: a timing block, a tree launch and a
    ResNet launch of B rows per (round, thread); not a grouped search."""
    t, bsz, steps = 3, 8, 4
    b = om.BatchedMCTS(1, history_size=4, num_simulations=96, num_threads=t, batch_size=bsz, seed=9,
                       node_capacity=1 << 14)
    b.engine.enable_timing(1)
    for _ in range(2):
        assert b.search(net, sync=False) is None
        b.selfplay_move(temperature_moves=3, emit_targets=False)
    c = _counters(b)
    print(c)
    assert c["nn_launches"] == 2 * steps * t
    assert c["rows"] == 2 * steps * t * bsz
    assert c["tree_launches"] == 2 * steps * t
    assert c["finals"] == 2 * t
    assert c["searches"] == 0 and c["rounds"] == 0
    assert 0 < c["busy_launches"] <= c["nn_launches"]
    assert c["ms"] > 0 and c["sel"] > 0 and c["bk"] > 0 and c["busy"] > 0
