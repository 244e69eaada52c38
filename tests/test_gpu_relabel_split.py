"""ReplayBuffer.relabel_endgames(split=True) on the GPU: the split solver
(csrc/solver.hip k_solve_plan / k_solve_items / k_solve_split_reduce, DESIGN.md
§15) between the unchanged list and apply kernels of csrc/replay.hip. On the
fixture-filled ring of tests/test_gpu_relabel.py the ring, ``exact`` and the
counters are bit for bit those of ``split=False`` and of the numpy restatement
tests/relabel_ref.py. No node limit binds (2^24 per item or root action; the
whole fixture takes fewer nodes), so both modes label the same positions.

Node totals (host twin): the 274 positions take 3,535,116 nodes with the
split solver, 8,532,650 with the current one."""

import functools

import numpy as np
import pytest
import torch

import relabel_ref as L

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
LIMIT = 1 << 24


@functools.lru_cache(maxsize=None)
def fix():
    f = L.fixture()
    return f, L.replay_positions(f), L.table_solver(f)


def to_dev(out):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in out.items()}


def grouped(positions, outcome_of, sizes=(1, 2, 3)):
    games, i, k = [], 0, 0
    while i < len(positions):
        n = sizes[k % len(sizes)]
        games.append((positions[i:i + n], outcome_of(positions[i], k)))
        i, k = i + n, k + 1
    return games


def disagreeing(p, k):
    _, score, best = fix()[2](*p)
    return L.disagreeing_outcome(p[0], L.mover_score(p[0], score, best), k)


def ring_state(rb):
    return {"boards": rb.boards.cpu().numpy(), "player": rb.player.cpu().numpy(), "exact": rb.exact.cpu().numpy(),
            "value": rb.value.cpu().numpy().view(np.uint32), "policy": rb.policy.cpu().numpy().view(np.uint32),
            "counters": np.array(rb.relabel_counters.tolist()), "scores": rb.exact_scores().cpu().numpy()}


@pytest.mark.parametrize("policy", ["keep", "optimal"])
@pytest.mark.parametrize("H", [1, 8])
def test_whole_fixture_split_equals_plain_and_reference(H, policy):
    import othello_mcts as om

    f, pos, solve = fix()
    rng = np.random.default_rng(10 * H + len(policy))
    script = L.games_script(rng, 3, H, grouped(pos, disagreeing))
    split = om.ReplayBuffer(3, H, 300, max_moves=4, device=DEV, track_exact=True)
    plain = om.ReplayBuffer(3, H, 300, max_moves=4, device=DEV, track_exact=True)
    ref = L.RelabelRef(3, H, 300, max_moves=4, solve=solve)
    for out in script:
        ref.add(out)
        split.add(to_dev(out))
        plain.add(to_dev(out))
    assert ref.size == len(pos) == 274
    v0 = ref.value.copy()
    assert split.relabel_endgames(12, node_limit=LIMIT, policy=policy, split=True) is None
    plain.relabel_endgames(12, node_limit=LIMIT, policy=policy)
    ref.relabel_endgames(12, 4096, policy=policy, retry=False, gives_up=None)
    a, b = ring_state(split), ring_state(plain)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    split.check()
    assert (split.size, split.head, split.games_completed) == (ref.size, ref.head, ref.games_completed)
    assert np.array_equal(a["boards"], ref.boards) and np.array_equal(a["player"], ref.player)
    assert np.array_equal(a["exact"], ref.exact)
    assert np.array_equal(a["value"], ref.value.view(np.uint32))
    assert np.array_equal(a["policy"], ref.policy.view(np.uint32))
    assert a["counters"].tolist() == ref.relabel_counters.tolist() == [274, 0, 0, 274]
    assert np.array_equal(a["scores"], ref.exact_scores())
    # the labels are there: every live slot is exact, and most game outcomes disagreed with the exact sign
    live = ref.live_slots()
    assert (np.abs(ref.exact[live].astype(int)) <= 64).all()
    assert (v0[live] != ref.value[live]).mean() >= 0.5
    # each mode keeps its own workspace, sized by its own query
    from othello_mcts import _othello_mcts_impl as impl

    assert list(split._relabel_split_ws) == [4096] and not split._relabel_ws
    assert split._relabel_split_ws[4096].numel() == impl._relabel_split_workspace_bytes(4096)
    assert list(plain._relabel_ws) == [4096] and not plain._relabel_split_ws
    # a second call finds nothing left and changes nothing
    split.relabel_endgames(12, node_limit=LIMIT, policy=policy, split=True)
    again = ring_state(split)
    assert again["counters"].tolist() == [274, 0, 0, 0]
    assert all(np.array_equal(again[k], a[k]) for k in a if k != "counters")


def test_untracked_buffer_raises_as_before():
    import othello_mcts as om

    rb = om.ReplayBuffer(3, 1, 64, max_moves=4, device=DEV)
    with pytest.raises(RuntimeError, match="relabel_endgames needs a buffer created with track_exact=True"):
        rb.relabel_endgames(12, node_limit=LIMIT, split=True)
