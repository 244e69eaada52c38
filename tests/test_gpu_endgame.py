"""The exact endgame solver on the GPU (csrc/solver.hip) against the fixture
tests/golden/endgames.npz (solved by the independent Python reference
tests/endgame_ref.py), against the host solver (same code, so equal node
counts), and end to end through BatchedMCTS.root_positions /
endgame_move_loss.

Node totals in the docstrings were computed with the host solver, which visits
the same nodes as the device: every test stays below 2 x 10^8 nodes."""

import functools
from pathlib import Path

import numpy as np
import pytest
import torch

import endgame_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NONE = -128
BIG = 1 << 40


@functools.lru_cache(maxsize=None)
def fixture():
    z = np.load(Path(__file__).parent / "golden" / "endgames.npz")
    return {k: z[k] for k in z.files}


def triples(idx=None):
    f = fixture()
    idx = range(len(f["player"])) if idx is None else idx
    return [(int(f["player"][i]), int(f["p1"][i]), int(f["p2"][i])) for i in idx]


@functools.lru_cache(maxsize=None)
def solved_all():
    """The whole fixture in one call on the default grid; shared, read only."""
    import othello_mcts as om

    s = om.solve_endgames(triples(), 12, BIG)
    return {k: getattr(s, k).cpu().numpy() for k in ("move_scores", "score", "best_action", "flags", "nodes")}


@functools.lru_cache(maxsize=None)
def host_all():
    import othello_mcts as om

    return [om.solve_position(p, 12, BIG) for p in triples()]


def assert_equals_fixture(s, idx):
    f = fixture()
    idx = list(idx)
    assert np.array_equal(s["move_scores"], f["move_scores"][idx])
    assert np.array_equal(s["score"], f["score"][idx])
    assert np.array_equal(s["best_action"], f["best_action"][idx])
    assert not s["flags"].any()


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_device_equals_fixture_small_batches(n):
    """The n deepest positions of the fixture (12 empties first). 65 positions:
    8,443,451 nodes."""
    import othello_mcts as om

    f = fixture()
    idx = np.argsort(-f["empties"], kind="stable")[:n].tolist()
    s = om.solve_endgames(triples(idx), 12, BIG)
    s.check()
    assert_equals_fixture({k: getattr(s, k).cpu().numpy() for k in ("move_scores", "score", "best_action", "flags")},
                          idx)


def test_device_equals_fixture_and_host_nodes():
    """All 274 positions in one call (8,532,650 nodes): outputs equal the
    fixture, node counts equal the host solver's per position."""
    s = solved_all()
    assert_equals_fixture(s, range(len(s["score"])))
    assert s["nodes"].tolist() == [h["nodes"] for h in host_all()]
    assert s["move_scores"].tolist() == [h["move_scores"] for h in host_all()]


def test_one_workgroup_equals_default_grid_and_runs_repeat():
    """274 positions = 17,810 slots through one 64-lane workgroup (every lane
    refills ~280 times), and the default grid a second time: 2 x 8,532,650
    nodes. Scores, flags and nodes are identical."""
    import othello_mcts as om

    base = solved_all()
    one = om.solve_endgames(triples(), 12, BIG, _workgroups=1)
    again = om.solve_endgames(triples(), 12, BIG)
    for k, v in base.items():
        assert np.array_equal(getattr(one, k).cpu().numpy(), v), k
        assert np.array_equal(getattr(again, k).cpu().numpy(), v), k


SENTINEL = {torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int32: 0x5A5A5A5A, torch.uint8: 0xA5}


class Bracketed:
    """A tensor between two sentinel rows; ``inner`` is the part handed out."""

    def __init__(self, shape, dtype):
        self.dtype = dtype
        self.big = torch.full((shape[0] + 2, *shape[1:]), SENTINEL[dtype], dtype=dtype, device=DEV)
        self.inner = self.big[1:-1]

    def intact(self):
        s = SENTINEL[self.dtype]
        return bool((self.big[0] == s).all()) and bool((self.big[-1] == s).all())


def test_outputs_stay_between_sentinel_rows():
    """65 positions (8,443,451 nodes) through the raw entry point with every
    output and the workspace bracketed by sentinel rows."""
    import othello_mcts as om
    from othello_mcts import _othello_mcts_impl as impl

    f = fixture()
    idx = np.argsort(-f["empties"], kind="stable")[:65].tolist()
    n = len(idx)
    pos = om.endgame.pack_positions(triples(idx)).to(DEV)
    ws_rows = impl._solve_workspace_bytes(n)
    B = {"move_scores": Bracketed((n, 65), torch.int32), "score": Bracketed((n,), torch.int32),
         "best_action": Bracketed((n,), torch.int32), "flags": Bracketed((n,), torch.int32),
         "nodes": Bracketed((n,), torch.int64)}
    # the workspace as rows of 8 bytes: 32 rows of counter block + one per slot
    assert ws_rows == 256 + n * 65 * 8
    ws = Bracketed((ws_rows // 8,), torch.int64)
    for grid in (0, 1, 3):
        for b in B.values():
            b.inner.fill_(SENTINEL[b.dtype])
        impl._gpu_solve(0, pos.data_ptr(), n, 12, BIG, B["move_scores"].inner.data_ptr(), B["score"].inner.data_ptr(),
                        B["best_action"].inner.data_ptr(), B["flags"].inner.data_ptr(), B["nodes"].inner.data_ptr(),
                        ws.inner.data_ptr(), grid, torch.cuda.current_stream(DEV).cuda_stream)
        torch.cuda.synchronize()
        assert all(b.intact() for b in B.values()) and ws.intact(), grid
        assert_equals_fixture({k: b.inner.cpu().numpy() for k, b in B.items()}, idx)
    # optional outputs: only move_scores
    B["move_scores"].inner.fill_(SENTINEL[torch.int32])
    impl._gpu_solve(0, pos.data_ptr(), n, 12, BIG, B["move_scores"].inner.data_ptr(), 0, 0, 0, 0, ws.inner.data_ptr(), 0,
                    torch.cuda.current_stream(DEV).cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(B["move_scores"].inner.cpu().numpy(), f["move_scores"][idx])
    assert all(b.intact() for b in B.values()) and ws.intact()


def test_flagged_rows_leave_their_neighbours_alone():
    """The 36 positions of the fixture with 9 and 10 empties, interleaved
    with rows that are refused: too many empties (12 > max 10), overlapping
    discs, player 3, and, in a second call with node_limit 10, every searched
    row. First call 36 solvable rows: 720,194 nodes."""
    import othello_mcts as om
    from othello_mcts import endgame as E

    f = fixture()
    good = [i for i in range(len(f["player"])) if 9 <= f["empties"][i] <= 10]
    deep = [i for i in range(len(f["player"])) if f["empties"][i] == 12]
    rows, want = [], []
    for j, i in enumerate(good):
        rows.append(triples([i])[0])
        want.append(("good", i))
        kind = j % 3
        if kind == 0:
            rows.append(triples([deep[j % len(deep)]])[0])
            want.append(("flag", E.FLAG_TOO_MANY_EMPTIES))
        elif kind == 1:
            player, p1, p2 = triples([i])[0]
            rows.append((player, p1 | 1 << 30, p2 | 1 << 30))
            want.append(("flag", E.FLAG_INVALID))
        else:
            rows.append((3,) + triples([i])[0][1:])
            want.append(("flag", E.FLAG_INVALID))
    s = om.solve_endgames(rows, 10, BIG)
    ms, score, best, flags, nodes = (getattr(s, k).cpu().numpy() for k in
                                     ("move_scores", "score", "best_action", "flags", "nodes"))
    for r, (what, v) in enumerate(want):
        if what == "good":
            assert flags[r] == 0 and np.array_equal(ms[r], f["move_scores"][v])
            assert score[r] == f["score"][v] and best[r] == f["best_action"][v] and nodes[r] == host_all()[v]["nodes"]
        else:
            assert flags[r] == v and (ms[r] == NONE).all() and score[r] == NONE and best[r] == -1 and nodes[r] == 0
    assert len(rows) == 72
    with pytest.raises(RuntimeError, match=r"36 of 72 positions were not solved: 12 x more empties than max_empties, "
                                           r"24 x invalid position"):
        s.check()
    # node limit 10: every searched row gives up at once; terminal rows between them are untouched
    terminal = [i for i in range(len(f["player"])) if f["best_action"][i] < 0][:8]
    mixed = []
    for j, i in enumerate(good[:16]):
        mixed += [triples([i])[0], triples([terminal[j % 8]])[0]]
    s = om.solve_endgames(mixed, 10, 10)
    flags, score, best, ms = (getattr(s, k).cpu().numpy() for k in ("flags", "score", "best_action", "move_scores"))
    assert (flags[0::2] == E.FLAG_NODE_LIMIT).all() and (score[0::2] == NONE).all() and (best[0::2] == -1).all()
    assert (flags[1::2] == 0).all() and (ms[1::2] == NONE).all() and (best[1::2] == -1).all()
    assert score[1::2].tolist() == [int(f["score"][terminal[j % 8]]) for j in range(16)]
    h = [om.solve_position(p, 10, 10) for p in mixed]
    assert s.nodes.cpu().tolist() == [x["nodes"] for x in h]
    assert ms.tolist() == [x["move_scores"] for x in h]


@pytest.mark.parametrize("empties,count,seed", [(12, 64, 5), (14, 16, 11)])
def test_perfect_play_is_self_consistent(empties, count, seed):
    """Depths the Python reference cannot afford: follow best_action with the
    batched apply_action and solve again after every ply (a pass is a ply).
    The score negates at every ply, i.e. it stays the first prediction for the
    first mover, and the final disc difference is that prediction.
    64 positions at 12 empties: 43,792,132 nodes over all plies;
    16 at 14 empties: 93,467,618 (the seed with the smallest largest
    search of 24 tried on the host: one lane searches one root action, so the
    largest root action sets the time)."""
    import othello_mcts as om
    from othello_mcts import _othello_mcts_impl as impl

    pos = om.endgame.pack_positions(om.endgame.random_play_positions(empties, count, seed)).to(DEV)
    first_player = (pos[:, 0] & 3).clone()
    s = om.solve_endgames(pos, empties, BIG)
    s.check()
    predicted = s.score.to(torch.int64).clone()
    assert bool((s.best_action >= 0).all())
    done = torch.zeros(count, dtype=torch.bool, device=DEV)
    plies = 0
    while not bool(done.all()):
        plies += 1
        assert plies <= 2 * empties + 2
        actions = torch.where(s.best_action >= 0, s.best_action, torch.full_like(s.best_action, 64)).contiguous()
        nxt = torch.empty_like(pos)
        impl._gpu_apply_action(pos.data_ptr(), actions.data_ptr(), nxt.data_ptr(), count,
                               torch.cuda.current_stream(DEV).cuda_stream)
        pos = torch.where(done[:, None], pos, nxt).contiguous()
        s = om.solve_endgames(pos, empties, BIG)
        s.check()
        player = pos[:, 0] & 3
        over = s.best_action < 0
        assert bool((over == (player == 0)).all())
        # a terminal score is black minus white; otherwise it is the mover's
        mover_is_first = torch.where(over, first_player == 1, player == first_player)
        for_first = torch.where(mover_is_first, s.score.to(torch.int64), -s.score.to(torch.int64))
        assert torch.equal(for_first, predicted), plies
        done = over
    black = torch.tensor([bin(int(x) & (2**64 - 1)).count("1") for x in pos[:, 1].cpu()])
    white = torch.tensor([bin(int(x) & (2**64 - 1)).count("1") for x in pos[:, 2].cpu()])
    final = torch.where(first_player.cpu() == 1, black - white, white - black)
    assert torch.equal(final, predicted.cpu())


def small_engine(seed):
    import othello_mcts as om
    from othello_mcts.synthetic import alphazero_state_dict

    net = om.NativeNet(alphazero_state_dict(4, 5, 128, 0, 32), device=0)
    b = om.BatchedMCTS(8, history_size=2, num_simulations=32, num_threads=1, batch_size=8, dirichlet_epsilon=0.0,
                       seed=seed, node_capacity=1 << 14)
    return b, net


def test_root_positions_equals_root_info():
    b, _ = small_engine(11)
    b.random_openings(40, seed=3)
    roots = b.root_positions()
    assert roots.shape == (8, 5) and roots.dtype == torch.int64 and roots.device == DEV
    rows = roots.cpu().numpy().view(np.uint64)
    seen = set()
    for g in range(8):
        info = b.root_info(g)
        assert int(rows[g, 0]) & 0xFFFFFFFF == info["player"]
        assert [int(x) for x in rows[g, 1:]] == [info["player1_discs"], info["player2_discs"], info["legal_moves"],
                                                 info["next_legal_moves"]]
        seen.add(int(rows[g, 1]))
    assert len(seen) > 1  # the openings differ


def test_endgame_move_loss_end_to_end():
    """8 games of a small net (128x0b, H = 2, 32 simulations) from random
    openings of up to 52 plies, played to the end; every recorded (root,
    action) with at most 8 empties against the Python reference. The solver
    runs with max_empties 8: at most 8 games x 8 roots of <= 8 empties, well
    under 10^6 nodes."""
    import othello_mcts as om

    b, net = small_engine(12)
    b.random_openings(52, seed=9)
    finished_once = torch.zeros(8, dtype=torch.bool, device=DEV)
    records = []
    for _ in range(70):
        roots = b.root_positions()
        sol = om.solve_endgames(roots, 8)
        b.search(net)
        out = b.selfplay_move(temperature_moves=0)
        actions = out["actions"].clone()
        loss, kept, empties = om.endgame_move_loss(roots, actions, 8, solution=sol)
        again = om.endgame_move_loss(roots, actions, 8)
        assert all(torch.equal(x, y) for x, y in zip((loss, kept, empties), again))
        live = ~finished_once  # a restarted game is back at 60 empties: recorded as -1 rows
        records.append([t.cpu().numpy() for t in (roots, actions, loss, kept, empties, sol.best_action, live)])
        finished_once |= (out["finished"] & 3) != 0
        if bool(finished_once.all()):
            break
    assert bool(finished_once.all())
    checked = 0
    for roots, actions, loss, kept, empties, best, live in records:
        rows = roots.view(np.uint64)
        for g in range(8):
            player, p1, p2 = int(rows[g, 0]) & 3, int(rows[g, 1]), int(rows[g, 2])
            assert empties[g] == 64 - R.popcount(p1 | p2)
            if empties[g] > 8 or actions[g] < 0 or player == 0:
                assert loss[g] == -1 and kept[g] == -1
                continue
            ms, score, ref_best = R.solve(player, p1, p2)
            a = int(actions[g])
            assert ms[a] != NONE and loss[g] == score - ms[a] and loss[g] >= 0, (g, a)
            assert kept[g] == int(np.sign(ms[a]) == np.sign(score))
            assert best[g] == ref_best
            if a == ref_best:
                assert loss[g] == 0
            checked += 1
    assert checked >= 30  # 8 games x their last plies
