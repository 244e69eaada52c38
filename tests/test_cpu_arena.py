"""Arena pieces that need no GPU: the paired openings, ArenaResult's
bookkeeping, and the preconditions of tests/test_gpu_arena.py checked on the
CPU reference matches alone (tests/arena_ref.py)."""

import numpy as np
import pytest
import torch

import arena_ref as R

import othello_mcts as om
from othello_mcts.arena import UNFINISHED, ArenaResult, paired_openings


def test_paired_openings_are_legal_paired_and_seeded():
    ops = paired_openings(10, 6, seed=3)
    assert ops.shape == (10, 6) and ops.dtype == np.int32
    for row in ops:
        p = om.Position.initial_position()
        for a in row:
            assert a >= 0  # no game ends within 6 plies
            p = p.apply_action(int(a))  # raises on an illegal action
    for i in range(5):
        assert (ops[2 * i] == ops[2 * i + 1]).all()
    assert len({tuple(r) for r in ops}) > 1  # the pairs differ
    assert (paired_openings(10, 6, seed=3) == ops).all()
    assert (paired_openings(10, 6, seed=4) != ops).any()
    odd = paired_openings(5, 2, seed=0)  # an odd count: the last opening has one match
    assert odd.shape == (5, 2) and (odd >= 0).all()
    assert paired_openings(4, 0).shape == (4, 0)


def _result(result, white, discs=None, actions=None):
    G = len(result)
    return ArenaResult(actions=torch.zeros((1, G), dtype=torch.int32) if actions is None else actions,
                       result=torch.tensor(result), a_is_white=torch.tensor(white),
                       discs=torch.zeros((G, 2), dtype=torch.int64) if discs is None else discs, plies=1)


def test_arena_result_counts_from_a_side_and_respects_swaps():
    # match: 0 black wins, A black -> A wins; 1 white wins, A white -> A wins;
    # 2 white wins, A black -> A loses; 3 black wins, A white -> A loses; 4 draw; 5 unfinished
    r = _result([1, 2, 2, 1, 0, UNFINISHED], [False, True, False, True, True, False])
    assert r.wdl() == (2, 1, 2)
    assert r.score_a() == pytest.approx((2 + 0.5) / 6)
    rec = r.records("new", "old")
    assert rec == [
        {"player1": "new", "player2": "old", "result": 1},
        {"player1": "old", "player2": "new", "result": 2},
        {"player1": "new", "player2": "old", "result": 2},
        {"player1": "old", "player2": "new", "result": 1},
        {"player1": "old", "player2": "new", "result": 0},
    ]
    # a white win in a swapped match is a win for A
    assert _result([2], [True]).wdl() == (1, 0, 0) and _result([2], [False]).wdl() == (0, 0, 1)
    assert _result([2], [True]).score_a() == 1.0


def test_arena_needs_matching_engines_without_touching_the_gpu():
    class Fake:
        def __init__(self, n, dev):
            self.num_games, self.device = n, torch.device(dev)

    with pytest.raises(ValueError, match="same number of games"):
        om.Arena(Fake(4, "cuda:0"), Fake(8, "cuda:0"))
    with pytest.raises(ValueError, match="same device"):
        om.Arena(Fake(4, "cuda:0"), Fake(4, "cuda:1"))


# (plies after the opening, passes, tied moves, black discs, white discs) of the
# eight reference matches with argmax moves
ARGMAX_GAMES = [(56, 0, 23, 19, 45), (56, 0, 18, 10, 54), (58, 2, 12, 36, 28), (55, 0, 10, 42, 21),
                (56, 0, 12, 50, 14), (59, 3, 8, 58, 6), (55, 0, 19, 56, 7), (56, 0, 13, 34, 30)]


@pytest.mark.parametrize("temperature_moves", [0, 6])
def test_reference_matches_cover_what_the_gpu_test_needs(temperature_moves):
    """The GPU parity test compares against these matches; they must exercise a
    forced pass, games of different lengths (a finished match beside running
    ones), a random tie-break in every game and wins for both colours."""
    ms = R.reference_matches(temperature_moves)
    games = [R.summary(m) for m in ms]
    assert sum(g[1] for g in games) >= 1, games            # a pass
    assert len({g[0] for g in games}) >= 3, games          # three distinct lengths
    assert all(g[2] >= 1 for g in games), games            # a tie-broken move in every game
    assert {m["result"] for m in ms} >= {1, 2}, games      # wins for both colours
    assert all(g[3] + g[4] <= 64 for g in games)
    if temperature_moves == 0:
        assert games == ARGMAX_GAMES
    else:
        assert min(g[0] for g in games) == 56 and max(g[0] for g in games) == 60
        assert sum(g[1] > 0 for g in games) >= 4
        # the sampled plies change every game
        assert all(a != b for a, b in zip(games, ARGMAX_GAMES))
    # both sides move in every match, the opening is shared by a pair
    for g, m in enumerate(ms):
        assert {p["a_moves"] for p in m["plies"]} == {True, False}
        assert m["plies"][0]["before"] == ms[g ^ 1]["plies"][0]["before"]
        assert m["plies"][0]["a_moves"] == (g % 2 == 0)  # black moves after 4 plies; A is black in even matches
