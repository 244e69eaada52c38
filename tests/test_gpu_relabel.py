"""ReplayBuffer(track_exact=True).relabel_endgames on the GPU
(csrc/replay.hip k_replay_endgame_list / k_replay_endgame_apply around
csrc/solver.hip) against the numpy restatement tests/relabel_ref.py: every case
compares the ring (boards, policy, value, player, exact) and the counters bit
for bit. Positions come from tests/golden/endgames.npz; the reference looks
their solutions up there (its own earlier results) instead of searching again.
"""

import functools

import numpy as np
import pytest
import torch

import endgame_ref as E
import relabel_ref as L
import replay_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
UNKNOWN, GAVE_UP = L.EXACT_UNKNOWN, L.EXACT_GAVE_UP


@functools.lru_cache(maxsize=None)
def fix():
    f = L.fixture()
    return f, L.replay_positions(f), L.table_solver(f)


def with_empties(lo, hi):
    f, pos, _ = fix()
    return [p for p, e, b in zip(pos, f["empties"], f["best_action"]) if lo <= e <= hi and b >= 0]


def to_dev(out):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in out.items()}


class Pair:
    """A tracked ReplayBuffer and its reference, fed and relabelled together."""

    def __init__(self, G, H, cap, max_moves=128, rb=None):
        import othello_mcts as om

        self.rb = rb or om.ReplayBuffer(G, H, cap, max_moves=max_moves, device=DEV, track_exact=True)
        self.ref = L.RelabelRef(G, H, cap, max_moves=max_moves, solve=fix()[2])

    def add(self, moves, stacked=False):
        for out in ([R.stack(moves)] if stacked else moves):
            self.ref.add(out)
            self.rb.add(to_dev(out))

    def relabel(self, max_empties=10, budget=4096, policy="keep", retry=False, node_limit=None, gives_up=None):
        kw = {} if node_limit is None else {"node_limit": node_limit}
        assert self.rb.relabel_endgames(max_empties, budget, policy=policy, retry=retry, **kw) is None
        self.ref.relabel_endgames(max_empties, budget, policy=policy, retry=retry, gives_up=gives_up)

    def check(self):
        assert_same(self.rb, self.ref)


def assert_same(rb, ref):
    assert (rb.size, rb.head, rb.games_completed) == (ref.size, ref.head, ref.games_completed)
    rb.check()
    assert ref.flags == 0
    assert np.array_equal(rb.boards.cpu().numpy(), ref.boards)
    assert np.array_equal(rb.player.cpu().numpy(), ref.player)
    got, want = rb.exact.cpu().numpy(), ref.exact
    assert np.array_equal(got, want), (np.nonzero(got != want)[0][:8], got[got != want][:8], want[got != want][:8])
    assert np.array_equal(rb.value.cpu().numpy().view(np.uint32), ref.value.view(np.uint32))
    assert np.array_equal(rb.policy.cpu().numpy().view(np.uint32), ref.policy.view(np.uint32))
    assert rb.relabel_counters.tolist() == ref.relabel_counters.tolist()
    assert rb.relabel_stats == dict(zip(("solved", "gave_up", "left", "taken"), ref.relabel_counters.tolist()))
    assert np.array_equal(rb.exact_scores().cpu().numpy(), ref.exact_scores())


def grouped(positions, outcome_of, sizes=(1, 2, 3)):
    """Games of 1, 2, 3, 1, ... consecutive positions; a game's outcome is
    chosen by its first position."""
    games, i, k = [], 0, 0
    while i < len(positions):
        n = sizes[k % len(sizes)]
        games.append((positions[i:i + n], outcome_of(positions[i], k)))
        i, k = i + n, k + 1
    return games


def disagreeing(p, k):
    _, score, best = fix()[2](*p)
    return L.disagreeing_outcome(p[0], L.mover_score(p[0], score, best), k)


# ------------------------------------------------------------------ 1. the whole fixture
@pytest.mark.parametrize("policy", ["keep", "optimal"])
@pytest.mark.parametrize("H", [1, 8])
def test_whole_fixture(H, policy):
    f, pos, _ = fix()
    rng = np.random.default_rng(10 * H + len(policy))
    pair = Pair(3, H, 300, max_moves=4)
    pair.add(L.games_script(rng, 3, H, grouped(pos, disagreeing)))
    pair.check()
    ref = pair.ref
    assert ref.size == len(pos) == 274
    v0, p0 = ref.value.copy(), ref.policy.copy()
    pair.relabel(10, policy=policy)
    pair.check()
    live = ref.live_slots()
    empties = np.array([64 - L.popcount(int(a) | int(b)) for a, b in ref.boards[live, :2]])
    e = ref.exact[live]
    assert (e[empties > 10] == UNKNOWN).all() and (empties > 10).sum() == 22
    assert np.array_equal(ref.value[live][empties > 10], v0[live][empties > 10])
    assert (np.abs(e[empties <= 10].astype(int)) <= 64).all()
    # an apply kernel that does nothing cannot pass: most game outcomes disagree with the exact sign
    changed = v0[live][empties <= 10] != ref.value[live][empties <= 10]
    assert changed.mean() >= 0.5
    assert (p0 != ref.policy).any() == (policy == "optimal")
    assert ref.relabel_counters.tolist() == [252, 0, 0, 252]
    pair.relabel(12, policy=policy)
    pair.check()
    assert (np.abs(ref.exact[live].astype(int)) <= 64).all()
    assert ref.relabel_counters.tolist() == [274, 0, 0, 22]


# ------------------------------------------------------------------ 2. the mover's view
def test_movers_view():
    f, pos, solve = fix()
    terminal = [p for p, b in zip(pos, f["best_action"]) if b < 0]
    four = [p for p, e in zip(pos, f["empties"]) if e == 4][:8]
    assert len(terminal) == 8 and len(four) == 8
    both = [(player, p[1], p[2]) for p in terminal + four for player in (1, 2)]
    rng = np.random.default_rng(2)
    pair = Pair(2, 2, 40)
    pair.add(L.games_script(rng, 2, 2, [([p], 1 + k % 3) for k, p in enumerate(both)]))
    pair.relabel(10, policy="optimal")
    pair.check()
    ref = pair.ref
    got = {}
    for slot in ref.live_slots().tolist():
        got[(int(ref.player[slot]) + 1, int(ref.boards[slot, 0]), int(ref.boards[slot, 1]))] = \
            (int(ref.exact[slot]), float(ref.value[slot]))
    assert len(got) == 32
    nonzero = 0
    for _, p1, p2 in terminal:
        diff = L.popcount(p1) - L.popcount(p2)
        assert got[(1, p1, p2)] == (diff, np.sign(diff)) and got[(2, p1, p2)] == (-diff, -np.sign(diff))
        nonzero += diff != 0
    assert nonzero >= 6
    for _, p1, p2 in four:  # both colours searched by the independent reference itself
        for player in (1, 2):
            _, score, best = E.solve(player, p1, p2)
            assert got[(player, p1, p2)][0] == L.mover_score(player, score, best)


# ------------------------------------------------------------------ 3. age order and budget
def test_age_order_and_budget():
    cands = with_empties(5, 10)
    rng = np.random.default_rng(3)
    # 45 records through a ring of 32: the first 13 (candidates too) are overwritten; of the 32 live ones 20
    # are candidates
    is_cand = [True] * 13 + [k % 8 not in (2, 5, 7) for k in range(32)]
    assert sum(is_cand[13:]) == 20
    it = iter(cands)
    records = [next(it) if c else None for c in is_cand]
    pair = Pair(1, 1, 32, max_moves=4)
    pair.add(L.games_script(rng, 1, 1, grouped(records, lambda p, k: 1 + k % 3)))
    ref = pair.ref
    assert ref.head == 13 and ref.size == 32
    live_cand = np.array(is_cand[13:])
    for call, (left, taken) in enumerate([(15, 5), (10, 5), (5, 5), (0, 5), (0, 0)]):
        pair.relabel(10, budget=5)
        pair.check()
        assert ref.relabel_counters.tolist() == [min(20, 5 * (call + 1)), 0, left, taken]
        labelled = ref.exact_scores() != UNKNOWN
        want = np.zeros(32, dtype=bool)
        want[np.nonzero(live_cand)[0][:5 * (call + 1)]] = True  # the oldest candidates first
        assert np.array_equal(labelled, want)


# ------------------------------------------------------------------ 4. the list kernel's chunk boundaries
@functools.lru_cache(maxsize=None)
def chunk_script():
    cands = with_empties(6, 10)
    n, cap = 2500, 2100
    at = [0, 1023, 1024, 2047, 2048, cap - 1]  # live indices; live index i is record n - cap + i
    records = [None] * n
    for k in range(n - cap):  # overwritten candidates before the live window
        if k % 7 == 0:
            records[k] = cands[k % len(cands)]
    for k, i in enumerate(at):
        records[n - cap + i] = cands[k]
    rng = np.random.default_rng(4)
    games = [(records[i:i + 100], 1 + (i // 100) % 3) for i in range(0, n, 100)]
    return R.stack(L.games_script(rng, 1, 1, games)), at


@pytest.mark.parametrize("budget", [8, 3])
def test_chunk_boundaries(budget):
    script, at = chunk_script()
    pair = Pair(1, 1, 2100)
    pair.ref.add(script)
    pair.rb.add(to_dev(script))
    ref = pair.ref
    assert ref.size == 2100 and ref.head == 400
    pair.relabel(10, budget=budget)
    pair.check()
    taken = min(budget, 6)
    assert ref.relabel_counters.tolist() == [taken, 0, 6 - taken, taken]
    assert np.nonzero(ref.exact_scores() != UNKNOWN)[0].tolist() == at[:taken]
    pair.relabel(10, budget=budget)
    pair.check()
    assert np.nonzero(ref.exact_scores() != UNKNOWN)[0].tolist() == at
    assert ref.relabel_counters.tolist() == [6, 0, 0, 6 - taken]


# ------------------------------------------------------------------ 5. overwritten slots
def test_overwrite_forgets_the_label():
    cands = with_empties(4, 9)
    rng = np.random.default_rng(5)
    first = [([cands[0], None, cands[1]], 2), ([cands[2]], 3), ([None, cands[3], cands[4]], 1)]  # 7 records
    later = [([None, cands[5]], 3), ([cands[6], None], 2)]  # overwrites slots 0..3
    a, b = Pair(1, 2, 7, max_moves=4), Pair(1, 2, 7, max_moves=4)  # a: one add per move; b: stacked adds
    m1, m2 = L.games_script(rng, 1, 2, first), L.games_script(rng, 1, 2, later)
    a.add(m1)
    b.add(m1, stacked=True)
    for pair in (a, b):
        pair.relabel(10)
        pair.check()
        assert pair.ref.relabel_counters.tolist() == [5, 0, 0, 5]
    a.add(m2)
    b.add(m2, stacked=True)
    for pair in (a, b):
        pair.check()
        ref = pair.ref
        assert ref.head == 4 and (ref.exact[:5] == UNKNOWN).all() and (ref.exact[5:] != UNKNOWN).all()  # 4: filler
        # the new games' outcomes (white won, then black won), negated where white is to move
        assert np.array_equal(ref.value[:4], np.float32([-1, -1, 1, 1]) * np.where(ref.player[:4], -1, 1))
        pair.relabel(10)
        pair.check()
        assert ref.relabel_counters.tolist() == [7, 0, 0, 2]
        assert (ref.exact[[1, 2]] != UNKNOWN).all() and (ref.exact[[0, 3]] == UNKNOWN).all()
    for k in ("boards", "policy", "value", "player", "exact", "relabel_counters", "counters"):
        assert torch.equal(getattr(a.rb, k).view(torch.uint8), getattr(b.rb, k).view(torch.uint8)), k


# ------------------------------------------------------------------ 6. giving up
def wipeouts():
    """Black to move with 8, 9 and 10 empties whose only action (square 0)
    takes white's last disc: one node per root action, so they are solved even
    with node_limit=10. The fixture's own positions of 8 to 10 empties all
    exceed that limit."""
    out = []
    for extra in ([], [47], [47, 56]):
        empty = {0, *range(40, 47), *extra}
        white = 1 << (63 - 1)
        black = sum(1 << (63 - s) for s in range(64) if s not in empty and s != 1)
        out.append((1, black, white))
    return out


def test_giving_up_and_retry():
    import othello_mcts as om

    f, pos, _ = fix()
    hard = [p for e in (8, 9, 10) for p in with_empties(e, e)[:3]]
    easy = wipeouts()
    records = [hard[0], easy[0], hard[1], hard[2], easy[1]] + hard[3:] + [easy[2]]
    assert [64 - L.popcount(p[1] | p[2]) for p in easy] == [8, 9, 10]

    def gives_up(*p):
        return om.solve_position(p, 10, 10)["flags"] != 0

    stopped = [gives_up(*p) for p in records]
    assert sum(stopped) == 9 and not any(gives_up(*p) for p in easy)  # some, not all
    overlap = (2, hard[0][1] | 1 << 20, hard[0][2] | 1 << 20)  # a corrupted record: square 43 on both sides
    assert overlap[1] & overlap[2] and 64 - L.popcount(overlap[1] | overlap[2]) <= 10
    records.insert(4, overlap)
    rng = np.random.default_rng(6)
    pair = Pair(2, 1, 16)
    pair.add(L.games_script(rng, 2, 1, grouped(records, lambda p, k: 1 + k % 3)))
    ref = pair.ref
    v0, p0 = ref.value.copy(), ref.policy.copy()
    pair.relabel(10, policy="optimal", node_limit=10, gives_up=gives_up)
    pair.check()
    assert ref.relabel_counters.tolist() == [3, 10, 0, 13]
    gave = ref.exact == GAVE_UP
    assert gave.sum() == 10 and np.array_equal(ref.value[gave], v0[gave]) and np.array_equal(ref.policy[gave], p0[gave])
    pair.relabel(10, policy="optimal")  # examined already: skipped
    pair.check()
    assert ref.relabel_counters.tolist() == [3, 10, 0, 0]
    pair.relabel(10, policy="optimal", retry=True)  # the default limit solves all but the corrupted record
    pair.check()
    assert ref.relabel_counters.tolist() == [12, 11, 0, 10]
    assert (ref.exact == GAVE_UP).sum() == 1


# ------------------------------------------------------------------ 7. off means off
def test_off_means_off():
    import othello_mcts as om

    G, H, cap, max_moves = 3, 2, 16, 6
    rng = np.random.default_rng(7)
    moves = R.random_script(rng, G, H, 24, max_len=max_moves)
    ref = R.ReplayRef(G, H, cap, max_moves=max_moves)
    tracked = om.ReplayBuffer(G, H, cap, max_moves=max_moves, device=DEV, track_exact=True)
    plain = om.ReplayBuffer(G, H, cap, max_moves=max_moves, device=DEV)
    for out in moves[:10]:
        ref.add(out)
        tracked.add(to_dev(out))
        plain.add(to_dev(out))
    ref.add(R.stack(moves[10:]))
    tracked.add(to_dev(R.stack(moves[10:])))
    plain.add(to_dev(R.stack(moves[10:])))
    assert ref.size == cap
    for k in ("boards", "policy", "value", "player", "stage_boards", "stage_policy", "stage_player", "moves",
              "counters"):
        assert torch.equal(getattr(tracked, k).view(torch.uint8), getattr(plain, k).view(torch.uint8)), k
    assert np.array_equal(plain.boards.cpu().numpy(), ref.boards)
    assert np.array_equal(plain.value.cpu().numpy().view(np.uint32), ref.value.view(np.uint32))
    ids = torch.from_numpy(rng.integers(0, 8 * cap, size=200))
    for x, y in zip(tracked.gather(ids), plain.gather(ids)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert (tracked.exact == UNKNOWN).all() and tracked.relabel_counters.tolist() == [0, 0, 0, 0]
    with pytest.raises(RuntimeError, match="track_exact=True"):
        plain.relabel_endgames()
    assert not hasattr(plain, "exact") and not hasattr(plain, "relabel_counters")
    today = {"boards", "policy", "value", "player", "stage_boards", "stage_policy", "stage_player", "moves",
             "counters", "num_games", "history_size", "capacity", "max_moves"}
    assert set(plain.state_dict()) == today
    assert set(tracked.state_dict()) == today | {"exact", "relabel_counters"}
    assert tracked.nbytes == plain.nbytes + cap + 32
    assert plain.nbytes == cap * (16 * H + 265) + G * max_moves * (16 * H + 261) + 8 * G + 32


# ------------------------------------------------------------------ 8. sentinels around everything
SENTINEL = {torch.float32: 12345.5, torch.int64: 0x5A5A5A5A5A5A5A5A, torch.int32: 0x5A5A5A5A, torch.uint8: 0xA5,
            torch.int8: 0x5A}


class Bracketed:
    """A tensor between two sentinel margins of ``pad`` rows; ``inner`` is the
    part handed out, holding ``fill``."""

    def __init__(self, like, pad=1, fill=0):
        raw = torch.int64 if like.dtype == torch.uint64 else like.dtype
        self.raw, self.pad = raw, pad
        self.big = torch.full((like.shape[0] + 2 * pad, *like.shape[1:]), SENTINEL[raw], dtype=raw, device=DEV)
        self.inner = self.big[pad:-pad]
        self.inner.fill_(fill)
        if like.dtype == torch.uint64:
            self.inner = self.inner.view(torch.uint64)

    def intact(self):
        s = SENTINEL[self.raw]
        return bool((self.big[:self.pad] == s).all()) and bool((self.big[-self.pad:] == s).all())


@pytest.mark.parametrize("budget", [4096, 1])
def test_sentinels_and_pad_rows(budget):
    import othello_mcts as om
    from othello_mcts._othello_mcts_impl import _relabel_workspace_bytes

    cands = with_empties(5, 10)[:9]
    records = [None, cands[0], cands[1], None] + cands[2:] + [None]
    rb = om.ReplayBuffer(2, 3, 12, max_moves=5, device=DEV, track_exact=True)
    guards = {}
    for name in ("boards", "policy", "value", "player", "stage_boards", "stage_policy", "stage_player", "moves",
                 "_pending", "counters", "exact", "relabel_counters"):
        guards[name] = Bracketed(getattr(rb, name), fill=UNKNOWN if name == "exact" else 0)
        setattr(rb, name, guards[name].inner)
    # the workspace between 256-byte margins, so that it stays aligned
    guards["workspace"] = Bracketed(torch.empty(_relabel_workspace_bytes(budget), dtype=torch.uint8), pad=256)
    rb._relabel_ws[budget] = guards["workspace"].inner
    pair = Pair(2, 3, 12, max_moves=5, rb=rb)
    rng = np.random.default_rng(8)
    pair.add(L.games_script(rng, 2, 3, grouped(records, lambda p, k: 1 + k % 3)))
    assert pair.ref.size == 12 and pair.ref.head == 0  # full, and the last live slot is the ring's last
    for call in range(10 if budget == 1 else 2):
        pair.relabel(10, budget=budget, policy="optimal")
        pair.check()
    assert rb._relabel_ws[budget] is guards["workspace"].inner and len(rb._relabel_ws) == 1
    assert pair.ref.relabel_counters.tolist() == [9, 0, 0, 0]
    assert all(g.intact() for g in guards.values()), [k for k, g in guards.items() if not g.intact()]


# ------------------------------------------------------------------ 9. real self-play
def test_real_self_play_end_to_end():
    import othello_mcts as om
    from othello_mcts.synthetic import alphazero_state_dict
    from othello_mcts.training import train_epoch_replay

    G, H = 16, 2
    net = om.NativeNet(alphazero_state_dict(4, 5, 128, 1, 32), device=0)
    b = om.BatchedMCTS(G, history_size=H, num_simulations=16, num_threads=1, batch_size=8, seed=3,
                       node_capacity=1 << 14)
    rb = om.ReplayBuffer(G, H, 4096, device=DEV, track_exact=True)
    while rb.games_completed < G:
        rb.add(b.selfplay_steps(net, 8, emit_targets=True, keep_all=True))
    rb.check()
    size = rb.size
    assert rb.head == size < 4096
    v0 = rb.value[:size].cpu().numpy()
    p0 = rb.policy[:size].cpu().numpy()
    rb.relabel_endgames(8)
    boards, player = rb.boards[:size].cpu().numpy(), rb.player[:size].cpu().numpy()
    value, exact = rb.value[:size].cpu().numpy(), rb.exact[:size].cpu().numpy()
    near = changed = 0
    for i in range(size):
        p1, p2 = int(boards[i, 0]), int(boards[i, 1])
        if 64 - L.popcount(p1 | p2) <= 8:
            _, score, best = E.solve(int(player[i]) + 1, p1, p2)
            assert best >= 0  # self-play stores no terminal position
            assert exact[i] == score and value[i] == np.sign(score), i
            near += 1
            changed += value[i] != v0[i]
        else:
            assert exact[i] == UNKNOWN and value[i] == v0[i], i
    assert near >= 8 * G // 2
    assert rb.relabel_stats == {"solved": near, "gave_up": 0, "left": 0, "taken": near}
    assert np.array_equal(rb.policy[:size].cpu().numpy(), p0)  # policy="keep"
    print(f"relabelled {near} of {size} positions, {changed} values changed")

    class Toy(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lin = torch.nn.Linear((1 + 2 * H) * 64, 66)

        def forward(self, x):
            y = self.lin(x.flatten(1))
            return {"policy": torch.softmax(y[:, :65], 1), "value": torch.tanh(y[:, 65])}

    torch.manual_seed(0)
    toy = Toy().to(DEV)
    means = train_epoch_replay(toy, torch.optim.SGD(toy.parameters(), lr=0.1), rb, 256,
                               generator=torch.Generator().manual_seed(1))
    assert set(means) == {"total_loss", "policy_loss", "value_loss", "l2_loss"}
    assert all(np.isfinite(v) for v in means.values())
    rb.check()


# ------------------------------------------------------------------ 10. persistence
def test_state_dict_round_trip_of_a_half_labelled_buffer():
    import othello_mcts as om

    cands = with_empties(5, 10)[10:22]
    records = [c for pair in zip(cands, [None] * 12) for c in pair]  # 24 records through a ring of 20
    rng = np.random.default_rng(9)
    a = Pair(2, 2, 20, max_moves=4)
    a.add(L.games_script(rng, 2, 2, grouped(records, lambda p, k: 1 + k % 3)))
    a.relabel(10, budget=4, policy="optimal")
    a.check()
    assert a.ref.relabel_counters.tolist()[2] > 0  # half labelled
    sd = a.rb.state_dict()
    assert sd["exact"].dtype == torch.int8 and sd["relabel_counters"].tolist() == a.ref.relabel_counters.tolist()
    assert all(t.device.type == "cpu" for t in sd.values() if isinstance(t, torch.Tensor))
    copy = om.ReplayBuffer(2, 2, 20, max_moves=4, device=DEV, track_exact=True)
    copy.load_state_dict(sd)
    a.relabel(10, policy="optimal")
    a.check()
    copy.relabel_endgames(10, policy="optimal")
    assert_same(copy, a.ref)
    # the keys are demanded exactly when tracking is on, and the codes are checked
    plain = om.ReplayBuffer(2, 2, 20, max_moves=4, device=DEV)
    with pytest.raises(ValueError, match="track_exact=False"):
        plain.load_state_dict(sd)
    without = {k: v for k, v in sd.items() if k not in ("exact", "relabel_counters")}
    plain.load_state_dict(without)
    with pytest.raises(ValueError, match="track_exact=True"):
        copy.load_state_dict(without)
    for bad in (-126, -65, 65, 127):
        broken = dict(sd, exact=sd["exact"].clone())
        broken["exact"][3] = bad
        with pytest.raises(ValueError, match="an exact code outside"):
            copy.load_state_dict(broken)
    assert_same(copy, a.ref)  # a refused state changes nothing
