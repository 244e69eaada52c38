"""liboamd.so through a foreign ctypes host (tests/capi_host.py), on the device.

Every other GPU test reaches the C ABI through pybind_module.cpp, calls
oamd_engine_features / oamd_engine_set_evaluation with row_begin = 0 and all
G * L rows, and evaluates every row with a well-behaved stub. A host written
against include/othello_mcts_amd.h evaluates only the rows whose
oamd_engine_leaf_flags entry is set, in runs. Here:
  a  the reference's known answers through the documented (dense) loop;
  b  whole games of three games in one engine through the sparse host, every
     unflagged row poisoned, against one oracle per game bit for bit, with the
     rows the evaluator saw accounted for against the oracle's NN calls;
  c  k_features_f32 on partial row ranges between sentinel rows;
  d  the call-order errors, and lock step == the documented order at T = 1;
  e  the bitboard kernels and f the native net through the raw entry points.
All comparisons are exact (lists, assert_array_equal, bytes). tests/test_cpu_capi.py
pins the structures and prototypes used here against the header.
"""

import contextlib
import ctypes
import json

import numpy as np
import pytest
import torch

import asym_stub as A
import capi_host as H
import numerics
import oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = -3.0


def _config(history_size, num_simulations, num_threads, batch_size, dirichlet_epsilon, c_puct_base=20000.0,
            c_puct_init=2.5, dirichlet_alpha=0.5):
    return H.SearchConfig(history_size, num_simulations, num_threads, batch_size, c_puct_base, c_puct_init,
                          dirichlet_epsilon, dirichlet_alpha)


@contextlib.contextmanager
def _engine(num_games, seed, node_capacity=1 << 16, **cfg):
    assert H.device_count() >= 1
    e = H.Engine(num_games, _config(**cfg), seed, node_capacity)
    try:
        yield e
    finally:
        e.destroy()


def _f32(values):
    return np.array(values, np.float32)


def _bits(a: np.ndarray) -> bytes:
    return np.ascontiguousarray(a).tobytes()


# ------------------------------------------------------------ a. known answers
@pytest.mark.parametrize("case", json.load(open(H.ROOT / "tests" / "golden" / "mcts_known_answers.json"))["cases"],
                         ids=lambda c: c["name"])
def test_known_answers_through_the_dense_loop(golden_dir, case):
    """INTEGRATION.md §3's loop, bound with ctypes: the reference's visit
    counts ([145, 85, 288, 266] and [14, 14, 14, 14])."""
    assert (golden_dir / "mcts_known_answers.json").exists()
    with _engine(1, 1234, history_size=case["history_size"], num_simulations=case["num_simulations"],
                 num_threads=case["num_threads"], batch_size=case["batch_size"],
                 dirichlet_epsilon=case["dirichlet_epsilon"]) as e:
        for a in case["actions"]:
            e.apply_action(0, a)
        H.search_dense(e, O.equivariant_stub if case["stub"] == "equivariant" else O.uniform_stub)
        assert e.root_info(0)["visits"] == case["visit_counts"]
        assert e.status() == (0, 0)
        L = case["num_threads"] * case["batch_size"]
        steps = -(-case["num_simulations"] // L)
        assert e.work_counters()[0] == steps * L


# -------------------------------------------- b. whole games, the sparse host
@pytest.mark.parametrize("name", list(H.WHOLE_GAMES))
def test_sparse_host_plays_whole_games_like_the_oracle(name):
    """G = 3 games of one engine, greedy until the first ends. The host reads
    and evaluates flagged rows only, run by run, after handing every row the
    poison. Per search and game: visits, Q bits, 8-fold targets and the root
    equal the oracle's; the flagged rows' features are the non-zero rows the
    oracle handed its evaluator, in order; the work counters count them.

    Measured on the CPU oracle (tests/test_cpu_capi.py): A skips NN calls in
    6 / 5 / 5 searches of games 0 / 1 / 2 and has 19 / 26 / 23 NN calls with a
    terminal row, B 6 / 6 / 5 and 18 / 24 / 19; the floors are 3 and 10."""
    cfg = H.WHOLE_GAMES[name]
    G, seed = H.WHOLE_GAME_GAMES, H.WHOLE_GAME_SEED
    T, B = cfg["num_threads"], cfg["batch_size"]
    L, steps = T * B, H.search_steps(cfg)
    with _engine(G, seed, **cfg) as e:
        assert (e.G, e.L, e.rows, e.C) == (G, L, G * L, 1 + 2 * cfg["history_size"])
        keys = [e.game_key(g) for g in range(G)]
        assert keys == [A.game_key(seed, g) for g in range(G)]
        taps = [H.EvaluatorTap(A.asymmetric_stub) for _ in range(G)]
        refs = [O.OracleMCTS(game_key=keys[g], **cfg) for g in range(G)]
        poison = H.make_poison(e)
        assert bool(torch.isfinite(poison[0]).all()) and bool(torch.isfinite(poison[1]).all())
        skipped, zero_rows = [0] * G, [0] * G
        flagged = unflagged = partial_calls = calls = moves = 0
        while all(r.position().player != 0 for r in refs):
            sims0, evals0 = e.work_counters()
            trace = H.search_sparse(e, A.asymmetric_stub, poison)
            sims1, evals1 = e.work_counters()
            assert len(trace) == steps
            assert e.status() == (0, 0)
            n_flagged = sum(int(s.flags.sum()) for s in trace)
            assert sims1 - sims0 == G * steps * L
            assert evals1 - evals0 == n_flagged
            flagged += n_flagged
            unflagged += steps * G * L - n_flagged
            for s in trace:
                assert set(np.unique(s.flags)) <= {0, 1}
                assert sum(n for _, n in s.runs) == int(s.flags.sum()) == len(s.features)
                calls += len(s.runs)
                partial_calls += sum(1 for r0, n in s.runs if (r0, n) != (0, G * L))
            for g, (r, tap) in enumerate(zip(refs, taps)):
                tag = f"configuration {name} move {moves} game {g}"
                tap.clear()
                r.search(tap)
                info = e.root_info(g)
                assert info["visits"] == r.visit_counts(), tag
                np.testing.assert_array_equal(info["q"], _f32(r.mean_action_values()), err_msg=tag)
                f, p = e.self_play_data(g)
                rf, rp = r.self_play_data()
                np.testing.assert_array_equal(f, rf, err_msg=tag)
                np.testing.assert_array_equal(p, rp, err_msg=tag)
                assert info["position"] == r.position().tuple(), tag
                assert info["overflow"] == 0
                # row accounting: what this game's flagged rows showed the host
                mine, nn_calls, zero_calls = [], 0, 0
                for s in trace:
                    idx = np.flatnonzero(s.flags)
                    mine.append(s.features[idx // L == g])
                    batches = s.flags[g * L:(g + 1) * L].reshape(T, B)
                    waiting = batches.any(axis=1)
                    nn_calls += int(waiting.sum())
                    zero_calls += int((waiting & ~batches.all(axis=1)).sum())
                assert _bits(np.concatenate(mine)) == _bits(tap.nonzero_rows(e.C)), tag
                assert (nn_calls, zero_calls) == (len(tap.calls), tap.zero_row_calls()), tag
                skipped[g] += nn_calls < T * steps
                zero_rows[g] += zero_calls
            for g, r in enumerate(refs):
                a = O.legal_actions(r.position())[int(np.argmax(r.visit_counts()))]
                e.apply_action(g, a)
                r.apply_action(a)
            moves += 1
        for g, r in enumerate(refs):
            assert e.root_info(g)["position"] == r.position().tuple()
        numerics.record(f"capi sparse host {name} (T={T} B={B} S={cfg['num_simulations']})",
                        f"moves={moves} flagged_rows={flagged} unflagged_rows={unflagged} "
                        f"range_calls={calls} partial_range_calls={partial_calls} "
                        f"searches_with_skipped_nn_calls={skipped} nn_calls_with_terminal_row={zero_rows}")
        assert moves >= 30
        assert partial_calls > 0 and unflagged > 0
        assert min(skipped) >= H.SKIPPED_SEARCHES_FLOOR, skipped
        assert min(zero_rows) >= H.ZERO_ROW_CALLS_FLOOR, zero_rows


# ------------------------------------------------------- c. the range kernels
# (row_begin, rows) of G * L = 72 rows, L = 24, B = 8, four rows per block: one
# row, odd starts, a block and a bit, (23, 2) and (46, 5) across a game boundary
# (the second also ends mid-block), the last row of a game and of the engine,
# all rows from an odd start, and nothing. (70, 5) would end at row 75: refused.
RANGES = [(0, 1), (1, 3), (5, 5), (23, 2), (46, 5), (47, 1), (71, 1), (3 * 24 - 1, 1), (1, 71), (0, 0)]
BAD_RANGES = [(70, 5), (72, 1), (0, 73), (70, 3), (-1, 1), (0, -1), (-1, -1), (2**31 - 1, 1), (1, 2**31 - 1)]


def test_feature_ranges_write_their_rows_and_nothing_else():
    """One select of configuration B (72 rows a step, four rows per block in
    k_features_f32) on three mid-game roots. The full read is the oracle's
    features of each root under its stream's draws; every partial range
    (row_begin, rows) then writes rows * C * 64 floats equal to that slice,
    between 9 + 9 sentinel rows it must not touch. Ranges outside [0, G * L]
    raise IndexError, for features and set_evaluation both."""
    cfg = H.WHOLE_GAMES["B"]
    G, Hs = A.ROW_GAMES, cfg["history_size"]
    L = cfg["num_threads"] * cfg["batch_size"]
    with _engine(G, A.ROW_SEED, **cfg) as e:
        assert e.rows == G * L == 72
        for g in range(G):
            for a in A.ROW_PREFIXES[g]:
                e.apply_action(g, a)
        e.set_stream()
        e.search_begin()
        e.select()
        W = e.C * 64
        full_dev = torch.full((e.rows, W), SENTINEL, dtype=torch.float32, device=DEV)
        e.features(full_dev.data_ptr(), 0, e.rows)
        full = full_dev.cpu().numpy()
        for g in range(G):
            assert e.game_key(g) == A.ROW_KEYS[g]
            _, expected = A.expected_first_rows(A.ROW_KEYS[g], A.ROW_PREFIXES[g], Hs, L)
            np.testing.assert_array_equal(full[g * L:(g + 1) * L].reshape(L, e.C, 8, 8), expected, err_msg=f"game {g}")
        assert e.leaf_flags().tolist() == [1] * e.rows

        pad = 9
        for r0, n in RANGES:
            # a game's rows are its root under 8 transforms, so rows repeat: the slice
            # a range must return differs from the slices 1..4 rows off
            for d in (-4, -3, -2, -1, 1, 2, 3, 4):
                if n > 0 and 0 <= r0 + d and r0 + d + n <= e.rows:
                    assert _bits(full[r0 + d:r0 + d + n]) != _bits(full[r0:r0 + n]), (r0, n, d)
            buf = torch.full((pad + n + pad, W), SENTINEL, dtype=torch.float32, device=DEV)
            e.features(buf.data_ptr() + pad * W * 4, r0, n)
            got = buf.cpu().numpy()
            assert _bits(got[pad:pad + n]) == _bits(full[r0:r0 + n]), (r0, n)
            assert _bits(got[:pad]) == _bits(got[pad + n:]) == _bits(np.full((pad, W), SENTINEL, np.float32)), (r0, n)

        buf = torch.full((4, W), SENTINEL, dtype=torch.float32, device=DEV)
        pol = torch.zeros((4, 65), dtype=torch.float32, device=DEV)
        val = torch.zeros(4, dtype=torch.float32, device=DEV)
        for r0, n in BAD_RANGES:
            with pytest.raises(IndexError, match="row range out of range"):
                e.features(buf.data_ptr(), r0, n)
            with pytest.raises(IndexError, match="row range out of range"):
                e.set_evaluation(pol.data_ptr(), val.data_ptr(), r0, n)
        assert _bits(buf.cpu().numpy()) == _bits(np.full((4, W), SENTINEL, np.float32))
        numerics.record("capi feature ranges (configuration B)", f"ranges={len(RANGES)} refused={len(BAD_RANGES)}")


# --------------------------------------------------------------- d. call order
ONE_THREAD = dict(history_size=3, num_simulations=64, num_threads=1, batch_size=8, dirichlet_epsilon=0.25)


def test_calls_out_of_order_raise():
    with _engine(1, 3, **ONE_THREAD) as e:
        with pytest.raises(ValueError, match=r"select called out of order \(search_begin first\)"):
            e.select()
        with pytest.raises(ValueError, match="backup called before select"):
            e.backup()
        assert e.search_begin() == 8
        with pytest.raises(ValueError, match="backup called before select"):
            e.backup()
        H.search_dense(e, A.asymmetric_stub)  # begins again: 8 selects, one backup
        with pytest.raises(ValueError, match=r"select called out of order \(search_begin first\)"):
            e.select()
        with pytest.raises(ValueError, match="backup called before select"):
            e.backup()
        assert e.status() == (0, 0)
        assert sum(e.root_info(0)["visits"]) == 64 - 8


def test_lock_step_is_the_documented_order_with_one_thread():
    """T = 1: backing up after every select (the header's lock-step order) and
    the documented loop (select backs up the previous round) are the same
    search, and both are the oracle's."""
    with _engine(1, 3, **ONE_THREAD) as doc, _engine(1, 3, **ONE_THREAD) as lock:
        ref = O.OracleMCTS(game_key=doc.game_key(0), **ONE_THREAD)
        assert lock.game_key(0) == doc.game_key(0)
        feat = torch.empty((lock.rows, lock.C, 8, 8), dtype=torch.float32, device=DEV)
        for move in range(3):
            H.search_dense(doc, A.asymmetric_stub)
            lock.set_stream()
            for _ in range(lock.search_begin()):
                lock.select()
                lock.features(feat.data_ptr(), 0, lock.rows)
                pol, val = H.evaluate_on_host(A.asymmetric_stub, feat)
                lock.set_evaluation(pol.data_ptr(), val.data_ptr(), 0, lock.rows)
                lock.backup()
            ref.search(A.asymmetric_stub)
            a, b = doc.root_info(0), lock.root_info(0)
            assert a["visits"] == b["visits"] == ref.visit_counts(), move
            np.testing.assert_array_equal(a["q"], b["q"])
            np.testing.assert_array_equal(a["q"], _f32(ref.mean_action_values()))
            assert doc.status() == lock.status() == (0, 0)
            action = O.legal_actions(ref.position())[int(np.argmax(a["visits"]))]
            for m in (doc, lock):
                m.apply_action(0, action)
            ref.apply_action(action)


# ------------------------------------------ e. bitboard kernels, raw entry points
def _u64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _dev(a: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(DEV)


def _host(t: torch.Tensor, dtype) -> np.ndarray:
    return t.cpu().numpy().view(dtype)


def _sentinel_bytes(nbytes: int) -> torch.Tensor:
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)


def _sizes(n):
    return [n, 1, 0]


def test_bitboard_kernels_through_the_raw_abi(golden_dir):
    """oamd_get_legal_moves / oamd_get_flips / oamd_apply_action on device
    buffers against tests/golden/bitboards.npz (the arrays test_gpu_parity.py
    hands the pybind layer): the whole fixture, n = 1, n = 0 (OK, output
    untouched) and n = -1 (ValueError). Positions are records of the ctypes
    oamd_position structure."""
    L = H.lib()
    bb = np.load(golden_dir / "bitboards.npz")
    stream = H.current_stream(DEV)
    tail = 16  # sentinel bytes behind every output

    # legal moves
    pl, p1, p2, idx = bb["pos_player"], _u64(bb["pos_p1"]), _u64(bb["pos_p2"]), bb["lm_index"]
    me = np.concatenate([_u64(bb["rnd_me"]), np.where(pl[idx] == 1, p1[idx], p2[idx])])
    opp = np.concatenate([_u64(bb["rnd_opp"]), np.where(pl[idx] == 1, p2[idx], p1[idx])])
    want = np.concatenate([_u64(bb["rnd_legal"]), _u64(bb["lm_value"])])
    me_d, opp_d = _dev(me), _dev(opp)
    for n in _sizes(len(me)):
        out = _sentinel_bytes(8 * n + tail)
        L.oamd_get_legal_moves(me_d.data_ptr(), opp_d.data_ptr(), out.data_ptr(), n, stream)
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[:8 * n].view(np.uint64), want[:n])
        assert (got[8 * n:] == 0xA5).all(), n
    with pytest.raises(ValueError, match="n must be >= 0"):
        L.oamd_get_legal_moves(me_d.data_ptr(), opp_d.data_ptr(), out.data_ptr(), -1, stream)

    # flips
    i = bb["fl_index"]
    mv = np.uint64(1) << (np.uint64(63) - bb["fl_square"].astype(np.uint64))
    mv_d, fme_d, fopp_d, want = _dev(mv), _dev(me[i]), _dev(opp[i]), _u64(bb["fl_flips"])
    for n in _sizes(len(mv)):
        out = _sentinel_bytes(8 * n + tail)
        L.oamd_get_flips(mv_d.data_ptr(), fme_d.data_ptr(), fopp_d.data_ptr(), out.data_ptr(), n, stream)
        got = out.cpu().numpy()
        np.testing.assert_array_equal(got[:8 * n].view(np.uint64), want[:n])
        assert (got[8 * n:] == 0xA5).all(), n
    with pytest.raises(ValueError, match="n must be >= 0"):
        L.oamd_get_flips(mv_d.data_ptr(), fme_d.data_ptr(), fopp_d.data_ptr(), out.data_ptr(), -1, stream)

    # apply_action on oamd_position records
    rec_t = np.dtype(H.Position)
    assert rec_t.itemsize == ctypes.sizeof(H.Position) == 40
    par, act = bb["ch_parent"], bb["ch_action"].astype(np.int32)
    pl, p1, p2 = bb["pos_player"][par], _u64(bb["pos_p1"])[par], _u64(bb["pos_p2"])[par]
    lg = _u64(bb["pos_legal"])[par]
    mine, theirs = np.where(pl == 1, p1, p2), np.where(pl == 1, p2, p1)
    rec = np.zeros(len(par), rec_t)
    rec["player"], rec["player1_discs"], rec["player2_discs"], rec["legal_moves"] = pl, p1, p2, lg
    rec["next_legal_moves"] = np.where(lg == 0, O.legal_moves_n(theirs, mine), np.uint64(0))  # position.h:351-357
    first = H.Position.from_buffer_copy(rec[:1].tobytes())
    assert first.tuple() == (int(pl[0]), int(p1[0]), int(p2[0]), int(lg[0]), int(rec["next_legal_moves"][0]))
    rec_d, act_d = _dev(rec), _dev(act)
    for n in _sizes(len(par)):
        out = _sentinel_bytes(40 * n + tail)
        L.oamd_apply_action(rec_d.data_ptr(), act_d.data_ptr(), out.data_ptr(), n, stream)
        got = out.cpu().numpy()
        child = got[:40 * n].view(rec_t)
        np.testing.assert_array_equal(child["player"], bb["ch_player"][:n])
        np.testing.assert_array_equal(child["player1_discs"], _u64(bb["ch_p1"])[:n])
        np.testing.assert_array_equal(child["player2_discs"], _u64(bb["ch_p2"])[:n])
        np.testing.assert_array_equal(child["legal_moves"], _u64(bb["ch_legal"])[:n])
        assert (got[40 * n:] == 0xA5).all(), n
    with pytest.raises(ValueError, match="n must be >= 0"):
        L.oamd_apply_action(rec_d.data_ptr(), act_d.data_ptr(), out.data_ptr(), -1, stream)
    numerics.record("capi bitboards", f"legal={len(me)} flips={len(mv)} apply={len(par)} boards, and n = 1, 0, -1")


# ------------------------------------------------- f. the native net, raw ABI
NET_SHAPE = dict(in_channels=9, conv_channels=128, num_residual_blocks=1, value_head_hidden_channels=32)


@pytest.fixture(scope="module")
def om():
    import othello_mcts

    assert othello_mcts.device_count() >= 1
    return othello_mcts


@pytest.fixture(scope="module")
def state_dict(om):
    from othello_mcts.synthetic import alphazero_state_dict

    return alphazero_state_dict(7, 9, 128, 1, 32)


@contextlib.contextmanager
def _net(state_dict, dtype):
    net = H.Net(H.NetDesc(num_squares=64, num_actions=65, dtype=H.DTYPES[dtype], **NET_SHAPE))
    try:
        keys = net.state_keys()
        assert len(keys) == len([k for k in state_dict if not k.endswith("num_batches_tracked")])
        for key, numel in keys:
            assert numel == np.asarray(state_dict[key]).size, key
        net.load_state(state_dict)
        yield net
    finally:
        net.destroy()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_native_net_forward_through_the_raw_abi(om, state_dict, dtype):
    """oamd_net_create / state_key / load_state / forward bound with ctypes
    give, on 5 rows, the bits of om.NativeNet (the pybind path to the same
    kernel), and leave the 9 rows behind the outputs alone."""
    rows, pad = 5, 9
    chains = A.random_game_chains(1)[10:10 + rows]
    x = torch.from_numpy(np.stack([O.features(c, 4, k % 8) for k, c in enumerate(chains)])).to(DEV)
    assert x.shape == (rows, 9, 8, 8)
    want = om.NativeNet(state_dict, device=0, dtype=dtype)(x)
    with _net(state_dict, dtype) as net:
        pol = torch.full((rows + pad, 65), SENTINEL, dtype=torch.float32, device=DEV)
        val = torch.full((rows + pad,), SENTINEL, dtype=torch.float32, device=DEV)
        net.forward(x.data_ptr(), rows, pol.data_ptr(), val.data_ptr())
        pol, val = pol.cpu().numpy(), val.cpu().numpy()
    assert _bits(pol[:rows]) == _bits(want["policy"].cpu().numpy())
    assert _bits(val[:rows]) == _bits(want["value"].cpu().numpy())
    assert (pol[rows:] == SENTINEL).all() and (val[rows:] == SENTINEL).all()
    np.testing.assert_allclose(pol[:rows].sum(axis=1), 1.0, atol=1e-5)
    assert (np.abs(val[:rows]) <= 1.0).all()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_native_search_through_the_raw_abi(om, state_dict, dtype):
    """oamd_engine_search(engine, net) on handles made with ctypes against
    om.BatchedMCTS.search(NativeNet) with the same seed: same visits, same Q bits."""
    kw = dict(history_size=4, num_simulations=64, num_threads=2, batch_size=8, dirichlet_epsilon=0.25)
    b = om.BatchedMCTS(4, seed=5, node_capacity=1 << 16, **kw)
    want_work = b.search(om.NativeNet(state_dict, device=0, dtype=dtype))
    with _net(state_dict, dtype) as net, _engine(4, 5, **kw) as e:
        assert e.search(net) == tuple(want_work) == (4 * 64, want_work[1])
        assert want_work[1] > 0
        assert e.status() == (0, 0)
        for g in range(4):
            got, want = e.root_info(g), b.root_info(g)
            assert got["visits"] == want["visit_counts"], g
            assert sum(got["visits"]) == 64 - 16
            np.testing.assert_array_equal(got["q"], _f32(want["mean_action_values"]))
