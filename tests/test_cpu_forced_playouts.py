"""Forced playouts and policy target pruning without a GPU: the
Python reference tests/forced_ref.py against the oracle, the host pruning rule
against the reference, the vacuity guards of the GPU tests' cases, and the new
surface."""

import ctypes
import functools
import subprocess

import numpy as np
import pytest

import asym_stub as A
import forced_ref as R
import oracle as O
from conftest import ROOT


def _bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


# ------------------------------------------------- 1. the reference is a yardstick
SHAPES = {
    "T1B8": dict(num_threads=1, batch_size=8, history_size=2, num_simulations=64, dirichlet_epsilon=0.25),
    "T2B8": dict(num_threads=2, batch_size=8, history_size=4, num_simulations=64, dirichlet_epsilon=0.25),
    "T2B4": dict(num_threads=2, batch_size=4, history_size=2, num_simulations=32, dirichlet_epsilon=0.0),
}


@pytest.mark.parametrize("stub", ["equivariant", "asymmetric"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_unforced_reference_equals_the_oracle(shape, stub):
    """forced_k = 0: 12 plies with tree reuse, everything the oracle reports bit
    for bit, and the move choice (temperature sampling for 6 plies, then argmax)."""
    kw, nn = SHAPES[shape], R.stub_of(stub)
    key = A.game_key(3, 1)
    o = O.OracleMCTS(game_key=key, **kw)
    r = R.ForcedMCTS(game_key=key, **kw)
    for ply in range(12):
        assert o.search(nn) == r.search(nn)
        assert o.visit_counts() == r.visit_counts(), ply
        assert np.array_equal(_bits(o.mean_action_values()), _bits(r.mean_action_values())), ply
        assert o.root_visit_count() == r.root_visit_count()
        assert (o.events(), o.node_count()) == (r.events(), r.node_count()), ply
        fo, po = o.self_play_data()
        fr, pr = r.self_play_data()
        assert np.array_equal(fo, fr) and np.array_equal(_bits(po), _bits(pr)), ply
        a = o.selfplay_action(ply, 6, 1.0)
        assert r.selfplay_action(ply, 6, 1.0) == a, ply
        assert o.events() == r.events()
        o.apply_action(a)
        r.apply_action(a)


def test_fast_search_of_the_reference_equals_the_budgeted_oracle():
    """The reference's fast search (n simulations, no noise) against the oracle
    poked to the same budget (tests/playout_cap_ref.py)."""
    import playout_cap_ref as C

    kw = SHAPES["T2B8"]
    o = C.BudgetedOracle(game_key=99, **kw)
    r = R.ForcedMCTS(game_key=99, **kw)
    for ply, fast in enumerate([False, True, True, False, True, False]):
        if fast:
            o.set_fast(16)
        else:
            o.set_full()
        assert o.search(O.equivariant_stub) == r.search(O.equivariant_stub, 16 if fast else None)
        assert o.visit_counts() == r.visit_counts() and o.events() == r.events(), ply
        a = o.selfplay_action(ply, 12, 1.0)
        assert r.selfplay_action(ply) == a
        o.apply_action(a)
        r.apply_action(a)


# --------------------------------------------------- 2. the host rule == the reference
def _random_root(rng):
    nc = int(rng.integers(1, 34))
    kind = rng.integers(4)
    n = rng.integers(0, 801, size=nc)
    if kind == 0:  # a search-like root: one child far ahead, many barely tried
        n = np.where(rng.random(nc) < 0.6, rng.integers(0, 4, size=nc), n)
    q = rng.uniform(-1.0, 1.0, size=nc).astype(np.float32)
    p = rng.dirichlet(np.full(nc, 0.3 if kind == 1 else 1.0)).astype(np.float32)
    n_root = int(n.sum()) + int(rng.integers(0, 3))
    return n_root, n.astype(np.int32), q, p


def test_host_pruning_equals_the_reference_on_random_roots():
    import othello_mcts as om

    rng = np.random.default_rng(2024)
    hits: set = set()
    changed = 0
    for i in range(4000):
        n_root, n, q, p = _random_root(rng)
        k = (2.0, 0.5, 8.0)[i % 3]
        want = R.prune(n_root, n, q, p, k=k, hits=hits)
        got = om.prune_visit_counts(n_root, n, q, p, k=k)
        assert got.dtype == np.int32 and np.array_equal(got, want), (i, n, q, p, got, want)
        assert (got <= n).all() and (got >= 0).all()
        changed += bool((got < n).any())
    assert changed > 1000
    assert {"single", "cap_stop", "puct_stop", "nothing", "one_dropped", "zeroed", "tie"} <= hits, hits


HAND = {
    # name: (visits, q, priors, expected branch, expected counts or None)
    "single": ([5], [0.1], [1.0], "single", [5]),
    "unvisited": ([0, 0, 0], [0.0, 0.0, 0.0], [0.5, 0.3, 0.2], "unvisited", [0, 0, 0]),
    # cap = (int)sqrt(2 * 0.02 * 120) = 2 and the child stays far below ubest
    "cap binds": ([100, 20], [0.5, -0.9], [0.9, 0.02], "cap_stop", [100, 18]),
    # cap = 10, but with 8 visits the child's score passes ubest
    "puct binds": ([100, 10], [0.5, -0.9], [0.5, 0.5], "puct_stop", [100, 8]),
    # 2 -> 1 by the loop, then the single playout is dropped
    "left at one": ([100, 2], [0.5, -1.0], [0.9, 0.1], "one_dropped", [100, 0]),
    # cap = (int)sqrt(2 * 0.001 * 101) = 0: nothing may be taken, the playout stays
    "one kept": ([100, 1], [0.5, -1.0], [0.99, 0.001], "one_kept", [100, 1]),
    # best = the first of the two largest; the second is pruned like any other child
    "tie": ([50, 50, 3], [0.2, 0.2, -1.0], [0.45, 0.45, 0.1], "tie", None),
    # q_j >= ubest: nothing is subtracted
    "q above": ([100, 10], [0.0, 0.9], [0.5, 0.5], "nothing", [100, 10]),
}


@pytest.mark.parametrize("name", list(HAND))
def test_host_pruning_hand_made_cases(name):
    import othello_mcts as om

    n, q, p, branch, expect = HAND[name]
    hits: set = set()
    want = R.prune(sum(n) + 1, n, q, p, hits=hits)
    assert branch in hits, (branch, hits)
    got = om.prune_visit_counts(sum(n) + 1, np.array(n, np.int32), np.array(q, np.float32), np.array(p, np.float32))
    assert np.array_equal(got, want), (got, want)
    if expect is not None:
        assert list(got) == expect
    if name == "tie":
        assert got[0] == 50 and got[1] <= 50 and got[2] == 0


# ------------------------------------------------------------- 3. vacuity guards
@functools.lru_cache(maxsize=None)
def _guard(name):
    return R.run_case_on_cpu(name)


@pytest.mark.parametrize("name", list(R.CASES))
def test_the_gpu_cases_can_see_the_feature(name):
    """With the reference alone: k = 2 changes the visit counts of at least a
    quarter of the case's full searches against k = 0 (same actions), and
    pruning takes a visit from at least half of their targets."""
    _guard(name).check()


def test_pruning_zeroes_a_child_somewhere():
    assert _guard("plain").zeroed > 0


def test_wide_and_pass_roots_are_what_they_claim():
    p = O.initial_position()
    for a in R.WIDE_PREFIX:
        assert a in O.legal_actions(p)
        p = O.apply_action(p, a)
    assert len(O.legal_actions(p)) >= 17
    p = O.initial_position()
    for a in R.PASS_PREFIX:
        assert a in O.legal_actions(p)
        p = O.apply_action(p, a)
    assert p.player != 0 and O.legal_actions(p) == [64]


# ------------------------------------------------------ 4. validation and surface
@pytest.mark.parametrize("k", [0.0, -1.0, float("nan"), float("inf")])
def test_bad_k_is_rejected_before_a_device_is_touched(k):
    import othello_mcts as om

    class NoDevice:
        @property
        def engine(self):
            raise AssertionError("the engine was touched")

    with pytest.raises(ValueError, match="k > 0"):
        om.BatchedMCTS.set_forced_playouts(NoDevice(), k)
    one = np.ones(2, np.float32)
    with pytest.raises(ValueError, match="k > 0"):
        om.prune_visit_counts(3, np.array([2, 1], np.int32), one, one / 2, k=k)


def test_prune_visit_counts_rejects_bad_arrays():
    import othello_mcts as om

    one = np.ones(2, np.float32)
    with pytest.raises(ValueError):
        om.prune_visit_counts(3, np.array([2, 1, 0], np.int32), one, one)
    with pytest.raises(ValueError, match="negative"):
        om.prune_visit_counts(3, np.array([2, -1], np.int32), one, one)
    with pytest.raises(ValueError, match="n_children"):
        om.prune_visit_counts(3, np.ones(65, np.int32), np.ones(65, np.float32), np.ones(65, np.float32))
    assert om.prune_visit_counts(0, np.zeros(0, np.int32), np.zeros(0, np.float32), np.zeros(0, np.float32)).size == 0


def test_new_symbols_are_exported_and_abi_version_stays():
    import capi_host as H
    import othello_mcts as om

    raw = ctypes.CDLL(str(H.LIB_PATH))
    header = H.HEADER.read_text()
    for name in ("oamd_engine_set_forced_playouts", "oamd_prune_visit_counts", "oamd_engine_root_priors",
                 "oamd_engine_game_event"):
        assert hasattr(raw, name), name
        assert name in header
    assert raw.oamd_abi_version() == 1
    assert "prune_visit_counts" in om.__all__
    for name in ("set_forced_playouts", "root_priors"):
        assert hasattr(om.BatchedMCTS, name)
    # the C function itself, through ctypes: a cap-binding root and a bad k
    fn = raw.oamd_prune_visit_counts
    I32, F32 = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
    fn.argtypes = [ctypes.c_int32, ctypes.c_int32, I32, F32, F32, ctypes.c_float, ctypes.c_float, ctypes.c_float, I32]
    fn.restype = ctypes.c_int
    n, q, p, _, expect = HAND["cap binds"]
    out = (ctypes.c_int32 * 2)()
    args = ((ctypes.c_int32 * 2)(*n), (ctypes.c_float * 2)(*q), (ctypes.c_float * 2)(*p))
    assert fn(2, sum(n) + 1, *args, 20000.0, 2.5, 2.0, out) == 0 and list(out) == expect
    assert fn(2, sum(n) + 1, *args, 20000.0, 2.5, 0.0, out) != 0


def test_forced_playouts_struct_has_the_headers_layout(tmp_path):
    src = tmp_path / "probe.c"
    src.write_text("\n".join([
        "#include <stddef.h>", "#include <stdio.h>", '#include "othello_mcts_amd.h"', "int main(void) {",
        '    printf("%zu %zu %zu\\n", sizeof(oamd_forced_playouts), offsetof(oamd_forced_playouts, k),',
        "           offsetof(oamd_forced_playouts, prune_targets));", "    return 0;", "}", ""]))
    subprocess.run(["g++", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o",
                    str(tmp_path / "probe")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()
    assert list(map(int, out)) == [8, 0, 4]
