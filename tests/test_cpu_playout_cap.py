"""Playout cap randomization without a GPU: the full / fast draw
against its mirror on the oracle's random stream, the new C struct's layout,
and the oracle helper the GPU tests lean on."""

import ctypes
import subprocess

import numpy as np
import pytest

import oracle as O
import playout_cap_ref as R
from conftest import ROOT


class PlayoutCap(ctypes.Structure):
    _fields_ = [("full_probability", ctypes.c_float), ("fast_simulations", ctypes.c_int32)]


def _keys(n, seed):
    rng = np.random.default_rng(seed)
    return [int(k) for k in rng.integers(0, 1 << 64, size=n, dtype=np.uint64)]


@pytest.mark.parametrize("p", [0.25, 0.5, 1.0])
def test_playout_cap_is_full_equals_the_mirror(p):
    """10,000 (key, ply) pairs: the exported draw is the oracle-stream mirror's;
    at p = 1 every search is full; at p < 1 the full share is near p."""
    import othello_mcts as om

    keys = _keys(100, 7)
    got = np.array([[om.playout_cap_is_full(k, ply, p) for ply in range(100)] for k in keys])
    want = np.array([[R.is_full(k, ply, p) for ply in range(100)] for k in keys])
    assert got.size == 10000 and (got == want).all()
    if p == 1.0:
        assert got.all()
    else:
        # binomial: 4 sigma of 10,000 draws
        assert abs(got.mean() - p) < 4 * np.sqrt(p * (1 - p) / got.size)


def test_draw_uses_no_event_of_the_normal_stream():
    """The draw's event has bit 63 set; events of a game's stream count up from
    0. Sixteen keys x 18 plies at p = 0.5: both classes occur and every key has
    a full search right after a fast one (what the GPU parity test relies on)."""
    keys = _keys(16, 3)
    d = np.array([[R.is_full(k, ply, 0.5) for ply in range(18)] for k in keys])
    assert 0.35 < d.mean() < 0.65
    assert all((~row[:-1] & row[1:]).any() for row in d)
    L = O.lib()
    for k in keys[:4]:
        assert L.orc_stream_key(k, (1 << 63) | 5, 0) != L.orc_stream_key(k, 5, 0)


def test_playout_cap_struct_has_the_headers_layout(tmp_path):
    """oamd_playout_cap as a C compiler lays the header out (the method of
    tests/test_cpu_capi.py)."""
    src = tmp_path / "probe.c"
    src.write_text("\n".join([
        "#include <stddef.h>", "#include <stdio.h>", '#include "othello_mcts_amd.h"', "int main(void) {",
        '    printf("%zu %zu %zu %zu %zu\\n", sizeof(oamd_playout_cap), offsetof(oamd_playout_cap, full_probability),',
        "           offsetof(oamd_playout_cap, fast_simulations), sizeof(((oamd_playout_cap *)0)->full_probability),",
        "           sizeof(((oamd_playout_cap *)0)->fast_simulations));",
        "    return 0;", "}", ""]))
    subprocess.run(["g++", "-x", "c", "-std=c99", "-Wall", "-Werror", "-I", str(ROOT / "include"), str(src), "-o",
                    str(tmp_path / "probe")], check=True)
    out = subprocess.run([str(tmp_path / "probe")], check=True, capture_output=True, text=True).stdout.split()
    size, off_p, off_n, w_p, w_n = map(int, out)
    assert size == ctypes.sizeof(PlayoutCap) == 8
    assert (off_p, off_n) == (PlayoutCap.full_probability.offset, PlayoutCap.fast_simulations.offset) == (0, 4)
    assert (w_p, w_n) == (4, 4)


def test_new_symbols_are_exported_and_abi_version_stays():
    import capi_host as H

    raw = ctypes.CDLL(str(H.LIB_PATH))
    for name in ("oamd_engine_set_playout_cap", "oamd_playout_cap_is_full", "oamd_engine_selfplay_steps_budget"):
        assert hasattr(raw, name), name
        assert name in H.HEADER.read_text()
    assert raw.oamd_abi_version() == 1
    fn = raw.oamd_playout_cap_is_full
    fn.argtypes = [ctypes.c_uint64, ctypes.c_int32, ctypes.c_float]
    fn.restype = ctypes.c_int
    assert fn(12345, 3, 1.0) == 1
    assert fn(12345, 3, 0.5) == int(R.is_full(12345, 3, 0.5))


def test_python_surface():
    import othello_mcts as om
    from othello_mcts import selfplay

    assert om.FIN_FAST == selfplay.FIN_FAST == 128
    assert "FIN_FAST" in om.__all__ and "playout_cap_is_full" in om.__all__
    assert "FIN_FAST" in selfplay.__all__


def test_oracle_budget_changes_through_the_handle():
    """A poked oracle runs 64 simulations with root noise, then 16 without
    (one event per simulation: the symmetry draws only), then 64 again on the
    reused tree."""
    kw = dict(history_size=4, num_simulations=64, num_threads=2, batch_size=8, dirichlet_epsilon=0.25)
    r = R.BudgetedOracle(game_key=99, **kw)
    assert r.search(O.equivariant_stub) == 64
    e1 = r.events()
    assert e1 > 64  # symmetry draws and root noise vectors
    a = O.legal_actions(r.position())[int(np.argmax(r.visit_counts()))]
    r.apply_action(a)
    n0 = r.root_visit_count()
    r.set_fast(16)
    assert r.search(O.equivariant_stub) == 16
    assert r.events() - e1 == 16  # no noise events
    assert r.root_visit_count() == n0 + 16
    e2 = r.events()
    r.set_full()
    assert r.search(O.equivariant_stub) == 64
    assert r.events() - e2 > 64
    assert r.root_visit_count() == n0 + 16 + 64
