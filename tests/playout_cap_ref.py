"""Test helpers for playout cap randomization.

The oracle fixes num_simulations and dirichlet_epsilon when an OracleMCTS is
created. A capped engine changes both between the searches of one game, so the
helper here changes them through the oracle's handle: ``struct orc_mcts``
(oracle/omcts_oracle.c) begins with four ints (history_size, num_simulations,
num_threads, batch_size) and four floats (c_puct_base, c_puct_init, eps,
alpha), so num_simulations is at byte 4 and eps at byte 24. All eight fields
are read back against the constructor's arguments before the first write, so
a layout change fails loudly instead of poking something else.

``is_full`` mirrors the engine's full / fast draw with the oracle's own
orc_stream_key and orc_uniform.
"""

from __future__ import annotations

import ctypes

import numpy as np

import oracle as O

_INT_FIELDS = ("history_size", "num_simulations", "num_threads", "batch_size")
_FLOAT_FIELDS = ("c_puct_base", "c_puct_init", "dirichlet_epsilon", "dirichlet_alpha")
_SIMS_OFFSET, _EPS_OFFSET = 4, 24


def is_full(game_key: int, ply: int, full_probability: float) -> bool:
    """full = uniform(stream_key(key, 2^63 | ply, 0), 0) < p, in float32 like the device."""
    L = O.lib()
    u = L.orc_uniform(L.orc_stream_key(game_key, (1 << 63) | ply, 0), 0)
    return bool(np.float32(u) < np.float32(full_probability))


class BudgetedOracle:
    """An OracleMCTS whose next search's simulation count and root noise weight
    can be set (a full search: the constructor's; a fast one: n simulations and
    no noise)."""

    def __init__(self, **kw):
        import inspect

        sig = inspect.signature(O.OracleMCTS.__init__).parameters
        self.kw = {k: kw.get(k, sig[k].default) for k in _INT_FIELDS + _FLOAT_FIELDS}
        self.mcts = O.OracleMCTS(**kw)
        self._ints = (ctypes.c_int32 * 4).from_address(self.mcts._h)
        self._floats = (ctypes.c_float * 4).from_address(self.mcts._h + 16)
        self._check_layout(self.kw["num_simulations"], self.kw["dirichlet_epsilon"])

    def _check_layout(self, sims: int, eps: float) -> None:
        want_i = [self.kw[k] if k != "num_simulations" else sims for k in _INT_FIELDS]
        want_f = [np.float32(self.kw[k] if k != "dirichlet_epsilon" else eps) for k in _FLOAT_FIELDS]
        got_i, got_f = list(self._ints), [np.float32(x) for x in self._floats]
        assert got_i == want_i, ("struct orc_mcts no longer begins with", _INT_FIELDS, got_i, want_i)
        assert got_f == want_f, ("struct orc_mcts floats moved", _FLOAT_FIELDS, got_f, want_f)
        assert ctypes.addressof(self._ints) + _SIMS_OFFSET == self.mcts._h + 4
        assert ctypes.addressof(self._floats) + 8 == self.mcts._h + _EPS_OFFSET

    def set_budget(self, num_simulations: int, eps: float) -> None:
        self._check_layout(self._ints[1], float(self._floats[2]))
        self._ints[1] = int(num_simulations)
        self._floats[2] = float(eps)
        self._check_layout(int(num_simulations), float(eps))

    def set_full(self) -> None:
        self.set_budget(self.kw["num_simulations"], self.kw["dirichlet_epsilon"])

    def set_fast(self, fast_simulations: int) -> None:
        self.set_budget(fast_simulations, 0.0)

    def __getattr__(self, name):
        return getattr(self.mcts, name)
