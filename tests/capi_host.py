"""A foreign host of liboamd.so: a ctypes binding of include/othello_mcts_amd.h
written from the header alone, and the two host loops over the step API that
INTEGRATION.md §3 describes.

The product's own Python layer reaches the C ABI through pybind_module.cpp.
This module is what an outside maintainer would write instead: it never
imports othello_mcts (nor its extension module), loads the library by path,
and uses torch only to own device memory and to copy it (tensor.data_ptr()
passed as a pointer). tests/test_cpu_capi.py pins the structures and
prototypes below against the header and INTEGRATION.md; tests/test_gpu_capi.py
runs everything through them on the device.

Two hosts:
  search_dense   INTEGRATION.md §3's loop: every row goes to the evaluator.
  search_sparse  the host the header permits: only rows whose leaf flag is set
                 are read and evaluated, run by run (row_begin != 0, partial
                 ranges); every other row holds a poison that a kernel which
                 wrongly read it would carry into its visit counts and Q.

Evaluators run on the host (features copied back, a numpy stub, answers copied
up): the oracle's results are bit-exact only against the same stub arithmetic.
"""

from __future__ import annotations

import ctypes
from pathlib import Path
from typing import Callable, NamedTuple

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
HEADER = ROOT / "include" / "othello_mcts_amd.h"
LIB_PATH = ROOT / "othello-alphazero_amd" / "othello_mcts" / "liboamd.so"

OAMD_OK, OAMD_INVALID_ARGUMENT, OAMD_OUT_OF_RANGE, OAMD_RUNTIME, OAMD_CAPACITY = range(5)
OAMD_BF16, OAMD_FP16 = 0, 1
DTYPES = {"bf16": OAMD_BF16, "fp16": OAMD_FP16}


# ----------------------------------------------------------------- structures
class Position(ctypes.Structure):  # oamd_position
    _fields_ = [("player", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("player1_discs", ctypes.c_uint64), ("player2_discs", ctypes.c_uint64),
                ("legal_moves", ctypes.c_uint64), ("next_legal_moves", ctypes.c_uint64)]

    def tuple(self):
        return (self.player, self.player1_discs, self.player2_discs, self.legal_moves, self.next_legal_moves)


class SearchConfig(ctypes.Structure):
    _fields_ = [("history_size", ctypes.c_int32), ("num_simulations", ctypes.c_int32),
                ("num_threads", ctypes.c_int32), ("batch_size", ctypes.c_int32),
                ("c_puct_base", ctypes.c_float), ("c_puct_init", ctypes.c_float),
                ("dirichlet_epsilon", ctypes.c_float), ("dirichlet_alpha", ctypes.c_float)]


class RootInfo(ctypes.Structure):  # oamd_root_info
    _fields_ = [("position", Position), ("num_children", ctypes.c_int32), ("visit_count", ctypes.c_int32),
                ("overflow", ctypes.c_int32), ("reserved", ctypes.c_int32), ("node_count", ctypes.c_int64)]


class NetDesc(ctypes.Structure):  # oamd_net_desc
    _fields_ = [("in_channels", ctypes.c_int32), ("conv_channels", ctypes.c_int32),
                ("num_residual_blocks", ctypes.c_int32), ("value_head_hidden_channels", ctypes.c_int32),
                ("num_squares", ctypes.c_int32), ("num_actions", ctypes.c_int32), ("dtype", ctypes.c_int32)]


class SelfplayConfig(ctypes.Structure):  # oamd_selfplay_config
    _fields_ = [("temperature_moves", ctypes.c_int32), ("temperature", ctypes.c_float),
                ("opening_moves", ctypes.c_int32), ("emit_targets", ctypes.c_int32)]


# header struct name -> its ctypes class
STRUCTS = {"oamd_position": Position, "oamd_search_config": SearchConfig, "oamd_root_info": RootInfo,
           "oamd_net_desc": NetDesc, "oamd_selfplay_config": SelfplayConfig}


# ----------------------------------------------------------------- prototypes
class OamdRuntimeError(RuntimeError):
    pass


def _check(rc, func, args):
    """errcheck of every entry point that returns an oamd_status."""
    if rc:
        msg = _lib.oamd_last_error().decode()
        raise {OAMD_INVALID_ARGUMENT: ValueError, OAMD_OUT_OF_RANGE: IndexError}.get(rc, OamdRuntimeError)(msg)
    return rc


_i32, _i64, _u64, _vp = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint64, ctypes.c_void_p
_P = ctypes.POINTER
STATUS = "oamd_status"  # int return value checked by _check

# name -> (restype, argtypes). Handles (oamd_engine *, oamd_net *), device
# pointers and streams are c_void_p; nothing is left to ctypes' default int.
PROTOTYPES = {
    "oamd_last_error": (ctypes.c_char_p, []),
    "oamd_abi_version": (ctypes.c_int, []),
    "oamd_device_count": (STATUS, [_P(_i32)]),
    "oamd_get_legal_moves": (STATUS, [_vp, _vp, _vp, _i64, _vp]),
    "oamd_get_flips": (STATUS, [_vp, _vp, _vp, _vp, _i64, _vp]),
    "oamd_apply_action": (STATUS, [_vp, _vp, _vp, _i64, _vp]),
    "oamd_initial_position": (STATUS, [_P(Position)]),
    "oamd_net_create": (STATUS, [_i32, _P(NetDesc), _P(_vp)]),
    "oamd_net_destroy": (STATUS, [_vp]),
    "oamd_net_state_size": (STATUS, [_vp, _P(_i32)]),
    "oamd_net_state_key": (STATUS, [_vp, _i32, _P(ctypes.c_char_p), _P(_i64)]),
    "oamd_net_load_state": (STATUS, [_vp, _P(_P(ctypes.c_float)), _i32]),
    "oamd_net_forward": (STATUS, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "oamd_engine_create": (STATUS, [_i32, _i32, _i64, _P(SearchConfig), _u64, _P(_vp)]),
    "oamd_engine_destroy": (STATUS, [_vp]),
    "oamd_engine_get_config": (STATUS, [_vp, _P(SearchConfig)]),
    "oamd_engine_num_games": (STATUS, [_vp, _P(_i32)]),
    "oamd_engine_set_stream": (STATUS, [_vp, _vp]),
    "oamd_engine_search": (STATUS, [_vp, _vp, _P(_i64), _P(_i64)]),
    "oamd_engine_work_counters": (STATUS, [_vp, _P(_i64), _P(_i64)]),
    "oamd_engine_search_begin": (STATUS, [_vp, _P(_i32)]),
    "oamd_engine_select": (STATUS, [_vp]),
    "oamd_engine_leaf_flags": (STATUS, [_vp, _P(ctypes.c_uint8)]),
    "oamd_engine_features": (STATUS, [_vp, _vp, _i32, _i32]),
    "oamd_engine_set_evaluation": (STATUS, [_vp, _vp, _vp, _i32, _i32]),
    "oamd_engine_backup": (STATUS, [_vp]),
    "oamd_engine_root_info": (STATUS, [_vp, _i32, _P(RootInfo), _P(_i32), _P(ctypes.c_float)]),
    "oamd_engine_status": (STATUS, [_vp, _P(_i32), _P(_i32)]),
    "oamd_engine_self_play_data": (STATUS, [_vp, _i32, _P(ctypes.c_float), _P(ctypes.c_float)]),
    "oamd_engine_apply_action": (STATUS, [_vp, _i32, _i32]),
    "oamd_engine_game_key": (STATUS, [_vp, _i32, _P(_u64)]),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = ctypes.CDLL(str(LIB_PATH))
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(L, name)
            fn.argtypes = args
            if res == STATUS:
                fn.restype = ctypes.c_int
                fn.errcheck = _check
            else:
                fn.restype = res
        _lib = L
    return _lib


def device_count() -> int:
    n = _i32(-1)
    lib().oamd_device_count(ctypes.byref(n))
    return n.value


def current_stream(device: torch.device) -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _fp(a: np.ndarray):
    return a.ctypes.data_as(_P(ctypes.c_float))


# --------------------------------------------------------------------- engine
class Engine:
    """G games of one oamd_engine. Rows of the step API: row = game * L + leaf,
    L = num_threads * batch_size."""

    def __init__(self, num_games: int, config: SearchConfig, seed: int, node_capacity: int = 0, device: int = 0):
        self.h = ctypes.c_void_p()
        lib().oamd_engine_create(device, num_games, node_capacity, ctypes.byref(config), seed, ctypes.byref(self.h))
        self.device = torch.device("cuda", device)
        got, n = SearchConfig(), _i32()
        _lib.oamd_engine_get_config(self.h, ctypes.byref(got))
        _lib.oamd_engine_num_games(self.h, ctypes.byref(n))
        self.config, self.G = got, n.value
        self.L = got.num_threads * got.batch_size
        self.C = 1 + 2 * got.history_size
        self.rows = self.G * self.L
        self.set_stream()

    def set_stream(self) -> None:
        """The engine works on torch's current stream, so its kernels and
        torch's copies of the buffers it is handed are ordered."""
        _lib.oamd_engine_set_stream(self.h, current_stream(self.device))

    def destroy(self) -> None:
        if self.h:
            _lib.oamd_engine_destroy(self.h)
            self.h = ctypes.c_void_p()

    def search_begin(self) -> int:
        steps = _i32()
        _lib.oamd_engine_search_begin(self.h, ctypes.byref(steps))
        return steps.value

    def select(self) -> None:
        _lib.oamd_engine_select(self.h)

    def leaf_flags(self) -> np.ndarray:
        out = np.zeros(self.rows, np.uint8)
        _lib.oamd_engine_leaf_flags(self.h, out.ctypes.data_as(_P(ctypes.c_uint8)))
        return out

    def features(self, dev_ptr: int, row_begin: int, rows: int) -> None:
        _lib.oamd_engine_features(self.h, dev_ptr, row_begin, rows)

    def set_evaluation(self, policy_ptr: int, value_ptr: int, row_begin: int, rows: int) -> None:
        _lib.oamd_engine_set_evaluation(self.h, policy_ptr, value_ptr, row_begin, rows)

    def backup(self) -> None:
        _lib.oamd_engine_backup(self.h)

    def status(self) -> tuple:
        over, capped = _i32(-1), _i32(-1)
        _lib.oamd_engine_status(self.h, ctypes.byref(over), ctypes.byref(capped))
        return over.value, capped.value

    def root_info(self, game: int) -> dict:
        info, visits, q = RootInfo(), (_i32 * 65)(), (ctypes.c_float * 65)()
        _lib.oamd_engine_root_info(self.h, game, ctypes.byref(info), visits, q)
        n = info.num_children
        return {"position": info.position.tuple(), "num_children": n, "visit_count": info.visit_count,
                "overflow": info.overflow, "node_count": info.node_count, "visits": list(visits[:n]),
                "q": np.array(q[:n], np.float32)}

    def self_play_data(self, game: int):
        f = np.zeros((8, self.C, 8, 8), np.float32)
        p = np.zeros((8, 65), np.float32)
        _lib.oamd_engine_self_play_data(self.h, game, _fp(f), _fp(p))
        return f, p

    def apply_action(self, game: int, action: int) -> None:
        _lib.oamd_engine_apply_action(self.h, game, action)

    def game_key(self, game: int) -> int:
        key = _u64()
        _lib.oamd_engine_game_key(self.h, game, ctypes.byref(key))
        return key.value

    def work_counters(self) -> tuple:
        sims, evals = _i64(-1), _i64(-1)
        _lib.oamd_engine_work_counters(self.h, ctypes.byref(sims), ctypes.byref(evals))
        return sims.value, evals.value

    def search(self, net: "Net") -> tuple:
        """The whole search with the native net; waits. (simulations, evaluations)."""
        sims, evals = _i64(-1), _i64(-1)
        _lib.oamd_engine_search(self.h, net.h, ctypes.byref(sims), ctypes.byref(evals))
        return sims.value, evals.value


# ------------------------------------------------------------------------ net
class Net:
    """oamd_net: `state` maps AlphaZeroNet.state_dict() keys to fp32 arrays."""

    def __init__(self, desc: NetDesc, device: int = 0):
        self.h = ctypes.c_void_p()
        lib().oamd_net_create(device, ctypes.byref(desc), ctypes.byref(self.h))
        self.device = torch.device("cuda", device)

    def destroy(self) -> None:
        if self.h:
            _lib.oamd_net_destroy(self.h)
            self.h = ctypes.c_void_p()

    def state_keys(self) -> list:
        n = _i32()
        _lib.oamd_net_state_size(self.h, ctypes.byref(n))
        out = []
        for i in range(n.value):
            key, numel = ctypes.c_char_p(), _i64()
            _lib.oamd_net_state_key(self.h, i, ctypes.byref(key), ctypes.byref(numel))
            out.append((key.value.decode(), numel.value))
        return out

    def load_state(self, state: dict) -> None:
        keys = self.state_keys()
        arrs = [np.ascontiguousarray(np.asarray(state[k], np.float32)).reshape(-1) for k, _ in keys]
        for (k, numel), a in zip(keys, arrs):
            if a.size != numel:
                raise ValueError(f"{k}: expected {numel} elements, got {a.size}")
        ptrs = (_P(ctypes.c_float) * len(arrs))(*[_fp(a) for a in arrs])
        _lib.oamd_net_load_state(self.h, ptrs, len(arrs))

    def forward(self, features_ptr: int, rows: int, policy_ptr: int, value_ptr: int) -> None:
        _lib.oamd_net_forward(self.h, features_ptr, rows, policy_ptr, value_ptr, current_stream(self.device))


# ----------------------------------------------------------------- host loops
Stub = Callable[[np.ndarray], tuple]


def evaluate_on_host(stub: Stub, features_dev: torch.Tensor):
    """features (n, C, 8, 8) on the device -> (policy (n, 65), value (n,)) on
    the device, computed by the numpy stub on the CPU."""
    p, v = stub(features_dev.cpu().numpy())
    dev = features_dev.device
    pol = torch.from_numpy(np.ascontiguousarray(p, np.float32)).to(dev)
    val = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev)
    return pol, val


def raise_on_status(engine: Engine) -> None:
    over, capped = engine.status()
    if over or capped:
        raise OamdRuntimeError(f"search diverged: {over} game(s) out of nodes, {capped} at the depth cap")


def search_dense(engine: Engine, stub: Stub) -> None:
    """INTEGRATION.md §3's loop: all G * L rows go to the evaluator every step."""
    engine.set_stream()
    rows = engine.rows
    feat = torch.empty((rows, engine.C, 8, 8), dtype=torch.float32, device=engine.device)
    steps = engine.search_begin()
    for _ in range(steps):
        engine.select()  # backs up the previous round thread by thread, then selects
        engine.features(feat.data_ptr(), 0, rows)
        pol, val = evaluate_on_host(stub, feat)
        engine.set_evaluation(pol.data_ptr(), val.data_ptr(), 0, rows)
    engine.backup()  # the last round
    raise_on_status(engine)


def make_poison(engine: Engine):
    """What search_sparse leaves in every row it does not evaluate: finite and
    in range (a one-hot policy on the pass action, values +1 / -1 by row), so a
    kernel that reads such a row goes wrong in its numbers, not its addresses."""
    pol = torch.zeros((engine.rows, 65), dtype=torch.float32)
    pol[:, 64] = 1.0
    val = torch.ones(engine.rows, dtype=torch.float32)
    val[1::2] = -1.0
    return pol.to(engine.device), val.to(engine.device)


def flagged_runs(flags: np.ndarray) -> list:
    """[(row_begin, rows)] of the maximal runs of consecutive nonzero flags."""
    runs, r, n = [], 0, len(flags)
    while r < n:
        if not flags[r]:
            r += 1
            continue
        r0 = r
        while r < n and flags[r]:
            r += 1
        runs.append((r0, r - r0))
    return runs


class SparseStep(NamedTuple):
    flags: np.ndarray      # (G * L,) uint8, oamd_engine_leaf_flags of the step
    features: np.ndarray   # (flagged rows, C, 8, 8): what the evaluator saw, rows ascending
    runs: list             # [(row_begin, rows)] of the features / set_evaluation calls


def search_sparse(engine: Engine, stub: Stub, poison) -> list:
    """The host the header permits: per step only the rows whose leaf flag is
    set are read and evaluated, one features / set_evaluation pair per maximal
    run of flagged rows; before that, one full-range set_evaluation hands every
    row the poison. Returns one SparseStep per step."""
    engine.set_stream()
    poison_policy, poison_value = poison
    C = engine.C
    feat = torch.empty((engine.rows, C, 8, 8), dtype=torch.float32, device=engine.device)
    out = []
    steps = engine.search_begin()
    for _ in range(steps):
        engine.select()
        flags = engine.leaf_flags()
        runs = flagged_runs(flags)
        seen = []
        engine.set_evaluation(poison_policy.data_ptr(), poison_value.data_ptr(), 0, engine.rows)
        for r0, n in runs:
            chunk = feat[:n]
            engine.features(chunk.data_ptr(), r0, n)
            pol, val = evaluate_on_host(stub, chunk)
            engine.set_evaluation(pol.data_ptr(), val.data_ptr(), r0, n)
            seen.append(chunk.cpu().numpy())
        out.append(SparseStep(flags, np.concatenate(seen) if seen else np.zeros((0, C, 8, 8), np.float32), runs))
    engine.backup()
    raise_on_status(engine)
    return out


# ---------------------------------------- shared by test_cpu_capi / test_gpu_capi
# The two whole-game configurations of the sparse-host test (G = 3 games of one
# engine, seed 17). B: num_simulations is no multiple of L = 24 and a step has
# 72 rows, so flagged runs cross thread and game boundaries.
WHOLE_GAME_SEED, WHOLE_GAME_GAMES = 17, 3
WHOLE_GAMES = {
    "A": dict(history_size=3, num_simulations=96, num_threads=2, batch_size=8, dirichlet_epsilon=0.25),
    "B": dict(history_size=3, num_simulations=100, num_threads=3, batch_size=8, dirichlet_epsilon=0.25),
}
# Per game, over its searches: searches in which fewer than T * steps batches
# went to the NN, and NN batches that held a terminal leaf (an all-zero row).
# Floors on the inputs (the sparse test must not pass vacuously), not tolerances.
SKIPPED_SEARCHES_FLOOR, ZERO_ROW_CALLS_FLOOR = 3, 10


def search_steps(cfg: dict) -> int:
    L = cfg["num_threads"] * cfg["batch_size"]
    return (cfg["num_simulations"] + L - 1) // L


class EvaluatorTap:
    """Wraps a stub and keeps what one OracleMCTS handed it: calls[i] is the
    (B, C, 8, 8) feature batch of the i-th NN call since the last clear()."""

    def __init__(self, stub: Stub):
        self.stub = stub
        self.calls: list = []

    def __call__(self, features: np.ndarray):
        self.calls.append(np.array(features, np.float32))
        return self.stub(features)

    def clear(self) -> None:
        self.calls = []

    def zero_row_calls(self) -> int:
        return sum(1 for f in self.calls if (~f.reshape(f.shape[0], -1).any(axis=1)).any())

    def nonzero_rows(self, C: int) -> np.ndarray:
        rows = [f[f.reshape(f.shape[0], -1).any(axis=1)] for f in self.calls]
        return np.concatenate(rows) if rows else np.zeros((0, C, 8, 8), np.float32)
