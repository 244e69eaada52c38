"""The search's bit-packed feature rows (csrc/tree_search.h write_feature_meta /
flush_ancestors), written and read back in numpy: what the packed prologue of
the fused ResNet (csrc/resnet.hip, IN == kPacked) decodes.

A row of history H is 2 + 2H uint64 words:
  word 0      meta: bit 0 = plane 0 (constant per board), bits 8-10 = the
              board symmetry t, bit 16 = valid
  word 1      0
  word 2+2h   plane 1+2h, word 3+2h plane 2+2h of position h, untransformed:
              bit 63 - s is square s
The decode gives plane c at square p the bit of square inverse_transform(p, t),
i.e. the stored square s shows at p = transform_action(s, t). An invalid row
(a terminal leaf) is all zeros and decodes to an all-zero board.

The symmetry table is the oracle's transform_action (oracle/oracle.py, pinned
against the reference by tests/test_oracle_golden.py); no table of its own.
"""

from __future__ import annotations

import functools

import numpy as np

META_PLAYER = np.uint64(1)
META_T_SHIFT = np.uint64(8)
META_VALID = np.uint64(1 << 16)


@functools.lru_cache(maxsize=None)
def _tables():
    """forward[t, s] = transform_action(s, t); inverse[t, forward[t, s]] = s."""
    import oracle

    fwd = np.array([[oracle.transform_action(s, t) for s in range(64)] for t in range(8)], dtype=np.int64)
    inv = np.empty_like(fwd)
    for t in range(8):
        assert sorted(fwd[t]) == list(range(64))
        inv[t, fwd[t]] = np.arange(64)
    return fwd, inv


def feature_words(H: int) -> int:
    return 2 + 2 * H


def meta(player_plane, t, valid=True) -> np.ndarray:
    """Meta words of valid rows (0 where valid is False)."""
    m = (np.asarray(player_plane, np.uint64) & META_PLAYER) | (np.asarray(t, np.uint64) << META_T_SHIFT) | META_VALID
    return np.where(np.asarray(valid, bool), m, np.uint64(0))


def pack(x: np.ndarray, t, valid=True) -> np.ndarray:
    """(N, 1+2H, 8, 8) 0/1 planes -> (N, 2+2H) uint64 rows whose decode under
    the per-row symmetry t (0..7) is x; rows with valid False are all zeros."""
    x = np.asarray(x)
    N, C = x.shape[:2]
    assert C % 2 == 1 and C >= 3 and x.shape[2:] == (8, 8), x.shape
    assert np.isin(x, (0, 1)).all()
    H = (C - 1) // 2
    flat = x.reshape(N, C, 64).astype(np.uint64)
    assert (flat[:, 0] == flat[:, 0, :1]).all(), "plane 0 must be constant per board"
    t = np.broadcast_to(np.asarray(t, np.int64), (N,))
    assert ((0 <= t) & (t < 8)).all()
    valid = np.broadcast_to(np.asarray(valid, bool), (N,))
    fwd, _ = _tables()
    # stored[n, c, s] = x[n, c, transform_action(s, t[n])]
    stored = np.take_along_axis(flat, np.broadcast_to(fwd[t][:, None, :], (N, C, 64)), axis=2)
    weights = np.uint64(1) << (np.uint64(63) - np.arange(64, dtype=np.uint64))
    rows = np.zeros((N, feature_words(H)), np.uint64)
    rows[:, 0] = meta(flat[:, 0, 0], t)
    rows[:, 2:] = (stored[:, 1:] * weights).sum(axis=2, dtype=np.uint64)
    rows[~valid] = 0
    return rows


def valid_bits(rows: np.ndarray) -> np.ndarray:
    return (np.asarray(rows, np.uint64)[:, 0] & META_VALID) != 0


def transforms(rows: np.ndarray) -> np.ndarray:
    return ((np.asarray(rows, np.uint64)[:, 0] >> META_T_SHIFT) & np.uint64(7)).astype(np.int64)


def unpack(rows: np.ndarray, H: int) -> np.ndarray:
    """(N, 2+2H) uint64 rows -> (N, 1+2H, 8, 8) float32 planes: k_features_f32 /
    plane_value of csrc/tree.hip restated (an invalid row gives zeros)."""
    rows = np.asarray(rows, np.uint64)
    N = rows.shape[0]
    assert rows.shape == (N, feature_words(H)), rows.shape
    C = 1 + 2 * H
    _, inv = _tables()
    src = inv[transforms(rows)]  # (N, 64): the stored square shown at p
    shift = (np.uint64(63) - src.astype(np.uint64))[:, None, :]
    out = np.empty((N, C, 64), np.float32)
    out[:, 0] = (rows[:, 0] & META_PLAYER).astype(np.float32)[:, None]
    out[:, 1:] = ((rows[:, 2:, None] >> shift) & np.uint64(1)).astype(np.float32)
    out[~valid_bits(rows)] = 0.0
    return out.reshape(N, C, 8, 8)
