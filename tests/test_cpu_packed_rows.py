"""tests/packed_rows.py, the numpy packer / unpacker of the search's bit-packed
feature rows that tests/test_gpu_resnet_packed.py feeds to the fused ResNet:
the round trip on the exact nets' master inputs, and that the comparison sees
each decode error the packed prologue could make (a wrong symmetry, the two
planes of a position swapped, the history shifted by one position)."""

import numpy as np
import pytest

import exact_nets as E
import packed_rows as P

HISTORIES = (1, 4, 8, 15)


def _master(H):
    return E.inputs(1 + 2 * H)


def _mixed_rows(x):
    """Master rows that are neither all zeros nor all ones (rows 1 and 2 are)."""
    flat = x.reshape(len(x), -1)
    return ~((flat == 0).all(1) | (flat == 1).all(1))


@pytest.mark.parametrize("H", HISTORIES)
def test_round_trip_under_every_symmetry(H):
    x = _master(H)
    for t in range(8):
        rows = P.pack(x, t)
        assert rows.shape == (len(x), 2 + 2 * H) and rows.dtype == np.uint64
        assert (rows[:, 1] == 0).all()
        assert P.valid_bits(rows).all() and (P.transforms(rows) == t).all()
        assert np.array_equal(P.unpack(rows, H), x), t
    t = np.arange(len(x)) % 8  # per-row symmetries, as the GPU tests pack them
    assert np.array_equal(P.unpack(P.pack(x, t), H), x)


def test_meta_word_layout():
    """write_feature_meta: bit 0 the player plane, bits 8-10 t, bit 16 valid."""
    x = _master(4)[:16]
    rows = P.pack(x, np.arange(16) % 8)
    for n in range(16):
        assert int(rows[n, 0]) == int(x[n, 0, 0, 0]) | ((n % 8) << 8) | (1 << 16)


def test_symmetry_table_is_the_oracles():
    """Bit 63 - s of word 2+2h / 3+2h is x[1+2h] / x[2+2h] at transform_action(s, t)."""
    import oracle

    x = _master(4)
    n, h = 5, 2
    for t in range(8):
        row = P.pack(x[n:n + 1], t)[0]
        for s in range(64):
            p = oracle.transform_action(s, t)
            assert (int(row[2 + 2 * h]) >> (63 - s)) & 1 == int(x[n, 1 + 2 * h, p // 8, p % 8])
            assert (int(row[3 + 2 * h]) >> (63 - s)) & 1 == int(x[n, 2 + 2 * h, p // 8, p % 8])


@pytest.mark.parametrize("H", HISTORIES)
def test_invalid_rows_are_all_zero_and_decode_to_zero(H):
    x = _master(H)[:9]
    valid = np.arange(9) % 3 != 0
    rows = P.pack(x, 3, valid)
    assert (rows[~valid] == 0).all() and P.valid_bits(rows).tolist() == valid.tolist()
    got = P.unpack(rows, H)
    assert np.array_equal(got[valid], x[valid]) and (got[~valid] == 0).all()


@pytest.mark.parametrize("H", HISTORIES)
def test_a_wrong_symmetry_shows_on_every_mixed_row(H):
    x = _master(H)
    mixed = _mixed_rows(x)
    assert mixed.sum() == len(x) - 2
    for t in range(8):
        rows = P.pack(x, t)
        for other in range(8):
            if other == t:
                continue
            wrong = rows.copy()
            wrong[:, 0] = P.meta(x[:, 0, 0, 0], other)
            differs = (P.unpack(wrong, H) != x).reshape(len(x), -1).any(1)
            assert differs[mixed].all(), (t, other)
            assert not differs[~mixed].any()


@pytest.mark.parametrize("H", HISTORIES)
def test_swapped_planes_of_a_position_show(H):
    x = _master(H)
    mixed = _mixed_rows(x)
    rows = P.pack(x, np.arange(len(x)) % 8)
    for h in range(H):
        wrong = rows.copy()
        wrong[:, [2 + 2 * h, 3 + 2 * h]] = rows[:, [3 + 2 * h, 2 + 2 * h]]
        differs = (P.unpack(wrong, H) != x).reshape(len(x), -1).any(1)
        assert differs[mixed].all(), h


@pytest.mark.parametrize("H", HISTORIES)
def test_a_history_shifted_by_one_position_shows(H):
    """Position h read from position h + 1's words (the last from zeros)."""
    x = _master(H)
    mixed = _mixed_rows(x)
    rows = P.pack(x, np.arange(len(x)) % 8)
    wrong = rows.copy()
    wrong[:, 2:-2] = rows[:, 4:]
    wrong[:, -2:] = 0
    differs = (P.unpack(wrong, H) != x).reshape(len(x), -1).any(1)
    assert differs[mixed].all()


def test_pack_rejects_what_a_row_cannot_hold():
    x = np.array(_master(4)[:2])
    x[0, 0, 3, 3] = 1.0 - x[0, 0, 0, 0]
    with pytest.raises(AssertionError, match="constant"):
        P.pack(x, 0)
    with pytest.raises(AssertionError):
        P.pack(_master(4)[:2], 8)
