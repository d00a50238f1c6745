"""The packed operand format of option pack7, restated in numpy (tests/pack7_ref.py): pack → unpack returns the bit patterns it was given,
and eligibility is what DESIGN.md §3 says, at the edges of the format."""
import numpy as np
import pytest

import pack7_ref as P


def bits(a):
    return np.asarray(a, dtype=np.float64).view(np.uint64)


def round_trip(v, bounds):
    v = np.asarray(v, dtype=np.float64)
    packed, e0 = P.pack(v, bounds)
    assert packed.size == P.RECORD * ((len(v) + 15) // 16)
    assert np.array_equal(e0, P.eligibility(v, bounds))
    u = P.unpack(packed, e0, bounds, v)
    assert np.array_equal(bits(u), bits(v))
    # a packed block really comes out of the records: decoding against a scrambled source gives the same entries
    junk = np.full(len(v), np.nan)
    w = P.unpack(packed, e0, bounds, junk)
    for q in range(len(bounds) - 1):
        if e0[q] >= 0:
            assert np.array_equal(bits(w[bounds[q]:bounds[q + 1]]), bits(v[bounds[q]:bounds[q + 1]]))
    return e0


def mantissas(rng, n):
    """doubles in [1, 2) with every mantissa bit in play"""
    m = rng.integers(0, 1 << 52, n, dtype=np.uint64)
    return (m | (np.uint64(1023) << np.uint64(52))).view(np.float64)


def test_exactly_eight_binades_is_eligible_nine_is_not():
    rng = np.random.default_rng(1)
    m = 0.25                                                               # binades are counted on the exponent field: the smallest value opens one
    v = m * np.ldexp(mantissas(rng, 300), rng.integers(0, 8, 300))       # min·1 … just under min·256
    v[0] = m; v[1] = np.nextafter(m * 256, 0)
    assert P.exponents(v).max() - P.exponents(v).min() == 7
    assert round_trip(v, [0, 300])[0] == P.exponents(m)
    v[2] = m * 256                                                         # the ninth binade
    assert round_trip(v, [0, 300])[0] == -1


def test_both_sides_of_two_and_both_signs_in_one_row():
    rng = np.random.default_rng(2)
    v = np.array([1.9999999999999998, 2.0, -2.0000000000000004, -1.5, 3.75, -0.51, 0.5, 1.0])
    assert round_trip(v, [0, 8])[0] == 1022
    w = mantissas(rng, 64) * rng.choice([-1.0, 1.0], 64) * np.ldexp(1.0, rng.integers(0, 3, 64))
    assert round_trip(w, [0, 64])[0] >= 0


@pytest.mark.parametrize("bad", [-0.0, 0.0, 5e-324, 2.2250738585072009e-308, np.inf, -np.inf, np.nan])
def test_values_that_make_a_block_ineligible(bad):
    v = np.array([1.0, 1.5, bad, 1.25] * 5)
    e0 = round_trip(v, [0, 10, 20])
    assert list(e0) == [-1, -1]
    e0 = round_trip(np.r_[np.ones(16), v], [0, 16, 36])                   # its neighbour stays packed
    assert list(e0) == [1023, -1]


def test_smallest_and_largest_exponents():
    rng = np.random.default_rng(3)
    tiny = np.ldexp(mantissas(rng, 40), -1022 + rng.integers(0, 8, 40)); tiny[0] = 2.2250738585072014e-308      # E0 = 1
    assert round_trip(tiny, [0, 40])[0] == 1
    huge = np.ldexp(mantissas(rng, 40), 1023 - rng.integers(0, 8, 40)); huge[0] = 1.7976931348623157e308; huge[1] = np.ldexp(1.0, 1016)
    assert P.exponents(huge).max() == 2046
    assert round_trip(huge, [0, 40])[0] == 2039                                                                    # E0 + 7 = 2046


def test_a_record_shared_by_two_blocks():
    rng = np.random.default_rng(4)
    a = mantissas(rng, 23) * 1e-6          # the first block ends inside record 1
    b = mantissas(rng, 30) * 1e+9 * rng.choice([-1.0, 1.0], 30)
    v = np.r_[a, b]
    e0 = round_trip(v, [0, 23, 53])
    assert e0[0] >= 0 and e0[1] >= 0 and e0[0] != e0[1]
    b[7] = 0.0                              # ... and with one of the two ineligible
    e0 = round_trip(np.r_[a, b], [0, 23, 53])
    assert e0[0] >= 0 and e0[1] == -1
    a[3] = np.inf
    b[7] = 1e9
    e0 = round_trip(np.r_[a, b], [0, 23, 53])
    assert e0[0] == -1 and e0[1] >= 0


def test_slices_off_the_record_grid_and_a_ragged_end():
    rng = np.random.default_rng(5)
    for n, bounds in ((37, [0, 5, 21, 37]), (100, [0, 3, 3, 50, 99, 100]), (16, [0, 16]), (1, [0, 1]), (257, [0, 129, 257])):
        v = mantissas(rng, n) * rng.choice([-1.0, 1.0], n) * np.ldexp(1.0, rng.integers(-2, 3, n))
        e0 = round_trip(v, bounds)
        for q in range(len(bounds) - 1):
            assert (e0[q] >= 0) == (bounds[q + 1] > bounds[q])             # an empty block is not packed


def test_fetch_is_three_reads_at_the_record_offsets():
    """the byte layout itself, spelled out for one entry"""
    v = np.arange(1, 41, dtype=np.float64) * -1.1
    packed, e0 = P.pack(v, [0, 40])
    k = 21
    rec = packed[P.RECORD * (k // 16):P.RECORD * (k // 16 + 1)]
    i = k % 16
    lo = int(rec[4 * i:4 * i + 4].view(np.uint32)[0]); mid = int(rec[64 + 2 * i:64 + 2 * i + 2].view(np.uint16)[0]); b = int(rec[96 + i])
    hi = (b >> 7) << 31 | (int(e0[0]) + ((b >> 4) & 7)) << 20 | (b & 15) << 16 | mid
    assert (hi << 32 | lo) == int(bits(v)[k])


def test_block_bounds_of_a_csr_operand():
    rowptr = np.arange(0, 7 * 601, 7)
    assert list(P.block_bounds(rowptr)) == [0, 7 * 256, 7 * 512, 7 * 600]
    assert list(P.block_bounds(rowptr, nd=True)) == [0, 6 * 256, 6 * 512, 6 * 600]
