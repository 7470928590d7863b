"""The first column of the maximum on ONE packed register (uc_sw_pk_impl.hpp:do_step, MODE 0 / 2): an integer model of the three-instruction update

    d    = pk_sub_sat(colmax, best)        non-zero in a half  <=>  colmax > best there
    nm   = pk_sub_sat(0x00010001, d)       1 where not improved, 0 where improved
    age2 = v_pk_mad_u16(age2, nm, nm)      (age + 1) where not improved, 0 where improved, mod 2^16
    best = pk_max(best, colmax)

against the compare / select form it replaces (col = colmax > best ? st - g : col), on packed 32-bit words, half by half, and of finish_slot's
reconstruction col = ((nst - 1 - g) - age) & 0xffff.  CPU only."""
import numpy as np
import pytest

BIAS = 128


def pk(lo, hi):
    return [(int(a) & 0xffff) | (int(b) << 16) for a, b in zip(lo, hi)]


def pk_sub_sat(a, b):
    return max((a & 0xffff) - (b & 0xffff), 0) | (max((a >> 16) - (b >> 16), 0) << 16)


def pk_max(a, b):
    return max(a & 0xffff, b & 0xffff) | (max(a >> 16, b >> 16) << 16)


def pk_mad(a, b, c):
    return (((a & 0xffff) * (b & 0xffff) + (c & 0xffff)) & 0xffff) | ((((a >> 16) * (b >> 16) + (c >> 16)) & 0xffff) << 16)


def run_packed(colmax):
    """colmax [steps] packed words of one lane -> (best, age2) after the last step"""
    best, age = BIAS * 0x10001, 0
    for cm in colmax:
        d = pk_sub_sat(cm, best)
        nm = pk_sub_sat(0x00010001, d)
        assert nm in (0, 1, 0x10000, 0x10001)
        age = pk_mad(age, nm, nm)
        best = pk_max(best, cm)
    return best, age


def run_select(colmax):
    """the form it replaces: an unpacking compare and a select per half and step -> (best, step of the first maximum) per half"""
    best, first = [BIAS, BIAS], [None, None]
    for st, cm in enumerate(colmax):
        for h, v in enumerate((cm & 0xffff, cm >> 16)):
            if v > best[h]:
                first[h], best[h] = st, v
    return best, first


def same(colmax, lanes=(0,)):
    """both forms on one stream; the column finish_slot rebuilds for each lane g of `lanes` -> the step of the first maximum per half"""
    nst = len(colmax)
    b, age = run_packed(colmax)
    rb, first = run_select(colmax)
    assert [b & 0xffff, b >> 16] == rb
    for h, a in enumerate((age & 0xffff, age >> 16)):
        if first[h] is None:                  # a half that never improved holds no column (its score is the bias: te = -1 goes out)
            continue
        for g in lanes:
            assert ((nst - 1 - g) - a) & 0xffff == (first[h] - g) & 0xffff, (h, g, a, first[h])
    return first


@pytest.mark.parametrize("seed", range(8))
def test_random_streams(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 400))
    # a random walk per half over the biased range, NaN patterns (>= 0x7C00: an overflowed pair) included in the odd seeds
    top = 0x8000 if seed % 2 else 600
    lo = np.clip(BIAS + np.cumsum(rng.integers(-40, 44, n)), BIAS, top - 1)
    hi = np.clip(BIAS + np.cumsum(rng.integers(-40, 44, n)), BIAS, top - 1)
    same(pk(lo, hi), (0, 1, 15, 63))


def test_equal_maxima_recur_and_the_first_stays():
    lo = [BIAS, 200, 150, 200, 200, BIAS, 200]
    hi = [BIAS, BIAS, 300, 300, 128, 300, 299]
    assert same(pk(lo, hi)) == [1, 2]


def test_improvement_by_exactly_one():
    lo = [BIAS + 5, BIAS + 6, BIAS + 6, BIAS + 7, BIAS + 7]
    hi = [BIAS + 1, BIAS + 1, BIAS + 1, BIAS + 1, BIAS + 2]
    assert same(pk(lo, hi)) == [3, 4]


def test_improvement_in_the_last_step_and_none_at_all():
    n = 50
    lo = np.full(n, BIAS); lo[-1] = BIAS + 1
    hi = np.full(n, BIAS)
    assert same(pk(lo, hi)) == [n - 1, None]
    # a half below the bias never improves either (colmax starts from 0 in lanes that hold PAD rows only)
    assert same(pk(np.zeros(n), np.full(n, BIAS)), (3,)) == [None, None]


def test_one_half_does_not_disturb_the_other():
    n = 300
    lo = np.full(n, BIAS); lo[7] = 0x7FFF          # the largest pattern a register holds, in the low half only
    hi = np.full(n, BIAS); hi[200] = BIAS + 1
    assert same(pk(lo, hi)) == [7, 200]
    assert same(pk(hi, lo)) == [200, 7]


def test_age_wraps():
    """65,600 steps: the age of an early improvement passes 2^16, and so does nst; the column is exact all the same"""
    n = 65600
    lo = np.full(n, BIAS); lo[10] = 500
    hi = np.full(n, BIAS); hi[40] = 300; hi[65590] = 301
    assert same(pk(lo, hi), (0, 9, 10, 63)) == [10, 65590]


def test_reconstruction_for_every_lane():
    """finish_slot: col = ((nst - 1 - g) - age) & 0xffff for g < 64, nst below and above 2^16, the improvement at the lane's first and last column"""
    for nst in (66, 70, 32769 + 64 - 1, 65598):
        for g in range(64):
            for st in sorted({g, g + 1, min(g + 65534, nst - 1)}):          # lane g holds column st - g <= 65,534 in step st
                age = (nst - 1 - st) & 0xffff
                assert ((nst - 1 - g) - age) & 0xffff == st - g
                assert 0 <= st - g <= 65534
