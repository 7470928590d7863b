"""Integer model of the packed gapped-DP recurrence in its two score domains (uc_sw_pk_impl.hpp:do_step), cell by cell on the CPU.

  unbiased (MODE 7, and every mode before the biased domain):  x = sat_sub(sat_add(Hdiag, ub), 128); h = max(x, e, f); t = sat_sub(h, open);
      E' = max(sat_sub(e, ext), t); f' = max(sat_sub(f, ext), t)                       - all per 16-bit half, H/E/F floored at 0
  biased (+128 on H and E):  x' = diag' + ub + 0xFF7FFF80 as ONE 32-bit add on the packed register; h' = max3(x', e', f');
      t' = sat_sub(h', open); E' = max3(sat_sub(e', ext), t', 0x0080); f' = max(sat_sub(f', ext), t'); lane 0 receives 0x0080 for H and 0 for F

with ub = s + 128 the profile byte sum.  The model keeps the two alignments of a register in one Python integer, so that a carry or borrow across
the halves would show: H' - 128 == H and E' - 128 == E in every cell of both halves, every packed sum stays below 2^32 and every half of x' in
[0, 65535].  The f16 maximum is modelled as what tools/ubench/pk_max3_f16.hip establishes on the device: an unsigned maximum over the patterns
below 0x7C00, patterns from 0x8000 on (negative numbers) losing against any positive one; no value of this test reaches 0x7C00."""
import numpy as np
import pytest

BIAS = 0x00800080
UNBIAS = 0xFF7FFF80          # -128 in either half as one 32-bit addend: 2^32 - BIAS


def _halves(v):
    return v & 0xFFFF, v >> 16


def _pack(lo, hi):
    assert 0 <= lo < 65536 and 0 <= hi < 65536
    return lo | (hi << 16)


def _pk(fn, a, b):
    return _pack(fn(a & 0xFFFF, b & 0xFFFF), fn(a >> 16, b >> 16))


def _sat_sub(a, b): return _pk(lambda x, y: max(x - y, 0), a, b)
def _sat_add(a, b): return _pk(lambda x, y: min(x + y, 65535), a, b)
def _max_u16(a, b): return _pk(max, a, b)


def _f16_key(x):
    assert x < 0x7C00 or x >= 0x8000, "the model covers no infinity / NaN pattern"
    assert x < 0xFC00
    return x if x < 0x8000 else -(x - 0x8000) - 0.5      # negative numbers (and -0) below every positive pattern


def _max3_f16(a, b, c):
    def one(x, y, z):
        return max((x, y, z), key=_f16_key)
    return _pack(one(a & 0xFFFF, b & 0xFFFF, c & 0xFFFF), one(a >> 16, b >> 16, c >> 16))


def _reference(sc, open_, ext):
    """plain local affine-gap DP on signed integers: H and E of every cell (E = the gap state ENTERING the next column, as the kernel keeps it)"""
    n, m = sc.shape
    H = np.zeros((n + 1, m + 1), np.int64)
    Eo = np.zeros((n, m), np.int64)
    E = np.zeros(n + 1, np.int64)
    for j in range(m):
        F = 0
        for i in range(n):
            h = max(0, H[i, j] + sc[i, j], E[i + 1], F)
            H[i + 1, j + 1] = h
            E[i + 1] = max(E[i + 1] - ext, h - open_, 0)
            F = max(F - ext, h - open_, 0)
            Eo[i, j] = E[i + 1]
    return H[1:, 1:], Eo


def _packed(scA, scB, open_, ext, biased):
    """both alignments of a register (A low, B high), column by column as a lane computes its rows"""
    n, m = scA.shape
    hb = BIAS if biased else 0
    open2, ext2 = open_ * 0x10001, ext * 0x10001
    Hprev = [hb] * n                     # the previous column
    E = [hb] * n
    Hout = np.zeros((2, n, m), np.int64)
    Eout = np.zeros((2, n, m), np.int64)
    for j in range(m):
        diag = hb                        # Hup of the previous step: the boundary above row 0
        f = 0
        for i in range(n):
            ub = _pack(int(scA[i, j]) + 128, int(scB[i, j]) + 128)
            if biased:
                s = diag + ub + UNBIAS
                assert s >> 32 == 1, "the packed sum leaves the register by exactly the one carry of the two's-complement constant"
                x = s & 0xFFFFFFFF
                lo, hi = _halves(x)
                dl, dh = _halves(diag)
                assert lo == dl + int(scA[i, j]) and hi == dh + int(scB[i, j]), "a half took a carry or a borrow from its neighbour"
            else:
                x = _sat_sub(_sat_add(diag, ub), BIAS)
            e = E[i]
            h = _max3_f16(x, e, f)
            diag = Hprev[i]
            Hprev[i] = h
            t = _sat_sub(h, open2)
            esub, fsub = _sat_sub(e, ext2), _sat_sub(f, ext2)
            E[i] = _max3_f16(esub, t, BIAS) if biased else _max_u16(esub, t)
            f = _max_u16(fsub, t)
            for half, (hv, ev) in enumerate(zip(_halves(h), _halves(E[i]))):
                Hout[half, i, j] = hv - (128 if biased else 0)
                Eout[half, i, j] = ev - (128 if biased else 0)
    return Hout, Eout


def _case(rng, open_, ext):
    """two 21-letter matrices at the +-48-per-track limit (entry sums in [-96, 96], the extremes present), one query against two targets"""
    S3 = rng.integers(-48, 49, (21, 21)); SA = rng.integers(-48, 49, (21, 21))
    S3[0, 0] = SA[0, 0] = 48; S3[1, 2] = SA[1, 2] = -48
    n, m = int(rng.integers(1, 15)), int(rng.integers(1, 19))
    mode = rng.integers(0, 3)
    lo = (0, 0, 1)[mode]; hi = (21, 3, 3)[mode]          # all letters; few letters (long high-scoring runs); the -96 pair only
    q3, qa = rng.integers(lo, hi, n), rng.integers(lo, hi, n)
    out = []
    for _ in range(2):
        t3, ta = rng.integers(lo, hi, m), rng.integers(lo, hi, m)
        if mode == 1:
            t3[: min(n, m)] = q3[: min(n, m)]; ta[: min(n, m)] = qa[: min(n, m)]
        out.append(S3[q3][:, t3] + SA[qa][:, ta])
    return out


@pytest.mark.parametrize("open_", [0, 1, 10, 31])
@pytest.mark.parametrize("ext", [0, 1, 3])
def test_both_recurrences_equal_the_reference_in_every_cell(open_, ext):
    rng = np.random.default_rng(1000 * open_ + ext)
    seen_min, seen_max = 0, 0
    for _ in range(25):
        scA, scB = _case(rng, open_, ext)
        seen_min = min(seen_min, int(scA.min())); seen_max = max(seen_max, int(scA.max()))
        refs = [_reference(scA, open_, ext), _reference(scB, open_, ext)]
        for biased in (False, True):
            H, E = _packed(scA, scB, open_, ext, biased)
            for half in range(2):
                assert np.array_equal(H[half], refs[half][0]), (biased, half)
                assert np.array_equal(E[half], refs[half][1]), (biased, half)
    assert seen_min == -96 and seen_max == 96


def test_masked_and_padded_cells_keep_the_floor():
    """a profile byte sum of 0 (PAD letter, masked row: s = -128) against the lowest stored value, the bias: x' = 0, no borrow"""
    sc = np.full((6, 6), -128)
    for biased in (False, True):
        H, E = _packed(sc, sc, 11, 1, biased)
        assert not H.any() and not E.any()


def test_biased_diagonal_sum_stays_inside_its_half():
    """exhaustive: diag' in [128, 0x7FFF] (what a register can hold: the bias at least, never a set sign bit), ub in [0, 255] - the half of
    x' = diag' + ub - 128 stays in [0, 65535]; and as packed 32-bit arithmetic with the other half at either extreme, neither half disturbs the other"""
    d = np.arange(128, 0x8000, dtype=np.int64)[:, None]
    ub = np.arange(0, 256, dtype=np.int64)[None, :]
    x = d + ub - 128
    assert x.min() == 0 and x.max() == 0x7FFF + 127 and x.max() < 65536
    for od, oub in ((128, 0), (0x7FFF, 255), (128, 255), (0x7FFF, 0)):
        want_other = od + oub - 128
        s = ((d | (od << 16)) + (ub | (oub << 16)) + UNBIAS) & 0xFFFFFFFF          # the varied half low
        assert np.array_equal(s & 0xFFFF, x) and ((s >> 16) == want_other).all()
        s = (((d << 16) | od) + ((ub << 16) | oub) + UNBIAS) & 0xFFFFFFFF          # ... and high
        assert np.array_equal(s >> 16, x) and ((s & 0xFFFF) == want_other).all()
    # the constant with -128 written into each half separately (0xFF80FF80) is off by one in the high half: the low half's sum always carries
    bad = ((d | (200 << 16)) + (ub | (100 << 16)) + 0xFF80FF80) & 0xFFFFFFFF
    assert ((bad >> 16) == 200 + 100 - 128 + 1).all()
