"""Kernel-level checks of the ProstT5 encoder (uc_t5_kernels.hip) through the uc_t5_kernel_* entry points of the C ABI:
every GEMM variant and epilogue, attention with relative-position bias, RMSNorm, the CNN head, the bias table and F32 weights.

References are float64 (numpy / torch) computed from the very f16 / fp32 values the kernel receives.  Tolerances are per output
element and follow from the roundings the kernels make; none is a global relative tolerance.  u = 2^-24 is the fp32 unit roundoff,
gamma(n) = n u / (1 - n u) bounds the relative error of an n-term fp32 sum in any order (Higham, Accuracy and Stability of
Numerical Algorithms, 3.1 / 3.5), half_ulp16(y) is half the spacing of f16 at magnitude |y| (the error of rounding to f16).

GEMM (fp32 MFMA accumulation of exact f16 x f16 products, then f16 RNE for epilogues 0 / 1, or + out in fp32 for epilogue 2):
    |kernel - A.W^T| <= gamma(K + 1) (|init| + sum_k |a_k w_k|) + half_ulp16(|ref| + that)       (epilogue 2: no f16 term)
    ReLU is 1-Lipschitz, so epilogue 1 has the same bound.  With integer operands in [-8, 8] every partial sum is an integer
    below 2^24 (|sum| <= 64 K = 2^20 at K = 16384, |init| < 2^22), so no fp32 rounding happens at all: the result must equal the
    float64 product rounded to f16 bit for bit, whatever the summation order - and therefore all variants must agree bit for bit.
Attention (S = Q K^T on MFMA + bias in fp32, exp2 of an FMA with the row maximum, P rounded to f16 for O = P V, l summed in fp32):
    per score the fp32 error is es_ij = gamma(129) (sum_d |q_id k_jd| + |b_ij|); the exponent is further perturbed by the rounding
    of m log2(e) and of the FMA (4 u (1 + |s|) each way) and the v_exp / rescale approximations (2^-20); so every weight carries a
    relative error of at most dd = expm1(2 max_j es_ij + 8 u (1 + max_j |s_ij|) + 2^-20) relative to a common factor, plus 2^-11
    (f16 rounding of P; subnormal P: 2^-25 absolute) in the numerator only.  With P_ij the exact probabilities and l_i >= 1 the
    exact denominator in units of the row maximum:
    |O - ref| <= ((dn + dd) / (1 - dd) + gamma(L + 2)) sum_j P_ij |v_jd| + 2^-25 sum_j |v_jd| / ((1 - dd) l_i) + 2 u |ref| + half_ulp16,
    dn = (1 + dd)(1 + 2^-11) - 1.  In the one-hot cases (Q = K = 0, one bias entry 40) every score is exact: the hot key has
    P = 1 and every other key exp(-40) (0 in f16), so the output row is V[hot] bit for bit; without a hot key P = 1 everywhere,
    l = L exactly, and the output is the mean of V within gamma(L + 2) sum |v| / L + 2 u |mean| + half_ulp16.
RMSNorm (fp32 sum of D squares, rsqrt, two products): relative error below (D + 8) u <= 6.3e-5 at D = 1024, less than the
    smallest relative half-ulp of f16 (2^-12); so the f16 result is within one f16 ulp of the float64 value.
CNN head (conv1 as one GEMM with f16 output, then fp32 sums of KW taps, ReLU, conv2 as fp32 sums of KW * C1 terms):
    ey  = gamma(D) sum_d |x w1| + half_ulp16(|y| + gamma(D) sum_d |x w1|)              per (token, tap, channel)
    ea  = sum_taps ey + gamma(KW + 1) (|b1| + sum_taps (|y| + ey))                      per (token, channel): h1 before / after ReLU
    ez  = sum_taps sum_c |w2| ea + gamma(KW C1 + 1) (|b2| + sum_taps sum_c |w2| (|h1| + ea))   per logit
    and the predicted state must agree wherever the reference's top-2 margin exceeds twice the row's largest ez.
"""
import os

import numpy as np
import pytest

import unicore_amd as U
from oracle import prostt5_ref as R

U32 = 2.0 ** -24


def gamma(n):
    n = np.asarray(n, np.float64)
    return n * U32 / (1 - n * U32)


def half_ulp16(y):
    e = np.floor(np.log2(np.maximum(np.abs(np.asarray(y, np.float64)), 2.0 ** -14)))
    return 2.0 ** (e - 11)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint16 if a.dtype == np.float16 else np.uint32)


def _cap():
    """UC_T5_GEMM256 caps the encoder's pick (0: 128 tile only, 1: no persistent kernel); unset = 2"""
    return int(os.environ.get("UC_T5_GEMM256", "2"))


def _capped(v):
    c = _cap()
    return 0 if c == 0 else (min(v, 1) if c == 1 else v)


def _expect_args_error(fn, *a, **kw):
    with pytest.raises(U.UcError) as e:
        fn(*a, **kw)
    assert e.value.code == U.UC_ERR_ARGS, str(e.value)


# ============================================================================================== GEMM
def _admissible(M, N, K):
    v = [0]
    if N % 256 == 0:
        v.append(1)
        if K >= 128 and M * K * 2 < 2 ** 32 and N * K * 2 < 2 ** 32:
            v.append(2)
    return v


@pytest.mark.parametrize("shape,variant", [
    ((1, 3072, 64), 0), ((2047, 256, 1024), 0), ((100, 1024, 16384), 0),                  # M < 2048
    ((2048, 256, 128), 2), ((2838, 3072, 1024), 2), ((65536, 1024, 16384), 2), ((131071, 1024, 16384), 2),   # M >= 2048, N % 256 = 0, K >= 128
    ((2048, 256, 64), 1), ((100000, 1024, 64), 1),                                        # K = 64
    ((2048, 320, 1024), 0), ((65536, 192, 1024), 0), ((4096, 64, 128), 0),                # N not a multiple of 256
    ((131072, 1024, 16384), 1), ((4096, 131072, 16384), 1),                               # M K 2 or N K 2 >= 2^32: 32-bit staging offsets
])
def test_gemm_dispatch_table(shape, variant):
    assert U.t5_gemm_variant(*shape) == _capped(variant)
    assert variant in _admissible(*shape)


def test_gemm_rejects_inadmissible_shapes_and_variants():
    """all of these fail before the device is touched (the CPU tier sees UC_ERR_ARGS, not UC_ERR_DEVICE)"""
    z = lambda m, k: np.zeros((m, k), np.float16)       # noqa: E731  (np.zeros: untouched pages, even at 4 GB)
    for M, N, K in ((64, 64, 96), (64, 66, 64), (64, 64, 32), (64, 2, 64)):
        _expect_args_error(U.t5_gemm_variant, M, N, K)
        _expect_args_error(U.t5_kernel_gemm, z(M, K), z(N, K), 0)
    _expect_args_error(U.t5_kernel_gemm, z(64, 64), z(64, 64), 3)                         # epilogue
    _expect_args_error(U.t5_kernel_gemm, z(64, 64), z(64, 64), 0, variant=3)
    _expect_args_error(U.t5_kernel_gemm, z(2048, 128), z(320, 128), 0, variant=1)         # N % 256
    _expect_args_error(U.t5_kernel_gemm, z(2048, 128), z(320, 128), 0, variant=2)
    _expect_args_error(U.t5_kernel_gemm, z(2048, 64), z(256, 64), 1, variant=2)           # K = 64: one K-tile
    _expect_args_error(U.t5_kernel_gemm, z(131072, 16384), z(256, 16384), 0, variant=2)                # M K 2 >= 2^32


def _int_ops(rng, M, N, K):
    return rng.integers(-8, 9, (M, K)).astype(np.float16), rng.integers(-8, 9, (N, K)).astype(np.float16)


def _init(rng, M, N):
    """distinct nonzero integers (within every 2^22 consecutive elements), |init| < 2^22"""
    v = (np.arange(M * N, dtype=np.int64) * 2654435761) % (2 ** 22 - 1) + 1
    return (v * rng.choice([-1, 1], M * N)).reshape(M, N).astype(np.float32)


def _check_exact(A, W, rng, variants):
    M, N, K = A.shape[0], W.shape[0], A.shape[1]
    ref = A.astype(np.float64) @ W.astype(np.float64).T
    assert np.abs(ref).max() < 2 ** 20
    init = _init(rng, M, N)
    want = {0: ref.astype(np.float16), 1: np.maximum(ref, 0).astype(np.float16), 2: (init.astype(np.float64) + ref).astype(np.float32)}
    assert np.array_equal(want[2].astype(np.float64), init.astype(np.float64) + ref)       # the fp32 result is exact too
    for v in variants:
        for epi in (0, 1, 2):
            got = U.t5_kernel_gemm(A, W, epi, variant=v, init=init if epi == 2 else None)
            bad = _bits(got) != _bits(want[epi])
            assert not bad.any(), "variant %d epilogue %d, %d x %d x %d: %d of %d outputs differ, first at %s" % (
                v, epi, M, N, K, bad.sum(), bad.size, np.argwhere(bad)[0].tolist())
            if epi == 1:
                assert not (_bits(got)[ref < 0]).any(), "ReLU must give +0 for negative sums"


EXACT_SHAPES = [(1, 64, 64), (17, 192, 192), (128, 320, 128), (129, 256, 1024), (255, 1024, 64), (256, 3072, 128), (257, 320, 192),
                (2047, 256, 192), (2048, 256, 64), (2048, 1024, 192), (2049, 320, 128), (2049, 256, 1024), (2838, 3072, 192),
                (2048, 256, 16384)]


@pytest.mark.gpu
def test_gemm_integer_operands_are_exact_in_every_variant_and_epilogue():
    """integer-valued f16 operands: each output is the float64 product rounded to f16 (epilogue 0), the same with negatives at
    exactly +0 (1), or init + A.W^T exactly (2) - for every variant the shape admits.  A dropped or doubled K-tile, a swizzle slip
    or a mis-stored row / column / tile shows up as an exact mismatch."""
    rng = np.random.default_rng(1)
    seen = set()
    for M, N, K in EXACT_SHAPES:
        vs = _admissible(M, N, K)
        seen.update(vs)
        A, W = _int_ops(rng, M, N, K)
        _check_exact(A, W, rng, vs)
        got = U.t5_kernel_gemm(A, W, 0)                                                    # the library's own pick
        assert np.array_equal(_bits(got), _bits((A.astype(np.float64) @ W.astype(np.float64).T).astype(np.float16)))
    assert seen == {0, 1, 2}


def _persistent_walks(M, N, cus, gxm=2):
    """the tiles each workgroup of t5_gemm256x_kernel walks (t5_gemm256x_launch's grid, the kernel's decode / seek)"""
    nn, nm = N // 256, -(-M // 256)
    n_local = ((nm + 7) // 8 + gxm - 1) // gxm * gxm * nn
    slots = min(n_local, max(1, cus // 8))
    walks = []
    for xcd in range(8):
        for s in range(slots):
            w = []
            for k in range(s, n_local, slots):
                g, r = k // (gxm * nn), k % (gxm * nn)
                mt = xcd + 8 * (g * gxm + r % gxm)
                if mt < nm:
                    w.append((mt, r // gxm))
            walks.append(w)
    return walks


@pytest.mark.gpu
def test_gemm_persistent_workgroups_walking_several_tiles_are_exact():
    """M = 8191, N = 4096: every persistent workgroup walks >= 2 tiles on an MI355X, across row tiles, so the K-stream that runs
    from one tile into the next (staging offsets switched piece by piece) is exercised; the last row tile is partial"""
    import torch
    M, N, K = 8191, 4096, 128
    walks = _persistent_walks(M, N, torch.cuda.get_device_properties(0).multi_processor_count)
    assert min(len(w) for w in walks if w) >= 2, [len(w) for w in walks]
    assert any(len({mt for mt, _ in w}) >= 2 for w in walks)
    rng = np.random.default_rng(2)
    A, W = _int_ops(rng, M, N, K)
    _check_exact(A, W, rng, [2])


RANDOM_SHAPES = [(17, 64, 1024), (129, 320, 192), (2048, 1024, 192), (2049, 256, 1024), (300, 256, 16384)]


@pytest.mark.gpu
def test_gemm_random_normal_operands_within_the_derived_bound_and_variants_bit_identical():
    rng = np.random.default_rng(3)
    for M, N, K in RANDOM_SHAPES:
        A = rng.standard_normal((M, K)).astype(np.float16)
        W = (rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float16)
        init = rng.standard_normal((M, N)).astype(np.float32)
        A64, W64 = A.astype(np.float64), W.astype(np.float64)
        ref, mag = A64 @ W64.T, np.abs(A64) @ np.abs(W64).T
        for epi in (0, 1, 2):
            r = ref if epi == 0 else np.maximum(ref, 0) if epi == 1 else init + ref
            err = gamma(K + 1) * (mag + (np.abs(init) if epi == 2 else 0))
            tol = err + (half_ulp16(np.abs(r) + err) if epi < 2 else 0)
            outs = []
            for v in _admissible(M, N, K):
                got = U.t5_kernel_gemm(A, W, epi, variant=v, init=init if epi == 2 else None)
                d = np.abs(got.astype(np.float64) - r)
                assert np.all(d <= tol), "variant %d epilogue %d, %d x %d x %d: worst excess %.3g at %s" % (
                    v, epi, M, N, K, (d - tol).max(), np.unravel_index(np.argmax(d - tol), d.shape))
                outs.append(got)
            for o in outs[1:]:
                assert np.array_equal(_bits(o), _bits(outs[0])), "variants disagree on %d x %d x %d epilogue %d" % (M, N, K, epi)


# ============================================================================================== attention
LENGTHS = [1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1000]
ONE_HOT_REL = [0, 1, -1, 5, -63, 64, -127, 128, -128, 129, -191, 192, 255, -256, 257, -999, 999, 31, -32, 33, -64, 63, 127, -129,
               191, -192, 2, -5, 100, -100, 500, -500]


def _offsets(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def _attn_ref_bound(q, k, v, b):
    """float64 softmax(q k^T + b) v of one (sequence, head) and the per-element bound of the module docstring"""
    L = len(q)
    s = q @ k.T + b
    m = s.max(1, keepdims=True)
    w = np.exp(s - m)
    l = w.sum(1, keepdims=True)
    P = w / l
    ref = P @ v
    es = gamma(129) * (np.abs(q) @ np.abs(k).T + np.abs(b))
    dd = np.expm1(2 * es.max(1, keepdims=True) + 8 * U32 * (1 + np.abs(s).max(1, keepdims=True)) + 2.0 ** -20)
    dn = (1 + dd) * (1 + 2.0 ** -11) - 1
    pv = P @ np.abs(v)
    err = ((dn + dd) / (1 - dd) + gamma(L + 2)) * pv + 2.0 ** -25 * np.abs(v).sum(0, keepdims=True) / ((1 - dd) * l) + 2 * U32 * np.abs(ref)
    return ref, err + half_ulp16(np.abs(ref) + err), s


def _bias_dense(bias_h, span, L):
    rel = np.arange(L)[None, :] - np.arange(L)[:, None]
    return bias_h.astype(np.float64)[rel + span - 1]


def _split(qkv, H):
    T = qkv.shape[0]
    x = qkv.astype(np.float64).reshape(T, 3, H, 128)
    return x[:, 0], x[:, 1], x[:, 2]


@pytest.mark.gpu
def test_attention_one_hot_bias_pins_window_heads_masks_and_sequence_isolation():
    """Q = K = 0, head h has bias 40 at key - query = ONE_HOT_REL[h] only: where that key exists the output row is V[key] bit for
    bit, elsewhere the mean of the sequence's V rows.  Pins the bias window, the head offsets in q | k | v, the last-block key mask
    and the isolation of the sequences packed into one call (each has its own V)."""
    H, rng = 32, np.random.default_rng(4)
    off = _offsets(LENGTHS)
    T, span = int(off[-1]), max(LENGTHS)                      # bias_span = max L: the smallest valid value
    mag = rng.uniform(0.5, 4.0, (T, H, 128)) * rng.choice([-1.0, 1.0], (T, H, 128))
    qkv = np.zeros((T, 3, H, 128), np.float16)
    qkv[:, 2] = mag.astype(np.float16)
    qkv = qkv.reshape(T, 3 * H * 128)
    bias = np.zeros((H, 2 * span - 1), np.float32)
    for h, r in enumerate(ONE_HOT_REL):
        bias[h, r + span - 1] = 40.0
    out = U.t5_kernel_attention(qkv, LENGTHS, bias, span, H).astype(np.float64).reshape(T, H, 128)
    V = qkv.reshape(T, 3, H, 128)[:, 2]
    hits = 0
    for s, L in enumerate(LENGTHS):
        b = int(off[s])
        v = V[b:b + L].astype(np.float64)                                                    # [L, H, 128]
        mean = v.mean(0)
        tol = gamma(L + 2) * np.abs(v).sum(0) / L + 2 * U32 * np.abs(mean)
        tol = tol + half_ulp16(np.abs(mean) + tol)
        for h, r in enumerate(ONE_HOT_REL):
            q = np.arange(L)
            hot = (q + r >= 0) & (q + r < L)
            if hot.any():
                exp = V[b + q[hot] + r, h]
                assert np.array_equal(_bits(out[b + q[hot], h].astype(np.float16)), _bits(exp)), "L %d head %d (rel %d)" % (L, h, r)
                hits += int(hot.sum())
            if (~hot).any():
                d = np.abs(out[b + q[~hot], h] - mean[h])
                assert np.all(d <= tol[h]), "L %d head %d (rel %d): uniform rows off by %.3g" % (L, h, r, (d - tol[h]).max())
    assert hits > 10000


def _random_attention_case(rng, lengths, H, span):
    off = _offsets(lengths)
    T = int(off[-1])
    qkv = np.empty((T, 3, H, 128), np.float16)
    qkv[:, 0] = (1.6 * rng.standard_normal((T, H, 128))).astype(np.float16)
    qkv[:, 1] = (1.6 * rng.standard_normal((T, H, 128))).astype(np.float16)
    qkv[:, 2] = rng.standard_normal((T, H, 128)).astype(np.float16)
    bias = (2.0 * rng.standard_normal((H, 2 * span - 1))).astype(np.float32)
    bias[:, span - 1 + 100] += 150.0                            # a query's maximum is its key + 100: a later key block than its first
    return qkv.reshape(T, 3 * H * 128), bias


def _check_random_attention(qkv, lengths, bias, span, H):
    out = U.t5_kernel_attention(qkv, lengths, bias, span, H)
    q, k, v = _split(qkv, H)
    o = out.astype(np.float64).reshape(-1, H, 128)
    off, later = _offsets(lengths), 0
    for s, L in enumerate(lengths):
        b = int(off[s])
        for h in range(H):
            ref, tol, sc = _attn_ref_bound(q[b:b + L, h], k[b:b + L, h], v[b:b + L, h], _bias_dense(bias[h], span, L))
            d = np.abs(o[b:b + L, h] - ref)
            assert np.all(d <= tol), "L %d head %d: worst excess %.3g at %s" % (L, h, (d - tol).max(), np.unravel_index(np.argmax(d - tol), d.shape))
            later += int((sc.argmax(1) >= 64).sum())
    assert later > 0
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("H,extra_span", [(1, 0), (3, 37)])
def test_attention_random_scores_against_fp64_softmax_and_packed_equals_per_sequence(H, extra_span):
    """random Q / K / V with scores up to ~+-100 plus a random bias table (span = max L, and a larger one); packing all lengths
    into one call gives the same bits as one call per sequence"""
    rng = np.random.default_rng(5 + H)
    span = max(LENGTHS) + extra_span
    qkv, bias = _random_attention_case(rng, LENGTHS, H, span)
    out = _check_random_attention(qkv, LENGTHS, bias, span, H)
    off = _offsets(LENGTHS)
    for s, L in enumerate(LENGTHS):
        one = U.t5_kernel_attention(qkv[off[s]:off[s + 1]], [L], bias, span, H)
        assert np.array_equal(_bits(one), _bits(out[off[s]:off[s + 1]])), "L %d alone differs from L %d packed" % (L, L)


@pytest.mark.gpu
def test_attention_random_32_heads():
    rng = np.random.default_rng(6)
    lengths, span = [1, 33, 129, 257, 64], 400
    qkv, bias = _random_attention_case(rng, lengths, 32, span)
    _check_random_attention(qkv, lengths, bias, span, 32)


def test_attention_rejects_bad_arguments():
    qkv, bias = np.zeros((10, 3 * 128), np.float16), np.zeros((1, 2 * 10 - 1), np.float32)
    _expect_args_error(U.t5_kernel_attention, qkv, [10], bias[:, :17], 9, 1)               # bias_span < max L
    _expect_args_error(U.t5_kernel_attention, qkv, [10, 0], bias, 10, 1)                   # empty sequence
    _expect_args_error(U.t5_kernel_attention, qkv, [], bias, 10, 1)
    _expect_args_error(U.t5_kernel_attention, qkv, [10], bias, 10, 0)                      # no head


# ============================================================================================== RMSNorm
@pytest.mark.gpu
def test_rmsnorm_within_one_f16_ulp_at_every_width_and_magnitude():
    """rows at ~1, ~1e-4 (eps dominates mean(x^2)), ~1e4 and all zero (must give 0, not NaN); D not a multiple of 256 included"""
    rng, eps = np.random.default_rng(7), 1e-6
    for D in (64, 192, 256, 320, 1024):
        w = (1 + 0.1 * rng.standard_normal(D)).astype(np.float32)
        for T in (1, 3, 4, 5, 257):
            scale = np.array([1.0, 1e-4, 1e4, 0.0])[np.arange(T) % 4]
            x = (rng.standard_normal((T, D)) * scale[:, None]).astype(np.float32)
            y = U.t5_kernel_rmsnorm(x, w, eps).astype(np.float64)
            x64 = x.astype(np.float64)
            ref = x64 / np.sqrt((x64 * x64).mean(1, keepdims=True) + np.float64(np.float32(eps))) * w.astype(np.float64)
            assert np.isfinite(y).all()
            d = np.abs(y - ref)
            assert np.all(d <= 2 * half_ulp16(ref)), "D %d T %d: %.3g ulp" % (D, T, (d / (2 * half_ulp16(ref))).max())
            assert not y[scale == 0].any()


def test_rmsnorm_rejects_widths_that_are_not_multiples_of_4():
    _expect_args_error(U.t5_kernel_rmsnorm, np.zeros((2, 66), np.float32), np.ones(66, np.float32), 1e-6)


# ============================================================================================== CNN head
def _taps(Y):
    """Y [n, C, KW] -> [n, C]: out[t] = sum_k Y[t + k - KW // 2, :, k] over the rows inside the sequence (zero padding)"""
    n, C, KW = Y.shape
    out = np.zeros((n, C))
    for k in range(KW):
        s = k - KW // 2
        lo, hi = max(0, -s), min(n, n - s)
        if hi > lo:
            out[lo:hi] += Y[lo + s:hi + s, :, k]
    return out


def _head_ref_bound(x, w1h, b1, w2, b2, eos_in_head):
    """x [L, D] float64 of one sequence (<AA2fold>, residues, </s>) -> logits [residues, NO] and the per-logit bound"""
    xs = x[1:].copy()                                        # the prefix is sliced off before the CNN
    if not eos_in_head:
        xs[-1] = 0                                           # predict_3Di: </s> masked to zero, its position stays
    D, KW, C1 = x.shape[1], w1h.shape[2], w1h.shape[0]
    Y = np.einsum("ud,cdk->uck", xs, w1h)
    Ya = np.einsum("ud,cdk->uck", np.abs(xs), np.abs(w1h))
    ey = gamma(D) * Ya
    ey = ey + half_ulp16(np.abs(Y) + ey)
    a = b1 + _taps(Y)
    ea = _taps(ey) + gamma(KW + 1) * (np.abs(b1) + _taps(np.abs(Y) + ey))
    h = np.maximum(a, 0)
    z = b2 + _taps(np.einsum("uc,ock->uok", h, w2))
    aw2 = np.abs(w2)
    ez = _taps(np.einsum("uc,ock->uok", ea, aw2)) + gamma(KW * C1 + 1) * (np.abs(b2) + _taps(np.einsum("uc,ock->uok", h + ea, aw2)))
    return z[:-1], ez[:-1]                                   # </s> dropped after the head


@pytest.mark.gpu
@pytest.mark.parametrize("eos_in_head", [1, 0])
def test_cnn_head_sequence_edges_against_fp64_convolutions(eos_in_head):
    """residue counts 1 .. 8 (shorter than the kernel width) and 300 packed into one call: the taps stop at each sequence's
    prefix and (eos_in_head = 0) its </s>; logits within the derived bound, states equal wherever the margin allows"""
    rng = np.random.default_rng(8 + eos_in_head)
    D, C1, KW, NO = 256, 32, 7, 20
    res = [1, 2, 3, 4, 7, 8, 300]
    lengths = [n + 2 for n in res]
    off = _offsets(lengths)
    x = rng.standard_normal((int(off[-1]), D)).astype(np.float16)
    w1 = (rng.standard_normal((C1, D, KW)) / np.sqrt(D * KW)).astype(np.float32)
    b1 = (0.1 * rng.standard_normal(C1)).astype(np.float32)
    w2 = (rng.standard_normal((NO, C1, KW)) / np.sqrt(C1)).astype(np.float32)
    b2 = (0.1 * rng.standard_normal(NO)).astype(np.float32)
    codes, logits = U.t5_kernel_cnn_head(x, lengths, w1, b1, w2, b2, eos_in_head)
    w1h = w1.astype(np.float16).astype(np.float64)            # the loader's rounding of conv1
    for s, n in enumerate(res):
        b = int(off[s])
        z, ez = _head_ref_bound(x[b:b + n + 2].astype(np.float64), w1h, b1.astype(np.float64), w2.astype(np.float64), b2.astype(np.float64), eos_in_head)
        got = logits[b + 1:b + 1 + n].astype(np.float64)
        d = np.abs(got - z)
        assert np.all(d <= ez), "%d residues: worst excess %.3g at %s" % (n, (d - ez).max(), np.unravel_index(np.argmax(d - ez), d.shape))
        top2 = np.sort(z, 1)[:, -2:]
        firm = (top2[:, 1] - top2[:, 0]) > 2 * ez.max(1)
        assert np.array_equal(codes[b + 1:b + 1 + n][firm], z.argmax(1)[firm]), "%d residues: states differ" % n


def test_cnn_head_rejects_bad_geometry():
    x, L = np.zeros((6, 128), np.float16), [3, 3]
    w1, b1, w2, b2 = np.zeros((4, 128, 7), np.float32), np.zeros(4, np.float32), np.zeros((20, 4, 7), np.float32), np.zeros(20, np.float32)
    _expect_args_error(U.t5_kernel_cnn_head, np.zeros((6, 96), np.float16), L, np.zeros((4, 96, 7), np.float32), b1, w2, b2, 1)   # D % 64
    _expect_args_error(U.t5_kernel_cnn_head, x, L, w1[:, :, :6], b1, w2[:, :, :6], b2, 1)                                         # even KW
    _expect_args_error(U.t5_kernel_cnn_head, x, L, w1, b1, np.zeros((22, 4, 7), np.float32), np.zeros(22, np.float32), 1)         # NO > 21
    _expect_args_error(U.t5_kernel_cnn_head, x, [1, 5], w1, b1, w2, b2, 1)                                                        # < prefix + </s>


# ============================================================================================== bias table
@pytest.mark.parametrize("buckets,max_dist", [(32, 128), (64, 256), (32, 64), (16, 128), (8, 32)])
def test_bias_table_matches_the_transformers_bucketing(buckets, max_dist):
    """the table the encoder uploads == rel_bias looked up through transformers' float32 bucket rule, for every |rel| < span;
    the exact powers of two (where float rounding of log(n / max_exact) / log(max_distance / max_exact) decides) named explicitly"""
    import torch
    rng, H, span = np.random.default_rng(buckets + max_dist), 3, 1100
    rb = rng.standard_normal((H, buckets)).astype(np.float32)
    tab = U.t5_bias_table(rb, max_dist, span)
    rel = np.arange(-(span - 1), span)
    bk = R.relative_position_bucket(torch.tensor(rel), buckets, max_dist).numpy()
    want = rb[:, bk]
    bad = np.nonzero((tab != want).any(0))[0]
    assert not len(bad), "rel %s: buckets differ" % rel[bad][:10].tolist()
    for n in (1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024):
        for r in (n, -n):
            assert np.array_equal(tab[:, r + span - 1], rb[:, int(R.relative_position_bucket(torch.tensor([r]), buckets, max_dist)[0])]), r


# ============================================================================================== F32 weights
@pytest.mark.gpu
def test_f32_weight_tensors_load_to_the_same_model_as_f16(tmp_path):
    """a GGUF file whose weight matrices are F32 (converted on the device by t5_f32_to_f16) holding f16 values encodes exactly
    like the same model stored as F16"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_t5_golden as G
    cfg = R.default_config(**G.CFG)
    raw = str(tmp_path / "raw.gguf")
    R.write_synthetic_gguf(raw, cfg, seed=G.SEED, f16=False)
    kv, w = R.read_gguf(raw)
    mats = ("token_embd.weight", "attn_q.weight", "attn_k.weight", "attn_v.weight", "attn_o.weight", "ffn_up.weight", "ffn_down.weight")
    as16 = {n: np.asarray(a).astype(np.float16) for n, a in w.items() if n.endswith(mats)}
    assert len(as16) == 1 + 6 * cfg["n_layers"] and all(w[n].dtype == np.float32 for n in as16)
    p16, p32 = str(tmp_path / "m16.gguf"), str(tmp_path / "m32.gguf")
    R.write_gguf(p16, kv, [(n, as16.get(n, a)) for n, a in w.items()])
    R.write_gguf(p32, kv, [(n, as16[n].astype(np.float32) if n in as16 else a) for n, a in w.items()])
    seqs = list(G.SEQS) + ["ACDEFGHIKLMNPQRSTVWY" * 9]
    res = []
    for p in (p16, p32):
        enc = U.T5Encoder(p)
        try:
            res.append(enc.encode(seqs, logits=True))
        finally:
            enc.close()
    (c16, l16), (c32, l32) = res
    for i in range(len(seqs)):
        assert np.array_equal(c16[i], c32[i]) and np.array_equal(l16[i].view(np.uint32), l32[i].view(np.uint32)), seqs[i][:20]
