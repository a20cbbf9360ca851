"""CPU tests of the oracle (test infrastructure) — pins it before it is
trusted as the GPU engine's checker.

Pins, in order of strength:
  1. big-integer golden vectors (tests/golden/, generated from the math by
     make_golden.py): NTT evaluation points/order, negacyclic products,
     coefficient-domain automorphisms;
  2. exact properties: fast basis conversion = x + u*Q with 0 <= u < |digit|
     (here, and word for word in tests/test_bigint_model.py), ModDown = the
     centred division by P, exact outside fp64 ties, rescale, the key switch
     and the ops built from them against Python integers
     (tests/bigint_model.py, tests/test_bigint_model.py);
  3. the reference's own tests and tolerances, restated:
       DecomposeTest.cpp:64-74, SignTest.cpp:41-122, CompareTest.cpp:43-63,
       RotationTest.cpp:63-130, SincTest.cpp (indicator on k/(2N)),
       DirectSortTest.cpp:90-170, DirectSortNTest.cpp:61-285.
OpenFHE itself is not available, so ciphertext-level parity with the
reference is "parity unpinned" (DESIGN.md §6).
"""
import json
import os
import sys

import numpy as np
import pytest

import pyoracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def load(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


# ---------------------------------------------------------------- golden ---
@pytest.mark.parametrize('case', load('ntt_golden.json'), ids=lambda c: f"logN{c['logN']}")
def test_ntt_golden(case):
    logN = case['logN']
    ctx = O.Context(logN, 1, 40, 60, 3, seed=1, keygen=False)
    q = int(case['q'])
    assert int(ctx.primes[0]) == q
    assert ctx.psi(0) == int(case['psi'])
    a = np.array([int(v) for v in case['a']], dtype=np.uint64)
    b = np.array([int(v) for v in case['b']], dtype=np.uint64)
    A = ctx.ntt(0, a)
    assert [int(v) for v in A] == [int(v) for v in case['ntt_a']]
    assert np.array_equal(ctx.ntt(0, A, inverse=True), a)
    B = ctx.ntt(0, b)
    prod = np.array([(int(x) * int(y)) % q for x, y in zip(A, B)], dtype=np.uint64)
    assert [int(v) for v in ctx.ntt(0, prod, inverse=True)] == [int(v) for v in case['negacyclic_ab']]


@pytest.mark.parametrize('case', load('automorph_golden.json'), ids=lambda c: f"k{c['k']}")
def test_automorphism_golden(case):
    logN = case['logN']
    ctx = O.Context(logN, 1, 40, 60, 3, seed=1, keygen=False)
    assert int(ctx.primes[0]) == int(case['q'])
    assert O.galois(logN, case['k']) == case['galois']
    a = np.array([int(v) for v in case['a']], dtype=np.uint64)
    perm = O.automorph_perm(logN, case['galois'])
    got = ctx.ntt(0, ctx.ntt(0, a)[perm], inverse=True)
    assert [int(v) for v in got] == [int(v) for v in case['sigma_a']]


def test_sinc_coefficients_reproduce_indicator():
    # SincTest.cpp:75-229 semantics: doubled sinc ~ [k == 0 or k == -N] on k/(2N)
    for case in load('sinc_golden.json'):
        N = case['N']
        c = O.doubled_sinc(N)
        x = np.array(case['x'])
        f = np.array(case['f'])
        approx = np.polynomial.chebyshev.chebval(x, np.concatenate([[c[0] / 2], c[1:]]))
        assert np.max(np.abs(approx - f)) < 1e-3
        ind = np.isclose(x * 2 * N, 0) | np.isclose(x * 2 * N, -N)
        assert np.max(np.abs(approx - ind)) < 0.01


def test_sinc_degrees():
    # degree of the truncated degree-13011 fit (utils/generate_cheb_doubled_coeffs.cpp:14-36)
    assert {N: len(O.doubled_sinc(N)) for N in (8, 128, 1024)} == {8: 71, 128: 849, 1024: 6511}


# ----------------------------------------------------------------- params --
def test_params_scale_stays_put():
    ctx = O.Context(12, 39, 40, 60, 3, seed=1, keygen=False)
    assert ctx.nq == 40 and ctx.alpha == 14 and ctx.K == 10
    assert np.all(np.abs(np.log2(ctx.delta) - 40) < 1e-3)  # no scale drift down the chain
    assert len(set(int(p) for p in ctx.primes)) == len(ctx.primes)
    assert all(int(p) % (2 * 4096) == 1 for p in ctx.primes)


def test_modup_is_exact_basis_extension():
    ctx = O.Context(6, 5, 40, 60, 3, seed=1, keygen=False)
    rng = np.random.default_rng(0)
    ell = 5
    primes = [int(p) for p in ctx.primes]
    d = np.stack([rng.integers(0, primes[i], size=ctx.n, dtype=np.uint64) for i in range(ell)])
    ext = ctx.modup(d)
    coef = np.stack([ctx.ntt(i, d[i], inverse=True) for i in range(ell)])
    tgt = list(range(ell)) + list(range(ctx.nq, ctx.nq + ctx.K))
    for j in range((ell + ctx.alpha - 1) // ctx.alpha):
        lo, hi = j * ctx.alpha, min(ell, (j + 1) * ctx.alpha)
        Qj = 1
        for i in range(lo, hi):
            Qj *= primes[i]
        for t_idx, pt in enumerate(tgt):
            if lo <= t_idx < hi:
                assert np.array_equal(ext[j, t_idx], d[t_idx])
                continue
            out = ctx.ntt(pt, ext[j, t_idx], inverse=True)
            for k in range(0, ctx.n, 7):
                X = 0  # CRT of the digit residues
                for i in range(lo, hi):
                    qh = Qj // primes[i]
                    X += int(coef[i, k]) * qh * pow(qh, -1, primes[i])
                X %= Qj
                diff = (int(out[k]) - X) % primes[pt]
                assert any(diff == (u * Qj) % primes[pt] for u in range(hi - lo)), (j, t_idx, k)


# ---------------------------------------------------------- decomposer -----
def test_decompose_compose_match():
    # tests/DecomposeTest.cpp:64-74
    rots = [1, 2, 4, 8, 16, 32, 64]
    for num in [1, 2, 3, 4, 7, 8, 15, 16, 31, 32, 63, 64, 65, 127, 128]:
        for algo in (O.NAF, O.BNAF, O.BINARY):
            steps = O.decompose(128, rots, num, 128, algo)
            assert sum(s for _, s in steps) == num, (num, algo, steps)


def test_decompose_directsort_steps():
    _, rots = O.size_parameters(1024)
    assert O.decompose(1024, rots, 40, 32768, O.BINARY) == [(1, 32), (1, 8)]
    assert O.decompose(1024, rots, 1016, 32768, O.BINARY) == [(1, 512), (1, 256), (1, 128), (1, 64),
                                                               (1, 32), (1, 16), (1, 8)]


def test_size_parameters_table():
    # src/sort_algo.h:87-201
    exp = {4: 23, 8: 24, 16: 25, 32: 28, 64: 29, 128: 30, 256: 34, 512: 35, 1024: 39}
    for N, d in exp.items():
        depth, rots = O.size_parameters(N)
        assert depth == d
    assert len(O.size_parameters(128)[1]) == 30
    assert len(O.size_parameters(1024)[1]) == 161
    with pytest.raises(ValueError):
        O.size_parameters(3)


# --------------------------------------------------------- ciphertexts -----
@pytest.fixture(scope='module')
def ctx30():
    c = O.Context(12, 30, 50, 60, 3, seed=3)
    c.gen_rotation_keys([-1, -2, -4, -8, -16, -32, 1, 2, 4, 8, 16, 32, 64, 512])
    return c


def test_encrypt_decrypt_roundtrip(ctx30):
    x = np.random.default_rng(1).uniform(-5, 5, 64)
    assert np.max(np.abs(ctx30.decrypt(ctx30.encrypt(x, 64)) - x)) < 1e-9


def test_composite_sign3_signtest(ctx30):
    # tests/SignTest.cpp:41-80: compositeSign<3>(dg=0, df=1)
    x = np.array([0.5, -0.3, 0.1, -0.7, 0.0, 0.8, -0.9, 0.2])
    y = ctx30.decrypt(ctx30.sign(ctx30.encrypt(x, 8), 3, 0, 1))
    # plaintext model of g3 then f3 (the composition the reference evaluates)
    g = lambda t: (4589 * t - 16577 * t**3 + 25614 * t**5 - 12860 * t**7) / 1024
    f = lambda t: (35 * t - 35 * t**3 + 21 * t**5 - 5 * t**7) / 16
    assert np.max(np.abs(y - f(g(x)))) < 1e-6
    assert np.all(np.sign(y[x != 0]) == np.sign(x[x != 0])) and abs(y[4]) < 0.1
    # the reference expects +-1 within 0.1 everywhere; f3(g3(0.1)) = 0.788 mathematically,
    # so that one element cannot meet it on any engine (documented in DESIGN.md §6)
    far = np.abs(x) >= 0.2
    assert np.max(np.abs(y[far] - np.sign(x[far]))) < 0.1


def test_composite_sign4_small_inputs(ctx30):
    # tests/SignTest.cpp:82-122: compositeSign<4>(3, 3)
    x = np.array([0.02, -0.02, 0.01, -0.01, 0.009, -0.009, 1, -1])
    y = ctx30.decrypt(ctx30.sign(ctx30.encrypt(x, 8), 4, 3, 3))
    assert np.max(np.abs(y - np.sign(x))) < 0.1


def test_compare_vectors():
    # tests/CompareTest.cpp:13-22, 43-63: depth 50, scaling mod 59 (g3's constant 25614/1024
    # times 2^59 exceeds 2^63: carried as a rounded mantissa and a power of two)
    c = O.Context(12, 50, 59, 60, 3, seed=4)
    a = c.encrypt([1.0, 5.0, 3.0, 4.0], 4)
    b = c.encrypt([2.0, 4.0, 3.0, 3.0], 4)
    y = c.decrypt(c.compare(a, b, 4, 3, 3))
    assert np.max(np.abs(y - [0.0, 1.0, 0.5, 1.0])) < 0.1


def test_indicator(ctx30):
    # Comparison::indicator: 1 iff |x| < c   (src/comparison.cpp:24-40)
    x = np.array([0.0, 0.3, -0.3, 0.05, -0.05, 0.6, -0.6, 0.0])
    y = ctx30.decrypt(ctx30.indicator(ctx30.encrypt(x, 8), 0.15, 3, 2, 2))
    assert np.max(np.abs(y - (np.abs(x) < 0.15))) < 0.1


def test_rotation_composer(ctx30):
    # tests/RotationTest.cpp:63-130 (NAF composer, keys {+-1..+-32, 64, 512})
    rots = [-1, -2, -4, -8, -16, -32, 1, 2, 4, 8, 16, 32, 64, 512]
    x = np.random.default_rng(2).permutation(128) / 100
    ct = ctx30.encrypt(x, 128)
    for r in (-4, 3, -7, 100, -128, 127):
        out = ctx30.compose_rotate(ct, 128, rots, O.NAF, r)
        assert np.max(np.abs(ctx30.decrypt(out) - np.roll(x, -r))) < 1e-6
        back = ctx30.compose_rotate(out, 128, rots, O.NAF, -r)
        assert np.max(np.abs(ctx30.decrypt(back) - x)) < 1e-5


def test_hoisted_equals_single(ctx30):
    ct = ctx30.encrypt(np.arange(16) / 16.0, 16)
    hs = ctx30.rotate_hoisted(ct, [1, 2, 4])
    for h, k in zip(hs, [1, 2, 4]):
        assert np.array_equal(h.data(), ctx30.rotate(ct, k).data())


def test_missing_key_raises(ctx30):
    with pytest.raises(RuntimeError, match='no rotation key'):
        ctx30.rotate(ctx30.encrypt([1.0, 2.0], 2), 3)


# Output level of a degree-d Chebyshev series in OpenFHE: the linear method
# below degree 5 (T_1..T_d, then one constant product); PS above, in the
# published depth bands (degree 6-13: 4, 14-27: 5, 28-59: 6, 60-119: 7,
# 120-247: 8 ...).  Degrees 6, 7 and 120-127 cost one level more than the
# depth-optimal ceil(log2(d+1)): N=16's doubled sinc has degree 126, which is
# why the reference budgets multDepth 25 for N=16 (src/sort_algo.h:104-108).
OPENFHE_PS_DEPTH = {2: 2, 3: 3, 5: 3, 6: 4, 7: 4, 15: 5, 60: 7, 126: 8}


@pytest.mark.parametrize('deg', [2, 3, 5, 6, 7, 15, 60, 126])
def test_chebyshev_ps_depth_and_value(deg):
    c = O.Context(11, 12, 40, 60, 3, seed=5)
    x = np.linspace(-1, 1, 32)
    ct = c.encrypt(x, 32)
    co = np.random.default_rng(deg).normal(size=deg + 1)
    y = c.cheb(ct, co)
    ref = np.polynomial.chebyshev.chebval(x, np.concatenate([[co[0] / 2], co[1:]]))
    assert np.max(np.abs(c.decrypt(y) - ref)) < 2e-6 * np.sum(np.abs(co))
    assert y.level == OPENFHE_PS_DEPTH[deg]  # levels OpenFHE's EvalChebyshevSeriesPS consumes


def test_ps_depth_tables():
    """Both Paterson-Stockmeyer splits consume the same levels for every degree
    (OpenFHE's (k, m) held to its published band up to 2204), so the
    conditioning fallback of the OpenFHE split never changes an output level."""
    for d in range(1, 4097):
        assert O.cheb_ps_depth(d, 1) == O.cheb_ps_depth(d, 0), d
    # the reference's series (doubled sinc N = 4..2048, g_4, scaled sinc, EvalMod)
    for d, depth in [(42, 6), (70, 7), (126, 8), (232, 8), (438, 9), (848, 10), (1662, 11), (3280, 12),
                     (6510, 13), (13020, 14), (27, 5), (88, 7)]:
        assert O.cheb_ps_depth(d, 1) == depth


@pytest.mark.parametrize('N', [16, 64])
def test_openfhe_split_doubled_sinc(N):
    """OpenFHE's split (the default) evaluates the doubled-sinc index-check series
    (src/sort_algo.h:725-728) on its grid x = j/(2N) at the depth the reference
    budgets, more precisely than the power-of-two split at the same 40-bit scale
    (the power-of-two split amplifies baby-step noise 4^11-fold at x = 0)."""
    c = np.fromfile(os.path.join(REPO, 'fhe-sorting_amd', 'data', f'doubled_sinc_{N}.f64'))
    x = np.resize(np.arange(-(2 * N - 2), N) / (2 * N), 256)
    ref = np.polynomial.chebyshev.chebval(x, np.concatenate([[c[0] / 2], c[1:]]))
    errs = {}
    for split in (1, 0):
        ctx = O.Context(11, 10, 40, 60, 3, seed=4, ps_split=split)
        y = ctx.cheb(ctx.encrypt(x, 256), c)
        assert y.level == O.cheb_ps_depth(len(c) - 1)
        errs[split] = float(np.max(np.abs(ctx.decrypt(y)[:256] - ref)))
    assert errs[1] < 1e-5 and errs[1] <= errs[0]


def test_openfhe_split_ill_conditioned_falls_back():
    """A series with O(1) coefficients that do not decay makes OpenFHE's second
    division blow up (|c| ~ 1e7 at degree 60): such a series is evaluated with the
    power-of-two split, word for word, instead of returning garbage."""
    co = np.random.default_rng(60).normal(size=61)
    x = np.linspace(-1, 1, 32)
    words = []
    for split in (1, 0):
        ctx = O.Context(11, 8, 40, 60, 3, seed=6, ps_split=split)
        y = ctx.cheb(ctx.encrypt(x, 32), co)
        words.append(y.data())
        ref = np.polynomial.chebyshev.chebval(x, np.concatenate([[co[0] / 2], co[1:]]))
        assert np.max(np.abs(ctx.decrypt(y)[:32] - ref)) < 1e-4
    assert np.array_equal(words[0], words[1])


def test_ps_noise_model_restatement():
    """scripts/ps_noise_model.py's restatements of both splits reproduce the plain
    series without noise (the model behind DESIGN.md §3's table)."""
    sys.path.insert(0, os.path.join(REPO, 'scripts'))
    import ps_noise_model as M
    c = M.coeffs(64)
    x = np.arange(-126, 64) / 128.0
    ref = np.polynomial.chebyshev.chebval(x, np.concatenate([[c[0] / 2], c[1:]]))
    for ev in (M.engine_eval, M.openfhe_eval):
        out = ev(c, x, M.Noisy(0.0, None, None), {})
        assert np.max(np.abs(out - ref)) < 1e-12
    assert M.compute_degrees_ps(6510) == (52, 7)


# ------------------------------------------------------------ DirectSort ---
def sort_cfg(N):
    return (3, 2, 2) if N <= 16 else (3, 3, 2) if N <= 128 else (3, 4, 2) if N <= 512 else (3, 5, 2)


@pytest.mark.parametrize('N', [4, 8, 16, 32])
def test_direct_sort(N):
    # tests/DirectSortTest.cpp:90-170 at ring 2^12 (reference: 2^17)
    depth, rots = O.size_parameters(N)
    c = O.Context(12, depth, 40, 60, 3, seed=200 + N)
    c.gen_rotation_keys(rots)
    x = np.random.default_rng(N).permutation(N) / N
    out = c.direct_sort(c.encrypt(x, N), N, rots, sort_cfg(N))
    y = c.decrypt(out)
    assert np.max(np.abs(y - np.sort(x))) < 0.01
    assert out.level == depth  # EXPECT_EQ(level, multDepth), DirectSortTest.cpp:128


def test_direct_sort_multi_batch():
    # N=64 at ring 2^11: num_partition=16, 4 comparator batches
    N = 64
    depth, rots = O.size_parameters(N)
    c = O.Context(11, depth, 40, 60, 3, seed=7)
    c.gen_rotation_keys(rots)
    x = np.random.default_rng(64).permutation(N) / N
    y = c.decrypt(c.direct_sort(c.encrypt(x, N), N, rots, sort_cfg(N)))
    assert np.max(np.abs(y - np.sort(x))) < 0.01


def test_construct_rank_and_index_check():
    # tests/DirectSortNTest.cpp:61-285 (ranks, exact-rank and noisy-rank index check)
    N = 8
    depth, rots = O.size_parameters(N)
    c = O.Context(12, depth, 40, 60, 3, seed=9)
    c.gen_rotation_keys(rots)
    x = np.random.default_rng(3).permutation(N) / N
    ct = c.encrypt(x, N)
    ranks = np.array([np.sum(x < v) for v in x], dtype=float)
    r = c.decrypt(c.direct_sort(ct, N, rots, (3, 2, 2), mode=1))
    assert np.max(np.abs(r - ranks)) < 1e-4
    for noise in (0.0, 1e-3):
        noisy = ranks + np.random.default_rng(5).uniform(-noise, noise, N)
        out = c.direct_sort(ct, N, rots, (3, 2, 2), mode=2, rank=c.encrypt(noisy, N))
        assert np.max(np.abs(c.decrypt(out) - np.sort(x))) < 0.01


def test_rotation_noise_is_unbiased():
    """ModDown rounds (centred exact conversion): a rotation adds noise of the
    order of the fresh noise, spread over the slots.  A flooring fast
    conversion leaves a 0..K overshoot whose product with s piles up in a few
    slots (measured before the fix: 1.3e-7 max at this size, 17x fresh)."""
    ctx = O.Context(13, 12, 40, 60, 3, seed=3)
    ctx.gen_rotation_keys([1, -1])
    x = np.random.default_rng(1).uniform(-1, 1, 4096)
    ct = ctx.encrypt_ext(x, 4096)
    fresh = np.max(np.abs(ctx.decrypt(ct) - x))
    r = ctx.rotate(ctx.rotate(ct, 1), -1)
    err = np.abs(ctx.decrypt(r) - x)
    assert err.max() < 4 * fresh and err.max() < 2e-8, (err.max(), fresh)
    assert err.max() < 12 * np.sqrt(np.mean(err ** 2))  # no outlier slots


def test_floor_moddown_is_the_biased_form():
    """The oracle's switch to OpenFHE's ApproxModDown (the flooring fast base
    conversion, Context.set_moddown_floor; verdict r5 item 7) restores the biased
    0..K overshoot the centred form removed: the same rotation pair at the same
    keys then errs several times more, in a few outlier slots."""
    ctx = O.Context(13, 12, 40, 60, 3, seed=3)
    ctx.gen_rotation_keys([1, -1])
    x = np.random.default_rng(1).uniform(-1, 1, 4096)
    ct = ctx.encrypt_ext(x, 4096)
    errs = {}
    for floor in (0, 1):
        ctx.set_moddown_floor(floor)
        r = ctx.rotate(ctx.rotate(ct, 1), -1)
        errs[floor] = np.abs(ctx.decrypt(r) - x)
    ctx.set_moddown_floor(0)
    assert errs[1].max() > 3 * errs[0].max(), (errs[1].max(), errs[0].max())
    with pytest.raises(ValueError):
        ctx.set_moddown_floor(2)


def test_floor_moddown_at_baseline_config2():
    """What the exact centred ModDown buys at the hot path's own configuration:
    BASELINE config 2 (DirectSort N=128, ring 2^16, depth 30, 40-bit scaling,
    CompositeSign(3,3,2)) sorted by the CPU oracle with both ModDown forms on the
    same keys and input (tests/golden/make_floor_moddown.py, 169 s on 8 threads,
    committed as floor_moddown.json).  The centred form meets DirectSortTest's 0.01
    bound (tests/DirectSortTest.cpp:169) at output level == multDepth; the flooring
    form -- OpenFHE's ApproxModDown, every other part of this build's numeric spec
    unchanged -- misses it.  (That is this spec with a flooring ModDown, not
    OpenFHE itself, which is absent: SURVEY §8(c).)"""
    with open(os.path.join(GOLD, 'floor_moddown.json')) as f:
        rec = json.load(f)
    cfg = rec['config']
    assert (cfg['N'], cfg['log_ring'], cfg['depth'], cfg['scale_bits'], cfg['sign']) == (128, 16, 30, 40, [3, 3, 2])
    assert (cfg['depth'], len(O.size_parameters(128)[1])) == O.size_parameters(128)[0:1] + (30,)
    runs = {r['floor']: r for r in rec['runs']}
    assert runs[0]['passes'] and runs[0]['max_abs_err'] < 0.01 and runs[0]['level'] == 30
    assert not runs[1]['passes'] and runs[1]['max_abs_err'] >= 0.01
    assert runs[1]['max_abs_err'] > 100 * runs[0]['max_abs_err']


def test_encrypt_ext_lowers_fresh_noise():
    ctx = O.Context(12, 6, 40, 60, 3, seed=3)
    x = np.random.default_rng(1).uniform(-1, 1, 2048)
    a, b = ctx.encrypt(x, 2048), ctx.encrypt_ext(x, 2048)
    assert a.level == 0 and b.level == 1 and b.info()['scale'] == ctx.delta[1]
    assert np.max(np.abs(ctx.decrypt(b) - x)) * 5 < np.max(np.abs(ctx.decrypt(a) - x))


def test_direct_sort_ties_follow_the_plaintext_model():
    """Verdict r4 item 1: what the reference's DirectSort does on tied inputs
    (tests/tie_model.py): compare(x, x) = 1/2, so a value of odd multiplicity m
    lands m times over in its middle slot and an even multiplicity spreads with
    sinc tails.  The oracle's decryption equals the plaintext model to CKKS
    precision at N = 8 with the CLI's CompositeSign(4, 3, 3); the output is not
    the sort of the input."""
    import tie_model as T
    N, cfg = 8, (4, 3, 3)
    rots = O.size_parameters(N)[1]
    orc = O.Context(12, 39, 50, 60, 3, seed=5)
    orc.gen_rotation_keys(rots)
    for x in ([0.5, 0.25, 0.5, 0.75, 0.25, 0.25, 0.1, 0.9], [0.3, 0.3, 0.3, 0.6, 0.6, 0.1, 0.2, 0.2]):
        x = np.array(x)
        y = orc.decrypt(orc.direct_sort(orc.encrypt(x, N), N, rots, cfg))[:N]
        m = T.direct_sort(x, cfg)
        assert np.max(np.abs(y - m)) < 1e-5
        assert np.max(np.abs(y - np.sort(x))) > 0.1  # ties: not a sort
    r = T.ranks([0.5, 0.25, 0.5, 0.75, 0.25, 0.25, 0.1, 0.9], cfg)
    assert np.allclose(r, [4.5, 2, 4.5, 6, 2, 2, 0, 7], atol=1e-9)
    # distinct values: the model is the sort
    x = np.random.default_rng(3).permutation(N) / N
    assert np.max(np.abs(T.direct_sort(x, cfg) - np.sort(x))) < 1e-9
