"""The CPU oracle against the exact big-integer model (tests/bigint_model.py).

The GPU suite compares the engine word for word with the oracle, and the
oracle was written from the same specification as the engine: a reading of
DESIGN.md §2 that both share is green everywhere.  The model restates that
section in Python integers -- ModUp, ModDown, rescale, ModRaise, the key
switch and the ops built from them -- and this file holds the oracle to it
word for word on a machine without a GPU (tests/test_gpu_bigint_model.py does
the same for the engine):

  * random inputs: NTT at every prime, ModUp / ModDown / rescale at full,
    partial and one-limb levels, mul, square, rotations (single and hoisted),
    conjugate, mul_plain.  Every such test first asserts that the model saw
    no ModDown tie (bigint_model's tau), then compares with array_equal;
  * boundary inputs built by the model in coefficient form: the rescale's
    and ModRaise's cut at (q -+ 1)/2, ModDown's at X_P near P/2 (exact cases
    far outside tau, and true ties (P -+ 1)/2 where either candidate counts);
  * the exact worst-case noise bound of a rotation and of a product, also on
    the three wide-digit contexts of test_wide_digits_match_oracle.
"""
import json
import os

import numpy as np
import pytest

import bigint_model as M
import pyoracle as O

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ROTS = [1, -3]

# ring 2^11 L=5 at 40 bits; the 41-bit context of test_gpu_mixed_classes.py (its
# prime classes interleave); 59-bit scaling primes as test_gpu_parity.py's pair59
CONTEXTS = {'scale40': (11, 5, 40, 60, 3, 7), 'scale41': (12, 12, 41, 60, 3, 41), 'scale59': (11, 5, 59, 60, 3, 12)}


def model_of(orc):
    return M.Model(orc.logN, orc.primes, orc.nq, orc.K, orc.alpha, orc.ntt)


@pytest.fixture(scope='module', params=list(CONTEXTS))
def pair(request):
    logN, L, bits, first, dnum, seed = CONTEXTS[request.param]
    orc = O.Context(logN, L, bits, first, dnum, seed=seed)
    orc.gen_rotation_keys(ROTS)
    orc.gen_galois_keys([2 * orc.n - 1])
    return orc, model_of(orc)


def no_ties(ties):
    assert len(ties) == 0, f'{len(ties)} ModDown ties on random input'


# ------------------------------------------------------ the model itself ---
def test_model_ntt_is_the_direct_evaluation():
    """ring 2^6: the staged transform equals A[k] = a(psi^(2 brev(k) + 1))
    evaluated term by term, its inverse inverts it, and the negacyclic product
    through it is the golden vectors' (tests/golden/make_golden.py)."""
    case = [c for c in json.load(open(os.path.join(GOLD, 'ntt_golden.json'))) if c['logN'] == 6][0]
    orc = O.Context(6, 1, 40, 60, 3, seed=1, keygen=False)
    m = model_of(orc)
    assert m.q[0] == int(case['q']) and m.psi[0] == int(case['psi'])
    a = np.array([int(v) for v in case['a']], dtype=object)
    b = np.array([int(v) for v in case['b']], dtype=object)
    A = m.fwd(0, a)
    assert list(A) == list(m.fwd_naive(0, a)) == [int(v) for v in case['ntt_a']]
    assert list(m.inv(0, A)) == list(a)
    assert list(m.inv(0, A * m.fwd(0, b) % m.q[0])) == [int(v) for v in case['negacyclic_ab']]


def test_model_automorphism_index_map():
    """the NTT-domain index map the model's key switch uses is the coefficient
    automorphism X -> X^g with X^n = -1 (and the golden vectors')"""
    orc = O.Context(6, 1, 40, 60, 3, seed=1, keygen=False)
    m = model_of(orc)
    rng = np.random.default_rng(6)
    a = M.obj(rng.integers(0, m.q[0], size=m.n, dtype=np.uint64))
    for g in (5, 25, 3, 2 * m.n - 1, M.galois_of_rotation(6, -3)):
        assert list(m.fwd(0, M.automorph_coeff(a, g, m.q[0]))) == list(m.fwd(0, a)[m.ntt_perm(g)]), g
    for case in json.load(open(os.path.join(GOLD, 'automorph_golden.json'))):
        if case['logN'] == 6:
            assert M.galois_of_rotation(6, case['k']) == case['galois']
            got = M.automorph_coeff([int(v) for v in case['a']], case['galois'], int(case['q']))
            assert list(got) == [int(v) for v in case['sigma_a']]


# --------------------------------------------------------- random inputs ---
def test_ntt_every_prime(pair):
    orc, m = pair
    rng = np.random.default_rng(1)
    for i, q in enumerate(m.q):
        x = rng.integers(0, q, size=m.n, dtype=np.uint64)
        assert np.array_equal(M.u64(m.fwd(i, x)), orc.ntt(i, x)), f'forward, prime {i}'
        assert np.array_equal(M.u64(m.inv(i, x)), orc.ntt(i, x, inverse=True)), f'inverse, prime {i}'


def test_modup(pair):
    orc, m = pair
    rng = np.random.default_rng(2)
    for ell in sorted({m.nq, m.nq - 1, m.alpha + 1, m.alpha, 1}, reverse=True):
        d = M.rand_limbs(rng, m.q[:ell], m.n)
        assert np.array_equal(m.modup(d), orc.modup(d)), f'ell={ell}'


def test_moddown(pair):
    orc, m = pair
    rng = np.random.default_rng(3)
    m.closest = 1.0
    for ell in (m.nq, 2, 1):
        x = M.rand_limbs(rng, m.q[:ell] + m.q[m.nq:], m.n)
        want, ties = m.moddown(x)
        no_ties(ties)
        assert np.array_equal(want, orc.moddown(x)), f'ell={ell}'
    print(f'closest |2 X_P - P| / P on random input: {m.closest:.3e}; tau = {M.tau_num(m.K) / 2 ** 53:.3e}')


def test_rescale(pair):
    orc, m = pair
    rng = np.random.default_rng(4)
    for ell in (m.nq, 2):
        data = np.stack([M.rand_limbs(rng, m.q[:ell], m.n) for _ in range(2)])
        got = orc.rescale(orc.ct_from(data, m.nq - ell, 8))
        assert np.array_equal(m.rescale(data), got.data()), f'ell={ell}'


def test_ops(pair):
    orc, m = pair
    rng = np.random.default_rng(5)
    va, vb = rng.uniform(-1, 1, 8), rng.uniform(-1, 1, 8)
    oa, ob = orc.encrypt(va, 8), orc.encrypt(vb, 8)
    a, b, relin = oa.data(), ob.data(), orc.relin_key()
    m.closest = 1.0
    for what, (want, ties), got in [
        ('mul', m.mul(a, b, relin), orc.mul(oa, ob)),
        ('square', m.square(a, relin), orc.square(oa)),
        ('rotate 1', m.rotate(a, 1, orc.rot_key(1)[1]), orc.rotate(oa, 1)),
        ('rotate -3', m.rotate(a, -3, orc.rot_key(-3)[1]), orc.rotate(oa, -3)),
        ('conjugate', m.conjugate(a, orc.galois_key(2 * m.n - 1)), orc.conjugate(oa)),
    ]:
        no_ties(ties)
        assert np.array_equal(want, got.data()), what
    for (want, ties), got in zip(m.rotate_hoisted(a, ROTS, [orc.rot_key(k)[1] for k in ROTS]),
                                 orc.rotate_hoisted(oa, ROTS)):
        no_ties(ties)
        assert np.array_equal(want, got.data()), 'hoisted'
    p = orc.encode(vb, 8, 0)
    assert np.array_equal(m.mul_plain(a, p.data()), orc.mul_plain(oa, p).data()), 'mul_plain + rescale'
    print(f'closest |2 X_P - P| / P in the ops: {m.closest:.3e}; tau = {M.tau_num(m.K) / 2 ** 53:.3e}')


# ------------------------------------------------------- boundary inputs ---
def test_rescale_boundary(pair):
    """the last limb's coefficients at 0, 1, (q_l - 1)/2, (q_l + 1)/2, q_l - 1:
    an integer compare, so exact equality, through rescale and through mul
    (operands built so that the product's pre-rescale last limb is that limb)"""
    orc, m = pair
    rng = np.random.default_rng(6)
    for ell in (m.nq, 2):
        level = m.nq - ell
        data = M.rescale_boundary_ct(m, rng, ell)
        assert np.array_equal(m.rescale(data), orc.rescale(orc.ct_from(data, level, 8)).data()), f'rescale, ell={ell}'
        a, b, ks = M.mul_boundary_operands(m, rng, ell, orc.relin_key())
        no_ties(ks[1])
        want, _ = m.mul(a, b, None, ks=ks)
        got = orc.mul(orc.ct_from(a, level, 8), orc.ct_from(b, level, 8))
        assert np.array_equal(want, got.data()), f'mul, ell={ell}'


def test_moddown_boundary_exact(pair):
    """X_P = floor(P (1/2 -+ 2^-30)), floor(P (1/2 -+ 2^-45)), 0, 1, P - 1: the
    sign boundary of the centred conversion, all far outside tau: exact"""
    orc, m = pair
    rng = np.random.default_rng(7)
    assert 2.0 ** -44 > 4 * M.tau_num(m.K) / 2 ** 53
    XP = M.blocks(M.moddown_exact_values(m.P), m.n)
    for ell in (m.nq, 2):
        x = M.moddown_input(m, rng, ell, XP)
        want, ties = m.moddown(x)
        no_ties(ties)
        assert np.array_equal(want, orc.moddown(x)), f'ell={ell}'


def test_moddown_boundary_ties(pair):
    """X_P = (P - 1)/2 and (P + 1)/2 at known coefficients: there, and only
    there, either candidate is accepted; every other coefficient is exact"""
    orc, m = pair
    rng = np.random.default_rng(8)
    for ell in (m.nq, 2):
        x, idx = M.moddown_tie_input(m, rng, ell)
        M.check_moddown_ties(m, x, orc.moddown(x), idx)


def test_mod_raise_boundary():
    """bootstrap stage 4 is the bare centred lift of the one limb left (oracle_core.cpp
    mod_raise; the scale adjustment and the trace are other stages): pinned at
    0, 1, (q_0 - 1)/2, (q_0 + 1)/2, q_0 - 1 like the rescale"""
    orc = O.Context(11, 24, 59, 60, 3, seed=61, keygen=False)
    m = model_of(orc)
    B = O.Bootstrapper(orc, 8, (2, 2), keygen=False)
    w = M.u64(m.fwd(0, M.blocks(M.lift_boundary_values(m.q[0]), m.n)))
    data = np.stack([w, M.u64(m.fwd(0, M.blocks(M.lift_boundary_values(m.q[0])[::-1], m.n, 7)))])[:, None, :]
    got = B.mod_raise(orc.ct_from(data, orc.L, 8))
    assert got.info()['limbs'] == m.nq
    assert np.array_equal(m.mod_raise(data), got.data())


# ------------------------------------------------------------ exact noise ---
def test_noise_bounds(pair):
    """worst-case bounds from the spec (derivations in bigint_model.check_*):
    fails if P is too small for a digit, which word parity cannot see"""
    orc, m = pair
    rng = np.random.default_rng(9)
    oa, ob = orc.encrypt(rng.uniform(-1, 1, 8), 8), orc.encrypt(rng.uniform(-1, 1, 8), 8)
    s = orc.secret_coeff()
    g = M.galois_of_rotation(m.logN, 1)
    got, bound = M.check_rotate_noise(m, oa.data(), orc.rotate(oa, 1).data(), g, s)
    print(f'rotation noise 2^{got:.1f}, bound 2^{bound:.1f}')
    got, bound = M.check_mul_noise(m, oa.data(), ob.data(), orc.mul(oa, ob).data(), s)
    print(f'product noise 2^{got:.1f}, bound 2^{bound:.1f}')


# --------------------------------------------- constants and their sums ---
def test_scaled_const_definition():
    """(k, sh) from the definition: exact rounding half away from zero up to
    2^62 in magnitude, above it 62 leading bits and a shift"""
    assert M.scaled_const(0.0) == (0, 0)
    assert M.scaled_const(2.5) == (3, 0) and M.scaled_const(-2.5) == (-3, 0)
    assert M.scaled_const(0.5) == (1, 0) and M.scaled_const(-0.5) == (-1, 0)
    assert M.scaled_const(0.49999999999999994) == (0, 0)
    assert M.scaled_const(2.0 ** 53 + 2) == (2 ** 53 + 2, 0)      # no floating-point + 0.5
    assert M.scaled_const(2.0 ** 62) == (2 ** 62, 0) and M.scaled_const(-2.0 ** 62) == (-2 ** 62, 0)
    assert M.scaled_const(2.0 ** 63) == (2 ** 62, 1)
    assert M.scaled_const(-3.0 * 2.0 ** 100) == (-3 * 2 ** 60, 40)
    rng = np.random.default_rng(10)
    for x in np.ldexp(rng.uniform(-1, 1, 200), rng.integers(40, 140, 200)):
        k, sh = M.scaled_const(x)
        assert abs(k) <= 2 ** 62 and sh >= 0
        assert abs(k * 2 ** sh - int(x)) <= 2 ** sh // 2 + 1, x
        if sh:
            assert abs(k) > 2 ** 60, x
    q = (1 << 60) - 93
    assert M.const_residue(-1, 0, q) == q - 1
    assert M.const_residue(-2 ** 62, 7, q) == (-(2 ** 69)) % q


def half_constant(scale):
    """a double c with c * scale = k + 1/2 exactly (rounds away from zero)"""
    for k in range(1, 4000):
        c = (k + 0.5) / scale
        if c * scale == k + 0.5:
            return c, k
    raise AssertionError('no constant lands on a half at this scale')


PATTERNS = {
    'zero': lambda q, n: np.zeros(n, dtype=np.uint64),
    'q-1': lambda q, n: np.full(n, q - 1, dtype=np.uint64),
    'alt 0/q-1': lambda q, n: np.where(np.arange(n) % 2 == 0, 0, q - 1).astype(np.uint64),
    'q/2': lambda q, n: np.full(n, q // 2, dtype=np.uint64),
    'q/2+1': lambda q, n: np.full(n, q // 2 + 1, dtype=np.uint64),
    'ramp': lambda q, n: (np.arange(n, dtype=np.uint64) % np.uint64(q)),
}


def pattern_ct(name, primes, n):
    w = np.stack([PATTERNS[name](int(q), n) for q in primes])
    return np.stack([w, w[:, ::-1]])


def large_constant(m):
    """a constant whose product with a scale of this context exceeds 2^62"""
    return 1.0e7 if m.q[1] < (1 << 42) else 37.5


def test_constant_ops(pair):
    """add_const, mul_const, mul_const_to, mul_int, level_adjust, linear_sum_to and
    mul_plain_sum of the oracle against the model, on real encryptions and on
    the edge patterns; constants 0, negative, on a half, and one in the
    large-constant form (sh > 0, asserted from the model)"""
    orc, m = pair
    rng = np.random.default_rng(11)
    delta = orc.delta
    big = large_constant(m)
    assert M.const_at_scale(big, delta[0])[1] > 0 and M.const_to_target(-big, delta[2], m.q[m.nq - 2], delta[1])[1] > 0
    half, hk = half_constant(delta[1])
    assert M.const_at_scale(half, delta[1]) == (hk + 1, 0) and M.const_at_scale(-half, delta[1]) == (-hk - 1, 0)
    consts = [0.0, 1.0, -1.0, 0.37, -2.75, half, -half, big, -big]
    for level in (0, 1):
        ell = m.nq - level
        cts = [('encryption', orc.encrypt(rng.uniform(-1, 1, 8), 8, level))]
        cts += [(name, orc.ct_from(pattern_ct(name, m.q[:ell], m.n), level, 8)) for name in PATTERNS]
        for name, oa in cts:
            a, sc = oa.data(), oa.info()['scale']
            tag = f'{name}, level {level}'
            for c in consts:
                assert np.array_equal(m.add_const(a, c, sc), orc.add_const(oa, c).data()), f'add_const {c}, {tag}'
                assert np.array_equal(m.mul_const(a, c, sc, level, delta), orc.mul_const(oa, c).data()), \
                    f'mul_const {c}, {tag}'
            for c in (0.37, -big):
                assert np.array_equal(m.mul_const_to(a, c, sc, level + 2, delta),
                                      orc.mul_const_to(oa, c, level + 2).data()), f'mul_const_to {c}, {tag}'
            for k in (0, 1, -1, 7, -3, 2 ** 62, -2 ** 62, 2 ** 40 + 1):
                assert np.array_equal(m.mul_int(a, k), orc.mul_int(oa, k).data()), f'mul_int {k}, {tag}'
            for t in (level, level + 1, level + 3):
                assert np.array_equal(m.level_adjust(a, sc, level, t, delta), orc.level_adjust(oa, t).data()), \
                    f'level_adjust to {t}, {tag}'
        # sums over inputs of two limb counts, every pattern and the encryption together
        lo = orc.encrypt(rng.uniform(-1, 1, 8), 8, 0)
        xs = [oa for _, oa in cts] + ([lo] if level else [])
        cs = [c for c, _ in zip(consts + [0.5, -0.25], xs)]
        want = m.linear_sum_to([x.data() for x in xs], cs, [x.info()['scale'] for x in xs], level + 1, delta)
        assert np.array_equal(want, orc.linear_sum_to(xs, cs, level + 1).data()), f'linear_sum_to, level {level}'
        pts = [orc.encode(rng.uniform(-1, 1, 8), 8, level) for _ in xs[:len(cts)]]
        want = m.mul_plain_sum([oa.data() for _, oa in cts], [p.data() for p in pts])
        assert np.array_equal(want, orc.mul_plain_sum([oa for _, oa in cts], pts).data()), f'mul_plain_sum, level {level}'


def test_linear_sums_is_the_sum_of_its_rows(pair):
    """linear_sums (the GPU tests' reference for the multi-output kernels) row
    by row against the oracle's linear_sum_to, and its constant fold against
    add_const behind the rescale: the identity the fold relies on"""
    orc, m = pair
    rng = np.random.default_rng(12)
    delta, target = orc.delta, 2
    ell = m.nq - 1
    xs = [orc.encrypt(rng.uniform(-1, 1, 8), 8, lv) for lv in (1, 1, 0)]
    cs = [[0.5, -1.25, 3.0], [0.0, large_constant(m), -1.0]]
    cc = [0.125, -0.7]
    ks = [[M.const_to_target(c, delta[target], m.q[ell - 1], x.info()['scale']) for c, x in zip(row, xs)] for row in cs]
    kc = [M.const_at_scale(c, delta[target]) for c in cc]
    K, sh = [[k for k, _ in r] for r in ks], [[s for _, s in r] for r in ks]
    assert any(s > 0 for r in sh for s in r)
    plain = M.linear_sums([x.data() for x in xs], K, sh, m.q[:ell])
    fold = M.linear_sums([x.data() for x in xs], K, sh, m.q[:ell], consts=([k for k, _ in kc], [s for _, s in kc]))
    for g in range(2):
        got = orc.linear_sum_to(xs, cs[g], target)
        assert np.array_equal(m.rescale(plain[g]), got.data()), f'row {g}'
        assert np.array_equal(fold[g][:, ell - 1], plain[g][:, ell - 1]), 'the fold touches the last limb'
        assert np.array_equal(m.rescale(fold[g]), orc.add_const(got, cc[g]).data()), f'row {g} with its constant'


# ------------------------------------------- the int32 budget of the rows ---
def test_row_budget_bounds():
    """the number that bounds the sources of one leaf-sum launch (LEAF_M = 64)"""
    assert M.budget_bound_window(64) == 1682964480 < 2 ** 31
    assert M.budget_bound_fold(64) == 1917968384 < 2 ** 31
    assert M.budget_bound_window(72) < 2 ** 31 <= M.budget_bound_window(82) and M.budget_bound_window(81) < 2 ** 31
    assert M.budget_bound_fold(71) < 2 ** 31 <= M.budget_bound_fold(72)
    # a single row, which the MFMA accumulates in int32 as well
    assert 64 * 911 * 128 < 2 ** 31


ALL_MINUS_128_60 = 15 * 2 ** 56 - 0x80808080808080
ALL_MINUS_128_40 = 2 ** 40 - 0x8080808080


@pytest.mark.parametrize('q', [(1 << 60) - 93, (1 << 59) - 55, (1 << 40) + 294913, (1 << 41) - 21],
                         ids=['60bit', '59bit', '40bit', '41bit'])
def test_rows_recombine_to_the_exact_sum(q):
    """the identity each kernel relies on, with its correction term (C0 sum c,
    128 sum d), on random and on targeted words; every combined word inside the
    proven bound; the targeted words reach further than random ones"""
    rng = np.random.default_rng(q % 1000)
    m, n = 17, 96
    assert M.balanced_digits(ALL_MINUS_128_60) == [-128] * 7 + [15]
    assert M.balanced_digits(ALL_MINUS_128_40) == [-128] * 5 + [1, 0, 0]
    special = ALL_MINUS_128_60 if q > ALL_MINUS_128_60 else ALL_MINUS_128_40
    assert special < q
    res = [[int(v) for v in rng.integers(0, q, size=m)], [special] * m, [q - 1] * m, [0] + [1] * (m - 1)]
    ys = rng.integers(0, q, size=(m, n), dtype=np.uint64)
    ys[:, 0], ys[:, 1] = q - 1, 0
    for form in ('window', 'fold'):
        tw, triples = M.target_words(form, res, q, n)
        assert int(tw.max()) < q
        for g, r in enumerate(res):
            reach = []
            for words in (ys, tw):
                exact = sum(M.obj(words[i]) * r[i] for i in range(m))
                if form == 'window':
                    rows, comb = M.rows_window(r, words)
                    assert np.all(M.recombine_window(rows, r) == exact), (form, g)
                    assert int(np.abs(comb).max()) <= M.budget_bound_window(m)
                else:
                    rows, comb = M.rows_fold(r, words, q)
                    assert np.all((M.recombine_fold(rows, r, q) - exact) % q == 0), (form, g)
                    assert int(np.abs(comb).max()) <= M.budget_bound_fold(m)
                reach.append(int(np.abs(comb).max()))
            if g == 0:
                assert reach[1] > 2 * reach[0], (form, reach)
    # zero words against the all -128 digits: a row of exactly 7 2^14 m (60-bit) in the window form
    if q > (1 << 59):
        rows, _ = M.rows_window([ALL_MINUS_128_60] * m, np.zeros((m, 1), dtype=np.uint64))
        assert int(rows.max()) == 7 * 2 ** 14 * m


@pytest.mark.parametrize('L,alpha,K', [(65, 22, 16), (61, 21, 15), (50, 17, 12)])
def test_wide_digits_rotation(L, alpha, K):
    """the three wide-digit contexts of test_wide_digits_match_oracle at ring
    2^11: one rotation, word for word and within the noise bound"""
    orc = O.Context(11, L, 40, 60, 3, seed=L)
    orc.gen_rotation_keys([1])
    assert (orc.alpha, orc.K) == (alpha, K)
    m = model_of(orc)
    oa = orc.encrypt(np.random.default_rng(L).uniform(-1, 1, 16), 16)
    got = orc.rotate(oa, 1).data()
    want, ties = m.rotate(oa.data(), 1, orc.rot_key(1)[1])
    no_ties(ties)
    assert np.array_equal(want, got)
    noise, bound = M.check_rotate_noise(m, oa.data(), got, M.galois_of_rotation(11, 1), orc.secret_coeff())
    print(f'L={L}: rotation noise 2^{noise:.1f}, bound 2^{bound:.1f}')
