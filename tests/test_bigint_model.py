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
