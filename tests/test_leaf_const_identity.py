"""The identity behind the folded leaf constants (Engine::linear_sums_to's
consts), in the exact big-integer model of tests/bigint_model.py:

    rescale(x with K q_last mod q_l added to every word of limb l < ell - 1)
        ==  rescale(x) with K mod q_l added to every word of limb l,

word for word.  A constant is the same word in every evaluation slot; the
rescale subtracts the lift of the last limb, which the added term does not
touch, and multiplies by q_last^-1, which turns K q_last into K.  Random small
RNS bases (a model of its own: the root psi of each prime is found here, nothing
comes from the oracle or the engine), random K, K < 0, K >= q_l, K = 0 and
multiples of q_last.  CPU only."""
import numpy as np
import pytest

import bigint_model as M

LOGN = 3


def is_prime(n):
    if n < 2:
        return False
    small = (2, 3, 5, 7, 11, 13, 17, 19, 23, 29, 31, 37)
    for p in small:
        if n % p == 0:
            return n == p
    d, s = n - 1, 0
    while d % 2 == 0:
        d, s = d // 2, s + 1
    for a in small:  # deterministic below 3.3e24
        x = pow(a, d, n)
        if x in (1, n - 1):
            continue
        for _ in range(s - 1):
            x = x * x % n
            if x == n - 1:
                break
        else:
            return False
    return True


def random_base(rng, ell):
    """ell distinct primes = 1 mod 2n of 17 to 45 bits, and a primitive 2n-th root of each"""
    two_n = 2 << LOGN
    primes, roots = [], []
    while len(primes) < ell:
        bits = int(rng.integers(17, 46))
        q = (int(rng.integers(1 << (bits - 1), 1 << bits)) // two_n) * two_n + 1
        if q in primes or not is_prime(q):
            continue
        for g in range(2, 1000):
            psi = pow(g, (q - 1) // two_n, q)
            if pow(psi, two_n // 2, q) == q - 1:
                break
        else:
            continue
        primes.append(q)
        roots.append(psi)
    return primes, roots


def constants(rng, primes):
    ql, big = primes[-1], max(primes)
    ks = [0, 1, -1, ql, -ql, 3 * ql + 5, -(3 * ql + 5), big, big + 1, -(big + 1), (1 << 62) - 1, -(1 << 62) + 1]
    ks += [int(rng.integers(-(1 << 62), 1 << 62)) for _ in range(4)]
    ks += [int(rng.integers(-(1 << 20), 1 << 20)) for _ in range(2)]
    return ks


@pytest.mark.parametrize('seed', range(6))
def test_constant_before_rescale_equals_constant_after(seed):
    rng = np.random.default_rng(9100 + seed)
    ell = int(rng.integers(2, 7))  # ell = 2: the only target is q_0
    primes, roots = random_base(rng, ell)

    def ntt(i, x):  # the model reads psi as ntt(i, X)[0] and defines the transform from it
        return np.array([roots[i]] + [0] * (len(x) - 1), dtype=np.uint64)

    m = M.Model(LOGN, primes, ell, 0, 1, ntt)
    ql = primes[-1]
    x = M.rand_limbs(rng, primes, m.n)
    plain = m.rescale_poly(x)
    seen_negative = seen_large = False
    for K in constants(rng, primes):
        seen_negative |= K < 0
        seen_large |= K >= min(primes)
        y = x.copy()
        for l in range(ell - 1):
            q = primes[l]
            y[l] = M.u64((M.obj(x[l]) + (K % q) * (ql % q) % q) % q)
        before = m.rescale_poly(y)
        for l in range(ell - 1):
            q = primes[l]
            after = M.u64((M.obj(plain[l]) + K % q) % q)
            assert np.array_equal(before[l], after), (seed, primes, K, l)
    assert seen_negative and seen_large
