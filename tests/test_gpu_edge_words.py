"""Edge words.  Every other GPU test feeds the kernels uniform-random residues;
an off-by-one in a conditional subtract, or a sum that overflows only at
maximal inputs, survives such data.  Here every limb carries a chosen pattern:
all q - 1 and alternating 0 / q - 1 (every lazy accumulator at its bound),
floor(q / 2) and floor(q / 2) + 1 (the sign boundary of the centred lifts:
ew_lift_centered, the fused rescale), 0, single spikes and a ramp -- through
the raw NTT, ModUp / ModDown and the ciphertext ops, word for word against the
CPU oracle, in a tidy 40-bit context and in a 41-bit one whose prime classes
interleave (tests/test_gpu_mixed_classes.py).  A ciphertext made of such words
decrypts to nothing meaningful, so only the words are compared.
"""
import numpy as np
import pytest

import fhesort as F
import pyoracle as O
from test_gpu_parity import same

pytestmark = pytest.mark.gpu


def _spike(n, at, v):
    x = np.zeros(n, dtype=np.uint64)
    x[at] = v
    return x


PATTERNS = {
    'zero': lambda q, n: np.zeros(n, dtype=np.uint64),
    'q-1': lambda q, n: np.full(n, q - 1, dtype=np.uint64),
    'alt 0/q-1': lambda q, n: np.where(np.arange(n) % 2 == 0, 0, q - 1).astype(np.uint64),
    'q/2': lambda q, n: np.full(n, q // 2, dtype=np.uint64),
    'q/2+1': lambda q, n: np.full(n, q // 2 + 1, dtype=np.uint64),
    'one at 0': lambda q, n: _spike(n, 0, 1),
    'q-1 at n-1': lambda q, n: _spike(n, n - 1, q - 1),
    'ramp': lambda q, n: (np.arange(n, dtype=np.uint64) % np.uint64(q)),
}
NAMES = list(PATTERNS)


def limbs_of(name, primes, n):
    return np.stack([PATTERNS[name](int(q), n) for q in primes])


@pytest.fixture(scope='module', params=[40, 41], ids=['scale40', 'scale41'])
def pair(request):
    bits = request.param
    orc = O.Context(12, 12, bits, 60, 3, seed=bits)
    orc.gen_rotation_keys([1])
    gpu = F.Context(12, 12, bits, 60, 3, seed=bits, keygen=False)
    gpu.load_keys_from(orc, [1])
    assert np.array_equal(orc.primes, gpu.primes)
    return orc, gpu


def test_ntt_edge_words(pair):
    orc, gpu = pair
    fp = [i for i, q in enumerate(orc.primes) if int(q) < 2 ** 41]
    for pi in (fp[-1], 0, orc.nq + orc.K - 1):  # an FP prime, q_0, a special prime
        q = int(orc.primes[pi])
        for name in NAMES:
            x = PATTERNS[name](q, orc.n)
            assert np.array_equal(gpu.ntt(pi, x), orc.ntt(pi, x)), f'forward NTT, prime {pi}, {name}'
            assert np.array_equal(gpu.ntt(pi, x, inverse=True), orc.ntt(pi, x, inverse=True)), \
                f'inverse NTT, prime {pi}, {name}'


def test_conversion_edge_words(pair):
    orc, gpu = pair
    for name in NAMES:
        for ell in (13, 5, 1):
            d = limbs_of(name, orc.primes[:ell], orc.n)
            assert np.array_equal(orc.modup(d), gpu.modup(d)), f'modup, ell={ell}, {name}'
        for ell in (13, 5):
            x = limbs_of(name, list(orc.primes[:ell]) + list(orc.primes[orc.nq:]), orc.n)
            assert np.array_equal(orc.moddown(x), gpu.moddown(x)), f'moddown, ell={ell}, {name}'


@pytest.mark.parametrize('level', [0, 8])
def test_ciphertext_edge_words(pair, level):
    orc, gpu = pair
    pr = orc.primes[:orc.nq - level]
    cts = []
    for name in NAMES:
        w = limbs_of(name, pr, orc.n)
        data = np.stack([w, w])
        cts.append((orc.ct_from(data, level, 16), gpu.upload(data, level, 16)))
    for i, name in enumerate(NAMES):
        (oa, ga), (ob, gb) = cts[i], cts[(i + 1) % len(cts)]  # with itself and with the next pattern
        ops = [
            ('mul self', lambda: (gpu.mul(ga, ga), orc.mul(oa, oa))),
            ('mul next', lambda: (gpu.mul(ga, gb), orc.mul(oa, ob))),
            ('square', lambda: (gpu.square(ga), orc.square(oa))),
            ('rescale', lambda: (gpu.rescale(gpu.mul_int(ga, 7)), orc.rescale(orc.mul_int(oa, 7)))),
            ('rotate', lambda: (gpu.rotate(ga, 1), orc.rotate(oa, 1))),
            ('add self', lambda: (gpu.add(ga, ga), orc.add(oa, oa))),
            ('add next', lambda: (gpu.add(ga, gb), orc.add(oa, ob))),
            ('sub self', lambda: (gpu.sub(ga, ga), orc.sub(oa, oa))),
            ('sub next', lambda: (gpu.sub(ga, gb), orc.sub(oa, ob))),
            ('negate', lambda: (gpu.negate(ga), orc.negate(oa))),
            ('mul_int', lambda: (gpu.mul_int(ga, -3), orc.mul_int(oa, -3))),
        ]
        for what, op in ops:
            g, o = op()
            try:
                same(g, o)
            except AssertionError as e:
                raise AssertionError(f'{what}, {name}, level {level}: {e}')
