"""Interleaved prime classes on the GPU.

The engine splits every limb list by prime class: primes below 2^41 run the
fp64 butterflies and the fp64 conversions ("FP"), the others the integer
kernels.  With 40-, 50- or 59-bit scaling primes the classes form three tidy
runs (q_0, the scaling primes, the special primes).  A 41-bit scale takes its
primes alternately above and below 2^41, so the classes interleave, which
drives the code for more than two runs per class: the extra launches of
ntt.hip launch_pass and the two-run NttFuse::limb_of, ntt_class_runs and the
run-pair loops of engine.hip mul_tail and modup, ntt_row_ks over interleaved
targets, integer targets in the middle of the fp64 conversions' target chunks,
and the per-limb constants of the fused NTT epilogues.  The depth-50 context
also builds the halfway-reduction (MID = 1) tables of the fp64 conversions
unforced (tests/test_conv_fp.py pins those tables on the host), and all of
them put FP primes right under 2^41, the top of the range the fp64 butterflies
claim.

Everything is compared word for word with the CPU oracle on identical keys.
Ciphertexts at a level are encrypted at that level or built from words
(ct_from / upload), so no test pays for a product chain on the CPU.
"""
import numpy as np
import pytest

import fhesort as F
import pyoracle as O
from test_gpu_parity import _Hip, same

pytestmark = pytest.mark.gpu

FP_BOUND = 1 << 41


def make_pair(logN, L, rots, seed):
    orc = O.Context(logN, L, 41, 60, 3, seed=seed)
    if rots:
        orc.gen_rotation_keys(rots)
    gpu = F.Context(logN, L, 41, 60, 3, seed=seed, keygen=False)
    gpu.load_keys_from(orc, rots)
    return orc, gpu


ROTS12 = [1, -3, 5]
ROTS50 = [1, -3]


@pytest.fixture(scope='module')
def pair12():
    return make_pair(12, 12, ROTS12, 41)


@pytest.fixture(scope='module')
def pair50():
    return make_pair(12, 50, ROTS50, 50)


@pytest.fixture(scope='module')
def pair16():
    return make_pair(16, 12, [], 16)


@pytest.fixture(scope='module')
def pair17():
    return make_pair(17, 8, [], 17)


def class_runs(primes):
    """(FP runs, integer runs) of a prime list, each a list of (start, length)"""
    runs = ([], [])
    for z, q in enumerate(primes):
        r = runs[0 if int(q) < FP_BOUND else 1]
        if r and r[-1][0] + r[-1][1] == z:
            r[-1] = (r[-1][0], r[-1][1] + 1)
        else:
            r.append((z, 1))
    return runs


def rand_limbs(rng, primes, n):
    return np.stack([rng.integers(0, int(q), size=n, dtype=np.uint64) for q in primes])


def rand_ct(orc, gpu, rng, level, slots=16):
    """the same ciphertext of uniform words at `level` on both sides"""
    pr = orc.primes[:orc.nq - level]
    data = np.stack([rand_limbs(rng, pr, orc.n), rand_limbs(rng, pr, orc.n)])
    return orc.ct_from(data, level, slots), gpu.upload(data, level, slots)


def check_conversions(orc, gpu, rng, ells):
    for ell in ells:
        d = rand_limbs(rng, orc.primes[:ell], orc.n)
        assert np.array_equal(orc.modup(d), gpu.modup(d)), f'modup differs at ell={ell}'
        x = rand_limbs(rng, list(orc.primes[:ell]) + list(orc.primes[orc.nq:]), orc.n)
        assert np.array_equal(orc.moddown(x), gpu.moddown(x)), f'moddown differs at ell={ell}'


def tagged(what, fn):
    try:
        fn()
    except AssertionError as e:
        raise AssertionError(f'{what}: {e}')


@pytest.mark.parametrize('name', ['pair12', 'pair50', 'pair16', 'pair17'])
def test_classes_interleave(name, request):
    """The precondition of every test below: the same primes on both sides, and
    among the Q primes at least three separate runs of each class.  A prime
    generator that made these contexts tidy again must fail here."""
    orc, gpu = request.getfixturevalue(name)
    assert np.array_equal(orc.primes, gpu.primes)
    fp, integer = class_runs(gpu.primes[:gpu.nq])
    assert len(fp) >= 3 and len(integer) >= 3, (fp, integer)
    assert all(int(q) >= FP_BOUND for q in gpu.primes[gpu.nq:])  # the special primes: integer


# ------------------------------------------------------ ring 2^12, depth 12 --
def test_ntt_every_prime(pair12):
    orc, gpu = pair12
    rng = np.random.default_rng(1)
    for pi, q in enumerate(orc.primes):
        x = rng.integers(0, int(q), size=orc.n, dtype=np.uint64)
        f_g = gpu.ntt(pi, x)
        assert np.array_equal(orc.ntt(pi, x), f_g), f'forward NTT differs, prime {pi}'
        assert np.array_equal(gpu.ntt(pi, f_g, inverse=True), x), f'inverse NTT does not round-trip, prime {pi}'


def test_ntt_batched_over_runs(pair12):
    """All Q limbs in one call: each pass takes one launch per pair of runs of a
    class (ntt.hip launch_pass), more than the two launches of a tidy context."""
    orc, gpu = pair12
    rng = np.random.default_rng(2)
    x = rand_limbs(rng, orc.primes[:orc.nq], orc.n)
    with F.KernelClock(gpu) as clk:
        g = gpu.ntt(0, x)
    for i in range(orc.nq):
        assert np.array_equal(g[i], orc.ntt(i, x[i])), f'limb {i}'
    assert np.array_equal(gpu.ntt(0, g, inverse=True), x)
    fp, integer = class_runs(orc.primes[:orc.nq])
    per_pass = (len(fp) + 1) // 2 + (len(integer) + 1) // 2
    assert per_pass > 2
    launches = sum(v['launches'] for k, v in clk.stats.items() if k.startswith('k_ntt_fwd'))
    assert launches == 2 * per_pass, sorted(clk.stats)


def test_ntt_on_device_memory(pair12):
    """fhe_ntt_dev over primes 1..L of two segments (a limb map offset into the
    context's, every run of both classes)"""
    orc, gpu = pair12
    hip = _Hip()
    n, first, limbs, segs = gpu.n, 1, gpu.nq - 1, 2
    rng = np.random.default_rng(3)
    x = np.stack([rand_limbs(rng, gpu.primes[first:first + limbs], n) for _ in range(segs)])
    want = np.stack([np.stack([orc.ntt(first + i, x[s, i]) for i in range(limbs)]) for s in range(segs)])
    dev = hip.upload(x)
    try:
        gpu.ntt_dev(dev, first, limbs, segments=segs, seg_stride=limbs * n)
        gpu.sync()
        assert np.array_equal(hip.download(dev, x), want)
        gpu.ntt_dev(dev, first, limbs, inverse=True, segments=segs, seg_stride=limbs * n)
        gpu.sync()
        assert np.array_equal(hip.download(dev, x), x)
    finally:
        hip.h.hipFree(hip.C.c_void_p(dev))


def test_conversions(pair12):
    orc, gpu = pair12
    assert (orc.alpha, orc.K) == (5, 4)
    check_conversions(orc, gpu, np.random.default_rng(4), (13, 10, 6, 5, 2, 1))


@pytest.mark.parametrize('level', [0, 3, 7, 11])
def test_ciphertext_ops(pair12, level):
    orc, gpu = pair12
    L = orc.L
    rng = np.random.default_rng(100 + level)
    a, b = rng.uniform(-1, 1, 16), rng.uniform(-1, 1, 16)
    oa, ob = orc.encrypt(a, 16, level), orc.encrypt(b, 16, level)
    ga, gb = gpu.from_oracle(oa), gpu.from_oracle(ob)
    assert oa.level == level and oa.info()['limbs'] == orc.nq - level
    om, gm = orc.mul(oa, ob), gpu.mul(ga, gb)
    tagged('mul', lambda: same(gm, om))
    assert np.max(np.abs(gpu.decrypt(gm) - orc.decrypt(om))) < 1e-9
    tagged('square', lambda: same(gpu.square(ga), orc.square(oa)))
    tagged('rescale', lambda: same(gpu.rescale(gpu.mul_int(ga, 7)), orc.rescale(orc.mul_int(oa, 7))))
    for k in ROTS12:
        tagged(f'rotate {k}', lambda: same(gpu.rotate(ga, k), orc.rotate(oa, k)))
    for h, k in zip(gpu.rotate_hoisted(ga, ROTS12 + [0]), ROTS12 + [0]):
        tagged(f'hoisted {k}', lambda: same(h, orc.rotate(oa, k) if k else oa))
    p = orc.encode(b, 16, level)
    tagged('mul_plain', lambda: same(gpu.mul_plain(ga, gpu.upload_pt(p.data(), level, 16)), orc.mul_plain(oa, p)))
    # a level mismatch is adjusted identically
    oo = orc.encrypt(b, 16, level - 1) if level else orc.mul_const(ob, 0.5)
    go = gpu.from_oracle(oo)
    assert abs(oo.level - level) == 1
    tagged('add', lambda: same(gpu.add(ga, go), orc.add(oa, oo)))
    cs, target = [0.25, -1.5, 3.0], max(level, oo.level) + 1
    tagged('linear_sum_to', lambda: same(gpu.linear_sum_to([ga, go, ga], cs, target),
                                         orc.linear_sum_to([oa, oo, oa], cs, target)))
    for deg in (7, 27):
        if level + O.cheb_ps_depth(deg) > L:
            continue
        c = np.random.default_rng(deg).normal(size=deg + 1) / (1 + np.arange(deg + 1))
        oy, gy = orc.cheb(oa, c), gpu.cheb(ga, c)
        tagged(f'cheb {deg}', lambda: same(gy, oy))
        assert np.max(np.abs(gpu.decrypt(gy) - orc.decrypt(oy))) < 1e-9


def test_product_chain(pair12):
    """four real products down the chain (the fused rescale of real products)"""
    orc, gpu = pair12
    rng = np.random.default_rng(5)
    oa, ob = orc.encrypt(rng.uniform(-1, 1, 8), 8), orc.encrypt(rng.uniform(-1, 1, 8), 8)
    oc, gc, gb = oa, gpu.from_oracle(oa), gpu.from_oracle(ob)
    for i in range(4):
        oc, gc = orc.mul(oc, ob), gpu.mul(gc, gb)
        tagged(f'product {i}', lambda: same(gc, oc))
    assert np.max(np.abs(gpu.decrypt(gc) - orc.decrypt(oc))) < 1e-9


@pytest.mark.parametrize('level', [0, 5])
def test_stack_of_three(pair12, level):
    orc, gpu = pair12
    rng = np.random.default_rng(6 + level)
    oxs = [orc.encrypt(rng.uniform(-0.9, 0.9, 16), 16, level) for _ in range(3)]
    gxs = [gpu.from_oracle(o) for o in oxs]
    S, one = gpu.stack(gxs), gxs[1]
    c = np.linspace(1, 0.1, 28)
    cases = [
        ('mul stacked', lambda g: gpu.mul(g, gpu.stack(gxs[::-1])), lambda m: orc.mul(oxs[m], oxs[2 - m])),
        ('mul broadcast', lambda g: gpu.mul(g, one), lambda m: orc.mul(oxs[m], oxs[1])),
        ('rotate', lambda g: gpu.rotate(g, -3), lambda m: orc.rotate(oxs[m], -3)),
        ('cheb27', lambda g: gpu.cheb(g, c), lambda m: orc.cheb(oxs[m], c)),
    ]
    for name, gop, oop in cases:
        R = gop(S)
        for m in range(3):
            tagged(f'{name}, member {m}', lambda: same(gpu.member(R, m), oop(m)))


# ------------------------------------- ring 2^12, depth 50: the MID = 1 tables --
def test_conversions_mid1(pair50):
    """full and partial digits of alpha = 17 sources, K = 13 special primes"""
    orc, gpu = pair50
    assert (orc.alpha, orc.K) == (17, 13)
    check_conversions(orc, gpu, np.random.default_rng(7), (51, 34, 29, 18, 17, 7))


@pytest.mark.parametrize('level', [0, 20, 40, 48])
def test_products_and_rotations_mid1(pair50, level):
    orc, gpu = pair50
    rng = np.random.default_rng(200 + level)
    (oa, ga), (ob, gb) = rand_ct(orc, gpu, rng, level), rand_ct(orc, gpu, rng, level)
    with F.KernelClock(gpu) as clk:
        gm = gpu.mul(ga, gb)
    # k_moddown_rescale_fp<K, MID, TPI, I32>: the fp64 ModDown + rescale ran, in
    # its halfway-reduction form
    assert any(k.startswith('k_moddown_rescale_fp<13, 1, ') for k in clk.stats), sorted(clk.stats)
    tagged('mul', lambda: same(gm, orc.mul(oa, ob)))
    for k in ROTS50:
        tagged(f'rotate {k}', lambda: same(gpu.rotate(ga, k), orc.rotate(oa, k)))


def test_real_product_mid1(pair50):
    orc, gpu = pair50
    rng = np.random.default_rng(8)
    oa, ob = orc.encrypt(rng.uniform(-1, 1, 16), 16), orc.encrypt(rng.uniform(-1, 1, 16), 16)
    om, gm = orc.mul(oa, ob), gpu.mul(gpu.from_oracle(oa), gpu.from_oracle(ob))
    same(gm, om)
    assert np.max(np.abs(gpu.decrypt(gm) - orc.decrypt(om))) < 1e-9


# ------------------------------------------------------ rings 2^16 and 2^17 --
def stacked_products(orc, gpu, rng, count, level):
    """a `count`-member stacked product at `level`, every member against the
    oracle; returns the kernels that ran"""
    pairs = [rand_ct(orc, gpu, rng, level, 64) for _ in range(2 * count)]
    xs, ys = pairs[:count], pairs[count:]
    with F.KernelClock(gpu) as clk:
        st = gpu.mul(gpu.stack([g for _, g in xs]), gpu.stack([g for _, g in ys]))
    for m in range(count):
        tagged(f'{count} members at level {level}, member {m}',
               lambda: same(gpu.member(st, m), orc.mul(xs[m][0], ys[m][0])))
    return clk.stats


@pytest.mark.parametrize('count,level', [(4, 0), (5, 0), (5, 6)])
def test_fused_row_pass_interleaved_targets(pair16, count, level):
    """Stacks of >= 4 members at ring 2^16 relinearise through dev::ntt_row_ks
    (ModUp's row pass fused with the key-switch inner product), one launch per
    pair of target runs of a class: full blocks of 4 members x 4 rows, and a
    partial block."""
    orc, gpu = pair16
    stats = stacked_products(orc, gpu, np.random.default_rng(300 + 10 * count + level), count, level)
    assert any(k.startswith('k_ntt_row_ks') for k in stats), sorted(stats)


def test_single_products_ring16(pair16):
    orc, gpu = pair16
    rng = np.random.default_rng(9)
    oa, ob = orc.encrypt(rng.uniform(-1, 1, 64), 64), orc.encrypt(rng.uniform(-1, 1, 64), 64)
    ga, gb = gpu.from_oracle(oa), gpu.from_oracle(ob)
    om, gm = orc.mul(oa, ob), gpu.mul(ga, gb)
    tagged('mul', lambda: same(gm, om))
    assert np.max(np.abs(gpu.decrypt(gm) - orc.decrypt(om))) < 1e-9
    tagged('square', lambda: same(gpu.square(ga), orc.square(oa)))


def test_ring17(pair17):
    orc, gpu = pair17
    rng = np.random.default_rng(10)
    oa = orc.encrypt(rng.uniform(-1, 1, 64), 64)
    tagged('square', lambda: same(gpu.square(gpu.from_oracle(oa)), orc.square(oa)))
    stats = stacked_products(orc, gpu, rng, 4, 0)
    assert any(k.startswith('k_ntt_row_ks') for k in stats), sorted(stats)
