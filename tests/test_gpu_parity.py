"""GPU parity: every engine op is bit-exact with the CPU oracle on identical
keys and inputs, and decrypts within the reference tests' tolerances.

All calls go through the C ABI (include/fhe_gpu.h) via fhesort.py.
"""
import os

import numpy as np
import pytest

import fhesort as F
import pyoracle as O

pytestmark = pytest.mark.gpu

ROTS = [1, 2, 3, -1, -4, 5, 8, 16]


@pytest.fixture(scope='module')
def pair():
    orc = O.Context(12, 12, 40, 60, 3, seed=5)
    orc.gen_rotation_keys(ROTS)
    gpu = F.Context(12, 12, 40, 60, 3, seed=5, keygen=False)
    gpu.load_keys_from(orc, ROTS)
    return orc, gpu


def same(gct, oct_):
    gi, oi = gct.info(), oct_.info()
    assert gi['level'] == oi['level'] and gi['slots'] == oi['slots'] and gi['limbs'] == oi['limbs']
    assert gi['scale'] == oi['scale']
    gd, od = gct.data(), oct_.data()
    assert gd.shape == od.shape
    if not np.array_equal(gd, od):
        bad = np.argwhere(gd != od)
        raise AssertionError(f'{len(bad)} limb words differ, first at {bad[0].tolist()}')


def test_params_identical(pair):
    orc, gpu = pair
    assert np.array_equal(orc.primes, gpu.primes)
    assert np.array_equal(orc.delta, gpu.delta)


@pytest.mark.parametrize('logN', [12, 13, 16, 17])
def test_ntt_matches_oracle(logN):
    orc = O.Context(logN, 3, 40, 60, 3, seed=1, keygen=False)
    gpu = F.Context(logN, 3, 40, 60, 3, seed=1, keygen=False)
    rng = np.random.default_rng(logN)
    for pi in range(len(orc.primes)):
        q = int(orc.primes[pi])
        x = rng.integers(0, q, size=orc.n, dtype=np.uint64)
        f_o = orc.ntt(pi, x)
        f_g = gpu.ntt(pi, x)
        assert np.array_equal(f_o, f_g), f'forward NTT differs, prime {pi}'
        assert np.array_equal(gpu.ntt(pi, f_g, inverse=True), x), 'inverse NTT does not round-trip'


def test_ntt_batched_limbs():
    gpu = F.Context(16, 6, 40, 60, 3, seed=1, keygen=False)
    orc = O.Context(16, 6, 40, 60, 3, seed=1, keygen=False)
    rng = np.random.default_rng(3)
    x = np.stack([rng.integers(0, int(q), size=gpu.n, dtype=np.uint64) for q in gpu.primes[:5]])
    g = gpu.ntt(0, x)
    for i in range(5):
        assert np.array_equal(g[i], orc.ntt(i, x[i]))


class _Hip:
    """device buffers and a stream through the HIP runtime the engine loaded
    (libamdhip64; torch's own HIP runtime cannot share this process)"""

    def __init__(self):
        import ctypes as C
        self.C = C
        self.h = C.CDLL('libamdhip64.so')
        self.h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.h.hipFree.argtypes = [C.c_void_p]
        self.h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        self.h.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
        self.h.hipStreamSynchronize.argtypes = [C.c_void_p]
        self.h.hipStreamDestroy.argtypes = [C.c_void_p]

    def upload(self, a):
        p = self.C.c_void_p()
        assert self.h.hipMalloc(self.C.byref(p), a.nbytes) == 0
        assert self.h.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p.value

    def download(self, p, like):
        out = np.empty_like(like)
        assert self.h.hipMemcpy(out.ctypes.data, self.C.c_void_p(p), out.nbytes, 2) == 0
        return out

    def stream(self):
        s = self.C.c_void_p()
        assert self.h.hipStreamCreate(self.C.byref(s)) == 0
        return s.value


@pytest.mark.parametrize('logN', [12, 16])
def test_ntt_and_automorph_on_device_memory(logN):
    """fhe_ntt_dev / fhe_automorph_dev: limbs in device memory,
    primes 1..4 of 2 segments, on a caller's stream and on the context stream,
    no host round trip -- the same words as the oracle's NTT; the inverse
    restores the input; an automorphism equals the index permutation."""
    orc = O.Context(logN, 5, 40, 60, 3, seed=1, keygen=False)
    gpu = F.Context(logN, 5, 40, 60, 3, seed=1, keygen=False)
    hip = _Hip()
    n, first, limbs, segs = gpu.n, 1, 4, 2
    rng = np.random.default_rng(logN)
    x = np.stack([np.stack([rng.integers(0, int(gpu.primes[first + i]), size=n, dtype=np.uint64)
                            for i in range(limbs)]) for _ in range(segs)])  # [seg][limb][n]
    want = np.stack([np.stack([orc.ntt(first + i, x[s_, i]) for i in range(limbs)]) for s_ in range(segs)])
    dev = hip.upload(x)
    st = hip.stream()
    gpu.ntt_dev(dev, first, limbs, segments=segs, seg_stride=limbs * n, stream=st)
    assert hip.h.hipStreamSynchronize(hip.C.c_void_p(st)) == 0
    assert np.array_equal(hip.download(dev, x), want)
    gpu.ntt_dev(dev, first, limbs, inverse=True, segments=segs, seg_stride=limbs * n)  # context stream
    gpu.sync()
    assert np.array_equal(hip.download(dev, x), x)
    g = O.galois(logN, 3)
    src = hip.upload(np.ascontiguousarray(want[0]))
    dst = hip.upload(np.zeros_like(want[0]))
    gpu.automorph_dev(src, limbs, g, dst, stream=st)
    assert hip.h.hipStreamSynchronize(hip.C.c_void_p(st)) == 0
    assert np.array_equal(hip.download(dst, want[0]), want[0][:, O.automorph_perm(logN, g)])
    with pytest.raises(F.FheError):
        gpu.ntt_dev(dev, gpu.nq + gpu.K - 1, 2)  # one prime beyond the context's
    for p in (dev, src, dst):
        hip.h.hipFree(hip.C.c_void_p(p))
    hip.h.hipStreamDestroy(hip.C.c_void_p(st))


def test_encrypt_decrypt_and_upload(pair):
    orc, gpu = pair
    x = np.linspace(-1, 1, 16)
    c = orc.encrypt(x, 16)
    g = gpu.from_oracle(c)
    same(g, c)
    assert np.max(np.abs(gpu.decrypt(g) - x)) < 1e-6


def test_elementwise_ops(pair):
    orc, gpu = pair
    rng = np.random.default_rng(0)
    a, b = rng.uniform(-1, 1, 8), rng.uniform(-1, 1, 8)
    oa, ob = orc.encrypt(a, 8), orc.encrypt(b, 8)
    ga, gb = gpu.from_oracle(oa), gpu.from_oracle(ob)
    same(gpu.add(ga, gb), orc.add(oa, ob))
    same(gpu.sub(ga, gb), orc.sub(oa, ob))
    same(gpu.negate(ga), orc.negate(oa))
    same(gpu.add_const(ga, 0.375), orc.add_const(oa, 0.375))
    same(gpu.mul_int(ga, -3), orc.mul_int(oa, -3))
    same(gpu.mul_const(ga, -2.5), orc.mul_const(oa, -2.5))
    same(gpu.mul_const_to(ga, 1.25, 3), orc.mul_const_to(oa, 1.25, 3))
    same(gpu.level_adjust(ga, 2), orc.level_adjust(oa, 2))
    same(gpu.rescale(gpu.mul_int(ga, 7)), orc.rescale(orc.mul_int(oa, 7)))
    p = orc.encode(b, 8, 0)
    gp = gpu.upload_pt(p.data(), 0, 8)
    same(gpu.mul_plain(ga, gp), orc.mul_plain(oa, p))
    same(gpu.add_plain(ga, gp), orc.add_plain(oa, p))
    # level mismatch is adjusted identically
    m = orc.mul_const(oa, 0.5)
    same(gpu.add(gpu.from_oracle(m), gb), orc.add(m, ob))


def test_relinearised_products(pair):
    orc, gpu = pair
    rng = np.random.default_rng(1)
    a, b = rng.uniform(-1, 1, 8), rng.uniform(-1, 1, 8)
    oa, ob = orc.encrypt(a, 8), orc.encrypt(b, 8)
    ga, gb = gpu.from_oracle(oa), gpu.from_oracle(ob)
    om, gm = orc.mul(oa, ob), gpu.mul(ga, gb)
    same(gm, om)
    assert np.max(np.abs(gpu.decrypt(gm) - a * b)) < 1e-6
    same(gpu.square(ga), orc.square(oa))
    # chained products down the modulus chain
    oc, gc = oa, ga
    for _ in range(4):
        oc, gc = orc.mul(oc, ob), gpu.mul(gc, gb)
    same(gc, oc)


def test_rotations(pair):
    orc, gpu = pair
    x = np.arange(16, dtype=float) / 16
    ox = orc.encrypt(x, 16)
    gx = gpu.from_oracle(ox)
    for k in [1, 2, 3, -1, -4, 5, 8]:
        gr = gpu.rotate(gx, k)
        same(gr, orc.rotate(ox, k))
        assert np.max(np.abs(gpu.decrypt(gr) - np.roll(x, -k))) < 1e-6
    hs = gpu.rotate_hoisted(gx, [1, 2, 3, 0])
    for h, k in zip(hs, [1, 2, 3, 0]):
        same(h, orc.rotate(ox, k) if k else ox)
    with pytest.raises(F.NoKeyError):
        gpu.rotate(gx, 7)


TREE_ROTS = [-1, -2, -4, -8, -16, -32, 1, 2, 4, 8, 16, 32, 64, 512]  # tests/RotationTest.cpp:43


def test_rotation_tree():
    """RotationTest.RotateTreeVector (tests/RotationTest.cpp:77-108): RotationTree<8>
    with NAF, treeRotate(ct, r) for r in [-4, 4] equals the rotated input (the
    reference's 1e-6), and word for word the oracle's chain of single rotations
    along the same NAF path (hoisted == single rotation).  The tree is built over
    [-8, 8]: buildTree(start, end) decomposes with wrapN = end while treeRotate uses
    the ciphertext's slots (src/rotation.h:275,284), so the reference's
    buildTree(-4, 4) leaves e.g. the path of -3 at 8 slots ([4, 1]) unbuilt."""
    orc = O.Context(12, 3, 40, 60, 3, seed=12)
    orc.gen_rotation_keys(TREE_ROTS)
    gpu = F.Context(12, 3, 40, 60, 3, seed=12, keygen=False)
    gpu.load_keys_from(orc, TREE_ROTS)
    x = np.arange(1.0, 9.0)
    ox = orc.encrypt(x, 8)
    gx = gpu.from_oracle(ox)
    tree = gpu.rotation_tree(8, TREE_ROTS, 0)
    tree.build(-8, 8)
    for r in range(-4, 5):
        got = tree.rotate(gx, r)
        ref = ox
        for v, step in F.decompose(8, TREE_ROTS, r, 8, 0):
            if v:
                ref = orc.rotate(ref, step)
        same(got, ref)
        assert np.max(np.abs(gpu.decrypt(got) - np.roll(x, -r))) < 1e-6, r
    st = tree.stats()
    assert st['cache_hits'] > 0 and st['fast'] == st['total'] > 0


def test_modup_moddown(pair):
    orc, gpu = pair
    rng = np.random.default_rng(2)
    for ell in (13, 9, 5, 1):
        d = np.stack([rng.integers(0, int(q), size=orc.n, dtype=np.uint64) for q in orc.primes[:ell]])
        eo, eg = orc.modup(d), gpu.modup(d)
        assert np.array_equal(eo, eg), f'modup differs at ell={ell}'
        x = np.stack([rng.integers(0, int(q), size=orc.n, dtype=np.uint64)
                      for q in list(orc.primes[:ell]) + list(orc.primes[orc.nq:])])
        assert np.array_equal(orc.moddown(x), gpu.moddown(x)), f'moddown differs at ell={ell}'


def test_automorphism(pair):
    orc, gpu = pair
    rng = np.random.default_rng(4)
    x = np.stack([rng.integers(0, int(q), size=orc.n, dtype=np.uint64) for q in orc.primes[:3]])
    for k in (1, 5, -1):
        g = O.galois(12, k)
        perm = O.automorph_perm(12, g)
        assert np.array_equal(gpu.automorph(x, g), x[:, perm])


def test_linear_sum_mixed_levels(pair):
    orc, gpu = pair
    rng = np.random.default_rng(5)
    xs = [orc.encrypt(rng.uniform(-1, 1, 8), 8) for _ in range(3)]
    xs[1] = orc.mul_const(xs[1], 1.0)  # level 1
    gx = [gpu.from_oracle(x) for x in xs]
    cs = [0.25, -1.5, 3.0]
    same(gpu.linear_sum_to(gx, cs, 3), orc.linear_sum_to(xs, cs, 3))


@pytest.mark.parametrize('split', [F.PS_SPLIT_OPENFHE, F.PS_SPLIT_ENGINE])
@pytest.mark.parametrize('deg', [1, 3, 7, 27, 70, 119, 200])
def test_chebyshev_ps(deg, split):
    """evalChebyshevSeriesPS under both Paterson-Stockmeyer splits (OpenFHE's
    (k, m) long division -- the default -- and the power-of-two one): word for
    word equal to the oracle, same output level (the depth OpenFHE consumes),
    within 1e-5 of the plain series."""
    L = 10 if deg <= 119 else 11
    orc = O.Context(12, L, 40, 60, 3, seed=9, ps_split=split)
    gpu = F.Context(12, L, 40, 60, 3, seed=9, keygen=False, ps_split=split)
    gpu.load_keys_from(orc)
    x = np.linspace(-1, 1, 16)
    ox = orc.encrypt(x, 16)
    c = np.random.default_rng(deg).normal(size=deg + 1) / (1 + np.arange(deg + 1))
    oy = orc.cheb(ox, c)
    gy = gpu.cheb(gpu.from_oracle(ox), c)
    same(gy, oy)
    assert gy.level == O.cheb_ps_depth(deg, split)
    ref = np.polynomial.chebyshev.chebval(x, np.concatenate([[c[0] / 2], c[1:]]))
    assert np.max(np.abs(gpu.decrypt(gy) - ref)) < 1e-5


@pytest.mark.parametrize('split', [F.PS_SPLIT_OPENFHE, F.PS_SPLIT_ENGINE])
def test_doubled_sinc_ps_bit_exact(split):
    """The N=128 doubled-sinc series (degree 848, src/sort_algo.h:725-728) on the
    index-check grid x = j/(2N): both splits word-identical to the oracle at ring
    2^12, and the OpenFHE split at least as precise as the power-of-two one."""
    N = 128
    c = np.fromfile(os.path.join(F.COEFF_DIR, f'doubled_sinc_{N}.f64'))
    orc = O.Context(12, 12, 40, 60, 3, seed=21, ps_split=split)
    gpu = F.Context(12, 12, 40, 60, 3, seed=21, keygen=False, ps_split=split)
    gpu.load_keys_from(orc)
    x = np.resize(np.arange(-(2 * N - 2), N) / (2 * N), 1024)
    ox = orc.encrypt(x, 1024)
    gy = gpu.cheb(gpu.from_oracle(ox), c)
    same(gy, orc.cheb(ox, c))
    assert gy.level == 10  # OpenFHE's depth for degree 848 (ComputeDegreesPS: k = 28, m = 5)
    ref = np.polynomial.chebyshev.chebval(x, np.concatenate([[c[0] / 2], c[1:]]))
    err = np.max(np.abs(gpu.decrypt(gy) - ref))
    assert err < (2e-5 if split == F.PS_SPLIT_OPENFHE else 1e-3)


def test_composite_sign_and_compare():
    # tests/SignTest.cpp:41-80 and tests/CompareTest.cpp:43-63 (see test_oracle for tolerances)
    orc = O.Context(12, 30, 40, 60, 3, seed=11)
    gpu = F.Context(12, 30, 40, 60, 3, seed=11, keygen=False)
    gpu.load_keys_from(orc)
    x = np.array([0.5, -0.3, 0.1, -0.7, 0.0, 0.8, -0.9, 0.2])
    ox = orc.encrypt(x, 8)
    gx = gpu.from_oracle(ox)
    same(gpu.sign(gx, 3, 0, 1), orc.sign(ox, 3, 0, 1))
    a = orc.encrypt([0.1, 0.5, 0.3, 0.4], 4)
    b = orc.encrypt([0.2, 0.4, 0.3, 0.3], 4)
    gc = gpu.compare(gpu.from_oracle(a), gpu.from_oracle(b), 3, 3, 2)
    same(gc, orc.compare(a, b, 3, 3, 2))
    assert np.allclose(gpu.decrypt(gc), [0, 1, 0.5, 1], atol=0.1)
    gi = gpu.indicator(gpu.from_oracle(a), 0.05, 3, 2, 1)
    same(gi, orc.indicator(a, 0.05, 3, 2, 1))


@pytest.fixture(scope='module')
def pair59():
    """CompareTest's context (tests/CompareTest.cpp:13-22): depth 50, 59-bit
    scaling primes; ring 2^12 here (the reference's ring is chosen by OpenFHE);
    dnum 4 keeps digits within the engine's 16 primes."""
    orc = O.Context(12, 50, 59, 60, 4, seed=12)
    gpu = F.Context(12, 50, 59, 60, 4, seed=12, keygen=False)
    gpu.load_keys_from(orc)
    return orc, gpu


def test_composite_sign4_bit_exact(pair59):
    """compositeSign<4>(3, 3) (src/sign.cpp:62-158: g4 = degree-27 Chebyshev PS,
    f4 = degree 15), the reference CLI's sign (src/sort.h:76-95) and SignTest's
    small inputs (tests/SignTest.cpp:82-122, within 0.1)."""
    orc, gpu = pair59
    x = np.array([0.02, -0.02, 0.01, -0.01, 0.009, -0.009, 1, -1])
    ox = orc.encrypt(x, 8)
    gy = gpu.sign(gpu.from_oracle(ox), 4, 3, 3)
    same(gy, orc.sign(ox, 4, 3, 3))
    assert np.max(np.abs(gpu.decrypt(gy) - np.sign(x))) < 0.1


def test_compare_vectors_scale59_bit_exact(pair59):
    """CompareTest's vectors with compositeSign(4, 3, 3) at 59-bit scaling
    (tests/CompareTest.cpp:43-63): [1,5,3,4] vs [2,4,3,3] -> [0,1,0.5,1] +- 0.1.
    The 59-bit scale makes f4's and g3's constants exceed 2^62 (mantissa +
    power-of-two path of host::SConst)."""
    orc, gpu = pair59
    a = orc.encrypt([1.0, 5.0, 3.0, 4.0], 4)
    b = orc.encrypt([2.0, 4.0, 3.0, 3.0], 4)
    gc = gpu.compare(gpu.from_oracle(a), gpu.from_oracle(b), 4, 3, 3)
    same(gc, orc.compare(a, b, 4, 3, 3))
    assert np.max(np.abs(gpu.decrypt(gc) - [0.0, 1.0, 0.5, 1.0])) < 0.1
    x = orc.encrypt([0.5, -0.3, 0.1, -0.7], 4)
    gs = gpu.sign(gpu.from_oracle(x), 3, 2, 2)  # g3's 25614/1024 at 2^59 > 2^63
    same(gs, orc.sign(x, 3, 2, 2))


def test_keygen_and_encrypt_parity():
    """GPU key generation + encryption == oracle's for the same seed (bit-exact)."""
    orc = O.Context(12, 6, 40, 60, 3, seed=77)
    orc.gen_rotation_keys([1, 3])
    gpu = F.Context(12, 6, 40, 60, 3, seed=77)
    gpu.gen_rotation_keys([1, 3])
    x = np.linspace(-0.5, 0.5, 8)
    oc, gc = orc.encrypt(x, 8), gpu.encrypt(x, 8)
    same(gc, oc)
    same(gpu.mul(gc, gc), orc.mul(oc, oc))
    same(gpu.rotate(gc, 3), orc.rotate(oc, 3))
    assert np.max(np.abs(orc.decrypt(orc.ct_from(gc.data(), 0, 8)) - x)) < 1e-6


@pytest.mark.parametrize('N,cfg', [(4, (3, 2, 2)), (8, (3, 2, 2)), (16, (3, 2, 2))])
def test_direct_sort_bit_exact(N, cfg):
    depth, rots = O.size_parameters(N)
    assert F.size_parameters(N) == (depth, rots)
    orc = O.Context(12, depth, 40, 60, 3, seed=100 + N)
    orc.gen_rotation_keys(rots)
    gpu = F.Context(12, depth, 40, 60, 3, seed=100 + N, keygen=False)
    gpu.load_keys_from(orc, rots)
    x = np.random.default_rng(20250704).permutation(N) / N
    ox = orc.encrypt(x, N)
    gx = gpu.from_oracle(ox)
    gout = gpu.direct_sort(gx, N, rots, cfg)
    oout = orc.direct_sort(ox, N, rots, cfg)
    same(gout, oout)
    y = gpu.decrypt(gout)
    assert np.max(np.abs(y - np.sort(x))) < 0.01
    assert gout.level == depth  # EXPECT_EQ(level, multDepth), tests/DirectSortTest.cpp:128


def test_batched_ops_match_members(pair):
    """A stacked ciphertext batch gives, member by member, exactly the oracle's
    single-ciphertext result for every op the sort path uses."""
    orc, gpu = pair
    rng = np.random.default_rng(3)
    oxs = [orc.encrypt(rng.uniform(-0.9, 0.9, 16), 16) for _ in range(3)]
    S = gpu.stack([gpu.from_oracle(o) for o in oxs])
    one = gpu.from_oracle(oxs[1])
    pt_vals = rng.uniform(-1, 1, 16)
    cases = [
        ('square', lambda g: gpu.square(g), lambda o: orc.square(o)),
        ('mul_self', lambda g: gpu.mul(g, g), lambda o: orc.mul(o, o)),
        ('mul_bcast', lambda g: gpu.mul(g, one), lambda o: orc.mul(o, oxs[1])),
        ('rotate', lambda g: gpu.rotate(g, 3), lambda o: orc.rotate(o, 3)),
        ('hoisted', lambda g: gpu.rotate_hoisted(g, [1, -4])[1], lambda o: orc.rotate_hoisted(o, [1, -4])[1]),
        ('add_const', lambda g: gpu.add_const(g, 0.375), lambda o: orc.add_const(o, 0.375)),
        ('mul_const', lambda g: gpu.mul_const(g, -1.25), lambda o: orc.mul_const(o, -1.25)),
        ('mul_const_to', lambda g: gpu.mul_const_to(g, 0.5, 3), lambda o: orc.mul_const_to(o, 0.5, 3)),
        ('add', lambda g: gpu.add(g, g), lambda o: orc.add(o, o)),
        ('negate', lambda g: gpu.negate(g), lambda o: orc.negate(o)),
        ('lin', lambda g: gpu.linear_sum_to([g, gpu.square(g)], [0.5, -2.0], 2),
         lambda o: orc.linear_sum_to([o, orc.square(o)], [0.5, -2.0], 2)),
        ('mul_plain', lambda g: gpu.mul_plain(g, gpu.encode(pt_vals, 16, 0)),
         lambda o: orc.mul_plain(o, orc.encode(pt_vals, 16, 0))),
        ('cheb27', lambda g: gpu.cheb(g, np.linspace(1, 0.1, 28)), lambda o: orc.cheb(o, np.linspace(1, 0.1, 28))),
        ('mul_plain_sum',
         lambda g: gpu.mul_plain_sum([g, gpu.rotate(g, 1)], [gpu.encode(pt_vals, 16, 0), gpu.encode(-pt_vals, 16, 0)]),
         lambda o: orc.mul_plain_sum([o, orc.rotate(o, 1)], [orc.encode(pt_vals, 16, 0), orc.encode(-pt_vals, 16, 0)])),
        ('sign', lambda g: gpu.sign(g, 3, 1, 1), lambda o: orc.sign(o, 3, 1, 1)),
    ]
    for name, gop, oop in cases:
        R = gop(S)
        for m, o in enumerate(oxs):
            try:
                same(gpu.member(R, m), oop(o))
            except AssertionError as e:
                raise AssertionError(f'{name}, member {m}: {e}')
    total = gpu.sum_members(S)
    ref = orc.add(orc.add(oxs[0], oxs[1]), oxs[2])
    same(total, ref)


@pytest.mark.parametrize('stack,lanes', [(32, 1), (3, 1), (32, 2), (1, 3)])
def test_direct_sort_multi_batch_stacked(stack, lanes):
    """N=64 at ring 2^11: 4 comparator batches and 4 index-check batches run
    stacked (all four at once, or 3 + 1) on one or more concurrent lanes
    (forked engines on their own streams) and match the oracle's serial loop."""
    N, cfg = 64, (3, 3, 2)
    depth, rots = O.size_parameters(N)
    orc = O.Context(11, depth, 40, 60, 3, seed=7)
    orc.gen_rotation_keys(rots)
    gpu = F.Context(11, depth, 40, 60, 3, seed=7, keygen=False)
    gpu.load_keys_from(orc, rots)
    gpu.set_sort_stack(stack)
    gpu.set_sort_lanes(lanes)
    x = np.random.default_rng(64).permutation(N) / N
    ox = orc.encrypt(x, N)
    gx = gpu.from_oracle(ox)
    grank = gpu.direct_sort(gx, N, rots, cfg, mode=1)
    orank = orc.direct_sort(ox, N, rots, cfg, mode=1)
    same(grank, orank)
    gout = gpu.direct_sort(gx, N, rots, cfg)
    oout = orc.direct_sort(ox, N, rots, cfg)
    same(gout, oout)
    assert np.max(np.abs(gpu.decrypt(gout) - np.sort(x))) < 0.01


def test_ps_split_change_reaches_cached_lanes():
    """the sorters cache forked lane engines; switching the
    Paterson-Stockmeyer split after a sort must reach them too (the split is
    shared by an engine and its forks), so a second sort on two lanes matches
    the oracle under the new split, and switching back matches the first."""
    N, cfg = 64, (3, 3, 2)
    depth, rots = O.size_parameters(N)
    orcs = {s: O.Context(11, depth, 40, 60, 3, seed=7, ps_split=s) for s in (F.PS_SPLIT_OPENFHE, F.PS_SPLIT_ENGINE)}
    for o in orcs.values():
        o.gen_rotation_keys(rots)
    gpu = F.Context(11, depth, 40, 60, 3, seed=7, keygen=False)
    gpu.load_keys_from(orcs[F.PS_SPLIT_OPENFHE], rots)
    gpu.set_sort_stack(1)
    gpu.set_sort_lanes(2)
    x = np.random.default_rng(65).permutation(N) / N
    ox = orcs[F.PS_SPLIT_OPENFHE].encrypt(x, N)
    gx = gpu.from_oracle(ox)
    for split in (F.PS_SPLIT_OPENFHE, F.PS_SPLIT_ENGINE, F.PS_SPLIT_OPENFHE):
        gpu.set_ps_split(split)
        assert gpu.ps_split == split
        same(gpu.direct_sort(gx, N, rots, cfg), orcs[split].direct_sort(ox, N, rots, cfg))


def test_ring_2_17_ops_match_oracle():
    """Ring 2^17 (the reference's MEHP24 ring; 2^8 x 2^9 NTT passes): encryption,
    products, rescales, rotations and plaintext products bit-exact."""
    orc = O.Context(17, 5, 40, 60, 3, seed=17)
    orc.gen_rotation_keys([1, -256, 32640, -32768])
    gpu = F.Context(17, 5, 40, 60, 3, seed=17, keygen=False)
    gpu.load_keys_from(orc, [1, -256, 32640, -32768])
    rng = np.random.default_rng(17)
    x = rng.uniform(-1, 1, 1 << 16)
    o = orc.encrypt_ext(x, 1 << 16)
    g = gpu.from_oracle(o)
    for name, gop, oop in [
        ('square', lambda c: gpu.square(c), lambda c: orc.square(c)),
        ('mul_const', lambda c: gpu.mul_const(c, 0.75), lambda c: orc.mul_const(c, 0.75)),
        ('rot1', lambda c: gpu.rotate(c, 1), lambda c: orc.rotate(c, 1)),
        ('rot-256', lambda c: gpu.rotate(c, -256), lambda c: orc.rotate(c, -256)),
        ('rot32640', lambda c: gpu.rotate(c, 32640), lambda c: orc.rotate(c, 32640)),
        ('rot-32768', lambda c: gpu.rotate(c, -32768), lambda c: orc.rotate(c, -32768)),
        ('mul_plain', lambda c: gpu.mul_plain(c, gpu.encode(x, 1 << 16, 1)),
         lambda c: orc.mul_plain(c, orc.encode(x, 1 << 16, 1))),
    ]:
        try:
            same(gop(g), oop(o))
        except AssertionError as e:
            raise AssertionError(f'{name}: {e}')
    r = gpu.rotate(g, -32768)
    assert np.max(np.abs(gpu.decrypt(r) - np.roll(x, 32768))) < 1e-5


@pytest.mark.parametrize('L,alpha,K', [(65, 22, 16), (61, 21, 15), (50, 17, 12)])
def test_wide_digits_match_oracle(L, alpha, K):
    """OpenFHE's default 3 digits at the MEHP24 depths (src/mehp24 leaves the digit
    count unset): digits of 17-22 primes and up to 16 special primes, past Acc4's
    16-term sums (ModUp alpha terms, ModDown K + 1) -- ModUp / ModDown at full and
    partial digits, relinearised products down the chain, rotations, hoisted
    rotations, all word-identical to the oracle."""
    rots = [1, -3, 7]
    orc = O.Context(12, L, 40, 60, 3, seed=L)
    orc.gen_rotation_keys(rots)
    gpu = F.Context(12, L, 40, 60, 3, seed=L, keygen=False)
    gpu.load_keys_from(orc, rots)
    assert (orc.alpha, orc.K) == (alpha, K) and np.array_equal(orc.primes, gpu.primes)
    rng = np.random.default_rng(L)
    for ell in (L + 1, 2 * alpha, 2 * alpha - 5, alpha + 1, alpha, 7):
        d = np.stack([rng.integers(0, int(q), size=orc.n, dtype=np.uint64) for q in orc.primes[:ell]])
        assert np.array_equal(orc.modup(d), gpu.modup(d)), f'modup differs at ell={ell}'
        x = np.stack([rng.integers(0, int(q), size=orc.n, dtype=np.uint64)
                      for q in list(orc.primes[:ell]) + list(orc.primes[orc.nq:])])
        assert np.array_equal(orc.moddown(x), gpu.moddown(x)), f'moddown differs at ell={ell}'
    a, b = rng.uniform(-1, 1, 16), rng.uniform(-1, 1, 16)
    oa, ob = orc.encrypt(a, 16), orc.encrypt(b, 16)
    ga, gb = gpu.from_oracle(oa), gpu.from_oracle(ob)
    oc, gc = oa, ga
    for i in range(L - 2):  # every level: each digit count, full and partial last digits
        oc, gc = orc.mul(oc, ob), gpu.mul(gc, gb)
        if i % 9 == 0:
            same(gc, oc)
            for k in rots:
                same(gpu.rotate(gc, k), orc.rotate(oc, k))
    same(gc, oc)
    for h, k in zip(gpu.rotate_hoisted(ga, rots), rots):
        same(h, orc.rotate(oa, k))
    assert np.max(np.abs(gpu.decrypt(gpu.mul(ga, gb)) - a * b)) < 1e-6


@pytest.mark.parametrize('logN,L', [(16, 10), (17, 6)])
def test_relinearised_products_large_rings(logN, L):
    """Rings 2^16 / 2^17 (256-point row passes: the ModUp row pass runs fused with
    the relinearisation inner product, k_modup_row_ks): single and stacked
    products, squares and mul_add down the chain, word-identical to the oracle."""
    orc = O.Context(logN, L, 40, 60, 3, seed=logN)
    gpu = F.Context(logN, L, 40, 60, 3, seed=logN, keygen=False)
    gpu.load_keys_from(orc, [])
    rng = np.random.default_rng(logN)
    xs = [orc.encrypt(rng.uniform(-1, 1, 64), 64) for _ in range(3)]
    gx = [gpu.from_oracle(x) for x in xs]
    oc, gc = xs[0], gx[0]
    for i in range(L - 1):
        oc, gc = orc.mul(oc, xs[1]), gpu.mul(gc, gx[1])
        if i % 2 == 0:
            same(gc, oc)
    same(gc, oc)
    same(gpu.square(gx[2]), orc.square(xs[2]))
    st = gpu.mul(gpu.stack(gx), gx[1])  # three members times one (broadcast)
    for m in range(3):
        same(gpu.member(st, m), orc.mul(xs[m], xs[1]))
    assert np.max(np.abs(gpu.decrypt(gpu.mul(gx[0], gx[1])) - orc.decrypt(orc.mul(xs[0], xs[1])))) < 1e-9
    # stacks of >= 4 members relinearise through dev::ntt_row_ks (ModUp's row pass
    # fused with the key-switch inner product; round 5): 16 members (full blocks),
    # 20 (a partial block), 8 (8 members x 2 rows per block) and 5 two levels
    # down (4 members x 4 rows per block, partial); the narrow ciphertext ops of
    # those batches stage 2-4 rows of twiddles per block
    ys = [orc.encrypt(rng.uniform(-1, 1, 64), 64) for _ in range(20)]
    gy = [gpu.from_oracle(y) for y in ys]
    for cnt in (16, 20, 8):  # 16 members per block (full, partial); 8 per block x 2 rows
        with F.KernelClock(gpu) as clk:  # (advisor r5: the fused kernel must be the one that ran)
            st = gpu.mul(gpu.stack(gy[:cnt]), gpu.stack(gy[::-1][:cnt]))
        assert any(k.startswith('k_ntt_row_ks') for k in clk.stats), sorted(clk.stats)
        # 40-bit scaling primes: the HMult tail's ModDown + rescale is the fp64 kernel
        assert any(k.startswith('k_moddown_rescale_fp<') for k in clk.stats), sorted(clk.stats)
        for m in (0, 7, cnt - 1):
            same(gpu.member(st, m), orc.mul(ys[m], ys[::-1][m]))
    lo = [orc.mul(orc.mul(y, xs[1]), xs[2]) for y in ys[:5]]
    gl = gpu.stack([gpu.from_oracle(y) for y in lo])
    with F.KernelClock(gpu) as clk:
        st = gpu.mul(gl, gl)
    assert any(k.startswith('k_ntt_row_ks') for k in clk.stats), sorted(clk.stats)
    for m in range(5):
        same(gpu.member(st, m), orc.mul(lo[m], lo[m]))


def test_config2_direct_sort_full_size_bit_exact():
    """BASELINE config 2 at its full size: DirectSort N=128 at ring 2^16, depth 30,
    the reference's 40-bit scaling primes, 30 rotation keys, CompositeSign(3,3,2)
    (src/sort_algo.h:117-123, tests/DirectSortTest.cpp:107-108): the GPU sort
    equals the CPU oracle's word for word on identical keys (the oracle's keys are
    generated on the host here: 31 limbs x 2^16, ~40 s of CPU work), and meets the
    reference's own bound (sorted within 0.01 at output level == multDepth)."""
    N = 128
    depth, rots = O.size_parameters(N)
    assert depth == 30 and len(rots) == 30
    orc = O.Context(16, depth, 40, 60, 3, seed=2)
    orc.gen_rotation_keys(rots)
    gpu = F.Context(16, depth, 40, 60, 3, seed=2, keygen=False)
    gpu.load_keys_from(orc, rots)
    x = np.random.default_rng(20250704).permutation(N) / N
    ox = orc.encrypt(x, N)
    gout = gpu.direct_sort(gpu.from_oracle(ox), N, rots, (3, 3, 2))
    same(gout, orc.direct_sort(ox, N, rots, (3, 3, 2)))
    assert gout.level == depth
    assert np.max(np.abs(gpu.decrypt(gout) - np.sort(x))) < 0.01


def test_config3_direct_sort_full_size():
    """The BASELINE metric's own configuration at full size: DirectSort N=1024 at ring
    2^16, depth 39, 161 rotation keys, CompositeSign(3,5,2), scale 2^50
    -- the bench workload.  Word-for-word parity with the oracle at this size is
    test_gpu_digests.py (oracle digests, 1 h of CPU); here the size-independent
    properties: the reference's bound (sorted within 0.01,
    output level == multDepth; tests/DirectSortTest.cpp:128,169), and the same
    ciphertext word for word whether the 32 comparator / index-check batches run as
    one stack on three concurrent lanes (the bench's setting) or in stacks of 5 on one
    lane."""
    N = 1024
    depth, rots = F.size_parameters(N)
    assert depth == 39 and len(rots) == 161
    gpu = F.Context(16, depth, 50, 60, 3, seed=20250704)
    gpu.gen_rotation_keys(rots)
    x = np.random.default_rng(20250704).permutation(N) / N
    ct = gpu.encrypt(x, N)
    gpu.set_sort_lanes(3)
    gpu.set_sort_stack(32)
    a = gpu.direct_sort(ct, N, rots, (3, 5, 2))
    gpu.set_sort_lanes(1)
    gpu.set_sort_stack(5)
    try:
        b = gpu.direct_sort(ct, N, rots, (3, 5, 2))
    finally:
        gpu.set_sort_stack(32)
    assert a.level == depth
    assert np.max(np.abs(gpu.decrypt(a) - np.sort(x))) < 0.01
    assert np.array_equal(a.data(), b.data())


@pytest.mark.parametrize('N,scale_bits', [(128, 40), (256, 40), (512, 40), (1024, 40), (1024, 50)])
def test_reference_shipped_context_ring17(N, scale_bits):
    """DirectSortTest's own context (tests/DirectSortTest.cpp:24-51): ring 2^17,
    the reference's 40-bit scaling primes, the getSizeParameters depth/rotations
    (src/sort_algo.h:87-201), N up to 1024 (DirectSortTest.cpp:174-179).  With
    OpenFHE's Paterson-Stockmeyer split (the default) the degree-6510 doubled-sinc
    index check holds the reference's 0.01 at 40 bits; the power-of-two split of
    rounds 1-2 missed it for N >= 256 (0.012 / 0.63 at N = 256 / 1024,
    profiles/r2_c/diag_ring17.jsonl).  Bound and level assertion as
    DirectSortTest.cpp:128,169."""
    depth, rots = F.size_parameters(N)
    gpu = F.Context(17, depth, scale_bits, 60, 3, seed=1234)
    try:
        assert gpu.ps_split == F.PS_SPLIT_OPENFHE
        gpu.gen_rotation_keys(rots)
        x = np.random.default_rng(N).permutation(N) / N
        cfg = (3, 2, 2) if N <= 16 else (3, 3, 2) if N <= 128 else (3, 4, 2) if N <= 512 else (3, 5, 2)
        out = gpu.direct_sort(gpu.encrypt(x, N), N, rots, cfg)
        assert out.level == depth
        err = float(np.max(np.abs(gpu.decrypt(out) - np.sort(x))))
        print(f'N={N} scale 2^{scale_bits} ring 2^17: max err {err:.3e}')
        assert err < 0.01
    finally:
        gpu.close()
