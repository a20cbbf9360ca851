"""The rings and key-switch digit counts between the benchmark configurations.

The other GPU tests compare words at rings 2^11, 2^12, 2^13, 2^16 and 2^17 and
with three key-switch digits.  fhe_ctx_create accepts log_n 10..17 and up to
eight digits, so these run the rows of the dispatch tables in between, word for
word against the CPU oracle and the big-integer model (tests/bigint_model.py):

  * rings 2^10, 2^14, 2^15, (L = 6, dnum 3) at 40- and 41-bit scaling (the
    latter interleaves the prime classes): the NTT of every prime against the
    model, fhe_ntt_dev over 1, 2, 3, 5 and 17 segments, ModUp / ModDown at
    full and partial digits against the model, stacked products, squares,
    rescales, rotations, hoisted rotations and plaintext products at three
    levels against the oracle, one product and one rotation of real
    encryptions against the model (in an L = 2 context of the same ring: the
    smallest depth with more than one digit, 3.4 s of model time at ring 2^15),
    one decrypted product, and the device encoder at its slot-count edges.
    Rings 2^14 and 2^15 are the only ones whose row pass is 7 bits
    (k_ntt_fwd<7, 4, false, ...>); ring 2^10 is the only one whose passes fill
    half a block (32 transforms in blocks of 64: the bounds-checked kernels
    with idle lanes).  test_dispatch_rows_ran asserts from the kernel clock
    that those instantiations are what ran.
  * rings 2^16 and 2^17 with 4..8 digits: k_ntt_row_ks<D, FP, FULL> for every
    D in 4..8, both prime classes, full and partial member blocks (4, 5 and 12
    members: 12 is blocks of 8 with a partial last one), against the oracle,
    and one product at ell = 8 against the model.

Every comparison is equality of level, slots, scale and every limb word; the
decrypted product's 1e-6 is test_wide_digits_match_oracle's bound.
"""
import re

import numpy as np
import pytest

import bigint_model as M
import fhesort as F
import pyoracle as O
from test_gpu_bigint_model import check_conversions, check_mul_rotate, check_ntt, fused_tail_ran, no_ties
from test_gpu_mixed_classes import class_runs, rand_ct, rand_limbs, tagged
from test_gpu_parity import _Hip, same

pytestmark = pytest.mark.gpu

ROTS = [1, -3]
L = 6
RINGS = [10, 14, 15]
NAMES = {}  # ring -> kernel names the clocked calls of this module launched


class clock:
    """KernelClock that also files the names under the context's ring"""

    def __init__(self, gpu):
        self.gpu, self.k = gpu, F.KernelClock(gpu)

    def __enter__(self):
        self.k.__enter__()
        return self.k

    def __exit__(self, *exc):
        self.k.__exit__(*exc)
        NAMES.setdefault(self.gpu.logN, set()).update(self.k.stats)
        return False


def make(logN, depth, bits, dnum, seed, rots=ROTS):
    orc = O.Context(logN, depth, bits, 60, dnum, seed=seed)
    if rots:
        orc.gen_rotation_keys(rots)
    gpu = F.Context(logN, depth, bits, 60, dnum, seed=seed, keygen=False)
    gpu.load_keys_from(orc, rots)
    assert np.array_equal(orc.primes, gpu.primes)
    return orc, gpu


@pytest.fixture(scope='module', params=[(r, b) for r in RINGS for b in (40, 41)], ids=lambda p: f'ring{p[0]}-scale{p[1]}')
def trio(request):
    logN, bits = request.param
    orc, gpu = make(logN, L, bits, 3, 100 * logN + bits)
    return orc, gpu, M.Model(logN, gpu.primes, gpu.nq, gpu.K, gpu.alpha, gpu.ntt)


@pytest.fixture(scope='module', params=[(r, b) for r in RINGS for b in (40, 41)], ids=lambda p: f'ring{p[0]}-scale{p[1]}')
def small(request):
    """L = 2: three one-prime digits, the smallest context whose product runs
    the whole key switch -- what keeps Model.mul + Model.rotate at 3.4 s at ring 2^15"""
    logN, bits = request.param
    orc, gpu = make(logN, 2, bits, 3, 200 * logN + bits, rots=[1])
    return orc, gpu, M.Model(logN, gpu.primes, gpu.nq, gpu.K, gpu.alpha, gpu.ntt)


def test_prime_classes(trio):
    """40 bits: q_0 and the special primes integer, the scaling primes fp64;
    41 bits: the scaling primes of both classes, interleaved"""
    _, gpu, m = trio
    fp, integer = class_runs(gpu.primes[:gpu.nq])
    assert (m.alpha, gpu.nq) == (3, L + 1)
    if max(m.q[1:m.nq]) >= (1 << 41):
        assert len(fp) >= 2 and len(integer) >= 2, (fp, integer)  # (q_0 opens the first integer run)
    else:
        assert fp == [(1, L)] and integer == [(0, 1)], (fp, integer)


# ------------------------------------------------------------------- NTT --
def test_ntt_every_prime_against_model(trio):
    _, gpu, m = trio
    with clock(gpu):
        check_ntt(gpu, m)


@pytest.mark.parametrize('segs', [1, 2, 3, 5, 17])
def test_ntt_on_device_memory(trio, segs):
    """fhe_ntt_dev over primes 1..4 of `segs` segments against the oracle's NTT
    limb by limb; the inverse restores the input"""
    orc, gpu, _ = trio
    hip = _Hip()
    n, first, limbs = gpu.n, 1, 4
    rng = np.random.default_rng(segs)
    x = np.stack([rand_limbs(rng, gpu.primes[first:first + limbs], n) for _ in range(segs)])
    want = np.stack([np.stack([orc.ntt(first + i, x[s, i]) for i in range(limbs)]) for s in range(segs)])
    dev = hip.upload(x)
    try:
        with clock(gpu):
            gpu.ntt_dev(dev, first, limbs, segments=segs, seg_stride=limbs * n)
            gpu.sync()
            got = hip.download(dev, x)
            gpu.ntt_dev(dev, first, limbs, inverse=True, segments=segs, seg_stride=limbs * n)
            gpu.sync()
        for s in range(segs):
            for i in range(limbs):
                assert np.array_equal(got[s, i], want[s, i]), f'forward, segment {s}, prime {first + i}'
        assert np.array_equal(hip.download(dev, x), x), 'the inverse does not restore the input'
    finally:
        hip.h.hipFree(hip.C.c_void_p(dev))


# ------------------------------------------------------------ conversions --
@pytest.mark.parametrize('which', ['L+1', '2alpha', 'alpha+1', 'alpha', '1'])
def test_conversions_against_model(trio, which):
    _, gpu, m = trio
    ell = {'L+1': m.nq, '2alpha': 2 * m.alpha, 'alpha+1': m.alpha + 1, 'alpha': m.alpha, '1': 1}[which]
    with clock(gpu):
        check_conversions(gpu, m, (ell,), (ell,))


# ------------------------------------------- products, rotations: the model --
def test_product_and_rotation_against_model(small):
    orc, gpu, m = small
    assert (m.alpha, m.K, gpu.nq) == (1, 1, 3)
    check_mul_rotate(orc, gpu, m, 0, gpu.logN)  # (asserts zero ties and that the fused ModDown + rescale ran)


def test_decrypted_product(trio):
    orc, gpu, _ = trio
    rng = np.random.default_rng(gpu.logN)
    a, b = rng.uniform(-1, 1, 16), rng.uniform(-1, 1, 16)
    oa, ob = orc.encrypt(a, 16), orc.encrypt(b, 16)
    with clock(gpu) as clk:
        gm = gpu.mul(gpu.from_oracle(oa), gpu.from_oracle(ob))
    fused_tail_ran(clk.stats)
    same(gm, orc.mul(oa, ob))
    assert np.max(np.abs(gpu.decrypt(gm) - a * b)) < 1e-6


# ------------------------------------------------- stacked ops: the oracle --
_inputs = {}


def stack_inputs(orc, gpu, level):
    """five random ciphertexts, five partners and a plaintext at `level`, the
    same words on both sides, built once per context and level"""
    key = (id(gpu), level)
    if key not in _inputs:
        rng = np.random.default_rng(1000 * gpu.logN + level)
        xs = [rand_ct(orc, gpu, rng, level) for _ in range(5)]
        ys = [rand_ct(orc, gpu, rng, level) for _ in range(5)]
        v = rng.uniform(-1, 1, 16)
        _inputs[key] = xs, ys, v, {}
    return _inputs[key]


@pytest.mark.parametrize('count', [1, 3, 5])
@pytest.mark.parametrize('level', [0, 3, L - 1])
def test_stacked_ops(trio, level, count):
    """level L - 1 leaves one limb above q_0: the FP class has a single limb (40 bits)"""
    orc, gpu, _ = trio
    xs, ys, v, memo = stack_inputs(orc, gpu, level)

    def want(name, m, fn):  # the oracle's result for member m, computed once per level
        if (name, m) not in memo:
            memo[name, m] = fn()
        return memo[name, m]

    S = gpu.stack([g for _, g in xs[:count]])
    T = gpu.stack([g for _, g in ys[:count]])
    pt_o = orc.encode(v, 16, level)
    cases = [
        ('mul stacked', lambda: gpu.mul(S, T), lambda m: orc.mul(xs[m][0], ys[m][0])),
        ('mul broadcast', lambda: gpu.mul(S, ys[1][1]), lambda m: orc.mul(xs[m][0], ys[1][0])),
        ('square', lambda: gpu.square(S), lambda m: orc.square(xs[m][0])),
        ('mul_const', lambda: gpu.mul_const(S, -0.75), lambda m: orc.mul_const(xs[m][0], -0.75)),
        ('rescale', lambda: gpu.rescale(gpu.mul_int(S, 7)), lambda m: orc.rescale(orc.mul_int(xs[m][0], 7))),
        ('rotate 1', lambda: gpu.rotate(S, 1), lambda m: orc.rotate(xs[m][0], 1)),
        ('rotate -3', lambda: gpu.rotate(S, -3), lambda m: orc.rotate(xs[m][0], -3)),
        ('mul_plain', lambda: gpu.mul_plain(S, gpu.encode_device(v, 16, level)), lambda m: orc.mul_plain(xs[m][0], pt_o)),
    ]
    if level + 2 <= L:
        cases.append(('rescale after mul_const', lambda: gpu.rescale(gpu.mul_const(S, 0.5)),
                      lambda m: orc.rescale(orc.mul_const(xs[m][0], 0.5))))
    for name, gop, oop in cases:
        with clock(gpu):
            R = gop()
        for m in range(count):
            tagged(f'{name}, member {m} of {count}, level {level}',
                   lambda: same(gpu.member(R, m) if count > 1 else R, want(name, m, lambda: oop(m))))
    with clock(gpu):
        hs = gpu.rotate_hoisted(S, ROTS + [0])
    for h, k in zip(hs, ROTS + [0]):
        for m in range(count):
            tagged(f'hoisted {k}, member {m} of {count}, level {level}',
                   lambda: same(gpu.member(h, m) if count > 1 else h,
                                want(f'rotate {k}', m, lambda: orc.rotate(xs[m][0], k)) if k else xs[m][0]))


# ------------------------------------------------------- the device encoder --
@pytest.mark.parametrize('logN', RINGS + [17])
def test_device_encoder_slot_edges(logN):
    """1 slot (the smallest the host encoder takes: zero bits to reverse), 2,
    4096 (exactly one LDS run), 8192 (one global stage in front of it) and n/2"""
    orc = O.Context(logN, L, 40, 60, 3, seed=5, keygen=False)
    gpu = F.Context(logN, L, 40, 60, 3, seed=5, keygen=False)
    n = 1 << logN
    rng = np.random.default_rng(logN)
    for slots in sorted({s for s in (1, 2, 4096, 8192, n // 2) if s <= n // 2}):
        for level in (0, L):
            v = rng.uniform(-1, 1, slots)
            want = orc.encode(v, slots, level).data()
            assert np.array_equal(gpu.encode(v, slots, level).data(), want), f'host encoder, slots {slots} level {level}'
            got = gpu.encode_device(v, slots, level).data()
            if not np.array_equal(got, want):
                bad = np.argwhere(got != want)
                raise AssertionError(f'slots {slots} level {level}: {len(bad)} words differ, first {bad[0].tolist()}')
    gpu.close()


# ------------------------------------------- what ran (after the tests above) --
def ran(names, prefix, suffix=''):
    return any(k.startswith(prefix) and k.split('@')[0].endswith(suffix) for k in names)


@pytest.mark.parametrize('logN', RINGS)
def test_dispatch_rows_ran(logN):
    """the instantiations only these rings reach.  k_ntt_fwd<PB, EB, COLS, MODE,
    FULL, FP>, k_ntt_inv<PB, EB, COLS, FULL, FP>; row modes 0 plain, 2 rescale,
    3 HMult tail, 4 key-switch finish (rotations take it at every ring)"""
    names = NAMES.get(logN, set())
    assert names, 'runs after the other tests of this module (it reads the names their launches left)'
    if logN == 10:
        # 32 columns / rows in blocks of 64: the bounds-checked forms (FULL = false)
        for prefix in ('k_ntt_fwd<5, 3, true, 0, false, ', 'k_ntt_inv<5, 3, true, false, ',
                       'k_ntt_fwd<5, 3, false, 0, false, ', 'k_ntt_inv<5, 3, false, false, '):
            for fp in ('true>', 'false>'):
                assert ran(names, prefix, fp), (prefix, fp, sorted(names))
        for mode in (2, 3, 4):
            assert ran(names, f'k_ntt_fwd<5, 3, false, {mode}, false, '), (mode, sorted(names))
        assert ran(names, 'k_ntt_fwd<5, 3, true, 1, false, '), sorted(names)  # the rescale's lifted column pass
        return
    for mode in (0, 2, 3, 4):
        for fp in ('true>', 'false>'):
            assert ran(names, f'k_ntt_fwd<7, 4, false, {mode}, ', fp), (mode, fp, sorted(names))
    for fp in ('true>', 'false>'):
        assert ran(names, 'k_ntt_inv<7, 4, false, ', fp), (fp, sorted(names))
        assert ran(names, f'k_ntt_fwd<{logN - 7}, 4, true, ', fp), (fp, sorted(names))


# ============================================ 4..8 digits at rings 2^16, 2^17 ==
ROW_KS = re.compile(r'k_ntt_row_ks<(\d+), (\w+), (\w+)>')
ROWS = set()  # (D, FP, FULL) of every k_ntt_row_ks the tests below launched


def note_row_ks(stats):
    found = {m.groups() for m in map(ROW_KS.match, stats) if m}
    ROWS.update((int(d), fp in ('1', 'true'), full in ('1', 'true')) for d, fp, full in found)
    return found


@pytest.fixture(scope='module')
def wide16():
    """alpha = 2: eight digits at the top level"""
    orc, gpu = make(16, 15, 40, 8, 168)
    assert (gpu.alpha, gpu.K, gpu.nq) == (2, 2, 16)
    return orc, gpu, {}


def digit_inputs(orc, gpu, memo, ell):
    if ell not in memo:
        memo.clear()  # one level's 24 ciphertexts at a time
        rng = np.random.default_rng(ell)
        level = gpu.nq - ell
        memo[ell] = ([rand_ct(orc, gpu, rng, level, 64) for _ in range(12)],
                     [rand_ct(orc, gpu, rng, level, 64) for _ in range(12)], {})
    return memo[ell]


@pytest.mark.parametrize('count', [4, 5, 12])
@pytest.mark.parametrize('ell,digits', [(16, 8), (14, 7), (13, 7), (11, 6), (9, 5), (8, 4)])
def test_digit_counts(wide16, ell, digits, count):
    """stacked products through dev::ntt_row_ks: 13, 11 and 9 limbs end in a
    one-prime digit; 4 members fill a block, 5 and 12 leave a partial one"""
    orc, gpu, memo = wide16
    xs, ys, want = digit_inputs(orc, gpu, memo, ell)
    with F.KernelClock(gpu) as clk:
        st = gpu.mul(gpu.stack([g for _, g in xs[:count]]), gpu.stack([g for _, g in ys[:count]]))
    found = note_row_ks(clk.stats)
    assert found and {int(d) for d, _, _ in found} == {digits}, sorted(clk.stats)
    fused_tail_ran(clk.stats)
    for m in (0, count // 2, count - 1):
        if m not in want:
            want[m] = orc.mul(xs[m][0], ys[m][0])
        tagged(f'{count} members at ell {ell}, member {m}', lambda: same(gpu.member(st, m), want[m]))


@pytest.mark.parametrize('ell', [16, 9])
def test_digit_counts_rotations(wide16, ell):
    orc, gpu, memo = wide16
    xs, _, _ = digit_inputs(orc, gpu, memo, ell)
    S = gpu.stack([g for _, g in xs[:4]])
    R = gpu.rotate(S, 1)
    hs = gpu.rotate_hoisted(S, ROTS)
    for m in (0, 3):
        r1 = orc.rotate(xs[m][0], 1)
        tagged(f'rotate, ell {ell}, member {m}', lambda: same(gpu.member(R, m), r1))
        tagged(f'hoisted 1, ell {ell}, member {m}', lambda: same(gpu.member(hs[0], m), r1))
        tagged(f'hoisted -3, ell {ell}, member {m}', lambda: same(gpu.member(hs[1], m), orc.rotate(xs[m][0], -3)))


def test_digit_counts_against_model(wide16):
    """four digits at ell = 8: member 0 of a stack of four against Model.mul"""
    orc, gpu, memo = wide16
    xs, ys, _ = digit_inputs(orc, gpu, memo, 8)
    m = M.Model(16, gpu.primes, gpu.nq, gpu.K, gpu.alpha, gpu.ntt)
    with F.KernelClock(gpu) as clk:
        st = gpu.mul(gpu.stack([g for _, g in xs[:4]]), gpu.stack([g for _, g in ys[:4]]))
    assert note_row_ks(clk.stats), sorted(clk.stats)
    want, ties = m.mul(xs[0][0].data(), ys[0][0].data(), orc.relin_key())
    no_ties(ties)
    assert np.array_equal(want, gpu.member(st, 0).data())


@pytest.mark.parametrize('logN,depth,dnum,alpha,K,ells', [(16, 7, 8, 1, 1, (8, 5)), (17, 9, 5, 2, 2, (10, 7))])
def test_one_prime_digits_and_ring17(logN, depth, dnum, alpha, K, ells):
    """(16, L = 7, dnum 8): eight digits of one prime, K = 1; (17, L = 9, dnum 5):
    five digits at ring 2^17, and four with a one-prime last digit"""
    orc, gpu = make(logN, depth, 40, dnum, logN + depth, rots=[])
    assert (gpu.alpha, gpu.K) == (alpha, K)
    rng = np.random.default_rng(depth)
    for ell in ells:
        level = gpu.nq - ell
        xs, ys = [rand_ct(orc, gpu, rng, level, 64) for _ in range(5)], [rand_ct(orc, gpu, rng, level, 64) for _ in range(5)]
        with F.KernelClock(gpu) as clk:
            st = gpu.mul(gpu.stack([g for _, g in xs]), gpu.stack([g for _, g in ys]))
        found = note_row_ks(clk.stats)
        assert found and {int(d) for d, _, _ in found} == {-(-ell // alpha)}, sorted(clk.stats)
        for m in (0, 4):
            tagged(f'ring 2^{logN}, ell {ell}, member {m}', lambda: same(gpu.member(st, m), orc.mul(xs[m][0], ys[m][0])))
    gpu.close()


def test_every_digit_count_ran():
    """k_ntt_row_ks<D, FP, FULL>: every D in 4..8 in both prime classes, and both block forms"""
    assert ROWS, 'runs after the digit-count tests of this module'
    for d in range(4, 9):
        for fp in (False, True):
            assert any(r[0] == d and r[1] == fp for r in ROWS), (d, fp, sorted(ROWS))
    assert {r[2] for r in ROWS} == {False, True}, sorted(ROWS)
