"""Lexicographic rank on the GPU (fhe_direct_lex_rank).

Kernel level: k_sub_lex_stacked and k_tensor_lex against the oracle ops they
fuse, member by member and word for word.  Operator level: lex_rank against the
CPU-oracle composition of tests/lex_model.py, word for word, for two and three
keys at N = 8 (one comparator batch) and N = 64 (two: the stacked path), with the
tie-break on tied tuples and without it on pairwise-distinct ones, at every
chunking, lane count and mask-cache setting and in the plain (unfused) form;
decrypted ranks against np.lexsort's; the rank feeding the record sort.
Oracle results are computed once per module and shared."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fhesort as F
import lex_model as X
import pyoracle as O
import stable_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
KERNELS = ('k_sub_lex_stacked', 'k_tensor_lex')

# Largest |decrypted - exact rank| of the CPU-oracle composition on these inputs and
# seeds, per (N, L, tie-break) (measured on the CPU).  The GPU
# words are the oracle's, so this is the GPU's error too; the tests assert 4x it,
# room for another seed's noise, not for a defect: a wrong word fails the word
# comparison first.
ORACLE_ERR = {
    (8, 2, True): 1.737e-07, (8, 2, False): 9.381e-08, (8, 3, True): 1.310e-07, (8, 3, False): 1.393e-07,
    (64, 2, True): 1.438e-07, (64, 2, False): 1.277e-06, (64, 3, True): 1.824e-07, (64, 3, False): 8.790e-07,
}


def same(g, o):
    """equal level, slots, scale and words"""
    gi, oi = g.info(), o.info()
    assert (gi['level'], gi['slots'], gi['limbs'], gi['scale']) == (oi['level'], oi['slots'], oi['limbs'], oi['scale'])
    gd, od = g.data(), o.data()
    if not np.array_equal(gd, od):
        bad = np.argwhere(gd != od)
        raise AssertionError(f'{len(bad)} limb words differ, first at {bad[0].tolist()}')


def has(clk, name):
    return any(k.startswith(name) for k in clk.stats)


def launches(clk, name):
    return sum(v['launches'] for k, v in clk.stats.items() if k.startswith(name))


# ------------------------------------------------------------ kernel level --
@pytest.fixture(scope='module')
def small():
    """ring 2^12, L = 3, 40-bit scaling beside the 60-bit q0; 40 encrypted vectors"""
    orc = O.Context(12, 3, 40, 60, 3, seed=53)
    gpu = F.Context(12, 3, 40, 60, 3, seed=53, keygen=False)
    gpu.load_keys_from(orc, [])
    rng = np.random.default_rng(19)
    vals = [rng.uniform(-1, 1, 16) for _ in range(40)]
    return orc, gpu, vals


def _lex_operands(orc, gpu, vals, L, B, la, lb, offsets):
    oas = [orc.encrypt(vals[l], 16, la) for l in range(L)]
    obs = [orc.encrypt(vals[4 + i], 16, lb) for i in range(L * B)]
    ops = [orc.encode(vals[20 + i], 16, max(la, lb)) for i in range(B)] if offsets else None
    gps = [gpu.encode(vals[20 + i], 16, max(la, lb)) for i in range(B)] if offsets else None
    return oas, obs, ops, gps


def _check_lex_stack(orc, gpu, R, oas, obs, ops, L, B, eps):
    with pytest.raises(F.FheError):
        gpu.member(R, (2 * L - 1) * B)
    for l in range(L):
        for i in range(B):
            d = orc.sub(oas[l], obs[l * B + i])
            if l < L - 1:
                same(gpu.member(R, 2 * l * B + i), orc.add_const(d, eps))
                same(gpu.member(R, (2 * l + 1) * B + i), orc.add_const(d, -eps))
            else:
                same(gpu.member(R, 2 * l * B + i), d if ops is None else orc.add_plain(d, ops[i]))


# five operands cross the guarded tail of a thread's four
@pytest.mark.parametrize('offsets', [False, True], ids=['no-offsets', 'offsets'])
@pytest.mark.parametrize('B', [1, 4, 5])
@pytest.mark.parametrize('L', [2, 3])
@pytest.mark.parametrize('la,lb', [(1, 1), (0, 1)], ids=['same-level', 'a-one-level-below'])
def test_sub_lex_stacked_matches_oracle(small, la, lb, L, B, offsets):
    orc, gpu, vals = small
    eps = 1.0 / 16
    oas, obs, ops, gps = _lex_operands(orc, gpu, vals, L, B, la, lb, offsets)
    with F.KernelClock(gpu) as clk:
        R = gpu.sub_lex_stacked([gpu.from_oracle(a) for a in oas], [gpu.from_oracle(b) for b in obs], eps, gps)
    assert clk.stats['k_sub_lex_stacked']['launches'] == 1, sorted(clk.stats)
    assert not has(clk, 'k_c0_op') and not has(clk, 'k_sub_add_plain_stacked') and 'k_sub' not in clk.stats, sorted(clk.stats)
    _check_lex_stack(orc, gpu, R, oas, obs, ops, L, B, eps)


def test_sub_lex_stacked_second_launch(small):
    """three keys with tie-break offsets, 11 operands: a launch holds min(32 / 3, 16) = 10, so the second
    takes its b at key * count + base + i and its offsets at base + i"""
    orc, gpu, vals = small
    eps, L, B = 1.0 / 16, 3, 11
    oas, obs, ops, gps = _lex_operands(orc, gpu, vals, L, B, 1, 1, True)
    with F.KernelClock(gpu) as clk:
        R = gpu.sub_lex_stacked([gpu.from_oracle(a) for a in oas], [gpu.from_oracle(b) for b in obs], eps, gps)
    assert clk.stats['k_sub_lex_stacked']['launches'] == 2, sorted(clk.stats)
    _check_lex_stack(orc, gpu, R, oas, obs, ops, L, B, eps)


@pytest.mark.parametrize('offsets', [False, True], ids=['no-offsets', 'offsets'])
@pytest.mark.parametrize('L', [2, 3])
def test_sub_lex_stacked_with_the_keys_above_the_operands(small, L, offsets):
    """keys deeper than the bs: every b is adjusted instead, so per-member ops (sub_stacked's rule)"""
    orc, gpu, vals = small
    eps, B = 0.125, 3
    oas, obs, ops, gps = _lex_operands(orc, gpu, vals, L, B, 2, 1, offsets)
    with F.KernelClock(gpu) as clk:
        R = gpu.sub_lex_stacked([gpu.from_oracle(a) for a in oas], [gpu.from_oracle(b) for b in obs], eps, gps)
    assert 'k_sub_lex_stacked' not in clk.stats
    _check_lex_stack(orc, gpu, R, oas, obs, ops, L, B, eps)


def test_sub_lex_stacked_refusals(small):
    orc, gpu, vals = small
    a1 = [gpu.encrypt(vals[i], 16, 1) for i in range(5)]
    a2 = gpu.encrypt(vals[5], 16, 2)
    b1 = [gpu.encrypt(vals[6 + i], 16, 1) for i in range(4)]
    b2 = gpu.encrypt(vals[10], 16, 2)
    p1, p0 = gpu.encode(vals[11], 16, 1), gpu.encode(vals[11], 16, 0)
    st = gpu.stack([b1[0], b1[1]])
    cases = [
        (a1[:1], b1[:1], None),                   # one key
        (a1[:5], b1 + b1[:1], None),              # five keys
        ([a1[0], a2], b1[:2], None),              # keys at different levels
        ([a1[0], st], b1[:2], None),              # a key is a stack
        (a1[:2], [b1[0], b2], None),              # operands at different levels
        (a1[:2], [b1[0], st], None),              # an operand is a stack
        (a1[:2], b1[:2], [p0]),                   # offsets at another level
    ]
    for as_, bs, ps in cases:
        with pytest.raises(F.FheError) as e:
            gpu.sub_lex_stacked(as_, bs, 0.1, ps)
        assert e.value.code == F.FHE_EINVAL, (len(as_), len(bs))
    # operand and offset counts that do not fit never reach the library
    with pytest.raises(ValueError):
        gpu.sub_lex_stacked(a1[:2], b1[:3], 0.1)
    with pytest.raises(ValueError):
        gpu.sub_lex_stacked(a1[:2], b1[:4], 0.1, [p1])
    o = C.c_void_p()
    arr = (C.c_void_p * 2)(a1[0].h, a1[1].h)
    assert F.lib().fhe_sub_lex_stacked(gpu.h, arr, 2, arr, 0, None, 0.1, C.byref(o)) == F.FHE_EINVAL  # count 0


# dnum 3 over the context's 4 primes: level 2 (2 limbs) takes one key-switch digit, level 0 (4 limbs) two
@pytest.mark.parametrize('t_const', [0.0, 1.0])
@pytest.mark.parametrize('B', [1, 4, 5])
@pytest.mark.parametrize('level', [2, 0], ids=['one-digit', 'multi-digit'])
def test_mul_lex_matches_oracle(small, level, B, t_const):
    orc, gpu, vals = small
    ot = [orc.encrypt(v, 16, level) for v in vals[0:B]]
    ou = [orc.encrypt(v, 16, level) for v in vals[5:5 + B]]
    ow = [orc.encrypt(v, 16, level) for v in vals[10:10 + B]]
    st = lambda xs: gpu.stack([gpu.from_oracle(x) for x in xs])
    with F.KernelClock(gpu) as clk:
        R = gpu.mul_lex(st(ot), t_const, st(ou), st(ow))
    assert launches(clk, 'k_tensor_lex') == 1, sorted(clk.stats)
    assert [k for k in clk.stats if k.startswith('k_tensor')] == ['k_tensor_lex'], sorted(clk.stats)
    assert 'k_sub' not in clk.stats and not has(clk, 'k_c0_op'), sorted(clk.stats)
    with pytest.raises(F.FheError):
        gpu.member(R, B)
    for z in range(B):
        same(gpu.member(R, z), orc.mul(orc.add_const(ot[z], t_const), orc.sub(ou[z], ow[z])))


def test_mul_lex_digit_counts(small):
    """the two levels above really differ in key-switch digits (dnum 3 over the context's primes)"""
    orc, gpu, vals = small
    limbs = {lv: orc.encrypt(vals[0], 16, lv).info()['limbs'] for lv in (0, 2)}
    alpha = -(-limbs[0] // 3)
    assert -(-limbs[2] // alpha) == 1 and -(-limbs[0] // alpha) > 1, limbs


@pytest.mark.parametrize('t_const', [0.0, 1.0])
@pytest.mark.parametrize('lt,lu', [(0, 1), (2, 1)], ids=['t-below', 't-above'])
def test_mul_lex_falls_back_when_t_sits_at_another_level(small, lt, lu, t_const):
    """the product would level-adjust an operand first: the difference, then the plain product"""
    orc, gpu, vals = small
    B = 3
    ot = [orc.encrypt(v, 16, lt) for v in vals[0:B]]
    ou = [orc.encrypt(v, 16, lu) for v in vals[5:5 + B]]
    ow = [orc.encrypt(v, 16, lu) for v in vals[10:10 + B]]
    st = lambda xs: gpu.stack([gpu.from_oracle(x) for x in xs])
    with F.KernelClock(gpu) as clk:
        R = gpu.mul_lex(st(ot), t_const, st(ou), st(ow))
    assert not has(clk, 'k_tensor_lex'), sorted(clk.stats)
    for z in range(B):
        same(gpu.member(R, z), orc.mul(orc.add_const(ot[z], t_const), orc.sub(ou[z], ow[z])))


def test_mul_lex_refusals(small):
    orc, gpu, vals = small
    x1 = [gpu.encrypt(v, 16, 1) for v in vals[:4]]
    x2 = [gpu.encrypt(v, 16, 2) for v in vals[:2]]
    t, u, w = gpu.stack(x1[:2]), gpu.stack(x1[2:]), gpu.stack(x1[1:3])
    cases = [(t, u, x1[0]),             # w holds fewer members
             (x1[0], u, w),             # t holds fewer members
             (t, u, gpu.stack(x2))]     # u and w at different levels
    for tt, uu, ww in cases:
        with pytest.raises(F.FheError) as e:
            gpu.mul_lex(tt, 1.0, uu, ww)
        assert e.value.code == F.FHE_EINVAL
    x3 = [gpu.encrypt(v, 16, 3) for v in vals[:2]]  # the last level: nothing left for the product
    with pytest.raises(F.FheError) as e:
        gpu.mul_lex(x3[0], 1.0, x3[1], x3[0])
    assert e.value.code == F.FHE_EDEPTH


# ---------------------------------------------------------- operator level --
LS = (2, 3)


def oracle_case(N, seed):
    """the oracle half of a fixture (no GPU): contexts, inputs and expected ranks"""
    depth, rots = O.size_parameters(N)
    depth += max(LS) - 1  # the lexicographic rank ends L - 1 levels below the plain one
    orc = O.Context(12, depth, 40, 60, 3, seed=seed)
    orc.gen_rotation_keys(rots)
    cfg, eps = M.sign_cfg(N), 1.0 / N
    d = dict(N=N, seed=seed, orc=orc, depth=depth, rots=rots, cfg=cfg, eps=eps, keys={}, okeys={}, oranks={})
    for L in LS:
        for tb in (True, False):
            # tied tuples with the tie-break, pairwise-distinct ones without it
            keys = X.tied_keys(N, L, X.KEY_SEED[(N, L)]) if tb else X.distinct_keys(N, L, 40 + L)
            okeys = [orc.encrypt(k, N) for k in keys]
            d['keys'][(L, tb)], d['okeys'][(L, tb)] = keys, okeys
            d['oranks'][(L, tb)] = X.oracle_lex_rank(orc, okeys, N, rots, cfg, eps, eps if tb else 0.0)
    return d


def oracle_errors(d):
    """largest |decrypted - exact rank| of the oracle composition per (L, tie-break)"""
    return {k: float(np.max(np.abs(r.decrypt() - X.exact_ranks(d['keys'][k])))) for k, r in d['oranks'].items()}


def _lex_ctx(N, seed):
    d = oracle_case(N, seed)
    gpu = F.Context(12, d['depth'], 40, 60, 3, seed=seed, keygen=False)
    gpu.load_keys_from(d['orc'], d['rots'])
    d.update(gpu=gpu, gkeys={k: [gpu.from_oracle(c) for c in v] for k, v in d['okeys'].items()})
    return d


@pytest.fixture(scope='module')
def n8():
    """one comparator batch"""
    d = _lex_ctx(8, 828)
    assert M.rank_shape(8, d['orc'].n // 2)[2] == 1
    for L in LS:  # rows tied on every key are present
        assert len(np.unique(np.stack(d['keys'][(L, True)], 1), axis=0)) < 8
    return d


@pytest.fixture(scope='module')
def n64():
    """N = 64 at ring 2^12: 2048 slots, two comparator batches (the stacked path)"""
    d = _lex_ctx(64, 884)
    assert M.rank_shape(64, d['orc'].n // 2)[2] == 2
    return d


def _lex_rank(d, L, tb, stack=32, lanes=2, cache=True):
    gpu = d['gpu']
    gpu.set_sort_stack(stack)
    gpu.set_sort_lanes(lanes)
    gpu.set_mask_cache(cache)
    gpu.set_sort_tiebreak(d['eps'] if tb else 0.0)
    try:
        return gpu.lex_rank(d['gkeys'][(L, tb)], d['eps'], d['N'], d['rots'], d['cfg'])
    finally:
        gpu.set_sort_tiebreak(0.0)
        gpu.set_mask_cache(True)
        gpu.set_sort_lanes(2)
        gpu.set_sort_stack(32)


@pytest.mark.parametrize('cache', [True, False], ids=['cached', 'uncached'])
@pytest.mark.parametrize('lanes', [1, 2])
@pytest.mark.parametrize('stack', [1, 32])
@pytest.mark.parametrize('tb', [True, False], ids=['tiebreak', 'distinct'])
@pytest.mark.parametrize('L', LS)
@pytest.mark.parametrize('which', ['n8', 'n64'])
def test_lex_rank_matches_oracle_composition(request, which, L, tb, stack, lanes, cache):
    d = request.getfixturevalue(which)
    with F.KernelClock(d['gpu']) as clk:
        rank = _lex_rank(d, L, tb, stack, lanes, cache)
    for name in KERNELS:
        assert has(clk, name), (name, sorted(clk.stats))
    same(rank, d['oranks'][(L, tb)])
    assert rank.level == F.lex_rank_levels(0, L, d['cfg'])


def test_decrypted_ranks_are_the_lexsort_ranks(n8, n64):
    for d in (n8, n64):
        for L in LS:
            for tb in (True, False):
                keys = d['keys'][(L, tb)]
                want = X.exact_ranks(keys)
                assert not np.array_equal(want, M.stable_ranks(keys[-1]))  # the leading keys decide
                err = float(np.max(np.abs(d['gpu'].decrypt(_lex_rank(d, L, tb)) - want)))
                ref = ORACLE_ERR[(d['N'], L, tb)]
                print(f"N={d['N']} L={L} tiebreak={tb}: max error {err:.3e} (oracle composition {ref:.3e})")
                assert err <= 4 * ref


def test_lex_sort_columns_orders_records_by_two_keys(n8):
    """the rank feeds the record sort as any rank does: each column word for word
    direct_sort(mode 2) of the oracle on that rank, and in np.lexsort order"""
    d = n8
    gpu, orc, N, L = d['gpu'], d['orc'], d['N'], 2
    keys = d['keys'][(L, True)]
    rng = np.random.default_rng(5)
    vals = [rng.uniform(-1, 1, N), np.arange(N) / N]
    ocols = [orc.encrypt(v, N) for v in vals]
    gpu.set_sort_tiebreak(d['eps'])
    try:
        outs = gpu.lex_sort_columns(d['gkeys'][(L, True)], [gpu.from_oracle(c) for c in ocols], d['eps'], N, d['rots'],
                                    d['cfg'])
    finally:
        gpu.set_sort_tiebreak(0.0)
    order = np.lexsort(keys[::-1])
    for g, oc, v in zip(outs, ocols, vals):
        same(g, orc.direct_sort(oc, N, d['rots'], d['cfg'], mode=2, rank=d['oranks'][(L, True)]))
        assert np.max(np.abs(gpu.decrypt(g) - v[order])) < 0.01  # DirectSortTest's bound


CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import fhesort as F
import pyoracle as O
work, N, seed, depth, L = sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6]), int(sys.argv[7])
cfg = (3, 2, 2) if N <= 16 else (3, 3, 2)
_, rots = O.size_parameters(N)
orc = O.Context(12, depth, 40, 60, 3, seed=seed)
orc.gen_rotation_keys(rots)
gpu = F.Context(12, depth, 40, 60, 3, seed=seed, keygen=False)
gpu.load_keys_from(orc, rots)
meta = np.load(work + '/meta.npy')
cts = [gpu.upload(np.load(work + f'/in{i}.npy'), int(meta[i][0]), N, meta[i][1]) for i in range(len(meta))]
gpu.set_sort_stack(32)
gpu.set_sort_lanes(1)
gpu.set_sort_tiebreak(1.0 / N)
with F.KernelClock(gpu) as clk:
    rank = gpu.lex_rank(cts[:L], 1.0 / N, N, rots, cfg)
assert not any(k.startswith(('k_sub_lex_stacked', 'k_tensor_lex')) for k in clk.stats), sorted(clk.stats)
np.save(work + '/out.npy', rank.data())
inf = rank.info()
np.save(work + '/out_meta.npy', np.array([inf['level'], inf['slots'], inf['scale']], dtype=np.float64))
print('ALLOK')
'''


def test_plain_form_gives_the_same_words(n64, tmp_path):
    """FHE_LEX_FUSED=0 (read once per process, so a fresh child): sub_stacked with
    add_const per key, and sub / add_const ahead of every product"""
    d, L = n64, 3
    ins = d['okeys'][(L, True)]
    np.save(tmp_path / 'meta.npy', np.array([[c.info()['level'], c.info()['scale']] for c in ins], dtype=np.float64))
    for i, c in enumerate(ins):
        np.save(tmp_path / f'in{i}.npy', c.data())
    env = dict(os.environ, FHE_LEX_FUSED='0')
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'),
                        os.path.join(REPO, 'oracle'), str(tmp_path), str(d['N']), str(d['seed']), str(d['depth']), str(L)],
                       env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
    o = d['oranks'][(L, True)]
    oi = o.info()
    assert np.load(tmp_path / 'out_meta.npy').tolist() == [oi['level'], oi['slots'], oi['scale']]
    assert np.array_equal(np.load(tmp_path / 'out.npy'), o.data())


# --------------------------------------------------------------- refusals --
def _raw_call(gpu, keys, nkeys, eps, N, rots, cfg):
    """fhe_direct_lex_rank itself: (status, the handle it left, the message)"""
    r = np.asarray(rots, dtype=np.int32)
    arr = (C.c_void_p * max(1, len(keys)))(*[None if k is None else k.h for k in keys])
    out = C.c_void_p(0xdead)
    rc = F.lib().fhe_direct_lex_rank(gpu.h, arr, nkeys, eps, N, F._int(r), len(r), cfg[0], cfg[1], cfg[2], C.byref(out))
    return rc, out.value, F.lib().fhe_last_error().decode()


def test_refusals(n8):
    d = n8
    gpu, N, rots, cfg, eps = d['gpu'], d['N'], d['rots'], d['cfg'], d['eps']
    k = d['gkeys'][(3, True)]
    wide = gpu.encrypt(np.zeros(2 * N), 2 * N)
    deeper = gpu.level_adjust(k[1], 1)
    stacked = gpu.stack([k[0], k[1]])
    cases = [
        ('one key', k[:1], 1, eps, 'nkeys'),
        ('five keys', k + k[:2], 5, eps, 'nkeys'),
        ('null key', [k[0], None], 2, eps, 'key 1'),
        ('null first key', [None, k[1]], 2, eps, 'key 0'),
        ('key is a stack', [k[0], k[1], stacked], 3, eps, 'key 2'),
        ('key slots', [k[0], wide], 2, eps, 'key 1'),
        ('key levels', [k[0], k[1], deeper], 3, eps, 'key 2'),
        ('eps = 0', k[:2], 2, 0.0, 'eps'),
        ('eps = 0.5', k[:2], 2, 0.5, 'eps'),
        ('eps nan', k[:2], 2, float('nan'), 'eps'),
    ]
    for what, keys, nkeys, e, names in cases:
        rc, out, msg = _raw_call(gpu, keys, nkeys, e, N, rots, cfg)
        assert rc == F.FHE_EINVAL, (what, rc, msg)
        assert out is None, what  # the handle is still null
        assert names in msg, (what, msg)


@pytest.mark.parametrize('L', LS)
def test_a_context_one_level_short_is_refused(n8, L):
    """keys so deep that the rank would end one level past the context's last: FHE_EDEPTH before any work"""
    d = n8
    gpu, N = d['gpu'], d['N']
    level = d['depth'] + 1 - F.lex_rank_levels(0, L, d['cfg'])  # rank_level(level) = depth + 1
    assert level >= 1 and F.lex_rank_levels(level, L, d['cfg']) == d['depth'] + 1
    keys = [gpu.encrypt(np.arange(N) / N, N, level) for _ in range(L)]
    with F.KernelClock(gpu) as clk:
        rc, out, msg = _raw_call(gpu, keys, L, d['eps'], N, d['rots'], d['cfg'])
    assert rc == F.FHE_EDEPTH, (rc, msg)
    assert out is None
    assert not clk.stats, sorted(clk.stats)  # no kernel ran


def test_shallow_context_is_refused(small):
    _, gpu, vals = small
    _, rots = O.size_parameters(8)
    key = gpu.encrypt(np.arange(8) / 8.0, 8)
    rc, out, msg = _raw_call(gpu, [key, key], 2, 1.0 / 8, 8, rots, (3, 2, 2))
    assert rc == F.FHE_EDEPTH, (rc, msg)
    assert out is None


# ---------------------------------------------------- the sort is untouched --
def test_sort_after_lex_rank_reproduces_the_oracle(n8):
    """the keys share the sorter's masks; the plain rank and sort are undisturbed"""
    d = n8
    gpu, orc, N = d['gpu'], d['orc'], d['N']
    same(_lex_rank(d, 2, True), d['oranks'][(2, True)])
    ok, gk = d['okeys'][(2, False)][-1], d['gkeys'][(2, False)][-1]
    same(gpu.direct_sort(gk, N, d['rots'], d['cfg']), orc.direct_sort(ok, N, d['rots'], d['cfg']))
    same(_lex_rank(d, 2, True, cache=False), d['oranks'][(2, True)])
