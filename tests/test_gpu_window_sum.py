"""Window sums on the GPU (fhe_direct_window_sum).

Kernel level: k_sub_window_stacked and k_tensor_win against the oracle ops they
fuse, member by member and word for word, and the stacked column product with
a zero constant against mul.  Operator level: window_sum against the CPU-oracle
composition of tests/window_model.py, word for word, for 2, 3 and 4 factors --
one partition key with ROWS, LE and BETWEEN, two with GROUP (the self join and
two tables) and LT, three with ROWS -- at N = 8 (one comparator batch) and N = 64
(two: the stacked path), at every chunking, lane count, column grouping and
mask-cache setting and in the plain (unfused) form; decrypted values against
the exact sums; the refusals; and the siblings afterwards.  Oracle results are
computed once per module and shared."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fhesort as F
import group_model as G
import lex_model as X
import pyoracle as O
import running_model as R
import stable_model as M
import window_model as W

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
KERNELS = ('k_sub_window_stacked', 'k_tensor_win')
# case -> (partition keys, mode); 'g2-tables' is GROUP over two tables, the others self joins
CASES = {'g1-rows': (1, W.ROWS), 'g1-le': (1, W.LE), 'g1-between': (1, W.BETWEEN), 'g2-group': (2, W.GROUP),
         'g2-tables': (2, W.GROUP), 'g2-lt': (2, W.LT), 'g3-rows': (3, W.ROWS)}
CASES_64 = tuple(c for c in CASES if c != 'g3-rows')  # four factors at N = 8 only
RUNS = [('n8', c) for c in CASES] + [('n64', c) for c in CASES_64]
RUN_IDS = [f'{w}-{c}' for w, c in RUNS]

# Largest |decrypted - exact| of the CPU-oracle composition on these inputs and
# seeds, per (N, case) (measured on the CPU with oracle_errors below; DESIGN.md
# §6.7).  The GPU words are the oracle's, so this is the GPU's error too; the
# tests assert 4x it, room for another seed's noise, not for a defect: a wrong
# word fails the word comparison first.
ORACLE_ERR = {
    (8, 'g1-rows'): 3.031e-07,
    (8, 'g1-le'): 3.025e-07,
    (8, 'g1-between'): 4.773e-07,
    (8, 'g2-group'): 2.603e-07,
    (8, 'g2-tables'): 7.190e-09,
    (8, 'g2-lt'): 1.303e-07,
    (8, 'g3-rows'): 1.313e-07,
    (64, 'g1-rows'): 1.649e-07,
    (64, 'g1-le'): 1.720e-07,
    (64, 'g1-between'): 8.597e-08,
    (64, 'g2-group'): 1.618e-07,
    (64, 'g2-tables'): 1.439e-07,
    (64, 'g2-lt'): 1.862e-07,
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
    """ring 2^12, L = 3, 40-bit scaling beside the 60-bit q0; 36 vectors, encrypted once per level on first use"""
    orc = O.Context(12, 3, 40, 60, 3, seed=53)
    gpu = F.Context(12, 3, 40, 60, 3, seed=53, keygen=False)
    gpu.load_keys_from(orc, [])
    rng = np.random.default_rng(19)
    vals = [rng.uniform(-1, 1, 16) for _ in range(36)]  # the 36th: the eleventh offset of a second launch
    cache = {}

    def ct(i, level):
        """(oracle ciphertext, its GPU copy) of vals[i] at the level"""
        if (i, level) not in cache:
            o = orc.encrypt(vals[i], 16, level)
            cache[(i, level)] = (o, gpu.from_oracle(o))
        return cache[(i, level)]

    return orc, gpu, vals, ct


def _window_operands(small, G_, B, mode, la, lb):
    """oracle and GPU operands of one sub_window_stacked call"""
    orc, gpu, vals, ct = small
    pa = [ct(g, la) for g in range(G_)]
    pb = [ct(5 + i, lb) for i in range(G_ * B)]
    oa = ct(3, la) if mode != W.GROUP else None
    olo = ct(4, la) if mode == W.BETWEEN else None
    ob = [ct(20 + i, lb) for i in range(B)] if mode != W.GROUP else None
    lv = max(la, lb)
    ps = [(orc.encode(vals[25 + i], 16, lv), gpu.encode(vals[25 + i], 16, lv)) for i in range(B)] if mode == W.ROWS else None
    return pa, pb, oa, olo, ob, ps


def _call_window(gpu, ops, mode, eps):
    pa, pb, oa, olo, ob, ps = ops
    g = lambda x: None if x is None else x[1]
    gl = lambda xs: None if xs is None else [x[1] for x in xs]
    return gpu.sub_window_stacked(gl(pa), gl(pb), eps, mode=mode, order_a=g(oa), order_bs=gl(ob), order_lo=g(olo),
                                  ps=gl(ps))


def _check_window_stack(orc, gpu, Rr, ops, G_, B, mode, eps):
    pa, pb, oa, olo, ob, ps = ops
    V = {W.GROUP: 0, W.BETWEEN: 2}.get(mode, 1)
    with pytest.raises(F.FheError):
        gpu.member(Rr, (2 * G_ + V) * B)
    for g in range(G_):
        for i in range(B):
            d = orc.sub(pa[g][0], pb[g * B + i][0])
            same(gpu.member(Rr, 2 * g * B + i), orc.add_const(d, eps))
            same(gpu.member(Rr, (2 * g + 1) * B + i), orc.add_const(d, -eps))
    for i in range(B if mode != W.GROUP else 0):
        d = orc.sub(oa[0], ob[i][0])
        if mode == W.ROWS:
            want = orc.add_plain(d, ps[i][0])
        else:
            want = orc.add_const(d, -eps if mode == W.LT else eps)
        same(gpu.member(Rr, 2 * G_ * B + i), want)
        if mode == W.BETWEEN:
            same(gpu.member(Rr, (2 * G_ + 1) * B + i), orc.add_const(orc.sub(olo[0], ob[i][0]), -eps))


# five members cross the guarded tail of a thread's four
@pytest.mark.parametrize('B', [1, 4, 5])
@pytest.mark.parametrize('G_', [1, 2, 3])
@pytest.mark.parametrize('mode', [W.GROUP, W.LT, W.ROWS, W.BETWEEN], ids=['none', 'constant', 'offsets', 'two-bounds'])
@pytest.mark.parametrize('la,lb', [(1, 1), (0, 1)], ids=['same-level', 'a-one-level-below'])
def test_sub_window_stacked_matches_oracle(small, la, lb, mode, G_, B):
    orc, gpu = small[0], small[1]
    eps = 1.0 / 16
    ops = _window_operands(small, G_, B, mode, la, lb)
    with F.KernelClock(gpu) as clk:
        Rr = _call_window(gpu, ops, mode, eps)
    assert launches(clk, 'k_sub_window_stacked') == 1, sorted(clk.stats)
    assert not has(clk, 'k_sub_lex_stacked') and not has(clk, 'k_sub_bounds_stacked') and not has(clk, 'k_c0_op')
    _check_window_stack(orc, gpu, Rr, ops, G_, B, mode, eps)


@pytest.mark.parametrize('mode', [W.BETWEEN, W.ROWS], ids=['two-bounds', 'offsets'])
def test_sub_window_stacked_second_launch(small, mode):
    """two partition keys and an order key, 11 members: three slots put min(32 / 3, 16) = 10 in a launch"""
    orc, gpu = small[0], small[1]
    eps, G_, B = 1.0 / 16, 2, 11
    ops = _window_operands(small, G_, B, mode, 1, 1)
    with F.KernelClock(gpu) as clk:
        Rr = _call_window(gpu, ops, mode, eps)
    assert launches(clk, 'k_sub_window_stacked') == 2, sorted(clk.stats)
    _check_window_stack(orc, gpu, Rr, ops, G_, B, mode, eps)


@pytest.mark.parametrize('mode', [W.GROUP, W.LE, W.ROWS, W.BETWEEN], ids=['none', 'constant', 'offsets', 'two-bounds'])
@pytest.mark.parametrize('G_', [1, 3])
def test_sub_window_stacked_with_the_keys_above_the_operands(small, G_, mode):
    """left operands deeper than the bs: every b is adjusted instead, so per-member ops (sub_stacked's rule)"""
    orc, gpu = small[0], small[1]
    eps, B = 0.125, 3
    ops = _window_operands(small, G_, B, mode, 2, 1)
    with F.KernelClock(gpu) as clk:
        Rr = _call_window(gpu, ops, mode, eps)
    assert not has(clk, 'k_sub_window_stacked'), sorted(clk.stats)
    _check_window_stack(orc, gpu, Rr, ops, G_, B, mode, eps)


def test_sub_window_stacked_refusals(small):
    orc, gpu, vals, ct = small
    a1 = [ct(i, 1)[1] for i in range(5)]
    a2 = ct(5, 2)[1]
    b1 = [ct(6 + i, 1)[1] for i in range(4)]
    b2 = ct(10, 2)[1]
    p1, p0 = gpu.encode(vals[11], 16, 1), gpu.encode(vals[11], 16, 0)
    st = gpu.stack([b1[0], b1[1]])
    kw = lambda **k: k
    cases = [
        (a1[:4], b1[:4], kw()),                                                     # four partition keys
        (a1[:1], [b1[0], b2], kw()),                                                # operands at two levels
        ([a1[0], a2], b1[:2], kw()),                                                # keys at two levels
        ([st], b1[:1], kw()),                                                       # a key is a stack
        (a1[:1], [st], kw()),                                                       # an operand is a stack
        (a1[:1], b1[:1], kw(mode=W.LE)),                                            # the mode's order key is missing
        (a1[:1], b1[:1], kw(mode=W.GROUP, order_a=a1[1], order_bs=b1[1:2])),        # an order key in GROUP
        (a1[:1], b1[:1], kw(mode=W.LE, order_a=a1[1], order_bs=b1[1:2], order_lo=a1[2])),  # a bound outside BETWEEN
        (a1[:1], b1[:1], kw(mode=W.BETWEEN, order_a=a1[1], order_bs=b1[1:2])),      # BETWEEN without its bound
        (a1[:1], b1[:1], kw(mode=W.BETWEEN, order_a=a1[1], order_bs=b1[1:2], order_lo=a2)),  # the bound at another level
        (a1[:1], b1[:1], kw(mode=W.ROWS, order_a=a1[1], order_bs=b1[1:2])),         # ROWS without its offsets
        (a1[:1], b1[:1], kw(mode=W.LT, order_a=a1[1], order_bs=b1[1:2], ps=[p1])),  # offsets outside ROWS
        (a1[:1], b1[:1], kw(mode=W.ROWS, order_a=a1[1], order_bs=b1[1:2], ps=[p0])),  # offsets at another level
        (a1[:1], b1[:1], kw(mode=W.LE, order_a=a1[1], order_bs=[b2])),              # order operands at another level
        (a1[:1], b1[:1], kw(mode=5, order_a=a1[1], order_bs=b1[1:2])),              # no such mode
    ]
    for as_, bs, k in cases:
        with pytest.raises(F.FheError) as e:
            gpu.sub_window_stacked(as_, bs, 0.1, **k)
        assert e.value.code == F.FHE_EINVAL, (len(as_), len(bs), sorted(k))
    # operand and offset counts that do not fit never reach the library
    with pytest.raises(ValueError):
        gpu.sub_window_stacked(a1[:2], b1[:3], 0.1)
    with pytest.raises(ValueError):
        gpu.sub_window_stacked(a1[:1], b1[:2], 0.1, mode=W.LE, order_a=a1[1], order_bs=b1[:1])
    o = C.c_void_p()
    arr = (C.c_void_p * 2)(a1[0].h, a1[1].h)
    assert F.lib().fhe_sub_window_stacked(gpu.h, arr, 2, arr, 0, W.GROUP, None, None, None, None, 0.1,
                                          C.byref(o)) == F.FHE_EINVAL  # count 0


def _four(small, B, lu, lu2):
    ct = small[3]
    return ([ct(i, lu) for i in range(B)], [ct(5 + i, lu) for i in range(B)], [ct(10 + i, lu2) for i in range(B)],
            [ct(15 + i, lu2) for i in range(B)])


def _check_mul_sub_sub(small, four, B):
    orc, gpu = small[0], small[1]
    st = lambda xs: gpu.stack([x[1] for x in xs])
    with F.KernelClock(gpu) as clk:
        Rr = gpu.mul_sub_sub(*[st(x) for x in four])
    with pytest.raises(F.FheError):
        gpu.member(Rr, B)
    u, w, u2, w2 = four
    for z in range(B):
        same(gpu.member(Rr, z), orc.mul(orc.sub(u[z][0], w[z][0]), orc.sub(u2[z][0], w2[z][0])))
    return clk


# dnum 3 over the context's 4 primes: level 2 (2 limbs) takes one key-switch digit, level 0 (4 limbs) two
@pytest.mark.parametrize('B', [1, 4, 5])
@pytest.mark.parametrize('level', [2, 0], ids=['one-digit', 'two-digits'])
def test_mul_sub_sub_matches_oracle(small, level, B):
    clk = _check_mul_sub_sub(small, _four(small, B, level, level), B)
    assert launches(clk, 'k_tensor_win') == 1, sorted(clk.stats)
    assert [k for k in clk.stats if k.startswith('k_tensor')] == ['k_tensor_win'], sorted(clk.stats)
    assert 'k_sub' not in clk.stats, sorted(clk.stats)


def test_mul_sub_sub_digit_counts(small):
    """the two levels above really differ in key-switch digits (dnum 3 over the context's primes)"""
    limbs = {lv: small[3](0, lv)[0].info()['limbs'] for lv in (0, 2)}
    alpha = -(-limbs[0] // 3)
    assert -(-limbs[2] // alpha) == 1 and -(-limbs[0] // alpha) == 2, limbs


@pytest.mark.parametrize('lu,lu2', [(0, 1), (2, 1)], ids=['first-below', 'first-above'])
def test_mul_sub_sub_falls_back_when_the_pairs_sit_at_two_levels(small, lu, lu2):
    """the product would level-adjust an operand first: the differences, then the plain product"""
    clk = _check_mul_sub_sub(small, _four(small, 3, lu, lu2), 3)
    assert not has(clk, 'k_tensor_win'), sorted(clk.stats)


def test_mul_sub_sub_refusals(small):
    gpu, ct = small[1], small[3]
    x1 = [ct(i, 1)[1] for i in range(4)]
    x2 = [ct(i, 2)[1] for i in range(2)]
    a, b = gpu.stack(x1[:2]), gpu.stack(x1[2:])
    for u, w, u2, w2 in [(a, x1[0], a, b),              # w holds fewer members
                         (a, b, a, x1[0]),              # w2 holds fewer members
                         (a, b, x1[0], x1[1]),          # the second pair holds fewer members
                         (a, gpu.stack(x2), a, b),      # w at another level than u
                         (a, b, a, gpu.stack(x2))]:     # w2 at another level than u2
        with pytest.raises(F.FheError) as e:
            gpu.mul_sub_sub(u, w, u2, w2)
        assert e.value.code == F.FHE_EINVAL


# the column product of windowSums: the running sums' stacked product with nothing added to the indicator
@pytest.mark.parametrize('B,P', [(1, 1), (4, 3), (5, 5)])
def test_stacked_column_product_with_a_zero_constant_is_mul(small, B, P):
    orc, gpu, vals, ct = small
    oa = [ct(i, 1) for i in range(B)]
    ob = [ct(5 + i, 1) for i in range(P * B)]
    st = lambda xs: gpu.stack([x[1] for x in xs])
    with F.KernelClock(gpu) as clk:
        Rr = gpu.mul_pairs_const(st(oa), 0.0, st(ob), P)
    assert launches(clk, 'k_tensor_run') == 1, sorted(clk.stats)
    for p in range(P):
        for z in range(B):
            same(gpu.member(Rr, p * B + z), orc.mul(oa[z][0], ob[p * B + z][0]))


# ---------------------------------------------------------- operator level --
def oracle_case(N, seed, cases):
    """the oracle half of a fixture (no GPU): contexts, inputs and expected outputs per case"""
    depth, rots = O.size_parameters(N)
    cfg, eps = M.sign_cfg(N), 1.0 / N
    tl, tr, teps, tcfg = W.two_tables(N)
    # size_parameters' depth where window_sum_levels says it suffices, else that depth plus the shortfall
    need = max(F.window_sum_levels(0, W.nfactors(*CASES[c]), tcfg if c == 'g2-tables' else cfg)[1] for c in cases)
    depth = max(depth, need)
    orc = O.Context(12, depth, 40, 60, 3, seed=seed)
    orc.gen_rotation_keys(rots)
    rng = np.random.default_rng(seed)
    vals = [rng.uniform(-1, 1, N), np.arange(N) / N, rng.uniform(-1, 1, N)]
    enc = lambda x, lv=0: None if x is None else orc.encrypt(x, N, lv)
    shallow = [enc(vals[0], 0), enc(vals[1], 1)]  # two of the three columns are shared by every case
    deep = {}
    spec, want = {}, {}
    inputs = {}
    for c in cases:
        Gn, mode = CASES[c]
        ccfg, ceps = (tcfg, teps) if c == 'g2-tables' else (cfg, eps)
        col_max, out_level = F.window_sum_levels(0, W.nfactors(Gn, mode), ccfg)
        if col_max not in deep:
            deep[col_max] = enc(vals[2], col_max)
        ocols = shallow + [deep[col_max]]
        if c == 'g2-tables':
            pl, pr, ol, orr, lo = tl, tr, None, None, None
            opl, opr = [enc(k) for k in pl], [enc(k) for k in pr]
        else:
            if Gn not in inputs:
                parts, t, l, h, e_, c_ = W.partitioned_input(N, Gn)
                assert (e_, c_) == (eps, cfg)
                op = [enc(k) for k in parts]
                inputs[Gn] = (parts, t, l, h, op, enc(t), enc(l), enc(h))
            parts, t, l, h, op, ot, olo_, ohi = inputs[Gn]
            pl = pr = parts
            opl = opr = op
            ol, orr, lo = (None, None, None) if mode == W.GROUP else (h, t, l) if mode == W.BETWEEN else (t, t, None)
        if c == 'g2-tables' or mode == W.GROUP:
            ool = oor = oolo = None
        elif mode == W.BETWEEN:
            ool, oor, oolo = ohi, ot, olo_
        else:
            ool, oor, oolo = ot, ot, None
        spec[c] = dict(mode=mode, eps=ceps, cfg=ccfg, col_max=col_max, out_level=out_level,
                       plain=(pl, pr, ol, orr, lo, vals), oracle=(opl, opr, ool, oor, oolo, ocols))
        want[c] = W.oracle_window_sums(orc, opl, opr, ocols, N, rots, ccfg, ceps, mode, True, ool, oor, oolo)
    return dict(N=N, seed=seed, orc=orc, depth=depth, rots=rots, cfg=cfg, eps=eps, spec=spec, want=want)


def oracle_errors(d):
    """largest |decrypted - exact| of the oracle composition per case"""
    errs = {}
    for case, s in d['spec'].items():
        pl, pr, ol, orr, lo, vals = s['plain']
        wsums, wcnt = W.exact(pl, pr, vals, s['mode'], s['eps'], ol, orr, lo)
        outs, cnt = d['want'][case]
        errs[case] = max(max(np.max(np.abs(o.decrypt() - w)) for o, w in zip(outs, wsums)),
                         np.max(np.abs(cnt.decrypt() - wcnt)))
    return errs


def _win_ctx(N, seed, cases):
    d = oracle_case(N, seed, cases)
    gpu = F.Context(12, d['depth'], 40, 60, 3, seed=seed, keygen=False)
    gpu.load_keys_from(d['orc'], d['rots'])
    up = {}  # every oracle ciphertext uploaded once

    def g(o):
        if o is None:
            return None
        if id(o) not in up:
            up[id(o)] = gpu.from_oracle(o)
        return up[id(o)]

    d['gin'] = {}
    for case, s in d['spec'].items():
        opl, opr, ool, oor, oolo, ocols = s['oracle']
        d['gin'][case] = ([g(k) for k in opl], [g(k) for k in opr], g(ool), g(oor), g(oolo), [g(c) for c in ocols])
    d['gpu'] = gpu
    return d


@pytest.fixture(scope='module')
def n8():
    """one comparator batch"""
    d = _win_ctx(8, 828, tuple(CASES))
    assert M.rank_shape(8, d['orc'].n // 2)[2] == 1
    return d


@pytest.fixture(scope='module')
def n64():
    """N = 64 at ring 2^12: 2048 slots, two comparator batches (the stacked path)"""
    d = _win_ctx(64, 884, CASES_64)
    assert M.rank_shape(64, d['orc'].n // 2)[2] == 2
    return d


def _run(d, case, stack=32, lanes=2, cache=True, members=F.SORT_COLUMN_MEMBERS_DEFAULT, cols=None, count=True):
    gpu, s = d['gpu'], d['spec'][case]
    pl, pr, ol, orr, lo, gcols = d['gin'][case]
    gpu.set_sort_stack(stack)
    gpu.set_sort_lanes(lanes)
    gpu.set_mask_cache(cache)
    gpu.set_sort_column_members(members)
    try:
        return gpu.window_sum(pl, pr, gcols if cols is None else cols, s['eps'], d['N'], d['rots'], s['cfg'],
                              order_left=ol, order_right=orr, mode=s['mode'], lo=lo, count=count)
    finally:
        gpu.set_sort_column_members(F.SORT_COLUMN_MEMBERS_DEFAULT)
        gpu.set_mask_cache(True)
        gpu.set_sort_lanes(2)
        gpu.set_sort_stack(32)


def _check(d, case, outs, cnt):
    wouts, wcnt = d['want'][case]
    out_level = d['spec'][case]['out_level']
    assert len(outs) == len(wouts) == 3
    for g, o in zip(outs, wouts):
        same(g, o)
        assert g.level == out_level and g.slots == d['N']
    same(cnt, wcnt)
    assert cnt.level == out_level and cnt.slots == d['N']


@pytest.mark.parametrize('cache', [True, False], ids=['cached', 'uncached'])
@pytest.mark.parametrize('lanes', [1, 2])
@pytest.mark.parametrize('stack', [1, 32])
@pytest.mark.parametrize('which,case', RUNS, ids=RUN_IDS)
def test_every_case_matches_oracle_composition(request, which, case, stack, lanes, cache):
    d = request.getfixturevalue(which)
    Gn, mode = CASES[case]
    with F.KernelClock(d['gpu']) as clk:
        outs, cnt = _run(d, case, stack, lanes, cache)
    assert has(clk, 'k_sub_window_stacked'), sorted(clk.stats)
    # two partition keys, or a partition key and two bounds, meet in k_tensor_win; s + 1 in k_tensor_lex
    assert has(clk, 'k_tensor_win') == (mode in (W.GROUP, W.BETWEEN) or Gn == 3), sorted(clk.stats)
    assert has(clk, 'k_tensor_lex') == (mode in (W.ROWS, W.LE, W.LT)), sorted(clk.stats)
    assert has(clk, 'k_tensor_run'), sorted(clk.stats)
    assert not has(clk, 'k_sub_lex_stacked') and not has(clk, 'k_sub_bounds_stacked'), sorted(clk.stats)
    _check(d, case, outs, cnt)


@pytest.mark.parametrize('members', [1, 2])
@pytest.mark.parametrize('which,case', [('n8', 'g1-rows'), ('n8', 'g3-rows'), ('n64', 'g1-between'), ('n64', 'g2-lt')])
def test_column_groups_give_the_same_words(request, which, case, members):
    """a member bound below P B splits the three columns over several products"""
    d = request.getfixturevalue(which)
    with F.KernelClock(d['gpu']) as clk:
        outs, cnt = _run(d, case, members=members)
    assert launches(clk, 'k_tensor_run') >= 2, sorted(clk.stats)
    _check(d, case, outs, cnt)


def test_decrypted_values_are_the_exact_sums(n8, n64):
    for d in (n8, n64):
        for case, s in d['spec'].items():
            pl, pr, ol, orr, lo, vals = s['plain']
            outs, cnt = _run(d, case)
            wsums, wcnt = W.exact(pl, pr, vals, s['mode'], s['eps'], ol, orr, lo)
            err = max(max(np.max(np.abs(d['gpu'].decrypt(o) - w)) for o, w in zip(outs, wsums)),
                      np.max(np.abs(d['gpu'].decrypt(cnt) - wcnt)))
            print(f"N={d['N']} {case}: max error {err:.3e} (oracle composition {ORACLE_ERR[(d['N'], case)]:.3e})")
            assert wcnt.min() < d['N'] and wcnt.max() >= 1
            assert err <= 4 * ORACLE_ERR[(d['N'], case)]


def test_count_alone_and_columns_alone(n8):
    d = n8
    for case in ('g1-rows', 'g2-group'):
        outs, cnt = _run(d, case, cols=[], count=True)
        assert outs == []
        same(cnt, d['want'][case][1])
        outs = _run(d, case, cols=d['gin'][case][5][:1], count=False)
        assert len(outs) == 1
        same(outs[0], d['want'][case][0][0])


def test_tiebreak_setting_has_no_effect(n8):
    d = n8
    d['gpu'].set_sort_tiebreak(0.4 / d['N'])  # another eps than the call's own
    try:
        res = {case: _run(d, case) for case in ('g1-rows', 'g2-lt')}
    finally:
        d['gpu'].set_sort_tiebreak(0.0)
    for case, (outs, cnt) in res.items():
        _check(d, case, outs, cnt)


CHILD = r'''
import json
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import fhesort as F
import pyoracle as O
work, N, seed, depth = sys.argv[3], int(sys.argv[4]), int(sys.argv[5]), int(sys.argv[6])
_, rots = O.size_parameters(N)
orc = O.Context(12, depth, 40, 60, 3, seed=seed)
orc.gen_rotation_keys(rots)
gpu = F.Context(12, depth, 40, 60, 3, seed=seed, keygen=False)
gpu.load_keys_from(orc, rots)
meta = np.load(work + '/meta.npy')
cts = [gpu.upload(np.load(work + f'/in{i}.npy'), int(meta[i][0]), N, meta[i][1]) for i in range(len(meta))]
plan = json.load(open(work + '/plan.json'))
pick = lambda i: None if i is None else cts[i]
res = {}
with F.KernelClock(gpu) as clk:
    for case, p in plan.items():
        res[case] = gpu.window_sum([pick(i) for i in p['pl']], [pick(i) for i in p['pr']], [pick(i) for i in p['cols']],
                                   p['eps'], N, rots, tuple(p['cfg']), order_left=pick(p['ol']), order_right=pick(p['or']),
                                   mode=p['mode'], lo=pick(p['lo']), count=True)
assert not any(name.startswith(('k_sub_window_stacked', 'k_tensor_win')) for name in clk.stats), sorted(clk.stats)
for case, (outs, cnt) in res.items():
    for i, o in enumerate(outs + [cnt]):
        np.save(work + f'/out_{case}_{i}.npy', o.data())
        inf = o.info()
        np.save(work + f'/out_{case}_{i}_meta.npy', np.array([inf['level'], inf['slots'], inf['scale']], dtype=np.float64))
print('ALLOK')
'''


def test_plain_form_gives_the_same_words(n64, tmp_path):
    """FHE_WIN_FUSED=0 (read once per process, so a fresh child): sub_stacked with the
    constants in place or the offsets per member, and sub, sub, mul for the products"""
    d = n64
    ins, index, plan = [], {}, {}

    def idx(o):
        if o is None:
            return None
        if id(o) not in index:
            index[id(o)] = len(ins)
            ins.append(o)
        return index[id(o)]

    for case in ('g1-rows', 'g1-between', 'g2-group', 'g2-lt'):
        s = d['spec'][case]
        opl, opr, ool, oor, oolo, ocols = s['oracle']
        plan[case] = dict(pl=[idx(k) for k in opl], pr=[idx(k) for k in opr], ol=idx(ool), lo=idx(oolo), cols=[idx(c) for c in ocols],
                          mode=s['mode'], eps=s['eps'], cfg=list(s['cfg']))
        plan[case]['or'] = idx(oor)
    np.save(tmp_path / 'meta.npy', np.array([[c.info()['level'], c.info()['scale']] for c in ins], dtype=np.float64))
    for i, c in enumerate(ins):
        np.save(tmp_path / f'in{i}.npy', c.data())
    with open(tmp_path / 'plan.json', 'w') as f:
        json.dump(plan, f)
    env = dict(os.environ, FHE_WIN_FUSED='0')
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'),
                        os.path.join(REPO, 'oracle'), str(tmp_path), str(d['N']), str(d['seed']), str(d['depth'])],
                       env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
    for case in plan:
        outs, cnt = d['want'][case]
        for i, o in enumerate(outs + [cnt]):
            oi = o.info()
            assert np.load(tmp_path / f'out_{case}_{i}_meta.npy').tolist() == [oi['level'], oi['slots'], oi['scale']], (case, i)
            assert np.array_equal(np.load(tmp_path / f'out_{case}_{i}.npy'), o.data()), (case, i)


# --------------------------------------------------------------- refusals --
def _raw_call(gpu, pl, pr, ol, lo, orr, cols, ncols, mode, eps, N, rots, cfg, want_count=True, nparts=None):
    """fhe_direct_window_sum itself: (status, the output handles it left, the message)"""
    r = np.asarray(rots, dtype=np.int32)
    h = lambda x: None if x is None else x.h
    arr = lambda xs: (C.c_void_p * max(1, len(xs)))(*[h(x) for x in xs])
    outs = (C.c_void_p * max(1, len(cols)))(*([0xdead] * max(1, len(cols))))
    cnt = C.c_void_p(0xdead)
    rc = F.lib().fhe_direct_window_sum(gpu.h, arr(pl), arr(pr), len(pl) if nparts is None else nparts, h(ol), h(lo), h(orr),
                                       arr(cols), ncols, mode, eps, N, F._int(r), len(r), cfg[0], cfg[1], cfg[2], outs,
                                       C.byref(cnt) if want_count else None)
    left = [outs[i] for i in range(max(ncols, 0))] + ([cnt.value] if want_count else [])
    return rc, left, F.lib().fhe_last_error().decode()


def test_refusals(n8):
    d = n8
    gpu, N, rots, cfg, eps = d['gpu'], d['N'], d['rots'], d['cfg'], d['eps']
    (k0, k1, k2), _, t, _, _, gcols = d['gin']['g3-rows']
    _, _, hi, tw, lo, _ = d['gin']['g1-between']
    col = gcols[0]
    wide = gpu.encrypt(np.zeros(2 * N), 2 * N)
    deeper = gpu.level_adjust(k0, 1)
    stacked = gpu.stack([col, col])
    ROWS, LE, BETWEEN, GROUP = F.WIN_ROWS, F.WIN_LE, F.WIN_BETWEEN, F.WIN_GROUP
    deep2 = gpu.level_adjust(col, F.window_sum_levels(0, 2, cfg)[0] + 1)
    deep4 = gpu.level_adjust(col, F.window_sum_levels(0, 4, cfg)[0] + 1)
    EINVAL, EDEPTH = F.FHE_EINVAL, F.FHE_EDEPTH
    # (what, pl, pr, ol, lo, orr, cols, ncols, mode, eps, want_count, status, word of the message, nparts)
    cases = [
        ('no partition key', [], [], t, None, t, [col], 1, ROWS, eps, True, EINVAL, 'nparts', None),
        ('four partition keys', [k0, k1, k2, k0], [k0, k1, k2, k0], None, None, None, [col], 1, GROUP, eps, True, EINVAL, 'nparts', None),
        ('one factor', [k0], [k0], None, None, None, [col], 1, GROUP, eps, True, EINVAL, 'group_sum', None),
        ('five factors', [k0, k1, k2, k0], [k0, k1, k2, k0], t, None, t, [col], 1, ROWS, eps, True, EINVAL, None, None),
        ('order key with GROUP', [k0, k1], [k0, k1], t, None, t, [col], 1, GROUP, eps, True, EINVAL, 'order', None),
        ('right order key with GROUP', [k0, k1], [k0, k1], None, None, t, [col], 1, GROUP, eps, True, EINVAL, 'order', None),
        ('no order key', [k0], [k0], None, None, None, [col], 1, ROWS, eps, True, EINVAL, 'order', None),
        ('no right order key', [k0], [k0], t, None, None, [col], 1, LE, eps, True, EINVAL, 'order', None),
        ('lo outside BETWEEN', [k0], [k0], t, lo, t, [col], 1, LE, eps, True, EINVAL, 'order_lo', None),
        ('lo in ROWS', [k0], [k0], t, lo, t, [col], 1, ROWS, eps, True, EINVAL, 'order_lo', None),
        ('lo with GROUP', [k0, k1], [k0, k1], None, lo, None, [col], 1, GROUP, eps, True, EINVAL, 'order', None),
        ('lo missing', [k0], [k0], hi, None, tw, [col], 1, BETWEEN, eps, True, EINVAL, 'order_lo', None),
        ('mode 5', [k0], [k0], t, None, t, [col], 1, 5, eps, True, EINVAL, 'mode', None),
        ('mode -1', [k0], [k0], t, None, t, [col], 1, -1, eps, True, EINVAL, 'mode', None),
        ('null partition key', [k0, None], [k0, k1], None, None, None, [col], 1, GROUP, eps, True, EINVAL, 'left partition key 1', None),
        ('null right partition key', [k0, k1], [None, k1], None, None, None, [col], 1, GROUP, eps, True, EINVAL, 'right partition key 0', None),
        ('partition key level', [k0, k1], [k0, gpu.level_adjust(k1, 1)], None, None, None, [col], 1, GROUP, eps, True, EINVAL, 'levels', None),
        ('left keys deeper', [deeper], [k0], t, None, t, [col], 1, ROWS, eps, True, EINVAL, 'levels', None),
        ('order key level', [k0], [k0], gpu.level_adjust(t, 1), None, t, [col], 1, LE, eps, True, EINVAL, 'levels', None),
        ('lo level', [k0], [k0], hi, gpu.level_adjust(lo, 1), tw, [col], 1, BETWEEN, eps, True, EINVAL, 'levels', None),
        ('partition key slots', [k0, wide], [k0, wide], None, None, None, [col], 1, GROUP, eps, True, EINVAL, 'slots', None),
        ('order key slots', [k0], [k0], t, None, wide, [col], 1, LE, eps, True, EINVAL, 'slots', None),
        ('every key wide', [wide], [wide], wide, None, wide, [col], 1, LE, eps, True, EINVAL, 'slots', None),
        ('key is a stack', [k0], [gpu.stack([k0, k0])], t, None, t, [col], 1, LE, eps, True, EINVAL, 'stack', None),
        ('null column', [k0], [k0], t, None, t, [col, None], 2, ROWS, eps, True, EINVAL, 'column 1', None),
        ('column is a stack', [k0], [k0], t, None, t, [col, col, stacked], 3, ROWS, eps, True, EINVAL, 'column 2', None),
        ('column slots', [k0], [k0], t, None, t, [wide, col], 2, ROWS, eps, True, EINVAL, 'column 0', None),
        ('eps = 0', [k0], [k0], t, None, t, [col], 1, ROWS, 0.0, True, EINVAL, 'eps', None),
        ('eps = 0.5', [k0], [k0], t, None, t, [col], 1, ROWS, 0.5, True, EINVAL, 'eps', None),
        ('eps nan', [k0], [k0], t, None, t, [col], 1, ROWS, float('nan'), True, EINVAL, 'eps', None),
        ('negative ncols', [k0], [k0], t, None, t, [col], -1, ROWS, eps, True, EINVAL, 'ncols', None),
        ('nothing asked for', [k0], [k0], t, None, t, [], 0, ROWS, eps, False, EINVAL, None, None),
        ('column too deep, two factors', [k0], [k0], t, None, t, [col, deep2], 2, ROWS, eps, True, EDEPTH, 'column 1', None),
        ('column too deep, four factors', [k0, k1, k2], [k0, k1, k2], t, None, t, [deep4], 1, ROWS, eps, True, EDEPTH, 'column 0', None),
    ]
    for what, pl, pr, ol, l, orr, cols, ncols, mode, e, want_count, status, word, nparts in cases:
        with F.KernelClock(gpu) as clk:
            rc, outs, msg = _raw_call(gpu, pl, pr, ol, l, orr, cols, ncols, mode, e, N, rots, cfg, want_count, nparts)
        assert rc == status, (what, rc, msg)
        assert all(o is None for o in outs), what  # every output handle still null
        assert not clk.stats, (what, sorted(clk.stats))  # refused before any work
        if word:
            assert word in msg, (what, msg)
    # the deepest allowed column is served (it is column 2 of every case of the fixture)
    for case in CASES:
        assert d['spec'][case]['oracle'][5][2].level == d['spec'][case]['col_max']


def test_shallow_context_is_refused(small):
    """a context without out_level levels: FHE_EDEPTH before any work"""
    gpu = small[1]
    _, rots = O.size_parameters(8)
    key = gpu.encrypt(np.arange(8) / 8.0, 8)
    for pl, ol, lo, mode in (([key], key, None, F.WIN_ROWS), ([key], key, key, F.WIN_BETWEEN), ([key, key], None, None, F.WIN_GROUP)):
        with F.KernelClock(gpu) as clk:
            rc, outs, msg = _raw_call(gpu, pl, pl, ol, lo, ol, [key], 1, mode, 1.0 / 8, 8, rots, (3, 2, 2))
        assert rc == F.FHE_EDEPTH, (rc, msg)
        assert all(o is None for o in outs) and not clk.stats


# ------------------------------------------------ the siblings are untouched --
def test_siblings_after_window_sums_reproduce_the_oracle(n8):
    """the columns' masks at L_a - 1 are one more cached set keyed by level; the others are undisturbed"""
    d = n8
    gpu, orc, N, rots, cfg, eps = d['gpu'], d['orc'], d['N'], d['rots'], d['cfg'], d['eps']
    gparts, _, gt, _, _, gcols = d['gin']['g3-rows']
    oparts, _, ot, _, _, ocols = d['spec']['g3-rows']['oracle']
    _check(d, 'g3-rows', *_run(d, 'g3-rows'))
    same(gpu.direct_sort(gt, N, rots, cfg), orc.direct_sort(ot, N, rots, cfg))
    _check(d, 'g1-between', *_run(d, 'g1-between', cache=False))
    wouts, wcnt = G.oracle_group_sums(orc, ot, ot, ocols[:1], N, rots, cfg, eps, True)
    outs, cnt = gpu.group_sum(gt, gt, gcols[:1], eps, N, rots, cfg, count=True)
    same(outs[0], wouts[0])
    same(cnt, wcnt)
    wouts, wcnt = R.oracle_running_sums(orc, ot, ot, ocols[:1], N, rots, cfg, eps, R.ROWS, True)
    outs, cnt = gpu.running_sum(gt, gt, gcols[:1], eps, N, rots, cfg, mode=F.RUN_ROWS, count=True)
    same(outs[0], wouts[0])
    same(cnt, wcnt)
    same(gpu.lex_rank([gparts[0], gt], eps, N, rots, cfg), X.oracle_lex_rank(orc, [oparts[0], ot], N, rots, cfg, eps, 0.0))
    _check(d, 'g2-group', *_run(d, 'g2-group'))
