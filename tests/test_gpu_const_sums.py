"""Constant sums of products at worst-case words, against the exact model.

The layer that multiplies ciphertext words by scalar constants and sums the
products -- every Paterson-Stockmeyer leaf of every series -- is otherwise
tested through cheb() and real encryptions only: uniformly random words and
constants of about 2^40.  Here the multi-output sums run through
Context.linear_sums_raw (fhe_linear_sums_raw: linear_sums_to behind its
doubles, so a constant can be any chosen residue) on the shapes, words and
constants of tests/const_sums_cases.py, and every word is compared with
bigint_model.linear_sums, plain Python integers.  No tolerance anywhere.

  * shapes (m sources, G outputs) from (1, 1) to the launch maximum (64, 32),
    (65, 3) beyond it and (12, 33) in two passes; stacks of 1 and 3 members,
    ell = 2 .. 6, sources with more limbs than the sum, with and without the
    constants folded in ahead of a rescale; rings 2^10 (all shapes) and 2^12;
    40-, 41- and 59-bit scaling;
  * words: zero, q - 1, alternating, q/2, q/2 + 1, a ramp, uniform, and words
    aimed byte by byte at one int32 row pair of the MFMA kernels
    (bigint_model.target_words); constants 0, +-1, +-2^62, shifts 1, 7 and 40,
    uniform 62-bit, and the residues whose balanced digits are all -128;
  * kernel forms: the default k_leaf_sums_fold (names asserted), the VALU
    k_linear_sum_multi (set_mfma_sums(0)), and in one child process each
    FHE_LEAF_SIX=0 (eight-digit rows on every prime) and FHE_LEAF_FOLD=0
    (k_leaf_sums_mfma).  The parent builds inputs and expectations, a child
    only runs the engine and writes what it got.

What each case is for is asserted from the model before the GPU is asked
(const_sums_cases.Case.check_conditions, and reach() below): the VALU middle
sum carries out of 64 bits, a window row equals 7 2^14 m exactly, the targeted
words drive the fold kernel's largest int32 pair to at least four times what
uniform words reach.

The public constant ops (add_const, mul_const, mul_const_to, mul_int,
level_adjust, linear_sum_to, mul_add_const, the mul_plain_sum family) follow
at ring 2^12 against the model's definitions."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bigint_model as M
import const_sums_cases as CS
import fhesort as F
import pyoracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


@pytest.fixture(autouse=True)
def mfma_on():
    prev = F.set_mfma_sums(7)
    yield
    F.set_mfma_sums(prev)


_ctx, _expected = {}, {}


def context(key):
    if key not in _ctx:
        logN, L, bits, seed = CS.CONTEXTS[key]
        _ctx[key] = F.Context(logN, L, bits, 60, 3, seed=seed, keygen=False)
    return _ctx[key]


def cases(key):
    gpu = context(key)
    return CS.cases(key, gpu.primes, gpu.nq)


def expected(case):
    """the model's words [G][members][2][ell][n], computed once per case"""
    k = (case.key, case.idx)
    if k not in _expected:
        _expected[k] = np.stack([np.stack(row) for row in case.expected()])
    return _expected[k]


def compare(case, got, names, form):
    want = expected(case)
    assert got.shape == want.shape, (case.name, got.shape, want.shape)
    for g in range(case.G):
        assert np.array_equal(got[g], want[g]), f'{case.name}, {form}, output {g}: {CS.first_difference(got[g], want[g])}'
    assert set(names) == CS.expected_names(case, form), (case.name, form, sorted(names))


def run(case, form):
    gpu = context(case.key)
    got, names = CS.run_case(F, gpu, case.xs, case.xlevels, case.members, case.K, case.sh, case.consts, case.level)
    compare(case, got, names, form)


KEYS = list(CS.CONTEXTS)


# ------------------------------------------------------------ the inputs ---
@pytest.mark.parametrize('key', KEYS)
def test_inputs_reach_what_they_are_for(key):
    """from the model alone: prime classes, large-constant forms, and the reach
    of the targeted words in the fold kernel's int32 pairs"""
    gpu = context(key)
    bits = CS.CONTEXTS[key][2]
    q = [int(p) for p in gpu.primes[:gpu.nq]]
    assert q[0] > 1 << 59
    fp = [p < (1 << 41) for p in q[1:]]
    assert all(fp) if bits == 40 else (any(fp) and not all(fp)) if bits == 41 else not any(fp), (key, q)
    cs = cases(key)
    assert any(s > 0 for c in cs for r in c.sh for s in r)
    assert any(M.const_residue(c.K[0][0], c.sh[0][0], q[0]) == q[0] - 1 and c.K[0][0] < 0 for c in cs)
    for c in cs:
        if c.words != 'target':
            continue
        for l in (0, 1):
            tgt, rnd = c.reach('fold', l, 0, outputs=4)
            wt, wr = c.reach('window', l, 1, outputs=4)
            print(f'{c.name} limb {l}: fold pair {tgt} = {tgt / 2 ** 31:.3f} of 2^31 (uniform words {rnd}); '
                  f'window pair {wt} = {wt / 2 ** 31:.3f} (uniform {wr})')
            assert tgt <= M.budget_bound_fold(c.m) < 2 ** 31 and wt <= M.budget_bound_window(c.m) < 2 ** 31
            if c.m >= 56:
                assert tgt >= 4 * rnd, (c.name, l, tgt, rnd)
                assert wt >= 4 * wr, (c.name, l, wt, wr)


# ------------------------------------------------------ the kernel forms ---
@pytest.mark.parametrize('key', KEYS)
def test_default_kernels(key):
    """k_leaf_sums_fold<KS, NG> up to 64 sources (the six-digit rows on primes
    below 2^41 where KS <= 7 and NG >= 2), k_linear_sum_multi beyond"""
    for case in cases(key):
        run(case, 'fold')


@pytest.mark.parametrize('key', KEYS)
def test_valu_kernels(key):
    F.set_mfma_sums(0)
    for case in cases(key):
        run(case, 'valu')


CHILD = r'''
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import fhesort as F
import const_sums_cases as CS
src, dst = sys.argv[3], sys.argv[4]
F.set_mfma_sums(7)
data = np.load(src)
meta = json.loads(bytes(data['meta']).decode())
ctx, out, names = {}, {}, []
for ci, c in enumerate(meta):
    if c['key'] not in ctx:
        logN, L, bits, seed = CS.CONTEXTS[c['key']]
        ctx[c['key']] = F.Context(logN, L, bits, 60, 3, seed=seed, keygen=False)
    xs = [data[f'c{ci}_x{i}'] for i in range(c['m'])]
    consts = (data[f'c{ci}_Kc'], data[f'c{ci}_shc']) if c['consts'] else None
    got, ks = CS.run_case(F, ctx[c['key']], xs, c['xlevels'], c['members'], data[f'c{ci}_K'], data[f'c{ci}_sh'],
                          consts, c['level'])
    out[f'c{ci}_o'] = got
    names.append(sorted(ks))
out['names'] = np.frombuffer(json.dumps(names).encode(), dtype=np.uint8)
np.savez(dst, **out)
print('ALLOK')
'''

SWITCHES = ('FHE_LEAF_SIX', 'FHE_LEAF_FOLD', 'FHE_MFMA')


@pytest.fixture(scope='module')
def child_inputs(tmp_path_factory):
    root = tmp_path_factory.mktemp('const_sums')
    every = [c for key in KEYS for c in cases(key)]
    CS.save_inputs(str(root / 'inputs.npz'), every)
    return root, every


def run_child(child_inputs, form, **switches):
    root, every = child_inputs
    dst = str(root / f'out_{"_".join(switches)}.npz')
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'), HERE,
                        str(root / 'inputs.npz'), dst], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
    data = np.load(dst)
    names = json.loads(bytes(data['names']).decode())
    for ci, case in enumerate(every):
        compare(case, data[f'c{ci}_o'], names[ci], form)


def test_eight_digit_rows_on_every_prime(child_inputs):
    run_child(child_inputs, 'fold', FHE_LEAF_SIX='0')


def test_window_kernel(child_inputs):
    run_child(child_inputs, 'window', FHE_LEAF_FOLD='0')


# -------------------------------------------------------- what is refused ---
def test_raw_sums_refusals():
    gpu = context('r10-40')
    n, q = gpu.n, [int(p) for p in gpu.primes[:gpu.nq]]
    at = lambda lv: gpu.upload(np.ones((2, gpu.nq - lv, n), dtype=np.uint64), lv, 8)
    a0, a1 = at(0), at(1)
    one = np.zeros((1, 1), dtype=np.uint8)
    for bad in (2 ** 62 + 1, -2 ** 62 - 1, -2 ** 63):
        with pytest.raises(F.FheError) as e:
            gpu.linear_sums_raw([a0], [[bad]], one, 0)
        assert e.value.code == F.FHE_EINVAL
    with pytest.raises(F.FheError) as e:
        gpu.linear_sums_raw([a0], [[1]], one, 0, consts=([2 ** 62 + 1], [0]))
    assert e.value.code == F.FHE_EINVAL
    with pytest.raises(F.FheError) as e:  # an input above the sums' level
        gpu.linear_sums_raw([a1], [[1]], one, 0)
    assert e.value.code == F.FHE_EINVAL
    with pytest.raises(F.FheError) as e:  # mixed batch sizes
        gpu.linear_sums_raw([a0, gpu.stack([a0, a0])], [[1, 1]], np.zeros((1, 2), dtype=np.uint8), 0)
    assert e.value.code == F.FHE_EINVAL
    with pytest.raises(F.FheError):       # no level left to rescale into
        gpu.linear_sums_raw([at(gpu.L)], [[1]], one, gpu.L)
    ok = gpu.linear_sums_raw([a0], [[2 ** 62]], one, 0)[0].data()
    assert np.array_equal(ok, M.linear_sums([np.ones((2, gpu.nq, n), dtype=np.uint64)], [[2 ** 62]], [[0]], q)[0])


# --------------------------------------------------- the public constant ops ---
PATTERNS = {
    'q-1': lambda q, n: np.full(n, q - 1, dtype=np.uint64),
    'alt 0/q-1': lambda q, n: np.where(np.arange(n) % 2 == 0, 0, q - 1).astype(np.uint64),
    'q/2+1': lambda q, n: np.full(n, q // 2 + 1, dtype=np.uint64),
    'ramp': lambda q, n: (np.arange(n, dtype=np.uint64) % np.uint64(q)),
}


def pattern_ct(name, primes, n):
    w = np.stack([PATTERNS[name](int(q), n) for q in primes])
    return np.stack([w, w[:, ::-1]])


@pytest.fixture(scope='module', params=[40, 41, 59], ids=['scale40', 'scale41', 'scale59'])
def trio(request):
    """the contexts of test_gpu_bigint_model.py: ring 2^12, L = 5; the oracle supplies the keys"""
    bits = request.param
    seed = {40: 7, 41: 41, 59: 12}[bits]
    orc = O.Context(12, 5, bits, 60, 3, seed=seed)
    gpu = F.Context(12, 5, bits, 60, 3, seed=seed, keygen=False)
    gpu.load_keys_from(orc, [])
    assert np.array_equal(orc.primes, gpu.primes)
    return orc, gpu, M.Model(12, gpu.primes, gpu.nq, gpu.K, gpu.alpha, gpu.ntt)


def large_constant(m):
    return 1.0e7 if m.q[1] < (1 << 42) else 37.5


def test_public_constant_ops(trio):
    orc, gpu, m = trio
    rng = np.random.default_rng(21)
    delta, level = gpu.delta, 1
    ell = m.nq - level
    big = large_constant(m)
    assert M.const_at_scale(big, delta[level])[1] > 0
    assert M.const_to_target(-big, delta[level + 1], m.q[ell - 1], delta[level])[1] > 0
    data = [('encryption', orc.encrypt(rng.uniform(-1, 1, 8), 8, level).data())]
    data += [(name, pattern_ct(name, m.q[:ell], m.n)) for name in ('q-1', 'alt 0/q-1', 'q/2+1')]
    for j, (name, a) in enumerate(data):
        ga = gpu.upload(a, level, 8)
        sc = ga.info()['scale']
        tag = f'{name}'
        for c in (0.0, -1.0, 0.37, 2.5 / sc, big, -big):
            assert np.array_equal(m.add_const(a, c, sc), gpu.add_const(ga, c).data()), f'add_const {c}, {tag}'
        for c in ((0.0, 0.37, -big), (-2.75, big), (1.0, -big), (-0.5, big))[j]:
            assert np.array_equal(m.mul_const(a, c, sc, level, delta), gpu.mul_const(ga, c).data()), f'mul_const {c}, {tag}'
        c = (-big, 0.37)[j % 2]
        assert np.array_equal(m.mul_const_to(a, c, sc, level + 2, delta), gpu.mul_const_to(ga, c, level + 2).data()), \
            f'mul_const_to {c}, {tag}'
        for k in (0, -1, 2 ** 62, -2 ** 62, 2 ** 40 + 1):
            assert np.array_equal(m.mul_int(a, k), gpu.mul_int(ga, k).data()), f'mul_int {k}, {tag}'
        for t in (level, level + 1 + j % 2):
            assert np.array_equal(m.level_adjust(a, sc, level, t, delta), gpu.level_adjust(ga, t).data()), \
                f'level_adjust to {t}, {tag}'
    # linear_sum_to over both limb counts, every pattern in one sum; the raw hook
    # with the model's (K, sh) of the same doubles, rescaled, gives the same words
    lo = orc.encrypt(rng.uniform(-1, 1, 8), 8, 0)
    xs = [a for _, a in data] + [lo.data()]
    gxs = [gpu.upload(a, level, 8) for _, a in data] + [gpu.from_oracle(lo)]
    scales = [g.info()['scale'] for g in gxs]
    cs = [0.37, -big, 0.0, 2.5, -1.0]
    want = m.linear_sum_to(xs, cs, scales, level + 1, delta)
    assert np.array_equal(want, gpu.linear_sum_to(gxs, cs, level + 1).data()), 'linear_sum_to'
    ks = [M.const_to_target(c, delta[level + 1], m.q[ell - 1], s) for c, s in zip(cs, scales)]
    assert any(s > 0 for _, s in ks)
    raw = gpu.linear_sums_raw(gxs, [[k for k, _ in ks]], [[s for _, s in ks]], level)[0]
    assert np.array_equal(want, gpu.rescale(raw).data()), 'linear_sums_raw + rescale'
    oxs = [orc.ct_from(a, level, 8) for _, a in data] + [lo]
    assert np.array_equal(want, orc.linear_sum_to(oxs, cs, level + 1).data()), 'the oracle agrees'


def test_mul_add_const(trio):
    """(a + a_add + a_const) b + sum c_i x_i + out_const through the tensor
    passes that fold the summands and both constants: 1 and 4 summands (TL_MAX)
    of one limb count, and summands of two limb counts (the separate sum)"""
    orc, gpu, m = trio
    rng = np.random.default_rng(22)
    delta, level = gpu.delta, 1
    ell = m.nq - level
    big = large_constant(m)
    relin = orc.relin_key()
    enc = lambda lv=level: orc.encrypt(rng.uniform(-1, 1, 8), 8, lv).data()
    a, b, a_add = enc(), enc(), pattern_ct('alt 0/q-1', m.q[:ell], m.n)
    summands = [pattern_ct('q-1', m.q[:ell], m.n), enc(), pattern_ct('q/2+1', m.q[:ell], m.n), pattern_ct('ramp', m.q[:ell], m.n)]
    ga, gb, gadd = (gpu.upload(x, level, 8) for x in (a, b, a_add))
    gs = [gpu.upload(x, level, 8) for x in summands]
    sa = ga.info()['scale']
    ks = None
    for what, nx, cs, kw, kernel in [
        ('one summand, both constants', 1, [-big], dict(a_const=0.37, out_const=-2.5), 'k_tensor_lin_c<1>'),
        ('four summands, both constants', 4, [0.5, -big, 0.0, -1.0], dict(a_const=-big, out_const=big), 'k_tensor_lin_c<4>'),
        ('four summands', 4, [big, 1.0, -0.25, 3.0], {}, 'k_tensor_lin<4>'),
        ('constants only', 0, [], dict(a_const=1.5, out_const=-0.125), 'k_tensor_c'),
    ]:
        want, ties, ks = m.mul_add_const(a, b, relin, level, sa, delta, xs=summands[:nx], cs=cs, scales=[sa] * nx, ks=ks, **kw)
        assert len(ties) == 0
        with F.KernelClock(gpu) as clk:
            got = gpu.mul_add_const(ga, gb, gs[:nx], cs, **kw)
        assert kernel in clk.stats, (what, sorted(clk.stats))
        assert np.array_equal(want, got.data()), what
    # a_add changes the left operand's c1: a key switch of its own; summands of two limb counts
    deep = enc(0)
    gdeep = gpu.upload(deep, 0, 8)
    xs, gx = [summands[0], deep, summands[3]], [gs[0], gdeep, gs[3]]
    cs, scales = [-big, 0.75, 1.0], [sa, gdeep.info()['scale'], sa]
    want, ties, _ = m.mul_add_const(a, b, relin, level, sa, delta, xs=xs, cs=cs, scales=scales, a_add=a_add,
                                    a_const=-0.37, out_const=big)
    assert len(ties) == 0
    with F.KernelClock(gpu) as clk:
        got = gpu.mul_add_const(ga, gb, gx, cs, a_add=gadd, a_const=-0.37, out_const=big)
    assert 'k_linear_sum' in clk.stats and 'k_tensor_c' in clk.stats, sorted(clk.stats)
    assert np.array_equal(want, got.data()), 'a_add, both constants, summands of two limb counts'


def test_mul_plain_sums_at_maximal_words(trio):
    """the lazy 128-bit sums of the mul_plain_sum family with every ciphertext
    word and every plaintext word at q - 1: 32 terms (one launch), 33 (the
    accumulate pass), 5 batches (a tile tail), groups"""
    orc, gpu, m = trio
    rng = np.random.default_rng(23)
    level = 3
    ell = m.nq - level
    top = np.stack([np.full(m.n, q - 1, dtype=np.uint64) for q in m.q[:ell]])
    ct_top, rnd = np.stack([top, top]), np.stack([M.rand_limbs(rng, m.q[:ell], m.n) for _ in range(2)])
    g_top, g_rnd, p_top = gpu.upload(ct_top, level, 8), gpu.upload(rnd, level, 8), gpu.upload_pt(top, level, 8)
    p_rnd = M.rand_limbs(rng, m.q[:ell], m.n)
    gp_rnd = gpu.upload_pt(p_rnd, level, 8)
    for terms in (32, 33):
        want = m.mul_plain_sum([ct_top] * terms, [top] * terms)
        assert np.array_equal(want, gpu.mul_plain_sum([g_top] * terms, [p_top] * terms).data()), f'{terms} terms'
    cts, gcts = [ct_top, rnd, ct_top], [g_top, g_rnd, g_top]
    rows = [[top, top, top], [p_rnd, top, p_rnd], [top, p_rnd, top], [p_rnd, p_rnd, p_rnd], [top, top, p_rnd]]
    grow = [[p_top if r is top else gp_rnd for r in row] for row in rows]
    got = gpu.mul_plain_sum_batches(gcts, grow)
    for bi, want in enumerate(m.mul_plain_sum_batches(cts, rows)):
        assert np.array_equal(want, gpu.member(got, bi).data()), f'batch {bi} of 5'
    members, gm = [ct_top, rnd, ct_top, ct_top, ct_top, rnd], [g_top, g_rnd, g_top, g_top, g_top, g_rnd]
    got = gpu.mul_plain_sum_groups(gpu.stack(gm), [p_top, gp_rnd, p_top], 2)
    for gi, want in enumerate(m.mul_plain_sum_groups(members, [top, p_rnd, top], 2)):
        assert np.array_equal(want, gpu.member(got, gi).data()), f'group {gi}'
