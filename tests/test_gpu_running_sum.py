"""Running sums on the GPU (fhe_direct_running_sum).

Kernel level: k_sub_bounds_stacked and k_tensor_run against the oracle ops they
fuse, member by member and word for word.  Operator level: running_sum against
the CPU-oracle composition of tests/running_model.py, word for word, in every
mode -- the self join on tied keys (ROWS, LE, LT), the sliding window (BETWEEN)
and two tables (the range lookup) -- at N = 8 (one comparator batch) and N = 64
(two: the stacked path), at every chunking, lane count, column grouping and
mask-cache setting and in the plain (unfused) form; the ROWS count against the
tie-broken rank; decrypted values against the exact sums.  Oracle results are
computed once per module and shared."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fhesort as F
import group_model as G
import pyoracle as O
import running_model as R
import stable_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
KERNELS = ('k_sub_bounds_stacked', 'k_tensor_run')
CASES = ('rows', 'le', 'lt', 'between', 'join')  # the four modes, and LE over two tables

# Largest |decrypted - exact| of the CPU-oracle composition on these inputs and
# seeds, per (N, case) (measured on the CPU with oracle_errors below; DESIGN.md
# §6.6).  The GPU words are the oracle's, so this is the GPU's error too; the
# tests assert 4x it, room for another seed's noise, not for a defect: a wrong
# word fails the word comparison first.
ORACLE_ERR = {
    (8, 'rows'): 9.317e-09,
    (8, 'le'): 4.811e-08,
    (8, 'lt'): 6.102e-08,
    (8, 'between'): 2.656e-07,
    (8, 'join'): 9.336e-09,
    (64, 'rows'): 3.030e-07,
    (64, 'le'): 3.044e-07,
    (64, 'lt'): 3.204e-07,
    (64, 'between'): 1.831e-07,
    (64, 'join'): 1.866e-07,
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
    """ring 2^12, L = 3, 40-bit scaling beside the 60-bit q0; 35 encrypted vectors (test_gpu_group_sum's)"""
    orc = O.Context(12, 3, 40, 60, 3, seed=47)
    gpu = F.Context(12, 3, 40, 60, 3, seed=47, keygen=False)
    gpu.load_keys_from(orc, [])
    rng = np.random.default_rng(17)
    vals = [rng.uniform(-1, 1, 16) for _ in range(35)]
    return orc, gpu, vals


def _check_sub_bounds(small, B, V, la, lb, nlaunch):
    orc, gpu, vals = small
    consts = [1.0 / 16, -1.0 / 16][:V]
    oas = [orc.encrypt(v, 16, la) for v in vals[0:V]]
    obs = [orc.encrypt(v, 16, lb) for v in vals[2:2 + B]]
    with F.KernelClock(gpu) as clk:
        Rr = gpu.sub_bounds_stacked([gpu.from_oracle(a) for a in oas], [gpu.from_oracle(b) for b in obs], consts)
    assert launches(clk, 'k_sub_bounds_stacked') == nlaunch, sorted(clk.stats)
    with pytest.raises(F.FheError):
        gpu.member(Rr, V * B)
    for v in range(V):
        for i in range(B):
            same(gpu.member(Rr, v * B + i), orc.add_const(orc.sub(oas[v], obs[i]), consts[v]))


# five members cross the guarded tail of a thread's four
@pytest.mark.parametrize('B', [1, 4, 5])
@pytest.mark.parametrize('V', [1, 2], ids=['one-bound', 'two-bounds'])
@pytest.mark.parametrize('la,lb', [(1, 1), (0, 1)], ids=['same-level', 'a-one-level-below'])
def test_sub_bounds_stacked_matches_oracle(small, B, V, la, lb):
    _check_sub_bounds(small, B, V, la, lb, 1)


def test_sub_bounds_stacked_second_launch(small):
    """33 members under two bounds: a launch takes 32, each bound's members stay 33 apart"""
    _check_sub_bounds(small, 33, 2, 1, 1, 2)


def test_sub_bounds_stacked_with_a_above_the_operands(small):
    """a deeper than the bs: every b is adjusted instead, so per-member ops (sub_stacked's rule)"""
    orc, gpu, vals = small
    consts = [-0.25, 0.125]
    oas = [orc.encrypt(v, 16, 2) for v in vals[0:2]]
    obs = [orc.encrypt(v, 16, 1) for v in vals[2:5]]
    with F.KernelClock(gpu) as clk:
        Rr = gpu.sub_bounds_stacked([gpu.from_oracle(a) for a in oas], [gpu.from_oracle(b) for b in obs], consts)
    assert not has(clk, 'k_sub_bounds_stacked'), sorted(clk.stats)
    for v in range(2):
        for i in range(3):
            same(gpu.member(Rr, v * 3 + i), orc.add_const(orc.sub(oas[v], obs[i]), consts[v]))


def test_sub_bounds_stacked_refusals(small):
    orc, gpu, vals = small
    a, a2 = gpu.encrypt(vals[0], 16, 1), gpu.encrypt(vals[3], 16, 2)
    b1, b2 = gpu.encrypt(vals[1], 16, 1), gpu.encrypt(vals[2], 16, 2)
    cases = [([a], [b1, b2], [0.1]),                  # operands at two levels
             ([a], [gpu.stack([b1, b1])], [0.1]),     # an operand is a stack
             ([gpu.stack([a, a])], [b1], [0.1]),      # a left operand is a stack
             ([a, a2], [b1], [0.1, 0.1]),             # left operands at two levels
             ([a], [], [0.1]),                        # no operand
             ([a, a, a], [b1], [0.1, 0.1, 0.1]),      # three bounds
             ([], [b1], [])]                          # no bound
    for as_, bs, cs in cases:
        with pytest.raises(F.FheError) as e:
            gpu.sub_bounds_stacked(as_, bs, cs)
        assert e.value.code == F.FHE_EINVAL
    with pytest.raises(ValueError):
        gpu.sub_bounds_stacked([a, a], [b1], [0.1])  # one constant per left operand


# five columns cross the guarded tail of a thread's four; five members leave the tile of the differences
@pytest.mark.parametrize('P', [1, 4, 5])
@pytest.mark.parametrize('B', [1, 4, 5])
@pytest.mark.parametrize('form', ['const', 'sub'])
def test_mul_pairs_left_matches_oracle(small, form, B, P):
    orc, gpu, vals = small
    oa = [orc.encrypt(v, 16, 1) for v in vals[0:B]]
    ow = [orc.encrypt(v, 16, 1) for v in vals[5:5 + B]]
    ob = [orc.encrypt(v, 16, 1) for v in vals[10:10 + P * B]]
    st = lambda xs: gpu.stack([gpu.from_oracle(x) for x in xs])
    with F.KernelClock(gpu) as clk:
        Rr = gpu.mul_pairs_const(st(oa), 1.0, st(ob), P) if form == 'const' else gpu.mul_pairs_sub(st(oa), st(ow), st(ob), P)
    assert launches(clk, 'k_tensor_run') == 1, sorted(clk.stats)
    assert not has(clk, 'k_tensor_pairs') and not has(clk, 'k_tensor_cols') and not has(clk, 'k_c0_op')
    with pytest.raises(F.FheError):
        gpu.member(Rr, P * B)
    for p in range(P):
        for z in range(B):
            left = orc.add_const(oa[z], 1.0) if form == 'const' else orc.sub(oa[z], ow[z])
            same(gpu.member(Rr, p * B + z), orc.mul(left, ob[p * B + z]))


def test_mul_pairs_left_refusals(small):
    orc, gpu, vals = small
    x1 = [gpu.encrypt(v, 16, 1) for v in vals[:4]]
    x2 = [gpu.encrypt(v, 16, 2) for v in vals[:4]]
    a, w, b = gpu.stack(x1[:2]), gpu.stack(x1[2:]), gpu.stack(x1)
    for aa, ww, bb, ncols in [(a, x1[0], b, 2),              # a_sub holds fewer members
                              (a, gpu.stack(x2[:2]), b, 2),  # a_sub at another level
                              (a, w, b, 3),                  # b is not ncols columns of B
                              (a, w, gpu.stack(x2), 2),      # b at another level
                              (a, w, b, 0)]:                 # P < 1
        with pytest.raises(F.FheError) as e:
            gpu.mul_pairs_sub(aa, ww, bb, ncols)
        assert e.value.code == F.FHE_EINVAL, ncols
    for aa, bb, ncols in [(a, b, 3), (a, gpu.stack(x2), 2), (a, b, 0), (a, b, -1)]:
        with pytest.raises(F.FheError) as e:
            gpu.mul_pairs_const(aa, 1.0, bb, ncols)
        assert e.value.code == F.FHE_EINVAL, ncols


# ---------------------------------------------------------- operator level --
def oracle_case(N, seed):
    """the oracle half of a fixture (no GPU): contexts, inputs and expected outputs per case"""
    depth, rots = O.size_parameters(N)
    orc = O.Context(12, depth, 40, 60, 3, seed=seed)
    orc.gen_rotation_keys(rots)
    cfg, eps = M.sign_cfg(N), 1.0 / N
    rng = np.random.default_rng(seed)
    # three columns entering at levels 0, 1 and the deepest allowed, shared by the four modes
    vals = [rng.uniform(-1, 1, N), np.arange(N) / N, rng.uniform(-1, 1, N)]
    col_max, out_level = F.group_sum_levels(0, cfg)
    ocols = [orc.encrypt(v, N, lv) for v, lv in zip(vals, (0, 1, col_max))]
    k = M.tied_input(N, M.SEEDS[N])  # the self join: tied keys
    ok = orc.encrypt(k, N)
    kw, lo, hi, weps, wcfg = R.window_input(N)  # the sliding window
    assert (weps, wcfg) == (eps, cfg)
    okw, olo, ohi = orc.encrypt(kw, N), orc.encrypt(lo, N), orc.encrypt(hi, N)
    kl, kr, jeps, jcfg = G.lookup_tables(N, seed + 1)  # two tables: the range lookup, one column
    jv = rng.uniform(-1, 1, N)
    okl, okr, ojv = orc.encrypt(kl, N), orc.encrypt(kr, N), orc.encrypt(jv, N)
    # case -> (mode, plaintext (kl, kr, lo, cols), oracle (kl, kr, lo, cols), eps, cfg)
    spec = {
        'rows': (R.ROWS, (k, k, None, vals), (ok, ok, None, ocols), eps, cfg),
        'le': (R.LE, (k, k, None, vals), (ok, ok, None, ocols), eps, cfg),
        'lt': (R.LT, (k, k, None, vals), (ok, ok, None, ocols), eps, cfg),
        'between': (R.BETWEEN, (hi, kw, lo, vals), (ohi, okw, olo, ocols), eps, cfg),
        'join': (R.LE, (kl, kr, None, [jv]), (okl, okr, None, [ojv]), jeps, jcfg),
    }
    want = {}
    for case, (mode, _, (a, b, l, cols), e, c) in spec.items():
        want[case] = R.oracle_running_sums(orc, a, b, cols, N, rots, c, e, mode, True, l)
    return dict(N=N, seed=seed, orc=orc, depth=depth, rots=rots, cfg=cfg, eps=eps, col_max=col_max, out_level=out_level,
                spec=spec, want=want, k=k, ok=ok)


def oracle_errors(d):
    """largest |decrypted - exact| of the oracle composition per case"""
    errs = {}
    for case, (mode, (kl, kr, lo, vals), _, eps, _) in d['spec'].items():
        wsums, wcnt = R.exact(kl, kr, vals, mode, eps, lo)
        outs, cnt = d['want'][case]
        errs[case] = max(max(np.max(np.abs(o.decrypt() - w)) for o, w in zip(outs, wsums)),
                         np.max(np.abs(cnt.decrypt() - wcnt)))
    return errs


def _run_ctx(N, seed):
    d = oracle_case(N, seed)
    gpu = F.Context(12, d['depth'], 40, 60, 3, seed=seed, keygen=False)
    gpu.load_keys_from(d['orc'], d['rots'])
    up = {}  # every oracle ciphertext uploaded once

    def g(o):
        if o is None:
            return None
        if id(o) not in up:
            up[id(o)] = gpu.from_oracle(o)
        return up[id(o)]

    d['gin'] = {case: (g(a), g(b), g(l), [g(c) for c in cols]) for case, (_, _, (a, b, l, cols), _, _) in d['spec'].items()}
    d['gpu'] = gpu
    return d


@pytest.fixture(scope='module')
def n8():
    """one comparator batch"""
    d = _run_ctx(8, 818)
    assert M.rank_shape(8, d['orc'].n // 2)[2] == 1
    return d


@pytest.fixture(scope='module')
def n64():
    """N = 64 at ring 2^12: 2048 slots, two comparator batches (the stacked path)"""
    d = _run_ctx(64, 874)
    assert M.rank_shape(64, d['orc'].n // 2)[2] == 2
    return d


def _run(d, case, stack=32, lanes=2, cache=True, members=F.SORT_COLUMN_MEMBERS_DEFAULT, cols=None, count=True):
    gpu = d['gpu']
    mode, _, _, eps, cfg = d['spec'][case]
    kl, kr, lo, gcols = d['gin'][case]
    gpu.set_sort_stack(stack)
    gpu.set_sort_lanes(lanes)
    gpu.set_mask_cache(cache)
    gpu.set_sort_column_members(members)
    try:
        return gpu.running_sum(kl, kr, gcols if cols is None else cols, eps, d['N'], d['rots'], cfg, mode=mode, lo=lo,
                               count=count)
    finally:
        gpu.set_sort_column_members(F.SORT_COLUMN_MEMBERS_DEFAULT)
        gpu.set_mask_cache(True)
        gpu.set_sort_lanes(2)
        gpu.set_sort_stack(32)


def _check(d, case, outs, cnt):
    wouts, wcnt = d['want'][case]
    out_level = F.group_sum_levels(0, d['spec'][case][4])[1]  # the two tables come with their own sign configuration
    assert len(outs) == len(wouts)
    for g, o in zip(outs, wouts):
        same(g, o)
        assert g.level == out_level and g.slots == d['N']
    same(cnt, wcnt)
    assert cnt.level == out_level


@pytest.mark.parametrize('cache', [True, False], ids=['cached', 'uncached'])
@pytest.mark.parametrize('lanes', [1, 2])
@pytest.mark.parametrize('stack', [1, 32])
@pytest.mark.parametrize('case', CASES)
@pytest.mark.parametrize('which', ['n8', 'n64'])
def test_every_mode_matches_oracle_composition(request, which, case, stack, lanes, cache):
    d = request.getfixturevalue(which)
    with F.KernelClock(d['gpu']) as clk:
        outs, cnt = _run(d, case, stack, lanes, cache)
    assert has(clk, 'k_tensor_run'), sorted(clk.stats)
    # ROWS takes the rank's own tie-broken differences; the others the bounded ones
    assert has(clk, 'k_sub_add_plain_stacked' if case == 'rows' else 'k_sub_bounds_stacked'), sorted(clk.stats)
    assert not has(clk, 'k_tensor_pairs') and not has(clk, 'k_sub_pm_const_stacked'), sorted(clk.stats)
    _check(d, case, outs, cnt)


@pytest.mark.parametrize('members', [1, 2])
@pytest.mark.parametrize('case', ['rows', 'between'])
@pytest.mark.parametrize('which', ['n8', 'n64'])
def test_column_groups_give_the_same_words(request, which, case, members):
    """a member bound below P B splits the three columns over several products"""
    d = request.getfixturevalue(which)
    with F.KernelClock(d['gpu']) as clk:
        outs, cnt = _run(d, case, members=members)
    assert launches(clk, 'k_tensor_run') >= 2, sorted(clk.stats)
    _check(d, case, outs, cnt)


def test_rows_count_is_the_tiebroken_rank(n8, n64):
    """ROWS self join: count - 1 is direct_sort(mode=1) under set_sort_tiebreak(eps), word for word"""
    for d in (n8, n64):
        gpu = d['gpu']
        _, cnt = _run(d, 'rows', cols=[])
        gk = d['gin']['rows'][0]
        gpu.set_sort_tiebreak(d['eps'])
        try:
            rank = gpu.direct_sort(gk, d['N'], d['rots'], d['cfg'], mode=1)
        finally:
            gpu.set_sort_tiebreak(0.0)
        same(gpu.add_const(cnt, -1.0), rank)
    same(rank, M.oracle_rank(n64['orc'], n64['ok'], 64, n64['rots'], n64['cfg'], n64['eps']))  # ... the oracle's too


def test_decrypted_values_are_the_exact_sums(n8, n64):
    for d in (n8, n64):
        for case in CASES:
            mode, (kl, kr, lo, vals), _, eps, _ = d['spec'][case]
            outs, cnt = _run(d, case)
            wsums, wcnt = R.exact(kl, kr, vals, mode, eps, lo)
            err = max(max(np.max(np.abs(d['gpu'].decrypt(o) - w)) for o, w in zip(outs, wsums)),
                      np.max(np.abs(d['gpu'].decrypt(cnt) - wcnt)))
            print(f"N={d['N']} {case}: max error {err:.3e} (oracle composition {ORACLE_ERR[(d['N'], case)]:.3e})")
            assert wcnt.min() < d['N'] and wcnt.max() >= 3  # neither the plain sum nor a single row
            assert err <= 4 * ORACLE_ERR[(d['N'], case)]


def test_count_alone_and_columns_alone(n8):
    d = n8
    for case in ('rows', 'between'):
        outs, cnt = _run(d, case, cols=[], count=True)
        assert outs == []
        same(cnt, d['want'][case][1])
        outs = _run(d, case, cols=d['gin'][case][3][:1], count=False)
        assert len(outs) == 1
        same(outs[0], d['want'][case][0][0])


def test_tiebreak_setting_has_no_effect(n8):
    d = n8
    d['gpu'].set_sort_tiebreak(0.4 / d['N'])  # another eps than the call's own
    try:
        res = {case: _run(d, case) for case in ('rows', 'le')}
    finally:
        d['gpu'].set_sort_tiebreak(0.0)
    for case, (outs, cnt) in res.items():
        _check(d, case, outs, cnt)


CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import fhesort as F
import pyoracle as O
work, N, seed = sys.argv[3], int(sys.argv[4]), int(sys.argv[5])
cfg = (3, 2, 2) if N <= 16 else (3, 3, 2)
depth, rots = O.size_parameters(N)
orc = O.Context(12, depth, 40, 60, 3, seed=seed)
orc.gen_rotation_keys(rots)
gpu = F.Context(12, depth, 40, 60, 3, seed=seed, keygen=False)
gpu.load_keys_from(orc, rots)
meta = np.load(work + '/meta.npy')
cts = [gpu.upload(np.load(work + f'/in{i}.npy'), int(meta[i][0]), N, meta[i][1]) for i in range(len(meta))]
# inputs: the self join's key, the window's hi, lo and key, then the three columns
k, hi, lo, kw, cols = cts[0], cts[1], cts[2], cts[3], cts[4:]
with F.KernelClock(gpu) as clk:
    res = [gpu.running_sum(k, k, cols, 1.0 / N, N, rots, cfg, mode=m, count=True) for m in (F.RUN_ROWS, F.RUN_LE, F.RUN_LT)]
    res.append(gpu.running_sum(hi, kw, cols, 1.0 / N, N, rots, cfg, mode=F.RUN_BETWEEN, lo=lo, count=True))
assert not any(name.startswith(('k_sub_bounds_stacked', 'k_tensor_run')) for name in clk.stats), sorted(clk.stats)
for m, (outs, cnt) in enumerate(res):
    for i, o in enumerate(outs + [cnt]):
        np.save(work + f'/out{m}_{i}.npy', o.data())
        inf = o.info()
        np.save(work + f'/out{m}_{i}_meta.npy', np.array([inf['level'], inf['slots'], inf['scale']], dtype=np.float64))
print('ALLOK')
'''


def test_plain_form_gives_the_same_words(n64, tmp_path):
    """FHE_RUN_FUSED=0 (read once per process, so a fresh child): sub_stacked with the
    constant in place, the indicator written out, and one mul per column"""
    d = n64
    _, _, (ok, _, _, ocols), _, _ = d['spec']['rows']
    _, _, (ohi, okw, olo, _), _, _ = d['spec']['between']
    ins = [ok, ohi, olo, okw] + ocols
    np.save(tmp_path / 'meta.npy', np.array([[c.info()['level'], c.info()['scale']] for c in ins], dtype=np.float64))
    for i, c in enumerate(ins):
        np.save(tmp_path / f'in{i}.npy', c.data())
    env = dict(os.environ, FHE_RUN_FUSED='0')
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'),
                        os.path.join(REPO, 'oracle'), str(tmp_path), str(d['N']), str(d['seed'])], env=env,
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
    for m, case in enumerate(('rows', 'le', 'lt', 'between')):
        outs, cnt = d['want'][case]
        for i, o in enumerate(outs + [cnt]):
            oi = o.info()
            assert np.load(tmp_path / f'out{m}_{i}_meta.npy').tolist() == [oi['level'], oi['slots'], oi['scale']], (case, i)
            assert np.array_equal(np.load(tmp_path / f'out{m}_{i}.npy'), o.data()), (case, i)


# --------------------------------------------------------------- refusals --
def _raw_call(gpu, kl, lo, kr, cols, ncols, mode, eps, N, rots, cfg, want_count=True):
    """fhe_direct_running_sum itself: (status, the output handles it left, the message)"""
    r = np.asarray(rots, dtype=np.int32)
    arr = (C.c_void_p * max(1, len(cols)))(*[None if c is None else c.h for c in cols])
    outs = (C.c_void_p * max(1, len(cols)))(*([0xdead] * max(1, len(cols))))
    cnt = C.c_void_p(0xdead)
    h = lambda x: None if x is None else x.h
    rc = F.lib().fhe_direct_running_sum(gpu.h, h(kl), h(lo), h(kr), arr, ncols, mode, eps, N, F._int(r), len(r), cfg[0],
                                        cfg[1], cfg[2], outs, C.byref(cnt) if want_count else None)
    left = [outs[i] for i in range(max(ncols, 0))] + ([cnt.value] if want_count else [])
    return rc, left, F.lib().fhe_last_error().decode()


def test_refusals(n8):
    d = n8
    gpu, N, rots, cfg, eps = d['gpu'], d['N'], d['rots'], d['cfg'], d['eps']
    key, _, _, gcols = d['gin']['rows']
    hi, kw, lo, _ = d['gin']['between']
    col = gcols[0]
    wide = gpu.encrypt(np.zeros(2 * N), 2 * N)
    deeper_key = gpu.level_adjust(key, 1)
    too_deep = gpu.level_adjust(col, d['col_max'] + 1)
    stacked = gpu.stack([col, col])
    ROWS, BETWEEN = F.RUN_ROWS, F.RUN_BETWEEN
    cases = [
        # every case of test_gpu_group_sum.test_refusals
        ('null left key', None, None, key, [col], 1, ROWS, eps, True, F.FHE_EINVAL, 'left key'),
        ('null right key', key, None, None, [col], 1, ROWS, eps, True, F.FHE_EINVAL, 'right key'),
        ('key is a stack', key, None, gpu.stack([key, key]), [col], 1, ROWS, eps, True, F.FHE_EINVAL, 'right key'),
        ('key slots', key, None, wide, [col], 1, ROWS, eps, True, F.FHE_EINVAL, 'slots'),
        ('key levels', key, None, deeper_key, [col], 1, ROWS, eps, True, F.FHE_EINVAL, 'levels'),
        ('null column', key, None, key, [col, None], 2, ROWS, eps, True, F.FHE_EINVAL, 'column 1'),
        ('column is a stack', key, None, key, [col, col, stacked], 3, ROWS, eps, True, F.FHE_EINVAL, 'column 2'),
        ('column slots', key, None, key, [wide, col], 2, ROWS, eps, True, F.FHE_EINVAL, 'column 0'),
        ('eps = 0', key, None, key, [col], 1, ROWS, 0.0, True, F.FHE_EINVAL, 'eps'),
        ('eps = 0.5', key, None, key, [col], 1, ROWS, 0.5, True, F.FHE_EINVAL, 'eps'),
        ('eps nan', key, None, key, [col], 1, ROWS, float('nan'), True, F.FHE_EINVAL, 'eps'),
        ('negative ncols', key, None, key, [col], -1, ROWS, eps, True, F.FHE_EINVAL, 'ncols'),
        ('nothing asked for', key, None, key, [], 0, ROWS, eps, False, F.FHE_EINVAL, None),
        ('column one level too deep', key, None, key, [col, too_deep], 2, ROWS, eps, True, F.FHE_EDEPTH, 'column 1'),
        # the running sum's own
        ('mode 4', key, None, key, [col], 1, 4, eps, True, F.FHE_EINVAL, 'mode'),
        ('mode -1', key, None, key, [col], 1, -1, eps, True, F.FHE_EINVAL, 'mode'),
        ('left_lo outside BETWEEN', key, lo, key, [col], 1, F.RUN_LE, eps, True, F.FHE_EINVAL, 'left_lo'),
        ('left_lo in ROWS', key, lo, key, [col], 1, ROWS, eps, True, F.FHE_EINVAL, 'left_lo'),
        ('left_lo missing', hi, None, kw, [col], 1, BETWEEN, eps, True, F.FHE_EINVAL, 'left_lo'),
        ('left_lo level', hi, gpu.level_adjust(lo, 1), kw, [col], 1, BETWEEN, eps, True, F.FHE_EINVAL, 'left_lo'),
        ('left_lo slots', hi, wide, kw, [col], 1, BETWEEN, eps, True, F.FHE_EINVAL, 'left_lo'),
        ('left_lo is a stack', hi, gpu.stack([lo, lo]), kw, [col], 1, BETWEEN, eps, True, F.FHE_EINVAL, 'left_lo'),
        ('too deep in BETWEEN', hi, lo, kw, [too_deep], 1, BETWEEN, eps, True, F.FHE_EDEPTH, 'column 0'),
    ]
    for what, kl, l, kr, cols, ncols, mode, e, want_count, status, names in cases:
        rc, outs, msg = _raw_call(gpu, kl, l, kr, cols, ncols, mode, e, N, rots, cfg, want_count)
        assert rc == status, (what, rc, msg)
        assert all(o is None for o in outs), what  # every output handle still null
        if names:
            assert names in msg, (what, msg)
    # the deepest allowed column is served (it is column 2 of the fixture)
    assert d['spec']['rows'][2][3][2].level == d['col_max']


def test_shallow_context_is_refused(small):
    """a context without L_m + 1 levels: FHE_EDEPTH before any work"""
    _, gpu, vals = small
    _, rots = O.size_parameters(8)
    key = gpu.encrypt(np.arange(8) / 8.0, 8)
    for mode, lo in ((F.RUN_ROWS, None), (F.RUN_BETWEEN, key)):
        rc, outs, msg = _raw_call(gpu, key, lo, key, [key], 1, mode, 1.0 / 8, 8, rots, (3, 2, 2))
        assert rc == F.FHE_EDEPTH, (rc, msg)
        assert all(o is None for o in outs)


# ------------------------------------------- the sort and the group sums are untouched --
def test_sort_and_group_sum_after_running_sums_reproduce_the_oracle(n8):
    """the columns' masks are groupSums' second cached set, shared; the sort's own are undisturbed"""
    d = n8
    gpu, orc, N, rots, cfg, eps = d['gpu'], d['orc'], d['N'], d['rots'], d['cfg'], d['eps']
    gk, _, _, gcols = d['gin']['rows']
    _, _, (ok, _, _, ocols), _, _ = d['spec']['rows']
    _check(d, 'rows', *_run(d, 'rows'))
    same(gpu.direct_sort(gk, N, rots, cfg), orc.direct_sort(ok, N, rots, cfg))
    _check(d, 'between', *_run(d, 'between', cache=False))
    same(gpu.direct_sort(gk, N, rots, cfg, mode=1), orc.direct_sort(ok, N, rots, cfg, mode=1))
    wouts, wcnt = G.oracle_group_sums(orc, ok, ok, ocols[:1], N, rots, cfg, eps, True)
    outs, cnt = gpu.group_sum(gk, gk, gcols[:1], eps, N, rots, cfg, count=True)
    same(outs[0], wouts[0])
    same(cnt, wcnt)
    _check(d, 'le', *_run(d, 'le'))
