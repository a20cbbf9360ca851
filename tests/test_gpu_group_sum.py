"""Group sums and lookups on the GPU (fhe_direct_group_sum).

Kernel level: k_sub_pm_const_stacked and k_tensor_pairs against the oracle ops
they fuse, member by member and word for word.  Operator level: group_sum
against the CPU-oracle composition of tests/group_model.py, word for word, for
the self join (SUM / COUNT OVER (PARTITION BY key)) and for two tables (the LEFT
JOIN lookup), at N = 8 (one comparator batch) and N = 64 (two: the stacked
path), at every chunking, lane count, column grouping and mask-cache setting
and in the plain (unfused) form; decrypted values against the exact sums.
Oracle results are computed once per module and shared."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fhesort as F
import group_model as G
import pyoracle as O
import stable_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
KERNELS = ('k_sub_pm_const_stacked', 'k_tensor_pairs')

# Largest |decrypted - exact| of the CPU-oracle composition on these inputs and
# seeds (measured on the CPU).  The GPU words are the oracle's, so
# this is the GPU's error too; the tests assert 4x it, room for another seed's
# noise, not for a defect: a wrong word fails the word comparison first.
ORACLE_ERR = {
    (8, 'self'): 5.812e-08,
    (64, 'self'): 1.920e-07,
    (8, 'join'): 5.332e-09,
    (64, 'join'): 1.373e-07,
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


# ------------------------------------------------------------ kernel level --
@pytest.fixture(scope='module')
def small():
    """ring 2^12, L = 3, 40-bit scaling beside the 60-bit q0; 35 encrypted vectors"""
    orc = O.Context(12, 3, 40, 60, 3, seed=47)
    gpu = F.Context(12, 3, 40, 60, 3, seed=47, keygen=False)
    gpu.load_keys_from(orc, [])
    rng = np.random.default_rng(17)
    vals = [rng.uniform(-1, 1, 16) for _ in range(35)]
    return orc, gpu, vals


def _check_sub_pm_const(small, B, la, lb, launches):
    orc, gpu, vals = small
    c = 1.0 / 16
    oa = orc.encrypt(vals[0], 16, la)
    obs = [orc.encrypt(v, 16, lb) for v in vals[1:1 + B]]
    with F.KernelClock(gpu) as clk:
        R = gpu.sub_pm_const_stacked(gpu.from_oracle(oa), [gpu.from_oracle(b) for b in obs], c)
    assert clk.stats['k_sub_pm_const_stacked']['launches'] == launches, sorted(clk.stats)
    with pytest.raises(F.FheError):
        gpu.member(R, 2 * B)
    for i in range(B):
        d = orc.sub(oa, obs[i])
        same(gpu.member(R, i), orc.add_const(d, c))
        same(gpu.member(R, B + i), orc.add_const(orc.negate(d), c))


# five members cross the guarded tail of a thread's four
@pytest.mark.parametrize('B', [1, 4, 5])
@pytest.mark.parametrize('la,lb', [(1, 1), (0, 1)], ids=['same-level', 'a-one-level-below'])
def test_sub_pm_const_stacked_matches_oracle(small, B, la, lb):
    _check_sub_pm_const(small, B, la, lb, 1)


def test_sub_pm_const_stacked_second_launch(small):
    """33 members: a launch takes 32, and the second one's minus side still sits the whole 33 members on"""
    _check_sub_pm_const(small, 33, 1, 1, 2)


def test_sub_pm_const_stacked_with_a_above_the_operands(small):
    """a deeper than the bs: every b is adjusted instead, so per-member ops (sub_stacked's rule)"""
    orc, gpu, vals = small
    c = -0.25
    oa = orc.encrypt(vals[0], 16, 2)
    obs = [orc.encrypt(v, 16, 1) for v in vals[1:4]]
    with F.KernelClock(gpu) as clk:
        R = gpu.sub_pm_const_stacked(gpu.from_oracle(oa), [gpu.from_oracle(b) for b in obs], c)
    assert 'k_sub_pm_const_stacked' not in clk.stats
    for i in range(3):
        d = orc.sub(oa, obs[i])
        same(gpu.member(R, i), orc.add_const(d, c))
        same(gpu.member(R, 3 + i), orc.add_const(orc.negate(d), c))


def test_sub_pm_const_stacked_refusals(small):
    orc, gpu, vals = small
    a = gpu.encrypt(vals[0], 16, 1)
    b1, b2 = gpu.encrypt(vals[1], 16, 1), gpu.encrypt(vals[2], 16, 2)
    for aa, bs in ((a, [b1, b2]), (a, [gpu.stack([b1, b1])]), (gpu.stack([a, a]), [b1]), (a, [])):
        with pytest.raises(F.FheError) as e:
            gpu.sub_pm_const_stacked(aa, bs, 0.1)
        assert e.value.code == F.FHE_EINVAL


# five columns cross the guarded tail of a thread's four; five members leave the tile of the differences
@pytest.mark.parametrize('P', [1, 4, 5])
@pytest.mark.parametrize('B', [1, 4, 5])
def test_mul_pairs_matches_oracle(small, B, P):
    orc, gpu, vals = small
    oa = [orc.encrypt(v, 16, 1) for v in vals[0:B]]
    oadd = [orc.encrypt(v, 16, 1) for v in vals[5:5 + B]]
    ob = [orc.encrypt(v, 16, 1) for v in vals[10:10 + P * B]]
    st = lambda xs: gpu.stack([gpu.from_oracle(x) for x in xs])
    with F.KernelClock(gpu) as clk:
        R = gpu.mul_pairs(st(oa), st(oadd), st(ob), P)
    assert [k for k in clk.stats if k.startswith('k_tensor_pairs')] and not has(clk, 'k_tensor_cols'), sorted(clk.stats)
    assert sum(v['launches'] for k, v in clk.stats.items() if k.startswith('k_tensor_pairs')) == 1
    with pytest.raises(F.FheError):
        gpu.member(R, P * B)
    for p in range(P):
        for z in range(B):
            same(gpu.member(R, p * B + z), orc.mul(orc.add(oa[z], oadd[z]), ob[p * B + z]))


def test_mul_pairs_refusals(small):
    orc, gpu, vals = small
    x1 = [gpu.encrypt(v, 16, 1) for v in vals[:4]]
    x2 = [gpu.encrypt(v, 16, 2) for v in vals[:4]]
    a, add, b = gpu.stack(x1[:2]), gpu.stack(x1[2:]), gpu.stack(x1)
    cases = [(a, x1[0], b, 2),               # a_add holds fewer members
             (a, gpu.stack(x2[:2]), b, 2),   # a_add at another level
             (a, add, b, 3),                 # b is not ncols columns of B
             (a, add, gpu.stack(x2), 2),     # b at another level
             (a, add, b, 0)]
    for aa, ad, bb, ncols in cases:
        with pytest.raises(F.FheError) as e:
            gpu.mul_pairs(aa, ad, bb, ncols)
        assert e.value.code == F.FHE_EINVAL, ncols


# ---------------------------------------------------------- operator level --
def oracle_case(N, seed):
    """the oracle half of a fixture (no GPU): contexts, inputs and expected outputs"""
    depth, rots = O.size_parameters(N)
    orc = O.Context(12, depth, 40, 60, 3, seed=seed)
    orc.gen_rotation_keys(rots)
    cfg, eps = M.sign_cfg(N), 1.0 / N
    rng = np.random.default_rng(seed)
    # self join: tied keys, three columns entering at levels 0, 1 and the deepest allowed, and the count
    k = M.tied_input(N, M.SEEDS[N])
    vals = [rng.uniform(-1, 1, N), np.arange(N) / N, rng.uniform(-1, 1, N)]
    col_max, out_level = F.group_sum_levels(0, cfg)
    ok = orc.encrypt(k, N)
    ocols = [orc.encrypt(v, N, lv) for v, lv in zip(vals, (0, 1, col_max))]
    oouts, ocnt = G.oracle_group_sums(orc, ok, ok, ocols, N, rots, cfg, eps, True)
    # two tables: unique right keys, about half of the left keys absent; one column and the count
    kl, kr, jeps, jcfg = G.lookup_tables(N, seed + 1)
    jv = rng.uniform(-1, 1, N)
    okl, okr, ojv = orc.encrypt(kl, N), orc.encrypt(kr, N), orc.encrypt(jv, N)
    ojouts, ojcnt = G.oracle_group_sums(orc, okl, okr, [ojv], N, rots, jcfg, jeps, True)
    return dict(N=N, seed=seed, orc=orc, depth=depth, rots=rots, cfg=cfg, eps=eps, k=k, vals=vals, ok=ok, ocols=ocols,
                oouts=oouts, ocnt=ocnt, col_max=col_max, out_level=out_level, kl=kl, kr=kr, jeps=jeps, jcfg=jcfg,
                jv=jv, okl=okl, okr=okr, ojv=ojv, ojouts=ojouts, ojcnt=ojcnt)


def oracle_errors(d):
    """largest |decrypted - exact| of the oracle composition: (self join, two tables)"""
    wsums, wcnt = G.exact(d['k'], d['k'], d['vals'], d['eps'])
    e_self = max(max(np.max(np.abs(o.decrypt() - w)) for o, w in zip(d['oouts'], wsums)),
                 np.max(np.abs(d['ocnt'].decrypt() - wcnt)))
    jsums, jcnt = G.exact(d['kl'], d['kr'], [d['jv']], d['jeps'])
    e_join = max(np.max(np.abs(d['ojouts'][0].decrypt() - jsums[0])), np.max(np.abs(d['ojcnt'].decrypt() - jcnt)))
    return e_self, e_join


def _group_ctx(N, seed):
    d = oracle_case(N, seed)
    gpu = F.Context(12, d['depth'], 40, 60, 3, seed=seed, keygen=False)
    gpu.load_keys_from(d['orc'], d['rots'])
    d.update(gpu=gpu, gk=gpu.from_oracle(d['ok']), gcols=[gpu.from_oracle(c) for c in d['ocols']],
             gkl=gpu.from_oracle(d['okl']), gkr=gpu.from_oracle(d['okr']), gjv=gpu.from_oracle(d['ojv']))
    return d


@pytest.fixture(scope='module')
def n8():
    """one comparator batch"""
    d = _group_ctx(8, 818)
    assert M.rank_shape(8, d['orc'].n // 2)[2] == 1
    return d


@pytest.fixture(scope='module')
def n64():
    """N = 64 at ring 2^12: 2048 slots, two comparator batches (the stacked path)"""
    d = _group_ctx(64, 874)
    assert M.rank_shape(64, d['orc'].n // 2)[2] == 2
    return d


def _self_join(d, stack=32, lanes=2, cache=True, members=F.SORT_COLUMN_MEMBERS_DEFAULT, cols=None, count=True):
    gpu = d['gpu']
    gpu.set_sort_stack(stack)
    gpu.set_sort_lanes(lanes)
    gpu.set_mask_cache(cache)
    gpu.set_sort_column_members(members)
    try:
        return gpu.group_sum(d['gk'], d['gk'], d['gcols'] if cols is None else cols, d['eps'], d['N'], d['rots'],
                             d['cfg'], count=count)
    finally:
        gpu.set_sort_column_members(F.SORT_COLUMN_MEMBERS_DEFAULT)
        gpu.set_mask_cache(True)
        gpu.set_sort_lanes(2)
        gpu.set_sort_stack(32)


def _check_self(d, outs, cnt):
    for g, o in zip(outs, d['oouts']):
        same(g, o)
        assert g.level == d['out_level']
    same(cnt, d['ocnt'])


@pytest.mark.parametrize('cache', [True, False], ids=['cached', 'uncached'])
@pytest.mark.parametrize('lanes', [1, 2])
@pytest.mark.parametrize('stack', [1, 32])
@pytest.mark.parametrize('which', ['n8', 'n64'])
def test_self_join_matches_oracle_composition(request, which, stack, lanes, cache):
    d = request.getfixturevalue(which)
    with F.KernelClock(d['gpu']) as clk:
        outs, cnt = _self_join(d, stack, lanes, cache)
    for name in KERNELS:
        assert has(clk, name), (name, sorted(clk.stats))
    _check_self(d, outs, cnt)


@pytest.mark.parametrize('members', [1, 2])
@pytest.mark.parametrize('which', ['n8', 'n64'])
def test_column_groups_give_the_same_words(request, which, members):
    """a member bound below P B splits the three columns over several products"""
    d = request.getfixturevalue(which)
    with F.KernelClock(d['gpu']) as clk:
        outs, cnt = _self_join(d, members=members)
    launches = sum(v['launches'] for k, v in clk.stats.items() if k.startswith('k_tensor_pairs'))
    assert launches >= 2, sorted(clk.stats)
    _check_self(d, outs, cnt)


def test_decrypted_self_join_is_the_window_aggregate(n8, n64):
    for d in (n8, n64):
        outs, cnt = _self_join(d)
        wsums, wcnt = G.exact(d['k'], d['k'], d['vals'], d['eps'])
        err = max(max(np.max(np.abs(d['gpu'].decrypt(o) - w)) for o, w in zip(outs, wsums)),
                  np.max(np.abs(d['gpu'].decrypt(cnt) - wcnt)))
        print(f"N={d['N']} self join: max error {err:.3e} (oracle composition {ORACLE_ERR[(d['N'], 'self')]:.3e})")
        assert wcnt.max() >= 3  # real groups
        assert err <= 4 * ORACLE_ERR[(d['N'], 'self')]


@pytest.mark.parametrize('which', ['n8', 'n64'])
def test_lookup_into_a_second_table(request, which):
    """unique right keys: the matching row's value, zero where the left key is absent"""
    d = request.getfixturevalue(which)
    gpu = d['gpu']
    outs, cnt = gpu.group_sum(d['gkl'], d['gkr'], [d['gjv']], d['jeps'], d['N'], d['rots'], d['jcfg'], count=True)
    same(outs[0], d['ojouts'][0])
    same(cnt, d['ojcnt'])
    jsums, jcnt = G.exact(d['kl'], d['kr'], [d['jv']], d['jeps'])
    absent = jcnt == 0
    assert absent.any() and (~absent).any() and jcnt.max() == 1
    got, gcnt = gpu.decrypt(outs[0]), gpu.decrypt(cnt)
    err = max(np.max(np.abs(got - jsums[0])), np.max(np.abs(gcnt - jcnt)))
    print(f"N={d['N']} lookup: max error {err:.3e}, absent slots {np.max(np.abs(got[absent])):.3e} "
          f"(oracle composition {ORACLE_ERR[(d['N'], 'join')]:.3e})")
    assert err <= 4 * ORACLE_ERR[(d['N'], 'join')]
    assert np.max(np.abs(got[absent])) <= 4 * ORACLE_ERR[(d['N'], 'join')]


def test_count_alone_and_columns_alone(n8):
    d = n8
    outs, cnt = _self_join(d, cols=[], count=True)
    assert outs == []
    same(cnt, d['ocnt'])
    outs = _self_join(d, cols=d['gcols'][:1], count=False)
    assert len(outs) == 1
    same(outs[0], d['oouts'][0])


def test_tiebreak_setting_has_no_effect(n8):
    d = n8
    d['gpu'].set_sort_tiebreak(1.0 / d['N'])
    try:
        outs, cnt = _self_join(d)
    finally:
        d['gpu'].set_sort_tiebreak(0.0)
    _check_self(d, outs, cnt)


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
with F.KernelClock(gpu) as clk:
    outs, cnt = gpu.group_sum(cts[0], cts[0], cts[1:], 1.0 / N, N, rots, cfg, count=True)
assert not any(k.startswith(('k_sub_pm_const_stacked', 'k_tensor_pairs')) for k in clk.stats), sorted(clk.stats)
for i, o in enumerate(outs + [cnt]):
    np.save(work + f'/out{i}.npy', o.data())
    inf = o.info()
    np.save(work + f'/out{i}_meta.npy', np.array([inf['level'], inf['slots'], inf['scale']], dtype=np.float64))
print('ALLOK')
'''


def test_plain_form_gives_the_same_words(n64, tmp_path):
    """FHE_GROUP_FUSED=0 (read once per process, so a fresh child): sub_stacked with
    negate / add_const on the stack, and one mul_add per column"""
    d = n64
    ins = [d['ok']] + d['ocols']
    np.save(tmp_path / 'meta.npy', np.array([[c.info()['level'], c.info()['scale']] for c in ins], dtype=np.float64))
    for i, c in enumerate(ins):
        np.save(tmp_path / f'in{i}.npy', c.data())
    env = dict(os.environ, FHE_GROUP_FUSED='0')
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'),
                        os.path.join(REPO, 'oracle'), str(tmp_path), str(d['N']), str(d['seed'])], env=env,
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
    for i, o in enumerate(d['oouts'] + [d['ocnt']]):
        oi = o.info()
        assert np.load(tmp_path / f'out{i}_meta.npy').tolist() == [oi['level'], oi['slots'], oi['scale']], i
        assert np.array_equal(np.load(tmp_path / f'out{i}.npy'), o.data()), i


# --------------------------------------------------------------- refusals --
def _raw_call(gpu, kl, kr, cols, ncols, eps, N, rots, cfg, want_count=True):
    """fhe_direct_group_sum itself: (status, the output handles it left, the message)"""
    r = np.asarray(rots, dtype=np.int32)
    arr = (C.c_void_p * max(1, len(cols)))(*[None if c is None else c.h for c in cols])
    outs = (C.c_void_p * max(1, len(cols)))(*([0xdead] * max(1, len(cols))))
    cnt = C.c_void_p(0xdead)
    rc = F.lib().fhe_direct_group_sum(gpu.h, None if kl is None else kl.h, None if kr is None else kr.h, arr, ncols,
                                      eps, N, F._int(r), len(r), cfg[0], cfg[1], cfg[2], outs,
                                      C.byref(cnt) if want_count else None)
    left = [outs[i] for i in range(max(ncols, 0))] + ([cnt.value] if want_count else [])
    return rc, left, F.lib().fhe_last_error().decode()


def test_refusals(n8):
    d = n8
    gpu, N, rots, cfg, eps = d['gpu'], d['N'], d['rots'], d['cfg'], d['eps']
    key, col = d['gk'], d['gcols'][0]
    wide = gpu.encrypt(np.zeros(2 * N), 2 * N)
    deeper_key = gpu.level_adjust(key, 1)
    too_deep = gpu.level_adjust(col, d['col_max'] + 1)
    stacked = gpu.stack([col, col])
    cases = [
        ('null left key', None, key, [col], 1, eps, True, F.FHE_EINVAL, 'left key'),
        ('null right key', key, None, [col], 1, eps, True, F.FHE_EINVAL, 'right key'),
        ('key is a stack', key, gpu.stack([key, key]), [col], 1, eps, True, F.FHE_EINVAL, 'right key'),
        ('key slots', key, wide, [col], 1, eps, True, F.FHE_EINVAL, 'slots'),
        ('key levels', key, deeper_key, [col], 1, eps, True, F.FHE_EINVAL, 'levels'),
        ('null column', key, key, [col, None], 2, eps, True, F.FHE_EINVAL, 'column 1'),
        ('column is a stack', key, key, [col, col, stacked], 3, eps, True, F.FHE_EINVAL, 'column 2'),
        ('column slots', key, key, [wide, col], 2, eps, True, F.FHE_EINVAL, 'column 0'),
        ('eps = 0', key, key, [col], 1, 0.0, True, F.FHE_EINVAL, 'eps'),
        ('eps = 0.5', key, key, [col], 1, 0.5, True, F.FHE_EINVAL, 'eps'),
        ('eps nan', key, key, [col], 1, float('nan'), True, F.FHE_EINVAL, 'eps'),
        ('negative ncols', key, key, [col], -1, eps, True, F.FHE_EINVAL, 'ncols'),
        ('nothing asked for', key, key, [], 0, eps, False, F.FHE_EINVAL, None),
        ('column one level too deep', key, key, [col, too_deep], 2, eps, True, F.FHE_EDEPTH, 'column 1'),
    ]
    for what, kl, kr, cols, ncols, e, want_count, status, names in cases:
        rc, outs, msg = _raw_call(gpu, kl, kr, cols, ncols, e, N, rots, cfg, want_count)
        assert rc == status, (what, rc, msg)
        assert all(o is None for o in outs), what  # every output handle still null
        if names:
            assert names in msg, (what, msg)
    # the deepest allowed column is served (it is column 2 of the fixture)
    assert d['ocols'][2].level == d['col_max']


def test_shallow_context_is_refused(small):
    """a context without L_m + 1 levels: FHE_EDEPTH before any work"""
    _, gpu, vals = small
    _, rots = O.size_parameters(8)
    key = gpu.encrypt(np.arange(8) / 8.0, 8)
    rc, outs, msg = _raw_call(gpu, key, key, [key], 1, 1.0 / 8, 8, rots, (3, 2, 2))
    assert rc == F.FHE_EDEPTH, (rc, msg)
    assert all(o is None for o in outs)


# ---------------------------------------------------- the sort is untouched --
def test_sort_after_group_sums_reproduces_the_oracle(n8):
    """the columns' masks are further entries of the sorter's cache; the sort's own are undisturbed"""
    d = n8
    gpu, orc, N = d['gpu'], d['orc'], d['N']
    _check_self(d, *_self_join(d))
    same(gpu.direct_sort(d['gk'], N, d['rots'], d['cfg']), orc.direct_sort(d['ok'], N, d['rots'], d['cfg']))
    _check_self(d, *_self_join(d, cache=False))
    same(gpu.direct_sort(d['gk'], N, d['rots'], d['cfg'], mode=1),
         orc.direct_sort(d['ok'], N, d['rots'], d['cfg'], mode=1))
