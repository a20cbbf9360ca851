"""Tables of different sizes in the all-pairs operators on the GPU
(fhe_set_pair_tables).

group_sum, running_sum, window_sum and gather between a left table of Nl rows
and a right table of Nr rows, word for word against the CPU-oracle compositions
of tests/rect_model.py, at the smallest shapes that reach each branch of the
layout:

    (8, 2)    ring 2^12   P' < P_: sparse num_slots, np = 2, one batch, right tiled
    (2, 8)    ring 2^12   the same with the left tiled and a two-round residue fold
    (64, 32)  ring 2^12   n = P_: the square's num_slots and masks, one batch of its two
    (32, 64)  ring 2^12   the same with a one-round residue fold
    (64, 32)  ring 2^11   P_ = 16: two batches, the stacked chunk path
    (32, 64)  ring 2^11   the same, left tiled, one-round fold

The existing kernels run here at shapes the square call never gave them: fewer
partitions than the square's, one-member chunks, sparse num_slots with tiled
operands.  Decrypted values against the exact sums and against today's square
call on the sentinel-padded tables; the setting with equal sizes against the
setting off; the refusals.  Oracle results are computed once per module."""
import ctypes as C

import numpy as np
import pytest

import fhesort as F
import rect_model as RM
import stable_model as M

pytestmark = pytest.mark.gpu

# Largest |decrypted - exact| of the CPU-oracle compositions on rect_model.oracle_case's inputs and seeds
# (measured on the CPU).  The GPU words are the oracle's, so this is the GPU's error too; the
# tests assert 4x it, room for another seed's noise, not for a defect: a wrong word fails the word comparison
# first.
ORACLE_ERR = {
    (8, 2, 12, 'group'): 9.002e-09,
    (8, 2, 12, 'run_le'): 8.983e-09,
    (8, 2, 12, 'run_between'): 2.107e-08,
    (8, 2, 12, 'win_le'): 8.890e-09,
    (8, 2, 12, 'win_group'): 9.033e-09,
    (8, 2, 12, 'gather'): 2.034e-08,
    (8, 2, 12, 'gather_sum'): 8.866e-09,
    (2, 8, 12, 'group'): 2.641e-08,
    (2, 8, 12, 'run_le'): 2.653e-08,
    (2, 8, 12, 'run_between'): 4.482e-08,
    (2, 8, 12, 'win_le'): 1.770e-08,
    (2, 8, 12, 'win_group'): 1.740e-08,
    (2, 8, 12, 'gather'): 1.255e-08,
    (2, 8, 12, 'gather_sum'): 6.073e-09,
    (64, 32, 12, 'group'): 1.997e-06,
    (32, 64, 12, 'group'): 5.605e-06,
    (64, 32, 11, 'group'): 2.019e-06,
    (64, 32, 11, 'run_le'): 1.312e-06,
    (64, 32, 11, 'run_between'): 1.475e-06,
    (64, 32, 11, 'win_le'): 1.201e-05,
    (64, 32, 11, 'win_group'): 2.863e-06,
    (64, 32, 11, 'gather'): 5.213e-07,
    (64, 32, 11, 'gather_sum'): 7.930e-07,
    (32, 64, 11, 'group'): 5.606e-06,
    (32, 64, 11, 'run_le'): 2.878e-06,
    (32, 64, 11, 'run_between'): 2.231e-06,
    (32, 64, 11, 'win_le'): 3.160e-05,
    (32, 64, 11, 'win_group'): 7.703e-06,
    (32, 64, 11, 'gather'): 5.901e-07,
    (32, 64, 11, 'gather_sum'): 5.812e-07,
}
# ... and of group_model.oracle_group_sums, the square call's definition, on the same tables padded to N rows
# by sentinels (rect_model.oracle_padded_group_sums), over the Nl real left rows
PADDED_ERR = {
    (8, 2, 12): 3.392e-08,
    (2, 8, 12): 2.695e-08,
    (64, 32, 12): 2.035e-06,
    (32, 64, 12): 5.610e-06,
    (64, 32, 11): 2.014e-06,
    (32, 64, 11): 5.605e-06,
}
# (num_slots, num_partition, num_batch, np, fold_steps) each case must have, or it tests another branch
SHAPE_OF = {
    (8, 2, 12): (16, 2, 1, 2, 0),
    (2, 8, 12): (16, 2, 1, 2, 2),
    (64, 32, 12): (2048, 32, 1, 8, 0),
    (32, 64, 12): (2048, 32, 1, 8, 1),
    (64, 32, 11): (1024, 16, 2, 8, 0),
    (32, 64, 11): (1024, 16, 2, 8, 1),
}
ALL = list(RM.SHAPES)
FULL = [k for k, every in RM.SHAPES.items() if every]
TWO_BATCH = [(64, 32, 11), (32, 64, 11)]
ids = lambda keys: [f'{a}x{b}-ring{r}' for a, b, r in keys]


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


_CASES = {}


def case(key):
    """the oracle half and the GPU context of a shape, made once per module"""
    if key in _CASES:
        return _CASES[key]
    Nl, Nr, logn = key
    assert F.pair_shape(Nl, Nr, 1 << (logn - 1)) == SHAPE_OF[key]
    if Nl >= Nr and (Nl, logn) == (64, 12):  # one batch of the square's two, on the square's own slot count
        assert M.rank_shape(64, 2048) == (2048, 32, 2, 8)
    c = RM.oracle_case(Nl, Nr, logn)
    gpu = F.Context(logn, c['depth'], 40, 60, 3, seed=RM.context_seed(Nl, Nr, logn), keygen=False)
    gpu.load_keys_from(c['orc'], c['rots'])
    e = c['enc']
    g = {k: gpu.from_oracle(v) for k, v in e.items() if k != 'cols'}
    g['cols'] = [gpu.from_oracle(v) for v in e['cols']]
    c.update(gpu=gpu, g=g, key=key, tables=(Nl, Nr))
    _CASES[key] = c
    return c


@pytest.fixture(scope='module', autouse=True)
def _release_cases():
    yield
    _CASES.clear()


def check(c, op, outs, cnt):
    """word for word against the composition, and the outputs' slot count"""
    oouts, ocnt = c['res'][op]
    assert len(outs) == len(oouts)
    for g, o in zip(outs, oouts):
        same(g, o)
        assert g.slots == c['d']['Nl']
    for g, o in zip(cnt if isinstance(cnt, list) else [cnt], ocnt if isinstance(ocnt, list) else [ocnt]):
        same(g, o)


def decrypted_error(c, outs, cnt, op):
    gpu = c['gpu']
    wsum, wcnt = c['want'][op]
    cnts = cnt if isinstance(cnt, list) else [cnt]
    err = max(np.max(np.abs(gpu.decrypt(o) - w)) for o, w in zip(outs, np.reshape(wsum, (len(outs), -1))))
    return max(err, max(np.max(np.abs(gpu.decrypt(x) - w)) for x, w in zip(cnts, np.reshape(wcnt, (len(cnts), -1)))))


def run(c, op, tables='case'):
    """one operator of rect_model.oracle_results on the GPU: (outs, count or flags)"""
    gpu, g, d = c['gpu'], c['g'], c['d']
    N, rots, cfg, eps = d['N'], c['rots'], d['cfg'], d['eps']
    t = c['tables'] if tables == 'case' else tables
    c1 = g['cols'][:1]
    if op == 'group':
        return gpu.group_sum(g['kl'], g['kr'], g['cols'], eps, N, rots, cfg, count=True, tables=t)
    if op == 'run_le':
        return gpu.running_sum(g['kl'], g['kr'], c1, eps, N, rots, cfg, mode=F.RUN_LE, count=True, tables=t)
    if op == 'run_between':
        return gpu.running_sum(g['hi'], g['kr'], c1, eps, N, rots, cfg, mode=F.RUN_BETWEEN, lo=g['lo'], count=True,
                               tables=t)
    if op == 'win_le':
        return gpu.window_sum([g['k2l']], [g['k2r']], c1, eps, N, rots, cfg, order_left=g['kl'], order_right=g['kr'],
                              mode=F.WIN_LE, count=True, tables=t)
    if op == 'win_group':
        return gpu.window_sum([g['kl'], g['k2l']], [g['kr'], g['k2r']], c1, eps, N, rots, cfg, mode=F.WIN_GROUP,
                              count=True, tables=t)
    assert op in ('gather', 'gather_sum')
    return gpu.gather(g['pl'], g['pr'], c1, RM.OFFSETS, N, rots, present=True, sum_offsets=op == 'gather_sum', tables=t)


KERNELS = {
    'group': ('k_sub_pm_const_stacked', 'k_tensor_pairs'),
    'run_le': ('k_sub_bounds_stacked', 'k_tensor_run'),
    'run_between': ('k_sub_bounds_stacked', 'k_tensor_run'),
    'win_le': ('k_sub_window_stacked', 'k_tensor_run'),
    'win_group': ('k_sub_window_stacked', 'k_tensor_win', 'k_tensor_run'),
    'gather': ('k_sub_offsets_stacked', 'k_tensor_gather'),
    'gather_sum': ('k_sub_offsets_stacked', 'k_tensor_gather'),
}


# -------------------------------------------------------------- group sums --
@pytest.mark.parametrize('key', ALL, ids=ids(ALL))
def test_group_sum_matches_oracle_composition(key):
    c = case(key)
    with F.KernelClock(c['gpu']) as clk:
        outs, cnt = run(c, 'group')
    for name in KERNELS['group']:
        assert has(clk, name), (name, sorted(clk.stats))
    check(c, 'group', outs, cnt)
    col_max, out_level = F.group_sum_levels(0, c['d']['cfg'])
    assert all(o.level == out_level for o in outs + [cnt])  # no level beyond the square call's
    assert c['gpu']._pair_tables == (0, 0)  # the keyword restored the setting


@pytest.mark.parametrize('stack,lanes,members,cache', [(1, 1, F.SORT_COLUMN_MEMBERS_DEFAULT, True),
                                                      (32, 2, F.SORT_COLUMN_MEMBERS_DEFAULT, True),
                                                      (32, 2, 1, True), (32, 2, F.SORT_COLUMN_MEMBERS_DEFAULT, False)],
                         ids=['stack1-lane1', 'stack32-lanes2', 'members1', 'uncached'])
@pytest.mark.parametrize('key', TWO_BATCH, ids=ids(TWO_BATCH))
def test_group_sum_words_do_not_depend_on_the_chunking(key, stack, lanes, members, cache):
    c = case(key)
    gpu = c['gpu']
    gpu.set_sort_stack(stack)
    gpu.set_sort_lanes(lanes)
    gpu.set_sort_column_members(members)
    gpu.set_mask_cache(cache)
    try:
        outs, cnt = run(c, 'group')
    finally:
        gpu.set_mask_cache(True)
        gpu.set_sort_column_members(F.SORT_COLUMN_MEMBERS_DEFAULT)
        gpu.set_sort_lanes(2)
        gpu.set_sort_stack(32)
    check(c, 'group', outs, cnt)


@pytest.mark.parametrize('key', ALL, ids=ids(ALL))
def test_decrypted_group_sums(key):
    """against the exact sums, and against today's square call on the sentinel-padded tables"""
    c = case(key)
    gpu, d = c['gpu'], c['d']
    Nl = d['Nl']
    outs, cnt = run(c, 'group')
    err = decrypted_error(c, outs, cnt, 'group')
    wcnt = c['want']['group'][1]
    assert (wcnt == 0).any() and (wcnt > 0).any()  # rows with and without a partner
    okl, okr, ocols = RM.encrypt_padded(c)
    pouts, pcnt = gpu.group_sum(gpu.from_oracle(okl), gpu.from_oracle(okr), [gpu.from_oracle(x) for x in ocols],
                                d['eps'], d['N'], c['rots'], d['cfg'], count=True)
    assert pcnt.slots == d['N']
    diff = max(max(np.max(np.abs(gpu.decrypt(o) - gpu.decrypt(p)[:Nl])) for o, p in zip(outs, pouts)),
               np.max(np.abs(gpu.decrypt(cnt) - gpu.decrypt(pcnt)[:Nl])))
    print(f'{key}: max error {err:.3e} (oracle composition {ORACLE_ERR[key + ("group",)]:.3e}), '
          f'against the padded square call {diff:.3e} (its own error {PADDED_ERR[key]:.3e})')
    assert err <= 4 * ORACLE_ERR[key + ('group',)]
    assert diff <= ORACLE_ERR[key + ('group',)] + PADDED_ERR[key]


# ------------------------------------------- running and window sums, gather --
@pytest.mark.parametrize('op', ['run_le', 'run_between', 'win_le', 'win_group', 'gather', 'gather_sum'])
@pytest.mark.parametrize('key', FULL, ids=ids(FULL))
def test_operator_matches_oracle_composition(key, op):
    c = case(key)
    with F.KernelClock(c['gpu']) as clk:
        outs, cnt = run(c, op)
    for name in KERNELS[op]:
        assert has(clk, name), (name, sorted(clk.stats))
    check(c, op, outs, cnt)
    err = decrypted_error(c, outs, cnt, op)
    print(f'{key} {op}: max error {err:.3e} (oracle composition {ORACLE_ERR[key + (op,)]:.3e})')
    assert err <= 4 * ORACLE_ERR[key + (op,)]


# ------------------------------------------------------------ the setting --
@pytest.fixture(scope='module')
def square():
    """self joins of the left table of (8, 2) with its own columns: both tables hold N = 8 rows"""
    c = case((8, 2, 12))
    gpu, g, d = c['gpu'], c['g'], c['d']
    rng = np.random.default_rng(8)
    cols = [gpu.encrypt(rng.uniform(-1, 1, 8), 8), gpu.encrypt(np.arange(8) / 8.0, 8, 1)]
    sq = dict(c, g=dict(g, kr=g['kl'], k2r=g['k2l'], pr=g['pl'], cols=cols))
    return sq


@pytest.mark.parametrize('op', ['group', 'run_le', 'run_between', 'win_le', 'win_group', 'gather', 'gather_sum'])
def test_equal_sizes_give_the_square_calls_words(square, op):
    off_outs, off_cnt = run(square, op, tables=None)
    on_outs, on_cnt = run(square, op, tables=(8, 8))
    as_list = lambda x: x if isinstance(x, list) else [x]
    for a, b in zip(off_outs + as_list(off_cnt), on_outs + as_list(on_cnt)):
        same(a, b)
        assert a.slots == 8


def test_rows_modes_run_under_equal_sizes(square):
    gpu, g, d = square['gpu'], square['g'], square['d']
    args = (g['kl'], g['kl'], g['cols'][:1], d['eps'], d['N'], square['rots'], d['cfg'])
    off = gpu.running_sum(*args, mode=F.RUN_ROWS, count=True)
    on = gpu.running_sum(*args, mode=F.RUN_ROWS, count=True, tables=(8, 8))
    same(off[0][0], on[0][0])
    same(off[1], on[1])


def test_setting_off_still_refuses_mismatched_slots():
    c = case((8, 2, 12))
    for op in ('group', 'run_le', 'win_le', 'gather'):
        with pytest.raises(F.FheError) as e:
            run(c, op, tables=None)
        assert e.value.code == F.FHE_EINVAL and 'slots' in str(e.value), op


def test_setting_persists_until_cleared_and_leaves_the_sort_alone():
    c = case((8, 2, 12))
    gpu, g, d = c['gpu'], c['g'], c['d']
    gpu.set_pair_tables(8, 2)
    try:
        outs, cnt = run(c, 'group', tables=None)  # the context's setting, not the keyword
        check(c, 'group', outs, cnt)
        cfg = M.sign_cfg(8)
        same(gpu.direct_sort(g['kl'], 8, c['rots'], cfg, mode=1),
             c['orc'].direct_sort(c['enc']['kl'], 8, c['rots'], cfg, mode=1))
    finally:
        gpu.set_pair_tables(0, 0)
    with pytest.raises(F.FheError):
        run(c, 'group', tables=None)


def test_set_pair_tables_refusals():
    gpu = case((8, 2, 12))['gpu']
    for nl, nr in ((3, 8), (8, 1), (2, 2), (4096, 8), (0, 8)):
        with pytest.raises(F.FheError) as e:
            gpu.set_pair_tables(nl, nr)
        assert e.value.code == F.FHE_EINVAL, (nl, nr)
    small = case((64, 32, 11))['gpu']  # 1024 slots
    with pytest.raises(F.FheError) as e:
        small.set_pair_tables(2048, 8)
    assert e.value.code == F.FHE_EINVAL and 'exceed' in str(e.value)
    assert gpu._pair_tables == (0, 0) and small._pair_tables == (0, 0)


def _outputs(n):
    return (C.c_void_p * n)(*([0xdead] * n)), C.c_void_p(0xdead)


def _handles(cts):
    return (C.c_void_p * max(1, len(cts)))(*[x.h for x in cts])


def test_refusals_between_unequal_sizes():
    """FHE_EINVAL with every output handle NULL; the message names the argument and both counts"""
    c = case((8, 2, 12))
    gpu, g, d = c['gpu'], c['g'], c['d']
    lib, eps, cfg = F.lib(), d['eps'], d['cfg']
    r = np.asarray(c['rots'], dtype=np.int32)
    r4 = np.asarray(F.size_parameters(4)[1], dtype=np.int32)
    left_col = gpu.encrypt(np.zeros(8), 8)  # a column with Nl slots
    gpu.set_pair_tables(8, 2)
    try:
        def group(kl, kr, cols, N, rots):
            outs, cnt = _outputs(len(cols))
            rc = lib.fhe_direct_group_sum(gpu.h, kl.h, kr.h, _handles(cols), len(cols), eps, N, F._int(rots), len(rots),
                                          *cfg, outs, C.byref(cnt))
            return rc, [outs[i] for i in range(len(cols))] + [cnt.value], lib.fhe_last_error().decode()

        def running(mode):
            outs, cnt = _outputs(1)
            rc = lib.fhe_direct_running_sum(gpu.h, g['kl'].h, None, g['kr'].h, _handles(g['cols'][:1]), 1, mode, eps, 8,
                                            F._int(r), len(r), *cfg, outs, C.byref(cnt))
            return rc, [outs[0], cnt.value], lib.fhe_last_error().decode()

        def window(mode):
            outs, cnt = _outputs(1)
            rc = lib.fhe_direct_window_sum(gpu.h, _handles([g['k2l']]), _handles([g['k2r']]), 1, g['kl'].h, None,
                                           g['kr'].h, _handles(g['cols'][:1]), 1, mode, eps, 8, F._int(r), len(r), *cfg,
                                           outs, C.byref(cnt))
            return rc, [outs[0], cnt.value], lib.fhe_last_error().decode()

        def gather(pl, pr):
            outs = (C.c_void_p * 2)(0xdead, 0xdead)
            off = np.asarray([0], dtype=np.int32)
            rc = lib.fhe_direct_gather(gpu.h, pl.h, pr.h, _handles(g['cols'][:1]), 1, F._int(off), 1, 1, 0, 8, F._int(r),
                                       len(r), outs)
            return rc, [outs[0], outs[1]], lib.fhe_last_error().decode()

        cases = [
            ('rows running sum', running(F.RUN_ROWS), 'rows mode'),
            ('rows window sum', window(F.WIN_ROWS), 'rows mode'),
            ('right column with Nl slots', group(g['kl'], g['kr'], [g['cols'][0], left_col], 8, r), 'column 1'),
            ('right key with Nl slots', group(g['kl'], g['kl'], g['cols'][:1], 8, r), 'right_key'),
            ('left key with Nr slots', group(g['kr'], g['kr'], g['cols'][:1], 8, r), 'left_key'),
            ('N is not the larger table', group(g['kl'], g['kr'], g['cols'][:1], 4, r4), 'N = 4'),
            ('left position with Nr slots', gather(g['pr'], g['pr']), 'pos_l'),
        ]
        for what, (rc, outs, msg), names in cases:
            assert rc == F.FHE_EINVAL, (what, rc, msg)
            assert all(o is None for o in outs), what
            assert names in msg, (what, msg)
            if 'slots' in msg:
                assert '(8, 2)' in msg or ('8' in msg and '2' in msg), (what, msg)
    finally:
        gpu.set_pair_tables(0, 0)
