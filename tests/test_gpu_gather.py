"""Gather by encrypted position on the GPU (fhe_direct_gather).

Kernel level: k_sub_offsets_stacked and k_tensor_gather against the oracle ops
they fuse, member by member and word for word.  Operator level: gather, lag and
lead against the CPU-oracle composition of tests/gather_model.py, word for word,
on a tie-broken rank (LAG / LEAD with the present flags, and the summed ROWS
BETWEEN frame) and for two tables (col[idx] by an encrypted index), at N = 8 (one
comparator batch) and N = 64 (two: the stacked path), at every chunking, lane
count, column grouping and mask-cache setting and in the plain (unfused) form;
decrypted values against the exact neighbours.  Oracle results are computed once
per module and shared."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fhesort as F
import gather_model as GM
import pyoracle as O
import stable_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
KERNELS = ('k_sub_offsets_stacked', 'k_tensor_gather')

# Largest |decrypted - exact| of the CPU-oracle composition on these inputs and
# seeds (measured on the CPU).  The GPU words are the oracle's, so
# this is the GPU's error too; the tests assert 4x it, room for another seed's
# noise, not for a defect: a wrong word fails the word comparison first.
ORACLE_ERR = {
    (8, 'rank'): 2.357e-08,
    (64, 'rank'): 1.197e-06,
    (8, 'frame'): 1.198e-08,
    (64, 'frame'): 1.293e-06,
    (8, 'lookup'): 1.300e-08,
    (64, 'lookup'): 1.074e-06,
}
FRAME = [-1, 0, 1]


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
    """ring 2^12, L = 3, 40-bit scaling beside the 60-bit q0; 50 encrypted vectors at level 1"""
    orc = O.Context(12, 3, 40, 60, 3, seed=53)
    gpu = F.Context(12, 3, 40, 60, 3, seed=53, keygen=False)
    gpu.load_keys_from(orc, [])
    rng = np.random.default_rng(19)
    vals = [rng.uniform(-1, 1, 16) for _ in range(50)]
    octs = [orc.encrypt(v, 16, 1) for v in vals]
    gcts = [gpu.from_oracle(c) for c in octs]
    return orc, gpu, vals, octs, gcts


# offsets of both signs and zero; five of them and five batches cross the guarded tail of a thread's four
OFFSETS = {1: [-3], 4: [0, 2, -2, 15], 5: [-15, -1, 0, 1, 15]}


def oriented(orc, d, o):
    v = orc.add_const(d, float(o))
    return orc.negate(v) if o < 0 else v


def _check_sub_offsets(small, B, offs, la, launches):
    orc, gpu, vals, octs, gcts = small
    K = len(offs)
    oa = orc.encrypt(vals[0], 16, la)
    with F.KernelClock(gpu) as clk:
        R = gpu.sub_offsets_stacked(gpu.from_oracle(oa), gcts[1:1 + B], offs)
    assert clk.stats['k_sub_offsets_stacked']['launches'] == launches, sorted(clk.stats)
    with pytest.raises(F.FheError):
        gpu.member(R, K * B)
    for i in range(B):
        d = orc.sub(oa, octs[1 + i])
        for k, o in enumerate(offs):
            same(gpu.member(R, k * B + i), oriented(orc, d, o))


@pytest.mark.parametrize('K', [1, 4, 5])
@pytest.mark.parametrize('B', [1, 4, 5])
@pytest.mark.parametrize('la', [1, 0], ids=['same-level', 'a-one-level-below'])
def test_sub_offsets_stacked_matches_oracle(small, B, K, la):
    _check_sub_offsets(small, B, OFFSETS[K], la, 1)


def test_sub_offsets_stacked_second_launch(small):
    """33 batches under offsets of both signs: a launch takes 32, every offset's members stay 33 apart"""
    _check_sub_offsets(small, 33, [-2, 3], 1, 2)


@pytest.mark.parametrize('offs', [[0], [3], [-3, 0, 3]], ids=['zero', 'positive', 'mixed'])
def test_sub_offsets_stacked_with_a_above_the_operands(small, offs):
    """a deeper than the bs: every b is adjusted instead, so per-member ops (sub_stacked's rule)"""
    orc, gpu, vals, octs, gcts = small
    oa = orc.encrypt(vals[0], 16, 2)
    with F.KernelClock(gpu) as clk:
        R = gpu.sub_offsets_stacked(gpu.from_oracle(oa), gcts[1:4], offs)
    assert 'k_sub_offsets_stacked' not in clk.stats
    for i in range(3):
        d = orc.sub(oa, octs[1 + i])
        for k, o in enumerate(offs):
            same(gpu.member(R, k * 3 + i), oriented(orc, d, o))


def test_sub_offsets_stacked_refusals(small):
    orc, gpu, vals, octs, gcts = small
    a, b1 = gcts[0], gcts[1]
    b2 = gpu.encrypt(vals[2], 16, 2)
    for aa, bs, offs in ((a, [b1, b2], [1]), (a, [gpu.stack([b1, b1])], [1]), (gpu.stack([a, a]), [b1], [1]),
                         (a, [], [1]), (a, [b1], [])):
        with pytest.raises(F.FheError) as e:
            gpu.sub_offsets_stacked(aa, bs, offs)
        assert e.value.code == F.FHE_EINVAL


# five offsets cross the guarded tail of a thread's four; five columns and five batches leave every tile
@pytest.mark.parametrize('P', [1, 4, 5])
@pytest.mark.parametrize('K', [1, 4, 5])
@pytest.mark.parametrize('B', [1, 4, 5])
def test_mul_gather_matches_oracle(small, B, K, P):
    orc, gpu, vals, octs, gcts = small
    oa, ob = octs[0:K * B], octs[25:25 + P * B]
    with F.KernelClock(gpu) as clk:
        R = gpu.mul_gather(gpu.stack(gcts[0:K * B]), gpu.stack(gcts[25:25 + P * B]), P, K)
    assert launches(clk, 'k_tensor_gather') == 1 and not has(clk, 'k_tensor_pairs'), sorted(clk.stats)
    with pytest.raises(F.FheError):
        gpu.member(R, P * K * B)
    for p in range(P):
        for k in range(K):
            for z in range(B):
                same(gpu.member(R, (p * K + k) * B + z), orc.mul(oa[k * B + z], ob[p * B + z]))


def test_mul_gather_refusals(small):
    orc, gpu, vals, octs, gcts = small
    x2 = [gpu.encrypt(v, 16, 2) for v in vals[:4]]
    a, b = gpu.stack(gcts[:4]), gpu.stack(gcts[4:8])
    cases = [(a, b, 2, 3),                 # a is not 3 offsets of B
             (a, b, 3, 2),                 # b is not 3 columns of B = 2
             (a, gpu.stack(x2), 2, 2),     # b at another level
             (a, b, 0, 2),
             (a, b, 2, 0)]
    for aa, bb, ncols, noff in cases:
        with pytest.raises(F.FheError) as e:
            gpu.mul_gather(aa, bb, ncols, noff)
        assert e.value.code == F.FHE_EINVAL, (ncols, noff)


# ---------------------------------------------------------- operator level --
def oracle_case(N, seed):
    """the oracle half of a fixture (no GPU): contexts, inputs and expected outputs"""
    depth, rots = O.size_parameters(N)
    orc = O.Context(12, depth, 40, 60, 3, seed=seed)
    orc.gen_rotation_keys(rots)
    cfg = M.sign_cfg(N)
    rng = np.random.default_rng(seed)
    # LAG / LEAD: a tie-broken rank of tied keys, three columns entering at levels 0, 1 and the deepest allowed
    key = M.tied_input(N, M.SEEDS[N])
    ok = orc.encrypt(key, N)
    orank = M.oracle_rank(orc, ok, N, rots, cfg, 1.0 / N)
    col_max, ser_level, out_level = F.gather_levels(orank.level, N)
    vals = [rng.uniform(-1, 1, N), np.arange(N) / N, rng.uniform(-1, 1, N)]
    ocols = [orc.encrypt(v, N, lv) for v, lv in zip(vals, (0, 1, col_max))]
    offs = [-(N - 1), -1, 0, 1, N - 1]
    oouts, opres = GM.oracle_gather(orc, orank, orank, ocols, offs, N, rots, present=True)
    # the frame ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING: one column and the frame's row count
    fouts, fpres = GM.oracle_gather(orc, orank, orank, ocols[:1], FRAME, N, rots, present=True, sum_offsets=True)
    # two tables: col[idx + shift] with an encrypted iota; about a quarter of the indices leave the table
    shift = N // 4
    idx = rng.integers(0, N, N).astype(np.float64)
    idx[0], idx[1] = N - 1, 0  # both kinds are present
    jv = rng.uniform(-1, 1, N)
    oidx, oiota, ojv = orc.encrypt(idx, N), orc.encrypt(np.arange(N, dtype=np.float64), N), orc.encrypt(jv, N)
    louts, lpres = GM.oracle_gather(orc, oidx, oiota, [ojv], [shift], N, rots, present=True)
    return dict(N=N, seed=seed, orc=orc, depth=depth, rots=rots, cfg=cfg, key=key, ok=ok, orank=orank, vals=vals,
                ocols=ocols, offs=offs, oouts=oouts, opres=opres, fouts=fouts, fpres=fpres, col_max=col_max,
                ser_level=ser_level, out_level=out_level, shift=shift, idx=idx, jv=jv, oidx=oidx, oiota=oiota,
                ojv=ojv, louts=louts, lpres=lpres)


def oracle_errors(d):
    """largest |decrypted - exact| of the oracle composition: (rank, frame, lookup)"""
    pos = M.stable_ranks(d['key'])
    K = len(d['offs'])
    wouts, wpres = GM.exact(pos, pos, d['vals'], d['offs'])
    e_rank = max(max(np.max(np.abs(d['oouts'][p * K + k].decrypt() - wouts[p][k])) for p in range(3) for k in range(K)),
                 max(np.max(np.abs(d['opres'][k].decrypt() - wpres[k])) for k in range(K)))
    fo, fp = GM.exact(pos, pos, d['vals'][:1], FRAME)
    e_frame = max(np.max(np.abs(d['fouts'][0].decrypt() - fo[0].sum(axis=0))),
                  np.max(np.abs(d['fpres'][0].decrypt() - fp.sum(axis=0))))
    lo, lp = GM.exact(d['idx'], np.arange(d['N']), [d['jv']], [d['shift']])
    e_look = max(np.max(np.abs(d['louts'][0].decrypt() - lo[0][0])), np.max(np.abs(d['lpres'][0].decrypt() - lp[0])))
    return e_rank, e_frame, e_look


def _gather_ctx(N, seed):
    d = oracle_case(N, seed)
    gpu = F.Context(12, d['depth'], 40, 60, 3, seed=seed, keygen=False)
    gpu.load_keys_from(d['orc'], d['rots'])
    d.update(gpu=gpu, gk=gpu.from_oracle(d['ok']), grank=gpu.from_oracle(d['orank']),
             gcols=[gpu.from_oracle(c) for c in d['ocols']], gidx=gpu.from_oracle(d['oidx']),
             giota=gpu.from_oracle(d['oiota']), gjv=gpu.from_oracle(d['ojv']))
    return d


@pytest.fixture(scope='module')
def n8():
    """one comparator batch"""
    d = _gather_ctx(8, 828)
    assert M.rank_shape(8, d['orc'].n // 2)[2] == 1
    return d


@pytest.fixture(scope='module')
def n64():
    """N = 64 at ring 2^12: 2048 slots, two comparator batches (the stacked path)"""
    d = _gather_ctx(64, 884)
    assert M.rank_shape(64, d['orc'].n // 2)[2] == 2
    return d


def _lag_lead(d, stack=32, lanes=2, cache=True, members=F.SORT_COLUMN_MEMBERS_DEFAULT, cols=None, present=True,
              offs=None, sum_offsets=False):
    gpu = d['gpu']
    gpu.set_sort_stack(stack)
    gpu.set_sort_lanes(lanes)
    gpu.set_mask_cache(cache)
    gpu.set_sort_column_members(members)
    try:
        return gpu.gather(d['grank'], d['grank'], d['gcols'] if cols is None else cols,
                          d['offs'] if offs is None else offs, d['N'], d['rots'], present=present,
                          sum_offsets=sum_offsets)
    finally:
        gpu.set_sort_column_members(F.SORT_COLUMN_MEMBERS_DEFAULT)
        gpu.set_mask_cache(True)
        gpu.set_sort_lanes(2)
        gpu.set_sort_stack(32)


def _check_rank(d, outs, pres):
    assert len(outs) == len(d['oouts']) and len(pres) == len(d['opres'])
    for g, o in zip(outs, d['oouts']):
        same(g, o)
        assert g.level == d['out_level']
    for g, o in zip(pres, d['opres']):
        same(g, o)
        assert g.level == d['ser_level']


@pytest.mark.parametrize('cache', [True, False], ids=['cached', 'uncached'])
@pytest.mark.parametrize('lanes', [1, 2])
@pytest.mark.parametrize('stack', [1, 32])
@pytest.mark.parametrize('which', ['n8', 'n64'])
def test_lag_lead_matches_oracle_composition(request, which, stack, lanes, cache):
    d = request.getfixturevalue(which)
    with F.KernelClock(d['gpu']) as clk:
        outs, pres = _lag_lead(d, stack, lanes, cache)
    for name in KERNELS:
        assert has(clk, name), (name, sorted(clk.stats))
    _check_rank(d, outs, pres)


@pytest.mark.parametrize('members', [1, 2])
@pytest.mark.parametrize('which', ['n8', 'n64'])
def test_column_groups_give_the_same_words(request, which, members):
    """a member bound below P K B splits the three columns over several products"""
    d = request.getfixturevalue(which)
    with F.KernelClock(d['gpu']) as clk:
        outs, pres = _lag_lead(d, members=members)
    assert launches(clk, 'k_tensor_gather') >= 2, sorted(clk.stats)
    _check_rank(d, outs, pres)


@pytest.mark.parametrize('which', ['n8', 'n64'])
def test_lag_and_lead_wrappers(request, which):
    """lag(k) is offset -k, lead(k) offset +k: the matching outputs of the five-offset call"""
    d = request.getfixturevalue(which)
    gpu, K = d['gpu'], len(d['offs'])
    lag, lpres = gpu.lag(d['grank'], d['gcols'], 1, d['N'], d['rots'], present=True)
    lead = gpu.lead(d['grank'], d['gcols'][:1], 1, d['N'], d['rots'])
    for p in range(3):
        same(lag[p], d['oouts'][p * K + d['offs'].index(-1)])
    same(lpres[0], d['opres'][d['offs'].index(-1)])
    assert len(lead) == 1
    same(lead[0], d['oouts'][d['offs'].index(1)])


def test_decrypted_lag_lead_are_the_neighbours(n8, n64):
    for d in (n8, n64):
        outs, pres = _lag_lead(d)
        pos = M.stable_ranks(d['key'])
        K = len(d['offs'])
        wouts, wpres = GM.exact(pos, pos, d['vals'], d['offs'])
        err = max(max(np.max(np.abs(d['gpu'].decrypt(outs[p * K + k]) - wouts[p][k])) for p in range(3) for k in range(K)),
                  max(np.max(np.abs(d['gpu'].decrypt(pres[k]) - wpres[k])) for k in range(K)))
        print(f"N={d['N']} lag/lead: max error {err:.3e} (oracle composition {ORACLE_ERR[(d['N'], 'rank')]:.3e})")
        # the last row has no LEAD(1), the first no LAG(1); offsets +-(N - 1) leave one neighbour each
        assert wpres[d['offs'].index(1)].sum() == d['N'] - 1 and wpres[d['offs'].index(d['N'] - 1)].sum() == 1
        assert err <= 4 * ORACLE_ERR[(d['N'], 'rank')]


@pytest.mark.parametrize('which', ['n8', 'n64'])
def test_summed_frame(request, which):
    """sum_offsets over {-1, 0, 1}: ROWS BETWEEN 1 PRECEDING AND 1 FOLLOWING and the frame's row count"""
    d = request.getfixturevalue(which)
    gpu = d['gpu']
    outs, pres = _lag_lead(d, cols=d['gcols'][:1], offs=FRAME, sum_offsets=True)
    assert len(outs) == 1 and len(pres) == 1
    same(outs[0], d['fouts'][0])
    same(pres[0], d['fpres'][0])
    pos = M.stable_ranks(d['key'])
    fo, fp = GM.exact(pos, pos, d['vals'][:1], FRAME)
    want, cnt = fo[0].sum(axis=0), fp.sum(axis=0)
    assert set(cnt) == {2.0, 3.0}
    err = max(np.max(np.abs(gpu.decrypt(outs[0]) - want)), np.max(np.abs(gpu.decrypt(pres[0]) - cnt)))
    print(f"N={d['N']} frame: max error {err:.3e} (oracle composition {ORACLE_ERR[(d['N'], 'frame')]:.3e})")
    assert err <= 4 * ORACLE_ERR[(d['N'], 'frame')]


@pytest.mark.parametrize('which', ['n8', 'n64'])
def test_lookup_by_encrypted_index(request, which):
    """pos_r an encrypted iota, pos_l encrypted indices: col[idx + shift], zero past the table's end"""
    d = request.getfixturevalue(which)
    gpu, N = d['gpu'], d['N']
    outs, pres = gpu.gather(d['gidx'], d['giota'], [d['gjv']], [d['shift']], N, d['rots'], present=True)
    same(outs[0], d['louts'][0])
    same(pres[0], d['lpres'][0])
    q = d['idx'].astype(int) + d['shift']
    outside = q >= N
    assert N // 8 <= outside.sum() <= N // 2  # about a quarter
    want = np.where(outside, 0.0, d['jv'][np.clip(q, 0, N - 1)])
    got, gp = gpu.decrypt(outs[0]), gpu.decrypt(pres[0])
    err = max(np.max(np.abs(got - want)), np.max(np.abs(gp - (~outside))))
    print(f"N={N} lookup: max error {err:.3e}, outside slots {np.max(np.abs(got[outside])):.3e} "
          f"(oracle composition {ORACLE_ERR[(N, 'lookup')]:.3e})")
    assert err <= 4 * ORACLE_ERR[(N, 'lookup')]


def test_present_alone_and_columns_alone(n8):
    d = n8
    K = len(d['offs'])
    outs, pres = _lag_lead(d, cols=[], present=True)
    assert outs == []
    for g, o in zip(pres, d['opres']):
        same(g, o)
    outs = _lag_lead(d, cols=d['gcols'][:1], present=False)
    assert len(outs) == K
    for g, o in zip(outs, d['oouts'][:K]):
        same(g, o)


def test_tiebreak_setting_has_no_effect(n8):
    d = n8
    d['gpu'].set_sort_tiebreak(1.0 / d['N'])
    try:
        outs, pres = _lag_lead(d)
    finally:
        d['gpu'].set_sort_tiebreak(0.0)
    _check_rank(d, outs, pres)


CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import fhesort as F
import pyoracle as O
work, N, seed = sys.argv[3], int(sys.argv[4]), int(sys.argv[5])
offs = [int(v) for v in sys.argv[6].split(',')]
depth, rots = O.size_parameters(N)
orc = O.Context(12, depth, 40, 60, 3, seed=seed)
orc.gen_rotation_keys(rots)
gpu = F.Context(12, depth, 40, 60, 3, seed=seed, keygen=False)
gpu.load_keys_from(orc, rots)
meta = np.load(work + '/meta.npy')
cts = [gpu.upload(np.load(work + f'/in{i}.npy'), int(meta[i][0]), N, meta[i][1]) for i in range(len(meta))]
with F.KernelClock(gpu) as clk:
    outs, pres = gpu.gather(cts[0], cts[0], cts[1:], offs, N, rots, present=True)
assert not any(k.startswith(('k_sub_offsets_stacked', 'k_tensor_gather')) for k in clk.stats), sorted(clk.stats)
for i, o in enumerate(outs + pres):
    np.save(work + f'/out{i}.npy', o.data())
    inf = o.info()
    np.save(work + f'/out{i}_meta.npy', np.array([inf['level'], inf['slots'], inf['scale']], dtype=np.float64))
print('ALLOK')
'''


def test_plain_form_gives_the_same_words(n64, tmp_path):
    """FHE_GATHER_FUSED=0 (read once per process, so a fresh child): sub_stacked with
    add_const / negate on the stack per offset, and one stacked mul per column and offset"""
    d = n64
    ins = [d['orank']] + d['ocols']
    np.save(tmp_path / 'meta.npy', np.array([[c.info()['level'], c.info()['scale']] for c in ins], dtype=np.float64))
    for i, c in enumerate(ins):
        np.save(tmp_path / f'in{i}.npy', c.data())
    env = dict(os.environ, FHE_GATHER_FUSED='0')
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'),
                        os.path.join(REPO, 'oracle'), str(tmp_path), str(d['N']), str(d['seed']),
                        ','.join(str(o) for o in d['offs'])], env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
    for i, o in enumerate(d['oouts'] + d['opres']):
        oi = o.info()
        assert np.load(tmp_path / f'out{i}_meta.npy').tolist() == [oi['level'], oi['slots'], oi['scale']], i
        assert np.array_equal(np.load(tmp_path / f'out{i}.npy'), o.data()), i


# --------------------------------------------------------------- refusals --
def _raw_call(gpu, pl, pr, cols, ncols, offs, N, rots, present=True, sum_offsets=False):
    """fhe_direct_gather itself: (status, the output handles it left, the message)"""
    r = np.asarray(rots, dtype=np.int32)
    off = np.asarray(offs, dtype=np.int32)
    ko = 1 if sum_offsets else len(off)
    nout = max(1, (max(ncols, 0) + (1 if present else 0)) * ko)
    arr = (C.c_void_p * max(1, len(cols)))(*[None if c is None else c.h for c in cols])
    outs = (C.c_void_p * nout)(*([0xdead] * nout))
    rc = F.lib().fhe_direct_gather(gpu.h, None if pl is None else pl.h, None if pr is None else pr.h, arr, ncols,
                                   F._int(off) if len(off) else None, len(off), int(present), int(sum_offsets), N,
                                   F._int(r), len(r), outs)
    left = [outs[i] for i in range((max(ncols, 0) + (1 if present else 0)) * ko)]
    return rc, left, F.lib().fhe_last_error().decode()


def test_refusals(n8):
    d = n8
    gpu, N, rots = d['gpu'], d['N'], d['rots']
    pos, col = d['grank'], d['gcols'][0]
    wide = gpu.encrypt(np.zeros(2 * N), 2 * N, pos.level)
    deeper_pos = gpu.level_adjust(pos, pos.level + 1)
    too_deep = gpu.level_adjust(col, d['col_max'] + 1)
    stacked = gpu.stack([col, col])
    cases = [
        ('null left position', None, pos, [col], 1, [1], True, F.FHE_EINVAL, 'left position'),
        ('null right position', pos, None, [col], 1, [1], True, F.FHE_EINVAL, 'right position'),
        ('position is a stack', pos, gpu.stack([pos, pos]), [col], 1, [1], True, F.FHE_EINVAL, 'right position'),
        ('position slots', pos, wide, [col], 1, [1], True, F.FHE_EINVAL, 'slots'),
        ('position levels', pos, deeper_pos, [col], 1, [1], True, F.FHE_EINVAL, 'levels'),
        ('null column', pos, pos, [col, None], 2, [1], True, F.FHE_EINVAL, 'column 1'),
        ('column is a stack', pos, pos, [col, col, stacked], 3, [1], True, F.FHE_EINVAL, 'column 2'),
        ('column slots', pos, pos, [wide, col], 2, [1], True, F.FHE_EINVAL, 'column 0'),
        ('no offsets', pos, pos, [col], 1, [], True, F.FHE_EINVAL, 'noffsets'),
        ('offset N', pos, pos, [col], 1, [0, N], True, F.FHE_EINVAL, 'offset 1'),
        ('offset -N', pos, pos, [col], 1, [-N], True, F.FHE_EINVAL, 'offset 0'),
        ('negative ncols', pos, pos, [col], -1, [1], True, F.FHE_EINVAL, 'ncols'),
        ('nothing asked for', pos, pos, [], 0, [1], False, F.FHE_EINVAL, None),
        ('column one level too deep', pos, pos, [col, too_deep], 2, [1], True, F.FHE_EDEPTH, 'column 1'),
    ]
    for what, pl, pr, cols, ncols, offs, present, status, names in cases:
        rc, outs, msg = _raw_call(gpu, pl, pr, cols, ncols, offs, N, rots, present)
        assert rc == status, (what, rc, msg)
        assert all(o is None for o in outs), what  # every output handle still null
        if names:
            assert names in msg, (what, msg)
    # the deepest allowed column is served (it is column 2 of the fixture)
    assert d['ocols'][2].level == d['col_max']


def test_shallow_context_is_refused(small):
    """a context without the series' levels: FHE_EDEPTH before any work"""
    _, gpu, vals, _, _ = small
    _, rots = O.size_parameters(8)
    pos = gpu.encrypt(np.arange(8.0), 8)
    rc, outs, msg = _raw_call(gpu, pos, pos, [pos], 1, [1], 8, rots)
    assert rc == F.FHE_EDEPTH, (rc, msg)
    assert all(o is None for o in outs)


# ---------------------------------------------------- the sort is untouched --
def test_sort_after_gather_reproduces_the_oracle(n8):
    """the columns' masks are further entries of the sorter's cache; the sort's own are undisturbed"""
    d = n8
    gpu, orc, N = d['gpu'], d['orc'], d['N']
    _check_rank(d, *_lag_lead(d))
    same(gpu.direct_sort(d['gk'], N, d['rots'], d['cfg']), orc.direct_sort(d['ok'], N, d['rots'], d['cfg']))
    _check_rank(d, *_lag_lead(d, cache=False))
    same(gpu.direct_sort(d['gk'], N, d['rots'], d['cfg'], mode=1),
         orc.direct_sort(d['ok'], N, d['rots'], d['cfg'], mode=1))
