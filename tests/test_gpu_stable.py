"""Tie-breaking DirectSort on the GPU (fhe_set_sort_tiebreak).

Kernel level: k_sub_add_plain_stacked against the oracle's add_plain(sub(a, b_i),
p_i) and k_tiebreak_slots against the host and oracle encoders, word for word.
Rank level: direct_sort(mode=1) under set_sort_tiebreak(1 / N) against the
CPU-oracle composition of tests/stable_model.py, word for word, at every
chunking, lane count and mask-cache setting and in the plain (unfused) form.
End to end: tied inputs sort, records come out in the stable permutation and
order statistics are exact, within the reference's DirectSortTest bound.
Oracle results are computed once per module and shared."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fhesort as F
import pyoracle as O
import stable_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
BOUND = 0.01  # the reference's DirectSortTest bound


def same(g, o):
    """equal level, slots, scale and words"""
    gi, oi = g.info(), o.info()
    assert (gi['level'], gi['slots'], gi['limbs'], gi['scale']) == (oi['level'], oi['slots'], oi['limbs'], oi['scale'])
    gd, od = g.data(), o.data()
    if not np.array_equal(gd, od):
        bad = np.argwhere(gd != od)
        raise AssertionError(f'{len(bad)} limb words differ, first at {bad[0].tolist()}')


# ------------------------------------------------------------ kernel level --
@pytest.fixture(scope='module')
def small():
    """ring 2^12, L = 3, 40-bit scaling beside the 60-bit q0"""
    orc = O.Context(12, 3, 40, 60, 3, seed=43)
    gpu = F.Context(12, 3, 40, 60, 3, seed=43, keygen=False)
    gpu.load_keys_from(orc, [])
    rng = np.random.default_rng(13)
    vals = [rng.uniform(-1, 1, 16) for _ in range(6)]
    pvals = [rng.uniform(-1, 1, 16) for _ in range(5)]
    # drawn after the others, which keep their values: operands and offsets for a second launch
    vals += [rng.uniform(-1, 1, 16) for _ in range(28)]
    pvals += [rng.uniform(-1, 1, 16) for _ in range(28)]
    return orc, gpu, vals, pvals


def _check_sub_add_plain(small, B, la, lb, launches):
    orc, gpu, vals, pvals = small
    oa = orc.encrypt(vals[0], 16, la)
    obs = [orc.encrypt(v, 16, lb) for v in vals[1:1 + B]]
    lev = max(la, lb)
    with F.KernelClock(gpu) as clk:
        R = gpu.sub_add_plain_stacked(gpu.from_oracle(oa), [gpu.from_oracle(b) for b in obs],
                                      [gpu.encode(p, 16, lev) for p in pvals[:B]])
    assert clk.stats['k_sub_add_plain_stacked']['launches'] == launches, sorted(clk.stats)
    with pytest.raises(F.FheError):
        gpu.member(R, B)
    for i in range(B):
        same(gpu.member(R, i), orc.add_plain(orc.sub(oa, obs[i]), orc.encode(pvals[i], 16, lev)))


# five members cross the guarded tail of a thread's four
@pytest.mark.parametrize('B', [1, 4, 5])
@pytest.mark.parametrize('la,lb', [(1, 1), (0, 1)], ids=['same-level', 'a-one-level-below'])
def test_sub_add_plain_stacked_matches_oracle(small, B, la, lb):
    _check_sub_add_plain(small, B, la, lb, 1)


def test_sub_add_plain_stacked_second_launch(small):
    """33 members: a launch takes 32, so member 32 comes from a second launch's table"""
    _check_sub_add_plain(small, 33, 1, 1, 2)


def test_sub_add_plain_stacked_with_a_above_the_operands(small):
    """a deeper than the bs: every b is adjusted instead, so per-member ops (sub_stacked's rule)"""
    orc, gpu, vals, pvals = small
    oa = orc.encrypt(vals[0], 16, 2)
    obs = [orc.encrypt(v, 16, 1) for v in vals[1:4]]
    with F.KernelClock(gpu) as clk:
        R = gpu.sub_add_plain_stacked(gpu.from_oracle(oa), [gpu.from_oracle(b) for b in obs],
                                      [gpu.encode(p, 16, 2) for p in pvals[:3]])
    assert 'k_sub_add_plain_stacked' not in clk.stats
    for i in range(3):
        same(gpu.member(R, i), orc.add_plain(orc.sub(oa, obs[i]), orc.encode(pvals[i], 16, 2)))


def test_sub_add_plain_stacked_refusals(small):
    orc, gpu, vals, pvals = small
    a = gpu.encrypt(vals[0], 16, 1)
    b1, b2 = gpu.encrypt(vals[1], 16, 1), gpu.encrypt(vals[2], 16, 2)
    p1, p2 = gpu.encode(pvals[0], 16, 1), gpu.encode(pvals[1], 16, 2)
    for bs, ps in (([b1, b2], [p1, p1]), ([b1], [p2]), ([b1, b1], [p1, p2]), ([gpu.stack([b1, b1])], [p1])):
        with pytest.raises(F.FheError) as e:
            gpu.sub_add_plain_stacked(a, bs, ps)
        assert e.value.code == F.FHE_EINVAL


def test_encode_tiebreak_matches_host_and_oracle_encode(small):
    """two batches of S = 64 slots over N = 16 (P_ = 4 < N), at level 1"""
    orc, gpu, _, _ = small
    N, S, eps = 16, 64, 1.0 / 16
    with F.KernelClock(gpu) as clk:
        got = gpu.encode_tiebreak([1, 3], S, N, eps, 1)
    assert clk.stats['k_tiebreak_slots']['launches'] == 1, sorted(clk.stats)
    for b, p in zip((1, 3), got):
        v = F.tiebreak_offsets(N, S, b, eps)
        assert np.array_equal(v, M.offsets(N, S, b, eps))
        assert np.array_equal(p.data(), gpu.encode(v, S, 1).data()), b
        assert np.array_equal(p.data(), orc.encode(v, S, 1).data()), b
    for args in (([4], S, N, eps, 1), ([0], S, N, 0.5, 1), ([0], S, N, eps, 9), ([0], 48, N, eps, 1)):
        with pytest.raises(F.FheError) as e:
            gpu.encode_tiebreak(*args)
        assert e.value.code == F.FHE_EINVAL, args


def test_set_sort_tiebreak_validates(small):
    _, gpu, _, _ = small
    for eps in (-1.0, 0.5, float('nan')):
        with pytest.raises(F.FheError) as e:
            gpu.set_sort_tiebreak(eps)
        assert e.value.code == F.FHE_EINVAL, eps
    gpu.set_sort_tiebreak(0.25)
    gpu.set_sort_tiebreak(0.0)


# -------------------------------------------------------------- rank level --
def _rank_ctx(N, seed):
    depth, rots = O.size_parameters(N)
    orc = O.Context(12, depth, 40, 60, 3, seed=seed)
    orc.gen_rotation_keys(rots)
    gpu = F.Context(12, depth, 40, 60, 3, seed=seed, keygen=False)
    gpu.load_keys_from(orc, rots)
    cfg = M.sign_cfg(N)
    x = M.tied_input(N, M.SEEDS[N])
    ox = orc.encrypt(x, N)
    orank = M.oracle_rank(orc, ox, N, rots, cfg, 1.0 / N)
    return dict(N=N, orc=orc, gpu=gpu, depth=depth, rots=rots, cfg=cfg, x=x, ox=ox, gx=gpu.from_oracle(ox),
                orank=orank, seed=seed)


@pytest.fixture(scope='module')
def n8():
    """one comparator batch"""
    d = _rank_ctx(8, 808)
    assert M.rank_shape(8, d['orc'].n // 2)[2] == 1
    return d


@pytest.fixture(scope='module')
def n64():
    """N = 64 at ring 2^12: 2048 slots, two comparator batches (the stacked path)"""
    d = _rank_ctx(64, 864)
    assert M.rank_shape(64, d['orc'].n // 2)[2] == 2
    return d


def _stable_rank(d, stack=32, lanes=2, cache=True):
    gpu, N = d['gpu'], d['N']
    gpu.set_sort_stack(stack)
    gpu.set_sort_lanes(lanes)
    gpu.set_mask_cache(cache)
    gpu.set_sort_tiebreak(1.0 / N)
    try:
        return gpu.direct_sort(d['gx'], N, d['rots'], d['cfg'], mode=1)
    finally:
        gpu.set_sort_tiebreak(0.0)
        gpu.set_mask_cache(True)
        gpu.set_sort_lanes(2)
        gpu.set_sort_stack(32)


@pytest.mark.parametrize('cache', [True, False], ids=['cached', 'uncached'])
@pytest.mark.parametrize('lanes', [1, 2])
@pytest.mark.parametrize('stack', [1, 32])
@pytest.mark.parametrize('which', ['n8', 'n64'])
def test_stable_rank_matches_oracle_composition(request, which, stack, lanes, cache):
    d = request.getfixturevalue(which)
    gpu, N = d['gpu'], d['N']
    with F.KernelClock(gpu) as clk:
        rank = _stable_rank(d, stack, lanes, cache)
    assert 'k_sub_add_plain_stacked' in clk.stats, sorted(clk.stats)
    if not cache:
        assert 'k_tiebreak_slots' in clk.stats  # re-encoded at the start of the rank
    same(rank, d['orank'])
    err = np.max(np.abs(gpu.decrypt(rank) - M.stable_ranks(d['x'])))
    print(f'N={N} stack={stack} lanes={lanes} cache={cache}: stable rank error {err:.3e}')
    assert err < 1e-4


def test_offsets_are_cached_per_context(n64):
    d = n64
    _stable_rank(d)
    with F.KernelClock(d['gpu']) as clk:
        same(_stable_rank(d), d['orank'])
    assert 'k_tiebreak_slots' not in clk.stats


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
x = gpu.upload(np.load(work + '/x.npy'), int(meta[0]), N, meta[1])
gpu.set_sort_lanes(1)
gpu.set_sort_tiebreak(1.0 / N)
with F.KernelClock(gpu) as clk:
    rank = gpu.direct_sort(x, N, rots, cfg, mode=1)
assert 'k_sub_add_plain_stacked' not in clk.stats, sorted(clk.stats)
np.save(work + '/rank.npy', rank.data())
i = rank.info()
np.save(work + '/rank_meta.npy', np.array([i['level'], i['slots'], i['scale']], dtype=np.float64))
print('ALLOK')
'''


def test_plain_form_gives_the_same_words(n64, tmp_path):
    """FHE_TIEBREAK_FUSED=0 (read once per process, so a fresh child): sub_stacked,
    then one c0 addition per member, on the two-member stack of N = 64"""
    d = n64
    inf = d['ox'].info()
    np.save(tmp_path / 'meta.npy', np.array([inf['level'], inf['scale']], dtype=np.float64))
    np.save(tmp_path / 'x.npy', d['ox'].data())
    env = dict(os.environ, FHE_TIEBREAK_FUSED='0')
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'),
                        os.path.join(REPO, 'oracle'), str(tmp_path), str(d['N']), str(d['seed'])], env=env,
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
    oi = d['orank'].info()
    assert np.load(tmp_path / 'rank_meta.npy').tolist() == [oi['level'], oi['slots'], oi['scale']]
    assert np.array_equal(np.load(tmp_path / 'rank.npy'), d['orank'].data())


# -------------------------------------------------------------- end to end --
def test_tied_input_sorts(n8):
    d = n8
    gpu, N, x = d['gpu'], d['N'], d['x']
    plain = gpu.direct_sort(d['gx'], N, d['rots'], d['cfg'])
    gpu.set_sort_tiebreak(1.0 / N)
    try:
        out = gpu.direct_sort(d['gx'], N, d['rots'], d['cfg'])
    finally:
        gpu.set_sort_tiebreak(0.0)
    same(out, d['orc'].direct_sort(d['ox'], N, d['rots'], d['cfg'], mode=2, rank=d['orank']))
    err = np.max(np.abs(gpu.decrypt(out) - np.sort(x)))
    perr = np.max(np.abs(gpu.decrypt(plain) - np.sort(x)))
    print(f'N={N} tied input: sort error {err:.3e} with the tie-break, {perr:.3e} without')
    assert out.level == plain.level == d['depth']
    assert err < BOUND
    assert perr > 0.1  # the plain sort does not sort this input


def test_records_come_out_in_the_stable_permutation(n8):
    d = n8
    gpu, N, x = d['gpu'], d['N'], d['x']
    rng = np.random.default_rng(88)
    vals = [rng.uniform(-1, 1, N), np.arange(N) / N]
    cols = [gpu.encrypt(v, N) for v in vals]
    gpu.set_sort_tiebreak(1.0 / N)
    try:
        outs = gpu.direct_sort_columns(d['gx'], cols, N, d['rots'], d['cfg'])
    finally:
        gpu.set_sort_tiebreak(0.0)
    order = np.argsort(x, kind='stable')
    for v, o in zip(vals, outs):
        err = np.max(np.abs(gpu.decrypt(o) - v[order]))
        print(f'N={N} payload column: max error {err:.3e}')
        assert err < BOUND


def test_order_statistics_are_exact(n8):
    d = n8
    gpu, N, x = d['gpu'], d['N'], d['x']
    targets = [0, N // 2, N - 1]
    gpu.set_sort_tiebreak(1.0 / N)
    try:
        got = gpu.direct_select(d['gx'], targets, N, d['rots'], d['cfg'])
    finally:
        gpu.set_sort_tiebreak(0.0)
    dec = gpu.decrypt(got)
    err = np.max(np.abs(dec[:3] - np.sort(x)[targets]))
    print(f'N={N} minimum, median, maximum: max error {err:.3e}, other slots {np.max(np.abs(dec[3:])):.3e}')
    assert err < BOUND and np.max(np.abs(dec[3:])) < BOUND


# -------------------------------------------------------------- off switch --
def test_switch_off_is_the_plain_rank(n8):
    d = n8
    gpu, N = d['gpu'], d['N']
    same(_stable_rank(d), d['orank'])
    with F.KernelClock(gpu) as clk:
        rank = gpu.direct_sort(d['gx'], N, d['rots'], d['cfg'], mode=1)
    assert 'k_sub_add_plain_stacked' not in clk.stats and 'k_tiebreak_slots' not in clk.stats
    same(rank, d['orc'].direct_sort(d['ox'], N, d['rots'], d['cfg'], mode=1))
