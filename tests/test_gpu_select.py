"""Order statistics by encrypted rank (fhe_direct_select): slot p of the output
holds the value whose rank is targets[p], from one index series per member
instead of the sort's N / num_partition stacked ones.

The reference has no such function, so every output is held word for word to
a composition of CPU-oracle ops that restates the definition (oracle_select
below), and within the reference's DirectSortTest bound of the plaintext order
statistics.  The two kernels under it (k_select_slots, k_mul_plain_sum_groups)
are held to the oracle's encode and mul_plain_sum.  Oracle results are computed
once per module and shared.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fhesort as F
import pyoracle as O
import select_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
BOUND = 0.01  # the reference's DirectSortTest bound; inputs have |x| <= 1 and distinct keys


def same(g, o):
    """equal level, slots and words"""
    gi, oi = g.info(), o.info()
    assert (gi['level'], gi['slots'], gi['limbs'], gi['scale']) == (oi['level'], oi['slots'], oi['limbs'], oi['scale'])
    gd, od = g.data(), o.data()
    if not np.array_equal(gd, od):
        bad = np.argwhere(gd != od)
        raise AssertionError(f'{len(bad)} limb words differ, first at {bad[0].tolist()}')


def same_words(g, h):
    assert g.info() == h.info()
    assert np.array_equal(g.data(), h.data())


def with_slots(orc, ct, slots):
    """a copy of the oracle ciphertext with its slot count set (the original is shared)"""
    inf = ct.info()
    return orc.ct_from(ct.data(), inf['level'], slots, inf['scale'])


def oracle_select(orc, orank, ocols, targets, N, S):
    """The definition, op by op on the CPU oracle: per member z the difference
    C_z - rank, the sort's scaling and doubled-sinc series, the product with every
    column, the window sums by log2(N) rotations; then per column the pick sum
    over all members with one rescale, and the sort's fold."""
    members, _, _ = F.select_layout(N, S, len(targets))
    coeffs = O.doubled_sinc(N)
    rk = with_slots(orc, orank, S)
    neg = orc.negate(rk)
    vs = [[] for _ in ocols]
    Ks = []
    for z in range(members):
        Cz, Kz = M.vectors(N, S, targets, z)
        Ks.append(Kz)
        d = orc.add_plain(neg, orc.encode(Cz, S, rk.level))
        r = orc.cheb(orc.mul_const(d, 1.0 / (2 * N)), coeffs, -1.0, 1.0)
        for c, col in enumerate(ocols):
            v = orc.mul(r, with_slots(orc, orc.level_adjust(col, r.level), S))
            for i in range(int(np.log2(N))):
                v = orc.add(v, orc.rotate(v, 1 << i))
            vs[c].append(v)
    outs = []
    for c in range(len(ocols)):
        out = orc.mul_plain_sum(vs[c], [orc.encode(Kz, S, vs[c][0].level) for Kz in Ks])
        i = 1
        while (1 << i) <= S // N:
            out = orc.add(out, orc.rotate(out, S >> i))
            i += 1
        out.set_slots(N)
        outs.append(out)
    return outs


# ------------------------------------------------------------ kernel level --
@pytest.fixture(scope='module')
def small():
    """ring 2^12, L = 3, 40-bit scaling beside the 60-bit q0"""
    orc = O.Context(12, 3, 40, 60, 3, seed=41)
    gpu = F.Context(12, 3, 40, 60, 3, seed=41, keygen=False)
    gpu.load_keys_from(orc, [])
    rng = np.random.default_rng(12)
    cts = [orc.encrypt(rng.uniform(-1, 1, 16), 16, 1) for _ in range(10)]
    pts = [rng.uniform(-1, 1, 16) for _ in range(3)]
    return orc, gpu, cts, pts


@pytest.mark.parametrize('N,S,targets', [(16, 256, list(range(15, -1, -1))), (4, 4, [2, 0, 3, 1])])
def test_encode_select_matches_oracle_encode(small, N, S, targets):
    """members 0 and 1 (the second starts its windows at member * cap), C and K
    at either level order"""
    orc, gpu, _, _ = small
    with F.KernelClock(gpu) as clk:
        got = {(z, lv): gpu.encode_select(targets, z, S, N, *lv) for z in (0, 1) for lv in ((0, 2), (2, 1))}
    # the clock covers the encoder's slot kernel (launched through the clocked path)
    assert any(k.startswith('k_select_slots') for k in clk.stats), sorted(clk.stats)
    for (z, (lc, lk)), (c, k) in got.items():
        Cz, Kz = M.vectors(N, S, targets, z)
        assert Kz.sum() == min(M.cap_of(N, S), len(targets) - z * M.cap_of(N, S))
        assert np.array_equal(c.data(), orc.encode(Cz, S, lc).data()), (z, lc)
        assert np.array_equal(k.data(), orc.encode(Kz, S, lk).data()), (z, lk)


def test_encode_select_refuses_bad_arguments(small):
    _, gpu, _, _ = small
    for args in (([0, 1], 2, 256, 16, 0, 1), ([0, 16], 0, 256, 16, 0, 1), ([0], 0, 256, 16, 0, 9), ([0], 0, 24, 16, 0, 1),
                 ([0] * 17, 0, 256, 16, 0, 1)):
        with pytest.raises(F.FheError) as e:
            gpu.encode_select(*args)
        assert e.value.code == F.FHE_EINVAL, args


# (5, 2): five groups cross the guarded tail of a thread's PLAIN_SUM_GROUPS_PER_THREAD groups
@pytest.mark.parametrize('G,Z', [(2, 3), (1, 1), (F.PLAIN_SUM_GROUPS_PER_THREAD + 1, 2)])
def test_mul_plain_sum_groups_matches_oracle(small, G, Z):
    orc, gpu, cts, pts = small
    assert G * Z <= len(cts)
    opts = [orc.encode(p, 16, 1) for p in pts[:Z]]
    gpts = [gpu.encode(p, 16, 1) for p in pts[:Z]]
    stack = gpu.stack([gpu.from_oracle(c) for c in cts[:G * Z]])
    with F.KernelClock(gpu) as clk:
        R = gpu.mul_plain_sum_groups(stack, gpts, G)
    assert any(k.startswith('k_mul_plain_sum_groups') for k in clk.stats), sorted(clk.stats)
    for g in range(G):
        same(gpu.member(R, g), orc.mul_plain_sum(cts[g * Z:(g + 1) * Z], opts))
    for bad in (G + 1, 0):
        with pytest.raises(F.FheError) as e:
            gpu.mul_plain_sum_groups(stack, gpts, bad)
        assert e.value.code == F.FHE_EINVAL


# ------------------------------------------------ N = 16: P_ = 16, cap = 15 --
N16, CFG16, S16 = 16, (3, 2, 2), 256
TARGETS16 = (list(range(16)), [15, 0, 8], [3])  # 16 targets: two members, the second shifted by cap


@pytest.fixture(scope='module')
def n16():
    depth, rots = O.size_parameters(N16)
    orc = O.Context(12, depth, 40, 60, 3, seed=116)
    orc.gen_rotation_keys(rots)
    gpu = F.Context(12, depth, 40, 60, 3, seed=116, keygen=False)
    gpu.load_keys_from(orc, rots)
    rng = np.random.default_rng(20250704)
    key = rng.permutation(N16) / N16
    vals = [key, rng.uniform(-1, 1, N16), rng.uniform(-1, 1, N16)]
    okey = orc.encrypt(key, N16)
    ocols = [okey, orc.encrypt(vals[1], N16), orc.level_adjust(orc.encrypt(vals[2], N16), 2)]
    orank = orc.direct_sort(okey, N16, rots, CFG16, mode=1)
    okeysel = {tuple(t): oracle_select(orc, orank, [okey], t, N16, S16)[0] for t in TARGETS16}
    ocolsel = oracle_select(orc, orank, ocols[1:], [15, 0, 8], N16, S16)
    gkey = gpu.from_oracle(okey)
    gcols = [gkey] + [gpu.from_oracle(c) for c in ocols[1:]]
    grank = gpu.from_oracle(orank)
    return dict(orc=orc, gpu=gpu, depth=depth, rots=rots, key=key, vals=vals, okey=okey, ocols=ocols, orank=orank,
                okeysel=okeysel, ocolsel=ocolsel, gkey=gkey, gcols=gcols, grank=grank)


@pytest.mark.parametrize('targets', TARGETS16, ids=lambda t: f'k{len(t)}')
def test_select_matches_oracle_and_plaintext(n16, targets):
    d = n16
    gpu = d['gpu']
    k = len(targets)
    got = gpu.direct_select(d['gkey'], targets, N16, d['rots'], CFG16, rank=d['grank'])
    same(got, d['okeysel'][tuple(targets)])
    assert got.level == d['depth'] and got.slots == N16
    dec = gpu.decrypt(got)
    err = np.max(np.abs(dec[:k] - np.sort(d['key'])[targets]))
    tail = np.max(np.abs(dec[k:])) if k < N16 else 0.0
    print(f'select k={k}: max error {err:.3e}, max |slot >= k| {tail:.3e}')
    assert err < BOUND and tail < BOUND
    if k == N16:  # every rank in order: the sort itself
        full = gpu.decrypt(gpu.direct_sort(d['gkey'], N16, d['rots'], CFG16, mode=2, rank=d['grank']))
        assert np.max(np.abs(dec - full)) < BOUND


def test_columns_equal_single_column_selects(n16):
    """three columns (one pre-adjusted to level 2) against the select of each alone
    and against the oracle composition"""
    d = n16
    gpu, t = d['gpu'], [15, 0, 8]
    outs = gpu.direct_select(None, t, N16, d['rots'], CFG16, cols=d['gcols'], rank=d['grank'])
    assert len(outs) == 3
    order = np.argsort(d['key'])
    for c, o in enumerate(outs):
        one = gpu.direct_select(None, t, N16, d['rots'], CFG16, cols=[d['gcols'][c]], rank=d['grank'])
        assert len(one) == 1
        same_words(o, one[0])
        assert np.max(np.abs(gpu.decrypt(o)[:3] - d['vals'][c][order][t])) < BOUND
    same(outs[0], d['okeysel'][tuple(t)])
    for o, want in zip(outs[1:], d['ocolsel']):
        same(o, want)


def test_equivalent_call_forms(n16):
    d = n16
    gpu, rots, t = d['gpu'], d['rots'], [15, 0, 8]
    want = d['okeysel'][tuple(t)]
    same(gpu.direct_select(d['gkey'], t, N16, rots, CFG16), want)                      # the key form ranks first
    same(gpu.direct_select(d['gkey'], t, N16, rots, CFG16, rank=d['grank']), want)     # cols=None: the key
    same(gpu.direct_select(d['gkey'], t, N16, rots, CFG16, cols=[d['gkey']])[0], want)


CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import fhesort as F
import pyoracle as O
work = sys.argv[3]
N, cfg = 16, (3, 2, 2)
depth, rots = O.size_parameters(N)
orc = O.Context(12, depth, 40, 60, 3, seed=116)
orc.gen_rotation_keys(rots)
gpu = F.Context(12, depth, 40, 60, 3, seed=116, keygen=False)
gpu.load_keys_from(orc, rots)
meta = np.load(work + '/meta.npy')  # (level, scale) of every column, then of the rank
cols = [gpu.upload(np.load(f'{work}/col{p}.npy'), int(meta[p][0]), N, meta[p][1]) for p in range(len(meta) - 1)]
rank = gpu.upload(np.load(work + '/rank.npy'), int(meta[-1][0]), N, meta[-1][1])
with F.KernelClock(gpu) as clk:
    outs = gpu.direct_select(None, list(range(N)), N, rots, cfg, cols=cols, rank=rank)
new = [k for k in clk.stats if k.startswith('k_mul_plain_sum_groups')]
assert not new, new
assert any(k.startswith('k_mul_plain_sum') for k in clk.stats), sorted(clk.stats)
for p, o in enumerate(outs):
    np.save(f'{work}/out{p}.npy', o.data())
print('ALLOK')
'''


def test_plain_form_gives_the_same_words(n16, tmp_path):
    """FHE_SELECT_FUSED=0 (read once per process, so a fresh child): one
    mul_plain_sum per column instead of k_mul_plain_sum_groups.  16 targets, so
    every pick sum has two terms."""
    d = n16
    gpu = d['gpu']
    with F.KernelClock(gpu) as clk:
        here = gpu.direct_select(None, list(range(N16)), N16, d['rots'], CFG16, cols=d['gcols'], rank=d['grank'])
    assert any(k.startswith('k_mul_plain_sum_groups') for k in clk.stats), sorted(clk.stats)
    same(here[0], d['okeysel'][tuple(range(N16))])
    infos = [c.info() for c in d['ocols']] + [d['orank'].info()]
    np.save(tmp_path / 'meta.npy', np.array([[i['level'], i['scale']] for i in infos], dtype=np.float64))
    for p, c in enumerate(d['ocols']):
        np.save(tmp_path / f'col{p}.npy', c.data())
    np.save(tmp_path / 'rank.npy', d['orank'].data())
    env = dict(os.environ, FHE_SELECT_FUSED='0')
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'),
                        os.path.join(REPO, 'oracle'), str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=280)
    assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
    for p, o in enumerate(here):
        assert np.array_equal(np.load(tmp_path / f'out{p}.npy'), o.data()), p


def test_mask_cache_off_gives_the_same_words(n16):
    """with the cache off a select re-encodes its own plaintexts at its start; the
    sort's masks are untouched by it"""
    d = n16
    gpu, rots, t = d['gpu'], d['rots'], list(range(N16))
    want = d['okeysel'][tuple(t)]
    sort_words = gpu.direct_sort(d['gkey'], N16, rots, CFG16, mode=2, rank=d['grank'])
    gpu.set_mask_cache(False)
    try:
        before = gpu.direct_sort(d['gkey'], N16, rots, CFG16, mode=2, rank=d['grank'])
        with F.KernelClock(gpu) as clk:
            a = gpu.direct_select(d['gkey'], t, N16, rots, CFG16, rank=d['grank'])
            b = gpu.direct_select(d['gkey'], t, N16, rots, CFG16, rank=d['grank'])
        after = gpu.direct_sort(d['gkey'], N16, rots, CFG16, mode=2, rank=d['grank'])
    finally:
        gpu.set_mask_cache(True)
    assert clk.stats['k_select_slots']['launches'] == 4, clk.stats.get('k_select_slots')  # two members, twice
    same(a, want)
    same(b, want)
    same_words(before, sort_words)
    same_words(after, sort_words)
    with F.KernelClock(gpu) as clk:
        same(gpu.direct_select(d['gkey'], t, N16, rots, CFG16, rank=d['grank']), want)
    assert 'k_select_slots' not in clk.stats  # cached again


def _raw_call(gpu, key, rank, cols, ncols, targets, ntargets, rots):
    """fhe_direct_select itself: (status, the output handles it left, the message)"""
    r = np.asarray(rots, dtype=np.int32)
    t = np.asarray(targets, dtype=np.int32)
    arr = (C.c_void_p * max(1, len(cols)))(*[None if c is None else c.h for c in cols])
    outs = (C.c_void_p * max(1, len(cols)))(*([0xdead] * max(1, len(cols))))
    rc = F.lib().fhe_direct_select(gpu.h, None if key is None else key.h, None if rank is None else rank.h, arr, ncols,
                                   t.ctypes.data_as(C.POINTER(C.c_int32)), ntargets, N16, F._int(r), len(r), 3, 2, 2,
                                   outs)
    return rc, [outs[i] for i in range(max(ncols, 0))], F.lib().fhe_last_error().decode()


def test_refusals(n16):
    d = n16
    gpu, rots = d['gpu'], d['rots']
    key, col, rank = d['gkey'], d['gcols'][1], d['grank']
    wide = gpu.encrypt(np.zeros(2 * N16), 2 * N16)
    deep = gpu.level_adjust(col, d['depth'])
    ok = [0, 5]
    cases = [
        ('null entry', key, rank, [col, None], 2, ok, 2, F.FHE_EINVAL, 'column 1'),
        ('stack', key, rank, [col, col, gpu.stack([col, col])], 3, ok, 2, F.FHE_EINVAL, 'column 2'),
        ('slots', key, rank, [wide, col], 2, ok, 2, F.FHE_EINVAL, 'column 0'),
        ('slots against the key', key, None, [col, wide], 2, ok, 2, F.FHE_EINVAL, 'column 1'),
        ('no key, no rank', None, None, [col], 1, ok, 2, F.FHE_EINVAL, None),
        ('no targets', key, rank, [col], 1, ok, 0, F.FHE_EINVAL, 'ntargets'),
        ('too many targets', key, rank, [col], 1, [0] * (N16 + 1), N16 + 1, F.FHE_EINVAL, 'ntargets'),
        ('target too large', key, rank, [col], 1, [0, 3, N16, -1], 4, F.FHE_EINVAL, 'target 2'),
        ('negative target', key, rank, [col, col], 2, [0, -1], 2, F.FHE_EINVAL, 'target 1'),
        ('depth', None, rank, [col, deep], 2, ok, 2, F.FHE_EDEPTH, 'column 1'),
    ]
    for what, k, rk, cols, ncols, targets, nt, status, names in cases:
        rc, outs, msg = _raw_call(gpu, k, rk, cols, ncols, targets, nt, rots)
        assert rc == status, (what, rc, msg)
        assert all(o is None for o in outs), what
        if names:
            assert names in msg, (what, msg)


# ------------------------------------------- N = 64: P_ = 16, five members --
N64, CFG64, S64 = 64, (3, 3, 2), 1024


@pytest.fixture(scope='module')
def n64():
    depth, rots = O.size_parameters(N64)
    orc = O.Context(11, depth, 40, 60, 3, seed=7)
    orc.gen_rotation_keys(rots)
    gpu = F.Context(11, depth, 40, 60, 3, seed=7, keygen=False)
    gpu.load_keys_from(orc, rots)
    rng = np.random.default_rng(64)
    key = rng.permutation(N64) / N64
    vals = [key, rng.uniform(-1, 1, N64)]
    okey = orc.encrypt(key, N64)
    ocols = [okey, orc.level_adjust(orc.encrypt(vals[1], N64), 1)]
    orank = orc.direct_sort(okey, N64, rots, CFG64, mode=1)
    targets = list(range(N64 - 1, -1, -1))
    oouts = oracle_select(orc, orank, ocols, targets, N64, S64)
    gcols = [gpu.from_oracle(c) for c in ocols]
    return dict(gpu=gpu, rots=rots, depth=depth, key=key, vals=vals, targets=targets, oouts=oouts, gcols=gcols,
                grank=gpu.from_oracle(orank))


@pytest.mark.parametrize('stack', [32, 3, 1])
def test_five_members_match_oracle_at_every_chunking(n64, stack):
    """64 targets over cap = 15 run five members: one stack, chunks of 3 + 2, one by one"""
    d = n64
    gpu = d['gpu']
    assert F.select_layout(N64, S64, N64)[0] == 5
    gpu.set_sort_stack(stack)
    try:
        outs = gpu.direct_select(None, d['targets'], N64, d['rots'], CFG64, cols=d['gcols'], rank=d['grank'])
    finally:
        gpu.set_sort_stack(32)
    order = np.argsort(d['key'])
    for c, (g, o) in enumerate(zip(outs, d['oouts'])):
        same(g, o)
        assert g.level == d['depth']
        err = np.max(np.abs(gpu.decrypt(g) - d['vals'][c][order][d['targets']]))
        print(f'N=64 column {c}: max error {err:.3e}')
        assert err < BOUND
