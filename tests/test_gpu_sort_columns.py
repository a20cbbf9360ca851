"""Records sorted by an encrypted key (fhe_direct_sort_columns): the payload
columns are permuted by the key's rank with the index series evaluated once.

Every output is held word for word to the CPU oracle's
direct_sort(col, mode=2, rank=rank) -- rotationIndexCheckN(rank, col), one
column at a time -- and the two kernels under it (k_tensor_cols,
k_sum_member_groups) to the oracle's products and sums.  Oracle results are
computed once per module and shared.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fhesort as F
import pyoracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


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


# ------------------------------------------------------------ kernel level --
@pytest.fixture(scope='module')
def small():
    """ring 2^12, L = 3, 40-bit scaling: q0 of 60 bits beside 40-bit limbs, so a
    product at level 1 runs both prime classes"""
    orc = O.Context(12, 3, 40, 60, 3, seed=41)
    orc.gen_rotation_keys([1])
    gpu = F.Context(12, 3, 40, 60, 3, seed=41, keygen=False)
    gpu.load_keys_from(orc, [1])
    rng = np.random.default_rng(11)
    xs = [orc.encrypt(rng.uniform(-1, 1, 16), 16, 1) for _ in range(3)]
    pc = F.TENSOR_COLS_PER_THREAD
    cols = [orc.encrypt(rng.uniform(-1, 1, 16), 16, 1) for _ in range(max(5, pc + 1))]
    cols[0] = orc.encrypt(rng.uniform(-1, 1, 16), 16, 0)                        # mul_columns adjusts it
    cols[1] = orc.level_adjust(orc.encrypt(rng.uniform(-1, 1, 16), 16, 0), 1)   # adjusted beforehand
    prods = [[orc.mul(x, c) for x in xs] for c in cols]                          # [p][z]
    return orc, gpu, xs, cols, prods


@pytest.mark.parametrize('P', sorted({1, 2, max(5, F.TENSOR_COLS_PER_THREAD + 1)}))
def test_mul_columns_and_group_sums_match_oracle(small, P):
    """Member p B + z of mul_columns is the oracle's mul(x_z, col_p); the largest
    P crosses a guarded column-group tail of k_tensor_cols.  Member p of
    sum_member_groups is the oracle's sum of group p."""
    orc, gpu, xs, cols, prods = small
    B = len(xs)
    S = gpu.stack([gpu.from_oracle(x) for x in xs])
    with F.KernelClock(gpu) as clk:
        R = gpu.mul_columns(S, [gpu.from_oracle(c) for c in cols[:P]])
        G = gpu.sum_member_groups(R, P)
    assert any(k.startswith('k_tensor_cols') for k in clk.stats), sorted(clk.stats)
    assert any(k.startswith('k_sum_member_groups') for k in clk.stats), sorted(clk.stats)
    for p in range(P):
        for z in range(B):
            same(gpu.member(R, p * B + z), prods[p][z])
        want = prods[p][0]
        for z in range(1, B):
            want = orc.add(want, prods[p][z])
        same(gpu.member(G, p), want)


def test_mul_columns_refuses_bad_columns(small):
    orc, gpu, xs, cols, _ = small
    S = gpu.stack([gpu.from_oracle(x) for x in xs])
    deep = gpu.level_adjust(gpu.from_oracle(cols[2]), 2)
    for bad in ([], [S], [deep]):
        with pytest.raises(F.FheError) as e:
            gpu.mul_columns(S, bad)
        assert e.value.code == F.FHE_EINVAL
    with pytest.raises(F.FheError) as e:
        gpu.sum_member_groups(S, 2)  # 3 members are not two groups
    assert e.value.code == F.FHE_EINVAL


# ------------------------------------------------------- N = 16, one batch --
N16, CFG16 = 16, (3, 2, 2)


@pytest.fixture(scope='module')
def one_batch():
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
    oouts = [orc.direct_sort(c, N16, rots, CFG16, mode=2, rank=orank) for c in ocols]
    gkey = gpu.from_oracle(okey)
    gcols = [gkey] + [gpu.from_oracle(c) for c in ocols[1:]]
    gouts = gpu.direct_sort_columns(gkey, gcols, N16, rots, CFG16)
    return dict(orc=orc, gpu=gpu, depth=depth, rots=rots, key=key, vals=vals, okey=okey, ocols=ocols, orank=orank,
                oouts=oouts, gkey=gkey, gcols=gcols, gouts=gouts)


def test_one_batch_columns_match_oracle_and_plaintext(one_batch):
    d = one_batch
    order = np.argsort(d['key'])
    for p, (g, o) in enumerate(zip(d['gouts'], d['oouts'])):
        same(g, o)
        err = np.max(np.abs(d['gpu'].decrypt(g)[:N16] - d['vals'][p][order]))
        assert err < 0.01, (p, err)  # the reference's DirectSortTest bound; |col| <= 1
        assert g.level == d['depth']


def test_equivalent_call_forms(one_batch):
    d = one_batch
    gpu, rots = d['gpu'], d['rots']
    grank = gpu.direct_sort(d['gkey'], N16, rots, CFG16, mode=1)
    same(grank, d['orank'])
    with_rank = gpu.direct_sort_columns(None, d['gcols'], N16, rots, CFG16, rank=grank)
    for a, b in zip(with_rank, d['gouts']):
        same_words(a, b)
    for p in (1, 2):  # P = 1 is the GPU's own index check
        one = gpu.direct_sort_columns(None, [d['gcols'][p]], N16, rots, CFG16, rank=grank)
        assert len(one) == 1
        same_words(one[0], gpu.direct_sort(d['gcols'][p], N16, rots, CFG16, mode=2, rank=grank))
    same_words(d['gouts'][0], gpu.direct_sort(d['gkey'], N16, rots, CFG16))  # the key among cols: the sort


def test_kernel_names(one_batch):
    d = one_batch
    gpu = d['gpu']
    grank = gpu.from_oracle(d['orank'])
    with F.KernelClock(gpu) as clk:
        outs = gpu.direct_sort_columns(None, d['gcols'], N16, d['rots'], CFG16, rank=grank)
    for a, b in zip(outs, d['gouts']):
        same_words(a, b)
    assert any(k.startswith('k_tensor_cols') for k in clk.stats), sorted(clk.stats)
    assert any(k.startswith('k_sum_member_groups') for k in clk.stats), sorted(clk.stats)


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
    outs = gpu.direct_sort_columns(None, cols, N, rots, cfg, rank=rank)
    S = gpu.stack([cols[0], cols[1]])
    R = gpu.mul_columns(S, [cols[1], cols[0], cols[1]])
    G = gpu.sum_member_groups(R, 3)
new = [k for k in clk.stats if k.startswith(('k_tensor_cols', 'k_sum_member_groups'))]
assert not new, new
assert any(k.startswith('k_tensor') for k in clk.stats), sorted(clk.stats)
for p, o in enumerate(outs):
    np.save(f'{work}/out{p}.npy', o.data())
for m in range(6):
    np.save(f'{work}/prod{m}.npy', gpu.member(R, m).data())
for p in range(3):
    np.save(f'{work}/sum{p}.npy', gpu.member(G, p).data())
print('ALLOK')
'''


def test_plain_form_gives_the_same_words(one_batch, tmp_path):
    """FHE_SORT_COLS_FUSED=0 (read once per process, so a fresh child): P
    broadcast products and per-group sums instead of the two kernels."""
    d = one_batch
    orc = d['orc']
    infos = [c.info() for c in d['ocols']] + [d['orank'].info()]
    np.save(tmp_path / 'meta.npy', np.array([[i['level'], i['scale']] for i in infos], dtype=np.float64))
    for p, c in enumerate(d['ocols']):
        np.save(tmp_path / f'col{p}.npy', c.data())
    np.save(tmp_path / 'rank.npy', d['orank'].data())
    env = dict(os.environ, FHE_SORT_COLS_FUSED='0')
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'),
                        os.path.join(REPO, 'oracle'), str(tmp_path)], env=env, capture_output=True, text=True,
                       timeout=280)
    assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
    for p, o in enumerate(d['oouts']):
        assert np.array_equal(np.load(tmp_path / f'out{p}.npy'), o.data()), p
    a, b = d['ocols'][0], d['ocols'][1]
    prods = [orc.mul(x, c) for c in (b, a, b) for x in (a, b)]
    for m, o in enumerate(prods):
        assert np.array_equal(np.load(tmp_path / f'prod{m}.npy'), o.data()), m
    for p in range(3):
        assert np.array_equal(np.load(tmp_path / f'sum{p}.npy'), orc.add(prods[2 * p], prods[2 * p + 1]).data()), p


def _raw_call(gpu, key, rank, cols, ncols, rots):
    """fhe_direct_sort_columns itself: (status, the output handles it left)"""
    r = np.asarray(rots, dtype=np.int32)
    arr = (C.c_void_p * max(1, len(cols)))(*[None if c is None else c.h for c in cols])
    outs = (C.c_void_p * max(1, len(cols)))()
    rc = F.lib().fhe_direct_sort_columns(gpu.h, None if key is None else key.h, None if rank is None else rank.h,
                                         arr, ncols, N16, F._int(r), len(r), 3, 2, 2, 0,
                                         1, None, None, outs)
    return rc, [outs[i] for i in range(len(outs))], F.lib().fhe_last_error().decode()


def test_refusals(one_batch):
    d = one_batch
    gpu, rots = d['gpu'], d['rots']
    key, col = d['gkey'], d['gcols'][1]
    rank = gpu.from_oracle(d['orank'])
    wide = gpu.encrypt(np.zeros(2 * N16), 2 * N16)
    deep = gpu.level_adjust(col, d['depth'])
    cases = [
        ('no columns', key, rank, [col], 0, F.FHE_EINVAL, None),
        ('null entry', key, rank, [col, None], 2, F.FHE_EINVAL, 'column 1'),
        ('stack', key, rank, [col, col, gpu.stack([col, col])], 3, F.FHE_EINVAL, 'column 2'),
        ('slots', key, rank, [wide, col], 2, F.FHE_EINVAL, 'column 0'),
        ('slots against the key', key, None, [col, wide], 2, F.FHE_EINVAL, 'column 1'),
        ('no key, no rank', None, None, [col], 1, F.FHE_EINVAL, None),
        ('depth', None, rank, [col, deep], 2, F.FHE_EDEPTH, 'column 1'),
    ]
    for what, k, rk, cols, ncols, status, names in cases:
        rc, outs, msg = _raw_call(gpu, k, rk, cols, ncols, rots)
        assert rc == status, (what, rc, msg)
        assert all(o is None for o in outs), what
        if names:
            assert names in msg, (what, msg)


# ---------------------------------------------------- N = 64, four batches --
N64, CFG64, P64 = 64, (3, 3, 2), 5


@pytest.fixture(scope='module')
def four_batches():
    depth, rots = O.size_parameters(N64)
    orc = O.Context(11, depth, 40, 60, 3, seed=7)
    orc.gen_rotation_keys(rots)
    gpu = F.Context(11, depth, 40, 60, 3, seed=7, keygen=False)
    gpu.load_keys_from(orc, rots)
    rng = np.random.default_rng(64)
    key = rng.permutation(N64) / N64
    okey = orc.encrypt(key, N64)
    ocols = [okey] + [orc.encrypt(rng.uniform(-1, 1, N64), N64) for _ in range(P64 - 1)]
    ocols[3] = orc.level_adjust(ocols[3], 1)
    orank = orc.direct_sort(okey, N64, rots, CFG64, mode=1)
    oouts = [orc.direct_sort(c, N64, rots, CFG64, mode=2, rank=orank) for c in ocols]
    gkey = gpu.from_oracle(okey)
    gcols = [gkey] + [gpu.from_oracle(c) for c in ocols[1:]]
    return dict(orc=orc, gpu=gpu, rots=rots, orank=orank, oouts=oouts, gkey=gkey, gcols=gcols)


def _settings(gpu, stack, lanes, bound):
    gpu.set_sort_stack(stack)
    gpu.set_sort_lanes(lanes)
    gpu.set_sort_column_members(F.SORT_COLUMN_MEMBERS_DEFAULT if bound is None else bound)


# (32, 2, 4): two lanes of two stacked batches each, so a bound of 4 members runs the columns as 2 + 2 + 1
@pytest.mark.parametrize('stack,lanes,bound', [(32, 1, None), (3, 2, None), (32, 2, 4), (1, 3, None)])
def test_multi_batch_columns_match_oracle(four_batches, stack, lanes, bound):
    d = four_batches
    gpu = d['gpu']
    _settings(gpu, stack, lanes, bound)
    try:
        outs = gpu.direct_sort_columns(d['gkey'], d['gcols'], N64, d['rots'], CFG64)
    finally:
        _settings(gpu, 32, 2, None)
    assert len(outs) == P64
    for g, o in zip(outs, d['oouts']):
        same(g, o)


class _Hip:
    def __init__(self):
        self.h = C.CDLL('libamdhip64.so')
        self.h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def get(self, ptr, count):
        buf = np.empty(count, dtype=np.uint64)
        assert self.h.hipMemcpy(buf.ctypes.data, C.cast(ptr, C.c_void_p), count * 8, 2) == 0
        return buf

    def put(self, ptr, buf):
        assert self.h.hipMemcpy(C.cast(ptr, C.c_void_p), buf.ctypes.data, buf.size * 8, 1) == 0


def test_sharded_columns_match_unsharded(four_batches):
    """Two ranks in one process.  Pass 1: each rank runs with a hook that only
    records its all-reduce buffers (the header, then the column stack's words).
    Pass 2: each rank runs again, its hook writing the wrapped u64 sum of both
    ranks' recorded buffers.  Both ranks then hold the unsharded outputs."""
    d = four_batches
    gpu, rots = d['gpu'], d['rots']
    hip = _Hip()
    grank = gpu.from_oracle(d['orank'])
    cols = d['gcols']

    def run(**kw):
        return gpu.direct_sort_columns(None, cols, N64, rots, CFG64, rank=grank, **kw)

    ref = run()
    for g, o in zip(ref, d['oouts']):
        same(g, o)
    seen = {0: [], 1: []}
    for r in (0, 1):
        run(shard=(r, 2), allreduce=lambda ptr, count, _u, r=r: seen[r].append(hip.get(ptr, count)))
    assert [len(b) for b in seen[0]] == [len(b) for b in seen[1]]
    assert len(seen[0]) == 2 and len(seen[0][0]) == 4  # one header, one exchange for all columns
    n_words = seen[0][1].size
    assert n_words == P64 * ref[0].data().size
    outs = {}
    for r in (0, 1):
        calls = iter(range(len(seen[0])))

        def hook(ptr, count, _u):
            i = next(calls)
            assert count == seen[0][i].size
            hip.put(ptr, seen[0][i] + seen[1][i])  # u64 wrap-around add

        outs[r] = run(shard=(r, 2), allreduce=hook)
    for a, b, c in zip(outs[0], outs[1], ref):
        same_words(a, b)
        same_words(a, c)
    for a, c in zip(run(shard=(0, 1), allreduce=lambda ptr, count, _u: None), ref):
        same_words(a, c)
