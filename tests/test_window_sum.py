"""CPU checks of the window sums (fhe_direct_window_sum): the
definition against independent numpy computations, the plaintext model on the
exact composite sign against the definition at every size, with one partition
against the running sums, its ROWS count against the per-partition stable rank,
the levels function against the model's levels and the oracle composition's, the
CPU-oracle composition against the exact sums in every mode and for 2, 3 and 4
factors, the new entry points declared, exported and bound, and the argument
refusals that need no device.  No GPU work."""
import ctypes as C
import re

import numpy as np
import pytest

import fhesort as F
import pyoracle as O
import running_model as R
import stable_model as S
import window_model as W

NEW = ('fhe_direct_window_sum', 'fhe_window_sum_levels', 'fhe_sub_window_stacked', 'fhe_mul_sub_sub')
# The group sums' and running sums' bound (tests/test_group_sum.py): the model is a
# fixed polynomial, so its error is the distance of the composite sign from +-1 at
# +-eps and beyond, summed over the N pairs of a row; a product of up to four such
# indicators, each within [0, 1], is at most four times as far off.  Measured here:
# <= 7.2e-7 at N = 8, 64 and 1024.
MODEL_BOUND = 2e-4
# (G, mode) of every combination the operator serves, by factor count
COMBOS = [(G, m) for G in (1, 2, 3) for m in W.MODES if 2 <= W.nfactors(G, m) <= 4]
COMBO_IDS = [f'G{G}-{W.MODE_IDS[m]}' for G, m in COMBOS]
# N = 1024 costs a second per sign of its 2^20 pairs: there, every mode and every factor count once
LARGE = [(1, W.ROWS), (1, W.BETWEEN), (2, W.LE), (2, W.GROUP), (2, W.LT), (3, W.ROWS)]
SIZED = [(N, G, m) for N in (8, 64, 1024) for G, m in COMBOS if N < 1024 or (G, m) in LARGE]
SIZED_IDS = [f'{N}-G{G}-{W.MODE_IDS[m]}' for N, G, m in SIZED]


def test_header_and_binding_declare_the_window_sum():
    text = open(F.HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = set(re.findall(r'\b(fhe_[a-z0-9_]+)\s*\(', src))
    for f in NEW:
        assert f in names, f
        assert f in F._SIGS, f
        assert getattr(F.lib(), f, None) is not None, f  # exported by the built library
    for m in ('window_sum', 'window_sum_levels', 'sub_window_stacked', 'mul_sub_sub'):
        assert callable(getattr(F.Context, m, None)), m
    for i, name in enumerate(('ROWS', 'LE', 'LT', 'BETWEEN', 'GROUP')):
        assert getattr(F, 'WIN_' + name) == getattr(W, name) == i
        assert re.search(r'#define\s+FHE_WIN_%s\s+%d\b' % (name, i), src), name
    for name in ('ROWS', 'LE', 'LT', 'BETWEEN'):
        assert getattr(F, 'WIN_' + name) == getattr(F, 'RUN_' + name)


def _order(mode, t, lo, hi):
    """(order_left, order_right, lo) of the self join for the mode"""
    if mode == W.GROUP:
        return None, None, None
    return (hi, t, lo) if mode == W.BETWEEN else (t, t, None)


def _columns(N):
    rng = np.random.default_rng(N)
    return [rng.uniform(-1, 1, N) for _ in range(3)]


def _independent(parts, t, lo, hi, cols, mode):
    """the sums and counts row by row, partition by partition, without any pair matrix"""
    N = len(t)
    sums, cnt = np.zeros((len(cols), N)), np.zeros(N)
    if mode == W.GROUP:  # a dict keyed by the key tuple
        tot = {}
        for j in range(N):
            key = tuple(p[j] for p in parts)
            s, c = tot.get(key, (np.zeros(len(cols)), 0))
            tot[key] = (s + np.array([v[j] for v in cols]), c + 1)
        for e in range(N):
            s, c = tot[tuple(p[e] for p in parts)]
            sums[:, e], cnt[e] = s, c
        return sums, cnt
    pid = W.partition_ids(parts)
    for g in np.unique(pid):
        rows = np.flatnonzero(pid == g)
        tg = t[rows]
        order = np.argsort(tg, kind='stable')
        ts = tg[order]
        csum = [np.concatenate([[0.0], np.cumsum(v[rows][order])]) for v in cols]
        if mode == W.ROWS:  # the cumulative sum in stable order, own row included
            k = np.empty(len(rows), dtype=int)
            k[order] = np.arange(1, len(rows) + 1)
            first = np.zeros(len(rows), dtype=int)
        elif mode in (W.LE, W.LT):
            k = np.searchsorted(ts, tg, side='right' if mode == W.LE else 'left')
            first = np.zeros(len(rows), dtype=int)
        else:  # the closed window, computed directly
            for i, e in enumerate(rows):
                inside = rows[(tg >= lo[e] - 1e-12) & (tg <= hi[e] + 1e-12)]
                cnt[e] = len(inside)
                for p, v in enumerate(cols):
                    sums[p, e] = v[inside].sum()
            continue
        cnt[rows] = k - first
        for p in range(len(cols)):
            sums[p, rows] = csum[p][k] - csum[p][first]
    return sums, cnt


@pytest.mark.parametrize('G,mode', COMBOS, ids=COMBO_IDS)
@pytest.mark.parametrize('N', [8, 64, 1024])
def test_exact_is_the_sql_window(N, G, mode):
    parts, t, lo, hi, eps, _ = W.partitioned_input(N, G)
    cols = _columns(N)
    ol, orr, l = _order(mode, t, lo, hi)
    sums, cnt = W.exact(parts, parts, cols, mode, eps, ol, orr, l)
    wsums, wcnt = _independent(parts, t, lo, hi, cols, mode)
    assert np.array_equal(cnt, wcnt) and np.allclose(sums, wsums, atol=1e-12)


def test_exact_is_the_join_on_two_keys():
    for N in (8, 64):
        pl, pr, eps, _ = W.two_tables(N)
        v = np.random.default_rng(N).uniform(-1, 1, N)
        sums, cnt = W.exact(pl, pr, [v], W.GROUP, eps)
        for e in range(N):
            rows = [j for j in range(N) if pl[0][e] == pr[0][j] and pl[1][e] == pr[1][j]]
            assert cnt[e] == len(rows) and abs(sums[0][e] - v[rows].sum()) < 1e-12


@pytest.mark.parametrize('noise', [0.0, 1e-5], ids=['exact', 'noise1e-5'])
@pytest.mark.parametrize('N,G,mode', SIZED, ids=SIZED_IDS)
def test_model_gives_the_window_sums_and_counts(N, G, mode, noise):
    parts, t, lo, hi, eps, cfg = W.partitioned_input(N, G)
    cols = _columns(N)
    ol, orr, l = _order(mode, t, lo, hi)
    nz = np.random.default_rng(N + 1).uniform(-noise, noise, (N, N)) if noise else None
    sums, cnt = W.window_sums(parts, parts, cols, cfg, mode, eps, ol, orr, l, nz)
    wsums, wcnt = W.exact(parts, parts, cols, mode, eps, ol, orr, l)
    es, ec = np.max(np.abs(sums - wsums)), np.max(np.abs(cnt - wcnt))
    print(f'N={N} G={G} mode={W.MODE_IDS[mode]} noise={noise}: sum error {es:.3e}, count error {ec:.3e}')
    assert es < MODEL_BOUND and ec < MODEL_BOUND


@pytest.mark.parametrize('N,mode', [(N, m) for N in (8, 64, 1024) for m in R.MODES if N < 1024 or m == R.ROWS],
                         ids=lambda x: str(x))
def test_one_constant_partition_key_gives_the_running_sums(N, mode):
    _, t, lo, hi, eps, cfg = W.partitioned_input(N, 1)
    cols = _columns(N)
    const = [np.full(N, 2.0 / N)]
    ol, orr, l = _order(mode, t, lo, hi)
    sums, cnt = W.window_sums(const, const, cols, cfg, mode, eps, ol, orr, l)
    rsums, rcnt = R.running_sums(ol, orr, cols, cfg, mode, eps, l)
    assert np.max(np.abs(sums - rsums)) < MODEL_BOUND and np.max(np.abs(cnt - rcnt)) < MODEL_BOUND


@pytest.mark.parametrize('N,G', [(N, G) for N in (8, 64, 1024) for G in (1, 2, 3) if N < 1024 or G == 1],
                         ids=lambda x: str(x))
def test_rows_count_is_the_stable_rank_inside_the_partition(N, G):
    parts, t, _, _, eps, cfg = W.partitioned_input(N, G)
    cnt = W.window_sums(parts, parts, [], cfg, W.ROWS, eps, t, t)[1]
    pid = W.partition_ids(parts)
    want = np.empty(N)
    for g in np.unique(pid):
        rows = np.flatnonzero(pid == g)
        want[rows] = S.stable_ranks(t[rows])
    assert np.max(np.abs(cnt - 1.0 - want)) < MODEL_BOUND


def test_levels_function_is_the_models():
    for cfg in ((3, 2, 2), (3, 3, 2), (3, 5, 2)):
        for key_level in (0, 1, 3):
            for Fn in (2, 3, 4):
                _, _, La, col_max, out = W.levels(key_level, Fn, cfg)
                assert F.window_sum_levels(key_level, Fn, cfg) == (col_max, out) == (La - 2, La + 1)
            # two factors sit one product above the group sums
            assert F.window_sum_levels(key_level, 2, cfg)[1] == F.group_sum_levels(key_level, cfg)[1] + 1
    for Fn in (1, 5):
        with pytest.raises(F.FheError) as e:
            F.window_sum_levels(0, Fn, (3, 2, 2))
        assert e.value.code == F.FHE_EINVAL


@pytest.fixture(scope='module')
def small_oracle():
    depth, rots = O.size_parameters(8)
    depth = max(depth, F.window_sum_levels(0, 4, S.sign_cfg(8))[1])
    orc = O.Context(12, depth, 40, 60, 3, seed=5)
    orc.gen_rotation_keys(rots)
    return orc, rots


@pytest.mark.parametrize('G,mode', COMBOS, ids=COMBO_IDS)
def test_oracle_composition_gives_the_exact_sums_at_the_levels(small_oracle, G, mode):
    orc, rots = small_oracle
    N = 8
    parts, t, lo, hi, eps, cfg = W.partitioned_input(N, G)
    Fn = W.nfactors(G, mode)
    col_max, out = F.window_sum_levels(0, Fn, cfg)
    v = np.arange(N) / N
    ol, orr, l = _order(mode, t, lo, hi)
    enc = lambda x: None if x is None else orc.encrypt(x, N)
    oparts = [enc(p) for p in parts]
    outs, cnt = W.oracle_window_sums(orc, oparts, oparts, [orc.encrypt(v, N, col_max)], N, rots, cfg, eps, mode, True,
                                     enc(ol), enc(orr), enc(l))
    assert outs[0].level == cnt.level == out
    assert outs[0].slots == cnt.slots == N
    wsums, wcnt = W.exact(parts, parts, [v], mode, eps, ol, orr, l)
    err = max(np.max(np.abs(outs[0].decrypt() - wsums[0])), np.max(np.abs(cnt.decrypt() - wcnt)))
    print(f'N={N} G={G} mode={W.MODE_IDS[mode]}: oracle composition error {err:.3e}')
    assert err < 1e-3


def test_entry_points_refuse_null_handles():
    out, cnt = (C.c_void_p * 2)(1, 1), C.c_void_p(1)
    rc = F.lib().fhe_direct_window_sum(None, None, None, 1, None, None, None, None, 2, 0, 0.1, 8, None, 0, 3, 2, 2, out,
                                       C.byref(cnt))
    assert rc == F.FHE_EINVAL
    assert out[0] is None and out[1] is None and cnt.value is None  # no output handle is set
    o = C.c_void_p()
    assert F.lib().fhe_sub_window_stacked(None, None, 1, None, 1, 4, None, None, None, None, 0.1, C.byref(o)) == F.FHE_EINVAL
    assert F.lib().fhe_mul_sub_sub(None, None, None, None, None, C.byref(o)) == F.FHE_EINVAL
