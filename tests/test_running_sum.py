"""CPU checks of the running sums (fhe_direct_running_sum): the
plaintext model on the exact composite sign gives the running sums and counts in
every mode and at every size, its ROWS count is the stable rank + 1, the CPU-oracle
composition ends at fhe_group_sum_levels' output level and decrypts to the exact
sums, the new entry points are declared, exported and bound, and the argument
refusals that need no device.  No GPU work."""
import ctypes as C
import re

import numpy as np
import pytest

import fhesort as F
import group_model as G
import pyoracle as O
import running_model as R
import stable_model as S

NEW = ('fhe_direct_running_sum', 'fhe_sub_bounds_stacked', 'fhe_mul_pairs_const', 'fhe_mul_pairs_sub')
# The group sums' bound (tests/test_group_sum.py): the model is a fixed polynomial,
# so its error is the distance of the composite sign from +-1 at +-eps and beyond,
# summed over the N pairs of a row.  Worst at N = 128, the largest size (3, 3, 2)
# serves: 7.4e-5 there on these columns, at most 2.5e-6 elsewhere.  2e-4 bounds that
# worst case with room for another draw and the noise on the sign arguments.
MODEL_BOUND = 2e-4


def test_header_and_binding_declare_the_running_sum():
    text = open(F.HEADER).read()
    src = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    names = set(re.findall(r'\b(fhe_[a-z0-9_]+)\s*\(', src))
    for f in NEW:
        assert f in names, f
        assert f in F._SIGS, f
        assert getattr(F.lib(), f, None) is not None, f  # exported by the built library
    for m in ('running_sum', 'sub_bounds_stacked', 'mul_pairs_const', 'mul_pairs_sub'):
        assert callable(getattr(F.Context, m, None)), m
    for i, name in enumerate(('ROWS', 'LE', 'LT', 'BETWEEN')):
        assert getattr(F, 'RUN_' + name) == getattr(R, name) == i
        assert re.search(r'#define\s+FHE_RUN_%s\s+%d\b' % (name, i), src), name


def _inputs(N, mode):
    """(kl, kr, lo, eps, cfg): the self join on tied keys, the window for BETWEEN"""
    if mode == R.BETWEEN:
        k, lo, hi, eps, cfg = R.window_input(N)
        return hi, k, lo, eps, cfg
    k = S.tied_input(N, S.SEEDS[N])
    return k, k, None, 1.0 / N, S.sign_cfg(N)


@pytest.mark.parametrize('noise', [0.0, 1e-5], ids=['exact', 'noise1e-5'])
@pytest.mark.parametrize('mode', R.MODES, ids=R.MODE_IDS)
@pytest.mark.parametrize('N', [8, 64, 128, 1024])
def test_model_gives_the_running_sums_and_counts(N, mode, noise):
    kl, kr, lo, eps, cfg = _inputs(N, mode)
    rng = np.random.default_rng(N)
    cols = [rng.uniform(-1, 1, N), np.arange(N) / N]
    nz = rng.uniform(-noise, noise, (N, N)) if noise else None
    sums, cnt = R.running_sums(kl, kr, cols, cfg, mode, eps, lo, nz)
    wsums, wcnt = R.exact(kl, kr, cols, mode, eps, lo)
    for a in R.sign_arguments(kl, kr, mode, eps, lo):
        assert np.max(np.abs(a)) <= 1.0 and np.min(np.abs(a)) >= eps * (1 - 1e-9)
    assert wcnt.min() < N and wcnt.max() >= 3  # no mode degenerates to the plain sum
    es, ec = np.max(np.abs(sums - wsums)), np.max(np.abs(cnt - wcnt))
    print(f'N={N} mode={R.MODE_IDS[mode]} noise={noise}: sum error {es:.3e}, count error {ec:.3e}')
    assert es < MODEL_BOUND and ec < MODEL_BOUND


@pytest.mark.parametrize('N', [8, 64, 128, 1024])
def test_exact_is_the_sql_window_and_searchsorted(N):
    """the definition against numpy: cumulative sums in stable order, searchsorted, the closed window"""
    k = S.tied_input(N, S.SEEDS[N])
    v = np.random.default_rng(N + 3).uniform(-1, 1, N)
    eps = 1.0 / N
    order = np.argsort(k, kind='stable')
    want = np.empty(N)
    want[order] = np.cumsum(v[order])
    sums, cnt = R.exact(k, k, [v], R.ROWS, eps)
    assert np.allclose(sums[0], want, atol=1e-12) and np.array_equal(cnt - 1, S.stable_ranks(k))
    ks = np.sort(k)
    assert np.array_equal(R.exact(k, k, [], R.LE, eps)[1], np.searchsorted(ks, k, side='right'))
    assert np.array_equal(R.exact(k, k, [], R.LT, eps)[1], np.searchsorted(ks, k, side='left'))
    kw, lo, hi, weps, _ = R.window_input(N)
    wsum, wcnt = R.exact(hi, kw, [v], R.BETWEEN, weps, lo)
    inside = (kw[None, :] >= lo[:, None] - 1e-12) & (kw[None, :] <= hi[:, None] + 1e-12)
    assert np.array_equal(wcnt, inside.sum(axis=1)) and np.allclose(wsum[0], inside @ v, atol=1e-12)


@pytest.mark.parametrize('N', [8, 64])
def test_model_gives_the_range_lookup(N):
    """two tables: SUM(b.v) WHERE b.k <= a.k and searchsorted of one table's keys in the other's"""
    kl, kr, eps, cfg = G.lookup_tables(N, 7 * N)
    v = np.random.default_rng(N + 1).uniform(-1, 1, N)
    for mode, side in ((R.LE, 'right'), (R.LT, 'left')):
        sums, cnt = R.running_sums(kl, kr, [v], cfg, mode, eps)
        wsums, wcnt = R.exact(kl, kr, [v], mode, eps)
        assert np.array_equal(wcnt, np.searchsorted(np.sort(kr), kl, side=side))
        assert np.max(np.abs(sums - wsums)) < MODEL_BOUND and np.max(np.abs(cnt - wcnt)) < MODEL_BOUND
    assert (R.exact(kl, kr, [], R.LE, eps)[1] != R.exact(kl, kr, [], R.LT, eps)[1]).any()  # a left key is present


@pytest.mark.parametrize('N', [8, 64, 128, 1024])
def test_rows_count_is_the_stable_rank_plus_one(N):
    k = S.tied_input(N, S.SEEDS[N])
    cfg, eps = S.sign_cfg(N), 1.0 / N
    cnt = R.running_sums(k, k, [], cfg, R.ROWS, eps)[1]
    assert np.max(np.abs(cnt - 1.0 - S.ranks(k, cfg, eps))) < 1e-9


@pytest.fixture(scope='module')
def small_oracle():
    depth, rots = O.size_parameters(8)
    orc = O.Context(12, depth, 40, 60, 3, seed=5)
    orc.gen_rotation_keys(rots)
    return orc, rots


# Largest |decrypted - exact| of the oracle composition at N = 8 per mode, recorded
# by the test below for the GPU tests' ORACLE_ERR (tests/test_gpu_running_sum.py
# measures its own inputs the same way).
COMPOSITION_ERR = {}


@pytest.mark.parametrize('mode', R.MODES, ids=R.MODE_IDS)
def test_oracle_composition_ends_at_the_group_sum_levels(small_oracle, mode):
    orc, rots = small_oracle
    N = 8
    kl, kr, lo, eps, cfg = _inputs(N, mode)
    col_max, out = F.group_sum_levels(0, cfg)
    v = np.arange(N) / N
    okl = orc.encrypt(kl, N)
    okr = okl if kr is kl else orc.encrypt(kr, N)
    olo = orc.encrypt(lo, N) if lo is not None else None
    outs, cnt = R.oracle_running_sums(orc, okl, okr, [orc.encrypt(v, N, col_max)], N, rots, cfg, eps, mode, True, olo)
    assert outs[0].level == cnt.level == out
    assert outs[0].slots == cnt.slots == N
    wsums, wcnt = R.exact(kl, kr, [v], mode, eps, lo)
    err = max(np.max(np.abs(outs[0].decrypt() - wsums[0])), np.max(np.abs(cnt.decrypt() - wcnt)))
    COMPOSITION_ERR[mode] = err
    print(f'N={N} mode={R.MODE_IDS[mode]}: oracle composition error {err:.3e}')
    assert err < 1e-3
    if mode == R.ROWS:  # ... and the count is the tie-broken rank + 1, word for word
        rank = S.oracle_rank(orc, okl, N, rots, cfg, eps)
        assert np.array_equal(orc.add_const(cnt, -1.0).data(), rank.data())
        assert rank.level == out


def test_entry_points_refuse_null_handles():
    out, cnt = (C.c_void_p * 2)(1, 1), C.c_void_p(1)
    rc = F.lib().fhe_direct_running_sum(None, None, None, None, None, 2, 0, 0.1, 8, None, 0, 3, 2, 2, out,
                                        C.byref(cnt))
    assert rc == F.FHE_EINVAL
    assert out[0] is None and out[1] is None and cnt.value is None  # no output handle is set
    o = C.c_void_p()
    assert F.lib().fhe_sub_bounds_stacked(None, None, 1, None, 1, None, C.byref(o)) == F.FHE_EINVAL
    assert F.lib().fhe_mul_pairs_const(None, None, 1.0, None, 1, C.byref(o)) == F.FHE_EINVAL
    assert F.lib().fhe_mul_pairs_sub(None, None, None, None, 1, C.byref(o)) == F.FHE_EINVAL
