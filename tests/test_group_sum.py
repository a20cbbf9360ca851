"""CPU checks of the group sums and lookups (fhe_direct_group_sum; DESIGN.md
§6.4): the plaintext model on the exact composite sign gives the group sums and
counts at every size, the pure host level function agrees with what the CPU
oracle does, the new entry points are declared, exported and bound, and the
argument refusals that need no device.  No GPU work."""
import ctypes as C
import re

import numpy as np
import pytest

import fhesort as F
import group_model as G
import pyoracle as O
import stable_model as S

NEW = ('fhe_direct_group_sum', 'fhe_group_sum_levels', 'fhe_sub_pm_const_stacked', 'fhe_mul_pairs')
# The model is a fixed polynomial, so its error is a property of the sign
# configuration, not of an implementation: per pair the distance of the composite
# sign from +-1 at +-eps (tied pairs) and beyond (the others), summed over the N
# pairs of a row.  The worst size is N = 128, the largest its (3, 3, 2) serves
# (smallest difference 1 / 128): 6.5e-5 to 7.4e-5 there depending on the draw, at most 7e-7 elsewhere.  2e-4
# bounds that worst case with room for the noise on the differences.
MODEL_BOUND = 2e-4


def test_header_and_binding_declare_the_group_sum():
    src = re.sub(r'/\*.*?\*/', '', open(F.HEADER).read(), flags=re.S)
    names = set(re.findall(r'\b(fhe_[a-z0-9_]+)\s*\(', src))
    for f in NEW:
        assert f in names, f
        assert f in F._SIGS, f
        assert getattr(F.lib(), f, None) is not None, f  # exported by the built library
    for m in ('group_sum', 'sub_pm_const_stacked', 'mul_pairs', 'group_sum_levels'):
        assert callable(getattr(F.Context, m, None)), m
    assert callable(F.group_sum_levels)


@pytest.mark.parametrize('noise', [0.0, 1e-5], ids=['exact', 'noise1e-5'])
@pytest.mark.parametrize('N', [8, 16, 32, 64, 128, 1024])
def test_model_gives_the_group_sums_and_counts(N, noise):
    """self join on tied keys (grid 2 / N, eps = 1 / N, the reference's sign configuration)"""
    cfg, eps = S.sign_cfg(N), 1.0 / N
    k = S.tied_input(N, S.SEEDS[N])
    rng = np.random.default_rng(N)
    cols = [rng.uniform(-1, 1, N), np.arange(N) / N]
    nz = rng.uniform(-noise, noise, (N, N)) if noise else None
    sums, cnt = G.group_sums(k, k, cols, cfg, eps, nz)
    wsums, wcnt = G.exact(k, k, cols, eps)
    assert wcnt.min() >= 1 and wcnt.max() >= 3  # every row is in its own group; real groups exist
    es, ec = np.max(np.abs(sums - wsums)), np.max(np.abs(cnt - wcnt))
    print(f'N={N} noise={noise}: group sum error {es:.3e}, count error {ec:.3e}')
    assert es < MODEL_BOUND and ec < MODEL_BOUND


@pytest.mark.parametrize('N', [8, 64])
def test_model_gives_the_lookup(N):
    """two tables: unique right keys, absent left keys give zero"""
    kl, kr, eps, cfg = G.lookup_tables(N, 7 * N)
    v = np.random.default_rng(N + 1).uniform(-1, 1, N)
    sums, cnt = G.group_sums(kl, kr, [v], cfg, eps)
    wsums, wcnt = G.exact(kl, kr, [v], eps)
    assert set(wcnt) == {0.0, 1.0}
    want = np.array([v[np.flatnonzero(kr == x)[0]] if x in kr else 0.0 for x in kl])
    assert np.array_equal(wsums[0], want)
    assert np.max(np.abs(sums - wsums)) < MODEL_BOUND and np.max(np.abs(cnt - wcnt)) < MODEL_BOUND


@pytest.fixture(scope='module')
def small_oracle():
    depth, rots = O.size_parameters(8)
    assert depth >= 1 + 1 + 21 + 1  # room for (3, 5, 2) below a level-1 input
    orc = O.Context(12, depth, 40, 60, 3, seed=5)
    orc.gen_rotation_keys(rots)
    return orc, rots


@pytest.mark.parametrize('cfg', [(3, 2, 2), (3, 3, 2), (3, 5, 2)])
def test_levels_follow_the_oracles_sign(small_oracle, cfg):
    orc, _ = small_oracle
    x = orc.encrypt(np.linspace(-0.9, 0.9, 8), 8, 1)
    D = orc.sign(x, *cfg).level - x.level
    assert D == G.sign_depth(cfg)
    for key_level in (0, 1, 4):
        col_max, out = F.group_sum_levels(key_level, cfg)
        assert (col_max, out) == (key_level + 1 + D - 2, key_level + 1 + D + 1)
        assert F.Context.group_sum_levels(key_level, cfg) == (col_max, out)


def test_levels_are_where_the_oracle_composition_ends(small_oracle):
    orc, rots = small_oracle
    N, cfg = 8, S.sign_cfg(8)
    k = S.tied_input(N, S.SEEDS[N])
    col_max, out = F.group_sum_levels(0, cfg)
    ok = orc.encrypt(k, N)
    outs, cnt = G.oracle_group_sums(orc, ok, ok, [orc.encrypt(np.arange(N) / N, N, col_max)], N, rots, cfg, 1.0 / N,
                                    True)
    assert outs[0].level == cnt.level == out
    assert outs[0].slots == cnt.slots == N
    # ... and where the rank ends
    assert orc.direct_sort(ok, N, rots, cfg, mode=1).level == out
    wsums, wcnt = G.exact(k, k, [np.arange(N) / N], 1.0 / N)
    assert np.max(np.abs(outs[0].decrypt() - wsums[0])) < 1e-3 and np.max(np.abs(cnt.decrypt() - wcnt)) < 1e-3


@pytest.mark.parametrize('args', [(-1, 3, 2, 2), (0, 2, 2, 2), (0, 5, 2, 2), (0, 3, -1, 2), (0, 3, 2, -1)])
def test_level_function_refuses_bad_arguments(args):
    with pytest.raises(F.FheError) as e:
        F.group_sum_levels(args[0], args[1:])
    assert e.value.code == F.FHE_EINVAL
    assert F.lib().fhe_group_sum_levels(*args, None, None) == F.FHE_EINVAL
    assert F.lib().fhe_group_sum_levels(0, 3, 2, 2, None, None) == F.FHE_OK  # either pointer may be null


def test_entry_points_refuse_null_handles():
    out, cnt = (C.c_void_p * 2)(1, 1), C.c_void_p(1)
    rc = F.lib().fhe_direct_group_sum(None, None, None, None, 2, 0.1, 8, None, 0, 3, 2, 2, out, C.byref(cnt))
    assert rc == F.FHE_EINVAL
    assert out[0] is None and out[1] is None and cnt.value is None  # no output handle is set
    o = C.c_void_p()
    assert F.lib().fhe_sub_pm_const_stacked(None, None, None, 1, 0.1, C.byref(o)) == F.FHE_EINVAL
    assert F.lib().fhe_mul_pairs(None, None, None, None, 1, C.byref(o)) == F.FHE_EINVAL
