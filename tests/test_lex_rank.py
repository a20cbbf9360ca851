"""CPU checks of the lexicographic rank (fhe_direct_lex_rank): the
plaintext recurrence on the exact composite sign against np.lexsort's stable
ranks, the pure host level function against the model's levels and the oracle's
sign, the oracle composition decrypted against the exact ranks, and the refusals
that need no device.  No GPU work."""
import ctypes as C
import re

import numpy as np
import pytest

import fhesort as F
import group_model as G
import lex_model as X
import pyoracle as O
import stable_model as S

NEW = ('fhe_direct_lex_rank', 'fhe_lex_rank_levels', 'fhe_sub_lex_stacked', 'fhe_mul_lex')

KEY_SEED = X.KEY_SEED

# Largest |model - np.lexsort rank| the recurrence was found to have when it was
# specified (leading keys on the grid 2 / N drawn from 4 / 8 values, last key
# stable_model.tied_input, eps = eps_tb = 1 / N, stable_model.sign_cfg): a property
# of the sign polynomial at +-eps summed over the N pairs of a row, not of an
# implementation.  The tests assert 4x it, the project's margin for another draw.
SPECIFIED_ERR = {(8, 2): 9.1e-8, (8, 3): 1.3e-7, (64, 2): 1.6e-7, (64, 3): 1.4e-7}
# L = 4 was not part of that specification.  The error mechanism is the same for
# every L (no growth from L = 2 to L = 3 above), so L = 4 is held to 4x the larger
# of the two specified figures of its N.  Measured here on KEY_SEED's draws:
# 2.605e-07 (N = 8) and 1.518e-07 (N = 64); over seeds 1 .. 6 at most 2.605e-07 and
# 1.713e-07.
MEASURED_L4 = {8: 2.605e-07, 64: 1.518e-07}


def bound(N, L):
    return 4 * (SPECIFIED_ERR[(N, L)] if L < 4 else max(SPECIFIED_ERR[(N, 2)], SPECIFIED_ERR[(N, 3)]))


def test_header_and_binding_declare_the_lex_rank():
    src = re.sub(r'/\*.*?\*/', '', open(F.HEADER).read(), flags=re.S)
    names = set(re.findall(r'\b(fhe_[a-z0-9_]+)\s*\(', src))
    for f in NEW:
        assert f in names, f
        assert f in F._SIGS, f
        assert getattr(F.lib(), f, None) is not None, f  # exported by the built library
    for m in ('lex_rank', 'lex_sort_columns', 'sub_lex_stacked', 'mul_lex', 'lex_rank_levels'):
        assert callable(getattr(F.Context, m, None)), m
    assert callable(F.lex_rank_levels)


@pytest.mark.parametrize('L', [2, 3, 4])
@pytest.mark.parametrize('N', [8, 64])
def test_model_gives_the_stable_lexicographic_rank(N, L):
    keys = X.tied_keys(N, L, KEY_SEED[(N, L)])
    want = X.exact_ranks(keys)
    assert sorted(want) == list(range(N))
    # the leading keys really tie, and the order really needs them: the last key alone ranks otherwise
    assert all(len(np.unique(k)) < N for k in keys[:-1])
    assert not np.array_equal(want, S.stable_ranks(keys[-1]))
    got = X.ranks(keys, S.sign_cfg(N), 1.0 / N, 1.0 / N)
    err = np.max(np.abs(got - want))
    print(f'N={N} L={L}: model error {err:.3e} (bound {bound(N, L):.3e})')
    assert err <= bound(N, L)
    if L == 4:  # the recorded figure is this draw's
        assert abs(err - MEASURED_L4[N]) <= 1e-3 * MEASURED_L4[N]


@pytest.mark.parametrize('L', [2, 3])
def test_model_without_the_tiebreak(L):
    """c = 1/2: exact on pairwise-distinct tuples; rows tied on every key share the plain rank's tie value"""
    N, cfg = 8, S.sign_cfg(8)
    keys = X.distinct_keys(N, L, 5 + L)
    assert len(np.unique(np.stack(keys, 1), axis=0)) == N
    assert np.max(np.abs(X.ranks(keys, cfg, 1.0 / N, 0.0) - X.exact_ranks(keys))) <= bound(N, L)
    keys = X.tied_keys(N, L, KEY_SEED[(N, L)])
    tup = np.stack(keys, 1)
    smaller = np.array([sum(tuple(tup[j]) < tuple(tup[e]) for j in range(N)) for e in range(N)])
    mult = np.array([sum(tuple(tup[j]) == tuple(tup[e]) for j in range(N)) for e in range(N)])
    assert mult.max() >= 2
    want = smaller + (mult - 1) / 2.0  # tie_model: #{smaller} + (m - 1) / 2
    assert np.max(np.abs(X.ranks(keys, cfg, 1.0 / N, 0.0) - want)) <= bound(N, L)


def test_a_wide_key_sorts_as_two_digits():
    """a 6-bit key split 3 + 3 at N = 8: (3, 2, 2) resolves the digits' 1 / 16, not the packed key's 1 / 64"""
    N, cfg = 8, S.sign_cfg(8)
    wide = np.random.default_rng(11).permutation(64)[:N]
    hi, lo = (wide // 8) / 8.0, (wide % 8) / 8.0
    got = X.ranks([hi, lo], cfg, 1.0 / 16, 0.0)
    assert np.max(np.abs(got - S.stable_ranks(wide))) <= bound(N, 2)


@pytest.fixture(scope='module')
def small_oracle():
    depth, rots = O.size_parameters(8)
    orc = O.Context(12, depth, 40, 60, 3, seed=5)
    orc.gen_rotation_keys(rots)
    return orc, rots


@pytest.mark.parametrize('cfg', [(3, 0, 2), (3, 2, 2), (3, 3, 2), (3, 5, 2)])
@pytest.mark.parametrize('L', [2, 3, 4])
def test_level_function_matches_the_model(cfg, L):
    for key_level in (0, 1, 4):
        want = X.levels(key_level, L, cfg)[2]
        assert want == key_level + 1 + G.sign_depth(cfg) + L
        assert F.lex_rank_levels(key_level, L, cfg) == want
        assert F.Context.lex_rank_levels(key_level, L, cfg) == want
        # L - 1 levels below where the plain rank (and the group sums) end
        assert want == F.group_sum_levels(key_level, cfg)[1] + L - 1


def test_model_levels_follow_the_oracles_sign(small_oracle):
    orc, _ = small_oracle
    x = orc.encrypt(np.linspace(-0.9, 0.9, 8), 8, 1)
    for cfg in ((3, 2, 2), (3, 3, 2)):
        assert orc.sign(x, *cfg).level - x.level == G.sign_depth(cfg)


@pytest.mark.parametrize('args', [(0, 1, 3, 2, 2), (0, 5, 3, 2, 2), (-1, 2, 3, 2, 2), (0, 2, 5, 2, 2), (0, 2, 3, -1, 2),
                                  (0, 2, 3, 2, -1)])
def test_level_function_refuses_bad_arguments(args):
    with pytest.raises(F.FheError) as e:
        F.lex_rank_levels(args[0], args[1], args[2:])
    assert e.value.code == F.FHE_EINVAL
    assert F.lib().fhe_lex_rank_levels(*args, None) == F.FHE_EINVAL
    assert F.lib().fhe_lex_rank_levels(0, 2, 3, 2, 2, None) == F.FHE_OK  # the pointer may be null


def test_oracle_composition_decrypts_to_the_exact_ranks(small_oracle):
    orc, rots = small_oracle
    N, L, cfg = 8, 2, S.sign_cfg(8)
    keys = X.tied_keys(N, L, KEY_SEED[(N, L)])
    rank = X.oracle_lex_rank(orc, [orc.encrypt(k, N) for k in keys], N, rots, cfg, 1.0 / N, 1.0 / N)
    assert rank.level == F.lex_rank_levels(0, L, cfg) and rank.slots == N
    # ... L - 1 levels below the plain rank
    assert rank.level == orc.direct_sort(orc.encrypt(keys[-1], N), N, rots, cfg, mode=1).level + L - 1
    err = np.max(np.abs(rank.decrypt() - X.exact_ranks(keys)))
    print(f'oracle composition N={N} L={L}: max error {err:.3e}')
    # CKKS noise on top of the model's error: the bound the oracle's rank is held to (tests/test_stable_rank.py)
    assert err < 1e-4


def test_entry_points_refuse_null_handles():
    out = C.c_void_p(1)
    rc = F.lib().fhe_direct_lex_rank(None, None, 2, 0.1, 8, None, 0, 3, 2, 2, C.byref(out))
    assert rc == F.FHE_EINVAL and out.value is None  # no handle is set
    o = C.c_void_p()
    assert F.lib().fhe_sub_lex_stacked(None, None, 2, None, 1, None, 0.1, C.byref(o)) == F.FHE_EINVAL
    assert F.lib().fhe_mul_lex(None, None, 0.0, None, None, C.byref(o)) == F.FHE_EINVAL
