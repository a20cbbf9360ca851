"""CPU checks of the gather by encrypted position (fhe_direct_gather; DESIGN.md
§6.8): the plaintext model on the committed doubled-sinc tables gives the
neighbours at every size and offset within twice the error of the sort's own index
check on the same tables and inputs, the orientation of the differences is pinned
(the other one wraps around the end of the order), the pure host level function
agrees with what the CPU oracle does and stays inside the sort's depth, the oracle
composition decrypts to the model's neighbours, the new entry points are declared,
exported and bound, and the argument refusals that need no device.  No GPU work."""
import ctypes as C
import re

import numpy as np
import pytest

import fhesort as F
import gather_model as GM
import pyoracle as O
import stable_model as S

NEW = ('fhe_direct_gather', 'fhe_gather_levels', 'fhe_sub_offsets_stacked', 'fhe_mul_gather')
MARGIN = 2.0  # over the sort's own index check, measured on the same model and inputs


def offsets_of(N):
    return [0, 1, -1, 2, -2, N // 2, -(N // 2), N - 1, -(N - 1)]


def model_case(N, noise):
    """a rank (a permutation of 0 .. N - 1), two columns and the noise on the positions"""
    rng = np.random.default_rng([N, int(noise * 1e6)])
    pos = rng.permutation(N).astype(np.float64)
    cols = [rng.uniform(-1, 1, N), np.arange(N) / N]
    noisy = pos + (rng.uniform(-noise, noise, N) if noise else 0.0)
    return pos, noisy, cols


def ranks_checked(N):
    """the ranks whose rows are checked: all of them up to N = 64; at N = 1024, where every pair costs a series
    of degree ~6500, both ends, the middle and a draw of the others (32 rows)"""
    if N <= 64:
        return np.arange(N)
    fixed = np.array([0, 1, 2, N // 2 - 1, N // 2, N - 3, N - 2, N - 1])
    rest = np.setdiff1d(np.arange(N), fixed)
    return np.sort(np.concatenate([fixed, np.random.default_rng(N).choice(rest, 24, replace=False)]))


def sort_error(pos, noisy, cols, N):
    """largest error of the sort's index check on these positions and columns, and on the column of ones: the
    present flag is the gather of that column, so the yardstick sorts it too.  (It is the sort's worst column
    under noise, its terms all of one sign.  Measured, noise 1e-3 on both positions of a difference: the gather's
    argument noise is twice the sort's, and at N = 8 its 2.00e-3 would miss twice the 0.91e-3 of the data columns
    alone; twice the ones column's 1.07e-3 holds it.  DESIGN.md §6.8 has every figure.)"""
    order, slots = np.argsort(pos), ranks_checked(N)
    return max(np.max(np.abs(GM.sort_index_check(noisy, c, N, slots) - np.asarray(c)[order][slots]))
               for c in list(cols) + [np.ones(N)])


def test_header_and_binding_declare_the_gather():
    src = re.sub(r'/\*.*?\*/', '', open(F.HEADER).read(), flags=re.S)
    names = set(re.findall(r'\b(fhe_[a-z0-9_]+)\s*\(', src))
    for f in NEW:
        assert f in names, f
        assert f in F._SIGS, f
        assert getattr(F.lib(), f, None) is not None, f  # exported by the built library
    for m in ('gather', 'lag', 'lead', 'sub_offsets_stacked', 'mul_gather', 'gather_levels'):
        assert callable(getattr(F.Context, m, None)), m
    assert callable(F.gather_levels)


@pytest.mark.parametrize('noise', [0.0, 1e-3], ids=['exact', 'noise1e-3'])
@pytest.mark.parametrize('N', [8, 64, 1024])
def test_model_gives_the_neighbours(N, noise):
    """LAG / LEAD on a rank: every offset, the zero fill included"""
    pos, noisy, cols = model_case(N, noise)
    offs = offsets_of(N)
    order = np.argsort(pos)
    rows = order[ranks_checked(N)]  # the left rows standing at the checked ranks
    outs, pres = GM.gather(noisy[rows], noisy, cols, offs, N)
    wouts, wpres = GM.exact(pos[rows], pos, cols, offs)
    # the definition is the neighbour in rank order, zero beyond either end
    for k, o in enumerate(offs):
        q = pos[rows].astype(int) + o
        inside = (q >= 0) & (q < N)
        want = np.where(inside, np.asarray(cols[0])[order[np.clip(q, 0, N - 1)]], 0.0)
        assert np.array_equal(wouts[0][k], want) and np.array_equal(wpres[k], inside.astype(float)), o
    assert (wpres == 0).any() and (wpres == 1).any()
    bound = MARGIN * sort_error(pos, noisy, cols, N)
    eo, ep = np.max(np.abs(outs - wouts)), np.max(np.abs(pres - wpres))
    print(f'N={N} noise={noise}: gather error {eo:.3e}, present error {ep:.3e}, '
          f'sort index check {bound / MARGIN:.3e} (bound {bound:.3e})')
    assert eo <= bound and ep <= bound


@pytest.mark.parametrize('N', [8, 64, 1024])
def test_the_other_orientation_wraps(N):
    """the doubled series also fires at -N: with d = -(pos_l - pos_r + 1) the last row's
    LEAD(1) is the first row's value; with the specified orientation it is 0"""
    pos, _, cols = model_case(N, 0.0)
    v = 0.5 + 0.5 * np.asarray(cols[1])  # no zero among the values
    last, first = int(np.flatnonzero(pos == N - 1)[0]), int(np.flatnonzero(pos == 0)[0])
    ends = np.array([last, first])  # the two left rows in question
    good = GM.gather(pos[ends], pos, [v], [1], N)[0][0][0]
    bad = GM.gather(pos[ends], pos, [v], [1], N, flip=True)[0][0][0]
    tol = MARGIN * sort_error(pos, pos, [v], N)
    assert abs(bad[0] - v[first]) <= tol and v[first] > 100 * tol
    assert abs(good[0]) <= tol
    # the same at the other end for LAG(1)
    good = GM.gather(pos[ends], pos, [v], [-1], N)[0][0][0]
    bad = GM.gather(pos[ends], pos, [v], [-1], N, flip=True)[0][0][0]
    assert abs(bad[1] - v[last]) <= tol and abs(good[1]) <= tol
    # and the specified differences stay above -N and inside the domain
    for o in offsets_of(N):
        d = GM.differences(pos, pos, o)
        assert d.min() > -N and np.max(np.abs(d)) <= 2 * N - 2, o


@pytest.fixture(scope='module', params=[8, 64])
def oracle_case(request):
    """a tie-broken oracle rank of tied keys at ring 2^12 (N = 8: one comparator batch, 64: two),
    three columns at different levels, and the oracle composition's outputs"""
    N = request.param
    depth, rots = O.size_parameters(N)
    orc = O.Context(12, depth, 40, 60, 3, seed=800 + N)
    orc.gen_rotation_keys(rots)
    cfg = S.sign_cfg(N)
    key = S.tied_input(N, S.SEEDS[N])
    orank = S.oracle_rank(orc, orc.encrypt(key, N), N, rots, cfg, 1.0 / N)
    col_max, ser, out = F.gather_levels(orank.level, N)
    rng = np.random.default_rng(N)
    vals = [rng.uniform(-1, 1, N), np.arange(N) / N, rng.uniform(-1, 1, N)]
    ocols = [orc.encrypt(v, N, lv) for v, lv in zip(vals, (0, 1, col_max))]
    offs = [-(N - 1), -1, 0, 1, N - 1]
    outs, pres = GM.oracle_gather(orc, orank, orank, ocols, offs, N, rots, present=True)
    return dict(N=N, depth=depth, orc=orc, rots=rots, key=key, orank=orank, vals=vals, offs=offs, outs=outs,
                pres=pres, levels=(col_max, ser, out))


def test_levels_are_where_the_oracle_composition_ends(oracle_case):
    d = oracle_case
    col_max, ser, out = d['levels']
    assert F.Context.gather_levels(d['orank'].level, d['N']) == (col_max, ser, out)
    assert GM.levels(d['orank'].level, d['N']) == (d['orank'].level + 1, ser, col_max, out)
    assert all(o.level == out and o.slots == d['N'] for o in d['outs'])
    assert all(p.level == ser and p.slots == d['N'] for p in d['pres'])
    assert len(d['outs']) == 3 * len(d['offs']) and len(d['pres']) == len(d['offs'])
    # a rank from a level-0 key: the gather ends inside the sort's depth
    assert out <= d['depth'], (out, d['depth'])
    assert col_max == ser - 2 and out == ser + 1


def test_oracle_composition_decrypts_to_the_neighbours(oracle_case):
    d = oracle_case
    N, offs = d['N'], d['offs']
    pos = S.stable_ranks(d['key'])
    noisy = d['orank'].decrypt()
    assert np.max(np.abs(noisy - pos)) < 1e-3  # the noise the model is held to
    wouts, wpres = GM.exact(pos, pos, d['vals'], offs)
    # the model's bound on these inputs: the sort's index check on the same tables, positions and columns under
    # the uniform noise of 1e-3 the model is held to (the rank's own noise, asserted above, lies inside it)
    bound = MARGIN * sort_error(pos, pos + np.random.default_rng(N).uniform(-1e-3, 1e-3, N), d['vals'], N)
    K = len(offs)
    eo = max(np.max(np.abs(d['outs'][p * K + k].decrypt() - wouts[p][k])) for p in range(3) for k in range(K))
    ep = max(np.max(np.abs(d['pres'][k].decrypt() - wpres[k])) for k in range(K))
    print(f'N={N}: oracle composition error {eo:.3e}, present {ep:.3e}, bound {bound:.3e}')
    assert eo <= bound and ep <= bound


@pytest.mark.parametrize('args', [(-1, 8), (0, 0), (0, -8)])
def test_level_function_refuses_bad_arguments(args):
    with pytest.raises(F.FheError) as e:
        F.gather_levels(*args)
    assert e.value.code == F.FHE_EINVAL
    assert F.lib().fhe_gather_levels(*args, None, None, None) == F.FHE_EINVAL
    assert F.lib().fhe_gather_levels(0, 8, None, None, None) == F.FHE_OK  # any pointer may be null


def test_entry_points_refuse_null_handles():
    out = (C.c_void_p * 4)(1, 1, 1, 1)
    off = (C.c_int32 * 2)(-1, 1)
    rc = F.lib().fhe_direct_gather(None, None, None, None, 1, off, 2, 1, 0, 8, None, 0, out)
    assert rc == F.FHE_EINVAL
    assert all(out[i] is None for i in range(4))  # no output handle is set
    o = C.c_void_p()
    assert F.lib().fhe_sub_offsets_stacked(None, None, None, 1, off, 2, C.byref(o)) == F.FHE_EINVAL
    assert F.lib().fhe_mul_gather(None, None, None, 1, 1, C.byref(o)) == F.FHE_EINVAL
