"""CPU checks of the record sort (fhe_direct_sort_columns): the boundary is
declared and bound, the binding's constants are the sources', and the contract
holds in plaintext -- out[p] = sum_i col_p[i] * [rank_i = j] is col_p[argsort(key)]
for distinct keys and follows tests/tie_model.py for tied ones.  No GPU work."""
import os
import re

import numpy as np

import fhesort as F
import tie_model

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('fhe_direct_sort_columns', 'fhe_set_sort_column_members', 'fhe_mul_columns', 'fhe_ct_sum_member_groups')


def test_header_declares_the_record_sort():
    src = re.sub(r'/\*.*?\*/', '', open(F.HEADER).read(), flags=re.S)
    names = set(re.findall(r'\b(fhe_[a-z0-9_]+)\s*\(', src))
    for f in NEW:
        assert f in names, f
        assert f in F._SIGS, f


def test_context_has_the_methods():
    for m in ('direct_sort_columns', 'mul_columns', 'sum_member_groups', 'set_sort_column_members'):
        assert callable(getattr(F.Context, m, None)), m


def test_binding_constants_are_the_sources():
    kern = open(os.path.join(REPO, 'fhe-sorting_amd', 'csrc', 'device', 'kernels.hip')).read()
    assert int(re.search(r'constexpr int TC_PC = (\d+);', kern).group(1)) == F.TENSOR_COLS_PER_THREAD
    capi = open(os.path.join(REPO, 'fhe-sorting_amd', 'csrc', 'capi', 'capi.cpp')).read()
    assert int(re.search(r'int sort_col_members = (\d+);', capi).group(1)) == F.SORT_COLUMN_MEMBERS_DEFAULT


def columns_model(key, cols, cfg):
    """The record sort in plaintext: the weights rotationIndexCheckN gives
    element i in output slot k depend on the key's ranks alone (tie_model), and
    every column is weighed by them."""
    key = np.asarray(key, dtype=np.float64)
    N = len(key)
    r = tie_model.ranks(key, cfg)
    k = np.arange(N)[None, :]
    d = k - r[:, None]
    w = np.sinc(d) + np.sinc(d + np.where(k > np.arange(N)[:, None], -N, N))
    return [np.asarray(c, dtype=np.float64) @ w for c in cols]


def test_model_permutes_columns_for_distinct_keys():
    rng = np.random.default_rng(1)
    for N, cfg in ((16, (3, 2, 2)), (64, (3, 3, 2))):
        key = rng.permutation(N) / N
        cols = [key, rng.uniform(-1, 1, N), rng.uniform(-1, 1, N)]
        order = np.argsort(key)
        outs = columns_model(key, cols, cfg)
        for c, o in zip(cols, outs):
            assert np.max(np.abs(o - c[order])) < 0.01  # the reference's DirectSortTest bound, |col| <= 1
        assert np.allclose(outs[0], tie_model.direct_sort(key, cfg), rtol=0, atol=1e-12)
        # exact integer ranks: the indicator form of the contract
        ind = (np.rint(tie_model.ranks(key, cfg))[:, None] == np.arange(N)[None, :]).astype(float)
        for c in cols:
            assert np.array_equal(c @ ind, c[order])


def test_model_follows_tie_model_for_tied_keys():
    """A key of odd multiplicity 3: its three records land summed in the one slot
    of their common rank, zeros in the run's other two slots -- for every column
    as for the key.  An even multiplicity spreads them with sinc tails."""
    N, cfg = 16, (3, 2, 2)
    key = np.arange(N) / N
    key[5] = key[6] = key[4]  # multiplicity 3 -> common rank 5
    rng = np.random.default_rng(2)
    col = rng.uniform(-1, 1, N)
    okey, ocol = columns_model(key, [key, col], cfg)
    assert np.allclose(okey, tie_model.direct_sort(key, cfg), rtol=0, atol=1e-12)
    assert abs(ocol[5] - col[4:7].sum()) < 0.01 and abs(ocol[4]) < 0.01 and abs(ocol[6]) < 0.01
    untouched = [i for i in range(N) if i not in (4, 5, 6)]
    assert np.max(np.abs(ocol[untouched] - col[untouched])) < 0.01
    key2 = np.arange(N) / N
    key2[9] = key2[8]  # multiplicity 2 -> half-integer rank
    o2 = columns_model(key2, [col], cfg)[0]
    assert np.max(np.abs(o2 - col)) > 0.05  # not a permutation: the pair is spread over the slots
