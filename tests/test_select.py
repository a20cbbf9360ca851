"""CPU checks of the order-statistic select (fhe_direct_select) through its pure
host entry point fhe_select_layout: the member count, the window starts and
their disjointness for every size table, and a numpy model of the definition
with an exact delta that returns sorted(x)[t[p]] at slot p.  No GPU work."""
import os
import re

import numpy as np
import pytest

import fhesort as F
import select_model as M

SIZES = (4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048)
NEW = ('fhe_direct_select', 'fhe_select_layout', 'fhe_pt_encode_select', 'fhe_mul_plain_sum_groups')


def test_header_and_binding_declare_the_select():
    src = re.sub(r'/\*.*?\*/', '', open(F.HEADER).read(), flags=re.S)
    names = set(re.findall(r'\b(fhe_[a-z0-9_]+)\s*\(', src))
    for f in NEW:
        assert f in names, f
        assert f in F._SIGS, f
    for m in ('direct_select', 'encode_select', 'mul_plain_sum_groups', 'select_layout'):
        assert callable(getattr(F.Context, m, None)), m


def test_binding_constant_is_the_sources():
    kern = open(os.path.join(F.HERE, 'csrc', 'device', 'kernels.hip')).read()
    assert int(re.search(r'constexpr int PSG_TG = (\d+);', kern).group(1)) == F.PLAIN_SUM_GROUPS_PER_THREAD


def shapes(N):
    return sorted({1, 2, 4, min(N, 32)})


@pytest.mark.parametrize('N', SIZES)
def test_layout(N):
    F.size_parameters(N)  # N is a size-table entry
    for parts in shapes(N):
        S = N * parts
        cap = parts - 1 if parts >= 2 else 1
        assert cap == M.cap_of(N, S)
        for k in sorted({1, cap, cap + 1, N}):
            members, member, start = F.select_layout(N, S, k)
            assert members == -(-k // cap), (N, S, k)
            assert len(member) == len(start) == k
            p = np.arange(k)
            assert np.array_equal(np.asarray(member), p // cap)
            assert np.array_equal(np.asarray(start) % N, p % N)
            assert all(0 <= s < S for s in start)
            for z in range(members):
                # pairwise disjoint cyclic intervals of N slots: together they cover
                # N slots each, none twice
                mine = [start[q] for q in range(k) if member[q] == z]
                hit = np.zeros(S, dtype=np.int64)
                for s in mine:
                    hit[(s + np.arange(N)) % S] += 1
                assert hit.max() == 1 and hit.sum() == N * len(mine), (N, S, k, z)


def target_lists(N, rng):
    yield 'ascending', list(range(N))
    yield 'descending', list(range(N - 1, -1, -1))
    yield 'repeated', [int(t) for t in rng.integers(0, N, size=N)]
    yield 'same', [N // 2] * min(N, 5)
    yield 'single', [N - 1]
    yield 'min max median', [0, N - 1, N // 2]


@pytest.mark.parametrize('N', (4, 8, 16, 32, 64))
def test_model_returns_the_order_statistics(N):
    rng = np.random.default_rng(N)
    x = rng.permutation(N) / N - 0.5
    want = np.sort(x)
    for parts in shapes(N):
        S = N * parts
        for what, t in target_lists(N, rng):
            got = M.select(x, t, N, S)
            assert np.array_equal(got[:len(t)], want[t]), (N, S, what)
            assert not got[len(t):].any(), (N, S, what)


def test_windows_hold_every_residue_once():
    """what makes the window sum the whole inner product: a window of N
    consecutive slots meets every rank_i (period N) exactly once"""
    for N, S in ((4, 4), (4, 8), (16, 256), (64, 1024)):
        _, _, start = F.select_layout(N, S, N)
        for s in start:
            assert sorted((s + np.arange(N)) % S % N) == list(range(N))


@pytest.mark.parametrize('args', [(3, 12, 1), (16, 24, 1), (16, 16 * 32, 1), (16, 16 * 3, 1), (16, 8, 1), (0, 0, 1),
                                  (16, 256, 0), (16, 256, 17), (16, 256, -1)])
def test_bad_arguments_are_refused(args):
    with pytest.raises(F.FheError) as e:
        F.select_layout(*args)
    assert e.value.code == F.FHE_EINVAL
    assert F.lib().fhe_select_layout(args[0], args[1], args[2], None, None, 0) == -F.FHE_EINVAL
