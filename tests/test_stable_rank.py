"""Tie-broken (stable) rank on the CPU: the offset layout of the C ABI against
its formula, the plaintext model against the stable argsort ranks, and the
CPU-oracle composition that the GPU rank is held to word for word
(tests/test_gpu_stable.py).  Inputs hold an odd and an even multiplicity, lie on
the grid 2 / N and are ranked with eps = 1 / N under the reference's sign
configuration for N."""
import numpy as np
import pytest

import fhesort as F
import pyoracle as O
import stable_model as M
import tie_model as T


@pytest.mark.parametrize('N', [4, 8, 64])
def test_offsets_follow_the_slot_layout(N):
    eps = 1.0 / N
    for P in sorted({1, 2, N // 2, N}):
        S = N * P
        seen_self = 0
        for b in range(N // P):
            got = F.tiebreak_offsets(N, S, b, eps)
            assert got.shape == (S,)
            assert np.array_equal(np.abs(got), np.full(S, eps)), (N, S, b)
            assert np.array_equal(got, M.offsets(N, S, b, eps)), (N, S, b)
            # element by element: slot s compares e = s mod N with j = (e + t) mod N
            s = np.arange(S)
            e, t = s % N, b * P + s // N
            j = (e + t) % N
            assert np.array_equal(got > 0, j <= e), (N, S, b)
            if b == 0:
                assert np.all(got[:N] == eps)  # t = 0: the self comparisons
                seen_self += 1
        assert seen_self == 1


def test_offsets_refuse_bad_arguments():
    for args in ((8, 64, 1, 0.1), (8, 16, 4, 0.1), (8, 16, -1, 0.1), (8, 24, 0, 0.1), (6, 12, 0, 0.1), (8, 16, 0, 0.5),
                 (8, 16, 0, -1.0), (8, 128, 0, 0.1)):
        with pytest.raises(F.FheError) as e:
            F.tiebreak_offsets(*args)
        assert e.value.code == F.FHE_EINVAL, args


@pytest.mark.parametrize('N', [8, 16, 32, 128, 1024])
def test_model_gives_the_stable_ranks(N):
    x = M.tied_input(N, M.SEEDS[N])
    cfg, eps = M.sign_cfg(N), 1.0 / N
    want = M.stable_ranks(x)
    clean = np.max(np.abs(M.ranks(x, cfg, eps) - want))
    noise = np.random.default_rng(N).uniform(-1e-5, 1e-5, (N, N))
    noisy = np.max(np.abs(M.ranks(x, cfg, eps, noise) - want))
    plain = np.max(np.abs(T.ranks(x, cfg) - want))
    print(f'N={N}: model rank error {clean:.3e}, with 1e-5 noise {noisy:.3e}; plain rank {plain:.3e}')
    assert clean < 1e-3 and noisy < 1e-3
    assert plain > 0.49  # the reference's rank does not order the ties: (m - 1) / 2 off at the ends of a run


def test_model_without_offset_is_the_tie_model():
    for N in (8, 64):
        x = M.tied_input(N, M.SEEDS[N])
        assert np.array_equal(M.ranks(x, M.sign_cfg(N), 0.0), T.ranks(x, M.sign_cfg(N)))


def test_oracle_composition_ranks_and_sorts_ties():
    """N = 8 at ring 2^12, the table depth, 40-bit scaling: the composition gives
    the stable ranks (measured 1.3e-7; the bound leaves room for other seeds),
    the oracle's index check on it sorts, the plain oracle sort does not; with
    eps = 0 the composition is the oracle's constructRank word for word."""
    N = 8
    cfg, eps = M.sign_cfg(N), 1.0 / N
    depth, rots = O.size_parameters(N)
    orc = O.Context(12, depth, 40, 60, 3, seed=308)
    orc.gen_rotation_keys(rots)
    x = M.tied_input(N, M.SEEDS[N])
    ox = orc.encrypt(x, N)
    plain_rank = orc.direct_sort(ox, N, rots, cfg, mode=1)
    same = M.oracle_rank(orc, ox, N, rots, cfg, 0.0)
    assert same.info() == plain_rank.info() and np.array_equal(same.data(), plain_rank.data())
    rank = M.oracle_rank(orc, ox, N, rots, cfg, eps)
    assert rank.level == plain_rank.level and rank.slots == N
    rerr = np.max(np.abs(orc.decrypt(rank) - M.stable_ranks(x)))
    out = orc.direct_sort(ox, N, rots, cfg, mode=2, rank=rank)
    serr = np.max(np.abs(orc.decrypt(out) - np.sort(x)))
    perr = np.max(np.abs(orc.decrypt(orc.direct_sort(ox, N, rots, cfg)) - np.sort(x)))
    print(f'oracle N={N}: stable rank error {rerr:.3e}, sort error {serr:.3e}; plain sort error {perr:.3e}')
    assert rerr < 1e-4
    assert serr < 0.01  # DirectSortTest's bound
    assert out.level == depth
    assert perr > 0.1
