"""Tables of different sizes in the all-pairs operators, on the CPU
(fhe_set_pair_tables, fhe_pair_shape).

The layout: fhe_pair_shape against the model for every power-of-two pair and
ring, the pair map by enumeration (every (left row, right row) met exactly once),
and a numpy walk of the whole layout -- tiling, shifts, masks, batch sums,
partition fold, residue fold -- against the exact sums.  The refusals of the two
host entry points.  The oracle compositions of tests/rect_model.py for the group
sums of (8, 2) and (2, 8), decrypted against the exact sums: their largest errors
are recorded here and in tests/test_gpu_rect_tables.py, which takes its margin
over them."""
import ctypes as C

import numpy as np
import pytest

import fhesort as F
import group_model as G
import rect_model as RM
import stable_model as S

POW2 = [1 << i for i in range(1, 11)]  # 2 .. 1024
PAIRS = [(a, b) for a in POW2 for b in POW2 if max(a, b) >= 4]
RINGS = [1 << i for i in range(9, 16)]

# Largest |decrypted - exact| of the oracle compositions of the group sums (count and two columns) on
# rect_model.oracle_case's inputs and seeds, measured on the CPU by test_oracle_group_sums_decrypt_to_the_exact_sums.
ORACLE_ERR = {(8, 2): 9.002e-09, (2, 8): 2.641e-08}


def test_pair_shape_matches_the_model():
    for ring in RINGS:
        for Nl, Nr in PAIRS:
            if max(Nl, Nr) > ring:  # the square shape's refusal: the ring does not hold N
                with pytest.raises(F.FheError) as e:
                    F.pair_shape(Nl, Nr, ring)
                assert e.value.code == F.FHE_EINVAL
                continue
            got = F.pair_shape(Nl, Nr, ring)
            assert got == RM.pair_shape(Nl, Nr, ring), (Nl, Nr, ring)
            S_, P, nb, npb, fold = got
            N, n = max(Nl, Nr), min(Nl, Nr)
            assert S_ <= ring and S_ == N * P and P * nb == n and P % npb == 0, (Nl, Nr, ring, got)
            assert Nl << fold == max(Nl, Nr), (Nl, Nr, fold)
            if Nl == Nr:
                assert got[:4] == S.rank_shape(N, ring) and fold == 0, (N, ring)
            else:  # never more batches than the square call on the padded table
                assert nb <= S.rank_shape(N, ring)[2]
    assert F.Context.pair_shape(1024, 32, 1 << 15) == (1 << 15, 32, 1, 32, 0)
    assert F.pair_shape(32, 1024, 1 << 15) == (1 << 15, 32, 1, 32, 5)
    assert F.pair_shape(1024, 256, 1 << 15)[2] == 8 and S.rank_shape(1024, 1 << 15)[2] == 32


def test_any_output_pointer_may_be_null():
    assert F.lib().fhe_pair_shape(8, 2, 2048, None, None, None, None, None) == F.FHE_OK
    nb = C.c_int()
    assert F.lib().fhe_pair_shape(64, 32, 1024, None, C.byref(nb), None, None, None) == F.FHE_OK
    assert nb.value == 2


@pytest.mark.parametrize('ring', [1 << 11, 1 << 12, 1 << 15])
def test_every_pair_is_met_exactly_once(ring):
    for Nl, Nr in PAIRS:
        if Nl * Nr > 1 << 14 or max(Nl, Nr) > ring:
            continue
        left, right = RM.pair_map(Nl, Nr, ring)
        assert left.size == Nl * Nr  # as many slots as pairs
        seen = np.bincount((left * Nr + right).reshape(-1), minlength=Nl * Nr)
        assert np.array_equal(seen, np.ones(Nl * Nr, dtype=seen.dtype)), (Nl, Nr, ring)


@pytest.mark.parametrize('ring', [1 << 9, 1 << 11, 1 << 12])
def test_numpy_walk_of_the_layout_gives_the_exact_sums(ring):
    rng = np.random.default_rng(ring)
    for Nl, Nr in PAIRS:
        if Nl * Nr > 1 << 12 or max(Nl, Nr) > ring:
            continue
        keys = rng.integers(0, max(2, min(Nl, Nr)), 2 * max(Nl, Nr)) / 8.0
        kl, kr = keys[:Nl], keys[max(Nl, Nr):max(Nl, Nr) + Nr]
        cols = [rng.uniform(-1, 1, Nr), np.arange(Nr, dtype=np.float64)]
        sums, cnt = RM.simulate_group_sums(kl, kr, cols, 1.0 / 32, ring)
        wsums, wcnt = G.exact(kl, kr, cols, 1.0 / 32)
        assert sums.shape == wsums.shape == (2, Nl)
        assert np.max(np.abs(sums - wsums)) <= 1e-12 and np.max(np.abs(cnt - wcnt)) <= 1e-12, (Nl, Nr, ring)


def test_sentinel_padding_matches_nothing():
    """the documented padding of today's square call: the padded rows add nothing, to the counts either"""
    d = RM.inputs(8, 2, RM.INPUT_SEED)
    kr = RM.sentinel_pad(d['kr'], 8, d['eps'])
    cols = [np.concatenate([c, np.zeros(6)]) for c in d['cols']]
    assert np.min(np.abs(kr[2:, None] - np.concatenate([d['kl'], kr[:2]])[None, :])) >= 2 * d['eps']
    psums, pcnt = G.exact(d['kl'], kr, cols, d['eps'])
    wsums, wcnt = G.exact(d['kl'], d['kr'], d['cols'], d['eps'])
    assert np.array_equal(psums, wsums) and np.array_equal(pcnt, wcnt)


BAD_COUNTS = [(3, 8), (8, 3), (1, 8), (8, 1), (0, 8), (8, 0), (-4, 8), (8, 12)]


@pytest.mark.parametrize('nl,nr', BAD_COUNTS)
def test_counts_that_are_no_powers_of_two_are_refused(nl, nr):
    with pytest.raises(F.FheError) as e:
        F.pair_shape(nl, nr, 2048)
    assert e.value.code == F.FHE_EINVAL and 'powers of two' in str(e.value)
    # fhe_set_pair_tables checks the counts before it looks at the context
    assert F.lib().fhe_set_pair_tables(None, nl, nr) == F.FHE_EINVAL
    assert 'powers of two' in F.lib().fhe_last_error().decode()


def test_sizes_the_sort_has_no_parameters_for_are_refused():
    for nl, nr in ((2, 2), (4096, 8), (8, 4096)):
        with pytest.raises(F.FheError) as e:
            F.pair_shape(nl, nr, 1 << 15)
        assert e.value.code == F.FHE_EINVAL and 'fhe_size_parameters' in str(e.value)
        assert F.lib().fhe_set_pair_tables(None, nl, nr) == F.FHE_EINVAL
        assert 'fhe_size_parameters' in F.lib().fhe_last_error().decode()


def test_a_ring_too_small_and_a_bad_ring_are_refused():
    for nl, nr, ring in ((1024, 32, 512), (32, 1024, 512), (8, 8, 4)):
        with pytest.raises(F.FheError) as e:
            F.pair_shape(nl, nr, ring)
        assert e.value.code == F.FHE_EINVAL and 'exceed' in str(e.value)
    for ring in (0, -8, 100):
        with pytest.raises(F.FheError) as e:
            F.pair_shape(8, 2, ring)
        assert e.value.code == F.FHE_EINVAL and 'ring_slots' in str(e.value)


def test_a_null_context_is_refused():
    for nl, nr in ((0, 0), (8, 2)):
        assert F.lib().fhe_set_pair_tables(None, nl, nr) == F.FHE_EINVAL
        assert 'ctx' in F.lib().fhe_last_error().decode()


@pytest.mark.parametrize('Nl,Nr', [(8, 2), (2, 8)])
def test_oracle_group_sums_decrypt_to_the_exact_sums(Nl, Nr):
    c = RM.oracle_case(Nl, Nr, 12, ['group'])
    outs, cnt = c['res']['group']
    col_max, out_level = F.group_sum_levels(0, c['d']['cfg'])
    assert all(o.slots == Nl and o.level == out_level for o in outs + [cnt])  # no level beyond the square call's
    assert c['enc']['cols'][1].level == 1 <= col_max
    err = RM.largest_error((outs, cnt), c['want']['group'])
    print(f'({Nl}, {Nr}) oracle composition: largest error {err:.3e} (recorded {ORACLE_ERR[(Nl, Nr)]:.3e})')
    wcnt = c['want']['group'][1]
    assert (wcnt == 0).any() and (wcnt > 0).any()
    # the margin the GPU tests take: room for another seed's noise, not for a defect
    assert err <= 4 * ORACLE_ERR[(Nl, Nr)]
