"""CPU checks of the pure host functions behind the folded constants and the
stacked masked sums: the byte formula the batched masked-sum launches book
 and the decision whether mul_add folds its left constant.
No GPU call is issued."""
import math

import pytest

import fhesort as F


def units(m, nb, tile):
    return F.lib().fhe_plain_sum_batches_limb_units(m, nb, tile)


def test_tile_is_four_batches():
    assert F.lib().fhe_plain_sum_tile() == 4


@pytest.mark.parametrize('m', [1, 4, 5, 32, 33])
@pytest.mark.parametrize('nb', [1, 3, 4, 5, 9, 32])
@pytest.mark.parametrize('tile', [1, 4, 8])
def test_limb_units_formula(m, nb, tile):
    # every ciphertext pair once per tile of batches, every mask once, every output pair once
    assert units(m, nb, tile) == 2 * m * math.ceil(nb / tile) + m * nb + 2 * nb


def test_limb_units_against_separate_sums():
    # the rank of the N = 1024 sort: 32 batches of 32 terms, 1,600 units against 3,136
    assert units(32, 32, 4) == 1600
    assert 32 * (3 * 32 + 2) == 3136
    # a tile of one batch is the separate sums' traffic
    for m, nb in ((1, 1), (5, 3), (32, 32)):
        assert units(m, nb, 1) == nb * (3 * m + 2)
    assert units(4, 4, 0) < 0


def test_left_constant_folds_only_without_level_adjustment():
    fold = F.lib().fhe_mul_fold_left
    for la in range(6):
        for lb in range(6):
            assert fold(1, la, lb) == (1 if la >= lb else 0)
            assert fold(0, la, lb) == 0
