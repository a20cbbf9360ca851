"""The k-way sorter's paired compares as one 2-member stack (fhe_set_kway_stack).

A k = 5 stage compares x against two rotations of itself.  With the switch on
the two sign chains run as one stack on the context's engine from the first
point at which they sit at one level, their lazy bootstraps included, and a pair
the level check has to bootstrap is refreshed in one pass; with it off they are
two one-ciphertext chains (on two lanes when fhe_set_sort_lanes >= 2).  The
output words must not depend on the switch.

Context as test_kway5_two_lanes_match_oracle (ring 2^11, depth 26, scale 2^59,
slots 32, budget (2, 2), CompositeSign(3, 2, 2)): that test pins the off path
to the CPU oracle, and at this depth the sorter bootstraps pairs.

All calls go through the C ABI (include/fhe_gpu.h) via fhesort.py.
"""
import numpy as np
import pytest

import fhesort as F

pytestmark = pytest.mark.gpu

CFG = (3, 2, 2)


def _slots(N):
    s = 1
    while s < N:
        s *= 2
    return s


@pytest.fixture(scope='module')
def kctx():
    gpu = F.Context(11, 26, 59, 60, 3, seed=54)
    gpu.gen_rotation_keys(F.kway_rotation_indices(25))
    boots = {s: F.Bootstrapper(gpu, s, (2, 2)) for s in (4, 16, 32)}
    yield gpu, boots
    for b in boots.values():
        b.close()
    gpu.close()


def run(gpu, boot, ct, k, M, stack, lanes=2):
    """one sort of `ct`: (output, checkLevelAndBoot bootstraps, boot counters)"""
    gpu.set_sort_lanes(lanes)
    gpu.set_kway_stack(stack)
    gpu.reset_counters()
    try:
        out = gpu.kway_sort(ct, k, M, CFG, boot=boot)
        return out, gpu.kway_bootstraps, gpu.boot_counters()
    finally:
        gpu.set_kway_stack(0)
        gpu.set_sort_lanes(2)


def test_switch_on_and_off_give_the_same_sort(kctx):
    gpu, boots = kctx
    k, M = 5, 2
    N = k ** M
    x = np.random.default_rng(5).permutation(N) * (1 - 1e-8) / N
    ct = gpu.encrypt(x, 32)

    def go(stack, lanes):
        return run(gpu, boots[32], ct, k, M, stack, lanes)

    off, nb_off, bc_off = go(0, 2)
    assert nb_off >= 1
    assert bc_off['calls'] == bc_off['ciphertexts'] > 0  # off: every bootstrap takes one ciphertext
    for lanes in (1, 2):
        on, nb_on, bc_on = go(1, lanes)
        assert on.info() == off.info()
        assert np.array_equal(on.data(), off.data()), f'lanes {lanes}: words differ with the switch on'
        assert nb_on == nb_off
        assert bc_on['ciphertexts'] == bc_off['ciphertexts']
        assert bc_on['calls'] < bc_on['ciphertexts'], bc_on  # a pair went through one stacked bootstrap
    off1, nb1, bc1 = go(0, 1)
    assert np.array_equal(off1.data(), off.data()) and nb1 == nb_off and bc1 == bc_off
    assert np.max(np.abs(gpu.decrypt(on)[:N] - np.sort(x))) < 0.01  # KWaySort235Test.cpp:291


@pytest.mark.parametrize('k,M', [(2, 2), (3, 2)])
def test_no_pairs_no_difference(kctx, k, M):
    gpu, boots = kctx
    N = k ** M
    x = np.random.default_rng(N).permutation(N) * (1 - 1e-8) / N
    s = _slots(N)
    ct = gpu.encrypt(x, s)
    off, nb_off, bc_off = run(gpu, boots[s], ct, k, M, 0)
    on, nb_on, bc_on = run(gpu, boots[s], ct, k, M, 1)
    assert on.info() == off.info() and np.array_equal(on.data(), off.data())
    assert nb_on == nb_off and bc_on == bc_off
    assert np.max(np.abs(gpu.decrypt(on)[:N] - np.sort(x))) < 0.01
