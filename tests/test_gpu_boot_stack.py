"""Bootstrapping a ciphertext stack in one pass (fhe_bootstrap, fhe_bootstrap_stage,
fhe_check_level_and_boot on fhe_ct_stack handles).

Every member of a stacked result holds, word for word, what the same call gives
for that member alone; the transforms run through the member-blocked kernels
(k_lt_inner_mb, k_ks_inner_mk_sum_mb: keys, permutation indices and plaintexts
read once per block of members), whose launch counts and byte model are checked
through the kernel clock.

Shapes (ring 2^11, scale 2^59, first modulus 2^60, dnum 3).  From the schedule
of bootstrap.cpp: slots 8 with budget (2, 1) has one rotated giant step in its
decode level (the stacked partial-trace / giant key switch runs); slots 32 with
budget (1, 1) has a giant step of 32 babies -- more than one launch holds
(LT_MAXB = 16), so the baby kernel runs chunked, accumulating -- and a rotated
giant as well.

All calls go through the C ABI (include/fhe_gpu.h) via fhesort.py.
"""
import numpy as np
import pytest

import fhesort as F
import pyoracle as O
from test_gpu_hybrid import same

pytestmark = pytest.mark.gpu

LOGN, DEPTH, SEED = 11, 24, 61
LT_MB, KS_MB, LT_ONE = 'k_lt_inner_mb<', 'k_ks_inner_mk_sum_mb<', 'k_lt_inner<'


def same_words(gpu, stack, singles):
    """member m of `stack` == singles[m]: shape and every limb word"""
    for m, one in enumerate(singles):
        got = gpu.member(stack, m)
        assert got.info() == one.info(), (m, got.info(), one.info())
        gd, od = got.data(), one.data()
        if not np.array_equal(gd, od):
            bad = np.argwhere(gd != od)
            raise AssertionError(f'member {m}: {len(bad)} limb words differ, first at {bad[0].tolist()}')


def clocked(stats, prefix, field):
    return sum(v[field] for k, v in stats.items() if k.startswith(prefix))


@pytest.fixture(scope='module')
def ctx8():
    """slots 8, budget (2, 1): three distinct ciphertexts at level L - 3"""
    gpu = F.Context(LOGN, DEPTH, 59, 60, 3, seed=SEED)
    gb = F.Bootstrapper(gpu, 8, (2, 1))
    vals = np.random.default_rng(8).uniform(-1, 1, (3, 8))
    cts = [gpu.encrypt(v, 8, level=DEPTH - 3) for v in vals]
    yield gpu, gb, vals, cts
    gb.close()
    gpu.close()


@pytest.fixture(scope='module')
def ctx32():
    """slots 32, budget (1, 1): five distinct ciphertexts at level L - 3 with their
    single-ciphertext raised forms, CoeffsToSlots and bootstraps (computed once)"""
    gpu = F.Context(LOGN, DEPTH, 59, 60, 3, seed=SEED + 1)
    gb = F.Bootstrapper(gpu, 32, (1, 1))
    vals = np.random.default_rng(32).uniform(-1, 1, (5, 32))
    cts = [gpu.encrypt(v, 32, level=DEPTH - 3) for v in vals]
    raised = [gb.mod_raise(gpu.mul_const_to(c, 0.25, DEPTH)) for c in cts]
    with F.KernelClock(gpu) as clk:
        c2s = [gb.coeffs_to_slots(r) for r in raised[:1]]
    c2s += [gb.coeffs_to_slots(r) for r in raised[1:]]
    boots = [gb.bootstrap(c) for c in cts]
    yield dict(gpu=gpu, gb=gb, vals=vals, cts=cts, raised=raised, c2s=c2s, boots=boots, clk1=clk.stats)
    gb.close()
    gpu.close()


def test_stages_and_bootstrap_same_words(ctx8):
    gpu, gb, vals, cts = ctx8
    st = gpu.stack(cts)
    same_words(gpu, gpu.conjugate(st), [gpu.conjugate(c) for c in cts])
    last1 = [gpu.mul_const_to(c, 0.25, DEPTH) for c in cts]
    last = gpu.mul_const_to(st, 0.25, DEPTH)
    same_words(gpu, last, last1)
    raised1 = [gb.mod_raise(c) for c in last1]
    raised = gb.mod_raise(last)
    same_words(gpu, raised, raised1)
    c2s1 = [gb.coeffs_to_slots(c) for c in raised1]
    c2s = gb.coeffs_to_slots(raised)
    same_words(gpu, c2s, c2s1)
    em1 = [gb.eval_mod(c) for c in c2s1]
    em = gb.eval_mod(c2s)
    same_words(gpu, em, em1)
    s2c1 = [gb.slots_to_coeffs(c) for c in em1]
    with F.KernelClock(gpu) as clk:
        s2c = gb.slots_to_coeffs(em)
    same_words(gpu, s2c, s2c1)
    # the decode level's rotated giant went through the stacked key-switch sum
    assert any(k.startswith(KS_MB) for k in clk.stats), sorted(clk.stats)
    assert any(k.startswith(LT_MB) for k in clk.stats), sorted(clk.stats)
    assert not any(k.startswith(LT_ONE) for k in clk.stats), sorted(clk.stats)

    out1 = [gb.bootstrap(c) for c in cts]
    out = gb.bootstrap(st)
    same_words(gpu, out, out1)
    assert out.level == gb.depth
    for m in range(3):
        # the bound test_bootstrap_refreshes_levels uses at this ring
        assert np.max(np.abs(gpu.decrypt(gpu.member(out, m)) - vals[m])) < 1e-4


def test_stacked_member0_equals_oracle(ctx8):
    gpu, gb, vals, cts = ctx8
    orc = O.Context(LOGN, DEPTH, 59, 60, 3, seed=SEED)  # GPU keygen == oracle keygen for one seed
    ob = O.Bootstrapper(orc, 8, (2, 1))
    assert gb.rotations() == ob.rotations() and gb.depth == ob.depth
    ox = orc.encrypt(vals[0], 8, level=DEPTH - 3)
    st = gpu.stack([gpu.from_oracle(ox), cts[1], cts[2]])
    same(gpu.member(gb.bootstrap(st), 0), ob.bootstrap(ox))


@pytest.mark.parametrize('B', [2, 5])  # one pair block; a full block of 4 and a guarded tail
def test_member_blocks_and_chunked_babies(ctx32, B):
    c = ctx32
    gpu, gb = c['gpu'], c['gb']
    with F.KernelClock(gpu) as clk:
        c2s = gb.coeffs_to_slots(gpu.stack(c['raised'][:B]))
    same_words(gpu, c2s, c['c2s'][:B])
    assert any(k.startswith(LT_MB) for k in clk.stats), sorted(clk.stats)
    same_words(gpu, gb.bootstrap(gpu.stack(c['cts'][:B])), c['boots'][:B])


def test_one_launch_serves_the_stack(ctx32):
    c = ctx32
    gpu, gb = c['gpu'], c['gb']
    one = c['clk1']  # CoeffsToSlots of one ciphertext: today's kernel under its own name
    assert clocked(one, LT_ONE, 'launches') > 0 and clocked(one, LT_MB, 'launches') == 0
    # the 32-baby giant cannot fit one launch: more launches than giants of the level
    assert clocked(one, LT_ONE, 'launches') >= 3
    st = {}
    for B in (2, 4):
        with F.KernelClock(gpu) as clk:
            gb.coeffs_to_slots(gpu.stack(c['raised'][:B]))
        st[B] = clk.stats
        assert clocked(st[B], LT_ONE, 'launches') == 0
    assert clocked(st[4], LT_MB, 'launches') == clocked(one, LT_ONE, 'launches')
    assert clocked(st[2], LT_MB, 'launches') == clocked(one, LT_ONE, 'launches')
    b1, b2, b4 = clocked(one, LT_ONE, 'bytes'), clocked(st[2], LT_MB, 'bytes'), clocked(st[4], LT_MB, 'bytes')
    assert b4 - b2 == 2 * (b2 - b1), (b1, b2, b4)
    assert b2 < 2 * b1, (b1, b2)


def test_counters_scale_with_the_stack(ctx8):
    gpu, gb, vals, cts = ctx8
    gpu.reset_counters()
    gb.bootstrap(cts[0])
    c1, bc1 = gpu.counters(), gpu.boot_counters()
    gpu.reset_counters()
    gb.bootstrap(gpu.stack(cts))
    c3, bc3 = gpu.counters(), gpu.boot_counters()
    gpu.reset_counters()
    assert gpu.boot_counters() == {'calls': 0, 'ciphertexts': 0}
    assert bc1 == {'calls': 1, 'ciphertexts': 1}
    assert bc3 == {'calls': 1, 'ciphertexts': 3}
    assert c3 == {k: 3 * v for k, v in c1.items()}, (c1, c3)


def test_check_level_and_boot_on_a_pair(ctx8):
    gpu, gb, vals, cts = ctx8
    low = [gpu.encrypt(v, 8, level=DEPTH - 1) for v in vals[:2]]
    out, booted = gpu.check_level_and_boot(gpu.stack(low), 3, gb)
    assert booted and out.level == gb.depth
    same_words(gpu, out, [gb.bootstrap(c) for c in low])
    # enough levels left: not bootstrapped, the handle shares the stack's storage
    st = gpu.stack(cts[:2])
    out, booted = gpu.check_level_and_boot(st, 2, gb)
    assert not booted and out.level == DEPTH - 3
    same_words(gpu, out, cts[:2])
    out.set_slots(4)
    assert st.slots == 4
    out.set_slots(8)


def test_errors_unchanged_for_stacks(ctx8):
    gpu, gb, vals, cts = ctx8
    wide = [gpu.encrypt(np.ones(16) * 0.5, 16, level=DEPTH - 4) for _ in range(2)]
    with pytest.raises(F.FheError) as e:
        gb.bootstrap(gpu.stack(wide))
    assert e.value.code == F.FHE_EINVAL
    top = [gpu.encrypt(np.ones(8) * 0.5, 8, level=DEPTH) for _ in range(2)]
    with pytest.raises(F.FheError) as e1:
        gb.bootstrap(top[0])
    with pytest.raises(F.FheError) as e2:
        gb.bootstrap(gpu.stack(top))
    assert e2.value.code == e1.value.code
