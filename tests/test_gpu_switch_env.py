"""Kernel-form switches that ship but that no other GPU test sets
("every setting gives the same words").  Each is read once per
process, so each set runs in a child process of its own, one after the other:

* alt: FHE_MODUP_FP=1 (the fp64 ModUp, k_modup_fp, off by default),
  FHE_CONV_TPI=4 and FHE_MDFP_I32=0 (the fp64 ModDown + rescale with four
  targets per work item and double-pair sources), FHE_LEAF_SIX=0 (the leaf
  sums without the six-digit rows), FHE_KS_FUSE_INT=0 (integer-class targets
  through ModUp's per-run row passes and ks_inner beside the fused
  k_ntt_row_ks of the FP targets);
* int: FHE_NTT_FP=0 and FHE_MODDOWN_FP=0, the integer-only fallbacks;
* unfused: FHE_KS_FUSE=0 (no k_ntt_row_ks at ring 2^16: ModUp's row passes and
  k_ks_inner) and FHE_TENSOR_LIN=0 (no k_tensor_lin: mul_add's summands in a
  pass of their own);
* rows16 / rows1: FHE_PS_CHUNK=5 / 1 (the series' leaf sums in more passes than
  the default 32 leaves per pass takes; the counts are compared across the
  children) with FHE_NTT_TWL_ROWS=16 / 1 (the staged-twiddle argument of
  k_ntt_fwd_row / k_ntt_inv_row: every shuffle row pass, or not the two-row
  blocks of the 5-member stack).  alt and int assert the defaults these turn.

All run ModUp at full and partial digits, products and rotations at two
levels, a 5-member stacked product and a degree-70 Chebyshev series in a tidy
40-bit context, in the depth-50 41-bit context whose classes interleave and
whose fp64 conversion tables take the halfway-reduction form (MID = 1), and at
ring 2^16 with interleaved classes (tests/test_gpu_mixed_classes.py); every
result is word-identical to the CPU oracle, and the kernel clock shows that the
forms asked for are the ones that ran."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import fhesort as F
import pyoracle as O
mode = sys.argv[3]

def same(g, o, what):
    gi, oi = g.info(), o.info()
    assert (gi['level'], gi['limbs'], gi['scale']) == (oi['level'], oi['limbs'], oi['scale']), what
    assert np.array_equal(g.data(), o.data()), what

def limbs(rng, primes, n):
    return np.stack([rng.integers(0, int(q), size=n, dtype=np.uint64) for q in primes])

# (logN, L, scale bits), the two levels of the products and rotations (the stack
# runs at the second), the level the series starts from (it consumes 7)
for (logn, L, bits), levels, cheb_level in (((12, 20, 40), (0, 9), 9), ((12, 50, 41), (0, 40), 40),
                                            ((16, 12, 41), (0, 6), 5)):
    tag = f'logN={logn} L={L} scale={bits}'
    orc = O.Context(logn, L, bits, 60, 3, seed=L + logn)
    orc.gen_rotation_keys([1])
    gpu = F.Context(logn, L, bits, 60, 3, seed=L + logn, keygen=False)
    gpu.load_keys_from(orc, [1])
    assert np.array_equal(orc.primes, gpu.primes)
    rng = np.random.default_rng(L)
    n, alpha = orc.n, orc.alpha
    names = set()
    launches = {}

    def clocked(fn):
        with F.KernelClock(gpu) as clk:
            r = fn()
        names.update(clk.stats)
        launches.clear()
        launches.update({k: v['launches'] for k, v in clk.stats.items()})
        return set(clk.stats), r

    def rand_ct(level):
        pr = orc.primes[:orc.nq - level]
        data = np.stack([limbs(rng, pr, n), limbs(rng, pr, n)])
        return orc.ct_from(data, level, 16), gpu.upload(data, level, 16)

    for ell in sorted({L + 1, 2 * alpha, 2 * alpha - 5, alpha + 1, alpha, 7, 1}):  # full and partial digits
        if ell > L + 1:
            continue
        d = limbs(rng, orc.primes[:ell], n)
        assert np.array_equal(orc.modup(d), clocked(lambda: gpu.modup(d))[1]), f'modup {tag} ell={ell}'
    for level in levels:
        (oa, ga), (ob, gb) = rand_ct(level), rand_ct(level)
        same(clocked(lambda: gpu.mul(ga, gb))[1], orc.mul(oa, ob), f'mul {tag} level {level}')
        same(clocked(lambda: gpu.rotate(ga, 1))[1], orc.rotate(oa, 1), f'rotate {tag} level {level}')
    xs, ys = [rand_ct(levels[1]) for _ in range(5)], [rand_ct(levels[1]) for _ in range(5)]
    product, st = clocked(lambda: gpu.mul(gpu.stack([g for _, g in xs]), gpu.stack([g for _, g in ys])))
    for m in range(5):
        same(gpu.member(st, m), orc.mul(xs[m][0], ys[m][0]), f'stacked member {m} {tag}')
    c = np.random.default_rng(70).normal(size=71) / (1 + np.arange(71))
    ox = orc.encrypt(np.linspace(-1, 1, 16), 16, cheb_level)
    gx = gpu.from_oracle(ox)
    series, gy = clocked(lambda: gpu.cheb(gx, c))
    same(gy, orc.cheb(ox, c), f'cheb70 {tag}')
    # the series' leaf-sum passes (FHE_PS_CHUNK leaves each): the parent compares the counts
    print('LEAFPASSES', logn, L, sum(v for k, v in launches.items() if k.startswith(('k_leaf_sums', 'k_linear_sum'))),
          flush=True)

    def ran(prefix, among=None):
        return any(k.startswith(prefix) for k in (names if among is None else among))

    def twl_flags(among):
        """the staged-twiddle argument of k_ntt_fwd_row<MODE, FULL, TWL, FP> / k_ntt_inv_row<FULL, TWL, FP>"""
        out = []
        for k in among:
            if k.startswith(('k_ntt_fwd_row<', 'k_ntt_inv_row<')):
                args = k.split('@')[0].split('<')[1].rstrip('>').split(', ')
                out.append(args[-2] == 'true')
        return out

    if mode in ('alt', 'int'):  # the defaults of the switches the modes below turn
        assert ran('k_tensor_lin', series), (tag, sorted(series))
        if logn == 16:
            assert ran('k_ntt_row_ks', product), (tag, sorted(product))
            # a 5-member product: 10 segments, two rows per block, staged (rows <= 4);
            # one ciphertext: two segments, eight rows per block, not staged
            assert all(twl_flags(product)) and twl_flags(product), (tag, sorted(product))
            assert not all(twl_flags(names)), (tag, sorted(names))
    if mode == 'unfused':  # FHE_KS_FUSE=0, FHE_TENSOR_LIN=0
        assert not ran('k_tensor_lin'), (tag, sorted(names))
        assert not ran('k_ntt_row_ks'), (tag, sorted(names))
        assert ran('k_ks_inner', product), (tag, sorted(product))
    elif mode == 'rows16':  # FHE_NTT_TWL_ROWS=16: every shuffle row pass stages its twiddles
        if logn == 16:
            assert twl_flags(names) and all(twl_flags(names)), (tag, sorted(names))
    elif mode == 'rows1':  # FHE_NTT_TWL_ROWS=1: the two-row blocks of the 5-member stack do not
        if logn == 16:
            assert twl_flags(product) and not all(twl_flags(product)), (tag, sorted(product))
    elif mode == 'alt':
        assert ran('k_modup_fp<'), (tag, sorted(names))
        assert ran('k_moddown_rescale_fp<'), (tag, sorted(names))
        # k_moddown_rescale_fp<K, MID, TPI, I32>, k_modup_fp<sources, MID>
        assert all(', 4, 0>' in k for k in names if k.startswith('k_moddown_rescale_fp<')), (tag, sorted(names))
        if (logn, L, bits) == (12, 50, 41):
            assert ran('k_moddown_rescale_fp<13, 1, 4, 0>'), (tag, sorted(names))
            assert any(k.startswith('k_modup_fp<') and k.endswith(', 1>') for k in names), (tag, sorted(names))
        if logn == 16:  # FP targets fused, integer targets through ks_inner, in one product
            assert ran('k_ntt_row_ks', product) and ran('k_ks_inner', product), (tag, sorted(product))
    else:
        assert not any('_fp' in k for k in names), (tag, sorted(names))
        assert ran('k_moddown_rescale_convert'), (tag, sorted(names))
        # the NTT passes name their class as the last template argument
        # ("k_ntt_fwd<..., false>@phase"), the fused row pass as its second
        ntt = [k for k in names if k.startswith(('k_ntt_fwd', 'k_ntt_inv'))]
        assert ntt and all(k.split('@')[0].endswith('false>') for k in ntt), (tag, sorted(ntt))
        assert all(k.split(',')[1].strip() == '0' for k in names if k.startswith('k_ntt_row_ks<')), (tag, sorted(names))
    print('ok', tag, alpha, flush=True)
print('ALLOK')
'''


LEAF_PASSES = {}  # mode -> {(logN, L): leaf-sum launches of the degree-70 series}


def run_child(mode, **switches):
    env = dict(os.environ, **switches)
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'),
                        os.path.join(REPO, 'oracle'), mode], env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
    LEAF_PASSES[mode] = {(int(w[1]), int(w[2])): int(w[3])
                         for w in (ln.split() for ln in r.stdout.splitlines()) if w and w[0] == 'LEAFPASSES'}
    assert len(LEAF_PASSES[mode]) == 3, r.stdout[-2000:]


def test_alternative_kernel_forms():
    run_child('alt', FHE_MODUP_FP='1', FHE_CONV_TPI='4', FHE_MDFP_I32='0', FHE_LEAF_SIX='0', FHE_KS_FUSE_INT='0')


def test_integer_only_fallbacks():
    run_child('int', FHE_NTT_FP='0', FHE_MODDOWN_FP='0')


def test_unfused_key_switch_and_tensor():
    """FHE_KS_FUSE=0: ModUp's row passes and k_ks_inner instead of k_ntt_row_ks at
    ring 2^16; FHE_TENSOR_LIN=0: mul_add's summands in a pass of their own"""
    run_child('unfused', **SETS['unfused'])


SETS = {'unfused': dict(FHE_KS_FUSE='0', FHE_TENSOR_LIN='0'),
        'rows16': dict(FHE_PS_CHUNK='5', FHE_NTT_TWL_ROWS='16'),
        'rows1': dict(FHE_PS_CHUNK='1', FHE_NTT_TWL_ROWS='1')}


def test_chunks_of_five_and_every_row_staged():
    """FHE_PS_CHUNK=5 with FHE_NTT_TWL_ROWS=16 (every shuffle row pass stages its twiddles)"""
    run_child('rows16', **SETS['rows16'])


def test_chunks_of_one_and_one_row_staged():
    """FHE_PS_CHUNK=1 with FHE_NTT_TWL_ROWS=1 (the 5-member stack's two-row blocks stage none)"""
    run_child('rows1', **SETS['rows1'])


def test_leaf_passes_grow_as_chunks_shrink():
    """FHE_PS_CHUNK=1 and 5: the degree-70 series' leaf sums take one pass per leaf,
    and several passes of at most five leaves, against the default's 32 leaves
    per pass (counted in the integer-only child, whose switches leave the
    series' passes alone); all three gave the oracle's words in the tests above"""
    if 'int' not in LEAF_PASSES:  # this test alone: the children it compares
        run_child('int', FHE_NTT_FP='0', FHE_MODDOWN_FP='0')
    for mode in ('rows16', 'rows1'):
        if mode not in LEAF_PASSES:
            run_child(mode, **SETS[mode])
    for key, base in LEAF_PASSES['int'].items():
        five, one = LEAF_PASSES['rows16'][key], LEAF_PASSES['rows1'][key]
        assert 1 <= base <= five < one and base < one, (key, base, five, one)
        # a pass of FHE_PS_CHUNK=5 takes at most five leaves: never one pass for them all
        assert five >= max(2, -(-one // 5)), (key, five, one)
