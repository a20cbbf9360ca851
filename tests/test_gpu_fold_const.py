"""Constants folded into an HMult's passes (Engine::mul_add's a_const and
out_const, FHE_MUL_FOLD_CONST, default 1): a_const is added to the left
operand's c0 as the tensor pass loads it (k_tensor_c, k_tensor_lin_c); out_const
joins d0 there as K q_last on the limbs below the last, which the HMult tail --
the accumulator form k_ntt_fwd_row<3, ...>, the one-digit <5, ...> and the
unfused one alike -- turns into + K on the result's c0.  Both must give the
words of add_const -> mul_add -> add_const.

Two contexts, dnum 3, q_0 60 bits and the rest 40 (both prime classes at every
level): ring 2^16, depth 8 (alpha = 3), where stacks of 4 and 5 take the fused
relinearisation -- ell = 3 <= alpha closes with <5, ...>, ell = 5 with
<3, ...> -- and a single ciphertext the unfused tail; and ring 2^12, depth 8,
whose tail is always ntt_forward_multail without the own-digit form (4-point
and 256-point row passes differ in their store loops).  On stacks of 1, 4 and
5, with b per member and broadcast: a plain product, a square (the constant
joins the left operand only), with a_add, with 1 and 4 summands, with a raw
summand; constants 0, -1.0 and 3e7 (K = c 2^40 > 2^62, so its SConst has
sh > 0).  An a below b's level must take the fallback (add_const first).

The switch is read once per process, so the checks run in two child processes,
FHE_MUL_FOLD_CONST unset and 0.  Each compares every folded call with the
explicit three-step reference on the GPU and a sample with the CPU oracle, the
launch clock shows that the folded arm ran no k_c0_op / k_add_scalar (and the
switched-off arm did), and the two children's output digests must be equal."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

CHILD = r'''
import hashlib
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import fhesort as F
import pyoracle as O
mode = sys.argv[3]
L = 8
BIG = 3.0e7
digest = hashlib.sha256()

def limbs(rng, primes, n):
    return np.stack([rng.integers(0, int(q), size=n, dtype=np.uint64) for q in primes])

def same_gpu(gpu, g, r, B, what):  # a stack downloads member by member; returns g's words
    gi, ri = g.info(), r.info()
    assert (gi['level'], gi['limbs'], gi['scale']) == (ri['level'], ri['limbs'], ri['scale']), what
    mem = lambda c: np.stack([gpu.member(c, m).data() for m in range(B)])
    w = mem(g)
    assert np.array_equal(w, mem(r)), what
    return w

def same(g, o, what):
    gi, oi = g.info(), o.info()
    assert (gi['level'], gi['limbs'], gi['scale']) == (oi['level'], oi['limbs'], oi['scale']), what
    assert np.array_equal(g.data(), o.data()), what

SCALAR = ('k_c0_op', 'k_add_scalar')

def run(logn):
    orc = O.Context(logn, L, 40, 60, 3, seed=L + logn)
    gpu = F.Context(logn, L, 40, 60, 3, seed=L + logn, keygen=False)
    gpu.load_keys_from(orc, [])
    n, alpha = orc.n, orc.alpha
    assert alpha == 3
    rng = np.random.default_rng(logn)
    fused_ring = logn == 16

    def rand_ct(level):
        pr = orc.primes[:orc.nq - level]
        data = np.stack([limbs(rng, pr, n), limbs(rng, pr, n)])
        return orc.ct_from(data, level, 16), gpu.upload(data, level, 16)

    def clocked(fn):
        with F.KernelClock(gpu) as clk:
            r = fn()
        return set(k.split('<')[0].split('@')[0] for k in clk.stats), set(clk.stats), r

    def rows(full, m):
        return [k for k in full if k.startswith(f'k_ntt_fwd_row<{m},')]

    # the product with its constants folded against the three explicit steps
    def check(what, a, b, xs, cs, raw, a_add, ca, co, fallback=False, ell=None, B=1):
        names, full, out = clocked(lambda: gpu.mul_add_const(a, b, xs, cs, raw=raw, a_add=a_add, a_const=ca,
                                                             out_const=co))
        left = a if a_add is None else gpu.add(a, a_add)
        left = gpu.add_const(left, ca)
        # a square multiplies the sum by the unchanged operand
        ref = gpu.add_const(gpu.mul_add(left, b, xs, cs, raw=raw), co)
        digest.update(same_gpu(gpu, out, ref, B, what).tobytes())
        scal = [k for k in SCALAR if k in names]
        if mode == 'on' and not fallback:
            assert not scal, (what, sorted(full))
            # the tensor form with constants exactly when there is one to fold
            assert (('k_tensor_c' in names or 'k_tensor_lin_c' in names) == (ca != 0.0 or co != 0.0)), (what, sorted(full))
        elif ca != 0.0:
            assert 'k_c0_op' in names, (what, sorted(full))
        if mode == 'off' and co != 0.0:
            assert 'k_add_scalar' in names, (what, sorted(full))
        if ell is not None and fused_ring and B >= 4:  # the closing row form the case is meant for
            own = ell <= alpha
            assert bool(rows(full, 5)) == own and bool(rows(full, 3)) == (not own), (what, sorted(full))
        elif ell is not None:  # the accumulator tail (ring 2^12: another row-pass shape of the same mode)
            assert not rows(full, 5) and (not fused_ring or rows(full, 3)), (what, sorted(full))
        return out

    consts = [(-1.0, 0.0), (0.0, -1.0), (BIG, -1.0), (-1.0, BIG), (0.0, 0.0), (-BIG, BIG)]
    for ell in (3, 5):  # one digit (<= alpha) and two
        level = L + 1 - ell
        xs_, ys_ = [rand_ct(level) for _ in range(5)], [rand_ct(level) for _ in range(5)]
        X, Y = [g for _, g in xs_], [g for _, g in ys_]
        rot = lambda v, B: v[1:B] + v[:1]
        ci = 0
        for B in (1, 4, 5):
            for bcast in (False, True):
                if B == 1 and bcast:
                    continue
                st = lambda v: v[0] if B == 1 else gpu.stack(v[:B])
                a, b = st(X), (Y[0] if bcast else st(Y))
                s1, s2, s3, s4 = st(Y), st(rot(X, B) if B > 1 else [X[1]]), st(rot(Y, B) if B > 1 else [Y[1]]), st(X)
                shapes = (('plain', b, [], [], None, None), ('a_add', b, [], [], None, s3),
                          ('lin1', b, [s2], [0.75], None, None), ('lin4', b, [s1, s2, s3, s4], [0.5, -1.25, 2.0, -0.125], None, None),
                          ('raw', b, [], [], s2, None), ('raw+a_add', b, [], [], s3, s2),
                          ('lin1+a_add', b, [s3], [-1.0], None, s2))
                if not bcast:
                    shapes += (('square', a, [], [], None, None), ('square+lin1', a, [s1], [0.5], None, None))
                for name, bb, sx, cs, raw, aa in shapes:
                    # every shape with both constants at once, and in turn with each constant pair
                    for ca, co in ((-1.0, BIG) if ci % 2 else (BIG, -1.0), consts[ci % len(consts)]):
                        what = f'logN={logn} ell={ell} stack {B}{" broadcast" if bcast else ""} {name} a_const={ca} out_const={co} {mode}'
                        out = check(what, a, bb, sx, cs, raw, aa, ca, co, ell=ell, B=B)
                    ci += 1
                # the oracle's words for the constants alone, first and last member
                for m in sorted({0, B - 1}):
                    for ca, co in ((-1.0, BIG), (BIG, -1.0)):
                        g = gpu.mul_add_const(a, b, a_const=ca, out_const=co)
                        o = orc.add_const(orc.mul(orc.add_const(xs_[m][0], ca), ys_[0 if bcast else m][0]), co)
                        same(gpu.member(g, m) if B > 1 else g, o, f'logN={logn} ell={ell} stack {B} member {m} oracle {ca} {co}')
                    if not bcast:
                        g = gpu.mul_add_const(a, a, a_const=-1.0, out_const=-1.0)
                        o = orc.add_const(orc.mul(orc.add_const(xs_[m][0], -1.0), xs_[m][0]), -1.0)
                        same(gpu.member(g, m) if B > 1 else g, o, f'logN={logn} ell={ell} stack {B} member {m} oracle square')
    # a below b's level: level-adjusted inside the product, so the constant is formed first
    lo = [rand_ct(2) for _ in range(4)]
    hi = [rand_ct(4) for _ in range(4)]
    for B in (1, 4):
        a = lo[0][1] if B == 1 else gpu.stack([g for _, g in lo])
        b = hi[0][1] if B == 1 else gpu.stack([g for _, g in hi])
        out = check(f'logN={logn} fallback stack {B} {mode}', a, b, [], [], None, None, -1.0, BIG, fallback=True, B=B)
        o = orc.add_const(orc.mul(orc.add_const(lo[0][0], -1.0), hi[0][0]), BIG)
        same(gpu.member(out, 0) if B > 1 else out, o, f'logN={logn} fallback stack {B} oracle')
        # the other way round (b adjusted, a not) folds
        check(f'logN={logn} b adjusted stack {B} {mode}', b, a, [], [], None, None, BIG, -1.0, B=B)
    # a Chebyshev series whose Paterson-Stockmeyer nodes and T_2i use both constants
    c = np.random.default_rng(70).normal(size=71) / (1 + np.arange(71))
    ox = orc.encrypt(np.linspace(-1, 1, 16), 16, 0)
    names, full, stc = clocked(lambda: gpu.cheb(gpu.stack([gpu.from_oracle(ox) for _ in range(4)]), c))
    ref = orc.cheb(ox, c)
    for m in (0, 3):
        same(gpu.member(stc, m), ref, f'cheb70 logN={logn} member {m} {mode}')
    digest.update(np.stack([gpu.member(stc, m).data() for m in range(4)]).tobytes())
    print('ok', logn, flush=True)

for logn in (12, 16):
    run(logn)
print('DIGEST', digest.hexdigest())
print('ALLOK')
'''

_runs = {}


def run_child(mode, **switches):
    if mode not in _runs:
        env = {k: v for k, v in os.environ.items() if k != 'FHE_MUL_FOLD_CONST'}
        env.update(switches)
        r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'),
                            os.path.join(REPO, 'oracle'), mode], env=env, capture_output=True, text=True, timeout=280)
        assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
        _runs[mode] = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith('DIGEST')][0]
    return _runs[mode]


def test_fold_const_default():
    run_child('on')


def test_fold_const_switched_off():
    run_child('off', FHE_MUL_FOLD_CONST='0')


def test_fold_const_same_words_either_way():
    assert run_child('on') == run_child('off', FHE_MUL_FOLD_CONST='0')
