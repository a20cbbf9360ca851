"""One-digit HMults (ell <= alpha): the closing row pass forms the own-digit key
product of the Q limbs below ell - 1 itself (k_ntt_fwd_row<5, ...>,
FHE_MULTAIL_OWN, default 1) and k_ntt_row_ks keeps only q_last and the special
primes.  Every setting must give the words of the CPU oracle.

Ring 2^16 (the fused path needs it), depth 12, dnum 3 (alpha = 5), in the tidy
40-bit context and in the 41-bit one whose prime classes interleave, so that
own-digit limbs of both classes occur.  Products run at ell = 2 (no Q limb but
q_0 and q_last), 3 (one more limb), alpha (the largest one-digit case) and
alpha + 1 (two digits: the accumulator path must be chosen), on stacks of 4, 5
(a partial block) and 16 members, with a stacked and with a broadcast second
operand, as a square, as mul_add with one and four summands (k_tensor_lin), a
raw summand (mul_add_raw), an added left operand (a_add) and the doubled left
operand of 2 T_i T_j, and inside a degree-70 Chebyshev series (whose
Paterson-Stockmeyer products are those calls at one- and two-digit levels;
FHE_MUL_FOLD_SCALARS, default 1, forms its a + a in the tensor pass).

The switches are read once per process, so each set runs in a child process:
the defaults, FHE_MULTAIL_OWN=0 FHE_MUL_FOLD_SCALARS=0 (the parent's paths: no
<5, ...> launch, the same words), and FHE_NTT_FP=0 (every limb integer class: the integer form of the new
mode)."""
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
mode, bits = sys.argv[3], int(sys.argv[4])
logn, L = 16, 12

def same(g, o, what):
    gi, oi = g.info(), o.info()
    assert (gi['level'], gi['limbs'], gi['scale']) == (oi['level'], oi['limbs'], oi['scale']), what
    assert np.array_equal(g.data(), o.data()), what

def limbs(rng, primes, n):
    return np.stack([rng.integers(0, int(q), size=n, dtype=np.uint64) for q in primes])

tag = f'logN={logn} L={L} scale={bits} {mode}'
orc = O.Context(logn, L, bits, 60, 3, seed=L + logn)
gpu = F.Context(logn, L, bits, 60, 3, seed=L + logn, keygen=False)
gpu.load_keys_from(orc, [])
assert np.array_equal(orc.primes, gpu.primes)
rng = np.random.default_rng(bits)
n, alpha = orc.n, orc.alpha
assert alpha == 5
fp = [int(q) < (1 << 41) for q in orc.primes[:orc.nq]]
if bits == 41 and mode != 'int':  # own-digit limbs of both classes below q_last at ell = alpha
    assert not fp[0] and any(fp[1:alpha - 1]) and not all(fp[1:alpha - 1]), fp

def clocked(fn):
    with F.KernelClock(gpu) as clk:
        r = fn()
    return set(clk.stats), r

def rand_ct(level):
    pr = orc.primes[:orc.nq - level]
    data = np.stack([limbs(rng, pr, n), limbs(rng, pr, n)])
    return orc.ct_from(data, level, 16), gpu.upload(data, level, 16)

def rows(names, m):
    return sorted(k for k in names if k.startswith(f'k_ntt_fwd_row<{m},'))

def check_forms(names, ell, what):
    own = ell <= alpha and mode != 'off'
    if own:
        assert rows(names, 5) and not rows(names, 3), (what, sorted(names))
        # k_ntt_row_ks keeps q_last and the special primes: no accumulator of a lower limb is made
        assert any(k.startswith('k_ntt_row_ks<1,') for k in names), (what, sorted(names))
    else:
        assert rows(names, 3) and not rows(names, 5), (what, sorted(names))
    if mode == 'int':
        assert all(k.split('@')[0].endswith('false>') for k in rows(names, 5) + rows(names, 3)), (what, sorted(names))

def same_gpu(g, r, what):
    gi, ri = g.info(), r.info()
    assert (gi['level'], gi['limbs'], gi['scale']) == (ri['level'], ri['limbs'], ri['scale']), what
    assert np.array_equal(g.data(), r.data()), what

# (a [+ a_add]) b + sum c_i x_i [+ raw] on a stack of B members (bcast: b one ciphertext).
# The oracle's Python surface has no mul_add and a summand joins the product before its
# rescale, so mul-then-add is another word; the reference of every member is the same call
# on that member alone -- one member never takes the fused relinearisation (asserted: no
# k_ntt_row_ks, no <5, ...>), the path the existing series tests pin to the oracle -- and,
# for a_add alone, the oracle's add then mul as well.
def mul_add_family(B, ell, bcast):
    X, Y = [g for _, g in xs], [g for _, g in ys]
    rot = lambda v: v[1:B] + v[:1]
    mem = {'a': X[:B], 'b': [Y[0]] * B if bcast else Y[:B], 's1': Y[:B], 's2': X[:B], 's3': rot(X), 's4': rot(Y)}
    st = {k: gpu.stack(v) for k, v in mem.items()}
    if bcast:
        st['b'] = Y[0]
    cases = (('lin1', ['s3'], [0.75], None, None), ('lin4', ['s1', 's2', 's3', 's4'], [0.5, -1.25, 2.0, -0.125], None, None),
             ('raw', [], [], 's3', None), ('lin1+a_add', ['s3'], [-1.0], None, 's4'), ('raw+a_add', [], [], 's3', 's4'),
             ('a_add', [], [], None, 's4'))
    for name, sx, cs, raw, aa in cases:
        what = f'{tag} ell={ell} mul_add {name} stack {B}{" broadcast" if bcast else ""}'
        pick = lambda d, k: None if k is None else d[k]
        names, out = clocked(lambda: gpu.mul_add(st['a'], st['b'], [st[k] for k in sx], cs, raw=pick(st, raw),
                                                 a_add=pick(st, aa)))
        check_forms(names, ell, what)
        if sx:
            assert any(k.startswith(f'k_tensor_lin<{len(sx)}>') for k in names), (what, sorted(names))
        for m in range(B):
            one = {k: v[m] for k, v in mem.items()}
            rn, r = clocked(lambda: gpu.mul_add(one['a'], one['b'], [one[k] for k in sx], cs, raw=pick(one, raw),
                                                a_add=pick(one, aa)))
            assert not rows(rn, 5) and not any(k.startswith('k_ntt_row_ks') for k in rn), (what, sorted(rn))
            same_gpu(gpu.member(out, m), r, f'{what} member {m}')
            if name == 'a_add' and m in (0, B - 1):
                o = orc.mul(orc.add(xs[m][0], ys[(m + 1) % B][0]), ys[0 if bcast else m][0])
                same(gpu.member(out, m), o, f'{what} member {m} against the oracle')

# every ell: stacks of 4 and 5 (a partial block); 16 (two full blocks) at the smallest
# and the largest one-digit ell (default switches); a stack of 5 by one broadcast
# ciphertext; a square
for ell in (2, 3, alpha, alpha + 1):
    level = L + 1 - ell
    sizes = (4, 5, 16) if ell in (2, alpha) and mode == 'on' else (4, 5)
    xs, ys = [rand_ct(level) for _ in range(max(sizes))], [rand_ct(level) for _ in range(max(sizes))]
    ref = [orc.mul(xs[m][0], ys[m][0]) for m in range(max(sizes))]
    for B in sizes:
        what = f'{tag} ell={ell} stack {B}'
        names, st = clocked(lambda: gpu.mul(gpu.stack([g for _, g in xs[:B]]), gpu.stack([g for _, g in ys[:B]])))
        check_forms(names, ell, what)
        for m in range(B):
            same(gpu.member(st, m), ref[m], f'{what} member {m}')
    what = f'{tag} ell={ell} broadcast'
    names, st = clocked(lambda: gpu.mul(gpu.stack([g for _, g in xs[:5]]), ys[0][1]))
    check_forms(names, ell, what)
    same(gpu.member(st, 0), ref[0], f'{what} member 0')
    for m in (1, 4):
        same(gpu.member(st, m), orc.mul(xs[m][0], ys[0][0]), f'{what} member {m}')
    if ell == alpha:
        what = f'{tag} ell={ell} square'
        names, st = clocked(lambda: gpu.square(gpu.stack([g for _, g in xs[:4]])))
        check_forms(names, ell, what)
        for m in (0, 3):
            same(gpu.member(st, m), orc.square(xs[m][0]), f'{what} member {m}')
    # mul_add with one and with four summands (k_tensor_lin), mul_add_raw (a raw summand),
    # a_add (an added left operand) and their combinations, on every stack size, and on a
    # stack of 5 by one broadcast ciphertext
    for B in sizes:
        mul_add_family(B, ell, False)
    mul_add_family(5, ell, True)
    # the doubled left operand of 2 T_i T_j (twice_prod's fold: a_add = a itself), also as
    # a square, where only the left operand doubles: no separate k_add, the oracle's words
    X5, Y5 = gpu.stack([g for _, g in xs[:5]]), gpu.stack([g for _, g in ys[:5]])
    for name, rhs, orhs in (('2ab', Y5, ys), ('2aa', X5, xs)):
        what = f'{tag} ell={ell} doubled {name}'
        names, st = clocked(lambda: gpu.mul_add(X5, rhs, a_add=X5))
        check_forms(names, ell, what)
        assert not any(k.split('@')[0] == 'k_add' for k in names), (what, sorted(names))
        for m in (0, 4):
            same(gpu.member(st, m), orc.mul(orc.add(xs[m][0], xs[m][0]), orhs[m][0]), f'{what} member {m}')
    # fewer than 4 members: the unfused path, whatever the digit count
    names, one = clocked(lambda: gpu.mul(xs[0][1], ys[0][1]))
    assert not rows(names, 5), (tag, ell, sorted(names))
    same(one, ref[0], f'{tag} ell={ell} single')

# a degree-70 series on a stack of 4 from level 5: its Paterson-Stockmeyer products
# (mul_add with summands, mul_add_raw, an added left operand) run at ell = 8 ... 2
if bits == 41 or mode == 'on':
    c = np.random.default_rng(70).normal(size=71) / (1 + np.arange(71))
    ox = orc.encrypt(np.linspace(-1, 1, 16), 16, 5)
    ref = orc.cheb(ox, c)
    names, st = clocked(lambda: gpu.cheb(gpu.stack([gpu.from_oracle(ox) for _ in range(4)]), c))
    for m in range(4):
        same(gpu.member(st, m), ref, f'cheb70 {tag} member {m}')
    assert rows(names, 3) and bool(rows(names, 5)) == (mode != 'off'), (tag, sorted(names))
    assert any(k.startswith('k_tensor_lin<') for k in names), (tag, sorted(names))
print('ALLOK')
'''


def run_child(mode, bits, **switches):
    env = dict(os.environ, **switches)
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'),
                        os.path.join(REPO, 'oracle'), mode, str(bits)], env=env, capture_output=True, text=True,
                       timeout=280)
    assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'


@pytest.mark.parametrize('bits', [40, 41])
def test_own_digit_tail_default(bits):
    run_child('on', bits)


def test_own_digit_tail_switched_off():
    run_child('off', 41, FHE_MULTAIL_OWN='0', FHE_MUL_FOLD_SCALARS='0')


def test_own_digit_tail_integer_form():
    run_child('int', 41, FHE_NTT_FP='0')
