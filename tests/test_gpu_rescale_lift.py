"""The lifted column pass of the rescale in both of its forms (INTEGRATION.md,
FHE_RESCALE_LIFT_LOOP): k_ntt_lift_loop, whose blocks load their tile of the
last limb once and loop over target limbs, and the per-limb k_ntt_fwd<.., 1, ..>.
Each switch is read once per process, so each setting runs in a child of its own:

* default: the loop runs where a launch keeps FHE_RESCALE_LIFT_MIN_BLOCKS
  (2048) blocks.  At ring 2^16 a 32-member rescale (64 x 16 tiles) loops, a
  one-member one (2 x 16 tiles) keeps the per-limb grid; the ring-2^12
  contexts never reach the threshold;
* off: FHE_RESCALE_LIFT_LOOP=0, the per-limb form everywhere;
* all: FHE_RESCALE_LIFT_MIN_BLOCKS=1, every launch of two or more limbs loops
  over all of them, so the small rings (64-point columns) and the interleaved
  classes (two limb runs per launch) run the loop as well.

Contexts: (logN 12, L 20, 40 bit), (12, 50, 41), whose prime classes
interleave, and (16, 12, 41).  Word for word against the CPU oracle:
rescale(ct * pt) at level 0, at a middle level and at two limbs (the only
target is q_0, the fp64 run is empty), mul_const_to with a constant that takes
the scaled lift, and linear_sum_to; with 1 and 5 stacked members, and 32 at
ring 2^16.  The kernel clock names the form that ran."""
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
LOOP, PER_LIMB = 'k_ntt_lift_loop<', 'k_ntt_fwd<'

def same(g, o, what):
    gi, oi = g.info(), o.info()
    assert (gi['level'], gi['limbs'], gi['scale']) == (oi['level'], oi['limbs'], oi['scale']), what
    assert np.array_equal(g.data(), o.data()), what

def limbs(rng, primes, n):
    return np.stack([rng.integers(0, int(q), size=n, dtype=np.uint64) for q in primes])

def lifts(stats):  # the lifted column passes among a clock's kernels: (looped, per-limb)
    col = [k for k in stats if k.startswith(LOOP) or (k.startswith(PER_LIMB) and k.split(',')[3].strip() == '1')]
    return any(k.startswith(LOOP) for k in col), any(k.startswith(PER_LIMB) for k in col)

for logn, L, bits in ((12, 20, 40), (12, 50, 41), (16, 12, 41)):
    tag = f'logN={logn} L={L} scale={bits} {mode}'
    orc = O.Context(logn, L, bits, 60, 3, seed=L + logn)
    gpu = F.Context(logn, L, bits, 60, 3, seed=L + logn, keygen=False)
    assert np.array_equal(orc.primes, gpu.primes)
    rng = np.random.default_rng(100 + L)
    n = orc.n
    seen = {}  # members -> [looped ran, per-limb ran]

    def rand_ct(level):
        pr = orc.primes[:orc.nq - level]
        data = np.stack([limbs(rng, pr, n), limbs(rng, pr, n)])
        return orc.ct_from(data, level, 16), gpu.upload(data, level, 16)

    def check(members, what, gpu_op, orc_op, distinct):
        # `distinct` random members, repeated to fill the stack
        with F.KernelClock(gpu) as clk:
            out = gpu_op()
        lo, pl = lifts(clk.stats)
        assert lo or pl, (what, sorted(clk.stats))
        s = seen.setdefault(members, [False, False])
        s[0] |= lo
        s[1] |= pl
        refs = [orc_op(d) for d in range(distinct)]
        for m in range(members):
            same(gpu.member(out, m) if members > 1 else out, refs[m % distinct], f'{what} member {m} {tag}')
        return lo, pl

    v = np.random.default_rng(7).uniform(-1, 1, 16)
    cases = [(1, lv) for lv in (0, L // 2, L - 1)] + [(5, lv) for lv in (0, L // 2, L - 1)]
    if logn == 16:
        cases.append((32, 0))
    for members, level in cases:
        distinct = min(members, 4)
        cts = [rand_ct(level) for _ in range(distinct)]
        st = gpu.stack([cts[m % distinct][1] for m in range(members)]) if members > 1 else cts[0][1]
        opt, gpt = orc.encode(v, 16, level), gpu.encode(v, 16, level)
        check(members, f'rescale(ct * pt) level {level} x{members}', lambda: gpu.mul_plain(st, gpt),
              lambda d: orc.mul_plain(cts[d][0], opt), distinct)
        if members == 32:
            continue
        check(members, f'mul_const_to level {level} x{members}', lambda: gpu.mul_const_to(st, -0.3718, level + 1),
              lambda d: orc.mul_const_to(cts[d][0], -0.3718, level + 1), distinct)
        if level < L - 1:  # inputs one level below the target's source level too
            lows = [rand_ct(level) for _ in range(distinct)]
            st2 = gpu.stack([lows[m % distinct][1] for m in range(members)]) if members > 1 else lows[0][1]
            cs = [0.61, -1.27]
            check(members, f'linear_sum_to level {level} x{members}',
                  lambda: gpu.linear_sum_to([st, st2], cs, level + 1),
                  lambda d: orc.linear_sum_to([cts[d][0], lows[d][0]], cs, level + 1), distinct)

    if mode == 'off':
        assert not any(s[0] for s in seen.values()), (tag, seen)
    elif mode == 'all':
        assert all(s[0] for s in seen.values()), (tag, seen)
    else:  # the threshold: 2048 blocks per launch
        assert seen[1] == [False, True] and seen[5] == [False, True], (tag, seen)
        if logn == 16:
            assert seen[32][0], (tag, seen)
    print('ok', tag, seen, flush=True)
print('ALLOK')
'''


def run_child(mode, **switches):
    env = dict(os.environ, **switches)
    for k in ('FHE_RESCALE_LIFT_LOOP', 'FHE_RESCALE_LIFT_MIN_BLOCKS'):
        if k not in switches:
            env.pop(k, None)
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'),
                        os.path.join(REPO, 'oracle'), mode], env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'


def test_default_threshold():
    run_child('default')


def test_per_limb_form():
    run_child('off', FHE_RESCALE_LIFT_LOOP='0')


def test_loop_everywhere():
    run_child('all', FHE_RESCALE_LIFT_MIN_BLOCKS='1')
