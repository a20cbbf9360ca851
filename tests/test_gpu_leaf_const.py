"""The constant terms of the rescaled Paterson-Stockmeyer leaves, folded into
the leaf-sum kernels (FHE_LEAF_CONST_FOLD) or added by one
add_const_inplace per leaf behind the rescale (0).  Either way the series is
word-identical to the CPU oracle's.

A Chebyshev series on [-1, 1] with seeded random coefficients, so every leaf has
a constant term: degree 70 and degree 250 (whose leaf-sum launches hold more than
four outputs, two groups of the MFMA kernels' tables), 1 and 5 stacked members,
both PS splits, at (logN 12, L 20, 40 bit) and (16, 12, 41).  The oracle's series
are computed once, in this process, and handed to the children as files.  Each
switch is read once per process, so each setting runs in a child of its own:

* default: the fold, in k_leaf_sums_fold with the six-digit rows; with the
  OpenFHE split no k_c0_op runs in the series;
* off: FHE_LEAF_CONST_FOLD=0; at least one k_c0_op runs;
* nosix / window / valu: the fold in k_leaf_sums_fold without the six-digit
  rows (FHE_LEAF_SIX=0), in k_leaf_sums_mfma (FHE_LEAF_FOLD=0) and in the VALU
  k_linear_sum_multi (FHE_MFMA=0)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pyoracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

CONTEXTS = ((12, 20, 40), (16, 12, 41))
DEGREES = (70, 250)
SPLITS = (1, 0)  # OpenFHE's, the engine's power-of-two split


def coefficients(deg):
    return np.random.default_rng(deg).normal(size=deg + 1) / (1 + np.arange(deg + 1))


def distinct_inputs(logn):
    return 2 if logn == 12 else 1


@pytest.fixture(scope='module')
def refs(tmp_path_factory):
    """the oracle's keys, inputs and outputs: secret / public / relin_<ctx>.npy,
    in_<ctx>_<d>.npy, out_<ctx>_<split>_<deg>_<d>.npy"""
    root = tmp_path_factory.mktemp('leaf_const')
    for ci, (logn, L, bits) in enumerate(CONTEXTS):
        orc = O.Context(logn, L, bits, 60, 3, seed=L + logn)
        np.save(root / f'secret_{ci}.npy', orc.secret_ntt())
        np.save(root / f'public_{ci}.npy', orc.public_key())
        np.save(root / f'relin_{ci}.npy', orc.relin_key())
        xs = []
        for d in range(distinct_inputs(logn)):
            ox = orc.encrypt(np.linspace(-1, 1, 16) * (1.0 - 0.25 * d), 16, 0)
            np.save(root / f'in_{ci}_{d}.npy', ox.data())
            xs.append(ox)
        for split in SPLITS:
            orc.set_ps_split(split)
            for deg in DEGREES:
                for d, ox in enumerate(xs):
                    out = orc.cheb(ox, coefficients(deg))
                    np.save(root / f'out_{ci}_{split}_{deg}_{d}.npy', out.data())
    return str(root)


CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import fhesort as F
mode, root = sys.argv[2], sys.argv[3]

class Keys:  # the oracle's keys, as load_keys_from reads them
    def __init__(self, ci):
        self.ci = ci
    def secret_ntt(self): return np.load(f'{root}/secret_{self.ci}.npy')
    def public_key(self): return np.load(f'{root}/public_{self.ci}.npy')
    def relin_key(self): return np.load(f'{root}/relin_{self.ci}.npy')

CONTEXTS = ((12, 20, 40), (16, 12, 41))
for ci, (logn, L, bits) in enumerate(CONTEXTS):
    gpu = F.Context(logn, L, bits, 60, 3, seed=L + logn, keygen=False)
    gpu.load_keys_from(Keys(ci))
    nd = 2 if logn == 12 else 1
    ins = [gpu.upload(np.load(f'{root}/in_{ci}_{d}.npy'), 0, 16) for d in range(nd)]
    for split in (1, 0):
        gpu.set_ps_split(split)
        for deg in (70, 250):
            c = np.random.default_rng(deg).normal(size=deg + 1) / (1 + np.arange(deg + 1))
            want = [np.load(f'{root}/out_{ci}_{split}_{deg}_{d}.npy') for d in range(nd)]
            for members in (1, 5):
                x = gpu.stack([ins[m % nd] for m in range(members)]) if members > 1 else ins[0]
                with F.KernelClock(gpu) as clk:
                    y = gpu.cheb(x, c)
                names = set(clk.stats)
                tag = f'logN={logn} split={split} degree={deg} x{members} {mode}'
                for m in range(members):
                    got = gpu.member(y, m) if members > 1 else y
                    assert np.array_equal(got.data(), want[m % nd]), f'{tag} member {m}'
                sums = sorted(k for k in names if k.startswith(('k_leaf_sums', 'k_linear_sum_multi')))
                assert sums, (tag, sorted(names))
                if mode in ('default', 'nosix'):
                    assert all(k.startswith('k_leaf_sums_fold<') for k in sums), (tag, sums)
                    if deg == 250:  # k_leaf_sums_fold<KS, NG>: two or more groups of four outputs
                        assert any(int(k.split(',')[1].strip(' >').split('>')[0]) >= 2 for k in sums), (tag, sums)
                elif mode == 'window':
                    assert all(k.startswith('k_leaf_sums_mfma<') for k in sums), (tag, sums)
                elif mode == 'valu':
                    assert all(k.startswith('k_linear_sum_multi<') for k in sums), (tag, sums)
                if split == 1:
                    c0 = [k for k in names if k.startswith('k_c0_op')]
                    assert (len(c0) >= 1) if mode == 'off' else not c0, (tag, sorted(names))
    print('ok', logn, flush=True)
print('ALLOK')
'''

SWITCHES = ('FHE_LEAF_CONST_FOLD', 'FHE_LEAF_SIX', 'FHE_LEAF_FOLD', 'FHE_MFMA')


def run_child(mode, root, **switches):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'), mode, root], env=env,
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'


def test_fold_default(refs):
    run_child('default', refs)


def test_fold_off(refs):
    run_child('off', refs, FHE_LEAF_CONST_FOLD='0')


def test_fold_without_six_digit_rows(refs):
    run_child('nosix', refs, FHE_LEAF_SIX='0')


def test_fold_window_kernel(refs):
    run_child('window', refs, FHE_LEAF_FOLD='0')


def test_fold_valu_kernel(refs):
    run_child('valu', refs, FHE_MFMA='0')
