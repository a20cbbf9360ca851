"""The masked sums of several batches over one list of ciphertexts in one pass
(Engine::mul_plain_sum_batches, k_mul_plain_sum_batches; FHE_RANK_STACK_MASKS,
default 1): member b must be mul_plain_sum(cts, pts[b]) word for word.

Ring 2^11, depth 4, dnum 3.  A thread of the kernel keeps plain_sum_tile() = 4
batches, so nb = 1, 3 (a narrow only tile), 5 (a full and a narrow tile) and 9
(two full, one narrow); 1, 4, 5 and 33 terms (33 crosses LIN_MAX = 32: a second,
accumulating launch).  At the context's top, ell = 5, the launch has 4 x 5
coefficient-block x limb tiles -- no multiple of 8, the plain 3-d grid -- and at
ell = 2 it has 8, the XCD-grouped flat grid.  Ciphertexts and plaintexts are
random words below each prime; one case with encoded plaintexts is compared
with the CPU oracle.  The switch is read once per process: a child process with
FHE_RANK_STACK_MASKS=0 must print the same digest of every result, and the
launch clock must show the new kernel only with the switch on."""
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
logn, L = 11, 4
digest = hashlib.sha256()
orc = O.Context(logn, L, 40, 60, 3, seed=7)
gpu = F.Context(logn, L, 40, 60, 3, seed=7, keygen=False)
gpu.load_keys_from(orc, [])
n = orc.n
rng = np.random.default_rng(11)
assert F.lib().fhe_plain_sum_tile() == 4

def limbs(primes):
    return np.stack([rng.integers(0, int(q), size=n, dtype=np.uint64) for q in primes])

def words(g, B):  # a stack downloads member by member
    return np.stack([gpu.member(g, m).data() for m in range(B)])

def same_gpu(g, r, B, what):
    gi, ri = g.info(), r.info()
    assert (gi['level'], gi['limbs'], gi['scale']) == (ri['level'], ri['limbs'], ri['scale']), what
    w = words(g, B)
    assert np.array_equal(w, words(r, B)), what
    return w

M, NB = 33, 9
for level in (0, L - 1):  # ell = 5 (20 tiles) and ell = 2 (8 tiles)
    pr = orc.primes[:orc.nq - level]
    assert (n // 512 * len(pr)) % 8 == (0 if level else 4)
    cts = [gpu.upload(np.stack([limbs(pr), limbs(pr)]), level, 16) for _ in range(M)]
    pts = [[gpu.upload_pt(limbs(pr), level, 16) for _ in range(M)] for _ in range(NB)]
    for nb in (1, 3, 5, 9):
        for m in (1, 4, 5, 33):
            what = f'level {level} nb {nb} terms {m} {mode}'
            gpu.reset_counters()
            with F.KernelClock(gpu) as clk:
                out = gpu.mul_plain_sum_batches(cts[:m], [row[:m] for row in pts[:nb]])
            booked = gpu.counters()
            names = set(k.split('@')[0] for k in clk.stats)
            assert ('k_mul_plain_sum_batches' in names) == (mode == 'on'), (what, sorted(names))
            assert ('k_mul_plain_sum' in names) == (mode == 'off'), (what, sorted(names))
            if mode == 'on':
                st = clk.stats[[k for k in clk.stats if k.split('@')[0] == 'k_mul_plain_sum_batches'][0]]
                assert st['launches'] == (m + 31) // 32, (what, st)
            gpu.reset_counters()
            ref = gpu.stack([gpu.mul_plain_sum(cts[:m], row[:m]) for row in pts[:nb]])
            assert booked == gpu.counters(), (what, booked, gpu.counters())
            digest.update(same_gpu(out, ref, nb, what).tobytes())

# encoded plaintexts against the oracle's masked sums
vals = [rng.uniform(-1, 1, 16) for _ in range(4)]
masks = [[(rng.uniform(size=16) < 0.5).astype(np.float64) for _ in range(4)] for _ in range(3)]
oc = [orc.encrypt(v, 16) for v in vals]
out = gpu.mul_plain_sum_batches([gpu.from_oracle(c) for c in oc], [[gpu.encode(mk, 16, 0) for mk in row] for row in masks])
for b in range(3):
    o = orc.mul_plain_sum(oc, [orc.encode(mk, 16, 0) for mk in masks[b]])
    g = gpu.member(out, b)
    assert np.array_equal(g.data(), o.data()), f'oracle batch {b} {mode}'
digest.update(words(out, 3).tobytes())
print('DIGEST', digest.hexdigest())
print('ALLOK')
'''

_runs = {}


def run_child(mode, **switches):
    if mode not in _runs:
        env = {k: v for k, v in os.environ.items() if k != 'FHE_RANK_STACK_MASKS'}
        env.update(switches)
        r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'),
                            os.path.join(REPO, 'oracle'), mode], env=env, capture_output=True, text=True, timeout=280)
        assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
        _runs[mode] = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith('DIGEST')][0]
    return _runs[mode]


def test_mask_batches_default():
    run_child('on')


def test_mask_batches_switched_off():
    run_child('off', FHE_RANK_STACK_MASKS='0')


def test_mask_batches_same_words_either_way():
    assert run_child('on') == run_child('off', FHE_RANK_STACK_MASKS='0')
