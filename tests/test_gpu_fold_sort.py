"""DirectSort end to end with the constants folded into the HMult passes
(FHE_MUL_FOLD_CONST) and the rank's masked sums stacked (FHE_RANK_STACK_MASKS):
N = 8 and N = 16 at ring 2^12 (at N = 16 the rank has np < num_partition, so
vecRotsOptMany's j loop runs more than once), on 1 and 2 lanes with comparator
stacks of 1 (the single-batch path, mul_plain_sum), 3 (a narrow tile, chunks of
uneven size) and 32 (every batch of a lane in one chunk).  Every output must be
the CPU oracle's word for word and decrypt to the sorted input.  At these sizes
N^2 fits the ring's slots, so the rank has a single comparator batch; N = 64 has
two, and its sort with both in one stack (the batched masked sum) must give the
words of the sort that runs them one by one.  A child process with both
switches off must print the same digest of the outputs."""
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
digest = hashlib.sha256()
cfg = (3, 2, 2)
for N in (8, 16):
    depth, rots = F.size_parameters(N)
    orc = O.Context(12, depth, 40, 60, 3, seed=2025 + N)
    orc.gen_rotation_keys(rots)
    gpu = F.Context(12, depth, 40, 60, 3, seed=2025 + N, device=0, keygen=False)
    gpu.load_keys_from(orc, rots)
    x = np.random.default_rng(N).permutation(N) / N
    ox = orc.encrypt(x, N)
    want = orc.direct_sort(ox, N, rots, cfg).data()
    for lanes in (1, 2):
        for stack in (1, 3, 32):
            gpu.set_sort_lanes(lanes)
            gpu.set_sort_stack(stack)
            with F.KernelClock(gpu) as clk:
                out = gpu.direct_sort(gpu.from_oracle(ox), N, rots, cfg)
            what = f'N={N} lanes={lanes} stack={stack} {mode}'
            names = set(k.split('<')[0].split('@')[0] for k in clk.stats)
            # N^2 fits the 2,048 slots: one comparator batch, so never the batched masked sum
            assert 'k_mul_plain_sum_batches' not in names, (what, sorted(names))
            assert ('k_tensor_c' in names) == (mode == 'on'), (what, sorted(names))
            assert np.array_equal(out.data(), want), what
            err = float(np.max(np.abs(gpu.decrypt(out)[:N] - np.sort(x))))
            assert err < 0.01, (what, err)
            digest.update(out.data().tobytes())
    print('ok', N, flush=True)
# N = 64 has two comparator batches of 32 partitions at this ring: a stack of 32 forms both
# masked sums in one pass (one narrow tile), a stack of 1 runs them one by one through
# mul_plain_sum -- the same words (the oracle's sort at this size takes too long for a test)
N = 64
depth, rots = F.size_parameters(N)
gpu = F.Context(12, depth, 40, 60, 3, seed=64, device=0)
gpu.gen_rotation_keys(rots)
x = np.random.default_rng(N).permutation(N) / N
cx = gpu.encrypt(x, N)
gpu.set_sort_lanes(1)
outs = {}
for stack in (1, 32):
    gpu.set_sort_stack(stack)
    with F.KernelClock(gpu) as clk:
        outs[stack] = gpu.direct_sort(cx, N, rots, cfg).data()
    names = set(k.split('<')[0].split('@')[0] for k in clk.stats)
    assert ('k_mul_plain_sum_batches' in names) == (mode == 'on' and stack == 32), (N, stack, mode, sorted(names))
assert np.array_equal(outs[1], outs[32]), f'N=64 stack 1 against stack 32 {mode}'
digest.update(outs[32].tobytes())
print('DIGEST', digest.hexdigest())
print('ALLOK')
'''

_runs = {}


def run_child(mode, **switches):
    if mode not in _runs:
        env = {k: v for k, v in os.environ.items() if k not in ('FHE_MUL_FOLD_CONST', 'FHE_RANK_STACK_MASKS')}
        env.update(switches)
        r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'),
                            os.path.join(REPO, 'oracle'), mode], env=env, capture_output=True, text=True, timeout=280)
        assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
        _runs[mode] = [ln.split()[1] for ln in r.stdout.splitlines() if ln.startswith('DIGEST')][0]
    return _runs[mode]


OFF = dict(FHE_MUL_FOLD_CONST='0', FHE_RANK_STACK_MASKS='0')


def test_sort_with_folds_matches_oracle():
    run_child('on')


def test_sort_with_folds_switched_off_matches_oracle():
    run_child('off', **OFF)


def test_sort_same_words_either_way():
    assert run_child('on') == run_child('off', **OFF)
