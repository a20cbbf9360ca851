#!/usr/bin/env python3
"""Kernel clocks of the tiled tensor kernels, k_tensor_lex / k_tensor_win and the
stacked differences on one MI355X, this build against the PARENT commit's
library (--baseline-lib, never this build against itself).

One context at ring 2^16, depth 12 (13 limbs at level 0), dnum 3; B = 8 members,
P = 8 columns, K = 3 offsets, 10 operands per key for the lex and window
differences.  A child process (one library, read once per process through
FHE_LIB) calls each primitive --steps times after one untimed call under the
kernel clock and reports, per kernel, the clocked ms per launch.  The parent and
this build alternate, parent first, for --rounds rounds.  Per kernel the summary
gives both arms' round values, `spread_parent` = the largest minus the smallest
of the parent's rounds, `diff` = mean(new) - mean(parent), and `inside` = |diff|
<= spread_parent.

usage: kernel_bodies_bench.py --baseline-lib PATH [--rounds 3] [--steps 5] [--out FILE.jsonl]
"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'fhe-sorting_amd'))
FAMILY = ('k_tensor_cols', 'k_tensor_pairs', 'k_tensor_run', 'k_tensor_gather', 'k_tensor_lex', 'k_tensor_win', 'k_sub_')


def child(steps):
    import numpy as np
    import fhesort as F
    B, P, K, BL = 8, 8, 3, 10
    gpu = F.Context(16, 12, 40, 60, 3, seed=7)
    rng = np.random.default_rng(3)
    ct = lambda: gpu.encrypt(rng.uniform(-1, 1, 16), 16, 0)
    pt = lambda: gpu.encode(rng.uniform(-1, 1, 16), 16, 0)
    cts = [ct() for _ in range(32)]
    pts = [pt() for _ in range(BL)]
    sB = [gpu.stack(cts[i * B:(i + 1) * B]) for i in range(4)]
    sPB = gpu.stack([cts[i % 32] for i in range(P * B)])
    sKB = gpu.stack([cts[(i + 5) % 32] for i in range(K * B)])
    ops = [
        lambda: gpu.sub_add_plain_stacked(cts[0], cts[1:1 + B], pts[:B]),
        lambda: gpu.sub_pm_const_stacked(cts[0], cts[1:1 + B], 1.0 / 16),
        lambda: gpu.sub_offsets_stacked(cts[0], cts[1:1 + B], [-1, 0, 1]),
        lambda: gpu.sub_bounds_stacked(cts[0:1], cts[2:2 + B], [1.0 / 16]),
        lambda: gpu.sub_bounds_stacked(cts[0:2], cts[2:2 + B], [1.0 / 16, -1.0 / 16]),
        lambda: gpu.sub_lex_stacked(cts[0:3], cts[2:2 + 3 * BL], 1.0 / 16, pts[:BL]),
        lambda: gpu.sub_window_stacked(cts[0:2], cts[2:2 + 2 * BL], 1.0 / 16, mode=F.WIN_BETWEEN, order_a=cts[30],
                                       order_bs=cts[20:20 + BL], order_lo=cts[31]),
        lambda: gpu.sub_window_stacked(cts[0:2], cts[2:2 + 2 * BL], 1.0 / 16, mode=F.WIN_ROWS, order_a=cts[30],
                                       order_bs=cts[20:20 + BL], ps=pts[:BL]),
        lambda: gpu.mul_columns(sB[0], cts[8:8 + P]),
        lambda: gpu.mul_pairs(sB[0], sB[1], sPB, P),
        lambda: gpu.mul_pairs_const(sB[0], 1.0, sPB, P),
        lambda: gpu.mul_pairs_sub(sB[0], sB[1], sPB, P),
        lambda: gpu.mul_gather(sKB, sPB, P, K),
        lambda: gpu.mul_lex(sB[0], 1.0, sB[1], sB[2]),
        lambda: gpu.mul_sub_sub(sB[0], sB[1], sB[2], sB[3]),
    ]
    refused = []
    for i, op in enumerate(list(ops)):  # one untimed call each; a refused call (an FheError, no GPU fault) is left out
        try:
            op()
        except F.FheError as e:
            refused.append(f'op {i}: {e}')
            ops.remove(op)
    with F.KernelClock(gpu) as clk:
        for _ in range(steps):
            for op in ops:
                op()
    out = {k: {'launches': v['launches'], 'ms_per_launch': v['ms'] / v['launches']}
           for k, v in clk.stats.items() if k.startswith(FAMILY)}
    print(json.dumps({'lib': "the parent commit's libfhesort.so" if os.environ.get('FHE_LIB') else 'this build', 'steps': steps, 'refused': refused, 'kernels': out}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--baseline-lib', default=None)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(HERE, '..', 'profiles', 'kernel_bodies', 'kernel_clock.jsonl'))
    ap.add_argument('--child-timeout', type=int, default=240)
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.steps)
    if not a.baseline_lib:
        sys.exit('kernel_bodies_bench.py: --baseline-lib (the parent commit\'s libfhesort.so) is required')
    vals = {'parent': {}, 'new': {}}
    with open(a.out, 'w') as f:
        for r in range(1, a.rounds + 1):
            for arm in ('parent', 'new'):
                env = dict(os.environ)
                env.pop('FHE_LIB', None)
                if arm == 'parent':
                    env['FHE_LIB'] = os.path.abspath(a.baseline_lib)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', '--steps', str(a.steps)],
                                   env=env, capture_output=True, text=True, timeout=a.child_timeout)
                if p.returncode != 0:  # a fault ends the job: nothing more is started on the GPU
                    sys.exit(f'arm {arm} round {r} ended with {p.returncode}\n{p.stderr[-2000:]}')
                rec = json.loads(p.stdout.strip().splitlines()[-1])
                f.write(json.dumps({'arm': arm, 'round': r, **rec}) + '\n')
                f.flush()
                for k, v in rec['kernels'].items():
                    vals[arm].setdefault(k, []).append(v['ms_per_launch'])
        summary = {}
        for k in sorted(vals['parent']):
            p, n = vals['parent'][k], vals['new'].get(k, [])
            if not n:
                continue
            spread, diff = max(p) - min(p), sum(n) / len(n) - sum(p) / len(p)
            summary[k] = {'parent_ms': [round(x, 5) for x in p], 'new_ms': [round(x, 5) for x in n],
                          'spread_parent': round(spread, 5), 'diff': round(diff, 5), 'inside': abs(diff) <= spread}
        f.write(json.dumps({'summary': summary}) + '\n')
    for k, v in summary.items():
        print(k, v)


if __name__ == '__main__':
    main()
