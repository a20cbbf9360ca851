#!/usr/bin/env python3
"""Bootstrap of one ciphertext against stacks of B on one MI355X, at BASELINE
config 4's context (ring 2^16, depth 40, scale 2^59, 4,096 slots, levelBudget
{5,5}; tests/k-way/KWaySort235Test.cpp:18-51).

Per B: the median wall time of fhe_bootstrap over --steps timed calls after
--warmup untimed ones (the stream drained before and after each call), divided
by B; and, from one more call under the kernel clock, the launches, the clocked
algorithmic bytes, the summed kernel time and the fraction of the 8 TB/s HBM peak
of the double-hoisted baby kernel (k_lt_inner for B = 1, k_lt_inner_mb for a
stack) and of the giants' key-switch sum.  B = 1 is the arm to beat.  The B are
interleaved inside every round so that all arms see the same box and clocks.

usage: boot_stack_bench.py [--stacks 1,2,4] [--steps 5] [--warmup 2] [--logn 16] [--slots 4096]
Prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'fhe-sorting_amd'))
import fhesort as F  # noqa: E402

HBM_PEAK = 8.0e12  # bytes/s, MI355X HBM3E spec peak (as bench.py)


def kernel_rows(stats, prefixes):
    rows = {}
    for name, prefix in prefixes.items():
        hit = {k: v for k, v in stats.items() if k.startswith(prefix)}
        ms, by = sum(v['ms'] for v in hit.values()), sum(v['bytes'] for v in hit.values())
        rows[name] = dict(kernels=sorted(hit), launches=sum(v['launches'] for v in hit.values()), ms=round(ms, 3),
                          bytes=int(by), frac_hbm_peak=round(by / (ms * 1e-3) / HBM_PEAK, 4) if ms > 0 else None)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--stacks', default='1,2,4')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--logn', type=int, default=16)
    ap.add_argument('--slots', type=int, default=4096)
    ap.add_argument('--depth', type=int, default=40)
    ap.add_argument('--budget', default='5,5')
    a = ap.parse_args()
    stacks = [int(v) for v in a.stacks.split(',')]
    budget = tuple(int(v) for v in a.budget.split(','))
    ctx = F.Context(a.logn, a.depth, 59, 60, 3, seed=2025)
    boot = F.Bootstrapper(ctx, a.slots, budget)
    rng = np.random.default_rng(a.slots)
    # one level left, as checkLevelAndBoot leaves a ciphertext
    cts = [ctx.encrypt(rng.uniform(-1, 1, a.slots), a.slots, level=a.depth - 1) for _ in range(max(stacks))]
    ins = {B: (cts[0] if B == 1 else ctx.stack(cts[:B])) for B in stacks}

    def once(B):
        ctx.sync()
        t0 = time.perf_counter()
        out = boot.bootstrap(ins[B])
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(a.warmup):
        for B in stacks:
            once(B)
    times = {B: [] for B in stacks}
    for _ in range(a.steps):
        for B in stacks:
            times[B].append(once(B)[0])
    res = {}
    for B in stacks:
        with F.KernelClock(ctx) as clk:
            out = boot.bootstrap(ins[B])
        single = B == 1
        rows = kernel_rows(clk.stats, {'lt_inner': 'k_lt_inner<' if single else 'k_lt_inner_mb<',
                                       'ks_inner_mk_sum': 'k_ks_inner_mk_sum<' if single else 'k_ks_inner_mk_sum_mb<'})
        clocked_ms = sum(v['ms'] for k, v in clk.stats.items() if not k.startswith('phase:'))
        med = statistics.median(times[B])
        res[str(B)] = dict(ms_per_call=round(med, 2), ms_per_ciphertext=round(med / B, 2),
                           min_ms=round(min(times[B]), 2), max_ms=round(max(times[B]), 2),
                           clocked_kernel_ms=round(clocked_ms, 2), level_out=out.level, **rows)
    one = res.get('1')
    if one:
        for B in stacks:
            res[str(B)]['per_ciphertext_vs_single'] = round(res[str(B)]['ms_per_ciphertext'] / one['ms_per_ciphertext'], 4)
    print(json.dumps(dict(logn=a.logn, depth=a.depth, slots=a.slots, budget=budget, boot_depth=boot.depth,
                          steps=a.steps, warmup=a.warmup, stacks=res)), flush=True)
    boot.close()
    ctx.close()


if __name__ == '__main__':
    main()
