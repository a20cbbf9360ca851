#!/usr/bin/env python3
"""Order-statistic select (fhe_direct_select) against the full index check, on one
MI355X at BASELINE config 3's context (N = 1024, ring 2^16, depth 39), from one
precomputed rank.

Arms:
  a  direct_select of the key for k in --ks targets (1, 31, 32, 256: one member,
     a full member, one target past it, nine members), and of P in --cols
     columns at k = --cols-k (31)
  b  the same under FHE_SELECT_FUSED=0 (one mul_plain_sum per column)
  c  the baseline, the PARENT commit's way to the same values: one
     direct_sort(mode=2) per column (every order statistic at once), on
     --baseline-lib -- the parent's library, never the code under test against
     itself.  Build it from a checkout of the parent (make -C fhe-sorting_amd
     lib/libfhesort.so) and pass its path; without it arm c is left out and
     nothing is concluded.

Every arm runs in a process of its own (the switch and the library are read once
per process); the arms alternate inside each of --rounds rounds.  A timing is one
call (arm c: the P calls) from a drained stream to fhe_sync; per process, the
median of --steps timings after --warmup untimed ones; per arm, the median of the
rounds' medians, and `spread` = the largest minus the smallest round median.
`separates`: the gap exceeds three times the larger of the two spreads (DESIGN.md
§5.7).  Every timed result is decrypted and compared with the plaintext order
statistics (max_abs_err).

One more run of arm a records, per k, the clocked time of the select's phases and
kernels (KernelClock), so the cost of one member's series at its narrow launch
shapes can be set against the index check's 32 stacked ones.

usage: select_bench.py [--ks 1,31,32,256] [--cols 1,8] [--cols-k 31] [--rounds 3] [--steps 3]
                       [--warmup 1] [--baseline-lib PATH] [--out FILE.jsonl] [--n 1024 --logn 16]
Appends one JSON line per process to --out (default profiles/select/select_bench.jsonl)
and prints the summary line.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'fhe-sorting_amd'))

NEW_SYMBOLS = ('fhe_direct_select', 'fhe_select_layout', 'fhe_pt_encode_select', 'fhe_mul_plain_sum_groups')


def sign_cfg(N):  # as bench.py
    return (3, 2, 2) if N <= 16 else (3, 3, 2) if N <= 128 else (3, 4, 2) if N <= 512 else (3, 5, 2)


def child(a):
    import ctypes
    import numpy as np
    import fhesort as F
    if a.child == 'c':  # the parent's library has none of the new entry points
        have = ctypes.CDLL(F.LIB_PATH)
        for s in NEW_SYMBOLS:
            if not hasattr(have, s):
                F._SIGS.pop(s, None)
    N, cfg = a.n, sign_cfg(a.n)
    depth, rots = F.size_parameters(N)
    ks = [int(v) for v in a.ks.split(',')]
    cols_list = [int(v) for v in a.cols.split(',')]
    ctx = F.Context(a.logn, depth, 40, 60, 3, seed=2025)
    ctx.gen_rotation_keys(rots)
    rng = np.random.default_rng(N)
    keyv = rng.permutation(N) / N
    colv = [keyv] + [rng.uniform(-1, 1, N) for _ in range(max(cols_list) - 1)]
    order = np.argsort(keyv)
    cols = [ctx.encrypt(v, N) for v in colv]
    rank = ctx.direct_sort(cols[0], N, rots, cfg, mode=1)
    ctx.sync()

    def targets(k):  # evenly spaced quantiles; k = 1: the median
        return [N // 2] if k == 1 else [int(t) for t in np.linspace(0, N - 1, k).astype(int)]

    def call(k, P):
        if a.child == 'c':  # the whole index check per column
            return [ctx.direct_sort(cols[p], N, rots, cfg, mode=2, rank=rank) for p in range(P)]
        return ctx.direct_select(None, targets(k), N, rots, cfg, cols=cols[:P], rank=rank)

    def err(out, k, P):
        if a.child == 'c':
            return float(max(np.max(np.abs(ctx.decrypt(o)[:N] - colv[p][order])) for p, o in enumerate(out)))
        t = targets(k)
        worst = 0.0
        for p, o in enumerate(out):
            dec = ctx.decrypt(o)
            worst = max(worst, float(np.max(np.abs(dec[:k] - colv[p][order][t]))),
                        float(np.max(np.abs(dec[k:]))) if k < N else 0.0)
        return worst

    def once(k, P):
        ctx.sync()
        t0 = time.perf_counter()
        out = call(k, P)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    res = dict(arm=a.child, round=a.round, N=N, logn=a.logn, depth=depth, lib=os.path.basename(F.LIB_PATH),
               fused=os.environ.get('FHE_SELECT_FUSED', '1'), steps=a.steps, warmup=a.warmup, cases={})
    # arm c computes every order statistic whatever k is: one case per column count
    cases = [(0, P) for P in sorted(set([1] + cols_list))] if a.child == 'c' else \
        [(k, 1) for k in ks] + [(a.cols_k, P) for P in cols_list if (a.cols_k, P) not in [(k, 1) for k in ks]]
    for k, P in cases:
        row = {}
        if a.child == 'clock':
            once(k, P)
            with F.KernelClock(ctx) as clk:
                out = call(k, P)
            for name, v in clk.stats.items():
                if name.startswith(('phase:select', 'k_mul_plain_sum_groups', 'k_select_slots')):
                    row[name] = dict(launches=v['launches'], ms=round(v['ms'], 4))
            row['members'] = F.select_layout(N, min(N, (1 << (a.logn - 1)) // N) * N, k)[0]
        else:
            for _ in range(a.warmup):
                once(k, P)
            ts = []
            for _ in range(a.steps):
                t, out = once(k, P)
                ts.append(t)
            row.update(ms=round(statistics.median(ts), 2), min_ms=round(min(ts), 2), max_ms=round(max(ts), 2))
        row['level_out'] = out[0].level
        row['max_abs_err'] = err(out, k, P)
        res['cases'][f'k{k}_P{P}'] = row
    print('RESULT ' + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ks', default='1,31,32,256')
    ap.add_argument('--cols', default='1,8')
    ap.add_argument('--cols-k', type=int, default=31)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--n', type=int, default=1024)
    ap.add_argument('--logn', type=int, default=16)
    ap.add_argument('--baseline-lib', default=None)
    ap.add_argument('--out', default=os.path.join(HERE, '..', 'profiles', 'select', 'select_bench.jsonl'))
    ap.add_argument('--child-timeout', type=int, default=240)
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--round', type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)

    def run(arm, rnd):
        env = dict(os.environ)
        env.pop('FHE_SELECT_FUSED', None)
        env.pop('FHE_LIB', None)
        if arm == 'b':
            env['FHE_SELECT_FUSED'] = '0'
        if arm == 'c':
            env['FHE_LIB'] = os.path.abspath(a.baseline_lib)
        cmd = [sys.executable, os.path.abspath(__file__), '--child', arm, '--round', str(rnd), '--ks', a.ks, '--cols',
               a.cols, '--cols-k', str(a.cols_k), '--steps', str(a.steps), '--warmup', str(a.warmup), '--n', str(a.n),
               '--logn', str(a.logn)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')), None)
        if r.returncode != 0 or line is None:  # stop here: nothing more is started after a failed process
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f'arm {arm} round {rnd} failed with status {r.returncode}')
        rec = json.loads(line[7:])
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(json.dumps(rec) + '\n')
        print(f'arm {arm} round {rnd}: ' + ', '.join(f'{c} {v.get("ms")}' for c, v in rec['cases'].items()), flush=True)
        return rec

    arms = ['a', 'b'] + (['c'] if a.baseline_lib else [])
    recs = {arm: [] for arm in arms}
    for rnd in range(a.rounds):
        for arm in arms:
            recs[arm].append(run(arm, rnd))
    clock = run('clock', 0)
    summary = dict(N=a.n, logn=a.logn, rounds=a.rounds, steps=a.steps, warmup=a.warmup, arms={}, clock=clock['cases'])
    for arm in arms:
        summary['arms'][arm] = {}
        for case in recs[arm][0]['cases']:
            meds = [r['cases'][case]['ms'] for r in recs[arm]]
            summary['arms'][arm][case] = dict(ms=round(statistics.median(meds), 2), spread=round(max(meds) - min(meds), 2),
                                              rounds=meds,
                                              max_abs_err=max(r['cases'][case]['max_abs_err'] for r in recs[arm]))
    if 'c' in arms:  # every select case against the index check of as many columns
        summary['select_vs_index_check'] = {}
        for case, row in summary['arms']['a'].items():
            base = summary['arms']['c'].get('k0_P' + case.split('_P')[1])
            if base:
                gap = base['ms'] - row['ms']
                summary['select_vs_index_check'][case] = dict(
                    select_ms=row['ms'], index_check_ms=base['ms'], fraction=round(row['ms'] / base['ms'], 4),
                    separates=bool(gap > 3 * max(row['spread'], base['spread'])))
    with open(a.out, 'a') as f:
        f.write(json.dumps(dict(summary=summary)) + '\n')
    print(json.dumps(summary), flush=True)


if __name__ == '__main__':
    main()
