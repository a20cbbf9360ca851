#!/usr/bin/env python3
"""Record sort (fhe_direct_sort_columns) against one index check per column, on
one MI355X at BASELINE config 3's context (N = 1024, ring 2^16, depth 39).

Arms, for P in --cols payload columns applied to one fixed rank:
  a  one direct_sort_columns call (k_tensor_cols, k_sum_member_groups)
  b  the same under FHE_SORT_COLS_FUSED=0 (P broadcast products, per-group sums)
  c  the baseline: P calls of direct_sort(mode=2), on --baseline-lib -- the
     PARENT commit's library, never the code under test against itself.  Build it
     from a checkout of the parent (make -C fhe-sorting_amd lib/libfhesort.so) and
     pass its path; without it arm c is left out and nothing is concluded.

Every arm runs in a process of its own (the switch and the library are read once
per process); the arms alternate inside each of --rounds rounds.  A timing is one
call (arm c: the P calls) from a drained stream to fhe_sync; per process, the
median of --steps timings after --warmup untimed ones; per arm, the median of the
rounds' medians, and `spread` = the largest minus the smallest round median (the
same-setting spread).  `separates` is the repository's criterion (DESIGN.md
§5.7): the gap exceeds three times the larger of the two spreads.

Also recorded, from one more run of arm a: the two kernels' launches, clocked
time, model bytes and achieved fraction of the 8 TB/s HBM peak (KernelClock), and
the peak pool bytes per P (pool_stats of a fresh one-lane context, P ascending;
each of two lanes holds at most this much).

usage: sort_columns_bench.py [--cols 1,2,4,8] [--rounds 3] [--steps 3] [--warmup 1]
                             [--baseline-lib PATH] [--out FILE.jsonl] [--n 1024 --logn 16]
Appends one JSON line per process to --out and prints the summary line.
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

HBM_PEAK = 8.0e12  # bytes/s, MI355X HBM3E spec peak (as bench.py)
NEW_SYMBOLS = ('fhe_direct_sort_columns', 'fhe_set_sort_column_members', 'fhe_mul_columns',
               'fhe_ct_sum_member_groups')


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
    cols_list = [int(v) for v in a.cols.split(',')]
    ctx = F.Context(a.logn, depth, 40, 60, 3, seed=2025)
    ctx.gen_rotation_keys(rots)
    rng = np.random.default_rng(N)
    keyv = rng.permutation(N) / N
    colv = [rng.uniform(-1, 1, N) for _ in range(max(cols_list))]
    order = np.argsort(keyv)
    key = ctx.encrypt(keyv, N)
    cols = [ctx.encrypt(v, N) for v in colv]
    rank = ctx.direct_sort(key, N, rots, cfg, mode=1)
    ctx.sync()
    live_before = None
    if a.child == 'mem':
        # a fresh context (same seed: same keys) that has not run constructRank, so
        # that its pool's peak is the column call's own
        inf, words = rank.info(), rank.data()
        col_words = [c.data() for c in cols]
        del key, cols, rank
        ctx.close()
        ctx = F.Context(a.logn, depth, 40, 60, 3, seed=2025)
        ctx.gen_rotation_keys(rots)
        ctx.set_sort_lanes(1)
        rank = ctx.upload(words, inf['level'], inf['slots'], inf['scale'])
        cols = [ctx.upload(w, 0, N) for w in col_words]
        ctx.sync()
        live_before = ctx.pool_stats()['live']

    def call(P):
        if a.child == 'c':
            return [ctx.direct_sort(cols[p], N, rots, cfg, mode=2, rank=rank) for p in range(P)]
        return ctx.direct_sort_columns(None, cols[:P], N, rots, cfg, rank=rank)

    def once(P):
        ctx.sync()
        t0 = time.perf_counter()
        out = call(P)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    res = dict(arm=a.child, round=a.round, N=N, logn=a.logn, depth=depth, lib=os.path.basename(F.LIB_PATH),
               fused=os.environ.get('FHE_SORT_COLS_FUSED', '1'), steps=a.steps, warmup=a.warmup, cols={})
    for P in sorted(cols_list):
        row = {}
        if a.child == 'mem':
            _, out = once(P)
            row['peak_pool_bytes'] = ctx.pool_stats()['peak']
            row['live_before_bytes'] = live_before  # keys and inputs: the call's working set is the difference
        elif a.child == 'clock':
            once(P)
            with F.KernelClock(ctx) as clk:
                out = call(P)
            for name in ('k_tensor_cols', 'k_sum_member_groups'):
                hit = [v for k, v in clk.stats.items() if k.startswith(name)]
                ms, by = sum(v['ms'] for v in hit), sum(v['bytes'] for v in hit)
                row[name] = dict(launches=sum(v['launches'] for v in hit), ms=round(ms, 4), bytes=int(by),
                                 frac_hbm_peak=round(by / (ms * 1e-3) / HBM_PEAK, 4) if ms > 0 else None)
        else:
            for _ in range(a.warmup):
                once(P)
            ts = []
            for _ in range(a.steps):
                t, out = once(P)
                ts.append(t)
            row.update(ms=round(statistics.median(ts), 2), min_ms=round(min(ts), 2), max_ms=round(max(ts), 2))
        row['level_out'] = out[0].level
        row['max_abs_err'] = float(max(np.max(np.abs(ctx.decrypt(o)[:N] - colv[p][order])) for p, o in enumerate(out)))
        res['cols'][str(P)] = row
    print('RESULT ' + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cols', default='1,2,4,8')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--n', type=int, default=1024)
    ap.add_argument('--logn', type=int, default=16)
    ap.add_argument('--baseline-lib', default=None)
    ap.add_argument('--out', default=None)
    ap.add_argument('--child-timeout', type=int, default=240)
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--round', type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)

    def run(arm, rnd):
        env = dict(os.environ)
        env.pop('FHE_SORT_COLS_FUSED', None)
        env.pop('FHE_LIB', None)
        if arm == 'b':
            env['FHE_SORT_COLS_FUSED'] = '0'
        if arm == 'c':
            env['FHE_LIB'] = os.path.abspath(a.baseline_lib)
        cmd = [sys.executable, os.path.abspath(__file__), '--child', arm, '--round', str(rnd), '--cols', a.cols,
               '--steps', str(a.steps), '--warmup', str(a.warmup), '--n', str(a.n), '--logn', str(a.logn)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')), None)
        if r.returncode != 0 or line is None:  # stop here: nothing more is started after a failed process
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f'arm {arm} round {rnd} failed with status {r.returncode}')
        rec = json.loads(line[7:])
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'a') as f:
                f.write(json.dumps(rec) + '\n')
        print(f'arm {arm} round {rnd}: ' + ', '.join(f'P={P} {v.get("ms")}' for P, v in rec['cols'].items()), flush=True)
        return rec

    arms = ['a', 'b'] + (['c'] if a.baseline_lib else [])
    recs = {arm: [] for arm in arms}
    for rnd in range(a.rounds):
        for arm in arms:
            recs[arm].append(run(arm, rnd))
    clock, mem = run('clock', 0), run('mem', 0)
    summary = dict(N=a.n, logn=a.logn, rounds=a.rounds, steps=a.steps, warmup=a.warmup, cols={})
    for P in sorted(int(v) for v in a.cols.split(',')):
        row = {}
        for arm in arms:
            meds = [r['cols'][str(P)]['ms'] for r in recs[arm]]
            row[arm] = dict(ms=round(statistics.median(meds), 2), spread=round(max(meds) - min(meds), 2), rounds=meds)
        for x, y in (('a', 'c'), ('b', 'a')):  # x faster than y by more than 3 x the larger spread?
            if x in row and y in row:
                gap = row[y]['ms'] - row[x]['ms']
                row[f'{x}_beats_{y}'] = dict(gap_ms=round(gap, 2), ratio=round(row[y]['ms'] / row[x]['ms'], 3),
                                             separates=bool(gap > 3 * max(row[x]['spread'], row[y]['spread'])))
        row['kernels'] = {k: v for k, v in clock['cols'][str(P)].items() if k.startswith('k_')}
        row['peak_pool_bytes_one_lane'] = mem['cols'][str(P)]['peak_pool_bytes']
        row['pool_bytes_before_call'] = mem['cols'][str(P)]['live_before_bytes']
        summary['cols'][str(P)] = row
    if a.out:
        with open(a.out, 'a') as f:
            f.write(json.dumps(dict(summary=summary)) + '\n')
    print(json.dumps(summary), flush=True)


if __name__ == '__main__':
    main()
