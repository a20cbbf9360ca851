#!/usr/bin/env python3
"""Tie-breaking DirectSort (fhe_set_sort_tiebreak) against the plain
sort, on one MI355X at BASELINE config 3's context (N = 1024, ring 2^16, depth 39,
sign (3,5,2)).

Arms, each timing one whole direct_sort (rank and index check):
  a  eps = 0 on a permutation input: the plain sort on this build
  p  the same on --baseline-lib, the PARENT commit's library (make -C
     fhe-sorting_amd lib/libfhesort.so in a checkout of the parent) -- never the
     code under test against itself; without it arm p is left out and nothing is
     concluded about arm a
  b  eps = 1 / N on a tied input (values on the grid 2 / N, multiplicities up to ~9)
  c  arm b under FHE_TIEBREAK_FUSED=0 (sub_stacked, then one c0 addition per member)

Every arm runs in a process of its own (the switch and the library are read once
per process); the arms alternate inside each of --rounds rounds.  A timing is one
call from a drained stream to fhe_sync; per process, the median of --steps timings
after --warmup untimed ones; per arm, the median of the rounds' medians, and
`spread` = the largest minus the smallest round median.  `separates`: the gap
exceeds three times the larger of the two spreads.  Every timed
result is decrypted and compared with np.sort of its input (max_abs_err).  Arm b
also records the device memory the cached offset plaintexts hold (fhe_pool_stats
live bytes after the first tie-broken sort minus before it, outputs released).

usage: stable_bench.py [--rounds 3] [--steps 3] [--warmup 1] [--baseline-lib PATH]
                       [--out FILE.jsonl] [--n 1024 --logn 16]
Appends one JSON line per process to --out (default profiles/stable/stable_bench.jsonl)
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


def sign_cfg(N):  # as bench.py
    return (3, 2, 2) if N <= 16 else (3, 3, 2) if N <= 128 else (3, 4, 2) if N <= 512 else (3, 5, 2)


def child(a):
    import ctypes
    import numpy as np
    import fhesort as F
    if a.child == 'p':  # the parent's library lacks the entry points added since
        have = ctypes.CDLL(F.LIB_PATH)
        for s in list(F._SIGS):
            if not hasattr(have, s):
                F._SIGS.pop(s)
    N, cfg = a.n, sign_cfg(a.n)
    depth, rots = F.size_parameters(N)
    ctx = F.Context(a.logn, depth, 40, 60, 3, seed=2025)
    ctx.gen_rotation_keys(rots)
    rng = np.random.default_rng(N)
    tied = a.child in ('b', 'c')
    x = rng.integers(0, N // 2, N) * 2.0 / N if tied else rng.permutation(N) / N
    ct = ctx.encrypt(x, N)
    ctx.sync()
    res = dict(arm=a.child, round=a.round, N=N, logn=a.logn, depth=depth,
               lib='parent' if a.child == 'p' else 'this build', eps=1.0 / N if tied else 0.0,
               fused=os.environ.get('FHE_TIEBREAK_FUSED', '1'), steps=a.steps, warmup=a.warmup,
               max_multiplicity=int(np.unique(x, return_counts=True)[1].max()))

    def once():
        ctx.sync()
        t0 = time.perf_counter()
        out = ctx.direct_sort(ct, N, rots, cfg)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    if tied:  # the plain sort first, so the masks are cached before the offsets are measured
        _, out = once()
        res['plain_sort_max_abs_err'] = float(np.max(np.abs(ctx.decrypt(out) - np.sort(x))))
        del out
        ctx.sync()
        live0 = ctx.pool_stats()['live']
        ctx.set_sort_tiebreak(1.0 / N)
        _, out = once()
        del out
        ctx.sync()
        res['offset_plaintext_bytes'] = int(ctx.pool_stats()['live'] - live0)
    for _ in range(a.warmup):
        once()
    ts = []
    for _ in range(a.steps):
        t, out = once()
        ts.append(t)
    res.update(ms=round(statistics.median(ts), 2), min_ms=round(min(ts), 2), max_ms=round(max(ts), 2),
               level_out=out.level, max_abs_err=float(np.max(np.abs(ctx.decrypt(out) - np.sort(x)))))
    print('RESULT ' + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--n', type=int, default=1024)
    ap.add_argument('--logn', type=int, default=16)
    ap.add_argument('--baseline-lib', default=None)
    ap.add_argument('--out', default=os.path.join(HERE, '..', 'profiles', 'stable', 'stable_bench.jsonl'))
    ap.add_argument('--child-timeout', type=int, default=240)
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--round', type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)

    def run(arm, rnd):
        env = dict(os.environ)
        env.pop('FHE_TIEBREAK_FUSED', None)
        env.pop('FHE_LIB', None)
        if arm == 'c':
            env['FHE_TIEBREAK_FUSED'] = '0'
        if arm == 'p':
            env['FHE_LIB'] = os.path.abspath(a.baseline_lib)
        cmd = [sys.executable, os.path.abspath(__file__), '--child', arm, '--round', str(rnd), '--steps', str(a.steps),
               '--warmup', str(a.warmup), '--n', str(a.n), '--logn', str(a.logn)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')), None)
        if r.returncode != 0 or line is None:  # stop here: nothing more is started after a failed process
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f'arm {arm} round {rnd} failed with status {r.returncode}')
        rec = json.loads(line[7:])
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(json.dumps(rec) + '\n')
        print(f'arm {arm} round {rnd}: {rec["ms"]} ms, max error {rec["max_abs_err"]:.3e}', flush=True)
        return rec

    arms = ['a'] + (['p'] if a.baseline_lib else []) + ['b', 'c']
    recs = {arm: [] for arm in arms}
    for rnd in range(a.rounds):
        for arm in arms:
            recs[arm].append(run(arm, rnd))
    summary = dict(N=a.n, logn=a.logn, rounds=a.rounds, steps=a.steps, warmup=a.warmup, arms={})
    for arm in arms:
        meds = [r['ms'] for r in recs[arm]]
        summary['arms'][arm] = dict(ms=round(statistics.median(meds), 2), spread=round(max(meds) - min(meds), 2),
                                    rounds=meds, max_abs_err=max(r['max_abs_err'] for r in recs[arm]),
                                    level_out=recs[arm][0]['level_out'])
    A = summary['arms']

    def versus(x, y):
        gap = abs(A[x]['ms'] - A[y]['ms'])
        return dict(gap_ms=round(A[x]['ms'] - A[y]['ms'], 2), separates=bool(gap > 3 * max(A[x]['spread'], A[y]['spread'])))

    if 'p' in arms:
        summary['plain_vs_parent'] = versus('a', 'p')
    summary['tiebreak_vs_plain'] = versus('b', 'a')
    summary['fused_vs_unfused'] = versus('b', 'c')
    summary['offset_plaintext_bytes'] = recs['b'][0]['offset_plaintext_bytes']
    summary['plain_sort_of_tied_input_max_abs_err'] = recs['b'][0]['plain_sort_max_abs_err']
    with open(a.out, 'a') as f:
        f.write(json.dumps(dict(summary=summary)) + '\n')
    print(json.dumps(summary), flush=True)


if __name__ == '__main__':
    main()
