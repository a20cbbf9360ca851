#!/usr/bin/env python3
"""Joins between tables of different sizes (fhe_set_pair_tables) on one MI355X at
BASELINE config 3's context (N = 1024, ring 2^16, depth 39, sign (3, 5, 2)):
group_sum with the count and 0 / 1 / 8 columns and gather with one offset and one
column (positions at the level constructRank leaves a level-0 key's rank at),
for (Nl, Nr) in --shapes (default 1024x32, 1024x256, 32x1024).  Keys lie on the
grid 2 / N, eps = 1 / N; the smaller table's keys are distinct and the larger one
draws from twice as many grid points.

Arms:
  r  the rectangular call of this build: tables=(Nl, Nr), the small table as it is
  p  the baseline, what a user does today: the square call with the small table
     padded to N rows by a sentinel key 2 eps below every real key (zero columns;
     unused positions for the gather), on --baseline-lib -- the parent's library,
     never the code under test against itself.  Build the library from a
     checkout of the parent (make -C fhe-sorting_amd lib/libfhesort.so) and pass
     its path; without it arm p is left out and nothing is concluded about it.

Every arm runs in a process of its own (the library is read once per process);
the arms alternate inside each of --rounds rounds.  A timing is one call from a
drained stream to fhe_sync; per process, the median of --steps timings after
--warmup untimed ones; per arm, the median of the rounds' medians, and `spread` =
the largest minus the smallest round median.  `separates`: the gap exceeds the
larger of the two spreads; `separates3`: three times it.  Every
timed result is decrypted and compared with the exact plaintext sums over the Nl
real left rows (max_abs_err).

usage: rect_tables_bench.py [--shapes 1024x32,1024x256,32x1024] [--cols 0,1,8] [--rounds 3] [--steps 3]
                            [--warmup 1] [--baseline-lib PATH] [--out FILE.jsonl] [--logn 16] [--summarise]
Appends one JSON line per process to --out (default profiles/rect_tables/rect_tables_bench.jsonl)
and prints the summary line; --summarise recomputes the summary from the file alone.
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

NEW_SYMBOLS = ('fhe_set_pair_tables', 'fhe_pair_shape')


def sign_cfg(N):  # as bench.py
    return (3, 2, 2) if N <= 16 else (3, 3, 2) if N <= 128 else (3, 4, 2) if N <= 512 else (3, 5, 2)


def tables(Nl, Nr, rng):
    """(kl, kr, pl, pr): keys on the grid 2 / N below 1 - 6 / N, integer positions below N (the right ones distinct)"""
    import numpy as np
    N, n = max(Nl, Nr), min(Nl, Nr)
    grid = rng.permutation(np.arange(N // 2 - 2) * 2.0 / N)
    small, large = grid[:n], rng.choice(grid[:2 * n], N)
    kl, kr = (large, small) if Nl >= Nr else (small, large)
    return kl, kr, rng.integers(0, N, Nl).astype(np.float64), rng.permutation(N)[:Nr].astype(np.float64)


def child(a):
    import ctypes
    import numpy as np
    import fhesort as F
    if a.child == 'p':  # the parent's library has none of the new entry points
        have = ctypes.CDLL(F.LIB_PATH)
        for s in NEW_SYMBOLS:
            if not hasattr(have, s):
                F._SIGS.pop(s, None)
    shapes = [tuple(int(v) for v in s.split('x')) for s in a.shapes.split(',')]
    cols_list = [int(v) for v in a.cols.split(',')]
    N = max(max(s) for s in shapes)
    assert all(max(s) == N for s in shapes), 'one context: every shape has the same larger table'
    cfg, eps = sign_cfg(N), 1.0 / N
    depth, rots = F.size_parameters(N)
    ctx = F.Context(a.logn, depth, 40, 60, 3, seed=2025)
    ctx.gen_rotation_keys(rots)
    rank_level = F.group_sum_levels(0, cfg)[1]  # where constructRank leaves the rank of a level-0 key
    res = dict(arm=a.child, round=a.round, N=N, logn=a.logn, depth=depth,
               lib='baseline' if os.environ.get('FHE_LIB') else 'this build', steps=a.steps, warmup=a.warmup,
               pos_level=rank_level, cases={})
    for Nl, Nr in shapes:
        rng = np.random.default_rng([N, Nl, Nr])
        kl, kr, pl, pr = tables(Nl, Nr, rng)
        colv = [rng.uniform(-1, 1, Nr) for _ in range(max(cols_list + [1]))]
        match = (np.abs(kl[:, None] - kr[None, :]) < eps).astype(np.float64)
        hit = (pl[:, None] == pr[None, :]).astype(np.float64)
        if a.child == 'p':  # today's call: both tables in N rows
            pad = lambda v, fill: np.concatenate([v, np.full(N - len(v), fill)])
            rest = np.setdiff1d(np.arange(N, dtype=np.float64), pr)  # the positions no right row holds
            kl_, kr_, pl_ = pad(kl, -2.0 / N), pad(kr, -4.0 / N), pad(pl, 0.0)
            pr_ = np.concatenate([pr, rest])
            colv_ = [pad(v, 0.0) for v in colv]
            tb, sl, sr = None, N, N
        else:
            kl_, kr_, pl_, pr_, colv_ = kl, kr, pl, pr, colv
            tb, sl, sr = (Nl, Nr), Nl, Nr
        ekl, ekr = ctx.encrypt(kl_, sl), ctx.encrypt(kr_, sr)
        epl, epr = ctx.encrypt(pl_, sl, rank_level), ctx.encrypt(pr_, sr, rank_level)
        ecols = [ctx.encrypt(v, sr) for v in colv_]
        ctx.sync()

        def call(case):
            if case == 'gather':
                return ctx.gather(epl, epr, ecols[:1], [0], N, rots, tables=tb)
            P = int(case[1:])
            if P == 0:
                return [ctx.group_sum(ekl, ekr, [], eps, N, rots, cfg, count=True, tables=tb)[1]]
            return ctx.group_sum(ekl, ekr, ecols[:P], eps, N, rots, cfg, tables=tb)

        def err(out, case):
            if case == 'gather':
                want = [hit @ colv[0]]
            else:
                P = int(case[1:])
                want = [match @ colv[p] for p in range(P)] if P else [match.sum(axis=1)]
            return float(max(np.max(np.abs(ctx.decrypt(o)[:Nl] - w)) for o, w in zip(out, want)))

        def once(case):
            ctx.sync()
            t0 = time.perf_counter()
            out = call(case)
            ctx.sync()
            return (time.perf_counter() - t0) * 1e3, out

        for case in [f'P{P}' for P in cols_list] + ['gather']:
            for _ in range(a.warmup):
                once(case)
            ts = []
            for _ in range(a.steps):
                t, out = once(case)
                ts.append(t)
            row = dict(ms=round(statistics.median(ts), 2), min_ms=round(min(ts), 2), max_ms=round(max(ts), 2),
                       level_out=out[0].level, slots_out=out[0].slots, max_abs_err=err(out, case))
            if a.child == 'r':
                row['shape'] = dict(zip(('num_slots', 'num_partition', 'num_batch', 'np', 'fold_steps'),
                                        F.pair_shape(Nl, Nr, 1 << (a.logn - 1))))
            res['cases'][f'{Nl}x{Nr}:{case}'] = row
            del out
    print('RESULT ' + json.dumps(res), flush=True)


def summarise(recs_by_arm, a):
    arms = [arm for arm in ('r', 'p') if recs_by_arm.get(arm)]
    summary = dict(logn=a.logn, rounds=a.rounds, steps=a.steps, warmup=a.warmup, arms={})
    for arm in arms:
        summary['arms'][arm] = {}
        for case in recs_by_arm[arm][0]['cases']:
            rows = [r['cases'][case] for r in recs_by_arm[arm] if case in r['cases']]
            meds = [r['ms'] for r in rows]
            summary['arms'][arm][case] = dict(ms=round(statistics.median(meds), 2), spread=round(max(meds) - min(meds), 2),
                                              rounds=meds, max_abs_err=max(r['max_abs_err'] for r in rows))
            if 'shape' in rows[0]:
                summary['arms'][arm][case]['shape'] = rows[0]['shape']
    if arms == ['r', 'p']:
        summary['rect_vs_padded'] = {}
        for case, row in summary['arms']['r'].items():
            base = summary['arms']['p'].get(case)
            if base:
                gap, lim = base['ms'] - row['ms'], max(row['spread'], base['spread'])
                summary['rect_vs_padded'][case] = dict(rect_ms=row['ms'], padded_ms=base['ms'],
                                                       ratio=round(base['ms'] / row['ms'], 3),
                                                       separates=bool(abs(gap) > lim), separates3=bool(abs(gap) > 3 * lim),
                                                       faster='rect' if gap > lim else ('padded' if -gap > lim else None))
    return summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='1024x32,1024x256,32x1024')
    ap.add_argument('--cols', default='0,1,8')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--logn', type=int, default=16)
    ap.add_argument('--baseline-lib', default=None)
    ap.add_argument('--out', default=os.path.join(HERE, '..', 'profiles', 'rect_tables', 'rect_tables_bench.jsonl'))
    ap.add_argument('--child-timeout', type=int, default=300)
    ap.add_argument('--summarise', action='store_true')
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--round', type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.summarise:
        recs = {}
        for ln in open(a.out):
            rec = json.loads(ln)
            if 'arm' in rec:
                recs.setdefault(rec['arm'], []).append(rec)
        print(json.dumps(summarise(recs, a)))
        return

    def run(arm, rnd):
        env = dict(os.environ)
        env.pop('FHE_LIB', None)
        if arm == 'p':
            env['FHE_LIB'] = os.path.abspath(a.baseline_lib)
        cmd = [sys.executable, os.path.abspath(__file__), '--child', arm, '--round', str(rnd), '--shapes', a.shapes,
               '--cols', a.cols, '--steps', str(a.steps), '--warmup', str(a.warmup), '--logn', str(a.logn)]
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

    arms = ['r'] + (['p'] if a.baseline_lib else [])
    recs = {arm: [] for arm in arms}
    for rnd in range(a.rounds):
        for arm in arms:
            recs[arm].append(run(arm, rnd))
    summary = summarise(recs, a)
    with open(a.out, 'a') as f:
        f.write(json.dumps(dict(summary=summary)) + '\n')
    print(json.dumps(summary), flush=True)


if __name__ == '__main__':
    main()
