#!/usr/bin/env python3
"""Gather by encrypted position (fhe_direct_gather) on one MI355X at BASELINE config
3's context (N = 1024, ring 2^16, depth 39): LAG / LEAD on a rank -- a permutation
of 0 .. N - 1 encrypted at the level constructRank leaves a level-0 key's rank at --
for the cases of --cases, each K<offsets>P<columns>[F]: K offsets (-1; or -1, 0, 1),
P columns (0 = the present flags alone), F the summed ROWS BETWEEN frame.

Arms:
  a  one gather call (k_sub_offsets_stacked, k_tensor_gather)
  b  the same under FHE_GATHER_FUSED=0 (sub_stacked with add_const / negate on the
     stack per offset, one stacked product per column and offset)
  c  the baseline, the PARENT commit's only way to the same values: the
     composition batch by batch through its public ops (compose_rotate,
     mul_plain_sum, sub, add_const, negate, mul_const, cheb, mul), on
     --baseline-lib -- the parent's library, never the code under test against
     itself.  Its masks are encoded on the device before the timed calls, as the
     operator's cached ones are.  Build the library from a checkout of the parent
     (make -C fhe-sorting_amd lib/libfhesort.so) and pass its path; without it arm
     c is left out and nothing is concluded about it.
  d  one index check (direct_sort mode 2 with the rank given) on this build, for
     scale: one series per batch where the gather runs K

Every arm runs in a process of its own (the switch and the library are read once
per process); the arms alternate inside each of --rounds rounds.  A timing is one
call (arm c: the whole composition) from a drained stream to fhe_sync; per
process, the median of --steps timings after --warmup untimed ones; per arm, the
median of the rounds' medians, and `spread` = the largest minus the smallest
round median.  `separates`: the gap exceeds three times the larger of the two
spreads.  Every timed result is decrypted and compared with the
exact neighbours (max_abs_err).

usage: gather_bench.py [--cases K1P0,K1P1,K1P8,K3P1,K3P1F] [--baseline-cases K1P1,K3P1] [--rounds 3] [--steps 3]
                       [--warmup 1] [--baseline-lib PATH] [--out FILE.jsonl] [--n 1024 --logn 16] [--summarise]
Appends one JSON line per process to --out (default profiles/gather/gather_bench.jsonl)
and prints the summary line; --summarise recomputes the summary from the file alone.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, '..', 'fhe-sorting_amd'))

NEW_SYMBOLS = ('fhe_direct_gather', 'fhe_gather_levels', 'fhe_sub_offsets_stacked', 'fhe_mul_gather')
BINARY = 2


def sign_cfg(N):  # as bench.py
    return (3, 2, 2) if N <= 16 else (3, 3, 2) if N <= 128 else (3, 4, 2) if N <= 512 else (3, 5, 2)


def rank_np(N, P):  # src/sort_algo.h:383-416
    for lim, v in ((8, 2), (32, 4), (128, 8), (512, 16), (2048, 32)):
        if N <= lim:
            return min(v, P) if N >= 4 else 1
    return 1


def parse_case(c):
    m = re.fullmatch(r'K(\d+)P(\d+)(F?)', c)
    if not m or int(m.group(1)) not in (1, 3):
        raise SystemExit(f'bad case {c}: K1 or K3, then P<columns>, then F for the summed frame')
    return ([-1] if m.group(1) == '1' else [-1, 0, 1]), int(m.group(2)), m.group(3) == 'F'


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
    cases = (a.baseline_cases if a.child == 'c' else a.cases).split(',')
    ctx = F.Context(a.logn, depth, 40, 60, 3, seed=2025)
    ctx.gen_rotation_keys(rots)
    rng = np.random.default_rng(N)
    posv = rng.permutation(N).astype(np.float64)
    colv = [rng.uniform(-1, 1, N) for _ in range(max([parse_case(c)[1] for c in cases] + [1]))]
    rank_level = F.group_sum_levels(0, cfg)[1]  # where constructRank leaves the rank of a level-0 key
    pos = ctx.encrypt(posv, N, rank_level)
    cols = [ctx.encrypt(v, N) for v in colv]
    ctx.sync()

    S = min(N, (1 << (a.logn - 1)) // N) * N
    Pn, nb = S // N, N // (S // N)
    npb = rank_np(N, Pn)
    coeffs = np.fromfile(os.path.join(F.COEFF_DIR, f'doubled_sinc_{N}.f64'))
    trimmed = len(np.trim_zeros(coeffs, 'b')) - 1
    masks = {}

    def slots(ct, s):
        ct.set_slots(s)
        return ct

    def baby_steps(x):
        return [ctx.compose_rotate(x, N, rots, BINARY, i) for i in range(npb)]

    def vec_rots_opt(baby, b):
        level, out = baby[0].level, None
        for j in range(Pn // npb):
            mk = (b, j, level)
            if mk not in masks:  # encoded once, outside the timed calls (the warm-up call)
                masks[mk] = ctx.encode_masks([(0, npb * j + i, -b * Pn - j * npb, level) for i in range(npb)], S, N)
            o = ctx.compose_rotate(ctx.mul_plain_sum(baby, masks[mk]), N, rots, BINARY, b * Pn + j * npb)
            out = o if out is None else ctx.add(out, o)
        return out

    def composed(offs, P, frame):
        """arm c: the definition op by op, batch by batch"""
        Ls = None
        rb = [slots(x, S) for x in baby_steps(pos)]
        dup = slots(ctx.add_const(pos, 0.0), S)
        Ko = 1 if frame else len(offs)
        accs, cnt, cb = [None] * (P * Ko), [None] * Ko, None
        for b in range(nb):
            base = ctx.sub(dup, vec_rots_opt(rb, b))
            rs = []
            for o in offs:
                d = ctx.add_const(base, float(o))
                if o < 0:
                    d = ctx.negate(d)
                rs.append(ctx.cheb(ctx.mul_const(d, 1.0 / N / 2), coeffs, -1.0, 1.0))
            if frame:
                tot = rs[0]
                for r in rs[1:]:
                    tot = ctx.add(tot, r)
                rs = [tot]
            if cb is None:
                Ls = rs[0].level
                cb = [[slots(x, S) for x in baby_steps(ctx.mul_const_to(cols[p], 1.0, Ls - 1))] for p in range(P)]
            if P == 0:
                for k in range(Ko):
                    cnt[k] = rs[k] if cnt[k] is None else ctx.add(cnt[k], rs[k])
            for p in range(P):
                sc = vec_rots_opt(cb[p], b)
                for k in range(Ko):
                    g = ctx.mul(rs[k], sc)
                    accs[p * Ko + k] = g if accs[p * Ko + k] is None else ctx.add(accs[p * Ko + k], g)

        def fold(v):
            i = 1
            while (1 << i) <= Pn:
                v = ctx.add(v, ctx.compose_rotate(v, N, rots, BINARY, S >> i))
                i += 1
            return slots(v, N)
        return [fold(v) for v in (accs if P else cnt)]

    def call(case):
        offs, P, frame = parse_case(case)
        if a.child == 'c':
            return composed(offs, P, frame)
        if a.child == 'd':
            return [ctx.direct_sort(cols[0], N, rots, cfg, mode=2, rank=pos)]
        if P == 0:
            return ctx.gather(pos, pos, [], offs, N, rots, present=True, sum_offsets=frame)[1]
        return ctx.gather(pos, pos, cols[:P], offs, N, rots, sum_offsets=frame)

    def err(out, case):
        offs, P, frame = parse_case(case)
        if a.child == 'd':
            want = [colv[0][np.argsort(posv)]]
        else:
            m = [(posv[:, None] + o == posv[None, :]).astype(np.float64) for o in offs]
            m = [sum(m)] if frame else m
            want = [mk @ colv[p] for p in range(P) for mk in m] if P else [mk.sum(axis=1) for mk in m]
        return float(max(np.max(np.abs(ctx.decrypt(o)[:N] - w)) for o, w in zip(out, want)))

    def once(case):
        ctx.sync()
        t0 = time.perf_counter()
        out = call(case)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    res = dict(arm=a.child, round=a.round, N=N, logn=a.logn, depth=depth, lib=os.path.basename(F.LIB_PATH),
               fused=os.environ.get('FHE_GATHER_FUSED', '1'), steps=a.steps, warmup=a.warmup, series_degree=trimmed,
               pos_level=rank_level, cases={})
    for case in (['K1P1'] if a.child == 'd' else cases):
        for _ in range(a.warmup):
            once(case)
        ts = []
        for _ in range(a.steps):
            t, out = once(case)
            ts.append(t)
        row = dict(ms=round(statistics.median(ts), 2), min_ms=round(min(ts), 2), max_ms=round(max(ts), 2))
        row['level_out'] = out[0].level
        row['max_abs_err'] = err(out, case)
        res['cases'][case] = row
    print('RESULT ' + json.dumps(res), flush=True)


def summarise(recs_by_arm, a):
    arms = [arm for arm in ('a', 'b', 'c', 'd') if recs_by_arm.get(arm)]
    summary = dict(N=a.n, logn=a.logn, rounds=a.rounds, steps=a.steps, warmup=a.warmup, arms={})
    for arm in arms:
        summary['arms'][arm] = {}
        for case in recs_by_arm[arm][0]['cases']:
            rows = [r['cases'][case] for r in recs_by_arm[arm] if case in r['cases']]
            meds = [r['ms'] for r in rows]
            summary['arms'][arm][case] = dict(ms=round(statistics.median(meds), 2), spread=round(max(meds) - min(meds), 2),
                                              rounds=meds, max_abs_err=max(r['max_abs_err'] for r in rows))
    for other, name in (('b', 'fused_vs_plain'), ('c', 'operator_vs_composition')):
        if other in arms and 'a' in arms:
            summary[name] = {}
            for case, row in summary['arms']['a'].items():
                base = summary['arms'][other].get(case)
                if base:
                    gap = base['ms'] - row['ms']
                    lim = 3 * max(row['spread'], base['spread'])
                    summary[name][case] = dict(a_ms=row['ms'], other_ms=base['ms'], ratio=round(base['ms'] / row['ms'], 4),
                                               separates=bool(abs(gap) > lim), faster='a' if gap > lim else
                                               (other if -gap > lim else None))
    if 'd' in arms and 'a' in arms:
        check_ms = summary['arms']['d']['K1P1']['ms']
        summary['against_index_check'] = {case: round(row['ms'] / check_ms, 3)
                                          for case, row in summary['arms']['a'].items()}
    return summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cases', default='K1P0,K1P1,K1P8,K3P0,K3P1,K3P8,K3P1F')
    ap.add_argument('--baseline-cases', default='K1P1,K3P1')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--n', type=int, default=1024)
    ap.add_argument('--logn', type=int, default=16)
    ap.add_argument('--baseline-lib', default=None)
    ap.add_argument('--out', default=os.path.join(HERE, '..', 'profiles', 'gather', 'gather_bench.jsonl'))
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
        env.pop('FHE_GATHER_FUSED', None)
        env.pop('FHE_LIB', None)
        if arm == 'b':
            env['FHE_GATHER_FUSED'] = '0'
        if arm == 'c':
            env['FHE_LIB'] = os.path.abspath(a.baseline_lib)
        cmd = [sys.executable, os.path.abspath(__file__), '--child', arm, '--round', str(rnd), '--cases', a.cases,
               '--baseline-cases', a.baseline_cases, '--steps', str(a.steps), '--warmup', str(a.warmup), '--n', str(a.n),
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

    arms = ['a', 'b'] + (['c'] if a.baseline_lib else []) + ['d']
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
