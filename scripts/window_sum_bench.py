#!/usr/bin/env python3
"""Window sums (fhe_direct_window_sum) on one MI355X at BASELINE config 3's
context (N = 1024, ring 2^16, depth 39, sign (3, 5, 2)), eps = 1 / N, for P in
--cols columns (0 = the count alone), in four cases, all self joins on the grid
2 / N:

  g1_rows     PARTITION BY g ORDER BY t ROWS UNBOUNDED PRECEDING -- three signs per batch
  g1_between  PARTITION BY g ORDER BY t RANGE BETWEEN 2 / N PRECEDING AND 2 / N FOLLOWING -- four
  g2_group    GROUP BY a, b -- four
  g2_le       PARTITION BY a, b ORDER BY t, the default RANGE frame -- five, three factors

Arms:
  a  one window_sum call (k_sub_window_stacked, k_tensor_win / k_tensor_lex, k_tensor_run)
  b  the same under FHE_WIN_FUSED=0 (sub_stacked with the constants in place or
     the offsets per member; sub, sub, mul)
  c  the baseline, the PARENT commit's only way to the same values: the
     composition batch by batch through its public ops (compose_rotate,
     mul_plain_sum, sub, add_plain / add_const, sign, mul), on --baseline-lib --
     the parent's library, never the code under test against itself.  Its masks
     and tie-break offsets are encoded on the device before the timed calls, as
     the operator's cached ones are.  Build the library from a checkout of the
     parent (make -C fhe-sorting_amd lib/libfhesort.so) and pass its path;
     without it arm c is left out and nothing is concluded about it.
  d  running_sum (ROWS) and group_sum on the order key (P in --cols) and lex_rank
     with two keys on this build, for scale

Every arm runs in a process of its own (the switch and the library are read once
per process); the arms alternate inside each of --rounds rounds.  A timing is one
call (arm c: the whole composition) from a drained stream to fhe_sync; per
process, the median of --steps timings after --warmup untimed ones; per arm, the
median of the rounds' medians, and `spread` = the largest minus the smallest
round median.  `separates`: the gap exceeds three times the larger of the two
spreads.  Every timed result of arms a, b and c is decrypted
and compared with the exact plaintext sums (max_abs_err).

usage: window_sum_bench.py [--cols 0,1,8] [--cases g1_rows,g1_between,g2_group,g2_le] [--rounds 3] [--steps 3]
                           [--warmup 1] [--baseline-lib PATH] [--out FILE.jsonl] [--n 1024 --logn 16] [--summarise]
Appends one JSON line per process to --out (default profiles/window_sum/window_sum_bench.jsonl)
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

NEW_SYMBOLS = ('fhe_direct_window_sum', 'fhe_window_sum_levels', 'fhe_sub_window_stacked', 'fhe_mul_sub_sub')
BINARY = 2
ROWS, LE, LT, BETWEEN, GROUP = range(5)
CASES = {'g1_rows': (1, ROWS), 'g1_between': (1, BETWEEN), 'g2_group': (2, GROUP), 'g2_le': (2, LE)}


def sign_cfg(N):  # as bench.py
    return (3, 2, 2) if N <= 16 else (3, 3, 2) if N <= 128 else (3, 4, 2) if N <= 512 else (3, 5, 2)


def rank_np(N, P):  # src/sort_algo.h:383-416
    for lim, v in ((8, 2), (32, 4), (128, 8), (512, 16), (2048, 32)):
        if N <= lim:
            return min(v, P) if N >= 4 else 1
    return 1


def child(a):
    import ctypes
    import numpy as np
    import fhesort as F
    if a.child == 'c':  # the parent's library has none of the new entry points
        have = ctypes.CDLL(F.LIB_PATH)
        for s in NEW_SYMBOLS:
            if not hasattr(have, s):
                F._SIGS.pop(s, None)
    N, cfg, eps = a.n, sign_cfg(a.n), 1.0 / a.n
    depth, rots = F.size_parameters(N)
    cols_list = [int(v) for v in a.cols.split(',')]
    cases = a.cases.split(',')
    ctx = F.Context(a.logn, depth, 40, 60, 3, seed=2025)
    ctx.gen_rotation_keys(rots)
    rng = np.random.default_rng(N)
    per2 = max(2, int(np.ceil((N / 8.0) ** 0.5)))
    partv = {1: [rng.integers(0, max(3, N // 8), N) * 2.0 / N],              # about eight rows per partition
             2: [rng.integers(0, per2, N) * 2.0 / N for _ in range(2)]}
    tv = rng.integers(0, N // 2 - 1, N) * 2.0 / N                            # the order key, ties included
    lov, hiv = tv - 2.0 / N, tv + 2.0 / N
    colv = [rng.uniform(-1, 1, N) for _ in range(max(cols_list + [1]))]
    e, j = np.arange(N)[:, None], np.arange(N)[None, :]
    dt = tv[:, None] - tv[None, :]
    order_w = {ROWS: (dt + np.where(j <= e, eps, -eps) > 0).astype(np.float64), LE: (dt + eps > 0).astype(np.float64),
               BETWEEN: (hiv[:, None] - tv[None, :] + eps > 0).astype(np.float64) - (lov[:, None] - tv[None, :] - eps > 0),
               GROUP: np.ones((N, N))}
    weight = {}
    for c, (G, mode) in CASES.items():
        w = order_w[mode].copy()
        for k in partv[G]:
            w *= np.abs(k[:, None] - k[None, :]) < eps
        weight[c] = w
    weight['running'] = order_w[ROWS]
    weight['group'] = (np.abs(dt) < eps).astype(np.float64)
    part = {G: [ctx.encrypt(k, N) for k in ks] for G, ks in partv.items()}
    t, lo, hi = (ctx.encrypt(v, N) for v in (tv, lov, hiv))
    cols = [ctx.encrypt(v, N) for v in colv]
    ctx.sync()

    S = min(N, (1 << (a.logn - 1)) // N) * N
    Pn, nb = S // N, N // (S // N)
    npb = rank_np(N, Pn)
    Lm = t.level + 1 + 3 * (max(cfg[1], 1) + cfg[2])
    masks, offsets = {}, {}

    def slots(ct, s):
        ct.set_slots(s)
        return ct

    def baby_steps(x):
        return [slots(y, S) for y in [ctx.compose_rotate(x, N, rots, BINARY, i) for i in range(npb)]]

    def vec_rots_opt(baby, b):
        level, out = baby[0].level, None
        for jj in range(Pn // npb):
            mk = (b, jj, level)
            if mk not in masks:  # encoded once, outside the timed calls (the warm-up call)
                masks[mk] = ctx.encode_masks([(0, npb * jj + i, -b * Pn - jj * npb, level) for i in range(npb)], S, N)
            o = ctx.compose_rotate(ctx.mul_plain_sum(baby, masks[mk]), N, rots, BINARY, b * Pn + jj * npb)
            out = o if out is None else ctx.add(out, o)
        return out

    def composed(case, P):
        """arm c: the definition op by op, batch by batch"""
        G, mode = CASES[case]
        Fn = G + (mode != GROUP)
        La = Lm + (1 if Fn == 2 else 2)
        dup = lambda x: slots(ctx.add_const(x, 0.0), S)
        pb = [baby_steps(k) for k in part[G]]
        pd = [dup(k) for k in part[G]]
        cb = [baby_steps(ctx.mul_const_to(cols[p], 2.0 ** -Fn, La - 1)) for p in range(P)]
        if mode != GROUP:
            ob, od = baby_steps(t), dup(hi if mode == BETWEEN else t)
            od_lo = dup(lo) if mode == BETWEEN else None
        accs, cnt = [None] * P, None
        for b in range(nb):
            phi = []
            for g in range(G):
                d = ctx.sub(pd[g], vec_rots_opt(pb[g], b))
                phi.append(ctx.sub(ctx.sign(ctx.add_const(d, eps), *cfg), ctx.sign(ctx.add_const(d, -eps), *cfg)))
            if mode != GROUP:
                sk = vec_rots_opt(ob, b)
                d = ctx.sub(od, sk)
                if mode == ROWS:
                    if (b, d.level) not in offsets:  # encoded once, as the masks are
                        offsets[(b, d.level)] = ctx.encode_tiebreak([b], S, N, eps, d.level)[0]
                    phi.append(ctx.add_const(ctx.sign(ctx.add_plain(d, offsets[(b, d.level)]), *cfg), 1.0))
                elif mode == BETWEEN:
                    su = ctx.sign(ctx.add_const(d, eps), *cfg)
                    sw = ctx.sign(ctx.add_const(ctx.sub(od_lo, sk), -eps), *cfg)
                    phi.append(ctx.sub(su, sw))
                else:
                    phi.append(ctx.add_const(ctx.sign(ctx.add_const(d, eps), *cfg), 1.0))
            ind = ctx.mul(phi[0], phi[1]) if Fn == 2 else ctx.mul(phi[0], ctx.mul(phi[1], phi[2]))
            if P == 0:
                c = ctx.mul_const(ind, 2.0 ** -Fn)
                cnt = c if cnt is None else ctx.add(cnt, c)
            for p in range(P):
                g = ctx.mul(ind, vec_rots_opt(cb[p], b))
                accs[p] = g if accs[p] is None else ctx.add(accs[p], g)

        def fold(v):
            i = 1
            while (1 << i) <= Pn:
                v = ctx.add(v, ctx.compose_rotate(v, N, rots, BINARY, S >> i))
                i += 1
            return slots(v, N)
        return [fold(v) for v in accs] if P else [fold(cnt)]

    def call(case, P):
        if a.child == 'c':
            return composed(case, P)
        if case == 'lex':
            return [ctx.lex_rank([part[1][0], t], eps, N, rots, cfg)]
        if case == 'running':
            if P == 0:
                return [ctx.running_sum(t, t, [], eps, N, rots, cfg, mode=ROWS, count=True)[1]]
            return ctx.running_sum(t, t, cols[:P], eps, N, rots, cfg, mode=ROWS)
        if case == 'group':
            if P == 0:
                return [ctx.group_sum(t, t, [], eps, N, rots, cfg, count=True)[1]]
            return ctx.group_sum(t, t, cols[:P], eps, N, rots, cfg)
        G, mode = CASES[case]
        kw = dict(mode=mode)
        if mode != GROUP:
            kw.update(order_left=hi if mode == BETWEEN else t, order_right=t, lo=lo if mode == BETWEEN else None)
        if P == 0:
            return [ctx.window_sum(part[G], part[G], [], eps, N, rots, cfg, count=True, **kw)[1]]
        return ctx.window_sum(part[G], part[G], cols[:P], eps, N, rots, cfg, **kw)

    def err(out, case, P):
        if case == 'lex':
            return None  # timed only
        w = weight[case]
        want = [w @ colv[p] for p in range(P)] if P else [w.sum(axis=1)]
        return float(max(np.max(np.abs(ctx.decrypt(o)[:N] - x)) for o, x in zip(out, want)))

    def once(case, P):
        ctx.sync()
        t0 = time.perf_counter()
        out = call(case, P)
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    res = dict(arm=a.child, round=a.round, N=N, logn=a.logn, depth=depth, lib=os.path.basename(F.LIB_PATH),
               fused=os.environ.get('FHE_WIN_FUSED', '1'), steps=a.steps, warmup=a.warmup, cases={})
    plan = ([('lex', 0)] + [(c, P) for c in ('running', 'group') for P in cols_list]) if a.child == 'd' else \
        [(c, P) for c in cases for P in cols_list]
    for case, P in plan:
        for _ in range(a.warmup):
            once(case, P)
        ts = []
        for _ in range(a.steps):
            tm, out = once(case, P)
            ts.append(tm)
        row = dict(ms=round(statistics.median(ts), 2), min_ms=round(min(ts), 2), max_ms=round(max(ts), 2))
        row['level_out'] = out[0].level
        row['max_abs_err'] = err(out, case, P)
        res['cases'][f'{case}_P{P}'] = row
    print('RESULT ' + json.dumps(res), flush=True)


def summarise(recs_by_arm, a):
    arms = [arm for arm in ('a', 'b', 'c', 'd') if recs_by_arm.get(arm)]
    summary = dict(N=a.n, logn=a.logn, rounds=a.rounds, steps=a.steps, warmup=a.warmup, arms={})
    for arm in arms:
        summary['arms'][arm] = {}
        for case in recs_by_arm[arm][0]['cases']:
            rows = [r['cases'][case] for r in recs_by_arm[arm] if case in r['cases']]
            meds = [r['ms'] for r in rows]
            errs = [r['max_abs_err'] for r in rows if r['max_abs_err'] is not None]
            summary['arms'][arm][case] = dict(ms=round(statistics.median(meds), 2), spread=round(max(meds) - min(meds), 2),
                                              rounds=meds, max_abs_err=max(errs) if errs else None)
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
    return summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--cols', default='0,1,8')
    ap.add_argument('--cases', default=','.join(CASES))
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--n', type=int, default=1024)
    ap.add_argument('--logn', type=int, default=16)
    ap.add_argument('--baseline-lib', default=None)
    ap.add_argument('--out', default=os.path.join(HERE, '..', 'profiles', 'window_sum', 'window_sum_bench.jsonl'))
    ap.add_argument('--child-timeout', type=int, default=400)
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
        env.pop('FHE_WIN_FUSED', None)
        env.pop('FHE_LIB', None)
        if arm == 'b':
            env['FHE_WIN_FUSED'] = '0'
        if arm == 'c':
            env['FHE_LIB'] = os.path.abspath(a.baseline_lib)
        cmd = [sys.executable, os.path.abspath(__file__), '--child', arm, '--round', str(rnd), '--cols', a.cols,
               '--cases', a.cases, '--steps', str(a.steps), '--warmup', str(a.warmup), '--n', str(a.n),
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
