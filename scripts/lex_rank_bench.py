#!/usr/bin/env python3
"""Lexicographic rank (fhe_direct_lex_rank) on one MI355X at BASELINE config 3's
ring and primes (N = 1024, ring 2^16, 40-bit scaling beside the 60-bit q0, dnum 3,
sign (3, 5, 2)) with depth 39 + L - 1: a wide key split into L digits on the grid
2 / N (9 bits each: 18 bits for L = 2, 27 for L = 3), 64 rows repeated so that rows
tie on every digit, eps = tie-break = 1 / N.

Arms, per L in --keys:
  a  one lex_rank call (k_sub_lex_stacked, k_tensor_lex)
  b  the same under FHE_LEX_FUSED=0 (sub_stacked and add_const per key, sub and
     add_const ahead of every product)
  c  the baseline, the PARENT commit's only way to the same values: the
     composition batch by batch through its public ops (compose_rotate,
     mul_plain_sum, sub, add_const, add_plain, sign, mul, mul_const_to), on
     --baseline-lib -- the parent's library, never the code under test against
     itself.  Its masks and offsets are encoded on the device before the timed
     calls, as the operator's cached ones are.  Build the library from a checkout
     of the parent (make -C fhe-sorting_amd lib/libfhesort.so) and pass its path;
     without it arm c is left out and nothing is concluded about it.
  d  direct_sort(mode=1) with the tie-break on the last digit alone, on this build
     and the same context, for scale: one sign member per batch where the
     lexicographic rank runs 2 L - 1

Every arm runs in a process of its own (the switch and the library are read once
per process); the arms alternate inside each of --rounds rounds.  A timing is one
call (arm c: the whole composition) from a drained stream to fhe_sync; per
process, the median of --steps timings after --warmup untimed ones; per arm, the
median of the rounds' medians, and `spread` = the largest minus the smallest
round median.  `separates`: the gap exceeds three times the larger of the two
spreads.  Every timed result of arms a, b, c is decrypted and
compared with np.lexsort's stable ranks (max_abs_err).

usage: lex_rank_bench.py [--keys 2,3] [--rounds 2] [--steps 3] [--warmup 1] [--baseline-lib PATH]
                         [--out FILE.jsonl] [--n 1024 --logn 16] [--summarise]
Appends one JSON line per process to --out (default profiles/lex_rank/lex_rank_bench.jsonl)
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

NEW_SYMBOLS = ('fhe_direct_lex_rank', 'fhe_lex_rank_levels', 'fhe_sub_lex_stacked', 'fhe_mul_lex')
BINARY = 2


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
    N, L, cfg, eps = a.n, a.L, sign_cfg(a.n), 1.0 / a.n
    depth, rots = F.size_parameters(N)
    depth += L - 1
    ctx = F.Context(a.logn, depth, 40, 60, 3, seed=2025)
    ctx.gen_rotation_keys(rots)
    rng = np.random.default_rng([N, L])
    digits = rng.integers(0, N // 2, (L, N))
    rep = min(64, N // 4)
    digits[:, N - rep:] = digits[:, :rep]  # rows tied on every digit
    keyv = [digits[l] * 2.0 / N for l in range(L)]
    order = np.lexsort(keyv[::-1])
    want = np.empty(N)
    want[order] = np.arange(N)
    keys = [ctx.encrypt(v, N) for v in keyv]
    ctx.set_sort_tiebreak(eps)
    ctx.sync()

    S = min(N, (1 << (a.logn - 1)) // N) * N
    Pn, nb = S // N, N // (S // N)
    npb = rank_np(N, Pn)
    masks, offs = {}, {}

    def slots(ct, s):
        ct.set_slots(s)
        return ct

    def vec_rots_opt(baby, b):
        level, out = baby[0].level, None
        for j in range(Pn // npb):
            mk = (b, j, level)
            if mk not in masks:  # encoded once, outside the timed calls (the warm-up call)
                masks[mk] = ctx.encode_masks([(0, npb * j + i, -b * Pn - j * npb, level) for i in range(npb)], S, N)
            o = ctx.compose_rotate(ctx.mul_plain_sum(baby, masks[mk]), N, rots, BINARY, b * Pn + j * npb)
            out = o if out is None else ctx.add(out, o)
        return out

    def composed():
        """arm c: the definition op by op, batch by batch"""
        baby = [[slots(ctx.compose_rotate(k, N, rots, BINARY, i), S) for i in range(npb)] for k in keys]
        dup = [slots(ctx.add_const(k, 0.0), S) for k in keys]
        rank = None
        for b in range(nb):
            d = [ctx.sub(dup[l], vec_rots_opt(baby[l], b)) for l in range(L)]
            ok = (b, d[L - 1].level)
            if ok not in offs:
                offs[ok] = ctx.encode_tiebreak([b], S, N, eps, d[L - 1].level)[0]
            t = ctx.add_const(ctx.sign(ctx.add_plain(d[L - 1], offs[ok]), *cfg), 1.0)
            for l in range(L - 2, -1, -1):
                u = ctx.sign(ctx.add_const(d[l], eps), *cfg)
                w = ctx.sign(ctx.add_const(d[l], -eps), *cfg)
                prod = ctx.mul(ctx.sub(u, w), t)
                t = ctx.add(prod, ctx.mul_const_to(ctx.add_const(w, 1.0), 2.0 ** (L - 1 - l), prod.level))
            rank = t if rank is None else ctx.add(rank, t)
        i = 1
        while (1 << i) <= Pn:
            rank = ctx.add(rank, ctx.compose_rotate(rank, N, rots, BINARY, S >> i))
            i += 1
        return slots(ctx.add_const(ctx.mul_const(rank, 2.0 ** -L), -1.0), N)

    def call():
        if a.child == 'c':
            return composed()
        if a.child == 'd':
            return ctx.direct_sort(keys[-1], N, rots, cfg, mode=1)
        return ctx.lex_rank(keys, eps, N, rots, cfg)

    def once():
        ctx.sync()
        t0 = time.perf_counter()
        out = call()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3, out

    for _ in range(a.warmup):
        once()
    ts = []
    for _ in range(a.steps):
        t, out = once()
        ts.append(t)
    err = None if a.child == 'd' else float(np.max(np.abs(ctx.decrypt(out)[:N] - want)))
    res = dict(arm=a.child, round=a.round, N=N, logn=a.logn, L=L, depth=depth, lib=os.path.basename(F.LIB_PATH),
               fused=os.environ.get('FHE_LEX_FUSED', '1'), steps=a.steps, warmup=a.warmup,
               ms=round(statistics.median(ts), 2), min_ms=round(min(ts), 2), max_ms=round(max(ts), 2),
               level_out=out.level, max_abs_err=err, tied_rows=int(2 * rep))
    print('RESULT ' + json.dumps(res), flush=True)


def summarise(recs, a):
    """recs: {(arm, L): [records]}"""
    summary = dict(N=a.n, logn=a.logn, rounds=a.rounds, steps=a.steps, warmup=a.warmup, cases={})
    for (arm, L), rows in sorted(recs.items()):
        meds = [r['ms'] for r in rows]
        errs = [r['max_abs_err'] for r in rows if r['max_abs_err'] is not None]
        summary['cases'].setdefault(f'L{L}', {})[arm] = dict(
            ms=round(statistics.median(meds), 2), spread=round(max(meds) - min(meds), 2), rounds=meds,
            max_abs_err=max(errs) if errs else None, level_out=rows[0]['level_out'], depth=rows[0]['depth'])
    for case in summary['cases'].values():
        if 'a' not in case:
            continue
        for other, name in (('b', 'fused_vs_plain'), ('c', 'operator_vs_composition')):
            if other in case:
                gap = case[other]['ms'] - case['a']['ms']
                lim = 3 * max(case['a']['spread'], case[other]['spread'])
                case[name] = dict(ratio=round(case[other]['ms'] / case['a']['ms'], 4), separates=bool(abs(gap) > lim),
                                  faster='a' if gap > lim else (other if -gap > lim else None))
        if 'd' in case:
            case['against_rank'] = round(case['a']['ms'] / case['d']['ms'], 3)
    return summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--keys', default='2,3')
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--steps', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=1)
    ap.add_argument('--n', type=int, default=1024)
    ap.add_argument('--logn', type=int, default=16)
    ap.add_argument('--baseline-lib', default=None)
    ap.add_argument('--out', default=os.path.join(HERE, '..', 'profiles', 'lex_rank', 'lex_rank_bench.jsonl'))
    ap.add_argument('--child-timeout', type=int, default=300)
    ap.add_argument('--summarise', action='store_true')
    ap.add_argument('--child', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--L', type=int, default=2, help=argparse.SUPPRESS)
    ap.add_argument('--round', type=int, default=0, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if a.summarise:
        recs = {}
        for ln in open(a.out):
            rec = json.loads(ln)
            if 'arm' in rec:
                recs.setdefault((rec['arm'], rec['L']), []).append(rec)
        print(json.dumps(summarise(recs, a)))
        return

    def run(arm, L, rnd):
        env = dict(os.environ)
        env.pop('FHE_LEX_FUSED', None)
        env.pop('FHE_LIB', None)
        if arm == 'b':
            env['FHE_LEX_FUSED'] = '0'
        if arm == 'c':
            env['FHE_LIB'] = os.path.abspath(a.baseline_lib)
        cmd = [sys.executable, os.path.abspath(__file__), '--child', arm, '--L', str(L), '--round', str(rnd), '--steps',
               str(a.steps), '--warmup', str(a.warmup), '--n', str(a.n), '--logn', str(a.logn)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
        line = next((ln for ln in r.stdout.splitlines() if ln.startswith('RESULT ')), None)
        if r.returncode != 0 or line is None:  # stop here: nothing more is started after a failed process
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f'arm {arm} L {L} round {rnd} failed with status {r.returncode}')
        rec = json.loads(line[7:])
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'a') as f:
            f.write(json.dumps(rec) + '\n')
        print(f"arm {arm} L {L} round {rnd}: {rec['ms']} ms, error {rec['max_abs_err']}", flush=True)
        return rec

    arms = ['a', 'b'] + (['c'] if a.baseline_lib else []) + ['d']
    recs = {}
    for rnd in range(a.rounds):
        for L in [int(v) for v in a.keys.split(',')]:
            for arm in arms:
                recs.setdefault((arm, L), []).append(run(arm, L, rnd))
    summary = summarise(recs, a)
    with open(a.out, 'a') as f:
        f.write(json.dumps(dict(summary=summary)) + '\n')
    print(json.dumps(summary), flush=True)


if __name__ == '__main__':
    main()
