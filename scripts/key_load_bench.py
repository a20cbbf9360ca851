#!/usr/bin/env python3
"""Key traffic of the competition CLI's context (ring 2^17, depth 44, 40-bit
scaling: src/config.json) in the full and the seeded wire format (kinds 3 / 4
against 7 / 8, csrc/wire/wire.hpp) on one MI355X.

The context holds the relinearisation key and 4 rotation keys (about 1.9 GB in
full).  Keys are generated once without and once with a public seed (keygen
seconds: the host's uniform sampling against the expansion kernel), the seeded
context's keys are written in both formats, and a context rebuilt from the
context file loads each format --loads times, alternating, after one untimed
load of each so the page cache is warm for both; each timing ends at fhe_sync.
The expansion kernel alone is timed with HIP events (fhe_time_kernel): one
digit's [nq + K][n] words per launch.

Conditions checked (exit status 1 otherwise): the seeded files have exactly the
derived size, 6 + digits nall n resp. 6 + count (1 + digits nall n) body words;
the median seeded load is no slower than the median full load; and the
eval-mult key loaded from the seeded file re-serialises to the full file.

usage: key_load_bench.py [--logn 17] [--depth 44] [--loads 5] [--dir D]
Prints one JSON line.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'fhe-sorting_amd'))
import fhesort as F  # noqa: E402

ROTS = [1, 2, 4, 8]
COPY_RATE = 5.94e12  # bytes/s moved by the grid-stride 16-B copy (scripts/row_pattern.hip)


def timed(f):
    t0 = time.perf_counter()
    f()
    return time.perf_counter() - t0


def keygen(ctx):
    ctx.keygen()
    ctx.gen_rotation_keys(ROTS)
    ctx.sync()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--logn', type=int, default=17)
    ap.add_argument('--depth', type=int, default=44)
    ap.add_argument('--loads', type=int, default=5)
    ap.add_argument('--dir', default=None, help='where the key files go (default: a temporary directory, removed)')
    a = ap.parse_args()
    d = a.dir or tempfile.mkdtemp(prefix='key_load_bench_')
    os.makedirs(d, exist_ok=True)
    p = {k: os.path.join(d, k + '.bin') for k in ('cc', 'mult', 'rot', 'mult_seeded', 'rot_seeded')}
    try:
        # both keygen paths once on a small ring, so neither timed one pays for loading the kernels
        for pub in (None, bytes(32)):
            warm = F.Context(12, 6, 40, 60, 3, seed=1, keygen=False)
            if pub:
                warm.set_public_seed(pub)
            keygen(warm)
            warm.close()
        plain = F.Context(a.logn, a.depth, 40, 60, 3, seed=2025, keygen=False)
        keygen_plain = timed(lambda: keygen(plain))
        plain.close()
        ctx = F.Context(a.logn, a.depth, 40, 60, 3, seed=2025, keygen=False)
        ctx.set_public_seed(bytes(range(32)))
        keygen_seeded = timed(lambda: keygen(ctx))
        nall, n, digits = ctx.nq + ctx.K, ctx.n, ctx.digits
        kernel = F.time_kernel(ctx, 'expand_uniform', ctx.nq, 20)
        ctx.serialize(p['cc'])
        ctx.serialize_eval_mult_key(p['mult'])
        ctx.serialize_eval_automorphism_key(p['rot'])
        ctx.serialize_eval_mult_key_seeded(p['mult_seeded'])
        ctx.serialize_eval_automorphism_key_seeded(p['rot_seeded'])
        ctx.close()
        size = {k: os.path.getsize(v) for k, v in p.items() if k != 'cc'}
        half = digits * nall * n
        derived = {'mult_seeded': (8 + 6 + half + 1) * 8, 'rot_seeded': (8 + 6 + len(ROTS) * (1 + half) + 1) * 8}

        loader = F.Context.deserialize(p['cc'])

        def load(fmt):
            loader.sync()
            t0 = time.perf_counter()
            loader.deserialize_eval_mult_key(p['mult' + fmt])
            loader.deserialize_eval_automorphism_key(p['rot' + fmt])
            loader.sync()
            return time.perf_counter() - t0

        for fmt in ('', '_seeded'):
            load(fmt)
        times = {'': [], '_seeded': []}
        for _ in range(a.loads):
            for fmt in ('', '_seeded'):
                times[fmt].append(load(fmt))
        # what the seeded load left on the device is what was generated: the full
        # eval-mult file re-serialised from it, byte for byte
        again = os.path.join(d, 'mult_again.bin')
        loader.deserialize_eval_mult_key(p['mult_seeded'])
        loader.serialize_eval_mult_key(again)
        ok_words = open(again, 'rb').read() == open(p['mult'], 'rb').read()
        loader.close()
        full_med, seeded_med = statistics.median(times['']), statistics.median(times['_seeded'])
        rate = kernel['bytes'] / (kernel['avg_ms'] * 1e-3)
        ok_size = all(size[k] == v for k, v in derived.items())
        ok_load = seeded_med <= full_med
        print(json.dumps(dict(
            logn=a.logn, depth=a.depth, nall=nall, digits=digits, keys=1 + len(ROTS),
            file_bytes=dict(full=size['mult'] + size['rot'], seeded=size['mult_seeded'] + size['rot_seeded'],
                            derived_seeded=sum(derived.values())),
            load_s=dict(full_median=round(full_med, 4), seeded_median=round(seeded_med, 4),
                        full=[round(t, 4) for t in times['']], seeded=[round(t, 4) for t in times['_seeded']]),
            expand_kernel=dict(ms=round(kernel['avg_ms'], 4), bytes=int(kernel['bytes']),
                               written_GBps=round(rate / 1e9, 1), frac_copy_rate=round(rate / COPY_RATE, 4)),
            keygen_s=dict(unseeded=round(keygen_plain, 3), seeded=round(keygen_seeded, 3)),
            ok=dict(file_size=ok_size, seeded_load_not_slower=ok_load, seeded_load_same_words=ok_words))),
            flush=True)
        return 0 if ok_size and ok_load and ok_words else 1
    finally:
        if not a.dir:
            shutil.rmtree(d, ignore_errors=True)


if __name__ == '__main__':
    sys.exit(main())
