"""The launch ledger of the all-pairs operators (tests/golden/pair_ledger.json).

Every operator that walks the all-pairs layout -- direct_sort, sort_columns,
select, group_sum, running_sum, window_sum, gather, lex_rank -- is run at N = 8
(one comparator batch) and N = 64 (two) in ring 2^12, under four settings of
(lanes, stack, column members), and what the library did is written down:

* the kernel clock's table without its times: launches and bytes per kernel
  and per phase, op_bytes per phase;
* counters();
* (level, slots, limbs, scale) and the SHA-256 of the words of every output;
* at one lane, the pool's peak live bytes.  The pool's peak is never reset, so
  the figure of a case is the largest since the process began, with the cases
  in the fixed order of CONFIGS and CASES.

tests/test_gpu_pair_ledger.py runs record() on the library under test and
compares it with the committed file field by field (the peak: no larger).

    python tests/golden/make_pair_ledger.py OUT.json          one recording
    python tests/golden/make_pair_ledger.py --merge A B OUT   keep what agrees

The committed file is two recordings of the commit before the operators moved
onto one driver, merged; its header names the fields the two disagreed on.
FHE_LIB selects the library (fhe-sorting_amd/fhesort.py).
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
REPO = os.path.dirname(TESTS)
for p in (os.path.join(REPO, 'oracle'), os.path.join(REPO, 'fhe-sorting_amd'), TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)

NS = (8, 64)
SEED = {8: 818, 64: 874}
OFFSETS = (-1, 0, 2)
# (name, lanes, stack, column members): one chunk per lane; two lanes; more than
# one chunk per lane; more than one column group (a member bound below the
# three columns' members)
# stack1 comes first and window_4 last: the peak only grows, so the smaller cases are measured before the larger
CONFIGS = (('stack1', 1, 1, None), ('members2', 1, 32, 2), ('lanes1', 1, 32, None), ('lanes2', 2, 32, None))
CASES = ('sort_rank', 'sort_rank_tiebreak', 'sort', 'sort_tiebreak', 'sort_columns', 'select', 'group_sum',
         'running_rows', 'running_between', 'window_2', 'gather', 'gather_sum_offsets', 'lex_rank', 'window_4')


def _ct(c):
    i = c.info()
    return {'level': i['level'], 'slots': i['slots'], 'limbs': i['limbs'], 'scale': i['scale'],
            'sha256': hashlib.sha256(c.data().tobytes()).hexdigest()}


def _table(stats):
    out = {}
    for k, v in stats.items():
        out[k] = {f: v[f] for f in ('launches', 'bytes', 'op_bytes') if f in v}
    return out


def record(N):
    """{'<config>/<case>': {'clock', 'counters', 'outputs'[, 'peak']}} of one N"""
    import numpy as np

    import fhesort as F
    import lex_model as X
    import pyoracle as O
    import running_model as R
    import stable_model as M
    import window_model as W

    cfg, eps = M.sign_cfg(N), 1.0 / N
    depth, rots = F.size_parameters(N)
    depth = max(depth + 2, F.window_sum_levels(0, 4, cfg)[1])  # three lexicographic keys; four window factors
    seed = SEED[N]
    orc = O.Context(12, depth, 40, 60, 3, seed=seed)
    orc.gen_rotation_keys(rots)
    gpu = F.Context(12, depth, 40, 60, 3, seed=seed, keygen=False)
    gpu.load_keys_from(orc, rots)
    assert M.rank_shape(N, orc.n // 2)[2] == (1 if N == 8 else 2)
    rng = np.random.default_rng(seed)
    enc = lambda v, level=0: gpu.from_oracle(orc.encrypt(np.asarray(v, dtype=np.float64), N, level))

    key = enc(M.tied_input(N, M.SEEDS[N]))
    plain_key = enc(rng.permutation(N) / N)
    vals = [rng.uniform(-1, 1, N), np.arange(N) / N, rng.uniform(-1, 1, N)]

    def cols_at(col_max):
        return [enc(v, lv) for v, lv in zip(vals, (0, 1, col_max))]

    gcols = cols_at(F.group_sum_levels(0, cfg)[0])
    kw, lo, hi, _, _ = R.window_input(N)
    gkw, glo, ghi = enc(kw), enc(lo), enc(hi)
    win = {}
    for nf, G in ((2, 1), (4, 3)):  # G partition keys and the order key, ROWS
        parts, t, _, _, _, _ = W.partitioned_input(N, G)
        win[nf] = ([enc(p) for p in parts], enc(t), cols_at(F.window_sum_levels(0, nf, cfg)[0]))
    lex_keys = [enc(k) for k in X.tied_keys(N, 3, X.KEY_SEED[(N, 3)])]
    targets = [N - 1, 0]

    # the gather's positions: a tie-broken rank, made once before anything is recorded
    gpu.set_sort_tiebreak(eps)
    rank = gpu.direct_sort(key, N, rots, cfg, mode=1)
    gpu.set_sort_tiebreak(0.0)
    gather_cols = cols_at(F.gather_levels(rank.level, N)[0])

    def tiebreak(fn):
        gpu.set_sort_tiebreak(eps)
        try:
            return fn()
        finally:
            gpu.set_sort_tiebreak(0.0)

    def flat(res):
        outs, extra = res
        return list(outs) + (list(extra) if isinstance(extra, (list, tuple)) else [extra])

    run = {
        'sort_rank': lambda: [gpu.direct_sort(plain_key, N, rots, cfg, mode=1)],
        'sort_rank_tiebreak': lambda: tiebreak(lambda: [gpu.direct_sort(key, N, rots, cfg, mode=1)]),
        'sort': lambda: [gpu.direct_sort(plain_key, N, rots, cfg, mode=0)],
        'sort_tiebreak': lambda: tiebreak(lambda: [gpu.direct_sort(key, N, rots, cfg, mode=0)]),
        'sort_columns': lambda: gpu.direct_sort_columns(plain_key, gcols, N, rots, cfg),
        'select': lambda: [gpu.direct_select(plain_key, targets, N, rots, cfg)],
        'group_sum': lambda: flat(gpu.group_sum(key, key, gcols, eps, N, rots, cfg, count=True)),
        'running_rows': lambda: flat(gpu.running_sum(key, key, gcols, eps, N, rots, cfg, mode=F.RUN_ROWS, count=True)),
        'running_between': lambda: flat(gpu.running_sum(ghi, gkw, gcols, eps, N, rots, cfg, mode=F.RUN_BETWEEN, lo=glo,
                                                        count=True)),
        'window_2': lambda: flat(gpu.window_sum(win[2][0], win[2][0], win[2][2], eps, N, rots, cfg, order_left=win[2][1],
                                                order_right=win[2][1], mode=F.WIN_ROWS, count=True)),
        'gather': lambda: flat(gpu.gather(rank, rank, gather_cols, OFFSETS, N, rots, present=True)),
        'gather_sum_offsets': lambda: flat(gpu.gather(rank, rank, gather_cols, OFFSETS, N, rots, present=True,
                                                      sum_offsets=True)),
        'lex_rank': lambda: [gpu.lex_rank(lex_keys, eps, N, rots, cfg)],
        'window_4': lambda: flat(gpu.window_sum(win[4][0], win[4][0], win[4][2], eps, N, rots, cfg, order_left=win[4][1],
                                                order_right=win[4][1], mode=F.WIN_ROWS, count=True)),
    }
    assert tuple(run) == CASES

    ledger = {}
    for name, lanes, stack, members in CONFIGS:
        gpu.set_sort_lanes(lanes)
        gpu.set_sort_stack(stack)
        gpu.set_sort_column_members(F.SORT_COLUMN_MEMBERS_DEFAULT if members is None else members)
        for case in CASES:
            gpu.sync()
            gpu.reset_counters()
            with F.KernelClock(gpu) as clk:
                outs = run[case]()
            entry = {'clock': _table(clk.stats), 'counters': gpu.counters(), 'outputs': [_ct(o) for o in outs]}
            if lanes == 1:
                entry['peak'] = gpu.pool_stats()['peak']
            ledger[f'{name}/{case}'] = entry
            del outs
            print(f'N={N} {name}/{case} ok', flush=True)
    return ledger


def merge(a, b):
    """the fields on which two recordings agree, and the paths of the others"""
    dropped = []

    def walk(x, y, path):
        if isinstance(x, dict) and isinstance(y, dict):
            out = {}
            for k in x:
                if k not in y:
                    dropped.append(f'{path}/{k}')
                    continue
                v = walk(x[k], y[k], f'{path}/{k}')
                if v is not None:
                    out[k] = v
            dropped.extend(f'{path}/{k}' for k in y if k not in x)
            return out
        if x == y:
            return x
        dropped.append(path)
        return None

    return walk(a, b, ''), dropped


COUNTERS = ('hmult', 'keyswitch', 'rotations', 'rescale', 'ptmult', 'constmult', 'opbytes')
CT_FIELDS = ('level', 'slots', 'limbs', 'scale', 'sha256')
CLOCK_FIELDS = ('launches', 'bytes', 'op_bytes')


def dump(doc, path):
    """The file form: the kernel and phase names once ('names'), every distinct
    clock table once ('tables': rows of [name index, launches, bytes(, op_bytes)]),
    and a case as {'clock': table index, 'counters': COUNTERS' values, 'outputs':
    rows of CT_FIELDS' values[, 'peak']}.  A field that merge() dropped is null.
    One table and one case per line."""
    names = sorted({k for c in doc['cases'].values() for e in c.values() for k in e.get('clock', {})})
    index = {k: i for i, k in enumerate(names)}
    tables, cases = {}, {}
    for N, c in doc['cases'].items():
        cases[N] = {}
        for key, e in c.items():
            rows = [[index[k]] + [v.get(f) for f in CLOCK_FIELDS if f in v or f != 'op_bytes']
                    for k, v in sorted(e.get('clock', {}).items())]
            packed = {'clock': tables.setdefault(json.dumps(rows, separators=(',', ':')), len(tables)),
                      'counters': [e.get('counters', {}).get(f) for f in COUNTERS],
                      'outputs': None if 'outputs' not in e else [[o[f] for f in CT_FIELDS] for o in e['outputs']]}
            if 'peak' in e:
                packed['peak'] = e['peak']
            cases[N][key] = packed
    js = lambda x: json.dumps(x, separators=(',', ':'))
    with open(path, 'w') as f:
        f.write('{"header":' + json.dumps(doc['header'], sort_keys=True) + ',\n"names":' + js(names) + ',\n"tables":[\n')
        f.write(',\n'.join(tables) + '\n],\n"cases":{\n')
        f.write(',\n'.join(js(N) + ':{\n' + ',\n'.join(js(k) + ':' + js(e) for k, e in c.items()) + '\n}'
                           for N, c in cases.items()))
        f.write('\n}}\n')


def load(path):
    """{'header', 'cases'} with every case in record()'s form; null fields left out"""
    with open(path) as f:
        doc = json.load(f)
    names, cases = doc['names'], {}
    for N, c in doc['cases'].items():
        cases[N] = {}
        for key, e in c.items():
            clock = {}
            for row in doc['tables'][e['clock']]:
                clock[names[row[0]]] = {f: v for f, v in zip(CLOCK_FIELDS, row[1:]) if v is not None}
            out = {'clock': clock, 'counters': {f: v for f, v in zip(COUNTERS, e['counters']) if v is not None}}
            if e['outputs'] is not None:
                out['outputs'] = [dict(zip(CT_FIELDS, o)) for o in e['outputs']]
            if 'peak' in e:
                out['peak'] = e['peak']
            cases[N][key] = out
    return {'header': doc['header'], 'cases': cases}


def main(argv):
    if argv and argv[0] == '--merge':
        a, b = (load(p) for p in argv[1:3])
        cases, dropped = merge(a['cases'], b['cases'])
        doc = {'header': {'what': 'launch ledger of the all-pairs operators; see tests/golden/make_pair_ledger.py',
                          'recordings': 2, 'dropped': dropped}, 'cases': cases}
        out = argv[3]
    else:
        doc = {'header': {'recordings': 1, 'dropped': []}, 'cases': {str(N): record(N) for N in NS}}
        out = argv[0]
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    dump(doc, out)
    print('wrote', out, 'dropped', doc['header']['dropped'])


if __name__ == '__main__':
    main(sys.argv[1:])
