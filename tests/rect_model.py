"""Plaintext model and CPU-oracle compositions of the all-pairs operators between
tables of different sizes (fhe_set_pair_tables; test infrastructure; DESIGN.md
§6.10).

A left table of Nl rows meets a right table of Nr rows, both powers of two.  With
N = max(Nl, Nr), n = min(Nl, Nr), P_ = min(N, ring_slots / N) and P' = min(P_, n)
the layout has S = N P' slots and n / P' comparator batches: slot s of batch b, with
i = s mod N and t = b P' + s // N < n, pairs left row i mod Nl with right row
(i + t) mod Nr.  A ciphertext of n slots viewed at S slots is its own tiling, so
the smaller table enters as it is.  After the sums over batches and the fold over
the P' partitions slot i holds the partial sum over t; for Nl < Nr left row e's sum
is spread over the slots i = e mod Nl and the residue fold v += rotate(v, Nl 2^k),
k < log2(Nr / Nl), collects it.

`pair_shape` and `pair_map` are the layout, `simulate_group_sums` walks it in numpy
(tiling, np.roll, masks, batch sums, both folds), and the `oracle_*_rect` functions
are the operators' compositions on pyoracle op by op: the existing models'
(group_model, running_model, window_model, gather_model) with the batch limit and
the residue fold added -- the definition the GPU is held to, word for word."""
import numpy as np

import gather_model as GA
import group_model as G
import pyoracle as O
import running_model as R
import stable_model as S
import window_model as W

BINARY = S.BINARY


def pair_shape(Nl, Nr, ring_slots):
    """(num_slots, num_partition, num_batch, np, fold_steps); the first four in stable_model.rank_shape's order"""
    N, n = max(Nl, Nr), min(Nl, Nr)
    P = min(min(N, ring_slots // N), n)
    assert P >= 1, (Nl, Nr, ring_slots)
    fold = 0
    while (Nl << fold) < Nr:
        fold += 1
    return N * P, P, n // P, S.rank_np(N, P), fold


def pair_map(Nl, Nr, ring_slots):
    """(left row [nb][S], right row [nb][S]) of every slot of every batch"""
    S_, P, nb, _, _ = pair_shape(Nl, Nr, ring_slots)
    N = max(Nl, Nr)
    s = np.arange(S_)
    i = s % N
    left = np.tile(i % Nl, (nb, 1))
    right = np.array([(i + b * P + s // N) % Nr for b in range(nb)])
    return left, right


def _shift(x, S_, N, P, npb, b):
    """vecRotsOpt of batch b on the tiled vector x [S]: baby steps, masks, giant steps"""
    out = np.zeros(S_)
    for j in range(P // npb):
        t = np.zeros(S_)
        for i in range(npb):
            m = np.zeros(S_)
            m[(npb * j + i) * N:(npb * j + i + 1) * N] = 1.0
            t += np.roll(x, -i) * np.roll(m, b * P + j * npb)  # rotate(x, i) under the mask rotated right
        out += np.roll(t, -(b * P + j * npb))
    return out


def simulate_group_sums(kl, kr, cols, eps, ring_slots):
    """(sums [P][Nl], counts [Nl]): the whole layout in numpy with the exact indicator"""
    Nl, Nr = len(kl), len(kr)
    S_, P, nb, npb, fold = pair_shape(Nl, Nr, ring_slots)
    N = max(Nl, Nr)
    tile = lambda v: np.tile(np.asarray(v, dtype=np.float64), S_ // len(v))
    dup, right, tcols = tile(kl), tile(kr), [tile(c) for c in cols]
    accs, cnt = [np.zeros(S_) for _ in cols], np.zeros(S_)
    for b in range(nb):
        m = (np.abs(dup - _shift(right, S_, N, P, npb, b)) < eps).astype(np.float64)
        cnt += m
        for p, c in enumerate(tcols):
            accs[p] += m * _shift(c, S_, N, P, npb, b)

    def folds(v):
        i = 1
        while (1 << i) <= P:
            v = v + np.roll(v, -(S_ >> i))
            i += 1
        for k in range(fold):
            v = v + np.roll(v, -(Nl << k))
        return v[:Nl]

    return np.array([folds(a) for a in accs]).reshape(len(cols), Nl), folds(cnt)


def sentinel_pad(keys, N, eps, which=0):
    """a table's keys padded to N rows by sentinels >= 2 eps from every real key and from each other; the
    two tables of a call take different `which`, so that their sentinels do not match one another"""
    pad = -2.0 * eps * (1 + 2 * np.arange(N - len(keys)) + which)
    return np.concatenate([np.asarray(keys, dtype=np.float64), pad])


# ------------------------------------------------- compositions on pyoracle --
class _Layout:
    """the shared walk of the compositions: the shape, the views and shifts, the folds"""

    def __init__(self, orc, Nl, Nr, rots):
        self.orc, self.Nl, self.Nr, self.rots = orc, Nl, Nr, rots
        self.N = max(Nl, Nr)
        self.S, self.P, self.nb, self.npb, self.fold_steps = pair_shape(Nl, Nr, orc.n // 2)

    def view(self, ct):
        return G._with_slots(self.orc, ct, self.S)

    def baby(self, x):
        return [self.view(self.orc.compose_rotate(x, self.N, self.rots, BINARY, i)) for i in range(self.npb)]

    def shifted(self, baby, b):
        return G._vec_rots_opt(self.orc, baby, self.N, self.rots, self.S, self.P, self.npb, b)

    def fold(self, acc):
        orc, i = self.orc, 1
        while (1 << i) <= self.P:
            acc = orc.add(acc, orc.compose_rotate(acc, self.N, self.rots, BINARY, self.S >> i))
            i += 1
        for k in range(self.fold_steps):
            acc = orc.add(acc, orc.compose_rotate(acc, self.N, self.rots, BINARY, self.Nl << k))
        return acc

    def close(self, acc):
        acc.set_slots(self.Nl)
        return acc


def _add(orc, acc, x):
    return x if acc is None else orc.add(acc, x)


def oracle_group_sums_rect(orc, okl, okr, ocols, Nl, Nr, rots, cfg, eps, count):
    """group_model.oracle_group_sums between tables of Nl and Nr rows: (outs, count or None)"""
    L = _Layout(orc, Nl, Nr, rots)
    Lm = okl.level + 1 + G.sign_depth(cfg)
    kbaby = L.baby(okr)
    cbaby = [L.baby(orc.mul_const_to(c, 0.5, Lm - 1)) for c in ocols]
    dup = L.view(okl)
    accs, cnt = [None] * len(ocols), None
    for b in range(L.nb):
        d = orc.sub(dup, L.shifted(kbaby, b))
        m = orc.add(orc.sign(orc.add_const(d, eps), *cfg), orc.sign(orc.add_const(orc.negate(d), eps), *cfg))
        assert m.level == Lm
        if count:
            cnt = _add(orc, cnt, m)
        for p in range(len(ocols)):
            accs[p] = _add(orc, accs[p], orc.mul(m, L.shifted(cbaby[p], b)))
    outs = [L.close(L.fold(a)) for a in accs]
    return outs, (L.close(orc.mul_const(L.fold(cnt), 0.5)) if count else None)


def _order_indicator(orc, cfg, eps, mode, d, dup_lo, sk):
    """running_model's indicator of one batch (2 or 0) for LE, LT and BETWEEN"""
    if mode == R.BETWEEN:
        u = orc.add_const(d, eps)
        w = orc.add_const(orc.sub(dup_lo, sk), -eps)
        return orc.sub(orc.sign(u, *cfg), orc.sign(w, *cfg))
    assert mode in (R.LE, R.LT), 'the rows mode has no meaning between tables of different sizes'
    return orc.add_const(orc.sign(orc.add_const(d, eps if mode == R.LE else -eps), *cfg), 1.0)


def oracle_running_sums_rect(orc, okl, okr, ocols, Nl, Nr, rots, cfg, eps, mode, count, olo=None):
    """running_model.oracle_running_sums (LE, LT, BETWEEN) between tables of Nl and Nr rows"""
    L = _Layout(orc, Nl, Nr, rots)
    Lm = okl.level + 1 + G.sign_depth(cfg)
    kbaby = L.baby(okr)
    cbaby = [L.baby(orc.mul_const_to(c, 0.5, Lm - 1)) for c in ocols]
    dup = L.view(okl)
    dup_lo = L.view(olo) if mode == R.BETWEEN else None
    accs, cnt = [None] * len(ocols), None
    for b in range(L.nb):
        sk = L.shifted(kbaby, b)
        a = _order_indicator(orc, cfg, eps, mode, orc.sub(dup, sk), dup_lo, sk)
        assert a.level == Lm
        if count:
            cnt = _add(orc, cnt, orc.mul_const(a, 0.5))
        for p in range(len(ocols)):
            accs[p] = _add(orc, accs[p], orc.mul(a, L.shifted(cbaby[p], b)))
    outs = [L.close(L.fold(a)) for a in accs]
    return outs, (L.close(L.fold(cnt)) if count else None)


def oracle_window_sums_rect(orc, opl, opr, ocols, Nl, Nr, rots, cfg, eps, mode, count, ool=None, oor=None, olo=None):
    """window_model.oracle_window_sums (LE, LT, BETWEEN, GROUP) between tables of Nl and Nr rows"""
    L = _Layout(orc, Nl, Nr, rots)
    Gn = len(opl)
    F = W.nfactors(Gn, mode)
    assert 2 <= F <= 4 and len(opr) == Gn
    _, Lm, La, _, out_level = W.levels(opl[0].level, F, cfg)
    cbaby = [L.baby(orc.mul_const_to(c, 2.0 ** -F, La - 1)) for c in ocols]
    pbaby = [L.baby(k) for k in opr]
    pdup = [L.view(k) for k in opl]
    if mode != W.GROUP:
        obaby, odup = L.baby(oor), L.view(ool)
        odup_lo = L.view(olo) if mode == W.BETWEEN else None
    accs, cnt = [None] * len(ocols), None
    for b in range(L.nb):
        phi = []
        for g in range(Gn):
            d = orc.sub(pdup[g], L.shifted(pbaby[g], b))
            phi.append(orc.sub(orc.sign(orc.add_const(d, eps), *cfg), orc.sign(orc.add_const(d, -eps), *cfg)))
        if mode != W.GROUP:
            sk = L.shifted(obaby, b)
            phi.append(_order_indicator(orc, cfg, eps, mode, orc.sub(odup, sk), odup_lo, sk))
        assert all(x.level == Lm for x in phi)
        if F == 2:
            a = orc.mul(phi[0], phi[1])
        elif F == 3:
            a = orc.mul(phi[0], orc.mul(phi[1], phi[2]))
        else:
            a = orc.mul(orc.mul(phi[0], phi[1]), orc.mul(phi[2], phi[3]))
        assert a.level == La
        if count:
            cnt = _add(orc, cnt, orc.mul_const(a, 2.0 ** -F))
        for p in range(len(ocols)):
            accs[p] = _add(orc, accs[p], orc.mul(a, L.shifted(cbaby[p], b)))
    outs = [L.close(L.fold(a)) for a in accs]
    assert all(o.level == out_level for o in outs)
    return outs, (L.close(L.fold(cnt)) if count else None)


def oracle_gather_rect(orc, opl, opr, ocols, offsets, Nl, Nr, rots, present=False, sum_offsets=False):
    """gather_model.oracle_gather between tables of Nl and Nr rows: positions, offsets and the series are
    those of N = max(Nl, Nr); (outs column-major, present flags)"""
    L = _Layout(orc, Nl, Nr, rots)
    N = L.N
    _, Ls, _, out_level = GA.levels(opl.level, N)
    coeffs = O.doubled_sinc(N)
    Ko = 1 if sum_offsets else len(offsets)
    rbaby = L.baby(opr)
    cbaby = [L.baby(orc.mul_const_to(c, 1.0, Ls - 1)) for c in ocols]
    dup = L.view(opl)
    accs, cnt = [None] * (len(ocols) * Ko), [None] * Ko
    for b in range(L.nb):
        base = orc.sub(dup, L.shifted(rbaby, b))
        rs = []
        for o in offsets:
            d = orc.add_const(base, float(o))
            if o < 0:
                d = orc.negate(d)
            rs.append(orc.cheb(orc.mul_const(d, 1.0 / N / 2), coeffs, -1.0, 1.0))
            assert rs[-1].level == Ls
        if sum_offsets:
            tot = rs[0]
            for r in rs[1:]:
                tot = orc.add(tot, r)
            rs = [tot]
        if present:
            for k in range(Ko):
                cnt[k] = _add(orc, cnt[k], rs[k])
        for p in range(len(ocols)):
            sc = L.shifted(cbaby[p], b)
            for k in range(Ko):
                accs[p * Ko + k] = _add(orc, accs[p * Ko + k], orc.mul(rs[k], sc))
    outs = [L.close(L.fold(a)) for a in accs]
    assert all(a.level == out_level for a in outs)
    return outs, ([L.close(L.fold(c)) for c in cnt] if present else [])


# ------------------------------------------------------------------ cases --
OFFSETS = (-1, 0, 1)


def inputs(Nl, Nr, seed):
    """The plaintext tables of a case.  Keys lie on the grid 1 / 4N below 1 / 2 (N = max(Nl, Nr)), eps = 1 / 8N
    and the sign configuration is the sort's for 8N values, whose smallest difference is that eps.  The
    smaller table holds distinct keys; the larger one draws from twice as many grid points, so that about
    half of its rows have a partner, some share one and some have none.  k2 is a second key of two values
    2 eps apart, lo / hi the band [k - 2 / 4N, k + 2 / 4N] of every left row, pl / pr integer positions below
    N, the right ones distinct, and two columns."""
    N, n = max(Nl, Nr), min(Nl, Nr)
    rng = np.random.default_rng([seed, Nl, Nr])
    grid = np.arange(2 * N) / (4.0 * N)
    perm = rng.permutation(grid)
    small, large = perm[:n], rng.choice(perm[:2 * n], N)
    kl, kr = (large, small) if Nl >= Nr else (small, large)
    eps = 1.0 / (8 * N)
    cnt = (np.abs(kl[:, None] - kr[None, :]) < eps).sum(axis=1)
    assert (cnt == 0).any() and (cnt > 0).any(), (Nl, Nr, seed, cnt)
    d = dict(Nl=Nl, Nr=Nr, N=N, eps=eps, cfg=S.sign_cfg(8 * N), kl=kl, kr=kr,
             k2l=rng.integers(0, 2, Nl) * 2.0 * eps, k2r=rng.integers(0, 2, Nr) * 2.0 * eps,
             lo=kl - 2.0 / (4 * N), hi=kl + 2.0 / (4 * N),
             pl=rng.integers(0, N, Nl).astype(np.float64), pr=rng.permutation(N)[:Nr].astype(np.float64),
             cols=[rng.uniform(-1, 1, Nr), np.arange(Nr) / Nr])
    for a in R.sign_arguments(d['hi'], kr, R.BETWEEN, eps, d['lo']):
        assert np.max(np.abs(a)) <= 1.0
    return d


def exact_results(d):
    """the exact sums of every operator of `oracle_results`, by the square models' definitions"""
    kl, kr, cols, eps = d['kl'], d['kr'], d['cols'], d['eps']
    gout, gpres = GA.exact(d['pl'], d['pr'], cols[:1], OFFSETS)
    return {
        'group': G.exact(kl, kr, cols, eps),
        'run_le': R.exact(kl, kr, cols[:1], R.LE, eps),
        'run_between': R.exact(d['hi'], kr, cols[:1], R.BETWEEN, eps, d['lo']),
        'win_le': W.exact([d['k2l']], [d['k2r']], cols[:1], W.LE, eps, kl, kr),
        'win_group': W.exact([kl, d['k2l']], [kr, d['k2r']], cols[:1], W.GROUP, eps),
        'gather': (gout[0], gpres),
        'gather_sum': (gout[0].sum(axis=0, keepdims=True), gpres.sum(axis=0, keepdims=True)),
    }


def encrypt_inputs(orc, d):
    """the case's ciphertexts on the oracle: left operands in Nl slots, right operands and columns in Nr,
    the columns entering at levels 0 and 1"""
    Nl, Nr = d['Nl'], d['Nr']
    e = {k: orc.encrypt(d[k], Nl) for k in ('kl', 'k2l', 'lo', 'hi', 'pl')}
    e.update({k: orc.encrypt(d[k], Nr) for k in ('kr', 'k2r', 'pr')})
    e['cols'] = [orc.encrypt(c, Nr, lv) for lv, c in enumerate(d['cols'])]
    return e


def oracle_results(orc, rots, d, e, ops=None):
    """{name: (outs, count or flags)} of every operator's composition; ops: the names wanted (all by default)"""
    Nl, Nr, cfg, eps = d['Nl'], d['Nr'], d['cfg'], d['eps']
    c1 = e['cols'][:1]
    todo = {
        'group': lambda: oracle_group_sums_rect(orc, e['kl'], e['kr'], e['cols'], Nl, Nr, rots, cfg, eps, True),
        'run_le': lambda: oracle_running_sums_rect(orc, e['kl'], e['kr'], c1, Nl, Nr, rots, cfg, eps, R.LE, True),
        'run_between': lambda: oracle_running_sums_rect(orc, e['hi'], e['kr'], c1, Nl, Nr, rots, cfg, eps, R.BETWEEN,
                                                        True, e['lo']),
        'win_le': lambda: oracle_window_sums_rect(orc, [e['k2l']], [e['k2r']], c1, Nl, Nr, rots, cfg, eps, W.LE, True,
                                                  e['kl'], e['kr']),
        'win_group': lambda: oracle_window_sums_rect(orc, [e['kl'], e['k2l']], [e['kr'], e['k2r']], c1, Nl, Nr, rots,
                                                     cfg, eps, W.GROUP, True),
        'gather': lambda: oracle_gather_rect(orc, e['pl'], e['pr'], c1, OFFSETS, Nl, Nr, rots, present=True),
        'gather_sum': lambda: oracle_gather_rect(orc, e['pl'], e['pr'], c1, OFFSETS, Nl, Nr, rots, present=True,
                                                 sum_offsets=True),
    }
    return {k: f() for k, f in todo.items() if ops is None or k in ops}


def largest_error(res, want):
    """largest |decrypted - exact| of one operator's (outs, count or flags) against exact_results' entry"""
    outs, cnt = res
    wsum, wcnt = want
    cnts = cnt if isinstance(cnt, list) else [cnt]
    err = max(np.max(np.abs(o.decrypt() - w)) for o, w in zip(outs, np.reshape(wsum, (len(outs), -1))))
    return max(err, max(np.max(np.abs(c.decrypt() - w)) for c, w in zip(cnts, np.reshape(wcnt, (len(cnts), -1)))))


# (Nl, Nr, log2 of the ring) of the GPU cases (tests/test_gpu_rect_tables.py): the smallest shapes that reach
# each branch of the layout; True where every operator runs, False where the group sum alone does
SHAPES = {(8, 2, 12): True, (2, 8, 12): True, (64, 32, 12): False, (32, 64, 12): False, (64, 32, 11): True,
          (32, 64, 11): True}
INPUT_SEED = 7


def context_seed(Nl, Nr, logn):
    return 1000 + 3 * Nl + Nr + 100 * logn


def oracle_case(Nl, Nr, logn, ops=None):
    """the oracle half of a case (no GPU): context, keys, inputs, ciphertexts, compositions and exact sums"""
    d = inputs(Nl, Nr, INPUT_SEED)
    depth, rots = O.size_parameters(d['N'])
    orc = O.Context(logn, depth, 40, 60, 3, seed=context_seed(Nl, Nr, logn))
    orc.gen_rotation_keys(rots)
    e = encrypt_inputs(orc, d)
    if ops is None and not SHAPES.get((Nl, Nr, logn), True):
        ops = ['group']
    return dict(d=d, depth=depth, rots=rots, orc=orc, enc=e, res=oracle_results(orc, rots, d, e, ops),
                want=exact_results(d), logn=logn)


def padded_tables(d):
    """(kl, kr, cols) of today's square call: the smaller table padded to N rows by sentinel keys and zero
    columns (sentinel_pad); the exact sums of the first Nl left rows are the unpadded tables'"""
    N = d['N']
    kl, kr = sentinel_pad(d['kl'], N, d['eps'], 0), sentinel_pad(d['kr'], N, d['eps'], 1)
    cols = [np.concatenate([c, np.zeros(N - len(c))]) for c in d['cols']]
    assert np.abs(kl[:, None] - kr[None, :]).max() + d['eps'] <= 1.0
    psums, pcnt = G.exact(kl, kr, cols, d['eps'])
    wsums, wcnt = G.exact(d['kl'], d['kr'], d['cols'], d['eps'])
    assert np.array_equal(psums[:, :d['Nl']], wsums) and np.array_equal(pcnt[:d['Nl']], wcnt)
    return kl, kr, cols


def encrypt_padded(c):
    """the padded tables on the case's oracle context: (left key, right key, columns at levels 0 and 1), N slots each"""
    d, orc = c['d'], c['orc']
    kl, kr, cols = padded_tables(d)
    return orc.encrypt(kl, d['N']), orc.encrypt(kr, d['N']), [orc.encrypt(v, d['N'], lv) for lv, v in enumerate(cols)]


def oracle_padded_group_sums(c):
    """group_model.oracle_group_sums of the padded tables (the square call's definition): (outs, count)"""
    d = c['d']
    okl, okr, ocols = encrypt_padded(c)
    return G.oracle_group_sums(c['orc'], okl, okr, ocols, d['N'], c['rots'], d['cfg'], d['eps'], True)
