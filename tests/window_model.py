"""Plaintext model and CPU-oracle composition of the window sums
(fhe_direct_window_sum; test infrastructure).

For every left row e:  out_p[e] = sum_j c_ej col_p[j],  cnt[e] = sum_j c_ej,  with
    c_ej = prod_g [pl_g[e] = pr_g[j]] * r_ej
over G partition keys and an order key.  A partition indicator is
(sign(d + eps) - sign(d - eps)) / 2 for d = pl_g[e] - pr_g[j] (lex_model's u - w); r_ej
is running_model's weight for the mode on the order key (ROWS, LE, LT, BETWEEN),
or 1 in GROUP mode, which has no order key.  F = G + (mode != GROUP) factors,
2 <= F <= 4.

`exact` is the definition, `window_sums` the model on the exact composite sign of
tie_model, `oracle_window_sums` the composition on the CPU oracle op by op in
constructRank's layout (running_model.oracle_running_sums' structure): the
definition the GPU is held to, word for word."""
import numpy as np

import group_model as G_
import running_model as R
import stable_model as S
import tie_model as T

ROWS, LE, LT, BETWEEN, GROUP = range(5)
MODES = (ROWS, LE, LT, BETWEEN, GROUP)
MODE_IDS = ('rows', 'le', 'lt', 'between', 'group')
BINARY = S.BINARY
# seeds of partitioned_input per (N, G) for which its conditions hold (searched on the CPU)
SEEDS = {(8, 1): 8, (8, 2): 0, (8, 3): 4, (64, 1): 36, (64, 2): 0, (64, 3): 59, (1024, 1): 0, (1024, 2): 0, (1024, 3): 0}
# seeds of two_tables per N
TABLE_SEEDS = {8: 0, 64: 0}


def nfactors(G, mode):
    return G + (mode != GROUP)


def sign_arguments(pl, pr, mode, eps, ol=None, orr=None, lo=None):
    """(partition arguments [(d_g + eps, d_g - eps)], order arguments as running_model's) of every pair [e][j]"""
    parts = []
    for a, b in zip(pl, pr):
        d = np.asarray(a, dtype=np.float64)[:, None] - np.asarray(b, dtype=np.float64)[None, :]
        parts.append((d + eps, d - eps))
    order = () if mode == GROUP else R.sign_arguments(ol, orr, mode, eps, lo)
    return parts, order


def _weights(parts, order, mode, sign):
    c = None
    for u, w in parts:
        m = (sign(u) - sign(w)) / 2.0
        c = m if c is None else c * m
    if mode == BETWEEN:
        c = c * (sign(order[0]) - sign(order[1])) / 2.0
    elif mode != GROUP:
        c = c * (sign(order[0]) + 1.0) / 2.0
    return c


def _sums(c, cols, n):
    return np.array([c @ np.asarray(v, dtype=np.float64) for v in cols]).reshape(len(cols), n), c.sum(axis=1)


def exact(pl, pr, cols, mode, eps, ol=None, orr=None, lo=None):
    """(sums [P][N], counts [N]) by definition"""
    parts, order = sign_arguments(pl, pr, mode, eps, ol, orr, lo)
    return _sums(_weights(parts, order, mode, lambda a: np.where(a > 0, 1.0, -1.0)), cols, len(pl[0]))


def window_sums(pl, pr, cols, cfg, mode, eps, ol=None, orr=None, lo=None, noise=None):
    """(sums [P][N], counts [N]) on the exact composite sign; noise: added to every sign argument"""
    parts, order = sign_arguments(pl, pr, mode, eps, ol, orr, lo)
    if noise is not None:
        parts = [(u + noise, w + noise) for u, w in parts]
        order = tuple(x + noise for x in order)
    return _sums(_weights(parts, order, mode, lambda a: T.composite_sign(a, *cfg)), cols, len(pl[0]))


def levels(key_level, F, cfg):
    """(diff_level, L_m, L_a, col_max_level, out_level)"""
    Lm = key_level + 1 + G_.sign_depth(cfg)
    La = Lm + (1 if F == 2 else 2)
    return key_level + 1, Lm, La, La - 2, La + 1


def partition_ids(parts):
    """the partition of every row: the index of its key tuple among the distinct tuples"""
    return np.unique(np.stack([np.asarray(p) for p in parts], axis=1), axis=0, return_inverse=True)[1].reshape(-1)


def partitioned_input(N, G, seed=None):
    """(parts [G][N], t, lo, hi, eps, cfg): G partition keys and an order key t on the
    grid 2 / N, t below 1 - 4 / N with the window [t - 2 / N, t + 2 / N] of every row,
    eps = 1 / N and the sort's sign configuration.  Asserts what makes the cases mean
    something: a partition of one row, one of >= 3 rows, an order value tied inside
    a partition, an order value shared by two partitions, a row with an empty LT
    set, and every sign argument within [-1, 1]."""
    seed = SEEDS[(N, G)] if seed is None else seed
    rng = np.random.default_rng([seed, N, G])
    per_key = max(3, N // 8) if G == 1 else max(2, int(np.ceil((N / 8.0) ** (1.0 / G))))
    parts = [rng.integers(0, per_key, N) * 2.0 / N for _ in range(G)]
    t = rng.integers(0, N // 2 - 1, N) * 2.0 / N
    lo, hi, eps = t - 2.0 / N, t + 2.0 / N, 1.0 / N
    pid = partition_ids(parts)
    sizes = np.bincount(pid)
    assert (sizes == 1).any() and (sizes >= 3).any(), (N, G, seed, sizes)
    same_part = pid[:, None] == pid[None, :]
    same_t = t[:, None] == t[None, :]
    off_diag = ~np.eye(N, dtype=bool)
    assert (same_part & same_t & off_diag).any(), (N, G, seed)  # a tie inside a partition
    assert (~same_part & same_t).any(), (N, G, seed)            # the partition factor matters
    assert (exact(parts, parts, [], LT, eps, t, t)[1] == 0).any(), (N, G, seed)
    for mode in (ROWS, LE, LT, BETWEEN):
        pa, oa = sign_arguments(parts, parts, mode, eps, hi if mode == BETWEEN else t, t, lo)
        for a in [x for uw in pa for x in uw] + list(oa):
            assert np.max(np.abs(a)) <= 1.0, (N, G, seed, mode)
    return parts, t, lo, hi, eps, S.sign_cfg(N)


def two_tables(N, seed=None):
    """([kl, kl2], [kr, kr2], eps, cfg): group_model.lookup_tables' two tables with a
    second key of two values 2 eps apart -- JOIN ON a.k1 = b.k1 AND a.k2 = b.k2.  Some
    pair agrees on both keys and some on the first alone."""
    seed = TABLE_SEEDS[N] if seed is None else seed
    kl, kr, eps, cfg = G_.lookup_tables(N, seed)
    rng = np.random.default_rng([seed, N])
    kl2, kr2 = rng.integers(0, 2, N) * 2.0 * eps, rng.integers(0, 2, N) * 2.0 * eps
    first = kl[:, None] == kr[None, :]
    second = kl2[:, None] == kr2[None, :]
    assert (first & second).any() and (first & ~second).any(), (N, seed)
    return [kl, kl2], [kr, kr2], eps, cfg


def oracle_window_sums(orc, opl, opr, ocols, N, rots, cfg, eps, mode, count, ool=None, oor=None, olo=None):
    """the definition of DESIGN.md §6.7 on pyoracle: (outs, count or None)"""
    S_, P, nb, npb = S.rank_shape(N, orc.n // 2)
    Gn = len(opl)
    F = nfactors(Gn, mode)
    assert 2 <= F <= 4 and len(opr) == Gn
    _, Lm, La, _, out_level = levels(opl[0].level, F, cfg)

    def baby_steps(x):
        return [G_._with_slots(orc, orc.compose_rotate(x, N, rots, BINARY, i), S_) for i in range(npb)]

    def shifted(baby, b):
        return G_._vec_rots_opt(orc, baby, N, rots, S_, P, npb, b)

    cbaby = [baby_steps(orc.mul_const_to(c, 2.0 ** -F, La - 1)) for c in ocols]
    pbaby = [baby_steps(k) for k in opr]
    pdup = [G_._with_slots(orc, k, S_) for k in opl]
    if mode != GROUP:
        obaby, odup = baby_steps(oor), G_._with_slots(orc, ool, S_)
        odup_lo = G_._with_slots(orc, olo, S_) if mode == BETWEEN else None
    accs, cnt = [None] * len(ocols), None
    for b in range(nb):
        phi = []
        for g in range(Gn):
            d = orc.sub(pdup[g], shifted(pbaby[g], b))
            u = orc.sign(orc.add_const(d, eps), *cfg)
            w = orc.sign(orc.add_const(d, -eps), *cfg)
            phi.append(orc.sub(u, w))
        if mode != GROUP:  # running_model.oracle_running_sums' indicator
            sk = shifted(obaby, b)
            d = orc.sub(odup, sk)
            if mode == ROWS:
                r = orc.add_const(orc.sign(orc.add_plain(d, orc.encode(S.offsets(N, S_, b, eps), S_, d.level)), *cfg), 1.0)
            elif mode == BETWEEN:
                u = orc.add_const(d, eps)
                w = orc.add_const(orc.sub(odup_lo, sk), -eps)
                r = orc.sub(orc.sign(u, *cfg), orc.sign(w, *cfg))
            else:
                r = orc.add_const(orc.sign(orc.add_const(d, eps if mode == LE else -eps), *cfg), 1.0)
            phi.append(r)
        assert all(x.level == Lm for x in phi)
        if F == 2:
            a = orc.mul(phi[0], phi[1])
        elif F == 3:
            a = orc.mul(phi[0], orc.mul(phi[1], phi[2]))  # operands at two levels: the product adjusts phi[0]
        else:
            a = orc.mul(orc.mul(phi[0], phi[1]), orc.mul(phi[2], phi[3]))
        assert a.level == La
        if count:
            c = orc.mul_const(a, 2.0 ** -F)
            cnt = c if cnt is None else orc.add(cnt, c)
        for p in range(len(ocols)):
            g = orc.mul(a, shifted(cbaby[p], b))
            accs[p] = g if accs[p] is None else orc.add(accs[p], g)

    def fold(acc):
        i = 1
        while (1 << i) <= P:
            acc = orc.add(acc, orc.compose_rotate(acc, N, rots, BINARY, S_ >> i))
            i += 1
        return acc

    outs = []
    for acc in accs:
        acc = fold(acc)
        acc.set_slots(N)
        assert acc.level == out_level
        outs.append(acc)
    if count:
        cnt = fold(cnt)
        cnt.set_slots(N)
        assert cnt.level == out_level
    return outs, cnt
