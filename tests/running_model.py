"""Plaintext model and CPU-oracle composition of the running sums
(fhe_direct_running_sum; test infrastructure).

For every left row e:  out_p[e] = sum_j c_ej col_p[j],  cnt[e] = sum_j c_ej,  with
the weight of a pair by mode (d = kl_e - kr_j):

    ROWS     (sign(d + E_ej) + 1) / 2, E = +eps where j <= e, -eps where j > e
             (stable_model.offsets): the stable row order, own row included;
    LE       (sign(d + eps) + 1) / 2: kr_j <= kl_e, peers included;
    LT       (sign(d - eps) + 1) / 2: kr_j < kl_e;
    BETWEEN  (sign(hi_e - kr_j + eps) - sign(lo_e - kr_j - eps)) / 2, kl = hi:
             lo_e <= kr_j <= hi_e, both ends closed.

Equal keys sit at +-eps, distinct ones (bounds included) >= 2 eps apart leave
every sign argument at magnitude >= eps, so each weight is a clean 1 or 0
wherever the sign resolves eps.

`exact` is the definition, `running_sums` the model on the exact composite sign
of tie_model, `oracle_running_sums` the composition on the CPU oracle op by op
in constructRank's layout (group_model.oracle_group_sums' structure)."""
import numpy as np

import group_model as G
import stable_model as S
import tie_model as T

ROWS, LE, LT, BETWEEN = range(4)
MODES = (ROWS, LE, LT, BETWEEN)
MODE_IDS = ('rows', 'le', 'lt', 'between')
BINARY = S.BINARY
WINDOW_SEED = 5


def sign_arguments(kl, kr, mode, eps, lo=None):
    """the arguments of the signs of every pair [e][j]: one matrix, two (u, w) for BETWEEN"""
    kl, kr = np.asarray(kl, dtype=np.float64), np.asarray(kr, dtype=np.float64)
    d = kl[:, None] - kr[None, :]
    if mode == ROWS:
        e, j = np.arange(len(kl))[:, None], np.arange(len(kr))[None, :]
        return (d + np.where(j <= e, eps, -eps),)
    if mode == LE:
        return (d + eps,)
    if mode == LT:
        return (d - eps,)
    assert mode == BETWEEN and lo is not None
    return (d + eps, np.asarray(lo, dtype=np.float64)[:, None] - kr[None, :] - eps)


def _sums(c, cols, n):
    return np.array([c @ np.asarray(v, dtype=np.float64) for v in cols]).reshape(len(cols), n), c.sum(axis=1)


def exact(kl, kr, cols, mode, eps, lo=None):
    """(sums [P][N], counts [N]) by definition"""
    a = sign_arguments(kl, kr, mode, eps, lo)
    c = (a[0] > 0).astype(np.float64)
    if mode == BETWEEN:
        c = c - (a[1] > 0)
    return _sums(c, cols, len(kl))


def running_sums(kl, kr, cols, cfg, mode, eps, lo=None, noise=None):
    """(sums [P][N], counts [N]) on the exact composite sign; noise: added to every sign argument"""
    a = sign_arguments(kl, kr, mode, eps, lo)
    if noise is not None:
        a = tuple(x + noise for x in a)
    if mode == BETWEEN:
        c = (T.composite_sign(a[0], *cfg) - T.composite_sign(a[1], *cfg)) / 2.0
    else:
        c = (T.composite_sign(a[0], *cfg) + 1.0) / 2.0
    return _sums(c, cols, len(kl))


def window_input(N, seed=WINDOW_SEED):
    """(k, lo, hi, eps, cfg): keys on the grid 2 / N below 1 - 4 / N and the window
    [k - 2 / N, k + 2 / N] of every row -- RANGE BETWEEN 2 / N PRECEDING AND 2 / N
    FOLLOWING.  Keys and bounds are grid points, so distinct ones are >= 2 eps
    apart for eps = 1 / N, and every sign argument stays within [-1, 1]."""
    k = np.random.default_rng(seed).integers(0, N // 2 - 1, N) * 2.0 / N
    lo, hi, eps = k - 2.0 / N, k + 2.0 / N, 1.0 / N
    u, w = sign_arguments(hi, k, BETWEEN, eps, lo)
    assert max(np.max(np.abs(u)), np.max(np.abs(w))) <= 1.0, (N, seed)
    cnt = exact(hi, k, [], BETWEEN, eps, lo)[1]
    assert cnt.min() < N, (N, seed)   # some window leaves a row out
    assert cnt.max() >= 3, (N, seed)  # some window holds >= 3 rows
    return k, lo, hi, eps, S.sign_cfg(N)


def oracle_running_sums(orc, okl, okr, ocols, N, rots, cfg, eps, mode, count, olo=None):
    """the definition of DESIGN.md §6.6 on pyoracle: (outs, count or None)"""
    S_, P, nb, npb = S.rank_shape(N, orc.n // 2)
    Lm = okl.level + 1 + G.sign_depth(cfg)

    def baby_steps(x):
        return [G._with_slots(orc, orc.compose_rotate(x, N, rots, BINARY, i), S_) for i in range(npb)]

    kbaby = baby_steps(okr)
    cbaby = [baby_steps(orc.mul_const_to(c, 0.5, Lm - 1)) for c in ocols]
    dup = G._with_slots(orc, okl, S_)
    dup_lo = G._with_slots(orc, olo, S_) if mode == BETWEEN else None
    accs, cnt = [None] * len(ocols), None
    for b in range(nb):
        sk = G._vec_rots_opt(orc, kbaby, N, rots, S_, P, npb, b)
        d = orc.sub(dup, sk)
        if mode == ROWS:
            a = orc.add_const(orc.sign(orc.add_plain(d, orc.encode(S.offsets(N, S_, b, eps), S_, d.level)), *cfg), 1.0)
        elif mode == BETWEEN:
            u = orc.add_const(d, eps)
            w = orc.add_const(orc.sub(dup_lo, sk), -eps)
            a = orc.sub(orc.sign(u, *cfg), orc.sign(w, *cfg))
        else:
            a = orc.add_const(orc.sign(orc.add_const(d, eps if mode == LE else -eps), *cfg), 1.0)
        assert a.level == Lm
        if count:
            c = orc.mul_const(a, 0.5)
            cnt = c if cnt is None else orc.add(cnt, c)
        for p in range(len(ocols)):
            g = orc.mul(a, G._vec_rots_opt(orc, cbaby[p], N, rots, S_, P, npb, b))
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
        outs.append(acc)
    if count:
        cnt = fold(cnt)
        cnt.set_slots(N)
    return outs, cnt
