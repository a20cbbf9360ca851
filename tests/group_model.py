"""Plaintext model and CPU-oracle composition of the group sums and lookups
(fhe_direct_group_sum; test infrastructure).

For every left row e:  out_p[e] = sum_j [ |kl_e - kr_j| < eps ] col_p[j].  The
match indicator of a pair is (sign(d + eps) + sign(-d + eps)) / 2 for the
difference d = kl_e - kr_j: with equal keys both signs sit at +eps, with keys
>= 2 eps apart one sits at <= -eps and the other at >= 3 eps, so the sum is a
clean 2 or 0 wherever the sign resolves eps.

`group_sums` is the model on the exact composite sign of tie_model;
`oracle_group_sums` builds the result on the CPU oracle op by op in
constructRank's layout (stable_model.oracle_rank): slot s of comparator batch b
holds kl[s mod N] - kr[(s mod N + t) mod N], t = b P_ + s // N, and the same
vecRotsOpt shift of a column puts col[(s mod N + t) mod N] beside it."""
import numpy as np

import stable_model as S
import tie_model as T

BINARY = S.BINARY


def sign_depth(cfg):
    """levels the composite sign consumes for n = 3 (g_3 and f_3 take 3 each; g runs once even when dg = 0)"""
    n, dg, df = cfg
    assert n == 3
    return 3 * (max(dg, 1) + df)


def exact(kl, kr, cols, eps):
    """(sums [P][N], counts [N]) by definition"""
    kl, kr = np.asarray(kl, dtype=np.float64), np.asarray(kr, dtype=np.float64)
    m = (np.abs(kl[:, None] - kr[None, :]) < eps).astype(np.float64)
    return np.array([m @ np.asarray(c, dtype=np.float64) for c in cols]).reshape(len(cols), len(kl)), m.sum(axis=1)


def group_sums(kl, kr, cols, cfg, eps, noise=None):
    """(sums [P][N], counts [N]) on the exact composite sign; noise: added to the differences"""
    kl, kr = np.asarray(kl, dtype=np.float64), np.asarray(kr, dtype=np.float64)
    d = kl[:, None] - kr[None, :]
    if noise is not None:
        d = d + noise
    m = (T.composite_sign(d + eps, *cfg) + T.composite_sign(-d + eps, *cfg)) / 2.0
    return np.array([m @ np.asarray(c, dtype=np.float64) for c in cols]).reshape(len(cols), len(kl)), m.sum(axis=1)


def lookup_tables(N, seed):
    """Two tables for the join lookup, (kl, kr, eps, cfg): keys on the grid 1 / 2N
    in [0, 1), the right keys N distinct grid points, the left keys drawn from the
    whole grid, so about half of them have no right row and some repeat.  Distinct
    keys are >= 1 / 2N = 2 eps apart, |kl - kr| + eps <= 1, and the sign
    configuration is the reference's for a sort of 4N values, whose smallest
    difference is that eps."""
    rng = np.random.default_rng(seed)
    grid = np.arange(2 * N) / (2.0 * N)
    kr = rng.permutation(grid)[:N]
    kl = rng.choice(grid, N)
    present = np.isin(kl, kr)
    assert present.any() and (~present).any(), (N, seed)
    return kl, kr, 1.0 / (4 * N), S.sign_cfg(4 * N)


def _with_slots(orc, ct, slots):
    inf = ct.info()
    return orc.ct_from(ct.data(), inf['level'], slots, inf['scale'])


def _vec_rots_opt(orc, baby, N, rots, S_, P, npb, b):
    """the vecRotsOpt result of batch b from the baby steps (oracle_rank's loop)"""
    shifted = None
    for j in range(P // npb):
        pts = []
        for i in range(npb):
            m = np.zeros(S_)
            m[(npb * j + i) * N:(npb * j + i + 1) * N] = 1.0
            pts.append(orc.encode(np.roll(m, b * P + j * npb), S_, baby[i].level))
        o = orc.compose_rotate(orc.mul_plain_sum(baby, pts), N, rots, BINARY, b * P + j * npb)
        shifted = o if shifted is None else orc.add(shifted, o)
    return shifted


def oracle_group_sums(orc, okl, okr, ocols, N, rots, cfg, eps, count):
    """the definition of DESIGN.md §6.4 on pyoracle: (outs, count or None)"""
    S_, P, nb, npb = S.rank_shape(N, orc.n // 2)
    Lm = okl.level + 1 + sign_depth(cfg)

    def baby_steps(x):
        return [_with_slots(orc, orc.compose_rotate(x, N, rots, BINARY, i), S_) for i in range(npb)]

    kbaby = baby_steps(okr)
    cbaby = [baby_steps(orc.mul_const_to(c, 0.5, Lm - 1)) for c in ocols]
    dup = _with_slots(orc, okl, S_)
    accs, cnt = [None] * len(ocols), None
    for b in range(nb):
        d = orc.sub(dup, _vec_rots_opt(orc, kbaby, N, rots, S_, P, npb, b))
        u = orc.add_const(d, eps)
        w = orc.add_const(orc.negate(d), eps)
        m = orc.add(orc.sign(u, *cfg), orc.sign(w, *cfg))
        assert m.level == Lm
        if count:
            cnt = m if cnt is None else orc.add(cnt, m)
        for p in range(len(ocols)):
            g = orc.mul(m, _vec_rots_opt(orc, cbaby[p], N, rots, S_, P, npb, b))
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
        cnt = orc.mul_const(fold(cnt), 0.5)
        cnt.set_slots(N)
    return outs, cnt
