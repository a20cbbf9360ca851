"""Plaintext model and CPU-oracle composition of the gather by encrypted position
(fhe_direct_gather; test infrastructure).

For every left row e, column p and public offset o:
    out_{p,o}[e] = sum_j delta(pos_l[e] + o - pos_r[j]) col_p[j],
the value of the right row standing o places after left row e's position, zero
where there is none; present_o[e] is the same sum without the column.  delta is the
sort's doubled-sinc series f(t) = sinc(2N t) + sinc(2N (t + 1/2)) at t = d / 2N
(tie_model), which is 1 at d = 0 and also at d = -N.  The difference is therefore
oriented: d = pos_l[e] - pos_r[j] + o for o >= 0 and its negation for o < 0, so that
d > -N always (and |d| <= 2N - 2 stays inside the series' domain); the other
orientation reaches -N and wraps around the end of the order.

`exact` is the definition, `gather` the model on the committed coefficient tables
evaluated with OpenFHE's halved c_0, `sort_index_check` the sort's own index check
on the same tables (the yardstick of the model's error), `oracle_gather` the
composition on the CPU oracle op by op in constructRank's layout
(group_model.oracle_group_sums' structure): the definition the GPU is held to,
word for word."""
import numpy as np
from numpy.polynomial import chebyshev as _cheb

import group_model as G_
import pyoracle as O
import stable_model as S

BINARY = S.BINARY


def series(N, d):
    """the doubled-sinc table of N at d / 2N (OpenFHE's convention: c_0 is halved)"""
    c = O.doubled_sinc(N)
    return _cheb.chebval(np.asarray(d, dtype=np.float64) / (2.0 * N), np.concatenate([[c[0] / 2], c[1:]]))


def differences(pos_l, pos_r, o, flip=False):
    """the oriented differences [e][j] of offset o; flip: the other (wrapping) orientation"""
    d = np.asarray(pos_l, dtype=np.float64)[:, None] - np.asarray(pos_r, dtype=np.float64)[None, :] + o
    return -d if (o < 0) != flip else d


def exact(pos_l, pos_r, cols, offsets):
    """(outs [P][K][len(pos_l)], present [K][len(pos_l)]) by definition, on integer positions"""
    pl, pr = np.rint(pos_l).astype(np.int64), np.rint(pos_r).astype(np.int64)
    m = np.array([(pl[:, None] + o == pr[None, :]).astype(np.float64) for o in offsets])
    outs = np.array([[mk @ np.asarray(c, dtype=np.float64) for mk in m] for c in cols])
    return outs.reshape(len(cols), len(offsets), len(pl)), m.sum(axis=2)


def gather(pos_l, pos_r, cols, offsets, N, flip=False):
    """(outs [P][K][len(pos_l)], present [K][len(pos_l)]) on the series of the oriented differences; pos_l may
    hold a subset of the left rows (the series of degree ~6500 at N = 1024 is the cost of every pair)"""
    w = np.array([series(N, differences(pos_l, pos_r, o, flip)) for o in offsets])
    outs = np.array([[wk @ np.asarray(c, dtype=np.float64) for wk in w] for c in cols])
    return outs.reshape(len(cols), len(offsets), len(pos_l)), w.sum(axis=2)


def sort_index_check(rank, x, N, slots=None):
    """rotationIndexCheckN on the same tables: slot k = sum_i x_i f((i - rank_i - s) / 2N), s = (i - k) mod N;
    slots: the output slots wanted (all N by default)"""
    i, k = np.arange(N)[:, None], (np.arange(N) if slots is None else np.asarray(slots))[None, :]
    d = i - np.asarray(rank, dtype=np.float64)[:, None] - (i - k) % N
    return np.asarray(x, dtype=np.float64) @ series(N, d)


def levels(pos_level, N):
    """(diff_level, series_level, col_max_level, out_level)"""
    Ls = pos_level + 2 + O.cheb_ps_depth(len(np.trim_zeros(O.doubled_sinc(N), 'b')) - 1)
    return pos_level + 1, Ls, Ls - 2, Ls + 1


def oracle_gather(orc, opl, opr, ocols, offsets, N, rots, present=False, sum_offsets=False):
    """the definition of DESIGN.md §6.8 on pyoracle: (outs, present flags); outs column-major
    (p K + k, or p alone under sum_offsets), the flags per offset (one under sum_offsets)"""
    S_, P, nb, npb = S.rank_shape(N, orc.n // 2)
    _, Ls, _, out_level = levels(opl.level, N)
    coeffs = O.doubled_sinc(N)
    K = len(offsets)
    Ko = 1 if sum_offsets else K

    def baby_steps(x):
        return [G_._with_slots(orc, orc.compose_rotate(x, N, rots, BINARY, i), S_) for i in range(npb)]

    rbaby = baby_steps(opr)
    cbaby = [baby_steps(orc.mul_const_to(c, 1.0, Ls - 1)) for c in ocols]
    dup = G_._with_slots(orc, opl, S_)
    accs, cnt = [None] * (len(ocols) * Ko), [None] * Ko
    for b in range(nb):
        base = orc.sub(dup, G_._vec_rots_opt(orc, rbaby, N, rots, S_, P, npb, b))
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
                cnt[k] = rs[k] if cnt[k] is None else orc.add(cnt[k], rs[k])
        for p in range(len(ocols)):
            sc = G_._vec_rots_opt(orc, cbaby[p], N, rots, S_, P, npb, b)
            for k in range(Ko):
                g = orc.mul(rs[k], sc)
                accs[p * Ko + k] = g if accs[p * Ko + k] is None else orc.add(accs[p * Ko + k], g)

    def fold(acc):
        i = 1
        while (1 << i) <= P:
            acc = orc.add(acc, orc.compose_rotate(acc, N, rots, BINARY, S_ >> i))
            i += 1
        acc.set_slots(N)
        return acc

    outs = [fold(a) for a in accs]
    assert all(a.level == out_level for a in outs)
    return outs, ([fold(c) for c in cnt] if present else [])
