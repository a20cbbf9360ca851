"""Plaintext model of the order-statistic select (fhe_direct_select), shared by
tests/test_select.py and tests/test_gpu_select.py.  The layout comes from
fhe_select_layout; everything else is the definition restated in numpy."""
import numpy as np

import fhesort as F


def cap_of(N, S):
    return S // N - 1 if S // N >= 2 else 1


def vectors(N, S, targets, z):
    """(C_z, K_z): C_z holds targets[p] on the window of every target p of member
    z, K_z holds 1 at the first slot of each of those windows, both 0 elsewhere"""
    _, member, start = F.select_layout(N, S, len(targets))
    Cz, Kz = np.zeros(S), np.zeros(S)
    for p, t in enumerate(targets):
        if member[p] != z:
            continue
        w = (start[p] + np.arange(N)) % S
        Cz[w] = t
        Kz[start[p]] = 1.0
    return Cz, Kz


def select(x, targets, N, S):
    """the definition with an exact delta: N output slots"""
    x = np.asarray(x, dtype=np.float64)
    rank = np.argsort(np.argsort(x, kind='stable'), kind='stable')
    rank_s, x_s = np.tile(rank, S // N).astype(np.float64), np.tile(x, S // N)
    members, _, _ = F.select_layout(N, S, len(targets))
    out = np.zeros(S)
    for z in range(members):
        Cz, Kz = vectors(N, S, targets, z)
        v = (Cz - rank_s == 0).astype(np.float64) * x_s
        for i in range(int(np.log2(N))):
            v = v + np.roll(v, -(1 << i))
        out += v * Kz
    i = 1
    while (1 << i) <= S // N:
        out = out + np.roll(out, -(S >> i))
        i += 1
    return out[:N]
