"""Plaintext model and CPU-oracle composition of the tie-broken rank (test
infrastructure).

constructRank compares element e with element j through sign(x_e - x_j).  With
fhe_set_sort_tiebreak(eps) a public offset is added to the difference first:
+eps where j <= e (the self comparison included), -eps where j > e.  Tied pairs
then sit at +-eps, distinct values >= 2 eps apart keep |d| >= eps, every compare
is a clean 0 or 1, the self comparison yields 1 (closing constant -1), and the
rank is the stable argsort rank  #{x_j < x_e} + #{j < e : x_j = x_e}.

Slot layout (vecRotsOpt, src/sort_algo.h:326-366): with S = N P_ slots, slot s of
comparator batch b holds x[s mod N] - x[(s mod N + t) mod N], t = b P_ + s // N,
so the compared element precedes (or is) element s mod N iff t == 0 or
(s mod N) + t >= N.

`ranks` is the model on the exact composite sign of tie_model; `oracle_rank`
builds the rank on the CPU oracle op by op the way the oracle's constructRank
does, with the one added add_plain(E_b) and the -1 constant.  With eps = 0 it
is the oracle's constructRank word for word."""
import numpy as np

import tie_model as T

BINARY = 2  # DecomposeAlgo of DirectSort's RotationComposer


def sign_cfg(N):  # tests/DirectSortTest.cpp:104-112
    return (3, 2, 2) if N <= 16 else (3, 3, 2) if N <= 128 else (3, 4, 2) if N <= 512 else (3, 5, 2)


def rank_np(N, P):  # src/sort_algo.h:383-416
    for lim, v in ((8, 2), (32, 4), (128, 8), (512, 16), (2048, 32)):
        if N <= lim:
            return min(v, P) if N >= 4 else 1
    return 1


def rank_shape(N, max_batch):
    """(num_slots, num_partition, num_batch, np) of constructRank on a ring with max_batch = n / 2 slots"""
    P = min(N, max_batch // N)
    return N * P, P, N // P, rank_np(N, P)


def offsets(N, S, batch, eps):
    s = np.arange(S)
    t = batch * (S // N) + s // N
    return np.where((t == 0) | (s % N + t >= N), eps, -eps).astype(np.float64)


def stable_ranks(x):
    return np.argsort(np.argsort(np.asarray(x), kind='stable'), kind='stable').astype(np.float64)


def tied_input(N, seed):
    """N values on the grid 2 / N holding at least one odd and one even multiplicity >= 2"""
    x = np.random.default_rng(seed).integers(0, N // 2, N) * 2.0 / N
    m = np.unique(x, return_counts=True)[1]
    assert any(c >= 3 and c % 2 for c in m) and any(c >= 2 and c % 2 == 0 for c in m), (N, seed, m)
    return x


# seeds whose draw holds both kinds of multiplicity (checked by tied_input)
SEEDS = {8: 3, 16: 1, 32: 1, 64: 1, 128: 1, 1024: 1}


def ranks(x, cfg, eps, noise=None):
    """the rank in plaintext: eps = 0 is tie_model.ranks"""
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    e, j = np.arange(N)[:, None], np.arange(N)[None, :]
    d = x[:, None] - x[None, :]
    if eps > 0:
        d = d + np.where(j <= e, eps, -eps)
    if noise is not None:
        d = d + noise
    c = (T.composite_sign(d, *cfg) + 1.0) / 2.0
    return c.sum(axis=1) - (1.0 if eps > 0 else 0.5)


def _with_slots(orc, ct, slots):
    inf = ct.info()
    return orc.ct_from(ct.data(), inf['level'], slots, inf['scale'])


def oracle_rank(orc, ox, N, rots, cfg, eps):
    S, P, nb, npb = rank_shape(N, orc.n // 2)
    baby = [_with_slots(orc, orc.compose_rotate(ox, N, rots, BINARY, i), S) for i in range(npb)]
    dup = _with_slots(orc, ox, S)
    rank = None
    for b in range(nb):
        shifted = None
        for j in range(P // npb):
            pts = []
            for i in range(npb):
                m = np.zeros(S)
                m[(npb * j + i) * N:(npb * j + i + 1) * N] = 1.0
                pts.append(orc.encode(np.roll(m, b * P + j * npb), S, baby[i].level))  # vector_rotate by -(b P + j np)
            o = orc.compose_rotate(orc.mul_plain_sum(baby, pts), N, rots, BINARY, b * P + j * npb)
            shifted = o if shifted is None else orc.add(shifted, o)
        d = orc.sub(dup, shifted)
        if eps > 0:
            d = orc.add_plain(d, orc.encode(offsets(N, S, b, eps), S, d.level))
        c = orc.mul_const(orc.add_const(orc.sign(d, *cfg), 1.0), 0.5)
        rank = c if rank is None else orc.add(rank, c)
    i = 1
    while (1 << i) <= P:
        rank = orc.add(rank, orc.compose_rotate(rank, N, rots, BINARY, S >> i))
        i += 1
    rank.set_slots(N)
    return orc.add_const(rank, -1.0 if eps > 0 else -0.5)
