"""Plaintext model and CPU-oracle composition of the lexicographic rank
(fhe_direct_lex_rank; test infrastructure).

Keys K_0 .. K_{L-1}, most significant first.  For a pair (e, j) and
d_l = K_l[e] - K_l[j]:
    leading keys   u_l = sign(d_l + eps),  w_l = sign(d_l - eps)
                   (w_l + 1) / 2 = "K_l[j] smaller by a margin", (u_l - w_l) / 2 = "equal"
    last key       s = sign(d_{L-1} + E), E the tie-break offset (+tb where j <= e,
                   -tb where j > e) or nothing
    Horner         T_{L-1} = s + 1,  T_l = (u_l - w_l) T_{l+1} + 2^(L-1-l) (w_l + 1)
    rank_e = 2^-L sum_j T_0(e, j) - c,   c = 1 with the tie-break, 1/2 without.
With the tie-break it is the stable lexicographic argsort rank (np.lexsort's).

`ranks` is the model on the exact composite sign of tie_model; `oracle_lex_rank`
builds the rank on the CPU oracle op by op in constructRank's layout
(stable_model.oracle_rank, group_model._vec_rots_opt): the definition the GPU is
held to, word for word."""
import numpy as np

import group_model as G
import stable_model as S
import tie_model as T

BINARY = S.BINARY

# leading keys are drawn from this many values of the grid 2 / N
LEADING_VALUES = {8: 4, 64: 8, 1024: 32}
# seeds of the leading keys' draw per (N, L) used by the tests; for L = 2, 3 every
# draw holds rows tied on every key
KEY_SEED = {(8, 2): 1, (8, 3): 1, (8, 4): 1, (64, 2): 1, (64, 3): 2, (64, 4): 1}


def exact_ranks(keys):
    """stable lexicographic argsort ranks (np.lexsort sorts by its last key first)"""
    order = np.lexsort([np.asarray(k) for k in keys][::-1])
    r = np.empty(len(order), dtype=np.float64)
    r[order] = np.arange(len(order))
    return r


def tied_keys(N, L, seed):
    """L keys of N rows: the leading ones on the grid 2 / N drawn from LEADING_VALUES[N]
    values (so every leading value repeats), the last one stable_model.tied_input"""
    rng = np.random.default_rng([seed, N, L])  # never the stream of tied_input's own draw
    lead = [rng.integers(0, LEADING_VALUES[N], N) * 2.0 / N for _ in range(L - 1)]
    return lead + [S.tied_input(N, S.SEEDS[N])]


def distinct_keys(N, L, seed):
    """pairwise-distinct tuples: tied leading keys, the last key a permutation of the grid 1 / N"""
    rng = np.random.default_rng([seed, N, L])
    lead = [rng.integers(0, LEADING_VALUES[N], N) * 2.0 / N for _ in range(L - 1)]
    return lead + [rng.permutation(N) / float(N)]


def ranks(keys, cfg, eps, tb, noise=None):
    """the rank in plaintext on the exact composite sign; tb = 0: no tie-break (c = 1/2)"""
    keys = [np.asarray(k, dtype=np.float64) for k in keys]
    L, N = len(keys), len(keys[0])
    e, j = np.arange(N)[:, None], np.arange(N)[None, :]
    d = keys[L - 1][:, None] - keys[L - 1][None, :]
    if tb > 0:
        d = d + np.where(j <= e, tb, -tb)
    if noise is not None:
        d = d + noise
    t = T.composite_sign(d, *cfg) + 1.0
    for l in range(L - 2, -1, -1):
        d = keys[l][:, None] - keys[l][None, :]
        u, w = T.composite_sign(d + eps, *cfg), T.composite_sign(d - eps, *cfg)
        t = (u - w) * t + 2.0 ** (L - 1 - l) * (w + 1.0)
    return t.sum(axis=1) / 2.0 ** L - (1.0 if tb > 0 else 0.5)


def levels(key_level, L, cfg):
    """(diff_level, sign_level L_m, rank_level)"""
    Lm = key_level + 1 + G.sign_depth(cfg)
    return key_level + 1, Lm, Lm + L


def oracle_lex_rank(orc, keys, N, rots, cfg, eps, tb):
    """the definition of DESIGN.md §6.5 on pyoracle; tb = 0: no tie-break"""
    S_, P, nb, npb = S.rank_shape(N, orc.n // 2)
    L = len(keys)
    _, Lm, rank_level = levels(keys[0].level, L, cfg)
    baby = [[G._with_slots(orc, orc.compose_rotate(k, N, rots, BINARY, i), S_) for i in range(npb)] for k in keys]
    dup = [G._with_slots(orc, k, S_) for k in keys]
    rank = None
    for b in range(nb):
        d = [orc.sub(dup[l], G._vec_rots_opt(orc, baby[l], N, rots, S_, P, npb, b)) for l in range(L)]
        last = d[L - 1]
        if tb > 0:
            last = orc.add_plain(last, orc.encode(S.offsets(N, S_, b, tb), S_, last.level))
        t = orc.add_const(orc.sign(last, *cfg), 1.0)
        assert t.level == Lm
        for l in range(L - 2, -1, -1):
            u = orc.sign(orc.add_const(d[l], eps), *cfg)
            w = orc.sign(orc.add_const(d[l], -eps), *cfg)
            prod = orc.mul(orc.sub(u, w), t)  # operands at different levels for l < L - 2: the product adjusts them
            t = orc.add(prod, orc.mul_const_to(orc.add_const(w, 1.0), 2.0 ** (L - 1 - l), prod.level))
            assert t.level == Lm + (L - 1 - l)
        rank = t if rank is None else orc.add(rank, t)
    i = 1
    while (1 << i) <= P:
        rank = orc.add(rank, orc.compose_rotate(rank, N, rots, BINARY, S_ >> i))
        i += 1
    rank = orc.add_const(orc.mul_const(rank, 2.0 ** -L), -1.0 if tb > 0 else -0.5)
    rank.set_slots(N)
    assert rank.level == rank_level
    return rank
