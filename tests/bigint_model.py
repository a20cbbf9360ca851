"""Exact big-integer model of the RNS-CKKS arithmetic of DESIGN.md §2.

A reference that shares no code with the oracle or the engine: every value is
a Python int or a numpy array of dtype=object holding Python ints, every
reduction is a plain `%`, and every basis conversion goes through the CRT
integer itself.  The only thing taken from the implementation under test is
each prime's root psi, read as ntt(i, X)[0] (X = the polynomial with
coefficient 1 at degree 1) and checked to be a primitive 2n-th root
(psi^n = -1 mod q); from there the transform is defined, not copied:

    forward   A[k] = a(psi^(2 brev(k) + 1)),  k = 0 .. n-1
    inverse   its inverse

evaluated by staged butterflies over object arrays (checked against the naive
evaluation at ring 2^6 by tests/test_bigint_model.py).

Definitions (q_0 .. q_{ell-1} the level's primes, p_0 .. p_{K-1} the special
primes, P their product, digit j = primes j alpha .. min(ell, (j+1) alpha) - 1
with product Q_j and Qhat_i = Q_j / q_i):

  ModUp of digit j   y_i = [x_i Qhat_i^-1]_{q_i},  S = sum_i y_i Qhat_i as an
                     integer (not reduced mod Q_j: S = X_j + u Q_j, 0 <= u <
                     alpha); out_t = S mod p_t for every target outside the
                     digit; the digit's own limbs are copied.
  ModDown            X_P = CRT of the P residues in [0, P); c = X_P if
                     2 X_P < P else X_P - P; out_i = (x_i - c) P^-1 mod q_i.
  Rescale            r = the last residue in coefficient form; c = r if
                     2 r < q_last else r - q_last;
                     out_i = (x_i - c) q_last^-1 mod q_i.
  ModRaise           r = the only residue in coefficient form, centred as in
                     the rescale; out_i = c mod q_i for every Q prime.
  Automorphism       a(X) -> a(X^g) on coefficients with X^n = -1.
  Key switch         ModUp, (automorphism,) sum_j ext_j key_j per target
                     prime, ModDown of both halves.
  mul                tensor (d0, d1, d2), relinearise d2, add, one rescale.
  rotate             (sigma_g c0 + ks0, ks1), ks = key switch of sigma_g c1.

Ties.  The implementations do not form X_P; they pick ModDown's multiple of
P as v = round(t), t = sum_k y_k / p_k accumulated in fp64 in ascending k
(y_k = [x_k Phat_k^-1]_{p_k}), computed as (u64)(t + 0.5).  Exactly,
t = X_P / P + u' with u' an integer, so v = u' + [X_P / P >= 1/2] unless the
fp64 error of t + 0.5 reaches |X_P / P - 1/2|.  Bound of that error with
u = 2^-53 (unit roundoff, round to nearest):
  * a term fl(fl(y_k) * fl(1 / fl(p_k))) carries four roundings (y_k < 2^60
    converted, p_k converted, the reciprocal, the product) on a value below
    1: at most 4u each, 4K u in all;
  * the K - 1 additions (the first, 0 + term, is exact) round a partial sum
    below i at the i-th term: at most u (2 + 3 + .. + K) = u (K(K+1)/2 - 1);
  * t + 0.5 < K + 1/2 rounds once more: at most u (K + 1/2);
so |error| <= eps = (K^2/2 + 5.5 K - 1/2) u, second-order terms (below
K^2 u^2) aside.  A coefficient is called a tie when the choice could go
either way, |X_P / P - 1/2| <= eps, i.e. with the distance written as
|2 X_P - P| / P:

    tie  <=>  |2 X_P - P| / P <= tau,   tau = 2 eps + u = (K^2 + 11 K) 2^-53

(the + u covers the second-order terms).  At a tie, and only there, the other
candidate c -+ P is correct as well; moddown() returns the tie indices and the
other candidate's coefficients.  The compare is done in integers:
|2 X_P - P| 2^53 <= (K^2 + 11 K) P.

Constants and their sums (second half of the file).  A real constant is
the pair (k, sh) standing for k 2^sh (scaled_const and its two callers);
linear_sums / mul_plain_sum_words are the sums of products over the
integers, reduced once; add_const, mul_const, mul_const_to, mul_int,
level_adjust, linear_sum_to, mul_plain_sum (batches, groups) and
mul_add_const are Model methods defined from those and from rescale / the
key switch above.  The last section restates how the matrix-core kernels
split such a sum into int32 rows of signed bytes times balanced digits
(rows_window, rows_fold), only to choose inputs (target_words) and to bound
the rows (budget_bound_window, budget_bound_fold); split30_middle does the
same for the VALU form's 30-bit halves.
"""
import math

import numpy as np


def obj(a):
    """integer array -> array of Python ints"""
    return np.asarray(a).astype(object)


def u64(a):
    """array of Python ints in [0, 2^64) -> uint64"""
    return np.asarray(a, dtype=object).astype(np.uint64)


def bitrev(logn):
    k = np.arange(1 << logn, dtype=np.int64)
    r = np.zeros_like(k)
    for b in range(logn):
        r |= ((k >> b) & 1) << (logn - 1 - b)
    return r


def tau_num(K):
    """tau = tau_num(K) / 2^53 (module docstring)"""
    return K * K + 11 * K


def galois_of_rotation(logn, k):
    """5^k mod 2n, k taken mod n/2"""
    return pow(5, k % (1 << (logn - 1)), 1 << (logn + 1))


def automorph_coeff(a, g, q=None):
    """a(X) -> a(X^g) mod X^n + 1 on a coefficient vector (object array or
    ints); reduced into [0, q) when q is given, signed otherwise"""
    a = obj(a)
    n = len(a)
    e = (np.arange(n, dtype=np.int64) * (g % (2 * n))) % (2 * n)
    out = np.empty(n, dtype=object)
    out[e % n] = np.where(e >= n, -a, a)
    return out % q if q is not None else out


def centre(x, m):
    """the centred representative as the spec's lifts cut it: x mod m if
    2 (x mod m) < m, else x mod m - m"""
    x = x % m
    return np.where(2 * x < m, x, x - m)


def crt(res, mods):
    """object arrays of residues -> the integer in [0, prod mods)"""
    M = 1
    for m in mods:
        M *= m
    X = 0
    for r, m in zip(res, mods):
        Mh = M // m
        X = X + r * (Mh * pow(Mh, -1, m))
    return X % M, M


class Model:
    """ntt(i, x) is the transform under test (prime index, uint64 vector ->
    uint64 vector); only psi is read through it."""

    def __init__(self, logN, primes, nq, K, alpha, ntt):
        self.logN, self.n = logN, 1 << logN
        self.q = [int(p) for p in primes]
        self.nq, self.K, self.alpha = nq, K, alpha
        assert len(self.q) == nq + K
        self.brev = bitrev(logN)
        X = np.zeros(self.n, dtype=np.uint64)
        X[1] = 1
        self.psi = []
        for i, q in enumerate(self.q):
            psi = int(ntt(i, X)[0])
            assert pow(psi, self.n, q) == q - 1, f'prime {i}: psi is no primitive 2n-th root'
            self.psi.append(psi)
        self._tab = {}
        self.P = 1
        for p in self.q[nq:]:
            self.P *= p

    # ------------------------------------------------------------- NTT ----
    def _tables(self, i):
        if i not in self._tab:
            q, psi, n = self.q[i], self.psi[i], self.n
            pw = [1] * (n + 1)
            for k in range(1, n + 1):
                pw[k] = pw[k - 1] * psi % q
            pw = np.array(pw, dtype=object)
            fwd = pw[self.brev]                       # psi^brev(k)
            inv = (-pw[self.n - self.brev]) % q       # psi^-r = -psi^(n - r)
            inv[0] = 1
            self._tab[i] = (fwd, inv, pow(n, -1, q))
        return self._tab[i]

    def fwd(self, i, a):
        """coefficients (object) -> evaluations in bit-reversed order (object)"""
        q, n = self.q[i], self.n
        W = self._tables(i)[0]
        a = obj(a)
        m, t = 1, n
        while m < n:
            t //= 2
            a = a.reshape(m, 2, t)
            U, V = a[:, 0, :], a[:, 1, :] * W[m:2 * m].reshape(m, 1) % q
            a = np.stack([U + V, U - V], axis=1)
            m *= 2
        return a.reshape(n) % q

    def inv(self, i, A):
        q, n = self.q[i], self.n
        _, W, ninv = self._tables(i)
        a = obj(A)
        m, t = n // 2, 1
        while m >= 1:
            a = a.reshape(m, 2, t)
            U, V = a[:, 0, :], a[:, 1, :]
            a = np.stack([(U + V) % q, (U - V) * W[m:2 * m].reshape(m, 1) % q], axis=1)
            m //= 2
            t *= 2
        return a.reshape(n) * ninv % q

    def fwd_naive(self, i, a):
        """A[k] = a(psi^(2 brev(k) + 1)) by direct evaluation (small rings)"""
        q, psi = self.q[i], self.psi[i]
        out = []
        for k in range(self.n):
            x = pow(psi, 2 * int(self.brev[k]) + 1, q)
            out.append(sum(int(c) * pow(x, j, q) for j, c in enumerate(a)) % q)
        return np.array(out, dtype=object)

    def ntt_perm(self, g):
        """index map of the automorphism in the NTT domain, from the definition:
        sigma_g(a)(psi^e_k) = a(psi^(e_k g)), e_k = 2 brev(k) + 1, so
        out[k] = A[k'] with e_k' = e_k g mod 2n"""
        e = ((2 * self.brev + 1) * (g % (2 * self.n))) % (2 * self.n)
        return self.brev[(e - 1) // 2]

    def prime_of(self, t, ell):
        return t if t < ell else self.nq + (t - ell)

    def to_ntt(self, coef, idx):
        """[len(idx)][n] coefficients (any integers) -> NTT words at primes idx"""
        return np.stack([u64(self.fwd(i, obj(c) % self.q[i])) for c, i in zip(coef, idx)])

    # ---------------------------------------------------- conversions ----
    def modup(self, d):
        """[ell][n] NTT words -> [digits][ell + K][n] NTT words"""
        ell, K, al = len(d), self.K, self.alpha
        W = ell + K
        coef = [self.inv(i, d[i]) for i in range(ell)]
        out = np.empty(((ell + al - 1) // al, W, self.n), dtype=np.uint64)
        for j in range(out.shape[0]):
            lo, hi = j * al, min(ell, (j + 1) * al)
            Qj = 1
            for i in range(lo, hi):
                Qj *= self.q[i]
            S = 0
            for i in range(lo, hi):
                Qh = Qj // self.q[i]
                S = S + (coef[i] * pow(Qh, -1, self.q[i]) % self.q[i]) * Qh
            assert np.all(S < (hi - lo) * Qj)
            for t in range(W):
                if lo <= t < hi:
                    out[j, t] = d[t]
                else:
                    pt = self.prime_of(t, ell)
                    out[j, t] = u64(self.fwd(pt, S % self.q[pt]))
        return out

    def moddown(self, x, detail=False):
        """[ell + K][n] NTT words -> ([ell][n] NTT words, tie indices); with
        detail also (coefficients of the result, the other candidate's), both
        [ell][n] object arrays"""
        K, nq = self.K, self.nq
        ell = len(x) - K
        ps = self.q[nq:]
        XP, P = crt([self.inv(nq + k, x[ell + k]) for k in range(K)], ps)
        d2 = 2 * XP - P
        c = np.where(d2 < 0, XP, XP - P)
        ties = np.nonzero(np.abs(d2) * (1 << 53) <= tau_num(K) * P)[0]
        self.closest = min(getattr(self, 'closest', 1.0), float(min(np.abs(d2))) / float(P))
        other = np.where(d2 < 0, XP - P, XP)
        out = np.empty((ell, self.n), dtype=np.uint64)
        co, alt = [], []
        for i in range(ell):
            q = self.q[i]
            Pinv = pow(P, -1, q)
            out[i] = u64((obj(x[i]) - self.fwd(i, c % q)) * Pinv % q)
            if detail:
                xc = self.inv(i, x[i])
                co.append((xc - c) * Pinv % q)
                alt.append((xc - other) * Pinv % q)
        return (out, ties, co, alt) if detail else (out, ties)

    def rescale_poly(self, x):
        """[ell][n] NTT words -> [ell - 1][n]"""
        ell = len(x)
        ql = self.q[ell - 1]
        r = self.inv(ell - 1, x[ell - 1])
        c = np.where(2 * r < ql, r, r - ql)
        out = np.empty((ell - 1, self.n), dtype=np.uint64)
        for i in range(ell - 1):
            q = self.q[i]
            out[i] = u64((obj(x[i]) - self.fwd(i, c % q)) * pow(ql, -1, q) % q)
        return out

    def mod_raise_poly(self, x0):
        """[n] NTT words at q_0 -> [nq][n]: the centred lift to every Q prime"""
        q0 = self.q[0]
        r = self.inv(0, x0)
        c = np.where(2 * r < q0, r, r - q0)
        return np.stack([u64(self.fwd(i, c % self.q[i])) for i in range(self.nq)])

    # ------------------------------------------------------ key switch ----
    def keyswitch(self, d, key, g=None):
        """d [ell][n] NTT words, key [digits][2][nq + K][n] (b half, a half) ->
        ([2][ell][n] NTT words, tie indices); with g the extended digits pass
        through the automorphism before the product"""
        ell = len(d)
        ext = self.modup(d)
        if g is not None:
            ext = ext[:, :, self.ntt_perm(g)]
        W = ell + self.K
        out, ties = [], []
        for h in range(2):
            acc = []
            for t in range(W):
                pt = self.prime_of(t, ell)
                s = 0
                for j in range(ext.shape[0]):
                    s = s + obj(ext[j, t]) * obj(key[j, h, pt])
                acc.append(s % self.q[pt])
            o, ti = self.moddown(acc)
            out.append(o)
            ties.extend(int(v) for v in ti)
        return np.stack(out), sorted(set(ties))

    def _limbwise(self, f, ell):
        return np.stack([u64(f(i) % self.q[i]) for i in range(ell)])

    # ------------------------------------------------------- whole ops ----
    def rescale(self, ct):
        return np.stack([self.rescale_poly(ct[0]), self.rescale_poly(ct[1])])

    def mod_raise(self, ct):
        return np.stack([self.mod_raise_poly(ct[0][0]), self.mod_raise_poly(ct[1][0])])

    def mul(self, a, b, relin, ks=None):
        """([2][ell - 1][n], ties); ks: keyswitch(a1 b1, relin) if already at hand"""
        ell = a.shape[1]
        a0, a1, b0, b1 = obj(a[0]), obj(a[1]), obj(b[0]), obj(b[1])
        d0 = self._limbwise(lambda i: a0[i] * b0[i], ell)
        d1 = self._limbwise(lambda i: a0[i] * b1[i] + a1[i] * b0[i], ell)
        d2 = self._limbwise(lambda i: a1[i] * b1[i], ell)
        ks, ties = ks if ks is not None else self.keyswitch(d2, relin)
        t0 = self._limbwise(lambda i: obj(d0[i]) + obj(ks[0, i]), ell)
        t1 = self._limbwise(lambda i: obj(d1[i]) + obj(ks[1, i]), ell)
        return self.rescale(np.stack([t0, t1])), ties

    def square(self, a, relin):
        return self.mul(a, a, relin)

    def mul_plain(self, a, pt):
        """product with plaintext words [ell][n], then the rescale"""
        ell = a.shape[1]
        p = obj(pt)
        return self.rescale(np.stack([self._limbwise(lambda i: obj(a[h, i]) * p[i], ell) for h in range(2)]))

    def apply_galois(self, ct, g, key):
        ell = ct.shape[1]
        ks, ties = self.keyswitch(ct[1], key, g)
        perm = self.ntt_perm(g)
        c0 = self._limbwise(lambda i: obj(ct[0, i][perm]) + obj(ks[0, i]), ell)
        return np.stack([c0, ks[1]]), ties

    def rotate(self, ct, k, key):
        return self.apply_galois(ct, galois_of_rotation(self.logN, k), key)

    def rotate_hoisted(self, ct, ks, keys):
        """one ModUp serves every rotation: the same integers as rotate()"""
        return [self.rotate(ct, k, key) for k, key in zip(ks, keys)]

    def conjugate(self, ct, key):
        return self.apply_galois(ct, 2 * self.n - 1, key)

    # ---------------------------------------------------------- phases ----
    def phase(self, ct, s):
        """centred integer coefficients of c0 + c1 s over Q_ell (s: the secret's
        coefficients); ct may carry a third row d2, then + d2 s^2"""
        ell = ct.shape[1]
        res = []
        for i in range(ell):
            q = self.q[i]
            sn = self.fwd(i, obj(s) % q)
            v = obj(ct[0, i]) + obj(ct[1, i]) * sn
            if len(ct) == 3:
                v = v + obj(ct[2, i]) * sn * sn
            res.append(self.inv(i, v % q))
        X, Q = crt(res, self.q[:ell])
        return centre(X, Q), Q


# ------------------------------------------------------ boundary inputs ----
def rand_limbs(rng, primes, n):
    return np.stack([rng.integers(0, int(q), size=n, dtype=np.uint64) for q in primes])


def blocks(vals, n, width=13):
    """vals repeated in blocks of `width` coefficients over the ring (13: no
    multiple of any tile), the last coefficient on the last value"""
    out = np.array([vals[(k // width) % len(vals)] for k in range(n)], dtype=object)
    out[n - 1] = vals[-1]
    return out


def lift_boundary_values(q):
    """both sides of a centred lift's cut, and the ends of the range; ordered so
    that blocks() puts the cut's two sides on the ring's first and last coefficient"""
    return [(q - 1) // 2, 0, 1, q - 1, (q + 1) // 2]


def rescale_boundary_limb(model, ell):
    """NTT words of a last limb whose coefficients sit on the rescale's cut"""
    q = model.q[ell - 1]
    return u64(model.fwd(ell - 1, blocks(lift_boundary_values(q), model.n)))


def rescale_boundary_ct(model, rng, ell):
    """[2][ell][n]: random lower limbs, the last limb of both halves on the cut"""
    data = np.stack([rand_limbs(rng, model.q[:ell], model.n) for _ in range(2)])
    data[0, ell - 1] = rescale_boundary_limb(model, ell)
    data[1, ell - 1] = u64(model.fwd(ell - 1, blocks(lift_boundary_values(model.q[ell - 1])[::-1], model.n, 7)))
    return data


def mul_boundary_operands(model, rng, ell, relin):
    """(a, b, ks): ciphertexts whose product's first half, after the tensor and
    the relinearisation and before the rescale, has its last limb on the
    rescale's cut.  b = (1, b1), so d0 = a0, d2 = a1 b1 and the key-switch
    output does not depend on a0; a0's last limb is the boundary limb minus
    that output.  ks = keyswitch(a1 b1), for Model.mul."""
    n = model.n
    a = np.stack([rand_limbs(rng, model.q[:ell], n) for _ in range(2)])
    b = np.stack([np.ones((ell, n), dtype=np.uint64), rand_limbs(rng, model.q[:ell], n)])
    d2 = model._limbwise(lambda i: obj(a[1, i]) * obj(b[1, i]), ell)
    ks = model.keyswitch(d2, relin)
    q = model.q[ell - 1]
    a[0, ell - 1] = u64((obj(rescale_boundary_limb(model, ell)) - obj(ks[0][0, ell - 1])) % q)
    return a, b, ks


def moddown_input(model, rng, ell, XP):
    """[ell + K][n] NTT words: random Q limbs, the special limbs the residues of
    the integers XP (coefficient form)"""
    x = np.empty((ell + model.K, model.n), dtype=np.uint64)
    x[:ell] = rand_limbs(rng, model.q[:ell], model.n)
    for k in range(model.K):
        x[ell + k] = u64(model.fwd(model.nq + k, XP % model.q[model.nq + k]))
    return x


def moddown_exact_values(P):
    """far outside tau on both sides of P/2, and the ends of [0, P)"""
    v = [(P * ((1 << (s - 1)) + d)) >> s for s in (30, 45) for d in (-1, 1)]
    return v + [0, 1, P - 1]


def moddown_tie_input(model, rng, ell):
    """(x, tie indices): X_P = (P -+ 1)/2 at the tie indices, random elsewhere"""
    n, P = model.n, model.P
    XP = np.array([int(rng.integers(0, 1 << 62)) for _ in range(n)], dtype=object)
    for _ in range(model.K):
        XP = (XP << 60) + np.array([int(v) for v in rng.integers(0, 1 << 60, size=n)], dtype=object)
    XP = XP % P
    idx = [0, 5, n // 2 - 1, n // 2, n - 2, n - 1]
    for m, k in enumerate(idx):
        XP[k] = (P - 1) // 2 if m % 2 == 0 else (P + 1) // 2
    return moddown_input(model, rng, ell, XP), idx


def check_moddown_ties(model, x, got, idx):
    """got = an implementation's ModDown of x: exact outside the tie indices;
    at a tie either candidate, the same one in every limb"""
    words, ties, co, alt = model.moddown(x, detail=True)
    assert [int(t) for t in ties] == sorted(idx), 'the model sees other ties than were built'
    mask = np.zeros(model.n, dtype=bool)
    mask[idx] = True
    picks = []
    for i in range(len(co)):
        g = model.inv(i, got[i])
        main, other = g == co[i], g == alt[i]
        assert np.all(main[~mask]), f'limb {i}: wrong outside the ties'
        assert np.all(main[mask] | other[mask]), f'limb {i}: neither candidate at a tie'
        picks.append(main[mask])
    assert all(np.array_equal(p, picks[0]) for p in picks), 'limbs disagree on a tie candidate'


# --------------------------------------------------------- noise bounds ----
def keyswitch_noise_bound(model, ell, h):
    """Worst-case |phase(key-switched pair) - phase it stands for|, as a pair
    (numerator, denominator).

    A switching key's digit j is (b_j, a_j) with b_j + a_j s = P Qhat-part
    times the old secret + e_j, |e_j| <= 21 (CBD eta = 21).  The inner product
    therefore carries sum_j ext_j e_j beside P times the wanted term.  ext_j
    is ModUp's representative of digit j, 0 <= S < alpha Q_j, and a negacyclic
    product of n coefficients sums n terms, so every coefficient of the error
    is at most E = digits n alpha max_j Q_j 21 in magnitude.  ModDown divides
    by P and rounds each half to nearest (at a tie either way, still within
    1/2): the b half adds at most 1/2, the a half at most 1/2 per coefficient
    times s, i.e. h/2 with h the Hamming weight of the ternary s.  One unit of
    slack covers the rounding of E / P itself:

        bound = E / P + (1 + h)/2 + 1
    """
    al = model.alpha
    digits = (ell + al - 1) // al
    maxQ = 1
    for j in range(digits):
        Qj = 1
        for i in range(j * al, min(ell, (j + 1) * al)):
            Qj *= model.q[i]
        maxQ = max(maxQ, Qj)
    E = digits * model.n * al * maxQ * 21
    # E / P + (3 + h) / 2 = (2 E + (3 + h) P) / (2 P)
    return 2 * E + (3 + h) * model.P, 2 * model.P


def bits(x):
    return float(np.log2(max(1.0, float(x))))


def check_rotate_noise(model, ct_in, ct_out, g, s):
    """noise = centred(phase(out) - sigma_g(phase(in))) mod Q_ell is the key
    switch's own error, bounded by keyswitch_noise_bound (derivation there).
    Returns (measured bits, bound bits)."""
    ell = ct_in.shape[1]
    h = int(np.count_nonzero(s))
    pin, Q = model.phase(ct_in, s)
    pout, _ = model.phase(ct_out, s)
    noise = centre(pout - automorph_coeff(pin, g), Q)
    worst = max(abs(int(v)) for v in noise)
    num, den = keyswitch_noise_bound(model, ell, h)
    assert worst * den <= num, f'rotation noise 2^{bits(worst):.1f} above the bound 2^{bits(num // den):.1f}'
    return bits(worst), bits(num // den)


def check_mul_noise(model, a, b, out, s):
    """out = rescale(tensor + keyswitch(d2)), so with T = phase(a) phase(b) mod
    Q_ell (formed limb by limb as the phase of the tensor (d0, d1, d2))

        q_last phase(out) = T + key-switch error - (c0 + c1 s),

    c0, c1 the rescale's centred lifts, |c| <= q_last / 2: the magnitude of
    q_last phase(out) - T is at most B_ks + q_last (1 + h)/2 with B_ks the
    key-switch bound.  Divided by q_last this is the product's noise at its
    new scale: B_ks / q_last + (1 + h)/2, plus one unit of slack.  Returns
    (measured bits, bound bits) of that scaled noise."""
    ell = a.shape[1]
    ql = model.q[ell - 1]
    h = int(np.count_nonzero(s))
    a0, a1, b0, b1 = obj(a[0]), obj(a[1]), obj(b[0]), obj(b[1])
    tensor = np.stack([model._limbwise(lambda i: a0[i] * b0[i], ell),
                       model._limbwise(lambda i: a0[i] * b1[i] + a1[i] * b0[i], ell),
                       model._limbwise(lambda i: a1[i] * b1[i], ell)])
    T, Q = model.phase(tensor, s)
    pout, _ = model.phase(out, s)
    noise = centre(ql * pout - T, Q)
    worst = max(abs(int(v)) for v in noise)
    num, den = keyswitch_noise_bound(model, ell, h)
    # worst / q_last <= num / (den q_last) + (1 + h)/2 + 1 - 1 (the slack is in num / den already)
    assert worst * 2 * den <= 2 * num + (1 + h) * ql * den, \
        f'product noise 2^{bits(worst // ql):.1f} above the bound 2^{bits((2 * num + (1 + h) * ql * den) // (2 * den * ql)):.1f}'
    return bits(worst // ql), bits((2 * num + (1 + h) * ql * den) // (2 * den * ql))


# ============================================================================
# Constants, and sums of products of ciphertext words with constants
# ============================================================================
# A real constant x enters the arithmetic as the integer pair (k, sh) standing
# for k 2^sh ("constants carried as k 2^sh"): x itself rounded
# half away from zero while |x| <= 2^62, else the 62 leading bits of x and a
# shift.  Everything downstream is integer: the residue (k 2^sh) mod q
# multiplies words, sums are taken over the integers and reduced once.
def round_half_away(x):
    """the nearest integer to the double x, ties away from zero (exact: through
    the double's integer ratio, no floating-point add)"""
    num, den = float(x).as_integer_ratio()
    r = (2 * abs(num) + den) // (2 * den)
    return r if num >= 0 else -r


def scaled_const(x):
    """x -> (k, sh): (round(x), 0) if |x| <= 2^62; else sh = ceil(log2 |x|) - 62
    (log2 evaluated in doubles, as the specification states it) and
    k = round(x / 2^sh), the division by a power of two being exact"""
    x = float(x)
    if not np.isfinite(x):
        raise ValueError('scaled constant is not finite')
    if abs(x) <= 2.0 ** 62:
        return round_half_away(x), 0
    sh =math.ceil(math.log2(abs(x))) - 62
    return round_half_away(math.ldexp(x, -sh)), sh


def const_at_scale(c, scale):
    return scaled_const(float(c) * float(scale))


def const_to_target(c, delta_t, q_dropped, scale_in):
    """the constant that takes an input at scale_in to delta_t after the
    rescale by q_dropped: doubles, left to right"""
    return scaled_const(float(c) * float(delta_t) * float(int(q_dropped)) / float(scale_in))


def const_residue(k, sh, q):
    return (int(k) * 2 ** int(sh)) % int(q)


def linear_sums(xs, K, sh, primes, consts=None):
    """out_g[p][l] = sum_i residue(K[g][i], sh[g][i]; q_l) x_i[p][l] mod q_l over
    the ell = len(primes) limbs; an input with more limbs contributes its
    first ell.  consts = (Kc, shc): + residue(Kc[g]) q_{ell-1} mod q_l on c0
    (p = 0) for l < ell - 1; the last limb is left as it is.
    xs: [2][limbs_i][n] words each; returns G arrays [2][ell][n] (uint64)."""
    ell, G, m = len(primes), len(K), len(xs)
    n = np.asarray(xs[0]).shape[-1]
    out = [np.empty((2, ell, n), dtype=np.uint64) for _ in range(G)]
    for l, q in enumerate(int(p) for p in primes):
        W = np.array([[const_residue(K[g][i], sh[g][i], q) for i in range(m)] for g in range(G)], dtype=object)
        X = np.stack([obj(np.asarray(x)[:, l, :]).reshape(2 * n) for x in xs])  # [m][2 n]
        S = W.dot(X)  # exact integers
        for g in range(G):
            s = S[g].reshape(2, n)
            if consts is not None and l < ell - 1:
                s[0] = s[0] + const_residue(consts[0][g], consts[1][g], q) * int(primes[ell - 1])
            out[g][:, l, :] = u64(s % q)
    return out


def mul_plain_sum_words(cts, pts, primes):
    """sum_i ct_i pt_i over the limbs of `primes`, unrescaled: cts [2][ell][n], pts [ell][n]"""
    ell = len(primes)
    n = np.asarray(cts[0]).shape[-1]
    out = np.empty((2, ell, n), dtype=np.uint64)
    for l, q in enumerate(int(p) for p in primes):
        for h in range(2):
            s = 0
            for c, p in zip(cts, pts):
                s = s + obj(c[h][l]) * obj(p[l])
            out[h, l] = u64(s % q)
    return out


def _add_ops(cls):
    """the constant ops of the engine's surface as Model methods; every scale is
    an argument (a double), every ciphertext [2][limbs][n] words"""
    def ell_of(self, level):
        return self.nq - level

    def add_const(self, ct, c, scale):
        """c at the ciphertext's scale joins c0 on every limb"""
        k, sh = const_at_scale(c, scale)
        out = np.array(ct, dtype=np.uint64)
        for l in range(out.shape[1]):
            out[0, l] = u64((obj(ct[0][l]) + const_residue(k, sh, self.q[l])) % self.q[l])
        return out

    def mul_int(self, ct, k):
        return np.stack([self._limbwise(lambda i: obj(ct[h][i]) * int(k), np.asarray(ct).shape[1]) for h in range(2)])

    def mul_const_to(self, ct, c, scale_in, target, delta):
        """the first ell = limbs(target - 1) limbs times the constant that lands
        the product at delta[target], then the rescale"""
        ell = self.ell_of(target - 1)
        k, sh = const_to_target(c, delta[target], self.q[ell - 1], scale_in)
        prod = np.stack([self._limbwise(lambda i: obj(ct[h][i]) * const_residue(k, sh, self.q[i]), ell)
                         for h in range(2)])
        return self.rescale(prod)

    def mul_const(self, ct, c, scale_in, level, delta):
        return self.mul_const_to(ct, c, scale_in, level + 1, delta)

    def level_adjust(self, ct, scale_in, level, target, delta):
        """the product with 1.0 to the target level; the identity at its own level"""
        if target == level:
            return np.array(ct, dtype=np.uint64)
        return self.mul_const_to(ct, 1.0, scale_in, target, delta)

    def linear_sum_to(self, xs, cs, scales, target, delta):
        ell = self.ell_of(target - 1)
        ks = [const_to_target(c, delta[target], self.q[ell - 1], s) for c, s in zip(cs, scales)]
        return self.rescale(linear_sums(xs, [[k for k, _ in ks]], [[s for _, s in ks]], self.q[:ell])[0])

    def mul_plain_sum(self, cts, pts):
        """sum_i ct_i pt_i, one rescale"""
        return self.rescale(mul_plain_sum_words(cts, pts, self.q[:np.asarray(cts[0]).shape[1]]))

    def mul_plain_sum_batches(self, cts, pts_per_batch):
        """member b = mul_plain_sum(cts, pts_per_batch[b])"""
        return [self.mul_plain_sum(cts, pts) for pts in pts_per_batch]

    def mul_plain_sum_groups(self, members, pts, groups):
        """member g = mul_plain_sum(members[g Z : (g + 1) Z], pts), Z = len(pts)"""
        Z = len(pts)
        return [self.mul_plain_sum(members[g * Z:(g + 1) * Z], pts) for g in range(groups)]

    def mul_add_const(self, a, b, relin, level, scale_a, delta, xs=(), cs=(), scales=(), a_add=None, a_const=0.0,
                      out_const=0.0, ks=None):
        """(a [+ a_add] + a_const) b + sum_i cs_i xs_i + out_const with one
        relinearisation and one rescale; a, b (and a_add) at `level`.  Returns
        ([2][ell - 1][n], ModDown ties, ks); ks = keyswitch(d2) may be handed back
        in for another call with the same (a + a_add)_1 b_1."""
        ell = self.ell_of(level)
        a = np.asarray(a)
        left = np.array(a, dtype=np.uint64)
        if a_add is not None:
            left = np.stack([self._limbwise(lambda i: obj(a[h][i]) + obj(a_add[h][i]), ell) for h in range(2)])
        if a_const != 0.0:
            left = self.add_const(left, a_const, scale_a)
        a0, a1, b0, b1 = obj(left[0]), obj(left[1]), obj(b[0]), obj(b[1])
        d0 = self._limbwise(lambda i: a0[i] * b0[i], ell)
        d1 = self._limbwise(lambda i: a0[i] * b1[i] + a1[i] * b0[i], ell)
        d2 = self._limbwise(lambda i: a1[i] * b1[i], ell)
        if len(xs):
            kk = [const_to_target(c, delta[level + 1], self.q[ell - 1], s) for c, s in zip(cs, scales)]
            lin = linear_sums(xs, [[k for k, _ in kk]], [[s for _, s in kk]], self.q[:ell])[0]
            d0 = self._limbwise(lambda i: obj(d0[i]) + obj(lin[0][i]), ell)
            d1 = self._limbwise(lambda i: obj(d1[i]) + obj(lin[1][i]), ell)
        if out_const != 0.0:
            k, sh = const_at_scale(out_const, delta[level + 1])
            d0 = np.stack([u64((obj(d0[i]) + (const_residue(k, sh, self.q[i]) * self.q[ell - 1] if i < ell - 1 else 0))
                               % self.q[i]) for i in range(ell)])
        ks = ks if ks is not None else self.keyswitch(d2, relin)
        t0 = self._limbwise(lambda i: obj(d0[i]) + obj(ks[0][0, i]), ell)
        t1 = self._limbwise(lambda i: obj(d1[i]) + obj(ks[0][1, i]), ell)
        return self.rescale(np.stack([t0, t1])), ks[1], ks

    for f in (ell_of, add_const, mul_int, mul_const_to, mul_const, level_adjust, linear_sum_to, mul_plain_sum,
              mul_plain_sum_batches, mul_plain_sum_groups, mul_add_const):
        setattr(cls, f.__name__, f)


_add_ops(Model)


# ---------------------------------------------- the MFMA kernels' int32 rows ----
# The matrix-core kernels form an exact sum of products from signed bytes:
# a word y < q < 2^60 is read as the bytes u_0 .. u_7 (y = sum_a u_a 256^a), of
# which bytes 0..6 are taken as s_a = u_a - 128 in [-128, 128) and byte 7 as
# s_7 = u_7 in [0, 16); a constant c < q is written in balanced base-256
# digits, c = sum_d e_d 256^d with e_d in [-128, 128).  For c < 2^60 the top
# digit satisfies 0 <= e_7 <= 16: the seven lower digits sum to a value in
# [-128, 127] (256^7 - 1)/255, of magnitude below 0.502 2^56, so
# e_7 2^56 = c - (lower digits) lies in (-0.502 2^56, 16.502 2^56).
#
# The functions below restate the two decompositions.  They choose inputs and
# account for the int32 budget; expected outputs always come from linear_sums.
C0 = 0x0080808080808080  # sum_{a<7} 128 256^a: y = C0 + sum_a s_a 256^a


def balanced_digits(c):
    """the 8 balanced base-256 digits of 0 <= c < 2^60, least significant first"""
    v, out = int(c), []
    for _ in range(8):
        d = v & 255
        if d >= 128:
            d -= 256
        v = (v - d) >> 8
        out.append(d)
    assert v == 0 and sum(d << (8 * i) for i, d in enumerate(out)) == int(c)
    return out


def signed_bytes(ys):
    """ys: integer array [...] of words < 2^60 -> int64 [8][...]: s_a"""
    y = np.asarray(ys, dtype=np.uint64)
    return np.stack([((y >> np.uint64(8 * a)) & np.uint64(255)).astype(np.int64) - (128 if a < 7 else 0) for a in range(8)])


def _combined(rows):
    return rows[0::2] + 256 * rows[1::2]


def rows_window(residues, ys):
    """The window kernel's rows for one output: residues c_i (m ints), ys [m][...]
    words.  Row s (0..15) = sum_{i, a} s_{i,a} e_{s-a}(c_i); then
    sum_s v_s 256^s + C0 sum_i c_i = sum_i c_i y_i over the integers.
    Returns (rows [16][...], combined [8][...]) as int64, combined[j] =
    v_{2j} + 256 v_{2j+1}: the words the kernel forms in int32."""
    ys = np.asarray(ys, dtype=np.uint64)
    rows = np.zeros((16,) + ys.shape[1:], dtype=np.int64)
    for i, c in enumerate(residues):
        e, s = balanced_digits(c), signed_bytes(ys[i])
        for a in range(8):
            for d in range(8):
                if e[d]:
                    rows[a + d] += s[a] * e[d]
    return rows, _combined(rows)


def rows_fold(residues, ys, q):
    """The fold kernel's rows for one output: d_{i,a} = 256^a c_i mod q, row b
    (0..7) = sum_{i, a} s_{i,a} e_b(d_{i,a}); then
    sum_b v_b 256^b + 128 sum_{i, a<7} d_{i,a} = sum_i c_i y_i mod q.
    Returns (rows [8][...], combined [4][...]) as int64."""
    ys = np.asarray(ys, dtype=np.uint64)
    rows = np.zeros((8,) + ys.shape[1:], dtype=np.int64)
    for i, c in enumerate(residues):
        s = signed_bytes(ys[i])
        for a in range(8):
            e = balanced_digits(int(c) * 256 ** a % int(q))
            for b in range(8):
                if e[b]:
                    rows[b] += s[a] * e[b]
    return rows, _combined(rows)


def recombine_window(rows, residues):
    """sum_s v_s 256^s + C0 sum c: the integer sum_i c_i y_i (object array)"""
    return sum(obj(rows[s]) * 256 ** s for s in range(16)) + C0 * sum(int(c) for c in residues)


def recombine_fold(rows, residues, q):
    """sum_b v_b 256^b + 128 sum_{i, a<7} d_{i,a}, congruent to sum_i c_i y_i mod q"""
    corr = 128 * sum(int(c) * 256 ** a % int(q) for c in residues for a in range(7))
    return sum(obj(rows[b]) * 256 ** b for b in range(8)) + corr


def digit_table(form, residues, q):
    """int64 [m][8][8]: entry [i][a][b] = e_b(c_i) (window, the same for every
    a) or e_b(256^a c_i mod q) (fold)"""
    t = np.zeros((len(residues), 8, 8), dtype=np.int64)
    for i, c in enumerate(residues):
        for a in range(8):
            t[i, a] = balanced_digits(c if form == 'window' else int(c) * 256 ** a % int(q))
    return t


def byte_weights(form, residues, q, pair, table=None):
    """w[i][a]: the factor of s_{i,a} in the combined word `pair`
    (v_{2 pair} + 256 v_{2 pair + 1}) of one output; form 'window' or 'fold'"""
    t = digit_table(form, residues, q) if table is None else table
    w = np.zeros((len(residues), 8), dtype=np.int64)
    for a in range(8):
        for row, f in ((2 * pair, 1), (2 * pair + 1, 256)):
            d = row - a if form == 'window' else row
            if 0 <= d < 8:
                w[:, a] += f * t[:, a, d]
    return w


def extreme_word(w, sign, q):
    """the word y < q whose signed bytes push sum_a s_a w[a] furthest in the
    direction `sign`: from the top byte down, the largest byte the bound y <= q - 1
    still allows where sign w[a] > 0, else 0 (0xFF / 0x00 once below the bound)"""
    top = [((int(q) - 1) >> (8 * a)) & 255 for a in range(8)]
    y, tight = 0, True
    for a in range(7, -1, -1):
        hi = top[a] if tight else 255
        u = hi if sign * int(w[a]) > 0 else 0
        tight = tight and u == top[a]
        y |= u << (8 * a)
    assert y < int(q)
    return y


def target_words(form, residues, q, n):
    """[m][n] words below q for the sources of one limb; residues [G][m] are the
    constants' residues at this limb.  Coefficient k aims at the triple
    (output, pair, sign) number k mod (2 G P), P = 8 pairs (window) or 4 (fold):
    every byte of every source is set by the sign of the factor it meets in that
    combined word.  Returns (words, triples)."""
    G, m = len(residues), len(residues[0])
    P = 8 if form == 'window' else 4
    triples = [(g, p, s) for g in range(G) for p in range(P) for s in (1, -1)]
    cols, tables = [], {}
    for g, p, s in triples[:n]:
        if g not in tables:
            tables[g] = digit_table(form, residues[g], q)
        w = byte_weights(form, residues[g], q, p, tables[g])
        cols.append([extreme_word(w[i], s, q) for i in range(m)])
    out = np.empty((m, n), dtype=np.uint64)
    for k in range(n):
        out[:, k] = np.array(cols[k % len(cols)], dtype=np.uint64)
    return out, triples


def split30_middle(residues, ys):
    """The VALU sums split words and constants into 30-bit halves and keep the
    four partial sums of up to 16 terms in 64 bits each; the two middle ones
    are added before they join the 128-bit total.  Returns the largest
    s01 + s10 = sum_i lo(y_i) hi(c_i) + sum_i hi(y_i) lo(c_i) over the chunks of
    16 sources (ys [m][...]), as Python ints: at 2^64 and above the addition
    carries."""
    M30 = (1 << 30) - 1
    best = 0
    for base in range(0, len(residues), 16):
        mid = 0
        for i in range(base, min(len(residues), base + 16)):
            y, c = obj(ys[i]), int(residues[i])
            s01, s10 = (y & M30) * (c >> 30), (y >> 30) * (c & M30)
            mid = mid + s01 + s10
        best = max(best, int(np.max(mid)))
    return best


# worst cases over every y < q < 2^60 and c < q: |s_a| <= S_a, |e_d| <= E_d
_S = [128] * 7 + [15]
_E = [128] * 7 + [16]


def budget_bound_window(m):
    """max |v_s + 256 v_{s+1}|, s even, of the window kernel with m sources.
    v_s + 256 v_{s+1} = sum_i sum_a s_{i,a} (e_{s-a} + 256 e_{s+1-a}) (digits
    outside 0..7 are zero), so by the triangle inequality one source adds at
    most B_s = sum_a S_a (E_{s-a} + 256 E_{s+1-a}) with S = (128 x 7, 15) the
    byte magnitudes and E = (128 x 7, 16) the digit magnitudes derived above.
    The maximum over the even s is at s = 6: v_6 <= 7 2^14 = 114,688 and
    v_7 <= 128 16 + 6 2^14 + 15 128 = 102,272, B_6 = 26,296,320.  The bound is
    m B_6: 1,682,964,480 at m = 64, below 2^31 up to m = 81."""
    def E(d):
        return _E[d] if 0 <= d < 8 else 0
    return m * max(sum(_S[a] * (E(s - a) + 256 * E(s + 1 - a)) for a in range(8)) for s in range(0, 16, 2))


def budget_bound_fold(m):
    """max |v_b + 256 v_{b+1}|, b even, of the fold kernel with m sources.  Row b
    is sum_{i,a} s_{i,a} e_b(d_{i,a}) with d_{i,a} = 256^a c_i mod q any residue
    below q, so the digits of different a are independent and one source adds
    at most (sum_a S_a) E_b = 911 E_b to |v_b|: 116,608 for b < 7, 14,576 for
    b = 7.  The pairs (0,1), (2,3), (4,5) reach 257 x 116,608 = 29,968,256 per
    source, the pair (6,7) less.  The bound is 29,968,256 m: 1,917,968,384 at
    m = 64, below 2^31 up to m = 71 and above it from m = 72 -- this kernel
    is what limits the sources of one launch (LEAF_M)."""
    tot = sum(_S)
    return m * max(tot * (_E[b] + 256 * _E[b + 1]) for b in range(0, 8, 2))
