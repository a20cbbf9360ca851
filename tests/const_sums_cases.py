"""Inputs of tests/test_gpu_const_sums.py: shapes, words and constants for the
multi-output sums of products (Context.linear_sums_raw), built from the prime
list alone so that the parent test, its child processes and a machine without
a GPU all see the same cases.  Expected words come from
bigint_model.linear_sums; the conditions a case exists for (a carry of the
VALU middle sum, a full row of the window kernel, the reach of the targeted
words) are asserted here or in reach(), from the model alone."""
import json

import numpy as np

import bigint_model as M

ALL_MINUS_128_60 = 15 * 2 ** 56 - 0x80808080808080  # balanced digits (-128 x 7, 15)
ALL_MINUS_128_40 = 2 ** 40 - 0x8080808080            # (-128 x 5, 1, 0, 0)

# (logN, L, scale bits, seed): ring 2^10 is the smallest that takes k_leaf_sums_fold
CONTEXTS = {
    'r10-40': (10, 3, 40, 3), 'r10-41': (10, 3, 41, 4), 'r10-59': (10, 3, 59, 5),
    'r12-40': (12, 5, 40, 7), 'r12-41': (12, 5, 41, 41), 'r12-59': (12, 5, 59, 12),
}

# m, G, limbs dropped (level), stack members, folded constants, sources with more limbs, words
SHAPES_R10 = [
    (1, 1, 0, 1, False, False, 'mix'),
    (8, 4, 2, 1, True, True, 'mix'),       # ell = 2: cfold = 1
    (9, 5, 1, 3, True, True, 'mix'),       # KS = 2, NG = 2, an odd group count under the six-digit rows
    (9, 5, 0, 1, False, False, 'target'),
    (16, 8, 0, 1, False, False, 'mix'),    # Acc4 exactly full
    (17, 9, 0, 1, True, False, 'mix'),
    (33, 10, 0, 3, True, False, 'mix'),    # VALU: a second pass with accumulate, MLS_G full
    (33, 11, 2, 1, False, True, 'mix'),    # VALU: two output passes
    (56, 16, 0, 3, True, False, 'mix'),    # KS = 7: the six-digit rows
    (56, 16, 0, 1, False, False, 'target'),
    (57, 17, 0, 1, True, False, 'mix'),    # KS = 8: eight-digit rows, NG = 8
    (57, 17, 0, 1, False, False, 'target'),
    (64, 32, 0, 1, True, False, 'mix'),    # the launch maximum
    (64, 32, 0, 1, False, False, 'target'),
    (64, 32, 1, 1, True, False, 'random'),
    (65, 3, 0, 3, True, False, 'mix'),     # beyond LEAF_M: VALU with the matrix cores on, three passes
    (12, 33, 2, 1, True, True, 'mix'),     # two balanced passes of 17 and 16 outputs
]
SHAPES_R12 = [
    (1, 1, 0, 1, False, False, 'mix'),
    (8, 4, 4, 1, True, True, 'mix'),
    (9, 5, 1, 3, True, True, 'mix'),
    (16, 8, 0, 1, False, False, 'mix'),
    (17, 9, 0, 1, True, False, 'target'),
]

PATTERNS = [
    lambda q, n, rng: np.zeros(n, dtype=np.uint64),
    lambda q, n, rng: np.full(n, q - 1, dtype=np.uint64),
    lambda q, n, rng: np.where(np.arange(n) % 2 == 0, 0, q - 1).astype(np.uint64),
    lambda q, n, rng: np.full(n, q // 2, dtype=np.uint64),
    lambda q, n, rng: rng.integers(0, q, size=n, dtype=np.uint64),
    lambda q, n, rng: np.full(n, q // 2 + 1, dtype=np.uint64),
    lambda q, n, rng: (np.arange(n, dtype=np.uint64) % np.uint64(q)),
    lambda q, n, rng: rng.integers(0, q, size=n, dtype=np.uint64),
]
ONES, ZEROS = slice(0, 16), slice(16, 32)  # coefficients where every source is q - 1 / 0 ('mix')


def u62(rng):
    """uniform in [-2^62, 2^62]"""
    return int(rng.integers(-2 ** 62, 2 ** 62, endpoint=True))


def cyclic_constant(rng, j):
    """the special constants in turn: (K, sh)"""
    return [(0, 0), (1, 0), (-1, 0), (2 ** 62, 0), (-2 ** 62, 0), (u62(rng), 1), (u62(rng), 7), (u62(rng), 40),
            (u62(rng), 0), (ALL_MINUS_128_60, 0), (ALL_MINUS_128_40, 0), (-abs(u62(rng)), 0), (u62(rng), 0),
            (2 ** 62, 40)][j % 14]


class Case:
    def __init__(self, key, idx, shape, primes, nq, n):
        self.m, self.G, self.level, self.members, consts, deep, self.words = shape
        self.key, self.idx, self.n = key, idx, n
        self.ell = nq - self.level
        self.primes = [int(p) for p in primes[:self.ell]]
        self.name = f'{key} ({self.m}, {self.G}) ell={self.ell} x{self.members} {self.words}' + \
            (' consts' if consts else '') + (' deep' if deep else '')
        rng = np.random.default_rng([idx, n] + [p % (1 << 32) for p in self.primes])
        m, G = self.m, self.G
        # sources at `level`, or with every limb of the chain (a segment stride of their own)
        self.xlevels = [0 if deep and i % 2 else self.level for i in range(m)]
        # ---- constants
        if self.words == 'mix':
            kinds = ['neg1', 'a60', 'a40', 'pm62'] if G >= 5 else ['neg1', 'a60'][:G]
            rows = []
            for g in range(G):
                kind = kinds[g] if g < len(kinds) else 'cyc'
                if kind == 'neg1':
                    rows.append([(-1, 0)] * m)
                elif kind == 'a60':
                    rows.append([(ALL_MINUS_128_60, 0)] * m)
                elif kind == 'a40':
                    rows.append([(ALL_MINUS_128_40, 0)] * m)
                elif kind == 'pm62':
                    rows.append([(2 ** 62 if i % 2 == 0 else -2 ** 62, 0) for i in range(m)])
                else:
                    rows.append([cyclic_constant(rng, g + i) for i in range(m)])
        else:
            rows = [[(u62(rng), 0) for _ in range(m)] for _ in range(G)]
        self.K = [[k for k, _ in r] for r in rows]
        self.sh = [[s for _, s in r] for r in rows]
        self.consts = None
        if consts:
            kc = [cyclic_constant(rng, 3 * g + 2) for g in range(G)]
            self.consts = ([k for k, _ in kc], [s for _, s in kc])
        # ---- words: xs[i] [members][2][limbs_i][n]
        self.xs = []
        full = self.full = [int(p) for p in primes[:nq]]
        res = [[[M.const_residue(self.K[g][i], self.sh[g][i], q) for i in range(m)] for g in range(G)]
               for q in self.primes]
        if self.words == 'target':
            # c0 aims at the fold kernel's combined words, c1 at the window kernel's
            tw = [[M.target_words(form, res[l], q, n)[0] for l, q in enumerate(self.primes)] for form in ('fold', 'window')]
        for i in range(m):
            pr = full[:nq - self.xlevels[i]]
            x = np.empty((self.members, 2, len(pr), n), dtype=np.uint64)
            for z in range(self.members):
                for p in range(2):
                    for l, q in enumerate(pr):
                        if self.words == 'mix':
                            w = PATTERNS[(i + 3 * p + z) % 8](q, n, rng)
                            w[ONES], w[ZEROS] = q - 1, 0
                        elif self.words == 'target' and l < self.ell:
                            w = tw[p][l][i]
                        else:
                            w = rng.integers(0, q, size=n, dtype=np.uint64)
                        x[z, p, l] = w
            self.xs.append(x)
        self.check_conditions(res)

    def residues(self, l):
        q = self.primes[l]
        return [[M.const_residue(self.K[g][i], self.sh[g][i], q) for i in range(self.m)] for g in range(self.G)]

    def check_conditions(self, res):
        """what the case is for, from the model alone"""
        q0 = self.primes[0]
        assert ALL_MINUS_128_60 < q0 and all(ALL_MINUS_128_40 < q for q in self.primes)
        assert all(abs(k) <= 2 ** 62 for r in self.K for k in r)
        for x in self.xs:  # valid residues only
            assert all(int(x[:, :, l].max()) < self.full[l] for l in range(x.shape[2]))
        if self.words != 'mix':
            return
        # a negative K whose residue is q - 1, against words of q - 1
        assert self.K[0][0] == -1 and all(res[l][0][0] == q - 1 for l, q in enumerate(self.primes))
        assert all(int(x[0, 0, 0, 0]) == q0 - 1 and int(x[0, 0, 0, 16]) == 0 for x in self.xs)
        if self.m >= 16:
            # the VALU middle sum s01 + s10 carries out of 64 bits on the 60-bit limb
            mid = M.split30_middle(res[0][0], [x[0, 0, 0, :1] for x in self.xs])
            assert mid >= 2 ** 64, (self.name, mid)
            # (a 59-bit prime's upper half is below 2^29: 16 terms stop just short of 2^64 there)
        if self.G >= 2:
            # zero words against all -128 digits: a window row of exactly 7 2^14 m
            assert M.balanced_digits(res[0][1][0]) == [-128] * 7 + [15]
            rows, comb = M.rows_window(res[0][1], [x[0, 0, 0, 16:17] for x in self.xs])
            assert int(rows.max()) == 7 * 2 ** 14 * self.m, (self.name, int(rows.max()))
            if self.m == 64:
                assert int(rows.max()) == 7340032
        if self.G >= 3:
            # a constant in the large form (sh > 0) in every launch
            assert any(s > 0 for r in self.sh for s in r)

    def expected(self):
        """[G][members] arrays [2][ell][n], from the model"""
        outs = [M.linear_sums([x[z] for x in self.xs], self.K, self.sh, self.primes, self.consts)
                for z in range(self.members)]
        return [[outs[z][g] for z in range(self.members)] for g in range(self.G)]

    def reach(self, form, l, poly, outputs=None):
        """largest |combined int32 word| of the kernel form on limb l over this
        case's words of polynomial `poly` and over uniform random words of the
        same shape: (case, random)"""
        q = self.primes[l]
        rng = np.random.default_rng(l + 17)
        rnd = rng.integers(0, q, size=(self.m, self.n), dtype=np.uint64)
        mine = [x[0, poly, l] for x in self.xs]
        best = [0, 0]
        for r in self.residues(l)[:outputs]:
            for j, words in enumerate((mine, rnd)):
                comb = M.rows_fold(r, words, q)[1] if form == 'fold' else M.rows_window(r, words)[1]
                best[j] = max(best[j], int(np.abs(comb).max()))
        return best


_cache = {}


def cases(key, primes, nq):
    """the cases of one context (built once per process)"""
    if key not in _cache:
        logN = CONTEXTS[key][0]
        shapes = SHAPES_R10 if logN == 10 else SHAPES_R12
        _cache[key] = [Case(key, i, s, primes, nq, 1 << logN) for i, s in enumerate(shapes)]
    return _cache[key]


def expected_names(case, form):
    """the kernels one call of the case must launch: form 'fold' (default, or
    without the six-digit rows), 'window' (FHE_LEAF_FOLD=0) or 'valu'"""
    m, G = case.m, case.G
    passes = (G + 31) // 32
    per = (G + passes - 1) // passes
    sizes = [min(per, G - g0) for g0 in range(0, G, per)]
    names = set()
    for g in sizes:
        if form != 'valu' and m <= 64:
            groups = (g + 3) // 4
            ng = 1 if groups <= 1 else 2 if groups <= 2 else 4 if groups <= 4 else 8
            kernel = 'k_leaf_sums_fold' if form == 'fold' else 'k_leaf_sums_mfma'
            names.add(f'{kernel}<{(m + 7) // 8}, {ng}>')
        else:
            for g0 in range(0, g, 10):
                names.add(f'k_linear_sum_multi<{min(10, g - g0)}>')
    return names


def sum_kernels(stats):
    return {k for k in stats if k.startswith(('k_leaf_sums', 'k_linear_sum'))}


def run_case(F, gpu, xs, xlevels, members, K, sh, consts, level):
    """one call of linear_sums_raw on the engine: ([G][members][2][ell][n] words,
    the names of the sum kernels it launched)"""
    cts = []
    for x, lv in zip(xs, xlevels):
        ms = [gpu.upload(x[z], lv, 8) for z in range(members)]
        cts.append(gpu.stack(ms) if members > 1 else ms[0])
    with F.KernelClock(gpu) as clk:
        outs = gpu.linear_sums_raw(cts, K, sh, level, consts)
    for o in outs:
        assert o.info()['level'] == level, o.info()
    got = np.stack([np.stack([(gpu.member(o, z) if members > 1 else o).data() for z in range(members)]) for o in outs])
    return got, sum_kernels(clk.stats)


def first_difference(got, want):
    """(member, polynomial, limb, coefficient) of the first differing word"""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return f'{len(bad)} words differ, first at (member, poly, limb, coefficient) = {bad[0].tolist()}'


# ------------------------------------------------- files for a child process ----
def save_inputs(path, all_cases):
    arrs, meta = {}, []
    for ci, c in enumerate(all_cases):
        for i, x in enumerate(c.xs):
            arrs[f'c{ci}_x{i}'] = x
        arrs[f'c{ci}_K'] = np.array(c.K, dtype=np.int64)
        arrs[f'c{ci}_sh'] = np.array(c.sh, dtype=np.uint8)
        if c.consts:
            arrs[f'c{ci}_Kc'] = np.array(c.consts[0], dtype=np.int64)
            arrs[f'c{ci}_shc'] = np.array(c.consts[1], dtype=np.uint8)
        meta.append(dict(key=c.key, m=c.m, G=c.G, level=c.level, members=c.members, xlevels=c.xlevels,
                         consts=bool(c.consts), name=c.name))
    arrs['meta'] = np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8)
    np.savez(path, **arrs)
