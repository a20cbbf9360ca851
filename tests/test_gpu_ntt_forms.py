"""Every compiled form of the 256-point NTT row passes against the CPU oracle.

csrc/device/ntt.hip compiles, for each row pass of rings 2^16 and 2^17, the
register-only DPP kernels k_ntt_fwd_row<MODE, FULL, TWL, FP> /
k_ntt_inv_row<FULL, TWL, FP> and the LDS-exchange kernels
k_ntt_fwd<8, 4, false, MODE, FULL, FP> / k_ntt_inv<8, 4, false, FULL, FP>;
launch_pass_one picks among them from FHE_NTT_ROW_SHFL (default 15),
FHE_NTT_FULL (default 181), FHE_NTT_TWL (default 1) and FHE_NTT_TWL_ROWS
(default 4), each read once per process.  Under the defaults most of that
matrix never runs.  Here each switch set runs in a child process of its own,
one after the other, and every word is compared with the CPU oracle (and, for
the transform of every prime, with tests/bigint_model.py); no child compares
the engine with itself.  The module fixture builds the inputs, the keys and the
expected words once and writes them to a temporary directory; the children load
them, run the engine and compare, so the oracle is paid for once.

Contexts (L = 6, dnum 3, alpha = 3): ring 2^16 at a 41-bit scale (the prime
classes interleave: every MODE runs with FP true and false), ring 2^16 at a
40-bit scale (q_0 the only integer limb beside six fp64 limbs), ring 2^17 at 41
bits with the reduced list (the transforms on device memory, the 5-member
product at level 0, rescales, rotations), rings 2^12 and 2^15 at 41 bits for
the two LDS children, which are the ones that turn FHE_NTT_FULL for every pass
(6 + 6 and 8 + 7 bit passes).

Operations: fhe_ntt_dev forward and inverse over primes 0..4 of 1, 2, 3, 5 and
17 segments (lsegb 0..4, ragged last blocks) on random words and on all 0, all
q - 1 and 0 / q - 1 alternating; the transform of every prime against the
big-integer model (one FULL=255 and one FULL=0 child); ModUp at ell = L + 1,
alpha + 1 and alpha; products of 1-, 4- and 5-member stacks at level 0 (MODE 3)
and at ell = alpha (MODE 5 where the key switch fuses, four members and up; the
4-member stack is the one whose grid of eight segments is exact); rescales (MODE 1 columns, MODE 2 rows) and rotations by 1 (MODE 4) of the 1- and
5-member stacks.  The rescale's lifted column pass is the per-limb kernel in
all of these: k_ntt_lift_loop needs more blocks than five members give
(tests/test_gpu_rescale_lift.py runs it).

What the kernel clock cannot show is that FHE_NTT_AUX=1 forked: launch_pass
turns the fork off under the clock.  It forks when a pass splits into exactly
two pieces (one integer, one fp64 launch) and the smaller covers at most two
limbs (AUX_MAX_LIMBS): in the 40-bit context every pass over the Q limbs is
q_0 beside fp64 limbs (one limb against up to six), and the transforms of primes
0..4 are one limb against four, so the aux child's products, rescales,
rotations and transforms all cross the two streams.

The last test takes the union of the forms the children's clocks showed and
asserts the whole PB = 8 row matrix, written out there.
"""
import json
import os
import shutil
import subprocess
import sys
import time

import numpy as np
import pytest

import bigint_model as M
import pyoracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

L, DNUM = 6, 3
# name -> (logN, L, scale bits, seed); 'cheb' is the depth the degree-70 series needs
CONTEXTS = {'r16s41': (16, L, 41, 1641), 'r16s40': (16, L, 40, 1640), 'r17s41': (17, L, 41, 1741),
            'r12s41': (12, L, 41, 1241), 'r15s41': (15, L, 41, 1541), 'cheb': (16, 12, 41, 28)}
NTT_PRIMES = 5
POOL = 17  # segments of the transform pool: 0..13 random, 14 all 0, 15 all q - 1, 16 alternating

# shared with the children: the template arguments of a clocked NTT kernel name
PARSE = r'''
def form_of(name):
    """k_ntt_fwd_row<MODE, FULL, TWL, FP> -> ('fwd_row', MODE, FULL, TWL, FP);
    k_ntt_inv_row<FULL, TWL, FP> -> ('inv_row', FULL, TWL, FP);
    k_ntt_fwd<PB, EB, COLS, MODE, FULL, FP> -> ('fwd', PB, COLS, MODE, FULL, FP);
    k_ntt_inv<PB, EB, COLS, FULL, FP> -> ('inv', PB, COLS, FULL, FP); anything else: None"""
    base = name.split('@')[0]
    if '<' not in base:
        return None
    fam, args = base.split('<', 1)
    a = [(x == 'true') if x in ('true', 'false') else x for x in args.rstrip('>').split(', ')]
    if fam == 'k_ntt_fwd_row':
        return ('fwd_row', int(a[0]), a[1], a[2], a[3])
    if fam == 'k_ntt_inv_row':
        return ('inv_row', a[0], a[1], a[2])
    if fam == 'k_ntt_fwd':
        return ('fwd', int(a[0]), a[2], int(a[3]), a[4], a[5])
    if fam == 'k_ntt_inv':
        return ('inv', int(a[0]), a[2], a[3], a[4])
    return None
'''
_shared = {}
exec(PARSE, _shared)
form_of = _shared['form_of']

CHILD = PARSE + r'''
import ctypes as C
import json
import os
import sys
import time
import numpy as np
sys.path.insert(0, sys.argv[1])
import fhesort as F
mode, store, contexts = sys.argv[2], sys.argv[3], sys.argv[4].split(',')
META = json.load(open(os.path.join(store, 'meta.json')))
BOTH = (False, True)
ROW_MODES = (0, 2, 3, 4, 5)


class Keys:
    """the oracle's keys as the fixture stored them (Context.load_keys_from)"""
    def __init__(self, z): self.z = z
    def secret_ntt(self): return self.z['secret']
    def public_key(self): return self.z['public']
    def relin_key(self): return self.z['relin']
    def rot_key(self, k): return (1, self.z['rot1']) if k == 1 and 'rot1' in self.z else (0, None)


hip = C.CDLL('libamdhip64.so')
hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
hip.hipFree.argtypes = [C.c_void_p]
hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]


def same(g, want, info, what):
    gi = g.info()
    got = np.array([gi['level'], gi['slots'], gi['scale'], gi['limbs']], dtype=np.float64)
    assert np.array_equal(got, info), (what, got.tolist(), info.tolist())
    gd = g.data()
    assert gd.shape == want.shape, (what, gd.shape, want.shape)
    if not np.array_equal(gd, want):
        bad = np.argwhere(gd != want)
        raise AssertionError(f'{what}: {len(bad)} limb words differ, first at {bad[0].tolist()}')


def run(name):
    t0 = time.time()
    logn, depth, bits, seed = META['contexts'][name]
    z = np.load(os.path.join(store, name + '.npz'))
    gpu = F.Context(logn, depth, bits, 60, 3, seed=seed, keygen=False)
    gpu.load_keys_from(Keys(z), [1])
    assert np.array_equal(z['primes'], gpu.primes), name
    n, alpha, nq = gpu.n, gpu.alpha, gpu.nq
    names = set()
    use_clock = mode != 'aux'  # launch_pass forks only outside the clock

    def clocked(fn):
        if not use_clock:
            return set(), fn()
        with F.KernelClock(gpu) as clk:
            r = fn()
        names.update(clk.stats)
        return set(clk.stats), r

    def stack(data, level, k):
        cts = [gpu.upload(x, level, 16) for x in data[:k]]
        return gpu.stack(cts) if k > 1 else cts[0]

    def members(R, k, want, info, what):
        for m in range(k):
            same(gpu.member(R, m) if k > 1 else R, want[m], info, f'{name} {what}, member {m} of {k}')

    def transforms():
        pool, want = z['ntt_in'], z['ntt_want']
        sels = [[0], [14], [15], [16], [0, 16], [14, 15], [1, 2, 3], [14, 15, 16], [0, 14, 15, 16, 1], list(range(17))]
        for sel in sels:
            x = np.ascontiguousarray(pool[sel])
            p = C.c_void_p()
            assert hip.hipMalloc(C.byref(p), x.nbytes) == 0
            try:
                assert hip.hipMemcpy(p, x.ctypes.data, x.nbytes, 1) == 0
                got, back = np.empty_like(x), np.empty_like(x)

                def both():
                    gpu.ntt_dev(p.value, 0, x.shape[1], segments=len(sel), seg_stride=x.shape[1] * n)
                    gpu.sync()
                    assert hip.hipMemcpy(got.ctypes.data, p, x.nbytes, 2) == 0
                    gpu.ntt_dev(p.value, 0, x.shape[1], inverse=True, segments=len(sel), seg_stride=x.shape[1] * n)
                    gpu.sync()
                    assert hip.hipMemcpy(back.ctypes.data, p, x.nbytes, 2) == 0
                clocked(both)
            finally:
                hip.hipFree(p)
            if not np.array_equal(got, want[sel]):
                bad = np.argwhere(got != want[sel])
                raise AssertionError(f'{name} ntt_dev forward, segments {sel}: {len(bad)} words differ, first (segment, '
                                     f'prime, index) {bad[0].tolist()}')
            assert np.array_equal(back, x), f'{name} ntt_dev: the inverse does not restore segments {sel}'

    def model_transforms():
        X = np.zeros(n, dtype=np.uint64)
        X[1] = 1
        # the model took its roots from the oracle's transform: it models the engine's if the roots agree
        assert [int(gpu.ntt(i, X)[0]) for i in range(nq + gpu.K)] == [int(v) for v in z['mdl_psi']], name
        for i in range(nq + gpu.K):
            x = z['mdl_x'][i]
            (_, f), (_, b) = clocked(lambda: gpu.ntt(i, x)), clocked(lambda: gpu.ntt(i, x, inverse=True))
            assert np.array_equal(f, z['mdl_fwd'][i]), f'{name} model forward, prime {i}'
            assert np.array_equal(b, z['mdl_inv'][i]), f'{name} model inverse, prime {i}'

    def modups():
        for ell in (nq, alpha + 1, alpha):
            d = z[f'modup_in{ell}']
            assert np.array_equal(clocked(lambda: gpu.modup(d))[1], z[f'modup_want{ell}']), f'{name} modup ell={ell}'

    def products(level, counts):
        got = {}
        for k in counts:
            S, T = stack(z[f'a{level}'], level, k), stack(z[f'b{level}'], level, k)
            got[k], R = clocked(lambda: gpu.mul(S, T))
            members(R, k, z[f'mul{level}'], z[f'mul{level}_info'], f'product at level {level}')
        return got

    def rescales(counts):
        for k in counts:
            S = stack(z['a0'], 0, k)
            members(clocked(lambda: gpu.rescale(S))[1], k, z['res0'], z['res0_info'], 'rescale')

    def rotations(counts):
        for k in counts:
            S = stack(z['a0'], 0, k)
            members(clocked(lambda: gpu.rotate(S, 1))[1], k, z['rot0'], z['rot0_info'], 'rotate 1')

    own = nq - alpha  # the level where ell = alpha: one digit
    reduced = logn == 17
    if mode == 'shapes':
        shapes(name, z, gpu, clocked, stack, members, products, rotations, modups)
    elif name == 'cheb':
        raise AssertionError('the series context belongs to the shapes child')
    else:
        transforms()
        if logn == 16 and bits == 41 and mode in ('dpp-full-twl', 'lds-checked'):
            model_transforms()
        if mode != 'aux' and not reduced:
            modups()
        if reduced:
            products(0, (5,))
        else:
            products(0, (1, 4, 5))
            got = products(own, (1, 4, 5))
            if use_clock and logn >= 16:  # the one-digit closing row forms the own-digit key product itself
                for k in (4, 5):
                    assert any(s.startswith(('k_ntt_fwd_row<5,', 'k_ntt_fwd<8, 4, false, 5,')) for s in got[k]), \
                        (name, k, sorted(got[k]))
        rescales((1, 5))
        rotations((1, 5))
    forms = {form_of(s) for s in names} - {None}
    for s in sorted({s.split('@')[0] for s in names if s.startswith(('k_ntt_', 'k_ks_inner'))}):
        print('FORM', name, s, flush=True)
    check_forms(name, logn, bits, forms, names)
    gpu.close()
    print(f'TIME {name} {time.time() - t0:.2f}', flush=True)


def shapes(name, z, gpu, clocked, stack, members, products, rotations, modups):
    """FHE_KS_FUSE_MIN=1 FHE_KS_MC=4 FHE_CONV_CHUNK=5 FHE_PS_XCD=0"""
    def row_ks(among):  # k_ntt_row_ks<D, FP, FULL>
        return [s.split('@')[0].rstrip('>').split(', ')[-1] in ('false', '0') for s in among if s.startswith('k_ntt_row_ks<')]
    if name == 'r16s41':
        # 1, 2 and 3 members: lmb = 2, a partial block of four members
        for level in (0, gpu.nq - gpu.alpha):
            for k, among in products(level, (1, 2, 3)).items():
                assert row_ks(among) and all(row_ks(among)), (name, level, k, sorted(among))
        rotations((1, 2, 3))
        modups()  # ell + K = 10, 7 and 6 targets in chunks of five
        cts = [gpu.upload(x, 0, 16) for x in z['a0'][:3]]
        pts = [gpu.upload_pt(p, 0, 16) for p in z['pts']]
        among, R = clocked(lambda: gpu.mul_plain_sum(cts, pts))
        assert any(s.startswith('k_mul_plain_sum') for s in among), sorted(among)
        same(R, z['mps'], z['mps_info'], f'{name} mul_plain_sum')
    elif name == 'cheb':
        x = gpu.upload(z['x'], int(z['x_info'][0]), int(z['x_info'][1]), float(z['x_info'][2]))
        same(clocked(lambda: gpu.cheb(x, z['coeffs']))[1], z['series'], z['series_info'], 'degree-70 series')
    elif name == 'r12s41':
        # nothing fuses below ring 2^16: eight members take k_ks_inner_mc<3, 8> by default
        S, T = stack(z['a8'], 0, 8), stack(z['b8'], 0, 8)
        among, R = clocked(lambda: gpu.mul(S, T))
        assert any(s.startswith('k_ks_inner_mc<3, 4>') for s in among), sorted(among)
        members(R, 8, z['mul8'], z['mul8_info'], 'product of eight')
    else:
        raise AssertionError(name)


def check_forms(name, logn, bits, forms, names):
    """the forms this child's switches ask for are the ones its clock shows"""
    if mode in ('aux', 'shapes'):
        return
    full, checked = mode.split('-')[1] == 'full', mode.split('-')[1] == 'checked'
    flag = {f: (f[2] if f[0] in ('fwd_row',) else f[1] if f[0] == 'inv_row' else f[4] if f[0] == 'fwd' else f[3])
            for f in forms}
    if checked:
        assert not any(flag.values()), (name, sorted(f for f in forms if flag[f]))
    missing = []

    def need(f):
        if f not in forms:
            missing.append(f)
    rows = [f for f in forms if f[0] in ('fwd_row', 'inv_row')]
    lds_rows = [f for f in forms if f[0] in ('fwd', 'inv') and f[1] == 8 and f[2] is False]
    if mode.startswith('lds'):
        assert not rows, (name, sorted(rows))
        # the LDS kernels' grids are exact at every ring here: FULL=255 leaves no checked form
        if full:
            assert all(flag.values()), (name, sorted(f for f in forms if not flag[f]))
        if logn >= 16:
            # (ring 2^17: the reduced list has no ell = alpha product)
            for fp in BOTH:
                for m in (ROW_MODES if logn == 16 else ROW_MODES[:-1]):
                    need(('fwd', 8, False, m, full, fp))
                need(('inv', 8, False, full, fp))
                need(('fwd', (logn + 1) // 2, True, 1, full, fp))  # the rescale's lifted column pass
    else:
        twl = mode.endswith('-twl')
        assert logn >= 16 and rows and not lds_rows, (name, sorted(lds_rows))
        assert all((f[3] if f[0] == 'fwd_row' else f[2]) == twl for f in rows), (name, twl, sorted(rows))
        for fp in BOTH:
            for m in (ROW_MODES if logn == 16 else ROW_MODES[:-1]):
                # the exact grid (1 or 4 members, 1 or 2 segments) and the ragged one (5 members; 3, 5, 17
                # segments); ring 2^17's only product is the ragged one
                if not (logn == 17 and m == 3):
                    need(('fwd_row', m, full, twl, fp))
                need(('fwd_row', m, False, twl, fp))
            need(('inv_row', full, twl, fp))
            need(('inv_row', False, twl, fp))
    assert not missing, (name, mode, 'not launched:', missing, 'launched:', sorted(forms, key=str))


t0 = time.time()
for name in contexts:
    run(name)
print(f'TIME all {time.time() - t0:.2f}', flush=True)
print('ALLOK')
'''


def rand_limbs(rng, primes, n):
    return np.stack([rng.integers(0, int(q), size=n, dtype=np.uint64) for q in primes])


def info_of(ct):
    i = ct.info()
    return np.array([i['level'], i['slots'], i['scale'], i['limbs']], dtype=np.float64)


def results(cts):
    """[members][2][limbs][n] and the members' common (level, slots, scale, limbs)"""
    infos = [info_of(c) for c in cts]
    assert all(np.array_equal(i, infos[0]) for i in infos)
    return np.stack([c.data() for c in cts]), infos[0]


def build_context(name, path):
    """inputs, keys and the oracle's words of one context into one .npz"""
    logN, depth, bits, seed = CONTEXTS[name]
    orc = O.Context(logN, depth, bits, 60, DNUM, seed=seed)
    out = {'primes': orc.primes, 'secret': orc.secret_ntt(), 'public': orc.public_key(), 'relin': orc.relin_key()}
    rng = np.random.default_rng(seed)
    n, nq, alpha = orc.n, orc.nq, orc.alpha

    def cts(level, count):
        pr = orc.primes[:nq - level]
        data = np.stack([np.stack([rand_limbs(rng, pr, n), rand_limbs(rng, pr, n)]) for _ in range(count)])
        return data, [orc.ct_from(d, level, 16) for d in data]

    if name == 'cheb':
        c = np.random.default_rng(70).normal(size=71) / (1 + np.arange(71))
        ox = orc.encrypt(np.linspace(-1, 1, 16), 16, 5)
        out['coeffs'], out['x'], out['x_info'] = c, ox.data(), info_of(ox)
        out['series'], out['series_info'] = results([orc.cheb(ox, c)])
        out['series'] = out['series'][0]
        np.savez(path, **out)
        return
    assert (alpha, nq, orc.K) == (3, L + 1, 3)
    orc.gen_rotation_keys([1])
    out['rot1'] = orc.rot_key(1)[1]
    # the transform pool over primes 0..4
    pool = np.stack([rand_limbs(rng, orc.primes[:NTT_PRIMES], n) for _ in range(POOL)])
    for i in range(NTT_PRIMES):
        q1 = np.uint64(int(orc.primes[i]) - 1)
        pool[14, i] = 0
        pool[15, i] = q1
        pool[16, i] = 0
        pool[16, i, 1::2] = q1
    out['ntt_in'] = pool
    out['ntt_want'] = np.stack([np.stack([orc.ntt(i, pool[s, i]) for i in range(NTT_PRIMES)]) for s in range(POOL)])
    reduced = logN == 17
    if not reduced:
        for ell in (nq, alpha + 1, alpha):
            out[f'modup_in{ell}'] = rand_limbs(rng, orc.primes[:ell], n)
            out[f'modup_want{ell}'] = orc.modup(out[f'modup_in{ell}'])
    for level in (0,) if reduced else (0, nq - alpha):
        out[f'a{level}'], xs = cts(level, 5)
        out[f'b{level}'], ys = cts(level, 5)
        out[f'mul{level}'], out[f'mul{level}_info'] = results([orc.mul(x, y) for x, y in zip(xs, ys)])
        if level == 0:
            out['res0'], out['res0_info'] = results([orc.rescale(x) for x in xs])
            out['rot0'], out['rot0_info'] = results([orc.rotate(x, 1) for x in xs])
            if name == 'r16s41':  # the shapes child's sum of plaintext products
                pts = [orc.encode(rng.uniform(-1, 1, 16), 16, 0) for _ in range(3)]
                out['pts'] = np.stack([p.data() for p in pts])
                mps, out['mps_info'] = results([orc.mul_plain_sum(xs[:3], pts)])
                out['mps'] = mps[0]
    if name == 'r12s41':  # the shapes child's stack of eight
        out['a8'], xs = cts(0, 8)
        out['b8'], ys = cts(0, 8)
        out['mul8'], out['mul8_info'] = results([orc.mul(x, y) for x, y in zip(xs, ys)])
    if name == 'r16s41':  # the transform of every prime by the big-integer model
        m = M.Model(logN, orc.primes, nq, orc.K, alpha, orc.ntt)
        mrng = np.random.default_rng(1)
        x = np.stack([mrng.integers(0, q, size=n, dtype=np.uint64) for q in m.q])
        out['mdl_x'], out['mdl_psi'] = x, np.array(m.psi, dtype=np.uint64)
        out['mdl_fwd'] = np.stack([M.u64(m.fwd(i, x[i])) for i in range(len(m.q))])
        out['mdl_inv'] = np.stack([M.u64(m.inv(i, x[i])) for i in range(len(m.q))])
    np.savez(path, **out)


@pytest.fixture(scope='module')
def store(tmp_path_factory):
    t0 = time.time()
    d = tmp_path_factory.mktemp('ntt_forms')
    for name in CONTEXTS:
        build_context(name, str(d / (name + '.npz')))
    with open(d / 'meta.json', 'w') as f:
        json.dump({'contexts': CONTEXTS}, f)
    print(f'fixture (CPU oracle and model): {time.time() - t0:.1f} s')
    yield str(d)
    shutil.rmtree(d, ignore_errors=True)  # 1.8 GB of keys, inputs and expected words


FORMS = {}  # child -> the forms its kernel clocks showed at rings 2^16 and 2^17
NAMES = {}  # child -> every NTT / key-switch kernel name it printed

FORM_CONTEXTS = 'r16s41,r16s40,r17s41'
CHILDREN = {
    'lds-full': (dict(FHE_NTT_ROW_SHFL='0', FHE_NTT_FULL='255'), FORM_CONTEXTS + ',r12s41,r15s41'),
    'lds-checked': (dict(FHE_NTT_ROW_SHFL='0', FHE_NTT_FULL='0'), FORM_CONTEXTS + ',r12s41,r15s41'),
    'dpp-full-twl': (dict(FHE_NTT_ROW_SHFL='31', FHE_NTT_FULL='255', FHE_NTT_TWL_ROWS='16'), FORM_CONTEXTS),
    'dpp-full-notwl': (dict(FHE_NTT_ROW_SHFL='31', FHE_NTT_FULL='255', FHE_NTT_TWL='0'), FORM_CONTEXTS),
    'dpp-checked-twl': (dict(FHE_NTT_ROW_SHFL='31', FHE_NTT_FULL='0', FHE_NTT_TWL_ROWS='16'), FORM_CONTEXTS),
    'dpp-checked-notwl': (dict(FHE_NTT_ROW_SHFL='31', FHE_NTT_FULL='0', FHE_NTT_TWL='0'), FORM_CONTEXTS),
    'shapes': (dict(FHE_KS_FUSE_MIN='1', FHE_KS_MC='4', FHE_CONV_CHUNK='5', FHE_PS_XCD='0'), 'r16s41,cheb,r12s41'),
    'aux': (dict(FHE_NTT_AUX='1'), 'r16s40'),
}
SWITCHES = sorted({k for env, _ in CHILDREN.values() for k in env})


def run_child(mode, store):
    switches, contexts = CHILDREN[mode]
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(switches)
    t0 = time.time()
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'), mode, store, contexts],
                       env=env, capture_output=True, text=True, timeout=280)
    print(f'child {mode}: {time.time() - t0:.1f} s; ' +
          ', '.join(ln[5:] for ln in r.stdout.splitlines() if ln.startswith('TIME ')))
    lines = [ln.split(' ', 2) for ln in r.stdout.splitlines() if ln.startswith('FORM ')]
    NAMES[mode] = sorted({(w[1], w[2]) for w in lines})
    FORMS[mode] = {form_of(w[2]) for w in lines if w[1] in ('r16s41', 'r16s40', 'r17s41')} - {None}
    for ctx, name in NAMES[mode]:
        print('   ', ctx, name)
    assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}'


def test_lds_rows_exact_grid(store):
    """FHE_NTT_ROW_SHFL=0 FHE_NTT_FULL=255: k_ntt_fwd<8, 4, false, M, true, *> for M = 0, 2, 3, 4, 5,
    k_ntt_inv<8, 4, false, true, *>, the lifted column pass with FULL = true, no k_ntt_*_row; rings 2^12 and
    2^15 with every pass on its exact-grid form"""
    run_child('lds-full', store)


def test_lds_rows_checked(store):
    """FHE_NTT_ROW_SHFL=0 FHE_NTT_FULL=0: the same with the bounds-checked forms, at every ring"""
    run_child('lds-checked', store)


def test_dpp_rows_exact_grid_staged(store):
    """FHE_NTT_ROW_SHFL=31 FHE_NTT_FULL=255 FHE_NTT_TWL_ROWS=16: k_ntt_fwd_row<M, true, true, *> and
    k_ntt_inv_row<true, true, *> where the grid is exact, <.., false, true, ..> on the ragged segment counts"""
    run_child('dpp-full-twl', store)


def test_dpp_rows_exact_grid_unstaged(store):
    """FHE_NTT_ROW_SHFL=31 FHE_NTT_FULL=255 FHE_NTT_TWL=0: <M, true, false, *> and the ragged <M, false, false, *>"""
    run_child('dpp-full-notwl', store)


def test_dpp_rows_checked_staged(store):
    """FHE_NTT_ROW_SHFL=31 FHE_NTT_FULL=0 FHE_NTT_TWL_ROWS=16: <M, false, true, *>"""
    run_child('dpp-checked-twl', store)


def test_dpp_rows_checked_unstaged(store):
    """FHE_NTT_ROW_SHFL=31 FHE_NTT_FULL=0 FHE_NTT_TWL=0: <M, false, false, *>"""
    run_child('dpp-checked-notwl', store)


def test_launch_shapes(store):
    """FHE_KS_FUSE_MIN=1 (k_ntt_row_ks<.., false> with 1, 2 and 3 members: lmb = 2, a partial block of four;
    products at level 0 and at ell = alpha; the rotations of those stacks, whose key switch does not fuse),
    FHE_KS_MC=4 (k_ks_inner_mc<3, 4> for eight members at ring 2^12), FHE_CONV_CHUNK=5 (ModUp's 10, 7 and 6
    targets and the products' conversions in chunks of five), FHE_PS_XCD=0 (k_mul_plain_sum on the plain grid),
    and a degree-70 Chebyshev series under all four"""
    run_child('shapes', store)


def test_aux_stream(store):
    """FHE_NTT_AUX=1 in the 40-bit context, outside the kernel clock: q_0's launch of every pass on the second
    stream, forked from and joined into the engine's by events (the condition is in the module docstring)"""
    run_child('aux', store)


def test_every_row_form_ran(store):
    """The union of the children's clocks holds every (family, MODE, FULL, TWL, FP) of the 256-point row pass:

      k_ntt_fwd_row<M, FULL, TWL, FP>         M in 0, 2, 3, 4, 5: 40 forms
      k_ntt_inv_row<FULL, TWL, FP>                                  8 forms
      k_ntt_fwd<8, 4, false, M, FULL, FP>     M in 0, 2, 3, 4, 5: 20 forms
      k_ntt_inv<8, 4, false, FULL, FP>                              4 forms

    MODE 1 is the rescale's lifted column pass and has no row form.  launch_pass_one can reach every one of the
    72: none is excluded.  The one its stated stacks miss is MODE 5 with FULL = true on the DPP kernels: the
    one-digit closing row runs only where the key switch fuses (Engine ks_fuse: four members and up), and
    `full` there needs segs % 2^lsegb == 0, which five members (ten segments, blocks of eight) do not give;
    the 4-member stack of the products is there for it."""
    for mode in CHILDREN:
        if mode not in FORMS:  # this test alone: run the children it reads
            run_child(mode, store)
    seen = set().union(*FORMS.values())
    both = (False, True)
    want = {('fwd_row', m, full, twl, fp) for m in (0, 2, 3, 4, 5) for full in both for twl in both for fp in both}
    want |= {('inv_row', full, twl, fp) for full in both for twl in both for fp in both}
    want |= {('fwd', 8, False, m, full, fp) for m in (0, 2, 3, 4, 5) for full in both for fp in both}
    want |= {('inv', 8, False, full, fp) for full in both for fp in both}
    assert len(want) == 72
    assert not want - seen, sorted(want - seen, key=str)
