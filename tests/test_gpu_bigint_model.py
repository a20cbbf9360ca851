"""The GPU engine against the exact big-integer model (tests/bigint_model.py).

Every other GPU test compares the engine with the CPU oracle, which was
written from the same specification; here the engine's words are compared
with Python-integer arithmetic that shares no code with either.  The oracle
only supplies the keys (load_keys_from) and, in the tie test, its choice of
candidate -- word parity at a true ModDown tie is the contract's hardest case.
Its results are consulted nowhere else.

  * ring 2^12, L = 5, 40- and 41-bit scaling (the latter interleaves the fp64
    and the integer prime classes): NTT, ModUp, ModDown, rescale, mul, square,
    rotations, conjugate, mul_plain on random inputs with zero ModDown ties
    asserted first; the boundary inputs of the rescale (through rescale and
    through mul's fused ModDown + rescale kernel), of ModDown (exact cases
    and true ties) and of ModRaise; the exact noise bounds;
  * 59-bit scaling (every limb integer class); L = 12 (alpha = 5) at two
    levels; the wide-digit contexts' noise bound;
  * ring 2^16 in one child process: stacked products at ell = 2 and 3 through
    the one-digit fused row passes (kernel names asserted), with the rescale
    boundary input as one member, and a rotation.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import bigint_model as M
import fhesort as F
import pyoracle as O

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
ROTS = [1, -3]


def make(logN, L, bits, seed, rots=ROTS, conj=True):
    orc = O.Context(logN, L, bits, 60, 3, seed=seed)
    orc.gen_rotation_keys(rots)
    gpu = F.Context(logN, L, bits, 60, 3, seed=seed, keygen=False)
    gpu.load_keys_from(orc, rots)
    if conj:
        orc.gen_galois_keys([2 * orc.n - 1])
        gpu.load_galois_keys_from(orc, [2 * orc.n - 1])
    assert np.array_equal(orc.primes, gpu.primes)
    return orc, gpu, M.Model(logN, gpu.primes, gpu.nq, gpu.K, gpu.alpha, gpu.ntt)


@pytest.fixture(scope='module', params=[40, 41], ids=['scale40', 'scale41'])
def trio(request):
    return make(12, 5, request.param, 7 if request.param == 40 else 41)


@pytest.fixture(scope='module')
def trio59():
    return make(12, 5, 59, 12, conj=False)


@pytest.fixture(scope='module')
def trio12():
    return make(12, 12, 40, 5, rots=[1], conj=False)


def no_ties(ties):
    assert len(ties) == 0, f'{len(ties)} ModDown ties on random input'


def fused_tail_ran(stats):
    assert any(k.startswith('k_moddown_rescale') for k in stats), sorted(stats)


def gpu_mul(gpu, a, b, level):
    """the engine's product of two uploaded ciphertexts; the fused ModDown +
    rescale kernel must be what ran"""
    ga, gb = gpu.upload(a, level, 8), gpu.upload(b, level, 8)
    with F.KernelClock(gpu) as clk:
        out = gpu.mul(ga, gb)
    fused_tail_ran(clk.stats)
    return out.data()


def check_ntt(gpu, m):
    rng = np.random.default_rng(1)
    for i, q in enumerate(m.q):
        x = rng.integers(0, q, size=m.n, dtype=np.uint64)
        assert np.array_equal(M.u64(m.fwd(i, x)), gpu.ntt(i, x)), f'forward, prime {i}'
        assert np.array_equal(M.u64(m.inv(i, x)), gpu.ntt(i, x, inverse=True)), f'inverse, prime {i}'


def check_conversions(gpu, m, up, down):
    rng = np.random.default_rng(2)
    for ell in up:
        d = M.rand_limbs(rng, m.q[:ell], m.n)
        assert np.array_equal(m.modup(d), gpu.modup(d)), f'modup, ell={ell}'
    m.closest = 1.0
    for ell in down:
        x = M.rand_limbs(rng, m.q[:ell] + m.q[m.nq:], m.n)
        want, ties = m.moddown(x)
        no_ties(ties)
        assert np.array_equal(want, gpu.moddown(x)), f'moddown, ell={ell}'
    print(f'closest |2 X_P - P| / P on random input: {m.closest:.3e}; tau = {M.tau_num(m.K) / 2 ** 53:.3e}')


def check_mul_rotate(orc, gpu, m, level, seed, noise=False):
    """one product and one rotation of real encryptions at `level`"""
    rng = np.random.default_rng(seed)
    oa, ob = orc.encrypt(rng.uniform(-1, 1, 8), 8, level), orc.encrypt(rng.uniform(-1, 1, 8), 8, level)
    a, b = oa.data(), ob.data()
    want, ties = m.mul(a, b, orc.relin_key())
    no_ties(ties)
    prod = gpu_mul(gpu, a, b, level)
    assert np.array_equal(want, prod), f'mul, level {level}'
    want, ties = m.rotate(a, 1, orc.rot_key(1)[1])
    no_ties(ties)
    rot = gpu.rotate(gpu.upload(a, level, 8), 1).data()
    assert np.array_equal(want, rot), f'rotate, level {level}'
    if noise:
        s = orc.secret_coeff()
        got, bound = M.check_rotate_noise(m, a, rot, M.galois_of_rotation(m.logN, 1), s)
        print(f'rotation noise 2^{got:.1f}, bound 2^{bound:.1f}')
        got, bound = M.check_mul_noise(m, a, b, prod, s)
        print(f'product noise 2^{got:.1f}, bound 2^{bound:.1f}')


# ------------------------------------------- ring 2^12, L = 5, 40 / 41 bits --
def test_prime_classes(trio):
    _, gpu, m = trio
    fp = [q < (1 << 41) for q in m.q[:m.nq]]
    runs = 1 + sum(x != y for x, y in zip(fp, fp[1:]))
    if max(m.q[1:m.nq]) >= (1 << 41):
        # the 41-bit context: scaling primes of both classes, the fp64 ones between integer ones
        assert any(fp[1:]) and not all(fp[1:]) and runs >= 3, fp
    else:
        assert not fp[0] and all(fp[1:]), fp


def test_ntt_every_prime(trio):
    _, gpu, m = trio
    check_ntt(gpu, m)


def test_conversions(trio):
    _, gpu, m = trio
    check_conversions(gpu, m, sorted({m.nq, m.nq - 1, m.alpha + 1, m.alpha, 1}, reverse=True), (m.nq, 2, 1))


def test_rescale(trio):
    _, gpu, m = trio
    rng = np.random.default_rng(4)
    for ell in (m.nq, 2):
        data = np.stack([M.rand_limbs(rng, m.q[:ell], m.n) for _ in range(2)])
        got = gpu.rescale(gpu.upload(data, m.nq - ell, 8)).data()
        assert np.array_equal(m.rescale(data), got), f'ell={ell}'


def test_ops(trio):
    orc, gpu, m = trio
    rng = np.random.default_rng(5)
    va, vb = rng.uniform(-1, 1, 8), rng.uniform(-1, 1, 8)
    oa, ob = orc.encrypt(va, 8), orc.encrypt(vb, 8)
    a, b, relin = oa.data(), ob.data(), orc.relin_key()
    ga = gpu.upload(a, 0, 8)
    m.closest = 1.0
    with F.KernelClock(gpu) as clk:
        sq = gpu.square(ga)
    fused_tail_ran(clk.stats)
    for what, (want, ties), got in [
        ('mul', m.mul(a, b, relin), gpu_mul(gpu, a, b, 0)),
        ('square', m.square(a, relin), sq.data()),
        ('rotate 1', m.rotate(a, 1, orc.rot_key(1)[1]), gpu.rotate(ga, 1).data()),
        ('rotate -3', m.rotate(a, -3, orc.rot_key(-3)[1]), gpu.rotate(ga, -3).data()),
        ('conjugate', m.conjugate(a, orc.galois_key(2 * m.n - 1)), gpu.conjugate(ga).data()),
    ]:
        no_ties(ties)
        assert np.array_equal(want, got), what
    for (want, ties), got in zip(m.rotate_hoisted(a, ROTS, [orc.rot_key(k)[1] for k in ROTS]),
                                 gpu.rotate_hoisted(ga, ROTS)):
        no_ties(ties)
        assert np.array_equal(want, got.data()), 'hoisted'
    p = orc.encode(vb, 8, 0).data()
    assert np.array_equal(m.mul_plain(a, p), gpu.mul_plain(ga, gpu.upload_pt(p, 0, 8)).data()), 'mul_plain + rescale'
    print(f'closest |2 X_P - P| / P in the ops: {m.closest:.3e}; tau = {M.tau_num(m.K) / 2 ** 53:.3e}')


def test_rescale_boundary(trio):
    """the last limb's coefficients at 0, 1, (q_l - 1)/2, (q_l + 1)/2, q_l - 1:
    exact, through rescale and through mul's fused ModDown + rescale kernel
    (operands built so that the product's pre-rescale last limb is that limb)"""
    orc, gpu, m = trio
    rng = np.random.default_rng(6)
    for ell in (m.nq, 2):
        level = m.nq - ell
        data = M.rescale_boundary_ct(m, rng, ell)
        assert np.array_equal(m.rescale(data), gpu.rescale(gpu.upload(data, level, 8)).data()), f'rescale, ell={ell}'
        a, b, ks = M.mul_boundary_operands(m, rng, ell, orc.relin_key())
        no_ties(ks[1])
        want, _ = m.mul(a, b, None, ks=ks)
        assert np.array_equal(want, gpu_mul(gpu, a, b, level)), f'mul, ell={ell}'


def test_moddown_boundary_exact(trio):
    """X_P = floor(P (1/2 -+ 2^-30)), floor(P (1/2 -+ 2^-45)), 0, 1, P - 1: the
    sign boundary of the centred conversion, all far outside tau: exact"""
    _, gpu, m = trio
    rng = np.random.default_rng(7)
    assert 2.0 ** -44 > 4 * M.tau_num(m.K) / 2 ** 53
    XP = M.blocks(M.moddown_exact_values(m.P), m.n)
    for ell in (m.nq, 2):
        x = M.moddown_input(m, rng, ell, XP)
        want, ties = m.moddown(x)
        no_ties(ties)
        assert np.array_equal(want, gpu.moddown(x)), f'ell={ell}'


def test_moddown_boundary_ties(trio):
    """X_P = (P - 1)/2 and (P + 1)/2 at known coefficients: there, and only
    there, either candidate is accepted -- and the engine picks the oracle's"""
    orc, gpu, m = trio
    rng = np.random.default_rng(8)
    for ell in (m.nq, 2):
        x, idx = M.moddown_tie_input(m, rng, ell)
        got = gpu.moddown(x)
        M.check_moddown_ties(m, x, got, idx)
        assert np.array_equal(got, orc.moddown(x)), f'ell={ell}: engine and oracle pick different tie candidates'


def test_noise_bounds(trio):
    orc, gpu, m = trio
    check_mul_rotate(orc, gpu, m, 0, 9, noise=True)


def test_mod_raise_boundary():
    """bootstrap stage 4 is the bare centred lift (Engine::mod_raise ->
    ew_lift_centered): pinned at 0, 1, (q_0 - 1)/2, (q_0 + 1)/2, q_0 - 1"""
    gpu = F.Context(11, 24, 59, 60, 3, seed=61, keygen=False)
    m = M.Model(11, gpu.primes, gpu.nq, gpu.K, gpu.alpha, gpu.ntt)
    B = F.Bootstrapper(gpu, 8, (2, 2), keygen=False)
    vals = M.lift_boundary_values(m.q[0])
    data = np.stack([M.u64(m.fwd(0, M.blocks(vals, m.n))), M.u64(m.fwd(0, M.blocks(vals[::-1], m.n, 7)))])[:, None, :]
    got = B.mod_raise(gpu.upload(data, gpu.L, 8))
    assert got.info()['limbs'] == m.nq
    assert np.array_equal(m.mod_raise(data), got.data())


# --------------------------------------------- 59 bits; L = 12; wide digits --
def test_scale59(trio59):
    orc, gpu, m = trio59
    assert all(q >= (1 << 41) for q in m.q)  # every limb integer class
    check_ntt(gpu, m)
    check_conversions(gpu, m, sorted({m.nq, m.nq - 1, m.alpha + 1, m.alpha, 1}, reverse=True), (m.nq, 2, 1))
    check_mul_rotate(orc, gpu, m, 0, 59)


@pytest.mark.parametrize('ell', [13, 6])
def test_depth12_levels(trio12, ell):
    """alpha = 5: three digits at level 0, two (ell = alpha + 1, a one-prime last digit) at level 7"""
    orc, gpu, m = trio12
    assert m.alpha == 5 and m.nq == 13
    check_mul_rotate(orc, gpu, m, m.nq - ell, ell)


@pytest.mark.parametrize('L,alpha,K', [(65, 22, 16), (61, 21, 15), (50, 17, 12)])
def test_wide_digits_rotation(L, alpha, K):
    """the contexts of test_wide_digits_match_oracle at its ring: one rotation,
    word for word and within the noise bound"""
    orc, gpu, m = make(12, L, 40, L, rots=[1], conj=False)
    assert (m.alpha, m.K) == (alpha, K)
    a = orc.encrypt(np.random.default_rng(L).uniform(-1, 1, 16), 16).data()
    got = gpu.rotate(gpu.upload(a, 0, 16), 1).data()
    want, ties = m.rotate(a, 1, orc.rot_key(1)[1])
    no_ties(ties)
    assert np.array_equal(want, got)
    noise, bound = M.check_rotate_noise(m, a, got, M.galois_of_rotation(12, 1), orc.secret_coeff())
    print(f'L={L}: rotation noise 2^{noise:.1f}, bound 2^{bound:.1f}')
    gpu.close()


# ------------------------------------------------ ring 2^16, one child process --
LOGN16, L16, SEED16 = 16, 12, 28

CHILD = r'''
import sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import fhesort as F
import pyoracle as O
logn, L, seed = (int(v) for v in sys.argv[5:8])
inp = np.load(sys.argv[3])
orc = O.Context(logn, L, 40, 60, 3, seed=seed)
orc.gen_rotation_keys([1])
gpu = F.Context(logn, L, 40, 60, 3, seed=seed, keygen=False)
gpu.load_keys_from(orc, [1])
out = {'primes': gpu.primes}
X = np.zeros(gpu.n, dtype=np.uint64)
X[1] = 1
out['psi'] = np.array([gpu.ntt(i, X)[0] for i in range(gpu.nq + gpu.K)], dtype=np.uint64)
for ell in (2, 3):
    level = gpu.nq - ell
    A, B = inp[f'a{ell}'], inp[f'b{ell}']
    ga = gpu.stack([gpu.upload(x, level, 8) for x in A])
    gb = gpu.stack([gpu.upload(x, level, 8) for x in B])
    with F.KernelClock(gpu) as clk:
        st = gpu.mul(ga, gb)
    out[f'mul{ell}'] = np.stack([gpu.member(st, i).data() for i in range(len(A))])
    out[f'names{ell}'] = np.array(sorted(clk.stats))
out['rot'] = gpu.rotate(gpu.upload(inp['a3'][0], gpu.nq - 3, 8), 1).data()
np.savez(sys.argv[4], **out)
print('ALLOK')
'''


@pytest.fixture(scope='module')
def ring16(tmp_path_factory):
    """Inputs built here by the model, one child process runs them on the engine.
    Stacks of four at ell = 2 and 3: member 0 random, member 3 the rescale
    boundary operands, members 1 and 2 those two with the operands exchanged (a
    product is symmetric, so the model's words serve both)."""
    orc = O.Context(LOGN16, L16, 40, 60, 3, seed=SEED16)
    orc.gen_rotation_keys([1])
    m = M.Model(LOGN16, orc.primes, orc.nq, orc.K, orc.alpha, orc.ntt)
    rng = np.random.default_rng(16)
    relin = orc.relin_key()
    inp, ks = {}, {}
    for ell in (2, 3):
        r = [np.stack([M.rand_limbs(rng, m.q[:ell], m.n) for _ in range(2)]) for _ in range(2)]
        a, b, ks[ell] = M.mul_boundary_operands(m, rng, ell, relin)
        inp[f'a{ell}'] = np.stack([r[0], r[1], b, a])
        inp[f'b{ell}'] = np.stack([r[1], r[0], a, b])
    d = tmp_path_factory.mktemp('ring16')
    fin, fout = str(d / 'in.npz'), str(d / 'out.npz')
    np.savez(fin, **inp)
    r = subprocess.run([sys.executable, '-c', CHILD, os.path.join(REPO, 'fhe-sorting_amd'), os.path.join(REPO, 'oracle'),
                        fin, fout, str(LOGN16), str(L16), str(SEED16)], capture_output=True, text=True, timeout=280)
    assert r.returncode == 0 and 'ALLOK' in r.stdout, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
    out = np.load(fout)
    # the model above took psi from the oracle's transform to build its inputs: it is
    # the model of the engine's transform if and only if the engine's roots are the same
    assert np.array_equal(out['primes'], orc.primes)
    assert [int(v) for v in out['psi']] == m.psi
    return orc, m, inp, ks, out


@pytest.mark.parametrize('ell', [2, 3])
def test_ring16_products(ring16, ell):
    """one-digit products (ell <= alpha) of a stack of four through the fused row
    passes that exist only at rings 2^16 and 2^17"""
    orc, m, inp, ks, out = ring16
    names = [str(k) for k in out[f'names{ell}']]
    assert any(k.startswith('k_ntt_fwd_row<5,') for k in names), names
    assert any(k.startswith('k_ntt_row_ks<') for k in names), names
    fused_tail_ran(names)
    got = out[f'mul{ell}']
    A, B = inp[f'a{ell}'], inp[f'b{ell}']
    want, ties = m.mul(A[0], B[0], orc.relin_key())
    no_ties(ties)
    assert np.array_equal(want, got[0]), 'member 0'
    assert np.array_equal(want, got[1]), 'member 1 (operands exchanged)'
    no_ties(ks[ell][1])
    want, _ = m.mul(A[3], B[3], None, ks=ks[ell])
    assert np.array_equal(want, got[3]), 'member 3 (rescale boundary)'
    assert np.array_equal(want, got[2]), 'member 2 (rescale boundary, operands exchanged)'


def test_ring16_rotation(ring16):
    orc, m, inp, ks, out = ring16
    a = inp['a3'][0]
    want, ties = m.rotate(a, 1, orc.rot_key(1)[1])
    no_ties(ties)
    assert np.array_equal(want, out['rot'])
    noise, bound = M.check_rotate_noise(m, a, out['rot'], M.galois_of_rotation(LOGN16, 1), orc.secret_coeff())
    print(f'ring 2^16 ell=3: rotation noise 2^{noise:.1f}, bound 2^{bound:.1f}')
