"""GPU: seeded switching keys (wire kinds 7 and 8, public stream v1:
csrc/wire/wire.hpp).  The expansion kernel against the numpy restatement of the
documented stream (tests/wire_seeded_spec.py) word for word; keys generated
under a public seed are keys and carry the stream in their a halves; full and
seeded files load to the same words and re-serialise byte for byte; everything a
seeded file can get wrong is refused; without a public seed nothing changes;
and the CLI sorts from seeded key files to the same words as from full ones.

The contexts: ring 2^12, depth 6, 40-bit scaling -- its chain holds scaling
primes on both sides of 2^40 (41-bit candidates, about half rejected, and 40-bit
ones, almost none), a 60-bit q_0 and three special primes -- and ring 2^13 with
dnum = 2, where nall, the digit count and n/8 all differ."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fhesort as F
import wire_spec as W
import wire_seeded_spec as S

pytestmark = pytest.mark.gpu

PKG = os.path.dirname(os.path.abspath(F.__file__))
CLI = os.path.join(PKG, 'bin', 'fhesort')
CLIENT = os.path.join(PKG, 'client.py')
ROTS = [1, 2, -1, 5]
LOGN, DEPTH = 12, 6
TEST_SEED = 0x5eed0123456789ab  # the context's test seed: its 8 bytes must reach no seeded file
PUB = bytes((37 * i + 11) & 0xff for i in range(32))
PUB2 = bytes((91 * i + 5) & 0xff for i in range(32))


def galois(k, n):
    return pow(5, k, 2 * n)


def _seeded_ctx(seed=TEST_SEED, pub=PUB, rots=ROTS):
    ctx = F.Context(LOGN, DEPTH, 40, 60, 3, seed=seed, keygen=False)
    ctx.set_public_seed(pub)
    ctx.keygen()
    ctx.gen_rotation_keys(rots)
    return ctx


def _save(ctx, d, seeded):
    d.mkdir(exist_ok=True)
    paths = {k: str(d / f'{k}.bin') for k in ('cc', 'pub', 'mult', 'rot', 'sec')}
    ctx.serialize(paths['cc'])
    ctx.serialize_public_key(paths['pub'])
    ctx.serialize_secret_key(paths['sec'])
    if seeded:
        ctx.serialize_eval_mult_key_seeded(paths['mult'])
        ctx.serialize_eval_automorphism_key_seeded(paths['rot'])
    else:
        ctx.serialize_eval_mult_key(paths['mult'])
        ctx.serialize_eval_automorphism_key(paths['rot'])
    return paths


def _load(paths):
    c = F.Context.deserialize(paths['cc'])
    c.deserialize_public_key(paths['pub'])
    c.deserialize_eval_mult_key(paths['mult'])
    n = c.deserialize_eval_automorphism_key(paths['rot'])
    c.deserialize_secret_key(paths['sec'])
    return c, n


def _body(path):
    """body words of a wire file the library wrote (its checksum is the library's)"""
    w = np.fromfile(path, dtype=np.uint64)
    assert int(w[0]) == W.MAGIC and len(w) == 8 + int(w[6]) + 1
    return w[8:-1]


def _full_keys(paths, ctx):
    """{kid: [digits][2][nall][n]} from the full-format files (kinds 3 and 4)"""
    nall, kw = ctx.nq + ctx.K, ctx.digits * 2 * (ctx.nq + ctx.K) * ctx.n
    b = _body(paths['mult'])
    assert int(b[0]) == ctx.digits and len(b) == 1 + kw
    keys = {0: S.full_switch_key(b[1:], ctx.digits, nall, ctx.n)}
    b = _body(paths['rot'])
    assert int(b[0]) == ctx.digits and len(b) == 2 + int(b[1]) * (1 + kw)
    for i in range(int(b[1])):
        o = 2 + i * (1 + kw)
        keys[int(b[o])] = S.full_switch_key(b[o + 1:o + 1 + kw], ctx.digits, nall, ctx.n)
    return keys


@pytest.fixture(scope='module')
def world(tmp_path_factory):
    """A: generated under a public seed; its full and seeded files."""
    d = tmp_path_factory.mktemp('seeded')
    a = _seeded_ctx()
    full, seeded = _save(a, d / 'full', False), _save(a, d / 'seeded', True)
    yield a, full, seeded
    a.close()


# ------------------------------------------------------------ 1 stream parity
@pytest.mark.parametrize('log_n,depth,dnum', [(12, 6, 3), (13, 6, 2)])
def test_expansion_kernel_equals_the_documented_stream(log_n, depth, dnum):
    ctx = F.Context(log_n, depth, 40, 60, dnum, seed=3, keygen=False)
    try:
        n = ctx.n
        bits = [int(q).bit_length() for q in ctx.primes]
        q_scale = [int(q) for q in ctx.primes[1:ctx.nq]]
        # both rejection regimes, the 60-bit q_0 and the special primes
        assert bits[0] == 60 and all(b == 60 for b in bits[ctx.nq:]) and ctx.K >= 3
        assert any(q > 2 ** 40 for q in q_scale) and any(q < 2 ** 40 for q in q_scale)
        assert ctx.digits == dnum and n // 8 == (512 if log_n == 12 else 1024)
        for kid in (0, galois(1, n), galois(-1, n), 2 * n - 1):
            for digit in (0, ctx.digits - 1):
                got = ctx.public_poly(PUB, kid, digit)
                want = S.public_poly(PUB, kid, digit, ctx.primes, n)
                assert got.shape == want.shape == (ctx.nq + ctx.K, n)
                assert np.array_equal(got, want), (kid, digit, np.argwhere(got != want)[:4])
                assert (got < ctx.primes[:, None]).all()
        # another seed gives another stream
        assert not np.array_equal(ctx.public_poly(PUB2, 0, 0)[0], ctx.public_poly(PUB, 0, 0)[0])
    finally:
        ctx.close()


# ---------------------------------------------------------- 2 keys are keys
def test_seeded_keygen_gives_working_keys_on_the_stream(world):
    a, full, _ = world
    n = a.n
    gs = [galois(k, n) for k in ROTS]
    assert a.get_public_seed() == PUB
    assert a.key_is_seeded(0) == 1
    for g in gs:
        assert a.key_is_seeded(g) == 1
    with pytest.raises(F.FheError):
        a.key_is_seeded(galois(3, n))  # no such key
    keys = _full_keys(full, a)
    assert sorted(keys) == sorted([0] + gs)
    for kid, key in keys.items():
        for j in range(a.digits):
            assert np.array_equal(key[j, 1], S.public_poly(PUB, kid, j, a.primes, n)), (kid, j)
    # b = -a s + e + P s' was formed with the expanded a: the keys switch keys
    v = np.linspace(-0.5, 0.5, 64)
    x = a.encrypt(v, 64)
    for k in ROTS:
        assert np.abs(a.decrypt(a.rotate(x, k))[:64] - np.roll(v, -k)).max() < 1e-6, k
    assert np.abs(a.decrypt(a.mul(x, x))[:64] - v * v).max() < 1e-6


# ------------------------------------------------------------- 3 round trip
def test_full_and_seeded_files_load_to_the_same_keys(world, tmp_path):
    a, full, seeded = world
    n, nall = a.n, a.nq + a.K
    bw = a.digits * nall * n
    i7, i8 = F.wire_inspect(seeded['mult']), F.wire_inspect(seeded['rot'])
    assert i7['kind'] == 'eval_mult_key_seeded' and i7['body_words'] == 6 + bw
    assert i8['kind'] == 'eval_automorphism_key_seeded' and i8['body_words'] == 6 + len(ROTS) * (1 + bw)
    assert os.path.getsize(seeded['mult']) == (8 + 6 + bw + 1) * 8
    # the restated parser reads them: the b halves of the full files, and the seed
    keys = _full_keys(full, a)
    h, seed, b = S.eval_mult(open(seeded['mult'], 'rb').read())
    assert seed == PUB and np.array_equal(b, keys[0][:, 0])
    assert h['params_id'] == F.wire_inspect(full['mult'])['params_id']
    h, seed, bs = S.automorphism(open(seeded['rot'], 'rb').read(), a.digits)
    assert seed == PUB and sorted(bs) == sorted(k for k in keys if k)
    for g, b in bs.items():
        assert np.array_equal(b, keys[g][:, 0]), g
    bctx, nb = _load(full)
    cctx, nc = _load(seeded)
    try:
        assert nb == nc == len(ROTS)
        assert bctx.key_is_seeded(0) == 0 and cctx.key_is_seeded(0) == 1
        for k in ROTS:
            assert bctx.key_is_seeded(galois(k, n)) == 0 and cctx.key_is_seeded(galois(k, n)) == 1
        v = np.linspace(-0.5, 0.5, 64)
        x = a.encrypt(v, 64)
        ct = str(tmp_path / 'x.bin')
        a.serialize_ciphertext(x, ct)
        xb, xc = bctx.deserialize_ciphertext(ct), cctx.deserialize_ciphertext(ct)
        for k in ROTS:
            want = a.rotate(x, k).data()
            assert np.array_equal(bctx.rotate(xb, k).data(), want), k
            assert np.array_equal(cctx.rotate(xc, k).data(), want), k
        want = a.mul(x, x).data()
        assert np.array_equal(bctx.mul(xb, xb).data(), want)
        assert np.array_equal(cctx.mul(xc, xc).data(), want)
        # C re-serialises both formats byte for byte
        for fmt, ref in ((False, full), (True, seeded)):
            again = _save(cctx, tmp_path / f'again{int(fmt)}', fmt)
            for k in ('mult', 'rot'):
                assert open(again[k], 'rb').read() == open(ref[k], 'rb').read(), (fmt, k)
    finally:
        bctx.close()
        cctx.close()


def test_bootstrapping_keys_round_trip_seeded(tmp_path):
    a = F.Context(11, 24, 59, 60, 3, seed=61, keygen=False)
    a.set_public_seed(PUB2)
    a.keygen()
    B = F.Bootstrapper(a, 8, (2, 1))  # fhe_boot_keygen: the transforms' rotations and the conjugation key
    c1 = c2 = None
    try:
        n = a.n
        conj = 2 * n - 1
        rots = [r for r in B.rotations() if r % (n // 2)]
        assert rots and a.key_is_seeded(conj) == 1
        assert all(a.key_is_seeded(galois(r, n)) == 1 for r in rots)
        full, seeded = _save(a, tmp_path / 'full', False), _save(a, tmp_path / 'seeded', True)
        assert os.path.getsize(seeded['rot']) < 0.51 * os.path.getsize(full['rot'])
        c1, n1 = _load(full)
        c2, n2 = _load(seeded)
        assert n1 == n2 and c2.key_is_seeded(conj) == 1 and c1.key_is_seeded(conj) == 0
        x = a.encrypt(np.linspace(-0.5, 0.5, 8), 8, level=20)
        ct = str(tmp_path / 'x.bin')
        a.serialize_ciphertext(x, ct)
        x1, x2 = c1.deserialize_ciphertext(ct), c2.deserialize_ciphertext(ct)
        want = a.conjugate(x).data()
        assert np.array_equal(c1.conjugate(x1).data(), want) and np.array_equal(c2.conjugate(x2).data(), want)
        for r in rots:
            want = a.rotate(x, r).data()
            assert np.array_equal(c1.rotate(x1, r).data(), want), r
            assert np.array_equal(c2.rotate(x2, r).data(), want), r
        for fmt, ref in ((False, full), (True, seeded)):
            again = _save(c2, tmp_path / f'again{int(fmt)}', fmt)
            for k in ('mult', 'rot'):
                assert open(again[k], 'rb').read() == open(ref[k], 'rb').read(), (fmt, k)
    finally:
        for c in (c1, c2, a):
            if c is not None:
                c.close()


# --------------------------------------------------------------- 4 refusals
def _einval(fn, *args):
    with pytest.raises(F.FheError) as e:
        fn(*args)
    assert e.value.code == F.FHE_EINVAL, str(e.value)
    return str(e.value)


def test_seeded_serialisation_needs_seeded_keys(world, tmp_path):
    a, full, _ = world
    out = str(tmp_path / 'o.bin')
    # a context without a public seed
    plain = F.Context(LOGN, DEPTH, 40, 60, 3, seed=5)
    plain.gen_rotation_keys([1])
    try:
        with pytest.raises(F.FheError) as e:
            plain.get_public_seed()
        assert e.value.code == F.FHE_EINVAL
        assert 'eval-mult key' in _einval(plain.serialize_eval_mult_key_seeded, out)
        assert f'galois element {galois(1, plain.n)}' in _einval(plain.serialize_eval_automorphism_key_seeded, out)
        # NULL asks for an OS-drawn seed: refused on a context with a test seed
        _einval(plain.set_public_seed, None)
        # one rotation key from before the seed
        plain.set_public_seed(PUB)
        plain.gen_rotation_keys([2])
        assert plain.key_is_seeded(galois(2, plain.n)) == 1 and plain.key_is_seeded(galois(1, plain.n)) == 0
        assert f'galois element {galois(1, plain.n)}' in _einval(plain.serialize_eval_automorphism_key_seeded, out)
        # two seeds in one key set
        plain.keygen()
        plain.serialize_eval_mult_key_seeded(out)
        other = F.Context(LOGN, DEPTH, 40, 60, 3, seed=5, keygen=False)
        try:
            other.set_public_seed(PUB)
            other.keygen()
            other.gen_rotation_keys([1])
            other.set_public_seed(PUB2)
            other.gen_rotation_keys([2])
            assert 'seed' in _einval(other.serialize_eval_automorphism_key_seeded, out)
        finally:
            other.close()
    finally:
        plain.close()
    # keys loaded from full files are not seeded, whatever the context's seed
    b, _ = _load(full)
    try:
        b.set_public_seed(PUB)
        _einval(b.serialize_eval_mult_key_seeded, out)
        _einval(b.serialize_eval_automorphism_key_seeded, out)
    finally:
        b.close()
    assert not os.path.exists(out) or F.wire_inspect(out)['kind'] == 'eval_mult_key_seeded'
    # a secure context draws its own seed
    sec = F.Context(LOGN, DEPTH, 40, 60, 3, keygen=False)
    try:
        sec.set_public_seed(None)
        s1 = sec.get_public_seed()
        sec.set_public_seed(None)
        assert len(s1) == 32 and s1 != sec.get_public_seed()
    finally:
        sec.close()


def test_bad_seeded_files_are_refused_and_change_nothing(world, tmp_path):
    a, _, seeded = world
    n = a.n
    x = a.encrypt(np.linspace(0, 1, 32), 32)
    before = {k: a.rotate(x, k).data() for k in ROTS}
    mul_before = a.mul(x, x).data()
    # another modulus chain
    other = F.Context(LOGN, DEPTH + 1, 40, 60, 3, seed=12, keygen=False)
    try:
        _einval(other.deserialize_eval_mult_key, seeded['mult'])
        _einval(other.deserialize_eval_automorphism_key, seeded['rot'])
    finally:
        other.close()
    h7, seed, b7 = S.eval_mult(open(seeded['mult'], 'rb').read())
    h8, _, b8 = S.automorphism(open(seeded['rot'], 'rb').read(), a.digits)
    keys8 = sorted(b8.items())
    hdr = lambda h: (h['params_id'], h['log_n'], h['nq'], h['K'])
    p = tmp_path / 'f.bin'
    # the restated writer's files are the engine's, byte for byte, and load
    assert S.pack_eval_mult(*hdr(h7), seed, b7) == open(seeded['mult'], 'rb').read()
    assert S.pack_automorphism(*hdr(h8), seed, keys8) == open(seeded['rot'], 'rb').read()
    # stream version 2, valid checksum
    p.write_bytes(S.pack_eval_mult(*hdr(h7), seed, b7, version=2))
    assert 'version' in _einval(a.deserialize_eval_mult_key, str(p))
    p.write_bytes(S.pack_automorphism(*hdr(h8), seed, keys8, version=2))
    assert 'version' in _einval(a.deserialize_eval_automorphism_key, str(p))
    # a residue >= q with a valid checksum: in the last key, so the earlier ones
    # must not have been installed either
    bad = b7.copy()
    bad[a.digits - 1, 1, 7] = a.primes[1]
    p.write_bytes(S.pack_eval_mult(*hdr(h7), seed, bad))
    assert 'out of range' in _einval(a.deserialize_eval_mult_key, str(p))
    forged = [(g, b.copy()) for g, b in keys8]
    forged[0] = (forged[0][0], forged[0][1] + np.uint64(1))  # a different first key, in range
    forged[-1][1][0, a.nq + a.K - 1, n - 1] = a.primes[-1]
    p.write_bytes(S.pack_automorphism(*hdr(h8), seed, forged))
    assert 'out of range' in _einval(a.deserialize_eval_automorphism_key, str(p))
    # an even galois element
    forged = [(g, b) for g, b in keys8]
    forged[1] = (forged[1][0] + 1, forged[1][1])
    p.write_bytes(S.pack_automorphism(*hdr(h8), seed, forged))
    _einval(a.deserialize_eval_automorphism_key, str(p))
    # a digit count that is not the context's
    p.write_bytes(S.pack_eval_mult(*hdr(h7), seed, b7[:2]))
    _einval(a.deserialize_eval_mult_key, str(p))
    # a flipped byte
    for k, load in (('mult', a.deserialize_eval_mult_key), ('rot', a.deserialize_eval_automorphism_key)):
        raw = bytearray(open(seeded[k], 'rb').read())
        raw[len(raw) // 2] ^= 0x10
        p.write_bytes(bytes(raw))
        with pytest.raises(F.FheError) as e:
            load(str(p))
        assert e.value.code == F.FHE_EIO
    # the context rotates and multiplies as before, its keys still seeded
    for k in ROTS:
        assert np.array_equal(a.rotate(x, k).data(), before[k]), k
        assert a.key_is_seeded(galois(k, n)) == 1
    assert np.array_equal(a.mul(x, x).data(), mul_before)
    # nothing of the test seed reaches a seeded file (megabytes of uniform words:
    # a coincidental 8-byte match has chance ~2^-44)
    needle = TEST_SEED.to_bytes(8, 'little')
    for k in ('mult', 'rot'):
        data = open(seeded[k], 'rb').read()
        assert needle not in data and needle[::-1] not in data
        assert PUB in data  # the public seed is there, as documented


# ------------------------------------------------------- 5 defaults untouched
def test_without_a_public_seed_nothing_changes(tmp_path):
    files = []
    for i in range(2):
        ctx = F.Context(LOGN, DEPTH, 40, 60, 3, seed=11)
        try:
            ctx.gen_rotation_keys(ROTS)
            assert ctx.key_is_seeded(0) == 0
            assert all(ctx.key_is_seeded(galois(k, ctx.n)) == 0 for k in ROTS)
            files.append(_save(ctx, tmp_path / f'c{i}', False))
            if i == 0:
                # ... nor does a seed set after the keys exist, or a parity call
                ctx.public_poly(PUB, 0, 0)
                ctx.set_public_seed(PUB)
                files.append(_save(ctx, tmp_path / 'c0b', False))
                assert ctx.key_is_seeded(0) == 0
        finally:
            ctx.close()
    for k in ('pub', 'sec', 'mult', 'rot'):
        ref = open(files[0][k], 'rb').read()
        assert all(open(f[k], 'rb').read() == ref for f in files[1:]), k
    # the secret, the errors and the public key do not depend on the public seed
    s = _seeded_ctx(seed=11)
    try:
        sp = _save(s, tmp_path / 's', False)
        for k in ('pub', 'sec'):
            assert open(sp[k], 'rb').read() == open(files[0][k], 'rb').read(), k
        assert open(sp['mult'], 'rb').read() != open(files[0]['mult'], 'rb').read()
    finally:
        s.close()


# -------------------------------------------------------------------- 6 CLI
def _run(cmd, ok=True):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    if ok:
        assert r.returncode == 0, f'{cmd[:3]} failed ({r.returncode}):\n{r.stdout}\n{r.stderr}'
    return r


def test_cli_sorts_from_seeded_key_files(tmp_path):
    N, d = 8, tmp_path / 'art'
    setup = [sys.executable, CLIENT, 'setup', '--dir', str(d), '--n', str(N), '--log-n', '12', '--scale-bits', '50',
             '--sign', '3,2,2', '--depth', '24', '--seed', '21', '--seeded-keys']
    r = _run(setup, ok=False)  # a test seed needs an explicit public seed
    assert r.returncode != 0 and '--public-seed' in r.stderr and not os.path.exists(d / 'key_mult.bin')
    _run(setup + ['--public-seed', PUB.hex()])
    assert F.wire_inspect(str(d / 'key_mult.bin'))['kind'] == 'eval_mult_key_seeded'
    assert F.wire_inspect(str(d / 'key_rot.bin'))['kind'] == 'eval_automorphism_key_seeded'
    inp = str(tmp_path / 'x.bin')
    _run([sys.executable, CLIENT, 'encrypt', '--dir', str(d), '--n', str(N), '--random', '5', '--output', inp])
    # the same directory's keys in the full format, through a context that loaded the seeded ones
    ctx = F.Context.deserialize(str(d / 'cc.bin'))
    try:
        ctx.deserialize_eval_mult_key(str(d / 'key_mult.bin'))
        ctx.deserialize_eval_automorphism_key(str(d / 'key_rot.bin'))
        ctx.serialize_eval_mult_key(str(d / 'key_mult_full.bin'))
        ctx.serialize_eval_automorphism_key(str(d / 'key_rot_full.bin'))
    finally:
        ctx.close()
    assert os.path.getsize(d / 'key_rot.bin') < 0.51 * os.path.getsize(d / 'key_rot_full.bin')
    outs = []
    for suffix in ('', '_full'):
        out = str(tmp_path / f'y{suffix}.bin')
        _run([CLI, '--cc', str(d / 'cc.bin'), '--key_pub', str(d / 'key_pub.bin'), '--key_mult',
              str(d / f'key_mult{suffix}.bin'), '--key_rot', str(d / f'key_rot{suffix}.bin'), '--input', inp,
              '--output', out, '--n', str(N), '--sign', '3,2,2'])
        outs.append(W.ciphertext(open(out, 'rb').read(), 1 << 12))
    assert outs[0][:4] == outs[1][:4] and outs[0][1] == N
    assert np.array_equal(outs[0][4], outs[1][4])
    r = _run([sys.executable, CLIENT, 'decrypt', '--dir', str(d), '--n', str(N), '--input', str(tmp_path / 'y.bin')])
    v = np.random.default_rng(5).permutation(N) / N
    assert np.abs(np.array([float(t) for t in r.stdout.split()]) - np.sort(v)).max() < 0.01
