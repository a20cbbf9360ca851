"""Seeded switching keys on the CPU (wire kinds 7 and 8, public stream v1:
csrc/wire/wire.hpp): the restatement's ChaCha20 against the library's block
function, restated files through the library's header / checksum validation,
the damage cases of test_wire.py on them, and the host stream function, run in
a stand-alone program under the address and undefined-behaviour sanitizers,
against the numpy restatement word for word.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import fhesort as F
import wire_seeded_spec as S

HERE = os.path.dirname(os.path.abspath(__file__))
HOST = os.path.join(HERE, '..', 'fhe-sorting_amd', 'csrc', 'host', 'hostmath.cpp')
SEED = bytes(range(100, 132))


def _prng_block(key, counter, nonce):
    u32 = F.C.c_uint32
    out = (u32 * 16)()
    assert F.lib().fhe_prng_block((u32 * 8)(*[int(k) for k in key]), int(counter), (u32 * 3)(*[int(x) for x in nonce]),
                                  out) == F.FHE_OK
    return np.array(list(out), dtype=np.uint32)


def test_restated_chacha20_is_rfc8439():
    # RFC 8439 §2.3.2: key 00..1f, counter 1, nonce 00 00 00 09 00 00 00 4a 00 00 00 00
    key = np.frombuffer(bytes(range(32)), dtype='<u4')
    nonce = (0x09000000, 0x4a000000, 0)
    want = np.array([0xe4e7f110, 0x15593bd1, 0x1fdd0f50, 0xc47120a3, 0xc7f4d1c7, 0x0368c033, 0x9aaa2204, 0x4e6cd4c3,
                     0x466482d2, 0x09aa9f07, 0x05d7c214, 0xa2028bd9, 0xd19c12b5, 0xb94e16de, 0xe883d0cb, 0x4e3c50a2],
                    dtype=np.uint32)
    got = S.chacha20_blocks(key, [1], nonce)
    assert np.array_equal(got[0], want)
    assert np.array_equal(_prng_block(key, 1, nonce), want)


def test_restated_chacha20_equals_the_library():
    rng = np.random.default_rng(8439)
    for _ in range(4):
        key = rng.integers(0, 1 << 32, size=8, dtype=np.uint64)
        nonce = [int(x) for x in rng.integers(0, 1 << 32, size=3, dtype=np.uint64)]
        counters = [0, 1, 0xffffffff] + [int(x) for x in rng.integers(0, 1 << 32, size=3, dtype=np.uint64)]
        got = S.chacha20_blocks(key, counters, nonce)
        for i, c in enumerate(counters):
            assert np.array_equal(got[i], _prng_block(key, c, nonce)), (c, nonce)


def _files(tmp_path, log_n=4, nq=3, K=2, digits=2):
    n, nall = 1 << log_n, nq + K
    rng = np.random.default_rng(78)
    b = rng.integers(0, 1 << 39, size=(digits, nall, n), dtype=np.uint64)
    p7, p8 = tmp_path / 'mult_seeded.bin', tmp_path / 'rot_seeded.bin'
    p7.write_bytes(S.pack_eval_mult(0x77, log_n, nq, K, SEED, b))
    keys = [(5, b), (25, b + np.uint64(1)), (2 * n - 1, b + np.uint64(2))]
    p8.write_bytes(S.pack_automorphism(0x88, log_n, nq, K, SEED, keys))
    return p7, p8, b, keys, digits * nall * n


def test_inspect_knows_the_seeded_kinds(tmp_path):
    p7, p8, b, keys, bw = _files(tmp_path)
    i7, i8 = F.wire_inspect(str(p7)), F.wire_inspect(str(p8))
    assert i7['kind'] == 'eval_mult_key_seeded' and i8['kind'] == 'eval_automorphism_key_seeded'
    assert i7['body_words'] == 6 + bw
    assert i8['body_words'] == 6 + len(keys) * (1 + bw)
    assert (i7['params_id'], i7['log_n'], i7['nq'], i7['K'], i7['version']) == (0x77, 4, 3, 2, 1)
    assert (i8['params_id'], i8['log_n'], i8['nq'], i8['K'], i8['version']) == (0x88, 4, 3, 2, 1)
    # the restated parsers read what was packed
    h, seed, got = S.eval_mult(p7.read_bytes())
    assert seed == SEED and np.array_equal(got, b) and h['params_id'] == 0x77
    h, seed, got = S.automorphism(p8.read_bytes(), b.shape[0])
    assert seed == SEED and sorted(got) == [g for g, _ in keys]
    for g, kb in keys:
        assert np.array_equal(got[g], kb)


def test_damaged_seeded_files_are_rejected_with_eio(tmp_path):
    for p in _files(tmp_path)[:2]:
        raw = bytearray(p.read_bytes())
        cases = {
            'flipped body bit': raw[:80] + bytes([raw[80] ^ 1]) + raw[81:],
            'flipped seed bit': raw[:64 + 16] + bytes([raw[64 + 16] ^ 0x80]) + raw[64 + 17:],
            'flipped header word': raw[:24] + bytes([raw[24] ^ 4]) + raw[25:],
            'truncated': raw[:-8],
            'extra bytes': raw + b'\0' * 8,
        }
        for what, data in cases.items():
            q = tmp_path / 'bad.bin'
            q.write_bytes(bytes(data))
            with pytest.raises(F.FheError) as e:
                F.wire_inspect(str(q))
            assert e.value.code == F.FHE_EIO, (p.name, what)


@pytest.fixture(scope='module')
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp('pubstream') / 'public_stream_check'
    r = subprocess.run(['g++', '-O1', '-g', '-std=c++17', '-ffp-contract=off', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=undefined', '-o', str(out),
                        os.path.join(HERE, 'public_stream_check.cpp'), HOST, '-lm'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return str(out)


# primes of the ring-2^12, depth-6, 40-bit context: the 60-bit q_0 and a special
# prime (just below 2^60: almost no candidate rejected), a scaling prime just
# above 2^40 (41-bit candidates, about half rejected) and one just below
STREAM_PRIMES = [1152921504606830593, 1099511922689, 1099511480321, 1152921504606748673]


@pytest.mark.parametrize('kid,digit,first,n', [(0, 0, 0, 64), (5, 2, 3, 64), (8191, 1, 9, 256), (25, 0, 1, 8)])
def test_host_stream_equals_the_restatement_under_sanitizers(exe, kid, digit, first, n):
    r = subprocess.run([exe, SEED.hex(), str(kid), str(digit), str(first), str(n)] + [str(q) for q in STREAM_PRIMES],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stderr == ''  # no sanitizer report
    rows = [np.array([int(t, 16) for t in line.split()], dtype=np.uint64) for line in r.stdout.splitlines()]
    assert len(rows) == len(STREAM_PRIMES)
    for i, q in enumerate(STREAM_PRIMES):
        want = S.public_limb(SEED, kid, digit, first + i, q, n)
        assert np.array_equal(rows[i], want), (kid, digit, first + i)
        assert int(rows[i].max()) < q
    # both regimes ran: the words of a prime just above 2^40 need second attempts
    first_try = S.chacha20_blocks(S.seed_key(SEED), np.arange(n // 8), (kid, digit | ((first + 1) << 16), S.NONCE_TAG))
    cand = (first_try[:, 0::2].astype(np.uint64) | (first_try[:, 1::2].astype(np.uint64) << np.uint64(32))) >> np.uint64(23)
    assert (cand.ravel() >= np.uint64(STREAM_PRIMES[1])).any() or n <= 8
