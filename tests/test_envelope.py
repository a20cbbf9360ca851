"""The parameter envelope (include/fhe_gpu.h at fhe_ctx_create; csrc/host/
envelope.hpp): a context the kernels' dispatch tables cannot serve is refused
with FHE_EINVAL and the parameter named, on the host, before any HIP call --
through fhe_ctx_create, through a context file, and through fhe_params_check,
the predicate alone.  Every context the suite and bench.py create is inside it.
The library loads without a device here and nothing is launched.
"""
import numpy as np
import pytest

import fhesort as F
import pyoracle as O
import wire_spec as W

# (log_n, mult_depth, scale_bits, first_bits, dnum) -> the word the message must hold
REFUSED = [
    ((12, 6, 40, 60, 0), 'dnum'),        # make_params divides by it
    ((12, 6, 40, 60, -1), 'dnum'),
    ((12, 12, 40, 60, 13), 'dnum'),      # alpha = 1: 13 digits at the top level (ModUpArgs holds 8)
    ((12, 26, 40, 60, 9), 'dnum'),       # alpha = 3: 9 digits
    ((9, 6, 40, 60, 3), 'log_n'),
    ((18, 6, 40, 60, 3), 'log_n'),
    ((4, 6, 40, 60, 3), 'log_n'),        # make_params itself takes it; the kernels' grids are n / 256
    ((12, 80, 40, 60, 3), 'dnum'),       # digits of 27 primes: dispatch_int<1, 24> of the ModUp kernels
    ((12, 47, 59, 60, 2), 'dnum'),       # digits of 24 primes at 59 bits: 24 special primes, ModDown serves 16
    ((12, 0, 40, 60, 3), 'mult_depth'),
    ((12, -1, 40, 60, 3), 'mult_depth'),
]
IDS = ['-'.join(str(v) for v in t) for t, _ in REFUSED]


def kway_dnum(depth):  # tests/test_gpu_kway.py
    return -(-(depth + 1) // 15)


def created_contexts():
    """every (log_n, mult_depth, scale_bits, first_bits, dnum) the GPU suite, smoke()
    and bench.py create an engine with"""
    out = {(12, F.size_parameters(8)[0], 40, 60, 3)}                        # smoke()
    for N in (4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048):                  # DirectSort, bench.py
        depth = F.size_parameters(N)[0]
        out |= {(lg, depth, sb, 60, 3) for lg in (11, 12, 13, 16, 17) for sb in (40, 50)}
    for N in (4, 8, 16, 32, 64, 128, 256, 512, 1024, 2048, 4096):            # MEHP24, bench.py
        p = F.mehp24_parameters(N)
        out |= {(p['log_ring'], p['depth'] + e, p['scale_bits'], 60, p['dnum']) for e in (0, 1)}
    for depth in (26, 30, 104):                                             # k-way
        out.add((11, depth, 40, 60, kway_dnum(depth)))
    out |= {(12, 50, 59, 60, 4), (12, 59, 59, 60, 4), (16, 30, 50, 60, 4), (15, 4, 50, 60, 3), (13, 30, 50, 60, 3)}
    out |= {(12, L, 40, 60, 3) for L in (3, 5, 6, 7, 8, 12, 20, 30, 50, 61, 65)}  # the wide digits: alpha 22, K 16
    out |= {(12, L, 41, 60, 3) for L in (5, 12, 50)} | {(12, 5, 59, 60, 3), (12, 12, 50, 60, 3)}
    out |= {(11, L, 59, 60, 3) for L in (24, 26, 28, 30)} | {(12, 30, 59, 60, 3), (16, 40, 59, 60, 3)}
    out |= {(16, L, b, 60, 3) for L in (6, 8, 12, 39) for b in (40, 41, 50)} | {(17, 5, 40, 60, 3), (17, 8, 41, 60, 3)}
    # tests/test_gpu_ring_sweep.py
    out |= {(lg, 6, b, 60, 3) for lg in (10, 14, 15) for b in (40, 41)}
    out |= {(16, 15, 40, 60, 8), (16, 7, 40, 60, 8), (17, 9, 40, 60, 5), (17, 6, 40, 60, 3)}
    return sorted(out)


@pytest.mark.parametrize('tup,word', REFUSED, ids=IDS)
def test_ctx_create_refuses(tup, word):
    p = F.Params(*tup, 1)
    h = F.C.c_void_p(0xdead)  # fhe_ctx_create must clear it
    rc = F.lib().fhe_ctx_create(F.C.byref(p), 0, F.C.byref(h))
    msg = F.lib().fhe_last_error().decode()
    assert rc == F.FHE_EINVAL, (rc, msg)
    assert not h.value, 'fhe_ctx_create left *out set'
    assert word in msg and str(tup[{'log_n': 0, 'mult_depth': 1, 'dnum': 4}[word]]) in msg, msg


@pytest.mark.parametrize('tup,word', REFUSED, ids=IDS)
def test_params_check_refuses(tup, word):
    with pytest.raises(F.FheError) as e:
        F.params_check(*tup)
    assert e.value.code == F.FHE_EINVAL and word in str(e.value)


@pytest.mark.parametrize('tup,word', REFUSED, ids=IDS)
def test_context_file_refused(tup, word, tmp_path):
    """a context file written with those parameters (tests/wire_spec.py): the
    header and the body agree, the checksum is right, the parameters are not"""
    log_n, depth, sb, fb, dnum = tup
    primes = [3, 5, 7]
    u = [v % 2 ** 64 for v in tup]  # the file's words are unsigned; the reader takes them as int
    body = np.array(u + [0, len(primes)] + primes, dtype=np.uint64)
    p = tmp_path / 'cc.bin'
    p.write_bytes(W.pack('context', W.params_id(*u, primes), u[0], (depth + 1) % 2 ** 64, 1, body))
    h = F.C.c_void_p(0xdead)
    rc = F.lib().fhe_deserialize_context(str(p).encode(), 0, F.C.byref(h))
    msg = F.lib().fhe_last_error().decode()
    assert rc == F.FHE_EINVAL, (rc, msg)
    assert not h.value
    assert word in msg, msg


def test_oracle_refuses_dnum_below_one():
    for dnum in (0, -1):
        with pytest.raises(Exception) as e:
            O.Context(12, 6, 40, 60, dnum, seed=1, keygen=False)
        assert 'dnum' in str(e.value)


def test_created_contexts_are_inside():
    """what the suite and bench.py create today stays creatable, with the digit
    layout the engine derives"""
    for tup in created_contexts():
        got = F.params_check(*tup)
        L, dnum = tup[1], tup[4]
        alpha = -(-(L + 1) // dnum)
        assert got['nq'] == L + 1 and got['alpha'] == alpha and got['digits'] == -(-(L + 1) // alpha), (tup, got)
        assert got['digits'] <= 8 and alpha <= 24 and 1 <= got['K'] <= 16, (tup, got)


def test_envelope_edges_are_inside():
    """the last tuple inside each bound"""
    assert F.params_check(10, 6, 40, 60, 3)['digits'] == 3
    assert F.params_check(17, 6, 40, 60, 3)['digits'] == 3
    assert F.params_check(12, 15, 40, 60, 8) == dict(nq=16, K=2, alpha=2, digits=8)
    assert F.params_check(12, 7, 40, 60, 8) == dict(nq=8, K=1, alpha=1, digits=8)
    assert F.params_check(12, 71, 30, 60, 3)['alpha'] == 24
    assert F.params_check(12, 65, 40, 60, 3) == dict(nq=66, K=16, alpha=22, digits=3)
    assert F.params_check(12, 1, 40, 60, 1) == dict(nq=2, K=2, alpha=2, digits=1)
