"""The all-pairs operators against the launch ledger of the commit before they
moved onto one driver (tests/golden/pair_ledger.json, written by
tests/golden/make_pair_ledger.py).

One child process runs the recording on the library under test -- direct_sort's
rank and sort with and without the tie-break, sort_columns, select, group_sum,
running_sum (ROWS, BETWEEN), window_sum (2 and 4 factors), gather (with and
without sum_offsets) and lex_rank, at N = 8 and N = 64, under four settings of
(lanes, stack, column members) -- and every case is compared with the ledger
field by field: the kernel clock's launches and bytes per kernel and per phase
(op_bytes per phase), the counters, every output's level, slots, limbs, scale
and the SHA-256 of its words.  At one lane the pool's peak live bytes may not
exceed the recorded figure."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_pair_ledger as L  # noqa: E402

GOLDEN = L.load(os.path.join(HERE, 'golden', 'pair_ledger.json'))
CASE_IDS = [f'N{N}-{cfg[0]}-{case}' for N in L.NS for cfg in L.CONFIGS for case in L.CASES]


def test_ledger_covers_every_case():
    assert GOLDEN['header']['recordings'] == 2
    for N in L.NS:
        assert sorted(GOLDEN['cases'][str(N)]) == sorted(f'{cfg[0]}/{case}' for cfg in L.CONFIGS for case in L.CASES)
    # a field the two recordings disagreed on is not compared: none of them may be a whole case
    assert not [d for d in GOLDEN['header']['dropped'] if d.count('/') <= 3], GOLDEN['header']['dropped']


@pytest.fixture(scope='module')
def current(tmp_path_factory):
    """the same recording on the library under test, in a child process of its own"""
    out = tmp_path_factory.mktemp('ledger') / 'now.json'
    r = subprocess.run([sys.executable, os.path.join(HERE, 'golden', 'make_pair_ledger.py'), str(out)],
                       capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, f'rc={r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}'
    return L.load(str(out))['cases']


def _same(want, got, path):
    """every field the ledger kept, equal in the current run; the ledger's keys are all present"""
    if isinstance(want, dict):
        assert isinstance(got, dict), path
        assert sorted(want) == sorted(got), (path, sorted(set(want) ^ set(got)))
        for k in want:
            _same(want[k], got[k], f'{path}/{k}')
    elif isinstance(want, list):
        assert isinstance(got, list) and len(want) == len(got), path
        for i, (w, g) in enumerate(zip(want, got)):
            _same(w, g, f'{path}[{i}]')
    else:
        assert want == got, (path, want, got)


@pytest.mark.parametrize('which', CASE_IDS)
def test_case_matches_the_ledger(current, which):
    N, cfg, case = which.split('-', 2)
    want, got = GOLDEN['cases'][N[1:]][f'{cfg}/{case}'], current[N[1:]][f'{cfg}/{case}']
    dropped = [d for d in GOLDEN['header']['dropped'] if d.startswith(f'/{N[1:]}/{cfg}/{case}/')]
    if dropped:  # fields the two recordings disagreed on: taken out of the current run too
        for d in dropped:
            node, keys = got, d.split('/')[4:]
            for k in keys[:-1]:
                node = node.get(k, {})
            node.pop(keys[-1], None)
    for field in ('clock', 'counters', 'outputs'):
        _same(want[field], got[field], f'{which}/{field}')
    if 'peak' in want:
        assert got['peak'] <= want['peak'], (which, got['peak'], want['peak'])
