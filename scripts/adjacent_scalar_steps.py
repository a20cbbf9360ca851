"""From a sort-only kernel trace: the scalar steps that sit next to a product.
usage: adjacent_scalar_steps.py run_kernel_trace.csv"""
import csv
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pmc_meta import region  # noqa: E402

rows, found = region(list(csv.DictReader(open(sys.argv[1]))))
rows = [r for r in rows if 'k_region_' not in r['Kernel_Name']]
rows.sort(key=lambda r: int(r['Start_Timestamp']))


def short(r):
    m = re.search(r'(k_[a-z0-9_]+(<[^>]*>)?)\(', r['Kernel_Name'])
    return m.group(1) if m else r['Kernel_Name'][:40]


names = [short(r) for r in rows]
dur = [int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in rows]
total = sum(dur)
print(f'region found: {found}; {len(rows)} dispatches, {total / 1e6:.2f} ms of kernel time')


def is_tail(n):  # the closing row pass of a product (either class launch)
    return n.startswith('k_ntt_fwd_row<3,') or n.startswith('k_ntt_fwd_row<5,')


def is_tensor(n):
    return n in ('k_tensor', 'k_tensor_c') or n.startswith('k_tensor_lin<') or n.startswith('k_tensor_lin_c<')


def report(label, idx):
    t = sum(dur[i] for i in idx)
    print(f'{label}: {len(idx)} launches, {t / 1e6:.3f} ms ({100 * t / total:.2f}% of the kernel time)')
    return t


for k in ('k_add', 'k_add_scalar', 'k_c0_op'):
    report(f'all {k}', [i for i, n in enumerate(names) if n == k])
a = report('k_add directly in front of k_tensor / k_tensor_lin (every a + a of twice_prod is one of these)',
           [i for i, n in enumerate(names[:-1]) if n == 'k_add' and is_tensor(names[i + 1])])
b = report('k_add_scalar directly behind a closing row pass (+ const after a product, in place)',
           [i for i, n in enumerate(names) if i and n == 'k_add_scalar' and is_tail(names[i - 1])])
c = report('k_c0_op directly behind a closing row pass (+ const after a product, copying)',
           [i for i, n in enumerate(names) if i and n == 'k_c0_op' and is_tail(names[i - 1])])
report('k_add directly behind a closing row pass (not a fold the design names; for the record)',
       [i for i, n in enumerate(names) if i and n == 'k_add' and is_tail(names[i - 1])])
print(f'upper bound of both folds (every such launch removed at no cost): {(a + b + c) / 1e6:.3f} ms')
t = sum(dur[i] for i in range(1, len(names)) if names[i] == 'k_add' and is_tensor(names[i - 1]))
k = sum(1 for i in range(1, len(names)) if names[i] == 'k_add' and is_tensor(names[i - 1]))
print(f"k_add directly behind k_tensor / k_tensor_lin (mul_add's raw summand): {k} launches, {t / 1e6:.3f} ms of "
      f'{total / 1e6:.2f} ms, {len(rows)} dispatches')
