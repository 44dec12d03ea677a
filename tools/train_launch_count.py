"""Launches and kernel time of ONE config-5 training step from two rocprofv3 --kernel-trace --stats runs of tools/train_step_time.py
with different step counts: (calls_b - calls_a) / (steps_b - steps_a) per kernel -- model set-up (weights, the encoder pass that
produces the features) cancels out.
    python tools/train_launch_count.py <stats_a.csv> <steps_a> <stats_b.csv> <steps_b> [rows]
Two steps kernel by kernel (e.g. the bf16 step against the fp16 + GradScaler one): the storage-typed twins (bf16_t / f16_t
instantiations of one kernel) share a row, and the launches only one of the two steps makes are listed at the end.
    python tools/train_launch_count.py --vs <x_a.csv> <steps_a> <x_b.csv> <steps_b> <y_a.csv> <steps_a> <y_b.csv> <steps_b>"""
import csv
import re
import sys


def load(path):
    return {r['Name']: (int(r['Calls']), float(r['TotalDurationNs'])) for r in csv.DictReader(open(path))}


def per_step(fa, na, fb, nb):
    a, b = load(fa), load(fb)
    rows = []
    for name, (cb, tb) in b.items():
        ca, ta = a.get(name, (0, 0.0))
        per, us = (cb - ca) / (nb - na), (tb - ta) / (nb - na) / 1e3
        if abs(per) > 1e-9:
            rows.append((per, us, name))
    return rows


def twin_key(name):
    return re.sub(r'\b(hs::)?(bf16_t|f16_t|__hip_bfloat16|c10::BFloat16|c10::Half|__half|at::BFloat16|at::Half)\b', 'T', name)


if sys.argv[1] == '--vs':
    x = per_step(sys.argv[2], int(sys.argv[3]), sys.argv[4], int(sys.argv[5]))
    y = per_step(sys.argv[6], int(sys.argv[7]), sys.argv[8], int(sys.argv[9]))
    kx, ky = {}, {}
    for per, us, name in x:
        kx.setdefault(twin_key(name), []).append((per, us))
    for per, us, name in y:
        ky.setdefault(twin_key(name), []).append((per, us))
    tot = lambda rows: (sum(r[0] for r in rows), sum(r[1] for r in rows))      # noqa: E731
    print(f'per step: first {tot(x)[0]:.1f} launches {tot(x)[1]:.1f} us | second {tot(y)[0]:.1f} launches {tot(y)[1]:.1f} us')
    print(f'{"calls":>6} {"first us":>9} {"second us":>9} {"ratio":>6}  kernel (both steps)')
    for k in sorted(set(kx) & set(ky), key=lambda k: -sum(u for _, u in ky[k])):
        cx, ux = map(sum, zip(*kx[k]))
        cy, uy = map(sum, zip(*ky[k]))
        print(f'{cy:6.1f} {ux:9.1f} {uy:9.1f} {uy / ux if ux else float("nan"):6.3f}  {k[:100]}' + ('' if abs(cx - cy) < 1e-9 else f'  (calls {cx:.1f} vs {cy:.1f})'))
    for label, only, rows in (('first step only', set(kx) - set(ky), kx), ('second step only', set(ky) - set(kx), ky)):
        print(f'-- {label}: {len(only)} kernels')
        for k in sorted(only):
            c, u = map(sum, zip(*rows[k]))
            print(f'{c:6.1f} x {u / c:7.2f} us = {u:7.1f}  {k[:110]}')
    sys.exit(0)

fa, na, fb, nb = sys.argv[1], int(sys.argv[2]), sys.argv[3], int(sys.argv[4])
top = int(sys.argv[5]) if len(sys.argv) > 5 else 0
rows = per_step(fa, na, fb, nb)
own = [r for r in rows if 'hs::' in r[2][:12]]
stock = [r for r in rows if 'hs::' not in r[2][:12]]
print(f'per step: {sum(r[0] for r in rows):.1f} launches, {sum(r[1] for r in rows):.1f} us of kernel time '
      f'| own {sum(r[0] for r in own):.1f} launches {sum(r[1] for r in own):.1f} us | stock {sum(r[0] for r in stock):.1f} launches {sum(r[1] for r in stock):.1f} us')
for per, us, name in sorted(rows, key=lambda r: -r[1])[:top]:
    print(f'{per:6.1f} x {us / per:7.2f} us = {us:7.1f}  {name[:110]}')
