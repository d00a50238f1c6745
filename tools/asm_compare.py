#!/usr/bin/env python3
"""Device assembly of two builds, function by function: which functions of the first build have a function with the same instructions in the
second (whatever its name or its file: a new template parameter or a moved type changes the mangled name, a split moves the function to
another unit), which do not, and which functions of the second are new.  Either side may be several files — one source file against the
units it was split into.  Make the inputs with
  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off --cuda-device-only -save-temps=obj -c UNIT.hip -o DIR/UNIT.o
for every unit concerned in each tree (the row-block kernels: kernels_spmv.hip, kernels_variants.hip, kernels_fused.hip, rowblock_setup.hip)
and pass the DIR/*-gfx950.s files.  Compared: everything between a function's label and its end label, comments and blank
lines dropped, the function's own name and the numbers of its local labels normalised, the `.amdhsa_kernarg_size` line left out (a trailing
parameter a form does not read changes nothing else).
usage: asm_compare.py PARENT.s NEW.s   or   asm_compare.py PARENT.s [PARENT.s ...] -- NEW.s [NEW.s ...]"""
import hashlib
import re
import subprocess
import sys


def funcs(paths):
    out, name, body = {}, None, []
    for line in (line for path in paths for line in open(path)):
        m = re.match(r'^(_Z\w+):\s*(;.*)?$', line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith('.Lfunc_end'):
                out[name], name = body, None
                continue
            text = line.split(';')[0].rstrip()
            if text.strip() and '.amdhsa_kernarg_size' not in text:
                body.append(text)
    return out


def digest(name, body):
    txt = re.sub(r'\.LBB\d+_', '.LBBn_', '\n'.join(body).replace(name, 'SELF'))
    return hashlib.md5(txt.encode()).hexdigest()


def demangled(names):
    r = subprocess.run(['c++filt'], input='\n'.join(names), capture_output=True, text=True)
    return dict(zip(names, r.stdout.split('\n')))


def main():
    args = sys.argv[1:]
    cut = args.index('--') if '--' in args else 1
    a, b = funcs(args[:cut]), funcs([p for p in args[cut:] if p != '--'])
    twins = {}
    for n, body in b.items():
        twins.setdefault(digest(n, body), []).append(n)
    da, db = demangled(list(a)), demangled(list(b))
    used, differ = set(), []
    for n, body in a.items():
        t = twins.get(digest(n, body))
        if t:
            used.update(t)
        else:
            differ.append(n)
    print(f"{len(a)} functions in the first build, {len(b)} in the second; {len(a) - len(differ)} of the first have the same instructions in the second")
    for n in differ:
        print("DIFFERS:", da[n].split('(int')[0], f"({len(a[n])} lines)")
    for n in b:
        if n not in used:
            print("NEW:", db[n].split('(int')[0], f"({len(b[n])} lines)")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
