"""Per-kernel comparison of two directories of gfx950 device assembly (refactoring tool: "same device code").

  hipcc <build.py's FLAGS> --cuda-device-only -S a/gn.hip -o /tmp/a/gn.s      (one .s per .hip, both sides)
  python tools/kernel_isa_diff.py /tmp/a /tmp/b [-v] [-q]

For every kernel symbol (the names of the .amdhsa_kernel blocks) of the *.s files of a directory: the body, from the
symbol's label to its .Lfunc_end, and the .amdhsa_kernel descriptor block, as text. A local label carries the index of
the function within its file, which changes when a kernel moves to another file: .LBB<n>_ becomes .LBB_ and
.Lfunc_end<n> becomes .Lfunc_end before the comparison. The assembler's trailing comments ("; in Loop: Header=BB14_4")
repeat that index and are no code: they are dropped. A symbol that several files define (internal linkage) is listed
once per file. One line per kernel: identical, differing, only in A, only in B
(-v: a unified diff of the differing ones; -q: the identical ones counted per file, not listed). Exit status 0 only if every kernel is identical.
"""
import difflib
import glob
import os
import re
import sys


def kernels(folder):
    out = {}
    for path in sorted(glob.glob(os.path.join(folder, '*.s'))):
        s = open(path).read()
        s = re.sub(r'\.LBB\d+_', '.LBB_', s)
        s = re.sub(r'\.Lfunc_end\d+', '.Lfunc_end', s)
        s = re.sub(r'[ \t]*;.*', '', s)             # trailing comments (';' starts one: no strings inside a kernel)
        lines = s.split('\n')
        start = {l[:-1].split(':')[0]: i for i, l in enumerate(lines) if l[:1] not in ('', '\t', ' ', '.', ';') and ':' in l}
        for i, l in enumerate(lines):
            t = l.strip()
            if not t.startswith('.amdhsa_kernel '):
                continue
            name = t.split()[1]
            j = next(k for k in range(i, len(lines)) if lines[k].strip() == '.end_amdhsa_kernel')
            b0 = start[name]
            b1 = next(k for k in range(b0, len(lines)) if lines[k].startswith('.Lfunc_end'))
            base = os.path.basename(path)
            if (name, base) in out:
                sys.exit(f'{name}: defined twice in {path}')
            out[(name, base)] = ('\n'.join(lines[b0:b1 + 1]), '\n'.join(lines[i:j + 1]), base)
    # a kernel with internal linkage (anonymous namespace in a shared header) exists once per file: keyed with its file
    seen = [n for n, _ in out]
    return {(n if seen.count(n) == 1 else f'{n} [{f}]'): v for (n, f), v in out.items()}


args = [a for a in sys.argv[1:] if a not in ('-v', '-q')]
verbose, quiet = '-v' in sys.argv[1:], '-q' in sys.argv[1:]
same = {}
A, B = kernels(args[0]), kernels(args[1])
count = {'identical': 0, 'differing': 0, 'only in A': 0, 'only in B': 0}
for name in sorted(set(A) | set(B)):
    if name not in B:
        res, where = 'only in A', A[name][2]
    elif name not in A:
        res, where = 'only in B', B[name][2]
    else:
        res = 'identical' if A[name][:2] == B[name][:2] else 'differing'
        where = f'{A[name][2]} -> {B[name][2]}'
    count[res] += 1
    if quiet and res == 'identical':
        same[where] = same.get(where, 0) + 1
        continue
    print(f'{res:10s} {name}  ({where})')
    if verbose and res == 'differing':
        for k, what in ((0, 'body'), (1, 'descriptor')):
            d = difflib.unified_diff(A[name][k].split('\n'), B[name][k].split('\n'), 'A ' + what, 'B ' + what, lineterm='', n=2)
            print('\n'.join(d))
for where, n in sorted(same.items()):
    print(f'identical  {n} kernels  ({where})')
print(f"{len(A)} kernels in A, {len(B)} in B: " + ', '.join(f'{v} {k}' for k, v in count.items()))
sys.exit(0 if count['identical'] == len(A) == len(B) else 1)
