#!/usr/bin/env python3
"""Compare two device assembly listings kernel by kernel: `hipcc -O3 -std=c++17 --offload-arch=gfx950 -S --cuda-device-only FILE.hip -o X.s` of two
trees.  A refactor that must leave device code alone shows here as "N kernels, 0 differ": for every .amdhsa_kernel of either listing, the
instruction text and the .amdhsa_* resource directives are compared; the order of kernels (and with it the function number inside local labels such as .LBB5_2), .file / .loc / .ident lines, comments and blank
lines do not count.

    python tools/asm_kernel_diff.py parent.s branch.s
"""
import re
import sys


def kernels(path):
    """{symbol: (instruction lines, resource directives)}"""
    text = open(path).read().splitlines()
    body, res, cur, in_desc = {}, {}, None, None
    for raw in text:
        line = re.sub(r'\s*;.*$', '', raw).strip()
        line = re.sub(r'\.L(BB|JTI|tmp|func_begin|func_end)\d+', r'.L\1#', line)      # local labels carry the function's position in the file
        if not line or re.match(r'\.(file|loc|ident|section|p2align|globl|protected|type|size|text|weak|hidden|cfi_\w+|addrsig\w*)\b', line):
            if line.startswith('.section') or line.startswith('.text'):
                cur = None
            continue
        m = re.match(r'\.amdhsa_kernel\s+(\S+)', line)
        if m:
            in_desc = m.group(1); res[in_desc] = []
            continue
        if line == '.end_amdhsa_kernel':
            in_desc = None
            continue
        if in_desc:
            res[in_desc].append(line)
            continue
        m = re.match(r'([A-Za-z_.$][\w.$]*):$', line)
        if m and not m.group(1).startswith('.L'):
            cur = m.group(1); body[cur] = []
            continue
        if cur is not None:
            body[cur].append(line)
    return {k: (body.get(k, []), res[k]) for k in res}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = sorted(set(a) ^ set(b))
    for k in bad:
        print('only in', sys.argv[1] if k in a else sys.argv[2], ':', k)
    differ = [k for k in sorted(set(a) & set(b)) if a[k] != b[k]]
    for k in differ:
        print('differs:', k, '(instructions)' if a[k][0] != b[k][0] else '(resource directives)')
    print(f'{len(a)} / {len(b)} kernels, {len(differ)} differ, {len(bad)} unmatched; '
          f'{sum(len(v[0]) for v in a.values())} / {sum(len(v[0]) for v in b.values())} instruction lines')
    return 1 if differ or bad else 0


if __name__ == '__main__':
    sys.exit(main())
