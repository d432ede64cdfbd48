#!/usr/bin/env python
"""Compare the gfx950 device code of two builds of the library kernel by kernel: is a kernel's compiled code the same,
instruction for instruction, in both trees?

Usage:  python tools/kernel_asm_diff.py OBJDIR_A OBJDIR_B [unit ...]
        (an OBJDIR is lirec_amd/_obj of a built tree; units default to every object both directories hold, e.g. gemm_p2_L2 lirec_hip)

For every unit the device code object is taken out of the host object (the .hip_fatbin section, un-bundled for gfx950),
disassembled with llvm-objdump, and each kernel symbol's instructions -- addresses and encodings stripped, operands kept -- are
compared as text.  Printed per symbol: same / DIFFERENT / ONLY-A / ONLY-B and the instruction counts.  Exit status 0; the table is
the result.  Needs ROCm's llvm tools (ROCM_PATH, default /opt/rocm); no GPU.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'lib', 'llvm', 'bin')
TARGET = 'hipv4-amdgcn-amd-amdhsa--gfx950'


def kernels(obj, tmp, tag):
    """{symbol: [instruction text]} of the device code in host object `obj`"""
    fat, co = os.path.join(tmp, tag + '.fatbin'), os.path.join(tmp, tag + '.co')
    subprocess.check_call([os.path.join(LLVM, 'llvm-objcopy'), '-O', 'binary', '--only-section=.hip_fatbin', obj, fat])
    subprocess.check_call([os.path.join(LLVM, 'clang-offload-bundler'), '--unbundle', '--type=o', '--targets=' + TARGET,
                           '--input=' + fat, '--output=' + co])
    text = subprocess.run([os.path.join(LLVM, 'llvm-objdump'), '-d', '--no-show-raw-insn', co], stdout=subprocess.PIPE, text=True, check=True).stdout
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r'^[0-9a-f]+ <(.+)>:', line)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur and line.strip():
            out[cur].append(re.sub(r'\s+', ' ', re.sub(r'//.*$', '', line)).strip())
    return {k: v for k, v in out.items() if k.startswith('_Z')}          # (kernels and functions; not the local labels)


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    a, b = sys.argv[1], sys.argv[2]
    units = sys.argv[3:] or sorted(f[:-2] for f in os.listdir(a) if f.endswith('.o') and os.path.exists(os.path.join(b, f)))
    with tempfile.TemporaryDirectory() as tmp:
        for u in units:
            ka, kb = kernels(os.path.join(a, u + '.o'), tmp, 'a'), kernels(os.path.join(b, u + '.o'), tmp, 'b')
            print('== %s' % u)
            for k in sorted(set(ka) | set(kb)):
                sa, sb = ka.get(k), kb.get(k)
                state = 'ONLY-B' if sa is None else 'ONLY-A' if sb is None else 'same' if sa == sb else 'DIFFERENT'
                print('%-10s %6s %6s  %s' % (state, '-' if sa is None else len(sa), '-' if sb is None else len(sb), k))


if __name__ == '__main__':
    main()
