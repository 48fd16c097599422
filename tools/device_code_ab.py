"""Do two builds of libraider_hip.so carry the same device code?   python tools/device_code_ab.py libA.so libB.so [out.json]
Takes the gfx950 code object out of each library's .hip_fatbin, then compares the set of kernel symbols and every kernel's
disassembly (instruction text, without addresses).  Needs no GPU.  Exit status 0: identical."""
import json
import os
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path(os.environ.get('ROCM_PATH', '/opt/rocm')) / 'llvm' / 'bin'


def kernels(lib, tmp):
    fat, co = tmp / (Path(lib).stem + '.fatbin'), tmp / (Path(lib).stem + '.co')
    subprocess.run([LLVM / 'llvm-objcopy', '-O', 'binary', '--only-section=.hip_fatbin', lib, fat], check=True)
    subprocess.run([LLVM / 'clang-offload-bundler', '--unbundle', '--type=o', '--targets=hipv4-amdgcn-amd-amdhsa--gfx950', f'--input={fat}',
                    f'--output={co}'], check=True)
    text = subprocess.run([LLVM / 'llvm-objdump', '-d', '--no-show-raw-insn', '--no-leading-addr', co], check=True, capture_output=True, text=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r'^[0-9a-f]* ?<(.+)>:$', line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.strip():
            out[name].append(re.sub(r'\s*//.*$', '', line).strip())      # (the trailing comment is the address)
    return out


def main():
    a_lib, b_lib = sys.argv[1], sys.argv[2]
    with tempfile.TemporaryDirectory() as d:
        a, b = kernels(a_lib, Path(d)), kernels(b_lib, Path(d))
    differing = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    res = {'symbols_a': len(a), 'symbols_b': len(b), 'only_a': sorted(set(a) - set(b)), 'only_b': sorted(set(b) - set(a)),
           'instructions_a': sum(map(len, a.values())), 'instructions_b': sum(map(len, b.values())), 'differing_kernels': differing,
           'identical': set(a) == set(b) and not differing}
    print(json.dumps(res, indent=1))
    if len(sys.argv) > 3:
        Path(sys.argv[3]).write_text(json.dumps(res, indent=1) + '\n')
    return 0 if res['identical'] else 1


if __name__ == '__main__':
    sys.exit(main())
