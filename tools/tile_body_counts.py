#!/usr/bin/env python3
"""Per ray kernel of an AMDGPU assembly file (hipcc -S --cuda-device-only): registers, scratch, occupancy and the counts of lane
spills (v_readlane / v_writelane) and 64-bit vector adds (v_lshl_add_u64) in the whole kernel and inside its tile loop - the
loop with the longest backward branch.  `--loops NAME_PART` also lists every loop nested in the tile loop with a hash of its opcode
sequence, and `--list HASH` the instructions of one of them.

    tile_body_counts.py file.s [--loops NAME_PART [--list HASH]]"""
import re
import sys


def kernels(txt):
    """name -> list of instruction / label lines of the kernel's body"""
    out = {}
    for m in re.finditer(r'^(_ZN3rdr\w+):.*?\n(.*?)^\s*s_endpgm', txt, re.S | re.M):
        lines = [l.split(';')[0].strip() for l in m.group(2).split('\n')]
        out[m.group(1)] = [l for l in lines if l and (not l.startswith('.') or re.fullmatch(r'\.\w+:', l))]
    return out


def loops(body):
    """(start, end) line indices of every backward branch"""
    labels = {l[:-1]: i for i, l in enumerate(body) if re.fullmatch(r'\.?\w+:', l)}
    res = []
    for i, l in enumerate(body):
        m = re.match(r's_c?branch\w*\s+(\.?\w+)', l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            res.append((labels[m.group(1)], i))
    return res


def count(lines, pat):
    return sum(1 for l in lines if re.match(pat, l))


def meta(txt):
    res = {}
    for blk in txt.split('  - .agpr_count')[1:]:
        name = re.search(r'\.name:\s+(\S+)', blk).group(1)
        g = lambda k: int(re.search(r'\.%s:\s+(\d+)' % k, blk).group(1))
        res[name] = (g('vgpr_count'), g('sgpr_count'), g('private_segment_fixed_size'))
    return res


def occupancy(txt, name):
    m = re.search(r'; Occupancy: (\d+)', txt[txt.index(name + ':'):])
    return int(m.group(1)) if m else -1


def short(name):
    name = re.sub(r'^_ZN3rdr\d+', '', name)
    name = re.sub(r'I15HIP_vector_typeI(.)Lj2EE', r'<\1,', name)
    name = re.sub(r'EEvNS_.*', '>', name)
    return re.sub(r'L[bi](\d+)E', r'\1,', name).replace(',>', '>')


def main():
    txt = open(sys.argv[1]).read()
    ks = kernels(txt)
    md = meta(txt)
    want = ('crossings_kernel', 'march_kernel', 'march_epochs_kernel')
    print(f"{'kernel':44s} vgpr sgpr scratch occ | lane r/w total loop | lshl_add_u64 total loop | valu loop")
    for name, body in ks.items():
        if not any(w in name for w in want):
            continue
        ls = loops(body)
        a, b = max(ls, key=lambda ab: ab[1] - ab[0]) if ls else (0, 0)
        lane = r'v_(read|write)lane_b32'
        v, s, sc = md.get(name, (-1, -1, -1))
        print(f"{short(name):44s} {v:4d} {s:4d} {sc:7d} {occupancy(txt, name):3d} | {count(body, lane):14d} {count(body[a:b], lane):4d} |"
              f" {count(body, 'v_lshl_add_u64'):18d} {count(body[a:b], 'v_lshl_add_u64'):4d} | {count(body[a:b], 'v_'):9d}")
    if '--loops' in sys.argv:
        # every loop nested in the tile loop of the kernels whose name holds NAME_PART: first label, lines, vector instructions and a
        # hash of its opcode sequence (registers and operands left out) - equal hashes in two builds: the loop did not move
        import hashlib
        part = sys.argv[sys.argv.index('--loops') + 1]
        for name, body in ks.items():
            if part not in name:
                continue
            ls = loops(body)
            ta, tb = max(ls, key=lambda ab: ab[1] - ab[0])
            print(f'\nloops inside the tile loop of {short(name)}: first label, lines, vector instructions, opcode hash')
            for a, b in sorted(set(ls)):
                if (a, b) == (ta, tb) or a < ta or b > tb:
                    continue
                ops = [l.split()[0] for l in body[a:b + 1] if not l.endswith(':')]
                print(f'  {b - a:5d} lines {count(body[a:b], "v_"):4d} v_  {hashlib.sha1(" ".join(ops).encode()).hexdigest()[:12]}')
            if '--list' in sys.argv:
                # the instructions of the loop with the given opcode hash that are not inside a loop nested in it
                want_hash = sys.argv[sys.argv.index('--list') + 1]
                for a, b in sorted(set(ls)):
                    ops = [l.split()[0] for l in body[a:b + 1] if not l.endswith(':')]
                    if hashlib.sha1(" ".join(ops).encode()).hexdigest()[:12] != want_hash:
                        continue
                    inner = [(c, d) for c, d in ls if a <= c and d <= b and (c, d) != (a, b)]
                    for i in range(a, b + 1):
                        if not any(c <= i <= d for c, d in inner):
                            print('    ' + body[i])


if __name__ == '__main__':
    main()
