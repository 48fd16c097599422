"""CPU: the dynamic-table mode of the device deflate encoder (csrc/deflate_kernels.h) on the host emulation, under sanitizers.

tools/probes/deflate_dynamic_host_check.cpp is a stand-alone program (64 threads as the lanes) built with AddressSanitizer and UBSan.
`codes`: the code lengths defl_build_lengths() - the function every wave runs - gives a histogram, against a package-merge written
here: the sum of count * length must EQUAL the optimum under the limit.  `streams`: complete zlib streams, decoded by zlib, never
larger than the fixed-mode probe's streams of the same inputs.  Nothing with a sanitizer is loaded into this process; no GPU."""
import heapq
import shutil
import struct
import subprocess
import zlib
from fractions import Fraction
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parent.parent
FLAGS = ['-O1', '-g', '-std=c++17', '-pthread', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']


@pytest.fixture(scope='module')
def probes(tmp_path_factory):
    cxx = shutil.which('g++') or shutil.which('clang++')
    if cxx is None:
        pytest.skip('no host C++ compiler to build the probes with')
    d = tmp_path_factory.mktemp('probes')
    for name in ('deflate_dynamic_host_check', 'deflate_host_check'):
        subprocess.run([cxx, *FLAGS, str(REPO / 'tools' / 'probes' / f'{name}.cpp'), '-o', str(d / name)], check=True)
    return d


def package_merge_cost(counts, limit):
    """The smallest sum of count * length of a prefix code over the used symbols with no length above `limit` (Larmore & Hirschberg):
    `limit` lists, each the leaves merged with the pairs of the list before; the 2m - 2 lightest items of the last one are the code."""
    leaves = sorted((c, (i,)) for i, c in enumerate(counts) if c > 0)
    m = len(leaves)
    assert m >= 2 and (1 << limit) >= m
    cur = list(leaves)
    for _ in range(limit - 1):
        pairs = [(cur[k][0] + cur[k + 1][0], cur[k][1] + cur[k + 1][1]) for k in range(0, len(cur) - 1, 2)]
        cur = sorted(leaves + pairs, key=lambda t: t[0])
    lens = [0] * len(counts)
    for _, syms in cur[:2 * m - 2]:
        for s in syms:
            lens[s] += 1
    assert sum(Fraction(1, 1 << n) for n in lens if n) == 1 and max(lens) <= limit
    return sum(c * n for c, n in zip(counts, lens))


def huffman_depth(counts):
    """The longest code of an unrestricted Huffman build."""
    heap = [(c, 0) for c in counts if c > 0]
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def _fib(n):
    f = [1, 1]
    while len(f) < n:
        f.append(f[-1] + f[-2])
    return f[:n]


def _smooth_chunk():
    """32 768 bytes of a shuffled smooth float32 field."""
    z, y, x = np.meshgrid(np.arange(8.0), np.arange(32.0), np.arange(32.0), indexing='ij')
    a = (2.3 * np.exp(-z / 7.0) * (1.0 + 0.1 * np.sin(x / 17.0) * np.cos(y / 23.0))).astype(np.float32)
    return np.ascontiguousarray(a.reshape(-1).view(np.uint8).reshape(-1, 4).T).tobytes()


def histograms():
    """(name, counts, limit, forces the limit)"""
    fib21 = [0] * 286
    for k, c in enumerate(_fib(21)):                       # F(1..21), sum 28 656, on symbols spread over the literals, plus EOB
        fib21[3 * k] = c
    fib21_eob = list(fib21); fib21_eob[256] = 1            # with the end-of-block count of 1 every partial sum ties with the next leaf: depth 11 is optimal too
    fib10 = [0] * 19
    for k, c in enumerate(_fib(10)):                       # sum 143
        fib10[(7 * k) % 19] = c
    one = [0] * 30; one[7] = 41
    one0 = [0] * 30; one0[0] = 5
    two = [0] * 286; two[65] = 1000; two[256] = 1
    two_d = [0] * 30; two_d[0] = 3; two_d[29] = 3
    skew = np.bincount(np.frombuffer(_smooth_chunk(), dtype=np.uint8), minlength=286).tolist()
    skew[256] = 1; skew[257] = 40; skew[260] = 7; skew[285] = 3
    rng = np.random.default_rng(12)
    return [('fib21', fib21, 15, True), ('fib21_eob', fib21_eob, 15, False), ('fib10', fib10, 7, True), ('flat286', [1] * 286, 15, False), ('one_used', one, 15, False),
            ('one_used_sym0', one0, 15, False), ('two_used_ll', two, 15, False), ('two_used_d', two_d, 15, False), ('none_used', [0] * 30, 15, False),
            ('smooth_skew', skew, 15, False), ('random19', rng.integers(0, 300, 19).tolist(), 7, False),
            ('random286', (rng.integers(0, 40, 286) ** 2).tolist(), 15, False), ('full30', (rng.integers(1, 2000, 30)).tolist(), 15, False)]


def test_code_lengths_are_optimal_under_the_limit(probes, tmp_path):
    hs = histograms()
    (tmp_path / 'h.bin').write_bytes(b''.join(struct.pack(f'<II{len(c)}I', len(c), lim, *c) for _, c, lim, _ in hs))
    r = subprocess.run([str(probes / 'deflate_dynamic_host_check'), 'codes', str(tmp_path / 'h.bin'), str(tmp_path / 'l.bin')], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    raw, pos = (tmp_path / 'l.bin').read_bytes(), 0
    for name, counts, limit, forces in hs:
        lens = list(struct.unpack_from(f'<{len(counts)}I', raw, pos)); pos += 4 * len(counts)
        used = [i for i, c in enumerate(counts) if c > 0]
        if forces:
            assert huffman_depth(counts) > limit, name                 # the case does force the limit: no optimal code is that shallow
            assert package_merge_cost(counts, limit) > package_merge_cost(counts, 2 * limit), name
        assert max(lens) <= limit, name
        assert sum(Fraction(1, 1 << n) for n in lens if n) == 1, (name, lens)          # Kraft: the code is complete
        if len(used) >= 2:
            assert all((n > 0) == (c > 0) for n, c in zip(lens, counts)), name
            want = package_merge_cost(counts, limit)
            got = sum(c * n for c, n in zip(counts, lens))
            assert got == want, (name, got, want)
        else:                                                          # zlib's padding: two codes of one bit, the used symbol among them
            assert sorted(lens)[-2:] == [1, 1] and sum(lens) == 2 and all(lens[i] == 1 for i in used), (name, lens)
    assert pos == len(raw)


def stream_cases():
    rng = np.random.default_rng(4)
    y, x = np.mgrid[0:24, 0:256]
    d = (np.sin(x / 40.0) * np.cos(y / 55.0) * 2.3 + 2.5).astype(np.float32).view(np.uint32).copy()
    d[:, 1:] = d[:, 1:] - d[:, :-1]
    far = rng.integers(0, 256, 2600, dtype=np.uint8); far[2200:2500] = far[:300]
    # the cases of the existing sanitizer test (tests/test_deflate_host.py) ...
    cases = {'zero1': b'\x00', 'ab': b'ab', 'zeros63': bytes(63), 'zeros64': bytes(64), 'ff65': b'\xff' * 65, 'period3': (np.arange(700) % 3).astype(np.uint8).tobytes(),
             'period259': (np.arange(1000) % 259).astype(np.uint8).tobytes(), 'far': far.tobytes(), 'random256': rng.integers(0, 256, 3000, dtype=np.uint8).tobytes(),
             'text': b'the wet and the hydrostatic delay of the troposphere ' * 40, 'raster_p2': d.tobytes(), 'zeros32769': bytes(32769), 'ff40000': b'\xff' * 40000}
    # ... and inputs over few symbols, where dynamic tables pay
    cases['alpha4_3000'] = rng.integers(0, 4, 3000).astype(np.uint8).tobytes()
    cases['alpha4_32769'] = rng.integers(0, 4, 32769).astype(np.uint8).tobytes()
    cases['geom_40000'] = np.minimum(rng.geometric(0.5, 40000), 255).astype(np.uint8).tobytes()
    cases['one_byte'] = b'\x07'
    cases['two_bytes'] = b'\x07\x09'
    return cases


def _read_streams(path, n):
    raw, pos, out = path.read_bytes(), 0, []
    for _ in range(n):
        k, = struct.unpack_from('<I', raw, pos)
        out.append(raw[pos + 4:pos + 4 + k]); pos += 4 + k
    assert pos == len(raw)
    return out


def test_dynamic_streams_are_clean_under_sanitizers_decode_and_never_exceed_the_fixed_ones(probes, tmp_path):
    from raider_amd import deflate
    cases = stream_cases()
    (tmp_path / 'in.bin').write_bytes(struct.pack('<I', len(cases)) + b''.join(struct.pack('<I', len(c)) + c for c in cases.values()))
    r = subprocess.run([str(probes / 'deflate_dynamic_host_check'), 'streams', str(tmp_path / 'in.bin'), str(tmp_path / 'dyn.bin')], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    f = subprocess.run([str(probes / 'deflate_host_check'), str(tmp_path / 'in.bin'), str(tmp_path / 'fix.bin')], capture_output=True, text=True)
    assert f.returncode == 0 and not f.stderr.strip(), f.stderr[-3000:]
    dyn, fix = _read_streams(tmp_path / 'dyn.bin', len(cases)), _read_streams(tmp_path / 'fix.bin', len(cases))
    kinds = {}
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('stream ')]
    assert len(lines) == len(cases)
    for (name, c), z, zf, ln in zip(cases.items(), dyn, fix, lines):
        assert z[:2] == b'\x78\x01' and zlib.decompress(z) == c, name
        assert zlib.decompress(zf) == c, name
        assert len(z) <= deflate.bound(len(c)), (name, len(z))
        assert len(z) <= len(zf), (name, len(z), len(zf))
        kinds[name] = ln.split('blocks:')[1].split()
        assert len(kinds[name]) == -(-len(c) // 32768) and set(kinds[name]) <= {'s', 'f', 'd'}, ln
        print(f'{name}: input {len(c)} dynamic {len(z)} fixed {len(zf)} blocks {"".join(kinds[name])}')
    for name in ('alpha4_3000', 'alpha4_32769', 'geom_40000'):
        assert 'd' in kinds[name], (name, kinds[name])
        assert len(dyn[list(cases).index(name)]) < len(fix[list(cases).index(name)]), name
    assert set(kinds['random256']) == {'s'}
