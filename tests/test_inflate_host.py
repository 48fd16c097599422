"""Device inflate, the parts that need no GPU: the decoder's own functions (raider_amd/csrc/inflate_kernels.h, what lane 0 of
inflate_kernel runs) compiled for the CPU under AddressSanitizer / UBSan and judged by zlib over the shared corpus and its damaged
variants; the NumPy restatement of rdr_h5_unchunk; the `inflate` keyword."""
import os
import shutil
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

from tests import deflate_craft as D
from raider_amd import deflate, h5lite, tifflite

REPO = Path(__file__).resolve().parent.parent


def all_variants():
    """[(label, stream)]: the corpus, its damaged variants and the crafted damage - the set the GPU test decodes too."""
    items = list(D.corpus())
    for name, s in D.corpus():
        items += D.damaged(name, s)
    return items + D.specials()


def test_corpus_is_what_it_claims():
    names = [n for n, _ in D.corpus()]
    assert len(set(names)) == len(names)
    for name, s in D.corpus():
        assert D.judge(s) is not None, name                      # zlib accepts every corpus stream, the crafted ones included
    assert D.judge(D.crafted_far()[0]) == D.crafted_far()[1] and len(D.crafted_far()[1]) == 33394
    assert D.judge(D.crafted_near_edge()[0]) == D.crafted_near_edge()[1]
    for f in (D.crafted_dynamic_single_distance, D.crafted_dynamic_repeat_16, D.crafted_dynamic_repeat_18):
        assert D.judge(f()[0]) == f()[1]
    verdict = {n: D.judge(s) for n, s in D.specials()}
    assert verdict.pop('trailing-bytes') is not None             # bytes behind the Adler-32 are ignored
    assert all(v is None for v in verdict.values()), verdict
    with pytest.raises(zlib.error, match='too far back'):
        zlib.decompress(D.crafted_too_far())
    two = dict(D.corpus())['random-l0']
    assert two[2] == 0 and two[3:5] in (b'\xfb\xff', b'\xff\xff')  # level 0: a first stored block of 65531 (zlib 1.2.11) or 65535 bytes, not the last
    assert dict(D.corpus())['stored-65535'][2:7] == b'\x00\xff\xff\x00\x00'


def test_probe_follows_zlib(tmp_path):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not (shutil.which(hipcc) or Path(hipcc).exists()):
        pytest.skip('no hipcc to build the probe with')
    exe = tmp_path / 'inflate_host_check'
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
                    str(REPO / 'tools' / 'probes' / 'inflate_host_check.cpp'), '-o', str(exe)], check=True)
    items = all_variants()
    good = [D.judge(s) for _, s in items]
    caps = [len(d) if d is not None else 70000 for d in good]
    # the slot-size rule: one byte too small, and a slot of exactly the size with the stream's own bytes before it
    text = dict(D.corpus())['text-l6']
    items += [('slot-1', text), ('slot+0', text), ('slot-0', dict(D.corpus())['empty-l6'])]
    n = len(zlib.decompress(text))
    caps += [n - 1, n, 0]
    good += [None, zlib.decompress(text), b'']
    D.pack_probe_file(tmp_path / 'streams.bin', [s for _, s in items], caps)
    r = subprocess.run([str(exe), str(tmp_path / 'streams.bin')], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    lines = r.stdout.split('\n')[:-1]
    assert len(lines) == len(items)
    accepted = 0
    for (label, _), want, line in zip(items, good, lines):
        status, produced, crc, _tokens = line.split()
        if want is None:
            assert 1 <= int(status) <= 4, (label, line)
        else:
            assert int(status) == 0 and int(produced) == len(want) and int(crc, 16) == zlib.crc32(want), (label, line)
            accepted += 1
    assert accepted >= len(D.corpus())
    by = {label: int(line.split()[0]) for (label, _), line in zip(items, lines)}
    assert by['slot-1'] == 2 and by['wrong-adler'] == 4 and by['preset-dictionary'] == 3 and by['block-type-3'] == 3 and by['len-nlen'] == 3
    assert by['too-far-back'] == 3 and by['bad-method'] == 3 and by['text-l6/cut0'] == 1


@pytest.mark.parametrize('shape,chunk', [((37,), (16,)), ((9, 21), (4, 8)), ((5, 37, 41), (2, 16, 16)), ((3, 5, 9, 11), (2, 2, 4, 8)), ((4, 6), (4, 6))])
@pytest.mark.parametrize('dtype', ['u1', 'i2', 'f4', 'f8'])
@pytest.mark.parametrize('shuffle', [True, False])
def test_unchunk_restatement_inverts_the_cutter(shape, chunk, dtype, shuffle):
    rng = np.random.default_rng(len(shape) * 100 + np.dtype(dtype).itemsize)
    a = rng.integers(1, 250, size=shape).astype(dtype)
    raw = deflate.h5_chunks_host(a, chunk, 0, shuffle=shuffle)
    n = int(np.prod(deflate.chunk_grid(shape, chunk)))
    cb = raw.size // n
    assert np.array_equal(deflate.h5_unchunk_host(raw, cb, np.arange(n), dtype, shape, chunk, shuffle=shuffle), a)
    # a stride beyond the chunk, the chunks in another order, the other byte order
    pad = np.zeros((n, cb + 24), dtype=np.uint8)
    order = rng.permutation(n)
    other = deflate.h5_chunks_host(a.astype(np.dtype(dtype).newbyteorder('S')), chunk, 0, shuffle=shuffle).reshape(n, cb)
    pad[:, :cb] = other[order]
    assert np.array_equal(deflate.h5_unchunk_host(pad, cb + 24, order, dtype, shape, chunk, shuffle=shuffle, swap=True), a)
    if n > 1:                                                    # one chunk absent: its elements are 0
        keep = np.delete(np.arange(n), n // 2)
        got = deflate.h5_unchunk_host(raw.reshape(n, cb)[keep], cb, keep, dtype, shape, chunk, shuffle=shuffle)
        offs = tuple(int(i) * c for i, c in zip(np.unravel_index(n // 2, deflate.chunk_grid(shape, chunk)), chunk))
        hole = tuple(slice(o, o + c) for o, c in zip(offs, chunk))
        want = a.copy()
        want[hole] = 0
        assert np.array_equal(got, want) and not np.array_equal(got, a)


def test_inflate_keyword_is_validated(tmp_path):
    from tests import tiff_codec as T
    p = tmp_path / 'a.tif'
    p.write_bytes(T.make_tiff(np.arange(12, dtype=np.uint16).reshape(3, 4), compression=8))
    for bad in ('gpu', None, 1, 'Device'):
        with pytest.raises(ValueError, match='inflate must be'):
            tifflite.read(p, inflate=bad)
        with pytest.raises(ValueError, match='inflate must be'):
            deflate.inflate_mode(bad)
    a, _ = tifflite.read(p, inflate='host')
    b, _ = tifflite.read(p)                                      # 'auto' without a device: NumPy all the way, no GPU needed
    assert np.array_equal(a, b) and np.array_equal(a, np.arange(12, dtype=np.uint16).reshape(3, 4))
    assert {deflate.inflate_mode(m) for m in ('auto', 'host', 'device')} == {'auto', 'host', 'device'}
    assert hasattr(h5lite.Dataset, 'read_device')
