"""The split inflater (rdr_inflate_decode_split), the parts that need no GPU: the candidate rule, the measure pass, the plan and the
piece decode of raider_amd/csrc/inflate_kernels.h compiled for the CPU under AddressSanitizer / UBSan (tools/probes/
inflate_split_host_check.cpp) over the shared corpus, its damaged variants and streams with true, history-keeping and false flush
points.  The probe itself compares the split decode with the serial one, slot byte by slot byte; this test adds zlib's verdict and the
piece counts, and asserts with zlib alone that every stream still exercises the case it stands for."""
import os
import shutil
import subprocess
import zlib
from pathlib import Path

import numpy as np
import pytest

from tests import deflate_craft as D
from raider_amd import deflate

REPO = Path(__file__).resolve().parent.parent
MARKER = b'\x00\x00\xff\xff'
GAP = 1024                                                       # INFL_GAP


def all_variants():
    """tests/test_inflate_host.py's set, restated."""
    items = list(D.corpus())
    for name, s in D.corpus():
        items += D.damaged(name, s)
    return items + D.specials()


def marker_ends(stream):
    """Every stream offset p with stream[p - 4 : p] == 00 00 FF FF in front of which a block header and behind which a block and the trailer fit
    (6 <= p <= len - 6)."""
    out, i = [], stream.find(MARKER)
    while i >= 0:
        if 6 <= i + 4 <= len(stream) - 6:
            out.append(i + 4)
        i = stream.find(MARKER, i + 1)
    return out


def candidates(stream):
    """The documented rule: of the marker ends in one 1024-byte window of the stream only the first and the last are kept."""
    first, last = {}, {}
    for p in marker_ends(stream):
        first.setdefault(p // GAP, p)
        last[p // GAP] = p
    return sorted(set(first.values()) | set(last.values()))


def periodic(period, n, seed):
    block = np.random.default_rng(seed).integers(0, 256, period, dtype=np.uint8).tobytes()
    return (block * (n // period + 1))[:n]


def flushed(data, step, mode, level=6):
    """(stream, flush points): `data` through one compressobj, flushed with mode(k) after every `step` bytes."""
    c = zlib.compressobj(level)
    out, points = b'', []
    for k, o in enumerate(range(0, len(data), step)):
        out += c.compress(data[o:o + step]) + c.flush(mode(k))
        points.append(len(out))
    return out + c.flush(), points


def full_stream():
    return flushed(periodic(3000, 60000, 31), 5000, lambda k: zlib.Z_FULL_FLUSH)


def sync_streams():
    return [flushed(periodic(3000, 60000, 31), 5000, lambda k: zlib.Z_SYNC_FLUSH), flushed(periodic(2500, 60000, 32), 1000, lambda k: zlib.Z_SYNC_FLUSH)]


def mixed_stream():
    return flushed(periodic(3000, 100000, 33), 5000, lambda k: zlib.Z_FULL_FLUSH if k % 2 == 0 else zlib.Z_SYNC_FLUSH)


def stored_false():
    """A level-0 stream whose payload spells the marker, once followed by a byte that reads as a final stored block's header."""
    payload = bytearray(np.random.default_rng(34).integers(1, 255, 5009, dtype=np.uint8).tobytes())
    payload[1234:1238] = MARKER
    payload[3004:3009] = MARKER + b'\x01'
    return zlib.compress(bytes(payload), 0), bytes(payload)


_CRAFTED = []


def crafted_false():
    """(stream, data): a fixed block whose codes spell 00 00 FF FF byte-aligned in the compressed bytes, or None.  In stream order a match
    of length 3 at distance 16385 is 0000001 11100 and thirteen zero extra bits, the literal 15 is 00111111 and the literal 255 nine
    ones: seventeen zeros and then twenty-four ones.  Literals of nine bits in front move the run one bit each, so one of eight
    counts puts the turn from zeros to ones on a byte boundary.  What follows the marker reads as block type 3: the candidate is false."""
    if _CRAFTED:
        return _CRAFTED[0]
    rng = np.random.default_rng(35)
    head = [int(b) for b in rng.integers(0, 144, 16400)]
    tail = [int(b) for b in rng.integers(0, 256, 700)]
    found = None
    for k in range(8):
        tokens = [200] * k + head + [(3, 16385), 15, 255, 255] + tail
        w = D.BitWriter()
        D.fixed_block(w, tokens)
        w.align()
        if MARKER in bytes(w.out):
            data = D.expand(tokens)
            found = (D.zlib_wrap(w.out, data), data)
            break
    _CRAFTED.append(found)
    return found


def extra_streams():
    """[(label, stream, expected pieces or None)]"""
    full, _ = full_stream()
    (s1, _), (s2, _) = sync_streams()
    mixed, _ = mixed_stream()
    items = [('full', full, len(candidates(full))), ('sync-5000', s1, 1), ('sync-1000', s2, 1), ('mixed', mixed, None), ('stored-false', stored_false()[0], 1)]
    crafted = crafted_false()
    if crafted is not None:
        items.append(('crafted-false', crafted[0], 1))
    return items


def test_the_streams_are_what_they_claim():
    """Each premise with zlib alone: a stream that stops exercising its case fails here."""
    full, points = full_stream()
    assert len(points) == 12 and all(full[p - 4:p] == MARKER for p in points)
    assert candidates(full) == points                            # no marker by chance, no two in one window: 12 pieces (the empty last one joins the twelfth)
    for p in points:
        zlib.decompressobj(-15).decompress(full[p:-4])           # every flush point starts a stream of its own
    for stream, points in sync_streams():
        assert all(stream[p - 4:p] == MARKER for p in points)
        for p in points[:4]:
            with pytest.raises(zlib.error, match='too far back'):
                zlib.decompressobj(-15).decompress(stream[p:-4])
    mixed, points = mixed_stream()
    assert len(points) == 20 and len(candidates(mixed)) >= 12
    stored, payload = stored_false()
    assert zlib.decompress(stored) == payload and len(candidates(stored)) >= 2
    crafted = crafted_false()
    assert crafted is not None, 'no byte-aligned marker could be crafted from fixed-code literals'
    assert zlib.decompress(crafted[0]) == crafted[1] and len(candidates(crafted[0])) >= 1
    assert deflate.flush_points(full) == 12 and deflate.flush_points(np.frombuffer(full, dtype=np.uint8)) == 12 and deflate.flush_points(b'') == 0


def test_split_probe_follows_zlib_and_the_serial_decode(tmp_path):
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not (shutil.which(hipcc) or Path(hipcc).exists()):
        pytest.skip('no hipcc to build the probe with')
    exe = tmp_path / 'inflate_split_host_check'
    subprocess.run([hipcc, '--offload-arch=gfx950', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined', '-Xarch_host', '-fno-sanitize-recover=all',
                    str(REPO / 'tools' / 'probes' / 'inflate_split_host_check.cpp'), '-o', str(exe)], check=True)
    items = [(label, s, None) for label, s in all_variants()] + extra_streams()
    good = [D.judge(s) for _, s, _ in items]
    caps = [len(d) if d is not None else 70000 for d in good]
    # damage of a stream that is decoded in pieces: truncated, a flipped byte, a wrong Adler-32, a slot one byte short
    full, points = full_stream()
    n = len(zlib.decompress(full))
    flipped = bytearray(full); flipped[points[1] + 700] ^= 0x10
    more = [('full/cut', full[:points[2] + 900], None, 70000), ('full/flip', bytes(flipped), None, 70000),
            ('full/adler', full[:-4] + bytes([full[-4] ^ 1]) + full[-3:], None, n), ('full/slot-1', full, None, n - 1), ('full/slot+7', full, 12, n + 7)]
    for label, s, pieces, cap in more:
        items.append((label, s, pieces))
        good.append(D.judge(s, cap))
        caps.append(cap)
    D.pack_probe_file(tmp_path / 'streams.bin', [s for _, s, _ in items], caps)
    r = subprocess.run([str(exe), str(tmp_path / 'streams.bin')], capture_output=True, text=True)
    assert r.returncode == 0 and not r.stderr.strip(), r.stderr[-3000:]
    lines = r.stdout.split('\n')[:-1]
    assert len(lines) == len(items)
    by = {}
    for (label, _, pieces), want, line in zip(items, good, lines):
        status, produced, crc, got = line.split()
        by[label] = (int(status), int(got))
        if want is None:
            assert 1 <= int(status) <= 4, (label, line)
            if int(status) != 4:
                assert int(got) == 1, (label, line)              # a stream that is not clean stays whole (a wrong checksum is found in pieces too)
        else:
            assert int(status) == 0 and int(produced) == len(want) and int(crc, 16) == zlib.crc32(want), (label, line)
        if pieces is not None:
            assert int(got) == pieces, (label, line)
    assert by['full'] == (0, 12) and by['sync-5000'] == (0, 1) and by['sync-1000'] == (0, 1) and by['stored-false'] == (0, 1)
    assert by['mixed'][0] == 0 and 2 <= by['mixed'][1] < 20
    assert by['fullflush'] == (0, 2) and by['syncflush'] == (0, 1)
    assert by['full/cut'][0] == 1 and by['full/flip'][0] in (3, 4) and by['full/adler'] == (4, 12) and by['full/slot-1'][0] == 2
    assert by['too-far-back'][0] == 3 and by['len-nlen'][0] == 3 and by['wrong-adler'][0] == 4
