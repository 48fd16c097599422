"""Slow, plain TIFF pieces for the GeoTIFF tests, independent of raider_amd.tifflite: an LZW encoder and decoder (TIFF flavour:
MSB-first codes of 9 - 12 bits, Clear = 256, EOI = 257, libtiff's early change), PackBits both ways, and a synthesiser of classic /
BigTIFF files in either byte order with strips or tiles, chunky or planar bands, a predictor and GeoTIFF tags.  Files made here are
shown to decode identically by Pillow's libtiff (where Pillow reads the variant) before a test relies on them."""
import struct
import zlib

import numpy as np

CLEAR, EOI = 256, 257


class _BitWriter:
    def __init__(self):
        self.out = bytearray(); self.acc = 0; self.n = 0

    def put(self, code, width):
        self.acc = (self.acc << width) | code; self.n += width
        while self.n >= 8:
            self.out.append((self.acc >> (self.n - 8)) & 0xff); self.n -= 8
        self.acc &= (1 << self.n) - 1

    def done(self):
        if self.n:
            self.out.append((self.acc << (8 - self.n)) & 0xff); self.n = 0; self.acc = 0
        return bytes(self.out)


def lzw_encode(data, eoi=True, stats=None):
    """TIFF LZW as libtiff writes it.  stats (a dict) receives: codes (data codes written), clears (Clear codes after the first),
    max_width, kwkwk (codes equal to the decoder's next free entry)."""
    data = bytes(data)
    bw = _BitWriter()
    st = dict(codes=0, clears=0, max_width=9, kwkwk=0)
    width, nxt = 9, 258                                   # the encoder's own table: its next entry is one ahead of a decoder's
    table = {}
    bw.put(CLEAR, width)
    w = b''
    first = True

    def emit(code):
        nonlocal first
        bw.put(code, width)
        st['codes'] += 1
        st['max_width'] = max(st['max_width'], width)
        if not first and code == nxt - 1:
            st['kwkwk'] += 1
        first = False
    for b in data:
        wc = w + bytes([b])
        if len(wc) == 1 or wc in table:
            w = wc
            continue
        emit(w[0] if len(w) == 1 else table[w])
        table[wc] = nxt; nxt += 1
        if nxt > 4094:
            bw.put(CLEAR, width); st['clears'] += 1
            table = {}; nxt = 258; width = 9; first = True
        elif nxt >= (1 << width) and width < 12:
            width += 1
        w = bytes([b])
    if w:
        emit(w[0] if len(w) == 1 else table[w])
        nxt += 1                                          # (the entry a decoder adds after this code)
        if nxt >= (1 << width) and width < 12:
            width += 1
    if eoi:
        bw.put(EOI, width)
    if stats is not None:
        stats.update(st)
    return bw.done()


def lzw_decode(data, cap=None):
    """(bytes, status): status 0 ok (EOI, or the stream ended exactly when `cap` bytes were out), 1 the input ended before EOI with
    fewer than `cap` bytes out / the stream holds more than `cap`, 2 a code beyond the table.  The bytes are those of the codes read
    before the stream ended or went wrong, cut at `cap`."""
    data = bytes(data)
    out = bytearray()
    pos, nbits = 0, len(data) * 8
    width, table, prev = 9, None, None

    def finish(status):
        if cap is not None and len(out) > cap:
            return bytes(out[:cap]), 1
        return bytes(out), status
    strings = [bytes([i]) for i in range(256)] + [b'', b'']
    table = list(strings)
    while True:
        if cap is not None and len(out) > cap:
            return finish(1)
        if pos + width > nbits:
            # not a whole code left.  (a decoder reading bytewise sees the same: it needs a byte that is not there)
            return finish(0 if (cap is not None and len(out) == cap) else 1)
        code = 0
        for k in range(width):
            code = (code << 1) | ((data[(pos + k) >> 3] >> (7 - ((pos + k) & 7))) & 1)
        pos += width
        if code == EOI:
            return finish(0)
        if code == CLEAR:
            table = list(strings); width = 9; prev = None
            continue
        if prev is None:
            if code >= 256:
                return finish(2)
            out += table[code]; prev = code
            continue
        if code < len(table):
            s = table[code]
        elif code == len(table) and len(table) < 4096:
            s = table[prev] + table[prev][:1]
        else:
            return finish(2)
        out += s
        if len(table) < 4096:
            table.append(table[prev] + s[:1])
            if len(table) >= (1 << width) - 1 and width < 12:
                width += 1
        prev = code


def packbits_encode(data):
    data = bytes(data)
    out = bytearray()
    i, n = 0, len(data)
    while i < n:
        j = i
        while j + 1 < n and data[j + 1] == data[i] and j - i < 127:
            j += 1
        if j > i:
            out += bytes([257 - (j - i + 1), data[i]]); i = j + 1
            continue
        j = i
        while j < n and j - i < 128 and not (j + 2 < n and data[j] == data[j + 1] == data[j + 2]):
            j += 1
        out += bytes([j - i - 1]) + data[i:j]; i = j
    return bytes(out)


def packbits_decode(data, expect):
    out = bytearray()
    i = 0
    while i < len(data) and len(out) < expect:
        c = data[i]; i += 1
        if c < 128:
            out += data[i:i + c + 1]; i += c + 1
        elif c > 128:
            out += data[i:i + 1] * (257 - c); i += 1
    return bytes(out[:expect])


_TYPES = {'B': 1, 'H': 3, 'I': 4, 'd': 12, 'Q': 16}


def make_tiff(arr, big=False, byteorder='<', tile=None, rows_per_strip=None, planar=1, compression=1, predictor=1, photometric=1, bits=None,
              scale=None, tiepoint=None, matrix=None, geokeys=None, nodata=None, gdal_metadata=None, extra=(), second_ifd=False):
    """The bytes of a TIFF holding arr ((H, W) or (bands, H, W)).  tile = (th, tw) or None for strips.  compression 1 / 5 / 8 / 32773
    are encoded for real; any other number is written into the tag over uncompressed bytes (for the refusals).  extra: (tag, 'H' / 'I' /
    'd' / 's', values) entries; second_ifd: a 1 x 1 overview directory chained behind the first."""
    a = np.asarray(arr)
    a = a[None] if a.ndim == 2 else a
    nb, H, W = a.shape
    dt = a.dtype
    udt = np.dtype(f'u{dt.itemsize}')
    th, tw = tile if tile else (rows_per_strip or H, W)
    tiles_y, tiles_x = -(-H // th), -(-W // tw)
    planes = [a[b:b + 1] for b in range(nb)] if (planar == 2 and nb > 1) else [a]
    segs = []
    for pl in planes:
        for ty in range(tiles_y):
            for tx in range(tiles_x):
                rows = th if tile else min(th, H - ty * th)
                blk = np.zeros((rows, tw, pl.shape[0]), dtype=dt)
                src = pl[:, ty * th:ty * th + rows, tx * tw:tx * tw + tw].transpose(1, 2, 0)
                blk[:src.shape[0], :src.shape[1]] = src
                if predictor == 2 and compression in (5, 8, 32946):        # (libtiff ignores the tag for the other codecs; so does this)
                    u = blk.view(udt).copy()
                    u[:, 1:] = u[:, 1:] - u[:, :-1]
                    blk = u.view(dt)
                raw = blk.astype(dt.newbyteorder(byteorder)).tobytes()
                if compression == 5:
                    raw = lzw_encode(raw)
                elif compression in (8, 32946):
                    raw = zlib.compress(raw)
                elif compression == 32773:
                    raw = b''.join(packbits_encode(raw[r * (len(raw) // rows):(r + 1) * (len(raw) // rows)]) for r in range(rows))
                segs.append(raw)
    sfmt = {'u': 1, 'i': 2, 'f': 3}[dt.kind]
    bo = byteorder
    off_t = 'Q' if big else 'I'
    ent = [(256, 'I', [W]), (257, 'I', [H]), (258, 'H', [bits or dt.itemsize * 8] * nb), (259, 'H', [compression]), (262, 'H', [photometric]), (277, 'H', [nb]),
           (284, 'H', [planar]), (339, 'H', [sfmt] * nb)]
    if predictor != 1:
        ent.append((317, 'H', [predictor]))
    if tile:
        ent += [(322, 'I', [tw]), (323, 'I', [th]), (324, off_t, None), (325, off_t, [len(s) for s in segs])]
    else:
        ent += [(278, 'I', [th]), (273, off_t, None), (279, off_t, [len(s) for s in segs])]
    if scale is not None:
        ent.append((33550, 'd', list(scale)))
    if tiepoint is not None:
        ent.append((33922, 'd', list(tiepoint)))
    if matrix is not None:
        ent.append((34264, 'd', list(matrix)))
    if geokeys is not None:
        ent.append((34735, 'H', list(geokeys)))
    if nodata is not None:
        ent.append((42113, 's', str(nodata)))
    if gdal_metadata is not None:
        ent.append((42112, 's', gdal_metadata))
    ent += list(extra)
    ent.sort(key=lambda e: e[0])
    head = 16 if big else 8
    pos = head
    offsets = []
    for s in segs:
        offsets.append(pos); pos += len(s) + (len(s) & 1)
    ifd_pos = pos
    esz, vsz = (20, 8) if big else (12, 4)
    cnt_fmt = 'Q' if big else 'H'
    extra_pos = ifd_pos + struct.calcsize('=' + cnt_fmt) + len(ent) * esz + vsz
    ifd = bytearray(struct.pack(bo + cnt_fmt, len(ent)))
    blob = bytearray()
    for tag, f, vals in ent:
        if vals is None:
            vals = offsets
        if f == 's':
            payload = vals.encode('latin-1') + b'\x00'; typ = 2; count = len(payload)
        else:
            payload = struct.pack(bo + f * len(vals), *vals); typ = _TYPES[f]; count = len(vals)
        ifd += struct.pack(bo + 'HH' + off_t, tag, typ, count)
        if len(payload) <= vsz:
            ifd += payload + bytes(vsz - len(payload))
        else:
            ifd += struct.pack(bo + off_t, extra_pos + len(blob)); blob += payload + bytes(len(payload) & 1)
    tail = b''
    next_pos = 0
    if second_ifd:                                        # a 1 x 1 uint8 overview whose pixel lives in its own StripOffsets value
        next_pos = extra_pos + len(blob)
        e2 = [(256, 'I', [1]), (257, 'I', [1]), (258, 'H', [8]), (259, 'H', [1]), (262, 'H', [1]), (273, off_t, [0]), (277, 'H', [1]), (278, 'I', [1]), (279, off_t, [1])]
        t = bytearray(struct.pack(bo + cnt_fmt, len(e2)))
        for tag, f, vals in e2:
            payload = struct.pack(bo + f * len(vals), *vals)
            t += struct.pack(bo + 'HH' + off_t, tag, _TYPES[f], len(vals)) + payload + bytes(vsz - len(payload))
        t += struct.pack(bo + off_t, 0)
        tail = bytes(t)
    ifd += struct.pack(bo + off_t, next_pos)
    mark = b'II' if bo == '<' else b'MM'
    out = bytearray(mark + (struct.pack(bo + 'HHHQ', 43, 8, 0, ifd_pos) if big else struct.pack(bo + 'HI', 42, ifd_pos)))
    for s in segs:
        out += s + bytes(len(s) & 1)
    return bytes(out + ifd + blob + tail)


GEO_4326 = [1, 1, 0, 3, 1024, 0, 1, 2, 1025, 0, 1, 1, 2048, 0, 1, 4326]


def pack_codes(codes):
    """(code, width) pairs as a TIFF LZW bit stream - for streams no encoder would write."""
    bw = _BitWriter()
    for c, w in codes:
        bw.put(c, w)
    return bw.done()


def lzw_cases():
    """{name: (stream, output capacity)}: the LZW streams both the host sanitizer probe and the device kernel are fed.  Good ones first,
    then the three damaged kinds.  Every property a name claims is asserted here from the encoder's own counts."""
    rng = np.random.default_rng(1234)
    cases = {}
    st = {}
    d = rng.integers(0, 256, 3000, dtype=np.uint8).tobytes()
    cases['widths_9_to_12'] = (lzw_encode(d, stats=st), len(d))
    assert st['max_width'] == 12 and st['clears'] == 0
    d = rng.integers(0, 256, 16384, dtype=np.uint8).tobytes()
    full = lzw_encode(d, stats=st)
    cases['table_fills_and_clears'] = (full, len(d))
    assert st['codes'] > 4094 and st['clears'] >= 1
    cases['run_of_one_byte'] = (lzw_encode(b'\x07' * 700, stats=st), 700)
    assert st['kwkwk'] > 10
    cases['eoi_before_full'] = (lzw_encode(b'hello world' * 3), 100)
    cases['one_byte'] = (lzw_encode(b'Z'), 1)
    d = rng.integers(0, 4, 1001, dtype=np.uint8).tobytes()
    cases['odd_output'] = (lzw_encode(d), 1001)
    cases['no_eoi_exactly_full'] = (lzw_encode(d, eoi=False), 1001)
    cases['bad_truncated'] = (full[:len(full) // 2], 16384)
    cases['bad_code_beyond_table'] = (pack_codes([(CLEAR, 9), (65, 9), (66, 9), (300, 9), (67, 9), (EOI, 9)]), 64)
    cases['bad_first_code_not_a_byte'] = (pack_codes([(CLEAR, 9), (258, 9), (EOI, 9)]), 64)
    cases['bad_output_shorter'] = (cases['widths_9_to_12'][0], 1000)
    cases['bad_empty'] = (b'', 16)
    return cases
