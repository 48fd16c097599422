"""Crafted DEFLATE streams and the corpus the inflate tests share (a helper, not a test).

zlib never emits a distance above 32506 (window minus lookahead), a distance code set of one code, or a code-length repeat that runs
from the literal / length lengths into the distance lengths, so streams that hold them are written here, bit by bit, from explicit
token lists: a token is a literal (an int 0 .. 255) or a match (len, dist).  zlib.decompress is the judge of every stream."""
import struct
import zlib

import numpy as np

_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
_CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


class BitWriter:
    """LSB-first bits, as RFC 1951 packs them."""

    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def bits(self, value, count):
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, code, length):
        """A Huffman code: most significant bit first."""
        for i in range(length - 1, -1, -1):
            self.bits((code >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bytes(self, data):
        self.align()
        self.out += data


def canonical(lengths):
    """{symbol: (code, length)} of the canonical code with these lengths (0 = no code)."""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for s, l in enumerate(lengths):
        if l:
            out[s] = (nxt[l], l)
            nxt[l] += 1
    return out


def _len_sym(n):
    if n == 258:
        return 28
    return max(i for i in range(28) if _LEN_BASE[i] <= n)


def _dist_sym(d):
    return max(i for i in range(30) if _DIST_BASE[i] <= d)


def _tokens(w, tokens, lit, dist):
    for t in tokens:
        if isinstance(t, tuple):
            n, d = t
            i = _len_sym(n)
            w.code(*lit[257 + i]); w.bits(n - _LEN_BASE[i], _LEN_EXTRA[i])
            j = _dist_sym(d)
            w.code(*dist[j]); w.bits(d - _DIST_BASE[j], _DIST_EXTRA[j])
        else:
            w.code(*lit[t])
    w.code(*lit[256])


FIXED_LIT = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_DIST = [5] * 32


def fixed_block(w, tokens, final=True, btype=1):
    w.bits(1 if final else 0, 1); w.bits(btype, 2)
    _tokens(w, tokens, canonical(FIXED_LIT), canonical(FIXED_DIST))


def stored_block(w, data, final=True, nlen=None):
    w.bits(1 if final else 0, 1); w.bits(0, 2)
    w.align()
    w.out += struct.pack('<HH', len(data), (len(data) ^ 0xffff) if nlen is None else nlen)
    w.out += data


def code_length_symbols(seq):
    """Run-length symbols (sym, extra bits, extra value) over the COMBINED literal / distance length sequence: unlike zlib's, a run
    does not stop at the boundary between the two."""
    out, i = [], 0
    while i < len(seq):
        v, r = seq[i], 1
        while i + r < len(seq) and seq[i + r] == v:
            r += 1
        i += r
        if v == 0:
            while r >= 11:
                k = min(r, 138); out.append((18, 7, k - 11)); r -= k
            if r >= 3:
                out.append((17, 3, r - 3)); r = 0
        else:
            out.append((v, 0, 0)); r -= 1
            while r >= 3:
                k = min(r, 6); out.append((16, 2, k - 3)); r -= k
        out += [(v, 0, 0)] * r
    return out


def dynamic_block(w, tokens, lit_lens, dist_lens, final=True):
    """A BTYPE 10 block with the given code lengths (len(lit_lens) >= 257, len(dist_lens) >= 1).  The code-length code gives
    symbols 0 .. 12 four bits and 13 .. 18 five: a complete set."""
    w.bits(1 if final else 0, 1); w.bits(2, 2)
    w.bits(len(lit_lens) - 257, 5); w.bits(len(dist_lens) - 1, 5); w.bits(19 - 4, 4)
    cl_lens = [4] * 13 + [5] * 6
    for s in _CL_ORDER:
        w.bits(cl_lens[s], 3)
    cl = canonical(cl_lens)
    for s, eb, ev in code_length_symbols(list(lit_lens) + list(dist_lens)):
        w.code(*cl[s]); w.bits(ev, eb)
    _tokens(w, tokens, canonical(lit_lens), canonical(dist_lens))


def expand(tokens, before=b''):
    out = bytearray(before)
    for t in tokens:
        if isinstance(t, tuple):
            n, d = t
            for _ in range(n):
                out.append(out[-d])
        else:
            out.append(t)
    return bytes(out[len(before):])


def zlib_wrap(body, data, cmf=0x78, flg=0x9c, adler=None):
    return bytes([cmf, flg]) + bytes(body) + struct.pack('>I', zlib.adler32(data) if adler is None else adler)


def crafted_far(seed=5):
    """32768 random literals, then matches at the window's edge and self-overlapping ones: (stream, its 33394 bytes)."""
    rng = np.random.default_rng(seed)
    tokens = [int(b) for b in rng.integers(0, 256, 32768)] + [(258, 32768), (3, 32768), (258, 1), (100, 32768), (7, 3)]
    w = BitWriter()
    fixed_block(w, tokens)
    w.align()
    data = expand(tokens)
    return zlib_wrap(w.out, data), data


def crafted_near_edge(seed=6):
    """Matches whose distance is a little below 32768, longer than the gap: they read ring slots the same match writes."""
    rng = np.random.default_rng(seed)
    tokens = [int(b) for b in rng.integers(0, 256, 33000)]
    for n, d in ((258, 32767), (200, 32705), (258, 32768 - 64), (65, 32768 - 63), (258, 32700), (130, 64), (258, 63), (258, 65)):
        tokens += [(n, d), int(rng.integers(0, 256))]
    w = BitWriter()
    fixed_block(w, tokens)
    w.align()
    data = expand(tokens)
    return zlib_wrap(w.out, data), data


def crafted_sync_tail(n, m, seed=10):
    """A fixed block of n literals, an EMPTY stored block (a Z_SYNC_FLUSH point; this project's encoder leaves one every 32 KiB), then
    a last fixed block of m literals.  With n a multiple of 64 the stored header ends a batch of the device decoder, and with m small
    it lies in the stream's last input window: the bytes the header hands back then lie before a window staged for that batch."""
    rng = np.random.default_rng(seed + 7919 * n + m)
    head = [int(b) for b in rng.integers(0, 256, n)]
    tail = [int(b) for b in rng.integers(0, 256, m)]
    w = BitWriter()
    fixed_block(w, head, final=False)
    stored_block(w, b'', final=False)
    fixed_block(w, tail)
    w.align()
    data = bytes(head + tail)
    return zlib_wrap(w.out, data), data


SYNC_TAILS = [(n, m) for n in (64, 1216, 1984, 2048) for m in (400, 777, 1446, 1700)]


def crafted_too_far():
    """A match that reaches one byte before the stream's start."""
    tokens = [1, 2, 3, (3, 4)]
    w = BitWriter()
    fixed_block(w, tokens)
    w.align()
    return zlib_wrap(w.out, b'\x01\x02\x03\x00\x01\x02')


def _dyn_tokens(rng, lit_ok, dists):
    tokens = [int(s) for s in rng.choice(lit_ok, 400)]
    for k, d in enumerate(dists):
        tokens += [(3 + (37 * k) % 250, d)] + [int(s) for s in rng.choice(lit_ok, 5)]
    return tokens


def crafted_dynamic_single_distance(seed=7):
    """A dynamic block whose distance code set is ONE code of length 1 (symbol 4: distances 5 and 6)."""
    rng = np.random.default_rng(seed)
    lit = [8] * 226 + [9] * 60
    dist = [0, 0, 0, 0, 1]
    tokens = _dyn_tokens(rng, np.arange(256), [5, 6, 5, 6, 6])
    w = BitWriter()
    dynamic_block(w, tokens, lit, dist)
    w.align()
    data = expand(tokens)
    return zlib_wrap(w.out, data), data


def crafted_dynamic_repeat_16(seed=8):
    """Symbol 16 repeats the last literal / length length (9) into the first four distance lengths."""
    rng = np.random.default_rng(seed)
    lit = [8] * 226 + [9] * 60
    dist = [9, 9, 9, 9, 1, 2, 3, 4, 5, 6, 7]
    assert any(s == 16 for s, _, _ in code_length_symbols(lit + dist)[-9:])
    tokens = _dyn_tokens(rng, np.arange(256), [1, 2, 3, 4, 5, 9, 17, 30, 40])
    w = BitWriter()
    dynamic_block(w, tokens, lit, dist)
    w.align()
    data = expand(tokens)
    return zlib_wrap(w.out, data), data


def crafted_dynamic_repeat_18(seed=9):
    """Symbol 18 runs zeros from the last six literal / length lengths into the first eight distance lengths."""
    rng = np.random.default_rng(seed)
    lit = [8] * 232 + [9] * 48 + [0] * 6                # symbols 280 .. 285 (lengths 115 and up) have no code
    dist = [0] * 8 + [4] * 10 + [5] * 12                # distances 1 .. 16 have no code
    assert (18, 7, 3) in code_length_symbols(lit + dist)
    tokens = _dyn_tokens(rng, np.arange(256), [17, 100, 300, 33, 64, 65])
    tokens = [t if not isinstance(t, tuple) else (min(t[0], 100), t[1]) for t in tokens]
    w = BitWriter()
    dynamic_block(w, tokens, lit, dist)
    w.align()
    data = expand(tokens)
    return zlib_wrap(w.out, data), data


# ---- the corpus ----------------------------------------------------------------------------------------------------------------------
def _compress(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    return c.compress(data) + c.flush()


def delay_like(n_floats, dtype=np.float32, seed=1, shuffle=True):
    """Smooth delay-like values, byte-shuffled as HDF5's filter does."""
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, 40.0, n_floats)
    a = (2.3 + 0.2 * np.sin(x) + 0.05 * np.cos(7.3 * x) + 1e-4 * rng.standard_normal(n_floats)).astype(dtype)
    b = a.view(np.uint8)
    return (b.reshape(-1, a.itemsize).T.copy().tobytes() if shuffle else b.tobytes())


def text_like(n=60000, seed=2):
    rng = np.random.default_rng(seed)
    words = [b'delay', b'wet', b'hydro', b'zenith', b'ray', b'cube', b'level', b'aaaa', b'eeee']
    out = bytearray()
    while len(out) < n:
        out += words[int(rng.integers(0, len(words)))] + b' '
    return bytes(out[:n])


_CORPUS = None


def corpus():
    """[(name, stream)]: a fixed, seeded set; built once and shared."""
    global _CORPUS
    if _CORPUS is not None:
        return _CORPUS
    rng = np.random.default_rng(3)
    modes = [('l0', 0, zlib.Z_DEFAULT_STRATEGY), ('l1', 1, zlib.Z_DEFAULT_STRATEGY), ('l6', 6, zlib.Z_DEFAULT_STRATEGY), ('l9', 9, zlib.Z_DEFAULT_STRATEGY),
             ('fixed', 6, zlib.Z_FIXED), ('huff', 6, zlib.Z_HUFFMAN_ONLY)]
    out = [('empty-literal', bytes.fromhex('789c030000000001'))]
    small = {'empty': b'', 'one': b'\x5a', 'zeros': bytes(100000), 'text': text_like()}
    for name, data in small.items():
        for m, level, strat in modes:
            out.append((f'{name}-{m}', _compress(data, level, strat)))
    out.append(('random-l0', _compress(rng.integers(0, 256, 70000, dtype=np.uint8).tobytes(), 0)))
    rnd = rng.integers(0, 256, 70000, dtype=np.uint8).tobytes()     # two stored blocks, the first of LEN 65535 (zlib 1.2.11 stops at 65531)
    w = BitWriter(); stored_block(w, rnd[:65535], final=False); stored_block(w, rnd[65535:])
    out.append(('stored-65535', zlib_wrap(w.out, rnd)))
    big = delay_like(50000)
    for m, level, strat in (modes[1], modes[2], modes[4], modes[5]):
        out.append((f'delay-{m}', _compress(big, level, strat)))
    for name, mode in (('syncflush', zlib.Z_SYNC_FLUSH), ('fullflush', zlib.Z_FULL_FLUSH)):
        c = zlib.compressobj(6)
        t = text_like(30000, seed=4)
        out.append((name, c.compress(t[:17000]) + c.flush(mode) + c.compress(t[17000:]) + c.flush()))
    out.append(('crafted-far', crafted_far()[0]))
    out.append(('crafted-near-edge', crafted_near_edge()[0]))
    out.append(('dyn-single-distance', crafted_dynamic_single_distance()[0]))
    out.append(('dyn-repeat-16', crafted_dynamic_repeat_16()[0]))
    out.append(('dyn-repeat-18', crafted_dynamic_repeat_18()[0]))
    for n, m in SYNC_TAILS:
        out.append((f'sync-tail-{n}-{m}', crafted_sync_tail(n, m)[0]))
    _CORPUS = out
    return out


def judge(stream, cap=None):
    """zlib's verdict: the decoded bytes when zlib.decompress accepts the stream (and they fit `cap`), else None."""
    try:
        data = zlib.decompress(bytes(stream))
    except zlib.error:
        return None
    if cap is not None and len(data) > cap:
        return None
    return data


def damaged(name, stream):
    """[(label, bytes)]: the stream truncated at 16 evenly spaced lengths and with one flipped bit at 32 seeded positions."""
    out = []
    n = len(stream)
    for k in range(16):
        cut = n * k // 16
        out.append((f'{name}/cut{cut}', stream[:cut]))
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    for pos in rng.integers(0, 8 * n, 32):
        b = bytearray(stream)
        b[int(pos) >> 3] ^= 1 << (int(pos) & 7)
        out.append((f'{name}/flip{int(pos)}', bytes(b)))
    return out


def specials():
    """[(label, bytes)]: the damage that needs crafting."""
    good = _compress(text_like(3000, seed=11), 6)
    w = BitWriter(); fixed_block(w, [65, 66, 67], btype=3); w.align()
    ws = BitWriter(); stored_block(ws, b'hello world', nlen=0x1234)
    return [('preset-dictionary', bytes([0x78, 0xbb]) + good[2:]),                       # FDICT set, FCHECK right (0x78bb % 31 == 0)
            ('block-type-3', zlib_wrap(w.out, b'ABC')),
            ('len-nlen', zlib_wrap(ws.out, b'hello world')),
            ('too-far-back', crafted_too_far()),
            ('wrong-adler', good[:-4] + struct.pack('>I', (zlib.adler32(text_like(3000, seed=11)) + 1) & 0xffffffff)),
            ('bad-method', bytes([0x79, 0x80 + 31 - (0x7980 % 31)]) + good[2:]),                  # CM = 9, FCHECK right
            ('trailing-bytes', good + b'\x01\x02\x03\x04')]


def pack_probe_file(path, streams, caps):
    """The input file of tools/probes/inflate_host_check: u32 count, then per stream u32 bytes, u32 capacity, the bytes."""
    with open(path, 'wb') as f:
        f.write(struct.pack('<I', len(streams)))
        for s, cap in zip(streams, caps):
            f.write(struct.pack('<II', len(s), int(cap)))
            f.write(bytes(s))
