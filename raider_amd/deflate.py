"""zlib streams written on the GPU (rdr_deflate_encode) and read back there (rdr_inflate_decode), the chunk cutter of the NetCDF-4
writer (rdr_h5_chunks) and its inverse (rdr_h5_unchunk).

The encoder turns independent byte ranges of one buffer into complete zlib streams, one wave per 32 KiB sub-block, with fixed-Huffman
and stored blocks; with tables='dynamic' every sub-block is the smallest of a stored, a fixed-Huffman and a
dynamic-Huffman block.  NumPy arrays go up and come back in one transfer each; device tensors stay where they are.
There is no CPU fallback: the writers that want host zlib call zlib."""
import numpy as np

from . import _lib as L


def bound(n):
    """The largest stream the encoder makes of `n` bytes (<= n + n // 2048 + 32)."""
    return int(L.load().rdr_deflate_bound(int(n)))


def _is_tensor(a):
    return type(a).__module__.split('.')[0] == 'torch'


def require_gpu(what):
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError(f'{what} runs on the GPU; no GPU is visible and there is no CPU fallback')


TABLES = {'fixed': L.RDR_DEFL_FIXED, 'dynamic': L.RDR_DEFL_DYNAMIC}
_last_counts = (0, 0, 0)
_last_pieces = np.zeros(0, dtype=np.int64)
FLUSH_MARKER = b'\x00\x00\xff\xff'


def tables_mode(tables):
    """The library's value of the `tables` keyword; anything but 'fixed' and 'dynamic' is a ValueError."""
    if tables not in TABLES:
        raise ValueError(f"tables must be 'fixed' or 'dynamic', not {tables!r}")
    return TABLES[tables]


def last_block_counts():
    """(stored, fixed, dynamic): the sub-blocks of each kind in the last deflate_segments call of this process."""
    return _last_counts


class _Route:
    """How one buffer goes through the library, NumPy array or device tensor alike: its C-contiguous form (`array`), that as bytes
    (`bytes`), the `loc` that goes with it, the context - on torch's current stream for a tensor - and buffers of the same kind (`new`).
    A tensor that is not on the GPU (or not contiguous, unless `make_contiguous`) is a TypeError of `need`; an array without a GPU
    is require_gpu's RuntimeError."""

    def __init__(self, buf, who, entry, need='a tensor must be contiguous and live on the GPU', make_contiguous=False):
        self.tensor = _is_tensor(buf)
        if self.tensor:
            import torch
            if not buf.is_cuda or not (make_contiguous or buf.is_contiguous()):
                raise TypeError(f'{who}: {need}')
            self.array = buf.contiguous()
            self.bytes = self.array.reshape(-1).view(torch.uint8)
            self.loc = L.RDR_DEVICE
        else:
            require_gpu(f'{who} ({entry})')
            self.array = np.ascontiguousarray(buf)
            self.bytes = self.array.reshape(-1).view(np.uint8)
            self.loc = L.RDR_HOST
        self.nbytes = self.bytes.numel() if self.tensor else self.bytes.size
        self.ctx = L.Context.default()
        if self.tensor:
            self.ctx.adopt_torch_stream(self.bytes)

    def new(self, n, dtype=np.uint8, fill=None):
        """`n` elements of `dtype` where the buffer lives: filled with `fill`, or uninitialised.  (Zeros come from zeros(): a memset on
        the device, untouched pages on the host.)"""
        if self.tensor:
            import torch
            kw = dict(dtype=getattr(torch, np.dtype(dtype).name), device=self.array.device)
            return torch.empty(n, **kw) if fill is None else torch.zeros(n, **kw) if fill == 0 else torch.full((n,), fill, **kw)
        return np.empty(n, dtype=dtype) if fill is None else np.zeros(n, dtype=dtype) if fill == 0 else np.full(n, fill, dtype=dtype)

    def owns(self, out):
        """`out` is a contiguous uint8 buffer of the buffer's own kind."""
        if self.tensor:
            import torch
            return _is_tensor(out) and out.dtype == torch.uint8 and out.is_cuda and out.is_contiguous()
        return isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous


def deflate_segments(buf, offsets, sizes, tables='fixed'):
    """(packed, out_offsets): the byte ranges buf[offsets[i] : offsets[i] + sizes[i]] as zlib streams packed back to back; stream i is
    packed[out_offsets[i] : out_offsets[i + 1]].  buf: a C-contiguous NumPy array or device tensor of any element type (taken as bytes);
    packed is a uint8 array / tensor of the same kind, out_offsets an int64 NumPy array of len(sizes) + 1.  tables: 'fixed' (stored and
    fixed-Huffman blocks) or 'dynamic' (dynamic-Huffman blocks too, wherever they are the smallest)."""
    global _last_counts
    mode = tables_mode(tables)
    so = np.ascontiguousarray(offsets, dtype=np.int64).ravel()
    sb = np.ascontiguousarray(sizes, dtype=np.int64).ravel()
    if so.size != sb.size:
        raise ValueError('offsets and sizes differ in length')
    if so.size == 0:
        raise ValueError('deflate_segments: no segments')
    if np.any(sb <= 0):
        raise ValueError('deflate_segments: every segment needs at least one byte')
    cap = sum(bound(int(v)) * int(c) for v, c in zip(*np.unique(sb, return_counts=True)))
    oo = np.zeros(so.size + 1, dtype=np.int64)
    kinds = np.zeros(3, dtype=np.int64)
    r = _Route(buf, 'deflate_segments', 'rdr_deflate_encode')
    out = r.new(cap)
    L.check(r.ctx.lib.rdr_deflate_encode_tables(r.ctx.handle, L.ptr(r.bytes), r.nbytes, L.ptr(so), L.ptr(sb), so.size, mode, L.ptr(out), cap, L.ptr(oo), L.ptr(kinds),
                                                r.loc), r.ctx.handle)
    _last_counts = tuple(int(k) for k in kinds)
    return out[:int(oo[-1])], oo


def chunk_grid(shape, chunk):
    """Chunks along every axis: ceil(shape / chunk)."""
    return tuple(-(-int(s) // int(c)) for s, c in zip(shape, chunk))


def h5_chunks(array, chunk, fill, shuffle=True):
    """`array` (NumPy or device tensor, at most 4-D) cut into full-size chunks in row-major chunk order, edge chunks padded with `fill`,
    each chunk byte-shuffled as HDF5's shuffle filter does when `shuffle`.  Returns a uint8 array / tensor of
    n_chunks * prod(chunk) * itemsize bytes: chunk k is bytes [k * chunk_bytes, (k + 1) * chunk_bytes)."""
    r = _Route(array, 'h5_chunks', 'rdr_h5_chunks', need='a tensor must live on the GPU', make_contiguous=True)
    dt = np.dtype(str(r.array.dtype).replace('torch.', '')) if r.tensor else r.array.dtype
    shape = tuple(r.array.shape)
    chunk = tuple(int(c) for c in chunk)
    if len(chunk) != len(shape) or not 1 <= len(shape) <= 4:
        raise ValueError(f'h5_chunks: chunk {chunk} does not fit an array of shape {shape} (1 to 4 axes)')
    if any(c <= 0 for c in chunk) or any(s <= 0 for s in shape):
        raise ValueError('h5_chunks: shape and chunk sizes must be positive')
    nbytes = int(np.prod(chunk_grid(shape, chunk), dtype=np.int64) * np.prod(chunk, dtype=np.int64)) * dt.itemsize
    fv = np.array([fill], dtype=dt)
    sh, ck = np.array(shape, dtype=np.int64), np.array(chunk, dtype=np.int64)
    out = r.new(nbytes)
    L.check(r.ctx.lib.rdr_h5_chunks(r.ctx.handle, L.ptr(r.bytes), dt.itemsize, len(shape), L.ptr(sh), L.ptr(ck), L.ptr(fv), int(bool(shuffle)), L.ptr(out), r.loc),
            r.ctx.handle)
    return out


def h5_chunks_host(array, chunk, fill, shuffle=True):
    """NumPy restatement of rdr_h5_chunks (what the tests compare it with, and what a caller without a GPU feeds to zlib)."""
    a = np.ascontiguousarray(array)
    chunk = tuple(int(c) for c in chunk)
    grid = chunk_grid(a.shape, chunk)
    padded = np.full(tuple(g * c for g, c in zip(grid, chunk)), fill, dtype=a.dtype)
    padded[tuple(slice(0, s) for s in a.shape)] = a
    out = []
    for idx in np.ndindex(*grid):
        blk = np.ascontiguousarray(padded[tuple(slice(i * c, (i + 1) * c) for i, c in zip(idx, chunk))])
        b = blk.reshape(-1).view(np.uint8)
        if shuffle:
            b = b.reshape(-1, a.dtype.itemsize).T
        out.append(np.ascontiguousarray(b).reshape(-1))
    return np.concatenate(out)


def compress_chunks(array, chunk, fill, shuffle=True, tables='fixed'):
    """(packed bytes as a NumPy uint8 array, offsets): `array` cut into chunks, shuffled and deflated on the device - what
    h5write takes as a chunked variable's data.  One download, of the packed streams.  tables: as deflate_segments."""
    tables_mode(tables)
    raw = h5_chunks(array, chunk, fill, shuffle)
    n = int(np.prod(chunk_grid(tuple(array.shape), chunk), dtype=np.int64))
    cb = (raw.numel() if _is_tensor(raw) else raw.size) // n
    packed, oo = deflate_segments(raw, np.arange(n, dtype=np.int64) * cb, np.full(n, cb, dtype=np.int64), tables=tables)
    if _is_tensor(packed):
        packed = packed.cpu().numpy()
    return packed, oo


# ---- the way back: zlib streams decoded on the device (rdr_inflate_decode), chunks put back into an array (rdr_h5_unchunk) -----------
def inflate_mode(inflate):
    """The `inflate` keyword of the readers, validated: 'auto', 'host' or 'device'."""
    if inflate not in ('auto', 'host', 'device'):
        raise ValueError(f"inflate must be 'auto', 'host' or 'device', not {inflate!r}")
    return inflate


def last_pieces():
    """int64 array, one entry per stream of the last inflate_segments(..., split=True) call of this process: the pieces of the stream
    that separate waves decoded; 1: the stream went through the serial kernel."""
    return _last_pieces


def flush_points(buf):
    """The occurrences of the byte-aligned empty stored block's LEN / NLEN words (00 00 FF FF: what Z_SYNC_FLUSH, Z_FULL_FLUSH and this
    package's encoder leave behind) in a host bytes-like.  Its only use is the readers' choice of a route: the split decoder can cut a
    stream at no other place."""
    if isinstance(buf, np.ndarray):
        buf = np.ascontiguousarray(buf).reshape(-1).view(np.uint8).tobytes()       # (bytes.count is a memchr-speed search)
    elif not isinstance(buf, (bytes, bytearray)):
        buf = bytes(buf)
    return buf.count(FLUSH_MARKER)


def inflate_segments(buf, offsets, sizes, out_sizes, out_stride=None, out=None, split=False):
    """(out, status, produced): the zlib streams buf[offsets[i] : offsets[i] + sizes[i]] decoded on the device, stream i into
    out[i * out_stride : i * out_stride + out_sizes[i]].  buf: a C-contiguous NumPy array or device tensor (taken as bytes); out is a
    uint8 array / tensor of the same kind of len(sizes) * out_stride bytes (out_stride: max(out_sizes) rounded up to 16 when None),
    status an int32 and produced an int64 array / tensor.  status[i] is one of RDR_INFL_*: 0 exactly when zlib.decompress accepts the
    stream and its output fits the slot.  `out`: an existing buffer to decode into - slot bytes a stream does not reach keep their value
    (a new buffer is zeroed).  One transfer each way for NumPy, none for tensors.
    split: long streams are cut at their flush points and decoded by many waves (rdr_inflate_decode_split); out, status and produced are
    byte for byte those of split=False, last_pieces() tells how many pieces each stream was decoded in, and the call synchronises."""
    global _last_pieces
    so = np.ascontiguousarray(offsets, dtype=np.int64).ravel()
    sb = np.ascontiguousarray(sizes, dtype=np.int64).ravel()
    cap = np.ascontiguousarray(out_sizes, dtype=np.int64).ravel()
    n = so.size
    if sb.size != n or cap.size != n:
        raise ValueError('offsets, sizes and out_sizes differ in length')
    if n == 0:
        raise ValueError('inflate_segments: no segments')
    if out_stride is None:
        out_stride = max(16, (int(cap.max()) + 15) // 16 * 16)
    out_stride = int(out_stride)
    r = _Route(buf, 'inflate_segments', 'rdr_inflate_decode')
    if out is None:
        out = r.new(n * out_stride, fill=0)
    elif not r.owns(out) or (out.numel() if r.tensor else out.size) < n * out_stride:
        kind = 'contiguous uint8 tensor on the GPU' if r.tensor else 'C-contiguous uint8 array'
        raise TypeError(f'inflate_segments: out must be a {kind} of {n} slots of {out_stride} bytes')
    status = r.new(n, np.int32, fill=-1)
    produced = r.new(n, np.int64, fill=0)
    if split:
        pieces = np.zeros(n, dtype=np.int64)
        L.check(r.ctx.lib.rdr_inflate_decode_split(r.ctx.handle, L.ptr(r.bytes), r.nbytes, L.ptr(so), L.ptr(sb), n, L.ptr(cap), L.ptr(out), out_stride, L.ptr(status),
                                                   L.ptr(produced), L.ptr(pieces), r.loc), r.ctx.handle)
        _last_pieces = pieces
        return out, status, produced
    L.check(r.ctx.lib.rdr_inflate_decode(r.ctx.handle, L.ptr(r.bytes), r.nbytes, L.ptr(so), L.ptr(sb), n, L.ptr(cap), L.ptr(out), out_stride, L.ptr(status),
                                         L.ptr(produced), r.loc), r.ctx.handle)
    return out, status, produced


def h5_unchunk(chunks, chunk_stride, chunk_index, dtype, shape, chunk, shuffle=True, swap=False):
    """The inverse of h5_chunks: decoded chunks (uint8 array / device tensor, chunk k at k * chunk_stride, its row-major index in the
    chunk grid chunk_index[k]) -> the C-ordered array / tensor of `shape` and `dtype` (native byte order; `swap`: the chunks hold
    the other one).  Elements of chunks that are not listed are 0."""
    dt = np.dtype(dtype).newbyteorder('=')
    shape = tuple(int(s) for s in shape)
    chunk = tuple(int(c) for c in chunk)
    idx = np.ascontiguousarray(chunk_index, dtype=np.int64).ravel()
    if len(chunk) != len(shape) or not 1 <= len(shape) <= 4:
        raise ValueError(f'h5_unchunk: chunk {chunk} does not fit an array of shape {shape} (1 to 4 axes)')
    if idx.size == 0:
        raise ValueError('h5_unchunk: no chunks')
    sh, ck = np.array(shape, dtype=np.int64), np.array(chunk, dtype=np.int64)
    nbytes = int(np.prod(sh)) * dt.itemsize
    r = _Route(chunks, 'h5_unchunk', 'rdr_h5_unchunk', need='a tensor must be contiguous, live on the GPU and hold every chunk')
    if r.nbytes < idx.size * int(chunk_stride):
        if r.tensor:
            raise TypeError('h5_unchunk: a tensor must be contiguous, live on the GPU and hold every chunk')
        raise ValueError('h5_unchunk: the buffer does not hold every chunk')
    out = r.new(nbytes)
    L.check(r.ctx.lib.rdr_h5_unchunk(r.ctx.handle, L.ptr(r.bytes), int(chunk_stride), L.ptr(idx), idx.size, dt.itemsize, len(shape), L.ptr(sh), L.ptr(ck),
                                     int(bool(shuffle)), int(bool(swap)), L.ptr(out), r.loc), r.ctx.handle)
    if r.tensor:
        import torch
        if not hasattr(torch, dt.name):
            raise TypeError(f'h5_unchunk: this torch build has no tensor type for {dt.name}')
        return out.view(getattr(torch, dt.name)).reshape(shape)
    return out.view(dt).reshape(shape)


def h5_unchunk_host(chunks, chunk_stride, chunk_index, dtype, shape, chunk, shuffle=True, swap=False):
    """NumPy restatement of rdr_h5_unchunk (what the tests compare it with)."""
    dt = np.dtype(dtype).newbyteorder('=')
    src_dt = dt.newbyteorder('S') if swap else dt
    shape = tuple(int(s) for s in shape)
    chunk = tuple(int(c) for c in chunk)
    grid = chunk_grid(shape, chunk)
    n = int(np.prod(chunk, dtype=np.int64))
    raw = np.ascontiguousarray(chunks).reshape(-1).view(np.uint8)
    out = np.zeros(shape, dtype=dt)
    for k, ci in enumerate(np.asarray(chunk_index, dtype=np.int64).ravel()):
        b = raw[k * int(chunk_stride):k * int(chunk_stride) + n * dt.itemsize]
        if shuffle:
            b = b.reshape(dt.itemsize, n).T
        blk = np.ascontiguousarray(b).reshape(-1).view(src_dt).reshape(chunk)
        offs = tuple(int(i) * c for i, c in zip(np.unravel_index(int(ci), grid), chunk))
        sel = tuple(slice(o, min(o + c, s)) for o, c, s in zip(offs, chunk, shape))
        out[sel] = blk[tuple(slice(0, s.stop - s.start) for s in sel)]
    return out
