"""A small read-only HDF5 / NetCDF-4 reader (pure Python + NumPy).

The reference reads and writes its processed weather cubes and delay cubes as NetCDF-4 = HDF5
(models/weatherModel.py:659-724, delay.py:329-401) through xarray + netCDF4/h5py.  None of those libraries is part of
this build's environment, and the delay path only needs to pull a handful of dense numeric arrays (x, y, z, wet, hydro,
wet_total, hydro_total) and a few attributes (the `proj` variable's crs_wkt) out of such a file.  This module implements
exactly that subset of the published HDF5 file format (HDF5 File Format Specification v3):

  * superblock versions 0-3; version-2 object headers (what libhdf5 >= 1.8 writes for NetCDF-4 files) and version-1
    object headers; header continuation blocks;
  * groups: compact links (link messages), dense links (fractal heap, objects located through the version-2 B-tree name index - a heap
    keeps the bytes of removed or renamed entries, only the index says which objects are live) and old-style symbol tables
    (B-tree v1 + local heap);
  * datasets: contiguous, compact, and chunked - version-3 layout with its B-tree v1 chunk index, version-4 layout with a
    single-chunk, implicit or (paged) fixed-array index - with the deflate, shuffle and fletcher32 filters; fixed-point and IEEE
    floating-point element types of either byte order;
  * attributes: compact (attribute messages) and dense (fractal heap through its version-2 B-tree name index), numeric or string
    (fixed or variable length).

Anything else (compound / reference types, the extensible-array and B-tree v2 chunk indices that datasets with unlimited dimensions get
under the >= v110 format bounds, external storage, ...) raises
`UnsupportedHDF5Feature` - loudly, never a silent wrong answer.

Test status: exercised on the NetCDF-4 files the reference's test suite holds (written by netCDF4 4.9 / libhdf5 1.12-1.14:
superblock v2, v2 object headers, dense links and attributes, contiguous datasets, variable-length string attributes) -
tests/test_ref_files.py checks what is read against physics identities and against the reference's own results.  The
version-0 superblock and symbol-table groups are exercised by the files of raider_amd.h5write (tests/test_h5write.py), the
chunked / deflate / shuffle / fletcher32 branches by libhdf5's own re-layouts of those files and of a reference cube (h5repack
1.10.6 of the build image, same test): arrays come back bit for bit.  tests/test_h5py_cross.py: files written by h5py (libhdf5
through an independent binding, when the image has one) under five file-format bounds - every layout, element type, byte order and
attribute storage above - are read back bit for bit or refused by name (an unlimited dimension under the >= v110 bounds), and
h5py reads what raider_amd.h5write writes.
"""
import zlib

import numpy as np

UNDEF = 0xFFFFFFFFFFFFFFFF


class UnsupportedHDF5Feature(NotImplementedError):
    pass


# Dataset.read_device(inflate='auto'): chunks from which the device route is taken.  Measured (tools/bench_inflate.py,
# profiles/r24_inflate.json) on 20 x 1000 x 1000 cubes: float32 in 16 chunks 665 ms on the device against 253 ms through zlib, in 64
# chunks 178 ms against 252 ms; float64 in 16 chunks 319 ms against 394 ms, in 64 chunks 94 ms against 390 ms.
_INFLATE_MIN_CHUNKS = 64
# Fewer chunks, but long ones that the split decoder cuts at their flush points: chunks + flush points from which the device route is
# taken.  Measured (tools/bench_inflate_split.py, profiles/r28_inflate_split.json): a 20 x 150 x 150 float32 cube in nine device-written
# chunks (63 units) 31.5 ms on the device against 6.3 ms through zlib - not ahead, two passes over one 32 KiB piece on one lane are a
# floor of about 30 ms; 20 x 1000 x 1000 cubes in 16 chunks (2400 - 4700 units) 86 against 437 ms (float32), 54 against 767 ms
# (float64).  Between them the crossing is the rasters' (tifflite._INFLATE_MIN_PIECES: not ahead at 264 units, ahead from 528), the same
# kernels on the same kind of stream.  One chunk alone stays on the host.  Chunks whose flush points keep the history (Z_SYNC_FLUSH) are
# not told apart before the measure pass and are slower on this route (72 units: 31.4 against 6.5 ms); the HDF5 library writes none.
_INFLATE_MIN_PIECES = 512


def _u(b, off, n):
    return int.from_bytes(b[off:off + n], 'little')


class _Datatype:
    def __init__(self, buf, off=0):
        cv = buf[off]
        self.cls = cv & 0x0F
        self.version = cv >> 4
        bits = buf[off + 1:off + 4]
        self.size = _u(buf, off + 4, 4)
        self.bits = bits
        self.base = None
        self.vlen_string = False
        p = off + 8
        if self.cls == 0:      # fixed point
            self.nbytes = p + 4 - off
            order = '>' if bits[0] & 1 else '<'
            signed = bool(bits[0] & 0x08)
            self.dtype = np.dtype(f'{order}{"i" if signed else "u"}{self.size}')
        elif self.cls == 1:    # floating point
            self.nbytes = p + 12 - off
            order = '>' if bits[0] & 1 else '<'
            if self.size not in (2, 4, 8):
                raise UnsupportedHDF5Feature(f'{self.size}-byte floating point type')
            self.dtype = np.dtype(f'{order}f{self.size}')
        elif self.cls == 3:    # fixed-length string
            self.nbytes = p - off
            self.dtype = np.dtype(f'S{self.size}')
        elif self.cls == 9:    # variable length
            self.base = _Datatype(buf, p)
            self.nbytes = None if self.base.nbytes is None else p + self.base.nbytes - off
            self.vlen_string = (bits[0] & 0x0F) == 1
            self.dtype = None
        else:
            self.nbytes = None
            self.dtype = None


def _dataspace(buf):
    ver = buf[0]
    rank = buf[1]
    flags = buf[2]
    if ver == 1:
        p = 8
    elif ver == 2:
        if buf[3] == 2:          # null dataspace
            return None
        p = 4
    else:
        raise UnsupportedHDF5Feature(f'dataspace message version {ver}')
    dims = tuple(_u(buf, p + 8 * i, 8) for i in range(rank))
    return dims


class Dataset:
    def __init__(self, f, name, msgs):
        self.file, self.name = f, name
        self.shape = None
        self.dt = None
        self.layout = None
        self.filters = []
        self._attr_msgs = []
        self._attr_info = None
        for t, body in msgs:
            if t == 0x01:
                self.shape = _dataspace(body)
            elif t == 0x03:
                self.dt = _Datatype(body)
            elif t == 0x08:
                self.layout = body
            elif t == 0x0B:
                self.filters = _filters(body)
            elif t == 0x0C:
                self._attr_msgs.append(body)
            elif t == 0x15:
                self._attr_info = body
        self.dtype = self.dt.dtype if self.dt is not None else None

    # -- data ---------------------------------------------------------------------------------------------------
    def __getitem__(self, key):
        return self.read()[key]

    def raw(self):
        """Zero-copy view of a CONTIGUOUS dataset in the file's own byte order (a read-only array over the mapped file), or None when
        the layout needs decoding (compact / chunked / filtered / never written): the caller then takes read()."""
        if self.dtype is None or self.dtype.kind not in 'fiu':
            return None
        lay = self.layout
        if lay[0] not in (3, 4) or lay[1] != 1:
            return None
        shape = self.shape if self.shape is not None else ()
        count = int(np.prod(shape)) if shape else 1
        addr = _u(lay, 2, 8)
        if addr == UNDEF:
            return None
        f = self.file
        return np.frombuffer(f.buf, dtype=self.dtype, count=count, offset=f.base + addr).reshape(shape)

    def read(self):
        if self.dtype is None or self.dtype.kind == 'S':
            raise UnsupportedHDF5Feature(f'dataset {self.name}: element type class {self.dt.cls} is not numeric')
        f, lay = self.file, self.layout
        shape = self.shape if self.shape is not None else ()
        count = int(np.prod(shape)) if shape else 1
        ver = lay[0]
        if ver not in (3, 4):
            raise UnsupportedHDF5Feature(f'data layout message version {ver}')
        cls = lay[1]
        if cls == 0:       # compact
            size = _u(lay, 2, 2)
            raw = lay[4:4 + size]
            return np.frombuffer(raw, dtype=self.dtype, count=count).reshape(shape).astype(self.dtype.newbyteorder('='))
        if cls == 1:       # contiguous
            addr, size = _u(lay, 2, 8), _u(lay, 10, 8)
            if addr == UNDEF:      # never written: fill value (0)
                return np.zeros(shape, dtype=self.dtype.newbyteorder('='))
            raw = f.buf[f.base + addr:f.base + addr + count * self.dtype.itemsize]
            return np.frombuffer(raw, dtype=self.dtype, count=count).reshape(shape).astype(self.dtype.newbyteorder('='))
        if cls == 2:
            return self._read_chunked(lay, shape)
        raise UnsupportedHDF5Feature(f'data layout class {cls}')

    def _chunks(self, lay, shape):
        """(chunk shape, iterator of (offsets, stored size, filter mask, address, may be filtered)) of a chunked dataset: the version-3
        layout with its version-1 B-tree, or a version-4 layout with a single-chunk, implicit or fixed-array index (what libhdf5 picks
        for fixed-shape datasets under the >= v110 format bounds)."""
        f = self.file
        es = self.dtype.itemsize
        if lay[0] == 3:
            nd = lay[2] - 1
            btree = _u(lay, 3, 8)
            chunk = tuple(_u(lay, 11 + 4 * i, 4) for i in range(nd))
            return chunk, (() if btree == UNDEF else ((o, sz, m, a, True) for o, sz, m, a in f._chunk_btree(btree, nd)))
        flags, nd1, enc = lay[2], lay[3], lay[4]
        nd = nd1 - 1
        chunk = tuple(_u(lay, 5 + enc * i, enc) for i in range(nd))
        p = 5 + enc * nd1
        itype = lay[p]; p += 1
        grid = [-(-s // c) for s, c in zip(shape, chunk)]
        nchunks = int(np.prod(grid)) if grid else 1
        plain = int(np.prod(chunk)) * es

        def offsets(i):
            idx = np.unravel_index(i, grid) if grid else ()
            return tuple(int(k) * c for k, c in zip(idx, chunk))

        partial = lambda offs: any(o + c > s for o, c, s in zip(offs, chunk, shape))
        edge_plain = bool(flags & 1)             # DONT_FILTER_PARTIAL_BOUND_CHUNKS
        if itype == 1:                           # single chunk
            size, mask = plain, 0
            if flags & 2:
                size, mask = _u(lay, p, 8), _u(lay, p + 8, 4); p += 12
            addr = _u(lay, p, 8)
            return chunk, (() if addr == UNDEF else [(offsets(0), size, mask, addr, bool(flags & 2))])
        if itype == 2:                           # implicit: every chunk allocated, back to back, never filtered
            addr = _u(lay, p, 8)
            return chunk, (() if addr == UNDEF else ((offsets(i), plain, 0, addr + i * plain, False) for i in range(nchunks)))
        if itype == 3:                           # fixed array
            addr = _u(lay, p + 1, 8)
            if addr == UNDEF:
                return chunk, ()
            b = f.buf
            a = f.base + addr
            if b[a:a + 4] != b'FAHD':
                raise ValueError('corrupt fixed-array header')
            client, esize, pbits = b[a + 5], b[a + 6], b[a + 7]
            nel, dblk = _u(b, a + 8, 8), _u(b, a + 16, 8)
            if dblk == UNDEF:
                return chunk, ()
            q = f.base + dblk
            if b[q:q + 4] != b'FADB':
                raise ValueError('corrupt fixed-array data block')
            q += 6 + 8
            per_page = 1 << pbits
            pages = []                           # (file position of the page's first element, number of elements)
            if nel > per_page:
                npages = -(-nel // per_page)
                bitmap = b[q:q + (npages + 7) // 8]
                q += (npages + 7) // 8 + 4
                for pg in range(npages):
                    cnt = min(per_page, nel - pg * per_page)
                    init = (bitmap[pg // 8] >> (7 - pg % 8)) & 1
                    pages.append((q if init else None, cnt))
                    q += cnt * esize + 4
            else:
                pages.append((q, nel))

            def elements():
                i = 0
                for pos, cnt in pages:
                    for k in range(cnt):
                        if pos is not None and i < nchunks:
                            e = pos + k * esize
                            caddr = _u(b, e, 8)
                            if caddr != UNDEF:
                                offs = offsets(i)
                                if client == 1:
                                    size, mask = _u(b, e + 8, esize - 12), _u(b, e + esize - 4, 4)
                                    yield offs, size, mask, caddr, not (edge_plain and partial(offs))
                                else:
                                    yield offs, plain, 0, caddr, False
                        i += 1
            return chunk, elements()
        raise UnsupportedHDF5Feature({4: 'version-4 chunked layout with an extensible-array chunk index (unlimited dimension)',
                                      5: 'version-4 chunked layout with a version-2 B-tree chunk index (several unlimited dimensions)'}
                                     .get(itype, f'version-4 chunked layout, chunk index type {itype}'))

    def _read_chunked(self, lay, shape):
        f = self.file
        chunk, entries = self._chunks(lay, shape)
        out = np.zeros(shape, dtype=self.dtype.newbyteorder('='))
        for offs, size, mask, addr, filtered in entries:
            raw = f.buf[f.base + addr:f.base + addr + size]
            for i, (fid, _) in reversed(list(enumerate(self.filters))):
                if not filtered or mask & (1 << i):
                    continue
                if fid == 1:
                    raw = zlib.decompress(raw)
                elif fid == 2:
                    a = np.frombuffer(raw, dtype=np.uint8)
                    n = a.size // self.dtype.itemsize
                    raw = a[:n * self.dtype.itemsize].reshape(self.dtype.itemsize, n).T.tobytes()
                elif fid == 3:     # fletcher32: drop the trailing checksum
                    raw = raw[:-4]
                else:
                    raise UnsupportedHDF5Feature(f'filter id {fid}')
            block = np.frombuffer(raw, dtype=self.dtype, count=int(np.prod(chunk))).reshape(chunk)
            sel = tuple(slice(o, min(o + c, s)) for o, c, s in zip(offs, chunk, shape))
            out[sel] = block[tuple(slice(0, s.stop - s.start) for s in sel)]
        return out

    def read_device(self, device=None, inflate='auto'):
        """The dataset as a device tensor in native byte order, its chunks inflated (rdr_inflate_decode_split) and put together
        (rdr_h5_unchunk) on the GPU - or None when the dataset is not a candidate, and the caller takes read().  Candidates: a chunked
        layout whose index _chunks() reads, a float or integer type of 1 / 2 / 4 / 8 bytes, the filter pipeline [shuffle,] deflate
        [, fletcher32] in that order, every chunk filtered (filter mask 0).  inflate: 'device', 'host' (always None) or 'auto' (the
        device from _INFLATE_MIN_CHUNKS chunks on, or from two chunks on when they and the flush points inside them, deflate.flush_points,
        together reach _INFLATE_MIN_PIECES).  A chunk the device does not accept is inflated by zlib on the host and patched
        in: a damaged chunk raises what read() raises.  The fletcher32 checksum is dropped unverified, as read() drops it."""
        from .deflate import inflate_mode, inflate_segments, flush_points, h5_unchunk
        inflate = inflate_mode(inflate)
        if inflate == 'host' or self.dtype is None or self.dtype.kind not in 'fiu' or self.dtype.itemsize not in (1, 2, 4, 8):
            return None
        lay, shape = self.layout, self.shape
        if lay[0] not in (3, 4) or lay[1] != 2 or not shape or not 1 <= len(shape) <= 4:
            return None
        fids = [fid for fid, _ in self.filters]
        if fids not in ([1], [2, 1], [1, 3], [2, 1, 3]):
            return None
        try:
            chunk, entries = self._chunks(lay, shape)
            entries = list(entries)
        except UnsupportedHDF5Feature:
            return None
        if not entries or any(mask != 0 or not filtered for _, _, mask, _, filtered in entries):
            return None
        import torch
        if not hasattr(torch, self.dtype.newbyteorder('=').name):
            return None                                               # (an unsigned type this torch build has no tensor for)
        f = self.file
        es = self.dtype.itemsize
        tail = 4 if 3 in fids else 0                                  # fletcher32's checksum behind the deflate stream
        grid = [-(-s // c) for s, c in zip(shape, chunk)]
        offsets = np.array([f.base + addr for _, _, _, addr, _ in entries], dtype=np.int64)
        sizes = np.array([size - tail for _, size, _, _, _ in entries], dtype=np.int64)
        index = np.array([np.ravel_multi_index([o // c for o, c in zip(offs, chunk)], grid) for offs, _, _, _, _ in entries], dtype=np.int64)
        buf = np.frombuffer(f.buf, dtype=np.uint8)
        if np.any(sizes <= 0) or np.any(offsets < 0) or np.any(offsets + sizes > buf.size):
            return None                                               # (read() says what is wrong with the file)
        if inflate == 'auto' and len(entries) < _INFLATE_MIN_CHUNKS:
            # a long chunk is decoded in as many pieces as it has flush points (rdr_inflate_decode_split): they count as chunks do.  One
            # chunk alone stays on the host (measured, not ahead), and without a visible GPU the caller's read() serves the file
            if len(entries) < 2 or not torch.cuda.is_available():
                return None
            marks = sum(flush_points(bytes(buf[o:o + n])) for o, n in zip(offsets, sizes))
            if len(entries) + marks < _INFLATE_MIN_PIECES:
                return None
        plain = int(np.prod(chunk)) * es
        stride = (plain + 15) // 16 * 16
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        # only the bytes between the first and the last chunk go up
        lo, hi = int(offsets.min()), int((offsets + sizes).max())
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')                           # (a read-only mapping: it is only read)
            src = torch.from_numpy(buf[lo:hi]).to(device)
        segs, status, produced = inflate_segments(src, offsets - lo, sizes, np.full(len(entries), plain, dtype=np.int64), out_stride=stride, split=True)
        bad = (status != 0) | (produced != plain)
        for k in np.nonzero(bad.cpu().numpy())[0]:
            k = int(k)
            raw = zlib.decompress(bytes(buf[offsets[k]:offsets[k] + sizes[k]]))
            block = np.frombuffer(raw, dtype=np.uint8, count=plain)   # (a short chunk: the ValueError read() raises)
            segs[k * stride:k * stride + plain] = torch.from_numpy(block.copy()).to(device)
        swap = es > 1 and not self.dtype.isnative
        return h5_unchunk(segs, stride, index, self.dtype, shape, chunk, shuffle=2 in fids, swap=swap)

    # -- attributes ---------------------------------------------------------------------------------------------
    @property
    def attrs(self):
        return self.file._attributes(self._attr_msgs, self._attr_info)


def _filters(body):
    ver = body[0]
    n = body[1]
    out = []
    p = 8 if ver == 1 else 2
    for _ in range(n):
        fid = _u(body, p, 2)
        if ver == 1 or fid >= 256:
            namelen = _u(body, p + 2, 2); p += 4
        else:
            namelen = 0; p += 2
        flags = _u(body, p, 2); ncv = _u(body, p + 2, 2); p += 4
        if namelen:
            p += (namelen + 7) // 8 * 8 if ver == 1 else namelen
        vals = [_u(body, p + 4 * i, 4) for i in range(ncv)]
        p += 4 * ncv
        if ver == 1 and ncv % 2:
            p += 4
        out.append((fid, vals))
    return out


class Group:
    def __init__(self, f, name, msgs):
        self.file, self.name = f, name
        self._links = None
        self._msgs = msgs
        self._attr_msgs = [b for t, b in msgs if t == 0x0C]
        self._attr_info = next((b for t, b in msgs if t == 0x15), None)

    @property
    def attrs(self):
        return self.file._attributes(self._attr_msgs, self._attr_info)

    def links(self):
        if self._links is None:
            f = self.file
            links = {}
            for t, body in self._msgs:
                if t == 0x06:
                    nm, addr = _link_message(body)
                    if addr is not None:
                        links[nm] = addr
                elif t == 0x02:       # link info -> dense storage
                    flags = body[1]
                    p = 2 + (8 if flags & 1 else 0)
                    heap, index = _u(body, p, 8), _u(body, p + 8, 8)
                    if heap != UNDEF:
                        objs = f._heap_objects_by_index(heap, index, 4, 7) if index != UNDEF else f._fractal_heap_objects(heap)
                        for obj in objs:                  # (type-5 records: name hash (4), heap ID (7))
                            nm, addr = _link_message(obj)
                            if addr is not None:
                                links[nm] = addr
                elif t == 0x11:       # old-style symbol table
                    btree, heap = _u(body, 0, 8), _u(body, 8, 8)
                    links.update(f._symbol_table(btree, heap))
            self._links = links
        return self._links

    def keys(self):
        return list(self.links().keys())

    def __contains__(self, k):
        return k in self.links()

    def __getitem__(self, k):
        return self.file._object(self.links()[k], k)


def _link_message(b):
    """(name, object header address | None for soft/external links) of a link message; (None, None) for free space"""
    if len(b) < 4 or b[0] != 1:
        return None, None
    flags = b[1]
    p = 2
    ltype = 0
    if flags & 0x08:
        ltype = b[p]; p += 1
    if flags & 0x04:
        p += 8
    if flags & 0x10:
        p += 1
    lsz = 1 << (flags & 3)
    n = _u(b, p, lsz); p += lsz
    name = bytes(b[p:p + n]).decode('utf-8', 'replace'); p += n
    if ltype != 0:
        return name, None
    return name, _u(b, p, 8)


class File(Group):
    """`File(path)['wet'][:]`, `File(path)['proj'].attrs['crs_wkt']`, `File(path).attrs['datetime']`."""

    def __init__(self, path):
        # the file is MAPPED, not read: opening a 170 MB processed cube costs nothing until a dataset is asked for, and a contiguous
        # dataset can be handed to the GPU upload straight from the page cache (Dataset.raw)
        import mmap
        with open(path, 'rb') as fh:
            try:
                self._map = mmap.mmap(fh.fileno(), 0, access=mmap.ACCESS_READ)
                self.buf = memoryview(self._map)
            except (ValueError, OSError):              # empty file / no mmap on this file system
                self._map = None
                self.buf = memoryview(fh.read())
        b = self.buf
        self.path = str(path)
        # the superblock may sit at 0, 512, 1024, ...
        sb = 0
        while b[sb:sb + 8] != b'\x89HDF\r\n\x1a\n':
            sb = 512 if sb == 0 else sb * 2
            if sb >= len(b):
                raise ValueError(f'{path}: not an HDF5 file')
        ver = b[sb + 8]
        if ver in (0, 1):
            so, sl = b[sb + 13], b[sb + 14]
            if (so, sl) != (8, 8):
                raise UnsupportedHDF5Feature('offsets / lengths that are not 8 bytes')
            p = sb + 24 + (4 if ver == 1 else 0)
            self.base = _u(b, p, 8)
            # root group symbol table entry: link name offset, object header address, cache type, reserved, scratch
            root = _u(b, p + 32 + 8, 8)
        elif ver in (2, 3):
            if (b[sb + 9], b[sb + 10]) != (8, 8):
                raise UnsupportedHDF5Feature('offsets / lengths that are not 8 bytes')
            self.base = _u(b, sb + 12, 8)
            root = _u(b, sb + 36, 8)
        else:
            raise UnsupportedHDF5Feature(f'superblock version {ver}')
        self._cache = {}
        Group.__init__(self, self, '/', self._header_messages(root))

    def close(self):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    # -- object headers -----------------------------------------------------------------------------------------
    def _header_messages(self, addr):
        b = self.buf
        a = self.base + addr
        msgs = []
        if b[a:a + 4] == b'OHDR':
            flags = b[a + 5]
            p = a + 6
            if flags & 0x20:
                p += 16
            if flags & 0x10:
                p += 4
            szb = 1 << (flags & 3)
            size0 = _u(b, p, szb); p += szb
            blocks = [(p, p + size0)]
            while blocks:
                p, end = blocks.pop(0)
                while p + 4 <= end:
                    t = b[p]; sz = _u(b, p + 1, 2); p += 4
                    if flags & 0x04:
                        p += 2
                    body = b[p:p + sz]; p += sz
                    if t == 0x10:
                        off, ln = _u(body, 0, 8), _u(body, 8, 8)
                        o = self.base + off
                        if b[o:o + 4] != b'OCHK':
                            raise ValueError('corrupt object header continuation')
                        blocks.append((o + 4, o + ln - 4))
                    elif t != 0:
                        msgs.append((t, body))
            return msgs
        # version 1 object header
        if b[a] != 1:
            raise UnsupportedHDF5Feature(f'object header version {b[a]} at {addr}')
        nmsg = _u(b, a + 2, 2)
        size0 = _u(b, a + 8, 4)
        blocks = [(a + 16, a + 16 + size0)]
        while blocks and len(msgs) < nmsg + 64:
            p, end = blocks.pop(0)
            while p + 8 <= end:
                t = _u(b, p, 2); sz = _u(b, p + 2, 2); p += 8
                body = b[p:p + sz]; p += sz
                if t == 0x10:
                    off, ln = _u(body, 0, 8), _u(body, 8, 8)
                    blocks.append((self.base + off, self.base + off + ln))
                elif t != 0:
                    msgs.append((t, body))
        return msgs

    def _object(self, addr, name):
        if addr not in self._cache:
            msgs = self._header_messages(addr)
            types = {t for t, _ in msgs}
            self._cache[addr] = Dataset(self, name, msgs) if 0x08 in types else Group(self, name, msgs)
        return self._cache[addr]

    # -- fractal heap (dense links / dense attributes) ---------------------------------------------------------------
    def _fractal_heap(self, addr):
        """(direct blocks as (file position, heap offset, size), header fields) of a fractal heap."""
        b = self.buf
        a = self.base + addr
        if b[a:a + 4] != b'FRHP':
            raise ValueError('corrupt fractal heap header')
        filt = _u(b, a + 7, 2)
        flags = b[a + 9]
        maxman = _u(b, a + 10, 4)
        p = a + 10 + 4 + 8 + 8 + 8 + 8 + 8 + 8 + 8
        nman = _u(b, p, 8); p += 8
        p += 8 * 4
        width = _u(b, p, 2); p += 2
        start = _u(b, p, 8); p += 8
        maxdirect = _u(b, p, 8); p += 8
        maxheapbits = _u(b, p, 2); p += 2
        p += 2
        root = _u(b, p, 8); p += 8
        nrows = _u(b, p, 2); p += 2
        if filt:
            raise UnsupportedHDF5Feature('filtered fractal heap')
        offbytes = (maxheapbits + 7) // 8
        hdr = 5 + 8 + offbytes + (4 if flags & 2 else 0)
        blocks = []

        def direct(addr_, size):
            q = self.base + addr_
            if b[q:q + 4] != b'FHDB':
                raise ValueError('corrupt fractal heap direct block')
            blocks.append((q, _u(b, q + 13, offbytes), size))

        def indirect(addr_, rows):
            q = self.base + addr_
            if b[q:q + 4] != b'FHIB':
                raise ValueError('corrupt fractal heap indirect block')
            pp = q + 5 + 8 + offbytes
            maxdrows = (maxdirect.bit_length() - 1) - (start.bit_length() - 1) + 2
            for r in range(rows):
                size = start if r < 2 else start << (r - 1)
                for _ in range(width):
                    child = _u(b, pp, 8); pp += 8
                    if child == UNDEF:
                        continue
                    if r < maxdrows:
                        direct(child, size)
                    else:
                        crow = (size // start).bit_length() - 1 - (width.bit_length() - 1) + 1
                        indirect(child, crow)

        if root != UNDEF:
            if nrows == 0:
                direct(root, start)
            else:
                indirect(root, nrows)
        enc = lambda x: (max(int(x), 1).bit_length() - 1) // 8 + 1                # H5VM_limit_enc_size
        lenbytes = min((maxdirect.bit_length() - 1 + 7) // 8, enc(maxman))
        return blocks, dict(nman=nman, hdr=hdr, offbytes=offbytes, lenbytes=lenbytes)

    def _fractal_heap_objects(self, addr):
        """Every managed object of the heap, in heap order, found by walking the direct blocks back to back (links and attributes are
        self-delimiting).  Only right for a heap nothing was ever removed from - the fallback when the object has no name index."""
        b = self.buf
        blocks, info = self._fractal_heap(addr)
        out = []
        for q, _off, size in blocks:
            p, hi = q + info['hdr'], q + size
            while p < hi and len(out) < info['nman']:
                n = self._self_delimited(b, p, hi)
                if n is None:
                    break
                out.append(b[p:p + n]); p += n
        return out

    def _heap_objects_by_index(self, heap_addr, btree_addr, id_off, id_len):
        """The LIVE objects of a fractal heap: the version-2 B-tree that indexes them (links by name hash: type 5, attributes by name: type 8)
        holds one record per object with its heap ID at record bytes [id_off, id_off + id_len) - offset and length inside the heap's
        address space.  Space freed by a deleted or renamed attribute / link still holds its old bytes, which a walk of the blocks would
        take for an object (h5py writes every attribute under a temporary name first)."""
        b = self.buf
        blocks, info = self._fractal_heap(heap_addr)
        out = []
        for rec in self._btree2_records(btree_addr):
            hid = rec[id_off:id_off + id_len]
            kind = (hid[0] >> 4) & 3
            if kind != 0:
                raise UnsupportedHDF5Feature('huge / tiny fractal-heap object')
            off = _u(hid, 1, info['offbytes']); ln = _u(hid, 1 + info['offbytes'], info['lenbytes'])
            for q, boff, size in blocks:
                if boff <= off < boff + size:
                    out.append(b[q + off - boff:q + off - boff + ln])
                    break
            else:
                raise ValueError('fractal heap ID outside every direct block')
        return out

    def _btree2_records(self, addr):
        """All records of a version-2 B-tree (HDF5 spec III.A.2), as raw bytes."""
        b = self.buf
        a = self.base + addr
        if b[a:a + 4] != b'BTHD':
            raise ValueError('corrupt version-2 B-tree header')
        nodesize, recsize, depth = _u(b, a + 6, 4), _u(b, a + 10, 2), _u(b, a + 12, 2)
        root, nroot = _u(b, a + 16, 8), _u(b, a + 24, 2)
        if root == UNDEF or nroot == 0:
            return []
        enc = lambda x: (max(int(x), 1).bit_length() - 1) // 8 + 1                # H5VM_limit_enc_size
        max_leaf = (nodesize - 10) // recsize
        nrec_size = enc(max_leaf)
        cum = [max_leaf]; cum_size = [0]                                           # per level: cumulative max records, and its field width
        for u in range(1, depth + 1):
            ptr = 8 + nrec_size + cum_size[u - 1]
            mx = (nodesize - (10 + ptr)) // (recsize + ptr)
            cum.append((mx + 1) * cum[u - 1] + mx); cum_size.append(enc(cum[u]))
        out = []

        def node(addr_, nrec, level):
            q = self.base + addr_
            sig = b'BTLF' if level == 0 else b'BTIN'
            if b[q:q + 4] != sig:
                raise ValueError('corrupt version-2 B-tree node')
            p = q + 6
            recs = [bytes(b[p + i * recsize:p + (i + 1) * recsize]) for i in range(nrec)]
            p += nrec * recsize
            if level == 0:
                out.extend(recs)
                return
            for i in range(nrec + 1):
                caddr = _u(b, p, 8); p += 8
                cn = _u(b, p, nrec_size); p += nrec_size
                p += cum_size[level - 1]
                node(caddr, cn, level - 1)
                if i < nrec:
                    out.append(recs[i])

        node(root, nroot, depth)
        return out

    @staticmethod
    def _self_delimited(b, p, hi):
        """length of the link / attribute message starting at p (None when the bytes there are free space)"""
        v = b[p]
        if v == 1:                         # link message
            flags = b[p + 1]
            q = p + 2
            ltype = 0
            if flags & 0x08:
                ltype = b[q]; q += 1
            if flags & 0x04:
                q += 8
            if flags & 0x10:
                q += 1
            lsz = 1 << (flags & 3)
            n = _u(b, q, lsz); q += lsz + n
            if ltype == 0:
                q += 8
            elif ltype == 1:
                q += 2 + _u(b, q, 2)
            elif ltype == 64:
                q += 2 + _u(b, q, 2)
            else:
                return None
            return q - p if q <= hi else None
        if v == 3:                         # attribute message (version 3)
            nsz, tsz, ssz = _u(b, p + 2, 2), _u(b, p + 4, 2), _u(b, p + 6, 2)
            q = p + 9 + nsz
            dt = _Datatype(b, q)
            dims = _dataspace(b[q + tsz:q + tsz + ssz])
            count = int(np.prod(dims)) if dims else (0 if dims is None else 1)
            q += tsz + ssz + count * dt.size
            return q - p if q <= hi else None
        return None

    # -- attributes -------------------------------------------------------------------------------------------------
    def _attributes(self, msgs, info):
        out = {}
        bodies = list(msgs)
        if info is not None:
            flags = info[1]
            p = 2 + (2 if flags & 1 else 0)
            heap, index = _u(info, p, 8), _u(info, p + 8, 8)
            if heap != UNDEF:       # (type-8 records: heap ID (8), message flags (1), creation order (4), name hash (4))
                bodies.extend(self._heap_objects_by_index(heap, index, 0, 8) if index != UNDEF else self._fractal_heap_objects(heap))
        for body in bodies:
            try:
                k, v = self._attribute(body)
            except UnsupportedHDF5Feature:
                continue
            out[k] = v
        return out

    def _attribute(self, m):
        ver = m[0]
        if ver == 1:
            nsz, tsz, ssz = _u(m, 2, 2), _u(m, 4, 2), _u(m, 6, 2)
            pad = lambda n: (n + 7) // 8 * 8
            p = 8
            name = bytes(m[p:p + nsz]).split(b'\0')[0].decode(); p += pad(nsz)
            dt = _Datatype(m, p); p += pad(tsz)
            dims = _dataspace(m[p:p + ssz]); p += pad(ssz)
        elif ver in (2, 3):
            nsz, tsz, ssz = _u(m, 2, 2), _u(m, 4, 2), _u(m, 6, 2)
            p = 8 + (1 if ver == 3 else 0)
            name = bytes(m[p:p + nsz]).split(b'\0')[0].decode(); p += nsz
            dt = _Datatype(m, p); p += tsz
            dims = _dataspace(m[p:p + ssz]); p += ssz
        else:
            raise UnsupportedHDF5Feature(f'attribute message version {ver}')
        count = int(np.prod(dims)) if dims else (0 if dims is None else 1)
        data = m[p:p + count * dt.size]
        if dt.cls == 3:
            vals = [bytes(data[i * dt.size:(i + 1) * dt.size]).split(b'\0')[0].decode('utf-8', 'replace') for i in range(count)]
            return name, (vals[0] if not dims else vals)
        if dt.cls == 9 and dt.vlen_string:
            vals = []
            for i in range(count):
                q = i * dt.size
                ln, col, idx = _u(data, q, 4), _u(data, q + 4, 8), _u(data, q + 12, 4)
                vals.append(self._global_heap(col, idx)[:ln].decode('utf-8', 'replace'))
            return name, (vals[0] if not dims else vals)
        if dt.dtype is None or dt.cls not in (0, 1):
            raise UnsupportedHDF5Feature('attribute type')
        arr = np.frombuffer(data, dtype=dt.dtype, count=count).astype(dt.dtype.newbyteorder('='))
        return name, (arr[0] if not dims else arr.reshape(dims))

    def _global_heap(self, addr, index):
        b = self.buf
        a = self.base + addr
        if b[a:a + 4] != b'GCOL':
            raise ValueError('corrupt global heap collection')
        size = _u(b, a + 8, 8)
        p = a + 16
        while p < a + size:
            idx = _u(b, p, 2); osz = _u(b, p + 8, 8)
            if idx == 0:
                break
            if idx == index:
                return bytes(b[p + 16:p + 16 + osz])
            p += 16 + (osz + 7) // 8 * 8
        raise KeyError(f'global heap object {index}')

    # -- version-1 B-trees: old-style groups and chunk indices -----------------------------------------------------------
    def _symbol_table(self, btree, heap):
        b = self.buf
        h = self.base + heap
        if b[h:h + 4] != b'HEAP':
            raise ValueError('corrupt local heap')
        data = self.base + _u(b, h + 24, 8)
        out = {}

        def node(addr):
            a = self.base + addr
            if b[a:a + 4] == b'TREE':
                level = b[a + 5]; n = _u(b, a + 6, 2)
                p = a + 24
                for i in range(n):
                    child = _u(b, p + 8, 8); p += 16
                    node(child)
            elif b[a:a + 4] == b'SNOD':
                n = _u(b, a + 6, 2)
                p = a + 8
                for i in range(n):
                    noff, oaddr = _u(b, p, 8), _u(b, p + 8, 8)
                    e = data + noff
                    while b[e] != 0:                      # (a memoryview has no .index)
                        e += 1
                    out[bytes(b[data + noff:e]).decode()] = oaddr
                    p += 40
            else:
                raise ValueError('corrupt group B-tree')
        node(btree)
        return out

    def _chunk_btree(self, addr, nd):
        b = self.buf
        a = self.base + addr
        if b[a:a + 4] != b'TREE':
            raise ValueError('corrupt chunk B-tree')
        level = b[a + 5]; n = _u(b, a + 6, 2)
        keysz = 8 + 8 * (nd + 1)
        p = a + 24
        for i in range(n):
            size, mask = _u(b, p, 4), _u(b, p + 4, 4)
            offs = tuple(_u(b, p + 8 + 8 * d, 8) for d in range(nd))
            child = _u(b, p + keysz, 8)
            p += keysz + 8
            if level == 0:
                yield offs, size, mask, child
            else:
                yield from self._chunk_btree(child, nd)
