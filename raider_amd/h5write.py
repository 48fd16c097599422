"""A small write-only HDF5 / NetCDF-4 writer (pure Python + NumPy) - the counterpart of raider_amd.h5lite.

The reference writes its processed weather cubes (models/weatherModel.py:659-724) and delay cubes (delay.py:329-401 ->
cli/raider.py:373-398, `ds.to_netcdf`) as NetCDF-4 = HDF5 through xarray + netCDF4.  Neither library is part of this build's
environment, so this module writes the same on-disk product itself: one HDF5 file whose layout follows the published HDF5
File Format Specification (version 3.0) in its most widely readable form, dressed with the NetCDF-4 conventions that
netCDF-C / h5netcdf / xarray rely on:

  * superblock version 0; version-1 object headers; the root group as a symbol table (one version-1 B-tree node, one symbol
    table node, a local heap with the link names) - readable by every libhdf5 since 1.0;
  * datasets: contiguous storage, little-endian IEEE floats / two's-complement integers, a fill-value message; scalar or
    N-dimensional simple dataspaces; or chunked storage behind a shuffle + deflate filter pipeline (ChunkedData: version-3 layout
    class 2, filter pipeline message version 1, ONE version-1 B-tree leaf - at most 64 chunks - and the chunks behind it), from
    chunk bytes the caller compressed;
  * attributes (version-1 attribute messages): fixed-length NUL-terminated ASCII strings, numeric scalars / vectors;
  * NetCDF-4 dimensions as HDF5 DIMENSION SCALES: every dimension has a coordinate variable carrying CLASS =
    "DIMENSION_SCALE", NAME, _Netcdf4Dimid and the REFERENCE_LIST back pointers (compound {object reference, uint32}); every
    variable on dimensions carries DIMENSION_LIST (variable-length sequences of object references, kept in a global heap
    collection) and _Netcdf4Coordinates; the root group carries _NCProperties.

Validated in the build container against libhdf5 1.10.6 itself (h5dump / h5ls / H5DSis_scale via ctypes, tests/test_h5write.py)
and read back by raider_amd.h5lite; the files the reference's own writer produced (tests/golden/ref_files) have the same
structure attribute for attribute (h5dump -H).  What a NetCDF-4 reader sees: dims z, y, x with coordinate variables, the data
variables with their CF attributes, the grid-mapping variable - i.e. the reference's product.
"""
import struct

import numpy as np

UNDEF = 0xFFFFFFFFFFFFFFFF
_LEAF_K = 32          # symbol table node holds 2 * K entries: one node is enough for a cube file (< 64 objects)
_INTERNAL_K = 16


def _pad8(b):
    return b + b'\0' * (-len(b) % 8)


# ---- datatype messages -------------------------------------------------------------------------------------------------
def _dt_numeric(dt, big_endian_ok=False):
    dt = np.dtype(dt)
    if dt.byteorder == '>':
        if not big_endian_ok:
            raise ValueError('big-endian arrays are not written')
        msg = bytearray(_dt_numeric(dt.newbyteorder('<')))
        msg[1] |= 1                                    # byte order: big-endian (a ChunkedData whose caller stored its chunks so)
        return bytes(msg)
    if dt.kind == 'f':
        if dt.itemsize == 4:
            props = struct.pack('<HHBBBBI', 0, 32, 23, 8, 0, 23, 127); bits = bytes([0x20, 31, 0])
        elif dt.itemsize == 8:
            props = struct.pack('<HHBBBBI', 0, 64, 52, 11, 0, 52, 1023); bits = bytes([0x20, 63, 0])
        else:
            raise ValueError(f'unsupported float size {dt.itemsize}')
        return bytes([0x11]) + bits + struct.pack('<I', dt.itemsize) + props
    if dt.kind in 'iu':
        bits = bytes([0x08 if dt.kind == 'i' else 0x00, 0, 0])
        return bytes([0x10]) + bits + struct.pack('<I', dt.itemsize) + struct.pack('<HH', 0, 8 * dt.itemsize)
    raise ValueError(f'unsupported element type {dt}')


def _dt_string(n):            # fixed length, NUL terminated, ASCII
    return bytes([0x13, 0x00, 0, 0]) + struct.pack('<I', n)


_DT_OBJREF = bytes([0x17, 0x00, 0, 0]) + struct.pack('<I', 8)
_DT_VLEN_OBJREF = bytes([0x19, 0x00, 0, 0]) + struct.pack('<I', 16) + _DT_OBJREF


def _dt_reference_list():
    """H5T_COMPOUND { H5T_STD_REF_OBJECT "dataset"; H5T_STD_U32LE "dimension" }, 12 bytes (version-1 compound encoding)."""
    def member(name, offset, dtmsg):
        return _pad8(name.encode() + b'\0') + struct.pack('<IB3xII4I', offset, 0, 0, 0, 0, 0, 0, 0) + dtmsg
    body = member('dataset', 0, _DT_OBJREF) + member('dimension', 8, _dt_numeric(np.uint32))
    return bytes([0x16, 2, 0, 0]) + struct.pack('<I', 12) + body


def _dataspace(shape):
    if shape == ():
        return struct.pack('<BBB5x', 1, 0, 0)
    return struct.pack('<BBB5x', 1, len(shape), 1) + b''.join(struct.pack('<Q', int(s)) for s in shape) * 2


# ---- attribute values --------------------------------------------------------------------------------------------------
class DimensionList:
    """DIMENSION_LIST of a variable: one scale (dimension) name per axis."""

    def __init__(self, dims):
        self.dims = list(dims)


class ReferenceList:
    """REFERENCE_LIST of a dimension scale: (variable name, axis index) for every variable axis that uses it."""

    def __init__(self, refs):
        self.refs = list(refs)


class _Attr:
    def __init__(self, name, value):
        self.name, self.value = name, value
        self.vlen_slots = None          # DimensionList: global heap object indices, filled by the writer

    def parts(self, addr_of, gcol_addr):
        """(datatype message, dataspace message, data bytes)"""
        v = self.value
        if isinstance(v, str):
            raw = v.encode('ascii', 'replace') + b'\0'
            return _dt_string(len(raw)), _dataspace(()), raw
        if isinstance(v, DimensionList):
            data = b''.join(struct.pack('<IQI', 1, gcol_addr, idx) for idx in self.vlen_slots)
            return _DT_VLEN_OBJREF, _dataspace((len(v.dims),)), data
        if isinstance(v, ReferenceList):
            data = b''.join(struct.pack('<QI', addr_of(nm), int(ax)) for nm, ax in v.refs)
            return _dt_reference_list(), _dataspace((len(v.refs),)), data
        a = _le_array(v)
        return _dt_numeric(a.dtype), _dataspace(a.shape), a.tobytes()

    def message(self, addr_of, gcol_addr):
        dt, sp, data = self.parts(addr_of, gcol_addr)
        nm = self.name.encode() + b'\0'
        return struct.pack('<BxHHH', 1, len(nm), len(dt), len(sp)) + _pad8(nm) + _pad8(dt) + _pad8(sp) + data


def _le_array(v):
    """C-ordered little-endian copy that KEEPS a 0-d array 0-d (np.ascontiguousarray would make it 1-d)."""
    a = np.asarray(v)
    if a.dtype.kind == 'b':
        a = a.astype(np.int8)
    if a.dtype == np.float16:
        a = a.astype(np.float32)
    if a.dtype.kind not in 'fiu':
        raise ValueError(f'unsupported element type {a.dtype}')
    return np.array(a, dtype=a.dtype.newbyteorder('<') if a.dtype.byteorder == '>' else a.dtype, order='C', copy=True)


def _message(mtype, body, flags=0):
    body = _pad8(body)
    return struct.pack('<HHB3x', mtype, len(body), flags) + body


def _object_header(messages):
    body = b''.join(messages)
    # version 1 prefix: version, reserved, number of messages, reference count, header data size, then 4 bytes of alignment
    return struct.pack('<BxHII4x', 1, len(messages), 1, len(body)) + body


class ChunkedData:
    """The data of a chunked, filtered variable, compressed by the CALLER: this writer lays the file out and never compresses.
    shape / dtype: the variable's; chunks: the chunk shape (every chunk is stored full size, edge chunks padded with the fill
    value); filters: ('shuffle', 'deflate'), ('deflate',) or () in HDF5's pipeline order, 'fletcher32' last when the caller put the four
    checksum bytes behind every chunk (this writer neither computes nor checks them: a file whose bytes are not HDF5's Fletcher-32 of
    the chunk is refused by libhdf5, while h5lite drops them unverified); a big-endian dtype says the caller stored the elements so; packed: the chunks' stored bytes back to
    back in row-major chunk order (a uint8 array or bytes), chunk k being packed[offsets[k]:offsets[k + 1]].  raider_amd.deflate
    .compress_chunks makes (packed, offsets) on the device; NumPy shuffle + zlib.compress make the same on the host."""

    def __init__(self, shape, dtype, chunks, packed, offsets, filters=('shuffle', 'deflate'), level=1):
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.chunks = tuple(int(c) for c in chunks)
        self.filters = tuple(filters)
        self.level = int(level)
        self.packed = np.frombuffer(packed, dtype=np.uint8) if isinstance(packed, (bytes, bytearray, memoryview)) else np.ascontiguousarray(packed, dtype=np.uint8).ravel()
        self.offsets = np.asarray(offsets, dtype=np.int64).ravel()
        if len(self.chunks) != len(self.shape) or not self.shape:
            raise ValueError(f'chunks {self.chunks} do not fit a variable of shape {self.shape}')
        if any(c <= 0 or c > s for c, s in zip(self.chunks, self.shape)):
            raise ValueError(f'chunk sizes must lie in 1 .. the dimension size: chunks {self.chunks}, shape {self.shape}')
        if any(f not in ('shuffle', 'deflate', 'fletcher32') for f in self.filters):
            raise ValueError(f"filters are 'shuffle', 'deflate' and 'fletcher32', not {self.filters}")
        self.grid = tuple(-(-s // c) for s, c in zip(self.shape, self.chunks))
        self.nchunks = int(np.prod(self.grid))
        if self.offsets.size != self.nchunks + 1 or self.offsets[0] != 0 or np.any(np.diff(self.offsets) <= 0) or self.offsets[-1] != self.packed.size:
            raise ValueError(f'{self.nchunks} chunks need {self.nchunks + 1} increasing offsets from 0 to len(packed) = {self.packed.size}')
        if np.any(np.diff(self.offsets) >= 1 << 32):
            raise ValueError('a stored chunk must be smaller than 4 GiB')


_CHUNK_K = 32         # superblock version 0 implies it: one leaf of the chunk B-tree holds 2 * K chunks
_FILTER_IDS = {'deflate': 1, 'shuffle': 2, 'fletcher32': 3}


class _Dataset:
    def __init__(self, name, data, attrs, fill=None):
        self.name = name
        self.chunked = data if isinstance(data, ChunkedData) else None
        if self.chunked is not None:
            if self.chunked.nchunks > 2 * _CHUNK_K:
                raise ValueError(f'variable {name!r} needs {self.chunked.nchunks} chunks; one B-tree leaf holds {2 * _CHUNK_K} '
                                 '(multi-level chunk trees are not written: choose larger chunks)')
            _dt_numeric(self.chunked.dtype, big_endian_ok=True)
            self.data = None
            self.shape, self.dtype = self.chunked.shape, self.chunked.dtype
        else:
            self.data = _le_array(data)
            self.shape, self.dtype = self.data.shape, self.data.dtype
        self.attrs = [_Attr(k, v) for k, v in attrs]
        self.fill = fill
        self.header_addr = None
        self.data_addr = None

    def storage_bytes(self):
        """Bytes behind data_addr: the array, or the chunk B-tree's leaf followed by the stored chunks."""
        if self.chunked is None:
            return self.data.nbytes
        return self._node_bytes() + int(self.chunked.packed.size)

    def _node_bytes(self):
        key = 8 + 8 * (len(self.shape) + 1)
        return 24 + 2 * _CHUNK_K * 8 + (2 * _CHUNK_K + 1) * key

    def storage(self):
        if self.chunked is None:
            return self.data.tobytes()
        c = self.chunked
        first = self.data_addr + self._node_bytes()
        node = b'TREE' + struct.pack('<BBHQQ', 1, 0, c.nchunks, UNDEF, UNDEF)
        for k, idx in enumerate(np.ndindex(*c.grid)):
            offs = [i * ch for i, ch in zip(idx, c.chunks)] + [0]
            node += struct.pack('<II', int(c.offsets[k + 1] - c.offsets[k]), 0) + struct.pack(f'<{len(offs)}Q', *offs)
            node += struct.pack('<Q', first + int(c.offsets[k]))
        beyond = [c.grid[0] * c.chunks[0]] + [0] * len(c.shape)              # the last key: greater than every chunk's offsets
        node += struct.pack('<II', 0, 0) + struct.pack(f'<{len(beyond)}Q', *beyond)
        node += bytes(self._node_bytes() - len(node))
        return node + c.packed.tobytes()

    def header(self, addr_of, gcol_addr):
        c = self.chunked
        msgs = [_message(0x01, _dataspace(self.shape)), _message(0x03, _dt_numeric(self.dtype, big_endian_ok=c is not None), flags=1)]
        alloc = 2 if c is None else 3                                        # late for contiguous, incremental for chunked storage: libhdf5's defaults
        if self.fill is not None:
            fv = np.asarray(self.fill, dtype=self.dtype).tobytes()
            msgs.append(_message(0x05, struct.pack('<BBBBI', 2, alloc, 2, 1, len(fv)) + fv))       # v2: write if set, defined
        else:
            msgs.append(_message(0x05, struct.pack('<BBBB', 2, alloc, 2, 0)))
        if c is None:
            addr = (self.data_addr or 0) if self.data.size else UNDEF
            msgs.append(_message(0x08, struct.pack('<BBQQ', 3, 1, addr, self.data.nbytes)))          # v3 layout, contiguous
        else:
            if c.filters:
                body = struct.pack('<BB6x', 1, len(c.filters))
                for f in c.filters:
                    client = [self.dtype.itemsize] if f == 'shuffle' else [c.level] if f == 'deflate' else []
                    name = _pad8(f.encode() + b'\0')
                    body += struct.pack('<HHHH', _FILTER_IDS[f], len(name), 1, len(client)) + name                # optional filter, named as libhdf5 names it
                    body += struct.pack(f'<{len(client)}I', *client) + (b'\0' * 4 if len(client) % 2 else b'')
                msgs.append(_message(0x0B, body))
            dims = list(c.chunks) + [self.dtype.itemsize]
            msgs.append(_message(0x08, struct.pack('<BBBQ', 3, 2, len(dims), self.data_addr or 0) + struct.pack(f'<{len(dims)}I', *dims)))
        for a in self.attrs:
            msgs.append(_message(0x0C, a.message(addr_of, gcol_addr)))
        return _object_header(msgs)


def write_hdf5(path, datasets, root_attrs=()):
    """datasets: list of (name, array or ChunkedData, [(attr name, value), ...], fill value or None).  Attribute values: str, numbers /
    NumPy arrays, DimensionList, ReferenceList."""
    dsets = [_Dataset(n, a, at, fv) for n, a, at, fv in datasets]
    names = [d.name for d in dsets]
    if len(set(names)) != len(names):
        raise ValueError('duplicate dataset names')
    if len(dsets) > 2 * _LEAF_K:
        raise ValueError(f'at most {2 * _LEAF_K} datasets per file')
    by_name = {d.name: d for d in dsets}
    root_attr = [_Attr(k, v) for k, v in root_attrs]
    # ---- global heap: one object (an 8-byte object reference) per DIMENSION_LIST entry
    vlen = []                        # (attr, position, target name)
    for d in dsets:
        for a in d.attrs:
            if isinstance(a.value, DimensionList):
                a.vlen_slots = []
                for nm in a.value.dims:
                    vlen.append(nm)
                    a.vlen_slots.append(len(vlen))          # heap object indices start at 1
    gcol_size = max(4096, 16 + 24 * len(vlen) + 16)
    gcol_size += -gcol_size % 8

    # ---- layout: sizes do not depend on addresses, so one dry serialisation fixes every address
    def dry(obj_header):
        return len(obj_header(lambda nm: 0, 0))
    pos = 96                                                  # superblock (version 0, 8-byte offsets / lengths)
    heap_names = b'\0' * 8
    name_off = {}
    for nm in sorted(names):
        name_off[nm] = len(heap_names)
        heap_names += _pad8(nm.encode() + b'\0')
    heap_data_size = len(heap_names) + (-len(heap_names) % 8)
    heap_data_size = max(heap_data_size, 88)

    def root_header(addr_of, gcol_addr):
        msgs = [_message(0x11, struct.pack('<QQ', btree_addr, heap_addr))]
        for a in root_attr:
            msgs.append(_message(0x0C, a.message(addr_of, gcol_addr)))
        return _object_header(msgs)
    btree_addr = heap_addr = 0
    root_addr = pos; pos += dry(root_header); pos += -pos % 8
    btree_addr = pos; pos += 24 + (2 * _INTERNAL_K + 1) * 8 + 2 * _INTERNAL_K * 8
    heap_addr = pos; pos += 32
    heap_data_addr = pos; pos += heap_data_size
    snod_addr = pos; pos += 8 + 2 * _LEAF_K * 40
    gcol_addr = pos if vlen else 0
    if vlen:
        pos += gcol_size
    for d in dsets:
        d.header_addr = pos; pos += dry(d.header); pos += -pos % 8
    for d in dsets:
        d.data_addr = pos; pos += d.storage_bytes(); pos += -pos % 8
    eof = pos
    addr_of = lambda nm: by_name[nm].header_addr

    out = bytearray(eof)

    def put(addr, b):
        out[addr:addr + len(b)] = b
    # superblock
    sb = b'\x89HDF\r\n\x1a\n' + struct.pack('<BBBxBBBx', 0, 0, 0, 0, 8, 8) + struct.pack('<HHI', _LEAF_K, _INTERNAL_K, 0)
    sb += struct.pack('<QQQQ', 0, UNDEF, eof, UNDEF)
    sb += struct.pack('<QQI4xQQ', 0, root_addr, 1, btree_addr, heap_addr)       # root symbol table entry (cached: B-tree + heap)
    assert len(sb) == 96
    put(0, sb)
    put(root_addr, root_header(addr_of, gcol_addr))
    # B-tree (group node, leaf level): keys are heap offsets of names; key[0] = 0 (the empty string), key[1] = the largest name
    ordered = sorted(names)
    bt = b'TREE' + struct.pack('<BBHQQ', 0, 0, 1, UNDEF, UNDEF) + struct.pack('<QQQ', 0, snod_addr, name_off[ordered[-1]] if ordered else 0)
    put(btree_addr, bt)
    # local heap
    free_off = len(heap_names)
    if heap_data_size - free_off >= 16:
        put(heap_data_addr + free_off, struct.pack('<QQ', 1, heap_data_size - free_off))      # one free block: next = 1 (none), size
        free_head = free_off
    else:
        free_head = 1                                                                             # H5HL_FREE_NULL
    put(heap_addr, b'HEAP' + struct.pack('<B3xQQQ', 0, heap_data_size, free_head, heap_data_addr))
    put(heap_data_addr, heap_names)
    # symbol table node
    sn = b'SNOD' + struct.pack('<BxH', 1, len(ordered))
    for nm in ordered:
        sn += struct.pack('<QQI4x16x', name_off[nm], by_name[nm].header_addr, 0)
    put(snod_addr, sn)
    # global heap collection
    if vlen:
        g = b'GCOL' + struct.pack('<B3xQ', 1, gcol_size)
        for i, nm in enumerate(vlen, start=1):
            g += struct.pack('<HH4xQ', i, 0, 8) + struct.pack('<Q', addr_of(nm))
        rest = gcol_size - len(g)
        g += struct.pack('<HH4xQ', 0, 0, rest)                                                    # object 0: the free space
        put(gcol_addr, g)
    for d in dsets:
        put(d.header_addr, d.header(addr_of, gcol_addr))
        if d.storage_bytes():
            put(d.data_addr, d.storage())
    with open(path, 'wb') as fh:
        fh.write(out)
    return str(path)


def write_netcdf4(path, dims, variables, global_attrs=None, fill_floats=True):
    """A NetCDF-4 (HDF5) file with the classic data model the reference's cubes use.

    dims: ordered {name: size}; every dimension needs a coordinate variable of the same name in `variables`.
    variables: ordered {name: (dim names tuple, array, {attribute: value})}; a scalar variable has dims ().  A ChunkedData in the
    array's place makes the variable chunked and filtered, from chunk bytes the caller has compressed.
    Floating-point variables get the _FillValue = NaN attribute and fill value xarray writes for them."""
    dims = dict(dims)
    for dname, size in dims.items():
        if dname not in variables or tuple(variables[dname][0]) != (dname,):
            raise ValueError(f'dimension {dname!r} needs a coordinate variable of that name on ({dname!r},)')
        if int(np.size(variables[dname][1])) != int(size):
            raise ValueError(f'coordinate variable {dname!r} has {np.size(variables[dname][1])} elements, the dimension {size}')
    dimid = {d: i for i, d in enumerate(dims)}
    users = {d: [] for d in dims}                      # REFERENCE_LIST back pointers
    for name, (vd, arr, _) in variables.items():
        arr = arr if isinstance(arr, ChunkedData) else np.asarray(arr)
        if tuple(arr.shape) != tuple(int(dims[d]) for d in vd):
            raise ValueError(f'variable {name!r} has shape {tuple(arr.shape)}, its dimensions say {tuple(int(dims[d]) for d in vd)}')
        if name in dims:
            continue
        for ax, d in enumerate(vd):
            users[d].append((name, ax))
    dsets = []
    for name, (vd, arr, attrs) in variables.items():
        arr = arr if isinstance(arr, ChunkedData) else np.asarray(arr)
        at = []
        fill = None
        if name in dims:
            at += [('CLASS', 'DIMENSION_SCALE'), ('NAME', name)]
            at.append(('_Netcdf4Coordinates', np.array([dimid[name]], dtype=np.int32)))
            at.append(('_Netcdf4Dimid', np.int32(dimid[name])))
        elif vd:
            at.append(('DIMENSION_LIST', DimensionList(vd)))
            at.append(('_Netcdf4Coordinates', np.array([dimid[d] for d in vd], dtype=np.int32)))
        if fill_floats and arr.dtype.kind == 'f' and '_FillValue' not in attrs:
            at.append(('_FillValue', np.array([np.nan], dtype=arr.dtype)))
            fill = np.nan
        for k, v in attrs.items():
            if k == '_FillValue':
                fill = np.asarray(v).ravel()[0]
                v = np.array([fill], dtype=arr.dtype)
            elif not isinstance(v, str) and np.ndim(v) == 0:
                v = np.atleast_1d(np.asarray(v))             # a NetCDF numeric attribute is a 1-D array, even of one element
            at.append((k, v))
        if name in dims and users[name]:
            # last, where netCDF-C puts it (it attaches the scales when the file is closed) - and where h5repack 1.10 needs it: its
            # reference pass takes every attribute stored AFTER a compound-with-reference one for a reference attribute as well
            at.append(('REFERENCE_LIST', ReferenceList(users[name])))
        dsets.append((name, arr, at, fill))
    root = [('_NCProperties', 'version=2,raider_amd_h5write=1')] + [(k, v if isinstance(v, str) or np.ndim(v) else np.atleast_1d(np.asarray(v))) for k, v in (global_attrs or {}).items()]
    return write_hdf5(path, dsets, root)
