"""GeoTIFF rasters without GDAL: the reader and writer behind `rio_open` / `writeDelays(outformat='GTiff')` when rasterio is absent.

Written from the TIFF 6.0, BigTIFF and GeoTIFF 1.1 specifications.  What is read: the FIRST image file directory (overviews and masks
in later ones are ignored) of a classic (magic 42) or BigTIFF (magic 43) file in either byte order; strips or tiles; chunky or planar
samples of uint8/16/32, int8/16/32, float32/64 in any band count; compression 1 (none), 5 (LZW), 8 / 32946 (deflate), 32773
(PackBits); predictor 1 and 2.  Everything else is refused BY NAME (`UnsupportedTIFFFeature`), as h5lite refuses what it does not read.

Where the bytes are decoded: PackBits on the host; deflate on the host (zlib) or, for files of many segments read with `device=`
(and whenever inflate='device' asks for it), on the GPU (rdr_inflate_decode, one wave per segment); LZW on the GPU (rdr_tiff_lzw_decode: the compressed segments go
up as they are, one wave decodes each) - there is no host LZW decoder here, a pure-Python one needs minutes for a real DEM.  With
`device=` the decoded segments are put together there too (rdr_tiff_assemble: padding clipped, bytes swapped, predictor undone) and
the raster never exists on the host; without it, and without LZW, everything is NumPy and no GPU is needed.  The writer deflates its
strips with zlib on the host or, with `encoder='device'`, on the GPU in one call (rdr_tiff_predict, rdr_deflate_encode).

Georeferencing as GDAL reads it: ModelPixelScale + ModelTiepoint or ModelTransformation -> the six-number geotransform (a raster-space
PixelIsPoint moves it by half a pixel), the GeoKey directory -> an EPSG code (ProjectedCSTypeGeoKey, else GeographicTypeGeoKey, else
None), GDAL_NODATA -> nodata, GDAL_METADATA's AREA_OR_POINT -> tags."""
import re
import struct
import zlib
from pathlib import Path

import numpy as np


class UnsupportedTIFFFeature(NotImplementedError):
    """The file is a TIFF, and uses something this reader does not implement; the message names it."""


class NotATIFF(OSError):
    pass


_TYPE_FMT = {1: 'B', 2: 'c', 3: 'H', 4: 'I', 5: 'II', 6: 'b', 7: 'B', 8: 'h', 9: 'i', 10: 'ii', 11: 'f', 12: 'd', 13: 'I', 16: 'Q', 17: 'q', 18: 'Q'}
_COMPRESSION_NAMES = {2: 'CCITT RLE', 3: 'CCITT Group 3 fax', 4: 'CCITT Group 4 fax', 6: 'old-style JPEG', 7: 'JPEG', 34712: 'JPEG 2000', 34887: 'LERC',
                      34925: 'LZMA', 50000: 'ZSTD', 50001: 'WebP', 50002: 'JPEG XL'}
_PHOTOMETRIC_REFUSED = {3: 'palette (colour-mapped) photometric interpretation', 6: 'YCbCr photometric interpretation'}
_SAMPLE_KIND = {1: 'u', 2: 'i', 3: 'f'}
# tags
_W, _H, _BPS, _COMP, _PHOTO, _STRIP_OFF, _SPP, _RPS, _STRIP_CNT, _PLANAR, _PRED = 256, 257, 258, 259, 262, 273, 277, 278, 279, 284, 317
_TILE_W, _TILE_H, _TILE_OFF, _TILE_CNT, _SFMT = 322, 323, 324, 325, 339
_SCALE, _TIEPOINT, _TRANSFORM, _GEOKEYS, _GEODOUBLE, _GEOASCII, _GDAL_META, _GDAL_NODATA = 33550, 33922, 34264, 34735, 34736, 34737, 42112, 42113


def is_tiff(path):
    """The first four bytes are a classic TIFF or BigTIFF header."""
    try:
        with open(path, 'rb') as f:
            h = f.read(4)
    except OSError:
        return False
    return h in (b'II*\x00', b'MM\x00*', b'II+\x00', b'MM\x00+')


def _read_ifd(f, path):
    """{tag: value tuple / bytes} of the first IFD, plus (byte order, is BigTIFF)."""
    head = f.read(16)
    if len(head) < 8 or head[:2] not in (b'II', b'MM'):
        raise NotATIFF(f'{path}: not a TIFF file')
    bo = '<' if head[:2] == b'II' else '>'
    magic = struct.unpack(bo + 'H', head[2:4])[0]
    if magic == 42:
        big, off = False, struct.unpack(bo + 'I', head[4:8])[0]
    elif magic == 43:
        size, zero, off = struct.unpack(bo + 'HHQ', head[4:16])
        if size != 8 or zero != 0:
            raise NotATIFF(f'{path}: malformed BigTIFF header')
        big = True
    else:
        raise NotATIFF(f'{path}: not a TIFF file (magic {magic})')
    f.seek(0, 2)
    fsize = f.tell()
    cnt_fmt, ent_size, val_size = ('Q', 20, 8) if big else ('H', 12, 4)
    if off + struct.calcsize(cnt_fmt) > fsize:
        raise NotATIFF(f'{path}: the first directory lies beyond the end of the file')
    f.seek(off)
    n = struct.unpack(bo + cnt_fmt, f.read(struct.calcsize(cnt_fmt)))[0]
    raw = f.read(n * ent_size)
    if len(raw) != n * ent_size:
        raise NotATIFF(f'{path}: truncated directory')
    tags = {}
    for i in range(n):
        e = raw[i * ent_size:(i + 1) * ent_size]
        tag, typ = struct.unpack(bo + 'HH', e[:4])
        count = struct.unpack(bo + ('Q' if big else 'I'), e[4:4 + val_size])[0]
        fmt = _TYPE_FMT.get(typ)
        if fmt is None:
            continue                                    # a field type from a later specification: the tag is skipped, as the standard asks
        nbytes = struct.calcsize('=' + fmt) * count
        if nbytes <= val_size:
            data = e[4 + val_size:4 + val_size + nbytes]
        else:
            pos = struct.unpack(bo + ('Q' if big else 'I'), e[4 + val_size:])[0]
            if pos + nbytes > fsize:
                raise NotATIFF(f'{path}: the value of tag {tag} lies beyond the end of the file')
            f.seek(pos)
            data = f.read(nbytes)
        if typ == 2:
            tags[tag] = data.split(b'\x00', 1)[0].decode('latin-1')
        elif typ == 7:
            tags[tag] = data
        else:
            tags[tag] = np.frombuffer(data, dtype=np.dtype(bo + np.dtype(fmt[0]).str[1:])).reshape(count, len(fmt)) if len(fmt) > 1 else \
                np.frombuffer(data, dtype=np.dtype(fmt[0]).newbyteorder(bo))
    return tags, bo, big, fsize


def _one(tags, tag, default=None):
    v = tags.get(tag)
    if v is None:
        return default
    return v if isinstance(v, (str, bytes)) else v.ravel()[0].item()


def _geotransform(tags):
    """GDAL's six numbers, or None; `rotated` geotransforms (a ModelTransformation with off-diagonal terms) come out as they are."""
    gt = None
    if _TRANSFORM in tags and len(tags[_TRANSFORM]) >= 16:
        m = [float(v) for v in tags[_TRANSFORM]]
        gt = [m[3], m[0], m[1], m[7], m[4], m[5]]
    elif _SCALE in tags and _TIEPOINT in tags and len(tags[_SCALE]) >= 2 and len(tags[_TIEPOINT]) >= 6:
        sx, sy = float(tags[_SCALE][0]), float(tags[_SCALE][1])
        i, j, _, x, y = (float(v) for v in tags[_TIEPOINT][:5])
        gt = [x - i * sx, sx, 0.0, y + j * sy, 0.0, -sy]
    if gt is None:
        return None
    if _geokey(tags, 1025) == 2:                          # GTRasterTypeGeoKey = RasterPixelIsPoint: the tie point is a pixel CENTRE
        gt[0] -= 0.5 * gt[1] + 0.5 * gt[2]
        gt[3] -= 0.5 * gt[4] + 0.5 * gt[5]
    return tuple(gt)


def _geokey(tags, key):
    """A SHORT-valued GeoKey stored in the directory itself (location 0), or None."""
    d = tags.get(_GEOKEYS)
    if d is None or len(d) < 4:
        return None
    d = [int(v) for v in d]
    for k in range(min(d[3], (len(d) - 4) // 4)):
        kid, loc, cnt, val = d[4 + 4 * k:8 + 4 * k]
        if kid == key and loc == 0:
            return val
    return None


def _epsg(tags):
    for key in (3072, 2048):                              # ProjectedCSTypeGeoKey, then GeographicTypeGeoKey
        v = _geokey(tags, key)
        if v is not None and v not in (0, 32767):         # (undefined, user-defined)
            return v
    return None


def _nodata(tags):
    v = tags.get(_GDAL_NODATA)
    if not isinstance(v, str) or not v.strip():
        return None
    try:
        return float(v.strip())
    except ValueError:
        return None


class TiffInfo:
    """The first image of a TIFF file: layout, sample type, segment table, georeferencing.  Raises UnsupportedTIFFFeature for what
    cannot be read."""

    def __init__(self, path):
        self.path = Path(path)
        with open(self.path, 'rb') as f:
            tags, self.byteorder, self.bigtiff, self.file_size = _read_ifd(f, self.path)
        self.ifd = tags
        p = str(self.path)
        try:
            self.width, self.height = int(_one(tags, _W)), int(_one(tags, _H))
        except TypeError:
            raise NotATIFF(f'{p}: no ImageWidth / ImageLength')
        self.count = int(_one(tags, _SPP, 1))
        bps = [int(v) for v in tags.get(_BPS, np.array([1]))]
        sfmt = [int(v) for v in tags.get(_SFMT, np.array([1]))]
        if len(set(bps)) != 1 or len(set(sfmt)) != 1:
            raise UnsupportedTIFFFeature(f'{p}: bands of different sample types (BitsPerSample {bps}, SampleFormat {sfmt})')
        if bps[0] % 8 != 0:
            raise UnsupportedTIFFFeature(f'{p}: sub-byte samples (BitsPerSample = {bps[0]})')
        kind = _SAMPLE_KIND.get(sfmt[0] if sfmt[0] != 4 else 1)
        name = f'{kind}{bps[0] // 8}' if kind else None
        if name not in ('u1', 'u2', 'u4', 'i1', 'i2', 'i4', 'f4', 'f8'):
            raise UnsupportedTIFFFeature(f'{p}: sample type BitsPerSample = {bps[0]}, SampleFormat = {sfmt[0]} (uint8/16/32, int8/16/32 and float32/64 are read)')
        self.dtype = np.dtype(name)
        self.compression = int(_one(tags, _COMP, 1))
        if self.compression not in (1, 5, 8, 32946, 32773):
            raise UnsupportedTIFFFeature(f'{p}: {_COMPRESSION_NAMES.get(self.compression, "unknown")} compression (Compression = {self.compression})')
        photo = int(_one(tags, _PHOTO, 1))
        if photo in _PHOTOMETRIC_REFUSED:
            raise UnsupportedTIFFFeature(f'{p}: {_PHOTOMETRIC_REFUSED[photo]}')
        self.predictor = int(_one(tags, _PRED, 1))
        if self.predictor == 3:
            raise UnsupportedTIFFFeature(f'{p}: floating-point predictor (Predictor = 3)')
        if self.predictor not in (1, 2):
            raise UnsupportedTIFFFeature(f'{p}: Predictor = {self.predictor}')
        if self.compression in (1, 32773):
            self.predictor = 1                          # the predictor belongs to the LZW / deflate codecs: libtiff ignores the tag elsewhere
        self.planar = int(_one(tags, _PLANAR, 1))
        if self.planar not in (1, 2):
            raise UnsupportedTIFFFeature(f'{p}: PlanarConfiguration = {self.planar}')
        if self.count == 1:
            self.planar = 1
        self.tiled = _TILE_W in tags
        if self.tiled:
            self.tile_w, self.tile_h = int(_one(tags, _TILE_W)), int(_one(tags, _TILE_H))
            off, cnt = tags.get(_TILE_OFF), tags.get(_TILE_CNT)
        else:
            self.tile_w = self.width
            self.tile_h = min(int(_one(tags, _RPS, self.height)), self.height)
            off, cnt = tags.get(_STRIP_OFF), tags.get(_STRIP_CNT)
        if off is None or cnt is None or self.tile_w <= 0 or self.tile_h <= 0 or self.width <= 0 or self.height <= 0 or self.count <= 0:
            raise NotATIFF(f'{p}: no segment offsets / byte counts, or a zero size')
        self.tiles_x = -(-self.width // self.tile_w)
        self.tiles_y = -(-self.height // self.tile_h)
        self.spp_seg = 1 if self.planar == 2 else self.count
        nseg = self.tiles_x * self.tiles_y * (self.count if self.planar == 2 else 1)
        self.offsets = np.asarray(off, dtype=np.int64)
        self.bytecounts = np.asarray(cnt, dtype=np.int64)
        if len(self.offsets) != nseg or len(self.bytecounts) != nseg:
            raise NotATIFF(f'{p}: {len(self.offsets)} segment offsets for {nseg} segments')
        if np.any(self.offsets < 0) or np.any(self.bytecounts < 0) or np.any(self.offsets + self.bytecounts > self.file_size):
            raise NotATIFF(f'{p}: a segment lies beyond the end of the file')
        self.transform = _geotransform(tags)
        self.crs = _epsg(tags)
        self.nodata = _nodata(tags)
        self.tags = {}
        meta = tags.get(_GDAL_META)
        if isinstance(meta, str):
            for m in re.finditer(r'<Item\s+name="([^"]+)"[^>]*>([^<]*)</Item>', meta):
                self.tags[m.group(1)] = m.group(2).replace('&lt;', '<').replace('&gt;', '>').replace('&amp;', '&')
        if 'AREA_OR_POINT' not in self.tags and _geokey(tags, 1025) in (1, 2):
            self.tags['AREA_OR_POINT'] = 'Point' if _geokey(tags, 1025) == 2 else 'Area'

    @property
    def swap(self):
        import sys
        return self.dtype.itemsize > 1 and (self.byteorder == '<') != (sys.byteorder == 'little')

    def seg_rows(self, k):
        """Rows a decoded segment holds: tiles are always whole, the last strip may be short."""
        if self.tiled:
            return self.tile_h
        ty = (k % (self.tiles_x * self.tiles_y)) // self.tiles_x
        return min(self.tile_h, self.height - ty * self.tile_h)

    def seg_bytes(self, k):
        return self.seg_rows(k) * self.tile_w * self.spp_seg * self.dtype.itemsize

    def profile(self):
        return dict(driver='GTiff', dtype=str(self.dtype), nodata=self.nodata, width=self.width, height=self.height, count=self.count, crs=self.crs,
                    transform=self.transform, tags=dict(self.tags))

    def north_up_transform(self):
        """The geotransform for a caller that needs a north-up raster; a rotated one is refused by name."""
        gt = self.transform
        if gt is not None and (gt[2] != 0.0 or gt[4] != 0.0):
            raise UnsupportedTIFFFeature(f'{self.path}: rotated or sheared geotransform (ModelTransformation with off-diagonal terms) where a north-up raster is needed')
        return gt


def _unpackbits(data, expect):
    """PackBits (TIFF 6.0 section 9)."""
    out = bytearray()
    i, n = 0, len(data)
    while i < n and len(out) < expect:
        c = data[i]
        i += 1
        if c < 128:
            out += data[i:i + c + 1]
            i += c + 1
        elif c > 128:
            if i >= n:
                break
            out += data[i:i + 1] * (257 - c)
            i += 1
    return bytes(out[:expect])


def _host_segment(info, raw, k):
    """Segment k decoded on the host: exactly seg_bytes(k) bytes (zero-filled where the stream is short)."""
    need = info.seg_bytes(k)
    if info.compression == 1:
        data = raw
    elif info.compression in (8, 32946):
        try:
            data = zlib.decompress(raw)
        except zlib.error as e:
            raise NotATIFF(f'{info.path}: segment {k}: deflate stream is damaged ({e})')
    else:
        data = _unpackbits(raw, need)
    if len(data) < need:
        data = data + bytes(need - len(data))
    return data[:need]


def _check_lzw_flavour(info, first2):
    if len(first2) >= 2 and first2[0] == 0 and (first2[1] & 1):
        raise UnsupportedTIFFFeature(f'{info.path}: old-style LZW (LSB-first codes, written by pre-1990s software)')


def _assemble_host(info, segs, band):
    """NumPy restatement of rdr_tiff_assemble over host-decoded segments; (bands, H, W) or (H, W)."""
    dt_file = info.dtype.newbyteorder(info.byteorder)
    udt = np.dtype(f'u{info.dtype.itemsize}')
    nb = info.count
    out = np.empty((nb if band is None else 1, info.height, info.width), dtype=info.dtype)
    per_plane = info.tiles_x * info.tiles_y
    for k, data in enumerate(segs):
        plane, ts = divmod(k, per_plane)
        if info.planar == 2 and band is not None and plane != band:
            continue
        ty, tx = divmod(ts, info.tiles_x)
        rows = info.seg_rows(k)
        a = np.frombuffer(data, dtype=dt_file, count=rows * info.tile_w * info.spp_seg).reshape(rows, info.tile_w, info.spp_seg)
        a = a.astype(info.dtype)
        if info.predictor == 2:
            a = np.cumsum(a.view(udt), axis=1, dtype=udt).view(info.dtype)
        y0, x0 = ty * info.tile_h, tx * info.tile_w
        ny, nx = min(rows, info.height - y0), min(info.tile_w, info.width - x0)
        if info.planar == 2:
            out[plane if band is None else 0, y0:y0 + ny, x0:x0 + nx] = a[:ny, :nx, 0]
        elif band is None:
            out[:, y0:y0 + ny, x0:x0 + nx] = a[:ny, :nx, :].transpose(2, 0, 1)
        else:
            out[0, y0:y0 + ny, x0:x0 + nx] = a[:ny, :nx, band]
    return out


def _torch_dtype(dt):
    import torch
    name = {'u1': 'uint8', 'u2': 'uint16', 'u4': 'uint32', 'i1': 'int8', 'i2': 'int16', 'i4': 'int32', 'f4': 'float32', 'f8': 'float64'}[dt.kind + str(dt.itemsize)]
    if not hasattr(torch, name):
        raise UnsupportedTIFFFeature(f'{name} samples as a device tensor (this torch build has no torch.{name})')
    return getattr(torch, name)


def lzw_decode_device(src, seg_offset, seg_bytes, seg_out_bytes, out, out_stride):
    """rdr_tiff_lzw_decode on device tensors: `src` / `out` uint8 tensors on the GPU, the three tables int64 NumPy arrays; returns the int32
    status tensor (0 ok, 1 short, 2 bad code), one per segment."""
    import torch
    from . import _lib as L
    ctx = L.Context.default()
    so, sb, cap = (np.ascontiguousarray(v, dtype=np.int64) for v in (seg_offset, seg_bytes, seg_out_bytes))
    n = so.size
    if sb.size != n or cap.size != n:
        raise ValueError('the three segment tables differ in length')
    if out.numel() < n * int(out_stride):
        raise ValueError(f'out holds {out.numel()} bytes, {n} slots of {out_stride} are needed')
    if src.dtype != torch.uint8 or out.dtype != torch.uint8 or not src.is_contiguous() or not out.is_contiguous():
        raise TypeError('src and out are contiguous uint8 tensors')
    status = torch.full((n,), -1, dtype=torch.int32, device=out.device)
    ctx.adopt_torch_stream(out)
    L.check(ctx.lib.rdr_tiff_lzw_decode(ctx.handle, L.ptr(src), src.numel(), L.ptr(so), L.ptr(sb), n, L.ptr(cap), L.ptr(out), int(out_stride), L.ptr(status),
                                        L.RDR_DEVICE), ctx.handle)
    return status


def assemble_device(segs, seg_stride, height, width, tile_h, tile_w, predictor, swap, dtype, planar, bands, band, device=None):
    """rdr_tiff_assemble on a uint8 device tensor of decoded segments; returns the (H, W) tensor of 0-based `band`, or (bands, H, W) for None."""
    import torch
    from . import _lib as L
    ctx = L.Context.default()
    dt = np.dtype(dtype)
    nb = bands if band is None else 1
    raw = torch.empty(nb * height * width * dt.itemsize, dtype=torch.uint8, device=segs.device)
    ctx.adopt_torch_stream(segs)
    L.check(ctx.lib.rdr_tiff_assemble(ctx.handle, L.ptr(segs), int(seg_stride), height, width, tile_h, tile_w, predictor, int(bool(swap)), dt.itemsize, planar, bands,
                                      -1 if band is None else int(band), L.ptr(raw), L.RDR_DEVICE), ctx.handle)
    return raw, ((nb, height, width) if band is None else (height, width))


def _gpu_device(device):
    import torch
    if device is None:
        if not torch.cuda.is_available():
            raise RuntimeError("LZW-compressed GeoTIFFs, and deflate ones read with inflate='device', are decoded on the GPU (rdr_tiff_lzw_decode, "
                               'rdr_inflate_decode); no GPU is visible and there is no CPU fallback')
        return torch.device('cuda', torch.cuda.current_device())
    device = torch.device(device)
    if device.type != 'cuda':
        raise TypeError(f'device must be a GPU, not {device}')
    return device


# inflate='auto': deflate segments from which the device route is taken.  Measured (tools/bench_inflate.py, profiles/r24_inflate.json): a
# 4000 x 4000 int16 DEM read to a device tensor in 64 segments takes 119 ms on the device route against 71 ms through zlib, in 256
# segments 32 ms against 80 ms - one wave decodes one segment, so the route pays only once a few hundred waves run side by side.
_INFLATE_MIN_SEGMENTS = 256
# Fewer segments, but long ones that the split decoder cuts at their flush points: segments + flush points (_inflate_units) from which the
# device route is taken.  Measured (tools/bench_inflate_split.py, profiles/r28_inflate_split.json) on float32 rasters in 8 or 16
# device-written strips: 264 units 26.7 ms on the device against 21.7 ms through zlib (not ahead: two passes over one 32 KiB piece on one
# lane are a floor of about 30 ms), 528 units 37.2 against 43.7 ms, 1024 units 60.7 against 85.5 ms, 1984 units 93.8 against 170.3 ms.
# One segment alone stays on the host whatever it holds (32 MB in 683 pieces: 57.0 against 58.8 ms, inside the spans).  Not told apart
# before the measure pass, and slower on this route: segments whose flush points keep the history (Z_SYNC_FLUSH), which collapse to one
# piece each and then run the serial kernel - libtiff and GDAL write none; inflate='host' is the way round them.
_INFLATE_MIN_PIECES = 512


def _inflate_units(info, whole=None):
    """What the device route decodes side by side: the segments and the flush points inside them, at which rdr_inflate_decode_split
    cuts a long segment into pieces (deflate.flush_points).  whole: the file's bytes as a uint8 array, when they have been read."""
    from .deflate import flush_points
    if whole is None:
        whole = np.fromfile(info.path, dtype=np.uint8)
    return len(info.offsets) + sum(flush_points(whole[int(o):int(o) + int(c)]) for o, c in zip(info.offsets, info.bytecounts))


def _read_device(info, band, device, inflate='host', whole=None):
    """The decode through the two kernels; a uint8 tensor holding the raster's bytes, and its shape.  inflate: where deflate segments
    are decoded, 'host' or 'device'.  whole: the file's bytes as a uint8 array when the caller has read them already."""
    import torch
    nseg = len(info.offsets)
    full = info.tile_h * info.tile_w * info.spp_seg * info.dtype.itemsize
    stride = (full + 15) // 16 * 16
    if info.compression == 5:
        whole = np.fromfile(info.path, dtype=np.uint8)
        first = int(info.offsets[0])
        _check_lzw_flavour(info, whole[first:first + 2])
        src = torch.from_numpy(whole).to(device)
        segs = torch.zeros(nseg * stride, dtype=torch.uint8, device=device)
        need = np.array([info.seg_bytes(k) for k in range(nseg)], dtype=np.int64)
        status = lzw_decode_device(src, info.offsets, info.bytecounts, need, segs, stride).cpu().numpy()
        bad = np.nonzero(status)[0]
        if bad.size:
            what = {1: 'ends early or holds more than the segment takes', 2: 'holds a code beyond the string table'}.get(int(status[bad[0]]), 'failed')
            raise NotATIFF(f'{info.path}: the LZW stream of segment {int(bad[0])} {what} ({bad.size} of {nseg} segments damaged)')
    elif info.compression in (8, 32946) and inflate == 'device':
        # the file's bytes go up, rdr_inflate_decode writes the (zeroed) slots; a segment it does not accept is decoded again on the
        # host and patched in, so that the host route's result - a truncated over-long stream - or its exception stands
        from . import deflate
        if whole is None:
            whole = np.fromfile(info.path, dtype=np.uint8)
        src = torch.from_numpy(whole).to(device)
        need = np.array([info.seg_bytes(k) for k in range(nseg)], dtype=np.int64)
        segs, status, _ = deflate.inflate_segments(src, info.offsets, info.bytecounts, need, out_stride=stride, split=True)
        for k in np.nonzero(status.cpu().numpy())[0]:
            k = int(k)
            o = int(info.offsets[k])
            d = _host_segment(info, whole[o:o + int(info.bytecounts[k])].tobytes(), k)
            segs[k * stride:k * stride + len(d)] = torch.from_numpy(np.frombuffer(d, dtype=np.uint8).copy()).to(device)
    else:
        buf = np.zeros(nseg * stride, dtype=np.uint8)
        if whole is not None:                                    # (read by the caller to choose the route: not read again)
            for k in range(nseg):
                o = int(info.offsets[k])
                d = _host_segment(info, whole[o:o + int(info.bytecounts[k])].tobytes(), k)
                buf[k * stride:k * stride + len(d)] = np.frombuffer(d, dtype=np.uint8)
        else:
            with open(info.path, 'rb') as f:
                for k in range(nseg):
                    f.seek(int(info.offsets[k]))
                    d = _host_segment(info, f.read(int(info.bytecounts[k])), k)
                    buf[k * stride:k * stride + len(d)] = np.frombuffer(d, dtype=np.uint8)
        segs = torch.from_numpy(buf).to(device)
    return assemble_device(segs, stride, info.height, info.width, info.tile_h, info.tile_w, info.predictor, info.swap, info.dtype, info.planar, info.count, band)


def read(path, band=None, device=None, inflate='auto'):
    """(array, profile) of the first image of a GeoTIFF.  band: 1-based, None = every band ((H, W) for a one-band file, else (bands, H, W)).
    device: a torch GPU device - the array is a tensor there and the decoded raster never exists on the host; None - a NumPy array
    (LZW files still pass through the GPU, which decodes them; all others are read without one).  inflate: where deflate segments
    are decoded - 'host' (zlib), 'device' (rdr_inflate_decode_split; with device=None the result is downloaded) or 'auto' (the device when
    `device` is given and the file has _INFLATE_MIN_SEGMENTS segments, or more than one and, with the flush points inside them,
    _INFLATE_MIN_PIECES).  Both routes give the same pixels and errors."""
    from .deflate import inflate_mode
    inflate = inflate_mode(inflate)
    info = TiffInfo(path)
    if band is not None and not 1 <= int(band) <= info.count:
        raise IndexError(f'{path}: band {band} of {info.count}')
    b0 = None if band is None else int(band) - 1
    deflated = info.compression in (8, 32946)
    whole = None
    if inflate == 'auto':
        inflate = 'host'
        if deflated and device is not None:
            nseg = len(info.offsets)
            if nseg >= _INFLATE_MIN_SEGMENTS:
                inflate = 'device'
            elif nseg > 1:
                # fewer segments, but long ones may be cut at their flush points: the file is read once, here, and the chosen route
                # decodes from these bytes.  A file of ONE segment stays on the host: measured, not ahead (see _INFLATE_MIN_PIECES)
                whole = np.fromfile(info.path, dtype=np.uint8)
                if _inflate_units(info, whole) >= _INFLATE_MIN_PIECES:
                    inflate = 'device'
    if device is not None or info.compression == 5 or (deflated and inflate == 'device'):
        raw, shape = _read_device(info, b0, _gpu_device(device), inflate, whole)
        if device is not None:
            arr = raw.view(_torch_dtype(info.dtype)).reshape(shape)
        else:
            arr = raw.cpu().numpy().view(info.dtype).reshape(shape)
    else:
        with open(info.path, 'rb') as f:
            segs = []
            for k in range(len(info.offsets)):
                f.seek(int(info.offsets[k]))
                segs.append(_host_segment(info, f.read(int(info.bytecounts[k])), k))
        arr = _assemble_host(info, segs, b0)
        arr = arr[0] if band is not None else arr
    if band is None and info.count == 1 and len(arr.shape) == 3:
        arr = arr[0]
    return arr, info.profile()


class TiffRaster:
    """The part of a rasterio dataset the delay path uses (see rawraster.RawRaster), over a GeoTIFF."""

    def __init__(self, path):
        path = Path(path)
        if not path.exists():
            raise FileNotFoundError(f'{path}: No such file or directory')
        self._info = TiffInfo(path)
        self.profile = self._info.profile()
        self.count, self.height, self.width = self._info.count, self._info.height, self._info.width
        self.nodatavals = (self._info.nodata,) * self.count

    def read(self, band=None):
        if band is not None:
            return read(self._info.path, band=band)[0]
        a = read(self._info.path)[0]
        return a[None] if a.ndim == 2 else a

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


# ---- writer ------------------------------------------------------------------------------------------------------------------------
_BIGTIFF_ABOVE = 0xFFFF0000                               # strip bytes + tables beyond this many bytes: classic 32-bit offsets no longer reach
_WRITE_TYPES = {'uint8': (8, 1), 'uint16': (16, 1), 'int16': (16, 2), 'float32': (32, 3), 'float64': (64, 3)}


def _epsg_of(proj):
    """EPSG code of what writeDelays hands on as `proj` (None, an int, 'EPSG:n', a WKT, an object with to_epsg), or None."""
    if proj is None:
        return None
    if hasattr(proj, 'to_epsg'):
        return proj.to_epsg()
    if isinstance(proj, (int, np.integer)):
        return int(proj)
    txt = str(proj).strip()
    m = re.fullmatch(r'(?:EPSG:)?(\d+)', txt, flags=re.I)
    if m:
        return int(m.group(1))
    if '[' in txt:
        from .crs import crs_from_wkt
        try:
            c = crs_from_wkt(txt)
        except ValueError:
            return None
        return c if isinstance(c, int) else None
    return None


def _is_geographic(epsg):
    """EPSG's geographic 2-D codes live in 4000 - 4999 (4326 WGS 84, 4269 NAD83, ...); everything else written here is projected."""
    return 4000 <= epsg <= 4999


def _device_strips(array, h, w, itemsize, rps, predictor, tables):
    """The strips of `array` (NumPy or device tensor) as zlib streams from the device encoder: the predictor as a kernel of its own
    (rdr_tiff_predict), every strip in ONE rdr_deflate_encode_tables call, one download of the packed streams."""
    import torch
    from . import _lib as L
    from . import deflate as D
    if not torch.cuda.is_available():
        raise RuntimeError("tifflite.write(encoder='device') deflates the strips on the GPU (rdr_deflate_encode); no GPU is visible - use encoder='host'")
    t = array if D._is_tensor(array) else torch.from_numpy(np.ascontiguousarray(array)).cuda()
    if not t.is_cuda:
        t = t.cuda()
    t = t.contiguous().reshape(-1).view(torch.uint8)
    if predictor == 2:
        ctx = L.Context.default()
        ctx.adopt_torch_stream(t)
        d = torch.empty_like(t)
        L.check(ctx.lib.rdr_tiff_predict(ctx.handle, L.ptr(t), itemsize, h, w, L.ptr(d), L.RDR_DEVICE), ctx.handle)
        t = d
    row_bytes = w * itemsize
    offs = np.arange(0, h, rps, dtype=np.int64) * row_bytes
    sizes = np.minimum(rps, h - np.arange(0, h, rps, dtype=np.int64)) * row_bytes
    packed, oo = D.deflate_segments(t, offs, sizes, tables=tables)
    packed = packed.cpu().numpy()
    return [packed[oo[i]:oo[i + 1]] for i in range(offs.size)]


def write(path, array, transform=None, crs=None, nodata=None, compress=None, rows_per_strip=None, predictor=None, encoder='host', tables='fixed', tags=None):
    """One band as a GeoTIFF in strips: classic TIFF, BigTIFF when the pixels pass 4 GiB; little-endian; compress None or 'deflate'
    (zlib).  array: 2-D uint16 / int16 / float32 / float64 (and uint8, what the delay writers make of integer arrays).  transform: GDAL's six numbers (north-up); crs: an EPSG code (see _epsg_of);
    nodata: written as GDAL_NODATA.  predictor: None, or 2 (with 'deflate': every row differenced along x in the unsigned integer type
    of the sample width, tag 317 - what the readers undo).  encoder: 'host' (zlib level 6), or 'device' (with 'deflate': the strips
    are deflated on the GPU in one call; array may then be a device tensor, and no GPU is an error by name).  tables: 'fixed', or
    'dynamic' (with encoder='device': dynamic-Huffman blocks wherever they are the smallest).  tags: None, or a dict written as the items
    of GDAL_METADATA (tag 42112) - what `read` hands back as profile['tags']; None leaves the tag out."""
    if compress not in (None, 'none', 'deflate', 'DEFLATE'):
        raise ValueError(f"compress must be None or 'deflate', not {compress!r}")
    deflate = compress in ('deflate', 'DEFLATE')
    if predictor not in (None, 1, 2):
        raise ValueError(f'predictor must be None or 2, not {predictor!r}')
    predictor = 2 if predictor == 2 else None
    if encoder not in ('host', 'device'):
        raise ValueError(f"encoder must be 'host' or 'device', not {encoder!r}")
    if (predictor or encoder == 'device') and not deflate:
        raise ValueError("predictor=2 and encoder='device' belong to compress='deflate'")
    if tables not in ('fixed', 'dynamic'):
        raise ValueError(f"tables must be 'fixed' or 'dynamic', not {tables!r}")
    if tables == 'dynamic' and encoder != 'device':
        raise ValueError("tables='dynamic' belongs to encoder='device'")
    tensor = type(array).__module__.split('.')[0] == 'torch'
    if tensor and encoder != 'device':
        array = array.cpu().numpy()
        tensor = False
    a = None if tensor else np.asarray(array)
    shape = tuple(array.shape) if tensor else a.shape
    dtype = np.dtype(str(array.dtype).replace('torch.', '')) if tensor else a.dtype
    if len(shape) != 2:
        raise RuntimeError(f'tifflite.write: cannot write an array of shape {shape} to a raster image')
    if dtype.name not in _WRITE_TYPES:
        raise TypeError(f'tifflite.write: uint8, uint16, int16, float32 and float64 are written, not {dtype}')
    bits, sfmt = _WRITE_TYPES[dtype.name]
    if a is not None:
        a = np.ascontiguousarray(a.astype(a.dtype.newbyteorder('<'), copy=False))
    h, w = shape
    if h == 0 or w == 0:
        raise ValueError('tifflite.write: empty raster')
    row_bytes = w * dtype.itemsize
    rps = int(rows_per_strip) if rows_per_strip else max(1, (1 << 16) // row_bytes)
    rps = min(max(rps, 1), h)
    if encoder == 'device':
        strips = _device_strips(array if tensor else a, h, w, dtype.itemsize, rps, predictor, tables)
    else:
        strips = []
        for y in range(0, h, rps):
            rows = a[y:y + rps]
            if predictor:
                u = rows.view(f'<u{dtype.itemsize}')
                rows = u.copy()
                rows[:, 1:] -= u[:, :-1]
            b = rows.tobytes()
            strips.append(zlib.compress(b, 6) if deflate else b)
    data_bytes = sum(len(s) for s in strips)
    big = data_bytes + 16 * len(strips) + 4096 > _BIGTIFF_ABOVE
    epsg = _epsg_of(crs)
    entries = []                                          # (tag, type, values)
    off_t = 16 if big else 4
    entries += [(_W, 4, [w]), (_H, 4, [h]), (_BPS, 3, [bits]), (_COMP, 3, [8 if deflate else 1]), (_PHOTO, 3, [1]), (_STRIP_OFF, off_t, None), (_SPP, 3, [1]),
                (_RPS, 4, [rps]), (_STRIP_CNT, off_t, [len(s) for s in strips]), (_PLANAR, 3, [1]), (_SFMT, 3, [sfmt])]
    if predictor:
        entries.append((_PRED, 3, [2]))
    if transform is not None:
        gt = [float(v) for v in (transform.to_gdal() if hasattr(transform, 'to_gdal') else transform)]
        if gt[2] != 0.0 or gt[4] != 0.0:
            entries.append((_TRANSFORM, 12, [gt[1], gt[2], 0.0, gt[0], gt[4], gt[5], 0.0, gt[3], 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]))
        else:
            entries += [(_SCALE, 12, [gt[1], -gt[5], 0.0]), (_TIEPOINT, 12, [0.0, 0.0, 0.0, gt[0], gt[3], 0.0])]
    if epsg is not None:
        if _is_geographic(epsg):
            keys = [1, 1, 0, 3, 1024, 0, 1, 2, 1025, 0, 1, 1, 2048, 0, 1, epsg]
        else:
            keys = [1, 1, 0, 3, 1024, 0, 1, 1, 1025, 0, 1, 1, 3072, 0, 1, epsg]
        entries.append((_GEOKEYS, 3, keys))
    elif transform is not None:
        entries.append((_GEOKEYS, 3, [1, 1, 0, 1, 1025, 0, 1, 1]))
    if nodata is not None:
        nd = float(nodata)
        txt = 'nan' if nd != nd else (str(int(nd)) if nd == int(nd) and abs(nd) < 1e15 else repr(nd))
        entries.append((_GDAL_NODATA, 2, txt))
    if tags:
        from xml.sax.saxutils import escape
        items = ''.join(f'  <Item name="{escape(str(k), {chr(34): "&quot;"})}">{escape(str(v))}</Item>\n' for k, v in tags.items())
        entries.append((_GDAL_META, 2, f'<GDALMetadata>\n{items}</GDALMetadata>\n'))
    entries.sort(key=lambda e: e[0])
    head = 16 if big else 8
    pos = head
    strip_offsets = []
    for s in strips:
        strip_offsets.append(pos)
        pos += len(s)
    pos += pos & 1                                        # directories start on a word boundary
    ifd_pos = pos
    ent_size, val_size, cnt_fmt, ptr_fmt = (20, 8, '<Q', '<Q') if big else (12, 4, '<H', '<I')
    extra_pos = ifd_pos + struct.calcsize(cnt_fmt) + len(entries) * ent_size + val_size
    ifd = bytearray(struct.pack(cnt_fmt, len(entries)))
    extra = bytearray()
    for tag, typ, vals in entries:
        if tag == _STRIP_OFF:
            vals = strip_offsets
        if typ == 2:
            payload = vals.encode('latin-1') + b'\x00'
            count = len(payload)
        else:
            payload = struct.pack('<' + _TYPE_FMT[typ] * len(vals), *vals)
            count = len(vals)
        ifd += struct.pack('<HH', tag, typ) + struct.pack('<Q' if big else '<I', count)
        if len(payload) <= val_size:
            ifd += payload + bytes(val_size - len(payload))
        else:
            ifd += struct.pack(ptr_fmt, extra_pos + len(extra))
            extra += payload + bytes(len(payload) & 1)
    ifd += struct.pack(ptr_fmt, 0)                        # no further directory
    path = Path(path)
    with open(path, 'wb') as f:
        f.write(struct.pack('<2sHHHQ', b'II', 43, 8, 0, ifd_pos) if big else struct.pack('<2sHI', b'II', 42, ifd_pos))
        for s in strips:
            f.write(s)
        if f.tell() & 1:
            f.write(b'\x00')
        f.write(ifd)
        f.write(extra)
    return str(path)
