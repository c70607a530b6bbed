"""The MPEG-1 encoder on the device (I pictures, or I + P with a GOP): the Python side of C ABI part 8 (include/jsmpeg_hip.h, jsmpeg_hip_encoder_*) and
the TS mux: on the device behind the pass (Encoder.set_ts), over any device bytes (ts_mux_device) and on the host (ts_mux).  Frames in HBM (a Batch's pool, a Live tick's pictures, any device pointers) or uint8 RGB torch tensors
-> elementary streams in a device buffer that Batch.attach_device takes as it is.  I pictures, or -- Encoder.set_gop -- I + P
with motion search on the device and a closed loop; one quantiser scale per picture, the caller's or -- Encoder.set_rate --
chosen on the device for a budget in bytes.  Frames of another size than the encoder's are cropped and scaled on the device,
plane by plane (Encoder.encode_scaled: renditions), and many sources are composed into one picture the same way
(Encoder.set_mosaic / encode_mosaic / encode_mosaic_latest: a wall of cameras).  torch is imported only when a tensor is handed in."""
import ctypes

import numpy as np

from . import batch as _batch

END = 1
CHAIN = 2        # continue the call's streams where their last chained call left them (JSMPEG_HIP_ENC_CHAIN)

SYMBOLS = ("jsmpeg_hip_encoder_create", "jsmpeg_hip_encoder_destroy", "jsmpeg_hip_encoder_encode", "jsmpeg_hip_encoder_encode_rgb",
           "jsmpeg_hip_encoder_sync", "jsmpeg_hip_encoder_query", "jsmpeg_hip_encoder_es", "jsmpeg_hip_encoder_stream_range",
           "jsmpeg_hip_encoder_picture_range", "jsmpeg_hip_encoder_read_es", "jsmpeg_hip_encoder_timings", "jsmpeg_hip_ts_mux_host",
           "jsmpeg_hip_encoder_set_gop", "jsmpeg_hip_encoder_recon", "jsmpeg_hip_encoder_picture_stats",
           "jsmpeg_hip_encoder_set_rate", "jsmpeg_hip_encoder_picture_rate", "jsmpeg_hip_encoder_chain_reset", "jsmpeg_hip_encoder_chain_info",
           "jsmpeg_hip_encoder_encode_scaled", "jsmpeg_hip_encoder_source",
           "jsmpeg_hip_encoder_set_mosaic", "jsmpeg_hip_encoder_encode_mosaic",
           "jsmpeg_hip_encoder_set_ts", "jsmpeg_hip_encoder_ts_pts", "jsmpeg_hip_encoder_ts", "jsmpeg_hip_encoder_ts_range",
           "jsmpeg_hip_encoder_ts_picture_range", "jsmpeg_hip_encoder_read_ts", "jsmpeg_hip_ts_bound", "jsmpeg_hip_ts_mux_device")

FRAME_RATES = {1: (24000, 1001), 2: (24, 1), 3: (25, 1), 4: (30000, 1001), 5: (30, 1), 6: (50, 1), 7: (60000, 1001), 8: (60, 1)}


def bytes_per_picture(bits_per_second, frame_rate_code=5):
    """the target of Encoder.set_rate for a bit rate: bits per second over 8 and the pictures per second of the sequence
    header's frame_rate_code (0: 5, as the handle reads it), rounded down, at least 1"""
    num, den = FRAME_RATES[frame_rate_code or 5]
    return max(1, int(bits_per_second) * den // (8 * num))



class EncoderConfig(ctypes.Structure):
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("max_pictures", ctypes.c_uint32),
                ("max_streams", ctypes.c_uint32), ("max_es_bytes", ctypes.c_uint64), ("frame_rate_code", ctypes.c_uint32),
                ("device", ctypes.c_int32)]


class EncSource(ctypes.Structure):
    """jsmpeg_hip_enc_source_t: the geometry of the frames an Encoder.encode_scaled call scales"""
    _fields_ = [(n, ctypes.c_uint32) for n in ("width", "height", "crop_x", "crop_y", "crop_width", "crop_height", "antialias")]


class EncCell(ctypes.Structure):
    """jsmpeg_hip_enc_cell_t: a cell of a mosaic layout -- the geometry of its frames and where they go in the picture"""
    _fields_ = [("source", EncSource)] + [(n, ctypes.c_uint32) for n in ("x", "y", "width", "height")]


def cell(source_size, x, y, width, height, crop=None, antialias=True):
    """an EncCell: frames of source_size = (width, height), cropped as in Encoder.encode_scaled, scaled to width x height and
    pasted at (x, y) -- both even -- of the encoder's picture"""
    src = EncSource(int(source_size[0]), int(source_size[1]), *([int(v) for v in crop] if crop is not None else [0, 0, 0, 0]), 1 if antialias else 0)
    return EncCell(src, int(x), int(y), int(width), int(height))


def grid(cols, rows, size, source_size, gap=0, crop=None, antialias=True):
    """the cells of a regular wall, row by row: cols x rows cells that share the `size` = (width, height) of the encoder's picture
    equally, `gap` pixels of fill between neighbours (none around the wall).  A cell's width is (size[0] - gap * (cols - 1)) //
    cols rounded DOWN to an even number, its x a multiple of width + gap (gap is rounded up to even), and the same for the rows:
    what is left over stays fill at the right and bottom.  Every cell reads frames of source_size with the same crop."""
    cols, rows, gap = int(cols), int(rows), (int(gap) + 1) & ~1
    if cols < 1 or rows < 1:
        raise ValueError("grid: %d x %d cells: at least one column and one row" % (cols, rows))
    cw, ch = ((size[0] - gap * (cols - 1)) // cols) & ~1, ((size[1] - gap * (rows - 1)) // rows) & ~1
    if cw < 2 or ch < 2:
        raise ValueError("grid: %d x %d cells with a gap of %d do not fit %d x %d" % (cols, rows, gap, size[0], size[1]))
    return [cell(source_size, c * (cw + gap), r * (ch + gap), cw, ch, crop, antialias) for r in range(rows) for c in range(cols)]


_bound = None


def lib():
    """libjsmpeg_hip with the part-8 argtypes set"""
    global _bound
    if _bound is None:
        L = _batch.lib()
        vp, u32, u64 = ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint64
        L.jsmpeg_hip_encoder_create.restype = vp
        L.jsmpeg_hip_encoder_create.argtypes = [ctypes.POINTER(EncoderConfig)]
        L.jsmpeg_hip_encoder_destroy.restype = None
        L.jsmpeg_hip_encoder_destroy.argtypes = [vp]
        L.jsmpeg_hip_encoder_encode.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_encode.argtypes = [vp, vp, vp, vp, u32, u32, u32, vp]
        L.jsmpeg_hip_encoder_encode_rgb.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_encode_rgb.argtypes = [vp, vp, u32, u32, vp, vp, u32, u32, u32, vp]
        for name in ("jsmpeg_hip_encoder_sync", "jsmpeg_hip_encoder_query"):
            getattr(L, name).restype = ctypes.c_int
            getattr(L, name).argtypes = [vp]
        L.jsmpeg_hip_encoder_es.restype = vp
        L.jsmpeg_hip_encoder_es.argtypes = [vp, ctypes.POINTER(u64)]
        L.jsmpeg_hip_encoder_stream_range.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_stream_range.argtypes = [vp, u32, ctypes.POINTER(u64), ctypes.POINTER(u64)]
        L.jsmpeg_hip_encoder_picture_range.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_picture_range.argtypes = [vp, u32, ctypes.POINTER(u64), ctypes.POINTER(u32)]
        L.jsmpeg_hip_encoder_read_es.restype = ctypes.c_int64
        L.jsmpeg_hip_encoder_read_es.argtypes = [vp, u32, vp, u64]
        L.jsmpeg_hip_encoder_timings.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_timings.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
        L.jsmpeg_hip_encoder_set_gop.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_set_gop.argtypes = [vp, u32, u32]
        L.jsmpeg_hip_encoder_recon.restype = vp
        L.jsmpeg_hip_encoder_recon.argtypes = [vp, u32]
        L.jsmpeg_hip_encoder_picture_stats.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_picture_stats.argtypes = [vp, u32, ctypes.POINTER(u32)]
        L.jsmpeg_hip_encoder_set_rate.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_set_rate.argtypes = [vp, u32, u32, u32, u32]
        L.jsmpeg_hip_encoder_picture_rate.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_picture_rate.argtypes = [vp, u32, ctypes.POINTER(u32)]
        L.jsmpeg_hip_encoder_chain_reset.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_chain_reset.argtypes = [vp, u32]
        L.jsmpeg_hip_encoder_chain_info.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_chain_info.argtypes = [vp, u32, ctypes.POINTER(u32)]
        L.jsmpeg_hip_encoder_encode_scaled.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_encode_scaled.argtypes = [vp, vp, ctypes.POINTER(EncSource), vp, vp, u32, u32, u32, vp]
        L.jsmpeg_hip_encoder_set_mosaic.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_set_mosaic.argtypes = [vp, ctypes.POINTER(EncCell), u32, u32]
        L.jsmpeg_hip_encoder_encode_mosaic.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_encode_mosaic.argtypes = [vp, vp, vp, vp, u32, u32, u32, vp]
        L.jsmpeg_hip_encoder_source.restype = vp
        L.jsmpeg_hip_encoder_source.argtypes = [vp, u32]
        L.jsmpeg_hip_ts_mux_host.restype = ctypes.c_int64
        L.jsmpeg_hip_ts_mux_host.argtypes = [vp, vp, vp, vp, u32, u32, u32, ctypes.POINTER(ctypes.c_uint8), vp, u64]
        L.jsmpeg_hip_encoder_set_ts.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_set_ts.argtypes = [vp, u32, u32, u64]
        L.jsmpeg_hip_encoder_ts_pts.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_ts_pts.argtypes = [vp, vp, u32]
        L.jsmpeg_hip_encoder_ts.restype = vp
        L.jsmpeg_hip_encoder_ts.argtypes = [vp, ctypes.POINTER(u64)]
        L.jsmpeg_hip_encoder_ts_range.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_ts_range.argtypes = [vp, u32, ctypes.POINTER(u64), ctypes.POINTER(u64), ctypes.POINTER(u32)]
        L.jsmpeg_hip_encoder_ts_picture_range.restype = ctypes.c_int
        L.jsmpeg_hip_encoder_ts_picture_range.argtypes = [vp, u32, ctypes.POINTER(u64), ctypes.POINTER(u32)]
        L.jsmpeg_hip_encoder_read_ts.restype = ctypes.c_int64
        L.jsmpeg_hip_encoder_read_ts.argtypes = [vp, u32, vp, u64]
        L.jsmpeg_hip_ts_bound.restype = u64
        L.jsmpeg_hip_ts_bound.argtypes = [u64, u32, u32]
        L.jsmpeg_hip_ts_mux_device.restype = ctypes.c_int64
        L.jsmpeg_hip_ts_mux_device.argtypes = [vp, vp, vp, vp, vp, u32, u32, u32, vp, u32, vp, u64, vp, vp]
        _bound = L
    return _bound


def pts_90k(pts):
    """seconds -> 90 kHz ticks, rounded as ts_mux() rounds"""
    return np.ascontiguousarray([int(round(float(t) * 90000.0)) for t in pts], dtype=np.uint64)


def ts_bound(es_bytes, units, streams=1):
    """a safe max_ts_bytes / ts_cap for es_bytes of payload in `units` units over `streams` streams"""
    return int(lib().jsmpeg_hip_ts_bound(int(es_bytes), int(units), int(streams)))


def ts_mux_device(dev_es, ranges, pts, dev_ts, ts_cap, streams=None, n_streams=None, stream_id=0xE0, pid=0x100, continuity=None):
    """The mux on the device over ANY device bytes (jsmpeg_hip_ts_mux_device): dev_es / dev_ts device addresses, ranges =
    [(offset, bytes)] -- one PES per range -- pts = seconds per range, streams = a stream number per range (ascending; None: all
    0), continuity = a counter per stream number (None: 0).  Synchronous.  Returns (total bytes, {stream: (begin, end)} of the
    streams that have units, [the counters to hand to the next call])."""
    L = lib()
    n = len(ranges)
    if len(pts) != n:
        raise ValueError("ts_mux_device: one pts per range")
    st = np.zeros(n, np.uint32) if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
    if st.shape != (n,):
        raise ValueError("ts_mux_device: one stream number per range")
    ns = int(n_streams) if n_streams is not None else (int(st.max()) + 1 if n else 1)
    off = np.ascontiguousarray([r[0] for r in ranges], dtype=np.uint64)
    ln = np.ascontiguousarray([r[1] for r in ranges], dtype=np.uint32)
    p90 = pts_90k(pts)
    cc = np.zeros(ns, np.uint8)
    if continuity is not None:
        cc[:] = np.asarray(continuity, dtype=np.int64) & 15
    sb, se = np.zeros(ns, np.uint64), np.zeros(ns, np.uint64)
    total = L.jsmpeg_hip_ts_mux_device(dev_es, off.ctypes.data, ln.ctypes.data, st.ctypes.data, p90.ctypes.data, n, stream_id, pid,
                                       cc.ctypes.data, ns, dev_ts, int(ts_cap), sb.ctypes.data, se.ctypes.data)
    if total < 0:
        raise RuntimeError(_batch.last_error())
    return int(total), {int(s): (int(sb[s]), int(se[s])) for s in sorted(set(int(v) for v in st))}, [int(c) for c in cc]


def ts_mux(es, ranges, pts, stream_id=0xE0, pid=0x100, continuity=0):
    """Host-side TS mux (no device): `es` bytes, ranges = [(offset, bytes)] -- one PES per range -- and pts = seconds per
    range -> (MPEG-TS bytes as a uint8 array, the continuity counter to hand to the next call)."""
    L = lib()
    es = np.ascontiguousarray(np.frombuffer(es, dtype=np.uint8) if isinstance(es, (bytes, bytearray)) else es, dtype=np.uint8)
    n = len(ranges)
    if len(pts) != n:
        raise ValueError("ts_mux: one pts per range")
    off = np.ascontiguousarray([r[0] for r in ranges], dtype=np.uint64)
    ln = np.ascontiguousarray([r[1] for r in ranges], dtype=np.uint32)
    if n and int((off + ln).max()) > es.size:
        raise ValueError("ts_mux: a range ends behind the bytes")
    p90 = pts_90k(pts)
    cc = ctypes.c_uint8(continuity & 15)
    need = L.jsmpeg_hip_ts_mux_host(es.ctypes.data, off.ctypes.data, ln.ctypes.data, p90.ctypes.data, n, stream_id, pid, ctypes.byref(cc), None, 0)
    if need < 0:
        raise RuntimeError(_batch.last_error())
    out = np.empty(max(1, need), dtype=np.uint8)
    got = L.jsmpeg_hip_ts_mux_host(es.ctypes.data, off.ctypes.data, ln.ctypes.data, p90.ctypes.data, n, stream_id, pid, ctypes.byref(cc), out.ctypes.data, need)
    if got != need:
        raise RuntimeError(_batch.last_error() or "jsmpeg_hip_ts_mux_host: %d bytes, %d expected" % (got, need))
    return out[:need], int(cc.value)


class Encoder:
    """Pictures on the device -> MPEG-1 elementary streams on the device: all I pictures, or I + P after set_gop.  A call is a
    pure enqueue; sync() or any reader settles it.  chain=True on a call continues its streams -- the stream NUMBER is a
    stream's identity from call to call -- where their last chained call left them: ordinals, P chain and GOP budget go on,
    and the pieces concatenated are the stream one call over all the pictures writes.  A piece that begins with a P picture
    begins at its picture start code: for concatenation or a Live that holds the sequence header already."""

    def __init__(self, width, height, max_pictures, max_streams, max_es_bytes, frame_rate_code=0, device=-1):
        self.L = lib()
        cfg = EncoderConfig(width, height, max_pictures, max_streams, max_es_bytes, frame_rate_code, device)
        self.width, self.height = width, height
        self.coded_width, self.coded_height = (width + 15) & ~15, (height + 15) & ~15
        self.frame_bytes = self.coded_width * self.coded_height * 3 // 2
        self.max_pictures, self.max_streams = max_pictures, max_streams
        self.frame_rate_code = frame_rate_code or 5
        self.h = self.L.jsmpeg_hip_encoder_create(ctypes.byref(cfg))
        if not self.h:
            raise RuntimeError("jsmpeg_hip_encoder_create: " + _batch.last_error())
        self.device = device
        self.count = 0
        self._continuity = 0
        self.cells = []             # the mosaic layout (set_mosaic)

    def _ok(self, rc):
        if rc < 0:
            raise RuntimeError(_batch.last_error())
        return rc

    def close(self):
        if self.h:
            self.L.jsmpeg_hip_encoder_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def _lists(self, count, streams, qscale):
        s = None if streams is None else np.ascontiguousarray(streams, dtype=np.uint32)
        if s is not None and s.shape != (count,):
            raise ValueError("streams: one stream number per picture")
        if isinstance(qscale, (int, np.integer)):
            return s, None, int(qscale)
        q = np.asarray(qscale)
        if q.shape != (count,) or (count and (q.min() < 0 or q.max() > 255)):
            raise ValueError("qscale: an integer or one per picture")
        return s, np.ascontiguousarray(q, dtype=np.uint8), 0

    @staticmethod
    def _flags(end, chain):
        return (END if end else 0) | (CHAIN if chain else 0)

    def _pts(self, pts):
        """pts: seconds per picture of the next call, rounded as ts_mux() rounds (None: the default rule of the frame rate)"""
        if pts is not None:
            p = pts_90k(pts)
            self._ok(self.L.jsmpeg_hip_encoder_ts_pts(self.h, p.ctypes.data, len(p)))

    def encode(self, frame_ptrs, streams=None, qscale=8, end=True, stream=None, chain=False, pts=None):
        """frame_ptrs: device addresses of Y | Cr | Cb planes of the coded size, one per picture; streams: ascending stream
        numbers (None: all stream 0); qscale: 1 .. 31, or one per picture; end: close every stream with a sequence end
        code; stream: the HIP stream to enqueue on -- the one the frames were produced on (ordering is the caller's); chain:
        continue the streams (end=True then closes them AND ends their chains); pts: with set_ts, seconds per picture for the
        PES headers (None: ordinal / frame rate)."""
        ptrs = [int(p) if p else 0 for p in frame_ptrs]
        n = len(ptrs)
        arr = (ctypes.c_void_p * max(1, n))(*ptrs)
        s, q, qs = self._lists(n, streams, qscale)
        self._pts(pts)
        self._ok(self.L.jsmpeg_hip_encoder_encode(self.h, arr, None if s is None else s.ctypes.data, None if q is None else q.ctypes.data,
                                                  n, qs, self._flags(end, chain), stream))
        self.count = n

    def encode_scaled(self, frame_ptrs, source_size, crop=None, antialias=True, streams=None, qscale=8, end=True, stream=None, chain=False, pts=None):
        """encode() from frames of ANOTHER size: frame_ptrs are Y | Cr | Cb planes of the coded size of source_size = (width,
        height), e.g. pool slots of a Batch or Live of that size; crop = (x, y, width, height) in display pixels, x / y even
        (None: the whole picture).  The planes are cropped and scaled on the device into the encoder's own frame store --
        torch's bilinear / antialiased filter in integers, bit for bit jsmpeg_amd/csrc/enc_scale.h -- and coded from there:
        GOP, rate control and chain behave as in encode().  source(k) returns what was coded."""
        ptrs = [int(p) if p else 0 for p in frame_ptrs]
        n = len(ptrs)
        arr = (ctypes.c_void_p * max(1, n))(*ptrs)
        s, q, qs = self._lists(n, streams, qscale)
        src = EncSource(int(source_size[0]), int(source_size[1]), *([int(v) for v in crop] if crop is not None else [0, 0, 0, 0]), 1 if antialias else 0)
        self._pts(pts)
        self._ok(self.L.jsmpeg_hip_encoder_encode_scaled(self.h, arr, ctypes.byref(src), None if s is None else s.ctypes.data,
                                                         None if q is None else q.ctypes.data, n, qs, self._flags(end, chain), stream))
        self.count = n

    def set_mosaic(self, cells, fill=(16, 128, 128)):
        """The layout of encode_mosaic: a list of EncCell (cell(), grid()), at most 64, and the fill colour (Y, Cr, Cb) of what
        no cell covers.  Every plane is filled, then the cells are pasted in list order -- a later cell wins where they overlap
        (picture in picture); bit for bit jsmpeg_amd/csrc/enc_mosaic.h.  State of the handle, like set_gop; an empty list
        removes the layout.  Refused while a pass is in flight, and for a layout the rule does not cover: the layout before
        stays then."""
        cells = list(cells)
        arr = (EncCell * max(1, len(cells)))(*cells)
        y, cr, cb = (int(v) for v in fill)
        if min(y, cr, cb) < 0 or max(y, cr, cb) > 255:
            raise ValueError("fill: three bytes (Y, Cr, Cb)")
        self._ok(self.L.jsmpeg_hip_encoder_set_mosaic(self.h, arr if cells else None, len(cells), y | cr << 8 | cb << 16))
        self.cells = [EncCell.from_buffer_copy(c) for c in cells]

    def encode_mosaic(self, frame_ptrs, streams=None, qscale=8, end=True, stream=None, chain=False, pts=None):
        """encode() of pictures COMPOSED on the device from the layout's cells: frame_ptrs is a list of pictures, each a list
        of one device address per cell -- Y | Cr | Cb planes of that cell's source's coded size, e.g. Live.latest_frames --
        or None / 0 for a cell that is absent from that picture (what lies under it shows).  Everything else is
        encode_scaled's; source(k) returns the composed planes."""
        n, nc = len(frame_ptrs), len(self.cells)
        flat = []
        for k, pic in enumerate(frame_ptrs):
            pic = list(pic)
            if len(pic) != nc:
                raise ValueError("encode_mosaic: picture %d has %d frame pointers, the layout has %d cells" % (k, len(pic), nc))
            flat += [int(p) if p else 0 for p in pic]
        arr = (ctypes.c_void_p * max(1, len(flat)))(*flat)
        s, q, qs = self._lists(n, streams, qscale)
        self._pts(pts)
        self._ok(self.L.jsmpeg_hip_encoder_encode_mosaic(self.h, arr, None if s is None else s.ctypes.data, None if q is None else q.ctypes.data,
                                                         n, qs, self._flags(end, chain), stream))
        self.count = n

    def encode_mosaic_latest(self, sources, streams=None, qscale=8, end=True, stream=None, chain=False, pts=None):
        """ONE picture from the newest decoded picture of a live stream per cell: sources[c] = (live, stream id) -- the Lives
        may differ, e.g. a router's Lives of several sizes; each must have the size of its cell's source.  A stream that has
        decoded nothing yet leaves its cell absent.  Returns [present] per cell.  The frames hold their pictures through the
        next tick of their Live (Live.latest_frames)."""
        if len(sources) != len(self.cells):
            raise ValueError("encode_mosaic_latest: %d sources, the layout has %d cells" % (len(sources), len(self.cells)))
        by_live = {}
        for c, (lv, sid) in enumerate(sources):
            src = self.cells[c].source
            if (lv.width, lv.height) != (src.width, src.height):
                raise ValueError("encode_mosaic_latest: cell %d reads %d x %d frames, its live is %d x %d" % (c, src.width, src.height, lv.width, lv.height))
            by_live.setdefault(id(lv), (lv, []))[1].append((c, int(sid)))
        ptrs = [0] * len(sources)
        for lv, want in by_live.values():
            for (c, _), p in zip(want, lv.latest_frames([sid for _, sid in want])):
                ptrs[c] = p or 0
        self.encode_mosaic([ptrs], streams, qscale, end, stream, chain, pts)
        return [bool(p) for p in ptrs]

    def _encode_from(self, ptrs, size, crop, antialias, streams, qscale, end, stream, chain, pts=None):
        """planes of `size`: straight in when that is the encoder's size and nothing is cropped, scaled otherwise"""
        if crop is None and tuple(size) == (self.width, self.height):
            self.encode(ptrs, streams, qscale, end, stream, chain, pts)
        else:
            self.encode_scaled(ptrs, size, crop, antialias, streams, qscale, end, stream, chain, pts)

    def encode_batch(self, batch, pictures, streams=None, qscale=8, end=True, stream=None, chain=False, crop=None, antialias=True, pts=None):
        """pictures of a Batch's last decode, straight from its frame pool (the batch is synchronised first; a picture that was
        not decoded is refused).  streams None: each picture's own stream number, which must then ascend.  A batch of another
        size than the encoder's, or a crop, goes through encode_scaled."""
        batch.sync()
        infos = [batch.picture_info(int(p)) for p in pictures]
        for p, info in zip(pictures, infos):
            if not info.decoded:
                raise ValueError("encode_batch: picture %d was not decoded" % int(p))
        if streams is None:
            streams = [info.stream for info in infos]
        base = batch.frame_pool_ptr
        self._encode_from([base + int(p) * batch.frame_stride for p in pictures], (batch.width, batch.height), crop, antialias,
                          streams, qscale, end, stream, chain, pts)

    def encode_live(self, live, pictures=None, streams=None, qscale=8, end=True, stream=None, chain=False, crop=None, antialias=True, pts=None):
        """pictures of a Live's last tick (None: all of them, in tick order), from their device_frame pointers.  streams
        None: the pictures are sorted by their live stream id (stable) and numbered 0, 1, .. in that order -- or, with
        chain=True, each picture's live stream id IS its stream number (an id at or above max_streams is refused), so that a
        stream keeps its identity when others join or leave.  A live of another size than the encoder's, or a crop, goes
        through encode_scaled: a rendition.  pts: per picture IN THE ORDER ENCODED (the sorted one).  Returns the pictures in
        the order they were encoded in."""
        pics = live.pictures()
        if pictures is not None:
            pics = [pics[int(i)] for i in pictures]
        if streams is None:
            order = sorted(range(len(pics)), key=lambda i: pics[i].stream)
            pics = [pics[i] for i in order]
            if chain:
                for p in pics:
                    if p.stream >= self.max_streams:
                        raise ValueError("encode_live: live stream id %d >= max_streams %d" % (p.stream, self.max_streams))
                streams = [p.stream for p in pics]
            else:
                ids = sorted({p.stream for p in pics})
                streams = [ids.index(p.stream) for p in pics]
        self._encode_from([p.device_frame for p in pics], (live.width, live.height), crop, antialias, streams, qscale, end, stream, chain, pts)
        return pics

    def encode_tensor(self, x, streams=None, qscale=8, end=True, order="rgb", chain=False, pts=None):
        """x: a contiguous torch uint8 CUDA tensor [N, 3, H, W] or [N, H, W, 3] of the display size; runs on torch's current
        stream of the tensor's device"""
        import torch
        if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8 or not x.is_cuda or x.dim() != 4 or not x.is_contiguous():
            raise ValueError("encode_tensor: a contiguous uint8 CUDA tensor [N, 3, H, W] or [N, H, W, 3] is needed")
        if tuple(x.shape[1:]) == (3, self.height, self.width):
            layout = 0
        elif tuple(x.shape[1:]) == (self.height, self.width, 3):
            layout = 1
        else:
            raise ValueError("encode_tensor: shape %r is neither [N, 3, %d, %d] nor [N, %d, %d, 3]" % (tuple(x.shape), self.height, self.width, self.height, self.width))
        if str(order).lower() not in ("rgb", "bgr"):
            raise ValueError("order %r: one of rgb, bgr" % (order,))
        n = int(x.shape[0])
        s, q, qs = self._lists(n, streams, qscale)
        st = torch.cuda.current_stream(x.device).cuda_stream
        self._pts(pts)
        self._ok(self.L.jsmpeg_hip_encoder_encode_rgb(self.h, x.data_ptr() if n else None, layout, 1 if str(order).lower() == "bgr" else 0,
                                                      None if s is None else s.ctypes.data, None if q is None else q.ctypes.data,
                                                      n, qs, self._flags(end, chain), st))
        self.count = n
        self._keep = x          # the tensor stays alive until the next call

    def set_gop(self, gop, search=7):
        """gop 1: I pictures only (the default).  gop N > 1: every N-th picture of a stream is an I picture, the others are P
        pictures predicted from the encoder's own reconstruction; search: full-pel radius 0 .. 15 of the motion search (0:
        zero vectors only).  State of the handle: every later encode* call uses it.  Every stream of a call begins with an
        I picture unless the call is chained (chain=True).  Ends every stream's chain."""
        self._ok(self.L.jsmpeg_hip_encoder_set_gop(self.h, gop, search))

    def chain_reset(self, stream=None):
        """ends the chain of `stream` (None: of every stream): its next chained picture is an I picture with its sequence header
        -- for a viewer that joins, or a stream number that is handed to another source.  Refused while a pass is in flight."""
        self._ok(self.L.jsmpeg_hip_encoder_chain_reset(self.h, 0xffffffff if stream is None else stream))

    def chain_info(self, stream):
        """(whether `stream` has chain state, the pictures it has coded = the ordinal of its next chained picture)"""
        out = (ctypes.c_uint32 * 2)()
        self._ok(self.L.jsmpeg_hip_encoder_chain_info(self.h, stream, out))
        return bool(out[0]), int(out[1])

    def recon_ptr(self, k):
        """device address of picture k's reconstruction (Y | Cr | Cb of the coded size) in the last call; gop > 1 only"""
        p = self.L.jsmpeg_hip_encoder_recon(self.h, k)
        if not p:
            raise RuntimeError(_batch.last_error())
        return p

    def source_ptr(self, k):
        """device address of the planes picture k of the last call was coded from (Y | Cr | Cb of the coded size): the caller's
        frame after encode, the encoder's store after encode_tensor (converted) and encode_scaled (scaled)"""
        p = self.L.jsmpeg_hip_encoder_source(self.h, k)
        if not p:
            raise RuntimeError(_batch.last_error())
        return p

    def source(self, k):
        """those planes on the host: (Y, Cr, Cb) uint8 of the coded size"""
        return self._read_planes(self.source_ptr(k))

    def recon(self, k):
        """picture k's reconstruction on the host: (Y, Cr, Cb) uint8 planes of the coded size -- what a decoder shows"""
        return self._read_planes(self.recon_ptr(k))

    def _read_planes(self, p):
        out = np.empty(self.frame_bytes, dtype=np.uint8)
        L = _batch.lib()
        L.jsmpeg_hip_device_read.restype = ctypes.c_int
        L.jsmpeg_hip_device_read.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64]
        self._ok(L.jsmpeg_hip_device_read(out.ctypes.data, p, self.frame_bytes))
        n, cw, ch = self.coded_width * self.coded_height, self.coded_width, self.coded_height
        return out[:n].reshape(ch, cw), out[n:n + n // 4].reshape(ch // 2, cw // 2), out[n + n // 4:].reshape(ch // 2, cw // 2)

    def picture_stats(self, k):
        """macroblocks of picture k of the last call by kind"""
        out = (ctypes.c_uint32 * 4)()
        self._ok(self.L.jsmpeg_hip_encoder_picture_stats(self.h, k, out))
        return dict(intra=int(out[0]), coded=int(out[1]), not_coded=int(out[2]), skipped=int(out[3]))

    def set_rate(self, bytes_per_picture, q_min=1, q_max=31, i_weight=4):
        """Rate control: 0 switches it off (the default; the qscale arguments hold).  Otherwise every GOP of a call has
        bytes_per_picture bytes per picture, its I picture i_weight shares of them against one per P picture, and each
        picture is coded at the smallest scale of q_min .. q_max at which it fits its budget, measured exactly on the device
        (q_max if it fits at none).  State of the handle, like set_gop; bytes_per_picture(bits_per_second,
        self.frame_rate_code) turns a bit rate into the target."""
        self._ok(self.L.jsmpeg_hip_encoder_set_rate(self.h, bytes_per_picture, q_min, q_max, i_weight))

    def picture_rate(self, k):
        """what rate control chose for picture k of the last call: the scale, the budget in bytes (saturated to 32 bits) and
        the picture's bytes"""
        out = (ctypes.c_uint32 * 3)()
        self._ok(self.L.jsmpeg_hip_encoder_picture_rate(self.h, k, out))
        return dict(q=int(out[0]), budget=int(out[1]), bytes=int(out[2]))

    def sync(self):
        self._ok(self.L.jsmpeg_hip_encoder_sync(self.h))

    def query(self):
        """True once the pass in flight has finished on the device; never waits"""
        return bool(self._ok(self.L.jsmpeg_hip_encoder_query(self.h)))

    def device_es(self):
        """(device address, total bytes) of the last call's buffer: 16-byte aligned stream begins, 0xff around them"""
        total = ctypes.c_uint64()
        p = self.L.jsmpeg_hip_encoder_es(self.h, ctypes.byref(total))
        if not p:
            raise RuntimeError(_batch.last_error())
        return p, int(total.value)

    def stream_range(self, stream):
        b, e = ctypes.c_uint64(), ctypes.c_uint64()
        self._ok(self.L.jsmpeg_hip_encoder_stream_range(self.h, stream, ctypes.byref(b), ctypes.byref(e)))
        return int(b.value), int(e.value)

    def es(self, stream=0):
        """the stream's bytes, copied to the host"""
        n = self._ok(self.L.jsmpeg_hip_encoder_read_es(self.h, stream, None, 0))
        out = np.empty(max(1, n), dtype=np.uint8)
        self._ok(self.L.jsmpeg_hip_encoder_read_es(self.h, stream, out.ctypes.data, n))
        return out[:n].tobytes()

    def picture_ranges(self):
        """[(offset in the device buffer, bytes)] per picture of the last call, from its sequence header on"""
        out = []
        for k in range(self.count):
            o, b = ctypes.c_uint64(), ctypes.c_uint32()
            self._ok(self.L.jsmpeg_hip_encoder_picture_range(self.h, k, ctypes.byref(o), ctypes.byref(b)))
            out.append((int(o.value), int(b.value)))
        return out

    def timings(self):
        ms = (ctypes.c_float * 4)()
        self._ok(self.L.jsmpeg_hip_encoder_timings(self.h, ms))
        return dict(convert_ms=ms[0], measure_ms=ms[1], write_ms=ms[2], total_ms=ms[3])

    def set_ts(self, max_ts_bytes, stream_id=0xE0, pid=0x100):
        """MPEG-TS on the device: 0 switches it off (the default).  Otherwise every later encode* call also leaves each stream
        as ready-to-send TS packets, one PES per picture, in a device buffer of max_ts_bytes (ts_bound gives a safe size) --
        the bytes ts_mux() writes over the call's picture ranges, muxed in the same enqueue.  A continuity counter per stream
        number lives on the device and goes on from call to call; chain_reset and set_gop leave it alone, set_ts zeroes all."""
        self._ok(self.L.jsmpeg_hip_encoder_set_ts(self.h, stream_id, pid, int(max_ts_bytes)))

    def device_ts(self):
        """(device address, total bytes) of the last call's TS buffer: 16-byte aligned stream begins"""
        total = ctypes.c_uint64()
        p = self.L.jsmpeg_hip_encoder_ts(self.h, ctypes.byref(total))
        if not p:
            raise RuntimeError(_batch.last_error())
        return p, int(total.value)

    def ts_range(self, stream):
        """(begin, end) of the stream in the TS buffer and the continuity counter its next packet will carry"""
        b, e, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint32()
        self._ok(self.L.jsmpeg_hip_encoder_ts_range(self.h, stream, ctypes.byref(b), ctypes.byref(e), ctypes.byref(c)))
        return int(b.value), int(e.value), int(c.value)

    def ts_picture_ranges(self):
        """[(offset in the TS buffer, bytes)] of each picture's packets; a viewer that joins starts at an I picture's"""
        out = []
        for k in range(self.count):
            o, b = ctypes.c_uint64(), ctypes.c_uint32()
            self._ok(self.L.jsmpeg_hip_encoder_ts_picture_range(self.h, k, ctypes.byref(o), ctypes.byref(b)))
            out.append((int(o.value), int(b.value)))
        return out

    def ts(self, stream=0):
        """the stream's TS packets of the last call, copied to the host"""
        n = self._ok(self.L.jsmpeg_hip_encoder_read_ts(self.h, stream, None, 0))
        out = np.empty(max(1, n), dtype=np.uint8)
        self._ok(self.L.jsmpeg_hip_encoder_read_ts(self.h, stream, out.ctypes.data, n))
        return out[:n].tobytes()

    def ts_all(self, streams=None):
        """every stream's TS in ONE copy: (the whole buffer as a uint8 array, {stream: (begin, end)}) -- of `streams`, or of
        every stream number that has packets"""
        n = self._ok(self.L.jsmpeg_hip_encoder_read_ts(self.h, 0xffffffff, None, 0))
        out = np.empty(max(1, n), dtype=np.uint8)
        self._ok(self.L.jsmpeg_hip_encoder_read_ts(self.h, 0xffffffff, out.ctypes.data, n))
        ranges = {}
        for s in (range(self.max_streams) if streams is None else streams):
            b, e, _ = self.ts_range(s)
            if e > b or streams is not None:
                ranges[int(s)] = (b, e)
        return out[:n], ranges

    def ts_mux(self, es, ranges, pts, stream_id=0xE0, pid=0x100):
        """ts_mux() with the continuity counter carried from call to call on this object"""
        out, self._continuity = ts_mux(es, ranges, pts, stream_id, pid, self._continuity)
        return out
