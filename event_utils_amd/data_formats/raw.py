"""Prophesee / Metavision `.raw` recordings: EVT3 (16-bit words) and EVT2 (32-bit words).  (No reference module: the reference's
lib/data_formats reads HDF5 and rosbags.)  The words are uploaded as they are -- 2 to 4 bytes per event, less for vectorised
streams, against 13 for decoded columns -- and decoded on the device (evk_rawdecode.hip: three launches, include/evk.h states the
decoding rules).  The rules are this library's definition of the formats, written from the public format descriptions; no
vendor-written file has been decoded with it.

    read_raw(path)                      -> RawFile(format, sensor_size, header, words, trailing_bytes)
    decode_evt3 / decode_evt2(words)    -> RawEvents(xs, ys, ts, ps, stats) on the device (+ RawState with return_state)
    decode_raw / iter_decode_raw(path)  -> the same for a file, piece by piece with the state carried
    encode_evt3 / encode_evt2, write_raw   host numpy: a file form for the simulator's output (and the tests' streams)
"""
import collections
import os
import warnings

import numpy as np
import torch

from .. import _device as D
from .. import _lib
from ..events import DeviceEvents

RawFile = collections.namedtuple("RawFile", ["format", "sensor_size", "header", "words", "trailing_bytes"])
RawStats = collections.namedtuple("RawStats", ["events", "triggers", "other", "before_time", "time_went_back", "out_of_range",
                                               "loops"])
RawState = collections.namedtuple("RawState", ["y", "base_x", "vect_pol", "t_low", "t_high", "loops", "have_time"])
RawState.__new__.__defaults__ = (0, 0, 0, 0, 0, 0, False)

_FORMATS = {"evt3": _lib.EVK_RAW_EVT3, "evt2": _lib.EVK_RAW_EVT2, 3: _lib.EVK_RAW_EVT3, 2: _lib.EVK_RAW_EVT2}
_WORD = {_lib.EVK_RAW_EVT3: np.dtype("<u2"), _lib.EVK_RAW_EVT2: np.dtype("<u4")}
_NAME = {_lib.EVK_RAW_EVT3: "evt3", _lib.EVK_RAW_EVT2: "evt2"}
_T_WORD = {_lib.EVK_RAW_EVT3: (torch.int16, getattr(torch, "uint16", torch.int16)),
           _lib.EVK_RAW_EVT2: (torch.int32, getattr(torch, "uint32", torch.int32))}


class RawEvents(collections.namedtuple("RawEvents", ["xs", "ys", "ts", "ps", "stats"])):
    """Decoded events on the device: xs, ys int16; ts int64 microseconds (or float64 seconds); ps uint8 {0, 1}; stats: RawStats."""
    __slots__ = ()

    def to_device_events(self, t_offset=None):
        """A DeviceEvents on the native columns (DeviceEvents.from_native, polarity {0, 1} -> -1 / +1, time in seconds)."""
        ts = self.ts if self.ts.dtype == torch.float64 else self.ts.to(torch.float64) / 1e6
        return DeviceEvents.from_native(self.xs, self.ys, ts, self.ps, polarity="pm1", t_offset=t_offset, device=self.xs.device)


def _format(fmt):
    key = fmt.lower() if isinstance(fmt, str) else fmt
    if key not in _FORMATS:
        raise ValueError("format must be 'evt3' or 'evt2' (got %r)" % (fmt,))
    return _FORMATS[key]


# ---- files ------------------------------------------------------------------------------------------------------------------

def parse_raw_header(data):
    """(format or None, sensor_size (H, W) or None, header dict, header length in bytes) of the bytes a .raw file starts with:
    the lines that start with '%', up to and including '% end'; without one (older files), up to the first line that does not
    start with '%'."""
    pos, header, fmt, size = 0, collections.OrderedDict(), None, None
    while pos < len(data) and data[pos:pos + 1] == b"%":
        nl = data.find(b"\n", pos)
        end = len(data) if nl < 0 else nl
        line = data[pos + 1:end].decode("latin-1").strip()
        pos = len(data) if nl < 0 else nl + 1
        key, _, value = line.partition(" ")
        key, value = key.strip().lower(), value.strip()
        if key == "end":
            break
        if not key:
            continue
        header[key] = value
        if key == "evt":
            fmt = {"3.0": "evt3", "2.0": "evt2"}.get(value, fmt)
        elif key == "format":
            parts = value.split(";")
            fmt = {"evt3": "evt3", "evt2": "evt2"}.get(parts[0].strip().lower(), fmt)
            kv = dict(p.split("=", 1) for p in parts[1:] if "=" in p)
            if "height" in kv and "width" in kv:
                size = (int(kv["height"]), int(kv["width"]))
        elif key == "geometry":
            w, _, h = value.lower().partition("x")
            size = (int(h), int(w))
    return fmt, size, header, pos


def read_raw(path):
    """RawFile(format 'evt3' | 'evt2', sensor_size (H, W) or None, header dict, words, trailing_bytes): the payload as a
    read-only np.memmap of uint16 / uint32 words.  Bytes at the end that do not fill a word are left out and counted in
    trailing_bytes (with a warning)."""
    size = os.path.getsize(path)
    take = 1 << 16
    while True:
        with open(path, "rb") as f:
            head = f.read(take)
        fmt, sensor, header, start = parse_raw_header(head)
        if start < len(head) or len(head) >= size:
            break
        take *= 4
    if fmt is None:
        raise ValueError("%s: the header names no event format this reader knows ('%% evt 3.0', '%% evt 2.0' or '%% format EVT3;...')"
                         % path)
    dt = _WORD[_format(fmt)]
    n, trailing = divmod(size - start, dt.itemsize)
    if trailing:
        warnings.warn("%s: %d trailing byte(s) do not fill a %d-byte word and are left out" % (path, trailing, dt.itemsize))
    words = np.memmap(path, dtype=dt, mode="r", offset=start, shape=(n,)) if n else np.empty(0, dtype=dt)
    return RawFile(fmt, sensor, header, words, trailing)


def write_raw(path, words, format, sensor_size):
    """A .raw file: the ASCII header ('% evt', '% format', '% geometry', '% end') and the little-endian words."""
    fmt = _format(format)
    h, w = (int(v) for v in sensor_size)
    words = np.ascontiguousarray(np.asarray(words).reshape(-1), dtype=_WORD[fmt])
    head = "%% evt %d.0\n%% format EVT%d;height=%d;width=%d\n%% geometry %dx%d\n%% end\n" % (fmt, fmt, h, w, w, h)
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(words.tobytes())


# ---- decoding ---------------------------------------------------------------------------------------------------------------

def _device_words(words, fmt, dev):
    """1-D device tensor that holds the words (a resident tensor or a slice of one is used in place), and their number."""
    item = _WORD[fmt].itemsize
    if isinstance(words, torch.Tensor):
        t = words.reshape(-1)
        if t.dtype == torch.uint8:
            if t.shape[0] % item:
                raise ValueError("%d bytes are no whole number of %d-byte words" % (t.shape[0], item))
        elif t.dtype not in _T_WORD[fmt]:
            raise TypeError("%s words are %d-byte integers or bytes (got %s)" % (_NAME[fmt], item, t.dtype))
        t = t.to(dev).contiguous()
        if t.data_ptr() % item:                       # bytes that start inside a word
            t = t.clone()
        return t, t.shape[0] * t.element_size() // item
    if isinstance(words, (bytes, bytearray, memoryview)):
        if len(words) % item:
            raise ValueError("%d bytes are no whole number of %d-byte words" % (len(words), item))
        a = np.frombuffer(words, dtype=_WORD[fmt])
    else:
        a = np.asarray(words).reshape(-1)
        if a.dtype.kind not in "iu" or a.dtype.itemsize != item:
            raise TypeError("%s words are %d-byte integers (got %s)" % (_NAME[fmt], item, a.dtype))
        if not a.dtype.isnative:
            a = a.astype(a.dtype.newbyteorder("="))
    a = np.ascontiguousarray(a).view(np.int16 if item == 2 else np.int32)
    if not a.flags.writeable:                         # (a read-only map or buffer: the copy is the read of the file)
        a = np.array(a)
    return torch.from_numpy(a).to(dev), a.shape[0]


def _drop_out_of_range(xs, ys, tcol, ps, h, w):
    """The events inside the sensor, in stream order, by the rule that counted the others (evk.h: unsigned 16-bit compares).  Up to
    32768 rows and columns that is clip_events_to_bounds on the int16 columns.  On a wider sensor a negative int16 is a coordinate
    from 32768 up, which may lie inside: the same compaction then evaluates the box on the coordinates' unsigned values."""
    from ..util import event_util as U
    if max(h, w) <= 32768:
        return U.clip_events_to_bounds(xs, ys, tcol, ps, [h, w])
    px, py = (c.to(torch.int32) & 0xFFFF for c in (xs, ys))
    kept, _, _ = U._compact(_lib.EVK_SELECT_BOX, px, py, _lib.EVK_SELECT_I32, [xs, ys, tcol, ps], params=[0.0, float(w), 0.0, float(h)],
                            t_col=2)
    return tuple(kept)


def _decode(words, fmt, sensor_size, ts, state, return_state, on_out_of_range, device, flags=0):
    if ts not in ("us", "seconds"):
        raise ValueError("ts must be 'us' or 'seconds' (got %r)" % (ts,))
    if on_out_of_range not in ("raise", "keep", "drop"):
        raise ValueError("on_out_of_range must be 'raise', 'keep' or 'drop' (got %r)" % (on_out_of_range,))
    h = w = 0
    if sensor_size is not None:
        h, w = (int(v) for v in sensor_size)
        if not (0 < h <= 65535 and 0 < w <= 65535):
            raise ValueError("sensor_size must be (H, W) with 0 < H, W <= 65535 (got %r)" % (sensor_size,))
    dev = torch.device(device) if device is not None else D.device_of(words)
    if dev.type != "cuda":
        raise _lib.EvkError("raw streams are decoded on the GPU (got device %s); there is no CPU fallback" % dev)
    D.require_gpu()
    with torch.cuda.device(dev):
        wt, n = _device_words(words, fmt, dev)
        L = _lib.lib()
        nbytes = int(L.evk_raw_decode_scratch_bytes(n))
        if nbytes < 0:
            raise _lib.EvkError("evk_raw_decode_scratch_bytes refused %d words" % n)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        report = torch.empty(16, dtype=torch.int64, device=dev)           # result | state_out
        st_in = None
        if state is not None:
            st_in = torch.tensor([int(v) for v in RawState(*state)] + [0], dtype=torch.int64).to(dev)
        stream = D.stream()
        _lib.call("evk_raw_decode_plan", D.ptr(wt), n, fmt, D.ptr(st_in), D.ptr(scratch), nbytes, D.ptr(report), D.ptr(report[8:]),
                  stream)
        host = [int(v) for v in report.tolist()]                          # the call's one read-back before the columns exist
        count = host[0]
        xs, ys = (torch.empty(count, dtype=torch.int16, device=dev) for _ in range(2))
        tcol = torch.empty(count, dtype=torch.float64 if ts == "seconds" else torch.int64, device=dev)
        ps = torch.empty(count, dtype=torch.uint8, device=dev)
        _lib.call("evk_raw_decode_write", D.ptr(wt), n, fmt, D.ptr(scratch), nbytes, D.ptr(report), D.ptr(xs), D.ptr(ys), D.ptr(tcol),
                  D.ptr(ps), _lib.EVK_RAW_TS_SECONDS if ts == "seconds" else _lib.EVK_RAW_TS_US, h, w, int(flags), stream)
        bad = int(report[5].item()) if (h and count) else 0
        if bad and on_out_of_range == "raise":
            raise ValueError("%d of %d decoded events lie outside the %d x %d sensor (on_out_of_range='keep' returns them, 'drop' "
                             "removes them)" % (bad, count, w, h))
        if bad and on_out_of_range == "drop":
            xs, ys, tcol, ps = _drop_out_of_range(xs, ys, tcol, ps, h, w)
            count = int(xs.shape[0])
    stats = RawStats(count, host[1], host[2], host[3], host[4], bad, host[6])
    out = RawEvents(xs, ys, tcol, ps, stats)
    if return_state:
        return out, RawState(*host[8:14], bool(host[14]))
    return out


def decode_evt3(words, sensor_size=None, ts="us", state=None, return_state=False, on_out_of_range="raise", device=None):
    """EVT3 words (numpy, host or device tensor of 16-bit integers or bytes, bytes) -> RawEvents on the device, in word and bit order.
    ts: 'us' int64 microseconds, 'seconds' float64 us / 1e6.  state / return_state: the decoder's RawState before the first and
    after the last word -- decode(a + b) is decode(a) followed by decode(b, state=the state a left).  With sensor_size = (H, W)
    events off the sensor are counted (stats.out_of_range) and on_out_of_range decides: 'raise' ValueError, 'keep' them,
    'drop' them (clip_events_to_bounds).  stats: events returned, triggers, words of other types, events before the first
    TIME_HIGH (not returned), small backward TIME_HIGH steps, out_of_range, time loops counted -- all of this call."""
    return _decode(words, _lib.EVK_RAW_EVT3, sensor_size, ts, state, return_state, on_out_of_range, device)


def decode_evt2(words, sensor_size=None, ts="us", state=None, return_state=False, on_out_of_range="raise", device=None):
    """EVT2 words (32-bit) -> RawEvents; arguments as decode_evt3.  The state uses t_high and have_time only."""
    return _decode(words, _lib.EVK_RAW_EVT2, sensor_size, ts, state, return_state, on_out_of_range, device)


def iter_decode_raw(path_or_rawfile, chunk_words=1 << 26, sensor_size=None, ts="us", on_out_of_range="raise", device=None):
    """The RawEvents of consecutive pieces of chunk_words words of a file (a path or a RawFile), each uploaded and decoded with the
    state the piece before it left.  sensor_size defaults to the header's."""
    rf = path_or_rawfile if isinstance(path_or_rawfile, RawFile) else read_raw(path_or_rawfile)
    fmt = _format(rf.format)
    chunk_words = int(chunk_words)
    if chunk_words < 1:
        raise ValueError("chunk_words must be positive")
    size = rf.sensor_size if sensor_size is None else sensor_size
    state = None
    for a in range(0, len(rf.words), chunk_words):
        piece, state = _decode(rf.words[a:a + chunk_words], fmt, size, ts, state, True, on_out_of_range, device)
        yield piece


def decode_raw(path_or_rawfile, chunk_words=1 << 26, sensor_size=None, ts="us", on_out_of_range="raise", device=None):
    """All events of a .raw file (a path or a RawFile) as one RawEvents: iter_decode_raw's pieces concatenated, their stats summed.
    The columns of the whole file must fit the device; a larger file is processed piece by piece with iter_decode_raw."""
    pieces = list(iter_decode_raw(path_or_rawfile, chunk_words, sensor_size, ts, on_out_of_range, device))
    if not pieces:
        return _decode(np.empty(0, dtype=np.uint16), _lib.EVK_RAW_EVT3, None, ts, None, False, on_out_of_range, device)
    if len(pieces) == 1:
        return pieces[0]
    cols = [torch.cat([p[k] for p in pieces]) for k in range(4)]
    return RawEvents(*cols, RawStats(*(sum(v) for v in zip(*(p.stats for p in pieces)))))


# ---- encoding (host numpy) --------------------------------------------------------------------------------------------------

def _event_columns(xs, ys, ts_us, ps, t_limit):
    x, y, t, p = (np.asarray(v).reshape(-1) for v in (xs, ys, ts_us, ps))
    if not (len(x) == len(y) == len(t) == len(p)):
        raise ValueError("event columns differ in length")
    if len(x) and any(v.dtype.kind not in "iub" for v in (x, y, t)):
        raise TypeError("xs, ys and ts_us must be integer columns (microseconds)")
    x, y, t = x.astype(np.int64), y.astype(np.int64), t.astype(np.int64)
    p = (np.asarray(p) > 0).astype(np.int64)
    if len(x):
        if x.min() < 0 or x.max() > 2047 or y.min() < 0 or y.max() > 2047:
            raise ValueError("coordinates must lie in [0, 2047]")
        if t.min() < 0 or t.max() >= t_limit:
            raise ValueError("timestamps must lie in [0, %d) microseconds" % t_limit)
        if np.any(t[1:] < t[:-1]):
            raise ValueError("timestamps go back: the events must be ordered by time")
    return x, y, t, p


def encode_evt3(xs, ys, ts_us, ps, vectorize=True):
    """Events -> EVT3 words (uint16).  xs, ys in [0, 2047]; ts_us non-decreasing integer microseconds; ps > 0 is ON.  An event
    (or, with vectorize, a group of events of one row, time and polarity whose x ascend inside one 12-column cell counted from
    the run's first x) becomes, in this order: TIME_HIGH when bits 12-23 of the time changed and in front of every 16th group
    (the format's redundancy; a step into another 2^24 us loop is led through TIME_HIGH 4095, 0 so that the decoder counts it),
    TIME_LOW and ADDR_Y when they changed, then ADDR_X -- or VECT_BASE_X, left out when the VECT_12 just before carried the base
    here, and VECT_12 / VECT_8 (all offsets below 8)."""
    x, y, t, p = _event_columns(xs, ys, ts_us, ps, 1 << 62)
    n = len(x)
    if n == 0:
        return np.empty(0, dtype=np.uint16)
    # groups: (segment, cell) with segment = run of one row, time and polarity with ascending x
    if vectorize:
        brk = np.ones(n, dtype=bool)
        brk[1:] = (y[1:] != y[:-1]) | (t[1:] != t[:-1]) | (p[1:] != p[:-1]) | (x[1:] <= x[:-1])
        seg = np.cumsum(brk) - 1
        seg_x0 = x[brk][seg]
        cell = (x - seg_x0) // 12
        first = brk.copy()
        first[1:] |= cell[1:] != cell[:-1]
    else:
        seg = np.arange(n)
        seg_x0, cell, first = x, np.zeros(n, dtype=np.int64), np.ones(n, dtype=bool)
    g = np.cumsum(first) - 1                                # group of every event
    gi = np.flatnonzero(first)                              # first event of every group
    ng = len(gi)
    count = np.bincount(g, minlength=ng)
    base = seg_x0[gi] + 12 * cell[gi]
    mask = np.bincount(g, weights=(1 << (x - base[g])).astype(np.float64), minlength=ng).astype(np.int64)
    gy, gt, gp, gseg, gcell = y[gi], t[gi], p[gi], seg[gi], cell[gi]
    is_vec = count > 1
    vec8 = is_vec & (mask < 256)
    vec12 = is_vec & ~vec8
    need_base = is_vec.copy()
    need_base[1:] &= ~(vec12[:-1] & (gseg[1:] == gseg[:-1]) & (gcell[1:] == gcell[:-1] + 1))
    hi = gt >> 12                                           # unbounded TIME_HIGH; bits 12+ of it are the loop
    hi_prev = np.concatenate(([0], hi[:-1]))
    crossings = (hi >> 12) - (hi_prev >> 12)
    need_th = (hi != hi_prev) | (np.arange(ng) % 16 == 0)
    tl = gt & 0xFFF
    need_tl = tl != np.concatenate(([0], tl[:-1]))
    need_y = gy != np.concatenate(([0], gy[:-1]))
    per = 2 * crossings + need_th + need_tl + need_y + need_base + 1
    end = np.cumsum(per)
    out = np.empty(int(end[-1]), dtype=np.uint16)
    pos = end - per
    for k in np.flatnonzero(crossings):                     # (one group per 16.8 s of stream)
        c = 2 * int(crossings[k])
        out[pos[k]:pos[k] + c] = np.tile(np.array([0x8FFF, 0x8000], dtype=np.uint16), c // 2)
    pos = pos + 2 * crossings
    for need, word in ((need_th, 0x8000 | (hi & 0xFFF)), (need_tl, 0x6000 | tl), (need_y, gy), (need_base, 0x3000 | (gp << 11) | base)):
        out[pos[need]] = word[need]
        pos = pos + need
    out[pos] = np.where(is_vec, np.where(vec8, 0x5000, 0x4000) | mask, 0x2000 | (gp << 11) | x[gi])
    return out


def encode_evt2(xs, ys, ts_us, ps):
    """Events -> EVT2 words (uint32): TIME_HIGH (bits 6-33 of the time) when it changed and in front of every 16th event, then
    CD_OFF / CD_ON with the time's low 6 bits.  Times below 2^34 us."""
    x, y, t, p = _event_columns(xs, ys, ts_us, ps, 1 << 34)
    n = len(x)
    if n == 0:
        return np.empty(0, dtype=np.uint32)
    hi = t >> 6
    need_th = (hi != np.concatenate(([-1], hi[:-1]))) | (np.arange(n) % 16 == 0)
    end = np.cumsum(need_th + 1)
    out = np.empty(int(end[-1]), dtype=np.uint32)
    out[end - 1] = (p << 28) | ((t & 0x3F) << 22) | (x << 11) | y
    out[(end - 2)[need_th]] = (0x8 << 28) | hi[need_th]
    return out
