"""CPU (no GPU): the .raw header parser, the hand-assembled EVT3 / EVT2 streams against the sequential restatement of the decoding
rules (tests/_raw_np.py), the host encoders through that restatement, and the argument checks of the three evk_raw_* entry points
(pointers that are never dereferenced: every call is answered before a launch)."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _raw_np as R  # noqa: E402

# ---- a hand-assembled EVT3 stream: every word with what it does -------------------------------------------------------------
T0 = (4094 << 12) + 0x123
T1 = (4095 << 12) + 0xFFF
T2 = 1 << 24                                    # after the loop 4095 -> 0
T3 = (1 << 24) + (12 << 12) + 5
T4 = (1 << 24) + (17 << 12) + 5
EVT3_WORDS = np.array([
    0x0005,   # ADDR_Y 5
    0x2803,   # ADDR_X 3, ON: before the first TIME_HIGH                                   (before_time 1)
    0x4003,   # VECT_12 bits 0, 1: before the first TIME_HIGH; base_x 0 -> 12              (before_time 3)
    0x6123,   # TIME_LOW 0x123
    0x8FFE,   # TIME_HIGH 4094
    0x200A,   # ADDR_X 10, OFF                         -> (10, 5, T0, 0)
    0x3814,   # VECT_BASE_X 20, ON
    0x4805,   # VECT_12 bits 0, 2, 11                  -> (20 | 22 | 31, 5, T0, 1); base_x -> 32
    0x5081,   # VECT_8 bits 0, 7 (base carried by 12)  -> (32 | 39, 5, T0, 1); base_x -> 40
    0xA001,   # EXT_TRIGGER                                                                (triggers 1)
    0x8FFF,   # TIME_HIGH 4095
    0x6FFF,   # TIME_LOW 0xFFF
    0x2FFF,   # ADDR_X 2047, ON                        -> (2047, 5, T1, 1)
    0x8000,   # TIME_HIGH 0: 4095 - 0 >= 4085, a loop                                      (loops 1)
    0x6000,   # TIME_LOW 0
    0x0FFF,   # ADDR_Y 2047 (bit 11 ignored)
    0x2000,   # ADDR_X 0, OFF                          -> (0, 2047, T2, 0)
    0x8010,   # TIME_HIGH 16
    0x800C,   # TIME_HIGH 12: a small step back, taken as it comes                         (time_went_back 1)
    0x6005,   # TIME_LOW 5
    0x2001,   # ADDR_X 1, OFF                          -> (1, 2047, T3, 0)
    0x7ABC,   # reserved type 7                                                            (other 1)
    0xF000,   # type 0xF                                                                   (other 2)
    0x1234,   # type 1                                                                     (other 3)
    0x3005,   # VECT_BASE_X 5, OFF
    0x4000,   # VECT_12, empty; base_x -> 17
    0x50FF,   # VECT_8, full                           -> (17 .. 24, 2047, T3, 0); base_x -> 25
    0x0003,   # ADDR_Y 3
    0x4FFF,   # VECT_12, full                          -> (25 .. 36, 3, T3, 0); base_x -> 37
    0x8011,   # TIME_HIGH 17
    0x2802,   # ADDR_X 2, ON                           -> (2, 3, T4, 1)
], dtype=np.uint16)
EVT3_XS = [10, 20, 22, 31, 32, 39, 2047, 0, 1] + list(range(17, 25)) + list(range(25, 37)) + [2]
EVT3_YS = [5] * 7 + [2047, 2047] + [2047] * 8 + [3] * 12 + [3]
EVT3_TS = [T0] * 6 + [T1, T2, T3] + [T3] * 20 + [T4]
EVT3_PS = [0, 1, 1, 1, 1, 1, 1, 0, 0] + [0] * 20 + [1]
EVT3_STATS = (30, 1, 3, 3, 1, 0, 1)              # events, triggers, other, before_time, time_went_back, out_of_range, loops
EVT3_STATE = (3, 37, 0, 5, 17, 1, True)          # y, base_x, vect_pol, t_low, t_high, loops, have_time


def _cd(kind, t6, x, y):
    return (kind << 28) | (t6 << 22) | (x << 11) | y


EVT2_WORDS = np.array([
    _cd(1, 5, 3, 4),               # CD_ON before the first TIME_HIGH                      (before_time 1)
    (0x8 << 28) | 100,             # TIME_HIGH 100
    _cd(0, 7, 10, 20),             # CD_OFF                  -> (10, 20, 100 << 6 | 7, 0)
    _cd(1, 63, 2047, 2047),        # CD_ON                   -> (2047, 2047, 100 << 6 | 63, 1)
    (0xA << 28) | 1,               # EXT_TRIGGER                                           (triggers 1)
    (0x8 << 28) | 0x0FFFFFFF,      # TIME_HIGH, all 28 bits
    _cd(1, 0, 0, 0),               # CD_ON                   -> (0, 0, 0x0FFFFFFF << 6, 1)
    (0x8 << 28) | 50,              # TIME_HIGH 50: back, taken as it comes, not counted
    _cd(0, 1, 5, 6),               # CD_OFF                  -> (5, 6, 50 << 6 | 1, 0)
    (0xE << 28) | 0x123,           # type 0xE                                              (other 1)
    0xF << 28,                     # type 0xF                                              (other 2)
    (0x2 << 28) | 5,               # type 2                                                (other 3)
    _cd(1, 2, 639, 479),           # CD_ON                   -> (639, 479, 50 << 6 | 2, 1)
], dtype=np.uint32)
EVT2_XS = [10, 2047, 0, 5, 639]
EVT2_YS = [20, 2047, 0, 6, 479]
EVT2_TS = [(100 << 6) | 7, (100 << 6) | 63, 0x0FFFFFFF << 6, (50 << 6) | 1, (50 << 6) | 2]
EVT2_PS = [0, 1, 1, 0, 1]
EVT2_STATS = (5, 1, 3, 1, 0, 0, 0)
EVT2_STATE = (0, 0, 0, 0, 50, 0, True)


def _check(got, xs, ys, ts, ps, stats, state):
    assert got[0].dtype == np.int16 and got[1].dtype == np.int16 and got[2].dtype == np.int64 and got[3].dtype == np.uint8
    assert got[0].tolist() == xs and got[1].tolist() == ys and got[2].tolist() == ts and got[3].tolist() == ps
    assert got[4] == stats and got[5] == state


def test_the_restatement_reproduces_the_handmade_evt3_stream(golden):
    assert len(EVT3_XS) == len(EVT3_YS) == len(EVT3_TS) == len(EVT3_PS) == 30
    _check(R.decode_evt3(EVT3_WORDS), EVT3_XS, EVT3_YS, EVT3_TS, EVT3_PS, EVT3_STATS, EVT3_STATE)
    g = golden("raw/evt3_handmade")
    assert sorted(g.files) == ["ps", "ts", "words", "xs", "ys"]
    assert g["words"].dtype == np.uint16 and np.array_equal(g["words"], EVT3_WORDS)
    _check(R.decode_evt3(g["words"]), g["xs"].tolist(), g["ys"].tolist(), g["ts"].tolist(), g["ps"].tolist(), EVT3_STATS, EVT3_STATE)
    assert g["xs"].tolist() == EVT3_XS and g["ts"].tolist() == EVT3_TS
    # with a sensor: x = 2047 and the two rows y = 2047 are off a 640 x 480 one
    assert R.decode_evt3(EVT3_WORDS, sensor_size=(480, 640))[4][5] == 1 + 2 + 8


def test_the_restatement_reproduces_the_handmade_evt2_stream(golden):
    _check(R.decode_evt2(EVT2_WORDS), EVT2_XS, EVT2_YS, EVT2_TS, EVT2_PS, EVT2_STATS, EVT2_STATE)
    g = golden("raw/evt2_handmade")
    assert g["words"].dtype == np.uint32 and np.array_equal(g["words"], EVT2_WORDS)
    _check(R.decode_evt2(g["words"]), g["xs"].tolist(), g["ys"].tolist(), g["ts"].tolist(), g["ps"].tolist(), EVT2_STATS, EVT2_STATE)


def test_the_restatement_continues_from_a_state():
    for words, dec in ((EVT3_WORDS, R.decode_evt3), (EVT2_WORDS, R.decode_evt2)):
        whole = dec(words)
        for k in range(len(words) + 1):
            a = dec(words[:k])
            b = dec(words[k:], state=a[5])
            for c in range(4):
                assert np.array_equal(np.concatenate((a[c], b[c])), whole[c])
            assert tuple(u + v for u, v in zip(a[4], b[4])) == whole[4] and b[5] == whole[5]


# ---- the header ----------------------------------------------------------------------------------------------------------------

def test_header_parsing(tmp_path):
    from event_utils_amd.data_formats import parse_raw_header, read_raw
    payload = EVT3_WORDS.tobytes()
    new = b"% date 2024-01-01 10:00:00\n% evt 3.0\n% format EVT3;height=720;width=1280\n% geometry 1280x720\n% end\n"
    fmt, size, header, n = parse_raw_header(new + payload)
    assert (fmt, size, n) == ("evt3", (720, 1280), len(new)) and header["date"] == "2024-01-01 10:00:00" and header["evt"] == "3.0"
    # an older file: no '% end', the header ends at the first line that does not start with '%'; geometry alone gives the size
    old = b"% Date 2020-02-02\n% evt 2.0\n% geometry 640x480\n"
    assert parse_raw_header(old + EVT2_WORDS.tobytes())[:2] == ("evt2", (480, 640))
    assert parse_raw_header(old + EVT2_WORDS.tobytes())[3] == len(old)
    # '% format' alone names format and size; a payload whose first byte is '%' is protected by '% end'
    only = b"% format EVT2;height=480;width=640\n% end\n"
    assert parse_raw_header(only + b"%%%%")[:2] == ("evt2", (480, 640)) and parse_raw_header(only + b"%%%%")[3] == len(only)
    assert parse_raw_header(b"% evt 3.0\n% end\n")[1] is None and parse_raw_header(payload)[0] is None
    # files: the payload as a map of words; a trailing half word is dropped and reported
    p = tmp_path / "a.raw"
    p.write_bytes(new + payload + b"\x07")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        rf = read_raw(str(p))
    assert rf.format == "evt3" and rf.sensor_size == (720, 1280) and rf.trailing_bytes == 1 and len(seen) == 1
    assert isinstance(rf.words, np.memmap) and rf.words.dtype == np.uint16 and np.array_equal(rf.words, EVT3_WORDS)
    p.write_bytes(old + EVT2_WORDS.tobytes())
    rf = read_raw(str(p))
    assert rf.format == "evt2" and rf.sensor_size == (480, 640) and rf.trailing_bytes == 0 and np.array_equal(rf.words, EVT2_WORDS)
    p.write_bytes(old + EVT2_WORDS.tobytes() + b"\x01\x02\x03")
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        rf = read_raw(str(p))
    assert rf.trailing_bytes == 3 and np.array_equal(rf.words, EVT2_WORDS)
    p.write_bytes(b"% camera unknown\n% end\n" + payload)
    with pytest.raises(ValueError):
        read_raw(str(p))


def test_write_raw_round_trips_through_read_raw(tmp_path):
    from event_utils_amd.data_formats import read_raw, write_raw
    for words, fmt in ((EVT3_WORDS, "evt3"), (EVT2_WORDS, "evt2")):
        p = str(tmp_path / (fmt + ".raw"))
        write_raw(p, words, fmt, (480, 640))
        rf = read_raw(p)
        assert rf.format == fmt and rf.sensor_size == (480, 640) and rf.trailing_bytes == 0 and np.array_equal(rf.words, words)
        assert rf.words.dtype == words.dtype


# ---- the encoders through the restatement ---------------------------------------------------------------------------------------

def stream(seed, n=3000, span=40_000_000, bursts=True):
    """Seeded simulator-like events: times in bursts of equal microseconds, rows read out left to right inside a burst (so that
    vectors form), the corners x = 2047 and y = 2047 present, a time span beyond 2^24 us."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(0, span, n // 8 if bursts else n))
    t = np.repeat(t, 8)[:n] if bursts else t
    y = np.repeat(rng.integers(0, 2048, len(t) // 4 + 1), 4)[:len(t)]
    x = rng.integers(0, 2048, len(t))
    p = np.repeat(rng.integers(0, 2, len(t) // 4 + 1), 4)[:len(t)]
    if bursts:                                       # runs of neighbouring columns in one row: a VECT_12, a VECT_8 and single events
        x = (np.repeat(rng.integers(0, 2010, len(t) // 4 + 1), 4)[:len(t)] +
             np.tile(np.array([0, 1, 9, 14, 0, 2, 5, 30]), len(t) // 8 + 1)[:len(t)])
    x[-1], y[-1] = 2047, 2047
    x[0], y[0] = 2047, 0
    return x.astype(np.int16), y.astype(np.int16), t.astype(np.int64), p.astype(np.uint8)


@pytest.mark.parametrize("seed", [0, 1, 2])
@pytest.mark.parametrize("vectorize", [True, False])
def test_encode_evt3_then_the_restatement_returns_the_events(seed, vectorize):
    from event_utils_amd.data_formats import encode_evt3
    x, y, t, p = stream(seed, bursts=seed != 2)
    assert t[-1] - t[0] > 1 << 24
    words = encode_evt3(x, y, t, p, vectorize=vectorize)
    assert words.dtype == np.uint16
    xs, ys, ts, ps, stats, state = R.decode_evt3(words)
    assert np.array_equal(xs, x) and np.array_equal(ys, y) and np.array_equal(ts, t) and np.array_equal(ps, p)
    assert stats[0] == len(x) and stats[1:6] == (0, 0, 0, 0, 0) and stats[6] == int(t[-1]) >> 24
    kinds = set((words >> 12).tolist())
    assert kinds >= {3, 4, 5} if (vectorize and seed != 2) else not (kinds & {3, 4, 5}) or vectorize
    if vectorize and seed != 2:
        assert len(words) < len(encode_evt3(x, y, t, p, vectorize=False))
    # TIME_HIGH at least in front of every 16th group: no run of 16 * 5 words without one
    th = np.flatnonzero((words >> 12) == 8)
    assert np.diff(th).max() <= 16 * 5


@pytest.mark.parametrize("seed", [0, 1])
def test_encode_evt2_then_the_restatement_returns_the_events(seed):
    from event_utils_amd.data_formats import encode_evt2
    x, y, t, p = stream(seed)
    words = encode_evt2(x, y, t, p)
    assert words.dtype == np.uint32
    xs, ys, ts, ps, stats, state = R.decode_evt2(words)
    assert np.array_equal(xs, x) and np.array_equal(ys, y) and np.array_equal(ts, t) and np.array_equal(ps, p)
    assert stats == (len(x), 0, 0, 0, 0, 0, 0)


def test_encoders_refuse_what_the_formats_cannot_hold():
    from event_utils_amd.data_formats import encode_evt2, encode_evt3
    one = np.array([1])
    for enc in (encode_evt3, encode_evt2):
        with pytest.raises(ValueError):
            enc([1, 2], [1, 2], [5, 4], [1, 1])                  # time goes back
        with pytest.raises(ValueError):
            enc([2048], one, one, one)
        with pytest.raises(ValueError):
            enc(one, [-1], one, one)
        with pytest.raises(TypeError):
            enc(one, one, [0.5], one)
        assert len(enc([], [], [], [])) == 0
    with pytest.raises(ValueError):
        encode_evt2(one, one, [1 << 34], one)
    # a vector run that continues into the next 12-column cell needs no second base
    w = encode_evt3([5, 16, 17, 18, 29], [7] * 5, [100] * 5, [1] * 5)
    assert (w >> 12).tolist() == [8, 6, 0, 3, 4, 5, 2] and R.decode_evt3(w)[0].tolist() == [5, 16, 17, 18, 29]


def test_the_public_names_and_the_reference_alias():
    import event_utils_amd as E
    import event_utils_amd.lib.data_formats as A
    from event_utils_amd import _lib
    assert A is E.data_formats and A.raw.decode_evt3 is E.decode_evt3
    for name in ("read_raw", "write_raw", "decode_evt3", "decode_evt2", "decode_raw", "iter_decode_raw", "encode_evt3", "encode_evt2",
                 "RawFile", "RawEvents"):
        assert getattr(E, name) is getattr(A, name)
    assert _lib.EVK_RAW_CHUNK == 4096 and _lib.EVK_RAW_SCAN_WIDTH == 256
    assert E.RawState() == R.INITIAL


# ---- the C entry points: refused (or answered) before anything is launched ----------------------------------------------------------

def test_scratch_bytes_refuses_counts_out_of_range_and_steps_once_per_chunk():
    from event_utils_amd import _lib
    size, C, top = _lib.lib().evk_raw_decode_scratch_bytes, _lib.EVK_RAW_CHUNK, _lib.EVK_RAW_MAX_WORDS
    assert size(-1) == _lib.EVK_EINVAL and size(-(1 << 62)) == _lib.EVK_EINVAL
    assert size(top + 1) == _lib.EVK_EINVAL and size((1 << 63) - 1) == _lib.EVK_EINVAL
    assert size(0) > 0 and size(0) % 16 == 0 and size(top) > size(top - C) > 0
    # constant inside a chunk, a step up behind every multiple of the chunk: non-decreasing in n, and nowhere else a step
    for k in (0, 1, 2, 5, 6, 7, _lib.EVK_RAW_SCAN_WIDTH, 1000):
        inside = [size(k * C + d) for d in (1, 2, 15, 16, 17, 1023, 1024, 1025, C - 1, C)]
        assert len(set(inside)) == 1 and size(k * C) < inside[0] and inside[0] % 16 == 0, k
    sizes = [size(n) for n in range(0, 3 * C + 2)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:]))
    assert [n for n in range(1, len(sizes)) if sizes[n] != sizes[n - 1]] == [1, C + 1, 2 * C + 1, 3 * C + 1]


def test_raw_decode_arguments_are_refused_before_the_device_is_touched():
    from event_utils_amd import _lib
    L = _lib.lib()
    C, top = _lib.EVK_RAW_CHUNK, _lib.EVK_RAW_MAX_WORDS
    einval, escratch, evt3, evt2 = _lib.EVK_EINVAL, _lib.EVK_ESCRATCH, _lib.EVK_RAW_EVT3, _lib.EVK_RAW_EVT2
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every call below is answered without a launch
    at = ctypes.c_void_p

    def plan(words=fake, n=3 * C + 5, fmt=evt3, state=None, scratch=fake, nbytes=None, result=fake, state_out=fake):
        nbytes = L.evk_raw_decode_scratch_bytes(max(0, min(n, top))) if nbytes is None else nbytes
        return L.evk_raw_decode_plan(words, n, fmt, state, scratch, nbytes, result, state_out, None)

    def write(words=fake, n=3 * C + 5, fmt=evt3, scratch=fake, nbytes=None, result=fake, cols=fake, ts_kind=_lib.EVK_RAW_TS_US, h=0, w=0,
              flags=0):
        nbytes = L.evk_raw_decode_scratch_bytes(max(0, min(n, top))) if nbytes is None else nbytes
        return L.evk_raw_decode_write(words, n, fmt, scratch, nbytes, result, cols, cols, cols, cols, ts_kind, h, w, flags, None)
    assert plan(state_out=None) == einval and plan(result=None, state=fake) == einval
    for call in (plan, write):
        assert call(result=None) == einval and call(scratch=None) == einval
        assert call(words=None) == einval and call(words=None, n=1) == einval
        assert call(n=-1) == einval and call(n=top + 1) == einval and call(n=(1 << 63) - 1) == einval
        for fmt in (0, 1, 4, -3, 30):
            assert call(fmt=fmt) == einval
        for off in (1, 4, 8, 15):
            assert call(scratch=at(4096 + off)) == einval                        # not 16-byte aligned
        for fmt in (evt3, evt2):
            assert call(fmt=fmt, words=at(4097)) == einval and call(fmt=fmt, words=at(4099)) == einval
        assert call(fmt=evt2, words=at(4098)) == einval                          # a half word is where EVT3 words may start
        for n in (1, C, C + 1, 3 * C + 5):
            need = L.evk_raw_decode_scratch_bytes(n)
            assert call(n=n, nbytes=need - 1) == escratch and call(n=n, nbytes=0) == escratch and call(n=n, nbytes=-5) == escratch
            assert call(n=n, nbytes=need - 1, fmt=evt2) == escratch
        assert call(n=0, words=None, nbytes=L.evk_raw_decode_scratch_bytes(0) - 1) == escratch
        # EINVAL stands before ESCRATCH
        assert call(nbytes=0, fmt=7) == einval and call(nbytes=0, scratch=at(4100)) == einval and call(nbytes=0, words=at(4097)) == einval
    for kind in (-1, 2, 3, 100):
        assert write(ts_kind=kind) == einval
    assert write(h=-1, w=640) == einval and write(h=480, w=-1) == einval and write(h=-1, w=-1) == einval
    assert write(h=65536, w=640) == einval and write(h=480, w=65536) == einval and write(h=1 << 30, w=1 << 30) == einval
    assert write(h=0, w=640) == einval and write(h=480, w=0) == einval                       # exactly one side given
    for flags in (2, 3, 4, 1 << 31, 0xFFFFFFFE, _lib.EVK_RAW_DIRECT_STORES | 8):
        assert write(flags=flags) == einval
    # the write's own checks stand before the head's: a short scratch does not hide them
    assert write(nbytes=0, flags=2) == einval and write(nbytes=0, ts_kind=5) == einval
    # nothing to write: EVK_OK without a launch, for every legal setting (the columns may be NULL)
    for fmt in (evt3, evt2):
        for kind in (_lib.EVK_RAW_TS_US, _lib.EVK_RAW_TS_SECONDS):
            for h, w in ((0, 0), (1, 1), (480, 640), (65535, 65535)):
                for flags in (0, _lib.EVK_RAW_DIRECT_STORES):
                    for words in (None, fake):
                        assert write(words=words, n=0, fmt=fmt, cols=None, ts_kind=kind, h=h, w=w, flags=flags) == _lib.EVK_OK
    assert write(n=0, h=0, w=640) == einval and write(n=0, flags=2) == einval and write(n=0, scratch=None) == einval
