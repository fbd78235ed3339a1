"""GPU (-m gpu): the EVT3 / EVT2 decoder (evk_rawdecode.hip behind event_utils_amd.data_formats) against the sequential
restatement of the decoding rules (tests/_raw_np.py).  Every comparison is BITWISE on the four columns, the stats and the
returned state; there is no tolerance in this feature.  C is the chunk (words per workgroup), S the number of lanes of the scan
launch (beyond S chunks a lane combines several): the cases sit on their borders.  check() decodes through both write kernels --
the staged one of the public calls and the one behind EVK_RAW_DIRECT_STORES -- and holds each to the restatement and to the other."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _raw_np as R  # noqa: E402
import _raw_streams as G  # noqa: E402
from _raw_streams import same  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def E():
    import event_utils_amd as E
    from event_utils_amd import _lib
    _lib.lib()
    assert torch.cuda.is_available()
    return E


def _C():
    from event_utils_amd import _lib
    return _lib.EVK_RAW_CHUNK, _lib.EVK_RAW_SCAN_WIDTH


def _fns(E, fmt):
    return (E.decode_evt3, R.decode_evt3) if fmt == 3 else (E.decode_evt2, R.decode_evt2)


def direct(E, words, fmt=3, sensor_size=None, ts="us", state=None, on_out_of_range="raise"):
    """(RawEvents, RawState) of the public call's worker with EVK_RAW_DIRECT_STORES: the write kernel without the LDS staging"""
    from event_utils_amd import _lib
    from event_utils_amd.data_formats import raw
    return raw._decode(words, fmt, sensor_size, ts, state, True, on_out_of_range, None, flags=_lib.EVK_RAW_DIRECT_STORES)


def same_bits(a, b):
    """two device results: the same columns bit for bit, the same stats"""
    for k in range(4):
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k
    assert tuple(a.stats) == tuple(b.stats)


def check(E, words, fmt=3, state=None, ref=None):
    """the staged and the direct write against the restatement, and against each other"""
    dec, rdec = _fns(E, fmt)
    ref = rdec(words, state=state) if ref is None else ref
    out, st = dec(words, state=state, return_state=True)
    same(out, st, ref)
    out_d, st_d = direct(E, words, fmt, state=state)
    same(out_d, st_d, ref)
    same_bits(out, out_d)
    assert st == st_d
    return ref


def stream(fmt, seed, n, **kw):
    rng = np.random.default_rng(seed)
    return G.structured_evt3(rng, n, **kw) if fmt == 3 else G.structured_evt2(rng, n, **kw)


@pytest.mark.parametrize("fmt", [3, 2])
def test_word_counts_around_the_chunk(E, fmt):
    C, _ = _C()
    whole = stream(fmt, 10 + fmt, 3 * C + 7)
    for n in (0, 1, C - 1, C, C + 1, 3 * C + 7):
        ref = check(E, whole[:n], fmt)
        assert n < C - 1 or ref[4][0] > 0


def test_state_set_in_chunk_0_and_first_used_in_chunk_2(E):
    C, _ = _C()
    rng = np.random.default_rng(0)
    head = np.array([0x8123, 0x6456, 0x0321, 0x3ABC], dtype=np.uint16)       # TIME_HIGH, TIME_LOW, ADDR_Y, VECT_BASE_X (ON)
    fill = lambda k: (0x2000 | rng.integers(0, 4096, k)).astype(np.uint16)  # noqa: E731
    words = np.concatenate((head, fill(C - 4), fill(C), np.array([0x4A5A, 0x50F0, 0x2001], dtype=np.uint16), fill(100)))
    ref = check(E, words)
    assert ref[0][2 * C - 4] == 0x2BC + 1 and ref[1][2 * C - 4] == 0x321 and ref[2][2 * C - 4] == (0x123 << 12) + 0x456


def test_a_base_as_last_word_of_a_chunk_and_a_full_vector_run_beyond_the_next(E):
    C, _ = _C()
    words = np.concatenate((np.array([0x8001, 0x0007], dtype=np.uint16), np.full(C - 3, 0x2005, dtype=np.uint16),
                            np.array([0x3000], dtype=np.uint16), np.full(C + 10, 0x4FFF, dtype=np.uint16),
                            np.array([0x50FF, 0x2003], dtype=np.uint16)))
    assert words[C - 1] == 0x3000
    ref = check(E, words)
    assert ref[4][0] == (C - 3) + 12 * (C + 10) + 8 + 1            # chunk 1 alone expands to 12 C events
    assert ref[0].min() < 0                                        # the run passes x = 32767: 16-bit base_x, int16 x


def test_time_high_4095_as_last_word_of_a_chunk_and_0_as_first_of_the_next(E):
    C, _ = _C()
    words = np.concatenate((np.array([0x8FF0], dtype=np.uint16), np.full(C - 2, 0x2005, dtype=np.uint16),
                            np.array([0x8FFF, 0x8000, 0x2006], dtype=np.uint16)))
    assert words[C - 1] == 0x8FFF and words[C] == 0x8000
    ref = check(E, words)
    assert ref[4][6] == 1 and ref[2][-1] == 1 << 24 and ref[5][5] == 1


def test_a_loop_whose_previous_time_high_lies_two_chunks_back(E):
    C, _ = _C()
    words = np.concatenate((np.array([0x8FFF], dtype=np.uint16), np.full(2 * C + 5, 0x2005, dtype=np.uint16),
                            np.array([0x8003, 0x2006, 0x8001, 0x2007], dtype=np.uint16)))
    ref = check(E, words)
    assert ref[4][6] == 1 and ref[4][4] == 1 and ref[2][-1] == (1 << 24) + (1 << 12)


def test_streams_without_time(E):
    C, _ = _C()
    words = stream(3, 5, 2 * C + 50, start_time=False)
    words = words[(words >> 12) != 8]
    ref = check(E, words)
    emitting = R.decode_evt3(np.concatenate((np.array([0x8000], dtype=np.uint16), words)))
    assert ref[4][0] == 0 and ref[4][3] == emitting[4][0] > 0 and not ref[5][6]
    # the only TIME_HIGH is the last word: still nothing, but the state has time now
    ref = check(E, np.concatenate((words, np.array([0x8005], dtype=np.uint16))))
    assert ref[4][0] == 0 and ref[5][6] and ref[5][4] == 5
    w2 = stream(2, 5, C + 9, start_time=False)
    w2 = w2[(w2 >> 28) != 8]
    ref = check(E, w2, 2)
    assert ref[4][0] == 0 and ref[4][3] > 0
    check(E, np.concatenate((w2, np.array([0x80000005], dtype=np.uint32))), 2)


def test_the_handmade_fixtures_on_the_device(E, golden):
    for fmt, name in ((3, "raw/evt3_handmade"), (2, "raw/evt2_handmade")):
        g = golden(name)
        out, st = _fns(E, fmt)[0](g["words"], return_state=True)
        for k, col in enumerate(("xs", "ys", "ts", "ps")):
            assert np.array_equal(out[k].cpu().numpy(), g[col]) and out[k].cpu().numpy().dtype == g[col].dtype
        check(E, g["words"], fmt)
        # bytes are words too
        same(_fns(E, fmt)[0](g["words"].tobytes()), None, _fns(E, fmt)[1](g["words"]))


@pytest.mark.parametrize("fmt", [3, 2])
def test_split_invariance(E, fmt):
    C, _ = _C()
    dec, rdec = _fns(E, fmt)
    words = stream(fmt, 20 + fmt, 2 * C + 300)
    if fmt == 3:                                                   # a vector run across the middle cut
        words[C + 100:C + 110] = [0x3010] + [0x4FFF] * 9
    whole = rdec(words)
    check(E, words, fmt, ref=whole)
    for k in (1, C - 1, C, C + 1, C + 105):
        a, sa = dec(words[:k], return_state=True)
        b, sb = dec(words[k:], state=sa, return_state=True)
        ra = rdec(words[:k])
        same(a, sa, ra)
        same(b, sb, rdec(words[k:], state=ra[5]))
        for c in range(4):
            assert np.array_equal(torch.cat((a[c], b[c])).cpu().numpy(), whole[c])
        assert tuple(u + v for u, v in zip(a.stats, b.stats)) == whole[4] and tuple(sb) == whole[5]


@pytest.mark.parametrize("fmt", [3, 2])
def test_slices_of_a_resident_tensor_are_read_in_place(E, fmt):
    C, _ = _C()
    words = stream(fmt, 30 + fmt, 2 * C + 77, start_time=False)
    dev = torch.from_numpy(words.view(np.int16 if fmt == 3 else np.int32)).cuda()
    dec, rdec = _fns(E, fmt)
    for k in (1, 3, 4, C + 1):
        out, st = dec(dev[k:], return_state=True)
        same(out, st, rdec(words[k:]))
    out = dec(dev.view(torch.uint8)[2 * (fmt == 3) + 4:])          # bytes, from a word boundary
    same(out, None, rdec(words[(3 if fmt == 3 else 1):]))


def test_sensor_size_counts_raises_keeps_and_drops(E):
    C, _ = _C()
    words = stream(3, 40, C + 500)
    H, W = 480, 640
    ref = R.decode_evt3(words, sensor_size=(H, W))
    n_bad = ref[4][5]
    assert 0 < n_bad < ref[4][0]
    with pytest.raises(ValueError, match=r"\b%d of %d\b" % (n_bad, ref[4][0])):
        E.decode_evt3(words, sensor_size=(H, W))
    out, st = E.decode_evt3(words, sensor_size=(H, W), on_out_of_range="keep", return_state=True)
    same(out, st, ref)
    out_d, st_d = direct(E, words, sensor_size=(H, W), on_out_of_range="keep")
    same(out_d, st_d, ref)
    same_bits(out, out_d)
    out, st = E.decode_evt3(words, sensor_size=(H, W), on_out_of_range="drop", return_state=True)
    keep = (ref[0].view(np.uint16) < W) & (ref[1].view(np.uint16) < H)
    stats = (int(keep.sum()),) + ref[4][1:]
    same(out, st, tuple(c[keep] for c in ref[:4]) + (stats, ref[5]))
    # a sensor that holds everything: nothing to report, whatever the policy
    same(E.decode_evt3(words, sensor_size=(65535, 65535)), None, R.decode_evt3(words, sensor_size=(65535, 65535)))
    e2 = stream(2, 41, 300)
    r2 = R.decode_evt2(e2, sensor_size=(H, W))
    assert r2[4][5] > 0
    same(E.decode_evt2(e2, sensor_size=(H, W), on_out_of_range="keep"), None, r2)
    same(direct(E, e2, 2, sensor_size=(H, W), on_out_of_range="keep")[0], None, r2)
    with pytest.raises(ValueError):
        E.decode_evt3(words, on_out_of_range="ignore")
    with pytest.raises(ValueError):
        E.decode_evt3(words, ts="ms")


def test_drop_removes_the_events_that_were_counted_on_a_sensor_wider_than_an_int16(E):
    """x is a 16-bit value stored as its int16 bits, and the count of events off the sensor compares it unsigned (evk.h).  On a sensor
    wider than 32768 columns a negative int16 may therefore lie inside: 'drop' removes the events that were counted, no others.
    (Found by the fuzz kind raw: a signed box dropped every negative x as well.)"""
    H, W = 1024, 40_000
    words = np.concatenate((np.array([0x8001, 0x0005, 0x37FF], dtype=np.uint16), np.full(4000, 0x4FFF, dtype=np.uint16),
                            np.array([0x0400, 0x2005], dtype=np.uint16)))      # x = 2047 .. 50046 in row 5, then one event in row 1024
    ref = R.decode_evt3(words, sensor_size=(H, W))
    keep = (ref[0].view(np.uint16) < W) & (ref[1].view(np.uint16) < H)
    assert ref[4][0] == 48001 and ref[4][5] == (50047 - W) + 1 == int((~keep).sum())
    assert (ref[0][keep] < 0).sum() == W - 32768 and not keep[-1]
    for dec in (lambda: E.decode_evt3(words, sensor_size=(H, W), on_out_of_range="drop", return_state=True),
                lambda: direct(E, words, sensor_size=(H, W), on_out_of_range="drop")):
        out, st = dec()
        same(out, st, tuple(c[keep] for c in ref[:4]) + ((int(keep.sum()),) + ref[4][1:], ref[5]))
        assert out.stats.events + out.stats.out_of_range == ref[4][0]
    # up to 32768 columns the int16 columns are clipped as they are: every negative x is off the sensor
    ref = R.decode_evt3(words, sensor_size=(H, 32768))
    out = E.decode_evt3(words, sensor_size=(H, 32768), on_out_of_range="drop")
    keep = (ref[0] >= 0) & (ref[1] < H)
    same(out, None, tuple(c[keep] for c in ref[:4]) + ((int(keep.sum()),) + ref[4][1:], ref[5]))
    assert ref[4][5] == int((~keep).sum()) and out.xs.min() >= 0


def test_more_chunks_than_the_scan_has_lanes(E):
    """mostly ADDR_X / TIME_LOW words (the restatement's loop stays short), with state that must cross the lanes' runs of chunks: a
    loop whose halves lie S chunks apart, a base and a row set in chunk 0 and used behind chunk S"""
    C, S = _C()
    n = S * C + 3 * C + 11
    rng = np.random.default_rng(7)
    words = (0x2000 | rng.integers(0, 4096, n)).astype(np.uint16)
    tl = rng.integers(0, n, n // 50)
    words[tl] = 0x6000 | rng.integers(0, 4096, len(tl))
    words[0], words[1], words[2] = 0x8FFE, 0x0123, 0x3805
    words[S * C - 1] = 0x8FFF
    words[S * C + 5] = 0x8001
    words[S * C + 9] = 0x4081
    words[(S + 2) * C] = 0x8000                                     # a small step back two chunks on
    ref = check(E, words)
    assert ref[4][6] == 1 and ref[4][4] == 1 and ref[4][0] > S * C * 9 // 10
    # EVT2 over the same border
    w2 = ((rng.integers(0, 2, n) << 28) | rng.integers(0, 1 << 28, n)).astype(np.uint32)
    w2[[0, S * C - 1, S * C + 1]] = [0x80000001, 0x80000002, 0x80000003]
    check(E, w2, 2)


@pytest.mark.parametrize("fmt", [3, 2])
def test_seconds_are_the_microseconds_divided_once(E, fmt):
    C, _ = _C()
    words = stream(fmt, 50 + fmt, C + 33)
    dec, rdec = _fns(E, fmt)
    ref = rdec(words)
    for out in (dec(words, ts="seconds"), direct(E, words, fmt, ts="seconds")[0]):
        assert out.ts.dtype == torch.float64
        assert np.array_equal(out.ts.cpu().numpy().view(np.uint64), (ref[2] / 1e6).view(np.uint64))
        for k in (0, 1, 3):
            assert np.array_equal(out[k].cpu().numpy(), ref[k])
        assert tuple(out.stats) == ref[4]


def test_decoded_events_feed_the_voxel_grid(E):
    H, W, B = 480, 640, 5
    rng = np.random.default_rng(3)
    n = 20000
    x, y = rng.integers(0, W, n), rng.integers(0, H, n)
    t = np.sort(rng.integers(1_000_000, 1_050_000, n))
    p = rng.integers(0, 2, n)
    words = E.encode_evt3(x, y, t, p)
    ref = R.decode_evt3(words)
    assert np.array_equal(ref[0], x) and np.array_equal(ref[2], t)
    for ts in ("us", "seconds"):
        ev = E.decode_evt3(words, sensor_size=(H, W), ts=ts).to_device_events()
        got = E.events_to_voxel_torch(ev, None, None, None, B, sensor_size=(H, W))
        want = E.events_to_voxel_torch(E.DeviceEvents.from_native(ref[0], ref[1], ref[2] / 1e6, ref[3]), None, None, None, B,
                                       sensor_size=(H, W))
        assert torch.equal(got, want) and float(got.abs().sum()) > 0


@pytest.mark.parametrize("fmt", ["evt3", "evt2"])
def test_decode_raw_reads_a_written_file_in_pieces(E, fmt, tmp_path):
    C, _ = _C()
    k = 3 if fmt == "evt3" else 2
    words = stream(k, 60 + k, 3 * C + 100)
    path = str(tmp_path / "rec.raw")
    E.write_raw(path, words, fmt, (2048, 2048))
    ref = _fns(E, k)[1](words, sensor_size=(2048, 2048))
    rf = E.read_raw(path)
    assert rf.format == fmt and rf.sensor_size == (2048, 2048) and np.array_equal(rf.words, words)
    for chunk_words in (C + 13, 1 << 26):
        same(E.decode_raw(path, chunk_words=chunk_words, on_out_of_range="keep"), None, ref)
    pieces = list(E.iter_decode_raw(rf, chunk_words=C + 13, on_out_of_range="keep"))
    assert len(pieces) == -(-len(words) // (C + 13)) >= 3 and sum(p.stats.events for p in pieces) == ref[4][0]
    assert np.array_equal(torch.cat([p.ts for p in pieces]).cpu().numpy(), ref[2])


def test_round_trip_from_the_simulator_to_time_surfaces(E, tmp_path):
    """simulate_events -> encode_evt3 -> write_raw -> decode_raw -> time_surfaces equals the surfaces of the simulator's own events"""
    H, W = 24, 32
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    frames = np.stack([1.5 * np.sin(0.4 * (xx - 1.7 * k) + 0.2 * yy) for k in range(6)])
    xs, ys, ts, ps = E.simulate_events(frames, 1.0e6 + 2.0e3 * np.arange(6), 0.2, 0.2)
    t_us = np.floor(ts).astype(np.int64)
    assert len(xs) > 1000
    for fmt, words in (("evt3", E.encode_evt3(xs, ys, t_us, ps > 0)), ("evt2", E.encode_evt2(xs, ys, t_us, ps > 0))):
        path = str(tmp_path / (fmt + ".raw"))
        E.write_raw(path, words, fmt, (H, W))
        rec = E.decode_raw(path, ts="seconds")
        assert rec.stats.events == len(xs) and rec.stats.out_of_range == 0
        assert np.array_equal(rec.xs.cpu().numpy(), xs) and np.array_equal(rec.ts.cpu().numpy(), t_us / 1e6)
        t_ref = [t_us[-1] / 1e6]
        got = E.time_surfaces(rec.to_device_events(), None, None, None, 0.01, (H, W), t_refs=t_ref)
        want = E.time_surfaces(E.DeviceEvents.from_native(xs.astype(np.int16), ys.astype(np.int16), t_us / 1e6, (ps > 0).astype(np.uint8)),
                               None, None, None, 0.01, (H, W), t_refs=t_ref)
        assert torch.equal(torch.as_tensor(got), torch.as_tensor(want)) and float(torch.as_tensor(got).sum()) > 0
