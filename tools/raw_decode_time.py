"""Timings of the raw-stream decoder (event_utils_amd.data_formats; evk_rawdecode.hip) on about 10 M events at 640x480 from the
simulator's seeded scene (tools/simulate_time.py), time stamps floored to microseconds and the events of one microsecond put in
read-out order (row, then column -- what a sensor's arbiter does and what lets vectors form), encoded three ways: EVT3 with
vectors, EVT3 without, EVT2.  Per encoding: words and bytes per event; the plan call (launch 1, the chunk summaries, and launch 2,
the scan) and the write call (launch 3) by HIP events on resident words, the write both with its LDS staging and with direct
stores; the per-kernel split of one call from the profiler where it is available; the sum against 2 bytes(words) + 13 N at 8 TB/s;
the whole decode call on resident words and on host words (upload included).  Two comparisons that are NOT the code under test, in
the same run: the upload of the already decoded 13-byte columns (what a host decoder still has to pay after decoding) and a numpy
host decode (np.maximum.accumulate / cumsum formulation, EVT3 and EVT2), whose output is checked against the device's.  Every
timed repetition synchronises before and after; medians.  No time here is a pass / fail criterion.
usage: timeout 900 python tools/raw_decode_time.py [--quick] [--out profiles/raw_decode_time.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

PEAK = 8.0e12                                # bytes / s


def _fill(mask, value, idx):
    """last-write-wins: value at the last position <= i where mask holds (0 before the first), and that position (-1)"""
    pos = np.maximum.accumulate(np.where(mask, idx, -1))
    return np.where(pos >= 0, value[np.maximum(pos, 0)], 0), pos


def numpy_decode_evt3(words):
    """EVT3 on the host, vectorised: forward fills for the last-write-wins state, a cumulative sum restarted at the last
    VECT_BASE_X for base_x, np.repeat for the expansion.  (Streams whose base_x stays below 2^15.)"""
    w = words.astype(np.int64)
    typ, v = w >> 12, w & 0xFFF
    idx = np.arange(len(w))
    y, _ = _fill(typ == 0, v & 0x7FF, idx)
    tl, _ = _fill(typ == 6, v, idx)
    is_th = typ == 8
    th, thpos = _fill(is_th, v, idx)
    thv = v[is_th]
    wraps = np.zeros(len(thv), dtype=np.int64)
    wraps[1:] = (thv[:-1] - thv[1:]) >= 4085
    loops_at = np.zeros(len(w), dtype=np.int64)
    loops_at[is_th] = np.cumsum(wraps)
    loops = np.where(thpos >= 0, loops_at[np.maximum(thpos, 0)], 0)
    inc = np.where(typ == 4, 12, np.where(typ == 5, 8, 0))
    cs = np.cumsum(inc) - inc
    basev, bpos = _fill(typ == 3, v & 0x7FF, idx)
    pol, _ = _fill(typ == 3, v >> 11, idx)
    base = basev + cs - np.where(bpos >= 0, cs[np.maximum(bpos, 0)], 0)
    mask = np.where(typ == 4, v, np.where(typ == 5, v & 0xFF, 0))
    pop = np.array([bin(m).count("1") for m in range(4096)], dtype=np.int64)
    nth = np.zeros((4096, 12), dtype=np.int64)
    for m in range(4096):
        bits = [i for i in range(12) if (m >> i) & 1]
        nth[m, :len(bits)] = bits
    cnt = np.where(typ == 2, 1, pop[mask]) * (thpos >= 0)
    src = np.repeat(idx, cnt)
    rank = np.arange(len(src)) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    single = typ[src] == 2
    xs = np.where(single, v[src] & 0x7FF, base[src] + nth[mask[src], rank]).astype(np.int16)
    ps = np.where(single, v[src] >> 11, pol[src]).astype(np.uint8)
    ts = (loops[src] << 24) + (th[src] << 12) + tl[src]
    return xs, y[src].astype(np.int16), ts, ps


def numpy_decode_evt2(words):
    w = words.astype(np.int64)
    typ = w >> 28
    idx = np.arange(len(w))
    th, thpos = _fill(typ == 8, w & 0x0FFFFFFF, idx)
    ev = (typ <= 1) & (thpos >= 0)
    return (((w >> 11) & 0x7FF)[ev].astype(np.int16), (w & 0x7FF)[ev].astype(np.int16),
            ((th << 6) | ((w >> 22) & 0x3F))[ev], typ[ev].astype(np.uint8))


def main():
    import torch
    import event_utils_amd as E
    from event_utils_amd import _device as D
    from event_utils_amd import _lib
    from event_utils_amd.data_formats import raw as RAW
    import simulate_time as ST
    quick = "--quick" in sys.argv
    h, w = (ST.H // 4, ST.W // 4) if quick else (ST.H, ST.W)
    reps = 5 if quick else 15
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "raw_decode_time.txt")
    target = ST.TARGET // 16 if quick else ST.TARGET

    def sync_ms(fn, reps=reps):
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    def event_ms(fn, reps=reps):
        fn()
        ts = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return float(np.median(ts))

    class Lines(list):
        def append(self, line):
            print(line, flush=True)
            list.append(self, line)

    unit = ST.scene(ST.F, h, w, 1.0)
    amplitude = target / 0.83 * ST.C_ON / float(np.abs(np.diff(unit, axis=0)).sum())
    fts = 1.0e6 + ST.DT * np.arange(ST.F)
    dev = D.require_gpu()
    xs, ys, ts, ps = E.simulate_events(torch.from_numpy(unit * amplitude).to(dev), fts, ST.C_ON, ST.C_OFF)
    x, y, p = xs.cpu().numpy(), ys.cpu().numpy(), (ps.cpu().numpy() > 0).astype(np.uint8)
    t = np.floor(ts.cpu().numpy()).astype(np.int64)
    del xs, ys, ts, ps
    order = np.lexsort((x, y, t))
    x, y, t, p = x[order].astype(np.int16), y[order].astype(np.int16), t[order], p[order]
    n = len(x)
    lines = Lines()
    lines.append("raw decoder timings: %d events at %dx%d over %.1f ms of stream (simulator scene, microsecond stamps, read-out order "
                 "inside a microsecond); median of %d; %s" % (n, w, h, (t[-1] - t[0]) / 1e3, reps, torch.cuda.get_device_name(0)))
    lines.append("conformance with vendor-written files is not verified: the decoding rules are the library's own statement of the formats")
    t0 = time.perf_counter()
    encodings = [("EVT3 vectorised", _lib.EVK_RAW_EVT3, E.encode_evt3(x, y, t, p, vectorize=True))]
    enc_s = time.perf_counter() - t0
    encodings.append(("EVT3 unvectorised", _lib.EVK_RAW_EVT3, E.encode_evt3(x, y, t, p, vectorize=False)))
    encodings.append(("EVT2", _lib.EVK_RAW_EVT2, E.encode_evt2(x, y, t, p)))
    lines.append("(host encode of the vectorised stream, numpy: %.2f s)" % enc_s)
    stream = D.stream()
    L = _lib.lib()
    for name, fmt, words in encodings:
        nbytes_w = words.nbytes
        lines.append("")
        lines.append("%s: %d words, %.3f words / event, %.3f bytes / event (decoded columns: 13)"
                     % (name, len(words), len(words) / n, nbytes_w / n))
        wt, nw = RAW._device_words(words, fmt, dev)
        sb = int(L.evk_raw_decode_scratch_bytes(nw))
        scratch = torch.empty(sb, dtype=torch.uint8, device=dev)
        report = torch.empty(16, dtype=torch.int64, device=dev)

        def plan():
            _lib.call("evk_raw_decode_plan", D.ptr(wt), nw, fmt, None, D.ptr(scratch), sb, D.ptr(report), D.ptr(report[8:]), stream)
        plan()
        count = int(report[0].item())
        assert count == n, (count, n)
        cols = [torch.empty(count, dtype=dt, device=dev) for dt in (torch.int16, torch.int16, torch.int64, torch.uint8)]

        def write(flags=0, kind=_lib.EVK_RAW_TS_US):
            _lib.call("evk_raw_decode_write", D.ptr(wt), nw, fmt, D.ptr(scratch), sb, D.ptr(report), *(D.ptr(c) for c in cols), kind,
                      h, w, flags, stream)
        for flags in (0, _lib.EVK_RAW_DIRECT_STORES):           # both forms give the events
            for c in cols:
                c.zero_()
            write(flags)
            assert all(np.array_equal(c.cpu().numpy(), r) for c, r in zip(cols, (x, y, t, p)))
        t_plan = event_ms(plan)
        t_staged = event_ms(lambda: write(0))
        t_direct = event_ms(lambda: write(_lib.EVK_RAW_DIRECT_STORES))
        moved = 2 * nbytes_w + 13 * n
        lines.append("  plan  (launch 1 summaries + launch 2 scan, HIP events)   %8.3f ms" % t_plan)
        lines.append("  write (launch 3, LDS staging, HIP events)                %8.3f ms" % t_staged)
        lines.append("  write (launch 3, direct stores, HIP events)              %8.3f ms" % t_direct)
        try:                                                   # the three kernels of one call, from the profiler
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                plan()
                write(0)
                torch.cuda.synchronize()
            ks = [(e.key, e.device_time_total if hasattr(e, "device_time_total") else e.cuda_time_total) for e in prof.key_averages()
                  if "k_raw_" in e.key]
            for key, us in sorted(ks):
                lines.append("    one call, %-44s %8.3f ms" % (key.split("(")[0][-44:], us / 1e3))
            if not ks:
                lines.append("    (the profiler reported no kernel of the call: no per-kernel split)")
        except Exception as e:      # noqa: BLE001
            lines.append("    (no per-kernel split: %s)" % (str(e).splitlines()[0] if str(e) else type(e).__name__))
        for label, tw in (("staged", t_staged), ("direct", t_direct)):
            lines.append("  plan + write (%s) %8.3f ms for 2 x %.1f + 13 x %.1f M = %.1f MB: %.1f %% of 8 TB/s"
                         % (label, t_plan + tw, nbytes_w / 1e6, n / 1e6, moved / 1e6, 100.0 * moved / ((t_plan + tw) * 1e-3) / PEAK))
        dec = E.decode_evt3 if fmt == _lib.EVK_RAW_EVT3 else E.decode_evt2
        lines.append("  %-57s %8.3f ms" % ("decode call, resident words (read-back, allocation)", sync_ms(lambda: dec(wt, sensor_size=(h, w)))))
        lines.append("  %-57s %8.3f ms" % ("decode call, host words (upload of %.1f MB included)" % (nbytes_w / 1e6),
                                            sync_ms(lambda: dec(words, sensor_size=(h, w)))))
        lines.append("  %-57s %8.3f ms" % ("decode call, host words, ts='seconds' (21 B / event out)",
                                            sync_ms(lambda: dec(words, sensor_size=(h, w), ts="seconds"))))
        del wt, scratch, cols
    lines.append("")
    lines.append("comparisons (not the code under test), same run:")
    host_cols = (x, y, t, p)
    lines.append("  %-57s %8.3f ms" % ("upload of the decoded columns (13 B / event, %.1f MB)" % (13 * n / 1e6),
                                        sync_ms(lambda: [torch.from_numpy(c).to(dev) for c in host_cols])))
    for name, fmt, words in encodings[::2]:
        fn = numpy_decode_evt3 if fmt == _lib.EVK_RAW_EVT3 else numpy_decode_evt2
        t0 = time.perf_counter()
        got = fn(words)
        dt = time.perf_counter() - t0
        assert all(np.array_equal(g, r) for g, r in zip(got, host_cols))
        lines.append("  %-57s %8.1f ms" % ("numpy host decode, %s (one run, one thread)" % name, dt * 1e3))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
