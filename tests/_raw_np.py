"""The sequential restatement of the EVT3 / EVT2 decoding rules (include/evk.h): one plain Python loop over the words
and one `if` chain per format.  It is the oracle of the raw-stream tests and shares no code with the package or its encoder."""
import numpy as np

INITIAL = (0, 0, 0, 0, 0, 0, False)     # y, base_x, vect_pol, t_low, t_high, loops, have_time
STAT_NAMES = ("events", "triggers", "other", "before_time", "time_went_back", "out_of_range", "loops")


def _i16(v):
    v &= 0xFFFF
    return v - 0x10000 if v & 0x8000 else v


def _finish(xs, ys, ts, ps, counts, state, sensor_size):
    xs, ys = np.array(xs, dtype=np.int16), np.array(ys, dtype=np.int16)
    ts, ps = np.array(ts, dtype=np.int64), np.array(ps, dtype=np.uint8)
    if sensor_size is not None:
        h, w = sensor_size
        counts["out_of_range"] = int(np.count_nonzero((xs.view(np.uint16) >= w) | (ys.view(np.uint16) >= h)))
    counts["events"] = len(xs)
    return xs, ys, ts, ps, tuple(counts[k] for k in STAT_NAMES), state


def decode_evt3(words, state=None, sensor_size=None):
    """(xs int16, ys int16, ts int64 us, ps uint8, stats tuple in STAT_NAMES order, state tuple) of uint16 words"""
    y, base_x, vect_pol, t_low, t_high, loops, have_time = INITIAL if state is None else tuple(state)
    have_time = bool(have_time)
    loops_in = loops
    xs, ys, ts, ps = [], [], [], []
    c = dict.fromkeys(STAT_NAMES, 0)
    for w in np.asarray(words).astype(np.uint16).tolist():
        kind = w >> 12
        if kind == 0x0:
            y = w & 0x7FF
        elif kind == 0x2:
            if have_time:
                xs.append(w & 0x7FF); ys.append(y); ts.append((loops << 24) + (t_high << 12) + t_low); ps.append((w >> 11) & 1)
            else:
                c["before_time"] += 1
        elif kind == 0x3:
            base_x = w & 0x7FF
            vect_pol = (w >> 11) & 1
        elif kind in (0x4, 0x5):
            width = 12 if kind == 0x4 else 8
            for i in range(width):
                if (w >> i) & 1:
                    if have_time:
                        xs.append(_i16(base_x + i)); ys.append(y); ts.append((loops << 24) + (t_high << 12) + t_low); ps.append(vect_pol)
                    else:
                        c["before_time"] += 1
            base_x = (base_x + width) & 0xFFFF
        elif kind == 0x6:
            t_low = w & 0xFFF
        elif kind == 0x8:
            h = w & 0xFFF
            if have_time and t_high - h >= 4085:
                loops += 1
            elif have_time and t_high > h:
                c["time_went_back"] += 1
            t_high = h
            have_time = True
        elif kind == 0xA:
            c["triggers"] += 1
        else:
            c["other"] += 1
    c["loops"] = loops - loops_in
    return _finish(xs, ys, ts, ps, c, (y, base_x, vect_pol, t_low, t_high, loops, have_time), sensor_size)


def decode_evt2(words, state=None, sensor_size=None):
    """The same for uint32 EVT2 words; the state uses t_high and have_time only."""
    y, base_x, vect_pol, t_low, t_high, loops, have_time = INITIAL if state is None else tuple(state)
    have_time = bool(have_time)
    xs, ys, ts, ps = [], [], [], []
    c = dict.fromkeys(STAT_NAMES, 0)
    for w in np.asarray(words).astype(np.uint32).tolist():
        kind = w >> 28
        if kind == 0x8:
            t_high = w & 0x0FFFFFFF
            have_time = True
        elif kind in (0x0, 0x1):
            if have_time:
                xs.append((w >> 11) & 0x7FF); ys.append(w & 0x7FF); ts.append((t_high << 6) | ((w >> 22) & 0x3F)); ps.append(kind)
            else:
                c["before_time"] += 1
        elif kind == 0xA:
            c["triggers"] += 1
        else:
            c["other"] += 1
    return _finish(xs, ys, ts, ps, c, (y, base_x, vect_pol, t_low, t_high, loops, have_time), sensor_size)
