"""Event simulation on the device (evk_simulate.hip; definition: include/evk.h, "Event simulation", and DESIGN.md section 6): events
from log-intensity frames by the threshold-crossing model (ESIM, Rebecq et al., CoRL 2018; the noise-free core of v2e, Hu et al.
2021).  No reference module: upstream simulates nothing.  It is the forward model of which leaky_integrator(alpha=0) is the inverse,
and it keeps that module's conventions: frames (F, H, W) in the LOG domain (log_intensity), frame_ts F strictly increasing times,
numpy in -> numpy out, tensors in -> device tensors out.

Per pixel the log intensity is linear between consecutive frames.  Starting from the level `reference`, the pixel fires an ON event
each time the intensity has risen c_on above its level and an OFF event each time it has fallen c_off below it, the level follows
by that contrast, and the time of the event is interpolated between the two frame times.  An event closer than `refractory` to
the pixel's previous crossing is dropped (the level still moves).  All arithmetic is float64 with one rounding per operation: the
stream is defined bit for bit and repeats bit for bit."""
import collections

import numpy as np
import torch

from .. import _device as D
from .. import _lib
from .._checks import check_gain, check_image, check_time, check_times

SimulatorState = collections.namedtuple("SimulatorState", ["reference", "last_event_ts"])
SimulatorState.__doc__ = """The per-pixel state after a simulate_events call, two (H, W) float64 images: `reference`, the level each
pixel last fired at, and `last_event_ts`, the time of its last crossing (-inf: none yet).  Pass both to the next chunk."""

SORT_MAX = 2 ** 31 - 1                                 # the sort's item count is an int


def _image(v):
    return v if isinstance(v, torch.Tensor) else np.asarray(v)


def _contrast(c, shape, what):
    """-> (scalar, None) or (1.0, map): a scalar is checked here, a map's shape here and its values on the device."""
    c = _image(c)
    if c.ndim == 0:
        return check_gain(c, what, False), None
    return 1.0, check_image(c, shape, what)


def _simulate(frames, frame_ts, c_on, c_off, refractory, reference, last_event_ts, return_state, wide=0):
    # ---- everything that can be refused on the arguments alone
    frames = _image(frames)
    numpy_in = not isinstance(frames, torch.Tensor)
    if frames.ndim != 3 or frames.shape[0] < 2 or frames.shape[1] < 1 or frames.shape[2] < 1:
        raise ValueError("frames must have shape (F, H, W) with F >= 2 (got %r)" % (tuple(frames.shape),))
    if (frames.dtype.kind not in "biuf") if numpy_in else frames.is_complex():
        raise ValueError("frames must be real (got %s)" % frames.dtype)
    nf, h, w = (int(v) for v in frames.shape)
    if h * w > 0xFFFFFFFF:
        raise ValueError("%d x %d pixels are more than a 32-bit pixel index holds" % (h, w))
    fts = check_times(frame_ts, "frame_ts", True) + 0.0          # (+ 0.0: a frame time of -0.0 counts as +0.0)
    if len(fts) != nf:
        raise ValueError("frame_ts must hold one time per frame (%d frames, %d times)" % (nf, len(fts)))
    c_on, on_map = _contrast(c_on, (h, w), "c_on")
    c_off, off_map = _contrast(c_off, (h, w), "c_off")
    refractory = check_time(refractory, "refractory")
    if reference is not None:
        reference = check_image(_image(reference), (h, w), "reference")
    if last_event_ts is not None:
        last_event_ts = check_image(_image(last_event_ts), (h, w), "last_event_ts")
    t_first = float(fts[0])
    t_max = float(np.max(fts[:-1] + (fts[1:] - fts[:-1])))       # every event time lies in [t_first, t_max]
    # ---- the count pass, the scan and the one read-back
    dev = frames.device if (not numpy_in and frames.is_cuda) else D.require_gpu()
    dframes = D.resident(frames, dev, torch.float64)
    dfts = torch.from_numpy(np.ascontiguousarray(fts)).to(dev)
    don, doff, dref, dtl = (None if v is None else D.resident(v, dev, torch.float64) for v in (on_map, off_map, reference, last_event_ts))
    head = (D.ptr(dframes), D.ptr(dfts), nf, h, w, c_on, c_off, D.ptr(don), D.ptr(doff), refractory, D.ptr(dref), D.ptr(dtl))
    counts = torch.empty(h * w, dtype=torch.int32, device=dev)            # (uint32 values)
    report = torch.empty(2, dtype=torch.int64, device=dev)
    _lib.call("evk_simulate_count", *head, D.ptr(counts), D.ptr(report), D.stream())
    counts = counts.to(torch.int64) & 0xFFFFFFFF
    ends = torch.cumsum(counts, 0)
    total, overflows, bad = (int(v) for v in torch.cat((ends[-1:], report)).tolist())
    if bad:
        raise ValueError("c_on and c_off must be finite and > 0 (%d pixels of the maps are not)" % bad)
    if overflows:
        raise ValueError("%d pixel-intervals exceeded %d crossings between two frames: the contrast is too small for the frame change"
                         % (overflows, _lib.EVK_SIMULATE_MAX_STEPS))
    if total > SORT_MAX:
        raise ValueError("%d events are more than one call can order (at most %d): simulate fewer frames per call" % (total, SORT_MAX))
    # ---- the emit pass, the order by time
    is_wide = bool(wide) or h * w > 2 ** 31
    keys = torch.empty(total, dtype=torch.int64, device=dev)
    vals = torch.empty(total, dtype=torch.int64 if is_wide else torch.int32, device=dev)
    state = SimulatorState(torch.empty((h, w), dtype=torch.float64, device=dev), torch.empty((h, w), dtype=torch.float64, device=dev))
    _lib.call("evk_simulate_emit", *head, D.ptr(ends - counts), total, t_first, int(wide), D.ptr(keys), D.ptr(vals),
              D.ptr(state.reference), D.ptr(state.last_event_ts), D.stream())
    xs, ys, ps = (torch.empty(total, dtype=torch.int64, device=dev) for _ in range(3))
    ts = torch.empty(total, dtype=torch.float64, device=dev)
    if total:
        nbytes = int(_lib.lib().evk_simulate_sort_scratch_bytes(total, h, w, int(wide), t_first, t_max))
        if nbytes < 0:
            raise _lib.EvkError("evk_simulate_sort_scratch_bytes refused %d events" % total)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.call("evk_simulate_sort", D.ptr(keys), D.ptr(vals), total, h, w, int(wide), t_first, t_max, D.ptr(scratch), nbytes,
                  D.ptr(xs), D.ptr(ys), D.ptr(ts), D.ptr(ps), D.stream())
    out = (xs, ys, ts, ps)
    if numpy_in:
        out = tuple(v.cpu().numpy() for v in out)
        state = SimulatorState(*(v.cpu().numpy() for v in state))
    return out + (state,) if return_state else out


def simulate_events(frames, frame_ts, c_on=0.2, c_off=0.2, refractory=0.0, reference=None, last_event_ts=None, return_state=False):
    """Events (xs, ys, ts, ps) from log-intensity frames.  frames: (F, H, W), F >= 2, in the LOG domain (log_intensity), any real
    dtype, converted to float64 on the device; frame_ts: F strictly increasing finite times.  c_on, c_off: the contrasts, each a
    positive scalar or a per-pixel (H, W) map (threshold mismatch: draw the maps).  refractory >= 0, in the unit of frame_ts.
    reference: (H, W) start levels, default frames[0]; last_event_ts: (H, W) times of the pixels' last crossings, default -inf.

    Per pixel and frame interval, with the log intensity linear from L0 at T0 to L1 at T1: while R + c_on <= L1 (rising) the level
    R steps up by c_on, or while R - c_off >= L1 (falling) down by c_off; each crossing has t = T0 + clamp((R - L0) / (L1 - L0), 0,
    1) (T1 - T0) and is emitted as (x, y, t, +1 / -1) unless t is less than `refractory` after the pixel's previous crossing.  An
    interval whose frame difference is zero or not finite emits nothing.

    Returns xs, ys, ps as int64 and ts as float64 (ps = +1 / -1), ordered by t, equal times by the pixel index y * W + x, then in
    emission order; numpy arrays for numpy frames, device tensors for tensors.  No events: four empty columns.  With return_state
    a fifth value, SimulatorState(reference, last_event_ts), two (H, W) float64 images.
    Streaming: a video continues across calls when the next chunk gets frames[F - 1:] of the longer video (its first frame is this
    call's last), reference=state.reference and last_event_ts=state.last_event_ts; the chunks' events, concatenated, are the events of
    one call on the whole video.
    ValueError for F < 2, shapes that do not match, frame_ts that are not finite and strictly increasing, a contrast that is not
    positive and finite, a negative or NaN refractory -- and, after the count pass, for a pixel that would cross more than 65 536
    times between two frames (the contrast is too small for the frame change) or more than 2^31 - 1 events in all."""
    return _simulate(frames, frame_ts, c_on, c_off, refractory, reference, last_event_ts, return_state)
