"""Differential fuzzing of the public voxel / event-image / get_iwe / objective calls against the CPU oracle (oracle/reference_np.py), beyond the
sizes and seeds of tests/: sensor sizes up to 1300 x 800, event counts around every boundary of the one-pass path (one wave,
one sub-chunk, the 'auto' thresholds, several sub-chunks per workgroup), scenes that cut hot tiles, polarities of every kind
(+-1, zeros, small integers, float32, huge, NaN / infinite), time stamps that are constant / few-valued / unsorted, every
EVK_IMPL.  The kinds filters, augment, datasets and motion do the same for the event filters (evk_select.hip), the event
augmentation (evk_augment.hip), the datasets' voxel windows and RobustNorm (evk_windows.hip) and the rotation / xyztheta
warps (evk_warps.hip), against the restatements the CPU suite checks against the reference (tests/test_cpu_filters.py,
tests/test_cpu_augment.py, tests/test_gpu_data_loaders.py, tests/_motion_models_np.py).  The kinds motion8 and zhu: the
angular-velocity / planar-flow warps (evk_warps.hip at up to 9 planes, evk_warp_models.h) against tests/_motion_models8_np.py
and the average-timestamp objective (evk_tsobj.hip: band and direct splat, post pass, adjoint gather) against
tests/_zhu_np.py; their cases are drawn by motion8_inputs / zhu_inputs without a GPU (tests/test_cpu_fuzz_inputs.py checks
what they cover); profiles/fuzz_motion8_zhu.txt.  The kinds denoise, tsurf, corners, planeflow and reconstruct: the five
feature sets on the per-pixel grouping (evk_group.h, evk_pred.h: evk_denoise.hip, evk_tsurf.hip, evk_corner.hip,
evk_planeflow.hip, evk_reconstruct.hip) against the fast_* / seq_reconstruct restatements of tests/_*_np.py, on one shared
event-stream generator (group_stream: degenerate sensors, h w around multiples of 64, hot pixels with runs exactly around
the wave thresholds, fractional / epoch / float32 / integer / unsorted time stamps, every column kind, select); rules those of
the dedicated GPU tests; profiles/fuzz_grouping_kinds.txt.  The kinds emvs and simulate: multi-view stereo (evk_emvs.hip) against
tests/_emvs_np.py and the event simulator (evk_simulate.hip) against tests/_simulate_np.py, both bit for bit: non-finite and
exactly representable coordinates on the rounding ties, packet sizes crossed with forced chunk counts, duplicated planes and planes
behind the camera, hand-built raw volumes; epoch-scale, neighbouring, 64-bit-apart and subnormal frame times, overflowing and
non-finite pixels, per-pixel contrasts crossed with state, refractory and the wide sort values, streaming splits with ties on the
split time; profiles/fuzz_emvs_simulate.txt.  The kinds flowts, flowcm and segment: the kernels that return gradients --
the average-timestamp and the contrast loss of a dense flow field (evk_flowloss.hip) against tests/_flow_loss_np.py and
tests/_flow_contrast_np.py, and motion segmentation (evk_segment.hip) against tests/_segmentation_np.py, by the rules and
tolerances of their dedicated GPU tests: fields from (2, 2), events beside the field's support and far outside, empty samples at
every place of a batch, every kind of offsets, time spans from 1e-6 s to 100 s, tied and equal stamps, real weights, one NaN,
blurs wider than the canvas; canvases of one band, of bands of two and three rows, of none (the direct kernel), several chunks,
rows of the associations off 16-byte alignment, zero rows; and bit for bit a second call, every form of input, a batch against
its samples, 'both' against its directions, autograd against the explicit calls, the band against the direct splat;
profiles/fuzz_flow_segment.txt.  The kind raw: the EVT3 / EVT2 decoder (evk_rawdecode.hip) against the sequential restatement
of tests/_raw_np.py, bit for bit, through the staged write and through EVK_RAW_DIRECT_STORES: structured and uniformly random words,
streams of TIME_HIGH words on the loop threshold, a first TIME_HIGH anywhere or nowhere, vector runs longer than a chunk whose base_x
wraps 2^16, word counts from 0 over partial lanes and wave rows to more chunks than the scan has lanes, every form of input (slices
on an odd half word among them), up to five cuts with the state carried (empty pieces, pieces shorter than a lane, cuts inside loops
and vector runs), seconds, sensor sizes and the three out-of-range policies, drawn initial states, iter_decode_raw / decode_raw on an
in-memory file, and the encoders' round trip; profiles/fuzz_raw.txt.
Test infrastructure (imports the oracle): not part of the product.
usage: python tools/fuzz_parity.py [--seconds S] [--seed0 K]
       [--kinds voxel,image,native,iwe,objective,windows,misc,errors,prims,search,filters,augment,datasets,motion,motion8,zhu,
               denoise,tsurf,corners,planeflow,reconstruct,emvs,simulate,flowts,flowcm,segment,raw]
       exit code 1 on any mismatch"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import event_utils_amd as E  # noqa: E402
from event_utils_amd import tiled  # noqa: E402
from oracle import reference_np as R  # noqa: E402

N_CHOICES = [1, 2, 63, 64, 65, 1000, 8191, 8192, 8193, 12_289, 79_999, 80_001, 149_999, 150_001, 319_999, 320_001, 1_000_003, 2_500_000]


def arg(name, default):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


def coords(rng, n, H, W, real, scene):
    if real:
        x = rng.uniform(0, W - 1, n); y = rng.uniform(0, H - 1, n)
    else:
        x = rng.integers(0, W, n).astype(np.float64); y = rng.integers(0, H, n).astype(np.float64)
    if scene == "blob" and n > 8:
        hot = rng.random(n) < 0.7
        x[hot] = np.clip(W // 2 + rng.integers(-2, 3, hot.sum()), 0, W - 1); y[hot] = np.clip(H // 3 + rng.integers(-2, 3, hot.sum()), 0, H - 1)
    elif scene == "pixel" and n > 8:
        hot = rng.random(n) < 0.9
        x[hot] = W - 1; y[hot] = H - 1
    elif scene == "edge" and n > 8:
        hot = rng.random(n) < 0.8
        x[hot] = np.clip(W * 0.37 + rng.normal(0, 0.6, hot.sum()), 0, W - 1)
        if not real:
            x = np.floor(x)
    return x.astype(np.float32), y.astype(np.float32)


def weights(rng, n, kind):
    if kind == "pm1":
        return (rng.integers(0, 2, n) * 2 - 1).astype(np.float32)
    if kind == "pm1z":
        return rng.integers(-1, 2, n).astype(np.float32)
    if kind == "ones":
        return np.ones(n, np.float32)
    if kind == "ints":
        return rng.integers(-3, 4, n).astype(np.float32)
    if kind == "float":
        return rng.normal(size=n).astype(np.float32)
    if kind == "huge":
        return (rng.normal(size=n) * 1e30).astype(np.float32)
    p = (rng.integers(0, 2, n) * 2 - 1).astype(np.float32)        # "special": a few NaN / inf / -0 among unit polarities
    if n > 4:
        idx = rng.integers(0, n, 4)
        p[idx] = [np.nan, np.inf, -np.inf, -0.0]
    return p


def times(rng, n, kind):
    if kind == "sorted":
        return np.sort(rng.uniform(3.0, 3.2, n)).astype(np.float32)
    if kind == "const":
        return np.full(n, 1.5, np.float32)
    if kind == "few":
        return np.sort(rng.integers(0, 4, n)).astype(np.float32)
    if kind == "ends":          # everything at the two ends: t_norm exactly 0 or B - 1
        t = np.zeros(n, np.float32); t[n // 2:] = 1.0
        return t
    t = rng.uniform(0.0, 1.0, n).astype(np.float32)           # "unsorted": ts[0], ts[-1] are whatever they are (Q9)
    return t


def device_cols(rng, arrays):
    """The arrays as device tensors -- usually freshly allocated (16-byte aligned), in a third of the cases as SLICES that start
    1-3 elements into a larger buffer, per column, with readable storage behind them or (one case in four of those) ending with
    their storage: the one-pass paths read the former where they lie and copy the latter (tiled.column_ok)."""
    if rng.random() > 0.33:
        return [torch.from_numpy(a).cuda() for a in arrays]
    out = []
    for a in arrays:
        off = int(rng.integers(0, 4))
        tail = 0 if rng.random() < 0.25 else int(rng.integers(3, 9))
        buf = torch.empty(off + len(a) + tail, dtype=torch.from_numpy(a[:1]).dtype if len(a) else torch.float32, device="cuda")
        buf[off:off + len(a)] = torch.from_numpy(a).cuda()
        out.append(buf[off:off + len(a)])
    return out


def same(got, ref, mag, what, magf=4e-7):
    """float32 accumulation against the float64 oracle: 1e-5 of the reference's maximum + the float32 rounding of the summed
    magnitudes (cancelling sums); NaN / infinite cells in the same places."""
    got = np.asarray(got, np.float64); ref = np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return "%s: shape %s vs %s" % (what, got.shape, ref.shape)
    bad_g, bad_r = ~np.isfinite(got), ~np.isfinite(ref)
    if not np.array_equal(bad_g, bad_r):
        return "%s: non-finite cells differ (%d vs %d)" % (what, bad_g.sum(), bad_r.sum())
    if bad_r.any() and not (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[bad_r & ~np.isnan(ref)], ref[bad_r & ~np.isnan(ref)])):
        return "%s: NaN / infinity pattern differs" % what
    ok = ~bad_r
    if not ok.any():
        return None
    fin = np.abs(ref[ok])
    tol = 1e-5 * max(fin.max(), 1e-30) + magf * float(np.max(np.abs(mag)[ok])) if mag is not None else 1e-5 * max(fin.max(), 1e-30)
    err = np.max(np.abs(got[ok] - ref[ok]))
    return None if err <= tol else "%s: max error %.3e > %.3e (max |ref| %.3e)" % (what, err, tol, fin.max())


def case_voxel(rng):
    H, W = int(rng.integers(2, 800)), int(rng.integers(2, 1300))
    if rng.random() < 0.3:
        H, W = [(180, 240), (260, 346), (480, 640), (720, 1280)][int(rng.integers(0, 4))]
    B = int(rng.integers(1, 12))
    n = int(rng.choice(N_CHOICES))
    real = bool(rng.integers(0, 2))
    scene = str(rng.choice(["uniform", "uniform", "blob", "pixel", "edge"]))
    pk = str(rng.choice(["pm1", "pm1", "pm1z", "ones", "ints", "float", "huge", "special"]))
    tk = str(rng.choice(["sorted", "sorted", "sorted", "const", "few", "ends", "unsorted"]))
    impl = str(rng.choice(["auto", "tiled", "tiled", "direct"]))
    det = bool(rng.random() < 0.25)
    rec = [None, None, 4, 8][int(rng.integers(0, 4))] if impl == "tiled" else None
    if det and impl == "direct":      # a contradiction the call refuses (ValueError)
        impl = "auto"
    desc = "voxel %dx%dx%d n=%d real=%d %s p=%s t=%s impl=%s det=%d rec=%s" % (B, H, W, n, real, scene, pk, tk, impl, det, rec)
    x, y = coords(rng, n, H, W, real, scene)
    p, t = weights(rng, n, pk), times(rng, n, tk)
    with np.errstate(all="ignore"):
        ref = R.events_to_voxel_torch(x, y, t, p, B, sensor_size=(H, W), accum="f64")
        fin = np.where(np.isfinite(p), np.abs(p), 0).astype(np.float32)
        mag = R.events_to_voxel_torch(x, y, t, fin, B, sensor_size=(H, W), accum="f64")
    os.environ["EVK_IMPL"] = impl
    if det:
        os.environ["EVK_VOXEL_DETERMINISTIC"] = "1"
    tiled.FORCE["rec"] = rec
    try:
        cols = device_cols(rng, (x, y, t, p))
        got = E.events_to_voxel_torch(*cols, B, sensor_size=(H, W)).cpu().numpy()
        if det and pk in ("huge", "special"):   # not representable in the fixed-point cells: refused (documented), not compared
            return desc, None
    except Exception as e:  # noqa: BLE001
        if det and pk in ("huge", "special"):
            return desc, None
        return desc, "raised %s: %s" % (type(e).__name__, e)
    finally:
        os.environ.pop("EVK_IMPL", None); os.environ.pop("EVK_VOXEL_DETERMINISTIC", None)
        tiled.FORCE["rec"] = None
    if not np.isfinite(mag).all():
        mag = np.where(np.isfinite(mag), mag, 0.0)
    # the direct kernels add float32 atomics as the reference's index_put_ does: on a pixel that collects 10^5 events their own
    # rounding reaches 10^-4 of the cell (the one-pass path accumulates float64 / integers)
    direct_like = impl == "direct" or (impl == "auto" and n < tiled.TILED_MIN_EVENTS and not det)
    # (a small call on columns that cannot be read in place -- no slack behind a misaligned slice -- keeps the direct kernel too)
    direct_like = direct_like or (impl == "auto" and not det and n * 2 < tiled.REALIGN_ATOMICS and not all(tiled.column_ok(c) for c in cols))
    return desc, same(got, ref, mag, "grid", 1e-3 if direct_like and scene in ("pixel", "blob", "edge") else 4e-7)


def case_image(rng):
    H, W = int(rng.integers(2, 800)), int(rng.integers(2, 1300))
    if rng.random() < 0.3:
        H, W = [(180, 240), (260, 346), (480, 640), (720, 1280)][int(rng.integers(0, 4))]
    n = int(rng.choice(N_CHOICES))
    interp = [None, "bilinear"][int(rng.integers(0, 2))]
    padding = bool(rng.integers(0, 2))
    clip = bool(rng.integers(0, 2)) or interp == "bilinear"
    default = float(rng.choice([0.0, 0.0, 0.5]))
    real = bool(rng.integers(0, 2))
    scene = str(rng.choice(["uniform", "uniform", "blob", "pixel", "edge"]))
    pk = str(rng.choice(["pm1", "pm1", "pm1z", "ones", "ints", "float", "huge", "special"]))
    impl = str(rng.choice(["auto", "tiled", "tiled", "direct"]))
    desc = "image %dx%d n=%d %s pad=%d clip=%d default=%g real=%d %s p=%s impl=%s" % (H, W, n, interp, padding, clip, default, real, scene, pk, impl)
    x, y = coords(rng, n, H, W, real, scene)
    if clip and n > 16:            # beyond the sensor: clipped events (Q8: they pile up at (0, 0) in the nearest branch)
        k = rng.integers(0, n, max(1, n // 50))
        x[k] += np.float32(W); y[k[: len(k) // 2]] += np.float32(H)
    elif not clip and real:
        x = np.minimum(x, np.float32(W - 1.001)); y = np.minimum(y, np.float32(H - 1.001))
        x = np.maximum(x, 0); y = np.maximum(y, 0)
    p = weights(rng, n, pk)
    xa, ya = (x, y) if real else (x.astype(np.int64), y.astype(np.int64))
    with np.errstate(all="ignore"):
        ref = R.events_to_image_torch(xa, ya, p, sensor_size=(H, W), clip_out_of_range=clip, interpolation=interp,
                                      padding=padding, default=default, accum="f64")
        fin = np.where(np.isfinite(p), np.abs(p), 0).astype(np.float32)
        mag = R.events_to_image_torch(xa, ya, fin, sensor_size=(H, W), clip_out_of_range=clip, interpolation=interp,
                                      padding=padding, default=abs(default), accum="f64")
    os.environ["EVK_IMPL"] = impl
    try:
        got = E.events_to_image_torch(*device_cols(rng, (xa, ya, p)),
                                      sensor_size=(H, W), clip_out_of_range=clip, interpolation=interp, padding=padding,
                                      default=default).cpu().numpy()
    except Exception as e:  # noqa: BLE001
        return desc, "raised %s: %s" % (type(e).__name__, e)
    finally:
        os.environ.pop("EVK_IMPL", None)
    err = same(got, ref, mag, "image")
    if err is None and rng.random() < 0.5:
        # numpy entry point (image.py:5-44): integer coordinates on the (H+1, W+1) canvas, bit-exact
        xi, yi = rng.integers(0, W + 1, n), rng.integers(0, H + 1, n)
        pi = rng.integers(-3, 4, n) if rng.random() < 0.5 else np.ones(n, np.int64)
        mv = bool(rng.integers(0, 2))
        os.environ["EVK_IMPL"] = impl
        try:
            a = E.events_to_image(xi, yi, pi, sensor_size=(H, W), meanval=mv, default=default)
        finally:
            os.environ.pop("EVK_IMPL", None)
        with np.errstate(all="ignore"):
            b = R.events_to_image(xi, yi, pi, sensor_size=(H, W), meanval=mv, default=default)
        if not (a.dtype == b.dtype and np.array_equal(a, b, equal_nan=True)):
            err = "events_to_image (meanval=%d): not bit-exact, %d cells differ" % (mv, int((a != b).sum()))
    return desc, err


def case_native(rng):
    """events in the on-disk dtypes (int16 coordinates, uint8 / bool polarities, float32 time stamps) through the public call"""
    H, W = [(180, 240), (260, 346), (480, 640), (720, 1280)][int(rng.integers(0, 4))]
    B = int(rng.integers(1, 10))
    n = int(rng.choice(N_CHOICES))
    scene = str(rng.choice(["uniform", "blob", "edge"]))
    impl = str(rng.choice(["auto", "tiled", "direct"]))
    desc = "native %dx%dx%d n=%d %s impl=%s" % (B, H, W, n, scene, impl)
    x, y = coords(rng, n, H, W, False, scene)
    t = times(rng, n, "sorted")
    p8 = rng.integers(0, 2, n).astype(np.uint8)
    with np.errstate(all="ignore"):
        ref = R.events_to_voxel_torch(x, y, t, p8.astype(np.float32), B, sensor_size=(H, W), accum="f64")
    os.environ["EVK_IMPL"] = impl
    try:
        got = E.events_to_voxel_torch(torch.from_numpy(x.astype(np.int16)).cuda(), torch.from_numpy(y.astype(np.int16)).cuda(),
                                      torch.from_numpy(t).cuda(), torch.from_numpy(p8).cuda(), B, sensor_size=(H, W)).cpu().numpy()
    except Exception as e:  # noqa: BLE001
        return desc, "raised %s: %s" % (type(e).__name__, e)
    finally:
        os.environ.pop("EVK_IMPL", None)
    return desc, same(got, ref, None, "grid")


def case_windows(rng):
    """voxel_grids_fixed_n_torch / voxel_grids_fixed_t_torch / events_to_voxel_timesync_torch / events_to_neg_pos_voxel_torch
    (voxel_grid.py:37-112,155-182): the reference loops events_to_voxel_torch over slices; so does the check"""
    H, W = int(rng.integers(2, 300)), int(rng.integers(2, 400))
    B = int(rng.integers(1, 8))
    n = int(rng.choice([65, 1000, 8193, 100_000, 400_000, 1_000_003]))
    which = str(rng.choice(["fixed_n", "fixed_t", "timesync", "neg_pos"]))
    scene = str(rng.choice(["uniform", "blob", "edge"]))
    impl = str(rng.choice(["auto", "tiled", "direct"]))
    x, y = coords(rng, n, H, W, bool(rng.integers(0, 2)), scene)
    t = times(rng, n, "sorted")
    p = weights(rng, n, str(rng.choice(["pm1", "pm1z", "float"])))
    desc = "windows %s %dx%dx%d n=%d %s impl=%s" % (which, B, H, W, n, scene, impl)
    tt = [torch.from_numpy(a).cuda() for a in (x, y, t, p)]
    os.environ["EVK_IMPL"] = impl
    try:
        with np.errstate(all="ignore"):
            if which == "fixed_n":
                k = int(rng.choice([max(2, n // 7), max(2, n // 3), n, 33 if n <= 1000 else max(2, n // 11)]))
                got = E.voxel_grids_fixed_n_torch(*tt, B, k, sensor_size=(H, W))
                ref = [R.events_to_voxel_torch(x[i:i + k], y[i:i + k], t[i:i + k], p[i:i + k], B, sensor_size=(H, W), accum="f64")
                       for i in range(0, n - k, k)]
                desc += " k=%d" % k
            elif which == "fixed_t":
                span = float(t[-1] - t[0])
                dt = span / float(rng.choice([1.5, 3.0, 7.3]))
                got = E.voxel_grids_fixed_t_torch(*tt, B, dt, sensor_size=(H, W))
                ref = []
                for ts0 in np.arange(t[0].item(), t[-1].item() - dt, dt):
                    a, b = np.searchsorted(t, ts0), np.searchsorted(t, ts0 + dt)
                    ref.append(R.events_to_voxel_torch(x[a:b], y[a:b], t[a:b], p[a:b], B, sensor_size=(H, W), accum="f64"))
            elif which == "timesync":
                t0 = float(t[0]) + 0.2 * float(t[-1] - t[0]); t1 = float(t[0]) + 0.7 * float(t[-1] - t[0])
                got = [E.events_to_voxel_timesync_torch(*tt, B, t0, t1, sensor_size=(H, W))]
                a, b = np.searchsorted(t, t0), np.searchsorted(t, t1)
                ref = [R.events_to_voxel_torch(x[a:b], y[a:b], t[a:b], p[a:b], B, sensor_size=(H, W), accum="f64")]
            else:
                got = list(E.events_to_neg_pos_voxel_torch(*tt, B, sensor_size=(H, W)))
                ref = [R.events_to_voxel_torch(x, y, t, np.where(p > 0, 1, 0).astype(np.float32), B, sensor_size=(H, W), accum="f64"),
                       R.events_to_voxel_torch(x, y, t, np.where(p <= 0, 1, 0).astype(np.float32), B, sensor_size=(H, W), accum="f64")]
    except Exception as e:  # noqa: BLE001
        return desc, "raised %s: %s" % (type(e).__name__, e)
    finally:
        os.environ.pop("EVK_IMPL", None)
    if len(got) != len(ref):
        return desc, "%d grids vs %d" % (len(got), len(ref))
    for k, (a, b) in enumerate(zip(got, ref)):
        hot = scene in ("blob", "edge")
        err = same(a.cpu().numpy(), b, np.abs(b) if hot else None, "grid %d" % k, 1e-3)   # windows / small calls: float32 atomics
        if err is not None:
            return desc, err
    return desc, None


def case_errors(rng):
    """coordinates beyond the sensor: index_put_ wraps -size <= index < 0 and raises IndexError outside (image.py:93-99 re-raises
    it); the oracle decides which, the call must do the same -- for every EVK_IMPL, synchronous and deferred reporting"""
    H, W = int(rng.integers(4, 500)), int(rng.integers(4, 700))
    n = int(rng.choice([3, 65, 1000, 8193, 100_000, 400_000, 1_000_003]))
    which = str(rng.choice(["voxel", "nearest", "bilinear"]))
    impl = str(rng.choice(["auto", "tiled", "direct"]))
    how = str(rng.choice(["neg_wrap", "neg_far", "beyond", "edge", "frac_neg"]))
    errs = str(rng.choice(["strict", "deferred"]))
    clip = bool(rng.integers(0, 2)) or which == "bilinear"
    pad = bool(rng.integers(0, 2))
    desc = "errors %s %dx%d n=%d impl=%s %s clip=%d pad=%d EVK_ERRORS=%s" % (which, H, W, n, impl, how, clip, pad, errs)
    x = rng.integers(0, W, n).astype(np.float32); y = rng.integers(0, H, n).astype(np.float32)
    if which == "bilinear":
        x = np.minimum(x + rng.random(n).astype(np.float32), np.float32(W - 1)); y = np.minimum(y + rng.random(n).astype(np.float32), np.float32(H - 1))
    k = rng.integers(0, n, min(n, 3))
    if how == "neg_wrap":
        x[k] = -float(rng.integers(1, W)); y[k[:1]] = -float(rng.integers(1, H))
    elif how == "neg_far":
        x[k[:1]] = -float(W + 1 + rng.integers(0, 50))
    elif how == "beyond":
        if rng.random() < 0.5:
            x[k[:1]] = float(W + rng.integers(0, 3))
        else:
            y[k[:1]] = float(H + rng.integers(0, 3))
    elif how == "edge":
        x[k] = float(W - 1); y[k] = float(H - 1)
    else:
        x[k] = -0.5; y[k[:1]] = -0.25          # truncation toward zero (nearest) vs floor (bilinear)
    t = np.sort(rng.uniform(0, 1, n)).astype(np.float32)
    p = weights(rng, n, str(rng.choice(["pm1", "float"])))
    B = int(rng.integers(1, 6))
    ref, ref_exc = None, None
    try:
        with np.errstate(all="ignore"):
            if which == "voxel":
                ref = R.events_to_voxel_torch(x, y, t, p, B, sensor_size=(H, W), accum="f64")
            else:
                ref = R.events_to_image_torch(x, y, p, sensor_size=(H, W), clip_out_of_range=clip,
                                              interpolation=None if which == "nearest" else "bilinear", padding=pad, accum="f64")
    except IndexError as e:
        ref_exc = e
    os.environ["EVK_IMPL"] = impl
    os.environ["EVK_ERRORS"] = errs
    got, exc = None, None
    try:
        c = [torch.from_numpy(a).cuda() for a in (x, y, t, p)]
        if which == "voxel":
            got = E.events_to_voxel_torch(*c, B, sensor_size=(H, W))
        else:
            got = E.events_to_image_torch(c[0], c[1], c[3], sensor_size=(H, W), clip_out_of_range=clip,
                                          interpolation=None if which == "nearest" else "bilinear", padding=pad)
        E.check_errors()           # deferred reports surface here at the latest
        got = got.cpu().numpy()
    except IndexError as e:
        exc = e
    except Exception as e:  # noqa: BLE001
        return desc, "raised %s: %s" % (type(e).__name__, e)
    finally:
        os.environ.pop("EVK_IMPL", None); os.environ.pop("EVK_ERRORS", None)
        try:
            E.check_errors()
        except Exception:  # noqa: BLE001
            pass
    if (ref_exc is None) != (exc is None):
        return desc, "reference %s, here %s" % ("raises IndexError" if ref_exc else "returns", "raises IndexError" if exc else "returns")
    if ref_exc is not None:
        return desc, None
    mag = None
    if which != "voxel":       # clipped events pile up at (0, 0) with their weights (Q8): float32 atomics in the direct kernels
        with np.errstate(all="ignore"):
            mag = R.events_to_image_torch(x, y, np.abs(p), sensor_size=(H, W), clip_out_of_range=clip,
                                          interpolation=None if which == "nearest" else "bilinear", padding=pad, accum="f64")
    return desc, same(got, ref, mag, which, 1e-4)


def case_prims(rng):
    """the building blocks: linvel_warp.warp and events_bounds_mask (bit-exact, float64), events_to_image_drv with arbitrary
    Jacobians, interpolate_to_image / interpolate_to_derivative_img, the dense-flow warp, the Gaussian blur (bit-identical to
    scipy's: oracle gaussian_filter_reflect is pinned to it by fixture f10)"""
    from event_utils_amd.contrast_max.objectives import gaussian_filter_device
    from event_utils_amd.transforms.optic_flow import warp_events_flow_torch
    which = str(rng.choice(["warp", "drv", "splat", "flow", "blur"]))
    H, W = int(rng.integers(4, 300)), int(rng.integers(4, 400))
    n = int(rng.choice([1, 65, 1000, 8193, 100_000, 400_000]))
    desc = "prims %s %dx%d n=%d" % (which, H, W, n)
    try:
        with np.errstate(all="ignore"):
            if which == "warp":
                x = rng.uniform(-5, W + 5, n); y = rng.uniform(-5, H + 5, n); t = np.sort(rng.uniform(0, 10 ** float(rng.integers(-3, 10)), n))
                prm = rng.normal(0, 1, 2) * float(rng.choice([0.0, 1e-3, 50.0, 1e4]))
                t0 = float(t[-1]) if rng.random() < 0.7 else float(rng.uniform(t[0], t[-1]))
                got = E.linvel_warp().warp(x, y, t, np.ones(n), t0, prm, compute_grad=True)
                ref = R.linvel_warp().warp(x, y, t, np.ones(n), t0, prm, compute_grad=True)
                for a, b, nm in zip(got, ref, ("x'", "y'", "jx", "jy")):
                    if not (np.asarray(a).dtype == np.float64 and np.array_equal(a, b)):
                        return desc, "%s not bit-exact" % nm
                lim = (0, W, 0, H) if rng.random() < 0.5 else (float(rng.uniform(-3, 3)), float(rng.uniform(3, W + 3)), float(rng.uniform(-3, 3)), float(rng.uniform(3, H + 3)))
                if not np.array_equal(E.events_bounds_mask(got[0], got[1], *lim), R.events_bounds_mask(ref[0], ref[1], *lim)):
                    return desc, "bounds mask differs"
                return desc, None
            if which == "drv":
                x = rng.uniform(-1, W + 2, n); y = rng.uniform(-1, H + 2, n)
                x, y = np.maximum(x, 0), np.maximum(y, 0)           # (negative pixels wrap or raise: the errors kind)
                p = rng.normal(size=n); jx = rng.normal(size=(2, n)); jy = rng.normal(size=(2, n))
                grad = bool(rng.integers(0, 2))
                gi, gd = E.events_to_image_drv(x, y, p, jx, jy, sensor_size=(H, W), compute_gradient=grad)
                ri, rd = R.events_to_image_drv(x, y, p, jx, jy, sensor_size=(H, W), compute_gradient=grad, accum="f64")
                mi, md = R.events_to_image_drv(x, y, np.abs(p), np.abs(jx), np.abs(jy), sensor_size=(H, W), compute_gradient=grad, accum="f64")
                err = same(gi, ri, mi, "iwe", 1e-6)
                if err is None and grad:
                    err = same(gd, rd, None, "d_iwe") if gd is not None else "d_iwe is None"
                return desc, err
            if which == "splat":
                px = rng.integers(0, W - 1, n); py = rng.integers(0, H - 1, n)
                dx = rng.random(n).astype(np.float32); dy = rng.random(n).astype(np.float32)
                kind = str(rng.choice(["random", "coords", "mixed"]))
                if kind != "random":      # pixels and fractions taken from float32 coordinates (what upstream's callers pass): records
                    xc, yc = coords(rng, n, H, W, True, str(rng.choice(["uniform", "blob", "pixel", "edge"])))
                    take = np.ones(n, bool) if kind == "coords" else rng.random(n) < 0.7
                    px = np.where(take, np.floor(xc).astype(np.int64), px); py = np.where(take, np.floor(yc).astype(np.int64), py)
                    dx = np.where(take, xc - np.floor(xc), dx).astype(np.float32); dy = np.where(take, yc - np.floor(yc), dy).astype(np.float32)
                    px = np.minimum(px, W - 2); py = np.minimum(py, H - 2)
                if n > 64 and rng.random() < 0.5:
                    px[:16] = -1; py[16:32] = -1                  # wrap once, as index_put_ does
                w = rng.normal(size=n).astype(np.float32) if rng.random() < 0.5 else weights(rng, n, str(rng.choice(["pm1", "pm1z", "ints"])))
                os.environ["EVK_IMPL"] = str(rng.choice(["auto", "tiled", "direct"]))
                desc += " %s impl=%s" % (kind, os.environ["EVK_IMPL"])
                w1 = rng.normal(size=(2, n)).astype(np.float32); w2 = rng.normal(size=(2, n)).astype(np.float32)
                ref = R.interpolate_to_image(px, py, dx, dy, w, np.zeros((H, W), np.float32), accum="f64")
                img = torch.zeros(H, W, device="cuda")
                E.interpolate_to_image(*(torch.from_numpy(a).cuda() for a in (px, py, dx, dy, w)), img)
                err = same(img.cpu().numpy(), ref, R.interpolate_to_image(px, py, dx, dy, np.abs(w), np.zeros((H, W), np.float32), accum="f64"), "splat", 1e-6)
                if err is not None:
                    return desc, err
                refd = R.interpolate_to_derivative_img(px, py, dx, dy, np.zeros((2, H, W), np.float32), w1, w2, accum="f64")
                dimg = torch.zeros(2, H, W, device="cuda")
                E.interpolate_to_derivative_img(*(torch.from_numpy(a).cuda() for a in (px, py, dx, dy)), dimg, torch.from_numpy(w1).cuda(), torch.from_numpy(w2).cuda())
                magd = R.interpolate_to_derivative_img(px, py, dx, dy, np.zeros((2, H, W), np.float32), np.abs(w1), np.abs(w2), accum="f64")
                return desc, same(dimg.cpu().numpy(), refd, np.full(refd.shape, np.max(np.abs(magd)) * 4 + 1.0), "derivative splat", 1e-6)
            if which == "flow":
                n = max(n, 2)           # (the oracle squeezes its inputs as upstream does: one event is a 0-d array there)
                x = rng.uniform(-2, W + 1, n).astype(np.float32); y = rng.uniform(-2, H + 1, n).astype(np.float32)
                t = np.sort(rng.uniform(0, 0.1, n)).astype(np.float32)
                flow = (rng.normal(size=(2, H, W)) * 30).astype(np.float32)
                t0 = None if rng.random() < 0.5 else float(rng.uniform(0, 0.1))
                gx, gy = warp_events_flow_torch(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), torch.from_numpy(t).cuda(), None,
                                                torch.from_numpy(flow).cuda(), t0=t0)
                rx, ry = R.warp_events_flow_torch(x, y, t, None, flow, t0=t0)
                for a, b, nm in ((gx, rx, "x"), (gy, ry, "y")):
                    err = same(a.cpu().numpy(), b, None, "warped " + nm)
                    if err is not None:
                        return desc, err
                return desc, None
            sigma = float(rng.choice([0.5, 1.0, 2.0, 3.3]))
            a = rng.normal(size=(2, H, W) if rng.random() < 0.5 else (H, W)).astype(np.float32)
            got = gaussian_filter_device(torch.from_numpy(a).cuda(), sigma).cpu().numpy()
            ref = R.gaussian_filter_reflect(a, sigma)
            return desc + " sigma=%g" % sigma, None if np.array_equal(got, ref) else "blur not bit-identical (max %.3e)" % np.max(np.abs(got - ref))
    except Exception as e:  # noqa: BLE001
        return desc, "raised %s: %s" % (type(e).__name__, e)
    finally:
        os.environ.pop("EVK_IMPL", None)


def case_search(rng):
    """grid_search_initial (every sample and the best one) and the objective landscape.  (The optimisers are not fuzzed: BFGS on
    forward differences over a rugged landscape amplifies a 1e-7 difference of the objective into another local optimum -- on the
    oracle and on the HIP path alike; their parity is the golden trace f9 and tests/test_gpu_parity.py::test_f9_*.)"""
    from event_utils_amd.contrast_max import events_cmax as C
    which = str(rng.choice(["grid", "landscape"]))
    H, W = int(rng.integers(60, 200)), int(rng.integers(80, 260))
    n = int(rng.choice([20_000, 60_000, 200_000]))
    v = rng.uniform(-60, 60, 2)
    desc = "search %s %dx%d n=%d true flow (%.1f, %.1f)" % (which, H, W, n, v[0], v[1])
    # edges moving at v: events at x = x_edge + v t (vertical lines) and y = y_edge + v t (horizontal lines), a little noise
    t = np.sort(rng.uniform(0, 0.1, n)).astype(np.float32).astype(np.float64)
    vert = rng.random(n) < 0.5
    ex, ey = rng.choice(np.linspace(0.25, 0.75, 4) * W, n), rng.choice(np.linspace(0.25, 0.75, 3) * H, n)
    x = np.where(vert, ex, rng.uniform(0.15 * W, 0.85 * W, n)) + v[0] * t + rng.normal(0, 0.3, n)
    y = np.where(vert, rng.uniform(0.15 * H, 0.85 * H, n), ey) + v[1] * t + rng.normal(0, 0.3, n)
    x, y = (np.clip(a, 1, lim - 2).astype(np.float32).astype(np.float64) for a, lim in ((x, W), (y, H)))
    p = rng.choice([-1.0, 1.0], n) if rng.random() < 0.5 else np.ones(n)
    eo, ro = E.variance_objective(), R.variance_objective()
    eo.sensor_size = ro.sensor_size = (H, W)
    ro.accum = "f64"
    try:
        with np.errstate(all="ignore"):
            if which == "grid":
                kw = dict(log_scale=bool(rng.integers(0, 2)), num_samples_per_param=int(rng.choice([3, 5])))
                if rng.random() < 0.5:
                    kw["param_ranges"] = [[-80, 80], [-100, 60]]
                r = C.grid_search_initial(x, y, t, p, E.linvel_warp(), eo, (H, W), **kw)
                ref = R.grid_search_initial(x, y, t, p, R.linvel_warp(), ro, (H, W), **kw)
                if not np.array_equal(np.array(r["params"]), np.array(ref["params"])):
                    return desc, "sample positions differ"
                ev, rv = np.asarray(r["eval"], np.float64), np.asarray(ref["eval"], np.float64)
                if np.max(np.abs(ev - rv)) > 2e-5 * np.max(np.abs(rv)):
                    return desc, "sample values: max error %.3e of %.3e" % (np.max(np.abs(ev - rv)), np.max(np.abs(rv)))
                # the best sample: the same one unless two samples tie within the tolerance
                if tuple(r["min_params"]) != tuple(ref["min_params"]):
                    i = ref["params"].index(tuple(r["min_params"]))
                    if abs(rv[i] - ref["min_func_eval"]) > 2e-5 * abs(ref["min_func_eval"]):
                        return desc, "best sample %s vs %s" % (r["min_params"], ref["min_params"])
                return desc, None
            if which == "landscape":
                res = int(rng.choice([40, 50]))
                got = C.objective_landscape(x, y, t, p, eo, E.linvel_warp(), x_range=(-100, 100), y_range=(-100, 100), resolution=res, img_size=(H, W))
                ref = R.objective_landscape(x, y, t, p, ro, R.linvel_warp(), x_range=(-100, 100), y_range=(-100, 100), resolution=res, img_size=(H, W))
                return desc, same(got, ref, None, "landscape", 0) if np.max(np.abs(np.asarray(got) - ref)) > 3e-5 else None
            return desc, None
    except Exception as e:  # noqa: BLE001
        return desc, "raised %s: %s" % (type(e).__name__, e)


def case_misc(rng):
    """events_to_voxel (numpy float64 path), the timestamp images, the event-weights gather, batched objective evaluation"""
    from event_utils_amd.events import DeviceEvents
    which = str(rng.choice(["voxel_np", "ts_image", "ts_image_torch", "ts_hard", "gather", "batch"]))
    H, W = int(rng.integers(4, 300)), int(rng.integers(4, 400))
    n = int(rng.choice([2, 65, 1000, 8193, 100_000, 400_000]))
    impl = str(rng.choice(["auto", "tiled", "direct"]))
    desc = "misc %s %dx%d n=%d impl=%s" % (which, H, W, n, impl)
    os.environ["EVK_IMPL"] = impl
    try:
        with np.errstate(all="ignore"):
            if which == "voxel_np":
                B = int(rng.integers(1, 9))
                x, y = rng.integers(0, W + 1, n), rng.integers(0, H + 1, n)       # the (H+1, W+1) canvas of events_to_image
                t = np.sort(rng.uniform(0, 1, n)); p = rng.choice([-1.0, 1.0], n) if rng.random() < 0.5 else rng.normal(size=n)
                got = E.events_to_voxel(x, y, t, p, B, sensor_size=(H, W))
                ref = R.events_to_voxel(x, y, t, p, B, sensor_size=(H, W))
                if got.dtype != np.float64:
                    return desc, "dtype %s" % got.dtype
                return desc + " B=%d" % B, same(got, ref, None, "grid")
            if which in ("ts_image", "ts_image_torch"):
                x = rng.uniform(0, W + 2, n); y = rng.uniform(0, H + 2, n)
                t = np.sort(rng.uniform(10, 11, n)); p = rng.choice([-1.0, 1.0], n)
                pad = bool(rng.integers(0, 2))
                if which == "ts_image":
                    norm = bool(rng.integers(0, 2))
                    got = E.events_to_timestamp_image(x, y, t, p, sensor_size=(H, W), padding=pad, normalize_timestamps=norm)
                    ref = R.events_to_timestamp_image(x, y, t, p, sensor_size=(H, W), padding=pad, normalize_timestamps=norm, accum="f64")
                else:
                    rev = bool(rng.integers(0, 2))
                    c = [torch.from_numpy(a.astype(np.float32)) for a in (x, y, t - 10.0, p)]
                    got = [g.cpu().numpy() for g in E.events_to_timestamp_image_torch(*c, sensor_size=(H, W), padding=pad, timestamp_reverse=rev)]
                    ref = R.events_to_timestamp_image_torch(*(a.numpy() for a in c), sensor_size=(H, W), padding=pad, timestamp_reverse=rev, accum="f64")
                for k in range(2):
                    # a ratio of two float32 images: where the count is a handful of weights, the quotient carries their rounding
                    err = same(got[k], ref[k], np.ones_like(ref[k]), "image %d" % k, 2e-5)
                    if err is not None:
                        return desc, err
                return desc, None
            if which == "ts_hard":
                # the one-pass timestamp path (round 6) on what the plain case leaves out: scenes that cut hot tiles, polarities of
                # every kind (zeros -> the non-positive class, NaN -> neither), unsorted / constant time stamps, pixels that wrap
                n = int(rng.choice([2, 65, 8193, 60_000, 400_000, 1_000_003, 2_500_000]))
                impl = str(rng.choice(["auto", "tiled"] + (["direct"] if n <= 100_000 else [])))
                os.environ["EVK_IMPL"] = impl
                scene = str(rng.choice(["uniform", "blob", "pixel", "edge"]))
                tk, pk = str(rng.choice(["sorted", "const", "few", "unsorted"])), str(rng.choice(["pm1", "pm1z", "float", "special"]))
                x, y = coords(rng, n, H + 1, W + 1, True, scene)
                if n > 100:
                    k = n // 50
                    x[:k] = rng.uniform(-1, 0, k).astype(np.float32)                  # px = -1: wraps to the last column
                    y[k:2 * k] = rng.uniform(-1, 0, k).astype(np.float32)
                    x[2 * k:3 * k] = rng.uniform(W, W + 3, k).astype(np.float32)      # clipped: pixel (0, 0) with its weights
                t, pw = times(rng, n, tk), weights(rng, n, pk)
                rev = bool(rng.integers(0, 2))
                desc = "misc ts_hard %dx%d n=%d %s t=%s p=%s rev=%d impl=%s" % (H, W, n, scene, tk, pk, rev, impl)
                c = device_cols(rng, (x, y, t, pw))
                got = [g.cpu().numpy() for g in E.events_to_timestamp_image_torch(*c, sensor_size=(H, W), timestamp_reverse=rev)]
                ref = R.events_to_timestamp_image_torch(x, y, t, pw, sensor_size=(H, W), timestamp_reverse=rev, accum="f64")
                for k in range(2):
                    err = same(got[k], ref[k], np.ones_like(ref[k]), "image %d" % k, 2e-5)
                    if err is not None:
                        return desc, err
                return desc, None
            if which == "gather":
                img = rng.normal(size=(H, W))
                x = rng.uniform(0, W + 1, n); y = rng.uniform(0, H + 1, n)
                got, ref = E.image_to_event_weights(x, y, img), R.image_to_event_weights(x, y, img)
                return desc, None if (got.dtype == np.float64 and np.array_equal(got, ref)) else "gather not bit-exact"
            # batch: evaluate_function_batch at K flows against K oracle evaluations
            H, W = max(H, 32), max(W, 32)
            x = rng.uniform(1, W - 1, n).astype(np.float32).astype(np.float64); y = rng.uniform(1, H - 1, n).astype(np.float32).astype(np.float64)
            t = np.sort(rng.uniform(0, 0.1, n).astype(np.float32).astype(np.float64)); p = rng.choice([-1.0, 1.0], n)
            K = int(rng.integers(1, 8))
            flows = [rng.normal(0, 1, 2) * float(rng.choice([5.0, 100.0, 1500.0])) for _ in range(K)]
            eo, ro = E.variance_objective(), R.variance_objective()
            eo.sensor_size = ro.sensor_size = (H, W); ro.accum = "f64"
            ev = DeviceEvents.from_arrays(x, y, t, p)
            got = eo.evaluate_function_batch(flows, ev, None, None, None, E.linvel_warp(), (H, W), 1.0)
            gnum = eo.evaluate_numeric_gradient(flows[0], ev, None, None, None, E.linvel_warp(), (H, W), 1.0, epsilon=1.0)
            ref = [float(ro.evaluate_function(q, x, y, t, p, R.linvel_warp(), (H, W), blur_sigma=1.0)) for q in flows]
            for k in range(K):
                if abs(float(got[k]) - ref[k]) > 3e-5 * abs(ref[k]) + 1e-12:
                    return desc + " K=%d" % K, "flow %d %s: %.9g vs %.9g" % (k, flows[k], float(got[k]), ref[k])
            f1 = [float(ro.evaluate_function(flows[0] + np.eye(2)[i], x, y, t, p, R.linvel_warp(), (H, W), blur_sigma=1.0)) for i in range(2)]
            rnum = np.array([f1[0] - ref[0], f1[1] - ref[0]])
            if np.max(np.abs(np.asarray(gnum, np.float64) - rnum)) > 1e-4 * abs(ref[0]) + 1e-12:     # a difference of two float32 values
                return desc, "numeric gradient %s vs %s" % (gnum, rnum)
            return desc + " K=%d" % K, None
    except Exception as e:  # noqa: BLE001
        return desc, "raised %s: %s" % (type(e).__name__, e)
    finally:
        os.environ.pop("EVK_IMPL", None)


N_IWE = [1, 2, 64, 1000, 8193, 149_999, 150_001, 400_000, 1_200_000]


def iwe_inputs(rng):
    sensor = None if rng.random() < 0.2 else ([(180, 240), (260, 346), (480, 640), (720, 1280)][int(rng.integers(0, 4))]
                                               if rng.random() < 0.4 else (int(rng.integers(8, 720)), int(rng.integers(8, 1280))))
    canvas = (180, 240) if sensor is None else sensor
    img_size = canvas if rng.random() < 0.5 else (max(2, canvas[0] + int(rng.integers(-10, 30))), max(2, canvas[1] + int(rng.integers(-10, 30))))
    n = int(rng.choice(N_IWE))
    H, W = canvas
    scene = str(rng.choice(["uniform", "uniform", "blob", "edge", "pixels"]))
    x = rng.uniform(-2, W + 2, n); y = rng.uniform(-2, H + 2, n)
    if scene == "blob" and n > 8:
        hot = rng.random(n) < 0.7
        x[hot] = W / 2 + rng.uniform(-3, 3, hot.sum()); y[hot] = H / 3 + rng.uniform(-3, 3, hot.sum())
    elif scene == "edge" and n > 8:
        hot = rng.random(n) < 0.8
        x[hot] = W * 0.37 + rng.normal(0, 0.6, hot.sum())
    elif scene == "pixels":        # sensor events: integer pixels
        x, y = np.floor(np.clip(x, 0, W - 1)), np.floor(np.clip(y, 0, H - 1))
    T = float(rng.choice([0.05, 0.2, 1.0]))
    t = np.sort(rng.uniform(0, T, n))
    f32 = rng.random() < 0.75
    if f32:          # float32-representable columns -> float32 device columns; else float64 ones
        x, y, t = (a.astype(np.float32).astype(np.float64) for a in (x, y, t))
        t = np.sort(t)
    pk = str(rng.choice(["pm1", "pm1", "float", "x100"]))
    p = rng.choice([-1.0, 1.0], n) * (100.0 if pk == "x100" else 1.0)
    if pk == "float":
        p = rng.normal(size=n).astype(np.float32).astype(np.float64)
    scale = float(rng.choice([0.0, 10.0, 100.0, 1000.0]))
    prm = rng.normal(0, 1, 2) * scale
    impl = str(rng.choice(["auto", "tiled", "direct"]))
    desc = "sensor=%s img_size=%s n=%d %s f32=%d p=%s T=%g prm=(%.1f, %.1f) impl=%s" % (sensor, img_size, n, scene, f32, pk, T, prm[0], prm[1], impl)
    return desc, sensor, img_size, n, scene, x, y, t, p, prm, impl


def case_iwe(rng):
    desc, sensor, img_size, n, scene, x, y, t, p, prm, impl = iwe_inputs(rng)
    grad, pol = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    desc = "iwe grad=%d pol=%d %s" % (grad, pol, desc)
    with np.errstate(all="ignore"):
        ri, rd = R.get_iwe(prm, x, y, t, p, R.linvel_warp(), img_size, compute_gradient=grad, use_polarity=pol,
                           sensor_size=sensor, accum="f64")
        mi, _ = R.get_iwe(prm, x, y, t, p, R.linvel_warp(), img_size, compute_gradient=False, use_polarity=False,
                          sensor_size=sensor, accum="f64")
    os.environ["EVK_IMPL"] = impl
    try:
        iwe, diwe = E.get_iwe(prm, x, y, t, p, E.linvel_warp(), img_size, compute_gradient=grad, use_polarity=pol, sensor_size=sensor)
    except Exception as e:  # noqa: BLE001
        return desc, "raised %s: %s" % (type(e).__name__, e)
    finally:
        os.environ.pop("EVK_IMPL", None)
    hot = scene in ("blob", "edge")
    # (float64 columns that are not float32-representable stay float64 on the device and take the direct kernels)
    direct_like = impl == "direct" or (impl == "auto" and n < tiled.TILED_MIN_EVENTS_IWE) or "f32=0" in desc
    err = same(iwe, ri, mi, "iwe", 1e-4 if direct_like and hot else 4e-7)
    if err is None and grad:
        if diwe is None:
            return desc, "d_iwe is None"
        # the derivative image's magnitudes: |p| * |t_ref - t| <= T per event and weight -- bounded through the IWE of |p|
        dm = np.broadcast_to(np.asarray(mi, np.float64) * float(t[-1] - t[0]) * 4.0, np.asarray(rd).shape)
        err = same(diwe, rd, dm, "d_iwe", 1e-4 if direct_like and hot else 4e-7)
    elif err is None and diwe is not None:
        err = "d_iwe returned without compute_gradient"
    return desc, err


def case_objective(rng):
    from event_utils_amd.contrast_max import objectives as O
    from event_utils_amd.events import DeviceEvents
    desc, sensor, img_size, n, scene, x, y, t, p, prm, impl = iwe_inputs(rng)
    if n < 64:
        n = 1000; x, y, t, p = (np.resize(a, n) for a in (x, y, t, p)); t = np.sort(t)
    name = str(rng.choice(["variance", "variance", "variance", "sos", "soe", "moa", "sosa", "r1", "rms"]))
    sigma = [None, 0.0, 1.0, 2.0][int(rng.integers(0, 4))]
    resident = bool(rng.integers(0, 2))
    desc = "objective %s sigma=%s resident=%d %s" % (name, sigma, resident, desc)
    mk = {"variance": "variance_objective", "sos": "sos_objective", "soe": "soe_objective", "moa": "moa_objective",
          "sosa": "sosa_objective", "r1": "r1_objective", "rms": "rms_objective"}[name]
    ro, eo = getattr(R, mk)(), getattr(O, mk)()
    ro.sensor_size, ro.accum = sensor, "f64"
    eo.sensor_size = sensor
    with np.errstate(all="ignore"):
        rf = float(ro.evaluate_function(prm, x, y, t, p, R.linvel_warp(), img_size, blur_sigma=sigma))
        rg = np.asarray(ro.evaluate_gradient(prm, x, y, t, p, R.linvel_warp(), img_size, blur_sigma=sigma), np.float64) \
            if getattr(ro, "has_derivative", True) and hasattr(ro, "evaluate_gradient") else None
    os.environ["EVK_IMPL"] = impl
    try:
        args = (DeviceEvents.from_arrays(x, y, t, p), None, None, None) if resident else (x, y, t, p)
        f = float(eo.evaluate_function(prm, *args, E.linvel_warp(), img_size, blur_sigma=sigma))
        g = np.asarray(eo.evaluate_gradient(prm, *args, E.linvel_warp(), img_size, blur_sigma=sigma), np.float64) \
            if rg is not None and eo.has_derivative else None
    except Exception as e:  # noqa: BLE001
        return desc, "raised %s: %s" % (type(e).__name__, e)
    finally:
        os.environ.pop("EVK_IMPL", None)
    if not np.isfinite(rf) or not np.isfinite(f):
        return desc, None if (np.isnan(rf) and np.isnan(f)) or rf == f else "f %r vs %r" % (f, rf)
    # float32 images summed / squared: 2e-5 relative (as tests/test_gpu_parity.py for the other objectives); tiny objectives
    # (a handful of events on a large canvas) get the absolute floor of the float32 image they are computed from
    # (soe = sum of exp(image): a relative error of the image's largest value times that value)
    rel = 3e-5 * (max(1.0, abs(np.log(max(abs(rf), 1e-300)))) if name == "soe" else 1.0)
    if abs(f - rf) > rel * abs(rf) + 1e-12:
        return desc, "f %.9g vs %.9g" % (f, rf)
    if g is not None:
        if g.shape != rg.shape:
            return desc, "gradient shape %s vs %s" % (g.shape, rg.shape)
        direct_like = impl == "direct" or (impl == "auto" and n < tiled.TILED_MIN_EVENTS_IWE) or "f32=0" in desc
        gtol = 1e-3 if direct_like and scene in ("blob", "edge") else 1e-4     # float32 atomics on hot pixels, as the reference's
        gtol *= max(1.0, abs(np.log(max(abs(rf), 1e-300)))) if name == "soe" else 1.0
        if np.isfinite(rg).all() and np.max(np.abs(g - rg)) > gtol * np.max(np.abs(rg)) + 1e-6 * abs(rf) + 1e-12:
            return desc, "gradient %s vs %s" % (g, rg)
    return desc, None


# ---- filters, augmentation, datasets, motion models -----------------------------------------------------------------------
# Their references are the restatements the CPU suite checks against the upstream code (tests/test_cpu_*.py,
# tests/test_gpu_data_loaders.py, tests/_motion_models_np.py), imported from tests/ on first use.

def _t(name):
    import importlib
    tests = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    return importlib.import_module(name)


def _host(a):
    return a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def exact(got, want, what):
    """Bit equality with the restatement: dtype, shape and bits (NaN payloads included)."""
    a, b = _host(got), np.asarray(want)
    if a.dtype != b.dtype or a.shape != b.shape:
        return "%s: %s%s vs %s%s" % (what, a.dtype, a.shape, b.dtype, b.shape)
    if not np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)):
        return "%s: %d of %d elements differ" % (what, int((a != b).sum()), a.size)
    return None


def equal(got, want, what):
    """Value equality (+0.0 == -0.0) with NaN in the same places: the rule of tests/test_gpu_data_loaders.py's RobustNorm
    checks.  (The reference's percentiles come from kthvalue, whose pick among equal values -- +0.0 or -0.0 -- is unspecified,
    and the sign of a zero follows it through the clamp and the subtraction.)"""
    a, b = _host(got), _host(want)
    if a.dtype != b.dtype or a.shape != b.shape:
        return "%s: %s%s vs %s%s" % (what, a.dtype, a.shape, b.dtype, b.shape)
    ok = (a == b) | (np.isnan(a) & np.isnan(b))
    return None if ok.all() else "%s: %d of %d elements differ" % (what, int((~ok).sum()), a.size)


def exact_all(got, want, what):
    from event_utils_amd.events import DeviceEvents
    if isinstance(got, DeviceEvents):
        got = (got.x, got.y, got.t, got.p)
    got, want = list(got), list(want)
    if len(got) != len(want):
        return "%s: %d outputs vs %d" % (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        err = exact(g, w, "%s[%d]" % (what, k))
        if err is not None:
            return err
    return None


def raises_as(ref_call, call, what):
    """(reference result, result, None) when neither raises; (None, None, verdict) when either does: the same exception type
    where the restatement raises, a report where only one side does."""
    try:
        with np.errstate(all="ignore"):
            ref = ref_call()
    except Exception as e:  # noqa: BLE001
        try:
            call()
        except type(e):
            return None, None, "ok"
        except Exception as e2:  # noqa: BLE001
            return None, None, "%s: restatement raises %s, here %s: %s" % (what, type(e).__name__, type(e2).__name__, e2)
        return None, None, "%s: restatement raises %s, here returns" % (what, type(e).__name__)
    try:
        got = call()
    except Exception as e:  # noqa: BLE001
        return None, None, "%s: raised %s: %s" % (what, type(e).__name__, e)
    return ref, got, None


def _dev(rng, a, sliced=None):
    """A numpy column as a device tensor: fresh (16-byte aligned) or a slice 1-3 elements into a larger buffer."""
    t = torch.from_numpy(np.ascontiguousarray(a))
    if sliced is None:
        sliced = rng.random() < 0.4
    if not sliced:
        return t.cuda()
    off = int(rng.integers(1, 4))
    buf = torch.zeros(off + len(a) + int(rng.integers(0, 5)), dtype=t.dtype, device="cuda")
    buf[off:off + len(a)] = t.cuda()
    return buf[off:off + len(a)]


N_SEL = [1, 2, 3, 5, 255, 1000, 4095, 4096, 4097, 8191, 8192, 8193, 12_287, 12_289, 40_959, 40_961, 65_537, 300_001]


def _n_around(rng, choices, unit, kmax):
    if rng.random() < 0.5:
        return int(rng.choice(choices))
    return max(1, int(rng.integers(1, kmax + 1)) * unit + int(rng.integers(-3, 4)))


def case_filters(rng):
    """remove_hot_pixels / clip_events_to_bounds / get_events_from_mask (evk_select.hip) bit for bit against
    tests/test_cpu_filters.py's restatement: images from 1 x 1 to 1300 x 800, n around the 4096-event SEL_CHUNK, coordinates
    in every integer / float dtype as numpy, device tensors (aligned or sliced) and DeviceEvents, tied pixel counts, num_hot
    from 0 to beyond the pixel count, bounds on / between / outside the coordinates, masks of any density."""
    Fm = _t("test_cpu_filters")
    from event_utils_amd.events import DeviceEvents
    which = str(rng.choice(["hot", "hot", "clip", "mask"]))
    H, W = (int(rng.integers(1, 9)), int(rng.integers(1, 9))) if rng.random() < 0.3 else (int(rng.integers(1, 800)), int(rng.integers(1, 1300)))
    n = _n_around(rng, N_SEL, 4096, 20)
    mode = str(rng.choice(["numpy", "numpy", "torch", "events"]))
    cdt = np.dtype(str(rng.choice(["int16", "int32", "int64", "float32", "float64"])))
    if mode == "events":
        cdt = np.dtype(str(rng.choice(["float32", "float64"])))
    scene = str(rng.choice(["uniform", "ties", "hot"]))
    desc = "filters %s %dx%d n=%d %s %s %s" % (which, H, W, n, mode, cdt, scene)
    x, y = rng.integers(0, W + (which == "hot"), n), rng.integers(0, H + (which == "hot"), n)     # hot: x == W / y == H legal
    if scene == "ties" and n > 8:           # k pixels with exactly the same count each (ties go to the lower index)
        k = int(rng.integers(2, 12))
        px, py = rng.integers(0, W, k), rng.integers(0, H, k)
        c = n // (k + 1)
        x[:k * c], y[:k * c] = np.repeat(px, c), np.repeat(py, c)
        perm = rng.permutation(n)
        x, y = x[perm], y[perm]
    elif scene == "hot" and n > 8:
        h = rng.random(n) < 0.2
        x[h], y[h] = int(rng.integers(0, W)), int(rng.integers(0, H))
    t = np.sort(rng.uniform(0, 1, n))
    pk = str(rng.choice(["pm1", "ones", "float", "bool", "nan"] if mode == "numpy" else ["pm1", "ones", "float"]))
    p = {"pm1": lambda: rng.integers(0, 2, n) * 2 - 1, "ones": lambda: np.ones(n, np.int64),
         "float": lambda: rng.integers(-2, 4, n) * 0.5, "bool": lambda: rng.random(n) < 0.7,
         "nan": lambda: np.where(rng.random(n) < 0.001, np.nan, 1.0)}[pk]()
    desc += " p=%s" % pk
    try:
        if which == "hot":
            P = H * W
            num_hot = int(rng.choice([0, 1, int(rng.integers(2, 60)), P, P + int(rng.integers(1, 5)), max(P - 1, 0)]))
            if num_hot > 64 and n > 8196:    # (the restatement removes pixel by pixel: n x hot pixels)
                n = int(rng.choice([4095, 4096, 4097, 8191, 8193]))
                x, y, t, p = x[:n], y[:n], t[:n], p[:n]
            desc += " n=%d num_hot=%d" % (n, num_hot)
            if mode == "numpy":
                cols = [x.astype(cdt), y.astype(cdt), t, p]
                ref, got, v = raises_as(lambda: Fm.np_remove_hot_pixels(*cols, sensor_size=(H, W), num_hot=num_hot),
                                        lambda: E.remove_hot_pixels(*cols, sensor_size=(H, W), num_hot=num_hot), "hot")
                return desc, None if v == "ok" else (v or exact_all(got, ref, "hot"))
            # device columns: every column in the coordinate dtype (float coordinates that hold integers are accepted)
            dt = cdt
            cols = [a.astype(dt) for a in (x, y, t if dt.kind == "f" else (t * 1000).astype(dt), p)]
            want = Fm.np_remove_hot_pixels(x, y, cols[2], cols[3], (H, W), num_hot)
            want = [w.astype(dt) for w in want]
            if mode == "torch":
                got = E.remove_hot_pixels(*[_dev(rng, c) for c in cols], sensor_size=(H, W), num_hot=num_hot)
            else:
                ev = DeviceEvents.from_arrays(*cols, precision="f32" if dt == np.float32 else "f64")
                got = E.remove_hot_pixels(ev, None, None, None, sensor_size=(H, W), num_hot=num_hot)
            return desc, exact_all(got, want, "hot")
        if which == "clip":
            real = rng.random() < 0.5
            xs = (x + rng.choice([0.0, 0.5, 0.25], n)) if real else x * 1.0
            ys = (y + rng.choice([0.0, 0.5, 0.75], n)) if real else y * 1.0
            dt = cdt if (real is False or cdt.kind == "f") else np.dtype(np.float64)
            cols = [xs.astype(dt), ys.astype(dt), t, p.astype(np.float64)]

            def bound(lim):
                k = rng.random()
                if k < 0.4:
                    return int(rng.integers(-1, lim + 2))               # on an integer coordinate
                if k < 0.7:
                    return int(rng.integers(-1, lim + 2)) + 0.5         # on a half-integer one
                return float(rng.uniform(-2, lim + 2))                  # between them
            miny, minx = bound(H), bound(W)
            b = [miny, max(miny, bound(H)), minx, max(minx, bound(W))] if rng.random() < 0.7 else [bound(H), bound(W)]
            sz = bool(rng.integers(0, 2))
            desc += " real=%d bounds=%s set_zero=%d" % (real, b, sz)
            want = Fm.np_clip_events_to_bounds(*cols, b, set_zero=sz)
            if mode == "numpy":
                got = E.clip_events_to_bounds(*cols, b, set_zero=sz)
            elif mode == "torch":
                got = E.clip_events_to_bounds(*[_dev(rng, c) for c in cols], b, set_zero=sz)
            else:
                cols = [c.astype(dt) for c in cols]
                want = Fm.np_clip_events_to_bounds(*cols, b, set_zero=sz)
                ev = DeviceEvents.from_arrays(*cols, precision="f32" if dt == np.float32 else "f64")
                got = E.clip_events_to_bounds(ev, None, None, None, b, set_zero=sz)
            return desc, exact_all(got, want, "clip")
        # mask: coordinates truncated toward zero, negative ones wrap; a few out of range / NaN -> IndexError
        dens = float(rng.choice([0.0, 0.01, 0.3, 0.9, 1.0]))
        mdt = np.dtype(str(rng.choice(["float32", "float64"])))
        mask = np.where(rng.random((H, W)) < dens, rng.uniform(0.01, 1.0, (H, W)), rng.uniform(0, 0.0101, (H, W))).astype(mdt)
        xs, ys = rng.uniform(-W + 0.01, W - 0.01, n), rng.uniform(-H + 0.01, H - 0.01, n)
        if rng.random() < 0.1:
            k = int(rng.integers(0, n))
            xs[k] = float(rng.choice([np.nan, W, -W - 1.0]))
        fdt = np.dtype(np.float64) if cdt.kind != "f" else cdt
        xs, ys = xs.astype(fdt), ys.astype(fdt)
        desc += " mask %s density=%g" % (mdt, dens)
        if mode == "numpy":
            args = (xs, ys)
        elif mode == "torch":
            args = (_dev(rng, xs), _dev(rng, ys))
        else:
            args = (DeviceEvents.from_arrays(xs, ys, np.zeros(n), np.zeros(n), precision="f32" if fdt == np.float32 else "f64"), None)
        mk = mask if rng.random() < 0.5 else torch.from_numpy(mask).cuda()
        ref, got, v = raises_as(lambda: Fm.np_get_events_from_mask(mask, xs, ys), lambda: E.get_events_from_mask(mk, *args), "mask")
        return desc, None if v == "ok" else (v or exact(got, ref, "mask"))
    except Exception as e:  # noqa: BLE001
        return desc, "raised %s: %s" % (type(e).__name__, e)


def case_augment(rng):
    """add_random_events / remove_events / add_correlated_events (evk_augment.hip, the subset select of evk_select.hip) and
    flip / crop / rotate bit for bit against tests/test_cpu_augment.py's restatement: numpy, device tensors and DeviceEvents,
    mixed column dtypes, random seeds, to_add / to_remove from 0 to beyond n, add_noise, time stamps with heavy ties (the
    sort's tie order), random resolutions, angles and centres."""
    Am = _t("test_cpu_augment")
    from event_utils_amd import DeviceEvents
    from event_utils_amd.augmentation import event_augmentation as A
    which = str(rng.choice(["random", "random", "remove", "correlated", "flip", "crop", "rotate"]))
    H, W = int(rng.integers(2, 800)), int(rng.integers(2, 1300))
    n = _n_around(rng, [1, 2, 3, 64, 1000, 4095, 4097, 65_537, 250_001], 4096, 30)
    mode = str(rng.choice(["numpy", "torch", "events"]))
    tk = str(rng.choice(["ties", "ties", "sorted", "unsorted"]))
    seed = int(rng.integers(0, 2 ** 63))
    dts = [np.dtype(str(rng.choice(["int16", "int32", "int64", "float32", "float64"]))) for _ in range(2)] + \
        [np.dtype(str(rng.choice(["float64", "float32"]))), np.dtype(str(rng.choice(["int8", "int64", "float32", "float64"])))]
    x, y = rng.integers(0, W, n), rng.integers(0, H, n)
    t = {"ties": lambda: np.sort(rng.integers(0, max(2, n // 50), n)) * 0.125, "sorted": lambda: np.sort(rng.uniform(0, 2, n)),
         "unsorted": lambda: rng.uniform(0, 2, n)}[tk]()
    p = rng.integers(0, 2, n) * 2 - 1
    cols = [a.astype(d) for a, d in zip((x, y, t, p), dts)]
    desc = "augment %s %dx%d n=%d %s t=%s dtypes=%s seed=%d" % (which, H, W, n, mode, tk, ",".join(d.name for d in dts), seed)

    def args():
        if mode == "numpy":
            return cols
        if mode == "torch":
            return [_dev(rng, c) for c in cols]
        return (DeviceEvents(*[_dev(rng, c.astype(np.float64)) for c in cols]), None, None, None)

    def f64(ws):
        return [np.asarray(w).astype(np.float64) for w in ws] if mode == "events" else ws
    try:
        if which == "random":
            m = int(rng.choice([0, 1, 7, int(rng.integers(0, 2 * n + 2)), n + 5, 70_001]))
            kw = [dict(), dict(sort=False, return_merged=False), dict(sort=True, return_merged=False), dict(sort=False, return_merged=True)][int(rng.integers(0, 4))]
            desc += " to_add=%d %s" % (m, kw)
            got = A.add_random_events(*args(), m, seed=seed, **kw)
            return desc, exact_all(got, f64(Am.np_add_random_events(*cols, m, seed=seed, **kw)), "add_random_events")
        if which == "remove":
            r = int(rng.choice([0, 1, int(rng.integers(0, n + 1)), n - 1, n, n + 1, n + int(rng.integers(2, 100))]))
            noise = int(rng.choice([0, 0, 1, int(rng.integers(1, n + 2))]))
            desc += " to_remove=%d add_noise=%d" % (r, noise)
            got = A.remove_events(*args(), r, add_noise=noise, seed=seed)
            want = Am.np_remove_events(*cols, r, add_noise=noise, seed=seed)
            return desc, exact_all(got, f64(want) if r <= n else want, "remove_events")
        if which == "correlated":
            m = int(rng.choice([0, 1, int(rng.integers(1, n + 1)), int(rng.integers(n, 3 * n + 2))]))
            m = min(m, 400_000)
            noise = int(rng.choice([0, 0, int(rng.integers(1, 50))]))
            xy_std, ts_std = (0.0, 0.0) if rng.random() < 0.6 else (float(rng.uniform(0, 4)), float(rng.uniform(0, 0.01)))
            desc += " to_add=%d noise=%d std=(%g, %g)" % (m, noise, xy_std, ts_std)
            got = A.add_correlated_events(*args(), m, xy_std=xy_std, ts_std=ts_std, add_noise=noise, seed=seed)
            g = [_host(c) for c in ((got.x, got.y, got.t, got.p) if isinstance(got, DeviceEvents) else got)]
            if any(c.dtype != np.float64 or len(c) != m + noise for c in g):
                return desc, "dtypes %s, lengths %s" % ([c.dtype for c in g], [len(c) for c in g])
            err = exact_all(g, Am.np_sort_events(*g), "sorted output")
            if err is not None or m == 0:
                return desc, err
            # without the noise rows (x, y, p from the input's ranges, t uniform): can't be told apart, so only the count
            if noise == 0:
                f = [c.astype(np.float64) for c in cols]
                mx, my = f[0].max(), f[1].max()
                if not (np.all((g[0] >= 0) & (g[0] <= mx) & (g[1] >= 0) & (g[1] <= my)) and np.all(g[0] == np.floor(g[0]))):
                    return desc, "correlated x / y outside [0, max] or not integral"
                if not set(np.unique(g[3])) <= set(np.unique(f[3])):
                    return desc, "correlated p not taken from the input"
                if xy_std == 0 and ts_std == 0:     # every event a copy of an input event, at most int(m / n) + 1 copies each
                    key = lambda c: np.stack(c, 1).view(np.dtype((np.void, 32))).ravel()    # noqa: E731
                    src, out = key([np.ascontiguousarray(c) for c in f]), key([np.ascontiguousarray(c) for c in g])
                    if not np.isin(out, src).all():
                        return desc, "a correlated event is not a copy of an input event"
                    u, c = np.unique(out, return_counts=True)
                    _, cin = np.unique(src, return_counts=True)
                    if c.max() > (int(m / n) + 1) * cin.max():
                        return desc, "an input event copied %d times (at most %d)" % (c.max(), int(m / n) + 1)
            return desc, None
        if which == "flip":
            f = A.flip_events_x if rng.random() < 0.5 else A.flip_events_y
            got = f(*args(), sensor_resolution=(H, W))
            want = f(*cols, sensor_resolution=(H, W))          # numpy's own arithmetic
            return desc, exact_all(got, f64(want), f.__name__)
        if which == "crop":
            nr = (int(rng.integers(0, H + 3)), int(rng.integers(0, W + 3)))
            desc += " to %s" % (nr,)
            a = args()
            got = A.crop_events(a[0], a[1], (H, W), nr)
            want = _t("test_cpu_filters").np_clip_events_to_bounds(cols[0], cols[1], None, None, nr)[:2]
            if isinstance(got, DeviceEvents):
                return desc, exact_all((got.x, got.y), [w.astype(np.float64) for w in want], "crop")
            return desc, exact_all(got, want, "crop")
        theta = None if rng.random() < 0.3 else float(rng.uniform(-7, 7))
        centre = None if rng.random() < 0.3 else ((int(rng.integers(-50, W + 50)), int(rng.integers(-50, H + 50))) if rng.random() < 0.5
                                                  else (float(rng.uniform(-50, W + 50)), float(rng.uniform(-50, H + 50))))
        np_seed = int(rng.integers(0, 2 ** 31))
        desc += " theta=%s centre=%s" % (theta, centre)
        np.random.seed(np_seed)
        want = Am.np_rotate_events(cols[0], cols[1], (H, W), theta, centre)
        np.random.seed(np_seed)
        if mode == "numpy":
            clip = bool(rng.integers(0, 2))
            got = A.rotate_events(cols[0], cols[1], (H, W), theta, centre, clip_to_range=clip)
            if clip:
                k = (want[0] >= 0) & (want[0] < W) & (want[1] >= 0) & (want[1] < H)
                want = (want[0][k], want[1][k]) + tuple(want[2:])
        else:
            got = A.rotate_events(_dev(rng, cols[0]), _dev(rng, cols[1]), (H, W), theta, centre)
        err = exact_all(got[:2], want[:2], "rotate")
        if err is None and (got[2] != want[2] or tuple(got[3]) != tuple(want[3])):
            err = "rotate: theta / centre %s %s vs %s %s" % (got[2], got[3], want[2], want[3])
        return desc, err
    except Exception as e:  # noqa: BLE001
        return desc, "raised %s: %s" % (type(e).__name__, e)


def _tile_sizes(rng, C):
    """H, W for a plane of H * W cells against the window kernel's tile of tile_px = (40 KiB / (4 C)) & ~3 cells: a multiple
    of it or not, H * W % 4 == 0 or not; neither above 32 767 (the streams hold int16 coordinates)."""
    tile = (40 * 1024 // (4 * C)) & ~3
    k = rng.random()
    for _ in range(200):
        if k < 0.3:                          # a whole number of tiles (H * W = m * tile)
            m = int(rng.integers(1, 12))
            cells = m * tile
            divs = [d for d in range(1, int(np.sqrt(cells)) + 1) if cells % d == 0]
            h = int(rng.choice(divs))
            H, W = (h, cells // h) if rng.random() < 0.5 else (cells // h, h)
        else:
            H, W = int(rng.integers(1, 300)), int(rng.integers(1, 400))
        if k >= 0.3 and k < 0.6 and (H * W) % 4 == 0:
            continue                         # the scalar store path
        if H * W <= 400 * 400 and max(H, W) <= 32_767:       # (int16 coordinates)
            return H, W
    return 13, 17


def case_datasets(rng):
    """MemMapDataset / NpyDataset voxel windows (evk_voxel_windows_f32), return_events rows and RobustNorm / CenterCrop
    (evk_robust_norm_f32) against the oracle per window (widen_native_events + events_to_voxel_torch, tests/test_gpu_data_loaders
    oracle_window) and the reference's RobustNorm: planes that are and are not a whole number of tiles, H * W % 4 != 0, B from
    1 to 12, combined / split channels, windows that start at any event, empty / one-event / equal-stamp / long windows,
    int16 / float32 / interleaved coordinates, every polarity byte kind, out-of-range coordinates; __getitem__ against
    __getitems__; RobustNorm on ties, +-0.0, negatives, NaN, short items and strided crops."""
    import tempfile
    G = _t("test_gpu_data_loaders")
    from event_utils_amd.data_loaders import _kernels as K
    which = str(rng.choice(["windows", "windows", "dataset", "robust"]))
    try:
        if which == "robust":
            return _robust_case(rng, G, K)
        B = int(rng.integers(1, 13))
        split = bool(rng.integers(0, 2))
        H, W = _tile_sizes(rng, 2 * B if split else B)
        if which == "dataset":
            with tempfile.TemporaryDirectory() as root:
                return _dataset_case(rng, G, root, H, W, B, split)
        n = int(rng.choice([1, 2, 5, 1000, 4099, 20_000, 60_001])) if rng.random() < 0.9 else K.LONG_WINDOW_EVENTS + int(rng.integers(1, 30_000))
        kind = str(rng.choice(["xy", "xs_ys", "f32", "bool", "int8", "literal", "literal"]))
        tdt = np.float32 if rng.random() < 0.25 else np.float64
        t = np.sort(rng.uniform(0.0, 1.0, n)) + (0.0 if tdt == np.float32 else 1.6e9)
        if n > 50:
            a = int(rng.integers(0, n - 40))
            t[a:a + int(rng.integers(2, 40))] = t[a]                        # a run of equal stamps
        t = t.astype(tdt)
        x, y = rng.integers(0, W, n), rng.integers(0, H, n)
        wrap = rng.random() < 0.3
        if wrap:                                                            # negative indices wrap once, as index_put_
            k = rng.random(n) < 0.05
            x[k] -= W
            y[rng.random(n) < 0.05] -= H
        bad = n > 10 and rng.random() < 0.1
        if bad:                                                             # outside: IndexError for the windows holding it
            j = int(rng.integers(0, n))
            if rng.random() < 0.5:
                x[j] = W if rng.random() < 0.5 else -W - 1
            else:
                y[j] = H if rng.random() < 0.5 else -H - 1
        pu = rng.integers(0, 2, n).astype(np.uint8)
        if kind == "xy":
            s_args, cols, pol = dict(xy=np.stack([x, y], 1).astype(np.int16), ts=t, ps=pu), (np.stack([x, y], 1).astype(np.int16), None, t, pu), "pm1"
        elif kind == "xs_ys":
            s_args, cols, pol = dict(xs=x.astype(np.int16), ys=y.astype(np.int16), ts=t, ps=pu), (x.astype(np.int16), y.astype(np.int16), t, pu), "pm1"
        elif kind == "bool":
            pb = pu.astype(bool)
            s_args, cols, pol = dict(xy=np.stack([x, y], 1).astype(np.int16), ts=t, ps=pb), (x, y, t, pb), "pm1"
        elif kind == "int8":       # not a native byte kind: widened on the host (p * 2.0 - 1.0), float32 coordinates
            p8 = pu.astype(np.int8)
            s_args, cols, pol = dict(xs=x.astype(np.float32), ys=y.astype(np.float32), ts=t, ps=p8), (x, y, t, p8), "pm1"
        elif kind == "literal":    # npy format: float coordinates, literal float polarities (+-1 and 0)
            pl = rng.integers(-1, 2, n).astype(np.float64)
            s_args, cols, pol = dict(xs=x.astype(np.float64), ys=y.astype(np.float64), ts=t, ps=pl, p_pm1=False), (x, y, t, pl), "literal"
        else:
            s_args, cols, pol = dict(xs=x.astype(np.float32), ys=y.astype(np.float32), ts=t, ps=pu), (x, y, t, pu), "pm1"
        nw = int(rng.integers(1, 9))
        wins = []
        for _ in range(nw):
            r = rng.random()
            a = int(rng.integers(0, n + 1))
            if r < 0.15:
                b = a                                                       # empty
            elif r < 0.3:
                b = min(a + 1, n)                                           # one event
            else:
                b = int(rng.integers(a, n + 1))
            wins.append((a, b))
        if n >= K.LONG_WINDOW_EVENTS and rng.random() < 0.5:
            wins = [(int(rng.integers(0, n - K.LONG_WINDOW_EVENTS)), n)]
        desc = "datasets windows %s %dx%d B=%d split=%d n=%d t=%s wrap=%d bad=%d windows=%s" % (
            kind, H, W, B, split, n, np.dtype(tdt).name, wrap, bad, wins if len(wins) < 4 else "%d" % len(wins))
        s = K.ResidentStream(**s_args)
        pm = (np.ones(n, np.uint8) if pol == "pm1" and cols[3].dtype != np.int8 else np.abs(cols[3].astype(np.float64))
              if pol == "literal" else np.ones(n, np.int8))
        refs, mags, ref_exc = [], [], None
        try:
            with np.errstate(all="ignore"):
                for a, b in wins:
                    refs.append(G.oracle_window(*cols, a, b, B, (H, W), split, pol))
                    mags.append(G.oracle_window(cols[0], cols[1], cols[2], pm, a, b, B, (H, W), split, pol))
        except IndexError as e:
            ref_exc = e
        try:
            got = s.voxel_windows(wins, B, (H, W), split).cpu().numpy()
        except IndexError:
            return desc, None if ref_exc is not None else "raised IndexError where the oracle returns"
        if ref_exc is not None:
            return desc, "returns where the oracle raises IndexError"
        for k, (r, m) in enumerate(zip(refs, mags)):
            err = same(got[k], r, np.where(np.isfinite(m), np.abs(m), 0), "window %d %s" % (k, wins[k]))
            if err is not None:
                return desc, err
        if rng.random() < 0.3:                          # return_events rows: [x, y, (float)(t - t[a]), p], bit for bit
            packed, rows, lens = s.pack_events(wins)
            for (a, b), r0, m in zip(wins, rows, lens):
                if m:
                    xs, ys, ts, ps = R.widen_native_events(cols[0][a:b], None if cols[1] is None else cols[1][a:b], cols[2][a:b],
                                                           cols[3][a:b], polarity=pol)
                    err = exact(packed[r0:r0 + m], np.stack((xs, ys, ts, ps), 1), "packed rows of window %s" % ((a, b),))
                    if err is not None:
                        return desc, err
        return desc, None
    except Exception as e:  # noqa: BLE001
        return "datasets %s" % which, "raised %s: %s" % (type(e).__name__, e)


def _dataset_case(rng, G, root, H, W, B, split):
    from event_utils_amd.data_loaders import MemMapDataset, NpyDataset
    from event_utils_amd.data_loaders.data_augmentation import CenterCrop
    fmt = str(rng.choice(["memmap", "memmap", "npy"]))
    n = int(rng.choice([300, 3000, 20_000, 20_000]))
    mth = str(rng.choice(["k_events", "t_seconds", "fixed_frames", "between_frames"] if fmt == "memmap" else ["k_events", "t_seconds", "fixed_frames"]))
    if mth == "k_events":
        k = int(rng.integers(1, n // 3))
        vm = {'method': mth, 'k': k, 'sliding_window_w': int(rng.integers(0, k))}
    elif mth == "t_seconds":
        span = 1.0 if fmt == "memmap" else 2.0
        tt = float(rng.uniform(0.002, span / 3))
        vm = {'method': mth, 't': tt, 'sliding_window_t': float(rng.choice([0.0, rng.uniform(0, tt * 0.9)]))}
    elif mth == "fixed_frames":
        vm = {'method': mth, 'num_frames': int(rng.integers(1, 25))}
    else:
        vm = {'method': mth}
    tr = {}
    if rng.random() < 0.5:
        if rng.random() < 0.5:
            tr['CenterCrop'] = {'size': (int(rng.integers(1, H + 1)), int(rng.integers(1, W + 1)))}
        lo = float(rng.choice([0, 0, 5, 12.5, rng.uniform(0, 50)]))
        tr['RobustNorm'] = {'low_perc': lo, 'top_perc': float(rng.choice([95, 100, lo, rng.uniform(lo, 100)]))}
    desc = "datasets %s %dx%d B=%d split=%d n=%d %s transforms=%s" % (fmt, H, W, B, split, n, vm, tr)
    kw = dict(voxel_method=dict(vm), combined_voxel_channels=not split, num_bins=B, return_frame=False, return_flow=False,
              sensor_resolution=(H, W),
              return_events=bool(rng.integers(0, 2)))
    if fmt == "memmap":
        _, xy, t, p = G.write_memmap(os.path.join(root, "mm"), n, H, W, seed=int(rng.integers(0, 1 << 30)),
                                     frames=int(rng.integers(2, 12)) if mth == "between_frames" else 0)
        cols, pol = (xy, None, t, p), "pm1"
        make = lambda trs: MemMapDataset(os.path.join(root, "mm"), transforms=trs, **kw)      # noqa: E731
    else:
        path, data = G.write_npy(os.path.join(root, "ev.npy"), n, H, W, seed=int(rng.integers(0, 1 << 30)))
        cols, pol = (data[:, 0], data[:, 1], data[:, 3] * 1e-6, data[:, 2] * 2 - 1), "literal"
        make = lambda trs: NpyDataset(path, transforms=trs, **kw)                              # noqa: E731
    ds = make({})
    H, W = (int(v) for v in ds.sensor_resolution)      # (the loaders take it from the data: max + 1 of the coordinates)
    idx = [i for i in range(len(ds)) if ds.event_indices[i][1] <= n]
    if not idx:
        return desc, None
    if len(idx) > 24:
        idx = sorted(rng.choice(idx, 24, replace=False).tolist())
    items = ds.__getitems__(idx)
    for i, item in zip(idx, items):
        a, b = ds.get_event_indices(i)
        with np.errstate(all="ignore"):
            ref = G.oracle_window(*cols, a, b, B, (H, W), split, pol)
            pm = np.ones(len(cols[3]), np.uint8) if pol == "pm1" else np.abs(cols[3])
            mag = G.oracle_window(cols[0], cols[1], cols[2], pm, a, b, B, (H, W), split, pol)
        err = same(item['voxel'].cpu().numpy(), ref, mag, "item %d (%d, %d)" % (i, a, b))
        if err is not None:
            return desc, err
    if tr:
        tds = make(tr)
        batch = tds.__getitems__(idx)
        for i, item, raw in zip(idx, batch, items):
            one = tds[i]
            # per item: the transforms applied by the reference's code to this item's own (device) grid, bit for bit
            v = raw['voxel'].cpu()
            if 'CenterCrop' in tr:
                v = CenterCrop(tr['CenterCrop']['size'])(v)
            want = G.reference_robust_norm(v, tr['RobustNorm']['low_perc'], tr['RobustNorm']['top_perc'])[0]
            for what, g in (("__getitems__", item['voxel']), ("__getitem__", one['voxel'])):
                # (a second launch of the window kernel: its LDS float atomics may add in another order, so not bit for bit)
                err = same(g.cpu().numpy(), want.numpy(), None, "%s transforms of item %d" % (what, i))
                if err is not None:
                    return desc, err
    for i in idx[:4]:                                   # __getitem__ against __getitems__
        one, many = ds[i], ds.__getitems__([i])[0]
        err = same(one['voxel'].cpu().numpy(), many['voxel'].cpu().numpy(), None, "__getitem__ vs __getitems__ item %d" % i)
        if err is None and kw['return_events']:
            err = exact(one['events'], many['events'].cpu().numpy(), "events of item %d" % i)
        if err is not None:
            return desc, err
    return desc, None


def _robust_case(rng, G, K):
    from event_utils_amd.data_loaders.data_augmentation import RobustNorm
    nb = int(rng.integers(1, 7))
    shape = tuple(int(v) for v in (rng.integers(1, 6), rng.integers(1, 40), rng.integers(1, 60)))
    if rng.random() < 0.3:
        shape = (1, 1, int(rng.integers(1, 300)))                           # items shorter than a block
    kind = str(rng.choice(["randn", "ties", "signed_zeros", "sparse", "constant", "wide"]))
    g = torch.Generator().manual_seed(int(rng.integers(0, 1 << 30)))
    x = {"randn": lambda: torch.randn((nb,) + shape, generator=g),
         "ties": lambda: torch.randint(-3, 4, (nb,) + shape, generator=g).float() * 0.5,
         "signed_zeros": lambda: torch.where(torch.rand((nb,) + shape, generator=g) < 0.5, -0.0, 0.0)
         + (torch.rand((nb,) + shape, generator=g) < 0.05) * torch.randn((nb,) + shape, generator=g),
         "sparse": lambda: torch.randn((nb,) + shape, generator=g) * (torch.rand((nb,) + shape, generator=g) < 0.05),
         "constant": lambda: torch.full((nb,) + shape, float(rng.choice([0.0, -2.5, 7.0]))),
         "wide": lambda: torch.randn((nb,) + shape, generator=g) * torch.exp(torch.randn((nb,) + shape, generator=g) * 20)}[kind]()
    if rng.random() < 0.2:
        x.view(-1)[int(rng.integers(0, x.numel()))] = float('nan')
    lo = float(rng.choice([0, 0, 3, 12.5, 50, rng.uniform(0, 100)]))
    top = float(rng.choice([95, 100, lo, rng.uniform(lo, 100)]))
    crop = rng.random() < 0.4 and shape[1] > 2 and shape[2] > 2
    xd = x.cuda()
    if crop:                                           # a strided view of every item
        r0, c0 = int(rng.integers(0, shape[1] // 2)), int(rng.integers(0, shape[2] // 2))
        r1, c1 = int(rng.integers(r0 + 1, shape[1] + 1)), int(rng.integers(c0 + 1, shape[2] + 1))
        x, xd = x[:, :, r0:r1, c0:c1], xd[:, :, r0:r1, c0:c1]
    desc = "datasets robust %s %s x %s crop=%d perc=(%g, %g)" % (kind, nb, tuple(x.shape[1:]), crop, lo, top)
    out, perc = K.robust_norm(xd, lo, top, batch_dims=1)
    for k in range(nb):
        ref, (t_min, t_max) = G.reference_robust_norm(x[k], lo, top)
        err = equal(out[k], ref, "item %d" % k)
        if err is None:
            err = equal(perc[k], torch.tensor([t_min, t_max]), "percentiles of item %d" % k)
        if err is not None:
            return desc, err
    if nb == 1:                                        # the CPU entry point: a CPU tensor comes back
        got = RobustNorm(lo, top)(x[0])
        err = "RobustNorm returned a device tensor" if got.is_cuda else equal(got, G.reference_robust_norm(x[0], lo, top)[0], "RobustNorm")
        if err is not None:
            return desc, err
    return desc, None


N_MOTION = [1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 1000, 8193, 16_383, 16_384, 16_385, 16_387, 32_767, 32_768, 32_769, 49_155,
            65_539, 150_001, 400_000]


def _motion_mag(M, model, params, x, y, t, p, img_size, sensor_size, center, p_scale):
    """Per plane and cell, the sum of |contribution| of the restatement's dIWE splat (|p| (|jx| + |jy|) on every corner):
    the magnitude term of `same` for the derivative images."""
    H, W = int(sensor_size[0]) + 1, int(sensor_size[1]) + 1
    dims = M.DIMS[model]
    out = np.zeros((dims, H, W))
    if len(t) == 0:
        return out
    with np.errstate(all="ignore"):
        xw, yw, jx, jy = M.warp(model, x, y, t, float(np.asarray(t, np.float64)[-1]), params, center)
        keep = (xw > 0) & (xw <= img_size[1]) & (yw > 0) & (yw <= img_size[0])
        xf, yf = xw.astype(np.float32), yw.astype(np.float32)
        keep &= (xf < W - 1) & (yf < H - 1)
        px, py = np.floor(xf[keep]).astype(np.int64), np.floor(yf[keep]).astype(np.int64)
        ap = np.abs(np.asarray(p, np.float64) * p_scale)[keep]
        ap = np.where(np.isfinite(ap), ap, 0.0)
        for i in range(dims):
            w = ap * (np.abs(jx[i][keep]) + np.abs(jy[i][keep]))
            for oy, ox in ((0, 0), (0, 1), (1, 0), (1, 1)):
                np.add.at(out[i], (py + oy, px + ox), w)
    return out


def _band_canvas(rng, planes):
    """(ch, cw) with the band count of evk_iwe_param_band_rows just under / at / just over 16 x planes, or with a last band
    of one row."""
    cw = int(rng.integers(max(520, 2), min(1301, 40960 // planes) + 1))
    rows = 40960 // (planes * cw)
    cap = 16 * planes
    k = str(rng.choice(["at", "over", "under", "one_row"]))
    ch = {"at": cap * rows, "over": cap * rows + 1, "under": (cap - 1) * rows + 1,
          "one_row": int(rng.integers(1, cap)) * rows + 1}[k]
    return max(ch, 2), cw, k


def case_motion(rng):
    """pure_rotation_warp / xyztheta_warp (evk_warps.hip: the fused IWE in the LDS-band and direct kernels, the plane gradient
    sums) against tests/_motion_models_np.py: sensors from 2 x 2 to 1300 x 800 and band counts around the 16 x planes cap,
    n around the 16 384-event chunk and tiny, columns as numpy float64, from_arrays f32 / f64 / relative_time (epoch
    stamps), from_native, misaligned .slice() views and small device slices (the scalar loads), .scaled(f), EVK_IMPL
    auto / direct, parameters from zero to large, a few NaN / inf coordinates, times and polarities."""
    M = _t("_motion_models_np")
    from event_utils_amd import DeviceEvents
    from event_utils_amd.contrast_max import objectives as O
    model = str(rng.choice([M.ROTATION, M.XYZTHETA]))
    dims = M.DIMS[model]
    grad, pol = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    planes = 1 + dims if grad else 1
    geo = "random"
    if rng.random() < 0.3:
        ch, cw, geo = _band_canvas(rng, planes)
        ss = (ch - 1, cw - 1)
    else:
        ss = (int(rng.integers(1, 800)), int(rng.integers(1, 1300)))
    H, W = ss
    img_size = ss if rng.random() < 0.6 else (max(1, H + int(rng.integers(-10, 10))), max(1, W + int(rng.integers(-10, 10))))
    n = int(rng.choice(N_MOTION))
    kind = str(rng.choice(["numpy", "f32", "f64", "relative", "native", "slice", "small_dev"]))
    if kind == "small_dev":
        n = min(n, 1023)
    scale = float(rng.choice([1.0, 1.0, 100.0, 0.5, -1.0]))
    impl = str(rng.choice(["auto", "auto", "direct"]))
    T = float(rng.choice([0.01, 0.1, 1.0]))
    x, y = rng.uniform(-5, W + 5, n), rng.uniform(-5, H + 5, n)
    if kind == "native":
        x, y = np.floor(x), np.floor(y)
    t = np.sort(rng.uniform(0, T, n))
    p = (rng.integers(0, 2, n) * 2 - 1).astype(np.float64)
    if rng.random() < 0.3:
        p = rng.integers(-3, 4, n) * 0.5
    ps = float(rng.choice([0.0, 1.0, 10.0, 300.0]))
    if model == M.ROTATION:
        q = np.array([rng.uniform(-W, 2 * W), rng.uniform(-H, 2 * H), rng.normal() * float(rng.choice([0.0, 0.1, 3.0, 60.0]))])
    else:
        q = np.array([rng.normal() * ps, rng.normal() * ps, rng.normal() * ps / 100, rng.normal() * ps / 100])
    center = (0.0, 0.0) if model == M.ROTATION else (float(rng.uniform(0, W)), float(rng.uniform(0, H)))
    bad = n > 8 and kind in ("numpy", "f32", "f64", "slice") and rng.random() < 0.1
    if bad:
        k = rng.integers(0, n - 1, 3)
        x[k[0]] = float(rng.choice([np.nan, np.inf, -np.inf]))
        t[k[1]] = float(rng.choice([np.nan, np.inf]))
        p[k[2]] = np.nan
    if kind in ("f32", "slice", "small_dev", "relative"):
        x, y, p = (a.astype(np.float32).astype(np.float64) for a in (x, y, p))
        if kind != "relative":
            t = t.astype(np.float32).astype(np.float64)
    desc = "motion %s grad=%d pol=%d sensor=%s img=%s (%s) n=%d %s scale=%g impl=%s q=%s bad=%d" % (
        model, grad, pol, ss, img_size, geo, n, kind, scale, impl, np.array2string(q, precision=3), bad)
    # what the kernels see, and the restatement's float64 inputs
    xr, yr, tr, pr = x, y, t, p
    if kind == "numpy":
        src = (x, y, t, p)
    elif kind in ("f32", "f64"):
        src = (DeviceEvents.from_arrays(x, y, t, p, precision=kind), None, None, None)
    elif kind == "relative":
        te = 1.6e9 + t
        src = (DeviceEvents.from_arrays(x, y, te, p, relative_time=True), None, None, None)
        tr = (te - te[-1]).astype(np.float32).astype(np.float64) if src[0].t_offset != 0.0 else te
    elif kind == "native":
        pu = (p > 0).astype(np.uint8)
        src = (DeviceEvents.from_native(x.astype(np.int16), y.astype(np.int16), t, pu), None, None, None)
        tr = (t - t[0]).astype(np.float32).astype(np.float64)
        pr = pu * 2.0 - 1.0
    elif kind == "slice":
        off = int(rng.integers(1, 4))
        pad = lambda a: np.concatenate([rng.uniform(0, 1, off), a, rng.uniform(0, 1, 5)]).astype(np.float32)     # noqa: E731
        base = DeviceEvents.from_arrays(pad(x), pad(y), pad(t), pad(p), precision="f32")
        src = (base.slice(off, off + n), None, None, None)
    else:
        src = (DeviceEvents.from_arrays(*[_dev(rng, a.astype(np.float32), sliced=True) for a in (x, y, t, p)]), None, None, None)
    if scale != 1.0:
        ev = src[0] if isinstance(src[0], DeviceEvents) else DeviceEvents.from_arrays(*src)
        src = (ev.scaled(scale), None, None, None)
    w = E.pure_rotation_warp() if model == M.ROTATION else E.xyztheta_warp(center=center)
    os.environ["EVK_IMPL"] = impl
    try:
        with np.errstate(all="ignore"):
            ri, rd = M.iwe(model, q, xr, yr, tr, pr, img_size, ss, use_polarity=pol, compute_gradient=grad, center=center, p_scale=scale)
            mi, _ = M.iwe(model, q, xr, yr, tr, np.where(np.isfinite(pr), pr, 0.0), img_size, ss, use_polarity=False,
                          compute_gradient=False, center=center, p_scale=scale)
        iwe, diwe = E.get_iwe(q, *src, w, img_size, compute_gradient=grad, use_polarity=pol, sensor_size=ss)
        err = same(iwe, ri, mi, "iwe")
        if err is None and grad:
            if diwe is None or diwe.shape != rd.shape:
                return desc, "d_iwe %s vs %s" % (None if diwe is None else diwe.shape, rd.shape)
            dm = _motion_mag(M, model, q, xr, yr, tr, pr, img_size, ss, center, scale)
            err = same(diwe, rd, dm, "d_iwe")
        if err is not None or not (grad and min(ss) >= 2):
            return desc, err
        # objectives: value and gradient over the dims planes from one pass, and one other objective's gradient
        sigma = float(rng.choice([0.0, 1.0, 2.5]))
        o = E.variance_objective()
        o.sensor_size = ss
        o.reference_exact = bool(rng.integers(0, 2))
        f, g = o.evaluate_function_and_gradient(q, *src, w, img_size, sigma)
        with np.errstate(all="ignore"):
            ri, rd = M.iwe(model, q, xr, yr, tr, pr, img_size, ss, use_polarity=o.use_polarity, center=center, p_scale=scale)
            fr, gr = M.variance_f(ri, sigma), M.variance_grad(ri, rd, sigma, o.reference_exact)
            # magnitudes: the variance and its gradient summed from |terms| (|a - mean| |d_i|, |a|^2)
            a, d = M.blurred(ri, rd, sigma, o.reference_exact, not o.reference_exact)
            am = np.abs(a - a.mean())
            dmag = _motion_mag(M, model, q, xr, yr, tr, pr, img_size, ss, center, scale)
            _, dmag = M.blurred(ri, dmag, sigma, o.reference_exact, not o.reference_exact)
            amag = M.blurred(mi, dmag, sigma, False, not o.reference_exact)[0]
            gmag = np.array([np.mean(2.0 * (am * dmag[i] + amag * np.abs(d[i]))) for i in range(dims)])
        desc += " sigma=%g exact=%d" % (sigma, o.reference_exact)
        err = same(np.array([f]), np.array([fr]), np.array([2.0 * np.mean(np.square(amag))]), "variance", 1e-6) or \
            same(g, gr, gmag, "variance gradient", 1e-6)
        if err is not None:
            return desc, err
        oo = O.sos_objective() if rng.random() < 0.5 else O.rms_objective()
        oo.sensor_size = ss
        s = oo.default_blur
        g2 = np.asarray(oo.evaluate_gradient(q, *src, w, img_size, s), np.float64)
        with np.errstate(all="ignore"):
            ri, rd = M.iwe(model, q, xr, yr, tr, pr, img_size, ss, use_polarity=True, center=center, p_scale=scale)
            gr2 = -2.0 * M.gradsums(ri, rd, s, lambda v: v, False)[0] / ri.size
            a, _ = M.blurred(ri, rd, s, True, False)
            _, dmag = M.blurred(ri, _motion_mag(M, model, q, xr, yr, tr, pr, img_size, ss, center, scale), s, True, False)
            amag = M.blurred(mi, mi[None], s, True, False)[0]
            gm2 = np.array([2.0 * np.sum(amag * dmag[i]) / ri.size for i in range(dims)])
        return desc, same(g2, gr2, gm2, oo.name + " gradient", 1e-6)
    except Exception as e:  # noqa: BLE001
        return desc, "raised %s: %s" % (type(e).__name__, e)
    finally:
        os.environ.pop("EVK_IMPL", None)


# ---- the 8-plane-stack models and the average-timestamp objective ---------------------------------------------------------
# Each kind is split into *_inputs(rng), which draws the whole case on the host (no GPU: tests/test_cpu_fuzz_inputs.py checks
# what the generators cover from the restatements alone), and the comparison.

COLUMN_KINDS = ("numpy", "f32", "f64", "relative", "native", "slice", "small_dev")
EPOCH = 1.6e9 + 0.25       # the absolute stamps of the 'relative' kind (not a float32 value)


def _lib_geometry():
    from event_utils_amd import _lib
    return _lib, _lib.lib()


def _f32_values(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def _f32_exact(cols):
    """DeviceEvents.from_arrays' 'auto' rule: float32 columns when every value survives the conversion (NaN does not)."""
    with np.errstate(all="ignore"):
        return all(np.array_equal(_f32_values(a), np.asarray(a, np.float64)) for a in cols)


def _column_plan(rng, kind, x, y, t, p):
    """Host half of a column kind: the arrays to hand over ('cols'), the random choices of the device half, and what the
    kernels then see -- 'ref' = (x, y, t, p) for the restatement (t in the device column's dtype: float32 columns form tau
    in float32), 't_offset' (absolute time of the column's zero) and 'f32' (whether the device columns are float32)."""
    n = len(t)
    plan = {"kind": kind, "cols": (x, y, t, p), "t_offset": 0.0}
    xr, yr, tr, pr = x, y, t, p
    if kind in ("numpy", "f64"):
        f32 = kind == "numpy" and _f32_exact((x, y, t, p))
    elif kind in ("f32", "slice", "small_dev"):
        f32 = True
        if kind == "slice":
            plan["off"] = int(rng.integers(1, 4))
            plan["pads"] = [(rng.uniform(0, 1, plan["off"]), rng.uniform(0, 1, 5)) for _ in range(4)]
        elif kind == "small_dev":
            plan["offs"] = [(int(rng.integers(1, 4)), int(rng.integers(0, 5))) for _ in range(4)]
    elif kind == "relative":
        te = EPOCH + t
        plan["cols"] = (x, y, te, p)
        f32 = True                                     # (x, y, p are float32 values in this kind)
        if _f32_exact((te,)):
            tr = te
        else:
            plan["t_offset"] = float(te[-1])
            tr = _f32_values(te - te[-1])
    else:                                              # native: int16 pixels, float64 stamps kept as (float)(t - t[0]), uint8 p
        pu = (p > 0).astype(np.uint8)
        plan["cols"] = (x.astype(np.int16), y.astype(np.int16), t, pu)
        plan["t_offset"] = float(t[0]) if n else 0.0
        tr = _f32_values(t - t[0]) if n else t
        pr = pu * 2.0 - 1.0
        f32 = True
    plan["f32"] = bool(f32)
    plan["ref"] = (xr, yr, np.asarray(tr, np.float32 if f32 else np.float64), pr)
    return plan


def _device_source(plan, scale):
    """Device half of a column kind -> (xs, ys, ts, ps) as the public calls take them."""
    from event_utils_amd import DeviceEvents
    kind, (x, y, t, p) = plan["kind"], plan["cols"]
    if kind == "numpy":
        src = (x, y, t, p)
    elif kind in ("f32", "f64"):
        src = (DeviceEvents.from_arrays(x, y, t, p, precision=kind), None, None, None)
    elif kind == "relative":
        src = (DeviceEvents.from_arrays(x, y, t, p, relative_time=True), None, None, None)
    elif kind == "native":
        src = (DeviceEvents.from_native(x, y, t, p), None, None, None)
    elif kind == "slice":
        off, n = plan["off"], len(t)
        padded = [np.concatenate([a, c, b]).astype(np.float32) for c, (a, b) in zip((x, y, t, p), plan["pads"])]
        src = (DeviceEvents.from_arrays(*padded, precision="f32").slice(off, off + n), None, None, None)
    else:
        cols = []
        for a, (off, tail) in zip((x, y, t, p), plan["offs"]):
            buf = torch.zeros(off + len(a) + tail, dtype=torch.float32, device="cuda")
            buf[off:off + len(a)] = torch.from_numpy(a.astype(np.float32)).cuda()
            cols.append(buf[off:off + len(a)])
        src = (DeviceEvents.from_arrays(*cols), None, None, None)
    if scale != 1.0:
        ev = src[0] if isinstance(src[0], DeviceEvents) else DeviceEvents.from_arrays(*src)
        src = (ev.scaled(scale), None, None, None)
    if isinstance(src[0], DeviceEvents) and src[0].t_offset != plan["t_offset"]:
        raise AssertionError("fuzz case: t_offset %r, planned %r" % (src[0].t_offset, plan["t_offset"]))
    if isinstance(src[0], DeviceEvents) and (src[0].dtype == torch.float32) != plan["f32"]:
        raise AssertionError("fuzz case: device columns %s, planned f32=%d" % (src[0].dtype, plan["f32"]))
    return src


def _band_canvas8(rng, model_id, planes):
    """(ch, cw, class) from evk_iwe_param_band_rows itself: the band count just under / at / just over 16 x planes (over: the
    direct kernel takes the canvas), or a last band of one row."""
    _lib, L = _lib_geometry()
    flags = _lib.EVK_IWE_GRADIENT if planes > 1 else 0
    cw = int(rng.integers(520, min(1301, 40960 // planes) + 1))
    rows = L.evk_iwe_param_band_rows(model_id, flags, 128, cw)     # 128 rows: taller than a band, well under the cap of bands
    cap = 16 * planes
    k = str(rng.choice(["at", "over", "under", "one_row"]))
    ch = {"at": cap * rows, "over": cap * rows + 1, "under": (cap - 1) * rows + 1,
          "one_row": int(rng.integers(1, cap)) * rows + 1}[k]
    ch = max(ch, 2)
    got = L.evk_iwe_param_band_rows(model_id, flags, ch, cw)
    if (got == 0) != (k == "over") or (got and got != min(rows, ch)):
        raise AssertionError("fuzz case: band geometry %s: rows %d for %dx%d planes %d" % (k, got, ch, cw, planes))
    return ch, cw, k


def motion8_inputs(rng):
    """angular_velocity_warp / planar_flow_warp: everything case_motion varies, and random intrinsics (fx != fy, the principal
    point on or somewhat off the sensor, focal lengths from 0.3 to 4 sensor widths), rotations that in 30 % of the ANGVEL
    cases ('behind') carry events behind the camera, planar parameters from all-zero through PF_TRUTH-sized to large linear
    terms with the quadratic ones scaled to the sensor, a random centre."""
    M = _t("_motion_models8_np")
    from event_utils_amd import _lib
    model = str(rng.choice([M.ANGVEL, M.PLANAR]))
    dims = M.DIMS[model]
    model_id = _lib.EVK_WARP_ANGULAR_VELOCITY if model == M.ANGVEL else _lib.EVK_WARP_PLANAR_FLOW
    grad, pol = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    planes = 1 + dims if grad else 1
    geo = "random"
    if rng.random() < 0.3:
        ch, cw, geo = _band_canvas8(rng, model_id, planes)
        ss = (ch - 1, cw - 1)
    else:
        ss = (int(rng.integers(1, 800)), int(rng.integers(1, 1300)))
    H, W = ss
    img_size = ss if rng.random() < 0.6 else (max(1, H + int(rng.integers(-10, 10))), max(1, W + int(rng.integers(-10, 10))))
    n = int(rng.choice(N_MOTION))
    kind = str(rng.choice(COLUMN_KINDS))
    if kind == "small_dev":
        n = min(n, 1023)
    scale = float(rng.choice([1.0, 1.0, 100.0, 0.5, -1.0]))
    impl = str(rng.choice(["auto", "auto", "direct"]))
    T = float(rng.choice([0.01, 0.1, 1.0]))
    mx, my = min(5.0, 0.05 * W + 0.5), min(5.0, 0.05 * H + 0.5)
    x, y = rng.uniform(-mx, W + mx, n), rng.uniform(-my, H + my, n)
    if kind == "native":
        x, y = np.floor(x), np.floor(y)
    t = np.sort(rng.uniform(0, T, n))
    p = (rng.integers(0, 2, n) * 2 - 1).astype(np.float64)
    if rng.random() < 0.3:
        p = rng.integers(-3, 4, n) * 0.5
    K, aim = M.K_DEFAULT, "none"
    center = (0.0, 0.0)
    if model == M.ANGVEL:
        f = W * float(np.exp(rng.uniform(np.log(0.3), np.log(4.0))))
        K = np.array([[f, 0.0, rng.uniform(-0.2 * W, 1.2 * W)], [0.0, f * rng.uniform(0.7, 1.4), rng.uniform(-0.2 * H, 1.2 * H)],
                      [0.0, 0.0, 1.0]])
        axis = rng.normal(size=3)
        aim = "behind" if rng.random() < 0.3 else "front"
        if aim == "behind":          # a rotation of 1.5 .. 3 rad over the stream about an axis near the image plane
            axis[2] *= 0.1
            angle = float(rng.uniform(1.5, 3.0))
        else:
            angle = float(rng.choice([0.0, 0.02, 0.1, 0.4]))
        q = axis / np.linalg.norm(axis) * angle / T
    else:
        center = (float(rng.uniform(0, W)), float(rng.uniform(0, H)))
        # displacements over the stream: translation in pixels, linear terms per pixel, quadratic ones per pixel^2 of the sensor
        tr_px, lin = float(rng.choice([0.0, 3.0, 30.0])), float(rng.choice([0.0, 0.02, 0.06, 0.6]))
        half = 0.5 * max(W, H, 2)
        q = np.array([rng.normal() * tr_px, rng.normal() * lin, rng.normal() * lin, rng.normal() * tr_px, rng.normal() * lin,
                      rng.normal() * lin, rng.normal() * lin / half, rng.normal() * lin / half]) / T
    bad = bool(n > 8 and kind in ("numpy", "f32", "f64", "slice") and rng.random() < 0.1)
    if bad:
        k = rng.integers(0, n - 1, 3)
        x[k[0]] = float(rng.choice([np.nan, np.inf, -np.inf]))
        t[k[1]] = float(rng.choice([np.nan, np.inf]))
        p[k[2]] = np.nan
    if kind in ("f32", "slice", "small_dev", "relative"):
        x, y, p = (_f32_values(a) for a in (x, y, p))
        if kind != "relative":
            t = _f32_values(t)
    plan = _column_plan(rng, kind, x, y, t, p)
    sigma = float(rng.choice([0.0, 1.0, 2.5]))
    exact_blur, other = bool(rng.integers(0, 2)), str(rng.choice(["sos", "rms"]))
    desc = "motion8 %s grad=%d pol=%d sensor=%s img=%s (%s) n=%d %s scale=%g impl=%s q=%s aim=%s bad=%d" % (
        model, grad, pol, ss, img_size, geo, n, kind, scale, impl, np.array2string(q, precision=3), aim, bad)
    if model == M.ANGVEL:
        desc += " K=(%.1f, %.1f, %.1f, %.1f)" % (K[0, 0], K[1, 1], K[0, 2], K[1, 2])
    else:
        desc += " center=(%.1f, %.1f)" % center
    return dict(desc=desc, model=model, dims=dims, grad=grad, pol=pol, planes=planes, geo=geo, ss=ss, img_size=img_size, n=n,
                kind=kind, scale=scale, impl=impl, q=q, K=K, center=center, aim=aim, bad=bad, plan=plan, sigma=sigma,
                exact_blur=exact_blur, other=other)


def motion8_reference(c, use_polarity=None, compute_gradient=None):
    """The restatement's (iwe, d_iwe) of a motion8 case, and the IWE of |p| (the magnitudes of `same`)."""
    M = _t("_motion_models8_np")
    xr, yr, tr, pr = c["plan"]["ref"]
    tr = np.asarray(tr, np.float64)
    pol = c["pol"] if use_polarity is None else use_polarity
    grad = c["grad"] if compute_gradient is None else compute_gradient
    with np.errstate(all="ignore"):
        ri, rd = M.iwe(c["model"], c["q"], xr, yr, tr, pr, c["img_size"], c["ss"], use_polarity=pol, compute_gradient=grad,
                       center=c["center"], camera_matrix=c["K"], p_scale=c["scale"])
        mi, _ = M.iwe(c["model"], c["q"], xr, yr, tr, np.where(np.isfinite(pr), pr, 0.0), c["img_size"], c["ss"], use_polarity=False,
                      compute_gradient=False, center=c["center"], camera_matrix=c["K"], p_scale=c["scale"])
    return ri, rd, mi


def _motion8_mag(M, c):
    """_motion_mag for the models with a camera matrix."""
    xr, yr, tr, pr = c["plan"]["ref"]
    tr = np.asarray(tr, np.float64)
    H, W = int(c["ss"][0]) + 1, int(c["ss"][1]) + 1
    out = np.zeros((c["dims"], H, W))
    if len(tr) == 0:
        return out
    with np.errstate(all="ignore"):
        xw, yw, jx, jy = M.warp(c["model"], xr, yr, tr, float(tr[-1]), c["q"], c["center"], c["K"])
        keep = (xw > 0) & (xw <= c["img_size"][1]) & (yw > 0) & (yw <= c["img_size"][0])
        xf, yf = xw.astype(np.float32), yw.astype(np.float32)
        keep &= (xf < W - 1) & (yf < H - 1)
        px, py = np.floor(xf[keep]).astype(np.int64), np.floor(yf[keep]).astype(np.int64)
        ap = np.abs(np.asarray(pr, np.float64) * c["scale"])[keep]
        ap = np.where(np.isfinite(ap), ap, 0.0)
        for i in range(c["dims"]):
            w = ap * (np.abs(jx[i][keep]) + np.abs(jy[i][keep]))
            for oy, ox in ((0, 0), (0, 1), (1, 0), (1, 1)):
                np.add.at(out[i], (py + oy, px + ox), w)
    return out


def case_motion8(rng):
    """angular_velocity_warp / planar_flow_warp (evk_warps.hip at up to 9 planes, evk_warp_models.h) against
    tests/_motion_models8_np.py: motion8_inputs, compared as case_motion compares."""
    M = _t("_motion_models8_np")
    from event_utils_amd.contrast_max import objectives as O
    c = motion8_inputs(rng)
    desc, model, q, ss, img_size, grad, dims, scale = (c[k] for k in ("desc", "model", "q", "ss", "img_size", "grad", "dims", "scale"))
    center, K = c["center"], c["K"]
    xr, yr, tr, pr = c["plan"]["ref"]
    tr = np.asarray(tr, np.float64)
    os.environ["EVK_IMPL"] = c["impl"]
    try:
        src = _device_source(c["plan"], scale)
        w = E.angular_velocity_warp(K) if model == M.ANGVEL else E.planar_flow_warp(center=center)
        ri, rd, mi = motion8_reference(c)
        iwe, diwe = E.get_iwe(q, *src, w, img_size, compute_gradient=grad, use_polarity=c["pol"], sensor_size=ss)
        err = same(iwe, ri, mi, "iwe")
        if err is None and grad:
            if diwe is None or diwe.shape != rd.shape:
                return desc, "d_iwe %s vs %s" % (None if diwe is None else diwe.shape, rd.shape)
            err = same(diwe, rd, _motion8_mag(M, c), "d_iwe")
        if err is not None or not (grad and min(ss) >= 2):
            return desc, err
        sigma = c["sigma"]
        o = E.variance_objective()
        o.sensor_size = ss
        o.reference_exact = c["exact_blur"]
        f, g = o.evaluate_function_and_gradient(q, *src, w, img_size, sigma)
        kw = dict(center=center, camera_matrix=K, p_scale=scale)
        with np.errstate(all="ignore"):
            ri, rd = M.iwe(model, q, xr, yr, tr, pr, img_size, ss, use_polarity=o.use_polarity, **kw)
            fr, gr = M.variance_f(ri, sigma), M.variance_grad(ri, rd, sigma, o.reference_exact)
            a, d = M.blurred(ri, rd, sigma, o.reference_exact, not o.reference_exact)
            am = np.abs(a - a.mean())
            dmag0 = _motion8_mag(M, c)
            _, dmag = M.blurred(ri, dmag0, sigma, o.reference_exact, not o.reference_exact)
            amag = M.blurred(mi, dmag, sigma, False, not o.reference_exact)[0]
            gmag = np.array([np.mean(2.0 * (am * dmag[i] + amag * np.abs(d[i]))) for i in range(dims)])
        desc += " sigma=%g exact=%d" % (sigma, o.reference_exact)
        err = same(np.array([f]), np.array([fr]), np.array([2.0 * np.mean(np.square(amag))]), "variance", 1e-6) or \
            same(g, gr, gmag, "variance gradient", 1e-6)
        if err is not None:
            return desc, err
        oo = O.sos_objective() if c["other"] == "sos" else O.rms_objective()
        oo.sensor_size = ss
        s = oo.default_blur
        g2 = np.asarray(oo.evaluate_gradient(q, *src, w, img_size, s), np.float64)
        with np.errstate(all="ignore"):
            ri, rd = M.iwe(model, q, xr, yr, tr, pr, img_size, ss, use_polarity=True, **kw)
            gr2 = -2.0 * M.gradsums(ri, rd, s, lambda v: v, False)[0] / ri.size
            _, dmag = M.blurred(ri, dmag0, s, True, False)
            amag = M.blurred(mi, mi[None], s, True, False)[0]
            gm2 = np.array([2.0 * np.sum(amag * dmag[i]) / ri.size for i in range(dims)])
        return desc, same(g2, gr2, gm2, oo.name + " gradient", 1e-6)
    except Exception as e:  # noqa: BLE001
        return desc, "raised %s: %s" % (type(e).__name__, e)
    finally:
        os.environ.pop("EVK_IMPL", None)


N_ZHU_SMALL = [1, 2, 3, 5, 7, 63, 64, 65, 1000, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4097, 8193, 16_383, 16_384, 16_385,
               16_387, 32_767, 32_769, 49_155, 65_539]
N_ZHU_LARGE = [150_001, 400_000, 1_100_003]       # the last: more than kGatherBlocks (1024) workgroups of 4 x 256 events
ZHU_SIGMAS = (0.0, 1.0, None, 2.5, 9.0)            # None: the objective's default (2.0); 9: the wide blur
ZHU_SCALES = (1.0, 1.0, 100.0, 0.5, -1.0, 0.0)
# |tau| of every event: evk_tsobj.hip documents tau w in [-1, 1] for its fixed-point cells.  The 'unsorted' kind places the stream
# ends so that |tau| <= 1, up to the 1e-6 of tdiv: with reversed ends (tdiv < 0, |ts[-1] - ts[0]| >= 2e-3) the last event
# itself has tau = D / (D - 1e-6) <= 1.0005, which a cell's 31 integer bits hold as they hold 1.
ZHU_TAU_BOUND = 1.001


def _zhu_canvas(rng):
    """(ch, cw, class) from evk_tsimg_band_rows itself: the band count just under / at / just over the 24 x 4 cap (over: the
    direct kernel), a last band of one row, the width where exactly one row fits a band and the one above where none does."""
    _lib, L = _lib_geometry()
    k = str(rng.choice(["at", "over", "under", "one_row", "one_row_fits", "no_row_fits"]))
    if k in ("one_row_fits", "no_row_fits"):
        cw = 2
        while L.evk_tsimg_band_rows(0, 2, cw * 2) > 0:        # the widest canvas a band still holds a row of
            cw *= 2
        lo, hi = cw, cw * 2
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if L.evk_tsimg_band_rows(0, 2, mid) > 0 else (lo, mid)
        cw = lo if k == "one_row_fits" else hi
        ch = int(rng.integers(2, 41))
        ok = L.evk_tsimg_band_rows(0, ch, cw) == (1 if k == "one_row_fits" else 0)
    else:
        cw = int(rng.integers(520, 1302))
        rows = L.evk_tsimg_band_rows(0, 128, cw)              # 128 rows: taller than a band, under the cap of bands
        cap = 24 * 4
        ch = {"at": cap * rows, "over": cap * rows + 1, "under": (cap - 1) * rows + 1,
              "one_row": int(rng.integers(1, cap)) * rows + 1}[k]
        got = L.evk_tsimg_band_rows(0, ch, cw)
        ok = rows > 0 and (got == 0) == (k == "over") and (got == 0 or got == rows)
    if not ok:
        raise AssertionError("fuzz case: timestamp band geometry %s at %dx%d" % (k, ch, cw))
    return ch, cw, k


def _zhu_times(rng, n, tk):
    """times(): float32 values.  'unsorted': the interior in any order, and the two ends placed so that
    tau = (t - ts[0]) / (ts[-1] - ts[0] + 1e-6) stays within ZHU_TAU_BOUND -- the range evk_tsobj.hip documents for its
    fixed-point cells: ends = min / max; both beyond the stream; reversed (tdiv < 0); or ts[0] inside the stream and ts[-1] a
    whole span above it (negative tau)."""
    t = times(rng, n, tk).astype(np.float64)
    how = "-"
    if tk == "unsorted" and n >= 2:
        how = str(rng.choice(["minmax", "beyond", "reversed", "inside"]))
        lo, hi = float(t[1:-1].min()) if n > 2 else 0.0, float(t[1:-1].max()) if n > 2 else 1.0
        span, d = hi - lo, float(rng.uniform(0.001, 0.2))
        if how == "minmax":
            t[0], t[-1] = lo, hi
        elif how == "beyond":
            t[0], t[-1] = lo - d, hi + d
        elif how == "reversed":
            t[0], t[-1] = hi + d, lo - d
        else:
            t[0] = lo + 0.5 * span
            t[-1] = t[0] + span + d
        t = _f32_values(t)
    return t, how


def zhu_inputs(rng):
    """One case of the average-timestamp objective, drawn on the host: model (all five, or a plugin linear flow), canvas
    (random 2 x 2 .. 1300 x 800 or from evk_tsimg_band_rows), obj.sensor_size equal to / above / below img_size, n (mostly
    small), column kind, .scaled factor, polarity kind, time kind, t_ref mode, blur, EVK_IMPL, a few NaN / inf injections."""
    Z = _t("_zhu_np")
    M8 = _t("_motion_models8_np")
    route = "plugin" if rng.random() < 0.15 else "fused"
    model = Z.LINVEL if route == "plugin" else str(rng.choice(Z.MODELS))
    # one case in ten: integer pixels under zero flow on an image smaller than the canvas, so that events sit exactly on
    # x' = W and y' = H of the bounds mask (counted: x' <= W) without the inner clip taking them
    border = bool(rng.random() < 0.1)
    if border:
        route, model = "fused", str(rng.choice([Z.LINVEL, Z.XYZTHETA, Z.PLANAR]))
    dims = Z.DIMS[model]
    if rng.random() < 0.45:
        ch, cw, geo = _zhu_canvas(rng)
    else:
        geo = "random"
        ch, cw = (int(rng.integers(2, 12)), int(rng.integers(2, 12))) if rng.random() < 0.15 else \
            (int(rng.integers(2, 802)), int(rng.integers(2, 1302)))
    ss = (ch - 1, cw - 1)
    H, W = ss
    size_mode = str(rng.choice(["equal", "equal", "img_smaller", "img_larger"]))
    if border:
        size_mode = "img_smaller"
    if size_mode == "img_smaller" and min(H, W) < 2:
        size_mode = "equal"
    if size_mode == "equal":
        img_size = ss
    elif size_mode == "img_smaller":
        img_size = (max(1, H - int(rng.integers(1, 10))), max(1, W - int(rng.integers(1, 10))))
    else:
        img_size = (H + int(rng.integers(1, 10)), W + int(rng.integers(1, 10)))
    n = int(rng.choice(N_ZHU_LARGE if rng.random() < 0.06 else N_ZHU_SMALL))
    kind = str(rng.choice(COLUMN_KINDS))
    if kind == "small_dev":
        n = min(n, 1023)
    scale = float(rng.choice(ZHU_SCALES))
    impl = str(rng.choice(["auto", "auto", "direct"]))
    scene = str(rng.choice(["uniform", "uniform", "pixels", "blob"]))
    if border:
        scene, n, scale = "pixels", max(n, 1000 if kind != "small_dev" else 1), scale if scale != 0.0 else 1.0
    iw, ih = min(img_size[1], W), min(img_size[0], H)
    mx, my = min(3.0, 0.05 * iw + 0.5), min(3.0, 0.05 * ih + 0.5)
    x, y = rng.uniform(-mx, iw + mx, n), rng.uniform(-my, ih + my, n)
    if scene == "blob" and n > 8:
        hot = rng.random(n) < 0.6
        x[hot] = iw * 0.4 + rng.uniform(-1.5, 1.5, hot.sum())
        y[hot] = ih * 0.6 + rng.uniform(-1.5, 1.5, hot.sum())
    if scene == "pixels" or kind == "native":          # sensor events: integer pixels, the image's border rows included
        x, y = rng.integers(0, img_size[1] + 1, n).astype(np.float64), rng.integers(0, img_size[0] + 1, n).astype(np.float64)
    tk = str(rng.choice(["sorted", "sorted", "sorted", "const", "few", "ends", "unsorted", "unsorted"]))
    if border and tk == "const":
        tk = "sorted"
    t, ends = _zhu_times(rng, n, tk)
    if tk == "sorted" and kind in ("numpy", "f64", "relative", "native") and rng.random() < 0.6:
        t = np.sort(rng.uniform(3.0, 3.2, n))          # float64 stamps that are not float32 values
    pk = str(rng.choice(["pm1", "pm1", "pm1", "pos", "neg", "pm1z", "pm1z", "ints", "ints", "nan"]))
    if pk == "nan" and (kind == "native" or rng.random() < 0.4):
        pk = "pm1"
    p = (rng.integers(0, 2, n) * 2 - 1).astype(np.float64)
    if pk == "pos":
        p = np.ones(n)
    elif pk == "neg":
        p = -np.ones(n)
    elif pk == "pm1z":
        p = rng.integers(-1, 2, n).astype(np.float64)
    elif pk == "ints":
        p = rng.integers(-3, 4, n).astype(np.float64)
    elif pk == "nan":
        p[rng.integers(0, n, max(1, n // 50))] = np.nan
    span = float(np.ptp(t)) if n else 0.0
    T = span if span > 0 else 1.0
    t_lo, t_hi = (float(t.min()), float(t.max())) if n else (0.0, 0.0)
    tref_mode = str(rng.choice(["none", "none", "inside", "outside"]))
    t_ref = None
    if tref_mode == "inside":
        t_ref = float(rng.uniform(t_lo, t_hi)) if t_hi > t_lo else t_lo
    elif tref_mode == "outside":
        t_ref = t_hi + float(rng.uniform(0.0, 0.5)) * T if rng.random() < 0.5 else t_lo - float(rng.uniform(0.0, 0.5)) * T
    # parameters as displacements over the stream: zero (the events stay where they are), a few pixels, tens of pixels
    K, center, aim = M8.K_DEFAULT, (0.0, 0.0), "none"
    px_, lin = float(rng.choice([0.0, 0.0, 3.0, 30.0])), float(rng.choice([0.0, 0.02, 0.06, 0.3]))
    if model == Z.LINVEL:
        q = rng.normal(size=2) * px_ / T
    elif model == Z.ROTATION:
        q = np.array([rng.uniform(-W, 2 * W), rng.uniform(-H, 2 * H), rng.normal() * lin / T])
    elif model == Z.XYZTHETA:
        center = (float(rng.uniform(0, W)), float(rng.uniform(0, H)))
        q = np.array([rng.normal() * px_, rng.normal() * px_, rng.normal() * lin, rng.normal() * lin]) / T
    elif model == Z.ANGVEL:
        f = max(W, 2) * float(np.exp(rng.uniform(np.log(0.3), np.log(4.0))))
        K = np.array([[f, 0.0, rng.uniform(-0.2 * W, 1.2 * W)], [0.0, f * rng.uniform(0.7, 1.4), rng.uniform(-0.2 * H, 1.2 * H)],
                      [0.0, 0.0, 1.0]])
        axis = rng.normal(size=3)
        aim = "behind" if rng.random() < 0.2 else "front"
        if aim == "behind":
            axis[2] *= 0.1
            angle = float(rng.uniform(1.5, 3.0))
        else:
            angle = float(rng.choice([0.0, 0.02, 0.1, 0.4]))
        q = axis / np.linalg.norm(axis) * angle / T
    else:
        center = (float(rng.uniform(0, W)), float(rng.uniform(0, H)))
        half = 0.5 * max(W, H, 2)
        q = np.array([rng.normal() * px_, rng.normal() * lin, rng.normal() * lin, rng.normal() * px_, rng.normal() * lin,
                      rng.normal() * lin, rng.normal() * lin / half, rng.normal() * lin / half]) / T
    if border or ((scene == "pixels" or kind == "native") and rng.random() < 0.5):
        q = q * 0.0 if model != Z.ROTATION else q * np.array([1.0, 1.0, 0.0])       # zero flow: integer x' = x, the border x' = W too
    # NaN / inf among the coordinates and the INTERIOR time stamps.  (A NaN at ts[0] or ts[-1] makes tau NaN for every event:
    # outside the range the fixed-point cells are documented for, and not drawn -- profiles/fuzz_motion8_zhu.txt.)
    bad = bool(n > 8 and kind in ("numpy", "f32", "f64", "slice") and rng.random() < 0.06)
    if bad:
        k = rng.integers(1, n - 1, 3)
        x[k[0]] = float(rng.choice([np.nan, np.inf, -np.inf]))
        y[k[2]] = np.nan
        t[k[1]] = float(rng.choice([np.nan, np.inf]))
    if kind in ("f32", "slice", "small_dev", "relative"):
        x, y, p = (_f32_values(a) for a in (x, y, p))
        if kind != "relative":
            t = _f32_values(t)
    epoch = False
    if kind in ("numpy", "f64"):
        # half of the float64 kinds carry absolute epoch stamps (what the h5 / rosbag readers deliver): float64 device columns
        # whose normalised time only float64 arithmetic can form
        sigma = ZHU_SIGMAS[int(rng.integers(0, len(ZHU_SIGMAS)))]
        epoch = bool(rng.random() < 0.5)
        if epoch:
            t = t + EPOCH
        plan = _column_plan(rng, kind, x, y, t, p)
    else:
        plan = _column_plan(rng, kind, x, y, t, p)
        sigma = ZHU_SIGMAS[int(rng.integers(0, len(ZHU_SIGMAS)))]
    if route == "plugin":        # warp() is handed float64 columns and tau is formed in float64 whatever the stored dtype
        plan["ref"] = plan["ref"][:2] + (np.asarray(plan["ref"][2], np.float64),) + plan["ref"][3:]
    if tref_mode != "none" and (kind == "relative" or epoch):
        t_ref += EPOCH                                   # .t_ref is an absolute time
    desc = "zhu %s %s sensor=%s img=%s (%s, %s) n=%d %s scale=%g impl=%s %s p=%s t=%s/%s t_ref=%s sigma=%s q=%s aim=%s bad=%d" % (
        route, model, ss, img_size, geo, size_mode, n, kind, scale, impl, scene, pk, tk, ends, tref_mode, sigma,
        np.array2string(q, precision=3), aim, bad) + (" epoch" if epoch else "")
    return dict(desc=desc, epoch=epoch, route=route, model=model, dims=dims, geo=geo, ss=ss, img_size=img_size, size_mode=size_mode, n=n,
                kind=kind, scale=scale, impl=impl, scene=scene, pk=pk, tk=tk, ends=ends, tref_mode=tref_mode, t_ref=t_ref,
                q=q, K=K, center=center, aim=aim, bad=bad or pk == "nan", plan=plan, sigma=sigma)


def zhu_reference(c, f32_images=False):
    """The restatement of a zhu case from ONE pass over its events: planes, their magnitudes (the splat of |tau| w and w),
    the two images, the loss and its gradient with the gradient's magnitudes (sums of |terms|), the number of counted events.
    f32_images: the planes and the adjoint images rounded to float32, as the kernels store them (the CPU measure of what the
    comparison rule has to allow)."""
    Z = _t("_zhu_np")
    xr, yr, tr, pr = c["plan"]["ref"]
    ss, dims = c["ss"], c["dims"]
    shape = (ss[0] + 1, ss[1] + 1)
    sigma = 2.0 if c["sigma"] is None else c["sigma"]
    out = dict(planes=np.zeros((4,) + shape), mag=np.zeros((4,) + shape), loss=0.0, grad=np.zeros(dims), gmag=np.zeros(dims), counted=0)
    out["images"] = np.zeros((2,) + shape)
    if len(tr) == 0:
        return out
    t_ref = None if c["t_ref"] is None else c["t_ref"] - c["plan"]["t_offset"]
    with np.errstate(all="ignore"):
        ev, keep = Z._events(c["model"], c["q"], xr, yr, tr, np.asarray(pr, np.float64) * c["scale"], c["img_size"], ss, c["center"],
                             c["K"], True, t_ref)
        px, py, dx, dy, tau, pos, jx, jy = ev
        pl = Z._splat(shape, ev)
        mag = Z._splat(shape, (px, py, dx, dy, np.abs(tau), pos, jx, jy))
        if f32_images:
            pl = _f32_values(pl)
        out.update(planes=pl, mag=mag, images=Z.averages(pl), loss=Z.loss_of_planes(pl, sigma), counted=int(keep.sum()))
        g, gm = np.zeros(dims), np.zeros(dims)
        for sel, base in ((pos, 0), (~pos, 2)):
            Tp, Cp = pl[base], pl[base + 1]
            S = Z._blur(Z._blur(Tp / (1.0 + Cp), sigma), sigma)
            gT, gC = 2.0 * S / (1.0 + Cp), -2.0 * S * Tp / (1.0 + Cp) ** 2
            if f32_images:
                gT, gC = _f32_values(gT), _f32_values(gC)
            qx, qy, fx, fy = px[sel], py[sel], dx[sel], dy[sel]

            def slopes(img):
                a, b, cc, d = img[qy, qx], img[qy, qx + 1], img[qy + 1, qx], img[qy + 1, qx + 1]
                return (b - a) * (1.0 - fy) + (d - cc) * fy, (cc - a) * (1.0 - fx) + (d - b) * fx
            tx, ty = slopes(gT)
            cx, cy = slopes(gC)
            ta = tau[sel]
            g += jx[:, sel] @ (ta * tx + cx) + jy[:, sel] @ (ta * ty + cy)
            gm += np.abs(jx[:, sel]) @ (np.abs(ta * tx) + np.abs(cx)) + np.abs(jy[:, sel]) @ (np.abs(ta * ty) + np.abs(cy))
        out.update(grad=g, gmag=gm)
    return out


def _zhu_warp(c):
    Z = _t("_zhu_np")
    if c["route"] == "plugin":
        class plugin_flow(E.warp_function):
            """A user plugin: linear flow in whatever array type it is handed."""

            def __init__(self):
                E.warp_function.__init__(self, "plugin_flow", 2)

            def warp(self, xs, ys, ts, ps, t0, params, compute_grad=False):
                dt = ts - t0
                xo, yo = xs - dt * params[0], ys - dt * params[1]
                if not compute_grad:
                    return xo, yo, None, None
                z = dt * 0
                stack = torch.stack if isinstance(dt, torch.Tensor) else np.stack
                return xo, yo, stack([-dt, z]), stack([z, -dt])
        return plugin_flow()
    return {Z.LINVEL: lambda: E.linvel_warp(), Z.ROTATION: lambda: E.pure_rotation_warp(),
            Z.XYZTHETA: lambda: E.xyztheta_warp(center=c["center"]), Z.ANGVEL: lambda: E.angular_velocity_warp(c["K"]),
            Z.PLANAR: lambda: E.planar_flow_warp(center=c["center"])}[c["model"]]()


def _bits(a, b):
    a, b = np.atleast_1d(np.asarray(a, np.float64)), np.atleast_1d(np.asarray(b, np.float64))
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def case_zhu(rng):
    """zhu_timestamp_objective, get_timestamp_images and timestamp_planes_device (evk_tsobj.hip: the fixed-point band and
    direct splats, the post pass, the adjoint gather) against tests/_zhu_np.py with f32_coords=True: zhu_inputs, through the
    public calls.  Planes and images with `same` and the splat of |tau| w and w as magnitudes; loss and gradient with
    magf = 1e-6 and the restatement's sums of |terms|; the one-call value and gradient against the two separate calls,
    a second evaluation on the fused route and the band against the direct planes, bit for bit."""
    from event_utils_amd.contrast_max import objectives as O
    c = zhu_inputs(rng)
    desc, q, ss, img_size, sigma = (c[k] for k in ("desc", "q", "ss", "img_size", "sigma"))
    fused = c["route"] == "fused"
    os.environ["EVK_IMPL"] = c["impl"]
    try:
        r = zhu_reference(c)
        src = _device_source(c["plan"], c["scale"])
        w = _zhu_warp(c)
        if fused:
            ev = O._as_device_events(*src)
            band = O.timestamp_planes_device(q, ev, w, img_size, sensor_size=ss, t_ref=c["t_ref"]).cpu().numpy()
            direct = O.timestamp_planes_device(q, ev, w, img_size, sensor_size=ss, impl="direct", t_ref=c["t_ref"]).cpu().numpy()
            err = same(band, r["planes"], r["mag"], "planes") or same(direct, r["planes"], r["mag"], "direct planes")
            if err is None and not np.array_equal(band.view(np.uint32), direct.view(np.uint32)):
                err = "band and direct planes differ in %d cells" % int((band != direct).sum())
            if err is not None:
                return desc, err
        if c["t_ref"] is None:       # (get_timestamp_images takes no reference time)
            img = E.get_timestamp_images(q, *src, w, img_size, sensor_size=ss)
            err = same(img.cpu().numpy(), r["images"], np.stack([r["mag"][0] / (1.0 + r["mag"][1]), r["mag"][2] / (1.0 + r["mag"][3])]),
                       "images")
            if err is not None:
                return desc, err
        obj = E.zhu_timestamp_objective()
        obj.sensor_size, obj.t_ref = ss, c["t_ref"]
        f = obj.evaluate_function(q, *src, w, img_size, sigma)
        g = obj.evaluate_gradient(q, *src, w, img_size, sigma)
        f2, g2 = obj.evaluate_function_and_gradient(q, *src, w, img_size, sigma)
        err = same(np.array([f]), np.array([r["loss"]]), np.array([r["loss"]]), "loss", 1e-6) or \
            same(g, r["grad"], r["gmag"], "gradient", 1e-6)
        if err is not None:
            return desc, err
        if not (_bits(f, f2) and _bits(g, g2)):
            return desc, "the one-call value / gradient differ from the separate calls: %r %r vs %r %r" % (f, g, f2, g2)
        fb = obj.evaluate_function_batch([q, q * 0.5], *src, w, img_size, sigma)
        if not _bits(fb[0], f):
            return desc, "evaluate_function_batch %r vs %r" % (fb[0], f)
        if fused:
            f3, g3 = obj.evaluate_function_and_gradient(q, *src, w, img_size, sigma)
            if not (_bits(f, f3) and _bits(g, g3)):
                return desc, "a second evaluation gives other bits: %r %r vs %r %r" % (f, g, f3, g3)
        return desc, None
    except Exception as e:  # noqa: BLE001
        return desc, "raised %s: %s" % (type(e).__name__, e)
    finally:
        os.environ.pop("EVK_IMPL", None)


# ---- the per-pixel grouping family: denoise, tsurf, corners, planeflow, reconstruct ---------------------------------------------
# All five run on evk_group.h (order[], start[]) and evk_pred.h.  One generator draws the event stream of a case for all of them
# (group_stream: pure numpy); <kind>_inputs draws the parameters, <kind>_reference evaluates tests/_*_np.py on what the device
# holds, case_<kind> runs the public calls.  The comparison rules are those of the dedicated GPU test of each feature, restated
# below as functions that return a report; profiles/fuzz_grouping_kinds.txt.

GROUP_EVENT_KINDS = tuple(k for k in COLUMN_KINDS if k != "numpy")       # DeviceEvents, through _column_plan / _device_source
GROUP_KINDS = ("numpy", "tensor", "tensor_slice") + GROUP_EVENT_KINDS
GROUP_SCALES = (1.0, 100.0, 0.5, -1.0)
GROUP_SCENES = ("noise", "edge", "blobs", "square", "ties", "front", "hot")
GROUP_TIMES = ("ticks", "frac", "micro", "epoch", "f32", "i16", "i32", "i64", "const")
GROUP_FRACTIONAL = ("frac", "micro", "epoch", "f32")  # ('micro': float64 seconds within 10 us of zero -- differences of the order of the
#                                                      rounding residue of a window's double sums times 1e10, see planeflow_inputs)
GROUP_POLS = ("pm1", "pos", "neg", "pm1z", "ints", "bool")
GROUP_SENSORS = ("1x1", "1xW", "Hx1", "small", "thin", "around64", "random")
GROUP_SELECTS = ("none", "empty", "one", "repeats", "reversed", "list", "device")
GROUP_DT = ("zero", "tick", "span/50", "span/5", "10span")
N_GROUP_SMALL = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 1023, 1024, 1025, 1279, 1280, 1281]
N_GROUP_LARGE = [4095, 4096, 4097, 4351, 4353, 6000, 12_289]
HOT_BASES = (1024, 1024 + 256, 4096, 4096 + 256)     # EVK_RECONSTRUCT_WAVE_RUN, EVK_DENOISE_WAVE_RUN and one 256-event step more
HOT_PLACES = ("boundary", "border", "inside")
GROUP_MAX_RUN = 1 << 14                              # the reconstruction tolerance is derived for shorter runs
GROUP_BAD_SHARE = 0.10                               # injected invalid inputs (at most 15 % of the cases of a kind)


def _ref_raises(exc):
    def call():
        raise exc("documented")
    return call


def _group_sensor(rng):
    """(h, w, class): 1 x 1, one row, one column, both sides below 9 (no corner is eligible, smaller than the windows), one
    side below 9, h w within one of a multiple of 64, anything up to 40 x 48."""
    c = str(rng.choice(GROUP_SENSORS, p=[0.04, 0.05, 0.05, 0.08, 0.06, 0.32, 0.40]))
    if c == "1x1":
        return 1, 1, c
    if c == "1xW":
        return 1, int(rng.integers(2, 49)), c
    if c == "Hx1":
        return int(rng.integers(2, 41)), 1, c
    if c == "small":
        return int(rng.integers(2, 9)), int(rng.integers(2, 9)), c
    if c == "thin":
        a, b = int(rng.integers(2, 9)), int(rng.integers(9, 49))
        return (a, b, c) if rng.random() < 0.5 else (min(b, 40), a, c)
    if c == "around64":
        while True:
            T = 64 * int(rng.integers(1, 13)) + int(rng.integers(-1, 2))
            pairs = [(a, T // a) for a in range(2, 41) if T % a == 0 and T // a <= 48]
            if pairs:
                h, w = pairs[int(rng.integers(0, len(pairs)))]
                return h, w, c
            if T <= 200:
                return 1, T, c
    return int(rng.integers(9, 41)), int(rng.integers(9, 49)), c


def _group_positions(rng, scene, n, h, w, dense):
    """int64 pixels of n events whose stream position i / n is their progress through the scene; dense: noise and edges stay
    in a region of about n / 6 pixels, so that a short stream still gives every window its samples.  -> x, y and, for the scene
    'front', the number of consecutive events that share a column (and then a time stamp: the plane of such a window is exactly
    axis-aligned, and the slope along the front is the rounding residue of a double sum, in the defined order)"""
    prog = np.arange(n) / max(n, 1)
    x, y = rng.integers(0, w, n), rng.integers(0, h, n)
    if (dense and scene in ("noise", "edge", "ties", "hot")) or scene == "front":
        hb = int(np.clip(n // 40, min(3, h), h))
        wb = int(np.clip(n // (6 * hb), min(3, w), w))
        x0, y0 = int(rng.integers(0, w - wb + 1)), int(rng.integers(0, h - hb + 1))
        x, y = x0 + rng.integers(0, wb, n), y0 + rng.integers(0, hb, n)
        if scene == "front":                         # a front that sweeps the region column by column: 3 hb events per column
            x = x0 + (np.arange(n) // (3 * hb)) % wb
            return x.astype(np.int64), y.astype(np.int64), 3 * hb
        if scene != "noise":
            on = rng.random(n) < 0.7
            x = np.where(on, x0 + np.clip((prog * wb).astype(np.int64) + rng.integers(-1, 2, n), 0, wb - 1), x)
    elif scene in ("edge", "ties", "hot"):
        on = rng.random(n) < 0.7
        x = np.where(on, np.clip((prog * w).astype(np.int64) + rng.integers(-1, 2, n), 0, w - 1), x)
    elif scene == "blobs":
        on = rng.random(n) < 0.7
        cx, cy, which = rng.integers(0, w, 3), rng.integers(0, h, 3), rng.integers(0, 3, n)
        x = np.where(on, np.clip(cx[which] + rng.integers(-3, 4, n), 0, w - 1), x)
        y = np.where(on, np.clip(cy[which] + rng.integers(-3, 4, n), 0, h - 1), y)
    elif scene == "square" and min(h, w) >= 6:       # the outline of a square that moves along the diagonal: corners
        side = min(9, min(h, w) - 2)
        ring = [(a, 0) for a in range(side)] + [(0, b) for b in range(1, side)]
        ring += [(a, side - 1) for a in range(1, side)] + [(side - 1, b) for b in range(1, side - 1)]
        ring = np.array(ring)
        pick = rng.integers(0, len(ring), n)
        on = rng.random(n) < 0.9
        travel = max(2, n // 60) if dense else max(h, w)
        x = np.where(on, ring[pick, 0] + (prog * min(w - side + 1, travel)).astype(np.int64), x)
        y = np.where(on, ring[pick, 1] + (prog * min(h - side + 1, travel)).astype(np.int64), y)
    return x.astype(np.int64), y.astype(np.int64), None


def _group_times(rng, tk, n, scene, group=None):
    """the sorted time column of kind tk in its dtype, and the length of one tick"""
    tick = 1.0
    if tk in ("ticks", "i16", "i32", "i64"):
        S = int(rng.choice([max(2, n // 3), n + 1, 4 * n + 3]))
        t = np.sort(rng.integers(0, min(S, 30_000) if tk == "i16" else S, n))
        t = {"ticks": lambda: t.astype(np.float64), "i16": lambda: t.astype(np.int16), "i32": lambda: (t + 1_000_000).astype(np.int32),
             "i64": lambda: t.astype(np.int64) + 1_600_000_000_000_000}[tk]()
    elif tk == "const":
        t = np.full(n, 7.5)
    else:                                            # fractional seconds: sums of these are inexact
        S = 1e-5 if tk == "micro" else float(rng.choice([0.05, 1.0, 37.0] if tk != "epoch" else [0.05, 1.0]))
        t = np.sort(rng.uniform(0.0, S, n)) + (0.0 if tk == "micro" else float(rng.choice([0.0, 3.0])))
        tick = S / max(n, 1)
        t = EPOCH + t if tk == "epoch" else (t.astype(np.float32) if tk == "f32" else t)
    if scene in ("ties", "front") and n:             # heavy ties: every group of g events carries the stamp of its first
        g = int(rng.integers(4, 41)) if group is None else group
        t = t[(np.arange(n) // g) * g]
    return t, tick


def _group_pol(rng, pk, n):
    if pk == "pm1":
        return rng.integers(0, 2, n) * 2 - 1
    if pk in ("pos", "neg"):
        return np.full(n, 1 if pk == "pos" else -1)
    if pk == "pm1z":
        return rng.integers(-1, 2, n)
    if pk == "ints":
        return rng.integers(-3, 4, n)
    return rng.integers(0, 2, n).astype(bool)


def group_stream(rng, bad=None, unsorted_ok=True, hot_share=0.15, large_share=0.12, times=None, tiny_share=0.2, dense_share=0.5,
                 front_share=0.11, force=None):
    """The event stream of one case of the grouping family, host side only.  Draws the sensor, the event count, the scene (with
    the hot pixel's run exactly around the wave thresholds), the time-stamp kind and order, the polarity kind, the column kind
    and the DeviceEvents' polarity scale.  bad: 'oob_pixel' / 'frac_pixel' / 'unsorted' inject that invalid input where the
    case allows it (s['bad'] says whether it did).  -> dict: 'cols' what the caller hands over, 'ref' = (x, y, t, p) as the
    restatements take them (t: the float64 values of the stored column, p: with the sign of a negative scale folded in),
    'stored' the columns a filter hands back, 't_offset', 'span' and 'tick' for the parameters, and every drawn class."""
    h, w, size_class = _group_sensor(rng)
    scene = str(rng.choice(GROUP_SCENES, p=np.array([0.15, 0.27, 0.14, 0.17, 0.12, 0.0, 0.0]) / 0.85 * (1.0 - hot_share - front_share) +
                           np.array([0, 0, 0, 0, 0, front_share, hot_share])))
    if rng.random() < large_share:
        n = int(rng.choice(N_GROUP_LARGE))
    else:                                            # (0 .. 3 events: tiny_share of these)
        n = int(rng.choice(N_GROUP_SMALL[:4])) if rng.random() < tiny_share else int(rng.choice(N_GROUP_SMALL[4:]))
    n_class, hot, dense = n, None, bool(rng.random() < dense_share)
    force = force or {}
    scene = force.get("scene", scene)
    tk = str(rng.choice(GROUP_TIMES if times is None else times))
    # (DeviceEvents hold floating columns and always have ps: integer stamps and ps=None come as numpy columns or tensors)
    kind = str(rng.choice(GROUP_KINDS[:3] if tk in ("i16", "i32", "i64") or bad == "ps_none" else GROUP_KINDS))
    if tk == "epoch" and kind in ("f32", "slice", "small_dev", "relative"):      # (float32 columns cannot hold it; 'relative' adds it)
        tk = "frac"
    pk = str(rng.choice(GROUP_POLS))
    if force:                                        # (a directed sub-class of a kind: see planeflow_inputs)
        tk, pk, kind, unsorted_ok = force["tk"], force["pk"], str(rng.choice(force["kinds"])), False
        n = n_class = int(rng.choice(force["n"]))
    scale = float(rng.choice(GROUP_SCALES)) if kind in GROUP_EVENT_KINDS and rng.random() < 0.6 else 1.0
    if scale < 0 and not force and rng.random() < 0.6:      # a negative scale swaps the classes of +-1 as a whole: only p == 0 shows the sign
        pk = str(rng.choice(["pm1z", "ints", "bool"]))
    if scene == "hot":
        base, delta, place = int(rng.choice(HOT_BASES)), int(rng.integers(-1, 2)), str(rng.choice(HOT_PLACES))
        hot = {"base": base, "delta": delta, "place": place, "len": base + delta, "len2": 0}
        if h * w > 1:                                # a second long run: at the first pixel of class 1, or next to the hot pixel
            hot["len2"] = int(rng.choice(HOT_BASES)) + int(rng.integers(-1, 2))
        if place == "boundary":
            pk = "pm1"
        n, n_class = int(rng.choice([65, 257, 1000, 1281])) + hot["len"] + hot["len2"], "hot"
    x, y, group = _group_positions(rng, scene, n, h, w, dense)
    p = _group_pol(rng, pk, n)
    if hot is not None:
        where = rng.permutation(n)
        a, b = where[:hot["len"]], where[hot["len"]:hot["len"] + hot["len2"]]
        if hot["place"] == "boundary":               # the last pixel of class 0 (p <= 0) and the first pixel of class 1
            x[a], y[a], p[a], x[b], y[b], p[b] = w - 1, h - 1, -1, 0, 0, 1
        else:
            if hot["place"] == "border":
                x[a], y[a] = (0, int(rng.integers(0, h))) if rng.random() < 0.5 else (int(rng.integers(0, w)), h - 1)
            else:
                x[a], y[a] = w // 2, h // 2
            p[a] = p[a[0]]                           # one polarity each: the runs have their lengths in a two-class grouping as well
            if len(b):
                kb = (int(y[a[0]]) * w + int(x[a[0]]) + 1 + int(rng.integers(0, 5)) % (h * w - 1)) % (h * w)
                x[b], y[b], p[b] = kb % w, kb // w, p[b[0]]
        hot["xy"] = (int(x[a[0]]), int(y[a[0]]))
        # the background keeps off the hot pixels, so that their runs have exactly the drawn lengths
        rest = where[hot["len"] + hot["len2"]:]
        hot_keys = {int(y[a[0]]) * w + int(x[a[0]])} | ({int(y[b[0]]) * w + int(x[b[0]])} if len(b) else set())
        free = np.array([k for k in range(min(h * w, 12)) if k not in hot_keys], dtype=np.int64)
        hit = rest[np.isin(y[rest] * w + x[rest], list(hot_keys))]
        if len(free) and len(hit):
            k = free[rng.integers(0, len(free), len(hit))]
            x[hit], y[hit] = k % w, k // w
        hot["exact"] = bool(len(free))
    t, tick = _group_times(rng, tk, n, scene, group)
    order = "sorted"
    if n >= 2 and tk != "const" and (bad == "unsorted" or (unsorted_ok and rng.random() < 0.15)):
        perm = rng.permutation(n)
        if (np.diff(np.asarray(t, np.float64)[perm]) < 0).any():
            t, order = t[perm], "unsorted"
    t64 = np.asarray(t, np.float64)
    span = float(t64.max() - t64.min()) if n and t64.max() > t64.min() else 1.0
    s = {"h": h, "w": w, "size_class": size_class, "hw_mod": {63: "m1", 0: "0", 1: "p1"}.get(h * w % 64, "other"), "n": n,
         "n_class": n_class, "scene": scene, "hot": hot, "tk": tk, "order": order, "pk": pk, "kind": kind, "scale": scale,
         "span": span, "tick": tick, "bad": None, "dev_seed": int(rng.integers(1 << 31)), "plan": None, "t_offset": 0.0}
    xc, yc = x.copy(), y.copy()
    if bad == "oob_pixel" and n:
        j = int(rng.integers(0, n))
        xc[j], yc[j] = [(w, y[j]), (x[j], h), (-1, y[j]), (x[j], -1)][int(rng.integers(0, 4))]
        s["bad"] = bad
    elif bad == "unsorted" and order == "unsorted":
        s["bad"] = bad
    if kind in GROUP_EVENT_KINDS:
        xf, yf = xc.astype(np.float32), yc.astype(np.float32)
        if bad == "frac_pixel" and n and kind != "native":      # (native columns are int16)
            xf[int(rng.integers(0, n))] += 0.5
            s["bad"] = bad
        plan = _column_plan(rng, kind, xf, yf, t if t.dtype == np.float32 and kind != "relative" else np.asarray(t, np.float64),
                            p.astype(np.float32))
        s["plan"], s["t_offset"] = plan, plan["t_offset"]
        s["cols"] = plan["cols"]
        xr, yr, tr, pr = plan["ref"]
        dt = np.float32 if plan["f32"] else np.float64
        s["stored"] = tuple(np.asarray(a).astype(dt) for a in (xr, yr, tr, pr))
        s["xy_dtype"], s["p_dtype"] = "float32", "float32"
    else:
        xy = str(rng.choice(["int64", "int16", "int32", "float32", "float64"]))
        pd = "bool" if pk == "bool" else str(rng.choice(["int64", "float64", "float32", "int8"]))
        if bad == "frac_pixel" and n:
            xy = "float64"
        xc, yc, pc = xc.astype(xy), yc.astype(xy), p.astype(pd)
        if bad == "frac_pixel" and n:
            xc[int(rng.integers(0, n))] += 0.5
            s["bad"] = bad
        s["cols"] = s["stored"] = (xc, yc, t, pc)
        xr, yr, tr, pr = xc, yc, t, pc
        s["xy_dtype"], s["p_dtype"] = xy, pd
    sign = -1.0 if scale < 0 else 1.0
    s["ref"] = (np.asarray(xr), np.asarray(yr), np.asarray(tr).astype(np.float64), np.asarray(pr).astype(np.float64) * sign)
    s["p_none"] = False
    s["desc"] = "%dx%d(%s) n=%d(%s) %s %s/%s p=%s kind=%s scale=%g xy=%s%s%s" % (
        h, w, size_class, n, n_class, scene, tk, order, pk, kind, scale, s["xy_dtype"],
        "" if hot is None else " hot=%d+%d@%s" % (hot["len"], hot["len2"], hot["place"]), "" if s["bad"] is None else " BAD=" + s["bad"])
    return s


def group_source(s):
    """Device half of group_stream -> (xs, ys, ts, ps) as the public calls take them."""
    if s["plan"] is not None:
        return _device_source(s["plan"], s["scale"])
    cols = list(s["cols"])
    if s["kind"] != "numpy":
        rng = np.random.default_rng(s["dev_seed"])
        cols = [_dev(rng, a, sliced=s["kind"] == "tensor_slice") for a in cols]
    if s["p_none"]:
        cols[3] = None
    return tuple(cols)


def group_keys(s, two):
    """the grouping's keys class * h w + y w + x of the stream (np.bincount of them: the run lengths)"""
    x, y, _, p = s["ref"]
    return ((p > 0).astype(np.int64) if two else 0) * (s["h"] * s["w"]) + y.astype(np.int64) * s["w"] + x.astype(np.int64)


def _group_dt(rng, s, p=None):
    k = int(rng.choice(5, p=p))
    return [0.0, s["tick"], s["span"] / 50.0, s["span"] / 5.0, 10.0 * s["span"]][k], GROUP_DT[k]


def _group_select(rng, n, oob=False):
    """{'class', 'index' (int64 array or None), 'form'}: none, empty, one index, repeats, reversed order, a host list, a device
    tensor; oob: one index outside [0, n) among them (IndexError)."""
    c = str(rng.choice(GROUP_SELECTS, p=[0.4, 0.08, 0.1, 0.1, 0.1, 0.11, 0.11]))
    if n == 0 and c not in ("none", "empty"):
        c = "empty" if not oob else "one"
    if oob and c in ("none", "empty"):
        c = "list"
    if c == "none":
        return {"class": c, "index": None, "form": "none"}
    m = int(rng.integers(1, max(2, min(n, 300) + 1)))
    index = {"empty": lambda: np.zeros(0, np.int64), "one": lambda: rng.integers(0, max(n, 1), 1),
             "repeats": lambda: rng.integers(0, max(n, 1), 3)[rng.integers(0, 3, m)], "reversed": lambda: np.arange(n)[::-1][:m].copy(),
             "list": lambda: rng.integers(0, max(n, 1), m), "device": lambda: rng.integers(0, max(n, 1), m)}[c]().astype(np.int64)
    if oob:
        index[int(rng.integers(0, len(index)))] = n if rng.random() < 0.5 else -1
    return {"class": c + ("_oob" if oob else ""), "index": index, "form": "device" if c == "device" else ("list" if c == "list" else "numpy")}


def _select_arg(sel):
    if sel["index"] is None:
        return None
    if sel["form"] == "device":
        return torch.from_numpy(sel["index"]).cuda()
    return sel["index"].tolist() if sel["form"] == "list" else sel["index"]


def _draw_bad(rng, choices, share=GROUP_BAD_SHARE):
    return str(rng.choice(choices)) if rng.random() < share else None


# ---- the comparison rules, each as a function that returns a report ------------------------------------------------------------

def flags_equal(got, want, what):
    """dtype, shape and every element EQUAL (tests/test_gpu_corners.py::flags_equal, tests/test_gpu_plane_flow.py::flags_equal:
    comparisons of float64 times and the defined double arithmetic leave no freedom)."""
    a, b = _host(got), np.asarray(want)
    if a.dtype != b.dtype or a.shape != b.shape:
        return "%s: %s%s vs %s%s" % (what, a.dtype, a.shape, b.dtype, b.shape)
    return None if np.array_equal(a, b) else "%s: %d of %d differ (%d set in the restatement)" % (what, int((a != b).sum()), b.size, int((b != 0).sum()))


def rel23_close(got, want, what):
    """|got - want| <= 2^-23 |want| + 1e-10 with NaN in the same places (tests/test_gpu_corners.py::scores_close, header of that
    file: the rounding to float32 plus the order of float64 sums of magnitude <= 32; tests/test_gpu_plane_flow.py::values_close)."""
    a, b = _host(got), np.asarray(want)
    if a.dtype != np.float32 or b.dtype != np.float32 or a.shape != b.shape:
        return "%s: %s%s vs %s%s" % (what, a.dtype, a.shape, b.dtype, b.shape)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return "%s: NaN in other places (%d vs %d)" % (what, int(np.isnan(a).sum()), int(np.isnan(b).sum()))
    ok = ~np.isnan(b)
    with np.errstate(invalid="ignore"):
        err = np.abs(a[ok].astype(np.float64) - b[ok].astype(np.float64))
        tol = 2.0 ** -23 * np.abs(b[ok].astype(np.float64)) + 1e-10
        good = (err <= tol) | (a[ok] == b[ok])       # (equal infinities)
    return None if good.all() else "%s: max error %g of the bound at %d of %d" % (what, float(np.nanmax(err / tol)), int((~good).sum()), good.size)


def ts_close(got, want, what, deep=False):
    """tests/test_gpu_time_surface.py::close (derived in that file's header): ages and counts exact; float32 values within
    np.spacing(float32(want)) with zeros in the same places.  deep (the cases with age / tau above 87 or 745, where the float32
    and the double exp underflow): an added absolute 2^-126, the term of tests/_reconstruct_np.py::tolerance that keeps a
    comparison independent of how float32 subnormals are handled, and zeros compared only where |want| >= 2^-126."""
    a, b = _host(got), np.asarray(want)
    if a.dtype != b.dtype or a.shape != b.shape:
        return "%s: %s%s vs %s%s" % (what, a.dtype, a.shape, b.dtype, b.shape)
    if b.dtype != np.float32:
        return None if np.array_equal(a, b) else "%s: %d of %d elements differ" % (what, int((a != b).sum()), b.size)
    if not np.isfinite(b).all():
        return "fuzz case: %s: the restatement is not finite" % what
    tiny = np.float32(2.0 ** -126)
    look = (np.abs(b) >= tiny) | (np.abs(a) >= tiny) if deep else np.ones(b.shape, bool)
    if not np.array_equal((a == 0)[look], (b == 0)[look]):
        return "%s: zeros in other places" % what
    err = np.abs(a.astype(np.float64) - b.astype(np.float64))
    tol = np.spacing(np.abs(b)).astype(np.float64) + (2.0 ** -126 if deep else 0.0)
    return None if (err <= tol).all() else "%s: max error %g float32 spacings at %d of %d" % (what, float((err / tol).max()), int((err > tol).sum()), b.size)


def rc_close(got, want, bound, what, factor=None):
    """tests/test_gpu_reconstruct.py::close (derived in that file's header): |got - want| <= N.tolerance(want, bound, factor),
    factor N.TOL_REASSOC = 2^-36 of the restatement's bound A, 2^-23 after a streaming hand-over through float32."""
    N = _t("_reconstruct_np")
    a = _host(got)
    if a.dtype != np.float32 or a.shape != want.shape:
        return "%s: %s%s vs %s%s" % (what, a.dtype, a.shape, want.dtype, want.shape)
    if not np.isfinite(want).all():
        return "fuzz case: %s: the restatement is not finite" % what
    err, tol = np.abs(a.astype(np.float64) - want.astype(np.float64)), N.tolerance(want, bound, N.TOL_REASSOC if factor is None else factor)
    return None if (err <= tol).all() else "%s: max error %g tolerances at %d of %d" % (what, float((err / tol).max()), int((err > tol).sum()), err.size)


def _first(*reports):
    for r in reports:
        if r is not None:
            return r
    return None


def _kept_report(s, out, keep, what, extra=0):
    """the columns a filter hands back against the stored columns under `keep`: exact, dtypes included; a None column stays None;
    a DeviceEvents keeps its t_offset and p_scale"""
    from event_utils_amd.events import DeviceEvents
    want = [None if (s["p_none"] and i == 3) else np.asarray(c)[keep] for i, c in enumerate(s["stored"])]
    if isinstance(out, DeviceEvents):
        if s["plan"] is None:
            return "%s: a DeviceEvents for %s columns" % (what, s["kind"])
        if out.t_offset != s["t_offset"] or out.p_scale != s["scale"]:
            return "%s: t_offset / p_scale %r %r, wanted %r %r" % (what, out.t_offset, out.p_scale, s["t_offset"], s["scale"])
        return exact_all(out, want, what)
    if s["plan"] is not None or len(out) != 4 + extra:
        return "%s: %s of %d for %s columns" % (what, type(out).__name__, len(out), s["kind"])
    for i, (g, w) in enumerate(zip(out[:4], want)):
        if w is None:
            if g is not None:
                return "%s[%d]: not None" % (what, i)
            continue
        if isinstance(g, np.ndarray) != (s["kind"] == "numpy"):
            return "%s[%d]: %s for %s columns" % (what, i, type(g).__name__, s["kind"])
        err = exact(g, w, "%s[%d]" % (what, i))
        if err is not None:
            return err
    return None


def _run_case(desc, body):
    """(desc, report) of body(); a case with an injected invalid input compares the exception and nothing else"""
    try:
        return desc, body()
    except Exception as e:  # noqa: BLE001
        return desc, "raised %s: %s" % (type(e).__name__, e)


def _expect(exc, call, what):
    return raises_as(_ref_raises(exc), call, what)[2]


def _ok(verdict):
    return None if verdict == "ok" else verdict


BAD_ERRORS = {"oob_pixel": ValueError, "frac_pixel": TypeError, "unsorted": ValueError, "ps_none": TypeError, "select_oob": IndexError,
              "bad_arg": ValueError}


# ---- denoise ---------------------------------------------------------------------------------------------------------------------

DENOISE_BAD_ARGS = ("radius", "dt", "support", "refractory")      # a 'bad_arg' case compares the error of each in turn


def denoise_inputs(rng):
    """neighbour_support / background_activity_filter / refractory_filter: every radius, include_self, polarity option and support
    threshold, dt and refractory from {0, one tick, span / 50, span / 5, 10 span}, both walk orders and wave_run in {1, 64,
    default, 2^30}.  The times may be unsorted (include/evk.h, "Event denoising").  Non-finite time stamps are not drawn."""
    bad = _draw_bad(rng, ["oob_pixel", "frac_pixel", "ps_none", "bad_arg"])
    s = group_stream(rng, bad=bad, hot_share=0.4, large_share=0.15)
    radius, include_self, two = int(rng.integers(1, 4)), bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    most = (2 * radius + 1) ** 2 - (0 if include_self else 1)
    support = int(rng.integers(1, min(most, 4) + 1)) if rng.random() < 0.85 else int(rng.integers(1, most + 1))
    dt, dt_class = _group_dt(rng, s, [0.08, 0.22, 0.3, 0.3, 0.1])
    refractory, rf_class = _group_dt(rng, s, [0.1, 0.25, 0.3, 0.25, 0.1])
    c = {"s": s, "radius": radius, "include_self": include_self, "two": two, "support": support, "dt": dt, "dt_class": dt_class,
         "refractory": refractory, "rf_class": rf_class, "return_support": bool(rng.integers(0, 2)),
         "walk": str(rng.choice(["default", "stream", "pixel"])), "wave_run": int(rng.choice([1, 64, 0, 1 << 30])), "bad": s["bad"]}
    if bad == "ps_none" and s["plan"] is None:
        s["p_none"], c["two"], c["bad"] = True, True, bad
    elif bad == "bad_arg":
        c["bad"], c["bad_arg"] = bad, DENOISE_BAD_ARGS
    elif s["plan"] is None and not two and bad is None and rng.random() < 0.3:
        s["p_none"] = True                           # ps may be None unless a polarity option is on
    _copy_classes(c)
    c["desc"] = "denoise %s r=%d self=%d two=%d support=%d dt=%s refractory=%s walk=%s wave_run=%d ret=%d p_none=%d%s" % (
        s["desc"], radius, include_self, c["two"], support, dt_class, rf_class, c["walk"], c["wave_run"], c["return_support"], s["p_none"],
        "" if c["bad"] in (None, s["bad"]) else " BAD=" + c["bad"])
    return c


def _copy_classes(c):
    """the stream's drawn classes beside the kind's own, for tests/test_cpu_fuzz_inputs.py"""
    s = c["s"]
    for k in ("size_class", "hw_mod", "n_class", "scene", "tk", "order", "pk", "kind", "scale", "p_none", "n"):
        c[k] = s[k]
    c["hot_base"], c["hot_delta"], c["hot_place"] = (s["hot"]["base"], s["hot"]["delta"], s["hot"]["place"]) if s["hot"] else (None, None, None)
    c["fractional"] = s["tk"] in GROUP_FRACTIONAL


def denoise_reference(c):
    N, s = _t("_denoise_np"), c["s"]
    x, y, t, p = s["ref"]
    size = (s["h"], s["w"])
    sup = N.fast_support(x, y, t, p, c["dt"], size, c["radius"], c["include_self"], c["two"])
    return {"sup": sup, "keep": sup >= c["support"], "rkeep": N.fast_refractory(x, y, t, p, c["refractory"], size, c["two"])}


def case_denoise(rng):
    """neighbour_support, background_activity_filter (with and without return_support), refractory_filter and the two passes of
    Grouped (_grouping.py) with the drawn walk order and wave_run (evk_denoise.hip) against tests/_denoise_np.py::fast_*.  Rule: every support
    byte, flag and kept column is exact, dtypes included (header of tests/test_gpu_denoise.py: the definition has no rounding
    freedom)."""
    from event_utils_amd import _lib
    from event_utils_amd import _grouping as G
    from event_utils_amd.util.event_util import _In
    c = denoise_inputs(rng)
    s, size = c["s"], (c["s"]["h"], c["s"]["w"])
    kw = dict(sensor_size=size, radius=c["radius"], include_self=c["include_self"], same_polarity=c["two"])

    def body():
        src = group_source(s)
        if c["bad"] is not None:
            reports = []
            for a in (c["bad_arg"] if c["bad"] == "bad_arg" else (None,)):
                exc, kb, dt, rf, sp = BAD_ERRORS[c["bad"]], dict(kw), c["dt"], c["refractory"], c["support"]
                kb["radius"] = 0 if a == "radius" else kb["radius"]
                dt, rf = (-1.0 if a == "dt" else dt), (float("nan") if a == "refractory" else rf)
                sp = 0 if a == "support" else sp
                calls = []
                if a in (None, "radius", "dt"):
                    calls.append(("neighbour_support", lambda: E.neighbour_support(*src, dt, **kb)))
                if a != "refractory":
                    calls.append(("background_activity_filter", lambda: E.background_activity_filter(*src, dt, support=sp, **kb)))
                if a in (None, "refractory"):
                    calls.append(("refractory_filter", lambda: E.refractory_filter(*src, rf, sensor_size=size, per_polarity=c["two"])))
                reports += [_ok(_expect(exc, call, "%s (%s)" % (what, a or c["bad"]))) for what, call in calls]
            return _first(*reports)
        r = denoise_reference(c)
        got = E.neighbour_support(*src, c["dt"], **kw)
        if isinstance(got, np.ndarray) != (s["kind"] == "numpy"):
            return "neighbour_support: %s for %s columns" % (type(got).__name__, s["kind"])
        err = exact(got, r["sup"], "neighbour_support")
        if err is not None:
            return err
        out = E.background_activity_filter(*src, c["dt"], support=c["support"], return_support=c["return_support"], **kw)
        if c["return_support"]:
            out, gs = (out[0], out[1]) if s["plan"] is not None else (out, out[4])
            err = exact(gs, r["sup"], "return_support")
        err = err or _kept_report(s, out, r["keep"], "background_activity_filter", extra=int(c["return_support"]))
        err = err or _kept_report(s, E.refractory_filter(*src, c["refractory"], sensor_size=size, per_polarity=c["two"]), r["rkeep"],
                                  "refractory_filter")
        if err is not None or s["n"] == 0:
            return err
        g = G.Grouped(_In(*src), size, c["two"], "fuzz")
        walk = {"default": _lib.EVK_DENOISE_WALK_DEFAULT, "stream": _lib.EVK_DENOISE_WALK_STREAM, "pixel": _lib.EVK_DENOISE_WALK_PIXEL}[c["walk"]]
        sup, keep = g.support(c["dt"], c["radius"], c["include_self"], c["support"], True, walk)
        return _first(exact(sup, r["sup"], "support pass (%s)" % c["walk"]), exact(keep, r["keep"].astype(np.uint8), "keep flags (%s)" % c["walk"]),
                      exact(g.refractory(c["refractory"], c["wave_run"]), r["rkeep"].astype(np.uint8), "refractory pass (wave_run %d)" % c["wave_run"]))
    return _run_case(c["desc"], body)


# ---- tsurf -----------------------------------------------------------------------------------------------------------------------

TSURF_BAD_ARGS = ("tau", "radius", "decay", "cell_size", "dt")


def tsurf_inputs(rng):
    """time_surfaces (t_refs before / on / after the stream and on a tied stamp, or indices with the cuts 0 and n and unsorted
    cuts; K = 1), local_time_surfaces and averaged_time_surfaces: every radius, decay, polarity mode, include_self, cell_size
    (1, above the sensor, not dividing it) and normalise.  local_time_surfaces and time_surfaces(indices=) take unsorted times;
    on those the two calls that need sorted times are compared by their ValueError.  With both polarity modes "ignore" ps may be
    None: drawn for numpy columns and tensors, where averaged_time_surfaces is compared by its TypeError.  'deep': tau so small that age / tau passes
    87 (float32 exp underflows) or 745 (double exp underflows).  Non-finite time stamps are not drawn."""
    bad = _draw_bad(rng, ["oob_pixel", "frac_pixel", "ps_none", "select_oob", "bad_arg"])
    s = group_stream(rng, bad=bad, hot_share=0.10, large_share=0.10)
    n, t = s["n"], s["ref"][2]
    deep = str(rng.choice(["none", "f32", "f64"], p=[0.8, 0.1, 0.1])) if s["order"] == "sorted" else "none"
    tau = s["span"] / {"none": float(rng.choice([0.3, 4.0, 20.0])), "f32": 120.0, "f64": 900.0}[deep]
    c = {"s": s, "tau": tau, "deep": deep, "decay": [None, "exp", "linear"][int(rng.integers(0, 3))], "radius": int(rng.integers(1, 5)),
         "g_polarity": str(rng.choice(["split", "ignore"])), "l_polarity": str(rng.choice(["same", "split", "ignore"])),
         "include_self": bool(rng.integers(0, 2)), "normalise": bool(rng.integers(0, 2)),
         "cell_size": int(rng.choice([1, 3, 7, 10, 100])), "query": str(rng.choice(["t_refs", "indices"])), "bad": s["bad"]}
    c["h_dt"], c["h_dt_class"] = _group_dt(rng, s, [0.1, 0.2, 0.3, 0.3, 0.1])
    if s["hot"] is not None or n > 3000 or n > 40 * s["h"] * s["w"]:      # (the HATS window walk is quadratic in a crowded pixel's run)
        c["h_dt"], c["h_dt_class"] = min(c["h_dt"], s["span"] / 50.0), "span/50" if c["h_dt"] > s["span"] / 50.0 else c["h_dt_class"]
    c["select"] = _group_select(rng, n, oob=bad == "select_oob")
    if bad == "select_oob":
        c["bad"] = bad
    elif bad == "ps_none" and s["plan"] is None:
        s["p_none"], c["bad"] = True, bad
        c["l_polarity"] = "same" if c["l_polarity"] == "ignore" else c["l_polarity"]
    elif bad == "bad_arg":
        c["bad"], c["bad_arg"] = bad, TSURF_BAD_ARGS
    elif s["plan"] is None and bad is None and rng.random() < 0.2:
        # polarity "ignore": ps may be None (time_surfaces, local_time_surfaces); averaged_time_surfaces needs ps: its TypeError
        s["p_none"], c["g_polarity"], c["l_polarity"] = True, "ignore", "ignore"
    K = 1 if rng.random() < 0.25 else int(rng.integers(2, 6))
    if c["query"] == "indices":
        cuts = np.concatenate([[0, n], rng.integers(0, n + 1, 4)])[rng.permutation(6)[:K]] if n else np.zeros(1, np.int64)
        c["indices"], c["t_refs"], c["ref_t_refs"], c["q_classes"] = [int(v) for v in cuts], None, None, {"cut0"} if 0 in cuts else set()
        c["q_classes"] |= {"cutn"} if n in cuts else set()
        c["q_classes"] |= {"unsorted_cuts"} if (np.diff(cuts) < 0).any() else set()
    else:
        lo, hi = (float(t.min()), float(t.max())) if n else (0.0, 1.0)
        tied = np.flatnonzero(np.diff(t) == 0) if n > 1 else np.zeros(0, np.int64)
        pool = {"before": lo - 0.37 * s["span"], "after": hi + 0.5 * s["span"], "on": float(t[int(rng.integers(0, n))]) if n else 0.5,
                "tied": float(t[tied[int(rng.integers(0, len(tied)))]]) if len(tied) else None, "between": lo + float(rng.uniform(0.2, 0.9)) * (hi - lo)}
        names = [k for k in pool if pool[k] is not None]
        names = [names[i] for i in rng.permutation(len(names))[:K]]
        absolute = np.array([pool[k] for k in names], np.float64) + s["t_offset"]      # t_refs are absolute times
        c["indices"], c["t_refs"], c["ref_t_refs"], c["q_classes"] = None, absolute, absolute - s["t_offset"], set(names)
    c["K"] = K
    _copy_classes(c)
    c["desc"] = "tsurf %s tau=span/%.3g(%s) decay=%s r=%d pol=%s/%s self=%d cell=%d norm=%d hdt=%s %s K=%d select=%s%s" % (
        s["desc"], s["span"] / tau, deep, c["decay"], c["radius"], c["g_polarity"], c["l_polarity"], c["include_self"], c["cell_size"],
        c["normalise"], c["h_dt_class"], c["query"], K, c["select"]["class"] + (" p_none" if s["p_none"] else ""),
        "" if c["bad"] in (None, s["bad"]) else " BAD=" + c["bad"])
    return c


def tsurf_reference(c):
    """the restatement's outputs of the calls the case makes; None for a call that must raise ValueError on unsorted times"""
    N, s = _t("_time_surface_np"), c["s"]
    x, y, t, p = s["ref"]
    size, is_sorted = (s["h"], s["w"]), s["order"] == "sorted"
    r = {"global": None, "hats": None}
    with np.errstate(all="ignore"):
        if c["query"] == "indices" or is_sorted:
            r["global"] = N.fast_time_surfaces(x, y, t, p, c["tau"], size, t_refs=c["ref_t_refs"], indices=c["indices"], decay=c["decay"],
                                               polarity=c["g_polarity"])
        r["local"] = N.fast_local_time_surfaces(x, y, t, p, c["tau"], size, radius=c["radius"], decay=c["decay"], polarity=c["l_polarity"],
                                                include_self=c["include_self"], select=c["select"]["index"])
        if is_sorted and not s["p_none"]:
            r["hats"] = N.fast_averaged_time_surfaces(x, y, t, p, c["tau"], c["h_dt"], size, cell_size=c["cell_size"], radius=c["radius"],
                                                      normalise=c["normalise"], return_counts=True)
    return r


def case_tsurf(rng):
    """time_surfaces, local_time_surfaces and averaged_time_surfaces (evk_tsurf.hip) against tests/_time_surface_np.py::fast_*,
    by ts_close."""
    c = tsurf_inputs(rng)
    s, size, deep = c["s"], (c["s"]["h"], c["s"]["w"]), c["deep"] != "none"
    gkw = dict(sensor_size=size, decay=c["decay"], polarity=c["g_polarity"], t_refs=c["t_refs"], indices=c["indices"])
    lkw = dict(sensor_size=size, radius=c["radius"], decay=c["decay"], polarity=c["l_polarity"], include_self=c["include_self"])
    hkw = dict(sensor_size=size, cell_size=c["cell_size"], radius=c["radius"], normalise=c["normalise"], return_counts=True)

    def body():
        src = group_source(s)
        tau, hdt = c["tau"], c["h_dt"]
        if c["bad"] is not None:
            reports = []
            for a in (c["bad_arg"] if c["bad"] == "bad_arg" else (None,)):
                exc, tb, db, gb, lb, hb = BAD_ERRORS[c["bad"]], tau, hdt, dict(gkw), dict(lkw), dict(hkw)
                if a == "tau":
                    tb = 0.0
                elif a == "radius":
                    lb["radius"] = hb["radius"] = 5
                elif a == "decay":
                    gb["decay"] = lb["decay"] = "gauss"
                elif a == "cell_size":
                    hb["cell_size"] = 0
                elif a == "dt":
                    db = -1.0
                calls = []
                if c["bad"] in ("oob_pixel", "frac_pixel") or a in ("tau", "decay") or (c["bad"] == "ps_none" and c["g_polarity"] == "split"):
                    calls.append(("time_surfaces", lambda: E.time_surfaces(*src, tb, **gb)))
                if c["bad"] != "bad_arg" or a in ("tau", "radius", "decay"):
                    calls.append(("local_time_surfaces", lambda: E.local_time_surfaces(*src, tb, select=_select_arg(c["select"]), **lb)))
                if c["bad"] in ("oob_pixel", "frac_pixel", "ps_none") or a in ("tau", "radius", "cell_size", "dt"):
                    calls.append(("averaged_time_surfaces", lambda: E.averaged_time_surfaces(*src, tb, db, **hb)))
                reports += [_ok(_expect(exc, call, "%s (%s)" % (what, a or c["bad"]))) for what, call in calls]
            return _first(*reports)
        r = tsurf_reference(c)
        if r["global"] is None:
            err = _ok(_expect(ValueError, lambda: E.time_surfaces(*src, tau, **gkw), "time_surfaces on unsorted times"))
        else:
            got = E.time_surfaces(*src, tau, **gkw)
            if isinstance(got, np.ndarray) != (s["kind"] == "numpy"):
                return "time_surfaces: %s for %s columns" % (type(got).__name__, s["kind"])
            err = ts_close(got, r["global"], "time_surfaces", deep)
        err = err or ts_close(E.local_time_surfaces(*src, tau, select=_select_arg(c["select"]), **lkw), r["local"], "local_time_surfaces", deep)
        if err is not None:
            return err
        if r["hats"] is None:        # (the classes come first: TypeError without ps, also on unsorted times)
            return _ok(_expect(TypeError if s["p_none"] else ValueError, lambda: E.averaged_time_surfaces(*src, tau, hdt, **hkw),
                               "averaged_time_surfaces %s" % ("without ps" if s["p_none"] else "on unsorted times")))
        got = E.averaged_time_surfaces(*src, tau, hdt, **hkw)
        return _first(ts_close(got[1], r["hats"][1], "HATS counts"), ts_close(got[0], r["hats"][0], "HATS", deep))
    return _run_case(c["desc"], body)


# ---- corners ---------------------------------------------------------------------------------------------------------------------

CORNERS_BAD_ARGS = ("window", "n_last", "k", "detector")


def corners_inputs(rng):
    """fast_corners, harris_scores / harris_corners (n_last in {1, 2, n, above n} or dt, a random k) and corner_events with and
    without return_index, and the documented chain corner_events(return_index=True) -> local_time_surfaces(select=index).  The
    times may be unsorted.  Non-finite time stamps are not drawn."""
    bad = _draw_bad(rng, ["oob_pixel", "frac_pixel", "ps_none", "select_oob", "select_oob", "bad_arg"])
    s = group_stream(rng, bad=bad, hot_share=0.08, large_share=0.08)
    n = s["n"]
    c = {"s": s, "polarity": str(rng.choice(["same", "ignore"])), "k": float(rng.choice([0.0, 0.04, float(rng.uniform(0.0, 0.2))])),
         "window": str(rng.choice(["n_last", "dt"])), "return_index": bool(rng.integers(0, 2)),
         "detector": str(rng.choice(["fast", "harris"])), "chain_radius": int(rng.integers(1, 5)), "bad": s["bad"]}
    c["n_last_class"] = str(rng.choice(["1", "2", "n", "above", "some"]))
    c["n_last"] = {"1": 1, "2": 2, "n": max(n, 1), "above": n + 7, "some": int(rng.integers(3, 200))}[c["n_last_class"]]
    c["dt"], c["dt_class"] = _group_dt(rng, s, [0.1, 0.2, 0.3, 0.3, 0.1])
    c["select"] = _group_select(rng, n, oob=bad == "select_oob")
    if bad == "select_oob":
        c["bad"] = bad
    elif bad == "ps_none" and s["plan"] is None:
        s["p_none"], c["polarity"], c["bad"] = True, "same", bad
    elif bad == "bad_arg":
        c["bad"], c["bad_arg"] = bad, CORNERS_BAD_ARGS
    elif s["plan"] is None and c["polarity"] == "ignore" and bad is None and rng.random() < 0.3:
        s["p_none"] = True
    _copy_classes(c)
    c["wkw"] = {"n_last": c["n_last"]} if c["window"] == "n_last" else {"dt": c["dt"]}
    c["desc"] = "corners %s pol=%s window=%s k=%.3g det=%s index=%d select=%s p_none=%d%s" % (
        s["desc"], c["polarity"], "n_last=%d(%s)" % (c["n_last"], c["n_last_class"]) if c["window"] == "n_last" else "dt=" + c["dt_class"],
        c["k"], c["detector"], c["return_index"], c["select"]["class"], s["p_none"],
        "" if c["bad"] in (None, s["bad"]) else " BAD=" + c["bad"])
    return c


def corners_reference(c):
    """flags and scores of every event (the selection is applied by the caller), the threshold of the 'harris' detector -- the
    middle of the widest gap between the restatement's scores, so that no score lies near it -- and the kept events"""
    N, s = _t("_corners_np"), c["s"]
    x, y, t, p = s["ref"]
    size = (s["h"], s["w"])
    flags = N.fast_fast_corners(x, y, t, p, size, c["polarity"])
    with np.errstate(all="ignore"):
        scores = N.fast_harris_scores(x, y, t, p, size, polarity=c["polarity"], k=c["k"], **c["wkw"])
    u = np.unique(scores[np.isfinite(scores)].astype(np.float64))
    threshold = 8.0
    if len(u) >= 2:
        g = int(np.argmax(np.diff(u)))
        threshold = float(0.5 * (u[g] + u[g + 1])) if u[g + 1] - u[g] > 1e-3 * (1.0 + abs(u[g])) else float(u[-1]) + 1.0
    with np.errstate(invalid="ignore"):
        keep = flags if c["detector"] == "fast" else scores > np.float32(threshold)
    return {"flags": flags, "scores": scores, "threshold": threshold, "keep": keep, "eligible": N._eligible(x.astype(np.int64), y.astype(np.int64), *size)}


def case_corners(rng):
    """fast_corners, harris_scores, harris_corners and corner_events (evk_corner.hip) against tests/_corners_np.py::fast_*: flags,
    kept columns and indices EQUAL, scores by rel23_close; harris_corners against the scores the device itself returned, as
    tests/test_gpu_corners.py does, so that no event near the threshold has to be left out; the chain
    corner_events(return_index=True) -> local_time_surfaces(select=index) by ts_close against the restatement's rows."""
    c = corners_inputs(rng)
    s, size = c["s"], (c["s"]["h"], c["s"]["w"])

    def body():
        src = group_source(s)
        sel = _select_arg(c["select"])
        kw = dict(sensor_size=size, polarity=c["polarity"])
        if c["bad"] is not None:
            reports = []
            for a in (c["bad_arg"] if c["bad"] == "bad_arg" else (None,)):
                exc, wkw, k = BAD_ERRORS[c["bad"]], dict(c["wkw"]), c["k"]
                calls = []
                if a == "window":
                    exc, wkw = TypeError, {}
                elif a == "n_last":
                    wkw = {"n_last": 0}
                elif a == "k":
                    k = float("nan")
                elif a == "detector":
                    reports.append(_ok(_expect(ValueError, lambda: E.corner_events(*src, detector="susan", **kw), "corner_events (detector)")))
                    continue
                if c["bad"] != "bad_arg":
                    calls.append(("fast_corners", lambda: E.fast_corners(*src, select=sel, **kw)))
                calls.append(("harris_scores", lambda: E.harris_scores(*src, k=k, select=sel, **wkw, **kw)))
                calls.append(("harris_corners", lambda: E.harris_corners(*src, k=k, select=sel, **wkw, **kw)))
                if c["bad"] != "select_oob":
                    calls.append(("corner_events", lambda: E.corner_events(*src, detector="harris", k=k, **wkw, **kw)))
                reports += [_ok(_expect(exc, call, "%s (%s)" % (what, a or c["bad"]))) for what, call in calls]
            return _first(*reports)
        r = corners_reference(c)
        rows = np.arange(s["n"]) if c["select"]["index"] is None else c["select"]["index"]
        got = E.fast_corners(*src, select=sel, **kw)
        if isinstance(got, np.ndarray) != (s["kind"] == "numpy"):
            return "fast_corners: %s for %s columns" % (type(got).__name__, s["kind"])
        scores = E.harris_scores(*src, k=c["k"], select=sel, **c["wkw"], **kw)
        with np.errstate(invalid="ignore"):
            err = _first(flags_equal(got, r["flags"][rows], "fast_corners"), rel23_close(scores, r["scores"][rows], "harris_scores"),
                         flags_equal(E.harris_corners(*src, k=c["k"], select=sel, threshold=r["threshold"], **c["wkw"], **kw),
                                     _host(scores) > np.float32(r["threshold"]), "harris_corners"))
        if err is not None:
            return err
        dkw = dict(kw) if c["detector"] == "fast" else dict(kw, k=c["k"], threshold=r["threshold"], **c["wkw"])
        out = E.corner_events(*src, detector=c["detector"], return_index=c["return_index"], **dkw)
        index = np.flatnonzero(r["keep"]).astype(np.int64)
        if c["return_index"]:
            out, gi = (out[0], out[1]) if s["plan"] is not None else (out, out[4])
            err = exact(gi, index, "corner_events index")
            if err is None and c["polarity"] == "same":      # the documented chain
                N = _t("_time_surface_np")
                x, y, t, p = s["ref"]
                want = N.fast_local_time_surfaces(x, y, t, p, s["span"], size, radius=c["chain_radius"], select=index)
                err = ts_close(E.local_time_surfaces(*src, s["span"], sensor_size=size, radius=c["chain_radius"], select=gi), want,
                               "local_time_surfaces(select=corner index)")
        return err or _kept_report(s, out, r["keep"], "corner_events(%s)" % c["detector"], extra=int(c["return_index"]))
    return _run_case(c["desc"], body)


# ---- planeflow -------------------------------------------------------------------------------------------------------------------

PLANEFLOW_TIMES = ("ticks", "ticks", "frac", "frac", "frac", "micro", "micro", "micro", "epoch", "epoch", "f32", "f32", "i16", "i32",
                   "i64", "const")                   # over a third fractional; a constant stamp fits no plane


# the sub-class that sees the order of the double sums through the rule's own tolerance: complete, symmetric windows (one polarity,
# sorted stamps) of a front on float64 microsecond stamps; float32 columns would make every sum exact
PLANEFLOW_ORDER_PROBE = {"scene": "front", "tk": "micro", "pk": "pos", "kinds": ("numpy", "tensor", "tensor_slice", "f64"), "n": (257, 1000, 1281)}
PLANEFLOW_BAD_ARGS = ("radius", "min_samples", "iterations", "outlier_threshold", "max_speed", "dt")
PLANEFLOW_DT = ("zero", "tick", "span/10", "span/3", "span", "10span")


def _planeflow_residual(c):
    """A residual e_k > 0 of the first fit of some event, formed as tests/_plane_flow_np.py::fast_local_plane_flow forms it: drawn
    as the outlier threshold it makes the strict comparison e_k > threshold of include/evk.h decide a sample (and holds the
    device to the definition's own order of the residual's operations, bit for bit).  None when no fit has one."""
    N, TS, s = _t("_plane_flow_np"), _t("_time_surface_np"), c["s"]
    x, y, t, p = s["ref"]
    r = c["radius"]
    P = 2 * r + 1
    with np.errstate(all="ignore"):
        age = TS.fast_local_time_surfaces(x, y, t, p, None, (s["h"], s["w"]), radius=r, decay=None, polarity=c["polarity"],
                                          include_self=True).reshape(len(x), P * P)
        dys, dxs = (v.reshape(-1) for v in np.meshgrid(np.arange(-r, r + 1), np.arange(-r, r + 1), indexing="ij"))
        centre = (dxs == 0) & (dys == 0)
        use = np.isfinite(age) & (age <= c["dt"])
        tau = np.where(np.isfinite(age), 0.0 - age, 0.0)
        use[:, centre] = True
        a, b, cc, ok = N._fit_all(use, tau, dxs, dys, c["min_samples"])
        e = np.abs(((a[:, None] * dxs.astype(np.float64) + b[:, None] * dys.astype(np.float64)) + cc[:, None]) - tau)
        cand = np.sort(e[use & ~centre & ok[:, None] & (e > 0) & np.isfinite(e)])
    return float(cand[len(cand) // 2]) if len(cand) else None


def planeflow_inputs(rng):
    """local_plane_flow (with and without return_valid / return_lifetime, select) and plane_flow_field with return_count: every
    radius, min_samples from 3 to (2 r + 1)^2, outlier_threshold from a fraction of dt (0, 1 and several rejection rounds),
    iterations 0 .. 8, max_speed.  The times may be unsorted.  What can see the ORDER of the double sums: a front whose columns
    share a stamp (scene 'front') has a plane that is exactly axis-aligned, so the slope along the front is the rounding residue
    of sum dy tau, and v = (a, b) / g carries it times 1 / g -- above the 1e-10 of the rule once the time differences are of the
    order of microseconds ('micro' stamps).  What can see the strictness of the residual test: a threshold drawn ON a residual of
    the first fit ('th_probe').  Non-finite time stamps are not drawn (tests/_plane_flow_np.py:
    finite times only)."""
    bad = _draw_bad(rng, ["oob_pixel", "frac_pixel", "ps_none", "select_oob", "select_oob", "bad_arg"])
    probe = bad is None and rng.random() < 0.08
    s = group_stream(rng, bad=bad, hot_share=0.06, large_share=0.16, times=PLANEFLOW_TIMES, tiny_share=0.05, dense_share=0.9, front_share=0.2,
                     force=PLANEFLOW_ORDER_PROBE if probe else None)
    radius = int(rng.integers(1, 5))
    most = (2 * radius + 1) ** 2
    c = {"s": s, "radius": radius, "polarity": str(rng.choice(["same", "ignore"])),
         "min_samples": int(rng.integers(3, min(most, 6) + 1)) if rng.random() < 0.95 else int(rng.integers(3, most + 1)),
         "iterations": int(rng.integers(0, 9)), "return_valid": bool(rng.integers(0, 2)), "return_lifetime": bool(rng.integers(0, 2)), "bad": s["bad"]}
    k = int(rng.choice(6, p=[0.03, 0.03, 0.2, 0.3, 0.24, 0.2]))      # (a window of span / 50 holds 2 % of a short stream: no fit)
    c["dt"], c["dt_class"] = [0.0, s["tick"], s["span"] / 10.0, s["span"] / 3.0, s["span"], 10.0 * s["span"]][k], PLANEFLOW_DT[k]
    c["outlier_threshold"] = None if rng.random() < 0.4 else max(min(c["dt"], s["span"]), s["tick"]) * float(rng.choice([0.1, 0.3, 1.0, 3.0]))
    c["max_speed"] = None if rng.random() < 0.6 else float(rng.choice([3.0, 30.0, 300.0])) * max(s["w"], 2) / s["span"]
    c["probe"] = probe
    if probe:
        c["dt"], c["dt_class"], c["outlier_threshold"], c["max_speed"], c["min_samples"] = 10.0 * s["span"], "10span", None, None, min(c["min_samples"], 6)
    c["select"] = _group_select(rng, s["n"], oob=bad == "select_oob")
    if bad == "select_oob":
        c["bad"] = bad
    elif bad == "ps_none" and s["plan"] is None:
        s["p_none"], c["polarity"], c["bad"] = True, "same", bad
    elif bad == "bad_arg":
        c["bad"], c["bad_arg"] = bad, PLANEFLOW_BAD_ARGS
    elif s["plan"] is None and c["polarity"] == "ignore" and bad is None and rng.random() < 0.3:
        s["p_none"] = True
    c["th_probe"] = False
    if c["outlier_threshold"] is not None and c["bad"] is None and not probe and s["n"] >= 16 and rng.random() < 0.2:
        th = _planeflow_residual(c)                  # the threshold ON a residual of the first fit: e > th against e >= th
        if th is not None:
            c["outlier_threshold"], c["iterations"], c["th_probe"] = th, max(c["iterations"], 1), True
    _copy_classes(c)
    c["fit"] = dict(radius=radius, polarity=c["polarity"], min_samples=c["min_samples"], outlier_threshold=c["outlier_threshold"],
                    iterations=c["iterations"], max_speed=c["max_speed"])
    c["desc"] = "planeflow %s r=%d pol=%s min=%d th=%s it=%d vmax=%s dt=%s select=%s ret=%d%d p_none=%d%s" % (
        s["desc"], radius, c["polarity"], c["min_samples"], "-" if c["outlier_threshold"] is None else "%.3g" % c["outlier_threshold"],
        c["iterations"], "-" if c["max_speed"] is None else "%.3g" % c["max_speed"], c["dt_class"], c["select"]["class"], c["return_valid"],
        c["return_lifetime"], s["p_none"], "" if c["bad"] in (None, s["bad"]) else " BAD=" + c["bad"])
    return c


def planeflow_reference(c, **override):
    """(flow, valid, lifetime) of every event and (field, count), by tests/_plane_flow_np.py::fast_*"""
    N, s = _t("_plane_flow_np"), c["s"]
    x, y, t, p = s["ref"]
    size, fit = (s["h"], s["w"]), dict(c["fit"], **override)
    flow, valid, life = N.fast_local_plane_flow(x, y, t, p, c["dt"], size, **fit)
    field, count = N.fast_field_of_flow(x, y, p, flow, valid, size, fit["polarity"])
    return {"flow": flow, "valid": valid, "life": life, "field": field, "count": count}


def case_planeflow(rng):
    """local_plane_flow and plane_flow_field (evk_planeflow.hip) against tests/_plane_flow_np.py::fast_*.  Rule (header of
    tests/test_gpu_plane_flow.py): the definition fixes every double operation and its order, so valid and count are EQUAL and
    NaN stands in the same places; flow, lifetime and field by rel23_close.  No event is left out."""
    c = planeflow_inputs(rng)
    s, size = c["s"], (c["s"]["h"], c["s"]["w"])

    def body():
        src = group_source(s)
        sel = _select_arg(c["select"])
        if c["bad"] is not None:
            reports = []
            for a in (c["bad_arg"] if c["bad"] == "bad_arg" else (None,)):
                exc, fit, dt = BAD_ERRORS[c["bad"]], dict(c["fit"]), c["dt"]
                if a == "dt":
                    dt = float("nan")
                elif a is not None:
                    fit[a] = {"radius": 5, "min_samples": 2, "iterations": 9, "outlier_threshold": 0.0, "max_speed": -1.0}[a]
                calls = [("local_plane_flow", lambda: E.local_plane_flow(*src, dt, sensor_size=size, select=sel, **fit))]
                if c["bad"] != "select_oob":
                    calls.append(("plane_flow_field", lambda: E.plane_flow_field(*src, dt, sensor_size=size, **fit)))
                reports += [_ok(_expect(exc, call, "%s (%s)" % (what, a or c["bad"]))) for what, call in calls]
            return _first(*reports)
        with np.errstate(all="ignore"):
            r = planeflow_reference(c)
        rows = np.arange(s["n"]) if c["select"]["index"] is None else c["select"]["index"]
        got = E.local_plane_flow(*src, c["dt"], sensor_size=size, select=sel, return_valid=c["return_valid"],
                                 return_lifetime=c["return_lifetime"], **c["fit"])
        got = list(got) if isinstance(got, tuple) else [got]
        if len(got) != 1 + c["return_valid"] + c["return_lifetime"] or isinstance(got[0], np.ndarray) != (s["kind"] == "numpy"):
            return "local_plane_flow: %d outputs, %s for %s columns" % (len(got), type(got[0]).__name__, s["kind"])
        flow = got.pop(0)
        err = None
        if c["return_valid"]:
            err = flags_equal(got.pop(0), r["valid"][rows], "valid")
        err = err or flags_equal(np.isnan(_host(flow)[:, 0]) if _host(flow).ndim == 2 else None, ~r["valid"][rows], "NaN flows")
        err = err or rel23_close(flow, r["flow"][rows], "flow")
        if err is None and c["return_lifetime"]:
            err = rel23_close(got.pop(0), r["life"][rows], "lifetime")
        if err is not None:
            return err
        gf, gc = E.plane_flow_field(*src, c["dt"], sensor_size=size, return_count=True, **c["fit"])
        return _first(flags_equal(gc, r["count"], "count"), rel23_close(gf, r["field"], "field"))
    return _run_case(c["desc"], body)


# ---- reconstruct -----------------------------------------------------------------------------------------------------------------

RECONSTRUCT_BAD_ARGS = ("alpha", "c_on", "c_off", "queries", "both")


def reconstruct_inputs(rng):
    """leaky_integrator and complementary_filter with t_refs or indices: alpha 0, moderate and so large that old terms underflow,
    c_on != c_off, with and without initial and t_start, 1 .. 4 frames with a frame time before, between, after and on the
    queries, the streaming hand-over, wave_run in {1, 64, 65, default, 2^30} through _reconstruct.  ts must be non-decreasing
    (ValueError) and ps is needed (TypeError).  Non-finite time stamps are not drawn."""
    bad = _draw_bad(rng, ["oob_pixel", "frac_pixel", "ps_none", "unsorted", "bad_arg", "bad_arg", "index_oob"], share=0.13)
    s = group_stream(rng, bad=bad, unsorted_ok=False, hot_share=0.35, large_share=0.24)
    n, t, span, off = s["n"], s["ref"][2], s["span"], s["t_offset"]
    lo, hi = (float(t[0]), float(t[-1])) if n and s["order"] == "sorted" else (0.0, 1.0)
    a_class = str(rng.choice(["zero", "slow", "fast", "underflow"], p=[0.15, 0.35, 0.3, 0.2]))
    c = {"s": s, "alpha_class": a_class, "alpha": {"zero": 0.0, "slow": 0.5 / span, "fast": 8.0 / span, "underflow": 2000.0 / span}[a_class],
         "c_on": float(rng.choice([0.1, 0.23, 1.0])), "query": str(rng.choice(["t_refs", "indices"])), "filter": str(rng.choice(["leaky", "complementary"])),
         "wave_run": int(rng.choice([1, 64, 65, 0, 1 << 30])), "stream": False, "bad": s["bad"]}
    c["c_off"] = c["c_on"] * float(rng.choice([0.5, 0.74, 1.7]))
    K = int(rng.integers(1, 5))
    c["has_initial"], c["has_t_start"] = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    c["initial"] = (rng.normal(size=(s["h"], s["w"])).astype(np.float32 if rng.random() < 0.3 else np.float64)) if c["has_initial"] else None
    start_class = "default"
    t_start = None                                   # in the stored time base; the caller gets t_start + t_offset
    if c["query"] == "indices":
        cuts = np.sort(np.concatenate([[0, n], rng.integers(0, n + 1, 4)])[rng.permutation(6)[:K]])
        if not c["has_t_start"] and c["filter"] == "leaky":
            pass                                     # default: the first event, T_k = ts[m_k - 1] >= it
        else:
            start_class, t_start = "before", lo - 0.25 * span
        c["indices"], Ts = [int(v) for v in cuts], None
    else:
        if c["has_t_start"]:
            start_class = str(rng.choice(["before", "inside"]))
            t_start = lo - 0.25 * span if start_class == "before" else lo + float(rng.uniform(0.05, 0.4)) * (hi - lo)
        first = lo + (1e-3 * span if off != 0.0 else 0.0) if t_start is None else t_start      # (lo + off - off may round below lo)
        pool = [first, float(t[int(rng.integers(0, n))]) if n else first + 0.3 * span, hi + 0.5 * span] + [float(v) for v in rng.uniform(first, hi + 0.2 * span, 3)]
        Ts = np.sort(np.maximum(np.array(pool)[rng.permutation(6)[:K]], first))
        if rng.random() < 0.2 and K >= 2:
            Ts[1] = Ts[0]                            # two equal queries
        c["indices"] = None
    c["K"], c["start_class"] = K, start_class
    # absolute times as the caller passes them, and what the wrapper makes of them: value - t_offset in float64
    c["t_start"] = None if t_start is None else t_start + off
    c["t_refs"] = None if Ts is None else Ts + off
    c["frames"], c["frame_ts"], c["f_classes"] = None, None, set()
    if c["filter"] == "complementary":
        F = int(rng.integers(1, 5))
        q = (c["t_refs"] - off) if Ts is not None else np.array([lo, hi])
        pool = {"before": q[0] - 0.3 * span, "after": q[-1] + 0.3 * span, "on": float(q[int(rng.integers(0, len(q)))]),
                "between": float(0.5 * (q[0] + q[-1])) + 1e-3 * span}
        names = [list(pool)[i] for i in rng.permutation(4)[:F]]
        fts = np.unique(np.array([pool[k] for k in names]))
        c["frame_ts"], c["f_classes"] = fts + off, set(names)
        c["frames"] = rng.normal(scale=2.0, size=(len(c["frame_ts"]), s["h"], s["w"])).astype(np.float32 if rng.random() < 0.3 else np.float64)
        if len(np.unique(c["frame_ts"])) != len(c["frame_ts"]):      # (the offset's rounding merged two frame times)
            c["frame_ts"], c["frames"] = c["frame_ts"][:1], c["frames"][:1]
        if c["t_start"] is None and c["t_refs"] is not None and c["t_refs"][0] < c["frame_ts"][0]:      # the default t_start is frame_ts[0]
            c["t_start"], c["start_class"] = float(c["t_refs"][0]), "first_query"
        if c["t_start"] is None and c["indices"] is not None:
            c["t_start"], c["start_class"] = lo - 0.25 * span + off, "before"
    c["F"] = 0 if c["frames"] is None else len(c["frame_ts"])
    if c["query"] == "t_refs" and c["filter"] == "leaky" and n >= 4 and K >= 2 and bad is None and rng.random() < 0.4:
        c["stream"] = True                           # the hand-over: the first window ends at the query K // 2
    if bad == "ps_none" and s["plan"] is None:
        s["p_none"], c["bad"] = True, bad
    elif bad == "bad_arg":
        c["bad"], c["bad_arg"] = bad, RECONSTRUCT_BAD_ARGS
    elif bad == "index_oob" and c["indices"] is not None:
        c["bad"], c["indices"] = bad, c["indices"][:-1] + [n + 1]
    _copy_classes(c)
    c["desc"] = "reconstruct %s %s alpha=%s c=%.3g/%.3g %s K=%d initial=%d t_start=%s F=%d%s wave_run=%d stream=%d%s" % (
        s["desc"], c["filter"], a_class, c["c_on"], c["c_off"], c["query"], K, c["has_initial"], c["start_class"], c["F"],
        sorted(c["f_classes"]), c["wave_run"], c["stream"], "" if c["bad"] in (None, s["bad"]) else " BAD=" + c["bad"])
    return c


def reconstruct_reference(c):
    """(want, A) of tests/_reconstruct_np.py::seq_reconstruct on the stored columns, every absolute time less the column's offset
    as the wrapper forms it"""
    N, s = _t("_reconstruct_np"), c["s"]
    x, y, t, p = s["ref"]
    off = s["t_offset"]
    sub = lambda v: None if v is None else np.asarray(v, np.float64) - off  # noqa: E731
    return N.seq_reconstruct(x, y, t, p, c["alpha"], (s["h"], s["w"]), t_refs=sub(c["t_refs"]), indices=c["indices"], c_on=c["c_on"],
                             c_off=c["c_off"], initial=c["initial"], t_start=None if c["t_start"] is None else float(c["t_start"] - off),
                             frames=c["frames"], frame_ts=sub(c["frame_ts"]))


def case_reconstruct(rng):
    """leaky_integrator, complementary_filter and _reconstruct with the drawn wave_run (evk_reconstruct.hip) against
    tests/_reconstruct_np.py::seq_reconstruct by rc_close; the second window of a streaming hand-over with the 2^-23 A term."""
    from event_utils_amd.representations import reconstruction as RC
    c = reconstruct_inputs(rng)
    s, size = c["s"], (c["s"]["h"], c["s"]["w"])

    def call(src, wave_run=None, **over):
        kw = dict(alpha=c["alpha"], t_refs=c["t_refs"], indices=c["indices"], c_on=c["c_on"], c_off=c["c_off"], initial=c["initial"],
                  t_start=c["t_start"], frames=c["frames"], frame_ts=c["frame_ts"])
        kw.update(over)
        if wave_run is not None:
            return RC._reconstruct("fuzz", *src, kw["alpha"], size, kw["t_refs"], kw["indices"], kw["c_on"], kw["c_off"], kw["initial"],
                                   kw["t_start"], kw["frames"], kw["frame_ts"], wave_run=wave_run)
        alpha, frames, fts = kw.pop("alpha"), kw.pop("frames"), kw.pop("frame_ts")
        if c["filter"] == "leaky":
            return E.leaky_integrator(*src, alpha, sensor_size=size, **kw)
        return E.complementary_filter(*src, alpha, frames, fts, sensor_size=size, **kw)

    def body():
        src = group_source(s)
        if c["bad"] is not None:
            exc, reports = BAD_ERRORS.get(c["bad"], IndexError), []
            for a in (c["bad_arg"] if c["bad"] == "bad_arg" else (None,)):
                over = {"alpha": {"alpha": -1.0}, "c_on": {"c_on": 0.0}, "c_off": {"c_off": float("inf")}, "queries": {"t_refs": None, "indices": None},
                        "both": {"t_refs": [0.0], "indices": [0]}, None: {}}[a]
                reports.append(_ok(_expect(exc, lambda: call(src, **over), "%s (%s)" % (c["filter"], a or c["bad"]))))
            return _first(*reports)
        want, bound = reconstruct_reference(c)
        got = call(src)
        if isinstance(got, np.ndarray) != (s["kind"] == "numpy"):
            return "%s: %s for %s columns" % (c["filter"], type(got).__name__, s["kind"])
        err = rc_close(got, want, bound, c["filter"]) or rc_close(call(src, wave_run=c["wave_run"]), want, bound, "wave_run %d" % c["wave_run"])
        if err is not None or not c["stream"]:
            return err
        # the hand-over: the events before the query k of the first window, then the rest with initial = out[-1], t_start = T_k
        k = c["K"] // 2
        m = int(np.searchsorted(s["ref"][2], c["t_refs"][k - 1] - s["t_offset"], side="left"))
        first = call(src, t_refs=c["t_refs"][:k])
        err = rc_close(first, want[:k], bound[:k], "first window")
        if err is not None or s["plan"] is not None:     # (the second window needs the columns themselves: numpy / tensor kinds)
            return err
        tail = tuple(None if a is None else a[m:] for a in src)
        second = call(tail, t_refs=c["t_refs"][k:], initial=first[-1], t_start=float(c["t_refs"][k - 1]))
        return rc_close(second, want[k:], bound[k:], "second window", factor=2.0 ** -23)
    return _run_case(c["desc"], body)


# ---- emvs ------------------------------------------------------------------------------------------------------------------------
# Multi-view stereo (depth/emvs.py, evk_emvs.hip) against tests/_emvs_np.py, bit for bit, by the rules of tests/test_gpu_emvs.py;
# profiles/fuzz_emvs_simulate.txt.

EMVS_KINDS = ("numpy", "tensor", "tensor_slice", "events_f64", "events_f32", "events_slice")
EMVS_F32_KINDS = ("events_f32", "events_slice")      # the device columns are float32: the restatement sees the rounded values
EMVS_COORDS = ("int", "real", "f32", "wild", "exact")
EMVS_TIMES = ("spread", "clustered", "equal")
EMVS_N_CLASSES = ("0", "1", "small", "mid", "large")
EMVS_N_LARGE = [4095, 4096, 4097, 8191, 8193, 5000, 6000]      # a trip of the vote loop is 4 x 1024 events
EMVS_PACKETS = ("1", "2", "3", "7", "63", "64", "65", "100", "1000", "n-1", "n", "n+1", "2^40")
EMVS_CHUNKS = ("auto", "1", "2", "3", "trip", "n", "over")
EMVS_PLANES = ("random", "dup", "behind")
EMVS_VOLUMES = ("sensor", "other", "tiles_row", "tiles_bands")
EMVS_WILD = ("nan", "+inf", "-inf", "huge")
EMVS_WILD_WHERE = ("xs", "ys", "both")
EMVS_RADII = (0, 1, 2, 3, 5, 16)
EMVS_THRESHOLDS = (0.0, 0.3, 1.0, 2.5, 1e9)
EMVS_BAD = ("packet_time", "depth", "lengths", "pose", "median", "radius")
EMVS_BAD_SHARE = 0.12
EMVS_RAW_SHARE = 0.15


def _emvs_chunk_count(rng, cls, n):
    """the forced chunk count of a class (0: the library's own); 'trip': chunks of 700 .. 3000 events, a boundary inside a trip"""
    if cls == "auto":
        return 0
    if cls in ("1", "2", "3"):
        return int(cls)
    if cls == "trip":
        return max(2, -(-n // int(rng.integers(700, 3000))))
    return n if cls == "n" else n + int(rng.integers(1, 50))


def _emvs_depth_map_args(rng, tiles=False):
    r = int(rng.choice(EMVS_RADII + (int(rng.integers(0, 17)),), p=[0.06, 0.2, 0.2, 0.15, 0.1, 0.12, 0.17]))
    th = float(rng.choice(EMVS_THRESHOLDS, p=[0.3, 0.25, 0.2, 0.17, 0.08]))
    return {"filter_radius": r, "threshold": th, "median_size": 0 if tiles else int(rng.choice([0, 3, 5]))}


def _emvs_raw_inputs(rng):
    """a hand-built raw volume for dsi_depth_map: zero columns, equal maxima, cells at and above 2^31"""
    H, W = (int(v) for v in rng.integers(1, 41, 2))
    D = int(rng.integers(1, 10))
    raw = (rng.integers(0, 60, (D, H, W)) * (rng.random((D, H, W)) < 0.5)).astype(np.int64)
    raw[:, rng.random((H, W)) < 0.3] = 0
    by, bx = int(rng.integers(0, H)), int(rng.integers(0, W))
    raw[:, by:by + 5, bx:bx + 5] += rng.integers(100, 400, raw[:, by:by + 5, bx:bx + 5].shape)      # a ridge above its surroundings
    ties = rng.random((H, W)) < 0.2
    if D >= 2:                                             # equal maxima: the first one wins
        a, b = (int(v) for v in rng.permutation(D)[:2])
        top = raw.max(axis=0) + 1
        raw[a][ties], raw[b][ties] = top[ties], top[ties]
    big = rng.random((D, H, W)) < 0.02
    raw[big] = rng.integers(2 ** 31, 2 ** 32, int(big.sum()))
    raw[int(rng.integers(0, D)), int(rng.integers(0, H)), int(rng.integers(0, W))] = int(rng.choice([2 ** 31, 2 ** 32 - 1]))
    c = {"mode": "raw", "raw": raw, "size": (H, W), "D": D, "scale": int(rng.choice([1, 256])), "depths": rng.permutation(np.linspace(0.5, 4.0, D)),
         "dm": _emvs_depth_map_args(rng), "numpy_view": str(rng.choice(["int32", "uint32"])), "has_ties": bool(D >= 2 and ties.any()),
         "bad": str(rng.choice(["median", "radius"])) if rng.random() < EMVS_BAD_SHARE else None}
    c["desc"] = "emvs raw %dx%dx%d scale=%d dm=%s%s" % (D, H, W, c["scale"], sorted(c["dm"].items()), "" if c["bad"] is None else " BAD=" + c["bad"])
    return c


def _emvs_trajectory(rng, identity, behind):
    P = int(rng.integers(2, 7))
    pose_ts = np.concatenate([[-0.05 - rng.uniform(0.0, 0.3)], np.sort(rng.uniform(0.0, 1.0, P - 2)), [1.05 + rng.uniform(0.0, 0.3)]])
    flips = rng.random() < 0.4
    unnorm = rng.random() < 0.5
    if identity:
        positions = np.zeros((P, 3))
        quats = np.tile([0.0, 0.0, 0.0, 1.0], (P, 1)) * (rng.choice([1.0, 2.0, 0.5, 4.0], (P, 1)) if unnorm else 1.0)
    else:
        positions = rng.normal(0.0, 0.12, (P, 3))
        if behind:
            positions[:, 2] += np.linspace(0.0, 1.2, P)
        axis = rng.normal(size=(P, 3))
        axis /= np.linalg.norm(axis, axis=1, keepdims=True)
        half = 0.5 * rng.uniform(-0.5, 0.5, (P, 1))
        quats = np.concatenate([axis * np.sin(half), np.cos(half)], axis=1) * (rng.uniform(0.3, 3.0, (P, 1)) if unnorm else 1.0)
    if flips:
        quats = quats * rng.choice([-1.0, 1.0], (P, 1))
    return pose_ts, positions, quats, flips, unnorm


def _emvs_exact_pool(S):
    """coordinates of the 'exact' class along an axis of S cells: the rounding ties of nearest voting, k - 0.5 with the two borders
    -0.5 and S - 0.5, dyadic fractions around -1 and S - 1, where bilinear voting drops corners, and odd multiples of 1 / 32 and 1 / 16,
    whose products put a bilinear weight on a tie of its own (256 w = k + 0.5)"""
    return np.concatenate([np.arange(0, S + 1) - 0.5, -1.0 + np.arange(-4, 5) / 8.0, S - 1.0 + np.arange(-4, 9) / 8.0, np.arange(S, dtype=np.float64),
                           np.arange(-32, 32 * S + 1, max(1, S // 4)) / 32.0 + 1.0 / 32.0, np.arange(-16, 16 * S + 1, max(1, S // 4)) / 16.0 + 1.0 / 16.0])


def emvs_inputs(rng):
    """dsi_votes / dsi_depth_map / emvs_depth_map: sensors and volumes of 1 .. 40 cells a side (a single row, a single column), a DSI of
    another size and camera, volumes of several tiles; 1 .. 9 unordered planes, duplicated, or behind some packets' camera centres;
    0 .. 8193 events around the trips of the vote loop; integer, real, float32, non-finite / huge and exactly representable
    coordinates (votes on the rounding ties and borders); every packet size and forced chunk count; 2 .. 6 poses with unnormalised
    and sign-flipped quaternions; every column kind; every depth-map parameter; a hand-built raw volume; injected invalid inputs."""
    if rng.random() < EMVS_RAW_SHARE:
        return _emvs_raw_inputs(rng)
    bad = str(rng.choice(EMVS_BAD)) if rng.random() < EMVS_BAD_SHARE else None
    kind = str(rng.choice(EMVS_KINDS))
    if bad == "lengths" and kind.startswith("events"):
        kind = "numpy"
    coord = str(rng.choice(EMVS_COORDS, p=[0.15, 0.25, 0.15, 0.2, 0.25]))
    volume = "sensor" if coord == "exact" else str(rng.choice(EMVS_VOLUMES, p=[0.45, 0.43, 0.06, 0.06]))
    tiles = volume.startswith("tiles")
    planes = str(rng.choice(EMVS_PLANES, p=[0.5, 0.2, 0.3]))
    # ---- sensor and volume
    shape = str(rng.choice(["row", "column", "random"], p=[0.1, 0.1, 0.8]))
    H = 1 if shape == "row" else int(rng.integers(1, 41))
    W = 1 if shape == "column" else int(rng.integers(1, 41))
    wide = coord != "exact" and rng.random() < 0.2             # a short focal length: rays with d2 <= 0
    if coord == "exact":
        K = np.array([[64.0, 0.0, W / 2.0 + 0.25], [0.0, 64.0, H / 2.0 - 0.125], [0.0, 0.0, 1.0]])
    else:
        f = (0.05 if wide else 0.9) * max(W, H, 8)
        K = np.array([[f, 0.0, W / 2.0 + 0.3], [0.0, 1.07 * f, H / 2.0 - 0.2], [0.0, 0.0, 1.0]])
    dsi_size, ref_K = None, None
    if volume != "sensor":
        if volume == "other":
            dsi_size = (int(rng.integers(1, 41)), int(rng.integers(1, 41)))
        elif volume == "tiles_row":
            dsi_size = (1, int(rng.integers(40_001, 40_400)))
        else:
            dsi_size = (int(rng.integers(205, 216)), int(rng.integers(199, 206)))
        fr = rng.uniform(0.7, 1.3) * 0.9 * max(W, H, 8)
        ref_K = np.array([[fr * dsi_size[1] / max(W, 8), 0.0, dsi_size[1] * rng.uniform(0.35, 0.65)],
                          [0.0, 1.13 * fr * dsi_size[0] / max(H, 8), dsi_size[0] * rng.uniform(0.35, 0.65)], [0.0, 0.0, 1.0]])
    size = (H, W) if dsi_size is None else dsi_size
    # ---- planes
    D = int(rng.integers(1, 3 if tiles else 10))
    if coord == "exact":
        depths = rng.choice([0.25, 0.5, 1.0, 2.0, 4.0, 8.0], D, replace=D > 6)
    else:
        depths = rng.permutation(1.0 / rng.uniform(0.25, 2.0 if planes != "behind" else 4.0, D))
    if planes == "dup" and D >= 2:
        depths[int(rng.integers(1, D))] = depths[0]
    # ---- events
    n_class = str(rng.choice(EMVS_N_CLASSES, p=[0.04, 0.04, 0.3, 0.3, 0.32]))
    n = {"0": 0, "1": 1, "small": int(rng.integers(2, 65)), "mid": int(rng.integers(65, 2000)), "large": int(rng.choice(EMVS_N_LARGE))}[n_class]
    if tiles and n < 65:
        n_class, n = "mid", int(rng.integers(500, 2000))
    if n == 0 and bad in ("packet_time", "lengths"):           # (no event: no packet time, and columns of one length)
        bad = "depth"
    tk = str(rng.choice(EMVS_TIMES, p=[0.6, 0.25, 0.15]))
    t = {"spread": lambda: np.sort(rng.uniform(0.0, 1.0, n)), "clustered": lambda: np.sort(rng.choice(rng.uniform(0.0, 1.0, 3), n)),
         "equal": lambda: np.full(n, float(rng.uniform(0.0, 1.0)))}[tk]()
    f32 = kind in EMVS_F32_KINDS
    wild, where, ties = set(), None, False
    if coord == "int":
        x, y = rng.integers(0, W, n), rng.integers(0, H, n)
    elif coord == "exact":
        x, y = rng.choice(_emvs_exact_pool(W), n), rng.choice(_emvs_exact_pool(H), n)
        ties = True
    else:
        x, y = rng.uniform(-2.0, W + 2.0, n), rng.uniform(-2.0, H + 2.0, n)
        if coord == "f32":
            x = x.astype(np.float32)
            y = y.astype(np.float32) if rng.random() < 0.7 else y          # (mixed widths: both are taken as float64)
        elif coord == "wild":
            where = str(rng.choice(EMVS_WILD_WHERE))
            huge = 3e38 if f32 else 1e300
            values = np.array([np.nan, np.inf, -np.inf, huge, -huge])
            for col in {"xs": (x,), "ys": (y,), "both": (x, y)}[where]:
                hit = np.flatnonzero(rng.random(n) < rng.uniform(0.02, 0.3))
                col[hit] = rng.choice(values, len(hit))
                col[hit[:5]] = values[:len(hit[:5])]                # (every class, where five events are hit)
            xy = np.concatenate([x, y])
            wild = {name for name, m in (("nan", np.isnan(xy)), ("+inf", xy == np.inf), ("-inf", xy == -np.inf),
                                         ("huge", np.isfinite(xy) & (np.abs(xy) > 1e30))) if m.any()}
    # ---- packets, chunks, voting, trajectory, reference pose
    pk = str(rng.choice(EMVS_PACKETS))
    packet_size = max(1, {"n-1": n - 1, "n": n, "n+1": n + 1, "2^40": 2 ** 40}[pk]) if pk in ("n-1", "n", "n+1", "2^40") else int(pk)
    ck = [str(v) for v in rng.choice(EMVS_CHUNKS, 2, replace=False)]
    chunks = [_emvs_chunk_count(rng, v, n) for v in ck]
    voting = str(rng.choice(["nearest", "bilinear"]))
    pose_ts, positions, quats, flips, unnorm = _emvs_trajectory(rng, coord == "exact", planes == "behind")
    on_traj = coord != "exact" and rng.random() < 0.4
    if coord == "exact":
        reference = (np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]))
    elif on_traj:
        i = int(rng.integers(0, len(pose_ts)))
        reference = (positions[i].copy(), quats[i].copy())
    else:
        reference = (rng.normal(0.0, 0.15, 3), np.concatenate([rng.normal(0.0, 0.1, 3), [1.0]]))
    eff = min(packet_size, max(n, 1))
    split = int(rng.integers(1, -(-n // eff))) * eff if packet_size < n else None       # a multiple of packet_size in (0, n)
    c = {"mode": "events", "kind": kind, "coord": coord, "volume": volume, "planes": planes, "shape": shape, "sensor": (H, W), "size": size,
         "K": K, "ref_K": ref_K, "dsi_size": dsi_size, "D": D, "depths": np.asarray(depths, np.float64), "n": n, "n_class": n_class, "tk": tk,
         "x": x, "y": y, "t": t, "wild": wild, "where": where, "wide": wide, "pk": pk, "packet_size": packet_size, "ck": ck, "chunks": chunks,
         "voting": voting, "pose_ts": pose_ts, "positions": positions, "quats": quats, "flips": flips, "unnorm": unnorm, "on_traj": on_traj,
         "reference": reference, "split": split, "dm": _emvs_depth_map_args(rng, tiles), "bad": bad, "with_ps": bool(rng.random() < 0.3),
         "offs": [(int(rng.integers(1, 4)), int(rng.integers(0, 5))) for _ in range(3)]}
    if f32:
        x, y, t = _f32_values(x), _f32_values(y), _f32_values(t)
    c["ref"] = (np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64), np.asarray(t, np.float64))
    c["on_centre"] = False
    if planes == "behind" and n and rng.random() < 0.5:        # a plane exactly at a packet's camera centre: s == 0 votes nowhere
        C2 = emvs_table(c)[1][:, 11]
        j, i = int(rng.integers(0, len(C2))), int(rng.integers(0, D))
        if C2[j] > 0 and np.isfinite(C2[j]):
            c["depths"][i], c["on_centre"] = C2[j], True
    c["desc"] = "emvs %s %s sensor=%dx%d dsi=%s(%dx%d) D=%d(%s) n=%d t=%s packet=%s chunks=%s/%s %s poses=%d ref=%s dm=%s%s" % (
        kind, coord + ("[%s:%s]" % (where, ",".join(sorted(wild))) if coord == "wild" else ""), H, W, volume, size[0], size[1], D, planes, n, tk, pk,
        ck[0], ck[1], voting, len(pose_ts), "on" if on_traj else "off", sorted(c["dm"].items()), "" if bad is None else " BAD=" + bad)
    return c


def emvs_table(c, ts=None):
    """the packet table of the case: the product's host-only packet_transforms (pinned by tests/test_cpu_emvs.py) on the
    restatement's packet times of the host time column"""
    from event_utils_amd.depth.emvs import packet_transforms
    N = _t("_emvs_np")
    ts = c["ref"][2] if ts is None else ts
    eff = min(c["packet_size"], max(len(ts), 1))
    times = N.packet_times(ts, eff) if len(ts) else np.empty(0)
    return times, packet_transforms(times, c["pose_ts"], c["positions"], c["quats"], c["K"], c["reference"]), eff


def emvs_reference(c):
    """tests/_emvs_np.py on the host columns -> {'raw' (int64 cells), 'times', 'table', 'dm' (depth, index, conf, mask)}; the depth
    map is taken from the cells modulo 2^32, which is what a DSI holds.  No device call."""
    N = _t("_emvs_np")
    if c["mode"] == "raw":
        return {"raw": c["raw"], "dm": N.dsi_depth_map(c["raw"], c["scale"], c["depths"], **c["dm"])}
    times, table, eff = emvs_table(c)
    Km = c["K"] if c["ref_K"] is None else c["ref_K"]
    raw = N.dsi_votes(c["ref"][0], c["ref"][1], table, c["depths"], (Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2]), c["size"], eff, c["voting"])
    return {"raw": raw, "times": times, "table": table, "dm": N.dsi_depth_map(raw & 0xFFFFFFFF, N.SCALE[c["voting"]], c["depths"], **c["dm"])}


def _emvs_i32(raw64):
    return (np.asarray(raw64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def _emvs_source(c, x=None, y=None, t=None):
    """the event columns of the case as its column kind hands them over"""
    from event_utils_amd import DeviceEvents
    x, y, t = (c["x"] if x is None else x), (c["y"] if y is None else y), (c["t"] if t is None else t)
    kind, n = c["kind"], len(t)
    ps = np.ones(n, np.int64)
    if kind == "numpy":
        return (x, y, t, ps if c["with_ps"] else None)
    if kind == "tensor":
        return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x, y, t)) + (None,)
    if kind == "tensor_slice":                              # slices 1 - 3 elements into larger buffers: misaligned views
        cols = []
        for a, (off, tail) in zip((x, y, t), c["offs"]):
            src = torch.from_numpy(np.ascontiguousarray(a))
            buf = torch.zeros(off + len(a) + tail, dtype=src.dtype, device="cuda")
            buf[off:off + len(a)] = src.cuda()
            cols.append(buf[off:off + len(a)])
        return tuple(cols) + (None,)
    if kind in ("events_f64", "events_f32"):
        return (DeviceEvents.from_arrays(x, y, t, ps, precision=kind[-3:]), None, None, None)
    off, tail = c["offs"][0]
    padded = [np.concatenate([np.zeros(off), np.asarray(a, np.float64), np.zeros(tail)]) for a in (x, y, t, ps)]
    return (DeviceEvents.from_arrays(*padded, precision="f32").slice(off, off + n), None, None, None)


def _emvs_part(src, a, b):
    from event_utils_amd import DeviceEvents
    if isinstance(src[0], DeviceEvents):
        return (src[0].slice(a, b), None, None, None)
    return tuple(None if col is None else col[a:b] for col in src)


def _emvs_dm_report(dm, want, scale, what):
    depth, idx, conf, mask = want
    if (dm.index.dtype, dm.mask.dtype, dm.depth.dtype, dm.confidence.dtype) != (torch.int32, torch.bool, torch.float64, torch.float32):
        return "%s: dtypes %s %s %s %s" % (what, dm.index.dtype, dm.mask.dtype, dm.depth.dtype, dm.confidence.dtype)
    return _first(flags_equal(dm.index, idx, what + " index"), flags_equal(dm.mask, mask, what + " mask"),
                  equal(dm.depth, depth, what + " depth"),
                  flags_equal(dm.confidence, (conf.astype(np.float64) / scale).astype(np.float32), what + " confidence"))


def _emvs_same_dm(a, b, what):
    return _first(*(exact(getattr(a, k), _host(getattr(b, k)), "%s %s" % (what, k)) for k in ("depth", "index", "confidence", "mask")))


def case_emvs(rng):
    """dsi_votes (through emvs._votes where the chunk count is forced), packet_times, dsi_depth_map and emvs_depth_map against
    tests/_emvs_np.py: every comparison exact."""
    from event_utils_amd.depth import emvs
    c = emvs_inputs(rng)
    N = _t("_emvs_np")

    def raw_body():
        want = emvs_reference(c)
        handed = (torch.from_numpy(_emvs_i32(c["raw"])).cuda(), _emvs_i32(c["raw"]).view(c["numpy_view"]))
        if c["bad"] is not None:
            kw = dict(c["dm"], **({"median_size": 4} if c["bad"] == "median" else {"filter_radius": 17}))
            err = _ok(_expect(ValueError, lambda: E.dsi_depth_map(E.DSI(handed[0], c["scale"], c["depths"]), **kw), c["bad"]))
            if err is not None:
                return err
        return _first(*(_emvs_dm_report(E.dsi_depth_map(E.DSI(h, c["scale"], c["depths"]), **c["dm"]), want["dm"], c["scale"], "raw %d" % i)
                        for i, h in enumerate(handed)))

    def votes(src, chunks, **over):
        kw = dict(camera_matrix=c["K"], pose_ts=c["pose_ts"], positions=c["positions"], quaternions=c["quats"], reference_pose=c["reference"],
                  depths=c["depths"], sensor_size=c["sensor"], packet_size=c["packet_size"], voting=c["voting"],
                  reference_camera_matrix=c["ref_K"], dsi_size=c["dsi_size"])
        kw.update(over)
        if not chunks:
            return E.dsi_votes(*src, **kw)
        return emvs._votes(src[0], src[1], src[2], kw["camera_matrix"], kw["pose_ts"], kw["positions"], kw["quaternions"], kw["reference_pose"],
                           kw["depths"], kw["sensor_size"], kw["packet_size"], kw["voting"], kw["reference_camera_matrix"], kw["dsi_size"],
                           chunks=chunks)

    def bad_call(src):
        b = c["bad"]
        if b == "packet_time":
            shifted = _emvs_source(c, t=c["t"] + (10.0 if c["n"] % 2 else -10.0))
            return lambda: votes(shifted, 0)
        if b == "depth":
            depths = c["depths"].copy()
            depths[len(depths) // 2] = [0.0, -1.0, np.nan, np.inf][c["n"] % 4]
            return lambda: votes(src, 0, depths=depths)
        if b == "lengths":
            return lambda: votes((src[0], src[1][:-1], src[2], None), 0)
        if b == "pose":
            if c["n"] % 2:
                positions = c["positions"].copy()
                positions[0, 1] = np.nan
                return lambda: votes(src, 0, positions=positions)
            quats = c["quats"].copy()
            quats[-1] = 0.0 if c["n"] % 4 else np.inf
            return lambda: votes(src, 0, quaternions=quats)
        kw = dict(c["dm"], **({"median_size": 4} if b == "median" else {"filter_radius": 17}))
        return lambda: E.dsi_depth_map(votes(src, 0), **kw)

    def body():
        if c["mode"] == "raw":
            return raw_body()
        src = _emvs_source(c)
        if c["bad"] is not None:                            # the ValueError, then the valid call on the same inputs below
            err = _ok(_expect(ValueError, bad_call(src), c["bad"]))
            if err is not None:
                return err
        want = emvs_reference(c)
        scale = N.SCALE[c["voting"]]
        dsi = votes(src, c["chunks"][0])
        if dsi.raw.dtype != torch.int32 or not dsi.raw.is_cuda or dsi.scale != scale:
            return "dsi: %s cuda=%d scale=%r" % (dsi.raw.dtype, dsi.raw.is_cuda, dsi.scale)
        err = _first(exact(dsi.raw, _emvs_i32(want["raw"]), "raw"), exact(dsi.depths, c["depths"], "depths"),
                     exact(dsi.votes(), ((want["raw"] & 0xFFFFFFFF) / scale).astype(np.float32), "votes()"),
                     exact(E.packet_times(*src, packet_size=c["packet_size"]), want["times"].astype(np.float64), "packet_times"),
                     _emvs_dm_report(E.dsi_depth_map(dsi, **c["dm"]), want["dm"], scale, "depth map"))
        if err is not None:
            return err
        again = votes(src, c["chunks"][1])
        if again.raw.data_ptr() == dsi.raw.data_ptr() or not torch.equal(again.raw, dsi.raw):
            return "chunks %s: other bytes than chunks %s" % (c["ck"][1], c["ck"][0])
        if c["split"] is not None:                          # adds commute: two calls on [0, k) and [k, n), k a multiple of packet_size
            k = c["split"]
            parts = [votes(_emvs_part(src, a, b), c["chunks"][i]).raw.cpu().numpy().view(np.uint32) for i, (a, b) in enumerate(((0, k), (k, c["n"])))]
            err = exact((parts[0] + parts[1]).view(np.int32), _emvs_i32(want["raw"]), "split at %d" % k)
            if err is not None:
                return err
        one = E.emvs_depth_map(*src, camera_matrix=c["K"], pose_ts=c["pose_ts"], positions=c["positions"], quaternions=c["quats"],
                               reference_pose=c["reference"], depths=c["depths"], sensor_size=c["sensor"], packet_size=c["packet_size"],
                               voting=c["voting"], reference_camera_matrix=c["ref_K"], dsi_size=c["dsi_size"], **c["dm"])
        return _emvs_same_dm(one, E.dsi_depth_map(votes(src, 0), **c["dm"]), "emvs_depth_map")
    return _run_case(c["desc"], body)


# ---- simulate --------------------------------------------------------------------------------------------------------------------
# The event simulator (simulation/event_simulator.py, evk_simulate.hip) against tests/_simulate_np.py::seq_simulate, bit for bit, by
# the rules of same() in tests/test_gpu_simulate.py; profiles/fuzz_emvs_simulate.txt.

SIM_SHAPES = ("random", "one_row", "around64", "around256")
SIM_AROUND = {"around64": [(7, 9), (8, 8), (5, 13), (3, 21), (11, 6)], "around256": [(15, 17), (16, 16), (11, 23), (13, 20), (12, 22)]}
SIM_TIMES = ("small", "nonuniform", "negative", "epoch9", "epoch15", "neighbours", "span64", "subnormal")
SIM_AMPS = ("none", "one", "hundreds", "limit")
SIM_DTYPES = ("f64", "f32", "int")
SIM_SPECIALS = ("none", "nonfinite", "huge")
SIM_INPUTS = ("numpy", "host_tensor", "device_tensor")
SIM_TS_KINDS = ("list", "array", "tensor")
SIM_CONTRASTS = ("scalar", "map_on", "map_off", "map_both")
SIM_MAP_KINDS = ("numpy_f64", "numpy_f32", "device_f64", "device_f32")
SIM_REFRACTORY = ("zero", "fraction", "interval", "beyond")
SIM_STATES = ("none", "reference", "last", "both")
SIM_LAYOUTS = ("contiguous", "strided", "transposed")
SIM_BAD = ("ts_order", "ts_nonfinite", "map_shape", "state_shape", "complex", "map_values", "overflow_tiny", "overflow_hot", "overflow_inf")
SIM_BAD_SHARE = 0.11


def _sim_times(rng, tk, F):
    if tk == "small":
        return float(rng.integers(0, 9)) + float(rng.choice([1.0, 0.5, 1024.0])) * np.arange(F)
    if tk == "nonuniform":
        return rng.uniform(-5.0, 5.0) + np.cumsum(rng.uniform(0.1, 3.0, F))
    if tk == "negative":                                   # crosses zero, with a -0.0 among the frame times
        T = (np.arange(F) - int(rng.integers(0, F))) * float(rng.choice([1024.0, 0.75]))
        T[T == 0] = -0.0
        return T
    if tk == "epoch9":                                     # seconds since 1970 with sub-second steps
        return 1.6e9 + np.cumsum(rng.uniform(0.01, 0.5, F))
    if tk == "epoch15":                                    # microseconds since 1970 with steps of a few thousand
        return 1.6e15 + np.cumsum(rng.integers(1000, 5000, F)).astype(np.float64)
    if tk == "neighbours":                                 # each time the next double after the one before
        T = [float(rng.choice([1.0, 1.6e9, -3.5, 0.0]))]
        for _ in range(F - 1):
            T.append(float(np.nextafter(T[-1], np.inf)))
        return np.array(T)
    if tk == "span64":
        return np.linspace(-1e300, 1e300, F)
    return (np.arange(F) - F // 2) * float(rng.integers(1, 6)) * 5e-324      # subnormal times around zero


def simulate_inputs(rng):
    """simulate_events: 2 .. 6 frames of 1 .. 24 pixels a side (pixel counts around 64 and 256, one row of 257 .. 600); frame times that
    are small, non-uniform, negative with a -0.0, epoch-scale, neighbouring doubles, 64 key bits apart, subnormal; dyadic and smooth
    frames of no, one, hundreds and almost 65 536 contrasts, float64 / float32 / integer, with NaN / infinite / overflowing pixels,
    as non-contiguous views, numpy or tensors; scalar and per-pixel contrasts; every refractory and state class; the wide sort
    values; injected invalid inputs, the step-limit overflow among them."""
    N = _t("_simulate_np")
    bad = str(rng.choice(SIM_BAD)) if rng.random() < SIM_BAD_SHARE else None
    shape = str(rng.choice(SIM_SHAPES, p=[0.55, 0.1, 0.2, 0.15]))
    F = int(rng.integers(2, 7))
    if shape == "random":
        H, W = (int(v) for v in rng.integers(1, 25, 2))
    elif shape == "one_row":
        H, W = 1, int(rng.integers(257, 601))
    else:
        H, W = SIM_AROUND[shape][int(rng.integers(0, 5))]
        H, W = (W, H) if max(H, W) <= 24 and rng.random() < 0.5 else (H, W)
    tk = str(rng.choice(SIM_TIMES))
    T = _sim_times(rng, tk, F)
    dtype = str(rng.choice(SIM_DTYPES, p=[0.5, 0.25, 0.25]))
    amp = str(rng.choice(SIM_AMPS, p=[0.08, 0.6, 0.28, 0.04]))
    special = str(rng.choice(SIM_SPECIALS, p=[0.7, 0.2, 0.1]))
    if amp == "limit" or special == "huge":
        dtype = "f64"
    if dtype == "int":
        special = "none"
    dyadic = dtype == "int" or rng.random() < 0.4
    c0 = float(rng.choice([0.5, 1.0])) if dtype == "int" else float(rng.choice([0.5, 0.25, 1.0])) if dyadic else float(rng.uniform(0.08, 0.3))
    c_on, c_off = c0, c0 * float(rng.choice([1.0, 0.5, 1.5]))
    # ---- contrasts
    ck = str(rng.choice(SIM_CONTRASTS, p=[0.4, 0.2, 0.2, 0.2]))
    mk = str(rng.choice(SIM_MAP_KINDS))
    con, coff = c_on, c_off
    draw_map = lambda c: ((rng.choice([0.5, 1.0, 1.5], (H, W)) if dyadic else rng.uniform(0.6, 1.5, (H, W))) * c).astype(  # noqa: E731
        np.float32 if mk.endswith("f32") else np.float64)
    if ck in ("map_on", "map_both"):
        con = draw_map(c_on)
    if ck in ("map_off", "map_both"):
        coff = draw_map(c_off)
    con_map, coff_map = (np.broadcast_to(np.asarray(v, np.float64), (H, W)) for v in (con, coff))
    # ---- frames
    if dtype == "int":
        frames = rng.integers(-3, 4, (F, H, W)).astype(np.float64)
    elif dyadic:
        frames = rng.integers(-4, 5, (F, H, W)) * (0.5 * c0)
    else:
        yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
        ph = rng.uniform(0.0, 2.0 * np.pi, 2)
        A = c0 * rng.uniform(1.0, 3.0)
        frames = np.stack([A * np.sin(0.5 * xx + 0.9 * f + ph[0]) * np.cos(0.4 * yy + ph[1]) for f in range(F)]) + 0.3 * A * rng.normal(size=(F, H, W))
    if amp == "none":                                      # no pixel moves one contrast away from frames[0]
        frames = np.repeat(frames[:1], F, axis=0) + (0.0 if dyadic else 0.2 * c0 * rng.uniform(-1.0, 1.0, (F, H, W)))
    elif amp in ("hundreds", "limit"):
        for _ in range(int(rng.integers(1, 7)) if amp == "hundreds" else 1):
            f, y, x = int(rng.integers(1, F)), int(rng.integers(0, H)), int(rng.integers(0, W))
            up = rng.random() < 0.5
            steps = float(rng.integers(100, 400)) if amp == "hundreds" else 65000.25      # (the limit counts 65 536 per interval)
            frames[f:, y, x] = frames[f - 1, y, x] + (steps * con_map[y, x] if up else -steps * coff_map[y, x])
    if dtype == "f32":
        frames = frames.astype(np.float32)
    elif dtype == "int":
        it = [np.int16, np.int32, np.uint8][int(rng.integers(0, 3))]
        if it is np.uint8 and amp in ("none", "one"):      # (0 .. 6; the large steps of the other classes need a signed type)
            frames = (frames + 3.0).astype(np.uint8)
        else:
            frames = frames.astype(np.int32 if it is np.uint8 else it)
    if special == "nonfinite":
        hit = rng.random((F, H, W)) < 0.04
        hit[0] = False                                     # (an infinite level in frames[0] never ends its walk: 'overflow_inf' below)
        frames[hit] = rng.choice([np.nan, np.inf, -np.inf], int(hit.sum()))
        frames[0, int(rng.integers(0, H)), int(rng.integers(0, W))] = np.nan               # a level that stays NaN
    elif special == "huge":                                # finite pixels whose difference overflows: the interval is skipped
        for _ in range(int(rng.integers(1, 4))):
            frames[:, int(rng.integers(0, H)), int(rng.integers(0, W))] = 1.5e308 * rng.choice([-1.0, 1.0], F)
    layout = str(rng.choice(SIM_LAYOUTS, p=[0.6, 0.2, 0.2]))
    if layout == "strided":
        big = np.zeros((F, 2 * H, 2 * W + 1), frames.dtype)
        big[:, ::2, 1::2] = frames
        frames = big[:, ::2, 1::2]
    elif layout == "transposed":
        frames = np.ascontiguousarray(frames.transpose(1, 2, 0)).transpose(2, 0, 1)
    # ---- refractory, state
    dT = np.diff(T)
    rk = str(rng.choice(SIM_REFRACTORY, p=[0.4, 0.25, 0.2, 0.15]))
    refractory = {"zero": 0.0, "fraction": 0.3 * float(dT.min()), "interval": float(np.median(dT)), "beyond": 2.0 * float(T[-1] - T[0])}[rk]
    sk = str(rng.choice(SIM_STATES, p=[0.4, 0.2, 0.2, 0.2]))
    reference, last = None, None
    f0 = np.asarray(frames[0]).astype(np.float64)
    if sk == "reference":                                  # several contrasts off frames[0]: a burst at frame_ts[0]
        reference = f0 + float(rng.choice([-1.0, 1.0])) * float(rng.integers(2, 6)) * c0 * (rng.random((H, W)) < 0.7)
    elif sk == "last":
        pool = np.array([-np.inf, np.inf, np.nan, T[0] - dT[0], T[0] + 0.5 * dT[0], T[0]])
        last = rng.choice(pool, (H, W), p=[0.3, 0.15, 0.15, 0.15, 0.15, 0.1])
    elif sk == "both":                                     # the state a previous call leaves: one more frame before frames[0]
        prev = f0 + (rng.integers(-3, 4, (H, W)) * c0 if dyadic else 2.0 * c0 * rng.normal(size=(H, W)))
        prev_t = float(np.nextafter(T[0], -np.inf)) if tk == "neighbours" else float(T[0] - dT[0])
        with np.errstate(all="ignore"):
            reference, last = N.seq_simulate(np.stack([prev, f0]), [prev_t, T[0]], con_map, coff_map, refractory)[4:6]
    c = {"F": F, "H": H, "W": W, "shape": shape, "tk": tk, "T": T, "dtype": dtype, "amp": amp, "special": special, "dyadic": dyadic,
         "frames": frames, "layout": layout, "ck": ck, "mk": mk, "con": con, "coff": coff, "rk": rk, "refractory": refractory, "sk": sk,
         "reference": reference, "last": last, "wide": bool(rng.random() < 0.25), "ik": str(rng.choice(SIM_INPUTS)),
         "tsk": str(rng.choice(SIM_TS_KINDS)), "split": int(rng.integers(1, F - 1)) if F >= 3 else None, "bad": bad, "bad_over": {}}
    # ---- one injected invalid argument: what replaces which argument
    j = int(rng.integers(1, F))
    if bad == "ts_order":
        Tb = T.copy()
        Tb[j] = Tb[j - 1] if rng.random() < 0.5 else np.nextafter(Tb[j - 1], -np.inf)
        c["bad_over"] = {"T": Tb}
    elif bad == "ts_nonfinite":
        Tb = T.copy()
        Tb[j if rng.random() < 0.7 else 0] = float(rng.choice([np.nan, np.inf, -np.inf]))
        c["bad_over"] = {"T": Tb}
    elif bad == "map_shape":
        c["bad_over"] = {"con" if rng.random() < 0.5 else "coff": np.full((H, W + 1), c0)}
    elif bad == "state_shape":
        c["bad_over"] = {"reference": np.zeros((H + 1, W))} if rng.random() < 0.5 else {"last": np.full((H, W, 1), -np.inf)}
    elif bad == "complex":
        c["bad_over"] = {"frames": np.asarray(frames).astype(np.complex128)}
    elif bad == "map_values":
        maps = {"con": np.array(con_map), "coff": np.array(coff_map)}
        for name in (("con",), ("coff",), ("con", "coff"))[int(rng.integers(0, 3))]:
            hit = rng.random((H, W)) < 0.1
            hit[int(rng.integers(0, H)), int(rng.integers(0, W))] = True
            maps[name][hit] = rng.choice([0.0, -0.1, np.nan, np.inf, -np.inf], int(hit.sum()))
        with np.errstate(invalid="ignore"):
            good = {k: np.isfinite(m) & (m > 0) for k, m in maps.items()}
        c["bad_pixels"] = int((~(good["con"] & good["coff"])).sum())
        c["bad_over"] = {k: v for k, v in maps.items() if not good[k].all()}
    elif bad == "overflow_hot":                            # a pixel of 70 000 contrasts between two frames
        fb = np.asarray(frames).astype(np.float64).copy()
        for _ in range(int(rng.integers(1, 3))):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            fb[:j, y, x], fb[j:, y, x] = 0.0, 70000.0 * float(con_map[y, x])
        c["bad_over"] = {"frames": fb, "reference": None, "last": None}
    elif bad == "overflow_inf" and F >= 3:                 # a level of +-inf from frames[0]: inf - c == inf >= L1 for ever
        fb = np.asarray(frames).astype(np.float64).copy()
        y, x, sign = int(rng.integers(0, H)), int(rng.integers(0, W)), float(rng.choice([-1.0, 1.0]))
        fb[0, y, x], fb[1, y, x], fb[2:, y, x] = sign * np.inf, sign, 0.0
        c["bad_over"] = {"frames": fb, "reference": None, "last": None}
    elif bad in ("overflow_tiny", "overflow_inf"):                           # the contrast lies below the ulp of the level: R + c == R, only the limit ends it
        fb = np.full((F, H, W), c0 * 2.0 ** 57)
        for _ in range(int(rng.integers(1, 3))):
            y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
            fb[j:, y, x] = fb[0, y, x] * (1.0 + float(rng.choice([-1.0, 1.0])) * 2.0 ** -40)
        c["bad_over"] = {"frames": fb, "reference": None, "last": None}
    c["desc"] = "simulate %dx%dx%d(%s) t=%s %s(%s%s) amp=%s special=%s c=%s(%s) refractory=%s state=%s in=%s/%s wide=%d split=%s%s" % (
        F, H, W, shape, tk, dtype, layout, ",dyadic" if dyadic else "", amp, special, ck, mk, rk, sk, c["ik"], c["tsk"], c["wide"], c["split"],
        "" if bad is None else " BAD=" + bad)
    return c


def simulate_reference(c, **over):
    """seq_simulate's seven values on the host arrays of the case; `over` replaces arguments (the parts of a split, the invalid ones)"""
    N = _t("_simulate_np")
    a = {k: c[k] for k in ("frames", "T", "con", "coff", "refractory", "reference", "last")}
    a.update(over)
    with np.errstate(all="ignore"):
        return N.seq_simulate(np.asarray(a["frames"]), a["T"], np.asarray(a["con"], np.float64), np.asarray(a["coff"], np.float64), a["refractory"],
                              a["reference"], a["last"])


def _sim_report(got, want, numpy_out, what):
    """the rules of same() in tests/test_gpu_simulate.py, as a report: columns equal with their dtypes, both state images equal with NaN
    in the same places, numpy in -> numpy out and tensors in -> device tensors out"""
    xs, ys, ts, ps, state = got
    for v in (xs, ys, ts, ps) + tuple(state):
        if isinstance(v, np.ndarray) != numpy_out or not (numpy_out or v.is_cuda):
            return "%s: %s out for %s in" % (what, type(v).__name__, "numpy" if numpy_out else "tensors")
    return _first(*(flags_equal(g, w, "%s %s" % (what, k)) for g, w, k in zip((xs, ys, ts, ps), want[:4], "xytp")),
                  equal(state.reference, want[4], what + " reference"), equal(state.last_event_ts, want[5], what + " last_event_ts"))


def case_simulate(rng):
    """simulate_events (and _simulate with wide=1) against seq_simulate: the whole call, a repeat, the two parts of a streaming split
    re-ordered by (t, pixel), and the ValueError of an injected invalid argument with the counts of its message."""
    import re
    from event_utils_amd.simulation import event_simulator as S
    c = simulate_inputs(rng)
    numpy_in = c["ik"] == "numpy"

    def hand(a, device=None):
        """a host array as the case's input kind hands it over"""
        if a is None or np.ndim(a) == 0:
            return a
        if isinstance(a, torch.Tensor):
            return a
        if (device is None and numpy_in) or device is False:
            return a
        t = torch.from_numpy(a)
        return t if (device is None and c["ik"] == "host_tensor") else t.cuda()

    def call(**over):
        a = {k: c[k] for k in ("frames", "T", "con", "coff", "refractory", "reference", "last")}
        a.update(over)
        T = a["T"]
        T = T if isinstance(T, torch.Tensor) else [float(v) for v in T] if c["tsk"] == "list" else T if c["tsk"] == "array" else torch.from_numpy(np.asarray(T))
        maps = [hand(a[k], device=c["mk"].startswith("device")) for k in ("con", "coff")]
        args = (hand(a["frames"]), T, maps[0], maps[1], a["refractory"], hand(a["reference"]), hand(a["last"]))
        return S._simulate(*args, True, wide=1) if c["wide"] else E.simulate_events(*args, return_state=True)

    def body():
        if c["bad"] is not None:                            # the ValueError, then the valid call on the same inputs below
            try:
                call(**c["bad_over"])
                return "%s: no ValueError" % c["bad"]
            except ValueError as e:
                msg = str(e)
            if c["bad"] == "map_values":
                m = re.search(r"\((\d+) pixels of the maps", msg)
                if not m or int(m.group(1)) != c["bad_pixels"]:
                    return "map_values: %r, the restatement counts %d pixels" % (msg, c["bad_pixels"])
            elif c["bad"].startswith("overflow"):
                count = simulate_reference(c, **c["bad_over"])[6]
                m = re.search(r"^(\d+) pixel-intervals exceeded 65536 crossings", msg)
                if not m or int(m.group(1)) != count or count == 0:
                    return "%s: %r, the restatement counts %d pixel-intervals" % (c["bad"], msg, count)
        want = simulate_reference(c)
        if want[6]:
            return "fuzz case: the restatement overflows in a valid case"
        got = call()
        err = _sim_report(got, want, numpy_in, "whole")
        if err is not None:
            return err
        again = call()
        for u, v in zip(got[:4] + tuple(got[4]), again[:4] + tuple(again[4])):
            if _host(u).tobytes() != _host(v).tobytes():
                return "a repeat call gives other bytes"
        if c["split"] is None:
            return None
        k = c["split"]
        x1, y1, t1, p1, s1 = call(frames=c["frames"][:k + 1], T=c["T"][:k + 1])
        x2, y2, t2, p2, s2 = call(frames=c["frames"][k:], T=c["T"][k:], reference=s1.reference, last=s1.last_event_ts)
        x, y, t, p = (np.concatenate([_host(u), _host(v)]) for u, v in ((x1, x2), (y1, y2), (t1, t2), (p1, p2)))
        order = np.lexsort((y * c["W"] + x, t))             # stable: within a pixel, chunk order is emission order
        return _first(*(flags_equal(g[order], w, "split at %d: %s" % (k, name)) for g, w, name in zip((x, y, t, p), want[:4], "xytp")),
                      equal(s2.reference, want[4], "split reference"), equal(s2.last_event_ts, want[5], "split last_event_ts"))
    return _run_case(c["desc"], body)


# ---- the dense-flow losses (evk_flowloss.hip) and motion segmentation (evk_segment.hip) ---------------------------------------------
# The kernels that hand gradients to an optimiser or a network.  flowts_inputs / flowcm_inputs / segment_inputs draw a case on the
# host (plain numpy arrays and settings); flow_reference / segment_reference evaluate tests/_flow_loss_np.py,
# tests/_flow_contrast_np.py and tests/_segmentation_np.py on it; case_flowts / case_flowcm / case_segment run the public calls.
# The comparison rules are those of tests/test_gpu_flow_loss.py, test_gpu_flow_contrast.py and test_gpu_segmentation.py, restated
# below as functions that return a report; profiles/fuzz_flow_segment.txt.

FLOW_SIZES = ("2", "3", "random", "64/65")
FLOW_FIELDS = ("zero", "constant", "smooth", "strong")
FLOW_N = (0, 1, 2, 63, 64, 65, 255, 256, 257, "random")
FLOW_N_WEIGHTS = (0.02, 0.02, 0.03, 0.12, 0.12, 0.12, 0.12, 0.12, 0.12, 0.21)
FLOW_EMPTY = ("none", "first", "middle", "last", "all")          # which samples of a batch are forced empty
FLOW_EMPTY_WEIGHTS = (0.37, 0.2, 0.2, 0.2, 0.03)
FLOW_OFFSETS = ("numpy_i64", "host_i32", "device_i64")
FLOW_POSITIONS = ("real", "integer", "off_support", "far")
FLOW_TIMES = ("u1e-6", "u0.05", "u100", "equal", "two", "f32_1e4")
FLOW_TIMES_WEIGHTS = (0.18, 0.32, 0.18, 0.03, 0.11, 0.18)
FLOW_POLS = ("pm1", "01", "pm1z")
FLOW_SCALES = (1.0, 0.5, -1.0, 100.0)
FLOW_NONFINITE = ("none", "p", "x", "field", "t")
FLOW_BLURS = ("none", "0.5", "1", "2", "wide", "over_canvas")
FLOW_DIRECTIONS = ("forward", "backward", "both")
FLOW_OBJECTIVES = ("variance", "mean_square")
FLOW_WIDE_SIGMA = 8.5                                            # radius 34 > EVK_MAX_RADIUS: evk_gaussian_filter_wide_f32
FLOW_SPANS = {"u1e-6": 1e-6, "u0.05": 0.05, "u100": 100.0, "two": 0.05}


def _flow_times(rng, n, tk):
    """The sorted float32 time stamps of one sample and their nominal span (what the field's speed is scaled by)."""
    if tk == "equal":
        return np.full(n, rng.uniform(0.0, 1.0)).astype(np.float32), 0.0
    if tk == "two":                                              # two distinct values: forward tau is 0 or D / (D + 1e-6)
        t = np.full(n, 0.25)
        if n >= 2:
            t[int(rng.integers(1, n)):] += FLOW_SPANS[tk]
        return t.astype(np.float32), FLOW_SPANS[tk]
    if tk == "f32_1e4":                                          # float32 at 1e4 s has a grid of 2^-10 s: many tied stamps
        span = 1e-3 * max(n, 2)
        return (1e4 + np.sort(rng.uniform(0.0, span, n))).astype(np.float32), span
    span = FLOW_SPANS[tk]
    return np.sort(rng.uniform(0.0, span, n)).astype(np.float32), span


def _flow_field(rng, fk, H, W, span):
    """(2, H, W) float32.  The displacement over the sample's span is what is drawn -- up to min(3, 0.3 min(H, W)) px for the
    constant and the smooth field (the smooth one is tests/_flow_loss_np.py's scene: 60 px/s over 0.05 s), 1.5 max(H, W) px for
    the strong one, which sends most events off the canvas -- and divided by the span (0.05 s where the span is zero)."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    amp = min(3.0, 0.3 * min(H, W))
    if fk == "zero":
        f = np.zeros((2, H, W))
    elif fk == "constant":
        f = rng.uniform(-amp, amp, 2)[:, None, None] * np.ones((2, H, W))
    else:
        amp = amp if fk == "smooth" else 1.5 * max(H, W)
        ph = rng.uniform(0.0, 2.0 * np.pi, 2)
        f = amp * np.stack([np.sin(0.31 * xx + 0.17 * yy + ph[0]), np.cos(0.23 * xx - 0.29 * yy + ph[1])])
        f = f + rng.normal(0.0, 0.1 * amp, f.shape)
    return (f / (span if span > 0 else 0.05)).astype(np.float32)


def _flow_positions(rng, pk, n, H, W):
    x, y = rng.uniform(0.0, W - 1.0, n), rng.uniform(0.0, H - 1.0, n)
    if pk == "integer":                                          # sensor pixels, the column W - 1 and the row H - 1 included
        x, y = rng.integers(0, W, n).astype(np.float64), rng.integers(0, H, n).astype(np.float64)
        if n >= 2:
            x[int(rng.integers(0, n))], y[int(rng.integers(0, n))] = W - 1.0, H - 1.0
    elif pk == "off_support":                                    # beside the field's support: fl_sample pads with zeros there
        for a, size in ((x, W), (y, H)):
            k = rng.random(n) < 0.3
            side = rng.random(n) < 0.6
            a[k & side] = rng.uniform(size - 1.0, size + 2.0, n)[k & side]
            a[k & ~side] = rng.uniform(-2.0, 0.0, n)[k & ~side]
        if n >= 2:                                               # one event for certain between the last column and the canvas edge
            x[int(rng.integers(0, n))] = W - 1.0 + float(rng.uniform(0.05, 0.95))
    elif pk == "far" and n:
        k = rng.integers(0, n, min(n, 3))
        x[k] = rng.choice([-1e4, 1e4], len(k))
        y[k[:1]] = rng.choice([-1e4, 1e4])
    return x.astype(np.float32), y.astype(np.float32)


def _flow_pol(rng, pk, n):
    if pk == "pm1":
        return (rng.integers(0, 2, n) * 2.0 - 1.0).astype(np.float32)
    if pk == "01":
        return rng.integers(0, 2, n).astype(np.float32)
    if pk == "pm1z":
        return rng.integers(-1, 2, n).astype(np.float32)
    mag = 10.0 ** rng.uniform(-3.0, 3.0)                         # 'real': one magnitude per sample, so that a batch holds
    return (rng.choice([-1.0, 1.0], n) * mag * rng.uniform(0.5, 1.0, n)).astype(np.float32)   # fixed-point exponents far apart


def _flow_inputs(rng, kind):
    """One case of flow_field_timestamp_loss ('flowts') or flow_field_contrast_loss ('flowcm'), drawn on the host: one value per
    axis, independently -- field size and kind, batch, event counts, offsets kind, positions, times, polarities, polarity factor,
    one isolated NaN, blur, direction (and objective, use_polarity).  Every column holds float32 values; samples are sorted."""
    cm = kind == "flowcm"
    sizes = [str(rng.choice(FLOW_SIZES)) for _ in range(2)]
    H, W = ({"2": 2, "3": 3, "random": int(rng.integers(4, 41)), "64/65": int(rng.choice([64, 65]))}[s] for s in sizes)
    fk = str(rng.choice(FLOW_FIELDS, p=(0.2, 0.2, 0.5, 0.1)))
    batched = bool(rng.random() < 0.65)
    B = int(rng.integers(1, 6)) if batched else 1
    empty = str(rng.choice(FLOW_EMPTY, p=FLOW_EMPTY_WEIGHTS)) if batched else "none"
    if (empty == "middle" and B < 3) or (empty in ("first", "last") and B < 2):
        B = 3
    ok_ = str(rng.choice(FLOW_OFFSETS)) if batched else "none"
    pk = str(rng.choice(FLOW_POSITIONS))
    tk0 = str(rng.choice(FLOW_TIMES, p=FLOW_TIMES_WEIGHTS))
    mixed = bool(batched and rng.random() < 0.4)                 # every sample its own kind of time stamps
    polk = str(rng.choice(FLOW_POLS + (("real",) if cm else ())))
    scale = float(rng.choice(FLOW_SCALES))
    nf = str(rng.choice(FLOW_NONFINITE, p=(0.6, 0.1, 0.1, 0.1, 0.1)))
    bk = str(rng.choice(FLOW_BLURS))
    direction = str(rng.choice(FLOW_DIRECTIONS))
    objective = str(rng.choice(FLOW_OBJECTIVES)) if cm else None
    use_polarity = bool(rng.random() < 0.7) if cm else True
    ch, cw = H + 1, W + 1
    sigma = {"none": float(rng.choice([0.0, -1.0])), "0.5": 0.5, "1": 1.0, "2": 2.0, "wide": FLOW_WIDE_SIGMA,
             "over_canvas": (min(ch, cw) * float(rng.uniform(1.0, 2.5)) + 1.0) / 4.0}[bk]      # radius = int(4 sigma + 0.5) > min(ch, cw)
    ns, tks, flows, cols = [], [], [], []
    for b in range(B):
        n = FLOW_N[int(rng.choice(len(FLOW_N), p=FLOW_N_WEIGHTS))]
        n = int(rng.integers(258, 4001)) if n == "random" else int(n)
        if empty == "all" or (empty == "first" and b == 0) or (empty == "last" and b == B - 1) or (empty == "middle" and b == B // 2):
            n = 0
        elif empty != "none":
            n = max(n, 1)
        tk = str(rng.choice(FLOW_TIMES, p=FLOW_TIMES_WEIGHTS)) if mixed else tk0
        t, span = _flow_times(rng, n, tk)
        x, y = _flow_positions(rng, pk, n, H, W)
        if tk == "two" and n >= 2:                                # the same pixels fire at both times: the timestamp loss has a
            k = int(np.searchsorted(t, t[-1]))                   # gradient only where events of the two groups meet
            x[k:], y[k:] = np.resize(x[:k], n - k), np.resize(y[:k], n - k)
        ns.append(n)
        tks.append(tk)
        flows.append(_flow_field(rng, fk, H, W, span))
        cols.append((x, y, t, _flow_pol(rng, polk, n)))
    flow = np.stack(flows)
    x, y, t, p = (np.concatenate([c[k] for c in cols]) for k in range(4))
    offsets = np.concatenate([[0], np.cumsum(ns)]).astype(np.int64)
    where = None
    if nf != "none":                                             # one NaN: a polarity, an x, a field cell, or an interior time stamp
        need = 3 if nf == "t" else 1
        cand = [b for b in range(B) if ns[b] >= need]
        if nf == "field":
            where = (int(rng.integers(0, B)), int(rng.integers(0, 2)), int(rng.integers(0, H)), int(rng.integers(0, W)))
            flow[where] = np.nan
        elif not cand:
            nf = "none"
        else:
            b = int(rng.choice(cand))
            where = int(offsets[b]) + (int(rng.integers(1, ns[b] - 1)) if nf == "t" else int(rng.integers(0, ns[b])))
            {"p": p, "x": x, "t": t}[nf][where] = np.nan
    desc = "%s %dx%d %s B=%s n=%s empty=%s offsets=%s pos=%s t=%s p=%s scale=%g nan=%s sigma=%.4g (%s) %s%s" % (
        kind, H, W, fk, B if batched else "-", ns, empty, ok_, pk, sorted(set(tks)), polk, scale, nf, sigma, bk, direction,
        (" %s use_polarity=%d" % (objective, use_polarity)) if cm else "")
    return dict(desc=desc, kind=kind, H=H, W=W, sizes=sizes, fk=fk, batched=batched, B=B, empty=empty, ok=ok_, pk=pk, tks=tks, mixed=mixed,
                polk=polk, scale=scale, nf=nf, where=where, bk=bk, sigma=sigma, direction=direction, objective=objective,
                use_polarity=use_polarity, ns=ns, flow=flow, cols=(x, y, t, p), offsets=offsets)


def flowts_inputs(rng):
    return _flow_inputs(rng, "flowts")


def flowcm_inputs(rng):
    return _flow_inputs(rng, "flowcm")


def _flow_module(kind):
    return _t("_flow_loss_np" if kind == "flowts" else "_flow_contrast_np")


def _flow_samples(c):
    """(b, flow (2, H, W), the four columns) of every sample"""
    off = c["offsets"]
    return [(b, c["flow"][b], tuple(col[off[b]:off[b + 1]] for col in c["cols"])) for b in range(c["B"])]


def flow_reference(c, warped=None, **more):
    """[(loss, gradient (2, H, W))] per sample from the restatement with f32_coords=True; warped[b]: what the restatement takes
    as warped= for sample b (the device's warp_events_flow_torch), None: the restatement's own float32 warp."""
    M, ts = _flow_module(c["kind"]), c["kind"] == "flowts"
    out = []
    for b, flow, cols in _flow_samples(c):
        if len(cols[0]) == 0:
            out.append((0.0, np.zeros(flow.shape)))
            continue
        kw = dict(f32_coords=True, warped=None if warped is None else warped[b], p_scale=c["scale"], **more)
        with np.errstate(all="ignore"):
            if ts:
                out.append(M.loss_and_grad(flow, *cols, c["sigma"], c["direction"], **kw))
            else:
                out.append(M.loss_and_grad(flow, *cols, c["sigma"], c["objective"], c["direction"], use_polarity=c["use_polarity"], **kw))
    return out


def flow_kept(c, b, direction):
    """The mask of sample b's events that count in `direction`, by the restatement's own float32 warp (no GPU)."""
    M = _flow_module(c["kind"])
    _, flow, cols = _flow_samples(c)[b]
    if len(cols[0]) == 0:
        return np.zeros(0, bool)
    with np.errstate(all="ignore"):
        if c["kind"] == "flowts":
            return M._events(flow, *cols, direction, True, None, c["scale"])[1]
        return M._events(flow, *cols, direction, True, None, c["scale"], c["use_polarity"])[1]


def _tbytes(a):
    return (a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)).tobytes()


def _same_bits(got, want, what):
    """bit equality of results of the same call made another way: (loss, gradient) pairs or single tensors"""
    got, want = (v if isinstance(v, (tuple, list)) else (v,) for v in (got, want))
    for g, w in zip(got, want):
        if tuple(g.shape) != tuple(w.shape) or _tbytes(g) != _tbytes(w):
            return "%s: other bits" % what
    return None


def close_planes(got, ref, what):
    """tests/test_gpu_flow_loss.py::_close_planes: per plane, atol = 1e-6 x the plane's maximum"""
    got, ref = np.asarray(_host(got), np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return "%s: shape %s vs %s" % (what, got.shape, ref.shape)
    got, ref = got.reshape((-1,) + ref.shape[-2:]), ref.reshape((-1,) + ref.shape[-2:])
    for k in range(ref.shape[0]):
        tol = 1e-6 * max(np.abs(ref[k]).max(), 1e-30)
        err = np.abs(got[k] - ref[k]).max()
        if not err <= tol:
            return "%s: plane %d max error %.3e > %.3e" % (what, k, err, tol)
    return None


def close_loss(got, ref, what, extra=0.0):
    """loss rtol = 1e-4; a reference of exactly zero is to be met exactly.  extra: an absolute allowance derived on the CPU."""
    got, ref = float(got), float(ref)
    if ref == 0.0 and extra == 0.0:
        return None if got == 0.0 else "%s: %r where the restatement has exactly 0" % (what, got)
    return None if abs(got - ref) <= 1e-4 * abs(ref) + extra else "%s: %.9g vs %.9g (|diff| %.3e > %.3e)" % (
        what, got, ref, abs(got - ref), 1e-4 * abs(ref) + extra)


def close_grad(got, ref, what, extra=0.0):
    """gradient rtol = 1e-4 with atol = 1e-4 max |g_ref|; where the reference is exactly zero everywhere, so is the kernel's"""
    got, ref = np.asarray(_host(got), np.float64), np.asarray(ref, np.float64)
    if got.shape != ref.shape:
        return "%s: shape %s vs %s" % (what, got.shape, ref.shape)
    if not ref.any() and extra == 0.0:
        return None if not got.any() else "%s: max |g| %.3e where the restatement's gradient is exactly zero" % (what, np.abs(got).max())
    tol = 1e-4 * np.abs(ref) + 1e-4 * np.abs(ref).max() + extra
    bad = ~(np.abs(got - ref) <= tol)
    if bad.any():
        k = int(np.argmax(np.where(bad, np.abs(got - ref) - tol, -np.inf)))
        return "%s: %d of %d components; worst %.9g vs %.9g (max |g_ref| %.3e, allowance %.3e)" % (
            what, int(bad.sum()), ref.size, got.reshape(-1)[k], ref.reshape(-1)[k], np.abs(ref).max(), extra)
    return None


def _flow_forms(c):
    """The events of a case in the four forms a caller may hand over: a DeviceEvents carrying the polarity factor (the primary
    form), numpy columns, device tensors, device tensors that start 4 bytes off a 16-byte boundary.  The three others hold the
    factor multiplied out in float32 (0.5, -1 and 100 are exact, so the product is the one rounding the kernel makes)."""
    x, y, t, p = c["cols"]
    ev = E.DeviceEvents.from_arrays(x, y, t, p, precision="f32")
    if c["scale"] != 1.0:
        ev = ev.scaled(c["scale"])
    with np.errstate(all="ignore"):
        ps = (p.astype(np.float64) * c["scale"]).astype(np.float32)
    host = (x, y, t, ps)
    tens = tuple(torch.from_numpy(a).cuda() for a in host)
    padded = tuple(torch.cat((a.new_zeros(1), a))[1:] for a in tens)
    if len(x) and not all(a.data_ptr() % 16 == 4 for a in padded):
        raise AssertionError("fuzz case: the padded columns are not 4 bytes off a 16-byte boundary")
    return {"events": (ev, None, None, None), "numpy": host, "tensor": tens, "slice": padded}, host


def _flow_offsets(c):
    if not c["batched"]:
        return None
    return {"numpy_i64": lambda o: o, "host_i32": lambda o: torch.from_numpy(o.astype(np.int32)),
            "device_i64": lambda o: torch.from_numpy(o).cuda()}[c["ok"]](c["offsets"])


def _flow_warped(c, directions):
    """per sample: what warp_events_flow_torch returns for its events, per direction (the dedicated tests' _warped)"""
    out = []
    for b, flow, cols in _flow_samples(c):
        if len(cols[0]) == 0:
            out.append(None)
            continue
        x, y, t, p = (torch.from_numpy(a) for a in cols)
        per = []
        for d in directions:
            t0 = float(cols[2][-1] if d == "forward" else cols[2][0])
            xw, yw = E.transforms.warp_events_flow_torch(x, y, t, p, torch.from_numpy(flow), t0=t0)
            per.append((_host(xw), _host(yw)))
        out.append(tuple(per) if len(per) == 2 else per[0])
    return out


F32_MARGIN, F32_DRAWS = 4.0, 8


def _f32_runs():
    """f32_images of the restatements, run by run: the plain float32 storage, then F32_DRAWS realisations of its last place"""
    rng = np.random.default_rng(0)
    return [True] + [rng] * F32_DRAWS


def flow_allowance(c, warped, ref):
    """What the float32 post pass of the contrast loss may add to the dedicated tests' tolerances, per sample, measured on the CPU
    and taken only where those tolerances are exceeded: F32_MARGIN x the largest |restatement with float32 images - restatement
    in float64| over the plain float32 storage and F32_DRAWS realisations of its last place, for the loss and for the largest
    gradient component.  Negligible where the dedicated tests compare (var(B) >= 1e-2 mean(B)^2); where B is nearly constant -- a
    blur wider than the canvas -- it is all that float32 images leave of var(B) and of the slopes of G, and it comes in whole
    units of the last place of S, so one realisation may show none of it; the same where a single event sits on the top of its
    own wide blob, whose slope there is a difference of nearly equal cells (profiles/fuzz_flow_segment.txt).  The timestamp loss
    has no such cancellation (sum B^2; slopes of S / (1 + C)) and gets no allowance."""
    out = [[0.0, 0.0] for _ in range(c["B"])]
    if c["kind"] == "flowcm":
        for run in _f32_runs():
            for o, a, b in zip(out, flow_reference(c, warped, f32_images=run), ref):
                o[0], o[1] = max(o[0], abs(a[0] - b[0])), max(o[1], float(np.abs(a[1] - b[1]).max()))
    return [(F32_MARGIN * o[0], F32_MARGIN * o[1]) for o in out]


def _case_flow(c):
    """The public calls of one flow kind against the restatement (warped= rule, the dedicated tests' tolerances, no case and
    no pixel excluded), and bit for bit: a second call, the value alone, every form of input, a batch against its samples run
    singly, 'both' against forward plus backward, the autograd function against the explicit calls."""
    ts = c["kind"] == "flowts"
    M = _flow_module(c["kind"])
    loss_fn, auto_fn, img_fn = (E.flow_field_timestamp_loss, E.flow_timestamp_loss, E.flow_field_timestamp_images) if ts else \
        (E.flow_field_contrast_loss, E.flow_contrast_loss, E.flow_field_iwe)
    kw = dict(blur_sigma=c["sigma"], direction=c["direction"])
    ikw = {}
    if not ts:
        kw.update(objective=c["objective"], use_polarity=c["use_polarity"])
        ikw.update(use_polarity=c["use_polarity"])
    B, batched = c["B"], c["batched"]
    field = c["flow"] if batched else c["flow"][0]

    def body():
        forms, host = _flow_forms(c)
        off = _flow_offsets(c)
        loss, grad = loss_fn(field, *forms["events"], offsets=off, compute_gradient=True, **kw)
        if loss.dtype != torch.float64 or grad.dtype != torch.float32 or tuple(grad.shape) != field.shape or \
                tuple(loss.shape) != ((B,) if batched else ()):
            return "result: %s%s %s%s" % (loss.dtype, tuple(loss.shape), grad.dtype, tuple(grad.shape))
        losses, grads = _host(loss).reshape(B), _host(grad).reshape((B,) + c["flow"].shape[1:])
        directions = M.DIRECTIONS if c["direction"] == "both" else (c["direction"],)
        warped = _flow_warped(c, directions)
        ref = flow_reference(c, warped)
        def against(allow):
            return _first(*(close_loss(losses[b], ref[b][0], "loss[%d]" % b, allow[b][0]) or
                            close_grad(grads[b], ref[b][1], "gradient[%d]" % b, allow[b][1]) for b in range(B)))
        err = against([(0.0, 0.0)] * B)
        if err is not None and not ts:
            err = against(flow_allowance(c, warped, ref))
        if err is not None:
            return err
        for k, d in enumerate(directions):                       # the planes behind the loss, through the public image calls
            img = _host(img_fn(field, *forms["events"], direction=d, offsets=off, **ikw))
            img = img.reshape((B,) + img.shape[(1 if batched else 0):])
            for b, flow, cols in _flow_samples(c):
                w = None if warped[b] is None else (warped[b][k] if len(directions) == 2 else warped[b])
                with np.errstate(all="ignore"):
                    if len(cols[0]) == 0:
                        want = np.zeros(img[b].shape)
                    elif ts:
                        want = M.images(flow, *cols, direction=d, f32_coords=True, warped=w, p_scale=c["scale"])
                    else:
                        want = M.iwe(flow, *cols, direction=d, f32_coords=True, warped=w, p_scale=c["scale"], use_polarity=c["use_polarity"])
                err = close_planes(img[b], want, "%s image[%d]" % (d, b))
                if err is not None:
                    return err
        first = (loss, grad)
        err = _same_bits(loss_fn(field, *forms["events"], offsets=off, compute_gradient=True, **kw), first, "a second call") or \
            _same_bits(loss_fn(field, *forms["events"], offsets=off, **kw), loss, "the value alone")
        for name in ("numpy", "tensor", "slice"):
            err = err or _same_bits(loss_fn(torch.from_numpy(field).cuda(), *forms[name], offsets=off, compute_gradient=True, **kw), first,
                                    "%s input" % name)
        if err is not None:
            return err
        if batched:
            o = c["offsets"]
            for b in range(B):
                one = loss_fn(c["flow"][b], *(a[o[b]:o[b + 1]] for a in host), compute_gradient=True, **kw)
                err = _same_bits(one, (loss[b], grad[b]), "sample %d run singly" % b)
                if err is not None:
                    return err
        if c["direction"] == "both":
            parts = [loss_fn(field, *forms["events"], offsets=off, compute_gradient=True, **dict(kw, direction=d)) for d in M.DIRECTIONS]
            err = _same_bits((parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]), first, "forward plus backward")
            if err is not None:
                return err
        leaf = torch.from_numpy(field).cuda().requires_grad_(True)
        out = auto_fn(leaf, *forms["events"], offsets=off, **kw)
        if not out.requires_grad:
            return "autograd: the loss of a leaf that requires a gradient does not"
        out.sum().backward()
        return _same_bits((out.detach(), leaf.grad), first, "autograd")
    return _run_case(c["desc"], body)


def case_flowts(rng):
    return _case_flow(flowts_inputs(rng))


def case_flowcm(rng):
    return _case_flow(flowcm_inputs(rng))


SEG_CANVASES = ("tiny", "one_band", "bands8", "no_band", "multi")
SEG_N = (0, 1, 2, 3, 4, 5, 1023, 1024, 1025, 1026, 16383, 16384, 16385, 16386, 32769)
SEG_N_WEIGHTS = (0.015, 0.02, 0.025, 0.09, 0.09, 0.09, 0.1125, 0.1125, 0.1125, 0.1125, 0.05, 0.05, 0.05, 0.04, 0.03)
SEG_PROBS = ("dirichlet", "one_hot", "zeros", "zero_row", "none")
SEG_POLS = ("pm1", "pm1z", "nan")
SEG_BLURS = ("0", "1", "wide")
SEG_MOTIONS = ("still", "small", "mixed")                     # 'mixed': some clusters push a part of the events off the canvas


def _seg_params(rng, Z, model, H, W, T, strong):
    """The parameters of one cluster as displacements over the stream's span T (zhu_inputs' scales); strong: a motion that takes
    a good part of the events across the canvas' borders."""
    px_ = float(rng.choice([0.0, 1.0, 3.0])) * min(1.0, 0.1 * min(H, W))
    lin = float(rng.choice([0.0, 0.02, 0.06]))
    if strong:
        px_, lin = 0.7 * max(H, W), 0.3
    if model == Z.LINVEL:
        return rng.normal(size=2) * px_ / T
    if model == Z.ROTATION:
        return np.array([rng.uniform(-W, 2 * W), rng.uniform(-H, 2 * H), rng.normal() * (lin + 0.01 * px_) / T])
    if model == Z.XYZTHETA:
        return np.array([rng.normal() * px_, rng.normal() * px_, rng.normal() * lin, rng.normal() * lin]) / T
    if model == Z.ANGVEL:
        axis = rng.normal(size=3)
        return axis / np.linalg.norm(axis) * float(rng.choice([0.0, 0.02, 0.1]) if not strong else 0.6) / T
    half = 0.5 * max(W, H, 2)
    return np.array([rng.normal() * px_, rng.normal() * lin, rng.normal() * lin, rng.normal() * px_, rng.normal() * lin,
                     rng.normal() * lin, rng.normal() * lin / half, rng.normal() * lin / half]) / T


def segment_inputs(rng):
    """One case of cluster_iwes / segmentation_loss / update_assignments, drawn on the host: model, clusters, column dtype, canvas
    class (evk_seg_band_rows itself names the band geometry), event count, associations, polarities, blur, motions."""
    Z, M8 = _t("_zhu_np"), _t("_motion_models8_np")
    _lib, lib = _lib_geometry()
    model = str(rng.choice(Z.MODELS))
    L = int(rng.integers(1, 9))
    f64 = bool(rng.random() < 0.35)
    ck = str(rng.choice(SEG_CANVASES, p=(0.25, 0.25, 0.25, 0.08, 0.17)))
    n = int(SEG_N[int(rng.choice(len(SEG_N), p=SEG_N_WEIGHTS))])
    if ck == "tiny":
        H, W = int(rng.integers(2, 9)), int(rng.integers(2, 9))
    elif ck == "one_band":
        H, W = int(rng.integers(10, 61)), int(rng.integers(10, 81))
        H = min(H, lib.evk_seg_band_rows(L, 0, H + 1, W + 1) - 1)
    elif ck == "bands8":                                          # bands of nine, three and two rows: most events straddle a band edge
        L, H, W = 8, int(rng.integers(8, 17)), int(rng.choice([256, 700, 900]))
    elif ck == "no_band":                                         # too many bands for the LDS kernel: the public default runs k_seg_direct
        L, H, W = int(rng.integers(1, 3)), int(rng.integers(200, 211)), int(rng.integers(2556, 2563))
        n = min(n, 16386)
    else:
        H, W = int(rng.integers(60, 201)), int(rng.integers(150, 401))
    rows = lib.evk_seg_band_rows(L, 0, H + 1, W + 1)
    bands = -(-(H + 1) // rows) if rows else 0
    if (ck == "no_band") != (rows == 0) or (ck == "one_band" and bands != 1):
        raise AssertionError("fuzz case: band geometry %s: rows %d bands %d for L=%d %dx%d" % (ck, rows, bands, L, H + 1, W + 1))
    chunks = min(max(256 // max(bands, 1), 1), -(-n // 16384)) if rows else 0           # chunk_plan (evk_warp_models.h)
    T = float(rng.choice([0.1, 0.5]))
    mx, my = min(3.0, 0.05 * W + 0.5), min(3.0, 0.05 * H + 0.5)
    x, y = rng.uniform(-mx, W + mx, n), rng.uniform(-my, H + my, n)
    t = np.sort(rng.uniform(0.0, T, n))
    polk = str(rng.choice(SEG_POLS, p=(0.5, 0.3, 0.2)))
    p = (rng.integers(0, 2, n) * 2.0 - 1.0) if polk != "pm1z" else rng.integers(-1, 2, n).astype(np.float64)
    if polk == "nan":
        if n:
            p[int(rng.integers(0, n))] = np.nan
        else:
            polk = "pm1"
    use_polarity = bool(rng.random() < 0.5)
    if not f64:
        x, y, t, p = (a.astype(np.float32) for a in (x, y, t, p))
    center, K = (0.0, 0.0), M8.K_DEFAULT
    if model in (Z.XYZTHETA, Z.PLANAR):
        center = (float(rng.uniform(0, W)), float(rng.uniform(0, H)))
    if model == Z.ANGVEL:
        f = max(W, 2) * float(np.exp(rng.uniform(np.log(0.5), np.log(4.0))))
        K = np.array([[f, 0.0, rng.uniform(0.2 * W, 0.8 * W)], [0.0, f * rng.uniform(0.7, 1.4), rng.uniform(0.2 * H, 0.8 * H)], [0.0, 0.0, 1.0]])
    mk = str(rng.choice(SEG_MOTIONS, p=(0.15, 0.45, 0.4)))
    strong = rng.random(L) < 0.4 if mk == "mixed" else np.zeros(L, bool)
    if mk == "mixed" and L > 1:
        strong[int(rng.integers(0, L))], strong[int(rng.integers(0, L))] = True, False          # (the second wins when they coincide)
    q = np.stack([_seg_params(rng, Z, model, H, W, T, bool(s)) for s in strong])
    if mk == "still":
        q = q * 0.0 if model != Z.ROTATION else q * np.array([1.0, 1.0, 0.0])
    prk = str(rng.choice(SEG_PROBS))
    if prk == "zero_row" and L == 1:                              # (the only row: nothing left to compare)
        prk = "dirichlet"
    probs = np.ascontiguousarray(rng.dirichlet(np.ones(L), n).T, dtype=np.float32).reshape(L, n)
    if prk == "one_hot":
        probs = (np.arange(L)[:, None] == rng.integers(0, L, n)[None, :]).astype(np.float32)
    elif prk == "zeros":
        probs[rng.random((L, n)) < 0.3] = 0.0
    elif prk == "zero_row":
        probs[int(rng.integers(0, L))] = 0.0
    elif prk == "none":
        probs = None
    pdev = bool(rng.random() < 0.5)
    bk = str(rng.choice(SEG_BLURS, p=(0.3, 0.5, 0.2)))
    sigma = {"0": 0.0, "1": 1.0, "wide": FLOW_WIDE_SIGMA}[bk]
    desc = "segment %s L=%d %s img=%dx%d (%s: rows %d, bands %d, chunks %d) n=%d probs=%s%s p=%s use_polarity=%d sigma=%g motions=%s" % (
        model, L, "f64" if f64 else "f32", H, W, ck, rows, bands, chunks, n, prk, "/device" if pdev else "", polk, use_polarity, sigma, mk)
    return dict(desc=desc, model=model, L=L, f64=f64, ck=ck, img_size=(H, W), rows=rows, bands=bands, chunks=chunks, n=n, cols=(x, y, t, p),
                polk=polk, use_polarity=use_polarity, center=center, K=K, mk=mk, strong=strong, q=q, prk=prk, probs=probs, pdev=pdev,
                bk=bk, sigma=sigma)


def _seg_probs(c):
    """the associations the kernels see: probs=None is the uniform 1 / L"""
    return np.full((c["L"], c["n"]), 1.0 / c["L"], dtype=np.float32) if c["probs"] is None else c["probs"]


def segment_reference(c):
    """tests/_segmentation_np.py with f32_coords=True on a case: planes, loss, gradient, the assignment step and -- for the rule
    that a row is kept -- which events have no positive c for certain: under every cluster off the canvas, on four cells of B
    that are exactly zero, or with s B at least 1e-6 max |B| below zero."""
    S = _t("_segmentation_np")
    kw = dict(img_size=c["img_size"], use_polarity=c["use_polarity"], center=c["center"], camera_matrix=c["K"], f32_coords=True)
    probs, (x, y, t, p), n = _seg_probs(c), c["cols"], c["n"]
    with np.errstate(all="ignore"):
        planes = S.iwes(c["model"], c["q"], probs, x, y, t, p, **kw)
        loss, grad = S.loss_and_grad(c["model"], c["q"], probs, x, y, t, p, c["sigma"], **kw)
        new, labels, ssum, cc, blurred = S.assign(c["model"], c["q"], probs, x, y, t, p, c["sigma"], **kw)
        zero = np.ones(n, bool)
        if n:
            bmax = np.abs(blurred).max()
            sgn = np.where(np.asarray(p, np.float64) > 0, 1.0, -1.0) if c["use_polarity"] else np.ones(n)
            ces = S._cluster_events(c["model"], c["q"], x, y, t, p, c["img_size"], c["center"], c["K"], True)
            for l, (idx, px, py, dx, dy, _, _) in enumerate(ces):
                b = blurred[l]
                cells = np.stack([b[py, px], b[py, px + 1], b[py + 1, px], b[py + 1, px + 1]])
                zero[idx] &= ~cells.any(axis=0) | (sgn[idx] * S._bilinear(b, px, py, dx, dy) <= -1e-6 * bmax)
    return dict(probs=probs, planes=planes, loss=loss, grad=grad, new=new, labels=labels, S=ssum, blurred=blurred, zero=zero & (ssum == 0))


def seg_assign_report(c, r, new, labels):
    """The rules of tests/test_gpu_segmentation.py::test_assignment_matches_the_restatement for rows and labels: P' within
    (1 + L) 5e-5 where the reference's S >= 0.02 max |B|; labels equal there unless the reference's two largest probabilities are
    within 1e-3; where no c is positive for certain the row is kept bit for bit and the label is its argmax."""
    new, labels, L = _host(new), _host(labels), c["L"]
    if new.shape != (L, c["n"]) or new.dtype != np.float32 or labels.shape != (c["n"],) or labels.dtype != np.int32:
        return "assignment: %s%s %s%s" % (new.dtype, new.shape, labels.dtype, labels.shape)
    if c["n"] == 0:
        return None
    rn, bmax = r["new"].astype(np.float64), np.abs(r["blurred"]).max()
    sure = (r["S"] > 0) & (r["S"] >= 0.02 * bmax)
    err = np.abs(new[:, sure].astype(np.float64) - rn[:, sure])
    if err.size and not err.max() <= (1 + L) * 5e-5:
        return "assignment: P' off by %.3e > %.3e at an event with S >= 0.02 max |B|" % (err.max(), (1 + L) * 5e-5)
    top = np.sort(rn, axis=0)
    clear = sure & ((top[-1] - top[-2] >= 1e-3) if L > 1 else True)
    zero = r["zero"]
    if not np.array_equal(new[:, zero].view(np.uint32), r["probs"][:, zero].view(np.uint32)):
        return "assignment: a row without a positive c is not kept bit for bit"
    check = clear | zero
    if not np.array_equal(labels[check], r["labels"][check]):
        return "assignment: %d labels differ" % int((labels[check] != r["labels"][check]).sum())
    return None


def _seg_warp(c):
    Z = _t("_zhu_np")
    return {Z.LINVEL: lambda: E.linvel_warp(), Z.ROTATION: lambda: E.pure_rotation_warp(),
            Z.XYZTHETA: lambda: E.xyztheta_warp(center=c["center"]), Z.ANGVEL: lambda: E.angular_velocity_warp(c["K"]),
            Z.PLANAR: lambda: E.planar_flow_warp(center=c["center"])}[c["model"]]()


def _seg_forms(c):
    """(events, probs) in the four forms: a DeviceEvents (the primary form), numpy columns, device tensors, and a DeviceEvents
    slice that starts one element into its buffers with the associations 4 bytes off a 16-byte boundary."""
    cols, n, L = c["cols"], c["n"], c["L"]
    prec = "f64" if c["f64"] else "f32"
    probs = c["probs"]
    dprobs = None if probs is None else torch.from_numpy(probs).cuda()
    first = dprobs if c["pdev"] else probs
    ev = E.DeviceEvents.from_arrays(*cols, precision=prec)
    padded = [np.concatenate([np.zeros(1, a.dtype), a, np.zeros(3, a.dtype)]) for a in cols]
    part = E.DeviceEvents.from_arrays(*padded, precision=prec).slice(1, 1 + n)
    if n and part.x.data_ptr() % 16 == 0:
        raise AssertionError("fuzz case: the sliced columns are 16-byte aligned")
    sprobs = None
    if probs is not None:
        buf = torch.zeros(L * n + 1, dtype=torch.float32, device="cuda")
        buf[1:] = dprobs.reshape(-1)
        sprobs = buf[1:].reshape(L, n)
    return {"events": ((ev, None, None, None), first), "numpy": (cols, probs if c["pdev"] else dprobs),
            "tensor": (tuple(torch.from_numpy(a).cuda() for a in cols), dprobs), "slice": ((part, None, None, None), sprobs)}


def case_segment(rng):
    """cluster_iwes, segmentation_loss and update_assignments against tests/_segmentation_np.py (f32_coords=True) by the rules of
    tests/test_gpu_segmentation.py, and bit for bit: a second call, the band form against impl='direct', every form of input."""
    c = segment_inputs(rng)

    def body():
        r = segment_reference(c)
        warp, img, L = _seg_warp(c), c["img_size"], c["L"]
        forms = _seg_forms(c)
        kw = dict(use_polarity=c["use_polarity"])

        def run(name):
            ev, probs = forms[name]
            planes = E.cluster_iwes(c["q"], probs, *ev, warp, img, **kw)
            f, g = E.segmentation_loss(c["q"], probs, *ev, warp, img, blur_sigma=c["sigma"], compute_gradient=True, **kw)
            new, labels = E.update_assignments(c["q"], probs, *ev, warp, img, blur_sigma=c["sigma"], **kw)
            return planes, np.float64(f), g, new, labels
        first = run("events")
        planes, f, g, new, labels = first
        if planes.dtype != torch.float32 or tuple(planes.shape) != (L, img[0] + 1, img[1] + 1) or g.shape != c["q"].shape or g.dtype != np.float64:
            return "result: %s%s, gradient %s%s" % (planes.dtype, tuple(planes.shape), g.dtype, g.shape)
        def against(allow):
            return close_loss(f, r["loss"], "loss", allow[0]) or close_grad(g, r["grad"], "gradient", allow[1])
        err = close_planes(planes, r["planes"], "planes") or against((0.0, 0.0))
        if err is not None and not err.startswith("planes") and c["n"]:
            err = against(segment_allowance(c, r))
        err = err or seg_assign_report(c, r, new, labels)
        if err is not None:
            return err
        ev, probs = forms["events"]
        direct = E.cluster_iwes(c["q"], probs, *ev, warp, img, impl="direct", **kw)
        err = _same_bits(direct, planes, "impl='direct'")
        value = E.segmentation_loss(c["q"], probs, *ev, warp, img, blur_sigma=c["sigma"], **kw)
        err = err or (None if _bits(value, f) else "the value alone: %r vs %r" % (value, f))
        for name in ("events", "numpy", "tensor", "slice"):
            err = err or _same_bits(run(name), first, "a second call" if name == "events" else "%s input" % name)
        return err
    return _run_case(c["desc"], body)


def segment_allowance(c, r):
    """flow_allowance for segmentation_loss: the same post pass, once per cluster image."""
    S = _t("_segmentation_np")
    kw = dict(img_size=c["img_size"], use_polarity=c["use_polarity"], center=c["center"], camera_matrix=c["K"], f32_coords=True)
    lo, gr = 0.0, 0.0
    for run in _f32_runs():
        with np.errstate(all="ignore"):
            f, g = S.loss_and_grad(c["model"], c["q"], r["probs"], *c["cols"], c["sigma"], f32_images=run, **kw)
        lo, gr = max(lo, abs(f - r["loss"])), max(gr, float(np.abs(g - r["grad"]).max()) if g.size else 0.0)
    return F32_MARGIN * lo, F32_MARGIN * gr


# ---- raw streams (evk_rawdecode.hip) ---------------------------------------------------------------------------------------------------
# The one kernel whose input is bytes from outside the process, and whose result -- a sequential state machine's -- comes from a scan of
# associative summaries.  raw_inputs draws the words, the cuts, the form of input and the settings on the host; raw_reference runs the
# sequential restatement (tests/_raw_np.py) over the whole stream and over its pieces; case_raw holds the device decoder, through the
# staged and through the direct write, to both.  Every comparison is bitwise.  profiles/fuzz_raw.txt.
RAW_FAMILIES = {3: ("structured", "random", "time_only", "late_time", "dense_vectors", "no_events"),
                2: ("structured", "random", "time_only", "late_time", "no_events")}
RAW_FAMILY_WEIGHTS = {3: (0.27, 0.12, 0.19, 0.18, 0.20, 0.04), 2: (0.35, 0.16, 0.24, 0.20, 0.05)}
RAW_TIME_ONLY = ("up", "loops", "back", "mixed")           # the TIME_HIGH walk of a 'time_only' stream
RAW_LATE = ("chunk0", "later_chunk", "last_word", "never")  # where the first TIME_HIGH of a 'late_time' stream stands
RAW_LATE_WEIGHTS = (0.3, 0.46, 0.1, 0.14)
RAW_N_CLASSES = ("0", "1-15", "16k", "wave", "chunk", "chunks", "scan")
RAW_N_WEIGHTS = (0.02, 0.10, 0.13, 0.14, 0.25, 0.348, 0.012)
RAW_FORMS = ("numpy", "signed", "bytes", "tensor", "slice1", "slice3", "sliceC1", "u8view")
RAW_CUTS = ("anywhere", "chunk_border", "vector_run", "loop_pair", "twice", "first15")
RAW_POLICIES = ("keep", "drop", "raise")
RAW_SENSORS = ("none", "drawn", "all")
RAW_SENSOR_SIZES = ((480, 640), (720, 1280), (1, 1), (2048, 2048), (1024, 40_000), (40_000, 50_000))
RAW_STATES = ("none", "no_time", "time")
RAW_STAGE = 4096                                             # events per staging round of k_raw_write (test_cpu_fuzz_inputs.py holds it
RAW_ROUND_TRIP_SHARE = 0.4                                   # to the kernel file); the share of cases with the encoders' round trip
RAW_MAX_PIECES = 12                                          # of iter_decode_raw: chunk_words is raised until there are no more


def _raw_geometry():
    from event_utils_amd import _lib
    return _lib.EVK_RAW_CHUNK, _lib.EVK_RAW_SCAN_WIDTH


def _raw_types(fmt, words):
    return (words >> 12) if fmt == 3 else (words >> 28)


def _raw_event_words(rng, fmt, k):
    """k words that emit one event each: ADDR_X / CD_OFF, CD_ON with random payloads"""
    if fmt == 3:
        return (0x2000 | rng.integers(0, 4096, k)).astype(np.uint16)
    return ((rng.integers(0, 2, k) << 28) | rng.integers(0, 1 << 28, k)).astype(np.uint32)


def _raw_time_only(rng, fmt, n, tk):
    """TIME_HIGH words -- ascending by one, alternating top / bottom around the loop threshold, descending by small steps, or a mix
    of the three with TIME_LOW -- with one word in eight an event, so that every loop and step shows in a time stamp"""
    bits = 12 if fmt == 3 else 28
    top, dt = (1 << bits) - 1, np.uint16 if fmt == 3 else np.uint32
    start = int(rng.integers(0, top + 1))
    walks = {"up": (start + np.arange(n)) & top,
             # top - bottom lies on both sides of 4085 (EVT3's loop step) and on it
             "loops": np.where(np.arange(n) % 2 == 0, top - rng.integers(0, 16, n), rng.integers(0, 11, n)),
             "back": (start - np.cumsum(rng.integers(0, 4, n))) & top}
    if tk == "mixed":
        pick = rng.integers(0, 3, -(-n // 40) + 1).repeat(40)[:n]
        th = np.choose(pick, [walks["up"], walks["loops"], walks["back"]])
    else:
        th = walks[tk]
    words = ((0x8 << bits) | th).astype(dt)
    r = rng.random(n)
    ev = r < (0.125 if n >= 64 else 0.4)
    words[ev] = _raw_event_words(rng, fmt, int(ev.sum()))
    if fmt == 3:
        low = (r >= 0.97) | ((tk == "mixed") & (r >= 0.7))
        words[low] = 0x6000 | rng.integers(0, 4096, int(low.sum()))
        rows = (r >= 0.95) & ~low
        words[rows] = rng.integers(0, 2048, int(rows.sum()))
    return words


def _raw_late_time(rng, fmt, n, lk, G):
    """a structured stream with no TIME_HIGH before a drawn position: in chunk 0, in a later chunk, the last word, never -> (words,
    the class that the length allowed)"""
    C, _ = _raw_geometry()
    words = (G.structured_evt3 if fmt == 3 else G.structured_evt2)(rng, n, start_time=False)
    if n == 0:
        return words, "never"
    if lk == "later_chunk" and n <= C + 1:
        lk = "chunk0"
    pos = {"chunk0": int(rng.integers(0, min(n, C))), "later_chunk": int(rng.integers(C, n)) if n > C else 0, "last_word": n - 1, "never": n}[lk]
    early = np.flatnonzero(_raw_types(fmt, words[:pos]) == 8)
    words[early] = _raw_event_words(rng, fmt, len(early))
    if pos < n:
        words[pos] = (0x8000 | int(rng.integers(0, 4096))) if fmt == 3 else ((0x8 << 28) | int(rng.integers(0, 1 << 28)))
    return words, lk


def _raw_dense_vectors(rng, n):
    """VECT_BASE_X near 2047 and runs of full and drawn VECT_12 / VECT_8 masks, one of them longer than a chunk where n allows: base_x
    wraps 2^16, x passes 32767, and every lane's events straddle the staging rounds.  Words that keep the base (TIME_HIGH, TIME_LOW,
    ADDR_Y) stand inside the runs."""
    out = [0x8000 | int(rng.integers(0, 4096)), int(rng.integers(0, 2048))]
    one_run = rng.random() < 0.6
    while len(out) < n:
        out.append(0x3000 | (int(rng.integers(0, 2)) << 11) | int(rng.integers(2040, 2048)))
        k = n if one_run else int(rng.integers(40, 3000))
        m = rng.random(k)
        run = np.where(m < 0.7, 0x4FFF, np.where(m < 0.8, 0x50FF, np.where(m < 0.9, 0x4000 | rng.integers(0, 4096, k), 0x5000 | rng.integers(0, 4096, k))))
        other = rng.random(k) < 0.02
        run[other] = rng.choice([0x8000, 0x6000, 0x0000], int(other.sum())) | rng.integers(0, 2048, int(other.sum()))
        out.extend(run.tolist())
    return np.array(out[:n], dtype=np.uint16)


def _raw_no_events(rng, fmt, n, G):
    """behind a TIME_HIGH only words that emit nothing: ADDR_Y, TIME_LOW, TIME_HIGH, triggers, reserved types"""
    if fmt == 3:
        kinds = np.array([0x0, 0x6, 0x8, 0xA] + list(G.RESERVED3))
        words = ((rng.choice(kinds, n) << 12) | rng.integers(0, 4096, n)).astype(np.uint16)
        first = 0x8000
    else:
        kinds = np.array([0x8, 0xA] + list(G.RESERVED2))
        words = ((rng.choice(kinds, n) << 28) | rng.integers(0, 1 << 28, n)).astype(np.uint32)
        first = 0x8 << 28
    if n:
        words[0] = first | int(rng.integers(0, 4096))
    return words


def _raw_plain(rng, fmt, n):
    """more chunks than the scan has lanes: ADDR_X / TIME_LOW words (plain EVT2 events), so that the restatement's loop stays short, with
    the state that must cross the lanes' runs of chunks -- a loop whose halves lie S chunks apart, a base and a row set in chunk 0"""
    C, S = _raw_geometry()
    words = _raw_event_words(rng, fmt, n)
    if fmt == 3:
        tl = rng.integers(0, n, n // 50)
        words[tl] = 0x6000 | rng.integers(0, 4096, len(tl))
        words[0], words[1], words[2] = 0x8FFE, 0x0123, 0x3805
        words[S * C - 1], words[S * C + 5], words[S * C + 9] = 0x8FFF, 0x8001, 0x4081
        words[n - 3] = 0x8000
    else:
        words[[0, S * C - 1, S * C + 1]] = [0x80000001, 0x80000002, 0x80000003]
    return words


def raw_loop_pairs(fmt, words):
    """(i, j): consecutive TIME_HIGH words of an EVT3 stream, at positions i < j, that form a loop"""
    if fmt != 3:
        return np.empty((0, 2), dtype=np.int64)
    pos = np.flatnonzero((words >> 12) == 8)
    h = (words[pos] & 0xFFF).astype(np.int64)
    k = np.flatnonzero(h[:-1] - h[1:] >= 4085)
    return np.stack((pos[k], pos[k + 1]), axis=1)


def raw_word_events(fmt, words, have_time):
    """events that every word emits (a restatement of the emission rule alone, for the coverage of the staging rounds: its sum is
    held to the sequential restatement's count)"""
    t = _raw_types(fmt, words)
    if fmt == 3:
        v = (words & 0xFFF).astype(np.uint16)
        mask = np.where(t == 2, 1, np.where(t == 4, v, np.where(t == 5, v & 0xFF, 0))).astype(np.uint16)
        count = np.unpackbits(mask.view(np.uint8)).reshape(-1, 16).sum(axis=1) if len(words) else np.zeros(0, dtype=np.int64)
    else:
        count = (t <= 1).astype(np.int64)
    timed = np.cumsum(t == 8) - (t == 8) > 0
    return np.where(timed | bool(have_time), count, 0).astype(np.int64)


def _raw_draw_cuts(rng, fmt, words, ncuts):
    """ncuts positions in [0, n] and the class each was drawn from (a class the stream has no place for falls back to 'anywhere')"""
    C, _ = _raw_geometry()
    n, cuts, classes = len(words), [], []
    t = _raw_types(fmt, words)
    while len(cuts) < ncuts:
        k = RAW_CUTS[int(rng.integers(0, len(RAW_CUTS)))]
        pos = None
        if k == "chunk_border" and n >= C - 1:
            pos = min(n, int(rng.integers(1, -(-n // C) + 1)) * C + int(rng.integers(-1, 2)))
        elif k == "vector_run" and fmt == 3:
            inside = np.flatnonzero(((t[1:] == 4) | (t[1:] == 5)) & ((t[:-1] == 4) | (t[:-1] == 5))) + 1
            pos = int(rng.choice(inside)) if len(inside) else None
        elif k == "loop_pair":
            pairs = raw_loop_pairs(fmt, words)
            if len(pairs):
                i, j = pairs[int(rng.integers(0, len(pairs)))]
                pos = int(rng.integers(i + 1, j + 1))
        elif k == "twice" and (cuts or ncuts >= 2):          # an empty piece
            if not cuts:
                cuts.append(int(rng.integers(0, n + 1)))
                classes.append(k)
            pos = int(rng.choice(cuts))
        elif k == "first15":
            pos = int(rng.integers(0, min(n, 15) + 1))
        if pos is None:
            k, pos = "anywhere", int(rng.integers(0, n + 1))
        cuts.append(pos)
        classes.append(k)
    order = np.argsort(cuts, kind="stable")
    return [cuts[i] for i in order], [classes[i] for i in order]


def _raw_round_trip(rng, fmt):
    """events in order of time with x, y < 2048 (rows read left to right inside bursts of one microsecond, so that vectors form) and
    their words from the package's encoder"""
    n = int(rng.choice([0, 1, 2, 17, 300, 1500, 4000]))
    span = int(rng.choice([50, 5000, 1 << 20, 1 << 25]))
    t0 = int(rng.integers(0, 1 << (27 if fmt == 3 else 33)))
    t = np.repeat(np.sort(t0 + rng.integers(0, span, n // 8 + 1)), 8)[:n]
    y = np.repeat(rng.integers(0, 2048, n // 4 + 1), 4)[:n]
    p = np.repeat(rng.integers(0, 2, n // 4 + 1), 4)[:n]
    x = np.repeat(rng.integers(0, 2010, n // 4 + 1), 4)[:n] + np.tile(np.array([0, 1, 9, 14, 0, 2, 5, 30]), n // 8 + 1)[:n]
    if n > 2:
        x[-1], y[-1], x[0], y[0] = 2047, 2047, 2047, 0
    vectorize = bool(rng.integers(0, 2))
    words = E.encode_evt3(x, y, t, p, vectorize=vectorize) if fmt == 3 else E.encode_evt2(x, y, t, p)
    return {"cols": (x.astype(np.int16), y.astype(np.int16), t.astype(np.int64), p.astype(np.uint8)), "vectorize": vectorize, "words": words}


def raw_inputs(rng):
    G = _t("_raw_streams")
    C, S = _raw_geometry()
    fmt = int(rng.choice([3, 2]))
    nk = str(rng.choice(RAW_N_CLASSES, p=RAW_N_WEIGHTS))
    family = str(rng.choice(RAW_FAMILIES[fmt], p=RAW_FAMILY_WEIGHTS[fmt]))
    if family in ("dense_vectors", "late_time") and nk not in ("scan", "0") and rng.random() < 0.7:
        nk = "chunks" if rng.random() < 0.7 else "chunk"     # a run longer than a chunk, a first TIME_HIGH in a late chunk
    n = {"0": 0, "1-15": int(rng.integers(1, 16)), "16k": 16 * int(rng.integers(1, 9)) + int(rng.integers(-1, 2)),
         "wave": 1024 + int(rng.integers(-3, 4)), "chunk": C + int(rng.integers(-1, 2)),
         "chunks": 2 * C + int(3 * C * rng.random() ** 3), "scan": S * C + int(rng.integers(16, 2 * C))}[nk]
    c = {"fmt": fmt, "nk": nk, "n": n, "family": family, "tk": None, "lk": None, "plain": nk == "scan"}
    if nk == "scan":
        c["family"], words = "structured", _raw_plain(rng, fmt, n)
    elif family == "structured":
        words = (G.structured_evt3 if fmt == 3 else G.structured_evt2)(rng, n, start_time=bool(rng.integers(0, 4 if n >= 64 else 12)))
    elif family == "random":
        words = G.random_words(rng, n, fmt)
    elif family == "time_only":
        c["tk"] = str(rng.choice(RAW_TIME_ONLY))
        words = _raw_time_only(rng, fmt, n, c["tk"])
    elif family == "late_time":
        words, c["lk"] = _raw_late_time(rng, fmt, n, str(rng.choice(RAW_LATE, p=RAW_LATE_WEIGHTS)), G)
    elif family == "dense_vectors":
        words = _raw_dense_vectors(rng, min(n, 2 * C + C // 2))
        c["n"] = n = len(words)
    else:
        words = _raw_no_events(rng, fmt, n, G)
    assert len(words) == n and words.dtype == (np.uint16 if fmt == 3 else np.uint32)
    c["words"] = words
    c["form"] = str(rng.choice(RAW_FORMS))
    c["off"] = {"slice1": 1, "slice3": 3, "sliceC1": C + 1, "u8view": int(rng.integers(1, 4))}.get(c["form"], 0)
    ncuts = int(rng.integers(0, 2)) if c["plain"] else int(rng.choice([0, 1, 2, 3, 4, 5], p=[0.1, 0.3, 0.2, 0.15, 0.15, 0.1]))
    c["cuts"], c["cut_classes"] = _raw_draw_cuts(rng, fmt, words, ncuts)
    c["ts"] = str(rng.choice(["us", "seconds"]))
    c["sk"] = str(rng.choice(RAW_SENSORS, p=[0.25, 0.6, 0.15]))
    if c["sk"] == "drawn":
        size = RAW_SENSOR_SIZES[int(rng.integers(0, len(RAW_SENSOR_SIZES)))]
        c["sensor"] = size if rng.random() < 0.75 else (int(rng.integers(1, 2049)), int(rng.integers(1, 2049)))
    else:
        c["sensor"] = None if c["sk"] == "none" else (65535, 65535)
    c["policy"] = str(rng.choice(RAW_POLICIES))
    c["stk"] = "none" if c["plain"] else str(rng.choice(RAW_STATES, p=[0.35, 0.15, 0.5]))
    c["state"] = None
    if c["stk"] != "none":
        loops = int(rng.choice([0, 1, int(rng.integers(2, 1 << 20)), int(rng.integers(1 << 16, (1 << 20) + 1)), 1 << 20]))
        c["state"] = (int(rng.integers(0, 2048)), int(rng.integers(0, 1 << 16)), int(rng.integers(0, 2)), int(rng.integers(0, 4096)),
                      int(rng.integers(0, 1 << (12 if fmt == 3 else 28))) if rng.random() < 0.7 else (1 << (12 if fmt == 3 else 28)) - 1 - int(rng.integers(0, 8)),
                      loops, c["stk"] == "time")
    cw = int(rng.choice([int(rng.integers(1, 16)), 16, 17, 1024 + int(rng.integers(-1, 2)), C + int(rng.integers(-1, 2)), int(rng.integers(1, max(2, n + 2)))]))
    c["chunk_words"] = max(cw, -(-n // RAW_MAX_PIECES))
    c["rt"] = _raw_round_trip(rng, fmt) if rng.random() < RAW_ROUND_TRIP_SHARE else None
    c["desc"] = ("raw evt%d %s%s n=%d(%s) %s cuts=%s%s ts=%s sensor=%s %s state=%s chunk_words=%d%s"
                 % (fmt, c["family"], "".join(":" + v for v in (c["tk"], c["lk"]) if v) + (":plain" if c["plain"] else ""), n, nk, c["form"],
                    c["cuts"], c["cut_classes"], c["ts"], c["sensor"], c["policy"], c["state"], c["chunk_words"],
                    "" if c["rt"] is None else " round trip of %d events%s" % (len(c["rt"]["cols"][0]), " (vectorize)" if c["rt"]["vectorize"] else "")))
    return c


def raw_bounds(c):
    return [0] + c["cuts"] + [c["n"]]


def raw_dropped(ref, sensor):
    """the restatement's result under on_out_of_range='drop': the rows inside the sensor by the unsigned comparison; the count of
    events is theirs, the other stats stay"""
    if sensor is None or ref[4][5] == 0:
        return ref
    keep = (ref[0].view(np.uint16) < sensor[1]) & (ref[1].view(np.uint16) < sensor[0])
    return tuple(col[keep] for col in ref[:4]) + ((int(keep.sum()),) + ref[4][1:], ref[5])


def raw_reference(c):
    """The sequential restatement over the whole stream from the case's state ('whole'), over each piece from the state the piece
    before it left ('pieces'; empty without cuts), and over the whole stream from the initial state ('fresh': what a file gives)."""
    N = _t("_raw_np")
    rdec = N.decode_evt3 if c["fmt"] == 3 else N.decode_evt2
    whole = rdec(c["words"], state=c["state"], sensor_size=c["sensor"])
    pieces, st, bounds = [], c["state"], raw_bounds(c)
    if c["cuts"]:
        for a, b in zip(bounds, bounds[1:]):
            pieces.append(rdec(c["words"][a:b], state=st, sensor_size=c["sensor"]))
            st = pieces[-1][5]
    fresh = whole if c["state"] is None else rdec(c["words"], state=None, sensor_size=c["sensor"])
    return {"whole": whole, "pieces": pieces, "fresh": fresh}


def _raw_report(out, st, ref, what, seconds):
    """a device result (RawEvents, RawState or None) against a restatement result, bit for bit: columns with their types, stats,
    state; the time column of ts='seconds' against us / 1e6 in float64"""
    for k, name in enumerate(("xs", "ys", "ts", "ps")):
        want = ref[2] / 1e6 if (k == 2 and seconds) else ref[k]
        if not out[k].is_cuda:
            return "%s: %s is not on the device" % (what, name)
        err = exact(out[k], want, "%s: %s" % (what, name))
        if err is not None:
            return err
    if tuple(out.stats) != tuple(ref[4]) or not all(type(v) is int for v in out.stats):
        return "%s: stats %r vs %r" % (what, tuple(out.stats), tuple(ref[4]))
    if st is not None and tuple(st) != tuple(ref[5]):
        return "%s: state %r vs %r" % (what, tuple(st), tuple(ref[5]))
    return None


def _raw_same_bits(a, b, what):
    for k, name in enumerate(("xs", "ys", "ts", "ps")):
        if a[k].dtype != b[k].dtype or _host(a[k]).tobytes() != _host(b[k]).tobytes():
            return "%s: %s differs" % (what, name)
    return None if tuple(a.stats) == tuple(b.stats) else "%s: stats %r vs %r" % (what, tuple(a.stats), tuple(b.stats))


def _raw_parts(c):
    """part(a, b): the words [a, b) in the case's form of input"""
    words, item = c["words"], c["words"].dtype.itemsize
    signed = words.view(np.int16 if item == 2 else np.int32)
    form, off = c["form"], c["off"]
    if form in ("numpy", "signed", "bytes"):
        return {"numpy": lambda a, b: words[a:b], "signed": lambda a, b: signed[a:b], "bytes": lambda a, b: words[a:b].tobytes()}[form]
    buf = torch.zeros(off + len(words) + 5, dtype=torch.int16 if item == 2 else torch.int32, device="cuda")
    buf[off:off + len(words)] = torch.from_numpy(signed).cuda()
    if form == "u8view":
        return lambda a, b: buf.view(torch.uint8)[item * (off + a):item * (off + b)]
    return lambda a, b: buf[off + a:off + b]


def case_raw(rng):
    """decode_evt3 / decode_evt2 through both write kernels against the restatement: the whole stream, a second call, the pieces of the
    cut plan with the state carried, the out-of-range policies, iter_decode_raw / decode_raw on an in-memory RawFile, and the
    encoders' round trip (which does not involve the restatement)."""
    from event_utils_amd import _lib
    from event_utils_amd.data_formats import raw as RAW
    c = raw_inputs(rng)
    fmt, sensor, seconds = c["fmt"], c["sensor"], c["ts"] == "seconds"
    paths = (("staged", 0), ("direct", _lib.EVK_RAW_DIRECT_STORES))

    def dec(words, state, flags, policy="keep", size=sensor, ts=c["ts"]):
        return RAW._decode(words, fmt, size, ts, state, True, policy, None, flags=flags)

    def body():
        r = raw_reference(c)
        part = _raw_parts(c)
        whole = {}
        for name, flags in paths:
            out, st = dec(part(0, c["n"]), c["state"], flags)
            whole[name] = out
            err = _raw_report(out, st, r["whole"], "whole stream, %s" % name, seconds)
            if err is not None:
                return err
        err = _raw_same_bits(whole["staged"], whole["direct"], "staged against direct")
        err = err or _raw_same_bits(dec(part(0, c["n"]), c["state"], int(rng.integers(0, 2)))[0], whole["staged"], "a second call")
        if err is not None:
            return err
        # the pieces, the state carried by the device's own answers
        bounds = raw_bounds(c)
        for name, flags in paths if c["cuts"] else ():
            st, outs = c["state"], []
            for i, (a, b) in enumerate(zip(bounds, bounds[1:])):
                before = st
                out, st = dec(part(a, b), st, flags)
                outs.append(out)
                what = "piece %d [%d, %d), %s" % (i, a, b, name)
                err = _raw_report(out, st, r["pieces"][i], what, seconds)
                if err is None and a == b and (len(out.xs) or any(out.stats) or tuple(st) != tuple(RAW.RawState() if before is None else before)):
                    err = "%s: an empty piece returns %d events, stats %r, state %r behind %r" % (what, len(out.xs), tuple(out.stats), st, before)
                if err is not None:
                    return err
            for k, col in enumerate(("xs", "ys", "ts", "ps")):
                if not torch.equal(torch.cat([o[k] for o in outs]), whole[name][k]):
                    return "pieces, %s: the concatenated %s is not the whole's" % (name, col)
            total = tuple(sum(v) for v in zip(*(o.stats for o in outs)))
            if total != tuple(r["whole"][4]) or tuple(st) != tuple(r["whole"][5]):
                return "pieces, %s: stats add up to %r, last state %r; the whole: %r, %r" % (name, total, tuple(st), r["whole"][4], r["whole"][5])
        # the policies
        bad, count = r["whole"][4][5], r["whole"][4][0]
        for name, flags in paths:
            what = "on_out_of_range=%r, %s" % (c["policy"], name)
            try:
                out, st = dec(part(0, c["n"]), c["state"], flags, c["policy"])
            except ValueError as e:
                if c["policy"] != "raise" or bad == 0:
                    return "%s: ValueError (%s) where the restatement counts %d out of range" % (what, e, bad)
                if "%d of %d decoded" % (bad, count) not in str(e):
                    return "%s: the message %r does not carry %d of %d" % (what, str(e), bad, count)
                continue
            if c["policy"] == "raise" and bad:
                return "%s: no ValueError, the restatement counts %d of %d out of range" % (what, bad, count)
            err = _raw_report(out, st, raw_dropped(r["whole"], sensor) if c["policy"] == "drop" else r["whole"], what, seconds)
            if err is not None:
                return err
        # a file of the words, piece by piece
        policy = "keep" if c["policy"] == "raise" else c["policy"]
        rf = RAW.RawFile("evt%d" % fmt, sensor, {}, c["words"], 0)
        kw = dict(chunk_words=c["chunk_words"], ts=c["ts"], on_out_of_range=policy)
        pieces = list(E.iter_decode_raw(rf, **kw))
        want = raw_dropped(r["fresh"], sensor) if policy == "drop" else r["fresh"]
        if len(pieces) != -(-c["n"] // c["chunk_words"]):
            return "iter_decode_raw: %d pieces of %d words for %d words" % (len(pieces), c["chunk_words"], c["n"])
        if pieces:
            joined = RAW.RawEvents(*(torch.cat([p[k] for p in pieces]) for k in range(4)), RAW.RawStats(*(sum(v) for v in zip(*(p.stats for p in pieces)))))
            err = _raw_report(joined, None, want, "iter_decode_raw with chunk_words=%d" % c["chunk_words"], seconds)
        err = err or _raw_report(E.decode_raw(rf, **kw), None, want, "decode_raw with chunk_words=%d" % c["chunk_words"], seconds)
        if err is not None:
            return err
        # the encoders: the events come back, without the restatement
        if c["rt"] is not None:
            x, y, t, p = c["rt"]["cols"]
            stats = (len(x), 0, 0, 0, 0, 0, (int(t[-1]) >> 24) if (fmt == 3 and len(t)) else 0)
            for name, flags in paths:
                out, st = dec(c["rt"]["words"], None, flags, "raise", (2048, 2048))
                err = _raw_report(out, None, (x, y, t, p, stats), "round trip through encode_evt%d, %s" % (fmt, name), seconds)
                if err is not None:
                    return err
        return None
    return _run_case(c["desc"], body)


if __name__ == "__main__":
    budget = float(arg("--seconds", "240"))
    seed = int(arg("--seed0", "0"))
    kinds = arg("--kinds", "voxel,image,native,iwe,objective,windows,misc,errors,prims,search,filters,augment,datasets,motion,motion8,zhu,denoise,tsurf,corners,planeflow,reconstruct,emvs,simulate,flowts,flowcm,segment,raw").split(",")
    fns = {"voxel": case_voxel, "image": case_image, "native": case_native, "iwe": case_iwe, "objective": case_objective,
           "windows": case_windows, "misc": case_misc, "errors": case_errors, "prims": case_prims, "search": case_search,
           "filters": case_filters, "augment": case_augment, "datasets": case_datasets, "motion": case_motion, "motion8": case_motion8, "zhu": case_zhu,
           "denoise": case_denoise, "tsurf": case_tsurf, "corners": case_corners, "planeflow": case_planeflow, "reconstruct": case_reconstruct,
           "emvs": case_emvs, "simulate": case_simulate, "flowts": case_flowts, "flowcm": case_flowcm, "segment": case_segment,
           "raw": case_raw}
    t0, done, failed = time.time(), {k: 0 for k in kinds}, []
    while time.time() - t0 < budget:
        kind = kinds[seed % len(kinds)]
        rng = np.random.default_rng(900_000 + seed)
        desc, err = fns[kind](rng)
        done[kind] += 1
        if err is not None:
            failed.append((seed, desc, err))
            print("FAIL seed %d: %s -> %s" % (seed, desc, err), flush=True)
        seed += 1
    print("cases", done, "failures", len(failed), "next seed", seed)
    sys.exit(1 if failed else 0)
