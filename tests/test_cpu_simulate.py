"""CPU (no GPU): the host restatement of the event simulator (tests/_simulate_np.py, the literal float64 walk) on hand-worked cases;
the evk_simulate_* entry points are declared, bound and exported and refuse bad arguments before they touch the device; the kernels
of evk_simulate.hip compile for gfx950 without register spills; the Python argument errors; the public surface."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _header
import _simulate_np as N

ENTRIES = {"evk_simulate_count", "evk_simulate_emit", "evk_simulate_sort", "evk_simulate_sort_scratch_bytes"}


def one(levels, ts=None, **kw):
    """seq_simulate of a 1 x 1 sensor whose frames are `levels` -> (ts list, ps list, R, tl, overflow)"""
    frames = np.asarray(levels, dtype=np.float64).reshape(-1, 1, 1)
    ts = np.arange(len(frames), dtype=np.float64) * 10.0 + 100.0 if ts is None else ts
    x, y, t, p, R, tl, over = N.seq_simulate(frames, ts, **kw)
    assert x.dtype == y.dtype == p.dtype == np.int64 and t.dtype == np.float64 and not x.any() and not y.any()
    return [float(v) for v in t], [int(v) for v in p], float(R[0, 0]), float(tl[0, 0]), over


# ---- hand-worked cases ----------------------------------------------------------------------------------------------------------

def test_a_rise_of_three_and_a_half_contrasts_gives_three_on_events():
    c = 0.25                                               # dyadic: every value below is exact
    t, p, R, tl, over = one([1.0, 1.0 + 3.5 * c], c_on=c, c_off=c)
    assert p == [1, 1, 1] and over == 0
    assert t == [100.0 + 10.0 * (k * c / (3.5 * c)) for k in (1, 2, 3)]
    assert R == 1.0 + 3 * c and tl == t[-1]
    # the level carries the half contrast over: the next interval fires after half a contrast more
    t, p, R, _, _ = one([1.0, 1.0 + 3.5 * c, 1.0 + 4.5 * c], c_on=c, c_off=c)
    assert p == [1] * 4 and t[3] == 110.0 + 10.0 * ((1.0 + 4 * c - (1.0 + 3.5 * c)) / c) and R == 1.0 + 4 * c


def test_a_fall_gives_off_events_with_the_off_contrast():
    t, p, R, tl, over = one([2.0, 0.75], c_on=0.25, c_off=0.5)
    assert p == [-1, -1] and t == [100.0 + 10.0 * (0.5 / 1.25), 100.0 + 10.0 * (1.0 / 1.25)] and R == 1.0 and over == 0
    # a change smaller than the contrast: nothing, and the level stays
    assert one([2.0, 1.75, 2.2], c_on=0.25, c_off=0.5)[:3] == ([], [], 2.0)


def test_a_crossing_inside_the_refractory_period_moves_the_level_but_emits_nothing():
    # crossings at 102.5, 105, 107.5, 110: with refractory 4 each is 2.5 after the previous CROSSING, emitted or not
    t, p, R, tl, _ = one([0.0, 1.0], c_on=0.25, c_off=0.25, refractory=4.0)
    assert t == [102.5] and p == [1] and R == 1.0 and tl == 110.0
    assert one([0.0, 1.0], c_on=0.25, c_off=0.25, refractory=2.5)[0] == [102.5, 105.0, 107.5, 110.0]
    # the state handed in counts: a last crossing at 99 silences the first one
    assert one([0.0, 1.0], c_on=0.25, c_off=0.25, refractory=4.0, last_event_ts=np.full((1, 1), 99.0))[0] == []
    assert one([0.0, 1.0], c_on=0.25, c_off=0.25, refractory=4.0, last_event_ts=np.full((1, 1), 98.5))[0] == [102.5]


def test_a_reference_far_from_the_first_frame_gives_a_burst_at_the_first_frame_time():
    t, p, R, _, _ = one([1.0, 1.5], c_on=0.25, c_off=0.25, reference=np.full((1, 1), 0.0))
    # R = 0.25 .. 1.0 lie at or below L0 = 1: frac <= 0 clamps to 0; then 1.25 and 1.5 interpolate
    assert t == [100.0] * 4 + [105.0, 110.0] and p == [1] * 6 and R == 1.5
    t, p, R, _, _ = one([1.0, 0.5], c_on=0.25, c_off=0.25, reference=np.full((1, 1), 2.0))
    assert t == [100.0] * 4 + [105.0, 110.0] and p == [-1] * 6 and R == 0.5
    # a reference on the far side of a rise: nothing is due
    assert one([1.0, 1.5], c_on=0.25, c_off=0.25, reference=np.full((1, 1), 5.0))[:3] == ([], [], 5.0)


def test_non_finite_and_constant_intervals_emit_nothing():
    inf, nan = float("inf"), float("nan")
    for levels in ([1.0, 1.0, 1.0], [1.0, nan, 1.0], [1.0, inf, 1.0], [1.0, -inf, nan], [inf, inf]):
        t, p, R, tl, over = one(levels, c_on=0.25, c_off=0.25, reference=np.full((1, 1), 0.5))
        assert (t, p, R, tl, over) == ([], [], 0.5, -inf, 0)
    # a finite interval after a broken one works from the level that was left
    t, p, R, _, _ = one([1.0, nan, 1.0, 1.5], c_on=0.25, c_off=0.25)
    assert t == [125.0, 130.0] and p == [1, 1] and R == 1.5


def test_the_step_limit_is_reported_as_overflow():
    assert N.MAX_STEPS == 65536
    c = 2.0 ** -10
    t, p, R, _, over = one([0.0, 64.0], c_on=c, c_off=c)          # exactly 65 536 crossings: the limit is reached, nothing is left
    assert len(t) == 65536 and over == 0 and R == 64.0 and t[-1] == 110.0
    t, p, R, _, over = one([0.0, 64.0 + c], c_on=c, c_off=c)      # one more is due
    assert len(t) == 65536 and over == 1 and R == 64.0
    t, p, R, _, over = one([2.0 ** 60, 2.0 ** 61], c_on=1.0, c_off=1.0)      # a contrast below the ulp of R: R never moves
    assert over == 1 and R == 2.0 ** 60 and len(t) == 65536 and set(t) == {100.0}
    # per pixel-interval: two overflowing intervals of one pixel count twice
    assert one([0.0, 100.0, -100.0], c_on=c, c_off=c)[4] == 2


def test_the_order_is_time_then_pixel_then_emission():
    frames = np.zeros((2, 1, 3))
    frames[1, 0] = [1.0, 0.5, -1.0]
    frames[0, 0, 0] = 0.0
    ref = np.array([[-0.5, 0.0, 0.0]])                     # pixel 0: two clamped crossings at t = 0, then 0.25, 0.5, ...
    x, y, t, p, R, tl, _ = N.seq_simulate(frames, [0.0, 8.0], 0.25, 0.5, reference=ref)
    got = list(zip(t.tolist(), x.tolist(), p.tolist()))
    assert got == [(0.0, 0, 1), (0.0, 0, 1), (2.0, 0, 1), (4.0, 0, 1), (4.0, 1, 1), (4.0, 2, -1), (6.0, 0, 1), (8.0, 0, 1), (8.0, 1, 1),
                   (8.0, 2, -1)]
    assert R.tolist() == [[1.0, 0.5, -1.0]] and tl.tolist() == [[8.0, 8.0, 8.0]]


@pytest.mark.parametrize("name", ["scene_a", "scene_b", "tie_scene"])
def test_the_level_ends_within_one_contrast_of_the_last_frame(name):
    frames, fts = getattr(N, name)()
    c_on, c_off = (0.5, 0.25) if name == "tie_scene" else (0.11, 0.13)
    x, y, t, p, R, tl, over = N.seq_simulate(frames, fts, c_on, c_off)
    assert over == 0 and len(t) > 5_000
    assert (np.abs(R - frames[-1]) < max(c_on, c_off)).all()
    assert (np.diff(t) >= 0).all() and t[0] >= fts[0] and t[-1] <= fts[-1]
    H, W = frames.shape[1:]
    assert (0 <= x).all() and (x < W).all() and (0 <= y).all() and (y < H).all() and set(p.tolist()) == {-1, 1}
    # the events integrate back to the level: R = frames[0] + c_on * (ON events) - c_off * (OFF events), up to summation rounding
    img = np.zeros((H, W))
    np.add.at(img, (y, x), np.where(p > 0, c_on, -c_off))
    assert np.abs(frames[0] + img - R).max() < 1e-12


def test_per_pixel_contrast_maps():
    frames = np.zeros((2, 1, 2))
    frames[1] = 1.0
    x, y, t, p, R, _, _ = N.seq_simulate(frames, [0.0, 1.0], np.array([[0.5, 0.25]]), 0.1)
    assert x.tolist() == [1, 0, 1, 1, 0, 1] and t.tolist() == [0.25, 0.5, 0.5, 0.75, 1.0, 1.0] and R.tolist() == [[1.0, 1.0]]


# ---- the public surface and the C ABI -----------------------------------------------------------------------------------------

def test_the_prototypes_are_bound_with_their_arguments():
    from event_utils_amd import _lib
    text = _header.TEXT
    protos = _header.prototypes("evk_simulate_")
    assert set(protos) == ENTRIES
    for name, (want, ret) in protos.items():
        assert ret in (ctypes.c_int, ctypes.c_int64) and _lib.PROTOTYPES[name] == (want, ret), name
        assert hasattr(_lib.lib(), name)
    assert _lib.EVK_SIMULATE_MAX_STEPS == N.MAX_STEPS == 65536
    assert re.search(r"^#define\s+EVK_SIMULATE_MAX_STEPS\s+65536\s*$", text, re.M)
    assert "Event simulation" in text


def test_public_surface():
    import event_utils_amd as E
    import event_utils_amd.lib.simulation as alias_pkg
    import event_utils_amd.lib.simulation.event_simulator as alias
    from event_utils_amd import simulation
    from event_utils_amd.simulation import event_simulator
    assert alias is event_simulator and alias_pkg is simulation
    for name in ("simulate_events", "SimulatorState"):
        assert getattr(E, name) is getattr(event_simulator, name) is getattr(simulation, name)
    assert "(no reference module)           -> event_utils_amd.simulation.event_simulator" in E.__doc__
    doc = E.simulate_events.__doc__
    assert "frames[F - 1:]" in doc and "reference=state.reference" in doc and "last_event_ts=state.last_event_ts" in doc
    assert E.SimulatorState._fields == ("reference", "last_event_ts")
    import inspect
    assert [(p.name, p.default) for p in inspect.signature(E.simulate_events).parameters.values()] == [
        ("frames", inspect.Parameter.empty), ("frame_ts", inspect.Parameter.empty), ("c_on", 0.2), ("c_off", 0.2), ("refractory", 0.0),
        ("reference", None), ("last_event_ts", None), ("return_state", False)]


def test_arguments_are_refused_before_the_device_is_touched():
    from event_utils_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every call below is refused first
    einval, nan, inf = -1, float("nan"), float("inf")

    def head(frames=fake, frame_ts=fake, nf=3, h=16, w=16, c_on=0.1, c_off=0.1, on_map=None, off_map=None, refractory=0.0,
             reference=None, last=None):
        return (frames, frame_ts, nf, h, w, c_on, c_off, on_map, off_map, refractory, reference, last)

    def count(counts=fake, report=fake, **kw):
        return L.evk_simulate_count(*head(**kw), counts, report, None)

    def emit(offsets=fake, total=8, t_first=0.0, wide=0, keys=fake, vals=fake, ref_out=fake, tl_out=fake, **kw):
        return L.evk_simulate_emit(*head(**kw), offsets, total, t_first, wide, keys, vals, ref_out, tl_out, None)

    def sort(keys=fake, vals=fake, total=8, h=16, w=16, wide=0, t_first=0.0, t_max=1.0, scratch=fake, nbytes=1 << 20, xs=fake, ys=fake,
             ts=fake, ps=fake):
        return L.evk_simulate_sort(keys, vals, total, h, w, wide, t_first, t_max, scratch, nbytes, xs, ys, ts, ps, None)
    for call in (count, emit):
        assert call(frames=None) == einval and call(frame_ts=None) == einval
        assert call(nf=1) == einval and call(nf=0) == einval and call(nf=-2) == einval
        assert call(h=0) == einval and call(w=0) == einval and call(h=-1) == einval and call(w=-3) == einval
        assert call(h=1 << 16, w=1 << 16) == einval          # more pixels than a uint32 index holds
        for bad in (0.0, -0.1, nan, inf, -inf):
            assert call(c_on=bad) == einval and call(c_off=bad) == einval
            assert call(c_on=bad, off_map=fake) == einval and call(c_off=bad, on_map=fake) == einval
        for bad in (-1e-300, nan, -inf):
            assert call(refractory=bad) == einval
    assert count(counts=None) == einval and count(report=None) == einval
    assert emit(offsets=None) == einval and emit(keys=None) == einval and emit(vals=None) == einval
    assert emit(ref_out=None) == einval and emit(tl_out=None) == einval
    assert emit(total=-1) == einval and emit(total=1 << 31) == einval and emit(t_first=nan) == einval
    assert sort(total=-1) == einval and sort(total=1 << 31) == einval
    assert sort(h=0) == einval and sort(w=0) == einval and sort(h=1 << 16, w=1 << 16) == einval
    assert sort(t_max=-1.0) == einval and sort(t_max=nan) == einval and sort(t_first=nan) == einval
    for missing in ("keys", "vals", "scratch", "xs", "ys", "ts", "ps"):
        assert sort(**{missing: None}) == einval
    assert sort(scratch=ctypes.c_void_p(4100)) == einval         # not 256-byte aligned
    assert sort(total=0, keys=None, vals=None, scratch=None, xs=None, ys=None, ts=None, ps=None) == 0      # nothing to do
    size = L.evk_simulate_sort_scratch_bytes
    assert size(-1, 16, 16, 0, 0.0, 1.0) == einval and size(1 << 31, 16, 16, 0, 0.0, 1.0) == einval
    assert size(8, 0, 16, 0, 0.0, 1.0) == einval and size(8, 16, 16, 0, 1.0, 0.0) == einval and size(8, 16, 16, 0, nan, 1.0) == einval
    assert 0 < size(1000, 16, 16, 0, 0.0, 1.0) < size(1000, 16, 16, 1, 0.0, 1.0)
    assert sort(nbytes=16) == -2                                  # EVK_ESCRATCH: also before any device work


def test_python_argument_errors_come_before_any_device_work():
    """every call below is refused on its arguments alone: none of them reaches the point where a missing GPU would matter"""
    import torch
    import event_utils_amd as E
    frames, fts = np.zeros((3, 8, 9)), [0.0, 1.5, 2.0]

    def bad(match, frames=frames, frame_ts=fts, **kw):
        with pytest.raises(ValueError, match=match):
            E.simulate_events(frames, frame_ts, **kw)
        with pytest.raises(ValueError, match=match):
            E.simulate_events(torch.from_numpy(np.asarray(frames)), frame_ts, **kw)
    bad("F >= 2", frames=np.zeros((1, 8, 9)), frame_ts=[0.0])
    bad("F >= 2", frames=np.zeros((8, 9)), frame_ts=[0.0, 1.0])
    bad("F >= 2", frames=np.zeros((3, 0, 9)))
    bad("one time per frame", frame_ts=[0.0, 1.0])
    bad("one time per frame", frame_ts=[0.0, 1.0, 2.0, 3.0])
    bad("increasing", frame_ts=[0.0, 2.0, 1.0])
    bad("increasing", frame_ts=[0.0, 1.0, 1.0])
    bad("finite", frame_ts=[0.0, 1.0, float("inf")])
    bad("finite", frame_ts=[0.0, float("nan"), 2.0])
    for value in (0.0, -0.2, float("nan"), float("inf")):
        bad("c_on", c_on=value)
        bad("c_off", c_off=value)
    bad("c_on", c_on=np.full((9, 8), 0.2))
    bad("c_off", c_off=np.full((1, 8, 9), 0.2))
    bad("refractory", refractory=-1.0)
    bad("refractory", refractory=float("nan"))
    bad("reference", reference=np.zeros((9, 8)))
    bad("last_event_ts", last_event_ts=np.zeros((8,)))


def test_the_kernels_compile_without_register_spills(tmp_path):
    """k_sim_count, both k_sim_emit and both k_sim_gather compile for gfx950 without spilling registers."""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    from event_utils_amd.csrc import build as B
    assert "-ffp-contract=off" in B.CFLAGS and not any("fast-math" in f for f in B.CFLAGS)      # one rounding per operation
    src = os.path.join(B.HERE, "evk_simulate.hip")
    subprocess.run([hipcc] + list(B.CFLAGS) + ["-c", src, "-o", str(tmp_path / "sim.o"), "-save-temps=obj"], check=True, cwd=B.HERE,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert asm, os.listdir(tmp_path)
    text = open(tmp_path / asm[0]).read()
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    seen = {n: (int(v), int(sp)) for n, v, sp in kernels}
    assert sum("k_sim_count" in n for n in seen) == 1
    assert sum("k_sim_emit" in n for n in seen) == 2 and sum("k_sim_gather" in n for n in seen) == 2
    assert not {n: vs for n, vs in seen.items() if vs[1]}
