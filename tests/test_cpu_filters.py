"""CPU: the event filters of lib/util/event_util.py (clip_events_to_bounds, get_events_from_mask, remove_hot_pixels).  A numpy
restatement of the three -- the hot-pixel rule in closed form -- checked against the real reference (loaded through
oracle.ref_loader, its remove_hot_pixels' np.delete given integer indices in memory), the C argument checks of the new entry
points, and the public signatures.  tests/test_gpu_filters.py checks the device implementation against the restatement."""
import ctypes
import inspect
import types

import numpy as np
import pytest

from oracle import ref_loader


# ---- the restatement ----------------------------------------------------------------------------------------------------

def np_hot_pixels(img, num_hot):
    """Flat indices (of the (H, W) image) the reference's loop "argmax, set to 0" picks in num_hot rounds, in closed form:
    value descending with NaN above +inf and ties to the lower index; the first min(num_hot, P) of the P pixels > 0 or NaN;
    when num_hot > P one more, the lowest pixel that is 0 after those picks, else (none) the argmax of the image."""
    flat = np.asarray(img).ravel()
    if num_hot <= 0:
        return []
    nan = np.isnan(flat) if flat.dtype.kind == "f" else np.zeros(flat.shape, bool)
    P = int(np.count_nonzero((flat > 0) | nan))
    order = np.lexsort((np.arange(flat.size), -np.where(nan, 0, flat), ~nan))
    hot = [int(i) for i in order[:min(num_hot, P)]]
    if num_hot > P:
        zero_after = np.flatnonzero(~(flat < 0))
        hot.append(int(zero_after[0]) if zero_after.size else int(np.argmax(flat)))
    return hot


def np_remove_hot_pixels(xs, ys, ts, ps, sensor_size=(180, 240), num_hot=50):
    H, W = sensor_size
    abs_coords = np.ravel_multi_index(np.stack((ys, xs)), (H + 1, W + 1))    # ValueError / TypeError as image.py:30-36
    img = np.bincount(abs_coords, weights=ps, minlength=(H + 1) * (W + 1)).reshape(H + 1, W + 1)[:H, :W]
    drop = np.zeros(len(xs), bool)
    for h in np_hot_pixels(img, num_hot):
        drop |= (xs == h % W) & (ys == h // W)
    keep = ~drop
    return xs[keep], ys[keep], ts[keep], ps[keep]


def np_clip_events_to_bounds(xs, ys, ts, ps, bounds, set_zero=False):
    if len(bounds) == 2:
        bounds = [0, bounds[0], 0, bounds[1]]
    elif len(bounds) != 4:
        raise Exception("Bounds must be of length 2 or 4")
    miny, maxy, minx, maxx = bounds
    if set_zero:
        mask = np.where((xs <= minx) | (xs > maxx), 0.0, 1.0) * np.where((ys <= miny) | (ys > maxy), 0.0, 1.0)
        return xs * mask, ys * mask, None if ts is None else ts * mask, None if ps is None else ps * mask
    keep = (xs >= minx) & (xs < maxx) & (ys >= miny) & (ys < maxy)
    return xs[keep], ys[keep], None if ts is None else ts[keep], None if ps is None else ps[keep]


def np_get_events_from_mask(mask, xs, ys):
    vals = mask[ys.astype(int), xs.astype(int)]
    return np.flatnonzero(vals >= 0.01).squeeze()


# ---- against the real reference -----------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ref():
    if not ref_loader.available():
        pytest.skip("reference checkout not present")
    ev = ref_loader.load().event_util
    f = ev.remove_hot_pixels
    shim = types.ModuleType("numpy_int_delete")
    shim.__dict__.update({k: getattr(np, k) for k in dir(np) if not k.startswith("__")})
    shim.delete = lambda a, idx, *r, **k: np.delete(a, np.asarray(idx).astype(np.int64), *r, **k)
    hot = types.FunctionType(f.__code__, dict(f.__globals__, np=shim), f.__name__, f.__defaults__)
    return types.SimpleNamespace(remove_hot_pixels=hot, clip=ev.clip_events_to_bounds, mask=ev.get_events_from_mask, mod=ev)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


def events(rng, n, H, W, pdtype=np.int64):
    x = rng.integers(0, W, n)
    y = rng.integers(0, H, n)
    t = np.sort(rng.uniform(0, 1, n))
    p = (rng.integers(0, 2, n) * 2 - 1).astype(pdtype)
    return x, y, t, p


HOT_CASES = {
    "ties": lambda rng: (np.repeat([3, 5, 7, 1], 4), np.repeat([2, 2, 4, 0], 4), np.arange(16.), np.ones(16, np.int64), 3),
    "num_hot_above_P": lambda rng: (np.array([1, 1, 2, 3]), np.array([0, 0, 1, 2]), np.arange(4.), np.array([1, 1, -1, 1]), 9),
    "num_hot_0": lambda rng: (*events(rng, 300, 6, 8), 0),
    "zero_sum_pixel_is_the_extra": lambda rng: (np.array([0, 0, 2, 5, 5]), np.array([0, 0, 1, 3, 3]), np.arange(5.),
                                                np.array([-1, -1, 1, 1, -1]), 3),
    "all_negative": lambda rng: (np.tile(np.arange(8), 6), np.repeat(np.arange(6), 8), np.arange(48.), -np.ones(48, np.int64), 4),
    "nan_weight": lambda rng: (np.array([1, 2, 3, 4]), np.array([1, 1, 1, 1]), np.arange(4.), np.array([1.0, np.nan, 5.0, 2.0]), 2),
    "x_equals_W": lambda rng: (np.array([8, 8, 8, 1]), np.array([0, 0, 0, 6]), np.arange(4.), np.ones(4, np.int64), 2),
    "random": lambda rng: (*events(rng, 2000, 6, 8), 5),
}


@pytest.mark.parametrize("case", sorted(HOT_CASES))
def test_hot_pixel_restatement_equals_the_reference(ref, case):
    rng = np.random.default_rng(7)
    x, y, t, p, k = HOT_CASES[case](rng)
    got = np_remove_hot_pixels(x, y, t, p, sensor_size=(6, 8), num_hot=k)
    want = ref.remove_hot_pixels(x, y, t, p, sensor_size=(6, 8), num_hot=k)
    for g, w in zip(got, want):
        same(g, w)


def test_hot_pixel_restatement_random_num_hot(ref):
    rng = np.random.default_rng(11)
    for trial in range(25):
        H, W = rng.integers(1, 7, 2)
        x, y, t, p = events(rng, int(rng.integers(1, 200)), H, W)
        p = p * rng.integers(0, 3, p.shape[0])                     # zeros and cancellations
        k = int(rng.integers(0, H * W + 3))
        for g, w in zip(np_remove_hot_pixels(x, y, t, p, (int(H), int(W)), k), ref.remove_hot_pixels(x, y, t, p, (int(H), int(W)), k)):
            same(g, w)


def test_hot_pixel_errors_equal_the_reference(ref):
    x, y, t, p = np.array([1, 9]), np.array([0, 0]), np.arange(2.), np.ones(2)
    for f in (np_remove_hot_pixels, ref.remove_hot_pixels):
        with pytest.raises(ValueError):
            f(x, y, t, p, sensor_size=(4, 4), num_hot=1)
        with pytest.raises(TypeError):
            f(x * 1.0, y * 1.0, t, p, sensor_size=(12, 12), num_hot=1)


@pytest.mark.parametrize("bounds", [(5, 7), (1, 5, 2, 7), (1.5, 4.25, 0.5, 6.75)])
@pytest.mark.parametrize("set_zero", [False, True])
def test_clip_restatement_equals_the_reference(ref, bounds, set_zero):
    rng = np.random.default_rng(3)
    x, y, t, p = events(rng, 500, 8, 10)
    for cols in ((x, y, t, p), (x.astype(np.float32), y.astype(np.float32), t.astype(np.float32), p.astype(np.float32)),
                 (x, y, None, None)):
        got = np_clip_events_to_bounds(*cols, bounds, set_zero)
        want = ref.clip(*cols, bounds, set_zero)
        for g, w in zip(got, want):
            assert (g is None) == (w is None)
            if g is not None:
                same(g, w)


def test_clip_bounds_of_length_3_raise(ref):
    x = np.arange(4)
    for f in (np_clip_events_to_bounds, ref.clip):
        with pytest.raises(Exception):
            f(x, x, x, x, [1, 2, 3])


def test_clip_float32_columns_against_a_bound_that_is_no_float32():
    """NEP 50: a float32 column against a python float compares in float32; the library rounds the bound so."""
    from event_utils_amd.util.event_util import _round_bound
    b = 0.7
    assert float(np.float32(b)) < b
    xs = np.array([np.float32(b), 0.8], np.float32)
    assert (xs >= b).tolist() == [True, True]                      # compared in float32: float32(0.1) >= float32(0.1)
    assert (xs.astype(np.float64) >= b).tolist() == [False, True]
    assert _round_bound(xs.dtype, b) == float(np.float32(b))
    assert _round_bound(np.dtype(np.float32), np.float64(b)) == b   # a float64 scalar is not weak: compared in float64
    assert _round_bound(np.dtype(np.int64), b) == b and _round_bound(np.dtype(np.int16), 3) == 3.0


def test_mask_restatement_equals_the_reference(ref):
    rng = np.random.default_rng(5)
    H, W = 6, 9
    x = rng.uniform(-W, W - 0.01, 300)
    y = rng.uniform(-H, H - 0.01, 300)
    for mask in (rng.uniform(0, 0.02, (H, W)), rng.uniform(0, 0.02, (H, W)).astype(np.float32), rng.integers(0, 2, (H, W)),
                 np.full((H, W), np.float32(0.01), np.float32), rng.uniform(0, 1, (H, W)) > 0.5):
        same(np_get_events_from_mask(mask, x, y), ref.mask(mask, x, y))
        same(np_get_events_from_mask(mask, x.astype(np.int64), y.astype(np.int16)), ref.mask(mask, x.astype(np.int64), y.astype(np.int16)))


def test_mask_float32_threshold_and_single_hit(ref):
    m = np.zeros((3, 4), np.float32)
    m[1, 2] = np.float32(0.01)                                     # float32(0.01) >= 0.01 holds in numpy 2 (compared in float32)
    x, y = np.array([2.7, 0.0, 3.0]), np.array([1.2, 0.0, 2.0])
    r = ref.mask(m, x, y)
    assert r.shape == () and int(r) == 0
    same(np_get_events_from_mask(m, x, y), r)
    assert not np.float64(np.float32(0.01)) >= 0.01              # ... but not in float64: the threshold is rounded first


def test_mask_wrap_and_out_of_range_equal_the_reference(ref):
    m = np.ones((3, 4))
    x, y = np.array([-4.5, -1.0, 3.9]), np.array([-3.0, -0.5, 2.0])    # -4.5 -> -4 wraps to 0; -0.5 -> 0
    same(np_get_events_from_mask(m, x, y), ref.mask(m, x, y))
    for xb, yb in ((np.array([-5.0]), np.array([0.0])), (np.array([4.0]), np.array([0.0])), (np.array([0.0]), np.array([3.0])),
                   (np.array([np.nan]), np.array([0.0]))):
        for f in (np_get_events_from_mask, ref.mask):
            with pytest.raises(IndexError):
                f(m, xb, yb)


# ---- the library without a GPU ------------------------------------------------------------------------------------------

def test_select_entry_points_reject_bad_arguments_without_a_gpu():
    from event_utils_amd import _lib
    L = _lib.lib()
    res = ctypes.c_void_p(16)                       # (never dereferenced: the checks come first)
    params = (ctypes.c_double * 4)(0, 1, 0, 1)
    src = (ctypes.c_void_p * 1)(16)
    eb = (ctypes.c_int * 1)(4)
    scratch = ctypes.c_void_p(16)
    args = lambda n, kind, pred, result: (pred, kind, scratch, scratch, n, params, None, 0, 0, 1, src, src, eb, -1, None, result,
                                         scratch, 1 << 20, None, None)
    assert L.evk_select_compact(*args(-1, _lib.EVK_SELECT_F32, _lib.EVK_SELECT_BOX, res)) == -1
    assert L.evk_select_compact(*args(10, _lib.EVK_SELECT_F32, _lib.EVK_SELECT_BOX, None)) == -1      # NULL result
    assert L.evk_select_compact(*args(10, 7, _lib.EVK_SELECT_BOX, res)) == -1                         # bad coordinate kind
    assert L.evk_select_compact(*args(10, _lib.EVK_SELECT_F32, 9, res)) == -1                         # bad predicate
    assert L.evk_select_compact(*args(10, _lib.EVK_SELECT_F32, _lib.EVK_SELECT_MASK, res)) == -1      # mask without image
    eb[0] = 3
    assert L.evk_select_compact(*args(10, _lib.EVK_SELECT_F32, _lib.EVK_SELECT_BOX, res)) == -1       # element size 3
    eb[0] = 4
    small = list(args(10_000_000, _lib.EVK_SELECT_F32, _lib.EVK_SELECT_BOX, res))
    small[17] = 64
    assert L.evk_select_compact(*small) == -2                                                          # scratch too small
    assert L.evk_select_scratch_bytes(-1) == -1
    assert L.evk_select_to_i32(_lib.EVK_SELECT_F32, None, -1, None, None, None) == -1
    assert L.evk_select_to_i32(9, scratch, 4, scratch, None, None) == -1
    assert L.evk_select_to_i32(_lib.EVK_SELECT_F32, scratch, 4, None, None, None) == -1
    hs = int(L.evk_hot_pixels_scratch_bytes())
    assert hs > 0
    assert L.evk_hot_pixels(scratch, _lib.EVK_SELECT_I32, 4, 4, 5, 1, None, scratch, hs, None) == -1   # NULL output
    assert L.evk_hot_pixels(scratch, _lib.EVK_SELECT_F32, 4, 4, 5, 1, scratch, scratch, hs, None) == -1
    assert L.evk_hot_pixels(scratch, _lib.EVK_SELECT_I32, 4, 4, 3, 1, scratch, scratch, hs, None) == -1   # pitch < w
    assert L.evk_hot_pixels(scratch, _lib.EVK_SELECT_I32, 4, 4, 5, 1, scratch, scratch, hs - 1, None) == -2
    assert L.evk_mask_multiply_f64(_lib.EVK_SELECT_F32, None, -1, 0.0, None, None, None) == -1
    assert L.evk_mask_multiply_f64(9, scratch, 4, 0.0, scratch, scratch, None) == -1
    assert L.evk_mask_multiply_f64(_lib.EVK_SELECT_F32, scratch, 4, 0.0, scratch, None, None) == -1


def test_filter_signatures_equal_the_reference():
    import event_utils_amd as E
    from event_utils_amd.lib.util import event_util as aliased

    def sig(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    E_ = inspect.Parameter.empty
    assert sig(E.remove_hot_pixels) == [("xs", E_), ("ys", E_), ("ts", E_), ("ps", E_), ("sensor_size", (180, 240)), ("num_hot", 50)]
    assert sig(E.clip_events_to_bounds) == [("xs", E_), ("ys", E_), ("ts", E_), ("ps", E_), ("bounds", E_), ("set_zero", False)]
    assert sig(E.get_events_from_mask) == [("mask", E_), ("xs", E_), ("ys", E_)]
    assert aliased.remove_hot_pixels is E.remove_hot_pixels
    if ref_loader.available():
        ev = ref_loader.load().event_util
        for name in ("remove_hot_pixels", "clip_events_to_bounds", "get_events_from_mask"):
            assert sig(getattr(E, name)) == sig(getattr(ev, name)), name


def test_select_kernels_compile_without_register_spills(tmp_path):
    """Every kernel of evk_select.hip (the compaction for five coordinate kinds x three predicates, the hot-pixel select) compiles
    for gfx950 without spilling registers."""
    import os
    import re
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    from event_utils_amd.csrc import build as B
    src = os.path.join(B.HERE, "evk_select.hip")
    subprocess.run([hipcc] + list(B.CFLAGS) + ["-c", src, "-o", str(tmp_path / "sel.o"), "-save-temps=obj"], check=True, cwd=B.HERE,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert asm, os.listdir(tmp_path)
    text = open(tmp_path / asm[0]).read()
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    seen = {n: (int(v), int(sp)) for n, v, sp in kernels}
    assert sum("k_sel_write" in n for n in seen) == 15 and sum("k_sel_count" in n for n in seen) == 15
    assert any("k_hot_hist" in n for n in seen)
    assert not {n: vs for n, vs in seen.items() if vs[1]}
