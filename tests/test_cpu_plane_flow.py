"""CPU (no GPU): the host restatements of the plane-fit flow definitions (tests/_plane_flow_np.py) against hand-worked cases and
against each other; the evk_planeflow_* entries are declared, bound and exported and refuse bad arguments before they touch the
device; every kernel of evk_planeflow.hip compiles for gfx950 without register spills; the Python argument errors.  seq_* is the
definition (a sequential loop over a per-class timestamp map); fast_* is what the GPU tests use on larger streams."""
import ctypes
import os
import re

import numpy as np
import pytest

import _header
import _plane_flow_np as N

SIZE = N.HAND_SIZE
BOTH = (N.seq_local_plane_flow, N.fast_local_plane_flow)


def last(fn, cols, dt=1000.0, **kw):
    """(vx, vy, lifetime, valid) of the event under test: the last of the stream"""
    flow, valid, life = fn(*cols, dt, SIZE, **kw)
    assert flow.dtype == np.float32 and life.dtype == np.float32 and valid.dtype == np.bool_
    assert np.array_equal(np.isnan(flow[:, 0]), ~valid) and np.array_equal(np.isnan(flow[:, 1]), ~valid)
    assert np.array_equal(np.isnan(life), ~valid)
    return float(flow[-1, 0]), float(flow[-1, 1]), float(life[-1]), bool(valid[-1])


# ---- hand-worked cases ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fn", BOTH)
def test_a_full_window_on_an_exact_plane(fn):
    assert last(fn, N.window_stream(N.plane_taus(4.0, 0.0))) == (0.25, 0.0, 4.0, True)
    assert last(fn, N.window_stream(N.plane_taus(0.0, -2.0))) == (0.0, -0.5, 2.0, True)
    vx, vy, life, ok = last(fn, N.window_stream(N.plane_taus(3.0, 4.0)))      # g = 25
    assert ok and (vx, vy, life) == (float(np.float32(3.0 / 25.0)), float(np.float32(4.0 / 25.0)), 5.0)
    for r in (1, 3, 4):
        assert last(fn, N.window_stream(N.plane_taus(4.0, 0.0, r), r), radius=r) == (0.25, 0.0, 4.0, True)
    # the other polarity is invisible under "same": only the centre is left
    cols = N.window_stream(N.plane_taus(4.0, 0.0))
    cols[3][:-1] = -1
    assert not last(fn, cols)[3] and last(fn, cols, polarity="ignore") == (0.25, 0.0, 4.0, True)


@pytest.mark.parametrize("fn", BOTH)
def test_collinear_samples_fail(fn):
    taus = [[None] * 5 for _ in range(5)]
    taus[2] = [4.0 * dx for dx in range(-2, 3)]       # the centre's own row: 5 samples on a line, D == 0
    assert not last(fn, N.window_stream(taus), min_samples=3)[3]
    taus = [[None] * 5 for _ in range(5)]
    for k in range(5):
        taus[k][k] = 3.0 * (k - 2)                     # a diagonal
    assert not last(fn, N.window_stream(taus), min_samples=3)[3]
    taus[1][2] = -7.0                                  # one sample off the line: a plane
    assert last(fn, N.window_stream(taus), min_samples=3)[3]


@pytest.mark.parametrize("fn", BOTH)
def test_min_samples(fn):
    taus = [[None] * 5 for _ in range(5)]
    taus[2][3], taus[3][2], taus[1][1], taus[3][4] = 4.0, 0.0, -4.0, 8.0      # with the centre: 5 samples on tau = 4 dx
    cols = N.window_stream(taus)
    assert last(fn, cols, min_samples=5) == (0.25, 0.0, 4.0, True)
    assert not last(fn, cols, min_samples=6)[3]        # n = min_samples - 1
    # dt takes a sample away: t_i - t_j = 4 > 3.5 for the sample at tau = -4
    assert not last(fn, cols, dt=3.5, min_samples=5)[3] and last(fn, cols, dt=4.0, min_samples=5)[3]


@pytest.mark.parametrize("fn", BOTH)
def test_one_gross_outlier_is_rejected(fn):
    taus = N.plane_taus(4.0, 0.0)
    taus[0][4] = 500.0                                 # instead of 8
    cols = N.window_stream(taus)
    plain = last(fn, cols)
    assert plain[3] and plain[:3] != (0.25, 0.0, 4.0)
    assert last(fn, cols, outlier_threshold=100.0, iterations=1) == (0.25, 0.0, 4.0, True)
    assert last(fn, cols, outlier_threshold=100.0, iterations=2) == (0.25, 0.0, 4.0, True)
    assert last(fn, cols, outlier_threshold=100.0, iterations=0) == plain
    assert last(fn, cols, outlier_threshold=1000.0, iterations=2) == plain      # nothing exceeds the threshold
    # (residuals of the first fit: 492 (1 - 0.2) = 393.6 at the outlier, at most 492 * 0.16 = 78.7 elsewhere)
    # a refit that fails makes the event invalid: 24 samples are left of the 25 wanted
    assert not last(fn, cols, outlier_threshold=100.0, iterations=1, min_samples=25)[3]
    assert last(fn, cols, outlier_threshold=100.0, iterations=0, min_samples=25) == plain


@pytest.mark.parametrize("fn", BOTH)
def test_a_zero_gradient_is_invalid(fn):
    assert not last(fn, N.window_stream(N.plane_taus(0.0, 0.0)))[3]           # a = b = 0: g == 0
    assert not last(fn, N.window_stream(N.plane_taus(0.0, 0.0)), dt=0.0)[3]


@pytest.mark.parametrize("fn", BOTH)
def test_max_speed_on_either_side(fn):
    cols = N.window_stream(N.plane_taus(4.0, 0.0))    # speed 1 / sqrt(g) = 0.25
    assert last(fn, cols, max_speed=0.25) == (0.25, 0.0, 4.0, True)
    assert not last(fn, cols, max_speed=float(np.nextafter(0.25, 0.0)))[3]
    assert last(fn, cols, max_speed=10.0)[3]


@pytest.mark.parametrize("fn", BOTH)
def test_the_window_is_clipped_to_the_sensor(fn):
    x, y, t, p = N.window_stream(N.plane_taus(4.0, 0.0))
    keep = x - 4 >= 0                                  # the centre moves to x = 1: the column dx = -2 falls off the sensor
    got = fn((x - 4)[keep], y[keep], t[keep], p[keep], 1000.0, SIZE)
    assert got[1][-1] and tuple(got[0][-1]) == (0.25, 0.0)
    for size in ((1, 1), (2, 5), (5, 2)):
        cols = random_stream(np.random.default_rng(3), 300, size[0], size[1], 40, False)
        flow, valid, _ = fn(*cols, 10.0, size, min_samples=3)
        assert flow.shape == (300, 2) and (size != (1, 1) or not valid.any())


# ---- fast_* against seq_* -----------------------------------------------------------------------------------------------------

def random_stream(rng, n, H, W, ticks, shuffle):
    """uniform noise and a moving column on integer ticks (ties occur); times unsorted with `shuffle`"""
    t = np.sort(rng.integers(0, ticks, n)).astype(np.float64)
    edge = rng.random(n) < 0.6
    x = np.where(edge, np.clip((t * W / max(ticks, 1)).astype(np.int64) + rng.integers(-1, 2, n), 0, W - 1), rng.integers(0, W, n))
    y = rng.integers(0, H, n)
    if shuffle:
        t = rng.permutation(t)
    return x, y, t, rng.integers(0, 2, n) * 2 - 1


@pytest.mark.parametrize("seed", range(40))
def test_fast_equals_seq(seed):
    rng = np.random.default_rng(7000 + seed)
    H, W = [(9, 9), (10, 13), (6, 11), (1, 1), (2, 5), (5, 2)][seed % 6]
    n = 0 if seed == 7 else int(rng.integers(1, 400))
    x, y, t, p = random_stream(rng, n, H, W, [8, 60, 1 << 30][seed % 3], seed % 4 == 1)
    r = seed % 4 + 1
    kw = dict(radius=r, polarity=("same", "ignore")[seed % 2], min_samples=[3, 5, 4][seed % 3],
              outlier_threshold=[None, 3.0, 1.0][seed % 3], iterations=(seed // 3) % 3,
              max_speed=[None, 2.0][seed % 2])
    dt = float([5, 20, 1 << 28][seed % 3])
    select = rng.integers(0, n, int(rng.integers(0, 2 * n))) if seed % 5 == 2 and n else None
    s = N.seq_local_plane_flow(x, y, t, p, dt, (H, W), select=select, **kw)
    f = N.fast_local_plane_flow(x, y, t, p, dt, (H, W), select=select, **kw)
    rows = n if select is None else len(select)
    assert s[0].shape == (rows, 2) and s[1].shape == s[2].shape == (rows,)
    for a, b in zip(s, f):
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if select is None:
        sf, sc = N.seq_plane_flow_field(x, y, t, p, dt, (H, W), **kw)
        ff, fc = N.fast_plane_flow_field(x, y, t, p, dt, (H, W), **kw)
        assert sf.dtype == np.float32 and sf.shape == (2, H, W) and sc.dtype == np.int32 and sc.shape == (H, W)
        assert sf.tobytes() == ff.tobytes() and np.array_equal(sc, fc) and sc.sum() == s[1].sum()
        assert not sf[:, sc == 0].any()


def test_the_edge_scene_populates_every_path():
    """the scene of the GPU tests: valid fits near the true flow, failed fits of both kinds, rejections that change the result"""
    x, y, t, p = N.edge_scene()
    assert len(x) == 3000 and (np.diff(t) >= 0).all() and (np.diff(t) == 0).sum() > 100
    size = (24, 32)
    plain = N.fast_local_plane_flow(x, y, t, p, N.EDGE_DT, size)
    rej = N.fast_local_plane_flow(x, y, t, p, N.EDGE_DT, size, outlier_threshold=N.EDGE_TH)
    for flow, valid, life in (plain, rej):
        assert 0.3 * len(x) < valid.sum() < 0.97 * len(x)
    assert (plain[1] != rej[1]).any() and (plain[0][plain[1] & rej[1]] != rej[0][plain[1] & rej[1]]).any()
    med = np.median(rej[0][rej[1]], axis=0)
    assert 0.010 < med[0] < 0.040 and 0.005 < med[1] < 0.020      # the edge moves at (0.020, 0.010), normal flow (0.020, 0.010)
    part = slice(0, 500)
    s = N.seq_local_plane_flow(x[part], y[part], t[part], p[part], N.EDGE_DT, size, outlier_threshold=N.EDGE_TH)
    for a, b in zip(s, rej):
        assert a.tobytes() == b[part].tobytes()
    field, count = N.fast_plane_flow_field(x, y, t, p, N.EDGE_DT, size, outlier_threshold=N.EDGE_TH)
    assert count.sum() == rej[1].sum() and count.max() >= 3 and (count == 0).any()


# ---- the public surface and the C ABI -----------------------------------------------------------------------------------------

def test_every_planeflow_prototype_is_bound_with_its_arguments():
    from event_utils_amd import _lib
    protos = _header.prototypes("evk_planeflow_")
    assert set(protos) == {"evk_planeflow_fit", "evk_planeflow_field"}
    for name, want in protos.items():
        assert _lib.PROTOTYPES[name] == want and want[1] is ctypes.c_int, name
        assert hasattr(_lib.lib(), name)
    assert (_lib.EVK_PLANEFLOW_MAX_RADIUS, _lib.EVK_PLANEFLOW_MAX_ITERATIONS) == (4, 8)
    header = _header.TEXT
    for name, value in (("EVK_PLANEFLOW_MAX_RADIUS", 4), ("EVK_PLANEFLOW_MAX_ITERATIONS", 8)):
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (name, value), header, re.M), name


def test_public_surface():
    import event_utils_amd as E
    import event_utils_amd.lib.features.plane_flow as alias
    from event_utils_amd import features
    from event_utils_amd.features import plane_flow
    assert alias is plane_flow
    for name in ("local_plane_flow", "plane_flow_field"):
        assert getattr(E, name) is getattr(plane_flow, name) is getattr(features, name)
    assert "features.plane_flow" in E.__doc__


def test_arguments_are_refused_before_the_device_is_touched():
    from event_utils_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every call below is refused first
    einval, f32, nan = -1, _lib.EVK_SELECT_F32, float("nan")

    def fit(kind=f32, t=fake, n=8, h=16, w=16, classes=2, radius=2, dt=1.0, m=5, use_th=0, th=0.0, it=2, use_ms=0, ms=0.0,
            select=None, rows=0, scratch=fake, flow=fake, life=fake, valid=fake):
        return L.evk_planeflow_fit(kind, t, n, h, w, classes, radius, dt, m, use_th, th, it, use_ms, ms, select, rows, scratch,
                                   flow, life, valid, None)

    def field(n=8, h=16, w=16, classes=2, scratch=fake, flow=fake, valid=fake, out=fake, count=fake):
        return L.evk_planeflow_field(n, h, w, classes, scratch, flow, valid, out, count, None)
    assert fit(kind=-1) == einval and fit(kind=5) == einval
    assert fit(n=-1) == einval and fit(n=1 << 31) == einval and fit(h=0) == einval and fit(w=-3) == einval
    assert fit(h=1 << 16, w=1 << 16) == einval          # more keys than a grouping holds
    assert fit(classes=0) == einval and fit(classes=3) == einval
    assert fit(select=fake, rows=-1) == einval and fit(rows=-1) == einval
    assert fit(t=None) == einval and fit(scratch=None) == einval and fit(flow=None) == einval and fit(valid=None) == einval
    assert fit(select=fake, rows=4, flow=None) == einval and fit(select=fake, rows=4, valid=None) == einval
    assert fit(n=0, t=None, select=fake, rows=3) == einval      # a selection from no events
    assert fit(scratch=ctypes.c_void_p(4100)) not in (0, einval)      # not aligned
    assert fit(radius=0) == einval and fit(radius=5) == einval and fit(radius=-1) == einval
    assert fit(dt=-1.0) == einval and fit(dt=nan) == einval
    assert fit(m=2) == einval and fit(m=26) == einval and fit(radius=1, m=10) == einval and fit(radius=4, m=82) == einval
    assert fit(use_th=1, th=0.0) == einval and fit(use_th=1, th=-1.0) == einval and fit(use_th=1, th=nan) == einval
    assert fit(th=nan) == einval and fit(use_th=2, th=1.0) == einval and fit(use_th=-1, th=1.0) == einval
    assert fit(it=-1) == einval and fit(it=9) == einval
    assert fit(use_ms=1, ms=0.0) == einval and fit(use_ms=1, ms=-2.0) == einval and fit(use_ms=1, ms=nan) == einval
    assert fit(ms=nan) == einval and fit(use_ms=2, ms=1.0) == einval
    # nothing to do: no launch (every parameter at an end of its range)
    assert fit(n=0, t=None, flow=None, valid=None, life=None) == 0 and fit(select=fake, rows=0, flow=None, valid=None) == 0
    assert fit(n=0, t=None, radius=1, m=9, dt=0.0, use_th=1, th=1e-300, it=8, use_ms=1, ms=1e300) == 0
    assert fit(n=0, t=None, radius=4, m=81, it=0) == 0 and fit(n=0, t=None, radius=1, m=3) == 0
    assert field(n=-1) == einval and field(n=1 << 31) == einval and field(h=0) == einval and field(w=-3) == einval
    assert field(h=1 << 16, w=1 << 16) == einval and field(classes=0) == einval and field(classes=3) == einval
    assert field(scratch=None) == einval and field(flow=None) == einval and field(valid=None) == einval
    assert field(out=None) == einval and field(count=None) == einval and field(n=0, flow=None, valid=None, out=None) == einval
    assert field(scratch=ctypes.c_void_p(4100)) not in (0, einval)


def test_planeflow_kernels_compile_without_register_spills(tmp_path):
    """Every kernel of evk_planeflow.hip (the fit for four radii, the field pass) compiles for gfx950 without spilling registers."""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    from event_utils_amd.csrc import build as B
    src = os.path.join(B.HERE, "evk_planeflow.hip")
    subprocess.run([hipcc] + list(B.CFLAGS) + ["-c", src, "-o", str(tmp_path / "pf.o"), "-save-temps=obj"], check=True, cwd=B.HERE,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert asm, os.listdir(tmp_path)
    text = open(tmp_path / asm[0]).read()
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    seen = {n: (int(v), int(sp)) for n, v, sp in kernels}
    assert sum("k_planeflow_fit" in n for n in seen) == 4 and sum("k_planeflow_field" in n for n in seen) == 1
    assert not {n: vs for n, vs in seen.items() if vs[1]}


def test_python_argument_errors_come_before_any_device_work():
    """every call below is refused on its arguments alone: none of them reaches the point where a missing GPU would matter"""
    import event_utils_amd as E
    x, y, t, p = np.array([5, 6]), np.array([5, 6]), np.array([1.0, 2.0]), np.array([1, -1])
    for fn in (E.local_plane_flow, E.plane_flow_field):
        for polarity in ("split", "both", None):
            with pytest.raises(ValueError):
                fn(x, y, t, p, 5.0, polarity=polarity)
        for bad in (-1.0, float("nan")):
            with pytest.raises(ValueError, match="dt"):
                fn(x, y, t, p, bad)
        for bad in (0, 5, -1, 1.5, True):
            with pytest.raises(ValueError, match="radius"):
                fn(x, y, t, p, 5.0, radius=bad)
        for bad, r in ((2, 2), (26, 2), (10, 1), (82, 4), (4.5, 2), (True, 2)):
            with pytest.raises(ValueError, match="min_samples"):
                fn(x, y, t, p, 5.0, radius=r, min_samples=bad)
        for bad in (0.0, -1.0, float("nan")):
            with pytest.raises(ValueError, match="outlier_threshold"):
                fn(x, y, t, p, 5.0, outlier_threshold=bad)
            with pytest.raises(ValueError, match="max_speed"):
                fn(x, y, t, p, 5.0, max_speed=bad)
        for bad in (-1, 9, 1.5, True):
            with pytest.raises(ValueError, match="iterations"):
                fn(x, y, t, p, 5.0, iterations=bad)
    with pytest.raises(TypeError):
        E.plane_flow_field(x, y, t, p, 5.0, select=[0])
