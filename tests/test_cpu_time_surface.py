"""CPU (no GPU): the two host restatements of the time-surface definitions (tests/_time_surface_np.py) agree with each other and
with a hand-worked stream, and have the properties the definitions imply; the evk_tsurf_* entries are declared, bound and
exported.  seq_* is the definition (a sequential loop over a per-pixel timestamp map; for HATS a per-pixel list of past times);
fast_* is what the GPU tests use on larger streams."""

import numpy as np
import pytest

import _header
import _time_surface_np as N

INF = np.inf
DECAYS = ("exp", "linear", None)


def random_stream(rng, n, H, W, sorted_times=True, ties=True):
    x = rng.integers(0, W, n)
    y = rng.integers(0, H, n)
    t = rng.integers(0, max(2, n // 2 if ties else 1 << 40), n).astype(np.float64)      # integer ticks: ties occur
    if sorted_times:
        t = np.sort(t)
    p = rng.integers(0, 2, n) * 2 - 1
    return x, y, t, p


def same(a, b):
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a, b, equal_nan=True)


def configurations():
    """60 seeded configurations: radius 1..4, every decay and polarity, ties, unsorted times where allowed, select with repeats,
    cell sizes that do not divide the sensor, sensors down to 1 x 1."""
    sensors = [(1, 1), (1, 7), (6, 1), (2, 2), (5, 8), (12, 9)]
    out = []
    for seed in range(60):
        rng = np.random.default_rng(7000 + seed)
        H, W = sensors[seed % len(sensors)]
        n = 0 if seed in (6, 7) else int(rng.integers(0, 401))
        out.append(dict(seed=seed, H=H, W=W, n=n, radius=1 + seed % 4, decay=DECAYS[seed % 3],
                        polarity=("ignore", "same", "split")[(seed // 3) % 3], include_self=bool(seed & 1),
                        sorted_times=seed % 5 != 0, ties=seed % 4 != 3, select=seed % 3 == 1,
                        tau=[1.0, 7.5, 300.0][seed % 3], dt=[0.0, 3.0, 40.0, 1e30][seed % 4], cell=[1, 2, 3, 5, 100][seed % 5],
                        normalise=bool(seed & 2)))
    return out


@pytest.mark.parametrize("cfg", configurations(), ids=lambda c: "seed%d" % c["seed"])
def test_fast_equals_seq(cfg):
    rng = np.random.default_rng(cfg["seed"])
    H, W, n = cfg["H"], cfg["W"], cfg["n"]
    x, y, t, p = random_stream(rng, n, H, W, cfg["sorted_times"], cfg["ties"])
    ts_sorted = np.sort(t)
    # per-event surfaces: unsorted times allowed
    select = rng.integers(0, n, int(rng.integers(0, 2 * n + 1))) if cfg["select"] and n else (np.zeros(0, np.int64) if cfg["select"] else None)
    kw = dict(radius=cfg["radius"], decay=cfg["decay"], polarity=cfg["polarity"], include_self=cfg["include_self"], select=select)
    s = N.seq_local_time_surfaces(x, y, t, p, cfg["tau"], (H, W), **kw)
    f = N.fast_local_time_surfaces(x, y, t, p, cfg["tau"], (H, W), **kw)
    P = 2 * cfg["radius"] + 1
    assert s.shape == (n if select is None else len(select), 2 if cfg["polarity"] == "split" else 1, P, P)
    assert s.dtype == (np.float64 if cfg["decay"] is None else np.float32)
    same(s, f)
    # surfaces at cuts (any times) and at reference times (sorted times)
    pol = "ignore" if cfg["polarity"] == "ignore" else "split"
    cuts = np.concatenate([[0, n], rng.integers(0, n + 1, 3)])
    s = N.seq_time_surfaces(x, y, t, p, cfg["tau"], (H, W), indices=cuts, decay=cfg["decay"], polarity=pol)
    f = N.fast_time_surfaces(x, y, t, p, cfg["tau"], (H, W), indices=cuts, decay=cfg["decay"], polarity=pol)
    assert s.shape == (5, 1 if pol == "ignore" else 2, H, W)
    same(s, f)
    refs = np.concatenate([[-1.0, 1e12], rng.integers(0, max(2, n // 2), 2) + 0.0, rng.random(1) * max(1, n // 2)])
    s = N.seq_time_surfaces(x, y, ts_sorted, p, cfg["tau"], (H, W), t_refs=refs, decay=cfg["decay"], polarity=pol)
    f = N.fast_time_surfaces(x, y, ts_sorted, p, cfg["tau"], (H, W), t_refs=refs, decay=cfg["decay"], polarity=pol)
    same(s, f)
    # HATS: sorted times
    kw = dict(cell_size=cfg["cell"], radius=cfg["radius"], normalise=cfg["normalise"], return_counts=True)
    sh, sc = N.seq_averaged_time_surfaces(x, y, ts_sorted, p, cfg["tau"], cfg["dt"], (H, W), **kw)
    fh, fc = N.fast_averaged_time_surfaces(x, y, ts_sorted, p, cfg["tau"], cfg["dt"], (H, W), **kw)
    cell = cfg["cell"]
    assert sh.shape == (-(-H // cell), -(-W // cell), 2, P, P) and sh.dtype == np.float32 and sc.dtype == np.int32
    same(sc, fc)
    assert int(sc.sum()) == n
    # the two sum the same terms in another order: float64 sums of fewer than 2^20 terms in (0, 1], then one rounding to float32
    assert np.array_equal(sh == 0, fh == 0)
    assert (np.abs(sh - fh) <= np.spacing(np.abs(sh))).all()


# A 3 x 4 sensor (H = 3, W = 4); events in stream order, times non-decreasing with two ties:
#   i  (x, y)  t   p
#   0  (1, 1)  10  +
#   1  (2, 1)  12  -
#   2  (1, 1)  13  +
#   3  (0, 0)  15  +
#   4  (1, 0)  15  -
#   5  (1, 1)  16  -
#   6  (2, 1)  16  -
#   7  (1, 1)  20  +
HAND = dict(x=[1, 2, 1, 0, 1, 1, 2, 1], y=[1, 1, 1, 0, 0, 1, 1, 1], t=[10, 12, 13, 15, 15, 16, 16, 20], p=[1, -1, 1, 1, -1, -1, -1, 1])
SIZE = (3, 4)


def hand():
    return tuple(np.array(HAND[k]) for k in "xytp")


def surface(C, entries):
    """a (C, 3, 4) surface of +inf ages with the listed (c, y, x) -> age"""
    s = np.full((C,) + SIZE, INF)
    for (c, y, x), a in entries.items():
        s[c, y, x] = a
    return s


def test_hand_worked_surfaces_of_active_events():
    x, y, t, p = hand()
    for fn in (N.seq_time_surfaces, N.fast_time_surfaces):
        # the first five events, T = t[4] = 15: "-" has (2,1) at 12 and (1,0) at 15; "+" has (1,1) at 13 (its later stamp) and (0,0) at 15
        cut5 = surface(2, {(0, 1, 2): 3.0, (0, 0, 1): 0.0, (1, 1, 1): 2.0, (1, 0, 0): 0.0})
        # t_refs = 16: the events with t < 16 are the same five, every age is one larger
        ref16 = surface(2, {(0, 1, 2): 4.0, (0, 0, 1): 1.0, (1, 1, 1): 3.0, (1, 0, 0): 1.0})
        same(fn(x, y, t, p, 4.0, SIZE, indices=[5, 0], decay=None), np.stack([cut5, surface(2, {})]))
        same(fn(x, y, t, p, 4.0, SIZE, t_refs=[16.0], decay=None), ref16[None])
        # all eight, one class, T = 20: (1,1) at 20, (2,1) at 16, (0,0) and (1,0) at 15
        same(fn(x, y, t, None, 4.0, SIZE, indices=[8], decay=None, polarity="ignore"),
             surface(1, {(0, 1, 1): 0.0, (0, 1, 2): 4.0, (0, 0, 0): 5.0, (0, 0, 1): 5.0})[None])
        # linear with tau = 4: 1 - 3/4, 1 - 0, 1 - 2/4, 1 - 0, empty pixels 0;  exp: exp(-age / 4)
        lin = np.zeros((2,) + SIZE, dtype=np.float32)
        lin[0, 1, 2], lin[0, 0, 1], lin[1, 1, 1], lin[1, 0, 0] = 0.25, 1.0, 0.5, 1.0
        same(fn(x, y, t, p, 4.0, SIZE, indices=[5], decay="linear"), lin[None])
        ex = np.zeros((2,) + SIZE, dtype=np.float32)
        ex[0, 1, 2], ex[0, 0, 1], ex[1, 1, 1], ex[1, 0, 0] = np.float32(np.exp(-0.75)), 1.0, np.float32(np.exp(-0.5)), 1.0
        same(fn(x, y, t, p, 4.0, SIZE, indices=[5]), ex[None])


def test_hand_worked_local_surfaces():
    x, y, t, p = hand()
    I = INF
    for fn in (N.seq_local_time_surfaces, N.fast_local_time_surfaces):
        def patch(i, **kw):
            return fn(x, y, t, p, 4.0, SIZE, radius=1, decay=None, select=[i], **kw)[0].tolist()
        # event 7, (1,1) "+" at 20: earlier "+" events at (1,1) (13, the centre) and (0,0) (15)
        assert patch(7) == [[[5, I, I], [I, 0, I], [I, I, I]]]
        assert patch(7, include_self=False) == [[[5, I, I], [I, 7, I], [I, I, I]]]
        # event 6, (2,1) "-" at 16: earlier "-" events at (1,0) (15), (1,1) (16, a tie with a smaller index) and (2,1) itself (12)
        assert patch(6) == [[[1, I, I], [0, 0, I], [I, I, I]]]
        assert patch(6, include_self=False) == [[[1, I, I], [0, 4, I], [I, I, I]]]
        # split: channel 0 is its own class; channel 1 ("+") sees (1,1) at 13, and its centre is not forced
        assert patch(6, polarity="split") == [[[1, I, I], [0, 0, I], [I, I, I]], [[I, I, I], [3, I, I], [I, I, I]]]
        # one class, no self: (1,0) at 15, (1,1) at 16 (event 5), (2,1) at 12
        assert patch(6, polarity="ignore", include_self=False) == [[[1, I, I], [0, 4, I], [I, I, I]]]
        # event 3, the corner (0,0) "+" at 15: the row above and the column to the left are off the sensor; (1,1) "+" at 13
        assert patch(3) == [[[I, I, I], [I, 0, I], [I, I, 2]]]
        # the first event has no history
        assert patch(0, include_self=False) == [[[I] * 3] * 3]
        full = fn(x, y, t, p, 4.0, SIZE, radius=1, decay="linear")
        assert full.shape == (8, 1, 3, 3) and full.dtype == np.float32
        assert full[6, 0].tolist() == [[0.75, 0, 0], [1, 1, 0], [0, 0, 0]]


def test_hand_worked_hats():
    """cell_size 2 on 3 x 4: cells (gy, gx) = (y // 2, x // 2).  (1,1), (0,0), (1,0) lie in cell (0,0); (2,1) in cell (0,1).
    tau = 4, dt = 5, e(a) = exp(-a / 4):
      "+" cell (0,0): event 2 sees (1,1) at 10 (age 3) at the centre; event 3 at (0,0) sees (1,1) at 10 and 13 (ages 5 and 2) at
                      (dy, dx) = (+1, +1); event 7 sees (1,1) at 10, 13 (ages 10, 7 > dt) and (0,0) at 15 (age 5) at (-1, -1)
      "-" cell (0,0): event 5 at (1,1) sees (1,0) at 15 (age 1) at (-1, 0); (2,1) at 12 lies in ANOTHER cell and is not seen
      "-" cell (0,1): event 6 at (2,1) sees itself at 12 (age 4) at the centre; (1,1) at 16 lies in another cell"""
    x, y, t, p = hand()

    def e(a):
        return np.exp(-a / 4.0)
    want = np.zeros((2, 2, 2, 3, 3))
    want[0, 0, 1, 1, 1] = e(3)
    want[0, 0, 1, 2, 2] = e(5) + e(2)
    want[0, 0, 1, 0, 0] = e(5)
    want[0, 0, 0, 0, 1] = e(1)
    want[0, 1, 0, 1, 1] = e(4)
    counts = np.zeros((2, 2, 2), dtype=np.int32)
    counts[0, 0, 1], counts[0, 0, 0], counts[0, 1, 0] = 4, 2, 2
    norm = want.copy()
    norm[0, 0, 1] /= 4
    norm[0, 0, 0] /= 2
    norm[0, 1, 0] /= 2
    for fn in (N.seq_averaged_time_surfaces, N.fast_averaged_time_surfaces):
        h, c = fn(x, y, t, p, 4.0, 5.0, SIZE, cell_size=2, radius=1, normalise=False, return_counts=True)
        same(h, want.astype(np.float32))
        same(c, counts)
        same(fn(x, y, t, p, 4.0, 5.0, SIZE, cell_size=2, radius=1), norm.astype(np.float32))
        # dt = 0: the only ties (15 / 15 and 16 / 16) are of different classes or cells
        assert not fn(x, y, t, p, 4.0, 0.0, SIZE, cell_size=2, radius=1).any()
        # one cell over the whole sensor: event 5 now sees (2,1) at 12 (age 4) at (0, +1), event 6 sees (1,1) at 16 (age 0) at (0, -1)
        one = fn(x, y, t, p, 4.0, 5.0, SIZE, cell_size=4, radius=1, normalise=False)
        assert one.shape == (1, 1, 2, 3, 3)
        wide = np.zeros((3, 3))
        wide[0, 1], wide[1, 2], wide[1, 1], wide[1, 0], wide[0, 0] = e(1), e(4), e(4), e(0), e(1)      # (1,0) at 15 is also (-1,-1) of event 6
        wide[2, 2] = e(3)                                  # event 4 at (1,0) sees (2,1) at 12 at (+1, +1)
        same(one[0, 0, 0], wide.astype(np.float32))


# ---- properties ---------------------------------------------------------------------------------------------------------------

def test_exp_values_lie_in_the_unit_interval_on_sorted_input():
    rng = np.random.default_rng(21)
    x, y, t, p = random_stream(rng, 500, 7, 9)
    loc = N.fast_local_time_surfaces(x, y, t, p, 20.0, (7, 9), radius=2, polarity="split")
    glo = N.fast_time_surfaces(x, y, t, p, 20.0, (7, 9), indices=[100, 500])
    for v in (loc, glo):
        assert v.min() >= 0.0 and v.max() <= 1.0 and v.max() > 0.0
    shuffled = rng.permutation(t)                      # unsorted: a negative age gives a value above 1
    assert N.fast_local_time_surfaces(x, y, shuffled, p, 20.0, (7, 9), radius=2).max() > 1.0


@pytest.mark.parametrize("decay", DECAYS)
def test_the_centre_is_the_event_itself_with_include_self(decay):
    rng = np.random.default_rng(22)
    x, y, t, p = random_stream(rng, 300, 5, 6, sorted_times=False)
    for polarity in ("ignore", "same"):
        v = N.fast_local_time_surfaces(x, y, t, p, 9.0, (5, 6), radius=3, decay=decay, polarity=polarity)
        assert (v[:, 0, 3, 3] == (0.0 if decay is None else 1.0)).all()
    v = N.fast_local_time_surfaces(x, y, t, p, 9.0, (5, 6), radius=3, decay=decay, polarity="split")
    own = (p > 0).astype(int)
    assert (v[np.arange(300), own, 3, 3] == (0.0 if decay is None else 1.0)).all()


def test_hats_without_a_window_is_zero_on_tie_free_input():
    rng = np.random.default_rng(23)
    x, y, t, p = random_stream(rng, 400, 6, 7, ties=False)
    assert len(np.unique(t)) == 400
    for fn in (N.seq_averaged_time_surfaces, N.fast_averaged_time_surfaces):
        h, c = fn(x, y, t, p, 5.0, 0.0, (6, 7), cell_size=3, radius=2, return_counts=True)
        assert not h.any() and c.sum() == 400
    assert N.fast_averaged_time_surfaces(x, y, t, p, 1e12, 1e30, (6, 7), cell_size=3, radius=2).any()      # (times up to 2^40)


@pytest.mark.parametrize("include_self", [False, True])
def test_the_own_channel_of_split_is_the_same_polarity_surface(include_self):
    rng = np.random.default_rng(24)
    x, y, t, p = random_stream(rng, 350, 6, 5, sorted_times=False)
    kw = dict(radius=2, decay=None, include_self=include_self)
    split = N.fast_local_time_surfaces(x, y, t, p, 3.0, (6, 5), polarity="split", **kw)
    own = N.fast_local_time_surfaces(x, y, t, p, 3.0, (6, 5), polarity="same", **kw)
    same(split[np.arange(350), (p > 0).astype(int)], own[:, 0])


def test_a_local_surface_is_the_window_of_the_surface_before_the_event():
    """L[i] (one class, no self) = the surface of active events at the cut i, re-timed to t_i, around the event's pixel"""
    rng = np.random.default_rng(25)
    H, W, n, r = 6, 7, 120, 2
    x, y, t, p = random_stream(rng, n, H, W, sorted_times=False)
    loc = N.seq_local_time_surfaces(x, y, t, p, 1.0, (H, W), radius=r, decay=None, polarity="ignore", include_self=False)
    for i in range(1, n):
        age = N.seq_time_surfaces(x, y, t, p, 1.0, (H, W), indices=[i], decay=None, polarity="ignore")[0, 0] + (t[i] - t[i - 1])
        pad = np.full((H + 2 * r, W + 2 * r), INF)
        pad[r:r + H, r:r + W] = age
        assert np.array_equal(loc[i, 0], pad[y[i]:y[i] + 2 * r + 1, x[i]:x[i] + 2 * r + 1])


# ---- the public surface and the C ABI -----------------------------------------------------------------------------------------

def test_every_tsurf_prototype_is_bound_with_its_arguments():
    import ctypes
    from event_utils_amd import _lib
    protos = _header.prototypes("evk_tsurf_")
    assert set(protos) == {"evk_tsurf_scratch_bytes", "evk_tsurf_check_sorted", "evk_tsurf_global", "evk_tsurf_local", "evk_tsurf_hats"}
    for name, (want, ret) in protos.items():
        assert ret in (ctypes.c_int, ctypes.c_int64), name
        assert _lib.PROTOTYPES[name] == (want, ret), (name, _lib.PROTOTYPES[name], want)
        assert hasattr(_lib.lib(), name)
    assert _lib.EVK_TSURF_MAX_RADIUS == 4
    assert (_lib.EVK_TSURF_EXP, _lib.EVK_TSURF_LINEAR, _lib.EVK_TSURF_AGE) == (0, 1, 2)


def test_public_surface():
    import event_utils_amd as E
    import event_utils_amd.lib.representations.time_surface as alias
    from event_utils_amd import representations
    from event_utils_amd.representations import time_surface
    assert alias is time_surface
    for name in ("time_surfaces", "local_time_surfaces", "averaged_time_surfaces"):
        assert getattr(E, name) is getattr(time_surface, name) is getattr(representations, name)
    assert "time_surface" in E.__doc__


def test_arguments_are_refused_before_the_device_is_touched():
    import ctypes
    from event_utils_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every call below is refused first
    einval = -1
    assert L.evk_tsurf_scratch_bytes(-1) == einval and L.evk_tsurf_scratch_bytes(1 << 31) == einval
    assert L.evk_tsurf_scratch_bytes(0) == 0 and L.evk_tsurf_scratch_bytes(33) == 512
    f32 = _lib.EVK_SELECT_F32
    assert L.evk_tsurf_check_sorted(7, fake, 8, fake, None) == einval
    assert L.evk_tsurf_check_sorted(f32, fake, 8, None, None) == einval
    assert L.evk_tsurf_check_sorted(f32, None, 1, fake, None) == einval

    def glob(kind=f32, n=8, h=4, w=4, classes=2, nq=1, cuts=fake, decay=0, tau=1.0, scratch=fake, out=fake):
        return L.evk_tsurf_global(kind, fake, n, h, w, classes, nq, cuts, None, decay, tau, scratch, out, None)
    assert glob(kind=-1) == einval and glob(n=-1) == einval and glob(h=0) == einval and glob(classes=3) == einval
    assert glob(nq=-1) == einval and glob(cuts=None) == einval and glob(decay=3) == einval and glob(tau=0.0) == einval
    assert glob(tau=float("nan")) == einval and glob(scratch=None) == einval and glob(out=None) == einval
    assert glob(scratch=ctypes.c_void_p(4100)) not in (0, einval)

    def local(radius=1, classes=2, split=0, tau=1.0, decay=0, m=0, scratch=fake, out=fake):
        return L.evk_tsurf_local(f32, fake, 8, 4, 4, classes, radius, decay, tau, split, 1, None, m, scratch, out, None)
    assert local(radius=0) == einval and local(radius=5) == einval and local(classes=1, split=1) == einval
    assert local(tau=-1.0) == einval and local(decay=-1) == einval and local(scratch=None) == einval and local(out=None) == einval

    def hats(cell=2, radius=1, tau=1.0, dt=1.0, scratch=fake, ts=fake, nbytes=1 << 20, out=fake):
        return L.evk_tsurf_hats(f32, fake, 8, 4, 4, cell, radius, tau, dt, 1, scratch, ts, nbytes, out, None, None)
    assert hats(cell=0) == einval and hats(radius=5) == einval and hats(tau=0.0) == einval and hats(dt=-1.0) == einval
    assert hats(dt=float("nan")) == einval and hats(ts=None) == einval and hats(out=None) == einval
    assert hats(nbytes=8) not in (0, einval) and hats(ts=ctypes.c_void_p(4104)) not in (0, einval)
