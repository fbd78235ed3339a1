"""CPU (no GPU): the host restatements of the corner definitions (tests/_corners_np.py) against hand-built streams and against
each other; the evk_corner_* entries are declared, bound and exported and refuse bad arguments before they touch the device; the
Python argument errors.  seq_* is the definition (a sequential loop over a per-class map, every start and every length of an
arc); fast_* is what the GPU tests use on larger streams."""
import ctypes
import re

import numpy as np
import pytest

import _corners_np as N
import _header

SIZE = N.HAND_SIZE
FAST = (N.seq_fast_corners, N.fast_fast_corners)
HARRIS = (N.seq_harris_scores, N.fast_harris_scores)
GOOD3, GOOD4 = N.arc(16, 2, 4), N.arc(20, 5, 6)       # valid arcs, held fixed while the other circle varies


def near(got, want):
    """a float32 score against the float64 formula: one rounding, and the order of the float64 sums"""
    return abs(float(got) - want) <= 2.0 ** -23 * abs(want) + 1e-10


def centre_flag(fn, cols, **kw):
    """the flag of the event under test: the last of the stream"""
    return bool(fn(*cols, SIZE, **kw)[-1])


# ---- eFAST against hand-built streams -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("fn", FAST)
@pytest.mark.parametrize("length,want", [(2, False), (3, True), (6, True), (7, False)])
def test_c3_arc_lengths(fn, length, want):
    for start in (0, 5, 11):
        assert centre_flag(fn, N.circle_stream(N.arc(16, start, length), GOOD4)) is want


@pytest.mark.parametrize("fn", FAST)
@pytest.mark.parametrize("length,want", [(3, False), (4, True), (8, True), (9, False)])
def test_c4_arc_lengths(fn, length, want):
    for start in (0, 7, 13):
        assert centre_flag(fn, N.circle_stream(GOOD3, N.arc(20, start, length))) is want


@pytest.mark.parametrize("fn", FAST)
def test_arcs_that_wrap_past_element_zero(fn):
    assert centre_flag(fn, N.circle_stream(N.arc(16, 14, 5), GOOD4))
    assert centre_flag(fn, N.circle_stream(GOOD3, N.arc(20, 17, 7)))
    assert centre_flag(fn, N.circle_stream(N.arc(16, 15, 3), N.arc(20, 19, 4)))


@pytest.mark.parametrize("fn", FAST)
def test_the_rest_of_a_circle_may_be_unfired_but_an_arc_may_not(fn):
    v3 = [None if v == 1.0 else v for v in GOOD3]     # only the arc fired: every arc value beats -inf
    assert centre_flag(fn, N.circle_stream(v3, GOOD4))
    # an arc of 5 with one pixel unfired: without an end a valid arc of 4 is left, a hole inside splits the newest values in two
    for hole in range(5):
        v3 = N.arc(16, 4, 5)
        v3[4 + hole] = None
        assert centre_flag(fn, N.circle_stream(v3, GOOD4)) is (hole in (0, 4))
    v3 = N.arc(16, 4, 5)
    v3[5], v3[6], v3[7], v3[8] = None, 12.0, 13.0, 14.0      # ... unless the piece beside the hole is newer than the other one
    assert centre_flag(fn, N.circle_stream(v3, GOOD4))
    v3 = [None] * 16
    assert not centre_flag(fn, N.circle_stream(v3, GOOD4))      # nothing fired: no arc
    v4 = N.arc(20, 3, 4)
    v4[4] = None
    assert not centre_flag(fn, N.circle_stream(GOOD3, v4))


@pytest.mark.parametrize("fn", FAST)
def test_a_tie_with_an_outside_element_defeats_the_arc(fn):
    v3 = N.arc(16, 6, 3)
    assert centre_flag(fn, N.circle_stream(v3, GOOD4))
    tied = list(v3)
    tied[6] = 1.0                                      # an end of the arc as old as the rest: two newer elements are left
    assert not centre_flag(fn, N.circle_stream(tied, GOOD4))
    tied = list(v3)
    tied[12] = v3[6]                                   # an outside element as new as the arc's oldest
    assert not centre_flag(fn, N.circle_stream(tied, GOOD4))
    equal_inside = N.arc(16, 6, 3)
    equal_inside[7] = equal_inside[8] = 11.0           # a tie INSIDE the arc is harmless, distinct times are too
    assert centre_flag(fn, N.circle_stream(equal_inside, GOOD4))
    v4 = N.arc(20, 9, 4)
    v4[0] = v4[9]
    assert not centre_flag(fn, N.circle_stream(GOOD3, v4))


@pytest.mark.parametrize("fn", FAST)
def test_the_other_polarity_is_invisible_under_same_and_visible_under_ignore(fn):
    cols = N.circle_stream(GOOD3, GOOD4, p3=-1)        # the inner circle fired with the other polarity
    assert not centre_flag(fn, cols, polarity="same")
    assert centre_flag(fn, cols, polarity="ignore")
    cols = N.circle_stream(GOOD3, GOOD4, p3=-1, p4=-1)
    assert not centre_flag(fn, cols, polarity="same") and centre_flag(fn, cols, polarity="ignore")
    # a stale inner circle of the event's own polarity under a fresh one of the other: "ignore" sees the fresh times
    x, y, t, p = N.circle_stream(GOOD3, GOOD4)
    x2, y2, t2, p2 = N.circle_stream([50.0] * 16, [None] * 20, p3=-1)
    both = tuple(np.concatenate([a[:-1], b]) for a, b in ((x, x2), (y, y2), (t, t2), (p, p2)))
    assert centre_flag(fn, both, polarity="same") and not centre_flag(fn, both, polarity="ignore")


@pytest.mark.parametrize("fn", FAST)
def test_border_events_are_never_corners(fn):
    x, y, t, p = N.circle_stream(GOOD3, GOOD4)
    assert fn(x, y, t, p, SIZE)[-1]
    for dx, dy, size in ((-3, 0, SIZE), (0, -3, SIZE), (0, 0, (13, 10)), (0, 0, (10, 20))):      # x = 3; y = 3; x = W - 4; y = H - 4
        keep = (x + dx >= 0) & (y + dy >= 0) & (x + dx < size[1]) & (y + dy < size[0])
        assert keep[-1] and not fn((x + dx)[keep], (y + dy)[keep], t[keep], p[keep], size)[-1]
    rng = np.random.default_rng(5)
    for size in ((8, 40), (40, 8), (1, 1)):            # no pixel is 4 away from every border
        cols = random_stream(rng, 400, size[0], size[1], 50, False)
        assert not fn(*cols, size).any()


# ---- Harris against hand-worked patches ---------------------------------------------------------------------------------------

def test_the_score_of_a_lone_centre_bit():
    """b = the centre only: Ix[a][c] = S[4 - a] D[4 - c], Iy[a][c] = D[4 - a] S[4 - c]"""
    Ix = np.outer(N.S[::-1], N.D[::-1]).astype(np.float64)
    Iy = np.outer(N.D[::-1], N.S[::-1]).astype(np.float64)
    A, B, C = ((N.G * a * b).sum() / 144.0 for a, b in ((Ix, Ix), (Iy, Iy), (Ix, Iy)))
    want = A * B - C * C - 0.04 * (A + B) ** 2
    assert abs(A - B) < 1e-14 and abs(C) < 1e-14 and want > 0
    assert abs(N.harris_score_of_patch(N.lone_patch()) - want) < 1e-15
    for fn in HARRIS:
        got = fn([6], [6], [3.0], [1], SIZE, n_last=1)
        assert got.dtype == np.float32 and near(got[0], want)
        assert np.isnan(fn([3], [6], [3.0], [1], SIZE, dt=1.0)[0])      # on the border


@pytest.mark.parametrize("fn", HARRIS)
def test_edge_and_corner_patches(fn):
    edge = fn(*N.patch_stream(N.edge_patch()), SIZE, n_last=1000)[-1]
    ell = fn(*N.patch_stream(N.l_patch()), SIZE, n_last=1000)[-1]
    assert near(edge, N.harris_score_of_patch(N.edge_patch())) and near(ell, N.harris_score_of_patch(N.l_patch()))
    assert edge < 0 < ell and ell > 2.0
    assert near(fn(*N.patch_stream(N.edge_patch().T), SIZE, n_last=1000)[-1], float(edge))      # a horizontal line: the same score
    k0 = fn(*N.patch_stream(N.l_patch()), SIZE, n_last=1000, k=0.0)[-1]
    assert k0 > ell


@pytest.mark.parametrize("fn", HARRIS)
def test_window_boundaries_are_inclusive(fn):
    b = N.lone_patch()
    b[4, 6] = 1
    lone = fn([6], [6], [0.0], [1], SIZE, n_last=1)[0]
    pair = fn([8, 6], [6, 6], [0.0, 1.0], [1, 1], SIZE, n_last=1)[-1]
    assert near(lone, N.harris_score_of_patch(N.lone_patch())) and near(pair, N.harris_score_of_patch(b)) and abs(pair - lone) > 0.01
    # the neighbour is event 0; four events outside the patch; the event under test is event 5
    x, y = np.array([8, 15, 15, 15, 15, 6]), np.array([6, 6, 6, 6, 6, 6])
    t, p = np.array([3.0, 4.0, 5.0, 6.0, 7.0, 10.0]), np.ones(6, dtype=np.int64)
    assert fn(x, y, t, p, SIZE, n_last=5)[-1] == pair and fn(x, y, t, p, SIZE, n_last=4)[-1] == lone      # 0 >= 5 - 5
    assert fn(x, y, t, p, SIZE, dt=7.0)[-1] == pair and fn(x, y, t, p, SIZE, dt=np.nextafter(7.0, 0.0))[-1] == lone
    assert fn(x, y, t, p, SIZE, dt=0.0)[-1] == lone
    t[0] = 10.0                                        # a tie with the event under test: within dt = 0
    assert fn(x, y, t, p, SIZE, dt=0.0)[-1] == pair
    p[0] = -1                                          # the other polarity
    assert fn(x, y, t, p, SIZE, dt=0.0)[-1] == lone and fn(x, y, t, p, SIZE, dt=0.0, polarity="ignore")[-1] == pair
    with pytest.raises(TypeError):
        fn(x, y, t, p, SIZE)
    with pytest.raises(TypeError):
        fn(x, y, t, p, SIZE, n_last=3, dt=1.0)


# ---- fast_* against seq_* -----------------------------------------------------------------------------------------------------

def random_stream(rng, n, H, W, ticks, shuffle):
    """a few bright blobs and uniform noise on integer ticks (ties occur); times unsorted with `shuffle`"""
    blob = rng.random(n) < 0.7
    cx, cy = rng.integers(0, W, 3), rng.integers(0, H, 3)
    which = rng.integers(0, 3, n)
    x = np.where(blob, np.clip(cx[which] + rng.integers(-3, 4, n), 0, W - 1), rng.integers(0, W, n))
    y = np.where(blob, np.clip(cy[which] + rng.integers(-3, 4, n), 0, H - 1), rng.integers(0, H, n))
    t = np.sort(rng.integers(0, ticks, n)).astype(np.float64)
    if shuffle:
        t = rng.permutation(t)
    return x, y, t, rng.integers(0, 2, n) * 2 - 1


@pytest.mark.parametrize("seed", range(40))
def test_fast_equals_seq(seed):
    rng = np.random.default_rng(9000 + seed)
    H, W = [(9, 9), (10, 13), (14, 11), (1, 1), (8, 12), (16, 16)][seed % 6]
    n = 0 if seed == 7 else int(rng.integers(1, 500))
    x, y, t, p = random_stream(rng, n, H, W, [8, 60, 1 << 30][seed % 3], seed % 4 == 1)
    polarity = ("same", "ignore")[seed % 2]
    select = rng.integers(0, n, int(rng.integers(0, 2 * n))) if seed % 5 == 2 and n else None
    s = N.seq_fast_corners(x, y, t, p, (H, W), polarity, select)
    f = N.fast_fast_corners(x, y, t, p, (H, W), polarity, select)
    assert s.dtype == f.dtype == np.bool_ and s.shape == (n if select is None else len(select),) and np.array_equal(s, f)
    kw = dict(n_last=int(rng.integers(1, 120))) if seed % 2 else dict(dt=float(rng.integers(0, 30)))
    kw.update(polarity=polarity, k=[0.04, 0.0, 0.1][seed % 3], select=select)
    s, f = N.seq_harris_scores(x, y, t, p, (H, W), **kw), N.fast_harris_scores(x, y, t, p, (H, W), **kw)
    assert s.dtype == f.dtype == np.float32 and s.shape == f.shape and np.array_equal(np.isnan(s), np.isnan(f))
    el = N._eligible(x, y, H, W)
    assert np.array_equal(np.isnan(s), ~(el if select is None else el[select]))
    ok = ~np.isnan(s)                                  # the same float64 terms in another order of summation, then one rounding
    assert (np.abs(s[ok].astype(np.float64) - f[ok]) <= 2.0 ** -23 * np.abs(s[ok]) + 1e-10).all()


def test_the_mixed_scene_has_corners_and_non_corners():
    """the scene of the GPU tests: every detector finds at least 20 corners and leaves at least 20 eligible events"""
    x, y, t, p, size = N.mixed_scene()
    assert len(x) == 3300 and (np.diff(t) >= 0).all() and (np.diff(t) == 0).sum() > 2000
    el = N._eligible(x, y, *size)
    part = slice(0, 700)
    for polarity in ("same", "ignore"):
        f = N.fast_fast_corners(x, y, t, p, size, polarity)
        assert f.sum() >= 20 and (el & ~f).sum() >= 20 and not f[~el].any()
        assert np.array_equal(f[part], N.seq_fast_corners(x[part], y[part], t[part], p[part], size, polarity))
    for kw in (dict(n_last=200), dict(dt=15.0)):
        c = N.fast_harris_scores(x, y, t, p, size, **kw) > 8.0
        assert c.sum() >= 20 and (el & ~c).sum() >= 20


# ---- the public surface and the C ABI -----------------------------------------------------------------------------------------

def test_every_corner_prototype_is_bound_with_its_arguments():
    from event_utils_amd import _lib
    protos = _header.prototypes("evk_corner_")
    assert set(protos) == {"evk_corner_fast", "evk_corner_harris"}
    for name, want in protos.items():
        assert _lib.PROTOTYPES[name] == want and want[1] is ctypes.c_int, name
        assert hasattr(_lib.lib(), name)
    assert _lib.EVK_CORNER_BORDER == 4 == N.BORDER
    assert (_lib.EVK_CORNER_WINDOW_COUNT, _lib.EVK_CORNER_WINDOW_TIME) == (0, 1)
    header = _header.TEXT
    for name, value in (("EVK_CORNER_BORDER", 4), ("EVK_CORNER_WINDOW_COUNT", 0), ("EVK_CORNER_WINDOW_TIME", 1)):
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (name, value), header, re.M), name


def test_public_surface():
    import event_utils_amd as E
    import event_utils_amd.lib.features.corners as alias
    from event_utils_amd import features
    from event_utils_amd.features import corners
    assert alias is corners
    for name in ("fast_corners", "harris_scores", "harris_corners", "corner_events"):
        assert getattr(E, name) is getattr(corners, name) is getattr(features, name)
    assert "features.corners" in E.__doc__


def test_arguments_are_refused_before_the_device_is_touched():
    from event_utils_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every call below is refused first
    einval, f32 = -1, _lib.EVK_SELECT_F32

    def fast(kind=f32, t=fake, n=8, h=16, w=16, classes=2, select=None, rows=0, scratch=fake, out=fake):
        return L.evk_corner_fast(kind, t, n, h, w, classes, select, rows, scratch, out, None)

    def harris(kind=f32, t=fake, n=8, h=16, w=16, classes=2, window=0, n_last=5, dt=1.0, k=0.04, select=None, rows=0,
               scratch=fake, out=fake):
        return L.evk_corner_harris(kind, t, n, h, w, classes, window, n_last, dt, k, select, rows, scratch, out, None)
    for fn in (fast, harris):
        assert fn(kind=-1) == einval and fn(kind=5) == einval
        assert fn(n=-1) == einval and fn(n=1 << 31) == einval and fn(h=0) == einval and fn(w=-3) == einval
        assert fn(h=1 << 16, w=1 << 16) == einval      # more keys than a grouping holds
        assert fn(classes=0) == einval and fn(classes=3) == einval
        assert fn(select=fake, rows=-1) == einval and fn(rows=-1) == einval
        assert fn(t=None) == einval and fn(scratch=None) == einval and fn(out=None) == einval
        assert fn(select=fake, rows=4, out=None) == einval
        assert fn(n=0, t=None, select=fake, rows=3) == einval      # a selection from no events
        assert fn(scratch=ctypes.c_void_p(4100)) not in (0, einval)      # not aligned
        # nothing to do: no launch
        assert fn(n=0, t=None, out=None) == 0 and fn(select=fake, rows=0, out=None) == 0
    assert harris(window=2) == einval and harris(window=-1) == einval
    assert harris(n_last=0) == einval and harris(n_last=-7) == einval and harris(window=1, n_last=0) == einval
    assert harris(dt=-1.0) == einval and harris(dt=float("nan")) == einval and harris(window=1, dt=-0.5) == einval
    assert harris(k=float("nan")) == einval
    assert harris(n=0, t=None, out=None, window=1, dt=0.0, k=-1.0) == 0


def test_python_argument_errors_come_before_any_device_work():
    """every call below is refused on its arguments alone: none of them reaches the point where a missing GPU would matter"""
    import event_utils_amd as E
    x, y, t, p = np.array([5, 6]), np.array([5, 6]), np.array([1.0, 2.0]), np.array([1, -1])
    for fn in (E.fast_corners, E.harris_scores, E.harris_corners):
        kw = {} if fn is E.fast_corners else dict(n_last=5)
        for polarity in ("split", "both", None):
            with pytest.raises(ValueError):
                fn(x, y, t, p, polarity=polarity, **kw)
    for fn in (E.harris_scores, E.harris_corners):
        with pytest.raises(TypeError):
            fn(x, y, t, p)
        with pytest.raises(TypeError):
            fn(x, y, t, p, n_last=5, dt=1.0)
        for bad in (0, -3, 2.5, True):
            with pytest.raises(ValueError):
                fn(x, y, t, p, n_last=bad)
        for bad in (-1.0, float("nan")):
            with pytest.raises(ValueError):
                fn(x, y, t, p, dt=bad)
        with pytest.raises(ValueError):
            fn(x, y, t, p, n_last=5, k=float("nan"))
    with pytest.raises(ValueError):
        E.harris_corners(x, y, t, p, n_last=5, threshold=float("nan"))
    with pytest.raises(ValueError):
        E.corner_events(x, y, t, p, detector="arc")
    with pytest.raises(TypeError):
        E.corner_events(x, y, t, p, select=[0])
    with pytest.raises(TypeError):
        E.corner_events(x, y, t, p, detector="fast", n_last=5)
    with pytest.raises(TypeError):
        E.corner_events(x, y, t, p, detector="harris")
    with pytest.raises(ValueError):
        E.corner_events(x, y, t, p, detector="harris", n_last=0)
    with pytest.raises(ValueError):
        E.corner_events(x, y, t, p, polarity="split")
