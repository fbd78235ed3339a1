"""CPU (no GPU): the two host restatements of the event-denoising definitions (tests/_denoise_np.py) agree with each other and
with a hand-worked stream, and have the properties the definitions imply.  seq_* is the definition (a sequential loop over a
per-pixel timestamp map); fast_* is what the GPU tests use on larger streams."""
import numpy as np
import pytest

import _denoise_np as N


def random_stream(rng, n, H, W, sorted_times=True, ties=True):
    x = rng.integers(0, W, n)
    y = rng.integers(0, H, n)
    t = rng.integers(0, max(2, n // 2 if ties else 1 << 40), n).astype(np.float64)      # integer ticks: ties occur
    if sorted_times:
        t = np.sort(t)
    p = rng.integers(0, 2, n) * 2 - 1
    return x, y, t, p


def configurations():
    """60 seeded configurations: radius, flags, dt (0, small, large), ties, unsorted times, sensors down to 1 x 1."""
    sensors = [(1, 1), (1, 7), (6, 1), (2, 2), (5, 8), (12, 9)]
    out = []
    for seed in range(60):
        rng = np.random.default_rng(9000 + seed)
        H, W = sensors[seed % len(sensors)]
        out.append(dict(seed=seed, H=H, W=W, n=int(rng.integers(0, 400)), radius=1 + seed % 3, include_self=bool(seed & 1),
                        polarity=bool(seed & 2), sorted_times=seed % 5 != 0, ties=seed % 4 != 3,
                        dt=[0.0, 3.0, 40.0, 1e30][seed % 4], refractory=[0.0, 1.0, 5.0, 1e30][(seed // 2) % 4]))
    return out


@pytest.mark.parametrize("cfg", configurations(), ids=lambda c: "seed%d" % c["seed"])
def test_fast_equals_seq(cfg):
    rng = np.random.default_rng(cfg["seed"])
    H, W = cfg["H"], cfg["W"]
    x, y, t, p = random_stream(rng, cfg["n"], H, W, cfg["sorted_times"], cfg["ties"])
    kw = dict(radius=cfg["radius"], include_self=cfg["include_self"], same_polarity=cfg["polarity"])
    s = N.seq_support(x, y, t, p, cfg["dt"], (H, W), **kw)
    f = N.fast_support(x, y, t, p, cfg["dt"], (H, W), **kw)
    assert s.dtype == f.dtype == np.uint8 and np.array_equal(s, f)
    most = (2 * cfg["radius"] + 1) ** 2 - (0 if cfg["include_self"] else 1)
    assert s.max(initial=0) <= most
    for k in (1, 2, most):
        assert np.array_equal(N.fast_support_keep(f, k), s >= k)
    ks = N.seq_refractory(x, y, t, p, cfg["refractory"], (H, W), per_polarity=cfg["polarity"])
    kf = N.fast_refractory(x, y, t, p, cfg["refractory"], (H, W), per_polarity=cfg["polarity"])
    assert ks.dtype == kf.dtype == np.bool_ and np.array_equal(ks, kf)


def test_fast_refractory_long_runs_take_the_scalar_walk():
    rng = np.random.default_rng(5)
    x, y, t, p = random_stream(rng, 3000, 3, 3)
    x[rng.random(3000) < 0.5] = 1
    for r in (0.0, 2.0, 50.0):
        assert np.array_equal(N.seq_refractory(x, y, t, p, r, (3, 3)), N.fast_refractory(x, y, t, p, r, (3, 3)))


# A 3 x 4 sensor (H = 3, W = 4); events in stream order (the fifth one is OUT of time order):
#   i  (x, y)  t   p
#   0  (1, 1)  10  +    nothing before it                                            support 0
#   1  (2, 1)  12  -    (1,1) at 10: 12 - 10 = 2 <= 3                                support 1
#   2  (1, 1)  13  +    (2,1) at 12: 1 <= 3; own pixel excluded                      support 1
#   3  (0, 0)  20  +    (1,1) last fired at 13: 7 > 3                                support 0
#   4  (1, 0)   5  -    (0,0) at 20: -15 <= 3, (1,1) at 13: -8, (2,1) at 12: -7      support 3 (negative differences count)
#   5  (3, 2)  21  +    window clipped to x 2..3, y 1..2: (2,1) at 12: 9 > 3         support 0
#   6  (1, 1)  16  -    (0,0) at 20: -4, (1,0) at 5: 11 > 3, (2,1) at 12: 4 > 3      support 1
#   7  (2, 1)  16  -    (1,1) at 16: 0 <= 3, (3,2) at 21: -5, (1,0) at 5: 11 > 3     support 2
HAND = dict(x=[1, 2, 1, 0, 1, 3, 1, 2], y=[1, 1, 1, 0, 0, 2, 1, 1], t=[10, 12, 13, 20, 5, 21, 16, 16], p=[1, -1, 1, 1, -1, 1, -1, -1])


def test_hand_worked_stream():
    x, y, t, p = (np.array(HAND[k]) for k in "xytp")
    size = (3, 4)
    for fn in (N.seq_support, N.fast_support):
        assert fn(x, y, t, p, 3.0, size).tolist() == [0, 1, 1, 0, 3, 0, 1, 2]
        # with the own pixel: event 2 sees (1,1) at 10 (3 <= 3), event 6 sees (1,1) at 13 (3 <= 3), event 7 sees (2,1) at 12 (4 > 3)
        assert fn(x, y, t, p, 3.0, size, include_self=True).tolist() == [0, 1, 2, 0, 3, 0, 2, 2]
        # same polarity only: 1 (-) has no earlier -; 2 (+) sees no + neighbour; 4 (-): (2,1)- at 12 only; 6 (-): (1,0)- at 5: 11 > 3,
        # (2,1)- at 12: 4 > 3; 7 (-): (1,1)- at 16: 0, (1,0)- at 5: no, (3,2) is +
        assert fn(x, y, t, p, 3.0, size, same_polarity=True).tolist() == [0, 0, 0, 0, 1, 0, 0, 1]
        # dt = 0 keeps exact ties and negative differences only
        assert fn(x, y, t, p, 0.0, size).tolist() == [0, 0, 0, 0, 3, 0, 1, 2]
    assert N.fast_support_keep(N.seq_support(x, y, t, p, 3.0, size), 1).tolist() == [False, True, True, False, True, False, True, True]
    assert N.fast_support_keep(N.seq_support(x, y, t, p, 3.0, size), 2).tolist() == [False, False, False, False, True, False, False, True]
    for fn in (N.seq_refractory, N.fast_refractory):
        # pixel (1,1): 10 kept, 13 - 10 = 3 < 4 dropped, 16 - 10 = 6 kept; pixel (2,1): 12 kept, 16 - 12 = 4 kept; the others are first
        assert fn(x, y, t, p, 4.0, size).tolist() == [True, True, False, True, True, True, True, True]
        # per polarity: (1,1)+ 10 kept, 13 dropped; (1,1)- 16 is the first of its class; (2,1)- 12 kept, 16 kept
        assert fn(x, y, t, p, 4.0, size, per_polarity=True).tolist() == [True, True, False, True, True, True, True, True]
        # a longer period: (1,1) 16 - 10 = 6 < 7 dropped without classes, kept as the first "-" with them; (2,1) 16 - 12 = 4 dropped
        assert fn(x, y, t, p, 7.0, size).tolist() == [True, True, False, True, True, True, False, False]
        assert fn(x, y, t, p, 7.0, size, per_polarity=True).tolist() == [True, True, False, True, True, True, True, False]


def test_support_is_monotone_in_dt_and_radius():
    rng = np.random.default_rng(11)
    x, y, t, p = random_stream(rng, 600, 9, 11, sorted_times=False)
    prev = None
    for dt in (0.0, 1.0, 5.0, 50.0, 1e9):
        s = N.seq_support(x, y, t, p, dt, (9, 11), radius=2).astype(int)
        assert prev is None or (s >= prev).all()
        prev = s
    prev = None
    for r in (1, 2, 3):
        s = N.seq_support(x, y, t, p, 6.0, (9, 11), radius=r, same_polarity=True).astype(int)
        assert prev is None or (s >= prev).all()
        prev = s


def test_include_self_adds_exactly_the_own_pixel_term():
    rng = np.random.default_rng(12)
    H, W = 5, 6
    x, y, t, p = random_stream(rng, 500, H, W, sorted_times=False)
    dt = 8.0
    own = np.zeros(len(x), dtype=int)
    last = {}
    for i in range(len(x)):
        q = (x[i], y[i])
        if q in last and t[i] - last[q] <= dt:
            own[i] = 1
        last[q] = t[i]
    without = N.seq_support(x, y, t, p, dt, (H, W), radius=2).astype(int)
    with_self = N.seq_support(x, y, t, p, dt, (H, W), radius=2, include_self=True).astype(int)
    assert own.any() and np.array_equal(with_self - without, own)


def test_zero_refractory_keeps_every_event_of_a_sorted_stream():
    rng = np.random.default_rng(13)
    x, y, t, p = random_stream(rng, 800, 4, 4)
    for per_polarity in (False, True):
        assert N.seq_refractory(x, y, t, p, 0.0, (4, 4), per_polarity).all()
        assert N.fast_refractory(x, y, t, p, 0.0, (4, 4), per_polarity).all()
    shuffled = rng.permutation(t)
    assert not N.seq_refractory(x, y, shuffled, p, 0.0, (4, 4)).all()      # unsorted: a step back in time is dropped
