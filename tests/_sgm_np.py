"""The definition of semi-global matching (include/evk.h, "Semi-global matching") restated literally in numpy: a
plain loop over the pixels in path order, vectorised over d only, every L_r kept apart and summed at the end.  The winner of a volume
is _stereo_np.match(volume=...) on the cells with a right pixel.  Nothing here is shared with the product; the tests compare the
device with it bit for bit.  Also the seeded structured pair: continuous contours on two planes and a slanted surface."""
import numpy as np

import _stereo_np as N

MAX_COST = 1 << 22
MAX_PENALTY = 1 << 20
DIRECTIONS = ((1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1))
BIG = np.int64(1) << 40                                    # an absent cell: more than any L + P2


def directions(paths):
    """4, 8 or a tuple of directions -> a tuple of directions in the order of DIRECTIONS"""
    if paths in (4, 8):
        return DIRECTIONS[:paths]
    return tuple(r for r in DIRECTIONS if r in tuple(tuple(p) for p in paths))


def path_costs(volume, p1, p2, r):
    """L_r, (K, D, H, W) int64, 0 where the cell is absent"""
    vol = np.asarray(volume, dtype=np.int64)
    K, D, H, W = vol.shape
    dx, dy = r
    present = vol >= 0
    C = np.minimum(vol, MAX_COST)
    L = np.zeros(vol.shape, dtype=np.int64)
    ys = range(H) if dy >= 0 else range(H - 1, -1, -1)     # q = p - r comes before p
    xs = range(W) if dx >= 0 else range(W - 1, -1, -1)
    pad = np.array([BIG])
    for k in range(K):
        some = present[k].any(axis=0)
        for y in ys:
            for x in xs:
                if not some[y, x]:
                    continue
                pp, c = present[k, :, y, x], C[k, :, y, x]
                qx, qy = x - dx, y - dy
                if not (0 <= qx < W and 0 <= qy < H) or not some[qy, qx]:
                    l = c
                else:
                    lq = np.where(present[k, :, qy, qx], L[k, :, qy, qx], BIG)
                    m = lq.min()
                    step = np.minimum(np.concatenate((pad, lq[:-1])), np.concatenate((lq[1:], pad))) + p1
                    l = c + np.minimum(np.minimum(lq, step), m + p2) - m
                assert (l[pp] >= c[pp]).all() and (l[pp] <= c[pp] + p2).all()
                L[k, :, y, x] = np.where(pp, l, 0)
    return L


def aggregate(volume, p1, p2, paths=8):
    """S, (K, D, H, W) int32: the sum of L_r over the directions where the cell is present, -1 elsewhere"""
    assert 0 <= p1 <= p2 <= MAX_PENALTY
    vol = np.asarray(volume, dtype=np.int64)
    total = np.zeros(vol.shape, dtype=np.int64)
    for r in directions(paths):
        total += path_costs(vol, p1, p2, r)
    return np.where(vol >= 0, total, -1).astype(np.int32)


def with_right_pixel(volume, d_min):
    """the volume with -1 where x - d < 0: such a cell has no right pixel and is not admissible for the winner"""
    vol = np.array(volume, dtype=np.int64)
    K, D, H, W = vol.shape
    for i in range(D):
        vol[:, i, :, :min(d_min + i, W)] = -1
    return vol


def match_volume(volume, activity, d_min=0, min_activity=128, uniqueness=10, max_cost=None, lr_tolerance=1, subpixel=True):
    """-> disparity, index, cost, mask, candidates as _stereo_np.match gives them, the cost limit an integer"""
    vol = with_right_pixel(volume, d_min)
    A = np.asarray(activity).max(axis=1, keepdims=True)    # one channel and a window of one pixel: the limit is max_cost itself
    return N.match(A, A, d_min, vol.shape[1], 0, min_activity, uniqueness, None if max_cost is None else int(max_cost), lr_tolerance,
                   subpixel, volume=vol)


# ---- the seeded structured pair --------------------------------------------------------------------------------------------------

PAIR_SIZE = (40, 96)                                       # (H, W)
PAIR_D, PAIR_R, PAIR_ACTIVITY = 16, 1, 128
PAIR_P1, PAIR_P2 = 144, 1152
PAIR_NOISE = 0.35
PAIR_MARGIN = 12                                           # candidates left of it are not counted: not every d is admissible there


def pair_truth():
    """(H, W) true disparities: the plane d = 4 on rows 0 .. 12, the plane d = 9 on rows 13 .. 25, and below them a surface
    slanted in x from d = 3 to d = 11"""
    H, W = PAIR_SIZE
    d = np.empty((H, W), dtype=np.int64)
    d[:13], d[13:26] = 4, 9
    d[26:] = 3 + (np.arange(W) * 9) // W
    return d


def structured_pair(seed, contours=28, length=36):
    """Continuous contours (random walks of `length` pixels that turn slowly, one surface value 140 .. 255 drifting along each)
    seen by a rectified pair: QR[y, x - d(y, x)] = QL[y, x], then a share PAIR_NOISE of all right pixels is redrawn (a random
    value 100 .. 255 at the left surface's density, else 0).  -> QL, QR (1, 1, H, W) uint8 and the true disparities"""
    rng = np.random.default_rng(seed)
    H, W = PAIR_SIZE
    truth = pair_truth()
    QL = np.zeros((H, W), dtype=np.uint8)
    for _ in range(contours):
        x, y = rng.uniform(0, W), rng.uniform(0, H)
        heading, value = rng.uniform(0, 2 * np.pi), rng.uniform(140, 255)
        for _ in range(length):
            xi, yi = int(x), int(y)
            if 0 <= xi < W and 0 <= yi < H:
                QL[yi, xi] = int(value)
            heading += rng.normal(0.0, 0.25)
            value = min(255.0, max(140.0, value + rng.normal(0.0, 6.0)))
            x, y = x + np.cos(heading), y + np.sin(heading)
    QR = np.zeros_like(QL)
    yy, xx = np.nonzero(QL)
    keep = xx - truth[yy, xx] >= 0
    QR[yy[keep], (xx - truth[yy, xx])[keep]] = QL[yy[keep], xx[keep]]
    density = float((QL > 0).mean())
    redraw = rng.random((H, W)) < PAIR_NOISE
    fresh = (rng.integers(100, 256, (H, W)) * (rng.random((H, W)) < density)).astype(np.uint8)
    QR[redraw] = fresh[redraw]
    return QL[None, None], QR[None, None], truth


def pair_fraction(index_or_volume, QL, truth, winners=None):
    """(candidates counted, the fraction of them whose d* is within 1 of the truth) of a volume's plain winners (no tests), or of
    the `index` of a match, where -1 counts as wrong"""
    H, W = PAIR_SIZE
    counted = (QL[0, 0] >= PAIR_ACTIVITY) & (np.arange(W)[None, :] >= PAIR_MARGIN)
    if winners is None:
        vol = np.asarray(index_or_volume, dtype=np.int64)[0]
        winners = np.where(vol >= 0, vol, BIG).argmin(axis=0)
    good = np.abs(winners - truth) <= 1
    return int(counted.sum()), float((good & counted).sum()) / max(int(counted.sum()), 1)
