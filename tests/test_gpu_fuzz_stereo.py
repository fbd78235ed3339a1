"""GPU (-m gpu): a short, seeded slice of random event-stereo cases against the restatement (tests/_stereo_np.py), by the rules of
tests/test_gpu_stereo.py: every output bit for bit.  A case draws the shape, the disparity range, the radius, the channels, the
queries, every switch of the matcher and how sparse the surfaces are."""
import numpy as np
import pytest
import torch

import _stereo_np as N

pytestmark = pytest.mark.gpu


def draw(rng):
    H, W = int(rng.integers(1, 41)), int(rng.choice([int(rng.integers(1, 12)), int(rng.integers(60, 70)), int(rng.integers(120, 200))]))
    D = int(rng.choice([1, 2, int(rng.integers(3, 9)), int(rng.integers(9, 65)), int(rng.integers(65, 257))]))
    case = dict(H=H, W=W, D=D, d_min=int(rng.choice([0, 0, 1, int(rng.integers(2, 12))])), r=int(rng.integers(1, 8)),
                C=int(rng.integers(1, 3)), K=int(rng.integers(1, 4)), density=float(rng.choice([0.02, 0.2, 0.6, 1.0])),
                noise=float(rng.choice([0.0, 0.1, 0.5])))
    tests = dict(min_activity=int(rng.choice([1, 64, 128, 255])), uniqueness=int(rng.choice([0, 10, 50, 99])),
                 max_mean_cost=None if rng.random() < 0.5 else float(rng.choice([0.0, 8.0, 40.5, 255.0])),
                 lr_tolerance=None if rng.random() < 0.3 else int(rng.choice([0, 1, 3])), subpixel=bool(rng.random() < 0.7))
    return case, tests


def run(E, case, tests, rng):
    QL, QR = N.random_pair(rng, case["K"], case["C"], case["H"], case["W"], density=case["density"], noise=case["noise"])
    d_min, D, r = case["d_min"], case["D"], case["r"]
    want_vol = N.cost_volume(QL, QR, d_min, D, r)
    dl, dr = torch.from_numpy(QL).cuda(), torch.from_numpy(QR).cuda()
    vol = E.stereo_cost_volume(dl, dr, d_min + D - 1, radius=r, min_disparity=d_min)
    if not np.array_equal(vol.cpu().numpy(), want_vol):
        return "cost volume: %d cells differ" % int((vol.cpu().numpy() != want_vol).sum())
    res = E.stereo_match(dl, dr, d_min + D - 1, radius=r, min_disparity=d_min, **tests)
    want = N.match(QL, QR, d_min, D, r, volume=want_vol, **tests)
    for name, got, exp in (("cost", res.cost, want[2]), ("index", res.index, want[1]), ("mask", res.mask, want[3])):
        if not torch.equal(got.cpu(), torch.from_numpy(exp)):
            return "%s: %d pixels differ" % (name, int((got.cpu().numpy() != exp).sum()))
    if not np.array_equal(res.disparity.cpu().numpy(), want[0], equal_nan=True):
        return "disparity differs"
    return None


def test_random_cases_agree_with_the_restatement():
    import event_utils_amd as E
    failed, seen = [], set()
    for seed in range(40):
        rng = np.random.default_rng(930_000 + seed)
        case, tests = draw(rng)
        err = run(E, case, tests, rng)
        seen.add((case["r"], case["C"]))
        if err is not None:
            failed.append("seed %d: %r %r -> %s" % (seed, case, tests, err))
    assert not failed, "\n".join(failed)
    assert {r for r, _ in seen} == set(range(1, 8)) and {c for _, c in seen} == {1, 2}      # every window width, both channel counts
