"""GPU (-m gpu): a short, seeded slice of random camera-tracking cases against the restatement (tests/_track_np.py), by the rules of
tests/test_gpu_track.py: the per-point values bit for bit, the count exact, every sum within n 2^-52 sum |term| of the correctly
rounded sum.  A case draws the number of points, the surface's size, the intrinsics, the pose, how far the projections spill over
the surface, the share of points that are behind the camera or not finite, the loss and the batch."""
import math

import numpy as np
import pytest
import torch

import _track_np as N

pytestmark = pytest.mark.gpu


def draw(rng):
    H, W = int(rng.integers(2, 70)), int(rng.integers(2, 90))
    m = int(rng.choice([int(rng.integers(1, 70)), int(rng.integers(200, 1100)), int(rng.integers(1100, 4200))]))
    intr = (float(rng.uniform(0.5, 2.0) * W), float(rng.uniform(0.5, 2.0) * W), float(rng.uniform(0.0, W - 1.0)), float(rng.uniform(0.0, H - 1.0)))
    xi = rng.normal(size=6) * np.array([0.1, 0.1, 0.1, 0.05, 0.05, 0.05]) * float(rng.choice([0.0, 1.0, 4.0]))
    return dict(H=H, W=W, m=m, intr=intr, xi=xi, spill=float(rng.choice([0.0, 1.0, 0.3 * W])), bad=float(rng.choice([0.0, 0.05, 0.5])),
                loss=str(rng.choice(["l2", "huber"])), delta=float(rng.choice([1.0, 40.0, 120.0, 1e6])), B=int(rng.choice([1, 2, 5])))


def run(E, case, rng):
    H, W, m, intr = case["H"], case["W"], case["m"], case["intr"]
    S = rng.uniform(0.0, 255.0, (H, W)).astype(np.float32)
    R, t = N.se3_exp(case["xi"])
    u, v = rng.uniform(-case["spill"], W - 1.0 + case["spill"], m), rng.uniform(-case["spill"], H - 1.0 + case["spill"], m)
    Z = rng.uniform(0.3, 5.0, m)
    P = (np.stack(((u - intr[2]) / intr[0] * Z, (v - intr[3]) / intr[1] * Z, Z), axis=1) - t) @ R
    bad = rng.uniform(size=m) < case["bad"]
    P[bad] *= rng.choice([-1.0, np.nan, np.inf, 0.0], size=(int(bad.sum()), 1))
    K = np.array([[intr[0], 0.0, intr[2]], [0.0, intr[1], intr[3]], [0.0, 0.0, 1.0]])
    dP, dS = torch.from_numpy(P).cuda(), torch.from_numpy(S).cuda()
    r, J, valid = E.registration_residuals(dP, dS, K, N.matrix(R, t))
    wr, wJ, wv = N.residuals(P, S, intr, R, t)
    if not np.array_equal(valid.cpu().numpy(), wv):
        return "valid: %d points differ" % int((valid.cpu().numpy() != wv).sum())
    for name, got, want in (("r", r, wr), ("J", J, wJ)):
        got = got.cpu().numpy()
        if not (np.isnan(got[~wv]).all() and np.array_equal(got[wv].view(np.uint64), want[wv].view(np.uint64))):
            return "%s differs" % name
    poses = [(R, t)] + [N.left(rng.normal(size=6) * 0.01, R, t) for _ in range(case["B"] - 1)]
    loss, delta = case["loss"], case["delta"] if case["loss"] == "huber" else None
    A, g, c, n = (x.cpu().numpy() for x in E.registration_terms(dP, dS, K, np.stack([N.matrix(*p) for p in poses]), loss, delta))
    iu = np.triu_indices(6)
    for b, pose in enumerate(poses):
        T = N.products(P, S, intr, *pose, loss, delta)
        got = np.concatenate((A[b][iu], g[b], c[b:b + 1]))
        if n[b] != len(T):
            return "pose %d: n = %d, expected %d" % (b, n[b], len(T))
        for k in range(28):
            if abs(got[k] - math.fsum(T[:, k])) > len(T) * 2.0 ** -52 * math.fsum(np.abs(T[:, k])):
                return "pose %d: sum %d = %r, expected %r" % (b, k, got[k], math.fsum(T[:, k]))
    return None


def test_random_cases_agree_with_the_restatement():
    import event_utils_amd as E
    failed, seen = [], set()
    for seed in range(40):
        rng = np.random.default_rng(940_000 + seed)
        case = draw(rng)
        err = run(E, case, rng)
        seen.add((case["loss"], case["m"] > 1024, case["B"] > 1))
        if err is not None:
            failed.append("seed %d: %r -> %s" % (seed, case, err))
    assert not failed, "\n".join(failed)
    assert len(seen) == 8                                   # both losses, one and several workgroup rows, one and several poses
