"""GPU: seeded random cases of semi-global matching against its restatement (tests/_sgm_np.py), bit for bit: the shape, D, d_min, K,
the holes, the penalties, the subset of directions and the switches of the winner are all drawn."""
import numpy as np
import pytest
import torch

import _sgm_np as G
from test_gpu_sgm import check_aggregate, check_match, random_volume

pytestmark = pytest.mark.gpu

D_CHOICES = (1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 100, 128, 129, 192, 193, 255, 256)


def draw(seed):
    rng = np.random.default_rng(1000 + seed)
    H, W = (int(v) for v in rng.integers(1, 40, 2))
    if seed % 5 == 0:
        W = int(rng.integers(64, 150))                      # more than one tile of pixels a row
    D = int(D_CHOICES[rng.integers(0, len(D_CHOICES))])
    K = int(rng.integers(1, 4))
    p2 = int(rng.choice([0, 1, 30, 500, 70000, G.MAX_PENALTY]))
    p1 = int(rng.integers(0, p2 + 1)) if rng.random() < 0.8 else p2
    dirs = tuple(r for r in G.DIRECTIONS if rng.random() < 0.5) or (G.DIRECTIONS[int(rng.integers(0, 8))],)
    paths = [4, 8, dirs][int(rng.integers(0, 3))]
    vol = random_volume(2000 + seed, K, D, H, W, holes=float(rng.choice([0.0, 0.1, 0.6])), pixels=float(rng.choice([0.0, 0.1, 0.5])),
                        high=int(rng.choice([4, 300, G.MAX_COST + 100])), big=float(rng.choice([0.0, 0.05])))
    A = rng.integers(0, 256, (K, int(rng.integers(1, 3)), H, W)).astype(np.uint8)
    kw = dict(min_activity=int(rng.choice([1, 64, 128, 255])), uniqueness=int(rng.choice([0, 10, 40, 99])),
              max_cost=None if rng.random() < 0.5 else int(rng.integers(0, 8 * 400)),
              lr_tolerance=None if rng.random() < 0.3 else int(rng.integers(0, 3)), subpixel=bool(rng.random() < 0.7))
    return vol, A, int(rng.choice([0, 0, 1, 7])), p1, p2, paths, kw


@pytest.mark.parametrize("seed", range(30))
def test_a_random_case(seed):
    import event_utils_amd as E
    vol, A, d_min, p1, p2, paths, kw = draw(seed)
    S = check_aggregate(E, vol, p1, p2, paths)
    check_match(E, vol, A, d_min, **kw)
    check_match(E, S, A, d_min, **kw)
    out = E.sgm_aggregate(torch.from_numpy(vol).cuda(), p1, p2, paths)
    assert torch.equal(out.cpu(), torch.from_numpy(S))     # the same bits again
