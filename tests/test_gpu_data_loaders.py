"""GPU: event_utils_amd.data_loaders on the device -- the voxel grids of every window method in both channel modes against the
oracle (widen_native_events + events_to_voxel_torch per window), __getitems__ against __getitem__, a DataLoader end to end,
the window edge cases (overlap, empty, one event, equal stamps, out of range, a long window), RobustNorm bit for bit against
the reference's torch code on the CPU, and the packed events of return_events."""
import os

import numpy as np
import pytest
import torch

from oracle import reference_np as R

pytestmark = pytest.mark.gpu


def close(a, b, rel=1e-5):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), "NaN positions differ: %d vs %d" % (na.sum(), nb.sum())
    fin = ~na
    scale = max(np.abs(b[fin]).max() if fin.any() else 0.0, 1e-30)
    err = np.abs(a[fin] - b[fin]).max() if fin.any() else 0.0
    assert err <= rel * scale, (err, scale)


def oracle_window(xs, ys, ts, ps, a, b, B, size, split, polarity):
    """base_dataset.py: get_events + preprocess_events + get_voxel_grid, on the widened columns (widen_native_events)."""
    if b <= a:
        x = y = t = p = np.zeros(1, np.float32)
    else:
        x, y, t, p = R.widen_native_events(xs[a:b], None if ys is None else ys[a:b], ts[a:b], ps[a:b], polarity=polarity)
    if not split:
        return R.events_to_voxel_torch(x, y, t, p, B, sensor_size=size, accum="f64")
    pos = np.where(p > 0, 1, 0).astype(np.float32)
    neg = np.where(p <= 0, 1, 0).astype(np.float32)
    return np.concatenate([R.events_to_voxel_torch(x, y, t, pos, B, sensor_size=size, accum="f64"),
                           R.events_to_voxel_torch(x, y, t, neg, B, sensor_size=size, accum="f64")])


def write_memmap(root, n, H, W, seed=0, frames=0):
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    t = 1.5e9 + np.sort(rng.uniform(0.0, 1.0, n))          # epoch-scale float64 stamps: the window offset must be float64
    t[200:260] = t[200]
    xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.int16)
    p = rng.integers(0, 2, n).astype(np.uint8)
    for name, a in (("t", t), ("xy", xy), ("p", p)):
        np.save(os.path.join(root, name + ".npy"), a)
    if frames:
        np.save(os.path.join(root, "images.npy"), rng.integers(0, 255, (frames, H, W, 1)).astype(np.uint8))
        np.save(os.path.join(root, "timestamps.npy"), np.linspace(t[0] + 0.05, t[-1] - 0.01, frames))
    return str(root), xy, t, p


def write_npy(path, n, H, W, seed=1):
    rng = np.random.default_rng(seed)
    data = np.stack([rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n),
                     np.sort(rng.uniform(0, 2e6, n)).round()], 1).astype(np.float64)
    np.save(path, data)
    return str(path), data


METHODS = [
    {'method': 'k_events', 'k': 1500, 'sliding_window_w': 0},
    {'method': 'k_events', 'k': 1500, 'sliding_window_w': 400},
    {'method': 't_seconds', 't': 0.05, 'sliding_window_t': 0.02},
    {'method': 'fixed_frames', 'num_frames': 7},
    {'method': 'between_frames'},
]
NO_FRAMES = dict(return_frame=False, return_flow=False)


@pytest.mark.parametrize("split", [False, True], ids=["combined", "split"])
@pytest.mark.parametrize("method", METHODS, ids=lambda m: m['method'] + str(m.get('sliding_window_w', '')))
@pytest.mark.parametrize("fmt,H,W", [("memmap", 60, 80), ("memmap", 45, 61), ("npy", 60, 80)])
def test_every_method_and_channel_mode_equals_the_oracle(tmp_path, fmt, H, W, method, split):
    from event_utils_amd.data_loaders import MemMapDataset, NpyDataset
    n = 20_000
    if fmt == "memmap":
        root, xy, t, p = write_memmap(tmp_path / "mm", n, H, W, frames=9 if method['method'] == 'between_frames' else 0)
        cols, pol = (xy, None, t, p), "pm1"
        ds = MemMapDataset(root, voxel_method=dict(method), combined_voxel_channels=not split, **NO_FRAMES)
    else:
        if method['method'] == 'between_frames':
            pytest.skip("the npy format has no frames")
        path, data = write_npy(tmp_path / "ev.npy", n, H, W)
        cols, pol = (data[:, 0], data[:, 1], data[:, 3] * 1e-6, data[:, 2] * 2 - 1), "literal"
        ds = NpyDataset(path, voxel_method=dict(method), combined_voxel_channels=not split, **NO_FRAMES)
    B = ds.num_bins
    idx = [i for i in range(len(ds)) if ds.event_indices[i][1] <= n]
    items = ds.__getitems__(idx)
    assert len(items) == len(idx) >= 3
    for i, item in zip(idx, items):
        vox = item['voxel']
        assert vox.is_cuda and vox.dtype == torch.float32 and vox.shape == ((2 * B if split else B), H, W)
        a, b = ds.get_event_indices(i)
        close(vox.cpu().numpy(), oracle_window(*cols, a, b, B, (H, W), split, pol))
        assert (item['idx0'], item['idx1']) == (a, b)
        if b > a:
            assert item['ts_idx0'] == cols[2][a] and item['timestamp'] == cols[2][b - 1]


@pytest.mark.parametrize("transforms", [{}, {'RobustNorm': {}}, {'CenterCrop': {'size': (40, 50)}, 'RobustNorm': {'top_perc': 90}}],
                         ids=["plain", "robustnorm", "crop+robustnorm"])
def test_batched_equals_per_item_and_a_dataloader_runs(tmp_path, transforms):
    from event_utils_amd.data_loaders import MemMapDataset
    root, xy, t, p = write_memmap(tmp_path / "mm", 30_000, 60, 80)
    ds = MemMapDataset(root, voxel_method={'method': 'k_events', 'k': 2000, 'sliding_window_w': 500}, transforms=transforms,
                       return_events=True, **NO_FRAMES)
    idx = list(range(0, 12))
    batch = ds.__getitems__(idx)
    for i, item in zip(idx, batch):
        one = ds[i]
        assert set(one) == set(item)
        assert item['voxel'].shape == one['voxel'].shape
        close(item['voxel'].cpu().numpy(), one['voxel'].cpu().numpy(), rel=1e-6)
        assert torch.equal(item['events'], one['events'])
    loader = torch.utils.data.DataLoader(ds, batch_size=8, collate_fn=ds.collate_fn)
    seen = 0
    for b in loader:
        vox = b['voxel']
        assert vox.is_cuda and vox.shape[0] == len(b['idx0'])
        for k in range(vox.shape[0]):
            a, e = int(b['idx0'][k]), int(b['idx1'][k])
            if e > len(t):
                continue
            if not transforms:
                close(vox[k].cpu().numpy(), oracle_window(xy, None, t, p, a, e, 5, (60, 80), True, "pm1"))
        assert b['events'].is_cuda and b['events'].shape == (int(b['events_batch_indices'][-1]), 4)
        seen += vox.shape[0]
        if seen >= 16:
            break
    assert seen >= 16


def test_window_edge_cases(tmp_path):
    from event_utils_amd.data_loaders import _kernels as K
    H, W, B = 30, 40, 5
    rng = np.random.default_rng(5)
    n = 3000
    t = 1.6e9 + np.sort(rng.uniform(0, 1, n))
    t[100:140] = t[100]
    xy = np.stack([rng.integers(-W, W, n), rng.integers(-H, H, n)], 1).astype(np.int16)   # negative indices wrap once
    p = rng.integers(0, 2, n).astype(np.uint8)
    s = K.ResidentStream(xy=xy, ts=t, ps=p)
    windows = [(0, 700), (300, 1000), (500, 500), (7, 8), (100, 140), (2990, 3000), (0, n)]
    for split in (False, True):
        out = s.voxel_windows(windows, B, (H, W), split).cpu().numpy()
        for k, (a, b) in enumerate(windows):
            close(out[k], oracle_window(xy, None, t, p, a, b, B, (H, W), split, "pm1"))
        assert np.isnan(out[2]).any() and np.isnan(out[3]).any() and np.isnan(out[4]).any()   # empty, one event, equal stamps
    bad = xy.copy()
    bad[1234, 0] = W                                               # x == W is outside the grid: IndexError, as index_put_
    sb = K.ResidentStream(xy=bad, ts=t, ps=p)
    with pytest.raises(IndexError):
        sb.voxel_windows([(1000, 1500)], B, (H, W), True)
    sb.voxel_windows([(0, 1000)], B, (H, W), True)                 # (a window without it is fine)
    torch.cuda.synchronize()


def test_a_window_above_the_long_window_threshold(tmp_path):
    """One long window alone takes the one-pass path; in a batch it goes through the window kernel with the others."""
    from event_utils_amd.data_loaders import _kernels as K
    H, W, B = 90, 120, 5
    n = K.LONG_WINDOW_EVENTS + 50_000
    rng = np.random.default_rng(6)
    t = 1.6e9 + np.sort(rng.uniform(0, 1, n))
    xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.int16)
    p = rng.integers(0, 2, n).astype(np.uint8)
    s = K.ResidentStream(xy=xy, ts=t, ps=p)
    for split in (False, True):
        want = oracle_window(xy, None, t, p, 10, n, B, (H, W), split, "pm1")
        close(s.voxel_windows([(10, n)], B, (H, W), split)[0].cpu().numpy(), want)
        both = s.voxel_windows([(10, n), (0, 1000)], B, (H, W), split).cpu().numpy()
        close(both[0], want)
        close(both[1], oracle_window(xy, None, t, p, 0, 1000, B, (H, W), split, "pm1"))
    bad = xy.copy()
    bad[n // 2, 1] = H                                              # out of range inside the long window: IndexError on both paths
    sb = K.ResidentStream(xy=bad, ts=t, ps=p)
    with pytest.raises(IndexError):
        sb.voxel_windows([(0, n)], B, (H, W), True)
    with pytest.raises(IndexError):
        sb.voxel_windows([(0, n), (0, 10)], B, (H, W), True)


def test_empty_window_of_a_dataset_gives_nan_cells(tmp_path):
    from event_utils_amd.data_loaders import MemMapDataset
    H, W, n = 30, 40, 4000
    rng = np.random.default_rng(7)
    t = np.concatenate([np.sort(rng.uniform(0, 0.2, n // 2)), np.sort(rng.uniform(0.6, 1.0, n - n // 2))])
    os.makedirs(tmp_path / "mm")
    np.save(tmp_path / "mm" / "t.npy", t)
    np.save(tmp_path / "mm" / "xy.npy", np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.int16))
    np.save(tmp_path / "mm" / "p.npy", rng.integers(0, 2, n).astype(np.uint8))
    ds = MemMapDataset(str(tmp_path / "mm"), voxel_method={'method': 't_seconds', 't': 0.1, 'sliding_window_t': 0.0},
                       sensor_resolution=(H, W), return_events=True, **NO_FRAMES)
    empty = [i for i in range(len(ds)) if ds.event_indices[i][0] == ds.event_indices[i][1]]
    assert empty
    item = ds[empty[0]]
    v = item['voxel'].cpu().numpy()
    assert np.isnan(v[:, 0, 0]).all() and not np.isnan(v[:, 1:, :]).any() and not np.isnan(v[:, 0, 1:]).any()
    assert item['events'].shape == (1, 4) and not item['events'].any()


# ---- RobustNorm -----------------------------------------------------------------------------------------------------------

def reference_robust_norm(x, low_perc=0, top_perc=95):
    """data_augmentation.py:113-146 on a CPU tensor (the reference's own code path)."""
    def percentile(t, q):
        k = 1 + round(.01 * float(q) * (t.numel() - 1))
        return t.reshape(-1).kthvalue(k).values.item()
    t_max = percentile(x, top_perc)
    t_min = percentile(x, low_perc)
    if t_max == 0 and t_min == 0:
        return x, (t_min, t_max)
    normed = torch.clamp(x, min=t_min, max=t_max)
    normed = (normed - torch.min(normed)) / (torch.max(normed) + 1e-6)
    return normed, (t_min, t_max)


def same(a, b):
    a, b = a.cpu(), b.cpu()
    assert a.shape == b.shape
    assert bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all()), (a, b)


def robust_inputs():
    g = torch.Generator().manual_seed(0)
    out = {"random": torch.randn(10, 18, 24, generator=g)}
    sparse = torch.zeros(10, 18, 24)
    m = torch.rand(sparse.shape, generator=g) < 0.03
    sparse[m] = torch.randn(int(m.sum()), generator=g)
    out["sparse"] = sparse
    out["zeros"] = torch.zeros(5, 7, 9)
    nanx = torch.randn(4, 9, 11, generator=g)
    nanx[1, 2, 3] = float('nan')
    out["nan"] = nanx
    out["ties"] = torch.randint(-3, 4, (6, 10, 10), generator=g).float() * 0.5
    out["neg_zero"] = torch.where(torch.rand(3, 8, 8, generator=g) < 0.5, -0.0, 0.0) + (torch.rand(3, 8, 8, generator=g) < 0.1) * 2.0
    vox = torch.zeros(10, 180, 240)                                 # a voxel grid's shape and sparsity: ~95 % zeros
    m = torch.rand(vox.shape, generator=g) < 0.05
    vox[m] = torch.randn(int(m.sum()), generator=g)
    out["voxel_like"] = vox
    for m_ in (1, 2, 3, 4, 6, 8, 21, 101):
        out["m%d" % m_] = torch.randn(1, 1, m_, generator=g)
    return out


@pytest.mark.parametrize("low,top", [(0, 95), (5, 50), (50, 50), (12.5, 100)])
def test_robust_norm_bit_exact_against_the_reference(low, top):
    from event_utils_amd.data_loaders import RobustNorm
    from event_utils_amd.data_loaders import _kernels as K
    for name, x in robust_inputs().items():
        ref, (t_min, t_max) = reference_robust_norm(x, low, top)
        got = RobustNorm(low, top)(x)
        assert not got.is_cuda, name                                # a CPU tensor comes back to the CPU
        same(got, ref)
        out, perc = K.robust_norm(x.cuda(), low, top)
        same(out, ref)
        lo, hi = perc[0].tolist()
        assert (lo == t_min or (np.isnan(lo) and np.isnan(t_min))) and (hi == t_max or (np.isnan(hi) and np.isnan(t_max))), name
        assert RobustNorm.percentile(x, top) == t_max or np.isnan(t_max)


def test_robust_norm_of_a_cropped_batch_equals_the_reference_per_item():
    from event_utils_amd.data_loaders import CenterCrop, Compose, RobustNorm
    g = torch.Generator().manual_seed(1)
    x = torch.randn(7, 10, 45, 61, generator=g)
    x[2] = 0.0                                                      # an item left unchanged
    x[4, 3, 10, 10] = float('nan')
    xd = x.cuda()
    tr = Compose([CenterCrop((30, 41)), RobustNorm(3, 97)])
    got = tr.batch(xd)
    for k in range(x.shape[0]):
        crop = CenterCrop((30, 41))(x[k])
        assert not crop.is_contiguous()
        same(got[k], reference_robust_norm(crop, 3, 97)[0])
        same(tr(xd[k]), reference_robust_norm(crop, 3, 97)[0])


def test_robust_norm_of_unaligned_items_equals_the_reference():
    """Items of 21 contiguous elements: every item but the first starts off a 16-byte boundary (the scalar load path)."""
    from event_utils_amd.data_loaders import _kernels as K
    g = torch.Generator().manual_seed(2)
    x = torch.randn(9, 1, 3, 7, generator=g)
    x[3] = 0.0
    out, perc = K.robust_norm(x.cuda(), 5, 95, batch_dims=1)
    for k in range(x.shape[0]):
        ref, (lo, hi) = reference_robust_norm(x[k], 5, 95)
        same(out[k], ref)
        assert perc[k].tolist() == [lo, hi]


def test_voxel_windows_into_an_unaligned_grid():
    """evk_voxel_windows_f32 into a grid that starts 4 bytes past a 16-byte boundary (h * wd a multiple of 4): scalar stores."""
    from event_utils_amd import _device as D
    from event_utils_amd import _lib
    from event_utils_amd.data_loaders import _kernels as K
    H, W, B, n = 20, 24, 3, 4000
    rng = np.random.default_rng(9)
    t = 1.6e9 + np.sort(rng.uniform(0, 1, n))
    xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.int16)
    p = rng.integers(0, 2, n).astype(np.uint8)
    s = K.ResidentStream(xy=xy, ts=t, ps=p)
    windows = [(0, 1500), (1000, 4000)]
    buf = torch.full((1 + len(windows) * 2 * B * H * W + 4,), -7.0, device=s.device)
    wd = torch.tensor(windows, dtype=torch.int64, device=s.device)
    oob = D.OobCounter(s.device)
    _lib.call("evk_voxel_windows_f32", *s.src_args(), D.ptr(wd), len(windows), B, H, W, 1, D.ptr(buf[1:]), oob.ptr, D.stream())
    oob.raise_if_set(IndexError, "out of range")
    got = buf[1:1 + len(windows) * 2 * B * H * W].reshape(len(windows), 2 * B, H, W).cpu().numpy()
    for k, (a, b) in enumerate(windows):
        close(got[k], oracle_window(xy, None, t, p, a, b, B, (H, W), True, "pm1"))
    assert buf[0].item() == -7.0 and bool((buf[1 + got.size:] == -7.0).all())


def test_packed_events_equal_the_float64_stack():
    from event_utils_amd.data_loaders import _kernels as K
    rng = np.random.default_rng(8)
    n = 5000
    t = 1.6e9 + np.sort(rng.uniform(0, 1, n))
    xy = np.stack([rng.integers(0, 346, n), rng.integers(0, 260, n)], 1).astype(np.int16)
    p = rng.integers(0, 2, n).astype(np.uint8)
    windows = [(0, 700), (300, 1000), (10, 10), (4000, 5000)]
    for s in (K.ResidentStream(xy=xy, ts=t, ps=p),
              K.ResidentStream(xs=xy[:, 0].astype(np.float64), ys=xy[:, 1].astype(np.float64), ts=t, ps=p * 2.0 - 1, p_pm1=False)):
        packed, rows, lens = s.pack_events(windows)
        assert packed.is_cuda and packed.shape == (int(lens.sum()), 4)
        for (a, b), r, m in zip(windows, rows, lens):
            xs, ys, ts, ps = xy[a:b, 0].astype(np.float32), xy[a:b, 1].astype(np.float32), t[a:b], p[a:b] * 2.0 - 1.0
            want = torch.from_numpy(np.stack((xs, ys, ts - t[a], ps), axis=1)).float()    # base_dataset.py:306
            assert torch.equal(packed[r:r + m].cpu(), want)
