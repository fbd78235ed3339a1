"""CPU (no GPU): the host side of event_utils_amd.data_loaders -- the window tables of the four voxel methods on small memmap /
npy fixtures against a restatement here and, when the reference checkout is importable, against the reference's own
BaseVoxelDataset index methods; CenterCrop offsets, RobustNorm's percentile ranks, collate_fn, unpack_batched_events, the
public signatures, and a register-spill check of the new kernels.  tests/test_gpu_data_loaders.py checks the device."""
import importlib
import inspect
import os
import sys
import types

import numpy as np
import pytest
import torch

from event_utils_amd.data_loaders import dataloader_util as DU
from event_utils_amd.data_loaders import _kernels as K
from event_utils_amd.data_loaders.base_dataset import BaseVoxelDataset
from event_utils_amd.data_loaders.data_augmentation import CenterCrop, Compose, RobustNorm
from event_utils_amd.data_loaders.memmap_dataset import MemMapDataset
from event_utils_amd.data_loaders.npy_dataset import NpyDataset

HOST_ONLY = dict(return_voxelgrid=False, return_events=False)     # no upload: the tables only
H, W, N = 30, 40, 5000


def write_memmap(root, n=N, frames=12, seed=0, images=True):
    rng = np.random.default_rng(seed)
    os.makedirs(root, exist_ok=True)
    t = np.sort(rng.uniform(100.0, 101.0, n))
    t[100:140] = t[100]                                               # a run of equal stamps
    np.save(os.path.join(root, "t.npy"), t)
    np.save(os.path.join(root, "xy.npy"), np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.int16))
    np.save(os.path.join(root, "p.npy"), rng.integers(0, 2, n).astype(np.uint8))
    if images:
        np.save(os.path.join(root, "images.npy"), rng.integers(0, 255, (frames, H, W, 1)).astype(np.uint8))
        np.save(os.path.join(root, "timestamps.npy"), np.linspace(100.05, 101.2, frames))
    return str(root)


def write_npy(path, n=N, seed=1):
    rng = np.random.default_rng(seed)
    t_us = np.sort(rng.uniform(0, 2e6, n)).round()
    data = np.stack([rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n), t_us], 1).astype(np.float64)
    np.save(path, data)
    return str(path)


METHODS = [
    {'method': 'k_events', 'k': 700, 'sliding_window_w': 0},
    {'method': 'k_events', 'k': 700, 'sliding_window_w': 100},
    {'method': 't_seconds', 't': 0.1, 'sliding_window_t': 0.0},
    {'method': 't_seconds', 't': 0.1, 'sliding_window_t': 0.04},
    {'method': 'fixed_frames', 'num_frames': 9},
    {'method': 'between_frames'},
]


def restated_windows(ts, method, frame_ts=None):
    """The reference's window rules (base_dataset.py:322-417), written out independently."""
    n = len(ts)
    m = method['method']
    if m == 'k_events':
        step = method['k'] - method['sliding_window_w']
        return [[step * i, step * i + method['k']] for i in range(int(n / step))]
    if m == 'between_frames':
        out, start = [], 0
        for f in frame_ts:
            end = min(int(np.searchsorted(ts, f)), n - 1)
            out.append([start, end])
            start = end
        return out
    if m == 'fixed_frames':
        length, t, sw = method['num_frames'], (ts[-1] - ts[0]) / method['num_frames'], 0
    else:
        t, sw = method['t'], method['sliding_window_t']
        length = int((ts[-1] - ts[0]) / (t - sw))
    out, start = [], 0
    for i in range(length):
        end = int(np.searchsorted(ts, (t - sw) * i + ts[0] + t))
        out.append([start, end])
        start = end
    return out


@pytest.mark.parametrize("method", METHODS, ids=lambda m: "-".join(str(v) for v in m.values()))
def test_memmap_window_tables_equal_the_restatement(tmp_path, method):
    # (frames only where every window ends inside the stream: upstream's compute_per_frame_indices reads ts[idx1] and raises
    # IndexError at construction otherwise, and so does this package)
    root = write_memmap(tmp_path / "mm", images=method['method'] in ('between_frames', 'fixed_frames'))
    ds = MemMapDataset(root, voxel_method=dict(method), **HOST_ONLY)
    ts = np.load(os.path.join(root, "t.npy"))
    want = restated_windows(ts, method, np.linspace(100.05, 101.2, 12))
    n_items = len(want) - 1 if method['method'] == 'between_frames' else len(want)
    assert len(ds) == n_items
    assert [list(map(int, w)) for w in ds.event_indices] == want
    assert tuple(map(int, ds.size())) == (H, W)
    for i in range(len(ds)):
        a, b = ds.get_event_indices(i)
        assert (a, b) == tuple(want[i])


@pytest.mark.parametrize("method", [m for m in METHODS if m['method'] != 'between_frames'],
                         ids=lambda m: "-".join(str(v) for v in m.values()))
def test_npy_window_tables_equal_the_restatement(tmp_path, method):
    path = write_npy(tmp_path / "ev.npy")
    ds = NpyDataset(path, voxel_method=dict(method), **HOST_ONLY)
    ts = np.load(path)[:, 3] * 1e-6
    assert [list(map(int, w)) for w in ds.event_indices] == restated_windows(ts, method)
    assert ds.size() == [H, W] or tuple(ds.size()) == (H, W)        # (max y + 1, max x + 1): the fixture fills the plane
    assert not ds.has_frames and ds.ts[3] == ts[3] and NpyDataset.ts(ds, 3) == ts[3]


def test_k_events_out_of_range_window_raises_and_the_length_cap(tmp_path):
    root = write_memmap(tmp_path / "mm", images=False)
    ds = MemMapDataset(root, voxel_method={'method': 'k_events', 'k': 700, 'sliding_window_w': 250}, **HOST_ONLY)
    last = ds.event_indices[-1]
    assert last[1] > N                                               # the last overlapping window runs past the stream
    with pytest.raises(Exception, match="out of bounds"):
        ds.get_event_indices(len(ds) - 1)
    capped = MemMapDataset(root, voxel_method={'method': 'k_events', 'k': 700, 'sliding_window_w': 0}, max_length=2,
                           **HOST_ONLY)
    assert len(capped) == 3                                          # max_length + 1, as upstream
    with pytest.raises(IndexError):
        capped[3]


def test_memmap_without_images_is_accepted(tmp_path):
    root = write_memmap(tmp_path / "mm", images=False)
    ds = MemMapDataset(root, voxel_method={'method': 'k_events', 'k': 1000, 'sliding_window_w': 0}, **HOST_ONLY)
    assert not ds.has_frames and ds.num_frames == 0 and len(ds) == 5
    assert tuple(ds.size()) == (H, W)


def test_memmap_reads_dataset_config(tmp_path):
    import json
    root = write_memmap(tmp_path / "mm", images=False)
    with open(os.path.join(root, "dataset_config.json"), "w") as f:
        json.dump({"data_source": "esim", "sensor_resolution": [31, 41]}, f)
    ds = MemMapDataset(root, voxel_method={'method': 'k_events', 'k': 1000, 'sliding_window_w': 0}, **HOST_ONLY)
    assert ds.size() == [31, 41] and ds.data_source == "esim"


def test_transform_names_come_from_a_table(tmp_path):
    root = write_memmap(tmp_path / "mm", images=False)
    method = {'method': 'k_events', 'k': 1000, 'sliding_window_w': 0}
    tr = {'CenterCrop': {'size': 20}, 'RobustNorm': {'low_perc': 5, 'top_perc': 90}}
    ds = MemMapDataset(root, voxel_method=dict(method), transforms=tr, **HOST_ONLY)
    assert 'RobustNorm' in tr                                        # the caller's dict is left as it was
    assert isinstance(ds.vox_transform, Compose) and [type(t) for t in ds.vox_transform.transforms] == [CenterCrop, RobustNorm]
    assert isinstance(ds.transform, CenterCrop)                      # frames get every transform but RobustNorm
    ds = MemMapDataset(root, voxel_method=dict(method), transforms={'CenterCrop': {'size': 20}}, **HOST_ONLY)
    assert ds.vox_transform is ds.transform and isinstance(ds.transform, CenterCrop)
    with pytest.raises(ValueError, match="unknown transform"):
        MemMapDataset(root, voxel_method=dict(method), transforms={'__import__("os")': {}}, **HOST_ONLY)


# ---- the reference's own index methods ------------------------------------------------------------------------------------

def _reference_loaders():
    root = os.environ.get("EVK_REFERENCE_ROOT", "/root/reference")
    path = os.path.join(root, "lib", "data_loaders")
    if not os.path.isfile(os.path.join(path, "base_dataset.py")):
        pytest.skip("reference checkout not available")
    import json
    for name in ("torchvision", "torchvision.transforms", "h5py"):
        sys.modules.setdefault(name, types.ModuleType(name))

    def pkg(name, p=None):
        m = sys.modules.get(name) or types.ModuleType(name)
        m.__path__ = [p] if p else []
        sys.modules[name] = m
        return m
    pkg("_evk_refdl")
    pkg("_evk_refdl.data_loaders", path)
    pkg("_evk_refdl.representations")
    pkg("_evk_refdl.util")
    vg = types.ModuleType("_evk_refdl.representations.voxel_grid")
    vg.events_to_voxel_torch = vg.events_to_neg_pos_voxel_torch = None
    sys.modules[vg.__name__] = vg
    uu = types.ModuleType("_evk_refdl.util.util")
    uu.read_json = lambda p: json.load(open(p))
    uu.write_json = None
    sys.modules[uu.__name__] = uu
    du = types.ModuleType("_evk_refdl.data_loaders.data_util")
    du.data_sources = ('esim', 'ijrr', 'mvsec', 'eccd', 'hqfd', 'unknown')
    sys.modules[du.__name__] = du
    return (importlib.import_module("_evk_refdl.data_loaders.memmap_dataset"),
            importlib.import_module("_evk_refdl.data_loaders.npy_dataset"),
            importlib.import_module("_evk_refdl.data_loaders.data_augmentation"))


@pytest.mark.parametrize("method", METHODS, ids=lambda m: "-".join(str(v) for v in m.values()))
def test_window_tables_equal_the_reference(tmp_path, method):
    ref_mm, ref_npy, _ = _reference_loaders()
    if method['method'] != 't_seconds':
        # (upstream's MemMapDataset needs images.npy, and with frames its t_seconds windows here end at num_events, where
        # compute_per_frame_indices raises IndexError: those go through the npy loader only)
        root = write_memmap(tmp_path / "mm")
        ref = ref_mm.MemMapDataset(root, voxel_method=dict(method))
        ours = MemMapDataset(root, voxel_method=dict(method), **HOST_ONLY)
        assert len(ours) == len(ref)
        assert [list(map(int, w)) for w in ours.event_indices] == [list(map(int, w)) for w in ref.event_indices]
        assert ours.frame_indices == [list(map(int, f)) for f in ref.frame_indices]
    if method['method'] != 'between_frames':
        path = write_npy(tmp_path / "ev.npy")
        ref = ref_npy.NpyDataset(path, voxel_method=dict(method), sensor_resolution=[H, W])
        ours = NpyDataset(path, voxel_method=dict(method), sensor_resolution=[H, W], **HOST_ONLY)
        assert [list(map(int, w)) for w in ours.event_indices] == [list(map(int, w)) for w in ref.event_indices]


def test_center_crop_equals_the_reference():
    _, _, ref_aug = _reference_loaders()
    x = torch.arange(2 * 17 * 23, dtype=torch.float32).reshape(2, 17, 23)
    for size in (5, (4, 9), (17, 23), (16, 22), (3, 20)):
        for mosaic in (False, True):
            if mosaic and (size == (17, 23)):
                continue                                             # (the even shift would run past the plane)
            a, b = CenterCrop(size, mosaic)(x), ref_aug.CenterCrop(size, mosaic)(x)
            assert torch.equal(a, b) and a.data_ptr() == b.data_ptr(), (size, mosaic)
            batch = CenterCrop(size, mosaic).batch(x[None])
            assert torch.equal(batch[0], a)


# ---- host logic -----------------------------------------------------------------------------------------------------------

def test_center_crop_offsets():
    assert CenterCrop(10).offsets(180, 240) == (85, 115)
    assert CenterCrop((3, 4)).offsets(8, 9) == (2, 2)                # round(2.5) = 2, round(2.5) = 2 (half to even)
    assert CenterCrop((3, 4), preserve_mosaicing_pattern=True).offsets(8, 10) == (2, 4)   # j = 3 -> 4
    assert CenterCrop((2, 2), preserve_mosaicing_pattern=True).offsets(5, 5) == (2, 2)
    assert CenterCrop((4, 4), preserve_mosaicing_pattern=True).offsets(7, 7) == (2, 2)    # round(1.5) = 2
    with pytest.raises(AssertionError):
        CenterCrop(50).offsets(40, 60)


def test_percentile_ranks_round_half_to_even():
    assert K.percentile_rank(0, 100) == 1 and K.percentile_rank(100, 100) == 100
    assert K.percentile_rank(50, 4) == 1 + round(1.5) == 3           # 1.5 -> 2
    assert K.percentile_rank(50, 6) == 1 + round(2.5) == 3           # 2.5 -> 2
    assert K.percentile_rank(50, 8) == 1 + round(3.5) == 5           # 3.5 -> 4
    assert K.percentile_rank(95, 432001) == 1 + round(.01 * 95.0 * 432000)
    assert K.percentile_rank(np.float32(95), 21) == 1 + round(.01 * float(np.float32(95)) * 20) == 20
    for q in (0, 5, 12.5, 50, 95, 100):
        for m in (1, 2, 7, 11, 101, 1000):
            k = K.percentile_rank(q, m)
            assert 1 <= k <= m and k == 1 + round(.01 * float(q) * (m - 1))


def test_percentile_ranks_equal_the_reference_kthvalue():
    _, _, ref_aug = _reference_loaders()
    rng = np.random.default_rng(3)
    for m in (1, 4, 6, 8, 21, 100):
        t = torch.from_numpy(rng.permutation(m).astype(np.float32))       # value == rank - 1
        for q in (0, 5, 50, 95, 100):
            assert ref_aug.RobustNorm.percentile(t, q) == K.percentile_rank(q, m) - 1


def test_collate_fn_batches_events():
    items = [{'events': torch.ones((3, 4)) * k, 'events_batch_indices': 3, 'voxel': torch.full((2, 2, 2), float(k)),
              'timestamp': np.float64(k)} for k in range(3)]
    out = BaseVoxelDataset.collate_fn(items)
    assert out['events'].shape == (9, 4)
    assert torch.equal(out['events_batch_indices'], torch.tensor([3, 6, 9]))        # (default_collate'd, as upstream)
    assert out['voxel'].shape == (3, 2, 2, 2) and torch.equal(out['timestamp'], torch.tensor([0., 1., 2.], dtype=torch.float64))


def test_unpack_batched_events():
    ev = torch.arange(9 * 4, dtype=torch.float32).reshape(9, 4)
    out = DU.unpack_batched_events(ev, [2, 7, 9])
    assert out.shape == (3, 1, 5, 4)
    assert torch.equal(out[0, 0, :2], ev[0:2]) and torch.equal(out[1, 0], ev[2:7]) and torch.equal(out[2, 0, :2], ev[7:9])
    assert not out[0, 0, 2:].any() and not out[2, 0, 2:].any()
    assert torch.equal(DU.unpack_batched_events(ev.reshape(1, 1, 9, 4), [9])[0, 0], ev)


def test_unpackage_events():
    ev = torch.arange(12.).reshape(3, 4)
    xs, ys, ts, ps = BaseVoxelDataset.unpackage_events(ev)
    assert torch.equal(ts, ev[:, 2]) and torch.equal(ps, ev[:, 3])


def _sig(f):
    return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]


def test_signatures_and_defaults():
    assert _sig(BaseVoxelDataset.__init__) == [
        ('self', inspect._empty), ('data_path', inspect._empty), ('transforms', {}), ('sensor_resolution', None),
        ('num_bins', 5), ('voxel_method', {'method': 'between_frames'}), ('max_length', None),
        ('combined_voxel_channels', False), ('return_events', False), ('return_voxelgrid', True), ('return_frame', True),
        ('return_prev_frame', False), ('return_flow', True), ('return_prev_flow', False), ('return_format', 'torch')]
    assert _sig(RobustNorm.__init__) == [('self', inspect._empty), ('low_perc', 0), ('top_perc', 95)]
    assert _sig(CenterCrop.__init__) == [('self', inspect._empty), ('size', inspect._empty), ('preserve_mosaicing_pattern', False)]
    import event_utils_amd.lib.data_loaders.memmap_dataset as aliased
    assert aliased.MemMapDataset is MemMapDataset
    from event_utils_amd.lib.data_loaders import base_dataset, data_augmentation, dataloader_util, npy_dataset  # noqa: F401
    ref = None
    try:
        ref = _reference_loaders()
    except pytest.skip.Exception:
        pass
    if ref is not None:
        ref_mm, ref_npy, ref_aug = ref
        for ours, theirs in ((MemMapDataset, ref_mm.MemMapDataset), (NpyDataset, ref_npy.NpyDataset)):
            for name in ("__init__", "__getitem__", "get_event_indices", "collate_fn", "unpackage_events", "size", "load_data",
                         "get_events", "preprocess_events", "set_voxel_method"):
                assert _sig(getattr(ours, name)) == _sig(getattr(theirs, name)), (ours, name)
        for name in ("Compose", "CenterCrop", "RobustNorm"):
            assert _sig(getattr(ref_aug, name).__init__) == _sig(globals()[name].__init__)


def test_window_kernels_compile_without_register_spills(tmp_path):
    """Every kernel of evk_windows.hip compiles for gfx950 without spilling registers or using scratch."""
    import re
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    from event_utils_amd.csrc import build as B
    src = os.path.join(B.HERE, "evk_windows.hip")
    subprocess.run([hipcc] + list(B.CFLAGS) + ["-c", src, "-o", str(tmp_path / "win.o"), "-save-temps=obj"], check=True,
                   cwd=B.HERE, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert asm, os.listdir(tmp_path)
    text = open(tmp_path / asm[0]).read()
    kernels = re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_spill_count:\s+(\d+)",
                         text)
    seen = {n: (int(sc), int(sp)) for n, sc, sp in kernels}
    assert {n for n in seen if "k_voxel_windows" in n} and {n for n in seen if "k_robust_select" in n}
    assert {n for n in seen if "k_robust_apply" in n}
    assert {n for n in seen if "k_pack_window_events" in n}
    assert not {n: v for n, v in seen.items() if any(v)}


def test_window_entry_points_reject_bad_arguments_without_a_gpu():
    """The argument checks of the new entry points run on the host, before anything is launched."""
    import ctypes
    from event_utils_amd import _lib
    from event_utils_amd.csrc import build
    build.build(verbose=False)
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)
    big = 1 << 15                                                   # 2^15 * 2^15 * 2 = 2^31 elements: past the loop bound
    assert L.evk_robust_norm_f32(fake, 1, 0, big, big, 2, 2 * big, 2, 1, 1, 1, fake, fake, None) == -1
    m_max = 0x7FFFFFFF - 4 * 1024
    assert L.evk_robust_norm_f32(fake, 1, 0, 1, 1, m_max + 1, 0, 0, 1, 1, 1, fake, fake, None) == -1
    assert L.evk_robust_norm_f32(fake, 1, 0, 1, 1, 10, 0, 0, 1, 11, 1, fake, fake, None) == -1     # rank past m
    assert L.evk_robust_norm_f32(fake, 1, 0, 1, 1, 10, 0, 0, 1, 1, 0, fake, fake, None) == -1      # rank 0
    assert L.evk_voxel_windows_f32(fake, None, _lib.EVK_SELECT_I16, 2, fake, _lib.EVK_T_F64, fake, 7, fake, 1, 5, 10, 10, 1,
                                   fake, None, None) == -1                                         # unknown polarity kind
    assert L.evk_pack_window_events_f32(fake, None, _lib.EVK_SELECT_I16, 2, fake, _lib.EVK_T_F64, fake, _lib.EVK_P_U8_PM1, fake,
                                        fake, 1, ctypes.c_void_p(4100), None) == -1                # unaligned rows
