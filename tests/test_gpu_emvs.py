"""GPU: event-based multi-view stereo (event_utils_amd/depth/emvs.py, evk_emvs.hip) against its float64 restatement
(tests/_emvs_np.py), bit for bit: the raw DSI, the index map and the mask are torch.equal, the depth map is equal NaNs included.  The
restatement is given the packet table the product computed (packet_times -> packet_transforms, host code checked in
test_cpu_emvs.py)."""
import functools
import math

import numpy as np
import pytest
import torch

import _emvs_np as N

pytestmark = pytest.mark.gpu

K = N.SCENE_K


def intr(Km):
    return (Km[0, 0], Km[1, 1], Km[0, 2], Km[1, 2])


def as_i32(raw64):
    """the restatement's int64 cells as the int32 tensor that holds the uint32 cells"""
    return torch.from_numpy((np.asarray(raw64) & 0xFFFFFFFF).astype(np.uint32).view(np.int32))


@functools.lru_cache(maxsize=None)
def scene():
    return N.scene()


def poses(sc):
    return dict(camera_matrix=K, pose_ts=sc["pose_ts"], positions=sc["positions"], quaternions=sc["quaternions"])


def check_votes(E, cols, host_xy, traj, reference, depths, sensor_size, packet_size, voting, ref_K=None, dsi_size=None, chunks=None):
    """dsi_votes on `cols` against the restatement on the host columns -> (DSI, expected int64 raw)"""
    from event_utils_amd.depth import emvs
    if chunks is None:
        dsi = E.dsi_votes(*cols, **traj, reference_pose=reference, depths=depths, sensor_size=sensor_size, packet_size=packet_size,
                          voting=voting, reference_camera_matrix=ref_K, dsi_size=dsi_size)
    else:                                                   # the call behind dsi_votes, with the event chunks forced
        dsi = emvs._votes(cols[0], cols[1], cols[2], traj["camera_matrix"], traj["pose_ts"], traj["positions"], traj["quaternions"],
                          reference, depths, sensor_size, packet_size, voting, ref_K, dsi_size, chunks=chunks)
    size = sensor_size if dsi_size is None else dsi_size
    n = len(host_xy[0])
    times = E.packet_times(cols[0], cols[1], cols[2], None, packet_size)
    assert times.shape == (math.ceil(n / min(packet_size, max(n, 1))),) and times.dtype == np.float64
    table = E.packet_transforms(times, traj["pose_ts"], traj["positions"], traj["quaternions"], traj["camera_matrix"], reference)
    want = N.dsi_votes(host_xy[0], host_xy[1], table, depths, intr(K if ref_K is None else ref_K), size, min(packet_size, max(n, 1)), voting)
    assert dsi.raw.dtype == torch.int32 and dsi.raw.is_cuda and tuple(dsi.raw.shape) == (len(depths),) + tuple(size)
    assert dsi.scale == N.SCALE[voting] and np.array_equal(dsi.depths, np.asarray(depths, dtype=np.float64))
    assert torch.equal(dsi.raw.cpu(), as_i32(want))
    return dsi, want


def check_depth_map(E, dsi, want_raw, **kw):
    dm = E.dsi_depth_map(dsi, **kw)
    depth, idx, conf, mask = N.dsi_depth_map(want_raw, dsi.scale, dsi.depths, **kw)
    assert dm.index.dtype == torch.int32 and dm.mask.dtype == torch.bool and dm.depth.dtype == torch.float64
    assert dm.confidence.dtype == torch.float32
    assert torch.equal(dm.index.cpu(), torch.from_numpy(idx)) and torch.equal(dm.mask.cpu(), torch.from_numpy(mask))
    assert np.array_equal(dm.depth.cpu().numpy(), depth, equal_nan=True)
    assert torch.equal(dm.confidence.cpu(), torch.from_numpy((conf.astype(np.float64) / dsi.scale).astype(np.float32)))
    return dm, mask


# ---- the seeded scene ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("voting", ["nearest", "bilinear"])
@pytest.mark.parametrize("kind", ["numpy", "tensors", "events_f64", "events_f32", "float32_xy"])
def test_the_seeded_scene(kind, voting):
    import event_utils_amd as E
    from event_utils_amd import _lib
    sc = scene()
    xs, ys, ts, ps = sc["xs"], sc["ys"], sc["ts"], sc["ps"]
    host = (xs, ys)
    if kind == "numpy":
        cols = (xs, ys, ts, ps)
    elif kind == "tensors":
        cols = tuple(torch.from_numpy(c).cuda() for c in (xs, ys, ts, ps))
    elif kind == "events_f64":
        cols = (E.DeviceEvents.from_arrays(xs, ys, ts, ps), None, None, None)
        assert cols[0].dtype == torch.float64
    elif kind == "events_f32":
        cols = (E.DeviceEvents.from_arrays(xs, ys, ts, ps, precision="f32"), None, None, None)
        assert cols[0].dtype == torch.float32
    else:                                                   # float32 coordinates off the pixel centres, float64 times
        host = ((xs + 0.25).astype(np.float32), (ys - 0.375).astype(np.float32))
        cols = (host[0], host[1], ts, None)
    assert _lib.lib().evk_emvs_chunks(len(ts), len(sc["depths"]), *N.SCENE_SIZE) == 2        # the call spans two event chunks
    dsi, want = check_votes(E, cols, host, poses(sc), N.SCENE_REFERENCE, sc["depths"], N.SCENE_SIZE, N.SCENE_PACKET, voting)
    assert int(want.sum()) > 500_000 * dsi.scale / 2
    votes = dsi.votes()
    assert votes.dtype == torch.float32 and torch.equal(votes.cpu(), torch.from_numpy((want / dsi.scale).astype(np.float32)))
    dm, mask = check_depth_map(E, dsi, want, filter_radius=2, threshold=40, median_size=0)
    assert mask.sum() > 50
    if kind == "numpy":
        check_depth_map(E, dsi, want, filter_radius=2, threshold=5.0, median_size=3)
        check_depth_map(E, dsi, want, filter_radius=3, threshold=12.5, median_size=5)
        # the times the packets took are those of the restatement
        assert np.array_equal(E.packet_times(xs, ys, ts, ps, N.SCENE_PACKET), N.packet_times(ts, N.SCENE_PACKET))


@pytest.mark.parametrize("voting", ["nearest", "bilinear"])
def test_two_calls_give_identical_bytes_and_the_chunks_do_not_matter(voting):
    import event_utils_amd as E
    sc = scene()
    cols = (sc["xs"], sc["ys"], sc["ts"], None)
    args = (E, cols, cols[:2], poses(sc), N.SCENE_REFERENCE, sc["depths"], N.SCENE_SIZE, N.SCENE_PACKET, voting)
    first, _ = check_votes(*args)
    second, _ = check_votes(*args)
    assert first.raw.data_ptr() != second.raw.data_ptr() and torch.equal(first.raw, second.raw)
    for chunks in (1, 5, 1000):                             # a one-chunk launch, several, more chunks than a wave of events each
        forced, _ = check_votes(*args, chunks=chunks)
        assert torch.equal(forced.raw, first.raw)
    dm = E.emvs_depth_map(*cols, **poses(sc), reference_pose=N.SCENE_REFERENCE, depths=sc["depths"], sensor_size=N.SCENE_SIZE,
                          packet_size=N.SCENE_PACKET, voting=voting, filter_radius=2, threshold=40, median_size=3)
    two = E.dsi_depth_map(first, filter_radius=2, threshold=40, median_size=3)
    assert torch.equal(dm.index, two.index) and torch.equal(dm.mask, two.mask) and torch.equal(dm.confidence, two.confidence)
    assert np.array_equal(dm.depth.cpu().numpy(), two.depth.cpu().numpy(), equal_nan=True) and bool(dm.mask.any())


# ---- packet edges, shapes ------------------------------------------------------------------------------------------------------------

def random_case(seed, n, size):
    """n events with real-valued coordinates over (and a little beyond) the sensor, times inside a five-pose trajectory"""
    rng = np.random.default_rng(seed)
    H, W = size
    xs = rng.uniform(-2.0, W + 2.0, n)
    ys = rng.uniform(-2.0, H + 2.0, n)
    ts = np.sort(rng.uniform(0.0, 1.0, n))
    pose_ts = np.linspace(0.0, 1.0, 5)
    positions = np.stack((-0.2 + 0.4 * pose_ts, 0.05 * np.cos(3 * pose_ts), 0.1 * pose_ts), axis=1)
    half = 0.5 * 0.2 * (pose_ts - 0.5)
    quats = np.stack((0.3 * np.sin(half), np.sin(half), np.zeros(5), np.cos(half)), axis=1)
    Km = np.array([[0.9 * W, 0.0, W / 2.0], [0.0, 0.9 * W, H / 2.0], [0.0, 0.0, 1.0]])
    return (xs, ys, ts), dict(camera_matrix=Km, pose_ts=pose_ts, positions=positions, quaternions=quats)


REF_NEAR = (np.array([0.02, -0.01, 0.0]), np.array([0.0, 0.01, 0.0, 1.0]))


@pytest.mark.parametrize("n, packet_size", [(0, 64), (1, 64), (37, 1), (37, 1000), (1000, 64), (1024, 64), (333, 2 ** 40)])
def test_packet_edges(n, packet_size):
    import event_utils_amd as E
    (xs, ys, ts), traj = random_case(n, n, (20, 31))
    depths = N.depth_planes(0.7, 3.0, 5)
    for voting in ("nearest", "bilinear"):
        dsi, want = check_votes(E, (xs, ys, ts, None), (xs, ys), traj, REF_NEAR, depths, (20, 31), packet_size, voting,
                                ref_K=traj["camera_matrix"])
        assert want.any() or n <= 1
        check_depth_map(E, dsi, want, filter_radius=1, threshold=0.0, median_size=3)


@pytest.mark.parametrize("depths, size", [([1.3], (20, 31)), ([3.0, 0.6, 1.0, 2.0, 0.8, 5.0, 1.5], (20, 31)), ([0.8, 2.0], (1, 45)),
                                          ([0.8, 2.0], (45, 1))])
def test_shapes(depths, size):
    import event_utils_amd as E
    (xs, ys, ts), traj = random_case(11, 3000, size)
    for voting in ("nearest", "bilinear"):
        dsi, want = check_votes(E, (xs, ys, ts, None), (xs, ys), traj, REF_NEAR, depths, size, 100, voting, ref_K=traj["camera_matrix"])
        assert want.any()
        check_depth_map(E, dsi, want, filter_radius=2, threshold=1.0, median_size=5)


def test_a_dsi_of_another_size_and_camera_than_the_sensor():
    import event_utils_amd as E
    (xs, ys, ts), traj = random_case(5, 4000, (30, 40))
    ref_K = np.array([[95.0, 0.0, 51.5], [0.0, 88.0, 33.25], [0.0, 0.0, 1.0]])
    for voting in ("nearest", "bilinear"):
        dsi, want = check_votes(E, (xs, ys, ts, None), (xs, ys), traj, REF_NEAR, [0.9, 1.7, 3.1], (30, 40), 128, voting, ref_K=ref_K,
                                dsi_size=(70, 101))
        assert want[:, 40:, :].any() and want[:, :, 50:].any()          # votes beyond the sensor's own extent


def test_row_bands_and_column_tiles():
    """a DSI of three row bands whose height is no multiple of the band, and one whose single row is wider than a tile"""
    import event_utils_amd as E
    from event_utils_amd import _lib
    L = _lib.lib()
    (xs, ys, ts), traj = random_case(8, 6000, (50, 64))
    for size, fx, fy in (((1300, 64), 60.0, 1500.0), ((1, 100001), 110000.0, 60.0), ((3, 50001), 60000.0, 60.0)):
        rows, cols = L.evk_emvs_band_rows(*size), L.evk_emvs_band_cols(*size)
        bands, tiles = math.ceil(size[0] / rows), math.ceil(size[1] / cols)
        assert bands * tiles >= 3 and (size[0] % rows or size[1] % cols)
        ref_K = np.array([[fx, 0.0, size[1] / 2.0], [0.0, fy, size[0] / 2.0], [0.0, 0.0, 1.0]])
        for voting in ("nearest", "bilinear"):
            dsi, want = check_votes(E, (xs, ys, ts, None), (xs, ys), traj, REF_NEAR, [1.1, 2.3], (50, 64), 256, voting, ref_K=ref_K,
                                    dsi_size=size)
            hit_rows, hit_cols = np.nonzero(want.sum(axis=0))
            assert len(set(hit_rows // rows)) == bands and len(set(hit_cols // cols)) == tiles          # every tile is voted into


def test_a_reference_pose_off_the_trajectory():
    """many rays leave the volume, and the nearest planes lie behind the camera centres of some packets but not of others"""
    import event_utils_amd as E
    (xs, ys, ts), traj = random_case(21, 8000, (40, 50))
    traj["positions"] = traj["positions"] + np.stack((np.zeros(5), np.zeros(5), np.linspace(0.0, 1.2, 5)), axis=1)
    reference = (np.array([0.5, 0.2, -0.1]), np.array([0.05, -0.2, 0.1, 1.0]))
    depths = N.depth_planes(0.4, 5.0, 9)
    table = E.packet_transforms(N.packet_times(ts, 200), traj["pose_ts"], traj["positions"], traj["quaternions"], traj["camera_matrix"],
                                reference)
    s = depths[:, None] - table[None, :, 11]
    assert ((s > 0).any(axis=1) & (s <= 0).any(axis=1)).sum() >= 2                  # planes behind some packets only
    for voting in ("nearest", "bilinear"):
        dsi, want = check_votes(E, (xs, ys, ts, None), (xs, ys), traj, reference, depths, (40, 50), 200, voting,
                                ref_K=traj["camera_matrix"])
        assert 0 < want.sum() < 0.5 * len(ts) * len(depths) * dsi.scale
        check_depth_map(E, dsi, want, filter_radius=2, threshold=2.0, median_size=3)


def test_planes_exactly_on_camera_centres_with_unnormalised_quaternions():
    """s = Z - C_2 == 0 votes nowhere.  The planes are C_2 of three packets of packet_transforms on the caller's unnormalised
    quaternions; dsi_votes once normalised them a second time, s came out an ulp above zero and every ray of those packets voted
    into the cell of the camera centre (tools/fuzz_parity.py --kinds emvs; the host-side pin is in test_cpu_emvs.py)."""
    import event_utils_amd as E
    from event_utils_amd.depth import emvs
    (xs, ys, ts), traj = random_case(31, 600, (20, 31))
    traj["positions"] = traj["positions"] + np.stack((np.zeros(5), np.zeros(5), np.linspace(0.3, 1.5, 5)), axis=1)
    rng = np.random.default_rng(3)                          # (a reference quaternion that a second normalisation moves the telling way)
    traj["quaternions"] = (traj["quaternions"] + 0.05 * rng.normal(size=(5, 4))) * np.array([1.7, 0.3, -2.9, 1.1, 0.6])[:, None]
    reference = (np.array([0.1, -0.05, 0.0]), np.array([0.0, 0.0, 0.0, 1.3]) + 0.1 * rng.normal(size=4))
    times = N.packet_times(ts, 20)
    table = E.packet_transforms(times, traj["pose_ts"], traj["positions"], traj["quaternions"], traj["camera_matrix"], reference)
    # the packets that tell the two tables apart: with the poses normalised twice their C_2 lies an ulp below
    checked = emvs._check_poses(traj["pose_ts"], traj["positions"], traj["quaternions"], reference)
    twice = E.packet_transforms(times, checked[0], checked[1], checked[2], traj["camera_matrix"], checked[3])
    packets = np.flatnonzero((twice[:, 11] < table[:, 11]) & (table[:, 11] > 0))[:3]
    depths = table[packets, 11]
    assert len(packets) == 3 and ((depths[:, None] - table[None, :, 11]) == 0).sum() == 3
    for voting in ("nearest", "bilinear"):
        dsi, want = check_votes(E, (xs, ys, ts, None), (xs, ys), traj, reference, depths, (20, 31), 20, voting, ref_K=traj["camera_matrix"])
        assert want.any()
        assert not np.array_equal(N.dsi_votes(xs, ys, twice, depths, intr(traj["camera_matrix"]), (20, 31), 20, voting), want)


@pytest.mark.parametrize("voting, x, y, cell", [("nearest", 10.0, 7.0, {(7, 10): 70000}),
                                                ("bilinear", 10.25, 7.5, {(7, 10): 96 * 70000, (7, 11): 32 * 70000, (8, 10): 96 * 70000,
                                                                          (8, 11): 32 * 70000})])
def test_a_hot_cell_counts_exactly(voting, x, y, cell):
    import event_utils_amd as E
    n = 70_000                                              # more than a 16-bit cell holds
    Km = np.array([[64.0, 0.0, 32.0], [0.0, 64.0, 24.0], [0.0, 0.0, 1.0]])
    traj = dict(camera_matrix=Km, pose_ts=np.array([0.0, 1.0]), positions=np.zeros((2, 3)), quaternions=np.tile([0.0, 0.0, 0.0, 1.0], (2, 1)))
    xs, ys, ts = np.full(n, x), np.full(n, y), np.linspace(0.0, 1.0, n)
    dsi = E.dsi_votes(xs, ys, ts, None, **traj, reference_pose=(np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0])), depths=[1.0, 2.0],
                      sensor_size=(48, 64), voting=voting)
    want = np.zeros((2, 48, 64), dtype=np.int64)
    for (yy, xx), v in cell.items():
        want[:, yy, xx] = v
    assert torch.equal(dsi.raw.cpu(), as_i32(want))


# ---- the depth map on its own ----------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def random_raw():
    rng = np.random.default_rng(17)
    raw = rng.integers(0, 60, (6, 19, 23)) * (rng.random((6, 19, 23)) < 0.5)
    raw[:, rng.random((19, 23)) < 0.3] = 0                  # all-zero columns
    raw[:, 4:9, 10:15] += rng.integers(100, 400, (6, 5, 5))  # a ridge that stands above its surroundings
    raw[2, 0, 0] = raw[4, 0, 0] = 300                       # a tie at an image corner
    raw[3, 18, 22] = 2 ** 32 - 7                            # a cell above 2^31: the cells are unsigned
    return raw.astype(np.int64)


@pytest.mark.parametrize("median_size", [0, 3, 5])
@pytest.mark.parametrize("radius", [0, 2])
@pytest.mark.parametrize("scale, threshold", [(1, 20.0), (256, 0.1)])
def test_depth_map_of_a_handed_in_raw(scale, threshold, radius, median_size):
    import event_utils_amd as E
    raw = random_raw()
    depths = np.array([4.0, 0.5, 1.0, 3.0, 2.0, 8.0])
    for handed in (as_i32(raw).cuda(), as_i32(raw).numpy()):
        dm, mask = check_depth_map(E, E.DSI(handed, scale, depths), raw, filter_radius=radius, threshold=threshold, median_size=median_size)
    assert mask.any() == (radius > 0) and not mask.all()    # (r = 0: conf - conf > threshold never holds)


def test_depth_to_points_against_numpy():
    import event_utils_amd as E
    sc = scene()
    reference = (np.array([0.3, -0.2, 0.1]), np.array([0.1, -0.05, 0.02, 0.99]))
    dm = E.emvs_depth_map(sc["xs"], sc["ys"], sc["ts"], None, **poses(sc), reference_pose=reference, depths=sc["depths"],
                          sensor_size=N.SCENE_SIZE, packet_size=N.SCENE_PACKET, threshold=20)
    points = E.depth_to_points(dm, K, reference)
    assert points.is_cuda and points.dtype == torch.float64
    mask, depth = dm.mask.cpu().numpy(), dm.depth.cpu().numpy()
    vs, us = np.nonzero(mask)
    assert len(vs) > 50 and points.shape == (len(vs), 3)
    R = N.quat_to_matrix(reference[1])
    want = np.stack([reference[0] + R @ (depth[v, u] * np.array([(u - K[0, 2]) / K[0, 0], (v - K[1, 2]) / K[1, 1], 1.0])) for v, u in zip(vs, us)])
    assert np.abs(points.cpu().numpy() - want).max() < 1e-12
    host = E.depth_to_points(E.DepthMap(depth, None, None, mask), K, reference)
    assert isinstance(host, np.ndarray) and np.abs(host - want).max() < 1e-12
