"""CPU (no GPU): the host restatement of event-based multi-view stereo (tests/_emvs_np.py, the literal float64 definition) on
hand-worked cases; packet_transforms against closed forms; the restatement recovers depth on the seeded scene; the evk_emvs_* entry
points are declared, bound and exported and refuse bad arguments before they touch the device; the Python argument errors; the
public surface; the kernels of evk_emvs.hip compile for gfx950 without register spills."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _emvs_np as N
import _header

ENTRIES = {"evk_emvs_packet_times", "evk_emvs_band_rows", "evk_emvs_band_cols", "evk_emvs_chunks", "evk_emvs_votes",
           "evk_emvs_depth_map"}

# identity pose, reference = camera, C = 0; power-of-two focal lengths keep K^-1 exact: every plane then votes at (x, y) exactly
FX, FY, CX, CY = 64.0, 64.0, 32.0, 24.0
INTR = (FX, FY, CX, CY)
H, W = 48, 64
IDENT = np.array([1 / FX, 0.0, -CX / FX, 0.0, 1 / FY, -CY / FY, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0])


def votes(xs, ys, rows=None, depths=(1.0, 2.0, 4.0), voting="nearest", packet_size=1, size=(H, W)):
    rows = [IDENT] * len(xs) if rows is None else rows
    return N.dsi_votes(np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64), np.array(rows), depths, INTR, size,
                       packet_size, voting)


def cells(raw):
    """{(plane, y, x): value} of the non-zero cells"""
    return {tuple(int(v) for v in k): int(raw[tuple(k)]) for k in np.argwhere(raw)}


# ---- hand-worked cases of the restatement --------------------------------------------------------------------------------------------

def test_identity_votes_at_the_event_pixel_on_every_plane():
    raw = votes([10.0, 40.0], [7.0, 30.0])
    assert cells(raw) == {(i, y, x): 1 for i in range(3) for x, y in ((10, 7), (40, 30))}
    assert raw.dtype == np.int64 and raw.shape == (3, H, W)


def test_a_camera_centre_at_or_beyond_a_plane_silences_that_plane():
    row = IDENT.copy()
    row[11] = 2.0                                           # C_2 = 2: the planes Z = 1 and Z = 2 have s <= 0
    raw = votes([32.0], [24.0], rows=[row])
    assert cells(raw) == {(2, 24, 32): 1}                   # on the axis the ray stays at the principal point
    row[11] = 4.0
    assert not votes([32.0], [24.0], rows=[row]).any()


def test_a_ray_with_d2_not_positive_is_skipped():
    for d2 in (0.0, -1.0):
        row = IDENT.copy()
        row[8] = d2
        assert not votes([10.0], [7.0], rows=[row]).any()
    row = IDENT.copy()
    row[6:9] = [float("nan"), 0.0, 1.0]                     # a NaN d_2 fails d_2 > 0 too
    assert not votes([10.0], [7.0], rows=[row]).any()


def test_nearest_rounds_half_up_and_drops_what_leaves_the_image():
    raw = votes([10.5, 11.5, -0.5, -0.75, W - 0.5], [7.5, 8.5, 0.0, 0.0, 0.0], depths=(1.0,))
    # u = k + 0.5 votes at k + 1 (not to even); -0.5 -> 0; -0.75 -> -1 and W - 0.5 -> W are outside
    assert cells(raw) == {(0, 8, 11): 1, (0, 9, 12): 1, (0, 0, 0): 1}
    assert not votes([float("nan"), float("inf"), 1e300], [3.0, 3.0, 3.0], depths=(1.0,)).any()


def test_bilinear_weights_of_a_dyadic_fraction():
    raw = votes([10.25], [7.5], depths=(1.0,), voting="bilinear")           # fu = 0.25, fv = 0.5
    assert cells(raw) == {(0, 7, 10): 96, (0, 7, 11): 32, (0, 8, 10): 96, (0, 8, 11): 32}
    assert votes([10.0], [7.0], depths=(1.0,), voting="bilinear")[0, 7, 10] == 256
    # rint is round-half-even: fu = 2^-9 gives 255.5 -> 256 and 0.5 -> 0
    raw = votes([10.0 + 2.0 ** -9], [7.0], depths=(1.0,), voting="bilinear")
    assert cells(raw) == {(0, 7, 10): 256}
    raw = votes([10.0 + 3 * 2.0 ** -9], [7.0], depths=(1.0,), voting="bilinear")   # 254.5 -> 254, 1.5 -> 2
    assert cells(raw) == {(0, 7, 10): 254, (0, 7, 11): 2}


def test_bilinear_drops_a_corner_outside_on_its_own():
    raw = votes([-0.75, W - 0.75], [7.5, H - 0.5], depths=(1.0,), voting="bilinear")
    # (-0.75, 7.5): x0 = -1 is outside, the two corners at x = 0 stay (fu = 0.25: 32 each)
    # (W - 0.75, H - 0.5): only the corner (W - 1, H - 1) is inside: (1 - 0.25)(1 - 0.5) 256 = 96
    assert cells(raw) == {(0, 7, 0): 32, (0, 8, 0): 32, (0, H - 1, W - 1): 96}
    assert not votes([float("nan"), float("-inf"), -1e300], [3.0, 3.0, 3.0], depths=(1.0,), voting="bilinear").any()


def test_packets_take_their_own_row():
    shifted = IDENT.copy()
    shifted[9] = 0.5                                        # C_0 = 0.5: u = fx (0.5 + Z a) / Z + cx moves by 32 / Z
    raw = votes([10.0] * 5, [7.0] * 5, rows=[IDENT, shifted, IDENT], depths=(1.0, 2.0), packet_size=2)
    assert cells(raw) == {(0, 7, 10): 3, (0, 7, 42): 2, (1, 7, 10): 3, (1, 7, 26): 2}
    assert N.packet_times([0.0, 1.0, 2.0, 3.0, 4.0], 2).tolist() == [1.0, 3.0, 4.0]
    assert N.packet_times([0.0, 1.0, 2.0], 5).tolist() == [1.0] and N.packet_times([], 4).tolist() == []


def test_depth_map_takes_the_first_maximum():
    raw = np.zeros((4, 3, 3), dtype=np.int64)
    raw[1, 1, 1] = raw[3, 1, 1] = 9                         # two equal maxima: the smaller plane index
    raw[2, 0, 0] = 1
    depth, idx, conf, mask = N.dsi_depth_map(raw, 1, [1.0, 2.0, 3.0, 4.0], filter_radius=1, threshold=0.0, median_size=0)
    assert conf[1, 1] == 9 and idx[1, 1] == 1 and depth[1, 1] == 2.0 and mask[1, 1]
    assert conf[2, 2] == 0 and idx[2, 2] == -1 and not mask[2, 2] and math.isnan(depth[2, 2])
    assert idx.dtype == np.int32 and mask.dtype == bool


def test_the_box_threshold_keeps_its_area_at_an_image_corner():
    raw = np.zeros((1, 6, 6), dtype=np.int64)
    raw[0, :3, :3] = 10                                     # the corner pixel's window holds 9 cells of 10, area stays 25
    # conf area - S = 250 - 90 = 160 against floor(t) 25: masked up to floor(t) = 6.  With the clipped area 9 instead,
    # conf area - S would be 0 and the corner never masked
    for t, want in ((0.0, True), (6.0, True), (6.9, True), (7.0, False)):
        assert bool(N.dsi_depth_map(raw, 1, [1.0], filter_radius=2, threshold=t, median_size=0)[3][0, 0]) == want, t
    # the pixel (2, 2) sees all nine: 250 - 90 as well; (3, 3) is empty
    mask = N.dsi_depth_map(raw, 1, [1.0], filter_radius=2, threshold=6.0, median_size=0)[3]
    assert mask[:3, :3].all() and mask.sum() == 9
    # the threshold is floor(threshold * scale) raw units: at scale 256 the level 10 is 10 / 256 votes
    assert not N.dsi_depth_map(raw, 256, [1.0], filter_radius=2, threshold=1.0, median_size=0)[3].any()
    assert N.dsi_depth_map(raw, 256, [1.0], filter_radius=2, threshold=6.0 / 256, median_size=0)[3][0, 0]
    assert not N.dsi_depth_map(raw, 256, [1.0], filter_radius=2, threshold=7.0 / 256, median_size=0)[3][0, 0]


def test_the_median_of_an_even_count_is_the_lower_one():
    raw = np.zeros((8, 5, 5), dtype=np.int64)
    for x, plane in ((0, 6), (1, 2), (3, 5), (4, 1)):       # four isolated peaks on one row; x = 2 stays empty
        raw[plane, 2, x] = 50
    _, idx0, _, mask = N.dsi_depth_map(raw, 1, np.arange(1.0, 9.0), filter_radius=0, threshold=0.0, median_size=0)
    assert not mask.any()                                   # r = 0: conf - conf > 0 never holds
    _, idx0, _, mask = N.dsi_depth_map(raw, 1, np.arange(1.0, 9.0), filter_radius=1, threshold=0.0, median_size=0)
    assert mask[2].tolist() == [True, True, False, True, True] and idx0[2].tolist() == [6, 2, -1, 5, 1]
    depth, idx3, _, _ = N.dsi_depth_map(raw, 1, np.arange(1.0, 9.0), filter_radius=1, threshold=0.0, median_size=3)
    assert idx3[2].tolist() == [2, 2, -1, 1, 1]             # windows {6, 2}, {6, 2}, -, {5, 1}, {5, 1}: the lower of two
    assert depth[2, 0] == 3.0 and math.isnan(depth[2, 2])
    _, idx5, _, _ = N.dsi_depth_map(raw, 1, np.arange(1.0, 9.0), filter_radius=1, threshold=0.0, median_size=5)
    assert idx5[2].tolist() == [2, 5, -1, 2, 1]             # {6, 2}, {6, 2, 5}, -, {2, 5, 1}, {5, 1}


# ---- packet_transforms -----------------------------------------------------------------------------------------------------------

def quat_y(angle):
    return np.array([0.0, math.sin(angle / 2), 0.0, math.cos(angle / 2)])


def rot_y(angle):
    c, s = math.cos(angle), math.sin(angle)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


K64 = np.array([[FX, 0.0, CX], [0.0, FY, CY], [0.0, 0.0, 1.0]])
KINV64 = np.array([[1 / FX, 0.0, -CX / FX], [0.0, 1 / FY, -CY / FY], [0.0, 0.0, 1.0]])
REF0 = (np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]))


def test_slerp_of_a_quarter_turn_against_closed_forms():
    import event_utils_amd as E
    positions = np.array([[1.0, 2.0, 3.0], [3.0, 2.0, -1.0]])
    quats = np.stack((quat_y(0.0), quat_y(math.pi / 2)))
    rows = E.packet_transforms([10.0, 10.5, 11.0, 10.25], [10.0, 11.0], positions, quats, K64, REF0)
    assert rows.shape == (4, 12) and rows.dtype == np.float64
    for row, f in zip(rows, (0.0, 0.5, 1.0, 0.25)):
        assert np.abs(row[:9].reshape(3, 3) - rot_y(f * math.pi / 2) @ KINV64).max() < 1e-12
        assert np.abs(row[9:] - (positions[0] + f * (positions[1] - positions[0]))).max() < 1e-12
    assert np.array_equal(rows[0], np.concatenate((KINV64.reshape(-1), positions[0])))        # identity: exact
    # a reference pose rotates and shifts both parts: M = R_ref^T R_j K^-1, C = R_ref^T (c_j - c_ref)
    ref = (np.array([0.5, -1.0, 2.0]), 3.0 * quat_y(math.pi / 6))                              # (normalised on entry)
    rows = E.packet_transforms([10.5], [10.0, 11.0], positions, quats, K64, ref)
    assert np.abs(rows[0, :9].reshape(3, 3) - rot_y(-math.pi / 6) @ rot_y(math.pi / 4) @ KINV64).max() < 1e-12
    assert np.abs(rows[0, 9:] - rot_y(-math.pi / 6) @ (np.array([2.0, 2.0, 1.0]) - ref[0])).max() < 1e-12


def test_sign_flipped_and_scaled_quaternions_give_the_same_rows():
    import event_utils_amd as E
    rng = np.random.default_rng(3)
    quats = rng.normal(size=(5, 4))
    positions = rng.normal(size=(5, 3))
    pose_ts = np.arange(5.0)
    times = rng.uniform(0.0, 4.0, 20)
    base = E.packet_transforms(times, pose_ts, positions, quats, K64, REF0)
    flipped = quats * np.array([1.0, -1.0, 2.5, -0.5, -1.0])[:, None]
    assert np.abs(E.packet_transforms(times, pose_ts, positions, flipped, K64, REF0) - base).max() < 1e-12
    assert np.abs(E.packet_transforms(times, pose_ts, positions, quats, K64, (REF0[0], -REF0[1])) - base).max() < 1e-12
    for row in base:                                        # every M K is a rotation
        R = row[:9].reshape(3, 3) @ K64
        assert np.abs(R @ R.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R) - 1.0) < 1e-12
    # nearly coincident quaternions take the normalised lerp: still a rotation, still continuous
    near = np.stack((quat_y(0.3), quat_y(0.3 + 1e-9)))
    row = E.packet_transforms([0.5], [0.0, 1.0], positions[:2], near, K64, REF0)[0]
    assert np.abs(row[:9].reshape(3, 3) - rot_y(0.3 + 0.5e-9) @ KINV64).max() < 1e-12


def test_dsi_votes_takes_the_table_of_the_callers_poses(monkeypatch):
    """dsi_votes votes with packet_transforms(packet_times(...), the caller's poses): it once handed packet_transforms quaternions
    it had already normalised, which packet_transforms normalised again -- most entries of the table moved by an ulp, and a plane
    that lies exactly on a packet's camera centre (s = Z - C_2 == 0: no vote) took all the packet's rays into one cell (found by
    tools/fuzz_parity.py --kinds emvs, profiles/fuzz_emvs_simulate.txt).  The device layer is replaced by a recorder: what is
    compared is the table that reaches evk_emvs_votes."""
    import torch
    import event_utils_amd as E
    from event_utils_amd.depth import emvs
    rng = np.random.default_rng(3)
    quats, positions, pose_ts = rng.normal(size=(5, 4)) * 1.7, rng.normal(size=(5, 3)), np.arange(5.0)
    reference = (rng.normal(size=3), rng.normal(size=4))
    ts = np.sort(rng.uniform(0.0, 4.0, 100))
    xs, ys = rng.uniform(0.0, 63.0, 100), rng.uniform(0.0, 47.0, 100)
    want = E.packet_transforms(N.packet_times(ts, 5), pose_ts, positions, quats, K64, reference)
    checked = emvs._check_poses(pose_ts, positions, quats, reference)
    twice = E.packet_transforms(N.packet_times(ts, 5), checked[0], checked[1], checked[2], K64, checked[3])
    assert (twice != want).any() and np.abs(twice - want).max() < 1e-12          # the case can tell the two tables apart
    seen = {}

    def record(name, *args):
        if name == "evk_emvs_votes":
            seen["table"] = np.ctypeslib.as_array((ctypes.c_double * (12 * args[6])).from_address(args[5].value)).reshape(-1, 12).copy()
            seen["depths"] = np.ctypeslib.as_array((ctypes.c_double * args[9]).from_address(args[7].value)).copy()
    monkeypatch.setattr(emvs, "_columns", lambda x, y, t: tuple(torch.from_numpy(np.asarray(c, np.float64)) for c in (x, y, t)) + (0.0,))
    monkeypatch.setattr(emvs, "_packet_times", lambda t, t_offset, n, packet_size: N.packet_times(t.numpy(), packet_size))
    monkeypatch.setattr(emvs.D, "stream", lambda: None)
    monkeypatch.setattr(emvs._lib, "call", record)
    Z = float(want[7, 11]) if want[7, 11] > 0 else 1.0      # a plane on the camera centre of packet 7, where there is one in front
    emvs.dsi_votes(xs, ys, ts, None, K64, pose_ts, positions, quats, reference, [Z, 2.0], (48, 64), packet_size=5)
    assert np.array_equal(seen["table"], want) and np.array_equal(seen["depths"], [Z, 2.0])
    assert Z == 1.0 or seen["depths"][0] - seen["table"][7, 11] == 0.0


def test_packet_times_outside_the_trajectory_are_refused():
    import event_utils_amd as E
    args = ([0.0, 1.0], np.zeros((2, 3)), np.tile(quat_y(0.0), (2, 1)), K64, REF0)
    assert E.packet_transforms([0.0, 1.0], *args).shape == (2, 12)
    assert E.packet_transforms([], *args).shape == (0, 12)
    for bad in (-1e-9, 1.0 + 1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="packet times"):
            E.packet_transforms([0.5, bad], *args)
    with pytest.raises(ValueError, match="strictly increasing"):
        E.packet_transforms([0.5], [0.0, 0.0], *args[1:])
    with pytest.raises(ValueError, match="positions"):
        E.packet_transforms([0.5], [0.0, 1.0], np.zeros((3, 3)), *args[2:])
    with pytest.raises(ValueError, match="quaternions"):
        E.packet_transforms([0.5], [0.0, 1.0], np.zeros((2, 3)), np.zeros((2, 4)), K64, REF0)
    with pytest.raises(ValueError, match="no skew"):
        E.packet_transforms([0.5], *args[:3], np.array([[64.0, 1.0, 32.0], [0.0, 64.0, 24.0], [0.0, 0.0, 1.0]]), REF0)
    with pytest.raises(ValueError, match="reference_pose"):
        E.packet_transforms([0.5], *args[:4], (np.zeros(2), quat_y(0.0)))


def test_depth_planes_are_uniform_in_inverse_depth():
    import event_utils_amd as E
    z = E.depth_planes(0.5, 4.0, 32)
    assert z.dtype == np.float64 and z.shape == (32,) and z[0] == 0.5 and abs(z[-1] - 4.0) < 1e-15
    assert np.abs(np.diff(1.0 / z) - (0.25 - 2.0) / 31).max() < 1e-15
    assert np.array_equal(z, N.depth_planes(0.5, 4.0, 32)) and E.depth_planes(2.0, 9.0, 1).tolist() == [2.0]
    for bad in ((0.0, 1.0, 4), (1.0, -2.0, 4), (1.0, 2.0, 0), (1.0, float("inf"), 3)):
        with pytest.raises(ValueError):
            E.depth_planes(*bad)


# ---- the seeded scene ------------------------------------------------------------------------------------------------------------

def test_the_restatement_recovers_depth_on_the_seeded_scene():
    """120 points on Z = 1 and Z = 2, 201 poses, 23 807 events, 32 planes, nearest voting, filter_radius 2, threshold 40, no median:
    measured 0.900 of the points' reference pixels masked in and 0.944 of those within one plane of the true one (bilinear voting:
    0.875 and 0.962, not asserted)."""
    import event_utils_amd as E
    sc = N.scene()
    assert len(sc["ts"]) == 23807
    table = E.packet_transforms(N.packet_times(sc["ts"], N.SCENE_PACKET), sc["pose_ts"], sc["positions"], sc["quaternions"], N.SCENE_K,
                                N.SCENE_REFERENCE)
    K = N.SCENE_K
    raw = N.dsi_votes(sc["xs"], sc["ys"], table, sc["depths"], (K[0, 0], K[1, 1], K[0, 2], K[1, 2]), N.SCENE_SIZE, N.SCENE_PACKET)
    depth, idx, conf, mask = N.dsi_depth_map(raw, 1, sc["depths"], filter_radius=2, threshold=40, median_size=0)
    px = np.rint(sc["pixels"]).astype(int)
    masked = mask[px[:, 1], px[:, 0]]
    true_idx = np.array([np.argmin(np.abs(1.0 / sc["depths"] - 1.0 / z)) for z in sc["true_depth"]])
    close = np.abs(idx[px[:, 1], px[:, 0]][masked] - true_idx[masked]) <= 1
    print("masked in %.3f, within one plane %.3f" % (masked.mean(), close.mean()))
    assert masked.mean() >= 0.80 and close.mean() >= 0.85
    assert np.array_equal(np.isnan(depth), ~mask) and np.array_equal(depth[mask], sc["depths"][idx[mask]])


# ---- the public surface and the C ABI ------------------------------------------------------------------------------------------------

def test_the_prototypes_are_bound_with_their_arguments():
    from event_utils_amd import _lib
    text = _header.TEXT
    protos = _header.prototypes("evk_emvs_")
    assert set(protos) == ENTRIES
    for name, want in protos.items():
        assert _lib.PROTOTYPES[name] == want and want[1] is ctypes.c_int, name
        assert hasattr(_lib.lib(), name)
    assert (_lib.EVK_EMVS_NEAREST, _lib.EVK_EMVS_BILINEAR, _lib.EVK_EMVS_BILINEAR_MAX_EVENTS) == (0, 1, 1 << 24)
    for name, value in (("EVK_EMVS_NEAREST", 0), ("EVK_EMVS_BILINEAR", 1), ("EVK_EMVS_BILINEAR_MAX_EVENTS", 1 << 24)):
        assert re.search(r"^#define\s+%s\s+%d\s*$" % (name, value), text, re.M)
    assert "Event-based multi-view stereo" in text


def test_public_surface():
    import inspect
    import event_utils_amd as E
    import event_utils_amd.lib.depth as alias_pkg
    import event_utils_amd.lib.depth.emvs as alias
    from event_utils_amd import depth
    from event_utils_amd.depth import emvs
    assert alias is emvs and alias_pkg is depth
    for name in ("DSI", "DepthMap", "depth_planes", "packet_transforms", "packet_times", "dsi_votes", "dsi_depth_map", "emvs_depth_map",
                 "depth_to_points"):
        assert getattr(E, name) is getattr(emvs, name) is getattr(depth, name)
    assert "(no reference module)           -> event_utils_amd.depth.emvs" in E.__doc__
    assert E.DSI._fields == ("raw", "scale", "depths") and callable(E.DSI.votes)
    assert E.DepthMap._fields == ("depth", "index", "confidence", "mask")
    empty = inspect.Parameter.empty

    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    head = [(n, empty) for n in ("xs", "ys", "ts", "ps", "camera_matrix", "pose_ts", "positions", "quaternions", "reference_pose",
                                 "depths", "sensor_size")]
    tail = [("packet_size", 1024), ("voting", "nearest"), ("reference_camera_matrix", None), ("dsi_size", None)]
    assert params(E.dsi_votes) == head + tail
    assert params(E.emvs_depth_map) == head + tail + [("filter_radius", 2), ("threshold", 5.0), ("median_size", 3)]
    assert params(E.dsi_depth_map) == [("dsi", empty), ("filter_radius", 2), ("threshold", 5.0), ("median_size", 3)]
    assert params(E.packet_transforms) == [(n, empty) for n in ("packet_ts", "pose_ts", "positions", "quaternions", "camera_matrix",
                                                                "reference_pose")]
    assert params(E.depth_to_points) == [(n, empty) for n in ("depth_map", "reference_camera_matrix", "reference_pose")]
    assert params(E.depth_planes) == [(n, empty) for n in ("z_min", "z_max", "n")]


def test_the_tiles_and_the_packet_division():
    """the geometry the GPU tests build their cases on, and the division by the packet size the kernels use (a multiply and a shift)"""
    from event_utils_amd import _lib
    L = _lib.lib()
    assert L.evk_emvs_band_rows(180, 240) == 90 and L.evk_emvs_band_cols(180, 240) == 240          # two bands of 86 400 bytes
    assert L.evk_emvs_band_rows(260, 346) == 87 and L.evk_emvs_band_rows(48, 64) == 48
    assert L.evk_emvs_band_rows(1300, 64) == 434 and L.evk_emvs_band_rows(1, 7) == 1
    assert L.evk_emvs_band_cols(1, 100001) == 33334 and L.evk_emvs_band_rows(3, 100001) == 1       # a row wider than the LDS
    for h, w in ((180, 240), (260, 346), (1300, 64), (1, 100001), (3, 100001), (40000, 1), (7, 39999)):
        assert 1 <= L.evk_emvs_band_rows(h, w) * L.evk_emvs_band_cols(h, w) <= 40000
    assert L.evk_emvs_chunks(10_000_000, 100, 180, 240) == 6 and L.evk_emvs_chunks(1000, 1, 8, 8) == 1
    assert L.evk_emvs_chunks(0, 1, 8, 8) == 1 and L.evk_emvs_chunks(100_000, 1, 8, 8) == 7
    rng = np.random.default_rng(0)
    ds = np.concatenate(([1, 2, 3, 5, 7, 1023, 1024, 1025, 2 ** 31 - 1, 2 ** 31, 2 ** 30 + 1], rng.integers(1, 2 ** 31, 200),
                         rng.integers(1, 5000, 200))).astype(object)
    top = 2 ** 31 - 1
    for d in ds:
        d = int(d)
        l = 0 if d <= 1 else (d - 1).bit_length()
        m = ((1 << (31 + l)) + d - 1) // d
        assert m < 2 ** 32
        tries = [0, 1, d - 1, d, d + 1, top, top - 1, (top // d) * d, (top // d) * d - 1] + [int(v) for v in rng.integers(0, 2 ** 31, 50)]
        for i in tries:
            if 0 <= i <= top:
                assert (i * m) >> (31 + l) == i // d, (i, d)


def test_arguments_are_refused_before_the_device_is_touched():
    from event_utils_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)                            # never dereferenced: every call below is refused first
    einval, nan, inf = -1, float("nan"), float("inf")

    def votes(kind=_lib.EVK_T_F32, xs=fake, ys=fake, n=2048, packet_size=1024, packets=fake, n_packets=2, depths=fake, inv=fake, nd=4,
              fx=60.0, fy=60.0, cx=32.0, cy=24.0, h=48, w=64, mode=0, chunks=0, rays=fake, raw=fake):
        return L.evk_emvs_votes(kind, xs, ys, n, packet_size, packets, n_packets, depths, inv, nd, fx, fy, cx, cy, h, w, mode, chunks,
                                rays, raw, None)
    for missing in ("xs", "ys", "packets", "depths", "inv", "rays", "raw"):
        assert votes(**{missing: None}) == einval, missing
    assert votes(kind=2) == einval and votes(kind=-1) == einval
    assert votes(nd=0) == einval and votes(nd=-3) == einval
    assert votes(h=0) == einval and votes(w=0) == einval and votes(h=-1) == einval
    assert votes(h=1 << 16, w=1 << 15) == einval            # H * W past 2^31 - 1
    assert votes(h=1 << 15, w=1 << 15, nd=1 << 11) == einval
    assert votes(mode=2) == einval and votes(mode=-1) == einval
    assert votes(packet_size=0) == einval and votes(packet_size=-5) == einval
    assert votes(n=-1) == einval and votes(n=1 << 31, n_packets=1 << 21) == einval
    assert votes(n=1 << 24, n_packets=1 << 14, mode=1) == einval
    assert votes(n_packets=3) == einval and votes(n_packets=1) == einval
    assert votes(packet_size=1 << 40, n_packets=2) == einval           # one packet: the size is clamped to n
    assert votes(chunks=-1) == einval and votes(chunks=65536) == einval
    for bad in (0.0, -1.0, nan, inf):
        assert votes(fx=bad) == einval and votes(fy=bad) == einval
    for bad in (nan, inf, -inf):
        assert votes(cx=bad) == einval and votes(cy=bad) == einval

    def times(kind=_lib.EVK_T_F64, ts=fake, n=100, packet_size=10, out=fake):
        return L.evk_emvs_packet_times(kind, ts, n, packet_size, out, None)
    assert times(kind=3) == einval and times(ts=None) == einval and times(out=None) == einval
    assert times(n=-1) == einval and times(n=1 << 31) == einval and times(packet_size=0) == einval
    assert times(n=0, ts=None, out=None) == 0               # nothing to do

    def dmap(raw=fake, depths=fake, nd=4, h=48, w=64, radius=2, threshold=5, median=3, conf=fake, peak=fake, mask=fake, index=fake,
             depth=fake):
        return L.evk_emvs_depth_map(raw, depths, nd, h, w, radius, threshold, median, conf, peak, mask, index, depth, None)
    for missing in ("raw", "depths", "conf", "peak", "mask", "index", "depth"):
        assert dmap(**{missing: None}) == einval, missing
    assert dmap(nd=0) == einval and dmap(h=0) == einval and dmap(w=-2) == einval and dmap(h=1 << 16, w=1 << 15) == einval
    assert dmap(radius=-1) == einval and dmap(radius=17) == einval
    assert dmap(threshold=-1) == einval and dmap(threshold=(1 << 45) + 1) == einval
    for bad in (1, 2, 4, 7, -3):
        assert dmap(median=bad) == einval
    for f in (L.evk_emvs_band_rows, L.evk_emvs_band_cols):
        assert f(0, 5) == einval and f(5, 0) == einval and f(1 << 16, 1 << 15) == einval
    assert L.evk_emvs_chunks(-1, 1, 8, 8) == einval and L.evk_emvs_chunks(1 << 31, 1, 8, 8) == einval
    assert L.evk_emvs_chunks(10, 0, 8, 8) == einval


class _Column:
    """a column that only has a length: whatever reads its values fails"""

    def __init__(self, n):
        self.shape = (n,)

    def __len__(self):
        return self.shape[0]


def test_python_argument_errors_come_before_any_device_work():
    """every call below is refused on its arguments alone: none of them reaches the point where a missing GPU would matter"""
    import torch
    import event_utils_amd as E
    sc = N.scene(points_per_plane=2, n_poses=5)

    def bad(match, xs=sc["xs"], ys=sc["ys"], ts=sc["ts"], **kw):
        args = dict(camera_matrix=N.SCENE_K, pose_ts=sc["pose_ts"], positions=sc["positions"], quaternions=sc["quaternions"],
                    reference_pose=N.SCENE_REFERENCE, depths=sc["depths"], sensor_size=N.SCENE_SIZE)
        args.update(kw)
        for f in (E.dsi_votes, E.emvs_depth_map):
            with pytest.raises(ValueError, match=match):
                f(xs, ys, ts, None, **args)
    bad("voting", voting="cubic")
    bad("3x3", camera_matrix=np.eye(4))
    bad("no skew", camera_matrix=np.array([[60.0, 0.5, 32.0], [0.0, 60.0, 24.0], [0.0, 0.0, 1.0]]))
    bad("fx > 0", camera_matrix=np.diag([-60.0, 60.0, 1.0]))
    bad("reference_camera_matrix", reference_camera_matrix=np.eye(2))
    bad("strictly increasing", pose_ts=sc["pose_ts"][::-1])
    bad("positions", positions=sc["positions"][:-1])
    bad("quaternions", quaternions=np.zeros((5, 4)))
    bad("quaternions", quaternions=sc["quaternions"][:, :3])
    bad("reference_pose", reference_pose=np.zeros(7))
    bad("reference_pose", reference_pose=(np.zeros(3), np.zeros(4)))
    for depths in ([], [1.0, 0.0], [1.0, -2.0], [float("nan")], [float("inf")]):
        bad("depths", depths=depths)
    bad("sensor_size", sensor_size=(0, 64))
    bad("dsi_size", dsi_size=(48, -1))
    bad("dsi_size", dsi_size=(1 << 16, 1 << 15))
    bad("dsi_size", dsi_size=(48,))
    bad("2\\^40", dsi_size=(1 << 15, 1 << 15), depths=np.full(1 << 11, 1.0))
    for packet_size in (0, -1, 2.5):
        bad("packet_size", packet_size=packet_size)
    bad("differ in length", ys=sc["ys"][:-1])
    bad("are needed", ys=None)
    big = _Column(1 << 31)
    bad("fewer than 2\\^31", xs=big, ys=big, ts=big)
    wide = _Column(1 << 24)
    bad("fewer than 2\\^24", xs=wide, ys=wide, ts=wide, voting="bilinear")
    dsi = E.DSI(torch.zeros((4, 6, 5), dtype=torch.int32), 1, np.arange(1.0, 5.0))
    for kw, match in ((dict(filter_radius=-1), "filter_radius"), (dict(filter_radius=17), "filter_radius"),
                      (dict(filter_radius=1.5), "filter_radius"), (dict(median_size=4), "median_size"), (dict(median_size=7), "median_size"),
                      (dict(threshold=-0.5), "threshold"), (dict(threshold=float("nan")), "threshold"),
                      (dict(threshold=float("inf")), "threshold")):
        with pytest.raises(ValueError, match=match):
            E.dsi_depth_map(dsi, **kw)
    for broken, match in ((E.DSI(dsi.raw, 1, np.arange(1.0, 4.0)), "dsi.raw"), (E.DSI(dsi.raw[0], 1, dsi.depths), "dsi.raw"),
                          (E.DSI(dsi.raw.to(torch.int64), 1, dsi.depths), "dsi.raw"), (E.DSI(dsi.raw, 0, dsi.depths), "scale"),
                          (E.DSI(dsi.raw, 1, [1.0, 2.0, -1.0, 3.0]), "depths"), ((dsi.raw, 1), "DSI")):
        with pytest.raises(ValueError, match=match):
            E.dsi_depth_map(broken)
    with pytest.raises(ValueError, match="packet_size"):
        E.packet_times(sc["xs"], sc["ys"], sc["ts"], None, packet_size=0)


def test_the_result_objects():
    import torch
    import event_utils_amd as E
    raw = torch.tensor([[[0, 256, -256]]], dtype=torch.int32)         # (-256: the uint32 cell 2^32 - 256)
    dsi = E.DSI(raw, 256, np.array([1.0]))
    assert dsi.votes().dtype == torch.float32 and dsi.votes().tolist() == [[[0.0, 1.0, 16777215.0]]]
    assert dsi.raw is raw and dsi.scale == 256 and tuple(dsi) == (raw, 256, dsi.depths)
    # depth_to_points on a host map: X = c_ref + R_ref (Z K^-1 (x, y, 1)), row-major pixel order
    depth = np.full((3, 4), np.nan)
    depth[0, 1], depth[2, 3] = 2.0, 4.0
    dm = E.DepthMap(depth, None, None, ~np.isnan(depth))
    ref = (np.array([1.0, -2.0, 0.5]), quat_y(math.pi / 2))
    points = E.depth_to_points(dm, K64, ref)
    want = np.stack([ref[0] + rot_y(math.pi / 2) @ (z * (KINV64 @ np.array([x, y, 1.0]))) for x, y, z in ((1, 0, 2.0), (3, 2, 4.0))])
    assert isinstance(points, np.ndarray) and points.shape == (2, 3) and np.abs(points - want).max() < 1e-12
    assert E.depth_to_points(E.DepthMap(np.full((2, 2), np.nan), None, None, np.zeros((2, 2), bool)), K64, ref).shape == (0, 3)


def test_the_kernels_compile_without_register_spills(tmp_path):
    """every kernel of evk_emvs.hip compiles for gfx950 without spilling registers; the vote kernels keep no scratch at all"""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    from event_utils_amd.csrc import build as B
    assert "-ffp-contract=off" in B.CFLAGS and not any("fast-math" in f for f in B.CFLAGS)      # one rounding per operation
    src = os.path.join(B.HERE, "evk_emvs.hip")
    subprocess.run([hipcc] + list(B.CFLAGS) + ["-c", src, "-o", str(tmp_path / "emvs.o"), "-save-temps=obj"], check=True, cwd=B.HERE,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert asm, os.listdir(tmp_path)
    text = open(tmp_path / asm[0]).read()
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    seen = {n: (int(v), int(sp)) for n, v, sp in kernels}
    for name, count in (("k_emvs_packet_times", 2), ("k_emvs_rays", 2), ("k_emvs_votes", 2), ("k_emvs_peak", 1), ("k_emvs_mask", 1),
                        ("k_emvs_median", 3)):
        assert sum(name in n for n in seen) == count, (name, sorted(seen))
    assert not {n: vs for n, vs in seen.items() if vs[1]}
    assert all(v <= 128 for n, (v, _) in seen.items() if "k_emvs_votes" in n)                   # 1024 threads: 16 waves on a CU
