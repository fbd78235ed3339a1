"""Timings of event-based multi-view stereo (event_utils_amd.depth.emvs; evk_emvs.hip): dsi_votes with nearest and bilinear voting
and dsi_depth_map, at 10 M events on 240x180 with 100 planes and at 1 M events on 346x260 with 64 planes.  The events are the
projections of random scene points at depths 1 .. 3 seen from a translating, slowly turning camera, as float32 resident columns
(a DeviceEvents).  Per case: the vote entry alone on a prepared packet table (the ray pass and the vote kernel), the ray pass with a
1 x 1 x 1 volume (what is left when there is nothing to vote into), the public call end to end (with the read-back of the packet
times and the host's packet table), the depth map, and for scale one events_to_voxel_torch call on the same events.  Beside the vote
times stand event-planes per second (N D over the time), votes per second (cell increments that landed) and the bounds of the sizing
note in DESIGN.md section 6, computed here from the shapes: float64 operations at the vector rate without FMA, LDS adds at one
wave-instruction per four cycles per CU.  Neither rate is measured by this tool; the LDS add rate is not in MI355X_MICROARCH.md
either and is taken to be that of a 4-byte LDS store.  Every timed repetition synchronises before and after; the median is reported.
No time here is a pass / fail criterion.
usage: timeout 900 python tools/emvs_time.py [--quick] [--out profiles/emvs_time.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (("10 M events, 240x180, D = 100", 10_000_000, (180, 240), 100), ("1 M events, 346x260, D = 64", 1_000_000, (260, 346), 64))
PACKET = 1024
CUS, CLOCK = 256, 2.4e9
F64_OPS_PER_CLK_CU = 64.0                   # 4 SIMDs x 16 lanes, one add or multiply per lane and clock (no FMA: -ffp-contract=off)
LDS_ADDS_PER_CLK_CU = 16.0                  # one 64-lane ds_add_u32 per 4 clocks, taken from ds_write_b32 (not measured)
F64_OPS_PER_EVENT_PLANE = 16.0              # s, 2 x (mul add mul mul add), 2 x (add floor), range compares and conversions aside
F64_OPS_PER_RAY = 40.0                      # 9 multiply-adds and two divisions (~12 operations each)


def scene(n, size, seed=0):
    """about n events (x, y float32, t float64, stream order = time order), the trajectory and the camera matrix"""
    rng = np.random.default_rng(seed)
    h, w = size
    f = 0.8 * w
    K = np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])
    points = 4000
    n_poses = -(-n // points) + 1
    z = rng.uniform(1.0, 3.0, points)
    world = np.stack((rng.uniform(-0.2, w + 0.2, points) - w / 2.0, rng.uniform(-0.2, h + 0.2, points) - h / 2.0, np.full(points, f)),
                     axis=0) / f * z
    pose_ts = np.linspace(0.0, 1.0, n_poses)
    positions = np.stack((-0.2 + 0.4 * pose_ts, 0.03 * np.sin(5 * pose_ts), np.zeros(n_poses)), axis=1)
    angle = 0.06 * (pose_ts - 0.5)
    quats = np.stack((np.zeros(n_poses), np.sin(angle / 2), np.zeros(n_poses), np.cos(angle / 2)), axis=1)
    xs, ys, ts = [], [], []
    for t, c, a in zip(pose_ts, positions, angle):
        ca, sa = np.cos(a), np.sin(a)
        d = world - c[:, None]
        cam = np.stack((ca * d[0] - sa * d[2], d[1], sa * d[0] + ca * d[2]))          # R_y(a)^T (X - c)
        u, v = np.rint(f * cam[0] / cam[2] + w / 2.0), np.rint(f * cam[1] / cam[2] + h / 2.0)
        vis = (u >= 0) & (u < w) & (v >= 0) & (v < h)
        xs.append(u[vis].astype(np.float32)), ys.append(v[vis].astype(np.float32)), ts.append(np.full(int(vis.sum()), t))
    xs, ys, ts = (np.concatenate(v)[:n] for v in (xs, ys, ts))
    return xs, ys, ts, pose_ts, positions, quats, K


def main():
    import torch
    import event_utils_amd as E
    from event_utils_amd import _device as D
    from event_utils_amd import _lib
    quick = "--quick" in sys.argv
    reps = 3 if quick else 9
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "emvs_time.txt")

    def median_ms(fn, reps=reps):
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return float(np.median(ts))

    class Lines(list):
        def append(self, line):
            print(line, flush=True)
            list.append(self, line)

    dev = D.require_gpu()
    L = _lib.lib()
    lines = Lines()
    lines.append("EMVS timings: float32 resident columns, packets of %d events, depths uniform in inverse depth 0.7 .. 5, reference = the "
                 "middle pose; median of %d; %s" % (PACKET, reps, torch.cuda.get_device_name(0)))
    reference = (np.zeros(3), np.array([0.0, 0.0, 0.0, 1.0]))
    for title, n, size, nd in CASES:
        if quick:
            n //= 20
        h, w = size
        xs, ys, ts, pose_ts, positions, quats, K = scene(n, size)
        n = len(ts)
        depths = E.depth_planes(0.7, 5.0, nd)
        ev = E.DeviceEvents.from_arrays(xs, ys, ts.astype(np.float32), np.ones(n, dtype=np.float32), precision="f32")
        traj = dict(camera_matrix=K, pose_ts=pose_ts, positions=positions, quaternions=quats, reference_pose=reference, depths=depths,
                    sensor_size=size, packet_size=PACKET)
        rows, cols = L.evk_emvs_band_rows(h, w), L.evk_emvs_band_cols(h, w)
        tiles = -(-h // rows) * -(-w // cols)
        chunks = L.evk_emvs_chunks(n, nd, h, w)
        lines.append("")
        lines.append("%s (%d events): tiles of %d x %d cells (%d per plane, %d B of LDS), %d event chunks, %d workgroups; DSI %.1f MB"
                     % (title, n, rows, cols, tiles, 4 * rows * cols, chunks, nd * tiles * chunks, 4 * nd * h * w / 1e6))
        table = torch.from_numpy(E.packet_transforms(E.packet_times(ev, None, None, None, PACKET), pose_ts, positions, quats, K,
                                                     reference)).to(dev)
        planes = torch.from_numpy(np.stack((depths, 1.0 / depths))).to(dev)
        rays = torch.empty((n, 2), dtype=torch.float64, device=dev)
        raw = torch.empty((nd, h, w), dtype=torch.int32, device=dev)
        one = torch.empty((1, 1, 1), dtype=torch.int32, device=dev)
        stream = D.stream()
        intr = (float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2]))

        def entry(mode, out=raw, planes_used=nd, hh=h, ww=w, forced=0):
            _lib.call("evk_emvs_votes", _lib.EVK_T_F32, D.ptr(ev.x), D.ptr(ev.y), n, PACKET, D.ptr(table), table.shape[0], D.ptr(planes[0]),
                      D.ptr(planes[1]), planes_used, *intr, hh, ww, mode, forced, D.ptr(rays), D.ptr(out), stream)

        def row(name, ms, extra=""):
            lines.append("%-58s %9.3f ms%s" % (name, ms, extra))
            return ms
        t_rays = row("ray pass and a 1 x 1 x 1 volume (evk_emvs_votes)", median_ms(lambda: entry(0, one, 1, 1, 1)))
        ray_bound = n * F64_OPS_PER_RAY / (F64_OPS_PER_CLK_CU * CUS * CLOCK) * 1e3
        lines.append("    bound: %.3f ms of float64 operations (%d per ray), %.3f ms to move 8 + 16 B per event at 4 TB/s"
                     % (ray_bound, F64_OPS_PER_RAY, n * 24 / 4e12 * 1e3))
        dsis = {}
        for voting, (mode, scale) in (("nearest", (0, 1)), ("bilinear", (1, 256))):
            entry(mode)
            once = raw.clone()
            entry(mode, forced=1)
            assert torch.equal(raw, once), "the DSI depends on the event chunks"
            landed = float((raw.to(torch.int64) & 0xFFFFFFFF).sum()) / scale
            cell_adds = landed * (1 if mode == 0 else 4)
            ms = row("vote entry, %s (evk_emvs_votes: rays + votes)" % voting, median_ms(lambda: entry(mode)))
            work = float(n) * nd
            f64_bound = work * tiles * F64_OPS_PER_EVENT_PLANE / (F64_OPS_PER_CLK_CU * CUS * CLOCK) * 1e3
            lds_bound = cell_adds / (LDS_ADDS_PER_CLK_CU * CUS * CLOCK) * 1e3
            lines.append("    %.1f G event-planes / s, %.1f G votes / s (%.3g votes landed, %.2f of N D)"
                         % (work / ms / 1e6, landed / ms / 1e6, landed, landed / work))
            lines.append("    bounds: %.3f ms of float64 operations (%d per event-plane, every event seen by each of the %d tiles of a "
                         "plane), %.3f ms of LDS adds (rate not measured), %.3f ms to read the rays once per workgroup row at 4 TB/s"
                         % (f64_bound, F64_OPS_PER_EVENT_PLANE, tiles, lds_bound, work * tiles * 16 / 4e12 * 1e3))
            row("  one event chunk instead of %d" % chunks, median_ms(lambda: entry(mode, forced=1)))
            row("dsi_votes, %s (end to end: packet times, host table, entry)" % voting,
                median_ms(lambda: E.dsi_votes(ev, None, None, None, voting=voting, **traj)))
            dsis[voting] = E.dsi_votes(ev, None, None, None, voting=voting, **traj)
            assert torch.equal(dsis[voting].raw, once)
        for voting, dsi in dsis.items():
            ms = median_ms(lambda: E.dsi_depth_map(dsi, 2, 5.0, 3))
            row("dsi_depth_map, %s DSI (radius 2, median 3)" % voting, ms,
                "   %8.1f MB to read, %6.0f GB/s" % (4 * nd * h * w / 1e6, 4 * nd * h * w / 1e6 / ms))
            dm = E.dsi_depth_map(dsi, 2, 5.0, 3)
            lines.append("    %d of %d pixels masked in" % (int(dm.mask.sum()), h * w))
        row("events_to_voxel_torch, 5 bins, the same events (for scale)",
            median_ms(lambda: E.events_to_voxel_torch(ev.x, ev.y, ev.t, ev.p, 5, sensor_size=size)))
        del ev, rays, raw, table
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
