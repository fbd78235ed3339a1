"""Timings of depth fusion (event_utils_amd.depth.fusion; evk_fusion.hip) at 640x480 with 16 views and about 15 % valid pixels: the
four steps of a fusion on resident buffers -- propagate (with its compaction), group, fuse, regularise -- each on its own, and the
whole public calls.  The views see a slanted plane from poses a few centimetres and a degree apart, with inverse-depth noise.  The
yardstick is the same steps written in torch on the same device in float64, what a user would write without the kernels: the
propagation as tensor arithmetic and a boolean selection, the grouping as a stable sort of pixel keys, the fusion as segment
reductions over the sorted candidates (scatter_reduce for the anchor, index_add_ for the sums: atomics, so its sums are NOT
reproducible bit for bit, which is why the library does not do it this way; its result is compared with the kernel's) and the
regularisation as (2 r + 1)^2 shifted copies of the map.  Every timed repetition runs CALLS calls between two synchronisations;
the median per call is reported.  No time here is a pass / fail criterion.
usage: timeout 900 python tools/fusion_time.py [--quick] [--out profiles/depth_fusion_time.txt]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SIZE = (480, 640)
INTRINSICS = (520.0, 520.0, 319.5, 239.5)
VIEWS, FRACTION, SIGMA_RHO = 16, 0.15, 0.004
GATE, RADIUS, MIN_NEIGHBOURS, CALLS = 2.0, 1, 2, 200


def camera():
    fx, fy, cx, cy = INTRINSICS
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


def scene(seed=0):
    """VIEWS maps of the plane Z = 3 + 0.4 X + 0.2 Y (in the target's frame), each from its own pose -> (rho, var, mask) stacked
    (V, H, W) numpy arrays and the (V, 12) target-from-source transforms"""
    import _fusion_np as N
    rng = np.random.default_rng(seed)
    h, w = SIZE
    fx, fy, cx, cy = INTRINSICS
    n, c = np.array([-0.4, -0.2, 1.0]), 3.0
    ys, xs = np.mgrid[0:h, 0:w]
    rays = np.stack(((xs - cx) / fx, (ys - cy) / fy, np.ones(SIZE)), axis=-1)
    rho, var, mask, T = [], [], [], []
    for s in range(VIEWS):
        R = N.rodrigues(rng.normal(size=3) * (0.01 if s else 0.0))
        t = rng.normal(size=3) * (0.03 if s else 0.0)
        Z = (c - n @ t) / (rays @ (R.T @ n))
        m = rng.random(SIZE) < FRACTION
        rho.append(np.where(m, 1.0 / Z + rng.normal(size=SIZE) * SIGMA_RHO, np.nan))
        var.append(np.where(m, SIGMA_RHO ** 2, np.nan))
        mask.append(m)
        T.append(N.transform12(R, t))
    return np.stack(rho), np.stack(var), np.stack(mask), np.array(T)


# ---- the same steps in torch -----------------------------------------------------------------------------------------------------

def torch_propagate(rho, var, mask, T, size):
    import torch
    fx, fy, cx, cy = INTRINSICS
    v, h, w = rho.shape
    ys, xs = torch.meshgrid(torch.arange(h, device=rho.device, dtype=torch.float64), torch.arange(w, device=rho.device, dtype=torch.float64),
                            indexing="ij")
    src = mask & torch.isfinite(rho) & (rho > 0) & torch.isfinite(var) & (var > 0)
    Z = 1.0 / rho
    X, Y = (xs - cx) / fx * Z, (ys - cy) / fy * Z
    R, t = T[:, :9].reshape(v, 3, 3, 1, 1), T[:, 9:].reshape(v, 3, 1, 1)
    Xp, Yp, Zp = (R[:, i, 0] * X + R[:, i, 1] * Y + R[:, i, 2] * Z + t[:, i] for i in range(3))
    rp = 1.0 / Zp
    xi, yi = torch.floor(fx * (Xp / Zp) + cx + 0.5), torch.floor(fy * (Yp / Zp) + cy + 0.5)
    q2 = (rp / rho) ** 2
    vp = q2 * q2 * var
    keep = src & (Zp > 0) & torch.isfinite(Xp) & torch.isfinite(Yp) & torch.isfinite(Zp) & (xi >= 0) & (xi < size[1]) & (yi >= 0) & \
        (yi < size[0]) & torch.isfinite(vp)
    return xi[keep].to(torch.int32), yi[keep].to(torch.int32), rp[keep], vp[keep]


def torch_group(xi, yi, size):
    """-> (the candidates' order by pixel, stable; the sorted pixel keys)"""
    import torch
    key = yi.to(torch.int64) * size[1] + xi.to(torch.int64)
    skey, order = torch.sort(key, stable=True)
    return order, skey


def torch_fuse(order, skey, rho, var, size, gate2):
    import torch
    hw = size[0] * size[1]
    r, v = rho[order], var[order]
    pos = torch.arange(len(order), device=rho.device)
    vmin = torch.full((hw,), float("inf"), dtype=torch.float64, device=rho.device).scatter_reduce(0, skey, v, "amin")
    first = torch.full((hw,), len(order), dtype=torch.int64, device=rho.device).scatter_reduce(
        0, skey, torch.where(v == vmin[skey], pos, len(order)), "amin")
    a = first[skey]
    d = r - r[a]
    inl = (pos == a) | (d * d <= gate2 * (v + v[a]))
    iw = torch.where(inl, 1.0 / v, 0.0)
    W = torch.zeros(hw, dtype=torch.float64, device=rho.device).index_add_(0, skey, iw)
    S = torch.zeros(hw, dtype=torch.float64, device=rho.device).index_add_(0, skey, r * iw)
    count = torch.zeros(hw, dtype=torch.int32, device=rho.device).index_add_(0, skey, inl.to(torch.int32))
    total = torch.bincount(skey, minlength=hw).to(torch.int32)
    nan = torch.full_like(W, float("nan"))
    return (torch.where(count > 0, S / W, nan).reshape(size), torch.where(count > 0, 1.0 / W, nan).reshape(size), count.reshape(size),
            (total - count).reshape(size), (count >= 1).reshape(size))


def torch_regularise(rho, var, mask, radius, gate2, min_neighbours):
    import torch
    import torch.nn.functional as F
    h, w = rho.shape
    pr, pv, pm = (F.pad(a, (radius,) * 4) for a in (torch.nan_to_num(rho), torch.nan_to_num(var), mask.to(torch.uint8)))
    pm = pm.bool()
    W, S = torch.zeros_like(rho), torch.zeros_like(rho)
    n = torch.zeros(rho.shape, dtype=torch.int32, device=rho.device)
    for dy in range(2 * radius + 1):
        for dx in range(2 * radius + 1):
            rq, vq, mq = pr[dy:dy + h, dx:dx + w], pv[dy:dy + h, dx:dx + w], pm[dy:dy + h, dx:dx + w]
            d = rq - rho
            ok = mq & mask & (d * d <= gate2 * (vq + var))
            iw = torch.where(ok, 1.0 / vq, 0.0)
            W += iw
            S += torch.where(ok, rq, 0.0) * iw
            if (dy, dx) != (radius, radius):
                n += ok
    return torch.where(mask, S / W, rho), mask & (n >= min_neighbours)


def main():
    import torch
    import event_utils_amd as E
    from event_utils_amd import _device as D
    from event_utils_amd import _lib
    quick = "--quick" in sys.argv
    reps = 3 if quick else 9
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "depth_fusion_time.txt")
    K = camera()
    h, w = SIZE

    def median_ms(fn, calls=CALLS):
        fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 / calls)
        return float(np.median(ts))

    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def row(name, ms, extra=""):
        say("%-86s %9.4f ms%s" % (name, ms, extra))
        return ms

    rho_n, var_n, mask_n, T = scene()
    rho, var, mask = (torch.from_numpy(a).cuda() for a in (rho_n, var_n, mask_n))
    mask8 = mask.to(torch.uint8)
    maps = [E.InverseDepthMap(rho[s], var[s], mask[s].to(torch.int32), torch.zeros(SIZE, dtype=torch.int32, device="cuda"), mask[s])
            for s in range(VIEWS)]
    n = VIEWS * h * w
    L = _lib.lib()
    nbytes = int(L.evk_fusion_scratch_bytes(VIEWS, h, w, h, w))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    xi, yi = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    crho, cvar = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(2))
    result = torch.zeros(3, dtype=torch.int64, device="cuda")
    params = np.empty((VIEWS, 17))
    params[:, :4], params[:, 4:16], params[:, 16] = INTRINSICS, T, 0.0
    target = np.array(INTRINSICS)
    gate2 = GATE * GATE

    def propagate():
        _lib.call("evk_fusion_propagate", D.ptr(rho), D.ptr(var), D.ptr(mask8), VIEWS, h, w, D.host_ptr(params), h, w, D.host_ptr(target),
                  D.ptr(scratch), D.ptr(xi), D.ptr(yi), D.ptr(crho), D.ptr(cvar), D.ptr(result), D.stream())
    propagate()
    m = int(result[0].item())

    def group():
        _lib.call("evk_denoise_group", D.ptr(xi), D.ptr(yi), None, m, h, w, 1, D.ptr(scratch), nbytes, None, D.stream())
    out_rho, out_var = (torch.empty(SIZE, dtype=torch.float64, device="cuda") for _ in range(2))
    out_count, out_rej = (torch.empty(SIZE, dtype=torch.int32, device="cuda") for _ in range(2))
    out_mask = torch.empty(SIZE, dtype=torch.uint8, device="cuda")

    def fuse():
        _lib.call("evk_fusion_fuse", m, h, w, D.ptr(scratch), D.ptr(crho), D.ptr(cvar), gate2, 1, 0, 0.0, D.ptr(out_rho), D.ptr(out_var),
                  D.ptr(out_count), D.ptr(out_rej), D.ptr(out_mask), D.stream())
    reg_rho, reg_mask = torch.empty_like(out_rho), torch.empty_like(out_mask)

    def regularise():
        _lib.call("evk_fusion_regularise", D.ptr(out_rho), D.ptr(out_var), D.ptr(out_mask), h, w, RADIUS, gate2, MIN_NEIGHBOURS, D.ptr(reg_rho),
                  D.ptr(reg_mask), D.stream())

    say("depth fusion timings: %d views of %d x %d, %.0f %% valid, gate %g, regularisation radius %d; median of %d repetitions of %d calls; %s"
        % (VIEWS, w, h, 100 * FRACTION, GATE, RADIUS, reps, CALLS, torch.cuda.get_device_name(0)))
    group(), fuse(), regularise()
    torch.cuda.synchronize()
    longest = int((out_count + out_rej).max())
    say("%d source pixels, %d candidates on %d of %d target pixels, the longest run %d; scratch %.1f MB"
        % (int(mask.sum()), m, int((out_count > 0).sum()), h * w, longest, nbytes / 1e6))
    say("")
    say("the library entries on resident buffers")
    k_p = row("  evk_fusion_propagate: %d (view, pixel) pairs, the four columns compacted in order" % n, median_ms(propagate))
    k_g = row("  evk_denoise_group: %d candidates by target pixel" % m, median_ms(group))
    k_f = row("  evk_fusion_fuse: one lane per target pixel, two walks over its run", median_ms(fuse))
    k_r = row("  evk_fusion_regularise: radius %d, a 32 x 8 tile and its halo in LDS" % RADIUS, median_ms(regularise))
    row("  the four together", k_p + k_g + k_f + k_r)
    say("the public calls (stacking the maps, the scratch and the outputs, the read-back of the count)")
    fused = E.fuse_inverse_depth(maps, K, T, gate=GATE)
    row("  fuse_inverse_depth", median_ms(lambda: E.fuse_inverse_depth(maps, K, T, gate=GATE)))
    row("  regularise_inverse_depth", median_ms(lambda: E.regularise_inverse_depth(fused, RADIUS, GATE, MIN_NEIGHBOURS)))
    again = E.fuse_inverse_depth(maps, K, T, gate=GATE)
    same = all(torch.equal(a.view(torch.int64) if a.dtype == torch.float64 else a, b.view(torch.int64) if b.dtype == torch.float64 else b)
               for a, b in zip(fused, again))
    say("  two calls give %s" % ("the same bits" if same else "DIFFERENT bits"))

    say("")
    say("yardstick: the same steps in torch on the device, float64")
    Td = torch.from_numpy(T).cuda()
    tc = torch_propagate(rho, var, mask, Td, SIZE)
    order, skey = torch_group(tc[0], tc[1], SIZE)
    tf = torch_fuse(order, skey, tc[2], tc[3], SIZE, gate2)
    tr = torch_regularise(tf[0], tf[1], tf[4], RADIUS, gate2, MIN_NEIGHBOURS)
    both = (out_count > 0) & (tf[2] > 0)
    say("  it gives the kernels' map: %d = %d candidates, counts %s, largest relative difference of inv_depth %.1e, regularised %.1e"
        % (len(tc[0]), m, "equal" if torch.equal(tf[2], out_count) else "DIFFERENT",
           float(((tf[0] - out_rho).abs() / out_rho.abs())[both].max()), float(((tr[0] - reg_rho).abs() / reg_rho.abs())[both].max())))
    t_p = row("  propagate: tensor arithmetic over (V, H, W) and a boolean selection", median_ms(lambda: torch_propagate(rho, var, mask, Td, SIZE)))
    t_g = row("  group: a stable sort of the pixel keys", median_ms(lambda: torch_group(tc[0], tc[1], SIZE)))
    t_f = row("  fuse: scatter_reduce for the anchor, index_add_ for the sums (atomics: not reproducible)",
              median_ms(lambda: torch_fuse(order, skey, tc[2], tc[3], SIZE, gate2)))
    t_r = row("  regularise: %d shifted copies" % (2 * RADIUS + 1) ** 2, median_ms(lambda: torch_regularise(tf[0], tf[1], tf[4], RADIUS, gate2,
                                                                                                    MIN_NEIGHBOURS)))
    row("  the four together", t_p + t_g + t_f + t_r)
    say("")
    say("torch / kernels: propagate %.1fx, group %.1fx, fuse %.1fx, regularise %.1fx, together %.1fx"
        % (t_p / k_p, t_g / k_g, t_f / k_f, t_r / k_r, (t_p + t_g + t_f + t_r) / (k_p + k_g + k_f + k_r)))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
