"""CPU: what the generators of the fuzz kinds motion8 and zhu (tools/fuzz_parity.py) cover over exactly the seeds of the GPU
slice (tests/test_gpu_fuzz.py), from the generators and the numpy restatements alone: every class is drawn, most cases put
most of their events on the canvas (a case with every event off it compares zeros with zeros), most zhu cases have a loss
and a gradient to compare, few carry injected non-finite inputs, and the angular-velocity cases that aim behind the camera
get there.  The only library calls are the host-only band geometry entries."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))


def _fuzz():
    argv, sys.argv = sys.argv, sys.argv[:1]
    try:
        import fuzz_parity as F
    finally:
        sys.argv = argv
    return F


def _slice(kind):
    """(seed0, cases) of `kind` in the parametrisation of tests/test_gpu_fuzz.py, read from its source (importing it would
    need nothing more, but its module-level mark is for the GPU run)."""
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_fuzz.py")).read()
    m = re.search(r'\("%s", (\d+), (\d+)\)' % kind, src)
    assert m, kind
    return int(m.group(1)), int(m.group(2))


def _rngs(kind):
    seed0, cases = _slice(kind)
    return [np.random.default_rng(910_000 + seed) for seed in range(seed0, seed0 + cases)]


def _finite(c):
    xr, yr, tr, pr = c["plan"]["ref"]
    with np.errstate(all="ignore"):
        return np.isfinite(xr) & np.isfinite(yr) & np.isfinite(np.asarray(tr, np.float64)) & np.isfinite(np.asarray(pr, np.float64) * c["scale"])


def _drawn(cases, key, values):
    seen = {c[key] for c in cases}
    assert seen >= set(values), "%s: never drawn: %s" % (key, sorted(set(values) - seen, key=str))


@pytest.fixture(scope="module")
def motion8_cases():
    F = _fuzz()
    return F, [F.motion8_inputs(rng) for rng in _rngs("motion8")]


@pytest.fixture(scope="module")
def zhu_cases():
    F = _fuzz()
    cases = [F.zhu_inputs(rng) for rng in _rngs("zhu")]
    return F, cases, [F.zhu_reference(c) for c in cases]


def test_motion8_generator_draws_every_class(motion8_cases):
    F, cases = motion8_cases
    M = F._t("_motion_models8_np")
    _drawn(cases, "model", [M.ANGVEL, M.PLANAR])
    _drawn(cases, "kind", F.COLUMN_KINDS)
    _drawn(cases, "geo", ["random", "at", "over", "under", "one_row"])
    _drawn(cases, "impl", ["auto", "direct"])
    _drawn(cases, "scale", [1.0, 100.0, 0.5, -1.0])
    _drawn(cases, "aim", ["behind", "front", "none"])
    _drawn(cases, "exact_blur", [False, True])
    _drawn(cases, "other", ["sos", "rms"])
    for key in ("grad", "pol"):
        _drawn(cases, key, [False, True])
    assert any(c["img_size"] != c["ss"] for c in cases) and any(c["img_size"] == c["ss"] for c in cases)
    assert any(c["planes"] == 9 and c["geo"] != "random" for c in cases)          # the band cap at 9 planes
    assert sum(c["bad"] for c in cases) <= 0.15 * len(cases)
    # intrinsics: fx != fy everywhere, the principal point off the sensor somewhere
    av = [c for c in cases if c["model"] == M.ANGVEL]
    assert all(c["K"][0, 0] != c["K"][1, 1] for c in av)
    assert any(not (0 <= c["K"][0, 2] <= c["ss"][1] and 0 <= c["K"][1, 2] <= c["ss"][0]) for c in av)
    # planar parameters: all-zero and large linear terms
    pf = [c for c in cases if c["model"] == M.PLANAR]
    assert any(not c["q"].any() for c in pf) and any(np.abs(c["q"][[1, 2, 4, 5]]).max() * 1.0 > 0.5 for c in pf)


def test_motion8_cases_put_their_events_on_the_canvas(motion8_cases):
    F, cases = motion8_cases
    M = F._t("_motion_models8_np")
    on, behind = [], []
    for c in cases:
        xr, yr, tr, pr = c["plan"]["ref"]
        tr, fin = np.asarray(tr, np.float64), _finite(c)
        with np.errstate(all="ignore"):
            ones, _ = M.iwe(c["model"], c["q"], xr, yr, tr, np.ones(len(tr)), c["img_size"], c["ss"], use_polarity=False,
                            compute_gradient=False, center=c["center"], camera_matrix=c["K"])
            on.append(ones.sum() > 0.5 * fin.sum())
            if c["aim"] == "behind":
                xw = M.warp(c["model"], xr, yr, tr, float(tr[-1]), c["q"], c["center"], c["K"])[0]
                behind.append(bool(np.isnan(xw[fin]).any()))
    assert np.mean(on) >= 0.7, np.mean(on)
    assert len(behind) >= 4 and np.mean(behind) >= 0.25, behind


def test_zhu_generator_draws_every_class(zhu_cases):
    F, cases, _ = zhu_cases
    Z = F._t("_zhu_np")
    _drawn(cases, "model", Z.MODELS)
    _drawn(cases, "route", ["fused", "plugin"])
    _drawn(cases, "kind", F.COLUMN_KINDS)
    _drawn(cases, "tk", ["sorted", "const", "few", "ends", "unsorted"])
    _drawn(cases, "pk", ["pm1", "pos", "neg", "pm1z", "ints", "nan"])
    _drawn(cases, "sigma", F.ZHU_SIGMAS)
    _drawn(cases, "scale", F.ZHU_SCALES)
    _drawn(cases, "geo", ["random", "at", "over", "under", "one_row", "one_row_fits", "no_row_fits"])
    _drawn(cases, "tref_mode", ["none", "inside", "outside"])
    _drawn(cases, "size_mode", ["equal", "img_smaller", "img_larger"])
    _drawn(cases, "impl", ["auto", "direct"])
    # band and direct canvases, by the library's own geometry
    from event_utils_amd import _lib
    rows = [_lib.lib().evk_tsimg_band_rows(0, c["ss"][0] + 1, c["ss"][1] + 1) for c in cases]
    assert any(r > 0 for r in rows) and any(r == 0 for r in rows)
    # the plugin on numpy columns and on a DeviceEvents; the branches that subtract a time offset from .t_ref
    plug = [c for c in cases if c["route"] == "plugin"]
    assert any(c["kind"] == "numpy" and c["scale"] == 1.0 for c in plug) and any(c["kind"] != "numpy" or c["scale"] != 1.0 for c in plug)
    assert any(c["t_ref"] is not None and c["plan"]["t_offset"] != 0.0 for c in cases)
    # float64 device columns with absolute epoch stamps, with and without .t_ref
    assert any(c["epoch"] and not c["plan"]["f32"] and c["t_ref"] is None for c in cases)
    assert any(c["epoch"] and not c["plan"]["f32"] and c["t_ref"] is not None for c in cases)
    assert any(min(c["ss"]) + 1 < 8 and (c["sigma"] is None or c["sigma"] >= 2.0) for c in cases)     # canvas below the blur radius
    assert sum(c["bad"] for c in cases) <= 0.15 * len(cases)


def test_zhu_cases_have_something_to_compare(zhu_cases):
    F, cases, refs = zhu_cases
    on = [r["counted"] > 0.5 * _finite(c).sum() for c, r in zip(cases, refs)]
    assert np.mean(on) >= 0.7, np.mean(on)
    nonzero = [r["loss"] != 0.0 and np.abs(r["grad"]).max() > 0.0 for r in refs]
    assert np.mean(nonzero) >= 0.7, np.mean(nonzero)
    assert all(np.isfinite(r["loss"]) and np.isfinite(r["grad"]).all() and np.isfinite(r["planes"]).all() for r in refs)


def test_zhu_time_stamps_stay_in_the_fixed_point_range(zhu_cases):
    """|tau| <= ZHU_TAU_BOUND for every finite time stamp of every case, the unsorted kind with its four end placements included."""
    F, cases, _ = zhu_cases
    _drawn([c for c in cases if c["tk"] == "unsorted" and c["n"] >= 2], "ends", ["minmax", "beyond", "reversed", "inside"])
    for c in cases:
        t = np.asarray(c["plan"]["ref"][2], np.float64)
        if len(t):
            with np.errstate(all="ignore"):
                tau = (t - t[0]) / (t[-1] - t[0] + 1e-6)
            assert np.isfinite(t[0]) and np.isfinite(t[-1]) and np.nanmax(np.abs(tau[np.isfinite(tau)]), initial=0.0) <= F.ZHU_TAU_BOUND, c["desc"]


def test_zhu_integer_pixels_reach_the_image_border_with_zero_flow(zhu_cases):
    """Events exactly on x' = W or y' = H of an image smaller than the canvas are counted (x' <= W): drawn, with zero flow."""
    F, cases, _ = zhu_cases
    Z = F._t("_zhu_np")
    hit = 0
    for c in cases:
        if c["size_mode"] == "img_smaller" and c["route"] == "fused" and c["model"] in (Z.LINVEL, Z.PLANAR, Z.XYZTHETA) and \
                not np.asarray(c["q"]).any() and c["scale"] != 0.0 and c["tk"] != "const":
            xr, yr = c["plan"]["ref"][:2]
            hit += bool(np.any((xr == c["img_size"][1]) & (yr > 0) & (yr < c["img_size"][0])))
    assert hit >= 1
