"""CPU: what the generators of the fuzz kinds motion8 and zhu (tools/fuzz_parity.py) cover over exactly the seeds of the GPU
slice (tests/test_gpu_fuzz.py), from the generators and the numpy restatements alone: every class is drawn, most cases put
most of their events on the canvas (a case with every event off it compares zeros with zeros), most zhu cases have a loss
and a gradient to compare, few carry injected non-finite inputs, and the angular-velocity cases that aim behind the camera
get there.  The only library calls are the host-only band geometry entries.

The same for the five kinds of the per-pixel grouping family (denoise, tsurf, corners, planeflow, reconstruct): the shared
stream generator draws every sensor, event-count, scene, time-stamp, polarity, column and select class; the crosses that the
dedicated GPU tests never make occur (a negative p_scale with a two-class mode, an integer time column with select, a sliced
column with a hot pixel, fractional stamps with an outlier threshold); most cases have something to compare; the plane-fit
cases can see rejection rounds and the order of a double sum; the runs straddle both wave thresholds, also on both sides of
the class boundary; no run reaches 2^14 events; no time stamp is non-finite (class (c) of profiles/fuzz_grouping_kinds.txt);
at most 15 % of the cases carry an injected invalid input.

The same for the two kinds that are compared bit for bit, emvs and simulate (profiles/fuzz_emvs_simulate.txt).  emvs: every class
of volume, plane, event count, coordinate, packet size, chunk count, trajectory, column kind and depth-map parameter is drawn; most
cases vote; planes are silent for some packets only, and one lies exactly on a camera centre; rays have d2 <= 0; bilinear corners
drop at a border while their neighbours land; the 'exact' cases (u == x, v == y, shown from the restatement) sit on every rounding
tie and border of both voting rules and on the ties of the bilinear weights; two planes tie for a pixel's maximum; most masks are
neither empty nor full and the median changes indices; the non-finite and huge coordinates are all there and the rest still votes.
simulate: every class of shape, frame time, amplitude, dtype, layout, input kind, contrast, refractory period and state is drawn;
most cases emit events, a quarter of those with equal-time neighbours, some in another than the (t, x, y, p) order; the refractory
period drops a part of the events; a shifted reference clamps events to frame_ts[0]; the key bits (sim_key_bits restated on the
host times) span the 8-bit floor, a middle range and all 64; the step limit overflows in the error cases only; streaming splits
have events exactly on the split time.  The only library calls are the host-only evk_emvs_band_rows / _band_cols / _chunks and
packet_transforms.

The same for the kernels that return gradients, flowts, flowcm and segment (profiles/fuzz_flow_segment.txt).  The flow kinds: every
class of field size and kind, batch, event count, offsets, position, time stamp, polarity, polarity factor, NaN, blur, direction and
objective is drawn, one value per axis; an empty sample stands at every place of a batch; events beside the field's support are
counted; tau stays in [0, 1] for every counted event; float32 stamps at 1e4 s tie and a span of 100 s absorbs the 1e-6 of tdiv; at
most 10 % of the cases have an identically zero reference gradient, and those are empty by design.  segment: all five models, 1 to
8 clusters, both column types, every canvas class as evk_seg_band_rows sees it (the only library call), every event count, every
residue of n mod 4 with several clusters, several chunks and several bands, bands of two and three rows whose events straddle the
band edge, zero rows of the associations, events that leave the canvas under some clusters only.

The same for raw, the EVT3 / EVT2 decoder (profiles/fuzz_raw.txt), from raw_inputs and the sequential restatement alone: every stream
family, word-count class, form of input and cut class is drawn in both formats where it applies, every time unit, policy, sensor and
initial-state kind; the restatement sees loops inside a piece and across a cut, steps back, events before and behind the first
TIME_HIGH of one call, events off the sensor under each policy, negative x and a base_x that wraps 2^16, chunks of more events than a
staging round (the 4096 of the kernel file) with lanes that straddle the round borders, a first TIME_HIGH in a late chunk, pieces
without a TIME_HIGH behind a state that has time; at most 15 % of the cases decode to nothing and every family that can emit has a
case of more than 1000 events."""
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


# ---- the per-pixel grouping family ---------------------------------------------------------------------------------------------

GROUP = ("denoise", "tsurf", "corners", "planeflow", "reconstruct")


@pytest.fixture(scope="module")
def group_cases():
    F = _fuzz()
    out = {}
    for kind in GROUP:
        cases = [getattr(F, kind + "_inputs")(rng) for rng in _rngs(kind)]
        with np.errstate(all="ignore"):
            refs = [None if c["bad"] is not None else getattr(F, kind + "_reference")(c) for c in cases]
        out[kind] = (cases, refs)
    return F, out


def _two(kind, c):
    """whether the case groups by two polarity classes somewhere"""
    return {"denoise": lambda: c["two"], "tsurf": lambda: True, "corners": lambda: c["polarity"] == "same",
            "planeflow": lambda: c["polarity"] == "same", "reconstruct": lambda: False}[kind]()


def _runs(F, c, two):
    s = c["s"]
    return np.bincount(F.group_keys(s, two), minlength=(2 if two else 1) * s["h"] * s["w"]) if s["n"] else np.zeros(1, np.int64)


@pytest.mark.parametrize("kind", GROUP)
def test_grouping_generators_draw_every_class(group_cases, kind):
    F, out = group_cases
    cases, _ = out[kind]
    _drawn(cases, "size_class", F.GROUP_SENSORS)
    _drawn(cases, "hw_mod", ["m1", "0", "p1", "other"])
    # (the 12 hot run lengths: in the two kinds with a wave path, test_runs_straddle_the_wave_thresholds, and in the family below)
    _drawn(cases, "n_class", F.N_GROUP_SMALL + F.N_GROUP_LARGE + ["hot"])
    _drawn(cases, "scene", F.GROUP_SCENES)
    _drawn(cases, "hot_place", F.HOT_PLACES)
    _drawn(cases, "tk", F.GROUP_TIMES)
    _drawn(cases, "pk", F.GROUP_POLS)
    _drawn(cases, "kind", F.GROUP_KINDS)
    _drawn(cases, "scale", F.GROUP_SCALES)
    _drawn(cases, "order", ["sorted", "unsorted"])
    valid = [c for c in cases if c["bad"] is None]
    if kind == "reconstruct":                              # ts must be non-decreasing: unsorted only as the expected ValueError
        assert all(c["order"] == "sorted" for c in valid)
    else:
        assert any(c["order"] == "unsorted" for c in valid)
    # ps=None where the docstring permits it: the one-class modes (tsurf: both polarity modes "ignore"; averaged_time_surfaces is then
    # compared by its TypeError); the reconstruction needs ps.  Where it does not: the TypeError, in every kind
    if kind == "reconstruct":
        assert not any(c["p_none"] for c in valid)
    else:
        assert sum(c["p_none"] and not _two(kind, c) or (kind == "tsurf" and c["p_none"] and c["g_polarity"] == c["l_polarity"] == "ignore")
                   for c in valid) >= 3
        assert not any(c["p_none"] and kind != "tsurf" and _two(kind, c) for c in valid)
    assert any(c["bad"] == "ps_none" and c["p_none"] for c in cases)
    # every invalid argument of the kind is compared (a 'bad_arg' case takes each in turn), and an index outside the stream
    assert any(c["bad"] == "bad_arg" and tuple(c["bad_arg"]) == getattr(F, kind.upper() + "_BAD_ARGS") for c in cases)
    assert sum(c["bad"] == "bad_arg" for c in cases) >= 2
    if kind in ("tsurf", "corners", "planeflow"):
        _drawn([c["select"] for c in valid], "class", F.GROUP_SELECTS)
        assert any(c["bad"] == "select_oob" for c in cases)
    assert any(_two(kind, c) and c["s"]["h"] * c["s"]["w"] % 64 for c in valid) or kind == "reconstruct"
    # the injected invalid inputs: few, and each kind of them somewhere in the family; no non-finite stamp anywhere
    assert 0 < sum(c["bad"] is not None for c in cases) <= 0.15 * len(cases)
    assert all(np.isfinite(c["s"]["ref"][2]).all() for c in cases)
    # int16 stays in range; no run reaches 2^14
    for c in cases:                                        # (a value that wrapped would be negative, or break the order of a sorted column)
        if c["tk"] == "i16":
            t16 = c["s"]["cols"][2]
            assert t16.dtype == np.int16 and (len(t16) == 0 or (t16.min() >= 0 and t16.max() < 30_000))
            assert c["order"] == "unsorted" or (np.diff(t16.astype(np.int64)) >= 0).all()
    assert max(int(_runs(F, c, False).max()) for c in valid) < F.GROUP_MAX_RUN


def test_grouping_family_draws_every_event_count_and_hot_run(group_cases):
    F, out = group_cases
    cases = [c for kind in GROUP for c in out[kind][0]]
    _drawn(cases, "n_class", F.N_GROUP_SMALL + F.N_GROUP_LARGE + ["hot"])
    for kind in ("denoise", "reconstruct"):
        _drawn(out[kind][0], "hot_base", F.HOT_BASES)
        _drawn(out[kind][0], "hot_delta", [-1, 0, 1])
    assert {(c["hot_base"], c["hot_delta"]) for c in cases} >= {(b, d) for b in F.HOT_BASES for d in (-1, 0, 1)}
    # every kind of injected invalid input, each compared by the exception type its docstring states
    _drawn(cases, "bad", [None, "oob_pixel", "frac_pixel", "ps_none", "select_oob", "bad_arg", "unsorted", "index_oob"])


@pytest.mark.parametrize("kind", GROUP)
def test_grouping_crosses_occur(group_cases, kind):
    F, out = group_cases
    valid = [c for c in out[kind][0] if c["bad"] is None]
    assert any(c["scale"] < 0 and c["kind"] in F.GROUP_EVENT_KINDS and (_two(kind, c) or kind == "reconstruct") for c in valid)
    assert any(c["kind"] in ("tensor_slice", "slice", "small_dev") and c["scene"] == "hot" for c in valid)
    if kind in ("tsurf", "corners", "planeflow"):
        assert any(c["tk"] in ("i16", "i32", "i64") and c["select"]["class"] not in ("none", "empty") for c in valid)
    if kind == "planeflow":
        assert any(c["fractional"] and c["outlier_threshold"] is not None for c in valid)
        assert sum(c["fractional"] for c in out[kind][0]) >= len(out[kind][0]) / 3.0


def test_denoise_cases_have_something_to_compare(group_cases):
    F, out = group_cases
    pairs = [(c, r) for c, r in zip(*out["denoise"]) if r is not None]
    assert len(pairs) >= 0.7 * len(out["denoise"][0])
    share = [float(r["keep"].mean()) if c["n"] else 0.0 for c, r in pairs]
    assert np.mean([0.0 < v < 1.0 for v in share]) >= 0.5, np.mean([0.0 < v < 1.0 for v in share])
    refr = [float(r["rkeep"].mean()) if c["n"] else 0.0 for c, r in pairs]
    assert np.mean([0.0 < v < 1.0 for v in refr]) >= 0.5
    for key, values in (("radius", [1, 2, 3]), ("include_self", [False, True]), ("two", [False, True]), ("dt_class", F.GROUP_DT),
                        ("rf_class", F.GROUP_DT), ("walk", ["default", "stream", "pixel"]), ("wave_run", [1, 64, 0, 1 << 30]),
                        ("return_support", [False, True])):
        _drawn([c for c, _ in pairs], key, values)
    assert any(c["support"] > 4 for c, _ in pairs)
    # a negative p_scale with two classes where the sign matters (p == 0 among the polarities: the classes of +-1 swap as a whole)
    N = F._t("_denoise_np")
    seen = 0
    for c, r in pairs:
        if c["scale"] < 0 and c["two"]:
            x, y, t, p = c["s"]["ref"]
            size = (c["s"]["h"], c["s"]["w"])
            seen += bool((N.fast_support(x, y, t, -p, c["dt"], size, c["radius"], c["include_self"], True) != r["sup"]).any() or
                         (N.fast_refractory(x, y, t, -p, c["refractory"], size, True) != r["rkeep"]).any())
    assert seen >= 3, seen


def test_tsurf_cases_have_something_to_compare(group_cases):
    F, out = group_cases
    cases, refs = out["tsurf"]
    good = []
    for c, r in zip(cases, refs):
        vals = [] if r is None else [r["local"]] + [v for v in (r["global"], r["hats"] and r["hats"][0]) if v is not None]
        good.append(any((np.isfinite(v) & (v != 0)).any() for v in vals))
    assert np.mean(good) >= 0.7, np.mean(good)
    valid = [c for c in cases if c["bad"] is None]
    for key, values in (("decay", [None, "exp", "linear"]), ("radius", [1, 2, 3, 4]), ("g_polarity", ["split", "ignore"]),
                        ("l_polarity", ["same", "split", "ignore"]), ("include_self", [False, True]), ("normalise", [False, True]),
                        ("cell_size", [1, 3, 7, 10, 100]), ("query", ["t_refs", "indices"]), ("deep", ["none", "f32", "f64"]), ("K", [1, 2])):
        _drawn(valid, key, values)
    seen = set().union(*[c["q_classes"] for c in valid])
    assert seen >= {"before", "after", "on", "tied", "between", "cut0", "cutn", "unsorted_cuts"}, seen
    assert any(c["cell_size"] > max(c["s"]["h"], c["s"]["w"]) for c in valid)
    assert any(c["s"]["h"] % c["cell_size"] and c["cell_size"] < c["s"]["h"] for c in valid)
    # the deep cases reach the underflow of the float32 and of the double exp; the others stay clear of subnormals
    T = F._t("_time_surface_np")
    for c, r in zip(cases, refs):
        if r is not None and c["deep"] == "none" and c["decay"] == "exp":
            for v in (r["local"], r["global"]):
                assert v is None or not ((v != 0) & (np.abs(v) < 2.0 ** -126)).any(), c["desc"]
    assert any(r is not None and c["deep"] == "f64" and c["n"] > 1 and c["s"]["span"] / c["tau"] > 745 for c, r in zip(cases, refs))
    assert T.value(np.array([746.0]), "exp", 1.0)[0] == 0 and T.value(np.array([88.0]), "exp", 1.0)[0] < 2.0 ** -126


def test_corner_cases_contain_corners(group_cases):
    F, out = group_cases
    pairs = [(c, r) for c, r in zip(*out["corners"]) if r is not None]
    assert len(pairs) >= 0.7 * len(out["corners"][0])
    eligible = [(c, r) for c, r in pairs if r["eligible"].any()]
    both = [bool((r["flags"] & r["eligible"]).any() and (~r["flags"] & r["eligible"]).any()) for c, r in eligible]
    assert len(eligible) >= 0.3 * len(pairs) and np.mean(both) >= 0.2, (len(eligible), np.mean(both))
    assert any(np.isfinite(r["scores"]).any() and (r["scores"] > r["threshold"]).any() and (r["scores"] <= r["threshold"]).any() for _, r in eligible)
    assert any(not r["eligible"].any() and c["n"] > 0 for c, r in pairs)            # a sensor with a side below 9
    for key, values in (("polarity", ["same", "ignore"]), ("window", ["n_last", "dt"]), ("detector", ["fast", "harris"]),
                        ("return_index", [False, True])):
        _drawn([c for c, _ in pairs], key, values)
    _drawn([c for c, _ in pairs if c["window"] == "n_last"], "n_last_class", ["1", "2", "n", "above", "some"])
    assert any(c["return_index"] and c["polarity"] == "same" and r["keep"].any() for c, r in pairs)      # the chain has rows


def test_planeflow_cases_fit_reject_and_see_the_order_of_a_sum(group_cases):
    F, out = group_cases
    pairs = [(c, r) for c, r in zip(*out["planeflow"]) if r is not None]
    assert len(pairs) >= 0.7 * len(out["planeflow"][0])
    fitted = [c["n"] > 0 and r["valid"].mean() >= 0.1 for c, r in pairs]
    assert np.mean(fitted) >= 0.5, np.mean(fitted)
    for key, values in (("radius", [1, 2, 3, 4]), ("polarity", ["same", "ignore"]), ("iterations", list(range(9))), ("dt_class", F.PLANEFLOW_DT),
                        ("return_valid", [False, True]), ("return_lifetime", [False, True])):
        _drawn([c for c, _ in pairs], key, values)
    assert any(c["min_samples"] == 3 for c, _ in pairs) and any(c["min_samples"] > 9 for c, _ in pairs)
    assert any(c["max_speed"] is not None and 0 < (r["valid"] != F.planeflow_reference(c, max_speed=None)["valid"]).sum() for c, r in pairs)
    # rejection: with iterations = 0 some but not all events differ; and in one case events take 0, 1 and several rounds
    some, rounds = False, False
    same = lambda a, b: np.all((a["flow"] == b["flow"]) | (np.isnan(a["flow"]) & np.isnan(b["flow"])), axis=1)  # noqa: E731
    for c, r in pairs:
        if c["outlier_threshold"] is None or c["iterations"] < 2 or c["n"] < 3:
            continue
        with np.errstate(all="ignore"):
            r0, r1 = F.planeflow_reference(c, iterations=0), F.planeflow_reference(c, iterations=1)
        d0, d1 = ~same(r0, r), ~same(r1, r)
        some |= bool(d0.any() and not d0.all())
        rounds |= bool((~d0).any() and (d0 & ~d1).any() and d1.any())      # none dropped / done after one round / a later round changed it
    assert some and rounds
    # summation order: in a fractional-time case the double sum of a window's tau depends on its order
    T = F._t("_time_surface_np")
    seen = False
    for c, r in pairs:
        if seen or not c["fractional"] or c["n"] < 64:
            continue
        x, y, t, p = c["s"]["ref"]
        age = T.fast_local_time_surfaces(x, y, t, p, None, (c["s"]["h"], c["s"]["w"]), radius=c["radius"], decay=None, polarity=c["polarity"])
        tau = np.where(np.isfinite(age) & (age <= c["dt"]), -age, 0.0).reshape(len(x), -1)
        fwd, rev = np.zeros(len(x)), np.zeros(len(x))
        for k in range(tau.shape[1]):
            fwd, rev = fwd + tau[:, k], rev + tau[:, tau.shape[1] - 1 - k]
        seen = bool((fwd != rev).any())
    assert seen
    # ... and through the rule itself: the restatement on the mirrored stream (x -> w - 1 - x, vx -> -vx) forms the same sums with
    # dx running from r down to -r; in the cases drawn for it (planeflow_inputs, 'probe') that changes a flow beyond the tolerance
    N = F._t("_plane_flow_np")
    reports = 0
    for c, r in pairs:
        if not c["probe"] or c["s"]["size_class"] in ("1x1", "1xW", "Hx1"):
            continue
        assert c["scene"] == "front" and c["tk"] == "micro" and c["order"] == "sorted" and c["outlier_threshold"] is None
        x, y, t, p = c["s"]["ref"]
        with np.errstate(all="ignore"):
            flow, valid, _ = N.fast_local_plane_flow(c["s"]["w"] - 1 - x.astype(np.int64), y, t, p, c["dt"], (c["s"]["h"], c["s"]["w"]), **c["fit"])
        flow = flow * np.float32([-1.0, 1.0])
        reports += F.flags_equal(valid, r["valid"], "valid") is not None or F.rel23_close(flow, r["flow"], "flow") is not None
    assert reports >= 5, reports
    # the strictness of the residual test: with the threshold one step lower (e > th- is e >= th) the restatement differs, in the cases
    # whose threshold lies on a residual ('th_probe')
    strict = 0
    for c, r in pairs:
        if c["th_probe"]:
            with np.errstate(all="ignore"):
                m = F.planeflow_reference(c, outlier_threshold=float(np.nextafter(c["outlier_threshold"], -np.inf)))
            strict += F.flags_equal(m["valid"], r["valid"], "valid") is not None or F.rel23_close(m["flow"], r["flow"], "flow") is not None
    assert strict >= 3, strict


def test_reconstruct_cases_count_events(group_cases):
    F, out = group_cases
    pairs = [(c, r) for c, r in zip(*out["reconstruct"]) if r is not None]
    assert len(pairs) >= 0.7 * len(out["reconstruct"][0])
    counted = []
    for c, (want, bound) in pairs:
        base = np.abs(np.zeros(want.shape[1:]) if c["initial"] is None else c["initial"].astype(np.float64))
        if c["initial"] is None and c["frames"] is not None:
            base = np.abs(c["frames"][0].astype(np.float64))
        fmax = 0.0 if c["frames"] is None else np.abs(c["frames"].astype(np.float64)).max(axis=0)
        counted.append(bool((bound[-1] > base + fmax).any()))
    assert np.mean(counted) >= 0.7, np.mean(counted)
    valid = [c for c, _ in pairs]
    for key, values in (("alpha_class", ["zero", "slow", "fast", "underflow"]), ("query", ["t_refs", "indices"]),
                        ("filter", ["leaky", "complementary"]), ("wave_run", [1, 64, 65, 0, 1 << 30]), ("has_initial", [False, True]),
                        ("start_class", ["default", "before", "inside"]), ("F", [0, 1, 2, 3, 4]), ("K", [1, 2, 3, 4]), ("stream", [False, True])):
        _drawn(valid, key, values)
    assert set().union(*[c["f_classes"] for c in valid]) >= {"before", "between", "after", "on"}
    assert all(c["c_on"] != c["c_off"] for c in valid)
    assert any(c["alpha_class"] == "underflow" and (want == 0).any() and (want != 0).any() for c, (want, _) in pairs)
    assert any(c["stream"] and c["s"]["plan"] is None for c in valid)


def test_runs_straddle_the_wave_thresholds(group_cases):
    """EVK_RECONSTRUCT_WAVE_RUN = 1024 and EVK_DENOISE_WAVE_RUN = 4096, steps of 256 events: the run lengths, from np.bincount of the
    grouping's keys, lie at each threshold and one step above it, each - 1, + 0 and + 1; and some two-class case has long runs
    at the last key of class 0 and the first key of class 1."""
    F, out = group_cases
    for kind in ("denoise", "reconstruct"):
        lengths, both_sides = set(), False
        for c in out[kind][0]:
            if c["bad"] is not None or c["scene"] != "hot":
                continue
            two = _two(kind, c)
            runs = _runs(F, c, two)
            lengths |= set(int(v) for v in runs[runs >= 1000])
            if c["s"]["hot"]["exact"]:
                assert int(runs.max()) == max(c["s"]["hot"]["len"], c["s"]["hot"]["len2"]), c["desc"]
            hw = c["s"]["h"] * c["s"]["w"]
            both_sides |= bool(two and hw > 1 and runs[hw - 1] >= 1023 and runs[hw] >= 1023)
        want = {b + d for b in F.HOT_BASES for d in (-1, 0, 1)}
        assert lengths >= want, sorted(want - lengths)
        assert both_sides or kind == "reconstruct"
    assert any(c["hot_place"] == "boundary" and c["s"]["h"] * c["s"]["w"] % 64 not in (0,) for c in out["reconstruct"][0] if c["bad"] is None)


# ---- the two features defined bit for bit: multi-view stereo and the event simulator ----------------------------------------------

@pytest.fixture(scope="module")
def emvs_cases():
    F = _fuzz()
    cases = [F.emvs_inputs(rng) for rng in _rngs("emvs")]
    return F, cases, [F.emvs_reference(c) for c in cases]


def _emvs_uv(c, r):
    """(u, v) of every event on every plane, (D, n) each, NaN where the ray or the plane is skipped: the formula of dsi_votes"""
    x, y, _ = c["ref"]
    M = r["table"][np.arange(len(x)) // min(c["packet_size"], max(len(x), 1))]
    Km = c["K"] if c["ref_K"] is None else c["ref_K"]
    with np.errstate(all="ignore"):
        d = [(M[:, 3 * k] * x + M[:, 3 * k + 1] * y) + M[:, 3 * k + 2] for k in range(3)]
        a, b = np.where(d[2] > 0, d[0] / d[2], np.nan), np.where(d[2] > 0, d[1] / d[2], np.nan)
        s = c["depths"][:, None] - M[None, :, 11]
        s = np.where(s > 0, s, np.nan)
        u = (Km[0, 0] * (M[None, :, 9] + s * a)) * (1.0 / c["depths"][:, None]) + Km[0, 2]
        v = (Km[1, 1] * (M[None, :, 10] + s * b)) * (1.0 / c["depths"][:, None]) + Km[1, 2]
    return u, v, d[2]


def test_emvs_generator_draws_every_class(emvs_cases):
    F, cases, _ = emvs_cases
    _, L = F._lib_geometry()
    ev, raw = [c for c in cases if c["mode"] == "events"], [c for c in cases if c["mode"] == "raw"]
    for key, values in (("kind", F.EMVS_KINDS), ("coord", F.EMVS_COORDS), ("volume", F.EMVS_VOLUMES), ("planes", F.EMVS_PLANES),
                        ("shape", ["row", "column", "random"]), ("n_class", F.EMVS_N_CLASSES), ("tk", F.EMVS_TIMES), ("pk", F.EMVS_PACKETS),
                        ("voting", ["nearest", "bilinear"]), ("flips", [False, True]), ("unnorm", [False, True]), ("on_traj", [False, True]),
                        ("D", range(1, 10))):
        _drawn(ev, key, values)
    assert {c["n"] for c in ev} >= {0, 1, 4095, 4096, 4097, 8191, 8193} and max(c["n"] for c in ev) <= 8193
    assert {len(c["pose_ts"]) for c in ev} == {2, 3, 4, 5, 6}
    assert all(c["sensor"][0] <= 40 and c["sensor"][1] <= 40 and (c["volume"].startswith("tiles") or max(c["size"]) <= 40) for c in ev)
    # the chunk counts: every class on the first and on the second call, crossed with the packet sizes around n; a boundary inside a trip
    for i in (0, 1):
        assert {c["ck"][i] for c in ev} >= set(F.EMVS_CHUNKS)
    assert all(c["ck"][0] != c["ck"][1] for c in ev)
    assert any(c["pk"] in ("n-1", "n", "n+1") and c["ck"][0] != "auto" and c["n"] > 64 for c in ev)
    assert any("trip" in c["ck"] and c["n"] > 4096 and -(-c["n"] // c["chunks"][c["ck"].index("trip")]) % 4096 for c in ev)
    chunks = [c["chunks"][0] or L.evk_emvs_chunks(c["n"], c["D"], *c["size"]) for c in ev]
    assert sum(min(k, c["n"]) >= 2 for k, c in zip(chunks, ev)) >= 10
    # volumes: another size and camera; several tiles by the library's own geometry
    assert all(c["ref_K"][0, 0] != c["ref_K"][1, 1] and c["ref_K"][0, 2] != c["size"][1] / 2 for c in ev if c["volume"] != "sensor")
    tiles = [c for c in ev if c["volume"].startswith("tiles")]
    assert 0 < len(tiles) <= 0.2 * len(ev)
    for c in tiles:
        rows, cols = L.evk_emvs_band_rows(*c["size"]), L.evk_emvs_band_cols(*c["size"])
        assert -(-c["size"][0] // rows) * -(-c["size"][1] // cols) >= 2 and c["D"] <= 2 and c["dm"]["median_size"] == 0
    # planes: unordered, duplicated
    assert any(c["D"] >= 3 and (np.diff(c["depths"]) > 0).any() and (np.diff(c["depths"]) < 0).any() for c in ev)
    assert any(c["planes"] == "dup" and len(set(c["depths"])) < c["D"] for c in ev)
    # coordinates: the wild classes in xs, in ys, in both; float32 columns of one and of mixed widths
    wild = [c for c in ev if c["coord"] == "wild"]
    _drawn(wild, "where", F.EMVS_WILD_WHERE)
    assert set().union(*[c["wild"] for c in wild]) >= set(F.EMVS_WILD)
    assert any(c["kind"] in F.EMVS_F32_KINDS and "huge" in c["wild"] for c in wild)
    assert any(c["coord"] == "f32" and c["x"].dtype != c["y"].dtype for c in ev)
    # the depth map
    both = ev + raw
    assert {c["dm"]["filter_radius"] for c in both} >= {0, 1, 2, 16} and {c["dm"]["median_size"] for c in both} == {0, 3, 5}
    assert {c["dm"]["threshold"] for c in both} >= set(F.EMVS_THRESHOLDS)
    assert any(c["dm"]["filter_radius"] > max(c["size"]) for c in both)
    # the hand-built raw volumes
    assert len(raw) >= 10 and {c["scale"] for c in raw} == {1, 256} and {c["numpy_view"] for c in raw} == {"int32", "uint32"}
    assert any(c["has_ties"] for c in raw) and all(c["size"][0] <= 40 and c["size"][1] <= 40 for c in raw)
    assert any((c["raw"] == 2 ** 32 - 1).any() for c in raw) and any((c["raw"] == 2 ** 31).any() for c in raw)
    assert all((c["raw"] >= 2 ** 31).any() and c["raw"].max() < 2 ** 32 for c in raw)
    assert any((c["raw"].max(axis=0) == 0).any() for c in raw) and any(c["size"] != (19, 23) for c in raw)
    # the injected invalid inputs
    assert {c["bad"] for c in ev} >= set(F.EMVS_BAD) and any(c["bad"] is not None for c in raw)
    assert sum(c["bad"] is not None for c in cases) <= 0.15 * len(cases)


def test_emvs_cases_vote_where_the_kernel_branches(emvs_cases):
    F, cases, refs = emvs_cases
    pairs = [(c, r) for c, r in zip(cases, refs) if c["mode"] == "events"]
    assert np.mean([bool(r["raw"].any()) for c, r in pairs]) >= 0.8
    silent = d2 = corner = ties = 0
    for c, r in pairs:
        if not c["n"]:
            continue
        s = c["depths"][:, None] - r["table"][None, :, 11]
        silent += bool(((s > 0).any(axis=1) & (s <= 0).any(axis=1)).any())              # a plane silent for some packets only
        u, v, dz = _emvs_uv(c, r)
        with np.errstate(invalid="ignore"):
            d2 += bool(((dz <= 0) & (np.abs(c["ref"][0]) < 1e30) & (np.abs(c["ref"][1]) < 1e30)).any())
            if c["voting"] == "bilinear":                   # a corner dropped at the left or right border while its neighbour lands
                H, W = c["size"]
                x0, y0 = np.floor(u), np.floor(v)
                fu, fv = u - x0, v - y0
                row = (y0 >= 0) & (y0 < H)
                corner += bool((row & (x0 == -1) & (np.rint(fu * (1 - fv) * 256) > 0)).any() or
                               (row & (x0 == W - 1) & (np.rint((1 - fu) * (1 - fv) * 256) > 0)).any())
        top = r["raw"].max(axis=0)
        ties += bool((((r["raw"] == top).sum(axis=0) >= 2) & (top > 0)).any())          # two planes tie for the maximum of a pixel
    assert silent >= 3 and d2 >= 3 and corner >= 3 and ties >= 5, (silent, d2, corner, ties)
    # a plane exactly at a packet's camera centre (s == 0: skipped), in a packet with rays that would otherwise vote
    centre = 0
    for c, r in pairs:
        if c["on_centre"]:
            zero = (c["depths"][:, None] - r["table"][None, :, 11]) == 0
            packet = np.arange(c["n"]) // min(c["packet_size"], c["n"])
            centre += bool(zero.any() and (_emvs_uv(c, r)[2][np.isin(packet, np.nonzero(zero.any(axis=0))[0])] > 0).any())
    assert centre >= 3, centre
    assert any(c["planes"] == "behind" and ((c["depths"][:, None] - r["table"][None, :, 11]) <= 0).any() and r["raw"].any() for c, r in pairs)
    # the wild cases: the finite events still vote
    wild = [(c, r) for c, r in pairs if c["coord"] == "wild" and c["n"] >= 64]
    assert len(wild) >= 5 and np.mean([bool(r["raw"].any()) for c, r in wild]) >= 0.8
    assert all(not np.isfinite(np.concatenate(c["ref"][:2])).all() for c, r in wild)


def test_emvs_exact_cases_land_on_every_tie(emvs_cases):
    """u == x and v == y exactly in the 'exact' class: the restatement's nearest votes are the hand count of floor(x + 0.5),
    floor(y + 0.5); the coordinates sit on the ties and borders of both voting rules."""
    F, cases, refs = emvs_cases
    pairs = [(c, r) for c, r in zip(cases, refs) if c["mode"] == "events" and c["coord"] == "exact" and c["n"]]
    _drawn([c for c, _ in pairs], "voting", ["nearest", "bilinear"])
    seen = set()
    for c, r in pairs:
        (H, W), (x, y, _) = c["size"], c["ref"]
        u, v, _ = _emvs_uv(c, r)
        assert np.array_equal(u, np.tile(x, (c["D"], 1))) and np.array_equal(v, np.tile(y, (c["D"], 1))), c["desc"]
        if c["voting"] == "nearest":
            iu, iv = np.floor(x + 0.5).astype(np.int64), np.floor(y + 0.5).astype(np.int64)
            inside = (iu >= 0) & (iu < W) & (iv >= 0) & (iv < H)
            hand = np.bincount(iv[inside] * W + iu[inside], minlength=H * W).reshape(H, W)
            assert all(np.array_equal(plane, hand) for plane in r["raw"]), c["desc"]
        for name, col, S in (("x", x, W), ("y", y, H)):
            k = col + 0.5
            seen |= {(c["voting"], name, what) for what, hit in (("k-0.5", (k == np.floor(k)) & (k > 0) & (k < S)), ("-0.5", col == -0.5),
                                                                 ("S-0.5", col == S - 0.5), ("floor=-1", np.floor(col) == -1),
                                                                 ("floor=S-1", np.floor(col) == S - 1)) if hit.any()}
    want = {(vt, name, what) for vt in ("nearest", "bilinear") for name in "xy" for what in ("k-0.5", "-0.5", "S-0.5", "floor=-1", "floor=S-1")}
    assert seen >= want, sorted(want - seen)
    # a bilinear weight on its own rounding tie, 256 w = k + 0.5, at a corner inside the volume, rounding down (k even) and up (k odd)
    down = up = 0
    for c, r in pairs:
        if c["voting"] == "bilinear":
            (H, W), (x, y, _) = c["size"], c["ref"]
            x0, y0 = np.floor(x), np.floor(y)
            w = 256.0 * (1.0 - (x - x0)) * (1.0 - (y - y0))
            tie = (w - np.floor(w) == 0.5) & (x0 >= 0) & (x0 < W) & (y0 >= 0) & (y0 < H)
            down += bool((tie & (np.floor(w) % 2 == 0)).any())
            up += bool((tie & (np.floor(w) % 2 == 1)).any())
    assert down >= 2 and up >= 2, (down, up)


def test_emvs_depth_maps_have_something_to_compare(emvs_cases):
    F, cases, refs = emvs_cases
    N = F._t("_emvs_np")
    valid = [(c, r) for c, r in zip(cases, refs)]
    partial = [bool(r["dm"][3].any() and not r["dm"][3].all()) for c, r in valid]
    assert np.mean(partial) > 0.5, np.mean(partial)
    changed = 0
    for c, r in valid:
        if c["dm"]["median_size"] and r["dm"][3].any():
            scale = c["scale"] if c["mode"] == "raw" else N.SCALE[c["voting"]]
            plain = N.dsi_depth_map(r["raw"] & 0xFFFFFFFF, scale, c["depths"], **dict(c["dm"], median_size=0))
            changed += bool((plain[1] != r["dm"][1]).any())
    assert changed >= 5, changed


@pytest.fixture(scope="module")
def simulate_cases():
    F = _fuzz()
    cases = [F.simulate_inputs(rng) for rng in _rngs("simulate")]
    return F, cases, [F.simulate_reference(c) for c in cases]


def _sim_image(t):
    u = int(np.float64(t).view(np.uint64))
    return (~u) & (2 ** 64 - 1) if u >> 63 else u | (1 << 63)


def _sim_key_bits(T):
    """sim_key_bits of evk_simulate.hip on the host times, as event_simulator.py forms t_first and t_max"""
    fts = np.asarray(T, np.float64) + 0.0
    t_max = float(np.max(fts[:-1] + (fts[1:] - fts[:-1])))
    return max((_sim_image(t_max) - _sim_image(float(fts[0]))).bit_length(), 8)


def test_simulate_generator_draws_every_class(simulate_cases):
    F, cases, _ = simulate_cases
    for key, values in (("shape", F.SIM_SHAPES), ("tk", F.SIM_TIMES), ("amp", F.SIM_AMPS), ("dtype", F.SIM_DTYPES), ("special", F.SIM_SPECIALS),
                        ("layout", F.SIM_LAYOUTS), ("ik", F.SIM_INPUTS), ("tsk", F.SIM_TS_KINDS), ("ck", F.SIM_CONTRASTS), ("rk", F.SIM_REFRACTORY),
                        ("sk", F.SIM_STATES), ("wide", [False, True]), ("F", range(2, 7)), ("bad", F.SIM_BAD + (None,))):
        _drawn(cases, key, values)
    _drawn([c for c in cases if c["ck"] != "scalar"], "mk", F.SIM_MAP_KINDS)
    assert sum(c["bad"] is not None for c in cases) <= 0.15 * len(cases)
    assert all(c["H"] <= 24 and c["W"] <= 24 or (c["shape"] == "one_row" and c["H"] == 1 and 257 <= c["W"] <= 600) for c in cases)
    hw = {c["H"] * c["W"] for c in cases}
    assert min(hw) < 8 and hw >= {63, 64, 65, 255, 256} and any(64 < v < 255 for v in hw) and any(v > 256 for v in hw)
    assert {np.asarray(c["frames"]).dtype for c in cases} >= {np.dtype(t) for t in (np.float64, np.float32, np.int16, np.int32, np.uint8)}
    assert all((c["layout"] == "contiguous") == bool(c["frames"].flags.c_contiguous) or c["H"] * c["W"] == 1 for c in cases)
    assert any(np.isnan(c["frames"][0]).any() for c in cases if c["special"] == "nonfinite")
    assert all(np.isfinite(c["frames"]).all() for c in cases if c["special"] == "huge")
    assert any(np.signbit(c["T"][c["T"] == 0]).any() for c in cases if c["tk"] == "negative") and any((c["T"] < 0).any() and (c["T"] > 0).any() for c in cases)
    assert all(np.array_equal(c["T"][1:], np.nextafter(c["T"][:-1], np.inf)) for c in cases if c["tk"] == "neighbours")
    assert all((np.abs(c["T"]) < 2.0 ** -1022).all() for c in cases if c["tk"] == "subnormal")
    # the state classes: last_event_ts alone holds +inf and NaN entries; a reference alone; both from a previous call
    last = [c for c in cases if c["sk"] == "last"]
    assert all(c["reference"] is None for c in last) and any(np.isnan(c["last"]).any() for c in last) and any(np.isposinf(c["last"]).any() for c in last)
    assert all(c["last"] is None and c["reference"] is not None for c in cases if c["sk"] == "reference")
    assert all(c["last"] is not None and c["reference"] is not None for c in cases if c["sk"] == "both")
    # maps crossed with a state, a refractory period and the wide sort values
    assert any(c["ck"] != "scalar" and c["sk"] in ("reference", "both") and c["rk"] != "zero" and c["wide"] for c in cases)
    # the key bits: the 8-bit floor, a middle range, all 64
    bits = {c["tk"]: set() for c in cases}
    for c in cases:
        bits[c["tk"]].add(_sim_key_bits(c["T"]))
    assert bits["neighbours"] == {8} and bits["span64"] == {64} and all(8 < b < 64 for b in bits["epoch9"] | bits["epoch15"] | bits["small"]), bits
    assert _sim_key_bits([1.0, 2.0]) == 53 and _sim_key_bits([-0.0, 5e-324]) == 8 and _sim_key_bits([-1.0, 1.0]) == 63 and _sim_key_bits([-1e300, 1e300]) == 64


def test_simulate_cases_emit_tie_drop_and_clamp(simulate_cases):
    F, cases, refs = simulate_cases
    assert all(r[6] == 0 for r in refs)                     # overflow occurs only in the error cases
    for c in cases:
        if c["bad"] is not None and c["bad"].startswith("overflow"):
            assert 1 <= F.simulate_reference(c, **c["bad_over"])[6] <= 2, c["desc"]
        if c["bad"] == "map_values":
            assert c["bad_pixels"] >= 1
    emitting = [(c, r) for c, r in zip(cases, refs) if len(r[2])]
    assert len(emitting) >= 0.8 * len(cases) and len(emitting) < len(cases)
    tied = [bool((np.diff(r[2]) == 0).any()) for c, r in emitting]
    assert np.mean(tied) >= 0.25, np.mean(tied)
    reordered = sum(not np.array_equal(np.lexsort((r[3], r[1], r[0], r[2])), np.arange(len(r[2]))) for c, r in emitting)
    assert reordered >= 10, reordered
    part = 0
    for c, r in emitting:
        if c["rk"] != "zero":
            part += len(r[2]) < len(F.simulate_reference(c, refractory=0.0)[2])
    assert part >= 10, part
    assert sum(c["sk"] == "reference" and bool((r[2] == c["T"][0]).any()) for c, r in emitting) >= 5
    assert sum(c["split"] is not None and bool((r[2] == c["T"][c["split"]]).any()) for c, r in emitting) >= 10
    assert any(c["amp"] == "limit" and np.bincount(r[1] * c["W"] + r[0]).max() > 60000 for c, r in emitting)
    assert any(c["special"] == "huge" and len(r[2]) for c, r in emitting)


# ---- the dense-flow losses and motion segmentation (profiles/fuzz_flow_segment.txt) -------------------------------------------------
@pytest.fixture(scope="module", params=["flowts", "flowcm"])
def flow_cases(request):
    F = _fuzz()
    gen = F.flowts_inputs if request.param == "flowts" else F.flowcm_inputs
    cases = [gen(rng) for rng in _rngs(request.param)]
    return F, request.param, cases, [F.flow_reference(c) for c in cases]        # the restatement's own float32 warp: no GPU


def _flow_samples(F, cases):
    """(case, b, flow, (x, y, t, p)) of every sample of every case"""
    return [(c, b, flow, cols) for c in cases for b, flow, cols in F._flow_samples(c)]


def test_flow_generators_draw_every_class(flow_cases):
    F, kind, cases, _ = flow_cases
    from event_utils_amd import _lib
    from event_utils_amd.contrast_max.objectives import _blur_kernel
    cm = kind == "flowcm"
    for axis in (0, 1):                                         # H and W, drawn independently
        assert {c["sizes"][axis] for c in cases} == set(F.FLOW_SIZES)
    assert {(c["H"], c["W"]) for c in cases} & {(2, 2), (2, 3), (3, 2), (3, 3)} and {64, 65} <= {c["H"] for c in cases} | {c["W"] for c in cases}
    assert any(c["sizes"][0] != c["sizes"][1] for c in cases)
    for key, values in (("fk", F.FLOW_FIELDS), ("batched", [False, True]), ("empty", F.FLOW_EMPTY), ("ok", F.FLOW_OFFSETS + ("none",)),
                        ("pk", F.FLOW_POSITIONS), ("polk", F.FLOW_POLS + (("real",) if cm else ())), ("scale", F.FLOW_SCALES),
                        ("nf", F.FLOW_NONFINITE), ("bk", F.FLOW_BLURS), ("direction", F.FLOW_DIRECTIONS)):
        _drawn(cases, key, values)
    if cm:
        _drawn(cases, "objective", F.FLOW_OBJECTIVES)
        _drawn(cases, "use_polarity", [False, True])
    assert {c["B"] for c in cases if c["batched"]} == {1, 2, 3, 4, 5}
    assert {tk for c in cases for tk in c["tks"]} == set(F.FLOW_TIMES) and any(len(set(c["tks"])) > 1 for c in cases)
    counts = {n for c in cases for n in c["ns"]}
    assert counts >= {0, 1, 2, 63, 64, 65, 255, 256, 257} and any(257 < n <= 4000 for n in counts) and max(counts) <= 4000
    # an empty sample at every place of a batch, and every sample empty; every kind of offsets with an empty sample
    place = {"first": lambda ns: ns[0] == 0 and all(ns[1:]), "last": lambda ns: ns[-1] == 0 and all(ns[:-1]),
             "middle": lambda ns: len(ns) >= 3 and ns[len(ns) // 2] == 0 and ns[0] and ns[-1], "all": lambda ns: not any(ns)}
    for name, holds in place.items():
        assert any(c["empty"] == name and holds(c["ns"]) for c in cases), name
    assert {c["ok"] for c in cases if 0 in c["ns"] and c["batched"]} == set(F.FLOW_OFFSETS)
    assert all(c["offsets"].dtype == np.int64 and c["offsets"][0] == 0 and c["offsets"][-1] == len(c["cols"][0]) for c in cases)
    samples = _flow_samples(F, cases)
    # columns: float32 values, sorted per sample (a NaN aside), one-event samples, D = 0
    for c, b, flow, (x, y, t, p) in samples:
        assert all(a.dtype == np.float32 for a in (flow, x, y, t, p))
        tt = t[~np.isnan(t)]
        assert np.all(np.diff(tt) >= 0), c["desc"]
    assert any(len(cols[0]) == 1 for _, _, _, cols in samples)
    assert any(len(cols[2]) > 2 and cols[2][0] == cols[2][-1] for _, _, _, cols in samples)
    assert any(len(np.unique(cols[2])) == 2 and len(cols[2]) > 2 for c, b, _, cols in samples if c["tks"][b] == "two")
    # float32 stamps at 1e4 s are tied; a span of 100 s absorbs the 1e-6 of tdiv
    assert any((np.diff(cols[2]) == 0).any() and cols[2][0] >= 1e4 for c, b, _, cols in samples if c["tks"][b] == "f32_1e4")
    assert any(len(cols[2]) and np.float32(np.float32(cols[2][-1] - cols[2][0]) + np.float32(1e-6)) == np.float32(cols[2][-1] - cols[2][0]) > 0
               for c, b, _, cols in samples if c["tks"][b] == "u100")
    # positions: the last column and row among the integer pixels; beside the support on both sides; far outside
    assert any(c["pk"] == "integer" and (cols[0] == c["W"] - 1).any() and (cols[1] == c["H"] - 1).any() and (cols[0] == np.floor(cols[0])).all()
               for c, _, _, cols in samples if len(cols[0]))
    off = [(c, cols) for c, _, _, cols in samples if c["pk"] == "off_support" and len(cols[0])]
    assert any(((cols[0] > c["W"] - 1) & (cols[0] < c["W"] + 2)).any() for c, cols in off) and any(((cols[0] > -2) & (cols[0] < 0)).any() for c, cols in off)
    assert any(((cols[1] > c["H"] - 1) & (cols[1] < c["H"] + 2)).any() for c, cols in off) and any(((cols[1] > -2) & (cols[1] < 0)).any() for c, cols in off)
    assert any((np.abs(cols[0]) == 1e4).any() for c, _, _, cols in samples if c["pk"] == "far")
    # polarities and the fields
    pols = {c["polk"]: set() for c in cases}
    for c, _, _, cols in samples:
        pols[c["polk"]] |= set(cols[3][~np.isnan(cols[3])].tolist())
    assert pols["pm1"] == {-1.0, 1.0} and pols["01"] == {0.0, 1.0} and pols["pm1z"] == {-1.0, 0.0, 1.0}
    if cm:
        mags = np.abs(np.array(sorted(pols["real"])))
        assert mags.min() < 1e-2 and mags.max() > 1e2 and 1e-3 * 0.5 <= mags.min() and mags.max() <= 1e3
        # a batch whose samples' weights -- and with them the fixed-point exponents -- lie many binades apart
        assert any(c["polk"] == "real" and max(m) >= 2.0 ** 10 * min(m) for c in cases
                   for m in [[np.abs(cols[3]).max() for _, _, cols in F._flow_samples(c) if len(cols[3]) and not np.isnan(cols[3]).any()]] if len(m) >= 2)
    assert all(not c["flow"].any() for c in cases if c["fk"] == "zero" and c["nf"] != "field")
    assert all((c["flow"] == c["flow"][:, :, :1, :1]).all() for c in cases if c["fk"] == "constant" and c["nf"] != "field")
    # the one NaN: where it was announced, a time stamp never first or last of its sample
    for c in cases:
        x, y, t, p = c["cols"]
        nans = {"p": np.isnan(p).sum(), "x": np.isnan(x).sum(), "t": np.isnan(t).sum(), "field": np.isnan(c["flow"]).sum()}
        assert all(v == (1 if c["nf"] == k else 0) for k, v in nans.items()) and not np.isnan(y).any(), c["desc"]
        if c["nf"] == "t":
            assert c["where"] not in c["offsets"] and c["where"] + 1 not in c["offsets"]
    # the blurs: past the fused radius, and wider than the canvas (more than one reflection)
    assert _blur_kernel(F.FLOW_WIDE_SIGMA)[1] > _lib.EVK_MAX_RADIUS
    assert all(_blur_kernel(c["sigma"])[1] > min(c["H"], c["W"]) + 1 for c in cases if c["bk"] == "over_canvas")
    assert any(_blur_kernel(c["sigma"])[1] > 2 * (min(c["H"], c["W"]) + 1) for c in cases if c["bk"] == "over_canvas")
    assert {c["sigma"] for c in cases if c["bk"] == "none"} == {0.0, -1.0}


def test_flow_cases_keep_tau_in_range_and_count_events_beside_the_support(flow_cases):
    F, kind, cases, _ = flow_cases
    M = F._flow_module(kind)
    beside = far = 0
    for c in cases:
        for b, flow, (x, y, t, p) in F._flow_samples(c):
            for d in M.DIRECTIONS:
                keep = F.flow_kept(c, b, d)
                if not keep.any():
                    continue
                with np.errstate(all="ignore"):
                    tau = M.time_constants(t, d, True)[1][keep].astype(np.float64)
                assert tau.min() >= 0.0 and tau.max() <= 1.0, c["desc"]          # tau w in the fixed-point range [-1, 1]
                out = (x > c["W"] - 1) | (x < 0) | (y > c["H"] - 1) | (y < 0)
                beside += bool((keep & out).any())
                far += bool((keep & (np.abs(x) == 1e4)).any())
    assert beside >= 10 and far == 0, (beside, far)


def test_flow_cases_have_a_gradient_to_compare(flow_cases):
    """The cases whose reference gradient is identically zero are few, and empty by design: every sample of theirs has at most two
    events (one event: dt = 0; two: one has tau = 0 and the other dt = 0), equal time stamps (D = 0), or a strong field; for the
    timestamp loss also two distinct time stamps, which is the two-event sample many times over: the group that moves has tau = 0
    and the group with tau > 0 has dt = 0, so there is a gradient only where the one lands beside the other."""
    F, kind, cases, refs = flow_cases
    without = [c for c, r in zip(cases, refs) if not any(g.any() for _, g in r)]
    assert len(without) <= 0.10 * len(cases), (len(without), [c["desc"] for c in without])
    for c in without:
        assert c["fk"] == "strong" or all(n <= 2 or tk == "equal" or (tk == "two" and kind == "flowts") for n, tk in zip(c["ns"], c["tks"])), c["desc"]
    # D = 0 with events on the canvas: the contrast loss has a value there, and its gradient is exactly zero
    assert any(l != 0.0 and not g.any() for c, r in zip(cases, refs) for (l, g), tk in zip(r, c["tks"]) if tk == "equal") == (kind == "flowcm")


@pytest.fixture(scope="module")
def segment_cases():
    F = _fuzz()
    cases = [F.segment_inputs(rng) for rng in _rngs("segment")]
    return F, cases, [F.segment_reference(c) for c in cases]


def test_segment_generator_draws_every_class(segment_cases):
    F, cases, refs = segment_cases
    from event_utils_amd import _lib
    Z = F._t("_zhu_np")
    lib = _lib.lib()
    for key, values in (("model", Z.MODELS), ("L", range(1, 9)), ("f64", [False, True]), ("ck", F.SEG_CANVASES), ("n", F.SEG_N),
                        ("prk", F.SEG_PROBS), ("pdev", [False, True]), ("polk", F.SEG_POLS), ("use_polarity", [False, True]),
                        ("bk", F.SEG_BLURS), ("mk", F.SEG_MOTIONS)):
        _drawn(cases, key, values)
    assert {c["model"] for c in cases if c["L"] not in (1, 3)} == set(Z.MODELS)              # all five models at L other than 3
    assert all(c["cols"][0].dtype == (np.float64 if c["f64"] else np.float32) for c in cases)
    # the canvases, as evk_seg_band_rows sees them
    for c in cases:
        H, W = c["img_size"]
        rows = lib.evk_seg_band_rows(c["L"], 0, H + 1, W + 1)
        assert rows == c["rows"] and lib.evk_seg_band_rows(c["L"], _lib.EVK_IWE_DIRECT, H + 1, W + 1) == 0
        assert (c["ck"] == "no_band") == (rows == 0) and (c["ck"] != "one_band" or c["bands"] == 1)
        assert c["ck"] != "tiny" or (2 <= H <= 8 and 2 <= W <= 8)
        assert c["ck"] != "bands8" or (c["L"] == 8 and 8 <= H <= 16 and W in (256, 700, 900))
    assert {c["rows"] for c in cases if c["ck"] == "bands8"} == {2, 3, 9} and any(c["ck"] == "bands8" and c["img_size"][1] == 256 and c["bands"] == 2 for c in cases)
    assert any(c["ck"] == "tiny" and min(c["img_size"]) == 2 for c in cases) and any(c["ck"] == "tiny" and max(c["img_size"]) == 8 for c in cases)
    # the crosses: every residue of n mod 4 with several clusters (rows of probs off 16-byte alignment), also on float64 columns;
    # several chunks; several bands; several chunks of several bands
    assert {c["n"] % 4 for c in cases if c["L"] > 1 and c["n"] > 4} == {0, 1, 2, 3}
    assert {c["n"] % 4 for c in cases if c["L"] > 1 and c["f64"] and c["n"] > 4} >= {1, 2, 3}
    assert sum(c["chunks"] >= 2 for c in cases) >= 5 and sum(c["bands"] >= 2 for c in cases) >= 20
    assert any(c["chunks"] >= 2 and c["bands"] >= 2 for c in cases) and any(c["chunks"] >= 2 and c["n"] % 4 and c["L"] > 1 for c in cases)
    assert any(c["ck"] == "no_band" and c["n"] >= 1023 for c in cases)
    # the associations
    for c in cases:
        pr = c["probs"]
        assert (pr is None) == (c["prk"] == "none")
        if pr is not None:
            assert pr.dtype == np.float32 and pr.shape == (c["L"], c["n"]) and pr.min(initial=0) >= 0 and pr.max(initial=0) <= 1
            if c["prk"] == "one_hot":
                assert set(np.unique(pr)) <= {0.0, 1.0} and (pr.sum(axis=0) == 1).all()
            if c["prk"] == "zero_row":
                assert c["L"] > 1 and (~pr.any(axis=1)).sum() == (1 if c["n"] else c["L"])
            if c["prk"] == "zeros" and c["n"] >= 1023:
                assert (pr == 0).any() and pr.any()
    assert all(np.isnan(c["cols"][3]).sum() == (c["polk"] == "nan") for c in cases)
    assert any(c["polk"] == "pm1z" and (c["cols"][3] == 0).any() for c in cases)
    # events that leave the canvas under some clusters only; events that straddle a band edge in the bands of two and three rows
    some, straddle = 0, []
    for c, r in zip(cases, refs):
        if c["n"] == 0:
            continue
        kw = dict(img_size=c["img_size"], center=c["center"], camera_matrix=c["K"], f32_coords=True)
        with np.errstate(all="ignore"):
            masks = np.stack([Z.mask(c["model"], q, *c["cols"], **kw) for q in c["q"]])
        some += bool((masks.any(axis=0) & ~masks.all(axis=0)).any())
        if c["ck"] == "bands8" and c["rows"] in (2, 3) and masks[0].any():
            with np.errstate(all="ignore"):
                py = Z._events(c["model"], c["q"][0], *c["cols"], c["img_size"], c["img_size"], c["center"], c["K"], True)[0][1]
            straddle.append(np.mean((py + 1) % c["rows"] == 0))
    assert some >= 20, some
    assert len(straddle) >= 5 and max(straddle) >= 0.3, straddle


def test_segment_cases_have_something_to_compare(segment_cases):
    """Few cases have an identically zero reference gradient, and those hold a handful of events (at most 5: one event has
    dt = 0, a few may all miss the canvas or each other) or only zero associations; most assignment steps have rows that are set
    and rows that are kept."""
    F, cases, refs = segment_cases
    without = [c for c, r in zip(cases, refs) if not r["grad"].any()]
    assert len(without) <= 0.10 * len(cases), (len(without), [c["desc"] for c in without])
    assert all(c["n"] <= 5 for c in without), [c["desc"] for c in without]
    assert any(r["loss"] != 0.0 and not r["grad"][l].any() and not r["planes"][l].any() for c, r in zip(cases, refs) if c["prk"] == "zero_row"
               for l in range(c["L"]))                                             # an empty plane beside planes that are not
    sure = [(r["S"] >= 0.02 * np.abs(r["blurred"]).max()) & (r["S"] > 0) for c, r in zip(cases, refs) if c["n"]]
    assert np.mean([s.any() for s in sure]) >= 0.8
    assert sum(r["zero"].any() and not r["zero"].all() for c, r in zip(cases, refs) if c["n"]) >= 20


# ---- raw: the EVT3 / EVT2 decoder ------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def raw_cases():
    F = _fuzz()
    cases = [F.raw_inputs(rng) for rng in _rngs("raw")]
    return F, cases, [F.raw_reference(c) for c in cases]


def _raw_calls(F, c, r):
    """(words, state that came in, restatement result) of every call of a case: the whole stream and each piece"""
    calls = [(c["words"], c["state"], r["whole"])]
    bounds, st = F.raw_bounds(c), c["state"]
    for (a, b), p in zip(zip(bounds, bounds[1:]), r["pieces"]):
        calls.append((c["words"][a:b], st, p))
        st = p[5]
    return calls


def test_raw_generator_draws_every_class(raw_cases):
    F, cases, refs = raw_cases
    from event_utils_amd import _lib
    C, S = _lib.EVK_RAW_CHUNK, _lib.EVK_RAW_SCAN_WIDTH
    for fmt in (3, 2):
        mine = [c for c in cases if c["fmt"] == fmt]
        _drawn(mine, "family", F.RAW_FAMILIES[fmt])
        _drawn([c for c in mine if c["family"] == "time_only"], "tk", F.RAW_TIME_ONLY)
        _drawn([c for c in mine if c["family"] == "late_time"], "lk", F.RAW_LATE)
        _drawn(mine, "nk", [k for k in F.RAW_N_CLASSES if k != "scan"])
        _drawn(mine, "form", F.RAW_FORMS)
        _drawn(mine, "ts", ["us", "seconds"])
        _drawn(mine, "policy", F.RAW_POLICIES)
        _drawn(mine, "sk", F.RAW_SENSORS)
        _drawn(mine, "stk", F.RAW_STATES)
        seen = {k for c in mine for k in c["cut_classes"]}
        assert seen == set(F.RAW_CUTS) - ({"vector_run", "loop_pair"} if fmt == 2 else set()), (fmt, seen)
        assert {len(c["cuts"]) for c in mine} == set(range(6))
        assert {c["n"] % 16 for c in mine if c["nk"] == "16k"} == {15, 0, 1}
        assert {c["n"] - C for c in mine if c["nk"] == "chunk"} == {-1, 0, 1}
        assert {c["off"] for c in mine if c["form"] == "u8view"} >= ({1, 3} if fmt == 3 else {1})    # EVT3: a view from an odd half word
    assert "dense_vectors" not in F.RAW_FAMILIES[2]
    # more chunks than the scan has lanes: at least one seed, at most two (the restatement walks a million words for each)
    scan = [c for c in cases if c["nk"] == "scan"]
    assert 1 <= len(scan) <= 2 and all(c["n"] > S * C and c["plain"] and c["family"] == "structured" for c in scan)
    assert {c["fmt"] for c in scan} == {3, 2}                                       # two seeds: one of each format
    assert all(c["n"] <= 5 * C for c in cases if c["nk"] != "scan") and np.median([c["n"] for c in cases]) <= 2 * C
    for c in cases:
        n, t = c["n"], F._raw_types(c["fmt"], c["words"])
        lo, hi = {"0": (0, 0), "1-15": (1, 15), "16k": (15, 129), "wave": (1021, 1027), "chunk": (C - 1, C + 1), "chunks": (2 * C, 5 * C),
                  "scan": (S * C + 1, (S + 2) * C)}[c["nk"]]
        assert lo <= n <= hi or (c["family"] == "dense_vectors" and 2 * C <= n <= 5 * C), c["desc"]
        assert c["cuts"] == sorted(c["cuts"]) and all(0 <= k <= n for k in c["cuts"]) and len(c["cuts"]) == len(c["cut_classes"])
        assert -(-n // c["chunk_words"]) <= F.RAW_MAX_PIECES
        for k, cls in zip(c["cuts"], c["cut_classes"]):
            if cls == "chunk_border":
                assert k == n or min(k % C, C - k % C) <= 1
            elif cls == "vector_run":
                assert t[k - 1] in (4, 5) and t[k] in (4, 5)
            elif cls == "loop_pair":
                assert any(i < k <= j for i, j in F.raw_loop_pairs(c["fmt"], c["words"]))
            elif cls == "twice":
                assert c["cuts"].count(k) >= 2
            elif cls == "first15":
                assert k <= 15
        # the families are what they say
        if c["family"] == "no_events":
            assert set(t.tolist()) <= ({0x0, 0x6, 0x8, 0xA} | set(F._t("_raw_streams").RESERVED3) if c["fmt"] == 3 else {0x8, 0xA} | set(F._t("_raw_streams").RESERVED2))
        if c["family"] == "late_time" and n:
            first = np.flatnonzero(t == 8)
            where = {"chunk0": lambda p: p < C, "later_chunk": lambda p: p >= C, "last_word": lambda p: p == n - 1}
            assert (len(first) == 0) if c["lk"] == "never" else where[c["lk"]](first[0]), c["desc"]
        if c["family"] == "time_only" and n >= 1000:
            assert 0.7 <= np.mean((t == 8) | (t == 6)) and 0.08 <= np.mean((t == 2) if c["fmt"] == 3 else (t <= 1)) <= 0.2
        if c["state"] is not None:
            y, base, pol, tl, th, loops, have = c["state"]
            assert y < 2048 and base < 1 << 16 and pol in (0, 1) and tl < 4096 and th < 1 << (12 if c["fmt"] == 3 else 28) and 0 <= loops <= 1 << 20
            assert have == (c["stk"] == "time")
    assert any(c["state"] is not None and c["state"][5] >= 1 << 16 and c["fmt"] == 3 and c["state"][6] for c in cases)
    assert any(c["state"] is not None and c["state"][5] == 1 << 20 for c in cases)
    # sensors: none, sizes that cut the stream, sizes wider than an int16, one that holds every 16-bit coordinate but 0xFFFF
    assert {c["sensor"] for c in cases if c["sk"] == "all"} == {(65535, 65535)} and all((c["sensor"] is None) == (c["sk"] == "none") for c in cases)
    assert any(c["sensor"] is not None and c["sensor"][1] > 32768 for c in cases) and any(c["sensor"] == (1, 1) for c in cases)
    # the pieces: shorter than a lane, shorter than a wave row, empty, empty in front of one that is not, five cuts; the files'
    # pieces below 16 words
    sizes = [(b - a, c) for c in cases if c["cuts"] for a, b in zip(F.raw_bounds(c), F.raw_bounds(c)[1:])]
    for fmt in (3, 2):
        own = [s for s, c in sizes if c["fmt"] == fmt]
        assert own.count(0) >= 5 and sum(0 < s < 16 for s in own) >= 5 and sum(16 <= s < 1024 for s in own) >= 5 and sum(s > C for s in own) >= 5
        assert sum(c["chunk_words"] < 16 and c["n"] > c["chunk_words"] for c in cases if c["fmt"] == fmt) >= 2
        assert any(c["chunk_words"] > c["n"] > 0 for c in cases if c["fmt"] == fmt)
    # the encoders' round trip: at least a third of the cases, both formats, with and without vectors, empty and long
    trips = [c for c in cases if c["rt"] is not None]
    assert 3 * len(trips) >= len(cases)
    for fmt in (3, 2):
        own = [c["rt"] for c in trips if c["fmt"] == fmt]
        assert {len(rt["cols"][0]) for rt in own} >= {0, 1, 4000} and (fmt == 2 or {rt["vectorize"] for rt in own} == {False, True})
        for rt in own:
            x, y, t, p = rt["cols"]
            assert (np.diff(t) >= 0).all() and x.min(initial=0) >= 0 and x.max(initial=0) < 2048 and y.max(initial=0) < 2048
            assert t.max(initial=0) < (1 << 34 if fmt == 2 else 1 << 62)
    assert any(rt["vectorize"] and {3, 4, 5} <= set((rt["words"] >> 12).tolist()) for rt in (c["rt"] for c in trips if c["fmt"] == 3))
    assert any(len(rt["cols"][2]) and int(rt["cols"][2][-1]) >> 24 > 0 for rt in (c["rt"] for c in trips if c["fmt"] == 3))


def test_raw_staging_round_is_the_kernels():
    F = _fuzz()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "event_utils_amd", "csrc", "evk_rawdecode.hip")).read()
    m = re.search(r"^constexpr int RAW_STAGE = (\d+);", src, re.M)
    assert m and int(m.group(1)) == F.RAW_STAGE == 4096
    assert re.search(r"^constexpr uint32_t RAW_LOOP_STEP = 4085;", src, re.M) and re.search(r"^constexpr int RAW_ITEMS = 16;", src, re.M)


def test_raw_restatement_results_cover_the_terms_of_the_summary(raw_cases):
    F, cases, refs = raw_cases
    from event_utils_amd import _lib
    C = _lib.EVK_RAW_CHUNK
    seen = dict.fromkeys(("loop_inside", "loop_across", "loop_across_counted", "back", "before_and_events", "negative_x", "wrap", "straddle",
                          "late_first_time", "no_time_word_behind_time", "no_time_word_behind_a_piece_with_time", "three_pieces_with_state",
                          "state_loops_shift_time", "threshold_on", "threshold_below", "negative_x_inside_a_wide_sensor_under_drop"), 0)
    bad_under = dict.fromkeys(F.RAW_POLICIES, 0)
    for c, r in zip(cases, refs):
        fmt, words, whole = c["fmt"], c["words"], r["whole"]
        t = F._raw_types(fmt, words)
        pairs = F.raw_loop_pairs(fmt, words)
        seen["loop_across"] += any(i < k <= j for i, j in pairs for k in c["cuts"])
        seen["back"] += whole[4][4] > 0
        seen["negative_x"] += bool(len(whole[0]) and whole[0].min() < 0)
        x = whole[0].astype(np.int64)
        seen["wrap"] += bool(c["family"] == "dense_vectors" and np.any((x[:-1] < 0) & (x[1:] >= 0) & (x[1:] < 12)))
        bad_under[c["policy"]] += whole[4][5] > 0
        if c["policy"] == "drop" and whole[4][5] > 0 and c["sensor"][1] > 32768:          # a signed box would drop these too
            seen["negative_x_inside_a_wide_sensor_under_drop"] += bool(((whole[0] < 0) & (whole[0].view(np.uint16) < c["sensor"][1])).any())
        seen["three_pieces_with_state"] += len(c["cuts"]) >= 2 and len({tuple(p[5]) for p in r["pieces"]}) >= 3
        seen["state_loops_shift_time"] += bool(fmt == 3 and c["state"] is not None and c["state"][5] > 0 and len(whole[2]) and whole[2][0] >> 24 >= c["state"][5])
        if fmt == 3:
            pos = np.flatnonzero(t == 8)
            step = (words[pos][:-1] & 0xFFF).astype(np.int64) - (words[pos][1:] & 0xFFF).astype(np.int64)
            seen["threshold_on"] += bool((step == 4085).any())
            seen["threshold_below"] += bool((step == 4084).any())
        calls = _raw_calls(F, c, r)
        for k, (w, st, ref) in enumerate(calls):
            have = bool(st is not None and st[6])
            own = F._raw_types(fmt, w) == 8
            inside = len(F.raw_loop_pairs(fmt, w))
            seen["loop_inside"] += ref[4][6] > 0 and inside > 0
            seen["loop_across_counted"] += k >= 2 and ref[4][6] > inside and any(p[5][6] and (F._raw_types(fmt, q) == 8).any() for q, _, p in calls[1:k])
            seen["before_and_events"] += ref[4][3] > 0 and ref[4][0] > 0
            seen["no_time_word_behind_time"] += have and not own.any() and ref[4][0] > 0
            seen["no_time_word_behind_a_piece_with_time"] += (k >= 2 and not own.any() and ref[4][0] > 0
                                                              and (F._raw_types(fmt, calls[k - 1][0]) == 8).any())
            seen["late_first_time"] += not have and own.any() and int(np.flatnonzero(own)[0]) >= C and ref[4][0] > 0
        # the emission rule by words: the restatement's count, then the staging rounds of the whole stream's chunks
        per = F.raw_word_events(fmt, words, c["state"] is not None and c["state"][6])
        assert int(per.sum()) == whole[4][0] + 0 and len(per) == c["n"], c["desc"]
        ends = np.concatenate(([0], np.cumsum(per)))
        for a in range(0, c["n"], C):
            out0, out1 = int(ends[a]), int(ends[min(a + C, c["n"])])
            if out1 - out0 <= F.RAW_STAGE:
                continue
            lanes = ends[np.minimum(np.arange(a, a + C + 16, 16), min(a + C, c["n"]))]
            for border in range(out0 + F.RAW_STAGE, out1, F.RAW_STAGE):
                seen["straddle"] += bool(np.any((lanes[:-1] < border) & (lanes[1:] > border)))
    assert all(seen.values()), seen
    assert all(bad_under.values()), bad_under
    assert seen["loop_inside"] >= 10 and seen["back"] >= 10 and seen["straddle"] >= 50 and seen["negative_x"] >= 5, seen


def test_raw_cases_have_events_to_compare(raw_cases):
    """At most 15 % of the cases decode to nothing (the empty stream, streams without time or without event words, a handful of
    words); every family that can emit has a case with more than 1000 events, in both formats."""
    F, cases, refs = raw_cases
    nothing = [c["desc"] for c, r in zip(cases, refs) if r["whole"][4][0] == 0]
    assert len(nothing) <= 0.15 * len(cases), (len(nothing), len(cases), nothing)
    most = {}
    for c, r in zip(cases, refs):
        key = (c["fmt"], c["family"], c["tk"], c["lk"])
        most[key] = max(most.get(key, 0), r["whole"][4][0])
    assert all(count == 0 for key, count in most.items() if key[1] == "no_events")
    for fmt in (3, 2):
        for family in F.RAW_FAMILIES[fmt]:
            assert family == "no_events" or max(v for k, v in most.items() if k[:2] == (fmt, family)) > 1000
