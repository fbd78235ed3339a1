"""CPU (no GPU): the return code of every entry point of the per-pixel grouping family (evk_group.h, dn_open) for malformed calls
that are refused before anything is launched.  TABLE was recorded from the library of the commit before dn_open existed (run
this file as a script with EVK_LIB_PATH naming that library: it prints the table), never from the code under test: one statement
of the opening checks must answer every call as the eleven restatements did, including which of EINVAL and EALIGN wins where two
checks compete, and evk_reconstruct's EINVAL for a misaligned scratch."""
import ctypes

import pytest

OK, EINVAL, ESCRATCH, EALIGN = 0, -1, -2, -3
FAKE = ctypes.c_void_p(4096)                           # never dereferenced: every call below is refused first
OFF8 = ctypes.c_void_p(4096 + 8)                       # not 256-byte aligned
F32 = 3                                                # EVK_SELECT_F32

# the logical arguments of a well-formed call; an entry point takes the ones it has
GOOD = dict(kind=F32, t=FAKE, n=8, h=16, w=16, classes=2, scratch=FAKE, out=FAKE, select=None, rows=8, t_scratch=FAKE)


def _entries(L):
    """name -> (the logical arguments it has, the call)"""
    return {
        "evk_denoise_scratch_bytes": ("n h classes", lambda a: L.evk_denoise_scratch_bytes(a["n"], a["h"], a["w"], a["classes"])),
        "evk_denoise_group": ("t n h classes scratch", lambda a: L.evk_denoise_group(
            a["t"], a["t"], FAKE, a["n"], a["h"], a["w"], a["classes"], a["scratch"], 0, None, None)),
        "evk_denoise_support": ("kind t n h classes scratch out", lambda a: L.evk_denoise_support(
            a["kind"], a["t"], a["n"], a["h"], a["w"], a["classes"], 1.0, 1, 0, 0, 0, a["scratch"], a["out"], None, None)),
        "evk_denoise_refractory": ("kind t n h classes scratch out", lambda a: L.evk_denoise_refractory(
            a["kind"], a["t"], a["n"], a["h"], a["w"], a["classes"], 1.0, 0, a["scratch"], a["out"], None)),
        "evk_tsurf_check_sorted": ("kind t n out", lambda a: L.evk_tsurf_check_sorted(a["kind"], a["t"], a["n"], a["out"], None)),
        "evk_tsurf_global": ("kind t n h classes scratch out", lambda a: L.evk_tsurf_global(
            a["kind"], a["t"], a["n"], a["h"], a["w"], a["classes"], 1, FAKE, FAKE, 0, 1.0, a["scratch"], a["out"], None)),
        "evk_tsurf_local": ("kind t n h classes scratch out select", lambda a: L.evk_tsurf_local(
            a["kind"], a["t"], a["n"], a["h"], a["w"], a["classes"], 1, 0, 1.0, 0, 1, a["select"], a["rows"], a["scratch"], a["out"],
            None)),
        "evk_tsurf_hats": ("kind t n h scratch out t_scratch", lambda a: L.evk_tsurf_hats(
            a["kind"], a["t"], a["n"], a["h"], a["w"], 4, 1, 1.0, 1.0, 1, a["scratch"], a["t_scratch"], 0, a["out"], None, None)),
        "evk_corner_fast": ("kind t n h classes scratch out select", lambda a: L.evk_corner_fast(
            a["kind"], a["t"], a["n"], a["h"], a["w"], a["classes"], a["select"], a["rows"], a["scratch"], a["out"], None)),
        "evk_corner_harris": ("kind t n h classes scratch out select", lambda a: L.evk_corner_harris(
            a["kind"], a["t"], a["n"], a["h"], a["w"], a["classes"], 0, 4, 1.0, 0.04, a["select"], a["rows"], a["scratch"], a["out"],
            None)),
        "evk_planeflow_fit": ("kind t n h classes scratch out select", lambda a: L.evk_planeflow_fit(
            a["kind"], a["t"], a["n"], a["h"], a["w"], a["classes"], 1, 1.0, 3, 0, 0.0, 0, 0, 0.0, a["select"], a["rows"],
            a["scratch"], a["out"], None, FAKE if a["out"] else None, None)),
        "evk_planeflow_field": ("n h classes scratch out", lambda a: L.evk_planeflow_field(
            a["n"], a["h"], a["w"], a["classes"], a["scratch"], FAKE, FAKE, a["out"], FAKE, None)),
        "evk_reconstruct": ("kind t n h scratch out", lambda a: L.evk_reconstruct(
            a["kind"], a["t"], FAKE, a["n"], a["h"], a["w"], 0.5, 0.1, 0.1, 0.0, None, 0, None, None, 1, FAKE, FAKE, 0, 0,
            a["scratch"], a["out"], None)),
    }


# what is wrong with a call: name -> the logical arguments it changes.  An entry point takes a case when it has all of them.
SINGLE = {
    "null scratch": dict(scratch=None),
    "scratch at base + 8": dict(scratch=OFF8),
    "h = 0": dict(h=0),
    "classes = 3": dict(classes=3),
    "n = -1": dict(n=-1),
    "n = 2^31": dict(n=1 << 31),
    "t_kind = 5": dict(kind=5),
    "t_kind = -1": dict(kind=-1),
    "null t, n = 1": dict(t=None, n=1),
    "null output, one row": dict(out=None, rows=1),
    "selection, n = 0": dict(select=FAKE, rows=1, n=0, t=None),
    "null t_scratch": dict(t_scratch=None),
    "t_scratch at base + 8": dict(t_scratch=OFF8),
}
PAIRS = [("scratch at base + 8", other) for other in SINGLE if other not in ("null scratch", "scratch at base + 8")] + \
        [("null scratch", "t_kind = 5"), ("null scratch", "h = 0"), ("h = 0", "classes = 3"), ("n = -1", "t_kind = -1"),
         ("null output, one row", "t_kind = 5"), ("selection, n = 0", "null output, one row"),
         ("t_scratch at base + 8", "null output, one row")]
CASES = dict(SINGLE, **{"%s + %s" % (p, q): dict(SINGLE[p], **SINGLE[q]) for p, q in PAIRS})


def _calls(L):
    for entry, (has, call) in _entries(L).items():
        for case, change in CASES.items():
            if set(change) - {"rows"} <= set(has.split()):
                yield entry, case, call, dict(GOOD, **change)


# (entry point, case) -> the code the parent commit's library returned: EALIGN to the 20 calls below, EINVAL to the other 239
# (a misaligned scratch loses against every EINVAL check that stands before it: to all of them in the denoise, global and field
# entry points, to all but the row checks in the passes that take a selection, and always in evk_reconstruct)
RECORDED_EALIGN = {
    "evk_denoise_group": ["scratch at base + 8"],
    "evk_denoise_support": ["scratch at base + 8"],
    "evk_denoise_refractory": ["scratch at base + 8"],
    "evk_tsurf_global": ["scratch at base + 8"],
    "evk_tsurf_local": ["scratch at base + 8", "scratch at base + 8 + null output, one row", "scratch at base + 8 + selection, n = 0"],
    "evk_tsurf_hats": ["scratch at base + 8", "t_scratch at base + 8", "scratch at base + 8 + t_scratch at base + 8"],
    "evk_corner_fast": ["scratch at base + 8", "scratch at base + 8 + null output, one row", "scratch at base + 8 + selection, n = 0"],
    "evk_corner_harris": ["scratch at base + 8", "scratch at base + 8 + null output, one row",
                          "scratch at base + 8 + selection, n = 0"],
    "evk_planeflow_fit": ["scratch at base + 8", "scratch at base + 8 + null output, one row",
                          "scratch at base + 8 + selection, n = 0"],
    "evk_planeflow_field": ["scratch at base + 8"],
}
TABLE = {(e, c): EALIGN if c in RECORDED_EALIGN.get(e, ()) else EINVAL for e, c, _, _ in _calls(None)}


def test_the_table_is_the_recorded_one():
    assert len(TABLE) == 259 and sum(v == EALIGN for v in TABLE.values()) == 20 == sum(len(v) for v in RECORDED_EALIGN.values())


@pytest.mark.parametrize("entry,case", list(TABLE), ids=["%s: %s" % k for k in TABLE])
def test_malformed_calls_return_the_recorded_code(entry, case):
    from event_utils_amd import _lib
    has, call = _entries(_lib.lib())[entry]
    assert call(dict(GOOD, **CASES[case])) == TABLE[(entry, case)]


def test_a_bool_is_not_an_integer_parameter():
    """check_int is plane_flow's rule for every integer parameter of the family: True is no radius 1 (the denoising filters and
    the time surfaces took it before); refused on the arguments alone, before any device work"""
    import numpy as np
    import event_utils_amd as E
    from event_utils_amd._checks import check_int
    x, y, t, p = np.array([5, 6]), np.array([5, 6]), np.array([1.0, 2.0]), np.array([1, -1])
    with pytest.raises(ValueError, match="radius must be 1 .. 3"):
        E.neighbour_support(x, y, t, p, 1.0, radius=True)
    with pytest.raises(ValueError, match="radius must be 1 .. 3"):
        E.background_activity_filter(x, y, t, p, 1.0, radius=True)
    with pytest.raises(ValueError, match="radius must be 1 .. 4"):
        E.local_time_surfaces(x, y, t, p, 1.0, radius=True)
    with pytest.raises(ValueError, match="radius must be 1 .. 4"):
        E.averaged_time_surfaces(x, y, t, p, 1.0, 1.0, radius=True)
    with pytest.raises(ValueError, match="cell_size must be a positive integer"):
        E.averaged_time_surfaces(x, y, t, p, 1.0, 1.0, cell_size=True)
    assert check_int(2.0, "radius", 1, 3) == 2 and isinstance(check_int(2.0, "radius", 1, 3), int) and check_int(7, "n_last", 1) == 7
    for bad in (0, 4, 1.5, False):
        with pytest.raises(ValueError, match=r"radius must be 1 \.\. 3 \(got"):
            check_int(bad, "radius", 1, 3)


if __name__ == "__main__":                            # the recorder: EVK_LIB_PATH=<the parent's library> python tests/test_cpu_grouping.py
    from event_utils_amd import _lib
    for e, c, call, a in _calls(_lib.lib()):
        print("    (%r, %r): %d," % (e, c, call(a)))
