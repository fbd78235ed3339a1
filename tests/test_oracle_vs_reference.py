"""CPU: the committed fixtures tests/golden/*.npz are what the REAL reference computes.
Every generator script under oracle/ (make_golden*.py) is re-run against the reference checkout -- imported through
oracle/ref_loader.py (EVK_REFERENCE_ROOT) -- with its `save` redirected into memory, and every array of every fixture must
come out bit for bit as committed.  Together with tests/test_oracle_golden.py (oracle == fixtures) this pins the oracle to
the reference.  The two regeneration tests are skipped where the reference checkout is absent; every other test here reads
committed fixtures only."""
import importlib
import os

import numpy as np
import pytest

from oracle import ref_loader

GENERATORS = ("make_golden", "make_golden_native", "make_golden_search", "make_golden_windows", "make_golden_classes")

needs_reference = pytest.mark.skipif(not ref_loader.available(), reason="the reference checkout is not on this machine")


@pytest.fixture(scope="module")
def regenerated():
    import warnings
    import torch
    threads = torch.get_num_threads()
    made = {}

    def capture(name, **arrs):
        made[name] = {k: np.asarray(v) for k, v in arrs.items()}
    import oracle.make_golden as base
    mods = [importlib.import_module("oracle." + g) for g in GENERATORS]
    saved = [(m, m.save) for m in mods]
    try:
        for m in mods:
            m.save = capture
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for m in mods:
                m.main()
    finally:
        for m, fn in saved:
            m.save = fn
        torch.set_num_threads(threads)
    assert base.save is saved[0][1]
    return made


@needs_reference
def test_every_committed_fixture_is_regenerated(regenerated):
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    committed = sorted(f[:-4] for f in os.listdir(golden) if f.endswith(".npz"))
    assert committed == sorted(regenerated), (committed, sorted(regenerated))


@needs_reference
def test_fixtures_reproduce_bit_for_bit_from_the_reference(regenerated):
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    checked = 0
    for name, arrs in sorted(regenerated.items()):
        g = np.load(os.path.join(golden, name + ".npz"))
        assert sorted(g.files) == sorted(arrs), name
        for k in g.files:
            a, b = g[k], arrs[k]
            assert a.dtype == b.dtype and a.shape == b.shape, (name, k, a.dtype, b.dtype, a.shape, b.shape)
            same = np.array_equal(a, b, equal_nan=True) if a.dtype.kind in "fc" else np.array_equal(a, b)
            assert same, (name, k)
            checked += 1
    assert checked > 250


def test_timestamp_image_with_a_nan_pixel_matches_the_reference(golden):
    """Round 6: scipy.stats.rankdata (image.py:371) propagates a NaN pixel to every rank; the oracle's dense rank (np.unique)
    is pinned to that behaviour by what the real class returns for two 12-pixel images (f18_timestamp_nan, regenerated from
    the reference above)."""
    from oracle import reference_np as R
    g = golden("f18_timestamp_nan")
    for tag, nanpix in (("nan", True), ("finite", False)):
        b = R.TimestampImage((3, 4))
        b.image[0, 0] = 5.0
        b.image[2, 1] = -1.0
        if nanpix:
            b.image[1, 2] = np.nan
        assert np.array_equal(b.image, g["image_" + tag], equal_nan=True)
        ga, gb = g["get_" + tag], b.get_image()
        assert ga.dtype == gb.dtype and np.array_equal(ga, gb, equal_nan=True) and bool(np.isnan(ga).all()) == nanpix
