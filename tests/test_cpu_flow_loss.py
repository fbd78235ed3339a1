"""CPU (no GPU): the average-timestamp loss of a dense flow field -- the numpy restatement the GPU tests compare against
(tests/_flow_loss_np.py): its adjoint against central differences, a constant field against the pinned linear-flow restatement
(tests/_zhu_np.py), batches; and the library's new entry points: declared, exported, bound, plain C, refusing bad arguments."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _flow_loss_np as F
import _zhu_np as Z

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("evk_flowts_time_constants_f32", "evk_flowts_warp_f32", "evk_flowts_grad_f32")


# ---- (a) the adjoint is the derivative -------------------------------------------------------------------------------------
@pytest.mark.parametrize("direction", F.DIRECTIONS)
@pytest.mark.parametrize("integer", (False, True), ids=("float", "integer"))
@pytest.mark.parametrize("sigma", (0.0, 1.0))
def test_gradient_matches_central_differences(sigma, integer, direction):
    """Every one of the 2 x 24 x 32 components, float64, h = 1e-6: within 1e-5 of max |g| (the prototype measured 1.5e-6, these
    eight cases 1.4e-6 to 5.1e-6)."""
    flow, x, y, t, p = F.scene(24, 32, 3000, integer=integer, seed=3)
    _, g = F.loss_and_grad(flow, x, y, t, p, sigma, direction)
    assert np.abs(g).max() > 0
    h, num = 1e-6, np.zeros_like(g)
    for k in range(flow.size):
        fp, fm = flow.copy(), flow.copy()
        fp.reshape(-1)[k] += h
        fm.reshape(-1)[k] -= h
        num.reshape(-1)[k] = (F.loss(fp, x, y, t, p, sigma, direction) - F.loss(fm, x, y, t, p, sigma, direction)) / (2 * h)
    err = np.abs(num - g).max() / np.abs(g).max()
    print("sigma %g, %s coordinates, %s: max |fd - g| / max |g| = %.3g" % (sigma, "integer" if integer else "float", direction, err))
    assert err <= 1e-5


def test_both_directions_is_the_sum():
    flow, x, y, t, p = F.scene(24, 32, 3000, seed=4)
    lf, gf = F.loss_and_grad(flow, x, y, t, p, 1.0, "forward")
    lb, gb = F.loss_and_grad(flow, x, y, t, p, 1.0, "backward")
    l2, g2 = F.loss_and_grad(flow, x, y, t, p, 1.0, "both")
    assert l2 == lf + lb and np.array_equal(g2, gf + gb) and lf != lb
    assert F.loss(flow, x, y, t, p, 1.0, "both") == l2


# ---- (b) pinned to the pinned restatement ------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", (0.0, 2.0))
def test_constant_field_is_the_linear_flow(sigma):
    """A constant field (a, b) moves every event by (a, b) dt: _zhu_np's linear flow at v = (-a, -b).  The loss agrees to 1e-12
    relative (the four field weights sum to 1 within an ulp) and sum_pixels g[c] = -dloss/dv_c: each side sums the same 3000
    float64 terms in another order, hence rtol 1e-9 and the same share of sum |g|."""
    x, y, t, p = Z.scene(Z.LINVEL, n=3000)
    assert x.min() >= 0 and x.max() <= 239 and y.min() >= 0 and y.max() <= 179
    a, b = -Z.LV_START
    flow = np.empty((2, 180, 240))
    flow[0], flow[1] = a, b
    lz = Z.loss(Z.LINVEL, (-a, -b), x, y, t, p, sigma=sigma)
    gz = Z.grad(Z.LINVEL, (-a, -b), x, y, t, p, sigma=sigma)
    lf, gf = F.loss_and_grad(flow, x, y, t, p, sigma, "forward")
    assert lz > 0 and abs(lf - lz) <= 1e-12 * lz
    np.testing.assert_allclose(gf.sum(axis=(1, 2)), -gz, rtol=1e-9, atol=1e-9 * np.abs(gf).sum())
    np.testing.assert_allclose(F.planes(flow, x, y, t, p), Z.planes(Z.LINVEL, (-a, -b), x, y, t, p), rtol=0, atol=1e-12)


def test_f32_restatement_is_close_to_the_definition():
    """The float32 expressions (round trip included) move the planes by float32 rounding only, apart from events that change
    cell: the sums over each plane agree to 1e-5 relative."""
    flow, x, y, t, p = F.scene(24, 32, 3000, seed=5)
    a, b = F.planes(flow, x, y, t, p), F.planes(flow, x, y, t, p, f32_coords=True)
    np.testing.assert_allclose(b.sum(axis=(1, 2)), a.sum(axis=(1, 2)), rtol=1e-5)
    xw, yw = F.warp(flow, x, y, t, f32_coords=True)
    assert xw.dtype == np.float32
    assert np.array_equal(F.planes(flow, x, y, t, p, f32_coords=True, warped=(xw, yw)), b)


# ---- (c) batches and the edge cases --------------------------------------------------------------------------------------------
def test_batch_of_three_with_an_empty_sample():
    flows, cols, offsets = [], [], [0]
    for n, seed in ((3001, 6), (0, 7), (517, 8)):
        flow, x, y, t, p = F.scene(24, 32, n, seed=seed)
        flows.append(flow)
        cols.append((x, y, t, p))
        offsets.append(offsets[-1] + n)
    x, y, t, p = (np.concatenate([c[k] for c in cols]) for k in range(4))
    for direction in ("forward", "both"):
        losses, grads = F.batch_loss_and_grad(np.stack(flows), x, y, t, p, offsets, 1.0, direction)
        for b in range(3):
            one, g = F.loss_and_grad(flows[b], *cols[b], 1.0, direction)
            assert losses[b] == one and np.array_equal(grads[b], g)
        assert losses[1] == 0 and not grads[1].any() and losses[0] > 0 and losses[2] > 0
    assert not F.planes(flows[1], *cols[1]).any()


def test_a_single_event_has_tau_zero():
    flow = np.zeros((2, 24, 32))
    one = (np.array([5.5]), np.array([7.25]), np.array([0.3]), np.array([1.0]))
    for direction in F.DIRECTIONS:
        pl = F.planes(flow, *one, direction=direction)
        assert not pl[0].any() and pl[1].sum() == 1.0
        assert F.loss_and_grad(flow, *one, 1.0, direction)[0] == 0


# ---- (d) library entry points --------------------------------------------------------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    from event_utils_amd.csrc import build
    build.build(verbose=False)
    from event_utils_amd import _lib
    text = open(os.path.join(ROOT, "include", "evk.h")).read()
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert hasattr(L, name), name
        assert _lib.PROTOTYPES[name][1] is ctypes.c_int, name
    assert (_lib.EVK_FLOWTS_FORWARD, _lib.EVK_FLOWTS_BACKWARD) == (0, 1)
    assert "2^-k <= 4 M D n 2^-61" in text          # the quantisation bound of the gradient is written down


def test_prototypes_compile_from_c(tmp_path):
    """The new prototypes are plain C99 and agree with the exported symbols' names: their addresses are taken through the
    declared types, and an entry is called through its prototype with arguments it must refuse."""
    from event_utils_amd import _lib
    if shutil.which("gcc") is None:
        pytest.skip("no gcc")
    src = tmp_path / "use_flowts.c"
    src.write_text(r"""
#include <dlfcn.h>
#include <stdio.h>
#include "evk.h"
typedef int (*tc_fn)(const float *, const int64_t *, int, int64_t, int, float *, void *);
int main(int argc, char **argv) {
    void *h = dlopen(argv[1], RTLD_NOW);
    if (!h) { fprintf(stderr, "%s\n", dlerror()); return 2; }
    tc_fn tc = (tc_fn)dlsym(h, "evk_flowts_time_constants_f32");
    if (!tc) return 3;
    tc_fn a = evk_flowts_time_constants_f32; (void)a;
    int (*b)(const float *, const float *, const float *, const float *, const int64_t *, int, int64_t, const float *, int, int,
             const float *, uint64_t *, float *, void *) = evk_flowts_warp_f32; (void)b;
    int (*c)(const float *, const float *, const float *, const float *, const int64_t *, int, int64_t, const float *, int, int,
             const float *, const float *, uint32_t *, int64_t *, float *, void *) = evk_flowts_grad_f32; (void)c;
    printf("%d|%d|%d\n", tc(0, 0, 1, 0, EVK_FLOWTS_FORWARD, 0, 0), EVK_FLOWTS_FORWARD, EVK_FLOWTS_BACKWARD);
    return 0;
}
""")
    exe = tmp_path / "use_flowts"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-ldl",
                    "-Wl,--unresolved-symbols=ignore-all"], check=True, capture_output=True)
    out = subprocess.run([str(exe), _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout.strip().split("|")
    assert [int(v) for v in out] == [-1, 0, 1]


def test_argument_errors_need_no_gpu():
    from event_utils_amd import _lib
    L = _lib.lib()
    fake, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4098)      # never dereferenced: every call below is refused first

    def tc(t=fake, off=fake, batch=1, n=8, direction=0, out=fake):
        return L.evk_flowts_time_constants_f32(t, off, batch, n, direction, out, None)
    assert tc(off=None) == -1 and tc(out=None) == -1 and tc(batch=0) == -1 and tc(batch=65536) == -1 and tc(n=-1) == -1
    assert tc(t=None) == -1 and tc(direction=2) == -1 and tc(direction=-1) == -1 and tc(t=odd) == -3

    def warp(x=fake, p=fake, off=fake, batch=1, n=8, flow=fake, h=24, w=32, tcs=fake, acc=fake, out=fake):
        return L.evk_flowts_warp_f32(x, fake, fake, p, off, batch, n, flow, h, w, tcs, acc, out, None)
    assert warp(x=None) == -1 and warp(p=None) == -1 and warp(off=None) == -1 and warp(batch=0) == -1 and warp(n=-1) == -1
    assert warp(flow=None) == -1 and warp(h=1) == -1 and warp(w=1) == -1 and warp(tcs=None) == -1 and warp(acc=None) == -1
    assert warp(out=None) == -1 and warp(x=odd) == -3

    def grad(x=fake, t=fake, off=fake, batch=1, n=8, flow=fake, h=24, w=32, tcs=fake, adj=fake, amax=fake, gacc=fake, out=fake):
        return L.evk_flowts_grad_f32(x, fake, t, fake, off, batch, n, flow, h, w, tcs, adj, amax, gacc, out, None)
    assert grad(x=None) == -1 and grad(t=None) == -1 and grad(off=None) == -1 and grad(batch=0) == -1 and grad(n=-1) == -1
    assert grad(flow=None) == -1 and grad(h=1) == -1 and grad(w=1) == -1 and grad(tcs=None) == -1 and grad(adj=None) == -1
    assert grad(amax=None) == -1 and grad(gacc=None) == -1 and grad(out=None) == -1 and grad(t=odd) == -3


def test_python_surface():
    import event_utils_amd as E
    from event_utils_amd import transforms
    from event_utils_amd.transforms import flow_loss
    for name in ("flow_field_timestamp_images", "flow_field_timestamp_loss", "flow_timestamp_loss"):
        assert getattr(E, name) is getattr(transforms, name) is getattr(flow_loss, name)
    flow = np.zeros((2, 24, 32), dtype=np.float32)
    cols = [np.zeros(4, dtype=np.float32)] * 4
    # refused before anything needs the device
    with pytest.raises(ValueError):
        E.flow_field_timestamp_loss(flow, *cols, direction="sideways")
    with pytest.raises(ValueError):
        E.flow_field_timestamp_loss(flow[0], *cols)
    with pytest.raises(ValueError):
        E.flow_field_timestamp_loss(np.zeros((3, 24, 32), dtype=np.float32), *cols)
    with pytest.raises(ValueError):
        E.flow_field_timestamp_loss(np.zeros((2, 2, 24, 32), dtype=np.float32), *cols)         # a batch without offsets
    with pytest.raises(ValueError):
        E.flow_field_timestamp_loss(flow, *cols, offsets=[0, 4])                                # offsets without a batch
    with pytest.raises(ValueError):
        E.flow_field_timestamp_images(flow, *cols, direction="both")
