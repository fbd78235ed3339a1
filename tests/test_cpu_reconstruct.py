"""CPU (no GPU): the host restatement of the intensity reconstruction (tests/_reconstruct_np.py, the literal merged event-and-frame
loop) on hand-worked cases; evk_reconstruct is declared, bound and exported and refuses bad arguments before it touches the
device; the kernel of evk_reconstruct.hip compiles for gfx950 without register spills; the Python argument errors."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _header
import _reconstruct_np as N

SIZE = (2, 3)


def at(want, x=1, y=1):
    return [float(v) for v in want[:, y, x]]


def one(t, p=1, x=1, y=1):
    """columns of events at one pixel"""
    t = np.atleast_1d(np.asarray(t, dtype=np.float64))
    p = np.broadcast_to(np.asarray(p), t.shape)
    return np.full(len(t), x), np.full(len(t), y), t, p


def f32(v):
    return float(np.float32(v))


# ---- hand-worked cases ----------------------------------------------------------------------------------------------------------

def test_one_event_decays():
    alpha = 0.25
    want, A = N.seq_reconstruct(*one(2.0), alpha, SIZE, t_refs=[3.0, 6.0], c_on=0.5, c_off=0.3)
    assert want.dtype == np.float32 and want.shape == (2, 2, 3) and A.shape == (2, 2, 3)
    assert at(want) == [f32(0.5 * math.exp(-alpha * 1.0)), f32(0.5 * math.exp(-alpha * 1.0) * math.exp(-alpha * 3.0))]
    assert [float(v) for v in A[:, 1, 1]] == [0.5 * math.exp(-alpha * 1.0), 0.5 * math.exp(-alpha * 4.0)]
    assert not want[:, 0, :].any() and not want[:, 1, 0].any() and not A[:, 0, 0].any()      # the pixels without events
    want, _ = N.seq_reconstruct(*one(2.0, -1), alpha, SIZE, t_refs=[3.0], c_on=0.5, c_off=0.3)
    assert at(want) == [f32(-0.3 * math.exp(-alpha))]


def test_an_on_off_pair():
    alpha = 0.5
    want, A = N.seq_reconstruct(*one([1.0, 3.0], [1, -1]), alpha, SIZE, t_refs=[4.0], c_on=0.2, c_off=0.7)
    L = 0.2 * math.exp(-alpha * 2.0) - 0.7                 # the literal recurrence: decay to the second event, step, decay
    assert at(want) == [f32(L * math.exp(-alpha * 1.0))]
    assert abs(A[0, 1, 1] - (0.2 * math.exp(-1.5) + 0.7 * math.exp(-0.5))) < 1e-15
    # polarity is p > 0: 0 is an OFF event
    assert at(N.seq_reconstruct(*one([1.0, 3.0], [1, 0]), alpha, SIZE, t_refs=[4.0], c_on=0.2, c_off=0.7)[0]) == at(want)


def test_a_frame_step_response_tends_to_the_new_frame():
    frames = np.zeros((2, 2, 3))
    frames[0], frames[1] = 1.0, 3.0
    none = one([])
    want, A = N.seq_reconstruct(*none, 0.5, SIZE, t_refs=[5.0, 10.0, 12.0, 20.0, 200.0], frames=frames, frame_ts=[0.0, 10.0])
    # initial = frames[0], t_start = 0: nothing moves until the second frame; a frame AT a query time has not acted yet
    got = at(want)
    assert got[:2] == [1.0, 1.0]
    at12 = 3.0 + (1.0 - 3.0) * math.exp(-0.5 * 2.0)
    assert got[2] == f32(at12) and got[3] == f32(3.0 + (at12 - 3.0) * math.exp(-0.5 * 8.0))
    assert got[4] == 3.0 and (A == 4.0).all()
    # before frame_ts[0] frames[0] holds already, and frames[F - 1] holds for ever
    want, _ = N.seq_reconstruct(*none, 0.5, SIZE, t_refs=[-2.0, 0.0], frames=frames, frame_ts=[0.0, 10.0], initial=np.zeros(SIZE),
                                t_start=-4.0)
    assert at(want) == [f32(1.0 - math.exp(-1.0)), f32(1.0 + ((1.0 - math.exp(-1.0)) - 1.0) * math.exp(-1.0))]


def test_an_event_exactly_at_a_query_time_is_excluded():
    want, A = N.seq_reconstruct(*one([1.0, 2.0, 2.0]), 0.0, SIZE, t_refs=[2.0, 2.0, 2.5], c_on=1.0)
    assert at(want) == [1.0, 1.0, 3.0] and [float(v) for v in A[:, 1, 1]] == [1.0, 1.0, 3.0]
    # with indices the first m_k events count and T_k = ts[m_k - 1]
    want, _ = N.seq_reconstruct(*one([1.0, 2.0, 2.0]), 0.5, SIZE, indices=[0, 1, 2, 3], c_on=1.0)
    assert at(want) == [0.0, 1.0, f32(math.exp(-0.5) + 1.0), f32(math.exp(-0.5) + 1.0 + 1.0)]


def test_a_frame_exactly_at_an_event_time():
    frames = np.zeros((2, 2, 3))
    frames[1] = 2.0
    alpha = 0.25
    want, _ = N.seq_reconstruct(*one(4.0), alpha, SIZE, t_refs=[6.0], c_on=0.5, frames=frames, frame_ts=[0.0, 4.0])
    # up to t = 4 the target is frames[0] = 0 = initial; the step and the new target both act from t = 4
    assert at(want) == [f32(2.0 + (0.5 - 2.0) * math.exp(-alpha * 2.0))]
    assert at(want, 0, 0) == [f32(2.0 - 2.0 * math.exp(-alpha * 2.0))]


def test_events_before_t_start_are_ignored():
    cols = one([1.0, 2.0, 3.0, 5.0])
    want, A = N.seq_reconstruct(*cols, 0.5, SIZE, t_refs=[6.0], c_on=1.0, t_start=3.0, initial=np.full(SIZE, 4.0))
    L = (4.0 + 1.0) * math.exp(-0.5 * 2.0) + 1.0           # the event AT t_start counts
    assert at(want) == [f32(L * math.exp(-0.5))]
    assert abs(A[0, 1, 1] - (4.0 + math.exp(-1.5) + math.exp(-0.5))) < 1e-15
    assert at(want, 0, 0) == [f32(4.0 * math.exp(-1.5))]


@pytest.mark.parametrize("seed", range(6))
def test_complementary_is_high_pass_plus_the_low_pass_of_the_frames(seed):
    rng = np.random.default_rng(seed)
    H, W, n = 3, 4, 400
    t = np.sort(rng.integers(0, 2_000, n)).astype(np.float64)
    x, y, p = rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n) * 2 - 1
    frames = rng.normal(size=(4, H, W))
    fts = [100.0, float(t[n // 3]), 1_200.5, 1_700.0]
    refs = [150.0, float(t[n // 2]), 1_500.0, 2_100.0]
    kw = dict(c_on=0.23, c_off=0.17)
    alpha = [1 / 400.0, 1 / 50.0, 0.0][seed % 3]
    full, A = N.seq_reconstruct(x, y, t, p, alpha, (H, W), t_refs=refs, frames=frames, frame_ts=fts, **kw)
    high, _ = N.seq_reconstruct(x, y, t, p, alpha, (H, W), t_refs=refs, t_start=100.0, **kw)
    low, _ = N.seq_reconstruct(x[:0], y[:0], t[:0], p[:0], alpha, (H, W), t_refs=refs, frames=frames, frame_ts=fts)
    err = np.abs(full.astype(np.float64) - (high.astype(np.float64) + low.astype(np.float64)))
    # three float32 roundings (full, high, low) on top of the 2^-40 A of the float64 orders
    assert (err <= 2.0 ** -40 * A + 3 * 2.0 ** -24 * A).all()
    if alpha == 0.0:                                       # the frames have no influence: the start state stays
        assert np.array_equal(low, np.broadcast_to(frames[0].astype(np.float32), low.shape))


def test_direct_integration_gives_integer_sums():
    rng = np.random.default_rng(11)
    H, W, n = 4, 5, 600
    t = np.sort(rng.integers(0, 300, n)).astype(np.float64)
    x, y, p = rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n) * 2 - 1
    want, A = N.seq_reconstruct(x, y, t, p, 0.0, (H, W), indices=[n // 2, n], c_on=1.0, c_off=1.0)
    for k, m in enumerate((n // 2, n)):
        img = np.zeros((H, W))
        np.add.at(img, (y[:m], x[:m]), p[:m])
        cnt = np.zeros((H, W))
        np.add.at(cnt, (y[:m], x[:m]), 1)
        assert np.array_equal(want[k], img.astype(np.float32)) and np.array_equal(A[k], cnt)


# ---- the public surface and the C ABI -----------------------------------------------------------------------------------------

def test_the_prototype_is_bound_with_its_arguments():
    from event_utils_amd import _lib
    protos = _header.prototypes("evk_reconstruct")
    assert set(protos) == {"evk_reconstruct"}
    assert _lib.PROTOTYPES["evk_reconstruct"] == protos["evk_reconstruct"] and protos["evk_reconstruct"][1] is ctypes.c_int
    assert hasattr(_lib.lib(), "evk_reconstruct")
    assert _lib.EVK_RECONSTRUCT_WAVE_RUN == 1024
    assert re.search(r"^#define\s+EVK_RECONSTRUCT_WAVE_RUN\s+1024\s*$", _header.TEXT, re.M)


def test_public_surface():
    import event_utils_amd as E
    import event_utils_amd.lib.representations.reconstruction as alias
    from event_utils_amd import representations
    from event_utils_amd.representations import reconstruction
    assert alias is reconstruction
    for name in ("leaky_integrator", "complementary_filter", "log_intensity", "to_intensity"):
        assert getattr(E, name) is getattr(reconstruction, name) is getattr(representations, name)
    assert "representations.reconstruction" in E.__doc__
    assert "initial=out[-1]" in E.leaky_integrator.__doc__ and "t_start" in E.leaky_integrator.__doc__


def test_the_intensity_helpers():
    import torch
    import event_utils_amd as E
    img = np.array([[0, 1, 128, 255]], dtype=np.uint8)
    L = E.log_intensity(img)
    assert isinstance(L, np.ndarray) and L.dtype == np.float64 and np.allclose(L, np.log(img.astype(np.float64) + 1e-3), rtol=1e-15)
    assert np.allclose(E.to_intensity(L), img, atol=1e-12)
    Lt = E.log_intensity(torch.from_numpy(img), eps=0.5)
    assert isinstance(Lt, torch.Tensor) and Lt.dtype == torch.float64 and np.allclose(Lt.numpy(), np.log(img + 0.5), rtol=1e-15)
    back = E.to_intensity(Lt.to(torch.float32), eps=0.5)
    assert back.dtype == torch.float32 and np.allclose(back.numpy(), img, rtol=1e-6, atol=1e-6)


def test_arguments_are_refused_before_the_device_is_touched():
    from event_utils_amd import _lib
    L = _lib.lib()
    fake = ctypes.c_void_p(4096)                       # never dereferenced: every call below is refused first
    einval, f32k, nan, inf = -1, _lib.EVK_SELECT_F32, float("nan"), float("inf")

    def rec(kind=f32k, t=fake, pos=fake, n=8, h=16, w=16, alpha=0.5, c_on=0.1, c_off=0.1, t_start=0.0, initial=None, nf=0,
            frames=None, frame_ts=None, nq=2, cuts=fake, t_refs=fake, start_cut=0, wave_run=0, scratch=fake, out=fake):
        return L.evk_reconstruct(kind, t, pos, n, h, w, alpha, c_on, c_off, t_start, initial, nf, frames, frame_ts, nq, cuts, t_refs,
                                 start_cut, wave_run, scratch, out, None)
    assert rec(kind=-1) == einval and rec(kind=5) == einval
    assert rec(n=-1) == einval and rec(n=1 << 31) == einval and rec(h=0) == einval and rec(w=-3) == einval
    assert rec(h=1 << 16, w=1 << 16) == einval          # more keys than a grouping holds
    assert rec(t=None) == einval and rec(pos=None) == einval and rec(scratch=None) == einval and rec(out=None) == einval
    assert rec(cuts=None) == einval and rec(t_refs=None) == einval
    assert rec(n=0, t=None, pos=None, scratch=None) == einval
    assert rec(nq=0) == einval and rec(nq=-1) == einval
    assert rec(alpha=-1e-300) == einval and rec(alpha=nan) == einval and rec(alpha=inf) == einval
    for bad in (0.0, -0.1, nan, inf):
        assert rec(c_on=bad) == einval and rec(c_off=bad) == einval
    assert rec(t_start=nan) == einval
    assert rec(nf=-1) == einval and rec(nf=2, frames=fake) == einval and rec(nf=2, frame_ts=fake) == einval and rec(nf=2) == einval
    assert rec(start_cut=-1) == einval and rec(start_cut=9) == einval
    assert rec(scratch=ctypes.c_void_p(4100)) == einval          # not 256-byte aligned


def test_the_kernel_compiles_without_register_spills(tmp_path):
    """Every instantiation of k_reconstruct (one per time-column kind) compiles for gfx950 without spilling registers."""
    import shutil
    import subprocess
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not (os.path.isfile(hipcc) or shutil.which(hipcc)):
        pytest.skip("no hipcc")
    from event_utils_amd.csrc import build as B
    src = os.path.join(B.HERE, "evk_reconstruct.hip")
    subprocess.run([hipcc] + list(B.CFLAGS) + ["-c", src, "-o", str(tmp_path / "rc.o"), "-save-temps=obj"], check=True, cwd=B.HERE,
                   stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    asm = [f for f in os.listdir(tmp_path) if f.endswith("gfx950.s")]
    assert asm, os.listdir(tmp_path)
    text = open(tmp_path / asm[0]).read()
    kernels = re.findall(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", text)
    seen = {n: (int(v), int(sp)) for n, v, sp in kernels}
    assert sum("k_reconstruct" in n for n in seen) == 5
    assert not {n: vs for n, vs in seen.items() if vs[1]}


def test_python_argument_errors_come_before_any_device_work():
    """every call below is refused on its arguments alone: none of them reaches the point where a missing GPU would matter"""
    import event_utils_amd as E
    x, y, t, p = np.array([5, 6]), np.array([5, 6]), np.array([1.0, 2.0]), np.array([1, -1])
    size = (8, 9)
    frames, fts = np.zeros((2, 8, 9)), [0.0, 1.5]

    def both(match, alpha=0.5, **kw):
        kw = dict(dict(sensor_size=size, t_refs=[3.0]), **kw)
        with pytest.raises(ValueError, match=match):
            E.leaky_integrator(x, y, t, p, alpha, **kw)
        kw.setdefault("frames", frames), kw.setdefault("frame_ts", fts)
        with pytest.raises(ValueError, match=match):
            E.complementary_filter(x, y, t, p, alpha, kw.pop("frames"), kw.pop("frame_ts"), **kw)
    for bad in (-1.0, float("nan"), float("inf")):
        both("alpha", alpha=bad)
    for bad in (0.0, -0.1, float("nan")):
        both("c_on", c_on=bad)
        both("c_off", c_off=bad)
    both("exactly one", t_refs=None)
    both("exactly one", indices=[1])
    both("non-decreasing", t_refs=[3.0, 2.5])
    both("non-decreasing", t_refs=None, indices=[2, 1])
    both("at least one", t_refs=[])
    both("before t_start", t_start=3.5)
    both("finite", t_refs=[float("nan")])
    both("initial", initial=np.zeros((9, 8)))
    both("initial", initial=np.zeros((1, 8, 9)))
    both("sensor_size", sensor_size=(0, 9))
    for bad_frames, bad_ts, match in ((np.zeros((2, 9, 8)), fts, "frames"), (np.zeros((3, 8, 9)), fts, "frames"),
                                      (np.zeros((8, 9)), [0.0], "frames"), (frames, [1.5, 0.0], "increasing"),
                                      (frames, [1.0, 1.0], "increasing"), (np.zeros((0, 8, 9)), [], "frames"),
                                      (frames, None, "frame_ts"), (None, fts, "frame_ts")):
        with pytest.raises(ValueError, match=match):
            E.complementary_filter(x, y, t, p, 0.5, bad_frames, bad_ts, sensor_size=size, t_refs=[3.0])
    with pytest.raises(ValueError, match="before t_start"):      # the default t_start of the complementary filter: frame_ts[0]
        E.complementary_filter(x, y, t, p, 0.5, frames, [2.5, 4.0], sensor_size=size, t_refs=[2.0])
