"""GPU: the contrast (focus) loss of a dense flow field (flow_field_iwe / flow_field_contrast_loss / flow_contrast_loss)
against its float64 numpy restatement (tests/_flow_contrast_np.py, pinned by tests/test_cpu_flow_contrast.py) and against
variance_objective on the linear flow.

Every comparison with the restatement hands it the warped coordinates warp_events_flow_torch returns for the same inputs
(warped=): the per-pixel slope is discontinuous at pixel edges, so both sides must put every event in the same cell.  Tolerances
are those of tests/test_gpu_flow_loss.py: image atol = 1e-6 x its maximum, loss rtol = 1e-4, gradient rtol = 1e-4 with atol =
1e-4 max|g_ref|.  Loss comparisons are made where the restatement's var(B) >= 1e-2 mean(B)^2, so that the float32 storage of B
(6e-8 relative, up to 100 times that in the variance) stays far inside the loss tolerance; each such test asserts it."""
import numpy as np
import pytest
import torch

import _flow_contrast_np as C
import _zhu_np as Z

pytestmark = pytest.mark.gpu

SMALL = (24, 32)
N_SMALL = 3001          # not a multiple of the wave (64) or of the block (256)
GD_STEP = 5.0e4         # chosen on the restatement: 20 steps take the loss from -0.19348 to -0.86562, each by at least 5.7 %
VO_SEED = 0             # the linear-flow scene of test_constant_field_is_the_variance_objective


def _f32(cols):
    return tuple(np.asarray(a, dtype=np.float32) for a in cols)


def _scene(n=N_SMALL, integer=False, seed=11, shape=SMALL, speed=60.0):
    flow, x, y, t, p = C.scene(shape[0], shape[1], n, integer=integer, seed=seed, speed=speed)
    return flow.astype(np.float32), _f32((x, y, t, p))


def _directions(direction):
    return C.DIRECTIONS if direction == "both" else (direction,)


def _warped(flow, cols, direction):
    """What warp_events_flow_torch returns for these inputs, per direction of the loss (numpy float32)."""
    import event_utils_amd as E
    x, y, t, p = (torch.from_numpy(a) for a in cols)
    out = []
    for d in _directions(direction):
        t0 = float(cols[2][-1] if d == "forward" else cols[2][0])
        xw, yw = E.transforms.warp_events_flow_torch(x, y, t, p, torch.from_numpy(flow), t0=t0)
        out.append((xw.numpy(), yw.numpy()))
    return tuple(out) if direction == "both" else out[0]


def _assert_measurable(flow, cols, sigma, direction, warped, **kw):
    """var(B) >= 1e-2 mean(B)^2 on the restatement, per direction (computed on the CPU)."""
    pairs = zip(C.DIRECTIONS, warped) if direction == "both" else ((direction, warped),)
    for d, w in pairs:
        b = C.blur(C.iwe(flow, *cols, direction=d, f32_coords=True, warped=w, **kw), sigma)
        assert b.var() >= 1e-2 * b.mean() ** 2, (d, b.var(), b.mean() ** 2)


def _oracle(flow, cols, sigma, objective, direction, use_polarity=True, p_scale=1.0):
    warped = _warped(flow, cols, direction)
    _assert_measurable(flow, cols, sigma, direction, warped, use_polarity=use_polarity, p_scale=p_scale)
    return C.loss_and_grad(flow, *cols, sigma, objective, direction, f32_coords=True, warped=warped, p_scale=p_scale,
                           use_polarity=use_polarity)


def _np(a):
    return a.detach().cpu().numpy().astype(np.float64)


def _close_image(got, ref):
    got = _np(got)
    assert got.shape == ref.shape
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-6 * max(np.abs(ref).max(), 1e-30))


def _close_loss(got, ref):
    got = float(got)
    assert abs(got - ref) <= 1e-4 * abs(ref), (got, ref)


def _close_grad(g, ref):
    assert np.abs(ref).max() > 0
    np.testing.assert_allclose(_np(g), ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


def _check_against_oracle(flow, cols, sigma, objective, direction, use_polarity=True):
    import event_utils_amd as E
    kw = dict(objective=objective, blur_sigma=sigma, direction=direction, use_polarity=use_polarity)
    loss, grad = E.flow_field_contrast_loss(flow, *cols, compute_gradient=True, **kw)
    assert loss.is_cuda and loss.dtype == torch.float64 and loss.dim() == 0
    assert grad.is_cuda and grad.dtype == torch.float32 and tuple(grad.shape) == flow.shape
    ref_loss, ref_grad = _oracle(flow, cols, sigma, objective, direction, use_polarity)
    err = np.abs(_np(grad) - ref_grad).max() / np.abs(ref_grad).max()
    print("loss %.9g (restatement %.9g), max |g - g_ref| / max |g_ref| = %.3g" % (float(loss), ref_loss, err))
    _close_loss(loss, ref_loss)
    _close_grad(grad, ref_grad)
    value = E.flow_field_contrast_loss(flow, *cols, **kw)
    assert float(value) == float(loss)                      # the value alone: the same bits
    return loss, grad


# ---- image, loss and gradient against the restatement --------------------------------------------------------------------------
@pytest.mark.parametrize("use_polarity", (True, False), ids=("signed", "abs"))
@pytest.mark.parametrize("integer", (False, True), ids=("float", "integer"))
@pytest.mark.parametrize("sigma", (0.0, 1.0))
@pytest.mark.parametrize("direction", ("forward", "backward", "both"))
@pytest.mark.parametrize("objective", C.OBJECTIVES)
def test_image_loss_and_gradient_match_the_restatement(objective, direction, sigma, integer, use_polarity):
    import event_utils_amd as E
    flow, cols = _scene(integer=integer)
    loss, grad = _check_against_oracle(flow, cols, sigma, objective, direction, use_polarity)
    kw = dict(objective=objective, blur_sigma=sigma, use_polarity=use_polarity, compute_gradient=True)
    if direction == "both":
        parts = [E.flow_field_contrast_loss(flow, *cols, direction=d, **kw) for d in C.DIRECTIONS]
        assert float(loss) == float(parts[0][0] + parts[1][0]) and torch.equal(grad, parts[0][1] + parts[1][1])
        return
    ref = C.iwe(flow, *cols, direction=direction, f32_coords=True, warped=_warped(flow, cols, direction), use_polarity=use_polarity)
    assert 0 < np.abs(ref).sum() and C.kept(flow, *cols, direction, True, _warped(flow, cols, direction)).sum() < len(cols[0])
    img = E.flow_field_iwe(flow, *cols, direction=direction, use_polarity=use_polarity)
    assert img.is_cuda and img.dtype == torch.float32 and tuple(img.shape) == (SMALL[0] + 1, SMALL[1] + 1)
    _close_image(img, ref)


@pytest.mark.parametrize("objective", C.OBJECTIVES)
def test_the_minimal_field(objective):
    """A (2, 2) field, a (3, 3) canvas, 65 events: one block with one full wave and one lane of the next; the blur's radius (4)
    exceeds the canvas."""
    flow, cols = _scene(n=65, seed=12, shape=(2, 2), speed=8.0)
    for sigma in (0.0, 1.0):
        _check_against_oracle(flow, cols, sigma, objective, "both")


def test_a_blur_wider_than_the_fused_radius():
    """sigma 8.5: radius 34 > EVK_MAX_RADIUS, through evk_gaussian_filter_wide_f32, and wider than the canvas."""
    from event_utils_amd import _lib
    from event_utils_amd.contrast_max.objectives import _blur_kernel
    assert _blur_kernel(8.5)[1] > _lib.EVK_MAX_RADIUS
    flow, cols = _scene()
    _check_against_oracle(flow, cols, 8.5, "variance", "forward")


# ---- repeatability and the kinds of input --------------------------------------------------------------------------------------
def test_repeatable_and_the_same_bits_from_every_kind_of_input():
    import event_utils_amd as E
    flow, cols = _scene()
    for objective in C.OBJECTIVES:
        kw = dict(objective=objective, direction="both", compute_gradient=True)
        ref = E.flow_field_contrast_loss(flow, *cols, **kw)
        tens = tuple(torch.from_numpy(a).cuda() for a in cols)
        ev = E.DeviceEvents.from_arrays(*cols)
        padded = tuple(torch.cat((c.new_zeros(1), c))[1:] for c in tens)        # columns that start off a 16-byte boundary
        assert all(c.data_ptr() % 16 == 4 for c in padded)
        for args in (cols, tens, tens, (ev, None, None, None), padded):
            loss, grad = E.flow_field_contrast_loss(torch.from_numpy(flow).cuda(), *args, **kw)
            assert float(loss) == float(ref[0]) and torch.equal(grad, ref[1])
    img = E.flow_field_iwe(flow, *cols)
    for args in (tens, (ev, None, None, None), padded):
        assert torch.equal(E.flow_field_iwe(flow, *args), img)


def test_contended_cells_are_repeatable():
    """20 000 events on the (24, 32) canvas, about 24 to a cell: integer atomics give the same bits twice."""
    import event_utils_amd as E
    flow, cols = _scene(n=20000, seed=42)
    dflow, dcols = torch.from_numpy(flow).cuda(), tuple(torch.from_numpy(a).cuda() for a in cols)
    first = E.flow_field_contrast_loss(dflow, *dcols, direction="both", compute_gradient=True)
    again = E.flow_field_contrast_loss(dflow, *dcols, direction="both", compute_gradient=True)
    assert float(first[0]) == float(again[0]) and torch.equal(first[1], again[1])
    ref_loss, ref_grad = _oracle(flow, cols, 1.0, "variance", "both")
    _close_loss(first[0], ref_loss)
    _close_grad(first[1], ref_grad)


def test_the_second_trip_of_the_event_loops():
    """2048 x 256 + 3 events on an (8, 8) field: the grid of the event passes is capped at 2048 workgroups of 256 threads, so
    three events are taken on a second trip of the grid-stride loops of both losses' splat and gather / scatter kernels (and of
    the max |q| pass).  Both losses with their gradients against the restatements (the timestamp loss by the rules of
    tests/test_gpu_flow_loss.py, which are the same).  About 6 500 events to a cell of the (9, 9) canvas."""
    import event_utils_amd as E
    import _flow_loss_np as T
    n = 2048 * 256 + 3
    flow, cols = _scene(n=n, seed=51, shape=(8, 8))
    dflow, dcols = torch.from_numpy(flow).cuda(), tuple(torch.from_numpy(a).cuda() for a in cols)
    warped = _warped(flow, cols, "forward")
    kept = C.kept(flow, *cols, "forward", True, warped)
    assert 0 < kept[-3:].sum() and 0.5 * n < kept.sum() < n                 # the second trip counts, and some events leave
    loss, grad = E.flow_field_contrast_loss(dflow, *dcols, compute_gradient=True)
    ref_loss, ref_grad = _oracle(flow, cols, 1.0, "variance", "forward")
    print("contrast: loss %.9g (restatement %.9g), max |g - g_ref| / max |g_ref| = %.3g"
          % (float(loss), ref_loss, np.abs(_np(grad) - ref_grad).max() / np.abs(ref_grad).max()))
    _close_image(E.flow_field_iwe(dflow, *dcols), C.iwe(flow, *cols, f32_coords=True, warped=warped))
    _close_loss(loss, ref_loss)
    _close_grad(grad, ref_grad)
    loss, grad = E.flow_field_timestamp_loss(dflow, *dcols, compute_gradient=True)
    ref_loss, ref_grad = T.loss_and_grad(flow, *cols, 2.0, "forward", f32_coords=True, warped=warped)
    print("timestamp: loss %.9g (restatement %.9g), max |g - g_ref| / max |g_ref| = %.3g"
          % (float(loss), ref_loss, np.abs(_np(grad) - ref_grad).max() / np.abs(ref_grad).max()))
    _close_loss(loss, ref_loss)
    _close_grad(grad, ref_grad)
    # without the last three events the results differ: they were not dropped (the gradient's bound would hide a dropped trip
    # only if it changed nothing)
    less = E.flow_field_contrast_loss(dflow, *(a[:-3] for a in dcols), compute_gradient=True)
    assert float(less[0]) != float(E.flow_field_contrast_loss(dflow, *dcols))


# ---- the polarity factor ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("objective", C.OBJECTIVES)
def test_a_polarity_factor_of_100_scales_the_loss_by_1e4(objective):
    """DeviceEvents.scaled(100.0): L and dL/dflow are quadratic in the weights.  The fixed-point scales differ and I and 100 I
    round differently to float32, so the results agree to rounding, not bitwise: loss rtol 1e-6; gradient rtol 1e-6 with atol
    1e-6 max |g| for the components that nearly cancel (the form of tests/test_gpu_flow_loss.py for a changed scale)."""
    import event_utils_amd as E
    flow, cols = _scene()
    ev = E.DeviceEvents.from_arrays(*cols)
    kw = dict(objective=objective, compute_gradient=True)
    loss, grad = E.flow_field_contrast_loss(flow, ev, **kw)
    loss100, grad100 = E.flow_field_contrast_loss(flow, ev.scaled(100.0), **kw)
    print("loss %.12g, scaled %.12g" % (float(loss), float(loss100)))
    assert abs(float(loss100) - 1e4 * float(loss)) <= 1e-6 * abs(1e4 * float(loss))
    np.testing.assert_allclose(_np(grad100), 1e4 * _np(grad), rtol=1e-6, atol=1e-6 * 1e4 * float(grad.abs().max()))
    ref_loss, ref_grad = _oracle(flow, cols, 1.0, objective, "forward", p_scale=100.0)
    _close_loss(loss100, ref_loss)
    _close_grad(grad100, ref_grad)


def test_huge_weights_do_not_wrap():
    """p = +-3e6 on 3001 events: a cell may reach 9e9, beyond what 32 fractional bits leave of 63; the per-sample scale holds
    it.  The same through a polarity factor."""
    import event_utils_amd as E
    flow, cols = _scene()
    big = cols[:3] + (cols[3] * np.float32(3e6),)
    warped = _warped(flow, cols, "forward")
    ref = C.iwe(flow, *big, f32_coords=True, warped=warped)
    assert np.abs(ref).max() > 2.0 ** 23
    _close_image(E.flow_field_iwe(flow, *big), ref)
    for objective in C.OBJECTIVES:
        loss, grad = _check_against_oracle(flow, big, 1.0, objective, "forward")
        got = E.flow_field_contrast_loss(flow, E.DeviceEvents.from_arrays(*cols).scaled(3e6), objective=objective,
                                         compute_gradient=True)
        assert float(got[0]) == float(loss) and torch.equal(got[1], grad)


def test_nan_and_infinite_weights():
    """A NaN polarity adds nothing (and does not enter max |q|); an infinite one makes the sample's image NaN."""
    import event_utils_amd as E
    flow, cols = _scene()
    p = cols[3].copy()
    p[5:2000:7] = np.nan
    ok = ~np.isnan(p)
    with_nan, without = cols[:3] + (p,), tuple(a[ok] for a in cols[:3]) + (p[ok],)
    a, b = E.flow_field_iwe(flow, *with_nan), E.flow_field_iwe(flow, *without)
    # the scale follows the event count, which differs: equal to the fixed point's rounding, far inside the image tolerance
    _close_image(a, _np(b))
    _close_image(a, C.iwe(flow, *with_nan, f32_coords=True, warped=_warped(flow, with_nan, "forward")))
    p[3] = np.inf
    assert bool(torch.isnan(E.flow_field_iwe(flow, *cols[:3], p)).all())


# ---- masks -------------------------------------------------------------------------------------------------------------------------
def test_a_strong_field_sends_events_off_the_canvas_and_they_add_nothing():
    import event_utils_amd as E
    flow, cols = _scene(speed=900.0)
    cols = cols[:3] + (cols[3] * np.float32(1.5),)
    xw, yw = _warped(flow, cols, "forward")
    kept = (xw > 0) & (xw < SMALL[1]) & (yw > 0) & (yw < SMALL[0])
    assert 0.2 < 1.0 - kept.mean() < 0.8
    img = _np(E.flow_field_iwe(flow, *cols, use_polarity=False))
    assert abs(img.sum() - 1.5 * kept.sum()) <= 1e-6 * 1.5 * kept.sum()          # the weights of a counted event sum to 1
    loss, grad = _check_against_oracle(flow, cols, 1.0, "variance", "forward")
    # rejected events get no gradient: a field cell that only they touch stays exactly zero ...
    _, _, corners = C.sample(flow, cols[0], cols[1], f32_coords=True)
    touched = np.zeros(SMALL, dtype=bool)
    for yy, xx, wt, inside in corners:
        m = inside & kept & (wt != 0)
        touched[yy[m], xx[m]] = True
    assert touched.any() and not touched.all()
    assert not bool(grad[:, torch.from_numpy(~touched).cuda()].any())
    # ... and without them (the stream's ends are kept, they set the time constants) the results are the same up to the
    # fixed-point scale, which follows the event count
    kept[0] = kept[-1] = True
    few = tuple(a[kept] for a in cols)
    loss2, grad2 = E.flow_field_contrast_loss(flow, *few, compute_gradient=True)
    assert abs(float(loss2) - float(loss)) <= 1e-6 * abs(float(loss))
    np.testing.assert_allclose(_np(grad2), _np(grad), rtol=1e-6, atol=1e-6 * float(grad.abs().max()))


def test_zero_field_with_integer_coordinates_pins_the_one_sided_slope():
    """Every event sits on a pixel corner and stays there: the slopes are those of the cell the floor convention names."""
    flow, cols = _scene(integer=True)
    flow = np.zeros_like(flow)
    xw, yw = _warped(flow, cols, "forward")
    assert np.array_equal(xw, cols[0]) and np.array_equal(yw, cols[1])
    for objective in C.OBJECTIVES:
        for sigma in (0.0, 1.0):
            _check_against_oracle(flow, cols, sigma, objective, "forward")


# ---- batches and the edge cases --------------------------------------------------------------------------------------------------
def _batch():
    flows, cols, offsets = [], [], [0]
    for n, seed in ((1500, 21), (0, 22), (1501, 23)):
        flow, c = _scene(n=n, seed=seed)
        flows.append(flow)
        cols.append(c)
        offsets.append(offsets[-1] + n)
    return np.stack(flows), cols, tuple(np.concatenate([c[k] for c in cols]) for k in range(4)), np.array(offsets, dtype=np.int64)


@pytest.mark.parametrize("objective,direction", (("variance", "forward"), ("mean_square", "both")))
def test_batch_of_three_equals_three_single_calls(objective, direction):
    import event_utils_amd as E
    flows, cols, cat, offsets = _batch()
    kw = dict(objective=objective, direction=direction, compute_gradient=True)
    for off in (offsets, torch.from_numpy(offsets).cuda()):
        losses, grads = E.flow_field_contrast_loss(flows, *cat, offsets=off, **kw)
        assert losses.is_cuda and losses.dtype == torch.float64 and tuple(losses.shape) == (3,) and grads.shape == flows.shape
        for b in range(3):
            one, g = E.flow_field_contrast_loss(flows[b], *cols[b], **kw)
            assert float(losses[b]) == float(one) and torch.equal(grads[b], g)
        assert float(losses[1]) == 0.0 and not bool(grads[1].any()) and float(losses[0]) < 0 and float(losses[2]) < 0
    if direction == "forward":
        imgs = E.flow_field_iwe(flows, *cat, offsets=offsets)
        assert tuple(imgs.shape) == (3, SMALL[0] + 1, SMALL[1] + 1) and not bool(imgs[1].any())
        for b in (0, 2):
            assert torch.equal(imgs[b], E.flow_field_iwe(flows[b], *cols[b]))
        ref_losses, ref_grads = C.batch_loss_and_grad(flows, *cat, offsets, 1.0, objective, direction, f32_coords=True)
        for b in (0, 2):
            # the restatement's own float32 warp is warp_events_flow_torch's, bit for bit
            xw, yw = _warped(flows[b], cols[b], "forward")
            mine = C.warp(flows[b], *cols[b][:3], "forward", f32_coords=True)
            assert np.array_equal(xw, mine[0]) and np.array_equal(yw, mine[1])
            _close_loss(losses[b], ref_losses[b])
            _close_grad(grads[b], ref_grads[b])


def test_bad_arguments_raise():
    import event_utils_amd as E
    flows, _, cat, offsets = _batch()
    one = tuple(a[:1500] for a in cat)
    for fn in (E.flow_field_contrast_loss, E.flow_field_iwe, E.flow_contrast_loss):
        dev = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if fn is E.flow_contrast_loss else (lambda a: a)
        for bad in (flows[0][0], np.zeros((3,) + SMALL, dtype=np.float32), np.zeros((2, 1, 32), dtype=np.float32)):
            with pytest.raises(ValueError):
                fn(dev(bad), *one)
        with pytest.raises(ValueError):
            fn(dev(flows), *cat)                                             # a batch without offsets
        for bad in (offsets[:-1], offsets + 1, np.array([0, 2000, 1500, offsets[-1]]), offsets[::-1].copy(),
                    np.array([0, 1500, 1500, offsets[-1] - 1]), offsets.astype(np.float64), offsets.reshape(2, 2)):
            with pytest.raises(ValueError):
                fn(dev(flows), *cat, offsets=bad)
        with pytest.raises(ValueError):
            fn(dev(flows), *cat, offsets=torch.from_numpy(offsets + 1).cuda())
        with pytest.raises(ValueError):
            fn(dev(flows[0]), *one, direction="sideways")
        with pytest.raises(ValueError):
            fn(dev(flows[0]), one[0], one[1], one[2][:-1], one[3])           # columns of different lengths
    for fn in (E.flow_field_contrast_loss, E.flow_contrast_loss):
        with pytest.raises(ValueError):
            fn(torch.from_numpy(flows[0]).cuda(), *one, objective="contrast")
    with pytest.raises(ValueError):
        E.flow_field_iwe(flows[0], *one, direction="both")
    with pytest.raises(ValueError):
        E.flow_contrast_loss(flows[0], *one)                                 # the differentiable form takes a device tensor


# ---- autograd ----------------------------------------------------------------------------------------------------------------------
def test_autograd_scalar_loss_gives_the_explicit_gradient():
    import event_utils_amd as E
    flow, cols = _scene()
    for objective, direction in (("variance", "forward"), ("mean_square", "both")):
        kw = dict(objective=objective, direction=direction)
        loss, grad = E.flow_field_contrast_loss(flow, *cols, compute_gradient=True, **kw)
        leaf = torch.from_numpy(flow).cuda().requires_grad_(True)
        out = E.flow_contrast_loss(leaf, *cols, **kw)
        assert out.requires_grad and out.dtype == torch.float64 and out.item() == float(loss)
        out.sum().backward()
        assert leaf.grad.dtype == torch.float32 and torch.equal(leaf.grad, grad)


def test_autograd_runs_no_backward_pass_without_requires_grad(monkeypatch):
    import event_utils_amd as E
    from event_utils_amd.transforms import flow_loss
    flow, cols = _scene()
    calls = []
    real = flow_loss._lib.call
    monkeypatch.setattr(flow_loss._lib, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    out = E.flow_contrast_loss(torch.from_numpy(flow).cuda(), *cols)
    assert not out.requires_grad and float(out) == float(E.flow_field_contrast_loss(flow, *cols))
    assert "evk_flowcm_warp_f32" in calls and "evk_flowcm_grad_f32" not in calls
    del calls[:]
    leaf = torch.from_numpy(flow).cuda().requires_grad_(True)
    out = E.flow_contrast_loss(leaf, *cols, direction="both")
    del calls[:]
    out.backward()
    assert calls == ["evk_flowcm_grad_f32"] * 2                  # backward: the gather / scatter entry, once per direction


def test_autograd_scales_per_sample_and_reaches_what_made_the_field():
    import event_utils_amd as E
    flows, _, cat, offsets = _batch()
    _, grads = E.flow_field_contrast_loss(flows, *cat, offsets=offsets, compute_gradient=True)
    weights = torch.tensor([0.5, 2.0, -4.0], dtype=torch.float64, device="cuda")      # powers of two: the products are exact
    leaf = torch.from_numpy(flows).cuda().requires_grad_(True)
    (E.flow_contrast_loss(leaf, *cat, offsets=offsets) * weights).sum().backward()
    assert torch.equal(leaf.grad, grads * weights.float().reshape(3, 1, 1, 1))
    # through an operation that produced the field: d/dscale of loss(scale * flow) = sum(flow * dloss/dflow)
    scale = torch.tensor(1.0, device="cuda", requires_grad=True)
    base = torch.from_numpy(flows).cuda()
    E.flow_contrast_loss(scale * base, *cat, offsets=offsets).sum().backward()
    want = float((base.double() * grads.double()).sum())
    assert abs(float(scale.grad) - want) <= 1e-5 * float((base.double() * grads.double()).abs().sum())


# ---- against variance_objective ------------------------------------------------------------------------------------------------
def _linear_scene():
    x, y, t, p = _f32(Z.scene(Z.LINVEL, n=6000, seed=VO_SEED))
    a, b = (float(v) for v in -Z.LV_START)
    flow = np.empty((2, 180, 240), dtype=np.float32)
    flow[0], flow[1] = a, b
    return flow, (x, y, t, p), (a, b)


def _same_cells(flow, cols, a, b):
    """Do the float32 field warp and the float64 linear warp (cast to float32, as get_iwe casts it) put every event in the same
    cell, and keep the same events?"""
    x, y, t, _ = cols
    xf, yf = C.warp(flow, x, y, t, "forward", f32_coords=True)
    dt = t.astype(np.float64) - float(t[-1])
    xd, yd = (x.astype(np.float64) + a * dt).astype(np.float32), (y.astype(np.float64) + b * dt).astype(np.float32)
    keep = [(u > 0) & (u < 240) & (v > 0) & (v < 180) for u, v in ((xf, yf), (xd, yd))]
    return np.array_equal(keep[0], keep[1]) and all(np.array_equal(np.floor(u)[keep[0]], np.floor(v)[keep[0]])
                                                    for u, v in ((xf, xd), (yf, yd)))


def test_constant_field_is_the_variance_objective():
    """A constant field (a, b) against variance_objective (reference_exact=False, sensor_size set) on linvel_warp at (-a, -b),
    through the public GPU path, which warps in float64: the scene is one where both warps put every event in the same cell."""
    import event_utils_amd as E
    flow, cols, (a, b) = _linear_scene()
    assert cols[0].min() >= 0 and cols[0].max() <= 239 and cols[1].min() >= 0 and cols[1].max() <= 179
    assert _same_cells(flow, cols, a, b)
    obj = E.variance_objective()
    obj.reference_exact, obj.sensor_size = False, (180, 240)
    args = (np.array([-a, -b]), *cols, E.linvel_warp(), (180, 240))
    f, g = float(obj.evaluate_function(*args, blur_sigma=1.0)), np.asarray(obj.evaluate_gradient(*args, blur_sigma=1.0), dtype=np.float64)
    loss, grad = E.flow_field_contrast_loss(flow, *cols, objective="variance", blur_sigma=1.0, compute_gradient=True)
    total = _np(grad).sum(axis=(1, 2))
    print("loss %.9g against %.9g; summed gradient %s against %s" % (float(loss), f, total, -g))
    _close_loss(loss, f)
    assert np.abs(total + g).max() <= 1e-3 * np.abs(g).max()


# ---- descent -----------------------------------------------------------------------------------------------------------------------
def test_gradient_descent_lowers_the_loss_monotonically():
    """Twenty steps of plain gradient descent from the (24, 32) scene's field (variance, sigma 1, forward).  GD_STEP was chosen
    on the restatement (steps 2e4, 3e4, 5e4, 7e4, 1e5 and 1.5e5 all descend monotonically, with float64 and with float32
    coordinates alike; 5e4 lowers the loss by 5.7 % to 10.4 % per step, -0.19348 -> -0.86562, a margin that neither the
    float32 kernels nor a single event crossing the mask can turn)."""
    import event_utils_amd as E
    flow, cols = _scene()
    dcols = tuple(torch.from_numpy(a).cuda() for a in cols)
    field = torch.from_numpy(flow).cuda()
    losses = []
    for _ in range(20):
        loss, grad = E.flow_field_contrast_loss(field, *dcols, compute_gradient=True)
        losses.append(float(loss))
        field = field - GD_STEP * grad
    losses.append(float(E.flow_field_contrast_loss(field, *dcols)))
    print(" ".join("%.5g" % v for v in losses))
    assert all(b < a for a, b in zip(losses[:-1], losses[1:]))
    assert abs(losses[0] + 0.19348) < 1e-4 and losses[-1] < -0.8        # the restatement's start, and near its end (-0.86562)
