"""GPU: the average-timestamp loss of a dense flow field (flow_field_timestamp_images / flow_field_timestamp_loss /
flow_timestamp_loss) against its float64 numpy restatement (tests/_flow_loss_np.py, pinned by tests/test_cpu_flow_loss.py),
against the composition warp_events_flow_torch -> get_timestamp_images, and against zhu_timestamp_objective.

Every comparison with the restatement hands it the warped coordinates warp_events_flow_torch returns for the same inputs
(warped=): the per-pixel slope is discontinuous at pixel edges, so both sides must put every event in the same cell; then no
case and no pixel needs excluding.  Tolerances are those of tests/test_gpu_zhu.py: planes and images atol = 1e-6 x the plane's
maximum, loss rtol = 1e-4, gradient rtol = 1e-4 with atol = 1e-4 max|g_ref|."""
import numpy as np
import pytest
import torch

import _flow_loss_np as F
import _zhu_np as Z

pytestmark = pytest.mark.gpu

SMALL = (24, 32)
N_SMALL = 3001          # not a multiple of the wave (64) or of the block (256)
GD_STEP = 300.0         # chosen on the restatement: 20 steps take the loss from 110.8 to 76.4, each by at least 1.3 %


def _f32(cols):
    return tuple(np.asarray(a, dtype=np.float32) for a in cols)


def _scene(n=N_SMALL, integer=False, seed=11, shape=SMALL, speed=60.0):
    flow, x, y, t, p = F.scene(shape[0], shape[1], n, integer=integer, seed=seed, speed=speed)
    return flow.astype(np.float32), _f32((x, y, t, p))


def _warped(flow, cols, direction):
    """What warp_events_flow_torch returns for these inputs, per direction of the loss (numpy float32)."""
    import event_utils_amd as E
    x, y, t, p = (torch.from_numpy(a) for a in cols)
    out = []
    for d in (F.DIRECTIONS if direction == "both" else (direction,)):
        t0 = float(cols[2][-1] if d == "forward" else cols[2][0])
        xw, yw = E.transforms.warp_events_flow_torch(x, y, t, p, torch.from_numpy(flow), t0=t0)
        out.append((xw.numpy(), yw.numpy()))
    return tuple(out) if direction == "both" else out[0]


def _oracle(flow, cols, sigma, direction, p_scale=1.0):
    if len(cols[0]) == 0:
        return F.loss_and_grad(flow, *cols, sigma, direction)
    return F.loss_and_grad(flow, *cols, sigma, direction, f32_coords=True, warped=_warped(flow, cols, direction), p_scale=p_scale)


def _np(a):
    return a.detach().cpu().numpy().astype(np.float64)


def _close_planes(got, ref):
    got = _np(got)
    assert got.shape == ref.shape
    for c in range(ref.shape[0]):
        np.testing.assert_allclose(got[c], ref[c], rtol=0, atol=1e-6 * max(np.abs(ref[c]).max(), 1e-30), err_msg="plane %d" % c)


def _close_loss(got, ref):
    got = float(got)
    assert abs(got - ref) <= 1e-4 * abs(ref), (got, ref)


def _close_grad(g, ref):
    assert np.abs(ref).max() > 0
    np.testing.assert_allclose(_np(g), ref, rtol=1e-4, atol=1e-4 * np.abs(ref).max())


def _check_against_oracle(flow, cols, sigma, direction):
    import event_utils_amd as E
    loss, grad = E.flow_field_timestamp_loss(flow, *cols, blur_sigma=sigma, direction=direction, compute_gradient=True)
    assert loss.is_cuda and loss.dtype == torch.float64 and loss.dim() == 0
    assert grad.is_cuda and grad.dtype == torch.float32 and tuple(grad.shape) == flow.shape
    ref_loss, ref_grad = _oracle(flow, cols, sigma, direction)
    err = np.abs(_np(grad) - ref_grad).max() / np.abs(ref_grad).max()
    print("loss %.9g (restatement %.9g), max |g - g_ref| / max |g_ref| = %.3g" % (float(loss), ref_loss, err))
    _close_loss(loss, ref_loss)
    _close_grad(grad, ref_grad)
    assert float(E.flow_field_timestamp_loss(flow, *cols, blur_sigma=sigma, direction=direction)) == float(loss)
    return loss, grad


# ---- planes, loss and gradient against the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("direction", ("forward", "backward", "both"))
@pytest.mark.parametrize("integer", (False, True), ids=("float", "integer"))
@pytest.mark.parametrize("sigma", (0.0, 2.0))
def test_planes_loss_and_gradient_match_the_restatement(sigma, integer, direction):
    import event_utils_amd as E
    from event_utils_amd.transforms import flow_loss
    flow, cols = _scene(integer=integer)
    loss, grad = _check_against_oracle(flow, cols, sigma, direction)
    if direction == "both":
        parts = [E.flow_field_timestamp_loss(flow, *cols, blur_sigma=sigma, direction=d, compute_gradient=True) for d in F.DIRECTIONS]
        assert float(loss) == float(parts[0][0] + parts[1][0]) and torch.equal(grad, parts[0][1] + parts[1][1])
        return
    warped = _warped(flow, cols, direction)
    ref = F.planes(flow, *cols, direction=direction, f32_coords=True, warped=warped)
    assert 0 < ref[1].sum() + ref[3].sum() < len(cols[0])                      # some events leave the canvas, most stay
    s = flow_loss._Setup(flow, *cols, direction, None)
    _close_planes(s.planes(s.time_constants(s.directions[0]))[0], ref)
    img = E.flow_field_timestamp_images(flow, *cols, direction=direction)
    assert img.is_cuda and img.dtype == torch.float32 and tuple(img.shape) == (2, SMALL[0] + 1, SMALL[1] + 1)
    _close_planes(img, Z.averages(ref))


def test_tensor_device_events_and_misaligned_inputs_give_the_same_bits():
    import event_utils_amd as E
    flow, cols = _scene()
    ref = E.flow_field_timestamp_loss(flow, *cols, compute_gradient=True)
    tens = tuple(torch.from_numpy(a).cuda() for a in cols)
    ev = E.DeviceEvents.from_arrays(*cols)
    padded = tuple(torch.cat((c.new_zeros(1), c))[1:] for c in tens)            # columns that start off a 16-byte boundary
    assert all(c.data_ptr() % 16 == 4 for c in padded)
    for args in (tens, (ev, None, None, None), padded):
        loss, grad = E.flow_field_timestamp_loss(torch.from_numpy(flow).cuda(), *args, compute_gradient=True)
        assert float(loss) == float(ref[0]) and torch.equal(grad, ref[1])


def test_zero_field_with_integer_coordinates_pins_the_one_sided_slope():
    """Every event sits on a pixel corner and stays there: the slopes are those of the cell the floor convention names."""
    flow, cols = _scene(integer=True)
    flow = np.zeros_like(flow)
    xw, yw = _warped(flow, cols, "forward")
    assert np.array_equal(xw, cols[0]) and np.array_equal(yw, cols[1])
    for sigma in (0.0, 2.0):
        _check_against_oracle(flow, cols, sigma, "forward")


def test_a_strong_field_sends_events_off_the_canvas_and_they_add_nothing():
    import event_utils_amd as E
    from event_utils_amd.transforms import flow_loss
    flow, cols = _scene(speed=900.0)
    xw, yw = _warped(flow, cols, "forward")
    kept = (xw > 0) & (xw < SMALL[1]) & (yw > 0) & (yw < SMALL[0])
    assert 0.2 < kept.mean() < 0.8
    s = flow_loss._Setup(flow, *cols, "forward", None)
    planes = _np(s.planes(s.time_constants(s.directions[0]))[0])
    assert abs(planes[1].sum() + planes[3].sum() - kept.sum()) < 1e-6 * kept.sum()      # the weights of a counted event sum to 1
    loss, grad = _check_against_oracle(flow, cols, 2.0, "forward")
    # the masked events are not there at all: without them (the stream's ends are kept, they set the time constants) the planes
    # and the loss are the same bits; the gradient's fixed-point scale follows the event count, so it may round differently: 2^-22
    # of the largest term at worst (evk.h), far inside 1e-6
    kept[0] = kept[-1] = True
    few = tuple(a[kept] for a in cols)
    loss2, grad2 = E.flow_field_timestamp_loss(flow, *few, compute_gradient=True)
    assert float(loss2) == float(loss)
    np.testing.assert_allclose(_np(grad2), _np(grad), rtol=1e-6, atol=1e-6 * float(grad.abs().max()))


def test_images_equal_the_composition_of_the_two_public_calls():
    """The fused kernel against warp_events_flow_torch -> get_timestamp_images at zero velocity: the same float32 expressions
    and fixed-point sums, hence the same bits (and the issue's tolerance a fortiori)."""
    import event_utils_amd as E
    for integer in (False, True):
        flow, cols = _scene(integer=integer)
        xw, yw = _warped(flow, cols, "forward")
        ref = E.get_timestamp_images([0.0, 0.0], xw, yw, cols[2], cols[3], E.linvel_warp(), SMALL, sensor_size=SMALL)
        out = E.flow_field_timestamp_images(flow, *cols)
        _close_planes(out, _np(ref))
        assert torch.equal(out, ref)


def test_constant_field_is_the_linear_flow_objective():
    import event_utils_amd as E
    x, y, t, p = _f32(Z.scene(Z.LINVEL, n=6000))
    a, b = (float(v) for v in -Z.LV_START)
    flow = np.empty((2, 180, 240), dtype=np.float32)
    flow[0], flow[1] = a, b
    f, g = E.zhu_timestamp_objective().evaluate_function_and_gradient(np.array([-a, -b]), x, y, t, p, E.linvel_warp(), (180, 240))
    loss, grad = E.flow_field_timestamp_loss(flow, x, y, t, p, compute_gradient=True)
    total = _np(grad).sum(axis=(1, 2))
    print("loss %.9g against %.9g; summed gradient %s against %s" % (float(loss), f, total, -g))
    _close_loss(loss, float(f))
    np.testing.assert_allclose(total, -g, rtol=1e-4, atol=1e-4 * np.abs(g).max())


# ---- batches and the edge cases --------------------------------------------------------------------------------------------------
def _batch():
    flows, cols, offsets = [], [], [0]
    for n, seed in ((N_SMALL, 21), (0, 22), (517, 23)):
        flow, c = _scene(n=n, seed=seed)
        flows.append(flow)
        cols.append(c)
        offsets.append(offsets[-1] + n)
    return np.stack(flows), cols, tuple(np.concatenate([c[k] for c in cols]) for k in range(4)), np.array(offsets, dtype=np.int64)


@pytest.mark.parametrize("direction", ("forward", "both"))
def test_batch_of_three_equals_three_single_calls(direction):
    import event_utils_amd as E
    flows, cols, cat, offsets = _batch()
    for off in (offsets, torch.from_numpy(offsets).cuda()):
        losses, grads = E.flow_field_timestamp_loss(flows, *cat, direction=direction, offsets=off, compute_gradient=True)
        assert losses.is_cuda and losses.dtype == torch.float64 and tuple(losses.shape) == (3,) and grads.shape == flows.shape
        for b in range(3):
            one, g = E.flow_field_timestamp_loss(flows[b], *cols[b], direction=direction, compute_gradient=True)
            assert float(losses[b]) == float(one) and torch.equal(grads[b], g)
        assert float(losses[1]) == 0.0 and not bool(grads[1].any()) and float(losses[0]) > 0 and float(losses[2]) > 0
    if direction == "forward":
        imgs = E.flow_field_timestamp_images(flows, *cat, offsets=offsets)
        assert tuple(imgs.shape) == (3, 2, SMALL[0] + 1, SMALL[1] + 1) and not bool(imgs[1].any())
        for b in (0, 2):
            assert torch.equal(imgs[b], E.flow_field_timestamp_images(flows[b], *cols[b]))


@pytest.mark.parametrize("n", (0, 1))
def test_empty_and_single_event_samples(n):
    import event_utils_amd as E
    flow, cols = _scene(n=max(n, 1), seed=31)
    cols = tuple(a[:n] for a in cols)
    for direction in ("forward", "backward", "both"):
        loss, grad = E.flow_field_timestamp_loss(flow, *cols, direction=direction, compute_gradient=True)
        assert float(loss) == 0.0 and not bool(grad.any()) and tuple(grad.shape) == flow.shape
    img = E.flow_field_timestamp_images(flow, *cols)
    assert not bool(img.any())               # no event, or one event with tau = 0


def test_a_negative_polarity_factor_swaps_the_classes():
    import event_utils_amd as E
    flow, cols = _scene()
    ev = E.DeviceEvents.from_arrays(*cols)
    img = E.flow_field_timestamp_images(flow, ev)
    swapped = E.flow_field_timestamp_images(flow, ev.scaled(-1.0))
    assert bool(img[0].any()) and bool(img[1].any()) and not torch.equal(img[0], img[1])
    assert torch.equal(swapped[0], img[1]) and torch.equal(swapped[1], img[0])
    neg = E.flow_field_timestamp_loss(flow, cols[0], cols[1], cols[2], -cols[3], compute_gradient=True)
    got = E.flow_field_timestamp_loss(flow, ev.scaled(-1.0), compute_gradient=True)
    assert float(got[0]) == float(neg[0]) and torch.equal(got[1], neg[1])
    ref_loss, ref_grad = _oracle(flow, cols, 2.0, "forward", p_scale=-1.0)
    _close_loss(got[0], ref_loss)
    _close_grad(got[1], ref_grad)


# ---- contention and repeatability --------------------------------------------------------------------------------------------------
def _hot_pixel():
    rng = np.random.default_rng(41)
    n = 50000
    t = np.sort(rng.uniform(0.0, 0.05, n))
    cols = _f32((np.full(n, 10.5), np.full(n, 7.25), t, np.where(rng.random(n) < 0.5, 1.0, -1.0)))
    return np.zeros((2,) + SMALL, dtype=np.float32), cols


@pytest.mark.parametrize("case", ("contention", "hot_pixel"))
def test_loss_and_gradient_are_bitwise_repeatable(case):
    """200 000 events on 180 x 240, and 50 000 events on one pixel: right against the restatement, and the same bits twice.
    Measured: max |g - g_ref| = 1.6e-7 max |g_ref| under contention and 7.8e-5 on the hot pixel, where tau d gT + d gC cancels
    to four digits on the float32 adjoint images."""
    import event_utils_amd as E
    flow, cols = _scene(n=200000, seed=42, shape=(180, 240)) if case == "contention" else _hot_pixel()
    dflow, dcols = torch.from_numpy(flow).cuda(), tuple(torch.from_numpy(a).cuda() for a in cols)
    first = E.flow_field_timestamp_loss(dflow, *dcols, direction="both", compute_gradient=True)
    again = E.flow_field_timestamp_loss(dflow, *dcols, direction="both", compute_gradient=True)
    assert float(first[0]) == float(again[0]) and torch.equal(first[1], again[1])
    ref_loss, ref_grad = _oracle(flow, cols, 2.0, "both")
    print("max |g - g_ref| / max |g_ref| = %.3g" % (np.abs(_np(first[1]) - ref_grad).max() / np.abs(ref_grad).max()))
    _close_loss(first[0], ref_loss)
    _close_grad(first[1], ref_grad)


# ---- autograd ----------------------------------------------------------------------------------------------------------------------
def test_autograd_scalar_loss_gives_the_explicit_gradient():
    import event_utils_amd as E
    flow, cols = _scene()
    for direction in ("forward", "both"):
        loss, grad = E.flow_field_timestamp_loss(flow, *cols, direction=direction, compute_gradient=True)
        leaf = torch.from_numpy(flow).cuda().requires_grad_(True)
        out = E.flow_timestamp_loss(leaf, *cols, direction=direction)
        assert out.requires_grad and out.dtype == torch.float64 and out.item() == float(loss)
        out.backward()
        assert leaf.grad.dtype == torch.float32 and torch.equal(leaf.grad, grad)
    with torch.no_grad():
        assert float(E.flow_timestamp_loss(leaf, *cols)) == float(E.flow_field_timestamp_loss(flow, *cols))


def test_autograd_scales_per_sample_and_reaches_what_made_the_field():
    import event_utils_amd as E
    flows, _, cat, offsets = _batch()
    _, grads = E.flow_field_timestamp_loss(flows, *cat, offsets=offsets, compute_gradient=True)
    weights = torch.tensor([0.5, 2.0, -3.0], dtype=torch.float64, device="cuda")      # exact in float32: the products are too
    leaf = torch.from_numpy(flows).cuda().requires_grad_(True)
    (E.flow_timestamp_loss(leaf, *cat, offsets=offsets) * weights).sum().backward()
    assert torch.equal(leaf.grad, grads * weights.float().reshape(3, 1, 1, 1))
    # through an operation that produced the field: d/dscale of loss(scale * flow) = sum(flow * dloss/dflow)
    scale = torch.tensor(1.0, device="cuda", requires_grad=True)
    base = torch.from_numpy(flows).cuda()
    E.flow_timestamp_loss(scale * base, *cat, offsets=offsets).sum().backward()
    want = float((base.double() * grads.double()).sum())
    assert abs(float(scale.grad) - want) <= 1e-5 * float((base.double() * grads.double()).abs().sum())


def test_gradient_descent_lowers_the_loss_monotonically():
    """Twenty steps of plain gradient descent on a zero field over the linear-flow scene of tests/_zhu_np.py (20 000 events,
    180 x 240, sigma 2).  GD_STEP was chosen on the restatement (steps 100, 300, 1000 and 3000 all descend monotonically; 300
    lowers the loss by 1.3 % to 2.5 % per step, 110.8 -> 76.4, a margin the float32 kernels cannot turn)."""
    import event_utils_amd as E
    cols = tuple(torch.from_numpy(a).cuda() for a in _f32(Z.scene(Z.LINVEL, n=20000)))
    flow = torch.zeros((2, 180, 240), dtype=torch.float32, device="cuda")
    losses = []
    for _ in range(20):
        loss, grad = E.flow_field_timestamp_loss(flow, *cols, compute_gradient=True)
        losses.append(float(loss))
        flow = flow - GD_STEP * grad
    losses.append(float(E.flow_field_timestamp_loss(flow, *cols)))
    print(" ".join("%.5g" % v for v in losses))
    assert all(b < a for a, b in zip(losses[:-1], losses[1:]))
    assert losses[-1] < losses[0]
    assert abs(losses[0] - 110.8) < 0.1 and losses[-1] < 80.0          # the restatement's start, and near its end (76.4)


# ---- input checks ------------------------------------------------------------------------------------------------------------------
def test_bad_shapes_offsets_and_directions_raise():
    import event_utils_amd as E
    flows, _, cat, offsets = _batch()
    one = tuple(a[:N_SMALL] for a in cat)
    for fn in (E.flow_field_timestamp_loss, E.flow_field_timestamp_images, E.flow_timestamp_loss):
        dev = (lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()) if fn is E.flow_timestamp_loss else (lambda a: a)
        for bad in (flows[0][0], flows[0][:1], np.zeros((3,) + SMALL, dtype=np.float32), np.zeros((1, 3) + SMALL, dtype=np.float32),
                    np.zeros((2, 1, 32), dtype=np.float32)):
            with pytest.raises(ValueError):
                fn(dev(bad), *one)
        with pytest.raises(ValueError):
            fn(dev(flows), *cat)                                             # a batch without offsets
        with pytest.raises(ValueError):
            fn(dev(flows[0]), *one, offsets=[0, N_SMALL])                    # offsets without a batch
        for bad in (offsets[:-1], offsets + 1, np.array([0, 4000, 3001, offsets[-1]]), offsets[::-1].copy(),
                    np.array([0, N_SMALL, N_SMALL, offsets[-1] - 1]), offsets.astype(np.float64), offsets.reshape(2, 2)):
            with pytest.raises(ValueError):
                fn(dev(flows), *cat, offsets=bad)
        with pytest.raises(ValueError):
            fn(dev(flows), *cat, offsets=torch.from_numpy(offsets + 1).cuda())
        with pytest.raises(ValueError):
            fn(dev(flows[0]), *one, direction="sideways")
        with pytest.raises(ValueError):
            fn(dev(flows[0]), one[0], one[1], one[2][:-1], one[3])           # columns of different lengths
    with pytest.raises(ValueError):
        E.flow_timestamp_loss(flows[0], *one)                                # the differentiable form takes a device tensor
