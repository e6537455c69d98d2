"""Raw NHWC max-pool bindings (csrc/kernels/pool.hip) against the float64 model of
tests/_norm_ref.py at the window, tie and special-value edges: the output and the one-byte argmax
must be exact, the backward gather exact in fp32 (the gradients are dyadic, so every fp32 sum is)
and within 1 bf16 ulp of the float64 sum in bf16."""
import pytest
import torch
import torch.nn.functional as F

from . import _norm_ref as R
from ._edge_ref import assert_within_bf16_ulp

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
# (kh, kw, sh, sw, ph, pw): non-square window and stride; the identity; stride > kernel (uncovered
# pixels); a window with two padding rings; the ResNet stem's
WINDOWS = [(3, 2, 2, 1, 1, 1), (1, 1, 1, 1, 0, 0), (2, 2, 3, 3, 0, 0), (5, 5, 1, 1, 2, 2), (3, 3, 2, 2, 1, 1)]


def _ksp(w):
    return [w[0], w[1]], [w[2], w[3]], [w[4], w[5]]


def _nhwc(t, dev, dtype):
    return t.to(dev, dtype).contiguous(memory_format=torch.channels_last)


def _dyadic(shape, gen):
    """Multiples of 1/16 in [-4, 4]: exact in bf16, and any sum of a window's worth is exact in fp32."""
    return torch.randint(-64, 65, shape, generator=gen).float() / 16.0


def _check(native, dev, dtype, x_cpu, w, gen):
    """Forward and backward of one pool against the model; returns the model's (y, arg, gx)."""
    k, s, p = _ksp(w)
    x = _nhwc(x_cpu, dev, dtype)
    y, arg = native.maxpool2d_fwd(x, k, s, p)
    assert y.dtype == dtype and arg.dtype == torch.uint8
    assert y.is_contiguous(memory_format=torch.channels_last) and arg.stride() == y.stride()
    y_ref, arg_ref = R.maxpool_ref(x, k, s, p)
    assert y.shape == y_ref.shape
    torch.testing.assert_close(y.double().cpu(), y_ref, rtol=0, atol=0, equal_nan=True)
    assert torch.equal(arg.cpu(), arg_ref), f"{int((arg.cpu() != arg_ref).sum())} argmax bytes differ"
    gy = _nhwc(_dyadic(tuple(y.shape), gen), dev, dtype)
    gx = native.maxpool2d_bwd(gy, arg, list(x.shape), k, s, p)
    assert gx.shape == x.shape and gx.is_contiguous(memory_format=torch.channels_last)
    gx_ref = R.maxpool_backward_ref(gy, arg_ref, tuple(x.shape), k, s, p)
    if dtype == torch.float32:
        torch.testing.assert_close(gx.double().cpu(), gx_ref, rtol=0, atol=0)
    else:
        assert_within_bf16_ulp(gx, gx_ref, "maxpool backward")
        assert (gx.double().cpu()[gx_ref == 0] == 0).all()
    return y_ref, arg_ref, gx_ref


@pytest.mark.parametrize("w", WINDOWS, ids=lambda w: "k%dx%d_s%dx%d_p%dx%d" % w)
@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_windows(native, dev, dtype, w):
    gen = torch.Generator().manual_seed(sum(w))
    x = torch.randn(2, 24, 7, 9, generator=gen)
    _, _, gx_ref = _check(native, dev, dtype, x, w, gen)
    if w[2] > w[0]:  # stride 3 over a 2x2 window: every third row and column is never looked at
        assert (gx_ref[:, :, 2::3, :] == 0).all() and (gx_ref[:, :, :, 2::3] == 0).all()
        assert (gx_ref != 0).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_window_larger_than_image(native, dev, dtype):
    gen = torch.Generator().manual_seed(5)
    y_ref, arg_ref, _ = _check(native, dev, dtype, torch.randn(2, 16, 2, 2, generator=gen), (3, 3, 2, 2, 1, 1), gen)
    assert y_ref.shape[2:] == (1, 1) and (arg_ref >= 4).all()


@pytest.mark.parametrize("w", WINDOWS, ids=lambda w: "k%dx%d_s%dx%d_p%dx%d" % w)
@pytest.mark.parametrize("kind,dtype", [("constant", torch.float32), ("constant", torch.bfloat16),
                                        ("post_relu", torch.float32), ("post_relu", torch.bfloat16),
                                        ("four_values", torch.bfloat16)])
def test_pool_ties_go_to_the_first_tap(native, dev, kind, dtype, w):
    gen = torch.Generator().manual_seed(7)
    if kind == "constant":
        x = torch.full((2, 16, 7, 9), 1.5)
    elif kind == "post_relu":
        x = torch.randn(2, 16, 7, 9, generator=gen).clamp_min(0)
        assert 0.4 < float((x == 0).float().mean()) < 0.6
    else:
        x = torch.tensor([-1.0, 0.0, 0.5, 2.0])[torch.randint(0, 4, (2, 16, 7, 9), generator=gen)]
    _check(native, dev, dtype, x, w, gen)


@pytest.mark.parametrize("w", [(3, 3, 2, 2, 1, 1), (3, 2, 2, 1, 1, 1), (2, 2, 2, 2, 0, 0)],
                         ids=lambda w: "k%dx%d_s%dx%d_p%dx%d" % w)
@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_nan_and_inf(native, dev, dtype, w):
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(2, 16, 6, 6, generator=gen)
    x[0, 0, 2, 3] = float("nan")   # propagates, and the argmax is the NaN's own tap
    x[1, 9, 5, 5] = float("nan")   # last pixel, last vector lane of bf16's second vector
    x[0, 1, 4, 1] = float("inf")
    x[1, 2, 0, 0] = float("-inf")  # one -inf among finite values never wins
    y_ref, _, _ = _check(native, dev, dtype, x, w, gen)
    assert y_ref[0, 0].isnan().any() and y_ref[1, 9].isnan().any() and (y_ref[0, 1] == float("inf")).any()
    assert not y_ref[:, 3:9].isnan().any()  # no leak into neighbouring channels


@pytest.mark.parametrize("w", [(3, 3, 2, 2, 1, 1), (2, 2, 2, 2, 0, 0), (3, 2, 2, 1, 1, 1), (5, 5, 1, 1, 2, 2)],
                         ids=lambda w: "k%dx%d_s%dx%d_p%dx%d" % w)
@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_all_minus_inf_window_points_at_its_first_in_range_tap(native, dev, dtype, w):
    """A window whose in-range taps are all -inf, with (p > 0) and without (p = 0) padding overlap:
    its gradient goes to the first in-range tap (torch's rule), never to a padded position."""
    gen = torch.Generator().manual_seed(11)
    x = torch.full((1, 8, 4, 4), float("-inf"))
    y_ref, arg_ref, gx_ref = _check(native, dev, dtype, x, w, gen)
    assert (y_ref == float("-inf")).all()
    if w == (3, 3, 2, 2, 1, 1):
        assert int(arg_ref[0, 0, 0, 0]) == 4 and int(arg_ref[0, 0, 1, 1]) == 0
    # and as one corner of an otherwise ordinary map
    x = torch.randn(2, 16, 6, 6, generator=gen)
    x[:, :, :2, :2] = float("-inf")
    x[1, :, 4:, 4:] = float("-inf")
    _check(native, dev, dtype, x, w, gen)


def test_pool_second_grid_stride_trip(native, dev):
    """fp32 [16, 64, 128, 128]: 4.2 M 16-B work items against the 2.1 M one trip of the capped grid
    covers, in the forward (k = 1: the identity, argmax 0) and in the backward of a 2x2 / s2 pool."""
    gen = torch.Generator(device=dev).manual_seed(13)
    x = torch.randn(16, 64, 128, 128, device=dev, generator=gen).contiguous(memory_format=torch.channels_last)
    assert x.numel() // 4 > 8192 * 256
    y, arg = native.maxpool2d_fwd(x, [1, 1], [1, 1], [0, 0])
    assert torch.equal(y, x) and not arg.any()
    y, arg = native.maxpool2d_fwd(x, [2, 2], [2, 2], [0, 0])
    xr = x.clone().requires_grad_()
    yr = F.max_pool2d(xr, 2, 2)
    assert torch.equal(y, yr)
    gy = torch.randn(yr.shape, device=dev, generator=gen).contiguous(memory_format=torch.channels_last)
    gx = native.maxpool2d_bwd(gy, arg, list(x.shape), [2, 2], [2, 2], [0, 0])
    yr.backward(gy)
    assert torch.equal(gx, xr.grad)  # disjoint windows, no ties: one addend per pixel


@pytest.mark.parametrize("w", [(3, 3, 2, 2, 1, 1), (3, 2, 2, 1, 1, 1)], ids=lambda w: "k%dx%d_s%dx%d_p%dx%d" % w)
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("dtype", DTYPES)
def test_pool_folded_affine_bit_identical_to_apply_then_pool(native, dev, dtype, relu, w):
    k, s, p = _ksp(w)
    gen = torch.Generator().manual_seed(17)
    C = 24
    x = _nhwc(torch.randn(2, C, 7, 9, generator=gen) * 2 + 0.5, dev, dtype)
    sign = torch.where(torch.rand(C, generator=gen) < 0.5, -1.0, 1.0)
    scale = (torch.empty(C).uniform_(0.5, 1.5, generator=gen) * sign).to(dev)
    shift = torch.empty(C).uniform_(-0.5, 0.5, generator=gen).to(dev)
    assert (scale < 0).any() and (scale > 0).any()
    y1, a1 = native.maxpool2d_fwd(x, k, s, p, scale, shift, relu)
    z = native.bn_apply(x, None, scale, shift, relu)
    y2, a2 = native.maxpool2d_fwd(z, k, s, p)
    assert torch.equal(y1, y2) and torch.equal(a1, a2)
    # the composed form against the model, from the kernel's own activation
    y_ref, arg_ref = R.maxpool_ref(z, k, s, p)
    torch.testing.assert_close(y1.double().cpu(), y_ref, rtol=0, atol=0)
    assert torch.equal(a1.cpu(), arg_ref)
    # and the activation itself: one fma (+ ReLU), rounded once to the tensor's type
    pre, act = R.bn_apply_ref(x, scale.double().cpu(), shift.double().cpu(), None, relu)
    zr = R.rows64(z)
    bound = 2.0 ** -23 * (R.rows64(x).abs() * scale.double().cpu().abs() + shift.double().cpu().abs())
    if dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * act.abs()
    assert ((zr - act).abs() <= bound).all()


def test_pool_binding_checks(native, dev):
    x = torch.randn(2, 8, 6, 6, device=dev).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="unsupported window"):
        native.maxpool2d_fwd(x, [2, 2], [1, 1], [2, 2])  # 2 p > k
    with pytest.raises(RuntimeError, match="unsupported window"):
        native.maxpool2d_fwd(x, [3, 2], [1, 1], [1, 2])
    y, arg = native.maxpool2d_fwd(x, [3, 3], [2, 2], [1, 1])
    with pytest.raises(RuntimeError, match="output size mismatch"):
        native.maxpool2d_bwd(torch.ones_like(y), arg, [2, 8, 8, 6], [3, 3], [2, 2], [1, 1])  # Ho would be 4
    with pytest.raises(RuntimeError, match="multiple of"):
        native.maxpool2d_fwd(x[:, :6].contiguous(memory_format=torch.channels_last), [3, 3], [2, 2], [1, 1])
    xb = torch.randn(2, 12, 6, 6, device=dev).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError, match="multiple of"):
        native.maxpool2d_fwd(xb, [3, 3], [2, 2], [1, 1])
