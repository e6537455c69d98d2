"""The float64 models of tests/_norm_ref.py against torch's own float64 batch_norm / max_pool2d
and autograd, on the CPU: the references the GPU edge tests lean on are proven here."""
import pytest
import torch
import torch.nn.functional as F

from . import _norm_ref as R

TOL = dict(rtol=1e-11, atol=1e-11)


@pytest.mark.parametrize("M,C", [(1, 8), (2, 4), (37, 12), (300, 24)])
@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (True, True), (False, True)])
@pytest.mark.parametrize("affine", [True, False])
def test_bn_model_matches_torch_float64(M, C, relu, res, affine):
    torch.manual_seed(M * 31 + C)
    x = (torch.randn(M, C, dtype=torch.float64) * 2 + 3).requires_grad_()
    r = torch.randn(M, C, dtype=torch.float64).requires_grad_() if res else None
    sign = torch.where(torch.rand(C) < 0.5, -1.0, 1.0).double()
    w = (torch.empty(C, dtype=torch.float64).uniform_(0.5, 1.5) * sign).requires_grad_() if affine else None
    b = torch.empty(C, dtype=torch.float64).uniform_(-0.5, 0.5).requires_grad_() if affine else None
    rm, rv = torch.randn(C, dtype=torch.float64), torch.rand(C, dtype=torch.float64) + 0.5
    rm0, rv0 = rm.clone(), rv.clone()
    eps, mom = 1e-5, 0.1
    if M > 1:
        pre_t = F.batch_norm(x, rm, rv, w, b, True, mom, eps)
    else:  # torch refuses one value per channel in training; the kernels normalise it to the bias
        pre_t = (x - x.detach()) * (w if affine else 1.0) / eps ** 0.5 + (b if affine else 0.0)
    if res:
        pre_t = pre_t + r
    y_t = F.relu(pre_t) if relu else pre_t
    dy = torch.randn(M, C, dtype=torch.float64)
    y_t.backward(dy)

    mean, var, invstd, scale, shift = R.bn_stats_ref(x, w, b, eps)
    pre, y = R.bn_apply_ref(x, scale, shift, r, relu)
    torch.testing.assert_close(y, y_t.detach(), **TOL)
    if M > 1:
        nrm, nrv = R.bn_running_ref(mean, var, M, rm0, rv0, mom)
        torch.testing.assert_close(nrm, rm, **TOL)
        torch.testing.assert_close(nrv, rv, **TOL)
    else:
        nrm, nrv = R.bn_running_ref(mean, var, M, rm0, rv0, mom)
        torch.testing.assert_close(nrv, (1 - mom) * rv0, **TOL)  # unbiased = var = 0
        torch.testing.assert_close(invstd, torch.full_like(invstd, eps ** -0.5), **TOL)
    g = dy * (pre > 0) if relu else dy
    dbias, dweight, A, B, Cc, dx = R.bn_backward_ref(g, x, mean, invstd, w, M)
    if M > 1:
        # at M == 1 the hand-made graph above treats the mean as a constant: dx is 0 by the model
        torch.testing.assert_close(dx, x.grad, rtol=1e-9, atol=1e-9)
    else:
        torch.testing.assert_close(dx, torch.zeros_like(dx), rtol=0, atol=1e-9)
    if res:
        torch.testing.assert_close(g, r.grad, **TOL)
    if affine:
        torch.testing.assert_close(dbias, b.grad, rtol=1e-9, atol=1e-9)
        if M > 1:
            torch.testing.assert_close(dweight, w.grad, rtol=1e-9, atol=1e-9)
    # the coefficient form is the direct one
    torch.testing.assert_close(A * R.rows64(g) + B * R.rows64(x) + Cc, dx, **TOL)


def test_bn_model_upcasts_bf16_exactly_and_reads_nhwc():
    x = torch.randn(3, 8, 5, 7).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    rows = R.rows64(x)
    assert rows.shape == (3 * 5 * 7, 8)
    assert torch.equal(rows, x.permute(0, 2, 3, 1).reshape(-1, 8).double())
    assert torch.equal(rows.to(torch.bfloat16).double(), rows)


@pytest.mark.parametrize("chunks", [(5, 0, 11, 1), (0, 7), (3,), (1, 1, 1)])
def test_sync_model_merges_to_the_whole_batch(chunks):
    torch.manual_seed(sum(chunks))
    C = 12
    x = torch.randn(sum(chunks), C, dtype=torch.float64) * 3 + 100.0
    recs, at = [], 0
    for n in chunks:
        if n:
            recs.append(R.sync_record_ref(x[at:at + n]))
        else:
            recs.append((torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64), 0))
        at += n
    mean, m2, n = R.sync_merge_ref(recs)
    assert n == sum(chunks)
    torch.testing.assert_close(mean, x.mean(0), **TOL)
    torch.testing.assert_close(m2 / n, x.var(0, unbiased=False) if n > 1 else torch.zeros(C).double(),
                               rtol=1e-10, atol=1e-10)
    # coefficients from summed per-chunk sums equal the whole-batch backward
    w = torch.randn(C, dtype=torch.float64)
    g = torch.randn_like(x)
    invstd = 1.0 / torch.sqrt(m2 / n + 1e-5)
    sg = sum(g[a:b].sum(0) for a, b in _bounds(chunks))
    sgx = sum((g[a:b] * (x[a:b] - mean)).sum(0) for a, b in _bounds(chunks))
    A, B, Cc = R.sync_coef_ref(sg, sgx, mean, invstd, w, n)
    ref = R.bn_backward_ref(g, x, mean, invstd, w, n)
    for got, want in zip((A, B, Cc), ref[2:5]):
        torch.testing.assert_close(got, want, rtol=1e-9, atol=1e-9)


def _bounds(chunks):
    at = 0
    for n in chunks:
        yield at, at + n
        at += n


# ----------------------------------------------------------------------------- max pooling
WINDOWS = [((3, 2), (2, 1), (1, 1)), ((1, 1), (1, 1), (0, 0)), ((2, 2), (3, 3), (0, 0)),
           ((5, 5), (1, 1), (2, 2)), ((3, 3), (2, 2), (1, 1))]


def _check_pool_against_torch(x, k, s, p):
    xt = x.clone().double().requires_grad_()
    yt, it = F.max_pool2d(xt, k, s, p, return_indices=True)
    y, arg = R.maxpool_ref(x, k, s, p)
    torch.testing.assert_close(y, yt.detach(), rtol=0, atol=0, equal_nan=True)
    assert torch.equal(R.maxpool_arg_to_flat(arg, x.shape[2:], k, s, p), it)
    gy = torch.randn_like(yt)
    yt.backward(gy)
    gx = R.maxpool_backward_ref(gy, arg, x.shape, k, s, p)
    torch.testing.assert_close(gx, xt.grad, rtol=1e-12, atol=1e-12)
    return y, arg, gx


@pytest.mark.parametrize("k,s,p", WINDOWS)
def test_pool_model_matches_torch_random(k, s, p):
    torch.manual_seed(0)
    _check_pool_against_torch(torch.randn(2, 3, 7, 9), k, s, p)


def test_pool_model_stride_over_kernel_leaves_exact_zeros():
    torch.manual_seed(1)
    x = torch.randn(1, 2, 7, 9)
    _, _, gx = _check_pool_against_torch(x, (2, 2), (3, 3), (0, 0))
    assert (gx[:, :, 2::3, :] == 0).all() and (gx[:, :, :, 2::3] == 0).all()


def test_pool_model_window_larger_than_image():
    torch.manual_seed(2)
    y, arg, _ = _check_pool_against_torch(torch.randn(2, 3, 2, 2), (3, 3), (2, 2), (1, 1))
    assert y.shape[2:] == (1, 1)
    assert (arg >= 4).all()  # row 0 and column 0 of the one window are padding


@pytest.mark.parametrize("k,s,p", WINDOWS)
@pytest.mark.parametrize("kind", ["constant", "post_relu", "four_values"])
def test_pool_model_ties_follow_torch(kind, k, s, p):
    torch.manual_seed(3)
    if kind == "constant":
        x = torch.full((1, 2, 7, 9), 1.5)
    elif kind == "post_relu":
        x = torch.randn(2, 3, 7, 9).clamp_min(0)
    else:
        x = torch.tensor([-1.0, 0.0, 0.5, 2.0])[torch.randint(0, 4, (2, 3, 7, 9))]
    _check_pool_against_torch(x, k, s, p)


@pytest.mark.parametrize("k,s,p", [((3, 3), (2, 2), (1, 1)), ((3, 2), (2, 1), (1, 1)), ((2, 2), (2, 2), (0, 0))])
def test_pool_model_specials_follow_torch(k, s, p):
    torch.manual_seed(4)
    x = torch.randn(1, 2, 6, 6)
    x[0, 0, 2, 3] = float("nan")  # one NaN: it wins every window it is in, with its own tap
    x[0, 1, 4, 1] = float("inf")
    y, arg, _ = _check_pool_against_torch(x, k, s, p)
    assert y[0, 0].isnan().any() and not y[0, 1].isnan().any()
    # all -inf, with and without padding overlap: the first in-range tap takes the gradient
    x = torch.full((1, 1, 4, 4), float("-inf"))
    y, arg, gx = _check_pool_against_torch(x, k, s, p)
    assert (y == float("-inf")).all()
    if p == (1, 1) and k == (3, 3):
        assert arg[0, 0, 0, 0] == 4 and arg[0, 0, 1, 1] == 0  # (1, 1) of the corner window: past the padding
        assert (gx[0, 0, :2, :2] != 0).all()


def test_pool_model_nan_stays_with_the_first_nan():
    """Two NaNs in one window: the model keeps the first (the kernel's rule: a NaN wins and stays)."""
    x = torch.zeros(1, 1, 2, 2)
    x[0, 0, 0, 1] = x[0, 0, 1, 0] = float("nan")
    y, arg = R.maxpool_ref(x, (2, 2), (2, 2), (0, 0))
    assert y.isnan().all() and int(arg[0, 0, 0, 0]) == 1
