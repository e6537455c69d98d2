"""Edge tests of the small kernels (loss.hip, rng.hip, elementwise.hip and the data movers
of optim.hip): bf16 instances, the second trip of every capped grid-stride loop, upstream
gradients other than 1, odd sizes and alignments, lists past the 32-tensor launch limit.

References are plain float64 computed on the CPU from the exact input values (bf16 inputs
upcast); inputs are drawn on the CPU so every machine tests the same numbers. Every index,
label and shape handed to a kernel is valid.

fp32 results are held to the project's rtol 1e-5 / atol 1e-6 (atol scaled down with the
reference where its largest value is below 1, so tiny gradients are still checked); where
a sum's order decides more than that, the kernel may be off by 4x the error torch's own
fp32 result on the same device shows against the same float64 reference (the measured
errors are kept in profiles/kernel_edges.md). bf16 gradients: within 1 bf16 ulp."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from ._edge_ref import (assert_by_measured_error, assert_within_bf16_ulp, ce_reference, f64, mse_reference,
                        philox_normal, philox_uniform)

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.bfloat16]
GRID_ELEMS = 2048 * 256 * 4  # elements one trip of a 2048-block, 4-per-thread grid covers


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(gen, shape, dev, dtype=torch.float32, scale=1.0):
    return (torch.randn(shape, generator=gen) * scale).to(dtype).to(dev)


def _assert_fp32(got, ref64, torch_f32, what):
    """rtol 1e-5 / atol 1e-6 against float64 (atol scaled by the reference's largest value when
    that is below 1); a case that needs more gets 4x torch's own fp32 error. ``torch_f32`` is a
    callable, only evaluated in the second case."""
    got64, ref64 = f64(got).reshape(-1), ref64.reshape(-1)
    assert got64.shape == ref64.shape
    assert torch.equal(torch.isnan(got64), torch.isnan(ref64)), what
    scale = min(1.0, float(ref64.abs().max())) if ref64.numel() else 1.0
    err = (got64 - ref64).abs()
    print(f"[fp32] {what}: max_abs_err={float(err.max()):.3e} max_abs_ref={float(ref64.abs().max()):.3e}")
    if bool((err <= 1e-6 * scale + 1e-5 * ref64.abs()).all()):
        return
    assert_by_measured_error(got, torch_f32(), ref64, what=what)


# ============================================================================= cross entropy
CE_SHAPES = [(1, 1), (1, 2), (3, 63), (5, 257), (2, 1025), (130, 8193)]  # the last: > 1024 * 256 * 4 elements


def _narrow(B, C, dtype):
    """Where 1 bf16 ulp of the float64 gradient is out of fp32 arithmetic's reach unless the inputs keep
    clear of cancellation: bf16 with a thousand elements or more. The kernel's p = exp(z - lse) carries
    about 1e-6 relative error, so an element whose gradient p * sum(t) - t (dense soft targets) or
    p - ls / C (label smoothing) cancels to less than 3e-4 of p is off by more than a bf16 ulp of that
    small difference, and among many elements drawn like the small cases some are. Measured with dense
    uniform targets and logits of spread 3: (2, 1025) on the GPU 1 of 2050 elements at 1.8 ulp; (130,
    8193) in an fp32 model of the kernel 8 of 1,065,090 elements, up to 20 ulp. There the logits are
    drawn narrow (every p above 2 * ls / C) and the soft targets two-hot (mixup); fp32 keeps the wide
    logits and dense targets at every shape, bf16 at the small ones."""
    return dtype == torch.bfloat16 and B * C >= 2 ** 10


def _ce_targets(gen, B, C, kind, dev, with_zero_labels, two_hot=False):
    if kind == "soft" and two_hot:
        # mixup rows: weights lam and 1 - lam on two classes, every row scaled so that sum(t) != 1
        t = torch.zeros(B, C)
        lam = torch.rand(B, generator=gen) * 0.8 + 0.1
        a = torch.randint(0, C // 2, (B,), generator=gen)
        t[torch.arange(B), a], t[torch.arange(B), a + C // 2] = lam, 1.0 - lam
        return (t * (torch.rand(B, 1, generator=gen) * 1.5 + 0.5)).to(dev)
    if kind == "soft":
        return torch.rand(B, C, generator=gen).to(dev)
    y = torch.randint(0, C, (B,), generator=gen)
    if with_zero_labels:
        y[::2] = 0  # rows 0, 2, ... carry the label that ignore_index=0 drops
        if B > 1:
            y[1] = C - 1  # and at least one row stays (B == 1: all ignored, covered below)
    return y.to(dev)


def _torch_ce(z, t, ign, ls, upstream):
    zr = z.detach().float().requires_grad_(True)
    l = F.cross_entropy(zr, t, ignore_index=ign, label_smoothing=ls)
    (l * upstream).backward()
    return l.detach(), zr.grad


@pytest.mark.parametrize("B,C", CE_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", ["soft", "index"])
def test_cross_entropy_edges(native, dev, B, C, dtype, kind):
    from pytorch_distributed_training_tutorials_amd.ops.loss import cross_entropy

    gen = _gen(1000 * B + C)
    narrow = _narrow(B, C, dtype)
    z0 = _randn(gen, (B, C), dev, dtype, scale=0.25 if narrow else 3.0)
    for ls in (0.0, 0.1):
        for ign in ((-100,) if kind == "soft" else (-100, 0)):
            t = _ce_targets(gen, B, C, kind, dev, with_zero_labels=(ign == 0), two_hot=narrow)
            if kind == "index" and ign == 0 and bool((t == 0).all()):
                continue  # every row ignored: test_cross_entropy_all_rows_ignored
            ref_l, ref_g = ce_reference(z0, t, ign, ls)
            for upstream in (1.0, -2.5):
                z = z0.clone().requires_grad_(True)
                l = cross_entropy(z, t, ignore_index=ign, label_smoothing=ls)
                (l * upstream).backward()
                what = f"ce {kind} B={B} C={C} {dtype} ls={ls} ign={ign} up={upstream}"
                assert l.dtype == torch.float32 and l.shape == () and z.grad.dtype == dtype
                # bf16 logits: the loss is an fp32 scalar, held to the fp32 rule
                _assert_fp32(l, ref_l, lambda: _torch_ce(z0, t, ign, ls, upstream)[0], what + " loss")
                if dtype == torch.float32:
                    _assert_fp32(z.grad, ref_g * upstream, lambda: _torch_ce(z0, t, ign, ls, upstream)[1],
                                 what + " grad")
                else:
                    assert_within_bf16_ulp(z.grad, ref_g * upstream, what + " grad")
                if kind == "index" and ign == 0:
                    assert not z.grad[t == 0].any()  # ignored rows get exactly 0


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ls", [0.0, 0.1])
def test_cross_entropy_single_class_soft_is_exactly_zero(native, dev, dtype, ls):
    """[B, 1] logits with float targets (the DDP toy's loss): loss and gradient are exactly 0, as torch gives."""
    from pytorch_distributed_training_tutorials_amd.ops.loss import cross_entropy

    gen = _gen(20)
    z = _randn(gen, (37, 1), dev, dtype, scale=5.0).requires_grad_(True)
    t = _randn(gen, (37, 1), dev, scale=5.0)
    l = cross_entropy(z, t, label_smoothing=ls)
    (l * -2.5).backward()
    assert l.item() == 0.0 and float(F.cross_entropy(z.detach().float(), t, label_smoothing=ls)) == 0.0
    assert not z.grad.any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_entropy_large_logits(native, dev, dtype):
    """Rows scaled to +-1e4: the row maximum is subtracted before exp, nothing overflows."""
    from pytorch_distributed_training_tutorials_amd.ops.loss import cross_entropy

    gen = _gen(21)
    z0 = _randn(gen, (6, 1025), dev, dtype, scale=1e4)
    z0[1] = z0[1].abs()       # all large positive
    z0[2] = -z0[2].abs()      # all large negative
    z0[3, :] = 1e4            # a constant row: uniform probabilities at a large offset
    t = torch.randint(0, 1025, (6,), generator=gen).to(dev)
    ref_l, ref_g = ce_reference(z0, t)
    z = z0.clone().requires_grad_(True)
    l = cross_entropy(z, t)
    l.backward()
    assert torch.isfinite(l) and torch.isfinite(z.grad).all()
    _assert_fp32(l, ref_l, lambda: _torch_ce(z0, t, -100, 0.0, 1.0)[0], f"ce 1e4 {dtype} loss")
    if dtype == torch.float32:
        _assert_fp32(z.grad, ref_g, lambda: _torch_ce(z0, t, -100, 0.0, 1.0)[1], f"ce 1e4 {dtype} grad")
    else:
        assert_within_bf16_ulp(z.grad, ref_g, "ce 1e4 bf16 grad")


@pytest.mark.parametrize("dtype", DTYPES)
def test_cross_entropy_masked_classes(native, dev, dtype):
    """-inf logits in non-target classes (a vocabulary mask): finite loss and gradient, the
    masked classes get gradient 0."""
    from pytorch_distributed_training_tutorials_amd.ops.loss import cross_entropy

    gen = _gen(22)
    B, C = 7, 300
    z0 = _randn(gen, (B, C), dev, dtype, scale=2.0)
    t = torch.randint(0, C, (B,), generator=gen).to(dev)
    mask = (torch.rand(B, C, generator=gen) < 0.4).to(dev)
    mask[3] = True  # one row keeps only its target class
    mask[torch.arange(B), t] = False
    z0 = z0.masked_fill(mask, float("-inf"))
    ref_l, ref_g = ce_reference(z0, t)
    for upstream in (1.0, -2.5):
        z = z0.clone().requires_grad_(True)
        l = cross_entropy(z, t)
        (l * upstream).backward()
        assert torch.isfinite(l) and torch.isfinite(z.grad).all()
        assert not z.grad[mask].any()
        _assert_fp32(l, ref_l, lambda: _torch_ce(z0, t, -100, 0.0, upstream)[0], f"ce masked {dtype} loss")
        if dtype == torch.float32:
            _assert_fp32(z.grad, ref_g * upstream, lambda: _torch_ce(z0, t, -100, 0.0, upstream)[1],
                         f"ce masked {dtype} grad")
        else:
            assert_within_bf16_ulp(z.grad, ref_g * upstream, "ce masked bf16 grad")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ls", [0.0, 0.1])
def test_cross_entropy_all_rows_ignored(native, dev, dtype, ls):
    """The mean over zero rows is NaN, as torch gives, and nothing flows back."""
    from pytorch_distributed_training_tutorials_amd.ops.loss import cross_entropy

    z = _randn(_gen(23), (5, 17), dev, dtype).requires_grad_(True)
    t = torch.zeros(5, dtype=torch.int64, device=dev)
    l = cross_entropy(z, t, ignore_index=0, label_smoothing=ls)
    (l * -2.5).backward()
    assert torch.isnan(l) and torch.isnan(F.cross_entropy(z.detach().float(), t, ignore_index=0))
    assert z.grad.shape == z.shape and not z.grad.any()


@pytest.mark.parametrize("B,C", [(3, 63), (5, 257)])
def test_cross_entropy_bf16_soft_targets(native, dev, B, C):
    """Soft targets handed over in bf16 are used at their bf16 values."""
    from pytorch_distributed_training_tutorials_amd.ops.loss import cross_entropy

    gen = _gen(24)
    z0 = _randn(gen, (B, C), dev)
    t = torch.rand(B, C, generator=gen).to(torch.bfloat16).to(dev)
    ref_l, ref_g = ce_reference(z0, t, label_smoothing=0.1)
    z = z0.clone().requires_grad_(True)
    l = cross_entropy(z, t, label_smoothing=0.1)
    (l * -2.5).backward()
    _assert_fp32(l, ref_l, lambda: _torch_ce(z0, t.float(), -100, 0.1, -2.5)[0], "ce bf16 soft loss")
    _assert_fp32(z.grad, ref_g * -2.5, lambda: _torch_ce(z0, t.float(), -100, 0.1, -2.5)[1], "ce bf16 soft grad")


@pytest.mark.parametrize("dtype", [torch.float16, torch.float64])
@pytest.mark.parametrize("kind", ["soft", "index"])
def test_cross_entropy_other_dtypes_fall_back(native, dev, dtype, kind):
    """fp16 / fp64 logits have no kernel: they go to F.cross_entropy instead of raising."""
    from pytorch_distributed_training_tutorials_amd.ops.loss import cross_entropy

    gen = _gen(25)
    z0 = _randn(gen, (9, 33), dev, dtype)
    t = torch.rand(9, 33, generator=gen).to(dtype).to(dev) if kind == "soft" \
        else torch.randint(0, 33, (9,), generator=gen).to(dev)
    z, zr = z0.clone().requires_grad_(True), z0.clone().requires_grad_(True)
    l, lr_ = cross_entropy(z, t, label_smoothing=0.1), F.cross_entropy(zr, t, label_smoothing=0.1)
    l.backward()
    lr_.backward()
    assert l.dtype == dtype
    torch.testing.assert_close(l, lr_)
    torch.testing.assert_close(z.grad, zr.grad)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ce_raw_bindings_without_upstream(native, dev, dtype):
    """ce_fwd / ce_bwd called directly, grad_out=None (an upstream gradient of 1 taken as given)."""
    gen = _gen(26)
    B, C = 5, 257
    z = _randn(gen, (B, C), dev, dtype)
    y = torch.randint(1, C, (B,), generator=gen).to(dev)
    y[2] = 0
    soft = torch.rand(B, C, generator=gen).to(dev)
    for s, i, ign in ((None, y, 0), (soft, None, -100)):
        loss, lse, valid = native.ce_fwd(z, s, i, ign, 0.1)
        d = native.ce_bwd(z, s, i, lse, valid, None, ign, 0.1)
        ref_l, ref_g = ce_reference(z, s if s is not None else i, ign, 0.1)
        assert loss.dtype == torch.float32 and lse.numel() == 3 * B and d.dtype == dtype
        assert float(valid) == (B - 1 if s is None else B)
        tf = lambda k: _torch_ce(z, s if s is not None else i, ign, 0.1, 1.0)[k]  # noqa: E731
        _assert_fp32(loss, ref_l, lambda: tf(0), "ce raw loss")
        _assert_fp32(lse[:B], torch.logsumexp(f64(z), 1), lambda: torch.logsumexp(z.float(), 1), "ce raw lse")
        if dtype == torch.float32:
            _assert_fp32(d, ref_g, lambda: tf(1), "ce raw grad")
        else:
            assert_within_bf16_ulp(d, ref_g, "ce raw grad")


# ============================================================================= MSE
MSE_SIZES = [1, 255, 4 * 256 * 1024 + 4099]  # the last is past the 1024-block grid cap


def _torch_mse(x, y, upstream):
    xr, yr = x.detach().float().requires_grad_(True), y.detach().float().requires_grad_(True)
    l = F.mse_loss(xr, yr)
    (l * upstream).backward()
    return l.detach(), xr.grad, yr.grad


@pytest.mark.parametrize("n", MSE_SIZES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_mse_edges(native, dev, n, dtype):
    from pytorch_distributed_training_tutorials_amd.ops.loss import mse_loss

    gen = _gen(30 + n % 97)
    x0, y0 = _randn(gen, (n,), dev, dtype), _randn(gen, (n,), dev, dtype)
    ref_l, ref_dx, ref_dy = mse_reference(x0, y0, upstream=-2.5)
    for need_x, need_y in ((True, True), (True, False), (False, True)):
        x, y = x0.clone().requires_grad_(need_x), y0.clone().requires_grad_(need_y)
        l = mse_loss(x, y)
        (l * -2.5).backward()
        what = f"mse n={n} {dtype} dx={need_x} dy={need_y}"
        assert l.dtype == torch.float32 and l.shape == ()
        _assert_fp32(l, ref_l, lambda: _torch_mse(x0, y0, -2.5)[0], what + " loss")
        assert (x.grad is not None) == need_x and (y.grad is not None) == need_y
        for k, (g, ref) in enumerate(((x.grad, ref_dx), (y.grad, ref_dy)), 1):
            if g is None:
                continue
            assert g.dtype == dtype and g.shape == x0.shape
            if dtype == torch.float32:
                _assert_fp32(g, ref, lambda: _torch_mse(x0, y0, -2.5)[k], what + f" grad{k}")
            else:
                assert_within_bf16_ulp(g, ref, what + f" grad{k}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_mse_raw_bindings_without_upstream(native, dev, dtype):
    gen = _gen(31)
    x, y = _randn(gen, (3, 85), dev, dtype), _randn(gen, (3, 85), dev, dtype)
    ref_l, ref_dx, ref_dy = mse_reference(x, y)
    _assert_fp32(native.mse_fwd(x, y), ref_l, lambda: _torch_mse(x, y, 1.0)[0], "mse raw loss")
    for need_x, need_y in ((True, True), (True, False), (False, True)):
        dx, dy = native.mse_bwd(x, y, None, need_x, need_y)
        for got, ref, need in ((dx, ref_dx, need_x), (dy, ref_dy, need_y)):
            assert (got is not None) == need
            if need and dtype == torch.float32:
                _assert_fp32(got, ref, lambda: _torch_mse(x, y, 1.0)[1], "mse raw grad")
            elif need:
                assert_within_bf16_ulp(got, ref, "mse raw grad")


# ============================================================================= Philox
def _fill(native, dev, n, seed, offset, dist, misalign=False):
    buf = torch.full((n + 1,), -7.0, device=dev)
    out = buf[1:] if misalign else buf[:n]
    native.philox_(out, seed, offset, dist)
    assert float(buf[0 if misalign else n]) == -7.0  # nothing written outside the view
    return out


def test_philox_known_answer(native, dev):
    """Random123's known answer for a zero counter and key."""
    words = [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    out = _fill(native, dev, 4, 0, 0, 0).cpu()
    assert out.tolist() == [(w >> 8) / 2 ** 24 for w in words]


def test_philox_model_constants_match_aten():
    """The model's multipliers and Weyl constants are the ones ATen's Philox engine uses."""
    import os
    import re

    from . import _edge_ref as m

    path = os.path.join(os.path.dirname(torch.__file__), "include", "ATen", "core", "PhiloxRNGEngine.h")
    consts = {int(c, 16) for c in re.findall(r"0x([0-9A-Fa-f]{8})\b", open(path).read())}
    assert {m.PHILOX_M0, m.PHILOX_M1, m.PHILOX_W0, m.PHILOX_W1} <= consts


@pytest.mark.parametrize("seed", [123, 2 ** 32 + 5, -1])
@pytest.mark.parametrize("offset", [0, 7, 2 ** 32 - 1])
def test_philox_uniform_bit_exact(native, dev, seed, offset):
    for n in (1, 3, 4, 1027):
        for misalign in (False, True):
            out = _fill(native, dev, n, seed, offset, 0, misalign).cpu().numpy()
            assert np.array_equal(out, philox_uniform(seed, offset, n)), (n, misalign)


def test_philox_second_grid_trip(native, dev):
    """n past 2048 * 256 * 4: the head and the tail against the model, the rest by the offset property."""
    n, k = GRID_ELEMS + 5, 1001
    out = _fill(native, dev, n, 123, 7, 0)
    assert np.array_equal(out[:4096].cpu().numpy(), philox_uniform(123, 7, 4096))
    assert np.array_equal(out[-4096:].cpu().numpy(), philox_uniform(123, 7, 4096, first=n - 4096))
    assert torch.equal(out[4 * k:], _fill(native, dev, n - 4 * k, 123, 7 + k, 0))


@pytest.mark.parametrize("dist", [0, 1])
@pytest.mark.parametrize("n,k", [(1027, 7), (5, 300)])
def test_philox_offset_property(native, dev, dist, n, k):
    """fill(n, offset=k) == fill(n + 4k, offset=0)[4k:]: what keeps the datasets' x and y streams disjoint."""
    assert torch.equal(_fill(native, dev, n, 99, k, dist), _fill(native, dev, n + 4 * k, 99, 0, dist)[4 * k:])
    assert torch.equal(_fill(native, dev, n, 99, k + 2 ** 32 - 1, dist, misalign=True),
                       _fill(native, dev, n + 4 * k, 99, 2 ** 32 - 1, dist)[4 * k:])


@pytest.mark.parametrize("seed,offset", [(123, 0), (2 ** 32 + 5, 7), (-1, 2 ** 32 - 1)])
def test_philox_normal_matches_box_muller(native, dev, seed, offset):
    """atol 2e-5, rtol 1e-5: the radius is at most 5.8, the float32 angle is reproduced exactly by the
    model, and sqrtf / logf / sincosf are a few float32 ulp off."""
    for n in (1, 3, 4, 1027):
        out = _fill(native, dev, n, seed, offset, 1, misalign=(n == 3))
        np.testing.assert_allclose(out.cpu().numpy().astype(np.float64), philox_normal(seed, offset, n),
                                   rtol=1e-5, atol=2e-5)


# ============================================================================= data movement
@pytest.mark.parametrize("dtype,trailing", [(torch.int64, ()), (torch.int64, (2,)), (torch.float32, (33,)),
                                            (torch.bfloat16, (3,)), (torch.uint8, (3,)), (torch.uint8, (8,)),
                                            (torch.float32, (3, 5)), (torch.bfloat16, (3, 5))])
def test_gather_rows_element_sizes(native, dev, dtype, trailing):
    """Every element size the loader gathers (int64 labels included), the byte path
    (row bytes not a multiple of 4), more rows than the 2048-block grid, repeated indices."""
    gen = _gen(40)
    N, rows = 300, 2500
    if dtype.is_floating_point:
        src = torch.randn((N, *trailing), generator=gen).to(dtype)
    else:
        hi = 2 ** 62 if dtype == torch.int64 else 256
        src = torch.randint(-hi if dtype == torch.int64 else 0, hi, (N, *trailing), generator=gen, dtype=dtype)
    src = src.to(dev)
    idx = torch.randint(0, N, (rows,), generator=gen, dtype=torch.int32)
    idx[:4] = torch.tensor([0, N - 1, N - 1, 0], dtype=torch.int32)
    idx = idx.to(dev)
    fill = 77 if not dtype.is_floating_point else -7.0
    out = torch.full((rows + 1, *trailing), fill, dtype=dtype, device=dev)
    native.gather_rows_(src, idx, out[:rows])
    assert torch.equal(out[:rows], src[idx.long()])
    assert bool((out[rows] == fill).all())  # nothing past the last row


@pytest.mark.parametrize("B,C", [(600, 1000), (600, 1), (1, 7)])
def test_one_hot_edges(native, dev, B, C):
    idx = torch.randint(0, C, (B,), generator=_gen(41)).to(dev)
    oh = native.one_hot(idx, C)
    assert oh.dtype == torch.float32 and torch.equal(oh, F.one_hot(idx, C).float())


def _seventy_shapes():
    sizes = [(3, 4), (0,), (9003,), (1,), (4096,), (4097,), (7, 5)]
    return [sizes[k % len(sizes)] for k in range(70)]


@pytest.mark.parametrize("dtype", DTYPES)
def test_bucket_copy_long_list(native, dev, dtype):
    """70 tensors (three launches), a zero-element and a 9003-element tensor among them; the
    scales 0.25 and 4.0 are exact in both types, so the comparison is exact."""
    gen = _gen(42)
    ts = [_randn(gen, s, dev, dtype) for s in _seventy_shapes()]
    total = sum(t.numel() for t in ts)
    flat = torch.full((total + 3,), -7.0, dtype=dtype, device=dev)
    native.bucket_copy(ts, flat, 0.25, False)
    assert torch.equal(flat[:total], torch.cat([t.reshape(-1) for t in ts]) * 0.25)
    assert bool((flat[total:] == -7.0).all())
    outs = [torch.full_like(t, -7.0) for t in ts]
    native.bucket_copy(outs, flat, 4.0, True)
    for o, t in zip(outs, ts):
        assert torch.equal(o, t)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, GRID_ELEMS + 5])
def test_scale_edges(native, dev, dtype, n):
    """Scales whose product with a bf16 / fp32 value rounds once: the result is exact."""
    x0 = _randn(_gen(43), (n,), dev, dtype)
    for s in (-0.5, 3.0):
        buf = torch.full((n + 1,), -7.0, dtype=dtype, device=dev)
        buf[:n] = x0
        native.scale_(buf[:n], s)
        assert torch.equal(buf[:n].cpu(), (f64(x0) * s).to(dtype))
        assert float(buf[n]) == -7.0


def test_cast_multi_long_list(native, dev):
    """40 bf16 -> f32 pairs (two launches), one pair channels_last, one empty."""
    gen = _gen(44)
    shapes = [[(5,), (4097,), (0,), (3, 7), (9003,)][k % 5] for k in range(40)]
    srcs = [_randn(gen, s, dev, torch.bfloat16) for s in shapes]
    srcs[7] = _randn(gen, (4, 6, 3, 3), dev, torch.bfloat16).to(memory_format=torch.channels_last)
    dsts = [torch.full_like(s, -7.0, dtype=torch.float32) for s in srcs]  # keeps each source's memory order
    assert not dsts[7].is_contiguous()
    native.cast_multi_(dsts, srcs)
    for d, s in zip(dsts, srcs):
        assert torch.equal(d, s.float())


# ============================================================================= reductions, elementwise
# (3000, 64) and (2049, 130): 3 row splits; (3001, 64): 3 splits of 1001 rows, the last one short (999)
COL_SUM_SHAPES = [(0, 5), (1, 1), (3, 65), (3000, 64), (3001, 64), (2049, 130)]


@pytest.mark.parametrize("rows,cols", COL_SUM_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("accumulate", [False, True])
def test_col_sum_edges(native, dev, rows, cols, dtype, accumulate):
    x = _randn(_gen(50 + rows), (rows, cols), dev, dtype)
    sentinel = 7.5
    buf = torch.full((cols + 1,), sentinel, device=dev)
    native.col_sum_(x, buf[:cols], accumulate)
    assert float(buf[cols]) == sentinel
    ref = f64(x).sum(0) + (sentinel if accumulate else 0.0)
    torch_f32 = x.float().sum(0) + (sentinel if accumulate else 0.0)
    terms = rows + (1 if accumulate else 0)
    biggest = max(float(x.float().abs().max()) if rows else 0.0, sentinel if accumulate else 0.0)
    assert_by_measured_error(buf[:cols], torch_f32, ref, floor=terms * 2.0 ** -24 * biggest,
                             what=f"col_sum ({rows}, {cols}) {dtype} accumulate={accumulate}")


@pytest.mark.parametrize("n", [1, 255, 1024, 1025, 4 * 256 * 37 + 513])
@pytest.mark.parametrize("dtype", DTYPES)
def test_sum_all_edges(native, dev, n, dtype):
    x = _randn(_gen(60 + n % 89), (n,), dev, dtype)
    out = native.sum_all(x)
    assert out.dtype == torch.float32 and out.shape == ()
    assert_by_measured_error(out, x.float().sum(), f64(x).sum(), floor=n * 2.0 ** -24 * float(x.float().abs().max()),
                             what=f"sum_all n={n} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_relu_bwd_edges(native, dev, dtype):
    """The mask is y > 0 exactly: +0 and -0 block, the smallest positive subnormal passes."""
    gen = _gen(70)
    n = GRID_ELEMS + 7
    tiny = torch.finfo(dtype).smallest_normal * torch.finfo(dtype).eps  # smallest positive subnormal
    y = torch.randn(n, generator=gen).to(dtype)
    dy = torch.randn(n, generator=gen).to(dtype)
    for base in (0, GRID_ELEMS - 2, n - 5):  # the first trip, the seam between the trips, the tail
        y[base:base + 5] = torch.tensor([0.0, -0.0, tiny, -tiny, 1.0], dtype=torch.float64).to(dtype)
    assert float(y[2]) > 0.0 and float(y[2]) == tiny
    want = torch.where(y > 0, dy, torch.zeros_like(dy))
    got = native.relu_bwd(dy.to(dev), y.to(dev))
    assert got.dtype == dtype and torch.equal(got.cpu(), want)


def test_relu_bwd_rejects_mismatches(native, dev):
    dy = torch.ones(64, device=dev)
    with pytest.raises(RuntimeError, match="relu_bwd"):
        native.relu_bwd(dy, torch.ones(64, device=dev, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="relu_bwd"):
        native.relu_bwd(dy, torch.ones(63, device=dev))
    with pytest.raises(RuntimeError, match="relu_bwd"):
        native.relu_bwd(dy.bfloat16(), torch.ones(128, device=dev, dtype=torch.bfloat16))
