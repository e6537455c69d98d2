"""Float64 models of the NHWC BatchNorm and max-pool kernels (csrc/kernels/batchnorm.hip,
pool.hip), pass by pass, over [M, C] rows. Pure torch: inputs of any other float dtype are upcast
exactly on the CPU, and nothing here touches the GPU of its own accord (float64 tensors are taken
where they live, so a caller may hand over float64 rows it keeps elsewhere).
tests/test_norm_ref_cpu.py proves these models against torch's own float64 batch_norm /
max_pool2d and autograd."""
from __future__ import annotations

import torch


def rows64(t: torch.Tensor) -> torch.Tensor:
    """[M, C] float64 CPU rows of a 2D [M, C] or a 4D [N, C, H, W] tensor (any memory format)."""
    t = t.detach()
    if t.dtype != torch.float64:
        t = t.to("cpu", torch.float64)
    if t.dim() == 4:
        t = t.permute(0, 2, 3, 1)
    return t.reshape(-1, t.shape[-1]).contiguous()


def _vec64(t: torch.Tensor) -> torch.Tensor:
    t = t.detach()
    return t if t.dtype == torch.float64 else t.to("cpu", torch.float64)


# ----------------------------------------------------------------------------- batch norm
def bn_stats_ref(x, weight=None, bias=None, eps=1e-5):
    """Batch statistics of rows ``x`` [M, C]: (mean, biased var, invstd, scale, shift), where
    y = x * scale + shift is the normalisation with the affine folded in."""
    x = rows64(x)
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    invstd = 1.0 / torch.sqrt(var + eps)
    w = torch.ones_like(mean) if weight is None else _vec64(weight)
    b = torch.zeros_like(mean) if bias is None else _vec64(bias)
    scale = w * invstd
    return mean, var, invstd, scale, b - mean * scale


def bn_running_ref(mean, var, M, running_mean, running_var, momentum):
    """torch's momentum update with the unbiased variance; one row has no unbiased variance and
    the kernels then take the biased one (0): ``unbiased = var`` for M == 1."""
    unbiased = var * M / (M - 1) if M > 1 else var
    return ((1.0 - momentum) * _vec64(running_mean) + momentum * mean,
            (1.0 - momentum) * _vec64(running_var) + momentum * unbiased)


def bn_apply_ref(x, scale, shift, residual=None, relu=False):
    """(pre-activation, y) of y = ReLU?(x * scale + shift + residual?)."""
    pre = rows64(x) * scale + shift
    if residual is not None:
        pre = pre + rows64(residual)
    return pre, (pre.clamp_min(0.0) if relu else pre)


def bn_coef_ref(sum_g, sum_gx, mean, invstd, weight, count):
    """Per-channel (A, B, C) of dx = A g + B x + C from sum g and sum g (x - mean) over ``count`` rows."""
    w = torch.ones_like(mean) if weight is None else _vec64(weight)
    k = w * invstd
    s1 = sum_g / count
    s2 = invstd * invstd * sum_gx / count
    return k, -k * s2, k * s2 * mean - k * s1


def bn_backward_ref(g, x, mean, invstd, weight, M):
    """From the already-masked gradient ``g`` [M, C]: (dbias, dweight, A, B, C, dx)."""
    g, x = rows64(g), rows64(x)
    sum_g = g.sum(0)
    sum_gx = (g * (x - mean)).sum(0)
    A, B, Cc = bn_coef_ref(sum_g, sum_gx, mean, invstd, weight, M)
    return sum_g, sum_gx * invstd, A, B, Cc, A * g + B * x + Cc


def sync_record_ref(x):
    """One rank's record: (mean, M2 = sum (x - mean)^2, row count)."""
    x = rows64(x)
    mean = x.mean(0)
    return mean, ((x - mean) ** 2).sum(0), x.shape[0]


def sync_merge_ref(records):
    """Chan's pairwise merge of (mean, M2, count) records in order; records without rows are
    skipped. Returns (mean, M2, count) of the union."""
    n, mean, m2 = 0, None, None
    for mb, m2b, nb in records:
        if not nb > 0:
            continue
        if n == 0:
            n, mean, m2 = nb, mb.clone(), m2b.clone()
        else:
            d = mb - mean
            tot = n + nb
            mean = mean + d * nb / tot
            m2 = m2 + m2b + d * d * n * nb / tot
            n = tot
    return mean, m2, n


def sync_coef_ref(sum_g, sum_gx, mean, invstd, weight, count):
    """bn_coef_ref over the all-reduced sums and the global row count."""
    return bn_coef_ref(sum_g, sum_gx, mean, invstd, weight, count)


# ----------------------------------------------------------------------------- max pooling
def _taps(n_out, n_in, stride, pad, d):
    """Input coordinate of tap ``d`` for every output coordinate, and which of them are in range."""
    pos = torch.arange(n_out) * stride - pad + d
    return pos, (pos >= 0) & (pos < n_in)


def pool_out_size(n_in, k, s, p):
    return (n_in + 2 * p - k) // s + 1


def maxpool_ref(x, k, s, p):
    """Max pooling of ``x`` [N, C, H, W] with window k = (kh, kw), stride s, padding p (no dilation,
    floor mode): (y float64, arg uint8) where arg is the window offset dy * kw + dx of the maximum.
    torch's tie rule: the first maximal in-range tap in row-major window order; a NaN wins and
    stays; in a window whose in-range taps are all -inf the first in-range tap wins."""
    x = x.detach().to("cpu", torch.float64)
    N, C, H, W = x.shape
    (kh, kw), (sh, sw), (ph, pw) = k, s, p
    Ho, Wo = pool_out_size(H, kh, sh, ph), pool_out_size(W, kw, sw, pw)
    best = torch.full((N, C, Ho, Wo), float("-inf"), dtype=torch.float64)
    arg = torch.zeros((N, C, Ho, Wo), dtype=torch.int64)
    seen = torch.zeros((1, 1, Ho, Wo), dtype=torch.bool)
    for dy in range(kh):
        hs, hv = _taps(Ho, H, sh, ph, dy)
        for dx in range(kw):
            ws, wv = _taps(Wo, W, sw, pw, dx)
            inr = (hv[:, None] & wv[None, :])[None, None]
            v = x[:, :, hs.clamp(0, H - 1)[:, None], ws.clamp(0, W - 1)[None, :]]
            take = inr & ((v > best) | v.isnan() | ~seen) & ~best.isnan()
            best = torch.where(take, v, best)
            arg = torch.where(take, torch.full_like(arg, dy * kw + dx), arg)
            seen = seen | inr
    return best, arg.to(torch.uint8)


def maxpool_arg_to_flat(arg, in_hw, k, s, p):
    """The window argmax as torch's flat input index h * W + w (``return_indices``)."""
    H, W = in_hw
    (kh, kw), (sh, sw), (ph, pw) = k, s, p
    a = arg.to(torch.int64)
    Ho, Wo = a.shape[2:]
    h = (torch.arange(Ho) * sh - ph)[:, None] + a // kw
    w = (torch.arange(Wo) * sw - pw)[None, :] + a % kw
    return h * W + w


def maxpool_backward_ref(gy, arg, in_shape, k, s, p):
    """The gather the backward kernel does, in float64: every output's gradient goes to the input
    pixel its argmax names; pixels no window points at get exactly 0."""
    gy = gy.detach().to("cpu", torch.float64)
    N, C, H, W = in_shape
    (kh, kw), (sh, sw), (ph, pw) = k, s, p
    Ho, Wo = gy.shape[2:]
    gx = torch.zeros(N, C, H, W, dtype=torch.float64)
    a = arg.detach().cpu().to(torch.int64)
    for dy in range(kh):
        hs, hv = _taps(Ho, H, sh, ph, dy)
        for dx in range(kw):
            ws, wv = _taps(Wo, W, sw, pw, dx)
            if not (hv.any() and wv.any()):
                continue
            ho, wo = torch.nonzero(hv)[:, 0], torch.nonzero(wv)[:, 0]
            sel = (a[:, :, ho[:, None], wo[None, :]] == dy * kw + dx).to(torch.float64)
            # one tap maps distinct windows to distinct pixels: a plain indexed add
            gx[:, :, hs[ho][:, None], ws[wo][None, :]] += sel * gy[:, :, ho[:, None], wo[None, :]]
    return gx
