"""Plain high-precision models for the kernel edge tests: float64 references computed on
the CPU from the exact input values (bf16 inputs upcast), a numpy model of the Philox
stream, and bf16 ulp arithmetic. Nothing here touches the GPU."""
from __future__ import annotations

import math

import numpy as np
import torch


def f64(t: torch.Tensor) -> torch.Tensor:
    return t.detach().to("cpu", torch.float64)


# ----------------------------------------------------------------------------- bf16 ulps
def bf16_ordinal(t: torch.Tensor) -> torch.Tensor:
    """Position of every bf16 value on the ordered line of bf16 numbers (+0 and -0 both 0):
    neighbours differ by exactly 1, across binades and across zero."""
    assert t.dtype == torch.bfloat16
    bits = t.detach().cpu().contiguous().view(torch.int16).to(torch.int64) & 0xFFFF
    mag = bits & 0x7FFF
    return torch.where(bits >= 0x8000, -mag, mag)


def bf16_ulp_distance(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return (bf16_ordinal(a) - bf16_ordinal(b)).abs()


def bf16_ulp_of(x64: torch.Tensor) -> torch.Tensor:
    """Spacing of bf16 numbers at |x| (8 significant bits; the subnormal spacing below 2^-126)."""
    a = x64.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7)


def assert_within_bf16_ulp(got: torch.Tensor, ref64: torch.Tensor, what: str = ""):
    """``got`` (bf16) is within 1 bf16 ulp of the float64 value ``ref64``."""
    assert got.dtype == torch.bfloat16
    err = (f64(got) - ref64).abs()
    bad = err > bf16_ulp_of(ref64)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.numel()} elements off by more than 1 bf16 ulp, "
                           f"worst {float((err / bf16_ulp_of(ref64)).max()):.3f} ulp")


# ----------------------------------------------------------------------------- measured tolerances
def assert_by_measured_error(got, torch_f32, ref64, floor: float = 0.0, what: str = ""):
    """The rule for sums whose order differs from torch's at the same accumulation width:
    the kernel may be off by 4x the error torch's own fp32 result shows against the same
    float64 reference, plus ``floor``. Returns (torch error, kernel error), both max-abs."""
    ref64 = ref64.reshape(-1)
    e_torch = float((f64(torch_f32).reshape(-1) - ref64).abs().max()) if ref64.numel() else 0.0
    e_kernel = float((f64(got).reshape(-1) - ref64).abs().max()) if ref64.numel() else 0.0
    print(f"[measured] {what}: torch_fp32_err={e_torch:.3e} kernel_err={e_kernel:.3e} floor={floor:.3e}")
    assert e_kernel <= 4.0 * e_torch + floor, (what, e_kernel, e_torch, floor)
    return e_torch, e_kernel


# ----------------------------------------------------------------------------- cross entropy / MSE
def ce_reference(z, target, ignore_index=-100, label_smoothing=0.0, upstream=1.0):
    """Mean cross entropy of logits ``z`` [B, C] (any float dtype, upcast) and its gradient,
    in float64. ``target``: class indices [B] (rows equal to ``ignore_index`` drop out of the
    sum and of the mean's count) or soft targets [B, C]. Returns (loss, dloss/dz * upstream)."""
    z = f64(z)
    B, C = z.shape
    ls = float(label_smoothing)
    lse = torch.logsumexp(z, dim=1, keepdim=True)
    p = torch.exp(z - lse)
    if target.is_floating_point():
        t = f64(target)
        t = t * (1.0 - ls) + ls / C
        # 0 * -inf never arises here: soft targets are only used with finite logits
        rows = -(t * (z - lse)).sum(1)
        loss = rows.sum() / B
        grad = (p * t.sum(1, keepdim=True) - t) / B
    else:
        y = target.detach().cpu().long()
        valid = y != ignore_index
        n = int(valid.sum())
        ys = torch.where(valid, y, torch.zeros_like(y))
        onehot = torch.zeros(B, C, dtype=torch.float64).scatter_(1, ys[:, None], 1.0)
        rows = (lse - z.gather(1, ys[:, None])).squeeze(1)
        grad = p - onehot
        if ls > 0.0:
            rows = (1.0 - ls) * rows + ls * (lse.squeeze(1) - z.mean(1))
            grad = (1.0 - ls) * grad + ls * (p - 1.0 / C)
        rows = torch.where(valid, rows, torch.zeros_like(rows))
        grad = grad * valid[:, None].to(torch.float64)
        loss = rows.sum() / n if n > 0 else torch.tensor(math.nan, dtype=torch.float64)
        grad = grad / max(n, 1)
    return loss, grad * upstream


def mse_reference(x, y, upstream=1.0):
    """(loss, dloss/dx * upstream, dloss/dy * upstream) in float64."""
    d = f64(x) - f64(y)
    g = 2.0 * d / d.numel() * upstream
    return (d * d).mean(), g, -g


# ----------------------------------------------------------------------------- Philox4x32-10
PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """Random123 Philox4x32 with 10 rounds, vectorised: ``ctr`` is four uint64 arrays holding
    32-bit words, ``key`` two Python ints. Returns the four output word arrays."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) for c in ctr)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(PHILOX_M0) * c0  # 32 x 32 -> 64 bits: exact in uint64
        p1 = np.uint64(PHILOX_M1) * c2
        hi0, lo0 = p0 >> np.uint64(32), p0 & _MASK32
        hi1, lo1 = p1 >> np.uint64(32), p1 & _MASK32
        c0, c1, c2, c3 = hi1 ^ c1 ^ np.uint64(k0), lo1, hi0 ^ c3 ^ np.uint64(k1), lo0
        k0 = (k0 + PHILOX_W0) & 0xFFFFFFFF
        k1 = (k1 + PHILOX_W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def philox_words(seed: int, offset: int, first: int, count: int) -> np.ndarray:
    """Output words ``[first, first + count)`` of the stream ``philox_(out, seed, offset, .)``
    draws from: element 4q+j is word j of the block with counter (lo(offset+q), hi(offset+q), 0, 0)
    under the key (lo(seed), hi(seed)), seed and offset taken modulo 2^64."""
    seed &= (1 << 64) - 1
    q0, q1 = first // 4, (first + count + 3) // 4
    c = (np.arange(q0, q1, dtype=np.uint64) + np.uint64(offset & ((1 << 64) - 1)))  # wraps modulo 2^64
    zero = np.zeros_like(c)
    w = philox4x32_10((c & _MASK32, c >> np.uint64(32), zero, zero), (seed & 0xFFFFFFFF, seed >> 32))
    flat = np.stack(w, axis=1).reshape(-1)
    return flat[first - 4 * q0: first - 4 * q0 + count]


def philox_uniform(seed: int, offset: int, n: int, first: int = 0) -> np.ndarray:
    """dist=0: the top 24 bits of every word, scaled to [0, 1) -- exact in float32."""
    w = philox_words(seed, offset, first, n)
    return ((w >> np.uint64(8)).astype(np.float64) / 16777216.0).astype(np.float32)


def philox_normal(seed: int, offset: int, n: int) -> np.ndarray:
    """dist=1 in float64: Box-Muller on word pairs (0,1) and (2,3) of every block; the angle is
    the float32 product 6.2831855f * u as the kernel forms it, everything else in float64."""
    nq = (n + 3) // 4
    u = philox_uniform(seed, offset, 4 * nq).reshape(nq, 4)
    out = np.empty((nq, 4), dtype=np.float64)
    for a, b in ((0, 1), (2, 3)):
        r = np.sqrt(-2.0 * np.log(1.0 - u[:, a].astype(np.float64)))
        t = (np.float32(6.2831853071795864) * u[:, b]).astype(np.float64)
        out[:, a], out[:, b] = r * np.cos(t), r * np.sin(t)
    return out.reshape(-1)[:n]
