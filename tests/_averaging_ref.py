"""float64 reference of weight averaging (ops/averaging.py, csrc/kernels/averaging.hip), shared by
tests/test_averaging.py and tests/test_averaging_gpu.py.

The weight of update number n (n updates applied before it) is the float64 formula rounded once to
float32, which is what the device stores; the update is ``a + w (p - a)`` in float64 with that
float32 weight, and a copy when ``w == 1``.

Per-step bound, with M = max(|a|, |p|): the kernel computes ``fmaf(w, p - a, a)`` in float32 from
the same float32 w. The subtraction rounds once, an error of at most 2^-24 |p - a| <= 2^-24 * 2 M,
which the multiplication by w <= 1 does not enlarge; the fused multiply-add rounds once more, at
most 2^-24 of a result that lies between a and p, so 2^-24 M. Together at most 3 * 2^-24 M =
1.8e-7 M. The bound is 1e-6 M: two float32 roundings on operands of size M with a few times
headroom. It is derived, not tuned; tests/test_averaging.py checks that a float32 evaluation on the
GPU tests' inputs stays inside it and prints the share it uses.
"""
import numpy as np
import torch

BOUND = 1e-6   # |err| <= BOUND * max(|a|, |p|) per element and step
DECAY = 0.999  # the EMA decay of the tests: (1 - d)(p - a) is below a bf16 ulp of a


def ref_weight(n: int, decay=None, warmup: bool = False) -> float:
    """float32(float64 formula) as a Python float."""
    if n == 0:
        w = np.float64(1.0)
    elif decay is None:
        w = np.float64(1.0) / np.float64(n + 1)
    else:
        d = np.float64(decay)
        if warmup:
            d = min(d, np.float64(1 + n) / np.float64(10 + n))
        w = np.float64(1.0) - d
    return float(np.float32(w))


def ref_step(a: torch.Tensor, p: torch.Tensor, w: float) -> torch.Tensor:
    """One update in float64 from the average ``a`` and the source ``p`` (any dtype, upcast exactly)."""
    a64, p64 = a.detach().double().cpu(), p.detach().double().cpu()
    if w == 1.0:
        return p64.clone()
    return a64 + w * (p64 - a64)


def step_bound(a: torch.Tensor, p: torch.Tensor) -> torch.Tensor:
    return BOUND * torch.maximum(a.detach().double().cpu().abs(), p.detach().double().cpu().abs())


def bound_share(got: torch.Tensor, a: torch.Tensor, p: torch.Tensor, w: float) -> float:
    """max over elements of |got - ref_step| / bound (elements with a zero bound must match exactly)."""
    err = (got.detach().double().cpu() - ref_step(a, p, w)).abs()
    bound = step_bound(a, p)
    assert bool((err[bound == 0] == 0).all())
    nz = bound > 0
    return float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0


# The tensor set of the GPU tests: scalar, below a vector, around the 4096-element chunk, two chunks
# and a tail, a channels_last conv weight, an odd matrix and 30 small ones (45 tensors: they cross
# the 32-tensor launch boundary). The two-chunk tensor comes first so that, in the flat buffer of
# the averaged copy, it starts 16-byte aligned and takes the 16-byte path; what follows it starts
# at odd offsets and takes the element path; (4096,) is met both ways in the direct kernel tests.
SHAPES = [(2 * 4096 + 5,), (1,), (3,), (4095,), (4096,), (4097,), (64, 3, 7, 7), (17, 33)] + [(5,)] * 30
CHANNELS_LAST = 6  # index of the channels_last tensor in SHAPES


def make_tensors(seed: int, dtype=torch.float32, device="cpu", offset_view: bool = True):
    """One tensor per SHAPES entry plus, last, a (4100,) view that starts one element into its
    storage (4-byte aligned in fp32, 2-byte aligned in bf16)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i, shape in enumerate(SHAPES):
        t = torch.randn(shape, generator=g).to(dtype).to(device)
        if i == CHANNELS_LAST:
            t = t.contiguous(memory_format=torch.channels_last)
        out.append(t)
    if offset_view:
        base = torch.randn(4101, generator=g).to(dtype).to(device)
        out.append(base[1:])
    return out
