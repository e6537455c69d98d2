"""Reference of the evaluation metrics (ops/metrics.py, csrc/kernels/eval_metrics.hip), shared by
tests/test_eval_metrics.py and tests/test_eval_metrics_gpu.py. Everything here runs on the CPU.

Ranks follow the rules of ops/metrics.py directly: ``#(z_c > z_y) + #(z_c == z_y and c < y)``, ``C``
when ``z_y`` is NaN, ``-1`` for ``ignore_index`` and ``-2`` for any other target outside ``[0, C)``.
For NaN-free rows that is the position of ``y`` in ``torch.sort(descending=True, stable=True)``
(``rank_by_sort``). Row losses are ``F.cross_entropy(z.double(), y, reduction="none")`` on the
logits as stored (already rounded to their dtype), 0 for ignored and bad rows.

Tolerance of a row loss: ``rtol = atol = 1e-5`` against the float64 value, the bound
tests/test_kernels_gpu.py holds ``ce_fwd`` to. With randn-scale logits the loss is ``lse - z_y`` of
two numbers of size <= ~12, each good to a few float32 ulps (~1e-6), so cancellation stays inside
it. A sum of n row losses is held to the same rtol / atol.
"""
import torch
import torch.nn.functional as F

RTOL = ATOL = 1e-5
BASE = ("rows", "valid", "ignored", "bad_target", "nonfinite")


def ref_rows(logits: torch.Tensor, target: torch.Tensor, ignore_index: int = -100):
    """``(loss float64[B], rank int64[B])``."""
    z, y = logits.detach().cpu().double(), target.detach().cpu()
    B, C = z.shape
    loss, rank = torch.zeros(B, dtype=torch.float64), torch.zeros(B, dtype=torch.int64)
    ignored = y == ignore_index
    ok = ~ignored & (y >= 0) & (y < C)
    rank[ignored] = -1
    rank[~ignored & ~ok] = -2
    if bool(ok.any()):
        zo, yo = z[ok], y[ok]
        loss[ok] = F.cross_entropy(zo, yo, reduction="none")
        zy = zo.gather(1, yo[:, None])
        r = (zo > zy).sum(1) + ((zo == zy) & (torch.arange(C)[None] < yo[:, None])).sum(1)
        r[torch.isnan(zy[:, 0])] = C
        rank[ok] = r
    return loss, rank


def rank_by_sort(logits: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
    """Position of the target in a stable descending sort (NaN-free rows, targets in range)."""
    z, y = logits.detach().cpu().double(), target.detach().cpu()
    order = torch.sort(z, dim=1, descending=True, stable=True).indices
    return (order == y[:, None]).int().argmax(1)


def ref_state(batches, topk, ignore_index: int = -100):
    """``(counters list, loss sum float)`` of a meter fed ``batches`` = [(logits, target), ...]:
    rows, valid, ignored, bad_target, nonfinite, correct@k...; the finite losses of valid rows."""
    c = dict.fromkeys(BASE + tuple(topk), 0)
    total = 0.0
    for logits, target in batches:
        loss, rank = ref_rows(logits, target, ignore_index)
        valid = rank >= 0
        finite = valid & torch.isfinite(loss)
        c["rows"] += rank.numel()
        c["valid"] += int(valid.sum())
        c["ignored"] += int((rank == -1).sum())
        c["bad_target"] += int((rank == -2).sum())
        c["nonfinite"] += int((valid & ~finite).sum())
        for k in topk:
            c[k] += int((valid & (rank < k)).sum())
        total += float(loss[finite].sum())
    return list(c.values()), total


def assert_rows(got_loss, got_rank, logits, target, ignore_index: int = -100):
    assert_rows_ref(got_loss, got_rank, *ref_rows(logits, target, ignore_index))


def assert_rows_ref(got_loss, got_rank, loss, rank):
    """Ranks exactly the reference's ``(loss, rank)``; losses within RTOL / ATOL where the reference
    is finite and non-finite exactly where it is not."""
    got_loss, got_rank = got_loss.detach().cpu(), got_rank.detach().cpu()
    assert got_loss.dtype == torch.float32 and got_rank.dtype == torch.int32
    assert torch.equal(got_rank.long(), rank), (got_rank.long() - rank).nonzero().flatten()[:8]
    finite = torch.isfinite(loss)
    assert torch.equal(torch.isfinite(got_loss), finite)
    torch.testing.assert_close(got_loss.double()[finite], loss[finite], rtol=RTOL, atol=ATOL)


def distinct_rows(B: int, C: int, dtype, seed: int) -> torch.Tensor:
    """[B, C] logits whose rows hold C distinct representable values (no ties). float32: a
    permutation of an exact grid in [-4, 4). bfloat16: bit patterns sampled without replacement
    from both signs of [2^-8, 2^4) (3072 values)."""
    g = torch.Generator().manual_seed(seed)
    if dtype == torch.float32:
        grid = (torch.arange(C, dtype=torch.float32) - C // 2) / 1024.0
        return torch.stack([grid[torch.randperm(C, generator=g)] for _ in range(B)])
    assert dtype == torch.bfloat16 and C <= 3072
    mag = torch.arange(119 << 7, 131 << 7, dtype=torch.int32)  # exponents 119..130, every mantissa
    bits = torch.cat([mag, mag | 0x8000])
    rows = torch.stack([bits[torch.randperm(bits.numel(), generator=g)[:C]] for _ in range(B)])
    rows = torch.where(rows >= 0x8000, rows - 0x10000, rows).to(torch.int16)
    return rows.view(torch.bfloat16)
