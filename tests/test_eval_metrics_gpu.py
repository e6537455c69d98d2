"""The evaluation kernels on the GPU (csrc/kernels/eval_metrics.hip through ops/metrics.py): parity
with the float64 reference of tests/_eval_ref.py at the launch-geometry edges, ties, special rows,
target checks, row independence, fixed-order accumulation, graph capture, strided logits and the
host validation of the bindings.

Bounds (tests/_eval_ref.py): ranks and counters exact; row losses and loss sums rtol = atol = 1e-5
against float64. Shapes are the smallest that reach every path: both 16-byte group widths (4 fp32,
8 bf16) with and without a tail, one to 257 rows (more than one workgroup of four one-wave rows),
and rows on both sides of the one-wave / one-workgroup threshold."""
import pytest
import torch

from pytorch_distributed_training_tutorials_amd.ops import ClassificationMeter, classification_rows

from . import _eval_ref as R

pytestmark = pytest.mark.gpu
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
ROWS_PER_BLOCK, WAVE_ROW_MAX_C = 4, 2048  # the kernel file's geometry (checked below)
CS = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 1001, WAVE_ROW_MAX_C, WAVE_ROW_MAX_C + 1, WAVE_ROW_MAX_C + 8, 4097]
BS = [1, ROWS_PER_BLOCK - 1, ROWS_PER_BLOCK + 1, 257]
NAN, INF = float("nan"), float("inf")


def _case(B, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, generator=g).to(dtype), torch.randint(0, C, (B,), generator=g)


def test_geometry_constants(native):
    assert native.EVAL_ROWS_PER_BLOCK == ROWS_PER_BLOCK and native.EVAL_WAVE_ROW_MAX_C == WAVE_ROW_MAX_C
    assert native.EVAL_MAX_K == 8


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("C", CS)
def test_rows_match_reference(dev, dt, C):
    """One reference over 257 rows; every B takes its first rows (and so the same rows at another B)."""
    z, y = _case(max(BS), C, DTYPES[dt], seed=C)
    loss, rank = R.ref_rows(z, y)
    zd, yd = z.to(dev), y.to(dev)
    for B in BS:
        got_loss, got_rank = classification_rows(zd[:B], yd[:B])
        R.assert_rows_ref(got_loss, got_rank, loss[:B], rank[:B])


def test_ties_rank_as_the_stable_sort(dev):
    """bf16 randn at C = 1000 repeats the target's value in most rows."""
    z, y = _case(64, 1000, torch.bfloat16, seed=0)
    tied = (z == z.gather(1, y[:, None])).sum(1) > 1
    assert int(tied.sum()) >= 16
    loss, rank = classification_rows(z.to(dev), y.to(dev))
    R.assert_rows(loss, rank, z, y)
    assert torch.equal(rank.cpu().long(), R.rank_by_sort(z, y))


def test_rank_below_k_is_topk_on_tie_free_rows(dev):
    z = R.distinct_rows(16, 1000, torch.bfloat16, seed=3)
    y = torch.randint(0, 1000, (16,), generator=torch.Generator().manual_seed(4))
    _, rank = classification_rows(z.to(dev), y.to(dev))
    for k in (1, 3, 5):
        assert torch.equal(rank.cpu() < k, z.float().topk(k, dim=1).indices.eq(y[:, None]).any(1)), k


# ------------------------------------------------------------------ special rows
def _special(C, dtype):
    """Rows 0-2 finite with -inf entries; 3-7 non-finite in the reference; 8 plain."""
    z, y = _case(9, C, dtype, seed=21)
    y[:] = torch.tensor([C - 1, 6, 0, 3, 2, 1, C - 1, 4, 7]) % C
    z[0, : C // 2] = -INF             # masked classes, the first 16-byte groups wholly -inf
    z[1, 1::2] = -INF                 # every other class masked
    z[2, 1:] = -INF                   # only the target left: loss 0
    z[3, :] = -INF                    # all -inf: lse = -inf
    z[4, y[4]] = INF                  # +inf target
    z[5, y[5]] = NAN                  # NaN target: rank C
    z[6, : min(16, C - 1)] = NAN      # NaNs elsewhere, whole groups of them before any number
    z[7, C // 2] = NAN                # one NaN elsewhere
    return z, y


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("C", [40, 1000, 1001, 4097, 4104])
def test_special_rows(dev, dt, C):
    z, y = _special(C, DTYPES[dt])
    loss, rank = R.ref_rows(z, y)
    assert torch.isfinite(loss).tolist() == [True] * 3 + [False] * 5 + [True] and loss[2] == 0
    got_loss, got_rank = classification_rows(z.to(dev), y.to(dev))
    R.assert_rows_ref(got_loss, got_rank, loss, rank)
    assert int(got_rank[5]) == C
    m = ClassificationMeter(topk=(1, 5), device=dev)
    m.update(z.to(dev), y.to(dev))
    counters, total = R.ref_state([(z, y)], (1, 5))
    assert m.counters.tolist() == counters and counters[:5] == [9, 9, 0, 0, 5]
    torch.testing.assert_close(m.loss_sum.item(), total, rtol=R.RTOL, atol=R.ATOL)  # the non-finite rows left out
    out = m.compute()
    assert out["nonfinite"] == 5 and out["count"] == 9
    torch.testing.assert_close(out["loss"], total / 4, rtol=R.RTOL, atol=R.ATOL)


# ------------------------------------------------------------------ targets
@pytest.mark.parametrize("C", [1000, 4097])
def test_ignored_and_out_of_range_targets(dev, C):
    """The logits are the last rows of a larger allocation whose other rows hold huge values: a
    read outside a row would show as a wrong loss or rank."""
    B = 12
    z, y = _case(B, C, torch.float32, seed=31)
    y[1], y[4], y[7], y[9], y[11] = -100, C, -1, 2 ** 40, -100
    big = torch.full((64 + B, C), 1e30, device=dev)
    big[-B:] = z.to(dev)
    zd = big[-B:]
    assert zd.is_contiguous() and zd.storage_offset() == 64 * C
    loss, rank = classification_rows(zd, y.to(dev))
    R.assert_rows(loss, rank, z, y)
    assert rank.cpu()[[1, 4, 7, 9, 11]].tolist() == [-1, -2, -2, -2, -1]
    assert loss.cpu()[[1, 4, 7, 9, 11]].tolist() == [0.0] * 5
    m = ClassificationMeter(topk=(1, 5), device=dev)
    m.update(zd, y.to(dev))
    counters, _ = R.ref_state([(z, y)], (1, 5))
    assert m.counters.tolist() == counters and counters[:5] == [12, 7, 2, 3, 0]
    with pytest.raises(ValueError, match="3 of 12 targets"):
        m.compute()


# ------------------------------------------------------------------ row independence
@pytest.mark.parametrize("dt,C", [("bf16", 1000), ("f32", 1001), ("bf16", 2056), ("f32", 4097), ("f32", 4100)])
def test_a_row_depends_on_its_contents_and_C_alone(dev, dt, C):
    """The same row alone, in the middle of 11 rows, near the end of 257 rows, and one element into
    its storage (off the 16-byte path): bitwise the same loss and rank."""
    dtype = DTYPES[dt]
    z, y = _case(257, C, dtype, seed=41)
    zd, yd = z.to(dev), y.to(dev)
    row, tgt = zd[17:18].clone(), yd[17:18].clone()
    want_loss, want_rank = classification_rows(row, tgt)
    for B, pos in ((11, 6), (257, 250)):
        zz, yy = zd[:B].clone(), yd[:B].clone()
        zz[pos], yy[pos] = row[0], tgt[0]
        loss, rank = classification_rows(zz, yy)
        assert torch.equal(loss[pos:pos + 1], want_loss) and torch.equal(rank[pos:pos + 1], want_rank), (B, pos)
    off = torch.empty(3 * C + 1, dtype=dtype, device=dev)[1:].view(3, C)
    off.copy_(zd[:3])
    off[1] = row[0]
    assert off.data_ptr() % 16 != 0
    loss, rank = classification_rows(off, torch.stack([yd[0], tgt[0], yd[2]]))
    assert torch.equal(loss[1:2], want_loss) and torch.equal(rank[1:2], want_rank)


# ------------------------------------------------------------------ accumulation
def _three_batches(dtype):
    out = []
    for i, B in enumerate((5, 257, 64)):
        z, y = _case(B, 1000, dtype, seed=50 + i)
        y[0] = -100
        out.append((z, y))
    out[1][0][9, 3] = NAN
    return out


def _fed(dev, batches, topk=(1, 3, 5)):
    m = ClassificationMeter(topk=topk, device=dev)
    for z, y in batches:
        m.update(z.to(dev), y.to(dev))
    return m


@pytest.mark.parametrize("dt", list(DTYPES))
def test_three_updates_equal_one_reference_and_repeat_bitwise(dev, dt):
    batches = _three_batches(DTYPES[dt])
    a = _fed(dev, batches)
    counters, total = R.ref_state(batches, (1, 3, 5))
    assert a.counters.tolist() == counters and counters[:5] == [326, 323, 3, 0, 1]
    torch.testing.assert_close(a.loss_sum.item(), total, rtol=R.RTOL, atol=R.ATOL)
    b = _fed(dev, batches)
    assert torch.equal(a.counters, b.counters) and torch.equal(a.loss_sum, b.loss_sum)
    assert sorted(a._ws) == [5, 64, 257]  # one workspace pair per batch size


def test_update_allocates_nothing_after_the_first_call(dev):
    z, y = _case(64, 1000, torch.bfloat16, seed=60)
    zd, yd = z.to(dev), y.to(dev)
    m = ClassificationMeter(device=dev)
    m.update(zd, yd)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats(dev)["allocation.all.allocated"]
    m.update(zd, yd)
    m.reset()
    assert torch.cuda.memory_stats(dev)["allocation.all.allocated"] == before


# ------------------------------------------------------------------ capture
def test_captured_update_equals_eager(dev):
    z, y = _case(64, 1000, torch.bfloat16, seed=70)
    y[5] = -100
    zd, yd = z.to(dev), y.to(dev)
    eager = ClassificationMeter(device=dev)
    for _ in range(3):
        eager.update(zd, yd)
    m = ClassificationMeter(device=dev)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        m.update(zd, yd)  # the workspaces of this B exist before the capture
    torch.cuda.current_stream(dev).wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        m.update(zd, yd)
    m.reset()
    for _ in range(3):
        graph.replay()
    torch.cuda.synchronize(dev)
    assert torch.equal(m.counters, eager.counters) and torch.equal(m.loss_sum, eager.loss_sum)
    assert int(m.counters[0]) == 192 and int(m.counters[2]) == 3


# ------------------------------------------------------------------ layouts and host checks
@pytest.mark.parametrize("dt", list(DTYPES))
def test_column_slices_are_handled_and_other_strides_refused(native, dev, dt):
    """Rows with column stride 1 at any row stride (the classes of a padded head) give the bits of
    a contiguous copy; a column stride or overlapping rows are refused by the binding."""
    z, y = _case(9, 1000, DTYPES[dt], seed=80)
    wide = torch.full((9, 1024), 1e30, dtype=DTYPES[dt], device=dev)
    wide[:, :1000] = z.to(dev)
    view = wide[:, :1000]
    assert not view.is_contiguous()
    loss, rank = classification_rows(view, y.to(dev))
    want_loss, want_rank = classification_rows(view.contiguous(), y.to(dev))
    assert torch.equal(loss, want_loss) and torch.equal(rank, want_rank)
    R.assert_rows(loss, rank, z, y)
    odd = wide[:, 1:1001]  # rows off the 16-byte path
    loss, rank = classification_rows(odd, y.to(dev))
    R.assert_rows(loss, rank, odd.cpu(), y)
    m = ClassificationMeter(device=dev)
    m.update(view, y.to(dev))
    assert int(m.counters[1]) == 9
    with pytest.raises(RuntimeError, match="rows must be contiguous"):
        classification_rows(z.to(dev).t().contiguous().t(), y.to(dev))
    with pytest.raises(RuntimeError, match="rows overlap"):
        classification_rows(z.to(dev)[:1].expand(9, 1000), y.to(dev))


def test_binding_checks_before_launching(native, dev):
    z, y = _case(8, 10, torch.float32, seed=90)
    zd, yd = z.to(dev), y.to(dev)
    counters, acc = torch.zeros(7, dtype=torch.int64, device=dev), torch.zeros(1, dtype=torch.float64, device=dev)
    ws = torch.empty(8, device=dev), torch.empty(8, dtype=torch.int32, device=dev)
    native.eval_update_(zd, yd, -100, [1, 5], counters, acc, *ws)
    assert counters.tolist()[:2] == [8, 8]
    for topk, msg in (([1, 11], "outside"), ([0, 1], "outside"), ([5, 1], "increasing"), ([1, 1], "increasing"),
                      ([], "values of k"), (list(range(1, 10)), "values of k")):
        with pytest.raises(RuntimeError, match=msg):
            native.eval_update_(zd, yd, -100, topk, torch.zeros(5 + len(topk), dtype=torch.int64, device=dev), acc, *ws)
    bad = [
        (dict(logits=zd.half()), "float32 and bfloat16"),
        (dict(logits=zd[0]), r"\[B, C\]"),
        (dict(logits=zd.cpu()), "one GPU"),
        (dict(target=yd.int()), "int64"),
        (dict(target=yd[:7]), "int64"),
        (dict(counters=counters[:6]), "counters"),
        (dict(counters=counters.int()), "counters"),
        (dict(counters=counters.cpu()), "counters"),
        (dict(loss_sum=acc.float()), "loss_sum"),
        (dict(row_loss=ws[0][:7]), "row_loss workspace"),
        (dict(rank=ws[1].long()), "rank workspace"),
    ]
    for change, msg in bad:
        kw = dict(logits=zd, target=yd, ignore_index=-100, topk=[1, 5], counters=counters, loss_sum=acc,
                  row_loss=ws[0], rank=ws[1])
        kw.update(change)
        with pytest.raises(RuntimeError, match=msg):
            native.eval_update_(**kw)
    assert counters.tolist()[:2] == [8, 8]  # nothing was launched by the refused calls
    with pytest.raises(RuntimeError, match="at least one row"):
        native.eval_rows(zd[:0], yd[:0], -100)


def test_trainer_evaluate_on_the_persistent_engine(dev):
    """The engine's parameters are live views of its flat buffer: after a persistent launch the
    module scores as a reference over its own logits does, and better than before training."""
    from pytorch_distributed_training_tutorials_amd import data as D
    from pytorch_distributed_training_tutorials_amd.models.toy import ToyMLP
    from pytorch_distributed_training_tutorials_amd.ops.optim import FusedSGD
    from pytorch_distributed_training_tutorials_amd.parallel import env
    from pytorch_distributed_training_tutorials_amd.utils.trainer import Trainer

    env.init_process_group("nccl")
    try:
        ds = D.DeviceTensorDataset.synthetic_classification(256, 20, 4, device=dev, seed=2)
        torch.manual_seed(0)
        model = ToyMLP(20, 32, 4)
        loader = D.DeviceDataLoader(ds, batch_size=32, sampler=D.DistributedSampler(ds, 1, 0))
        t = Trainer(model, loader, FusedSGD(model.parameters(), lr=0.05), 0, verbose=False)
        assert t.engine_name == "persistent"
        held = D.DeviceDataLoader(ds, batch_size=48, sampler=D.DistributedSampler(ds, 1, 0, shuffle=False))
        before = t.evaluate(held, topk=(1, 2))
        t.train(5)
        after = t.evaluate(held, topk=(1, 2))
        assert t.model.training and before["count"] == after["count"] == 256
        assert after["loss"] < before["loss"]
        with torch.no_grad():
            logits = t.model.module(ds.tensors[0]).float().cpu()
        counters, total = R.ref_state([(logits, ds.tensors[1].cpu())], (1, 2))
        assert (after["top1"], after["top2"]) == (counters[5] / 256, counters[6] / 256)
        torch.testing.assert_close(after["loss"], total / 256, rtol=1e-4, atol=1e-4)  # other batch split, fp32 GEMMs
    finally:
        env.destroy_process_group()


def test_meter_on_the_gpu_checks_k_and_takes_other_dtypes(dev):
    z, y = _case(6, 4, torch.float32, seed=91)
    with pytest.raises(ValueError, match="exceeds the 4 classes"):
        ClassificationMeter(topk=(1, 5), device=dev).update(z.to(dev), y.to(dev))
    half = z.half()
    loss, rank = classification_rows(half.to(dev), y.to(dev))  # float16: the torch rules on the device
    R.assert_rows(loss, rank, half, y)
    follow = ClassificationMeter(topk=(1,))  # device=None: the state follows the first logits
    follow.update(z.to(dev), y.to(dev))
    assert follow.device == dev and follow.compute()["count"] == 6
