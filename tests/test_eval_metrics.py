"""The evaluation meter (ops/metrics.py) without a GPU: the torch implementation of the row rules
against tests/_eval_ref.py, top-k against ``torch.topk`` on tie-free rows, the tie rule, special
rows, the meter's host checks, ``compute`` keys, state round trip, ``Trainer.evaluate`` and the
cross-rank reduction on two gloo ranks. The native kernels are covered by
tests/test_eval_metrics_gpu.py."""
import json
import os

import pytest
import torch

from pytorch_distributed_training_tutorials_amd.ops import AveragedModel, ClassificationMeter, classification_rows
from pytorch_distributed_training_tutorials_amd.parallel.env import free_port
from pytorch_distributed_training_tutorials_amd.parallel.launcher import spawn

from . import _eval_ref as R
from . import _eval_workers as W

DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
NAN, INF = float("nan"), float("inf")


def _case(B, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, C, generator=g).to(dtype), torch.randint(0, C, (B,), generator=g)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("C", [1, 2, 65, 1000])
def test_fallback_matches_reference(dt, C):
    z, y = _case(33, C, DTYPES[dt], seed=C)
    loss, rank = classification_rows(z, y)
    R.assert_rows(loss, rank, z, y)
    assert torch.equal(rank.long(), R.rank_by_sort(z, y))  # the rules are the stable-sort position


@pytest.mark.parametrize("dt", list(DTYPES))
def test_rank_below_k_is_topk_on_tie_free_rows(dt):
    C = 1000
    z = R.distinct_rows(16, C, DTYPES[dt], seed=3)
    assert all(z[b].float().unique().numel() == C for b in range(z.size(0)))
    y = torch.randint(0, C, (16,), generator=torch.Generator().manual_seed(4))
    y[:6] = z.float().topk(6, dim=1).indices[torch.arange(6), torch.arange(6)]  # targets at ranks 0..5
    _, rank = classification_rows(z, y)
    assert rank[:6].tolist() == list(range(6))
    for k in (1, 3, 5):
        want = z.float().topk(k, dim=1).indices.eq(y[:, None]).any(1)
        assert torch.equal(rank < k, want), k


def test_tie_rule():
    """Equal logits rank by class index: the target's position in a stable descending sort."""
    z = torch.tensor([[1.0, 2.0, 2.0, 2.0, 0.0]]).repeat(5, 1)
    y = torch.arange(5)
    _, rank = classification_rows(z, y)
    assert rank.tolist() == [3, 0, 1, 2, 4] == R.rank_by_sort(z, y).tolist()


def test_special_rows():
    z = torch.tensor([[0.5, NAN, 2.0, 1.0],    # the target's logit is NaN
                      [0.5, NAN, 2.0, 1.0],    # a NaN elsewhere: not greater
                      [0.5, 1.0, 2.0, 1.0],    # ignored
                      [0.5, 1.0, 2.0, 1.0],    # target == C
                      [0.5, 1.0, 2.0, 1.0],    # target == -1
                      [0.5, 1.0, 2.0, 1.0],    # target far outside
                      [0.5, -INF, 2.0, 1.0]])  # a masked class
    y = torch.tensor([1, 3, -100, 4, -1, 2 ** 40, 3])
    loss, rank = classification_rows(z, y)
    assert rank.tolist() == [4, 1, -1, -2, -2, -2, 1]
    assert torch.isnan(loss[0]) and torch.isnan(loss[1])
    assert loss[2:6].tolist() == [0.0] * 4
    R.assert_rows(loss, rank, z, y)
    assert torch.isfinite(loss[6])
    loss7, rank7 = classification_rows(z, y.clamp(-1, 4), ignore_index=-1)  # another ignore_index
    assert rank7.tolist() == [4, 1, -1, -2, -1, -2, 1] and loss7[4] == 0


def test_meter_counts_and_keys():
    z, y = _case(40, 10, torch.float32, seed=1)
    y[3], y[17] = -100, -100
    z[5, 2] = NAN  # a non-finite loss: counted, left out of the mean, its rank still counts
    m = ClassificationMeter(topk=(1, 5))
    m.update(z[:25], y[:25])
    m.update(z[25:], y[25:])
    counters, total = R.ref_state([(z, y)], (1, 5))
    assert m.counters.tolist() == counters and counters[:5] == [40, 38, 2, 0, 1]
    torch.testing.assert_close(m.loss_sum.item(), total, rtol=R.RTOL, atol=R.ATOL)
    out = m.compute()
    assert list(out) == ["loss", "top1", "top5", "count", "ignored", "nonfinite"]
    assert (out["count"], out["ignored"], out["nonfinite"]) == (38, 2, 1)
    assert out["top1"] == counters[5] / 38 and out["top5"] == counters[6] / 38
    torch.testing.assert_close(out["loss"], total / 37, rtol=R.RTOL, atol=R.ATOL)
    m.reset()
    assert m.counters.tolist() == [0] * 7 and m.loss_sum.item() == 0.0
    empty = m.compute()
    assert empty["count"] == 0 and empty["loss"] != empty["loss"] and empty["top1"] != empty["top1"]


def test_meter_host_checks():
    z, y = _case(4, 3, torch.float32, seed=2)
    with pytest.raises(ValueError, match="exceeds the 3 classes"):
        ClassificationMeter(topk=(1, 5)).update(z, y)  # as torch.topk(5) of 3 classes would
    for bad in ((), (0, 1), (3, 2), (2, 2), tuple(range(1, 10))):
        with pytest.raises(ValueError):
            ClassificationMeter(topk=bad)
    m = ClassificationMeter(topk=(1, 3))
    with pytest.raises(ValueError, match="int64"):
        m.update(z, y.int())
    with pytest.raises(ValueError, match=r"\[B, C\]"):
        m.update(z[0], y)
    with pytest.raises(ValueError, match="int64"):
        m.update(z, y[:3])
    y[1], y[2] = 3, -7
    m.update(z, y)
    with pytest.raises(ValueError, match="2 of 4 targets"):
        m.compute()


def test_state_dict_round_trip():
    z, y = _case(12, 6, torch.float32, seed=5)
    a = ClassificationMeter(topk=(1, 2, 4))
    a.update(z, y)
    state = a.state_dict()
    assert sorted(state) == ["counters", "loss_sum", "topk"] and state["topk"] == (1, 2, 4)
    a.update(z, y)  # the saved state is a copy
    b = ClassificationMeter(topk=(1, 2, 4))
    b.load_state_dict(state)
    b.update(z, y)
    assert torch.equal(a.counters, b.counters) and torch.equal(a.loss_sum, b.loss_sum)
    assert a.compute() == b.compute()
    with pytest.raises(ValueError, match="topk"):
        ClassificationMeter(topk=(1, 2)).load_state_dict(state)


def _toy_trainer(tmp_path, averaged=False):
    from torch.utils.data import DataLoader, TensorDataset

    from pytorch_distributed_training_tutorials_amd.models.toy import ToyMLP
    from pytorch_distributed_training_tutorials_amd.ops.optim import FusedSGD
    from pytorch_distributed_training_tutorials_amd.utils.trainer import Trainer

    g = torch.Generator().manual_seed(8)
    X, Y = torch.randn(48, 20, generator=g), torch.randint(0, 6, (48,), generator=g)
    Y[5] = -100
    torch.manual_seed(1)
    model = ToyMLP(20, 16, 6)
    loader = DataLoader(TensorDataset(X, Y), batch_size=16)
    kw = dict(averaged_model=lambda m: AveragedModel(m, decay=0.5)) if averaged else {}
    t = Trainer(model, loader, FusedSGD(model.parameters(), lr=0.05), verbose=False,
                metrics_path=str(tmp_path / "metrics.jsonl"), **kw)
    return t, X, Y, DataLoader(TensorDataset(X, Y), batch_size=20)  # the last evaluation batch is short


def test_trainer_evaluate(tmp_path):
    t, X, Y, loader = _toy_trainer(tmp_path, averaged=True)
    t.train(1)
    t.model.module[1].eval()  # a frozen layer inside a training model stays frozen
    flags = {n: m.training for n, m in t.model.named_modules()}
    assert t.model.training and not flags["module.1"]
    out = t.evaluate(loader, topk=(1, 3))
    assert {n: m.training for n, m in t.model.named_modules()} == flags  # restored, module by module
    with torch.no_grad():  # ReLU has no modes: the frozen flag changes nothing in the outputs
        logits = t.model.module(X.to(t.device)).float().cpu()
    counters, total = R.ref_state([(logits, Y)], (1, 3))
    assert (out["count"], out["ignored"], out["nonfinite"]) == (47, 1, 0)
    assert out["top1"] == counters[5] / 47 and out["top3"] == counters[6] / 47
    torch.testing.assert_close(out["loss"], total / 47, rtol=1e-4, atol=1e-4)
    avg = t.evaluate(loader, model=t.averaged_model, topk=(1, 3))  # the averaged copy scores differently
    assert avg["count"] == 47 and avg["loss"] != out["loss"]
    with open(tmp_path / "metrics.jsonl") as f:
        recs = [r for r in map(json.loads, f) if r["event"] == "eval"]
    assert len(recs) == 2 and recs[0]["batches"] == 3 and recs[0]["top1"] == out["top1"]
    assert recs[1]["model"] == "AveragedModel" and recs[1]["loss"] == avg["loss"]


def test_trainer_evaluate_restores_eval_mode(tmp_path):
    t, _, _, loader = _toy_trainer(tmp_path)
    t.model.eval()
    t.evaluate(loader, topk=(1,))
    assert not any(m.training for m in t.model.modules())


def test_two_ranks_equal_one_meter_over_the_union(tmp_path):
    spawn(W.two_rank_compute, args=(2, free_port(), str(tmp_path)), nprocs=2)
    res = [torch.load(os.path.join(tmp_path, f"r{r}.pt"), weights_only=True) for r in range(2)]
    union = ClassificationMeter(W.TOPK)
    for rank in range(2):
        for z, y in W.make_batches(rank):
            union.update(z, y)
    want = union.compute()
    assert [r["local_rows"] for r in res] == [sum(s) for s in W.SIZES]  # the ranks saw different batches
    assert res[0]["result"] == res[1]["result"]
    assert {k: v for k, v in res[0]["result"].items() if k != "loss"} == {k: v for k, v in want.items() if k != "loss"}
    # the loss sum is added in another order (per rank, then across ranks): a few float64 ulps
    torch.testing.assert_close(res[0]["result"]["loss"], want["loss"], rtol=1e-12, atol=0)
