"""SyncBatchNorm's plain-torch protocol path on two gloo ranks (CPU tensors, NCHW): the record
gather and merge, the backward's all-reduce of the two sums, the running statistics, the empty-rank
error, and the module conversion. The native kernels are covered by tests/test_syncbn_gpu.py."""
import os

import pytest
import torch

from pytorch_distributed_training_tutorials_amd.ops import SyncBatchNorm  # noqa: F401  (the public export)
from pytorch_distributed_training_tutorials_amd.parallel.env import free_port
from pytorch_distributed_training_tutorials_amd.parallel.launcher import spawn

from . import _syncbn_workers as W


def _two_ranks(tmp_path, momentum, split):
    spawn(W.cpu_reference_path, args=(2, free_port(), str(tmp_path), momentum, split), nprocs=2)
    return [torch.load(os.path.join(tmp_path, f"r{r}.pt"), weights_only=True) for r in range(2)]


@pytest.mark.parametrize("momentum", [0.1, None])
def test_two_rank_uneven_split_matches_full_batch(tmp_path, momentum):
    """Rank 0 holds 3 images and rank 1 holds 5 of one (8, 64, 7, 7) batch; momentum=None is the
    cumulative moving average (first batch: the batch statistics themselves)."""
    W.assert_matches_full_batch(_two_ranks(tmp_path, momentum, W.SPLIT), momentum)


def test_empty_rank_raises_on_every_rank(tmp_path):
    res = _two_ranks(tmp_path, 0.1, (8, 0))
    for r in res:
        assert "at least one row" in r["error"] and "[1]" in r["error"]


def test_convert_sync_batchnorm_keeps_tensors_keys_and_flags():
    W.conversion_checks("cpu")


def test_world_one_cpu_is_the_parent_layer():
    """Outside a multi-rank job the layer is BatchNorm2d's own code path: bitwise equal."""
    from pytorch_distributed_training_tutorials_amd.ops.norm import BatchNorm2d

    torch.manual_seed(0)
    x = torch.randn(4, 6, 5, 5)
    a, b = SyncBatchNorm(6), BatchNorm2d(6)
    xa, xb = x.clone().requires_grad_(), x.clone().requires_grad_()
    ya, yb = a(xa, relu=True), b(xb, relu=True)
    ya.sum().backward(), yb.sum().backward()
    assert a.sync_forwards == 0 and list(a.state_dict()) == list(b.state_dict())
    assert torch.equal(ya, yb) and torch.equal(xa.grad, xb.grad) and torch.equal(a.running_var, b.running_var)
