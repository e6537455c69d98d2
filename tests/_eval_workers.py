"""Spawned ranks of the evaluation-meter test (tests/test_eval_metrics.py): two gloo ranks feed
different batches to their own meter and call ``compute(comm)``. Straight-line code: the first
error ends the rank (and, through the launcher, the test)."""
import os

import torch

TOPK = (1, 3)
C = 7
SIZES = ((5, 9), (4, 2, 6))  # batch sizes of rank 0, rank 1


def make_batches(rank: int):
    """The rank's batches: seeded randn logits, targets with one ignored row per batch."""
    g = torch.Generator().manual_seed(100 + rank)
    out = []
    for B in SIZES[rank]:
        z = torch.randn(B, C, generator=g)
        y = torch.randint(0, C, (B,), generator=g)
        y[0] = -100
        out.append((z, y))
    return out


def two_rank_compute(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    from pytorch_distributed_training_tutorials_amd.ops import ClassificationMeter
    from pytorch_distributed_training_tutorials_amd.parallel.comm import Communicator

    comm = Communicator(device=torch.device("cpu"))
    assert comm.world == world
    meter = ClassificationMeter(TOPK)
    for z, y in make_batches(rank):
        meter.update(z, y)
    local = meter.state_dict()
    res = meter.compute(comm)
    after = meter.state_dict()  # compute() leaves the rank's own state alone
    assert torch.equal(local["counters"], after["counters"]) and torch.equal(local["loss_sum"], after["loss_sum"])
    torch.save({"result": res, "local_rows": int(local["counters"][0])}, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()
