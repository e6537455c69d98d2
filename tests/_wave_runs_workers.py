"""Worker of tests/test_wave_loop_runs_gpu.py: two ranks sharing cuda:0, the wave engine's lean and
generic all-reduce kernels on the same MSE run over epochs of 9 steps (runs of two and three unchecked
groups, one ending at the list's end), one after the other in each process."""
import os

import torch

S, B = 9, 32
LAUNCHES = (7, 2 * S + 4)


def lean_and_generic_two_ranks(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    import torch.distributed as dist

    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from pytorch_distributed_training_tutorials_amd.data.device_sampler import DeviceDistributedSampler
    from pytorch_distributed_training_tutorials_amd.ops.fused_step import FusedMLPStep
    from pytorch_distributed_training_tutorials_amd.parallel.comm import Communicator
    from pytorch_distributed_training_tutorials_amd.parallel.xgmi import XgmiAllReduce

    dev = torch.device("cuda", 0)
    ctl = Communicator(device=torch.device("cpu"))
    xg = XgmiAllReduce(ctl, dev, max_elems=4096)
    n = world * B * S
    X = torch.randn(n, 20, generator=torch.Generator().manual_seed(9)).to(dev)
    Y = torch.rand(n, 1, generator=torch.Generator().manual_seed(10)).to(dev)
    out = {}
    for mode in ("lean", "generic"):
        if mode == "generic":
            os.environ["PTDT_WAVE_GENERIC"] = "1"  # read when the plan is built
        else:
            os.environ.pop("PTDT_WAVE_GENERIC", None)
        torch.manual_seed(5)
        eng = FusedMLPStep(torch.nn.Linear(20, 1).to(dev), loss="mse", lr=0.05, xgmi=xg)
        sampler = DeviceDistributedSampler(n, world, rank, seed=3, device=dev)
        cursor = torch.zeros(2, dtype=torch.int32, device=dev)
        losses = torch.zeros(max(LAUNCHES), device=dev)
        plan = eng.persistent_plan(X, Y, B, sampler, cursor, losses, variant="wave_f")
        snaps = []
        for steps in LAUNCHES:
            plan.launch(steps)
            torch.cuda.synchronize()
            xg.check()
            snaps.append(torch.cat([eng.P, eng.G, losses[:steps]]).cpu())
        out[mode] = torch.cat(snaps)
        out[mode + "_variant"] = plan.kernel_variant
        out[mode + "_engine"] = plan.engine
        out[mode + "_cursor"] = cursor.cpu()
    os.environ.pop("PTDT_WAVE_GENERIC", None)
    torch.save(out, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()
