"""Worker of the two-rank validation test (gloo on the CPU, HIP launchers replaced by tests/emu_eval_ops): Trainer.validate under a process
group evaluates this rank's contiguous shard and all-reduces the table."""
import os
import sys

import torch
import torch.distributed as dist

CFG = dict(channels=6, spatial=2, activation=torch.nn.SiLU, embedding_dim=64, hidden_channels=[32, 64], hidden_blocks=[1, 1],
           attention_levels=[1], kernel_size=3, padding_mode="zeros")


def held_out(n=7, seed=21):
    return torch.randn(n, 6, 16, 16, generator=torch.Generator().manual_seed(seed)) * 0.5 + 0.5


def run(rank: int, world: int, port: int, out_dir: str):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    import emu_eval_ops
    import emu_ops
    from climate2weather_amd import ops as c2w_ops
    for name in emu_ops.ALL:
        if hasattr(c2w_ops, name):
            setattr(c2w_ops, name, getattr(emu_ops, name))
    for name in emu_eval_ops.NAMES:
        setattr(c2w_ops, name, getattr(emu_eval_ops, name))
    from climate2weather_amd.score import ScoreUNet
    from climate2weather_amd.training import Trainer

    torch.manual_seed(3 + 100 * rank)  # the trainer broadcasts rank 0's weights
    net = ScoreUNet(**CFG)
    tr = Trainer(net, lr=1e-3, precision="fp32", ema_rates=[0.9])
    res = tr.validate(held_out(), weights="net", batch=2, bins=4, seed=5, window=3)
    torch.save(dict(table=res.table.clone(), count=res.count.clone()), os.path.join(out_dir, f"valid{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()
