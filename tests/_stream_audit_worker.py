"""Worker of tests/test_gpu_stream_order.py::test_bucketed_all_reduce_over_rccl_single_rank: one rank over RCCL (a real communicator,
real collectives), the tiny network of tests/_ddp_worker.py, small buckets.  Per case -- fp32 wire, bf16 wire, chased optimizer -- two
warmed-up steps are recorded once (tests/stream_audit.py), analysed here, and what was found goes to ``stream_audit.json`` for the parent."""
import json
import os
import sys
from collections import Counter

import numpy as np
import pytest
import torch
import torch.distributed as dist


def run(rank: int, port: int, golden_dir: str, out_dir: str):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from _ddp_worker import _init
    dev = _init(rank, 1, port, "nccl")
    import stream_audit as SA
    from climate2weather_amd import ops
    from climate2weather_amd.score import ScoreUNet
    from climate2weather_amd.training import Trainer
    from test_gpu_stream_order import count_calls, load_bearing, mark, waits_in

    os.environ["C2W_FORCE_DIST"] = "1"  # one rank: still bucket and all-reduce through the communicator
    g = np.load(os.path.join(golden_dir, "tiny_net.npz"))
    x, t, eps = (torch.from_numpy(g[k]).to(dev) for k in ("x", "t", "eps"))
    t = t.reshape(-1)
    steps, res = 2, {}
    for case in ("fp32", "bf16", "chase"):
        torch.manual_seed(3)
        net = ScoreUNet(channels=6, spatial=2, activation=torch.nn.SiLU, embedding_dim=64, hidden_channels=[32, 64], hidden_blocks=[1, 1],
                        attention_levels=[1], kernel_size=3, padding_mode="zeros").to(dev)
        tr = Trainer(net, lr=1e-3, precision="fp32", ema_rates=[0.9], bucket_mb=0.05, allreduce_dtype="bf16" if case == "bf16" else "fp32")
        tr.chase_optimizer = case == "chase"
        assert tr.sync_grads and len(tr.buckets) > 4 and (tr.wire is not None) == (case == "bf16")
        tr.step(x, t=t, eps=eps)
        torch.cuda.synchronize()
        counter, marks = Counter(), []
        mp = pytest.MonkeyPatch()
        try:
            count_calls(mp, ops, counter)
            with SA.record(mp, ops, dist_module=dist) as trace:
                trace.recorder.name_storages(tr.eng, "eng")
                trace.recorder.name_storages(tr, "trainer")
                mark(mp, trace, Trainer, "_finish_allreduce", marks)
                for _ in range(steps):
                    tr.step(x, t=t, eps=eps)
                weights = tr.eng.flat.clone()  # whoever runs next on the compute stream: the reader the last step's join is for
                torch.cuda.synchronize()
        finally:
            mp.undo()
        pairs = SA.conflicting_pairs(trace)
        pw = SA.power(trace, pairs)
        compute = torch.cuda.current_stream().cuda_stream
        final = [w for _, p0, p1 in marks for w in waits_in(trace, p0, p1, tl=compute)]  # the compute stream's waits in _finish_allreduce
        verdicts = [load_bearing(trace, pairs, pw, w) for w in final]
        kinds = Counter()
        for pos, bad in pw.items():
            e = trace.entries[pos]
            kinds[(f"stream {e['tl']} waits" + (" for a collective" if e["kind"] == "waittl" else ""), "load-bearing" if bad else "redundant")] += 1
        res[case] = dict(
            stats=SA.stats(trace, pairs, pw), r1=[f.text for f in SA.r1(trace, pairs)], r2=[repr(b) for b in SA.r2(trace)],
            launches=trace.launches, counted=sum(counter.values()), buckets=len(tr.buckets), steps=steps,
            collectives=sum(1 for e in trace.accesses() if e["src"] == "coll"), grad_stream=tr.eng.grad_stream() is not None,
            final=final, final_load_bearing=sum(1 for ok, _ in verdicts if ok), final_with_twin=sum(1 for ok, tw in verdicts if ok and tw),
            edges=[f"{who}: {n} {verdict}" for (who, verdict), n in sorted(kinds.items())])
        if os.environ.get("STREAM_AUDIT_DUMP"):
            import pickle
            os.makedirs(os.environ["STREAM_AUDIT_DUMP"], exist_ok=True)
            with open(os.path.join(os.environ["STREAM_AUDIT_DUMP"], f"collectives_{case}_{os.environ.get('C2W_WGRAD_STREAM', '0')}.pkl"), "wb") as f:
                pickle.dump(dict(trace=trace, marks=marks, counter=dict(counter)), f)
        del weights
    with open(os.path.join(out_dir, "stream_audit.json"), "w") as f:
        json.dump(res, f)
    dist.barrier()
    dist.destroy_process_group()
