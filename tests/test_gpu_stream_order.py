"""Cross-stream ordering of real runs, audited from one recording each (tests/stream_audit.py): every launch, every ATen op and
every event edge of a training step, a two-stream backward, a multi-stream score evaluation, a validation between steps and the
bucketed all-reduce is recorded once, in host enqueue order, and checked with vector clocks -- R1: two accesses to the same bytes on
different streams, one of them a write, are ordered by some chain of edges; R2: a temporary used on another stream than the one that
allocated it had record_stream.  The verdict is a property of the enqueue order and the edges, not of timing: nothing is repeated,
nothing has to go wrong on the device, and a pair of streams that happens to share a hardware queue hides nothing.

Power check, on the recorded trace and on the host only: every wait edge is deleted alone and the trace analysed again.  The final
joins -- join_grad_stream at the end of the backward, the wait_stream loop at the end of BatchedScoreFunction.score_fn, the compute
stream's wait in Trainer._finish_allreduce -- must each be load-bearing (their deletion brings a finding whose later entry lies
behind them); the other edges are classified and printed.  Where two of them coincide -- with C2W_WGRAD_STREAM=1 the gradient stream
is the communication stream, and under the bf16 wire or the chased optimizer _finish_allreduce's wait comes directly behind backward's
own join with nothing new on that stream in between -- each is redundant alone by construction (stream_audit.twins); there the group
is deleted together and must be load-bearing, and the output says so (measured: profiles/stream_audit.md).  A trace must not be vacuous: the expected number of streams, at least one
cross-stream pair looked at, and as many recorded launches as a plain call counter under the recorder saw.

Out of scope: captured hipGraphs, races between the workgroups of one kernel, whether streams overlap in time (streams.overtakes),
two ranks.  STREAM_AUDIT_DUMP=<directory> keeps every trace as a pickle for analysis elsewhere.
"""
import json
import os
import pickle
import socket
import time
from collections import Counter

import pytest
import torch

import launch_replay as LR
import stream_audit as SA
from climate2weather_amd import ops
from climate2weather_amd.engine import Engine
from climate2weather_amd.pipelines import SDAPipeline
from climate2weather_amd.score_fn import BatchedScoreFunction, PoolStrideOperator
from climate2weather_amd.training import Trainer
from test_gpu_launch_layer import knob  # noqa: F401  (the fixture: sets a knob, reloads the library's table, undoes both)
from test_gpu_launch_replay import DEV, _data, _net, _windows

pytestmark = pytest.mark.gpu


def count_calls(mp, ops_module, counter):
    """the plain call counter the recorder is held against: installed UNDER it, it knows nothing of footprints or streams"""
    for name in sorted(LR.SIGS):
        fn = getattr(ops_module, name, None)
        if fn is None or not callable(fn) or name in SA.UNRECORDED or LR.is_host_query(name):
            continue

        def wrap(name=name, fn=fn):
            def counted(*a, **kw):
                ret = fn(*a, **kw)
                if ret is not False:
                    counter[name] += 1
                return ret
            return counted
        mp.setattr(ops_module, name, wrap())


def mark(mp, tr, cls, method, marks):
    """note which trace entries a call of cls.method added: (method, first position, position behind the last)"""
    real = getattr(cls, method)

    def wrapped(self, *a, **kw):
        p0 = len(tr.entries)
        try:
            return real(self, *a, **kw)
        finally:
            marks.append((method, p0, len(tr.entries)))
    mp.setattr(cls, method, wrapped)


def waits_in(tr, p0, p1, tl=None):
    return [e["pos"] for e in tr.entries[p0:p1] if e["kind"] in ("wait", "waittl") and (tl is None or e["tl"] == tl)]


def audit(monkeypatch, request, body, *, owners=(), streams=1, marked=(), dist_module=None):
    """run ``body`` once under the recorder -> (trace, pairs, marks); R1 and R2 clean, the trace not vacuous"""
    t0 = time.perf_counter()
    counter, marks = Counter(), []
    with monkeypatch.context() as mp:
        count_calls(mp, ops, counter)
        with SA.record(mp, ops, dist_module=dist_module) as tr:
            for obj, prefix in owners:
                tr.recorder.name_storages(obj, prefix)
            for cls, method in marked:
                mark(mp, tr, cls, method, marks)
            body()
    pairs = SA.conflicting_pairs(tr)
    name = request if isinstance(request, str) else request.node.name
    if os.environ.get("STREAM_AUDIT_DUMP"):
        os.makedirs(os.environ["STREAM_AUDIT_DUMP"], exist_ok=True)
        with open(os.path.join(os.environ["STREAM_AUDIT_DUMP"], name.replace("/", "_") + ".pkl"), "wb") as f:
            pickle.dump(dict(trace=tr, marks=marks, counter=dict(counter)), f)
    st = SA.stats(tr, pairs)
    print(f"\n== {name}: {json.dumps(st)} recorded in {time.perf_counter() - t0:.2f} s")
    SA.assert_clean(tr, pairs)
    assert tr.launches == sum(counter.values()) > 0 and tr.calls == dict(counter), (tr.launches, sum(counter.values()))
    assert st["launch_streams"] >= streams, f"{st['launch_streams']} streams with launches, expected at least {streams}"
    if streams > 1:
        assert pairs, "no cross-stream pair was looked at: the trace says nothing"
    return tr, pairs, marks


def load_bearing(tr, pairs, pw, pos, tw=None):
    """does deleting the join at ``pos`` bring a finding whose later entry lies behind it?  -> (verdict, twins deleted with it).  A join
    that has a twin -- another wait of the same stream for the same point of the other stream, as the wait in _finish_allreduce is of
    backward's own join when the gradient stream is the communication stream and the last bucket went out inside the backward -- is
    redundant alone by construction: the group is deleted together."""
    if any(f.b["pos"] > pos for f in pw[pos]):
        return True, []
    grp = (SA.twins(tr) if tw is None else tw).get(pos, [pos])
    if len(grp) > 1:
        return any(f.b["pos"] > min(grp) for f in SA.r1(tr, pairs, drop=set(grp))), [p for p in grp if p != pos]
    return False, []


def power(request, tr, pairs, final):
    """delete every wait edge alone; ``final``: the positions of the joins that must be load-bearing"""
    t0 = time.perf_counter()
    pw = SA.power(tr, pairs)
    assert final, "the final joins of this scenario were not found in the trace"
    tw, grouped = SA.twins(tr), 0
    for pos in final:
        ok, with_ = load_bearing(tr, pairs, pw, pos, tw)
        grouped += bool(with_)
        assert ok, f"the join at entry {pos} ({tr.entries[pos]}) is not load-bearing: deleting it (twins: {with_}) brings no finding"
    st = SA.stats(tr, pairs, pw)
    kinds = Counter()
    for pos, bad in pw.items():
        e = tr.entries[pos]
        kinds[(f"stream {e['tl']} waits" + (" for a collective" if e["kind"] == "waittl" else ""), "load-bearing" if bad else "redundant")] += 1
    name = request if isinstance(request, str) else request.node.name
    print(f"== {name}: power check of {len(pw)} edges in {time.perf_counter() - t0:.2f} s: {st['load_bearing']} load-bearing, {st['redundant']} redundant; "
          f"{len(final)} final joins, all load-bearing ({grouped} of them only together with a twin)")
    for (who, verdict), n in sorted(kinds.items()):
        print(f"   {who}: {n} {verdict}")
    return st


def final_joins_of_backward(tr, marks):
    """the wait of the last join_grad_stream in front of every optimizer launch (adamw_ema / grad_scaler_check): the one at the end of backward"""
    joins = [(p0, p1) for m, p0, p1 in marks if m == "join_grad_stream" and waits_in(tr, p0, p1)]
    out = []
    opt = [e["pos"] for e in tr.accesses() if e["name"] in ("adamw_ema", "grad_scaler_check")]
    for i, (p0, p1) in enumerate(joins):
        nxt = joins[i + 1][0] if i + 1 < len(joins) else len(tr.entries)
        if any(p1 <= o < nxt for o in opt):
            out.append(waits_in(tr, p0, p1)[-1])
    return out


def test_the_stream_methods_are_python_over_the_event_methods(monkeypatch):
    """what the recorder relies on: wait_stream, wait_event and record_event arrive through Event.record / Event.wait, once each"""
    main, side = torch.cuda.current_stream(), torch.cuda.Stream()
    with SA.record(monkeypatch, ops) as tr:
        side.wait_stream(main)
        ev = main.record_event()
        side.wait_event(ev)
        ev2 = torch.cuda.Event()
        ev2.record()
        ev2.wait(side)
        side.synchronize()
        ev2.synchronize()
        torch.cuda.synchronize()
    kinds = [(e["kind"], e.get("tl"), e.get("what")) for e in tr.entries]
    m, s = main.cuda_stream, side.cuda_stream
    assert kinds == [("record", m, None), ("wait", s, None), ("record", m, None), ("wait", s, None), ("record", m, None), ("wait", s, None),
                     ("host", s, "stream"), ("host", None, "event"), ("host", None, "all")], kinds
    assert tr.entries[0]["ev"] == tr.entries[1]["ev"] != tr.entries[2]["ev"] == tr.entries[3]["ev"]


# ------------------------------------------------------------------------------------------------------------- 1-3: Trainer.step

def _trainer(precision, **kw):
    return Trainer(_net(), lr=1e-3, precision=precision, ema_rates=[0.999], seed=11, **kw)


def _steps(tr, batches, n=3):
    def body():
        for _ in range(n):
            tr.step(batches)
        torch.cuda.synchronize()
    return body


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_three_training_steps_default_knobs(monkeypatch, request, precision):
    """scenario 1: the step boundary is inside the trace (_step_done, weights_changed, the shadow refresh, publish)"""
    monkeypatch.delenv("C2W_WGRAD_STREAM", raising=False)
    tr = _trainer(precision)
    x = _windows()
    tr.step(x)
    trace, _, _ = audit(monkeypatch, request, _steps(tr, x), owners=[(tr.eng, "eng"), (tr, "trainer")])
    assert any(e["kind"] == "host" and e["what"] == "event" for e in trace.entries), "_step_done was not synchronised inside three steps"


@pytest.mark.parametrize("case", ["bf16", "fp16", "bf16-t3-16", "bf16-deterministic"])
def test_three_training_steps_on_the_gradient_stream(monkeypatch, request, knob, case):  # noqa: F811
    """scenario 2: C2W_WGRAD_STREAM=1 -- _on_grad_stream / join_grad_stream, prefetch_backward_operands and _dg_ready; under
    C2W_CONV_T3=16 the packed weights and _pk_sync; the deterministic mode's per-stream scratch"""
    monkeypatch.setenv("C2W_WGRAD_STREAM", "1")
    if "t3" in case:
        knob("C2W_CONV_T3", "16")
    tr = _trainer(case.split("-")[0], deterministic=case.endswith("deterministic"))
    assert tr.eng.grad_stream() is not None
    x = _data() if "t3" in case else _windows()
    tr.step(x)
    trace, pairs, marks = audit(monkeypatch, request, _steps(tr, x), owners=[(tr.eng, "eng"), (tr, "trainer")], streams=2,
                                marked=[(Engine, "join_grad_stream")])
    if "t3" in case:
        assert any(e["name"] == "pack_conv_weights_batched" for e in trace.accesses())
    final = final_joins_of_backward(trace, marks)
    assert len(final) == 3, final
    power(request, trace, pairs, final)


def test_gradient_accumulation_on_the_gradient_stream(monkeypatch, request):
    """scenario 3: two rounds in one step"""
    monkeypatch.setenv("C2W_WGRAD_STREAM", "1")
    tr = _trainer("bf16")
    xs = [_windows(seed=2), _windows(seed=4)]
    tr.step(xs)
    audit(monkeypatch, request, _steps(tr, xs, n=2), owners=[(tr.eng, "eng"), (tr, "trainer")], streams=2)


def test_segmented_gradient_delivery_on_the_gradient_stream(monkeypatch, request):
    """scenario 4: the module path, score.py's per-segment events (as test_segmented_gradient_delivery_equals_the_single_node_on_the_gpu)"""
    from _module_loop import _batch
    from test_gpu_module_api import _tiny
    monkeypatch.setenv("C2W_WGRAD_STREAM", "1")
    pipe = SDAPipeline()
    net = _tiny(precision="auto")
    net.grad_segments = 4
    x = _batch(0, DEV)

    def once():
        with torch.autocast("cuda", dtype=torch.bfloat16):
            loss = pipe.loss(net=net, x=x).mean()
        loss.backward()
    once()
    torch.cuda.synchronize()
    eng = net._get_engine()
    assert eng.grad_stream() is not None

    def body():
        once()
        once()  # the second pass accumulates into the gradients the first delivered
        torch.cuda.synchronize()
    audit(monkeypatch, request, body, owners=[(eng, "eng")], streams=2)


# ----------------------------------------------------------------------------------------------------------------- 5: the sampler

@pytest.mark.parametrize("case", ["bf16", "fp16", "bf16-t3-16"])
def test_window_batches_on_four_streams_and_two_sampler_steps(monkeypatch, request, knob, case):  # noqa: F811
    """scenario 5: three co-sampled members in five window batches (the last one partial) over four streams through one shared Engine,
    twice in a row so that the second call's packs and buffers meet the first call's readers; then two SDAPipeline.sample steps with
    one corrector and guidance on the same score function"""
    if "t3" in case:
        knob("C2W_CONV_T3", "16")
    F, k, L = 13, 2, 11
    net = _net().eval().requires_grad_(False)
    net.precision = case.split("-")[0]
    pipe = SDAPipeline()
    dev = torch.device(DEV)
    sf = BatchedScoreFunction(net, markov_order=k, batch_size=5, device=dev, noise_process=pipe)  # 3 x 7 windows: 5 + 5 + 5 + 5 + 1
    assert not sf.use_graphs and sf.num_streams == 4
    net._get_engine().use_center_conv = True
    g = torch.Generator().manual_seed(5)
    A = PoolStrideOperator(8, 2)
    truth, noise = torch.randn(L, F, 32, 32, generator=g), torch.randn(L, F, 32, 32, generator=g)
    zs = [torch.randn(L, F, 32, 32, generator=g) for _ in range(2)]
    std = torch.rand(1, F, 1, 1, generator=g) * 0.2 + 0.1
    sf.condition_on(A=A, y=A(truth), std=std, gamma=1e-2, exact_grad=False)
    x = torch.randn(3, L, F, 32, 32, generator=g).to(dev)
    t = torch.tensor(0.4)
    with torch.no_grad():
        sf.score_fn(x, t)  # warm-up: lazy operands, the streams, the split-K scratch
        torch.cuda.synchronize()
    kept = []

    def body():
        with torch.no_grad():
            a = sf.score_fn(x, t)
            kept.append(a.clone())  # a reader of every frame of the result on the caller's stream: what the final joins are for
            b = sf.score_fn(x, t)
            kept.append(a + b)
            pipe.sample(sf, noise, steps=2, corrections=1, tau=0.4, device=dev, show_progressbar=False, z_draws=zs)
        torch.cuda.synchronize()
    trace, pairs, marks = audit(monkeypatch, request, body, owners=[(net._get_engine(), "eng")], streams=4,
                                marked=[(BatchedScoreFunction, "score_fn")])
    main = torch.cuda.current_stream().cuda_stream
    final = []
    for _, p0, p1 in marks:
        launches = [e["pos"] for e in trace.entries[p0:p1] if e["kind"] == "access" and e["src"] == "ops"]
        final += [w for w in waits_in(trace, p0, p1, tl=main) if w > launches[-1]]  # the loop behind the last batch
    assert len(final) >= 2 * 4 + 2, final
    power(request, trace, pairs, final)


# ------------------------------------------------------------------------------------------------- 6: validation between steps

@pytest.mark.parametrize("two_streams", ["0", "1"])
def test_validation_between_two_training_steps(monkeypatch, request, two_streams):
    monkeypatch.setenv("C2W_WGRAD_STREAM", two_streams)
    tr = _trainer("bf16")
    x, held = _data(), _data(n=8, seed=9)
    tr.step(x)
    tr.validate(held, batch=4, bins=10, seed=3, window=5)

    def body():
        tr.step(x)
        tr.validate(held, batch=4, bins=10, seed=3, window=5)
        tr.step(x)
        torch.cuda.synchronize()
    trace, _, _ = audit(monkeypatch, request, body, owners=[(tr.eng, "eng"), (tr, "trainer")], streams=1 + int(two_streams))
    assert any(e["name"] == "sq_err_levels" for e in trace.accesses())


# ------------------------------------------------------------------------------------------------------ 7: collectives over RCCL

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


@pytest.mark.parametrize("two_streams", ["0", "1"])
def test_bucketed_all_reduce_over_rccl_single_rank(golden_dir, tmp_path, monkeypatch, two_streams):
    """scenario 7, in a spawned child (a communicator wants a process of its own): the fp32 wire, the bf16 wire and the chased
    optimizer, small buckets; the child records, analyses and writes what it found, the parent asserts on that file"""
    import torch.multiprocessing as mp
    from _stream_audit_worker import run
    monkeypatch.setenv("C2W_WGRAD_STREAM", two_streams)  # the child inherits it
    mp.spawn(run, args=(_free_port(), golden_dir, str(tmp_path)), nprocs=1, join=True)
    with open(tmp_path / "stream_audit.json") as f:
        res = json.load(f)
    assert sorted(res) == ["bf16", "chase", "fp32"]
    for case, r in res.items():
        print(f"\n== collectives[{case}, C2W_WGRAD_STREAM={two_streams}]: {json.dumps(r['stats'])}")
        for line in r["edges"]:
            print("   " + line)
        assert r["r1"] == [] and r["r2"] == [], (case, r["r1"][:4], r["r2"][:4])
        assert r["launches"] == r["counted"] > 0 and r["buckets"] > 4 and r["collectives"] == r["buckets"] * r["steps"], (case, r)
        assert r["stats"]["pairs"] > 0 and r["stats"]["streams"] >= 1 + r["collectives"]
        assert r["grad_stream"] == (two_streams == "1")
        assert r["final"] and r["final_load_bearing"] == len(r["final"]), (case, r["final"], r["final_load_bearing"])
        print(f"   {len(r['final'])} waits of the compute stream in _finish_allreduce, all load-bearing ({r['final_with_twin']} only together with a twin)")
