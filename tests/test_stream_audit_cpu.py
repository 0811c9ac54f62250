"""The stream audit (tests/stream_audit.py) against known answers, without a GPU: the vector-clock semantics one edge kind at a time,
the overlap rule, a miniature of every synchronisation pattern the product uses (clean as written, exactly one pair when its one
load-bearing edge is taken out), the footprints derived from the launchers' integer arguments against what the restatement of each
launcher really writes, the lifetime rule, and what the dispatch capture makes of plain ATen calls.  Traces are written by hand
through the constructors the recorder itself uses."""
import pytest
import torch

import emu_exact_ops
import emu_ops
import launch_replay as LR
import stream_audit as SA
from climate2weather_amd import ops as c2w_ops

M, G, S1, S2, S3 = 1, 2, 11, 12, 13  # synthetic stream handles


def fp(buf, lo=0, n=64):
    return [(buf, SA.box(lo, n), buf)]


def _keys(findings):
    return [f.key() for f in findings]


# ------------------------------------------------------------------------------------------------------------ clock semantics

def test_a_wait_on_an_event_recorded_earlier_orders():
    tr = SA.Trace()
    tr.launch("a", S1, writes=fp("x"))
    ev = tr.new_event()
    tr.record_event(ev, S1)
    tr.wait_event(S2, ev)
    tr.launch("b", S2, reads=fp("x"))
    assert len(SA.conflicting_pairs(tr)) == 1 and not SA.r1(tr)


def test_a_wait_issued_before_the_record_does_not_order():
    tr = SA.Trace()
    ev = tr.new_event()
    tr.wait_event(S2, ev)  # never recorded yet: a no-op
    tr.launch("a", S1, writes=fp("x"))
    tr.record_event(ev, S1)
    tr.launch("b", S2, reads=fp("x"))
    assert _keys(SA.r1(tr)) == [("a", 0, "b", 1)]


def test_recording_an_event_again_after_a_wait_does_not_change_the_wait():
    tr = SA.Trace()
    ev = tr.new_event()
    tr.launch("a0", S1, writes=fp("x"))
    tr.record_event(ev, S1)
    tr.wait_event(S2, ev)
    tr.launch("a1", S1, writes=fp("y"))
    tr.record_event(ev, S1)  # the wait above still holds the first snapshot
    tr.launch("b", S2, reads=fp("x") + fp("y"))
    assert _keys(SA.r1(tr)) == [("a1", 1, "b", 2)]


def test_wait_stream_orders_everything_enqueued_so_far_and_nothing_later():
    tr = SA.Trace()
    tr.launch("before0", S1, writes=fp("x"))
    tr.launch("before1", S1, writes=fp("y"))
    tr.wait_stream(S2, S1)
    tr.launch("after", S1, writes=fp("z"))
    tr.launch("b", S2, reads=fp("x") + fp("y") + fp("z"))
    assert _keys(SA.r1(tr)) == [("after", 2, "b", 3)]


def test_a_host_synchronize_of_a_side_stream_orders_later_launches_on_every_stream_behind_its_earlier_work():
    tr = SA.Trace()
    tr.launch("a", S1, writes=fp("x"))
    tr.sync_stream(S1)
    tr.launch("late", S1, writes=fp("y"))
    tr.launch("b", S2, reads=fp("x"))
    tr.launch("c", S3, reads=fp("x"))
    tr.launch("d", S2, reads=fp("y"))
    assert _keys(SA.r1(tr)) == [("late", 1, "d", 4)]  # b and c are behind a; only what came after the synchronize is open


def test_event_synchronize_and_device_synchronize_join_into_the_host():
    tr = SA.Trace()
    tr.launch("a", S1, writes=fp("x"))
    ev = tr.new_event()
    tr.record_event(ev, S1)
    tr.launch("a2", S1, writes=fp("y"))
    tr.sync_event(ev)
    tr.launch("b", S2, reads=fp("x") + fp("y"))
    assert _keys(SA.r1(tr)) == [("a2", 1, "b", 2)]
    tr.sync_all()
    tr.launch("c", S3, reads=fp("y"))
    assert _keys(SA.r1(tr)) == [("a2", 1, "b", 2)]


def test_a_collective_forks_from_its_stream_and_work_wait_joins_the_current_one():
    tr = SA.Trace()
    tr.launch("wgrad", S1, writes=fp("g"))
    c = tr.collective("all_reduce", S1, fp("g"))  # behind wgrad: forked from S1 here
    tr.launch("early", S1, reads=fp("g"))          # S1 has not waited for the collective
    w = tr.work_wait(S1, c)
    tr.launch("adamw", S1, reads=fp("g"))
    assert [(f.a["name"], f.b["name"]) for f in SA.r1(tr)] == [("all_reduce", "early")]
    assert [(f.a["name"], f.b["name"]) for f in SA.r1(tr, drop=w)] == [("all_reduce", "early"), ("all_reduce", "adamw")]


def test_order_is_transitive_over_three_streams():
    tr = SA.Trace()
    tr.launch("a", S1, writes=fp("x"))
    tr.wait_stream(S2, S1)
    tr.launch("b", S2, writes=fp("y"))
    w = tr.wait_stream(S3, S2)
    tr.launch("c", S3, reads=fp("x"))
    assert not SA.r1(tr)
    assert _keys(SA.r1(tr, drop=w)) == [("a", 0, "c", 2)]


def test_no_implicit_order_with_the_default_stream():
    tr = SA.Trace()
    tr.launch("a", 0, writes=fp("x"))
    tr.launch("b", S1, reads=fp("x"))
    assert _keys(SA.r1(tr)) == [("a", 0, "b", 1)]


# ------------------------------------------------------------------------------------------------------------------- overlap

def _two(fa, fb, wa=True, wb=False, sb=S2):
    tr = SA.Trace()
    tr.launch("a", S1, **{"writes" if wa else "reads": fa})
    tr.launch("b", sb, **{"writes" if wb else "reads": fb})
    return SA.r1(tr)


def test_a_one_byte_overlap_counts_and_names_the_byte():
    (f,) = _two(fp("x", 0, 64), fp("x", 63, 10))
    assert f.bytes == (63, 64)


def test_adjacent_ranges_do_not_conflict():
    assert not _two(fp("x", 0, 64), fp("x", 64, 64))


def test_two_reads_never_conflict():
    assert not _two(fp("x"), fp("x"), wa=False, wb=False)
    assert len(_two(fp("x"), fp("x"), wa=False, wb=True)) == 1


def test_the_same_stream_never_conflicts_with_itself():
    assert not _two(fp("x"), fp("x"), wb=True, sb=S1)


def test_the_gaps_between_rows_are_not_part_of_a_box():
    rows = [("x", SA.rows_box(0, 4, 8, 32), "y")]  # bytes 0-8, 32-40, 64-72, 96-104
    assert not _two(rows, [("x", SA.rows_box(8, 4, 24, 32), "pad")], wb=True)
    assert _two(rows, [("x", SA.box(39, 1), "z")], wb=True)[0].bytes == (39, 40)
    assert not _two(rows, [("x", SA.box(40, 24), "z")], wb=True)


def test_tensor_box_of_a_column_slice_and_of_a_tail():
    buf = torch.zeros(6, 16)
    lo = buf.data_ptr()
    assert SA.tensor_box(buf[:, :5]) == (lo, 6, 20, 64)
    assert SA.tensor_box(buf.reshape(-1)[10:]) == (lo + 40, 1, 86 * 4, 86 * 4)
    assert SA.tensor_box(buf[2:4]) == (lo + 128, 1, 128, 128)


# ----------------------------------------------------------------------------------------- the product's patterns in miniature

def _grad_stream():
    """Engine._on_grad_stream / join_grad_stream"""
    tr = SA.Trace()
    tr.launch("conv", M, writes=fp("gy"))
    tr.wait_stream(G, M)
    tr.launch("conv_wgrad", G, reads=fp("gy"), writes=fp("flat_grad"))
    tr.launch("conv", M, reads=fp("gy"), writes=fp("gx"))
    edge = tr.wait_stream(M, G)  # join_grad_stream at the end of backward
    tr.launch("adamw_ema", M, reads=fp("flat_grad"), writes=fp("flat"))
    return tr, edge, ("conv_wgrad", 1, "adamw_ema", 3)


def _pk_sync():
    """Engine._packed: one event per pack launch, a per-stream seen set, a newcomer packed by another stream"""
    tr = SA.Trace()
    tr.launch("pack_conv_weights_batched", S1, writes=fp("pk", 0, 100))
    e1 = tr.new_event()
    tr.record_event(e1, S1)
    tr.launch("conv", S1, reads=fp("pk", 0, 100))
    tr.wait_event(S2, e1)
    tr.launch("conv", S2, reads=fp("pk", 0, 100))
    tr.launch("pack_conv_weights_batched", S2, writes=fp("pk", 100, 100))  # the newcomer
    e2 = tr.new_event()
    tr.record_event(e2, S2)
    tr.launch("conv", S2, reads=fp("pk", 100, 100))
    edge = tr.wait_event(S1, e2)  # S1 is not in the newcomer's seen set yet
    tr.launch("conv", S1, reads=fp("pk", 100, 100))
    return tr, edge, ("pack_conv_weights_batched", 3, "conv", 5)


def _prefetch():
    """Engine.prefetch_backward_operands and the wait for _dg_ready in backward"""
    tr = SA.Trace()
    tr.launch("adamw_ema", M, writes=fp("flat"))
    tr.wait_stream(G, M)
    tr.launch("weight_transpose_batched", G, reads=fp("flat"), writes=fp("dg"))
    ev = tr.new_event()
    tr.record_event(ev, G)
    tr.launch("conv", M, reads=fp("shadow"), writes=fp("y"))
    edge = tr.wait_event(M, ev)
    tr.launch("conv", M, reads=fp("dg"), writes=fp("gx"))
    return tr, edge, ("weight_transpose_batched", 1, "conv", 3)


def _window_batches():
    """score_fn: window batches alternating over side streams, joined one by one at the end"""
    tr = SA.Trace()
    tr.launch("affine_channels", M, writes=fp("xd", 0, 300))
    tr.wait_stream(S1, M)
    tr.wait_stream(S2, M)
    for bi, st in enumerate((S1, S2, S1)):
        tr.launch("window_gather", st, reads=fp("xd", 0, 300), writes=fp(f"rows{st}"))
        tr.launch("window_scatter", st, reads=fp(f"rows{st}"), writes=fp("eps", 100 * bi, 100))
    tr.wait_stream(M, S1)
    edge = tr.wait_stream(M, S2)
    tr.launch("sampler_predict", M, reads=fp("eps", 0, 300), writes=fp("x", 0, 300))
    return tr, edge, ("window_scatter", 4, "sampler_predict", 7)


def _bucket():
    """Trainer._on_progress / _finish_allreduce with the bf16 wire format on the communication stream"""
    tr = SA.Trace()
    tr.launch("conv_wgrad", M, writes=fp("flat_grad"))
    tr.wait_stream(G, M)
    tr.access("aten::copy_", G, reads=fp("flat_grad"), writes=fp("wire"), src="aten")
    c = tr.collective("all_reduce", G, fp("wire"))
    tr.work_wait(G, c)
    tr.access("aten::copy_", G, reads=fp("wire"), writes=fp("flat_grad"), src="aten")
    tr.launch("conv", M, writes=fp("gx"))
    edge = tr.wait_stream(M, G)  # the ONE point where the compute stream waits
    tr.launch("adamw_ema", M, reads=fp("flat_grad"), writes=fp("flat"))
    return tr, edge, ("aten::copy_", None, "adamw_ema", 2)


def _run_ahead():
    """Trainer._step_done: step k + 2 is not enqueued before step k has finished -- what step k's gradient stream still reads may
    then be handed to any stream"""
    tr = SA.Trace()
    tr.launch("conv_wgrad", G, reads=fp("tmp"), writes=fp("flat_grad"))
    tr.wait_stream(M, G)
    ev = tr.new_event()
    tr.record_event(ev, M)
    tr.launch("conv", M, writes=fp("y"))  # step k + 1
    edge = tr.sync_event(ev)              # step k + 2 begins
    tr.launch("window_gather", S3, writes=fp("tmp"))  # the block, reused elsewhere
    return tr, edge, ("conv_wgrad", 0, "window_gather", 2)


@pytest.mark.parametrize("pattern", [_grad_stream, _pk_sync, _prefetch, _window_batches, _bucket, _run_ahead], ids=lambda f: f.__name__)
def test_a_product_pattern_is_clean_and_reports_exactly_one_pair_without_its_load_bearing_edge(pattern):
    tr, edge, want = pattern()
    pairs = SA.conflicting_pairs(tr)
    assert pairs and not SA.r1(tr, pairs)
    bad = SA.r1(tr, pairs, drop=edge)
    assert _keys(bad) == [want], [f.text for f in bad]
    assert bad[0].b["pos"] > edge  # the later entry lies behind the edge
    text = bad[0].text
    assert want[0] in text and want[2] in text and "bytes [" in text and "last wait" in text
    if pattern is not _run_ahead:
        assert SA.power(tr, pairs)[edge], "the power check must classify this edge as load-bearing"


def test_two_joins_back_to_back_are_twins_and_load_bearing_as_a_group():
    tr = SA.Trace()
    tr.launch("conv_wgrad", G, writes=fp("flat_grad"))
    first = tr.wait_stream(M, G)   # join_grad_stream at the end of backward
    tr.launch("mul", M, writes=fp("loss"))
    second = tr.wait_stream(M, G)  # _finish_allreduce, with the gradient stream as the communication stream and nothing new on it
    tr.launch("adamw_ema", M, reads=fp("flat_grad"))
    tr.launch("conv_wgrad", G, writes=fp("other"))
    third = tr.wait_stream(M, G)
    tw = SA.twins(tr)
    assert tw[first] == tw[second] == [first, second] and tw[third] == [third]
    assert not SA.r1(tr, drop=first) and not SA.r1(tr, drop=second)
    assert _keys(SA.r1(tr, drop={first, second})) == [("conv_wgrad", 0, "adamw_ema", 2)]


def test_power_classifies_a_redundant_edge():
    tr = SA.Trace()
    tr.launch("conv_wgrad", G, writes=fp("flat_grad"))
    first = tr.wait_stream(M, G)
    again = tr.wait_stream(M, G)  # a second join with nothing new behind it
    tr.launch("adamw_ema", M, reads=fp("flat_grad"))
    pw = SA.power(tr)
    assert pw[first] == [] and pw[again] == []  # either of the two joins alone still orders the optimizer: each is redundant
    tr2, _, _ = _grad_stream()
    assert [bool(v) for v in SA.power(tr2).values()] == [True, True]  # the fork and the join


# ------------------------------------------------------------------------------- footprints against the launchers' restatements

C1, C2 = 1.5, 2.25  # two canaries; positive, so that second moments stay second moments


def _declared_equals_written(name, fn, args, outs):
    """Run the restatement twice on output buffers pre-filled with two canaries.  An element was written if both runs left the same
    value there -- or if a run changed it: an accumulating output (dw += ...) depends on what was there and never agrees between
    the runs.  That set must EQUAL the declared write footprint, byte for byte, over every buffer handed in."""
    got = []
    for c in (C1, C2):
        for o in outs:
            o.fill_(c)
        fn(**args)
        got.append([o.clone() for o in outs])
    ba = LR.SIGS[name].bind(**args)
    ba.apply_defaults()
    _, writes = SA.footprints(name, SA.plain(dict(ba.arguments)))
    stores = {o.untyped_storage().data_ptr() for o in outs}
    assert all(sk in stores for sk, _, _ in writes), "a declared write outside the buffers of this case"
    for o, o1, o2 in zip(outs, *got):
        assert o.is_contiguous() and o.storage_offset() == 0
        touched = ((o1 == o2) | (o1 != C1) | (o2 != C2)).reshape(-1).repeat_interleave(o.element_size())
        declared = torch.zeros(o.numel() * o.element_size(), dtype=torch.bool)
        for sk, b, _ in writes:
            if sk == o.untyped_storage().data_ptr():
                for lo, hi in SA.ranges(b):
                    assert o.data_ptr() <= lo and hi <= o.data_ptr() + declared.numel(), f"{name}: declared bytes outside the buffer"
                    declared[lo - o.data_ptr(): hi - o.data_ptr()] = True
        assert touched.any(), f"{name}: the restatement wrote nothing"
        extra, missing = int((declared & ~touched).sum()), int((touched & ~declared).sum())
        assert extra == 0 and missing == 0, f"{name}: {extra} declared bytes never written, {missing} written bytes not declared"


def _g(**kw):
    g = dict(B=2, Hin=4, Win=4, Cin=16, Hout=4, Wout=4, Cout=48, ldy=64, wrows=64, mode=emu_ops.CONV_S1)
    g.update(kw)
    return g


def _rand(*shape, seed=0, dtype=torch.float32):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * 0.5).to(dtype)


def _conv_case(g, dtype=emu_ops.DTYPE_F32, **kw):
    T = emu_ops.TD[dtype]
    taps = 1 if g["mode"] == emu_ops.CONV_1X1 else 9
    x = _rand(g["B"] * g["Hin"] * g["Win"], g["Cin"], seed=1, dtype=T)
    w = _rand(g["wrows"] * taps * g["Cin"] + 100, seed=2, dtype=T)  # an open-ended tail, as the engine hands it over
    bias = _rand(g["wrows"] + 7, seed=3)
    npix = g["B"] * g["Hout"] * g["Wout"]
    y = torch.empty(npix * g["ldy"] + 96, dtype=T)  # room behind the last row
    return dict(x=x, w=w, bias=bias, y=y, g=g, dtype=dtype, **kw), [y], T, npix


def test_conv_writes_rows_times_cout_and_neither_padding_columns_nor_the_tail():
    args, outs, _, _ = _conv_case(_g())  # Cout 48 of ldy 64, 64 padded weight rows
    _declared_equals_written("conv", emu_ops.conv, args, outs)


def test_conv_with_a_second_output_in_bf16():
    args, outs, T, npix = _conv_case(_g(), dtype=emu_ops.DTYPE_BF16)
    y2 = torch.empty(npix * 64 + 32, dtype=T)
    _declared_equals_written("conv", emu_ops.conv, dict(args, y2=y2), outs + [y2])


def test_conv_pool2_writes_a_quarter_of_the_rows():
    g = _g(Hin=8, Win=16, Hout=8, Wout=16, B=1)
    assert emu_ops.conv_pool2_supported(g, emu_ops.DTYPE_F32)
    args, outs, _, _ = _conv_case(g, pool2=True)
    _declared_equals_written("conv", emu_ops.conv, args, outs)


def test_conv_with_an_emitted_layernorm_and_kept_statistics():
    g = _g(Cout=64, Hin=8, Win=16, Hout=8, Wout=16)
    args, outs, T, npix = _conv_case(g)
    stats = torch.empty(2 * npix + 40)  # rstd, then room: one buffer, two views
    lnf = dict(y=torch.empty(npix * 64 + 64, dtype=T), m=_rand(2, 80, seed=5), ldm=80, eps=1e-5, unbiased=False, rstd=stats[:npix + 20])
    _declared_equals_written("conv", emu_ops.conv, dict(args, lnf=lnf), outs + [lnf["y"], stats])


def test_conv_with_the_fused_layernorm_backward_accumulates_one_row_per_image():
    g = _g(Cout=64, Hin=8, Win=16, Hout=8, Wout=16)
    args, outs, T, npix = _conv_case(g)
    dm_all = torch.empty(3 * 80 + 11)  # [B][ldm] rows inside a larger modulation-gradient buffer, from an offset on
    ln = dict(x=_rand(npix, 64, seed=6, dtype=T), m=_rand(2, 80, seed=7), dm=dm_all[16:], ldm=80, eps=1e-5, unbiased=False)
    _declared_equals_written("conv", emu_ops.conv, dict(args, ln=ln, res=_rand(npix, 64, seed=8, dtype=T)), outs + [dm_all])


def _wgrad_buffers(g, n=1):
    flat = torch.empty(n * (g["Cout"] * 9 * g["Cin"] + g["Cout"]) + 500)  # flat_grad: [dw | dbias] per layer, then other layers
    npix = g["B"] * g["Hout"] * g["Wout"]
    items = []
    for i in range(n):
        off = 40 + i * (g["Cout"] * 9 * g["Cin"] + g["Cout"])
        items.append((_rand(g["B"] * g["Hin"] * g["Win"], g["Cin"], seed=10 + i), _rand(npix, g["ldy"], seed=20 + i), flat[off:],
                      flat[off + g["Cout"] * 9 * g["Cin"]:]))
    return flat, items


def test_conv_wgrad_writes_its_matrix_and_bias_row_of_the_flat_gradient_and_nothing_behind_them():
    g = _g()
    flat, [(x, dy, dw, db)] = _wgrad_buffers(g)
    _declared_equals_written("conv_wgrad", emu_ops.conv_wgrad, dict(x=x, dy=dy, dw=dw, g=g, dtype=emu_ops.DTYPE_F32, dbias=db), [flat])


def test_conv_wgrad_grouped_writes_every_items_matrix_and_bias_row():
    g = _g()
    flat, items = _wgrad_buffers(g, n=2)
    _declared_equals_written("conv_wgrad_grouped", emu_ops.conv_wgrad_grouped, dict(items=items, g=g, dtype=emu_ops.DTYPE_F32), [flat])


F_, HW_, K_ = 5, 12, 1  # five variables, twelve pixels, windows of three frames: 15 of ldc = 32 channels


def test_window_gather_of_a_partial_batch_that_does_not_start_at_window_zero():
    x = _rand(9, F_, HW_, seed=1)
    y = torch.empty(3 * HW_ * 32 + 8)  # room for a full batch of three windows
    _declared_equals_written("window_gather", emu_ops.window_gather, dict(x=x, y=y, nw=2, F=F_, HW=HW_, k=K_, i0=3, ldc=32, dtype=emu_ops.DTYPE_F32), [y])


@pytest.mark.parametrize("i0,nw", [(0, 3), (3, 2), (5, 2)], ids=["first", "middle", "last-partial"])
def test_window_scatter_writes_the_frames_the_fold_keeps(i0, nw):
    L = 9
    nwin = L - 2 * K_  # 7 windows
    eps = torch.empty(L * F_ * HW_ + 30)
    y = _rand(nw * HW_, 32, seed=2)
    _declared_equals_written("window_scatter", emu_ops.window_scatter,
                             dict(y=y, eps=eps, nw=nw, F=F_, HW=HW_, k=K_, i0=i0, nwin_total=nwin, ldc=32, dtype=emu_ops.DTYPE_F32), [eps])
    want = {(0, 3): [0, 1, 2, 3], (3, 2): [4, 5], (5, 2): [6, 7, 8]}[(i0, nw)]
    assert sorted(set(SA.kept_frames(nw, K_, i0, nwin))) == want


def test_conv_center_writes_nr_planes_per_image_at_the_trajectorys_stride():
    H, W, Cin, Fc, k = 8, 16, 64, 5, 1
    assert emu_ops.conv_center_supported(H, W, Cin, Fc, emu_ops.DTYPE_F32)
    eps = torch.empty(7 * Fc * H * W + 50)
    i0, B = 2, 2
    args = dict(x=_rand(B * H * W, Cin, seed=1), w=_rand(3 * Fc * 9 * Cin + 64, seed=2), bias=_rand(3 * Fc + 3, seed=3), out=eps[(i0 + k) * Fc * H * W:],
                B=B, H=H, W=W, Cin=Cin, wrows=3 * Fc, r0=k * Fc, nr=Fc, ostride=Fc * H * W, dtype=emu_ops.DTYPE_F32)
    _declared_equals_written("conv_center", emu_ops.conv_center, args, [eps])
    args["nr"], args["ostride"] = 3, 2 * Fc * H * W  # fewer rows than the stride: gaps between the images
    _declared_equals_written("conv_center", emu_ops.conv_center, args, [eps])


def test_window_grad_fold_list_adds_into_its_frame_range_only():
    n, w = 3, 2 * K_ + 1
    out = torch.empty(8 * F_ * HW_)  # frames 0-1 and 5-7 stay as they are
    args = dict(dx=_rand(n * w * F_ * HW_ + 10, seed=4), out=out, first=torch.tensor([1, 2, 3], dtype=torch.int32), n=n, l0=2, nl=3, F=F_, HW=HW_, k=K_, scale=0.5)
    _declared_equals_written("window_grad_fold_list", emu_exact_ops.window_grad_fold_list, args, [out])


def test_window_cotangent_list_writes_every_row_of_its_windows_padding_included():
    n, L, nobs = 2, 6, 3
    dy = torch.empty(3 * HW_ * 32 + 16)
    args = dict(delta=_rand(1, nobs, F_, HW_, seed=5), dy=dy, first=torch.tensor([0, 3], dtype=torch.int32), kind=torch.tensor([1, 2], dtype=torch.int32),
                n=n, L=L, F=F_, HW=HW_, k=K_, t_step=2, nobs=nobs, ldc=32, dtype=emu_ops.DTYPE_F32)
    _declared_equals_written("window_cotangent_list", emu_exact_ops.window_cotangent_list, args, [dy])


def test_adamw_ema_on_a_slice_writes_n_elements_of_every_state_buffer():
    N, s, e = 300, 40, 250
    p, m, v, ema = (torch.empty(N) for _ in range(4))
    shadow = torch.empty(N, dtype=torch.bfloat16)
    g = _rand(N, seed=6)
    args = dict(p=p[s:], g=g[s:], m=m[s:], v=v[s:], ema=ema[s:], shadow=shadow[s:], n=e - s, lr=1e-2, beta1=0.9, beta2=0.99, eps=1e-8, weight_decay=0.1,
                step=3, ema_rate=0.9, grad_scale=1.0)
    _declared_equals_written("adamw_ema", emu_ops.adamw_ema, args, [p, m, v, ema, shadow])
    reads, _ = SA.footprints("adamw_ema", SA.plain(dict(LR.SIGS["adamw_ema"].bind(**args).arguments)))
    assert [b for _, b, pth in reads if pth == "g"] == [SA.box(g.data_ptr() + 4 * s, 4 * (e - s))]


def test_nchw_to_nhwc_writes_the_padding_columns_too():
    B, C, HW, ldc = 2, 5, 12, 8
    y = torch.empty(B * HW * ldc + 24)
    args = dict(x=_rand(B, C, HW, seed=7), eps=None, musig=None, y=y, B=B, C=C, HW=HW, ldc=ldc, dtype=emu_ops.DTYPE_F32)
    _declared_equals_written("nchw_to_nhwc", emu_ops.nchw_to_nhwc, args, [y])


def test_packed_weights_are_written_and_read_per_matrix():
    src, dst = torch.zeros(5000, dtype=torch.bfloat16), torch.zeros(80000, dtype=torch.bfloat16)
    a = SA.plain(dict(src=src, dst=dst, desc=torch.zeros(8, dtype=torch.int64), n=2, dtype=1))
    a["desc_rows"] = [(100, 0, 4, 32), (2000, 40000, 3, 32)]
    reads, writes = SA.footprints("pack_conv_weights_batched", a)
    per = 9 * 32 * 128 * 2
    assert [b for _, b, p in writes if p == "dst"] == [SA.box(dst.data_ptr(), per), SA.box(dst.data_ptr() + 80000, per)]
    assert [b for _, b, p in reads if p == "src"] == [SA.box(src.data_ptr() + 200, 4 * 9 * 32 * 2), SA.box(src.data_ptr() + 4000, 3 * 9 * 32 * 2)]


def test_scratch_arguments_count_as_written():
    ws = torch.zeros(64)
    g = _g()
    flat, [(x, dy, dw, db)] = _wgrad_buffers(g)
    ba = LR.SIGS["conv_wgrad"].bind(x, dy, dw, g, 0, dbias=db, workspace=ws)
    ba.apply_defaults()
    _, writes = SA.footprints("conv_wgrad", SA.plain(dict(ba.arguments)))
    assert ("workspace" in [p for _, _, p in writes]) and SA.box(ws.data_ptr(), 256) in [b for _, b, _ in writes]


# -------------------------------------------------------------------------------------------------- the recorder on CPU tensors

def _recording(monkeypatch, cur):
    return SA.record(monkeypatch, c2w_ops, gpu=False, current_stream=lambda: cur[0])


def test_a_temporary_that_crosses_streams_needs_record_stream(monkeypatch):
    cur = [S1]
    with _recording(monkeypatch, cur) as tr:
        t = torch.empty(64)  # fresh on S1
        key = t.untyped_storage().data_ptr()
        cur[0] = S2
        t.add_(1)
        del t
    assert tr.storages[key]["fresh"] == S1 and tr.storages[key]["owned"] is False
    (bad,) = SA.r2(tr)
    assert bad[0] == key and bad[1] == S2 and bad[2][0] == "aten::add_"
    with pytest.raises(AssertionError, match="record_stream"):
        SA.assert_clean(tr)
    # an entry of the exemption table does not help: the block was let go while S1, whose pool it returns to, knew nothing of S2's use
    (still,) = SA.r2(tr, exempt={("aten::add_", "self"): "for the test"})
    assert "released before" in still[3] and tr.storages[key]["released"] is not None


def test_an_exempted_temporary_must_be_let_go_behind_a_join(monkeypatch):
    cur = [S1]
    with _recording(monkeypatch, cur) as tr:
        t = torch.empty(64)
        key = t.untyped_storage().data_ptr()
        cur[0] = S2
        t.add_(1)
        tr.wait_stream(S1, S2)  # the allocating stream joins the user ...
        del t                   # ... and only then the last owner lets go
    assert tr.entries[tr.storages[key]["released"]]["kind"] == "release"
    assert len(SA.r2(tr)) == 1 and not SA.r2(tr, exempt={("aten::add_", "self"): "joined before it is dropped"})


def test_a_temporary_with_record_stream_and_a_persistent_buffer_are_fine(monkeypatch):
    cur = [S1]
    with _recording(monkeypatch, cur) as tr:
        t = torch.empty(64)
        kept = torch.empty(64)
        keys = [t.untyped_storage().data_ptr(), kept.untyped_storage().data_ptr()]
        tr.note_record_stream(keys[0], S2)  # what Tensor.record_stream records on a device
        cur[0] = S2
        t.add_(1)
        kept.add_(1)
        del t
    assert tr.storages[keys[0]]["owned"] is False and tr.storages[keys[1]]["owned"] is True
    assert SA.r2_crossings(tr) == 2 and not SA.r2(tr)
    assert kept is not None


def test_a_buffer_that_existed_before_the_recording_is_not_a_temporary(monkeypatch):
    cur = [S1]
    old = torch.zeros(64)
    with _recording(monkeypatch, cur) as tr:
        cur[0] = S2
        old.add_(1)
    assert tr.storages[old.untyped_storage().data_ptr()]["fresh"] is None and not SA.r2(tr)


def test_dispatch_capture_of_plain_aten_calls(monkeypatch):
    cur = [S1]
    buf, src = torch.ones(100), torch.arange(10.0)
    lo = buf.data_ptr()
    with _recording(monkeypatch, cur) as tr:
        buf[10:20].zero_()
        buf[3:7].view(2, 2).t()  # views: nothing
        n = len(tr.entries)
        buf[50:60].copy_(src)
        v = float(buf[0].item())
    z, c, it = tr.accesses()
    assert n == 1 and v == 1.0
    assert z["name"] == "aten::zero_" and [b for _, b, _ in z["writes"]] == [SA.box(lo + 40, 40)] and not z["reads"]
    assert c["name"] == "aten::copy_" and [b for _, b, _ in c["writes"]] == [SA.box(lo + 200, 40)] and [b for _, b, _ in c["reads"]] == [SA.box(src.data_ptr(), 40)]
    assert [b for _, b, _ in it["reads"]] == [SA.box(lo, 4)] and tr.entries[-1] == dict(kind="host", what="stream", tl=S1, pos=it["pos"] + 1)


def test_the_recorder_sees_every_launch_of_an_emulated_step_and_host_queries_record_nothing(monkeypatch):
    from test_launch_replay_cpu import _batch, _net
    from climate2weather_amd.training import Trainer
    emu_ops.install(monkeypatch, c2w_ops)
    x, t, eps = _batch()
    tr_ = Trainer(_net(), lr=1e-3, precision="bf16", ema_rates=[0.9])
    tr_.step(x, t=t, eps=eps)
    with _recording(monkeypatch, [S1]) as tr:
        tr.recorder.name_storages(tr_.eng, "eng")
        tr_.step(x, t=t, eps=eps)
    names = {e["name"] for e in tr.accesses() if e["src"] == "ops"}
    assert tr.launches == sum(tr.calls.values()) > 50 and {"conv", "conv_wgrad", "adamw_ema"} <= names
    assert not any(LR.is_host_query(n) or n in SA.UNRECORDED for n in names)
    assert any(e["name"] == "aten::zero_" for e in tr.accesses())  # flat_grad.zero_()
    wg = next(e for e in tr.accesses() if e["name"] == "conv_wgrad")
    sk, b, _ = wg["writes"][0]
    assert tr.name_of(sk, b[0]).startswith("eng.flat_grad+") and SA.hull(b)[1] - b[0] < tr_.eng.flat_grad.numel() * 4 // 2
    assert not SA.conflicting_pairs(tr)  # one stream
