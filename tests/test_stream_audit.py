"""tests/stream_audit.py: the checker's two rules on hand-written traces (CPU, pure Python, no library), then on the
MI355X the planted pairs on the real allocator and the product's own step, which must come out without a report.

Out of scope here as in the auditor: captured replays, graph.WGRAD_STREAM / graph.TAIL_WGRAD_SIDE (off in the product),
more than one rank; torch's own kernels are not in the log (see the auditor's docstring)."""
import math
import os
import re

import pytest

from tests.stream_audit import Checker

M, S, T = "main", "side", "third"
X, Y = 0x10000, 0x20000
AMAX_BYTES = 4097 * 4


def rd(ptr, name="x", index=0, nbytes=None):
    return (index, name, ptr, nbytes, "r")


def wr(ptr, name="y", index=1, nbytes=None):
    return (index, name, ptr, nbytes, "w")


def trace():
    c = Checker()
    c.alloc(X, 1024, M)
    return c


def done(c):
    c.close()
    return c.reports


# ---- rule 1: ordering -------------------------------------------------------------------------------------------
def test_order_event_after_write_passes():
    c = trace()
    c.launch("dasr_copy", M, [wr(X)])
    c.record_event("e", M)
    c.wait_event("e", S)
    c.record_stream(X, S)
    c.launch("dasr_add", S, [rd(X)])
    assert done(c) == []


def test_order_event_recorded_before_the_write():
    c = trace()
    c.record_event("e", M)
    c.launch("dasr_copy", M, [wr(X)])
    c.wait_event("e", S)
    c.record_stream(X, S)
    c.launch("dasr_add", S, [rd(X)], site="graph.py:1 (f)")
    r = done(c)
    assert len(r) == 1 and r[0].startswith("ORDER #1 dasr_add arg 0 'x' (read) on stream")
    assert "#0 dasr_copy arg 1 'y' (write)" in r[0] and "1024 B" in r[0] and "graph.py:1 (f)" in r[0]


def test_order_wait_on_the_wrong_event():
    c = trace()
    c.launch("dasr_copy", M, [wr(Y)])          # (Y is unknown to the trace: not an operand)
    c.record_event("early", M)
    c.launch("dasr_copy", M, [wr(X)])
    c.record_event("right", M)
    c.wait_event("early", S)
    c.record_stream(X, S)
    c.launch("dasr_add", S, [rd(X)])
    r = done(c)
    assert len(r) == 1 and r[0].startswith("ORDER #2 dasr_add") and "#1 dasr_copy" in r[0]
    c = trace()
    c.launch("dasr_copy", M, [wr(X)])
    c.record_event("right", M)
    c.record_event("other", T)
    c.wait_event("other", S)
    c.launch("dasr_add", S, [rd(X)])
    c.record_stream(X, S)
    assert len(done(c)) == 1


def test_order_wait_stream_direction():
    for waiter, waited, want in ((S, M, 0), (M, S, 1)):
        c = trace()
        c.launch("dasr_copy", M, [wr(X)])
        c.wait_stream(waiter, waited)
        c.record_stream(X, S)
        c.launch("dasr_add", S, [rd(X)])
        assert len(done(c)) == want, (waiter, waited)


def test_order_read_before_write_through_out_accumulation():
    """The side stream reads a gradient, the main stream then accumulates into it (``out=``: ``float* dx``, a write)."""
    for wait, want in ((True, 0), (False, 1)):
        c = trace()
        c.launch("dasr_conv2d_dgrad", M, [wr(X, "dx", 2)])
        c.wait_stream(S, M)
        c.record_stream(X, S)
        c.launch("dasr_conv2d_wgrad", S, [rd(X, "dconv", 1)])
        c.record_event("read", S)
        if wait:
            c.wait_event("read", M)
        c.launch("dasr_conv2d_dgrad", M, [wr(X, "dx", 2)])
        r = done(c)
        assert len(r) == want, r
        if want:
            assert "#2 dasr_conv2d_dgrad arg 2 'dx' (write)" in r[0] and "#1 dasr_conv2d_wgrad arg 1 'dconv' (read)" in r[0]


def test_order_write_write_and_third_stream():
    c = trace()
    c.launch("dasr_copy", M, [wr(X)])
    c.launch("dasr_copy", S, [wr(X)])
    c.record_stream(X, S)
    r = done(c)
    assert len(r) == 1 and "#1 dasr_copy" in r[0] and "#0 dasr_copy" in r[0]
    # ordered through a third stream: transitive
    c = trace()
    c.launch("dasr_copy", M, [wr(X)])
    c.wait_stream(T, M)
    c.wait_stream(S, T)
    c.record_stream(X, S)
    c.launch("dasr_add", S, [rd(X)])
    assert done(c) == []


def test_order_disjoint_bytes_of_one_storage_do_not_conflict():
    c = trace()
    c.record_stream(X, S)
    c.launch("dasr_copy", M, [wr(X, nbytes=512)])
    c.launch("dasr_copy", S, [wr(X + 512, nbytes=512)])
    assert done(c) == []
    c = trace()
    c.record_stream(X, S)
    c.launch("dasr_copy", M, [wr(X, nbytes=516)])
    c.launch("dasr_copy", S, [wr(X + 512, nbytes=512)])
    assert len(done(c)) == 1


def test_order_two_reads_do_not_conflict_and_host_sync_orders_everything():
    c = trace()
    c.record_stream(X, S)
    c.launch("dasr_add", M, [rd(X)])
    c.launch("dasr_add", S, [rd(X)])
    assert c.reports == []
    c.sync_all()
    c.launch("dasr_copy", T, [wr(X)])
    c.record_stream(X, T)
    assert done(c) == []
    c = trace()
    c.record_stream(X, S)
    c.launch("dasr_copy", M, [wr(X)])
    c.sync_stream(S)                            # the wrong stream: the host has not waited for main
    c.launch("dasr_add", S, [rd(X)])
    assert len(c.reports) == 1
    c.record_event("e", M)
    c.sync_event("e")
    c.launch("dasr_add", S, [rd(X)])
    assert len(done(c)) == 1


# ---- rule 2: lifetime -------------------------------------------------------------------------------------------
def _handed_over(c, record=None, when="before"):
    st = c.lookup(X)
    c.launch("dasr_copy", M, [wr(X)])
    c.wait_stream(S, M)
    if record is not None and when == "before":
        c.record_stream(X, record)
    c.launch("dasr_add", S, [rd(X)], site="graph.py:2 (bwd)")
    return st


def test_lifetime_record_stream_passes():
    c = trace()
    c.free(_handed_over(c, S))
    assert done(c) == []


def test_lifetime_free_before_record_stream():
    c = trace()
    st = _handed_over(c)
    c.free(st, "graph.py:3 (bwd)")
    c.record_stream(X, S)                       # too late: the block is back in main's pool
    r = done(c)
    assert len(r) == 1 and r[0].startswith("LIFETIME storage 1024 B @0x10000 allocated on stream")
    assert "#1 dasr_add arg 0 'x' (read)" in r[0] and "graph.py:2 (bwd)" in r[0] and "free at graph.py:3 (bwd)" in r[0]


def test_lifetime_record_stream_on_the_wrong_stream():
    c = trace()
    c.free(_handed_over(c, M))
    assert len(done(c)) == 1
    c = trace()
    c.free(_handed_over(c, T))
    assert len(done(c)) == 1


def test_lifetime_free_made_safe_by_a_later_join():
    c = trace()
    st = _handed_over(c)
    c.record_event("used", S)
    c.wait_event("used", M)
    c.free(st)
    assert done(c) == []
    c = trace()                                 # an event of the side stream from BEFORE the use is no such join
    c.launch("dasr_copy", M, [wr(X)])
    c.wait_stream(S, M)
    c.record_event("early", S)
    c.launch("dasr_add", S, [rd(X)])
    c.wait_event("early", M)
    c.free(c.lookup(X))
    assert len(done(c)) == 1


def test_lifetime_same_stream_and_interior_pointer():
    c = trace()
    c.launch("dasr_copy", M, [wr(X)])
    c.launch("dasr_add", M, [rd(X)])
    c.free(c.lookup(X))
    assert done(c) == []
    c = trace()                                 # buf[128:] handed to the side stream: it is buf's storage that is freed
    assert c.resolve(X + 512) == (c.lookup(X), 512) and c.resolve(X + 1024) is None and c.resolve(X - 1) is None
    c.wait_stream(S, M)
    L = c.launch("dasr_copy", S, [wr(X + 512, "dst", 0, 256)])
    assert L.args[0].storage is c.lookup(X) and (L.args[0].lo, L.args[0].hi) == (512, 768)
    c.free_at(X + 512)
    r = done(c)
    assert len(r) == 1 and "storage 1024 B @0x10000" in r[0] and "arg 0 'dst' (write)" in r[0]


def test_lifetime_address_reused_by_a_new_storage():
    c = trace()
    st = _handed_over(c, S)
    c.free(st)
    new = c.alloc(X, 2048, S)                   # the allocator hands the address out again: a new storage, a clean record
    assert c.lookup(X) is new and new.foreign == {} and st.freed
    c.launch("dasr_copy", S, [wr(X)])
    c.free(new)
    assert done(c) == []


def _amax_pattern(record_amax):
    """graph.sean_mod's backward leaves d(gamma2|beta2) and its amax side-car on the main stream; the gamma_o|beta_o
    convolution's backward on the side stream records the gradient only."""
    DGB2, DMAX, DW, DX = 0xA0000, 0xB0000, 0xC0000, 0xD0000
    c = Checker()
    dgb2, dmax = c.alloc(DGB2, 1 << 20, M), c.alloc(DMAX, AMAX_BYTES, M)
    c.alloc(DW, 4096, S)
    c.alloc(DX, 1 << 20, S)
    c.launch("dasr_sean_bwd", M, [wr(DGB2, "dgb2", 15), wr(DMAX, "dgb2_amax", 23)])
    c.record_event("grad", M)
    c.wait_event("grad", S)
    c.record_stream(DGB2, S)
    if record_amax:
        c.record_stream(DMAX, S)
    c.launch("dasr_conv3x3_wgrad_split2", S, [rd(DGB2, "dconv", 2), rd(DMAX, "dmax", 3), wr(DW, "dw_hwio", 4)])
    c.launch("dasr_conv3x3_dgrad_split2", S, [rd(DGB2, "dconv", 0), rd(DMAX, "dmax", 1), wr(DX, "dx", 4)],
             site="graph.py:488 (bwd)")
    c.free(dgb2)
    c.free(dmax)                                # the tensor's attribute goes with it
    return done(c)


def test_amax_side_car_is_flagged():
    r = _amax_pattern(False)
    assert len(r) == 1 and r[0].startswith("LIFETIME storage %d B" % AMAX_BYTES)
    assert "dasr_conv3x3_dgrad_split2 arg 1 'dmax' (read)" in r[0] and "graph.py:488" in r[0]
    assert _amax_pattern(True) == []


def test_header_argument_names():
    """The report's argument names come from include/dasr.h and line up with _lib.declared_functions()'s types."""
    from tests.stream_audit import declared_arguments
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    names = declared_arguments(os.path.join(root, "include", "dasr.h"))
    assert names["dasr_conv3x3_dgrad_split2"][:5] == ["dconv", "dmax", "w_split", "wmax", "dx"]
    assert names["dasr_conv3x3_dgrad_split2"][-1] == "stream" and names["dasr_copy"] == ["dst", "src", "n", "stream"]
    assert names["dasr_conv3x3_split2_weights_slabs"] == ["Cin", "Cout"]


# ---- the MI355X: the real allocator, the product's step ------------------------------------------------------------
@pytest.fixture
def device_lib():
    from dasr_amd import _lib
    os.environ.pop("DASR_HIPEMU_LIB", None)
    _lib.reset_for_tests()


def _show(log):
    print("stream audit: %d launches on streams %s, %d unresolved pointers, %d reports"
          % (len(log.launches), ["0x%x" % s for s in log.streams()], log.unresolved, len(log.reports)))
    for line in log.reports:
        print(line)


def _planted(kind, repaired):
    """Two streams, 1 KiB tensors, ops.copy_ / ops.add only, events in the right places; ``repaired`` False leaves out
    exactly one record_stream or one wait.  Nothing is launched after the early free."""
    import torch
    from dasr_amd import ops
    from tests.stream_audit import audit
    from dasr_amd import graph
    main = torch.cuda.current_stream()
    side = graph._side_stream(torch.device("cuda", torch.cuda.current_device()))   # the product's own: no new stream
    src = torch.arange(256, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    with audit() as log:
        if kind == "free_main_to_side":          # allocated on main, read on the side stream, dropped
            a = ops.copy_(torch.empty(256, device="cuda"), src)
            ev = main.record_event()
            with torch.cuda.stream(side):
                side.wait_event(ev)
                if repaired:
                    a.record_stream(side)
                b = ops.add(a, a)
            del a
        elif kind == "free_side_to_main":        # allocated on the side stream, first seen by the library on main
            with torch.cuda.stream(side):
                a = torch.empty(256, device="cuda")
            main.wait_stream(side)
            if repaired:
                a.record_stream(main)
            b = ops.copy_(a, src)
            del a, b
        elif kind == "free_view":                # an interior view is all the side stream ever saw
            a = ops.copy_(torch.empty(256, device="cuda"), src)
            side.wait_stream(main)
            with torch.cuda.stream(side):
                if repaired:
                    a.record_stream(side)
                b = ops.add(a[128:], a[128:])
            del a
        elif kind == "order_missing_wait":       # the side stream reads what main wrote
            a = ops.copy_(torch.empty(256, device="cuda"), src)
            ev = main.record_event()
            with torch.cuda.stream(side):
                if repaired:
                    side.wait_event(ev)
                a.record_stream(side)
                b = ops.add(a, src)
        else:
            raise KeyError(kind)
    torch.cuda.synchronize()
    _show(log)
    assert log.launches and log.unresolved == 0
    return log


PLANTED = ("free_main_to_side", "free_side_to_main", "free_view", "order_missing_wait")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", PLANTED)
def test_planted_gpu(device_lib, kind):
    good = _planted(kind, True)
    assert good.reports == [], good.reports
    bad = _planted(kind, False)
    assert len(bad.reports) == 1, bad.reports
    assert bad.reports[0].startswith("ORDER" if kind.startswith("order") else "LIFETIME"), bad.reports
    assert "1024 B" in bad.reports[0]
    if kind == "free_side_to_main":              # the pool is the side stream's although main was current at first sight
        import torch
        main = torch.cuda.current_stream().cuda_stream
        assert "allocated on stream 0x%x" % main not in bad.reports[0], bad.reports


def _net(case):
    import torch
    from dasr_amd import synth
    from tests.parity_checks import build_net
    net, cfg = build_net(case, "cuda")
    lq, gt, dm, mk = [t.to("cuda") for t in synth.closed_form_batch(case.get("batch_idx", 2), case["B"], case["H"],
                                                                   case["W"], cfg["scale"])]
    return net, cfg, lq, gt, dm, mk


def _fresh(*tensors):
    """Inputs as a training loop passes them: tensors nobody else holds (``batch.to(device)``), which die during the step.
    The net reads its depth map and masks on the side stream; kept alive by the test they would hide that hand-over."""
    return [t.clone() for t in tensors]


def _train(net, lq, dm, mk, iterations=2, masks=None):
    """Forward + backward of a linear functional, ``iterations`` times, under the audit.  ``masks``: makes the step's mask
    tensor from its depth map (prepared masks carry their region bytes as an attribute a clone would lose)."""
    import torch
    from tests.stream_audit import audit
    shape = (lq.shape[0], 3, lq.shape[2] * net.scale, lq.shape[3] * net.scale)
    wgt = torch.cos(torch.arange(math.prod(shape), dtype=torch.float32) * 0.013).reshape(shape).to("cuda")
    torch.cuda.synchronize()
    with audit() as log:
        for _ in range(iterations):
            net.zero_grad(set_to_none=True)
            a, b, c = _fresh(lq, dm, mk if masks is None else dm)
            sr = net(a, b, c if masks is None else masks(b))
            del a, b, c
            (sr * wgt).sum().backward()
            del sr
    torch.cuda.synchronize()
    _show(log)
    return log


def _clean(log, two_streams=True):
    assert len(log.launches) > 100 and log.unresolved == 0
    if two_streams:
        assert len(log.streams()) == 2, log.streams()
    assert log.reports == [], "\n".join(log.reports)


SOFT_CASE = dict(scale=2, which=[0, 1, 2, 3], L=16, nb=4, B=1, H=8, W=12)


@pytest.mark.gpu
def test_step_soft_mask_net_gpu(device_lib):
    from dasr_amd import synth
    net, cfg, lq, gt, dm, mk = _net(SOFT_CASE)
    soft = (0.7 * mk + 0.3 * synth.hash_uniform(mk.numel(), "soft").reshape(mk.shape).float().to("cuda")).contiguous()
    _clean(_train(net, lq, dm, soft))


@pytest.mark.gpu
def test_step_onehot_net_gpu(device_lib):
    """Both mask sources of check_onehot_whole_net_unclaimed: planes with unclaimed pixels, and prepared masks that bring
    their region bytes."""
    import torch
    from dasr_amd import prep, synth
    from tests.onehot_sean_checks import WHOLE_NET_CASE
    net, cfg, lq, gt, dm, mk = _net(dict(WHOLE_NET_CASE, B=2, H=10, W=14))
    mk = mk.clone()
    mk[0, :, 2:8, 3:12] = 0
    mk[1] = 0
    _clean(_train(net, lq, dm, mk))
    depth = torch.empty(2, 1, 10, 14)
    depth[0] = 3.25
    depth[1] = (synth.hash_uniform(10 * 14, "onehot.depth") * 1.4 - 0.2).reshape(1, 10, 14).float()
    depth = depth.to("cuda")
    assert getattr(prep.depth_to_masks(depth, 10, fixed_range=True), "_dasr_region", None) is not None
    _clean(_train(net, lq, depth, None, masks=lambda d: prep.depth_to_masks(d, 10, fixed_range=True)))


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ("f32", "bf16"))
def test_step_x8_split_net_gpu(device_lib, monkeypatch, dtype):
    """The x8 net of conv9_dgrad_act_checks.check_net at 64 x 96 HR pixels with every split convolution forced on: in fp32
    the depth branch's gamma_o|beta_o convolution runs the fp16 x 2 kernels, whose backward on the side stream reads the
    amax side-car that SEAN's backward wrote on the main stream."""
    import torch
    from dasr_amd import graph
    from tests.conv9_dgrad_act_checks import NET_CASE
    monkeypatch.setattr(graph, "SPLIT_MIN_PIXELS", 0)
    assert graph.SPLIT_BF16 and graph.SPLIT_PIECES == 2 and graph.SIDE_STREAM
    net, cfg, lq, gt, dm, mk = _net(dict(NET_CASE, batch_idx=0))
    net.set_compute_dtype(dtype)
    log = _train(net, lq, dm, mk)
    if dtype == "f32":
        main = torch.cuda.current_stream().cuda_stream
        crossing = [L for L in log.launches if re.fullmatch(r"dasr_conv3x3_\w*dgrad\w*_split2", L.name) and L.stream != main
                    and any(a.name == "dmax" and a.writer is not None and a.writer.stream == main for a in L.args)]
        print("split dgrads on the side stream reading a main-stream dmax:", len(crossing))
        assert crossing, "no split dgrad on the side stream read an amax written on the main stream: nothing exercised"
    _clean(log)


@pytest.mark.gpu
def test_step_half_resolution_depth_gpu(device_lib):
    """check_constant_alpha_and_mask_resize's configuration: the resized masks are allocated on the side stream."""
    import torch
    from dasr_amd import synth
    from dasr_amd.depthnet import DepthNet
    net = DepthNet(which_ResBlk_depth=[0, 1], nb=4, scale=4, depth_latent_ch=16, use_trainable_params=False,
                   norm_gamma=0.3, norm_beta=0.6)
    synth.closed_form_fill_(net.state_dict().items())
    net = net.to("cuda")
    lq = synth.closed_form_batch(0, 2, 12, 16, 4)[0].to("cuda")
    _, _, dm, mk = [t.to("cuda") for t in synth.closed_form_batch(0, 2, 6, 8, 4)]
    log = _train(net, lq, dm, mk)
    assert any(L.name == "dasr_resize_nearest_nchw" and L.stream != torch.cuda.current_stream().cuda_stream
               for L in log.launches), "no mask was resized on the side stream"
    _clean(log)


@pytest.mark.gpu
def test_step_trainer_gpu(device_lib):
    """harness.Trainer, eager, one rank, default criteria, two optimisation steps on the soft-mask net."""
    import torch
    from dasr_amd import harness
    from tests.stream_audit import audit
    net, cfg, lq, gt, dm, mk = _net(SOFT_CASE)
    tr = harness.Trainer(net)
    torch.cuda.synchronize()
    with audit() as log:
        for _ in range(2):
            tr.optimize_parameters(*_fresh(lq, gt, dm, mk))
    torch.cuda.synchronize()
    _show(log)
    _clean(log)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("soft", "x8_split"))
def test_eval_forward_twice_gpu(device_lib, monkeypatch, which):
    """eval() + no_grad: the fold cache's buffers are first allocated (and filled) on the side stream."""
    import torch
    from dasr_amd import graph
    from tests.conv9_dgrad_act_checks import NET_CASE
    from tests.stream_audit import audit
    if which == "x8_split":
        monkeypatch.setattr(graph, "SPLIT_MIN_PIXELS", 0)
    net, cfg, lq, gt, dm, mk = _net(SOFT_CASE if which == "soft" else dict(NET_CASE, batch_idx=0))
    net.eval()
    torch.cuda.synchronize()
    with audit() as log, torch.no_grad():
        a = net(*_fresh(lq, dm, mk))
        b = net(*_fresh(lq, dm, mk))
    torch.cuda.synchronize()
    _show(log)
    assert torch.equal(a, b)
    _clean(log)
