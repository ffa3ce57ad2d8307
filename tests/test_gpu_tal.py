"""The task-aligned anchor assignment on the device: ``snn_tal_assign`` (csrc/targets.hip) through the C ABI on guarded
buffers against the fp64 reference of tests/tal_ref.py on every case of its table, ``roi.TaskAlignedAssigner`` on device
tensors (the same bits), the six-column / steps form slot by slot, batch independence, the GEN1 anchor count, the
refusals, and ``SODa(assigner="tal")`` - without host synchronisation, and against the host assigner composed with the
existing loss.

The integer results (``assigned_row``, classes, masks) must be the reference's exactly: the case table keeps every
decision's margin above 1e-4 relative (tests/test_tal_host.py asserts that on the inputs).  The offsets hold the bounds of
tests/test_gpu_targets_fp64.py::check_roi against the fp64 offsets of the assignment."""
import pytest
import torch

from tests import tal_ref as T
from tests.test_gpu_targets_fp64 import GUARD
from tests.test_gpu_targets_fp64 import Guarded as _Guarded
from tests.test_tal_host import CASES, ref_of

pytestmark = pytest.mark.gpu


class Guarded(_Guarded):
    """The guarded buffer of tests/test_gpu_targets_fp64.py, with int32 (0x7F bytes) next to its dtypes."""

    def __init__(self, n, dtype):
        if dtype != torch.int32:
            super().__init__(n, dtype)
            return
        self.n = n
        self.buf = torch.full((n + GUARD,), 0x7F7F7F7F, dtype=dtype, device="cuda")
        self.fill_bytes = self.buf[n:].clone().view(torch.uint8)
        self.ptr = self.buf.data_ptr()


@pytest.fixture(scope="module")
def hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from snn_for_object_detection_amd import _hip
    return _hip


def _st():
    return torch.cuda.current_stream().cuda_stream


def run_tal_abi(hip, anchors, labels, cls, bb, topk, alpha=1.0, beta=6.0, steps=None, t0=0, with_rows=True):
    """snn_tal_assign through the C ABI on guarded buffers -> (offset, mask, cls, rows) on the host, leading shape [S]."""
    anchors, labels, cls, bb = (t.cuda().contiguous() for t in (anchors, labels, cls, bb))
    B, N, _ = labels.shape
    A, C = anchors.shape[0], cls.shape[-1]
    K = 1 if steps is None else steps.shape[0]
    S = K * B
    if steps is not None:
        steps = steps.cuda().contiguous()
    ws = Guarded(hip.query("snn_tal_workspace_size", S, A, N, topk), torch.uint8)
    off, mask = Guarded(S * A * 4, torch.float32), Guarded(S * A * 4, torch.float32)
    out_cls, rows = Guarded(S * A, torch.int64), Guarded(S * A, torch.int32)
    hip.call("snn_tal_assign", anchors.data_ptr(), labels.data_ptr(), None if steps is None else steps.data_ptr(),
             cls.data_ptr(), bb.data_ptr(), K, B, A, N, C, t0, topk, alpha, beta, ws.ptr, off.ptr, mask.ptr, out_cls.ptr,
             rows.ptr if with_rows else None, _st())
    torch.cuda.synchronize()
    for name, g in (("workspace", ws), ("offset", off), ("mask", mask), ("class", out_cls), ("rows", rows)):
        assert g.guard_intact(), f"the guard behind the {name} buffer changed"
    if not with_rows:
        assert rows.untouched()
    return off.out(S, A, 4), mask.out(S, A, 4), out_cls.out(S, A), rows.out(S, A)


def check_against(ref, off, mask, cls, rows):
    assert rows.dtype == torch.int32 and torch.equal(rows.long(), ref.rows)
    assert cls.dtype == torch.int64 and torch.equal(cls, ref.classes)
    assert torch.equal(mask, ref.masks)
    return T.check_offsets(off, ref)


@pytest.mark.parametrize("cs", CASES, ids=[c.id for c in CASES])
def test_tal_assign_against_the_reference(hip, cs):
    from snn_for_object_detection_amd.roi import TaskAlignedAssigner
    ref = ref_of(cs)
    if cs.check is not None:
        cs.check(ref.records)                            # the edge the case is there for is reached by the reference
    off, mask, cls, rows = run_tal_abi(hip, cs.anchors, cs.labels, cs.cls, cs.bb, cs.topk, cs.alpha, cs.beta)
    xy, wh = check_against(ref, off, mask, cls, rows)
    print(f"{cs.id}: offsets vs fp64 {xy:.3g} / {wh:.3g} of their bounds")
    # ---- the same through roi.TaskAlignedAssigner: the same bits; assigned_row is optional
    tal = TaskAlignedAssigner(cs.topk, cs.alpha, cs.beta)
    o2, m2, c2, r2 = tal(cs.anchors.cuda(), cs.labels.cuda(), cs.cls.cuda(), cs.bb.cuda(), return_rows=True)
    assert c2.dtype == torch.int64 and torch.equal(c2.cpu(), cls) and torch.equal(m2.cpu(), mask)
    assert r2.dtype == torch.int32 and torch.equal(r2.cpu(), rows)
    assert torch.equal(o2.cpu().view(torch.int32), off.view(torch.int32))
    o3, m3, c3, _ = run_tal_abi(hip, cs.anchors, cs.labels, cs.cls, cs.bb, cs.topk, cs.alpha, cs.beta, with_rows=False)
    assert torch.equal(c3, cls) and torch.equal(m3, mask) and torch.equal(o3.view(torch.int32), off.view(torch.int32))


def test_other_exponents(hip):
    """alpha = 0.5, beta = 2 and alpha = 0 (the probability drops out: 0^0 = 1) on the conflict case, whose margins are
    asserted here for these exponents as the table's are for its own."""
    cs = next(c for c in CASES if c.id == "conflict")
    for alpha, beta in ((0.5, 2.0), (0.0, 6.0)):
        ref = T.tal_targets_ref(cs.anchors, cs.labels, cs.cls, cs.bb, cs.topk, alpha, beta)
        ms, tiny = T.margins(ref.records[0])
        assert tiny == 0 and all(m > T.MARGIN for m in ms), (alpha, beta, sorted(ms)[:3])
        check_against(ref, *run_tal_abi(hip, cs.anchors, cs.labels, cs.cls, cs.bb, cs.topk, alpha, beta))


@pytest.mark.parametrize("K,case_id", [(1, "rand_N8_C4_B2_k10"), (3, "rand_N5_C3_B3_k3")])
def test_steps_form_slot_by_slot(hip, K, case_id):
    """Six-column labels with rows of K + 1 timesteps (one of them in no slot) and an empty slot: every slot equals the
    five-column call on that slot's rows and predictions bit for bit, the empty slot is exact zeros with rows -1; and
    ``TaskAlignedAssigner.steps`` returns the same bits."""
    from snn_for_object_detection_amd.roi import TaskAlignedAssigner
    cs = next(c for c in CASES if c.id == case_id)
    t0 = 2
    labels6, steps, slot_rows = T.steps_labels(cs, K, t0, seed=7)
    B, N, _ = cs.labels.shape
    A, C = cs.anchors.shape[0], cs.cls.shape[2]
    assert bool((labels6[:, :, 0] == 9 + t0 if K == 3 else labels6[:, :, 0] == 5 + t0).any())      # rows of no slot
    g = torch.Generator().manual_seed(70 + K)
    cls, bb = T.predictions(K * B, A, C, g)
    cls, bb = cls.reshape(K, B, A, C), bb.reshape(K, B, A, 4)
    off, mask, out_cls, rows = run_tal_abi(hip, cs.anchors, labels6, cls, bb, cs.topk, steps=steps, t0=t0)
    positives = 0
    for k in range(K):
        for b in range(B):
            s = k * B + b
            if int(steps[k, b]) < 0:
                assert not bool(off[s].any()) and not bool(mask[s].any()) and not bool(out_cls[s].any())
                assert bool((rows[s] == -1).all())
                continue
            o1, m1, c1, r1 = run_tal_abi(hip, cs.anchors, slot_rows[k, b][None], cls[k, b][None], bb[k, b][None], cs.topk)
            assert torch.equal(r1[0], rows[s]) and torch.equal(c1[0], out_cls[s]) and torch.equal(m1[0], mask[s]), (k, b)
            assert torch.equal(o1[0].view(torch.int32), off[s].view(torch.int32)), (k, b)
            positives += int((rows[s] >= 0).sum())
    assert positives > 0 and int(steps[K - 1, 0]) == -1
    o2, m2, c2, r2 = TaskAlignedAssigner(cs.topk).steps(cs.anchors.cuda(), labels6.cuda(), steps.cuda(), t0, cls.cuda(),
                                                        bb.cuda(), return_rows=True)
    assert tuple(o2.shape) == (K, B, A, 4) and tuple(c2.shape) == (K, B, A) and c2.dtype == torch.int64
    assert torch.equal(c2.cpu().reshape(K * B, A), out_cls) and torch.equal(r2.cpu().reshape(K * B, A), rows)
    assert torch.equal(m2.cpu().reshape(K * B, A, 4), mask)
    assert torch.equal(o2.cpu().reshape(K * B, A, 4).view(torch.int32), off.view(torch.int32))


def test_a_sample_is_independent_of_its_batch(hip):
    cs = next(c for c in CASES if c.id == "rand_N5_C3_B3_k3")
    off, mask, cls, rows = run_tal_abi(hip, cs.anchors, cs.labels, cs.cls, cs.bb, cs.topk)
    for b in range(3):
        o1, m1, c1, r1 = run_tal_abi(hip, cs.anchors, cs.labels[b:b + 1], cs.cls[b:b + 1], cs.bb[b:b + 1], cs.topk)
        assert torch.equal(r1[0], rows[b]) and torch.equal(c1[0], cls[b]) and torch.equal(m1[0], mask[b]), b
        assert torch.equal(o1[0].view(torch.int32), off[b].view(torch.int32)), b


def test_the_gen1_anchor_count(hip):
    """A = 13 545, N = 16, B = 2: every grid-stride loop takes several passes.  The same condition: exact integers."""
    cs = T.gen1_case()
    ref = ref_of(cs)
    xy, wh = check_against(ref, *run_tal_abi(hip, cs.anchors, cs.labels, cs.cls, cs.bb, cs.topk))
    print(f"{cs.id}: {int((ref.rows >= 0).sum())} positives, offsets vs fp64 {xy:.3g} / {wh:.3g} of their bounds")


def test_anchors_behind_the_metric_cache(hip):
    """A = 15 000 > the 14 336 metrics k_tal_select keeps in LDS: the rounds after the first recompute the anchors behind
    the cache.  The reference selects anchors on both sides of the boundary (asserted), the margins hold (asserted
    here, as tests/test_tal_host.py asserts the table's), and the integers are exact."""
    from tests.test_tal_host import check_margins
    cs = T.beyond_cache_case()
    ref = ref_of(cs)
    cs.check(ref.records)
    check_margins(cs, ref)
    check_against(ref, *run_tal_abi(hip, cs.anchors, cs.labels, cs.cls, cs.bb, cs.topk))


def test_refusals_leave_the_outputs_untouched(hip):
    A, N, C = 8, 2, 3
    cs = CASES[1]
    anchors = torch.cat([cs.anchors[:A], cs.anchors[:1]]).cuda()
    labels = cs.labels[:, :N].cuda().contiguous()
    cls = cs.cls[:, :A].cuda().contiguous()
    bb = torch.cat([cs.bb[0, :A], cs.bb[0, :1]]).cuda()
    steps = torch.zeros(1, 1, dtype=torch.int32, device="cuda")
    ws = Guarded(hip.query("snn_tal_workspace_size", 1, A, N, 10) + 16, torch.uint8)
    off, mask = Guarded(A * 4 + 4, torch.float32), Guarded(A * 4 + 4, torch.float32)
    out_cls, rows = Guarded(A, torch.int64), Guarded(A, torch.int32)
    good = [anchors.data_ptr(), labels.data_ptr(), None, cls.data_ptr(), bb.data_ptr(), 1, 1, A, N, C, 0, 10, 1.0, 6.0,
            ws.ptr, off.ptr, mask.ptr, out_cls.ptr, rows.ptr, _st()]

    def refused(**kw):
        args = list(good)
        for k, v in kw.items():
            args[int(k[1:])] = v
        with pytest.raises(RuntimeError, match="snn_tal_assign"):
            hip.call("snn_tal_assign", *args)

    for i in (0, 1, 3, 4, 14, 15, 16, 17):
        refused(**{f"a{i}": None})                                   # null pointers
    for topk in (0, 65):
        refused(a11=topk)
    for c in (1, 65):
        refused(a9=c)
    for v in (-1.0, float("nan"), float("inf")):
        refused(a12=v)
        refused(a13=v)
    refused(a7=1 << 16, a8=1 << 15)                                  # A * N = 2^31
    refused(a7=(1 << 31) - 1024, a8=1)
    for i, p in ((0, anchors.data_ptr()), (4, bb.data_ptr()), (14, ws.ptr), (15, off.ptr), (16, mask.ptr)):
        refused(**{f"a{i}": p + 4})                                  # boxes are read and written as float4
    refused(a5=2)
    refused(a2=steps.data_ptr(), a5=33)
    torch.cuda.synchronize()
    assert ws.untouched() and off.untouched() and mask.untouched() and out_cls.untouched() and rows.untouched()
    hip.call("snn_tal_assign", *good)                                # the same arguments unchanged are accepted
    torch.cuda.synchronize()
    assert not rows.untouched() and rows.guard_intact()


# ====================================================================================================== model level
T_, B_, H_, W_ = 4, 2, 32, 48


def _batch(label_steps):
    from tests.util import synthetic_events, synthetic_labels
    X = synthetic_events(T_, B_, H_, W_, p=0.08).cuda()
    labels = synthetic_labels(B_, n_boxes=2, seed=1)
    if label_steps:
        six = torch.full((B_, 3, 6), -1.0)
        six[:, :2, 1:] = labels
        six[0, 0, 0], six[0, 1, 0], six[1, 0, 0], six[1, 1, 0] = 1.0, 3.0, 3.0, 3.0       # sample 1: one empty slot
        labels = six
    return X, labels.cuda()


def test_training_step_does_not_synchronise(hip):
    """``SODa(assigner="tal").training_step`` with five-column labels and with ``label_steps=2`` under
    ``set_sync_debug_mode("error")``: the assignment reads the predictions on the device and nothing comes back."""
    import snn_for_object_detection_amd as S
    from tests.test_gpu_det_loss_ext import _tiny_net
    Net = _tiny_net(S)
    runs = []
    for label_steps in (None, 2):
        torch.manual_seed(2)
        model = Net(num_classes=2, time_window=0, label_steps=label_steps, assigner="tal", tal_topk=3).cuda().train()
        batch = _batch(label_steps)
        model.training_step(batch).backward()      # the first step: library, workspaces, autotuned plans
        runs.append((model, batch))
    torch.cuda.synchronize()
    probe = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.sum().item()                       # the mode is live: a host read of a device value raises
        losses = [model.training_step(batch) for model, batch in runs]
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert all(bool(torch.isfinite(loss)) for loss in losses)


def test_training_step_against_the_host_assigner(hip, monkeypatch):
    """A tiny generated SODa with ``assigner="tal"`` under focal + CIoU: the loss is finite, gradients reach the head and
    the first layer, and the loss equals the existing host loss (``soda.detection_loss_host``) applied to the targets of
    the HOST assigner on the same predictions - at the tolerance of
    tests/test_gpu_det_loss_ext.py::test_training_step_with_a_selected_objective.  The device targets are the host
    assigner's: classes and masks exactly."""
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd import functional as HF
    from snn_for_object_detection_amd import soda
    from snn_for_object_detection_amd.roi import TaskAlignedAssigner
    from tests.test_gpu_det_loss_ext import GAMMA, WEIGHT, YARD_LOSS, _spy, _tiny_net
    calls = []
    for name in ("detection_loss", "detection_loss_ext"):
        _spy(monkeypatch, HF, name, calls)
    opts = dict(cls_loss="focal", focal_gamma=GAMMA, box_loss="ciou", box_loss_weight=WEIGHT)
    X, labels = _batch(None)
    torch.manual_seed(2)
    model = _tiny_net(S)(num_classes=2, time_window=0, assigner="tal", tal_topk=3, **opts).cuda().train()
    loss = model.training_step((X, labels))
    loss.backward()
    assert [c[0] for c in calls] == ["detection_loss_ext"]
    cls_preds, bbox_preds, off, mask, lab, anchors, ratio = [t.detach().cpu() if isinstance(t, torch.Tensor) else t
                                                             for t in calls[0][1][:7]]
    h_off, h_mask, h_lab = TaskAlignedAssigner(3)(anchors, labels.cpu(), cls_preds, bbox_preds)
    assert int((h_lab > 0).sum()) >= 4
    assert torch.equal(lab, h_lab) and torch.equal(mask, h_mask)
    t_cls, t_box = soda.detection_loss_host(cls_preds, bbox_preds, h_off, h_mask, h_lab, anchors, ratio, **opts)
    cpu, dev = float(t_cls + t_box), float(loss.detach())
    print(f"device {dev!r} host assigner + host loss {cpu!r}")
    assert bool(torch.isfinite(loss)) and dev > 0
    assert abs(dev - cpu) <= 5 * YARD_LOSS[("focal", "ciou")] * abs(cpu)
    weights = {n: p.grad for n, p in model.head_net.named_parameters() if p.dim() == 4}      # the convolutions' weights
    bad = [n for n, g in weights.items() if g is None or not bool(torch.isfinite(g).all()) or not bool(g.any())]
    assert weights and not bad, (bad, sorted(weights))
    g0 = next(model.base_net.parameters()).grad
    assert g0 is not None and bool(torch.isfinite(g0).all()) and bool(g0.any())
    # ---- the default assigner goes through the static rule, with the targets of RoI alone
    del calls[:]
    torch.manual_seed(2)
    plain = _tiny_net(S)(num_classes=2, time_window=0, **opts).cuda().train()
    assert plain.tal_blk is None
    plain.training_step((X, labels))
    r_off, r_mask, r_lab = plain.roi_blk(calls[0][1][5], labels)
    assert torch.equal(calls[0][1][4], r_lab) and torch.equal(calls[0][1][3], r_mask)
