"""The task-aligned anchor assignment, host side (no GPU needed): the margin condition of the committed case table, the
torch host path of ``roi.TaskAlignedAssigner`` against the fp64 reference of tests/tal_ref.py, the declaration / binding /
export and the host-side refusals of the new C-ABI symbols, the ``SODa`` keywords, and the CPU branch of ``SODa._loss`` -
what ``training_step`` runs behind the networks, which have no CPU path (the whole step is in tests/test_gpu_tal.py)."""
import ctypes
import os
import re

import pytest
import torch

import snn_for_object_detection_amd as S
from snn_for_object_detection_amd import soda
from snn_for_object_detection_amd.roi import TaskAlignedAssigner
from tests import tal_ref as T

CASES = T.tal_cases()
_REF = {}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ref_of(cs):
    """The reference of a case, computed once and shared (tests/test_gpu_tal.py uses it too)."""
    if cs.id not in _REF:
        _REF[cs.id] = T.tal_targets_ref(cs.anchors, cs.labels, cs.cls, cs.bb, cs.topk, cs.alpha, cs.beta)
    return _REF[cs.id]


def check_margins(cs, ref):
    for b, rec in enumerate(ref.records):
        ms, tiny = T.margins(rec)
        assert tiny == 0, (cs.id, b, "a top-k decision on a metric inside (0, 1e-30)")
        if cs.duplication:      # the ties that are there on purpose are exact; everything else keeps the margin
            assert all(m == 0.0 or m > T.MARGIN for m in ms), (cs.id, b, sorted(ms)[:3])
            assert any(m == 0.0 for m in ms), (cs.id, b)
        else:
            assert all(m > T.MARGIN for m in ms), (cs.id, b, sorted(ms)[:3])


def test_the_case_table_covers_the_stated_ranges():
    shapes = [(c.anchors.shape[0], c.labels.shape[1], c.cls.shape[2], c.labels.shape[0], c.topk) for c in CASES]
    assert all(100 <= a <= 200 and a % 64 != 0 for a, *_ in shapes)
    assert {n for _, n, *_ in shapes} >= {1, 2, 3, 5, 8} and max(n for _, n, *_ in shapes) == 8
    assert {c for _, _, c, _, _ in shapes} == {2, 3, 4, 5}
    assert {b for *_, b, _ in shapes} == {1, 2, 3}
    assert {k for *_, k in shapes} == {1, 3, 10}
    assert sum(c.duplication for c in CASES) == 2
    assert sum(c.check is not None for c in CASES) == 7


@pytest.mark.parametrize("cs", CASES, ids=[c.id for c in CASES])
def test_every_decision_of_the_table_keeps_its_margin(cs):
    """A condition on the INPUTS: outside the duplication cases every top-k, conflict and fall-back decision of the fp64
    reference has a relative margin above 1e-4 - orders of magnitude above the fp32 rounding of s^alpha u^beta - and the
    edge a case is there for is reached by the reference."""
    ref = ref_of(cs)
    if cs.check is not None:
        cs.check(ref.records)
    check_margins(cs, ref)


def test_the_large_case_keeps_its_margin():
    cs = T.gen1_case()
    assert cs.anchors.shape[0] == 13_545 and cs.labels.shape[1] == 16
    ref = ref_of(cs)
    check_margins(cs, ref)
    assert sum(len(r.conflict) for r in ref.records) > 0 and int((ref.rows >= 0).sum()) > 100


def test_the_case_behind_the_metric_cache_keeps_its_margin():
    cs = T.beyond_cache_case()
    assert cs.anchors.shape[0] == 15_000 > T.CACHE and cs.topk == 3
    kernels = open(os.path.join(ROOT, "snn_for_object_detection_amd", "csrc", "targets.hip")).read()
    assert f"constexpr int kTalCache = {T.CACHE};" in kernels          # the boundary the case is built around
    ref = ref_of(cs)
    cs.check(ref.records)
    check_margins(cs, ref)


@pytest.mark.parametrize("cs", CASES, ids=[c.id for c in CASES])
def test_host_path_against_the_reference(cs):
    """The integer assignment is the reference's; classes and masks follow from it; the offsets hold the bounds
    tests/test_gpu_targets_fp64.py sets for snn_roi_assign's against the fp64 offsets of that assignment."""
    ref = ref_of(cs)
    tal = TaskAlignedAssigner(cs.topk, cs.alpha, cs.beta)
    off, mask, cls, rows = tal(cs.anchors, cs.labels, cs.cls, cs.bb, return_rows=True)
    assert rows.dtype == torch.int64 and torch.equal(rows, ref.rows)
    assert cls.dtype == torch.int64 and torch.equal(cls, ref.classes)
    assert mask.dtype == torch.float32 and torch.equal(mask, ref.masks)
    assert off.dtype == torch.float32 and tuple(off.shape) == tuple(mask.shape) == tuple(cs.labels.shape[:1]) + (cs.anchors.shape[0], 4)
    xy, wh = T.check_offsets(off, ref)
    print(f"{cs.id}: offsets vs fp64 {xy:.3g} / {wh:.3g} of their bounds")
    three = tal(cs.anchors, cs.labels, cs.cls, cs.bb)
    assert len(three) == 3 and torch.equal(three[2], cls)


def test_predictions_are_read_as_constants_and_options_are_checked():
    cs = CASES[1]
    cls, bb = cs.cls.clone().requires_grad_(), cs.bb.clone().requires_grad_()
    out = TaskAlignedAssigner(cs.topk)(cs.anchors, cs.labels, cls, bb)
    assert not any(t.requires_grad for t in out)
    for kw in (dict(topk=0), dict(topk=65), dict(alpha=-1.0), dict(beta=float("nan")), dict(alpha=float("inf"))):
        with pytest.raises(ValueError, match=next(iter(kw))):
            TaskAlignedAssigner(**kw)
    with pytest.raises(RuntimeError, match="device tensors only"):
        TaskAlignedAssigner().steps(cs.anchors, torch.zeros(1, 2, 6), torch.zeros(1, 1, dtype=torch.int32), 0, cls, bb)


# ------------------------------------------------------------------------------------------------------ C ABI
P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
NEW = {
    "snn_tal_workspace_size": (ctypes.c_size_t, [I, I, I, I]),
    "snn_tal_assign": (ctypes.c_int, [P] * 5 + [I] * 7 + [F, F] + [P] * 6),
}


def test_new_symbols_are_declared_exported_and_bound(hip_lib):
    from snn_for_object_detection_amd import _build, _hip
    header = open(os.path.join(ROOT, "include", "snn_hip.h")).read()
    assert "#define SNN_ABI_VERSION 20" in header and _hip.ABI_VERSION == 20 and hip_lib.snn_abi_version() == 20
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    declared = set(re.findall(r"\b(snn_[a-z0-9_]+)\s*\(", code))
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name, sig in NEW.items():
        assert name in declared and hasattr(raw, name), name
        assert _hip.SIGNATURES[name] == sig, name
    assert "targets.hip" in _build.SOURCES
    # the entry points the static assigner goes through keep their prototypes
    assert len(_hip.SIGNATURES["snn_roi_assign"][1]) == 11 and len(_hip.SIGNATURES["snn_roi_assign_steps"][1]) == 14
    per_slot = 100 * (16 + 8 + 4) + 7 * 10 * 4
    assert hip_lib.snn_tal_workspace_size(6, 100, 7, 10) == 6 * per_slot
    assert hip_lib.snn_tal_workspace_size(0, 100, 7, 10) == 0


def test_refusals_come_before_any_launch(hip_lib):
    """Every refusal with host addresses that are never dereferenced (a launch would fault on them): null pointers, topk,
    C, alpha / beta, A * N, alignment, K.  tests/test_gpu_tal.py repeats them on device buffers and reads those back."""
    host = (ctypes.c_float * 64)()
    a = (ctypes.addressof(host) + 15) & ~15
    name = "snn_tal_assign"

    def call(K=1, B=1, A=8, N=2, C=3, t0=0, topk=10, alpha=1.0, beta=6.0, **ptr):
        p = {k: ptr.get(k, None if k in ("steps", "rows") else a)
             for k in ("anchors", "labels", "steps", "cls", "bb", "ws", "off", "mask", "out_cls", "rows")}
        return hip_lib.snn_tal_assign(p["anchors"], p["labels"], p["steps"], p["cls"], p["bb"], K, B, A, N, C, t0, topk,
                                      alpha, beta, p["ws"], p["off"], p["mask"], p["out_cls"], p["rows"], None)

    def refused(rc, *words):
        msg = hip_lib.snn_last_error().decode()
        assert rc != 0 and msg.startswith(name + ":"), (rc, msg)
        for w in words:
            assert w in msg, (w, msg)

    for arg in ("anchors", "labels", "cls", "bb", "ws", "off", "mask", "out_cls"):
        refused(call(**{arg: None}), "null pointer")
    for topk in (0, -1, 65):
        refused(call(topk=topk), "topk")
    for C in (1, 0, 65):
        refused(call(C=C), "C must be")
    for kw in (dict(alpha=-0.5), dict(beta=-1.0), dict(alpha=float("nan")), dict(beta=float("inf")),
               dict(alpha=float("inf"))):
        refused(call(**kw), "alpha and beta")
    refused(call(A=1 << 16, N=1 << 15), "bad shape")             # A * N = 2^31
    refused(call(A=(1 << 31) - 1024, N=1), "bad shape")          # at the limit
    for kw in (dict(B=0), dict(A=0), dict(N=0), dict(t0=-1)):
        refused(call(**kw), "bad shape")
    for arg in ("anchors", "bb", "off", "mask", "ws"):
        refused(call(**{arg: a + 4}), "16-byte aligned")
    refused(call(K=2), "K must be")                               # five-column labels: one slot per sample
    refused(call(K=0, steps=a), "K must be")
    refused(call(K=33, steps=a), "K must be")


# ------------------------------------------------------------------------------------------------------ SODa
def _model(**kw):
    return S.TinyYolo(num_classes=2, time_window=0, **kw)


def test_constructor_validates_the_assigner_options_by_name():
    for kw in (dict(assigner="atss"), dict(assigner="TAL"), dict(assigner=None)):
        with pytest.raises(ValueError, match="assigner"):
            _model(**kw)
    for topk in (0, 65, 2.5, True):
        with pytest.raises(ValueError, match="tal_topk"):
            _model(assigner="tal", tal_topk=topk)
    for v in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tal_alpha"):
            _model(assigner="tal", tal_alpha=v)
        with pytest.raises(ValueError, match="tal_beta"):
            _model(assigner="tal", tal_beta=v)
    m = _model(assigner="tal", tal_topk=5, tal_alpha=0.5, tal_beta=4.0)
    hp = m.hparams
    assert (hp.assigner, hp.tal_topk, hp.tal_alpha, hp.tal_beta) == ("tal", 5, 0.5, 4.0)
    assert (m.tal_blk.topk, m.tal_blk.alpha, m.tal_blk.beta) == (5, 0.5, 4.0)
    d = _model()
    assert (d.hparams.assigner, d.hparams.tal_topk, d.hparams.tal_alpha, d.hparams.tal_beta) == ("iou", 10, 1.0, 6.0)
    assert d.tal_blk is None and soda.ASSIGNER_NAMES == ("iou", "tal")
    assert list(m.state_dict().keys()) == list(d.state_dict().keys())            # no parameter or buffer is added


def _preds_and_labels(seed=5, B=2, C=3):
    g = torch.Generator().manual_seed(seed)
    anchors = T.make_anchors()
    cls, bb = T.predictions(B, anchors.shape[0], C, g)
    labels = torch.stack([T.random_labels(3, C, g) for _ in range(B)])
    labels[1, 2] = -1.0
    return (anchors, cls, bb), labels


def test_default_and_iou_give_bit_equal_losses_from_the_same_seed():
    """``SODa()`` and ``SODa(assigner="iou")``: the same parameters from the same seed, and the same loss bits - under
    the default objective and under a selected one."""
    preds, labels = _preds_and_labels()
    for opts in ({}, dict(cls_loss="focal", box_loss="giou")):
        torch.manual_seed(4)
        a = _model(**opts)
        torch.manual_seed(4)
        b = _model(assigner="iou", **opts)
        for (ka, va), (kb, vb) in zip(a.state_dict().items(), b.state_dict().items()):
            assert ka == kb and torch.equal(va, vb), ka
        la, lb = a._loss(preds, labels), b._loss(preds, labels)
        assert torch.equal(la.reshape(1).view(torch.int32), lb.reshape(1).view(torch.int32))


@pytest.mark.parametrize("opts", [{}, dict(cls_loss="focal", box_loss="ciou", box_loss_weight=2.0)],
                         ids=["ce_l1", "focal_ciou"])
def test_cpu_loss_is_the_host_assigner_composed_with_the_existing_loss(opts):
    """``SODa(assigner="tal")._loss`` on CPU tensors: finite, the bits of the existing host loss applied to the targets of
    ``TaskAlignedAssigner`` on the same (detached) predictions, different from the static rule's loss, and the gradient
    reaches the predictions only through the loss."""
    (anchors, cls, bb), labels = _preds_and_labels()
    cls, bb = cls.clone().requires_grad_(), bb.clone().requires_grad_()
    m = _model(assigner="tal", tal_topk=3, **opts)
    loss = m._loss((anchors, cls, bb), labels)
    assert bool(torch.isfinite(loss))
    off, mask, lab = TaskAlignedAssigner(3)(anchors, labels, cls, bb)
    assert int((lab > 0).sum()) >= 9
    plain = _model(**opts)
    if opts:
        t_cls, t_box = soda.detection_loss_host(cls, bb, off, mask, lab, anchors, plain.hparams.loss_ratio, **opts)
        want = t_cls + t_box
    else:
        ce = torch.nn.CrossEntropyLoss(reduction="none")(cls.reshape(-1, 3), lab.reshape(-1))
        l1 = torch.nn.L1Loss(reduction="none")(bb * mask, off * mask)
        pos = lab.reshape(-1) > 0
        want = ce[pos].mean() * plain.hparams.loss_ratio + ce[~pos].mean() * (1 - plain.hparams.loss_ratio) + l1.mean()
    assert torch.equal(loss.detach().reshape(1).view(torch.int32), want.detach().reshape(1).view(torch.int32))
    assert float(plain._loss((anchors, cls, bb), labels).detach()) != float(loss.detach())
    loss.backward()
    assert bool(torch.isfinite(cls.grad).all()) and bool(cls.grad.any()) and bool(bb.grad.any())


class _ModelBuilt(Exception):
    pass


@pytest.mark.parametrize("tool,argv", [("train_demo.py", ["2"]), ("train_on_recordings.py", ["--data-dir", "nowhere"])])
def test_training_tools_hand_the_assigner_to_the_model(tool, argv, monkeypatch):
    """The tools run as ``__main__`` with the model constructor replaced by a recorder that stops the run: ``--assigner``
    is parsed, reaches ``TinyYolo`` as the keyword ``assigner``, defaults to ``"iou"``, and refuses another name."""
    import runpy
    import sys
    built = []

    def record(**kw):
        built.append(kw)
        raise _ModelBuilt

    class Feed:
        def __init__(self, *a, **k):
            pass

        def get_labels(self):
            return ["car", "pedestrian"]

    monkeypatch.setattr(S, "TinyYolo", record)
    monkeypatch.setattr(S, "PropheseeFeed", Feed)
    path = os.path.join(ROOT, "tools", tool)
    for extra, want in ((["--assigner", "tal"], "tal"), ([], "iou")):
        monkeypatch.setattr(sys, "argv", [path] + argv + extra)
        with pytest.raises(_ModelBuilt):
            runpy.run_path(path, run_name="__main__")
        assert built[-1]["assigner"] == want
    monkeypatch.setattr(sys, "argv", [path] + argv + ["--assigner", "atss"])
    with pytest.raises(SystemExit):
        runpy.run_path(path, run_name="__main__")
    assert len(built) == 2
