"""The selectable detection loss, host side: constructor validation, the defaults (which must leave the reference's
objective exactly as it was), the CPU branch of ``SODa._loss`` for every (cls, box) combination against the fp64
restatement of tests/det_loss_ext_ref.py, the yardstick constants of tests/test_gpu_det_loss_ext.py, and the declaration /
binding of the new C-ABI symbols."""
import os
import re

import pytest
import torch

import snn_for_object_detection_amd as S
from snn_for_object_detection_amd import soda
from tests import det_loss_ext_ref as R
from tests import test_gpu_det_loss_ext as G

NEW_SYMBOLS = {"snn_det_loss_ext_workspace_size": 1, "snn_det_loss_ext_fwd": 19, "snn_det_loss_ext_bwd": 20}
RATIO, GAMMA, WEIGHT = G.RATIO, G.GAMMA, G.WEIGHT


def _model(**kw):
    return S.TinyYolo(num_classes=2, time_window=0, **kw)


def _preds_and_labels(seed=3, A=120, B=2):
    """Predictions of the shapes ``SODa._loss`` takes and five-column labels that assign some anchors."""
    g = torch.Generator().manual_seed(seed)
    inp = R.ext_inputs(B, A, 3, "random", seed)
    labels = torch.full((B, 3, 5), -1.0)
    for b in range(B):
        for j in range(2):
            a = inp.anchors[int(torch.randint(0, A, (1,), generator=g))]
            labels[b, j, 0] = float(torch.randint(0, 2, (1,), generator=g))
            labels[b, j, 1:] = a + 0.01 * torch.randn(4, generator=g).abs() * torch.tensor([-1.0, -1.0, 1.0, 1.0])
    return (inp.anchors, inp.logits, inp.bbox), labels


def test_constructor_validates_the_loss_options_by_name():
    for kw in (dict(cls_loss="bce"), dict(cls_loss="Focal"), dict(cls_loss=None)):
        with pytest.raises(ValueError, match="cls_loss"):
            _model(**kw)
    for kw in (dict(box_loss="iou"), dict(box_loss="L1"), dict(box_loss=1)):
        with pytest.raises(ValueError, match="box_loss"):
            _model(**kw)
    for gamma in (-0.5, float("nan")):
        with pytest.raises(ValueError, match="focal_gamma"):
            _model(cls_loss="focal", focal_gamma=gamma)
    with pytest.raises(ValueError, match="box_loss_weight"):
        _model(box_loss="giou", box_loss_weight=-1.0)
    m = _model(cls_loss="focal", focal_gamma=1.5, box_loss="ciou", box_loss_weight=2.0)
    hp = m.hparams
    assert (hp.cls_loss, hp.focal_gamma, hp.box_loss, hp.box_loss_weight) == ("focal", 1.5, "ciou", 2.0)
    assert list(m.state_dict().keys()) == list(_model().state_dict().keys())     # no parameter or buffer is added
    from snn_for_object_detection_amd import functional as HF
    assert HF.check_loss_options("focal", 1.5, "ciou", 2.0) == (1, 1.5, 3, 2.0)
    for bad in (("x", 2.0, "l1", 1.0), ("ce", 2.0, "x", 1.0), ("ce", -1.0, "l1", 1.0), ("ce", 2.0, "l1", -1.0)):
        with pytest.raises(ValueError):
            HF.check_loss_options(*bad)


def _tiny_net():
    class Net(S.SODa):
        def backbone_cfgs(self):
            return [S.Conv(8, 3, 2), S.Norm(), S.ReLU()]

        def neck_cfgs(self):
            return [S.Conv(8, 3, 2), S.Norm(), S.Tanh(), S.Return()]

        def head_cfgs(self, box_out, cls_out):
            return [[S.Conv(kernel_size=1)], [S.Conv(box_out, 1)], [S.Conv(cls_out, 1)]]
    return Net


@pytest.mark.parametrize("kind", ["TinyYolo", "SODa"])
def test_defaults_keep_the_reference_objective_bit_for_bit(kind):
    """Default hparams, and the default ``_loss`` on CPU tensors against the expression of the parent commit (the
    reference's, models/soda.py:259-281), restated here: the same bits, and no loss terms are kept for logging."""
    cls_ = S.TinyYolo if kind == "TinyYolo" else _tiny_net()
    m = cls_(num_classes=2, time_window=0)
    hp = m.hparams
    assert (hp.cls_loss, hp.focal_gamma, hp.box_loss, hp.box_loss_weight) == ("ce", 2.0, "l1", 1.0)
    preds, labels = _preds_and_labels()
    anchors, cls_preds, bbox_preds = preds
    loss = m._loss(preds, labels)
    off, mask, lab = m.roi_blk(anchors, labels)
    assert int((lab > 0).sum()) > 0
    ce = torch.nn.CrossEntropyLoss(reduction="none")(cls_preds.reshape(-1, 3), lab.reshape(-1))
    l1 = torch.nn.L1Loss(reduction="none")(bbox_preds * mask, off * mask)
    pos = lab.reshape(-1) > 0
    parent = ce[pos].mean() * hp.loss_ratio + ce[~pos].mean() * (1 - hp.loss_ratio) + l1.mean()
    assert torch.equal(loss.reshape(1).view(torch.int32), parent.reshape(1).view(torch.int32))
    assert m._loss_terms is None


def test_focal_gamma_0_with_l1_is_the_default_cpu_loss():
    """``(1 - p)^0 = 1`` exactly and ``sum / n`` is how torch forms a mean, so the classification term has the default's
    bits; the three terms are added as (pos + neg) + box in both.  Measured here: equal to the last bit."""
    preds, labels = _preds_and_labels()
    default = _model()._loss(preds, labels)
    m = _model(cls_loss="focal", focal_gamma=0.0, box_loss="l1")
    got = m._loss(preds, labels)
    print(f"default {float(default)!r} focal(gamma = 0) + l1 {float(got)!r}")
    assert torch.equal(got.reshape(1).view(torch.int32), default.reshape(1).view(torch.int32))
    assert float(m._loss_terms[0] + m._loss_terms[1]) == float(got)


@pytest.mark.parametrize("cls_mode,box_mode", R.MODES, ids=[f"{c}-{b}" for c, b in R.MODES])
def test_cpu_branch_against_fp64(cls_mode, box_mode):
    """``SODa._loss`` on CPU tensors (fp32 torch) against the fp64 restatement on the targets the model's own RoI assigns:
    the loss within 4x the fp32 yardstick of the mode (tests/test_gpu_det_loss_ext.py), its autograd gradients likewise."""
    preds, labels = _preds_and_labels()
    anchors, cls_preds, bbox_preds = preds
    cls_preds, bbox_preds = cls_preds.clone().requires_grad_(), bbox_preds.clone().requires_grad_()
    m = _model(loss_ratio=RATIO, cls_loss=cls_mode, focal_gamma=GAMMA, box_loss=box_mode, box_loss_weight=WEIGHT)
    loss = m._loss((anchors, cls_preds, bbox_preds), labels)
    loss.backward()
    off, mask, lab = m.roi_blk(anchors, labels)
    assert not bool(R.tied_rows(bbox_preds, off, mask, lab, anchors).any())
    ref = R.ext_loss_ref(cls_preds, bbox_preds, off, mask, lab, anchors, RATIO, cls_mode, GAMMA, box_mode, WEIGHT)
    assert ref.n_pos > 0
    d = R.deviation(loss.detach(), cls_preds.grad, bbox_preds.grad, ref)
    print(f"{cls_mode}-{box_mode}: deviations {d}")
    assert d[0] <= 4 * G.YARD_LOSS[(cls_mode, box_mode)]
    assert d[1] <= 4 * G.YARD_G_LOGITS[cls_mode]
    assert d[2] <= 4 * G.YARD_G_BBOX[("random", box_mode)]
    t_cls, t_box = (float(t.detach()) for t in m._loss_terms)
    assert abs(t_cls - ref.cls) <= 4 * G.YARD_LOSS[(cls_mode, box_mode)] * abs(ref.loss)
    assert abs(t_box - ref.box) <= 4 * G.YARD_LOSS[(cls_mode, box_mode)] * abs(ref.loss)


def test_host_expression_over_slots_drops_the_empty_ones():
    """``soda.detection_loss_host(valid=...)``: the frames of empty slots take no part; no valid frame gives zeros."""
    inp = R.ext_inputs(6, 50, 3, "random", 9)
    steps = torch.tensor([[3, -1], [5, 2], [7, 4]], dtype=torch.int32)
    cls, box = soda.detection_loss_host(inp.logits, inp.bbox, inp.offset, inp.mask, inp.labels, inp.anchors, RATIO,
                                        "focal", GAMMA, "ciou", WEIGHT, valid=steps >= 0)
    ref = R.ext_loss_ref(*inp, RATIO, "focal", GAMMA, "ciou", WEIGHT, steps=steps)
    assert ref.V == 5
    assert abs(float(cls) - ref.cls) <= 4 * G.YARD_LOSS[("focal", "ciou")] * ref.loss
    assert abs(float(box) - ref.box) <= 4 * G.YARD_LOSS[("focal", "ciou")] * ref.loss
    cls, box = soda.detection_loss_host(inp.logits, inp.bbox, inp.offset, inp.mask, inp.labels, inp.anchors, RATIO,
                                        "focal", GAMMA, "giou", WEIGHT, valid=torch.zeros(3, 2, dtype=torch.bool))
    assert float(cls) == 0.0 and float(box) == 0.0
    none = R.ext_loss_ref(*inp, RATIO, "focal", GAMMA, "giou", WEIGHT, steps=torch.full((3, 2), -1))
    assert none.V == 0 and none.loss == 0.0 and not none.g_logits.any() and not none.g_bbox.any()


def test_the_yardstick_constants_cover_the_fp32_evaluation():
    """The constants of tests/test_gpu_det_loss_ext.py are the largest fp32-CPU deviations from fp64 over that file's
    shapes and cases; re-measured here on its small shapes (the large one takes part in the recorded numbers only).  The
    reference rows are free of ties, the named cases reach what they are named for."""
    for Fr, A, K in G.SMALL_SHAPES:
        for case in R.CASES:
            inp = G.inputs(Fr, A, K, case)
            if case != "equal":
                assert not bool(R.tied_rows(inp.bbox, inp.offset, inp.mask, inp.labels, inp.anchors).any())
            G.check_case_reaches_its_edge(inp, case)
            for c, b in R.MODES:
                args = (*inp, RATIO, c, GAMMA, b, WEIGHT)
                r64, r32 = R.ext_loss_ref(*args), R.ext_loss_ref(*args, dtype=torch.float32)
                d = R.deviation(r32.loss, r32.g_logits, r32.g_bbox, r64, skip_box_rows=case == "equal")
                # (another CPU may round the fp32 evaluation differently in the last bits: 1.5x)
                assert d[0] <= 1.5 * G.YARD_LOSS[(c, b)], (Fr, A, K, case, c, b, d)
                assert d[1] <= 1.5 * G.YARD_G_LOGITS[c], (Fr, A, K, case, c, b, d)
                assert d[2] <= 1.5 * G.YARD_G_BBOX[(case, b)], (Fr, A, K, case, c, b, d)


def test_new_symbols_are_declared_and_bound():
    from snn_for_object_detection_amd import _build, _hip
    header = open(os.path.join(os.path.dirname(_hip._HERE), "include", "snn_hip.h")).read()
    assert "#define SNN_ABI_VERSION 20" in header and _hip.ABI_VERSION == 20        # symbols added, nothing changed
    plain = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    declared = set(re.findall(r"\b(snn_[a-z0-9_]+)\s*\(", plain))
    for name, n_args in NEW_SYMBOLS.items():
        assert name in declared, name
        assert name in _hip.SIGNATURES and len(_hip.SIGNATURES[name][1]) == n_args, name
    for name, value in (("SNN_LOSS_CLS_CE", 0), ("SNN_LOSS_CLS_FOCAL", 1), ("SNN_LOSS_BOX_L1", 0),
                        ("SNN_LOSS_BOX_GIOU", 1), ("SNN_LOSS_BOX_DIOU", 2), ("SNN_LOSS_BOX_CIOU", 3)):
        assert re.search(rf"\b{name} = {value}\b", plain), name
    assert _hip.LOSS_CLS_MODES == {"ce": 0, "focal": 1}
    assert _hip.LOSS_BOX_MODES == {"l1": 0, "giou": 1, "diou": 2, "ciou": 3}
    assert tuple(_hip.LOSS_CLS_MODES) == soda.LOSS_CLS_NAMES and tuple(_hip.LOSS_BOX_MODES) == soda.LOSS_BOX_NAMES
    assert "det_loss.hip" in _build.SOURCES
    # the signatures of the existing loss entry points are the parent's
    assert len(_hip.SIGNATURES["snn_det_loss_fwd"][1]) == 12 and len(_hip.SIGNATURES["snn_det_loss_bwd"][1]) == 13
    assert len(_hip.SIGNATURES["snn_det_loss_steps_fwd"][1]) == 15 and len(_hip.SIGNATURES["snn_det_loss_steps_bwd"][1]) == 16


def test_training_tool_takes_the_loss_options():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools",
                            "train_on_recordings.py")).read()
    for flag in ("--cls-loss", "--focal-gamma", "--box-loss", "--box-loss-weight"):
        assert f'"{flag}"' in src, flag
