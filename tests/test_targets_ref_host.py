"""The references of tests/targets_ref.py are themselves checked (host only): the fp32 assignment against vectors the
reference's own code produced and against the package's host path, the closed-form fp64 loss against torch autograd."""
import os
import time

import numpy as np
import pytest
import torch

from tests import targets_ref as TR

CASES = TR.roi_cases()


def test_roi_ref_reproduces_the_reference_vectors(golden_dir):
    """tests/golden/detect_roi.npz holds outputs of the reference's utils/roi.py on the GEN1 anchor set."""
    z = np.load(os.path.join(golden_dir, "detect_roi.npz"))
    anchors = torch.from_numpy(np.load(os.path.join(golden_dir, "detect_anchors.npz"))["anchors_gen1"])
    for tag in ("plain", "padded"):
        ref = TR.roi_assign_ref(anchors, torch.from_numpy(z[f"labels_{tag}"]), float(z["iou_threshold"]))
        assert torch.equal(ref.classes, torch.from_numpy(z[f"cls_{tag}"])), tag
        assert torch.equal(ref.masks, torch.from_numpy(z[f"mask_{tag}"])), tag
        assert torch.equal(ref.offsets, torch.from_numpy(z[f"offset_{tag}"])), tag


@pytest.mark.parametrize("cs", CASES, ids=[c.id for c in CASES])
def test_roi_ref_equals_the_host_path(cs):
    """Every case of the table: the reference reaches the edge the case is there for (its own check on the per-round
    record), and the package's host path (roi.RoI on CPU tensors) gives the same classes, masks and offsets."""
    from snn_for_object_detection_amd.roi import RoI
    t0 = time.perf_counter()
    ref = TR.roi_assign_ref(cs.anchors, cs.labels, cs.thr)
    took = time.perf_counter() - t0
    if cs.check is not None:
        cs.check(ref)
    assert all(r[2] < cs.anchors.shape[0] for rounds in ref.rounds for r in rounds)
    off, mask, cls = RoI(cs.thr)(cs.anchors.clone(), cs.labels.clone())
    assert cls.dtype == torch.int64 and torch.equal(cls, ref.classes)
    assert torch.equal(mask, ref.masks)
    assert torch.equal(off, ref.offsets)
    # the fp64 offsets are the same assignment: they differ from the fp32 ones by fp32 rounding only
    assert torch.allclose(ref.offsets.double(), ref.offsets64, rtol=1e-5, atol=1e-5)
    assert took < 5.0, f"the host reference took {took:.1f} s"


def test_roi_ref_float_quotient_differs_from_integer_quotient_only_above_2p24():
    """The fp32 quotient the reference forms is idx // N for every flat index below 2^24 (both operands exact)."""
    g = torch.Generator().manual_seed(1)
    for N in (1, 2, 7, 33, 100, 128):
        idx = torch.randint(0, 2 ** 24, (200_000,), generator=g)
        assert torch.equal((idx / N).long(), idx // N), N
    idx = torch.tensor([540_000 * 32 + 31])
    assert int((idx / 32).long()) == 540_001


LOSS_SMALL = [(1, 2), (7, 3), (255, 3), (257, 8), (300, 64)]
LOSS_CONDS = ("base", "g_ratio", "no_pos", "no_neg", "big_logits")


@pytest.mark.parametrize("cond", LOSS_CONDS)
@pytest.mark.parametrize("rows,K", LOSS_SMALL)
def test_det_loss_ref_equals_autograd_in_float64(rows, K, cond):
    """The reference expression (models/soda.py:259-281) through torch autograd in float64: 1e-12 relative, elementwise."""
    logits, bbox, offset, mask, labels, ratio, g_loss = TR.loss_inputs(rows, K, cond, seed=rows * 131 + K)
    ref = TR.det_loss_ref(logits, bbox, offset, mask, labels, ratio, g_loss)
    r32 = float(torch.tensor(ratio, dtype=torch.float32))
    x = logits.double().requires_grad_()
    b = bbox.double().requires_grad_()
    ce = torch.nn.functional.cross_entropy(x, labels, reduction="none")
    pos = labels > 0
    m, off = mask.double(), offset.double()
    loss = ce[pos].mean() * r32 + ce[~pos].mean() * (1 - r32) + torch.nn.functional.l1_loss(b * m, off * m)
    assert int(ref.stats[1]) == int(pos.sum()) and int(ref.stats[3]) == int((~pos).sum())
    if cond in ("no_pos", "no_neg") or pos.all() or not pos.any():
        assert torch.isnan(loss) and ref.loss != ref.loss
        # the gradient of the terms that have rows (the mean of nothing has no row to send a gradient to)
        live = ce[pos].mean() * r32 if pos.any() else ce[~pos].mean() * (1 - r32)
        (live + torch.nn.functional.l1_loss(b * m, off * m)).backward(torch.tensor(float(torch.tensor(g_loss)),
                                                                                    dtype=torch.float64))
    else:
        assert abs(ref.loss - loss.item()) <= 1e-12 * abs(loss.item())
        loss.backward(torch.tensor(float(torch.tensor(g_loss)), dtype=torch.float64))
    assert torch.isfinite(ref.g_logits).all() and torch.isfinite(ref.g_bbox).all()
    # softmax - onehot lies in [-1, 1] and cancels at the label's entry of a well-classified row (both sides round
    # p - 1 at 1e-16): relative to the row's weight there, relative to the value everywhere else
    err = (ref.g_logits - x.grad).abs()
    onehot = torch.nn.functional.one_hot(labels, K).bool()
    assert bool((err <= 1e-12 * torch.where(onehot, ref.w.abs()[:, None].expand_as(err), x.grad.abs()) + 1e-300).all())
    assert bool(((ref.g_bbox - b.grad).abs() <= 1e-12 * b.grad.abs()).all())
    # torch forms log(1 + rest) from the rounded sum 1 + rest and rounds the result again (2^-53 absolute each, and its
    # accumulation of the sum); the reference takes log1p(rest)
    assert bool(((ref.ce - ce.detach()).abs() <= 1e-12 * ce.detach().abs() + 2.0 ** -51).all())
    # the edges every case carries
    diff = b.detach() * m - off * m
    assert bool((diff == 0).any()) and bool((ref.g_bbox[diff == 0] == 0).all())
    if rows >= 5 and cond != "no_neg":
        assert bool(((labels == 0) & (mask[:, 0] == 1)).any())
