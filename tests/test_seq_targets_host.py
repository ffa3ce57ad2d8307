"""Training on every labelled timestep, host side: the CPU restatement (tests/seq_targets_ref.py) against the
single-label references it must reduce to, the slot selection on hand-written cases and on the stored MT sample, the
refusal of six-column labels without ``label_steps``, and the declaration / binding of the new C-ABI symbols."""
import os
import re

import numpy as np
import pytest
import torch

import snn_for_object_detection_amd as S
from tests import seq_targets_ref as SR
from tests import targets_ref as TR

NEW_SYMBOLS = ("snn_label_steps", "snn_gather_steps_fwd", "snn_gather_steps_bwd", "snn_roi_steps_workspace_size",
               "snn_roi_assign_steps", "snn_det_loss_steps_workspace_size", "snn_det_loss_steps_fwd",
               "snn_det_loss_steps_bwd")


def _row(ts, cls=0.0):
    return [float(ts), cls, 0.25, 0.25, 0.5, 0.5]


PAD = [-1.0] * 6


@pytest.mark.parametrize("pad_rows", [0, 2])
def test_one_step_and_one_slot_is_the_single_label_assignment_and_loss(pad_rows):
    """All real rows on one step, K = 1: the slot's rows are the five-column labels, padding rows included, so the
    assignment and the loss are those of ``roi_assign_ref`` / ``det_loss_ref`` on them."""
    anchors = SR.grid_anchors()
    A, N, B, T = anchors.shape[0], 5, 3, 6
    labels6 = SR.labels6_from(anchors, [[5] * (N - pad_rows)] * B, N)
    labels5 = labels6[:, :, 1:].contiguous()
    steps = SR.select_steps_ref(labels6, T, 1)
    assert steps.tolist() == [[5, 5, 5]]
    got = SR.roi_steps_ref(anchors, labels6, steps, 0, 0.5)
    ref = TR.roi_assign_ref(anchors, labels5, 0.5)
    assert torch.equal(got.classes[0], ref.classes) and torch.equal(got.masks[0], ref.masks)
    assert torch.equal(got.offsets[0], ref.offsets) and torch.equal(got.offsets64[0], ref.offsets64)
    if pad_rows:
        assert int(((ref.classes == 0) & (ref.masks[..., 0] == 1)).sum()) == pad_rows * B   # the padding quirk is there
    g = torch.Generator().manual_seed(3)
    logits, bbox = torch.randn(1, B, A, 3, generator=g), torch.randn(1, B, A, 4, generator=g)
    for g_loss in (1.0, -2.5):
        a = SR.loss_steps_ref(logits, bbox, got.offsets, got.masks, got.classes, steps, 0.04, g_loss)
        b = TR.det_loss_ref(logits[0], bbox[0], ref.offsets, ref.masks, ref.classes, 0.04, g_loss)
        assert a.V == B and a.loss == b.loss
        assert torch.equal(a.g_logits.reshape(-1, 3), b.g_logits) and torch.equal(a.g_bbox.reshape(-1, 4), b.g_bbox)


def test_slot_selection_on_hand_written_cases():
    labels = torch.tensor([
        [_row(2), _row(2, 1.0), _row(4), PAD, PAD],               # duplicate rows on one step
        [_row(0), _row(1), _row(3), _row(5), _row(3)],            # more than K distinct steps: the latest stay
        [PAD, PAD, PAD, PAD, PAD],                                # padding rows only
        [_row(1), _row(6), _row(9), PAD, _row(4)],                # ts >= T
    ])
    T = 6
    assert SR.select_steps_ref(labels, T, 1).tolist() == [[4, 5, -1, 4]]
    assert SR.select_steps_ref(labels, T, 2).tolist() == [[2, 3, -1, 1], [4, 5, -1, 4]]
    assert SR.select_steps_ref(labels, T, 3).tolist() == [[2, 1, -1, 1], [4, 3, -1, 4], [-1, 5, -1, -1]]
    # a prefix of t0 = 2 frames cuts the steps below 2 away and shifts the others; T counts the frames that are left
    assert SR.select_steps_ref(labels, T - 2, 3, t0=2).tolist() == [[0, 1, -1, 2], [2, 3, -1, -1], [-1, -1, -1, -1]]
    assert SR.select_steps_ref(labels, 4, 2, t0=3).tolist() == [[1, 0, -1, 1], [-1, 2, -1, 3]]
    # the rows that take part: the step's real rows and the padding rows, in their order
    rows = SR.slot_rows(labels[0], 2, 0)
    assert rows.shape == (4, 5) and rows[:, 0].tolist() == [0.0, 1.0, -1.0, -1.0]
    assert SR.slot_rows(labels[0], 2, 2).tolist() == [_row(4)[1:], PAD[1:], PAD[1:]]
    assert SR.slot_rows(labels[3], 4, 0)[:, 0].tolist() == [-1.0, 0.0]


def test_an_empty_batch_has_loss_zero_and_zero_gradients():
    anchors = SR.grid_anchors()
    A, B, K = anchors.shape[0], 2, 2
    labels6 = torch.full((B, 3, 6), -1.0)
    steps = SR.select_steps_ref(labels6, 6, K)
    assert bool((steps == -1).all())
    roi = SR.roi_steps_ref(anchors, labels6, steps, 0, 0.5)
    assert not roi.classes.any() and not roi.masks.any() and not roi.offsets.any()
    out = SR.loss_steps_ref(torch.randn(K, B, A, 3), torch.randn(K, B, A, 4), roi.offsets, roi.masks, roi.classes, steps,
                            0.04)
    assert out.V == 0 and out.loss == 0.0 and not out.g_logits.any() and not out.g_bbox.any()


def test_the_stored_mt_sample_passes_through_the_selection(golden_dir):
    """``MTPropheseeDataset.parse_data``'s labels as tests/golden/events.npz pins them: rows on the steps 0, 2 and 4 of a
    five-step window."""
    z = np.load(os.path.join(golden_dir, "events.npz"))
    lab = torch.from_numpy(z["mt_labels"])
    T = int(z["mt_params"][0])
    assert lab.shape == (3, 6) and T == 5
    batch = torch.stack([lab, torch.full_like(lab, -1.0)])
    assert SR.select_steps_ref(batch, T, 2).tolist() == [[2, -1], [4, -1]]
    assert SR.select_steps_ref(batch, T, 3).tolist() == [[0, -1], [2, -1], [4, -1]]
    assert SR.select_steps_ref(batch, T - 1, 3, t0=1).tolist() == [[1, -1], [3, -1], [-1, -1]]
    rows = SR.slot_rows(batch[0], 2, 0)
    assert torch.equal(rows, lab[1:2, 1:])


def test_six_column_labels_need_label_steps():
    m = S.TinyYolo(num_classes=2, time_window=0)
    assert m.hparams.label_steps is None
    X, labels = torch.zeros(3, 1, 2, 32, 48), torch.full((1, 2, 6), -1.0)
    for step in (m.training_step, m.validation_step, m.test_step):
        with pytest.raises(ValueError, match="label_steps"):
            step((X, labels))
    m2 = S.TinyYolo(num_classes=2, time_window=0, label_steps=2)
    assert m2.hparams.label_steps == 2
    assert list(m2.state_dict().keys()) == list(m.state_dict().keys())        # the keyword adds no parameter or buffer
    with pytest.raises(ValueError, match="label_steps"):
        S.TinyYolo(num_classes=2, label_steps=0)
    with pytest.raises(ValueError, match="label_steps"):
        S.TinyYolo(num_classes=2, label_steps=33)


def test_label_collation_keeps_the_width_of_the_rows_it_is_given():
    """``EventBatcher``'s label padding (``data.collate_labels``, host side): six-column rows stay six columns wide, a
    sample without boxes fits either width whatever its own shape, no row at all falls back to five columns, mixed
    widths raise."""
    from snn_for_object_detection_amd.data import collate_labels
    six = [torch.tensor([_row(2), _row(4, 1.0)]), torch.zeros(0, 6), torch.tensor([_row(1)])]
    out = collate_labels(six, 3)
    assert out.shape == (3, 2, 6) and out.dtype == torch.float32
    assert torch.equal(out[0], six[0]) and bool((out[1] == -1).all())
    assert torch.equal(out[2, 0], six[2][0]) and bool((out[2, 1] == -1).all())
    # an empty sample written as (0, 5) or as a plain empty tensor next to six-column samples
    for empty in (torch.zeros(0, 5), torch.zeros(0)):
        assert torch.equal(collate_labels([six[0], empty, six[2]], 3), out)
    five = [torch.tensor([_row(0)[1:]]), torch.zeros(0, 5)]
    out5 = collate_labels(five, 2)
    assert out5.shape == (2, 1, 5) and torch.equal(out5[0], five[0]) and bool((out5[1] == -1).all())
    assert collate_labels([torch.zeros(0, 6), torch.zeros(0, 5)], 2).shape == (2, 0, 5)
    assert collate_labels([], 0).shape == (0, 0, 5)
    with pytest.raises(ValueError, match="5 or all have 6"):
        collate_labels([six[0], five[0]], 2)
    with pytest.raises(ValueError, match="5 or all have 6"):
        collate_labels([torch.zeros(2, 4)], 1)
    # the selection reads what the collation wrote
    assert SR.select_steps_ref(out, 6, 2).tolist() == [[2, -1, 1], [4, -1, -1]]


def test_head_refuses_steps_for_a_single_frame():
    head = S.HeadGen(lambda box_out, cls_out: [[S.Conv(kernel_size=1)], [S.Conv(box_out, 1)], [S.Conv(cls_out, 1)]],
                     8, 6, in_channels=4)
    with pytest.raises(ValueError, match="sequence"):
        head(torch.zeros(2, 4, 3, 3), None, steps=torch.zeros(1, 2, dtype=torch.int32))


def test_new_symbols_are_declared_and_bound():
    from snn_for_object_detection_amd import _hip
    header = open(os.path.join(os.path.dirname(_hip._HERE), "include", "snn_hip.h")).read()
    assert "#define SNN_ABI_VERSION 20" in header and _hip.ABI_VERSION == 20
    declared = set(re.findall(r"\b(snn_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", " ", header, flags=re.S)))
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert name in _hip.SIGNATURES, name
