"""CPU restatement of training on every labelled timestep (TEST INFRASTRUCTURE ONLY; nothing here imports the package).

Labels are ``[B, N, 6]`` rows ``(ts, class, x1, y1, x2, y2)``: ``ts`` the integer-valued timestep of the uncut sequence,
-1 in every column a padding row.  The training step drops a prefix of ``t0`` frames, so a row belongs to step
``ts - t0`` of the cut sequence of ``T`` steps; rows outside ``[0, T)`` are ignored.

``select_steps_ref``   the slots: per sample the latest ``K`` distinct steps of its real rows, ascending, -1 behind them.
``slot_rows``          the ``[n, 5]`` label tensor of one slot: the sample's real rows of that step and its padding rows,
                       in their order (padding rows keep upstream's quirk of claiming an anchor; rows of other
                       timesteps take no part).
``roi_steps_ref``      per valid slot ``targets_ref.roi_assign_ref`` on those rows; zeros for an empty slot.
``loss_steps_ref``     ``targets_ref.det_loss_ref`` over the concatenated rows of the valid slots (so the L1 term is
                       divided by ``4 A V``), scattered back to ``[K, B, A, .]`` with exact zeros in the empty slots;
                       ``V = 0`` gives loss 0.0 and zero gradients.
"""
from typing import List, NamedTuple, Optional

import torch

from tests import targets_ref as TR

F32, F64 = torch.float32, torch.float64


def row_step(row, t0: int, T: int) -> int:
    """Step of the cut sequence of one six-column row; -1 for a padding row or a row outside ``[0, T)``."""
    if float(row[1]) < 0:
        return -1
    s = int(row[0]) - t0
    return s if 0 <= s < T else -1


def select_steps_ref(labels6: torch.Tensor, T: int, K: int, t0: int = 0) -> torch.Tensor:
    """-> ``steps[K, B]`` int32."""
    B = labels6.shape[0]
    steps = torch.full((K, B), -1, dtype=torch.int32)
    for b in range(B):
        distinct = sorted({row_step(r, t0, T) for r in labels6[b]} - {-1})
        for k, s in enumerate(distinct[-K:]):
            steps[k, b] = s
    return steps


def slot_rows(sample6: torch.Tensor, s: int, t0: int) -> torch.Tensor:
    """The rows of one sample ``[N, 6]`` that take part in the slot of step ``s``, as ``[n, 5]``."""
    keep = [j for j, r in enumerate(sample6) if float(r[1]) < 0 or int(r[0]) - t0 == s]
    return sample6[keep][:, 1:].to(F32).contiguous()


class RoiStepsRef(NamedTuple):
    classes: torch.Tensor        # [K, B, A] int64
    masks: torch.Tensor          # [K, B, A, 4] fp32
    offsets: torch.Tensor        # [K, B, A, 4] fp32
    offsets64: torch.Tensor      # [K, B, A, 4] fp64
    rows: List[List[Optional[torch.Tensor]]]   # [K][B]: the [n, 5] rows of the slot, None when it is empty


def roi_steps_ref(anchors: torch.Tensor, labels6: torch.Tensor, steps: torch.Tensor, t0: int, thr: float) -> RoiStepsRef:
    K, B = steps.shape
    A = anchors.shape[0]
    classes = torch.zeros(K, B, A, dtype=torch.long)
    masks = torch.zeros(K, B, A, 4, dtype=F32)
    offsets = torch.zeros(K, B, A, 4, dtype=F32)
    offsets64 = torch.zeros(K, B, A, 4, dtype=F64)
    rows = [[None] * B for _ in range(K)]
    for k in range(K):
        for b in range(B):
            s = int(steps[k, b])
            if s < 0:
                continue
            rows[k][b] = slot_rows(labels6[b], s, t0)
            ref = TR.roi_assign_ref(anchors, rows[k][b].unsqueeze(0), thr)
            classes[k, b], masks[k, b], offsets[k, b], offsets64[k, b] = (ref.classes[0], ref.masks[0], ref.offsets[0],
                                                                          ref.offsets64[0])
    return RoiStepsRef(classes, masks, offsets, offsets64, rows)


class LossStepsRef(NamedTuple):
    V: int
    loss: float
    g_logits: torch.Tensor       # [K, B, A, C] fp64, zeros in the empty slots
    g_bbox: torch.Tensor         # [K, B, A, 4] fp64
    valid: torch.Tensor          # [K, B] bool
    inner: Optional[TR.LossRef]  # det_loss_ref over the [V * A] rows of the valid slots (slot order); None when V = 0


def loss_steps_ref(logits, bbox, offset, mask, classes, steps, ratio, g_loss=1.0) -> LossStepsRef:
    """``logits[K, B, A, C]``, ``bbox / offset / mask [K, B, A, 4]``, ``classes[K, B, A]``, ``steps[K, B]``."""
    K, B, A, C = logits.shape
    valid = steps.cpu() >= 0
    V = int(valid.sum())
    g_logits = torch.zeros(K, B, A, C, dtype=F64)
    g_bbox = torch.zeros(K, B, A, 4, dtype=F64)
    if V == 0:
        return LossStepsRef(0, 0.0, g_logits, g_bbox, valid, None)
    sel = valid.reshape(-1)

    def rows(t, last):
        return t.detach().cpu().reshape(K * B, A, last)[sel].reshape(V * A, last)

    inner = TR.det_loss_ref(rows(logits, C), rows(bbox, 4), rows(offset, 4), rows(mask, 4),
                            classes.detach().cpu().reshape(K * B, A)[sel].reshape(-1), ratio, g_loss)
    g_logits.reshape(K * B, A, C)[sel] = inner.g_logits.reshape(V, A, C)
    g_bbox.reshape(K * B, A, 4)[sel] = inner.g_bbox.reshape(V, A, 4)
    return LossStepsRef(V, inner.loss, g_logits, g_bbox, valid, inner)


# ------------------------------------------------------------------------------------------------------ inputs
def grid_anchors(h: int = 4, w: int = 4, per_cell: int = 9, seed: int = 11) -> torch.Tensor:
    """``h * w * per_cell`` anchors with corners on the 1/64 grid (``targets_ref.grid_boxes``): equal geometry gives
    bit-equal IoUs, and the fp32 assignment arithmetic stays exact."""
    return TR.grid_boxes(h * w * per_cell, torch.Generator().manual_seed(seed), max_side=24)


def labels6_from(anchors: torch.Tensor, plan, N: int, seed: int = 5, classes: int = 2) -> torch.Tensor:
    """``plan[b]`` lists the timestep of each real row of sample ``b`` (at most ``N``); the remaining rows are padding.
    The rows themselves come from ``targets_ref.populated_labels`` (``classes`` of them: C + 1 = 3 logits by default)."""
    g = torch.Generator().manual_seed(seed)
    out = torch.full((len(plan), N, 6), -1.0)
    for b, ts in enumerate(plan):
        rows = TR.populated_labels(anchors, N, g, classes=classes)
        for j, t in enumerate(ts):
            out[b, j, 0] = float(t)
            out[b, j, 1:] = rows[j]
    return out
