"""Anchor <-> ground-truth assignment (mirror of the reference's ``utils/roi.py``).

Same arithmetic and the same results as ``utils/roi.py:18-109`` (pinned bit-exactly by
``tests/golden/detect_roi.npz``).  Device tensors take ONE HIP kernel launch for the whole batch
(``snn_roi_assign``, ``csrc/targets.hip``: one block per sample, the greedy per-ground-truth phase included); the
tensor form below is the host path the fixtures pin, written without ``nonzero`` / boolean indexing.
"""

import math

import torch

from . import box


class RoI:
    """``RoI(iou_threshold)(anchors[A,4], labels[B,N,5]) -> (bbox_offset, bbox_mask, class_labels)``.

    An anchor takes the ground-truth box of highest IoU when that IoU reaches the threshold; afterwards
    every ground-truth ROW (padding rows of -1 included - a reference quirk kept for parity) greedily
    claims the globally best remaining anchor.  Class 0 is background.
    """

    def __init__(self, iou_threshold=0.5) -> None:
        self.iou_threshold = iou_threshold

    def __call__(self, anchors: torch.Tensor, labels: torch.Tensor):
        if anchors.is_cuda:
            return self._device(anchors, labels)
        offsets, masks, classes = [], [], []
        for label in labels:
            amap = self._assign_anchor_to_box(label[:, 1:], anchors)
            assigned = amap >= 0
            bbox_mask = assigned.float().unsqueeze(-1).repeat(1, 4)
            row = amap.clamp(min=0)
            class_labels = torch.where(assigned, label[row, 0].long() + 1, torch.zeros_like(amap))
            assigned_bb = torch.where(assigned.unsqueeze(-1), label[row, 1:], torch.zeros_like(anchors))
            offsets.append(box.offset_boxes(anchors, assigned_bb) * bbox_mask)
            masks.append(bbox_mask)
            classes.append(class_labels)
        return torch.stack(offsets), torch.stack(masks), torch.stack(classes)

    def _device(self, anchors: torch.Tensor, labels: torch.Tensor):
        from . import _hip
        anchors = anchors.detach().contiguous().float()
        labels = labels.detach().to(anchors.device).contiguous().float()
        B, N, _ = labels.shape
        A = anchors.shape[0]
        dev = anchors.device
        ws = torch.empty(_hip.query("snn_roi_workspace_size", B, A, N), device=dev, dtype=torch.uint8)
        offset = torch.empty((B, A, 4), device=dev, dtype=torch.float32)
        mask = torch.empty((B, A, 4), device=dev, dtype=torch.float32)
        cls = torch.empty((B, A), device=dev, dtype=torch.int64)
        _hip.call("snn_roi_assign", anchors.data_ptr(), labels.data_ptr(), B, A, N, float(self.iou_threshold),
                  ws.data_ptr(), offset.data_ptr(), mask.data_ptr(), cls.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
        return offset, mask, cls

    def steps(self, anchors: torch.Tensor, labels: torch.Tensor, steps: torch.Tensor, t0: int = 0):
        """Targets of every labelled frame (device only): ``labels[B,N,6]`` rows ``(ts, class, x1, y1, x2, y2)``,
        ``steps[K,B]`` from ``functional.select_label_steps`` ->
        ``(bbox_offset[K,B,A,4], bbox_mask[K,B,A,4], class_labels[K,B,A])``.

        Slot ``(k, b)`` is ``__call__`` for one sample whose label tensor holds the real rows of sample ``b`` with
        ``ts - t0 == steps[k][b]`` and its padding rows, in their order; rows of other timesteps take no part, an empty
        slot (-1) gets zeros.  One launch for all slots."""
        from . import _hip
        if not anchors.is_cuda:
            raise RuntimeError("RoI.steps runs on device tensors only (no CPU fallback)")
        anchors = anchors.detach().contiguous().float()
        labels = labels.detach().to(anchors.device).contiguous().float()
        if labels.dim() != 3 or labels.shape[2] != 6:
            raise RuntimeError(f"RoI.steps: labels[B,N,6] required, got {tuple(labels.shape)}")
        B, N, _ = labels.shape
        if steps.dim() != 2 or steps.shape[1] != B or steps.dtype != torch.int32 or steps.device != anchors.device:
            raise RuntimeError(f"RoI.steps: steps must be an int32 [K, {B}] tensor on {anchors.device}")
        steps = steps.contiguous()
        K, A, dev = int(steps.shape[0]), anchors.shape[0], anchors.device
        if N == 0:   # no rows at all: every slot is empty
            return (torch.zeros((K, B, A, 4), device=dev), torch.zeros((K, B, A, 4), device=dev),
                    torch.zeros((K, B, A), device=dev, dtype=torch.int64))
        ws = torch.empty(_hip.query("snn_roi_steps_workspace_size", K, B, A, N), device=dev, dtype=torch.uint8)
        offset = torch.empty((K, B, A, 4), device=dev, dtype=torch.float32)
        mask = torch.empty((K, B, A, 4), device=dev, dtype=torch.float32)
        cls = torch.empty((K, B, A), device=dev, dtype=torch.int64)
        _hip.call("snn_roi_assign_steps", anchors.data_ptr(), labels.data_ptr(), steps.data_ptr(), K, B, A, N, int(t0),
                  float(self.iou_threshold), ws.data_ptr(), offset.data_ptr(), mask.data_ptr(), cls.data_ptr(),
                  torch.cuda.current_stream().cuda_stream)
        return offset, mask, cls

    def _assign_anchor_to_box(self, ground_truth: torch.Tensor, anchors: torch.Tensor) -> torch.Tensor:
        num_gt = ground_truth.shape[0]
        iou = box.box_iou(anchors, ground_truth)
        best_iou, best_gt = torch.max(iou, dim=1)
        amap = torch.where(best_iou >= self.iou_threshold, best_gt, torch.full_like(best_gt, -1))
        for _ in range(num_gt):
            flat = torch.argmax(iou)
            gt_idx = (flat % num_gt).long()
            anc_idx = (flat / num_gt).long()  # float division + truncation, as the reference does
            amap.index_fill_(0, anc_idx.reshape(1), 0)
            amap.index_add_(0, anc_idx.reshape(1), gt_idx.reshape(1))
            iou.index_fill_(1, gt_idx.reshape(1), -1.0)
            iou.index_fill_(0, anc_idx.reshape(1), -1.0)
        return amap


_EXP_CLAMP = math.log(1000.0 / 16.0)   # upper clamp of the exponent argument of a decoded box side (csrc/det_loss.hip)
_IOU_EPS = 1e-7


class TaskAlignedAssigner:
    """``TaskAlignedAssigner(topk, alpha, beta)(anchors[A,4], labels[B,N,5], cls_preds[B,A,C+1], bbox_preds[B,A,4])
    -> (bbox_offset, bbox_mask, class_labels)`` with the shapes and dtypes of ``RoI``.

    The positives follow the predictions (DESIGN "Anchor assignment"), which are read as constants: every label row that
    takes part (a real class the logits have a column for, a box of positive area) selects, among the anchors whose centre
    lies strictly inside its box, the ``topk`` of largest ``t = s^alpha * u^beta`` - ``s`` the softmax probability of the
    row's class, ``u`` the IoU of the decoded predicted box with the row's box; an anchor selected by several rows goes
    to the row of largest ``u``; a row left without an anchor claims the unassigned anchor of highest anchor IoU.  Padding
    rows take no part.  Device tensors take ``snn_tal_assign`` (``csrc/targets.hip``: three launches for the whole batch,
    no host synchronisation); the tensor form below is the host path, written without ``nonzero`` / boolean indexing.
    """

    def __init__(self, topk: int = 10, alpha: float = 1.0, beta: float = 6.0) -> None:
        if not 1 <= int(topk) <= 64:
            raise ValueError(f"topk must be in 1 .. 64, got {topk}")
        for name, v in (("alpha", alpha), ("beta", beta)):
            if not (float(v) >= 0.0 and math.isfinite(float(v))):
                raise ValueError(f"{name} must be finite and >= 0, got {v}")
        self.topk, self.alpha, self.beta = int(topk), float(alpha), float(beta)

    def __call__(self, anchors: torch.Tensor, labels: torch.Tensor, cls_preds: torch.Tensor, bbox_preds: torch.Tensor,
                 return_rows: bool = False):
        """``return_rows``: additionally the label-row index per anchor (``[B,A]``, -1 = background; int32 on the device,
        int64 on the host)."""
        if anchors.is_cuda:
            return self._device(anchors, labels, None, 0, cls_preds, bbox_preds, return_rows)
        anchors = anchors.detach().float()
        offsets, masks, classes, rows = [], [], [], []
        for label, cls, bb in zip(labels.detach().float(), cls_preds.detach().float(), bbox_preds.detach().float()):
            amap = self._assign(anchors, label, cls, bb)
            assigned = amap >= 0
            bbox_mask = assigned.float().unsqueeze(-1).repeat(1, 4)
            row = amap.clamp(min=0)
            class_labels = torch.where(assigned, label[row, 0].long() + 1, torch.zeros_like(amap))
            assigned_bb = torch.where(assigned.unsqueeze(-1), label[row, 1:], torch.zeros_like(anchors))
            offsets.append(box.offset_boxes(anchors, assigned_bb) * bbox_mask)
            masks.append(bbox_mask)
            classes.append(class_labels)
            rows.append(amap)
        out = (torch.stack(offsets), torch.stack(masks), torch.stack(classes))
        return out + (torch.stack(rows),) if return_rows else out

    def steps(self, anchors: torch.Tensor, labels: torch.Tensor, steps: torch.Tensor, t0: int, cls_preds: torch.Tensor,
              bbox_preds: torch.Tensor, return_rows: bool = False):
        """Targets of every labelled frame (device only), as ``RoI.steps``: ``labels[B,N,6]``, ``steps[K,B]``,
        ``cls_preds[K,B,A,C+1]``, ``bbox_preds[K,B,A,4]`` -> ``(bbox_offset[K,B,A,4], bbox_mask[K,B,A,4],
        class_labels[K,B,A])``.  Slot ``(k, b)`` is ``__call__`` on the rows of sample ``b`` with
        ``ts - t0 == steps[k][b]``; an empty slot gets zeros."""
        if not anchors.is_cuda:
            raise RuntimeError("TaskAlignedAssigner.steps runs on device tensors only (no CPU fallback)")
        if labels.dim() != 3 or labels.shape[2] != 6:
            raise RuntimeError(f"TaskAlignedAssigner.steps: labels[B,N,6] required, got {tuple(labels.shape)}")
        B = labels.shape[0]
        if steps.dim() != 2 or steps.shape[1] != B or steps.dtype != torch.int32 or steps.device != anchors.device:
            raise RuntimeError(f"TaskAlignedAssigner.steps: steps must be an int32 [K, {B}] tensor on {anchors.device}")
        return self._device(anchors, labels, steps.contiguous(), int(t0), cls_preds, bbox_preds, return_rows)

    def _device(self, anchors, labels, steps, t0, cls_preds, bbox_preds, return_rows):
        from . import _hip
        dev = anchors.device
        anchors = anchors.detach().contiguous().float()
        labels = labels.detach().to(dev).contiguous().float()
        cls_preds = cls_preds.detach().contiguous().float()
        bbox_preds = bbox_preds.detach().contiguous().float()
        B, N, cols = labels.shape
        A, C = anchors.shape[0], cls_preds.shape[-1]
        K = 1 if steps is None else int(steps.shape[0])
        lead = (B,) if steps is None else (K, B)
        if cols != (5 if steps is None else 6):
            raise RuntimeError(f"TaskAlignedAssigner: labels with {cols} columns where {5 if steps is None else 6} are required")
        if not cls_preds.is_cuda or not bbox_preds.is_cuda or tuple(cls_preds.shape) != lead + (A, C) \
                or tuple(bbox_preds.shape) != lead + (A, 4):
            raise RuntimeError(f"TaskAlignedAssigner: predictions must be device tensors {lead + (A, 'C')} / "
                               f"{lead + (A, 4)}, got {tuple(cls_preds.shape)} / {tuple(bbox_preds.shape)}")
        offset = torch.empty(lead + (A, 4), device=dev, dtype=torch.float32)
        mask = torch.empty(lead + (A, 4), device=dev, dtype=torch.float32)
        cls = torch.empty(lead + (A,), device=dev, dtype=torch.int64)
        rows = torch.empty(lead + (A,), device=dev, dtype=torch.int32) if return_rows else None
        if N == 0:   # no rows at all: nothing is a positive
            offset.zero_(), mask.zero_(), cls.zero_()
            if return_rows:
                rows.fill_(-1)
        else:
            ws = torch.empty(_hip.query("snn_tal_workspace_size", K * B, A, N, self.topk), device=dev, dtype=torch.uint8)
            _hip.call("snn_tal_assign", anchors.data_ptr(), labels.data_ptr(), None if steps is None else steps.data_ptr(),
                      cls_preds.data_ptr(), bbox_preds.data_ptr(), K, B, A, N, C, t0, self.topk, self.alpha, self.beta,
                      ws.data_ptr(), offset.data_ptr(), mask.data_ptr(), cls.data_ptr(),
                      None if rows is None else rows.data_ptr(), torch.cuda.current_stream().cuda_stream)
        return (offset, mask, cls, rows) if return_rows else (offset, mask, cls)

    def _assign(self, anchors: torch.Tensor, label: torch.Tensor, cls: torch.Tensor, bb: torch.Tensor) -> torch.Tensor:
        """The label row of every anchor of ONE sample (-1 = background): ``label[N,5]``, ``cls[A,C+1]``, ``bb[A,4]``."""
        A, N, C = anchors.shape[0], label.shape[0], cls.shape[1]
        if N == 0:
            return torch.full((A,), -1, dtype=torch.long)
        c, gt = label[:, 0], label[:, 1:]
        part = (c >= 0) & (c + 1 < C) & (gt[:, 2] > gt[:, 0]) & (gt[:, 3] > gt[:, 1])            # [N]
        col = torch.where(part, c.long() + 1, torch.zeros_like(c, dtype=torch.long))
        # decoded predictions: offset_inverse with the exponent argument replaced by the clamp where it is not <= it
        anc = box.box_corner_to_center(anchors)
        e = bb[:, 2:] / 5
        wh = torch.exp(torch.where(e <= _EXP_CLAMP, e, torch.full_like(e, _EXP_CLAMP))) * anc[:, 2:]
        xy = (bb[:, :2] * anc[:, 2:] / 10) + anc[:, :2]
        p = box.box_center_to_corner(torch.cat((xy, wh), dim=1))
        zero = torch.zeros((), dtype=torch.float32)
        s = torch.softmax(cls, dim=1)[:, col]                                                  # [A, N]
        s = torch.where(s > 0, s, zero)
        ap = (p[:, 2] - p[:, 0]) * (p[:, 3] - p[:, 1])
        ag = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1])
        iw = torch.clamp(torch.minimum(p[:, None, 2], gt[:, 2]) - torch.maximum(p[:, None, 0], gt[:, 0]), min=0)
        ih = torch.clamp(torch.minimum(p[:, None, 3], gt[:, 3]) - torch.maximum(p[:, None, 1], gt[:, 1]), min=0)
        inter = iw * ih
        u = inter / ((ap[:, None] + ag - inter) + _IOU_EPS)
        u = torch.where(u > 0, u, zero)
        inside = (anc[:, None, 0] > gt[:, 0]) & (anc[:, None, 0] < gt[:, 2]) & (anc[:, None, 1] > gt[:, 1]) \
            & (anc[:, None, 1] < gt[:, 3])
        cand = inside & part
        t = torch.pow(s, self.alpha) * torch.pow(u, self.beta)
        t = torch.where(cand, torch.where(t > 0, t, zero), torch.full((), -1.0))
        # per row the topk candidates: a stable descending sort keeps the lower anchor on ties
        k = min(self.topk, A)
        val, idx = torch.sort(t, dim=0, descending=True, stable=True)
        selected = torch.zeros((A, N), dtype=torch.bool).scatter_(0, idx[:k], val[:k] >= 0)
        # conflicts: the row of largest overlap, the first (lowest) on ties
        best = torch.where(selected, u, torch.full((), -1.0)).max(dim=1)
        amap = torch.where(best.values >= 0, best.indices, torch.full((A,), -1, dtype=torch.long))
        # fall-back, in row order: a row left with no anchor claims the unassigned anchor of highest anchor IoU
        iou = box.box_iou(anchors, gt)
        every = torch.arange(A)
        for j in range(N):
            need = part[j] & ~(amap == j).any()
            v = torch.where((amap < 0) & (iou[:, j] == iou[:, j]), iou[:, j], torch.full((), -math.inf))
            a = torch.argmax(v)
            amap = torch.where((every == a) & need & (v[a] > -math.inf), torch.full_like(amap, j), amap)
        return amap
