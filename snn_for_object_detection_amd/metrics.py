"""COCO bounding-box mAP on the device (the reference's ``torchmetrics.detection.MeanAveragePrecision``, models/soda.py:89-96,
283-321).

``MeanAveragePrecision`` restates COCOeval for ``iou_type="bbox"``, area range "all" and no crowd boxes; the arithmetic runs
in the HIP kernels of ``csrc/metrics.hip`` and torch is plumbing (device sorts, concatenation):

1. Detections are rows ``(class, score, x1, y1, x2, y2)`` (``box.multibox_detection``), ground truth rows
   ``(class, x1, y1, x2, y2)``; rows with ``class < 0`` are padding.  Boxes are not clamped.
2. Per (image, class) the detections are sorted by score, descending and stably, and cut to the largest maxDet (100)
   BEFORE matching.
3. IoU is pycocotools' ``bbIou`` in fp64 on ``w = fl32(x2 - x1)``, ``h = fl32(y2 - y1)`` (torchmetrics forms xywh in
   fp32), bit for bit.
4. At each IoU threshold ``t`` the detections, in score order, take the still-free ground truth of largest IoU
   ``>= min(t, 1 - 1e-10)``; equal IoU goes to the later ground-truth row.
5. Per class and maxDet the records of all images (update order, then batch index) are sorted stably by score;
   cumulative ``tp`` / ``fp`` give ``rc = tp / npig`` and ``pr = tp / (tp + fp + 2^-52)``; ``pr`` is made non-increasing
   from the right and read at ``searchsorted_left(rc, r)`` for every recall threshold ``r`` (0 past the end).  A class
   without ground truth is left out of every mean.
6. ``map`` / ``map_50`` / ``map_75`` average the interpolated precision at the largest maxDet, ``mar_<m>`` the recall
   at maxDet ``m``; fp64 throughout, rounded once to fp32; -1 where no class is valid.

``update_padded`` is what ``SODa`` calls: fixed shapes, no host synchronisation.  ``compute`` synchronises once (it
raises on class ids outside ``[0, num_classes)``, which ``update*`` count on the device).  As in the reference
(``sync_on_compute=False``) each process's result covers the images that process saw; there is no cross-rank gather.
"""

from typing import Dict, List, Optional, Sequence

import torch

MAX_GT_ROWS = 2048       # ground-truth rows per image the match kernel takes (64 lanes x 32 "taken" bits)
MAX_DETECTIONS = 1024    # largest maxDet (detection slots per image and class)
MAX_IOU_THRESHOLDS = 31  # bits of a slot's match mask
MAX_REC_THRESHOLDS = 1024


def _require_device(t: torch.Tensor, what: str) -> None:
    if not t.is_cuda:
        raise RuntimeError(f"MeanAveragePrecision.{what}: tensor is on {t.device}; the MI355X path has no CPU fallback "
                           "(move the predictions and targets to a HIP device)")


class MeanAveragePrecision:
    """COCO mAP for ``box_format="xyxy"``, ``iou_type="bbox"``; constructor arguments carry torchmetrics' names and
    defaults.  Not an ``nn.Module``: a model holding one keeps its ``state_dict`` unchanged.

    The default tables are torchmetrics': ``torch.linspace(0.5, 0.95, 10).tolist()`` and
    ``torch.linspace(0.0, 1.0, 101).tolist()`` - fp32 linspace values (0.55 is 0.550000011920929), not numpy's."""

    def __init__(self, num_classes: int, iou_thresholds: Optional[Sequence[float]] = None,
                 rec_thresholds: Optional[Sequence[float]] = None,
                 max_detection_thresholds: Optional[Sequence[int]] = None):
        self.num_classes = int(num_classes)
        self.iou_thresholds = [float(t) for t in iou_thresholds] if iou_thresholds else \
            torch.linspace(0.5, 0.95, round((0.95 - 0.5) / 0.05) + 1).tolist()
        self.rec_thresholds = [float(r) for r in rec_thresholds] if rec_thresholds else \
            torch.linspace(0.0, 1.00, round(1.00 / 0.01) + 1).tolist()
        self.max_detection_thresholds = sorted(int(m) for m in (max_detection_thresholds or [1, 10, 100]))
        if self.num_classes < 1:
            raise ValueError("MeanAveragePrecision: num_classes must be >= 1")
        if not 1 <= len(self.iou_thresholds) <= MAX_IOU_THRESHOLDS:
            raise ValueError(f"MeanAveragePrecision: 1 to {MAX_IOU_THRESHOLDS} IoU thresholds are supported")
        if not 1 <= len(self.rec_thresholds) <= MAX_REC_THRESHOLDS:
            raise ValueError(f"MeanAveragePrecision: 1 to {MAX_REC_THRESHOLDS} recall thresholds are supported")
        if self.rec_thresholds != sorted(self.rec_thresholds):
            raise ValueError("MeanAveragePrecision: rec_thresholds must be ascending")
        if not 1 <= self.max_detection_thresholds[0] or self.max_detection_thresholds[-1] > MAX_DETECTIONS:
            raise ValueError(f"MeanAveragePrecision: max_detection_thresholds must lie in 1..{MAX_DETECTIONS}")
        self._tables = {}
        self.reset()

    # ------------------------------------------------------------------ state
    def reset(self) -> None:
        self._scores: List[torch.Tensor] = []   # [B, C, S] per update: score of each kept detection (-inf: empty)
        self._masks: List[torch.Tensor] = []    # [B, C, S] int32: bit 31 used, bit t matched at IoU threshold t
        self._npig: Optional[torch.Tensor] = None   # [C] int32 ground-truth count per class
        self._bad: Optional[torch.Tensor] = None    # int64: class ids >= num_classes seen
        self._device: Optional[torch.device] = None

    def _state(self, dev: torch.device):
        if self._device is None:
            self._device = dev
            self._npig = torch.zeros(self.num_classes, device=dev, dtype=torch.int32)
            self._bad = torch.zeros((), device=dev, dtype=torch.int64)
        elif dev != self._device:
            raise RuntimeError(f"MeanAveragePrecision: inputs on {dev}, state on {self._device}")
        if dev not in self._tables:
            def table(values, dtype):   # pinned source, asynchronous copy: the first update does not synchronise either
                return torch.tensor(values, dtype=dtype).pin_memory().to(dev, non_blocking=True)
            self._tables[dev] = (table(self.iou_thresholds, torch.float64), table(self.rec_thresholds, torch.float64),
                                 table(self.max_detection_thresholds, torch.int32),
                                 torch.arange(self.num_classes + 1, device=dev, dtype=torch.int32))
        return self._tables[dev]

    # ------------------------------------------------------------------ update
    def update_padded(self, dets: torch.Tensor, labels: torch.Tensor) -> None:
        """One batch: ``dets[B, A, 6]`` rows ``(class, score, x1, y1, x2, y2)`` and ``labels[B, G, 5]`` rows
        ``(class, x1, y1, x2, y2)``, class < 0 = padding.  No host synchronisation."""
        from . import _hip
        _require_device(dets, "update_padded")
        _require_device(labels, "update_padded")
        if dets.dim() != 3 or dets.shape[2] != 6 or labels.dim() != 3 or labels.shape[2] != 5 \
                or dets.shape[0] != labels.shape[0]:
            raise ValueError(f"MeanAveragePrecision.update_padded: expected dets [B, A, 6] and labels [B, G, 5], got "
                             f"{tuple(dets.shape)} and {tuple(labels.shape)}")
        B, A, G = dets.shape[0], dets.shape[1], labels.shape[1]
        if G > MAX_GT_ROWS:
            raise ValueError(f"MeanAveragePrecision: {G} ground-truth rows per image exceed the limit of {MAX_GT_ROWS}")
        if B == 0:
            return
        dev = dets.device
        iou_t, _, _, classes = self._state(dev)
        dets = dets.detach().float()
        labels = labels.detach().float()
        if A == 0:
            dets = torch.full((B, 1, 6), -1.0, device=dev)
            A = 1
        if G == 0:
            labels = torch.full((B, 1, 5), -1.0, device=dev)
            G = 1
        dets, labels = dets.contiguous(), labels.contiguous()
        C, S = self.num_classes, self.max_detection_thresholds[-1]
        cls = dets[..., 0]
        # class key: 0..C-1, C = out of range (counted), C + 1 = padding; both sort behind every valid class
        key = torch.where(cls < 0, C + 1, cls.clamp(max=C).to(torch.int32))
        self._bad += (key == C).sum() + (labels[..., 0] >= C).sum()
        # (class ascending, score descending, row ascending): two stable device sorts
        by_score = torch.sort(dets[..., 1], dim=1, descending=True, stable=True).indices
        key_sorted, by_class = torch.sort(key.gather(1, by_score), dim=1, stable=True)
        order = by_score.gather(1, by_class).to(torch.int32).contiguous()
        seg = torch.searchsorted(key_sorted.contiguous(), classes.expand(B, C + 1).contiguous()).to(torch.int32)
        score = torch.empty(B, C, S, device=dev, dtype=torch.float32)
        mask = torch.empty(B, C, S, device=dev, dtype=torch.int32)
        _hip.call("snn_map_match", dets.data_ptr(), labels.data_ptr(), order.data_ptr(), seg.contiguous().data_ptr(),
                  B, A, G, C, S, iou_t.data_ptr(), len(self.iou_thresholds), score.data_ptr(), mask.data_ptr(),
                  self._npig.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        self._scores.append(score)
        self._masks.append(mask)

    def update(self, preds: List[Dict[str, torch.Tensor]], target: List[Dict[str, torch.Tensor]]) -> None:
        """torchmetrics' form: ``preds[i] = {"boxes": [n, 4], "scores": [n], "labels": [n]}``,
        ``target[i] = {"boxes": [g, 4], "labels": [g]}``; padded and handed to ``update_padded``."""
        if len(preds) != len(target):
            raise ValueError("MeanAveragePrecision.update: preds and target differ in length")
        if not preds:
            return
        for p, t in zip(preds, target):
            for name, v in (("boxes", p["boxes"]), ("scores", p["scores"]), ("labels", p["labels"]),
                            ("boxes", t["boxes"]), ("labels", t["labels"])):
                _require_device(v, f"update ({name})")
        dev = preds[0]["boxes"].device
        B = len(preds)
        A = max(1, max(p["boxes"].shape[0] for p in preds))
        G = max(1, max(t["boxes"].shape[0] for t in target))
        dets = torch.full((B, A, 6), -1.0, device=dev)
        labels = torch.full((B, G, 5), -1.0, device=dev)
        for b, (p, t) in enumerate(zip(preds, target)):
            n, g = p["boxes"].shape[0], t["boxes"].shape[0]
            dets[b, :n, 0] = p["labels"].float()
            dets[b, :n, 1] = p["scores"].float()
            dets[b, :n, 2:] = p["boxes"].float()
            labels[b, :g, 0] = t["labels"].float()
            labels[b, :g, 1:] = t["boxes"].float()
        self.update_padded(dets, labels)

    # ------------------------------------------------------------------ compute
    def compute(self) -> Dict[str, torch.Tensor]:
        """``{map, map_50, map_75, mar_<m> for each maxDet m}`` as fp32 0-dim device tensors."""
        from . import _hip
        keys = ["map", "map_50", "map_75"] + [f"mar_{m}" for m in self.max_detection_thresholds]
        if not self._scores:
            dev = self._device or torch.device("cuda", torch.cuda.current_device())
            return {k: torch.full((), -1.0, device=dev) for k in keys}
        bad = int(self._bad)
        if bad:
            raise ValueError(f"MeanAveragePrecision: {bad} class ids outside [0, {self.num_classes})")
        dev = self._device
        _, rec_t, max_dets, _ = self._state(dev)
        C, S, M, T = self.num_classes, self.max_detection_thresholds[-1], len(self.max_detection_thresholds), \
            len(self.iou_thresholds)
        scores = torch.cat(self._scores)                 # [images, C, S]
        N = scores.shape[0] * S
        if N >= 2 ** 31:
            raise ValueError(f"MeanAveragePrecision: {N} records per class exceed the 32-bit index of the kernels")
        scores = scores.permute(1, 0, 2).reshape(C, N)
        masks = torch.cat(self._masks).permute(1, 0, 2).reshape(C, N).contiguous()
        order = torch.sort(scores, dim=1, descending=True, stable=True).indices.to(torch.int32).contiguous()
        ws = torch.empty(_hip.query("snn_map_workspace_size", C, M, T), device=dev, dtype=torch.uint8)
        out = torch.empty(3 + M, device=dev, dtype=torch.float32)
        t50 = next((i for i, t in enumerate(self.iou_thresholds) if t == 0.5), -1)
        t75 = next((i for i, t in enumerate(self.iou_thresholds) if t == 0.75), -1)
        _hip.call("snn_map_accumulate", order.data_ptr(), masks.data_ptr(), self._npig.data_ptr(), C, N, S,
                  max_dets.data_ptr(), M, rec_t.data_ptr(), len(self.rec_thresholds), T, t50, t75, ws.data_ptr(),
                  out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        return {k: out[i] for i, k in enumerate(keys)}
