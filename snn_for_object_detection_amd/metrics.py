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
(``sync_on_compute=False``) each process's result covers the images that process saw, unless ``sync_on_compute=True``
asks for the cross-rank result (option D).

Options beyond the reference's six scalars, all off by default (then exactly the launches and keys above):

A. Area ranges (``area_ranges=True``, COCOeval's small / medium / large).  With ``image_size = (H, W)`` a row's pixel
   width is ``wp = (double)fl32(x2 - x1) * W``, its height ``hp = (double)fl32(y2 - y1) * H``, its area ``wp * hp`` in
   fp64 (the reference's boxes are normalised, so torchmetrics files every one of them under "small").  Ranges are
   ``small [0, 32^2]``, ``medium [32^2, 96^2]``, ``large [96^2, 1e10]``; a row is outside when ``area < lo or area > hi``
   (both ends inclusive: an area of exactly 1024 is small and medium).  Per range a ground-truth row outside it is
   *ignored* and ``npig`` counts the others; a detection takes the free NON-IGNORED row by rule 4 and looks among the free
   ignored rows (same rule, ties to the later row) only when no non-ignored row qualifies, so a qualifying non-ignored row
   wins over a better-overlapping ignored one.  A detection matched to an ignored row, or unmatched with its own area
   outside the range, is ignored: neither tp nor fp, though it keeps its slot among an image's first maxDet.  Adds
   ``map_<range>`` / ``mar_<range>`` at the largest maxDet (torchmetrics' names); a class with ``npig == 0`` in a range
   is left out of that range's means.  "all" stays rules 1-6 with NO area test - real COCOeval applies ``[0, 1e10]`` to
   "all" as well, which differs only for a box with a negative side (negative or > 1e10 area).
B. Per-class output (``class_metrics=True``): ``map_per_class`` (a class's mean over IoU x recall thresholds at the
   largest maxDet) and ``mar_<largest maxDet>_per_class`` for "all", ``[C]`` fp32, -1 for a class without ground truth;
   ``classes`` is ``arange(C)`` int32.
C. Size filter (``min_box_diag = D`` and / or ``min_box_side = s`` in pixels, each active only when > 0): a row with
   ``wp^2 + hp^2 < D^2``, ``wp < s`` or ``hp < s`` is removed, detections and ground truth alike, before the (class,
   score) sort and the cut to the largest maxDet; a removed row behaves exactly like padding, in "all" as well.  This is
   the shape of the Prophesee evaluation protocol's filter; its constants are NOT shipped (protocol unpinned).
D. ``sync_on_compute=True``: ``compute()`` is collective over ``process_group``; the ranks' records are gathered and
   evaluated in rank order, then update order, so every rank returns the bits of one metric fed rank 0's images, then
   rank 1's, ...  A rank without an update takes part.  ``reset()`` stays local.  Without an initialised process group
   the result is the local one.
"""

from typing import Dict, List, Optional, Sequence, Tuple

import torch

MAX_GT_ROWS = 2048       # ground-truth rows per image the match kernel takes (64 lanes x 32 "taken" bits)
MAX_DETECTIONS = 1024    # largest maxDet (detection slots per image and class)
MAX_IOU_THRESHOLDS = 31  # bits of a slot's match mask
MAX_REC_THRESHOLDS = 1024
AREA_RANGES = ("small", "medium", "large")


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
                 max_detection_thresholds: Optional[Sequence[int]] = None, class_metrics: bool = False,
                 area_ranges: bool = False, image_size: Optional[Sequence[int]] = None, min_box_diag: float = 0.0,
                 min_box_side: float = 0.0, sync_on_compute: bool = False, process_group=None):
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
        self.class_metrics, self.area_ranges = bool(class_metrics), bool(area_ranges)
        self.image_size = self._image_size(image_size)
        self.min_box_diag, self.min_box_side = float(min_box_diag), float(min_box_side)
        if not (self.min_box_diag >= 0.0 and self.min_box_side >= 0.0):
            raise ValueError("MeanAveragePrecision: min_box_diag and min_box_side must be >= 0 (0: off)")
        self.sync_on_compute, self.process_group = bool(sync_on_compute), process_group
        # rows go through the filter kernel and the match kernel with areas only when a range or a limit asks for it
        self._pixels = self.area_ranges or self.min_box_diag > 0.0 or self.min_box_side > 0.0
        self._ranges = len(AREA_RANGES) if self.area_ranges else 0
        self._tables = {}
        self.reset()

    @staticmethod
    def _image_size(image_size) -> Optional[Tuple[float, float]]:
        if image_size is None:
            return None
        h, w = (float(v) for v in image_size)
        if not (h > 0.0 and w > 0.0):
            raise ValueError(f"MeanAveragePrecision: image_size must be positive (H, W), got {tuple(image_size)}")
        return h, w

    # ------------------------------------------------------------------ state
    def reset(self) -> None:
        self._scores: List[torch.Tensor] = []   # [B, C, S] per update: score of each kept detection (-inf: empty)
        self._masks: List[torch.Tensor] = []    # [B, C, S] int32: bit 31 used, bit t matched at IoU threshold t
        self._area_matched: List[torch.Tensor] = []   # [B, C, 3, S] int32 (area_ranges): bit t matched at threshold t
        self._area_ignored: List[torch.Tensor] = []   # ... bit t: ignored at threshold t (neither tp nor fp)
        self._npig: Optional[torch.Tensor] = None   # [C] int32 ground-truth count per class
        self._npig_area: Optional[torch.Tensor] = None   # [3, C] int32 (area_ranges): the non-ignored rows per range
        self._bad: Optional[torch.Tensor] = None    # int64: class ids >= num_classes seen
        self._device: Optional[torch.device] = None

    def _state(self, dev: torch.device):
        if self._device is None:
            self._device = dev
            self._npig = torch.zeros(self.num_classes, device=dev, dtype=torch.int32)
            self._npig_area = torch.zeros(self._ranges, self.num_classes, device=dev, dtype=torch.int32)
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
    def update_padded(self, dets: torch.Tensor, labels: torch.Tensor,
                      image_size: Optional[Sequence[int]] = None) -> None:
        """One batch: ``dets[B, A, 6]`` rows ``(class, score, x1, y1, x2, y2)`` and ``labels[B, G, 5]`` rows
        ``(class, x1, y1, x2, y2)``, class < 0 = padding.  ``image_size = (H, W)`` of this batch overrides the
        constructor's (read only by the area ranges and the size filter).  No host synchronisation."""
        from . import _hip
        size = self._image_size(image_size) or self.image_size
        if self._pixels and size is None:
            raise ValueError("MeanAveragePrecision: area_ranges, min_box_diag and min_box_side measure boxes in pixels "
                             "and need image_size = (H, W), in the constructor or in update_padded")
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
        stream = torch.cuda.current_stream(dev).cuda_stream
        # class key: 0..C-1, C = out of range (counted), C + 1 = padding; both sort behind every valid class
        if self._pixels:   # ... or removed by the size filter: the kernel forms the key and the labels' class column
            key = torch.empty(B, A, device=dev, dtype=torch.int32)
            label_cls = torch.empty(B, G, device=dev, dtype=torch.float32)
            _hip.call("snn_map_filter_rows", dets.data_ptr(), labels.data_ptr(), B, A, G, C, size[0], size[1],
                      self.min_box_diag, self.min_box_side, key.data_ptr(), label_cls.data_ptr(), self._bad.data_ptr(),
                      stream)
        else:
            cls = dets[..., 0]
            key = torch.where(cls < 0, C + 1, cls.clamp(max=C).to(torch.int32))
            self._bad += (key == C).sum() + (labels[..., 0] >= C).sum()
        # (class ascending, score descending, row ascending): two stable device sorts
        by_score = torch.sort(dets[..., 1], dim=1, descending=True, stable=True).indices
        key_sorted, by_class = torch.sort(key.gather(1, by_score), dim=1, stable=True)
        order = by_score.gather(1, by_class).to(torch.int32).contiguous()
        seg = torch.searchsorted(key_sorted.contiguous(), classes.expand(B, C + 1).contiguous()).to(torch.int32)
        score = torch.empty(B, C, S, device=dev, dtype=torch.float32)
        mask = torch.empty(B, C, S, device=dev, dtype=torch.int32)
        seg = seg.contiguous()
        if self._pixels:
            R = self._ranges
            matched = torch.empty(B, C, R, S, device=dev, dtype=torch.int32)
            ignored = torch.empty(B, C, R, S, device=dev, dtype=torch.int32)
            _hip.call("snn_map_match_areas", dets.data_ptr(), labels.data_ptr(), label_cls.data_ptr(), order.data_ptr(),
                      seg.data_ptr(), B, A, G, C, S, iou_t.data_ptr(), len(self.iou_thresholds), size[0], size[1], R,
                      score.data_ptr(), mask.data_ptr(), matched.data_ptr() if R else None,
                      ignored.data_ptr() if R else None, self._npig.data_ptr(),
                      self._npig_area.data_ptr() if R else None, stream)
            if R:
                self._area_matched.append(matched)
                self._area_ignored.append(ignored)
        else:
            _hip.call("snn_map_match", dets.data_ptr(), labels.data_ptr(), order.data_ptr(), seg.data_ptr(),
                      B, A, G, C, S, iou_t.data_ptr(), len(self.iou_thresholds), score.data_ptr(), mask.data_ptr(),
                      self._npig.data_ptr(), stream)
        self._scores.append(score)
        self._masks.append(mask)

    def update(self, preds: List[Dict[str, torch.Tensor]], target: List[Dict[str, torch.Tensor]],
               image_size: Optional[Sequence[int]] = None) -> None:
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
        self.update_padded(dets, labels, image_size=image_size)

    # ------------------------------------------------------------------ compute
    def _keys(self) -> List[str]:
        keys = ["map", "map_50", "map_75"] + [f"mar_{m}" for m in self.max_detection_thresholds]
        for name in AREA_RANGES[:self._ranges]:
            keys += [f"map_{name}", f"mar_{name}"]
        return keys

    def _empty(self, dev: torch.device) -> Dict[str, torch.Tensor]:
        out = {k: torch.full((), -1.0, device=dev) for k in self._keys()}
        if self.class_metrics:
            out["map_per_class"] = torch.full((self.num_classes,), -1.0, device=dev)
            out[f"mar_{self.max_detection_thresholds[-1]}_per_class"] = torch.full((self.num_classes,), -1.0, device=dev)
            out["classes"] = torch.arange(self.num_classes, device=dev, dtype=torch.int32)
        return out

    def _records(self, dev: torch.device) -> torch.Tensor:
        """This process's records as one int32 tensor ``[images, C, 2 + 2 * ranges, S]``: score bits, "all" mask, then
        the ranges' matched and ignored masks."""
        C, S, R = self.num_classes, self.max_detection_thresholds[-1], self._ranges
        if not self._scores:
            return torch.empty(0, C, 2 + 2 * R, S, device=dev, dtype=torch.int32)
        parts = [torch.cat(self._scores).view(torch.int32).unsqueeze(2), torch.cat(self._masks).unsqueeze(2)]
        if R:
            parts += [torch.cat(self._area_matched), torch.cat(self._area_ignored)]
        return torch.cat(parts, dim=2)

    def _gather(self, dev: torch.device):
        """The records of every rank in rank order (padded to the largest image count for the exchange, trimmed after
        it) and the summed counters.  A backend that cannot gather device tensors is served through the host."""
        import torch.distributed as dist
        group = self.process_group
        world = dist.get_world_size(group)
        via = dev if dist.get_backend(group) == "nccl" else torch.device("cpu")
        C, R = self.num_classes, self._ranges
        local = self._records(dev)
        counts = [torch.zeros(1, dtype=torch.int64, device=via) for _ in range(world)]
        dist.all_gather(counts, torch.tensor([local.shape[0]], dtype=torch.int64, device=via), group=group)
        counts = [int(n) for n in counts]
        padded = torch.zeros((max(counts),) + tuple(local.shape[1:]), dtype=torch.int32, device=via)
        padded[:local.shape[0]] = local.to(via)
        parts = [torch.empty_like(padded) for _ in range(world)]
        dist.all_gather(parts, padded, group=group)
        records = torch.cat([p[:n] for p, n in zip(parts, counts)]).to(dev)
        tally = torch.zeros((1 + R) * C + 1, dtype=torch.int64, device=via)
        if self._device is not None:
            tally[:C] = self._npig.to(via)
            tally[C:-1] = self._npig_area.reshape(-1).to(via)
            tally[-1] = self._bad.to(via)
        dist.all_reduce(tally, op=dist.ReduceOp.SUM, group=group)
        tally = tally.to(dev)
        return records, tally[:C].to(torch.int32), tally[C:-1].to(torch.int32).reshape(R, C).contiguous(), tally[-1]

    def compute(self) -> Dict[str, torch.Tensor]:
        """``{map, map_50, map_75, mar_<m> for each maxDet m}`` as fp32 0-dim device tensors; with ``area_ranges`` also
        ``map_<range>`` / ``mar_<range>``, with ``class_metrics`` ``map_per_class``, ``mar_<largest maxDet>_per_class``
        (``[C]`` fp32) and ``classes`` (``[C]`` int32)."""
        from . import _hip
        dev = self._device or torch.device("cuda", torch.cuda.current_device())
        C, S, M, T, R = self.num_classes, self.max_detection_thresholds[-1], len(self.max_detection_thresholds), \
            len(self.iou_thresholds), self._ranges
        import torch.distributed as dist
        if self.sync_on_compute and dist.is_available() and dist.is_initialized():
            records, npig, npig_area, bad = self._gather(dev)
            if records.shape[0] == 0:
                return self._empty(dev)
            scores, masks = records[:, :, 0].contiguous().view(torch.float32), records[:, :, 1]
            matched, ignored = records[:, :, 2:2 + R], records[:, :, 2 + R:]
        else:
            if not self._scores:
                return self._empty(dev)
            npig, npig_area, bad = self._npig, self._npig_area, self._bad
            scores, masks = torch.cat(self._scores), torch.cat(self._masks)      # [images, C, S]
            if R:
                matched, ignored = torch.cat(self._area_matched), torch.cat(self._area_ignored)
        bad = int(bad)
        if bad:
            raise ValueError(f"MeanAveragePrecision: {bad} class ids outside [0, {self.num_classes})")
        _, rec_t, max_dets, _ = self._state(dev)
        N = scores.shape[0] * S
        if N >= 2 ** 31:
            raise ValueError(f"MeanAveragePrecision: {N} records per class exceed the 32-bit index of the kernels")
        scores = scores.permute(1, 0, 2).reshape(C, N)
        masks = masks.permute(1, 0, 2).reshape(C, N).contiguous()
        order = torch.sort(scores, dim=1, descending=True, stable=True).indices.to(torch.int32).contiguous()
        t50 = next((i for i, t in enumerate(self.iou_thresholds) if t == 0.5), -1)
        t75 = next((i for i, t in enumerate(self.iou_thresholds) if t == 0.75), -1)
        stream = torch.cuda.current_stream(dev).cuda_stream
        keys = self._keys()
        out = torch.empty(len(keys), device=dev, dtype=torch.float32)
        if not (R or self.class_metrics):
            ws = torch.empty(_hip.query("snn_map_workspace_size", C, M, T), device=dev, dtype=torch.uint8)
            _hip.call("snn_map_accumulate", order.data_ptr(), masks.data_ptr(), npig.data_ptr(), C, N, S,
                      max_dets.data_ptr(), M, rec_t.data_ptr(), len(self.rec_thresholds), T, t50, t75, ws.data_ptr(),
                      out.data_ptr(), stream)
            return {k: out[i] for i, k in enumerate(keys)}
        if R:   # [images, C, 3, S] -> [C, 3, records]
            matched = matched.permute(1, 2, 0, 3).reshape(C, R, N).contiguous()
            ignored = ignored.permute(1, 2, 0, 3).reshape(C, R, N).contiguous()
        per_class = torch.empty(2, C, device=dev, dtype=torch.float32) if self.class_metrics else None
        ws = torch.empty(_hip.query("snn_map_areas_workspace_size", C, M, T, R), device=dev, dtype=torch.uint8)
        _hip.call("snn_map_accumulate_areas", order.data_ptr(), masks.data_ptr(), matched.data_ptr() if R else None,
                  ignored.data_ptr() if R else None, npig.data_ptr(), npig_area.data_ptr() if R else None, C, N, S,
                  max_dets.data_ptr(), M, rec_t.data_ptr(), len(self.rec_thresholds), T, t50, t75, R, ws.data_ptr(),
                  out.data_ptr(), per_class.data_ptr() if self.class_metrics else None, stream)
        result = {k: out[i] for i, k in enumerate(keys)}
        if self.class_metrics:
            result["map_per_class"] = per_class[0]
            result[f"mar_{self.max_detection_thresholds[-1]}_per_class"] = per_class[1]
            result["classes"] = torch.arange(C, device=dev, dtype=torch.int32)
        return result
