"""Prophesee recordings as the feed of the detector: DAT files, their ``*_bbox.npy`` labels, the reference's sample
decisions and an endless batch iterator - all on the host, with NOTHING decoded there.

A DAT record is 8 bytes, ``uint32 ts_us, uint32 data`` with ``x = data & 0x3FFF``, ``y = (data >> 14) & 0x3FFF``,
``p = (data >> 28) & 1``.  ``DatRecording`` memory-maps the records as ``uint32 [n, 2]``; a sample is a SLICE of that map,
found by binary search on the timestamp column, and ``EventBatcher`` copies the slice into pinned memory and lets
``snn_events_to_frames_packed`` unpack the words on the GPU (8 bytes per event over PCIe, no host pass over the events).

FORMAT UNPINNED: the layout above is written from Prophesee's public description of the DAT format; the toolbox that
holds the reader the reference uses (``PSEELoader``) is an un-fetched submodule of the reference, so no file written by
it has been read here.  What IS pinned (``tests/golden/events.npz``, ``tests/golden/boxes.npz``) are the decisions of
``STPropheseeDataset.parse_data`` / ``MTPropheseeDataset.parse_data`` and the label conversion ``_labels_prepare``.

The one place the samplers differ from the reference: a multi-target sample whose events have ``x >= W`` is clipped to
the last column by the scatter kernel, where the reference's indexing raises ``IndexError``.  Two more, in the feed: the
file cycle hands every file to a group (the reference's ``enumerate`` loop drops the file it breaks on), and shuffling
draws from the feed's own ``random.Random(seed)``, not from the global generator.
"""
import glob
import itertools
import os
import random
from typing import Iterator, List, Optional, Tuple

import numpy as np
import torch

Y_SHIFT, P_SHIFT, FIELD_MASK = 14, 28, 0x3FFF
EVENT_BYTES = 8
DAT_EVENT_TYPE_CD = 12
GEOMETRY = {"gen1": (240, 304), "1mpx": (720, 1280)}          # (height, width)
TIME_FIELD = {"gen1": "ts", "1mpx": "t"}
CLASS_NAMES = {"gen1": ["car", "person"],
               "1mpx": ["pedestrians", "two wheelers", "cars", "trucks", "buses", "signs", "traffic lights"]}
RECORD_TIME_US = 60_000_000


def _check_dataset(dataset: str) -> str:
    if dataset not in GEOMETRY:
        raise ValueError(f'The dataset parameter cannot be "{dataset}"! ("gen1" or "1mpx")')
    return dataset


def lower_bound(column, value: int, lo: int = 0, hi: Optional[int] = None) -> int:
    """First index in ``[lo, hi)`` whose entry is ``>= value`` (``hi`` when none is): a bisection that reads one entry
    per step, so a memory-mapped column is touched in ~log2(n) pages and never copied."""
    hi = len(column) if hi is None else hi
    value = int(value)
    while lo < hi:
        mid = (lo + hi) >> 1
        if int(column[mid]) < value:
            lo = mid + 1
        else:
            hi = mid
    return lo


# ---------------------------------------------------------------------------------------------- words
def pack_events(t, x, y, p) -> np.ndarray:
    """``(t_us, x, y, p)`` integer arrays -> DAT records ``uint32 [n, 2]``.  Values that do not fit their field raise."""
    t, x, y, p = (np.asarray(v).astype(np.int64).reshape(-1) for v in (t, x, y, p))
    if not (t.size == x.size == y.size == p.size):
        raise ValueError("pack_events: t, x, y, p must have the same length")
    for name, v, top in (("t", t, (1 << 32) - 1), ("x", x, FIELD_MASK), ("y", y, FIELD_MASK), ("p", p, 1)):
        if v.size and (int(v.min()) < 0 or int(v.max()) > top):
            raise ValueError(f"pack_events: {name} outside [0, {top}]")
    words = np.empty((t.size, 2), dtype=np.uint32)
    words[:, 0] = t
    words[:, 1] = x | (y << Y_SHIFT) | (p << P_SHIFT)
    return words


def unpack_events(words) -> Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]:
    """DAT records ``uint32 [n, 2]`` -> ``(t_us int64, x int32, y int32, p int32)``; bits 29-31 of the data word are
    ignored.  For conversion, tools and tests: the feed never calls it."""
    words = np.asarray(words)
    if words.ndim != 2 or words.shape[1] != 2 or words.dtype.itemsize != 4 or words.dtype.kind not in "ui":
        raise ValueError(f"unpack_events: uint32 [n, 2] required, got {words.dtype} {tuple(words.shape)}")
    words = words.view(np.uint32) if words.dtype != np.uint32 else words
    d = words[:, 1]
    return (words[:, 0].astype(np.int64), (d & FIELD_MASK).astype(np.int32),
            ((d >> Y_SHIFT) & FIELD_MASK).astype(np.int32), ((d >> P_SHIFT) & 1).astype(np.int32))


def write_dat(path: str, words, width: Optional[int] = None, height: Optional[int] = None) -> None:
    """Write records ``uint32 [n, 2]`` as a DAT file: ``%`` header lines (Width / Height when given), the event type and
    event size bytes, the little-endian records."""
    words = np.ascontiguousarray(np.asarray(words), dtype="<u4")
    if words.ndim != 2 or words.shape[1] != 2:
        raise ValueError(f"write_dat: uint32 [n, 2] required, got shape {tuple(words.shape)}")
    header = "% Data file containing CD events.\n% Version 2\n"
    if width is not None:
        header += f"% Width {int(width)}\n"
    if height is not None:
        header += f"% Height {int(height)}\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(bytes([DAT_EVENT_TYPE_CD, EVENT_BYTES]))
        f.write(words.tobytes())


class DatRecording:
    """A DAT file as a memory map of its records, with the three members the reference's ``parse_data`` methods use of
    their reader - ``current_time``, ``load_delta_t``, ``done`` - plus ``reset``, ``seek_time`` and ``total_time``.

    ``words`` is ``uint32 [n, 2]`` (``ts_us, data``), mapped read-only; ``width`` / ``height`` come from the header's
    ``% Width N`` / ``% Height N`` lines (``None`` when absent).  Timestamps must not decrease (recordings do not wrap:
    2^32 us is 71 minutes, the recordings are 60 s)."""

    def __init__(self, path: str):
        self.path = str(path)
        self.width = self.height = None
        with open(self.path, "rb") as f:
            while True:
                at = f.tell()
                first = f.read(1)
                if first != b"%":
                    f.seek(at)
                    break
                line = f.readline()
                fields = line.decode("ascii", errors="replace").split()
                if len(fields) >= 2 and fields[0] in ("Width", "Height"):
                    try:
                        setattr(self, fields[0].lower(), int(fields[1]))
                    except ValueError:
                        pass
            info = f.read(2)
            if len(info) < 2:
                raise ValueError(f"DatRecording: {self.path}: no event type / event size bytes after the header")
            self.event_type, self.event_size = info[0], info[1]
            if self.event_size != EVENT_BYTES:
                raise ValueError(f"DatRecording: {self.path}: event size {self.event_size} is not supported "
                                 f"({EVENT_BYTES}-byte records only)")
            start = f.tell()
        n = (os.path.getsize(self.path) - start) // EVENT_BYTES   # a trailing partial record is ignored
        if n:
            self.words = np.memmap(self.path, dtype="<u4", mode="r", offset=start, shape=(n, 2))
        else:
            self.words = np.zeros((0, 2), dtype=np.uint32)
        self._ts = self.words[:, 0]
        self.current_time = 0
        self._pos = 0

    def __len__(self) -> int:
        return int(self.words.shape[0])

    @property
    def done(self) -> bool:
        """True once every event has been passed."""
        return self._pos >= len(self)

    def reset(self) -> None:
        self.current_time, self._pos = 0, 0

    def seek_time(self, t_us: int) -> None:
        self.current_time = int(t_us)
        self._pos = lower_bound(self._ts, self.current_time)

    def total_time(self) -> int:
        """Timestamp of the last event (0 for an empty recording)."""
        return int(self._ts[-1]) if len(self) else 0

    def load_delta_t(self, delta_us: int) -> np.ndarray:
        """The events with ``current_time <= ts < current_time + delta_us`` as a zero-copy slice of ``words``; the clock
        advances by ``delta_us``."""
        end = self.current_time + int(delta_us)
        hi = lower_bound(self._ts, end, self._pos)
        out = self.words[self._pos:hi]
        self.current_time, self._pos = end, hi
        return out


# ---------------------------------------------------------------------------------------------- labels
def load_boxes(path, dataset: str, time_step_us: int) -> np.ndarray:
    """The structured ``*_bbox.npy`` of a recording (a path, or the array itself) -> ``float32 [n, 6]`` rows ``(step,
    class, x1, y1, x2, y2)`` with the boxes normalised to the frame: what the reference's ``_labels_prepare`` makes.
    ``step`` is the timestamp (field ``ts`` for gen1, ``t`` for 1mpx) floor-divided by ``time_step_us`` in integers and
    only then cast; the coordinates are divided in the precision of their fields (float32 in the datasets)."""
    height, width = GEOMETRY[_check_dataset(dataset)]
    boxes = np.load(path) if isinstance(path, (str, os.PathLike)) else np.asarray(path)
    out = np.empty((boxes.shape[0], 6), dtype=np.float32)
    out[:, 0] = boxes[TIME_FIELD[dataset]] // int(time_step_us)
    out[:, 1] = boxes["class_id"]
    out[:, 2] = boxes["x"] / width
    out[:, 3] = boxes["y"] / height
    out[:, 4] = (boxes["x"] + boxes["w"]) / width
    out[:, 5] = (boxes["y"] + boxes["h"]) / height
    return out


# ---------------------------------------------------------------------------------------------- samplers
class STSampler:
    """The decisions of ``STPropheseeDataset.parse_data`` (single-target training samples) on a ``DatRecording``:
    ``sampler(gt_boxes, recording) -> (sample or None, more)`` with ``sample = (words_slice, t0_us, labels[n, 5])``.

    The labels are the rows of the first labelled step at or after ``start_step + num_steps`` whose area exceeds
    ``box_size_threshold``; the recording is read up to ``label time + time_shift`` steps, the window starts ``num_steps``
    steps before that end; a window with fewer than ``events_threshold`` events per step on average is rejected (``None,
    True``).  The event count is the distance of two search positions - nothing is decoded."""

    def __init__(self, num_steps: int, time_shift: int, time_step_us: int, events_threshold: int = 4000,
                 box_size_threshold: float = 0.01):
        self.num_steps, self.time_shift, self.time_step_us = int(num_steps), int(time_shift), int(time_step_us)
        self.events_threshold, self.box_size_threshold = int(events_threshold), float(box_size_threshold)

    def __call__(self, gt_boxes: np.ndarray, rec: DatRecording):
        if rec.done:
            return None, False
        T, step = self.num_steps, self.time_step_us
        clock = rec.current_time
        start_step = clock // step
        gt = gt_boxes[gt_boxes[:, 0] >= start_step + T]
        if gt.size == 0:
            return None, False
        labels = gt[gt[:, 0] == gt[0, 0]]
        area = (labels[:, 4] - labels[:, 2]) * (labels[:, 5] - labels[:, 3])
        labels = labels[area > np.float32(self.box_size_threshold)]
        if labels.size == 0:
            return None, False
        label_us = int(labels[0, 0]) * step
        t0 = label_us - step * (T - self.time_shift)
        words = rec.load_delta_t(label_us + step * self.time_shift - clock)
        first = lower_bound(words[:, 0], t0)                   # events before the window are not part of the sample
        count = int(words.shape[0]) - first
        if count // T < self.events_threshold:
            return None, True
        if count == 0:
            return None, False
        return (words[first:], t0, labels[:, 1:]), True


class MTSampler:
    """The decisions of ``MTPropheseeDataset.parse_data`` (multi-target evaluation samples): ``sampler(gt_boxes,
    recording) -> (words_slice, t0_us, labels[n, 6])`` - the next ``num_steps`` steps of the recording (wrapping to its
    start once it is ``done``), the labels of those steps with their step made window-relative; no label when the window
    holds no event."""

    def __init__(self, num_steps: int, time_step_us: int):
        self.num_steps, self.time_step_us = int(num_steps), int(time_step_us)

    def __call__(self, gt_boxes: np.ndarray, rec: DatRecording):
        if rec.done:
            rec.reset()
        T, step = self.num_steps, self.time_step_us
        start_step = rec.current_time // step
        words = rec.load_delta_t(step * T)
        if words.shape[0] == 0:
            return words, start_step * step, gt_boxes[0:0]
        labels = gt_boxes[(gt_boxes[:, 0] >= start_step) & (gt_boxes[:, 0] < start_step + T)].copy()
        labels[:, 0] -= start_step
        return words, start_step * step, labels


# ---------------------------------------------------------------------------------------------- feed
class PropheseeFeed:
    """Endless iterator of device batches ``(X[T, B, 2, H, W], labels)`` from ``<data_dir>/<dataset>/<split>/*_bbox.npy``
    and their ``*_td.dat``, through ``EventBatcher``'s packed path.  The arguments are those of the reference's
    ``PropheseeDataModule`` (``time_step`` in milliseconds; ``files_in_flight`` is its ``num_load_file``); ``rank`` /
    ``world`` divide the files the way the reference divides them among DataLoader workers (``per = n // world``, slice
    ``rank``).  ``one_label=False`` yields 6-column labels for ``SODa(label_steps=K)``.  ``samples()`` is the host side
    alone (no device needed).  ``chained=True`` (with ``one_label=False``) binds every batch slot to one recording and
    yields its windows in time order, batches ``(X, labels, first)`` for ``SODa(carry_state=True)``
    (``_chained_samples``).  ``representation`` (a name or a ``data.EventRepresentation``) is handed to the batcher: what
    a cell of ``X`` holds; samples, labels and their order do not depend on it."""

    def __init__(self, data_dir: str, dataset: str = "gen1", split: str = "train", batch_size: int = 4,
                 num_steps: int = 42, time_step: int = 16, time_shift: int = 16, one_label: bool = True,
                 files_in_flight: int = 8, rank: int = 0, world: int = 1, seed: int = 0, device="cuda", augment=None,
                 events_threshold: int = 4000, box_size_threshold: float = 0.01, chained: bool = False,
                 representation="binary"):
        self.dataset = _check_dataset(dataset)
        if chained and one_label:
            raise ValueError("PropheseeFeed: chained=True needs one_label=False (consecutive windows carry the six-column "
                             "labels of SODa(label_steps=K); chained single-label windows are not built)")
        self.chained = bool(chained)
        if files_in_flight <= 0:
            raise ValueError("PropheseeFeed: files_in_flight must be more than zero")
        if batch_size <= 0 or num_steps <= 0 or time_step <= 0:
            raise ValueError("PropheseeFeed: batch_size, num_steps and time_step must be positive")
        if not 0 <= rank < world:
            raise ValueError(f"PropheseeFeed: rank {rank} outside [0, {world})")
        self.height, self.width = GEOMETRY[dataset]
        self.batch_size, self.num_steps, self.one_label = int(batch_size), int(num_steps), bool(one_label)
        self.time_step_us = int(time_step) * 1000
        from .data import EventRepresentation
        self.representation = EventRepresentation.of(representation, "PropheseeFeed")
        if not self.representation.is_binary:
            self.representation.check(self.time_step_us, "PropheseeFeed")
        self.files_in_flight, self.device, self.augment = int(files_in_flight), device, augment
        directory = os.path.join(data_dir, dataset, split)
        gt_files = sorted(glob.glob(os.path.join(directory, "*_bbox.npy")))
        data_files = [p[:-len("_bbox.npy")] + "_td.dat" for p in gt_files]
        missing = [p for p in data_files if not os.path.exists(p)]
        if not gt_files or missing:
            raise RuntimeError(f"Directory '{directory}' does not contain data or data is invalid: expecting "
                               f"{directory}/*_bbox.npy, each with its *_td.dat"
                               + (f" (missing {missing[0]})" if missing else "")
                               + ". The datasets are Prophesee's GEN1 automotive detection dataset and 1 megapixel "
                                 "automotive detection dataset.")
        per = len(gt_files) // int(world)
        if per == 0:
            raise RuntimeError(f"PropheseeFeed: {len(gt_files)} recordings in '{directory}' are fewer than {world} ranks")
        self.files: List[Tuple[str, str]] = list(zip(gt_files, data_files))[per * rank:per * (rank + 1)]
        self._rng = random.Random(seed)
        if self.one_label:
            self.sampler = STSampler(num_steps, time_shift, self.time_step_us, events_threshold, box_size_threshold)
        else:
            self.sampler = MTSampler(num_steps, self.time_step_us)
        self._batcher = None
        self._samples = None

    def get_labels(self) -> List[str]:
        """The class names of the dataset."""
        return list(CLASS_NAMES[self.dataset])

    def _groups(self):
        """Groups of ``files_in_flight`` opened recordings with their boxes, from an endless cycle over this rank's files
        in an order shuffled once."""
        order = list(range(len(self.files)))
        self._rng.shuffle(order)
        cycle = itertools.cycle(order)
        while True:
            group = list(itertools.islice(cycle, self.files_in_flight))
            yield group, [load_boxes(self.files[i][0], self.dataset, self.time_step_us) for i in group], \
                [DatRecording(self.files[i][1]) for i in group]

    def samples(self, with_file: bool = False) -> Iterator:
        """Host samples ``(words_slice, t0_us, labels)`` in the feed's order (``with_file``: ``(file index, sample)``)."""
        if self.chained:
            yield from self._chained_samples(with_file)
            return
        groups = self._groups()
        if self.one_label:
            # round-robin over the files in flight; an exhausted file leaves the round, the next group is opened when all have
            barren = 0   # groups in a row that gave no sample: a whole cycle of them means no file ever will
            while True:
                group, boxes, recs = next(groups)
                live = list(range(len(group)))
                barren += 1
                if barren * self.files_in_flight > len(self.files) + self.files_in_flight:
                    raise RuntimeError("PropheseeFeed: no recording of this rank yields a sample (labels missing, boxes "
                                       "under box_size_threshold, or fewer events than events_threshold per step)")
                while live:
                    still = []
                    for k in live:
                        sample, more = self.sampler(boxes[k], recs[k])
                        if more:
                            still.append(k)
                        if sample is not None:
                            barren = 0
                            yield (group[k], sample) if with_file else sample
                    live = still
                    self._rng.shuffle(live)
        else:
            windows = RECORD_TIME_US // (self.time_step_us * self.num_steps)
            visits = list(range(self.files_in_flight * windows))
            self._rng.shuffle(visits)
            while True:
                group, boxes, recs = next(groups)
                for v in visits:
                    k = v % self.files_in_flight
                    sample = self.sampler(boxes[k], recs[k])
                    yield (group[k], sample) if with_file else sample

    def _chained_samples(self, with_file: bool = False) -> Iterator:
        """``chained=True``: sample ``k`` belongs to batch slot ``k % batch_size``, and a slot is bound to ONE recording -
        it yields that recording's windows in time order (``MTSampler``'s rule, window ``n + 1`` starting ``num_steps *
        time_step`` after window ``n``, without the wrap to the start), then takes the next file of the shuffled cycle over
        this rank's files.  A sample is ``(words_slice, t0_us, labels[n, 6], first, aug_row)``: ``first`` is 1 on the first
        window of a recording in its slot (the very first batch included), ``aug_row`` the slot's ``EventAugment`` row
        (``int32[8]``; None without ``augment``), drawn when the slot opens the recording and unchanged until the next -
        the carried state keeps belonging to the same transformed scene.  (The drop stays a draw per event: the row's seed
        is hashed with every event's index.)  A recording without events has no window and is passed over."""
        order = list(range(len(self.files)))
        self._rng.shuffle(order)
        cycle = itertools.cycle(order)

        def open_next():
            for _ in range(len(self.files)):
                i = next(cycle)
                rec = DatRecording(self.files[i][1])
                if len(rec):
                    row = None if self.augment is None else self.augment.draw(1, self.width, self.height)[0]
                    return i, load_boxes(self.files[i][0], self.dataset, self.time_step_us), rec, row
            raise RuntimeError("PropheseeFeed: no recording of this rank holds an event")

        slots = [None] * self.batch_size
        while True:
            for b in range(self.batch_size):
                first = 0
                if slots[b] is None or slots[b][2].done:
                    slots[b], first = open_next(), 1
                i, boxes, rec, row = slots[b]
                sample = (*self.sampler(boxes, rec), first, row)
                yield (i, sample) if with_file else sample

    def __iter__(self):
        return self

    def _next_chained(self):
        """``(X, labels[B, N, 6], first)``: ``first`` int32 ``[B]`` on the device, for ``SODa(carry_state=True)``."""
        batch = [next(self._samples) for _ in range(self.batch_size)]
        labels = [torch.from_numpy(np.ascontiguousarray(s[2])) for s in batch]
        if not any(int(l.shape[0]) for l in labels):
            labels[0] = torch.full((1, 6), -1.0)   # (a batch without any row would collate five columns wide)
        table = None if self.augment is None else torch.stack([s[4] for s in batch])
        X, lab = self._batcher([(s[0], s[1]) for s in batch], labels, aug_table=table)
        first = torch.tensor([s[3] for s in batch], dtype=torch.int32).pin_memory()
        return X, lab, first.to(X.device, non_blocking=True)

    def __next__(self):
        from .data import EventBatcher
        if self._batcher is None:
            self._batcher = EventBatcher(self.num_steps, self.height, self.width, self.time_step_us, device=self.device,
                                         augment=self.augment, representation=self.representation)
            self._samples = self.samples()
        if self.chained:
            return self._next_chained()
        batch = [next(self._samples) for _ in range(self.batch_size)]
        return self._batcher([(w, t0) for w, t0, _ in batch], [torch.from_numpy(np.ascontiguousarray(l)) for _, _, l in batch])
