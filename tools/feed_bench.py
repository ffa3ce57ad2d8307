#!/usr/bin/env python3
"""PCIe-inclusive rates of the step feeding the path, GEN1 B=5 T=32, 5 % occupancy.

  (a) reference-style feed: dense fp32 frames [T,B,2,H,W] built on the host, pinned H2D copy, NCHW -> NHWC pass
  (b) EventBatcher: raw events (4 x int32 per event) pinned H2D on a copy stream + HIP scatter into channels-last frames
and the training throughput with (b) inside the loop (the feed of step n+1 overlaps step n).

``--augment`` adds the augmented feed (``EventAugment``: raw int64 timestamps binned inside the scatter kernel, 4 copies
per sample and one launch): with identity tables, with ``hflip=0.5, zoom=(0.75, 1.25), drop=(0, 0.1)``, and the fed
training step with that augmentation beside the plain one.

``--packed`` adds the packed feed (8-byte DAT records unpacked inside the scatter kernel, one staging copy and one H2D
copy per batch): plain beside (b) and augmented beside (d), alternating, the training step fed by it, the bytes per batch
of the three forms, and the host time per batch of ``PropheseeFeed`` reading seeded recordings from a temporary
directory.

``--representation NAME`` (count, time or voxel) times the feed of that representation beside the binary one in the same
run, alternating: packed records with ``--packed``, tuple samples otherwise, augmented with ``--augment``."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import snn_for_object_detection_amd as S  # noqa: E402
from snn_for_object_detection_amd.trainer import FlatTrainer  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("--augment", action="store_true", help="also time the augmented feed and the training step fed by it")
ap.add_argument("--packed", action="store_true", help="also time the packed feed (DAT records unpacked in the kernel), "
                "the training step fed by it and PropheseeFeed's host time per batch")
ap.add_argument("--representation", default=None, choices=("count", "time", "voxel"),
                help="also time the feed with this event representation beside the binary feed")
args = ap.parse_args()

T, B, H, W, step_us = 32, 5, 240, 304, 1000
rng = np.random.default_rng(0)
samples = []
n_events = 0
for b in range(B):
    n = int(0.05 * T * 2 * H * W)
    t = rng.integers(0, T * step_us, n).astype(np.int32)
    x = rng.integers(0, W, n).astype(np.int32)
    y = rng.integers(0, H, n).astype(np.int32)
    p = rng.integers(0, 2, n).astype(np.int32)
    samples.append(tuple(torch.from_numpy(v).pin_memory() for v in (t, x, y, p)) + (0,))
    n_events += n
labels = [torch.tensor([[0, 0.2, 0.2, 0.5, 0.6], [1, 0.5, 0.4, 0.9, 0.8]])] * B
batcher = S.EventBatcher(T, H, W, step_us)
if args.augment or args.packed:
    # the augmented feed takes the timestamps as the recordings hold them: int64 microseconds (20 bytes per event)
    samples_aug = [(s[0].to(torch.int64).pin_memory(),) + s[1:] for s in samples]
    aug_batcher = S.EventBatcher(T, H, W, step_us,
                                 augment=S.EventAugment(hflip=0.5, zoom=(0.75, 1.25), drop=(0.0, 0.1), seed=0))
dense_host = batcher(samples).cpu().contiguous().pin_memory()   # what the reference's DataLoader would hand over


def timeit(fn, n=10):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / n


def feed_dense():
    return S.functional.to_channels_last(dense_host.cuda(non_blocking=True))


def feed_events():
    return batcher(samples)


print(f"events per batch {n_events} ({16 * n_events / 1e6:.1f} MB as 4 x int32) vs dense {dense_host.numel() * 4 / 1e6:.1f} MB")
print(f"(a) dense H2D + layout pass : {timeit(feed_dense):6.2f} ms per batch")
print(f"(b) events H2D + scatter    : {timeit(feed_events):6.2f} ms per batch")


def feed_identity():
    return aug_batcher(samples_aug, augment=False)


def feed_augmented_frames():
    return aug_batcher(samples_aug)


def feed_augmented():
    return aug_batcher(samples_aug, labels)


if args.augment:
    # the feeds differ by tenths of a millisecond: alternate them over five rounds and report the median with the spread
    feeds = (("(b) again, beside the feeds below", feed_events),
             (f"(c) raw events H2D ({20 * n_events / 1e6:.1f} MB, int64 t) + binning scatter, identity tables", feed_identity),
             ("(d) (c) with flip / zoom / shift / drop", feed_augmented_frames),
             ("(e) (d) with the boxes collated, copied and augmented", feed_augmented))
    rounds = [[timeit(fn, n=20) for _, fn in feeds] for _ in range(5)]
    for k, (name, _) in enumerate(feeds):
        ms = sorted(r[k] for r in rounds)
        print(f"{name:<86}: {ms[2]:6.2f} ms per batch (median of 5 x 20; {ms[0]:.2f} .. {ms[-1]:.2f})")

if args.packed:
    # the same events as 8-byte DAT records (sorted by time, as a recording holds them), window start 0
    samples_packed = []
    for s in samples:
        order = np.argsort(s[0].numpy(), kind="stable")
        samples_packed.append((S.pack_events(*(v.numpy()[order] for v in s[:4])), 0))

    def feed_packed():
        return batcher(samples_packed)

    def feed_packed_augmented():
        return aug_batcher(samples_packed)

    assert torch.equal(feed_packed(), feed_events())
    print(f"bytes per batch: packed records {8 * n_events / 1e6:.1f} MB (8 per event, 1 copy), 4 x int32 "
          f"{16 * n_events / 1e6:.1f} MB (16 per event, {4 * B} copies), int64 t + 3 x int32 {20 * n_events / 1e6:.1f} MB "
          f"(20 per event, {4 * B} copies)")
    feeds = (("(b) again, beside the feeds below", feed_events),
             ("(p) packed records H2D + unpacking scatter, no table", feed_packed),
             ("(d) tuple events (int64 t) with flip / zoom / shift / drop", feed_augmented_frames),
             ("(q) packed records with flip / zoom / shift / drop", feed_packed_augmented))
    rounds = [[timeit(fn, n=20) for _, fn in feeds] for _ in range(5)]
    for k, (name, _) in enumerate(feeds):
        ms = sorted(r[k] for r in rounds)
        print(f"{name:<86}: {ms[2]:6.2f} ms per batch (median of 5 x 20; {ms[0]:.2f} .. {ms[-1]:.2f})")

if args.representation:
    # the same samples through two batchers that differ in the representation alone, alternating over five rounds
    kw = dict(augment=S.EventAugment(hflip=0.5, zoom=(0.75, 1.25), drop=(0.0, 0.1), seed=0)) if args.augment else {}
    pair = [S.EventBatcher(T, H, W, step_us, representation=r, **kw) for r in ("binary", args.representation)]
    fed = samples_packed if args.packed else (samples_aug if args.augment else samples)
    form = ("packed records" if args.packed else "tuple events") + (", flip / zoom / shift / drop" if args.augment else "")
    X_rep = pair[1](fed)
    torch.cuda.synchronize()
    print(f"representation {args.representation}: max {float(X_rep.max()):.4f}, {int((X_rep != 0).sum())} cells set")
    rounds = [[timeit(lambda b=b: b(fed), n=20) for b in pair] for _ in range(5)]
    for k, name in enumerate(("binary", args.representation)):
        ms = sorted(r[k] for r in rounds)
        print(f"(r) {form}, {name:<6}: {ms[2]:6.2f} ms per batch (median of 5 x 20; {ms[0]:.2f} .. {ms[-1]:.2f})")

torch.manual_seed(2)
model = S.TinyYolo(num_classes=2, time_window=0).cuda().train()
trainer = FlatTrainer(model)
lab = torch.stack(labels).cuda()


def train_step(X):
    trainer.zero_grad()
    loss = model.training_step((X, lab))
    loss.backward()
    trainer.step()


X = feed_events()
resident = timeit(lambda: train_step(X), n=10)


def fed_step():
    global X
    train_step(X)          # queue step n ...
    X = feed_events()      # ... and feed step n+1 while it runs


fed = timeit(fed_step, n=10)
print(f"training step, batch resident in HBM : {resident:6.2f} ms -> {B * T / resident * 1e3:7.0f} event-frames/s")
print(f"training step, events fed every step : {fed:6.2f} ms -> {B * T / fed * 1e3:7.0f} event-frames/s (PCIe inclusive)")

if args.augment:
    batch = feed_augmented()

    def fed_step_augmented():
        global batch
        trainer.zero_grad()
        loss = model.training_step(batch)   # the augmented boxes train with the augmented frames
        loss.backward()
        trainer.step()
        batch = feed_augmented()

    fed_aug = timeit(fed_step_augmented, n=10)
    print(f"training step, augmented events fed   : {fed_aug:6.2f} ms -> {B * T / fed_aug * 1e3:7.0f} event-frames/s "
          f"(PCIe inclusive)")

if args.packed:
    import statistics
    import tempfile

    def fed_step_packed():
        global X
        train_step(X)
        X = feed_packed()

    # alternate with the tuple-fed step: the two differ by less than the run-to-run spread of a step
    rounds = [(timeit(fed_step, n=10), timeit(fed_step_packed, n=10)) for _ in range(5)]
    for k, name in enumerate(("training step, tuple events fed (again) ", "training step, packed records fed       ")):
        ms = sorted(r[k] for r in rounds)
        print(f"{name}: {ms[2]:6.2f} ms -> {B * T / ms[2] * 1e3:7.0f} event-frames/s (PCIe inclusive; median of 5 x 10; "
              f"{ms[0]:.2f} .. {ms[-1]:.2f})")

    # PropheseeFeed on recordings of two seconds at the same event rate (5 % occupancy per 1 ms step), labels every 40 ms:
    # host time of one batch = binary searches + staging copy + enqueue, to the end of the enqueue (no device wait asked for)
    with tempfile.TemporaryDirectory() as root:
        d = os.path.join(root, "gen1", "train")
        os.makedirs(d)
        box_dtype = [("ts", "<u8"), ("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("class_id", "u1"),
                     ("confidence", "<f4"), ("track_id", "<u4")]
        per_ms, seconds = int(0.05 * 2 * H * W), 2
        for i in range(2):
            n = per_ms * 1000 * seconds
            t = np.sort(rng.integers(0, seconds * 1_000_000, n))
            words = S.pack_events(t, rng.integers(0, W, n), rng.integers(0, H, n), rng.integers(0, 2, n))
            S.write_dat(os.path.join(d, f"bench_{i}_td.dat"), words, W, H)
            boxes = np.zeros(seconds * 25 - 1, dtype=box_dtype)
            boxes["ts"] = (np.arange(boxes.size) + 1) * 40_000 + 500
            boxes["x"], boxes["y"], boxes["w"], boxes["h"] = 0.2 * W, 0.2 * H, 0.4 * W, 0.5 * H
            np.save(os.path.join(d, f"bench_{i}_bbox.npy"), boxes)
            del words, t
        feed = S.PropheseeFeed(root, dataset="gen1", split="train", batch_size=B, num_steps=T, time_step=1, time_shift=16,
                               files_in_flight=2, seed=0)
        for _ in range(4):
            next(feed)
        torch.cuda.synchronize()
        host, events_fed = [], []
        for _ in range(40):
            t0 = time.perf_counter()
            Xf, _ = next(feed)
            host.append(1e3 * (time.perf_counter() - t0))
            torch.cuda.synchronize()
            events_fed.append(int(Xf.sum()))
        host.sort()
        print(f"PropheseeFeed host time per batch (B={B}, T={T}, 2 s recordings, ~{per_ms * T * B} events per batch): "
              f"median {statistics.median(host):.2f} ms ({host[0]:.2f} .. {host[-1]:.2f}, 40 batches; search + staging copy + "
              f"enqueue), {statistics.median(events_fed)} cells set per batch")
        del feed
