#!/usr/bin/env python3
"""Detection decode (softmax probs -> NMS'd rows): device kernels vs the host torch path, GEN1 anchor count.

``--frames N`` (N > 1) times the batched path (``box.multibox_detection_batched``: no loop over the
frames) against the per-frame loop over the same N frames: device events, median of ``--repeats`` runs after warm-up."""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from snn_for_object_detection_amd import box  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=1)
ap.add_argument("--repeats", type=int, default=20)
args = ap.parse_args()

torch.manual_seed(21)
A, K, N = 13545, 3, args.frames
centers = torch.rand(A, 2)
wh = 0.02 + 0.1 * torch.rand(A, 2)
anchors = torch.cat([centers - wh / 2, centers + wh / 2], dim=1)
probs = torch.softmax(4 * torch.randn(N, A, K), dim=2)
offs = 0.3 * torch.randn(N, A, 4)
pd, od, ad = probs.cuda(), offs.cuda(), anchors.cuda()


def per_frame_loop():
    return torch.cat([box._multibox_detection_device(pd[n:n + 1], od[n:n + 1], ad, 0.1, 0.009999999) for n in range(N)])


def median_ms(fns, repeats):
    """Median device time of each of ``fns`` (events around every run; three warm-up runs first; the candidates alternate,
    so that a change of clock or of load on the machine falls on all of them)."""
    for _ in range(3):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(repeats):
        for fn, ts in zip(fns, times):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            ts.append(start.elapsed_time(stop))
    return [statistics.median(ts) for ts in times]


if N == 1:
    t0 = time.perf_counter()
    ref = box.multibox_detection(probs.clone(), offs.clone(), anchors)
    t_host = time.perf_counter() - t0
    for _ in range(3):
        box.multibox_detection(pd, od, ad)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(20):
        det = box.multibox_detection(pd, od, ad)
    torch.cuda.synchronize()
    t_dev = (time.perf_counter() - t0) / 20
    print(f"A={A}: kept {int((ref[0, :, 0] >= 0).sum())}; host torch path {1e3 * t_host:.1f} ms; device path {1e3 * t_dev:.2f} ms "
          f"per frame (no host synchronisation)")
else:
    assert torch.equal(box.multibox_detection_batched(pd, od, ad), per_frame_loop())
    t_loop, t_batched = median_ms([per_frame_loop, lambda: box.multibox_detection_batched(pd, od, ad)], args.repeats)
    print(f"A={A}, {N} frames: per-frame loop {t_loop:.2f} ms ({t_loop / N:.3f} ms per frame); batched {t_batched:.2f} ms "
          f"({t_batched / N:.3f} ms per frame); x{t_loop / t_batched:.1f}")
