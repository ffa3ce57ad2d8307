"""Device time of the detection mAP (metrics.MeanAveragePrecision) on a GEN1-shaped validation batch.

Times, with HIP events, (1) ``update_padded`` of one batch of ``multibox_detection`` rows (B=5, A=13 545 anchors, C=2
classes; scores / boxes drawn from a seed) and (2) ``compute()`` over ``--batches`` such updates.  Prints one JSON line.
``--areas`` adds the small / medium / large ranges, ``--class-metrics`` the per-class AP / AR, ``--filter`` a minimum box
diagonal and side (pixels of the ``--image-size`` frame); without them the metric runs its default launches.

    python tools/map_bench.py [--batches 100] [--reps 20] [--areas] [--class-metrics] [--filter]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from snn_for_object_detection_amd.metrics import MeanAveragePrecision  # noqa: E402


def batch(B, A, C, G, gen):
    dev = "cuda"
    lo = torch.rand(B, A, 2, generator=gen) * 0.9
    dets = torch.cat([torch.randint(-1, C, (B, A, 1), generator=gen).float(), torch.rand(B, A, 1, generator=gen),
                      lo, lo + 0.01 + torch.rand(B, A, 2, generator=gen) * 0.1], dim=2)
    lo = torch.rand(B, G, 2, generator=gen) * 0.9
    labels = torch.cat([torch.randint(-1, C, (B, G, 1), generator=gen).float(), lo,
                        lo + 0.01 + torch.rand(B, G, 2, generator=gen) * 0.1], dim=2)
    return dets.to(dev), labels.to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=5)
    ap.add_argument("--A", type=int, default=13545)
    ap.add_argument("--C", type=int, default=2)
    ap.add_argument("--G", type=int, default=16)
    ap.add_argument("--batches", type=int, default=100)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--areas", action="store_true", help="area_ranges=True")
    ap.add_argument("--class-metrics", action="store_true", help="class_metrics=True")
    ap.add_argument("--filter", action="store_true", help="min_box_diag=12, min_box_side=6 (arbitrary: protocol unpinned)")
    ap.add_argument("--image-size", type=int, nargs=2, default=[240, 304], metavar=("H", "W"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("map_bench: needs a HIP device")
    gen = torch.Generator().manual_seed(0)
    data = [batch(a.B, a.A, a.C, a.G, gen) for _ in range(a.batches)]
    opts = {}
    if a.areas:
        opts.update(area_ranges=True)
    if a.class_metrics:
        opts.update(class_metrics=True)
    if a.filter:
        opts.update(min_box_diag=12.0, min_box_side=6.0)
    if a.areas or a.filter:
        opts.update(image_size=tuple(a.image_size))
    m = MeanAveragePrecision(a.C, **opts)
    for d, g in data[:3]:                      # warm-up: library load, torch sort plans, threshold tables
        m.update_padded(d, g)
    m.compute()
    m.reset()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    upd = []
    for r in range(a.reps):
        d, g = data[r % a.batches]
        ev[0].record()
        m.update_padded(d, g)
        ev[1].record()
        torch.cuda.synchronize()
        upd.append(ev[0].elapsed_time(ev[1]))
    comp = []
    for r in range(max(3, a.reps // 4)):
        m.reset()
        for d, g in data:
            m.update_padded(d, g)
        torch.cuda.synchronize()
        ev[0].record()
        out = m.compute()
        ev[1].record()
        torch.cuda.synchronize()
        comp.append(ev[0].elapsed_time(ev[1]))
    upd.sort()
    comp.sort()
    print(json.dumps({"update_padded_ms_median": upd[len(upd) // 2], "update_padded_ms_min": upd[0],
                      "compute_ms_median": comp[len(comp) // 2], "compute_ms_min": comp[0], "batches": a.batches,
                      "B": a.B, "A": a.A, "C": a.C, "G": a.G, "options": sorted(opts), "map": float(out["map"])}))


if __name__ == "__main__":
    main()
