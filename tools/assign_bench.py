"""What the task-aligned anchor assignment costs, at the GEN1 shape (A = 13 545 anchors, B = 5, N = 16 label rows).

Two measurements, both comparing inside ONE call (boxes differ by a few percent, runs inside a call do not):

* the assignment alone - ``snn_tal_assign`` (three launches) against ``snn_roi_assign`` (one launch), on five-column
  labels and on the ``K = 4`` steps form (``snn_roi_assign_steps``) - device time from events around ``--iters``
  back-to-back calls, the variants in turn, ``--rounds`` times, median per variant;
* ``--step``: forward + backward + update of TinyYolo (304 x 240, T = 32) with ``assigner="iou"`` and ``assigner="tal"``,
  timed as tools/mt_step_bench.py times its steps.

Prints one JSON line.  No threshold is claimed.

    python tools/assign_bench.py [--iters 50] [--rounds 5] [--step] [--steps 10] [--warmup 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def _labels(B, N, classes, gen):
    lo = torch.rand(B, N, 2, generator=gen) * 0.6
    wh = 0.05 + torch.rand(B, N, 2, generator=gen) * 0.35
    cls = torch.randint(0, classes, (B, N, 1), generator=gen).float()
    return torch.cat([cls, lo, lo + wh], dim=2)


def _median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def assignment(a):
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd.roi import RoI, TaskAlignedAssigner
    gen = torch.Generator().manual_seed(0)
    model = S.TinyYolo(num_classes=a.classes, time_window=0).cuda().eval()
    with torch.no_grad():
        anchors = model(torch.zeros(1, 1, 2, a.H, a.W, device="cuda"))[0].contiguous()
    A, C, B, N, K = anchors.shape[0], a.classes + 1, a.B, a.N, a.K
    labels5 = _labels(B, N, a.classes, gen).cuda()
    ts = torch.randint(0, K, (B, N, 1), generator=gen).float()
    labels6 = torch.cat([ts.cuda(), labels5], dim=2).contiguous()
    steps = torch.arange(K, dtype=torch.int32).view(K, 1).repeat(1, B).cuda()
    cls5, bb5 = torch.randn(B, A, C, generator=gen).cuda(), torch.randn(B, A, 4, generator=gen).cuda()
    cls6, bb6 = torch.randn(K, B, A, C, generator=gen).cuda(), torch.randn(K, B, A, 4, generator=gen).cuda()
    roi, tal = RoI(0.4), TaskAlignedAssigner(a.topk)
    variants = {
        "roi_assign": lambda: roi(anchors, labels5),
        "tal_assign": lambda: tal(anchors, labels5, cls5, bb5),
        f"roi_assign_steps_K{K}": lambda: roi.steps(anchors, labels6, steps, 0),
        f"tal_assign_steps_K{K}": lambda: tal.steps(anchors, labels6, steps, 0, cls6, bb6),
    }
    runs = {name: [] for name in variants}
    for fn in variants.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, fn in variants.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                fn()
            t1.record()
            torch.cuda.synchronize()
            runs[name].append(t0.elapsed_time(t1) * 1000.0 / a.iters)
    return {"A": A, "B": B, "N": N, "K": K, "topk": a.topk,
            "us_per_call": {n: {"median": round(_median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                            for n, v in runs.items()}}


def full_step(a):
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd.trainer import FlatTrainer
    gen = torch.Generator().manual_seed(0)
    X = (torch.rand(a.T, a.B, 2, a.H, a.W, generator=gen) < 0.05).float().cuda()
    labels = _labels(a.B, a.N, a.classes, gen).cuda()
    steps_of = {}
    for name in ("iou", "tal"):
        torch.manual_seed(2)
        model = S.TinyYolo(num_classes=a.classes, time_window=0, assigner=name, tal_topk=a.topk).cuda().train()
        trainer = FlatTrainer(model, lr=model.hparams.learning_rate)

        def step(model=model, trainer=trainer):
            trainer.zero_grad()
            loss = model.training_step((X, labels))
            loss.backward()
            trainer.step()
            return loss
        for _ in range(a.warmup):
            step()
        steps_of[name] = step
    runs = {name: [] for name in steps_of}
    for _ in range(a.rounds):
        for name, step in steps_of.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                step()
            torch.cuda.synchronize()
            runs[name].append((time.perf_counter() - t0) * 1000.0 / a.steps)
    return {"T": a.T, "ms_per_step": {n: {"median": round(_median(v), 3), "min": round(min(v), 3),
                                          "max": round(max(v), 3)} for n, v in runs.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--B", type=int, default=5)
    ap.add_argument("--H", type=int, default=240)
    ap.add_argument("--W", type=int, default=304)
    ap.add_argument("--N", type=int, default=16)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--topk", type=int, default=10)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--step", action="store_true", help="also time the full training step with either assigner")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("assign_bench: needs a HIP device")
    out = {"tool": "assign_bench", "device": torch.cuda.get_device_name(0), "assignment": assignment(a)}
    if a.step:
        out["step"] = full_step(a)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
