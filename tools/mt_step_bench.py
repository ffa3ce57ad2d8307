"""What training on every labelled timestep costs: forward + backward + update of TinyYolo at the GEN1 shape
(304 x 240, B = 5, T = 32) for the single-label step and for ``label_steps`` 1, 2 and 4.

Every variant gets its own model (same seed) and ``FlatTrainer``, the same synthetic events and the same boxes; the
six-column labels put two boxes on each of the sample's labelled steps (the last ``K`` of T - 1, T - 9, T - 17, T - 25:
Prophesee boxes arrive at 1 - 4 Hz).  ``--warmup`` untimed steps, then ``--steps`` steps between two device
synchronisations on the wall clock, as bench.py times its step; the variants are measured in turn, ``--rounds`` times,
and the median per variant is reported.  The single-label step is the baseline the others are read against; no
threshold is claimed.  Prints one JSON line.

    python tools/mt_step_bench.py [--steps 10] [--warmup 3] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def boxes(B, n, classes, gen):
    out = torch.empty(B, n, 5)
    for b in range(B):
        for k in range(n):
            while True:
                xy = torch.rand(2, 2, generator=gen)
                lo, hi = xy.min(0).values, xy.max(0).values
                if (hi - lo).prod() > 0.01:
                    break
            out[b, k, 0] = float(torch.randint(0, classes, (1,), generator=gen))
            out[b, k, 1:3], out[b, k, 3:5] = lo, hi
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--B", type=int, default=5)
    ap.add_argument("--H", type=int, default=240)
    ap.add_argument("--W", type=int, default=304)
    ap.add_argument("--classes", type=int, default=2)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mt_step_bench: needs a HIP device")
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd.trainer import FlatTrainer

    gen = torch.Generator().manual_seed(0)
    X = (torch.rand(a.T, a.B, 2, a.H, a.W, generator=gen) < 0.05).float().cuda()
    per_step = 2
    labelled = [a.T - 1 - 8 * i for i in range(4) if a.T - 1 - 8 * i >= 0]
    bx = boxes(a.B, per_step * len(labelled), a.classes, gen)
    labels5 = bx[:, :per_step].contiguous().cuda()                     # the single-label step: the last frame's boxes

    def labels6(K):
        ts = torch.tensor([t for t in labelled[:K] for _ in range(per_step)], dtype=torch.float32)
        n = ts.numel()
        return torch.cat([ts.view(1, n, 1).expand(a.B, n, 1), bx[:, :n]], dim=2).contiguous().cuda()

    variants = [("single_label", None, labels5)] + [(f"label_steps_{K}", K, labels6(K)) for K in (1, 2, 4)
                                                    if K <= len(labelled)]
    runs = {}
    for name, K, labels in variants:
        torch.manual_seed(2)
        model = S.TinyYolo(num_classes=a.classes, time_window=0, label_steps=K).cuda().train()
        trainer = FlatTrainer(model, lr=model.hparams.learning_rate)

        def step(model=model, trainer=trainer, labels=labels):
            trainer.zero_grad()
            loss = model.training_step((X, labels))
            loss.backward()
            trainer.step()
            return loss
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        runs[name] = (step, [])
    for _ in range(a.rounds):
        for name, (step, times) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = step()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0) / a.steps)
            if not bool(torch.isfinite(loss)):
                raise SystemExit(f"mt_step_bench: {name} gave a non-finite loss")
    out = {"T": a.T, "B": a.B, "H": a.H, "W": a.W, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds}
    for name, (_, times) in runs.items():
        times.sort()
        out[name + "_ms"] = round(times[len(times) // 2], 3)
        out[name + "_ms_all"] = [round(t, 3) for t in times]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
