"""What carrying the neuron state across training steps costs: TinyYolo at the GEN1 shape (304 x 240, B = 5, T = 32,
resident batch, ``label_steps = 2``), forward + backward + update, stateless against ``carry_state=True``.

The carried step hands every scan an initial state, so its reverse LIF scans leave the from-state fast path (they read the
convolution output ``y`` again for the BatchNorm sums), and it launches ``snn_state_reset`` once.  Both variants get their
own model (same seed) and ``FlatTrainer``, the same events and labels; ``--warmup`` untimed steps, then ``--steps`` steps
between two device synchronisations on the wall clock, the variants in turn, ``--rounds`` times; medians are reported.

The reset launch alone, on the state tree the carried model holds: ``functional.reset_state_`` with ``first`` all zero and
all one, against the same reset written with torch operators - a ``mul_`` per tensor by a broadcast keep-mask, and one
``torch._foreach_mul_`` over all of them - wall clock per call over ``--reset-calls`` calls between two synchronisations.
No threshold is claimed.  Prints one JSON line.

    python tools/carry_bench.py [--steps 10] [--warmup 3] [--rounds 3]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402


def leaves(tree):
    if isinstance(tree, torch.Tensor):
        return [tree]
    if isinstance(tree, (list, tuple)):
        return [t for k in tree for t in leaves(k)]
    return []


def median(times):
    times = sorted(times)
    return times[len(times) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=32)
    ap.add_argument("--B", type=int, default=5)
    ap.add_argument("--H", type=int, default=240)
    ap.add_argument("--W", type=int, default=304)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reset-calls", type=int, default=200)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("carry_bench: needs a HIP device")
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd import functional as HF
    from snn_for_object_detection_amd.trainer import FlatTrainer

    gen = torch.Generator().manual_seed(0)
    X = (torch.rand(a.T, a.B, 2, a.H, a.W, generator=gen) < 0.05).float().cuda()
    labels = torch.full((a.B, 4, 6), -1.0)
    for b in range(a.B):
        for j, ts in enumerate((a.T - 1, a.T - 1, max(a.T - 9, 0), max(a.T - 9, 0))):
            lo = torch.rand(2, generator=gen) * 0.5
            labels[b, j] = torch.tensor([float(ts), float(j % 2), float(lo[0]), float(lo[1]), float(lo[0]) + 0.3,
                                         float(lo[1]) + 0.3])
    labels = labels.cuda()
    zeros = torch.zeros(a.B, dtype=torch.int32).cuda()
    ones = torch.ones(a.B, dtype=torch.int32).cuda()

    runs = {}
    for name, carried in (("stateless", False), ("carried", True)):
        torch.manual_seed(2)
        model = S.TinyYolo(num_classes=2, time_window=0, label_steps=2, carry_state=carried).cuda().train()
        trainer = FlatTrainer(model, lr=model.hparams.learning_rate)
        batch = (X, labels, zeros) if carried else (X, labels)

        def step(model=model, trainer=trainer, batch=batch):
            trainer.zero_grad()
            loss = model.training_step(batch)
            loss.backward()
            trainer.step()
            return loss
        for _ in range(a.warmup):
            step()
        torch.cuda.synchronize()
        runs[name] = (step, [], model)
    for _ in range(a.rounds):
        for name, (step, times, _) in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = step()
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0) / a.steps)
            if not bool(torch.isfinite(loss)):
                raise SystemExit(f"carry_bench: {name} gave a non-finite loss")
    out = {"T": a.T, "B": a.B, "H": a.H, "W": a.W, "steps": a.steps, "warmup": a.warmup, "rounds": a.rounds}
    for name, (_, times, _) in runs.items():
        out[name + "_ms"] = round(median(times), 3)
        out[name + "_ms_all"] = [round(t, 3) for t in times]

    # ---- the reset alone, on the carried model's state tree
    tree = runs["carried"][2]._carried["train"][1]
    flat = leaves(tree)
    out["state_tensors"] = len(flat)
    out["state_mbytes"] = round(sum(t.numel() for t in flat) * 4 / 2 ** 20, 2)

    def torch_each(first):
        keep = (first == 0).to(torch.float32)
        for t in flat:
            t.mul_(keep.view(-1, *([1] * (t.dim() - 1))))

    def torch_foreach(first):
        keep = (first == 0).to(torch.float32)
        torch._foreach_mul_(flat, [keep.view(-1, *([1] * (t.dim() - 1))).expand_as(t) for t in flat])

    variants = {"kernel": lambda f: HF.reset_state_(tree, f), "torch_mul": torch_each, "torch_foreach_mul": torch_foreach}
    times = {(n, k): [] for n in variants for k in ("none", "all")}
    for fn in variants.values():
        fn(zeros)
    for _ in range(a.rounds):
        for n, fn in variants.items():
            for k, first in (("none", zeros), ("all", ones)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.reset_calls):
                    fn(first)
                torch.cuda.synchronize()
                times[n, k].append(1e6 * (time.perf_counter() - t0) / a.reset_calls)
    for (n, k), ts in times.items():
        out[f"reset_{n}_first_{k}_us"] = round(median(ts), 1)
        out[f"reset_{n}_first_{k}_us_all"] = [round(t, 1) for t in ts]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
