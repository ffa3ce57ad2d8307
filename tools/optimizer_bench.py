"""Device time of ``FlatTrainer.step()`` with and without the weight average (EMA), on TinyYolo at the GEN1 class count.

Two trainers on two identically seeded models in ONE process: a default one and one with ``ema_decay=0.9999``.  Each takes
one real training step on a tiny clip (so every gradient slot is written and the composed 1x1 groups are registered as in
training), then ``flat_grad`` is filled once from a seed and only ``step()`` is timed: the two trainers alternate, ``--steps``
steps per block between two HIP events, ``--reps`` blocks each.  The fused Adamax launch alone is timed the same way
through the C ABI on the first trainer's buffers.  Prints one JSON line: median / min / max ms per step of both, the same
for the kernel alone, and the 28 and 36 bytes per parameter the two kernels move over those times.

    python tools/optimizer_bench.py [--steps 200] [--reps 5]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import snn_for_object_detection_amd as S  # noqa: E402
from snn_for_object_detection_amd import _hip  # noqa: E402
from snn_for_object_detection_amd.trainer import FlatTrainer  # noqa: E402

GEN1_CLASSES = 2
EMA_DECAY = 0.9999


def tiny_batch(device):
    g = torch.Generator().manual_seed(0)
    X = (torch.rand(2, 1, 2, 32, 48, generator=g) < 0.1).float()
    labels = torch.tensor([[[0.0, 0.2, 0.2, 0.6, 0.7], [1.0, 0.4, 0.1, 0.9, 0.5]]])
    return X.to(device), labels.to(device)


def build(ema: bool, batch):
    torch.manual_seed(0)
    model = S.TinyYolo(num_classes=GEN1_CLASSES, time_window=0).cuda().train()
    tr = FlatTrainer(model, lr=1e-4, **({"ema_decay": EMA_DECAY} if ema else {}))
    tr.zero_grad()
    model.training_step(batch).backward()
    tr.step()
    g = torch.Generator().manual_seed(1)
    tr.synchronize()
    tr.flat_grad.copy_(torch.randn(tr.flat_grad.shape, generator=g) * 1e-3)
    assert all(slot.written for slot in tr.slots)
    return model, tr


def timed_blocks(fns, steps, reps, warmup):
    """``fns``: name -> callable of one step.  Alternates the callables block by block; -> name -> sorted ms per step."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            start.record()
            for _ in range(steps):
                fn()
            end.record()
            torch.cuda.synchronize()
            out[name].append(start.elapsed_time(end) / steps)
    return {name: sorted(v) for name, v in out.items()}


def stats(ms, bytes_moved):
    med = ms[len(ms) // 2]
    return {"ms_median": med, "ms_min": ms[0], "ms_max": ms[-1], "gbs_at_median": bytes_moved / (med * 1e-3) / 1e9}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200, help="steps per timed block (at least 200 for a quotable number)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("optimizer_bench: needs a HIP device")
    batch = tiny_batch("cuda")
    (_, plain), (_, ema) = build(False, batch), build(True, batch)
    n = plain.flat_param.numel()
    steps = timed_blocks({"default": plain.step, "ema": ema.step}, a.steps, a.reps, a.warmup)

    st = torch.cuda.current_stream().cuda_stream
    ptrs = [t.data_ptr() for t in (plain.flat_param, plain.flat_grad, plain.exp_avg, plain.exp_inf)]
    scratch_ema = plain.flat_param.clone()
    hyper = (n, 1e-4, 0.9, 0.999, 1e-8, 1000, 1.0)
    kernels = timed_blocks({
        "default": lambda: _hip.call("snn_adamax_step", *ptrs, *hyper, st),
        "ema": lambda: _hip.call("snn_adamax_step_ema", *ptrs, scratch_ema.data_ptr(), *hyper, 0.0, 0.0, 1.0 - EMA_DECAY, None,
                                 st),
    }, a.steps, a.reps, a.warmup)
    d, e = stats(steps["default"], 28.0 * n), stats(steps["ema"], 36.0 * n)
    print(json.dumps({
        "parameters": plain.numel, "elements_per_launch": n, "steps_per_block": a.steps, "reps": a.reps,
        "ema_decay": EMA_DECAY, "float_buffer_elements": int(ema.ema_buffers.numel()),
        "step_default": d, "step_ema": e,
        "step_ema_overhead_ms_median": e["ms_median"] - d["ms_median"],
        "kernel_adamax_28B": stats(kernels["default"], 28.0 * n),
        "kernel_adamax_ema_36B": stats(kernels["ema"], 36.0 * n),
        "note": "step_* time the whole FlatTrainer.step() (optimiser launch, weight-image refresh, with the average also the "
                "buffer update); their gbs_at_median divides the optimiser launch's bytes by that whole time",
    }))


if __name__ == "__main__":
    main()
