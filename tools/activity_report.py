"""Per-layer firing rates and synaptic operations of a benchmark workload, and what recording them costs.

Builds the network and the synthetic batch of ``bench.py --config ...``, runs one pass under ``activity.record`` and prints
the per-layer table (``activity.format_report``).  Then times the pass with the recorder on and off: device events around
every pass, the two modes ALTERNATING in one process (the same clocks, caches and allocator state for both), medians over
``--reps`` pairs.  Without ``--train`` the pass is the eval-mode, no_grad forward (``SODa.activity_report``); with it, the
whole training step (forward, loss, backward, optimiser) with the recorder around the forward.  The last line is JSON.

    python tools/activity_report.py --config gen1|1mpx|deep12 [--train] [--per-step] [--reps 10] [--batch B] [--T T]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

import bench  # noqa: E402
from snn_for_object_detection_amd import _hip, activity  # noqa: E402
from snn_for_object_detection_amd.trainer import FlatTrainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(bench.CONFIGS), default="gen1")
    ap.add_argument("--train", action="store_true", help="record and time a training step instead of the eval forward")
    ap.add_argument("--per-step", action="store_true", help="LIF counts per timestep")
    ap.add_argument("--reps", type=int, default=10, help="timed on / off pairs")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=None)
    ap.add_argument("--T", type=int, default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("activity_report.py needs a HIP device")
    _hip.load()
    cfg = bench.CONFIGS[a.config]
    H, W, classes = cfg["H"], cfg["W"], cfg["classes"]
    B, T = a.batch or cfg["batch"], a.T or cfg["T"]
    dev = "cuda:0"
    X, labels = bench.synthetic_batch(T, B, H, W, classes, dev, seed=0, p=cfg["p"])
    model, lr = bench.build_model(a, cfg, classes, dev)
    deep = a.config == "deep12"
    probe = bench.deep12_probe(B, H, W, dev) if deep else None
    rec = activity.Recorder(model, per_step=a.per_step)

    if a.train:
        trainer = FlatTrainer(model, lr=lr, find_unused_parameters=False)

        def forward():
            if deep:
                out, _ = model(X, last_only=True)
                return (out * probe).mean()
            return model.training_step((X, labels))

        def run(on):
            trainer.zero_grad()
            if on:
                with activity.record(rec):
                    loss = forward()
            else:
                loss = forward()
            loss.backward()
            trainer.step()
    else:
        model.eval()

        def run(on):
            with torch.no_grad():
                if on:
                    with activity.record(rec):
                        model(X)
                else:
                    model(X)

    if not a.train:
        # running statistics of an untrained network: one train-mode pass, as a validation after the first epoch would see
        model.train()
        with torch.no_grad():
            model(X)
        model.eval()
    for _ in range(a.warmup):
        run(False)
    torch.cuda.synchronize()
    run(True)                       # the pass the table shows
    rep = rec.report()
    print(activity.format_report(rep))

    times = {False: [], True: []}
    for _ in range(a.reps):
        for on in (False, True):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            run(on)
            end.record()
            end.synchronize()
            times[on].append(start.elapsed_time(end))
    off, on = statistics.median(times[False]), statistics.median(times[True])
    t = rep["totals"]
    print(json.dumps({"config": a.config, "pass": "training step" if a.train else "eval forward", "batch": B, "T": T,
                      "lif_layers": len(rep["layers"]), "convolutions": len(rep["convs"]),
                      "mean_rate": t["rate"], "gsynops": t["synops"] / 1e9, "gmacs": t["macs"] / 1e9,
                      "ms_recorder_off": round(off, 3), "ms_recorder_on": round(on, 3),
                      "overhead_percent": round(100.0 * (on - off) / off, 2), "reps": a.reps}))


if __name__ == "__main__":
    main()
