#!/usr/bin/env python3
"""Depthwise 3x3 convolutions at the TinyYolo GEN1 layer shapes (B = 5, T = 32: N = 160 frames; tools/layer_table.py), one
MI355X.

    python tools/dwconv_bench.py [--rounds 3] [--iters 20] [--warmup 3] [--frames 160]

Per shape, alternating inside ONE call (so that the comparisons share the machine's state):

* snn_dwconv_fwd / snn_dwconv_dgrad / snn_dwconv_wgrad, each alone: time from device events after warm-up, the bytes the
  call has to move computed from the shapes (operands read once + result written once; the weights and the weight
  gradient's slab rows are counted too), and the achieved TB/s against the ~6.3 TB/s a streaming kernel reaches here;
* the DENSE 3x3 layer of the same place in the network on today's path (functional.conv2d, default arithmetic): forward,
  and backward (data + weight gradient);
* the PAIR depthwise 3x3 + dense 1x1 (Cin -> Cout) that would replace it, forward and backward, against the dense layer.

The median over the rounds is reported with the min - max spread.  Prints a table and one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from snn_for_object_detection_amd import _hip  # noqa: E402
from snn_for_object_detection_amd import functional as HF  # noqa: E402

ACHIEVABLE_TBS = 6.3
# (H, W, Cin, Cout, stride) of the 3x3 layers of TinyYolo at 240 x 304 (profiles/r04_layer_table_gen1.txt): the bottleneck
# layers (stride 1, C -> C) and the stage-entry layers (stride 2)
SHAPES = [(60, 76, 64, 64, 1), (30, 38, 128, 128, 1), (15, 19, 128, 128, 1),
          (120, 152, 64, 128, 2), (60, 76, 128, 256, 2), (30, 38, 256, 256, 2)]
K = 3


def timed(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters   # ms


def cl(*shape):
    """Random {0,1}-ish channels-last [1,N,C,H,W] tensor (spikes: what these layers read in the network)."""
    n, c, h, w = shape
    return HF._cl_view((torch.rand(1, n, h, w, c, device="cuda") < 0.2).float())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=160)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dwconv_bench needs a HIP device: a time measured anywhere else says nothing")
    _hip.load()
    N = args.frames
    st = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    results = []
    for H, W, Cin, Cout, s in SHAPES:
        C = Cin
        Ho, Wo = (H + 2 - K) // s + 1, (W + 2 - K) // s + 1
        x = cl(N, C, H, W)
        w_dw = torch.randn(C, 1, K, K, device="cuda") / K
        wt = torch.empty(K * K, C, device="cuda")
        _hip.call("snn_weight_transpose", w_dw.data_ptr(), wt.data_ptr(), C, K, K, 1, st)
        y = HF._new_cl((1, N), C, Ho, Wo, x)
        gy = HF._cl_view(torch.randn(1, N, Ho, Wo, C, device="cuda"))
        dx = HF._new_cl((1, N), C, H, W, x)
        dw = torch.empty(C, K * K, device="cuda")
        ws_bytes = _hip.query("snn_dwconv_wgrad_workspace_size", N, H, W, C, K, s, 1, 0)
        ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device="cuda")
        n_in, n_out = 4 * N * H * W * C, 4 * N * Ho * Wo * C
        calls = {
            "dw_fwd": (lambda: _hip.call("snn_dwconv_fwd", x.data_ptr(), C, wt.data_ptr(), y.data_ptr(), C, N, H, W, C, K, s, 1, st),
                       n_in + n_out + 4 * K * K * C),
            "dw_dgrad": (lambda: _hip.call("snn_dwconv_dgrad", gy.data_ptr(), C, wt.data_ptr(), dx.data_ptr(), C, N, H, W, C, K, s,
                                           1, st),
                         n_in + n_out + 4 * K * K * C),
            "dw_wgrad": (lambda: _hip.call("snn_dwconv_wgrad", x.data_ptr(), C, gy.data_ptr(), C, dw.data_ptr(), N, H, W, C, K, s, 1,
                                           0, ws.data_ptr(), 0, st),
                         n_in + n_out + 2 * ws_bytes + 4 * K * K * C),
        }
        # the dense layer of this place, and the separable pair that would replace it (autograd: fwd, then dgrad + wgrad)
        w_dense = torch.nn.Parameter((torch.randn(Cout, Cin, K, K, device="cuda") / (3 * Cin ** 0.5))
                                     .contiguous(memory_format=torch.channels_last))
        w_pw = torch.nn.Parameter((torch.randn(Cout, Cin, 1, 1, device="cuda") / Cin ** 0.5)
                                  .contiguous(memory_format=torch.channels_last))
        w_dwp = torch.nn.Parameter(w_dw.clone())
        xg = x.detach().clone().requires_grad_()
        g_out = HF._cl_view(torch.randn(1, N, Ho, Wo, Cout, device="cuda"))

        def dense_fwd():
            return HF.conv2d(xg, w_dense, s, 1)

        def pair_fwd():
            return HF.conv2d(HF.depthwise_conv2d(xg, w_dwp, s, 1), w_pw, 1, 0)

        def fwd_bwd(f):
            def run():
                f().backward(g_out)
                xg.grad = w_dense.grad = w_pw.grad = w_dwp.grad = None
            return run

        def only_fwd(f):
            def run():
                with torch.no_grad():
                    f()
            return run

        plan = [(k, fn) for k, (fn, _) in calls.items()]
        plan += [("dense_fwd", only_fwd(dense_fwd)), ("dense_fwd_bwd", fwd_bwd(dense_fwd)),
                 ("pair_fwd", only_fwd(pair_fwd)), ("pair_fwd_bwd", fwd_bwd(pair_fwd))]
        times = {k: [] for k, _ in plan}
        for _ in range(args.rounds):
            for k, fn in plan:      # alternating: every round visits every variant once
                times[k].append(timed(fn, args.warmup, args.iters))
        row = {"shape": f"N{N} {H}x{W} {Cin}->{Cout} k{K} s{s}"}
        for k, v in times.items():
            row[k] = {"ms": statistics.median(v), "min": min(v), "max": max(v)}
            if k in calls:
                row[k]["bytes"] = calls[k][1]
                row[k]["tbs"] = calls[k][1] / (row[k]["ms"] * 1e-3) / 1e12
        for k in ("dense", "pair"):
            row[f"{k}_bwd_ms"] = row[f"{k}_fwd_bwd"]["ms"] - row[f"{k}_fwd"]["ms"]
        results.append(row)
        del x, y, gy, dx, ws, xg, g_out
        torch.cuda.empty_cache()

    print(f"depthwise 3x3 kernels, fp32, median of {args.rounds} rounds x {args.iters} launches (min - max); "
          f"achievable ~{ACHIEVABLE_TBS} TB/s")
    print(f"{'shape':<30}{'kernel':<10}{'us':>9}{'min':>9}{'max':>9}{'MB':>9}{'TB/s':>7}{'of achievable':>15}")
    for r in results:
        for k in ("dw_fwd", "dw_dgrad", "dw_wgrad"):
            e = r[k]
            print(f"{r['shape']:<30}{k:<10}{e['ms'] * 1e3:>9.1f}{e['min'] * 1e3:>9.1f}{e['max'] * 1e3:>9.1f}"
                  f"{e['bytes'] / 1e6:>9.1f}{e['tbs']:>7.2f}{100 * e['tbs'] / ACHIEVABLE_TBS:>14.0f}%")
    print()
    print("dense 3x3 layer (today's path, default arithmetic) against the pair depthwise 3x3 + dense 1x1; "
          "fwd and fwd+bwd (bwd = data + weight gradients), us")
    print(f"{'shape':<30}{'dense fwd':>11}{'pair fwd':>10}{'ratio':>7}{'dense f+b':>11}{'pair f+b':>10}{'ratio':>7}")
    for r in results:
        df, pf, db, pb = (r[k]["ms"] * 1e3 for k in ("dense_fwd", "pair_fwd", "dense_fwd_bwd", "pair_fwd_bwd"))
        print(f"{r['shape']:<30}{df:>11.1f}{pf:>10.1f}{pf / df:>7.2f}{db:>11.1f}{pb:>10.1f}{pb / db:>7.2f}")
    print()
    print(json.dumps({"tool": "dwconv_bench", "frames": N, "rounds": args.rounds, "iters": args.iters, "results": results}))


if __name__ == "__main__":
    main()
