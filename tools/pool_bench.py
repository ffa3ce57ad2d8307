#!/usr/bin/env python3
"""Padded pooling and the SPP pyramid at the two shapes an SPPF stage would see in TinyYolo GEN1 behind a C -> C/2 1x1
convolution (B = 5, T = 32: N = 160 frames of 76x60x64 and of 38x30x128), one MI355X.

    python tools/pool_bench.py [--rounds 5] [--iters 20] [--warmup 3] [--frames 160] [--out profiles/spp_ab.txt]

Per shape, alternating inside ONE call (so that the comparisons share the machine's state):

* SPP(5, 3) as generated (``BlockGen(C, [SPP(5, 3)])``: one ``snn_spp_fwd``, three ``snn_pool2d_bwd``) against the
  spelled-out ``Dense([[Pass()], [P], [P, P], [P, P, P]])`` of ``P = Pool("M", 5, 1, 2)``: forward, and forward + backward;
* ``snn_spp_fwd`` alone against the chained launches it replaces (one ``snn_copy_channels`` + three ``snn_pool2d_fwd`` into
  the same buffer): time, the bytes the call has to move computed from the shapes (operands read once + results written
  once), and the achieved GB/s beside the ~6.3 TB/s a streaming copy reaches on this chip;
* ``snn_pool2d_bwd`` (MAX, 5, 1, 2, with addend) alone;
* the new kernels at (2, 2, 0) against ``snn_pool_fwd`` / ``snn_pool_bwd`` (MAX) - what a later move of the unpadded
  ``Pool`` onto them would change.

Before timing, the outputs of every pair are compared (``torch.equal``).  The median over the rounds is reported with the
min - max spread.  Prints the table, writes it to ``--out`` and prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import snn_for_object_detection_amd as S  # noqa: E402
from snn_for_object_detection_amd import _hip  # noqa: E402
from snn_for_object_detection_amd import functional as HF  # noqa: E402

COPY_TBS = 6.3          # measured float4 copy rate of the chip (79 % of the 8.0 TB/s specification)
SHAPES = [(76, 60, 64), (38, 30, 128)]
K, LEVELS = 5, 3


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


def spikes(n, h, w, c):
    """Random {0,1} channels-last [1,N,C,H,W] tensor (what a LIF layer hands an SPPF stage)."""
    return HF._cl_view((torch.rand(1, n, h, w, c, device="cuda") < 0.2).float())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--frames", type=int, default=160)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "spp_ab.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pool_bench needs a HIP device: a time measured anywhere else says nothing")
    _hip.load()
    N = args.frames
    st = torch.cuda.current_stream().cuda_stream
    torch.manual_seed(0)
    MAXK = _hip.POOL_MAX
    results = []
    for H, W, C in SHAPES:
        CT = (LEVELS + 1) * C
        unit = 4 * N * H * W * C                     # bytes of one C-channel tensor
        x = spikes(N, H, W, C)
        fused = S.BlockGen(C, [S.SPP(K, LEVELS)]).cuda()
        P = lambda: S.Pool("M", K, 1, K // 2)
        spelled = S.BlockGen(C, S.Dense([[S.Pass()], [P()], [P(), P()], [P(), P(), P()]])).cuda()
        xg = x.detach().clone().requires_grad_()
        g_out = HF._cl_view(torch.randint(-4, 5, (1, N, H, W, CT), device="cuda").float())

        # the two spellings compute the same thing, bit for bit
        ya, yb = fused(xg)[0], spelled(xg)[0]
        assert torch.equal(ya, yb)
        ya.backward(g_out)
        ga, xg.grad = xg.grad, None
        yb.backward(g_out)
        assert torch.equal(ga, xg.grad)
        xg.grad = None
        del ya, yb, ga

        def fwd_bwd(blk):
            def run():
                blk(xg)[0].backward(g_out)
                xg.grad = None
            return run

        def only_fwd(blk):
            def run():
                with torch.no_grad():
                    blk(x)
            return run

        # the kernels alone
        y = torch.empty(N, H, W, CT, device="cuda")
        y2 = torch.empty(N, H, W, CT, device="cuda")
        h = torch.empty(N, H, W, C, device="cuda")
        gy = g_out.permute(0, 1, 3, 4, 2).reshape(N, H, W, CT).contiguous()

        def spp_kernel():
            _hip.call("snn_spp_fwd", x.data_ptr(), C, y.data_ptr(), CT, N, H, W, C, K, LEVELS, st)

        def chained_kernels():
            _hip.call("snn_copy_channels", x.data_ptr(), C, y2.data_ptr(), CT, N * H * W, C, st)
            for j in range(LEVELS):
                _hip.call("snn_pool2d_fwd", MAXK, y2.data_ptr() + 4 * j * C, CT, y2.data_ptr() + 4 * (j + 1) * C, CT, N, H, W, C,
                          K, 1, K // 2, st)

        def bwd_kernel():   # R(y_2; g_3) + g_2: one level of the SPP backward
            _hip.call("snn_pool2d_bwd", MAXK, y.data_ptr() + 8 * C, CT, gy.data_ptr() + 12 * C, CT, gy.data_ptr() + 8 * C, CT,
                      h.data_ptr(), C, N, H, W, C, K, 1, K // 2, st)

        spp_kernel()
        chained_kernels()
        assert torch.equal(y, y2)
        # (2, 2, 0): the unpadded entry points against the new kernels, dense operands
        Ho, Wo = H // 2, W // 2
        xd = x.permute(0, 1, 3, 4, 2).reshape(N, H, W, C).contiguous()
        p_old, p_new = torch.empty(N, Ho, Wo, C, device="cuda"), torch.empty(N, Ho, Wo, C, device="cuda")
        gp = torch.randn(N, Ho, Wo, C, device="cuda")
        gx_old, gx_new = torch.empty_like(xd), torch.empty_like(xd)
        k220 = {
            "pool_fwd_220": lambda: _hip.call("snn_pool_fwd", MAXK, xd.data_ptr(), p_old.data_ptr(), N, H, W, C, Ho, Wo, 2, 2, st),
            "pool2d_fwd_220": lambda: _hip.call("snn_pool2d_fwd", MAXK, xd.data_ptr(), C, p_new.data_ptr(), C, N, H, W, C, 2, 2,
                                                0, st),
            "pool_bwd_220": lambda: _hip.call("snn_pool_bwd", MAXK, xd.data_ptr(), gp.data_ptr(), gx_old.data_ptr(), N, H, W, C,
                                              Ho, Wo, 2, 2, st),
            "pool2d_bwd_220": lambda: _hip.call("snn_pool2d_bwd", MAXK, xd.data_ptr(), C, gp.data_ptr(), C, None, 0,
                                                gx_new.data_ptr(), C, N, H, W, C, 2, 2, 0, st),
        }
        for fn in k220.values():
            fn()
        assert torch.equal(p_old, p_new) and torch.equal(gx_old, gx_new)

        small = 4 * N * Ho * Wo * C
        nbytes = {"spp_fwd_kernel": 5 * unit,                       # x read once, four slices written
                  "chained_fwd_kernels": 8 * unit,                  # copy: 1 + 1; each pool: 1 + 1
                  "pool2d_bwd_512": 4 * unit,                       # x, gy, addend read; gx written
                  "pool_fwd_220": unit + small, "pool2d_fwd_220": unit + small,
                  "pool_bwd_220": 2 * unit + small, "pool2d_bwd_220": 2 * unit + small}
        plan = [("spp_fwd", only_fwd(fused)), ("spelled_fwd", only_fwd(spelled)),
                ("spp_fwd_bwd", fwd_bwd(fused)), ("spelled_fwd_bwd", fwd_bwd(spelled)),
                ("spp_fwd_kernel", spp_kernel), ("chained_fwd_kernels", chained_kernels), ("pool2d_bwd_512", bwd_kernel)]
        plan += list(k220.items())
        times = {k: [] for k, _ in plan}
        for _ in range(args.rounds):
            for k, fn in plan:      # alternating: every round visits every variant once
                times[k].append(timed(fn, args.warmup, args.iters))
        row = {"shape": f"N{N} {H}x{W}x{C}"}
        for k, v in times.items():
            row[k] = {"ms": statistics.median(v), "min": min(v), "max": max(v)}
            if k in nbytes:
                row[k]["bytes"] = nbytes[k]
                row[k]["gbs"] = nbytes[k] / (row[k]["ms"] * 1e-3) / 1e9
        results.append(row)
        del x, xg, g_out, y, y2, h, gy, xd, p_old, p_new, gp, gx_old, gx_new, fused, spelled
        torch.cuda.empty_cache()

    lines = [f"pool_bench: SPP({K}, {LEVELS}) and padded pooling, fp32, {torch.cuda.get_device_name(0)}; median of "
             f"{args.rounds} rounds x {args.iters} launches (min - max), variants alternating inside every round",
             f"outputs and input gradients of the two spellings, of the fused and the chained forward kernels and of the new and "
             f"old (2,2,0) kernels compared before timing: equal",
             "",
             "SPP as generated (1 forward launch, 3 backward launches) against Dense([[Pass],[P],[P,P],[P,P,P]]), us",
             f"{'shape':<20}{'SPP fwd':>10}{'(min-max)':>18}{'spelled fwd':>13}{'(min-max)':>18}{'ratio':>7}"
             f"{'SPP f+b':>10}{'(min-max)':>18}{'spelled f+b':>13}{'(min-max)':>18}{'ratio':>7}"]

    def mm(e):
        return f"({e['min'] * 1e3:.0f}-{e['max'] * 1e3:.0f})"
    for r in results:
        a, b, c, d = (r[k] for k in ("spp_fwd", "spelled_fwd", "spp_fwd_bwd", "spelled_fwd_bwd"))
        lines.append(f"{r['shape']:<20}{a['ms'] * 1e3:>10.1f}{mm(a):>18}{b['ms'] * 1e3:>13.1f}{mm(b):>18}{a['ms'] / b['ms']:>7.2f}"
                     f"{c['ms'] * 1e3:>10.1f}{mm(c):>18}{d['ms'] * 1e3:>13.1f}{mm(d):>18}{c['ms'] / d['ms']:>7.2f}")
    lines += ["", f"kernels alone: time, bytes the call must move (from the shapes), effective GB/s; a streaming copy reaches "
                  f"~{COPY_TBS * 1e3:.0f} GB/s here",
              f"{'shape':<20}{'call':<22}{'us':>9}{'min':>9}{'max':>9}{'MB':>9}{'GB/s':>8}{'of copy rate':>14}"]
    for r in results:
        for k in ("spp_fwd_kernel", "chained_fwd_kernels", "pool2d_bwd_512", "pool_fwd_220", "pool2d_fwd_220", "pool_bwd_220",
                  "pool2d_bwd_220"):
            e = r[k]
            lines.append(f"{r['shape']:<20}{k:<22}{e['ms'] * 1e3:>9.1f}{e['min'] * 1e3:>9.1f}{e['max'] * 1e3:>9.1f}"
                         f"{e['bytes'] / 1e6:>9.1f}{e['gbs']:>8.0f}{100 * e['gbs'] / (COPY_TBS * 1e3):>13.0f}%")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(json.dumps({"tool": "pool_bench", "frames": N, "rounds": args.rounds, "iters": args.iters, "results": results}))


if __name__ == "__main__":
    main()
