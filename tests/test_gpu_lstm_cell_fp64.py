"""The pointwise ConvLSTM cell kernels - snn_lstm_cell_fwd / snn_lstm_cell_bwd (csrc/lstm.hip) - through the C ABI, every
element against the fp64 restatements of tests/lstm_kernel_ref.py within their derived bounds (no norm anywhere).

Outputs are NaN-filled buffers with a NaN guard behind them (``Guarded``); the guards, and every output the call was not
asked for, must come back bit for bit.  Shapes: M C in {1, 255 .. 272} with C in {1, 3, 16} (below, at and past one
256-thread block, rows that straddle a block), and one row past the grid cap of 8 blocks per CU with a partial second
trip of the grid-stride loop.  Values: the pre-activation grid over [-104, 104] (each gate drawn on its own, so that
saturated gates meet unsaturated ones), random values at three scales, cell states up to +-50.  Every NULL combination
of c_prev, gh, gc and g_c_prev.

``test_libm_allowances_are_twice_the_measurement`` measures what the bounds take as constants: the error of the device's
sigmoidf_ and tanhf, in fp32 ulps, read through the cell kernel (F c_prev + I G with I = 0, c_prev = 1 is F; with F = 0, I = 1
it is G).  Run with -s to see the figures DESIGN quotes.
"""
import pytest
import torch

from tests import lstm_kernel_ref as R
from tests.elementwise_ref import ulps
from tests.test_gpu_targets_fp64 import Guarded

pytestmark = pytest.mark.gpu
F32 = torch.float32
_WORST = {}


@pytest.fixture(scope="module")
def hip(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from snn_for_object_detection_amd import _hip
    return _hip


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bits(t):
    return t.contiguous().view(torch.int32)


def run_fwd(hip, gates, c_prev):
    M, C = gates.shape[0], gates.shape[1] // 4
    g, cp = gates.cuda(), None if c_prev is None else c_prev.cuda()
    h, c = Guarded(M * C, F32), Guarded(M * C, F32)
    hip.call("snn_lstm_cell_fwd", g.data_ptr(), _ptr(cp), h.ptr, c.ptr, M, C, _st())
    torch.cuda.synchronize()
    assert h.guard_intact() and c.guard_intact()
    return {"h": h.out(M, C), "c": c.out(M, C)}


def run_bwd(hip, gates, c_prev, c, gh, gc, want_cp):
    M, C = c.shape
    dev = [None if t is None else t.cuda() for t in (gates, c_prev, c, gh, gc)]
    gg, gcp = Guarded(M * 4 * C, F32), Guarded(M * C, F32)
    hip.call("snn_lstm_cell_bwd", *[_ptr(t) for t in dev], gg.ptr, gcp.ptr if want_cp else None, M, C, _st())
    torch.cuda.synchronize()
    assert gg.guard_intact() and gcp.guard_intact()
    if not want_cp:
        assert gcp.untouched()
    return {"g_gates": gg.out(M, 4 * C), "g_c_prev": gcp.out(M, C) if want_cp else None}


def _check(out, res, names, what):
    for n in names:
        assert bool(torch.isfinite(out[n]).all()), (what, n)
        r = R.worst_ratio(out[n], res, n)
        _WORST[n] = max(_WORST.get(n, 0.0), r)
        assert r <= 1.0, (what, n, r)


def _check_exact_zeros(gates, g_gates, what):
    """From 17 up 1 + expf(-x) is 1.0f whatever expf's last bit, and tanhf is +-1.0f: I (1 - I), .. and 1 - G G are 0."""
    C = gates.shape[1] // 4
    for k, name in enumerate("IFOG"):
        pre, d = gates[:, k * C:(k + 1) * C], g_gates[:, k * C:(k + 1) * C]
        sat = (pre >= 17.0) | ((pre <= -17.0) if name == "G" else torch.zeros_like(pre, dtype=torch.bool))
        assert bool((d[sat] == 0).all()), (what, name)


def check_cell(hip, M, C, kind):
    d = R.cell_values(M, C, kind)
    what = (M, C, kind)
    for cp in (None, d["c_prev"]):
        out = run_fwd(hip, d["gates"], cp)
        _check(out, R.cell_fwd(d["gates"], cp), ("c", "h"), what + ("fwd", cp is not None))
        again = run_fwd(hip, d["gates"], cp)
        assert torch.equal(_bits(out["h"]), _bits(again["h"])) and torch.equal(_bits(out["c"]), _bits(again["c"]))
        for gh, gc in ((d["gh"], None), (None, d["gc"]), (d["gh"], d["gc"])):
            res = R.cell_bwd(d["gates"], cp, d["c"], gh, gc)
            for want_cp in (False, True):
                tag = what + ("bwd", cp is not None, gh is not None, gc is not None, want_cp)
                out = run_bwd(hip, d["gates"], cp, d["c"], gh, gc, want_cp)
                _check(out, res, ("g_gates", "g_c_prev") if want_cp else ("g_gates",), tag)
                _check_exact_zeros(d["gates"], out["g_gates"], tag)
            again = run_bwd(hip, d["gates"], cp, d["c"], gh, gc, True)
            assert torch.equal(_bits(out["g_gates"]), _bits(again["g_gates"]))
            assert torch.equal(_bits(out["g_c_prev"]), _bits(again["g_c_prev"]))


@pytest.mark.parametrize("M,C", R.CELL_SHAPES, ids=[f"{m}x{c}" for m, c in R.CELL_SHAPES])
def test_cell_kernels_per_element(hip, M, C):
    for kind in R.CELL_VALUES:
        check_cell(hip, M, C, kind)
    print(f"cell {M}x{C}: worst error / bound so far " + ", ".join(f"{n} {r:.3f}" for n, r in sorted(_WORST.items())))


def test_grid_stride_loop_reaches_the_tail(hip):
    cap = 8 * torch.cuda.get_device_properties(0).multi_processor_count * 256      # threads of the capped grid
    C = 3
    M = (cap + cap // 3) // C + 1
    assert cap < M * C < 2 * cap
    d = R.cell_values(M, C, "grid")
    out = run_fwd(hip, d["gates"], d["c_prev"])
    _check(out, R.cell_fwd(d["gates"], d["c_prev"]), ("c", "h"), "oversize fwd")
    res = R.cell_bwd(d["gates"], d["c_prev"], d["c"], d["gh"], d["gc"])
    out = run_bwd(hip, d["gates"], d["c_prev"], d["c"], d["gh"], d["gc"], True)
    _check(out, res, ("g_gates", "g_c_prev"), "oversize bwd")
    _check_exact_zeros(d["gates"], out["g_gates"], "oversize bwd")
    print("oversize row: worst error / bound so far " + ", ".join(f"{n} {r:.3f}" for n, r in sorted(_WORST.items())))


def test_libm_allowances_are_twice_the_measurement(hip):
    g = torch.Generator().manual_seed(11)
    v = torch.cat([R.grid_values()] + [torch.randn(2048, generator=g) * s for s in (0.1, 1.0, 10.0)])
    n = v.numel()
    col = lambda x: torch.full((n,), x)  # noqa: E731
    # c = F * 1 + I * G with I = sigmoid(-200) = 0 and G = tanh(0) = 0: the device's sigmoidf_(v), exactly
    sig = run_fwd(hip, torch.stack([col(-200.0), v, col(0.0), col(0.0)], 1), torch.ones(n, 1))["c"][:, 0]
    # c = F * 0 + I * G with F = 0 and I = sigmoid(104) = 1.0f: the device's tanhf(v), exactly
    tanh = run_fwd(hip, torch.stack([col(104.0), col(-200.0), col(0.0), v], 1), None)["c"][:, 0]
    for name, out, ref, allow in (("sigmoidf_", sig, torch.sigmoid(v.double()), R.A_SIG),
                                  ("tanhf", tanh, torch.tanh(v.double()), R.A_TANH)):
        e = ulps(out, ref)
        i = int(e.argmax())
        print(f"{name}: max {float(e[i]):.3f} fp32 ulps at x = {float(v[i])!r} (device {float(out[i])!r}, fp64 {float(ref[i])!r}); "
              f"allowance {allow}")
        assert bool(torch.isfinite(out).all())
        assert 2.0 * float(e[i]) <= allow, (name, float(e[i]), float(v[i]))
    # what the overflow of expf(-x) used to flush to zero: the subnormal tail of the sigmoid
    tail = (v < -88.0) & (v > -103.0)
    assert bool((sig[tail] > 0).all())
