"""Host side of the layout / merge / pooling / activation / small-GEMM tests: what needs no GPU.

* tests/elementwise_ref.py (the loops tests/test_gpu_elementwise_fp64.py compares the kernels with) against torch's own fp64
  CPU operators on the same inputs, ties, NaN and -inf included;
* the argument checks of the C ABI of csrc/elementwise.hip and csrc/small_gemm.hip: every refusal returns 1 before any launch
  (a failed launch would return 2) with a message that names the call."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import elementwise_ref as R

EPS64 = 2.0 ** -53


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def _same(a, b):
    """Equal as values, NaN == NaN."""
    return bool((((a != a) & (b != b)) | (a == b)).all())


def _pool_inputs(N, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randn((N, H, W, C), generator=g, dtype=torch.float64)
    spikes = (torch.rand((N, H, W, C), generator=g) < 0.4).double()
    const = torch.full((N, H, W, C), 0.75, dtype=torch.float64)
    bad = rnd.clone()
    bad[0, 0, 0, 0] = math.nan                       # a corner: in one window only
    bad[0, H // 2, W // 2, :] = math.nan             # the middle: in every overlapping window around it
    bad[-1, 1:, :, -1] = -math.inf                   # whole windows of -inf
    bad[-1, H - 1, W - 1, 0] = math.nan              # the ragged tail (when there is one)
    bad[0, 1, 1, 0] = -math.inf
    allneg = torch.full((N, H, W, C), -math.inf, dtype=torch.float64)
    return {"random": rnd, "spikes": spikes, "const": const, "nan-inf": bad, "all-inf": allneg}


POOL_GEOMS = [(1, 1, 4, 5), (2, 2, 5, 7), (2, 1, 4, 5), (3, 1, 5, 6), (3, 2, 6, 8), (2, 3, 6, 7), (4, 4, 4, 4)]


@pytest.mark.parametrize("k,stride,H,W", POOL_GEOMS)
def test_pool_references_match_torch_fp64(k, stride, H, W):
    N, C = 2, 3
    for name, x in _pool_inputs(N, H, W, C, seed=k * 10 + stride).items():
        Ho, Wo = R.pool_out(H, k, stride), R.pool_out(W, k, stride)
        g = torch.Generator().manual_seed(5)
        gy = torch.randn((N, Ho, Wo, C), generator=g, dtype=torch.float64)
        gy_int = torch.randint(-4, 5, (N, Ho, Wo, C), generator=g).double()
        # max: forward and the routed gradient are exact
        xt = _nchw(x).requires_grad_()
        want = F.max_pool2d(xt, k, stride)
        got, _ = R.pool_fwd_ref(R.POOL_MAX, x, k, stride)
        assert _same(got, _nhwc(want.detach())), (name, "max fwd")
        for gsel, exact in ((gy_int, True), (gy, False)):
            (gx_t,) = torch.autograd.grad(want, xt, _nchw(gsel), retain_graph=True)
            gx, gmag = R.pool_bwd_ref(R.POOL_MAX, x, gsel, k, stride)
            if exact:       # integer gradients: the order in which overlapping windows are added does not matter
                assert torch.equal(gx, _nhwc(gx_t)), (name, "max bwd")
            else:
                assert bool(((gx - _nhwc(gx_t)).abs() <= k * k * EPS64 * gmag).all()), (name, "max bwd")
        if name in ("nan-inf", "all-inf"):
            continue   # a sum over NaN / inf is NaN / inf in both: nothing to compare per element
        for kind, scale in ((R.POOL_AVG, 1.0), (R.POOL_SUM, float(k * k))):
            xt = _nchw(x).requires_grad_()
            want = F.avg_pool2d(xt, k, stride) * scale
            got, mag = R.pool_fwd_ref(kind, x, k, stride)
            assert bool(((got - _nhwc(want.detach())).abs() <= (k * k + 4) * EPS64 * mag).all()), (name, kind, "fwd")
            (gx_t,) = torch.autograd.grad(want, xt, _nchw(gy))
            gx, gmag = R.pool_bwd_ref(kind, x, gy, k, stride)
            assert bool(((gx - _nhwc(gx_t)).abs() <= (k * k + 4) * EPS64 * gmag).all()), (name, kind, "bwd")
            cover = R.pool_cover(H, W, k, stride)
            assert bool((gx[:, cover == 0, :] == 0).all()) and bool((_nhwc(gx_t)[:, cover == 0, :] == 0).all())


def test_max_pool_tie_rule_is_the_first_maximum():
    """Hand-made windows: the gradient goes to the first maximum in row-major order, to the LAST NaN, and to tap 0 of a
    window of -inf; torch's fp64 backward agrees."""
    inf, nan = math.inf, math.nan
    rows = [([[1, 1], [1, 1]], (0, 0)), ([[0, 1], [1, 1]], (0, 1)), ([[0, 0], [0, 1]], (1, 1)),
            ([[nan, 5], [6, 7]], (0, 0)), ([[nan, 5], [nan, 7]], (1, 0)), ([[3, nan], [9, 2]], (0, 1)),
            ([[-inf, -inf], [-inf, -inf]], (0, 0)), ([[-inf, -2], [-2, -inf]], (0, 1))]
    for win, (bi, bj) in rows:
        x = torch.tensor(win, dtype=torch.float64).reshape(1, 2, 2, 1)
        gy = torch.full((1, 1, 1, 1), 3.0, dtype=torch.float64)
        gx, _ = R.pool_bwd_ref(R.POOL_MAX, x, gy, 2, 2)
        want = torch.zeros(2, 2, dtype=torch.float64)
        want[bi, bj] = 3.0
        assert torch.equal(gx.reshape(2, 2), want), win
        xt = _nchw(x).requires_grad_()
        (gt,) = torch.autograd.grad(F.max_pool2d(xt, 2, 2), xt, _nchw(gy))
        assert torch.equal(gt.reshape(2, 2), want), win


@pytest.mark.parametrize("s", [1, 2, 3])
def test_upsample_references_match_torch_fp64(s):
    g = torch.Generator().manual_seed(s)
    x = torch.randn((2, 3, 5, 4), generator=g, dtype=torch.float64)
    xt = _nchw(x).requires_grad_()
    want = F.interpolate(xt, scale_factor=s, mode="nearest")
    got, _ = R.upsample_fwd_ref(x, s)
    assert torch.equal(got, _nhwc(want.detach()))
    for gy in (torch.randint(-4, 5, got.shape, generator=g).double(), torch.randn(got.shape, generator=g, dtype=torch.float64)):
        (gt,) = torch.autograd.grad(want, xt, _nchw(gy), retain_graph=True)
        gx, mag = R.upsample_bwd_ref(gy, s)
        assert bool(((gx - _nhwc(gt)).abs() <= s * s * EPS64 * mag).all())
        if float(gy.frac().abs().max()) == 0.0:
            assert torch.equal(gx, _nhwc(gt))


def test_activation_references_match_torch_fp64():
    x = R.act_inputs().double()
    gy = torch.randn(x.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    for act, fn in ((R.ACT_RELU, F.relu), (R.ACT_SILU, F.silu), (R.ACT_TANH, torch.tanh)):
        xt = x.clone().requires_grad_()
        want = fn(xt)
        (gt,) = torch.autograd.grad(want, xt, gy)
        got, _ = R.act_ref(act, x)
        grad, _ = R.act_grad_ref(act, x, gy)
        want = want.detach()
        assert torch.equal(got != got, want != want) and torch.equal(grad != grad, gt != gt), act
        ok = want == want
        if act == R.ACT_RELU:
            assert torch.equal(got[ok], want[ok]) and torch.equal(grad[gt == gt], gt[gt == gt])
            continue
        ok &= got != want                                   # (equal infinities: nothing to subtract)
        assert bool(((got - want)[ok].abs() <= 8 * EPS64 * want[ok].abs()).all()), act
        okg = (gt == gt) & (grad != gt)
        assert bool(((grad - gt)[okg].abs() <= 16 * EPS64 * gy[okg].abs()).all()), act


def test_small_gemm_reference_matches_torch_fp64():
    g = torch.Generator().manual_seed(9)
    for M, N, K in ((1, 1, 1), (5, 7, 129), (33, 2, 64)):
        a, b = torch.randn((M, K), generator=g, dtype=torch.float64), torch.randn((K, N), generator=g, dtype=torch.float64)
        for ta in (False, True):
            for tb in (False, True):
                c, mag = R.small_gemm_ref(a.t().contiguous() if ta else a, ta, b.t().contiguous() if tb else b, tb)
                assert bool(((c - a @ b).abs() <= (K + 2) * EPS64 * mag).all())
                assert bool((mag >= c.abs() * (1 - 1e-12)).all())


def test_ulps_counts_fp32_units():
    one = torch.tensor([1.0, 1.0, 3.0, 0.0, math.nan, math.inf, math.inf, 1.0], dtype=torch.float64)
    out = torch.tensor([1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24, 3.0 + 2.0 ** -21, 2.0 ** -149, math.nan, math.inf, 1.0, math.nan],
                       dtype=torch.float64)
    assert R.ulps(out, one).tolist() == [1.0, 0.5, 2.0, 1.0, 0.0, 0.0, math.inf, math.inf]


# ------------------------------------------------------------------------------------------ argument checks
def _owned(n):
    """n floats the test owns, on the device when there is one (a library that launched instead of refusing would then
    still read and write only this memory)."""
    t = torch.zeros(n, device="cuda" if torch.cuda.is_available() else "cpu")
    return t, t.data_ptr()


def _refused(lib, name, *args):
    rc = getattr(lib, name)(*args)
    msg = lib.snn_last_error().decode()
    assert rc == 1, (name, args, rc, msg)          # 1: refused on the host; 2 would be a failed launch
    return msg


def test_refusals_return_before_any_launch(hip_lib):
    keep, p = _owned(4096)
    big = 1 << 20
    cases = []
    for fn in ("snn_nchw_to_nhwc", "snn_nhwc_to_nchw"):
        ok = [p, p, 2, 8, 3, 3, None]
        cases += [(fn, ok, 0, None), (fn, ok, 1, None), (fn, ok, 2, 0), (fn, ok, 3, 0), (fn, ok, 4, -1), (fn, ok, 5, 0),
                  (fn, ok, 2, 65536)]
    ok = [p, p, 4, 3, 3, 4, None]
    cases += [("snn_weight_transpose", ok, i, v) for i, v in ((0, None), (1, None), (2, 0), (3, 0), (4, -3), (5, 0))]
    ok = [p, p, p, 2, None]
    cases += [("snn_weight_transpose_batched", ok, i, v) for i, v in ((0, None), (1, None), (2, None), (3, 0), (3, 65536))]
    for fn in ("snn_copy_channels", "snn_add_channels", "snn_copy_channels_bf16"):
        ok = [p, 8, p, 8, 4, 8, None]
        cases += [(fn, ok, i, v) for i, v in ((0, None), (2, None), (4, 0), (4, -1), (5, 0), (1, 7), (3, 7))]
    for fn in ("snn_add", "snn_add_bf16"):
        ok = [p, 8, p, 8, p, 8, 4, 8, None]
        cases += [(fn, ok, i, v) for i, v in ((0, None), (2, None), (4, None), (6, 0), (7, 0), (7, -2), (1, 7), (3, 7), (5, 7))]
    ok = [p, p, 16, 1, None]
    cases += [("snn_convert_bf16", ok, i, v) for i, v in ((0, None), (1, None), (2, 0), (2, -1))]
    ok = [0, p, p, 16, None]
    cases += [("snn_act_fwd", ok, i, v) for i, v in ((1, None), (2, None), (3, 0), (0, -1), (0, 3))]
    ok = [0, p, p, p, p, 16, None]
    cases += [("snn_act_bwd", ok, i, v) for i, v in ((1, None), (2, None), (3, None), (4, None), (5, 0), (0, -1), (0, 3))]
    ok = [0, p, p, 1, 4, 4, 2, 2, 2, 2, 2, None]
    cases += [("snn_pool_fwd", ok, i, v) for i, v in ((1, None), (2, None), (3, 0), (4, 0), (5, 0), (6, 0), (9, 0), (10, 0),
                                                      (0, -1), (0, 3), (7, 3), (8, 1), (7, 0), (9, 5))]
    ok = [1, p, p, p, 1, 4, 4, 2, 2, 2, 2, 2, None]
    cases += [("snn_pool_bwd", ok, i, v) for i, v in ((1, None), (2, None), (3, None), (4, 0), (5, 0), (6, 0), (7, 0), (10, 0),
                                                      (11, 0), (0, -1), (0, 3), (8, 3), (9, 1), (8, 0), (9, big), (10, 5))]
    for fn in ("snn_upsample_fwd", "snn_upsample_bwd"):
        ok = [p, p, 1, 2, 2, 2, 2, None]
        cases += [(fn, ok, i, v) for i, v in ((0, None), (1, None), (2, 0), (3, 0), (4, 0), (5, 0), (6, 0), (6, -1))]
    #      A  lda tA B  ldb tB C  ldc M  N  K  acc Ct    ldct
    ok = [p, 8, 0, p, 8, 0, p, 8, 4, 8, 8, 0, None, 0, None]
    cases += [("snn_small_gemm", ok, i, v) for i, v in ((0, None), (3, None), (6, None), (8, 0), (9, 0), (10, -1), (1, 7),
                                                        (4, 7), (7, 7))]
    cases += [("snn_small_gemm", [p, 3, 1, p, 8, 0, p, 8, 4, 8, 8, 0, None, 0, None], 1, 3),     # A^T: rows of M
              ("snn_small_gemm", [p, 8, 0, p, 7, 1, p, 8, 4, 8, 8, 0, None, 0, None], 4, 7),     # B^T: rows of K
              ("snn_small_gemm", [p, 8, 0, p, 8, 0, p, 8, 4, 8, 8, 1, p, 4, None], 11, 1),       # Ct with accumulate
              ("snn_small_gemm", [p, 8, 0, p, 8, 0, p, 8, 4, 8, 8, 0, p, 3, None], 13, 3)]       # ldct < M
    ok = [p, p, p, p, p, 2, 4, None]
    cases += [("snn_small_gemm_batched", ok, i, v) for i, v in ((0, None), (1, None), (2, None), (4, None), (5, 0), (5, 65536),
                                                                (6, 0))]
    assert len(cases) == 146
    for fn, ok, i, v in cases:
        args = list(ok)
        args[i] = v
        msg = _refused(hip_lib, fn, *args)
        assert msg.startswith(fn + ":"), (fn, i, v, msg)
    # bad act / kind name the value where the message has one
    assert "bad pool kind 7" in _refused(hip_lib, "snn_pool_fwd", 7, p, p, 1, 4, 4, 2, 2, 2, 2, 2, None)
    assert "bad pool kind -2" in _refused(hip_lib, "snn_pool_bwd", -2, p, p, p, 1, 4, 4, 2, 2, 2, 2, 2, None)
    assert "max pooling needs" in _refused(hip_lib, "snn_pool_bwd", 1, None, p, p, 1, 4, 4, 2, 2, 2, 2, 2, None)
    del keep


def test_pool_window_larger_than_the_image_is_refused(hip_lib):
    """H = 2, k = 3, stride = 2: (H - k) / stride + 1 is 1 in C (division truncates toward zero), so the output-size check
    alone lets the call through and the window reads a third row.  The buffers below hold the 3x3 window the call names."""
    keep, p = _owned(4096)
    for H, W in ((2, 2), (2, 8), (8, 2)):
        Ho, Wo = (H - 3) // 2 + 1 if H >= 3 else 1, (W - 3) // 2 + 1 if W >= 3 else 1
        for kind in (0, 1, 2):
            msg = _refused(hip_lib, "snn_pool_fwd", kind, p, p + 2048, 1, H, W, 2, Ho, Wo, 3, 2, None)
            assert msg.startswith("snn_pool_fwd: window 3 larger than the"), msg
            msg = _refused(hip_lib, "snn_pool_bwd", kind, p, p + 1024, p + 2048, 1, H, W, 2, Ho, Wo, 3, 2, None)
            assert msg.startswith("snn_pool_bwd: window 3 larger than the"), msg
    del keep


def test_pool_bwd_requires_the_forward_geometry(hip_lib):
    keep, p = _owned(4096)
    # H = W = 7, k = 3, stride = 2 -> 3 x 3 windows; anything else is refused (gy and gx are sized for 7 x 7 either way)
    for Ho, Wo in ((4, 3), (3, 4), (2, 3), (3, 2), (7, 7), (0, 3), (3, -1)):
        for kind in (0, 1, 2):
            msg = _refused(hip_lib, "snn_pool_bwd", kind, p, p + 1024, p + 2048, 1, 7, 7, 2, Ho, Wo, 3, 2, None)
            assert msg == "snn_pool_bwd: output size mismatch", msg
            msg = _refused(hip_lib, "snn_pool_fwd", kind, p, p + 2048, 1, 7, 7, 2, Ho, Wo, 3, 2, None)
            assert msg == "snn_pool_fwd: output size mismatch", msg
    del keep
