"""The three depthwise-convolution entry points (csrc/conv_depthwise.hip) per element against fp64, on every operand layout.

snn_dwconv_fwd / _dgrad / _wgrad take channel slices of wider channels-last buffers at any channel offset and a weight
(image or gradient) at any float of a flat buffer; the host side picks 16-byte or guarded scalar accesses per call.  Each
test runs ONE set of values through the layouts of test_gpu_conv_layouts._layouts and checks

* per element |out - ref| <= 2^-19 * mag + 1e-12 (conv_ref's bound for "fp32": exact products; at most 32 of them are added
  in fp32 - 25 taps in forward / data gradient, 32 pixels per lane in the weight gradient - before fp64 takes over), mag the
  same fp64 operation on |operands|, plus the norm-wise 1e-5;
* that every output element was written (outputs start as NaN), that nothing around a slice changed, bit for bit, and that
  the inputs are unchanged;
* that the check has teeth: a reference with one tap dropped, the padding shifted by one, or one stride-2 phase class
  zeroed must FAIL it.

Shapes: K in {3, 5} x stride in {1, 2}; C in {1, 3, 4, 36, 260} (scalar only; a vector body; more channel groups than the
64 lanes of a wave, and, in the weight gradient, than one block's 64 channel lanes); maps from 1x1 (narrower than a lane's
run of 4 / 2 output pixels) to 8x9, odd and even for stride 2; N in {1, 3}."""
import pytest
import torch

from tests.dwconv_ref import _check, _teeth, dw_dgrad_ref, dw_fwd_ref, dw_geom, dw_wgrad_ref, shifted
from tests.test_gpu_conv_layouts import Flat, Slab, _layouts

gpu = pytest.mark.gpu

KS = [(3, 1), (3, 2), (5, 1), (5, 2)]
CHANNELS = [1, 3, 4, 36, 260]
MAPS = [(1, 1), (2, 3), (7, 10), (8, 9)]
BATCHES = [1, 3]
CASES = [(K, s, C) for K, s in KS for C in CHANNELS]
IDS = [f"k{K}s{s}-c{C}" for K, s, C in CASES]


@pytest.fixture(scope="module")
def H_(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from snn_for_object_detection_amd import _hip
    return _hip


def _data(N, H, W, C, K, s, seed):
    g = torch.Generator().manual_seed(seed)
    pad, Ho, Wo = dw_geom(H, W, K, s)
    x = torch.randn(N, H, W, C, generator=g)
    w = torch.randn(C, K, K, generator=g) / K
    dy = torch.randn(N, Ho, Wo, C, generator=g)
    return pad, Ho, Wo, x, w, dy


def _tap_major(w):
    """[C,K,K] -> the kernels' weight image [K*K][C]."""
    C, K = w.shape[0], w.shape[-1]
    return w.reshape(C, K * K).t().contiguous()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _shapes():
    for H, W in MAPS:
        for N in BATCHES:
            yield N, H, W


# ---------------------------------------------------------------------------------------------------- forward
def _run_fwd(_hip, x, w, N, H, W, C, K, s, lx, ly, woff=0):
    pad, Ho, Wo = dw_geom(H, W, K, s)
    X = Slab(N, H, W, C, lx[1], lx[2], values=x)
    WT = Flat((K * K, C), woff, values=_tap_major(w))
    Y = Slab(N, Ho, Wo, C, ly[1], ly[2], fill=float("nan"))
    _hip.call("snn_dwconv_fwd", X.ptr, X.ld, WT.ptr, Y.ptr, Y.ld, N, H, W, C, K, s, pad, _stream())
    torch.cuda.synchronize()
    assert X.guards_intact(whole=True) and WT.guards_intact(whole=True), "snn_dwconv_fwd changed an input"
    assert Y.guards_intact(), "snn_dwconv_fwd wrote outside its output slice"
    return Y.value()


def _layout_runs(C):
    L = _layouts(C)
    runs = [(f"in:{l[0]}", l, L[0], 0) for l in L] + [(f"out:{l[0]}", L[0], l, 0) for l in L[1:]]
    runs += [(f"w+{o}", L[0], L[0], o) for o in (1, 2, 3)]
    runs += [("in:off2,out:ld_odd,w+1", L[3], L[5], 1), ("in:merge,out:merge", L[1], L[1], 0)]
    return runs


@gpu
@pytest.mark.parametrize("K,s,C", CASES, ids=IDS)
def test_forward_per_element_on_every_layout(H_, K, s, C):
    _hip = H_
    for N, H, W in _shapes():
        assert _hip.query("snn_dwconv_supported", N, H, W, C, K, s, K // 2) == 1
        pad, Ho, Wo, x, w, _ = _data(N, H, W, C, K, s, seed=7 * C + H)
        xd, wd = x.double(), w.double()
        ref, mag = dw_fwd_ref(xd, wd, s), dw_fwd_ref(xd.abs(), wd.abs(), s)
        for what, lx, ly, woff in _layout_runs(C):
            out = _run_fwd(_hip, x, w, N, H, W, C, K, s, lx, ly, woff)
            _check(f"fwd {N}x{H}x{W} {what}", out, ref, mag, "fp32")
            if what == "in:dense":
                ww = wd.clone()
                ww[:, K // 2, K // 2] = 0                                      # one tap dropped (the one every pixel has)
                _teeth("fwd tap", out, dw_fwd_ref(xd, ww, s), mag, "fp32")
                _teeth("fwd padding", out, dw_fwd_ref(shifted(xd), wd, s), mag, "fp32")   # padding shifted by one


# ---------------------------------------------------------------------------------------------------- data gradient
def _run_dgrad(_hip, dy, w, N, H, W, C, K, s, ly, lx, woff=0):
    pad, Ho, Wo = dw_geom(H, W, K, s)
    DY = Slab(N, Ho, Wo, C, ly[1], ly[2], values=dy)
    WT = Flat((K * K, C), woff, values=_tap_major(w))
    DX = Slab(N, H, W, C, lx[1], lx[2], fill=float("nan"))
    _hip.call("snn_dwconv_dgrad", DY.ptr, DY.ld, WT.ptr, DX.ptr, DX.ld, N, H, W, C, K, s, pad, _stream())
    torch.cuda.synchronize()
    assert DY.guards_intact(whole=True) and WT.guards_intact(whole=True), "snn_dwconv_dgrad changed an input"
    assert DX.guards_intact(), "snn_dwconv_dgrad wrote outside its output slice"
    return DX.value()


@gpu
@pytest.mark.parametrize("K,s,C", CASES, ids=IDS)
def test_data_gradient_per_element_on_every_layout(H_, K, s, C):
    _hip = H_
    for N, H, W in _shapes():
        pad, Ho, Wo, _, w, dy = _data(N, H, W, C, K, s, seed=5 * C + W)
        dyd, wd = dy.double(), w.double()
        ref, mag = dw_dgrad_ref(dyd, wd, H, W, s), dw_dgrad_ref(dyd.abs(), wd.abs(), H, W, s)
        for what, ly, lx, woff in _layout_runs(C):
            out = _run_dgrad(_hip, dy, w, N, H, W, C, K, s, ly, lx, woff)
            _check(f"dgrad {N}x{H}x{W} {what}", out, ref, mag, "fp32")
            if what == "in:dense":
                ww = wd.clone()
                ww[:, K // 2, K // 2] = 0                                      # one tap dropped
                _teeth("dgrad tap", out, dw_dgrad_ref(dyd, ww, H, W, s), mag, "fp32")
                _teeth("dgrad padding", out, shifted(ref), mag, "fp32")        # every dx pixel one column off
                if s == 2:
                    wrong = ref.clone()
                    wrong[:, 0::2, 0::2] = 0                                   # one stride-2 phase class zeroed
                    _teeth("dgrad phase", out, wrong, mag, "fp32")


# ---------------------------------------------------------------------------------------------------- weight gradient
def _run_wgrad(_hip, x, dy, N, H, W, C, K, s, lx, ly, doff=0, prev=None, chunks=0):
    pad, Ho, Wo = dw_geom(H, W, K, s)
    X = Slab(N, H, W, C, lx[1], lx[2], values=x)
    DY = Slab(N, Ho, Wo, C, ly[1], ly[2], values=dy)
    DW = Flat((C, K, K), doff, values=prev) if prev is not None else Flat((C, K, K), doff, fill=float("nan"))
    n_ws = _hip.query("snn_dwconv_wgrad_workspace_size", N, H, W, C, K, s, pad, chunks)
    assert n_ws >= max(chunks, 1) * C * K * K * 8
    ws = torch.full((n_ws // 8 + 2,), float("nan"), dtype=torch.float64, device="cuda")   # (NaN: a row nobody wrote shows)
    ws[n_ws // 8:] = 77.0
    _hip.call("snn_dwconv_wgrad", X.ptr, X.ld, DY.ptr, DY.ld, DW.ptr, N, H, W, C, K, s, pad, int(prev is not None),
              ws.data_ptr(), chunks, _stream())
    torch.cuda.synchronize()
    assert X.guards_intact(whole=True) and DY.guards_intact(whole=True), "snn_dwconv_wgrad changed an input"
    assert DW.guards_intact(), "snn_dwconv_wgrad wrote outside dw"
    assert bool((ws[n_ws // 8:] == 77.0).all()), "snn_dwconv_wgrad wrote past the workspace it asked for"
    return DW


def _ragged(P):
    """A chunk count >= 3 that does not divide the P pixels: the last chunk is shorter than the others (P = 1: empty)."""
    for n in (3, 4, 5, 7):
        if P % n:
            return n
    return 3


@gpu
@pytest.mark.parametrize("K,s,C", CASES, ids=IDS)
def test_weight_gradient_per_element_on_every_layout(H_, K, s, C):
    _hip = H_
    L = _layouts(C)
    for N, H, W in _shapes():
        pad, Ho, Wo, x, _, dy = _data(N, H, W, C, K, s, seed=3 * C + H + W)
        xd, dyd = x.double(), dy.double()
        ref, mag = dw_wgrad_ref(xd, dyd, K, s), dw_wgrad_ref(xd.abs(), dyd.abs(), K, s)
        runs = [(f"x:{l[0]}", l, L[0]) for l in L] + [(f"dy:{l[0]}", L[0], l) for l in L[1:]]
        runs += [("x:off2,dy:ld_odd", L[3], L[5]), ("x:merge,dy:merge", L[1], L[1])]
        for what, lx, ly in runs:
            out = _run_wgrad(_hip, x, dy, N, H, W, C, K, s, lx, ly).value()
            _check(f"wgrad {N}x{H}x{W} {what}", out, ref, mag, "fp32")
            if what == "x:dense":
                xw = xd.clone()
                xw[:, 0, 0] = 0                                                # one pixel's products dropped
                _teeth("wgrad pixel", out, dw_wgrad_ref(xw, dyd, K, s), mag, "fp32")
                _teeth("wgrad padding", out, dw_wgrad_ref(shifted(xd), dyd, K, s), mag, "fp32")
                wrong = ref.clone()
                wrong[:, K // 2, K // 2] = 0                                   # one tap dropped
                _teeth("wgrad tap", out, wrong, mag, "fp32")
        # dw at flat offsets 0 .. 3 of a larger buffer, stored and accumulated
        prev = torch.randn(C, K, K, generator=torch.Generator().manual_seed(C + K))
        for doff in range(4):
            out = _run_wgrad(_hip, x, dy, N, H, W, C, K, s, L[0], L[0], doff).value()
            _check(f"wgrad {N}x{H}x{W} dw+{doff}", out, ref, mag, "fp32")
            out = _run_wgrad(_hip, x, dy, N, H, W, C, K, s, L[1], L[2], doff, prev=prev).value()
            _check(f"wgrad {N}x{H}x{W} dw+{doff} accumulate", out, ref + prev.double(), mag, "fp32",
                   extra_mag=prev.double().abs())
        # the chunk count forced: one chunk, a ragged last chunk, more chunks than pixels; the same bits twice
        P = N * Ho * Wo
        for chunks in (1, _ragged(P), P + 5):
            for lx, ly in ((L[0], L[0]), (L[2], L[1])):
                a = _run_wgrad(_hip, x, dy, N, H, W, C, K, s, lx, ly, chunks=chunks)
                b = _run_wgrad(_hip, x, dy, N, H, W, C, K, s, lx, ly, chunks=chunks)
                _check(f"wgrad {N}x{H}x{W} {chunks} chunks x:{lx[0]}", a.value(), ref, mag, "fp32")
                assert torch.equal(a.buf.view(torch.int32), b.buf.view(torch.int32)), f"wgrad {chunks} chunks: two runs differ"


@gpu
@pytest.mark.parametrize("K,C", [(3, 256), (5, 128)], ids=["k3", "k5"])
def test_weight_gradient_long_sums_continue_in_fp64(H_, K, C):
    """A map large enough that a lane of the weight gradient passes its 32 fp32 terms many times inside one chunk (64
    channel lanes leave 4 pixel lanes: one forced chunk of 3 x 40 x 48 pixels is 45 rounds of 128 pixels), and the planned
    chunking of the same call: the same per-element bound, which an fp32 sum over all 5760 pixels is not held to."""
    _hip = H_
    N, H, W, s = 3, 40, 48, 1
    pad, Ho, Wo, x, _, dy = _data(N, H, W, C, K, s, seed=99)
    x, dy = x.abs(), dy.abs()                     # same-sign products: the rounding errors of a running sum do not cancel
    xd, dyd = x.double(), dy.double()
    ref = dw_wgrad_ref(xd, dyd, K, s)
    L = _layouts(C)
    for chunks in (1, 0):
        out = _run_wgrad(_hip, x, dy, N, H, W, C, K, s, L[0], L[1], chunks=chunks).value()
        _check(f"wgrad long sums, chunks {chunks}", out, ref, ref, "fp32")


@gpu
def test_launchers_refuse_what_the_query_refuses(H_):
    _hip = H_
    t = torch.zeros(64, device="cuda")
    for K, s, pad in ((7, 1, 3), (3, 3, 1), (3, 1, 0), (4, 1, 2)):
        assert _hip.query("snn_dwconv_supported", 1, 2, 2, 4, K, s, pad) == 0
        assert _hip.query("snn_dwconv_wgrad_workspace_size", 1, 2, 2, 4, K, s, pad, 0) == 0
        with pytest.raises(RuntimeError, match="not covered"):
            _hip.call("snn_dwconv_fwd", t.data_ptr(), 4, t.data_ptr(), t.data_ptr(), 4, 1, 2, 2, 4, K, s, pad, _stream())
        with pytest.raises(RuntimeError, match="not covered"):
            _hip.call("snn_dwconv_dgrad", t.data_ptr(), 4, t.data_ptr(), t.data_ptr(), 4, 1, 2, 2, 4, K, s, pad, _stream())
        with pytest.raises(RuntimeError, match="not covered"):
            _hip.call("snn_dwconv_wgrad", t.data_ptr(), 4, t.data_ptr(), 4, t.data_ptr(), 1, 2, 2, 4, K, s, pad, 0,
                      t.data_ptr(), 0, _stream())
