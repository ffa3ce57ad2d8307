"""Every load / store path of the convolution entry points on the operand layouts the model hands them, against fp64.

The zero-copy Dense / C2f merge gives the convolutions channel slices of wider channels-last buffers (pixel stride >
channel count), outputs at a channel offset inside a concat buffer and data gradients that are slices of a concat
gradient; FlatTrainer puts every weight into one flat buffer without padding, so a weight starts on any float.  The host
side of csrc/conv_gather.hip and csrc/conv_wgrad.hip picks a different kernel for each of these (launch_gather: vec / fast /
out_vec; wgrad_common: the
event-frame row kernels, the halo-resident weight gradient and its drop to the implicit GEMM, pipelined or not), so each
test here runs ONE set of values through every layout and checks:

* per element, against torch's CPU convolution in float64 over exactly the values of the slice, with a bound scaled by
  the same operation on |operands| (no channel or pixel can hide behind a norm), plus the norm-wise bound of
  test_gpu_ops.py::test_conv2d_fwd_bwd;
* that every output element was written (outputs start as NaN) and nothing around a slice changed (bit for bit);
* that the metric has teeth: a float64 reference that is wrong in a small way (one channel dropped, padding shifted,
  one stride-phase class zeroed) must FAIL it.

The spike-operand entry points (z = (v_dec > v_th) formed on load) must give the plain kernel's bits on the stored spikes
wherever functional routes a layer to them, and functional must route every layout they cannot run to the plain path
(host-side table test below, no GPU).  The last two tests are the model-level regressions of that routing.

Layouts select the branches; the SNN_CONV_NO_FAST / SNN_WGRAD_NO_PIPE tuning switches are never used.  Every slice lies
inside an allocation with guard channels and guard pixels at both ends, and no kernel gets a buffer smaller than its
geometry says.
"""
import ctypes

import pytest
import torch

from tests.conv_ref import _check, _dgrad_ref, _fwd_ref, _teeth, _wgrad_ref
from tests.util import rel_err, synthetic_events

gpu = pytest.mark.gpu

SENT = 77.0          # the channels and pixels around a slice: far outside the data, so a stray read shows as well
GUARD = 4            # guard pixels at each end of a buffer: 4 * ld floats is a multiple of 16 bytes, so the channel
                     # offset alone sets the slice's alignment


@pytest.fixture(scope="module")
def H_(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from snn_for_object_detection_amd import _hip
    return _hip


def _prec(_hip, name):
    return {"fp16x3": _hip.PREC_FP16X3, "bf16x6": _hip.PREC_BF16X6, "fp32": _hip.PREC_FP32, "bf16x3": _hip.PREC_BF16X3,
            "bf16x1": _hip.PREC_BF16X1}[name]


# ---------------------------------------------------------------------------------------------------- layouts
def _layouts(C):
    """(name, channel offset, pixel stride) of a C-channel operand: the layouts the model produces."""
    r4 = (C + 3) // 4 * 4
    ld_odd = C + 1 if (C + 1) % 4 else C + 2
    return [("dense", 0, C),                  # freshly allocated tensor: the baseline
            ("merge", 4, r4 + 8),             # Dense merge slice: 16-byte aligned, ld % 4 == 0, ld > C
            ("off1", 1, r4 + 4),              # 4-byte aligned only: vec / out_vec / pipe refuse it
            ("off2", 2, r4 + 4),              # 8-byte aligned: what the event-frame kernels' aligned(8, ...) accepts
            ("off3", 3, r4 + 4),
            ("ld_odd", 0, ld_odd)]            # aligned start, but the pixel stride breaks every 4-wide access


class Slab:
    """Channels-last operand [N,H,W,C] = channels off .. off+C of a [GUARD + N*H*W + GUARD, ld] buffer whose other
    elements hold SENT."""

    def __init__(self, N, H, W, C, off=0, ld=None, values=None, fill=None):
        ld = C if ld is None else ld
        assert 0 <= off and off + C <= ld
        P = N * H * W
        self.shape, self.ld = (N, H, W, C), ld
        self.buf = torch.full((P + 2 * GUARD, ld), SENT, device="cuda")
        self.view = self.buf[GUARD:GUARD + P, off:off + C]
        if values is not None:
            self.view.copy_(values.reshape(P, C))
        elif fill is not None:
            self.view.fill_(fill)
        self.ptr = self.view.data_ptr()
        self.mask = torch.zeros(self.buf.shape, dtype=torch.bool, device="cuda")
        self.mask[GUARD:GUARD + P, off:off + C] = True
        self.before = self.buf.clone()

    def value(self):
        return self.view.double().cpu().reshape(self.shape)

    def guards_intact(self, whole=False):
        """Nothing outside the slice changed, bit for bit (whole: not inside either - an input)."""
        keep = torch.ones_like(self.mask) if whole else ~self.mask
        return torch.equal(self.buf.view(torch.int32)[keep], self.before.view(torch.int32)[keep])


class Flat:
    """A dense tensor at float offset `off` of a larger allocation (a parameter of FlatTrainer's flat buffer)."""

    def __init__(self, shape, off=0, values=None, fill=None):
        n = 1
        for s in shape:
            n *= s
        self.shape, self.off, self.n = tuple(shape), off, n
        self.buf = torch.full((n + 8,), SENT, device="cuda")
        if values is not None:
            self.buf[off:off + n] = values.reshape(-1).to(self.buf.device)
        elif fill is not None:
            self.buf[off:off + n] = fill
        self.ptr = self.buf[off:].data_ptr()
        self.before = self.buf.clone()

    def value(self):
        return self.buf[self.off:self.off + self.n].double().cpu().reshape(self.shape)

    def guards_intact(self, whole=False):
        a, b = self.buf.view(torch.int32), self.before.view(torch.int32)
        if whole:
            return torch.equal(a, b)
        return torch.equal(a[:self.off], b[:self.off]) and torch.equal(a[self.off + self.n:], b[self.off + self.n:])


def _geom(H, W, k, s):
    pad = k // 2
    return pad, (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1


CASES = [
    # N, H, W, Cin, Cout, k, s      branches taken on the dense layout (other layouts: see _layouts)
    (2, 17, 23, 2, 16, 3, 2),     # event-frame layer: k_conv_first row kernels (fwd; wgrad while ldx % 2 == 0, x 8-byte
                                  # aligned, lddy % 4 == 0, dy 16-byte aligned), scalar gather otherwise; odd H, W
    (1, 11, 9, 64, 32, 3, 2),     # Cin % 32: the pipelined implicit GEMM (fast) and k_conv_wgrad_pipe; stride 2, odd H, W
    (2, 7, 10, 32, 36, 1, 1),     # 1x1, Cin % 32, Cout = 36 (a 64-wide tile, not a multiple of 32)
    (1, 9, 11, 12, 20, 5, 1),     # Cin % 4 but not % 32: vec, not fast; non-pipelined k_conv_wgrad<vec>; 5x5
    (1, 8, 7, 7, 5, 3, 2),        # odd Cin and Cout: scalar gather and scalar stores, k_conv_wgrad<scalar>
    (1, 5, 6, 96, 27, 1, 1),      # the head's class convolution: Cout = 27
    (1, 13, 11, 32, 64, 5, 2),    # 5x5 stride 2 pipelined, 42 output pixels (not a multiple of the 128-pixel tile)
    (2, 9, 13, 64, 64, 3, 1),     # 3x3 stride 1, 64 channels: the implicit GEMM (fwd, dgrad), pipelined while aligned
]
CASE_IDS = ["first", "pipe-s2", "1x1-c36", "vec-5x5", "scalar-odd", "head-c27", "pipe-5x5-s2", "pipe-3x3"]


def _case_data(N, H, W, Cin, Cout, k, s, seed):
    g = torch.Generator().manual_seed(seed)
    pad, Ho, Wo = _geom(H, W, k, s)
    x = torch.randn(N, H, W, Cin, generator=g)
    w = torch.randn(Cout, k, k, Cin, generator=g) / (Cin * k * k) ** 0.5
    dy = torch.randn(N, Ho, Wo, Cout, generator=g)
    return pad, Ho, Wo, x, w, dy


# ---------------------------------------------------------------------------------------------------- forward
def _run_fwd(_hip, x, w, shape, prec, lx, ly, woff=0, addend=None, la=None, bn=False):
    """snn_conv2d_fwd on the given layouts; returns (y slab, sums of the BatchNorm partials or None)."""
    N, H, W, Cin, Cout, k, s = shape
    pad, Ho, Wo = _geom(H, W, k, s)
    st = torch.cuda.current_stream().cuda_stream
    X = Slab(N, H, W, Cin, lx[1], lx[2], values=x)
    Wt = Flat(w.shape, woff, values=w)
    Y = Slab(N, Ho, Wo, Cout, ly[1], ly[2], fill=float("nan"))
    A = Slab(N, Ho, Wo, Cout, la[1], la[2], values=addend) if addend is not None else None
    part = lay = None
    fps = 1
    if bn:
        part = torch.zeros(_hip.query("snn_conv2d_fwd_bn_partial_size", N, fps, Ho, Wo, Cout), dtype=torch.float64,
                           device="cuda")
        lay = (ctypes.c_int * 2)()
    _hip.call("snn_conv2d_fwd", X.ptr, X.ld, Wt.ptr, None, Y.ptr, Y.ld, N, H, W, Cin, Ho, Wo, Cout, k, k, s, pad,
              A.ptr if A else None, A.ld if A else 0, part.data_ptr() if bn else None, fps, lay, _prec(_hip, prec), st)
    sums = None
    if bn and lay[0] > 0:
        sums = torch.empty(N // fps, Cout, 2, dtype=torch.float64, device="cuda")
        _hip.call("snn_bn_stats_reduce", part.data_ptr(), lay[0], lay[1], N // fps, fps * Ho * Wo, Cout, sums.data_ptr(), st)
    torch.cuda.synchronize()
    assert X.guards_intact(whole=True) and Wt.guards_intact(whole=True) and (A is None or A.guards_intact(whole=True))
    assert Y.guards_intact(), "snn_conv2d_fwd wrote outside its output slice"
    return Y, (None if sums is None else sums.cpu())


@gpu
@pytest.mark.parametrize("shape", CASES, ids=CASE_IDS)
def test_forward_on_every_layout(H_, shape):
    _hip = H_
    N, H, W, Cin, Cout, k, s = shape
    pad, Ho, Wo, x, w, _ = _case_data(*shape, seed=Cin * 7 + Cout)
    a = torch.randn(N, Ho, Wo, Cout, generator=torch.Generator().manual_seed(3))
    xd, wd, ad = x.double(), w.double(), a.double()
    ref, mag = _fwd_ref(xd, wd, s, pad), _fwd_ref(xd.abs(), wd.abs(), s, pad)
    lx_d, ly_d = _layouts(Cin)[0], _layouts(Cout)[0]
    runs = [(f"x:{L[0]}", L, ly_d, 0) for L in _layouts(Cin)] + [(f"y:{L[0]}", lx_d, L, 0) for L in _layouts(Cout)[1:]]
    runs += [(f"w+{o}", lx_d, ly_d, o) for o in (1, 2, 3)]
    runs += [("x:off2,y:ld_odd,w+1", _layouts(Cin)[3], _layouts(Cout)[5], 1)]
    for what, lx, ly, woff in runs:
        Y, _ = _run_fwd(_hip, x, w, shape, "fp16x3", lx, ly, woff)
        out = Y.value()
        _check(f"fwd {what}", out, ref, mag, "fp16x3")
        if what == "x:dense":
            c = Cin // 2
            xw = xd.clone()
            xw[..., c] = 0                                      # one input channel dropped
            _teeth("fwd", out, _fwd_ref(xw, wd, s, pad), mag, "fp16x3")
    # fused addend (y = conv + addend) on its own layouts, and the output at a slice at the same time
    for L in _layouts(Cout):
        Y, _ = _run_fwd(_hip, x, w, shape, "fp16x3", lx_d, _layouts(Cout)[2], 0, addend=a, la=L)
        _check(f"fwd addend:{L[0]}", Y.value(), ref + ad, mag, "fp16x3", extra_mag=ad.abs())
    # BatchNorm statistics partials out of the epilogue: y as before, the per-(t,c) sums those of the stored values
    for lx, ly in ((lx_d, ly_d), (_layouts(Cin)[1], _layouts(Cout)[1]), (_layouts(Cin)[2], _layouts(Cout)[3])):
        Y, sums = _run_fwd(_hip, x, w, shape, "fp16x3", lx, ly, bn=True)
        out = Y.value()
        _check(f"fwd bn x:{lx[0]} y:{ly[0]}", out, ref, mag, "fp16x3")
        if sums is not None:
            yt = out.reshape(N, -1, Cout)
            want = torch.stack([yt.sum(1), (yt * yt).sum(1)], -1)
            scale = torch.stack([yt.abs().sum(1), (yt * yt).sum(1)], -1)
            # (the event-frame row kernel sums a few pixels of a row in fp32 first: 1e-6, test_gpu_ops.py)
            assert bool(((sums - want).abs() <= 1e-6 * scale + 1e-12).all()), f"bn partials x:{lx[0]} y:{ly[0]}"


@gpu
@pytest.mark.parametrize("prec", ["bf16x6", "fp32"])
@pytest.mark.parametrize("shape", [CASES[1], CASES[4], CASES[7]], ids=[CASE_IDS[1], CASE_IDS[4], CASE_IDS[7]])
def test_forward_arithmetic_modes_on_slices(H_, shape, prec):
    _hip = H_
    pad, Ho, Wo, x, w, _ = _case_data(*shape, seed=11)
    xd, wd = x.double(), w.double()
    ref, mag = _fwd_ref(xd, wd, shape[6], pad), _fwd_ref(xd.abs(), wd.abs(), shape[6], pad)
    Lx, Ly = _layouts(shape[3]), _layouts(shape[4])
    for lx, ly, woff in ((Lx[0], Ly[0], 0), (Lx[1], Ly[2], 0), (Lx[3], Ly[5], 3), (Lx[5], Ly[1], 1)):
        Y, _ = _run_fwd(_hip, x, w, shape, prec, lx, ly, woff)
        _check(f"fwd {prec} x:{lx[0]} y:{ly[0]} w+{woff}", Y.value(), ref, mag, prec)


# ---------------------------------------------------------------------------------------------------- data gradient
def _run_dgrad(_hip, dy, w, shape, prec, ldy_, ldx_, woff=0, adds=()):
    N, H, W, Cin, Cout, k, s = shape
    pad, Ho, Wo = _geom(H, W, k, s)
    st = torch.cuda.current_stream().cuda_stream
    DY = Slab(N, Ho, Wo, Cout, ldy_[1], ldy_[2], values=dy)
    WT = Flat((Cin, k, k, Cout), woff, values=w.permute(3, 1, 2, 0))     # wt[ci,kh,kw,co] = w[co,kh,kw,ci]
    DX = Slab(N, H, W, Cin, ldx_[1], ldx_[2], fill=float("nan"))
    AS = [Slab(N, H, W, Cin, L[1], L[2], values=v) for v, L in adds]
    a_args = []
    for i in range(2):
        a_args += [AS[i].ptr, AS[i].ld] if i < len(AS) else [None, 0]
    _hip.call("snn_conv2d_dgrad", DY.ptr, DY.ld, WT.ptr, None, DX.ptr, DX.ld, N, H, W, Cin, Ho, Wo, Cout, k, k, s, pad,
              *a_args, _prec(_hip, prec), st)
    torch.cuda.synchronize()
    assert DY.guards_intact(whole=True) and WT.guards_intact(whole=True) and all(A.guards_intact(whole=True) for A in AS)
    assert DX.guards_intact(), "snn_conv2d_dgrad wrote outside its output slice"
    return DX.value()


@gpu
@pytest.mark.parametrize("shape", CASES, ids=CASE_IDS)
def test_data_gradient_on_every_layout(H_, shape):
    _hip = H_
    N, H, W, Cin, Cout, k, s = shape
    pad, Ho, Wo, _, w, dy = _case_data(*shape, seed=Cin + 5 * Cout)
    g = torch.Generator().manual_seed(8)
    a1, a2 = torch.randn(N, H, W, Cin, generator=g), torch.randn(N, H, W, Cin, generator=g)
    dyd, wd = dy.double(), w.double()
    ref, mag = _dgrad_ref(dyd, wd, H, W, s, pad), _dgrad_ref(dyd.abs(), wd.abs(), H, W, s, pad)
    Ly, Lx = _layouts(Cout), _layouts(Cin)
    runs = [(f"dy:{L[0]}", L, Lx[0], 0) for L in Ly] + [(f"dx:{L[0]}", Ly[0], L, 0) for L in Lx[1:]]
    runs += [(f"wt+{o}", Ly[0], Lx[0], o) for o in (1, 2, 3)]
    for what, ly, lx, woff in runs:
        out = _run_dgrad(_hip, dy, w, shape, "bf16x3", ly, lx, woff)
        _check(f"dgrad {what}", out, ref, mag, "bf16x3")
        if what == "dy:dense":
            if s > 1:
                wrong = ref.clone()
                wrong[:, 1::s, 1::s] = 0                          # one stride-phase class zeroed
            else:
                dyw = dyd.clone()
                dyw[..., Cout // 2] = 0                           # one output-gradient channel dropped
                wrong = _dgrad_ref(dyw, wd, H, W, s, pad)
            _teeth("dgrad", out, wrong, mag, "bf16x3")
    # one and two fused addends (dx = conv^T(dy) + addend + addend2), each on its own layout, dx at a slice
    for L in Lx:
        out = _run_dgrad(_hip, dy, w, shape, "bf16x3", Ly[1], Lx[3], 0, adds=[(a1, L)])
        _check(f"dgrad addend:{L[0]}", out, ref + a1.double(), mag, "bf16x3", extra_mag=a1.double().abs())
        out = _run_dgrad(_hip, dy, w, shape, "bf16x3", Ly[0], Lx[1], 0, adds=[(a1, Lx[2]), (a2, L)])
        _check(f"dgrad addend2:{L[0]}", out, ref + a1.double() + a2.double(), mag, "bf16x3",
               extra_mag=a1.double().abs() + a2.double().abs())


@gpu
@pytest.mark.parametrize("prec", ["bf16x1", "fp32"])
@pytest.mark.parametrize("shape", [CASES[1], CASES[4], CASES[7]], ids=[CASE_IDS[1], CASE_IDS[4], CASE_IDS[7]])
def test_data_gradient_arithmetic_modes_on_slices(H_, shape, prec):
    _hip = H_
    N, H, W, Cin, Cout, k, s = shape
    pad, Ho, Wo, _, w, dy = _case_data(*shape, seed=12)
    dyd, wd = dy.double(), w.double()
    ref, mag = _dgrad_ref(dyd, wd, H, W, s, pad), _dgrad_ref(dyd.abs(), wd.abs(), H, W, s, pad)
    Ly, Lx = _layouts(Cout), _layouts(Cin)
    for ly, lx, woff in ((Ly[0], Lx[0], 0), (Ly[1], Lx[2], 0), (Ly[3], Lx[5], 3), (Ly[5], Lx[1], 1)):
        out = _run_dgrad(_hip, dy, w, shape, prec, ly, lx, woff)
        _check(f"dgrad {prec} dy:{ly[0]} dx:{lx[0]} wt+{woff}", out, ref, mag, prec)


@gpu
def test_stride2_3x3_data_gradient_on_slices(H_):
    """snn_conv3x3_s2_dgrad (one pass over dy for the four stride-phase classes) where its query accepts the shape:
    dy and dx slices, both addends on their own layouts.  A dy the kernel cannot stage (not 16-byte aligned, or
    lddy % 4 != 0) is refused on the host - functional then takes snn_conv2d_dgrad (_halo_operand_ok)."""
    from snn_for_object_detection_amd import functional as HF
    _hip = H_
    N, H, W, Cin, Cout = 2, 13, 17, 64, 32
    assert _hip.query("snn_conv3x3_s2_dgrad_supported", N, H, W, Cin, 7, 9, Cout) == 1
    shape = (N, H, W, Cin, Cout, 3, 2)
    pad, Ho, Wo, _, w, dy = _case_data(*shape, seed=21)
    g = torch.Generator().manual_seed(9)
    a1, a2 = torch.randn(N, H, W, Cin, generator=g).double(), torch.randn(N, H, W, Cin, generator=g).double()
    dyd, wd = dy.double(), w.double()
    ref, mag = _dgrad_ref(dyd, wd, H, W, 2, 1), _dgrad_ref(dyd.abs(), wd.abs(), H, W, 2, 1)
    st = torch.cuda.current_stream().cuda_stream
    wt = w.permute(3, 1, 2, 0).contiguous().cuda()                # [Cin][3][3][Cout]
    img = torch.empty(9 * Cin * Cout, device="cuda")
    table = torch.tensor([[0, 0, Cin, Cout]], dtype=torch.int64, device="cuda")
    _hip.call("snn_weight_frag_image_batched", wt.data_ptr(), img.data_ptr(), table.data_ptr(), 1,
              9 * (Cout // 32) * (Cin // 32) * 128, 1, _hip.PREC_BF16X3, st)
    Ly, Lx = _layouts(Cout), _layouts(Cin)
    runs = [(L, Lx[0], None, None) for L in Ly] + [(Ly[0], L, None, None) for L in Lx[1:]]
    runs += [(Ly[1], Lx[2], L, Lx[3]) for L in Lx]
    for ly, lx, la1, la2 in runs:
        DY = Slab(N, Ho, Wo, Cout, ly[1], ly[2], values=dy)
        DX = Slab(N, H, W, Cin, lx[1], lx[2], fill=float("nan"))
        A1 = Slab(N, H, W, Cin, la1[1], la1[2], values=a1.float()) if la1 else None
        A2 = Slab(N, H, W, Cin, la2[1], la2[2], values=a2.float()) if la2 else None
        if not HF._halo_operand_ok(DY.ptr, DY.ld, False):
            with pytest.raises(RuntimeError, match="must be aligned|bad pixel strides"):
                _hip.call("snn_conv3x3_s2_dgrad", DY.ptr, DY.ld, img.data_ptr(), DX.ptr, DX.ld, N, H, W, Cin, Ho, Wo, Cout,
                          None, 0, None, 0, _hip.PREC_BF16X3, st)
            assert DX.guards_intact() and bool(DX.view.isnan().all())            # nothing launched
            continue
        _hip.call("snn_conv3x3_s2_dgrad", DY.ptr, DY.ld, img.data_ptr(), DX.ptr, DX.ld, N, H, W, Cin, Ho, Wo, Cout,
                  A1.ptr if A1 else None, A1.ld if A1 else 0, A2.ptr if A2 else None, A2.ld if A2 else 0,
                  _hip.PREC_BF16X3, st)
        torch.cuda.synchronize()
        what = f"s2 dgrad dy:{ly[0]} dx:{lx[0]} addends:{la1[0] if la1 else '-'}"
        assert DY.guards_intact(whole=True) and DX.guards_intact(), what
        assert A1 is None or (A1.guards_intact(whole=True) and A2.guards_intact(whole=True)), what
        out = DX.value()
        if A1 is None:
            _check(what, out, ref, mag, "bf16x3")
            if ly[0] == "dense" and lx[0] == "dense":
                wrong = ref.clone()
                wrong[:, 0::2, 1::2] = 0                              # one stride-phase class zeroed
                _teeth("s2 dgrad", out, wrong, mag, "bf16x3")
        else:
            _check(what, out, ref + a1 + a2, mag, "bf16x3", extra_mag=a1.abs() + a2.abs())


# ---------------------------------------------------------------------------------------------------- weight gradient
def _run_wgrad(_hip, x, dy, shape, prec, lx, ly, dwoff=0, old=None):
    N, H, W, Cin, Cout, k, s = shape
    pad, Ho, Wo = _geom(H, W, k, s)
    st = torch.cuda.current_stream().cuda_stream
    X = Slab(N, H, W, Cin, lx[1], lx[2], values=x)
    DY = Slab(N, Ho, Wo, Cout, ly[1], ly[2], values=dy)
    DW = Flat((Cout, k, k, Cin), dwoff, values=old, fill=None if old is not None else float("nan"))
    splitk = _hip.query("snn_conv2d_wgrad_splitk", N, H, W, Cin, Ho, Wo, Cout, k, k, s, pad, _prec(_hip, prec))
    ws = torch.empty(splitk, Cout * k * k * Cin, device="cuda")
    _hip.call("snn_conv2d_wgrad", X.ptr, X.ld, DY.ptr, DY.ld, DW.ptr, N, H, W, Cin, Ho, Wo, Cout, k, k, s, pad,
              int(old is not None), ws.data_ptr(), splitk, _prec(_hip, prec), st)
    torch.cuda.synchronize()
    assert X.guards_intact(whole=True) and DY.guards_intact(whole=True)
    assert DW.guards_intact(), "snn_conv2d_wgrad wrote outside its weight gradient"
    return DW.value()


def _wgrad_layout_runs(Cin, Cout):
    Lx, Ly = _layouts(Cin), _layouts(Cout)
    runs = [(f"x:{L[0]}", L, Ly[0], 0) for L in Lx] + [(f"dy:{L[0]}", Lx[0], L, 0) for L in Ly[1:]]
    runs += [(f"dw+{o}", Lx[0], Ly[0], o) for o in (1, 3)]
    return runs


@gpu
@pytest.mark.parametrize("shape", CASES, ids=CASE_IDS)
def test_weight_gradient_on_every_layout(H_, shape):
    _hip = H_
    N, H, W, Cin, Cout, k, s = shape
    pad, Ho, Wo, x, _, dy = _case_data(*shape, seed=3 * Cin + Cout)
    xd, dyd = x.double(), dy.double()
    ref, mag = _wgrad_ref(xd, dyd, k, k, s, pad), _wgrad_ref(xd.abs(), dyd.abs(), k, k, s, pad)
    for what, lx, ly, dwoff in _wgrad_layout_runs(Cin, Cout):
        out = _run_wgrad(_hip, x, dy, shape, "bf16x3", lx, ly, dwoff)
        _check(f"wgrad {what}", out, ref, mag, "bf16x3")
        if what == "x:dense":
            shifted = torch.roll(xd, 1, dims=2)                   # the padding shifted by one column
            shifted[:, :, 0] = 0
            _teeth("wgrad", out, _wgrad_ref(shifted, dyd, k, k, s, pad), mag, "bf16x3")
    # accumulate = 1 onto known non-zero values: old + ref
    old = torch.randn(Cout, k, k, Cin, generator=torch.Generator().manual_seed(5))
    for what, lx, ly, dwoff in [("dense", _layouts(Cin)[0], _layouts(Cout)[0], 0),
                                ("x:off1,dy:ld_odd,dw+2", _layouts(Cin)[2], _layouts(Cout)[5], 2),
                                ("x:merge,dy:off2,dw+1", _layouts(Cin)[1], _layouts(Cout)[3], 1)]:
        out = _run_wgrad(_hip, x, dy, shape, "bf16x3", lx, ly, dwoff, old=old)
        _check(f"wgrad accumulate {what}", out, old.double() + ref, mag, "bf16x3", extra_mag=old.double().abs())


@gpu
@pytest.mark.parametrize("prec", ["bf16x1", "fp32"])
@pytest.mark.parametrize("shape", [CASES[0], CASES[1], CASES[4]], ids=[CASE_IDS[0], CASE_IDS[1], CASE_IDS[4]])
def test_weight_gradient_arithmetic_modes_on_slices(H_, shape, prec):
    _hip = H_
    N, H, W, Cin, Cout, k, s = shape
    pad, Ho, Wo, x, _, dy = _case_data(*shape, seed=13)
    xd, dyd = x.double(), dy.double()
    ref, mag = _wgrad_ref(xd, dyd, k, k, s, pad), _wgrad_ref(xd.abs(), dyd.abs(), k, k, s, pad)
    Lx, Ly = _layouts(Cin), _layouts(Cout)
    for lx, ly, dwoff in ((Lx[0], Ly[0], 0), (Lx[1], Ly[1], 0), (Lx[3], Ly[5], 3), (Lx[2], Ly[3], 1)):
        out = _run_wgrad(_hip, x, dy, shape, prec, lx, ly, dwoff)
        _check(f"wgrad {prec} x:{lx[0]} dy:{ly[0]} dw+{dwoff}", out, ref, mag, prec)


# 3x3 stride 1, Cin = Cout = 32 and 150 000 output pixels: the halo-resident weight gradient's size threshold
HALO_WGRAD_SHAPE = (2, 250, 301, 32, 32, 3, 1)


@gpu
def test_halo_resident_weight_gradient_and_its_drop_to_the_implicit_gemm(H_):
    """Aligned potentials take k_conv_wgrad_halo; x at an offset that is not 16-byte aligned or with ld % 4 != 0 makes
    it return rc < 0 and the implicit GEMM (non-pipelined: vec fails) runs instead; a misaligned dy stays in the halo
    kernel.  Every one against fp64 per element."""
    _hip = H_
    shape = HALO_WGRAD_SHAPE
    N, H, W, Cin, Cout, k, s = shape
    pad, Ho, Wo = _geom(H, W, k, s)
    assert _hip.query("snn_conv2d_wgrad_kernel", N, H, W, Cin, Ho, Wo, Cout, k, k, s, pad, _hip.PREC_BF16X3) == 1
    g = torch.Generator().manual_seed(17)
    x, dy = torch.randn(N, H, W, Cin, generator=g), torch.randn(N, Ho, Wo, Cout, generator=g)
    xd, dyd = x.double(), dy.double()
    ref, mag = _wgrad_ref(xd, dyd, k, k, s, pad), _wgrad_ref(xd.abs(), dyd.abs(), k, k, s, pad)
    Lx, Ly = _layouts(Cin), _layouts(Cout)
    for lx, ly, dwoff in ((Lx[0], Ly[0], 0), (Lx[1], Ly[1], 0), (Lx[2], Ly[0], 0), (Lx[5], Ly[0], 0),
                          (Lx[0], Ly[3], 1)):
        out = _run_wgrad(_hip, x, dy, shape, "bf16x3", lx, ly, dwoff)
        _check(f"halo wgrad x:{lx[0]} dy:{ly[0]} dw+{dwoff}", out, ref, mag, "bf16x3")
        if lx[0] == "dense" and ly[0] == "dense":
            xw = xd.clone()
            xw[..., 5] = 0                                         # one input channel dropped
            _teeth("halo wgrad", out, _wgrad_ref(xw, dyd, k, k, s, pad), mag, "bf16x3")


# ---------------------------------------------------------------------------------------------------- spike operands
SPIKE_CASES = [
    # N, H, W, Cin, Cout, k, s
    (2, 9, 13, 64, 64, 3, 1),     # snn_conv3x3_halo_spikes forward (halo-resident), pipelined weight gradient
    (1, 11, 9, 64, 32, 3, 2),     # snn_conv2d_spikes_fwd: k_conv_gather XSP, stride 2
    (2, 7, 10, 32, 36, 1, 1),     # 1x1: snn_conv1x1_spikes_fwd / _wgrad
    (1, 13, 11, 32, 64, 5, 2),    # 5x5 stride 2
    (2, 9, 13, 64, 16, 3, 1),     # 3x3 stride 1 without a halo plan (16 channels): k_conv_gather XSP, two k-steps per tap
]
SPIKE_IDS = ["halo3x3", "gather-s2", "1x1", "5x5-s2", "gather-3x3-c16"]
V_TH = 1.0


def _potentials(N, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    v = 1.0 + 0.8 * torch.randn(N, H, W, C, generator=g)
    v.view(-1)[:4] = torch.tensor([1.0, 1.0 + 2 ** -23, 1.0 - 2 ** -24, 0.0])   # exactly at / next to the threshold
    return v


def _spikes_supported(_hip, shape, ld):
    N, H, W, Cin, Cout, k, s = shape
    pad, Ho, Wo = _geom(H, W, k, s)
    if k == 1:
        return bool(_hip.query("snn_conv1x1_spikes_supported", N, H, W, Cin, Cout, ld, _hip.PREC_FP16X3, _hip.PREC_BF16X3))
    return bool(_hip.query("snn_conv2d_spikes_supported", N, H, W, Cin, Ho, Wo, Cout, k, k, s, pad, ld, _hip.PREC_FP16X3,
                           _hip.PREC_BF16X3))


@gpu
@pytest.mark.parametrize("shape", SPIKE_CASES, ids=SPIKE_IDS)
def test_spike_operand_convolutions_on_every_layout(H_, shape):
    """Where the query accepts a layout and functional's routing (_spikes_fwd_ok / _spikes_wgrad_ok) sends a layer to the
    thresholding kernels, their result is bit for bit the plain kernel's on the stored spikes (and within the fp64 bound);
    where the routing refuses it, the kernel itself refuses it on the host, before any launch."""
    from snn_for_object_detection_amd import functional as HF
    _hip = H_
    N, H, W, Cin, Cout, k, s = shape
    pad, Ho, Wo = _geom(H, W, k, s)
    st = torch.cuda.current_stream().cuda_stream
    v = _potentials(N, H, W, Cin, seed=Cin + Cout + k)
    z = (v > V_TH).float()
    g = torch.Generator().manual_seed(4)
    w = torch.randn(Cout, k, k, Cin, generator=g) / (Cin * k * k) ** 0.5
    dy = torch.randn(N, Ho, Wo, Cout, generator=g)
    zd, wd, dyd = z.double(), w.double(), dy.double()
    y_ref, y_mag = _fwd_ref(zd, wd, s, pad), _fwd_ref(zd, wd.abs(), s, pad)
    g_ref, g_mag = _wgrad_ref(zd, dyd, k, k, s, pad), _wgrad_ref(zd, dyd.abs(), k, k, s, pad)
    halo = HF._halo_ok(N, H, W, Cin, Cout, k, k, s, pad)
    img = None
    if halo:
        img = torch.empty(9 * Cout * Cin, device="cuda")
        wdev = w.contiguous().cuda()
        table = torch.tensor([[0, 0, Cout, Cin]], dtype=torch.int64, device="cuda")
        _hip.call("snn_weight_frag_image_batched", wdev.data_ptr(), img.data_ptr(), table.data_ptr(), 1,
                  9 * (Cin // 32) * (Cout // 32) * 128, 0, _hip.PREC_FP16X3, st)
    Lx, Ly = _layouts(Cin), _layouts(Cout)
    runs = [(L, Ly[0], 0) for L in Lx] + [(Lx[0], L, 0) for L in Ly[1:]] + [(Lx[0], Ly[0], o) for o in (1, 2, 3)]
    taken = refused = 0
    y_dense = None
    for lx, ly, woff in runs:
        what = f"x:{lx[0]} y/dy:{ly[0]} w+{woff}"
        V = Slab(N, H, W, Cin, lx[1], lx[2], values=v)
        Z = Slab(N, H, W, Cin, lx[1], lx[2], values=z)
        Wt = Flat(w.shape, woff, values=w)
        supported = _spikes_supported(_hip, shape, V.ld)
        # ---- forward
        fwd_ok = HF._spikes_fwd_ok(supported, halo, V.ptr, Wt.ptr)
        Y1 = Slab(N, Ho, Wo, Cout, ly[1], ly[2], fill=float("nan"))
        Y0 = Slab(N, Ho, Wo, Cout, ly[1], ly[2], fill=float("nan"))
        if fwd_ok:
            taken += 1
            if halo:
                _hip.call("snn_conv3x3_halo_spikes", V.ptr, V.ld, V_TH, img.data_ptr(), Y1.ptr, Y1.ld, N, H, W, Cin, Cout,
                          None, 0, None, st)
                _hip.call("snn_conv3x3_halo", Z.ptr, Z.ld, img.data_ptr(), Y0.ptr, Y0.ld, N, H, W, Cin, Cout, None, 0, None,
                          0, None, 0, None, _hip.PREC_FP16X3, st)
            else:
                if k == 1:
                    _hip.call("snn_conv1x1_spikes_fwd", V.ptr, V.ld, V_TH, Wt.ptr, Y1.ptr, Y1.ld, N, H, W, Cin, Cout, st)
                else:
                    _hip.call("snn_conv2d_spikes_fwd", V.ptr, V.ld, V_TH, Wt.ptr, Y1.ptr, Y1.ld, N, H, W, Cin, Ho, Wo, Cout,
                              k, k, s, pad, None, 0, None, st)
                _hip.call("snn_conv2d_fwd", Z.ptr, Z.ld, Wt.ptr, None, Y0.ptr, Y0.ld, N, H, W, Cin, Ho, Wo, Cout, k, k, s,
                          pad, None, 0, None, 0, None, _hip.PREC_FP16X3, st)
            torch.cuda.synchronize()
            assert V.guards_intact(whole=True) and Wt.guards_intact(whole=True) and Y1.guards_intact(), what
            y1 = Y1.value()
            assert torch.equal(y1, Y0.value()), f"spike forward {what}: not the plain kernel's bits"
            if (lx[0], ly[0], woff) == ("dense", "dense", 0):
                y_dense = y1
            _check(f"spike forward {what}", y1, y_ref, y_mag, "fp16x3")
        elif supported and not halo:
            refused += 1
            with pytest.raises(RuntimeError, match="16-byte aligned"):
                _hip.call("snn_conv2d_spikes_fwd", V.ptr, V.ld, V_TH, Wt.ptr, Y1.ptr, Y1.ld, N, H, W, Cin, Ho, Wo, Cout,
                          k, k, s, pad, None, 0, None, st)
        # ---- weight gradient (dy on the layout of y), accumulating onto 0.25
        DY = Slab(N, Ho, Wo, Cout, ly[1], ly[2], values=dy)
        wg_ok = supported and HF._spikes_wgrad_ok(V.ptr, V.ld, DY.ptr, DY.ld)
        splitk = _hip.query("snn_conv2d_wgrad_splitk", N, H, W, Cin, Ho, Wo, Cout, k, k, s, pad, _hip.PREC_BF16X3)
        ws = torch.empty(splitk, Cout * k * k * Cin, device="cuda")
        G1 = Flat(w.shape, woff, fill=0.25)
        G0 = Flat(w.shape, woff, fill=0.25)
        if wg_ok:
            taken += 1
            if k == 1:
                _hip.call("snn_conv1x1_spikes_wgrad", V.ptr, V.ld, V_TH, DY.ptr, DY.ld, G1.ptr, N, H, W, Cin, Cout, 1,
                          ws.data_ptr(), splitk, st)
            else:
                _hip.call("snn_conv2d_spikes_wgrad", V.ptr, V.ld, V_TH, DY.ptr, DY.ld, G1.ptr, N, H, W, Cin, Ho, Wo, Cout,
                          k, k, s, pad, 1, ws.data_ptr(), splitk, st)
            _hip.call("snn_conv2d_wgrad", Z.ptr, Z.ld, DY.ptr, DY.ld, G0.ptr, N, H, W, Cin, Ho, Wo, Cout, k, k, s, pad, 1,
                      ws.data_ptr(), splitk, _hip.PREC_BF16X3, st)
            torch.cuda.synchronize()
            assert V.guards_intact(whole=True) and DY.guards_intact(whole=True) and G1.guards_intact(), what
            g1 = G1.value()
            assert torch.equal(g1, G0.value()), f"spike weight gradient {what}: not the plain kernel's bits"
            _check(f"spike weight gradient {what}", g1, g_ref + 0.25, g_mag, "bf16x3", extra_mag=torch.full_like(g_mag, 0.25))
        elif supported:
            refused += 1
            with pytest.raises(RuntimeError, match="16-byte aligned"):
                _hip.call("snn_conv2d_spikes_wgrad", V.ptr, V.ld, V_TH, DY.ptr, DY.ld, G1.ptr, N, H, W, Cin, Ho, Wo, Cout,
                          k, k, s, pad, 1, ws.data_ptr(), splitk, st)
    assert taken >= 10 and refused >= 3, (taken, refused)
    zw = zd.clone()
    zw[..., Cin // 2] = 0                                              # one input channel of spikes dropped
    _teeth("spike forward", y_dense, _fwd_ref(zw, wd, s, pad), y_mag, "fp16x3")


def test_spike_routing_table_sends_uncovered_layouts_to_the_plain_path(hip_lib):
    """Host side, no device: for each layout the model can produce, functional's choice between the thresholding kernels
    and the stored-spike path.  The shape queries see shapes and strides only; the kernels also need 16-byte aligned
    potentials, weight (implicit GEMM; the halo-resident forward reads its own image) and output gradient, and strides
    that are multiples of 4 - a layout the query accepts but the kernels cannot run must go to the plain path."""
    from snn_for_object_detection_amd import _hip
    from snn_for_object_detection_amd import functional as HF
    B = 0x7f0000000000                          # a 256-byte aligned base address; offsets in floats
    # N, H, W, Cin, Cout, k, s, ld(x), x float offset, w float offset, ldg, gy float offset, -> forward thresholds?,
    # backward thresholds? (only behind a forward that kept the potentials: otherwise it has the stored spikes)
    table = [
        ((8, 16, 20, 64, 32, 3, 2), 64, 0, 0, 32, 0, True, True),       # dense: both thresholding kernels
        ((8, 16, 20, 64, 32, 3, 2), 64, 0, 1, 32, 0, False, False),     # weight at a flat offset = 1 (mod 4)
        ((8, 16, 20, 64, 32, 3, 2), 64, 0, 2, 32, 0, False, False),     # ... = 2 (mod 4): 8-byte aligned only
        ((8, 16, 20, 64, 32, 3, 2), 64, 0, 3, 32, 0, False, False),
        ((8, 16, 20, 64, 32, 3, 2), 64, 0, 0, 34, 2, True, False),      # gy: Dense concat slice behind a 2-channel branch
        ((8, 16, 20, 64, 32, 3, 2), 64, 0, 0, 36, 4, True, True),       # ... behind a 4-channel branch: aligned
        ((8, 16, 20, 64, 32, 3, 2), 64, 0, 0, 40, 1, True, False),      # gy at an odd offset, ld % 4 == 0
        ((8, 16, 20, 64, 32, 3, 2), 64, 0, 0, 33, 0, True, False),      # ld(gy) % 4 != 0
        ((8, 16, 20, 64, 32, 3, 2), 64, 1, 0, 32, 0, False, False),     # potentials not 16-byte aligned
        ((8, 16, 20, 64, 32, 3, 2), 66, 0, 0, 32, 0, False, False),     # ld(x) % 4 != 0: the query refuses
        ((8, 16, 20, 48, 32, 3, 2), 48, 0, 0, 32, 0, False, False),     # Cin % 32 != 0: the query refuses
        ((8, 16, 20, 64, 64, 3, 1), 64, 0, 1, 64, 0, True, True),       # halo-resident forward: its own weight image
        ((8, 16, 20, 64, 64, 3, 1), 64, 0, 0, 66, 2, True, False),      # ... and a misaligned gradient slice
        ((8, 16, 20, 64, 36, 1, 1), 64, 0, 3, 36, 0, False, False),     # 1x1 (sibling): weight at offset 3
        ((8, 16, 20, 64, 36, 1, 1), 64, 0, 0, 38, 2, True, False),      # 1x1 (sibling): gradient slice at offset 2
    ]
    for shape, ldx, xo, wo, ldg, go, want_fwd, want_wgrad in table:
        N, H, W, Cin, Cout, k, s = shape
        pad, Ho, Wo = _geom(H, W, k, s)
        if k == 1:
            sup = _hip.query("snn_conv1x1_spikes_supported", N, H, W, Cin, Cout, ldx, _hip.PREC_FP16X3, _hip.PREC_BF16X3)
            halo = False                         # _SiblingConv1x1: the implicit GEMM only
        else:
            sup = _hip.query("snn_conv2d_spikes_supported", N, H, W, Cin, Ho, Wo, Cout, k, k, s, pad, ldx,
                             _hip.PREC_FP16X3, _hip.PREC_BF16X3)
            halo = HF._halo_ok(N, H, W, Cin, Cout, k, k, s, pad) and ldx % 4 == 0
        got_fwd = HF._spikes_fwd_ok(sup, halo, B + 4 * xo, B + 4 * wo)
        got_wgrad = got_fwd and HF._spikes_wgrad_ok(B + 4 * xo, ldx, B + 4 * go, ldg)
        assert got_fwd == want_fwd, (shape, ldx, xo, wo, "forward")
        assert got_wgrad == want_wgrad, (shape, ldx, xo, ldg, go, "weight gradient")
    # the operand the halo-resident kernels stage (x of the forward, dy of the stride-1 / stride-2 data gradients):
    # (float offset, pixel stride, bf16 storage) -> halo kernel?  Otherwise the implicit GEMM, which takes any layout.
    for off, ld, bf16, want in [(0, 64, False, True), (4, 72, False, True), (2, 36, False, False), (1, 68, False, False),
                                (0, 66, False, False), (4, 36, True, True), (2, 36, True, False), (0, 34, True, False)]:
        assert HF._halo_operand_ok(B + (2 if bf16 else 4) * off, ld, bf16) == want, (off, ld, bf16)


# ---------------------------------------------------------------------------------------------------- model level
def _spy(_hip, calls):
    class Spy:
        def before(self, name, args):
            calls.append((name, args))

        def after(self, tok):
            pass
    _hip.PROFILER = Spy()


@gpu
@pytest.mark.parametrize("net", ["pass2-conv3x3", "conv-s2-between"])
def test_spike_branch_writing_into_a_misaligned_concat_slice_trains(H_, net):
    """pass2-conv3x3: Dense([[Pass()], [Conv(32, 3), Norm(), LIF(), Conv(8, 3)]]) - the 2-channel event input passes
    through, so the spike-operand convolution writes channels 2..10 of the concat and its backward gets that misaligned
    slice of the concat gradient (ldg = 10).  conv-s2-between: the same behind a 2-channel stride-2 branch with a 32-channel
    3x3 stride-2 convolution (ldg = 36, a multiple of 4, but 8-byte aligned only), whose data gradient the stride-2
    halo kernel would take for an aligned dy.  One training step against the CPU oracle, and bit for bit the step with
    the spike path off (functional.USE_SPIKES_FROM_VDEC)."""
    _hip = H_
    import snn_for_object_detection_amd as S
    from oracle.net import BlockRef
    HF = S.functional
    T, B, H, W = 2, 2, 12, 14
    s2 = net == "conv-s2-between"
    Ct, Ho, Wo = (36, H // 2, W // 2) if s2 else (10, H, W)

    def cfg():
        if s2:
            return [S.Dense([[S.Conv(2, 3, 2)], [S.Conv(64, 3), S.Norm(), S.LIF(), S.Conv(32, 3, 2)], [S.Conv(2, 3, 2)]])]
        return [S.Dense([[S.Pass()], [S.Conv(32, 3), S.Norm(), S.LIF(), S.Conv(8, 3)]])]

    torch.manual_seed(6)
    blk = S.BlockGen(2, cfg())
    ref = BlockRef(2, cfg())
    ref.load_state_dict(blk.state_dict())
    blk = blk.cuda().train()
    X = synthetic_events(T, B, H, W, p=0.3, seed=5)
    probe = torch.randn(T, B, Ct, Ho, Wo, generator=torch.Generator().manual_seed(2))

    def run(on):
        calls = []
        _spy(_hip, calls)
        try:
            with HF.levers(USE_SPIKES_FROM_VDEC=on):
                blk.zero_grad(set_to_none=True)
                y, _ = blk(X.cuda())
                (y * probe.cuda()).sum().backward()
                torch.cuda.synchronize()
                HF.wgrad_stream_sync()
                torch.cuda.synchronize()
                return y.detach().cpu(), {n: p.grad.detach().cpu().clone() for n, p in blk.named_parameters()}, calls
        finally:
            _hip.PROFILER = None

    y1, g1, calls1 = run(True)
    fwd = [a for nm, a in calls1 if nm == "snn_conv2d_spikes_fwd"]
    assert len(fwd) == 1, [nm for nm, _ in calls1]
    ldy, y_ptr = fwd[0][5], fwd[0][4]
    assert ldy == Ct and (y_ptr - 8) % 16 == 0                          # the case stays misaligned: channel offset 2
    Cin = 64 if s2 else 32
    wg = [a for nm, a in calls1 if nm == "snn_conv2d_wgrad" and a[1] == Cin and a[3] == Ct]
    assert len(wg) == 1 and "snn_conv2d_spikes_wgrad" not in [nm for nm, _ in calls1]   # the stored-spike fallback
    if s2:   # the data gradient of that convolution reads the same slice: the implicit GEMM, not the halo kernel
        dg = [a for nm, a in calls1 if nm == "snn_conv2d_dgrad" and a[1] == Ct and a[9] == Cin]
        assert len(dg) == 1 and "snn_conv3x3_s2_dgrad" not in [nm for nm, _ in calls1]
    y0, g0, calls0 = run(False)
    assert not any("spikes" in nm for nm, _ in calls0)
    assert float(y0.abs().sum()) > 0 and torch.equal(y1, y0)
    for n in g0:
        assert torch.equal(g1[n], g0[n]), n
    # against the oracle (time loop, fp32 CPU autograd)
    state, outs = None, []
    for t in range(T):
        o, state = ref(X[t], state)
        outs.append(o)
    yr = torch.stack(outs)
    (yr * probe).sum().backward()
    assert rel_err(y1, yr) < 1e-4
    for n, p in ref.named_parameters():
        if p.grad is not None:
            assert rel_err(g1[n], p.grad) < 1e-3, n


@gpu
def test_spike_convolution_with_a_misaligned_flat_weight_trains(H_):
    """Conv(3, 3) -> LIF -> Conv(32, 3) -> Norm -> LIF -> Conv(8, 3): the 54-float first weight puts the spike-operand
    convolution's weight at a flat-buffer offset = 2 (mod 4) under FlatTrainer.  Two optimiser steps against
    torch.optim.Adamax on the same net (whose weights are separate, aligned tensors)."""
    _hip = H_
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd.trainer import FlatTrainer
    HF = S.functional
    T, B, H, W = 3, 2, 16, 20

    def cfg():
        return [S.Conv(3, 3), S.LIF(), S.Conv(32, 3), S.Norm(), S.LIF(), S.Conv(8, 3)]

    torch.manual_seed(8)
    a = S.BlockGen(2, cfg()).cuda().train()
    b = S.BlockGen(2, cfg()).cuda().train()
    b.load_state_dict(a.state_dict())
    tr = FlatTrainer(a, lr=1e-3)
    opt = torch.optim.Adamax([p for p in b.parameters() if p.requires_grad], lr=1e-3)
    spike_w = [p for p in a.parameters() if p.dim() == 4 and p.shape[:2] == (8, 32)]
    assert len(spike_w) == 1 and tr._offset_of[id(spike_w[0])] % 4 != 0
    assert spike_w[0].data_ptr() % 16 != 0
    X = synthetic_events(T, B, H, W, p=0.3, seed=7).cuda()
    probe = torch.randn(T, B, 8, H, W, generator=torch.Generator().manual_seed(3)).cuda()
    for it in range(2):
        calls = []
        _spy(_hip, calls)
        try:
            tr.zero_grad()
            la = (a(X)[0] * probe).sum()
            la.backward()
            torch.cuda.synchronize()
        finally:
            _hip.PROFILER = None
        # the LIF in front wrote no spike tensor (the pair is on the spike route), the convolution wrote them after all
        no_out = [a_ for nm, a_ in calls if nm == "snn_affine_neuron_fwd" and a_[7] is None]
        assert len(no_out) == 1 and no_out[0][18] & _hip.SCAN_SPIKES_FROM_VDEC
        assert not any("spikes" in nm for nm, _ in calls), [nm for nm, _ in calls]
        opt.zero_grad()
        lb = (b(X)[0] * probe).sum()
        lb.backward()
        assert abs(la.item() - lb.item()) <= 1e-4 * abs(lb.item()) + 1e-4
        by_name = tr.grads_by_name(a)
        for name, p in b.named_parameters():
            if p.requires_grad:
                assert rel_err(by_name[name], p.grad) < 1e-4, (it, name)
        tr.step()
        opt.step()
        for (n, pa), pb in zip(a.named_parameters(), b.parameters()):
            if pa.requires_grad:
                assert rel_err(pa, pb) < 1e-5, (it, n)
    assert HF.USE_SPIKES_FROM_VDEC
