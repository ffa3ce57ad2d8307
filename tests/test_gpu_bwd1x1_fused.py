"""Both gradients of a stride-1 1x1 convolution from one pass over dy (``snn_conv1x1_bwd`` / ``snn_conv1x1_mask_bwd`` /
``snn_conv1x1_bwd_supported``; k_conv_wgrad_pipe DX).

The fused kernel runs the arithmetic of the two launches it replaces in their order, so the first check is for EQUAL BITS
against ``snn_conv2d_dgrad`` plus ``snn_conv2d_wgrad`` (``snn_conv1x1_mask_wgrad`` for the mask form) given the same
splitk - dx, dw and every byte around the dx channel slice.  The second is the per-element fp64 bound the separate
kernels are held to (tests/test_gpu_gemm_fp64.py), the third that the query answers 0 exactly where the launch refuses,
then the Python path with the lever on and off."""
import pytest
import torch

from tests.test_gpu_gemm_fp64 import _check, _dgrad_ref, _wgrad_ref
from tests.util import synthetic_events

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import snn_for_object_detection_amd as pkg
    return pkg


def _st():
    return torch.cuda.current_stream().cuda_stream


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _pack(z):
    """[pixels, C] bool -> [pixels, C/32] int32, bit c & 31 of word c >> 5."""
    P, C = z.shape
    w = (z.reshape(P, C // 32, 32).to(torch.int64) << torch.arange(32, dtype=torch.int64)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


# id, N, H, W, Cin, Cout, splitk (0: snn_conv2d_wgrad_splitk's)
SHAPES = [
    ("105px-64-64", 3, 5, 7, 64, 64, 0),      # 105 pixels: no multiple of either stage length, a masked tail
    ("198px-128-64", 2, 9, 11, 128, 64, 0),   # two column tiles of the 64 x 64 weight-gradient tile
    ("72px-320-128", 2, 6, 6, 320, 128, 0),   # 2.5 column tiles of the 128 x 128 tile: the last one half masked
    ("64px-96-48", 2, 4, 8, 96, 48, 0),       # channel counts that fill neither a 32-row MFMA tile nor a 128 tile
    ("200px-splitk3", 2, 10, 10, 64, 64, 3),  # splits of 128 and 72 pixels and one that owns none
    ("one-pixel", 1, 1, 1, 64, 64, 0),
]
SENT = 7.0
_DATA = {}


def _data(sid):
    """The operands of a shape, made once and never modified (CPU fp32): dy, x, spikes z and their mask, w, two addends."""
    if sid not in _DATA:
        _, N, H, W, Cin, Cout, _ = next(s for s in SHAPES if s[0] == sid)
        P = N * H * W
        g = _gen(1000 * Cin + 10 * Cout + P)
        d = {"dy": torch.randn(P, Cout, generator=g), "x": torch.randn(P, Cin, generator=g),
             "w": torch.randn(Cout, Cin, generator=g) * Cin ** -0.5,
             "adds": [torch.randn(P, Cin, generator=g), torch.randn(P, Cin, generator=g)]}
        z = torch.rand(P, Cin, generator=g) < 0.3
        d["z"] = z.float()
        if Cin % 32 == 0:
            d["mask"] = torch.full((P, Cin // 32 + 1), 0x5A5A5A5A, dtype=torch.int32)   # a sentinel word behind every row
            d["mask"][:, : Cin // 32] = _pack(z)
        _DATA[sid] = d
    return _DATA[sid]


def _slice_of(values, wide, fill=SENT):
    """``values`` [P, C] on the device as a channel slice of a buffer 12 channels wider (``wide``) or as it is:
    -> (buffer, slice view, pixel stride)."""
    P, C = values.shape
    if not wide:
        buf = values.cuda().contiguous()
        return buf, buf, C
    buf = torch.full((P, C + 12), fill, device="cuda")
    buf[:, 8:8 + C] = values.cuda()
    return buf, buf[:, 8:8 + C], C + 12


def _run_pair(_hip, sid, form, wide, nadd, *, fused_only=False):
    """The fused launch and the two launches it replaces on the same operands, accumulate 0 then 1.
    -> per accumulate flag (dx buffers, dw) of both, and the operands."""
    _, N, H, W, Cin, Cout, splitk = next(s for s in SHAPES if s[0] == sid)
    P = N * H * W
    d = _data(sid)
    prec = _hip.PREC_BF16X3
    if splitk == 0:
        splitk = _hip.query("snn_conv2d_wgrad_splitk", N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, prec)
    _, dy, lddy = _slice_of(d["dy"], wide)
    wt = d["w"].t().contiguous().cuda()                # [Cin][Cout]
    if form == "mask":
        xop, ldx = d["mask"].cuda(), d["mask"].shape[1]
        xop0 = xop.clone()
    else:
        _, xop, ldx = _slice_of(d["x"], wide)
    adds = [_slice_of(a, wide)[1:] for a in d["adds"][:nadd]]
    a_args = []
    for i in range(2):
        a_args += [adds[i][0].data_ptr(), adds[i][1]] if i < nadd else [None, 0]
    nan = torch.full((P, Cin), float("nan"))
    bufs = [_slice_of(nan, wide) for _ in range(2)]    # dx of the fused launch, of snn_conv2d_dgrad
    (dxb1, dx1, lddx), (dxb0, dx0, _) = bufs
    old = torch.randn(Cout, Cin, generator=_gen(5)).cuda()
    dw1, dw0 = old.clone(), old.clone()
    ws = torch.empty(splitk * Cout * Cin, device="cuda")
    out = []
    for accumulate in (0, 1):
        head = (dy.data_ptr(), lddy, wt.data_ptr(), dx1.data_ptr(), lddx, *a_args, dw1.data_ptr(), N, H, W, Cin, Cout, accumulate,
                ws.data_ptr(), splitk, prec, _st())
        _hip.call("snn_conv1x1_mask_bwd" if form == "mask" else "snn_conv1x1_bwd", xop.data_ptr(), ldx, *head)
        if not fused_only:
            _hip.call("snn_conv2d_dgrad", dy.data_ptr(), lddy, wt.data_ptr(), None, dx0.data_ptr(), lddx, N, H, W, Cin, H, W, Cout,
                      1, 1, 1, 0, *a_args, prec, _st())
            if form == "mask":
                _hip.call("snn_conv1x1_mask_wgrad", xop.data_ptr(), ldx, dy.data_ptr(), lddy, dw0.data_ptr(), N, H, W, Cin, Cout,
                          accumulate, ws.data_ptr(), splitk, _st())
            else:
                _hip.call("snn_conv2d_wgrad", xop.data_ptr(), ldx, dy.data_ptr(), lddy, dw0.data_ptr(), N, H, W, Cin, H, W, Cout,
                          1, 1, 1, 0, accumulate, ws.data_ptr(), splitk, prec, _st())
        torch.cuda.synchronize()
        out.append((dxb1.clone(), dxb0.clone(), dw1.clone(), dw0.clone()))
    if form == "mask":
        assert torch.equal(xop, xop0)                  # the mask and the sentinel words behind its rows survive
    return out, dx1, old


def _forms(sid):
    Cin = next(s for s in SHAPES if s[0] == sid)[4]
    return ("x", "mask") if Cin in (64, 128) else ("x",)


CASES = [(s[0], form, wide, nadd) for s in SHAPES for form in _forms(s[0]) for wide in (False, True) for nadd in (0, 1, 2)]


@pytest.mark.parametrize("sid,form,wide,nadd", CASES, ids=[f"{c[0]}-{c[1]}-{'wide' if c[2] else 'dense'}-add{c[3]}" for c in CASES])
def test_fused_launch_equals_the_two_launches_bit_for_bit(S, sid, form, wide, nadd):
    from snn_for_object_detection_amd import _hip
    out, dx1, _ = _run_pair(_hip, sid, form, wide, nadd)
    for accumulate, (dxb1, dxb0, dw1, dw0) in enumerate(out):
        assert torch.equal(dxb1, dxb0), f"dx (and the bytes around its slice), accumulate {accumulate}"
        assert torch.equal(dw1, dw0), f"dw, accumulate {accumulate}"
    assert not bool(torch.isnan(dx1).any()) and float(out[0][2].abs().max()) > 0


def test_dx_written_over_its_second_addend(S):
    """dx may alias addend2 (the concat-gradient slice the total is left in): every lane reads what it overwrites."""
    from snn_for_object_detection_amd import _hip
    sid, N, H, W, Cin, Cout, _ = SHAPES[1]
    d = _data(sid)
    prec = _hip.PREC_BF16X3
    splitk = _hip.query("snn_conv2d_wgrad_splitk", N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, prec)
    dy, x, wt = d["dy"].cuda(), d["x"].cuda(), d["w"].t().contiguous().cuda()
    a1 = d["adds"][0].cuda()
    res = []
    for fused in (True, False):
        _, dx, ld = _slice_of(d["adds"][1], True)
        dw = torch.empty(Cout, Cin, device="cuda")
        ws = torch.empty(splitk * Cout * Cin, device="cuda")
        adds = (a1.data_ptr(), Cin, dx.data_ptr(), ld)
        if fused:
            _hip.call("snn_conv1x1_bwd", x.data_ptr(), Cin, dy.data_ptr(), Cout, wt.data_ptr(), dx.data_ptr(), ld, *adds,
                      dw.data_ptr(), N, H, W, Cin, Cout, 0, ws.data_ptr(), splitk, prec, _st())
        else:
            _hip.call("snn_conv2d_dgrad", dy.data_ptr(), Cout, wt.data_ptr(), None, dx.data_ptr(), ld, N, H, W, Cin, H, W, Cout,
                      1, 1, 1, 0, *adds, prec, _st())
        torch.cuda.synchronize()
        res.append(dx.clone())
    assert torch.equal(res[0], res[1])


def test_slabs_left_for_a_later_reduction(S):
    """dw = NULL leaves the slabs in the workspace; snn_conv2d_wgrad_reduce then gives the dw of the one-call form."""
    from snn_for_object_detection_amd import _hip
    sid, N, H, W, Cin, Cout, _ = SHAPES[0]
    d = _data(sid)
    prec = _hip.PREC_BF16X3
    splitk = _hip.query("snn_conv2d_wgrad_splitk", N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, prec)
    dy, x, wt = d["dy"].cuda(), d["x"].cuda(), d["w"].t().contiguous().cuda()
    dws = []
    for later in (False, True):
        dx, dw = torch.empty(N * H * W, Cin, device="cuda"), torch.full((Cout, Cin), 3.0, device="cuda")
        ws = torch.empty(splitk * Cout * Cin, device="cuda")
        _hip.call("snn_conv1x1_bwd", x.data_ptr(), Cin, dy.data_ptr(), Cout, wt.data_ptr(), dx.data_ptr(), Cin, None, 0, None, 0,
                  None if later else dw.data_ptr(), N, H, W, Cin, Cout, 1, ws.data_ptr(), splitk, prec, _st())
        if later:
            _hip.call("snn_conv2d_wgrad_reduce", ws.data_ptr(), dw.data_ptr(), Cout * Cin, splitk, 1, _st())
        torch.cuda.synchronize()
        dws.append(dw)
    assert torch.equal(dws[0], dws[1])


@pytest.mark.parametrize("sid,form", [(s[0], f) for s in SHAPES for f in _forms(s[0])],
                         ids=[f"{s[0]}-{f}" for s in SHAPES for f in _forms(s[0])])
def test_against_fp64(S, sid, form):
    """Per element against fp64 with the bound of the bf16 x 3 data and weight gradients (wide strides, both addends)."""
    from snn_for_object_detection_amd import _hip
    _, N, H, W, Cin, Cout, _ = next(s for s in SHAPES if s[0] == sid)
    d = _data(sid)
    out, _, old = _run_pair(_hip, sid, form, True, 2, fused_only=True)
    dy = d["dy"].double().reshape(N, H, W, Cout)
    x = (d["z"] if form == "mask" else d["x"]).double().reshape(N, H, W, Cin)
    w = d["w"].double().reshape(Cout, 1, 1, Cin)
    adds = [a.double().reshape(N, H, W, Cin) for a in d["adds"]]
    dx_ref, dx_mag = _dgrad_ref(dy, w, H, W, 1, 0), _dgrad_ref(dy.abs(), w.abs(), H, W, 1, 0)
    dw_ref, dw_mag = _wgrad_ref(x, dy, 1, 1, 1, 0), _wgrad_ref(x.abs(), dy.abs(), 1, 1, 1, 0)
    old64 = old.cpu().double().reshape(Cout, 1, 1, Cin)
    for accumulate, (dxb1, _, dw1, _) in enumerate(out):
        dx = dxb1[:, 8:8 + Cin].cpu().double().reshape(N, H, W, Cin)
        _check(f"{sid} {form} dx", dx, dx_ref + adds[0] + adds[1], dx_mag, "bf16x3", extra_mag=adds[0].abs() + adds[1].abs())
        dw = dw1.cpu().double().reshape(Cout, 1, 1, Cin)
        if accumulate == 0:
            _check(f"{sid} {form} dw", dw, dw_ref, dw_mag, "bf16x3")
        else:   # on top of the first round's result, itself on top of nothing: old was overwritten by round 0
            first = out[0][2].cpu().double().reshape(Cout, 1, 1, Cin)
            _check(f"{sid} {form} dw accumulated", dw, first + dw_ref, dw_mag, "bf16x3", extra_mag=first.abs())
    assert old64.shape == dw_ref.shape


# -------------------------------------------------------------------------------------------------------- refusals
def test_query_and_launch_refuse_the_same_calls(S):
    """Everything the query answers 0 for here the launch refuses on the host: an error code with snn_last_error set,
    before any kernel starts."""
    from snn_for_object_detection_amd import _hip
    N, H, W = 2, 4, 8
    P = N * H * W
    B3 = _hip.PREC_BF16X3
    big = torch.zeros(P * 400 + 64, device="cuda")
    imask = torch.zeros(P * 8 + 8, device="cuda", dtype=torch.int32)
    ws = torch.zeros(8 * 128 * 400, device="cuda")
    base = big.data_ptr()
    x, dy, wt, dx, a1, a2, dw = (base + 4 * P * 64 * i for i in range(7))   # 16-byte aligned, far enough apart for 64 channels

    def both(Cin=64, Cout=64, x=x, ldx=64, mask=False, dy=dy, lddy=64, wt=wt, dx=dx, lddx=64, a1=None, ld1=0, a2=None, ld2=0,
             prec=B3, n=N, h=H, w=W):
        q = _hip.query("snn_conv1x1_bwd_supported", n, h, w, Cin, Cout, x, ldx, int(mask), dy, lddy, wt, dx, lddx, a1, ld1, a2, ld2,
                       dw, 1, prec)
        args = (x, ldx, dy, lddy, wt, dx, lddx, a1, ld1, a2, ld2, dw, n, h, w, Cin, Cout, 0, ws.data_ptr(), 1, prec, _st())
        name = "snn_conv1x1_mask_bwd" if mask else "snn_conv1x1_bwd"
        if q:
            return 1
        with pytest.raises(RuntimeError, match=name):
            _hip.call(name, *args)
        return 0

    m = imask.data_ptr()
    assert both() == 1 and both(a1=a1, ld1=64, a2=a2, ld2=64) == 1
    assert both(x=m, ldx=2, mask=True) == 1
    assert both(Cout=132, lddy=132) == 0                      # more than 128 output channels
    assert both(Cin=256, Cout=48, ldx=256, lddx=256, lddy=48) == 0   # a weight-gradient tile without a fused instance
    assert both(Cin=62, ldx=62, lddx=62) == 0 and both(Cout=62, lddy=62) == 0   # channel counts no multiples of 4
    assert both(Cin=48, x=m, ldx=2, mask=True, lddx=48) == 0    # mask form: Cin % 32
    assert both(x=m, ldx=1, mask=True) == 0                    # ... and fewer words per pixel than Cin / 32
    for key in ("x", "dy", "wt", "dx"):                        # misaligned pointers
        assert both(**{key: locals()[key] + 4}) == 0, key
    assert both(x=m + 2, ldx=2, mask=True) == 0
    assert both(a1=a1 + 4, ld1=64) == 0 and both(a2=a2 + 8, ld2=64) == 0
    assert both(ldx=66) == 0 and both(lddy=66) == 0 and both(lddx=66) == 0 and both(a1=a1, ld1=66) == 0   # strides % 4
    assert both(ldx=60) == 0 and both(lddy=60) == 0 and both(lddx=60) == 0 and both(a2=a2, ld2=60) == 0   # strides < channels
    assert both(n=1, h=4096, w=4096) == 0                      # one image of x alone is beyond the 2 GiB span
    for prec in (_hip.PREC_FP32, _hip.PREC_BF16X1, _hip.PREC_BF16S):   # exact fp32, one product, bf16 storage
        assert both(prec=prec) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- Python path
class _Spy:
    def __init__(self):
        self.names = []

    def before(self, name, args):
        self.names.append(name)

    def after(self, tok):
        pass


class _OffsetGrad(torch.autograd.Function):
    """Identity whose backward hands the gradient on as a channel slice that starts 2 channels into a wider buffer: a
    pointer that is not 16-byte aligned, as a slice of a concat gradient can have."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        T, B, C, H, W = g.shape
        buf = torch.zeros(T, B, H, W, C + 4, device=g.device, dtype=g.dtype)
        buf[..., 2:2 + C] = g.permute(0, 1, 3, 4, 2)
        return buf[..., 2:2 + C].permute(0, 1, 4, 2, 3)


def _conv_step(S, x5, w, probe, offset, on):
    from snn_for_object_detection_amd import _hip
    HF = S.functional
    x = x5.detach().requires_grad_()
    wp = w.detach().clone().requires_grad_()
    spy = _Spy()
    _hip.PROFILER = spy
    try:
        with HF.levers(USE_FUSED_BWD1X1=on, FUSED_BWD1X1_MIN_BYTES=0):
            y = HF.conv2d(x, wp, 1, 0)
            ((_OffsetGrad.apply(y) if offset else y) * probe).sum().backward()
            torch.cuda.synchronize()
            HF.wgrad_stream_sync()
            torch.cuda.synchronize()
    finally:
        _hip.PROFILER = None
    return x.grad.detach(), wp.grad.detach(), spy.names


@pytest.mark.parametrize("offset", [False, True], ids=["aligned", "gy-at-an-offset"])
def test_python_path_falls_back_to_the_two_launches(S, offset):
    """A ``gy`` that is a channel slice at an offset the query refuses trains through the two launches, with the results
    of the lever switched off; an aligned one takes the fused entry point (size gate opened for this small map)."""
    T, B, H, W, Cin, Cout = 2, 2, 5, 7, 64, 64
    g = _gen(11)
    x5 = torch.randn(T, B, H, W, Cin, generator=g).cuda().permute(0, 1, 4, 2, 3)
    w = (torch.randn(Cout, Cin, 1, 1, generator=g) * 0.1).cuda()
    probe = torch.randn(T, B, Cout, H, W, generator=g).cuda()
    dx1, dw1, names1 = _conv_step(S, x5, w, probe, offset, True)
    dx0, dw0, names0 = _conv_step(S, x5, w, probe, offset, False)
    assert torch.equal(dx1, dx0) and torch.equal(dw1, dw0)
    assert float(dx1.abs().max()) > 0 and float(dw1.abs().max()) > 0
    assert "snn_conv1x1_bwd" not in names0 and "snn_conv2d_dgrad" in names0 and "snn_conv2d_wgrad" in names0
    if offset:
        assert names1 == names0
    else:
        assert "snn_conv1x1_bwd" in names1 and "snn_conv2d_wgrad_reduce" in names1
        assert "snn_conv2d_dgrad" not in names1 and "snn_conv2d_wgrad" not in names1


def test_tiny_model_is_bit_equal_with_the_lever_on_and_off(S):
    """One training step of a two-stage TinyYolo-shaped description at 32 x 40, B = 2, T = 3: loss and every parameter
    gradient with the fused backward (default) and without (``SNN_NO_FUSED_BWD1X1=1``: ``USE_FUSED_BWD1X1`` off).  The
    size gates of the fusion and of the spike mask are opened: the maps are far below ``FUSED_BWD1X1_MIN_BYTES``."""
    from snn_for_object_detection_amd import _hip
    HF = S.functional

    def stage(c):
        half = c // 2
        inner = [S.Residual([[S.Conv(), S.Norm(), S.LIF()], [S.Pass()]])]
        return [S.Conv(c, 3, 2), S.Norm(), S.LIF(), S.Conv(c, 1),
                S.Dense([[S.Conv(half, 1), S.Dense([inner, [S.Pass()]])], [S.Conv(half, 1)]]), S.Conv(c, 1), S.Norm(), S.LIF()]

    torch.manual_seed(3)
    blk = S.BlockGen(2, stage(64) + stage(128)).cuda().train()
    x = synthetic_events(3, 2, 32, 40, p=0.3, seed=1).cuda()
    probe = torch.randn(3, 2, 128, 8, 10, generator=_gen(4)).cuda()

    def run(on):
        spy = _Spy()
        _hip.PROFILER = spy
        try:
            with HF.levers(USE_FUSED_BWD1X1=on, FUSED_BWD1X1_MIN_BYTES=0, SPIKE_MASK_MIN_BYTES=0):
                for p in blk.parameters():
                    p.grad = None
                out, _ = blk(x)
                loss = (out * probe).sum()
                loss.backward()
                torch.cuda.synchronize()
                HF.wgrad_stream_sync()
                torch.cuda.synchronize()
        finally:
            _hip.PROFILER = None
        return loss.detach().clone(), {n: p.grad.detach().clone() for n, p in blk.named_parameters()}, spy.names

    loss1, g1, names1 = run(True)
    loss0, g0, names0 = run(False)
    assert not [n for n in names0 if n in ("snn_conv1x1_bwd", "snn_conv1x1_mask_bwd", "snn_conv2d_wgrad_reduce")]
    fused = [n for n in names1 if n in ("snn_conv1x1_bwd", "snn_conv1x1_mask_bwd")]
    assert fused and names1.count("snn_conv2d_wgrad_reduce") == len(fused)
    assert torch.equal(loss1, loss0)
    assert g1.keys() == g0.keys() and len(g1) > 0
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
    assert sum(float(g.abs().max()) > 0 for g in g0.values()) > len(g0) // 2   # (a silent layer deep in the block may have none)
