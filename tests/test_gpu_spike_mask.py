"""The spike bit mask of the stage-entry LIF layers (``SNN_SCAN_SPIKE_MASK``, ``snn_affine_neuron_fwd_mask``) and the 1x1
convolutions that read it (``snn_conv1x1_mask_fwd`` / ``_wgrad`` / ``_supported``).

The mask is the comparison the potentials-fed kernels perform on load, stored as one bit: every check here is for EQUAL
BITS - the mask against ``vdec > v_th`` of the potentials the same call wrote, ``y`` and ``dw`` against the potentials-fed
calls (``snn_conv1x1_spikes_fwd`` / ``_wgrad``), a tiny model's loss and gradients with and without the mask."""
import pytest
import torch

from tests.util import synthetic_events

pytestmark = pytest.mark.gpu

V_TH = 1.0


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


# ------------------------------------------------------------------------------------------------------------ scan
def _scan_params(S):
    """c_mem = 1/2, c_syn = -1/2, v_leak = v_reset = 0, v_th = 1: from the initial state step 0 gives v_dec = x / 2
    exactly, so y in {2, 2 +- 1 ulp} (alpha = 1, beta = 0: x = y exactly) lands on the threshold and one ulp either side."""
    p = S.functional.neuron_params(v_th=V_TH)
    p.c_mem, p.c_syn, p.v_leak, p.v_reset = 0.5, -0.5, 0.0, 0.0
    return p


@pytest.mark.parametrize("C", [32, 64, 96, 160])
@pytest.mark.parametrize("M", [1, 37, 257])
@pytest.mark.parametrize("T", [1, 3])
def test_scan_mask_is_the_threshold_comparison_of_the_stored_potentials(S, T, M, C):
    from snn_for_object_detection_amd import _hip
    p = _scan_params(S)
    g = _gen(1000 * T + 10 * M + C)
    two = torch.tensor(2.0)
    crafted = torch.stack([two, torch.nextafter(two, torch.tensor(3.0)), torch.nextafter(two, torch.tensor(1.0))])
    # multiples of 1/4 in [-1, 4): v_dec of step 0 is exact, potentials near and across the threshold in every step
    y = (torch.randint(-4, 16, (T, M, C), generator=g).float() / 4.0)
    pick = torch.randint(0, 4, (M, C), generator=g)
    y[0] = torch.where(pick < 3, crafted[pick.clamp(max=2)], y[0])
    y = y.cuda()
    alpha = torch.ones(T, C, device="cuda")
    beta = torch.zeros(T, C, device="cuda")
    ldm = C // 32 + 1
    SENT = 0x5A5A5A5A

    def run(with_mask):
        vdec = torch.full((T, M, C), float("nan"), device="cuda")
        vT, iT = torch.empty(M, C, device="cuda"), torch.empty(M, C, device="cuda")
        mask = torch.full((T, M, ldm), SENT, device="cuda", dtype=torch.int32)
        head = (_hip.NEURON_LIF, y.data_ptr(), C, alpha.data_ptr(), beta.data_ptr(), None, None, None, C, None, 0,
                vT.data_ptr(), iT.data_ptr(), vdec.data_ptr(), T, M, C, p)
        if with_mask:
            _hip.call("snn_affine_neuron_fwd_mask", *head, _hip.SCAN_SPIKES_FROM_VDEC | _hip.SCAN_SPIKE_MASK, _st(),
                      mask.data_ptr(), ldm)
        else:
            _hip.call("snn_affine_neuron_fwd", *head, _hip.SCAN_SPIKES_FROM_VDEC, _st())
        torch.cuda.synchronize()
        return vdec.cpu(), vT.cpu(), iT.cpu(), mask.cpu()

    vdec1, vT1, iT1, mask = run(True)
    vdec0, vT0, iT0, _ = run(False)
    assert torch.equal(vdec1, vdec0) and torch.equal(vT1, vT0) and torch.equal(iT1, iT0)
    # the crafted potentials were reached without rounding: exactly v_th and one ulp either side
    one = torch.tensor(V_TH)
    for k, want in enumerate((one, torch.nextafter(one, torch.tensor(2.0)), torch.nextafter(one, torch.tensor(0.0)))):
        sel = pick == k
        assert torch.equal(vdec1[0][sel], want.expand(int(sel.sum())))
    if M * C >= 64:
        assert all(int((pick == k).sum()) > 0 for k in range(3))
    z = vdec1 > V_TH                                   # [T, M, C], strict
    bits = (mask[..., : C // 32].unsqueeze(-1) >> torch.arange(32, dtype=torch.int32)) & 1   # [T, M, C/32, 32]
    assert torch.equal(bits.reshape(T, M, C).bool(), z)
    assert torch.equal(mask[..., C // 32], torch.full((T, M), SENT, dtype=torch.int32))      # the sentinel words survive


def test_scan_mask_flag_refusals(S):
    from snn_for_object_detection_amd import _hip
    p = _scan_params(S)
    T, M, C = 1, 8, 32
    y = torch.zeros(T, M, C, device="cuda")
    ab = torch.ones(T, C, device="cuda")
    vdec, st = torch.empty_like(y), torch.empty(M, C, device="cuda")
    mask = torch.zeros(T, M, 1, device="cuda", dtype=torch.int32)
    head = (_hip.NEURON_LIF, y.data_ptr(), C, ab.data_ptr(), ab.data_ptr(), None, None, None, C, None, 0, st.data_ptr(),
            st.data_ptr(), vdec.data_ptr(), T, M, C, p)
    both = _hip.SCAN_SPIKES_FROM_VDEC | _hip.SCAN_SPIKE_MASK
    with pytest.raises(RuntimeError):   # the flag without SNN_SCAN_SPIKES_FROM_VDEC
        _hip.call("snn_affine_neuron_fwd_mask", *head, _hip.SCAN_SPIKE_MASK, _st(), mask.data_ptr(), 1)
    with pytest.raises(RuntimeError):   # the flag without a buffer, and through the entry point that has none
        _hip.call("snn_affine_neuron_fwd_mask", *head, both, _st(), None, 1)
    with pytest.raises(RuntimeError):
        _hip.call("snn_affine_neuron_fwd", *head, both, _st())
    with pytest.raises(RuntimeError):   # ld_mask < C / 32
        _hip.call("snn_affine_neuron_fwd_mask", *head, both, _st(), mask.data_ptr(), 0)
    head48 = head[:16] + (48, p)
    with pytest.raises(RuntimeError):   # C % 32
        _hip.call("snn_affine_neuron_fwd_mask", *head48, both, _st(), mask.data_ptr(), 2)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- convolutions
def _pack(z):
    """[pixels, C] bool -> [pixels, C/32] int32, bit c & 31 of word c >> 5."""
    P, C = z.shape
    w = (z.reshape(P, C // 32, 32).to(torch.int64) << torch.arange(32, dtype=torch.int64)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


_POT = {}


def _potentials(N, H, W, Cin):
    """Potentials around the threshold (shared by the cases of a shape, never modified) and their mask, ld_mask = Cin/32 + 1."""
    key = (N, H, W, Cin)
    if key not in _POT:
        P = N * H * W
        v = torch.randn(P, Cin, generator=_gen(7 + Cin + H)) * 0.8 + 0.8
        v[::5, ::3] = V_TH                                        # exactly on the threshold: no spike
        mask = torch.full((P, Cin // 32 + 1), -1, dtype=torch.int32)   # (the spare word is all ones: must not be read)
        mask[:, : Cin // 32] = _pack(v > V_TH)
        _POT[key] = (v.cuda(), mask.cuda())
    return _POT[key]


@pytest.mark.parametrize("Cout", [4, 36, 64, 132])
@pytest.mark.parametrize("Cin", [32, 96, 160])
@pytest.mark.parametrize("H,W", [(5, 7), (9, 13)])
def test_mask_fed_convolutions_equal_the_potentials_fed_ones(S, H, W, Cin, Cout):
    from snn_for_object_detection_amd import _hip
    N = 3
    P = N * H * W
    v, mask = _potentials(N, H, W, Cin)
    ldm = mask.shape[1]
    g = _gen(Cin * 1000 + Cout)
    w = (torch.randn(Cout, Cin, generator=g) * 0.1).cuda()
    ldy = Cout + 12                                    # y / dy: a channel slice of a wider buffer
    ybuf0 = torch.full((P, ldy), 7.0, device="cuda")
    ybuf1 = ybuf0.clone()
    y0, y1 = ybuf0[:, 8:8 + Cout], ybuf1[:, 8:8 + Cout]
    dybuf = torch.randn(P, ldy, generator=g).cuda()
    dy = dybuf[:, 8:8 + Cout]
    dw0 = torch.randn(Cout, Cin, generator=g).cuda()
    dw1 = dw0.clone()
    assert _hip.query("snn_conv1x1_spikes_supported", N, H, W, Cin, Cout, Cin, _hip.PREC_FP16X3, _hip.PREC_BF16X3) == 1
    assert _hip.query("snn_conv1x1_mask_supported", N, H, W, Cin, Cout, mask.data_ptr(), ldm, w.data_ptr(), y1.data_ptr(), ldy,
                      dy.data_ptr(), ldy, dw1.data_ptr(), _hip.PREC_FP16X3, _hip.PREC_BF16X3) == 1
    # forward (fp16 x 3, two products)
    _hip.call("snn_conv1x1_spikes_fwd", v.data_ptr(), Cin, V_TH, w.data_ptr(), y0.data_ptr(), ldy, N, H, W, Cin, Cout, _st())
    _hip.call("snn_conv1x1_mask_fwd", mask.data_ptr(), ldm, w.data_ptr(), y1.data_ptr(), ldy, N, H, W, Cin, Cout, _st())
    torch.cuda.synchronize()
    assert torch.equal(ybuf1, ybuf0)                   # y bit for bit, and nothing outside the slice touched
    assert float(y0.abs().max()) > 0
    # weight gradient (bf16 x 3, two products): overwrite, then accumulate on top
    splitk = _hip.query("snn_conv2d_wgrad_splitk", N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, _hip.PREC_BF16X3)
    ws = torch.empty(splitk * Cout * Cin, device="cuda")
    for accumulate in (0, 1):
        _hip.call("snn_conv1x1_spikes_wgrad", v.data_ptr(), Cin, V_TH, dy.data_ptr(), ldy, dw0.data_ptr(), N, H, W, Cin, Cout,
                  accumulate, ws.data_ptr(), splitk, _st())
        _hip.call("snn_conv1x1_mask_wgrad", mask.data_ptr(), ldm, dy.data_ptr(), ldy, dw1.data_ptr(), N, H, W, Cin, Cout,
                  accumulate, ws.data_ptr(), splitk, _st())
        torch.cuda.synchronize()
        assert torch.equal(dw1, dw0), accumulate
    assert float(dw0.abs().max()) > 0


def test_more_than_one_block_and_split(S):
    """A map of several 128-pixel tiles whose pixel count is no multiple of the tile, on the flagship's widest pair."""
    from snn_for_object_detection_amd import _hip
    N, H, W, Cin, Cout = 3, 30, 38, 256, 256
    v, mask = _potentials(N, H, W, Cin)
    ldm = mask.shape[1]
    g = _gen(5)
    w = (torch.randn(Cout, Cin, generator=g) * 0.1).cuda()
    dy = torch.randn(N * H * W, Cout, generator=g).cuda()
    y0, y1 = torch.empty(N * H * W, Cout, device="cuda"), torch.empty(N * H * W, Cout, device="cuda")
    dw0, dw1 = torch.empty(Cout, Cin, device="cuda"), torch.empty(Cout, Cin, device="cuda")
    splitk = _hip.query("snn_conv2d_wgrad_splitk", N, H, W, Cin, H, W, Cout, 1, 1, 1, 0, _hip.PREC_BF16X3)
    ws = torch.empty(splitk * Cout * Cin, device="cuda")
    _hip.call("snn_conv1x1_spikes_fwd", v.data_ptr(), Cin, V_TH, w.data_ptr(), y0.data_ptr(), Cout, N, H, W, Cin, Cout, _st())
    _hip.call("snn_conv1x1_mask_fwd", mask.data_ptr(), ldm, w.data_ptr(), y1.data_ptr(), Cout, N, H, W, Cin, Cout, _st())
    _hip.call("snn_conv1x1_spikes_wgrad", v.data_ptr(), Cin, V_TH, dy.data_ptr(), Cout, dw0.data_ptr(), N, H, W, Cin, Cout, 0,
              ws.data_ptr(), splitk, _st())
    _hip.call("snn_conv1x1_mask_wgrad", mask.data_ptr(), ldm, dy.data_ptr(), Cout, dw1.data_ptr(), N, H, W, Cin, Cout, 0,
              ws.data_ptr(), splitk, _st())
    torch.cuda.synchronize()
    assert torch.equal(y1, y0) and torch.equal(dw1, dw0)


# -------------------------------------------------------------------------------------------------------- refusals
def test_supported_refuses_what_the_launches_would(S):
    from snn_for_object_detection_amd import _hip
    N, H, W, Cout = 3, 5, 7, 36
    P = N * H * W
    F, B = _hip.PREC_FP16X3, _hip.PREC_BF16X3
    buf = torch.zeros(P * 8 + 8, device="cuda", dtype=torch.int32)
    w = torch.zeros(Cout * 96 + 4, device="cuda")
    y = torch.zeros(P, Cout + 2, device="cuda")
    dy = torch.zeros(P * (Cout + 4) + 4, device="cuda")
    dw = torch.zeros(Cout, 96, device="cuda")
    q = lambda Cin, mp, ldm, wp, yp, ldy, dyp, lddy, dwp, f=F, b=B: _hip.query(   # noqa: E731
        "snn_conv1x1_mask_supported", N, H, W, Cin, Cout, mp, ldm, wp, yp, ldy, dyp, lddy, dwp, f, b)
    m, wp, yp, dyp, dwp = buf.data_ptr(), w.data_ptr(), y.data_ptr(), dy.data_ptr(), dw.data_ptr()
    assert q(64, m, 2, wp, yp, Cout + 2, dyp, Cout + 4, dwp) == 1
    assert q(64, m, 2, wp, yp, Cout + 2, None, 0, None) == 1          # forward only
    assert q(64, m, 2, None, None, 0, dyp, Cout + 4, dwp) == 1        # weight gradient only
    assert q(48, m, 2, wp, yp, Cout + 2, dyp, Cout + 4, dwp) == 0     # Cin = 48
    assert q(64, m + 2, 2, wp, yp, Cout + 2, dyp, Cout + 4, dwp) == 0  # a misaligned mask pointer
    assert q(64, m, 2, wp, yp, Cout + 2, dyp, Cout + 2, dwp) == 0     # lddy not a multiple of 4
    assert q(64, m, 1, wp, yp, Cout + 2, None, 0, None) == 0          # ld_mask < Cin / 32
    assert q(64, m, 2, wp + 4, yp, Cout + 2, None, 0, None) == 0      # weight not 16-byte aligned
    assert q(64, m, 2, None, None, 0, dyp + 4, Cout + 4, dwp) == 0    # dy not 16-byte aligned
    assert q(64, m, 2, wp, yp, Cout - 4, None, 0, None) == 0          # ldy < Cout
    assert q(64, m, 2, wp, yp, Cout + 2, None, 0, None, _hip.PREC_FP32, B) == 0   # the two default arithmetics only
    assert q(64, m, 2, None, None, 0, dyp, Cout + 4, dwp, F, _hip.PREC_FP32) == 0
    # what the query refuses the launches refuse on the host (an error, nothing launched)
    with pytest.raises(RuntimeError):
        _hip.call("snn_conv1x1_mask_fwd", m, 1, wp, yp, Cout + 2, N, H, W, 64, Cout, _st())
    ws = torch.zeros(64 * Cout * 64, device="cuda")
    with pytest.raises(RuntimeError):
        _hip.call("snn_conv1x1_mask_wgrad", m, 2, dyp, Cout + 2, dwp, N, H, W, 64, Cout, 0, ws.data_ptr(), 1, _st())
    torch.cuda.synchronize()


class _Spy:
    def __init__(self):
        self.names = []

    def before(self, name, args):
        self.names.append(name)

    def after(self, tok):
        pass


class _OddStrideGrad(torch.autograd.Function):
    """Identity whose backward hands the gradient on as a channel slice of a buffer two channels wider: a pixel stride that
    is no multiple of 4, as a slice of a concat gradient can have."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        T, B, C, H, W = g.shape
        buf = torch.zeros(T, B, H, W, C + 2, device=g.device, dtype=g.dtype)
        buf[..., :C] = g.permute(0, 1, 3, 4, 2)
        return buf[..., :C].permute(0, 1, 4, 2, 3)


def _sibling(S, x5, mask, w2s, probe, odd_grad=False):
    """sibling_conv1x1 over potentials ``x5`` [T,B,C,H,W] (channels-last) marked with the threshold and, if given, a mask."""
    from snn_for_object_detection_amd import _hip
    HF = S.functional
    x = x5.detach().requires_grad_()
    x._snn_spike_threshold = V_TH
    if mask is not None:
        x._snn_spike_mask = mask
    ws = [w.detach().clone().requires_grad_() for w in w2s]
    spy = _Spy()
    _hip.PROFILER = spy
    try:
        y = HF.sibling_conv1x1(x, None, ws)
        ((_OddStrideGrad.apply(y) if odd_grad else y) * probe).sum().backward()
        torch.cuda.synchronize()
        HF.wgrad_stream_sync()
        torch.cuda.synchronize()
    finally:
        _hip.PROFILER = None
    return y.detach(), [w.grad.detach() for w in ws], spy.names


@pytest.mark.parametrize("Cin,ldm,odd", [(64, 2, False), (64, 1, False), (48, 2, False), (64, 2, True)],
                         ids=["covered", "short-mask", "cin48", "lddy-odd"])
def test_python_path_falls_back_to_the_potentials(S, Cin, ldm, odd):
    """A mask the query refuses (too few words per pixel, Cin = 48) leaves the call on the potentials (or, where those are
    not covered either, on written spikes): same tensors as without any mask; a covered one takes the mask entry points.
    An output gradient whose pixel stride is no multiple of 4 leaves the WEIGHT GRADIENT alone on the old path."""
    T, B, H, W = 2, 2, 5, 7
    g = _gen(11)
    v = (torch.randn(T, B, H, W, Cin, generator=g) * 0.8 + 0.8).cuda()
    x5 = v.permute(0, 1, 4, 2, 3)
    mask = torch.zeros(T, B, H, W, ldm, dtype=torch.int32)
    if Cin % 32 == 0 and ldm >= Cin // 32:
        mask[..., : Cin // 32] = _pack((v.cpu() > V_TH).reshape(-1, Cin)).reshape(T, B, H, W, -1)
    mask = mask.cuda()
    w2s = [(torch.randn(16, Cin, 1, 1, generator=g) * 0.1).cuda(), (torch.randn(20, Cin, 1, 1, generator=g) * 0.1).cuda()]
    probe = torch.randn(T, B, 36, H, W, generator=g).cuda()
    y1, g1, names1 = _sibling(S, x5, mask, w2s, probe, odd)
    y0, g0, names0 = _sibling(S, x5, None, w2s, probe, odd)
    assert torch.equal(y1, y0) and all(torch.equal(a, b) for a, b in zip(g1, g0))
    assert all(float(g.abs().max()) > 0 for g in g1)
    covered = Cin % 32 == 0 and ldm >= Cin // 32
    assert ("snn_conv1x1_mask_fwd" in names1) == covered and ("snn_conv1x1_mask_wgrad" in names1) == (covered and not odd)
    assert not [n for n in names0 if "mask" in n]
    if not covered:
        assert names1 == names0


# ------------------------------------------------------------------------------------------------------ tiny model
def test_tiny_model_is_bit_equal_with_and_without_the_mask(S):
    """One C2f stage behind a Conv(c, 3, 2) -> Norm -> LIF, B = 1, T = 3, 16 x 24 input: loss and every parameter gradient
    with the mask (default) and without (``SNN_NO_SPIKE_MASK=1``: ``functional.USE_SPIKE_MASK`` off).  The size gate is
    opened for the test: the stage's potentials are far below ``SPIKE_MASK_MIN_BYTES``."""
    from snn_for_object_detection_amd import _hip
    HF = S.functional
    c, half = 64, 32
    inner = [S.Residual([[S.Conv(), S.Norm(), S.LIF()], [S.Pass()]])]
    cfg = [S.Conv(c, 3, 2), S.Norm(), S.LIF(), S.Conv(c, 1), S.Dense([[S.Conv(half, 1), S.Dense([inner, [S.Pass()]])],
                                                                        [S.Conv(half, 1)]]), S.Conv(c, 1)]
    torch.manual_seed(3)
    blk = S.BlockGen(2, cfg).cuda().train()
    x = synthetic_events(3, 1, 16, 24, p=0.3, seed=1).cuda()
    probe = torch.randn(3, 1, c, 8, 12, generator=_gen(4)).cuda()

    def run(on):
        spy = _Spy()
        _hip.PROFILER = spy
        try:
            with HF.levers(USE_SPIKE_MASK=on, SPIKE_MASK_MIN_BYTES=0):
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
    assert names1.count("snn_affine_neuron_fwd_mask") == 1
    assert names1.count("snn_conv1x1_mask_fwd") == 1 and names1.count("snn_conv1x1_mask_wgrad") == 1
    assert not [n for n in names0 if "mask" in n]
    assert names0.count("snn_conv1x1_spikes_fwd") == 1 and names0.count("snn_conv1x1_spikes_wgrad") == 1
    assert torch.equal(loss1, loss0)
    assert g1.keys() == g0.keys() and len(g1) > 0
    for k in g0:
        assert torch.equal(g1[k], g0[k]), k
