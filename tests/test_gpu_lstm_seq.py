"""The whole-sequence ConvLSTM scan (csrc/lstm.hip, ``functional.conv_lstm_sequence``) against the fp64 restatement of
the reference cell (tests/lstm_seq_ref.py), and per element against the stepwise path run on the same inputs.

Bounds: the project's ConvLSTM bounds (1e-5 outputs / 1e-4 gradients, norm-wise); per element the scan's error may be at
most 4x the stepwise path's (a different summation order of equally accurate fp32-grade arithmetic), with a floor of
``K * 2^-23 * max|fp64|`` (K = Cin + Ch, the accumulation length) where the stepwise result happens to be exact.
Unsupported shapes are checked through the routing predicate (tests/test_lstm_seq_host.py), never launched.
"""
import pytest
import torch

from tests.lstm_seq_ref import conv_lstm_fp64
from tests.util import rel_err

pytestmark = pytest.mark.gpu

NAMES = ("hs", "c_T", "dx", "dw", "dh0", "dc0")
BOUND = {"hs": 1e-5, "c_T": 1e-5, "dx": 1e-4, "dw": 1e-4, "dh0": 1e-4, "dc0": 1e-4}


@pytest.fixture(scope="module")
def S(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import snn_for_object_detection_amd as pkg
    return pkg


def _tile(Cin, Ch, M):
    from snn_for_object_detection_amd import functional as HF
    return HF.conv_lstm_scan_tile(Cin, Ch, M)


# (id, pixels as (B, H, W) or a function of the tile size, Cin, Ch, T, with state, x is a channel slice, loss)
# The kernels have ONE weight mode: every case streams the weight from L2; "k512" is the largest Cin + Ch (1024 threads,
# the operand tiles beyond 64 KiB of LDS).  "fills_chip" has enough pixels for the 32-pixel tile on a 256-CU device.
CASES = [
    ("below_tile", (1, 3, 5), 3, 16, 1, False, False, "dense"),
    ("tile_plus_1", lambda P: (1, 1, P + 1), 20, 48, 2, True, False, "dense"),
    ("tiles_and_tail", (2, 5, 7), 64, 64, 5, True, False, "final"),
    ("sliced_x", (2, 3, 5), 20, 16, 5, False, True, "dense"),
    ("final_only_no_state", (1, 4, 9), 3, 48, 2, False, False, "final"),
    ("sliced_x_state", (1, 3, 7), 3, 64, 2, True, True, "both"),
    ("k512_streamed", lambda P: (1, 1, P + 1), 256, 256, 2, True, False, "both"),
    ("fills_chip", (1, 97, 85), 20, 48, 2, True, False, "dense"),
]


def _inputs(case):
    name, px, Cin, Ch, T, with_state, sliced, loss = case
    B, H, W = px(_tile(Cin, Ch, 1)) if callable(px) else px
    gen = torch.Generator().manual_seed(len(name) * 131 + Cin * 7 + Ch)
    r = lambda *s: torch.randn(*s, generator=gen)  # noqa: E731
    d = {"x": r(T, B, Cin, H, W), "w": r(4 * Ch, Cin + Ch, 1, 1) * (1.5 / (Cin + Ch) ** 0.5),
         "state": (0.5 * r(B, Ch, H, W), r(B, Ch, H, W)) if with_state else None,
         "gh": r(T, B, Ch, H, W) if loss in ("dense", "both") else None,
         "ghT": r(B, Ch, H, W) if loss in ("final", "both") else None,
         "gcT": r(B, Ch, H, W) if loss in ("final", "both") else None}
    return d, (T, B, Cin, Ch, H, W, sliced)


POISON = 3.0e38


def _run(d, dims, scan: bool):
    """One forward + backward of a fresh ``ConvLSTM`` on the device -> the six compared tensors (+ the x buffer)."""
    from snn_for_object_detection_amd import functional as HF
    from snn_for_object_detection_amd.layer_gen import ConvLSTM
    T, B, Cin, Ch, H, W, sliced = dims
    cell = ConvLSTM(Cin, Ch).cuda()
    with torch.no_grad():
        cell.conv.weight.copy_(d["w"].cuda())
    pad = 7 if sliced else 0
    buf = torch.full((T, B, H, W, Cin + pad), POISON, device="cuda")
    buf[..., 3 * bool(pad):3 * bool(pad) + Cin] = d["x"].cuda().permute(0, 1, 3, 4, 2)
    x = buf[..., 3 * bool(pad):3 * bool(pad) + Cin].permute(0, 1, 4, 2, 3).requires_grad_()
    state = None if d["state"] is None else tuple(s.cuda().requires_grad_() for s in d["state"])
    with HF.levers(USE_LSTM_SCAN=scan):
        assert cell.takes_scan(x, state) == scan
        hs, (hT, cT) = cell(x, state)
        loss = 0.0
        for out, g in ((hs, d["gh"]), (hT, d["ghT"]), (cT, d["gcT"])):
            if g is not None:
                loss = loss + (out * g.cuda()).sum()
        loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(hT, hs[-1])
    res = {"hs": hs.detach(), "c_T": cT.detach(), "dx": x.grad, "dw": cell.conv.weight.grad,
           "dh0": None if state is None else state[0].grad, "dc0": None if state is None else state[1].grad}
    return res, buf


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_scan_matches_fp64_and_stepwise(S, case):
    d, dims = _inputs(case)
    T, B, Cin, Ch, H, W, sliced = dims
    ref = conv_lstm_fp64(d["x"], d["w"], d["state"], d["gh"], d["ghT"], d["gcT"])
    scan, buf = _run(d, dims, True)
    step, _ = _run(d, dims, False)
    again, _ = _run(d, dims, True)
    if sliced:   # the neighbours of the channel slice come back untouched
        assert bool((buf[..., :3] == POISON).all()) and bool((buf[..., 3 + Cin:] == POISON).all())
    K, worst = Cin + Ch, 0.0
    for n in NAMES:
        if ref[n] is None:
            assert scan[n] is None
            continue
        r = ref[n]
        e_scan, e_step = rel_err(scan[n], r), rel_err(step[n], r)
        m_scan = float((scan[n].double().cpu() - r).abs().max())
        m_step = float((step[n].double().cpu() - r).abs().max())
        floor = K * 2.0 ** -23 * float(r.abs().max())
        ratio = m_scan / max(m_step, 1e-300)
        worst = max(worst, m_scan / max(4.0 * m_step, floor))
        print(f"{case[0]:>20} {n:>4}: rel scan {e_scan:.2e} stepwise {e_step:.2e} | max scan {m_scan:.2e} "
              f"stepwise {m_step:.2e} ratio {ratio:.2f} floor {floor:.2e}")
        assert e_scan < BOUND[n], (n, e_scan)
        assert m_scan <= max(4.0 * m_step, floor), (n, m_scan, m_step, floor)
    print(f"{case[0]:>20} worst max-error / bound: {worst:.3f}")
    for n in ("hs", "dx", "dw"):   # fixed reduction order, no atomics: the same inputs give the same bits
        assert torch.equal(scan[n], again[n]), n


def test_no_grad_forward_saves_nothing(S):
    from snn_for_object_detection_amd.layer_gen import ConvLSTM
    T, B, Cin, Ch, H, W = 5, 2, 20, 48, 9, 11
    M = B * H * W
    torch.manual_seed(2)
    cell = ConvLSTM(Cin, Ch).cuda()
    x = torch.randn(T, B, H, W, Cin, device="cuda").permute(0, 1, 4, 2, 3)   # channels-last: no layout copy
    assert cell.takes_scan(x)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        hs0, (hT0, cT0) = cell(x)
    quiet = torch.cuda.memory_allocated() - base
    base = torch.cuda.memory_allocated()
    hs1, (hT1, cT1) = cell(x)
    kept = torch.cuda.memory_allocated() - base
    outputs, saved = (T + 2) * M * Ch * 4, T * M * 5 * Ch * 4
    print(f"no_grad forward keeps {quiet} B (outputs {outputs} B); with grad {kept} B (save buffers {saved} B)")
    assert quiet <= outputs + 3 * 512          # hs, h_T, c_T and the allocator's rounding: no save buffer
    assert kept - quiet >= saved
    assert torch.equal(hs0, hs1.detach()) and torch.equal(cT0, cT1.detach())


def test_model_level_against_reference_and_chained_windows(S):
    from snn_for_object_detection_amd import BlockGen, Conv, LSTM, Norm
    from snn_for_object_detection_amd.layer_gen import ConvLSTM
    from oracle.net import BlockRef
    torch.manual_seed(8)
    T, B, Cin, H, W = 4, 2, 5, 6, 7
    cfg = lambda: [Conv(16, 1), Norm(), LSTM(), LSTM(32)]  # noqa: E731
    blk, ref = BlockGen(Cin, cfg()), BlockRef(Cin, cfg())
    ref.load_state_dict(blk.state_dict())
    blk = blk.cuda()
    cells = [m for m in blk.modules() if isinstance(m, ConvLSTM)]
    assert [c.takes_scan(torch.zeros(T, B, 16, H, W)) for c in cells] == [True, True]
    x = torch.randn(2 * T, B, Cin, H, W)
    outd, std = blk(x[:T].cuda())
    state, outs = None, []
    for t in range(T):
        o, state = ref(x[t], state)
        outs.append(o)
    outr = torch.stack(outs)
    g = torch.randn_like(outr)
    (outr * g).sum().backward()
    (outd * g.cuda()).sum().backward()
    assert outd.shape == (T, B, 32, H, W) and rel_err(outd, outr) < 1e-5
    assert rel_err(std[0][3][1], state[0][3][1]) < 1e-5           # final cell state of the last LSTM
    for pd, pr in zip(blk.parameters(), ref.parameters()):
        assert rel_err(pd.grad, pr.grad) < 1e-4
    # the state carries over consecutive windows: window 2 behind window 1 equals steps T .. 2T-1 of one 2T-step run
    with torch.no_grad():
        _, st1 = blk(x[:T].cuda())
        out2, st2 = blk(x[T:].cuda(), st1)
        whole, stw = blk(x.cuda())
    assert rel_err(out2, whole[T:]) < 1e-5
    assert rel_err(st2[0][3][1], stw[0][3][1]) < 1e-5 and rel_err(st2[0][2][0], stw[0][2][0]) < 1e-5


def test_flat_trainer_writes_the_weight_gradient_through_its_slot(S):
    from snn_for_object_detection_amd import BlockGen, Conv, LSTM, Norm
    from snn_for_object_detection_amd import functional as HF
    from snn_for_object_detection_amd.layer_gen import ConvLSTM
    from snn_for_object_detection_amd.trainer import FlatTrainer
    T, B, Cin, H, W = 4, 2, 5, 6, 7
    x = torch.randn(T, B, Cin, H, W, generator=torch.Generator().manual_seed(5)).cuda()
    g = torch.randn(T, B, 32, H, W, generator=torch.Generator().manual_seed(6)).cuda()

    def grads(scan):
        torch.manual_seed(9)
        blk = BlockGen(Cin, [Conv(16, 1), Norm(), LSTM(), LSTM(32)]).cuda()
        tr = FlatTrainer(blk)
        tr.zero_grad()
        with HF.levers(USE_LSTM_SCAN=scan):
            out, _ = blk(x)
            (out * g).sum().backward()
            tr.synchronize()
        for cell in (m for m in blk.modules() if isinstance(m, ConvLSTM)):
            p = cell.conv.weight
            assert p.grad is None and p._snn_grad_slot.written
        return {n: v.clone() for n, v in tr.grads_by_name(blk).items()}

    g_scan, g_step = grads(True), grads(False)
    assert list(g_scan) == list(g_step)
    for n in g_scan:
        assert g_step[n].abs().max() > 0
        assert rel_err(g_scan[n], g_step[n]) < 1e-4, n
