"""The whole-sequence ConvLSTM scans - snn_convlstm_seq_fwd / snn_convlstm_seq_bwd (csrc/lstm.hip) - through the C ABI,
every element against the fp64 restatements of tests/lstm_kernel_ref.py within their derived bounds; no norm anywhere
below the module-level section at the end, which keeps the criteria of tests/test_gpu_lstm_seq.py.

Every output (hs, cT, save_g, save_c, dgates, dx inside an lddx-wide buffer, dh0, dc0) is a NaN-filled buffer with a NaN
guard behind it; x is read from a channel slice at an odd offset of a wider buffer of a sentinel.  What a call is not
asked for stays NaN.  Each row asserts from its arguments which kernel instance it takes - MT from snn_convlstm_seq_tile,
VEC from ``Cin % 4`` and the weight pointer, LDS above / below 64 KiB from the byte counts recomputed here - and
``test_every_kernel_instance_is_reached`` fails when the table stops covering them.

Forward: teacher-forced.  Step t of the device is compared with ONE fp64 step from the device's own hs[t-1] and
save_c[t-1], so the bound stays a one-step bound; save_g is compared gate by gate, which pins the gate order.
Backward: on saves the test supplies (the device's own, and a crafted set with gates exactly 0 and 1, G = +-1 and
save_c up to +-50), against the linear recurrence in fp64 with its running-error bound.
"""
import pytest
import torch

from tests import lstm_kernel_ref as R
from tests.lstm_seq_ref import conv_lstm_fp64
from tests.test_gpu_targets_fp64 import Guarded
from tests.util import rel_err

pytestmark = pytest.mark.gpu
F32 = torch.float32
NAN_BITS = 0x7FC00000
SENTINEL = 3.0e38
X_OFF, X_PAD = 3, 7                 # x sits at channel 3 of rows 7 floats wider than Cin
CROSS = (20, 48, 17, 3)
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


def _cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _pixels(M):
    return 32 * _cu() + 21 if M is None else M


class Weight:
    """w [4Ch, K] on the device at a 16-byte aligned address, or one float behind one."""

    def __init__(self, w, shifted):
        self.buf = torch.zeros(w.numel() + 4, device="cuda")
        off = 1 if shifted else 0
        self.buf[off:off + w.numel()] = w.reshape(-1).cuda()
        self.ptr = self.buf.data_ptr() + 4 * off
        assert self.buf.data_ptr() % 16 == 0 and (self.ptr % 16 != 0) == shifted


def instance(hip, Cin, Ch, M, w_ptr):
    """(MT, VEC, forward LDS > 64 KiB, backward LDS > 64 KiB) of a launch, from its arguments."""
    P = hip.query("snn_convlstm_seq_tile", Cin, Ch, M)
    assert P in (16, 32)
    return P // 16, Cin % 4 == 0 and w_ptr % 16 == 0, R.fwd_lds_bytes(P, Cin, Ch) > 65536, R.bwd_lds_bytes(P, Ch) > 65536


def run_fwd(hip, x, W, h0, c0, Ch, save=True):
    """x [T, M, Cin] (host) -> hs, cT, save_g, save_c on the host (save_* None when not asked for)."""
    T, M, Cin = x.shape
    ldx = Cin + X_PAD
    xb = torch.full((T * M, ldx), SENTINEL, device="cuda")
    xb[:, X_OFF:X_OFF + Cin] = x.reshape(T * M, Cin).cuda()
    dev = [None if t is None else t.cuda().contiguous() for t in (h0, c0)]
    hs, cT = Guarded(T * M * Ch, F32), Guarded(M * Ch, F32)
    sg, sc = Guarded(T * M * 4 * Ch, F32), Guarded(T * M * Ch, F32)
    hip.call("snn_convlstm_seq_fwd", xb.data_ptr() + 4 * X_OFF, ldx, W.ptr, _ptr(dev[0]), _ptr(dev[1]), hs.ptr, cT.ptr,
             sg.ptr if save else None, sc.ptr if save else None, T, M, Cin, Ch, _st())
    torch.cuda.synchronize()
    for g in (hs, cT, sg, sc):
        assert g.guard_intact()
    if not save:
        assert sg.untouched() and sc.untouched()
    keep = torch.ones(ldx, dtype=torch.bool)
    keep[X_OFF:X_OFF + Cin] = False
    assert bool((xb[:, keep.cuda()] == SENTINEL).all())
    return {"hs": hs.out(T, M, Ch), "cT": cT.out(M, Ch), "save_g": sg.out(T, M, 4 * Ch) if save else None,
            "save_c": sc.out(T, M, Ch) if save else None}


def run_bwd(hip, W, sg, sc, c0, gh, ghT, gcT, Cin, lddx, want_state):
    """-> dgates, dx (None when lddx is None: dx = NULL), dh0, dc0 (None unless want_state) on the host."""
    T, M, C4 = sg.shape
    Ch = C4 // 4
    dev = [None if t is None else t.cuda().contiguous() for t in (sg, sc, c0, gh, ghT, gcT)]
    dg = Guarded(T * M * C4, F32)
    dx = Guarded(T * M * (lddx or Cin), F32)
    dh0, dc0 = Guarded(M * Ch, F32), Guarded(M * Ch, F32)
    hip.call("snn_convlstm_seq_bwd", W.ptr, *[_ptr(t) for t in dev], dg.ptr, dx.ptr if lddx else None, lddx or Cin,
             dh0.ptr if want_state else None, dc0.ptr if want_state else None, T, M, Cin, Ch, _st())
    torch.cuda.synchronize()
    for g in (dg, dx, dh0, dc0):
        assert g.guard_intact()
    out = {"dgates": dg.out(T, M, C4), "dx": None, "dh0": None, "dc0": None}
    if lddx:
        full = dx.out(T, M, lddx)
        assert bool((_bits(full[..., Cin:]) == NAN_BITS).all())         # the columns beside dx keep their fill
        out["dx"] = full[..., :Cin].contiguous()
    else:
        assert dx.untouched()
    if want_state:
        out["dh0"], out["dc0"] = dh0.out(M, Ch), dc0.out(M, Ch)
    else:
        assert dh0.untouched() and dc0.untouched()
    return out


def _check(out, res, names, what):
    for n in names:
        r = R.worst_ratio(out[n], res, n)
        _WORST[n] = max(_WORST.get(n, 0.0), r)
        assert r <= 1.0, (what, n, r)


def check_forward(x, w, h0, c0, f, what):
    """Teacher-forced: step t against scan_step_fwd on the device's own hs[t-1] / save_c[t-1]."""
    Ch = w.shape[0] // 4
    for t in range(x.shape[0]):
        res = R.scan_step_fwd(x[t], f["hs"][t - 1] if t else h0, f["save_c"][t - 1] if t else c0, w)
        got = dict(zip("IFOG", f["save_g"][t].split(Ch, 1)), c=f["save_c"][t], h=f["hs"][t])
        _check(got, res, ("I", "F", "O", "G", "c", "h"), what + (t,))
    assert torch.equal(_bits(f["cT"]), _bits(f["save_c"][-1]))


def check_backward(hip, W, w, saves, c0, grads, Cin, lddx, want_state, what, res=None):
    res = R.scan_bwd(w, *saves, c0, *grads) if res is None else res
    out = run_bwd(hip, W, *saves, c0, *grads, Cin, lddx, want_state)
    names = ["dgates"] + (["dx"] if lddx else []) + (["dh0", "dc0"] if want_state else [])
    _check(out, res, names, what)
    return out, res


def _plan(i):
    """What row i of the table runs besides its shape: (with state, loss of the device-save backward, lddx - Cin or None
    for dx = NULL, dh0 / dc0 wanted)."""
    return i % 2 == 0, R.LOSSES[i % 4], (0, 5, None)[i % 3], i % 4 < 2


@pytest.mark.parametrize("i", range(len(R.SCAN_ROWS)), ids=[r[0] for r in R.SCAN_ROWS])
def test_scan_kernels_per_element(hip, i):
    name, Cin, Ch, M, T, shifted = R.SCAN_ROWS[i]
    big = M is None
    M = _pixels(M)
    with_state, loss, pad, want_state = _plan(i)
    d = R.scan_inputs(Cin, Ch, M, T)
    W = Weight(d["w"], shifted)
    MT, vec, lds_f, lds_b = instance(hip, Cin, Ch, M, W.ptr)
    assert MT == (2 if big else 1) and vec == (Cin % 4 == 0 and not shifted)
    assert (MT, vec, lds_f, lds_b) == expected_instance(R.SCAN_ROWS[i])
    h0, c0 = (d["h0"], d["c0"]) if with_state else (None, None)
    f = run_fwd(hip, d["x"], W, h0, c0, Ch)
    check_forward(d["x"], d["w"], h0, c0, f, (name,))
    quiet = run_fwd(hip, d["x"], W, h0, c0, Ch, save=False)
    assert torch.equal(_bits(quiet["hs"]), _bits(f["hs"])) and torch.equal(_bits(quiet["cT"]), _bits(f["cT"]))
    lddx = None if pad is None else Cin + pad
    check_backward(hip, W, d["w"], (f["save_g"], f["save_c"]), c0, R.loss_set(d, loss), Cin, lddx, want_state and with_state,
                   (name, "device saves", loss))
    loss2 = R.LOSSES[(i + 1) % 4]
    check_backward(hip, W, d["w"], R.crafted_saves(Ch, M, T), c0, R.loss_set(d, loss2), Cin, Cin + 5 if lddx is None else None,
                   with_state, (name, "crafted saves", loss2))
    print(f"{name}: MT {MT} VEC {int(vec)} LDS fwd {R.fwd_lds_bytes(16 * MT, Cin, Ch)} bwd {R.bwd_lds_bytes(16 * MT, Ch)} B; "
          "worst error / bound so far " + ", ".join(f"{n} {r:.3f}" for n, r in sorted(_WORST.items())))


def expected_instance(row):
    """The instance a row of the table is there for (MT 2 exactly for the rows sized by the CU count)."""
    _, Cin, Ch, M, _, shifted = row
    MT = 2 if M is None else 1
    return MT, Cin % 4 == 0 and not shifted, R.fwd_lds_bytes(16 * MT, Cin, Ch) > 65536, R.bwd_lds_bytes(16 * MT, Ch) > 65536


def test_every_kernel_instance_is_reached(hip):
    fwd = {expected_instance(r)[:3] for r in R.SCAN_ROWS}
    bwd = {(expected_instance(r)[0], expected_instance(r)[3]) for r in R.SCAN_ROWS}
    assert fwd == {(mt, vec, lds) for mt in (1, 2) for vec in (False, True) for lds in (False, True)}, sorted(fwd)
    assert bwd == {(mt, lds) for mt in (1, 2) for lds in (False, True)}, sorted(bwd)
    for r in R.SCAN_ROWS:      # the plan agrees with what the table expects of it (each row asserts the rest when it runs)
        assert hip.query("snn_convlstm_seq_tile", r[1], r[2], _pixels(r[3])) == 16 * expected_instance(r)[0], r[0]
    assert {r[2] for r in R.SCAN_ROWS} >= {16, 48, 128, 144, 256} and {r[1] for r in R.SCAN_ROWS} >= {1, 15, 16, 17, 20, 256}
    print("forward instances (MT, VEC, LDS > 64 KiB):", sorted(fwd), "backward (MT, LDS > 64 KiB):", sorted(bwd))


def test_backward_pointer_and_loss_combinations(hip):
    """Every loss set x (no c0 | c0 with dh0 / dc0 | c0 detached: dh0 = dc0 = NULL) x (dx NULL | lddx = Cin | Cin + 5), on
    the device's saves; the crafted saves with the widest dx."""
    Cin, Ch, M, T = CROSS
    d = R.scan_inputs(Cin, Ch, M, T)
    W = Weight(d["w"], False)
    for with_state in (False, True):
        h0, c0 = (d["h0"], d["c0"]) if with_state else (None, None)
        f = run_fwd(hip, d["x"], W, h0, c0, Ch)
        crafted = R.crafted_saves(Ch, M, T)
        for loss in R.LOSSES:
            grads = R.loss_set(d, loss)
            res, first = None, None
            for want_state in ((False, True) if with_state else (False,)):
                for lddx in (None, Cin, Cin + 5):
                    out, res = check_backward(hip, W, d["w"], (f["save_g"], f["save_c"]), c0, grads, Cin, lddx, want_state,
                                              ("cross", loss, with_state, want_state, lddx), res)
                    first = first or out
                    assert torch.equal(_bits(out["dgates"]), _bits(first["dgates"]))   # whatever else is asked for
            check_backward(hip, W, d["w"], crafted, c0, grads, Cin, Cin + 5, with_state, ("cross crafted", loss, with_state))
    print("cross: worst error / bound so far " + ", ".join(f"{n} {r:.3f}" for n, r in sorted(_WORST.items())))


@pytest.mark.parametrize("Cin,Ch,M,T", [CROSS, (17, 16, 33, 3), (3, 144, 17, 2)])
def test_exact_backward_is_bit_equal_to_fp64(hip, Cin, Ch, M, T):
    e = R.exact_backward_inputs(Cin, Ch, M, T)
    W = Weight(e["w"], False)
    ref = R.scan_bwd(e["w"], e["save_g"], e["save_c"], e["c0"], e["gh"], e["ghT"], e["gcT"]).val
    out = run_bwd(hip, W, e["save_g"], e["save_c"], e["c0"], e["gh"], e["ghT"], e["gcT"], Cin, Cin + 5, True)
    for n in ("dgates", "dx", "dh0", "dc0"):
        assert float(ref[n].abs().max()) > 0, n
        assert torch.equal(out[n].double(), ref[n]), n


def test_saturated_gates_stay_finite_and_bounded(hip):
    Cin, Ch, M, T, scale = R.SATURATED
    d = R.scan_inputs(Cin, Ch, M, T, scale)
    W = Weight(d["w"], False)
    f = run_fwd(hip, d["x"], W, d["h0"], d["c0"], Ch)
    pre = R.scan_step_fwd(d["x"][0], d["h0"], d["c0"], d["w"]).val["pre"]
    assert float(pre.max()) > 55 and float(pre.min()) < -55
    for n in ("hs", "cT", "save_g", "save_c"):
        assert bool(torch.isfinite(f[n]).all()), n
    check_forward(d["x"], d["w"], d["h0"], d["c0"], f, ("saturated",))
    out, _ = check_backward(hip, W, d["w"], (f["save_g"], f["save_c"]), d["c0"], R.loss_set(d, "all"), Cin, Cin, True,
                            ("saturated",))
    for n in ("dgates", "dx", "dh0", "dc0"):
        assert bool(torch.isfinite(out[n]).all()), n


# ====================================================================================================== module level
@pytest.mark.parametrize("T", [3, 1])
def test_module_gradient_flags(hip, T):
    """ConvLSTM(20, 16) with each of x / weight / state requiring a gradient or not: gradients are None exactly where the
    fp64 reference's are, the others within the bounds of tests/test_gpu_lstm_seq.py; nothing required = nothing saved."""
    from snn_for_object_detection_amd.layer_gen import ConvLSTM
    from tests.test_gpu_lstm_seq import BOUND
    B, Cin, Ch, H, W = 1, 20, 16, 3, 5
    g = torch.Generator().manual_seed(40 + T)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    x, w = r(T, B, Cin, H, W), r(4 * Ch, Cin + Ch, 1, 1) * (1.5 / (Cin + Ch) ** 0.5)
    state = (0.5 * r(B, Ch, H, W), r(B, Ch, H, W))
    gh, ghT, gcT = r(T, B, Ch, H, W), r(B, Ch, H, W), r(B, Ch, H, W)
    cl = lambda t: t.cuda().permute(*range(t.dim() - 3), -2, -1, -3).contiguous().permute(*range(t.dim() - 3), -1, -3, -2)  # noqa: E731
    for flags in range(8):
        xg, wg, sg = bool(flags & 1), bool(flags & 2), bool(flags & 4)
        ref = conv_lstm_fp64(x, w, state, gh, ghT, gcT, x_grad=xg, weight_grad=wg, state_grad=sg)
        cell = ConvLSTM(Cin, Ch).cuda()
        with torch.no_grad():
            cell.conv.weight.copy_(w.cuda())
        cell.conv.weight.requires_grad_(wg)
        xd = cl(x).requires_grad_(xg)
        st = tuple(cl(s).requires_grad_(sg) for s in state)
        assert cell.takes_scan(xd, st)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        hs, (hT, cT) = cell(xd, st)
        kept = torch.cuda.memory_allocated() - base
        assert hs.requires_grad == (xg or wg or sg)
        if not (xg or wg or sg):
            assert kept <= (T + 2) * B * H * W * Ch * 4 + 3 * 512, kept       # hs, h_T, c_T and the allocator's rounding
            assert hs.grad_fn is None and cT.grad_fn is None
        else:
            ((hs * gh.cuda()).sum() + (hT * ghT.cuda()).sum() + (cT * gcT.cuda()).sum()).backward()
        torch.cuda.synchronize()
        got = {"hs": hs.detach(), "c_T": cT.detach(), "dx": xd.grad, "dw": cell.conv.weight.grad, "dh0": st[0].grad,
               "dc0": st[1].grad}
        for n in ("hs", "c_T", "dx", "dw", "dh0", "dc0"):
            assert (got[n] is None) == (ref[n] is None), (flags, n)
            if ref[n] is not None:
                e = rel_err(got[n], ref[n])
                assert e < BOUND[n], (flags, n, e)
