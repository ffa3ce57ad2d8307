"""Host side of the per-element ConvLSTM kernel tests (no device):

* tests/lstm_kernel_ref.py (what tests/test_gpu_lstm_cell_fp64.py and tests/test_gpu_lstm_scan_fp64.py compare the kernels
  with) against torch's fp64 autograd over ``oracle.net.ConvLSTM`` (tests/lstm_seq_ref.py), to 1e-12 of the largest
  reference value, per element;
* its bounds ACCEPT the same formulas evaluated in fp32 by torch on the CPU, at every element of every input set the GPU
  tests use with M <= 33, and REJECT six mutated references on at least one element each;
* the refusals of the four launchers of csrc/lstm.hip through the C ABI: each returns 1 before any HIP call, with a
  message that names the entry point."""
import pytest
import torch

from tests import lstm_kernel_ref as R
from tests.lstm_seq_ref import conv_lstm_fp64

SMALL = [r for r in R.SCAN_ROWS if r[3] is not None and r[3] <= 33]
CROSS = (20, 48, 17, 3)
A = 2 * R.A_TANH


def _close(a, b, what):
    tol = 1e-12 * max(float(b.abs().max()), 1e-300)
    assert float((a - b).abs().max()) <= tol, (what, float((a - b).abs().max()), tol)


# ====================================================================================================== against torch fp64
def _chain64(d, T, with_state):
    """scan_step_fwd chained over t in fp64 -> hs, save_g, save_c (fp64)."""
    h, c = (d["h0"].double(), d["c0"].double()) if with_state else (None, None)
    hs, sg, sc = [], [], []
    for t in range(T):
        v = R.scan_step_fwd(d["x"][t], h, c, d["w"]).val
        h, c = v["h"], v["c"]
        hs.append(h)
        sc.append(c)
        sg.append(torch.cat([v["I"], v["F"], v["O"], v["G"]], 1))
    return torch.stack(hs), torch.stack(sg), torch.stack(sc)


def _img(t):
    """[.., M, C] -> [.., 1, C, 1, M] (one image row of M pixels)."""
    return t.transpose(-1, -2).unsqueeze(-2).unsqueeze(-4)


def _flat(t):
    return t.squeeze(-4).squeeze(-2).transpose(-1, -2)


@pytest.mark.parametrize("row", SMALL, ids=[r[0] for r in SMALL])
def test_restatements_match_torch_fp64_autograd(row):
    name, Cin, Ch, M, T, _ = row
    d = R.scan_inputs(Cin, Ch, M, T)
    for with_state in (False, True):
        for loss in R.LOSSES:
            gh, ghT, gcT = R.loss_set(d, loss)
            ref = conv_lstm_fp64(_img(d["x"]), d["w"][:, :, None, None], (_img(d["h0"]), _img(d["c0"])) if with_state else None,
                                 None if gh is None else _img(gh), None if ghT is None else _img(ghT),
                                 None if gcT is None else _img(gcT))
            hs, sg, sc = _chain64(d, T, with_state)
            _close(hs, _flat(ref["hs"]), "hs")
            _close(sc[-1], _flat(ref["c_T"]), "c_T")
            b = R.scan_bwd(d["w"], sg, sc, d["c0"] if with_state else None, gh, ghT, gcT).val
            _close(b["dx"], _flat(ref["dx"]), "dx")
            if with_state:
                _close(b["dh0"], _flat(ref["dh0"]), "dh0")
                _close(b["dc0"], _flat(ref["dc0"]), "dc0")
            # dgates, through the weight gradient it is formed from: dw = sum_t dgates_t^T [x_t ; h_{t-1}]
            hprev = torch.cat([(d["h0"].double() if with_state else torch.zeros(M, Ch, dtype=torch.float64))[None], hs[:-1]])
            xh = torch.cat([d["x"].double(), hprev], 2)
            dw = torch.einsum("tmo,tmk->ok", b["dgates"], xh)
            _close(dw, ref["dw"][:, :, 0, 0], "dw")


def test_cell_restatements_match_torch_fp64_autograd():
    for M, C in R.CELL_SHAPES:
        for kind in R.CELL_VALUES:
            d = R.cell_values(M, C, kind)
            for use_cp in (False, True):
                gates = d["gates"].double().requires_grad_()
                cp = d["c_prev"].double().requires_grad_()
                gi, gf, go, gg = gates.split(C, 1)
                c = torch.sigmoid(gf) * (cp if use_cp else 0.0) + torch.sigmoid(gi) * torch.tanh(gg)
                h = torch.sigmoid(go) * torch.tanh(c)
                f = R.cell_fwd(d["gates"], d["c_prev"] if use_cp else None)
                _close(f.val["c"], c.detach(), "c")
                _close(f.val["h"], h.detach(), "h")
                (h * d["gh"].double()).sum().add((c * d["gc"].double()).sum()).backward()
                b = R.cell_bwd(d["gates"], d["c_prev"] if use_cp else None, c.detach(), d["gh"], d["gc"])
                _close(b.val["g_gates"], gates.grad, "g_gates")
                if use_cp:
                    _close(b.val["g_c_prev"], cp.grad, "g_c_prev")


def test_backward_depth_is_the_documented_count():
    Cin, Ch, M, T = 3, 16, 2, 3
    d = R.scan_inputs(Cin, Ch, M, T)
    _, sg, sc = _chain64(d, T, True)
    depth = R.scan_bwd(d["w"], sg, sc, d["c0"], d["gh"], d["ghT"], d["gcT"]).depth
    step = 8 * Ch + 2 * A + 10
    assert depth["dh0"] == T * step and depth["dx"] == [(T - t) * step for t in range(T)]
    assert depth["dgates"] == [(T - 1 - t) * step + 2 * A + 10 for t in range(T)]
    assert depth["dc0"] == (T - 1) * step + 2 * A + 7


# ====================================================================================================== fp32 on the CPU
def sig32(x):
    """sigmoidf_ of csrc/snn_common.h in torch fp32."""
    return torch.where(x < -88.0, torch.exp(x), 1.0 / (1.0 + torch.exp(-x)))


def cell_fwd32(gates, c_prev):
    C = gates.shape[1] // 4
    gi, gf, go, gg = gates.split(C, 1)
    I, F, O, G = sig32(gi), sig32(gf), sig32(go), torch.tanh(gg)
    c = F * (torch.zeros_like(I) if c_prev is None else c_prev) + I * G
    return {"I": I, "F": F, "O": O, "G": G, "c": c, "h": O * torch.tanh(c)}


def cell_bwd_step32(I, F, O, G, tc, cp, dh, dcar):
    dc = dcar + dh * O * (1.0 - tc * tc)
    dg = torch.cat([(dc * G) * (I * (1.0 - I)), (dc * cp) * (F * (1.0 - F)), (dh * tc) * (O * (1.0 - O)),
                    (dc * I) * (1.0 - G * G)], 1)
    return dg, dc * F


def cell_bwd32(gates, c_prev, c, gh, gc):
    C = c.shape[1]
    gi, gf, go, gg = gates.split(C, 1)
    z = torch.zeros_like(c)
    dg, dcp = cell_bwd_step32(sig32(gi), sig32(gf), sig32(go), torch.tanh(gg), torch.tanh(c), z if c_prev is None else c_prev,
                              z if gh is None else gh, z if gc is None else gc)
    return {"g_gates": dg, "g_c_prev": dcp}


def scan_fwd32(x, w, h0, c0):
    """The forward scan in torch fp32 -> hs, save_g, save_c."""
    T, M, _ = x.shape
    Ch = w.shape[0] // 4
    h = torch.zeros(M, Ch) if h0 is None else h0
    c = None if c0 is None else c0
    hs, sg, sc = [], [], []
    for t in range(T):
        v = cell_fwd32(torch.cat([x[t], h], 1) @ w.t(), c)
        h, c = v["h"], v["c"]
        hs.append(h)
        sc.append(c)
        sg.append(torch.cat([v["I"], v["F"], v["O"], v["G"]], 1))
    return torch.stack(hs), torch.stack(sg), torch.stack(sc)


def scan_bwd32(w, sg, sc, c0, gh, ghT, gcT):
    T, M, C4 = sg.shape
    Ch = C4 // 4
    Cin = w.shape[1] - Ch
    z = torch.zeros(M, Ch)
    dcar, dhl = z if gcT is None else gcT, z if ghT is None else ghT
    dgs, dxs = [None] * T, [None] * T
    for t in range(T - 1, -1, -1):
        I, F, O, G = sg[t].split(Ch, 1)
        cp = sc[t - 1] if t > 0 else (z if c0 is None else c0)
        dh = (z if gh is None else gh[t]) + dhl
        dgs[t], dcar = cell_bwd_step32(I, F, O, G, torch.tanh(sc[t]), cp, dh, dcar)
        dxh = dgs[t] @ w
        dxs[t], dhl = dxh[:, :Cin], dxh[:, Cin:]
    return {"dgates": torch.stack(dgs), "dx": torch.stack(dxs), "dh0": dhl, "dc0": dcar}


def _accept(out, res, names, what):
    for n in names:
        r = R.worst_ratio(out[n], res, n)
        assert r <= 1.0, (what, n, r)


def check_forward_teacher_forced(x, w, h0, c0, hs, sg, sc, what):
    """Every step of a forward scan (fp32 tensors hs, save_g, save_c) against scan_step_fwd on ITS OWN previous step."""
    Ch = w.shape[0] // 4
    for t in range(x.shape[0]):
        res = R.scan_step_fwd(x[t], hs[t - 1] if t else h0, sc[t - 1] if t else c0, w)
        got = dict(zip("IFOG", sg[t].split(Ch, 1)), c=sc[t], h=hs[t])
        _accept(got, res, ("I", "F", "O", "G", "c", "h"), (what, t))


def test_cell_bounds_accept_fp32():
    for M, C in R.CELL_SHAPES + [(8191, 3)]:        # (the last: enough draws from the grid for subnormal gates to meet large factors)
        for kind in R.CELL_VALUES:
            d = R.cell_values(M, C, kind)
            for cp in (None, d["c_prev"]):
                _accept(cell_fwd32(d["gates"], cp), R.cell_fwd(d["gates"], cp), ("c", "h"), (M, C, kind))
                for gh, gc in ((d["gh"], None), (None, d["gc"]), (d["gh"], d["gc"])):
                    _accept(cell_bwd32(d["gates"], cp, d["c"], gh, gc), R.cell_bwd(d["gates"], cp, d["c"], gh, gc),
                            ("g_gates", "g_c_prev"), (M, C, kind))


def _scan_sets():
    """(what, Cin, Ch, M, T, scale) of every scan input set with M <= 33."""
    sets = [(r[0], r[1], r[2], r[3], r[4], 1.0) for r in SMALL]
    sets.append(("cross",) + CROSS + (1.0,))
    sets.append(("saturated",) + R.SATURATED)
    return sets


@pytest.mark.parametrize("s", _scan_sets(), ids=[s[0] for s in _scan_sets()])
def test_scan_bounds_accept_fp32(s):
    what, Cin, Ch, M, T, scale = s
    d = R.scan_inputs(Cin, Ch, M, T, scale)
    for with_state in (False, True):
        h0, c0 = (d["h0"], d["c0"]) if with_state else (None, None)
        hs, sg, sc = scan_fwd32(d["x"], d["w"], h0, c0)
        assert bool(torch.isfinite(hs).all())
        check_forward_teacher_forced(d["x"], d["w"], h0, c0, hs, sg, sc, what)
        for saves in ((sg, sc), R.crafted_saves(Ch, M, T)):
            for loss in R.LOSSES:
                gh, ghT, gcT = R.loss_set(d, loss)
                _accept(scan_bwd32(d["w"], *saves, c0, gh, ghT, gcT), R.scan_bwd(d["w"], *saves, c0, gh, ghT, gcT),
                        ("dgates", "dx", "dh0", "dc0"), (what, loss))


def test_exact_backward_is_bit_equal_in_fp32():
    Cin, Ch, M, T = CROSS
    e = R.exact_backward_inputs(Cin, Ch, M, T)
    args = (e["w"], e["save_g"], e["save_c"], e["c0"], e["gh"], e["ghT"], e["gcT"])
    got, ref = scan_bwd32(*args), R.scan_bwd(*args).val
    for n in ("dgates", "dx", "dh0", "dc0"):
        assert torch.equal(got[n].double(), ref[n]), n
        assert float(ref[n].abs().max()) > 0, n


# ====================================================================================================== mutations
def _rejected(val, res, name):
    return bool(((val - res.val[name]).abs() > res.bound[name]).any())


@pytest.mark.parametrize("Cin,Ch,M,T", [(1, 16, 17, 3), (15, 16, 17, 3), (17, 16, 17, 3), CROSS])
def test_bounds_reject_mutated_references(Cin, Ch, M, T):
    d = R.scan_inputs(Cin, Ch, M, T)
    hs, sg, sc = scan_fwd32(d["x"], d["w"], d["h0"], d["c0"])
    t = T - 1
    step = (d["x"][t], hs[t - 1], sc[t - 1], d["w"])
    good = R.scan_step_fwd(*step)
    for m, names in (("drop_k", ("I", "F", "O", "G", "c", "h")), ("swap_fo", ("F", "O", "c", "h")), ("no_tanh", ("h",)),
                     ("pad_one", ("I", "F", "O", "G", "c", "h"))):
        bad = R.scan_step_fwd(*step, mutate=m).val
        for n in names:
            assert _rejected(bad[n], good, n), (m, n)
    late = R.scan_step_fwd(d["x"][t], hs[t - 1], sc[t - 2] if t >= 2 else d["c0"], d["w"]).val     # c_prev one step late
    assert _rejected(late["c"], good, "c") and _rejected(late["h"], good, "h")
    # (behind three steps of crafted saves, with |c_prev| up to 50 in every dF, the magnitude of dh0 / dc0 is some 1e4
    # times their value: there the mutations are asked of dgates and dx only)
    for crafted, saves in ((False, (sg, sc)), (True, R.crafted_saves(Ch, M, T))):
        args = (d["w"], *saves, d["c0"], d["gh"], d["ghT"], d["gcT"])
        good_b = R.scan_bwd(*args)
        for m, names in (("drop_k", ("dx",)), ("swap_fo", ("dgates", "dx", "dh0", "dc0")), ("late_c", ("dgates", "dx")),
                         ("no_tanh", ("dgates", "dx", "dh0", "dc0")), ("no_dh", ("dgates", "dx", "dh0", "dc0"))):
            bad = R.scan_bwd(*args, mutate=m).val
            for n in (names[:2] if crafted else names):
                assert _rejected(bad[n], good_b, n), (m, n)


def test_bounds_reject_mutated_cell_references():
    d = R.cell_values(17, 16, "1")
    good = R.cell_fwd(d["gates"], d["c_prev"])
    for m, names in (("swap_fo", ("c", "h")), ("no_tanh", ("h",))):
        bad = R.cell_fwd(d["gates"], d["c_prev"], mutate=m).val
        for n in names:
            assert _rejected(bad[n], good, n), (m, n)
    good_b = R.cell_bwd(d["gates"], d["c_prev"], d["c"], d["gh"], d["gc"])
    for m in ("swap_fo", "no_tanh"):
        bad = R.cell_bwd(d["gates"], d["c_prev"], d["c"], d["gh"], d["gc"], mutate=m).val
        assert _rejected(bad["g_gates"], good_b, "g_gates"), m


# ====================================================================================================== refusals
def _owned(n):
    t = torch.zeros(n, device="cuda" if torch.cuda.is_available() else "cpu")
    return t, t.data_ptr()


def _rc(lib, name, args):
    rc = getattr(lib, name)(*args)
    return rc, lib.snn_last_error().decode()


def test_launchers_refuse_before_any_launch(hip_lib):
    """The buffers hold the largest accepted variant of each call (T = 1, M = 2, Cin = 4, Ch = 16), so a library that
    launched instead of refusing would still stay inside memory the test owns."""
    keep, p = _owned(1 << 16)
    q = [p + 4096 * i for i in range(12)]
    #      x     ldx w     h0    c0    hs    cT    save_g save_c T  M  Cin Ch  stream
    fwd = [q[0], 4, q[1], q[2], q[3], q[4], q[5], q[6], q[7], 1, 2, 4, 16, None]
    #      w     save_g save_c c0   gh    ghT   gcT   dgates dx   lddx dh0   dc0    T  M  Cin Ch  stream
    bwd = [q[1], q[6], q[7], q[3], q[4], q[5], q[2], q[8], q[9], 4, q[10], q[11], 1, 2, 4, 16, None]
    cases = []
    cases += [("snn_convlstm_seq_fwd", fwd, {12: Ch}) for Ch in (12, 272)]
    cases += [("snn_convlstm_seq_fwd", fwd, {11: Cin, 1: 300}) for Cin in (0, 257)]
    cases += [("snn_convlstm_seq_fwd", fwd, {1: 3}), ("snn_convlstm_seq_fwd", fwd, {9: 0}), ("snn_convlstm_seq_fwd", fwd, {10: 0})]
    cases += [("snn_convlstm_seq_fwd", fwd, {i: None}) for i in (0, 2, 5, 6)]
    cases += [("snn_convlstm_seq_fwd", fwd, {7: None}), ("snn_convlstm_seq_fwd", fwd, {8: None})]
    cases += [("snn_convlstm_seq_bwd", bwd, {15: Ch}) for Ch in (12, 272)]
    cases += [("snn_convlstm_seq_bwd", bwd, {14: Cin, 9: 300}) for Cin in (0, 257)]
    cases += [("snn_convlstm_seq_bwd", bwd, {9: 3}), ("snn_convlstm_seq_bwd", bwd, {12: 0}), ("snn_convlstm_seq_bwd", bwd, {13: 0})]
    cases += [("snn_convlstm_seq_bwd", bwd, {i: None}) for i in (0, 1, 2, 7)]
    cell_f = [q[0], q[1], q[2], q[3], 2, 16, None]
    cell_b = [q[0], q[1], q[2], q[3], q[4], q[5], q[6], 2, 16, None]
    cases += [("snn_lstm_cell_fwd", cell_f, {i: v}) for i, v in ((0, None), (2, None), (3, None), (4, 0), (5, 0))]
    cases += [("snn_lstm_cell_bwd", cell_b, {i: v}) for i, v in ((0, None), (2, None), (5, None), (7, 0), (8, 0))]
    assert len(cases) == 34
    for fn, ok, change in cases:
        args = list(ok)
        for i, v in change.items():
            args[i] = v
        rc, msg = _rc(hip_lib, fn, args)
        assert rc == 1, (fn, change, rc, msg)            # 1: refused on the host; 2 would be a failed launch
        assert msg.startswith(fn + ":"), (fn, change, msg)
    # lddx < Cin with dx = NULL passes the argument checks: where there is no device the call gets as far as the launch
    # and fails THERE (2), with a device it runs (0) - either way it is not refused (1)
    args = list(bwd)
    args[8], args[9] = None, 3
    rc, msg = _rc(hip_lib, "snn_convlstm_seq_bwd", args)
    assert rc != 1, (rc, msg)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    del keep
