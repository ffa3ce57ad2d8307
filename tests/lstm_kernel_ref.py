"""Plain fp64 restatements of the four kernels of csrc/lstm.hip (the pointwise cell kernels ``k_lstm_fwd`` / ``k_lstm_bwd``
and the whole-sequence scans ``k_convlstm_seq_fwd`` / ``k_convlstm_seq_bwd``), computed from the fp32 values the kernels are
given, with the error bounds the per-element tests hold the kernels to, and the shapes and inputs those tests share
(tests/test_lstm_kernel_ref_host.py, tests/test_gpu_lstm_cell_fp64.py, tests/test_gpu_lstm_scan_fp64.py).

Every function returns ``Res(val, mag, bound)``: dictionaries of fp64 tensors by output name; ``mag`` is the same expression
evaluated over absolute values (a subtraction adds), ``bound`` the largest ``|kernel - val|`` that fp32 arithmetic allows.

Bounds.  ``U = 2^-24`` is one fp32 rounding (the build has ``-ffp-contract=off``: every ``*``, ``+``, ``-`` rounds once).

* A K-term MFMA product: ``K * 2^-23 * mag`` (two roundings per term, any summation order).
* ``sigmoidf_`` (``1 / (1 + expf(-x))``, ``expf(x)`` below -88) and ``tanhf`` of an fp32 argument: ``A_SIG`` / ``A_TANH`` fp32
  ulps of ``max(|result|, 2^-126)``.  Both are MEASURED on the MI355X through the cell kernel over the value grid of
  ``cell_values`` (tests/test_gpu_lstm_cell_fp64.py prints them and fails when twice the measurement exceeds the constant),
  doubled and rounded up to a whole ulp.
* Forward, to first order in the errors: an argument error ``e`` passes a sigmoid as ``e / 4`` and a tanh as ``e``
  (sigmoid' <= 1/4, tanh' <= 1); a product ``a b`` carries ``|a| e_b + |b| e_a``; every fp32 operation adds ``U |result|``
  (+ ``2^-149`` where the result may be subnormal).  ``c = F c_prev + I G`` is 3 operations, ``h = O tanhf(c)`` is 1 on top
  of the tanh: see ``_update``.
* Backward: the recurrence is LINEAR in the incoming gradients with coefficients taken from the saves, so its bound is
  the running-error bound ``depth * U * mag`` (+ the absolute term of ``_L`` for results below 2^-126): ``depth`` counts
  the roundings along the longest path to the element (``_L`` counts them as the expression is evaluated: a product adds the depths of its factors + 1, a sum takes the deeper
  operand + 1, a K-term MFMA product adds 2 K, ``tanhf`` of a given value is ``2 * A_TANH``).  With ``a = 2 * A_TANH`` and
  ``d_dh`` / ``d_dc`` the depths of the carried gradients entering a step:
  ``dh = gh + carry`` is ``d_dh + 1``; ``1 - tc tc`` is ``2 a + 2``; ``dc = carry + (dh O)(1 - tc tc)`` is
  ``max(d_dc, d_dh + 2 a + 5) + 1``; ``dI``, ``dF``, ``dG`` are ``dc + 4`` and ``dO`` is ``dh + a + 4`` (each the product of a
  two-factor term and a term of two operations); the carried ``dc F`` is ``dc + 1``; ``d[x ; h] = dgates . w`` adds
  ``2 * 4Ch``.  A step therefore adds ``8 Ch + 2 a + 10`` to the depth of ``dh`` (asserted by the host test): the count grows
  linearly with the steps behind an element.  The cell backward is the same expression for one step, on gates that
  went through the device's sigmoidf_ / tanhf: gate depths ``2 * A_SIG`` and ``a``.
"""
import math
from collections import namedtuple

import torch

U = 2.0 ** -24
TINY = 2.0 ** -149
# fp32 ulps: twice the maxima measured on the MI355X, rounded up (sigmoidf_ 1.985 at x = -0.0391, tanhf 1.139 at x = 0.6756;
# DESIGN, "Whole-sequence ConvLSTM scan")
A_SIG = 4
A_TANH = 3

Res = namedtuple("Res", "val mag bound depth", defaults=(None,))
F64 = torch.float64


def ulp32(v):
    """One fp32 ulp of max(|v|, 2^-126), as fp64."""
    return torch.exp2(torch.floor(torch.log2(v.abs().clamp_min(2.0 ** -126))) - 23)


def _d(t):
    return None if t is None else t.detach().to("cpu", F64)


# ====================================================================================================== forward
def _gates(pre, b_pre, swap_fo=False):
    """Pre-activations [.., 4C] (order input, forget, output, candidate) and their error bound -> values and bounds."""
    C = pre.shape[-1] // 4
    gi, gf, go, gg = pre.split(C, -1)
    bi, bf, bo, bg = b_pre.split(C, -1)
    if swap_fo:
        gf, go, bf, bo = go, gf, bo, bf
    v = {"I": torch.sigmoid(gi), "F": torch.sigmoid(gf), "O": torch.sigmoid(go), "G": torch.tanh(gg)}
    b = {n: e / 4 + A_SIG * ulp32(v[n]) for n, e in (("I", bi), ("F", bf), ("O", bo))}
    b["G"] = bg + A_TANH * ulp32(v["G"])
    return v, b


def _update(v, b, c_prev, no_tanh=False):
    """``c = F c_prev + I G`` (two products, one sum: 3 roundings, each <= U mag_c) and ``h = O tanhf(c)`` (tanhf of the
    kernel's own c: its error passes with tanh' <= 1, then A_TANH ulps, then 1 rounding) -> adds c, h to v, b; mag."""
    cp = torch.zeros_like(v["I"]) if c_prev is None else c_prev
    c = v["F"] * cp + v["I"] * v["G"]
    mag_c = v["F"] * cp.abs() + v["I"] * v["G"].abs()
    b_c = cp.abs() * b["F"] + v["G"].abs() * b["I"] + v["I"] * b["G"] + 3 * (U * mag_c + TINY)
    tc = c if no_tanh else torch.tanh(c)
    h = v["O"] * tc
    b_h = v["O"] * (b_c + A_TANH * ulp32(tc)) + tc.abs() * b["O"] + U * h.abs() + TINY
    v.update(c=c, h=h)
    b.update(c=b_c, h=b_h)
    mag = {n: v[n].abs() for n in ("I", "F", "O", "G")}
    mag.update(c=mag_c, h=h.abs())
    return mag


def cell_fwd(gates, c_prev, mutate=None):
    """``k_lstm_fwd``: gates [M, 4C] (pre-activations), c_prev [M, C] or None -> c, h (and the gate values)."""
    pre, cp = _d(gates), _d(c_prev)
    v, b = _gates(pre, torch.zeros_like(pre), swap_fo=mutate == "swap_fo")
    mag = _update(v, b, cp, no_tanh=mutate == "no_tanh")
    return Res(v, mag, b)


def x_padding(Cin):
    """Columns the x tile is padded by (K is walked in blocks of 16)."""
    return -Cin % 16


def scan_step_fwd(x_t, h_prev, c_prev, w, mutate=None):
    """ONE step of ``k_convlstm_seq_fwd``: x_t [M, Cin], h_prev / c_prev [M, Ch] or None (zeros), w [4Ch, Cin + Ch] ->
    pre, I, F, O, G, c, h.  ``mutate`` (the host test's proof that the bounds can reject): "drop_k" leaves the last K
    term out, "swap_fo" swaps two gates, "no_tanh" replaces tanh(c) by c, "pad_one" reads the x tile's K padding as 1
    (against the weight columns that follow in the row)."""
    x, w = _d(x_t), _d(w)
    Cin, Ch = x.shape[1], w.shape[0] // 4
    K = Cin + Ch
    h = torch.zeros((x.shape[0], Ch), dtype=F64) if h_prev is None else _d(h_prev)
    xh = torch.cat([x, h], 1)
    wt = w.t().contiguous()
    if mutate == "drop_k":
        xh = xh.clone()
        xh[:, K - 1] = 0.0
    pre = xh @ wt
    if mutate == "pad_one":
        pre = pre + w[:, Cin:min(K, Cin + x_padding(Cin))].sum(1)
    mag_pre = xh.abs() @ wt.abs()
    b_pre = K * 2.0 ** -23 * mag_pre
    v, b = _gates(pre, b_pre, swap_fo=mutate == "swap_fo")
    mag = _update(v, b, _d(c_prev), no_tanh=mutate == "no_tanh")
    v["pre"], mag["pre"], b["pre"] = pre, mag_pre, b_pre
    return Res(v, mag, b)


# ====================================================================================================== backward
class _L:
    """A value of the linear backward recurrence: fp64 value ``v``, magnitude ``m``, the rounding count ``d`` behind it,
    and ``a``, the absolute error that does not scale with the value: a result below 2^-126 is rounded to a multiple of
    2^-149, and a sigmoid down there is A_SIG such steps off, whatever factor it then meets.  bound = d U m + a."""
    __slots__ = ("v", "m", "d", "a")

    def __init__(self, v, m=None, d=0, a=0.0):
        self.v, self.m, self.d, self.a = v, (v.abs() if m is None else m), d, a

    def __mul__(self, o):
        return _L(self.v * o.v, self.m * o.m, self.d + o.d + 1, self.m * o.a + o.m * self.a + TINY)

    def __add__(self, o):
        return _L(self.v + o.v, self.m + o.m, max(self.d, o.d) + 1, self.a + o.a)

    def __sub__(self, o):
        return _L(self.v - o.v, self.m + o.m, max(self.d, o.d) + 1, self.a + o.a)

    def dot(self, wmat, K):
        """[M, K] . [K, N] on the MFMA: two roundings per term."""
        a = self.a @ wmat.abs() if torch.is_tensor(self.a) else self.a * wmat.abs().sum(0)
        return _L(self.v @ wmat, self.m @ wmat.abs(), self.d + 2 * K, a + K * TINY)

    def cols(self, a, b):
        return _L(self.v[:, a:b], self.m[:, a:b], self.d, self.a[:, a:b] if torch.is_tensor(self.a) else self.a)

    def bound(self):
        return self.d * U * self.m + self.a


def _libm(v, ulps):
    """The device's sigmoidf_ / tanhf of a given fp32 value: ``ulps`` ulps of max(|v|, 2^-126)."""
    return _L(v, d=2 * ulps, a=ulps * TINY)


def _cat(parts):
    a = torch.cat([p.a + torch.zeros_like(p.v) for p in parts], 1)
    return _L(torch.cat([p.v for p in parts], 1), torch.cat([p.m for p in parts], 1), max(p.d for p in parts), a)


def _cell_bwd_step(I, F, O, G, tc, cp, dh, dcar, swap_fo=False):
    """The cell backward of ``k_lstm_bwd`` / ``k_convlstm_seq_bwd`` with their parentheses -> (dgates [M, 4C], dc F)."""
    if swap_fo:
        F, O = O, F
    one = _L(torch.ones_like(I.v))
    dc = dcar + (dh * O) * (one - tc * tc)
    dI = (dc * G) * (I * (one - I))
    dF = (dc * cp) * (F * (one - F))
    dO = (dh * tc) * (O * (one - O))
    dG = (dc * I) * (one - G * G)
    return _cat([dI, dF, dO, dG]), dc * F


def _or_zero(t, like):
    return _L(torch.zeros_like(like) if t is None else _d(t))


def cell_bwd(gates, c_prev, c, gh, gc, mutate=None):
    """``k_lstm_bwd``: gates [M, 4C] (pre-activations), c_prev [M, C] or None, c [M, C], gh / gc [M, C] or None ->
    g_gates [M, 4C], g_c_prev [M, C].  The gates go through the device's sigmoidf_ / tanhf: depths 2 A_SIG, 2 A_TANH."""
    pre, c = _d(gates), _d(c)
    C = c.shape[1]
    gi, gf, go, gg = pre.split(C, -1)
    I, F, O = (_libm(torch.sigmoid(g), A_SIG) for g in (gi, gf, go))
    G = _libm(torch.tanh(gg), A_TANH)
    tc = _libm(c if mutate == "no_tanh" else torch.tanh(c), A_TANH)
    dg, dcp = _cell_bwd_step(I, F, O, G, tc, _or_zero(c_prev, c), _or_zero(gh, c), _or_zero(gc, c),
                             swap_fo=mutate == "swap_fo")
    out = {"g_gates": dg, "g_c_prev": dcp}
    return Res({n: o.v for n, o in out.items()}, {n: o.m for n, o in out.items()}, {n: o.bound() for n, o in out.items()})


def scan_bwd(w, save_g, save_c, c0, gh, ghT, gcT, mutate=None):
    """``k_convlstm_seq_bwd`` on GIVEN saves: w [4Ch, K], save_g [T, M, 4Ch] (gate VALUES, order I F O G), save_c
    [T, M, Ch], c0 [M, Ch] or None, gh [T, M, Ch] / ghT / gcT [M, Ch] or None -> dgates [T, M, 4Ch], dx [T, M, Cin], dh0,
    dc0 [M, Ch] (always computed; the kernel writes what it is asked for).  ``mutate``: "drop_k" (one of the 4Ch terms of
    d[x ; h]), "swap_fo", "late_c" (c_prev taken one step late: c_t for c_{t-1}), "no_tanh", "no_dh" (dh of step t + 1 left
    out of step t)."""
    w, sg, sc = _d(w), _d(save_g), _d(save_c)
    T, M, C4 = sg.shape
    Ch, Cin = C4 // 4, w.shape[1] - C4 // 4
    dcar, dhl = _or_zero(gcT, sc[0]), _or_zero(ghT, sc[0])
    dgs, dxs = [None] * T, [None] * T
    wm = w
    if mutate == "drop_k":
        wm = w.clone()
        wm[C4 - 1] = 0.0
    for t in range(T - 1, -1, -1):
        I, F, O, G = (_L(g) for g in sg[t].split(Ch, -1))
        tc = _libm(sc[t] if mutate == "no_tanh" else torch.tanh(sc[t]), A_TANH)
        if mutate == "late_c":
            cp = _L(sc[t])
        else:
            cp = _L(sc[t - 1]) if t > 0 else _or_zero(c0, sc[0])
        dh = _or_zero(None if gh is None else gh[t], sc[0]) + dhl
        dgs[t], dcar = _cell_bwd_step(I, F, O, G, tc, cp, dh, dcar, swap_fo=mutate == "swap_fo")
        dxh = dgs[t].dot(wm, C4)
        dxs[t], dhl = dxh.cols(0, Cin), dxh.cols(Cin, Cin + Ch)
        if mutate == "no_dh":
            dhl = _L(torch.zeros_like(dhl.v), d=dhl.d, a=dhl.a)
    val = {"dgates": torch.stack([g.v for g in dgs]), "dx": torch.stack([g.v for g in dxs]), "dh0": dhl.v, "dc0": dcar.v}
    mag = {"dgates": torch.stack([g.m for g in dgs]), "dx": torch.stack([g.m for g in dxs]), "dh0": dhl.m, "dc0": dcar.m}
    bound = {"dgates": torch.stack([g.bound() for g in dgs]), "dx": torch.stack([g.bound() for g in dxs]),
             "dh0": dhl.bound(), "dc0": dcar.bound()}
    depth = {"dgates": [g.d for g in dgs], "dx": [g.d for g in dxs], "dh0": dhl.d, "dc0": dcar.d}
    return Res(val, mag, bound, depth)


# ====================================================================================================== shared inputs
def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * int(k) for i, k in enumerate(key)) % (2 ** 31))


def grid_values():
    """The pre-activation grid: [-104, 104] in steps of 1/8 with +-0, +-17, +-88 (fp32)."""
    g = torch.arange(-104 * 8, 104 * 8 + 1, dtype=torch.float32) / 8
    extra = torch.tensor([0.0, -0.0, 17.0, -17.0, 88.0, -88.0, 104.0, -104.0])
    return torch.cat([g, extra])


CELL_SHAPES = [(1, 1), (255, 1), (256, 1), (257, 1), (85, 3), (86, 3), (16, 16), (17, 16)]   # (M, C): M C = 1, 255 .. 272
CELL_VALUES = ("grid", "0.1", "1", "10")


def cell_values(M, C, kind):
    """gates [M, 4C], c_prev, c, gh, gc [M, C] (fp32) of the cell tests: pre-activations drawn from the grid (each gate on
    its own, so saturated and unsaturated gates meet) or random at a scale; cell states up to +-50 in one half of the
    elements and of order 1 in the other."""
    g = _gen(M, C, CELL_VALUES.index(kind))
    if kind == "grid":
        grid = grid_values()
        gates = grid[torch.randint(0, grid.numel(), (M, 4 * C), generator=g)]
    else:
        gates = torch.randn((M, 4 * C), generator=g) * float(kind)
    scale = torch.where(torch.rand((M, C), generator=g) < 0.5, torch.tensor(50.0), torch.tensor(1.0))
    out = {"gates": gates}
    for n in ("c_prev", "c"):
        out[n] = (2 * torch.rand((M, C), generator=g) - 1) * scale
    if M * C >= 2:
        out["c_prev"].view(-1)[0], out["c"].view(-1)[1] = 50.0, -50.0
    out["gh"], out["gc"] = torch.randn((M, C), generator=g), torch.randn((M, C), generator=g)
    return out


# (id, Cin, Ch, M (None: 32 * CU + 21), T, weight moved by one float)
def scan_rows():
    rows = []
    shapes, Ms = [(1, 16), (15, 16), (16, 16), (17, 16), (20, 48)], [1, 15, 16, 17, 33]
    for i, (Cin, Ch) in enumerate(shapes):          # K padding on both sides of a 16-block / a straddling output tile
        for j, M in enumerate(Ms):
            rows.append((f"pad-{Cin}-{Ch}-m{M}", Cin, Ch, M, 1 + (i + j) % 3, False))
    rows += [("waves9", 20, 144, 17, 3, False),
             ("largest-block", 256, 256, 17, 2, False),
             ("largest-block-unaligned-w", 256, 256, 17, 1, True),
             ("mt2-registers", 3, 128, None, 3, False),
             ("mt2-vec", 20, 48, None, 1, False),
             ("mt2-lds", 256, 128, None, 2, False),
             ("mt2-lds-unaligned-w", 256, 128, None, 2, True),
             ("unaligned-w", 20, 48, 17, 3, True)]
    return rows


SCAN_ROWS = scan_rows()
SATURATED = (20, 48, 17, 3, 4.5)    # Cin, Ch, M, T, scale of x and of w: pre-activations up to +-60
LOSSES = ("gh", "final", "all", "gcT")


def fwd_lds_bytes(P, Cin, Ch):
    return 4 * 2 * P * (-(-Cin // 16) * 16 + 4 + Ch + 4)


def bwd_lds_bytes(P, Ch):
    return 4 * P * (4 * Ch + 4 + Ch)


def scan_inputs(Cin, Ch, M, T, scale=1.0):
    """x [T, M, Cin], w [4Ch, K], h0, c0 [M, Ch], gh [T, M, Ch], ghT, gcT [M, Ch] (fp32).  ``scale`` multiplies x and w
    (the saturated run)."""
    g = _gen(Cin, Ch, M, T)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    K = Cin + Ch
    return {"x": r(T, M, Cin) * scale, "w": r(4 * Ch, K) * (1.5 / K ** 0.5) * scale, "h0": 0.5 * r(M, Ch), "c0": r(M, Ch),
            "gh": r(T, M, Ch), "ghT": r(M, Ch), "gcT": r(M, Ch)}


def loss_set(d, loss):
    """(gh, ghT, gcT) of one of LOSSES."""
    return {"gh": (d["gh"], None, None), "final": (None, d["ghT"], d["gcT"]), "all": (d["gh"], d["ghT"], d["gcT"]),
            "gcT": (None, None, d["gcT"])}[loss]


def crafted_saves(Ch, M, T, exact=False):
    """Saves no forward would write: gates exactly 0 and exactly 1 among ordinary ones, G = +-1, save_c up to +-50.
    ``exact``: every gate 0 or 1, G in {-1, 0, 1} and save_c in {0, +-0.5, ..} replaced by 0 (tanh(0) = 0 exactly), so that
    with integer gradients and a power-of-two weight every sum of the backward is exact."""
    g = _gen(Ch, M, T, 77)
    sg = torch.rand((T, M, 4 * Ch), generator=g)
    pick = torch.rand((T, M, 4 * Ch), generator=g)
    sg = torch.where(pick < 0.25, torch.zeros(()), torch.where(pick < 0.5, torch.ones(()), sg))
    G = 2 * torch.rand((T, M, Ch), generator=g) - 1
    pg = torch.rand((T, M, Ch), generator=g)
    G = torch.where(pg < 0.25, -torch.ones(()), torch.where(pg < 0.5, torch.ones(()), G))
    sg[..., 3 * Ch:] = G
    sc = (2 * torch.rand((T, M, Ch), generator=g) - 1) * torch.where(torch.rand((T, M, Ch), generator=g) < 0.5,
                                                                     torch.tensor(50.0), torch.tensor(1.0))
    sc.view(-1)[0] = 50.0
    sc.view(-1)[-1] = -50.0
    if exact:
        sg = (sg >= 0.5).float()
        sg[..., 3 * Ch:] = torch.randint(-1, 2, (T, M, Ch), generator=g).float()
        sc = torch.zeros_like(sc)
    return sg, sc


def exact_backward_inputs(Cin, Ch, M, T):
    """Integer gradients, 0 / 1 gates and a weight of +-2^-k: every product and partial sum of the backward is an
    integer multiple of 2^-6 far below 2^24, so fp32 and fp64 agree bit for bit."""
    g = _gen(Cin, Ch, M, T, 5)
    K = Cin + Ch
    sg, sc = crafted_saves(Ch, M, T, exact=True)
    sign = torch.randint(0, 2, (4 * Ch, K), generator=g).float() * 2 - 1
    w = sign * torch.exp2(-torch.randint(0, 3, (4 * Ch, K), generator=g).float())
    ints = lambda *s: torch.randint(-3, 4, s, generator=g).float()  # noqa: E731
    return {"w": w, "save_g": sg, "save_c": sc, "c0": ints(M, Ch), "gh": ints(T, M, Ch), "ghT": ints(M, Ch),
            "gcT": ints(M, Ch)}


# ====================================================================================================== comparison
def worst_ratio(out, res, name):
    """max over elements of |out - val| / bound (0 / 0 counts 0); inf when out is not finite somewhere."""
    out = out.detach().to("cpu", F64)
    if not bool(torch.isfinite(out).all()):
        return math.inf
    err, b = (out - res.val[name]).abs(), res.bound[name]
    r = torch.where(err == 0, torch.zeros_like(err), err / b.clamp_min(1e-300))
    return float(r.max()) if r.numel() else 0.0
