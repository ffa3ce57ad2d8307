"""The halo-resident 3x3 kernels, one row per plan class, against fp64 per element.

k_conv_halo3 (forward / stride-1 data gradient, csrc/conv_halo.hip), k_conv_s2dgrad3 (stride-2 data gradient, same file)
and k_conv_wgrad_halo (weight gradient, csrc/wgrad_halo.hip) through the C ABI.  Every row
* asserts the plan it runs through the host-only queries (snn_conv3x3_halo_plan, snn_conv3x3_s2_dgrad_plan,
  snn_conv2d_wgrad_halo_plan): strip or 4 x 32 rectangles, channel tile, tile counts, idle XCD-padding blocks, patch
  shape, K-steps and split count (planned for the device's CU count; it is in the row's messages);
* writes into a NaN-filled slice of a wider buffer whose guard channels and guard pixels must come back bit for bit;
* checks every element against torch's fp64 CPU convolution, |out - ref| <= tol * mag + ACC_TOL * mag (tests/conv_ref.py),
  plus the norm-wise bound, and that the bound rejects a slightly wrong reference (_teeth);
* runs again on EXACT operands - x (and dy) small integers or spikes, w = k * 2^-6 with |k| <= 31 - where every product
  and partial sum of fp16 x 3, bf16 x 3 and bf16 x 1 is exact: the outputs and the BatchNorm partials must equal fp64
  bit for bit.  A stale piece or a wrong DMA slot in one tile moves a few elements by ~2^-11: no norm sees that.
NaN locality (one NaN in x or dy poisons exactly its 3x3 neighbourhood in its own image) and the fp16 x 3 range
contract are checked on the halo kernels themselves.  Each row prints its largest error / bound ratio (RATIO lines, -s).
"""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests.conv_ref import ACC_TOL, PREC_TOL, TINY, _check, _dgrad_ref, _fwd_ref, _teeth
from tests.fp64_buffers import BF16_ROUND, GUARD, SENT, V_TH, Buf, _exact_operands, _exact_weights, _random, _st
from tests.util import rel_err

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def H_(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from snn_for_object_detection_amd import _hip
    return _hip


# ---------------------------------------------------------------------------------------------------- plan queries
HALO_KEYS = ("mode", "co_tile", "tiles", "tiles_per_group", "tiles_per_xcd", "co_tiles", "blocks")
WGRAD_KEYS = ("ok", "R", "CW", "wco", "wk", "nks", "npr", "npc", "patches", "splits", "pps", "HR", "HC", "HWD",
              "tiles_co", "tiles_ci")
MODES = {1: "strip", 2: "rect"}


def halo_plan(_hip, N, H, W, Cin, Cout, fps=0):
    out = (ctypes.c_int * 7)()
    rc = _hip.query("snn_conv3x3_halo_plan", N, H, W, Cin, Cout, fps, ctypes.addressof(out))
    assert rc == 0, (N, H, W, Cin, Cout, fps)
    return dict(zip(HALO_KEYS, out))


def s2_plan(_hip, N, H, W, Cin, Ho, Wo, Cout):
    out = (ctypes.c_int * 7)()
    rc = _hip.query("snn_conv3x3_s2_dgrad_plan", N, H, W, Cin, Ho, Wo, Cout, ctypes.addressof(out))
    assert rc == 0, (N, H, W, Cin, Cout)
    return dict(zip(HALO_KEYS, out))


def wgrad_plan(_hip, N, H, W, Cin, Ho, Wo, Cout, s, num_cu=0):
    out = (ctypes.c_int * 16)()
    _hip.query("snn_conv2d_wgrad_halo_plan", N, H, W, Cin, Ho, Wo, Cout, s, num_cu, ctypes.addressof(out))
    return dict(zip(WGRAD_KEYS, out))


def _image(_hip, src, O, I, flip, prec):
    src = src.contiguous().cuda()
    img = torch.empty(9 * O * I, device="cuda")
    table = torch.tensor([[0, 0, O, I]], dtype=torch.int64, device="cuda")
    _hip.call("snn_weight_frag_image_batched", src.data_ptr(), img.data_ptr(), table.data_ptr(), 1,
              9 * (I // 32) * (O // 32) * 128, flip, prec, _st())
    return img


def _ratio(tag, out, ref, mag, tol):
    r = float(((out - ref).abs() / (tol * mag + TINY)).max())
    print(f"RATIO {tag} {r:.4g}")
    return r


# ---------------------------------------------------------------------------------------------------- k_conv_halo3
def _run_halo(_hip, img, x, Cy, prec, *, y_off=0, y_ld=None, adds=(), fps=0, xsp=False, sbf=False):
    """snn_conv3x3_halo (or _spikes) of x [N,H,W,Cx] into a guarded slice; returns (out fp64 CPU, per-(t,c) sums)."""
    N, H, W, Cx = x.shape
    dt = torch.bfloat16 if sbf else torch.float32
    X = Buf(x.shape, values=x, dtype=dt)
    Y = Buf((N, H, W, Cy), y_off, y_ld, fill=float("nan"), dtype=dt)
    A = [Buf((N, H, W, Cy), off, ld, values=v, dtype=dt) for v, off, ld in adds]
    a_args = []
    for i in range(2):
        a_args += [A[i].ptr, A[i].ld] if i < len(A) else [None, 0]
    part = lay = None
    if fps:
        n_part = _hip.query("snn_conv2d_fwd_bn_partial_size", N, fps, H, W, Cy)
        part = torch.full((n_part,), float("nan"), dtype=torch.float64, device="cuda")
        lay = (ctypes.c_int * 2)()
    if xsp:
        _hip.call("snn_conv3x3_halo_spikes", X.ptr, X.ld, V_TH, img.data_ptr(), Y.ptr, Y.ld, N, H, W, Cx, Cy,
                  part.data_ptr() if fps else None, fps, lay, _st())
    else:
        _hip.call("snn_conv3x3_halo", X.ptr, X.ld, img.data_ptr(), Y.ptr, Y.ld, N, H, W, Cx, Cy, *a_args,
                  part.data_ptr() if fps else None, fps, lay, prec, _st())
    sums = None
    if fps:
        assert lay[0] == _hip.query("snn_conv3x3_halo_bn_chunks", fps, H, W) and lay[1] == 0
        sums = torch.empty(N // fps, Cy, 2, dtype=torch.float64, device="cuda")
        _hip.call("snn_bn_stats_reduce", part.data_ptr(), lay[0], lay[1], N // fps, fps * H * W, Cy, sums.data_ptr(), _st())
    torch.cuda.synchronize()
    assert X.guards_intact(whole=True) and all(a.guards_intact(whole=True) for a in A)
    assert Y.guards_intact(), "snn_conv3x3_halo wrote outside its output slice"
    return Y.value(), (None if sums is None else sums.cpu())


def _layer(kind, N, H, W, Cin, Cout):
    """(channels of x, channels of y) of the kernel call for a layer Cin -> Cout."""
    return (Cin, Cout) if kind == "fwd" else (Cout, Cin)


def _halo_case(_hip, kind, N, H, W, Cin, Cout, x, w, prec_name):
    """image and fp64 reference of one call: forward (x [N,H,W,Cin], fp16 x 3 image of w) or data gradient (x = dy
    [N,H,W,Cout], bf16 x 3 image of the transposed weights with mirrored taps)."""
    xd, wd = x.double(), w.double()
    img = _layer_image(_hip, kind, w, prec_name)
    if kind == "fwd":
        return img, _fwd_ref(xd, wd, 1, 1), _fwd_ref(xd.abs(), wd.abs(), 1, 1)
    return img, _dgrad_ref(xd, wd, H, W, 1, 1), _dgrad_ref(xd.abs(), wd.abs(), H, W, 1, 1)


def _layer_image(_hip, kind, w, prec_name="fp16x3"):
    Cout, Cin = w.shape[0], w.shape[3]
    if kind == "fwd":
        return _image(_hip, w, Cout, Cin, 0, _hip.PREC_FP16X3 if prec_name == "fp16x3" else _hip.PREC_BF16X3)
    return _image(_hip, w.permute(3, 1, 2, 0), Cin, Cout, 1, _hip.PREC_BF16X3)


# id, kind, N, H, W, layer Cin, layer Cout, plan mode, channel tile, options
HALO_ROWS = [
    ("strip-co32-fwd-idle", "fwd", 2, 12, 20, 64, 32, "strip", 32, dict(adds=1, idle=True)),
    ("strip-co64-fwd-multi-image", "fwd", 3, 7, 5, 32, 64, "strip", 64, dict(adds=2, multi=True)),
    ("strip-co128-fwd-W78", "fwd", 2, 9, 78, 64, 128, "strip", 128, dict(misaligned=True)),
    ("rect-co32-fwd-W79", "fwd", 2, 9, 79, 32, 32, "rect", 32, dict(misaligned=True, idle=True)),
    ("rect-co64-fwd", "fwd", 1, 6, 100, 64, 64, "rect", 64, dict(adds=1)),
    ("rect-co128-fwd", "fwd", 1, 5, 90, 32, 128, "rect", 128, dict(adds=2)),
    ("strip-co32-dgrad", "dgrad", 2, 11, 30, 32, 64, "strip", 32, dict(adds=2, idle=True)),
    ("strip-co64-dgrad-1px", "dgrad", 3, 1, 1, 64, 64, "strip", 64, dict(adds=1)),
    ("strip-co128-dgrad", "dgrad", 2, 6, 17, 128, 32, "strip", 128, dict(misaligned=True)),
    ("rect-co32-dgrad", "dgrad", 1, 7, 81, 32, 32, "rect", 32, dict(adds=1)),
    ("rect-co64-dgrad-W79", "dgrad", 2, 5, 79, 64, 32, "rect", 64, dict(misaligned=True)),
    ("rect-co128-dgrad", "dgrad", 1, 4, 130, 128, 64, "rect", 128, dict(adds=2)),
]


def _assert_halo_plan(_hip, row, fps=0):
    rid, kind, N, H, W, Cin, Cout, mode, co, opt = row
    Cx, Cy = _layer(kind, N, H, W, Cin, Cout)
    p = halo_plan(_hip, N, H, W, Cx, Cy, fps)
    assert (MODES.get(p["mode"]), p["co_tile"]) == (mode, co), (rid, p)
    assert p["blocks"] == 8 * p["tiles_per_xcd"] * p["co_tiles"] and p["tiles_per_xcd"] * 8 >= p["tiles"], (rid, p)
    if opt.get("idle"):
        assert p["tiles"] % 8 != 0, (rid, p)                     # idle padding blocks in the last XCD share
    if opt.get("multi"):
        assert (H + 1) * (W + 1) < 128 and mode == "strip", rid   # one strip tile holds several images
    return p


@pytest.mark.parametrize("row", HALO_ROWS, ids=[r[0] for r in HALO_ROWS])
def test_halo3_row_against_fp64(H_, row):
    _hip = H_
    rid, kind, N, H, W, Cin, Cout, mode, co, opt = row
    p = _assert_halo_plan(_hip, row)
    Cx, Cy = _layer(kind, N, H, W, Cin, Cout)
    prec_name = "fp16x3" if kind == "fwd" else "bf16x3"
    prec = _hip.PREC_FP16X3 if kind == "fwd" else _hip.PREC_BF16X3
    tol = PREC_TOL[prec_name] + ACC_TOL
    y_off, y_ld = (1, Cy + 4) if opt.get("misaligned") else (0, None)    # y not 16-byte aligned: out_vec = 0
    seed = N * 1000 + H * 10 + W
    for exact in (False, True):
        if exact:
            x, w = _exact_operands((N, H, W, Cx), seed), _exact_weights((Cout, 3, 3, Cin), seed + 1)
            adds = [_exact_operands((N, H, W, Cy), seed + 2 + i, lim=8) for i in range(opt.get("adds", 0))]
        else:
            x, w = _random((N, H, W, Cx), seed), _random((Cout, 3, 3, Cin), seed + 1, (9 * Cin) ** -0.5)
            adds = [_random((N, H, W, Cy), seed + 2 + i) for i in range(opt.get("adds", 0))]
        img, ref, mag = _halo_case(_hip, kind, N, H, W, Cin, Cout, x, w, prec_name)
        a_lay = [(a, 4 * i, Cy + 8) for i, a in enumerate(adds)]           # addends at their own offsets / strides
        out, _ = _run_halo(_hip, img, x, Cy, prec, y_off=y_off, y_ld=y_ld, adds=a_lay)
        what = f"{rid} {'exact' if exact else 'random'} plan {p}"
        want = ref + sum(a.double() for a in adds) if adds else ref
        if exact:
            assert torch.equal(out, want), f"{what}: {int((out != want).sum())} elements differ from fp64"
            continue
        _check(what, out, want, mag, prec_name, extra_mag=sum(a.double().abs() for a in adds) if adds else None)
        _ratio(f"k_conv_halo3 {prec_name} {rid}", out, want, mag + (sum(a.double().abs() for a in adds) if adds else 0), tol)
        c = Cx // 2                                                      # one input channel dropped
        if kind == "fwd":
            drop = _fwd_ref(x.double()[..., c:c + 1], w.double()[..., c:c + 1], 1, 1)
        else:
            drop = _dgrad_ref(x.double()[..., c:c + 1], w.double()[c:c + 1], H, W, 1, 1)
        _teeth(what, out, want - drop, mag, prec_name)


# statistics partials: groups (timesteps) whose last strip tile is partial, and rectangles
BN_ROWS = [("strip-bn-partial-tile", 3, 2, 7, 9, 32, 64, "strip", 64), ("rect-bn", 2, 2, 6, 100, 32, 64, "rect", 64),
           ("strip-bn-co32", 2, 3, 5, 6, 32, 32, "strip", 32), ("rect-bn-co128", 2, 1, 9, 80, 32, 128, "rect", 128)]


@pytest.mark.parametrize("row", BN_ROWS, ids=[r[0] for r in BN_ROWS])
def test_halo3_batchnorm_partials_against_fp64(H_, row):
    _hip = H_
    rid, T, B, H, W, Cin, Cout, mode, co = row
    N = T * B
    p = _assert_halo_plan(_hip, (rid, "fwd", N, H, W, Cin, Cout, mode, co, {}), fps=B)
    assert p["tiles_per_group"] == _hip.query("snn_conv3x3_halo_bn_chunks", B, H, W)
    if mode == "strip":
        assert (B * (H + 1) * (W + 1)) % 128 != 0, rid                  # the last tile of every timestep is partial
    for exact in (False, True):
        if exact:
            x, w = _exact_operands((N, H, W, Cin), T + H), _exact_weights((Cout, 3, 3, Cin), W)
        else:
            x, w = _random((N, H, W, Cin), T + H), _random((Cout, 3, 3, Cin), W, (9 * Cin) ** -0.5)
        img, ref, mag = _halo_case(_hip, "fwd", N, H, W, Cin, Cout, x, w, "fp16x3")
        out, sums = _run_halo(_hip, img, x, Cout, _hip.PREC_FP16X3, fps=B)
        yt = (ref if exact else out).reshape(T, -1, Cout)
        want = torch.stack([yt.sum(1), (yt * yt).sum(1)], -1)
        what = f"{rid} {'exact' if exact else 'random'} plan {p}"
        if exact:
            assert torch.equal(out, ref), what
            assert torch.equal(sums, want), f"{what}: BatchNorm partials differ from the fp64 sums"
        else:
            _check(what, out, ref, mag, "fp16x3")
            scale = torch.stack([yt.abs().sum(1), (yt * yt).sum(1)], -1)
            assert bool(((sums - want).abs() <= 1e-12 * scale + 1e-30).all()), f"{what}: BatchNorm partials"


XSP_ROWS = [r for r in HALO_ROWS if r[1] == "fwd"]


@pytest.mark.parametrize("row", XSP_ROWS, ids=[r[0].replace("fwd", "xsp") for r in XSP_ROWS])
def test_halo3_spikes_from_potentials(H_, row):
    """snn_conv3x3_halo_spikes: the plain kernel's bits on the stored spikes, and within the bound of fp64."""
    _hip = H_
    rid, kind, N, H, W, Cin, Cout, mode, co, opt = row
    p = _assert_halo_plan(_hip, row)
    v = 1.0 + 0.8 * _random((N, H, W, Cin), H + W)
    v.view(-1)[:3] = torch.tensor([V_TH, V_TH + 2 ** -23, 0.0])          # at / just above the threshold
    z = (v > V_TH).float()
    w = _random((Cout, 3, 3, Cin), Cin + Cout, (9 * Cin) ** -0.5)
    img, ref, mag = _halo_case(_hip, "fwd", N, H, W, Cin, Cout, z, w, "fp16x3")
    out, _ = _run_halo(_hip, img, v, Cout, _hip.PREC_FP16X3, xsp=True)
    plain, _ = _run_halo(_hip, img, z, Cout, _hip.PREC_FP16X3)
    what = f"xsp {rid} plan {p}"
    assert torch.equal(out, plain), f"{what}: not the plain kernel's bits on the stored spikes"
    _check(what, out, ref, mag, "fp16x3")
    _ratio(f"k_conv_halo3 xsp {rid}", out, ref, mag, PREC_TOL["fp16x3"] + ACC_TOL)
    zw = z.double().clone()
    zw[..., Cin // 2] = 0
    _teeth(what, out, _fwd_ref(zw, w.double(), 1, 1), mag, "fp16x3")
    wi = _exact_weights((Cout, 3, 3, Cin), 7)                            # spikes x exact weights: exact
    img = _image(_hip, wi, Cout, Cin, 0, _hip.PREC_FP16X3)
    out, _ = _run_halo(_hip, img, v, Cout, _hip.PREC_FP16X3, xsp=True)
    assert torch.equal(out, _fwd_ref(z.double(), wi.double(), 1, 1)), f"{what}: exact operands"


SBF_ROWS = [("strip-sbf", 2, 12, 20, 64, 64, "strip", 64), ("rect-sbf", 1, 6, 100, 64, 128, "rect", 128)]


@pytest.mark.parametrize("row", SBF_ROWS, ids=[r[0] for r in SBF_ROWS])
def test_halo3_bf16_storage(H_, row):
    """SBF: bf16 x / y, one product of the bf16 weights.  Against fp64 of the stored bf16 operands, one bf16 rounding of
    the result on top of the accumulation bound; exact operands: the bf16 rounding of the exact result."""
    _hip = H_
    rid, N, H, W, Cin, Cout, mode, co = row
    p = _assert_halo_plan(_hip, (rid, "fwd", N, H, W, Cin, Cout, mode, co, {}))
    for exact in (False, True):
        if exact:
            x, w = _exact_operands((N, H, W, Cin), N + W), _exact_weights((Cout, 3, 3, Cin), H)
        else:
            x, w = _random((N, H, W, Cin), N + W), _random((Cout, 3, 3, Cin), H, (9 * Cin) ** -0.5)
        xb, wb = x.bfloat16().float(), w.bfloat16().float()             # the stored operands
        img, ref, mag = _halo_case(_hip, "fwd", N, H, W, Cin, Cout, xb, wb, "bf16s")
        img = _image(_hip, w, Cout, Cin, 0, _hip.PREC_BF16X3)            # the kernel rounds w itself (hi pieces)
        out, _ = _run_halo(_hip, img, xb, Cout, _hip.PREC_BF16S, sbf=True)
        what = f"{rid} {'exact' if exact else 'random'} plan {p}"
        if exact:
            assert torch.equal(out, ref.float().bfloat16().double()), what
            continue
        bound = ACC_TOL * mag + BF16_ROUND * ref.abs() + TINY
        err = (out - ref).abs()
        assert bool((err <= bound).all()), f"{what}: {int((err > bound).sum())} elements off"
        print(f"RATIO k_conv_halo3 bf16s {rid} {float((err / bound).max()):.4g}")
        wrong = ref.clone()
        wrong[:, :, -1] = 0                                              # the last column (a partial RECT edge) dropped
        assert not bool(((out - wrong).abs() <= ACC_TOL * mag + BF16_ROUND * wrong.abs() + TINY).all()), what


# ---------------------------------------------------------------------------------------------------- k_conv_s2dgrad3
# id, N, H, W, Cin (dx), Cout (dy), mode, addends, bf16 storage
S2_ROWS = [
    ("s2-strip-odd", 2, 13, 17, 64, 32, "strip", 1, False),
    ("s2-strip-even", 2, 10, 16, 128, 64, "strip", 2, False),
    ("s2-strip-Wo157", 1, 4, 313, 64, 32, "strip", 0, False),     # the widest strip row; odd W
    ("s2-rect-Wo158", 1, 5, 315, 64, 32, "rect", 1, False),       # the narrowest rectangle row; odd H, W
    ("s2-rect-even", 1, 6, 316, 64, 64, "rect", 2, False),
    ("s2-strip-sbf", 2, 13, 17, 64, 32, "strip", 0, True),
    ("s2-rect-sbf", 1, 5, 315, 64, 32, "rect", 1, True),
]


def _run_s2(_hip, img, dy, H, W, Cin, adds, sbf):
    N, Ho, Wo, Cout = dy.shape
    dt = torch.bfloat16 if sbf else torch.float32
    DY = Buf(dy.shape, values=dy, dtype=dt)
    DX = Buf((N, H, W, Cin), 4, Cin + 12, fill=float("nan"), dtype=dt)
    A = [Buf((N, H, W, Cin), 4 * i, Cin + 8, values=a, dtype=dt) for i, a in enumerate(adds)]
    a_args = []
    for i in range(2):
        a_args += [A[i].ptr, A[i].ld] if i < len(A) else [None, 0]
    _hip.call("snn_conv3x3_s2_dgrad", DY.ptr, DY.ld, img.data_ptr(), DX.ptr, DX.ld, N, H, W, Cin, Ho, Wo, Cout, *a_args,
              _hip.PREC_BF16S if sbf else _hip.PREC_BF16X3, _st())
    torch.cuda.synchronize()
    assert DY.guards_intact(whole=True) and all(a.guards_intact(whole=True) for a in A)
    assert DX.guards_intact(), "snn_conv3x3_s2_dgrad wrote outside its output slice"
    return DX.value()


@pytest.mark.parametrize("row", S2_ROWS, ids=[r[0] for r in S2_ROWS])
def test_s2dgrad_row_against_fp64(H_, row):
    _hip = H_
    rid, N, H, W, Cin, Cout, mode, nadd, sbf = row
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    p = s2_plan(_hip, N, H, W, Cin, Ho, Wo, Cout)
    assert (MODES.get(p["mode"]), p["co_tile"]) == (mode, 64), (rid, p)
    assert p["blocks"] == 8 * p["tiles_per_xcd"] * p["co_tiles"], (rid, p)
    tol = PREC_TOL["bf16x3"] + ACC_TOL
    for exact in (False, True):
        if exact:
            dy, w = _exact_operands((N, Ho, Wo, Cout), N + H), _exact_weights((Cout, 3, 3, Cin), W)
            adds = [_exact_operands((N, H, W, Cin), 5 + i, lim=8) for i in range(nadd)]
        else:
            dy, w = _random((N, Ho, Wo, Cout), N + H), _random((Cout, 3, 3, Cin), W, (9 * Cin) ** -0.5)
            adds = [_random((N, H, W, Cin), 5 + i) for i in range(nadd)]
        if sbf:
            dy, w, adds = dy.bfloat16().float(), w.bfloat16().float(), [a.bfloat16().float() for a in adds]
        img = _image(_hip, w.permute(3, 1, 2, 0), Cin, Cout, 1, _hip.PREC_BF16X3)
        dyd, wd = dy.double(), w.double()
        ref = _dgrad_ref(dyd, wd, H, W, 2, 1) + sum(a.double() for a in adds)
        mag = _dgrad_ref(dyd.abs(), wd.abs(), H, W, 2, 1) + sum(a.double().abs() for a in adds)
        out = _run_s2(_hip, img, dy, H, W, Cin, adds, sbf)
        what = f"{rid} {'exact' if exact else 'random'} plan {p}"
        if exact:
            want = ref.float().bfloat16().double() if sbf else ref
            assert torch.equal(out, want), f"{what}: {int((out != want).sum())} elements differ from fp64"
            continue
        if sbf:
            bound = ACC_TOL * mag + BF16_ROUND * ref.abs() + TINY
            assert bool(((out - ref).abs() <= bound).all()), what
            print(f"RATIO k_conv_s2dgrad3 bf16s {rid} {float(((out - ref).abs() / bound).max()):.4g}")
        else:
            _check(what, out, ref, mag, "bf16x3")
            _ratio(f"k_conv_s2dgrad3 bf16x3 {rid}", out, ref, mag, tol)
        wrong = ref.clone()
        wrong[:, :, W - 1] += (2.0 ** -6 if sbf else 2.0 ** -10) * mag[:, :, W - 1]   # the last dx column, slightly off
        ok = bool(((out - wrong).abs() <= (BF16_ROUND * wrong.abs() if sbf else 0) + tol * mag + TINY).all())
        assert not ok, f"{what}: the bound does not see a small error in the last column"


# ---------------------------------------------------------------------------------------------------- NaN locality / range
def _poison_mask(N, H, W, pts, s2=False, OH=None, OW=None):
    """[N, OH, OW] output pixels a NaN at each (n, y, x) of the input grid must reach: the 3x3 neighbourhood in its image
    (stride 2: dx rows 2a-1 .. 2a+1, columns alike)."""
    OH, OW = (H, W) if not s2 else (OH, OW)
    m = torch.zeros(N, OH, OW, dtype=torch.bool)
    for n, y, x in pts:
        c = (2 * y, 2 * x) if s2 else (y, x)
        m[n, max(c[0] - 1, 0):min(c[0] + 2, OH), max(c[1] - 1, 0):min(c[1] + 2, OW)] = True
    return m


# id, kind, N, H, W, layer Cin, layer Cout, NaN positions (n, y, x) of the kernel's input
NAN_ROWS = [
    # corner; last column; first row of the next image, inside the same 128-cell strip tile (48-cell images)
    ("strip-fwd", "fwd", 3, 5, 7, 32, 64, [(0, 0, 0), (0, 2, 6), (1, 0, 3)]),
    ("strip-dgrad", "dgrad", 3, 5, 7, 64, 32, [(0, 0, 0), (0, 2, 6), (1, 0, 3)]),
    # rectangle edges (columns 31 | 32, rows 3 | 4) and the last column of the partial rectangle
    ("rect-fwd", "fwd", 2, 9, 79, 32, 64, [(0, 3, 31), (0, 4, 32), (1, 5, 78), (1, 8, 0)]),
    ("rect-dgrad", "dgrad", 2, 9, 79, 64, 32, [(0, 3, 31), (0, 4, 32), (1, 5, 78), (1, 8, 0)]),
]


@pytest.mark.parametrize("row", NAN_ROWS, ids=[r[0] for r in NAN_ROWS])
def test_halo3_nan_reaches_exactly_its_neighbourhood(H_, row):
    _hip = H_
    rid, kind, N, H, W, Cin, Cout, pts = row
    Cx, Cy = _layer(kind, N, H, W, Cin, Cout)
    w = _exact_weights((Cout, 3, 3, Cin), 3)
    x = torch.zeros(N, H, W, Cx)
    for n, y, xx in pts:
        x[n, y, xx, 1] = float("nan")
    img = _layer_image(_hip, kind, w)
    prec = _hip.PREC_FP16X3 if kind == "fwd" else _hip.PREC_BF16X3
    out, _ = _run_halo(_hip, img, x, Cy, prec)
    bad = ~torch.isfinite(out)
    want = _poison_mask(N, H, W, pts)[..., None].expand_as(bad)
    assert torch.equal(bad, want), f"{rid}: {int((bad != want).sum())} outputs differ from the NaN neighbourhood"


S2_NAN_ROWS = [
    ("s2-strip", 2, 13, 17, 64, 32, [(0, 0, 0), (0, 3, 8), (1, 0, 2)]),
    ("s2-rect", 1, 9, 315, 64, 32, [(0, 1, 31), (0, 0, 32), (0, 4, 157), (0, 3, 0)]),
]


@pytest.mark.parametrize("row", S2_NAN_ROWS, ids=[r[0] for r in S2_NAN_ROWS])
def test_s2dgrad_nan_reaches_exactly_its_neighbourhood(H_, row):
    _hip = H_
    rid, N, H, W, Cin, Cout, pts = row
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    w = _exact_weights((Cout, 3, 3, Cin), 4)
    dy = torch.zeros(N, Ho, Wo, Cout)
    for n, y, x in pts:
        dy[n, y, x, 2] = float("nan")
    img = _image(_hip, w.permute(3, 1, 2, 0), Cin, Cout, 1, _hip.PREC_BF16X3)
    out = _run_s2(_hip, img, dy, H, W, Cin, [], False)
    bad = ~torch.isfinite(out)
    want = _poison_mask(N, Ho, Wo, pts, s2=True, OH=H, OW=W)[..., None].expand_as(bad)
    assert torch.equal(bad, want), f"{rid}: {int((bad != want).sum())} outputs differ from the NaN neighbourhood"


@pytest.mark.parametrize("shape", [(2, 6, 20, 64, 64), (1, 6, 90, 32, 128)], ids=["strip", "rect"])
def test_halo3_fp16x3_range_contract(H_, shape):
    """x * 2^4 must fit fp16: |x| >= 4095 rounds to inf (non-finite outputs, exactly the neighbourhood), |x| = 4094 is
    still exact (2^4 * 4094 = 65504, the largest fp16) and within the bound; small |x| stays within
    test_gpu_ops.py::test_fp16x3_range_contract's graceful bounds."""
    _hip = H_
    N, H, W, Cin, Cout = shape
    w = _random((Cout, 3, 3, Cin), 1, (9 * Cin) ** -0.5)
    img = _image(_hip, w, Cout, Cin, 0, _hip.PREC_FP16X3)
    pts = [(0, 2, 5), (N - 1, H - 1, W - 1)]
    for big, loud in ((4094.0, False), (4095.0, True), (1e5, True)):
        x = _random((N, H, W, Cin), 2)
        for n, y, xx in pts:
            x[n, y, xx, 3] = big
        out, _ = _run_halo(_hip, img, x, Cout, _hip.PREC_FP16X3)
        bad = ~torch.isfinite(out)
        if loud:
            assert torch.equal(bad, _poison_mask(N, H, W, pts)[..., None].expand_as(bad)), big
        else:
            xd, wd = x.double(), w.double()
            _check(f"|x| = {big}", out, _fwd_ref(xd, wd, 1, 1), _fwd_ref(xd.abs(), wd.abs(), 1, 1), "fp16x3")
    for scale, tol in ((1e-2, 1.5e-6), (1e-4, 1e-4)):
        x = _random((N, H, W, Cin), 3, scale)
        out, _ = _run_halo(_hip, img, x, Cout, _hip.PREC_FP16X3)
        assert rel_err(out, _fwd_ref(x.double(), w.double(), 1, 1)) < tol, scale


# ---------------------------------------------------------------------------------------------------- k_conv_wgrad_halo
def _wgrad64(x, dy, s, rows=None):
    """dw [Co,3,3,Ci] = sum over pixels of dy * shifted x, in fp64 (one GEMM per tap); rows: output rows to sum over."""
    Co, Ci = dy.shape[3], x.shape[3]
    Ho, Wo = dy.shape[1], dy.shape[2]
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    r0, r1 = (0, Ho) if rows is None else rows
    D = dy[:, r0:r1].reshape(-1, Co)
    out = torch.empty(Co, 3, 3, Ci, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            xs = xp[:, kh + s * r0:kh + s * (r1 - 1) + 1:s, kw:kw + s * (Wo - 1) + 1:s].reshape(-1, Ci)
            out[:, kh, kw] = D.t() @ xs
    return out


# id, N, H, W, Cout, stride, features the plan must show, extras.  Cin = 32 throughout (the fp64 references are GEMMs
# over 150 000+ pixels).  With the 256 CUs of an MI355X every covered shape plans 8k splits (s >= 16 rounds to whole
# groups of 8) and several (not zero) splits; split counts of 1 or not a multiple of 8 need > 256 channel tiles or far
# fewer CUs (test_host_logic.py::test_halo_plan_invariants shows both on the host).
WGRAD_ROWS = [
    ("s1-wco1", 1, 310, 517, 32, 1, {"partial", "idle_splits"}, {"accumulate"}),
    ("s1-wco2-masked-k", 3, 390, 161, 64, 1, {"partial", "idle_splits", "masked_k"}, {"sb"}),
    ("s1-wco4", 1, 310, 517, 128, 1, {"partial", "idle_splits"}, set()),
    ("s2-wco1-nks", 1, 591, 1034, 32, 2, {"partial", "idle_splits", "nks_wk"}, {"sb"}),
    ("s2-wco2", 1, 625, 1034, 64, 2, {"partial", "idle_splits"}, set()),
    ("s2-wco4", 1, 591, 1034, 128, 2, {"partial", "idle_splits"}, {"accumulate"}),
    ("s1-150000px", 1, 60, 2500, 32, 1, {"idle_splits"}, set()),
    ("s1-149999px", 1, 61, 2459, 32, 1, {"below"}, set()),
]


def _run_wgrad(_hip, x, dy, s, prec, *, spikes=False, old=None, sb=False):
    N, H, W, Cin = x.shape
    _, Ho, Wo, Cout = dy.shape
    dt = torch.bfloat16 if sb else torch.float32
    X = Buf(x.shape, values=x, dtype=dt)
    DY = Buf(dy.shape, values=dy, dtype=dt)
    n = Cout * 9 * Cin
    dwb = torch.full((n + 8,), SENT, device="cuda")
    if old is not None:
        dwb[4:4 + n] = old.reshape(-1).cuda()
    else:
        dwb[4:4 + n] = float("nan")
    before = dwb.clone()
    splitk = _hip.query("snn_conv2d_wgrad_splitk", N, H, W, Cin, Ho, Wo, Cout, 3, 3, s, 1, prec)
    ws = torch.full((splitk, n), float("nan"), device="cuda")               # a slab nobody writes poisons dw
    acc = int(old is not None)
    if spikes:
        _hip.call("snn_conv2d_spikes_wgrad", X.ptr, X.ld, V_TH, DY.ptr, DY.ld, dwb[4:].data_ptr(), N, H, W, Cin, Ho, Wo,
                  Cout, 3, 3, s, 1, acc, ws.data_ptr(), splitk, _st())
    else:
        _hip.call("snn_conv2d_wgrad", X.ptr, X.ld, DY.ptr, DY.ld, dwb[4:].data_ptr(), N, H, W, Cin, Ho, Wo, Cout, 3, 3, s, 1,
                  acc, ws.data_ptr(), splitk, prec, _st())
    torch.cuda.synchronize()
    assert X.guards_intact(whole=True) and DY.guards_intact(whole=True)
    a, b = dwb.view(torch.int32), before.view(torch.int32)
    assert torch.equal(a[:4], b[:4]) and torch.equal(a[4 + n:], b[4 + n:]), "snn_conv2d_wgrad wrote outside dw"
    return dwb[4:4 + n].double().cpu().reshape(Cout, 3, 3, Cin), splitk


@pytest.mark.parametrize("row", WGRAD_ROWS, ids=[r[0] for r in WGRAD_ROWS])
def test_wgrad_halo_row_against_fp64(H_, row):
    _hip = H_
    rid, N, H, W, Cout, s, feats, extra = row
    Cin = 32
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    p = wgrad_plan(_hip, N, H, W, Cin, Ho, Wo, Cout, s)
    assert p == wgrad_plan(_hip, N, H, W, Cin, Ho, Wo, Cout, s, num_cu)
    what = f"{rid} ({N * Ho * Wo} px, {num_cu} CUs) plan {p}"
    kern = _hip.query("snn_conv2d_wgrad_kernel", N, H, W, Cin, Ho, Wo, Cout, 3, 3, s, 1, _hip.PREC_BF16X3)
    if "below" in feats:
        assert N * Ho * Wo == 149_999 and p["ok"] == 0 and kern == 0, what
    else:
        assert N * Ho * Wo >= 150_000 and p["ok"] == 1 and kern == 1, what
        assert p["wco"] == {32: 1, 64: 2, 128: 4}[Cout] and p["wco"] * p["wk"] == 4, what
        assert p["splits"] == _hip.query("snn_conv2d_wgrad_splitk", N, H, W, Cin, Ho, Wo, Cout, 3, 3, s, 1,
                                         _hip.PREC_BF16X3), what
        assert ("partial" in feats) == (Ho % p["R"] != 0 and Wo % p["CW"] != 0), what
        assert ("idle_splits" in feats) == ((p["splits"] - 1) * p["pps"] >= p["patches"]), what
        assert ("masked_k" in feats) == (p["R"] * p["CW"] % 16 != 0), what
        assert ("nks_wk" in feats) == (p["nks"] % p["wk"] != 0), what
    print(f"PLAN {what}")
    # random operands: bf16 x 3 and bf16 x 1 share the reference
    x, dy = _random((N, H, W, Cin), Ho), _random((N, Ho, Wo, Cout), Wo)
    xd, dyd = x.double(), dy.double()
    ref, mag = _wgrad64(xd, dyd, s), _wgrad64(xd.abs(), dyd.abs(), s)
    last = _wgrad64(xd, dyd, s, rows=(Ho - 1, Ho))                         # the bottom row of output pixels
    modes = [("bf16x3", _hip.PREC_BF16X3), ("bf16x1", _hip.PREC_BF16X1)] if "below" not in feats else [("bf16x3", _hip.PREC_BF16X3)]
    for name, prec in modes:
        out, _ = _run_wgrad(_hip, x, dy, s, prec)
        _check(f"{what} {name}", out, ref, mag, name)
        _ratio(f"k_conv_wgrad_halo {name} {rid}", out, ref, mag, PREC_TOL[name] + ACC_TOL)
        if name == "bf16x3":   # (one output row is ~2^-12 of mag: below the bf16 x 1 bound)
            _teeth(f"{what} {name}", out, ref - last, mag, name)
    if "accumulate" in extra:
        old = _random((Cout, 3, 3, Cin), 99)
        out, _ = _run_wgrad(_hip, x, dy, s, _hip.PREC_BF16X3, old=old)
        _check(f"{what} accumulate", out, ref + old.double(), mag, "bf16x3", extra_mag=old.double().abs())
    if "sb" in extra:                                                      # bf16 storage: exact operands of the product
        xb, dyb = x.bfloat16().float(), dy.bfloat16().float()
        rb, mb = _wgrad64(xb.double(), dyb.double(), s), _wgrad64(xb.double().abs(), dyb.double().abs(), s)
        out, _ = _run_wgrad(_hip, xb, dyb, s, _hip.PREC_BF16S, sb=True)
        ok = bool(((out - rb).abs() <= ACC_TOL * mb + TINY).all())
        assert ok, f"{what} bf16s: {int(((out - rb).abs() > ACC_TOL * mb + TINY).sum())} elements off"
        _ratio(f"k_conv_wgrad_halo bf16s {rid}", out, rb, mb, ACC_TOL)
    if "below" in feats:
        return
    # exact operands: small integers (spikes for NPROD 2): every mode equals fp64 bit for bit
    xi, dyi = _exact_operands((N, H, W, Cin), 1, lim=3), _exact_operands((N, Ho, Wo, Cout), 2, lim=3)
    refi = _wgrad64(xi.double(), dyi.double(), s).float().double()
    for name, prec in modes:
        out, _ = _run_wgrad(_hip, xi, dyi, s, prec)
        assert torch.equal(out, refi), f"{what} {name} exact: {int((out != refi).sum())} elements differ"
    if "sb" in extra:
        out, _ = _run_wgrad(_hip, xi, dyi, s, _hip.PREC_BF16S, sb=True)
        assert torch.equal(out, refi), f"{what} bf16s exact"
    if "accumulate" in extra:
        old = _exact_operands((Cout, 3, 3, Cin), 3) * 0.25
        out, _ = _run_wgrad(_hip, xi, dyi, s, _hip.PREC_BF16X3, old=old)
        assert torch.equal(out, refi + old.double()), f"{what} accumulate exact"
    v = xi.abs() * 0.75 + 0.5 * (xi == 0).float() - 0.25 * (xi.abs() == 1).float()   # 0 -> 0.5, 1 -> 0.5, 2+ -> 1.5+
    z = (v > V_TH).double()
    out, _ = _run_wgrad(_hip, v, dyi, s, _hip.PREC_BF16X3, spikes=True)
    refz = _wgrad64(z, dyi.double(), s)
    assert torch.equal(out, refz), f"{what} spikes (NPROD 2) exact: {int((out != refz).sum())} elements differ"
