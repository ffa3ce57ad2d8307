"""Padded pooling and SPP, host side (no GPU): the C ABI additions, the fp64 references of tests/pool_ref.py against CPU
torch, ``Pool(padding=...)`` / ``SPP()`` and what they refuse, ``BlockGen`` channel accounting, and the launchers'
refusals (which arrive before any launch)."""
import ctypes
import os
import re
from ctypes import c_int, c_int64, c_void_p

import pytest
import torch
import torch.nn.functional as F

from tests import pool_ref as R
import snn_for_object_detection_amd as S
from snn_for_object_detection_amd.layer_gen import AvgPool2d, HipSPP, MaxPool2d, SumPool2d

NEW = {
    "snn_pool2d_supported": (c_int, [c_int64] + [c_int] * 6),
    "snn_pool2d_fwd": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_int64] + [c_int] * 6 + [c_void_p]),
    "snn_pool2d_bwd": (c_int, [c_int, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int64]
                       + [c_int] * 6 + [c_void_p]),
    "snn_spp_supported": (c_int, [c_int64] + [c_int] * 5),
    "snn_spp_fwd": (c_int, [c_void_p, c_int64, c_void_p, c_int64, c_int64] + [c_int] * 5 + [c_void_p]),
}
SIZES = [(1, 1), (2, 7), (5, 5), (13, 9)]
KINDS = ["binary", "normal", "nan", "inf"]
KSP = [(2, 2, 0), (3, 2, 1), (5, 1, 2), (3, 1, 1), (4, 3, 1), (7, 1, 3), (5, 2, 0), (2, 1, 1)]


def test_abi_declares_exports_and_binds_the_pooling_symbols(hip_lib):
    from snn_for_object_detection_amd import _build, _hip
    root = os.path.dirname(_hip._HERE)
    header = re.sub(r"/\*.*?\*/", " ", open(os.path.join(root, "include", "snn_hip.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name, sig in NEW.items():
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/snn_hip.h"
        assert hasattr(raw, name), f"{name} is not exported"
        assert _hip.SIGNATURES[name] == sig, name
        fn = getattr(hip_lib, name)
        assert fn.restype is sig[0] and list(fn.argtypes) == sig[1]
    assert "pool.hip" in _build.SOURCES
    assert _hip.ABI_VERSION == 20 and hip_lib.snn_abi_version() == 20     # symbols were added, nothing changed
    integration = open(os.path.join(root, "INTEGRATION.md")).read()
    for name in NEW:
        assert name in integration, f"{name} is not described in INTEGRATION.md"


# ------------------------------------------------------------------------------------------ references against torch
def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _same(a, b):
    """Equal where finite, the same infinities, NaN where the other has NaN."""
    a, b = a.double(), b.double()
    return a.shape == b.shape and bool((((a != a) & (b != b)) | (a == b)).all())


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_max_references_against_torch(kind, H, W):
    x = R.inputs(kind, (3, H, W, 3), seed=H * 16 + W).double()
    for k, s, p in KSP:
        if H + 2 * p < k or W + 2 * p < k:
            continue
        Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
        xt = _nchw(x).requires_grad_()
        yt = F.max_pool2d(xt, k, s, p)
        y, _ = R.pool2d_fwd_ref(R.POOL_MAX, x, k, s, p)
        assert _same(y, _nhwc(yt.detach())), (k, s, p)
        g = torch.randint(-4, 5, (3, Ho, Wo, 3), generator=torch.Generator().manual_seed(k)).double()
        add = torch.randint(-4, 5, x.shape, generator=torch.Generator().manual_seed(s)).double()
        yt.backward(_nchw(g))
        gx, _ = R.pool2d_bwd_ref(R.POOL_MAX, x, g, k, s, p)
        assert torch.equal(gx, _nhwc(xt.grad)), (k, s, p)       # integer gradients: every sum is exact
        gxa, _ = R.pool2d_bwd_ref(R.POOL_MAX, x, g, k, s, p, addend=add)
        assert torch.equal(gxa, _nhwc(xt.grad) + add)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_avg_and_sum_references_against_torch(kind, H, W):
    x = R.inputs(kind, (2, H, W, 3), seed=H * 16 + W + 1).double()
    for k, s, p in KSP:
        if H + 2 * p < k or W + 2 * p < k:
            continue
        xt = _nchw(x).requires_grad_()
        yt = F.avg_pool2d(xt, k, s, p)                          # count_include_pad=True: the divisor is k * k
        ya, mag = R.pool2d_fwd_ref(R.POOL_AVG, x, k, s, p)
        ys, _ = R.pool2d_fwd_ref(R.POOL_SUM, x, k, s, p)
        ref = _nhwc(yt.detach())
        fin = torch.isfinite(ref)
        assert bool((torch.isfinite(ya) == fin).all())
        assert bool(((ya - ref).abs()[fin] <= 1e-13 * mag[fin] + 1e-300).all()), (k, s, p)
        assert bool(((ys - ref * k * k).abs()[fin] <= 1e-13 * (mag * k * k)[fin] + 1e-300).all())
        if kind in ("nan", "inf"):
            assert _same(torch.where(fin, torch.zeros_like(ya), ya), torch.where(fin, torch.zeros_like(ref), ref))
        g = torch.randint(-4, 5, ref.shape, generator=torch.Generator().manual_seed(k)).double()
        yt.backward(_nchw(g))
        ga, maga = R.pool2d_bwd_ref(R.POOL_AVG, x, g, k, s, p)
        gs, _ = R.pool2d_bwd_ref(R.POOL_SUM, x, g, k, s, p)
        assert bool(((ga - _nhwc(xt.grad)).abs() <= 1e-13 * maga + 1e-300).all())
        assert bool(((gs - _nhwc(xt.grad) * k * k).abs() <= 1e-13 * maga * k * k + 1e-300).all())


def _chain(xt, k, levels):
    outs = [xt]
    for _ in range(levels):
        outs.append(F.max_pool2d(outs[-1], k, 1, k // 2))
    return torch.cat(outs, dim=1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("H,W", SIZES)
def test_spp_references_against_torch_autograd_through_the_chain(kind, H, W):
    C = 2
    x = R.inputs(kind, (3, H, W, C), seed=H * 16 + W + 2).double()
    for k in (3, 5):
        for levels in (1, 2, 3):
            xt = _nchw(x).requires_grad_()
            yt = _chain(xt, k, levels)
            y = R.spp_fwd_ref(x, k, levels)
            assert _same(y, _nhwc(yt.detach())), (k, levels)
            g = torch.randint(-4, 5, y.shape, generator=torch.Generator().manual_seed(k * levels)).double()
            yt.backward(_nchw(g))
            gx, _ = R.spp_bwd_ref(y, g, k, levels)
            assert torch.equal(gx, _nhwc(xt.grad)), (k, levels)
            # the chain equals one max pool of window j (k - 1) + 1 per slice - in VALUE
            for j in range(1, levels + 1):
                kj = j * (k - 1) + 1
                one = F.max_pool2d(_nchw(x), kj, 1, kj // 2)
                assert _same(y[..., j * C:(j + 1) * C], _nhwc(one))


def test_spp_backward_sums_stay_exact_in_fp32():
    """All ties (a constant frame), k = 5, 3 levels, |g| <= 4: the largest |partial sum| of the recursion is the bound the
    issue states (336), far below 2^24 - so the GPU tests may ask for equality."""
    x = torch.ones((1, 13, 9, 1))
    y = R.spp_fwd_ref(x, 5, 3)
    g = torch.full(y.shape, 4.0)
    gx, mag = R.spp_bwd_ref(y, g, 5, 3)
    assert float(gx.abs().max()) == 336.0 and float(mag.max()) < 2 ** 24
    assert float(gx.sum()) == float(g.sum())                    # a max pool moves gradient, it neither makes nor loses any


def test_parallel_spelling_differs_where_maxima_tie():
    x = R.inputs("binary", (1, 13, 9, 1), seed=5).double()
    xt = _nchw(x).requires_grad_()
    par = torch.cat([xt] + [F.max_pool2d(xt, kj, 1, kj // 2) for kj in (5, 9, 13)], dim=1)
    g = torch.randint(-4, 5, par.shape, generator=torch.Generator().manual_seed(1)).double()
    par.backward(g)
    y = R.spp_fwd_ref(x, 5, 3)
    gx, _ = R.spp_bwd_ref(y, _nhwc(g), 5, 3)
    assert _same(y, _nhwc(par.detach())) and not torch.equal(gx, _nhwc(xt.grad))


# ------------------------------------------------------------------------------------------ generators
def test_pool_without_padding_builds_the_module_it_always_built():
    for t, cls in (("A", AvgPool2d), ("M", MaxPool2d), ("S", SumPool2d)):
        m, out = S.Pool(t, 2).get(7)
        assert type(m) is cls and out == 7 and (m.kernel_size, m.stride, m.padding) == (2, 2, 0)
        m, out = S.Pool(t, 3, 1).get(5)
        assert type(m) is cls and out == 5 and (m.kernel_size, m.stride, m.padding) == (3, 1, 0)
    gen = S.Pool("M")
    assert (gen.type, gen.kernel_size, gen.stride, gen.padding) == ("M", 2, 2, 0)
    assert not list(S.Pool("M", 2).get(3)[0].parameters())
    with pytest.raises(ValueError):
        S.Pool("X", 2)


def test_padded_pool_and_spp_modules(hip_lib):
    for t, cls in (("A", AvgPool2d), ("M", MaxPool2d), ("S", SumPool2d)):
        for k, s, p in ((5, 1, 2), (3, 2, 1), (7, 1, 3), (4, 3, 1), (2, 1, 1)):
            m, out = S.Pool(t, k, s, p).get(6)
            assert type(m) is cls and out == 6 and (m.kernel_size, m.stride, m.padding) == (k, s, p)
    m, out = S.Pool("M", 3, padding=1).get(4)                    # stride defaults to the window
    assert (m.kernel_size, m.stride, m.padding) == (3, 3, 1)
    m, out = S.SPP().get(6)
    assert type(m) is HipSPP and out == 24 and (m.kernel_size, m.levels) == (5, 3) and not list(m.parameters())
    m, out = S.SPP(3, 2).get(6)
    assert out == 18 and (m.kernel_size, m.levels) == (3, 2)
    assert S.SPP(5, 1).get(3)[1] == 6
    assert "SPP" in S.layer_gen.layers_list and S.HipSPP is HipSPP


def test_blockgen_channel_accounting(hip_lib):
    blk = S.BlockGen(6, [S.SPP(5, 3)])
    assert blk.out_channels == 24 and isinstance(blk.net[0][0], HipSPP) and blk.branch_state[0] == [False]
    den = S.BlockGen(6, S.Dense([[S.SPP(3, 2)], [S.Pass()]]))
    assert den.out_channels == 24 and den._offsets == [0, 18] and den._pass_offset == 18
    P = lambda: S.Pool("M", 5, 1, 2)
    spelled = S.BlockGen(6, S.Dense([[S.Pass()], [P()], [P(), P()], [P(), P(), P()]]))
    assert spelled.out_channels == 24
    stage = S.BlockGen(8, [S.Conv(16, 1), S.Norm(), S.LIF(), S.SPP(), S.Conv(32, 1), S.Norm(), S.LIF()])
    assert stage.out_channels == 32 and stage.net[0][4].in_channels == 64
    assert stage._plan[0] == [("layer", 0, 1), ("norm_neuron", 1, 2), ("layer", 3, 1), ("layer", 4, 1), ("norm_neuron", 5, 2)]
    from snn_for_object_detection_amd import generator as G
    assert not G._takes_potentials(stage.net[0][3])              # the LIF in front of an SPP writes its spikes
    # boundedness is handed on: SumPool upstream makes the convolution behind the SPP take the any-range arithmetic
    unb = S.BlockGen(8, [S.Pool("S", 3, 1, 1), S.SPP(3, 1), S.Conv(8, 1)])
    assert unb.net[0][2].forward_precision == "bf16x6"
    bnd = S.BlockGen(8, [S.Pool("M", 3, 1, 1), S.SPP(3, 1), S.Conv(8, 1)])
    assert bnd.net[0][2].forward_precision is None


@pytest.mark.parametrize("gen,names", [
    (lambda: S.Pool("M", 5, 1, 3), ("padding", "{0, 1, 2}")),         # pad > k / 2
    (lambda: S.Pool("A", 3, 1, 2), ("padding", "{0, 1}")),
    (lambda: S.Pool("M", 3, 1, -1), ("padding", "{0, 1}")),
    (lambda: S.Pool("M", 3, 1, True), ("padding", "{0, 1}")),
    (lambda: S.Pool("M", 8, 1, 1), ("kernel_size", "{2, 3, 4, 5, 6, 7}")),   # k outside the set
    (lambda: S.Pool("S", 1, 1, 1), ("kernel_size", "{2, 3, 4, 5, 6, 7}")),
    (lambda: S.Pool("M", 3, 4, 1), ("stride", "{1, 2, 3}")),
    (lambda: S.Pool("M", 3, 0, 1), ("stride", "{1, 2, 3}")),
    (lambda: S.SPP(4), ("kernel_size", "{3, 5}")),                    # even window
    (lambda: S.SPP(7), ("kernel_size", "{3, 5}")),
    (lambda: S.SPP(5, 4), ("levels", "{1, 2, 3}")),
    (lambda: S.SPP(3, 0), ("levels", "{1, 2, 3}")),
])
def test_generators_refuse_by_name(hip_lib, gen, names):
    g = gen()                                                # (a description is written before the channels are known)
    with pytest.raises(ValueError) as e:
        g.get(8)
    for n in names:
        assert n in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        S.BlockGen(8, [g])


# ------------------------------------------------------------------------------------------ the library's own checks
def test_supported_queries(hip_lib):
    q, qs = hip_lib.snn_pool2d_supported, hip_lib.snn_spp_supported
    for k in range(2, 8):
        for s in range(1, k + 1):
            for p in range(0, k // 2 + 1):
                assert q(160, 76, 60, 64, k, s, p) == 1, (k, s, p)
                assert q(1, max(1, k - 2 * p), max(1, k - 2 * p), 1, k, s, p) == 1, (k, s, p)   # exactly one window
    for bad in ((1, 8, 8, 4, 1, 1, 0), (1, 8, 8, 4, 8, 1, 0), (1, 8, 8, 4, 0, 1, 0),                    # k
                (1, 8, 8, 4, 3, 0, 1), (1, 8, 8, 4, 3, 4, 1), (1, 8, 8, 4, 5, 6, 2),                    # stride
                (1, 8, 8, 4, 3, 1, 2), (1, 8, 8, 4, 3, 1, -1), (1, 8, 8, 4, 5, 1, 3), (1, 8, 8, 4, 2, 1, 2),   # pad
                (1, 2, 8, 4, 5, 1, 1), (1, 8, 2, 4, 5, 1, 1), (1, 1, 1, 1, 2, 1, 0), (1, 4, 4, 1, 7, 1, 1),    # window
                (0, 8, 8, 4, 3, 1, 1), (1, 0, 8, 4, 3, 1, 1), (1, 8, 0, 4, 3, 1, 1), (1, 8, 8, 0, 3, 1, 1),    # empty
                (2 ** 31 // (720 * 1280) + 1, 720, 1280, 4, 3, 1, 1)):                                  # 32-bit pixel index
        assert q(*bad) == 0, bad
    assert q(2 ** 31 // (720 * 1280), 720, 1280, 4, 3, 1, 1) == 1
    for k in (3, 5):
        for levels in (1, 2, 3):
            for N, H, W, C in ((1, 1, 1, 1), (160, 76, 60, 64), (160, 38, 30, 128), (2, 3, 200, 7)):
                assert qs(N, H, W, C, k, levels) == 1
    for bad in ((1, 8, 8, 4, 4, 3), (1, 8, 8, 4, 2, 1), (1, 8, 8, 4, 7, 1), (1, 8, 8, 4, 1, 1),          # k
                (1, 8, 8, 4, 5, 4), (1, 8, 8, 4, 5, 0), (1, 8, 8, 4, 3, -1),                             # levels
                (0, 8, 8, 4, 5, 3), (1, 0, 8, 4, 5, 3), (1, 8, 8, 0, 5, 3),
                (2 ** 31 // (720 * 1280) + 1, 720, 1280, 4, 5, 3)):
        assert qs(*bad) == 0, bad


def test_python_asks_the_library_what_is_supported(hip_lib):
    from snn_for_object_detection_amd import functional as HF
    assert HF.pool_sets() == ((2, 3, 4, 5, 6, 7), (3, 5))
    assert HF.pool_covers(160, 76, 60, 64, 5, 1, 2) and not HF.pool_covers(160, 76, 60, 64, 5, 1, 3)
    assert HF.spp_covers(160, 76, 60, 64, 5, 3) and not HF.spp_covers(160, 76, 60, 64, 5, 4)


def _owned(n):
    t = torch.zeros(n, device="cuda" if torch.cuda.is_available() else "cpu")
    return t, t.data_ptr()


def _refused(lib, name, *args):
    rc = getattr(lib, name)(*args)
    msg = lib.snn_last_error().decode()
    assert rc == 1, (name, args, rc, msg)          # 1: refused on the host; 2 would be a failed launch
    return msg


def test_launchers_refuse_before_any_launch(hip_lib):
    keep, p = _owned(4096)
    big = 2 ** 31 // (720 * 1280) + 1
    #        kind x ldx y ldy N  H  W  C  k  s  pad stream
    fwd = [1, p, 4, p, 4, 1, 8, 8, 4, 5, 1, 2, None]
    for i, v, word in ((1, None, "null pointer"), (3, None, "null pointer"), (0, 3, "bad pool kind"), (0, -1, "bad pool kind"),
                       (11, 3, "pad <= k / 2"), (11, -1, "pad <= k / 2"), (9, 8, "k <= 7"), (9, 1, "2 <= k"),
                       (10, 6, "stride <= k"), (10, 0, "1 <= stride"), (2, 3, "below the 4 channels"),
                       (4, 3, "below the 4 channels"), (5, 0, "not covered"), (8, 0, "not covered")):
        a = list(fwd)
        a[i] = v
        assert word in _refused(hip_lib, "snn_pool2d_fwd", *a), (i, v)
    # a window larger than the padded image, in either direction
    assert "W + 2 pad >= k" in _refused(hip_lib, "snn_pool2d_fwd", 1, p, 4, p, 4, 1, 8, 3, 4, 7, 1, 1, None)
    assert "H + 2 pad >= k" in _refused(hip_lib, "snn_pool2d_fwd", 1, p, 4, p, 4, 1, 4, 8, 4, 7, 1, 1, None)
    assert "N * H * W < 2^31" in _refused(hip_lib, "snn_pool2d_fwd", 1, p, 4, p, 4, big, 720, 1280, 4, 3, 1, 1, None)
    #        kind x ldx gy ldgy add ldadd gx ldgx N  H  W  C  k  s  pad stream
    bwd = [1, p, 4, p, 4, None, 0, p + 1024, 4, 1, 8, 8, 4, 5, 1, 2, None]
    for i, v, word in ((1, None, "needs the forward input"), (3, None, "null pointer"), (7, None, "null pointer"),
                       (0, 3, "bad pool kind"), (15, 3, "pad <= k / 2"), (13, 8, "k <= 7"), (14, 6, "stride <= k"),
                       (2, 3, "below the 4 channels"), (4, 3, "below the 4 channels"), (8, 3, "below the 4 channels"),
                       (10, 0, "H + 2 pad >= k"), (9, 0, "not covered")):
        a = list(bwd)
        a[i] = v
        assert word in _refused(hip_lib, "snn_pool2d_bwd", *a), (i, v)
    a = list(bwd)
    a[10], a[13], a[15] = 4, 7, 1                                                      # 4 + 2 < 7: no window fits
    assert "H + 2 pad >= k" in _refused(hip_lib, "snn_pool2d_bwd", *a)
    a = list(bwd)
    a[5], a[6] = p + 2048, 3
    assert "below the 4 channels" in _refused(hip_lib, "snn_pool2d_bwd", *a)           # the addend's pixel stride
    a[5], a[6] = p + 1024, 4
    assert "must not alias" in _refused(hip_lib, "snn_pool2d_bwd", *a)
    a = list(bwd)
    a[9], a[10], a[11], a[13], a[15] = big, 720, 1280, 3, 1
    assert "N * H * W < 2^31" in _refused(hip_lib, "snn_pool2d_bwd", *a)
    #      x ldx y ldy N  H  W  C  k  levels stream
    spp = [p, 4, p + 1024, 16, 1, 8, 8, 4, 5, 3, None]
    for i, v, word in ((0, None, "null pointer"), (2, None, "null pointer"), (8, 4, "k in {3, 5}"), (8, 7, "k in {3, 5}"),
                       (9, 4, "levels in {1, 2, 3}"), (9, 0, "levels in {1, 2, 3}"), (1, 3, "below the 4 / 16 channels"),
                       (3, 15, "below the 4 / 16 channels"), (3, 4, "below the 4 / 16 channels"), (4, 0, "not covered"),
                       (7, 0, "not covered")):
        a = list(spp)
        a[i] = v
        assert word in _refused(hip_lib, "snn_spp_fwd", *a), (i, v)
    a = list(spp)
    a[4], a[5], a[6] = big, 720, 1280
    assert "N * H * W < 2^31" in _refused(hip_lib, "snn_spp_fwd", *a)
    del keep


def test_functional_refuses_by_name_before_any_launch(hip_lib):
    """The Python entry asks ``snn_pool2d_supported`` / ``snn_spp_supported`` first - but only for tensors on the device
    (there is no CPU path): on a CPU tensor the device check comes first."""
    from snn_for_object_detection_amd import functional as HF
    x = torch.zeros(1, 4, 8, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.pool2d(x, 1, 5, 1, 2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.spp(x)
