"""The layout, merge, conversion, activation, pooling, up-sampling kernels (csrc/elementwise.hip) and the small GEMM
(csrc/small_gemm.hip) per element against plain fp64 (tests/elementwise_ref.py), through the C ABI.  Every row

* names the kernel instances it exists for and asserts that the launcher's conditions select them, recomputed from the very
  pointers, strides and sizes it passes (``_merge_instance`` and friends mirror the launchers' branches);
  test_every_kernel_instance_is_named fails when the tables stop covering REQUIRED;
* writes into a NaN-filled slice of a wider buffer of SENT whose guard channels / guard elements must come back bit for bit;
* is checked per element - bit-exact where the operation moves data or the operands make every step exact, else against a
  derived bound stated on ``mag`` (the sum of the absolute terms of that element) - never by a norm over the tensor;
* proves that its check has teeth: the same comparison rejects the reference with one tap, one addend or one k term dropped,
  and a data-movement result with two elements swapped.

Bounds (U = 2^-24, the fp32 unit roundoff; derivations in DESIGN.md, "Per-element tests of the elementwise kernels"):
  merges            bit-equal to the fp32 CPU sum and |out - (a + b)| <= U |a + b|
  AVG / SUM forward (k k + 4) U mag        k k sequential additions, one division, at most two multiplications
  AVG / SUM bwd     (n + 2) U mag          n windows cover the pixel: n - 1 additions, <= 3 roundings per term
  up-sampling bwd   (s s) U mag
  small GEMM        (K + 2) U mag          K fmaf roundings; + U |c_old + acc| when accumulating
  activations       ACT_ULPS below (measured on the MI355X, doubled)
The ``-oversize`` rows launch more than 8 * CU * 256 work items (the CU count is read from the device) with a ragged second
trip of the grid-stride loop, and use the exact comparisons only.  Each row prints its largest error / bound (RATIO lines,
-s).  Tensors above 2^31 elements (the 64-bit index paths) stay untested by design: a few GB per row.
"""
import math

import pytest
import torch

from tests import elementwise_ref as R
from tests.fp64_buffers import BF16_ROUND, SENT, Buf, _exact_operands, _exact_weights, _random, _st

pytestmark = pytest.mark.gpu

U = R.U
NAN = float("nan")
BF = torch.bfloat16


@pytest.fixture(scope="module")
def H_(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    from snn_for_object_detection_amd import _hip
    return _hip


def _cap():
    """Work items one trip of a capped grid covers: 8 blocks per CU (snn_grid_for, csrc/snn_common.h) of 256 threads."""
    return 8 * torch.cuda.get_device_properties(0).multi_processor_count * 256


# ------------------------------------------------------------------------------------------ buffers and comparisons
class Flat:
    """n elements at element offset ``off`` behind PAD guard elements of a flat buffer of SENT (the allocation and
    PAD elements are 16-byte multiples, so ``off`` alone decides the alignment of ``ptr``)."""
    PAD = 8

    def __init__(self, n, off=0, values=None, fill=None, dtype=torch.float32):
        self.buf = torch.full((n + off + 2 * self.PAD,), SENT, dtype=dtype, device="cuda")
        self.lo, self.hi = self.PAD + off, self.PAD + off + n
        self.view = self.buf[self.lo:self.hi]
        if values is not None:
            self.view.copy_(values.reshape(-1))
        elif fill is not None:
            self.view.fill_(fill)
        self.ptr = self.view.data_ptr()
        self.before = self.buf.clone()

    def value(self, shape=None):
        v = self.view.double().cpu()
        return v if shape is None else v.reshape(shape)

    def guards_intact(self, whole=False):
        it = torch.int32 if self.buf.dtype == torch.float32 else torch.int16
        a, b = self.buf.view(it), self.before.view(it)
        if whole:
            return torch.equal(a, b)
        return torch.equal(a[:self.lo], b[:self.lo]) and torch.equal(a[self.hi:], b[self.hi:])


def _same(out, ref):
    """Equal as values per element, NaN matching NaN (fp64 CPU tensors holding fp32 / bf16 values)."""
    return out.shape == ref.shape and bool((((out != out) & (ref != ref)) | (out == ref)).all())


def _swapped(ref):
    """ref with two unequal elements swapped (None when all elements are equal)."""
    flat = ref.reshape(-1).clone()
    other = ((flat != flat[0]) & ~((flat != flat) & (flat[0] != flat[0]))).nonzero()
    if other.numel() == 0:
        return None
    j = int(other[0])
    flat[0], flat[j] = ref.reshape(-1)[j], ref.reshape(-1)[0]
    return flat.reshape(ref.shape)


def _exact(what, out, ref):
    assert _same(out, ref), f"{what}: {int((~(((out != out) & (ref != ref)) | (out == ref))).sum())} elements differ"
    wrong = _swapped(ref)
    if wrong is not None:
        assert not _same(out, wrong), f"{what}: the comparison does not notice two swapped elements"


def _within(out, ref, bound):
    """|out - ref| <= bound where ref is finite; the same value (NaN, +-inf) elsewhere."""
    fin = torch.isfinite(ref)
    ok = torch.where(fin, (out - ref).abs() <= bound, ((out != out) & (ref != ref)) | (out == ref))
    return bool(ok.all())


def _bounded(tag, out, ref, bound, wrong_refs=()):
    fin = torch.isfinite(ref)
    r = float(((out - ref).abs()[fin] / (bound[fin] + 1e-300)).max()) if bool(fin.any()) else 0.0
    print(f"RATIO {tag} {r:.4g}")
    assert _within(out, ref, bound), f"{tag}: largest error / bound {r:.4g}"
    for i, wrong in enumerate(wrong_refs):
        assert not _within(out, wrong, bound), f"{tag}: the bound does not reject perturbed reference {i}"


def _a(ptr, n=16):
    return ptr % n == 0


# ------------------------------------------------------------------------------------------ instances
OVERSIZE = {"k_nchw_to_nhwc_small", "k_weight_transpose", "k_channels<4>", "k_channels<1>", "k_add<4>", "k_add<1>",
            "k_merge_bf16<4>", "k_merge_bf16<1>", "k_convert_bf16", "k_act_fwd", "k_act_bwd", "k_pool_fwd", "k_pool_bwd",
            "k_upsample_fwd", "k_upsample_bwd"}
REQUIRED = {
    # snn_nchw_to_nhwc / snn_nhwc_to_nchw
    "copy_c1", "k_nchw_to_nhwc_small<2>", "k_nchw_to_nhwc_small<3>", "k_nchw_to_nhwc_small<4>", "k_transpose_cp:to_nhwc",
    "k_transpose_cp:to_nchw", "tile_full", "tile_partial", "tile_one_past",
    "k_weight_transpose", "k_weight_transpose_batched", "k_weight_transpose_batched:tiles>64",
    # channels_op, snn_add, the bf16 merges, the conversion
    "k_channels<4,copy>", "k_channels<1,copy>", "k_channels<4,add>", "k_channels<1,add>", "k_add<4>", "k_add<1>",
    "k_merge_bf16<4,copy>", "k_merge_bf16<1,copy>", "k_merge_bf16<4,add>", "k_merge_bf16<1,add>", "k_convert_bf16<to>",
    "k_convert_bf16<from>",
    "k_act_fwd", "k_act_bwd", "k_pool_fwd", "k_pool_bwd", "k_upsample_fwd", "k_upsample_bwd",
    "k_small_gemm<0,0>", "k_small_gemm<0,1>", "k_small_gemm<1,0>", "k_small_gemm<1,1>", "k_small_gemm_batched",
} | {f"{k}-oversize" for k in OVERSIZE}


def _layout_instances(fn, C, HW):
    """What snn_nchw_to_nhwc / snn_nhwc_to_nchw launch for C channels, and how the 32 x 32 LDS tiles are filled."""
    if fn == "snn_nchw_to_nhwc" and C <= 4:
        return {"copy_c1"} if C == 1 else {f"k_nchw_to_nhwc_small<{C}>"}
    got = {"k_transpose_cp:to_nhwc" if fn == "snn_nchw_to_nhwc" else "k_transpose_cp:to_nchw"}
    for n in (C, HW):
        got.add("tile_full" if n % 32 == 0 else "tile_one_past" if n % 32 == 1 and n > 32 else "tile_partial")
    return got


def _merge_instance(kernel, mode, C, lds, ptrs, nbytes):
    """The launchers' vector condition: C and every stride a multiple of 4 elements, every pointer on nbytes."""
    v4 = C % 4 == 0 and all(ld % 4 == 0 for ld in lds) and all(_a(p, nbytes) for p in ptrs)
    return f"{kernel}<{4 if v4 else 1}{',' + mode if mode else ''}>"


# ------------------------------------------------------------------------------------------ layout
LAYOUT_C = (1, 2, 3, 4, 5, 31, 32, 33, 65)
LAYOUT_HW = ((1, 1), (5, 7), (8, 8), (9, 11))           # H*W = 1, 35, 64, 99
LAYOUT_WANT = {
    "snn_nchw_to_nhwc": {"copy_c1", "k_nchw_to_nhwc_small<2>", "k_nchw_to_nhwc_small<3>", "k_nchw_to_nhwc_small<4>",
                         "k_transpose_cp:to_nhwc", "tile_full", "tile_partial", "tile_one_past"},
    "snn_nhwc_to_nchw": {"k_transpose_cp:to_nchw", "tile_full", "tile_partial", "tile_one_past"},
}


@pytest.mark.parametrize("fn", sorted(LAYOUT_WANT))
def test_layout_adapters_bit_exact(H_, fn):
    reached = set()
    for C in LAYOUT_C:
        for H, W in LAYOUT_HW:
            for N in (1, 3):
                reached |= _layout_instances(fn, C, H * W)
                x = _random((N, C, H, W), 100 * C + H + N)          # logical NCHW values
                src_v = x if fn == "snn_nchw_to_nhwc" else x.permute(0, 2, 3, 1)
                want = (x.permute(0, 2, 3, 1) if fn == "snn_nchw_to_nhwc" else x).contiguous().double().reshape(-1)
                src = Flat(x.numel(), values=src_v.contiguous())
                dst = Flat(x.numel(), fill=NAN)
                H_.call(fn, src.ptr, dst.ptr, N, C, H, W, _st())
                torch.cuda.synchronize()
                what = f"{fn} N{N} C{C} {H}x{W}"
                _exact(what, dst.value(), want)
                assert dst.guards_intact() and src.guards_intact(whole=True), what
    assert reached == LAYOUT_WANT[fn], reached ^ LAYOUT_WANT[fn]


WT_SHAPES = ((1, 1, 1), (33, 9, 5), (5, 9, 33), (64, 1, 32), (31, 49, 2), (130, 9, 36))     # (Cout, taps, Cin)
_KHKW = {1: (1, 1), 9: (3, 3), 49: (7, 7)}
WT_CLASSES = {"k_weight_transpose", "k_weight_transpose_batched", "k_weight_transpose_batched:tiles>64"}


def test_weight_transposes_match_permute_and_each_other(H_):
    ws = [_random(s, 7 + i) for i, s in enumerate(WT_SHAPES)]
    # one flat table: offsets that are no multiple of 4 floats, guard floats between the layers
    offs, end = [], 5
    for w in ws:
        off = end + 3
        off += 1 if off % 4 == 0 else 0
        offs.append(off)
        end = off + w.numel()
    total = end + 6
    assert all(o % 4 for o in offs)
    flat_w = torch.full((total,), SENT, device="cuda")
    flat_wt = torch.full((total,), SENT, device="cuda")
    for w, o in zip(ws, offs):
        flat_w[o:o + w.numel()] = w.reshape(-1).cuda()
        flat_wt[o:o + w.numel()] = NAN
    before_w, before_wt = flat_w.clone(), flat_wt.clone()
    table = torch.tensor([[o, *s] for o, s in zip(offs, WT_SHAPES)], dtype=torch.int64, device="cuda")
    tiles = [t * ((co + 31) // 32) * ((ci + 31) // 32) for co, t, ci in WT_SHAPES]
    assert max(tiles) > 64 and min(tiles) == 1           # the t += gridDim.x loop and its second barrier run / idle blocks
    H_.call("snn_weight_transpose_batched", flat_w.data_ptr(), flat_wt.data_ptr(), table.data_ptr(), len(ws), _st())
    torch.cuda.synchronize()
    written = torch.zeros(total, dtype=torch.bool)
    for w, o, (co, taps, ci) in zip(ws, offs, WT_SHAPES):
        want = w.permute(2, 1, 0).contiguous().double().reshape(-1)              # [Cin][taps][Cout]
        single = Flat(w.numel(), off=1, fill=NAN)
        src = Flat(w.numel(), off=3, values=w)
        H_.call("snn_weight_transpose", src.ptr, single.ptr, co, *_KHKW[taps], ci, _st())
        torch.cuda.synchronize()
        _exact(f"snn_weight_transpose {co, taps, ci}", single.value(), want)
        assert single.guards_intact() and src.guards_intact(whole=True)
        _exact(f"snn_weight_transpose_batched {co, taps, ci}", flat_wt[o:o + w.numel()].double().cpu(), want)
        written[o:o + w.numel()] = True
    keep = ~written.cuda()
    assert torch.equal(flat_wt.view(torch.int32)[keep], before_wt.view(torch.int32)[keep]), "floats between layers written"
    assert torch.equal(flat_w.view(torch.int32), before_w.view(torch.int32))


# ------------------------------------------------------------------------------------------ merges, fp32
# id, C, (ld, channel offset) of src / a, of b (snn_add only), of dst, the instance the row exists for.  Pointers: GUARD
# rows of ld floats lie in front of every slice, so (channel offset * 4) % 16 is the pointer's alignment.
CHANNEL_ROWS = [
    ("vector",       8, (12, 4), (16, 8), 4),
    ("C%4",          6, (12, 4), (16, 8), 1),
    ("src-stride%4", 8, (13, 0), (16, 8), 1),
    ("dst-stride%4", 8, (12, 4), (15, 4), 1),
    ("src-ptr%16",   8, (12, 1), (16, 8), 1),
    ("dst-ptr%16",   8, (12, 4), (16, 3), 1),
]
ADD_ROWS = [
    ("vector",       8, (12, 4), (20, 8), (16, 4), 4),
    ("C%4",          5, (12, 4), (20, 8), (16, 4), 1),
    ("a-stride%4",   8, (11, 0), (20, 8), (16, 4), 1),
    ("b-stride%4",   8, (12, 4), (21, 8), (16, 4), 1),
    ("dst-stride%4", 8, (12, 4), (20, 8), (18, 4), 1),
    ("a-ptr%16",     8, (12, 2), (20, 8), (16, 4), 1),
    ("b-ptr%16",     8, (12, 4), (20, 5), (16, 4), 1),
    ("dst-ptr%16",   8, (12, 4), (20, 8), (16, 7), 1),
]
MERGE_CLASSES = ({f"k_channels<{r[-1]},{m}>" for r in CHANNEL_ROWS for m in ("copy", "add")}
                 | {f"k_add<{r[-1]}>" for r in ADD_ROWS})


def _sum_checks(what, out, a, b):
    """out = a + b in fp32: bit-equal to the CPU's fp32 sum, within one rounding of the fp64 sum, and not a alone."""
    _exact(what, out, (a + b).double())
    exact = a.double() + b.double()
    _bounded(what, out, exact, U * exact.abs(), wrong_refs=(a.double(), b.double()))


@pytest.mark.parametrize("M", [1, 777])
@pytest.mark.parametrize("row", CHANNEL_ROWS, ids=[r[0] for r in CHANNEL_ROWS])
def test_copy_and_add_channels(H_, row, M):
    name, C, (lds, so), (ldd, do), width = row
    s, d0 = _random((1, 1, M, C), 31), _random((1, 1, M, C), 32)
    for fn, mode in (("snn_copy_channels", "copy"), ("snn_add_channels", "add")):
        S, D = Buf(s.shape, so, lds, values=s), Buf(s.shape, do, ldd, values=d0 if mode == "add" else None,
                                                    fill=None if mode == "add" else NAN)
        assert _merge_instance("k_channels", mode, C, (lds, ldd), (S.ptr, D.ptr), 16) == f"k_channels<{width},{mode}>", name
        H_.call(fn, S.ptr, lds, D.ptr, ldd, M, C, _st())
        torch.cuda.synchronize()
        what = f"{fn} {name} M{M}"
        if mode == "copy":
            _exact(what, D.value(), s.double())
        else:
            _sum_checks(what, D.value(), s, d0)
        assert D.guards_intact() and S.guards_intact(whole=True), what


# dst aliasing a / b: the destination then has no stride or pointer of its own, so the dst-* rows run unaliased only
ADD_CASES = [(r, al) for r in ADD_ROWS for al in (None, "a", "b") if not (al and r[0].startswith("dst-"))]


@pytest.mark.parametrize("M", [1, 777])
@pytest.mark.parametrize("row,alias", ADD_CASES, ids=[f"{r[0]}-alias_{al}" for r, al in ADD_CASES])
def test_add(H_, row, alias, M):
    name, C, (lda, ao), (ldb, bo), (ldd, do), width = row
    a, b = _random((1, 1, M, C), 41), _random((1, 1, M, C), 42)
    A, B = Buf(a.shape, ao, lda, values=a), Buf(a.shape, bo, ldb, values=b)
    D = {None: Buf(a.shape, do, ldd, fill=NAN), "a": A, "b": B}[alias]
    assert _merge_instance("k_add", "", C, (lda, ldb, D.ld), (A.ptr, B.ptr, D.ptr), 16) == f"k_add<{width}>", name
    H_.call("snn_add", A.ptr, lda, B.ptr, ldb, D.ptr, D.ld, M, C, _st())
    torch.cuda.synchronize()
    what = f"snn_add {name} alias={alias} M{M}"
    _sum_checks(what, D.value(), a, b)
    for X in (A, B, D):
        assert X.guards_intact(whole=X is not D), what


# ------------------------------------------------------------------------------------------ activations
# Largest error of each kernel against fp64 over R.act_inputs(), measured on the MI355X (gfx950, ROCm 7 device libm), in fp32
# ulps of max(|ref|, 2^-126) - the tanh gradient in ulps of |gy|, because 1 - y*y cancels - and the bound: twice the measured
# maximum rounded up to a whole ulp (room for another libm version).  ReLU is exact.  Before the kernels were corrected the
# same measurement gave 1.6e7 ulps for the SiLU forward at x = -90.5 (e^-x overflows: x / inf = -0 for a result of -4.5e-38),
# about 50 ulps for the SiLU gradient next to its root at x = -1.2785 (fp32 cancellation) and a ReLU that turned NaN into 0.
#                   measured  bound    where
ACT_ULPS = {
    ("silu", "fwd"): (1.723, 4),     # x = -1.1e-4
    ("silu", "bwd"): (1.337, 3),     # x = -92.125 (a subnormal result)
    ("tanh", "fwd"): (1.132, 3),     # x = -0.6845
    ("tanh", "bwd"): (1.242, 3),     # x = -3.5146
}
ACT_CODES = {"relu": R.ACT_RELU, "silu": R.ACT_SILU, "tanh": R.ACT_TANH}


def act_measure(H_, act, x, gy):
    """(forward, gradient) of the kernels on x, gy with their fp64 references and the ulps per element."""
    n = x.numel()
    X, G = Flat(n, off=1, values=x), Flat(n, off=2, values=gy)
    Y, GX = Flat(n, off=3, fill=NAN), Flat(n, off=1, fill=NAN)
    H_.call("snn_act_fwd", ACT_CODES[act], X.ptr, Y.ptr, n, _st())
    H_.call("snn_act_bwd", ACT_CODES[act], X.ptr, Y.ptr, G.ptr, GX.ptr, n, _st())
    torch.cuda.synchronize()
    assert Y.guards_intact() and GX.guards_intact() and X.guards_intact(whole=True) and G.guards_intact(whole=True)
    y, gx = Y.value(), GX.value()
    y_ref, _ = R.act_ref(ACT_CODES[act], x)
    g_ref, _ = R.act_grad_ref(ACT_CODES[act], x, gy)
    return y, y_ref, R.ulps(y, y_ref), gx, g_ref, R.ulps(gx, g_ref, scale=gy if act == "tanh" else None)


@pytest.mark.parametrize("act", ["relu", "silu", "tanh"])
def test_activations_per_element(H_, act):
    x = R.act_inputs()
    gy = torch.sign(_random(x.shape, 78)) * (0.25 + _random(x.shape, 77).abs())      # no |gy| near 0
    y, y_ref, uy, gx, g_ref, ug = act_measure(H_, act, x, gy)
    rows = (("fwd", y, y_ref, uy), ("bwd", gx, g_ref, ug))
    for what, out, ref, u in rows:
        i = int(u.argmax())
        print(f"RATIO act-{act}-{what} max_ulps={float(u.max()):.4g} at x={float(x[i])!r}")
    for what, out, ref, u in rows:
        i = int(u.argmax())
        assert torch.equal(out != out, ref != ref), f"{act} {what}: NaN where the reference has none, or the reverse"
        assert torch.equal(torch.isfinite(out), torch.isfinite(ref)), f"{act} {what}: non-finite elements differ"
        if act == "relu":
            assert _same(out, ref), f"relu {what} is not exact"
        else:
            bound = ACT_ULPS[(act, what)][1]
            assert float(u.max()) <= bound, f"{act} {what}: {float(u.max()):.4g} ulps at x={float(x[i])!r} > {bound}"
    # teeth: a forward that returned the input's neighbour value, a gradient without its gy
    assert not _same(y, R.act_ref(ACT_CODES[act], x + 0.5)[0])
    assert float(R.ulps(g_ref / gy.double(), g_ref, scale=gy if act == "tanh" else None).max()) > 8


# ------------------------------------------------------------------------------------------ pooling
#             k  s  H  W
POOL_GEOMS = [(1, 1, 4, 5), (2, 2, 5, 7), (2, 1, 4, 5), (3, 1, 5, 6), (3, 2, 6, 8), (2, 3, 6, 7), (4, 4, 4, 4)]
POOL_C = (1, 3, 6, 33)
POOL_KINDS = (("avg", R.POOL_AVG), ("max", R.POOL_MAX), ("sum", R.POOL_SUM))


def _pool_inputs(N, H, W, C, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randn((N, H, W, C), generator=g)
    spikes = (torch.rand((N, H, W, C), generator=g) < 0.4).float()
    const = torch.full((N, H, W, C), 0.75)
    bad = rnd.clone()
    bad[0, 0, 0, 0] = NAN                            # a corner: inside one window
    bad[0, H // 2, W // 2, :] = NAN                  # the middle: inside every overlapping window around it
    bad[-1, 1:, :, -1] = -math.inf                   # whole windows of -inf
    bad[-1, H - 1, W - 1, 0] = NAN                   # the ragged tail, outside every window (when there is one)
    bad[0, 1, 1, 0] = -math.inf
    return {"random": rnd, "spikes": spikes, "const": const, "nan-inf": bad}


def _pool_call(H_, kind, x, gy, k, stride):
    N, H, W, C = x.shape
    Ho, Wo = R.pool_out(H, k, stride), R.pool_out(W, k, stride)
    X, G = Buf(x.shape, values=x), Buf(gy.shape, values=gy)
    Y, GX = Buf(gy.shape, fill=NAN), Buf(x.shape, fill=NAN)
    H_.call("snn_pool_fwd", kind, X.ptr, Y.ptr, N, H, W, C, Ho, Wo, k, stride, _st())
    H_.call("snn_pool_bwd", kind, X.ptr, G.ptr, GX.ptr, N, H, W, C, Ho, Wo, k, stride, _st())
    torch.cuda.synchronize()
    assert Y.guards_intact() and GX.guards_intact() and X.guards_intact(whole=True) and G.guards_intact(whole=True)
    return Y.value(), GX.value()


def _drop_tap(kind, x, gy, k, stride):
    """The references with tap (0, 0) of every window left out: (forward, gradient)."""
    N, H, W, C = x.shape
    Ho, Wo = R.pool_out(H, k, stride), R.pool_out(W, k, stride)
    rs, cs = slice(0, (Ho - 1) * stride + 1, stride), slice(0, (Wo - 1) * stride + 1, stride)
    scale = 1.0 / (k * k) if kind == R.POOL_AVG else 1.0
    y = R.pool_fwd_ref(kind, x, k, stride)[0] - x.double()[:, rs, cs, :] * scale
    gx = R.pool_bwd_ref(kind, x, gy, k, stride)[0]
    gx[:, rs, cs, :] -= gy.double() * scale
    return y, gx


@pytest.mark.parametrize("k,stride,H,W", POOL_GEOMS, ids=[f"k{g[0]}s{g[1]}-{g[2]}x{g[3]}" for g in POOL_GEOMS])
def test_pooling_per_element(H_, k, stride, H, W):
    N = 2
    cover = R.pool_cover(H, W, k, stride)
    if (k, stride) in ((3, 2), (2, 3)):
        assert (H - k) % stride != 0 and bool((cover == 0).any())        # a ragged tail / pixels between windows
    ncov = cover.double().reshape(1, H, W, 1)
    for C in POOL_C:
        Ho, Wo = R.pool_out(H, k, stride), R.pool_out(W, k, stride)
        gy_int = _exact_operands((N, Ho, Wo, C), 5)
        gy_rnd = _random((N, Ho, Wo, C), 6)
        for name, x in _pool_inputs(N, H, W, C, 10 * k + stride).items():
            for kname, kind in POOL_KINDS:
                tag = f"pool-{kname}-k{k}s{stride}-{H}x{W}-C{C}-{name}"
                y_ref, y_mag = R.pool_fwd_ref(kind, x, k, stride)
                for gname, gy in (("int", gy_int), ("rnd", gy_rnd)):
                    y, gx = _pool_call(H_, kind, x, gy, k, stride)
                    g_ref, g_mag = R.pool_bwd_ref(kind, x, gy, k, stride)
                    assert bool((gx[:, cover == 0, :] == 0).all()), f"{tag}: gradient outside every window"
                    if kind == R.POOL_MAX:
                        _exact(tag + " fwd", y, y_ref)
                        if gname == "int":           # integer gradients: every partial sum is exact
                            _exact(tag + " bwd", gx, g_ref)
                        else:
                            _bounded(tag + " bwd", gx, g_ref, (ncov + 2) * U * g_mag)
                        continue
                    teeth = _drop_tap(kind, x, gy, k, stride) if name in ("random", "const") else (None, None)
                    _bounded(tag + " fwd", y, y_ref, (k * k + 4) * U * y_mag, wrong_refs=[t for t in teeth[:1] if t is not None])
                    if gname == "int" and kind == R.POOL_SUM and k in (1, 2, 4):
                        _exact(tag + " bwd", gx, g_ref)          # g * k * k / (k k) is exact for a power of two
                    _bounded(tag + f" bwd-{gname}", gx, g_ref, (ncov + 2) * U * g_mag,
                             wrong_refs=[t for t in teeth[1:] if t is not None])


# ------------------------------------------------------------------------------------------ up-sampling
@pytest.mark.parametrize("s", [1, 2, 3])
def test_upsampling_per_element(H_, s):
    N, H, W = 2, 3, 5
    for C in (1, 6, 33):
        x = _random((N, H, W, C), 50 + C)
        X, Y = Buf(x.shape, values=x), Buf((N, H * s, W * s, C), fill=NAN)
        H_.call("snn_upsample_fwd", X.ptr, Y.ptr, N, H, W, C, s, _st())
        torch.cuda.synchronize()
        _exact(f"upsample-fwd s{s} C{C}", Y.value(), R.upsample_fwd_ref(x, s)[0])
        assert Y.guards_intact() and X.guards_intact(whole=True)
        for gname, gy in (("int", _exact_operands(Y.shape, 8)), ("rnd", _random(Y.shape, 9))):
            G, GX = Buf(Y.shape, values=gy), Buf(x.shape, fill=NAN)
            H_.call("snn_upsample_bwd", G.ptr, GX.ptr, N, H, W, C, s, _st())
            torch.cuda.synchronize()
            ref, mag = R.upsample_bwd_ref(gy, s)
            if gname == "int":
                _exact(f"upsample-bwd s{s} C{C}", GX.value(), ref)
            wrong = ref - gy.double()[:, 0::s, 0::s, :]                 # tap (0, 0) dropped
            _bounded(f"upsample-bwd-{gname}-s{s}-C{C}", GX.value(), ref, s * s * U * mag, wrong_refs=(wrong,))
            assert GX.guards_intact() and G.guards_intact(whole=True)


# ------------------------------------------------------------------------------------------ small GEMM
GEMM_MNK = [(1, 1, 1), (31, 33, 127), (32, 32, 128), (33, 31, 129), (65, 65, 257), (1, 65, 128), (65, 1, 129), (32, 33, 1),
            (31, 32, 257), (33, 65, 127)]
GEMM_CLASSES = {f"k_small_gemm<{ta},{tb}>" for ta in (0, 1) for tb in (0, 1)}


def _mat(values, pad, off=1, fill=None):
    """[rows, cols] inside a guarded [GUARD + rows + GUARD, cols + pad] buffer, starting `off` floats into each row."""
    rows, cols = values.shape if values is not None else fill[1]
    return Buf((1, 1, rows, cols), off, cols + pad, values=values, fill=None if values is not None else fill[0])


def _gemm(H_, A, ta, B, tb, C, M, N, K, acc, Ct=None):
    for X, row in ((A, M if ta else K), (B, K if tb else N), (C, N)) + (((Ct, M),) if Ct is not None else ()):
        assert X.ld > row                                    # every leading dimension larger than its row
    H_.call("snn_small_gemm", A.ptr, A.ld, ta, B.ptr, B.ld, tb, C.ptr, C.ld, M, N, K, acc, Ct.ptr if Ct is not None else None,
            Ct.ld if Ct is not None else 0, _st())
    torch.cuda.synchronize()
    assert A.guards_intact(whole=True) and B.guards_intact(whole=True) and C.guards_intact()
    assert Ct is None or Ct.guards_intact()


@pytest.mark.parametrize("M,N,K", GEMM_MNK, ids=[f"{m}x{n}x{k}" for m, n, k in GEMM_MNK])
def test_small_gemm_per_element(H_, M, N, K):
    assert {v for r in GEMM_MNK for v in r[:2]} == {1, 31, 32, 33, 65} and {r[2] for r in GEMM_MNK} == {1, 127, 128, 129, 257}
    for exact in (False, True):
        a = _exact_operands((M, K), 3) if exact else _random((M, K), 3)
        b = _exact_weights((K, N), 4) if exact else _random((K, N), 4)
        c_old = _exact_operands((M, N), 5) if exact else _random((M, N), 5)
        ref, mag = R.small_gemm_ref(a, 0, b, 0)
        wrong = ref - a.double()[:, K // 2:K // 2 + 1] * b.double()[K // 2:K // 2 + 1, :]       # one k term dropped
        for ta in (0, 1):
            for tb in (0, 1):
                tag = f"gemm-{M}x{N}x{K}-{'T' if ta else 'N'}{'T' if tb else 'N'}-{'exact' if exact else 'rnd'}"
                assert f"k_small_gemm<{ta},{tb}>" in GEMM_CLASSES          # the launcher branches on the two flags alone
                A = _mat(a.t().contiguous() if ta else a, 3)
                B = _mat(b.t().contiguous() if tb else b, 5, off=2)
                C, Ct = _mat(None, 1, fill=(NAN, (M, N))), _mat(None, 4, off=3, fill=(NAN, (N, M)))
                _gemm(H_, A, ta, B, tb, C, M, N, K, 0, Ct)
                c = C.value().reshape(M, N)
                if exact:
                    _exact(tag, c, ref)
                else:
                    _bounded(tag, c, ref, (K + 2) * U * mag, wrong_refs=(wrong,))
                _exact(tag + " Ct", Ct.value().reshape(N, M), c.t())
                # the transposed product's launch: B^T A^T, the same fmaf chains
                C2 = _mat(None, 4, off=2, fill=(NAN, (N, M)))
                _gemm(H_, B, 1 - tb, A, 1 - ta, C2, N, M, K, 0)
                _exact(tag + " transposed launch", C2.value().reshape(N, M), c.t())
                # without Ct, then accumulated onto c_old
                C3, C4 = _mat(None, 1, fill=(NAN, (M, N))), _mat(c_old, 6, off=1)
                _gemm(H_, A, ta, B, tb, C3, M, N, K, 0)
                _exact(tag + " no Ct", C3.value().reshape(M, N), c)
                _gemm(H_, A, ta, B, tb, C4, M, N, K, 1)
                c4, tot = C4.value().reshape(M, N), c_old.double() + ref
                _exact(tag + " accumulate", c4, (c_old + c.float()).double())      # one fp32 addition onto the product
                if exact:
                    _exact(tag + " accumulate fp64", c4, tot)
                else:
                    bound = (K + 2) * U * mag
                    _bounded(tag + " acc", c4, tot, bound + U * (tot.abs() + bound), wrong_refs=(c_old.double() + wrong,))


def test_small_gemm_batched(H_):
    #         M   N   K  ldct (0 = M)
    prods = [(5, 7, 3, 0), (33, 65, 129, 35), (64, 32, 128, 0), (12, 40, 20, 33), (21, 40, 20, 33)]
    tiles = [((m + 31) // 32) * ((n + 31) // 32) for m, n, _, _ in prods]
    max_tiles = max(tiles) + 1
    assert min(tiles) == 1 and max_tiles > 6                  # the smallest product's surplus blocks leave early
    sizes = {"a": [m * k for m, n, k, _ in prods], "b": [k * n for m, n, k, _ in prods], "c": [m * n for m, n, k, _ in prods]}
    offs, totals = {}, {}
    for key, sz in sizes.items():
        offs[key], end = [], 2
        for n in sz:
            o = end + 3
            o += 1 if o % 4 == 0 else 0
            offs[key].append(o)
            end = o + n
        totals[key] = end + 5
    # transposed copies: products 3 and 4 write column blocks 0..12 and 12..33 of ONE [40][33] matrix
    ct_sizes = [7 * 5, (65 - 1) * 35 + 33, 32 * 64, 40 * 33, None]
    ct_offs, end = [], 3
    for n in ct_sizes[:4]:
        o = end + 2
        o += 1 if o % 4 == 0 else 0
        ct_offs.append(o)
        end = o + n
    ct_offs.append(ct_offs[3] + 12)
    total_ct = end + 7
    assert all(o % 4 for k in offs for o in offs[k]) and all(o % 4 for o in ct_offs[:4])
    a = [_random((m, k), 20 + i) for i, (m, n, k, _) in enumerate(prods)]
    b = [_random((k, n), 30 + i) for i, (m, n, k, _) in enumerate(prods)]
    base = {k: torch.full((totals[k],), SENT, device="cuda") for k in "abc"}
    for i in range(len(prods)):
        base["a"][offs["a"][i]:offs["a"][i] + sizes["a"][i]] = a[i].reshape(-1).cuda()
        base["b"][offs["b"][i]:offs["b"][i] + sizes["b"][i]] = b[i].reshape(-1).cuda()
    table = torch.tensor([[offs["a"][i], offs["b"][i], offs["c"][i], ct_offs[i], *prods[i]] for i in range(len(prods))],
                         dtype=torch.int64, device="cuda")
    singles = []
    for i, (m, n, k, _) in enumerate(prods):
        A, B, C = _mat(a[i], 1), _mat(b[i], 2), _mat(None, 3, fill=(NAN, (m, n)))
        _gemm(H_, A, 0, B, 0, C, m, n, k, 0)
        singles.append(C.value().reshape(m, n))
        ref, mag = R.small_gemm_ref(a[i], 0, b[i], 0)
        wrong = ref - a[i].double()[:, :1] * b[i].double()[:1, :]
        _bounded(f"gemm-batched-single-{i}", singles[-1], ref, (k + 2) * U * mag, wrong_refs=(wrong,))
    for with_ct in (True, False):
        cbuf = base["c"].clone()
        ctbuf = torch.full((total_ct,), SENT, device="cuda")
        before_a, before_b, before_c, before_ct = base["a"].clone(), base["b"].clone(), cbuf.clone(), ctbuf.clone()
        H_.call("snn_small_gemm_batched", base["a"].data_ptr(), base["b"].data_ptr(), cbuf.data_ptr(),
                ctbuf.data_ptr() if with_ct else None, table.data_ptr(), len(prods), max_tiles, _st())
        torch.cuda.synchronize()
        wrote_c = torch.zeros(totals["c"], dtype=torch.bool)
        wrote_ct = torch.zeros(total_ct, dtype=torch.bool)
        for i, (m, n, k, ldct) in enumerate(prods):
            o = offs["c"][i]
            _exact(f"gemm-batched-{i}", cbuf[o:o + m * n].double().cpu().reshape(m, n), singles[i])   # (and so within the bound)
            wrote_c[o:o + m * n] = True
            if with_ct:
                ld = ldct or m
                idx = ct_offs[i] + torch.arange(n).reshape(n, 1) * ld + torch.arange(m).reshape(1, m)
                _exact(f"gemm-batched-{i} Ct", ctbuf.cpu()[idx].double(), singles[i].t())
                wrote_ct[idx.reshape(-1)] = True
        for buf, before, wrote in ((cbuf, before_c, wrote_c), (ctbuf, before_ct, wrote_ct if with_ct else torch.zeros_like(wrote_ct))):
            keep = ~wrote.cuda()
            assert torch.equal(buf.view(torch.int32)[keep], before.view(torch.int32)[keep]), "floats between products written"
        assert torch.equal(base["a"], before_a) and torch.equal(base["b"], before_b)
    # the two column blocks tile the shared matrix exactly: 12 + 21 = 33 = ldct
    assert prods[3][0] + prods[4][0] == prods[3][3] == prods[4][3]


# ------------------------------------------------------------------------------------------ over-size rows
def _ragged(total):
    cap = _cap()
    assert cap < total < 2 * cap, (total, cap)      # a second, partial trip of the grid-stride loop
    return total


OVERSIZE_ROWS = ["k_nchw_to_nhwc_small", "k_weight_transpose", "k_channels<4>", "k_channels<1>", "k_add<4>", "k_add<1>",
                 "k_merge_bf16<4>", "k_merge_bf16<1>", "k_convert_bf16", "k_act", "k_pool", "k_upsample"]
OVERSIZE_CLASSES = {f"{k}-oversize" for k in OVERSIZE}
# asserted inside the over-size rows (the bf16 merges and the conversion have their small rows in test_gpu_bf16_storage.py)
BF16_CLASSES = {"k_merge_bf16<4,copy>", "k_merge_bf16<1,copy>", "k_merge_bf16<4,add>", "k_merge_bf16<1,add>",
                "k_convert_bf16<to>", "k_convert_bf16<from>"}
# launchers with one kernel and no branch: every call of the entry point reaches it
SINGLE_BRANCH = {"k_act_fwd", "k_act_bwd", "k_pool_fwd", "k_pool_bwd", "k_upsample_fwd", "k_upsample_bwd",
                 "k_small_gemm_batched"}


@pytest.mark.parametrize("row", OVERSIZE_ROWS)
def test_oversize_rows(H_, row):
    cap = _cap()
    if row == "k_nchw_to_nhwc_small":
        N, C = 3, 3
        H = W = math.isqrt(cap // N) + 2
        _ragged(N * H * W)                                       # one thread per pixel
        x = _random((N, C, H, W), 1)
        src, dst = Flat(x.numel(), values=x), Flat(x.numel(), fill=NAN)
        assert _layout_instances("snn_nchw_to_nhwc", C, H * W) == {"k_nchw_to_nhwc_small<3>"}
        H_.call("snn_nchw_to_nhwc", src.ptr, dst.ptr, N, C, H, W, _st())
        torch.cuda.synchronize()
        _exact(row, dst.value(), x.permute(0, 2, 3, 1).contiguous().double().reshape(-1))
        assert dst.guards_intact()
    elif row == "k_weight_transpose":
        co, taps = 257, 9
        ci = cap // (co * taps) + 2
        _ragged(co * taps * ci)
        w = _random((co, taps, ci), 2)
        src, dst = Flat(w.numel(), values=w), Flat(w.numel(), off=1, fill=NAN)
        H_.call("snn_weight_transpose", src.ptr, dst.ptr, co, 3, 3, ci, _st())
        torch.cuda.synchronize()
        _exact(row, dst.value(), w.permute(2, 1, 0).contiguous().double().reshape(-1))
        assert dst.guards_intact()
    elif row.startswith(("k_channels", "k_add", "k_merge_bf16")):
        width = int(row[-2])
        C = 4 if width == 4 else 3
        M = _ragged(cap + 1237) if width == 4 else cap // 3 + 411
        _ragged(M * (C // width))
        bf = row.startswith("k_merge_bf16")
        dt, nbytes = (BF, 8) if bf else (torch.float32, 16)
        a, b = _random((1, 1, M, C), 3).to(dt), _random((1, 1, M, C), 4).to(dt)
        ld = C + (4 if width == 4 else 2)
        A, B = Buf(a.shape, 0, ld, values=a, dtype=dt), Buf(a.shape, 0, ld, values=b, dtype=dt)
        want = (a.float() + b.float()).to(dt).double()
        if row.startswith("k_channels"):
            for fn, mode in (("snn_copy_channels", "copy"), ("snn_add_channels", "add")):
                D = Buf(a.shape, 0, ld, values=b)
                assert _merge_instance("k_channels", mode, C, (ld, ld), (A.ptr, D.ptr), 16) == f"k_channels<{width},{mode}>"
                H_.call(fn, A.ptr, ld, D.ptr, ld, M, C, _st())
                torch.cuda.synchronize()
                _exact(f"{row} {mode}", D.value(), a.double() if mode == "copy" else want)
                assert D.guards_intact()
        else:
            D = Buf(a.shape, 0, ld, fill=NAN, dtype=dt)
            kern = "k_merge_bf16" if bf else "k_add"
            assert _merge_instance(kern, "add" if bf else "", C, (ld, ld, ld), (A.ptr, B.ptr, D.ptr), nbytes) == \
                (f"k_merge_bf16<{width},add>" if bf else f"k_add<{width}>")
            H_.call("snn_add_bf16" if bf else "snn_add", A.ptr, ld, B.ptr, ld, D.ptr, ld, M, C, _st())
            torch.cuda.synchronize()
            _exact(row, D.value(), want)
            assert D.guards_intact()
            if bf:
                D = Buf(a.shape, 0, ld, fill=NAN, dtype=dt)
                assert _merge_instance(kern, "copy", C, (ld, ld), (A.ptr, D.ptr), nbytes) == f"k_merge_bf16<{width},copy>"
                H_.call("snn_copy_channels_bf16", A.ptr, ld, D.ptr, ld, M, C, _st())
                torch.cuda.synchronize()
                _exact(row + " copy", D.value(), a.double())
                assert D.guards_intact()
    elif row == "k_convert_bf16":
        n = _ragged(cap + 1234)
        x = _random((n,), 5) * 3
        x[:4] = torch.tensor([math.inf, 1e-40, NAN, -0.0])
        X, Y = Flat(n, off=1, values=x), Flat(n, off=1, fill=NAN, dtype=BF)
        H_.call("snn_convert_bf16", X.ptr, Y.ptr, n, 1, _st())
        torch.cuda.synchronize()
        _exact(row + " to", Y.value(), x.to(BF).double())
        Z = Flat(n, off=3, fill=NAN)
        H_.call("snn_convert_bf16", Y.ptr, Z.ptr, n, 0, _st())
        torch.cuda.synchronize()
        _exact(row + " from", Z.value(), x.to(BF).double())
        assert Y.guards_intact() and Z.guards_intact()
    elif row == "k_act":
        n = _ragged(cap + 777)
        x, gy = _random((n,), 6), _exact_operands((n,), 7)
        y, y_ref, _, gx, g_ref, _ = act_measure(H_, "relu", x, gy)
        _exact(row + " fwd", y, y_ref)
        _exact(row + " bwd", gx, g_ref)
    elif row == "k_pool":
        N, C, k, stride = 2, 6, 2, 2
        Ho = math.isqrt(cap // (N * C)) + 2
        H = W = Ho * stride + 1                                   # a ragged tail of one row and one column
        _ragged(N * Ho * Ho * C)
        assert N * H * W * C > cap
        x = (torch.rand((N, H, W, C), generator=torch.Generator().manual_seed(8)) < 0.4).float()
        gy = _exact_operands((N, Ho, Ho, C), 9)
        y, gx = _pool_call(H_, R.POOL_MAX, x, gy, k, stride)
        _exact(row + " fwd", y, R.pool_fwd_ref(R.POOL_MAX, x, k, stride)[0])
        _exact(row + " bwd", gx, R.pool_bwd_ref(R.POOL_MAX, x, gy, k, stride)[0])
    else:
        N, C, s = 2, 3, 2
        H = W = math.isqrt(cap // (N * C)) + 2
        _ragged(N * H * W * C)
        x, gy = _random((N, H, W, C), 10), _exact_operands((N, H * s, W * s, C), 11)
        X, Y = Buf(x.shape, values=x), Buf(gy.shape, fill=NAN)
        G, GX = Buf(gy.shape, values=gy), Buf(x.shape, fill=NAN)
        H_.call("snn_upsample_fwd", X.ptr, Y.ptr, N, H, W, C, s, _st())
        H_.call("snn_upsample_bwd", G.ptr, GX.ptr, N, H, W, C, s, _st())
        torch.cuda.synchronize()
        _exact(row + " fwd", Y.value(), R.upsample_fwd_ref(x, s)[0])
        _exact(row + " bwd", GX.value(), R.upsample_bwd_ref(gy, s)[0])
        assert Y.guards_intact() and GX.guards_intact()


# ------------------------------------------------------------------------------------------ the autograd layer
def _nhwc64(t):
    """logical [..., C, H, W] device tensor -> fp64 CPU [N, H, W, C]."""
    t = t.detach().float().cpu().double()
    t = t.reshape(-1, *t.shape[-3:])
    return t.permute(0, 2, 3, 1).contiguous()


def _layouts(shape5, seed):
    """name -> (leaf tensor that receives the gradient, the logical [T,B,C,H,W] / [B,C,H,W] operand built from it)."""
    T, B, C, H, W = shape5
    v = _random((T, B, H, W, C), seed)                     # channels-last values
    out = {}
    leaf = v[0].cuda().permute(0, 3, 1, 2).requires_grad_()
    out["single-step"] = (leaf, leaf, v[0:1])
    leaf = v.permute(0, 1, 4, 2, 3).contiguous().cuda().requires_grad_()
    assert leaf.is_contiguous()
    out["nchw"] = (leaf, leaf, v)
    wide = torch.full((T, B, H, W, C + 7), SENT, device="cuda")
    wide[..., 3:3 + C] = v.cuda()
    leaf = wide.permute(0, 1, 4, 2, 3).requires_grad_()
    out["channel-slice"] = (leaf, leaf.narrow(2, 3, C), v)
    vb = v.to(BF)
    leaf = vb.cuda().permute(0, 1, 4, 2, 3).requires_grad_()
    out["bf16"] = (leaf, leaf, vb.float())
    return out


def _leaf_grad(name, leaf, C):
    g = leaf.grad
    if name == "channel-slice":
        rest = torch.cat([g[:, :, :3], g[:, :, 3 + C:]], dim=2)
        assert bool((rest == 0).all()), "gradient outside the channel slice"
        g = g[:, :, 3:3 + C]
    return _nhwc64(g)


AUTOGRAD_OPS = ["pool-max-k3s2", "pool-avg-k2s1", "pool-sum-k2s2", "upsample-s2", "act-relu", "act-silu", "act-tanh"]


@pytest.mark.parametrize("op", AUTOGRAD_OPS)
def test_autograd_layer_on_every_accepted_layout(H_, op):
    from snn_for_object_detection_amd import functional as HF
    T, B, C, H, W = 2, 2, 5, 7, 6
    for name, (leaf, x, v) in _layouts((T, B, C, H, W), 3).items():
        xv = v.reshape(-1, H, W, C)                                        # what the operator sees, [N,H,W,C] fp32
        bf = name == "bf16"
        if op.startswith("pool"):
            kind = {"max": R.POOL_MAX, "avg": R.POOL_AVG, "sum": R.POOL_SUM}[op[5:8]]
            k, s = int(op[10]), int(op[12])
            y = HF.pool2d(x, kind, k, s)
            y_ref, y_mag = R.pool_fwd_ref(kind, xv, k, s)
        elif op.startswith("upsample"):
            y = HF.upsample_nearest(x, 2)
            y_ref, y_mag = R.upsample_fwd_ref(xv, 2)
        else:
            y = HF.activation(x, ACT_CODES[op[4:]])
            y_ref, y_mag = R.act_ref(ACT_CODES[op[4:]], xv)
        assert y.dim() == x.dim() and y.dtype == x.dtype
        gy = _exact_operands(tuple(y_ref.shape), 12) + 0.5      # [N,Ho,Wo,C]; never 0, exact in bf16, every sum of them exact
        gy_dev = gy.reshape(*y.shape[:-3], *gy.shape[1:]).cuda()
        gy_dev = gy_dev.permute(*range(gy_dev.dim() - 3), -1, -3, -2).to(y.dtype)
        y.backward(gy_dev)
        torch.cuda.synchronize()
        gx = _leaf_grad(name, leaf, C)
        if op.startswith("pool"):
            g_ref, g_mag = R.pool_bwd_ref(kind, xv, gy, k, s)
            n = R.pool_cover(H, W, k, s).double().reshape(1, H, W, 1)
            fb, gb = (k * k + 4) * U * y_mag, (n + 2) * U * g_mag
            if kind == R.POOL_MAX:
                fb, gb = 0 * y_mag, 0 * g_mag
        elif op.startswith("upsample"):
            g_ref, g_mag = R.upsample_bwd_ref(gy, 2)
            fb, gb = 0 * y_mag, 0 * g_mag                                  # integer + 0.5 gradients: exact sums
        else:
            g_ref, g_mag = R.act_grad_ref(ACT_CODES[op[4:]], xv, gy)
            if op == "act-relu":
                fb, gb = 0 * y_mag, 0 * g_mag
            else:                                                          # ACT_ULPS ulps: one ulp is at most 2^-23 relative
                fb = ACT_ULPS[(op[4:], "fwd")][1] * 2 * U * y_mag
                gb = ACT_ULPS[(op[4:], "bwd")][1] * 2 * U * (gy.double().abs() if op == "act-tanh" else g_mag)
        if bf:      # one bf16 rounding of the stored result (of the fp32 value, itself within the bound)
            fb, gb = fb + BF16_ROUND * (y_ref.abs() + fb), gb + BF16_ROUND * (g_ref.abs() + gb)
        tag = f"autograd-{op}-{name}"
        _bounded(tag + " fwd", _nhwc64(y), y_ref, fb)
        _bounded(tag + " bwd", gx, g_ref, gb)
        # teeth: the same bounds reject the forward of another operand and a gradient routed one pixel to the side
        assert not _within(_nhwc64(y), torch.roll(y_ref, 1, 2), fb) and not _within(gx, torch.roll(g_ref, 1, 2), gb), tag


def test_sum_and_concat_through_the_merge_kernels(H_):
    from snn_for_object_detection_amd import functional as HF
    T, B, H, W = 2, 2, 3, 5
    widths = (3, 5, 8)
    # Dense merge: slices of the 16-channel result start at channels 0, 3 (scalar kernel) and 8 (16-byte kernel)
    xs = [_random((T, B, H, W, c), 60 + c).cuda().permute(0, 1, 4, 2, 3).requires_grad_() for c in widths]
    out = HF.concat_channels(xs)
    want = torch.cat([x.detach() for x in xs], dim=2)
    offs = (0, 3, 8)
    ld = HF.cl_stride(out)
    assert ld == 16
    for c, o in zip(widths, offs):
        dst = out.narrow(2, o, c)
        inst = _merge_instance("k_channels", "copy", c, (c, ld), (xs[offs.index(o)].data_ptr(), dst.data_ptr()), 16)
        assert inst == ("k_channels<4,copy>" if o == 8 else "k_channels<1,copy>"), (c, o, inst)
    _exact("concat_channels", _nhwc64(out), _nhwc64(want))
    g = _random((T, B, H, W, 16), 70).cuda().permute(0, 1, 4, 2, 3)
    out.backward(g)
    for x, c, o in zip(xs, widths, offs):
        _exact(f"concat gradient {o}", _nhwc64(x.grad), _nhwc64(g.narrow(2, o, c)))
    # Residual merge of three addends: out = a + b, then the in-place out = out + c
    for c in widths:
        xs = [_random((T, B, H, W, c), 80 + i).cuda().permute(0, 1, 4, 2, 3).requires_grad_() for i in range(3)]
        out = HF.sum_tensors(xs)
        inst = _merge_instance("k_add", "", c, (c, c, c), tuple(x.data_ptr() for x in xs[:2]) + (out.data_ptr(),), 16)
        assert inst == ("k_add<4>" if c == 8 else "k_add<1>")
        cpu = [x.detach().cpu() for x in xs]
        _exact(f"sum_tensors C{c}", _nhwc64(out), _nhwc64((cpu[0] + cpu[1]) + cpu[2]))
        exact = sum(t.double() for t in cpu)
        _bounded(f"sum_tensors-C{c}", _nhwc64(out), _nhwc64(exact), 2 * U * _nhwc64(sum(t.double().abs() for t in cpu)),
                 wrong_refs=(_nhwc64(cpu[0].double() + cpu[1].double()),))
        g = _random((T, B, H, W, c), 90).cuda().permute(0, 1, 4, 2, 3)
        out.backward(g)
        for x in xs:
            _exact(f"sum gradient C{c}", _nhwc64(x.grad), _nhwc64(g))


# ------------------------------------------------------------------------------------------ coverage of the tables
def test_every_kernel_instance_is_named():
    """The instances the tables above declare (each row asserts its own from the pointers and strides it passes) cover every
    launcher branch of elementwise.hip and small_gemm.hip and every over-size row."""
    declared = (set().union(*LAYOUT_WANT.values()) | WT_CLASSES | MERGE_CLASSES | GEMM_CLASSES | OVERSIZE_CLASSES
                | BF16_CLASSES | SINGLE_BRANCH)
    assert REQUIRED <= declared, REQUIRED - declared
    covered = set()
    for row in OVERSIZE_ROWS:
        covered |= {k for k in OVERSIZE if k == row or k.startswith(row + "_")}
    assert covered == OVERSIZE, OVERSIZE - covered
