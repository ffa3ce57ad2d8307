"""The padded pooling kernels and the fused SPP forward (csrc/pool.hip) kernel by kernel against tests/pool_ref.py, at the
smallest shapes that can go wrong: 4 frames of distinct content (a halo that reaches into a neighbouring frame shows),
frames from 1x1 up to 37x70 (more than one backward tile of 8x8, more than one SPP row chunk and column tile of 64 lanes,
every last tile ragged), channel counts on both sides of the 4-channel lane, and every operand dense, as a channel slice at
a 4-aligned offset (the 16-byte path) and as a slice at an odd offset (the scalar path).

Agreement asked for: MAX forward and backward, and everything SPP: bit equality.  AVG / SUM: ``(k*k + 2) * 2^-24 * mag``
(k*k sequential additions plus the division / the two multiplications; the backward adds at most k*k terms, each rounded
once or three times, to an addend), and equality wherever every operation is exact.  pad = 0: the bits of the unpadded
entry points."""
import pytest
import torch

from tests import pool_ref as R

pytestmark = pytest.mark.gpu

SENT = -777.25
N = 4
SHAPES = [(1, 1), (1, 3), (2, 7), (5, 5), (13, 9), (37, 70)]
CHANNELS = [1, 3, 4, 6, 8, 36]
LAYOUTS = ["dense", "vec4", "odd"]
KSP = [(2, 2, 0), (3, 2, 1), (5, 1, 2), (3, 1, 1), (4, 3, 1), (7, 1, 3), (5, 2, 0)]
KSP_IDS = [f"k{k}s{s}p{p}" for k, s, p in KSP]
KINDS = {"avg": R.POOL_AVG, "max": R.POOL_MAX, "sum": R.POOL_SUM}


@pytest.fixture(scope="module")
def H_(hip_lib):
    from snn_for_object_detection_amd import _hip
    assert torch.cuda.is_available()
    return _hip


def _st():
    return torch.cuda.current_stream().cuda_stream


def _layout(C, layout):
    """(channel offset, pixel stride) of a C-channel operand"""
    return {"dense": (0, C), "vec4": (4, (C + 3) // 4 * 4 + 8), "odd": (3, C + 5)}[layout]


class Op:
    """An operand [N,H,W,C] inside a sentinel-filled buffer [N,H,W,ld]."""

    def __init__(self, shape, layout, value=None):
        n, h, w, c = shape
        self.C = c
        self.off, self.ld = _layout(c, layout)
        self.buf = torch.full((n, h, w, self.ld), SENT, device="cuda")
        if value is not None:
            self.buf[..., self.off:self.off + c] = value.float().cuda()
        self.ptr = self.buf.data_ptr() + 4 * self.off

    def value(self):
        return self.buf[..., self.off:self.off + self.C].cpu()

    def untouched(self):
        rest = torch.cat([self.buf[..., :self.off], self.buf[..., self.off + self.C:]], dim=-1)
        return bool((rest == SENT).all())


def _combos(k, p, more=()):
    """(H, W, C, layout, index): every shape the window fits x every channel count, the layout rotating so that every
    channel count meets every layout"""
    i = 0
    for a, (H, W) in enumerate(SHAPES + list(more)):
        if H + 2 * p < k or W + 2 * p < k:
            continue
        for b, C in enumerate(CHANNELS):
            yield H, W, C, LAYOUTS[(a + b) % 3], i
            i += 1


def _int_grad(shape, seed):
    return torch.randint(-4, 5, shape, generator=torch.Generator().manual_seed(seed)).float()


def _fwd(H_, kind, X, Y, H, W, C, k, s, p):
    H_.call("snn_pool2d_fwd", kind, X.ptr, X.ld, Y.ptr, Y.ld, N, H, W, C, k, s, p, _st())


def _bwd(H_, kind, X, G, A, GX, H, W, C, k, s, p):
    H_.call("snn_pool2d_bwd", kind, X.ptr if X is not None else None, X.ld if X is not None else 0, G.ptr, G.ld,
            A.ptr if A is not None else None, A.ld if A is not None else 0, GX.ptr, GX.ld, N, H, W, C, k, s, p, _st())


# ------------------------------------------------------------------------------------------ MAX
@pytest.mark.parametrize("k,s,p", KSP, ids=KSP_IDS)
def test_max_forward_bits(H_, k, s, p):
    for H, W, C, layout, i in _combos(k, p):
        kind = ["binary", "normal", "nan", "inf"][i % 4]          # "inf": +-inf and a frame of all -inf windows
        x = R.inputs(kind, (N, H, W, C), seed=100 + i)
        Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
        X, Y = Op(x.shape, layout, x), Op((N, Ho, Wo, C), LAYOUTS[(i + 1) % 3])
        _fwd(H_, R.POOL_MAX, X, Y, H, W, C, k, s, p)
        ref, _ = R.pool2d_fwd_ref(R.POOL_MAX, x, k, s, p)
        assert R.same_bits(Y.value(), ref), (H, W, C, layout, kind)
        assert Y.untouched() and R.same_bits(X.buf, Op(x.shape, layout, x).buf)     # (the input is only read)


@pytest.mark.parametrize("k,s,p", KSP, ids=KSP_IDS)
def test_max_backward_bits(H_, k, s, p):
    for H, W, C, layout, i in _combos(k, p):
        x = R.inputs("binary", (N, H, W, C), seed=200 + i)      # ties everywhere: the first maximum must be the one
        Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
        g, add = _int_grad((N, Ho, Wo, C), 300 + i), _int_grad(x.shape, 400 + i)
        X, G, A = Op(x.shape, layout, x), Op(g.shape, LAYOUTS[(i + 1) % 3], g), Op(x.shape, LAYOUTS[(i + 2) % 3], add)
        for addend in (None, A):
            GX = Op(x.shape, LAYOUTS[(i + (1 if addend is None else 0)) % 3])
            _bwd(H_, R.POOL_MAX, X, G, addend, GX, H, W, C, k, s, p)
            ref, _ = R.pool2d_bwd_ref(R.POOL_MAX, x, g, k, s, p, addend=None if addend is None else add)
            assert torch.equal(GX.value().double(), ref), (H, W, C, layout, addend is not None)
            assert GX.untouched()


def test_max_backward_routes_by_the_nan_and_inf_rules(H_):
    """NaN wins (the last one), an all -inf window sends its gradient to its first in-image tap."""
    k, s, p = 5, 1, 2
    for i, kind in enumerate(("nan", "inf")):
        H, W, C = 13, 9, 6
        x = R.inputs(kind, (N, H, W, C), seed=500 + i)
        g = _int_grad((N, H, W, C), 510 + i)
        X, G, GX = Op(x.shape, "vec4", x), Op(g.shape, "dense", g), Op(x.shape, "odd")
        _bwd(H_, R.POOL_MAX, X, G, None, GX, H, W, C, k, s, p)
        ref, _ = R.pool2d_bwd_ref(R.POOL_MAX, x, g, k, s, p)
        assert torch.equal(GX.value().double(), ref), kind


# ------------------------------------------------------------------------------------------ AVG / SUM
@pytest.mark.parametrize("kind", ["avg", "sum"])
@pytest.mark.parametrize("k,s,p", KSP, ids=KSP_IDS)
def test_avg_and_sum_within_the_rounding_bound(H_, k, s, p, kind):
    kd = KINDS[kind]
    roundings = k * k + 2
    pow2 = k in (2, 4)                                           # dividing by and multiplying with k, k*k is then exact
    for H, W, C, layout, i in _combos(k, p):
        Ho, Wo = R.out_size(H, k, s, p), R.out_size(W, k, s, p)
        for dyadic in (False, True):
            gen = torch.Generator().manual_seed(600 + i)
            if dyadic:
                x = torch.randint(-64, 65, (N, H, W, C), generator=gen).float() / 8
                g = torch.randint(-64, 65, (N, Ho, Wo, C), generator=gen).float() / 8
                add = torch.randint(-64, 65, (N, H, W, C), generator=gen).float() / 8
            else:
                x, g = torch.randn((N, H, W, C), generator=gen), torch.randn((N, Ho, Wo, C), generator=gen)
                add = torch.randn((N, H, W, C), generator=gen)
            X, Y = Op(x.shape, layout, x), Op(g.shape, LAYOUTS[(i + 1) % 3])
            _fwd(H_, kd, X, Y, H, W, C, k, s, p)
            ref, mag = R.pool2d_fwd_ref(kd, x, k, s, p)
            out = Y.value().double()
            err = (out - ref).abs()
            print(f"{kind} fwd k{k}s{s}p{p} {H}x{W}x{C} {layout} dyadic={dyadic}: max err / (U mag) = "
                  f"{float((err / (R.U * mag).clamp_min(1e-300)).max()):.3f} (bound {roundings})")
            assert bool((err <= roundings * R.U * mag).all()), (H, W, C, layout)
            if dyadic and (kd == R.POOL_AVG or pow2):
                # the sum is exact; AVG then rounds the exact quotient once, as the reference rounded to fp32 does
                assert torch.equal(out, ref.float().double()), (H, W, C, layout)
            assert Y.untouched()
            G, A = Op(g.shape, LAYOUTS[(i + 2) % 3], g), Op(x.shape, layout, add)
            for addend in (None, A):
                GX = Op(x.shape, LAYOUTS[(i + 1) % 3])
                _bwd(H_, kd, None, G, addend, GX, H, W, C, k, s, p)
                gref, gmag = R.pool2d_bwd_ref(kd, x, g, k, s, p, addend=None if addend is None else add)
                gout = GX.value().double()
                gerr = (gout - gref).abs()
                print(f"{kind} bwd k{k}s{s}p{p} {H}x{W}x{C} addend={addend is not None} dyadic={dyadic}: max err / (U mag)"
                      f" = {float((gerr / (R.U * gmag).clamp_min(1e-300)).max()):.3f} (bound {roundings})")
                assert bool((gerr <= roundings * R.U * gmag).all()), (H, W, C, layout)
                if dyadic and pow2:
                    assert torch.equal(gout, gref), (H, W, C, layout)
                assert GX.untouched()


@pytest.mark.parametrize("k,s", [(2, 2), (5, 2), (3, 1), (2, 1), (7, 3), (4, 4)])
def test_without_padding_the_bits_of_the_unpadded_entry_points(H_, k, s):
    for (H, W), C in zip(((7, 7), (13, 9), (37, 70), (8, 11)), (3, 8, 6, 36)):
        Ho, Wo = R.out_size(H, k, s, 0), R.out_size(W, k, s, 0)
        gen = torch.Generator().manual_seed(700 + H)
        for name, kd in KINDS.items():
            x = (torch.rand((N, H, W, C), generator=gen) < 0.4).float() if name == "max" else \
                torch.randn((N, H, W, C), generator=gen)
            g = torch.randn((N, Ho, Wo, C), generator=gen)
            xd, gd = x.cuda(), g.cuda()
            y0, gx0 = torch.empty((N, Ho, Wo, C), device="cuda"), torch.empty((N, H, W, C), device="cuda")
            H_.call("snn_pool_fwd", kd, xd.data_ptr(), y0.data_ptr(), N, H, W, C, Ho, Wo, k, s, _st())
            H_.call("snn_pool_bwd", kd, xd.data_ptr(), gd.data_ptr(), gx0.data_ptr(), N, H, W, C, Ho, Wo, k, s, _st())
            for layout in LAYOUTS:
                X, G = Op(x.shape, layout, x), Op(g.shape, layout, g)
                Y, GX = Op(g.shape, layout), Op(x.shape, layout)
                _fwd(H_, kd, X, Y, H, W, C, k, s, 0)
                _bwd(H_, kd, X if kd == R.POOL_MAX else None, G, None, GX, H, W, C, k, s, 0)
                assert R.same_bits(Y.value(), y0), (name, H, W, C, layout)
                assert R.same_bits(GX.value(), gx0), (name, H, W, C, layout)


# ------------------------------------------------------------------------------------------ SPP
@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("k", [3, 5])
def test_spp_forward_bits(H_, k, levels):
    # the kernel lays 16, 32 or 64 column lanes over a frame's width (SHAPES: 16 and, at 70 wide, two column tiles of 64):
    # 33x30 takes 32 lanes and two row chunks with a ragged second one, 18x60 takes 64 lanes in one tile
    for H, W, C, layout, i in _combos(1, 0, more=[(33, 30), (18, 60)]):
        kind = ["binary", "normal", "nan", "inf"][i % 4]
        x = R.inputs(kind, (N, H, W, C), seed=800 + i)
        X = Op(x.shape, layout, x)
        Y = Op((N, H, W, (levels + 1) * C), LAYOUTS[(i + 1) % 3])     # a wider buffer, at a channel offset
        H_.call("snn_spp_fwd", X.ptr, X.ld, Y.ptr, Y.ld, N, H, W, C, k, levels, _st())
        ref = R.spp_fwd_ref(x, k, levels)
        assert R.same_bits(Y.value(), ref), (H, W, C, layout, kind)
        assert Y.untouched()
        # ... and the chained launches of the padded pool
        Z = Op((N, H, W, (levels + 1) * C), "dense")
        Z.buf[..., :C] = x.cuda()
        for j in range(levels):
            H_.call("snn_pool2d_fwd", R.POOL_MAX, Z.ptr + 4 * j * C, Z.ld, Z.ptr + 4 * (j + 1) * C, Z.ld, N, H, W, C, k, 1,
                    k // 2, _st())
        assert R.same_bits(Y.value(), Z.value()), (H, W, C, layout, kind)


@pytest.mark.parametrize("levels", [1, 2, 3])
@pytest.mark.parametrize("k", [3, 5])
def test_spp_backward_through_functional(H_, k, levels):
    from snn_for_object_detection_amd import functional as HF
    T, B = 2, 2
    for (H, W), C in zip(SHAPES, (6, 1, 3, 8, 36, 4)):
        x = R.inputs("binary", (N, H, W, C), seed=900 + H)
        g = _int_grad((N, H, W, (levels + 1) * C), 910 + H)
        xd = x.cuda().view(T, B, H, W, C).permute(0, 1, 4, 2, 3).requires_grad_()
        y = HF.spp(xd, k, levels)
        assert tuple(y.shape) == (T, B, (levels + 1) * C, H, W)
        yref = R.spp_fwd_ref(x, k, levels)
        assert R.same_bits(y.detach().permute(0, 1, 3, 4, 2).reshape(N, H, W, -1), yref)
        y.backward(g.cuda().view(T, B, H, W, -1).permute(0, 1, 4, 2, 3))
        ref, _ = R.spp_bwd_ref(yref, g, k, levels)
        got = xd.grad.permute(0, 1, 3, 4, 2).reshape(N, H, W, C).cpu().double()
        assert torch.equal(got, ref), (H, W, C)
