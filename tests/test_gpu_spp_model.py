"""``SPP()`` and padded ``Pool`` inside generated networks: the fused pyramid against its spelled-out form
``Dense([[Pass()], [P], [P, P], [P, P, P]])`` with ``P = Pool("M", k, 1, k // 2)``, placement in a parent's concat
buffer, one timestep against a sequence of one, bf16 storage, and a small detector that closes its backbone with the SPPF
stage.  Max pooling only selects, so forward outputs and neuron states must be ``torch.equal``; with binary inputs and
integer output gradients so must the input gradients of a bare pyramid.  Behind convolutions the gradients take the
project's block-level bound (rel_err < 1e-4, tests/test_gpu_next_ops.py): their sums are not exact."""
import pytest
import torch

from tests.util import rel_err, synthetic_events, synthetic_labels

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S(hip_lib):
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import snn_for_object_detection_amd as pkg
    return pkg


def _spelled(S, k=5, levels=3):
    P = lambda: S.Pool("M", k, 1, k // 2)
    return S.Dense([[S.Pass()]] + [[P() for _ in range(j)] for j in range(1, levels + 1)])


def _flat_states(tree):
    out = []
    for s in tree:
        if isinstance(s, (list, tuple)) and not hasattr(s, "_fields"):
            out += _flat_states(s)
        elif s is not None:
            out += [t for t in s if t is not None] if isinstance(s, tuple) else [s]
    return out


@pytest.mark.parametrize("k,levels", [(5, 3), (3, 2), (5, 1)])
def test_bare_pyramid_equals_the_spelled_out_dense(S, k, levels):
    T, B, C, H, W = 2, 2, 6, 13, 9
    a = S.BlockGen(C, [S.SPP(k, levels)]).cuda()
    b = S.BlockGen(C, _spelled(S, k, levels)).cuda()
    assert a.out_channels == b.out_channels == (levels + 1) * C
    x = (torch.rand(T, B, C, H, W, generator=torch.Generator().manual_seed(1)) < 0.3).float()
    xa = S.functional.to_channels_last(x.cuda()).requires_grad_()
    xb = S.functional.to_channels_last(x.cuda()).requires_grad_()
    ya, _ = a(xa)
    yb, _ = b(xb)
    assert ya.shape == yb.shape == (T, B, (levels + 1) * C, H, W) and torch.equal(ya, yb)
    assert torch.equal(ya[:, :, :C], xa.detach()) and float(ya.detach().sum()) > float(xa.detach().sum())
    g = torch.randint(-4, 5, ya.shape, generator=torch.Generator().manual_seed(2)).float().cuda()
    ya.backward(g)
    yb.backward(g)
    assert torch.equal(xa.grad, xb.grad)


@pytest.mark.parametrize("trainer", [False, True], ids=["autograd", "flat_trainer"])
def test_sppf_stage_equals_the_spelled_out_stage(S, trainer):
    from snn_for_object_detection_amd.trainer import FlatTrainer
    T, B, C, H, W = 8, 2, 32, 9, 10

    def stage(mid):
        return [S.Conv(16, 1), S.Norm(), S.LIF(), mid, S.Conv(32, 1), S.Norm(), S.LIF()]

    torch.manual_seed(7)
    a = S.BlockGen(C, stage(S.SPP(5, 3)))
    b = S.BlockGen(C, stage(_spelled(S)))
    g = torch.Generator().manual_seed(8)
    for m in a.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            # (large enough that the LIF layers spike within the few timesteps of a test)
            m.weight.data.copy_(2.0 + torch.rand(m.weight.shape, generator=g))
    b.load_state_dict({k: v.clone() for k, v in a.state_dict().items()})
    a, b = a.cuda().train(), b.cuda().train()
    x = (torch.rand(T, B, C, H, W, generator=torch.Generator().manual_seed(4)) < 0.3).float()
    tr_a = tr_b = None
    if trainer:
        tr_a, tr_b = FlatTrainer(a, lr=1e-3), FlatTrainer(b, lr=1e-3)
        tr_a.zero_grad()
        tr_b.zero_grad()
    xa = S.functional.to_channels_last(x.cuda()).requires_grad_()
    xb = S.functional.to_channels_last(x.cuda()).requires_grad_()
    ya, sa = a(xa)
    yb, sb = b(xb)
    assert ya.shape == yb.shape and torch.equal(ya, yb), f"forward differs: {rel_err(ya, yb):.3g}"
    assert float(ya.detach().abs().sum()) > 0                    # (spikes: the comparison is not one of zeros)
    fa, fb = _flat_states(sa), _flat_states(sb)
    assert len(fa) == len(fb) > 0
    for u, v in zip(fa, fb):
        assert torch.equal(u, v), "neuron state differs"
    gy = torch.randn(ya.shape, generator=torch.Generator().manual_seed(5)).cuda()
    (ya * gy).sum().backward()
    (yb * gy).sum().backward()
    assert rel_err(xa.grad, xb.grad) < 1e-4, f"input gradient {rel_err(xa.grad, xb.grad):.3g}"
    if trainer:
        ga, gb = tr_a.grads_by_name(a), tr_b.grads_by_name(b)
    else:
        ga = {n: p.grad for n, p in a.named_parameters()}
        gb = {n: p.grad for n, p in b.named_parameters()}
    assert set(ga) == set(gb) and len(ga) == 4
    for n in ga:
        assert float(ga[n].abs().max()) > 0
        assert rel_err(ga[n], gb[n]) < 1e-4, f"{n}: {rel_err(ga[n], gb[n]):.3g}"


def test_spp_writes_its_slices_of_the_parent_buffer_itself(S, monkeypatch):
    HF = S.functional
    T, B, C, H, W = 2, 2, 6, 5, 7
    x = HF.to_channels_last((torch.rand(T, B, C, H, W, generator=torch.Generator().manual_seed(3)) < 0.3).float().cuda())
    promise = HF.ConcatPromise(24)
    dest = HF.Dest(promise, 0, 18)
    y = HF.spp(x, 3, 2, dest=dest)
    assert dest.holds(y) and y.untyped_storage().data_ptr() == promise.buf.untyped_storage().data_ptr()
    assert HF.cl_stride(y) == 24 and torch.equal(y, HF.spp(x, 3, 2))
    # ... and inside a block: the placement that follows the layer finds the result in place
    seen = []
    place = HF.place

    def spy(t, d):
        seen.append((t.shape[2], d.holds(t)))
        return place(t, d)
    monkeypatch.setattr(HF, "place", spy)
    blk = S.BlockGen(C, S.Dense([[S.SPP(3, 2)], [S.Pass()]])).cuda()
    out, _ = blk(x)
    assert (18, True) in seen and (18, False) not in seen
    assert tuple(out.shape) == (T, B, 24, H, W)
    assert torch.equal(out[:, :, :18], HF.spp(x, 3, 2)) and torch.equal(out[:, :, 18:], x)


def test_one_timestep_is_the_sequence_of_one(S):
    HF = S.functional
    x = HF.to_channels_last(torch.randn(1, 3, 6, 13, 9, generator=torch.Generator().manual_seed(5)).cuda())
    assert torch.equal(HF.spp(x[0], 5, 3), HF.spp(x, 5, 3)[0])
    assert tuple(HF.spp(x[0], 3, 1).shape) == (3, 12, 13, 9)
    for kind in (0, 1, 2):
        assert torch.equal(HF.pool2d(x[0], kind, 3, 2, 1), HF.pool2d(x, kind, 3, 2, 1)[0])
    mod = S.Pool("M", 5, 1, 2).get(6)[0]
    assert torch.equal(mod(x[0]), mod(x)[0]) and tuple(mod(x).shape) == (1, 3, 6, 13, 9)
    blk = S.BlockGen(6, [S.SPP()]).cuda()
    assert torch.equal(blk(x[0])[0], blk(x)[0][0])


def test_bf16_storage_runs_the_fp32_kernels_between_two_conversions(S):
    HF = S.functional
    x = HF.to_bfloat16(HF.to_channels_last(torch.randn(2, 2, 36, 7, 10, generator=torch.Generator().manual_seed(6)).cuda()))
    y = HF.spp(x, 5, 3)
    want = HF.to_bfloat16(HF.spp(HF.to_float32(x), 5, 3))
    assert y.dtype == torch.bfloat16 and tuple(y.shape) == (2, 2, 144, 7, 10)
    assert torch.equal(y.view(torch.int16), want.view(torch.int16))
    for kind in (0, 1, 2):
        y = HF.pool2d(x, kind, 3, 2, 1)
        want = HF.to_bfloat16(HF.pool2d(HF.to_float32(x), kind, 3, 2, 1))
        assert y.dtype == torch.bfloat16 and tuple(y.shape) == (2, 2, 36, 4, 5)
        assert torch.equal(y.view(torch.int16), want.view(torch.int16))


def test_functional_refuses_what_the_library_does_not_cover(S):
    HF = S.functional
    x = HF.to_channels_last(torch.zeros(1, 1, 4, 6, 6).cuda())
    with pytest.raises(RuntimeError, match="not covered"):
        HF.pool2d(x, 1, 5, 1, 3)
    with pytest.raises(RuntimeError, match="not covered"):
        HF.pool2d(x, 1, 9, 1, 2)
    with pytest.raises(RuntimeError, match="not covered"):
        HF.pool2d(x[..., :2, :], 0, 7, 1, 1)                     # a window larger than the padded image
    with pytest.raises(RuntimeError, match="not covered"):
        HF.spp(x, 4, 3)
    with pytest.raises(RuntimeError, match="not covered"):
        HF.spp(x, 5, 4)


def test_detector_with_an_sppf_stage_trains(S):
    """A small generated detector that closes its backbone with Conv(c/2, 1), SPP(), Conv(c, 1) takes two FlatTrainer steps."""
    from snn_for_object_detection_amd.layer_gen import HipSPP
    from snn_for_object_detection_amd.trainer import FlatTrainer
    L = S

    class Net(S.SODa):
        def backbone_cfgs(self):
            return [L.Conv(32, 3, 2), L.Norm(), L.LIF(), L.Conv(64, 3, 2), L.Norm(), L.LIF(),
                    L.Conv(32, 1), L.Norm(), L.LIF(), L.SPP(), L.Conv(64, 1), L.Norm(), L.LIF()]

        def neck_cfgs(self):
            return [L.Conv(64, 3, 1), L.Norm(), L.LIF(), L.Return(), L.Conv(64, 3, 2), L.Norm(), L.LIF(), L.Return()]

        def head_cfgs(self, box_out, cls_out):
            return [[L.Conv(kernel_size=1), L.Norm(), L.LI(), L.Tanh()], [L.Conv(box_out, 1)], [L.Conv(cls_out, 1)]]

    T, B, H, W = 3, 2, 64, 64
    X, labels = synthetic_events(T, B, H, W, p=0.1).cuda(), synthetic_labels(B).cuda()
    torch.manual_seed(3)
    m = Net(num_classes=2, time_window=0).cuda().train()
    assert sum(isinstance(mod, HipSPP) for mod in m.modules()) == 1
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            torch.nn.init.constant_(mod.weight, 2.5)             # (every LIF layer spikes within the 3 timesteps)
    tr = FlatTrainer(m, lr=1e-2)
    start = {n: p.detach().clone() for n, p in m.named_parameters() if p.requires_grad}
    for _ in range(2):
        tr.zero_grad()
        loss = m.training_step((X, labels))
        loss.backward()
        tr.synchronize()
        assert torch.isfinite(loss).item()
        tr.step()
    assert len(start) >= 16                                      # (convolution and BatchNorm weights of every part)
    still = [n for n, p in m.named_parameters()
             if n in start and (torch.equal(start[n], p.detach()) or not torch.isfinite(p).all().item())]
    assert not still, f"weights that did not move: {still}"
