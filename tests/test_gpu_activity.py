"""The activity monitor on the device: ``snn_activity_count`` against ``tests/activity_ref.py`` on every instance, the three
sources of a LIF layer's count against each other, and the recorder on a model in eval mode and in a training step.

Counts are integers: every comparison is ``torch.equal``."""
import pytest
import torch

from tests import activity_ref as ref
from tests.util import synthetic_events, synthetic_labels

pytestmark = pytest.mark.gpu

TH = 0.5            # a threshold bf16 holds exactly; the next bf16 above it is 0.5 + 2^-8
SENTINEL = 0x7F7F7F7F7F7F7F7F


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


# --------------------------------------------------------------------------------------------- 1. every kind
def _values(shape, bf16, g):
    """Random values with the edge cases sprinkled in: +-0, a denormal, NaN, the threshold and its upper neighbour."""
    x = torch.randn(shape, generator=g)
    if bf16:
        special = torch.tensor([0.0, -0.0, 1e-40, float("nan"), TH, TH + 2.0 ** -8, -TH, 3.0]).to(torch.bfloat16)
        x = x.to(torch.bfloat16)
    else:
        th = torch.tensor(TH)
        special = torch.stack([torch.tensor(0.0), torch.tensor(-0.0), torch.tensor(1e-45), torch.tensor(float("nan")), th,
                               torch.nextafter(th, torch.tensor(float("inf"))), -th, torch.tensor(3.0)])
    pick = torch.randint(0, 16, shape, generator=g)
    return torch.where(pick < 8, special[pick.clamp(max=7)], x)


def _layouts(kind, C):
    """(name, row width of the buffer, channel offset of the slice) per case of one channel count."""
    if kind == ref.MASK:
        return [("spare-word", C // 32 + 1, 0), ("dense", C // 32, 0)]
    out = [("dense", C, 0), ("slice+8", C + 16, 8), ("slice+2", C + 16, 2)]
    if kind in (ref.NONZERO_BF16, ref.ABOVE_BF16):
        out.append(("slice+4", C + 16, 4))      # bf16: 8- but not 16-byte aligned
    return out


@pytest.mark.parametrize("per_step", [False, True], ids=["sum", "per-step"])
@pytest.mark.parametrize("kind", [ref.NONZERO_F32, ref.NONZERO_BF16, ref.ABOVE_F32, ref.ABOVE_BF16, ref.MASK],
                         ids=["nonzero-f32", "nonzero-bf16", "above-f32", "above-bf16", "mask"])
def test_counts_equal_the_reference_on_every_instance(S, kind, per_step):
    from snn_for_object_detection_amd import _hip
    HF = S.functional
    bf = kind in (ref.NONZERO_BF16, ref.ABOVE_BF16)
    es = 2 if bf else 4
    th = TH if kind in (ref.ABOVE_F32, ref.ABOVE_BF16) else 0.0
    channels = (32, 64, 96, 512) if kind == ref.MASK else (1, 3, 4, 24, 32, 64, 96, 512)
    seen = set()
    pending = []
    for T in (1, 6):
        for M in (1, 63, 64, 65, 315, 1425):
            for C in channels:
                for name, width, off in _layouts(kind, C):
                    g = _gen(T * 100000 + M * 1000 + C + off)
                    if kind == ref.MASK:
                        host = torch.randint(-2 ** 31, 2 ** 31, (T, M, width), generator=g, dtype=torch.int64).to(torch.int32)
                        host[:, ::3, 0] = 0
                        host[:, 1::7, 0] = -1
                        if width > C // 32:
                            host[..., C // 32:] = -1      # the spare word is all ones: never counted
                        view = host
                        ld = width
                    else:
                        host = _values((T, M, width), bf, g)
                        view = host[..., off:off + C]
                        ld = width
                    dev = host.cuda()
                    src_ptr = dev.data_ptr() + (0 if kind == ref.MASK else off * es)
                    aligned = src_ptr % (8 if bf else 16) == 0
                    vec = 32 if kind == ref.MASK else (4 if (C % 4 == 0 and ld % 4 == 0 and aligned) else 1)
                    plan = HF.activity_plan(kind, T, M, C, ld, aligned)
                    assert plan[0] == vec, (name, T, M, C, plan)
                    assert (plan[2] - 1) * plan[1] < M <= plan[2] * plan[1] and plan[3] % T == 0
                    seen.add(vec)
                    n = T * C if per_step else C
                    buf = torch.full((n + 16,), SENTINEL, dtype=torch.int64, device="cuda")    # bytes 0x7F throughout
                    counts = buf[8:8 + n]
                    want = ref.count(view if kind != ref.MASK else host, kind, C, th, per_step).reshape(-1)
                    got = []
                    for accumulate in (0, 1, 1):
                        _hip.call("snn_activity_count", src_ptr, kind, ld, th, T, M, C, int(per_step), counts.data_ptr(),
                                  accumulate, _st())
                        got.append(buf.clone())
                    pending.append(((name, T, M, C), want, got, dev, host))
    torch.cuda.synchronize()
    for case, want, got, dev, host in pending:
        n = want.numel()
        for k, b in enumerate(got):
            b = b.cpu()
            assert torch.equal(b[8:8 + n], want * (k + 1)), (case, k)        # overwrite, then add twice
            assert bool((b[:8] == SENTINEL).all()) and bool((b[8 + n:] == SENTINEL).all()), case
        back = dev.cpu()
        ints = torch.int32 if host.dtype != torch.bfloat16 else torch.int16
        assert torch.equal(back.view(ints), host.view(ints)), case          # the source is read only
    assert sum(int(want.sum()) for _, want, _, _, _ in pending) > 0
    assert seen == ({32} if kind == ref.MASK else {1, 4})                     # both instances have run


def test_edge_values_count_as_the_header_says(S):
    """One element of each edge value per channel: what counts is exactly what the header lists."""
    HF = S.functional
    th = torch.tensor(TH)
    up = torch.nextafter(th, torch.tensor(float("inf")))
    row = torch.stack([torch.tensor(0.0), torch.tensor(-0.0), torch.tensor(1e-45), torch.tensor(float("nan")), th, up,
                       torch.tensor(float("inf")), torch.tensor(-float("inf"))])
    x = row.reshape(1, 1, 1, 1, 8).cuda().permute(0, 1, 4, 2, 3)            # [T,B,C,H,W] = [1,1,8,1,1], channels-last
    assert HF.cl_stride(x) == 8
    nz = HF.spike_count(x).cpu()
    above = HF.spike_count(x, threshold=TH).cpu()
    assert nz.tolist() == [0, 0, 1, 1, 1, 1, 1, 1]          # -0.0 is zero; the denormal and NaN are not
    assert above.tolist() == [0, 0, 0, 0, 0, 1, 1, 0]       # strict; NaN is not above
    xb = torch.tensor([0.0, -0.0, 1e-40, float("nan"), TH, TH + 2.0 ** -8, float("inf"), -1.0]).to(torch.bfloat16)
    xb = xb.reshape(1, 1, 1, 1, 8).cuda().permute(0, 1, 4, 2, 3)
    assert HF.spike_count(xb).cpu().tolist() == [0, 0, 1, 1, 1, 1, 1, 1]
    assert HF.spike_count(xb, threshold=TH).cpu().tolist() == [0, 0, 0, 0, 0, 1, 1, 0]


def test_spike_count_wrapper_takes_slices_masks_and_out(S):
    HF = S.functional
    T, B, H, W, C = 3, 2, 5, 7, 32
    g = _gen(3)
    wide = _values((T, B, H, W, C + 16), False, g)
    x = wide.cuda()[..., 8:8 + C].permute(0, 1, 4, 2, 3)                   # a channel slice of a wider buffer
    rows = wide[..., 8:8 + C].reshape(T, B * H * W, C)
    assert torch.equal(HF.spike_count(x).cpu(), ref.count(rows, ref.NONZERO_F32, C))
    per = HF.spike_count(x, threshold=TH, per_step=True)
    assert torch.equal(per.cpu(), ref.count(rows, ref.ABOVE_F32, C, TH, True))
    again = HF.spike_count(x, threshold=TH, per_step=True, out=per)       # `out` is added to
    assert again is per and torch.equal(per.cpu(), 2 * ref.count(rows, ref.ABOVE_F32, C, TH, True))
    words = torch.randint(-2 ** 31, 2 ** 31, (T, B, H, W, 2), generator=g, dtype=torch.int64).to(torch.int32)
    words[..., 1] = -1
    m = words.cuda()[..., :1]                                              # the first word of two-word rows
    assert torch.equal(HF.spike_count(None, mask=m).cpu(), ref.count(words.reshape(T, B * H * W, 2), ref.MASK, 32))
    with pytest.raises(RuntimeError):
        HF.spike_count(x.permute(0, 1, 2, 4, 3))                           # not channels-last
    with pytest.raises(RuntimeError):
        HF.spike_count(x, out=torch.zeros(C, device="cuda"))               # not int64


# ------------------------------------------------------------------------------- 2. three sources, one answer
def test_spikes_potentials_and_mask_give_one_count(S):
    from snn_for_object_detection_amd import _hip
    HF = S.functional
    T, M, C = 6, 315, 64
    g = _gen(21)
    p = HF.neuron_params()
    y = (torch.randn(T, M, C, generator=g) * 4.0 + 2.0).cuda()
    alpha = (1.0 + 0.2 * torch.randn(T, C, generator=g)).cuda()          # the BatchNorm affine of the fused scan
    beta = (0.3 * torch.randn(T, C, generator=g)).cuda()
    out = torch.empty(T, M, C, device="cuda")
    vdec0, vdec1 = torch.empty(T, M, C, device="cuda"), torch.empty(T, M, C, device="cuda")
    vT, iT = torch.empty(M, C, device="cuda"), torch.empty(M, C, device="cuda")
    mask = torch.empty(T, M, C // 32, device="cuda", dtype=torch.int32)
    head = (_hip.NEURON_LIF, y.data_ptr(), C, alpha.data_ptr(), beta.data_ptr(), None, None)
    tail = (vT.data_ptr(), iT.data_ptr())
    _hip.call("snn_affine_neuron_fwd", *head, out.data_ptr(), C, None, 0, *tail, vdec0.data_ptr(), T, M, C, p, 0, _st())
    _hip.call("snn_affine_neuron_fwd_mask", *head, None, C, None, 0, *tail, vdec1.data_ptr(), T, M, C, p,
              _hip.SCAN_SPIKES_FROM_VDEC | _hip.SCAN_SPIKE_MASK, _st(), mask.data_ptr(), C // 32)
    for per_step in (False, True):
        shape = (T, C) if per_step else (C,)
        got = []
        for src, kind, ld, th in ((out, ref.NONZERO_F32, C, 0.0), (vdec0, ref.ABOVE_F32, C, float(p.v_th)),
                                  (vdec1, ref.ABOVE_F32, C, float(p.v_th)), (mask, ref.MASK, C // 32, 0.0)):
            counts = torch.empty(shape, dtype=torch.int64, device="cuda")
            _hip.call("snn_activity_count", src.data_ptr(), kind, ld, th, T, M, C, int(per_step), counts.data_ptr(), 0, _st())
            got.append(counts.cpu())
        assert all(torch.equal(got[0], c) for c in got[1:])
        assert torch.equal(got[0], ref.count(out.cpu(), ref.NONZERO_F32, C, 0.0, per_step))
        total = int(got[0].sum())
        assert 0 < total < T * M * C


# ------------------------------------------------------------------------------------------- 3. model, eval
def _adopt_batch_statistics(model):
    """BatchNorm momentum 1: one train-mode pass leaves the statistics of that pass as the running ones, so the eval-mode
    network fires as the train-mode one does (with the default momentum of 0.1, one pass leaves it nearly silent)."""
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm2d):
            m.momentum = 1.0


@pytest.mark.parametrize("T,adopt", [(5, False), (20, True)], ids=["one-warm-pass", "batch-statistics-T20"])
def test_eval_report_equals_the_spike_taps_of_all_19_lif_layers(S, T, adopt):
    """The clip of ``test_tiny_yolo_eval_spikes_and_preds_match_oracle`` (5 steps, one warming pass: only the first layers
    fire at all), and a longer one on the statistics of the warming pass, in which the spikes reach deep layers."""
    B, H, W = 2, 32, 48
    torch.manual_seed(2)
    model = S.TinyYolo(num_classes=2, time_window=0, state_storage=True).cuda()
    X = synthetic_events(T, B, H, W, p=0.1, seed=3).cuda()
    if adopt:
        _adopt_batch_statistics(model)
    model.train()
    with torch.no_grad():
        model(X)            # warms the running statistics
    model.eval()
    with pytest.raises(RuntimeError, match="eval mode"):
        model.train().activity_report(X)
    model.eval()
    rep = model.activity_report(X, per_step=True)
    taps = {n: z for n, z in model.spike_taps().items() if "head_net" not in n}      # (the head's taps are LI potentials)
    assert len(taps) == 19 and len(rep["layers"]) == 19
    assert {n + ".module" for n in taps} == set(rep["layers"])
    fired = 0
    for name, z in taps.items():
        layer = rep["layers"][name + ".module"]
        want = z.sum((1, 3, 4)).to(torch.int64).cpu()                                  # [T, C]
        assert torch.equal(layer["spikes"], want), name
        assert layer["neurons"] == T * B * z.shape[3] * z.shape[4]
        assert layer["sources"] == {"spikes": 1}
        fired += int(want.sum())
    assert rep["totals"]["spikes"] == fired
    if adopt:
        assert fired > 0 and sum(1 for r in rep["layers"].values() if r["rate"] > 0) >= 5
    # without per_step: the same counts summed over the timesteps, and a second clip adds up
    from snn_for_object_detection_amd import activity
    with torch.no_grad(), activity.record(model) as rec:
        model(X)
        model(X)
    twice = rec.report()
    for name, layer in rep["layers"].items():
        assert torch.equal(twice["layers"][name]["spikes"], 2 * layer["spikes"].sum(0)), name
        assert twice["layers"][name]["neurons"] == 2 * layer["neurons"]


def test_eval_default_executor_counts_fused_shortcuts_from_potentials(S):
    """The default model (no taps) folds the bottleneck shortcuts into the LIF store: under ``no_grad`` those layers keep
    nothing to count and get potentials for the pass.  Same weights, same clip: the counts of the tapped model."""
    T, B, H, W = 20, 2, 32, 48      # (long enough for the spikes to reach the bottlenecks)
    X = synthetic_events(T, B, H, W, p=0.1, seed=3).cuda()
    reports = []
    for taps in (True, False):
        torch.manual_seed(2)
        model = S.TinyYolo(num_classes=2, time_window=0, state_storage=taps).cuda().train()
        _adopt_batch_statistics(model)
        with torch.no_grad():
            model(X)
        reports.append(model.eval().activity_report(X))
    tapped = {n.replace(".module", ""): r for n, r in reports[0]["layers"].items()}
    plain = reports[1]["layers"]
    assert set(tapped) == set(plain) and len(plain) == 19
    for name in plain:
        assert torch.equal(plain[name]["spikes"], tapped[name]["spikes"]), name
    shortcut = [r for r in plain.values() if r["sources"] == {"potentials": 1}]
    assert len(shortcut) >= 9 and sum(int(r["spikes"].sum()) for r in shortcut) > 0      # the nine bottlenecks


# --------------------------------------------------------------------------------------- 4. / 5. model, training
class _Spy:
    def __init__(self):
        self.calls = []

    def before(self, name, args):
        self.calls.append((name, args[1] if name == "snn_activity_count" else None))

    def after(self, tok):
        pass


def _training_step(S, X, labels, record, storage="fp32", **settings):
    """One training step of a freshly built default TinyYolo under a FlatTrainer -> (loss, flat gradient, report, calls)."""
    from snn_for_object_detection_amd import _hip, activity
    from snn_for_object_detection_amd.trainer import FlatTrainer
    HF = S.functional
    was_storage = HF.get_activation_storage()
    HF.set_activation_storage(storage)
    spy = _Spy()
    _hip.PROFILER = spy
    try:
        with HF.levers(**settings):
            torch.manual_seed(2)
            model = S.TinyYolo(num_classes=2, time_window=0).cuda().train()
            tr = FlatTrainer(model, lr=1e-3)
            tr.zero_grad()
            rep = None
            if record:
                with activity.record(model) as rec:
                    loss = model.training_step((X, labels))
                loss.backward()
                tr.synchronize()
                rep = rec.report()
            else:
                loss = model.training_step((X, labels))
                loss.backward()
                tr.synchronize()
            torch.cuda.synchronize()
    finally:
        _hip.PROFILER = None
        HF.set_activation_storage(was_storage)
    return loss.detach().clone(), tr.flat_grad.clone(), rep, spy.calls


@pytest.fixture(scope="module")
def training_runs(S):
    T, B, H, W = 12, 2, 32, 48      # (long enough for the spikes to pass the first stage)
    X = synthetic_events(T, B, H, W, p=0.1, seed=3).cuda()
    labels = synthetic_labels(B).cuda()
    runs = {"off": _training_step(S, X, labels, False),
            "as-built": _training_step(S, X, labels, True),
            "no-mask": _training_step(S, X, labels, True, USE_SPIKE_MASK=False),
            "no-vdec-spikes": _training_step(S, X, labels, True, USE_SPIKES_FROM_VDEC=False),
            "mask-everywhere": _training_step(S, X, labels, True, SPIKE_MASK_MIN_BYTES=0)}
    return X, runs


def test_training_counts_do_not_depend_on_the_executor_setting(S, training_runs):
    _, runs = training_runs
    base = runs["as-built"][2]
    assert len(base["layers"]) == 19 and base["totals"]["spikes"] > 0
    for name in ("no-mask", "no-vdec-spikes", "mask-everywhere"):
        rep = runs[name][2]
        assert list(rep["layers"]) == list(base["layers"]), name
        for layer in base["layers"]:
            assert torch.equal(rep["layers"][layer]["spikes"], base["layers"][layer]["spikes"]), (name, layer)
            assert rep["layers"][layer]["neurons"] == base["layers"][layer]["neurons"]
        assert rep["totals"]["synops"] == base["totals"]["synops"], name
        # the operands the convolutions read carry the same spikes in every form
        assert {k: v["nonzero_inputs"] for k, v in rep["convs"].items()} == \
               {k: v["nonzero_inputs"] for k, v in base["convs"].items()}, name
    # the settings did change what was counted: the default step reads masks or potentials where spikes were never
    # written, the opened size gate takes the mask, and without either every layer has a spike tensor or potentials
    kinds = {name: {k for n, k in runs[name][3] if n == "snn_activity_count"} for name in runs}
    assert kinds["as-built"] & {ref.ABOVE_F32, ref.MASK}
    assert ref.MASK in kinds["mask-everywhere"] and ref.MASK not in kinds["no-mask"]
    sources = lambda name: [tuple(r["sources"]) for r in runs[name][2]["layers"].values()]   # noqa: E731
    assert ("mask",) in sources("mask-everywhere") and ("mask",) not in sources("no-mask")
    assert ("potentials",) in sources("as-built")
    assert sum(int(r["spikes"].sum()) for r in runs["mask-everywhere"][2]["layers"].values() if tuple(r["sources"]) == ("mask",)) > 0


def test_recorder_changes_neither_loss_nor_gradient_and_off_means_no_launch(S, training_runs):
    _, runs = training_runs
    loss_off, grad_off, _, calls_off = runs["off"]
    loss_on, grad_on, _, calls_on = runs["as-built"]
    assert torch.equal(loss_on, loss_off) and torch.equal(grad_on, grad_off)
    assert float(grad_off.abs().max()) > 0
    assert not [n for n, _ in calls_off if n.startswith("snn_activity")]
    on = [n for n, _ in calls_on if n.startswith("snn_activity")]
    assert len(on) >= 19 and [n for n, _ in calls_on if not n.startswith("snn_activity")] == [n for n, _ in calls_off]


def test_bf16_storage_step_reports_every_lif_layer(S, training_runs):
    X, _ = training_runs
    labels = synthetic_labels(X.shape[1]).cuda()
    loss, _, rep, calls = _training_step(S, X, labels, True, storage="bf16")
    assert bool(torch.isfinite(loss))
    assert len(rep["layers"]) == 19
    for name, layer in rep["layers"].items():
        s = layer["spikes"]
        assert s.shape == (layer["channel_rate"].numel(),) and bool((s >= 0).all()) and bool((s <= layer["neurons"]).all()), name
        assert 0.0 <= layer["rate"] <= 1.0
    assert {k for n, k in calls if n == "snn_activity_count"} & {ref.NONZERO_BF16, ref.ABOVE_BF16}


def test_synops_of_the_first_convolution_and_of_a_conv_behind_a_lif(S, training_runs):
    from snn_for_object_detection_amd import activity
    X, runs = training_runs
    rep = runs["as-built"][2]
    first = next(iter(rep["convs"]))
    assert first == "base_net.net.net.0.0.weight"
    nz = int(X.count_nonzero())
    conv = rep["convs"][first]
    assert conv["nonzero_inputs"] == nz and conv["inputs"] == X.numel()
    assert conv["synops"] == nz * 64 * 9 / 4 and conv["macs"] == X.numel() * 64 * 9 / 4
    assert rep["totals"]["synops"] == sum(c["synops"] for c in rep["convs"].values()) <= rep["totals"]["macs"]
    # Conv -> Norm -> LIF -> Conv: what the second convolution reads is what the LIF layer fired - in a training pass (the
    # convolution thresholds the potentials itself) and in eval mode under no_grad (it reads the spike tensor)
    torch.manual_seed(5)
    blk = S.BlockGen(2, [S.Conv(32), S.Norm(), S.LIF(), S.Conv(32, 1)]).cuda().train()
    x = synthetic_events(3, 2, 16, 24, p=0.3, seed=1).cuda()
    _adopt_batch_statistics(blk)
    for grad in (True, False):
        blk.train(grad)          # (the eval pass runs on the statistics the training pass left)
        with torch.set_grad_enabled(grad), activity.record(blk) as rec:
            blk(x)
        r = rec.report()
        (lif_name, lif), = r["layers"].items()
        assert lif_name == "net.0.2" and list(r["convs"]) == ["net.0.0.weight", "net.0.3.weight"]
        fired = int(lif["spikes"].sum())
        assert fired > 0 and r["convs"]["net.0.3.weight"]["nonzero_inputs"] == fired
        assert r["convs"]["net.0.3.weight"]["synops"] == fired * 32
        assert tuple(lif["sources"]) == (("potentials",) if grad else ("spikes",))
