"""Pins that come from the REFERENCE itself (fixtures written by tests/golden/make_golden.py in the build container):

* ``convlstm.npz``       - outputs / gradients of the reference's own ``models/modules/conv_lstm.py:51-78`` on seeded
  inputs: pins ``oracle.net.ConvLSTM`` (the HIP ``LSTM()`` layer is checked against the same file in
  ``tests/test_gpu_next_ops.py``);
* ``tiny_yolo_desc.json`` - the nested layer lists the reference's ``models/tiny_yolo.py:16-89`` builds: pins the
  product's transcription of the net description independently of the oracle (which consumes the product's
  description object), together with the layer census of SURVEY Appendix A.
"""
import json
import os

import numpy as np
import pytest
import torch

import snn_for_object_detection_amd as S
from oracle import net as ON
from tests.util import executor_block_cfg, executor_net


@pytest.fixture(autouse=True)
def _recorded_thread_count():
    """The fixtures were recorded with 8 intra-op threads (``make_golden.py``); fewer split some CPU reductions of the
    ConvLSTM and executor runs differently, and the bit-exact pins then depend on the host's core count."""
    n = torch.get_num_threads()
    torch.set_num_threads(8)
    yield
    torch.set_num_threads(n)


def test_oracle_convlstm_matches_reference_vectors(golden_dir):
    z = np.load(os.path.join(golden_dir, "convlstm.npz"))
    x = torch.from_numpy(z["x"]).requires_grad_()
    T, B, Cin = x.shape[:3]
    Ch = z["h"].shape[2]
    cell = ON.ConvLSTM(Cin, Ch)
    with torch.no_grad():
        cell.conv.weight.copy_(torch.from_numpy(z["weight"]))
    state, hs, cs = None, [], []
    for t in range(T):
        h, state = cell(x[t], state)
        hs.append(h)
        cs.append(state[1])
    hs, cs = torch.stack(hs), torch.stack(cs)
    assert torch.equal(hs.detach(), torch.from_numpy(z["h"])) and torch.equal(cs.detach(), torch.from_numpy(z["c"]))
    ((hs * torch.from_numpy(z["gh"])).sum() + (state[1] * torch.from_numpy(z["gc"])).sum()).backward()
    assert torch.allclose(x.grad, torch.from_numpy(z["gx"]), rtol=1e-6, atol=1e-7)
    assert torch.allclose(cell.conv.weight.grad, torch.from_numpy(z["gw"]), rtol=1e-6, atol=1e-6)


def _render(item):
    if isinstance(item, (list, tuple)):
        tag = type(item).__name__ if type(item).__name__ in ("Residual", "Dense") else "list"
        return {"merge": tag, "items": [_render(i) for i in item]}
    kind = type(item).__name__
    fields = {"Conv": ("out_channels", "kernel_size", "stride"), "Norm": ("bias",), "LIF": ("state_storage",),
              "LI": ("state_storage",), "SLI": ("state_storage",), "LSTM": ("hidden_size",),
              "Pool": ("type", "kernel_size", "stride"), "Up": ("scale", "mode")}.get(kind, ())
    return {"layer": kind, **{f: getattr(item, f) for f in fields}}


def test_tiny_yolo_description_equals_the_reference_description(golden_dir):
    want = json.load(open(os.path.join(golden_dir, "tiny_yolo_desc.json")))
    m = S.TinyYolo(num_classes=2, time_window=0)
    got = {"backbone": _render(m.backbone_cfgs()), "neck": _render(m.neck_cfgs()),
           "head": _render(m.head_cfgs(36, 27))}
    assert json.loads(json.dumps(got, sort_keys=True)) == want


def test_tiny_yolo_layer_census():
    """48 Conv, 22 Norm, 19 LIF, 3 LI, 14 Residual merges, 19 Dense merges, 28 Pass, 3 Tanh,
    3 Return - counted on the product's module tree, no oracle involved."""
    m = S.TinyYolo(num_classes=2, time_window=0)
    kinds = [type(x).__name__ for x in m.modules()]
    count = {k: kinds.count(k) for k in set(kinds)}
    assert count["HipConv2d"] == 48 and count["HipBatchNorm2d"] == 22
    assert count["LIFCell"] == 19 and count["LICell"] == 3
    assert count["Identity"] == 28 and count["HipTanh"] == 3 and count["Storage"] == 3
    merges = [b.merge for b in m.modules() if isinstance(b, S.BlockGen)]
    assert merges.count("residual") == 14 and merges.count("dense") == 19
    # conv census by (Cin, Cout, k, stride): the stage structure of the Appendix-A table
    convs = sorted((c.in_channels, c.out_channels, c.kernel_size[0], c.stride[0])
                   for c in m.modules() if isinstance(c, torch.nn.Conv2d))
    assert convs.count((2, 64, 3, 2)) == 1 and convs.count((32, 32, 3, 1)) == 2
    assert convs.count((64, 64, 3, 1)) == 3 and convs.count((128, 128, 3, 1)) == 9
    assert convs.count((64, 128, 3, 2)) == 1 and convs.count((128, 256, 3, 2)) == 1
    assert convs.count((256, 256, 3, 2)) == 2
    assert convs.count((768, 256, 1, 1)) == 1 and convs.count((640, 256, 1, 1)) == 1
    assert convs.count((512, 256, 1, 1)) == 1 and convs.count((320, 128, 1, 1)) == 1
    assert convs.count((256, 36, 1, 1)) == 3 and convs.count((256, 27, 1, 1)) == 3
    assert sum(1 for c in convs if c[2] == 3) == 19 and sum(1 for c in convs if c[2] == 1) == 29


def test_oracle_sli_matches_reference_vectors(golden_dir):
    """``sli.npz``: the reference's own ``sli_feed_forward_step`` (models/modules/sli.py:110-126) over a seeded
    sequence - the in-tree witness of norse's LI step ordering, pinned as data."""
    z = np.load(os.path.join(golden_dir, "sli.npz"))
    x = torch.from_numpy(z["x"]).requires_grad_()
    cell = ON.SLICell(dt=float(z["dt"]))
    state, vs = None, []
    for t in range(x.shape[0]):
        v, state = cell(x[t], state)   # state None at t = 0: the oracle builds SLICell.initial_state (0-dim v, zero i)
        vs.append(v)
    vs = torch.stack(vs)
    assert torch.equal(vs.detach(), torch.from_numpy(z["v"]))
    assert torch.equal(state[1].detach(), torch.from_numpy(z["i_final"]))
    ((vs * torch.from_numpy(z["gv"])).sum() + (state[1] * torch.from_numpy(z["gi"])).sum()).backward()
    assert torch.allclose(x.grad, torch.from_numpy(z["gx"]), rtol=1e-6, atol=1e-7)


def test_oracle_li_step_is_the_sli_step_without_the_gate(golden_dir):
    """The LI restatement (oracle/neurons.py, norse absent) against the reference-generated SLI vectors: with the
    saturation gate forced to 1 the SLI step IS norse's LI step (sli.py:110-126 vs SURVEY 8a-7), so feeding the LI
    restatement the gated inputs ``x * sigmoid(v_st - |v_prev|)`` recorded from the fixture must reproduce the fixture's
    potentials bit for bit - this pins the LI ordering (current jump first) and constants on reference data."""
    from oracle import neurons as NE
    z = np.load(os.path.join(golden_dir, "sli.npz"))
    x, v_ref = torch.from_numpy(z["x"]), torch.from_numpy(z["v"])
    state = None
    v_prev = torch.zeros_like(x[0])
    for t in range(x.shape[0]):
        gated = x[t] * torch.sigmoid(torch.as_tensor(1.0) - torch.abs(v_prev))
        v, state = NE.LICell(dt=float(z["dt"]))(gated, state)
        assert torch.equal(v.detach(), v_ref[t])
        v_prev = v.detach()
    assert torch.equal(state.i.detach(), torch.from_numpy(z["i_final"]))


def test_oracle_synapse_matches_reference_vectors(golden_dir):
    """``synapse.npz``: ``synapse_feed_forward_step`` (models/modules/synapse.py:73-103), sigma = 0 and 0.7."""
    z = np.load(os.path.join(golden_dir, "synapse.npz"))
    for tag in ("s0", "s07"):
        x = torch.from_numpy(z["x"]).clone().requires_grad_()
        cell = ON.SynapseCell(dt=float(z["dt"]), sigma_inhibition=float(z[f"sigma_{tag}"]))
        state, gs = None, []
        for t in range(x.shape[0]):
            g, state = cell(x[t], state)
            gs.append(g)
        gs = torch.stack(gs)
        assert torch.equal(gs.detach(), torch.from_numpy(z[f"g_{tag}"]))
        assert torch.equal(state[0].detach(), torch.from_numpy(z[f"p_final_{tag}"]))
        (gs * torch.from_numpy(z["gg"])).sum().backward()
        assert torch.allclose(x.grad, torch.from_numpy(z[f"gx_{tag}"]), rtol=1e-6, atol=1e-7)


# ------------------------------------------------------------------------------------------- event feed
def _events_case(z, tag):
    T, shift, step_us, clock, H, W, thr = (int(v) for v in z[f"{tag}_params"])
    ev = tuple(z[f"{tag}_events_{k}"] for k in "txyp")
    return T, shift, step_us, clock, H, W, thr, ev, z[f"{tag}_gt"]


def test_oracle_event_voxelisation_matches_reference_vectors(golden_dir):
    """``oracle/events.py`` against what the reference's OWN ``parse_data`` / ``_stack_data`` produced
    (``tests/golden/events.npz``, written by ``make_golden.py::events_golden`` from ``utils/datasets.py:311-344,378-435,
    127-135`` executed unmodified): non-zero cells, labels, the recording clock afterwards and the rejection of a sparse
    window, bit for bit - single-target GEN1, single-target 1 Mpx with events past the frame (clipped), multi-target."""
    from oracle import events as OE
    z = np.load(os.path.join(golden_dir, "events.npz"))
    for tag in ("st_gen1", "st_1mpx", "st_sparse"):
        T, shift, step_us, clock, H, W, thr, ev, gt = _events_case(z, tag)
        sample, more, clock_after, _ = OE.st_sample(gt, *ev, clock, T, shift, step_us, H, W, thr,
                                                    float(z[f"{tag}_box_size_threshold"]))
        assert more == bool(z[f"{tag}_more"]) and clock_after == int(z[f"{tag}_clock_after"]), tag
        assert (sample is None) == bool(z[f"{tag}_rejected"]), tag
        if sample is not None:
            feats, labels = sample
            assert feats.shape == (T, 2, H, W) and feats.dtype == np.float32
            assert np.array_equal(np.flatnonzero(feats.reshape(-1)), z[f"{tag}_nonzero"]), tag
            assert set(np.unique(feats)) <= {0.0, 1.0}
            assert np.array_equal(labels, z[f"{tag}_labels"]), tag
    assert bool(z["st_sparse_rejected"]) and not bool(z["st_gen1_rejected"])     # the fixture exercises both outcomes
    assert int(z["st_1mpx_events_x"].max()) > 1279                                 # ... and the clip of x past the frame
    T, _, step_us, clock, H, W, _, ev, gt = _events_case(z, "mt")
    feats, labels, clock_after = OE.mt_sample(gt, *ev, clock, T, step_us, H, W)
    assert np.array_equal(np.flatnonzero(feats.reshape(-1)), z["mt_nonzero"]) and clock_after == int(z["mt_clock_after"])
    assert np.array_equal(labels, z["mt_labels"])
    feats0, labels0, _ = OE.mt_sample(gt, *(e[:0] for e in ev), clock, T, step_us, H, W)
    assert int(np.count_nonzero(feats0)) == int(z["mt_empty_nonzero_count"]) == 0
    assert tuple(labels0.shape) == tuple(z["mt_empty_labels_shape"])
    # collate: ragged label lists (one sample without a box) padded with -1
    samples = [(z[f"stack_features_{b}"], z[f"stack_labels_{b}"]) for b in range(3)]
    feats, targets = OE.stack_batch(samples)
    assert np.array_equal(feats, z["stack_out_features"]) and np.array_equal(targets, z["stack_out_targets"])


# ------------------------------------------------------------------------------------------- executor, heads, loss
def test_oracle_executor_heads_and_loss_match_the_reference_run(golden_dir):
    """``oracle.net`` (BlockRef / SODaRef: executor, merges, state threading, taps, heads, flatten / concat, the time loop and
    ``_loss``) against ``tests/golden/executor.npz`` - what the REFERENCE's own ``BlockGen / BackboneGen / NeckGen / Head /
    SODa.forward / SODa._loss`` produced for a description without spiking neurons (``make_golden.py::executor_golden``: every
    file as on disk but two PEP 695 alias statements of ``models/generator.py``).  Same module-tree keys, and - both sides are
    torch CPU kernels behind the same sequence of calls - the same bits: predictions, loss, every gradient, the BatchNorm
    buffers, the ConvLSTM state tree of a block threaded through four steps."""
    z = np.load(os.path.join(golden_dir, "executor.npz"))
    keys = [str(k) for k in z["state_keys"]]
    torch.manual_seed(0)
    desc = executor_net(S)(num_classes=int(z["num_classes"]), time_window=0)
    ref = ON.SODaRef(desc, int(z["num_classes"]), loss_ratio=float(z["loss_ratio"]), time_window=0,
                     iou_threshold=float(z["iou_threshold"]))
    assert list(ref.state_dict().keys()) == keys and list(desc.state_dict().keys()) == keys
    ref.load_state_dict({k: torch.from_numpy(z["init/" + k]) for k in keys})
    ref.train()
    X, labels = torch.from_numpy(z["X"]), torch.from_numpy(z["labels"])
    anchors, cls_preds, bbox_preds = ref(X)
    loss = ref._loss((anchors, cls_preds, bbox_preds), labels)
    loss.backward()
    assert torch.equal(anchors, torch.from_numpy(z["anchors"]))
    assert torch.equal(cls_preds.detach(), torch.from_numpy(z["cls_preds"]))
    assert torch.equal(bbox_preds.detach(), torch.from_numpy(z["bbox_preds"]))
    assert float(loss.detach()) == float(z["loss"])
    no_grad = {str(k) for k in z["no_grad"]}
    for k, p in ref.named_parameters():
        if k in no_grad:
            continue
        assert torch.equal(p.grad, torch.from_numpy(z["grad/" + k])), k
    for k, v in ref.state_dict().items():
        if "running_" in k or "num_batches" in k:
            assert torch.equal(v, torch.from_numpy(z["after/" + k])), k
    # training_step with time_window = 16: the same draw from the global generator, the same dropped prefix, the same loss
    ref2 = ON.SODaRef(desc, int(z["num_classes"]), loss_ratio=float(z["loss_ratio"]), time_window=int(z["ts_time_window"]),
                      iou_threshold=float(z["iou_threshold"]))
    ref2.load_state_dict({k: torch.from_numpy(z["init/" + k]) for k in keys})
    ref2.train()
    torch.manual_seed(int(z["ts_seed"]))
    loss2 = ref2.training_step((torch.from_numpy(z["ts_X"]), labels))
    loss2.backward()
    assert float(loss2.detach()) == float(z["ts_loss"])
    assert int(ref2.base_net.net.net[0][1].num_batches_tracked) == int(z["ts_nbt"]) < z["ts_X"].shape[0]
    assert torch.equal(ref2.base_net.net.net[0][0].weight.grad, torch.from_numpy(z["ts_grad_first"]))
    # streaming inference (soda.py:202-233): eval mode, frame by frame, state threaded by the caller - same rows, same order
    ref.eval()
    st = None
    with torch.no_grad():
        for t in range(X.shape[0]):
            det, st = ref.predict(X[t, 0], st)
            assert torch.equal(det, torch.from_numpy(z[f"predict_{t}"])), t
    for path in z["predict_state_paths"]:
        node = st
        for i in str(path).split("."):
            node = node[int(i)]
        assert torch.equal(node, torch.from_numpy(z["predict_state/" + str(path)])), path
    # one block with an explicit state tree
    blk = ON.BlockRef(4, executor_block_cfg(S)).eval()
    assert blk.out_channels == int(z["blk_out_channels"])
    blk.load_state_dict({k[4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("blk/")})
    assert json.dumps(blk.branch_state) == str(z["blk_state_mask"])
    xs = torch.from_numpy(z["blk_x"])
    state, ys = None, []
    with torch.no_grad():
        for t in range(xs.shape[0]):
            y, state = blk(xs[t], state)
            ys.append(y)
    assert torch.equal(torch.stack(ys), torch.from_numpy(z["blk_y"]))
    for path in z["blk_state_paths"]:
        node = state
        for i in str(path).split("."):
            node = node[int(i)]
        assert torch.equal(node, torch.from_numpy(z["blk_state/" + str(path)])), path
