"""Host-side checks of the activity monitor: the two C entry points in header, binding and library; the launch plan and
the refusals of ``snn_activity_count`` (nothing here launches); the report arithmetic on hand-made counts; the recorder
switch; and the cross-rank sum of the counts as ONE collective, on CPU tensors over gloo."""
import os
import re
import socket
from ctypes import c_int, c_int64, c_float, c_void_p

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

NEW = ("snn_activity_count", "snn_activity_count_plan")
A = 1 << 20   # a 16-byte aligned "address": the calls below are refused, or host-only, before anything is read


def _header():
    from snn_for_object_detection_amd import _hip
    text = open(os.path.join(os.path.dirname(_hip._HERE), "include", "snn_hip.h")).read()
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_header_binding_and_library_agree(hip_lib):
    from snn_for_object_detection_amd import _build, _hip
    code = _header()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        decls = [d.strip() for d in m.group(1).split(",")]
        restype, argtypes = _hip.SIGNATURES[name]
        assert restype is c_int and len(decls) == len(argtypes), name
        for d, a in zip(decls, argtypes):
            want = c_void_p if "*" in d else {"int": c_int, "int64_t": c_int64, "float": c_float}[d.rsplit(None, 1)[0]]
            assert a is want, (name, d)
        assert hasattr(hip_lib, name)
    for k, sym in enumerate(("NONZERO_F32", "NONZERO_BF16", "ABOVE_F32", "ABOVE_BF16", "MASK")):
        assert re.search(r"SNN_ACT_" + sym + r"\s*=\s*%d\b" % k, code) and getattr(_hip, "ACTIVITY_" + sym) == k
    assert "activity.hip" in _build.SOURCES
    # symbols were only added: the version stays
    assert hip_lib.snn_abi_version() == 20 and _hip.ABI_VERSION == 20
    assert re.search(r"#define\s+SNN_ABI_VERSION\s+20\b", code)


def _plan(lib, kind, T, M, C, ld, aligned):
    out = (c_int64 * 4)()
    assert lib.snn_activity_count_plan(kind, T, M, C, ld, int(aligned), out) == 0, lib.snn_last_error()
    return tuple(out)


@pytest.mark.parametrize("kind", [0, 1, 2, 3])
def test_plan_picks_the_four_channel_instance_only_where_the_call_allows(hip_lib, kind):
    T, M = 6, 1425
    assert _plan(hip_lib, kind, T, M, 64, 64, True)[0] == 4
    assert _plan(hip_lib, kind, T, M, 3, 3, True)[0] == 1        # C % 4
    assert _plan(hip_lib, kind, T, M, 64, 66, True)[0] == 1      # ld % 4
    assert _plan(hip_lib, kind, T, M, 64, 64, False)[0] == 1     # the pointer
    assert _plan(hip_lib, kind, T, M, 64, 80, True)[0] == 4      # a channel slice of wider rows


def test_plan_covers_every_row_once(hip_lib):
    for kind, C, ld in ((0, 64, 64), (0, 3, 3), (2, 512, 528), (1, 24, 24), (4, 32, 2), (4, 96, 3), (4, 512, 17)):
        for T in (1, 6):
            for M in (1, 63, 64, 65, 315, 1425, 5 * 120 * 152):
                vec, rows, gx, gy = _plan(hip_lib, kind, T, M, C, ld, True)
                assert vec == (32 if kind == 4 else (4 if C % 4 == 0 else 1))
                assert rows >= 1 and gx >= 1 and (gx - 1) * rows < M <= gx * rows     # every pixel row in exactly one block
                assert gy >= T and gy % T == 0                                        # timesteps x channel chunks
    # a large map spreads over the chip; a tiny one stays in one block
    vec, rows, gx, gy = _plan(hip_lib, 2, 32, 5 * 120 * 152, 64, 64, True)
    assert gx * gy >= 128 and gy == 32
    assert _plan(hip_lib, 2, 1, 63, 64, 64, True)[2] == 1


def _refused(lib, rc, *words):
    msg = lib.snn_last_error().decode()
    assert rc != 0 and all(w in msg for w in words), (rc, msg)


def test_refusals_name_the_entry_point_and_the_reason(hip_lib):
    count, plan = hip_lib.snn_activity_count, hip_lib.snn_activity_count_plan
    out = (c_int64 * 4)()
    fn, pn = "snn_activity_count:", "snn_activity_count_plan:"
    _refused(hip_lib, count(A, 5, 64, 0.0, 1, 8, 64, 0, A, 0, None), fn, "unknown kind 5")
    _refused(hip_lib, count(A, -1, 64, 0.0, 1, 8, 64, 0, A, 0, None), fn, "unknown kind -1")
    _refused(hip_lib, plan(7, 1, 8, 64, 64, 1, out), pn, "unknown kind 7")
    for T, M, C in ((0, 8, 64), (1, 0, 64), (1, 8, 0), (-1, 8, 64), (1, -8, 64), (1, 8, -64)):
        _refused(hip_lib, count(A, 0, 64, 0.0, T, M, C, 0, A, 0, None), fn, "non-positive shape")
        _refused(hip_lib, plan(0, T, M, C, 64, 1, out), pn, "non-positive shape")
    _refused(hip_lib, count(A, 2, 63, 1.0, 1, 8, 64, 0, A, 0, None), fn, "ld too small")
    _refused(hip_lib, count(A, 4, 1, 0.0, 1, 8, 64, 0, A, 0, None), fn, "ld too small")      # a mask: words
    _refused(hip_lib, plan(4, 1, 8, 96, 2, 1, out), pn, "ld too small")
    _refused(hip_lib, count(A, 4, 2, 0.0, 1, 8, 48, 0, A, 0, None), fn, "C % 32 != 0")
    _refused(hip_lib, plan(4, 1, 8, 48, 2, 1, out), pn, "C % 32 != 0")
    _refused(hip_lib, count(None, 0, 64, 0.0, 1, 8, 64, 0, A, 0, None), fn, "null pointer")
    _refused(hip_lib, count(A, 0, 64, 0.0, 1, 8, 64, 0, None, 0, None), fn, "null pointer")
    _refused(hip_lib, plan(0, 1, 8, 64, 64, 1, None), pn, "null pointer")


def test_spike_count_has_no_cpu_fallback():
    from snn_for_object_detection_amd import functional as HF
    x = torch.zeros(2, 1, 3, 3, 4).permute(0, 1, 4, 2, 3)   # channels-last [T,B,C,H,W], on the CPU
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.spike_count(x)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        HF.spike_count(None, mask=torch.zeros(2, 1, 3, 3, 1, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------------- report
def test_report_arithmetic_on_hand_made_counts():
    from snn_for_object_detection_amd import activity
    # layer a: 4 channels, 50 neuron-timesteps each: one dead, one saturated
    a = torch.tensor([0, 50, 10, 25])
    # layer b, per step [T=2, C=3], 20 neuron-timesteps per channel (10 per step): channel 2 fires always, channel 0 never
    b = torch.tensor([[0, 3, 10], [0, 4, 10]])
    lif = {"a": (a, 50), "b": (b, 20)}
    convs = {"c3s2": (120, 1000, 64, 3, 3, 2),    # nonzero, inputs, Cout, KH, KW, stride
             "c1": (85, 260, 32, 1, 1, 1)}
    rep = activity.make_report(lif, convs)
    la, lb = rep["layers"]["a"], rep["layers"]["b"]
    assert la["neurons"] == 50 and la["rate"] == 85 / 200
    assert la["dead_channels"] == [0] and la["saturated_channels"] == [1]
    assert torch.equal(la["channel_rate"], torch.tensor([0.0, 1.0, 0.2, 0.5], dtype=torch.float64))
    assert torch.equal(la["spikes"], a) and la["spikes"].dtype == torch.int64
    assert torch.equal(lb["spikes"], b) and lb["rate"] == 27 / 60
    assert lb["dead_channels"] == [0] and lb["saturated_channels"] == [2]
    c3, c1 = rep["convs"]["c3s2"], rep["convs"]["c1"]
    assert c3["nonzero_inputs"] == 120 and c3["inputs"] == 1000 and c3["density"] == 0.12
    assert c3["synops"] == 120 * 64 * 9 / 4 and c3["macs"] == 1000 * 64 * 9 / 4
    assert c1["synops"] == 85 * 32 and c1["macs"] == 260 * 32 and c1["density"] == 85 / 260
    t = rep["totals"]
    assert t["synops"] == 120 * 144 + 85 * 32 and t["macs"] == 1000 * 144 + 260 * 32
    assert t["spikes"] == 112 and t["neurons"] == 260 and t["rate"] == 112 / 260     # weighted by neurons, not by layer
    assert "a" in activity.format_report(rep)
    empty = activity.make_report({}, {})
    assert empty["totals"] == {"synops": 0.0, "macs": 0.0, "spikes": 0, "neurons": 0, "rate": 0.0}


def test_recorder_is_off_by_default_and_restored_after_an_exception():
    import snn_for_object_detection_amd as S
    from snn_for_object_detection_amd import activity, functional as HF
    assert HF._ACTIVITY is None
    blk = S.BlockGen(2, [S.Conv(8, 3, 2), S.Norm(), S.LIF(), S.Conv(4, 1)])
    with pytest.raises(KeyError):
        with activity.record(blk) as rec:
            assert HF._ACTIVITY is rec and rec.per_step is False
            with activity.record(blk, per_step=True) as inner:     # nests: the outer recorder comes back
                assert HF._ACTIVITY is inner
            assert HF._ACTIVITY is rec
            raise KeyError("inside the block")
    assert HF._ACTIVITY is None
    assert rec.report() == activity.make_report({}, {})            # nothing ran: an empty report, no device needed
    # the recorder knows the LIF cell and the weights by their qualified names
    assert list(rec._cells.values()) == ["net.0.2"]
    assert {"net.0.0.weight", "net.0.3.weight"} <= set(rec._weights.values())


# ---------------------------------------------------------------------------------------------------- two ranks
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from snn_for_object_detection_amd import activity
        g = torch.Generator().manual_seed(5 + rank)
        local = [torch.randint(0, 1 << 40, (6, 8), generator=g), torch.randint(0, 1 << 40, (3,), generator=g),
                 torch.tensor([rank + 1, 7], dtype=torch.int64)]
        calls = []
        real = dist.all_reduce

        def counting(*a, **kw):
            calls.append(1)
            return real(*a, **kw)

        dist.all_reduce = counting
        try:
            summed = activity.all_reduce_counts([t.clone() for t in local], dist.group.WORLD)
        finally:
            dist.all_reduce = real
        torch.save({"local": local, "sum": summed, "calls": len(calls)}, os.path.join(out_dir, f"act{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(120)
def test_counts_are_summed_over_two_ranks_by_one_collective(tmp_path):
    world, port = 2, _free_port()
    mp.spawn(_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = (torch.load(tmp_path / f"act{r}.pt") for r in range(world))
    assert r0["calls"] == 1 and r1["calls"] == 1
    for k in range(3):
        want = r0["local"][k] + r1["local"][k]
        assert r0["sum"][k].shape == want.shape and r0["sum"][k].dtype == torch.int64
        assert torch.equal(r0["sum"][k], want) and torch.equal(r1["sum"][k], want)
