"""CPU-side checks: description API, module-tree / state_dict layout, C-ABI symbol export, build."""
import ctypes
import os
import re

import pytest
import torch

import snn_for_object_detection_amd as S
from oracle.net import SODaRef
from tests.fp64_buffers import GATHER_KEYS, WGRAD_PLAN_KEYS


def test_tiny_yolo_structure_and_param_count():
    m = S.TinyYolo(num_classes=2, time_window=0)
    assert sum(p.numel() for p in m.parameters() if p.requires_grad) == 4_228_544
    kinds = [type(x).__name__ for x in m.modules()]
    assert kinds.count("HipConv2d") == 48 and kinds.count("HipBatchNorm2d") == 22
    assert kinds.count("LIFCell") == 19 and kinds.count("LICell") == 3 and kinds.count("Storage") == 3
    assert m.neck_net.out_shape == [256, 256, 256]
    m7 = S.TinyYolo(num_classes=7, time_window=0)
    assert sum(p.numel() for p in m7.parameters() if p.requires_grad) == 4_263_104


def test_state_dict_layout_is_the_reference_layout():
    m = S.TinyYolo(num_classes=2)
    keys = list(m.state_dict().keys())
    assert keys[0] == "base_net.net.net.0.0.weight"                    # ModuleList nesting, generator.py:115,143
    assert "base_net.net.net.0.1.running_mean" in keys and "base_net.net.net.0.1.bias" not in keys
    assert "head_net.model_0.base_net.net.0.0.net.0.0.weight" in keys  # generator.py:403-413,522-525
    assert "head_net.anchor_gen_2.sizes" in keys
    ref = SODaRef(m, 2)
    assert list(ref.state_dict().keys()) == keys                       # oracle and product interchange weights
    ref.load_state_dict(m.state_dict())
    w = m.base_net.net.net[0][0].weight
    assert w.shape == (64, 2, 3, 3) and w.permute(0, 2, 3, 1).is_contiguous()   # OHWI storage for the kernels


def test_block_state_tree_and_fusion_plan():
    blk = S.BlockGen(4, [S.Conv(8), S.Norm(), S.LIF(), S.Dense([[S.Conv(8, 1), S.Norm(), S.LI(), S.Tanh()], [S.Pass()]])])
    assert blk.out_channels == 16
    assert blk.branch_state == [[False, False, True, True]]
    assert blk._plan[0] == [("layer", 0, 1), ("norm_neuron", 1, 2), ("layer", 3, 1)]
    inner = blk.net[0][3]
    assert inner.merge == "dense" and inner._plan[0] == [("layer", 0, 1), ("norm_neuron", 1, 3)]
    with pytest.raises(RuntimeError):
        S.BlockGen(4, S.Residual([[S.Conv(8, 1)], [S.Conv(6, 1)]]))
    with pytest.raises(ValueError):
        S.Pool("Q")
    with pytest.raises(NotImplementedError):
        S.SODa(num_classes=2)


def test_product_refuses_cpu_tensors():
    m = S.TinyYolo(num_classes=2, time_window=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.zeros(2, 1, 2, 32, 48))


def test_c_abi_exports_every_declared_symbol(hip_lib):
    from snn_for_object_detection_amd import _hip
    header = open(os.path.join(os.path.dirname(_hip._HERE), "include", "snn_hip.h")).read()
    declared = set(re.findall(r"\b(snn_[a-z0-9_]+)\s*\(", header))
    declared.discard("snn_neuron_params")
    assert declared == set(_hip.SIGNATURES), declared ^ set(_hip.SIGNATURES)
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name in declared:
        assert hasattr(raw, name), name
    assert hip_lib.snn_abi_version() == _hip.ABI_VERSION
    # shape planning helpers are host-only and callable without a GPU
    assert hip_lib.snn_conv2d_wgrad_splitk(160, 120, 152, 32, 120, 152, 32, 3, 3, 1, 1, _hip.PREC_BF16X3) >= 1
    assert hip_lib.snn_bn_stats_partial_size(32, 5 * 120 * 152, 64) > 0
    assert hip_lib.snn_affine_neuron_bwd_sums_size(32, 5 * 120 * 152, 64) > 0
    # partials a forward convolution leaves for the BatchNorm behind it: bound over the three producing kernels
    n = hip_lib.snn_conv2d_fwd_bn_partial_size(160, 5, 120, 152, 64)
    assert n >= 32 * (5 * 120 * 152 // 128 + 1) * 64 * 2           # >= the implicit-GEMM layout (128-row tiles)
    assert n >= 32 * hip_lib.snn_conv3x3_halo_bn_chunks(5, 120, 152) * 64 * 2   # >= the halo-resident layout (4 x 32 rectangles)
    assert hip_lib.snn_conv2d_fwd_bn_partial_size(160, 7, 120, 152, 64) == 0   # frames per step must divide N
    # ... and the halo-resident 3x3 kernel's layout (strip tiles of 128 cells per timestep), where that kernel applies
    assert hip_lib.snn_conv3x3_halo_supported(160, 30, 38, 128, 128) == 1
    assert hip_lib.snn_conv3x3_halo_supported(160, 120, 152, 64, 64) == 1      # long rows: 4 x 32 rectangles
    assert hip_lib.snn_conv3x3_halo_bn_chunks(5, 120, 152) == 5 * 30 * 5
    assert hip_lib.snn_conv3x3_halo_supported(160, 30, 38, 128, 32) == 1       # the 32-channel tile
    assert hip_lib.snn_conv3x3_halo_supported(160, 30, 38, 128, 96) == 0       # channel tiles: 32, or multiples of 64
    assert hip_lib.snn_conv3x3_halo_bn_chunks(5, 30, 38) == (5 * 31 * 39 + 127) // 128
    assert hip_lib.snn_conv2d_fwd_bn_partial_size(160, 5, 30, 38, 128) >= 32 * hip_lib.snn_conv3x3_halo_bn_chunks(5, 30, 38) * 128 * 2
    assert hip_lib.snn_weight_frag_image_bytes(128, 64) == 9 * 128 * 64 * 4
    # the reverse scan that rebuilds the BatchNorm statistic from the saved state: LIF, ordered-sums plans, fp32, all steps
    from snn_for_object_detection_amd import functional as HF
    prm = HF.neuron_params()
    q = hip_lib.snn_affine_neuron_bwd_sums_from_state
    assert q(_hip.NEURON_LIF, 32, 5 * 120 * 152, 64, 64, prm, 0) == 1
    assert q(_hip.NEURON_LIF, 32, 5 * 120 * 152, 64, 128, prm, 0) == 1                    # g_out as a slice of a wider buffer
    assert q(_hip.NEURON_LI, 32, 5 * 120 * 152, 64, 64, prm, 0) == 0                       # LIF only
    assert q(_hip.NEURON_LIF, 32, 5 * 120 * 152, 64, 64, prm, _hip.SCAN_LAST_STEP_ONLY) == 0
    assert q(_hip.NEURON_LIF, 32, 5 * 120 * 152, 64, 64, prm, _hip.SCAN_BF16_STORAGE) == 0  # a bf16 potential does not determine the input
    assert q(_hip.NEURON_LIF, 32, 5 * 120 * 152, 24, 24, prm, 0) == 0                       # 6 channel quads: the LDS-atomics plan
    assert q(_hip.NEURON_LIF, 32, 40_000_000, 64, 64, prm, 0) == 0                         # a timestep beyond the 31-bit buffer offsets


def test_ctypes_signatures_agree_with_the_header():
    """Every prototype of include/snn_hip.h, parameter by parameter, against the ctypes signature the product calls it
    with (a missing or mistyped argument would otherwise hand the kernels garbage without any error)."""
    from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int64, c_size_t, c_void_p
    from snn_for_object_detection_amd import _hip
    header = open(os.path.join(os.path.dirname(_hip._HERE), "include", "snn_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    protos = re.findall(r"\b(int64_t|int|size_t|const char\s*\*)\s+(snn_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", header)
    assert len(protos) == len(_hip.SIGNATURES), (len(protos), len(_hip.SIGNATURES))

    def ctype_of(decl):
        decl = decl.strip()
        if "*" in decl:
            return POINTER(_hip.NeuronParams) if "snn_neuron_params" in decl else c_void_p
        base = decl.rsplit(None, 1)[0].replace("const ", "").strip()   # drop the parameter name
        return {"int": c_int, "int64_t": c_int64, "float": c_float, "double": c_double, "size_t": c_size_t}[base]

    for ret, name, params in protos:
        restype, argtypes = _hip.SIGNATURES[name]
        want_ret = {"int": c_int, "size_t": c_size_t, "int64_t": c_int64}.get(ret, c_char_p)
        assert restype is want_ret, (name, restype, want_ret)
        decls = [] if params.strip() in ("", "void") else params.split(",")
        assert len(decls) == len(argtypes), (name, len(decls), len(argtypes))
        for k, (d, a) in enumerate(zip(decls, argtypes)):
            assert ctype_of(d) is a, (name, k, d.strip(), a)


def test_build_lists_every_kernel_source_and_header():
    """The build compiles exactly the ``csrc/*.hip`` files, and every ``csrc/*.h`` is part of each object's cache key
    (a forgotten source fails at link time, a forgotten header leaves stale objects behind).  Needs no library."""
    from snn_for_object_detection_amd import _build
    on_disk = os.listdir(_build.CSRC)
    assert {n for n in on_disk if n.endswith(".hip")} == set(_build.SOURCES)
    assert len(_build.SOURCES) == len(set(_build.SOURCES))
    keyed = {os.path.realpath(h) for h in _build.headers()}
    for name in on_disk:
        if name.endswith(".h"):
            assert os.path.realpath(os.path.join(_build.CSRC, name)) in keyed, name
    assert os.path.realpath(os.path.join(_build.INCLUDE, "snn_hip.h")) in keyed
    assert 1 <= _build.MAX_WORKERS <= 8


def test_neuron_constants_match_oracle():
    from oracle.neurons import neuron_constants
    p = S.functional.neuron_params()
    assert (p.c_mem, p.c_syn, p.v_leak, p.v_th, p.v_reset, p.alpha) == tuple(
        torch.tensor(neuron_constants(), dtype=torch.float32).tolist())


def test_oracle_event_voxelisation_known_answers():
    """oracle/events.py restates utils/datasets.py:403-435 / :127-135 (not importable: prophesee_toolbox is absent);
    hand-checked cases pin it: binning, the t >= t0 filter, x clipping, flag-not-count, -1 label padding."""
    import numpy as np
    from oracle import events as OE
    t = np.array([1000, 1999, 2000, 5999, 6000, 999, 2500, 2500], dtype=np.int64)
    x = np.array([0, 3, 9, 2, 1, 1, 3, 3], dtype=np.int64)      # x = 9 lies outside a 6-wide frame: clipped to 5
    y = np.array([0, 1, 2, 3, 0, 0, 1, 1], dtype=np.int64)
    p = np.array([1, 0, 1, 0, 1, 1, 0, 0], dtype=np.int64)
    f = OE.voxelize(t, x, y, p, t0_us=1000, time_step_us=1000, num_steps=5, height=4, width=6)
    assert f.shape == (5, 2, 4, 6) and f.sum() == 5
    assert f[0, 1, 0, 0] == 1 and f[0, 0, 1, 3] == 1             # t = 1000 and 1999 -> bin 0
    assert f[1, 1, 2, 5] == 1                                     # t = 2000 -> bin 1, x clipped 9 -> 5
    assert f[4, 0, 3, 2] == 1                                     # t = 5999 -> bin 4
    assert f[1, 0, 1, 3] == 1                                     # the duplicate event is a flag, not a count
    # t = 6000 is past the 5-step window, t = 999 precedes t0: both dropped
    a = (f, np.array([[0, .1, .1, .5, .5]], dtype=np.float32))
    b = (f * 0, np.array([[1, .2, .2, .6, .6], [0, .3, .3, .9, .9]], dtype=np.float32))
    X, lab = OE.stack_batch([a, b])
    assert X.shape == (5, 2, 2, 4, 6) and (X[:, 0] == f).all() and X[:, 1].sum() == 0
    assert lab.shape == (2, 2, 5) and (lab[0, 1] == -1).all() and lab[1, 1, 0] == 0


def test_unbounded_activation_status_reaches_every_convolution_it_feeds():
    """fp16x3 (default forward arithmetic) needs |x| < 4094.  A convolution takes the any-range bf16x6 arithmetic whenever
    its input is not provably bounded - not only right behind ReLU / SiLU / SumPool / ConvLSTM (the previous rule looked at
    the preceding sibling only) but through convolutions, nested blocks, Residual / Dense merges and passes, until a
    BatchNorm, a spiking neuron or a Tanh bounds it again."""
    from snn_for_object_detection_amd import BlockGen, Conv, Dense, LIF, Norm, Pass, Pool, ReLU, Residual, Tanh

    def precisions(cfg, cin=4):
        blk = BlockGen(cin, cfg)
        return [m.forward_precision for m in blk.modules() if isinstance(m, torch.nn.Conv2d)], blk

    p, blk = precisions([Conv(8, 3), ReLU(), Conv(8, 1)])
    assert p == [None, "bf16x6"] and blk.out_unbounded                       # conv keeps the status of its input
    p, _ = precisions([Conv(8, 3), ReLU(), [Conv(8, 1)], Conv(4, 1)])
    assert p == [None, "bf16x6", "bf16x6"]                                   # into a nested block and out of it again
    p, blk = precisions([Conv(8, 3), Residual([[Conv(8, 3), ReLU()], [Pass()]]), Conv(4, 1)])
    assert p == [None, None, "bf16x6"]                                       # one unbounded branch tail taints the sum
    p, blk = precisions([Conv(8, 3), Dense([[Conv(8, 3), Norm(), LIF()], [Pass()]]), Conv(4, 1)])
    assert p == [None, None, None] and not blk.out_unbounded                 # spikes + a bounded pass-through
    p, blk = precisions([Conv(8, 3), ReLU(), Pool("S"), Conv(8, 3), Norm(), Conv(8, 1), Tanh()])
    assert p == [None, "bf16x6", None] and not blk.out_unbounded             # BatchNorm bounds it again
    p, _ = precisions([Conv(8, 3), ReLU(), Conv(8, 1, 1)], cin=4)
    from snn_for_object_detection_amd.layer_gen import Conv as ConvGen
    gen = ConvGen(8, 1)
    assert getattr(gen, "forward_precision", None) is None                   # an explicit setting is respected
    m = S.TinyYolo(num_classes=2, time_window=0)
    assert all(c.forward_precision is None for c in m.modules() if isinstance(c, torch.nn.Conv2d))


def test_profiler_byte_model_of_both_storage_modes():
    """bench.py's per-launch work model (profiler.work_of): activation tensors count 4 bytes per element, 2 in the bf16-storage
    mode (weights and weight gradients stay fp32; the event frames stay fp32), last-step-only scans write one step, and the
    labels of the bf16 instances carry the suffix bench.py keys the bf16 MFMA peak on."""
    from snn_for_object_detection_amd.profiler import work_of
    N, H, W, Cin, Cout = 160, 30, 38, 128, 128
    px = N * H * W
    # snn_conv3x3_halo(x, ldx, img, y, ldy, N, H, W, Cin, Cout, add, ld, add2, ld2, partial, fps, layout, precision, stream)
    base = [1, Cin, 2, 3, Cout, N, H, W, Cin, Cout, None, 0, None, 0, None, 0, None]
    l32, f32, b32 = work_of("snn_conv3x3_halo", base + [4, 0])
    l16, f16, b16 = work_of("snn_conv3x3_halo", base + [6, 0])
    assert l32 == "k_conv_halo3<128, fwd>" and l16 == "k_conv_halo3<128, bf16s>" and f32 == f16 == 2.0 * px * Cout * 9 * Cin
    assert b32 == 4.0 * (2 * px * Cin) + 4.0 * Cout * 9 * Cin and b16 == 2.0 * (2 * px * Cin) + 4.0 * Cout * 9 * Cin
    assert work_of("snn_conv3x3_halo", [1, 32, 2, 3, 32, N, H, W, 32, 32] + base[10:] + [1, 0])[0] == "k_conv_halo3<32, dgrad>"
    # snn_affine_neuron_fwd(neuron, y, ldy, alpha, beta, v0, i0, out, ldo, addend, ld, vT, iT, vdec, T, M, C, params, flags, stream)
    T, M, C = 32, 5700, 128
    scan = [1, 1, C, 2, 3, None, None, 4, C, None, 0, 5, 6, 7, T, M, C, None]
    assert work_of("snn_affine_neuron_fwd", scan + [0, 0])[2] == 4.0 * T * M * C * 3          # y, out, vdec
    assert work_of("snn_affine_neuron_fwd", scan + [4, 0])[2] == 2.0 * T * M * C * 3
    assert work_of("snn_affine_neuron_fwd", scan + [4, 0])[0].endswith(", bf16s")
    assert work_of("snn_affine_neuron_fwd", scan + [2, 0])[2] == 4.0 * T * M * C * (2 + 1.0 / T)   # one step of out
    # the event-frame layer in bf16 storage: fp32 frames in, bf16 out
    # snn_conv2d_fwd(x, ldx, w, w_split, y, ldy, N, H, W, Cin, Ho, Wo, Cout, KH, KW, stride, pad, add, ld, partial, fps, layout, prec, st)
    first = [1, 2, 2, None, 3, 64, N, 240, 304, 2, 240, 304, 64, 3, 3, 1, 1, None, 0, None, 0, None]
    lab, _, byts = work_of("snn_conv2d_fwd", first + [6, 0])
    assert lab.startswith("k_conv_first") and byts == 4.0 * N * 240 * 304 * 2 + 2.0 * N * 240 * 304 * 64 + 4.0 * 64 * 9 * 2
    assert work_of("snn_bn_bwd_apply_bf16", [0] * 8 + [T, M, C])[2] == 6.0 * T * M * C


def test_reverse_scan_plan_invariants(hip_lib):
    """snn_affine_neuron_bwd_plan over a grid of (T, M, C): every plan fits the block, covers every pixel and channel,
    stays inside 64 KiB of LDS, and takes the ordered-slab sums only where the wave combine is defined."""
    from snn_for_object_detection_amd import _hip
    from snn_for_object_detection_amd import functional as HF
    prm = HF.neuron_params()
    seen = set()
    for T in (1, 2, 4, 32, 33, 70, 128):
        for C in (1, 3, 4, 6, 8, 16, 24, 32, 36, 64, 100, 128, 256, 384, 512, 1024):
            for M in (1, 7, 126, 400, 1425, 5700, 22800, 91200, 364800):
                for with_sums in (False, True):
                    pl = HF.affine_neuron_bwd_plan(_hip.NEURON_LIF, T, M, C, C, C, with_sums, 0, prm)
                    P = 256 // pl.cvb
                    assert pl.vec == (4 if C % 4 == 0 else 1)
                    assert 1 <= pl.cvb and pl.cvb * P <= 256 and P >= 1, pl
                    assert pl.gy * pl.cvb >= C // pl.vec and (pl.gy - 1) * pl.cvb < C // pl.vec, pl
                    assert pl.gx * pl.rpb * P >= M and (pl.gx - 1) * pl.rpb * P < M, pl      # no idle pixel block
                    assert pl.partial_row == (1 if M % P else 0)
                    assert pl.mode == (0 if not with_sums else (1 if pl.mode == 1 else 2))
                    if pl.mode == 1:
                        assert (pl.cvb & (pl.cvb - 1)) == 0 or pl.cvb >= 64, pl
                    slabs = {0: 0, 1: 4, 2: 1}[pl.mode]
                    assert pl.lds_bytes == slabs * T * pl.cvb * pl.vec * 2 * 4 and pl.lds_bytes <= 64 * 1024, pl
                    assert pl.np == (1 if (pl.buf and pl.rpb == 1) else 4), pl
                    assert pl.buf == (1 if pl.vec == 4 and M * C * 4 < 2 ** 31 - 1 else 0), pl
                    if with_sums:
                        assert hip_lib.snn_affine_neuron_bwd_sums_size(T, M, C) == pl.gx * T * C * 2
                    seen.add((pl.vec, pl.mode, pl.np, pl.gy > 1, pl.partial_row))
    assert {(4, 1, 4, True, 1), (4, 1, 1, True, 1), (1, 2, 4, False, 1), (4, 2, 1, False, 1), (4, 0, 4, False, 0)} <= seen
    # the forced 64-bit addressing takes the branchy instance; the y-free sums take 1 / 2 / 3 pixel rows per thread
    assert HF.affine_neuron_bwd_plan(_hip.NEURON_LIF, 32, 1425, 256, 256, 256, True, _hip.SCAN_WIDE_ADDRESSING).buf == 0
    assert HF.affine_neuron_bwd_plan(_hip.NEURON_LIF, 32, 1425, 256, 256, 256, True, _hip.SCAN_WIDE_ADDRESSING).np == 4
    for M in (1425, 5700, 22800, 91200):
        pl = HF.affine_neuron_bwd_plan(_hip.NEURON_LIF, 32, M, 128, 128, 128, True, _hip.SCAN_SUMS_FROM_STATE)
        assert pl.buf == 1 and pl.np == min(pl.rpb, 3), (M, pl)
    with pytest.raises(RuntimeError, match="SNN_SCAN_SUMS_FROM_STATE not covered"):
        HF.affine_neuron_bwd_plan(_hip.NEURON_LI, 32, 5700, 256, 256, 256, True, _hip.SCAN_SUMS_FROM_STATE)
    with pytest.raises(RuntimeError, match="bad shape"):
        HF.affine_neuron_bwd_plan(_hip.NEURON_LIF, 32, 5700, 256, 128, 256, True)


def test_halo_plan_invariants(hip_lib):
    """The host-only plan queries of the halo-resident kernels over a grid of shapes: the launch geometry covers every tile
    in whole XCD groups, the mode boundaries sit where the LDS halo stops fitting, and the weight-gradient patches fit the
    staged halo, cover the output and are owned by the splits."""
    from ctypes import addressof, c_int

    def plan(name, n, *args):
        out = (c_int * n)()
        rc = getattr(hip_lib, name)(*args, addressof(out))
        return rc, list(out)

    for N, H, W in ((1, 1, 1), (3, 7, 5), (2, 9, 78), (2, 9, 79), (6, 30, 38), (4, 120, 152), (2, 1, 300)):
        for Cin, Cout in ((32, 32), (64, 64), (32, 128), (128, 256), (64, 192)):
            for fps in (0, 1, N):
                rc, (mode, co, tiles, tpg, tpx, cot, blocks) = plan("snn_conv3x3_halo_plan", 7, N, H, W, Cin, Cout, fps)
                assert rc == 0 and mode == (1 if W <= 78 else 2), (N, H, W, fps)        # W = 78 strip, W = 79 RECT
                assert co == (128 if Cout % 128 == 0 else 64 if Cout % 64 == 0 else 32) and cot * co == Cout
                G = fps or N
                if mode == 1:
                    assert tpg == -(-G * (H + 1) * (W + 1) // 128)                      # 128-cell tiles of a group
                else:
                    assert tpg == G * -(-H // 4) * -(-W // 32)                          # 4 x 32 rectangles
                assert tiles == N // G * tpg and tpx == -(-tiles // 8) and blocks == 8 * tpx * cot
                if fps:
                    assert tpg == hip_lib.snn_conv3x3_halo_bn_chunks(G, H, W)
    assert plan("snn_conv3x3_halo_plan", 7, 4, 8, 8, 64, 96, 0)[0] == 1                  # channel tile not covered
    assert plan("snn_conv3x3_halo_plan", 7, 6, 8, 8, 64, 64, 4)[0] == 1                  # frames per step must divide N
    # stride-2 data gradient: strip tiles while the tile and the PW + 1 cells behind it fit the 288 staged cells
    for Wo, mode in ((1, 1), (155, 1), (157, 1), (158, 2), (321, 2)):
        for W in (2 * Wo - 1, 2 * Wo):
            for H in (1, 13, 14):
                Ho = (H - 1) // 2 + 1
                rc, (m, co, tiles, tpg, tpx, cot, blocks) = plan("snn_conv3x3_s2_dgrad_plan", 7, 2, H, W, 128, Ho, Wo, 32)
                assert rc == 0 and m == mode and co == 64 and cot == 2 and blocks == 8 * tpx * cot, (H, W)
                assert (m == 1) == (128 + Wo + 3 <= 288)
                assert tiles == (-(-2 * (Ho + 1) * (Wo + 1) // 128) if m == 1 else 2 * -(-Ho // 4) * -(-Wo // 32))
    # weight gradient: R x CW patches whose ((R-1)s+3) x ((CW-1)s+3) halo fits the 256 staged pixels
    keys = "ok R CW wco wk nks npr npc patches splits pps HR HC HWD tiles_co tiles_ci".split()
    seen = set()
    for s in (1, 2):
        for N, Ho, Wo in ((1, 300, 500), (2, 250, 301), (1, 61, 2459), (1, 60, 2500), (3, 390, 161), (1, 296, 517),
                          (4, 120, 152), (1, 8, 18750), (160, 30, 38)):
            H, W = (Ho, Wo) if s == 1 else (2 * Ho, 2 * Wo - 1)
            for Cin, Cout in ((32, 32), (32, 64), (64, 128), (512, 512)):
                for num_cu in (256, 80, 8):
                    rc, v = plan("snn_conv2d_wgrad_halo_plan", 16, N, H, W, Cin, Ho, Wo, Cout, s, num_cu)
                    p = dict(zip(keys, v))
                    assert rc == 0 and p["ok"] == (1 if N * Ho * Wo >= 150_000 else 0), (N, Ho, Wo, p)
                    if not p["ok"]:
                        continue
                    assert p["CW"] % 8 == 0 and p["HR"] == (p["R"] - 1) * s + 3 and p["HC"] == (p["CW"] - 1) * s + 3
                    assert p["HR"] * p["HWD"] <= 256 and p["HWD"] >= p["HC"], p                     # HALO_CAP
                    assert p["npr"] == -(-Ho // p["R"]) and p["npc"] == -(-Wo // p["CW"]), p      # patches cover Ho x Wo
                    assert p["patches"] == N * p["npr"] * p["npc"] and p["nks"] == -(-p["R"] * p["CW"] // 16)
                    assert p["wco"] == (4 if Cout >= 128 else 2 if Cout >= 64 else 1) and p["wco"] * p["wk"] == 4
                    assert p["tiles_co"] == Cout // (32 * p["wco"]) and p["tiles_ci"] == Cin // 32
                    assert 1 <= p["splits"] <= p["patches"] and p["pps"] == -(-p["patches"] // p["splits"])
                    assert p["splits"] * p["pps"] >= p["patches"] and (p["splits"] < 16 or p["splits"] % 8 == 0), p
                    assert p["splits"] <= max(1, 2 * num_cu // (p["tiles_co"] * p["tiles_ci"])), p
                    seen.add(("splits1", num_cu) if p["splits"] == 1 else ("idle", num_cu)
                             if (p["splits"] - 1) * p["pps"] >= p["patches"] else ("full", num_cu))
                    seen.add("masked_k" if p["R"] * p["CW"] % 16 else "whole_k")
                    if p["nks"] % p["wk"]:
                        seen.add("nks_wk")
                    if num_cu == 256 and not torch.cuda.is_available():   # no device: 0 plans for 256 CUs
                        assert plan("snn_conv2d_wgrad_halo_plan", 16, N, H, W, Cin, Ho, Wo, Cout, s, 0)[1] == v
    # splits owning no patch occur at 256 CUs; a single split only with few CUs per channel tile
    assert {("idle", 256), ("splits1", 8), "masked_k", "whole_k", "nks_wk"} <= seen, seen
    assert ("splits1", 256) not in seen


def test_first_layer_plan_invariants(hip_lib):
    """The host-only plan query of the event-frame row kernel (k_conv_first): staged rows per barrier pair at the LDS
    boundaries, the shapes it takes, the grid of each launch and the statistics groups (one timestep each)."""
    from ctypes import addressof, c_int

    def plan(N, H, W, Cout, s, pad, fps=0, wgrad=0, num_cu=256):
        Ho, Wo = (H + 2 * pad - 3) // s + 1, (W + 2 * pad - 3) // s + 1
        out = (c_int * 10)()
        rc = hip_lib.snn_conv_first_plan(N, H, W, Ho, Wo, Cout, s, pad, fps, wgrad, num_cu, addressof(out))
        keys = "ok rs LW cgs PP blocks group_rows group_blocks max_rows last_stage".split()
        p = dict(zip(keys, out))
        assert rc == (0 if p["ok"] else 1), p
        return p

    # rs = floor(20 KiB / (24 LW)) clamped to 1..4: 4 up to LW 213, 3 to 284, 2 to 426, 1 to 853, then clamped 1 to 1408
    for LW, rs in ((213, 4), (214, 3), (284, 3), (285, 2), (426, 2), (427, 1), (853, 1), (854, 1), (1408, 1)):
        assert (20 << 10) // (24 * LW) == (rs if LW < 854 else 0), LW
        for pad in (0, 1):
            p = plan(2, 5, LW - 2 * pad, 16, 1, pad)
            assert p["ok"] == 1 and p["rs"] == rs and p["LW"] == LW, (LW, pad, p)
    assert plan(2, 5, 1406, 16, 1, 1)["ok"] == 1 and plan(2, 5, 1407, 16, 1, 1)["ok"] == 0     # LW 1408 / 1409
    assert plan(2, 5, 1408, 16, 2, 0)["ok"] == 1 and plan(2, 5, 1409, 16, 2, 0)["ok"] == 0
    for Cout in (4, 8, 16, 32, 64, 128, 256):
        p = plan(2, 5, 9, Cout, 1, 1)
        assert p["ok"] == 1 and p["cgs"] == Cout // 4 and p["PP"] == 256 // (Cout // 4), (Cout, p)
    for Cout in (2, 12, 20, 48, 96, 192, 260, 512):                                            # not 4 * 2^k <= 256
        assert plan(2, 5, 9, Cout, 1, 1)["ok"] == 0, Cout
    out = (c_int * 10)()                                                                         # Ho / Wo must match
    assert hip_lib.snn_conv_first_plan(2, 5, 9, 5, 8, 16, 1, 1, 0, 0, 256, addressof(out)) == 1 and out[0] == 0
    assert plan(6, 5, 9, 16, 1, 1, fps=4)["ok"] == 0                                             # fps must divide N
    seen = set()
    for num_cu in (256, 80, 8):
        for N, H, W, s, pad in ((1, 3, 3, 1, 0), (3, 17, 23, 2, 1), (160, 240, 304, 2, 1), (8, 720, 1280, 2, 1),
                                (4, 9, 1406, 1, 1), (600, 4, 6, 1, 1), (2, 1500, 40, 1, 0), (64, 30, 38, 2, 1)):
            Ho = (H + 2 * pad - 3) // s + 1
            rows = N * Ho
            for Cout in (4, 64, 256):
                p = plan(N, H, W, Cout, s, pad, num_cu=num_cu)                                   # forward
                assert p["blocks"] == p["group_blocks"] == min(rows, 8 * num_cu) and p["group_rows"] == rows, p
                m = -(-rows // p["blocks"])
                assert p["max_rows"] == m and p["last_stage"] == (m - 1) % p["rs"] + 1, p
                seen.add("multi_row" if m > 1 else "one_row")
                if m > 1 and p["last_stage"] < p["rs"]:
                    seen.add("partial_stage")
                w = plan(N, H, W, Cout, s, pad, wgrad=1, num_cu=num_cu)                          # weight gradient
                assert w["blocks"] == w["group_blocks"] == min(rows, 4 * num_cu) and w["max_rows"] == -(-rows // w["blocks"])
                assert w["rs"] == p["rs"] and w["LW"] == p["LW"]
                if num_cu == 256 and not torch.cuda.is_available():   # no device: snn_conv2d_wgrad_splitk plans 256 CUs
                    Wo = (W + 2 * pad - 3) // s + 1
                    assert w["blocks"] == hip_lib.snn_conv2d_wgrad_splitk(N, H, W, 2, Ho, Wo, Cout, 3, 3, s, pad, 0)
                    assert plan(N, H, W, Cout, s, pad, wgrad=1, num_cu=0) == w
                for fps in {1, N} | ({N // 2} if N % 2 == 0 else set()):                        # statistics groups
                    b = plan(N, H, W, Cout, s, pad, fps=fps, num_cu=num_cu)
                    steps, rps = N // fps, fps * Ho
                    target = min(max(8 * num_cu // steps, 1), rps)
                    per = -(-rps // target)
                    assert b["group_rows"] == rps and b["group_blocks"] == -(-rps // per), b
                    assert b["blocks"] == steps * b["group_blocks"] and b["max_rows"] == per, b
                    assert (b["group_blocks"] - 1) * per < rps <= b["group_blocks"] * per     # the last block is short
                    seen.add("target1" if 8 * num_cu // steps < 1 else "per_block" if per > 1 else "row_per_block")
    assert {"multi_row", "one_row", "partial_stage", "target1", "per_block", "row_per_block"} <= seen, seen
    # the three workloads' event-frame layers (Cout 64, pad 1) at 256 CUs
    g = plan(160, 240, 304, 64, 2, 1)                                                            # GEN1
    assert (g["rs"], g["LW"], g["PP"], g["blocks"], g["max_rows"]) == (2, 306, 16, 2048, 10), g
    assert plan(160, 240, 304, 64, 2, 1, wgrad=1)["blocks"] == 1024
    m = plan(256, 720, 1280, 64, 2, 1)                                                           # 1 Mpx
    assert (m["rs"], m["LW"], m["blocks"], m["max_rows"], m["last_stage"]) == (1, 1282, 2048, 45, 1), m
    d = plan(256, 240, 304, 64, 1, 1, fps=2)                                                     # deep-12, T = 128
    assert (d["rs"], d["group_rows"], d["group_blocks"], d["blocks"], d["max_rows"]) == (2, 480, 16, 2048, 30), d


# ---------------------------------------------------------------------------------------------------- implicit GEMM plans
ALL_ALIGNED = 1023


def gather_plan(lib, mode, N, H, W, Cin, Cout, KH, KW, s, pad, prec, *, phase=0, fps=0, align=ALL_ALIGNED, ld_in=None,
                ld_out=None, split=0, add=0, add2=0):
    """snn_conv2d_gather_plan as a dict (mode 0 forward, 1 data-gradient phase, 2 forward over spikes); None: refused."""
    from ctypes import addressof, c_int
    Ho, Wo = (H + 2 * pad - KH) // s + 1, (W + 2 * pad - KW) // s + 1
    ci, co = (Cout, Cin) if mode == 1 else (Cin, Cout)                    # channels of the gathered / produced tensor
    out = (c_int * 17)()
    rc = lib.snn_conv2d_gather_plan(mode, N, H, W, Cin, Ho, Wo, Cout, KH, KW, s, pad, ld_in or ci, ld_out or co, align, split,
                                    add, add2, fps, prec, phase, addressof(out))
    assert rc == (0 if out[0] else 1)
    return dict(zip(GATHER_KEYS, out)) if rc == 0 else None


def wgrad_plan(lib, N, H, W, Cin, Cout, KH, KW, s, pad, prec, num_cu, *, align=ALL_ALIGNED, ldx=None, lddy=None, spikes=0):
    """snn_conv2d_wgrad_plan as a dict; None: refused."""
    from ctypes import addressof, c_int
    Ho, Wo = (H + 2 * pad - KH) // s + 1, (W + 2 * pad - KW) // s + 1
    out = (c_int * 18)()
    rc = lib.snn_conv2d_wgrad_plan(N, H, W, Cin, Ho, Wo, Cout, KH, KW, s, pad, ldx or Cin, lddy or Cout, align, prec, spikes,
                                   num_cu, addressof(out))
    assert rc == (0 if out[0] else 1)
    return dict(zip(WGRAD_PLAN_KEYS, out)) if rc == 0 else None


def _model_conv_layers(H, W, deep12=False):
    """(Cin, Cout, k, stride, pad, H, W) of every convolution of TinyYolo (deep12: of the twelve-layer backbone config) on
    an H x W frame, read off the model: the CPU reference runs one frame of the product's own description with a hook on
    each convolution."""
    if deep12:
        from oracle.net import BlockRef
        ref = BlockRef(2, [layer for _ in range(12) for layer in (S.Conv(64, 3), S.Norm(), S.LIF())]).eval()
    else:
        ref = SODaRef(S.TinyYolo(num_classes=2, time_window=0), 2).eval()
    rows = []

    def hook(mod, inp, out):
        rows.append((mod.in_channels, mod.out_channels, mod.kernel_size[0], mod.stride[0], mod.padding[0],
                     inp[0].shape[-2], inp[0].shape[-1]))

    for c in ref.modules():
        if isinstance(c, torch.nn.Conv2d):
            c.register_forward_hook(hook)
    with torch.no_grad():
        ref(torch.zeros(1, 2, H, W) if deep12 else torch.zeros(1, 1, 2, H, W))
    assert len(rows) == (12 if deep12 else 48)
    return sorted(set(rows))


# (Cin, Cout, k, stride, H, W): (tile id, stage pixels, splitk, reducer, KG) of the implicit-GEMM weight gradients at 256
# CUs, bf16 x 3.  Every other convolution of the model takes the halo-resident or the event-frame kernel.
GEN1_WGRAD = {   # TinyYolo GEN1 240 x 304, B = 5, T = 32: N = 160
    (64, 32, 1, 1, 120, 152): (4, 64, 512, 1, 16),
    (64, 64, 1, 1, 120, 152): (4, 64, 512, 1, 16),
    (128, 64, 1, 1, 60, 76): (4, 64, 256, 1, 16),
    (128, 64, 1, 1, 120, 152): (4, 64, 256, 1, 16),
    (128, 128, 1, 1, 60, 76): (0, 32, 768, 1, 16),
    (128, 128, 3, 1, 8, 10): (0, 32, 48, 1, 4),
    (128, 128, 3, 1, 15, 19): (0, 32, 56, 1, 4),
    (256, 27, 1, 1, 8, 10): (2, 32, 48, 1, 8),
    (256, 27, 1, 1, 15, 19): (2, 32, 176, 1, 16),
    (256, 27, 1, 1, 30, 38): (2, 32, 712, 1, 16),
    (256, 36, 1, 1, 8, 10): (1, 32, 48, 1, 8),
    (256, 36, 1, 1, 15, 19): (1, 32, 176, 1, 16),
    (256, 36, 1, 1, 30, 38): (1, 32, 512, 1, 16),
    (256, 128, 1, 1, 8, 10): (0, 32, 48, 1, 8),
    (256, 128, 1, 1, 15, 19): (0, 32, 176, 1, 16),
    (256, 128, 1, 1, 30, 38): (0, 32, 256, 1, 16),
    (256, 256, 1, 1, 8, 10): (0, 32, 48, 1, 8),
    (256, 256, 1, 1, 15, 19): (0, 32, 128, 1, 8),
    (256, 256, 1, 1, 30, 38): (0, 32, 192, 1, 8),
    (256, 256, 3, 2, 15, 19): (0, 32, 14, 1, 1),
    (256, 256, 3, 2, 30, 38): (0, 32, 21, 1, 1),
    (320, 128, 1, 1, 60, 76): (0, 32, 256, 1, 16),
    (512, 256, 1, 1, 8, 10): (0, 32, 48, 1, 4),
    (640, 256, 1, 1, 15, 19): (0, 32, 48, 1, 4),
    (768, 256, 1, 1, 30, 38): (0, 32, 64, 1, 4),
}
MPX_WGRAD = {    # TinyYolo 1 Mpx 720 x 1280, B = 8, T = 32: N = 256
    (64, 32, 1, 1, 360, 640): (4, 64, 512, 1, 16),
    (64, 64, 1, 1, 360, 640): (4, 64, 512, 1, 16),
    (128, 64, 1, 1, 180, 320): (4, 64, 256, 1, 16),
    (128, 64, 1, 1, 360, 640): (4, 64, 256, 1, 16),
    (128, 128, 1, 1, 180, 320): (0, 32, 768, 1, 16),
    (256, 27, 1, 1, 23, 40): (2, 32, 920, 2, 1),
    (256, 27, 1, 1, 45, 80): (2, 32, 1024, 2, 1),
    (256, 27, 1, 1, 90, 160): (2, 32, 1024, 2, 1),
    (256, 36, 1, 1, 23, 40): (1, 32, 512, 1, 16),
    (256, 36, 1, 1, 45, 80): (1, 32, 512, 1, 16),
    (256, 36, 1, 1, 90, 160): (1, 32, 512, 1, 16),
    (256, 128, 1, 1, 23, 40): (0, 32, 256, 1, 16),
    (256, 128, 1, 1, 45, 80): (0, 32, 384, 1, 16),
    (256, 128, 1, 1, 90, 160): (0, 32, 384, 1, 16),
    (256, 256, 1, 1, 23, 40): (0, 32, 192, 1, 8),
    (256, 256, 1, 1, 45, 80): (0, 32, 192, 1, 8),
    (256, 256, 1, 1, 90, 160): (0, 32, 192, 1, 8),
    (320, 128, 1, 1, 180, 320): (0, 32, 256, 1, 16),
    (512, 256, 1, 1, 23, 40): (0, 32, 96, 1, 4),
    (640, 256, 1, 1, 45, 80): (0, 32, 72, 1, 4),
    (768, 256, 1, 1, 90, 160): (0, 32, 64, 1, 4),
}


@pytest.mark.parametrize("name,N,H,W,table", [("gen1", 160, 240, 304, GEN1_WGRAD), ("1mpx", 256, 720, 1280, MPX_WGRAD)])
def test_gemm_plans_of_the_model_layers(hip_lib, name, N, H, W, table):
    """The plan of every implicit-GEMM layer of the model at 256 CUs is pinned: a retuning of wgrad_tile, split_resident or
    the reducer choice shows here as the rows it moves.  The forward of every such layer takes the pipelined loader."""
    from snn_for_object_detection_amd import _hip
    got = {}
    for Cin, Cout, k, s, pad, h, w in _model_conv_layers(H, W):
        p = wgrad_plan(hip_lib, N, h, w, Cin, Cout, k, k, s, pad, _hip.PREC_BF16X3, 256)
        assert p is not None
        if p["kernel"] <= 2:
            assert p["kernel"] == (0 if Cout % 4 == 0 else 2), (Cin, Cout, k, s, h, w, p)   # pipelined; the heads' 27: scalar
            got[(Cin, Cout, k, s, h, w)] = (p["tile"], p["stage"], p["splitk"], p["reducer"], p["kg"])
            f = gather_plan(hip_lib, 0, N, h, w, Cin, Cout, k, k, s, pad, _hip.PREC_FP16X3, fps=N // 32, split=1)
            assert f["loader"] == 3 and f["bn"] == (32 if Cout <= 32 else 64 if Cout <= 64 else 128), (Cin, Cout, f)
            rows = N // 32 * ((h + 2 * pad - k) // s + 1) * ((w + 2 * pad - k) // s + 1)   # output pixels of a timestep
            assert rows >= 128 and (f["bn_chunks"], f["bn_rows"]) == (-(-rows // 128) + 1, 128), (Cin, Cout, f)
        else:
            assert (k == 3) and p["kernel"] == (4 if Cin == 2 else 3), (Cin, Cout, k, s, h, w, p)
    assert got == table, {k: v for k, v in got.items() if table.get(k) != v}


def test_deep12_has_no_implicit_gemm_layer(hip_lib):
    """The deep-12 config (twelve 64-channel 3x3 layers behind the event-frame layer, 240 x 304, B = 2, T = 128) runs no
    implicit GEMM: its forward / data gradients are halo-resident and so are its weight gradients."""
    from snn_for_object_detection_amd import _hip
    layers = _model_conv_layers(240, 304, deep12=True)
    assert layers == [(2, 64, 3, 1, 1, 240, 304), (64, 64, 3, 1, 1, 240, 304)]
    for Cin, Cout, k, s, pad, h, w in layers:
        p = wgrad_plan(hip_lib, 256, h, w, Cin, Cout, k, k, s, pad, _hip.PREC_BF16X3, 256)
        assert p["kernel"] == (4 if Cin == 2 else 3), (Cin, Cout, p)
        if Cin == 2:
            assert gather_plan(hip_lib, 0, 256, h, w, Cin, Cout, k, k, s, pad, _hip.PREC_FP16X3) is None   # k_conv_first takes it
        else:
            assert hip_lib.snn_conv3x3_halo_supported(256, h, w, Cin, Cout) == 1


def _reduce_groups(p):
    """The slab rows each group of the planned reducer walks, exactly as the kernels clip them."""
    launched = p["kg"] if p["reducer"] in (0, 1) else p["groups"]
    rows = [(j * p["per"], min((j + 1) * p["per"], p["splitk"])) for j in range(launched)]
    return [r for r in rows if r[0] < r[1]], launched


# Plan classes the sweep below must reach (it fails when one disappears) ...
GEMM_REACHABLE = (
    {("tile", i) for i in range(6)} | {("stage", 32), ("stage", 64)} | {("kernel", i) for i in range(5)}
    | {("reducer", 0, kg) for kg in (1, 4, 16, 64)} | {("reducer", 1, kg) for kg in (1, 2, 4, 8, 16)}
    | {("reducer", 2, 1), "empty_split", "idle_reduce_group", "splitk%8", "splitk%8!=0", "splitk>=32", "splitk=1"}
    | {("loader", i) for i in range(6)} | {("bn", 32), ("bn", 64), ("bn", 128), "idle_blocks", "mtiles_per_xcd>1",
                                           "phase_without_tap"})
# ... and the ones it must NOT reach: dead code as the planners stand.  k_wgrad_reduce4 in ONE pass needs more than 48
# slabs of at least 4 * num_cu * 1024 elements each and a 16-byte aligned dw; the 256 MiB workspace cap and the
# one-resident-wave rule (splitk <= 3 * num_cu / tiles with tiles >= n / 128^2) keep splitk below 49 there for every
# kernel family that feeds the reducer.
GEMM_UNREACHABLE = {("reducer", 3, 1)}


def test_gemm_plan_invariants(hip_lib):
    """snn_conv2d_wgrad_plan / snn_conv2d_gather_plan over a host-side sweep of shapes, layouts and CU counts: the splits
    cover every pixel in whole stages, the tiles cover Cout x Ktot, the workspace stays within 256 MiB, the reducer's
    groups cover the slab rows exactly once, the XCD-padded grid covers the tiles and the phases of a data gradient
    partition the taps and the pixels."""
    from snn_for_object_detection_amd import _hip
    seen = set()
    chans = (1, 3, 4, 27, 32, 36, 64, 100, 130, 132, 256, 768, 1024)
    frames = ((1, 1, 1), (1, 5, 7), (2, 9, 13), (3, 30, 38), (5, 60, 76), (160, 30, 38), (160, 120, 152), (256, 360, 640))
    for num_cu in (64, 256, 304):
        for N, H, W in frames:
            for k in (1, 3, 5, 7):
                for s in (1, 2, 3):
                    pad = k // 2
                    if H + 2 * pad < k or W + 2 * pad < k:
                        continue
                    Ho, Wo = (H + 2 * pad - k) // s + 1, (W + 2 * pad - k) // s + 1
                    M = N * Ho * Wo
                    for Cin in chans:
                        for Cout in chans:
                            if (Cin * Cout > 1024 * 256 and k > 1) or k * k * Cin * Cout >= 2 ** 26:
                                continue
                            for prec in (_hip.PREC_BF16X3, _hip.PREC_FP32):
                                for align in (ALL_ALIGNED, 0):
                                    p = wgrad_plan(hip_lib, N, H, W, Cin, Cout, k, k, s, pad, prec, num_cu, align=align)
                                    assert p is not None, (N, H, W, Cin, Cout, k, s)
                                    what = (num_cu, N, H, W, Cin, Cout, k, s, prec, align, p)
                                    n = Cout * k * k * Cin
                                    assert 1 <= p["splitk"] <= 32768 and p["splitk"] * n * 4 <= 256 << 20 or p["splitk"] == 1, what
                                    if num_cu == 256 and align and not torch.cuda.is_available():
                                        assert p["splitk"] == hip_lib.snn_conv2d_wgrad_splitk(N, H, W, Cin, Ho, Wo, Cout, k, k, s, pad, prec)
                                    seen.add(("kernel", p["kernel"]))
                                    groups, launched = _reduce_groups(p)
                                    assert len(groups) == p["groups"] and groups[0][0] == 0 and groups[-1][1] == p["splitk"], what
                                    assert all(a[1] == b[0] for a, b in zip(groups, groups[1:])), what
                                    assert (p["reducer"] in (1, 2, 3)) <= (n % 4 == 0 and align != 0), what
                                    seen.add(("reducer", p["reducer"], p["kg"]))
                                    if launched > p["groups"]:
                                        seen.add("idle_reduce_group")
                                    if p["kernel"] > 2:
                                        continue
                                    # pipelined: 32-bit byte offsets inside a pixel split (its images and one more on each side)
                                    near = ((p["pps"] * s * s + 3 * H * W) * Cin * 4 < 2 ** 31 - 1 and p["pps"] * Cout * 4 < 2 ** 31 - 1)
                                    assert p["kernel"] == (2 if (not align or Cin % 4 or Cout % 4) else 0 if prec and near else 1), what
                                    assert p["splitk"] * p["pps"] >= M and p["pps"] % p["stage"] == 0, what
                                    assert p["tiles_m"] * p["bm"] >= Cout > (p["tiles_m"] - 1) * p["bm"], what
                                    assert p["tiles_n"] * p["bn"] >= k * k * Cin > (p["tiles_n"] - 1) * p["bn"], what
                                    assert p["splitk"] < 32 or p["splitk"] % 8 == 0, what
                                    owners = p["splitk"] - p["empty"]
                                    assert (owners - 1) * p["pps"] + p["last_pix"] == M and 1 <= p["last_pix"] <= p["pps"], what
                                    assert p["grid"] == p["tiles_m"] * p["tiles_n"] * p["splitk"], what
                                    seen |= {("tile", p["tile"]), ("stage", p["stage"])}
                                    seen.add("splitk=1" if p["splitk"] == 1 else "splitk>=32" if p["splitk"] >= 32
                                             else "splitk%8" if p["splitk"] % 8 == 0 else "splitk%8!=0")
                                    if p["empty"]:
                                        seen.add("empty_split")
                            # forward and every phase of the data gradient
                            for mode, prec in ((0, _hip.PREC_FP16X3), (1, _hip.PREC_BF16X3)):
                                if num_cu != 256:
                                    continue
                                taps, pix = set(), 0
                                first = gather_plan(hip_lib, mode, N, H, W, Cin, Cout, k, k, s, pad, prec)
                                if first is None:
                                    assert mode == 0 and Cin == 2, (N, H, W, Cin, Cout, k, s)
                                    continue
                                for ph in range(first["nphases"]):
                                    g = gather_plan(hip_lib, mode, N, H, W, Cin, Cout, k, k, s, pad, prec, phase=ph,
                                                    split=(Cin + Cout) % 2, add=mode, add2=mode)
                                    what = (mode, N, H, W, Cin, Cout, k, s, ph, g)
                                    oc, ic = (Cout, Cin) if mode == 0 else (Cin, Cout)
                                    assert g["bn"] == (32 if oc <= 32 else 64 if oc <= 64 else 128), what
                                    assert g["ntiles"] * g["bn"] >= oc > (g["ntiles"] - 1) * g["bn"], what
                                    assert g["mtiles"] == -(-N * g["ohc"] * g["owc"] // 128), what
                                    assert g["mtiles_per_xcd"] * 8 >= g["mtiles"] > (g["mtiles_per_xcd"] - 1) * 8, what
                                    assert g["blocks"] == g["mtiles_per_xcd"] * 8 * g["ntiles"], what
                                    assert g["idle"] == g["blocks"] - g["mtiles"] * g["ntiles"], what
                                    assert g["ktot"] == g["nkh"] * g["nkw"] * ic, what
                                    ih, iw = (H, W) if mode == 0 else (Ho, Wo)            # the gathered image: < 2 GiB for four
                                    fast_ok = (ic % 32 == 0 and 1 <= g["nkh"] * g["nkw"] <= 31 and max(g["nkh"], g["nkw"]) <= 6
                                               and ih * iw * ic * 16 < 2 ** 31 - 1 and oc * k * k * ic * 4 < 2 ** 31 - 1)
                                    assert g["loader"] == ((3 if (Cin + Cout) % 2 else 2) if fast_ok else 1 if ic % 4 == 0 else 0), what
                                    seen |= {("loader", g["loader"]), ("bn", g["bn"])}
                                    if g["idle"]:
                                        seen.add("idle_blocks")
                                    if g["mtiles_per_xcd"] > 1:
                                        seen.add("mtiles_per_xcd>1")
                                    if g["ktot"] == 0:
                                        seen.add("phase_without_tap")
                                    if mode == 1:
                                        sh, sw = min(s, H), min(s, W)
                                        ph_, pw_ = ph // sw, ph % sw
                                        kh0, kw0 = (ph_ + pad) % s, (pw_ + pad) % s
                                        mine = {(kh, kw) for kh in range(kh0, k, s) for kw in range(kw0, k, s)}
                                        assert len(mine) == g["nkh"] * g["nkw"] and not (mine & taps), what
                                        taps |= mine
                                        assert (g["ohc"], g["owc"]) == (len(range(ph_, H, s)), len(range(pw_, W, s))), what
                                        pix += g["ohc"] * g["owc"]
                                if mode == 1:
                                    assert first["nphases"] == min(s, H) * min(s, W) and pix == H * W, (H, W, s)
                                    if s <= min(H, W):
                                        assert taps == {(a, b) for a in range(k) for b in range(k)}, (k, s, taps)
    # the two loaders the sweep's plain operands cannot select, on the shapes test_gpu_bf16_storage.py / test_gpu_siblings.py use
    assert gather_plan(hip_lib, 0, 6, 9, 11, 64, 128, 3, 3, 2, 1, _hip.PREC_BF16S)["loader"] == 4
    assert gather_plan(hip_lib, 2, 6, 9, 11, 64, 128, 1, 1, 1, 0, _hip.PREC_FP16X3)["loader"] == 5
    seen |= {("loader", 4), ("loader", 5)}
    for num_cu in (64, 256, 304):                      # the slab counts of the halo-resident and event-frame kernels
        for N, H, W, Cin, Cout in ((1, 310, 517, 32, 32), (160, 120, 152, 32, 32), (160, 240, 304, 2, 64), (1, 9, 9, 2, 4),
                                   (3, 17, 23, 2, 16), (256, 360, 640, 32, 32)):
            p = wgrad_plan(hip_lib, N, H, W, Cin, Cout, 3, 3, 1, 1, _hip.PREC_BF16X3, num_cu)
            assert p["kernel"] in (3, 4) and p["tile"] == p["stage"] == p["grid"] == 0
            groups, launched = _reduce_groups(p)
            assert len(groups) == p["groups"] and groups[0][0] == 0 and groups[-1][1] == p["splitk"]
            seen |= {("kernel", p["kernel"]), ("reducer", p["reducer"], p["kg"])}
    assert GEMM_REACHABLE <= seen, GEMM_REACHABLE - seen
    assert not (GEMM_UNREACHABLE & seen), GEMM_UNREACHABLE & seen
    assert {x for x in seen if isinstance(x, tuple) and x[0] == "reducer"} <= GEMM_REACHABLE, seen
