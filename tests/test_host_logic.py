"""CPU-side checks: description API, module-tree / state_dict layout, C-ABI symbol export, build."""
import ctypes
import os
import re

import pytest
import torch

import snn_for_object_detection_amd as S
from oracle.net import SODaRef


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
