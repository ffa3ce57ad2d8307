"""Host-side checks of the spike-bit-mask entry points: header and ctypes table agree on them, the ABI version stays, the
shape query answers without a device, and the profiler prices the mask at one bit per element."""
import os
import re
from ctypes import c_int, c_int64, c_void_p

NEW = ("snn_affine_neuron_fwd_mask", "snn_conv1x1_mask_supported", "snn_conv1x1_mask_fwd", "snn_conv1x1_mask_wgrad")


def _header():
    from snn_for_object_detection_amd import _hip
    text = open(os.path.join(os.path.dirname(_hip._HERE), "include", "snn_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_header_and_binding_agree_on_the_new_signatures(hip_lib):
    from ctypes import POINTER
    from snn_for_object_detection_amd import _hip
    raw, code = _header()
    for name in NEW:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        decls = [d.strip() for d in m.group(1).split(",")]
        restype, argtypes = _hip.SIGNATURES[name]
        assert restype is c_int and len(decls) == len(argtypes), name
        for d, a in zip(decls, argtypes):
            if "*" in d:
                want = POINTER(_hip.NeuronParams) if "snn_neuron_params" in d else c_void_p
            else:
                want = {"int": c_int, "int64_t": c_int64}[d.rsplit(None, 1)[0].replace("const ", "").strip()]
            assert a is want, (name, d)
        assert hasattr(hip_lib, name)
    # the scan entry point is snn_affine_neuron_fwd plus (mask, ld_mask); the convolutions take (mask, ld_mask) first
    assert _hip.SIGNATURES["snn_affine_neuron_fwd_mask"][1][:-2] == _hip.SIGNATURES["snn_affine_neuron_fwd"][1]
    assert _hip.SIGNATURES["snn_affine_neuron_fwd_mask"][1][-2:] == [c_void_p, c_int64]
    for name in ("snn_conv1x1_mask_fwd", "snn_conv1x1_mask_wgrad"):
        assert _hip.SIGNATURES[name][1][:2] == [c_void_p, c_int64]
        assert re.search(name + r"\s*\(\s*const uint32_t\s*\*\s*mask\s*,\s*int64_t ld_mask", code)
    assert re.search(r"SNN_SCAN_SPIKE_MASK\s*=\s*32\b", code) and _hip.SCAN_SPIKE_MASK == 32
    assert "bit (c & 31) of word (c >> 5)" in raw          # the layout rule is written down


def test_abi_version_is_still_20(hip_lib):
    from snn_for_object_detection_amd import _hip
    _, code = _header()
    assert hip_lib.snn_abi_version() == 20 and _hip.ABI_VERSION == 20
    assert re.search(r"#define\s+SNN_ABI_VERSION\s+20\b", code)


def test_supported_query_is_host_only(hip_lib):
    """Pointers are only inspected (alignment), never dereferenced: the query runs without a device."""
    from snn_for_object_detection_amd import _hip
    F, B = _hip.PREC_FP16X3, _hip.PREC_BF16X3
    q = hip_lib.snn_conv1x1_mask_supported
    A = 1 << 20   # a 16-byte aligned "address"
    assert q(160, 120, 152, 64, 64, A, 2, A, A, 64, A, 64, A, F, B) == 1          # the flagship's first stage entry
    assert q(160, 8, 10, 256, 256, A, 8, A, A, 256, A, 256, A, F, B) == 1
    assert q(160, 120, 152, 64, 64, A, 2, A, A, 64, None, 0, None, F, B) == 1
    assert q(160, 120, 152, 48, 64, A, 2, A, A, 64, A, 64, A, F, B) == 0          # Cin % 32
    assert q(160, 120, 152, 64, 64, A + 2, 2, A, A, 64, A, 64, A, F, B) == 0      # mask pointer
    assert q(160, 120, 152, 64, 64, A, 2, A, A, 64, A, 66, A, F, B) == 0          # lddy % 4
    assert q(160, 120, 152, 64, 64, A, 2, A + 4, A, 64, A, 64, A, F, B) == 0      # weight alignment
    assert q(160, 120, 152, 64, 64, A, 2, A, A, 64, A + 8, 64, A, F, B) == 0      # dy alignment
    assert q(160, 120, 152, 64, 64, None, 2, A, A, 64, A, 64, A, F, B) == 0
    assert q(1 << 20, 120, 152, 64, 64, A, 2, A, A, 64, A, 64, A, F, B) == 0      # beyond 31-bit offsets


def test_profiler_prices_the_mask_at_one_bit_per_element():
    from snn_for_object_detection_amd.profiler import work_of
    n, h, w, cin, cout = 160, 120, 152, 64, 64
    px = n * h * w
    label, flops, byts = work_of("snn_conv1x1_mask_fwd", (1, 2, 3, 4, cout, n, h, w, cin, cout, 0))
    assert label.endswith(", spikes") and label.startswith("k_conv_gather<") and "mask" in label
    assert flops == 2.0 * px * cin * cout and byts == px * cin / 8.0 + 4.0 * (px * cout + cout * cin)
    label, flops, byts = work_of("snn_conv1x1_mask_wgrad", (1, 2, 3, cout, 5, n, h, w, cin, cout, 0, 6, 7, 0))
    assert label.endswith(", spikes") and label.startswith("k_conv_wgrad")
    assert byts == px * cin / 8.0 + 4.0 * (px * cout + cout * cin)
    T, M, C = 32, 5 * 120 * 152, 64
    scan = [1, 1, C, 1, 1, None, None, None, C, None, 0, 1, 1, 1, T, M, C, None, 8 | 32, 0, 1, C // 32]
    label, _, byts = work_of("snn_affine_neuron_fwd_mask", scan)
    assert label == "k_affine_neuron_fwd<1>" and byts == 4.0 * T * M * C * 2 + T * M * C / 8.0   # y, vdec, + the mask
