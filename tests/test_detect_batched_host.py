"""Host-side checks of the batched detection path: the C ABI carries the three entry points with the signatures the binding
calls them with, and ``predict_sequence`` refuses what it cannot interpret before anything reaches the device."""
import ctypes
from ctypes import c_float, c_int, c_void_p

import pytest
import torch


def test_batched_detect_symbols_are_exported_with_the_bound_signatures(hip_lib):
    from snn_for_object_detection_amd import _hip
    P, I, F = c_void_p, c_int, c_float
    want = {
        # prob, offsets, anchors, N, A, K, conf, cls, boxes, stream
        "snn_detect_decode_batched": [P, P, P, I, I, I, P, P, P, P],
        # boxes, order, seg, N, A, classes, iou threshold, kept, nkept, kept_flag, kept_rank, stream
        "snn_nms_sorted_batched": [P, P, P, I, I, I, F, P, P, P, P, P],
        # conf, cls, boxes, nkept, kept_flag, kept_rank, N, A, classes, pos threshold, out, stream
        "snn_detect_assemble": [P, P, P, P, P, P, I, I, I, F, P, P],
    }
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name, args in want.items():
        assert _hip.SIGNATURES[name] == (c_int, args), name
        assert hasattr(raw, name), name
        fn = getattr(hip_lib, name)
        assert fn.restype is c_int and list(fn.argtypes) == args
    assert hip_lib.snn_abi_version() == _hip.ABI_VERSION >= 19
    # argument checks run on the host, in front of the launch: a null pointer is an error code, not a fault
    assert hip_lib.snn_detect_decode_batched(None, None, None, 1, 1, 2, None, None, None, None) != 0
    assert b"snn_detect_decode_batched" in hip_lib.snn_last_error()


def test_predict_sequence_rejects_a_tensor_of_the_wrong_rank():
    import snn_for_object_detection_amd as S
    m = S.TinyYolo(num_classes=2, time_window=0).eval()
    for shape in ((2, 32, 48), (1, 1, 1, 2, 32, 48)):
        with pytest.raises(ValueError, match="rank"):
            m.predict_sequence(torch.zeros(*shape))
    from snn_for_object_detection_amd import box
    with pytest.raises(RuntimeError, match="device tensors"):
        box.multibox_detection_batched(torch.rand(2, 8, 3), torch.rand(2, 8, 4), torch.rand(8, 4))
