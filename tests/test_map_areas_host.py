"""The C ABI of the mAP area ranges, per-class output and size filter (csrc/metrics.hip): declared, exported and bound
alike; ABI 20 with the old three entry points unchanged; every refusal by name, in front of any launch.  No GPU needed."""
import ctypes
import os
import re
from ctypes import c_double, c_int, c_size_t, c_void_p

import pytest

P, I, D = c_void_p, c_int, c_double
NEW = {
    "snn_map_filter_rows": (c_int, [P, P, I, I, I, I, D, D, D, D, P, P, P, P]),
    "snn_map_match_areas": (c_int, [P] * 5 + [I] * 5 + [P, I, D, D, I] + [P] * 7),
    "snn_map_areas_workspace_size": (c_size_t, [I, I, I, I]),
    "snn_map_accumulate_areas": (c_int, [P] * 6 + [I, I, I, P, I, P] + [I] * 5 + [P] * 4),
}
OLD = {
    "snn_map_match": (c_int, [P, P, P, P, I, I, I, I, I, P, I, P, P, P, P]),
    "snn_map_workspace_size": (c_size_t, [I, I, I]),
    "snn_map_accumulate": (c_int, [P, P, P, I, I, I, P, I, P, I, I, I, I, P, P, P]),
}


def _header():
    from snn_for_object_detection_amd import _hip
    text = open(os.path.join(os.path.dirname(_hip._HERE), "include", "snn_hip.h")).read()
    return text, re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def test_symbols_are_declared_exported_and_bound(hip_lib):
    from snn_for_object_detection_amd import _hip
    text, code = _header()
    assert "#define SNN_ABI_VERSION 20" in text and _hip.ABI_VERSION == 20 and hip_lib.snn_abi_version() == 20
    declared = set(re.findall(r"\b(snn_[a-z0-9_]+)\s*\(", code))
    raw = ctypes.CDLL(_hip.LIB_PATH)
    for name, sig in {**NEW, **OLD}.items():
        assert name in declared and hasattr(raw, name), name
        assert _hip.SIGNATURES[name] == sig, name
        fn = getattr(hip_lib, name)
        assert fn.restype is sig[0] and list(fn.argtypes) == sig[1], name


def test_old_prototypes_are_unchanged():
    """The three entry points that tests/test_gpu_map.py calls directly, parameter for parameter."""
    _, code = _header()
    flat = re.sub(r"\s+", " ", code)
    assert ("int snn_map_match(const float* dets, const float* labels, const int* order, const int* seg, int B, int A, "
            "int G, int num_classes, int slots, const double* iou_thresholds, int num_iou, float* score, "
            "unsigned* match_mask, int* npig, void* stream);") in flat
    assert "size_t snn_map_workspace_size(int num_classes, int num_max_dets, int num_iou);" in flat
    assert ("int snn_map_accumulate(const int* order, const unsigned* match_mask, const int* npig, int num_classes, "
            "int records, int slots, const int* max_dets, int num_max_dets, const double* rec_thresholds, int num_rec, "
            "int num_iou, int t50, int t75, void* workspace, float* out, void* stream);") in flat


def test_workspace_size(hip_lib):
    base = hip_lib.snn_map_workspace_size(7, 3, 10)
    assert base == 2 * 7 * 3 * 10 * 8
    assert hip_lib.snn_map_areas_workspace_size(7, 3, 10, 0) == base
    assert hip_lib.snn_map_areas_workspace_size(7, 3, 10, 3) == 4 * base
    assert hip_lib.snn_map_areas_workspace_size(7, 3, 10, 2) == 0 and hip_lib.snn_map_areas_workspace_size(0, 3, 10, 3) == 0


def _refused(lib, rc, name, *words):
    msg = lib.snn_last_error().decode()
    assert rc != 0 and msg.startswith(name + ":"), (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_filter_rows_refusals(hip_lib):
    """Null pointers throughout: nothing could have been launched."""
    host = (ctypes.c_float * 8)()
    a = ctypes.addressof(host)      # never dereferenced: every call below is refused first
    name = "snn_map_filter_rows"

    def call(dets=a, labels=a, B=1, A=1, G=1, C=2, h=240.0, w=304.0, diag=0.0, side=0.0, key=a, cls=a, bad=a):
        return hip_lib.snn_map_filter_rows(dets, labels, B, A, G, C, h, w, diag, side, key, cls, bad, None)

    for arg in ("dets", "labels", "key", "cls", "bad"):
        _refused(hip_lib, call(**{arg: None}), name, "null pointer")
    for kw in (dict(B=0), dict(A=0), dict(G=0), dict(C=0)):
        _refused(hip_lib, call(**kw), name, "bad shape")
    _refused(hip_lib, call(B=65535, A=40000), name, "31-bit")
    for kw in (dict(h=0.0), dict(w=-1.0), dict(h=float("nan"))):
        _refused(hip_lib, call(**kw), name, "image size")
    for kw in (dict(diag=-1.0), dict(side=-0.5), dict(side=float("nan"))):
        _refused(hip_lib, call(**kw), name, "min_box_diag", "min_box_side")


def test_match_areas_refusals(hip_lib):
    host = (ctypes.c_float * 8)()
    a = ctypes.addressof(host)
    name = "snn_map_match_areas"

    def call(B=1, A=1, G=1, C=2, S=100, T=10, h=240.0, w=304.0, nr=3, **ptr):
        p = {k: ptr.get(k, a) for k in ("dets", "labels", "label_cls", "order", "seg", "iou", "score", "mask",
                                        "matched", "ignored", "npig", "npig_area")}
        return hip_lib.snn_map_match_areas(p["dets"], p["labels"], p["label_cls"], p["order"], p["seg"], B, A, G, C, S,
                                           p["iou"], T, h, w, nr, p["score"], p["mask"], p["matched"], p["ignored"],
                                           p["npig"], p["npig_area"], None)

    for arg in ("dets", "labels", "label_cls", "order", "seg", "iou", "score", "mask", "npig"):
        _refused(hip_lib, call(**{arg: None}), name, "null pointer")
    for arg in ("matched", "ignored", "npig_area"):
        _refused(hip_lib, call(**{arg: None}), name, "null area pointer")
    for nr in (1, 2, 4, -1):
        _refused(hip_lib, call(nr=nr), name, "num_ranges", str(nr))
    _refused(hip_lib, call(G=2049), name, "2049", "2048")
    _refused(hip_lib, call(S=1025), name, "1025", "1024")
    _refused(hip_lib, call(S=0), name, "slots")
    _refused(hip_lib, call(T=32), name, "32", "31")
    _refused(hip_lib, call(B=0), name, "bad shape")
    _refused(hip_lib, call(B=65536), name, "bad shape")
    _refused(hip_lib, call(h=0.0), name, "image size")
    _refused(hip_lib, call(w=float("nan")), name, "image size")


def test_accumulate_areas_refusals(hip_lib):
    host = (ctypes.c_float * 8)()
    a = ctypes.addressof(host)
    name = "snn_map_accumulate_areas"

    def call(C=2, N=200, S=100, M=3, R=101, T=10, t50=0, t75=5, nr=3, **ptr):
        p = {k: ptr.get(k, a) for k in ("order", "mask", "matched", "ignored", "npig", "npig_area", "max_dets", "rec",
                                        "ws", "out", "out_class")}
        return hip_lib.snn_map_accumulate_areas(p["order"], p["mask"], p["matched"], p["ignored"], p["npig"],
                                                p["npig_area"], C, N, S, p["max_dets"], M, p["rec"], R, T, t50, t75, nr,
                                                p["ws"], p["out"], p["out_class"], None)

    for arg in ("order", "mask", "npig", "max_dets", "rec", "ws", "out"):
        _refused(hip_lib, call(**{arg: None}), name, "null pointer")
    for arg in ("matched", "ignored", "npig_area"):
        _refused(hip_lib, call(**{arg: None}), name, "null area pointer")
    for nr in (1, 2, 4, -1):
        _refused(hip_lib, call(nr=nr), name, "num_ranges", str(nr))
    _refused(hip_lib, call(N=150), name, "bad shape")             # records is images x slots
    _refused(hip_lib, call(C=0), name, "bad shape")
    _refused(hip_lib, call(M=0), name, "maxDet")
    _refused(hip_lib, call(T=32), name, "32", "31")
    _refused(hip_lib, call(R=1025), name, "1025", "1024")
    _refused(hip_lib, call(t50=10), name, "threshold index")


def test_metric_validates_its_options_on_the_host():
    """Constructor and ``update_padded`` checks that come before any device work."""
    from snn_for_object_detection_amd.metrics import MeanAveragePrecision
    for kw in (dict(min_box_diag=-1.0), dict(min_box_side=float("nan")), dict(image_size=(0, 304)),
               dict(image_size=(240, -1))):
        with pytest.raises(ValueError):
            MeanAveragePrecision(2, **kw)
    m = MeanAveragePrecision(2, class_metrics=True, area_ranges=True, image_size=(240, 304), min_box_diag=30.0)
    assert m._keys()[6:] == ["map_small", "mar_small", "map_medium", "mar_medium", "map_large", "mar_large"]
    assert MeanAveragePrecision(2)._keys() == ["map", "map_50", "map_75", "mar_1", "mar_10", "mar_100"]
