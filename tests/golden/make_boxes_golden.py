"""Generate ``tests/golden/boxes.npz`` from the REFERENCE's own label conversion (run in the build container only).

    python tests/golden/make_boxes_golden.py            # needs the reference tree (SNN_REFERENCE, default /root/reference)

``PropheseeDatasetBase._labels_prepare`` of the reference's ``utils/datasets.py`` is executed unmodified on small seeded
structured arrays with the field layouts of the two datasets' ``*_bbox.npy`` files, and the arrays and what came out are
stored as DATA - no reference source.  The module imports ``lightning`` and the Prophesee toolbox's ``PSEELoader`` at
import time only; empty stand-in modules satisfy both (the same device ``make_golden.py::events_golden`` uses).  The
fixture pins ``snn_for_object_detection_amd.recordings.load_boxes`` (``tests/test_recordings_host.py``).
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = os.environ.get("SNN_REFERENCE", "/root/reference")
OUT = os.path.dirname(os.path.abspath(__file__))

GEN1_DTYPE = [("ts", "<u8"), ("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("class_id", "u1"),
              ("confidence", "<f4"), ("track_id", "<u4")]
MPX_DTYPE = [("t", "<u8"), ("x", "<f4"), ("y", "<f4"), ("w", "<f4"), ("h", "<f4"), ("class_id", "<u4"),
             ("track_id", "<u4"), ("class_confidence", "<f4")]


def load_reference_datasets():
    stand_ins = {"lightning": types.ModuleType("lightning")}
    stand_ins["lightning"].LightningDataModule = type("LightningDataModule", (), {"__init__": lambda self, *a, **k: None})
    chain = ("prophesee_toolbox", "prophesee_toolbox.src", "prophesee_toolbox.src.io",
             "prophesee_toolbox.src.io.psee_loader")
    for name in chain:
        stand_ins[name] = types.ModuleType(name)
        stand_ins[name].__path__ = []
    stand_ins[chain[-1]].PSEELoader = type("PSEELoader", (), {})
    saved = {k: sys.modules.get(k) for k in stand_ins}
    sys.modules.update(stand_ins)
    try:
        spec = importlib.util.spec_from_file_location("ref_datasets_boxes", os.path.join(REF, "utils", "datasets.py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return mod


def boxes(rng, dtype, n, width, height, time_field):
    """Seeded rows: timestamps over the whole 60 s (some exactly on a step boundary, one just below it), boxes with
    fractional pixel coordinates, some reaching past the frame (the recordings hold such rows)."""
    b = np.zeros(n, dtype=dtype)
    t = np.sort(rng.integers(0, 60_000_000, n))
    t[1], t[2], t[3] = 16_000 * 7, 16_000 * 7 + 15_999, 16_000 * 8
    b[time_field] = np.sort(t)
    b["x"] = rng.uniform(0, width, n).astype(np.float32)
    b["y"] = rng.uniform(0, height, n).astype(np.float32)
    b["w"] = rng.uniform(1, width / 2, n).astype(np.float32)
    b["h"] = rng.uniform(1, height / 2, n).astype(np.float32)
    b["class_id"] = rng.integers(0, 2 if time_field == "ts" else 7, n)
    b["track_id"] = rng.integers(0, 1000, n)
    b["confidence" if time_field == "ts" else "class_confidence"] = rng.uniform(0, 1, n).astype(np.float32)
    return b


def main():
    ds = load_reference_datasets()
    rng = np.random.default_rng(2024)
    out = {}
    for tag, name, dtype, time_field, time_step_ms in (("gen1", "gen1", GEN1_DTYPE, "ts", 16),
                                                       ("1mpx", "1mpx", MPX_DTYPE, "t", 10)):
        d = ds.STPropheseeDataset(num_steps=4, time_shift=2, gt_files=["g"], data_files=["d"], time_step=time_step_ms,
                                  num_load_file=1, name=name)
        arr = boxes(rng, dtype, 24, d._width, d._height, time_field)
        (labels,) = d._labels_prepare([arr])
        assert tuple(labels.shape) == (24, 6) and str(labels.dtype) == "torch.float32"
        out[f"{tag}_boxes"] = arr
        out[f"{tag}_labels"] = labels.numpy().copy()
        out[f"{tag}_time_step_us"] = d.time_step_us
    np.savez_compressed(os.path.join(OUT, "boxes.npz"), **out)
    print("boxes.npz written to", OUT)


if __name__ == "__main__":
    main()
