"""The reverse-scan plans of ``snn_affine_neuron_bwd_plan`` / ``snn_lif_tau_bwd_plan`` against a recorded table.

``tests/golden/scan_bwd_plans.json`` was recorded ONCE, from the library of the commit before the two planners and the two
launchers of ``csrc/neuron.hip`` (now ``csrc/scan_bwd.hip``) became one (``ScanBwdPlan`` / ``scan_bwd``) - not from the code under test: that commit
was built in a separate worktree and this module run as a script with ``SNN_HIP_LIB`` pointing at its ``libsnn_hip.so``
(``SNN_HIP_LIB=<old tree>/snn_for_object_detection_amd/libsnn_hip.so python -m tests.test_scan_bwd_plans_host``; the ABI
is the same, so this tree's binding drives it).  Both queries are host-only, and without a device the planner counts on
256 compute units - the MI355X's own count - so the table holds on a machine with or without one.

Rows, in the order of ``cases()``: shape x with_sums x flags x gradient rule x neuron x time-constant request.  A row is
the ten (twelve with a time-constant request) plan words, or the refusal: an index into ``messages``, the full text of
``snn_last_error``.  ``sizes`` holds, per shape, ``snn_affine_neuron_bwd_sums_size``, ``snn_lif_tau_bwd_partial_size``
(without / with the BatchNorm sums) and ``snn_affine_neuron_bwd_sums_from_state`` (default rule / atan + detached).
"""
import ctypes
import itertools
import json
import os

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "scan_bwd_plans.json")
SHAPES = [(8, 98, 4), (6, 180, 3), (8, 84, 16), (6, 84, 24), (32, 42, 512), (32, 1425, 256), (5, 7, 64), (128, 300, 128)]
REQUESTS = ("none", "constants", "constants+sums")


def _space():
    from snn_for_object_detection_amd import _hip
    from snn_for_object_detection_amd import functional as HF
    flags = (0, _hip.SCAN_WIDE_ADDRESSING, _hip.SCAN_LAST_STEP_ONLY, _hip.SCAN_BF16_STORAGE, _hip.SCAN_SUMS_FROM_STATE,
             _hip.SCAN_SUMS_FROM_STATE | _hip.SCAN_STATE_LOOKBACK)
    rules = (HF.neuron_params(), HF.neuron_params(surrogate="atan", detach_reset=True))
    neurons = (_hip.NEURON_LIF, _hip.NEURON_LI, _hip.NEURON_SLI)
    return flags, rules, neurons


def cases():
    flags, rules, neurons = _space()
    return itertools.product(SHAPES, (0, 1), flags, rules, neurons, REQUESTS)


def ask(lib, shape, with_sums, flags, params, neuron, request):
    """-> the plan words, or the refusal's text."""
    T, M, C = shape
    if request == "none":
        out = (ctypes.c_int64 * 10)()
        rc = lib.snn_affine_neuron_bwd_plan(neuron, T, M, C, C, C, with_sums, params, flags, ctypes.addressof(out))
    else:
        out = (ctypes.c_int64 * 12)()
        rc = lib.snn_lif_tau_bwd_plan(neuron, T, M, C, C, C, with_sums, int(request == "constants+sums"), params, flags,
                                      ctypes.addressof(out))
    return list(out) if rc == 0 else lib.snn_last_error().decode()


def sizes(lib):
    from snn_for_object_detection_amd import _hip
    _, rules, _ = _space()
    return [[lib.snn_affine_neuron_bwd_sums_size(T, M, C), lib.snn_lif_tau_bwd_partial_size(T, M, C, 0),
             lib.snn_lif_tau_bwd_partial_size(T, M, C, 1)]
            + [lib.snn_affine_neuron_bwd_sums_from_state(_hip.NEURON_LIF, T, M, C, C, p, 0) for p in rules]
            for T, M, C in SHAPES]


def test_plans_and_refusals_equal_the_recorded_table(hip_lib):
    table = json.load(open(GOLDEN))
    assert table["shapes"] == [list(s) for s in SHAPES]
    assert sizes(hip_lib) == table["sizes"]
    rows, messages = table["rows"], table["messages"]
    all_cases = list(cases())
    assert len(rows) == len(all_cases) == 8 * 2 * 6 * 2 * 3 * 3
    plans = refusals = 0
    for case, row in zip(all_cases, rows):
        want = row if isinstance(row, list) else messages[row]
        got = ask(hip_lib, *case)
        shape, with_sums, flags, params, neuron, request = case
        assert got == want, (shape, with_sums, flags, params.surrogate, neuron, request)
        plans += isinstance(row, list)
        refusals += not isinstance(row, list)
    assert plans >= 200 and refusals >= 200   # the table exercises both


def record():
    from snn_for_object_detection_amd import _hip
    assert os.environ.get("SNN_HIP_LIB"), "record from the library of the commit before the change (SNN_HIP_LIB=...)"
    lib = _hip.load()
    messages, rows = [], []
    for case in cases():
        got = ask(lib, *case)
        if isinstance(got, str):
            if got not in messages:
                messages.append(got)
            got = messages.index(got)
        rows.append(got)
    with open(GOLDEN, "w") as f:
        f.write('{"shapes": %s,\n "sizes": %s,\n "messages": [\n  %s\n ],\n "rows": [\n  %s\n ]}\n' % (
            json.dumps([list(s) for s in SHAPES]), json.dumps(sizes(lib)),
            ",\n  ".join(json.dumps(m) for m in messages), ",\n  ".join(json.dumps(r) for r in rows)))
    print(GOLDEN, len(rows), "rows,", len(messages), "messages")


if __name__ == "__main__":
    record()
