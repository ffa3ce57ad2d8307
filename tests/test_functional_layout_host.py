"""The layering of the Python operators (host only, no device): ``functional`` is the one namespace and the one home of
levers and mutable state; ``_layout``, ``pointwise``, ``losses`` and ``event_ops`` lie below it and never look up."""

import ast
import os

import pytest

import snn_for_object_detection_amd as S
from snn_for_object_detection_amd import _layout, event_ops, functional, losses, pointwise

LOWER = (_layout, pointwise, losses, event_ops)
ALLOWED_SIBLINGS = {"_hip", "_layout"}
PACKAGE = S.__name__
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "functional_names.txt")


def _tree(module) -> ast.Module:
    with open(module.__file__) as f:
        return ast.parse(f.read())


def _package_imports(tree: ast.Module):
    """``(module inside the package or "", imported name)`` of every import from the package, in any spelling."""
    found = []
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            for a in node.names:
                if a.name == PACKAGE or a.name.startswith(PACKAGE + "."):
                    found.append((a.name[len(PACKAGE) + 1:], ""))
        elif isinstance(node, ast.ImportFrom):
            mod = node.module or ""
            if node.level == 0 and not (mod == PACKAGE or mod.startswith(PACKAGE + ".")):
                continue
            inner = mod if node.level else mod[len(PACKAGE) + 1:]
            found.extend((inner, a.name) for a in node.names)
    return found


def test_every_earlier_name_is_still_an_attribute_of_functional():
    with open(GOLDEN) as f:
        names = f.read().split()
    assert len(names) == 216 and names == sorted(names)
    missing = [n for n in names if not hasattr(functional, n)]
    assert not missing, missing
    moved = 0
    for n in names:
        for home in LOWER:
            if n in vars(home):
                assert getattr(functional, n) is getattr(home, n), (n, home.__name__)
                moved += 1
    assert moved > 60     # the four families did move (a façade of copies would fail the identity above)


@pytest.mark.parametrize("module", LOWER, ids=lambda m: m.__name__.rsplit(".", 1)[-1])
def test_lower_modules_import_only_hip_and_layout(module):
    tree = _tree(module)
    imports = _package_imports(tree)
    assert imports, "the module calls the library: it imports _hip"
    for inner, name in imports:
        first = (inner or name).split(".")[0]
        assert first in ALLOWED_SIBLINGS, f"{module.__name__} imports {inner or '.'}:{name}"
        assert "functional" not in (inner.split(".") + [name])
        assert name != "*"
    assert not any(a.name == "*" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom) for a in n.names)


def test_functional_has_no_star_import():
    assert not any(a.name == "*" for n in ast.walk(_tree(functional)) if isinstance(n, ast.ImportFrom) for a in n.names)


@pytest.mark.parametrize("module", LOWER, ids=lambda m: m.__name__.rsplit(".", 1)[-1])
def test_state_has_one_home(module):
    tree = _tree(module)
    assigned = set()
    for node in tree.body:
        targets = node.targets if isinstance(node, ast.Assign) else \
            [node.target] if isinstance(node, (ast.AnnAssign, ast.AugAssign)) else []
        assigned.update(n.id for t in targets for n in ast.walk(t) if isinstance(n, ast.Name))
    assert not assigned & set(functional.LEVERS)
    for node in ast.walk(tree):
        assert not isinstance(node, ast.Global)
        assert not (isinstance(node, ast.Attribute) and node.attr in ("environ", "getenv", "putenv")), node.lineno
        if isinstance(node, (ast.Import, ast.ImportFrom)):
            assert "os" not in [a.name for a in node.names] + [getattr(node, "module", None)], node.lineno


def _snapshot():
    return {n: getattr(functional, n) for n in functional.LEVERS}


def test_levers_lists_the_assignable_names():
    assert len(set(functional.LEVERS)) == len(functional.LEVERS)
    for n in functional.LEVERS:
        assert n in vars(functional), n
    for n in vars(functional):
        if n.startswith("USE_"):
            assert n in functional.LEVERS, n
    for n in ("FUSE_OUTER_ADDEND", "WGRAD_SIDE_DEPTH", "SPIKE_MASK_MIN_BYTES", "SCAN_SEGMENT_T", "SCAN_FLAGS",
              "LIF_CHECKPOINT_BYTES"):
        assert n in functional.LEVERS, n


def test_levers_refuses_an_unknown_name_before_changing_anything():
    before = _snapshot()
    with pytest.raises(AttributeError, match="USE_SIBLING_FUSON"):
        with functional.levers(USE_HALO_CONV=not before["USE_HALO_CONV"], USE_SIBLING_FUSON=False):
            raise AssertionError("the block must not run")
    assert _snapshot() == before
    assert not hasattr(functional, "USE_SIBLING_FUSON")
    with pytest.raises(AttributeError):
        with functional.levers(_ACTIVITY=None):       # module state, not a lever
            raise AssertionError("the block must not run")


def test_levers_sets_inside_and_restores_after_exit_and_exception():
    before = _snapshot()
    flipped = not before["USE_HALO_CONV"]
    with functional.levers(USE_HALO_CONV=flipped, SCAN_SEGMENT_T=7):
        assert functional.USE_HALO_CONV is flipped and functional.SCAN_SEGMENT_T == 7
        assert functional.SCAN_FLAGS == before["SCAN_FLAGS"]
    assert _snapshot() == before
    with pytest.raises(ZeroDivisionError):
        with functional.levers(USE_HALO_CONV=flipped, SCAN_FLAGS=5):
            assert functional.SCAN_FLAGS == 5
            1 / 0
    assert _snapshot() == before


def test_nested_levers_restore_in_order_and_none_comes_back_as_none():
    before = _snapshot()
    assert before["LIF_CHECKPOINT_BYTES"] is None
    with functional.levers(LIF_CHECKPOINT_BYTES=0, SCAN_SEGMENT_T=5):
        assert functional.LIF_CHECKPOINT_BYTES == 0
        with functional.levers(LIF_CHECKPOINT_BYTES=1 << 20, SCAN_SEGMENT_T=None):
            assert functional.LIF_CHECKPOINT_BYTES == 1 << 20 and functional.SCAN_SEGMENT_T is None
        assert functional.LIF_CHECKPOINT_BYTES == 0 and functional.SCAN_SEGMENT_T == 5
    assert functional.LIF_CHECKPOINT_BYTES is None
    assert _snapshot() == before
