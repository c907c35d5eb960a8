"""The Python adapter's surface: every name importable from vaq_amd and vaq_amd.index, and every public method,
property and signature of the five adapter classes, against the list recorded in tests/golden/adapter_surface.json
BEFORE vaq_amd/index.py was split into one module per class.  A name may be added; a recorded one that is missing
or whose signature changed fails under its own name.  Needs neither the library nor a GPU.

Regenerate (only when the surface is meant to change): python tests/test_adapter_surface_cpu.py > tests/golden/adapter_surface.json
"""
import inspect
import json
import os
import sys
import types

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "adapter_surface.json")
CLASSES = ("VaqHip", "VaqHipFast", "VaqHipMulti", "VaqRefiner", "VaqMultiRefiner")


def _kind(obj) -> str:
    """What a name is, as a string that changes when its call changes."""
    if isinstance(obj, property):
        return "property"
    if isinstance(obj, (staticmethod, classmethod)):
        obj = obj.__func__
    if inspect.isclass(obj):
        return "class" + str(inspect.signature(obj.__init__))
    if inspect.isfunction(obj):
        return str(inspect.signature(obj))
    return "attribute"


def _module_names(mod) -> dict:
    """The adapter's own public names in a module: not the modules it imported, not typing's or dataclasses' names.
    (Of the helpers with an underscore, the two a test imports are checked by name below.)"""
    out = {}
    for name, obj in vars(mod).items():
        if name.startswith("_") or isinstance(obj, types.ModuleType):
            continue
        if getattr(obj, "__module__", "").split(".")[0] == "vaq_amd":
            out[name] = _kind(obj)
    return out


def _class_members(cls) -> dict:
    out = {"__init__": _kind(cls.__init__)}
    for name in dir(cls):
        if not name.startswith("_"):
            out[name] = _kind(inspect.getattr_static(cls, name))
    return out


def surface() -> dict:
    import vaq_amd
    import vaq_amd.index
    return {"vaq_amd": _module_names(vaq_amd), "vaq_amd.__all__": sorted(vaq_amd.__all__),
            "vaq_amd.index": _module_names(vaq_amd.index),
            "classes": {c: _class_members(getattr(vaq_amd.index, c)) for c in CLASSES}}


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def current():
    return surface()


@pytest.mark.parametrize("module", ["vaq_amd", "vaq_amd.index"])
def test_module_names_and_signatures(recorded, current, module):
    assert len(recorded[module]) >= 18
    bad = [f"{module}.{n}: recorded {k!r}, now {current[module].get(n, 'MISSING')!r}"
           for n, k in recorded[module].items() if current[module].get(n) != k]
    assert not bad, "\n".join(bad)


def test_package_all(recorded, current):
    missing = sorted(set(recorded["vaq_amd.__all__"]) - set(current["vaq_amd.__all__"]))
    assert not missing, f"gone from vaq_amd.__all__: {missing}"


@pytest.mark.parametrize("cls", CLASSES)
def test_class_members_and_signatures(recorded, current, cls):
    assert len(recorded["classes"][cls]) >= 10
    bad = [f"{cls}.{n}: recorded {k!r}, now {current['classes'][cls].get(n, 'MISSING')!r}"
           for n, k in recorded["classes"][cls].items() if current["classes"][cls].get(n) != k]
    assert not bad, "\n".join(bad)


def test_names_other_files_import_resolve():
    """bench.py, tools/ and the tests import these from vaq_amd.index."""
    import vaq_amd.index as ix
    for name in ("_same", "_wref", "merge_topk_packed_device", "merge_topk_device", "merge_fast_device", "VaqHipMulti",
                 "VaqHip", "NNMethod"):
        assert callable(getattr(ix, name)), name
    a = [1]
    assert ix._same(ix._wref(a), a) and not ix._same(ix._wref(a), [1]) and ix._same(None, None)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    json.dump(surface(), sys.stdout, indent=1, sort_keys=True)
    sys.stdout.write("\n")
