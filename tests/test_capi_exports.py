"""CPU (`-m "not gpu"`): liblmi_hip.so loads and exports every symbol include/lmi_hip.h declares.
No compute is called (there is no GPU in the build container)."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "lmi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(lmi_[a-z_0-9]+)\s*\(", text)))


def test_header_symbols_exported_and_bound():
    from learnedmetricindex_amd import _capi

    names = _declared()
    assert len(names) >= 18
    assert os.path.exists(_capi.LIB_PATH), "build liblmi_hip.so first (__graft_entry__.build())"
    L = ctypes.CDLL(_capi.LIB_PATH)
    for n in names:
        assert hasattr(L, n), f"{n} declared in lmi_hip.h but not exported"
    assert sorted(_capi.SIGNATURES) == names  # the Python binding covers exactly the header
    assert L.lmi_abi_version() == 1


def test_plan_fields_follow_the_header_enum():
    """_capi.PLAN_FIELDS names the LMI_PLAN_* words of lmi_hip.h, in the enum's order (LMI_PLAN_COUNT closes it)."""
    from learnedmetricindex_amd import _capi

    text = open(os.path.join(ROOT, "include", "lmi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\bLMI_PLAN_([A-Z0-9_]+)\b\s*(?:=\s*0\s*)?[,\n]", text)
    assert names[-1] == "COUNT" and len(names) == len(set(names))
    assert [n.lower() for n in names[:-1]] == [f.lower() for f in _capi.PLAN_FIELDS]


def test_mlp_plan_fields_follow_the_header_enum():
    """_capi.MLP_PLAN_FIELDS names the LMI_MLP_PLAN_* words of lmi_hip.h, in the enum's order (LMI_MLP_PLAN_COUNT closes it)."""
    from learnedmetricindex_amd import _capi

    text = open(os.path.join(ROOT, "include", "lmi_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\bLMI_MLP_PLAN_([A-Z0-9_]+)\b\s*(?:=\s*0\s*)?[,\n]", text)
    assert names[-1] == "COUNT" and len(names) == len(set(names))
    assert [n.lower() for n in names[:-1]] == [f.lower() for f in _capi.MLP_PLAN_FIELDS]
    assert len(names) - 1 <= 32   # CallState::PLAN_WORDS


def test_missing_library_fails_loudly(monkeypatch):
    from learnedmetricindex_amd import _capi

    monkeypatch.setattr(_capi, "_lib", None)
    monkeypatch.setattr(_capi, "LIB_PATH", "/nonexistent/liblmi_hip.so")
    try:
        _capi.lib()
    except _capi.LmiError as e:
        assert "no CPU fallback" in str(e)
    else:
        raise AssertionError("expected LmiError")
