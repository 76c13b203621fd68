"""The families of entry points added behind the nine of tests/test_abi_families.py (vla_adapter_amd/native.py: LATER_FAMILIES) against
their headers under include/, the built library and the memory-contract modules that exercise them - the same agreement checks, on the
second registry (no compute calls: nothing here needs a GPU).

Two literal tables carry what is pinned per family: FAMILY (the names with their argument counts, and the files the csrc Makefile must
name) and CONTRACT_MODULE (where the family's memory-contract cases live).  A new family adds one row to each."""
import importlib
import os

import pytest

from tests import abi_headers as H
from tests import test_abi_families as NINE
from vla_adapter_amd import native

KEYS = [fam.key for fam in native.LATER_FAMILIES]
FAMILY = {
    "jpeg_encode": ({"vla_jpeg_encode_plan": 11, "vla_jpeg_encode_workspace_bytes": 4, "vla_jpeg_encode_write": 11},
                    ("jpeg_encode.hip", "vla_jpeg_encode.h", "jpeg_encode_core.h", "jpeg_stage_a.h")),
}
CONTRACT_MODULE = {"jpeg_encode": "test_jpeg_encode_memory_contract_gpu"}


def test_the_later_registry_is_these_families_beside_the_nine():
    assert KEYS == list(FAMILY) == list(CONTRACT_MODULE)
    assert [fam.header for fam in native.LATER_FAMILIES] == ["vla_" + k + ".h" for k in KEYS]
    names = [n for fam in native.LATER_FAMILIES for n in fam.protos]
    assert len(names) == len(set(names)) == len(native.LATER_PROTOS), "an entry point belongs to one header"
    assert not set(names) & set(native.PROTOS) and not set(KEYS) & set(NINE.KEYS), "no name and no key of the nine families"
    assert [fam.key for fam in native.FAMILIES] == NINE.KEYS and len(NINE.KEYS) == 9, "the nine stay the nine"
    assert all(native.family(k) is fam for k, fam in zip(KEYS, native.LATER_FAMILIES))
    assert all(isinstance(fam, native.Family) for fam in native.LATER_FAMILIES)
    for name in names:
        assert name not in H.header_text("vla_native.h"), "vla_native.h does not move for a later family"


@pytest.mark.parametrize("key", KEYS)
def test_header_table_library_and_makefile_agree(key):
    fam, (pinned, files) = native.family(key), FAMILY[key]
    assert {n: len(args) for n, (args, _) in sorted(fam.protos.items())} == pinned
    text = H.header_text(fam.header)
    assert H.disagreements(text, fam.protos) == []
    assert H.symbols(text) == sorted(fam.protos)
    lib = H.load_library()
    for name, (args, res) in fam.protos.items():
        fn = getattr(lib, name, None)
        assert fn is not None, f"libvla_native.so does not export {name}"
        assert list(fn.argtypes) == list(args) and fn.restype is res, f"{name}: native.load() binds the table's signature"
    mk = open(os.path.join(H.ROOT, "vla_adapter_amd", "csrc", "Makefile")).read()
    assert not [f for f in files if f not in mk], "the Makefile names the family's header and sources"


@pytest.mark.parametrize("key", KEYS)
def test_every_symbol_has_a_memory_contract_case_or_an_exemption(key):
    M = importlib.import_module("tests." + CONTRACT_MODULE[key])
    table = set(native.family(key).protos)
    covered, exempt = set(M.COVERED), set(M.EXEMPT)
    assert not (covered | exempt) - table, f"names that are no entry points of this family: {sorted((covered | exempt) - table)}"
    assert not covered & exempt, f"both tested and exempt: {sorted(covered & exempt)}"
    assert not table - covered - exempt, f"entry points with neither a case nor an exemption: {sorted(table - covered - exempt)}"
    for name, reason in M.EXEMPT.items():
        assert isinstance(reason, str) and 4 <= len(reason) and "\n" not in reason, f"{name}: a one-line reason"
    for name, tests in M.COVERED.items():
        for t in tests:
            assert callable(getattr(M, t, None)), f"{name}: case {t} does not exist"


def test_the_comparison_reports_a_doctored_header():
    fam = native.family("jpeg_encode")
    text = H.header_text(fam.header)

    def doctored(old, new):
        assert text.count(old) == 1
        return H.disagreements(text.replace(old, new), fam.protos)
    assert doctored("long long workspace_bytes, long long* frame_off);", "int workspace_bytes, long long* frame_off);") == \
        ["vla_jpeg_encode_plan: parameter 9 is int, bound as long long"]
    assert doctored("long long* frame_off);", "long long* frame_off, int flags);") == ["vla_jpeg_encode_plan: 12 parameters in the header, 11 in the table"]
    assert doctored("int vla_jpeg_encode_write(", "long long vla_jpeg_encode_write(") == ["vla_jpeg_encode_write: returns long long, bound as int"]
