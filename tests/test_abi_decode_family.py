"""The open end of the registry of entry-point families (vla_adapter_amd/native.py: ADDED_FAMILIES, behind the nine of
tests/test_abi_families.py and the pinned LATER_FAMILIES of tests/test_abi_later_families.py) against its headers under include/, the
built library and the memory-contract modules that exercise it - the same agreement checks (no compute calls: nothing here needs a
GPU), written over the tuple and not over one name.

Two literal tables carry what is pinned per family: FAMILY (the names with their argument counts, and the files the csrc Makefile must
name) and CONTRACT_MODULE (where the family's memory-contract cases live).  The next family adds one row to ADDED_FAMILIES and one
row to each table here - not a fourth tuple and not another copy of this file."""
import importlib
import os

import pytest

from tests import abi_headers as H
from tests import test_abi_families as NINE
from tests import test_abi_later_families as LATER
from vla_adapter_amd import native

KEYS = [fam.key for fam in native.ADDED_FAMILIES]
FAMILY = {
    "decode": ({"vla_decode_argmax_slabs": 1, "vla_decode_attn": 16, "vla_decode_lm_head_argmax": 23, "vla_decode_prompt": 13,
                "vla_decode_rope_append": 15},
               ("decode.hip", "vla_decode.h", "argmax_order.h")),
}
CONTRACT_MODULE = {"decode": "test_decode_memory_contract_gpu"}


def test_the_open_registry_is_these_families_behind_the_pinned_ones():
    assert KEYS == list(FAMILY) == list(CONTRACT_MODULE)
    assert [fam.header for fam in native.ADDED_FAMILIES] == ["vla_" + k + ".h" for k in KEYS]
    names = [n for fam in native.ADDED_FAMILIES for n in fam.protos]
    assert len(names) == len(set(names)) == len(native.ADDED_PROTOS), "an entry point belongs to one header"
    assert not set(names) & (set(native.PROTOS) | set(native.LATER_PROTOS)), "no name of an earlier family"
    assert not set(KEYS) & (set(NINE.KEYS) | set(LATER.KEYS)), "no key of an earlier family"
    assert [fam.key for fam in native.FAMILIES] == NINE.KEYS and [fam.key for fam in native.LATER_FAMILIES] == LATER.KEYS, "the pinned tuples stay"
    assert native.ALL_FAMILIES == native.FAMILIES + native.LATER_FAMILIES + native.ADDED_FAMILIES
    assert all(native.family(k) is fam for k, fam in zip(KEYS, native.ADDED_FAMILIES))
    assert all(isinstance(fam, native.Family) for fam in native.ADDED_FAMILIES)
    for name in names:
        assert name not in H.header_text("vla_native.h"), "vla_native.h does not move for an added family"
    assert native.ABI_VERSION == 8, "VLA_ABI_VERSION does not move for an added family"


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


@pytest.mark.parametrize("key", KEYS)
def test_the_comparison_reports_a_doctored_header(key):
    """Whatever the family: one parameter more, and another return type, on its first prototype."""
    fam = native.family(key)
    text = H.header_text(fam.header)
    first = next(iter(H.prototypes(text)))
    n = len(fam.protos[first][0])
    at = text.index(first + "(")
    close = text.index(");", at)
    assert H.disagreements(text[:close] + ", int flags" + text[close:], fam.protos) == [f"{first}: {n + 1} parameters in the header, {n} in the table"]
    line = text.rfind("\n", 0, at) + 1
    assert text[line:at] == "int "
    assert H.disagreements(text[:line] + "long long " + text[at:], fam.protos) == [f"{first}: returns long long, bound as int"]
