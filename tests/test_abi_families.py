"""Every family of entry points (vla_adapter_amd/native.py: FAMILIES) against its header under include/, the built library and the
memory-contract module that exercises it - once, for all families (no compute calls: nothing here needs a GPU).

Two literal tables carry what is pinned per family: FAMILY (the names with their argument counts, and the files the csrc Makefile must
name) and CONTRACT_MODULE (where the family's memory-contract cases live).  A new family adds one row to each."""
import importlib
import os
import re

import pytest

from tests import abi_headers as H
from vla_adapter_amd import native

KEYS = [fam.key for fam in native.FAMILIES]
# family -> ({entry point: argument count}, files of the csrc Makefile).  The training family is pinned by its size: vla_native.h, its 69
# entry points and VLA_ABI_VERSION 8 do not move when a family is added.
FAMILY = {
    "native": (69, ("vla_native.h",)),
    "serve": ({"vla_normalize_proprio_serve": 9, "vla_serve_gather_hidden": 11, "vla_serve_tokens": 17, "vla_unnormalize_actions": 12},
              ("serve.hip", "vla_serve.h")),
    "episodes": ({"vla_episode_gather": 23, "vla_episode_sample": 14}, ("episodes.hip", "vla_episodes.h")),
    "mixture": ({"vla_mixture_sample": 18, "vla_normalize_bounds_rows": 12}, ("mixture.hip", "vla_mixture.h")),
    "heldout": ({"vla_heldout_l1_accumulate": 11, "vla_heldout_sweep": 18}, ("heldout.hip", "vla_heldout.h")),
    "digest": ({"vla_state_digest": 7, "vla_state_digest_slots": 0, "vla_token_ce_metrics_ordered": 13}, ("digest.hip", "vla_digest.h")),
    "jpeg": ({"vla_jpeg_decode_rows": 28, "vla_jpeg_workspace_bytes": 4}, ("jpeg.hip", "jpeg_core.h", "episode_row.h", "vla_jpeg.h")),
    "jpeg_index": ({"vla_jpeg_decode_rows_at": 29, "vla_jpeg_index_build": 24}, ("jpeg_index.hip", "vla_jpeg_index.h")),
    "policy_image": ({"vla_policy_image_workspace_bytes": 6, "vla_policy_jpeg_round_trip": 11, "vla_policy_lanczos3_resize": 17},
                     ("policy_image.hip", "vla_policy_image.h", "jpeg_forward.h", "jpeg_stage_b.h")),
}
CONTRACT_MODULE = {
    "native": "test_memory_contract_gpu", "serve": "test_serve_memory_contract_gpu", "episodes": "test_episodes_memory_contract_gpu",
    "mixture": "test_mixture_memory_contract_gpu", "heldout": "test_heldout_memory_contract_gpu", "digest": "test_digest_gpu",
    "jpeg": "test_jpeg_memory_contract_gpu", "jpeg_index": "test_jpeg_index_memory_contract_gpu",
    "policy_image": "test_policy_image_memory_contract_gpu",
}
EXTRA = {"native": ("vla_last_error",)}          # declared by vla_native.h, bound apart from the table (it returns the text, not a code)


def test_the_registry_is_the_nine_families_and_no_name_belongs_to_two():
    assert KEYS == list(FAMILY) == list(CONTRACT_MODULE)
    assert [fam.header for fam in native.FAMILIES] == ["vla_" + k + ".h" for k in KEYS]
    names = [n for fam in native.FAMILIES for n in fam.protos]
    assert len(names) == len(set(names)) == len(native.PROTOS), "an entry point belongs to one header"
    assert all(native.family(k) is fam for k, fam in zip(KEYS, native.FAMILIES))
    assert native.ABI_VERSION == 8 == int(re.search(r"#define VLA_ABI_VERSION (\d+)", H.header_text("vla_native.h")).group(1))


@pytest.mark.parametrize("key", KEYS)
def test_header_table_library_and_makefile_agree(key):
    fam, (pinned, files) = native.family(key), FAMILY[key]
    if isinstance(pinned, int):
        assert len(fam.protos) == pinned
    else:
        assert {n: len(args) for n, (args, _) in sorted(fam.protos.items())} == pinned
    # the header declares the table's names (H.disagreements names a missing or an extra one) with the table's types
    text = H.header_text(fam.header)
    assert H.disagreements(text, fam.protos, EXTRA.get(key, ())) == []
    assert H.symbols(text) == sorted(list(fam.protos) + list(EXTRA.get(key, ())))
    # the library exports them, and native.load() has bound exactly the table's signature
    lib = H.load_library()
    for name, (args, res) in fam.protos.items():
        fn = getattr(lib, name, None)
        assert fn is not None, f"libvla_native.so does not export {name}"
        assert list(fn.argtypes) == list(args) and fn.restype is res, f"{name}: native.load() binds the table's signature"
    for name in EXTRA.get(key, ()):
        assert hasattr(lib, name), f"libvla_native.so does not export {name}"
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
    """The check above on text alone: one header, spoilt four ways, against the unchanged table."""
    fam = native.family("jpeg_index")
    text = H.header_text(fam.header)
    assert H.disagreements(text, fam.protos) == []

    def doctored(old, new):
        assert text.count(old) == 1
        return H.disagreements(text.replace(old, new), fam.protos)
    # parameter 6 of vla_jpeg_decode_rows_at, the segment count: long long -> int
    assert doctored("const int* seg_ent, long long S,", "const int* seg_ent, int S,") == ["vla_jpeg_decode_rows_at: parameter 6 is int, bound as long long"]
    assert doctored(" long long S_out,", "") == ["vla_jpeg_index_build: 23 parameters in the header, 24 in the table"]
    assert doctored("#ifdef __cplusplus\n}", "int vla_jpeg_index_rows(void* stream, long long S);\n#ifdef __cplusplus\n}") == \
        ["vla_jpeg_index_rows: declared by the header, not in the table"]
    assert doctored("int vla_jpeg_index_build(", "long long vla_jpeg_index_build(") == ["vla_jpeg_index_build: returns long long, bound as int"]
    # and the other direction: a table whose long long was bound as int
    args, res = fam.protos["vla_jpeg_decode_rows_at"]
    spoilt = dict(fam.protos, vla_jpeg_decode_rows_at=(args[:25] + [native._I] + args[26:], res))
    assert H.disagreements(text, spoilt) == ["vla_jpeg_decode_rows_at: parameter 25 is long long, bound as int"]
