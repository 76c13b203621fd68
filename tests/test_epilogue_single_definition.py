"""The epilogue arithmetic of a Linear is stated once (csrc/gemm_epilogue.h, the bf16 packing in csrc/common.h): a source-level guard
against re-duplication.  Reads the HIP sources as text; no GPU, no build."""
import pathlib
import re

CSRC = pathlib.Path(__file__).resolve().parent.parent / "vla_adapter_amd" / "csrc"

# what is guarded -> (regular expression, the one file that may hold it)
SINGLE = {
    # sigmoid(g) = 1 / (1 + exp(-g)): the core of SiLU, as a reciprocal or a division
    "SiLU": (r"1\.0?f\s*\+\s*__expf\(\s*-", "gemm_epilogue.h"),
    # silu'(g) = sg (1 + g (1 - sg))
    "SiLU'": (r"\*\s*\(\s*1\.0?f\s*-\s*sg\s*\)", "gemm_epilogue.h"),
    # the pair rotation with every product rounded: rbf(a c) + rbf(-b s) and rbf(b c) + rbf(a s)
    "RoPE rotation (a c - b s)": (r"rbf\([^()]*\*[^()]*\)\s*\+\s*rbf\(\s*-[^()]*\*[^()]*\)", "gemm_epilogue.h"),
    "RoPE rotation (b c + a s)": (r"rbf\([^()]*\*[^()]*\)\s*\+\s*rbf\(\s*[^-\s(][^()]*\*[^()]*\)", "gemm_epilogue.h"),
    # a packed bf16 pair to two floats: the old spelling bf2f((bf16_t)(x & 0xffff)) / (x >> 16), and the one spelling's body
    "bf16-pair unpack": (r"\(bf16_t\)\s*\(.*(&\s*0xffffu?\s*\)|>>\s*16\s*\))|&\s*0xffff0000u", "common.h"),
}

# open-coded sites that stay, each with its reason: {guard: {file: (lines that may match, reason)}}
ALLOWED = {
    "SiLU": {
        # sigmoid by an exact division, du associated as d (g sg): sharing swiglu_bwd (reciprocal, (d g) sg) would change the bits of
        # vla_swiglu_bwd, which a refactor must not
        "elementwise.hip": (1, "swiglu_bwd_kernel keeps its exact-division sigmoid; silu' comes from the header"),
        # exp(-x^2) / exp(-x^2 / 2) of the erf and GELU-gradient approximations: not a sigmoid
        "common.h": (1, "fast_erf: 1.0f - poly * __expf(-ax * ax) is the erf series, not SiLU"),
    },
    "bf16-pair unpack": {
        # raw 16-bit element copy of a staged segment's ragged tail: bits moved, no float conversion, nothing to round
        "gemm256.hip": (1, "ragged tail of the SwiGLU product h: a bit copy of packed elements, no arithmetic"),
    },
}


def sources():
    return sorted(p for p in CSRC.iterdir() if p.suffix in (".hip", ".h"))


def strip_comments(text):
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return "\n".join(line.split("//")[0] for line in text.splitlines())


def test_sources_found():
    names = {p.name for p in sources()}
    assert {"gemm_epilogue.h", "common.h", "gemm.hip", "gemm256.hip", "gemm_skinny.hip", "gemm_tn.hip", "elementwise.hip"} <= names


def test_each_epilogue_expression_is_defined_in_one_file():
    problems = []
    for what, (pattern, home) in SINGLE.items():
        rx = re.compile(pattern)
        hits = {}
        for path in sources():
            n = sum(1 for line in strip_comments(path.read_text()).splitlines() if rx.search(line))
            if n:
                hits[path.name] = n
        assert hits.get(home, 0) >= 1, f"{what}: the pattern no longer matches its definition in {home} - update the guard"
        for name, n in hits.items():
            if name == home:
                continue
            allowed = ALLOWED.get(what, {}).get(name, (0, ""))[0]
            if n > allowed:
                problems.append(f"{what}: {n} open-coded line(s) in {name} (allowed: {allowed}); use {home}")
    assert not problems, "\n".join(problems)


def test_shared_helpers_are_defined_once():
    text = {p.name: strip_comments(p.read_text()) for p in sources()}
    for helper in (r"void glds16s\(", r"v8i_f8 cat8\(", r"#define \w*BARRIER\(\)", r"int xcd_order\(", r"void unpack8\w*\(", r"uint4 pack8\("):
        where = [name for name, t in text.items() if re.search(helper, t)]
        assert where == ["common.h"], f"{helper}: defined in {where}, expected common.h"
