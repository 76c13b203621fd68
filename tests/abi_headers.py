"""The C headers under include/ read as text, and compared with the binding's signature tables (vla_adapter_amd/native.py: FAMILIES).

prototypes(text) gives every function a header declares as (return type, [parameter types]) in C spelling without names and without
`const`; disagreements(text, protos) lists, one line each, where a signature table departs from that: a function the other side lacks, a
parameter count, the type of parameter i, the return type.  Both work on text, so a test can hand them a doctored header.  load_library
is the one place that builds the library when it is missing."""
import ctypes as C
import os
import re

from vla_adapter_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int": C.c_int, "unsigned": C.c_uint, "unsigned int": C.c_uint, "long long": C.c_longlong, "unsigned long long": C.c_ulonglong,
           "float": C.c_float, "double": C.c_double}
# what a typed pointer of the table may point to: POINTER(T) -> the C spelling of T
POINTEES = {C.c_float: "float", C.c_int: "int", native.GemmDesc: "vla_gemm_desc", native.GemmTnDesc: "vla_gemm_tn_desc",
            native.AttnDesc: "vla_attn_desc", native.HeadAttnDesc: "vla_head_attn_desc"}
TYPE_WORDS = {"void", "char", "short", "int", "long", "unsigned", "signed", "float", "double"}


def header_text(header: str) -> str:
    return open(os.path.join(ROOT, "include", header)).read()


def load_library():
    """The bound library, built first when a clean checkout has none."""
    if not os.path.exists(native.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return native.load()


def strip(text: str) -> str:
    """Without comments and preprocessor lines."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return re.sub(r"^[ \t]*#[^\n]*$", " ", text, flags=re.M)


def c_type(decl: str) -> str:
    """`const unsigned char* bytes` -> `unsigned char*`: a declaration without `const` and without the name."""
    words = [w for w in decl.replace("*", " * ").split() if w != "const"]
    stars = words.count("*")
    base = words[:words.index("*")] if stars else words
    if len(base) > 1 and base[-1] not in TYPE_WORDS:          # a scalar's name follows its type; a pointer's follows the star
        base = base[:-1]
    assert base and stars <= 1 and "[" not in decl, f"a declaration this reader does not know: {decl!r}"
    return " ".join(base) + "*" * stars


def prototypes(text: str) -> dict:
    """{name: (return type, [parameter types])} of every `type vla_name(...);` of a header's text."""
    out = {}
    for ret, name, params in re.findall(r"([\w \t\n*]+?)\b(vla_[a-z0-9_]+)\s*\(([^(){};]*)\)\s*;", strip(text)):
        assert name not in out, f"{name} is declared twice"
        params = [] if params.strip() in ("", "void") else [c_type(p) for p in params.split(",")]
        out[name] = (c_type(ret), params)
    return out


def symbols(text: str) -> list:
    """Every vla_ name in front of a parenthesis, prototype or not: what prototypes() must account for."""
    return sorted(set(re.findall(r"\b(vla_[a-z0-9_]+)\s*\(", strip(text))))


def agrees(c: str, bound) -> bool:
    """Does the ctypes type `bound` pass what the C type `c` takes?  Any pointer may be bound as c_void_p; a POINTER(T) must name the pointee."""
    if c.endswith("*"):
        return bound is C.c_void_p or (hasattr(bound, "_type_") and POINTEES.get(bound._type_) == c[:-1])
    return c in SCALARS and bound is SCALARS[c]


def spelled(bound) -> str:
    """The C spelling of a ctypes type of the tables (ctypes' own names differ between platforms: c_longlong is c_long on LP64)."""
    if bound is C.c_void_p:
        return "void*"
    if hasattr(bound, "_type_") and bound._type_ in POINTEES:
        return POINTEES[bound._type_] + "*"
    return next((c for c, t in SCALARS.items() if t is bound), repr(bound))


def disagreements(text: str, protos: dict, extra=()) -> list:
    """Where the table `protos` {name: (argtypes, restype)} and the header's text differ; [] when they agree.  `extra`: names the header
    declares that are bound outside the table."""
    declared = prototypes(text)
    out = [f"{n}: in the header's text, but no prototype was read" for n in symbols(text) if n not in declared]
    out += [f"{n}: declared by the header, not in the table" for n in declared if n not in protos and n not in extra]
    out += [f"{n}: in the table, not declared by the header" for n in list(protos) + list(extra) if n not in declared]
    for name in (n for n in protos if n in declared):
        (ret, params), (args, res) = declared[name], protos[name]
        if not agrees(ret, res):
            out.append(f"{name}: returns {ret}, bound as {spelled(res)}")
        if len(params) != len(args):
            out.append(f"{name}: {len(params)} parameters in the header, {len(args)} in the table")
            continue
        out += [f"{name}: parameter {i} is {c}, bound as {spelled(b)}" for i, (c, b) in enumerate(zip(params, args)) if not agrees(c, b)]
    return out
