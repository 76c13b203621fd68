"""Sampling of action tokens without a GPU: the float64 rule of tests/sample_rule_np.py against the installed transformers' warpers, its
generator against Python-integer arithmetic, the distribution of its draws, what generate_actions and the entry point of
include/vla_sample.h refuse on the host, and the agreement checks of the registry's open end (native.OPEN_FAMILIES)."""
import ctypes as C
import importlib
import math
import os

import numpy as np
import pytest
import torch

from tests import abi_headers as H
from tests import sample_rule_np as R
from vla_adapter_amd import native

# ---------------------------------------------------------------------------------------------------------------- the rule against HF
SETTINGS = [(0.7, 50, 0.9), (1.0, 0, 0.95), (1.6, 5, 1.0), (1.0, 1, 1.0)]      # (temperature, top_k, top_p)


def bf16_logits(rows, V, seed=0, std=4.0):
    g = torch.Generator().manual_seed(seed)
    return (std * torch.randn(rows, V, generator=g)).to(torch.bfloat16).float()


@pytest.mark.parametrize("temperature,top_k,top_p", SETTINGS)
def test_the_rule_keeps_what_the_transformers_warpers_keep(temperature, top_k, top_p):
    from transformers.generation.logits_process import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    l = bf16_logits(4, 1016)
    scores = TemperatureLogitsWarper(temperature)(None, l.clone())
    if top_k:
        scores = TopKLogitsWarper(top_k=top_k)(None, scores)
    if top_p < 1:
        scores = TopPLogitsWarper(top_p=top_p)(None, scores)
    hf = torch.isfinite(scores).numpy()
    counts = []
    for b in range(4):
        z = R.scale(l[b].numpy(), temperature)
        kept, gap = R.keep(z, top_k, top_p)
        assert gap > 1e-4, f"row {b}: the top-p boundary is {gap:.2e} from flipping; the comparison needs another generator seed"
        assert not (hf[b] & ~kept).any(), f"row {b}: the rule drops a token the warpers keep"
        extra = kept & ~hf[b]
        assert (z[extra] == z[hf[b]].min()).all(), f"row {b}: an extra token outside the boundary class of equal logits"
        counts.append(int(kept.sum()))
    if (temperature, top_k, top_p) == SETTINGS[0]:
        assert counts == [2, 1, 3, 9]
    if top_k == 1:
        assert all(c >= 1 for c in counts) and all((l[b].numpy()[R.keep(R.scale(l[b].numpy(), 1.0), 1, 1.0)[0]] == float(l[b].max())).all() for b in range(4))


def test_top_k_keeps_ties_and_top_p_works_on_value_classes():
    z = np.array([1.0, 3.0, 3.0, 2.0, 2.0, 0.0, -0.0])
    assert R.keep(z, 1, 1.0)[0].tolist() == [False, True, True, False, False, False, False]
    assert R.keep(z, 3, 1.0)[0].tolist() == [False, True, True, True, True, False, False]            # the tie at the third value
    assert R.keep(z, 0, 1.0)[0].all() and R.keep(z, 7, 1.0)[0].all() and R.keep(z, 99, 1.0)[0].all()
    p = np.exp(z - R.logsumexp(z))
    below_twos = p[[0, 5, 6]].sum()
    kept, gap = R.keep(z, 0, 1.0 - (below_twos + 1e-3))                     # the mass below the 2s may go, the 2s may not
    assert kept.tolist() == [False, True, True, True, True, False, False] and abs(gap - 1e-3) < 1e-6
    assert R.keep(z, 0, 1e-6)[0].tolist() == [False, True, True, False, False, False, False]         # the largest class always stays
    assert R.keep(z, 0, 1.0 - 1e-9)[0].all()
    # -0.0 and 0.0 are one class: dropped or kept together
    assert R.keep(z, 0, 1.0 - (p[[5, 6]].sum() + 1e-3))[0].tolist() == [True, True, True, True, True, False, False]


# ---------------------------------------------------------------------------------------------------------------- the generator
M64 = (1 << 64) - 1


def splitmix_int(seed, idx):
    z = (seed + idx * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


KNOWN = {(0, 0, 0, 0): 0x277AB99AF6178267, (1, 2, 3, 4): 0x3D7A15A980F41EEA, (2 ** 63 + 5, 7, 13, 151935): 0x662E1495BDC7528F}


def test_draw_bits_known_answers():
    for (seed, stream, t, v), want in KNOWN.items():
        r = int(R.draw_bits(seed, stream, t, v + 1)[v])
        assert r == want == splitmix_int(splitmix_int(splitmix_int(seed ^ R.SAMPLE_STREAM, stream), t), v)
    for seed, stream, t in [(3, 0, 0), (3, 1, 0), (3, 0, 1), (4, 0, 0), (-1 & M64, 2 ** 40, 55)]:
        r = R.draw_bits(seed, stream, t, 300)
        assert [int(x) for x in r[[0, 1, 299]]] == [splitmix_int(splitmix_int(splitmix_int(seed ^ R.SAMPLE_STREAM, stream), t), v) for v in (0, 1, 299)]
    a = R.draw_bits(3, 0, 0, 64)
    assert all((a != R.draw_bits(*k, 64)).all() for k in [(4, 0, 0), (3, 1, 0), (3, 0, 1)]), "seed, stream and step each move every draw"


def test_uniform_is_exact_in_float32_and_inside_the_open_interval():
    r = np.concatenate([R.draw_bits(11, 5, 9, 4096), np.array([0, M64, 1 << 41, (1 << 41) - 1, M64 - (1 << 41) + 1], dtype=np.uint64)])
    u = R.uniform(r)
    assert (u.astype(np.float32).astype(np.float64) == u).all(), "u has at most 24 significant bits"
    assert u.min() == 2.0 ** -24 and u.max() == 1.0 - 2.0 ** -24 and np.isfinite(-np.log(-np.log(u))).all()
    n = (r >> np.uint64(41)).astype(np.float32)
    assert (((n + np.float32(0.5)) * np.float32(2.0 ** -23)).astype(np.float64) == u).all(), "the float32 arithmetic of the device forms the same value"


# ---------------------------------------------------------------------------------------------------------------- the distribution
DIST_SEED, DIST_V, DIST_STREAMS, DIST_STEPS = 0, 24, 64, 128


def dist_logits():
    return bf16_logits(1, DIST_V, seed=0, std=2.0)[0].numpy()


def chi2_quantile(df, tail):
    """The 1 - tail quantile of chi-square with df degrees of freedom."""
    try:
        from scipy.stats import chi2
        return float(chi2.isf(tail, df))
    except ImportError:                                        # Wilson-Hilferty, with the normal quantile by bisection on erfc
        lo, hi = 0.0, 10.0
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            lo, hi = (mid, hi) if 0.5 * math.erfc(mid / math.sqrt(2.0)) > tail else (lo, mid)
        return df * (1.0 - 2.0 / (9.0 * df) + lo * math.sqrt(2.0 / (9.0 * df))) ** 3


def chi_square(tokens, l):
    z = l.astype(np.float64)
    expect = tokens.size * np.exp(z - R.logsumexp(z))
    return float(((np.bincount(tokens.ravel(), minlength=l.size) - expect) ** 2 / expect).sum())


def test_draws_follow_the_softmax():
    l = dist_logits()
    tokens = np.array([[R.step(l, seed=DIST_SEED, stream=s, t=t)["token"] for t in range(DIST_STEPS)] for s in range(DIST_STREAMS)])
    bound = chi2_quantile(DIST_V - 1, 1e-6)
    assert 70.0 < bound < 76.0
    stat = chi_square(tokens, l)
    print(f"chi-square of {tokens.size} draws over {DIST_V} tokens: {stat:.2f} (bound {bound:.2f})")
    assert stat < bound


def test_greedy_and_non_finite_rows():
    l = bf16_logits(1, 1000, seed=3)[0].numpy()
    g = R.step(l, greedy=True)
    assert g["token"] == int(np.argmax(l)) and abs(g["logprob"] - float(torch.log_softmax(torch.from_numpy(l).double(), 0)[g["token"]])) < 1e-12
    tie = l.copy()
    tie[[7, 900]] = l.max() + 1
    assert R.step(tie, greedy=True)["token"] == 7
    for bad, want in ((np.nan, 500), (np.inf, 500)):
        x = tie.copy()
        x[500] = bad
        for greedy in (True, False):
            r = R.step(x, 0.7, 50, 0.9, seed=1, greedy=greedy)
            assert r["token"] == want and np.isnan(r["logprob"]) and np.isnan(r["probs"]).all()   # the first NaN; +inf is the largest
    assert np.isnan(R.step(np.full(8, -np.inf, np.float32))["logprob"]) and R.step(np.full(8, -np.inf, np.float32))["token"] == 0


# ---------------------------------------------------------------------------------------------------------------- generate_actions refuses
@pytest.fixture()
def model():
    """The refusals come before any device work: an instance with a configuration, statistics and a stand-in engine is enough."""
    from types import SimpleNamespace

    from vla_adapter_amd import engine as E
    from vla_adapter_amd.modeling_prismatic import OpenVLAForActionPrediction
    m = object.__new__(OpenVLAForActionPrediction)
    m.cfg = E.tiny_config()
    m.engine = SimpleNamespace(fp8_frozen=False)
    m.norm_stats = {"libero": {"action": {"q01": [-1.0] * 7, "q99": [1.0] * 7}}}
    return m


PX = torch.zeros(1, 3, 8, 8)


def test_generate_actions_refuses_sampling_settings_without_do_sample(model):
    for kw in (dict(temperature=0.7), dict(top_k=0), dict(top_p=0.9), dict(seed=3), dict(sample_streams=[0])):
        with pytest.raises(ValueError, match="belong to do_sample=True"):
            model.generate_actions([[5, 6]], pixel_values=PX, **kw)


def test_generate_actions_refuses_bad_sampling_settings(model):
    call = lambda **kw: model.generate_actions([[5, 6]], pixel_values=PX, do_sample=True, **kw)
    with pytest.raises(ValueError, match="needs an int seed"):
        call()
    with pytest.raises(ValueError, match="needs an int seed"):
        call(seed=1.5)
    for bad in (0.0, -1.0, float("nan"), "1"):
        with pytest.raises(ValueError, match="temperature must be a number above 0"):
            call(seed=1, temperature=bad)
    for bad in (-1, 2.0, True):
        with pytest.raises(ValueError, match="top_k must be an int >= 0"):
            call(seed=1, top_k=bad)
    for bad in (0.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match=r"top_p must lie in \(0, 1\]"):
            call(seed=1, top_p=bad)
    for bad in ([0, 1], [0.5], "a", [True]):
        with pytest.raises(ValueError, match="sample_streams must be B = 1 ints"):
            call(seed=1, sample_streams=bad)


def test_the_earlier_refusals_come_first_and_stay(model):
    with pytest.raises(NotImplementedError, match="FiLM"):
        model.generate_actions([[5, 6]], pixel_values=PX, use_film=True, do_sample=True, seed=1)
    with pytest.raises(ValueError, match="exactly one"):
        model.generate_actions([[5, 6]], do_sample=True, seed=1, return_logprobs=True)
    model.engine.fp8_frozen = True
    with pytest.raises(NotImplementedError, match="fp8"):
        model.generate_actions([[5, 6]], pixel_values=PX, return_logprobs=True)
    with pytest.raises(NotImplementedError, match="lm_head"):
        model.predict_action(torch.zeros(1, 4, dtype=torch.int64), action_head=None)


# ---------------------------------------------------------------------------------------------------------------- host-side refusals
@pytest.fixture(scope="module")
def lib():
    return H.load_library()


P = 4096            # a non-null 16-B aligned stand-in for a device pointer: refused calls never dereference it


def test_sample_tokens_argument_validation(lib):
    def f(logits=P, ldl=1016, B=2, V=1016, params=P, ids=P, lp=None, probs=None, ldp=0, out_ids=None, T=4, step=P, pos=P, emb=P, lde=64, xn=P, ldn=64, D=64):
        return lib.vla_sample_tokens(None, logits, ldl, B, V, params, None, ids, lp, probs, ldp, out_ids, T, step, pos, None, emb, 1000, lde, xn, ldn, D)
    assert f(logits=None) == -1 and f(params=None) == -1 and f(ids=None) == -1 and f(step=None) == -1 and b"null" in lib.vla_last_error()
    assert f(B=0) == -1 and f(B=65) == -1 and f(V=0) == -1 and b"B in [1, 64], V >= 1" in lib.vla_last_error()
    assert f(ldl=1015) == -1 and f(logits=P + 1) == -1 and b"ld_logits" in lib.vla_last_error()
    assert f(params=P + 4) == -1 and b"8-B aligned" in lib.vla_last_error()
    assert f(lp=P, T=0) == -1 and b"logprob_out needs T >= 1" in lib.vla_last_error()
    assert f(probs=P, ldp=1015) == -1 and b"ld_probs" in lib.vla_last_error()
    assert f(out_ids=P, T=0) == -1 and f(out_ids=P, pos=None) == -1 and f(out_ids=P, emb=None) == -1 and f(out_ids=P, xn=None) == -1 \
        and b"the advance needs" in lib.vla_last_error()
    assert f(out_ids=P, D=60) == -1 and f(out_ids=P, D=0) == -1 and f(out_ids=P, lde=56) == -1 and f(out_ids=P, ldn=68) == -1 \
        and f(out_ids=P, xn=P + 8) == -1 and f(out_ids=P, emb=P + 2) == -1 and b"embed / x_next" in lib.vla_last_error()


def test_wrappers_refuse_on_the_host_before_any_launch():
    from vla_adapter_amd import ops
    blk = ops.sample_params(temperature=0.7, top_k=50, top_p=0.9, seed=2 ** 64 - 1)
    assert blk.dtype == torch.uint8 and blk.numel() == ops.SAMPLE_PARAM_BYTES == 24
    import struct
    t, p, k, g, s = struct.unpack("<ffiiQ", bytes(blk.tolist()))
    assert (t, p, k, g, s) == (np.float32(0.7), np.float32(0.9), 50, 0, 2 ** 64 - 1)
    assert struct.unpack("<ffiiQ", bytes(ops.sample_params(greedy=True, seed=-1).tolist()))[3:] == (1, 2 ** 64 - 1)
    for kw, msg in ((dict(temperature=0), "temperature"), (dict(top_k=-1), "top_k"), (dict(top_p=0), "top_p"), (dict(seed=1.0), "seed")):
        with pytest.raises(ValueError, match=msg):
            ops.sample_params(**kw)
    step = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="bf16 \\[B, V\\] device tensor"):
        ops.sample_tokens(torch.zeros(2, 8, dtype=torch.bfloat16), blk, step)               # logits on the host
    with pytest.raises(ValueError, match="bf16 \\[B, V\\] device tensor"):
        ops.sample_tokens(torch.zeros(2, 8), blk, step)


# ---------------------------------------------------------------------------------------------------------------- the registry's open end
KEYS = [fam.key for fam in native.OPEN_FAMILIES]
# per family: the argument count of every entry point, the files the csrc Makefile must name, and where its memory-contract cases live
FAMILY = {
    "sample": ({"vla_sample_tokens": 22}, ("sample.hip", "vla_sample.h", "decode_advance.h", "argmax_order.h"), "test_sample_memory_contract_gpu"),
}


def test_the_open_end_stands_behind_the_pinned_tuples():
    from tests import test_abi_decode_family as ADDED
    assert KEYS == list(FAMILY)
    assert native.ALL_FAMILIES == native.FAMILIES + native.LATER_FAMILIES + native.ADDED_FAMILIES, "ALL_FAMILIES is unchanged"
    assert [fam.key for fam in native.ADDED_FAMILIES] == ADDED.KEYS == list(ADDED.FAMILY)
    assert not set(KEYS) & {fam.key for fam in native.ALL_FAMILIES}, "no key of a pinned family"
    names = [n for fam in native.OPEN_FAMILIES for n in fam.protos]
    assert len(names) == len(set(names)) == len(native.OPEN_PROTOS)
    assert not set(names) & {n for fam in native.ALL_FAMILIES for n in fam.protos}, "an entry point belongs to one header"
    assert all(native.family(k) is fam and isinstance(fam, native.Family) and fam.header == "vla_" + k + ".h" for k, fam in zip(KEYS, native.OPEN_FAMILIES))
    for name in names:
        assert name not in H.header_text("vla_native.h") and name not in H.header_text("vla_decode.h")
    assert native.ABI_VERSION == 8, "VLA_ABI_VERSION does not move for an added family"


@pytest.mark.parametrize("key", KEYS)
def test_header_table_library_and_makefile_agree(key):
    fam, (pinned, files, _) = native.family(key), FAMILY[key]
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
    M = importlib.import_module("tests." + FAMILY[key][2])
    table = set(native.family(key).protos)
    covered, exempt = set(M.COVERED), set(M.EXEMPT)
    assert not (covered | exempt) - table and not covered & exempt and not table - covered - exempt
    for name, reason in M.EXEMPT.items():
        assert isinstance(reason, str) and 4 <= len(reason) and "\n" not in reason, f"{name}: a one-line reason"
    for name, tests in M.COVERED.items():
        for t in tests:
            assert callable(getattr(M, t, None)), f"{name}: case {t} does not exist"


@pytest.mark.parametrize("key", KEYS)
def test_the_comparison_reports_a_doctored_header(key):
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
    assert C.sizeof(C.c_longlong) == 8
