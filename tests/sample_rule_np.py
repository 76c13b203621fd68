"""One decoding step of the sampler (include/vla_sample.h, csrc/sample.hip) for one row, restated in float64.

The row is the bf16 logits l[0..V) that vla_decode_lm_head_argmax stores, passed as a float32 array of bf16-representable values.
  temperature   z = l / temperature in float32 (correctly rounded, as the device divides), then everything in float64;
  top-k         keep z >= the k-th largest z, ties kept (TopKLogitsWarper); 0 switches it off, k >= V keeps everything;
  top-p         over the softmax of what top-k kept: the classes of equal z in ascending order, a class dropped while the cumulative
                probability through it is <= 1 - top_p; the largest class is always kept (TopPLogitsWarper at the granularity of values);
  draw          token = argmax over the kept v of z[v] + g[v], g = -log(-log(u)), u = ((r >> 41) + 0.5) / 2^23 with
                r = splitmix64_key(splitmix64_key(splitmix64_key(seed ^ SAMPLE_STREAM, stream), t), v); the lowest id among equal sums;
  logprob       z[token] - logsumexp(z over the kept tokens);
  greedy        token = the argmax of l (lowest id among equals, the first NaN above everything), logprob = log_softmax(l)[token];
  non-finite    a row with a NaN or +inf logit, or whose largest logit is -inf: the greedy token, logprob NaN, probabilities NaN.
u takes the top 23 bits of r: (n + 0.5) / 2^23 = (2 n + 1) / 2^24 has 24 significant bits, so it is exact in float32 and lies in
[2^-24, 1 - 2^-24]; 24 bits of r would need 25 and round to 1.0 at the top."""
import numpy as np

SAMPLE_STREAM = 0x5A3D1E70C0DE5          # csrc/sample.hip
_M64 = (1 << 64) - 1


def splitmix64_key(seed, idx):
    """csrc/common.h: the splitmix64 finaliser of seed + idx * golden ratio.  Python integers or uint64 arrays (idx)."""
    if isinstance(idx, np.ndarray):
        with np.errstate(over="ignore"):
            z = np.uint64(seed & _M64) + idx.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            return z ^ (z >> np.uint64(31))
    z = ((seed & _M64) + (idx & _M64) * 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def draw_bits(seed: int, stream: int, t: int, V: int) -> np.ndarray:
    """r[v], uint64 [V]: a function of (seed, stream, t, v) and nothing else."""
    base = splitmix64_key(splitmix64_key((seed & _M64) ^ SAMPLE_STREAM, stream), t)
    return splitmix64_key(base, np.arange(V, dtype=np.uint64))


def uniform(r: np.ndarray) -> np.ndarray:
    """u = ((r >> 41) + 0.5) / 2^23 in float64: exactly the float32 value the device forms."""
    return ((r >> np.uint64(41)).astype(np.float64) + 0.5) / float(1 << 23)


def gumbel(seed: int, stream: int, t: int, V: int) -> np.ndarray:
    return -np.log(-np.log(uniform(draw_bits(seed, stream, t, V))))


def greedy_token(l: np.ndarray) -> int:
    nan = np.flatnonzero(np.isnan(l))
    return int(nan[0]) if nan.size else int(np.flatnonzero(l == l.max())[0])


def non_finite(l: np.ndarray) -> bool:
    return bool(np.isnan(l).any() or np.isposinf(l).any() or l.max() == -np.inf)


def scale(l: np.ndarray, temperature: float) -> np.ndarray:
    with np.errstate(all="ignore"):
        return (np.asarray(l, np.float32) / np.float32(temperature)).astype(np.float64)


def logsumexp(z: np.ndarray) -> float:
    m = z.max()
    return float(m + np.log(np.exp(z - m).sum()))


def keep(z: np.ndarray, top_k: int, top_p: float):
    """-> (kept bool [V], gap): gap = |cumulative probability - (1 - top_p)| at the class nearest to the top-p boundary (inf without
    top-p): how far the decision is from flipping."""
    V = z.shape[0]
    kept = np.ones(V, bool)
    if 1 <= top_k < V:
        kept = z >= np.sort(z)[V - top_k]
    gap = np.inf
    top_p = float(np.float32(top_p))
    if top_p < 1.0:
        p = np.where(kept, np.exp(z - logsumexp(z[kept])), 0.0)
        vals, cls = np.unique(z[kept], return_inverse=True)    # ascending; -0.0 and 0.0 are one value
        cum = np.cumsum(np.bincount(cls.ravel(), weights=p[kept], minlength=len(vals)))
        drop = cum <= 1.0 - top_p
        drop[-1] = False                                       # the largest class is always kept
        gap = float(np.abs(cum[:-1] - (1.0 - top_p)).min()) if len(vals) > 1 else np.inf
        kept = kept & np.isin(z, vals[~drop])
    return kept, gap


def step(l, temperature=1.0, top_k=0, top_p=1.0, seed=0, stream=0, t=0, greedy=False) -> dict:
    """-> token, logprob, probs float64 [V] (0 for a removed token), kept bool [V], margin (best minus second-best z + g; inf for one
    kept token or greedy), gap (keep())."""
    l = np.asarray(l, np.float32)
    V = l.shape[0]
    if non_finite(l):
        return dict(token=greedy_token(l), logprob=np.nan, probs=np.full(V, np.nan), kept=np.ones(V, bool), margin=np.inf, gap=np.inf)
    if greedy:
        z = l.astype(np.float64)
        lse = logsumexp(z)
        tok = greedy_token(l)
        return dict(token=tok, logprob=float(z[tok] - lse), probs=np.exp(z - lse), kept=np.ones(V, bool), margin=np.inf, gap=np.inf)
    z = scale(l, temperature)
    kept, gap = keep(z, int(top_k), top_p)
    lse = logsumexp(z[kept])
    score = np.where(kept, z + gumbel(seed, stream, t, V), -np.inf)
    tok = int(np.argmax(score))                                # (numpy's argmax: the first of equal values)
    rest = np.delete(score, tok)
    margin = float(score[tok] - rest.max()) if kept.sum() > 1 else np.inf
    return dict(token=tok, logprob=float(z[tok] - lse), probs=np.where(kept, np.exp(z - lse), 0.0), kept=kept, margin=margin, gap=gap)
