"""The evaluator's frame pipeline as a numpy rule (the reference's resize_image_for_policy: JPEG round trip, then TF's lanczos3 resize
with antialiasing), the truth the device and the stand-alone host program are compared with bit for bit.

Round trip: the forward half of a baseline 4:2:0 file as libjpeg writes it - jccolor.c rgb_ycc_convert, jcsample.c h2v2_downsample,
jfdctint.c jpeg_fdct_islow, the division-quantisation of jcdctmgr.c - joined to the inverse half of tests/jpeg_rule_np.py.  The
entropy coding between them is lossless and left out.  tests/test_policy_image_cpu.py pins both halves to Pillow: the quantised
coefficients to those of Pillow's file, the pixels to Pillow's decode of it.

Resize: TF's ScaleAndTranslate (ComputeSpansCore, Lanczos3 kernel, antialias) restated in float32, written as plain loops, on purpose
another shape than the vectorised input_stage.tf_lanczos3_spans.  TensorFlow itself is not pinned: its last bits, its pass order and
glibc's sinf (numpy's float32 sin stands in) are unconfirmed."""
import numpy as np

from tests import jpeg_rule_np as R

LUMA = [16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
        18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99]
CHROMA = [17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32


# ---------------------------------------------------------------------------------------------------------------- the round trip
def quant_table(base, quality: int) -> np.ndarray:
    """jpeg_set_quality: int64 [8, 8], natural order."""
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((np.array(base, dtype=np.int64) * s + 50) // 100, 1, 255).reshape(8, 8)


def FIX(x):
    return int(x * 65536 + 0.5)


def rgb_ycc(a):
    r, g, b = (a[..., i].astype(np.int64) for i in range(3))
    y = (FIX(.299) * r + FIX(.587) * g + FIX(.114) * b + 32768) >> 16
    cb = (-FIX(.16874) * r - FIX(.33126) * g + FIX(.5) * b + (128 << 16) + 32767) >> 16
    cr = (FIX(.5) * r - FIX(.41869) * g - FIX(.08131) * b + (128 << 16) + 32767) >> 16
    return y, cb, cr


def downsample_h2v2(c):
    s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
    bias = np.where(np.arange(s.shape[1]) % 2 == 0, 1, 2)
    return (s + bias) >> 2


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def fdct_1d(d, first: bool):
    """One pass of jpeg_fdct_islow over the last axis of an int64 array [..., 8]."""
    t0, t7, t1, t6 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7], d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5, t3, t4 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5], d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    o[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    o[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * 4433
    o[2], o[6] = _descale(z1 + t13 * 6270, n), _descale(z1 - t12 * 15137, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * 9633
    t4, t5, t6, t7 = t4 * 2446, t5 * 16819, t6 * 25172, t7 * 12299
    z1, z2, z3, z4 = -z1 * 7373, -z2 * 20995, -z3 * 16069 + z5, -z4 * 3196 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, -1)


def fdct_islow(plane):
    """uint8-valued [h, w] -> int64 [h / 8, w / 8, 8, 8]: rows first, then columns; the result carries the factor 8 the quantiser divides out."""
    h, w = plane.shape
    b = plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3).astype(np.int64) - 128
    b = fdct_1d(b, True)
    return np.swapaxes(fdct_1d(np.swapaxes(b, -1, -2), False), -1, -2)


def quantise(c, q):
    qv = q * 8
    t = (np.abs(c) + (qv >> 1)) // qv
    return np.where(c < 0, -t, t)


def jpeg_round_trip(a: np.ndarray, quality: int = 95, stats: dict = None) -> np.ndarray:
    """uint8 [H, W, 3], H and W multiples of 16 -> uint8 [H, W, 3]: the pixels of the frame's 4:2:0 baseline file of ``quality``.
    ``stats``, when given, receives "quantised": [Y, Cb, Cr] int64 [bh, bw, 64] in zigzag order, as jpeg_rule_np.decode reports them."""
    assert a.dtype == np.uint8 and a.ndim == 3 and a.shape[2] == 3 and a.shape[0] % 16 == 0 and a.shape[1] % 16 == 0
    y, cb, cr = rgb_ycc(a)
    planes = [y, downsample_h2v2(cb), downsample_h2v2(cr)]
    qs = [quant_table(LUMA, quality), quant_table(CHROMA, quality), quant_table(CHROMA, quality)]
    qc = [quantise(fdct_islow(p), q) for p, q in zip(planes, qs)]
    if stats is not None:
        stats["quantised"] = [c.reshape(c.shape[0], c.shape[1], 64)[..., R.ZIGZAG] for c in qc]
    pix = [R.idct_islow(c * q).transpose(0, 2, 1, 3).reshape(p.shape) for c, q, p in zip(qc, qs, planes)]
    return R.ycc_to_rgb(pix[0], R.upsample_h2v2(pix[1]), R.upsample_h2v2(pix[2]))


# ---------------------------------------------------------------------------------------------------------------- the resize
f32 = np.float32
PASS_ORDER = ("vertical", "horizontal")         # THE PASS ORDER of the rule (csrc/policy_image.hip states the same for the device)


def lanczos3_kernel(x):
    pi, r = f32(3.14159265359), f32(3.0)
    x = np.abs(x).astype(f32)
    with np.errstate(all="ignore"):
        v = (r * np.sin(pi * x) * np.sin(pi * x / r) / (pi * pi * x * x)).astype(f32)
    return np.where(x > r, f32(0), np.where(x <= f32(1e-3), f32(1), v)).astype(f32)


def spans(n_in: int, n_out: int):
    """(starts int32 [n_out], weights f32 [n_out, span], span) of one side, output by output."""
    scale = f32(n_out) / f32(n_in)
    inv = f32(1.0) / scale
    ks = max(inv, f32(1.0))
    oks, rad = f32(1.0) / ks, f32(3.0)
    span = min(2 * int(np.ceil(rad * ks)) + 1, n_in)
    starts, W = np.zeros(n_out, np.int32), np.zeros((n_out, span), f32)
    for x in range(n_out):
        s = f32(f32(x) + f32(0.5)) * inv
        a = int(np.ceil(f32(s - rad * ks) - f32(0.5)))
        b = int(np.floor(f32(s + rad * ks) - f32(0.5)))
        a, b = min(max(a, 0), n_in - 1), min(max(b, 0), n_in - 1) + 1
        w = lanczos3_kernel(np.abs(((np.arange(a, b).astype(f32) + f32(0.5)) - s) * oks))
        tot = f32(0)
        for t in w:
            tot = f32(tot + t)
        if abs(tot) >= 1000 * np.finfo(f32).tiny:
            w = (w * (f32(1) / tot)).astype(f32)
        starts[x], W[x, :b - a] = a, w
    return starts, W, span


def _pass(x, n_out):
    """One pass along axis 0 of a float32 array: acc = 0; acc += w * v over the span, in source order, every step rounded to float32."""
    st, w, sp = spans(x.shape[0], n_out)
    out = np.zeros((n_out,) + x.shape[1:], f32)
    for k in range(sp):
        idx = np.minimum(st.astype(np.int64) + k, x.shape[0] - 1)
        prod = (w[:, k].reshape((-1,) + (1,) * (x.ndim - 1)) * x[idx]).astype(f32)
        out = (out + prod).astype(f32)
    return out


def tf_lanczos3_resize(a: np.ndarray, out_h: int, out_w: int, order=PASS_ORDER, skip_equal: bool = True) -> np.ndarray:
    """uint8 [H, W, 3] -> uint8 [out_h, out_w, 3]: tf.image.resize(method="lanczos3", antialias=True), then round (half to even), clip,
    cast.  ``order``: which pass runs first, its result kept in float32.  ``skip_equal``: a side that does not change is not
    resampled, as the device has it (with both sides equal the input comes back untouched); False runs the pass all the same - at
    scale 1 its off-centre weights are sin(k pi) in float32, about 1e-8."""
    assert a.dtype == np.uint8 and a.ndim == 3
    x = a.astype(f32)
    for which in order:
        if which == "vertical":
            if x.shape[0] != out_h or not skip_equal:
                x = _pass(x, out_h)
        else:
            if x.shape[1] != out_w or not skip_equal:
                x = _pass(x.transpose(1, 0, 2), out_w).transpose(1, 0, 2)
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def policy_frame(a: np.ndarray, size: int = 224, quality: int = 95) -> np.ndarray:
    """resize_image_for_policy of one frame: the round trip, then the resize to size x size."""
    return tf_lanczos3_resize(jpeg_round_trip(a, quality), size, size)


def band_limited(seed: int = 3, n: int = 256) -> np.ndarray:
    """The 256 x 256 frame the resize is compared with Pillow's LANCZOS on: 128 + 50 sin cos + 8 sin + N(0, 2), values inside
    [64, 192], so that neither resampler clips."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:n, 0:n]
    a = np.stack([128 + 50 * np.sin(xx / 9.0 + c) * np.cos(yy / 7.0 - c) + 8 * np.sin(xx * 0.9 + yy * 0.7) for c in range(3)], -1)
    return np.clip(a + rng.normal(0, 2, a.shape), 0, 255).astype(np.uint8)
