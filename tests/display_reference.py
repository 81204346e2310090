"""numpy restatement of the display transform (csrc/pt_display.h), for tests/test_display_host.py and tests/test_gpu_display.py.

Floating point is float32 in the order the header writes it (numpy's + - * / on float32 arrays are correctly rounded, and every intermediate is an array of
that type, so each operation rounds once); a fused multiply-add is lens_reference's round-to-odd `_fma`.  fmin2 / fmax2 are the header's selects, not
numpy's minimum / maximum: they decide what a NaN gives.  The metering is in Python integers.  `neutral(..., dt=F64)` evaluates the Khronos formula in
float64: the yardstick of the operator's accuracy test."""
import numpy as np

from lens_reference import _fma

F32, F64, U32 = np.float32, np.float64, np.uint32
ACES, NEUTRAL, REINHARD, CLAMP = 0, 1, 2, 3
GAMMA22, SRGB = 0, 1
BINS = 4096
DEFAULTS = dict(gain=1.0, auto_exposure=0, key=0.18, percentile_lo=0.1, percentile_hi=0.9, adapt_rate=1.0, min_luminance=1e-4, max_luminance=1e6,
                tonemap=ACES, white=4.0, oetf=GAMMA22)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def fmin2(a, b):
    a, b = np.broadcast_arrays(a, b)
    return np.where(a < b, a, b)


def fmax2(a, b):
    a, b = np.broadcast_arrays(a, b)
    return np.where(a > b, a, b)


def bits(x):
    return np.ascontiguousarray(x, F32).view(U32)


def as_float(u):
    return np.ascontiguousarray(u, U32).view(F32)


def lum(r, g, b, dt=F32):
    return (dt(0.2126) * r + dt(0.7152) * g) + dt(0.0722) * b


# ---- pt_pow ------------------------------------------------------------------------------------------------------------------------------------------
def pt_log2(x):
    u = bits(x)
    e = ((u >> U32(23)) & U32(0xFF)).astype(np.int32) - np.int32(127)
    m = as_float((u & U32(0x007FFFFF)) | U32(0x3F800000))
    big = m > F32(1.41421356)
    m = np.where(big, m * F32(0.5), m)
    e = np.where(big, e + 1, e)
    z = (m - F32(1)) / (m + F32(1))
    z2 = z * z
    p = _fma(z2, _fma(z2, _fma(z2, _fma(z2, F32(0.3205989), F32(0.4121984)), F32(0.5770780)), F32(0.9617967)), F32(2.8853901))
    return _fma(z, p, e.astype(F32))


def pt_exp2(x):
    x = np.asarray(x, F32)
    zero = x < F32(-126)
    x = np.where(x > F32(127), F32(127), x)
    x = np.where(zero, F32(0), x)          # the lanes that return 0 take a harmless value through the rest
    fl = np.floor(x)
    f = x - fl
    p = _fma(f, _fma(f, _fma(f, _fma(f, _fma(f, F32(1.8775767e-3), F32(8.9893397e-3)), F32(5.5826318e-2)), F32(2.4015361e-1)), F32(6.9315308e-1)), F32(9.9999994e-1))
    scale = as_float(((fl.astype(np.int32) + 127).astype(U32)) << U32(23))
    return np.where(zero, F32(0), p * scale)


def pt_pow(x, y):
    x = np.asarray(x, F32)
    ok = x > F32(0)
    xs = np.where(ok, x, F32(1))
    return np.where(ok, pt_exp2(F32(y) * pt_log2(xs)), F32(0))


# ---- operators ---------------------------------------------------------------------------------------------------------------------------------------
def rrt_odt(c):
    num = c * (c + F32(0.0245786)) - F32(0.000090537)
    den = c * (F32(0.983729) * c + F32(0.4329510)) + F32(0.238081)
    return num / den


def aces(r, g, b):
    ir = F32(0.59719) * r + F32(0.07600) * g + F32(0.02840) * b
    ig = F32(0.35458) * r + F32(0.90834) * g + F32(0.13383) * b
    ib = F32(0.04823) * r + F32(0.01566) * g + F32(0.83777) * b
    fr, fg, fb = rrt_odt(ir), rrt_odt(ig), rrt_odt(ib)
    return (F32(1.60475) * fr + F32(-0.10208) * fg + F32(-0.00327) * fb,
            F32(-0.53108) * fr + F32(1.10813) * fg + F32(-0.07276) * fb,
            F32(-0.07367) * fr + F32(-0.00605) * fg + F32(1.07602) * fb)


def neutral(r, g, b, dt=F32):
    """Khronos PBR Neutral.  dt=F64: the formula with its decimal constants in float64 (startCompression = 0.8 - 0.04, desaturation = 0.15)."""
    if dt is F64:
        r, g, b = (np.asarray(v, F64) for v in (r, g, b))
        sc, d = 0.8 - 0.04, 1.0 - (0.8 - 0.04)
        x = np.minimum(r, np.minimum(g, b))
        off = np.where(x < 0.08, x - 6.25 * x * x, 0.04)
        r, g, b = r - off, g - off, b - off
        peak = np.maximum(r, np.maximum(g, b))
        hot = peak >= sc
        pk = np.where(hot, peak, 1.0)
        npk = 1.0 - d * d / (pk + d - sc)
        k = npk / pk
        q = 1.0 - 1.0 / (0.15 * (pk - npk) + 1.0)
        mix = lambda c: np.where(hot, (c * k) * (1.0 - q) + npk * q, c)
        return mix(r), mix(g), mix(b)
    x = fmin2(r, fmin2(g, b))
    off = np.where(x < F32(0.08), x - F32(6.25) * (x * x), F32(0.04))
    r, g, b = r - off, g - off, b - off
    peak = fmax2(r, fmax2(g, b))
    hot = peak >= F32(0.76)
    npk = F32(1) - (F32(0.24) * F32(0.24)) / ((peak + F32(0.24)) - F32(0.76))
    k = npk / peak
    q = F32(1) - F32(1) / (F32(0.15) * (peak - npk) + F32(1))
    iq, nq = F32(1) - q, npk * q
    mix = lambda c: np.where(hot, (c * k) * iq + nq, c)
    return mix(r), mix(g), mix(b)


def reinhard(r, g, b, white):
    l = fmax2(lum(r, g, b), F32(0))
    w = F32(white)
    s = (F32(1) + l / (w * w)) / (F32(1) + l)
    return r * s, g * s, b * s


def oetf(v, which):
    if which == SRGB:
        return np.where(v <= F32(0.0031308), F32(12.92) * v, F32(1.055) * pt_pow(v, F32(1) / F32(2.4)) - F32(0.055))
    return pt_pow(v, F32(1) / F32(2.2))


def unorm8(v):
    v = fmin2(fmax2(v, F32(0)), F32(1))
    return (v * F32(255) + F32(0.5)).astype(np.int32).astype(U32)


def display_encoded(rgba, E, p):
    """(..., 4) float32 -> the three colour channels after exposure, operator and transfer function, before the clamp and the quantisation (float32)."""
    with np.errstate(all="ignore"):
        px = np.asarray(rgba, F32)
        E = F32(E)
        r, g, b = px[..., 0] * E, px[..., 1] * E, px[..., 2] * E
        op = p["tonemap"]
        if op == ACES:
            r, g, b = aces(r, g, b)
        elif op == NEUTRAL:
            r, g, b = neutral(r, g, b)
        elif op == REINHARD:
            r, g, b = reinhard(r, g, b, p["white"])
        return [oetf(fmax2(v, F32(0)), p["oetf"]) for v in (r, g, b)]


def display_rgba8(rgba, E, p):
    """(..., 4) float32 -> (..., 4) uint8: c = rgb E, operator, transfer function, quantisation; alpha: clamp and quantisation."""
    with np.errstate(all="ignore"):
        out = [unorm8(v) for v in display_encoded(rgba, E, p)] + [unorm8(np.asarray(rgba, F32)[..., 3])]
        return np.stack(out, axis=-1).astype(np.uint8)


def half_bits(v):
    with np.errstate(all="ignore"):
        v = np.asarray(v, F32)
        h = np.ascontiguousarray(v.astype(np.float16)).view(np.uint16)
        return np.where(np.isnan(v), np.uint16(0x7E00), h)


def display_rgba16f(rgba, E):
    """(..., 4) float32 -> (..., 4) uint16 bit patterns of half(rgb E), alpha copied."""
    with np.errstate(all="ignore"):
        px = np.asarray(rgba, F32)
        E = F32(E)
        return np.stack([half_bits(px[..., 0] * E), half_bits(px[..., 1] * E), half_bits(px[..., 2] * E), half_bits(px[..., 3])], axis=-1)


# ---- metering ----------------------------------------------------------------------------------------------------------------------------------------
def quantise(x):
    """(uint32)(x * 65536.0f) of the percentiles and the rate."""
    return int(F32(x) * F32(65536.0))


def histogram(rgba):
    """(hist (4096,) uint32, rejected) of the pixels (..., 4)."""
    with np.errstate(all="ignore"):
        px = np.asarray(rgba, F32).reshape(-1, 4)
        l = lum(px[:, 0], px[:, 1], px[:, 2])
        counted = px[:, 3] > F32(0)
        ok = counted & (l > F32(0)) & np.isfinite(l)
        keys = bits(l[ok]) >> U32(19)
        return np.bincount(keys, minlength=BINS).astype(U32), int((counted & ~ok).sum())


def trimmed_mean(hist, p):
    """(Q, N, M) of a histogram, in Python integers."""
    h = [int(v) for v in hist]
    N = sum(h)
    n_lo, n_hi = (N * quantise(p["percentile_lo"])) >> 16, (N * quantise(p["percentile_hi"])) >> 16
    if n_hi <= n_lo:
        n_lo, n_hi = 0, N
    S = M = before = 0
    for k, c in enumerate(h):
        kept = max(0, min(before + c, n_hi) - max(before, n_lo))
        S += kept * (2 * k + 1)
        M += kept
        before += c
    return ((S << 18) // M if M else 0), N, M


def adapt(A, Q, M, rate):
    if M == 0:
        return A
    rq = quantise(rate)
    if A == 0 or rq == 65536:
        return Q
    return A + ((Q - A) * rq) // 65536          # Python's // floors


def meter(rgba, p, A=0):
    """One metering of the pixels (..., 4) from the state A: dict(A, Q, N, M, rejected, hist)."""
    hist, rejected = histogram(rgba)
    Q, N, M = trimmed_mean(hist, p)
    return {"A": adapt(A, Q, M, p["adapt_rate"]), "Q": Q, "N": N, "M": M, "rejected": rejected, "hist": hist}


def scale(p, A):
    """The exposure scale E (float32) of the state A."""
    if not p["auto_exposure"] or A == 0:
        return F32(p["gain"])
    La = fmin2(fmax2(as_float(U32(A)), F32(p["min_luminance"])), F32(p["max_luminance"]))
    return F32(F32(p["gain"]) * (F32(p["key"]) / F32(La)))


# ---- test inputs ---------------------------------------------------------------------------------------------------------------------------------------
EXPOSURES = (1.0, 2.0 ** -10, 3.7, 2.0 ** 12)
BREAKPOINTS = (0.08, 0.76, 0.8, 0.04, 0.0031308)      # x, peak, peak + the offset, the offset, the sRGB knee


def _around(v, k=3):
    out = [F32(v)]
    for d in (np.inf, -np.inf):
        x = F32(v)
        for _ in range(k):
            x = np.nextafter(x, F32(d))
            out.append(x)
    return out


def special_pixels():
    """Exact zeros, negative channels, NaN and +-inf in every channel position, alpha off the [0, 1] range."""
    nan, inf = np.nan, np.inf
    rows = [[0, 0, 0, 1], [0, 0, 0, 0], [-0.5, 0.3, 0.2, 1], [0.3, -0.5, 0.2, 1], [0.3, 0.2, -0.5, 1], [-1, -2, -3, 1], [1, 1, 1, 0], [1, 1, 1, -1],
            [1, 1, 1, 2], [1, 1, 1, 0.5], [1, 1, 1, nan], [1, 1, 1, inf], [1, 1, 1, -inf], [nan, nan, nan, 1], [inf, inf, inf, 1], [-inf, -inf, -inf, 1],
            [inf, -inf, 1, 1], [3.4028235e38, 3.4028235e38, 3.4028235e38, 1], [1e-40, 1e-41, 1e-42, 1]]
    for bad in (nan, inf, -inf):
        for k in range(3):
            for rest in (1.0, 0.01, 30.0):
                c = [rest, rest * 0.5, rest * 0.25, 1.0]
                c[k] = bad
                rows.append(c)
    return np.array(rows, F32)


def colours(seed=7):
    """About 4000 RGBA pixels: uniform in [-0.1, 20], log-uniform over 2^+-20, the special values, the operators' breakpoints and their float neighbours
    (as they are and divided by every exposure of EXPOSURES)."""
    rng = np.random.default_rng(seed)
    uni = np.concatenate([rng.uniform(-0.1, 20.0, (1500, 3)), np.ones((1500, 1))], axis=1)
    log = np.concatenate([2.0 ** rng.uniform(-20, 20, (1500, 3)), rng.choice([0.0, 0.25, 1.0], (1500, 1))], axis=1)
    grey = np.repeat(2.0 ** rng.uniform(-12, 8, (200, 1)), 3, axis=1)
    grey = np.concatenate([grey, np.ones((200, 1))], axis=1)
    brk = []
    for bp in BREAKPOINTS:
        for E in (1.0,) + EXPOSURES[1:]:
            for v in _around(F32(bp) / F32(E)):
                brk += [[v, v, v, 1], [v, F32(1) / F32(E), F32(1) / F32(E), 1], [v, v * F32(0.125), v * F32(0.125), 1]]
    return np.concatenate([uni.astype(F32), log.astype(F32), grey.astype(F32), special_pixels(), np.array(brk, F32)], axis=0)


def all_keys_image():
    """One grey pixel at the centre of every bin that can be metered (keys 0 .. 4079, denormals included), and one at FLT_MAX."""
    v = as_float(((2 * np.arange(4080, dtype=np.uint64) + 1) << np.uint64(18)).astype(U32))
    v = np.concatenate([v, [F32(3.4028235e38)]]).astype(F32)
    return np.stack([v, v, v, np.ones_like(v)], axis=-1)


def random_image(n, seed):
    """n pixels over 30 stops with some alpha-0, zero, negative, NaN and inf pixels among them."""
    rng = np.random.default_rng(seed)
    px = np.concatenate([(2.0 ** rng.uniform(-15, 15, (n, 1))) * rng.uniform(0.2, 1.0, (n, 3)), np.ones((n, 1))], axis=1).astype(F32)
    kind = rng.integers(0, 40, n)
    px[kind == 0, 3] = 0.0
    px[kind == 1, :3] = 0.0
    px[kind == 2, :3] *= F32(-1)
    px[kind == 3, 1] = np.nan
    px[kind == 4, 2] = np.inf
    return px
