"""The display transform without a GPU (include/ptc.h: ptc_set_display ... ptc_get_display_seconds, ptc_debug_display_pixel, ptc_debug_meter): symbols, defaults
and the validation table, the host evaluation of csrc/pt_display.h against its numpy restatement (tests/display_reference.py) bit for bit — operators, transfer
functions, RGBA16F, metering, adaptation —, the ACES default against the oracle's tonemapper, PBR Neutral against the Khronos formula in float64, and the
identities the metering's definition promises."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import display_reference as ref  # noqa: E402

NEW = ("ptc_display_default_params", "ptc_set_display", "ptc_get_display", "ptc_meter_exposure", "ptc_exposure_reset", "ptc_get_exposure",
       "ptc_read_luminance_histogram", "ptc_display_rgba8", "ptc_display_rgba16f", "ptc_display_rgba16f_device_ptr", "ptc_get_display_seconds",
       "ptc_debug_display_pixel", "ptc_debug_meter", "ptc_debug_display_internals", "ptc_debug_display_state")
E_ARG, E_STATE, E_DEVICE = -1, -2, -3
F32, F64, U32 = np.float32, np.float64, np.uint32
OPERATORS = (ref.ACES, ref.NEUTRAL, ref.REINHARD, ref.CLAMP)
OETFS = (ref.GAMMA22, ref.SRGB)


def _ctx(pbr):
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE)
    assert pbr.load_library().ptc_scene_begin(pt._h) == 0
    return pt


def _meter_both(pbr, img, A=0, **fields):
    got = pbr.ptc.meter(img, state=A, **fields)
    want = ref.meter(img, ref.params(**fields), A)
    return got, want


def _assert_same_metering(got, want, what=""):
    for k in ("A", "Q", "N", "M", "rejected"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.array_equal(got["hist"], want["hist"]), what


def test_symbols_defaults_round_trip_and_validation(pbr):
    header = open(os.path.join(ROOT, "include", "ptc.h")).read()
    L = pbr.load_library()
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in pbr.ptc.ABI_SYMBOLS and hasattr(L, sym) and getattr(L, sym).argtypes is not None, sym
    assert re.search(r"typedef struct ptc_display_params \{", header)
    assert "#define PTC_ABI_VERSION 4" in header and L.ptc_abi_version() == 4            # additive: the ABI version stays
    assert C.sizeof(pbr.ptc.PtcDisplayParams) == 44
    d = pbr.ptc.display_default_params()
    want = {k: (v if isinstance(v, int) else float(F32(v))) for k, v in ref.DEFAULTS.items()}
    assert d == want
    pt = _ctx(pbr)
    assert pt.get_display() == want                                                      # a fresh context holds the defaults
    changed = dict(gain=2.5, auto_exposure=1, key=0.25, percentile_lo=0.0, percentile_hi=1.0, adapt_rate=0.5, min_luminance=0.5, max_luminance=0.5,
                   tonemap=pbr.ptc.TONEMAP_REINHARD, white=2.0, oetf=pbr.ptc.OETF_SRGB)
    pt.set_display(**changed)
    assert pt.get_display() == changed
    assert L.ptc_scene_begin(pt._h) == 0 and pt.get_display() == changed                 # a context setting: kept across ptc_scene_begin
    nan, inf = float("nan"), float("inf")
    refused = [("gain", 0.0), ("gain", -1.0), ("gain", nan), ("gain", inf), ("auto_exposure", 2), ("auto_exposure", -1), ("key", 0.0), ("key", nan), ("key", inf),
               ("percentile_lo", -0.01), ("percentile_lo", 1.0), ("percentile_lo", nan), ("percentile_hi", 0.0), ("percentile_hi", 1.01), ("percentile_hi", nan),
               ("adapt_rate", -0.1), ("adapt_rate", 1.1), ("adapt_rate", nan), ("min_luminance", 0.0), ("min_luminance", nan), ("min_luminance", inf),
               ("max_luminance", 0.25), ("max_luminance", inf), ("max_luminance", nan), ("tonemap", -1), ("tonemap", 4), ("white", 0.0), ("white", nan),
               ("white", inf), ("oetf", 2), ("oetf", -1)]
    for field, value in refused:
        p = pbr.ptc.PtcDisplayParams(**changed)
        setattr(p, field, value)
        assert L.ptc_set_display(pt._h, C.byref(p)) == E_ARG, (field, value)
        assert pt.get_display() == changed, (field, value)                               # nothing changed
    p = pbr.ptc.PtcDisplayParams(**dict(changed, percentile_lo=0.6, percentile_hi=0.6))  # lo < hi
    assert L.ptc_set_display(pt._h, C.byref(p)) == E_ARG and pt.get_display() == changed
    assert L.ptc_set_display(pt._h, None) == 0 and pt.get_display() == want              # NULL: the defaults
    assert pt.set_display().get_display() == want
    # the device calls on a description-only context
    buf8, buf16, hist = (C.c_uint8 * 4)(), (C.c_uint16 * 4)(), (C.c_uint32 * 4096)()
    dbl = C.c_double(0)
    assert L.ptc_meter_exposure(pt._h) == E_DEVICE and L.ptc_exposure_reset(pt._h) == E_DEVICE
    assert L.ptc_get_exposure(pt._h, None, None, None, None, None) == E_DEVICE
    assert L.ptc_read_luminance_histogram(pt._h, hist) == E_DEVICE
    assert L.ptc_display_rgba8(pt._h, buf8) == E_DEVICE and L.ptc_display_rgba16f(pt._h, buf16) == E_DEVICE
    assert not L.ptc_display_rgba16f_device_ptr(pt._h)
    assert L.ptc_get_display_seconds(pt._h, C.byref(dbl), None) == E_DEVICE
    assert "no device" in L.ptc_last_error(pt._h).decode()
    assert pt.display_internals()[0] > 0                                                 # the grid's coverage needs no device
    assert pbr.ptc.ev_to_gain(0) == 1.0 and pbr.ptc.ev_to_gain(-3) == 0.125 and pbr.ptc.ev_to_gain(0.5) == float(F32(2.0 ** 0.5))
    # the hooks refuse what ptc_set_display refuses
    bad = pbr.ptc.PtcDisplayParams(**dict(changed, white=-1.0))
    px = (C.c_float * 4)(1, 1, 1, 1)
    assert L.ptc_debug_display_pixel(C.byref(bad), 1.0, px, buf8, buf16) == E_ARG
    assert L.ptc_debug_display_pixel(None, 1.0, None, buf8, buf16) == E_ARG
    assert L.ptc_debug_meter(C.byref(bad), px, 1, 0, None, None, None, None, None, None) == E_ARG


@pytest.fixture(scope="module")
def colours():
    px = ref.colours()
    assert 3500 <= len(px) <= 4500
    return px


@pytest.mark.parametrize("oetf", OETFS)
@pytest.mark.parametrize("op", OPERATORS)
def test_pixel_hook_equals_reference_bit_for_bit(pbr, colours, op, oetf):
    for E in ref.EXPOSURES:
        got8, got16 = pbr.ptc.display_pixels(colours, E, tonemap=op, oetf=oetf, white=3.0)
        want8 = ref.display_rgba8(colours, E, ref.params(tonemap=op, oetf=oetf, white=3.0))
        want16 = ref.display_rgba16f(colours, E)
        bad = np.flatnonzero((got8 != want8).any(axis=1))
        assert bad.size == 0, (E, colours[bad[:4]], got8[bad[:4]], want8[bad[:4]])
        bad = np.flatnonzero((got16 != want16).any(axis=1))
        assert bad.size == 0, (E, colours[bad[:4]], got16[bad[:4]], want16[bad[:4]])


def test_non_finite_pixels_are_what_the_header_says(pbr):
    nan, inf = np.nan, np.inf
    rgb = lambda c, **kw: pbr.ptc.display_pixels([list(c) + [1.0]], 1.0, **kw)[0][0, :3].tolist()
    assert rgb((nan, 1, 1), tonemap="clamp") == [0, 255, 255] and rgb((inf, 0, -inf), tonemap="clamp") == [255, 0, 0]
    assert rgb((nan, 1, 1)) == [0, 0, 0] and rgb((1, inf, 1)) == [0, 0, 0] and rgb((1, 1, -inf)) == [0, 0, 0]             # ACES mixes the channels
    ok = rgb((0.5, 1, 1), tonemap="reinhard")
    assert rgb((nan, 1, 1), tonemap="reinhard")[0] == 0 and rgb((1, inf, 1), tonemap="reinhard") == [0, 0, 0] and ok[0] > 0
    assert rgb((inf, 1, 1), tonemap="neutral") == [0, 255, 255] and rgb((-inf, 1, 1), tonemap="neutral") == [0, 0, 0]
    a8, a16 = pbr.ptc.display_pixels([[1, 1, 1, nan], [1, 1, 1, -2], [1, 1, 1, inf], [nan, 1e6, -1e6, 0.5]], 1.0)
    assert a8[:, 3].tolist() == [0, 0, 255, 128]
    assert a16[3].tolist() == [0x7E00, 0x7C00, 0xFC00, 0x3800]                           # NaN, overflow to +-inf, alpha copied


def test_aces_default_equals_the_oracle_tonemapper(pbr, ora):
    rng = np.random.default_rng(3)
    px = np.concatenate([rng.uniform(-0.1, 2.0, (3000, 4)), 10.0 ** rng.uniform(-6, 4, (3000, 4)), rng.uniform(-0.1, 1e4, (500, 4))]).astype(F32)
    assert np.isfinite(px).all() and px.min() >= -0.1 and px.max() <= 1e4
    got8, _ = pbr.ptc.display_pixels(px, 1.0)
    assert np.array_equal(got8, ora.tonemap_rgba8(px))


def test_pbr_neutral_against_the_khronos_formula_in_float64(pbr):
    """Inputs in [0, 64].  Measured on these inputs, numpy float32 restatement against the float64 formula: 1.39e-7 after the operator, 4.73e-6 after the
    gamma-2.2 encoding (pt_pow's polynomials), 7.77e-7 after the sRGB encoding.  The tolerances are twice that; the hook's byte is the rounding of 255 v, so it
    may lie half a step plus 255 times the tolerance from the float64 value."""
    measured = {"linear": 1.39e-7, ref.GAMMA22: 4.73e-6, ref.SRGB: 7.77e-7}
    rng = np.random.default_rng(11)
    rgb = np.concatenate([rng.uniform(0, 64, (20000, 3)), 2.0 ** rng.uniform(-10, 6, (20000, 3)), np.repeat(rng.uniform(0, 64, (2000, 1)), 3, 1)]).astype(F32)
    px = np.concatenate([rgb, np.ones((len(rgb), 1), F32)], axis=1)
    lin64 = ref.neutral(rgb[:, 0], rgb[:, 1], rgb[:, 2], dt=F64)
    lin32 = ref.neutral(rgb[:, 0], rgb[:, 1], rgb[:, 2])
    dev = max(float(np.abs(a.astype(F64) - b).max()) for a, b in zip(lin32, lin64))
    print(f"neutral, float32 restatement vs float64: {dev:.3e} after the operator")
    assert dev <= 2 * measured["linear"]
    assert all(0.0 <= v.min() and v.max() <= 1.0 for v in lin64) and all(0.0 <= v.min() and v.max() <= 1.0 for v in lin32)      # the output lies in [0, 1]
    for oetf in OETFS:
        enc64 = []
        for v in lin64:
            enc64.append(np.where(v <= 0.0031308, 12.92 * v, 1.055 * v ** (1 / 2.4) - 0.055) if oetf == ref.SRGB else v ** (1 / 2.2))
        enc32 = ref.display_encoded(px, 1.0, ref.params(tonemap=ref.NEUTRAL, oetf=oetf))
        dev = max(float(np.abs(a.astype(F64) - b).max()) for a, b in zip(enc32, enc64))
        print(f"neutral, oetf {oetf}: {dev:.3e} after the encoding")
        assert dev <= 2 * measured[oetf]
        got8, _ = pbr.ptc.display_pixels(px[::8], 1.0, tonemap="neutral", oetf=oetf)
        for k in range(3):
            assert np.abs(got8[:, k].astype(F64) - 255.0 * enc64[k][::8]).max() <= 0.5 + 255.0 * 2 * measured[oetf]
    # along grey: grey stays grey, and the bytes do not fall as the exposure rises
    grey = np.ones((1, 4), F32) * F32(0.37)
    last = -1
    for E in 2.0 ** np.arange(-14, 12, 0.25):
        got8, _ = pbr.ptc.display_pixels(grey, float(F32(E)), tonemap="neutral", oetf="srgb")
        r, g, b, a = got8[0].tolist()
        assert r == g == b and r >= last and a == 94                # alpha 0.37: not exposed
        last = r
    assert last == 255 or last >= 250


def test_metering_hook_equals_reference_bit_for_bit(pbr):
    keys = ref.all_keys_image()
    want = ref.meter(keys, ref.params())
    assert (want["hist"][:4080] >= 1).all() and want["hist"][4080:].sum() == 0 and want["N"] == 4081       # every key that can be metered, FLT_MAX included
    images = {"all keys": keys, "random": ref.random_image(6000, 1), "random small": ref.random_image(37, 2), "special": ref.special_pixels(),
              "constant": np.tile(np.array([[0.3, 0.2, 0.1, 1.0]], F32), (500, 1)),
              "alpha 0": np.tile(np.array([[0.3, 0.2, 0.1, 0.0]], F32), (64, 1)),
              "rejected only": np.tile(np.array([[0.0, -1.0, 0.0, 1.0]], F32), (10, 1)), "empty": np.zeros((0, 4), F32)}
    settings = [dict(), dict(percentile_lo=0.0, percentile_hi=1.0), dict(percentile_lo=0.45, percentile_hi=0.55), dict(percentile_lo=0.0, percentile_hi=0.01),
                dict(percentile_lo=0.99, percentile_hi=1.0), dict(adapt_rate=0.3)]
    for name, img in images.items():
        for kw in settings:
            for A in (0, 0x3F000000):
                got, want = _meter_both(pbr, img, A, **kw)
                _assert_same_metering(got, want, (name, kw, A))
    got, _ = _meter_both(pbr, images["alpha 0"])
    assert got["N"] == 0 and got["rejected"] == 0 and got["M"] == 0 and got["Q"] == 0                       # alpha 0 is not counted at all
    got, _ = _meter_both(pbr, images["rejected only"], 0x3F000000)
    assert got["N"] == 0 and got["rejected"] == 10 and got["A"] == 0x3F000000                              # M = 0 leaves the state alone
    got, _ = _meter_both(pbr, ref.special_pixels())
    assert got["rejected"] > 20 and got["N"] >= 5
    three = np.array([[1, 1, 1, 1], [4, 4, 4, 1], [16, 16, 16, 1]], F32)                                   # n_lo = n_hi = 0: n_hi <= n_lo keeps all
    got, want = _meter_both(pbr, three, percentile_lo=0.1, percentile_hi=0.3)
    _assert_same_metering(got, want)
    assert got["N"] == 3 and got["M"] == 3


def test_metering_identities(pbr):
    # a constant image of luminance L meters within half a bin of L: a factor 1 +- 1/32
    rng = np.random.default_rng(5)
    worst = 0.0
    for L in 2.0 ** rng.uniform(-30, 30, 300):
        img = np.tile(np.array([[L, L, L, 1.0]], F32), (16, 1))
        got = pbr.ptc.meter(img)
        lum = float(ref.lum(img[0, 0], img[0, 1], img[0, 2]))
        m = float(ref.as_float(U32(got["Q"]))[0])
        worst = max(worst, abs(m / lum - 1.0))
    assert worst <= 1.0 / 32.0, worst
    # half the pixels at 2^-3 and half at 2^5: the geometric mean 2 at its bin's centre
    img = np.ones((128, 4), F32)
    img[:64, :3], img[64:, :3] = 2.0 ** -3, 2.0 ** 5
    got = pbr.ptc.meter(img, percentile_lo=0.0, percentile_hi=1.0)
    assert float(ref.as_float(U32(got["Q"]))[0]) == 2.0625
    # a bright decile is trimmed away: 10 % of the pixels at 1e6 over a 0.2 field meter what the field alone does
    field = np.tile(np.array([[0.2, 0.2, 0.2, 1.0]], F32), (1000, 1))
    lit = field.copy()
    lit[::10, :3] = 1e6
    a = pbr.ptc.meter(lit, percentile_lo=0.0, percentile_hi=0.9)
    b = pbr.ptc.meter(field, percentile_lo=0.0, percentile_hi=0.9)
    assert a["Q"] == b["Q"] and a["N"] == 1000 and a["M"] == (1000 * int(F32(0.9) * F32(65536.0))) >> 16 == 899      # hi_q = 58982: below 0.9 x 65536
    assert pbr.ptc.meter(lit, percentile_lo=0.0, percentile_hi=1.0)["Q"] > a["Q"]


@pytest.mark.parametrize("rate", [0.0, 0.25, 0.5, 1.0])
def test_adaptation_follows_the_integer_recurrence(pbr, rate):
    levels = [0.2, 0.2, 50.0, 50.0, 50.0, 1e-3, 1e5, 1e5, 0.18, 0.18, 0.18]
    A = 0
    for i, L in enumerate(levels):
        img = np.tile(np.array([[L, L, L, 1.0]], F32), (8, 1))
        got = pbr.ptc.meter(img, state=A, adapt_rate=rate)
        Q = got["Q"]
        rq = int(F32(rate) * F32(65536.0))
        want = Q if (A == 0 or rq == 65536) else A + ((Q - A) * rq) // 65536
        assert got["A"] == want == ref.adapt(A, Q, got["M"], rate), (i, L)
        if i == 0:
            assert got["A"] == Q                                   # no state: the first metering is taken at once, whatever the rate
        elif rate == 0.0:
            assert got["A"] == A
        A = got["A"]
    if rate == 0.5:      # between two fixed levels the step is half the distance, rounded down: the floor, also of a negative distance
        lo = np.tile(np.array([[0.01, 0.01, 0.01, 1.0]], F32), (8, 1))
        hi = np.tile(np.array([[300.0, 300.0, 300.0, 1.0]], F32), (8, 1))
        for start, target in ((lo, hi), (hi, lo)):
            A = pbr.ptc.meter(start, adapt_rate=rate)["A"]
            Q = pbr.ptc.meter(target, adapt_rate=rate)["Q"]
            for _ in range(40):
                nxt = pbr.ptc.meter(target, state=A, adapt_rate=rate)["A"]
                assert nxt - A == (Q - A) // 2                     # Python's // floors
                A = nxt
            assert Q - A == (1 if target is hi else 0)             # from below the floor leaves one step, from above it arrives


def test_command_line_and_shim_without_a_device(pbr, tmp_path):
    """ptc_render reports bad display flags before any device work; viewer_shim's optional `exposure` mode changes nothing for a description-only run."""
    import subprocess

    lib = os.path.dirname(pbr.ptc.LIB_PATH)
    exe, out = os.path.join(lib, "ptc_render"), str(tmp_path / "x.pfm")
    run = lambda *args: subprocess.run([exe, "--scene", "cornell", "--width", "8", "--height", "8", "--spp", "1", "--out", out] + list(args), capture_output=True, text=True, timeout=60)
    r = run("--tonemap", "filmic")
    assert r.returncode == 2 and "--tonemap aces|neutral|reinhard|clamp" in r.stderr
    r = run("--key", "0.3")
    assert r.returncode == 1 and "--key K sets the target of --auto-exposure" in r.stderr
    r = run("--auto-exposure", "--key", "-1")
    assert r.returncode == 1 and "--key K: a finite value > 0" in r.stderr
    r = run("--exposure", "400")
    assert r.returncode == 1 and "--exposure EV" in r.stderr
    shim = os.path.join(lib, "viewer_shim")
    plain = subprocess.run([shim, "-1", "2"], capture_output=True, text=True, timeout=60)
    exposed = subprocess.run([shim, "-1", "2", "1.2", "exposure"], capture_output=True, text=True, timeout=60)
    assert plain.returncode == 0 and exposed.returncode == 0 and plain.stdout == exposed.stdout
