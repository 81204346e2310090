#!/usr/bin/env python3
"""What the display transform costs at 1920x1080 (csrc/pt_display.hip): the metering (k_meter_hist + k_meter_reduce, with the memset of the histogram in front) on a
rendered atrium frame and on a constant image — every pixel in one bin, the worst case for the LDS atomics —, each display kernel, and ptc_tonemap_rgba8 as the
yardstick, in one process.
  device time   HIP events around the launches (ptc_get_display_seconds), median of --reps calls, each waited for
  queued        host clock around 100 calls queued back to back and one wait, per call: what a viewer's frame pays when nothing waits in between
  call time     host clock around display() and tonemap() (kernel + wait + the 8 MB copy to the host): ptc_tonemap_rgba8 keeps no events, so the yardstick is the
                difference of two calls that differ in their kernel only; `--one` under rocprofv3 --kernel-trace --stats gives the kernels' own times by name
Bytes: metering reads 16 B per pixel (33.2 MB), display reads 16 B and writes 4 B (8 B for RGBA16F) per pixel.  Nothing is gated.
`--one`: warmed, 20 calls of each kind: the run to put behind `rocprofv3 --kernel-trace --stats --` (k_meter_hist, k_meter_reduce, k_display_rgba8, k_display_half, k_tonemap).
usage: python3 tools/display_bench.py [--one] [--reps K] [--spp N]   (-> profiles/display_1080p.txt)"""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd"))
import numpy as np
import pbr_amd as pbr

ap = argparse.ArgumentParser()
ap.add_argument("--one", action="store_true")
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--spp", type=int, default=4)
a = ap.parse_args()
W, H = 1920, 1080
N = W * H
OPS = ("aces", "neutral", "reinhard", "clamp")
OETFS = ("gamma22", "srgb")


def med(v):
    return 1e6 * float(np.median(v))


pt = pbr.PathTracer(0).load_scene(pbr.scenes.atrium())
pt.set_display(auto_exposure=1)
frame = pt.render(W, H, a.spp, seed=1, max_bounces=8)
constant = np.tile(np.array([0.3, 0.2, 0.1, 1.0], np.float32), (H, W, 1))
out = {"size": [W, H], "spp": a.spp, "reps": a.reps, "bytes": {"meter": 16 * N, "display_rgba8": 20 * N, "display_half": 24 * N}}

if a.one:
    for k in range(22):      # the first two are the warm-up
        pt.meter_exposure(); pt.display(); pt.display_f16(); pt.tonemap()
        pt.set_display(tonemap="neutral", oetf="srgb"); pt.display(); pt.set_display(tonemap="aces", oetf="gamma22")
    pt.write_radiance(constant)
    for k in range(22):
        pt.meter_exposure()
    pt.sync()
    out["one"] = {"exposure": pt.exposure()}
    print(json.dumps(out))
    sys.exit(0)

# ---- metering on both images ----
for image_name, image in (("atrium", None), ("constant", constant)):
    if image is not None:
        pt.write_radiance(image)
    t = []
    for r in range(a.reps + 3):
        pt.exposure_reset()
        pt.meter_exposure()
        pt.sync()
        if r >= 3:
            t.append(pt.display_seconds()[0])
    state, hist = pt.exposure_state(), pt.luminance_histogram()
    t0 = time.perf_counter()
    for _ in range(100):
        pt.meter_exposure()
    pt.sync()
    q = (time.perf_counter() - t0) / 100
    out[f"meter_{image_name}"] = {"state": state, "bins_in_use": int((hist > 0).sum()), "largest_bin_share": float(hist.max()) / max(1, int(hist.sum())),
                                  "device_us_median": med(t), "device_us_min": 1e6 * float(np.min(t)), "device_us_max": 1e6 * float(np.max(t)), "queued_us_per_call": 1e6 * q,
                                  "GBps_at_median": 16 * N / float(np.median(t)) / 1e9}

# ---- display: every kernel on the rendered frame, exposed by its own metering ----
pt.write_radiance(frame)
pt.exposure_reset(); pt.meter_exposure()
out["exposure"] = pt.exposure()
disp = {}
for op in OPS:
    for oe in OETFS:
        pt.set_display(tonemap=op, oetf=oe)
        ts = []
        for r in range(a.reps + 3):
            pt.display()
            if r >= 3:
                ts.append(pt.display_seconds()[1])
        disp[f"{op}_{oe}"] = {"device_us_median": med(ts), "device_us_min": 1e6 * float(np.min(ts)), "GBps_at_median": 20 * N / float(np.median(ts)) / 1e9}
ts = []
for r in range(a.reps + 3):
    pt.display_f16()
    if r >= 3:
        ts.append(pt.display_seconds()[1])
disp["half"] = {"device_us_median": med(ts), "device_us_min": 1e6 * float(np.min(ts)), "GBps_at_median": 24 * N / float(np.median(ts)) / 1e9}
out["display"] = disp

# ---- the yardstick: ptc_tonemap_rgba8 against ptc_display_rgba8 with the defaults (the same bytes), as whole calls, alternating ----
pt.set_display()
pt.exposure_reset()
assert np.array_equal(pt.display(), pt.tonemap())
tt, td = [], []
for r in range(a.reps + 3):
    t0 = time.perf_counter(); pt.tonemap(); t1 = time.perf_counter(); pt.display(); t2 = time.perf_counter()
    if r >= 3:
        tt.append(t1 - t0); td.append(t2 - t1)
out["call_us"] = {"tonemap_median": med(tt), "display_defaults_median": med(td), "display_minus_tonemap": med(td) - med(tt)}
print(json.dumps(out))
