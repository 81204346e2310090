"""What adaptive sampling buys at 1920x1080: the atrium and the textured atrium with max_spp 1024 at a few thresholds against the uniform 1024-spp frame,
alternating in one process (GPU box; -> profiles/adaptive_1080p.txt).

Per workload: a uniform high-spp reference with another seed; the uniform frame's relMSE = mean((x - ref)^2 / (ref^2 + 0.01)) at 16 ... 1024 spp from ONE
progressive frame (resolve at every level); then, three times over, the timed uniform frame and the timed adaptive frames: HIP-event time (ptc_stats.seconds_render
+ ptc_adaptive_stats.seconds_adapt), wall time around a ptc_sync, mean count, relMSE, and the uniform spp that reaches the same relMSE (log-log interpolation of
the curve) — the speed-up at equal quality is uniform time at that spp / adaptive time.

  python tools/adaptive_bench.py [atrium|textured|both] [--ref-spp N] [--max-spp N] [--reps N] [--size W H]
  python tools/adaptive_bench.py atrium --one THRESH      one warmed adaptive frame and nothing else: the run to put behind `rocprofv3 --kernel-trace --stats --`
                                                          for the k_ad_* rows (per-launch times, share of the frame)
  python tools/adaptive_bench.py atrium --sampled [--max-spp N] [--reps N]
                                                          what the per-sample covariance costs and ptc_denoise_sampled takes (-> profiles/sampled_variance_1080p.txt):
                                                          the adaptive render at the default threshold with ptc_set_sample_covariance on against off, alternating, and
                                                          the HIP-event time of ptc_denoise_sampled against ptc_denoise on the same frame.  With --one THRESH: one
                                                          warmed frame with the covariance on + guides + ptc_denoise_sampled, the run to put behind rocprofv3 for the
                                                          k_ad_accumulate<true> / k_ad_sampled_* rows"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd"))
import pbr_amd  # noqa: E402
from pbr_amd import scenes  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("workload", nargs="?", default="both", choices=("atrium", "textured", "both"))
ap.add_argument("--ref-spp", type=int, default=4096)
ap.add_argument("--max-spp", type=int, default=1024)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--size", type=int, nargs=2, default=(1920, 1080))
ap.add_argument("--one", type=float, default=None)
ap.add_argument("--sampled", action="store_true")
args = ap.parse_args()
W, H = args.size
SEED, REF_SEED, BOUNCES = 1, 99, 8
# (threshold, min_samples, step_samples): the library's 16 / 16 at four thresholds, and fewer, larger decision steps at the default threshold
ROWS = [(0.2, 16, 16), (0.1, 16, 16), (0.05, 16, 16), (0.02, 16, 16), (0.05, 32, 128)]


def rel_mse(x, ref):
    x, ref = x[..., :3].astype(np.float64), ref[..., :3].astype(np.float64)
    return float(np.mean((x - ref) ** 2 / (ref ** 2 + 0.01)))


def uniform_frame(pt, spp):
    t0 = time.perf_counter()
    pt.frame_begin(W, H, spp, seed=SEED, max_bounces=BOUNCES)
    pt.frame_add_samples(spp)
    pt.frame_resolve()
    pt.sync()
    wall = time.perf_counter() - t0
    return pt.stats()["seconds_render"], wall


def adaptive_frame(pt, thr, mn, step):
    t0 = time.perf_counter()
    L, h = pt._L, pt._h
    pt._ck(L.ptc_render_adaptive(h, W, H, args.max_spp, SEED, BOUNCES, pbr_amd.ptc.C.byref(pbr_amd.ptc.PtcAdaptiveParams.defaults(threshold=thr, min_samples=mn, step_samples=step))))
    wall = time.perf_counter() - t0
    pt._w, pt._h_px = W, H
    st, ad = pt.stats(), pt.adaptive_stats()
    return st["seconds_render"] + ad["seconds_adapt"], wall, st, ad


def run_sampled(pt, name):
    """The adaptive render with the covariance on against off (alternating, same process), then ptc_denoise against ptc_denoise_sampled on the last frame."""
    thr = 0.05 if args.one is None else args.one
    if args.one is not None:
        pt.set_sample_covariance(1)
        adaptive_frame(pt, thr, 16, 16)
        ev, wall, st, ad = adaptive_frame(pt, thr, 16, 16)
        pt.frame_guides()
        pt.denoise_sampled()
        pt.sync()
        print(f"one adaptive frame with the covariance, threshold {thr}: event {ev:.4f} s, wall {wall:.4f} s, mean count {ad['samples_total'] / ad['owned_pixels']:.2f}; "
              f"ptc_denoise_sampled {pt.denoise_seconds()[1] * 1e3:.3f} ms", flush=True)
        return
    for on in (0, 1):                                                # warm-up: queues and both sets of buffers allocated, code loaded
        pt.set_sample_covariance(on)
        adaptive_frame(pt, thr, 16, 16)
    rows = {0: [], 1: []}
    for rep in range(args.reps):
        for on in (0, 1):
            pt.set_sample_covariance(on)
            ev, wall, st, ad = adaptive_frame(pt, thr, 16, 16)
            rows[on].append((ev, wall, ad["samples_total"] / ad["owned_pixels"], st["paths"]))
    for on in (0, 1):
        v = rows[on]
        print(f"adaptive threshold {thr}, covariance {'on' if on else 'off'}: event s {[round(x[0], 4) for x in v]}, wall s {[round(x[1], 4) for x in v]}, mean count {v[-1][2]:.2f}, paths {v[-1][3]}", flush=True)
    e0, e1 = np.median([x[0] for x in rows[0]]), np.median([x[0] for x in rows[1]])
    w0, w1 = np.median([x[1] for x in rows[0]]), np.median([x[1] for x in rows[1]])
    print(f"covariance on / off: event {e1 / e0:.4f}, wall {w1 / w0:.4f} (medians of {args.reps})", flush=True)
    pt.frame_guides()                                                # the last frame keeps the covariance
    plain, sampled = [], []
    for rep in range(max(args.reps, 3) + 1):
        pt.denoise()
        plain.append(pt.denoise_seconds()[1])
        pt.denoise_sampled()
        sampled.append(pt.denoise_seconds()[1])
    print(f"ptc_denoise ms {[round(t * 1e3, 3) for t in plain[1:]]}, ptc_denoise_sampled ms {[round(t * 1e3, 3) for t in sampled[1:]]} (4 iterations, the first pair dropped); "
          f"sampled / plain {np.median(sampled[1:]) / np.median(plain[1:]):.3f}", flush=True)
    pt.set_sample_covariance(0)


def spp_for(curve, target):
    """the uniform spp whose relMSE is `target`: log-log interpolation between the measured levels (extrapolated with the last slope beyond them)"""
    lv = sorted(curve)
    x, y = np.log([float(v) for v in lv]), np.log([curve[v] for v in lv])
    t = np.log(target)
    for i in range(len(lv) - 1):
        if y[i] >= t >= y[i + 1]:
            return float(np.exp(x[i] + (t - y[i]) * (x[i + 1] - x[i]) / (y[i + 1] - y[i])))
    i = 0 if t > y[0] else len(lv) - 2
    return float(np.exp(x[i] + (t - y[i]) * (x[i + 1] - x[i]) / (y[i + 1] - y[i])))


def run(name):
    desc = scenes.atrium() if name == "atrium" else scenes.textured_atrium()
    pt = pbr_amd.PathTracer(0).load_scene(desc)
    print(f"== {name} {W}x{H}, max_spp {args.max_spp}, max_bounces {BOUNCES}; {pbr_amd.load_library().ptc_build_info().decode()}", flush=True)
    if args.sampled:
        run_sampled(pt, name)
        pt.close()
        return
    if args.one is not None:
        adaptive_frame(pt, args.one, 16, 16)
        ev, wall, st, ad = adaptive_frame(pt, args.one, 16, 16)
        print(f"one adaptive frame, threshold {args.one}: event {ev:.4f} s (of it decision steps {ad['seconds_adapt'] * 1e3:.3f} ms in {ad['passes']} passes), wall {wall:.4f} s, "
              f"mean count {ad['samples_total'] / ad['owned_pixels']:.2f}, paths {st['paths']}", flush=True)
        return
    ref = pt.render(W, H, args.ref_spp, seed=REF_SEED, max_bounces=BOUNCES)
    print(f"reference: uniform {args.ref_spp} spp, seed {REF_SEED}", flush=True)
    # the uniform frame's error by spp, from one progressive frame
    levels = [n for n in (16, 32, 64, 128, 256, 512, 1024, 2048) if n < args.max_spp] + [args.max_spp]
    curve, done = {}, 0
    pt.frame_begin(W, H, args.max_spp, seed=SEED, max_bounces=BOUNCES)
    for n in levels:
        pt.frame_add_samples(n - done); done = n
        pt.frame_resolve()
        curve[n] = rel_mse(pt.read_radiance(), ref)
    print("uniform relMSE by spp: " + ", ".join(f"{n}: {curve[n]:.3e}" for n in levels), flush=True)
    uniform_frame(pt, args.max_spp)                                  # warm-up: queues allocated, code loaded
    for thr, mn, step in ROWS[:1]:
        adaptive_frame(pt, thr, mn, step)
    uni, rows = [], {r: [] for r in ROWS}
    for rep in range(args.reps):
        uni.append(uniform_frame(pt, args.max_spp))
        for r in ROWS:
            ev, wall, st, ad = adaptive_frame(pt, *r)
            rows[r].append((ev, wall, ad["samples_total"] / ad["owned_pixels"], ad["passes"], ad["seconds_adapt"], rel_mse(pt.read_radiance(), ref), st["paths"]))
    u_ev, u_wall = np.median([u[0] for u in uni]), np.median([u[1] for u in uni])
    print(f"uniform {args.max_spp} spp: event s {[round(u[0], 4) for u in uni]}, wall s {[round(u[1], 4) for u in uni]}, relMSE {curve[args.max_spp]:.3e}", flush=True)
    for r in ROWS:
        v = rows[r]
        ev, wall = np.median([x[0] for x in v]), np.median([x[1] for x in v])
        mean_n, passes, t_ad, err = v[-1][2], v[-1][3], np.median([x[4] for x in v]), v[-1][5]
        n_eq = spp_for(curve, err)
        print(f"adaptive threshold {r[0]} min {r[1]} step {r[2]}: event s {[round(x[0], 4) for x in v]}, wall s {[round(x[1], 4) for x in v]}, mean count {mean_n:.1f}, {passes} decision steps "
              f"({t_ad * 1e3:.2f} ms of kernels), relMSE {err:.3e} = uniform at {n_eq:.0f} spp; time {wall / u_wall:.3f} of the uniform frame's, "
              f"speed-up at equal relMSE {(u_wall * n_eq / args.max_spp) / wall:.2f}x (wall; uniform time taken as proportional to spp), event {(u_ev * n_eq / args.max_spp) / ev:.2f}x", flush=True)
    pt.close()


for wl in (("atrium", "textured") if args.workload == "both" else (args.workload,)):
    run(wl)
