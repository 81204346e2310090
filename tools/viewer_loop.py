#!/usr/bin/env python3
"""The reference viewer's frame loop over the C-ABI (src/gltf_viewer/App.cpp:306-313 turns the nodes, :384-393 renders): per frame a third of the
instances get a new rotation (ptc_update_instance), the scene is refitted (ptc_scene_refit, on the device), the frame is path-traced at `spp` samples
per pixel and resolved into the RGBA16F image the viewer's tonemapper reads (ptc_radiance_rgba16f_device_ptr: no copy to the host).  Wall time per
frame over `frames` frames, and where it goes.  VIEWER_REBUILD_RATIO=r in the environment adds the policy of examples/viewer_shim.cpp: after the refit, a rebuild on the
device (ptc_scene_rebuild) when ptc_stats.bvh_sa_cost has grown past r times bvh_sa_cost_built; the frame times before and after the first rebuild are reported apart.
With PTC_DEVICE_BVH=sah in the environment the rebuilt tree is the binned-SAH tree (ptc_set_device_builder), else the LBVH.
--denoise runs the loop a second time in the same process with the first-hit guides (ptc_frame_guides) and the à-trous filter (ptc_denoise, default
parameters) between the resolve and the RGBA16F hand-off, and reports that frame time beside the plain one, with the HIP-event times of the two passes.
--temporal runs it once more with the temporal path: guides, ptc_temporal_accumulate (the history reprojected through the refit and blended with the frame),
ptc_denoise_accumulated, hand-off; reported like --denoise's, against --denoise's frame time when both are given, with the accumulate's HIP-event time.
--auto-exposure runs the plain loop once more with the display transform: one metering per displayed frame (ptc_meter_exposure, adapt_rate 0.1) and the exposed RGBA16F
(ptc_display_rgba16f_device_ptr) instead of the raw one, queued behind the resolve without a wait in between.  The scene keeps turning and the refitted tree keeps getting
slower, so this loop alternates plain and metered frames and reports the two medians of the same stretch, with the HIP-event times of the metering and of the display
kernel and the exposure the loop ended at.
usage: python3 tools/viewer_loop.py [atrium|textured] [spp] [frames] [w h] [--denoise] [--temporal] [--auto-exposure]"""
import json, math, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "physically-based-renderer_amd"))
import numpy as np
import pbr_amd as pbr

denoise = "--denoise" in sys.argv
temporal = "--temporal" in sys.argv
auto_exposure = "--auto-exposure" in sys.argv
argv = [a for a in sys.argv if a not in ("--denoise", "--temporal", "--auto-exposure")]
name = argv[1] if len(argv) > 1 else "atrium"
spp = int(argv[2]) if len(argv) > 2 else 1
frames = int(argv[3]) if len(argv) > 3 else 60
w, h = (int(argv[4]), int(argv[5])) if len(argv) > 5 else (1920, 1080)
d = pbr.scenes.by_name("textured_atrium" if name == "textured" else "atrium")
pt = pbr.PathTracer(0).load_scene(d)
moving = [i for i, it in enumerate(d.instances) if i % 3 == 0 and getattr(it, "matrix", None) is None]
t_refit, t_frame = [], []
ratio = float(os.environ.get("VIEWER_REBUILD_RATIO", "0"))
rebuilds = 0
first_rebuild = None                                  # index into t_frame of the first frame after the first rebuild
for k in range(frames + 5):
    t0 = time.perf_counter()
    a = 0.01 * (k + 1)
    for i in moving:
        pt.update_instance(i, d.instances[i].t, (math.cos(a / 2), 0.0, math.sin(a / 2), 0.0), d.instances[i].s)
    pt.scene_refit()
    if ratio > 0.0:
        st_ = pt.stats()
        if st_["bvh_sa_cost"] > ratio * st_["bvh_sa_cost_built"]:
            pt.scene_rebuild(); rebuilds += 1
            if first_rebuild is None: first_rebuild = max(k - 5, 0)
    t1 = time.perf_counter()
    pt.frame_begin(w, h, spp, seed=k, max_bounces=8)
    pt.frame_add_samples(spp)
    pt.frame_resolve()
    pt.sync()
    ptr = pt.radiance_f16_device_ptr()
    t2 = time.perf_counter()
    if k >= 5:                                        # the first frames size the queues and build the refit plan
        t_refit.append(t1 - t0); t_frame.append(t2 - t0)
st = pt.stats()
out = {"scene": d.name, "triangles": st["n_triangles"], "moving_instances": len(moving), "w": w, "h": h, "spp": spp, "frames": frames,
       "ms_per_frame": {"median": 1e3 * float(np.median(t_frame)), "min": 1e3 * float(np.min(t_frame)), "max": 1e3 * float(np.max(t_frame))},
       "fps": 1.0 / float(np.median(t_frame)),
       "ms_update_and_refit": 1e3 * float(np.median(t_refit)), "ms_refit_device_side": 1e3 * st["seconds_refit"],
       "Mpaths_per_s": w * h * spp / float(np.median(t_frame)) / 1e6, "half_image_device_ptr": hex(ptr),
       "rebuild_ratio": ratio, "rebuilds": rebuilds, "sa_cost_ratio_at_end": st["bvh_sa_cost"] / st["bvh_sa_cost_built"],
       "device_builder": "sah" if os.environ.get("PTC_DEVICE_BVH") == "sah" else "lbvh"}
if first_rebuild is not None and 0 < first_rebuild < len(t_frame) - 1:     # the rebuild frame itself counts in neither
    out["ms_per_frame_before_first_rebuild"] = 1e3 * float(np.median(t_frame[:first_rebuild]))
    out["ms_per_frame_after_first_rebuild"] = 1e3 * float(np.median(t_frame[first_rebuild + 1:]))
if denoise:      # the same loop again, the frame filtered before the hand-off: the scene keeps turning, every frame's guides are traced anew
    t_dn, s_guides, s_filter = [], [], []
    for k in range(frames + 5, 2 * frames + 10):
        t0 = time.perf_counter()
        a = 0.01 * (k + 1)
        for i in moving:
            pt.update_instance(i, d.instances[i].t, (math.cos(a / 2), 0.0, math.sin(a / 2), 0.0), d.instances[i].s)
        pt.scene_refit()
        pt.frame_begin(w, h, spp, seed=k, max_bounces=8)
        pt.frame_add_samples(spp)
        pt.frame_guides()
        pt.frame_resolve()
        pt.denoise()
        pt.select_output(pbr.ptc.OUTPUT_DENOISED)
        pt.sync()
        ptr = pt.radiance_f16_device_ptr()
        t2 = time.perf_counter()
        if k >= frames + 10:
            t_dn.append(t2 - t0)
            g_s, f_s = pt.denoise_seconds()
            s_guides.append(g_s); s_filter.append(f_s)
    out["denoise"] = {"params": pbr.PathTracer.denoise_default_params(), "ms_per_frame": {"median": 1e3 * float(np.median(t_dn)), "min": 1e3 * float(np.min(t_dn)), "max": 1e3 * float(np.max(t_dn))},
                      "ms_added_per_frame": 1e3 * float(np.median(t_dn) - np.median(t_frame)), "ms_guide_pass_device": 1e3 * float(np.median(s_guides)),
                      "ms_filter_device": 1e3 * float(np.median(s_filter))}
if temporal:     # once more: the frame blended into the reprojected history, then filtered; the history survives every refit
    t_tp, s_guides, s_acc, s_filter = [], [], [], []
    for k in range(2 * frames + 10, 3 * frames + 15):
        t0 = time.perf_counter()
        a = 0.01 * (k + 1)
        for i in moving:
            pt.update_instance(i, d.instances[i].t, (math.cos(a / 2), 0.0, math.sin(a / 2), 0.0), d.instances[i].s)
        pt.scene_refit()
        pt.frame_begin(w, h, spp, seed=k, max_bounces=8)
        pt.frame_add_samples(spp)
        pt.frame_guides()
        pt.frame_resolve()
        pt.temporal_accumulate()
        pt.denoise_accumulated()
        pt.select_output(pbr.ptc.OUTPUT_DENOISED)
        pt.sync()
        ptr = pt.radiance_f16_device_ptr()
        t2 = time.perf_counter()
        if k >= 2 * frames + 15:
            t_tp.append(t2 - t0)
            g_s, f_s = pt.denoise_seconds()
            s_guides.append(g_s); s_filter.append(f_s); s_acc.append(pt.temporal_seconds())
    n_hist = pt.read_temporal(pbr.ptc.TEMPORAL_HISTORY)[..., 3]
    out["temporal"] = {"params": pbr.PathTracer.temporal_default_params(), "ms_per_frame": {"median": 1e3 * float(np.median(t_tp)), "min": 1e3 * float(np.min(t_tp)), "max": 1e3 * float(np.max(t_tp))},
                       "ms_added_per_frame": 1e3 * float(np.median(t_tp) - np.median(t_frame)), "ms_guide_pass_device": 1e3 * float(np.median(s_guides)),
                       "ms_accumulate_device": 1e3 * float(np.median(s_acc)), "ms_filter_device": 1e3 * float(np.median(s_filter)),
                       "mean_history_length": float(n_hist[n_hist > 0].mean())}
    if denoise:
        out["temporal"]["ms_added_to_denoise_frame"] = 1e3 * float(np.median(t_tp) - np.median(t_dn))
if auto_exposure:      # plain and metered frames alternating: nothing waits between the resolve, the metering and the conversion of a metered frame
    pt.set_display(auto_exposure=1, adapt_rate=0.1)
    t_ae, t_pl, s_meter, s_disp = [], [], [], []
    for k in range(3 * frames + 15, 5 * frames + 25):
        metered = k % 2 == 1
        t0 = time.perf_counter()
        a = 0.01 * (k + 1)
        for i in moving:
            pt.update_instance(i, d.instances[i].t, (math.cos(a / 2), 0.0, math.sin(a / 2), 0.0), d.instances[i].s)
        pt.scene_refit()
        pt.frame_begin(w, h, spp, seed=k, max_bounces=8)
        pt.frame_add_samples(spp)
        pt.frame_resolve()
        if metered:
            pt.meter_exposure()
            ptr = pt.display_f16_device_ptr()
        else:
            pt.sync()
            pt.radiance_f16_device_ptr()
        t2 = time.perf_counter()
        if k >= 3 * frames + 25:
            (t_ae if metered else t_pl).append(t2 - t0)
            if metered:
                m_s, d_s = pt.display_seconds()
                s_meter.append(m_s); s_disp.append(d_s)
    out["auto_exposure"] = {"params": pt.get_display(), "ms_per_frame": {"median": 1e3 * float(np.median(t_ae)), "min": 1e3 * float(np.min(t_ae)), "max": 1e3 * float(np.max(t_ae))},
                            "ms_per_plain_frame_of_the_same_stretch": {"median": 1e3 * float(np.median(t_pl)), "min": 1e3 * float(np.min(t_pl)), "max": 1e3 * float(np.max(t_pl))},
                            "ms_added_per_frame": 1e3 * float(np.median(t_ae) - np.median(t_pl)), "ms_meter_device": 1e3 * float(np.median(s_meter)),
                            "ms_display_half_device": 1e3 * float(np.median(s_disp)), "exposure": pt.exposure(), "exposed_half_image_device_ptr": hex(ptr)}
print(json.dumps(out))
