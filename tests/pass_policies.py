"""What tests/test_gpu_pass_policies.py and tests/test_pass_policies_host.py share: contexts under a launch policy, the segment layout restated, the policy table
and the comparison of two frames.

A launch policy is a set of PTC_* variables a context reads when it is created (csrc/ptc_api.cpp: ptc_create; csrc/ptc_api_scene.cpp for PTC_STACK_LDS and
PTC_TRACE_BLOCKS_PER_CU, read at the commit).  None of them may change what a frame computes: the image's bits, the nine counters of ptc_stats that count rays and
traversal steps, and the per-record counters of the optional passes."""
import contextlib
import math
import os
import re

import numpy as np

F32 = np.float32
COUNTERS = ("paths", "segments", "shadow_rays", "hits", "node_visits_closest", "tri_tests_closest", "node_visits_any", "tri_tests_any", "algorithmic_bytes")
SEG_MIN_LEN = 512      # PTC_SEG_MIN_LEN (csrc/ptc_internal.h)
BOUNCES = 4
SEED = 0x5EED0FA11

# ---- the two frame shapes ------------------------------------------------------------------------------------------------------------------------------------
RAGGED = (37, 23, 5)              # 851 pixels (no multiple of 64) x 5 spp = 4,255 paths: 9 segments of 512 slots, a walk grid of 3 blocks whose last has one live wave
CAPPED_W, CAPPED_SPP = 163, 8     # x a height that follows shade_segments (capped_height): 163 x 121 x 8 = 157,784 paths at 256 segments
CAPPED_ENV = {"PTC_SEGMENTS_PER_CU": "1"}


def seg_layout(n, max_seg):
    """ptc_seg_layout (csrc/ptc_internal.h): (n_seg, seg_len) of a batch of n slots over at most max_seg segments, in uint32 arithmetic."""
    M = 0xFFFFFFFF      # the header's sums wrap at 32 bits (a batch never comes near: batch_samples keeps it under 2^32 - 64 max_seg - 80 slots, and max_seg >= the CU count)
    n, max_seg = int(n), int(max_seg)
    s = ((n + SEG_MIN_LEN - 1) & M) // SEG_MIN_LEN
    s = max(min(s, max_seg), 1)
    per = ((n + s - 1) & M) // s
    return s, ((((per + 63) & M) & ~63) if per else 64)


def seg_slots(cap, max_seg):
    """ptc_seg_slots: the slots a lane's queue arrays hold for `cap` paths."""
    return int(cap) + 64 * int(max_seg) + 64


def capped_paths(shade_segments):
    """A batch size at which the layout is capped and its segments are no whole trace chunks: about 616 slots in use per segment, 640 after the rounding to 64."""
    return int(shade_segments) * 616 + 88


def capped_height(shade_segments):
    """The height of the capped frame: 121 at 256 segments."""
    return max(1, round(capped_paths(shade_segments) / (CAPPED_W * CAPPED_SPP)))


def is_capped(n_paths, shade_segments):
    n_seg, seg_len = seg_layout(n_paths, shade_segments)
    return n_seg == shade_segments and seg_len % SEG_MIN_LEN != 0


# ---- contexts ------------------------------------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def environment(**env):
    """The PTC_* variables of `env` set, and the environment as it was afterwards."""
    assert all(k.startswith("PTC_") for k in env), env
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)


@contextlib.contextmanager
def tracer(pbr, desc, setup=None, device=0, **env):
    """A PathTracer created and committed under the variables `env` (the pattern of test_gpu_path_order._context), `setup(pt)` applied, closed on exit."""
    with environment(**env):
        pt = pbr.PathTracer(device).load_scene(desc)
    try:
        if setup is not None:
            setup(pt)
        yield pt
    finally:
        pt.close()


def policy_field(pt, name):
    """The value of `name=` in ptc_launch_policy, as a string (the LAST occurrence: the committed context's figures follow the defaults)."""
    m = re.findall(r"(?:^|[ |])" + re.escape(name) + r"=(\S+)", pt.launch_policy())
    assert m, (name, pt.launch_policy())
    return m[-1]


def layout_of(pt, n_owned, spp):
    """(batches, n_seg, seg_len) of the frame of n_owned pixels x spp samples that `pt` has begun (or just rendered): per_batch is that frame's, the layout that of
    its first — full — batch."""
    shade_segments = int(policy_field(pt, "shade_segments"))
    per_batch = pt.internals()["per_batch"]
    assert per_batch >= 1
    k = min(per_batch, spp)
    n_seg, seg_len = seg_layout(n_owned * k, shade_segments)
    return math.ceil(spp / per_batch), n_seg, seg_len


# ---- the policies ----------------------------------------------------------------------------------------------------------------------------------------------
# (name, environment, frame, what must also hold: a function of (pt, layout) that asserts).  "frame": "ragged" or "capped".
def _has(**fields):
    def check(pt, layout):
        for k, v in fields.items():
            assert policy_field(pt, k).split("(")[0] == str(v), (k, v, pt.launch_policy())
    return check


def _capped(pt, layout):
    batches, n_seg, seg_len = layout
    assert batches == 1 and n_seg == int(policy_field(pt, "shade_segments")) and seg_len % SEG_MIN_LEN != 0, layout


def _both(*checks):
    def check(pt, layout):
        for c in checks:
            c(pt, layout)
    return check


def _batches(n=None, at_least=None, n_seg=None):
    def check(pt, layout):
        assert (n is None or layout[0] == n) and (at_least is None or layout[0] >= at_least) and (n_seg is None or layout[1] == n_seg), layout
    return check


def _lanes_ran(lanes):
    def check(pt, layout):      # batch i runs on lane i % lanes (csrc/ptc_api.cpp: issue), and every batch traces BOUNCES + 1 times
        assert layout[0] >= lanes and pt.stats()["launches_trace_closest"] == layout[0] * (BOUNCES + 1), (layout, pt.stats()["launches_trace_closest"])
    return check


ENV_POLICIES = [
    ("capped", dict(CAPPED_ENV), "capped", _capped),
    ("capped+sort", dict(CAPPED_ENV, PTC_SHADE_SORT="1"), "capped", _both(_capped, _has(shade_sort=1))),
    ("sort", dict(PTC_SHADE_SORT="1"), "ragged", _has(shade_sort=1)),
    ("sample-order", dict(PTC_PATH_ORDER="sample"), "ragged", _has(path_order="sample")),
    # 2048 paths hold two samples of 851 pixels (per_batch = 2048 / 851 = 2): batches of 2, 2 and 1 samples.  The five one-sample batches the table asks for need a
    # budget under 2 x 851; 1024 is the smallest the library accepts
    ("batch-2048", dict(PTC_BATCH_PATHS="2048"), "ragged", _batches(3, n_seg=4)),
    ("batch-1024", dict(PTC_BATCH_PATHS="1024"), "ragged", _batches(5, n_seg=2)),
    ("lanes2", dict(PTC_LANES="2", PTC_BATCH_PATHS="2048"), "ragged", _both(_has(lanes=2), _batches(at_least=5), _lanes_ran(2))),
    ("lanes3", dict(PTC_LANES="3", PTC_BATCH_PATHS="6000"), "ragged", _both(_has(lanes=3), _batches(3), _lanes_ran(3))),
    ("small-grid", dict(PTC_TRACE_BLOCKS_PER_CU="1", PTC_STACK_LDS="2"), "ragged", _has(trace_blocks_per_cu=1, stack_lds=2)),
]


# ---- comparison ------------------------------------------------------------------------------------------------------------------------------------------------
def bits_equal(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def frame_record(pt, image):
    """What a finished frame is compared by.  Every integer field of the passes' statistics counts RECORDS — rays passed on, records walked, surfaces passed, events,
    segments that crossed, additions (include/ptc_alpha.h, ptc_glass.h, ptc_glass_shadows.h, ptc_medium.h, ptc_emissive_tex.h) — so each is compared as it is; none
    counts launches or rounds.  What does scale with the number of batches is ptc_stats' launches_trace_closest / launches_trace_any, which are not among the nine
    counters and are left out here (pass_policies._lanes_ran holds the former to batches x (bounces + 1)).  Seconds are never compared."""
    st = pt.stats()
    rec = {"image": np.array(image, F32), "counters": {k: st[k] for k in COUNTERS}}
    for name in ("alpha_stats", "glass_stats", "glass_shadow_stats", "medium_stats", "emissive_tex_stats"):
        rec[name] = {k: v for k, v in getattr(pt, name)().items() if not k.startswith("seconds")}
    return rec


def activity(rec):
    """The activity counters of a record, flat: what a reader needs to see that a feature ran."""
    out = {"shadow_rays": rec["counters"]["shadow_rays"]}
    for name in ("alpha_stats", "glass_stats", "glass_shadow_stats", "medium_stats", "emissive_tex_stats"):
        out.update({name[:-6] + "." + k: v for k, v in rec[name].items() if v})
    return out


def assert_same_frame(got, want, what):
    assert got["image"].shape == want["image"].shape, what
    differ = (got["image"].view(np.uint32) != want["image"].view(np.uint32)).any(-1)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} pixels differ from the default policy's, first at {np.argwhere(differ)[0].tolist()}"
    for name in got:
        if name != "image":
            assert got[name] == want[name], f"{what}: {name} {got[name]} != {want[name]}"
