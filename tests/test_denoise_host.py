"""The denoiser's interface without a GPU: the symbols are exported and bound, a description-only context refuses every call that needs the
device with PTC_E_DEVICE, the defaults are the documented ones, a NULL context is PTC_E_ARG."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("ptc_frame_guides", "ptc_read_guide_rgba32f", "ptc_read_guide_hit", "ptc_denoise_default_params", "ptc_denoise", "ptc_select_output", "ptc_get_denoise_seconds")
E_ARG, E_DEVICE = -1, -3


def test_symbols_are_declared_exported_and_bound(pbr):
    header = open(os.path.join(ROOT, "include", "ptc.h")).read()
    L = pbr.load_library()
    for sym in NEW:
        assert re.search(r"\b%s\s*\(" % sym, header), sym
        assert sym in pbr.ptc.ABI_SYMBOLS and hasattr(L, sym), sym
    for enum in ("PTC_GUIDE_ALBEDO = 0", "PTC_GUIDE_NORMAL_DEPTH = 1", "PTC_OUTPUT_RADIANCE = 0", "PTC_OUTPUT_DENOISED = 1"):
        assert enum in header
    assert (pbr.ptc.GUIDE_ALBEDO, pbr.ptc.GUIDE_NORMAL_DEPTH, pbr.ptc.OUTPUT_RADIANCE, pbr.ptc.OUTPUT_DENOISED) == (0, 1, 0, 1)
    assert "#define PTC_ABI_VERSION 4" in header and L.ptc_abi_version() == 4            # additive: the ABI version stays
    for m in ("frame_guides", "read_guide", "read_guide_hit", "denoise", "select_output", "denoise_seconds", "denoise_default_params"):
        assert callable(getattr(pbr.PathTracer, m)), m


def test_default_parameters(pbr):
    assert pbr.PathTracer.denoise_default_params() == dict(iterations=4, sigma_l=4.0, sigma_n=128.0, sigma_p=1.0, demodulate=1)
    assert C.sizeof(pbr.ptc.PtcDenoiseParams) == 20
    pbr.load_library().ptc_denoise_default_params(None)                                   # a NULL pointer is ignored


def test_description_only_context_refuses_with_e_device(pbr):
    L = pbr.load_library()
    pt = pbr.PathTracer(pbr.ptc.DEVICE_NONE).load_scene(pbr.scenes.cornell_box())
    h = pt._h
    img = np.zeros((4, 4, 4), np.float32)
    prim = np.zeros((4, 4), np.int32)
    fp = img.ctypes.data_as(C.POINTER(C.c_float))
    p = pbr.ptc.PtcDenoiseParams()
    L.ptc_denoise_default_params(C.byref(p))
    g, d = C.c_double(), C.c_double()
    calls = {
        "ptc_frame_guides": lambda c: L.ptc_frame_guides(c),
        "ptc_read_guide_rgba32f": lambda c: L.ptc_read_guide_rgba32f(c, 0, fp),
        "ptc_read_guide_hit": lambda c: L.ptc_read_guide_hit(c, prim.ctypes.data_as(C.POINTER(C.c_int32)), fp),
        "ptc_denoise": lambda c: L.ptc_denoise(c, C.byref(p)),
        "ptc_denoise (NULL parameters)": lambda c: L.ptc_denoise(c, None),
        "ptc_select_output": lambda c: L.ptc_select_output(c, 1),
        "ptc_get_denoise_seconds": lambda c: L.ptc_get_denoise_seconds(c, C.byref(g), C.byref(d)),
    }
    for name, call in calls.items():
        assert call(h) == E_DEVICE, name
        assert b"PTC_DEVICE_NONE" in L.ptc_last_error(h), name
        assert call(None) == E_ARG, name
    with pytest.raises(pbr.PtcError, match="ptc error -3"):
        pt.frame_guides()
    with pytest.raises(pbr.PtcError, match="ptc error -3"):
        pt.denoise(iterations=2)
    with pytest.raises(TypeError):
        pt.denoise(sigma_x=1.0)
