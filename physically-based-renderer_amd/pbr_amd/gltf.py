"""glTF 2.0 / GLB: ctypes binding of the C++ loader (include/ptc_gltf.h, libptc_gltf.so) and a small writer.

`load_into(pt, path)` is the path-tracer counterpart of the reference's `gltf::Loader::loadAsset` +
`Asset::loadScene` (src/pbr_engine/gltf/pbr/gltf/Loader.cpp:10-32, Asset.cpp:259-273): it fills a PathTracer's scene
from a file; the camera stays the caller's unless it asks for one of the asset's (Asset.cameras, Asset.apply_camera, cameras()).

`write_glb(desc, path)` serialises a SceneDesc — used by the tests to produce assets, since the reference's own
(assets/models/test_scene.glb) is stripped from the checkout (.MISSING_LARGE_BLOBS).
"""
from __future__ import annotations

import ctypes as C
import json
import os
import struct
import zlib

import numpy as np

from . import ptc as _ptc

_LIB = os.path.join(os.path.dirname(_ptc.LIB_PATH), "libptc_gltf.so")
_lib = None


def _load():
    global _lib
    if _lib is None:
        _ptc.load_library()
        if not os.path.exists(_LIB):
            raise _ptc.PtcError(f"{_LIB} is missing: run __graft_entry__.build()")
        L = C.CDLL(_LIB)
        L.ptc_gltf_load.restype = C.c_longlong
        L.ptc_gltf_load.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_float), C.c_char_p, C.c_int]
        L.ptc_gltf_emissive_textures.restype = C.c_int
        L.ptc_gltf_emissive_textures.argtypes = [C.c_int]
        L.ptc_gltf_open.restype = C.c_void_p
        L.ptc_gltf_open.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
        L.ptc_gltf_close.restype = None
        L.ptc_gltf_close.argtypes = [C.c_void_p]
        L.ptc_gltf_asset_load.restype = C.c_longlong
        L.ptc_gltf_asset_load.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_float)]
        L.ptc_gltf_asset_animations.argtypes = [C.c_void_p]
        L.ptc_gltf_asset_duration.restype = C.c_double
        L.ptc_gltf_asset_duration.argtypes = [C.c_void_p, C.c_int]
        L.ptc_gltf_asset_pose.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double]
        cp = C.POINTER(_ptc.PtcCameraParams)
        L.ptc_gltf_asset_cameras.argtypes = [C.c_void_p]
        L.ptc_gltf_asset_camera.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_float, cp]
        L.ptc_gltf_cameras.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_float, cp, C.c_int, C.c_char_p, C.c_int]
        L.ptc_gltf_asset_last_error.restype = C.c_char_p
        L.ptc_gltf_asset_last_error.argtypes = [C.c_void_p]
        _lib = L
    return _lib


class Asset:
    """A glTF file kept open (ptc_gltf_open): load it into a PathTracer with its skins and morph targets, then pose it along its animations.

        a = Asset(path); a.load_into(pt, camera); a.pose(pt, 0, 0.4); pt.scene_refit()"""

    def __init__(self, path: str):
        self._L = _load()
        err = C.create_string_buffer(512)
        self._a = self._L.ptc_gltf_open(os.fsencode(path), err, 512)
        if not self._a:
            raise _ptc.PtcError(err.value.decode() or "ptc_gltf_open failed")

    def close(self):
        if getattr(self, "_a", None):
            self._L.ptc_gltf_close(self._a)
            self._a = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc < 0:
            raise _ptc.PtcError(self._L.ptc_gltf_asset_last_error(self._a).decode() or f"glTF asset call failed ({rc})")
        return rc

    @property
    def n_animations(self) -> int:
        return int(self._L.ptc_gltf_asset_animations(self._a))

    def duration(self, animation: int) -> float:
        return float(self._L.ptc_gltf_asset_duration(self._a, int(animation)))

    def load_into(self, pt, camera=None, scene_index: int = -1, compose_parents: bool = True, animation=None, time: float = 0.0):
        """scene_begin -> the file's scene with targets and skins -> (the pose of `animation` at `time`) -> camera -> scene_commit.
        Returns (n_triangles, bbox_lo, bbox_hi) of the bind pose."""
        h = pt._h
        pt._ck(pt._L.ptc_scene_begin(h))
        bbox = (C.c_float * 6)()
        n = self._ck(self._L.ptc_gltf_asset_load(self._a, h, scene_index, 1 if compose_parents else 0, bbox))
        if animation is not None:
            self._ck(self._L.ptc_gltf_asset_pose(self._a, h, int(animation), float(time)))
        lo, hi = np.array(bbox[0:3], np.float32), np.array(bbox[3:6], np.float32)
        if camera is None:
            c = 0.5 * (lo + hi)
            r = 0.5 * float(np.linalg.norm(hi - lo))
            fov = np.radians(60.0)
            pt.set_camera((c[0], c[1], c[2] + r / np.tan(0.5 * fov) + r), c, float(fov), 1.0)
        else:
            pt.set_camera(camera.position, camera.target, camera.fov_y, camera.aspect)
        pt._ck(pt._L.ptc_scene_commit(h))
        return int(n), lo, hi

    @property
    def n_cameras(self) -> int:
        return int(self._ck(self._L.ptc_gltf_asset_cameras(self._a)))

    def camera(self, index: int = 0, frame_aspect: float = 1.0, animation=None, time: float = 0.0):
        """ptc_gltf_asset_camera: the PtcCameraParams of camera node `index` (scene-traversal order) at rest, or at `time` of `animation`.  aspect is the
        camera's aspectRatio when it has one, else frame_aspect."""
        p = _ptc.PtcCameraParams()
        self._ck(self._L.ptc_gltf_asset_camera(self._a, int(index), -1 if animation is None else int(animation), float(time), float(frame_aspect), C.byref(p)))
        return p

    @property
    def cameras(self):
        """The asset's camera nodes at rest, as dicts (ptc_camera_params; aspect 1 where the camera has no aspectRatio)."""
        return [self.camera(k).as_dict() for k in range(self.n_cameras)]

    def apply_camera(self, pt, index: int = 0, frame_aspect: float = 1.0, animation=None, time: float = 0.0):
        """The asset's camera `index` becomes pt's camera (ptc_set_camera_ex).  Needs no commit; call it again with a time to fly along an animation."""
        p = self.camera(index, frame_aspect, animation, time)
        pt._ck(pt._L.ptc_set_camera_ex(pt._h, C.byref(p)))
        return p.as_dict()

    def pose(self, pt, animation: int, time: float):
        """ptc_gltf_asset_pose: instance matrices and mesh poses of `animation` at `time` (clamped); the caller refits or rebuilds."""
        self._ck(self._L.ptc_gltf_asset_pose(self._a, pt._h, int(animation), float(time)))
        return self


def cameras(path: str, frame_aspect: float = 1.0, scene_index: int = -1, compose_parents: bool = True):
    """ptc_gltf_cameras: the rest-pose cameras of the stateless loader, a list of PtcCameraParams."""
    L = _load()
    err = C.create_string_buffer(512)
    n = L.ptc_gltf_cameras(os.fsencode(path), scene_index, 1 if compose_parents else 0, float(frame_aspect), None, 0, err, 512)
    if n < 0:
        raise _ptc.PtcError(err.value.decode() or f"ptc_gltf_cameras failed ({n})")
    out = (_ptc.PtcCameraParams * max(n, 1))()
    L.ptc_gltf_cameras(os.fsencode(path), scene_index, 1 if compose_parents else 0, float(frame_aspect), out, n, err, 512)
    return [out[k] for k in range(n)]


def emissive_textures(on=None) -> bool:
    """ptc_gltf_emissive_textures: whether the loaders give a material with an emissiveTexture its emission texture (the default) or read it as a uniform emitter of its
    factor.  on=None only asks.  Returns the previous setting."""
    return bool(_load().ptc_gltf_emissive_textures(-1 if on is None else int(bool(on))))


def load_into(pt, path: str, camera=None, scene_index: int = -1, compose_parents: bool = True, env=None, emissive_textures: bool = True):
    """scene_begin → materials/meshes/instances from the file → camera → scene_commit.
    Returns (n_triangles, bbox_lo, bbox_hi).  camera: CameraDesc, or None to frame the bounding box from +z.
    env: optional (h, w, 3) float32 lat-long environment map (glTF has no such thing; ptc_set_env_latlong_rgb32f).
    emissive_textures=False: a material with an emissiveTexture is read as a uniform emitter of its factor (ptc_render --no-emissive-textures).  The loader's switch is
    one per process and is set around this call: not to be used from two threads with different values at once."""
    L = _load()
    h = pt._h
    pt._ck(pt._L.ptc_scene_begin(h))
    bbox = (C.c_float * 6)()
    err = C.create_string_buffer(512)
    was = L.ptc_gltf_emissive_textures(1 if emissive_textures else 0)
    try:
        n = L.ptc_gltf_load(h, os.fsencode(path), scene_index, 1 if compose_parents else 0, bbox, err, 512)
    finally:
        L.ptc_gltf_emissive_textures(was)
    if n < 0:
        raise _ptc.PtcError(err.value.decode() or f"ptc_gltf_load failed ({n})")
    lo, hi = np.array(bbox[0:3], np.float32), np.array(bbox[3:6], np.float32)
    if camera is None:
        c = 0.5 * (lo + hi)
        r = 0.5 * float(np.linalg.norm(hi - lo))
        fov = np.radians(60.0)
        pt.set_camera((c[0], c[1], c[2] + r / np.tan(0.5 * fov) + r), c, float(fov), 1.0)
    else:
        pt.set_camera(camera.position, camera.target, camera.fov_y, camera.aspect)
    if env is not None:
        e = np.ascontiguousarray(env, np.float32)
        assert e.ndim == 3 and e.shape[2] == 3, "env is (h, w, 3) float32"
        pt._ck(pt._L.ptc_set_env_latlong_rgb32f(h, e.ctypes.data_as(C.POINTER(C.c_float)), e.shape[1], e.shape[0]))
    pt._ck(pt._L.ptc_scene_commit(h))
    return int(n), lo, hi


def _decode(fn_name: str, data: bytes) -> np.ndarray:
    L = _load()
    fn = getattr(L, fn_name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_ulonglong, C.c_void_p, C.c_ulonglong, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    w, h = C.c_int(0), C.c_int(0)
    err = C.create_string_buffer(256)
    if fn(data, len(data), None, 0, C.byref(w), C.byref(h), err, 256):
        raise _ptc.PtcError(err.value.decode())
    out = np.empty((h.value, w.value, 4), np.uint8)
    if fn(data, len(data), out.ctypes.data, out.nbytes, C.byref(w), C.byref(h), err, 256):
        raise _ptc.PtcError(err.value.decode())
    return out


def png_decode(data: bytes) -> np.ndarray:
    """PNG file image → (h, w, 4) uint8 through the loader's own decoder (ptc_png_decode_rgba8)."""
    return _decode("ptc_png_decode_rgba8", data)


def jpeg_decode(data: bytes) -> np.ndarray:
    """JPEG file image → (h, w, 4) uint8 through the loader's own decoder (ptc_jpeg_decode_rgba8)."""
    return _decode("ptc_jpeg_decode_rgba8", data)


def image_decode(data: bytes, kind: int = 0) -> np.ndarray:
    """BMP / TGA / binary PGM-PPM file image → (h, w, 4) uint8 through the loader's decoders (ptc_image_decode_rgba8; kind 0 = by content, 1 BMP, 2 TGA, 3 PNM)."""
    L = _load()
    fn = L.ptc_image_decode_rgba8
    fn.restype = C.c_int
    fn.argtypes = [C.c_int, C.c_char_p, C.c_ulonglong, C.c_void_p, C.c_ulonglong, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    w, h = C.c_int(0), C.c_int(0)
    err = C.create_string_buffer(256)
    if fn(kind, data, len(data), None, 0, C.byref(w), C.byref(h), err, 256):
        raise ValueError(err.value.decode())
    out = np.empty((h.value, w.value, 4), np.uint8)
    if fn(kind, data, len(data), out.ctypes.data, out.nbytes, C.byref(w), C.byref(h), err, 256):
        raise ValueError(err.value.decode())
    return out


def hdr_decode(data: bytes) -> np.ndarray:
    """Radiance RGBE file image → (h, w, 3) float32 through the library's decoder (ptc_hdr_decode_rgb32f)."""
    L = _load()
    L.ptc_hdr_decode_rgb32f.argtypes = [C.c_char_p, C.c_ulonglong, C.POINTER(C.c_float), C.c_ulonglong, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_char_p, C.c_int]
    w, h = C.c_int(0), C.c_int(0)
    err = C.create_string_buffer(256)
    if L.ptc_hdr_decode_rgb32f(data, len(data), None, 0, C.byref(w), C.byref(h), err, 256) < 0:
        raise ValueError(err.value.decode())
    out = np.zeros((h.value, w.value, 3), np.float32)
    if L.ptc_hdr_decode_rgb32f(data, len(data), out.ctypes.data_as(C.POINTER(C.c_float)), out.size, C.byref(w), C.byref(h), err, 256) < 0:
        raise ValueError(err.value.decode())
    return out


def hdr_encode(rgb: np.ndarray, rle: bool = True, magic: str = "#?RADIANCE") -> bytes:
    """Small Radiance RGBE writer for tests and assets: (h, w, 3) float → shared-exponent pixels (mantissas by truncation, as Ward's float2rgbe), "-Y h +X w",
    new-style run-length scanlines when `rle` and 8 <= w < 32768 (runs of >= 3 equal bytes, literal blocks otherwise), flat pixels else."""
    a = np.asarray(rgb, np.float64)
    h, w = a.shape[:2]
    v = a.max(2)
    m, e = np.frexp(np.where(v > 1e-32, v, 1.0))
    scale = np.where(v > 1e-32, m * 256.0 / np.where(v > 1e-32, v, 1.0), 0.0)
    px = np.zeros((h, w, 4), np.uint8)
    px[..., :3] = np.clip((a * scale[..., None]).astype(np.int64), 0, 255)
    px[..., 3] = np.where(v > 1e-32, e + 128, 0)
    out = bytearray(f"{magic}\nFORMAT=32-bit_rle_rgbe\nEXPOSURE=1.0\n\n-Y {h} +X {w}\n".encode())
    if not rle or w < 8 or w >= 32768:
        return bytes(out) + px.tobytes()
    for y in range(h):
        out += bytes((2, 2, w >> 8, w & 255))
        for k in range(4):
            row = px[y, :, k]
            i = 0
            while i < w:
                run = 1
                while i + run < w and run < 127 and row[i + run] == row[i]:
                    run += 1
                if run >= 3:
                    out += bytes((128 + run, int(row[i])))
                    i += run
                    continue
                j = i                                                  # a literal block: up to the next run of >= 3, at most 128 bytes
                while j < w and j - i < 128:
                    if j + 2 < w and row[j] == row[j + 1] == row[j + 2]:
                        break
                    j += 1
                if j == i:
                    j = i + 1
                out += bytes((j - i,)) + row[i:j].tobytes()
                i = j
    return bytes(out)


# ----------------------------------------------------------------------------------------------------
_ADAM7 = ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2))


def png_encode(samples: np.ndarray, color_type: int = 6, depth: int = 8, interlace: bool = False, filters="cycle",
               level: int = 9, strategy: int = 0, palette=None, trns: bytes = None, idat_split: int = 0) -> bytes:
    """Small PNG writer for assets and decoder tests.  samples: (h, w, channels) unsigned integers already in the
    file's sample range (channels = 1, 3, 1, 2, 4 for colour types 0, 2, 3, 4, 6).  filters: "cycle" (row y uses
    filter y % 5), or a fixed filter type 0..4.  strategy: zlib strategy (zlib.Z_FIXED forces fixed Huffman blocks)."""
    s = np.asarray(samples)
    h, w, ch = s.shape
    assert ch == {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}[color_type]
    bpp = max(1, ch * depth // 8)

    def pack_rows(img):
        hh, ww, _ = img.shape
        flat = img.reshape(hh, ww * ch)
        if depth == 16:
            return flat.astype(">u2").view(np.uint8).reshape(hh, -1)
        if depth == 8:
            return flat.astype(np.uint8)
        bits = np.zeros((hh, (ww * ch * depth + 7) // 8 * 8), np.uint8)
        for b in range(depth):
            bits[:, b : ww * ch * depth : depth] = (flat >> (depth - 1 - b)) & 1
        return np.packbits(bits, axis=1)

    def paeth(a, b, c):
        p = a + b - c
        pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
        return a if pa <= pb and pa <= pc else (b if pb <= pc else c)

    def filtered(rows):
        out = bytearray()
        prev = np.zeros(rows.shape[1], np.int32)
        for y in range(rows.shape[0]):
            cur = rows[y].astype(np.int32)
            ft = y % 5 if filters == "cycle" else int(filters)
            left = np.concatenate([np.zeros(bpp, np.int32), cur[:-bpp]]) if cur.size > bpp else np.zeros(cur.size, np.int32)
            ul = np.concatenate([np.zeros(bpp, np.int32), prev[:-bpp]]) if cur.size > bpp else np.zeros(cur.size, np.int32)
            if ft == 0:
                f = cur
            elif ft == 1:
                f = cur - left
            elif ft == 2:
                f = cur - prev
            elif ft == 3:
                f = cur - ((left + prev) >> 1)
            else:
                f = cur - np.array([paeth(int(a), int(b), int(c)) for a, b, c in zip(left, prev, ul)], np.int32)
            out.append(ft)
            out.extend((f & 255).astype(np.uint8).tobytes())
            prev = cur
        return bytes(out)

    if interlace:
        raw = b"".join(filtered(pack_rows(s[y0::dy, x0::dx])) for x0, y0, dx, dy in _ADAM7 if s[y0::dy, x0::dx].size)
    else:
        raw = filtered(pack_rows(s))
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, strategy)
    z = co.compress(raw) + co.flush()

    def chunk(t: bytes, body: bytes) -> bytes:
        return struct.pack(">I", len(body)) + t + body + struct.pack(">I", zlib.crc32(t + body) & 0xFFFFFFFF)

    out = b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, color_type, 0, 0, 1 if interlace else 0))
    if palette is not None:
        out += chunk(b"PLTE", bytes(np.asarray(palette, np.uint8).reshape(-1)))
    if trns is not None:
        out += chunk(b"tRNS", bytes(trns))
    if idat_split:
        for k in range(0, len(z), idat_split):
            out += chunk(b"IDAT", z[k : k + idat_split])
    else:
        out += chunk(b"IDAT", z)
    return out + chunk(b"IEND", b"")


def _pad4(b: bytes, fill: bytes = b"\x00") -> bytes:
    return b + fill * ((4 - len(b) % 4) % 4)


def write_glb(desc, path: str, index_type: str = "auto", interleaved: bool = False, nodes=None, skins=None, animations=None,
              joints_type: str = "u16", weights_type: str = "f32", lights=None, cameras=None) -> None:
    """SceneDesc → GLB.  One glTF mesh per MeshDesc (one primitive each), one node per instance (TRS, or `matrix`
    when the instance carries one).  `nodes`: optional explicit node list (dicts with mesh/translation/rotation/
    scale/matrix/children) + root list, to exercise hierarchies: nodes=(node_dicts, root_indices).
    index_type: "u16" | "u32" | "auto" (u16 when the mesh has < 65536 vertices, like the reference's indices).
    Deformation: a MeshDesc with morph_dpos (/ morph_dnormal / morph_dtangent, morph_weights) gets `targets` (and `weights`), one with joints / weights gets
    JOINTS_0 (joints_type "u8" | "u16") and WEIGHTS_0 (weights_type "f32", or normalised "u8" | "u16").  skins: [{"joints": [node, ...],
    "inverseBindMatrices": (n, 16) column-major or None}] (a node dict names its skin with "skin").  animations: [{"channels": [{"node", "path"
    ("translation" | "rotation" (x, y, z, w) | "scale" | "weights"), "times", "values", "interpolation" ("LINEAR" | "STEP" | "CUBICSPLINE")}]}].
    lights: KHR_lights_punctual — [{"type" ("point" | "spot" | "directional"), "color", "intensity", "range", "inner", "outer" (cone angles, radians)}], each either on an
    existing node ("node": its index) or on a node of its own, appended behind the others in list order, with "translation", "rotation" (w, x, y, z), "scale" and "parent"
    (the index IN `lights` of the light whose node it hangs under; none: a root).  A light shines along its node's -Z.
    cameras: [{"type" ("perspective": "yfov", optional "aspectRatio", "znear"; "orthographic": "xmag", "ymag", "znear", "zfar")}], placed as lights are: on an existing
    node ("node"), or on a node of its own behind the others (and behind the lights' own nodes) with "translation", "rotation" (w, x, y, z), "scale" and "parent" (the
    index IN `cameras`).  A camera looks along its node's -Z with +Y up."""
    blob = bytearray()
    views, accessors, meshes = [], [], []

    def add_view(data: bytes, stride: int = 0, target: int = 0) -> int:
        while len(blob) % 4:
            blob.append(0)
        v = {"buffer": 0, "byteOffset": len(blob), "byteLength": len(data)}
        if stride:
            v["byteStride"] = stride
        if target:
            v["target"] = target
        blob.extend(data)
        views.append(v)
        return len(views) - 1

    def add_acc(view: int, ctype: int, count: int, typ: str, offset: int = 0, minmax=None) -> int:
        a = {"bufferView": view, "componentType": ctype, "count": count, "type": typ}
        if offset:
            a["byteOffset"] = offset
        if minmax is not None:
            a["min"], a["max"] = [float(x) for x in minmax[0]], [float(x) for x in minmax[1]]
        accessors.append(a)
        return len(accessors) - 1

    for m in desc.meshes:
        v = np.ascontiguousarray(m.vertices)
        n = v.size
        pos = np.ascontiguousarray(v["position"], "<f4")
        mm = (pos.min(0), pos.max(0))
        if interleaved:  # one 48-byte-stride view holding the R1 record as is
            bv = add_view(v.tobytes(), stride=48, target=34962)
            attrs = {"POSITION": add_acc(bv, 5126, n, "VEC3", 0, mm), "NORMAL": add_acc(bv, 5126, n, "VEC3", 12),
                     "TANGENT": add_acc(bv, 5126, n, "VEC4", 24), "TEXCOORD_0": add_acc(bv, 5126, n, "VEC2", 40)}
        else:
            attrs = {"POSITION": add_acc(add_view(pos.tobytes(), target=34962), 5126, n, "VEC3", 0, mm),
                     "NORMAL": add_acc(add_view(np.ascontiguousarray(v["normal"], "<f4").tobytes(), target=34962), 5126, n, "VEC3"),
                     "TANGENT": add_acc(add_view(np.ascontiguousarray(v["tangent"], "<f4").tobytes(), target=34962), 5126, n, "VEC4"),
                     "TEXCOORD_0": add_acc(add_view(np.ascontiguousarray(v["texCoords"], "<f4").tobytes(), target=34962), 5126, n, "VEC2")}
        idx = np.ascontiguousarray(m.indices, np.uint32)
        use16 = index_type == "u16" or (index_type == "auto" and n < 65536)
        ib = idx.astype("<u2").tobytes() if use16 else idx.astype("<u4").tobytes()
        ia = add_acc(add_view(ib, target=34963), 5123 if use16 else 5125, idx.size, "SCALAR")
        prim = {"attributes": attrs, "indices": ia, "material": int(m.material), "mode": 4}
        gm = {"primitives": [prim]}
        if getattr(m, "joints", None) is not None:
            j = np.ascontiguousarray(m.joints, "<u1" if joints_type == "u8" else "<u2")
            attrs["JOINTS_0"] = add_acc(add_view(j.tobytes(), target=34962), 5121 if joints_type == "u8" else 5123, n, "VEC4")
            w = np.asarray(m.weights, np.float32)
            if weights_type == "f32":
                attrs["WEIGHTS_0"] = add_acc(add_view(np.ascontiguousarray(w, "<f4").tobytes(), target=34962), 5126, n, "VEC4")
            else:
                top, dt, ct = (255, "<u1", 5121) if weights_type == "u8" else (65535, "<u2", 5123)
                attrs["WEIGHTS_0"] = add_acc(add_view(np.ascontiguousarray(np.rint(w * top), dt).tobytes(), target=34962), ct, n, "VEC4")
                accessors[attrs["WEIGHTS_0"]]["normalized"] = True
        if getattr(m, "morph_dpos", None) is not None:
            targets = []
            for k in range(len(m.morph_dpos)):
                t = {"POSITION": add_acc(add_view(np.ascontiguousarray(m.morph_dpos[k], "<f4").tobytes(), target=34962), 5126, n, "VEC3", 0,
                                         (np.asarray(m.morph_dpos[k]).min(0), np.asarray(m.morph_dpos[k]).max(0)))}
                if getattr(m, "morph_dnormal", None) is not None:
                    t["NORMAL"] = add_acc(add_view(np.ascontiguousarray(m.morph_dnormal[k], "<f4").tobytes(), target=34962), 5126, n, "VEC3")
                if getattr(m, "morph_dtangent", None) is not None:
                    t["TANGENT"] = add_acc(add_view(np.ascontiguousarray(m.morph_dtangent[k], "<f4").tobytes(), target=34962), 5126, n, "VEC3")
                targets.append(t)
            prim["targets"] = targets
            if getattr(m, "morph_weights", None) is not None:
                gm["weights"] = [float(x) for x in m.morph_weights]
        meshes.append(gm)

    images = []
    for t in getattr(desc, "textures", []) or []:   # RGBA8 images embedded as PNG bufferViews, one glTF texture per image
        images.append({"bufferView": add_view(png_encode(np.ascontiguousarray(t, np.uint8), 6, 8)), "mimeType": "image/png"})
    mats = []
    for m in desc.materials:
        e = [float(x) for x in m.emissive]
        strength = max(1.0, max(e))
        g = {"pbrMetallicRoughness": {"baseColorFactor": [float(x) for x in m.base_color], "metallicFactor": float(m.metallic), "roughnessFactor": float(m.roughness)},
             "emissiveFactor": [x / strength for x in e]}
        if getattr(m, "tex_color", -1) >= 0:
            g["pbrMetallicRoughness"]["baseColorTexture"] = {"index": int(m.tex_color)}
        if getattr(m, "tex_mr", -1) >= 0:
            g["pbrMetallicRoughness"]["metallicRoughnessTexture"] = {"index": int(m.tex_mr)}
        if getattr(m, "tex_normal", -1) >= 0:
            g["normalTexture"] = {"index": int(m.tex_normal)}
        if getattr(m, "emissive_texture", -1) >= 0:      # the texture's factor goes where glTF has it: emissiveFactor x emissive_strength
            e = [float(x) for x in getattr(m, "emissive_texture_factor", (1.0, 1.0, 1.0))]
            strength = max(1.0, max(e))
            g["emissiveFactor"] = [x / strength for x in e]
            g["emissiveTexture"] = {"index": int(m.emissive_texture)}
        if strength > 1.0:
            g["extensions"] = {"KHR_materials_emissive_strength": {"emissiveStrength": strength}}
        mode = getattr(m, "alpha_mode", None)      # None: the key is left out (glTF's default, OPAQUE); any string is written as given
        if mode is not None and not (mode == "opaque" and getattr(m, "alpha_cutoff", 0.5) == 0.5):
            g["alphaMode"] = str(mode).upper() if str(mode).lower() in ("opaque", "mask", "blend") else str(mode)
            if str(mode).lower() == "mask":
                g["alphaCutoff"] = float(getattr(m, "alpha_cutoff", 0.5))
        if getattr(m, "transmission", 0.0) > 0.0:      # KHR_materials_transmission, _ior and, for a solid, _volume (thicknessFactor 1: "has a volume")
            ext = g.setdefault("extensions", {})
            ext["KHR_materials_transmission"] = {"transmissionFactor": float(m.transmission)}
            ext["KHR_materials_ior"] = {"ior": float(getattr(m, "ior", 1.5))}
            if not getattr(m, "thin_walled", True):
                vol = {"thicknessFactor": 1.0, "attenuationColor": [float(x) for x in getattr(m, "attenuation_color", (1.0, 1.0, 1.0))]}
                if getattr(m, "attenuation_distance", 0.0) > 0.0:
                    vol["attenuationDistance"] = float(m.attenuation_distance)
                ext["KHR_materials_volume"] = vol
        mats.append(g)

    if nodes is None:
        node_list, roots = [], []
        for k, it in enumerate(desc.instances):
            nd = {"mesh": int(it.mesh), "name": f"inst{k}"}
            if getattr(it, "matrix", None) is not None:
                nd["matrix"] = [float(x) for x in np.asarray(it.matrix, np.float32).reshape(16)]
            else:
                q = it.q_wxyz
                nd["translation"] = [float(x) for x in it.t]
                nd["rotation"] = [float(q[1]), float(q[2]), float(q[3]), float(q[0])]  # glTF stores (x,y,z,w)
                nd["scale"] = [float(x) for x in it.s]
            node_list.append(nd)
            roots.append(k)
    else:
        node_list, roots = nodes
    light_defs = []
    if lights:
        node_list, roots = [dict(n) for n in node_list], list(roots)
        own = {}      # index in `lights` -> its own node
        for k, l in enumerate(lights):
            g = {"type": l["type"]}
            if "color" in l:
                g["color"] = [float(x) for x in l["color"]]
            if "intensity" in l:
                g["intensity"] = float(l["intensity"])
            if l.get("range"):
                g["range"] = float(l["range"])
            if l["type"] == "spot":
                g["spot"] = {kk: float(l[src]) for kk, src in (("innerConeAngle", "inner"), ("outerConeAngle", "outer")) if src in l}
            light_defs.append(g)
            if "node" in l:
                nd = node_list[int(l["node"])]
            else:
                nd = {"name": f"light{k}"}
                if "translation" in l:
                    nd["translation"] = [float(x) for x in l["translation"]]
                if "rotation" in l:
                    q = l["rotation"]
                    nd["rotation"] = [float(q[1]), float(q[2]), float(q[3]), float(q[0])]
                if "scale" in l:
                    nd["scale"] = [float(x) for x in l["scale"]]
                node_list.append(nd)
                own[k] = len(node_list) - 1
                if l.get("parent") is not None:
                    node_list[own[int(l["parent"])]].setdefault("children", []).append(own[k])
                else:
                    roots.append(own[k])
            nd.setdefault("extensions", {})["KHR_lights_punctual"] = {"light": k}
    camera_defs = []
    if cameras:
        node_list, roots = [dict(n) for n in node_list], list(roots)
        own = {}      # index in `cameras` -> its own node
        for k, c in enumerate(cameras):
            if c["type"] == "perspective":
                g = {"yfov": float(c["yfov"]), "znear": float(c.get("znear", 0.01))}
                if c.get("aspectRatio") is not None:
                    g["aspectRatio"] = float(c["aspectRatio"])
            else:
                g = {"xmag": float(c["xmag"]), "ymag": float(c["ymag"]), "znear": float(c.get("znear", 0.01)), "zfar": float(c.get("zfar", 1000.0))}
            camera_defs.append({"type": c["type"], c["type"]: g})
            if "node" in c:
                nd = node_list[int(c["node"])]
            else:
                nd = {"name": f"camera{k}"}
                if "translation" in c:
                    nd["translation"] = [float(x) for x in c["translation"]]
                if "rotation" in c:
                    q = c["rotation"]
                    nd["rotation"] = [float(q[1]), float(q[2]), float(q[3]), float(q[0])]
                if "scale" in c:
                    nd["scale"] = [float(x) for x in c["scale"]]
                node_list.append(nd)
                own[k] = len(node_list) - 1
                if c.get("parent") is not None:
                    node_list[own[int(c["parent"])]].setdefault("children", []).append(own[k])
                else:
                    roots.append(own[k])
            nd["camera"] = k
    doc = {"asset": {"version": "2.0", "generator": "pbr_amd.gltf.write_glb"}, "scene": 0, "scenes": [{"nodes": list(roots)}], "nodes": node_list,
           "meshes": meshes, "materials": mats, "accessors": accessors, "bufferViews": views, "buffers": [{"byteLength": len(blob)}]}
    if camera_defs:
        doc["cameras"] = camera_defs
    if skins:
        doc["skins"] = []
        for sk in skins:
            g = {"joints": [int(j) for j in sk["joints"]]}
            if sk.get("inverseBindMatrices") is not None:
                ibm = np.ascontiguousarray(sk["inverseBindMatrices"], "<f4").reshape(-1, 16)
                g["inverseBindMatrices"] = add_acc(add_view(ibm.tobytes()), 5126, ibm.shape[0], "MAT4")
            doc["skins"].append(g)
    if animations:
        doc["animations"] = []
        for an in animations:
            samplers, channels = [], []
            for ch in an["channels"]:
                times = np.ascontiguousarray(ch["times"], "<f4").reshape(-1)
                vals = np.ascontiguousarray(ch["values"], "<f4")
                typ = {"translation": "VEC3", "scale": "VEC3", "rotation": "VEC4", "weights": "SCALAR"}[ch["path"]]
                per = {"VEC3": 3, "VEC4": 4, "SCALAR": 1}[typ]
                samplers.append({"input": add_acc(add_view(times.tobytes()), 5126, times.size, "SCALAR", 0, ([times.min()], [times.max()])),
                                 "output": add_acc(add_view(vals.tobytes()), 5126, vals.size // per, typ), "interpolation": ch.get("interpolation", "LINEAR")})
                channels.append({"sampler": len(samplers) - 1, "target": {"node": int(ch["node"]), "path": ch["path"]}})
            doc["animations"].append({"samplers": samplers, "channels": channels})
    doc["buffers"] = [{"byteLength": len(blob)}]
    if images:
        doc["images"] = images
        doc["samplers"] = [{"magFilter": 9728, "minFilter": 9728, "wrapS": 10497, "wrapT": 10497}]   # NEAREST, REPEAT (what the reference uses regardless)
        doc["textures"] = [{"source": k, "sampler": 0} for k in range(len(images))]
    used = sorted({k for g in mats for k in g.get("extensions", {})})
    if used:
        doc["extensionsUsed"] = used
    if light_defs:
        doc["extensions"] = {"KHR_lights_punctual": {"lights": light_defs}}
        doc["extensionsUsed"] = doc.get("extensionsUsed", []) + ["KHR_lights_punctual"]
    js = _pad4(json.dumps(doc, separators=(",", ":")).encode(), b" ")
    bn = _pad4(bytes(blob))
    with open(path, "wb") as f:
        f.write(struct.pack("<4sII", b"glTF", 2, 12 + 8 + len(js) + 8 + len(bn)))
        f.write(struct.pack("<II", len(js), 0x4E4F534A) + js)
        f.write(struct.pack("<II", len(bn), 0x004E4942) + bn)
