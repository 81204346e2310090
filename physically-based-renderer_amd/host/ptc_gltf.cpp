// ptc_gltf.cpp — C-ABI wrapper of gltf_loader.hpp (include/ptc_gltf.h).
#include "gltf_loader.hpp"
#include "gltf_anim.hpp"
#include "image_io.hpp"

#include <ptc_gltf.h>

#include <cstdio>
#include <cstring>

extern "C" long long ptc_gltf_load(ptc_ctx* ctx, const char* path, int scene_index, int compose_parents, float bbox6[6], char* err, int err_len) {
  auto say = [&](const std::string& m) { if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", m.c_str()); };
  if (!ctx || !path) { say("ptc_gltf_load: null argument"); return PTC_E_ARG; }
  try {
    const pbr::gltf::FlatScene s = pbr::gltf::load(path, scene_index, compose_parents != 0);
    const int rc = pbr::gltf::upload(ctx, s);
    if (rc < 0) { say(std::string("ptc_gltf_load: ") + ptc_last_error(ctx)); return rc; }
    if (bbox6) { for (int k = 0; k < 3; ++k) { bbox6[k] = s.bbox_lo[k]; bbox6[3 + k] = s.bbox_hi[k]; } }
    return (long long)s.n_triangles;
  } catch (std::exception const& e) {
    say(std::string("ptc_gltf_load: ") + e.what());
    return PTC_E_ARG;
  }
}

extern "C" int ptc_gltf_emissive_textures(int on) {
  const bool was = pbr::gltf::emissive_textures_enabled();
  if (on >= 0) pbr::gltf::emissive_textures_enabled() = on != 0;
  return was ? 1 : 0;
}

// ---- the asset as a handle: skins, morph targets, animations (host/gltf_anim.hpp) ----
struct ptc_gltf_asset { pbr::gltf::Asset asset; std::string err; explicit ptc_gltf_asset(const char* path) : asset(path) {} };

extern "C" ptc_gltf_asset* ptc_gltf_open(const char* path, char* err, int err_len) {
  auto say = [&](const std::string& m) { if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", m.c_str()); };
  if (!path) { say("ptc_gltf_open: null argument"); return nullptr; }
  try { return new ptc_gltf_asset(path); }
  catch (std::exception const& e) { say(std::string("ptc_gltf_open: ") + e.what()); return nullptr; }
}
extern "C" void ptc_gltf_close(ptc_gltf_asset* a) { delete a; }
extern "C" const char* ptc_gltf_asset_last_error(const ptc_gltf_asset* a) { return a ? a->err.c_str() : "null asset"; }
extern "C" long long ptc_gltf_asset_load(ptc_gltf_asset* a, ptc_ctx* ctx, int scene_index, int compose_parents, float bbox6[6]) {
  if (!a || !ctx) return PTC_E_ARG;
  try {
    const long long n = a->asset.load_into(ctx, scene_index, compose_parents != 0, bbox6);
    if (n < 0) a->err = std::string("ptc_gltf_asset_load: ") + ptc_last_error(ctx);
    return n;
  } catch (std::exception const& e) { a->err = std::string("ptc_gltf_asset_load: ") + e.what(); return PTC_E_ARG; }
}
extern "C" int ptc_gltf_asset_animations(const ptc_gltf_asset* a) { return a ? a->asset.animations() : PTC_E_ARG; }
extern "C" double ptc_gltf_asset_duration(const ptc_gltf_asset* a, int animation) { return a ? a->asset.duration(animation) : -1.0; }
extern "C" int ptc_gltf_asset_pose(ptc_gltf_asset* a, ptc_ctx* ctx, int animation, double time_seconds) {
  if (!a || !ctx) return PTC_E_ARG;
  try {
    const int rc = a->asset.pose(ctx, animation, time_seconds);
    if (rc < 0) a->err = rc == PTC_E_ARG && (animation < 0 || animation >= a->asset.animations()) ? "ptc_gltf_asset_pose: animation out of range" : std::string("ptc_gltf_asset_pose: ") + ptc_last_error(ctx);
    return rc;
  } catch (std::exception const& e) { a->err = std::string("ptc_gltf_asset_pose: ") + e.what(); return PTC_E_ARG; }
}

extern "C" int ptc_gltf_asset_cameras(const ptc_gltf_asset* a) {
  if (!a) return PTC_E_ARG;
  try { return a->asset.cameras(); }
  catch (std::exception const&) { return PTC_E_ARG; }
}
extern "C" int ptc_gltf_asset_camera(ptc_gltf_asset* a, int index, int animation, double time_seconds, float frame_aspect, ptc_camera_params* out) {
  if (!a || !out) return PTC_E_ARG;
  try {
    const int rc = a->asset.camera(index, animation, time_seconds, frame_aspect, out);
    if (rc < 0) a->err = animation >= a->asset.animations() ? "ptc_gltf_asset_camera: animation out of range" : "ptc_gltf_asset_camera: camera index out of range";
    return rc;
  } catch (std::exception const& e) { a->err = std::string("ptc_gltf_asset_camera: ") + e.what(); return PTC_E_ARG; }
}
extern "C" int ptc_gltf_cameras(const char* path, int scene_index, int compose_parents, float frame_aspect, ptc_camera_params* out, int capacity, char* err, int err_len) {
  auto say = [&](const std::string& m) { if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", m.c_str()); };
  if (!path || capacity < 0 || (capacity > 0 && !out)) { say("ptc_gltf_cameras: bad argument"); return PTC_E_ARG; }
  try {
    const pbr::gltf::FlatScene s = pbr::gltf::load(path, scene_index, compose_parents != 0);
    for (size_t k = 0; k < s.cameras.size() && k < (size_t)capacity; ++k) pbr::gltf::detail::camera_params(s.cameras[k], frame_aspect, out + k);
    return (int)s.cameras.size();
  } catch (std::exception const& e) { say(std::string("ptc_gltf_cameras: ") + e.what()); return PTC_E_ARG; }
}

namespace {
template <class Decode>
int decode_into(const char* who, Decode&& dec, unsigned char* out, unsigned long long out_capacity, int* w, int* h, char* err, int err_len) {
  auto say = [&](const std::string& m) { if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", m.c_str()); };
  if (!w || !h) { say(std::string(who) + ": null argument"); return PTC_E_ARG; }
  try {
    const std::vector<std::uint8_t> px = dec(*w, *h);
    if (out) {
      if (out_capacity < px.size()) { say(std::string(who) + ": output buffer too small"); return PTC_E_ARG; }
      std::memcpy(out, px.data(), px.size());
    }
    return PTC_OK;
  } catch (std::exception const& e) {
    say(std::string(who) + ": " + e.what());
    return PTC_E_ARG;
  }
}
}  // namespace

extern "C" int ptc_jpeg_decode_rgba8(const unsigned char* data, unsigned long long n, unsigned char* out, unsigned long long out_capacity, int* w, int* h, char* err, int err_len) {
  if (!data) { if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "ptc_jpeg_decode_rgba8: null argument"); return PTC_E_ARG; }
  return decode_into("ptc_jpeg_decode_rgba8", [&](int& ww, int& hh) { return pbr::image::decode_jpeg(data, (std::size_t)n, ww, hh); }, out, out_capacity, w, h, err, err_len);
}

extern "C" int ptc_png_decode_rgba8(const unsigned char* data, unsigned long long n, unsigned char* out, unsigned long long out_capacity, int* w, int* h, char* err, int err_len) {
  auto say = [&](const std::string& m) { if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", m.c_str()); };
  if (!data || !w || !h) { say("ptc_png_decode_rgba8: null argument"); return PTC_E_ARG; }
  try {
    const std::vector<std::uint8_t> px = pbr::image::decode_png(data, (std::size_t)n, *w, *h);
    if (out) {
      if (out_capacity < px.size()) { say("ptc_png_decode_rgba8: output buffer too small"); return PTC_E_ARG; }
      std::memcpy(out, px.data(), px.size());
    }
    return PTC_OK;
  } catch (std::exception const& e) {
    say(std::string("ptc_png_decode_rgba8: ") + e.what());
    return PTC_E_ARG;
  }
}

extern "C" int ptc_hdr_decode_rgb32f(const unsigned char* data, unsigned long long n, float* out, unsigned long long out_capacity_floats, int* w, int* h, char* err, int err_len) {
  auto say = [&](const std::string& m) { if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "%s", m.c_str()); };
  if (!data || !w || !h) { say("ptc_hdr_decode_rgb32f: null argument"); return PTC_E_ARG; }
  try {
    const std::vector<float> px = pbr::image::decode_hdr(data, (std::size_t)n, *w, *h);
    if (out) {
      if (out_capacity_floats < px.size()) { say("ptc_hdr_decode_rgb32f: output buffer too small"); return PTC_E_ARG; }
      std::memcpy(out, px.data(), px.size() * sizeof(float));
    }
    return PTC_OK;
  } catch (std::exception const& e) {
    say(std::string("ptc_hdr_decode_rgb32f: ") + e.what());
    return PTC_E_ARG;
  }
}


// BMP / TGA / binary PGM-PPM (host/misc_decode.hpp); kind: 0 = by content in the reference's order (BMP, GIF, PSD, PIC, PNM, Radiance, TGA), 1 BMP, 2 TGA, 3 PNM, 4 Radiance as an 8-bit texture, 5 GIF, 6 PSD, 7 PIC
extern "C" int ptc_image_decode_rgba8(int kind, const unsigned char* data, unsigned long long n, unsigned char* out, unsigned long long out_capacity, int* w, int* h, char* err, int err_len) {
  if (!data) { if (err && err_len > 0) std::snprintf(err, (size_t)err_len, "ptc_image_decode_rgba8: null argument"); return PTC_E_ARG; }
  return decode_into("ptc_image_decode_rgba8", [&](int& ww, int& hh) {
    const std::size_t nn = (std::size_t)n;
    if (kind == 1 || (kind == 0 && pbr::image::is_bmp(data, nn))) return pbr::image::decode_bmp(data, nn, ww, hh);
    if (kind == 5 || (kind == 0 && pbr::image::is_gif(data, nn))) return pbr::image::decode_gif(data, nn, ww, hh);
    if (kind == 6 || (kind == 0 && pbr::image::is_psd(data, nn))) return pbr::image::decode_psd(data, nn, ww, hh);
    if (kind == 7 || (kind == 0 && pbr::image::is_pic(data, nn))) return pbr::image::decode_pic(data, nn, ww, hh);
    if (kind == 3 || (kind == 0 && pbr::image::is_pnm(data, nn))) return pbr::image::decode_pnm(data, nn, ww, hh);
    if (kind == 4 || (kind == 0 && pbr::image::is_hdr(data, nn))) return pbr::image::decode_hdr_rgba8(data, nn, ww, hh);
    if (kind == 2 || (kind == 0 && pbr::image::is_tga(data, nn))) return pbr::image::decode_tga(data, nn, ww, hh);
    throw std::runtime_error("not a BMP, GIF, PSD, PIC, PGM / PPM, Radiance or TGA image");
  }, out, out_capacity, w, h, err, err_len);
}
