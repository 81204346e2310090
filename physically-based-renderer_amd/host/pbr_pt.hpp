// pbr_pt.hpp — C++17 host-side mirror of the reference's scene interface over the C-ABI (include/ptc.h).
//
// Names and argument meaning follow the reference so that code written against it reads the same:
//   pbr::MeshVertex       src/pbr_engine/engine/pbr/MeshVertex.hpp:14-19
//   pbr::MeshBuilder      src/pbr_engine/engine/pbr/MeshBuilder.hpp:12-37   (indices widened to u32)
//   pbr::Transform        src/pbr_engine/engine/pbr/Scene.hpp:19-23         (rotation as w,x,y,z)
//   pbr::MaterialData     src/pbr_engine/engine/pbr/Material.hpp:14-16      (+ metal-rough, emissive)
//   pbr::PathTraceRenderSystem::render  replaces  pbr::PbrRenderSystem::render (PbrRenderSystem.hpp:46-47)
// Errors become std::runtime_error, like the reference's own failure sites (gltf_viewer/App.cpp:80,83).
#pragma once
#include <ptc.h>

#include <array>
#include <cmath>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace pbr {

struct MeshVertex {
  std::array<float, 3> position{};
  std::array<float, 3> normal{};
  std::array<float, 4> tangent{};
  std::array<float, 2> texCoords{};
};
static_assert(sizeof(MeshVertex) == sizeof(ptc_vertex), "R1: 48-byte vertex record");

struct Transform {
  std::array<float, 3> position{0, 0, 0};
  std::array<float, 4> rotation{1, 0, 0, 0};   // w, x, y, z
  std::array<float, 3> scale{1, 1, 1};
};

struct MaterialData {
  std::array<float, 4> color{1, 1, 1, 1};
  float metallic = 0.0f, roughness = 1.0f;
  std::array<float, 3> emissive{0, 0, 0};
  int alphaMode = PTC_ALPHA_OPAQUE;      // glTF alphaMode: PTC_ALPHA_OPAQUE / _MASK / _BLEND (ptc_set_material_alpha; an emissive material must stay opaque)
  float alphaCutoff = 0.5f;
  // KHR_materials_transmission / _ior / _volume (ptc_set_material_transmission): an emissive or non-opaque material must stay at transmission 0
  float transmission = 0.0f, ior = 1.5f;
  bool thinWalled = true;
  std::array<float, 3> attenuationColor{1, 1, 1};
  float attenuationDistance = 0.0f;
};

// The viewer's start-up camera: app::CameraController's defaults (src/gltf_viewer/CameraController.hpp:25-40: position 0, pitch 0,
// yaw -pi/2, vertical fov pi/2) and its getDirection() / getCameraData() (CameraController.hpp:128-136), in the same float arithmetic.
struct ViewerCamera {
  std::array<float, 3> position{0.0f, 0.0f, 0.0f};
  float pitch = 0.0f, yaw = -1.57079632679489661923f, fov = 1.57079632679489661923f;
  [[nodiscard]] auto direction() const -> std::array<float, 3> {
    const float cp = std::cos(pitch);
    const float x = cp * std::cos(yaw), y = std::sin(pitch), z = cp * std::sin(yaw);
    const float il = 1.0f / std::sqrt(x * x + y * y + z * z);
    return {x * il, y * il, z * il};
  }
  [[nodiscard]] auto target() const -> std::array<float, 3> { const auto d = direction(); return {position[0] + d[0], position[1] + d[1], position[2] + d[2]}; }
};

struct PrimitiveSpan { int material; std::uint32_t firstVertex, vertexCount, firstIndex, indexCount; };

class MeshBuilder {
public:
  struct Primitive { int material = 0; std::vector<MeshVertex> vertices; std::vector<std::uint32_t> indices; };
  struct BuiltMesh { std::vector<MeshVertex> vertices; std::vector<std::uint32_t> indices; std::vector<PrimitiveSpan> primitives; };
  auto addPrimitive(Primitive p) -> MeshBuilder& { _primitives.emplace_back(std::move(p)); return *this; }
  [[nodiscard]] auto build() const -> BuiltMesh {
    BuiltMesh b;
    std::uint32_t cv = 0, ci = 0;
    for (auto const& p : _primitives) {
      b.vertices.insert(b.vertices.end(), p.vertices.begin(), p.vertices.end());
      b.indices.insert(b.indices.end(), p.indices.begin(), p.indices.end());
      b.primitives.push_back({p.material, cv, (std::uint32_t)p.vertices.size(), ci, (std::uint32_t)p.indices.size()});
      cv += (std::uint32_t)p.vertices.size();
      ci += (std::uint32_t)p.indices.size();
    }
    return b;
  }
private:
  std::vector<Primitive> _primitives;
};

class PathTraceRenderSystem {
public:
  explicit PathTraceRenderSystem(int device) : _ctx(ptc_create(device)) {
    if (!_ctx) throw std::runtime_error(ptc_last_error(nullptr));
  }
  // a view of a context owned elsewhere (one device of a DeviceGroup)
  explicit PathTraceRenderSystem(ptc_ctx* borrowed) : _ctx(borrowed), _owned(false) {
    if (!_ctx) throw std::runtime_error("PathTraceRenderSystem: null context");
  }
  ~PathTraceRenderSystem() { if (_owned) ptc_destroy(_ctx); }
  PathTraceRenderSystem(PathTraceRenderSystem const&) = delete;
  auto operator=(PathTraceRenderSystem const&) -> PathTraceRenderSystem& = delete;

  auto beginScene() -> void { ck(ptc_scene_begin(_ctx)); }
  auto addMaterial(MaterialData const& m) -> int {
    const int id = ck(ptc_add_material(_ctx, m.color.data(), m.metallic, m.roughness, m.emissive.data(), -1, -1, -1));
    if (m.alphaMode != PTC_ALPHA_OPAQUE) ck(ptc_set_material_alpha(_ctx, id, m.alphaMode, m.alphaCutoff));
    if (m.transmission > 0.0f) {
      const ptc_transmission_params t{m.transmission, m.ior, m.thinWalled ? 1 : 0, {m.attenuationColor[0], m.attenuationColor[1], m.attenuationColor[2]}, m.attenuationDistance};
      ck(ptc_set_material_transmission(_ctx, id, &t));
    }
    return id;
  }
  // one ptc mesh per PrimitiveSpan, firstVertex applied like drawIndexed's vertexOffset (PbrRenderSystem.cpp:454-460)
  auto addMesh(MeshBuilder::BuiltMesh const& b) -> std::vector<int> {
    std::vector<int> ids;
    for (auto const& s : b.primitives)
      ids.push_back(ck(ptc_add_mesh(_ctx, reinterpret_cast<ptc_vertex const*>(b.vertices.data() + s.firstVertex), s.vertexCount,
                                    b.indices.data() + s.firstIndex, s.indexCount, s.material)));
    return ids;
  }
  auto addInstance(int mesh, Transform const& t) -> void { ck(ptc_add_instance(_ctx, mesh, t.position.data(), t.rotation.data(), t.scale.data())); }
  // pbr::makeCameraData(position, target, fov, aspect), CameraData.hpp:22-32
  auto setCamera(std::array<float, 3> position, std::array<float, 3> target, float fov, float aspect) -> void {
    ck(ptc_set_camera(_ctx, position.data(), target.data(), fov, aspect));
  }
  // ---- thin-lens camera (include/ptc.h; the reference's camera is a pinhole): depth of field for the path integrator ----
  // apertureRadius 0 = pinhole; blades 0 = disk, 3..16 = regular polygon with a vertex at `rotation` turns; focusDistance = view depth of the plane of focus.
  // Kept across setCamera, reset by beginScene; the raster integrators and the guides ignore it
  static auto lensDefaults() -> ptc_lens_params { ptc_lens_params p; ptc_lens_default_params(&p); return p; }
  auto setCameraLens(ptc_lens_params const& lens) -> void { ck(ptc_set_camera_lens(_ctx, &lens)); }
  auto setCameraLens(float apertureRadius, float focusDistance, int blades = 0, float rotation = 0.0f) -> void {
    setCameraLens(ptc_lens_params{apertureRadius, focusDistance, blades, rotation});
  }
  auto cameraLens() const -> ptc_lens_params { ptc_lens_params p; ptc_get_camera_lens(_ctx, &p); return p; }
  // ---- camera models (include/ptc_camera.h): a camera-to-world matrix in glTF camera space with a perspective, orthographic or equirectangular projection ----
  // Replaces setCamera's camera and is replaced by it; dropped by beginScene; needs no commit
  static auto cameraDefaults() -> ptc_camera_params { ptc_camera_params p; ptc_camera_default_params(&p); return p; }
  auto setCameraEx(ptc_camera_params const& camera) -> void { ck(ptc_set_camera_ex(_ctx, &camera)); }
  auto cameraEx(ptc_camera_params& out) const -> bool { return ptc_get_camera_ex(_ctx, &out) == 1; }
  // punctual lights (ptc_add_light ...): point / spot / directional, sampled by the path integrator in a pass of its own.  They need no commit and no
  // refit; a frame sees the lights recorded when it began.  Dropped by beginScene
  static auto lightDefaults() -> ptc_light_params { ptc_light_params p; ptc_light_default_params(&p); return p; }
  auto addLight(ptc_light_params const& light) -> int { return ck(ptc_add_light(_ctx, &light)); }
  auto updateLight(int id, ptc_light_params const& light) -> void { ck(ptc_update_light(_ctx, id, &light)); }
  auto light(int id) const -> ptc_light_params { ptc_light_params p = lightDefaults(); ptc_get_light(_ctx, id, &p); return p; }
  auto lightCount() const -> int { return ptc_light_count(_ctx); }
  auto clearLights() -> void { ck(ptc_clear_lights(_ctx)); }
  // transparent shadows (include/ptc_glass_shadows.h): shadow rays pass thin-walled transmissive panes with their expected transmittance.  Off by
  // default, kept across beginScene; a frame renders with the value it was begun with
  auto setGlassShadows(bool on) -> void { ck(ptc_set_glass_shadows(_ctx, on ? 1 : 0)); }
  auto glassShadows() const -> bool { int on = 0; ptc_get_glass_shadows(_ctx, &on); return on != 0; }
  auto glassShadowStats() -> ptc_glass_shadow_stats { ptc_glass_shadow_stats s{}; ck(ptc_get_glass_shadow_stats(_ctx, &s)); return s; }
  // the participating medium (include/ptc_medium.h): a homogeneous fog box.  Recorded like a light — no commit, dropped by beginScene — and used by the
  // next frame; sigma_t 0 or clearMedium(): off
  auto setMedium(const ptc_medium_params& m) -> void { ck(ptc_set_medium(_ctx, &m)); }
  auto clearMedium() -> void { ck(ptc_clear_medium(_ctx)); }
  auto mediumStats() -> ptc_medium_stats { ptc_medium_stats s{}; ck(ptc_get_medium_stats(_ctx, &s)); return s; }
  // the view depth of what pixel (x, y)'s centre sees, 0 on a miss: needs frameGuides() of the current frame
  auto focusDistanceAtPixel(int x, int y) -> float { float d = 0.0f; ck(ptc_focus_distance_at_pixel(_ctx, x, y, &d)); return d; }
  // PTC_BVH_SAH (default) or PTC_BVH_LBVH, for the scene being described
  auto setBvhBuilder(int builder) -> void { ck(ptc_set_bvh_builder(_ctx, builder)); }
  // the tree a build on the device makes (kept across beginScene): PTC_BVH_LBVH (default), or PTC_BVH_SAH — a SAH scene then commits on the device and
  // ptc_scene_rebuild makes the SAH tree
  auto setDeviceBuilder(int builder) -> void { ck(ptc_set_device_builder(_ctx, builder)); }
  auto commitScene() -> void { ck(ptc_scene_commit(_ctx)); }

  // replaces PbrRenderSystem::render: fills an fp32 RGBA radiance buffer (w*h*4, y-down)
  auto render(int w, int h, int spp, std::uint64_t seed, int maxBounces, int integrator = PTC_INTEGRATOR_PATH) -> std::vector<float> {
    ck(ptc_render(_ctx, w, h, spp, seed, maxBounces, integrator));
    std::vector<float> out((std::size_t)w * h * 4);
    ck(ptc_read_radiance_rgba32f(_ctx, out.data()));
    _w = w; _h = h;
    return out;
  }
  // TonemapperSystem::run (TonemapperSystem.cpp:97-134)
  auto tonemap() -> std::vector<std::uint8_t> {
    std::vector<std::uint8_t> out((std::size_t)_w * _h * 4);
    ck(ptc_tonemap_rgba8(_ctx, out.data()));
    return out;
  }
  // ---- display transform (include/ptc.h): exposure (fixed, or metered on the device), tone-mapping operator, transfer function.  The radiance is in
  // physical units; tonemap() and radianceHalf() take it as it is, these expose it first.  The parameters are a context setting, kept across beginScene
  static auto displayDefaults() -> ptc_display_params { ptc_display_params p; ptc_display_default_params(&p); return p; }
  auto setDisplay(ptc_display_params const& params) -> void { ck(ptc_set_display(_ctx, &params)); }
  auto displayParams() const -> ptc_display_params { ptc_display_params p; ptc_get_display(_ctx, &p); return p; }
  // meters the image selectOutput serves and moves the adaptation state; queued on the context's stream, does not wait: display() / displayHalf() behind it use it
  auto meterExposure() -> void { ck(ptc_meter_exposure(_ctx)); }
  auto exposureReset() -> void { ck(ptc_exposure_reset(_ctx)); }
  struct Exposure { float scale = 1.0f, adaptedLuminance = 0.0f, meteredLuminance = 0.0f; std::uint64_t metered = 0, rejected = 0; };
  auto exposure() -> Exposure { Exposure e; ck(ptc_get_exposure(_ctx, &e.scale, &e.adaptedLuminance, &e.meteredLuminance, &e.metered, &e.rejected)); return e; }
  auto luminanceHistogram() -> std::vector<std::uint32_t> { std::vector<std::uint32_t> h(4096); ck(ptc_read_luminance_histogram(_ctx, h.data())); return h; }
  auto display() -> std::vector<std::uint8_t> {
    std::vector<std::uint8_t> out((std::size_t)_w * _h * 4);
    ck(ptc_display_rgba8(_ctx, out.data()));
    return out;
  }
  // the exposed image as RGBA16F, for a viewer's own tonemapper; displayHalfDevicePtr: the same in device memory (valid until the next of the two calls)
  auto displayHalf() -> std::vector<std::uint16_t> {
    std::vector<std::uint16_t> out((std::size_t)_w * _h * 4);
    ck(ptc_display_rgba16f(_ctx, out.data()));
    return out;
  }
  auto displayHalfDevicePtr() -> void* { return ptc_display_rgba16f_device_ptr(_ctx); }
  // HIP-event seconds of the last meterExposure() and the last display kernel
  auto displaySeconds() -> std::array<double, 2> { std::array<double, 2> t{0.0, 0.0}; ck(ptc_get_display_seconds(_ctx, &t[0], &t[1])); return t; }
  // the same image in the reference's HdrImage format, RGBA16F (PbrRenderSystem.hpp:21, HdrImage.cpp:20): what a viewer shim
  // copies into the image the tonemapper samples
  auto radianceHalf() -> std::vector<std::uint16_t> {
    std::vector<std::uint16_t> out((std::size_t)_w * _h * 4);
    ck(ptc_read_radiance_rgba16f(_ctx, out.data()));
    return out;
  }
  auto readRadiance(int w, int h) -> std::vector<float> {
    std::vector<float> out((std::size_t)w * h * 4);
    ck(ptc_read_radiance_rgba32f(_ctx, out.data()));
    _w = w; _h = h;
    return out;
  }
  // ---- first-hit guides, denoiser, output selection (include/ptc.h; the reference has no counterpart: its raster image is noise-free) ----
  // guides of every pixel of the frame in progress (render() leaves its frame open, and so does DeviceGroup::render on device(0))
  auto frameGuides() -> void { ck(ptc_frame_guides(_ctx)); }
  // PTC_GUIDE_ALBEDO: (albedo rgb, class 0 miss / 1 surface / 2 emitter); PTC_GUIDE_NORMAL_DEPTH: (vertex normal, t along the unit camera ray)
  auto readGuide(int which) -> std::vector<float> {
    std::vector<float> out((std::size_t)_w * _h * 4);
    ck(ptc_read_guide_rgba32f(_ctx, which, out.data()));
    return out;
  }
  auto readGuideHit(std::vector<std::int32_t>& prim, std::vector<float>& uv) -> void {
    prim.resize((std::size_t)_w * _h); uv.resize((std::size_t)_w * _h * 2);
    ck(ptc_read_guide_hit(_ctx, prim.data(), uv.data()));
  }
  static auto denoiseDefaults() -> ptc_denoise_params { ptc_denoise_params p; ptc_denoise_default_params(&p); return p; }
  // radiance buffer + guides -> the denoised buffer; selectOutput(PTC_OUTPUT_DENOISED) makes readRadiance / radianceHalf / tonemap serve it
  auto denoise(ptc_denoise_params const* params = nullptr) -> void { ck(ptc_denoise(_ctx, params)); }
  auto selectOutput(int output) -> void { ck(ptc_select_output(_ctx, output)); }
  // HIP-event seconds of the last frameGuides() and the last denoise()
  auto denoiseSeconds() -> std::array<double, 2> { std::array<double, 2> t{0.0, 0.0}; ck(ptc_get_denoise_seconds(_ctx, &t[0], &t[1])); return t; }
  // ---- temporal accumulation (include/ptc.h): the previous frames' result, reprojected through the guides, blended with this frame's radiance buffer ----
  static auto temporalDefaults() -> ptc_temporal_params { ptc_temporal_params p; ptc_temporal_default_params(&p); return p; }
  // needs frameGuides() of the current frame; selectOutput(PTC_OUTPUT_ACCUMULATED) serves the accumulated image.  The history survives a new frame, a new
  // camera, refit() and rebuild(); temporalReset() and a new commit drop it
  auto temporalAccumulate(ptc_temporal_params const* params = nullptr) -> void { ck(ptc_temporal_accumulate(_ctx, params)); }
  auto temporalReset() -> void { ck(ptc_temporal_reset(_ctx)); }
  // PTC_TEMPORAL_HISTORY (D rgb, n), PTC_TEMPORAL_MOMENTS (m1, m2, Var_t, a), PTC_TEMPORAL_MOTION (x_prev, y_prev, W, reprojected n), PTC_TEMPORAL_NORMAL_DEPTH (N, Z) and
  // PTC_TEMPORAL_POSITION_CLASS (P, K: the history's copies of its frame's guides).  w x h: the current frame's size, which must be the accumulated frame's — the library
  // refuses (PTC_E_STATE -> an exception) when a frame of another size was begun since the accumulate, so the buffer sized here is the size that is copied
  auto readTemporal(int which, int w, int h) -> std::vector<float> {
    std::vector<float> out((std::size_t)w * (std::size_t)h * 4);
    ck(ptc_read_temporal_rgba32f(_ctx, which, out.data()));
    return out;
  }
  // the denoiser's iterations over the accumulated image -> the denoised buffer (PTC_OUTPUT_DENOISED)
  auto denoiseAccumulated(ptc_denoise_params const* params = nullptr) -> void { ck(ptc_denoise_accumulated(_ctx, params)); }
  auto temporalSeconds() -> double { double t = 0.0; ck(ptc_get_temporal_seconds(_ctx, &t)); return t; }
  // ---- adaptive sampling (include/ptc.h): samples go to the pixels whose estimate has not converged; at most maxSpp per pixel ----
  static auto adaptiveDefaults() -> ptc_adaptive_params { ptc_adaptive_params p; ptc_adaptive_default_params(&p); return p; }
  auto renderAdaptive(int w, int h, int maxSpp, std::uint64_t seed, int maxBounces, ptc_adaptive_params const* params = nullptr) -> std::vector<float> {
    ck(ptc_render_adaptive(_ctx, w, h, maxSpp, seed, maxBounces, params));
    return readRadiance(w, h);
  }
  // the caller-driven form: after ptc_frame_begin, setAdaptive(); then ptc_frame_add_samples feeds the active pixels and adapt() takes the converged ones out
  auto setAdaptive(ptc_adaptive_params const* params = nullptr) -> void { ck(ptc_frame_set_adaptive(_ctx, params)); }
  auto adapt() -> std::uint64_t { std::uint64_t n = 0; ck(ptc_frame_adapt(_ctx, &n)); return n; }
  auto sampleCounts() -> std::vector<std::uint32_t> {
    std::vector<std::uint32_t> out((std::size_t)_w * _h);
    ck(ptc_read_sample_counts(_ctx, out.data()));
    return out;
  }
  auto adaptiveStats() -> ptc_adaptive_stats { ptc_adaptive_stats s; ck(ptc_get_adaptive_stats(_ctx, &s)); return s; }
  // ---- denoising from per-sample statistics (include/ptc.h): adaptive frames begun while the setting is on keep the RGB covariance of their samples ----
  auto setSampleCovariance(bool on) -> void { ck(ptc_set_sample_covariance(_ctx, on ? 1 : 0)); }
  // the raw sums (rr, gg, bb, rg, rb, gb) per pixel of the current frame
  auto sampleCovariance() -> std::vector<float> {
    std::vector<float> out((std::size_t)_w * _h * 6);
    ck(ptc_read_sample_covariance(_ctx, out.data()));
    return out;
  }
  // after ptc_frame_resolve and frameGuides(): the denoiser's iterations with the variance of the frame's own samples -> the denoised buffer (PTC_OUTPUT_DENOISED)
  auto denoiseSampled(ptc_denoise_params const* params = nullptr) -> void { ck(ptc_denoise_sampled(_ctx, params)); }
  // (Var_s, 1 / n) per pixel as the last denoiseSampled() computed them
  auto sampledVariance() -> std::vector<float> {
    std::vector<float> out((std::size_t)_w * _h * 2);
    ck(ptc_read_sampled_variance(_ctx, out.data()));
    return out;
  }
  // a uniform frame that keeps the statistics: an adaptive frame without a decision step, whose image is render()'s bit for bit
  auto renderWithStatistics(int w, int h, int spp, std::uint64_t seed, int maxBounces) -> std::vector<float> {
    setSampleCovariance(true);
    ck(ptc_frame_begin(_ctx, w, h, spp, seed, maxBounces, PTC_INTEGRATOR_PATH, 0, 1));
    ck(ptc_frame_set_adaptive(_ctx, nullptr));
    ck(ptc_frame_add_samples(_ctx, spp));
    ck(ptc_frame_resolve(_ctx));
    ck(ptc_sync(_ctx));
    return readRadiance(w, h);
  }
  // light probes (ptc_probes_begin ...): positions = 3 floats per probe; 27 floats per probe come back, laid out [probe][k][rgb]
  auto renderProbes(std::vector<float> const& positions, int spp, std::uint64_t seed = 0, int maxBounces = 8) -> std::vector<float> {
    std::vector<float> out(positions.size() / 3 * 27);
    ck(ptc_render_probes(_ctx, positions.data(), (int)(positions.size() / 3), spp, seed, maxBounces, out.data()));
    _probes = positions.size() / 3;      // the probe frame stays in progress: readProbesSh() may follow
    return out;
  }
  // the caller-driven form: beginProbes(), ptc_frame_add_samples as in any frame, readProbesSh() whenever coefficients are wanted; indexBase shards a probe set
  auto beginProbes(std::vector<float> const& positions, int sppTotal, std::uint64_t seed = 0, int maxBounces = 8, std::uint32_t indexBase = 0) -> void {
    ck(ptc_probes_begin(_ctx, positions.data(), (int)(positions.size() / 3), indexBase, sppTotal, seed, maxBounces));
    _probes = positions.size() / 3;
  }
  auto readProbesSh() -> std::vector<float> {
    if (!_probes) throw std::runtime_error("readProbesSh: no probe frame was begun through this object (beginProbes / renderProbes)");
    std::vector<float> out(_probes * 27);      // ptc_probes_read_sh writes 27 floats per probe of the frame in progress
    ck(ptc_probes_read_sh(_ctx, out.data()));
    return out;
  }
  // lightmaps (ptc_lightmap_begin ...): the irradiance over the width x height atlas of one instance, spp samples per covered texel: width * height
  // RGBA floats, row 0 first — RGB the irradiance, alpha 1 baked / 0.5 filled by dilation / 0 empty.  uv: 2 floats per vertex of the instance's mesh, or empty = the
  // mesh's texCoords; texels whose first hits are back faces in more than backfaceThreshold of their samples are invalid and filled from their neighbours
  auto bakeLightmap(int instance, int width, int height, int spp, std::vector<float> const& uv = {}, std::uint64_t seed = 0, int maxBounces = 8, int dilateIters = 2,
                    float backfaceThreshold = 0.1f, std::uint32_t indexBase = 0) -> std::vector<float> {
    ptc_lightmap_desc d{};
    d.instance = instance; d.width = width; d.height = height; d.uv = uv.empty() ? nullptr : uv.data(); d.texel_index_base = indexBase; d.spp_total = spp; d.seed = seed;
    d.max_bounces = maxBounces;
    std::vector<float> out(width > 0 && height > 0 ? (std::size_t)width * (std::size_t)height * 4 : 0);
    ck(ptc_render_lightmap(_ctx, &d, dilateIters, backfaceThreshold, out.empty() ? nullptr : out.data()));
    return out;
  }
  // (entries, owned texels dropped for a degenerate world triangle) of the lightmap frame in progress
  auto lightmapTexelCount() -> std::array<std::uint32_t, 2> { std::array<std::uint32_t, 2> n{}; ck(ptc_lightmap_texel_count(_ctx, &n[0], &n[1])); return n; }
  static auto sh9Eval(float const* sh27, std::array<float, 3> const& dir) -> std::array<float, 3> { std::array<float, 3> o{}; ptc_sh9_eval(sh27, dir.data(), o.data()); return o; }
  static auto sh9Irradiance(float const* sh27, std::array<float, 3> const& normal) -> std::array<float, 3> { std::array<float, 3> o{}; ptc_sh9_irradiance(sh27, normal.data(), o.data()); return o; }
  auto stats() -> ptc_stats { ptc_stats s; ck(ptc_get_stats(_ctx, &s)); return s; }
  auto handle() -> ptc_ctx* { return _ctx; }

private:
  auto ck(int rc) -> int { if (rc < 0) throw std::runtime_error(ptc_last_error(_ctx)); return rc; }
  ptc_ctx* _ctx;
  bool _owned = true;
  int _w = 0, _h = 0;
  std::size_t _probes = 0;
};

// Several GPUs driven by one process (ptc_group: one context per device + an RCCL communicator): the scene described on device(0) is
// committed to every device by commitScene(), render() traces device i's 32x32-pixel tiles on device i and reduces the framebuffer onto device 0 (ncclReduce).
// The reference has a single vk::Device (core/GpuHandle.cpp:94-101); this is the build's multi-GPU addition.
class DeviceGroup {
public:
  explicit DeviceGroup(std::vector<int> const& devices) : _g(ptc_group_create(devices.data(), (int)devices.size())) {
    if (!_g) throw std::runtime_error(ptc_group_last_error(nullptr));
    for (int i = 0; i < ptc_group_size(_g); ++i) _views.emplace_back(new PathTraceRenderSystem(ptc_group_ctx(_g, i)));
  }
  ~DeviceGroup() { _views.clear(); ptc_group_destroy(_g); }
  DeviceGroup(DeviceGroup const&) = delete;
  auto operator=(DeviceGroup const&) -> DeviceGroup& = delete;
  [[nodiscard]] auto size() const -> int { return (int)_views.size(); }
  auto device(int i) -> PathTraceRenderSystem& { return *_views[(std::size_t)i]; }
  // the scene described (and possibly committed) on device(0) goes to every device with one host build
  void commitScene() { if (ptc_group_scene_commit(_g) < 0) throw std::runtime_error(ptc_group_last_error(_g)); }
  auto render(int w, int h, int spp, std::uint64_t seed, int maxBounces, int integrator = PTC_INTEGRATOR_PATH) -> std::vector<float> {
    if (ptc_group_render(_g, w, h, spp, seed, maxBounces, integrator) < 0) throw std::runtime_error(ptc_group_last_error(_g));
    return _views[0]->readRadiance(w, h);
  }

private:
  ptc_group* _g;
  std::vector<std::unique_ptr<PathTraceRenderSystem>> _views;
};

}  // namespace pbr
