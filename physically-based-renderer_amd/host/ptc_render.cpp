// ptc_render — dependency-free C++17 offline renderer over the C-ABI (include/ptc.h).
//   ptc_render (--scene cornell|sphere | --gltf file.glb [--animation N --time T] [--cam-pos x y z --cam-target x y z --fov deg | --viewer-camera]) --width W --height H
//              --spp N --seed S --bounces B [--raster | --raster16] [--env latlong.pfm|latlong.hdr | --sky] [--filter nearest|linear] [--bvh sah|lbvh] [--device-bvh sah|lbvh] [--device D] [--gpus N]
//              --out image.pfm [--png image.png] [--ppm image.ppm] [--half image.f16] [--denoise] [--denoise-iters N] [--denoise-sampled] [--guides PREFIX]
//              [--adaptive THRESH [--min-spp N] [--spp-step N] [--adaptive-radius R] [--counts out.pfm]]
//              [--aperture R [--blades N] [--aperture-rotation T] [--focus D | --focus-pixel X,Y]]
//              [--light point:x,y,z:r,g,b[:range]] [--light spot:x,y,z:dx,dy,dz:r,g,b:inner_deg,outer_deg[:range]] [--light sun:dx,dy,dz:r,g,b] [--no-gltf-lights] [--no-alpha] [--no-transmission] [--no-emissive-textures] [--glass-shadows]
//              [--fog x,y,z:x,y,z:sigma_t[:albedo[:g]] | --fog scene:sigma_t[:albedo[:g]]]
//              [--exposure EV] [--auto-exposure [--key K]] [--tonemap aces|neutral|reinhard|clamp] [--srgb]
//              [(--probe-grid NX,NY,NZ | --probes positions.txt) --probes-out sh.pfm]
//              [--lightmap INSTANCE:WxH --lightmap-out lm.pfm [--lightmap-alpha a.pfm] [--lightmap-dilate N] [--lightmap-backface F]]
// --lightmap INSTANCE:WxH with --lightmap-out lm.pfm: bake the irradiance on instance INSTANCE over its W x H UV atlas (the mesh's texture coordinates) instead of an
// image (ptc_render_lightmap), at --spp samples per covered texel, --seed, --bounces.  lm.pfm holds the irradiance, row 0 of the atlas (v = 0) at the
// top; --lightmap-alpha writes the coverage (1 baked, 0.5 filled, 0 empty) in all three channels.  --lightmap-dilate N: N dilation iterations into the gutters
// (default 2, 0..64); --lightmap-backface F: a texel whose first hits are back faces in more than F of its samples is invalid and filled from its neighbours
// (default 0.1; 1 switches the test off).  One context, path integrator.  Bad values are reported before any device work.
// --probe-grid NX,NY,NZ / --probes FILE with --probes-out sh.pfm: bake light probes instead of an image (ptc_render_probes) — the centres of the
// NX x NY x NZ cells of the scene's bounding box (x fastest, then y, then z; the grid's origin and cell size are printed), or the `x y z` lines of a text file —
// at --spp samples each, --seed, --bounces.  sh.pfm is a 9 x n RGB image: row j holds the nine SH coefficients of probe j.  One context, path integrator.
// --exposure EV / --auto-exposure / --tonemap / --srgb: the display transform (ptc_set_display) for --png, --ppm and --half.  --exposure multiplies the
// radiance by 2^EV; --auto-exposure meters the image on the device (ptc_meter_exposure) and maps its metered luminance to the key K (default 0.18), times 2^EV;
// --tonemap picks the operator (neutral: Khronos PBR Neutral) and --srgb the sRGB transfer function instead of gamma 2.2; --half then holds the exposed radiance.
// With none of them the three files are what ptc_tonemap_rgba8 and ptc_read_radiance_rgba16f give.  Bad values are reported before any device work.
// --light (repeatable): a punctual light (ptc_add_light), path integrator only.  point / spot: position, intensity rgb in W/sr, an optional range; a spot points along
// dx,dy,dz with full intensity inside inner_deg of the axis and none outside outer_deg.  sun: a directional light travelling along dx,dy,dz, rgb = the irradiance of a
// facing surface.  A --gltf scene brings the KHR_lights_punctual lights of its nodes (with --animation they move with them); --no-gltf-lights drops those.
// Bad values are reported before any device work.
// --no-alpha: a --gltf scene is rendered with the alphaMode of its materials (MASK: holes where the alpha lies below alphaCutoff, BLEND: stochastic coverage and
// attenuated shadows; ptc_set_material_alpha), path integrator only; --no-alpha renders every material opaque, as the raster integrators always do.
// --no-transmission: a --gltf scene is rendered with KHR_materials_transmission, KHR_materials_ior and KHR_materials_volume of its materials (glass and thin panes;
// ptc_set_material_transmission), path integrator only; --no-transmission renders them as the opaque surfaces they were before.
// --no-emissive-textures: a --gltf scene is rendered with the emissiveTexture of its materials (ptc_set_material_emission_texture, DESIGN.md §2h: the texture masks the
// emission; path integrator only, and not with --fog); --no-emissive-textures reads such a material as a uniform emitter of its emissiveFactor, as before.
// --glass-shadows: shadow rays pass thin-walled transmissive panes with their expected transmittance (ptc_set_glass_shadows): punctual lights, emitters
// and the environment light what lies behind a window directly.  Off by default; with --gpus device D's setting goes to every member.
// --fog LO:HI:SIGMA_T[:ALBEDO[:G]]: a homogeneous fog box from corner LO to corner HI (ptc_set_medium) with extinction SIGMA_T per world unit, grey
// single-scattering albedo (default 0.9) and Henyey-Greenstein anisotropy G (default 0); --fog scene:SIGMA_T[:ALBEDO[:G]] takes the bounding box of the committed
// scene, its faces moved out by a thousandth of its diagonal, and prints it; path integrator only, and not with alpha or transmissive materials
// (--no-alpha, --no-transmission).  With --gpus device D's medium goes to every member.
// --aperture R: the thin lens (ptc_set_camera_lens) with aperture radius R in world units — depth of field, path integrator only.  --blades N: a regular polygon
// of 3..16 sides instead of the disk, --aperture-rotation T: its rotation in turns, [0, 1).  --focus D: the view depth of the plane of focus (default 1);
// --focus-pixel X,Y: focus on what that pixel's centre sees — the guides are traced once before the render and ptc_focus_distance_at_pixel is taken (a miss is
// an error).  The two exclude each other.  Bad values are reported before any device work.
// --denoise: first-hit guides + the variance-guided a-trous filter (ptc_frame_guides, ptc_denoise) after the render; every output is then the denoised
// image.  --denoise-iters N: N iterations instead of the default 4 (implies --denoise).  --guides PREFIX: PREFIX_albedo.pfm, PREFIX_normal.pfm and
// PREFIX_depth.pfm (the depth in all three channels) beside the image, for a denoiser outside the library.  With --gpus N device D denoises after the reduce.
// --denoise-sampled (implies --denoise): the filter takes its variance from the per-sample RGB covariance of the frame's own samples (ptc_set_sample_covariance,
// ptc_denoise_sampled) instead of the 7x7 window of the mean image.  With --adaptive the adaptive frame keeps the covariance; without, the frame runs as an
// adaptive frame with no decision step, whose image is the uniform frame's bit for bit.  One context, path integrator.
// --adaptive THRESH [--min-spp N] [--spp-step N] [--adaptive-radius R] [--counts out.pfm]: adaptive sampling (ptc_render_adaptive): --spp is then the
// per-pixel maximum, a pixel stops when the relative standard error of its mean luminance is <= THRESH and no pixel within R of it (default 1) is above; N
// samples before the first decision and between decisions (default 16 each).  --counts writes the per-pixel sample counts (all three channels).  One context
// only (not with --gpus), path integrator only.
// --gpus N: devices D..D+N-1 share the frame by 32x32-pixel tiles, one RCCL reduce brings it to device D (ptc_group_*).
// --raster16: the reference's Blinn-Phong pass lit from its G-buffer formats; --half writes the RGBA16F buffer (raw little-endian halves).
// --env: ordinary lat-long RGB environment map (PFM or Radiance .hdr, top row = up).  The reference's world is y-down (up = -y, CameraData.hpp:28) and
// ptc_set_env_latlong_rgb32f takes row 0 = +y, so the rows are flipped on the way in.  --sky: a built-in gradient sky with a sun, for
// assets that carry no emitters.
// --animation N --time T: the glTF scene is loaded with its skins and morph targets (host/gltf_anim.hpp) and posed at T seconds of its animation N before the commit.
// Without --cam-* a glTF scene is framed from its bounding box.  Camera models (ptc_set_camera_ex), path integrator:
// --camera N: camera node N of the --gltf asset (scene-traversal order), frame aspect W/H, at --time of --animation when given.  --cam-matrix m0,...,m15: a
// column-major camera-to-world matrix in glTF camera space (looks along -Z, +Y up), perspective with --fov.  --ortho XMAG,YMAG and --panorama switch the
// projection of whatever camera is in force: the asset's, the matrix's, or the look-at camera's (+Y up; --panorama takes its position with the rotation identity).
// A --panorama image (--out / --pfm, --png, --ppm) is written as --env reads a map, its rows reversed: `--panorama --pfm p.pfm`, then `--env p.pfm`, round-trips exactly.
// The scenes are the procedural stand-ins of BASELINE configs 1 and 2 (the reference's assets are stripped).
#include "gltf_anim.hpp"
#include "gltf_loader.hpp"
#include "image_io.hpp"
#include "pbr_pt.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <iostream>

namespace {
using V3 = std::array<float, 3>;

// --light SPEC -> ptc_light_params; throws with the expected form on anything else
ptc_light_params parseLight(const std::string& spec) {
  std::vector<std::vector<float>> f;
  std::string kind;
  size_t at = 0;
  for (int part = 0; at <= spec.size(); ++part) {
    const size_t e = std::min(spec.find(':', at), spec.size());
    const std::string tok = spec.substr(at, e - at);
    if (part == 0) kind = tok;
    else {
      f.emplace_back();
      size_t p = 0;
      while (p <= tok.size()) {
        const size_t c = std::min(tok.find(',', p), tok.size());
        char* end = nullptr;
        const std::string num = tok.substr(p, c - p);
        const float v = std::strtof(num.c_str(), &end);
        if (num.empty() || *end) throw std::runtime_error("--light " + spec + ": '" + num + "' is not a number");
        f.back().push_back(v);
        p = c + 1;
      }
    }
    at = e + 1;
  }
  auto is = [&](size_t i, size_t n) { return i < f.size() && f[i].size() == n; };
  ptc_light_params p;
  ptc_light_default_params(&p);
  const double deg = 3.14159265358979323846 / 180.0;
  if (kind == "point" && (f.size() == 2 || f.size() == 3) && is(0, 3) && is(1, 3) && (f.size() == 2 || is(2, 1))) {
    p.type = PTC_LIGHT_POINT;
    for (int k = 0; k < 3; ++k) { p.position[k] = f[0][(size_t)k]; p.intensity[k] = f[1][(size_t)k]; }
    if (f.size() == 3) p.range = f[2][0];
  } else if (kind == "spot" && (f.size() == 4 || f.size() == 5) && is(0, 3) && is(1, 3) && is(2, 3) && is(3, 2) && (f.size() == 4 || is(4, 1))) {
    p.type = PTC_LIGHT_SPOT;
    for (int k = 0; k < 3; ++k) { p.position[k] = f[0][(size_t)k]; p.direction[k] = f[1][(size_t)k]; p.intensity[k] = f[2][(size_t)k]; }
    p.cos_inner = (float)std::cos((double)f[3][0] * deg); p.cos_outer = (float)std::cos((double)f[3][1] * deg);
    if (!(f[3][0] >= 0.0f && f[3][0] < f[3][1] && f[3][1] <= 180.0f)) throw std::runtime_error("--light " + spec + ": 0 <= inner_deg < outer_deg <= 180");
    if (f.size() == 5) p.range = f[4][0];
  } else if (kind == "sun" && f.size() == 2 && is(0, 3) && is(1, 3)) {
    p.type = PTC_LIGHT_DIRECTIONAL;
    for (int k = 0; k < 3; ++k) { p.direction[k] = f[0][(size_t)k]; p.intensity[k] = f[1][(size_t)k]; }
  } else
    throw std::runtime_error("--light " + spec + ": point:x,y,z:r,g,b[:range] | spot:x,y,z:dx,dy,dz:r,g,b:inner_deg,outer_deg[:range] | sun:dx,dy,dz:r,g,b");
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(p.position[k]) || !std::isfinite(p.direction[k]) || !(p.intensity[k] >= 0.0f) || !std::isfinite(p.intensity[k])) throw std::runtime_error("--light " + spec + ": finite values, intensity >= 0");
  if (!(p.range >= 0.0f) || !std::isfinite(p.range)) throw std::runtime_error("--light " + spec + ": a finite range >= 0");
  if (p.type != PTC_LIGHT_POINT && p.direction[0] == 0.0f && p.direction[1] == 0.0f && p.direction[2] == 0.0f) throw std::runtime_error("--light " + spec + ": the direction is zero");
  if (p.type == PTC_LIGHT_SPOT && !(p.cos_inner > p.cos_outer)) throw std::runtime_error("--light " + spec + ": the cone angles are too close");
  return p;
}

pbr::MeshBuilder::Primitive quad(V3 a, V3 b, V3 c, V3 d, int material) {   // CCW seen from the front
  V3 e1{b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2{c[0] - a[0], c[1] - a[1], c[2] - a[2]};
  V3 n{e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
  float l = std::sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), le = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
  pbr::MeshBuilder::Primitive p;
  p.material = material;
  const V3 pts[4] = {a, b, c, d};
  const float uv[4][2] = {{0, 0}, {1, 0}, {1, 1}, {0, 1}};
  for (int i = 0; i < 4; ++i) {
    pbr::MeshVertex v;
    v.position = pts[i]; v.normal = {n[0] / l, n[1] / l, n[2] / l}; v.tangent = {e1[0] / le, e1[1] / le, e1[2] / le, 1.0f};
    v.texCoords = {uv[i][0], uv[i][1]};
    p.vertices.push_back(v);
  }
  p.indices = {0, 1, 2, 0, 2, 3};
  return p;
}

pbr::MeshBuilder::Primitive uvSphere(int nu, int nv, float radius, int material) {
  pbr::MeshBuilder::Primitive p;
  p.material = material;
  const double pi = 3.14159265358979323846;
  for (int j = 0; j <= nv; ++j)
    for (int i = 0; i <= nu; ++i) {
      const double th = pi * j / nv, ph = 2.0 * pi * i / nu;
      const float nx = (float)(std::sin(th) * std::cos(ph)), ny = (float)std::cos(th), nz = (float)(std::sin(th) * std::sin(ph));
      pbr::MeshVertex v;
      v.position = {radius * nx, radius * ny, radius * nz}; v.normal = {nx, ny, nz};
      v.tangent = {(float)-std::sin(ph), 0.0f, (float)std::cos(ph), 1.0f}; v.texCoords = {(float)i / nu, (float)j / nv};
      p.vertices.push_back(v);
    }
  for (int j = 0; j < nv; ++j)
    for (int i = 0; i < nu; ++i) {
      const std::uint32_t a = j * (nu + 1) + i, b = a + 1, c = a + nu + 1, d = c + 1;
      if (j != 0) p.indices.insert(p.indices.end(), {a, b, c});
      if (j != nv - 1) p.indices.insert(p.indices.end(), {b, d, c});
    }
  return p;
}

void buildCornell(pbr::PathTraceRenderSystem& rs) {
  rs.beginScene();
  const int white = rs.addMaterial({{0.73f, 0.73f, 0.73f, 1}, 0, 1, {0, 0, 0}});
  const int red = rs.addMaterial({{0.65f, 0.05f, 0.05f, 1}, 0, 1, {0, 0, 0}});
  const int green = rs.addMaterial({{0.12f, 0.45f, 0.15f, 1}, 0, 1, {0, 0, 0}});
  const int light = rs.addMaterial({{0, 0, 0, 1}, 0, 1, {15, 15, 15}});
  pbr::MeshBuilder mb;
  mb.addPrimitive(quad({-1, -1, 1}, {1, -1, 1}, {1, -1, -1}, {-1, -1, -1}, white));
  mb.addPrimitive(quad({-1, 1, -1}, {1, 1, -1}, {1, 1, 1}, {-1, 1, 1}, white));
  mb.addPrimitive(quad({-1, -1, -1}, {1, -1, -1}, {1, 1, -1}, {-1, 1, -1}, white));
  mb.addPrimitive(quad({-1, -1, 1}, {-1, -1, -1}, {-1, 1, -1}, {-1, 1, 1}, red));
  mb.addPrimitive(quad({1, -1, -1}, {1, -1, 1}, {1, 1, 1}, {1, 1, -1}, green));
  mb.addPrimitive(quad({-0.25f, 0.998f, -0.25f}, {0.25f, 0.998f, -0.25f}, {0.25f, 0.998f, 0.25f}, {-0.25f, 0.998f, 0.25f}, light));
  for (int m : rs.addMesh(mb.build())) rs.addInstance(m, pbr::Transform{});
  // double arithmetic then one rounding to float, like the Python scene generator (pbr_amd/scenes.py)
  const double deg = 3.14159265358979323846 / 180.0;
  const double d = 1.0 / std::tan(20.0 * deg);
  rs.setCamera({0, 0, (float)(1.0 + d)}, {0, 0, 0}, (float)(40.0 * deg), 1.0f);
  rs.commitScene();
}

void buildSphere(pbr::PathTraceRenderSystem& rs, float aspect) {
  rs.beginScene();
  const int gold = rs.addMaterial({{0.9f, 0.6f, 0.2f, 1}, 1.0f, 0.3f, {0, 0, 0}});
  const int ground = rs.addMaterial({{0.6f, 0.6f, 0.6f, 1}, 0, 1, {0, 0, 0}});
  const int light = rs.addMaterial({{0, 0, 0, 1}, 0, 1, {12, 11, 10}});
  pbr::MeshBuilder mb;
  mb.addPrimitive(uvSphere(100, 51, 1.0f, gold));
  const int sphere = rs.addMesh(mb.build())[0];
  pbr::MeshBuilder rest;
  rest.addPrimitive(quad({-10, -1, 10}, {10, -1, 10}, {10, -1, -10}, {-10, -1, -10}, ground));
  rest.addPrimitive(quad({-2, 4, -2}, {2, 4, -2}, {2, 4, 2}, {-2, 4, 2}, light));
  const double a = 30.0 * (3.14159265358979323846 / 180.0);
  rs.addInstance(sphere, pbr::Transform{{0, -0.2f, 0}, {(float)std::cos(a / 2), 0, (float)std::sin(a / 2), 0}, {1, 0.8f, 1}});
  for (int m : rs.addMesh(rest.build())) rs.addInstance(m, pbr::Transform{});
  rs.setCamera({0, 1.2f, 4.5f}, {0, -0.1f, 0}, (float)(45.0 * (3.14159265358979323846 / 180.0)), aspect);
  rs.commitScene();
}
}  // namespace

int main(int argc, char** argv) {
  std::string scene = "cornell", out = "out.pfm", ppm, png, gltf, envPath;
  bool sky = false;
  int filter = PTC_FILTER_NEAREST;          // what the reference's default-constructed samplers do
  int bvh = -1;                             // -1: the context's default (SAH, or PTC_BVH in the environment)
  int deviceBvh = -1;                       // --device-bvh: the tree a build on the device makes; -1: the context's default (LBVH, or PTC_DEVICE_BVH)
  float camPos[3] = {0, 0, 0}, camTarget[3] = {0, 0, -1}, fovDeg = 60.0f;
  bool haveCam = false;
  float viewerFov = 0.0f;                    // --viewer-camera: the reference's fov in radians, passed on without a degree round trip
  int w = 256, h = 256, spp = 64, bounces = 8, device = 0, gpus = 0 /* 0: one plain context; N >= 1: a device group of N */, integrator = PTC_INTEGRATOR_PATH;
  std::string halfPath, guidesPrefix;
  bool denoise = false, denoiseSampled = false;
  int denoiseIters = -1;                     // -1: the library's default
  std::uint64_t seed = 1;
  bool adaptive = false;
  ptc_adaptive_params ap = pbr::PathTraceRenderSystem::adaptiveDefaults();
  std::string countsPath;
  ptc_lens_params lens = pbr::PathTraceRenderSystem::lensDefaults();      // --aperture / --blades / --aperture-rotation / --focus
  bool haveFocus = false, haveFocusPixel = false, haveLensShape = false;
  int cameraIndex = -1;                      // --camera N: the asset's camera node N
  bool haveOrtho = false, panorama = false, haveCamMatrix = false;      // --ortho XMAG,YMAG / --panorama / --cam-matrix
  float orthoMag[2] = {1.0f, 1.0f}, camMatrix[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  int focusX = 0, focusY = 0;
  int animation = -1;                        // --animation: pose the glTF scene along this animation ...
  double animTime = 0.0;                     // ... at --time seconds, before the commit
  std::vector<std::string> lightSpecs;       // --light, in order
  std::vector<ptc_light_params> lights;
  bool noGltfLights = false;
  bool noAlpha = false;                      // --no-alpha: ignore the asset's alpha modes
  bool noTransmission = false;               // --no-transmission: ignore the asset's transmission extensions
  bool noEmissiveTextures = false;           // --no-emissive-textures: ignore the asset's emissiveTexture
  bool glassShadows = false;                 // --glass-shadows: transparent shadows through thin panes
  std::string fogSpec;                       // --fog: the medium
  ptc_medium_params fog{};
  ptc_display_params disp = pbr::PathTraceRenderSystem::displayDefaults();      // --exposure / --auto-exposure / --key / --tonemap / --srgb
  bool useDisplay = false, haveKey = false;
  double exposureEv = 0.0;
  int probeGrid[3] = {0, 0, 0};              // --probe-grid
  std::string probesFile, probesOut;         // --probes, --probes-out
  std::string lmSpec, lmOut, lmAlpha;        // --lightmap, --lightmap-out, --lightmap-alpha
  int lmInstance = -1, lmW = 0, lmH = 0, lmDilate = 2;
  float lmBackface = 0.1f;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    auto next = [&]() -> const char* { if (i + 1 >= argc) { std::cerr << "missing value for " << a << "\n"; std::exit(2); } return argv[++i]; };
    if (a == "--scene") scene = next(); else if (a == "--width") w = std::atoi(next()); else if (a == "--height") h = std::atoi(next());
    else if (a == "--spp") spp = std::atoi(next()); else if (a == "--seed") seed = std::strtoull(next(), nullptr, 10);
    else if (a == "--bounces") bounces = std::atoi(next()); else if (a == "--device") device = std::atoi(next());
    else if (a == "--gpus") gpus = std::atoi(next()); else if (a == "--half") halfPath = next(); else if (a == "--raster16") integrator = PTC_INTEGRATOR_RASTER_GBUFFER16;
    else if (a == "--gltf") gltf = next();
    else if (a == "--animation") animation = std::atoi(next()); else if (a == "--time") animTime = std::atof(next());
    else if (a == "--denoise") denoise = true; else if (a == "--denoise-iters") { denoiseIters = std::atoi(next()); denoise = true; } else if (a == "--guides") guidesPrefix = next();
    else if (a == "--denoise-sampled") { denoiseSampled = true; denoise = true; }
    else if (a == "--adaptive") { ap.threshold = (float)std::atof(next()); adaptive = true; } else if (a == "--min-spp") ap.min_samples = std::atoi(next());
    else if (a == "--spp-step") ap.step_samples = std::atoi(next()); else if (a == "--adaptive-radius") ap.radius = std::atoi(next()); else if (a == "--counts") countsPath = next();
    else if (a == "--aperture") lens.aperture_radius = (float)std::atof(next());
    else if (a == "--blades") { lens.blades = std::atoi(next()); haveLensShape = true; } else if (a == "--aperture-rotation") { lens.rotation = (float)std::atof(next()); haveLensShape = true; }
    else if (a == "--focus") { lens.focus_distance = (float)std::atof(next()); haveFocus = true; }
    else if (a == "--focus-pixel") { if (std::sscanf(next(), "%d,%d", &focusX, &focusY) != 2) { std::cerr << "--focus-pixel X,Y\n"; return 2; } haveFocusPixel = true; }
    else if (a == "--camera") cameraIndex = std::atoi(next()); else if (a == "--panorama") panorama = true;
    else if (a == "--ortho") { if (std::sscanf(next(), "%f,%f", &orthoMag[0], &orthoMag[1]) != 2) { std::cerr << "--ortho XMAG,YMAG\n"; return 2; } haveOrtho = true; }
    else if (a == "--cam-matrix") {
      const char* s = next(); char* end = nullptr; int n = 0;
      for (; n < 16; ++n) { camMatrix[n] = std::strtof(s, &end); if (end == s) break; s = *end == ',' ? end + 1 : end; }
      if (n != 16 || *end != '\0') { std::cerr << "--cam-matrix m0,...,m15 (column-major camera-to-world)\n"; return 2; }
      haveCamMatrix = true;
    }
    else if (a == "--light") lightSpecs.push_back(next()); else if (a == "--no-gltf-lights") noGltfLights = true; else if (a == "--no-alpha") noAlpha = true; else if (a == "--no-transmission") noTransmission = true; else if (a == "--no-emissive-textures") noEmissiveTextures = true; else if (a == "--glass-shadows") glassShadows = true;
    else if (a == "--fog") fogSpec = next();
    else if (a == "--exposure") { exposureEv = std::atof(next()); useDisplay = true; } else if (a == "--auto-exposure") { disp.auto_exposure = 1; useDisplay = true; }
    else if (a == "--key") { disp.key = (float)std::atof(next()); haveKey = true; } else if (a == "--srgb") { disp.oetf = PTC_OETF_SRGB; useDisplay = true; }
    else if (a == "--tonemap") {
      const std::string f = next();
      if (f == "aces") disp.tonemap = PTC_TONEMAP_ACES; else if (f == "neutral") disp.tonemap = PTC_TONEMAP_PBR_NEUTRAL; else if (f == "reinhard") disp.tonemap = PTC_TONEMAP_REINHARD;
      else if (f == "clamp") disp.tonemap = PTC_TONEMAP_CLAMP; else { std::cerr << "--tonemap aces|neutral|reinhard|clamp\n"; return 2; }
      useDisplay = true;
    }
    else if (a == "--probe-grid") { if (std::sscanf(next(), "%d,%d,%d", &probeGrid[0], &probeGrid[1], &probeGrid[2]) != 3) { std::cerr << "--probe-grid NX,NY,NZ\n"; return 2; } }
    else if (a == "--probes") probesFile = next(); else if (a == "--probes-out") probesOut = next();
    else if (a == "--lightmap") lmSpec = next(); else if (a == "--lightmap-out") lmOut = next(); else if (a == "--lightmap-alpha") lmAlpha = next();
    else if (a == "--lightmap-dilate") lmDilate = std::atoi(next()); else if (a == "--lightmap-backface") lmBackface = (float)std::atof(next());
    else if (a == "--env") envPath = next(); else if (a == "--sky") sky = true;
    else if (a == "--filter") { const std::string f = next(); if (f == "linear") filter = PTC_FILTER_LINEAR; else if (f == "nearest") filter = PTC_FILTER_NEAREST; else { std::cerr << "--filter nearest|linear\n"; return 2; } }
    else if (a == "--cam-pos") { for (float& v : camPos) v = (float)std::atof(next()); haveCam = true; }
    else if (a == "--viewer-camera") {     // the reference viewer's start-up view: CameraController.hpp:25-40 (position 0, looking down -z, fovY pi/2, aspect W/H)
      const pbr::ViewerCamera vc;
      const auto tg = vc.target();
      for (int k = 0; k < 3; ++k) { camPos[k] = vc.position[(std::size_t)k]; camTarget[k] = tg[(std::size_t)k]; }
      fovDeg = vc.fov * 180.0f / 3.14159265358979323846f; viewerFov = vc.fov; haveCam = true;
    }
    else if (a == "--cam-target") { for (float& v : camTarget) v = (float)std::atof(next()); }
    else if (a == "--fov") fovDeg = (float)std::atof(next());
    else if (a == "--bvh") { const std::string f = next(); if (f == "lbvh") bvh = PTC_BVH_LBVH; else if (f == "sah") bvh = PTC_BVH_SAH; else { std::cerr << "--bvh sah|lbvh\n"; return 2; } }
    else if (a == "--device-bvh") { const std::string f = next(); if (f == "lbvh") deviceBvh = PTC_BVH_LBVH; else if (f == "sah") deviceBvh = PTC_BVH_SAH; else { std::cerr << "--device-bvh sah|lbvh\n"; return 2; } }
    else if (a == "--out" || a == "--pfm") out = next(); else if (a == "--png") png = next(); else if (a == "--ppm") ppm = next(); else if (a == "--raster") integrator = PTC_INTEGRATOR_RASTER_COMPAT;
    else { std::cerr << "unknown argument " << a << "\n"; return 2; }
  }
  try {
    if (gpus < 0) throw std::runtime_error("--gpus must be >= 1");
    if (adaptive && (gpus != 0 || integrator != PTC_INTEGRATOR_PATH)) throw std::runtime_error("--adaptive renders on one context with the path integrator (not with --gpus / --raster)");
    if (denoiseSampled && (gpus != 0 || integrator != PTC_INTEGRATOR_PATH)) throw std::runtime_error("--denoise-sampled renders on one context with the path integrator (not with --gpus / --raster)");
    if (!adaptive && !countsPath.empty()) throw std::runtime_error("--counts needs --adaptive");
    {   // the lens: everything that can be refused is refused here, before a device is touched
      if (haveFocus && haveFocusPixel) throw std::runtime_error("--focus and --focus-pixel exclude each other");
      const bool anyLens = lens.aperture_radius != 0.0f || haveFocus || haveFocusPixel || haveLensShape;
      if (anyLens && integrator != PTC_INTEGRATOR_PATH) throw std::runtime_error("--aperture / --focus* / --blades apply to the path integrator (not with --raster / --raster16)");
      if (!(lens.aperture_radius >= 0.0f) || !std::isfinite(lens.aperture_radius)) throw std::runtime_error("--aperture R: a finite radius >= 0");
      if (!(lens.focus_distance > 0.0f) || !std::isfinite(lens.focus_distance)) throw std::runtime_error("--focus D: a finite distance > 0");
      if (lens.blades != 0 && (lens.blades < 3 || lens.blades > 16)) throw std::runtime_error("--blades N: 0 (disk) or 3..16");
      if (!(lens.rotation >= 0.0f && lens.rotation < 1.0f)) throw std::runtime_error("--aperture-rotation T: turns in [0, 1)");
      if (haveFocusPixel && (focusX < 0 || focusY < 0 || focusX >= w || focusY >= h)) throw std::runtime_error("--focus-pixel X,Y: a pixel of the image");
    }
    const bool cameraEx = cameraIndex >= 0 || haveOrtho || panorama || haveCamMatrix;
    {   // the camera models: everything that can be refused is refused here, before a device is touched
      if (cameraIndex >= 0 && gltf.empty()) throw std::runtime_error("--camera N takes camera N of a --gltf scene");
      if (cameraIndex >= 0 && haveCamMatrix) throw std::runtime_error("--camera and --cam-matrix exclude each other");
      if (haveOrtho && panorama) throw std::runtime_error("--ortho and --panorama exclude each other");
      if (haveOrtho && !(orthoMag[0] > 0.0f && orthoMag[1] > 0.0f && std::isfinite(orthoMag[0]) && std::isfinite(orthoMag[1]))) throw std::runtime_error("--ortho XMAG,YMAG: finite half extents > 0");
      if ((haveOrtho || panorama) && integrator != PTC_INTEGRATOR_PATH) throw std::runtime_error("--ortho / --panorama apply to the path integrator (not with --raster / --raster16)");
      if ((haveOrtho || panorama) && (haveFocusPixel || lens.aperture_radius != 0.0f)) throw std::runtime_error("--ortho / --panorama have no lens (not with --aperture / --focus-pixel)");
      if (cameraEx && gltf.empty() && !haveCamMatrix) throw std::runtime_error("--ortho / --panorama on a built-in scene need --cam-matrix");
      if (cameraEx && gltf.empty() && gpus != 0) throw std::runtime_error("a camera model on a built-in scene renders on one context (not with --gpus)");
    }
    // the extended camera (ptc_set_camera_ex) of --camera / --cam-matrix / --ortho / --panorama; needs no commit
    auto applyCameraEx = [&](pbr::PathTraceRenderSystem& rs) {
      if (!cameraEx) return;
      ptc_camera_params p;
      ptc_camera_default_params(&p);
      p.yfov = viewerFov > 0.0f ? viewerFov : fovDeg * 3.14159265f / 180.0f; p.aspect = (float)w / h;
      if (cameraIndex >= 0) {      // the asset's camera, at --time of --animation when given
        pbr::gltf::Asset asset(gltf);
        if (cameraIndex >= asset.cameras()) throw std::runtime_error("--camera: the asset has " + std::to_string(asset.cameras()) + " camera(s)");
        if (asset.camera(cameraIndex, animation, animTime, (float)w / h, &p) < 0) throw std::runtime_error("--camera: the asset's camera could not be read");
      } else if (haveCamMatrix) std::memcpy(p.camera_to_world, camMatrix, sizeof camMatrix);
      else {      // the look-at camera in force: +Y up; a panorama takes its position alone
        float Z[3] = {camPos[0] - camTarget[0], camPos[1] - camTarget[1], camPos[2] - camTarget[2]};
        const float lz = std::sqrt(Z[0] * Z[0] + Z[1] * Z[1] + Z[2] * Z[2]);
        for (float& v : Z) v /= lz;
        float X[3] = {Z[2], 0.0f, -Z[0]};      // (0, 1, 0) x Z
        const float lx = std::sqrt(X[0] * X[0] + X[2] * X[2]);
        if (!(lz > 0.0f) || !(lx > 0.0f)) throw std::runtime_error("--ortho: the camera looks straight up or down; give --cam-matrix");
        for (float& v : X) v /= lx;
        const float Y[3] = {Z[1] * X[2] - Z[2] * X[1], Z[2] * X[0] - Z[0] * X[2], Z[0] * X[1] - Z[1] * X[0]};
        for (int k = 0; k < 3; ++k) { p.camera_to_world[k] = X[k]; p.camera_to_world[4 + k] = Y[k]; p.camera_to_world[8 + k] = Z[k]; p.camera_to_world[12 + k] = camPos[k]; }
      }
      if (haveOrtho) { p.projection = PTC_PROJ_ORTHOGRAPHIC; p.xmag = orthoMag[0]; p.ymag = orthoMag[1]; }
      if (panorama) {
        p.projection = PTC_PROJ_EQUIRECT;
        if (cameraIndex < 0 && !haveCamMatrix) for (int k = 0; k < 12; ++k) p.camera_to_world[k] = (k % 5 == 0) ? 1.0f : 0.0f;      // the rotation identity
      }
      if (ptc_set_camera_ex(rs.handle(), &p) < 0) throw std::runtime_error(ptc_last_error(rs.handle()));
    };
    {   // the display transform
      disp.gain = (float)std::exp2(exposureEv);
      if (!std::isfinite(exposureEv) || !(disp.gain > 0.0f) || !std::isfinite(disp.gain)) throw std::runtime_error("--exposure EV: 2^EV must be a finite float > 0");
      if (haveKey && !disp.auto_exposure) throw std::runtime_error("--key K sets the target of --auto-exposure");
      if (!(disp.key > 0.0f) || !std::isfinite(disp.key)) throw std::runtime_error("--key K: a finite value > 0");
    }
    const bool haveGrid = probeGrid[0] || probeGrid[1] || probeGrid[2], bakeProbes = haveGrid || !probesFile.empty() || !probesOut.empty();
    std::vector<float> probePos;
    if (bakeProbes) {      // light probes: refused here, before a device is touched
      if (probesOut.empty()) throw std::runtime_error("--probe-grid / --probes need --probes-out sh.pfm");
      if (haveGrid == !probesFile.empty()) throw std::runtime_error("--probes-out needs either --probe-grid NX,NY,NZ or --probes FILE");
      if (gpus != 0 || integrator != PTC_INTEGRATOR_PATH || adaptive || denoise) throw std::runtime_error("probes are baked on one context with the path integrator (not with --gpus / --raster / --adaptive / --denoise)");
      if (haveGrid && (probeGrid[0] < 1 || probeGrid[1] < 1 || probeGrid[2] < 1 || (long long)probeGrid[0] * probeGrid[1] * probeGrid[2] > (1ll << 26)))
        throw std::runtime_error("--probe-grid NX,NY,NZ: three counts >= 1, at most 2^26 probes");
      if (spp < 1) throw std::runtime_error("--spp N: at least one sample per probe");
      if (!probesFile.empty()) {
        std::ifstream f(probesFile);
        if (!f) throw std::runtime_error("--probes: cannot read " + probesFile);
        float x, y, z;
        while (f >> x >> y >> z) { probePos.push_back(x); probePos.push_back(y); probePos.push_back(z); }
        if (!f.eof() || probePos.empty()) throw std::runtime_error("--probes FILE: lines of `x y z`, at least one");
      }
    }
    const bool bakeLightmap = !lmSpec.empty() || !lmOut.empty() || !lmAlpha.empty();
    if (bakeLightmap) {      // a lightmap: refused here, before a device is touched
      if (lmSpec.empty() || lmOut.empty()) throw std::runtime_error("--lightmap INSTANCE:WxH needs --lightmap-out lm.pfm, and the other way round");
      if (std::sscanf(lmSpec.c_str(), "%d:%dx%d", &lmInstance, &lmW, &lmH) != 3 || lmInstance < 0 || lmW < 1 || lmW > 8192 || lmH < 1 || lmH > 8192)
        throw std::runtime_error("--lightmap INSTANCE:WxH: an instance index >= 0 and an atlas of 1..8192 texels a side");
      if (bakeProbes || gpus != 0 || integrator != PTC_INTEGRATOR_PATH || adaptive || denoise) throw std::runtime_error("a lightmap is baked on one context with the path integrator (not with --gpus / --raster / --adaptive / --denoise / probes)");
      if (lmDilate < 0 || lmDilate > 64) throw std::runtime_error("--lightmap-dilate N: 0..64 iterations");
      if (!(lmBackface >= 0.0f) || !std::isfinite(lmBackface)) throw std::runtime_error("--lightmap-backface F: a finite fraction >= 0");
      if (spp < 1) throw std::runtime_error("--spp N: at least one sample per texel");
    }
    for (const std::string& sp : lightSpecs) lights.push_back(parseLight(sp));
    if (!lights.empty() && integrator != PTC_INTEGRATOR_PATH) throw std::runtime_error("--light applies to the path integrator (not with --raster / --raster16)");
    if (noGltfLights && gltf.empty()) throw std::runtime_error("--no-gltf-lights drops the lights of a --gltf scene");
    if (glassShadows && integrator != PTC_INTEGRATOR_PATH) throw std::runtime_error("--glass-shadows applies to the path integrator (not with --raster / --raster16)");
    bool fogSceneBox = false;                  // --fog scene:...: the box is the committed scene's bounding box
    if (!fogSpec.empty()) {
      float al = 0.9f, g = 0.0f;
      int got;
      if (fogSpec.compare(0, 6, "scene:") == 0) { fogSceneBox = true; got = 6 + std::sscanf(fogSpec.c_str() + 6, "%f:%f:%f", &fog.sigma_t, &al, &g); }
      else got = std::sscanf(fogSpec.c_str(), "%f,%f,%f:%f,%f,%f:%f:%f:%f", &fog.box_lo[0], &fog.box_lo[1], &fog.box_lo[2], &fog.box_hi[0], &fog.box_hi[1], &fog.box_hi[2], &fog.sigma_t, &al, &g);
      if (got < 7) throw std::runtime_error("--fog x,y,z:x,y,z:sigma_t[:albedo[:g]] or --fog scene:sigma_t[:albedo[:g]]");
      if (integrator != PTC_INTEGRATOR_PATH) throw std::runtime_error("--fog applies to the path integrator (not with --raster / --raster16)");
      fog.albedo[0] = fog.albedo[1] = fog.albedo[2] = al; fog.g = g;
    }
    // --fog scene:...: the bounding box of the committed scene's vertices (--probe-grid's box), each face moved out by a thousandth of the diagonal so that the
    // scene's outer surfaces lie inside the fog and a flat scene still has a box
    auto sceneFogBox = [&](pbr::PathTraceRenderSystem& rs) {
      std::uint32_t nv = 0, nt = 0;
      if (ptc_debug_get_flat_scene(rs.handle(), &nv, &nt, nullptr, nullptr, nullptr) < 0 || nv == 0) throw std::runtime_error("--fog scene: the scene has no geometry");
      std::vector<ptc_vertex> verts(nv);
      if (ptc_debug_get_flat_scene(rs.handle(), &nv, &nt, verts.data(), nullptr, nullptr) < 0) throw std::runtime_error(ptc_last_error(rs.handle()));
      float lo[3] = {verts[0].position[0], verts[0].position[1], verts[0].position[2]}, hi[3] = {lo[0], lo[1], lo[2]};
      for (const ptc_vertex& v : verts)
        for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], v.position[k]); hi[k] = std::max(hi[k], v.position[k]); }
      const float pad = 1e-3f * std::max(1e-3f, std::sqrt((hi[0] - lo[0]) * (hi[0] - lo[0]) + (hi[1] - lo[1]) * (hi[1] - lo[1]) + (hi[2] - lo[2]) * (hi[2] - lo[2])));
      for (int k = 0; k < 3; ++k) { fog.box_lo[k] = lo[k] - pad; fog.box_hi[k] = hi[k] + pad; }
      std::printf("{\"fog_box\": [[%.9g, %.9g, %.9g], [%.9g, %.9g, %.9g]], \"sigma_t\": %.9g}\n", (double)fog.box_lo[0], (double)fog.box_lo[1], (double)fog.box_lo[2], (double)fog.box_hi[0],
                  (double)fog.box_hi[1], (double)fog.box_hi[2], (double)fog.sigma_t);
    };
    // after the scene: the punctual lights (they need no commit) — the asset's own unless dropped, then the command line's — and how shadow rays see thin glass
    auto applyLights = [&](pbr::PathTraceRenderSystem& rs) {
      rs.setGlassShadows(glassShadows);
      if (fogSceneBox) sceneFogBox(rs);
      if (!fogSpec.empty()) rs.setMedium(fog);
      if (noGltfLights && ptc_clear_lights(rs.handle()) < 0) throw std::runtime_error(ptc_last_error(rs.handle()));
      for (const ptc_light_params& l : lights)
        if (ptc_add_light(rs.handle(), &l) < 0) throw std::runtime_error(ptc_last_error(rs.handle()));
    };
    // after the commit: the lens, focused on a pixel if asked (one guide pass of a one-sample frame; the render that follows begins its own frame)
    auto applyLens = [&](pbr::PathTraceRenderSystem& rs) {
      if (haveFocusPixel) {
        if (ptc_frame_begin(rs.handle(), w, h, 1, seed, bounces, PTC_INTEGRATOR_PATH, 0, 1) < 0) throw std::runtime_error(ptc_last_error(rs.handle()));
        rs.frameGuides();
        lens.focus_distance = rs.focusDistanceAtPixel(focusX, focusY);
        if (!(lens.focus_distance > 0.0f)) throw std::runtime_error("--focus-pixel: the pixel sees nothing to focus on");
        std::printf("{\"focus_pixel\": [%d, %d], \"focus_distance\": %.9g}\n", focusX, focusY, (double)lens.focus_distance);
      }
      rs.setCameraLens(lens);
    };
    if (gltf.empty() && animation >= 0) throw std::runtime_error("--animation poses a --gltf scene");
    if (gltf.empty() && (!envPath.empty() || sky)) throw std::runtime_error("--env / --sky light a --gltf scene; the built-in scenes carry their own lights");
    auto buildScene = [&](pbr::PathTraceRenderSystem& rs) {
    if (deviceBvh >= 0) rs.setDeviceBuilder(deviceBvh);
    if (!gltf.empty()) {
      pbr::gltf::emissive_textures_enabled() = !noEmissiveTextures;
      pbr::gltf::FlatScene fs;
      if (animation >= 0) {      // the asset as a handle: targets, skins, and the pose of the animation at --time; the box that frames it is the bind pose's
        pbr::gltf::Asset asset(gltf);
        if (animation >= asset.animations()) throw std::runtime_error("--animation: the asset has " + std::to_string(asset.animations()) + " animation(s)");
        rs.beginScene();
        float box[6];
        if (asset.load_into(rs.handle(), -1, true, box) < 0 || asset.pose(rs.handle(), animation, animTime) < 0) throw std::runtime_error(ptc_last_error(rs.handle()));
        for (int k = 0; k < 3; ++k) { fs.bbox_lo[k] = box[k]; fs.bbox_hi[k] = box[3 + k]; }
      } else {
        fs = pbr::gltf::load(gltf);
        rs.beginScene();
        if (pbr::gltf::upload(rs.handle(), fs) < 0) throw std::runtime_error(ptc_last_error(rs.handle()));
      }
      if (noTransmission) {      // every material back to transmission 0
        int nMats = 0;
        if (ptc_debug_get_description(rs.handle(), &nMats, nullptr) < 0) throw std::runtime_error(ptc_last_error(rs.handle()));
        ptc_transmission_params off;
        ptc_transmission_default_params(&off);
        for (int m = 0; m < nMats; ++m) (void)ptc_set_material_transmission(rs.handle(), m, &off);
      }
      if (noAlpha) {      // every material back to OPAQUE (an emissive one is refused: it is opaque anyway)
        int nMats = 0;
        if (ptc_debug_get_description(rs.handle(), &nMats, nullptr) < 0) throw std::runtime_error(ptc_last_error(rs.handle()));
        for (int m = 0; m < nMats; ++m) (void)ptc_set_material_alpha(rs.handle(), m, PTC_ALPHA_OPAQUE, 0.5f);
      }
      if (ptc_set_texture_filter(rs.handle(), filter) < 0) throw std::runtime_error(ptc_last_error(rs.handle()));
      if (bvh >= 0) rs.setBvhBuilder(bvh);
      if (!haveCam) {   // frame the bounding box from +z
        const float cx = 0.5f * (fs.bbox_lo[0] + fs.bbox_hi[0]), cy = 0.5f * (fs.bbox_lo[1] + fs.bbox_hi[1]), cz = 0.5f * (fs.bbox_lo[2] + fs.bbox_hi[2]);
        const float r = 0.5f * std::sqrt((fs.bbox_hi[0] - fs.bbox_lo[0]) * (fs.bbox_hi[0] - fs.bbox_lo[0]) + (fs.bbox_hi[1] - fs.bbox_lo[1]) * (fs.bbox_hi[1] - fs.bbox_lo[1]) +
                                         (fs.bbox_hi[2] - fs.bbox_lo[2]) * (fs.bbox_hi[2] - fs.bbox_lo[2]));
        camTarget[0] = cx; camTarget[1] = cy; camTarget[2] = cz;
        camPos[0] = cx; camPos[1] = cy; camPos[2] = cz + r / std::tan(0.5f * fovDeg * 3.14159265f / 180.0f) + r;
        haveCam = true;
      }
      rs.setCamera({camPos[0], camPos[1], camPos[2]}, {camTarget[0], camTarget[1], camTarget[2]}, viewerFov > 0.0f ? viewerFov : fovDeg * 3.14159265f / 180.0f, (float)w / h);
      if (!envPath.empty()) {
        int ew = 0, eh = 0;
        const bool isHdr = envPath.size() > 4 && (envPath.compare(envPath.size() - 4, 4, ".hdr") == 0 || envPath.compare(envPath.size() - 4, 4, ".pic") == 0);
        std::vector<float> env = isHdr ? pbr::image::read_hdr(envPath, ew, eh) : pbr::image::read_pfm(envPath, ew, eh);     // Radiance RGBE or PFM, row 0 = top either way
        for (int y = 0; y < eh / 2; ++y)                 // top row = up = -y = the map's last row
          for (int k = 0; k < ew * 3; ++k) std::swap(env[(std::size_t)y * ew * 3 + k], env[(std::size_t)(eh - 1 - y) * ew * 3 + k]);
        if (ptc_set_env_latlong_rgb32f(rs.handle(), env.data(), ew, eh) < 0) throw std::runtime_error(ptc_last_error(rs.handle()));
      } else if (sky) {                                  // 256 x 128 gradient + sun; row 0 is the map's +y pole = down
        const int ew = 256, eh = 128;
        std::vector<float> env((std::size_t)ew * eh * 3);
        for (int y = 0; y < eh; ++y)
          for (int x = 0; x < ew; ++x) {
            const float t = 1.0f - (float)y / (eh - 1);     // 0 at the zenith (-y), 1 at the nadir
            float r = 0.9f - 0.55f * (1.0f - t), g = 0.95f - 0.35f * (1.0f - t), b = 1.0f;
            if (t > 0.5f) { r = g = b = 0.25f; }                       // ground half
            const float dx = (float)(x - ew / 4) / ew * 2.0f, dy = (float)(y - 3 * eh / 4) / eh;
            if (dx * dx + dy * dy < 0.0004f) { r = 60.0f; g = 55.0f; b = 45.0f; }
            float* o = &env[((std::size_t)y * ew + x) * 3];
            o[0] = r; o[1] = g; o[2] = b;
          }
        if (ptc_set_env_latlong_rgb32f(rs.handle(), env.data(), ew, eh) < 0) throw std::runtime_error(ptc_last_error(rs.handle()));
      }
      applyCameraEx(rs);
      rs.commitScene();
    } else if (scene == "cornell") { buildCornell(rs); applyCameraEx(rs); } else if (scene == "sphere") { buildSphere(rs, (float)w / h); applyCameraEx(rs); } else throw std::runtime_error("unknown scene " + scene);
    };
    std::unique_ptr<pbr::PathTraceRenderSystem> single;
    std::unique_ptr<pbr::DeviceGroup> group;
    std::vector<float> img;
    if (gpus == 0) {
      single.reset(new pbr::PathTraceRenderSystem(device));
      buildScene(*single);
      applyLights(*single);
      if (bakeProbes) {
        pbr::PathTraceRenderSystem& rs = *single;
        if (haveGrid) {      // the cell centres of the committed scene's bounding box
          std::uint32_t nv = 0, nt = 0;
          if (ptc_debug_get_flat_scene(rs.handle(), &nv, &nt, nullptr, nullptr, nullptr) < 0 || nv == 0) throw std::runtime_error("--probe-grid: the scene has no geometry");
          std::vector<ptc_vertex> verts(nv);
          if (ptc_debug_get_flat_scene(rs.handle(), &nv, &nt, verts.data(), nullptr, nullptr) < 0) throw std::runtime_error(ptc_last_error(rs.handle()));
          float lo[3] = {verts[0].position[0], verts[0].position[1], verts[0].position[2]}, hi[3] = {lo[0], lo[1], lo[2]}, cell[3];
          for (const ptc_vertex& v : verts)
            for (int k = 0; k < 3; ++k) { lo[k] = std::min(lo[k], v.position[k]); hi[k] = std::max(hi[k], v.position[k]); }
          for (int k = 0; k < 3; ++k) cell[k] = (hi[k] - lo[k]) / (float)probeGrid[k];
          for (int z = 0; z < probeGrid[2]; ++z)
            for (int y = 0; y < probeGrid[1]; ++y)
              for (int x = 0; x < probeGrid[0]; ++x) {
                probePos.push_back(lo[0] + ((float)x + 0.5f) * cell[0]); probePos.push_back(lo[1] + ((float)y + 0.5f) * cell[1]); probePos.push_back(lo[2] + ((float)z + 0.5f) * cell[2]);
              }
          std::printf("{\"probe_grid\": [%d, %d, %d], \"origin\": [%.9g, %.9g, %.9g], \"cell\": [%.9g, %.9g, %.9g]}\n", probeGrid[0], probeGrid[1], probeGrid[2], (double)lo[0], (double)lo[1],
                      (double)lo[2], (double)cell[0], (double)cell[1], (double)cell[2]);
        }
        const std::size_t n = probePos.size() / 3;
        const std::vector<float> sh = rs.renderProbes(probePos, spp, seed, bounces);
        std::vector<float> rows(n * 9 * 4);      // the writer takes RGBA: 9 pixels per probe
        for (std::size_t p = 0; p < n * 9; ++p) { rows[p * 4] = sh[p * 3]; rows[p * 4 + 1] = sh[p * 3 + 1]; rows[p * 4 + 2] = sh[p * 3 + 2]; rows[p * 4 + 3] = 1.0f; }
        pbr::image::write_pfm(probesOut, rows.data(), 9, (int)n);
        const ptc_stats st = rs.stats();
        std::printf("{\"scene\": \"%s\", \"probes\": %zu, \"spp\": %d, \"paths\": %llu, \"seconds_render\": %.6f, \"mpaths_per_s\": %.2f}\n", (gltf.empty() ? scene : gltf).c_str(), n, spp,
                    (unsigned long long)st.paths, st.seconds_render, st.seconds_render > 0 ? st.paths / st.seconds_render / 1e6 : 0.0);
        return 0;
      }
      if (bakeLightmap) {
        pbr::PathTraceRenderSystem& rs = *single;
        const std::vector<float> lm = rs.bakeLightmap(lmInstance, lmW, lmH, spp, {}, seed, bounces, lmDilate, lmBackface);
        const auto count = rs.lightmapTexelCount();
        pbr::image::write_pfm(lmOut, lm.data(), lmW, lmH);
        if (!lmAlpha.empty()) {
          std::vector<float> al(lm.size());
          for (std::size_t p = 0; p < lm.size() / 4; ++p) { al[p * 4] = al[p * 4 + 1] = al[p * 4 + 2] = lm[p * 4 + 3]; al[p * 4 + 3] = 1.0f; }
          pbr::image::write_pfm(lmAlpha, al.data(), lmW, lmH);
        }
        const ptc_stats st = rs.stats();
        std::printf("{\"scene\": \"%s\", \"lightmap\": [%d, %d, %d], \"texels\": %u, \"dropped\": %u, \"spp\": %d, \"paths\": %llu, \"seconds_render\": %.6f, \"mpaths_per_s\": %.2f}\n",
                    (gltf.empty() ? scene : gltf).c_str(), lmInstance, lmW, lmH, count[0], count[1], spp, (unsigned long long)st.paths, st.seconds_render,
                    st.seconds_render > 0 ? st.paths / st.seconds_render / 1e6 : 0.0);
        return 0;
      }
      applyLens(*single);
      if (denoiseSampled) single->setSampleCovariance(true);
      img = adaptive ? single->renderAdaptive(w, h, spp, seed, bounces, &ap) : denoiseSampled ? single->renderWithStatistics(w, h, spp, seed, bounces)
                                                                                                : single->render(w, h, spp, seed, bounces, integrator);
    } else {
      std::vector<int> ids;
      for (int i = 0; i < gpus; ++i) ids.push_back(device + i);
      group.reset(new pbr::DeviceGroup(ids));
      buildScene(group->device(0));
      applyLights(group->device(0)); // the group commit and the group render give every member device 0's lights and its choice of transparent shadows
      applyLens(group->device(0));   // the group commit copies the lens with the camera
      group->commitScene();          // one flatten + BVH build on the host, uploaded to every device
      img = group->render(w, h, spp, seed, bounces, integrator);
    }
    pbr::PathTraceRenderSystem& rs = single ? *single : group->device(0);
    if (!gltf.empty()) scene = gltf;
    ptc_stats st = rs.stats();
    for (int i = 1; i < gpus; ++i) { const ptc_stats o = group->device(i).stats(); st.paths += o.paths; st.node_visits_closest += o.node_visits_closest; st.node_visits_any += o.node_visits_any; }
    if (adaptive) {
      const ptc_adaptive_stats as = rs.adaptiveStats();
      std::printf("{\"adaptive_threshold\": %g, \"mean_spp\": %.3f, \"max_spp\": %u, \"passes\": %u, \"seconds_adapt\": %.6f}\n", (double)ap.threshold,
                  as.owned_pixels ? (double)as.samples_total / (double)as.owned_pixels : 0.0, as.max_count, as.passes, as.seconds_adapt);
      if (!countsPath.empty()) {
        const std::vector<std::uint32_t> cnt = rs.sampleCounts();
        std::vector<float> cf(cnt.size() * 4);
        for (std::size_t p = 0; p < cnt.size(); ++p) { cf[p * 4] = cf[p * 4 + 1] = cf[p * 4 + 2] = (float)cnt[p]; cf[p * 4 + 3] = 1.0f; }
        pbr::image::write_pfm(countsPath, cf.data(), w, h);
      }
    }
    if (denoise || !guidesPrefix.empty()) {
      if (integrator != PTC_INTEGRATOR_PATH) throw std::runtime_error("--denoise / --guides need the path integrator (the raster passes are noise-free)");
      rs.frameGuides();
      if (!guidesPrefix.empty()) {
        const std::vector<float> ak = rs.readGuide(PTC_GUIDE_ALBEDO);
        std::vector<float> nz = rs.readGuide(PTC_GUIDE_NORMAL_DEPTH), zz(nz.size());
        for (std::size_t p = 0; p < nz.size(); p += 4) zz[p] = zz[p + 1] = zz[p + 2] = zz[p + 3] = nz[p + 3];
        pbr::image::write_pfm(guidesPrefix + "_albedo.pfm", ak.data(), w, h);
        pbr::image::write_pfm(guidesPrefix + "_normal.pfm", nz.data(), w, h);
        pbr::image::write_pfm(guidesPrefix + "_depth.pfm", zz.data(), w, h);
      }
      if (denoise) {
        ptc_denoise_params dp = pbr::PathTraceRenderSystem::denoiseDefaults();
        if (denoiseIters >= 0) dp.iterations = denoiseIters;
        if (denoiseSampled) rs.denoiseSampled(&dp); else rs.denoise(&dp);
        rs.selectOutput(PTC_OUTPUT_DENOISED);
        img = rs.readRadiance(w, h);
      }
    }
    if (useDisplay) {      // behind the denoiser: the image the outputs serve is the one that is metered
      rs.setDisplay(disp);
      if (disp.auto_exposure) {
        rs.meterExposure();
        const pbr::PathTraceRenderSystem::Exposure e = rs.exposure();
        std::printf("{\"metered_luminance\": %.9g, \"exposure_scale\": %.9g, \"metered_pixels\": %llu, \"rejected_pixels\": %llu}\n", (double)e.meteredLuminance, (double)e.scale,
                    (unsigned long long)e.metered, (unsigned long long)e.rejected);
      }
    }
    if (!halfPath.empty()) {
      const std::vector<std::uint16_t> hb = useDisplay ? rs.displayHalf() : rs.radianceHalf();
      std::ofstream g(halfPath, std::ios::binary);
      g.write(reinterpret_cast<const char*>(hb.data()), (std::streamsize)(hb.size() * 2));
    }
    // A panorama is written the way --env reads a map: top row = up in the reference's y-down world = -y, i.e. with its rows reversed (the library's row 0 is +y).
    // `--panorama --pfm p.pfm` followed by `--env p.pfm` therefore hands the library the image it rendered: the round trip is exact.
    auto panoramaRows = [&](auto& pixels) {
      if (!panorama) return;
      const std::size_t row = (std::size_t)w * 4;
      for (int y = 0; y < h / 2; ++y) std::swap_ranges(pixels.begin() + (std::ptrdiff_t)(y * row), pixels.begin() + (std::ptrdiff_t)((y + 1) * row), pixels.begin() + (std::ptrdiff_t)((h - 1 - y) * row));
    };
    panoramaRows(img);
    pbr::image::write_pfm(out, img.data(), w, h);
    if (!png.empty()) { std::vector<std::uint8_t> ldr = useDisplay ? rs.display() : rs.tonemap(); panoramaRows(ldr); pbr::image::write_png(png, ldr.data(), w, h); }
    if (!ppm.empty()) {
      std::vector<std::uint8_t> ldr = useDisplay ? rs.display() : rs.tonemap();
      panoramaRows(ldr);
      std::ofstream g(ppm, std::ios::binary);
      g << "P6\n" << w << " " << h << "\n255\n";
      for (std::size_t p = 0; p < (std::size_t)w * h; ++p) g.write(reinterpret_cast<const char*>(&ldr[p * 4]), 3);
    }
    std::printf("{\"scene\": \"%s\", \"gpus\": %d, \"paths\": %llu, \"seconds_render\": %.6f, \"mpaths_per_s\": %.2f, \"node_visits\": %llu}\n", scene.c_str(), gpus ? gpus : 1,
                (unsigned long long)st.paths, st.seconds_render, st.seconds_render > 0 ? st.paths / st.seconds_render / 1e6 : 0.0,
                (unsigned long long)(st.node_visits_closest + st.node_visits_any));
  } catch (std::exception const& e) {
    std::cerr << "ptc_render: " << e.what() << "\n";
    return 1;
  }
  return 0;
}
