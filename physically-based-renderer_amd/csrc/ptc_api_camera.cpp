// ptc_api_camera.cpp — camera models over the C-ABI (pt_camera.h, include/ptc_camera.h): the extended camera's validation and basis, the calls that
// record it, the DevCamera of the camera in force and the refusals of what serves the perspective projection alone.
#include "ptc_ctx.h"

#include <cmath>

using namespace ptc_detail;

namespace {
const char* projection_name(int projection) {
  return projection == PTC_PROJ_ORTHOGRAPHIC ? "PTC_PROJ_ORTHOGRAPHIC" : projection == PTC_PROJ_EQUIRECT ? "PTC_PROJ_EQUIRECT" : "PTC_PROJ_PERSPECTIVE";
}

// The basis of the matrix in binary32, in the header's order: X, Y, Z = the normalised columns, pos = column 3.  The reason it is refused, else nullptr.
const char* camera_basis(const ptc_camera_params& p, v3& X, v3& Y, v3& Z, v3& pos) {
  for (int k = 0; k < 16; ++k) if (!std::isfinite(p.camera_to_world[k])) return "a matrix entry is not finite";
  const v3 c0 = V3(p.camera_to_world), c1 = V3(p.camera_to_world + 4), c2 = V3(p.camera_to_world + 8);
  for (const v3& col : {c0, c1, c2}) if (!(dot3(col, col) > 0.0f)) return "a column of the matrix has zero length";
  X = normalize3(c0); Y = normalize3(c1); Z = normalize3(c2);
  pos = V3(p.camera_to_world + 12);
  for (const v3& a : {X, Y, Z}) if (!std::isfinite(a.x) || !std::isfinite(a.y) || !std::isfinite(a.z)) return "a column of the matrix cannot be normalised";
  if (std::fabs(dot3(X, Y)) > 1e-4f || std::fabs(dot3(X, Z)) > 1e-4f || std::fabs(dot3(Y, Z)) > 1e-4f) return "the columns of the matrix are not orthogonal";
  if (!(dot3(cross3(X, Y), Z) > 0.0f)) return "the matrix is a left-handed frame";
  return nullptr;
}

const char* camera_params_error(const ptc_camera_params& p) {
  if (p.projection != PTC_PROJ_PERSPECTIVE && p.projection != PTC_PROJ_ORTHOGRAPHIC && p.projection != PTC_PROJ_EQUIRECT) return "unknown projection";
  v3 X, Y, Z, pos;
  if (const char* e = camera_basis(p, X, Y, Z, pos)) return e;
  if (p.projection == PTC_PROJ_PERSPECTIVE) {
    if (!(p.yfov > 0.0f && p.yfov < PT_PI)) return "yfov must be in (0, pi)";
    if (!(p.aspect > 0.0f) || !std::isfinite(p.aspect)) return "aspect must be finite and > 0";
  }
  if (p.projection == PTC_PROJ_ORTHOGRAPHIC) {
    if (!(p.xmag > 0.0f) || !std::isfinite(p.xmag) || !(p.ymag > 0.0f) || !std::isfinite(p.ymag)) return "xmag and ymag must be finite and > 0";
  }
  return nullptr;
}
}  // namespace

namespace ptc_detail {
void make_camera_in_force(const ptc_ctx* c, DevCamera& cam) {
  if (!c->cam_ex_set) { ptc_make_camera(c->cam_pos, c->cam_target, c->cam_fov, c->cam_aspect, cam); return; }
  const ptc_camera_params& p = c->cam_ex;
  v3 X, Y, Z, pos;
  (void)camera_basis(p, X, Y, Z, pos);      // accepted when it was set
  scene_rules::store3(cam.pos, pos); scene_rules::store3(cam.s, X); scene_rules::store3(cam.u, -Y); scene_rules::store3(cam.f, -Z);
  if (p.projection == PTC_PROJ_PERSPECTIVE) {
    const float th = (float)std::tan((double)p.yfov * 0.5);      // as ptc_make_camera
    cam.sy = th;
    cam.sx = p.aspect * th;
  } else cam.sx = cam.sy = 1.0f;      // no kernel that reads them runs under the other projections
}

std::string projection_refusal(const ptc_ctx* c, const char* who, const char* what) {
  const int pr = cam_projection(c);
  if (pr == PTC_PROJ_PERSPECTIVE) return std::string();
  return std::string(who) + ": " + what + " under " + projection_name(pr) + " (ptc_set_camera_ex): it serves the perspective projection alone";
}
}  // namespace ptc_detail

extern "C" {
void ptc_camera_default_params(ptc_camera_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof *p);
  p->projection = PTC_PROJ_PERSPECTIVE;
  p->camera_to_world[0] = p->camera_to_world[5] = p->camera_to_world[10] = p->camera_to_world[15] = 1.0f;
  p->yfov = PT_HALF_PI; p->aspect = 1.0f;
  p->xmag = p->ymag = 1.0f;
}

int ptc_set_camera_ex(ptc_ctx* c, const ptc_camera_params* p) {
  if (!c) return PTC_E_ARG;
  if (!p) return fail(c, PTC_E_ARG, "set_camera_ex: null pointer");
  if (const char* e = camera_params_error(*p)) return fail(c, PTC_E_ARG, std::string("set_camera_ex: ") + e);
  // a raster frame in progress would run its next batches on a basis without a projection: the refusal of ptc_frame_begin, made here for a change during the frame
  if (c->in_frame && c->integrator != PTC_INTEGRATOR_PATH && p->projection != PTC_PROJ_PERSPECTIVE)
    return fail(c, PTC_E_STATE, std::string("set_camera_ex: a raster frame is in progress, and the raster integrators do not serve ") + projection_name(p->projection));
  c->cam_ex = *p; c->cam_ex_set = true;
  c->have_cam = true;
  c->guides.valid = false;      // the guides are those of the camera they were traced from
  if (c->committed) make_camera_in_force(c, c->cam);
  return PTC_OK;
}

int ptc_get_camera_ex(const ptc_ctx* c, ptc_camera_params* out) {
  if (!c || !out) return PTC_E_ARG;
  if (!c->cam_ex_set) { std::memset(out, 0, sizeof *out); return 0; }
  *out = c->cam_ex;
  return 1;
}

int ptc_debug_read_guide_positions(ptc_ctx* c, float* out) {
  return read_image(c, "debug_read_guide_positions", out, sizeof(float4), /*all_lanes=*/false, [&](const void*& src) -> int {
    if (!c->guides.valid) return fail(c, PTC_E_STATE, "debug_read_guide_positions: no guides (ptc_frame_guides)");
    src = c->guides.pos.p;
    return PTC_OK;
  });
}
}  // extern "C"
