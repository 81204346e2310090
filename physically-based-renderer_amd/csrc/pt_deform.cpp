// pt_deform.cpp — host evaluation of a posed mesh: the definition of DESIGN.md §7a (pt_deform.h has the arithmetic, shared with the kernel).
// The host runs it for the vertices of emissive primitives on every refit (ptc_refit_emitters reads them) and for whole meshes whenever a host path
// needs the description: PTC_REFIT=host, PTC_REBUILD=host, a description-only context, a change of the emitter set, a host commit.
#include "pt_deform.h"

#include <cmath>

void pt_deform_eval_vertex(const DeformMesh& d, const HostVertex* base, const float* pose, uint32_t v, HostVertex& out) {
  const HostVertex b = base[v];
  float p[3] = {b.position[0], b.position[1], b.position[2]};
  float n[3] = {b.normal[0], b.normal[1], b.normal[2]};
  float t[3] = {b.tangent[0], b.tangent[1], b.tangent[2]};
  const float zero[3] = {0.0f, 0.0f, 0.0f};
  for (uint32_t k = 0; k < d.n_targets; ++k) {
    const size_t at = ((size_t)k * d.n_verts + v) * 3;
    pt_deform_morph(p, n, t, pose[k], &d.dp[at], d.dn.empty() ? zero : &d.dn[at], d.dt.empty() ? zero : &d.dt[at]);
  }
  if (!d.skin.empty()) {
    const DeformSkinRec& s = d.skin[v];
    const float* J = pose + d.n_targets;
    pt_deform_skin(p, n, t, s.w, J + (size_t)s.j[0] * 12, J + (size_t)s.j[1] * 12, J + (size_t)s.j[2] * 12, J + (size_t)s.j[3] * 12);
  }
  out = b;      // tangent.w and the texcoord are copied
  for (int c = 0; c < 3; ++c) { out.position[c] = p[c]; out.normal[c] = n[c]; out.tangent[c] = t[c]; }
}

void pt_deform_eval_mesh(const DeformMesh& d, const HostVertex* base, const float* pose, HostVertex* out) {
  for (uint32_t v = 0; v < d.n_verts; ++v) pt_deform_eval_vertex(d, base, pose, v, out[v]);
}

bool pt_deform_pose_finite(const float* pose, size_t n) {
  for (size_t i = 0; i < n; ++i) if (!std::isfinite(pose[i])) return false;
  return true;
}
