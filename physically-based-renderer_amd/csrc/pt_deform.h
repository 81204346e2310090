// pt_deform.h — deforming meshes: morph targets and skinning of a mesh's object-space vertices.
//
// The stage BEFORE the flatten: a posed mesh's slice of the object-space vertex array (RefitPlan::mesh_verts and its copy in HBM) is rewritten from the
// mesh's base vertices and a pose; the flatten, the refit, the rebuild and the commit on the device then run as for any other mesh.  pt_deform_morph
// and pt_deform_skin below are the definition — IEEE binary32, no contraction (-ffp-contract=off), in the order written; the host evaluation (pt_deform.cpp) and the kernel
// (pt_deform.hip) both call it, so the device writes the bytes the host computes.  tests/deform_reference.py restates it in numpy.
#pragma once
#include "ptc_internal.h"

// joints and weights of one vertex: one aligned 24-byte record (three 8-byte loads)
struct alignas(8) DeformSkinRec { uint16_t j[4]; float w[4]; };
static_assert(sizeof(DeformSkinRec) == 24, "skin record is 24 bytes");

// What a mesh carries besides its vertices; fixed from ptc_mesh_set_morph_targets / ptc_mesh_set_skin on (the contexts of a group share one copy).
struct DeformMesh {
  uint32_t n_verts = 0, n_targets = 0, n_joints = 0;
  std::vector<float> dp, dn, dt;      // TARGET-MAJOR deltas, [target][vertex][3]: a wave's loads of one target are contiguous.  dn / dt empty: zeros
  std::vector<DeformSkinRec> skin;    // per vertex; empty: the mesh has no skin
};

// A pose: n_targets morph weights, then n_joints joint matrices of 12 floats each — rows 0..2 of a column-major 4x4, column by column:
// J[c * 3 + r] = M[c * 4 + r] (the layout of the instance transforms in pt_refit.h).
inline size_t pt_deform_pose_floats(uint32_t n_targets, uint32_t n_joints) { return (size_t)n_targets + (size_t)n_joints * 12; }

#define PT_DEFORM_HD __host__ __device__ inline

// One morph target: x_c = x_c + w * d_c for position, normal and tangent.xyz (a missing delta array is a zero: the sum is still taken).
PT_DEFORM_HD void pt_deform_morph(float p[3], float n[3], float t[3], float w, const float dp[3], const float dn[3], const float dt[3]) {
  for (int c = 0; c < 3; ++c) { p[c] = p[c] + w * dp[c]; n[c] = n[c] + w * dn[c]; t[c] = t[c] + w * dt[c]; }
}
// The skin: S_e = ((a0 J[j0]_e + a1 J[j1]_e) + a2 J[j2]_e) + a3 J[j3]_e for the 12 entries, weights as given; p'_r = ((S_r0 p_0 + S_r1 p_1) + S_r2 p_2) + S_r3;
// normal and tangent.xyz through the upper 3x3, a three-term sum in the same order.  Nothing is normalised: the flatten does that after the normal matrix.
PT_DEFORM_HD void pt_deform_skin(float p[3], float n[3], float t[3], const float a[4], const float* J0, const float* J1, const float* J2, const float* J3) {
  float S[12];
  for (int e = 0; e < 12; ++e) S[e] = ((a[0] * J0[e] + a[1] * J1[e]) + a[2] * J2[e]) + a[3] * J3[e];
  float q[3], m[3], u[3];
  for (int r = 0; r < 3; ++r) {
    q[r] = ((S[0 + r] * p[0] + S[3 + r] * p[1]) + S[6 + r] * p[2]) + S[9 + r];
    m[r] = (S[0 + r] * n[0] + S[3 + r] * n[1]) + S[6 + r] * n[2];
    u[r] = (S[0 + r] * t[0] + S[3 + r] * t[1]) + S[6 + r] * t[2];
  }
  for (int r = 0; r < 3; ++r) { p[r] = q[r]; n[r] = m[r]; t[r] = u[r]; }
}

// ---- host evaluation: the definition (pt_deform.cpp) ----------------------------------------------------------------------------------
// pose: pt_deform_pose_floats(n_targets, n_joints) floats.  Vertex v of the mesh from base[v]; tangent.w and the texcoord are copied.
void pt_deform_eval_vertex(const DeformMesh&, const HostVertex* base, const float* pose, uint32_t v, HostVertex& out);
void pt_deform_eval_mesh(const DeformMesh&, const HostVertex* base, const float* pose, HostVertex* out);
bool pt_deform_pose_finite(const float* pose, size_t n);

// ---- the kernel (pt_deform.hip) ---------------------------------------------------------------------------------------------------------
struct DevDeform {      // one posed mesh in HBM; base, deltas and skin records stay there from the commit on, the pose is uploaded per evaluation
  const HostVertex* base;
  const float* dp; const float* dn; const float* dt;      // target-major; dn / dt may be null (zeros)
  const DeformSkinRec* skin;                              // null: no skin
  const float* pose;
  HostVertex* out;                                        // the mesh's slice of the object-space vertex array
  uint32_t n_verts, n_targets, n_joints;
};
// one launch per posed mesh: out[v] = pose(base[v]) for every vertex of the mesh
void pt_launch_deform(hipStream_t, const DevDeform&);
