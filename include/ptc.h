/* ptc.h — C-ABI boundary of the MI355X path-tracing core ("ptc").
 *
 * This is the drop-in boundary of SURVEY.md §8(b).  The reference
 * (WeaponizedSchizophrenia/physically-based-renderer) has no FFI/plugin
 * interface for its render path; the seam is the C++ member call
 *
 *   pbr::PbrRenderSystem::render(cmd, scene, gBuffer, renderTarget, extent)
 *       src/pbr_engine/engine/pbr/PbrRenderSystem.hpp:46-47
 *   called from app::App::recordCommands  src/gltf_viewer/App.cpp:387-388
 *
 * fed by  gltf::Loader::loadAsset / Asset::loadScene
 *       src/pbr_engine/gltf/pbr/gltf/Loader.hpp:20-21, Asset.hpp:76-78
 * and consumed by TonemapperSystem::run
 *       src/pbr_engine/engine/pbr/TonemapperSystem.cpp:97-134.
 *
 * Each entry point below names the reference interface it replaces.  Plain C:
 * opaque handle, plain pointers and sizes, int status (0 = ok, <0 = error,
 * text via ptc_last_error).  The caller owns every input array (copied during
 * the call); the library owns all device memory.  A context is bound to one
 * HIP device and is not re-entrant; distinct contexts are independent.
 *
 * The library behind this header is HIP-only.  There is no CPU fallback:
 * ptc_create fails (returns NULL, ptc_last_error(NULL) says why) when no
 * gfx950 device is usable.
 */
#ifndef PTC_H
#define PTC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTC_ABI_VERSION 4

typedef struct ptc_ctx ptc_ctx;

/* status codes */
enum {
  PTC_OK = 0,
  PTC_E_ARG = -1,      /* bad argument (null pointer, index out of range, bad size) */
  PTC_E_STATE = -2,    /* call out of order (e.g. render before scene_commit)       */
  PTC_E_DEVICE = -3,   /* HIP / RCCL error (text carries hipGetErrorString)         */
  PTC_E_NOMEM = -4     /* hipErrorOutOfMemory: queues or scene do not fit the device */
};

/* integrators */
enum {
  PTC_INTEGRATOR_PATH = 0,          /* wavefront path tracer (SURVEY §8a-2 P1–P10)                  */
  PTC_INTEGRATOR_RASTER_COMPAT = 1, /* primary hit + the reference's Blinn-Phong pass (R6,R7,R8):
                                       assets/shaders/pbr/lighting.glsl:19-29, lit from fp32 P, N, albedo */
  PTC_INTEGRATOR_RASTER_GBUFFER16 = 2 /* the same pass lit from what the reference's G-buffer holds
                                       (engine/pbr/GBuffer.hpp:13-16): positions and normals rounded to
                                       RGBA16F (round to nearest even), albedo to RGBA16 UNORM, the normal not
                                       re-normalised; read the result with ptc_read_radiance_rgba16f for the
                                       RGBA16F lighting target (PbrRenderSystem.hpp:21)              */
};

/* Vertex record == pbr::MeshVertex (src/pbr_engine/engine/pbr/MeshVertex.hpp:14-19):
 * {vec3 position; vec3 normal; vec4 tangent; vec2 texCoords}, 48 bytes, tightly packed. */
typedef struct ptc_vertex {
  float position[3];
  float normal[3];
  float tangent[4];
  float texcoord[2];
} ptc_vertex;

/* Counters of the last frame ("counted, not estimated"). */
typedef struct ptc_stats {
  uint64_t paths;             /* camera samples traced                                   */
  uint64_t segments;          /* closest-hit rays cast (camera + continuation)           */
  uint64_t shadow_rays;       /* any-hit (NEE) rays cast                                 */
  uint64_t hits;              /* closest-hit rays that hit a surface                     */
  uint64_t node_visits_closest;
  uint64_t tri_tests_closest;
  uint64_t node_visits_any;
  uint64_t tri_tests_any;
  uint64_t algorithmic_bytes; /* SURVEY §8d byte formula evaluated on the counters above */
  double seconds_render;      /* device time of the frame's kernels (HIP events)         */
  double seconds_trace_closest; /* HIP-event time of the dominant kernel (sum over launches).  The three per-kernel sums cover the batches whose
                                 * kernels run one after the other; a small batch (<= 2^26 paths) runs k_trace_any(b) beside k_trace_closest(b + 1) and
                                 * carries the batch's span only (seconds_render) — PTC_TIMING=2 records per-kernel spans for those too (they then
                                 * include each other), PTC_TIMING=0 records nothing */
  double seconds_trace_any;
  double seconds_shade;
  double seconds_commit;      /* flatten + BVH build + upload                               */
  double seconds_reduce;      /* HIP-event time of ptc_comm_reduce_radiance on this rank's stream (includes waiting for the slowest rank) */
  double seconds_refit;       /* the last ptc_scene_refit: re-flatten + refit of the committed tree + upload                */
  uint32_t launches_trace_closest;
  uint32_t launches_trace_any;
  uint32_t n_triangles;
  uint32_t n_bvh_nodes;
  uint32_t n_emitters;
  uint32_t bvh_max_depth;
  /* ABI 4 (round 4): what a moved scene's tree costs, so that a caller can decide when a refit is no longer enough.
   * bvh_sa_cost = the surface-area cost of the 8-wide tree as it lies in HBM: sum over the nodes' child slots of half_area(child box) /
   * half_area(scene box when the tree's topology was made), a two-triangle leaf counted twice — the expected number of node visits + triangle
   * tests of a random long ray, up to a constant; the unit stays through refits, so the figures of a moving scene can be compared.  Written by ptc_scene_commit, by every ptc_scene_refit and ptc_scene_rebuild (one reduction inside the node pass, in
   * fixed point: the same bits whatever the order).  bvh_sa_cost_built = its value when the tree's TOPOLOGY was made (commit or rebuild): the ratio
   * of the two is what examples/viewer_shim.cpp watches. */
  double bvh_sa_cost;
  double bvh_sa_cost_built;
  double seconds_rebuild;     /* the last ptc_scene_rebuild: flatten + build (the device builder's) + refit pass, all on the device */
} ptc_stats;

/* ---- context ------------------------------------------------------------------------------
 * Replaces core::makeGpuHandle + MemoryAllocator bring-up
 * (src/pbr_engine/core/pbr/core/GpuHandle.cpp:94-101, engine/pbr/memory/MemoryAllocator.cpp:68-88).
 * device_id: HIP ordinal.  Returns NULL on failure.
 * PTC_DEVICE_NONE gives a description-only context: the scene calls (begin/add/commit: flatten +
 * BVH build on the host) and the ptc_debug_get_* hooks work, every call that needs the GPU fails with
 * PTC_E_DEVICE.  It exists so that the host logic can be checked without a GPU; it renders nothing. */
#define PTC_DEVICE_NONE (-1)
ptc_ctx* ptc_create(int device_id);
void ptc_destroy(ptc_ctx*);
/* Last error text of the context (or of the last failed ptc_create when ctx == NULL). */
const char* ptc_last_error(const ptc_ctx*);
int ptc_abi_version(void);
/* "ptc abi N gfx950 kernels-sha256 <64 hex digits>": the hash is over the kernel sources this library was built from
 * (csrc/Makefile); bench.py compares it with the hash in the committed kernel model its roofline block is calibrated on. */
const char* ptc_build_info(void);
/* "name=value ..." of everything that decides how the kernels are launched: their compile-time constants (block sizes, chunk, ring, thresholds), the
 * context's knobs after the environment was read (lanes, batch size, overlap mode, nodelets, builder ...) and, once a scene is committed on a device, what
 * followed from them (trace blocks per CU, stack entries in LDS, queue segments).  ctx == NULL: the built-in defaults, no device needed.  A measured
 * per-kernel figure is only valid for the policy it was measured under: tools/make_kernel_model.py records this string with the profile, bench.py prints
 * it and reports model_stale when it differs, tests/test_profiles.py fails when the defaults move without a new profile.  The pointer is valid until the
 * calling thread's next call. */
const char* ptc_launch_policy(const ptc_ctx*);

/* ---- scene description --------------------------------------------------------------------
 * Replaces gltf::Asset::loadScene → MeshBuilder::build → TransferStager
 * (src/pbr_engine/gltf/pbr/gltf/Asset.cpp:135-273, engine/pbr/MeshBuilder.cpp:16-55,
 *  engine/pbr/TransferStager.cpp:51-177). */
int ptc_scene_begin(ptc_ctx*);

/* pbr::MaterialData{vec4 color} (engine/pbr/Material.hpp:14-16) widened with the glTF
 * metal-rough + emissive factors the reference ignores (gltf/Asset.cpp:142-150).
 * tex_* are texture ids from ptc_add_texture_rgba8 or -1.  Returns material id >= 0. */
int ptc_add_material(ptc_ctx*, const float base_color[4], float metallic, float roughness,
                     const float emissive[3], int tex_color, int tex_normal, int tex_mr);

/* image::loadImage2D output: RGBA8, 4 channels forced (image/pbr/image/LoadImage.cpp:56-73);
 * sampled NEAREST/REPEAT like the reference's default sampler (gltf/Asset.cpp:116-117).
 * Returns texture id >= 0. */
int ptc_add_texture_rgba8(ptc_ctx*, const uint8_t* px, int w, int h);

/* One MeshBuilder::Primitive (engine/pbr/MeshBuilder.hpp:14-18) with indices widened to u32
 * (reference: u16, Asset.cpp:197-201).  Triangle list, indices primitive-local.
 * Returns mesh id >= 0. */
int ptc_add_mesh(ptc_ctx*, const ptc_vertex* verts, uint32_t n_verts, const uint32_t* indices,
                 uint32_t n_indices, int material);

/* pbr::Transform + makeModelPushConstant (engine/pbr/Scene.hpp:19-23,
 * ModelPushConstant.hpp:33-46): model = T·R·S, quaternion order (w,x,y,z). */
int ptc_add_instance(ptc_ctx*, int mesh, const float t[3], const float q_wxyz[4],
                     const float s[3]);
/* makeModelPushConstant(glm::mat4x4 model) (ModelPushConstant.hpp:33-38): an instance by its column-major
 * 4x4 model matrix (used by the glTF loader, which composes parent transforms). */
int ptc_add_instance_matrix(ptc_ctx*, int mesh, const float model[16]);

/* Scene dynamics.  The viewer turns its nodes every frame (src/gltf_viewer/App.cpp:306-313) and draws each node with its own
 * model matrix (the push constant of PbrRenderSystem.cpp:444-448), so a transform change costs the reference nothing.  Here the
 * triangles live in one world-space tree, so a change is two steps: ptc_update_instance / ptc_update_instance_matrix give instance
 * `instance` (the value ptc_add_instance* returned) a new transform, any number of them; ptc_scene_refit then re-flattens the
 * vertices and REFITS the committed tree — same topology, same slots, same layout; every box re-computed bottom-up and re-quantised,
 * triangle records, shading records and emitters rewritten — in place in HBM (textures, environment and materials are not
 * touched).  The refit runs ON THE DEVICE (csrc/pt_refit.hip: the same arithmetic as the host's, element-parallel; 84 bytes per
 * instance and the emitter table are all that crosses the bus); PTC_REFIT=host in the environment, a description-only context, or
 * a move that changes which triangles are emitters (a zero-area scale) take the host refit + upload instead — both give the same
 * bytes (ptc_debug_get_bvh / ptc_debug_get_shading_tables).  No re-build either way (ptc_stats.seconds_refit beside seconds_commit).  A refitted tree renders the same image as a fresh commit of the same transforms
 * (closest hit = minimum of (t, primitive id), whatever the tree); its traversal counters are those of the refitted tree, and the
 * oracle refits the same way.  Meshes, materials or the number of instances cannot change this way: that is a new scene.
 * A frame in progress ends (call ptc_frame_begin again).  PTC_E_STATE before the first ptc_scene_commit. */
int ptc_update_instance(ptc_ctx*, int instance, const float t[3], const float q_wxyz[4], const float s[3]);
int ptc_update_instance_matrix(ptc_ctx*, int instance, const float model[16]);
int ptc_scene_refit(ptc_ctx*);
/* A refit keeps the tree of the commit: topology and octant slots follow the geometry they were made for, and the viewer turns its nodes without
 * bound (App.cpp:306-313: rotate(rotation, deltaTime) every frame) — after a third of a turn the atrium's rays visit 1.5x the nodes
 * (profiles/r04_refit_curve.txt).  ptc_scene_rebuild applies the pending instance transforms like ptc_scene_refit and then builds a NEW tree for the
 * geometry as it now lies in HBM, ON THE DEVICE (csrc/pt_build.hip): 63-bit Morton codes, LDS radix sort, the radix tree, bottom-up boxes and collapse
 * costs, the same cost-optimal 8-wide collapse, octant slots, quantisation and unit layout as the host's LBVH builder (PTC_BVH_LBVH) — the bytes a
 * fresh ptc_scene_commit of the moved scene with that builder would upload (tests/test_gpu_parity.py compares them), in milliseconds and without
 * the description crossing the bus again.  The image does not depend on the tree; counters and speed are those of the new tree.  Whatever builder
 * the commit used, the rebuilt tree is the device builder's (ptc_set_device_builder): the LBVH by default, the host's binned-SAH tree (the
 * bytes of a fresh PTC_BVH_SAH commit of the moved scene) with PTC_BVH_SAH.  Needs a device; PTC_E_STATE before the first commit; a move that changes which triangles are
 * emitters falls back to a host build + upload (as ptc_scene_refit does).  ptc_stats.bvh_sa_cost / bvh_sa_cost_built say when it is worth calling. */
int ptc_scene_rebuild(ptc_ctx*);

/* ---- deforming meshes: morph targets and skinning, evaluated on the device (csrc/pt_deform.h is the definition) ----------------
 * A mesh may carry T >= 0 morph targets — per vertex a position, a normal and a tangent delta — and a skin: per vertex 4 joint indices and 4 weights over
 * n_joints >= 1 joints.  A POSE is T weights and n_joints joint matrices of 12 floats: rows 0..2 of a column-major 4x4, column by column
 * (J[c * 3 + r] = M[c * 4 + r]); the default pose is weights 0 and identity matrices.  Per vertex, from the mesh's BASE vertex, in IEEE binary32 without
 * contraction, in the order written:
 *   morph   for k = 0 .. T-1 ascending: p_c = p_c + w_k dp_k,c; the same for the normal and for tangent.xyz (a missing delta array is zeros)
 *   skin    S_e = ((a0 J[j0]_e + a1 J[j1]_e) + a2 J[j2]_e) + a3 J[j3]_e for the 12 entries, the weights as given (no renormalisation);
 *           p'_r = ((S_r0 p_0 + S_r1 p_1) + S_r2 p_2) + S_r3; normal and tangent.xyz through the upper 3x3, a three-term sum in the same order
 *   tangent.w and the texcoord are copied; nothing is normalised (the flatten normalises N, T, B after the normal matrix, as for every mesh).
 * The instance transform applies afterwards, unchanged: a glTF joint matrix is inverse(global(mesh node)) global(joint) inverseBind.
 *
 * ptc_mesh_set_morph_targets / ptc_mesh_set_skin belong to the description: after ptc_add_mesh, before ptc_scene_commit (PTC_E_STATE once committed).
 *   dpos, dnormal, dtangent: n_targets * n_verts * 3 floats each, TARGET-major ([target][vertex][3]); dnormal and dtangent may be NULL; n_targets = 0
 *   removes the targets.  joints_u16x4 / weights_f32x4: n_verts * 4 each; a joint index >= n_joints gives PTC_E_ARG.  Both reset that half of the pose
 *   to the default.
 * ptc_update_mesh_pose (any time after the mesh exists): a non-NULL array must come with the mesh's count (T weights, n_joints matrices), otherwise
 *   PTC_E_ARG and nothing changes; a NULL array leaves that half of the pose as it is.
 * ptc_update_mesh_vertices: replaces the mesh's BASE vertices (same count, otherwise PTC_E_ARG) — for a caller who deforms on their own, e.g. a
 *   simulation; works on any mesh.
 * Both update calls only record.  ptc_scene_commit, ptc_scene_refit, ptc_scene_rebuild and ptc_group_scene_refit (the poses set on ptc_group_ctx(g, 0), as
 * for transforms) apply them.  Where the refit runs on the device, the posed meshes are evaluated there by csrc/pt_deform.hip, into the object-space
 * vertices the flatten reads: only the pose crosses the bus.  The host evaluates the same expressions for the vertices of emissive primitives (the emitter
 * table is the host's), and whole meshes when a host path needs them (PTC_REFIT=host, PTC_REBUILD=host, a description-only context, a change of the
 * emitter set, a host commit).  A commit of a posed description is byte for byte the commit of plain meshes that hold the posed vertices; a refit refused
 * for a non-finite position leaves the scene in HBM, object-space vertices included, as it was; the temporal history survives a deformation as it
 * survives a refit.  ptc_scene_begin drops all of it.  A context that never calls these computes what it always did. */
int ptc_mesh_set_morph_targets(ptc_ctx*, int mesh, uint32_t n_targets, const float* dpos, const float* dnormal, const float* dtangent);
int ptc_mesh_set_skin(ptc_ctx*, int mesh, uint32_t n_joints, const uint16_t* joints_u16x4, const float* weights_f32x4);
int ptc_update_mesh_pose(ptc_ctx*, int mesh, const float* morph_weights, uint32_t n_weights, const float* joint_matrices, uint32_t n_joints);
int ptc_update_mesh_vertices(ptc_ctx*, int mesh, const ptc_vertex* verts, uint32_t n_verts);

/* pbr::makeCameraData (engine/pbr/CameraData.hpp:22-32): lookAtRH(pos,target,up=(0,-1,0)),
 * perspective fovY/aspect; y-down un-flipped viewport (PbrRenderSystem.cpp:425-430). */
int ptc_set_camera(ptc_ctx*, const float pos[3], const float target[3], float fov_y,
                   float aspect);

/* ---- thin-lens camera: depth of field with a circular or a bladed aperture (no counterpart in the reference, whose camera is a pinhole) ----
 * The lens belongs to the camera and lives in ray generation alone.  With aperture_radius R > 0 every sample of the path integrator starts at a point l of
 * the aperture — a disk of radius R, or a regular polygon of `blades` sides with circumradius R and a vertex at `rotation` turns, in the camera's (right, up)
 * plane through its position — and goes through the point that the pinhole ray of the same jittered pixel position meets at view depth focus_distance F
 * (measured along the forward axis): surfaces at depth F are sharp, a point at depth z spreads over a disk of radius R |1 - z / F| on its own depth plane.
 * Throughput 1, no cos^4 term and no vignetting, as for the pinhole.  The lens point is drawn from dimensions 2 and 3 of the path's RNG index 0, which
 * nothing else uses; DESIGN.md 2a and csrc/pt_lens.h have the arithmetic (IEEE binary32 in the order written, as every value of the renderer).
 * R = 0 (the default) is the pinhole: ray generation then runs as it always did, and a context that never calls these computes what it always did.
 *
 * ptc_set_camera_lens: params == NULL means the defaults (0, 1, 0, 0).  Needs no device.  PTC_E_ARG, and nothing changed, for a negative or non-finite
 *   aperture_radius, a focus_distance that is not finite and > 0, blades other than 0 or 3..16, a rotation outside [0, 1) or non-finite.  The lens has the
 *   lifetime of the camera: kept across ptc_set_camera, reset to the defaults by ptc_scene_begin, copied by ptc_group_scene_commit wherever the camera is; a
 *   change during a frame applies to the batches queued afterwards, as a ptc_set_camera does.
 * What ignores the lens: the raster integrators; ptc_frame_guides, the temporal reprojection and the denoisers, which keep the ray through the lens centre —
 *   the pinhole ray — so setting the lens does not invalidate guides.  Known limit: the guides of an out-of-focus region are sharp, so the edge-stopping
 *   filters smooth less there than the blur of the radiance would allow; lens-averaged guides are not provided.
 * ptc_focus_distance_at_pixel: the view depth of what the pixel centre of (px, py) sees, for focusing on it: *out = Z / sqrt(fma(dvy, dvy, fma(dvx, dvx, 1)))
 *   with Z the depth guide of the pixel and dvx, dvy the view-space slopes of its centre ray; 0 on a miss.  Needs valid guides of the current frame
 *   (PTC_E_STATE otherwise) and a pixel inside it (PTC_E_ARG otherwise).  One 16-byte read-back: the call waits for the device. */
typedef struct ptc_lens_params {
  float aperture_radius;  /* R >= 0, world units; 0 = pinhole (default 0)                               */
  float focus_distance;   /* F > 0, view depth of the plane of focus along the forward axis (default 1) */
  int   blades;           /* 0 = disk, 3..16 = regular polygon with circumradius R (default 0)          */
  float rotation;         /* of the polygon, in turns, [0, 1) (default 0)                               */
} ptc_lens_params;
void ptc_lens_default_params(ptc_lens_params*);
int  ptc_set_camera_lens(ptc_ctx*, const ptc_lens_params*);    /* NULL: the defaults */
int  ptc_get_camera_lens(const ptc_ctx*, ptc_lens_params*);
int  ptc_focus_distance_at_pixel(ptc_ctx*, int px, int py, float* out);

/* ---- punctual lights: point, spot and directional (glTF KHR_lights_punctual; no counterpart in the reference, which has no lights) ----
 * A punctual light has no area.  The path integrator samples it by next-event estimation in a pass of its own behind the shading of every bounce
 * b < max_bounces: one light per hit, chosen with probability sampling_weight / sum of the weights, a shadow ray, and the unoccluded contribution
 * T f(wo, wi) Li cos / pmf added to the path.  No MIS weight: a BSDF sample cannot hit such a light, the term adds to emitters and environment.
 * Radiance arriving at P from the unit direction wi (csrc/pt_lights.h and DESIGN.md 2b have the arithmetic, IEEE binary32 in the order written):
 *   PTC_LIGHT_POINT        Li = intensity / d^2 (W/sr: glTF colour x candela), times the window clamp(1 - (d / range)^4, 0, 1) when range > 0
 *   PTC_LIGHT_SPOT         the same times s^2, s = clamp((cd - cos_outer) / max(cos_inner - cos_outer, 0.001), 0, 1), cd = dot(direction, -wi): `direction` is
 *                          the axis the light points along; 1 >= cos_inner > cos_outer >= -1
 *   PTC_LIGHT_DIRECTIONAL  Li = intensity, the irradiance on a facing surface (glTF colour x lux); `direction` is the way the light travels
 * At most PTC_MAX_LIGHTS lights.  A scene without them launches exactly the kernels it always launched.
 *
 * The calls need no device and only record; they are valid any time after ptc_scene_begin, which drops all lights.  Lights are not part of the tree: adding,
 * changing or clearing them needs no commit and no refit.  ptc_frame_begin uploads a changed table, so a change during a frame applies from the next
 * ptc_frame_begin.  ptc_group_scene_commit and ptc_group_render give every member the lights of ptc_group_ctx(g, 0).
 * ptc_add_light returns the light's id (>= 0; ids count from 0 in the order added).  ptc_add_light / ptc_update_light: PTC_E_ARG, and nothing changed, for
 *   an unknown type, a non-finite field, a negative intensity or range, a zero direction where one is needed (spot, directional), cone cosines out of order
 *   (spot), a sampling_weight that is not finite and > 0, an id out of range, a light beyond PTC_MAX_LIGHTS.  The direction is stored normalised.
 * What ignores the lights: the raster integrators, ptc_frame_guides, the denoisers and the temporal history. */
enum { PTC_LIGHT_POINT = 0, PTC_LIGHT_SPOT = 1, PTC_LIGHT_DIRECTIONAL = 2 };
#define PTC_MAX_LIGHTS 256
typedef struct ptc_light_params {
  int   type;             /* PTC_LIGHT_*                                                                  */
  float position[3];      /* point, spot                                                                  */
  float direction[3];     /* spot: the axis it points along; directional: the way the light travels      */
  float intensity[3];     /* rgb >= 0: W/sr (point, spot) or irradiance (directional)                     */
  float range;            /* >= 0; 0 = no range window (point, spot)                                      */
  float cos_inner;        /* spot: full intensity inside this cosine ...                                  */
  float cos_outer;        /* ... none outside this one                                                    */
  float sampling_weight;  /* > 0: relative probability of being chosen for a hit (default 1)             */
} ptc_light_params;
void ptc_light_default_params(ptc_light_params*);   /* a white point light of intensity 1 at the origin, direction -z, no range, cone cosines 1 and cos(pi/4), weight 1 */
int  ptc_add_light(ptc_ctx*, const ptc_light_params*);
int  ptc_update_light(ptc_ctx*, int id, const ptc_light_params*);
int  ptc_get_light(const ptc_ctx*, int id, ptc_light_params* out);
int  ptc_light_count(const ptc_ctx*);
int  ptc_clear_lights(ptc_ctx*);

/* Alpha coverage: the glTF alphaMode of a material (OPAQUE is the default).  The calls that set it, the statistics and the test hooks are declared in ptc_alpha.h,
 * which this header includes at its end; DESIGN.md 2d has the specification. */
enum { PTC_ALPHA_OPAQUE = 0, PTC_ALPHA_MASK = 1, PTC_ALPHA_BLEND = 2 };

/* Lat-long environment light (BASELINE config 5; no counterpart in the reference, which has no lights): w*h RGB
 * fp32 texels, row 0 = +y, u = atan2(d.z, d.x)/(2 pi) + 1/2, piecewise-constant radiance, importance-sampled by
 * luminance x sin(theta).  rgb == NULL removes it.  Call before ptc_scene_commit. */
int ptc_set_env_latlong_rgb32f(ptc_ctx*, const float* rgb, int w, int h);

/* Texture filter of the scene being described (applies to every texture; reset to NEAREST by ptc_scene_begin).
 * PTC_FILTER_NEAREST is what the reference renders with — its samplers are default-constructed (gltf/Asset.cpp:116-117:
 * NEAREST, REPEAT, no mips).  PTC_FILTER_LINEAR is an option the reference does not have: bilinear over the 4 nearest
 * texels (centres at i + 1/2), REPEAT wrap, lerp(a, b, t) = fma(t, b - a, a) along x then y. */
enum { PTC_FILTER_NEAREST = 0, PTC_FILTER_LINEAR = 1 };
int ptc_set_texture_filter(ptc_ctx*, int filter);

/* BVH builder of the scene being described (reset by ptc_scene_begin to the context's default: PTC_BVH_SAH, or PTC_BVH_LBVH when
 * the environment has PTC_BVH=lbvh).  Both give a binary tree over single triangles that the same cost-optimal collapse turns into
 * the 8-wide quantised tree; images are identical up to the order-independence of closest hit, traversal counters differ.
 *   PTC_BVH_SAH   top-down binned surface-area splits (32 bins): the default; on the benchmark scene 17 % fewer node visits per
 *                 closest-hit ray and 28 % fewer per shadow ray than the LBVH
 *   PTC_BVH_LBVH  the radix tree of 63-bit Morton codes of the triangle-box centres (BASELINE.json north_star's "flattened LBVH") */
enum { PTC_BVH_SAH = 0, PTC_BVH_LBVH = 1 };
int ptc_set_bvh_builder(ptc_ctx*, int builder);

/* The tree a build ON THE DEVICE makes (context setting, kept across ptc_scene_begin; default PTC_BVH_LBVH, or PTC_BVH_SAH when the
 * environment has PTC_DEVICE_BVH=sah at ptc_create).  With PTC_BVH_SAH, ptc_scene_commit of a PTC_BVH_SAH scene on a device context
 * builds on the device too (csrc/pt_build.hip: the host's binned-SAH binary tree, cut for cut, then the same collapse and layout — the
 * bytes of the host's SAH commit), and ptc_scene_rebuild makes the SAH tree whatever builder the commit used; the host fallbacks of a
 * rebuild (PTC_REBUILD=host, a change of the emitters, a single triangle) build the SAH tree too.  A PTC_BVH_LBVH scene still commits
 * as the LBVH.  ptc_group_scene_commit keeps its one host build on device 0.  A description-only context takes the setting and builds
 * on the host as before.  ptc_debug_get_internals [7] bit 2 says that the tree in HBM is a device SAH build. */
int ptc_set_device_builder(ptc_ctx*, int builder);   /* PTC_BVH_LBVH | PTC_BVH_SAH; anything else: PTC_E_ARG, setting unchanged */

/* Flatten instances to world space (geometry_pass/vertex.glsl:25-36), build + flatten the BVH,
 * build the emitter CDF, upload everything to HBM.  With PTC_BVH_SAH (the default) flatten and build run on the host's
 * thread pool (75 ms at 250 k triangles).  With PTC_BVH_LBVH on a device context — or PTC_BVH_SAH with the SAH device
 * builder (ptc_set_device_builder) — the host only describes (indices, materials, emitter table, textures) and the DEVICE
 * flattens the vertices, writes the shading records and builds the tree (csrc/pt_refit.hip, csrc/pt_build.hip): 3-5 ms at
 * 250 k triangles for the LBVH, the arrays in HBM byte for byte those of the host's commit with the same builder
 * (PTC_COMMIT=host in the environment keeps that path; ptc_debug_get_internals [7] bit 1 says which ran). */
int ptc_scene_commit(ptc_ctx*);

/* ---- rendering ----------------------------------------------------------------------------
 * Replaces PbrRenderSystem::render (engine/pbr/PbrRenderSystem.cpp:357-365).
 * ptc_render == frame_begin + frame_add_samples(spp) + frame_resolve. */
int ptc_render(ptc_ctx*, int w, int h, int spp, uint64_t seed, int max_bounces, int integrator);

/* Progressive form.  tile_rank/tile_count select the 32×32-pixel tiles this context owns
 * (tile t along a Morton walk belongs to rank t mod tile_count); 0/1 = whole frame.
 * spp_total is the sample BUDGET of the frame: frame_add_samples fails with PTC_E_ARG beyond it. */
int ptc_frame_begin(ptc_ctx*, int w, int h, int spp_total, uint64_t seed, int max_bounces,
                    int integrator, int tile_rank, int tile_count);
/* Accept the next n_samples samples of every owned pixel.  Asynchronous: full wavefront batches (as many samples as
 * fit the path budget, PTC_BATCH_PATHS, split over the lanes) are queued on the device at once; a remainder is held
 * back and merged with the samples of later calls, so that many small calls still produce full-width launches.
 * ptc_frame_resolve / ptc_sync / ptc_get_stats queue whatever is still held back.  Queues are sized by the batches
 * actually issued: adding one sample per call needs queues for one sample per pixel. */
int ptc_frame_add_samples(ptc_ctx*, int n_samples);
/* Optional: allocate the current frame's wavefront queues for FULL batches now (min(batch, spp_total) samples per owned pixel and
 * lane).  Without it the queues grow with the batches issued — right for a viewer that adds a sample per displayed frame, but a
 * growth step drains the device and reallocates; an offline render that will spend its budget calls this once after
 * ptc_frame_begin so that nothing is allocated while it renders.  PTC_E_NOMEM if the queues do not fit. */
int ptc_frame_reserve(ptc_ctx*);
/* sum / (samples accumulated so far) → full-frame RGBA32F (zeros in pixels this context does not own): after k of
 * N samples the buffer holds the k-sample image, correctly exposed (progressive display). */
int ptc_frame_resolve(ptc_ctx*);
/* Block until all queued device work of this context has finished. */
int ptc_sync(ptc_ctx*);

/* Output == the HdrImage the tonemapper consumes (engine/pbr/HdrImage.cpp:12-45), as fp32:
 * w*h*4 floats, row-major, y-down, alpha = 1 where owned. */
int ptc_read_radiance_rgba32f(ptc_ctx*, float* out);
/* Device pointer of that buffer (w*h*4 floats) for in-place RCCL reduction by the caller. */
void* ptc_radiance_device_ptr(ptc_ctx*);
/* Overwrite the radiance buffer from host (e.g. after a reduce) before tonemapping. */
int ptc_write_radiance_rgba32f(ptc_ctx*, const float* in);
/* The same image in the reference's own HdrImage format, vk::Format::eR16G16B16A16Sfloat
 * (engine/pbr/PbrRenderSystem.hpp:21, HdrImage.cpp:20): w*h*4 IEEE binary16 values (as uint16_t), fp32 → fp16 by
 * round-to-nearest-even, overflow → inf, half denormals kept.  This is what a viewer shim copies into the HdrImage
 * (INTEGRATION.md §2).  The device-pointer form converts on the context's stream, waits for the conversion and
 * returns a buffer that stays valid until the next call of either function (NULL on error). */
int ptc_read_radiance_rgba16f(ptc_ctx*, uint16_t* out);
void* ptc_radiance_rgba16f_device_ptr(ptc_ctx*);

/* TonemapperSystem::run + tonemappers/aces+gamma.glsl:10-40 on the radiance buffer → RGBA8. */
int ptc_tonemap_rgba8(ptc_ctx*, uint8_t* out);

/* ---- checkpoint / resume, sample ranges (SURVEY §5 "optional later", §8e "kept as an option").  The RNG is counter-based — sample k of pixel p draws from
 * hash(seed, p, k) — and a pixel's sum is taken in sample order, so a frame is resumable by its sums and a count.
 *   ptc_frame_checkpoint: everything queued is finished; the per-pixel sums (n_owned x RGBA fp32, in the order of the frame's owned pixels: an opaque blob for
 *     ptc_frame_restore; NULL to query the sizes only) and the number of samples in them.
 *   ptc_frame_restore: right after a ptc_frame_begin with the SAME parameters (size, seed, bounces, tile share; spp_total may be larger): the sums and the
 *     count are put back, the next sample added is sample `samples_done`.  checkpoint after k samples + restore + the remaining samples = the uninterrupted
 *     frame, bit for bit.
 *   ptc_frame_set_sample_range: right after ptc_frame_begin: the frame's samples have the indices first_sample, first_sample + 1, ...; with resolve_divisor != 0
 *     the resolve divides by it instead of by the samples accumulated.  Sharding a frame by SAMPLES instead of by tiles: rank r of N renders all pixels
 *     (tile_count 1), spp/N samples from first_sample = r x spp/N, resolve_divisor = spp: the reduce's sum of the partial means is the frame (fp32 sums in another
 *     order than on one GPU: equal to rounding, not bit for bit — which is why tiles are the default). */
int ptc_frame_checkpoint(ptc_ctx*, float* accum_rgba, uint64_t* n_owned_pixels, uint32_t* samples_done);
int ptc_frame_restore(ptc_ctx*, const float* accum_rgba, uint64_t n_owned_pixels, uint32_t samples_done);
int ptc_frame_set_sample_range(ptc_ctx*, uint32_t first_sample, uint32_t resolve_divisor);

int ptc_get_stats(ptc_ctx*, ptc_stats* out);

/* ---- first-hit guide buffers, the denoiser, output selection ---------------------------------------------------------------------
 * A path-traced frame of a few samples is mostly noise; these calls turn it into a displayable image.  Nothing here changes what a context that never
 * calls them computes.
 *
 * ptc_frame_guides: needs a frame begun with PTC_INTEGRATOR_PATH (PTC_E_STATE otherwise: the raster integrators are noise-free).  For EVERY pixel of the
 *   frame, whatever the frame's tile share (the root of a tile-sharded frame holds the whole image after the reduce), it traces the path integrator's camera ray
 *   with the jitter fixed at (0.5, 0.5) — no near/far clip, no culling, closest hit = minimum of (t, primitive id) — and writes per pixel
 *     class K    0 miss, 1 surface, 2 emitter (the hit material's emissive factor has a non-zero component)
 *     albedo A   K = 1: the base colour rgb after the colour texture (the scene's filter mode included); (1, 1, 1) otherwise
 *     normal N   K = 1: the normalised interpolated vertex normal (no normal map); 0 otherwise.  depth Z: the hit's t along the unit ray, 0 on a miss
 *     the primitive id (-1 = miss) and the barycentrics of the hit
 *   PTC_GUIDE_ALBEDO reads (A, (float)K), PTC_GUIDE_NORMAL_DEPTH (N, Z).  Queued on the context's stream; the frame in progress is not disturbed: sums, sample
 *   counts, held-back samples, the frame's ptc_stats counters and the RNG are untouched.  The guides stay valid until the next ptc_frame_begin, ptc_set_camera,
 *   ptc_scene_commit, ptc_scene_refit or ptc_scene_rebuild.
 * ptc_denoise: the variance-guided edge-avoiding a-trous filter of DESIGN.md ("Denoiser") over the radiance buffer as it lies (after ptc_frame_resolve,
 *   ptc_comm_reduce_radiance or ptc_write_radiance_rgba32f) and the guides, into a separate RGBA32F buffer (alpha copied); the radiance buffer is not modified.
 *   Only class-1 pixels are filtered; misses and emitters are copied bit for bit.  params == NULL: the defaults.  PTC_E_STATE without valid guides; PTC_E_ARG for
 *   iterations outside 0..8 or a negative / non-finite sigma; iterations = 0 copies the radiance bit for bit.
 * ptc_select_output: which image ptc_read_radiance_rgba32f, ptc_read_radiance_rgba16f, ptc_radiance_rgba16f_device_ptr and ptc_tonemap_rgba8 serve.
 *   PTC_OUTPUT_RADIANCE by default and again after every ptc_frame_begin; PTC_OUTPUT_DENOISED before any ptc_denoise of the frame: PTC_E_STATE.
 *   ptc_radiance_device_ptr, ptc_write_radiance_rgba32f and ptc_comm_reduce_radiance always mean the radiance buffer.
 * ptc_get_denoise_seconds: HIP-event times of the last ptc_frame_guides and the last ptc_denoise (0 when there was none); either pointer may be NULL. */
enum { PTC_GUIDE_ALBEDO = 0, PTC_GUIDE_NORMAL_DEPTH = 1 };
enum { PTC_OUTPUT_RADIANCE = 0, PTC_OUTPUT_DENOISED = 1 };
typedef struct ptc_denoise_params {
  int iterations;     /* a-trous iterations, step 2^i: 0..8 (default 4)                                            */
  float sigma_l;      /* luminance: differences are measured in standard deviations of the local estimate (4)      */
  float sigma_n;      /* normal: exponent of max(0, Np.Nq) (128)                                                   */
  float sigma_p;      /* plane distance, in pixel footprints at the centre's depth (1)                             */
  int demodulate;     /* filter radiance / albedo and multiply the albedo back: keeps texture detail (1)           */
} ptc_denoise_params;
int ptc_frame_guides(ptc_ctx*);
int ptc_read_guide_rgba32f(ptc_ctx*, int which, float* out);       /* w*h*4 floats, full frame */
int ptc_read_guide_hit(ptc_ctx*, int32_t* prim, float* uv);        /* w*h primitive ids, w*h*2 barycentrics; either may be NULL */
void ptc_denoise_default_params(ptc_denoise_params*);
int ptc_denoise(ptc_ctx*, const ptc_denoise_params*);
int ptc_select_output(ptc_ctx*, int output);
int ptc_get_denoise_seconds(ptc_ctx*, double* guides, double* denoise);

/* ---- adaptive sampling: a per-pixel error estimate and batches of the pixels that still need samples ------------------------------
 * A uniform frame spends spp samples on every pixel, converged or not.  An adaptive frame keeps an ACTIVE SET of pixels — at first every owned pixel —
 * and ptc_frame_add_samples adds its samples to the active pixels only; ptc_frame_adapt takes out the pixels whose estimate has converged.  Nothing here
 * changes what a context that never calls ptc_frame_set_adaptive computes.  DESIGN.md ("Adaptive sampling") has the specification; in short, all in IEEE
 * binary32 in the order written:
 *   per owned pixel  the RGB sum, m1 = sum l_k and m2 = sum l_k l_k in sample order, l_k = (0.2126 r + 0.7152 g) + 0.0722 b of sample k's radiance, and
 *                    count, the samples received.  Every active pixel has count = the samples added so far.
 *   ptc_frame_adapt  queues what is held back, then with n = the samples added so far, per active pixel: mean = m1 / n, var = max(m2 / n - mean mean, 0),
 *                    e = sqrt(var / n) / (mean + 0.01), flag = e > threshold.  A pixel stays active iff n < spp_total and an active pixel within Chebyshev
 *                    distance `radius` — inside the image and inside the pixel's own 32x32 ownership tile — has its flag set.  A pixel that has left the set
 *                    never returns.  *n_active (may be NULL) receives the size of the new set.  One 4-byte read-back: the call waits for the device.
 *                    PTC_E_STATE before the frame's first sample.
 *   resolve          ptc_frame_resolve divides each pixel's sum by (float)count of that pixel.
 * The RNG is counter-based and a pixel's sum is taken in sample order, so a pixel with count n holds the bits of the same pixel of a uniform n-spp frame,
 * whatever its neighbours received; the neighbourhood stops at tile borders, so a tile-sharded adaptive frame is the unsharded one bit for bit.
 * ptc_frame_set_adaptive: right after a ptc_frame_begin with PTC_INTEGRATOR_PATH, before any sample, once per frame, and not after a
 *   ptc_frame_set_sample_range with a divisor: PTC_E_STATE otherwise.  params == NULL: the defaults.  PTC_E_ARG, and nothing changed, for a negative or non-finite threshold, a radius
 *   outside 0..2, min_samples or step_samples < 1.  In an adaptive frame ptc_frame_set_sample_range with a non-zero divisor, ptc_frame_checkpoint and
 *   ptc_frame_restore return PTC_E_STATE; with an empty active set ptc_frame_add_samples accepts and does nothing.  ptc_stats counts what was traced.
 *   Guides, denoiser, output selection, the read-backs and ptc_comm_reduce_radiance work on an adaptive frame as on any other; ptc_group_render is uniform.
 * ptc_read_sample_counts: w*h counts, 0 where this context does not own the pixel.  ptc_get_adaptive_stats: the frame's totals (both wait for the device).
 *   Both, like ptc_frame_adapt, return PTC_E_STATE in a frame that is not adaptive.
 * ptc_render_adaptive == frame_begin(max_spp) + set_adaptive + add(min_samples) + { adapt; add(min(step_samples, max_spp - done)) } until nothing is
 *   active + resolve + sync. */
typedef struct ptc_adaptive_params {
  float threshold;    /* relative standard error of the pixel mean's luminance (default 0.05) */
  int   radius;       /* 0..2, neighbourhood of the keep rule (default 1)                      */
  int   min_samples;  /* ptc_render_adaptive only: samples before the first decision (16)      */
  int   step_samples; /* ptc_render_adaptive only: samples between decisions (16)              */
} ptc_adaptive_params;
void ptc_adaptive_default_params(ptc_adaptive_params*);
int  ptc_frame_set_adaptive(ptc_ctx*, const ptc_adaptive_params*);  /* NULL: the defaults */
int  ptc_frame_adapt(ptc_ctx*, uint64_t* n_active);                 /* decision step; n_active may be NULL */
int  ptc_read_sample_counts(ptc_ctx*, uint32_t* out);               /* w*h, 0 where not owned */
int  ptc_render_adaptive(ptc_ctx*, int w, int h, int max_spp, uint64_t seed, int max_bounces,
                         const ptc_adaptive_params*);
typedef struct ptc_adaptive_stats {
  uint64_t owned_pixels, active_pixels, samples_total;   /* samples_total = sum of count */
  uint32_t passes, max_count;                            /* decision steps so far; the largest count */
  double   seconds_adapt;                                /* HIP-event time of the decision steps' kernels */
} ptc_adaptive_stats;
int  ptc_get_adaptive_stats(ptc_ctx*, ptc_adaptive_stats*);

/* ---- denoising from per-sample statistics: the per-pixel RGB covariance of an adaptive frame's samples ------------
 * ptc_denoise estimates a pixel's variance from the 7x7 window of the mean image; at tens of samples per pixel that window measures the signal, not the
 * noise.  An adaptive frame begun while ptc_set_sample_covariance is on also keeps, per owned pixel and in sample order, the six sums
 *   q_rr += r r, q_gg += g g, q_bb += b b, q_rg += r g, q_rb += r b, q_gb += g b            (24 B per owned pixel, zeroed at ptc_frame_set_adaptive)
 * of every sample's radiance (r, g, b).  Nothing else about the frame changes: image, counts and ptc_stats are those of the frame without them, bit for bit.
 * A uniform frame with statistics is an adaptive frame on which ptc_frame_adapt is never called.
 * ptc_denoise_sampled: per owned pixel with count n >= 1, sums s, fn = (float)n, w = (0.2126, 0.7152, 0.0722), albedo guide A, all in binary32 as written:
 *     mu_c = s_c / fn;   c_ij = q_ij / fn - mu_i mu_j;   a_c = w_c / max(A_c, 1e-3)  (a_c = w_c with demodulate = 0)
 *     V = ((a_r a_r) c_rr + (a_g a_g) c_gg) + (a_b a_b) c_bb + 2 (((a_r a_g) c_rg + (a_r a_b) c_rb) + (a_g a_b) c_gb);   Var_s = max(V, 0)
 *   the exact variance of the samples' (demodulated) luminance.  The filter is ptc_denoise_accumulated's with the input (D, fn), D = radiance / max(A, 1e-3)
 *   (or the radiance), and the variance (1 / fn) Var_s, the variance of the pixel mean, where n >= 4; elsewhere (fewer samples, pixels of another
 *   context's tiles) ptc_denoise's 7x7 estimate over lum(D).  The result goes to the denoised buffer (PTC_OUTPUT_DENOISED serves it), its time to
 *   ptc_get_denoise_seconds; the frame is not disturbed.  Parameters as ptc_denoise (NULL: the defaults; PTC_E_ARG alike; iterations = 0 copies the radiance).
 *   PTC_E_STATE without valid guides, in a frame that is not an adaptive frame keeping the covariance, and when samples were added since the last
 *   ptc_frame_resolve (the radiance buffer and the sums must describe the same samples).
 * ptc_set_sample_covariance: a setting of the context (it needs no device), 0 | 1, anything else PTC_E_ARG and the setting unchanged; default 0.  It is read
 *   by ptc_frame_set_adaptive (ptc_render_adaptive included): a frame keeps what it was begun with.
 * ptc_read_sample_covariance: the raw sums (rr, gg, bb, rg, rb, gb), 0 where this context does not own the pixel; waits for the device; PTC_E_STATE unless
 *   the current frame keeps the covariance.
 * ptc_read_sampled_variance: (Var_s, 1 / fn) as the frame's last ptc_denoise_sampled computed them, (0, 0) where count = 0; PTC_E_STATE before it. */
int  ptc_set_sample_covariance(ptc_ctx*, int on);
int  ptc_read_sample_covariance(ptc_ctx*, float* out);                /* w*h*6 floats */
int  ptc_denoise_sampled(ptc_ctx*, const ptc_denoise_params*);        /* NULL: the defaults */
int  ptc_read_sampled_variance(ptc_ctx*, float* out);                 /* w*h*2 floats */

/* ---- temporal accumulation: reproject the previous frame's accumulated image and blend the new frame in ---------------------------
 * A viewer that adds one sample per displayed frame starts every frame from nothing; these calls carry the previous frames' result across camera
 * motion, ptc_scene_refit and ptc_scene_rebuild.  Nothing here changes what a context that never calls them computes.  DESIGN.md §8c has the
 * specification; in short, per class-1 pixel: the hit point's position in the HISTORY's frame (the hit primitive's positions as they were then, at the
 * barycentrics of the guide hit) is projected through the history's camera; the four bilinear taps around it are valid where they lie inside the image,
 * are class 1, hold history (n > 0) and lie within sigma_z pixel footprints of the tap's plane (the history's normal, depth and position); the valid taps'
 * weighted mean H of the demodulated colour, of the luminance moments and of n is blended with this frame's D = radiance / max(albedo, 1e-3):
 * n_new = min(n + 1, max_history), a = 1 / n_new, D_new = (1 - a) H + a D.  Pixels of another class copy the radiance bit for bit.
 *
 * ptc_temporal_accumulate: needs valid guides of the current frame (PTC_E_STATE otherwise); reads the radiance buffer as it lies (after
 *   ptc_frame_resolve, ptc_comm_reduce_radiance or ptc_write_radiance_rgba32f) and never writes it; writes the accumulated image into a buffer of its own and
 *   replaces the context's history by this frame's state.  Queued on the context's stream; the frame in progress is not disturbed (sums, counts, held-back
 *   samples, ptc_stats, guides).  params == NULL: the defaults.  PTC_E_ARG, and nothing changed, for max_history outside 1..1024 or a negative or non-finite
 *   sigma_z.  A call refused with PTC_E_ARG or PTC_E_STATE leaves the history as it is; one that fails for lack of memory (PTC_E_NOMEM, PTC_E_DEVICE) drops it.
 * The history survives ptc_frame_begin, ptc_set_camera, ptc_scene_refit and ptc_scene_rebuild (and ptc_group_scene_refit).  ptc_temporal_reset, ptc_scene_begin
 *   (the scene whose shading records the history reads goes) and every commit — ptc_scene_commit, and ptc_group_scene_commit on every context of the group: new
 *   primitive ids — drop it; a frame of another size, or another `demodulate`, drops it silently at the next accumulate.  Without history every pixel is a
 *   first frame (n_new = 1).
 * ptc_select_output(PTC_OUTPUT_ACCUMULATED): the four read-backs serve the accumulated image; PTC_E_STATE before the frame's first ptc_temporal_accumulate.
 * ptc_denoise_accumulated: ptc_denoise's iterations over the accumulated image into the denoised buffer (PTC_OUTPUT_DENOISED then serves it); the variance
 *   is a Var_t, the variance of the accumulated mean, where n_new >= 4, and the 7x7 spatial estimate over lum(D_new) elsewhere.  PTC_E_STATE before the frame's
 *   accumulate, PTC_E_ARG if params->demodulate differs from the accumulate's (and for what ptc_denoise refuses).
 * ptc_read_temporal_rgba32f: the state the last accumulate left, w*h*4 floats each, w x h the size of the frame it accumulated: PTC_TEMPORAL_HISTORY (D_new.rgb, n_new), PTC_TEMPORAL_MOMENTS
 *   (m1, m2, Var_t, a), PTC_TEMPORAL_MOTION (x_prev, y_prev, W, reprojected n; zeros without history or behind the history's camera), and the two guide copies
 *   the history keeps of its frame, PTC_TEMPORAL_NORMAL_DEPTH (N, Z) and PTC_TEMPORAL_POSITION_CLASS (P, K).  PTC_E_STATE without history, and
 *   when a ptc_frame_begin with another size came after the accumulate (the history is then of a size the caller's buffer is not: accumulate first).
 * ptc_get_temporal_seconds: HIP-event time of the last ptc_temporal_accumulate (0 when there was none). */
enum { PTC_OUTPUT_ACCUMULATED = 2 };
enum { PTC_TEMPORAL_HISTORY = 0,   /* (D.rgb, n)                         */
       PTC_TEMPORAL_MOMENTS = 1,   /* (m1, m2, Var_t, a)                 */
       PTC_TEMPORAL_MOTION  = 2,   /* (x_prev, y_prev, W, n_reprojected) */
       PTC_TEMPORAL_NORMAL_DEPTH = 3,     /* the history's copy of its frame's (N, Z) guide */
       PTC_TEMPORAL_POSITION_CLASS = 4 }; /* the history's copy of its frame's (P, K)       */
typedef struct ptc_temporal_params {
  int   max_history;  /* 1..1024 (default 32)                                          */
  float sigma_z;      /* plane tolerance of a history tap, in pixel footprints (1)     */
  int   demodulate;   /* accumulate radiance / albedo (1)                              */
} ptc_temporal_params;
void ptc_temporal_default_params(ptc_temporal_params*);
int  ptc_temporal_accumulate(ptc_ctx*, const ptc_temporal_params*);   /* NULL: the defaults */
int  ptc_temporal_reset(ptc_ctx*);
int  ptc_read_temporal_rgba32f(ptc_ctx*, int which, float* out);      /* w*h*4 floats, w x h of the current (= the accumulated) frame */
int  ptc_denoise_accumulated(ptc_ctx*, const ptc_denoise_params*);    /* NULL: the defaults */
int  ptc_get_temporal_seconds(ptc_ctx*, double* accumulate);

/* ---- display transform: metered exposure, tone-mapping operators, transfer functions (csrc/pt_display.h) -----------
 * The images above are scene-referred radiance in physical units: a sun of 100 000 lx is worth 100 000.  ptc_tonemap_rgba8 and the RGBA16F read-backs take that
 * radiance as it is (they ignore everything here); these calls expose it first.  Nothing here changes what a context that never calls them computes, and nothing
 * here writes the radiance, denoised or accumulated buffers, the frame's sums, its ptc_stats or the temporal history.
 *
 * ptc_set_display: a setting of the context (it needs no device), kept across ptc_scene_begin.  NULL: the defaults.  PTC_E_ARG, and nothing changed, for a value
 *   outside the ranges in the struct's comments.
 * ptc_meter_exposure: meters the image ptc_select_output serves — radiance, denoised or accumulated — on the context's stream behind whatever wrote it, and
 *   returns without waiting.  A pixel's luminance is l = (0.2126 r + 0.7152 g) + 0.0722 b; pixels with alpha > 0 and a finite l > 0 are metered, pixels with
 *   alpha > 0 and any other l are counted as rejected, the others are not counted.  The metered luminance is the trimmed mean, between the two percentiles, of a
 *   piecewise-linear log2 of l over a histogram of 4096 bins, 16 per stop, in integers (csrc/pt_display.h has the definition): exact, whatever order the device
 *   adds in.  The adaptation state then moves towards it by adapt_rate (1: follows at once; the first metering after a reset always does).  A metering without
 *   metered pixels leaves the state alone.  The state survives ptc_frame_begin, ptc_set_camera, refit, rebuild and commit; ptc_exposure_reset and ptc_scene_begin
 *   drop it.
 * ptc_display_rgba8 / ptc_display_rgba16f: the served image times the exposure scale E — gain (key / clamp(adapted luminance, min_luminance, max_luminance))
 *   with auto_exposure on and an adaptation state, gain otherwise — through the operator and the transfer function to RGBA8 (alpha: clamp and quantisation only),
 *   or converted to RGBA16F as ptc_read_radiance_rgba16f converts (no operator, no transfer function: what a viewer's own tonemapper consumes; a NaN becomes
 *   0x7e00).  The kernels read the adaptation state from device memory: ptc_meter_exposure followed by a display call needs no wait in between.  With the defaults
 *   ptc_display_rgba8 writes ptc_tonemap_rgba8's bytes.  ptc_display_rgba16f_device_ptr: the device-pointer form, valid until the next RGBA16F display call.
 * ptc_get_exposure: waits for the device; the scale E a display call would use now, the adapted luminance (the state as a float, before the clamp; 0: none), the
 *   last metering's luminance, its metered and rejected pixel counts.  Any pointer may be NULL.
 * ptc_read_luminance_histogram: the 4096 bins of the last metering (waits); bin k counts the pixels with bits(l) >> 19 == k.
 * ptc_get_display_seconds: HIP-event times of the last metering and the last display kernel (0 when there was none); either pointer may be NULL.
 * The device calls return PTC_E_DEVICE on a description-only context and PTC_E_STATE before anything is rendered. */
enum { PTC_TONEMAP_ACES = 0,         /* the ACES fit of ptc_tonemap_rgba8 */
       PTC_TONEMAP_PBR_NEUTRAL = 1,  /* Khronos PBR Neutral, the glTF sample viewer's operator */
       PTC_TONEMAP_REINHARD = 2,     /* extended Reinhard on luminance, `white` maps to 1 */
       PTC_TONEMAP_CLAMP = 3 };      /* none */
enum { PTC_OETF_GAMMA22 = 0, PTC_OETF_SRGB = 1 };
typedef struct ptc_display_params {
  float gain;            /* linear exposure multiplier, finite, > 0 (1)            */
  int   auto_exposure;   /* 0 | 1 (0)                                              */
  float key;             /* metered luminance is mapped to this, > 0 (0.18)        */
  float percentile_lo;   /* [0, 1), < percentile_hi (0.1)                          */
  float percentile_hi;   /* (0, 1]  (0.9)                                          */
  float adapt_rate;      /* [0, 1]; 1 = follow at once (1)                         */
  float min_luminance;   /* clamp of the adapted luminance, > 0 (1e-4)             */
  float max_luminance;   /* >= min_luminance (1e6)                                 */
  int   tonemap;         /* PTC_TONEMAP_* (ACES)                                   */
  float white;           /* REINHARD only, > 0 (4)                                 */
  int   oetf;            /* PTC_OETF_* (GAMMA22)                                   */
} ptc_display_params;
void  ptc_display_default_params(ptc_display_params*);
int   ptc_set_display(ptc_ctx*, const ptc_display_params*);   /* NULL: the defaults */
int   ptc_get_display(const ptc_ctx*, ptc_display_params*);
int   ptc_meter_exposure(ptc_ctx*);                            /* asynchronous */
int   ptc_exposure_reset(ptc_ctx*);
int   ptc_get_exposure(ptc_ctx*, float* scale_E, float* adapted_luminance, float* metered_luminance, uint64_t* metered, uint64_t* rejected);
int   ptc_read_luminance_histogram(ptc_ctx*, uint32_t out[4096]);
int   ptc_display_rgba8(ptc_ctx*, uint8_t* out);
int   ptc_display_rgba16f(ptc_ctx*, uint16_t* out);
void* ptc_display_rgba16f_device_ptr(ptc_ctx*);
int   ptc_get_display_seconds(ptc_ctx*, double* meter, double* display);

/* ---- light probes: path-traced radiance at arbitrary points as 9 spherical-harmonic coefficients per channel (csrc/pt_probes.h) ----
 * A probe answers "what light arrives at this point, from every direction": the path integrator's radiance L(w) over the whole sphere of directions around the
 * position, projected onto the real SH basis up to band 2 (world axes, no Condon-Shortley sign; k = 0 | y z x | xy yz 3z^2-1 xz x^2-y^2), so that
 * L(w) ~ sum_k coef_k Y_k(w).  ptc_sh9_irradiance turns the 27 floats into the irradiance on a surface with a given normal: what a rasterizer's lighting pass
 * multiplies by albedo / pi for baked diffuse global illumination.
 *
 * A probe frame is a frame of the path integrator with one "pixel" per probe: sample s of probe j leaves the probe's position in a direction uniform over the
 * sphere, drawn from the two jitter dimensions of the key path_key(seed, probe_index_base + j, s), and is traced and shaded as a camera path is — an emitter or
 * the environment seen directly counts in full.  ptc_probes_begin begins it and ends whatever frame was in progress; the next ptc_frame_begin leaves probe mode.
 * ptc_frame_add_samples (with its deferred batching), ptc_frame_reserve, ptc_frame_set_sample_range, ptc_sync and ptc_get_stats work as in any frame, and after
 * ptc_frame_resolve the radiance read-backs return an n_probes x 1 image: each probe's mean incoming radiance.  Every sum has one owner and runs in sample order:
 * the coefficients do not depend on how the samples were cut into calls, batches or lanes, and the probes [a, b) of a set rendered with probe_index_base = a
 * are bit for bit the probes [a, b) of the whole set.  Punctual lights are sampled at the bounces as always; the lens is ignored.
 * What a probe does not see: the direct term of a punctual light (a delta that no ray hits — a real-time engine evaluates those lights itself; their bounced
 *   light is in the probe), and whether it lies inside geometry.
 * ptc_probes_begin: positions_xyz holds 3 floats per probe.  PTC_E_ARG, and nothing changed, for a NULL pointer, n_probes outside 1..2^26, probe indices beyond
 *   32 bits, a non-finite position, spp_total < 1 or max_bounces < 0; then PTC_E_DEVICE on a description-only context, PTC_E_STATE before ptc_scene_commit.
 * ptc_probes_read_sh: n_probes * 27 floats laid out [probe][k][rgb]: queues what ptc_frame_add_samples held back, waits, and returns sums * (4 pi / N), N the
 *   samples accumulated or the resolve divisor of ptc_frame_set_sample_range (shards of a sample range then add up to the whole).  PTC_E_STATE outside a probe frame.
 * ptc_render_probes == ptc_probes_begin(base 0) + ptc_frame_add_samples(spp) + ptc_probes_read_sh.
 * Refused with PTC_E_STATE in a probe frame, which they leave untouched: ptc_frame_guides, ptc_set_sample_covariance(1) (the setting stays as it
 *   was; 0 is accepted), ptc_frame_set_adaptive and ptc_frame_adapt, the denoisers, ptc_temporal_accumulate, ptc_frame_checkpoint / _restore, ptc_comm_reduce_radiance,
 *   ptc_focus_distance_at_pixel, ptc_debug_camera_rays.
 * ptc_sh9_eval / ptc_sh9_irradiance: pure functions, no context; sh = 27 floats [k][rgb], direction and normal of unit length.  Radiance sum_k sh_k Y_k(dir);
 *   irradiance E(n) = sum_k A_l sh_k Y_k(n) with A_0 = pi, A_1 = 2 pi / 3, A_2 = pi / 4 (Ramamoorthi and Hanrahan 2001).  PTC_E_ARG for a NULL pointer. */
int ptc_probes_begin(ptc_ctx*, const float* positions_xyz, int n_probes, uint32_t probe_index_base, int spp_total, uint64_t seed, int max_bounces);
int ptc_probes_read_sh(ptc_ctx*, float* out);
int ptc_render_probes(ptc_ctx*, const float* positions_xyz, int n_probes, int spp, uint64_t seed, int max_bounces, float* out);
int ptc_sh9_eval(const float sh[27], const float dir[3], float out[3]);
int ptc_sh9_irradiance(const float sh[27], const float normal[3], float out[3]);

/* ---- multi-GPU: tiles shard over devices, one RCCL reduce brings the framebuffer to the root -----------
 * The reference has no multi-device path (one vk::Device, core/GpuHandle.cpp:94-101); this is BASELINE.json's
 * "independent pixel/sample tiles shard across the 8 GPUs of one node with an RCCL reduce onto rank 0".
 *
 * One process per GPU: rank 0 calls ptc_comm_unique_id and ships the 128 bytes to the other ranks by whatever channel
 * the host has (MPI, torch.distributed, a file); every rank then calls ptc_comm_init on its context (collective:
 * ncclCommInitRank), renders its tiles (ptc_frame_begin with tile_rank/tile_count) and, after ptc_frame_resolve,
 * ptc_comm_reduce_radiance(root): ncclReduce(fp32, sum) in place on the full-frame radiance buffer, queued on the
 * context's stream behind the resolve (asynchronous; ptc_sync or a read-back waits for it).  Tiles are disjoint and the
 * other pixels are zero, so the sum is x + 0: the root's image is bit-identical to the single-GPU image. */
#define PTC_COMM_ID_BYTES 128
int ptc_comm_unique_id(uint8_t out[PTC_COMM_ID_BYTES]);
int ptc_comm_init(ptc_ctx*, const uint8_t id[PTC_COMM_ID_BYTES], int rank, int n_ranks);
int ptc_comm_reduce_radiance(ptc_ctx*, int root);
int ptc_comm_destroy(ptc_ctx*);

/* One process driving several GPUs: n contexts (one per device id) + ncclCommInitAll.  Describe and commit the same
 * scene on every ptc_group_ctx(g, i); ptc_group_render then traces device i's tiles on device i (all devices are queued
 * before anything is waited for), reduces onto device 0 and syncs: ptc_group_ctx(g, 0) holds the whole frame
 * (ptc_read_radiance_* / ptc_tonemap_rgba8 on it).  ptc_group_create returns NULL on failure (ptc_group_last_error(NULL)). */
typedef struct ptc_group ptc_group;
ptc_group* ptc_group_create(const int* device_ids, int n_devices);   /* every id PTC_DEVICE_NONE: a description-only group (no GPU, no RCCL): the host half of the group calls */
int ptc_group_size(const ptc_group*);
/* Commit ONE scene to every device of the group: the scene is described on ptc_group_ctx(g, 0) only; this call flattens it and
 * builds the BVH once on the host (unless device 0 has committed it already: that build is then used) and uploads that one build to
 * every device (N contexts committing on their own would each repeat the build, one after the other on the calling thread). */
int ptc_group_scene_commit(ptc_group*);
/* Scene dynamics for a group: ptc_update_instance* on ptc_group_ctx(g, 0), then every device refits its copy in place (or, on the
 * host path, ONE refit on the host whose arrays go to every device). */
int ptc_group_scene_refit(ptc_group*);
ptc_ctx* ptc_group_ctx(ptc_group*, int i);
int ptc_group_render(ptc_group*, int w, int h, int spp, uint64_t seed, int max_bounces, int integrator);
const char* ptc_group_last_error(const ptc_group*);
void ptc_group_destroy(ptc_group*);

/* ---- test hooks (parity of single stages; not needed by a renderer) -------------------------
 * Closest-hit of n explicit rays through the same trace kernel: origins/dirs are n*3 floats;
 * out_t n floats (t, or -1 on miss), out_prim n int32 (original primitive id or -1),
 * out_uv n*2 floats. */
int ptc_debug_trace_closest(ptc_ctx*, const float* origins, const float* dirs, uint32_t n,
                            float* out_t, int32_t* out_prim, float* out_uv);
/* Any-hit of n explicit rays with tmax each; out_occluded n uint8. */
int ptc_debug_trace_any(ptc_ctx*, const float* origins, const float* dirs, const float* tmax,
                        uint32_t n, uint8_t* out_occluded);
/* The aperture point (lx, ly) that the lens selects for the pair (u1, u2) in [0,1)^2: a pure host evaluation of csrc/pt_lens.h, no context.
 * PTC_E_ARG for a null pointer, lens parameters ptc_set_camera_lens would refuse, or u outside [0, 1). */
int ptc_debug_lens_sample(const ptc_lens_params*, float u1, float u2, float out_xy[2]);
/* Punctual lights (csrc/pt_lights.h).
 * ptc_debug_light_sample: the host evaluation of pt_light_sample for one light and one point P, no context: unit direction towards the light, the distance
 *   (3.0e38 for a directional light) and the arriving radiance.  Returns 1 when there is a sample, 0 when there is none (P on the light; outputs untouched),
 *   PTC_E_ARG for a null pointer or parameters ptc_add_light would refuse.
 * ptc_debug_get_light_table: the 64-byte records (16 floats per light: position, type as int bits | direction, range | intensity, pmf | spot scale, spot
 *   offset, cos_inner, cos_outer) and the cdf (one float per light) as ptc_frame_begin uploads them for the lights recorded now.  Arrays may be NULL (count only).
 *   Works on a description-only context.
 * ptc_debug_punctual_nee: n explicit rays in identity layout with throughput 1, path id = index and the given RNG keys through k_trace_closest and then
 *   k_shade_punctual at `bounce`, with the lights recorded now (at least one: PTC_E_STATE otherwise).  Per ray: out_valid 1 if it produced a shadow record, and
 *   that record — origin (3), direction (3), tmax, contribution (3); records are matched by the path id they carry.  Preconditions and side effects as
 *   ptc_debug_trace_closest. */
int ptc_debug_light_sample(const ptc_light_params*, const float P[3], float out_wi[3], float* out_dist, float out_Li[3]);
int ptc_debug_get_light_table(ptc_ctx*, uint32_t* n_lights, float* records, float* cdf);
int ptc_debug_punctual_nee(ptc_ctx*, const float* origins, const float* dirs, const uint32_t* keys, uint32_t n, uint32_t bounce,
                           uint8_t* out_valid, float* out_origin, float* out_dir, float* out_tmax, float* out_contrib);
/* The display transform (csrc/pt_display.h).  The first two are pure host evaluations of the header and need no context.
 * ptc_debug_display_pixel: one RGBA pixel at the exposure scale E through the operator and transfer function of params (NULL: the defaults): the four RGBA8
 *   bytes and the four RGBA16F values.  Either output may be NULL.  PTC_E_ARG for a null input or parameters ptc_set_display would refuse.
 * ptc_debug_meter: a metering of n_pixels RGBA pixels (at most 2^28) from the adaptation state state_in: the new state, Q, the metered pixels N, the pixels the
 *   trim kept M, the rejected pixels and the histogram.  Every output may be NULL.
 * ptc_debug_display_internals: [0] the pixels one pass of k_meter_hist's grid covers (an image with more takes a second pass of the grid-stride loop), [1] the
 *   same for the display kernels, 0: they are not grid-stride, [2], [3] 0.
 *   Works on a description-only context.
 * ptc_debug_display_state: waits; the state record in device memory, out[0..4] = A, Q, N, M, rejected (zeros before the first metering). */
int ptc_debug_display_pixel(const ptc_display_params*, float E, const float rgba_in[4], uint8_t out8[4], uint16_t out16[4]);
int ptc_debug_meter(const ptc_display_params*, const float* rgba, uint64_t n_pixels, uint32_t state_in, uint32_t* state_out, uint32_t* Q, uint64_t* N, uint64_t* M,
                    uint64_t* rejected, uint32_t hist[4096]);
int ptc_debug_display_internals(ptc_ctx*, uint64_t out[4]);
int ptc_debug_display_state(ptc_ctx*, uint32_t out[8]);
/* The camera rays of the path integrator for n_pixels pixels (indices y*w+x of a w x h frame) and the samples first_sample .. first_sample + n_samples - 1,
 * with the context's camera and lens and the seed hashed as ptc_frame_begin hashes it: n_pixels * n_samples rays in path order, ray p = sample_local *
 * n_pixels + j, origins and dirs 3 floats each.  On a device context the launcher a batch would choose — k_raygen for R = 0, the lens kernel otherwise —
 * writes lane 0's ray queue, which is read back; same preconditions and side effects as ptc_debug_trace_closest (committed scene; ends the frame).  On a
 * description-only context (a camera must have been set) the host evaluates csrc/pt_lens.h, which restates the pinhole ray for R = 0. */
int ptc_debug_camera_rays(ptc_ctx*, int w, int h, uint64_t seed, uint32_t first_sample, uint32_t n_samples, const uint32_t* pixels, uint32_t n_pixels,
                          float* origins, float* dirs);
/* Light probes (csrc/pt_probes.h).  On a description-only context the host evaluates the header; on a device context the kernels run on lane 0's queues
 * (any frame in progress ends; no scene is needed).  Paths are in batch order: path p = sample_local * n_probes + j.
 * ptc_debug_probe_rays: the rays k_raygen_probe writes for the samples first_sample .. first_sample + n_samples - 1: 6 floats per path (origin, direction) and
 *   the path's RNG key.
 * ptc_debug_probe_project: k_accumulate_sh's step: acc_inout (n_probes * 27 running sums) += the projection of lpath_rgba (4 floats per path, alpha unused).
 * ptc_debug_probe_resolve: the resolve of ptc_probes_read_sh, out = acc * (4 pi / n_samples); no context.
 * PTC_E_ARG for a NULL pointer, n_probes outside 1..2^26, n_samples = 0, more than 2^31 - 1 paths, sample or probe indices beyond 32 bits. */
int ptc_debug_probe_rays(ptc_ctx*, const float* positions_xyz, int n_probes, uint32_t probe_index_base, uint64_t seed, uint32_t first_sample, uint32_t n_samples,
                         float* out_o_d, uint32_t* out_key);
int ptc_debug_probe_project(ptc_ctx*, int n_probes, uint32_t probe_index_base, uint64_t seed, uint32_t first_sample, uint32_t n_samples, const float* lpath_rgba,
                            float* acc_inout);
int ptc_debug_probe_resolve(const float* acc, int n_probes, uint32_t n_samples, float* out);
/* World-space flattened geometry as committed: verts (n_verts*12 floats = ptc_vertex),
 * indices (n_tris*3 u32), per-triangle material.  Pass NULL to query sizes only. */
int ptc_debug_get_flat_scene(ptc_ctx*, uint32_t* n_verts, uint32_t* n_tris, ptc_vertex* verts,
                             uint32_t* indices, int32_t* tri_material);
/* The current posed object-space vertices of mesh `mesh` (n_verts of the mesh).  On a committed scene that is the LIVE pose, the one the
 * last commit, refit or rebuild applied: a pose that is only recorded, or that a refit refused, does not show.  They are read from HBM
 * when the kernel evaluated them there (ptc_debug_get_internals [7] bit 3 then says so); else the host evaluates them.  Before the first
 * commit: the host's evaluation of the recorded pose. */
int ptc_debug_get_mesh_vertices(ptc_ctx*, int mesh, ptc_vertex* out);

/* The scene description as received (valid from ptc_scene_begin on, committed or not): number of materials and
 * textures; material i as 12 values (base rgba, metallic, roughness, emissive rgb as floats; tex_color, tex_normal,
 * tex_mr as ints); texture i's size and, when rgba is non-NULL, its w*h*4 bytes. */
int ptc_debug_get_description(ptc_ctx*, int* n_materials, int* n_textures);
int ptc_debug_get_material(ptc_ctx*, int index, float out_factors[9], int out_textures[3]);
int ptc_debug_get_texture(ptc_ctx*, int index, int* w, int* h, uint8_t* rgba);

/* Raw device counter array of the current frame (segments, shadow rays, hits, node/triangle counts, then the
 * loop-iteration diagnostics that only an instrumented build fills: profiles/instr_diag.patch, built with EXTRA=-DPT_DIAG).  Returns the number of counters the library keeps. */
int ptc_debug_get_counters(ptc_ctx*, uint64_t* out, int n);

/* The flattened 8-wide BVH as committed: ONE array of n_units 16-byte units (n_units*4 32-bit words) holding 64-byte nodes
 * (origin on a 16-bit grid over the scene box, exponents, interior / leaf slot masks, the unit address of the children block,
 * 8-bit quantised child planes of the 8 slots) and 48-byte triangle records (v0,prim | e1,class | e2,0) inside the children
 * blocks; the root is the node at unit 0 (layout in csrc/ptc_scene.cpp).  grid: scene_lo.xyz, step.xyz of the origin grid.
 * Pass NULL to query sizes only. */
int ptc_debug_get_bvh(ptc_ctx*, uint32_t* n_nodes, uint32_t* n_tris, uint32_t* n_units, float* units, float grid[6]);

/* Identity (an address, as a number) of the host build the context renders from.  The contexts of a ptc_group share ONE build after
 * ptc_group_scene_commit / ptc_group_scene_refit (one flatten + BVH build for N devices): equal values say so.  0 for a null context. */
uint64_t ptc_debug_host_build_id(const ptc_ctx*);
/* Context internals for tests of the host logic: [0] HIP events created so far, [1] timing spans waiting to be
 * collected, [2] queue capacity (paths) of a lane, [3] samples of one full batch, [4] samples accepted but not yet
 * issued, [5] trace blocks per CU, [6] stack entries per lane kept in LDS, [7] bit 0: the last ptc_scene_refit ran on the
 * device (csrc/pt_refit.hip), not on the host; bit 1: the last ptc_scene_commit flattened and built on the device
 * (csrc/pt_refit.hip + csrc/pt_build.hip: the LBVH builder on a device context, or the SAH builder with the SAH device builder); bit 2: the
 * tree now in HBM was built on the device by the SAH front end (ptc_set_device_builder); bit 3: the last ptc_debug_get_mesh_vertices
 * read the mesh's slice in HBM, where csrc/pt_deform.hip had written it. */
int ptc_debug_get_internals(ptc_ctx*, uint64_t out[8]);

/* The host's share of a commit ON THE DEVICE (the LBVH builder on a device context: indices and material per primitive, materials, the emitter table from the
 * emissive primitives alone, textures, environment tables — no flatten), computed again for the committed description and held against the host build, without a device.
 * out: [0] primitives, [1] emitters, [2] indices + material per primitive agree, [3] emitter index per primitive, emitter table and cdf agree bit for bit, [4] material table,
 * [5] textures / texture sets / environment tables, [6] shading-record stride and vertex count — 1 each when equal. */
int ptc_debug_commit_host_parts(ptc_ctx*, uint64_t out[8]);

/* The tables shading reads besides the BVH, as they lie in HBM: the per-primitive shading records (4 * stride floats each,
 * stride 5 or 12), the emitters (20 floats each) and their power cdf (max(n_lights, 1) floats).  Arrays may be NULL (sizes only).
 * With ptc_debug_get_bvh this is everything a refit rewrites: the tests hold the refit on the device against the one on the
 * host and the oracle's through these two calls. */
int ptc_debug_get_shading_tables(ptc_ctx*, uint32_t* stride, float* shade, uint32_t* n_lights, float* lights, float* cdf);

/* The HOST's share of a refit on the device, runnable without one (CPU tests, sanitizer builds): the plan of the committed scene (vertex ->
 * instance, node addresses by level) and the emitter table of the current transforms from the emissive primitives alone, checked against the
 * host build; call it after ptc_scene_refit on a description-only context.  out: [0] world vertices, [1] primitives, [2] nodes in the level
 * lists, [3] levels, [4] primitives with an emissive material, [5] 1 if the lists hold every node once with children in earlier levels,
 * [6] 1 if emitter table and cdf equal the host refit's bit for bit, [7] 1 if every instance transform is finite. */
int ptc_debug_refit_host_parts(ptc_ctx*, uint64_t out[8]);

#ifdef __cplusplus
}
#endif
#include "ptc_alpha.h"   /* alpha coverage: an extension with a header and a symbol prefix of its own */
#include "ptc_glass.h"   /* dielectric transmission: likewise */
#include "ptc_glass_shadows.h"   /* transparent shadows through thin glass: likewise */
#include "ptc_shade_debug.h"   /* test hooks around k_shade: likewise */
#include "ptc_exact_debug.h"   /* test hook for the exact fast paths of division and square root: likewise */
#include "ptc_medium.h"   /* a homogeneous participating medium: likewise */
#include "ptc_lightmap.h"   /* lightmaps, irradiance over an instance's UV atlas: likewise */
#include "ptc_emissive_tex.h"   /* textured emission, glTF emissiveTexture as a light set of its own: likewise */
#include "ptc_camera.h"   /* camera models, a camera-to-world matrix with a perspective, orthographic or equirectangular projection: likewise */
#endif /* PTC_H */
