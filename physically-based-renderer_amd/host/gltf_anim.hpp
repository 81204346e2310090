// gltf_anim.hpp — the glTF asset as a HANDLE: skins, morph targets and animations on top of gltf_loader.hpp (include/ptc_gltf.h, ptc_gltf_open ...).
//
// pbr::gltf::load stays what it is: stateless, bind pose.  An Asset keeps the parsed document, so that a caller can pose the scene it loaded:
//   load_into   the scene's materials, textures and primitives as load() reads them; ONE ptc mesh per (primitive, skin) pair — and per node for a
//               primitive that deforms, because a pose belongs to a mesh — with `targets` (+ mesh / node `weights`) through ptc_mesh_set_morph_targets and
//               JOINTS_0 (u8 / u16) + WEIGHTS_0 (float, normalised u8 / u16) through ptc_mesh_set_skin; instances in load()'s order
//   pose        node transforms at time t of an animation (channels translation / rotation / scale / weights; samplers LINEAR and STEP, rotations by slerp;
//               CUBICSPLINE is sampled LINEARLY over its value entries, its tangents are not used), t clamped to the animation's range; then
//               ptc_update_instance_matrix for every instance and ptc_update_mesh_pose for every deforming mesh, with the joint matrices
//               inverse(global(mesh node)) global(joint) inverseBind.  The caller refits or rebuilds (or commits).  KHR_lights_punctual lights follow their nodes
//               through ptc_update_light.
//   camera      the ptc_camera_params of camera node `index` (the scene's camera nodes in the order load() reaches them) at rest or at time t of an animation:
//               the node's world matrix as pose composes the instance matrices, so a camera on an animated node flies.  Needs no context and no load_into.
// Node matrices for the instances are composed in binary32 exactly as load() composes them; joint matrices are composed in binary64 and rounded once.
#pragma once
#include "gltf_loader.hpp"

#include <algorithm>
#include <memory>

namespace pbr::gltf {

class Asset {
public:
  explicit Asset(const std::string& path) : path_(path), doc_(detail::open(path)) {
    const auto& nodes = doc_.root.array("nodes");
    parent_.assign(nodes.size(), -1);
    for (size_t i = 0; i < nodes.size(); ++i)
      for (const JValue& c : nodes[i].array("children")) {
        const long k = (long)c.num;
        if (k < 0 || (size_t)k >= nodes.size()) throw std::runtime_error("node index out of range");
        parent_[(size_t)k] = (long)i;
      }
    for (const JValue& a : doc_.root.array("animations")) anims_.push_back(read_animation(a));
  }

  int animations() const { return (int)anims_.size(); }
  double duration(int a) const { return a >= 0 && (size_t)a < anims_.size() ? (double)anims_[(size_t)a].t_max : -1.0; }

  // between ptc_scene_begin and ptc_scene_commit.  Returns the number of triangles instanced, or a negative PTC_E_* code (ptc_last_error has the text).
  long long load_into(ptc_ctx* ctx, int scene_index, bool compose_parents, float bbox6[6]) {
    using namespace detail;
    const FlatScene fs = load(path_, scene_index, compose_parents);
    compose_ = compose_parents; scene_ = scene_index;
    insts_.clear(); meshes_.clear(); lights_.clear();
    std::vector<int> tex_id, mat_id;
    for (const Texture& t : fs.textures) { const int id = ptc_add_texture_rgba8(ctx, t.rgba.data(), t.w, t.h); if (id < 0) return id; tex_id.push_back(id); }
    for (const Material& m : fs.materials) {
      const int id = add_material(ctx, m, tex_id);
      if (id < 0) return id;
      mat_id.push_back(id);
    }
    // primitive index (FlatScene order: mesh order, then primitive order) -> its JSON
    std::vector<std::pair<int, int>> mesh_span;
    std::vector<std::pair<const JValue*, const JValue*>> prim_json;     // (mesh, primitive)
    for (const JValue& mesh : doc_.root.array("meshes")) {
      const int first = (int)prim_json.size();
      for (const JValue& prim : mesh.array("primitives")) prim_json.emplace_back(&mesh, &prim);
      mesh_span.emplace_back(first, (int)prim_json.size() - first);
    }
    // the scene's nodes in load()'s order (depth-first, children before the node's own mesh)
    const auto& nodes = doc_.root.array("nodes");
    const auto& scenes = doc_.root.array("scenes");
    const long si = scene_index >= 0 ? scene_index : doc_.root.integer("scene", 0);
    std::vector<long> order;
    for (const JValue& r : scenes[(size_t)si].array("nodes")) walk((long)r.num, 0, order);
    const Pose bind = sample(-1, 0.0);
    size_t at = 0;
    for (long n : order) {
      const long mesh = nodes[(size_t)n].integer("mesh", -1);
      if (mesh < 0) continue;
      const long skin = nodes[(size_t)n].integer("skin", -1);
      for (int k = 0; k < mesh_span[(size_t)mesh].second; ++k, ++at) {
        const int pi = mesh_span[(size_t)mesh].first + k;
        if (at >= fs.instances.size() || fs.instances[at].primitive != pi) throw std::runtime_error("asset: instance order differs from the loader's");
        const JValue& pj = *prim_json[(size_t)pi].second;
        const JValue* attrs = pj.get("attributes");
        const bool skinned = skin >= 0 && attrs && attrs->get("JOINTS_0") && attrs->get("WEIGHTS_0");
        const bool morphed = !pj.array("targets").empty();
        const std::array<long, 3> key = {pi, skinned ? skin : -1, (skinned || morphed) ? n : -1};
        int mi = -1;
        for (size_t j = 0; j < meshes_.size(); ++j) if (meshes_[j].key == key) mi = (int)j;
        if (mi < 0) {
          const Primitive& P = fs.primitives[(size_t)pi];
          MeshRec M;
          M.key = key; M.node = n; M.skin = skinned ? skin : -1;
          M.ptc_mesh = ptc_add_mesh(ctx, P.vertices.data(), (std::uint32_t)P.vertices.size(), P.indices.data(), (std::uint32_t)P.indices.size(), mat_id[(size_t)P.material]);
          if (M.ptc_mesh < 0) return M.ptc_mesh;
          const size_t nv = P.vertices.size();
          if (morphed) {
            const auto& targets = pj.array("targets");
            M.n_targets = (int)targets.size();
            std::vector<float> dp(targets.size() * nv * 3, 0.0f), dn, dt;
            for (size_t t = 0; t < targets.size(); ++t) {
              auto take = [&](const char* name, std::vector<float>& dst) {
                if (!targets[t].get(name)) return;
                const std::vector<float> d = doc_.floats(targets[t].integer(name, -1), 3);
                if (d.size() != nv * 3) throw std::runtime_error(std::string("morph target ") + name + " count differs from POSITION count");
                if (dst.empty()) dst.assign(targets.size() * nv * 3, 0.0f);
                std::copy(d.begin(), d.end(), dst.begin() + (long)(t * nv * 3));
              };
              take("POSITION", dp); take("NORMAL", dn); take("TANGENT", dt);
            }
            const int rc = ptc_mesh_set_morph_targets(ctx, M.ptc_mesh, (std::uint32_t)targets.size(), dp.data(), dn.empty() ? nullptr : dn.data(), dt.empty() ? nullptr : dt.data());
            if (rc < 0) return rc;
            const auto& mw = prim_json[(size_t)pi].first->array("weights");
            M.weights0.assign(targets.size(), 0.0f);
            for (size_t t = 0; t < targets.size() && t < mw.size(); ++t) M.weights0[t] = (float)mw[t].num;
          }
          if (skinned) {
            const auto& skins = doc_.root.array("skins");
            if ((size_t)skin >= skins.size()) throw std::runtime_error("skin index out of range");
            const JValue& S = skins[(size_t)skin];
            for (const JValue& j : S.array("joints")) {
              if ((long)j.num < 0 || (size_t)j.num >= nodes.size()) throw std::runtime_error("skin joint is not a node");
              M.joints.push_back((long)j.num);
            }
            if (M.joints.empty() || M.joints.size() > 65536) throw std::runtime_error("skin without joints (or with too many)");
            M.ibm.assign(M.joints.size() * 16, 0.0);
            for (size_t j = 0; j < M.joints.size(); ++j) for (int d = 0; d < 4; ++d) M.ibm[j * 16 + (size_t)d * 5] = 1.0;
            if (S.get("inverseBindMatrices")) {
              const std::vector<float> m = doc_.floats(S.integer("inverseBindMatrices", -1), 16);
              if (m.size() != M.joints.size() * 16) throw std::runtime_error("inverseBindMatrices count differs from the number of joints");
              for (size_t e = 0; e < m.size(); ++e) M.ibm[e] = (double)m[e];
            }
            const std::vector<float> jf = doc_.floats(attrs->integer("JOINTS_0", -1), 4), wf = doc_.floats(attrs->integer("WEIGHTS_0", -1), 4);
            if (jf.size() != nv * 4 || wf.size() != nv * 4) throw std::runtime_error("JOINTS_0 / WEIGHTS_0 count differs from POSITION count");
            std::vector<std::uint16_t> ju(nv * 4);
            for (size_t e = 0; e < ju.size(); ++e) {
              if (!(jf[e] >= 0.0f && jf[e] < (float)M.joints.size())) throw std::runtime_error("JOINTS_0 names a joint the skin does not have");
              ju[e] = (std::uint16_t)jf[e];
            }
            const int rc = ptc_mesh_set_skin(ctx, M.ptc_mesh, (std::uint32_t)M.joints.size(), ju.data(), wf.data());
            if (rc < 0) return rc;
          }
          meshes_.push_back(std::move(M));
          mi = (int)meshes_.size() - 1;
        }
        const int id = ptc_add_instance_matrix(ctx, meshes_[(size_t)mi].ptc_mesh, fs.instances[at].model.data());
        if (id < 0) return id;
        insts_.push_back({n, id});
      }
    }
    for (const Light& l : fs.lights) {      // KHR_lights_punctual: the lights move with their nodes (apply)
      const int id = ptc_add_light(ctx, &l.params);
      if (id < 0) return id;
      lights_.push_back({l.node, id, l.params});
    }
    { const int rc = apply(ctx, bind, /*instances=*/false); if (rc < 0) return rc; }      // the bind pose and the asset's default weights
    if (bbox6) for (int k = 0; k < 3; ++k) { bbox6[k] = fs.bbox_lo[k]; bbox6[3 + k] = fs.bbox_hi[k]; }
    return (long long)fs.n_triangles;
  }

  // node transforms of animation `a` at time t (clamped to its range) -> ptc_update_instance_matrix / ptc_update_mesh_pose
  int pose(ptc_ctx* ctx, int a, double t) {
    if (a < 0 || (size_t)a >= anims_.size()) return PTC_E_ARG;
    return apply(ctx, sample(a, t), /*instances=*/true);
  }

  // the camera nodes of the scene (load_into's, or the asset's default one), in load()'s order
  int cameras() const { return (int)camera_nodes().size(); }
  // animation < 0: the rest pose.  PTC_E_ARG: no such camera or animation
  int camera(int index, int a, double t, float frame_aspect, ptc_camera_params* out) const {
    const std::vector<long> cn = camera_nodes();
    if (!out || index < 0 || (size_t)index >= cn.size() || a >= (int)anims_.size()) return PTC_E_ARG;
    const long node = cn[(size_t)index];
    Camera c = detail::camera_def(doc_.root, doc_.root.array("nodes")[(size_t)node].integer("camera", -1));
    c.node = node; c.world = world32(sample(a < 0 ? -1 : a, t), node);
    detail::camera_params(c, frame_aspect, out);
    return PTC_OK;
  }

private:
  struct Channel { long node; int path; int interp; std::vector<float> times, values; int width; };      // path 0 T, 1 R, 2 S, 3 weights; interp 0 LINEAR, 1 STEP, 2 CUBICSPLINE
  struct Anim { std::vector<Channel> ch; float t_min = 0, t_max = 0; };
  struct MeshRec { std::array<long, 3> key; long node = -1, skin = -1; int ptc_mesh = -1, n_targets = 0; std::vector<long> joints; std::vector<double> ibm; std::vector<float> weights0; };
  struct InstRec { long node; int ptc_inst; };
  struct LightRec { long node; int ptc_light; ptc_light_params params; };
  struct Local { bool matrix = false; float m[16]; float t[3] = {0, 0, 0}, q[4] = {1, 0, 0, 0}, s[3] = {1, 1, 1}; };
  struct Pose { std::vector<Local> local; std::map<long, std::vector<float>> weights; };      // weights: per node with an animated `weights` channel

  std::string path_;
  detail::Doc doc_;
  std::vector<long> parent_;
  std::vector<Anim> anims_;
  std::vector<MeshRec> meshes_;
  std::vector<InstRec> insts_;
  std::vector<LightRec> lights_;
  bool compose_ = true;
  long scene_ = -1;      // the scene load_into read (-1: the asset's default)

  void walk_cameras(long n, int depth, std::vector<long>& out) const {      // pre-order: the order load()'s traversal first reaches the nodes
    const auto& nodes = doc_.root.array("nodes");
    if (n < 0 || (size_t)n >= nodes.size()) throw std::runtime_error("node index out of range");
    if (depth > 256) throw std::runtime_error("node hierarchy too deep (cycle?)");
    if (nodes[(size_t)n].integer("camera", -1) >= 0) out.push_back(n);
    for (const JValue& c : nodes[(size_t)n].array("children")) walk_cameras((long)c.num, depth + 1, out);
  }
  std::vector<long> camera_nodes() const {
    const auto& scenes = doc_.root.array("scenes");
    const long si = scene_ >= 0 ? scene_ : doc_.root.integer("scene", 0);
    if (si < 0 || (size_t)si >= scenes.size()) throw std::runtime_error("scene index out of range");
    std::vector<long> out;
    for (const JValue& r : scenes[(size_t)si].array("nodes")) walk_cameras((long)r.num, 0, out);
    return out;
  }

  void walk(long n, int depth, std::vector<long>& out) const {
    const auto& nodes = doc_.root.array("nodes");
    if (n < 0 || (size_t)n >= nodes.size()) throw std::runtime_error("node index out of range");
    if (depth > 256) throw std::runtime_error("node hierarchy too deep (cycle?)");
    for (const JValue& c : nodes[(size_t)n].array("children")) walk((long)c.num, depth + 1, out);
    out.push_back(n);
  }

  Anim read_animation(const JValue& a) const {
    Anim A;
    const auto& samplers = a.array("samplers");
    bool first = true;
    for (const JValue& c : a.array("channels")) {
      const JValue* tg = c.get("target");
      const long s = c.integer("sampler", -1);
      if (!tg || s < 0 || (size_t)s >= samplers.size()) throw std::runtime_error("animation channel without target or sampler");
      if (!tg->get("node")) continue;      // a channel without a node is ignored (glTF 2.0 §5.5)
      Channel ch;
      ch.node = tg->integer("node", -1);
      if (ch.node < 0 || (size_t)ch.node >= parent_.size()) throw std::runtime_error("animation targets a node that does not exist");
      const std::string p = tg->string("path");
      ch.path = p == "translation" ? 0 : p == "rotation" ? 1 : p == "scale" ? 2 : p == "weights" ? 3 : -1;
      if (ch.path < 0) continue;
      const std::string ip = samplers[(size_t)s].string("interpolation", "LINEAR");
      ch.interp = ip == "STEP" ? 1 : ip == "CUBICSPLINE" ? 2 : 0;
      ch.times = doc_.floats(samplers[(size_t)s].integer("input", -1), 1);
      const long out = samplers[(size_t)s].integer("output", -1);
      const int comps = ch.path == 1 ? 4 : ch.path == 3 ? 1 : 3;
      ch.values = doc_.floats(out, comps);
      if (ch.times.empty()) throw std::runtime_error("animation sampler without keys");
      for (size_t k = 1; k < ch.times.size(); ++k) if (!(ch.times[k] > ch.times[k - 1])) throw std::runtime_error("animation sampler times must increase");
      const size_t per_key = ch.values.size() / ch.times.size();      // weights: targets per key; CUBICSPLINE: three entries per key
      if (per_key * ch.times.size() != ch.values.size() || per_key == 0) throw std::runtime_error("animation sampler output does not match its input");
      ch.width = (int)per_key;
      if (first) { A.t_min = ch.times.front(); A.t_max = ch.times.back(); first = false; }
      A.t_min = std::min(A.t_min, ch.times.front()); A.t_max = std::max(A.t_max, ch.times.back());
      A.ch.push_back(std::move(ch));
    }
    return A;
  }

  // the value of a channel at time t: `n` floats (the value entries of a CUBICSPLINE sampler are sampled linearly)
  static void channel_value(const Channel& c, float t, float* out, int n) {
    const int entries = c.interp == 2 ? 3 : 1;
    const int stride = c.width;                       // floats per key
    const int off = c.interp == 2 ? n : 0;            // (in-tangent, VALUE, out-tangent)
    if (stride != n * entries) throw std::runtime_error("animation sampler output has the wrong width for its target");
    size_t k = 0;
    while (k + 1 < c.times.size() && t >= c.times[k + 1]) ++k;
    const float* a = &c.values[k * (size_t)stride + (size_t)off];
    if (k + 1 >= c.times.size() || t <= c.times[k] || c.interp == 1) { for (int i = 0; i < n; ++i) out[i] = a[i]; return; }
    const float* b = &c.values[(k + 1) * (size_t)stride + (size_t)off];
    const float u = (t - c.times[k]) / (c.times[k + 1] - c.times[k]);
    if (c.path == 1) {      // slerp along the shorter arc
      double d = 0.0;
      for (int i = 0; i < 4; ++i) d += (double)a[i] * (double)b[i];
      const double sgn = d < 0.0 ? -1.0 : 1.0;
      d = std::fabs(d);
      double wa = 1.0 - (double)u, wb = (double)u;
      if (d < 0.9995) { const double th = std::acos(d), sn = std::sin(th); wa = std::sin((1.0 - (double)u) * th) / sn; wb = std::sin((double)u * th) / sn; }
      double q[4], l = 0.0;
      for (int i = 0; i < 4; ++i) { q[i] = wa * (double)a[i] + wb * sgn * (double)b[i]; l += q[i] * q[i]; }
      l = std::sqrt(l);
      for (int i = 0; i < 4; ++i) out[i] = (float)(q[i] / l);
      return;
    }
    for (int i = 0; i < n; ++i) out[i] = a[i] + u * (b[i] - a[i]);
  }

  Pose sample(int a, double time) const {
    const auto& nodes = doc_.root.array("nodes");
    Pose P;
    P.local.resize(nodes.size());
    for (size_t i = 0; i < nodes.size(); ++i) {
      const JValue& n = nodes[i];
      Local& L = P.local[i];
      const auto& mtx = n.array("matrix");
      if (mtx.size() == 16) { L.matrix = true; for (int k = 0; k < 16; ++k) L.m[k] = (float)mtx[(size_t)k].num; continue; }
      const auto& T = n.array("translation"); const auto& R = n.array("rotation"); const auto& S = n.array("scale");
      for (size_t k = 0; k < 3 && k < T.size(); ++k) L.t[k] = (float)T[k].num;
      if (R.size() == 4) { L.q[0] = (float)R[3].num; L.q[1] = (float)R[0].num; L.q[2] = (float)R[1].num; L.q[3] = (float)R[2].num; }
      for (size_t k = 0; k < 3 && k < S.size(); ++k) L.s[k] = (float)S[k].num;
      const auto& W = n.array("weights");
      if (!W.empty()) { std::vector<float>& w = P.weights[(long)i]; for (const JValue& x : W) w.push_back((float)x.num); }
    }
    if (a < 0) return P;
    const Anim& A = anims_[(size_t)a];
    const float t = (float)std::min(std::max(time, (double)A.t_min), (double)A.t_max);
    for (const Channel& c : A.ch) {
      Local& L = P.local[(size_t)c.node];
      if (c.path == 3) {
        const int n = c.interp == 2 ? c.width / 3 : c.width;
        std::vector<float>& w = P.weights[c.node];
        w.assign((size_t)n, 0.0f);
        channel_value(c, t, w.data(), n);
        continue;
      }
      if (L.matrix) throw std::runtime_error("animation targets a node that has a matrix");
      if (c.path == 0) channel_value(c, t, L.t, 3);
      else if (c.path == 2) channel_value(c, t, L.s, 3);
      else { float q[4]; channel_value(c, t, q, 4); L.q[0] = q[3]; L.q[1] = q[0]; L.q[2] = q[1]; L.q[3] = q[2]; }
    }
    return P;
  }

  static detail::Mat4 local_matrix(const Local& L) {
    if (L.matrix) { detail::Mat4 m; for (int k = 0; k < 16; ++k) m[(size_t)k] = L.m[k]; return m; }
    return detail::from_trs(L.t, L.q, L.s);
  }
  // binary32, composed as load() composes: the instance matrices
  detail::Mat4 world32(const Pose& P, long n) const {
    const detail::Mat4 l = local_matrix(P.local[(size_t)n]);
    if (!compose_ || parent_[(size_t)n] < 0) return compose_ ? detail::mul(detail::identity(), l) : l;
    return detail::mul(world32(P, parent_[(size_t)n]), l);
  }
  using Mat4d = std::array<double, 16>;
  static Mat4d mul64(const Mat4d& a, const Mat4d& b) {
    Mat4d r{};
    for (int j = 0; j < 4; ++j) for (int i = 0; i < 4; ++i) { double s = 0.0; for (int k = 0; k < 4; ++k) s += a[(size_t)(k * 4 + i)] * b[(size_t)(j * 4 + k)]; r[(size_t)(j * 4 + i)] = s; }
    return r;
  }
  Mat4d world64(const Pose& P, long n) const {
    const detail::Mat4 l = local_matrix(P.local[(size_t)n]);
    Mat4d m;
    for (int k = 0; k < 16; ++k) m[(size_t)k] = (double)l[(size_t)k];
    return parent_[(size_t)n] < 0 ? m : mul64(world64(P, parent_[(size_t)n]), m);
  }
  static Mat4d inverse_affine(const Mat4d& m) {      // upper 3x3 by cofactors, then the translation
    const double a = m[0], b = m[4], c = m[8], d = m[1], e = m[5], f = m[9], g = m[2], h = m[6], i = m[10];
    const double det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g);
    if (det == 0.0 || !std::isfinite(det)) throw std::runtime_error("the transform of a skinned mesh's node is singular");
    const double r = 1.0 / det;
    Mat4d o{};
    o[0] = (e * i - f * h) * r; o[4] = (c * h - b * i) * r; o[8] = (b * f - c * e) * r;
    o[1] = (f * g - d * i) * r; o[5] = (a * i - c * g) * r; o[9] = (c * d - a * f) * r;
    o[2] = (d * h - e * g) * r; o[6] = (b * g - a * h) * r; o[10] = (a * e - b * d) * r;
    for (int k = 0; k < 3; ++k) o[(size_t)(12 + k)] = -(o[(size_t)k] * m[12] + o[(size_t)(4 + k)] * m[13] + o[(size_t)(8 + k)] * m[14]);
    o[15] = 1.0;
    return o;
  }

  int apply(ptc_ctx* ctx, const Pose& P, bool instances) const {
    if (instances)
      for (const InstRec& I : insts_) {
        const detail::Mat4 m = world32(P, I.node);
        const int rc = ptc_update_instance_matrix(ctx, I.ptc_inst, m.data());
        if (rc < 0) return rc;
      }
    if (instances)
      for (const LightRec& L : lights_) {
        ptc_light_params p = L.params;
        detail::place_light(world32(P, L.node), p);
        const int rc = ptc_update_light(ctx, L.ptc_light, &p);
        if (rc < 0) return rc;
      }
    for (const MeshRec& M : meshes_) {
      if (M.skin < 0 && M.n_targets == 0) continue;
      std::vector<float> w, J;
      if (M.n_targets) {
        w = M.weights0;
        auto it = P.weights.find(M.node);
        if (it != P.weights.end()) for (size_t k = 0; k < w.size() && k < it->second.size(); ++k) w[k] = it->second[k];
      }
      if (M.skin >= 0) {
        const Mat4d inv = inverse_affine(world64(P, M.node));
        J.resize(M.joints.size() * 12);
        for (size_t j = 0; j < M.joints.size(); ++j) {
          Mat4d ibm;
          for (int k = 0; k < 16; ++k) ibm[(size_t)k] = M.ibm[j * 16 + (size_t)k];
          const Mat4d m = mul64(inv, mul64(world64(P, M.joints[j]), ibm));
          for (int c = 0; c < 4; ++c) for (int r = 0; r < 3; ++r) J[j * 12 + (size_t)(c * 3 + r)] = (float)m[(size_t)(c * 4 + r)];
        }
      }
      const int rc = ptc_update_mesh_pose(ctx, M.ptc_mesh, w.empty() ? nullptr : w.data(), (std::uint32_t)w.size(), J.empty() ? nullptr : J.data(), (std::uint32_t)(J.size() / 12));
      if (rc < 0) return rc;
    }
    return PTC_OK;
  }
};

}  // namespace pbr::gltf
