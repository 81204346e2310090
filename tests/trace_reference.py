"""What the geometric queries are held to: a float64 search of ALL triangles, and the rules by which an answer is compared with it.
For tests/test_trace_truth_host.py (the oracle), tests/test_gpu_trace_truth.py (k_trace_closest / k_trace_any) and tests/test_oracle_golden.py.

Nothing here knows a tree, a box, a slab test, an octant order or `safe_dir`: the reference is Möller–Trumbore in float64 of every ray against every
triangle of `flat_scene()`, on the TRUE vertices (not the tree's (v0, e1, e2) records, whose edges are rounded differences), in numpy, chunked over rays.

Per ray-triangle pair (`pair_terms`): t, u, v, the edge margin m = min(u, v, 1 - u - v) and the grazing measure g = |d.n| / (|d| |n|), n = e1 x e2.

CLASSIFICATION.  float32 and float64 need not agree about a ray through an edge or a vertex (which side of the edge?), nor about a ray that lies
almost in a triangle's plane (det ~ 1e-8: t, u, v mean nothing in any precision).  A comparison that counts those reports hundreds of "lost" and
"ghost" hits, none of them a defect.  So every PAIR is classed first, with fixed margins (MARGIN = 1e-3, GRAZE = 0.05, T_EPS = 1e-3):
  solid      m > MARGIN  and  g > GRAZE  and  t > T_EPS                       a hit in any precision
  clear      a miss by the same margins:  g > GRAZE and (m < -MARGIN or t < -T_EPS);
             and for g <= GRAZE, where u and v lose their meaning as det -> 0 but their numerators do not:  m * g < -MARGIN * GRAZE
             (m * g is the Möller–Trumbore numerator over |d| |n|: the rule continues the miss margin at g = GRAZE down to the exactly
             parallel ray, which misses a triangle whose plane it does not lie in; for det = 0 the value is the limit, `pair_terms`)
  undecided  everything else.  An undecided pair never makes a ray fail.
and a candidate answer (t, primitive, u, v per ray; occluded or not per ray) is then
  LOST    when the ray has a solid pair and the candidate reports no hit, or a t beyond the nearest solid hit (beyond = by more than the accuracy
          bound below, so that the rounding of t itself is not a loss)
  GHOST   when the candidate's own primitive is a clear miss in float64 for that ray, or that pair is solid but the candidate's t, u, v are off
  any-hit WRONG  when a solid pair lies inside (0, tmax (1 - MARGIN)) and the ray is reported free, or when no pair that is solid or undecided lies
          inside (0, tmax (1 + MARGIN)) and the ray is reported occluded (an undecided pair with g <= GRAZE has no t to speak of: it may block
          at any distance).
A ray is DECIDED for closest hit when it has a solid pair (the candidate must hit, no farther than it) or when all its pairs are clear (it must
miss); a ray to an edge or a vertex is decided when a solid hit lies behind the ambiguous one.  A candidate hit is left out AS GRAZING when its own
pair has g <= GRAZE.  The classification cannot be used to hide a failure: `check` holds three caps per case — at least 90 % of the rays aimed
at triangle interiors end with a solid reference hit, at least 60 % of all rays are decided, at most 10 % of the candidate's hits are left out as grazing.

ACCURACY of a solid hit (the project's convention): the same formula evaluated in numpy float32 gives, over the nearest solid
hits of the case, E32 = the largest float32-float64 gap (relative for t, absolute for u and v).  The candidate lies within 16 x E32 of the float64
value.  No literal tolerance is fixed in advance; `check` reports E32 and the candidate's worst ratio.

The stated limits of the contract: rays on an edge or a vertex, rays in a triangle's plane, and the sub-ulp overshoot of a record triangle v0 + e1 over
its box are undecided by construction — not defects, and no reason to change the triangle test, the slab test or the boxes."""
import dataclasses

import numpy as np

F32, F64 = np.float32, np.float64
MARGIN, GRAZE, T_EPS = 1e-3, 0.05, 1e-3
ACCURACY = 16.0
CAP_INTERIOR_SOLID, CAP_DECIDED, CAP_GRAZING = 0.90, 0.60, 0.10
INTERIOR, EDGE, VERTEX, MISS, SECONDARY = range(5)


def triangles(verts, idx):
    """(a, b, c): the true world-space corners, float64 (n_tris, 3) each, from flat_scene()'s (verts, idx)."""
    P = np.asarray(verts)[:, :3].astype(F64)
    idx = np.asarray(idx).reshape(-1, 3).astype(np.int64)
    return P[idx[:, 0]], P[idx[:, 1]], P[idx[:, 2]]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2], a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _from_numerators(un, vn, tn, det, dn):
    """(t, u, v, m, g, mg) from the Möller–Trumbore numerators, det and dn = |d| |n|; mg = m * g, for det = 0 its limit."""
    with np.errstate(all="ignore"):
        inv = 1.0 / det
        u, v, t = un * inv, vn * inv, tn * inv
        m = np.minimum(np.minimum(u, v), 1.0 - u - v)
        g = np.abs(det) / dn
        # det -> 0: the three numerators (un, vn, det - un - vn) sum to det, so unless all vanish one barycentric runs to -inf, at least half as fast as the largest
        mg = np.where(det == 0, -0.5 * np.maximum(np.maximum(np.abs(un), np.abs(vn)), np.abs(un + vn)) / dn, m * g)
        mg = np.where(dn > 0, mg, np.nan)                       # a zero-area triangle is never hit and never decides anything
    return t, u, v, m, g, mg


def pair_terms(a, b, c, o, d, dt=F64):
    """Möller–Trumbore of rays (o, d) against triangles (a, b, c), all broadcast against each other, evaluated in `dt` in the order of the textbook
    formula (numpy rounds every operation to `dt`).  Returns (t, u, v, m, g, mg)."""
    a, b, c, o, d = (np.asarray(x).astype(dt) for x in (a, b, c, o, d))
    e1, e2 = b - a, c - a
    p = _cross(d, e2)
    det = (e1 * p).sum(-1)
    tv = o - a
    q = _cross(tv, e1)
    n = _cross(e1, e2)
    dn = np.sqrt((d * d).sum(-1) * (n * n).sum(-1))
    return _from_numerators((tv * p).sum(-1), (d * q).sum(-1), (e2 * q).sum(-1), det, dn)


def _classes(t, m, g, mg):
    with np.errstate(invalid="ignore"):
        steep = g > GRAZE
        solid = steep & (m > MARGIN) & (t > T_EPS)
        clear = (steep & ((m < -MARGIN) | (t < -T_EPS))) | ((g <= GRAZE) & (mg < -MARGIN * GRAZE))
    return solid, clear


@dataclasses.dataclass
class Truth:
    """Per ray: the nearest and the second solid pair (prim -1, t inf where there is none), whether every pair is clear, and for any-hit whether a
    solid blocker lies inside tmax (1 - MARGIN) / whether anything not clear may lie inside tmax (1 + MARGIN)."""
    n_tris: int
    t: np.ndarray
    prim: np.ndarray
    t2: np.ndarray
    prim2: np.ndarray
    all_clear: np.ndarray
    must_block: np.ndarray
    may_block: np.ndarray


def _scan(tri, org, dirs, tmax, chunk):
    a, b, c = tri
    e1, e2 = b - a, c - a
    N = _cross(e1, e2)
    nlen = np.sqrt((N * N).sum(1))
    Xu, Xv, an = _cross(e2, a), _cross(a, e1), (a * N).sum(1)
    n = len(org)
    out = Truth(len(a), np.full(n, np.inf), np.full(n, -1, np.int64), np.full(n, np.inf), np.full(n, -1, np.int64), np.zeros(n, bool), np.zeros(n, bool), np.zeros(n, bool))
    if chunk is None:
        chunk = max(1, min(256, (1 << 22) // max(1, len(a))))
    for s in range(0, n, chunk):
        o, d = np.asarray(org[s:s + chunk]).astype(F64), np.asarray(dirs[s:s + chunk]).astype(F64)
        M = _cross(o, d)
        # the scalar triple products of the formula as seven (rays x 3) @ (3 x triangles) products: tv.(d x e2) = e2.(o x d) - d.(e2 x a), d.(tv x e1) =
        # -e1.(o x d) - d.(a x e1), e2.(tv x e1) = (o - a).n, e1.(d x e2) = -d.n; `check` holds the nearest hits of this against the textbook order
        det = -(d @ N.T)
        un, vn, tn = M @ e2.T - d @ Xu.T, -(M @ e1.T) - d @ Xv.T, o @ N.T - an[None]
        dn = np.sqrt((d * d).sum(1))[:, None] * nlen[None]
        t, u, v, m, g, mg = _from_numerators(un, vn, tn, det, dn)
        solid, clear = _classes(t, m, g, mg)
        r = np.arange(len(o))
        ts = np.where(solid, t, np.inf)
        k = ts.argmin(1)
        out.t[s:s + chunk] = ts[r, k]
        out.prim[s:s + chunk] = np.where(np.isfinite(ts[r, k]), k, -1)
        ts[r, k] = np.inf
        k2 = ts.argmin(1)
        out.t2[s:s + chunk] = ts[r, k2]
        out.prim2[s:s + chunk] = np.where(np.isfinite(ts[r, k2]), k2, -1)
        out.all_clear[s:s + chunk] = clear.all(1)
        if tmax is not None:
            tm = np.asarray(tmax[s:s + chunk]).astype(F64)[:, None]
            out.must_block[s:s + chunk] = (solid & (t < tm * (1 - MARGIN))).any(1)
            with np.errstate(invalid="ignore"):
                out.may_block[s:s + chunk] = (~clear & ((g <= GRAZE) | ~(t >= tm * (1 + MARGIN)))).any(1)
    return out


def closest_all(verts, idx, org, dirs, chunk=None):
    """Truth of closest hit: float64, every ray against every triangle."""
    return _scan(triangles(verts, idx), org, dirs, None, chunk)


def any_all(verts, idx, org, dirs, tmax, chunk=None):
    """Truth of closest hit and of occlusion within (0, tmax) in one pass."""
    return _scan(triangles(verts, idx), org, dirs, tmax, chunk)


def pair_at(verts, idx, org, dirs, prim, dt=F64):
    """pair_terms of every ray against ITS triangle `prim` (rays with prim < 0 get triangle 0; mask them)."""
    a, b, c = triangles(verts, idx)
    k = np.maximum(np.asarray(prim, np.int64), 0)
    if dt is F32:       # the float32 evaluation starts from the float32 data
        return pair_terms(a[k].astype(F32), b[k].astype(F32), c[k].astype(F32), np.asarray(org, F32), np.asarray(dirs, F32), F32)
    return pair_terms(a[k], b[k], c[k], org, dirs, F64)


def e32_of(verts, idx, org, dirs, truth):
    """(E32 of t, relative; E32 of u and v, absolute; hits): the float32-float64 gap of pair_terms over the nearest solid hits.  Also holds _scan's
    rearranged arithmetic against the textbook order."""
    h = truth.prim >= 0
    if not h.any():
        return 0.0, 0.0, 0
    t64, u64, v64, m64, _, _ = pair_at(verts, idx, org[h], dirs[h], truth.prim[h])
    assert (m64 > MARGIN * 0.999).all() and np.allclose(t64, truth.t[h], rtol=1e-9, atol=0), "the two float64 evaluations disagree"
    t32, u32, v32, _, _, _ = pair_at(verts, idx, org[h], dirs[h], truth.prim[h], F32)
    et = float(np.max(np.abs(t32.astype(F64) - t64) / t64))
    euv = float(max(np.max(np.abs(u32.astype(F64) - u64)), np.max(np.abs(v32.astype(F64) - v64))))
    return et, euv, int(h.sum())


def check_closest(verts, idx, org, dirs, truth, e32, t, prim, uv):
    """Masks and figures of a candidate closest-hit answer.  e32 = (E32 of t, E32 of uv) of the case."""
    t, prim, uv = np.asarray(t), np.asarray(prim), np.asarray(uv)
    hit = prim >= 0
    assert (prim < truth.n_tris).all(), "primitive id out of range"
    t64, u64, v64, m, g, mg = pair_at(verts, idx, org, dirs, prim)
    solid, clear = _classes(t64, m, g, mg)
    solid, clear = solid & hit, clear & hit
    bound_t, bound_uv = ACCURACY * e32[0], ACCURACY * e32[1]
    has = truth.prim >= 0
    tc = t.astype(F64)
    lost = has & (~hit | (tc > truth.t * (1 + bound_t)))
    with np.errstate(all="ignore"):
        rt = np.where(solid, np.abs(tc - t64) / t64, 0.0)
        ruv = np.where(solid, np.maximum(np.abs(uv[:, 0].astype(F64) - u64), np.abs(uv[:, 1].astype(F64) - v64)), 0.0)
    off = solid & ((rt > bound_t) | (ruv > bound_uv))
    ghost = clear | off | (hit & truth.all_clear)
    grazing = hit & ~(g > GRAZE)
    ratio = max(float(rt.max(initial=0.0)) / e32[0] if e32[0] > 0 else 0.0, float(ruv.max(initial=0.0)) / e32[1] if e32[1] > 0 else 0.0)
    return dict(lost=lost, ghost=ghost, decided=has | truth.all_clear, grazing=grazing, hits=int(hit.sum()), ratio=ratio)


def check_any(truth, occ):
    occ = np.asarray(occ) != 0
    return (truth.must_block & ~occ) | (~truth.may_block & occ)


def check(tag, verts, idx, rays, truth, e32, t, prim, uv, occ, caps=True, sel=None):
    """One case: prints its figures, asserts the caps (unless the candidate is a deliberately altered one) and returns
    (lost, ghost, any-hit wrong) as masks.  `sel`: the candidate answers rays[sel] only (a ragged launch); the caps are the whole set's."""
    org, dirs, tmax, kind = rays
    if sel is not None:
        org, dirs, tmax, kind = org[sel], dirs[sel], tmax[sel], kind[sel]
        truth = Truth(truth.n_tris, *(getattr(truth, f.name)[sel] for f in dataclasses.fields(Truth)[1:]))
    r = check_closest(verts, idx, org, dirs, truth, e32, t, prim, uv)
    wrong = check_any(truth, occ) if occ is not None else np.zeros(len(org), bool)            # occ None: a closest-hit answer alone (the guide buffers)
    n = len(org)
    interior = kind == INTERIOR
    share_int = float((truth.prim >= 0)[interior].mean()) if interior.any() else 1.0
    decided, graze = float(r["decided"].mean()), float(r["grazing"].sum()) / max(1, r["hits"])
    any_decided = float((truth.must_block | ~truth.may_block).mean())
    print("%s: rays %d decided %.1f %% (any-hit %.1f %%) interior-solid %.1f %% grazing %.1f %% of %d hits E32 t %.2e uv %.2e worst ratio %.2f lost %d ghost %d any-hit wrong %d"
          % (tag, n, 100 * decided, 100 * any_decided, 100 * share_int, 100 * graze, r["hits"], e32[0], e32[1], r["ratio"],
             int(r["lost"].sum()), int(r["ghost"].sum()), int(wrong.sum())), flush=True)
    if caps and sel is None:
        assert share_int >= CAP_INTERIOR_SOLID, "%s: only %.1f %% of the rays aimed at interiors have a solid hit" % (tag, 100 * share_int)
        assert decided >= CAP_DECIDED, "%s: only %.1f %% of the rays are decided" % (tag, 100 * decided)
        assert graze <= CAP_GRAZING, "%s: %.1f %% of the hits are left out as grazing" % (tag, 100 * graze)
    return r["lost"], r["ghost"], wrong


def assert_true(tag, verts, idx, rays, truth, e32, t, prim, uv, occ, sel=None):
    """The candidate answers are right: 0 lost, 0 ghost, any-hit never wrong, caps held, accuracy within 16 x E32."""
    lost, ghost, wrong = check(tag, verts, idx, rays, truth, e32, t, prim, uv, occ, sel=sel)
    bad = np.nonzero(lost | ghost | wrong)[0]
    o, d = (rays[0], rays[1]) if sel is None else (rays[0][sel], rays[1][sel])
    assert len(bad) == 0, "%s: rays %s fail; the first: org %r dir %r -> t %r prim %r uv %r occ %r (lost %s ghost %s any %s)" % (
        tag, bad[:8].tolist(), o[bad[0]].tolist(), d[bad[0]].tolist(), float(t[bad[0]]), int(prim[bad[0]]), uv[bad[0]].tolist(), -1 if occ is None else int(occ[bad[0]]),
        bool(lost[bad[0]]), bool(ghost[bad[0]]), bool(wrong[bad[0]]))


# ---- rays ------------------------------------------------------------------------------------------------------------------------------
def box_planes(ora_nodes):
    """(axis, value) of every child-box plane of the oracle's tree (Oracle.bvh()[0]): node origin + q * 2^(e - 127), as float32."""
    w = np.asarray(ora_nodes).view(np.uint32)
    org, e = np.asarray(ora_nodes)[:, 0:3].astype(F64), w[:, 6:9].astype(np.int64)
    code = w[:, 57:65].view(np.int32)
    q = np.concatenate([w[:, 9:33].reshape(-1, 3, 8), w[:, 33:57].reshape(-1, 3, 8)], 2).astype(F64)          # (nodes, axis, 16 planes)
    val = org[:, :, None] + q * np.exp2((e - 127).astype(F64))[:, :, None]
    used = np.concatenate([code != -(2 ** 31)] * 2, 1)[:, None, :] & np.ones((1, 3, 1), bool)
    axis = np.broadcast_to(np.arange(3)[None, :, None], val.shape)
    return axis[used].astype(np.int64), val[used].astype(F32)


MIX = (0.45, 0.15, 0.10, 0.10, 0.20)       # interior, edge, vertex, miss, secondary


def make_rays(verts, idx, planes, n, seed):
    """(org, dirs, tmax, kind), seeded.  Targets on triangles: interior points (Dirichlet barycentrics), points on edges, vertices; origins spread
    through and around the scene bounds, so that rays start inside boxes, a tenth of them exactly on a box plane of the tree (`planes` =
    box_planes(...)); a third of the aimed rays with one or two direction components exactly 0.0, -0.0 or of magnitude 1e-8 .. 1e-30 (either side of
    safe_dir's 1e-20); rays that leave the scene and miss everything; rays from a surface point along the surface normal with a small offset (the
    shape of a secondary ray).  Rays shorter than 1e-3 are dropped, so slightly fewer than n come back.  kind: INTERIOR .. SECONDARY."""
    rng = np.random.default_rng(seed)
    a, b, c = triangles(verts, idx)
    nrm = _cross(b - a, c - a)
    ok = np.nonzero((nrm * nrm).sum(1) > 0)[0]
    lo, hi = np.minimum(np.minimum(a, b), c).min(0), np.maximum(np.maximum(a, b), c).max(0)
    ext, ctr = hi - lo, 0.5 * (lo + hi)
    diag = float(np.linalg.norm(ext))
    kind = rng.choice(5, n, p=MIX)
    tri = ok[rng.integers(0, len(ok), n)]
    bary = rng.dirichlet((1.0, 1.0, 1.0), n)
    e = kind == EDGE
    bary[e, rng.integers(0, 3, n)[e]] = 0.0
    bary[e] /= bary[e].sum(1, keepdims=True)
    bary[kind == VERTEX] = np.eye(3)[rng.integers(0, 3, int((kind == VERTEX).sum()))]
    bary[kind == SECONDARY] = rng.dirichlet((2.0, 2.0, 2.0), int((kind == SECONDARY).sum()))
    tgt = a[tri] * bary[:, 0:1] + b[tri] * bary[:, 1:2] + c[tri] * bary[:, 2:3]
    pad = np.maximum(0.1 * ext, 0.25 * ext.max())              # a flat scene's origins are not all down at its ground
    org = rng.uniform(lo - pad, hi + pad, (n, 3))
    # the mix, not the margins, keeps a case inside `check`'s caps: an origin from which the ray would graze its own interior target (g <= 2 GRAZE; common
    # in a flat scene, whose bounds hug the ground) is drawn again, up to three times; rays to edges and vertices keep whatever angle they get
    nlen = np.linalg.norm(nrm[tri], axis=1)
    for _ in range(3):
        d = tgt - org
        again = (kind == INTERIOR) & (np.abs((d * nrm[tri]).sum(1)) <= 2 * GRAZE * np.linalg.norm(d, axis=1) * nlen)
        org[again] = rng.uniform(lo - pad, hi + pad, (int(again.sum()), 3))
    on_plane = np.nonzero((rng.random(n) < 0.1) & (kind <= VERTEX))[0]
    if len(planes[0]):
        pk = rng.integers(0, len(planes[0]), len(on_plane))
        org[on_plane, planes[0][pk]] = planes[1][pk]
    org = org.astype(F32).astype(F64)
    d = tgt - org
    # a third of the aimed rays: one (mostly) or two direction components zero, negative zero or tiny; the origin takes the target's coordinate there
    special = (rng.random(n) < 1.0 / 3.0) & (kind <= VERTEX)
    two = rng.random(n) < 0.3
    ax0 = rng.integers(0, 3, n)
    ax1 = (ax0 + 1 + rng.integers(0, 2, n)) % 3
    # ... for an interior target the two axes in which its triangle's normal is smallest, or such a ray would lie in the plane of an axis-aligned wall it aims at
    flat = np.argsort(np.abs(nrm[tri]), axis=1)
    first = rng.integers(0, 2, n)
    ax0 = np.where(kind == INTERIOR, flat[np.arange(n), first], ax0)
    ax1 = np.where(kind == INTERIOR, flat[np.arange(n), 1 - first], ax1)
    tiny = np.zeros((n, 3))
    for ax, on in ((ax0, special), (ax1, special & two)):
        j = np.nonzero(on)[0]
        org[j, ax[j]] = tgt[j, ax[j]].astype(F32)
        how = rng.integers(0, 3, len(j))
        val = np.where(how == 0, 0.0, np.where(how == 1, -0.0, rng.choice([-1.0, 1.0], len(j)) * 10.0 ** -rng.uniform(8, 30, len(j))))
        d[j, ax[j]] = np.nan
        tiny[j, ax[j]] = val
    put = np.isnan(d)
    d = np.where(put, 0.0, tgt - org)
    # misses: from the bounds' shell outwards
    ms = kind == MISS
    out_dir = rng.standard_normal((n, 3))
    out_dir /= np.linalg.norm(out_dir, axis=1, keepdims=True)
    org[ms] = (ctr + out_dir[ms] * (0.55 * diag + 0.3 * diag * rng.random((int(ms.sum()), 1)))).astype(F32)
    away = out_dir + 0.3 * rng.standard_normal((n, 3))
    d[ms] = away[ms]
    # secondary rays: from the surface point, off the surface by a ray epsilon, along the normal (either side), half of them tilted
    sec = kind == SECONDARY
    nh = nrm[tri] / np.linalg.norm(nrm[tri], axis=1, keepdims=True) * rng.choice([-1.0, 1.0], (n, 1))
    org[sec] = (tgt[sec] + nh[sec] * (1e-4 * diag)).astype(F32)
    tilt = nh + np.where(rng.random((n, 1)) < 0.5, 0.0, 0.8) * rng.standard_normal((n, 3))
    tilt = np.where((tilt * nh).sum(1, keepdims=True) > 0.1, tilt, nh)
    d[sec] = tilt[sec]
    length = np.linalg.norm(d, axis=1)
    keep = length > 1e-3
    dirs = d / np.maximum(length, 1e-30)[:, None]
    dirs = np.where(put, tiny, dirs).astype(F32)
    aimed = kind <= VERTEX
    tmax = np.where(aimed, length * rng.choice([0.5, 0.9, 1.1, 2.0], n), diag * rng.uniform(0.01, 1.0, n)).astype(F32)
    return org[keep].astype(F32), dirs[keep], tmax[keep], kind[keep]
