// pm_select_polygon_kernel: polygon queries -- which items a query polygon K of 3 .. 4096 vertices TOUCHES and which it ENCLOSES,
// under the non-zero or the even-odd rule: lasso selection, and a marquee dragged in a rotated view.  Not on the frame path: like
// pm_select_rect_kernel it reads the scene and the scene index, nothing a frame writes.  Included by pm_context.hip after
// pm_hit_rect.h (RectQ, RectOverlaps); D13's predicates (HitWinding, HitStroke), the chunk walk (ForItemChunks), the item head
// and the constants are pm_query_common.h's, as they are.
//
// What "touches" and "encloses" mean is decision D20: binary64 arithmetic on the scene's f32 / u16 values and the
// polygon's f32 values, one rounding per written operation, in the written order (-ffp-contract=off) -- tests/np_poly.py states
// the same operations in numpy and the two must agree bit for bit.
//
// The shape is pm_select_rect_kernel's, the plainest that answers: ONE polygon against every item, the 64-item steps dealt over
// the waves of the grid, a word per item.  No LDS, no barrier, no atomic: a wave never waits for another.  K's vertices are read
// from device memory; K's box, a box for every group of kPolyGroup consecutive edges and whether K is finite come from the host,
// which has the vertices in hand.  Every loop over K's edges goes group by group and skips a group that cannot matter (below).
//  * a Circle or a Line is decided on its lane, by a loop over K's edge groups;
//  * a Fill or a Polyline becomes a candidate by its box against K's box and is finished by the whole wave: first its POINTS, 64
//    per round, each lane asking inK of its own -- the walk ends as soon as one point is inside and one is not (touched, not
//    enclosed) --, then, if that left the answer open, its SEGMENTS through ForItemChunks, each lane asking its chunk's segments
//    against every edge; a Fill collects the winding of v_0 in the same walk.  B ends the walk at once.
// Winding sums are integers and the rest are any-lane "or"s: how points and chunks fall on the lanes cannot show in a word.
//
// Culling is conservative with respect to D20:
//  * a ShortBbox saturates at 0 and 65 535, so a box edge AT those values bounds nothing on its side;
//  * a segment that crosses an edge has both ends finite and its extents overlap the edge's (D20 asks it), so the box of its
//    chunk, super-chunk and item overlaps K's box; a stroke within hw of an edge overlaps K's box widened by |hw| (a Polyline's
//    item box holds the width already, pm_hit_rect.h);
//  * inK(p) needs an edge with c.y <= p.y < d.y (or the reverse) that p is not to the right of (pm_hit_test.h: there s <= 0 on a
//    rising and s >= 0 on a falling edge, by monotonic rounding): p.y within K's y-extent and p.x <= K's largest x.  So a point
//    above, below or right of K's box is outside, an item whose box is above, below or right of K's box has no point in K, and an
//    edge group whose box is above, below or left of p adds nothing to p's sum.  There is NO such cull on the fourth side: in real
//    arithmetic the sum left of K is 0 (a closed line rises as often as it falls), but with vertices of 2^35 and more a rising
//    edge's once-rounded s can be 0 where the falling edge still counts, and D20 is what numpy computes.  An item left of K's box
//    is a candidate, and a group right of p is walked;
//  * an edge group is skipped for a Fill's segment if the segment's extents miss the group's box: D20 asks the extents of a
//    crossing pair to overlap, and these are comparisons, exact;
//  * a DISTANCE (a stroke's near, a Circle's reach) is culled by boxes only with a pad: the clamped projection's closest point is
//    computed to within a few 2^-53 of the largest coordinate M that enters it, so two boxes |hw| + 2^-40 M apart (kPolyPad) hold
//    no pair whose computed distance is <= hw.  With vertices of 2^60 the pad is larger than any scene and nothing is culled,
//    which is right: there the computed distance is far from the real one, and D20 is the computed one.  The same pad widens
//    a Polyline's chunk boxes and, if no side of it is saturated (else M is unknown), its item box.  A segment with a non-finite
//    end skips nothing;
//  * the winding of v_0 in a Fill is culled as pm_hit_kernel culls a point: by boxes not above, not below, not wholly left of it.
#pragma once

#include "pm_hit_rect.h"

namespace pm {

// One launch of pm_select_polygon_kernel
struct HitPolyParams {
    SceneView V;
    const float *verts;     // [2 m] K's vertices, device memory
    const float *boxes;     // [4 ceil(m / kPolyGroup)] {min x, min y, max x, max y} of the ends of edges g kPolyGroup .. (group g)
    uint32_t m;             // 3 .. kPolyMaxVertices
    uint32_t even_odd;      // K's rule
    uint32_t valid;         // every vertex is finite (else K touches nothing)
    float box[4];           // K's box: the smallest x and y, the largest x and y of its vertices
    uint32_t *item_flags;   // [n_items] PM_SEL_*
};

namespace {

constexpr uint32_t kPolyMaxVertices = 4096u;   // PM_POLYGON_MAX_VERTICES
constexpr uint32_t kPolyGroup = 16u;           // edges to a box
constexpr double kPolyPad = 0x1p-40;           // of the largest coordinate: what a box cull of a distance leaves for its rounding

__device__ __forceinline__ double PolyMaxAbs(float4 bb) {
    return fmax(fmax(fabs(static_cast<double>(bb.x)), fabs(static_cast<double>(bb.z))), fmax(fabs(static_cast<double>(bb.y)), fabs(static_cast<double>(bb.w))));
}
__device__ __forceinline__ double PolyMaxAbs(const RectQ &b) { return fmax(fmax(fabs(b.x0), fabs(b.x1)), fmax(fabs(b.y0), fabs(b.y1))); }

// K as a wave sees it (wave-uniform)
struct PolyQ {
    const uint8_t *v;
    const float4 *gb;
    uint32_t m;
    bool even_odd;
    RectQ box;
    double v0x, v0y;
};

__device__ __forceinline__ float2 PolyVertex(const PolyQ &K, uint32_t j) { return LoadF2(K.v + static_cast<size_t>(j) * 8); }

// D20, inK(p) for a finite p
__device__ __forceinline__ bool PolyInside(const PolyQ &K, double px, double py) {
    if (!(K.box.y0 <= py && py <= K.box.y1 && px <= K.box.x1)) return false;   // (above, below or right of every edge: nothing counts)
    int w = 0;
    for (uint32_t j0 = 0; j0 < K.m; j0 += kPolyGroup) {
        const float4 bb = K.gb[j0 / kPolyGroup];
        if (!(static_cast<double>(bb.y) <= py && py <= static_cast<double>(bb.w) && px <= static_cast<double>(bb.z))) continue;
        const uint32_t j1 = min(j0 + kPolyGroup, K.m);
        float2 c = PolyVertex(K, j0);
        for (uint32_t j = j0; j < j1; ++j) {
            const float2 d = PolyVertex(K, j + 1u == K.m ? 0u : j + 1u);
            w += HitWinding(c, d, px, py);
            c = d;
        }
    }
    return K.even_odd ? (w & 1) != 0 : w != 0;
}
__device__ __forceinline__ bool PolyInside(const PolyQ &K, float2 p) {
    return RectFinite(p) && PolyInside(K, static_cast<double>(p.x), static_cast<double>(p.y));
}

// D20, crosses(a -> b, c -> d) for finite ends
__device__ __forceinline__ bool PolyCrosses(double ax, double ay, double bx, double by, double cx, double cy, double dx, double dy) {
    if (!(fmin(ax, bx) <= fmax(cx, dx) && fmax(ax, bx) >= fmin(cx, dx) && fmin(ay, by) <= fmax(cy, dy) && fmax(ay, by) >= fmin(cy, dy))) return false;
    const double s1 = (bx - ax) * (cy - ay) - (cx - ax) * (by - ay);
    const double s2 = (bx - ax) * (dy - ay) - (dx - ax) * (by - ay);
    const double s3 = (dx - cx) * (ay - cy) - (ax - cx) * (dy - cy);
    const double s4 = (dx - cx) * (by - cy) - (bx - cx) * (dy - cy);
    return !((s1 > 0.0 && s2 > 0.0) || (s1 < 0.0 && s2 < 0.0) || (s3 > 0.0 && s4 > 0.0) || (s3 < 0.0 && s4 < 0.0));
}

// D20, B for one segment a -> b of an item: it crosses an edge of K, or -- a stroke of half width hw (hw2 = hw * hw) -- is near
// one.  K closes itself, so every vertex is some edge's c: "c or d to a -> b" over all edges is "c to a -> b" over all edges.
__device__ __forceinline__ bool PolyReach(const PolyQ &K, float2 a, float2 b, bool stroke, double hw2, double wide) {
    const bool fin = RectFinite(a) && RectFinite(b);
    if (!fin && !stroke) return false;
    const double ax = a.x, ay = a.y, bx = b.x, by = b.y;
    const double sx0 = fmin(ax, bx) - wide, sx1 = fmax(ax, bx) + wide, sy0 = fmin(ay, by) - wide, sy1 = fmax(ay, by) + wide;
    const double smax = fmax(fmax(fabs(ax), fabs(bx)), fmax(fabs(ay), fabs(by)));
    for (uint32_t j0 = 0; j0 < K.m; j0 += kPolyGroup) {
        const float4 bb = K.gb[j0 / kPolyGroup];
        const double pad = stroke ? fmax(smax, PolyMaxAbs(bb)) * kPolyPad : 0.0;
        if (fin && (sx1 + pad < static_cast<double>(bb.x) || sx0 - pad > static_cast<double>(bb.z) || sy1 + pad < static_cast<double>(bb.y) ||
                    sy0 - pad > static_cast<double>(bb.w)))
            continue;
        const uint32_t j1 = min(j0 + kPolyGroup, K.m);
        float2 c = PolyVertex(K, j0);
        for (uint32_t j = j0; j < j1; ++j) {
            const float2 d = PolyVertex(K, j + 1u == K.m ? 0u : j + 1u);
            if (fin && PolyCrosses(ax, ay, bx, by, c.x, c.y, d.x, d.y)) return true;
            if (stroke && (HitStroke(a, b, c.x, c.y, hw2) || HitStroke(c, d, ax, ay, hw2) || HitStroke(c, d, bx, by, hw2))) return true;
            c = d;
        }
    }
    return false;
}

// D13's squared distance from (0, 0) to a -> b in binary64 (an ellipse's mapped edge ends are no f32 values): <= 1
__device__ __forceinline__ bool PolyUnitDisc(double ax, double ay, double bx, double by) {
    const double abx = bx - ax, aby = by - ay;
    const double apx = 0.0 - ax, apy = 0.0 - ay;
    const double L = abx * abx + aby * aby;
    double t = 0.0;
    if (L != 0.0) t = fmin(fmax((apx * abx + apy * aby) / L, 0.0), 1.0);
    const double qx = ax + abx * t, qy = ay + aby * t;
    const double dx = 0.0 - qx, dy = 0.0 - qy;
    return dx * dx + dy * dy <= 1.0;
}

__device__ __forceinline__ uint32_t PolyWord(bool reach, bool any_in, bool all_in) {
    return ((reach || any_in) ? kSelTouches : 0u) | ((!reach && all_in) ? kSelEncloses : 0u);
}

// D20, Circle / ellipse, from the item's ShortBbox alone: PM_SEL_* of it
__device__ __forceinline__ uint32_t PolyCircle(const PolyQ &K, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, bool ellipse) {
    const double fx0 = static_cast<double>(x0), fy0 = static_cast<double>(y0);
    const double cx = (fx0 + static_cast<double>(x1)) * 0.5, cy = (fy0 + static_cast<double>(y1)) * 0.5;
    const double rx = cx - fx0, ry = cy - fy0;
    if (ellipse && !(rx > 0.0 && ry > 0.0)) return 0u;   // (no geometry)
    const double r = fmin(rx, ry);
    const double wx = ellipse ? rx : r, wy = ellipse ? ry : r;
    bool reach = false;
    for (uint32_t j0 = 0; j0 < K.m && !reach; j0 += kPolyGroup) {
        const float4 bb = K.gb[j0 / kPolyGroup];
        const double pad = fmax(65535.0, PolyMaxAbs(bb)) * kPolyPad;
        if (cx + wx + pad < static_cast<double>(bb.x) || cx - wx - pad > static_cast<double>(bb.z) || cy + wy + pad < static_cast<double>(bb.y) ||
            cy - wy - pad > static_cast<double>(bb.w))
            continue;
        const uint32_t j1 = min(j0 + kPolyGroup, K.m);
        float2 c = PolyVertex(K, j0);
        for (uint32_t j = j0; j < j1 && !reach; ++j) {
            const float2 d = PolyVertex(K, j + 1u == K.m ? 0u : j + 1u);
            if (ellipse) {
                reach = PolyUnitDisc((static_cast<double>(c.x) - cx) / rx, (static_cast<double>(c.y) - cy) / ry, (static_cast<double>(d.x) - cx) / rx,
                                     (static_cast<double>(d.y) - cy) / ry);
            } else {
                reach = HitStroke(c, d, cx, cy, r * r);
            }
            c = d;
        }
    }
    const bool in = PolyInside(K, cx, cy);
    return PolyWord(reach, in, in);
}

// D20, a Line item: PM_SEL_* of it
__device__ __forceinline__ uint32_t PolyLine(const PolyQ &K, const uint8_t *it) {
    const double hw = 0.5 * static_cast<double>(__uint_as_float(LoadU32(it + 12)));
    if (hw != hw) return 0u;
    const float2 a = LoadF2(it + 16), b = LoadF2(it + 24);
    const bool reach = PolyReach(K, a, b, true, hw * hw, fabs(hw));
    const bool in_a = PolyInside(K, a), in_b = PolyInside(K, b);
    return PolyWord(reach, in_a || in_b, in_a && in_b);
}

// inK of the npt points of a Fill or a Polyline, 64 per round: is one inside, are all (a separator is no point)?  False if the
// item has no point.  The walk ends once both are known.
__device__ __forceinline__ bool PolyPoints(const PolyQ &K, const uint8_t *pts, uint32_t npt, bool compound, uint32_t lane, bool &any_in, bool &all_in) {
    bool has = false;
    any_in = false;
    all_in = true;
    for (uint32_t k0 = 0; k0 < npt; k0 += 64u) {
        const uint32_t k = k0 + lane;
        bool real = false, in = false;
        if (k < npt) {
            const float2 p = LoadF2(pts + static_cast<size_t>(k) * 8);
            if (!(compound && p.x != p.x)) {
                real = true;
                in = PolyInside(K, p);
            }
        }
        has = has || __ballot(real) != 0ull;
        any_in = any_in || __ballot(in) != 0ull;
        all_in = all_in && __ballot(real && !in) == 0ull;
        if (any_in && !all_in) break;
    }
    return has;
}

// Fill item `item`: PM_SEL_* of it (wave-uniform arguments and result)
__device__ __forceinline__ uint32_t PolyFill(const SceneView &V, uint32_t item, const uint8_t *it, const PolyQ &K, uint32_t lane) {
    const uint32_t flags = LoadU32(it + 4), npt = LoadU32(it + 12);
    const uint8_t *pts = V.scene + LoadU32(it + 16);
    const bool compound = (flags & kFillCompound) != 0;
    bool any_in, all_in;
    if (!PolyPoints(K, pts, npt, compound, lane, any_in, all_in)) return 0u;
    if (any_in && !all_in) return kSelTouches;
    const uint32_t cb0 = V.chunk_base[item], cb1 = V.chunk_base[item + 1];
    int w = 0;
    bool reach = false, any = false;
    ForItemChunks(
        V, cb0, cb1, lane,
        [&](float4 bb) {
            const bool winds = static_cast<double>(bb.y) <= K.v0y && K.v0y < static_cast<double>(bb.w) && static_cast<double>(bb.z) >= K.v0x;
            return winds || RectOverlaps(K.box, bb);
        },
        [&](uint32_t c) {
            const uint32_t k0 = (c - cb0) * kChunkSegs, k1 = min(k0 + kChunkSegs, FillSegs(npt));
            for (uint32_t k = k0; k < k1; ++k) {
                float2 a, b;
                if (!FillSegmentEnds(pts, npt, compound, k, a, b)) continue;
                reach = reach || PolyReach(K, a, b, false, 0.0, 0.0);
                w += HitWinding(a, b, K.v0x, K.v0y);
            }
        },
        [&] {
            any = __ballot(reach) != 0ull;
            return any;
        });
    if (any) return kSelTouches;
    bool v0_in = false;
    if (__ballot(w != 0) != 0ull) {
        const int sum = static_cast<int>(WaveLast(WaveInclusiveScan(static_cast<uint32_t>(w))));
        v0_in = (flags & kFillEvenOdd) ? (sum & 1) != 0 : sum != 0;
    }
    return PolyWord(false, any_in || v0_in, all_in);
}

// Polyline item `item`: PM_SEL_* of it
__device__ __forceinline__ uint32_t PolyPoly(const SceneView &V, uint32_t item, const uint8_t *it, const PolyQ &K, uint32_t lane) {
    const uint32_t npt = LoadU32(it + 12);
    const uint8_t *pts = V.scene + LoadU32(it + 16);
    const double hw = 0.5 * static_cast<double>(__uint_as_float(LoadU32(it + 8)));
    const double hw2 = hw * hw, wide = fabs(hw);
    if (npt == 0u || hw != hw) return 0u;
    bool any_in, all_in;
    (void)PolyPoints(K, pts, npt, false, lane, any_in, all_in);
    if (any_in && !all_in) return kSelTouches;
    bool reach = false, any = false;
    if (npt == 1u) {  // one degenerate segment (the scene index has no chunk for it)
        const float2 a = LoadF2(pts);
        any = PolyReach(K, a, a, true, hw2, wide);
    } else {
        const uint32_t cb0 = V.chunk_base[item], cb1 = V.chunk_base[item + 1];
        const double kmax = PolyMaxAbs(K.box);
        ForItemChunks(
            V, cb0, cb1, lane,
            [&](float4 bb) {
                const double far = wide + fmax(kmax, PolyMaxAbs(bb)) * kPolyPad;
                return !(K.box.x1 < static_cast<double>(bb.x) - far || K.box.x0 > static_cast<double>(bb.z) + far ||
                         K.box.y1 < static_cast<double>(bb.y) - far || K.box.y0 > static_cast<double>(bb.w) + far);
            },
            [&](uint32_t c) {
                const uint32_t k0 = (c - cb0) * kChunkSegs, k1 = min(k0 + kChunkSegs, PolySegs(npt));
                float2 a = LoadF2(pts + static_cast<size_t>(k0) * 8);
                for (uint32_t k = k0; k < k1 && !reach; ++k) {
                    const float2 b = LoadF2(pts + static_cast<size_t>(k + 1u) * 8);
                    reach = PolyReach(K, a, b, true, hw2, wide);
                    a = b;
                }
            },
            [&] {
                any = __ballot(reach) != 0ull;
                return any;
            });
    }
    return PolyWord(any, any_in, all_in);
}

// Is the ShortBbox a reason to look at a Fill (fill = true) or a Polyline: an edge at a saturated value bounds nothing.  The box
// is not above, below or right of K's box -- it can reach K's boundary only if it overlaps K's box, and can have a point in K
// also when it lies left of it (no cull on that side, see above) --, or -- a Fill -- passes pm_hit_kernel's cull for v_0.
__device__ __forceinline__ bool PolyCandidate(const PolyQ &K, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, bool fill) {
    const bool lo_x = x0 != 0u, lo_y = y0 != 0u, hi_x = x1 != 0xffffu, hi_y = y1 != 0xffffu;
    const double bx0 = static_cast<double>(x0), by0 = static_cast<double>(y0), bx1 = static_cast<double>(x1), by1 = static_cast<double>(y1);
    bool apart = (lo_x && K.box.x1 < bx0) || (lo_y && K.box.y1 < by0) || (hi_y && K.box.y0 > by1);
    if (!fill) {  // distances: only a box that bounds every point says how large the coordinates are, and then with the pad
        const double pad = fmax(65535.0, PolyMaxAbs(K.box)) * kPolyPad;
        apart = lo_x && lo_y && hi_x && hi_y && (K.box.x1 + pad < bx0 || K.box.y1 + pad < by0 || K.box.y0 - pad > by1);
    }
    const bool v0_out = (lo_y && K.v0y < by0) || (hi_y && K.v0y > by1) || (hi_x && K.v0x > bx1);
    return !apart || (fill && !v0_out);
}

}  // namespace

__global__ __launch_bounds__(kHitThreads) void pm_select_polygon_kernel(HitPolyParams Q) {
    const SceneView &V = Q.V;
    const uint32_t lane = LaneId();
    const bool skip = (V.flags & kHitSkipTransparent) != 0;
    const bool valid = Q.valid != 0u && Q.m >= 3u && Q.m <= kPolyMaxVertices;
    PolyQ K;
    K.v = reinterpret_cast<const uint8_t *>(Q.verts);
    K.gb = reinterpret_cast<const float4 *>(Q.boxes);
    K.m = Q.m;
    K.even_odd = Q.even_odd != 0u;
    K.box.x0 = static_cast<double>(Q.box[0]);
    K.box.y0 = static_cast<double>(Q.box[1]);
    K.box.x1 = static_cast<double>(Q.box[2]);
    K.box.y1 = static_cast<double>(Q.box[3]);
    K.v0x = K.v0y = 0.0;
    if (valid) {
        const float2 v0 = PolyVertex(K, 0u);
        K.v0x = static_cast<double>(v0.x);
        K.v0y = static_cast<double>(v0.y);
    }
    const uint32_t n_waves = GridWaves(), n_steps = ItemSteps(V.n_items);
    for (uint32_t step = FirstWaveUnit(); step < n_steps; step += n_waves) {
        // lane 0 looks at the topmost item of the step
        const uint32_t hi = min(step * 64u + 64u, V.n_items);
        const bool mine = step * 64u + lane < hi;
        const uint32_t i = mine ? hi - 1u - lane : 0u;
        uint32_t word = 0u;
        bool cand = false;
        if (mine && valid) {
            const ItemHead h = LoadItemHead(V, i);
            if (h.tag == kItemCircle) {
                word = PolyCircle(K, h.x0, h.y0, h.x1, h.y1, (h.w0 & kCircleEllipse) != 0);
            } else if (h.tag == kItemLine) {
                if (!(skip && ItemTransparent(h))) word = PolyLine(K, h.it);
            } else if (h.tag == kItemFill) {
                cand = PolyCandidate(K, h.x0, h.y0, h.x1, h.y1, true) && !(skip && ItemTransparent(h));
            } else if (h.tag == kItemPoly) {
                cand = PolyCandidate(K, h.x0, h.y0, h.x1, h.y1, false) && !(skip && ItemTransparent(h));
            }
        }
        uint64_t m = __ballot(cand);
        while (m != 0ull) {   // every candidate is finished: no item's word waits for another's
            const uint32_t l = TakeLowestLane(m);
            const ItemHead h = LoadItemHead(V, hi - 1u - l);
            const uint32_t w = h.tag == kItemFill ? PolyFill(V, h.item, h.it, K, lane) : PolyPoly(V, h.item, h.it, K, lane);
            if (lane == l) word = w;
        }
        if (mine) Q.item_flags[i] = word;
    }
}

// grid: a wave per step of 64 items, at most what the chip holds at once
void LaunchSelectPolygon(const HitPolyParams &p, uint32_t n_cus, hipStream_t stream) {
    LaunchQuery(pm_select_polygon_kernel, p, ItemSteps(p.V.n_items), n_cus, stream);
}

}  // namespace pm
