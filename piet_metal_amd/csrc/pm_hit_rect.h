// pm_hit_rects_kernel, pm_select_rect_kernel: rectangle queries -- does an item's shape have a point in common with a closed
// axis-aligned rectangle R (it TOUCHES R), and does all of it lie in R (R ENCLOSES it).  Picking with a tolerance is the first
// question asked of a small square around the cursor, marquee selection is both asked of every item.  Not on the frame path:
// like pm_hit_kernel they read the scene and the scene index, nothing a frame writes.  Included by pm_context.hip; D13's predicates
// (HitWinding, HitStroke), the chunk walk (ForItemChunks), the item head and the constants are pm_query_common.h's, as they are.
//
// What "touches" and "encloses" mean is decision D19: binary64 arithmetic on the scene's f32 / u16 values and the
// query's f32 values, one rounding per written operation, in the written order (-ffp-contract=off) -- tests/np_rect.py states
// the same operations in numpy and the two must agree bit for bit.
//
//  pm_hit_rects_kernel    one WAVE owns a query rectangle and walks the items from the top of paint order down, 64 per step, as
//                         pm_hit_kernel does: a Circle or a Line is decided on its lane, a Fill or a Polyline becomes a
//                         candidate by its box against R, and the candidates are worked off from the topmost lane on.  Without
//                         a count the walk ends at the first item that touches.
//  pm_select_rect_kernel  ONE rectangle against every item: the 64-item steps are dealt over the waves of the grid, and every
//                         item gets a word -- bit 0 touches, bit 1 encloses.  Every candidate of a step is finished.
//
// A candidate's chunks go through ForItemChunks: chunk boxes, for an item of more than 64 chunks its super-chunks' boxes first.
// A Fill's winding is an integer sum over the wave and "some segment meets R" an any-lane ballot: how the chunks fall on the
// lanes cannot show.  A predicate may end early -- a Fill at its first meeting segment, a stroke at its first hit.
//
// Culling is conservative with respect to D19:
//  * a ShortBbox saturates at 0 and 65 535, so a box edge AT those values bounds nothing on its side;
//  * a segment that meets R has both ends finite and its own box overlaps R, so the box of its chunk (the exact minimum and
//    maximum of the chunk's points, NaNs ignored), of its super-chunk and of its item overlaps R;
//  * a Fill is asked two things in ONE walk of its chunks: a chunk whose box overlaps R can hold a meeting segment, and a chunk
//    that passes pm_hit_kernel's own cull for the corner (x0, y0) -- not above, not below, not wholly left of it -- can add to the
//    corner's winding.  A chunk that passes either is worked, and both predicates are evaluated on all its segments: each is D19's
//    own, so a segment too many changes nothing.  The winding is NOT culled by "R is left of the box": D13 never does;
//  * a stroke's chunk boxes are widened by |hw| (its item box holds the width already).  The six squared distances compare
//    against hw * hw, which has no sign;
//  * an item R encloses has only finite points, all in R, so its box overlaps R: it is a candidate.  Whether R encloses a
//    candidate is asked of its points directly, 64 per step, ending at the first step with a point outside -- for an item that
//    is not enclosed that is nearly always the first.
#pragma once

#include "pm_query_common.h"

namespace pm {

// One launch of pm_hit_rects_kernel: n query rectangles
struct HitRectParams {
    SceneView V;
    const float *rects;     // [4 n] {x0, y0, x1, y1}
    uint32_t *top_item;     // [n] last-painted item that touches the rectangle, or 0xffffffff
    uint32_t *n_hit;        // [n] items that touch it (nullptr: not asked for -- the walk ends at the first)
    uint32_t n;
};

// One launch of pm_select_rect_kernel: one rectangle against every item
struct SelectRectParams {
    SceneView V;
    uint32_t *item_flags;   // [n_items] PM_SEL_*
    float rect[4];
};

namespace {

// The query rectangle in binary64 (wave-uniform)
struct RectQ {
    double x0, y0, x1, y1;
};

// D19: a rectangle with a non-finite value, or with x1 < x0 or y1 < y0, touches nothing and encloses nothing
__device__ __forceinline__ bool RectLoad(const float *r, RectQ &R) {
    const uint32_t b0 = UniformF32Bits(__float_as_uint(r[0]));
    const uint32_t b1 = UniformF32Bits(__float_as_uint(r[1]));
    const uint32_t b2 = UniformF32Bits(__float_as_uint(r[2]));
    const uint32_t b3 = UniformF32Bits(__float_as_uint(r[3]));
    R.x0 = static_cast<double>(__uint_as_float(b0));
    R.y0 = static_cast<double>(__uint_as_float(b1));
    R.x1 = static_cast<double>(__uint_as_float(b2));
    R.y1 = static_cast<double>(__uint_as_float(b3));
    return RectFiniteBits(b0) && RectFiniteBits(b1) && RectFiniteBits(b2) && RectFiniteBits(b3) && !(R.x1 < R.x0) && !(R.y1 < R.y0);
}

// D19, point to rectangle: dR2(p).  A NaN coordinate makes it NaN (the decision's max keeps a NaN), which compares false.
__device__ __forceinline__ double RectDist2(const RectQ &R, double px, double py) {
    const double ex = px != px ? px : fmax(fmax(R.x0 - px, 0.0), px - R.x1);
    const double ey = py != py ? py : fmax(fmax(R.y0 - py, 0.0), py - R.y1);
    return ex * ex + ey * ey;
}

// D19, segment a -> b meets R
__device__ __forceinline__ bool RectMeets(const RectQ &R, float2 a, float2 b) {
    if (!(RectFinite(a) && RectFinite(b))) return false;
    const double ax = a.x, ay = a.y, bx = b.x, by = b.y;
    if (!(fmin(ax, bx) <= R.x1 && fmax(ax, bx) >= R.x0 && fmin(ay, by) <= R.y1 && fmax(ay, by) >= R.y0)) return false;
    const double s0 = (bx - ax) * (R.y0 - ay) - (R.x0 - ax) * (by - ay);
    const double s1 = (bx - ax) * (R.y0 - ay) - (R.x1 - ax) * (by - ay);
    const double s2 = (bx - ax) * (R.y1 - ay) - (R.x1 - ax) * (by - ay);
    const double s3 = (bx - ax) * (R.y1 - ay) - (R.x0 - ax) * (by - ay);
    const bool pos = s0 > 0.0 && s1 > 0.0 && s2 > 0.0 && s3 > 0.0;
    const bool neg = s0 < 0.0 && s1 < 0.0 && s2 < 0.0 && s3 < 0.0;
    return !(pos || neg);
}

// D19, Line and Polyline: segment a -> b of half width hw (hw2 = hw * hw) touches R
__device__ __forceinline__ bool RectStroke(const RectQ &R, float2 a, float2 b, double hw2) {
    if (RectMeets(R, a, b)) return true;
    if (HitStroke(a, b, R.x0, R.y0, hw2) || HitStroke(a, b, R.x1, R.y0, hw2) || HitStroke(a, b, R.x1, R.y1, hw2) || HitStroke(a, b, R.x0, R.y1, hw2)) return true;
    return RectDist2(R, a.x, a.y) <= hw2 || RectDist2(R, b.x, b.y) <= hw2;
}

// D19, Circle / ellipse, from the item's ShortBbox alone: PM_SEL_* of it
__device__ __forceinline__ uint32_t RectCircle(const RectQ &R, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, bool ellipse) {
    const double fx0 = static_cast<double>(x0), fy0 = static_cast<double>(y0);
    const double cx = (fx0 + static_cast<double>(x1)) * 0.5, cy = (fy0 + static_cast<double>(y1)) * 0.5;
    double rx = cx - fx0, ry = cy - fy0;
    const double ex = fmax(fmax(R.x0 - cx, 0.0), cx - R.x1), ey = fmax(fmax(R.y0 - cy, 0.0), cy - R.y1);
    bool touches;
    if (ellipse) {
        if (!(rx > 0.0 && ry > 0.0)) return 0u;   // (it contains no point: no geometry)
        touches = (ex / rx) * (ex / rx) + (ey / ry) * (ey / ry) <= 1.0;
    } else {
        const double r = fmin(rx, ry);
        touches = ex * ex + ey * ey <= r * r;
        rx = ry = r;
    }
    const bool encloses = R.x0 <= cx - rx && cx + rx <= R.x1 && R.y0 <= cy - ry && cy + ry <= R.y1;
    return (touches ? kSelTouches : 0u) | (encloses ? kSelEncloses : 0u);
}

// D19, a Line item: PM_SEL_* of it
__device__ __forceinline__ uint32_t RectLine(const RectQ &R, const uint8_t *it) {
    const double hw = 0.5 * static_cast<double>(__uint_as_float(LoadU32(it + 12)));
    if (hw != hw) return 0u;
    const float2 a = LoadF2(it + 16), b = LoadF2(it + 24);
    const bool touches = RectStroke(R, a, b, hw * hw);
    const double ax = a.x, ay = a.y, bx = b.x, by = b.y;
    const bool encloses = RectFinite(a) && RectFinite(b) && R.x0 <= ax - hw && ax + hw <= R.x1 && R.y0 <= ay - hw && ay + hw <= R.y1 &&
                          R.x0 <= bx - hw && bx + hw <= R.x1 && R.y0 <= by - hw && by + hw <= R.y1;
    return (touches ? kSelTouches : 0u) | (encloses ? kSelEncloses : 0u);
}

__device__ __forceinline__ bool RectOverlaps(const RectQ &R, float4 bb) {
    return static_cast<double>(bb.x) <= R.x1 && static_cast<double>(bb.z) >= R.x0 && static_cast<double>(bb.y) <= R.y1 && static_cast<double>(bb.w) >= R.y0;
}

// Does Fill item `item` touch R (wave-uniform arguments and result)
__device__ __forceinline__ bool RectFill(const SceneView &V, uint32_t item, const uint8_t *it, const RectQ &R, uint32_t lane) {
    const uint32_t flags = LoadU32(it + 4), npt = LoadU32(it + 12);
    const uint8_t *pts = V.scene + LoadU32(it + 16);
    const bool compound = (flags & kFillCompound) != 0;
    const uint32_t cb0 = V.chunk_base[item], cb1 = V.chunk_base[item + 1];
    int w = 0;
    bool meets = false, any = false;
    ForItemChunks(
        V, cb0, cb1, lane,
        [&](float4 bb) {
            const bool winds = static_cast<double>(bb.y) <= R.y0 && R.y0 < static_cast<double>(bb.w) && static_cast<double>(bb.z) >= R.x0;
            return winds || RectOverlaps(R, bb);
        },
        [&](uint32_t c) {
            const uint32_t k0 = (c - cb0) * kChunkSegs, k1 = min(k0 + kChunkSegs, FillSegs(npt));
            for (uint32_t k = k0; k < k1; ++k) {
                float2 a, b;
                if (!FillSegmentEnds(pts, npt, compound, k, a, b)) continue;
                meets = meets || RectMeets(R, a, b);
                w += HitWinding(a, b, R.x0, R.y0);
            }
        },
        [&] {
            any = __ballot(meets) != 0ull;
            return any;
        });
    if (any) return true;
    if (__ballot(w != 0) == 0ull) return false;
    const int sum = static_cast<int>(WaveLast(WaveInclusiveScan(static_cast<uint32_t>(w))));
    return (flags & kFillEvenOdd) ? (sum & 1) != 0 : sum != 0;
}

// Does Polyline item `item` touch R
__device__ __forceinline__ bool RectPoly(const SceneView &V, uint32_t item, const uint8_t *it, const RectQ &R, uint32_t lane) {
    const uint32_t npt = LoadU32(it + 12);
    const uint8_t *pts = V.scene + LoadU32(it + 16);
    const double hw = 0.5 * static_cast<double>(__uint_as_float(LoadU32(it + 8)));
    const double hw2 = hw * hw, wide = fabs(hw);
    if (npt == 0u || hw != hw) return false;
    if (npt == 1u) {  // one degenerate segment (the scene index has no chunk for it)
        const float2 a = LoadF2(pts);
        return RectStroke(R, a, a, hw2);
    }
    const uint32_t cb0 = V.chunk_base[item], cb1 = V.chunk_base[item + 1];
    bool hit = false, any = false;
    ForItemChunks(
        V, cb0, cb1, lane,
        [&](float4 bb) {
            return !(R.x1 < static_cast<double>(bb.x) - wide || R.x0 > static_cast<double>(bb.z) + wide || R.y1 < static_cast<double>(bb.y) - wide ||
                     R.y0 > static_cast<double>(bb.w) + wide);
        },
        [&](uint32_t c) {
            const uint32_t k0 = (c - cb0) * kChunkSegs, k1 = min(k0 + kChunkSegs, PolySegs(npt));
            float2 a = LoadF2(pts + static_cast<size_t>(k0) * 8);
            for (uint32_t k = k0; k < k1 && !hit; ++k) {
                const float2 b = LoadF2(pts + static_cast<size_t>(k + 1u) * 8);
                hit = RectStroke(R, a, b, hw2);
                a = b;
            }
        },
        [&] {
            any = __ballot(hit) != 0ull;
            return any;
        });
    return any;
}

// Does R enclose the npt points of a Fill (hw = 0) or a Polyline: 64 points per step, ended by the first point outside
__device__ __forceinline__ bool RectEnclosesPoints(const uint8_t *pts, uint32_t npt, bool compound, double hw, const RectQ &R, uint32_t lane) {
    bool any = false;
    for (uint32_t k0 = 0; k0 < npt; k0 += 64u) {
        const uint32_t k = k0 + lane;
        bool real = false, bad = false;
        if (k < npt) {
            const float2 p = LoadF2(pts + static_cast<size_t>(k) * 8);
            if (!(compound && p.x != p.x)) {  // (a separator is no point)
                const double px = p.x, py = p.y;
                real = true;
                bad = !(RectFinite(p) && R.x0 <= px - hw && px + hw <= R.x1 && R.y0 <= py - hw && py + hw <= R.y1);
            }
        }
        if (__ballot(bad) != 0ull) return false;
        any = any || __ballot(real) != 0ull;
    }
    return any;
}

// Is the ShortBbox {x0, y0, x1, y1} a reason to look at a Fill (fill = true) or a Polyline: an edge at a saturated value bounds
// nothing.  The box overlaps R, or -- a Fill -- passes pm_hit_kernel's cull for the corner (R.x0, R.y0).
__device__ __forceinline__ bool RectCandidate(const RectQ &R, uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, bool fill) {
    const bool lo_x = x0 != 0u, lo_y = y0 != 0u, hi_x = x1 != 0xffffu, hi_y = y1 != 0xffffu;
    const double bx0 = static_cast<double>(x0), by0 = static_cast<double>(y0), bx1 = static_cast<double>(x1), by1 = static_cast<double>(y1);
    const bool apart = (lo_x && R.x1 < bx0) || (hi_x && R.x0 > bx1) || (lo_y && R.y1 < by0) || (hi_y && R.y0 > by1);
    const bool corner_out = (lo_y && R.y0 < by0) || (hi_y && R.y0 > by1) || (hi_x && R.x0 > bx1);
    return !apart || (fill && !corner_out);
}

// What a lane makes of a Fill's or a Polyline's head for both kernels: a candidate by its box, unless the flags skip it
__device__ __forceinline__ bool RectCandidate(const RectQ &R, const ItemHead &h, bool fill, bool skip) {
    return RectCandidate(R, h.x0, h.y0, h.x1, h.y1, fill) && !(skip && ItemTransparent(h));
}

}  // namespace

__global__ __launch_bounds__(kHitThreads) void pm_hit_rects_kernel(HitRectParams Q) {
    const SceneView &V = Q.V;
    const uint32_t lane = LaneId();
    const bool counts = Q.n_hit != nullptr;
    const bool skip = (V.flags & kHitSkipTransparent) != 0;
    const uint32_t n_waves = GridWaves();
    for (uint32_t q = FirstWaveUnit(); q < Q.n; q += n_waves) {
        RectQ R;
        const bool valid = RectLoad(Q.rects + static_cast<size_t>(q) * 4, R);
        bool done = !valid;
        uint32_t top = kHitNone, cnt = 0;
        for (uint32_t hi = V.n_items; hi != 0u && !done; hi = hi > 64u ? hi - 64u : 0u) {
            // lane 0 looks at the topmost item of the step
            bool direct = false, cand = false;
            if (lane < hi) {
                const ItemHead h = LoadItemHead(V, hi - 1u - lane);
                if (h.tag == kItemCircle) {
                    direct = (RectCircle(R, h.x0, h.y0, h.x1, h.y1, (h.w0 & kCircleEllipse) != 0) & kSelTouches) != 0u;
                } else if (h.tag == kItemLine) {
                    if (!(skip && ItemTransparent(h))) direct = (RectLine(R, h.it) & kSelTouches) != 0u;
                } else if (h.tag == kItemFill) {
                    cand = RectCandidate(R, h, true, skip);
                } else if (h.tag == kItemPoly) {
                    cand = RectCandidate(R, h, false, skip);
                }
            }
            const uint64_t md = __ballot(direct);
            uint64_t m = md | __ballot(cand);
            while (m != 0ull) {
                const uint32_t l = TakeLowestLane(m);
                bool hit = ((md >> l) & 1ull) != 0ull;
                if (!hit) {
                    const ItemHead h = LoadItemHead(V, hi - 1u - l);
                    hit = h.tag == kItemFill ? RectFill(V, h.item, h.it, R, lane) : RectPoly(V, h.item, h.it, R, lane);
                }
                if (hit) {
                    if (top == kHitNone) top = hi - 1u - l;
                    cnt += 1u;
                    if (!counts) {
                        done = true;
                        break;
                    }
                }
            }
        }
        if (lane == 0u) {
            Q.top_item[q] = top;
            if (counts) Q.n_hit[q] = cnt;
        }
    }
}

__global__ __launch_bounds__(kHitThreads) void pm_select_rect_kernel(SelectRectParams Q) {
    const SceneView &V = Q.V;
    const uint32_t lane = LaneId();
    const bool skip = (V.flags & kHitSkipTransparent) != 0;
    RectQ R;
    const bool valid = RectLoad(Q.rect, R);
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
                word = RectCircle(R, h.x0, h.y0, h.x1, h.y1, (h.w0 & kCircleEllipse) != 0);
            } else if (h.tag == kItemLine) {
                if (!(skip && ItemTransparent(h))) word = RectLine(R, h.it);
            } else if (h.tag == kItemFill) {
                cand = RectCandidate(R, h, true, skip);
            } else if (h.tag == kItemPoly) {
                cand = RectCandidate(R, h, false, skip);
            }
        }
        uint64_t m = __ballot(cand);
        while (m != 0ull) {   // every candidate is finished: no item's word waits for another's
            const uint32_t l = TakeLowestLane(m);
            const ItemHead h = LoadItemHead(V, hi - 1u - l);
            const uint32_t npt = LoadU32(h.it + 12);
            const uint8_t *pts = V.scene + LoadU32(h.it + 16);
            bool touches, encloses;
            if (h.tag == kItemFill) {
                touches = RectFill(V, h.item, h.it, R, lane);
                encloses = RectEnclosesPoints(pts, npt, (LoadU32(h.it + 4) & kFillCompound) != 0, 0.0, R, lane);
            } else {
                const double hw = 0.5 * static_cast<double>(__uint_as_float(LoadU32(h.it + 8)));
                touches = RectPoly(V, h.item, h.it, R, lane);
                encloses = RectEnclosesPoints(pts, npt, false, hw, R, lane);
            }
            if (lane == l) word = (touches ? kSelTouches : 0u) | (encloses ? kSelEncloses : 0u);
        }
        if (mine) Q.item_flags[i] = word;
    }
}

void LaunchHitRects(const HitRectParams &p, uint32_t n_cus, hipStream_t stream) { LaunchQuery(pm_hit_rects_kernel, p, p.n, n_cus, stream); }

// ... or a wave per step of 64 items
void LaunchSelectRect(const SelectRectParams &p, uint32_t n_cus, hipStream_t stream) {
    LaunchQuery(pm_select_rect_kernel, p, ItemSteps(p.V.n_items), n_cus, stream);
}

}  // namespace pm
