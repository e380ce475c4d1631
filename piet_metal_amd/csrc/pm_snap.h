// pm_snap_kernel: snapping -- for every query {x, y, r} the nearest vertex and the nearest point of an edge of the resident scene
// within r of (x, y): which item, which vertex or which point of which segment, and how far.  Not on the frame path: like the
// other query kernels it reads the scene and the scene index, nothing a frame writes.  Included by pm_context.hip; the item
// head, the chunk walk (ForItemChunks) and the constants are pm_query_common.h's, as they are.
//
// What an item offers, how far a candidate is and which one wins is decision D21: binary64 arithmetic on the
// scene's f32 / u16 values and the query's f32 values, one rounding per written operation, in the written order
// (-ffp-contract=off) -- tests/np_snap.py states the same operations in numpy and the records must agree byte for byte.  The
// distance to a segment is D13's own clamped projection (HitStroke), kept instead of compared.
//
// One WAVE owns a query, the launch shape of pm_hit_rects_kernel.  It walks the items 64 per step: a Circle or a Line is
// evaluated on its lane, a Fill or a Polyline becomes a candidate by its box against the query widened by r, and a candidate's
// chunks go through ForItemChunks, a chunk per lane.  Every lane keeps its own best vertex and its own best edge as a key --
// (d2's bit pattern, ~item << 32 | index): d2 >= 0, so the bits order as an unsigned integer, the larger item and then the
// smaller index win a tie -- together with the winner's point.  Nothing is reduced per item: at the end of the query the wave
// takes the lexicographic minimum of the keys (six butterfly steps), the lane that owns it hands over the point, and lane 0
// writes the 32-byte record with vector stores.  A minimum of a total order: how the candidates fall on the lanes, and in
// what order a lane meets them, cannot show.  No atomics, no LDS, no scratch.
//
// Culling is conservative with respect to D21.  A box is passed unless SnapBoxD2 -- the squared distance from the query to the
// box, by the decision's own operations -- exceeds r * r:
//  * for a vertex p in a box left of x, x - p.x >= x - hi, and every later step (the rounding of the difference, of its
//    square, of the sum of the two squares) is monotonic: D21's d2 of the vertex is >= the box's, whatever was rounded.  A
//    query exactly r from a vertex ON the box's edge has the box's d2 EQUAL to the vertex's: passed;
//  * the point c = a + ab * t of a segment lies between a and a + (b - a) in each coordinate (t is in [0, 1], rounding is
//    monotonic), and a + (b - a) is b itself unless b - a is inexact in binary64 -- two f32 values more than 2^29 apart in
//    magnitude.  Then two roundings stand between it and b: that of b - a, at most 2^-53 of |b - a| <= 2 M, and that of the
//    sum, at most 2^-53 of about M, where M is the larger of |a| and |b|: 3 * 2^-53 M in all.  A box that BOUNDS the segment's
//    ends on both sides of an axis has an edge value >= M there, so it is widened by 2^-50 of its larger edge value on every
//    side before the distance is taken: c lies in the widened box and the vertex argument holds for it;
//  * a chunk's box is the exact minimum and maximum of its points, NaNs ignored (a chunk of nothing but separators keeps an
//    empty box, which is never passed); a super-chunk's is a union of chunk boxes, chunks of the neighbouring items only make
//    it larger; a comparison with a NaN distance is false: passed;
//  * a ShortBbox saturates at 0 and 65 535, so a box edge AT those values bounds nothing on its side -- and then the OTHER side
//    of that axis bounds nothing either: an end of 1e30 beyond the saturated side absorbs the other end in b - a, and D21's own
//    c = a + ab * t comes out at 0, far outside the side the box does bound (M is not the box's to know).  An axis of a ShortBbox
//    counts only if neither of its two edges is saturated; every point is then within [0, 65 535] on it; a Polyline's item box holds
//    its width as well, which only makes it looser -- of a width >= 0.  D21 gives the width no part, so a Polyline whose width is
//    negative or NaN (its box is narrower than its points, or no box at all) is a candidate whatever its box says.
// The running best is NOT used to cull: r alone bounds the search.
#pragma once

#include "pm_query_common.h"

namespace pm {

// One launch of pm_snap_kernel
struct SnapParams {
    SceneView V;                 // flags: PM_HIT_SKIP_TRANSPARENT and PM_SNAP_VERTICES / PM_SNAP_EDGES
    const float *xyr;            // [3 n] {x, y, r}
    const uint32_t *skip_items;  // [n_items] a non-zero word takes the item out of the search (nullptr: none)
    uint8_t *out;                // [32 n] pm_snap_result
    uint32_t n;
};

namespace {

constexpr uint32_t kSnapVertices = 2u;    // PM_SNAP_VERTICES
constexpr uint32_t kSnapEdges = 4u;       // PM_SNAP_EDGES
constexpr uint32_t kSnapKindVertex = 1u;  // PM_SNAP_KIND_VERTEX
constexpr uint32_t kSnapKindEdge = 2u;    // PM_SNAP_KIND_EDGE

// The query in binary64 (wave-uniform) and what is asked of it
struct SnapQ {
    double x, y, r2;
    bool vertices, edges;
};

// D21 (and D23): query {x, y, r} at in[0 .. 2]; a non-finite value, or r < 0, snaps to nothing
__device__ __forceinline__ bool SnapLoad(const float *in, SnapQ &Q) {
    const uint32_t xb = UniformF32Bits(__float_as_uint(in[0]));
    const uint32_t yb = UniformF32Bits(__float_as_uint(in[1]));
    const uint32_t rb = UniformF32Bits(__float_as_uint(in[2]));
    const double r = static_cast<double>(__uint_as_float(rb));
    Q.x = static_cast<double>(__uint_as_float(xb));
    Q.y = static_cast<double>(__uint_as_float(yb));
    Q.r2 = r * r;
    return RectFiniteBits(xb) && RectFiniteBits(yb) && RectFiniteBits(rb) && !(r < 0.0);
}

// A lane's best candidate of one kind.  d2 = all ones: none yet (no qualifying d2 has that pattern: it is <= r * r, finite)
struct SnapBest {
    uint64_t d2 = ~0ull;
    uint64_t key = ~0ull;   // ~item << 32 | index
    float t = 0.0f, x = 0.0f, y = 0.0f;
};

__device__ __forceinline__ uint64_t SnapKey(uint32_t item, uint32_t index) { return (static_cast<uint64_t>(~item) << 32) | index; }

__device__ __forceinline__ void SnapOffer(SnapBest &best, double d2, double r2, uint32_t item, uint32_t index, float t, float x, float y) {
    if (!(d2 <= r2)) return;
    const uint64_t bits = __builtin_bit_cast(uint64_t, d2), key = SnapKey(item, index);
    if (bits < best.d2 || (bits == best.d2 && key < best.key)) {
        best.d2 = bits;
        best.key = key;
        best.t = t;
        best.x = x;
        best.y = y;
    }
}

// D21, a vertex
__device__ __forceinline__ void SnapVertex(SnapBest &best, const SnapQ &Q, float2 p, uint32_t item, uint32_t index) {
    if (!RectFinite(p)) return;
    const double dx = Q.x - static_cast<double>(p.x), dy = Q.y - static_cast<double>(p.y);
    SnapOffer(best, dx * dx + dy * dy, Q.r2, item, index, 0.0f, p.x, p.y);
}

// D21, an edge a -> b: HitStroke's operations
__device__ __forceinline__ void SnapEdge(SnapBest &best, const SnapQ &Q, float2 a, float2 b, uint32_t item, uint32_t index) {
    if (!(RectFinite(a) && RectFinite(b))) return;
    const double ax = a.x, ay = a.y;
    const double abx = static_cast<double>(b.x) - ax, aby = static_cast<double>(b.y) - ay;
    const double apx = Q.x - ax, apy = Q.y - ay;
    const double L = abx * abx + aby * aby;
    double t = 0.0;
    if (L != 0.0) t = fmin(fmax((apx * abx + apy * aby) / L, 0.0), 1.0);
    const double cx = ax + abx * t, cy = ay + aby * t;
    const double dx = Q.x - cx, dy = Q.y - cy;
    SnapOffer(best, dx * dx + dy * dy, Q.r2, item, index, static_cast<float>(t), static_cast<float>(cx), static_cast<float>(cy));
}

// The squared distance from the query to the box [x0, x1] x [y0, y1], widened (see above), by D21's operations; lo_* / hi_*
// false: the box does not bound that side.  A NaN edge gives 0 on its axis (fmax returns its other argument).
__device__ __forceinline__ double SnapBoxD2(const SnapQ &Q, double x0, double y0, double x1, double y1, bool lo_x, bool lo_y, bool hi_x, bool hi_y) {
    const double wx = 0x1p-50 * fmax(fabs(x0), fabs(x1)), wy = 0x1p-50 * fmax(fabs(y0), fabs(y1));
    double ex = 0.0, ey = 0.0;
    if (lo_x) ex = fmax(ex, (x0 - wx) - Q.x);
    if (hi_x) ex = fmax(ex, Q.x - (x1 + wx));
    if (lo_y) ey = fmax(ey, (y0 - wy) - Q.y);
    if (hi_y) ey = fmax(ey, Q.y - (y1 + wy));
    return ex * ex + ey * ey;
}

__device__ __forceinline__ bool SnapPass(const SnapQ &Q, float4 bb) {
    return !(SnapBoxD2(Q, bb.x, bb.y, bb.z, bb.w, true, true, true, true) > Q.r2);
}

// Fill item `item` (wave-uniform arguments): every entry k is met once, as the start of its segment
__device__ __forceinline__ void SnapFill(const SceneView &V, uint32_t item, const uint8_t *it, const SnapQ &Q, uint32_t lane, SnapBest &bv, SnapBest &be) {
    const uint32_t flags = LoadU32(it + 4), npt = LoadU32(it + 12);
    const uint8_t *pts = V.scene + LoadU32(it + 16);
    const bool compound = (flags & kFillCompound) != 0;
    const uint32_t cb0 = V.chunk_base[item], cb1 = V.chunk_base[item + 1];
    ForItemChunks(
        V, cb0, cb1, lane, [&](float4 bb) { return SnapPass(Q, bb); },
        [&](uint32_t c) {
            const uint32_t k0 = (c - cb0) * kChunkSegs, k1 = min(k0 + kChunkSegs, FillSegs(npt));
            for (uint32_t k = k0; k < k1; ++k) {
                float2 a, b;
                if (!FillSegmentEnds(pts, npt, compound, k, a, b)) continue;   // (a separator: no vertex, no segment)
                if (Q.vertices) SnapVertex(bv, Q, a, item, k);
                if (Q.edges) SnapEdge(be, Q, a, b, item, k);
            }
        },
        [] { return false; });
}

// Polyline item `item`: point k is met as the start of segment k, the last point as the end of the last segment
__device__ __forceinline__ void SnapPoly(const SceneView &V, uint32_t item, const uint8_t *it, const SnapQ &Q, uint32_t lane, SnapBest &bv, SnapBest &be) {
    const uint32_t npt = LoadU32(it + 12);
    const uint8_t *pts = V.scene + LoadU32(it + 16);
    if (npt == 0u) return;
    if (npt == 1u) {  // one vertex and one degenerate segment (the scene index has no chunk for it)
        if (lane == 0u) {
            const float2 a = LoadF2(pts);
            if (Q.vertices) SnapVertex(bv, Q, a, item, 0u);
            if (Q.edges) SnapEdge(be, Q, a, a, item, 0u);
        }
        return;
    }
    const uint32_t cb0 = V.chunk_base[item], cb1 = V.chunk_base[item + 1];
    ForItemChunks(
        V, cb0, cb1, lane, [&](float4 bb) { return SnapPass(Q, bb); },
        [&](uint32_t c) {
            const uint32_t k0 = (c - cb0) * kChunkSegs, k1 = min(k0 + kChunkSegs, PolySegs(npt));
            float2 a = LoadF2(pts + static_cast<size_t>(k0) * 8);
            for (uint32_t k = k0; k < k1; ++k) {
                const float2 b = LoadF2(pts + static_cast<size_t>(k + 1u) * 8);
                if (Q.vertices) {
                    SnapVertex(bv, Q, a, item, k);
                    if (k + 2u == npt) SnapVertex(bv, Q, b, item, k + 1u);
                }
                if (Q.edges) SnapEdge(be, Q, a, b, item, k);
                a = b;
            }
        },
        [] { return false; });
}

// Is the ShortBbox of a Fill or a Polyline a reason to look at it: an axis with an edge at a saturated value bounds nothing
__device__ __forceinline__ bool SnapCandidate(const SnapQ &Q, const ItemHead &h) {
    const bool bx = h.x0 != 0u && h.x1 != 0xffffu, by = h.y0 != 0u && h.y1 != 0xffffu;
    return !(SnapBoxD2(Q, static_cast<double>(h.x0), static_cast<double>(h.y0), static_cast<double>(h.x1), static_cast<double>(h.y1), bx, by, bx, by) > Q.r2);
}

// The wave's minimum of (d2, key), in every lane
__device__ __forceinline__ void SnapWaveMin(uint64_t &d2, uint64_t &key) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t od = __shfl_xor(static_cast<unsigned long long>(d2), d, 64), ok = __shfl_xor(static_cast<unsigned long long>(key), d, 64);
        if (od < d2 || (od == d2 && ok < key)) {
            d2 = od;
            key = ok;
        }
    }
}

}  // namespace

__global__ __launch_bounds__(kHitThreads) void pm_snap_kernel(SnapParams S) {
    const SceneView &V = S.V;
    const uint32_t lane = LaneId();
    const bool skip = (V.flags & kHitSkipTransparent) != 0;
    const uint32_t n_waves = GridWaves();
    for (uint32_t q = FirstWaveUnit(); q < S.n; q += n_waves) {
        SnapQ Q;
        const bool valid = SnapLoad(S.xyr + static_cast<size_t>(q) * 3, Q);
        Q.vertices = (V.flags & kSnapVertices) != 0;
        Q.edges = (V.flags & kSnapEdges) != 0;
        SnapBest bv, be;
        for (uint32_t hi = V.n_items; hi != 0u && valid; hi = hi > 64u ? hi - 64u : 0u) {
            // lane 0 looks at the topmost item of the step
            bool cand = false;
            if (lane < hi) {
                const ItemHead h = LoadItemHead(V, hi - 1u - lane);
                const uint32_t i = h.item;
                const bool taken_out = S.skip_items != nullptr && S.skip_items[i] != 0u;
                if (taken_out) {
                } else if (h.tag == kItemCircle) {
                    // D13's centre and radii, from the ShortBbox alone; the centre is exact in f32
                    const double fx0 = static_cast<double>(h.x0), fy0 = static_cast<double>(h.y0);
                    const double cx = (fx0 + static_cast<double>(h.x1)) * 0.5, cy = (fy0 + static_cast<double>(h.y1)) * 0.5;
                    const bool offers = (h.w0 & kCircleEllipse) == 0u || (cx - fx0 > 0.0 && cy - fy0 > 0.0);
                    if (Q.vertices && offers) SnapVertex(bv, Q, make_float2(static_cast<float>(cx), static_cast<float>(cy)), i, 0u);
                } else if (h.tag == kItemLine) {
                    if (!(skip && ItemTransparent(h))) {
                        const float2 a = LoadF2(h.it + 16), b = LoadF2(h.it + 24);
                        if (Q.vertices) {
                            SnapVertex(bv, Q, a, i, 0u);
                            SnapVertex(bv, Q, b, i, 1u);
                        }
                        if (Q.edges) SnapEdge(be, Q, a, b, i, 0u);
                    }
                } else if (h.tag == kItemFill) {
                    cand = SnapCandidate(Q, h) && !(skip && ItemTransparent(h));
                } else if (h.tag == kItemPoly) {
                    // (its box was made from the points and the width: of a width that is NaN or negative it bounds nothing)
                    const bool boxed = __uint_as_float(LoadU32(h.it + 8)) >= 0.0f;
                    cand = (!boxed || SnapCandidate(Q, h)) && !(skip && ItemTransparent(h));
                }
            }
            uint64_t m = __ballot(cand);
            while (m != 0ull) {   // every candidate is finished: the nearest may be in any of them
                const ItemHead h = LoadItemHead(V, hi - 1u - TakeLowestLane(m));
                if (h.tag == kItemFill) SnapFill(V, h.item, h.it, Q, lane, bv, be);
                else SnapPoly(V, h.item, h.it, Q, lane, bv, be);
            }
        }
        // D21: a qualifying vertex wins over every edge
        uint64_t d2 = bv.d2, key = bv.key;
        SnapWaveMin(d2, key);
        uint32_t kind = kSnapKindVertex;
        bool mine = bv.d2 == d2 && bv.key == key;
        float wt = bv.t, wx = bv.x, wy = bv.y;
        if (d2 == ~0ull) {
            d2 = be.d2;
            key = be.key;
            SnapWaveMin(d2, key);
            kind = kSnapKindEdge;
            mine = be.d2 == d2 && be.key == key;
            wt = be.t;
            wx = be.x;
            wy = be.y;
        }
        uint4 lo = make_uint4(kHitNone, 0u, 0u, 0u), up = make_uint4(0u, 0u, 0u, 0u);
        if (d2 != ~0ull) {   // (keys are unique: one lane owns the winner)
            const int l = __builtin_amdgcn_readfirstlane(__builtin_ctzll(__ballot(mine)));
            lo = make_uint4(~static_cast<uint32_t>(key >> 32), kind, static_cast<uint32_t>(key),
                            static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(__float_as_uint(wt)), l)));
            up = make_uint4(static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(__float_as_uint(wx)), l)),
                            static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(__float_as_uint(wy)), l)), static_cast<uint32_t>(d2),
                            static_cast<uint32_t>(d2 >> 32));
        }
        if (lane == 0u) {
            uint2 *rec = reinterpret_cast<uint2 *>(S.out + static_cast<size_t>(q) * 32);   // (8-byte aligned, as the record's double is)
            rec[0] = make_uint2(lo.x, lo.y);
            rec[1] = make_uint2(lo.z, lo.w);
            rec[2] = make_uint2(up.x, up.y);
            rec[3] = make_uint2(up.z, up.w);
        }
    }
}

void LaunchSnap(const SnapParams &p, uint32_t n_cus, hipStream_t stream) { LaunchQuery(pm_snap_kernel, p, p.n, n_cus, stream); }

}  // namespace pm
