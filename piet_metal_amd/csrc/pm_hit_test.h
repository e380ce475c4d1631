// pm_hit_kernel: point hit testing -- for every query point the LAST-painted item of the resident scene that contains it
// (and, if asked, how many do).  Not on the frame path: it reads the scene and the scene index (pm_index_kernel), nothing a
// frame writes.  Included by pm_context.hip, whose unit it is compiled in (the frame path's units stay as they are).
//
// What "contains" means is decision D13: every predicate below is binary64 arithmetic on the scene's f32 / u16
// values, one rounding per written operation, in the written order (-ffp-contract=off) -- tests/np_hit.py states the same
// operations in numpy and the two must agree bit for bit.
//
// One WAVE owns a query.  It walks the item list from the top of paint order downward, 64 items per step: every lane looks at
// one item -- a Circle or a Line is decided right there, a Fill or a Polyline becomes a candidate if the query can be inside by
// its box -- and the two ballots are worked off from the topmost lane on.  A candidate's chunks of kChunkSegs segments (the
// scene index) are spread over the lanes; an item of more than 64 chunks is first cut down by its super-chunks' boxes.  A Fill's
// winding is a sum of integers over the wave (the order of additions cannot change it), a stroke is an "any lane" ballot.
// Without a count the walk ends at the first hit.  The chunk walk (ForItemChunks), the item head and D13's segment and
// circle predicates are pm_query_common.h's, which the other query kernels share.
//
// Culling is conservative with respect to D13:
//  * a ShortBbox saturates at 0 and 65 535, so a box edge AT those values bounds nothing on its side;
//  * a Fill segment counts only if a.y <= y < b.y (or b.y <= y < a.y) and the query is not to the right of both of its ends
//    (there s <= 0 on a rising and s >= 0 on a falling segment: the two products are of factors ordered the same way, and
//    rounding is monotonic): a box -- of the item, a chunk or a super-chunk -- wholly above, below or left of the query adds 0;
//  * a stroke's boxes are widened by hw.  A query outside the widened box by one f32 step is farther than hw from the
//    segment by a relative 6e-8, eight orders of magnitude more than the binary64 roundings of the distance can hide.
#pragma once

#include "pm_query_common.h"

namespace pm {

// One launch of pm_hit_kernel: n query points against the resident scene and its index.
struct HitParams {
    SceneView V;
    const float *xy;      // [2 n] {x, y} in scene coordinates
    uint32_t *top_item;   // [n] last-painted item that contains the point, or 0xffffffff
    uint32_t *n_hit;      // [n] items that contain it (nullptr: not asked for -- the walk ends at the first hit)
    uint32_t n;
};

namespace {

// Is (x, y) inside Fill item `item` (wave-uniform arguments and result)
__device__ __forceinline__ bool HitFill(const SceneView &V, uint32_t item, const uint8_t *it, double x, double y, uint32_t lane) {
    const uint32_t flags = LoadU32(it + 4), npt = LoadU32(it + 12);
    const uint8_t *pts = V.scene + LoadU32(it + 16);
    const bool compound = (flags & kFillCompound) != 0;
    const uint32_t cb0 = V.chunk_base[item], cb1 = V.chunk_base[item + 1];
    int w = 0;
    ForItemChunks(
        V, cb0, cb1, lane, [&](float4 bb) { return static_cast<double>(bb.y) <= y && y < static_cast<double>(bb.w) && static_cast<double>(bb.z) >= x; },
        [&](uint32_t c) {
            const uint32_t k0 = (c - cb0) * kChunkSegs, k1 = min(k0 + kChunkSegs, FillSegs(npt));
            for (uint32_t k = k0; k < k1; ++k) {
                float2 a, b;
                if (FillSegmentEnds(pts, npt, compound, k, a, b)) w += HitWinding(a, b, x, y);
            }
        },
        [] { return false; });
    if (__ballot(w != 0) == 0ull) return false;
    const int sum = static_cast<int>(WaveLast(WaveInclusiveScan(static_cast<uint32_t>(w))));
    return (flags & kFillEvenOdd) ? (sum & 1) != 0 : sum != 0;
}

// Is (x, y) within half the width of Polyline item `item`
__device__ __forceinline__ bool HitPoly(const SceneView &V, uint32_t item, const uint8_t *it, double x, double y, uint32_t lane) {
    const uint32_t npt = LoadU32(it + 12);
    const uint8_t *pts = V.scene + LoadU32(it + 16);
    const double hw = 0.5 * static_cast<double>(__uint_as_float(LoadU32(it + 8)));
    const double hw2 = hw * hw;
    if (npt == 0u) return false;
    if (npt == 1u) {  // one degenerate segment (the scene index has no chunk for it)
        const float2 a = LoadF2(pts);
        return HitStroke(a, a, x, y, hw2);
    }
    const uint32_t cb0 = V.chunk_base[item], cb1 = V.chunk_base[item + 1];
    bool hit = false, any = false;
    ForItemChunks(
        V, cb0, cb1, lane,
        [&](float4 bb) {
            return !(x < static_cast<double>(bb.x) - hw || x > static_cast<double>(bb.z) + hw || y < static_cast<double>(bb.y) - hw ||
                     y > static_cast<double>(bb.w) + hw);
        },
        [&](uint32_t c) {
            const uint32_t k0 = (c - cb0) * kChunkSegs, k1 = min(k0 + kChunkSegs, PolySegs(npt));
            float2 a = LoadF2(pts + static_cast<size_t>(k0) * 8);
            for (uint32_t k = k0; k < k1; ++k) {
                const float2 b = LoadF2(pts + static_cast<size_t>(k + 1u) * 8);
                hit = hit || HitStroke(a, b, x, y, hw2);
                a = b;
            }
        },
        [&] {
            any = __ballot(hit) != 0ull;
            return any;
        });
    return any;
}

}  // namespace

__global__ __launch_bounds__(kHitThreads) void pm_hit_kernel(HitParams P) {
    const SceneView &V = P.V;
    const uint32_t lane = LaneId();
    const bool counts = P.n_hit != nullptr;
    const bool skip = (V.flags & kHitSkipTransparent) != 0;
    const uint32_t n_waves = GridWaves();
    for (uint32_t q = FirstWaveUnit(); q < P.n; q += n_waves) {
        const float2 pq = LoadF2(reinterpret_cast<const uint8_t *>(P.xy) + static_cast<size_t>(q) * 8);
        const uint32_t xb = UniformF32Bits(__float_as_uint(pq.x));
        const uint32_t yb = UniformF32Bits(__float_as_uint(pq.y));
        const double x = static_cast<double>(__uint_as_float(xb)), y = static_cast<double>(__uint_as_float(yb));
        uint32_t top = kHitNone, cnt = 0;
        // (a non-finite coordinate hits nothing)
        bool done = !(RectFiniteBits(xb) && RectFiniteBits(yb));
        for (uint32_t hi = V.n_items; hi != 0u && !done; hi = hi > 64u ? hi - 64u : 0u) {
            // lane 0 looks at the topmost item of the step
            bool direct = false, cand = false;
            if (lane < hi) {
                const ItemHead h = LoadItemHead(V, hi - 1u - lane);
                // the box as bounds in binary64: an edge at a saturated value bounds nothing
                const bool above = h.y0 != 0u && y < static_cast<double>(h.y0), below = h.y1 != 0xffffu && y > static_cast<double>(h.y1);
                const bool left = h.x0 != 0u && x < static_cast<double>(h.x0), right = h.x1 != 0xffffu && x > static_cast<double>(h.x1);
                if (h.tag == kItemCircle) {
                    direct = HitCircle(h.x0, h.y0, h.x1, h.y1, (h.w0 & kCircleEllipse) != 0, x, y);
                } else if (h.tag == kItemLine) {
                    if (!(skip && ItemTransparent(h))) {
                        const double hw = 0.5 * static_cast<double>(__uint_as_float(LoadU32(h.it + 12)));
                        direct = HitStroke(LoadF2(h.it + 16), LoadF2(h.it + 24), x, y, hw * hw);
                    }
                } else if (h.tag == kItemFill) {
                    cand = !(above || below || right) && !(skip && ItemTransparent(h));
                } else if (h.tag == kItemPoly) {
                    cand = !(above || below || left || right) && !(skip && ItemTransparent(h));
                }
            }
            const uint64_t md = __ballot(direct);
            uint64_t m = md | __ballot(cand);
            while (m != 0ull) {
                const uint32_t l = TakeLowestLane(m);
                bool hit = ((md >> l) & 1ull) != 0ull;
                if (!hit) {
                    const ItemHead h = LoadItemHead(V, hi - 1u - l);
                    hit = h.tag == kItemFill ? HitFill(V, h.item, h.it, x, y, lane) : HitPoly(V, h.item, h.it, x, y, lane);
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
            P.top_item[q] = top;
            if (counts) P.n_hit[q] = cnt;
        }
    }
}

void LaunchHitTest(const HitParams &p, uint32_t n_cus, hipStream_t stream) { LaunchQuery(pm_hit_kernel, p, p.n, n_cus, stream); }

}  // namespace pm
