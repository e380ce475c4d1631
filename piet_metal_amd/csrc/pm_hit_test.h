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
// Without a count the walk ends at the first hit.
//
// Culling is conservative with respect to D13:
//  * a ShortBbox saturates at 0 and 65 535, so a box edge AT those values bounds nothing on its side;
//  * a Fill segment counts only if a.y <= y < b.y (or b.y <= y < a.y) and the query is not to the right of both of its ends
//    (there s <= 0 on a rising and s >= 0 on a falling segment: the two products are of factors ordered the same way, and
//    rounding is monotonic): a box -- of the item, a chunk or a super-chunk -- wholly above, below or left of the query adds 0;
//  * a stroke's boxes are widened by hw.  A query outside the widened box by one f32 step is farther than hw from the
//    segment by a relative 6e-8, eight orders of magnitude more than the binary64 roundings of the distance can hide.
#pragma once

#include "pm_kernels_common.h"

namespace pm {

// One launch of pm_hit_kernel: n query points against the resident scene and its index.
struct HitParams {
    const uint8_t *scene;
    uint32_t n_items, items_ix, bbox_ix;  // the drawn group, as in FrameParams
    const uint32_t *chunk_base;
    const float4 *chunk_bbox;
    const float4 *sup_bbox;
    const float *xy;      // [2 n] {x, y} in scene coordinates
    uint32_t *top_item;   // [n] last-painted item that contains the point, or 0xffffffff
    uint32_t *n_hit;      // [n] items that contain it (nullptr: not asked for -- the walk ends at the first hit)
    uint32_t n;
    uint32_t flags;       // PM_HIT_*
};

namespace {

constexpr int kHitWaves = 4;
constexpr int kHitThreads = 64 * kHitWaves;
constexpr uint32_t kHitNone = 0xffffffffu;         // PM_HIT_NONE
constexpr uint32_t kHitSkipTransparent = 1u;       // PM_HIT_SKIP_TRANSPARENT

// D13, Fill: what segment a -> b adds to the winding sum of (x, y)
__device__ __forceinline__ int HitWinding(float2 a, float2 b, double x, double y) {
    const double ax = a.x, ay = a.y, bx = b.x, by = b.y;
    const double s = (bx - ax) * (y - ay) - (x - ax) * (by - ay);
    int w = 0;
    if (ay <= y && y < by && s > 0.0) w = 1;
    if (by <= y && y < ay && s < 0.0) w = -1;
    return w;
}

// D13, Line and Polyline: is (x, y) within hw of segment a -> b (hw2 = hw * hw)
__device__ __forceinline__ bool HitStroke(float2 a, float2 b, double x, double y, double hw2) {
    const double ax = a.x, ay = a.y;
    const double abx = static_cast<double>(b.x) - ax, aby = static_cast<double>(b.y) - ay;
    const double apx = x - ax, apy = y - ay;
    const double L = abx * abx + aby * aby;
    double t = 0.0;
    if (L != 0.0) t = fmin(fmax((apx * abx + apy * aby) / L, 0.0), 1.0);
    const double cx = ax + abx * t, cy = ay + aby * t;
    const double dx = x - cx, dy = y - cy;
    return dx * dx + dy * dy <= hw2;
}

// D13, Circle / ellipse: from the item's ShortBbox alone
__device__ __forceinline__ bool HitCircle(uint32_t x0, uint32_t y0, uint32_t x1, uint32_t y1, bool ellipse, double x, double y) {
    const double fx0 = static_cast<double>(x0), fy0 = static_cast<double>(y0);
    const double cx = (fx0 + static_cast<double>(x1)) * 0.5, cy = (fy0 + static_cast<double>(y1)) * 0.5;
    const double rx = cx - fx0, ry = cy - fy0;
    const double dx = x - cx, dy = y - cy;
    if (ellipse) return rx > 0.0 && ry > 0.0 && (dx / rx) * (dx / rx) + (dy / ry) * (dy / ry) <= 1.0;
    const double r = fmin(rx, ry);
    return dx * dx + dy * dy <= r * r;
}

// The chunks [cb0, cb1) of one item, spread over the lanes: work(c) runs on ONE lane for every chunk c whose box passes
// (divergent: no cross-lane operation inside); after every round the uniform done() may end the walk.  Up to 64 chunks: one
// round, a chunk per lane.  More: the super-chunks that hold them are tested first, 64 per round, and the survivors are worked
// off eight at a time -- lane 8 r + u takes chunk u of the r-th surviving super-chunk (a super-chunk's box is the union of
// eight consecutive entries of the GLOBAL chunk table: chunks of the neighbouring items only make it larger).
template <typename Pass, typename Work, typename Done>
__device__ __forceinline__ void ForItemChunks(const HitParams &P, uint32_t cb0, uint32_t cb1, uint32_t lane, Pass &&pass, Work &&work, Done &&done) {
    if (cb1 - cb0 <= 64u) {
        const uint32_t c = cb0 + lane;
        if (c < cb1 && pass(P.chunk_bbox[c])) work(c);
        (void)done();
        return;
    }
    const uint32_t g1 = (cb1 - 1u) / kSuperChunks + 1u;
    for (uint32_t gb = cb0 / kSuperChunks; gb < g1; gb += 64u) {
        const uint32_t g = gb + lane;
        uint64_t m = __ballot(g < g1 && pass(P.sup_bbox[g < g1 ? g : gb]));
        while (m != 0ull) {
            uint64_t mine = m;  // ... with its r lowest bits cleared
            for (uint32_t k = 0; k < (lane >> 3); ++k) mine &= mine - 1ull;
            if (mine != 0ull) {
                const uint32_t c = (gb + static_cast<uint32_t>(__builtin_ctzll(mine))) * kSuperChunks + (lane & 7u);
                if (c >= cb0 && c < cb1 && pass(P.chunk_bbox[c])) work(c);
            }
            if (done()) return;
            for (uint32_t k = 0; k < 8u; ++k) m &= m - 1ull;
        }
    }
}

// Is (x, y) inside Fill item `item` (wave-uniform arguments and result)
__device__ __forceinline__ bool HitFill(const HitParams &P, uint32_t item, const uint8_t *it, double x, double y, uint32_t lane) {
    const uint32_t flags = LoadU32(it + 4), npt = LoadU32(it + 12);
    const uint8_t *pts = P.scene + LoadU32(it + 16);
    const bool compound = (flags & kFillCompound) != 0;
    const uint32_t cb0 = P.chunk_base[item], cb1 = P.chunk_base[item + 1];
    int w = 0;
    ForItemChunks(
        P, cb0, cb1, lane, [&](float4 bb) { return static_cast<double>(bb.y) <= y && y < static_cast<double>(bb.w) && static_cast<double>(bb.z) >= x; },
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
__device__ __forceinline__ bool HitPoly(const HitParams &P, uint32_t item, const uint8_t *it, double x, double y, uint32_t lane) {
    const uint32_t npt = LoadU32(it + 12);
    const uint8_t *pts = P.scene + LoadU32(it + 16);
    const double hw = 0.5 * static_cast<double>(__uint_as_float(LoadU32(it + 8)));
    const double hw2 = hw * hw;
    if (npt == 0u) return false;
    if (npt == 1u) {  // one degenerate segment (the scene index has no chunk for it)
        const float2 a = LoadF2(pts);
        return HitStroke(a, a, x, y, hw2);
    }
    const uint32_t cb0 = P.chunk_base[item], cb1 = P.chunk_base[item + 1];
    bool hit = false, any = false;
    ForItemChunks(
        P, cb0, cb1, lane,
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
    const uint32_t lane = LaneId();
    const uint32_t n_waves = gridDim.x * kHitWaves;
    const bool counts = P.n_hit != nullptr;
    const bool skip = (P.flags & kHitSkipTransparent) != 0;
    for (uint32_t q = blockIdx.x * kHitWaves + WaveId(); q < P.n; q += n_waves) {
        const float2 pq = LoadF2(reinterpret_cast<const uint8_t *>(P.xy) + static_cast<size_t>(q) * 8);
        const uint32_t xb = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(__float_as_uint(pq.x))));
        const uint32_t yb = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(__float_as_uint(pq.y))));
        const double x = static_cast<double>(__uint_as_float(xb)), y = static_cast<double>(__uint_as_float(yb));
        uint32_t top = kHitNone, cnt = 0;
        // (a non-finite coordinate hits nothing)
        bool done = (xb & 0x7f800000u) == 0x7f800000u || (yb & 0x7f800000u) == 0x7f800000u;
        for (uint32_t hi = P.n_items; hi != 0u && !done; hi = hi > 64u ? hi - 64u : 0u) {
            // lane 0 looks at the topmost item of the step
            bool direct = false, cand = false;
            if (lane < hi) {
                const uint32_t i = hi - 1u - lane;
                const uint8_t *it = P.scene + P.items_ix + static_cast<size_t>(i) * kItemSize;
                const uint32_t w0 = LoadU32(it);
                const uint32_t tag = w0 & 0xffffu;
                const uint2 bb = *reinterpret_cast<const uint2 *>(P.scene + P.bbox_ix + static_cast<size_t>(i) * sizeof(ShortBbox));
                const uint32_t x0 = bb.x & 0xffffu, y0 = bb.x >> 16, x1 = bb.y & 0xffffu, y1 = bb.y >> 16;
                // the box as bounds in binary64: an edge at a saturated value bounds nothing
                const bool above = y0 != 0u && y < static_cast<double>(y0), below = y1 != 0xffffu && y > static_cast<double>(y1);
                const bool left = x0 != 0u && x < static_cast<double>(x0), right = x1 != 0xffffu && x > static_cast<double>(x1);
                if (tag == kItemCircle) {
                    direct = HitCircle(x0, y0, x1, y1, (w0 & kCircleEllipse) != 0, x, y);
                } else if (tag == kItemLine) {
                    if (!(skip && (LoadU32(it + 8) >> 24) == 0u)) {
                        const double hw = 0.5 * static_cast<double>(__uint_as_float(LoadU32(it + 12)));
                        direct = HitStroke(LoadF2(it + 16), LoadF2(it + 24), x, y, hw * hw);
                    }
                } else if (tag == kItemFill) {
                    cand = !(above || below || right) && !(skip && (LoadU32(it + 8) >> 24) == 0u);
                } else if (tag == kItemPoly) {
                    cand = !(above || below || left || right) && !(skip && (LoadU32(it + 4) >> 24) == 0u);
                }
            }
            const uint64_t md = __ballot(direct);
            uint64_t m = md | __ballot(cand);
            while (m != 0ull) {
                const uint32_t l = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(__builtin_ctzll(m)));
                m &= m - 1ull;
                bool hit = ((md >> l) & 1ull) != 0ull;
                if (!hit) {
                    const uint32_t i = hi - 1u - l;
                    const uint8_t *it = P.scene + P.items_ix + static_cast<size_t>(i) * kItemSize;
                    hit = (LoadU32(it) & 0xffffu) == kItemFill ? HitFill(P, i, it, x, y, lane) : HitPoly(P, i, it, x, y, lane);
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

// grid: what the chip holds at once (eight workgroups of four waves per CU), or a wave per query if that is less
void LaunchHitTest(const HitParams &p, uint32_t n_cus, hipStream_t stream) {
    if (p.n == 0u) return;
    const uint32_t grid = min((p.n + kHitWaves - 1u) / kHitWaves, max(n_cus, 1u) * 8u);
    hipLaunchKernelGGL(pm_hit_kernel, dim3(grid), dim3(kHitThreads), 0, stream, p);
}

}  // namespace pm
