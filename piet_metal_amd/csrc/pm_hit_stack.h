// pm_hit_stack_kernel, pm_hit_rects_stack_kernel: hit stacks -- for every query point (rectangle) the k topmost items that contain
// (touch) it, topmost first, and, if asked, how many do: select-behind, "the objects under the cursor".  Not on the frame path: like
// pm_hit_kernel they read the scene and the scene index, nothing a frame writes.  Included by pm_context.hip, whose unit they are
// compiled in.
//
// What the stack is is decision D24, a definition by reference: membership is D13's "contains" (points) or D19's
// "touches" (rectangles), a boolean per item.  Nothing here evaluates geometry of its own: the predicates are pm_hit_test.h's
// (HitFill, HitPoly; HitCircle, HitStroke) and pm_hit_rect.h's (RectLoad, RectCandidate, RectFill, RectPoly, RectLine, RectCircle), as
// they are -- same culls, same arithmetic --, the pieces (SceneView, FirstWaveUnit / GridWaves, LoadItemHead, TakeLowestLane,
// LaunchQuery) pm_query_common.h's.
//
// The walk is pm_hit_kernel's: one WAVE owns a query and goes through the items from the top of paint order down, 64 per step, the
// direct and the candidate ballots worked off from the topmost lane on.  Every hit is wave-uniform; lane 0 stores its index at
// items[q k + cnt] while cnt < k.  The walk ends at a hit that is opaque under PM_HIT_STOP_AT_OPAQUE (a third ballot of the step:
// a Circle, or an alpha byte of 255), at the k-th hit if no count was asked for, or at the bottom.  Then the lanes fill the words
// cnt .. k - 1 with PM_HIT_NONE.  The list lives in global memory only -- no LDS, no per-lane array: k is a loop bound and no
// register count --, offsets are 64-bit (q k reaches 2^38), and every loop exit depends on wave-uniform values alone.
#pragma once

#include "pm_hit_rect.h"
#include "pm_hit_test.h"

namespace pm {

// One launch of pm_hit_stack_kernel: n query points
struct HitStackParams {
    SceneView V;          // flags: PM_HIT_SKIP_TRANSPARENT, PM_HIT_STOP_AT_OPAQUE
    const float *xy;      // [2 n] {x, y} in scene coordinates
    uint32_t *items;      // [n k] the items that contain the point, topmost first, then PM_HIT_NONE
    uint32_t *n_hit;      // [n] the length of the stack, not clipped by k (nullptr: not asked for -- the walk may end at the k-th hit)
    uint32_t n, k;
};

// One launch of pm_hit_rects_stack_kernel: n query rectangles
struct HitRectStackParams {
    SceneView V;
    const float *rects;   // [4 n] {x0, y0, x1, y1}
    uint32_t *items;      // [n k] the items the rectangle touches, topmost first, then PM_HIT_NONE
    uint32_t *n_hit;      // [n] (nullptr: not asked for)
    uint32_t n, k;
};

namespace {

// the kernels' copies of the public constants: pm_context.hip asserts that they are include/piet_metal_amd.h's
constexpr uint32_t kHitStopAtOpaque = 8u;   // PM_HIT_STOP_AT_OPAQUE
constexpr uint32_t kHitStackMax = 256u;     // PM_HIT_STACK_MAX

// D24: a Circle is drawn opaque black; a Line, a Fill or a Polyline is opaque iff the alpha byte ItemTransparent reads is 255
__device__ __forceinline__ bool ItemOpaque(const ItemHead &h) {
    return h.tag == kItemCircle || (LoadU32(h.it + (h.tag == kItemPoly ? 4 : 8)) >> 24) == 0xffu;
}

// The words cnt .. k - 1 of a query's list (cnt >= k: none), strided over the wave
__device__ __forceinline__ void StackFill(uint32_t *out, uint32_t cnt, uint32_t k, uint32_t lane) {
    for (uint32_t j0 = cnt; j0 < k; j0 += 64u) {
        if (j0 + lane < k) out[j0 + lane] = kHitNone;
    }
}

}  // namespace

__global__ __launch_bounds__(kHitThreads) void pm_hit_stack_kernel(HitStackParams P) {
    const SceneView &V = P.V;
    const uint32_t lane = LaneId();
    const bool counts = P.n_hit != nullptr;
    const bool skip = (V.flags & kHitSkipTransparent) != 0;
    const bool stop = (V.flags & kHitStopAtOpaque) != 0;
    const uint32_t n_waves = GridWaves();
    for (uint32_t q = FirstWaveUnit(); q < P.n; q += n_waves) {
        const float2 pq = LoadF2(reinterpret_cast<const uint8_t *>(P.xy) + static_cast<size_t>(q) * 8);
        const uint32_t xb = UniformF32Bits(__float_as_uint(pq.x));
        const uint32_t yb = UniformF32Bits(__float_as_uint(pq.y));
        const double x = static_cast<double>(__uint_as_float(xb)), y = static_cast<double>(__uint_as_float(yb));
        uint32_t *out = P.items + static_cast<size_t>(q) * P.k;
        uint32_t cnt = 0;
        // (a non-finite coordinate hits nothing)
        bool done = !(RectFiniteBits(xb) && RectFiniteBits(yb));
        for (uint32_t hi = V.n_items; hi != 0u && !done; hi = hi > 64u ? hi - 64u : 0u) {
            // lane 0 looks at the topmost item of the step
            bool direct = false, cand = false, opaque = false;
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
                opaque = stop && (direct || cand) && ItemOpaque(h);
            }
            const uint64_t md = __ballot(direct), mo = __ballot(opaque);
            uint64_t m = md | __ballot(cand);
            while (m != 0ull) {
                const uint32_t l = TakeLowestLane(m);
                bool hit = ((md >> l) & 1ull) != 0ull;
                if (!hit) {
                    const ItemHead h = LoadItemHead(V, hi - 1u - l);
                    hit = h.tag == kItemFill ? HitFill(V, h.item, h.it, x, y, lane) : HitPoly(V, h.item, h.it, x, y, lane);
                }
                if (hit) {
                    if (cnt < P.k && lane == 0u) out[cnt] = hi - 1u - l;
                    cnt += 1u;
                    if (((mo >> l) & 1ull) != 0ull || (!counts && cnt == P.k)) {
                        done = true;
                        break;
                    }
                }
            }
        }
        StackFill(out, cnt, P.k, lane);
        if (counts && lane == 0u) P.n_hit[q] = cnt;
    }
}

__global__ __launch_bounds__(kHitThreads) void pm_hit_rects_stack_kernel(HitRectStackParams Q) {
    const SceneView &V = Q.V;
    const uint32_t lane = LaneId();
    const bool counts = Q.n_hit != nullptr;
    const bool skip = (V.flags & kHitSkipTransparent) != 0;
    const bool stop = (V.flags & kHitStopAtOpaque) != 0;
    const uint32_t n_waves = GridWaves();
    for (uint32_t q = FirstWaveUnit(); q < Q.n; q += n_waves) {
        RectQ R;
        const bool valid = RectLoad(Q.rects + static_cast<size_t>(q) * 4, R);
        uint32_t *out = Q.items + static_cast<size_t>(q) * Q.k;
        uint32_t cnt = 0;
        bool done = !valid;
        for (uint32_t hi = V.n_items; hi != 0u && !done; hi = hi > 64u ? hi - 64u : 0u) {
            // lane 0 looks at the topmost item of the step
            bool direct = false, cand = false, opaque = false;
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
                opaque = stop && (direct || cand) && ItemOpaque(h);
            }
            const uint64_t md = __ballot(direct), mo = __ballot(opaque);
            uint64_t m = md | __ballot(cand);
            while (m != 0ull) {
                const uint32_t l = TakeLowestLane(m);
                bool hit = ((md >> l) & 1ull) != 0ull;
                if (!hit) {
                    const ItemHead h = LoadItemHead(V, hi - 1u - l);
                    hit = h.tag == kItemFill ? RectFill(V, h.item, h.it, R, lane) : RectPoly(V, h.item, h.it, R, lane);
                }
                if (hit) {
                    if (cnt < Q.k && lane == 0u) out[cnt] = hi - 1u - l;
                    cnt += 1u;
                    if (((mo >> l) & 1ull) != 0ull || (!counts && cnt == Q.k)) {
                        done = true;
                        break;
                    }
                }
            }
        }
        StackFill(out, cnt, Q.k, lane);
        if (counts && lane == 0u) Q.n_hit[q] = cnt;
    }
}

void LaunchHitStack(const HitStackParams &p, uint32_t n_cus, hipStream_t stream) { LaunchQuery(pm_hit_stack_kernel, p, p.n, n_cus, stream); }

void LaunchHitRectsStack(const HitRectStackParams &p, uint32_t n_cus, hipStream_t stream) { LaunchQuery(pm_hit_rects_stack_kernel, p, p.n, n_cus, stream); }

}  // namespace pm
