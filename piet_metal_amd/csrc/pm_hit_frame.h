// pm_hit_frame_kernel: the item map -- for every pixel of a rectangle the LAST-painted item of the resident scene that contains
// the pixel's centre (and, if asked, how many do).  Decision D18: it is D13 (pm_hit_test.h) evaluated at (px + 0.5, py + 0.5) and
// nothing else, so every word equals what pm_hit_kernel answers for that point.  Not on the frame path; included by pm_context.hip.
// D13's predicates (HitWinding, HitStroke, HitCircle), the item head and the constants are pm_query_common.h's, as they are; the walk
// is the tile's own.
//
// One WORKGROUP of 256 threads owns a 16 x 16 tile of the rectangle (tiles are aligned to the rectangle's origin), thread t the
// pixel (t & 15, t >> 4).  What pm_hit_kernel does per query -- walk the items, test the chunk boxes, stream the segments -- the tile
// does once for its 256 queries:
//  * items are walked from the top of paint order down, kFrameItems per step, one per thread, and culled against the tile's
//    extent of pixel centres [xmin, xmax] x [ymin, ymax] (tightened to the rectangle's edge); the survivors are compacted in paint
//    order into LDS;
//  * per survivor, uniformly over the workgroup: a Circle or a Line is evaluated by every thread for its own pixel; a Fill's or a
//    Polyline's chunk boxes (for an item of more than kFrameChunks chunks its super-chunks' boxes first) are tested against the
//    extent kFrameChunks per round, the surviving chunk ids are compacted into LDS, and every thread runs through their segments
//    for its own pixel.  A round never holds more than kFrameChunks ids however long the item is.  A thread owns its pixel's
//    winding sum and stroke "or": nothing is reduced across lanes, and the order of the chunks cannot matter (an integer sum, an or);
//  * without a count a pixel is finished at its first hit and the tile's walk ends when every pixel of it inside the rectangle is.
//
// The cull is conservative with respect to D13.  Every rule drops a box only if pm_hit_kernel's rule for that box (proved in
// pm_hit_test.h) rejects EVERY query q of the extent:
//  * a ShortBbox edge at 0 or 65 535 is saturated and bounds nothing on its side;
//  * a Fill's box -- of the item, a chunk, a super-chunk -- adds 0 to q if it is wholly above (q.y < box.ymin), wholly below or
//    touching from below (q.y >= box.ymax; for the item's u16 box only q.y > box.ymax, which is what rounding outward allows) or
//    left of q (q.x > box.xmax).  For all q at once: ymax < box.ymin, ymin >= box.ymax, xmin > box.xmax.  A Fill to the RIGHT of
//    the tile is kept: its segments wind around every pixel to their left;
//  * a stroke's box, widened by hw for chunks, is dropped on four sides: xmax < lo, xmin > hi and the same in y;
//  * a Circle is its ShortBbox (HitCircle reads nothing else), all values are multiples of 0.5 below 2^17 and their squares and
//    quotients are well inside binary64: a centre beyond the box on any side is farther than the radius of that axis, exactly;
//  * an item whose colour has alpha 0 is skipped under PM_HIT_SKIP_TRANSPARENT, as in pm_hit_kernel;
//  * nothing else is culled: a Line is simply evaluated.
// Every box test is written so that a NaN compares "not passing" and no loop's trip count depends on a box.
// A thread also skips the chunks whose box pm_hit_kernel's own per-query test rejects for its pixel; the segments it does
// evaluate are a superset of pm_hit_kernel's, and D13 gives every segment outside that set a contribution of 0.
#pragma once

#include "pm_query_common.h"

namespace pm {

// One launch of pm_hit_frame_kernel: the w x h pixels from (x0, y0) against the resident scene and its index.
struct HitFrameParams {
    SceneView V;
    uint32_t *top_item;   // [h][stride], words beyond w in a row are not written
    uint32_t *n_hit;      // the same (nullptr: not asked for -- a pixel is finished at its first hit)
    size_t stride;        // in 32-bit elements
    uint32_t x0, y0, w, h;   // x0 + w <= 65 536, y0 + h <= 65 536: every centre is exact in f32
    uint32_t tiles_x, n_tiles;
};

namespace {

constexpr uint32_t kFrameTile = 16;      // a tile is kFrameTile x kFrameTile pixels, a thread each
constexpr int kFrameThreads = 256;
constexpr int kFrameWaves = kFrameThreads / 64;
constexpr uint32_t kFrameItems = 256;    // items per step of the walk
constexpr uint32_t kFrameChunks = 256;   // chunk ids (and super-chunk ids) per round: what the LDS lists hold
constexpr uint32_t kFrameSupers = kFrameChunks / kSuperChunks;   // surviving super-chunks expanded per round
static_assert(kFrameItems == kFrameThreads && kFrameChunks == kFrameThreads && kFrameTile * kFrameTile == kFrameThreads, "a thread per entry");

// The tile's queries: the extent of its pixel centres inside the rectangle, and this thread's own.
struct FrameTile {
    double xmin, xmax, ymin, ymax;   // workgroup-uniform
    double x, y;
    bool live;                       // this thread still has a question to answer
};

__device__ __forceinline__ uint32_t Uniform(uint32_t v) { return static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(static_cast<int>(v))); }

// Does a Fill's chunk or super-chunk box hold a segment that can count for some query of the tile / for this thread's
__device__ __forceinline__ bool FrameFillBoxTile(float4 bb, const FrameTile &T) {
    return static_cast<double>(bb.y) <= T.ymax && T.ymin < static_cast<double>(bb.w) && static_cast<double>(bb.z) >= T.xmin;
}
__device__ __forceinline__ bool FrameFillBoxOwn(float4 bb, const FrameTile &T) {
    return static_cast<double>(bb.y) <= T.y && T.y < static_cast<double>(bb.w) && static_cast<double>(bb.z) >= T.x;
}
__device__ __forceinline__ bool FramePolyBoxTile(float4 bb, double hw, const FrameTile &T) {
    return T.xmax >= static_cast<double>(bb.x) - hw && T.xmin <= static_cast<double>(bb.z) + hw && T.ymax >= static_cast<double>(bb.y) - hw &&
           T.ymin <= static_cast<double>(bb.w) + hw;
}
__device__ __forceinline__ bool FramePolyBoxOwn(float4 bb, double hw, const FrameTile &T) {
    return !(T.x < static_cast<double>(bb.x) - hw || T.x > static_cast<double>(bb.z) + hw || T.y < static_cast<double>(bb.y) - hw ||
             T.y > static_cast<double>(bb.w) + hw);
}

// The chunks [cb0, cb1) of one item against the tile, workgroup-uniform: work(c) runs on EVERY thread for every chunk c whose box
// passes pass() (c is a scalar; the order of the calls is that of the compaction, which no caller may depend on).  Up to
// kFrameChunks chunks: one round, a chunk per thread.  More: the super-chunks that hold them are tested kFrameChunks per round
// and the survivors expanded kFrameSupers at a time -- thread 8 r + u takes chunk u of the r-th of them (a super-chunk's box is
// the union of eight consecutive entries of the GLOBAL chunk table: the neighbouring items' chunks only make it larger, and
// the chunks outside [cb0, cb1) are not this item's).
template <typename Pass, typename Work>
__device__ __forceinline__ void ForTileChunks(const SceneView &V, uint32_t cb0, uint32_t cb1, uint32_t t, uint32_t *s_part, uint32_t *s_sup,
                                              uint32_t *s_chunk, Pass &&pass, Work &&work) {
    auto round = [&](bool mine, uint32_t c) {   // one round: compact the passing chunk ids, then everyone works them off
        uint32_t n = 0;
        const uint32_t r = BlockRank<kFrameWaves>(mine, s_part, &n);   // (its first barrier is behind every read of the round before)
        if (mine) s_chunk[r] = c;
        LdsBarrier();
        n = Uniform(n);
        for (uint32_t j = 0; j < n; ++j) work(Uniform(s_chunk[j]));
    };
    if (cb1 - cb0 <= kFrameChunks) {
        const uint32_t c = cb0 + t;
        round(c < cb1 && pass(V.chunk_bbox[c < cb1 ? c : cb0]), c);
        return;
    }
    const uint32_t g1 = (cb1 - 1u) / kSuperChunks + 1u;
    for (uint32_t gb = cb0 / kSuperChunks; gb < g1; gb += kFrameChunks) {
        const uint32_t g = gb + t;
        const bool keep = g < g1 && pass(V.sup_bbox[g < g1 ? g : gb]);
        uint32_t ns = 0;
        const uint32_t r = BlockRank<kFrameWaves>(keep, s_part, &ns);
        if (keep) s_sup[r] = g;
        LdsBarrier();
        ns = Uniform(ns);
        for (uint32_t sb = 0; sb < ns; sb += kFrameSupers) {
            const uint32_t at = sb + t / kSuperChunks;
            const uint32_t c = at < ns ? s_sup[at] * kSuperChunks + (t % kSuperChunks) : cb1;
            const bool in = c >= cb0 && c < cb1;
            round(in && pass(V.chunk_bbox[in ? c : cb0]), c);
        }
    }
}

}  // namespace

__global__ __launch_bounds__(kFrameThreads) void pm_hit_frame_kernel(HitFrameParams P) {
    __shared__ uint32_t s_cand[kFrameItems];    // the step's surviving items, topmost first
    __shared__ uint32_t s_sup[kFrameChunks];    // a round's surviving super-chunks
    __shared__ uint32_t s_chunk[kFrameChunks];  // a round's surviving chunks
    __shared__ uint32_t s_part[kFrameWaves];    // BlockRank's
    __shared__ uint32_t s_live[2][kFrameWaves]; // waves with a live pixel, two generations (one barrier per look)
    const SceneView &V = P.V;
    const uint32_t t = threadIdx.x;
    const uint32_t wave = t >> 6;
    const bool counts = P.n_hit != nullptr;
    const bool skip = (V.flags & kHitSkipTransparent) != 0;
    for (uint32_t tile = blockIdx.x; tile < P.n_tiles; tile += gridDim.x) {
        const uint32_t ox = (tile % P.tiles_x) * kFrameTile, oy = (tile / P.tiles_x) * kFrameTile;   // in the rectangle
        const uint32_t ix = ox + (t % kFrameTile), iy = oy + (t / kFrameTile);
        const bool inside = ix < P.w && iy < P.h;   // (a partial tile's other threads store nothing and keep no walk alive)
        FrameTile T;
        T.xmin = static_cast<double>(P.x0 + ox) + 0.5;
        T.ymin = static_cast<double>(P.y0 + oy) + 0.5;
        T.xmax = static_cast<double>(P.x0 + min(ox + kFrameTile, P.w) - 1u) + 0.5;
        T.ymax = static_cast<double>(P.y0 + min(oy + kFrameTile, P.h) - 1u) + 0.5;
        T.x = static_cast<double>(P.x0 + ix) + 0.5;
        T.y = static_cast<double>(P.y0 + iy) + 0.5;
        T.live = inside;
        uint32_t top = kHitNone, cnt = 0, looks = 0;
        bool tile_done = false;
        for (uint32_t hi = V.n_items; hi != 0u && !tile_done; hi = hi > kFrameItems ? hi - kFrameItems : 0u) {
            // thread 0 looks at the topmost item of the step
            bool keep = false;
            const uint32_t mine = hi - 1u - t;
            if (t < hi) {
                const ItemHead h = LoadItemHead(V, mine);
                const uint32_t tag = h.tag, x0 = h.x0, y0 = h.y0, x1 = h.x1, y1 = h.y1;
                if (tag == kItemCircle) {  // the box IS the shape: no edge of it is "saturated"
                    keep = !(T.ymax < static_cast<double>(y0) || T.ymin > static_cast<double>(y1) || T.xmax < static_cast<double>(x0) ||
                             T.xmin > static_cast<double>(x1));
                } else {
                    // the box as bounds in binary64: an edge at a saturated value bounds nothing
                    const bool above = y0 != 0u && T.ymax < static_cast<double>(y0), below = y1 != 0xffffu && T.ymin > static_cast<double>(y1);
                    const bool left = x0 != 0u && T.xmax < static_cast<double>(x0), right = x1 != 0xffffu && T.xmin > static_cast<double>(x1);
                    if (tag == kItemLine) {
                        keep = !(skip && ItemTransparent(h));
                    } else if (tag == kItemFill) {
                        keep = !(above || below || right) && !(skip && ItemTransparent(h));
                    } else if (tag == kItemPoly) {
                        keep = !(above || below || left || right) && !(skip && ItemTransparent(h));
                    }
                }
            }
            uint32_t n_cand = 0;
            const uint32_t rank = BlockRank<kFrameWaves>(keep, s_part, &n_cand);
            if (keep) s_cand[rank] = mine;
            LdsBarrier();
            n_cand = Uniform(n_cand);
            for (uint32_t k = 0; k < n_cand; ++k) {
                if (!counts) {  // is any pixel of the tile still unanswered (only those inside the rectangle ever were)
                    const uint64_t m = __ballot(T.live);
                    if (LaneId() == 0u) s_live[looks & 1u][wave] = m != 0ull ? 1u : 0u;
                    LdsBarrier();
                    uint32_t any = 0;
#pragma unroll
                    for (int w = 0; w < kFrameWaves; ++w) any |= s_live[looks & 1u][w];
                    looks += 1u;
                    if (Uniform(any) == 0u) {
                        tile_done = true;
                        break;
                    }
                }
                const uint32_t i = Uniform(s_cand[k]);
                const ItemHead h = LoadItemHead(V, i);
                const uint8_t *it = h.it;
                const uint32_t tag = h.tag;
                bool hit = false;
                if (tag == kItemCircle) {
                    if (T.live) hit = HitCircle(h.x0, h.y0, h.x1, h.y1, (h.w0 & kCircleEllipse) != 0, T.x, T.y);
                } else if (tag == kItemLine) {
                    if (T.live) {
                        const double hw = 0.5 * static_cast<double>(__uint_as_float(LoadU32(it + 12)));
                        hit = HitStroke(LoadF2(it + 16), LoadF2(it + 24), T.x, T.y, hw * hw);
                    }
                } else if (tag == kItemFill) {
                    const uint32_t flags = LoadU32(it + 4), npt = LoadU32(it + 12);
                    const uint8_t *pts = V.scene + LoadU32(it + 16);
                    const bool compound = (flags & kFillCompound) != 0;
                    const uint32_t cb0 = V.chunk_base[i], cb1 = V.chunk_base[i + 1];
                    int wsum = 0;
                    ForTileChunks(
                        V, cb0, cb1, t, s_part, s_sup, s_chunk, [&](float4 bb) { return FrameFillBoxTile(bb, T); },
                        [&](uint32_t c) {
                            if (!(T.live && FrameFillBoxOwn(V.chunk_bbox[c], T))) return;
                            const uint32_t k0 = (c - cb0) * kChunkSegs, k1 = min(k0 + kChunkSegs, FillSegs(npt));
                            for (uint32_t s = k0; s < k1; ++s) {
                                float2 a, b;
                                if (FillSegmentEnds(pts, npt, compound, s, a, b)) wsum += HitWinding(a, b, T.x, T.y);
                            }
                        });
                    hit = (flags & kFillEvenOdd) ? (wsum & 1) != 0 : wsum != 0;
                } else if (tag == kItemPoly) {
                    const uint32_t npt = LoadU32(it + 12);
                    const uint8_t *pts = V.scene + LoadU32(it + 16);
                    const double hw = 0.5 * static_cast<double>(__uint_as_float(LoadU32(it + 8)));
                    const double hw2 = hw * hw;
                    if (npt == 1u) {  // one degenerate segment (the scene index has no chunk for it)
                        const float2 a = LoadF2(pts);
                        hit = T.live && HitStroke(a, a, T.x, T.y, hw2);
                    } else if (npt != 0u) {
                        const uint32_t cb0 = V.chunk_base[i], cb1 = V.chunk_base[i + 1];
                        ForTileChunks(
                            V, cb0, cb1, t, s_part, s_sup, s_chunk, [&](float4 bb) { return FramePolyBoxTile(bb, hw, T); },
                            [&](uint32_t c) {
                                if (hit || !(T.live && FramePolyBoxOwn(V.chunk_bbox[c], hw, T))) return;
                                const uint32_t k0 = (c - cb0) * kChunkSegs, k1 = min(k0 + kChunkSegs, PolySegs(npt));
                                float2 a = LoadF2(pts + static_cast<size_t>(k0) * 8);
                                for (uint32_t s = k0; s < k1; ++s) {
                                    const float2 b = LoadF2(pts + static_cast<size_t>(s + 1u) * 8);
                                    hit = hit || HitStroke(a, b, T.x, T.y, hw2);
                                    a = b;
                                }
                            });
                    }
                }
                if (hit && T.live) {
                    if (top == kHitNone) top = i;
                    cnt += 1u;
                    if (!counts) T.live = false;
                }
            }
        }
        if (inside) {
            const size_t at = static_cast<size_t>(iy) * P.stride + ix;
            P.top_item[at] = top;
            if (counts) P.n_hit[at] = cnt;
        }
        LdsBarrier();   // (the next tile's first writes to s_cand / s_live are behind every read of this one)
    }
}

// grid: what the chip holds at once (eight workgroups of four waves per CU), or a workgroup per tile if that is less
void LaunchHitFrame(HitFrameParams p, uint32_t n_cus, hipStream_t stream) {
    if (p.w == 0u || p.h == 0u) return;
    p.tiles_x = (p.w + kFrameTile - 1u) / kFrameTile;
    p.n_tiles = p.tiles_x * ((p.h + kFrameTile - 1u) / kFrameTile);   // (at most 4096 x 4096)
    const uint32_t grid = min(p.n_tiles, max(n_cus, 1u) * 8u);
    hipLaunchKernelGGL(pm_hit_frame_kernel, dim3(grid), dim3(kFrameThreads), 0, stream, p);
}

}  // namespace pm
