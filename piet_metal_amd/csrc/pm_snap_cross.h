// pm_cross_kernel: snapping to intersections -- for every query {x, y, r} the nearest point within r of (x, y) where two edges of
// the resident scene cross: which two edges, where on each, where, and how far.  Not on the frame path: like the other query
// kernels it reads the scene and the scene index, nothing a frame writes.  Included by pm_context.hip after pm_snap.h, whose
// query (SnapQ, SnapLoad), edge distance (SnapEdge), culling (SnapBoxD2, SnapPass, SnapCandidate) and key (SnapKey) are used as they
// are; the item head and the chunk walk (ForItemChunks) are pm_query_common.h's.
//
// What an edge is, which edges are near, which pairs of them cross, where, and which pair wins is decision D23:
// binary64 arithmetic, one rounding per written operation, in the written order (-ffp-contract=off) -- tests/np_cross.py states
// the same operations in numpy and the 48-byte records must agree byte for byte.
//
// One WAVE owns a query, the launch shape of pm_snap_kernel, in two phases.
//  1. The near list.  pm_snap_kernel's item walk with edges only: an edge is NEAR iff D21's own d2 (SnapEdge) is <= r * r, so
//     the conservative cull argued in pm_snap.h holds word for word -- a culled box holds no near edge.  Near
//     edges go into a slice of LDS that belongs to the wave alone, kCrossMaxNear entries of {a, b, item, index}.  They are
//     appended in wave-uniform control flow only: ForItemChunks' per-lane work callback notes which of its chunk's <= 4 segments
//     are near and keeps their ends, its wave-uniform third callback ranks the noted segments with ballots and mbcnt and stores them
//     (the ends are kept in registers: loading them again at the append cost the compiler 256 VGPRs and 22 more); Lines and
//     one-point Polylines are evaluated on their item's lane and ranked once after the 64-item step.  The count goes on beyond
//     kCrossMaxNear without storing: more near edges than that is the answer "too many" (D23), a count, as order-free as the rest.
//  2. The pairs.  For i in [0, n_near) under scalar control the lanes take j = i + 1 + lane, + 64, ...: a lane orients its pair
//     by "precedes" (the smaller SnapKey), drops it if the edges share an end, applies D23's operations and keeps its best as
//     (d2's bits, first edge's key, second edge's key) with t, u and the point.  One lexicographic wave minimum over the three
//     words at the end; the lane that owns it hands its values over and lane 0 writes the record with vector stores.  A minimum
//     of a total order over unique keys: neither the order of the near list nor the split over the lanes can show.
//
// LDS: kCrossLdsBytes = 4 waves x 512 entries x 24 bytes = 48 KB a workgroup.  No LDS atomics, no workgroup barrier (the four
// waves own different queries with different trip counts), nothing passed between waves: a wave's own LDS traffic is ordered by
// WaveSync() alone.  No scratch, no global atomics.
#pragma once

#include "pm_snap.h"

namespace pm {

// One launch of pm_cross_kernel
struct CrossParams {
    SceneView V;
    const float *xyr;            // [3 n] {x, y, r}
    const uint32_t *skip_items;  // [n_items] a non-zero word takes the item out of the search (nullptr: none)
    uint8_t *out;                // [48 n] pm_snap_cross_result
    uint32_t n;
};

namespace {

constexpr uint32_t kCrossMaxNear = 512u;           // PM_SNAP_MAX_NEAR_EDGES
constexpr uint32_t kSnapKindIntersection = 3u;     // PM_SNAP_KIND_INTERSECTION
constexpr uint32_t kSnapKindTooMany = 4u;          // PM_SNAP_KIND_TOO_MANY

// A wave's near edges: entry e is {a, b} in ab[e] and {item, index} in id[e]
struct CrossList {
    float4 ab[kCrossMaxNear];
    uint2 id[kCrossMaxNear];
};
constexpr uint32_t kCrossLdsBytes = kHitWaves * sizeof(CrossList);
static_assert(sizeof(CrossList) == kCrossMaxNear * 24u && kCrossLdsBytes == 49152u, "24 bytes an entry: 48 KB a workgroup, three workgroups in a CU's 160 KB");

// A lane's best pair.  d2 = all ones: none yet (no qualifying d2 has that pattern: it is <= r * r, finite)
struct CrossBest {
    uint64_t d2 = ~0ull;
    uint64_t key1 = ~0ull, key2 = ~0ull;   // SnapKey of the first and of the second edge
    float t = 0.0f, u = 0.0f, x = 0.0f, y = 0.0f;
};

// D23, near: D21's edge d2 <= r * r, by SnapEdge itself
__device__ __forceinline__ bool CrossNear(const SnapQ &Q, float2 a, float2 b) {
    SnapBest s;
    SnapEdge(s, Q, a, b, 0u, 0u);
    return s.d2 != ~0ull;
}

// Wave-uniform: the lanes with `on` append their edge behind the n_near counted so far; beyond kCrossMaxNear only the count goes on
__device__ __forceinline__ void CrossAppend(CrossList &L, uint32_t &n_near, bool on, float4 ab, uint32_t item, uint32_t index) {
    const uint64_t m = __ballot(on);
    const uint32_t at = n_near + RankBelow(m);
    if (on && at < kCrossMaxNear) {
        L.ab[at] = ab;
        L.id[at] = make_uint2(item, index);
    }
    n_near += static_cast<uint32_t>(__popcll(m));
}

// Fill item `item` (wave-uniform arguments): a lane notes which of its chunk's segments are near, the round's end stores them
__device__ __forceinline__ void CrossFill(const SceneView &V, uint32_t item, const uint8_t *it, const SnapQ &Q, uint32_t lane, CrossList &L, uint32_t &n_near) {
    const uint32_t flags = LoadU32(it + 4), npt = LoadU32(it + 12);
    const uint8_t *pts = V.scene + LoadU32(it + 16);
    const bool compound = (flags & kFillCompound) != 0;
    const uint32_t cb0 = V.chunk_base[item], cb1 = V.chunk_base[item + 1];
    uint32_t noted = 0u, k0_noted = 0u;   // bit s: segment k0_noted + s is near, and seg[s] holds its ends
    float4 seg[kChunkSegs] = {};
    ForItemChunks(
        V, cb0, cb1, lane, [&](float4 bb) { return SnapPass(Q, bb); },
        [&](uint32_t c) {
            const uint32_t k0 = (c - cb0) * kChunkSegs, k1 = min(k0 + kChunkSegs, FillSegs(npt));
            k0_noted = k0;
#pragma unroll
            for (uint32_t s = 0; s < kChunkSegs; ++s) {
                float2 a, b;
                if (k0 + s < k1 && FillSegmentEnds(pts, npt, compound, k0 + s, a, b) && CrossNear(Q, a, b)) {   // (a separator: no segment)
                    noted |= 1u << s;
                    seg[s] = make_float4(a.x, a.y, b.x, b.y);
                }
            }
        },
        [&] {
            if (__ballot(noted != 0u) != 0ull) {
#pragma unroll
                for (uint32_t s = 0; s < kChunkSegs; ++s) CrossAppend(L, n_near, ((noted >> s) & 1u) != 0u, seg[s], item, k0_noted + s);
                noted = 0u;
            }
            return false;
        });
}

// Polyline item `item` of two points or more (one-point Polylines are evaluated on their item's lane)
__device__ __forceinline__ void CrossPoly(const SceneView &V, uint32_t item, const uint8_t *it, const SnapQ &Q, uint32_t lane, CrossList &L, uint32_t &n_near) {
    const uint32_t npt = LoadU32(it + 12);
    const uint8_t *pts = V.scene + LoadU32(it + 16);
    const uint32_t cb0 = V.chunk_base[item], cb1 = V.chunk_base[item + 1];
    uint32_t noted = 0u, k0_noted = 0u;
    float4 seg[kChunkSegs] = {};
    ForItemChunks(
        V, cb0, cb1, lane, [&](float4 bb) { return SnapPass(Q, bb); },
        [&](uint32_t c) {
            const uint32_t k0 = (c - cb0) * kChunkSegs, k1 = min(k0 + kChunkSegs, PolySegs(npt));
            k0_noted = k0;
            float2 a = LoadF2(pts + static_cast<size_t>(k0) * 8);
#pragma unroll
            for (uint32_t s = 0; s < kChunkSegs; ++s) {
                if (k0 + s < k1) {
                    const float2 b = LoadF2(pts + static_cast<size_t>(k0 + s + 1u) * 8);
                    if (CrossNear(Q, a, b)) {
                        noted |= 1u << s;
                        seg[s] = make_float4(a.x, a.y, b.x, b.y);
                    }
                    a = b;
                }
            }
        },
        [&] {
            if (__ballot(noted != 0u) != 0ull) {
#pragma unroll
                for (uint32_t s = 0; s < kChunkSegs; ++s) CrossAppend(L, n_near, ((noted >> s) & 1u) != 0u, seg[s], item, k0_noted + s);
                noted = 0u;
            }
            return false;
        });
}

// D23, one pair of distinct near edges: oriented by "precedes", dropped if the edges share an end, then the crossing
__device__ __forceinline__ void CrossPair(CrossBest &best, const SnapQ &Q, float4 e, uint2 eid, float4 f, uint2 fid) {
    uint64_t k1 = SnapKey(eid.x, eid.y), k2 = SnapKey(fid.x, fid.y);
    if (k2 < k1) {   // f precedes: the larger item, then the smaller index
        const float4 g = e;
        e = f;
        f = g;
        const uint64_t k = k1;
        k1 = k2;
        k2 = k;
    }
    if ((e.x == f.x && e.y == f.y) || (e.x == f.z && e.y == f.w) || (e.z == f.x && e.w == f.y) || (e.z == f.z && e.w == f.w)) return;
    const double ax = e.x, ay = e.y, cx = f.x, cy = f.y;
    const double rx = static_cast<double>(e.z) - ax, ry = static_cast<double>(e.w) - ay;
    const double sx = static_cast<double>(f.z) - cx, sy = static_cast<double>(f.w) - cy;
    const double den = rx * sy - ry * sx;
    if (!(den != 0.0)) return;
    const double wx = cx - ax, wy = cy - ay;
    const double t = (wx * sy - wy * sx) / den;
    if (!(0.0 <= t && t <= 1.0)) return;   // (before u is taken: most pairs of near edges do not cross)
    const double u = (wx * ry - wy * rx) / den;
    if (!(0.0 <= u && u <= 1.0)) return;
    const double X = ax + rx * t, Y = ay + ry * t;
    const double dx = Q.x - X, dy = Q.y - Y;
    const double d2 = dx * dx + dy * dy;
    if (!(d2 <= Q.r2)) return;
    const uint64_t bits = __builtin_bit_cast(uint64_t, d2);
    if (bits < best.d2 || (bits == best.d2 && (k1 < best.key1 || (k1 == best.key1 && k2 < best.key2)))) {
        best.d2 = bits;
        best.key1 = k1;
        best.key2 = k2;
        best.t = static_cast<float>(t);
        best.u = static_cast<float>(u);
        best.x = static_cast<float>(X);
        best.y = static_cast<float>(Y);
    }
}

// The wave's minimum of (d2, key1, key2), in every lane: SnapWaveMin by a word more
__device__ __forceinline__ void CrossWaveMin(uint64_t &d2, uint64_t &key1, uint64_t &key2) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint64_t od = __shfl_xor(static_cast<unsigned long long>(d2), d, 64), o1 = __shfl_xor(static_cast<unsigned long long>(key1), d, 64),
                       o2 = __shfl_xor(static_cast<unsigned long long>(key2), d, 64);
        if (od < d2 || (od == d2 && (o1 < key1 || (o1 == key1 && o2 < key2)))) {
            d2 = od;
            key1 = o1;
            key2 = o2;
        }
    }
}

}  // namespace

__global__ __launch_bounds__(kHitThreads) void pm_cross_kernel(CrossParams S) {
    __shared__ CrossList s_list[kHitWaves];   // a slice per wave: no wave reads or writes another's
    const SceneView &V = S.V;
    const uint32_t lane = LaneId();
    const bool skip = (V.flags & kHitSkipTransparent) != 0;
    CrossList &L = s_list[WaveId()];
    const uint32_t n_waves = GridWaves();
    for (uint32_t q = FirstWaveUnit(); q < S.n; q += n_waves) {
        SnapQ Q;
        const bool valid = SnapLoad(S.xyr + static_cast<size_t>(q) * 3, Q);
        Q.vertices = false;
        Q.edges = true;
        // ---- phase 1: the near list
        uint32_t n_near = 0u;   // (wave-uniform)
        for (uint32_t hi = V.n_items; hi != 0u && valid; hi = hi > 64u ? hi - 64u : 0u) {
            // lane 0 looks at the topmost item of the step
            bool cand = false, one = false;   // one: this lane's item is a single near edge, a and b
            float2 a = make_float2(0.0f, 0.0f), b = a;
            if (lane < hi) {
                const ItemHead h = LoadItemHead(V, hi - 1u - lane);
                const bool taken_out = S.skip_items != nullptr && S.skip_items[h.item] != 0u;
                if (taken_out) {
                } else if (h.tag == kItemLine) {
                    if (!(skip && ItemTransparent(h))) {
                        a = LoadF2(h.it + 16);
                        b = LoadF2(h.it + 24);
                        one = CrossNear(Q, a, b);
                    }
                } else if (h.tag == kItemFill) {
                    cand = SnapCandidate(Q, h) && !(skip && ItemTransparent(h));
                } else if (h.tag == kItemPoly) {
                    const uint32_t npt = LoadU32(h.it + 12);
                    const bool shown = !(skip && ItemTransparent(h));
                    if (npt == 1u) {   // one degenerate segment (the scene index has no chunk for it)
                        if (shown) {
                            a = b = LoadF2(V.scene + LoadU32(h.it + 16));
                            one = CrossNear(Q, a, b);
                        }
                    } else if (npt != 0u) {
                        // (its box was made from the points and the width: of a width that is NaN or negative it bounds nothing)
                        const bool boxed = __uint_as_float(LoadU32(h.it + 8)) >= 0.0f;
                        cand = (!boxed || SnapCandidate(Q, h)) && shown;
                    }
                }
            }
            CrossAppend(L, n_near, one, make_float4(a.x, a.y, b.x, b.y), hi - 1u - lane, 0u);
            uint64_t m = __ballot(cand);
            while (m != 0ull) {   // every candidate is finished: a near edge may be in any of them
                const ItemHead h = LoadItemHead(V, hi - 1u - TakeLowestLane(m));
                if (h.tag == kItemFill) CrossFill(V, h.item, h.it, Q, lane, L, n_near);
                else CrossPoly(V, h.item, h.it, Q, lane, L, n_near);
            }
        }
        WaveSync();   // the list is written: the wave reads it
        // ---- phase 2: the pairs
        CrossBest best;
        if (n_near <= kCrossMaxNear) {
#pragma unroll 1
            for (uint32_t i = 0; i + 1u < n_near; ++i) {
                const float4 e = L.ab[i];
                const uint2 eid = L.id[i];
#pragma unroll 1
                for (uint32_t j = i + 1u + lane; j < n_near; j += 64u) CrossPair(best, Q, e, eid, L.ab[j], L.id[j]);
            }
        }
        uint64_t d2 = best.d2, key1 = best.key1, key2 = best.key2;
        CrossWaveMin(d2, key1, key2);
        const bool mine = best.d2 == d2 && best.key1 == key1 && best.key2 == key2;
        uint32_t w[12] = {kHitNone, n_near > kCrossMaxNear ? kSnapKindTooMany : 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, n_near};
        if (d2 != ~0ull) {   // (a pair's keys are unique: one lane owns the winner)
            const int l = __builtin_amdgcn_readfirstlane(__builtin_ctzll(__ballot(mine)));
            w[0] = ~static_cast<uint32_t>(key1 >> 32);
            w[1] = kSnapKindIntersection;
            w[2] = static_cast<uint32_t>(key1);
            w[3] = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(__float_as_uint(best.t)), l));
            w[4] = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(__float_as_uint(best.x)), l));
            w[5] = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(__float_as_uint(best.y)), l));
            w[6] = static_cast<uint32_t>(d2);
            w[7] = static_cast<uint32_t>(d2 >> 32);
            w[8] = ~static_cast<uint32_t>(key2 >> 32);
            w[9] = static_cast<uint32_t>(key2);
            w[10] = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(__float_as_uint(best.u)), l));
        }
        if (lane == 0u) {
            uint2 *rec = reinterpret_cast<uint2 *>(S.out + static_cast<size_t>(q) * 48);   // (8-byte aligned, as the record's double is)
#pragma unroll
            for (int k = 0; k < 6; ++k) rec[k] = make_uint2(w[2 * k], w[2 * k + 1]);
        }
        WaveSync();   // the list is read: the next query's may overwrite it
    }
}

// grid: LaunchSnap's rule (the workgroups beyond the three a CU's LDS holds at once wait their turn)
void LaunchCross(const CrossParams &p, uint32_t n_cus, hipStream_t stream) { LaunchQuery(pm_cross_kernel, p, p.n, n_cus, stream); }

}  // namespace pm
