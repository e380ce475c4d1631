// pm_crossings_kernel: item crossings -- every point where an edge of item A crosses an edge of item B, or where an item crosses
// itself, as 48-byte records in the order (i, j) of the two edges' names.  Not on the frame path: like the other query kernels it
// reads the scene and the scene index, nothing a frame writes.  Included by pm_context.hip after pm_trim.h; the walk and the edge
// names are pm_measure.h's (MeasureWalkOf, MeasureEnds), the chunk walk is pm_query_common.h's (ForItemChunks), the union of boxes is
// pm_bounds.h's (BoundsAcc, BoundsAddChunk, BoundsWaveUnion), all as they are.
//
// What an edge is, which pairs are crossings, what a record holds and in which order the records come is decision D29:
// binary64 arithmetic on the scene's f32 values, one rounding per written operation, in the written order (-ffp-contract=off) --
// tests/np_crossings.py states the same from the decision's text and records, untouched rows and infos must agree byte for byte.
//
// One WAVE owns a request, in pm_query_common.h's persistent launch shape.
//  * K(A) * K(B) > 2^28 answers "too many" before any edge is looked at: a request's work is bounded by a count of index ranges.
//  * B's box: the union of B's chunk boxes (a Line: the box of its two points), once per request.
//  * A's edges i in increasing order under scalar control.  A's chunks are tested against B's box 64 at a time, one ballot, and the
//    survivors are taken lowest first; edge i's four floats are moved into scalar registers.
//  * For each i, B's chunks are spread over the lanes by ForItemChunks with pass = the chunk's box overlaps edge i's box (closed
//    comparisons, D29's box rule itself: a chunk box holds the boxes of its edges, so a culled chunk holds no crossing, and the rule
//    keeps the cull out of the bytes).  A lane tests its chunk's up to kChunkSegs segments and keeps t, u, x, y and the side.
//  * The wave-uniform done callback ranks what the lanes noted lane-major -- ForItemChunks hands chunks out in increasing order
//    over the lanes, so that is increasing j -- from kChunkSegs ballots: the population counts below the lane, plus the lane's own
//    lower bits.  Record p goes to out[first + p] iff p < cap and first + p < out_cap, behind a scalar running count.
//  * Lane 0 writes the info after the walk.
// Vector stores only; no atomics, no LDS, no scratch, nothing passed between waves.
#pragma once

#include "pm_bounds.h"
#include "pm_trim.h"

namespace pm {

struct CrossingsParams {
    SceneView V;            // flags: PM_HIT_SKIP_TRANSPARENT
    const uint8_t *q;       // [16 n] pm_crossings_query
    uint8_t *out;           // [48 out_cap] pm_crossing
    uint8_t *info;          // [16 n] pm_crossings_info
    unsigned long long out_cap;
    uint32_t n;
};

namespace {

constexpr uint32_t kCrossingsTruncated = 1u;                    // PM_CROSSINGS_TRUNCATED
constexpr uint32_t kCrossingsTooMany = 2u;                      // PM_CROSSINGS_TOO_MANY
constexpr unsigned long long kCrossingsMaxPairs = 1ull << 28;   // PM_CROSSINGS_MAX_PAIRS

// What a lane found in its chunk: bit s of noted says that segment k0 + s crosses the edge in hand
struct CrossingsNoted {
    uint32_t noted = 0u, k0 = 0u, side = 0u;   // side: bit s set: den < 0
    float t[kChunkSegs] = {}, u[kChunkSegs] = {}, x[kChunkSegs] = {}, y[kChunkSegs] = {};
};

// D29: is the pair e = a -> b (e.xy, e.zw), f = c -> d a crossing, and where.  Both edges have finite ends.
__device__ __forceinline__ bool CrossingsPair(float4 e, float4 f, float &t, float &u, float &x, float &y, bool &neg) {
    // 1. the box rule, on the stored values
    if (!(fmaxf(e.x, e.z) >= fminf(f.x, f.z) && fmaxf(f.x, f.z) >= fminf(e.x, e.z) && fmaxf(e.y, e.w) >= fminf(f.y, f.w) && fmaxf(f.y, f.w) >= fminf(e.y, e.w)))
        return false;
    // 2. no shared end
    if ((e.x == f.x && e.y == f.y) || (e.x == f.z && e.y == f.w) || (e.z == f.x && e.w == f.y) || (e.z == f.z && e.w == f.w)) return false;
    // 3. D23's steps 1 to 5
    const double ax = e.x, ay = e.y, cx = f.x, cy = f.y;
    const double rx = static_cast<double>(e.z) - ax, ry = static_cast<double>(e.w) - ay;
    const double sx = static_cast<double>(f.z) - cx, sy = static_cast<double>(f.w) - cy;
    const double den = rx * sy - ry * sx;
    if (!(den != 0.0)) return false;
    const double wx = cx - ax, wy = cy - ay;
    const double t64 = (wx * sy - wy * sx) / den;
    if (!(0.0 <= t64 && t64 <= 1.0)) return false;   // (before u is taken: most pairs do not cross)
    const double u64 = (wx * ry - wy * rx) / den;
    if (!(0.0 <= u64 && u64 <= 1.0)) return false;
    t = static_cast<float>(t64);
    u = static_cast<float>(u64);
    x = static_cast<float>(ax + rx * t64);
    y = static_cast<float>(ay + ry * t64);
    neg = den < 0.0;
    return true;
}

// A 48-byte pm_crossing, by ONE lane (8-byte aligned)
__device__ __forceinline__ void CrossingsStore(uint8_t *at, uint32_t item_a, uint32_t i, float t, uint32_t item_b, uint32_t j, float u, float x, float y, uint32_t side) {
    uint2 *rec = reinterpret_cast<uint2 *>(at);
    rec[0] = make_uint2(item_a, i);
    rec[1] = make_uint2(__float_as_uint(t), 0u);
    rec[2] = make_uint2(item_b, j);
    rec[3] = make_uint2(__float_as_uint(u), 0u);
    rec[4] = make_uint2(__float_as_uint(x), __float_as_uint(y));
    rec[5] = make_uint2(side, 0u);
}

// A 16-byte pm_crossings_info (8-byte aligned)
__device__ __forceinline__ void CrossingsStoreInfo(uint8_t *at, uint32_t n_crossings, uint32_t flags, uint32_t n_a, uint32_t n_b) {
    uint2 *rec = reinterpret_cast<uint2 *>(at);
    rec[0] = make_uint2(n_crossings, flags);
    rec[1] = make_uint2(n_a, n_b);
}

// Do two closed boxes {x0, y0, x1, y1} meet (an empty box, or one of a NaN, meets nothing)
__device__ __forceinline__ bool CrossingsBoxesMeet(float4 p, float4 q) { return p.z >= q.x && q.z >= p.x && p.w >= q.y && q.w >= p.y; }

}  // namespace

__global__ __launch_bounds__(kHitThreads) void pm_crossings_kernel(CrossingsParams M) {
    const SceneView &V = M.V;
    const uint32_t lane = LaneId();
    const uint32_t n_waves = GridWaves();
    for (uint32_t qi = FirstWaveUnit(); qi < M.n; qi += n_waves) {
        // {u32 item_a; u32 item_b; u32 first; u32 cap}, every lane alike: into scalar registers
        const uint2 *in = reinterpret_cast<const uint2 *>(M.q + static_cast<size_t>(qi) * 16);   // (8-byte aligned)
        const uint2 in0 = in[0], in1 = in[1];
        const uint32_t item_a = UniformF32Bits(in0.x), item_b = UniformF32Bits(in0.y), first = UniformF32Bits(in1.x), cap = UniformF32Bits(in1.y);
        uint8_t *info = M.info + static_cast<size_t>(qi) * 16;
        const MeasureWalk WA = MeasureWalkOf(V, item_a), WB = MeasureWalkOf(V, item_b);
        const uint32_t n_a = UniformF32Bits(WA.n_idx), n_b = UniformF32Bits(WB.n_idx);
        if (static_cast<unsigned long long>(n_a) * n_b > kCrossingsMaxPairs) {   // (uniform) before any edge is looked at
            if (lane == 0u) CrossingsStoreInfo(info, 0u, kCrossingsTooMany, n_a, n_b);
            continue;
        }
        if (n_a == 0u || n_b == 0u) {   // (uniform) an item without edges
            if (lane == 0u) CrossingsStoreInfo(info, 0u, 0u, n_a, n_b);
            continue;
        }
        const bool self = item_a == item_b;
        // an item of edges has its chunks, ceil(K / kChunkSegs) of them, or is a Line and has none
        const uint32_t ca0 = V.chunk_base[item_a], ca1 = V.chunk_base[item_a + 1u];
        const uint32_t cb0 = V.chunk_base[item_b], cb1 = V.chunk_base[item_b + 1u];
        // record p goes to out[first + p] for p < room
        const unsigned long long left = M.out_cap > first ? M.out_cap - first : 0ull;
        const uint32_t room = left < cap ? static_cast<uint32_t>(left) : cap;
        // B's box: a superset of the box of every edge of B
        float4 bbox;
        {
            BoundsAcc acc;
            if (cb1 != cb0) {
                for (uint32_t c = cb0 + lane; c < cb1; c += 64u) BoundsAddChunk(acc, V.chunk_bbox[c]);
            } else {
                BoundsAddPoint(acc, LoadF2(WB.pts));
                BoundsAddPoint(acc, LoadF2(WB.pts + 8));
            }
            BoundsWaveUnion(acc);
            bbox = make_float4(__uint_as_float(UniformF32Bits(__float_as_uint(acc.x0))), __uint_as_float(UniformF32Bits(__float_as_uint(acc.y0))),
                               __uint_as_float(UniformF32Bits(__float_as_uint(acc.x1))), __uint_as_float(UniformF32Bits(__float_as_uint(acc.y1))));
        }
        uint32_t n_crossings = 0u;   // (wave-uniform)
        // edge i of A against every edge of B (self: every later edge)
        auto edge = [&](uint32_t i) {
            float2 a, b;
            const bool is_edge = MeasureEnds(WA, i, a, b) && RectFinite(a) && RectFinite(b);
            if (__ballot(is_edge) == 0ull) return;   // (uniform: every lane loaded the same entry)
            const float4 e = make_float4(__uint_as_float(UniformF32Bits(__float_as_uint(a.x))), __uint_as_float(UniformF32Bits(__float_as_uint(a.y))),
                                         __uint_as_float(UniformF32Bits(__float_as_uint(b.x))), __uint_as_float(UniformF32Bits(__float_as_uint(b.y))));
            const float4 ebox = make_float4(fminf(e.x, e.z), fminf(e.y, e.w), fmaxf(e.x, e.z), fmaxf(e.y, e.w));
            CrossingsNoted N;
            // a lane's chunk: segments k0 .. k0 + kChunkSegs - 1 of B
            //  (ONE copy of the pair arithmetic, not kChunkSegs interleaved ones: unrolled, the kernel took 130 VGPRs)
            auto chunk = [&](uint32_t k0) {
                N.k0 = k0;
#pragma unroll 1
                for (uint32_t s = 0; s < kChunkSegs; ++s) {
                    const uint32_t j = k0 + s;
                    float2 c, d;
                    float t, u, x, y;
                    bool neg = false;
                    if (j < n_b && (!self || j > i) && MeasureEnds(WB, j, c, d) && RectFinite(c) && RectFinite(d) &&
                        CrossingsPair(e, make_float4(c.x, c.y, d.x, d.y), t, u, x, y, neg)) {
                        N.noted |= 1u << s;
                        N.side |= (neg ? 1u : 0u) << s;
#pragma unroll
                        for (uint32_t k = 0; k < kChunkSegs; ++k) {   // (selects: a slot indexed by a register would live in scratch)
                            N.t[k] = s == k ? t : N.t[k];
                            N.u[k] = s == k ? u : N.u[k];
                            N.x[k] = s == k ? x : N.x[k];
                            N.y[k] = s == k ? y : N.y[k];
                        }
                    }
                }
            };
            // (uniform) the records of a round, lane-major
            auto emit = [&] {
                if (__ballot(N.noted != 0u) != 0ull) {
                    uint32_t below = 0u, total = 0u;
#pragma unroll
                    for (uint32_t s = 0; s < kChunkSegs; ++s) {
                        const uint64_t m = __ballot(((N.noted >> s) & 1u) != 0u);
                        below += RankBelow(m);
                        total += static_cast<uint32_t>(__popcll(m));
                    }
                    uint32_t p = n_crossings + below;
#pragma unroll
                    for (uint32_t s = 0; s < kChunkSegs; ++s) {
                        if (((N.noted >> s) & 1u) != 0u) {
                            if (p < room)
                                CrossingsStore(M.out + (static_cast<size_t>(first) + p) * 48, item_a, i, N.t[s], item_b, N.k0 + s, N.u[s], N.x[s], N.y[s],
                                               ((N.side >> s) & 1u) != 0u ? 2u : 1u);
                            ++p;
                        }
                    }
                    n_crossings += total;
                    N.noted = 0u;
                    N.side = 0u;
                }
                return false;
            };
            if (cb1 == cb0) {   // B is a Line: its one edge, on lane 0
                if (lane == 0u) chunk(0u);
                (void)emit();
            } else {
                ForItemChunks(
                    V, cb0, cb1, lane, [&](float4 bb) { return CrossingsBoxesMeet(bb, ebox); }, [&](uint32_t c) { chunk((c - cb0) * kChunkSegs); }, emit);
            }
        };
        if (ca1 == ca0) {   // A is a Line
            edge(0u);
        } else {
            for (uint32_t base = ca0; base < ca1; base += 64u) {
                const uint32_t c = base + lane;
                uint64_t m = __ballot(c < ca1 && CrossingsBoxesMeet(V.chunk_bbox[c < ca1 ? c : ca0], bbox));
                while (m != 0ull) {
                    const uint32_t k0 = (base + TakeLowestLane(m) - ca0) * kChunkSegs;
#pragma unroll 1
                    for (uint32_t s = 0; s < kChunkSegs; ++s)
                        if (k0 + s < n_a) edge(k0 + s);
                }
            }
        }
        if (lane == 0u) CrossingsStoreInfo(info, n_crossings, n_crossings > room ? kCrossingsTruncated : 0u, n_a, n_b);
    }
}

void LaunchCrossings(const CrossingsParams &p, uint32_t n_cus, hipStream_t stream) { LaunchQuery(pm_crossings_kernel, p, p.n, n_cus, stream); }

}  // namespace pm
