// pm_trim_kernel: trimming -- the piece of an item between two lengths, as poly-line runs of vertices in the order of the walk.
// Not on the frame path: like the measure kernels it reads the scene, nothing a frame writes.  Included by pm_context.hip after
// pm_resample.h, whose float shuffle it uses; the walk, the fix, the scan, the point and the lane helpers are pm_measure.h's as they
// are: that a cut vertex is byte for byte what pm_points_at_length_kernel answers at the same position follows from shared code, not
// from a restatement.
//
// What a request is, which segments a piece covers and which vertices it has is decision D27; tests/np_trim.py states
// the same from the decision's text in Python integers over np_measure's segment lists.
//
// A wave per request, in pm_query_common.h's persistent launch shape.  It is the first query kernel whose answer has a VARIABLE
// number of records in a fixed order:
//
//  * part mode first sums T as pm_resample_kernel's even mode does, then one division and one remainder give [b_j, b_j+1];
//  * ONE walk, 64 entries per step: q, the inclusive scan with the carry, Q0 = Q1 - q, and the covered predicate Q0 < hi && Q1 > lo.
//    A step no lane of which is covered costs the scan, one ballot and one uniform branch;
//  * a covered lane's A is a's stored pair, or the point at lo where the piece starts inside the segment; its B is b's stored pair, or
//    the point at hi.  At most one lane of a request cuts at lo and one at hi: the two MeasurePoint calls sit on divergent lanes;
//  * the previous covered segment's B comes by a shuffle from the highest covered lane below; for a step's lowest covered lane it is
//    the pair the step before left in scalar registers.  A differs from it (as f32 values), or there is none: A is emitted, with MOVE;
//  * vertex number p of a lane's first vertex is the running total plus two ballot population counts below the lane, of the covered
//    lanes (each emits a B) and of the MOVE lanes (each emits an A too).  Vertex p goes to out[first + p] iff p < cap and
//    first + p < out_cap; lane 0 writes the info after the walk.
//
// Range mode does not know T before the walk ends and needs it in ONE place only: hi = min(s1, T) leaves a segment of no length at
// Q0 == T out of the piece, s1 > T alone would take it in.  Such a lane shows as a covered lane of no length at the step's very end;
// the first step that has one sums the rest of the walk (the strided sum again, once a request at the most) and hi is exact from
// there on.  Everywhere else min(s0, T) and min(s1, T) decide as s0 and s1 do, because no Q exceeds T.
// No atomics, no LDS, no scratch.
#pragma once

#include "pm_resample.h"

namespace pm {

struct TrimParams {
    SceneView V;            // flags: PM_HIT_SKIP_TRANSPARENT
    const uint8_t *q;       // [32 n] pm_trim_query
    uint8_t *out;           // [16 out_cap] pm_trim_vertex
    uint8_t *info;          // [24 n] pm_trim_info
    unsigned long long out_cap;
    uint32_t n;
};

namespace {

constexpr uint32_t kTrimRange = 0u;                 // PM_TRIM_RANGE
constexpr uint32_t kTrimPart = 1u;                  // PM_TRIM_PART
constexpr uint32_t kTrimMaxParts = 1u << 20;        // PM_TRIM_MAX_PARTS
constexpr uint32_t kTrimInvalid = 0xffffffffu;      // PM_TRIM_INVALID
constexpr uint32_t kTrimMove = 1u;                  // PM_TRIM_MOVE
constexpr uint32_t kTrimCut = 2u;                   // PM_TRIM_CUT
constexpr uint32_t kTrimTruncated = 1u;             // PM_TRIM_TRUNCATED
constexpr uint32_t kTrimEndClamped = 2u;            // PM_TRIM_END_CLAMPED

// A 16-byte pm_trim_vertex, by ONE lane (8-byte aligned)
__device__ __forceinline__ void TrimStoreVertex(uint8_t *at, float x, float y, uint32_t index, uint32_t flags) {
    uint2 *rec = reinterpret_cast<uint2 *>(at);
    rec[0] = make_uint2(__float_as_uint(x), __float_as_uint(y));
    rec[1] = make_uint2(index, flags);
}

// A 24-byte pm_trim_info (8-byte aligned)
__device__ __forceinline__ void TrimStoreInfo(uint8_t *at, unsigned long long length, uint32_t n_vertices, uint32_t n_runs, uint32_t kind, uint32_t flags) {
    uint2 *rec = reinterpret_cast<uint2 *>(at);
    rec[0] = make_uint2(static_cast<uint32_t>(length), static_cast<uint32_t>(length >> 32));
    rec[1] = make_uint2(n_vertices, n_runs);
    rec[2] = make_uint2(kind, flags);
}

}  // namespace

__global__ __launch_bounds__(kHitThreads) void pm_trim_kernel(TrimParams M) {
    const SceneView &V = M.V;
    const uint32_t lane = LaneId();
    const uint32_t n_waves = GridWaves();
    for (uint32_t qi = FirstWaveUnit(); qi < M.n; qi += n_waves) {
        // {u32 item; u32 mode; u32 first; u32 cap; u64 s0; u64 s1}, every lane alike: into scalar registers
        const uint2 *in = reinterpret_cast<const uint2 *>(M.q + static_cast<size_t>(qi) * 32);   // (8-byte aligned)
        const uint2 in0 = in[0], in1 = in[1], in2 = in[2], in3 = in[3];
        const uint32_t item = UniformF32Bits(in0.x), mode = UniformF32Bits(in0.y), first = UniformF32Bits(in1.x), cap = UniformF32Bits(in1.y);
        const unsigned long long s0 = (static_cast<unsigned long long>(UniformF32Bits(in2.y)) << 32) | UniformF32Bits(in2.x);
        const unsigned long long s1 = (static_cast<unsigned long long>(UniformF32Bits(in3.y)) << 32) | UniformF32Bits(in3.x);
        uint8_t *info = M.info + static_cast<size_t>(qi) * 24;
        const bool part = mode == kTrimPart;
        if (mode > kTrimPart || (part ? (s1 == 0ull || s1 > kTrimMaxParts || s0 >= s1) : s0 > s1)) {   // (uniform)
            if (lane == 0u) TrimStoreInfo(info, 0ull, 0u, 0u, kTrimInvalid, 0u);
            continue;
        }
        const MeasureWalk W = MeasureWalkOf(V, item);
        unsigned long long lo = s0, hi = s1;   // range mode: min(., T) decides nothing but what exact_hi below says
        bool exact_hi = part;                  // is hi min(s1, T) already
        if (part) {   // T first: pm_item_lengths_kernel's strided sum
            unsigned long long T = 0ull;
            for (uint32_t k = lane; k < W.n_idx; k += 64u) {
                bool seg;
                T += MeasureQ(W, k, seg);
            }
            T = MeasureWaveSum(T);
            T = MeasureLane64(T, 0u);
            const unsigned long long d = T / s1, r = T % s1;   // b_i = i d + min(i, r): b_j+1 - b_j is d, and one more below r
            lo = s0 * d + (s0 < r ? s0 : r);
            hi = lo + d + (s0 < r ? 1ull : 0ull);
        }
        if (lo >= hi) lo = hi = 0ull;   // the empty piece: no Q0 is below 0
        // vertex p of the piece goes to out[first + p] for p < room
        const unsigned long long left = M.out_cap > first ? M.out_cap - first : 0ull;
        const uint32_t room = left < cap ? static_cast<uint32_t>(left) : cap;
        uint32_t n_vertices = 0u, n_runs = 0u;
        unsigned long long carry = 0ull;     // Q of the step's first entry
        bool have_prev = false;              // has a segment been covered in a step before, and its B
        uint32_t pbx = 0u, pby = 0u;
        for (uint32_t base = 0; base < W.n_idx; base += 64u) {
            const uint32_t k = base + lane;
            float2 a = make_float2(0.0f, 0.0f), b = a;
            const bool seg = k < W.n_idx && MeasureEnds(W, k, a, b);
            const unsigned long long q = seg ? MeasureFix(a, b) : 0ull;
            const unsigned long long q1 = carry + MeasureScan(q, lane), q0 = q1 - q;
            const unsigned long long end = MeasureLane64(q1, 63u);
            bool covered = seg && q0 < hi && q1 > lo;
            uint64_t cm = __ballot(covered);
            if (cm == 0ull) {   // (uniform) a step wholly outside the piece
                carry = end;
                continue;
            }
            if (!exact_hi && __ballot(covered && q == 0ull && q0 == end) != 0ull) {   // (uniform) is that lane at T itself: the rest of the walk says
                unsigned long long rest = 0ull;
                for (uint32_t j = base + 64u + lane; j < W.n_idx; j += 64u) {
                    bool sg;
                    rest += MeasureQ(W, j, sg);
                }
                rest = MeasureWaveSum(rest);
                const unsigned long long T = end + MeasureLane64(rest, 0u);
                if (T < hi) hi = T;
                exact_hi = true;
                covered = covered && q0 < hi;
                cm = __ballot(covered);
                if (cm == 0ull) {
                    carry = end;
                    continue;
                }
            }
            // the lane's two vertices: stored values, or the point at lo / at hi inside the segment (divergent: a lane of each per request)
            float Ax = a.x, Ay = a.y, Bx = b.x, By = b.y;
            uint32_t fa = 0u, fb = 0u;
            if (covered && q0 < lo) {
                float t;
                MeasurePoint(a, b, q0, q, lo, t, Ax, Ay);
                fa = kTrimCut;
            }
            if (covered && hi < q1) {
                float t;
                MeasurePoint(a, b, q0, q, hi, t, Bx, By);
                fb = kTrimCut;
            }
            // the B of the covered segment before: the highest covered lane below, or what the steps before left
            const uint64_t below = cm & ((1ull << lane) - 1ull);
            const uint32_t src = below != 0ull ? 63u - static_cast<uint32_t>(__builtin_clzll(below)) : lane;
            float Px = ResampleShflF(Bx, src), Py = ResampleShflF(By, src);
            bool has = below != 0ull;
            if (!has && have_prev) {
                Px = __uint_as_float(pbx);
                Py = __uint_as_float(pby);
                has = true;
            }
            const bool move = covered && !(has && Ax == Px && Ay == Py);   // (f32 values: -0 equals 0, a NaN nothing)
            const uint64_t mm = __ballot(move);
            if (covered) {
                uint32_t p = n_vertices + RankBelow(cm) + RankBelow(mm);
                if (move) {
                    if (p < room) TrimStoreVertex(M.out + (static_cast<size_t>(first) + p) * 16, Ax, Ay, k, kTrimMove | fa);
                    ++p;
                }
                if (p < room) TrimStoreVertex(M.out + (static_cast<size_t>(first) + p) * 16, Bx, By, k, fb);
            }
            n_vertices += static_cast<uint32_t>(__popcll(cm)) + static_cast<uint32_t>(__popcll(mm));
            n_runs += static_cast<uint32_t>(__popcll(mm));
            const uint32_t top = 63u - static_cast<uint32_t>(__builtin_clzll(cm));
            pbx = MeasureLane32(__float_as_uint(Bx), top);
            pby = MeasureLane32(__float_as_uint(By), top);
            have_prev = true;
            carry = end;
        }
        // the walk is over: carry is T
        if (lane == 0u)
            TrimStoreInfo(info, carry, n_vertices, n_runs, W.kind, (n_vertices > room ? kTrimTruncated : 0u) | (!part && s1 > carry ? kTrimEndClamped : 0u));
    }
}

void LaunchTrim(const TrimParams &p, uint32_t n_cus, hipStream_t stream) { LaunchQuery(pm_trim_kernel, p, p.n, n_cus, stream); }

}  // namespace pm
