// Dashed strokes: a styled stroke with a dash pattern stays ONE compound non-zero Fill item per sub-path; its entries are the D14
// outlines (pm_stroke_outline.h) of its dashes, one after another.  Included by pm_flatten.hip behind pm_stroke_outline.h, inside
// namespace pm { namespace {; it reuses that header's OutlineJob, OutlineSink, EmitCorner, EmitJoin, RimDir and WaveBox.
//
// ---- decision D15 (tests/np_dash.py is the independent numpy statement) ---------------------------------------
// The walk W = P (+ P[0] if closed), N points, segment k from W[k] to W[k + 1].  Lengths are INTEGERS in units of 2^-16 px -- the
// reproducible sum: integer addition is associative, so any scan order gives the same positions.
//   q_k = 0 if len_k is NaN, else min(floor(len_k * 65536 + 0.5), 2^32), len_k = sqrt(d.x*d.x + d.y*d.y) in binary64
//   Q[0] = 0, Q[k + 1] = Q[k] + q_k, T = Q[N - 1]
//   g_j = min(floor(f64(v_j * width_scale) * 65536 + 0.5), 2^32); an odd count repeats the pattern once (c' = 2c); G = sum g_j,
//   Pf_j its prefix sums; go = min(floor(|f64(offset * width_scale)| * 65536 + 0.5), 2^62); phase phi = go mod G if the scaled
//   offset is >= 0, else (G - go mod G) mod G
//   G == 0, every gap (odd j) 0, or T == 0: not dashed, the item is exactly the D14 outline.
// On-intervals: for every cycle r >= 0 and even j, A = r*G + Pf_j - phi, B = r*G + Pf_(j+1) - phi, clipped A' = max(A, 0),
// B' = min(B, T); a dash iff A' < B', or A == B with 0 <= A < T (a zero-length dash); in the order of (r, j).
// A dash's poly-line: its start point (s = A': the largest k with Q[k] <= s), every W[i] with A' < Q[i] < B', its end point
// (s = B': the smallest k with Q[k + 1] >= s; a zero-length dash: the start rule twice); a point at s is W[k] / W[k + 1] where s
// meets Q[k] / Q[k + 1], else a + (b - a) * (f64(s - Q[k]) / f64(q_k)) in binary64, rounded once to f32.
// Closed: an on-interval with A <= 0 and B >= T makes the item the D14 closed outline of P; otherwise, if the first dash has
// A <= 0 < B, the last A < T <= B and they are two dashes, the last one's points followed by the first one's are ONE poly-line in
// the first one's place.  Every dash's poly-line is outlined by D14 as an open sub-path; separator indices count from the
// item's entry 0.
//
// How the kernels find their way without storing Q (the host does not know the point count before its one wait, so nothing per
// point is allocated): the on-intervals are numbered m = r*h + j/2 (h = c'/2 per cycle); A_m and B_m grow with m, so the dashes
// are a range [m_lo, m_hi) of m and "how many dashes start / end before position x" is a division by G plus a pass over the
// <= 32 intervals of one cycle (CountAt) -- never a loop over dashes.
#pragma once

constexpr unsigned long long kFixCap = 1ull << 32;        // a segment or a pattern value longer than 65 536 px counts as that
constexpr unsigned long long kDashCountCap = 1ull << 36;  // entries of one sub-path, saturated (such a scene never fits)
constexpr uint32_t kDashWaves = 4;                        // waves (sub-paths) per workgroup

__device__ __forceinline__ void DashWaveSync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ unsigned long long DashFix(double v, unsigned long long cap) {
    if (!(v == v)) return 0ull;
    const double f = floor(v * 65536.0 + 0.5);
    return f >= static_cast<double>(cap) ? cap : static_cast<unsigned long long>(f);
}

__device__ __forceinline__ uint32_t Bcast32(uint32_t v, uint32_t src) { return static_cast<uint32_t>(__shfl(static_cast<int>(v), static_cast<int>(src), 64)); }
__device__ __forceinline__ unsigned long long Bcast64(unsigned long long v, uint32_t src) {
    const uint32_t lo = Bcast32(static_cast<uint32_t>(v), src), hi = Bcast32(static_cast<uint32_t>(v >> 32), src);
    return (static_cast<unsigned long long>(hi) << 32) | lo;
}

// One wave's pattern: the prefix sums Pf_0 .. Pf_c' in LDS (pf[65]: some gap is not 0), the rest uniform.
struct DashPattern {
    const unsigned long long *pf;
    uint32_t h;  // on-intervals per cycle
    unsigned long long G, phi, m_lo;
    bool dashed;
};

__device__ __forceinline__ DashPattern LoadPattern(unsigned long long *pf, const pm_path_dash rec, const float *values, float width_scale, uint32_t lane) {
    DashPattern pat;
    const uint32_t c = rec.count, c2 = (c & 1u) ? 2u * c : c;
    if (lane == 0) {
        unsigned long long acc = 0, gaps = 0;
        pf[0] = 0;
        for (uint32_t j = 0; j < c2; ++j) {
            const float w = values[rec.first + (j >= c ? j - c : j)] * width_scale;
            const unsigned long long g = DashFix(static_cast<double>(w), kFixCap);
            acc += g;
            pf[j + 1u] = acc;
            if ((j & 1u) && g) gaps = 1;
        }
        pf[65] = gaps;
    }
    DashWaveSync();
    pat.pf = pf;
    pat.h = c2 >> 1;
    pat.G = pf[c2];
    pat.dashed = pat.G != 0 && pf[65] != 0;
    const float wo = rec.offset * width_scale;
    const unsigned long long go = DashFix(fabs(static_cast<double>(wo)), 1ull << 62);
    pat.phi = pat.G ? (wo >= 0.0f ? go % pat.G : (pat.G - go % pat.G) % pat.G) : 0ull;
    pat.m_lo = 0;  // the on-intervals that end at or before position 0 without being a dash there (all of cycle 0)
    for (uint32_t jj = 0; jj < pat.h; ++jj) {
        const unsigned long long a = pf[2u * jj], b = pf[2u * jj + 1u];
        if (b < pat.phi || (b == pat.phi && b > a)) ++pat.m_lo;
    }
    return pat;
}

// s = #{m : A_m < x}; e = #{m of a length : B_m <= x} + #{m of no length : A_m < x} (the dashes whose END belongs to a segment
// before position x, m_lo included); inside = x lies strictly inside an on-interval.  x >= 0.
struct DashCount {
    long long s, e;
    bool inside;
};

__device__ __forceinline__ DashCount CountAt(const DashPattern &pat, unsigned long long x) {
    const unsigned long long X = x + pat.phi, Xm = X % pat.G;
    unsigned long long Xd = X / pat.G;
    if (Xd > (1ull << 50)) Xd = 1ull << 50;  // (saturates: a count that large never fits)
    const long long at_G = (Xm == 0 && Xd > 0) ? -1 : 0;  // an interval that starts at Pf == G is the next cycle's at 0
    DashCount c{static_cast<long long>(Xd * pat.h), static_cast<long long>(Xd * pat.h), false};
    for (uint32_t jj = 0; jj < pat.h; ++jj) {
        const unsigned long long a = pat.pf[2u * jj], b = pat.pf[2u * jj + 1u];
        const long long lt = a < pat.G ? (a < Xm ? 1 : 0) : at_G;
        c.s += lt;
        c.e += b > a ? ((b < pat.G && b <= Xm) ? 1 : 0) : lt;
        c.inside = c.inside || (a < Xm && Xm < b);
    }
    return c;
}

struct DashSpan {
    long long A, B;
    bool zero;
};

// on-interval m (dash d is m_lo + d)
__device__ __forceinline__ DashSpan SpanOf(const DashPattern &pat, unsigned long long m) {
    const unsigned long long r = m / pat.h, jj = m % pat.h;
    const unsigned long long a = pat.pf[2u * jj], b = pat.pf[2u * jj + 1u];
    const long long base = static_cast<long long>(r * pat.G) - static_cast<long long>(pat.phi);
    return DashSpan{base + static_cast<long long>(a), base + static_cast<long long>(b), a == b};
}

__device__ __forceinline__ V2 WalkPoint(const uint8_t *scene, const OutlineJob &job, uint32_t i) {
    return LoadPoint(scene, job.pts_ix, i >= job.n ? 0u : i);  // (W[n] of a closed sub-path is P[0])
}

__device__ __forceinline__ unsigned long long SegFix(V2 a, V2 b) {
    const double dx = b.x - a.x, dy = b.y - a.y;
    return DashFix(sqrt(dx * dx + dy * dy), kFixCap);
}

// inclusive scan of the lanes' q (each <= 2^32) in two 32-bit halves
__device__ __forceinline__ unsigned long long WaveScanQ(unsigned long long q, uint32_t lane) {
    uint32_t a = static_cast<uint32_t>(q & 0xffffffull), b = static_cast<uint32_t>(q >> 24);
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t ta = __shfl_up(a, d, 64), tb = __shfl_up(b, d, 64);
        if (lane >= d) {
            a += ta;
            b += tb;
        }
    }
    return static_cast<unsigned long long>(a) + (static_cast<unsigned long long>(b) << 24);
}

__device__ __forceinline__ uint32_t WaveScan32(uint32_t v, uint32_t lane) {
#pragma unroll
    for (uint32_t d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// T: the lanes stride over the segments, the sum is an integer
__device__ __forceinline__ unsigned long long WalkLength(const uint8_t *scene, const OutlineJob &job, uint32_t N, uint32_t lane) {
    unsigned long long t = 0;
    for (uint32_t k = lane; k + 1u < N; k += 64u) t += SegFix(WalkPoint(scene, job, k), WalkPoint(scene, job, k + 1u));
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) t += __shfl_xor(t, d, 64);
    return t;
}

enum DashMode : uint32_t { kDashOutline, kDashCut, kDashMerged };  // the plain D14 outline / dashes / dashes, first and last one

struct DashPlan {
    DashMode mode;
    unsigned long long nd;  // dashes (the merged pair counts twice)
};

__device__ __forceinline__ DashPlan PlanOf(const DashPattern &pat, unsigned long long T, bool closed) {
    DashPlan plan{kDashOutline, 0ull};
    if (!pat.dashed || T == 0) return plan;
    if (closed) {  // the on-interval that covers position 0 is the last one with A <= 0 (all of cycle 0)
        uint32_t cnt = 0;
        for (uint32_t jj = 0; jj < pat.h; ++jj) cnt += pat.pf[2u * jj] <= pat.phi ? 1u : 0u;
        if (cnt != 0 && SpanOf(pat, cnt - 1u).B >= static_cast<long long>(T)) return plan;
    }
    plan.mode = kDashCut;
    const long long m_hi = CountAt(pat, T).s;
    plan.nd = m_hi > static_cast<long long>(pat.m_lo) ? static_cast<unsigned long long>(m_hi) - pat.m_lo : 0ull;
    if (closed && plan.nd >= 2) {
        const DashSpan f = SpanOf(pat, pat.m_lo), l = SpanOf(pat, pat.m_lo + plan.nd - 1ull);
        if (f.A <= 0 && f.B > 0 && l.A < static_cast<long long>(T) && l.B >= static_cast<long long>(T)) plan.mode = kDashMerged;
    }
    return plan;
}

__device__ __forceinline__ pm_path_dash DashOf(const pm_path_dash *dashes, uint32_t ix) { return dashes[ix]; }

// A wave per dashed sub-path: out_cnt[s] = the entries of its item, added to *out_total (before KOutlineScan).
template <bool kGrouped>
__device__ __forceinline__ void DashCountBody(unsigned long long (*s_pf)[66], const pm_path *paths, uint32_t n_paths, const pm_path_el *els,
                                              float width_scale_u, const GroupTable &gt, const uint32_t *el_ptoff, const uint32_t *el_mvoff,
                                              const uint32_t *path_item_base, const uint32_t *path_pt_base, const uint32_t *sub_first_el,
                                              const uint32_t *totals, const unsigned long long *n_pts64, const uint32_t *path_dash,
                                              const pm_path_dash *dashes, const float *dash_values, const uint8_t *scene, uint32_t scene_cap,
                                              uint32_t *out_cnt, unsigned long long *out_total) {
    const uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u, wave = (threadIdx.x >> 6) & (kDashWaves - 1u);
    if (s >= totals[2]) return;  // (whole waves)
    const OutlineJob job = MakeOutlineJob<kGrouped>(paths, n_paths, els, width_scale_u, gt, el_ptoff, el_mvoff, path_item_base, path_pt_base, sub_first_el, totals[0], s);
    if (!job.styled || !IsDashed(path_dash, job.path)) return;  // (uniform)
    const float width_scale = WidthScaleOf<kGrouped>(width_scale_u, gt, job.path);
    const DashPattern pat = LoadPattern(s_pf[wave], DashOf(dashes, path_dash[job.path]), dash_values, width_scale, lane);
    const OutlineLayout lay = LayoutOf(job);
    unsigned long long total = lay.total;
    // (the points are there only if the scene without outlines fits, *n_pts64 as it stands before KOutlineScan: KPoints wrote
    //  none otherwise, and the need reported then counts the undashed outline -- the call that follows it learns the dashes')
    const bool have_points = !Overfull(totals[0], *n_pts64, scene_cap);
    const uint32_t N = job.n + (job.closed ? 1u : 0u);
    const unsigned long long T = (pat.dashed && have_points) ? WalkLength(scene, job, N, lane) : 0ull;
    const DashPlan plan = PlanOf(pat, T, job.closed);
    if (plan.mode != kDashOutline) {
        unsigned long long inside = 0, q_base = 0;
        for (uint32_t base = 0; base + 1u < N; base += 64u) {
            const uint32_t k = base + lane;
            const unsigned long long q = k + 1u < N ? SegFix(WalkPoint(scene, job, k), WalkPoint(scene, job, k + 1u)) : 0ull;
            const unsigned long long q1 = q_base + WaveScanQ(q, lane);
            if (k + 1u < N && q1 > 0 && q1 < T && CountAt(pat, q1).inside) ++inside;  // vertex k + 1 lies inside a dash
            q_base = Bcast64(q1, 63u);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) inside += __shfl_xor(inside, d, 64);
        const long long seg = 5, J = static_cast<long long>(lay.join_size), C = static_cast<long long>(lay.cap_size);
        long long cnt = static_cast<long long>(plan.nd) * (seg + 2 * C) + (seg + J) * static_cast<long long>(inside);
        if (plan.mode == kDashMerged) cnt += seg + 2 * J - 2 * C;  // one segment and two joins more, one pair of caps fewer
        total = static_cast<unsigned long long>(cnt);
    }
    if (total > kDashCountCap) total = kDashCountCap;
    if (lane == 0) {
        out_cnt[s] = static_cast<uint32_t>(total);
        if (total) atomicAdd(out_total, total);
    }
}

__global__ __launch_bounds__(256) void KDashCount(const pm_path *paths, uint32_t n_paths, const pm_path_el *els, float width_scale, const uint32_t *el_ptoff,
                                                  const uint32_t *el_mvoff, const uint32_t *path_item_base, const uint32_t *path_pt_base,
                                                  const uint32_t *sub_first_el, const uint32_t *totals, const unsigned long long *n_pts64,
                                                  const uint32_t *path_dash, const pm_path_dash *dashes, const float *dash_values, const uint8_t *scene,
                                                  uint32_t scene_cap, uint32_t *out_cnt, unsigned long long *out_total) {
    __shared__ unsigned long long s_pf[kDashWaves][66];
    DashCountBody<false>(s_pf, paths, n_paths, els, width_scale, GroupTable{nullptr, nullptr}, el_ptoff, el_mvoff, path_item_base, path_pt_base,
                         sub_first_el, totals, n_pts64, path_dash, dashes, dash_values, scene, scene_cap, out_cnt, out_total);
}

__global__ __launch_bounds__(256) void KDashCountGrouped(const pm_path *paths, uint32_t n_paths, const pm_path_el *els, GroupTable gt,
                                                         const uint32_t *el_ptoff, const uint32_t *el_mvoff, const uint32_t *path_item_base,
                                                         const uint32_t *path_pt_base, const uint32_t *sub_first_el, const uint32_t *totals,
                                                         const unsigned long long *n_pts64, const uint32_t *path_dash, const pm_path_dash *dashes,
                                                         const float *dash_values, const uint8_t *scene, uint32_t scene_cap, uint32_t *out_cnt,
                                                         unsigned long long *out_total) {
    __shared__ unsigned long long s_pf[kDashWaves][66];
    DashCountBody<true>(s_pf, paths, n_paths, els, 0.0f, gt, el_ptoff, el_mvoff, path_item_base, path_pt_base, sub_first_el, totals, n_pts64,
                        path_dash, dashes, dash_values, scene, scene_cap, out_cnt, out_total);
}

// What a lane knows of its segment k during one step of KDash (LDS, a record per lane).
struct DashSeg {
    unsigned long long Q0, q;            // Q[k], q_k
    float ax, ay, bx, by;                // W[k], W[k + 1]
    uint32_t cs0, cs1, ce0, ce1;         // the dashes that start on it are [cs0, cs1), those that end on it [ce0, ce1)
    uint32_t iex, in0;                   // vertices inside dashes before k; vertex k is inside one
    uint32_t pex, pad;                   // pieces before this lane's
};

// Where dash d begins and ends on the walk.
struct DashEnds {
    bool valid;
    uint32_t d, lo, hi, ilo;  // its inside vertices are [lo, hi); ilo = vertices inside dashes before lo
    float2 sp, ep;
};

// The poly-line a piece belongs to: part 0 (only the merged pair has one: the last dash) followed by part 1.
struct DashPoly {
    uint32_t lo0, n0, lo1, n1;
    float2 sp0, ep0, sp1, ep1;
    unsigned long long E;  // its first entry
};

__device__ __forceinline__ float2 CutPoint(V2 a, V2 b, unsigned long long Q0, unsigned long long q, unsigned long long s) {
    if (s == Q0) return make_float2(static_cast<float>(a.x), static_cast<float>(a.y));
    if (s == Q0 + q) return make_float2(static_cast<float>(b.x), static_cast<float>(b.y));
    const double t = static_cast<double>(s - Q0) / static_cast<double>(q);
    const double x = a.x + (b.x - a.x) * t, y = a.y + (b.y - a.y) * t;
    return make_float2(static_cast<float>(x), static_cast<float>(y));
}

__device__ __forceinline__ float2 CutOn(const DashSeg &g, unsigned long long s) {
    return CutPoint(V2{static_cast<double>(g.ax), static_cast<double>(g.ay)}, V2{static_cast<double>(g.bx), static_cast<double>(g.by)}, g.Q0, g.q, s);
}

// The segment that owns position s (start rule: Q[k] <= s < Q[k + 1]; end rule: Q[k] < s <= Q[k + 1]) and the point there, found
// by walking on from segment k_from, where the walk stands at q_from.  The whole wave, uniform result.
struct DashCut {
    uint32_t k;
    float2 pt;
};

__device__ __forceinline__ DashCut LocateCut(const uint8_t *scene, const OutlineJob &job, uint32_t N, uint32_t k_from, unsigned long long q_from,
                                             unsigned long long s, bool end_rule, uint32_t lane) {
    for (uint32_t base = k_from; base + 1u < N; base += 64u) {
        const uint32_t k = base + lane;
        const bool valid = k + 1u < N;
        const V2 a = WalkPoint(scene, job, valid ? k : 0u), b = WalkPoint(scene, job, valid ? k + 1u : 0u);
        const unsigned long long q = valid ? SegFix(a, b) : 0ull;
        const unsigned long long q1 = q_from + WaveScanQ(q, lane), q0 = q1 - q;
        const bool hit = q != 0 && (end_rule ? (q0 < s && s <= q1) : (q0 <= s && s < q1));
        const unsigned long long m = __ballot(hit);
        if (m != 0ull) {  // (uniform)
            const uint32_t src = static_cast<uint32_t>(__popcll((m & (0ull - m)) - 1ull));
            const float2 c = CutPoint(a, b, q0, q ? q : 1ull, hit ? s : q0);
            const float x = __uint_as_float(Bcast32(__float_as_uint(c.x), src)), y = __uint_as_float(Bcast32(__float_as_uint(c.y), src));
            return DashCut{base + src, make_float2(x, y)};
        }
        q_from = Bcast64(q1, 63u);
    }
    const V2 e = WalkPoint(scene, job, N - 1u);  // (not reached: every position asked for lies on a segment of a length)
    return DashCut{N >= 2u ? N - 2u : 0u, make_float2(static_cast<float>(e.x), static_cast<float>(e.y))};
}

__device__ __forceinline__ V2 PolyPoint(const uint8_t *scene, const OutlineJob &job, const DashPoly poly, uint32_t p) {
    const bool first = p < poly.n0;
    const uint32_t i = first ? p : p - poly.n0, n = first ? poly.n0 : poly.n1, lo = first ? poly.lo0 : poly.lo1;
    const float2 sp = first ? poly.sp0 : poly.sp1, ep = first ? poly.ep0 : poly.ep1;
    if (i == 0) return V2{static_cast<double>(sp.x), static_cast<double>(sp.y)};
    if (i + 1u >= n) return V2{static_cast<double>(ep.x), static_cast<double>(ep.y)};
    return WalkPoint(scene, job, lo + i - 1u);
}

__device__ __forceinline__ bool PointsDir(V2 a, V2 b, V2 *u) {
    const double dx = b.x - a.x, dy = b.y - a.y;
    if (dx == 0.0 && dy == 0.0) return false;
    const double len = sqrt(dx * dx + dy * dy);
    u->x = dx / len;
    u->y = dy / len;
    return true;
}

// din(i) (back) / dout(i) of D14 on the dash's own poly-line, an open one
__device__ __forceinline__ bool PolyDir(const uint8_t *scene, const OutlineJob &job, const DashPoly poly, uint32_t n, uint32_t i, bool back, V2 *u) {
    if (back) {
        for (uint32_t k = i; k > 0;) {
            --k;
            if (PointsDir(PolyPoint(scene, job, poly, k), PolyPoint(scene, job, poly, k + 1u), u)) return true;
        }
    } else {
        for (uint32_t k = i; k + 1u < n; ++k)
            if (PointsDir(PolyPoint(scene, job, poly, k), PolyPoint(scene, job, poly, k + 1u), u)) return true;
    }
    return false;
}

// One piece: what vertex p of the dash's poly-line adds to its D14 outline -- the segment that starts there, its join, or a cap.
__device__ __forceinline__ void EmitDashPiece(const uint8_t *scene, const OutlineJob &job, OutlineSink &sink, const DashPoly poly, uint32_t p, unsigned long long J,
                              unsigned long long C) {
    const uint32_t n = poly.n0 + poly.n1, nseg = n - 1u;
    const double hw = job.hw;
    const unsigned long long joins_at = poly.E + 5ull * nseg, caps_at = joins_at + J * (nseg - 1u);
    const CornerKind join_kind = job.join == PM_STROKE_JOIN_BEVEL ? kCornerBevel : (job.join == PM_STROKE_JOIN_MITER ? kCornerMiter : kCornerFan);
    const CornerKind cap_kind = job.cap == PM_STROKE_CAP_SQUARE ? kCornerSquare : kCornerFan;
    const V2 pt = PolyPoint(scene, job, poly, p);
    if (p < nseg) {
        const V2 b = PolyPoint(scene, job, poly, p + 1u);
        V2 u;
        const unsigned long long e = poly.E + 5ull * p;
        if (PointsDir(pt, b, &u)) {
            const double nx = -(hw * u.y), ny = hw * u.x;
            sink.Point(e + 0, pt.x - nx, pt.y - ny);
            sink.Point(e + 1, b.x - nx, b.y - ny);
            sink.Point(e + 2, b.x + nx, b.y + ny);
            sink.Point(e + 3, pt.x + nx, pt.y + ny);
        } else {
            for (uint32_t k = 0; k < 4; ++k) sink.Point(e + k, pt.x, pt.y);
        }
        sink.Separator(e + 4, e);
    }
    const bool joined = p > 0 && p < nseg, capped = C != 0 && (p == 0 || p == nseg);
    if (!joined && !capped) return;
    V2 d1{0.0, 0.0}, d2{0.0, 0.0};
    const bool has1 = PolyDir(scene, job, poly, n, p, true, &d1), has2 = PolyDir(scene, job, poly, n, p, false, &d2);
    if (joined) {
        EmitJoin(sink, joins_at + J * (p - 1u), join_kind, pt, has1, d1, has2, d2, hw, job.mlim, job.L);
    } else {
        const uint32_t end = p == 0 ? 0u : 1u;
        V2 d = end == 0 ? V2{-d2.x, -d2.y} : d1;
        if (!has1 && !has2) d = V2{end == 0 ? -1.0 : 1.0, 0.0};  // a dot
        EmitCorner(sink, caps_at + C * end, cap_kind, pt, V2{d.y, -d.x}, V2{-d.y, d.x}, d, true, false, 0.0, hw, job.mlim, job.L);
    }
}

// first lane whose value (DashSeg::cs1 / ce1) is above d
__device__ __forceinline__ uint32_t FirstAbove(const DashSeg *seg, bool ends, uint32_t d) {
    uint32_t lo = 0, hi = 63;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((ends ? seg[mid].ce1 : seg[mid].cs1) > d) hi = mid; else lo = mid + 1u;
    }
    return lo;
}

// A wave per dashed sub-path: the same walk, 64 segments a step.  Within a step the work is dealt by PIECES, not by segments: the
// scan of the segments' piece counts hands the lanes (dash start -> cap + first quad), (inside vertex -> join + following quad),
// (dash end -> cap), so that one long segment with a thousand dashes occupies 64 lanes, not one.  A dash that is still open at
// the end of a step is looked ahead for once (LocateCut) and carried: its outline's layout needs its vertex count.
template <bool kGrouped>
__device__ __forceinline__ void DashBody(unsigned long long (*s_pf)[66], DashSeg (*s_seg)[64], const pm_path *paths, uint32_t n_paths,
                                         const pm_path_el *els, float width_scale_u, const GroupTable &gt, const uint32_t *el_ptoff,
                                         const uint32_t *el_mvoff, const uint32_t *path_item_base, const uint32_t *path_pt_base,
                                         const uint32_t *sub_first_el, const uint32_t *totals, const unsigned long long *n_pts64,
                                         const uint32_t *out_cnt, const uint32_t *out_off, const unsigned long long *out_total,
                                         const uint32_t *path_dash, const pm_path_dash *dashes, const float *dash_values, uint8_t *scene,
                                         uint32_t scene_cap) {
    const uint32_t s = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t lane = threadIdx.x & 63u, wave = (threadIdx.x >> 6) & (kDashWaves - 1u);
    const uint32_t n_items = totals[0], n_subs = totals[2];
    if (s >= n_subs || Overfull(n_items, *n_pts64, scene_cap)) return;  // (whole waves)
    const OutlineJob job = MakeOutlineJob<kGrouped>(paths, n_paths, els, width_scale_u, gt, el_ptoff, el_mvoff, path_item_base, path_pt_base, sub_first_el, n_items, s);
    if (!job.styled || !IsDashed(path_dash, job.path)) return;  // (uniform)
    const float width_scale = WidthScaleOf<kGrouped>(width_scale_u, gt, job.path);
    const DashPattern pat = LoadPattern(s_pf[wave], DashOf(dashes, path_dash[job.path]), dash_values, width_scale, lane);
    const OutlineLayout lay = LayoutOf(job);
    const size_t outlines_start = sizeof(SimpleGroup) + static_cast<size_t>(n_items) * (sizeof(ShortBbox) + kItemSize) + 8 * static_cast<size_t>(out_total[1]);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    OutlineSink sink{scene, outlines_start + 8 * static_cast<size_t>(out_off[s]), scene_cap, nan, nan, nan, nan, false};
    const uint32_t N = job.n + (job.closed ? 1u : 0u);
    const unsigned long long T = pat.dashed ? WalkLength(scene, job, N, lane) : 0ull;
    const DashPlan plan = PlanOf(pat, T, job.closed);
    if (plan.mode == kDashOutline) {
        OutlineSubpath(scene, job, lay, sink, lane);
        WriteOutlineItem(scene, scene_cap, n_items, job, sink, out_cnt[s], lane);
        return;
    }
    const unsigned long long J = lay.join_size, C = lay.cap_size, per_dash = 5ull + 2ull * C, per_inside = 5ull + J;
    const uint32_t nd = static_cast<uint32_t>(plan.nd);  // (a scene that fits holds fewer than 2^29 dashes)
    const long long m_lo = static_cast<long long>(pat.m_lo);
    DashSeg *seg = s_seg[wave];

    DashPoly merged{0, 0, 0, 0, make_float2(0.f, 0.f), make_float2(0.f, 0.f), make_float2(0.f, 0.f), make_float2(0.f, 0.f), 0ull};
    unsigned long long merged_size = 0;
    if (plan.mode == kDashMerged) {  // (uniform) the last dash's points, then the first one's
        const DashSpan f = SpanOf(pat, pat.m_lo), l = SpanOf(pat, pat.m_lo + nd - 1ull);
        const DashCut ls = LocateCut(scene, job, N, 0u, 0ull, static_cast<unsigned long long>(l.A), false, lane);
        const DashCut le = LocateCut(scene, job, N, 0u, 0ull, T, true, lane);
        const DashCut fs = LocateCut(scene, job, N, 0u, 0ull, 0ull, false, lane);
        const DashCut fe = LocateCut(scene, job, N, 0u, 0ull, static_cast<unsigned long long>(f.B), true, lane);
        merged.lo0 = ls.k + 1u;
        merged.n0 = 2u + (le.k + 1u - merged.lo0);
        merged.sp0 = ls.pt;
        merged.ep0 = le.pt;
        merged.lo1 = fs.k + 1u;
        merged.n1 = 2u + (fe.k + 1u - merged.lo1);
        merged.sp1 = fs.pt;
        merged.ep1 = fe.pt;
        const unsigned long long n = merged.n0 + merged.n1;
        merged_size = 5ull * (n - 1ull) + J * (n - 2ull) + 2ull * C;
    }

    DashEnds cur{false, 0, 0, 0, 0, make_float2(0.f, 0.f), make_float2(0.f, 0.f)}, nxt = cur;
    unsigned long long q_base = 0;
    uint32_t i_base = 0, cs_prev = 0, ce_prev = 0, in_prev = 0;
    for (uint32_t base = 0; base + 1u < N; base += 64u) {
        const uint32_t k = base + lane;
        const bool valid = k + 1u < N;
        const V2 a = WalkPoint(scene, job, valid ? k : 0u), b = WalkPoint(scene, job, valid ? k + 1u : 0u);
        const unsigned long long q = valid ? SegFix(a, b) : 0ull;
        const unsigned long long q1 = q_base + WaveScanQ(q, lane), q0 = q1 - q;
        const DashCount c1 = CountAt(pat, q1);
        const uint32_t cs1 = q1 > 0 ? static_cast<uint32_t>(c1.s - m_lo) : 0u;
        const uint32_t ce1 = q1 >= T ? nd : static_cast<uint32_t>(c1.e - m_lo);
        const uint32_t in1 = (c1.inside && q1 > 0 && q1 < T) ? 1u : 0u;
        uint32_t cs0 = __shfl_up(cs1, 1u, 64), ce0 = __shfl_up(ce1, 1u, 64), in0 = __shfl_up(in1, 1u, 64);
        if (lane == 0) {
            cs0 = cs_prev;
            ce0 = ce_prev;
            in0 = in_prev;
        }
        const unsigned long long in_mask = __ballot(in0 != 0);
        const uint32_t iex = i_base + static_cast<uint32_t>(__popcll(in_mask & ((1ull << lane) - 1ull)));
        const uint32_t pieces = in0 + (cs1 - cs0) + (ce1 - ce0);
        const uint32_t pin = WaveScan32(pieces, lane);
        // (every piece but a butt end writes entries and a dash has one end: a bound that keeps a wrong count from looping long)
        const uint32_t n_pieces = min(Bcast32(pin, 63u), 64u + out_cnt[s]), cs_end = Bcast32(cs1, 63u), ce_end = Bcast32(ce1, 63u);
        const unsigned long long q_end = Bcast64(q1, 63u);
        seg[lane] = DashSeg{q0, q, static_cast<float>(a.x), static_cast<float>(a.y), static_cast<float>(b.x), static_cast<float>(b.y),
                            cs0, cs1, ce0, ce1, iex, in0, pin - pieces, 0u};
        DashWaveSync();

        nxt.valid = false;
        if (ce_end < cs_end) {  // (uniform) the last dash begun is open at the step's end
            const uint32_t dl = cs_end - 1u;
            if (cur.valid && cur.d == dl) {
                nxt = cur;
            } else {
                const DashSpan sp = SpanOf(pat, pat.m_lo + dl);
                const DashSeg &gs = seg[FirstAbove(seg, false, dl)];
                nxt.d = dl;
                nxt.lo = base + static_cast<uint32_t>(&gs - seg) + 1u;
                nxt.ilo = gs.iex + gs.in0;
                nxt.sp = CutOn(gs, static_cast<unsigned long long>(sp.A > 0 ? sp.A : 0));
                const DashCut ce = LocateCut(scene, job, N, base + 64u, q_end, static_cast<unsigned long long>(sp.B) < T ? static_cast<unsigned long long>(sp.B) : T,
                                             true, lane);
                nxt.ep = ce.pt;
                nxt.hi = ce.k + 1u;
                nxt.valid = true;
            }
        }

        for (uint32_t t = lane; t < n_pieces; t += 64u) {
            uint32_t lo = 0, hi = 63;  // the last lane with pex <= t owns piece t
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1u) >> 1;
                if (seg[mid].pex <= t) lo = mid; else hi = mid - 1u;
            }
            const DashSeg &g = seg[lo];
            const uint32_t kv = base + lo;
            uint32_t u = t - g.pex, d, kind;  // kind 0: the inside vertex kv, 1: a dash's start, 2: its end
            if (u < g.in0) {
                kind = 0;
                d = g.cs0 - 1u;
            } else if ((u -= g.in0) < g.cs1 - g.cs0) {
                kind = 1;
                d = g.cs0 + u;
            } else {
                kind = 2;
                d = g.ce0 + (u - (g.cs1 - g.cs0));
            }
            // (every field chosen on its own: a struct picked from two lives in memory)
            const bool mg = plan.mode == kDashMerged && (d == 0 || d + 1u == nd);
            const bool from_cur = cur.valid && cur.d == d, from_nxt = nxt.valid && nxt.d == d;
            uint32_t e_lo = from_cur ? cur.lo : nxt.lo, e_hi = from_cur ? cur.hi : nxt.hi, e_ilo = from_cur ? cur.ilo : nxt.ilo;
            float2 e_sp = from_cur ? cur.sp : nxt.sp, e_ep = from_cur ? cur.ep : nxt.ep;
            if (!mg && !from_cur && !from_nxt) {
                const DashSpan sp = SpanOf(pat, pat.m_lo + d);
                const DashSeg &gs = seg[FirstAbove(seg, false, d)];
                e_lo = base + static_cast<uint32_t>(&gs - seg) + 1u;
                e_ilo = gs.iex + gs.in0;
                e_sp = CutOn(gs, static_cast<unsigned long long>(sp.A > 0 ? sp.A : 0));
                if (sp.zero) {
                    e_hi = e_lo;
                    e_ep = e_sp;
                } else {
                    const uint32_t le = FirstAbove(seg, true, d);
                    e_hi = base + le + 1u;
                    e_ep = CutOn(seg[le], static_cast<unsigned long long>(sp.B) < T ? static_cast<unsigned long long>(sp.B) : T);
                }
            }
            DashPoly poly;
            poly.lo0 = mg ? merged.lo0 : 0u;
            poly.n0 = mg ? merged.n0 : 0u;
            poly.sp0 = mg ? merged.sp0 : e_sp;
            poly.ep0 = mg ? merged.ep0 : e_sp;
            poly.lo1 = mg ? merged.lo1 : e_lo;
            poly.n1 = mg ? merged.n1 : 2u + (e_hi - e_lo);
            poly.sp1 = mg ? merged.sp1 : e_sp;
            poly.ep1 = mg ? merged.ep1 : e_ep;
            poly.E = mg ? 0ull
                        : (plan.mode == kDashMerged ? merged_size + (d - 1ull) * per_dash + per_inside * (e_ilo - (merged.n1 - 2u)) : d * per_dash + per_inside * e_ilo);
            uint32_t p;
            if (mg && d == 0) p = kind == 0 ? poly.n0 + 1u + (kv - poly.lo1) : (kind == 1 ? poly.n0 : poly.n0 + poly.n1 - 1u);
            else if (mg) p = kind == 0 ? 1u + (kv - poly.lo0) : (kind == 1 ? 0u : poly.n0 - 1u);
            else p = kind == 0 ? 1u + (kv - e_lo) : (kind == 1 ? 0u : poly.n1 - 1u);
            EmitDashPiece(scene, job, sink, poly, p, J, C);
        }
        DashWaveSync();  // (the records are rewritten by the next step)
        q_base = q_end;
        i_base += static_cast<uint32_t>(__popcll(in_mask));
        cs_prev = cs_end;
        ce_prev = ce_end;
        in_prev = Bcast32(in1, 63u);
        cur = nxt;
    }
    WriteOutlineItem(scene, scene_cap, n_items, job, sink, out_cnt[s], lane);
}

__global__ __launch_bounds__(256) void KDash(const pm_path *paths, uint32_t n_paths, const pm_path_el *els, float width_scale, const uint32_t *el_ptoff,
                                             const uint32_t *el_mvoff, const uint32_t *path_item_base, const uint32_t *path_pt_base,
                                             const uint32_t *sub_first_el, const uint32_t *totals, const unsigned long long *n_pts64,
                                             const uint32_t *out_cnt, const uint32_t *out_off, const unsigned long long *out_total, const uint32_t *path_dash,
                                             const pm_path_dash *dashes, const float *dash_values, uint8_t *scene, uint32_t scene_cap) {
    __shared__ unsigned long long s_pf[kDashWaves][66];
    __shared__ DashSeg s_seg[kDashWaves][64];
    DashBody<false>(s_pf, s_seg, paths, n_paths, els, width_scale, GroupTable{nullptr, nullptr}, el_ptoff, el_mvoff, path_item_base, path_pt_base,
                    sub_first_el, totals, n_pts64, out_cnt, out_off, out_total, path_dash, dashes, dash_values, scene, scene_cap);
}

__global__ __launch_bounds__(256) void KDashGrouped(const pm_path *paths, uint32_t n_paths, const pm_path_el *els, GroupTable gt,
                                                    const uint32_t *el_ptoff, const uint32_t *el_mvoff, const uint32_t *path_item_base,
                                                    const uint32_t *path_pt_base, const uint32_t *sub_first_el, const uint32_t *totals,
                                                    const unsigned long long *n_pts64, const uint32_t *out_cnt, const uint32_t *out_off,
                                                    const unsigned long long *out_total, const uint32_t *path_dash, const pm_path_dash *dashes,
                                                    const float *dash_values, uint8_t *scene, uint32_t scene_cap) {
    __shared__ unsigned long long s_pf[kDashWaves][66];
    __shared__ DashSeg s_seg[kDashWaves][64];
    DashBody<true>(s_pf, s_seg, paths, n_paths, els, 0.0f, gt, el_ptoff, el_mvoff, path_item_base, path_pt_base, sub_first_el, totals, n_pts64,
                   out_cnt, out_off, out_total, path_dash, dashes, dash_values, scene, scene_cap);
}
