// Host runtime behind the C ABI: the MI355X replacement for PietRenderer
// (TestApp/PietRenderer.{h,m}).  One context = one GPU + one HIP stream.
//
//   -initWithMetalKitView:               -> pm_create      (PietRenderer.m:23-57)
//   -mtkView:drawableSizeWillChange:     -> pm_resize      (PietRenderer.m:105-146)
//   init_test_scene(_sceneBuf.contents)  -> pm_scene_buffer / pm_upload_scene /
//                                           pm_flatten_and_encode (PietRenderer.m:203-205)
//   -drawInMTKView:                      -> pm_render      (PietRenderer.m:59-103)
//
// Frames overlap like the reference's command buffers ([commandBuffer commit] never waits,
// PietRenderer.m:102): frame N runs its three kernels back to back on stream N % 4 and owns
// frame slot N % 4 (arena, queues, command lists, framebuffer), so frames in flight share no
// mutable state and need no cross-stream events; the in-order queues do the ordering.  At 4K
// every kernel alone leaves most of the chip idle (its span is set by its longest dependent
// chain), and four frames side by side fill it.  Measured alternatives: one stream per kernel
// stage chained by events (each cross-stream dependency costs 10-15 us to release the next
// dispatch) was 5 % slower; more than four streams (ROCm's default number of hardware queues)
// was slower still.  A frame rendered into a caller-owned buffer (pm_render_to) runs on the
// caller's stream.
//
// There is deliberately no CPU rendering path in this library: without a gfx950
// device pm_create fails with PM_ERR_NO_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/piet_metal_amd.h"
#include "pm_device.h"
#include "pm_dev_array.h"
#include "pm_plan.h"
#include "pm_flatten.h"
#include "pm_hit_test.h"  // pm_hit_kernel + LaunchHitTest: point hit testing
#include "pm_hit_frame.h"  // pm_hit_frame_kernel + LaunchHitFrame: the item map, a workgroup per 16 x 16 tile
#include "pm_hit_rect.h"   // pm_hit_rects_kernel, pm_select_rect_kernel: rectangle queries (pick with a tolerance, marquee selection)
#include "pm_hit_poly.h"   // pm_select_polygon_kernel: polygon queries (lasso, rotated marquee)
#include "pm_hit_stack.h"  // pm_hit_stack_kernel, pm_hit_rects_stack_kernel: hit stacks (the k topmost items under a point or rectangle)
#include "pm_coverage.h"   // pm_item_coverage_kernel: covered, visible and topmost pixels per item, a workgroup per 16 x 16 tile
#include "pm_snap.h"       // pm_snap_kernel: snapping (the nearest vertex or edge to a cursor)
#include "pm_snap_cross.h" // pm_cross_kernel: snapping to intersections (the nearest crossing of two edges)
#include "pm_bounds.h"     // pm_item_bounds_kernel, pm_union_bounds_kernel: item, selection and group boxes
#include "pm_measure.h"    // pm_item_lengths_kernel, pm_points_at_length_kernel, pm_positions_on_edges_kernel: path measurement
#include "pm_resample.h"   // pm_resample_kernel: many points along an item in one walk
#include "pm_trim.h"       // pm_trim_kernel: the piece of an item between two lengths
#include "pm_crossings.h"  // pm_crossings_kernel: every point where two items' edges cross
#include "pm_layout.h"

namespace {

thread_local std::string g_last_error;

void SetError(const std::string &s) { g_last_error = s; }

int HipFail(hipError_t e, const char *what) {
    SetError(std::string(what) + ": " + hipGetErrorString(e));
    return PM_ERR_HIP;
}

#define PM_TRY(expr)                                         \
    do {                                                     \
        hipError_t e_ = (expr);                              \
        if (e_ != hipSuccess) return HipFail(e_, #expr);     \
    } while (0)

// ---- binary16 helpers for the pinned lookup tables ----------------------------------------
// (host-side only; the kernels use native _Float16)

uint16_t HalfBitsFromDouble(double d) {  // one rounding, nearest-even
    if (d != d) return 0x7e00;
    uint16_t sign = 0;
    if (std::signbit(d)) {
        sign = 0x8000;
        d = -d;
    }
    if (d == 0.0) return sign;
    if (d >= 65520.0) return sign | 0x7c00;
    int e;
    const double m = std::frexp(d, &e);  // d = m * 2^e, m in [0.5, 1)
    int E = e - 1;
    if (E < -14) return sign | static_cast<uint16_t>(std::nearbyint(std::ldexp(d, 24)));
    double q = std::nearbyint(std::ldexp(m, 11));  // [1024, 2048]
    if (q == 2048.0) {
        q = 1024.0;
        E += 1;
    }
    return sign | static_cast<uint16_t>(((E + 15) << 10) | (static_cast<int>(q) - 1024));
}

float HalfBitsToFloat(uint16_t h) {
    const int s = h >> 15, e = (h >> 10) & 31, m = h & 1023;
    float v;
    if (e == 0) v = std::ldexp(static_cast<float>(m), -24);
    else if (e == 31) v = m ? NAN : INFINITY;
    else v = std::ldexp(static_cast<float>(m + 1024), e - 25);
    return s ? -v : v;
}

inline uint16_t RoundHalf(float f) { return HalfBitsFromDouble(static_cast<double>(f)); }

struct Luts {
    uint32_t srgb2lin[256];
    uint32_t unorm2h[256];
    uint8_t lin2srgb[65536];
};

// The three tables pin what Metal leaves to its half library:
//   unpack_unorm4x8_srgb_to_half  : exact EOTF, rounded once to binary16
//   final select(1.055*pow(rgb,1/2.4)-0.055, 12.92*rgb, rgb<0.0031308) on half3
//   (PietRender.metal:563), constants and exponent taken in binary16, pow
//   correctly rounded to binary16, then clamp*255 round-half-even to unorm8.
void BuildLuts(Luts *l) {
    for (int i = 0; i < 256; ++i) {
        const double c = i / 255.0;
        const double lin = (c <= 0.04045) ? c / 12.92 : std::pow((c + 0.055) / 1.055, 2.4);
        l->srgb2lin[i] = HalfBitsFromDouble(lin);
        l->unorm2h[i] = HalfBitsFromDouble(c);
    }
    const float thr = HalfBitsToFloat(RoundHalf(0.0031308f));
    const float k = HalfBitsToFloat(RoundHalf(12.92f));
    const float s = HalfBitsToFloat(RoundHalf(1.055f));
    const float o = HalfBitsToFloat(RoundHalf(0.055f));
    const double ex = HalfBitsToFloat(RoundHalf(1.0f / 2.4f));
    for (uint32_t h = 0; h < 65536; ++h) {
        const float x = HalfBitsToFloat(static_cast<uint16_t>(h));
        if (x != x) {
            l->lin2srgb[h] = 0;
            continue;
        }
        float y;
        if (x < thr) {
            y = HalfBitsToFloat(RoundHalf(k * x));
        } else {
            const float p = HalfBitsToFloat(HalfBitsFromDouble(std::pow(static_cast<double>(x), ex)));
            const float sp = HalfBitsToFloat(RoundHalf(s * p));
            y = HalfBitsToFloat(RoundHalf(sp - o));
        }
        const float cl = std::fmin(std::fmax(y, 0.0f), 1.0f);
        l->lin2srgb[h] = static_cast<uint8_t>(std::rintf(cl * 255.0f));
    }
}

}  // namespace


namespace {
constexpr int kMaxSlots = 16;
constexpr int kDefaultFrameStreams = 4;  // = ROCm's default hardware queues; measured best on Tiger 4K

int EnvInt(const char *name, int dflt, int lo, int hi) {
    const char *v = std::getenv(name);
    if (!v || !*v) return dflt;
    return std::max(lo, std::min(hi, std::atoi(v)));
}
}

struct FrameSlot {
    uint8_t *d_fb = nullptr;  // this slot's framebuffer (pm_render); pm_render_to uses the caller's
    size_t fb_cap = 0;        // bytes allocated for it, and entries the queue / per-tile tables were allocated for: a viewport that
    size_t queue_cap = 0;     // entries of d_queue (all sub-queues together); the per-tile tables start behind them
    size_t tables_cap = 0;    // fits keeps the buffers (grow only: a resize to anything smaller than what came before allocates nothing)
    uint32_t *d_arena = nullptr;
    uint32_t arena_cap = 0;  // dwords allocated for this slot (allocated when the slot is first used)
    uint4 *d_queue = nullptr;
    uint32_t *d_tile_state = nullptr;
    uint32_t *d_tile_ptcl = nullptr;
    uint32_t *d_tile_ncmd = nullptr;
    pm::DevArray<uint4> ptcl;  // tile arena: per-tile pieces + command lists, in quads (16 B; never more than 2^31 of them)
    uint2 *d_row_bbox = nullptr;  // per-tile-row item lists of this slot's frame (large scenes)
    uint32_t *d_row_item = nullptr;
    uint64_t row_cap = 0;         // entries allocated for them
    uint32_t state_epoch = 0;     // arena_epoch its tile_state was last reset for (0: never)
    uint32_t vp_epoch = 0;        // viewport its buffers were allocated for (pm_ctx::vp_epoch; stale ones go when the slot is next used)
    pm::Counters *d_ctr = nullptr;  // two: a frame's binning kernel zeroes the one the slot's next frame uses
    uint32_t *h_overflow = nullptr;  // pinned: raised by a frame of this slot whose tile arena ran out (what pm_sync looks at first)
    uint32_t *d_overflow = nullptr;  // ... as the device sees it ([1]: a one-launch frame of this slot gave up waiting)
    uint4 *d_fifo = nullptr;         // one-launch frames: kFifos x fifo_cap queue entries, all zero between frames (made when first needed)
    uint32_t fifo_cap = 0;
    uint32_t parity = 0;
    hipEvent_t ev_done = nullptr;  // end of the slot's last frame
    bool in_flight = false;        // a frame using this slot was submitted; ev_done marks its end
    bool needs_check = false;      // ... and pm_sync has not yet looked at its overflow flag (SyncAll only waits)
    pm::FrameParams params{};
    hipStream_t frame_stream = nullptr;  // stream the slot's last frame ran on (compared, never dereferenced, if user_stream)
    bool user_stream = false;            // the frame ran on a caller-owned stream: ev_done was recorded behind it at submit
};

struct pm_ctx {
    int device = 0;
    hipStream_t stream = nullptr;      // == streams[0]: scene upload, flatten, index, debug replays
    std::vector<hipStream_t> streams;  // frame N runs on streams[N % n]; stream == streams[0]
    bool fold_clear = true;  // a frame alone: pm_fine_kernel's launch also writes the resolved tiles (no pm_clear_kernel launch)
    int fold_clear_mode = 2;  // PM_FOLD_CLEAR: 0 never, 1 always, 2 (default) per frame -- folded when the frame is alone
    bool fused = true;       // pm_fine_kernel<true>: each tile's list is built and interpreted by the same wave(s)
    int handout = 0;         // tile hand-out: 0 = drawn for a lone frame, static when frames overlap; 1 = static; 2 = drawn
    int target_fmt = PM_FMT_RGBA8;  // byte order the kernels store pixels in (pm_set_target_format)
    uint32_t split_mode = 1;  // fine kernel: long lists get 4 waves per tile (16 measured no faster)
    // A frame whose tile kernel found it dense (above) is followed by frames whose tile kernel is the one-wave-per-tile instantiation:
    // 80 VGPRs and 19 KB of LDS instead of 96 and 31, six workgroups per CU instead of five (PM_DENSE_KERNEL=0: never).  The verdict is
    // the kernel's own, left in a pinned word by every frame (FrameSlot::h_overflow[2]); a new scene or viewport starts undecided.
    int dense_kernel_mode = 1;
    uint32_t fine_wg_dense = 6, fine_wg_dense_inflight = 4;  // PM_FINE_WG_PER_CU_DENSE, PM_FINE_WG_PER_CU_DENSE_INFLIGHT
    uint32_t frames_dense_kernel = 0;  // frames whose tile kernel was that instantiation (pm_tile_kernel_info)
    uint32_t dense_factor = 4;  // PM_DENSE_FACTOR: a frame whose long lists x this would fill every wave renders each tile with one wave
    uint32_t heavy_stream = 72, heavy_stream_lone = 40, vheavy_stream = 112;  // list-length classes (PM_HEAVY_STREAM / PM_VHEAVY_STREAM)
    uint32_t bin_waves_env = 0;     // PM_BIN_WAVES: 4 / 1 waves per strip row in pm_bin_kernel (0: by the number of strip rows, EnsureArena)
    uint32_t bin_waves_inflight = 1;  // PM_BIN_WAVES_INFLIGHT: waves per strip row for frames submitted behind frames still running (1 / 4)
    uint32_t bin_wg_per_cu = 0xff;  // pm_bin_kernel's workgroups per CU (PM_BIN_WG_PER_CU; 0 = one per strip row, default: by the number of strip rows)
    uint32_t coarse_wg_per_cu = 5, fine_wg_per_cu = 5;  // persistent grids (PM_COARSE_WG_PER_CU, PM_FINE_WG_PER_CU)
    uint32_t fine_wg_per_cu_inflight = 3;               // ... of a frame behind other frames (PM_FINE_WG_PER_CU_INFLIGHT)
    hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int n_cus = 0;
    // One launch per frame (pm_frame_kernel, pm_frame.hip): PM_ONE_LAUNCH=1 for every frame that has the device to itself,
    // whose strip rows fit the resident grid two to a workgroup, and that needs nothing the one kernel does not do (per-tile-row
    // item lists, a wave per strip row, separate list building).  Off by default: measured slower than two launches on every
    // scene ("one launch per frame") -- the chains that set a frame's length are strings of memory round trips, and
    // they stretch when the rest of the chip renders tiles beside them instead of idling.
    int one_launch_mode = 0;
    bool one_launch_split = false;    // PM_ONE_LAUNCH_SPLIT=1 (developer experiment): the kernel's two roles as two launches of it
    bool one_launch_broken = false;   // a frame gave up waiting inside the launch (pm_sync rendered it again): two launches from then on
    uint32_t frame_wg_per_cu = 0;     // resident workgroups of pm_frame_kernel per CU (0: cannot run five, one-launch frames are off)
    uint32_t frame_spin_ticks = 200000;  // PM_ONE_LAUNCH_SPIN_US x 100: a wait inside the launch gives up after this long
    pm::DevArray<uint32_t> sr_next_one;  // [work list] chains of the one-launch grid (0: the workgroup's last strip row)
    pm::DevArray<uint32_t> idle_sr;      // strip rows of the band no item reaches (the launch writes their pixels too)
    uint32_t frames_one_launch = 0;   // frames submitted as one launch (pm_one_launch_info)
    // pm_debug_capture_ptcl of a one-launch frame: the frame is rendered once more with the capture instantiation of its kernel
    uint32_t *cap_counts = nullptr, *cap_solid = nullptr;
    pm::Cmd *cap_cmds = nullptr;
    uint32_t cap_max = 0;

    // scene
    uint8_t *h_scene = nullptr;  // pinned staging (pm_scene_buffer): only pm_scene_reserve moves it
    size_t scene_cap = 0;        // its capacity
    uint8_t *d_scene = nullptr;
    size_t dev_scene_cap = 0;    // >= scene_cap: the device copy also grows on its own (flat groups, device flatten)
    // what the flatten kernels write while frames in flight still read d_scene; the two change places when the new scene is in
    // (a view change then no longer begins by waiting for the previous frame: 0.197 -> 0.15 ms per re-encoded 4K Tiger frame)
    uint8_t *d_scene_alt = nullptr;
    size_t dev_scene_alt_cap = 0;
    size_t scene_bytes = 0;       // resident bytes (with the flat form of nested groups appended)
    size_t user_scene_bytes = 0;  // what the caller uploaded / the flatten kernels wrote
    uint32_t dev_bbox_ix = 8, dev_items_ix = 0;  // the drawn group's ShortBbox / item arrays in d_scene
    uint32_t n_items = 0;
    // copy of header + bboxes + items (arena sizing).  After pm_repaint_groups (decision D17) it is not refreshed: the records are
    // geometry-valid and colour-stale (meta_colours_stale).  The host reads tags, point counts, point offsets and boxes from it,
    // never a colour; pm_fill_coverage, which hands a record back to the device, then fetches that record from the scene.
    std::vector<uint8_t> item_meta;
    bool meta_colours_stale = false;
    std::vector<uint32_t> chunk_base_host;  // source of the asynchronous upload of the chunk table
    uint32_t *d_chunk_base = nullptr;  // scene index: first chunk of every item (+ total)
    float4 *d_chunk_bbox = nullptr;    // scene index: bounding box of every chunk of segments
    float4 *d_sup_bbox = nullptr;      // ... and of every super-chunk (kSuperChunks consecutive chunk-table entries)
    size_t chunk_base_cap = 0, chunk_bbox_cap = 0, sup_bbox_cap = 0;
    uint32_t n_chunks = 0;

    // viewport
    uint32_t width = 0, height = 0, tiles_x = 0, tiles_y = 0, strips_x = 0;
    uint32_t row0 = 0, row1 = 0;
    size_t fb_stride = 0;
    size_t fb_bytes = 0;
    uint32_t vp_epoch = 1;  // bumped by every resize / band change

    // binning state shared by the slots
    // The plan in force (pm_plan.h: strip-row work list, arena regions, band list, the item boxes it was made for) -- its vectors are
    // the sources of the asynchronous uploads -- and its lists on the device (grow only).  A view change (pm_reflatten) plans with
    // every box widened by a tile, so that the scenes that follow can keep the plan while their boxes stay inside the widened ones
    // and their items keep their segment counts: no host sizing, no uploads, no waits (0.04 of an animated frame's 0.18 ms).
    pm::BinPlan plan;
    pm::DevArray<uint4> sr_desc;    // strip rows some item reaches: {strip row, arena region begin, end, next of the chain}
    pm::DevArray<uint2> sr_list;    // ... and, for large scenes, where their tile row's item list is
    uint32_t bin_prio_slots = 1024; // PM_BIN_PRIO_SLOTS
    // Heavy strip rows cut in two (round 6): binning ends with its heaviest strip rows (a 4K Tiger frame: 1 109 rows, the mean one
    // through at 15 us, the heaviest at 24), and a row's length is dependent steps of its four waves, so the heaviest rows get EIGHT:
    // two entries of the work list, tiles 0-7 and 8-15, a workgroup each, while the plan's rows leave workgroups of the resident
    // grid free.  Which rows: those the previous frames of this scene and viewport found heaviest (segment slots per strip row, left
    // in a pinned array by pm_bin_kernel; before any frame has said anything: by candidates, PM_BIN_SPLIT_CANDS).
    int bin_wt_mode = 2;             // PM_BIN_WT: binning's output stored write-through: 0 never, 1 always, 2 frames whose strip rows all fit the resident grid
    int bin_split_mode = 1;          // PM_BIN_SPLIT: 0 never, 1 while the resident grid has room, 2 every strip row (tests)
    uint32_t bin_split_cands = 1u << 30;  // PM_BIN_SPLIT_CANDS: a row with at least this many candidates is cut before any frame has reported (default: none --
                                          // candidates predict a row's segment slots poorly: of the 4K Tiger's 60 heaviest rows they name 32)
    uint32_t bin_split_slots = 224;  // PM_BIN_SPLIT_SLOTS: ... with at least this many segment slots, once frames have reported
    uint32_t bin_split_fill = 15;    // PM_BIN_SPLIT_FILL: cut rows while the work list stays within this many sixteenths of the resident grid
    pm::DevArray<uint4> sr_desc_whole;  // the same work list with every cut strip row whole again (same arena regions): what frames behind
                                        // running frames bin from -- there instructions count, not the frame's own latency (sustained -3 % with cuts)
    pm::DevArray<uint32_t> sr_slots;  // segment slots every entry of the work list found in the latest frame
    std::vector<uint32_t> fb_slots;  // per strip row of the band: the slots the frames of this scene and viewport reported (empty: nothing yet)
    std::vector<uint32_t> stage_slots;
    uint32_t frames_on_plan = 0;     // frames submitted since the plan in force was made
    uint32_t plans_fed_back = 0;     // plans remade from the frames' report (pm_binning_info)
    pm::DevArray<uint2> band_bbox;  // items that reach the band (bbox, scene index), paint order
    pm::DevArray<uint32_t> band_item;
    pm::DevArray<uint32_t> row_base;  // per-tile-row item lists (large scenes): offsets
    uint32_t frames_bin_wave = 0, frames_bin_wave_inflight = 0, frames_bin_no_chains = 0;  // pm_binning_info
    uint32_t arena_cap = 0;         // dwords per slot
    uint64_t ptcl_want = 0;         // commands a slot's list arena starts with / was grown to
    bool arena_dirty = true;
    bool replan_wide = false;         // the next plan widens the boxes (set by pm_reflatten)
    uint32_t arena_epoch = 0;       // bumped whenever the set of strip rows without a workgroup changes (EnsureArena)

    std::vector<FrameSlot> slot;
    uint32_t frame = 0;
    std::chrono::steady_clock::time_point last_submit{};  // when the previous frame was submitted, and what was found then:
    bool prev_running = false;                            // its predecessor was still running (hipStreamQuery) -- an answer kept for
    uint32_t query_keep = 0;                              // this many more frames submitted back to back (Enqueue)
    bool idle_seen = false;                               // the last answer was "idle", asked within a run of back-to-back frames
    uint32_t query_every = 8;                             // PM_QUERY_EVERY: ... asked again every this many frames
    int last_slot = -1;  // slot of the most recently submitted frame

    pm::FlattenCache flatten_cache;  // resident paths + scratch of the flatten stage
    bool scene_from_paths = false;   // the resident scene is the flatten kernels' (pm_item_paths maps its items to their paths)

    // the queries (hit testing, the item map, rectangle and polygon queries, snapping, bounds): they read the scene and the scene
    // index, nothing of a frame
    hipEvent_t ev_scene = nullptr;     // end of what the last scene replacement left on `stream` (upload, index): a hit test on another stream starts behind it
    hipEvent_t ev_hit = nullptr;       // end of the hit tests submitted so far; a scene replacement waits for it (SyncAll)
    hipStream_t hit_stream = nullptr;  // the stream it was last recorded on (compared, never dereferenced)
    bool hit_pending = false;          // a hit test was submitted since everything was last waited for
    uint8_t *d_stage = nullptr;        // the host-memory queries' device staging (QueryStaging): every such call ends synchronised, so one serves all
    size_t stage_cap = 0;              // bytes it holds
    // pm_select_polygon's vertices: a ring of slots, each a pinned host buffer, its device copy and the event behind the kernel
    // that last read it.  A call takes the next slot, waits for that event, and copies and launches on its own stream.
    static constexpr int kPolySlots = 4;
    float *h_poly[kPolySlots] = {};
    float *d_poly[kPolySlots] = {};
    hipEvent_t ev_poly[kPolySlots] = {};
    bool poly_used[kPolySlots] = {};
    uint32_t poly_next = 0;

    // wall-clock cost of the last scene replacement, host view (pm_get_scene_timings)
    float t_flatten_ms = 0, t_index_ms = 0, t_arena_ms = 0;
    uint32_t plans_made = 0;

    // tables
    uint32_t *d_lut_srgb2lin = nullptr;
    uint32_t *d_lut_unorm2h = nullptr;
    uint8_t *d_lut_lin2srgb = nullptr;
};

namespace {

struct WallTimer {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    float ms() const { return std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};

uint32_t BandRows(const pm_ctx *c) { return c->row1 - c->row0; }
size_t BandTiles(const pm_ctx *c) { return std::max<size_t>(static_cast<size_t>(BandRows(c)) * c->tiles_x, 1); }

// Entries of ONE sub-queue of the class queues (pm_device.h) for a work list of `entries`: every tile of every entry of a shard may
// land in the same class -- kStripTiles x ceil(entries / kClassShards), and never more than the band has tiles.
size_t QueueSubCap(size_t tiles, size_t entries) {
    return std::min<size_t>(std::max<size_t>(tiles, 1), pm::kStripTiles * ((std::max<size_t>(entries, 1) + pm::kClassShards - 1) / pm::kClassShards));
}
// ... and of all sub-queues together, for the longest work list a viewport of `strip_rows` strip rows can have (every row cut in two)
size_t QueueEntries(size_t tiles, size_t strip_rows) { return std::max<size_t>(pm::kClassCursors * QueueSubCap(tiles, 2 * strip_rows), 4); }

// Waits for everything this context submitted.  A caller-owned stream (pm_render_to) is never
// touched after submission -- the caller may have destroyed it: the slot's event, recorded behind
// the frame at submit time, is waited on instead.
int SyncAll(pm_ctx *c) {
    for (hipStream_t q : c->streams) PM_TRY(hipStreamSynchronize(q));
    for (auto &s : c->slot) {
        if (s.in_flight && s.user_stream) PM_TRY(hipEventSynchronize(s.ev_done));
        s.in_flight = false;
    }
    // (hit tests on a caller's stream read the scene and its index like a frame does)
    if (c->hit_pending) PM_TRY(hipEventSynchronize(c->ev_hit));
    c->hit_pending = false;
    return PM_OK;
}

void FreeSlotViewport(FrameSlot *s) {
    if (s->d_fb) (void)hipFree(s->d_fb);
    if (s->d_queue) (void)hipFree(s->d_queue);  // (the three per-tile tables live behind the queues: one allocation)
    if (s->d_fifo) (void)hipFree(s->d_fifo);
    s->d_fifo = nullptr;
    s->fifo_cap = 0;
    s->d_fb = nullptr;
    s->d_queue = nullptr;
    s->fb_cap = s->tables_cap = s->queue_cap = 0;
    s->d_tile_state = s->d_tile_ptcl = s->d_tile_ncmd = nullptr;
    s->state_epoch = 0;
}

void FreeViewport(pm_ctx *c) {
    for (auto &s : c->slot) {
        FreeSlotViewport(&s);
        s.in_flight = false;
        s.needs_check = false;
    }
    c->last_slot = -1;
}

int AllocSlotViewport(pm_ctx *c, FrameSlot *s) {
    if (s->d_fb && s->vp_epoch == c->vp_epoch) return PM_OK;  // (all five buffers exist, or none: a partial set is released below)
    const size_t tiles = BandTiles(c);
    const size_t tables = std::max<size_t>(tiles, 4);
    const size_t queue_want = QueueEntries(tiles, static_cast<size_t>(BandRows(c)) * c->strips_x);
    const size_t fb_want = std::max<size_t>(c->fb_bytes, 16);
    hipError_t e = hipSuccess;
    if (s->d_fb && s->d_queue && s->fb_cap >= fb_want && s->tables_cap >= tables && s->queue_cap >= queue_want) {
        // the buffers of an earlier (larger or equal) viewport serve this one: nothing is released, nothing allocated -- a one-launch
        // frame's FIFOs excepted, whose capacity is the viewport's (they come back when they are next needed, EnsureFifo)
        if (s->d_fifo) (void)hipFree(s->d_fifo);
        s->d_fifo = nullptr;
        s->fifo_cap = 0;
    } else {
        FreeSlotViewport(s);  // (buffers of an earlier viewport: released now, when the slot is used again, not by the resize)
        // two allocations (each costs 50-300 us): the pixels, and -- behind one another -- the class queues (kClassShards sub-queues
        // per cost class) and the three per-tile tables
        e = hipMalloc(&s->d_fb, fb_want);
        if (e == hipSuccess) e = hipMalloc(&s->d_queue, queue_want * sizeof(uint4) + 3 * tables * sizeof(uint32_t));
        if (e == hipSuccess) {
            s->fb_cap = fb_want;
            s->tables_cap = tables;
            s->queue_cap = queue_want;
        }
    }
    s->vp_epoch = c->vp_epoch;
    if (e == hipSuccess) {
        s->d_tile_state = reinterpret_cast<uint32_t *>(s->d_queue + s->queue_cap);  // (behind the queues as they were allocated)
        s->d_tile_ptcl = s->d_tile_state + tables;
        s->d_tile_ncmd = s->d_tile_ptcl + tables;
    }
    s->state_epoch = 0;  // (never initialised)
    if (e != hipSuccess) {
        if (s->d_fb) (void)hipFree(s->d_fb);
        if (s->d_queue) (void)hipFree(s->d_queue);
        s->d_fb = nullptr;
        s->d_queue = nullptr;
        s->fb_cap = s->tables_cap = s->queue_cap = 0;
        s->d_tile_state = s->d_tile_ptcl = s->d_tile_ncmd = nullptr;
        return HipFail(e, "hipMalloc(frame slot viewport buffers)");
    }
    return PM_OK;
}

int AllocViewport(pm_ctx *c) {
    // (a resize releases and re-allocates frame slot 0's buffers only -- twenty hipFree of a large viewport are 1.5 ms --:
    //  the other slots' go when a frame next uses them, AllocSlotViewport)
    c->vp_epoch += 1;
    for (auto &s : c->slot) {
        s.in_flight = false;
        s.needs_check = false;
        if (s.h_overflow) s.h_overflow[2] = 0;  // (the tile kernel's dense / not dense verdict belongs to the old viewport)
    }
    c->last_slot = -1;
    const uint32_t rows = BandRows(c);
    c->fb_stride = static_cast<size_t>(c->width) * 4;
    c->fb_bytes = c->fb_stride * static_cast<size_t>(rows) * pm::kTileH;
    // (slot 0 now -- pm_framebuffer_device_ptr names its framebuffer before the first frame --, the
    //  others when they are first used: a resize followed by one frame pays for one set of buffers)
    const int r0 = AllocSlotViewport(c, &c->slot[0]);
    if (r0 != PM_OK) return r0;
    c->arena_dirty = true;
    c->plan.reusable = false;  // (another viewport or band: the plan goes with it)
    c->fb_slots.clear();       // (... and what its frames said about its strip rows)
    c->plan.fb_applied = false;
    return PM_OK;
}

// Walks header + bboxes + items (host copy) and checks every offset the kernels
// will dereference.  The kernels trust the scene after this.
int ValidateScene(const uint8_t *meta, size_t meta_len, size_t scene_bytes, uint32_t *n_items_out) {
    if (scene_bytes < 8 || meta_len < 8) return PM_ERR_SCENE;
    uint32_t n, items_ix;
    std::memcpy(&n, meta, 4);
    std::memcpy(&items_ix, meta + 4, 4);
    const uint64_t bbox_end = 8ull + 8ull * n;
    const uint64_t items_end = static_cast<uint64_t>(items_ix) + 32ull * n;
    if (bbox_end > scene_bytes || items_end > scene_bytes || items_ix < bbox_end) return PM_ERR_SCENE;
    if (items_ix & 7u) return PM_ERR_SCENE;  // the encoder keeps everything 8-byte aligned (src/lib.rs:113-130)
    if (items_end > meta_len) return PM_ERR_SCENE;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t *it = meta + items_ix + 32ull * i;
        uint32_t tag, npt, pix;
        std::memcpy(&tag, it, 4);
        tag &= 0xffffu;
        if (tag == pm::kItemFill || tag == pm::kItemPoly) {
            std::memcpy(&npt, it + 12, 4);
            std::memcpy(&pix, it + 16, 4);
            if ((pix & 7u) != 0 || static_cast<uint64_t>(pix) + 8ull * npt > scene_bytes) return PM_ERR_SCENE;
        }
    }
    *n_items_out = n;
    return PM_OK;
}

// Class thresholds in stream elements, descending: three classes of long lists (a workgroup per
// tile: > vheavy, > midway, > heavy), five of short ones.
void SetClassThresholds(const pm_ctx *c, pm::FrameParams *p, uint32_t heavy) {
    const uint32_t h = heavy, v = std::max(c->vheavy_stream, h);
    const uint32_t thr[pm::kClasses - 1] = {v, (v + h) / 2, h, h * 3 / 4, h / 2, h * 5 / 16, h * 5 / 32};
    for (uint32_t k = 0; k < pm::kClasses - 1; ++k) p->class_thr[k] = thr[k];
}

// A slot's binning arena and command-list arena, allocated (or grown to what EnsureArena asked for)
// when the slot is about to be used.
int EnsureSlotBuffers(pm_ctx *c, FrameSlot *s) {
    const int rv = AllocSlotViewport(c, s);
    if (rv != PM_OK) return rv;
    if (!s->d_arena || s->arena_cap < c->arena_cap) {
        if (s->d_arena) (void)hipFree(s->d_arena);  // (hipFree waits for the device: nothing is using it any more)
        s->d_arena = nullptr;
        s->arena_cap = 0;
        PM_TRY(hipMalloc(&s->d_arena, static_cast<size_t>(std::max<uint32_t>(c->arena_cap, pm::kArenaBase)) * sizeof(uint32_t)));
        s->arena_cap = c->arena_cap;
    }
    if (c->plan.use_row_lists && (!s->d_row_bbox || s->row_cap < c->plan.row_want)) {
        // per-tile-row item lists of this slot's frames (pm_rowcull_kernel writes them): boxes, then indices, ONE allocation
        if (s->d_row_bbox) (void)hipFree(s->d_row_bbox);
        s->d_row_bbox = nullptr;
        s->d_row_item = nullptr;
        s->row_cap = 0;
        const uint64_t cap = c->plan.row_want + c->plan.row_want / 4;
        PM_TRY(hipMalloc(&s->d_row_bbox, cap * (sizeof(uint2) + sizeof(uint32_t))));
        s->d_row_item = reinterpret_cast<uint32_t *>(s->d_row_bbox + cap);
        s->row_cap = cap;
    }
    PM_TRY(s->ptcl.Reserve(c->ptcl_want, std::max<uint64_t>(c->ptcl_want, 64)));
    return PM_OK;
}

// A list of the plan on its way to the device: asynchronous, on the context's stream, read from the plan's own vector.
template <typename T>
hipError_t UploadList(pm_ctx *c, T *dst, const std::vector<T> &src) {
    if (src.empty()) return hipSuccess;
    return hipMemcpyAsync(dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, c->stream);
}

// The binning plan of the resident scene, viewport and band (pm_plan.h), made when something it depends on changed, and its lists
// on the device: the reuse check, the planner, a wait for the frames in flight, the device lists grown and filled, one stream wait.
int EnsureArena(pm_ctx *c) {
    if (!c->arena_dirty && c->arena_cap != 0) return PM_OK;
    if (c->item_meta.empty() || c->tiles_x == 0) return PM_OK;  // nothing to size against yet
    const WallTimer timer;
    pm::BinPlan &plan = c->plan;
    pm::PlanInput in;
    in.item_meta = c->item_meta.data();
    in.n_items = c->n_items;
    in.n_chunks = c->n_chunks;
    in.tiles_x = c->tiles_x;
    in.strips_x = c->strips_x;
    in.row0 = c->row0;
    in.row1 = c->row1;
    in.n_cus = c->n_cus;
    in.margin = c->replan_wide ? static_cast<int>(pm::kTileW) : 0;
    in.bin_split_mode = c->bin_split_mode;
    in.bin_split_cands = c->bin_split_cands;
    in.bin_split_slots = c->bin_split_slots;
    in.bin_split_fill = c->bin_split_fill;
    in.bin_wg_per_cu = c->bin_wg_per_cu;
    in.bin_waves_env = c->bin_waves_env;
    in.bin_waves_inflight = c->bin_waves_inflight;
    in.one_launch_mode = c->one_launch_mode;
    in.frame_wg_per_cu = c->frame_wg_per_cu;
    in.fold_clear_mode = c->fold_clear_mode;
    in.fb_slots = c->fb_slots.data();
    in.n_fb_slots = c->fb_slots.size();
    in.arena_cap = c->arena_cap;
    in.ptcl_want = c->ptcl_want;
    if (pm::PlanStillHolds(in, plan)) {
        // (the scene index of the new scene is still being built on the context's stream; frames run on the others)
        PM_TRY(hipStreamSynchronize(c->stream));
        c->arena_dirty = false;
        c->t_arena_ms = timer.ms();
        return PM_OK;
    }
    // (host work first: the scene-index kernel of a scene replacement is still running on the device)
    in.row_list_min_items = EnvInt("PM_ROW_LIST_MIN_ITEMS", 2048, 0, 1 << 30);
    in.row_list_part_items = EnvInt("PM_ROW_LIST_PART_ITEMS", 0, 1, 1 << 30);  // (the tests cut small scenes into many parts)
    if (const char *v = std::getenv("PM_PTCL_INITIAL_CMDS"))  // tests: force the overflow -> grow -> re-render path
        in.ptcl_initial_cmds = std::max<uint64_t>(64, std::strtoull(v, nullptr, 10));
    if (pm::MakeBinPlan(in, &plan) != PM_OK) {
        SetError("scene x viewport needs a binning arena beyond 16 GiB");
        plan = pm::BinPlan();  // (nothing of the failed plan stays: arena_dirty still stands, the next plan is made from scratch)
        return PM_ERR_CAPACITY;
    }
    // (the slots' arenas and per-tile-row list buffers themselves are allocated when a slot is next used, EnsureSlotBuffers: the
    //  first frame of a scene pays for one slot's, not for four -- hundreds of MB each at 8K)
    c->arena_cap = plan.arena_alloc;
    c->ptcl_want = plan.ptcl_want;
    PM_TRY(SyncAll(c) == PM_OK ? hipSuccess : hipErrorUnknown);  // frames in flight still read the lists replaced below
    const size_t n = plan.desc.size();  // (grow only: an animation re-sizes every frame)
    PM_TRY(c->sr_desc.Reserve(n));
    PM_TRY(c->sr_list.Reserve(n));
    PM_TRY(c->sr_slots.Reserve(n));
    PM_TRY(c->sr_desc_whole.Reserve(n));
    if (c->one_launch_mode != 0) PM_TRY(c->sr_next_one.Reserve(n));  // (only a context that renders one-launch frames pays for the table)
    PM_TRY(c->band_bbox.Reserve(plan.band_item.size()));
    PM_TRY(c->band_item.Reserve(plan.band_item.size()));
    PM_TRY(hipMemsetAsync(c->sr_slots.p, 0, n * sizeof(uint32_t), c->stream));
    PM_TRY(UploadList(c, c->sr_desc.p, plan.desc));
    if (!plan.band_identity) {
        PM_TRY(UploadList(c, c->band_bbox.p, plan.band_bbox));
        PM_TRY(UploadList(c, c->band_item.p, plan.band_item));
    }
    // The rest of the plan, made while the uploads above are under way.  (Its failure is out of reach through this call -- per-row
    // lists that long come with an arena beyond its limit, four dwords per entry at least -- and handled all the same: the uploads
    // above read the plan's vectors, so they are waited for before the plan goes.)
    if (pm::MakeSideLists(in, &plan) != PM_OK) {
        SetError("per-row item lists beyond 2^32 entries");
        (void)hipStreamSynchronize(c->stream);
        plan = pm::BinPlan();
        return PM_ERR_CAPACITY;
    }
    PM_TRY(UploadList(c, c->sr_desc_whole.p, plan.desc_whole));
    if (c->one_launch_mode != 0) PM_TRY(UploadList(c, c->sr_next_one.p, plan.next_one));
    PM_TRY(c->idle_sr.Reserve(plan.idle.size()));
    PM_TRY(UploadList(c, c->idle_sr.p, plan.idle));
    if (plan.use_row_lists) {
        PM_TRY(c->row_base.Reserve(plan.row_base.size(), plan.row_base.size() + 64));
        PM_TRY(UploadList(c, c->row_base.p, plan.row_base));
        PM_TRY(UploadList(c, c->sr_list.p, plan.sr_list));
    }
    PM_TRY(hipStreamSynchronize(c->stream));  // ONE wait: the lists are in place before a frame on any stream reads them
    c->frames_on_plan = 0;
    c->arena_epoch += 1;  // (a slot's tile_state is reset to "background" on the frame's own stream when the slot is next used)
    c->plans_made += 1;
    c->arena_dirty = false;
    c->t_arena_ms = timer.ms();
    return PM_OK;
}

uint32_t FineGrid(const pm_ctx *c);

int BuildParams(pm_ctx *c, FrameSlot *s, uint8_t *fb, size_t stride, pm::FrameParams *p) {
    if (!c->d_scene || c->scene_bytes < 8) {
        SetError("no scene resident (pm_upload_scene / pm_flatten_and_encode first)");
        return PM_ERR_INVALID;
    }
    if (c->tiles_x == 0 || BandRows(c) == 0) {
        SetError("no viewport (pm_resize first)");
        return PM_ERR_INVALID;
    }
    const WallTimer tm;
    int r = EnsureArena(c);
    if (r != PM_OK) return r;
    const float t_plan = tm.ms();
    r = EnsureSlotBuffers(c, s);  // (the slot's buffers come into being when it is first used)
    if (r != PM_OK) return r;
    if (tm.ms() > 0.05f && std::getenv("PM_HOST_TIMING")) std::fprintf(stderr, "BuildParams: plan %.3f slot buffers %.3f ms (arena %u dwords, tile arena %llu quads)\n", t_plan, tm.ms() - t_plan, c->arena_cap, static_cast<unsigned long long>(c->ptcl_want));
    if (!fb) fb = s->d_fb;
    std::memset(p, 0, sizeof(*p));
    p->scene = c->d_scene;
    p->scene_bytes = static_cast<uint32_t>(c->scene_bytes);
    p->n_items = c->n_items;
    p->items_ix = c->dev_items_ix;
    p->bbox_ix = c->dev_bbox_ix;
    p->width = c->width;
    p->height = c->height;
    p->tiles_x = c->tiles_x;
    p->tiles_y = c->tiles_y;
    p->row0 = c->row0;
    p->row1 = c->row1;
    p->strips_x = c->strips_x;
    p->fb = fb;
    p->fb_stride = static_cast<uint32_t>(stride);
    p->fb_vec16 = ((reinterpret_cast<uintptr_t>(fb) & 15u) == 0 && (stride & 15u) == 0) ? 1u : 0u;
    p->fb_bgra = c->target_fmt == PM_FMT_BGRA8 ? 1u : 0u;
    p->arena = s->d_arena;
    p->arena_cap = s->arena_cap;
    p->sr_desc = c->sr_desc.p;
    p->sr_list = c->sr_list.p;
    p->n_sr_active = c->plan.n_sr_active();
    p->sr_slots = c->sr_slots.p;
    p->bin_prio_slots = c->bin_prio_slots;
    p->bin_grid = c->plan.bin_grid;
    p->sr_empty_dwords = c->plan.sr_empty_dwords;
    p->queue = s->d_queue;
    // (the plan's longer work list: the one with the cuts -- the list without them, which frames behind running frames bin from, has fewer entries)
    p->queue_sub_cap = static_cast<uint32_t>(QueueSubCap(BandTiles(c), std::max(c->plan.n_sr_active(), c->plan.n_sr_whole())));
    if (static_cast<size_t>(pm::kClassCursors) * p->queue_sub_cap > s->queue_cap) {  // (cannot happen: a work list has two entries per strip row at most)
        SetError("the work list is longer than the slot's tile queues were sized for");
        return PM_ERR_CAPACITY;
    }
    p->tile_state = s->d_tile_state;
    p->tarena = s->ptcl.p;
    p->tarena_cap = static_cast<uint32_t>(s->ptcl.cap);
    p->tile_ptcl = s->d_tile_ptcl;
    p->tile_ncmd = s->d_tile_ncmd;
    p->ctr_cur = s->d_ctr + s->parity;
    p->ctr_next = s->d_ctr + (s->parity ^ 1u);
    p->host_overflow = s->d_overflow;
    p->host_fail = s->d_overflow + 1;
    p->host_dense = s->d_overflow + 2;
    p->fine_dense = 0;
    p->fifo = s->d_fifo;
    p->fifo_cap = s->fifo_cap;
    p->one_launch = 0;
    p->sr_next_one = c->sr_next_one.p;
    p->one_grid_rows = c->plan.one_grid_rows;
    p->idle_sr = c->idle_sr.p;
    p->n_idle_sr = static_cast<uint32_t>(c->plan.idle.size());
    p->spin_ticks = c->frame_spin_ticks;
    // (the whole item list in scene order: the scene's own boxes, no list of indices)
    p->band_bbox = c->plan.band_identity ? reinterpret_cast<const uint2 *>(c->d_scene + c->dev_bbox_ix) : c->band_bbox.p;
    p->band_item = c->plan.band_identity ? nullptr : c->band_item.p;
    p->n_band_items = static_cast<uint32_t>(c->plan.band_item.size());
    p->bin_waves = c->plan.bin_waves;
    // (PM_FOLD_CLEAR=3: a frame whose strip rows are chained -- config 5: lone frame 0.482 -> 0.456 ms -- and, Enqueue, any frame behind
    //  running frames: 4K Tiger sustained +1.5 %.  A small frame alone keeps the fold into the tile kernel's launch: with the
    //  clearing its binning kernel ends a microsecond later, and that is on the frame's critical path.  PM_FOLD_CLEAR=4: always.)
    p->clear_in_bin = c->fold_clear_mode == 4 || (c->fold_clear_mode == 3 && c->plan.n_sr_active() > c->plan.bin_grid) ? 1u : 0u;
    p->bin_wt = c->bin_wt_mode == 1 || (c->bin_wt_mode == 2 && c->plan.n_sr_active() <= c->plan.bin_grid) ? 1u : 0u;
    p->split_mode = c->split_mode;
    p->dense_factor = c->dense_factor;
    p->verdict_waves = static_cast<uint32_t>(c->n_cus) * c->fine_wg_per_cu * 4u;
    {
        SetClassThresholds(c, p, c->heavy_stream_lone);
        p->n_heavy_classes = 3;
        p->handout_static = c->handout == 1 ? 1u : 0u;  // (Enqueue decides per frame when PM_HANDOUT is 0)
    }
    p->fine_grid = FineGrid(c);
    p->use_row_lists = c->plan.use_row_lists ? 1u : 0u;
    p->row_base = c->row_base.p;
    p->row_parts = c->plan.row_parts;
    p->row_part_items = c->plan.row_part_items;
    p->row_bbox = s->d_row_bbox;
    p->row_item = s->d_row_item;
    p->chunk_base = c->d_chunk_base;
    p->chunk_bbox = c->d_chunk_bbox;
    p->sup_bbox = c->d_sup_bbox;
    p->lut_srgb2lin = c->d_lut_srgb2lin;
    p->lut_unorm2h = c->d_lut_unorm2h;
    p->lut_lin2srgb = c->d_lut_lin2srgb;
    return PM_OK;
}

// Persistent grids: workgroups of 4 waves, one wave per tile (or per part of a tile).
// (per CU: 6 workgroups for pm_coarse_kernel, 4 for pm_fine_kernel by default -- with four frames in
//  flight anything from 2 to 8 measures within 2 %)

uint32_t CoarseGrid(const pm_ctx *c) {
    const uint32_t tiles = static_cast<uint32_t>(BandTiles(c));
    return std::max(1u, std::min((tiles + 3u) / 4u, static_cast<uint32_t>(c->n_cus) * c->coarse_wg_per_cu));
}

uint32_t FineGrid(const pm_ctx *c) {
    const uint32_t tiles = static_cast<uint32_t>(BandTiles(c));
    return std::max(1u, std::min(tiles, static_cast<uint32_t>(c->n_cus) * c->fine_wg_per_cu));
}

// Strip rows no item reaches get no workgroup: their tiles are background for as long as this scene
// and viewport last -- set once per slot and arena epoch, in stream order before the frame.
hipError_t ResetTileState(pm_ctx *c, FrameSlot *s, hipStream_t q) {
    if (s->state_epoch == c->arena_epoch) return hipSuccess;
    const hipError_t e = hipMemsetAsync(s->d_tile_state, 0xff, BandTiles(c) * sizeof(uint32_t), q);
    if (e == hipSuccess) s->state_epoch = c->arena_epoch;
    return e;
}

void Submitted(pm_ctx *c, int si, const pm::FrameParams &p, hipStream_t frame_stream) {
    FrameSlot *s = &c->slot[si];
    s->in_flight = true;
    s->needs_check = true;
    s->user_stream = false;
    s->params = p;
    s->frame_stream = frame_stream;
    s->parity ^= 1u;
    c->last_slot = si;
    c->frame += 1;
}

// The tile kernel's instantiation for this frame: the one-wave-per-tile one when the latest frame of this scene and viewport that said
// anything called itself dense (its pinned word; read without waiting -- a verdict a frame or two old is as good).
void ChooseTileKernel(pm_ctx *c, pm::FrameParams *p) {
    if (!c->dense_kernel_mode || !c->fused || c->last_slot < 0) return;
    uint32_t verdict = 0;
    for (size_t k = 0; k < c->slot.size() && verdict == 0; ++k) {  // newest first
        const FrameSlot &t = c->slot[(static_cast<size_t>(c->last_slot) + c->slot.size() - k) % c->slot.size()];
        if (t.h_overflow) verdict = static_cast<volatile uint32_t *>(t.h_overflow)[2];
    }
    if (verdict != 2u) return;
    p->fine_dense = 1u;
    c->frames_dense_kernel += 1;
    const uint32_t per_cu = p->handout_static ? c->fine_wg_dense_inflight : c->fine_wg_dense;
    p->fine_grid = std::max(1u, std::min(static_cast<uint32_t>(BandTiles(c)), static_cast<uint32_t>(c->n_cus) * per_cu));
}

// Workgroups of a one-launch frame (0: this frame takes two launches).  Every strip row some item reaches needs its own
// workgroup, all resident at once; beyond those, as many as there could be tiles to take from the FIFOs.
uint32_t OneLaunchGrid(const pm_ctx *c) {
    if (c->one_launch_mode == 0 || c->frame_wg_per_cu == 0 || !c->fused || c->plan.use_row_lists || c->plan.bin_waves != 4) return 0u;
    const uint32_t resident = static_cast<uint32_t>(c->n_cus) * c->frame_wg_per_cu;
    if (c->plan.one_grid_rows == 0u) return 0u;  // (more than two strip rows per resident workgroup: EnsureArena)
    const uint64_t tiles = BandTiles(c);
    if (tiles > 0xffffffu) return 0u;
    return std::max(c->plan.one_grid_rows, std::min(resident, static_cast<uint32_t>((tiles + 3u) / 4u)));
}

// The slot's FIFO entries (zeroed once: whoever takes an entry leaves a zero behind).
// (zeroed on the stream the frame is about to run on: the context's streams do not wait for the null stream)
int EnsureFifo(pm_ctx *c, FrameSlot *s, hipStream_t q) {
    const uint32_t cap = static_cast<uint32_t>(BandTiles(c));
    if (s->d_fifo && s->fifo_cap >= cap) return PM_OK;
    if (s->d_fifo) (void)hipFree(s->d_fifo);
    s->d_fifo = nullptr;
    s->fifo_cap = 0;
    const size_t bytes = static_cast<size_t>(pm::kFifos) * cap * sizeof(uint4);
    PM_TRY(hipMalloc(&s->d_fifo, bytes));
    PM_TRY(hipMemsetAsync(s->d_fifo, 0, bytes, q));
    s->fifo_cap = cap;
    return PM_OK;
}

// The third frame of a plan: what the first frames' binning kernels found per strip row (segment slots) comes back, once, and the plan
// is made again with the heaviest strip rows cut in two (EnsureArena, bin_split_mode).  A wait for the frames in flight and a copy
// of a few kilobytes: about 0.1 ms, once per scene and viewport.
int FeedBackStripRows(pm_ctx *c) {
    if (c->arena_dirty || c->arena_cap == 0) return PM_OK;  // (a new plan is about to be made anyway)
    if (c->frames_on_plan == 0xffffffffu) return PM_OK;
    c->frames_on_plan += 1;
    if (c->frames_on_plan != 3u || c->bin_split_mode != 1 || c->one_launch_mode != 0 || c->plan.fb_applied || !c->sr_slots.p) return PM_OK;
    // (only where cutting can happen at all: the plan's rows leave workgroups of the resident grid free, and the band bins from the
    //  one work list -- per-tile-row item lists are addressed by its entries, EnsureArena cuts nothing)
    if (c->plan.use_row_lists) return PM_OK;
    if (c->plan.n_sr_active() >= pm::ResidentBinWorkgroups(c->n_cus, c->bin_wg_per_cu, 1u)) return PM_OK;
    int r = SyncAll(c);
    if (r != PM_OK) return r;
    std::vector<uint32_t> &sl = c->stage_slots;
    sl.resize(c->plan.n_sr_active());
    PM_TRY(hipMemcpy(sl.data(), c->sr_slots.p, sl.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
    const size_t n_rows = static_cast<size_t>(BandRows(c)) * c->strips_x;
    c->fb_slots.assign(n_rows, 0u);
    uint32_t heaviest = 0;
    for (size_t k = 0; k < sl.size() && k < c->plan.desc.size(); ++k) {
        const uint32_t x = c->plan.desc[k].x;
        const size_t i = static_cast<size_t>(x >> 16) * c->strips_x + (x & 0xffu);
        if (i < n_rows) c->fb_slots[i] += sl[k];  // (a row already cut: its halves' slots)
        if (i < n_rows) heaviest = std::max(heaviest, c->fb_slots[i]);
    }
    if (heaviest < c->bin_split_slots && c->plan.n_sr_split == 0) {  // nothing to cut, nothing cut: the plan stands
        c->plan.fb_applied = true;
        return PM_OK;
    }
    c->arena_dirty = true;
    c->plan.reusable = false;
    c->plans_fed_back += 1;
    return PM_OK;
}

// One frame: its kernels back to back on one in-order stream -- the context's stream
// frame % n, or the caller's.  tev (timing passes): eight events {begin, end} x {bin, clear,
// coarse, fine} carried by the dispatches themselves, so that a timed frame puts exactly the
// same packets on the queue as an untimed one.
// (developer: PM_HOST_TIMING=2 prints, when the context goes, where pm_render's host time went -- mean microseconds per section)
struct SubmitProfile {
    bool on = std::getenv("PM_HOST_TIMING") && std::atoi(std::getenv("PM_HOST_TIMING")) >= 2;
    double acc[6] = {0, 0, 0, 0, 0, 0};
    uint64_t n = 0;
    std::chrono::steady_clock::time_point t;
    void start() { if (on) t = std::chrono::steady_clock::now(); }
    void mark(int k) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        acc[k] += std::chrono::duration<double, std::micro>(now - t).count();
        t = now;
    }
    ~SubmitProfile() {
        if (on && n) std::fprintf(stderr, "pm_render host time per frame over %llu frames (us): params %.2f | slot/stream order %.2f | in-flight query %.2f | policy %.2f | binning launch %.2f | tile launch + bookkeeping %.2f\n",
                                  static_cast<unsigned long long>(n), acc[0] / n, acc[1] / n, acc[2] / n, acc[3] / n, acc[4] / n, acc[5] / n);
    }
};
SubmitProfile g_submit_profile;

int Enqueue(pm_ctx *c, uint8_t *fb, size_t stride, hipStream_t user_stream, hipEvent_t *tev = nullptr) {
    g_submit_profile.start();
    const int si = static_cast<int>(c->frame % c->slot.size());
    FrameSlot *s = &c->slot[si];
    if (c->tiles_x != 0) {  // (a slot's viewport buffers come into being when the slot is first used)
        const int ra = AllocSlotViewport(c, s);
        if (ra != PM_OK) return ra;
    }
    if (!fb) fb = s->d_fb;
    pm::FrameParams p;
    hipStream_t q = user_stream ? user_stream : c->streams[c->frame % c->streams.size()];
    int r = FeedBackStripRows(c);
    if (r != PM_OK) return r;
    r = BuildParams(c, s, fb, stride, &p);
    if (r != PM_OK) return r;
    g_submit_profile.mark(0);
    hipEvent_t none[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t *t = tev ? tev : none;
    // the slot's previous frame (same stream unless the caller's streams are involved or the
    // slot count differs from the stream count: then the event orders the reuse)
    // (no event is recorded per frame: one recorded on the other stream when the need arises
    //  marks the end of everything submitted there so far, the slot's frame included)
    if (s->in_flight && s->frame_stream != q) {
        if (!s->user_stream) PM_TRY(hipEventRecord(s->ev_done, s->frame_stream));
        PM_TRY(hipStreamWaitEvent(q, s->ev_done, 0));
    }
    // frames that target the same caller-owned buffer must not overlap each other
    if (c->last_slot >= 0 && c->last_slot != si) {
        FrameSlot &l = c->slot[c->last_slot];
        if (l.in_flight && l.params.fb == fb && l.frame_stream != q) {
            if (!l.user_stream) PM_TRY(hipEventRecord(l.ev_done, l.frame_stream));
            PM_TRY(hipStreamWaitEvent(q, l.ev_done, 0));
        }
    }
    // Tile hand-out: drawn when this frame will have the device to itself, static when the previous
    // frame is still running (the frames then overlap, and neighbours fill what a static hand-out
    // leaves idle): lone frame -4.6 us, sustained throughput as before.  PM_HANDOUT=1 / 2 pins it.
    g_submit_profile.mark(1);
    p.handout_static = c->handout == 1 ? 1u : 0u;
    if (c->handout == 0 && c->last_slot >= 0) {
        const FrameSlot &l = c->slot[c->last_slot];
        if (l.in_flight) {
            // The question "is the previous frame still running?" costs 3.3 us of host time (hipStreamQuery, measured: a quarter of a
            // pm_render call, and small frames in flight are bound by exactly that).  Frames submitted back to back get the same
            // answer most of the time: it is asked once in eight such frames and kept in between (a gap of 0.2 ms asks again).
            const auto now = std::chrono::steady_clock::now();
            const bool back_to_back = std::chrono::duration<double, std::micro>(now - c->last_submit).count() < 200.0;
            c->last_submit = now;
            if (back_to_back && c->query_keep != 0u) {
                c->query_keep -= 1u;
            } else {
                const hipError_t st = l.user_stream ? hipEventQuery(l.ev_done) : hipStreamQuery(l.frame_stream);
                const bool was_running = c->prev_running;
                c->prev_running = st == hipErrorNotReady;
                // (kept for the rest of the eight -- except the FIRST "idle" behind "running" or behind a pause, kept for one frame: the first
                //  frames of a burst find the device idle, and a burst planned as lone frames for eight frames on the strength of that was
                //  measured 14 % slower; a loop of lone frames -- idle, idle, idle -- asks once in eight as before: asking every other
                //  frame cost the 4K Tiger's lone frame 0.5 us)
                c->query_keep = (c->prev_running || (!was_running && back_to_back && c->idle_seen)) ? c->query_every - 1u : min(1u, c->query_every - 1u);
                c->idle_seen = !c->prev_running && back_to_back;
                (void)hipGetLastError();  // (hipErrorNotReady is an answer, not a failure)
            }
            p.handout_static = c->prev_running && l.frame_stream != q ? 1u : 0u;  // (behind it on the same stream: alone all the same)
        } else {
            c->query_keep = 0u;
        }
    }
    g_submit_profile.mark(2);
    // overlapping frames also keep fewer tiles for whole workgroups (a workgroup tile idles three
    // waves while its list is built: cheap when the frame is alone and its longest lists set the
    // span, wasteful when neighbours could use the SIMDs): lone frame -1.4 us, sustained +2.6 %
    if (p.handout_static) SetClassThresholds(c, &p, c->heavy_stream);
    // ... and bin with a wave per strip row: behind other frames what counts is instructions issued, not this frame's
    // latency (a wave per row: a quarter fewer of them; 4K Tiger sustained 255 -> 266 k Mpix/s).  Only frames with enough
    // strip rows to fill the chip that way (at 1080p, 544 rows, a row's 50 us then set the pace: 142 -> 96 k), and only where
    // no workgroup walks a chain of rows -- the chains are linked for one grid (EnsureArena).
    // ... and only LIGHT rows: a wave's record holds 64 candidates, and a strip row with more of them pays a second pass over
    // everything (held-out workload 2, 2 k blobs at 2048^2, 79 candidates per row: sustained 164 -> 139 us per frame with
    // workgroups; the rule is the one that picks a wave per row for a frame alone, EnsureArena).
    // (round 5, found by the held-out policy check: held-out 3 -- 2 025 light strip rows, more than the 1 280 workgroups of the plan's
    //  grid, so its rows are chained -- ran 14 % faster in flight with a wave per row.  Sixteen one-wave groups per CU hold 4 096 rows at
    //  once: such a frame gets a wave for EVERY row and does not walk the chains.)
    // ... from the work list WITHOUT the cuts (a cut strip row is two rows' worth of fixed work: worth it on a lone frame's critical
    // path, a loss where frames overlap): the same arena regions, every cut row whole again
    uint32_t n_rows_frame = c->plan.n_sr_active();
    if (p.handout_static && c->plan.n_sr_split != 0 && c->plan.n_sr_whole() != 0) {
        p.sr_desc = c->sr_desc_whole.p;
        p.n_sr_active = c->plan.n_sr_whole();
        p.bin_grid = std::min(p.bin_grid, c->plan.n_sr_whole());
        p.sr_slots = nullptr;  // (the report is by entry of the list with the cuts)
        n_rows_frame = c->plan.n_sr_whole();
    }
    if (p.handout_static && c->bin_waves_inflight == 1 && c->plan.bin_waves == 4 && n_rows_frame >= 4u * static_cast<uint32_t>(c->n_cus) &&
        c->plan.cands <= 32ull * n_rows_frame) {
        if (n_rows_frame <= p.bin_grid) {
            p.bin_waves = 1;
            c->frames_bin_wave_inflight += 1;
        } else if (n_rows_frame <= 16u * static_cast<uint32_t>(c->n_cus) && c->bin_wg_per_cu == 0xffu) {
            p.bin_waves = 1;
            p.bin_grid = n_rows_frame;
            p.bin_no_chains = 1u;
            c->frames_bin_wave_inflight += 1;
            c->frames_bin_no_chains += 1;
        }
    }
    if (p.bin_waves == 1) c->frames_bin_wave += 1;
    // ... and a smaller persistent grid: three tile workgroups per CU leave two slots (LDS, VGPRs) to
    // the neighbours' binning workgroups (Tiger 4K sustained 221 -> 227 k Mpix/s, the other configurations
    // unchanged; two cost config 4 2 %; alone, five end the frame 0.8 us earlier)
    if (p.handout_static && c->fine_wg_per_cu_inflight < c->fine_wg_per_cu)
        p.fine_grid = std::max(1u, std::min(p.fine_grid, static_cast<uint32_t>(c->n_cus) * c->fine_wg_per_cu_inflight));
    // (the waves a frame's dense / not dense verdict is judged against: the GENERAL kernel's grid for this kind of frame, whichever
    //  instantiation runs it -- round-5 advisor: judged against its own, larger grid the one-wave kernel called a scene "not dense"
    //  that the general kernel called dense, and such a scene changed kernels every other frame)
    p.verdict_waves = p.fine_grid * 4u;
    ChooseTileKernel(c, &p);
    const uint32_t n_striprows = BandRows(c) * c->strips_x;
    PM_TRY(ResetTileState(c, s, q));
    // One launch for the whole frame (pm_frame.hip) when the frame has the device to itself -- two such launches at once could
    // each hold the slots the other's binning workgroups wait for -- and every strip row gets its own resident workgroup.
    const uint32_t frame_grid = OneLaunchGrid(c);
    if (frame_grid != 0u && !tev && !p.handout_static && !c->one_launch_broken) {
        r = EnsureFifo(c, s, q);
        if (r != PM_OK) return r;
        p.fifo = s->d_fifo;
        p.fifo_cap = s->fifo_cap;
        if (c->cap_counts) {
            p.dbg_counts = c->cap_counts;
            p.dbg_solid = c->cap_solid;
            p.dbg_cmds = c->cap_cmds;
            p.dbg_max = c->cap_max;
        }
#ifdef PM_EMU
        const bool split = true;  // (the CPU emulation runs workgroups one after the other: the binning roles first, then everybody takes from the FIFOs)
#else
        const bool split = c->one_launch_split;
#endif
        if (split) {
            p.one_launch = 1u;
            pm::LaunchFrame(p, frame_grid, q);
            p.one_launch = 2u;
            pm::LaunchFrame(p, frame_grid, q);
        } else {
            p.one_launch = 3u;
            pm::LaunchFrame(p, frame_grid, q);
        }
        PM_TRY(hipGetLastError());
        c->frames_one_launch += 1;
        Submitted(c, si, p, q);
        s->user_stream = user_stream != nullptr && std::find(c->streams.begin(), c->streams.end(), q) == c->streams.end();
        if (s->user_stream) PM_TRY(hipEventRecord(s->ev_done, q));
        return PM_OK;
    }
    // The resolved tiles' pixels (26 MB of stores at Tiger 4K): extra workgroups of the tile kernel's
    // launch for a frame alone (one launch less: -7 us), a launch of its own between the two kernels
    // when other frames are in flight -- there it fills the SIMDs binning's tail leaves idle instead of
    // queueing behind the persistent tile workgroups (sustained +3 %).
    // (Small frames keep the fold: at 1080p a pipelined frame is 17 us, about what submitting two launches
    //  costs the host, and a third one took the sustained rate from 122 k to 100 k Mpix/s.)
    // (round 6, PM_FOLD_CLEAR=3, the default: neither -- the binning launch writes them, every strip row's workgroup its own at the
    //  row's end and extra workgroups those of the strip rows no item reaches: stores under a kernel of dependent chains, and the
    //  tile kernel's first tiles no longer share the chip with 2 025 clearing workgroups)
    if (c->fold_clear_mode == 3 && p.handout_static) p.clear_in_bin = 1u;
    const bool fold = p.clear_in_bin == 0u && (c->fold_clear_mode == 1 || (c->fold_clear_mode >= 2 && (!p.handout_static || BandTiles(c) < 16384u)));
    g_submit_profile.mark(3);
    pm::LaunchBin(p, q, t[0], t[1]);
    g_submit_profile.mark(4);
    if (!fold && p.clear_in_bin == 0u) pm::LaunchClear(p, n_striprows, q, t[2], t[3]);  // (needs tile_state)
    if (!c->fused) pm::LaunchCoarse(p, CoarseGrid(c), false, q, t[4], t[5]);
    pm::LaunchFine(p, fold ? n_striprows : 0u, c->fused, q, t[6], t[7]);
    PM_TRY(hipGetLastError());
    Submitted(c, si, p, q);
    s->user_stream = user_stream != nullptr && std::find(c->streams.begin(), c->streams.end(), q) == c->streams.end();
    if (s->user_stream) PM_TRY(hipEventRecord(s->ev_done, q));  // the only handle kept on a caller's stream
    g_submit_profile.mark(5);
    g_submit_profile.n += 1;
    return PM_OK;
}

// Scene index: chunk table offsets on the host (a prefix sum over the item headers we
// already copied), chunk boxes on the device.  Built once per scene, like the
// reference builds its per-item ShortBbox array at encode time (src/lib.rs:88-97).
int BuildSceneIndex(pm_ctx *c) {
    const uint8_t *meta = c->item_meta.data();
    uint32_t n, items_ix;
    std::memcpy(&n, meta, 4);
    std::memcpy(&items_ix, meta + 4, 4);
    std::vector<uint32_t> &base = c->chunk_base_host;  // (the source of an asynchronous copy: it lives in the context)
    base.resize(static_cast<size_t>(n) + 1);
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        base[i] = static_cast<uint32_t>(total);
        const uint8_t *it = meta + items_ix + 32ull * i;
        uint32_t tag, npt;
        std::memcpy(&tag, it, 4);
        std::memcpy(&npt, it + 12, 4);
        tag &= 0xffffu;
        uint64_t nseg = 0;
        if (tag == pm::kItemFill) nseg = npt;
        else if (tag == pm::kItemPoly && npt >= 2) nseg = npt - 1;
        total += (nseg + pm::kChunkSegs - 1) / pm::kChunkSegs;
    }
    base[n] = static_cast<uint32_t>(total);
    if (total > 0xffffffull) {  // (a chunk's index inside its item travels in 24 bits, pm_bin_kernel's survivor lists)
        SetError("scene has too many segments for the chunk index (2^24 chunks of 4 segments)");
        return PM_ERR_CAPACITY;
    }
    if (base.size() > c->chunk_base_cap) {
        if (c->d_chunk_base) (void)hipFree(c->d_chunk_base);
        c->d_chunk_base = nullptr;
        PM_TRY(hipMalloc(&c->d_chunk_base, base.size() * sizeof(uint32_t)));
        c->chunk_base_cap = base.size();
    }
    if (total > c->chunk_bbox_cap || !c->d_chunk_bbox) {
        if (c->d_chunk_bbox) (void)hipFree(c->d_chunk_bbox);
        c->d_chunk_bbox = nullptr;
        PM_TRY(hipMalloc(&c->d_chunk_bbox, std::max<uint64_t>(total, 1) * sizeof(float4)));
        c->chunk_bbox_cap = std::max<uint64_t>(total, 1);
    }
    const uint64_t n_sup = (total + pm::kSuperChunks - 1) / pm::kSuperChunks;
    if (n_sup > c->sup_bbox_cap || !c->d_sup_bbox) {
        if (c->d_sup_bbox) (void)hipFree(c->d_sup_bbox);
        c->d_sup_bbox = nullptr;
        PM_TRY(hipMalloc(&c->d_sup_bbox, std::max<uint64_t>(n_sup, 1) * sizeof(float4)));
        c->sup_bbox_cap = std::max<uint64_t>(n_sup, 1);
    }
    c->n_chunks = static_cast<uint32_t>(total);
    PM_TRY(hipMemcpyAsync(c->d_chunk_base, base.data(), base.size() * sizeof(uint32_t), hipMemcpyHostToDevice, c->stream));
    pm::LaunchIndex(c->d_scene, n, c->dev_items_ix, c->d_chunk_base, c->n_chunks, c->d_chunk_bbox, c->d_sup_bbox, c->stream);
    PM_TRY(hipGetLastError());
    PM_TRY(hipEventRecord(c->ev_scene, c->stream));  // (what a hit test on a caller's stream starts behind)
    // (no wait: frames run on streams that are ordered behind c->stream where it matters -- Enqueue below --
    //  and the next scene replacement starts with SyncAll before `base` is touched again)
    return PM_OK;
}

// A scene replacement starts by forgetting the old scene: if the upload, the flatten kernels or
// the validation fail, no later pm_render can pair the old item count / index / arena bounds
// with new, unvalidated device bytes (BuildParams refuses to render without a scene).
void InvalidateScene(pm_ctx *c) {
    c->scene_bytes = 0;
    c->user_scene_bytes = 0;
    c->n_items = 0;
    c->n_chunks = 0;
    c->item_meta.clear();
    c->meta_colours_stale = false;
    c->scene_from_paths = false;
    c->last_slot = -1;
    c->arena_dirty = true;
    for (auto &t : c->slot)  // (another scene: whether its frames are dense is for its own tile kernels to say)
        if (t.h_overflow) t.h_overflow[2] = 0;
}

int ReserveDevice(pm_ctx *c, size_t cap, size_t keep_bytes);

// Nested groups (extension, src/lib.rs:148): a scene with PietGroup items renders like the same
// items inlined depth first, in paint order.  The kernels only ever see a flat group, so the
// host appends that flat form -- {n, items_ix}, boxes, 32-byte items, the items' point arrays
// stay where they are -- behind the scene bytes.  Every offset is checked here.
struct FlatGroup {
    std::vector<uint8_t> boxes, items;
    uint32_t n = 0;
    uint64_t visits = 0;  // groups entered: a DAG of (empty) groups shared by many parents is cut off too
};

bool FlattenGroup(const uint8_t *sc, size_t len, uint64_t group, int depth, FlatGroup *out) {
    if (depth > 32 || group + 8 > len || (group & 3u) || ++out->visits > (1u << 24)) return false;
    uint32_t n, items_ix;
    std::memcpy(&n, sc + group, 4);
    std::memcpy(&items_ix, sc + group + 4, 4);
    if (group + 8ull + 8ull * n > len || static_cast<uint64_t>(items_ix) + 32ull * n > len || (items_ix & 3u)) return false;
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t *it = sc + items_ix + 32ull * i;
        uint32_t tag, child;
        std::memcpy(&tag, it, 4);
        if ((tag & 0xffffu) == pm::kItemGroup) {
            std::memcpy(&child, it + 8, 4);
            if (!FlattenGroup(sc, len, child, depth + 1, out)) return false;
            continue;
        }
        if (out->n >= (1u << 24)) return false;  // (also ends cyclic scenes)
        out->boxes.insert(out->boxes.end(), sc + group + 8 + 8ull * i, sc + group + 16 + 8ull * i);
        out->items.insert(out->items.end(), it, it + 32);
        out->n += 1;
    }
    return true;
}

// The scene bytes are resident in d_scene (`host` = the same bytes in host memory, or nullptr for
// a scene the flatten kernels wrote).  Builds the host copy of the drawn group in normal form
// {n, 8 + 8n}{boxes}{items} (validation, arena sizing) and the scene index.
int SetScene(pm_ctx *c, size_t bytes, const uint8_t *host) {
    if (bytes < 8) return PM_ERR_SCENE;
    const WallTimer timer;
    auto fail = [&](const char *what) {
        SetError(what);
        InvalidateScene(c);
        return PM_ERR_SCENE;
    };
    // (a scene the flatten kernels wrote: its head -- header, boxes, items -- came back with the totals)
    const uint8_t *head = c->flatten_cache.meta_bytes >= 8 && !host ? c->flatten_cache.h_meta + 32 : nullptr;
    const size_t head_bytes = head ? c->flatten_cache.meta_bytes : 0;
    uint32_t hdr[2];
    if (host) {
        std::memcpy(hdr, host, 8);
    } else if (head) {
        std::memcpy(hdr, head, 8);
    } else {
        PM_TRY(hipMemcpyAsync(hdr, c->d_scene, 8, hipMemcpyDeviceToHost, c->stream));
        PM_TRY(hipStreamSynchronize(c->stream));
    }
    const uint64_t n0 = hdr[0], items0 = hdr[1];
    if (items0 + 32ull * n0 > bytes || items0 < 8ull + 8ull * n0 || (items0 & 7u)) return fail("scene header out of range");
    std::vector<uint8_t> meta(8 + 40 * n0);
    uint32_t dev_bbox_ix = 8, dev_items_ix = hdr[1];
    size_t total = bytes;
    bool nested = false;
    if (host)
        for (uint64_t i = 0; i < n0 && !nested; ++i) {
            uint32_t tag;
            std::memcpy(&tag, host + items0 + 32 * i, 4);
            nested = (tag & 0xffffu) == pm::kItemGroup;
        }
    uint32_t n = hdr[0];
    if (nested) {
        FlatGroup flat;
        if (!FlattenGroup(host, bytes, 0, 0, &flat)) return fail("nested groups: offset out of range, too deep, or cyclic");
        n = flat.n;
        const size_t root = (bytes + 7u) & ~static_cast<size_t>(7u);
        total = root + 8 + 40ull * n;
        std::vector<uint8_t> blk(total - bytes, 0);
        const uint32_t ghdr[2] = {n, static_cast<uint32_t>(root + 8 + 8ull * n)};
        std::memcpy(blk.data() + (root - bytes), ghdr, 8);
        std::memcpy(blk.data() + (root - bytes) + 8, flat.boxes.data(), flat.boxes.size());
        std::memcpy(blk.data() + (root - bytes) + 8 + 8ull * n, flat.items.data(), flat.items.size());
        if (total > c->dev_scene_cap) {
            PM_TRY(hipStreamSynchronize(c->stream));  // the upload of the scene bytes is still in flight
            // (device copy only: the pinned buffer the caller encodes into stays where it is)
            const int rr = ReserveDevice(c, total + (total >> 3), bytes);
            if (rr != PM_OK) {
                InvalidateScene(c);
                return rr;
            }
        }
        PM_TRY(hipMemcpyAsync(c->d_scene + bytes, blk.data(), blk.size(), hipMemcpyHostToDevice, c->stream));
        PM_TRY(hipStreamSynchronize(c->stream));  // blk is a stack-owned source
        dev_bbox_ix = static_cast<uint32_t>(root + 8);
        dev_items_ix = ghdr[1];
        meta.resize(8 + 40ull * n);
        std::memcpy(meta.data() + 8, flat.boxes.data(), flat.boxes.size());
        std::memcpy(meta.data() + 8 + 8ull * n, flat.items.data(), flat.items.size());
    } else if (host) {
        std::memcpy(meta.data() + 8, host + 8, 8 * n0);
        std::memcpy(meta.data() + 8 + 8 * n0, host + items0, 32 * n0);
    } else if (head && items0 + 32 * n0 <= head_bytes) {
        std::memcpy(meta.data() + 8, head + 8, 8 * n0);
        std::memcpy(meta.data() + 8 + 8 * n0, head + items0, 32 * n0);
    } else if (n0) {
        PM_TRY(hipMemcpyAsync(meta.data() + 8, c->d_scene + 8, 8 * n0, hipMemcpyDeviceToHost, c->stream));
        PM_TRY(hipMemcpyAsync(meta.data() + 8 + 8 * n0, c->d_scene + items0, 32 * n0, hipMemcpyDeviceToHost, c->stream));
        PM_TRY(hipStreamSynchronize(c->stream));
    }
    const uint32_t mhdr[2] = {n, 8u + 8u * n};
    std::memcpy(meta.data(), mhdr, 8);
    uint32_t n_checked = 0;
    const int r = ValidateScene(meta.data(), meta.size(), total, &n_checked);
    if (r != PM_OK) {
        (void)fail("scene buffer failed validation");
        return r;
    }
    c->item_meta.swap(meta);
    c->meta_colours_stale = false;
    c->n_items = n;
    c->dev_bbox_ix = dev_bbox_ix;
    c->dev_items_ix = dev_items_ix;
    c->arena_dirty = true;
    c->last_slot = -1;
    const int ri = BuildSceneIndex(c);
    if (ri != PM_OK) {
        InvalidateScene(c);
        return ri;
    }
    c->user_scene_bytes = bytes;
    c->scene_bytes = total;  // only now is there a scene to render
    c->t_index_ms = timer.ms();
    return PM_OK;
}

int CheckSceneCap(size_t cap) {
    if (cap > 0xffffffffull) {  // offsets in the scene format (and in the kernels' bounds checks) are u32
        SetError("scene buffers are limited to 4 GiB - 1 (u32 offsets in the scene format)");
        return PM_ERR_CAPACITY;
    }
    return PM_OK;
}

// Grows the device copy of the scene (keeping its first keep_bytes).  The pinned host buffer is not
// touched: a pointer pm_scene_buffer returned stays valid (round-2 advisor finding).
int ReserveDevice(pm_ctx *c, size_t cap, size_t keep_bytes = 0) {
    if (cap <= c->dev_scene_cap) return PM_OK;
    keep_bytes = std::max(keep_bytes, c->scene_bytes);
    const int rc = CheckSceneCap(cap);
    if (rc != PM_OK) return rc;
    uint8_t *d = nullptr;
    PM_TRY(hipMalloc(&d, cap));
    if (c->d_scene) {
        if (keep_bytes) (void)hipMemcpy(d, c->d_scene, std::min(keep_bytes, c->dev_scene_cap), hipMemcpyDeviceToDevice);
        (void)hipFree(c->d_scene);
    }
    c->d_scene = d;
    c->dev_scene_cap = cap;
    return PM_OK;
}

// pm_create / pm_scene_reserve: the pinned host buffer AND the device copy.
int ReserveScene(pm_ctx *c, size_t cap) {
    if (cap > c->scene_cap) {
        const int rc = CheckSceneCap(cap);
        if (rc != PM_OK) return rc;
        uint8_t *h = nullptr;
        PM_TRY(hipHostMalloc(&h, cap, hipHostMallocDefault));
        std::memset(h, 0, cap);
        if (c->h_scene) {
            std::memcpy(h, c->h_scene, c->scene_cap);
            (void)hipHostFree(c->h_scene);
        }
        c->h_scene = h;
        c->scene_cap = cap;
    }
    return ReserveDevice(c, cap);
}

}  // namespace

// ---- what pm_gather.hip needs to know about a context -------------------------------------
namespace pm {
void SetLastError(const std::string &s) { SetError(s); }
int ContextDevice(const pm_ctx *c) { return c->device; }
hipStream_t ContextStream(pm_ctx *c) { return c->stream; }
int ContextViewport(const pm_ctx *c, uint32_t *width, uint32_t *height, uint32_t *row0, uint32_t *row1) {
    if (!c || c->tiles_x == 0) return PM_ERR_INVALID;
    *width = c->width;
    *height = c->height;
    *row0 = c->row0;
    *row1 = c->row1;
    return PM_OK;
}
// The last frame's framebuffer; work submitted to gather_stream after this call runs behind the frame.
int ContextLastFrame(pm_ctx *c, const void **fb, size_t *stride, hipStream_t gather_stream) {
    if (!c || c->last_slot < 0) {
        SetError("pm_gather: no frame rendered yet");
        return PM_ERR_INVALID;
    }
    FrameSlot &s = c->slot[c->last_slot];
    if (s.in_flight && s.frame_stream != gather_stream) {
        if (!s.user_stream) PM_TRY(hipEventRecord(s.ev_done, s.frame_stream));
        PM_TRY(hipStreamWaitEvent(gather_stream, s.ev_done, 0));
    }
    *fb = s.params.fb;
    *stride = s.params.fb_stride;
    return PM_OK;
}
}  // namespace pm

extern "C" {

const char *pm_last_error(void) { return g_last_error.c_str(); }

uint32_t pm_abi_version(void) { return PM_ABI_VERSION; }

pm_ctx *pm_create(int device, int *err) {
    int dummy;
    if (!err) err = &dummy;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) {
        SetError("no HIP device visible: piet_metal_amd has no CPU fallback");
        *err = PM_ERR_NO_DEVICE;
        return nullptr;
    }
    if (device < 0 || device >= count) {
        SetError("device index out of range");
        *err = PM_ERR_INVALID;
        return nullptr;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess || std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        SetError(std::string("device is not gfx950 (MI355X): ") + prop.gcnArchName);
        *err = PM_ERR_NO_DEVICE;
        return nullptr;
    }
    pm_ctx *c = new (std::nothrow) pm_ctx();
    if (!c) {
        *err = PM_ERR_CAPACITY;
        return nullptr;
    }
    c->device = device;
    c->n_cus = prop.multiProcessorCount;
    auto fail = [&](hipError_t e, const char *what) {
        HipFail(e, what);
        *err = PM_ERR_HIP;
        pm_destroy(c);
        return static_cast<pm_ctx *>(nullptr);
    };
    hipError_t e;
    if ((e = hipSetDevice(device)) != hipSuccess) return fail(e, "hipSetDevice");
    // Frames in flight (see the top of this file); tunable for experiments.
    const int n_streams = EnvInt("PM_FRAME_STREAMS", kDefaultFrameStreams, 1, kMaxSlots);
    c->slot.resize(static_cast<size_t>(EnvInt("PM_SLOTS", n_streams, 1, kMaxSlots)));
    for (int i = 0; i < n_streams; ++i) {
        hipStream_t q = nullptr;
        if ((e = hipStreamCreateWithFlags(&q, hipStreamNonBlocking)) != hipSuccess) return fail(e, "hipStreamCreate");
        c->streams.push_back(q);
    }
    c->stream = c->streams[0];
    c->coarse_wg_per_cu = static_cast<uint32_t>(EnvInt("PM_COARSE_WG_PER_CU", 5, 1, 16));
    c->split_mode = static_cast<uint32_t>(EnvInt("PM_FINE_SPLIT", 1, 0, 1));
    c->dense_factor = static_cast<uint32_t>(EnvInt("PM_DENSE_FACTOR", 4, 1, 1 << 20));
    c->dense_kernel_mode = EnvInt("PM_DENSE_KERNEL", 1, 0, 1);
    c->fine_wg_dense = static_cast<uint32_t>(EnvInt("PM_FINE_WG_PER_CU_DENSE", 6, 1, 16));
    c->fine_wg_dense_inflight = static_cast<uint32_t>(EnvInt("PM_FINE_WG_PER_CU_DENSE_INFLIGHT", 4, 1, 16));
    c->heavy_stream = static_cast<uint32_t>(EnvInt("PM_HEAVY_STREAM", 72, 1, 1 << 20));
    c->heavy_stream_lone = static_cast<uint32_t>(EnvInt("PM_HEAVY_STREAM_LONE", std::min<int>(40, static_cast<int>(c->heavy_stream)), 1, 1 << 20));
    c->vheavy_stream = static_cast<uint32_t>(EnvInt("PM_VHEAVY_STREAM", 112, 1, 1 << 20));
    c->fold_clear_mode = EnvInt("PM_FOLD_CLEAR", 3, 0, 4);
    c->fold_clear = c->fold_clear_mode != 0;
    c->fused = EnvInt("PM_FUSED", 1, 0, 1) != 0;
    c->handout = EnvInt("PM_HANDOUT", 0, 0, 2);
    c->fine_wg_per_cu = static_cast<uint32_t>(EnvInt("PM_FINE_WG_PER_CU", 5, 1, 16));
    c->fine_wg_per_cu_inflight = static_cast<uint32_t>(EnvInt("PM_FINE_WG_PER_CU_INFLIGHT", 3, 1, 16));
    c->bin_wg_per_cu = static_cast<uint32_t>(EnvInt("PM_BIN_WG_PER_CU", 0xff, 0, 0xff));
    c->bin_waves_env = static_cast<uint32_t>(EnvInt("PM_BIN_WAVES", 0, 0, 4));
    c->bin_waves_inflight = c->bin_waves_env ? c->bin_waves_env : static_cast<uint32_t>(EnvInt("PM_BIN_WAVES_INFLIGHT", 1, 1, 4));
    c->bin_prio_slots = static_cast<uint32_t>(EnvInt("PM_BIN_PRIO_SLOTS", 320, 0, 1 << 30));
    c->query_every = static_cast<uint32_t>(EnvInt("PM_QUERY_EVERY", 8, 1, 1 << 20));
    c->bin_split_mode = EnvInt("PM_BIN_SPLIT", 1, 0, 2);
    c->bin_wt_mode = EnvInt("PM_BIN_WT", 2, 0, 2);
    c->bin_split_cands = static_cast<uint32_t>(EnvInt("PM_BIN_SPLIT_CANDS", 1 << 30, 1, 1 << 30));
    c->bin_split_slots = static_cast<uint32_t>(EnvInt("PM_BIN_SPLIT_SLOTS", 224, 1, 1 << 30));
    c->bin_split_fill = static_cast<uint32_t>(EnvInt("PM_BIN_SPLIT_FILL", 15, 1, 16));
    c->one_launch_mode = EnvInt("PM_ONE_LAUNCH", 0, 0, 1);
    c->one_launch_split = EnvInt("PM_ONE_LAUNCH_SPLIT", 0, 0, 1) != 0;
    c->frame_spin_ticks = static_cast<uint32_t>(EnvInt("PM_ONE_LAUNCH_SPIN_US", 2000, 1, 1000000)) * 100u;
    {
        // the one-launch grid must be resident as a whole: what the occupancy API says a CU holds, four at most (the
        // kernel's registers are sized for four)
        const int res = pm::FrameKernelResidency();
        c->frame_wg_per_cu = res >= 4 ? 4u : 0u;
        if (const char *v = std::getenv("PM_FRAME_WG_PER_CU")) c->frame_wg_per_cu = static_cast<uint32_t>(std::max(0, std::min(res, std::atoi(v))));
    }

    for (auto &ev : c->ev)
        if ((e = hipEventCreate(&ev)) != hipSuccess) return fail(e, "hipEventCreate");
    if ((e = hipEventCreateWithFlags(&c->ev_scene, hipEventDisableTiming)) != hipSuccess) return fail(e, "hipEventCreate");
    if ((e = hipEventCreateWithFlags(&c->ev_hit, hipEventDisableTiming)) != hipSuccess) return fail(e, "hipEventCreate");
    for (auto &s : c->slot) {
        if ((e = hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming)) != hipSuccess) return fail(e, "hipEventCreate");
        if ((e = hipMalloc(&s.d_ctr, 2 * sizeof(pm::Counters))) != hipSuccess) return fail(e, "hipMalloc(counters)");
        if ((e = hipMemset(s.d_ctr, 0, 2 * sizeof(pm::Counters))) != hipSuccess) return fail(e, "hipMemset(counters)");
        if ((e = hipHostMalloc(&s.h_overflow, 64, hipHostMallocDefault)) != hipSuccess) return fail(e, "hipHostMalloc(overflow word)");
        s.h_overflow[0] = s.h_overflow[1] = s.h_overflow[2] = 0;
        void *dp = nullptr;
        if ((e = hipHostGetDevicePointer(&dp, s.h_overflow, 0)) != hipSuccess) return fail(e, "hipHostGetDevicePointer");
        s.d_overflow = static_cast<uint32_t *>(dp);
    }
    Luts *l = new (std::nothrow) Luts();
    if (!l) {
        *err = PM_ERR_CAPACITY;
        pm_destroy(c);
        return nullptr;
    }
    BuildLuts(l);
    e = hipMalloc(&c->d_lut_srgb2lin, sizeof(l->srgb2lin));
    if (e == hipSuccess) e = hipMalloc(&c->d_lut_unorm2h, sizeof(l->unorm2h));
    if (e == hipSuccess) e = hipMalloc(&c->d_lut_lin2srgb, sizeof(l->lin2srgb));
    if (e == hipSuccess) e = hipMemcpy(c->d_lut_srgb2lin, l->srgb2lin, sizeof(l->srgb2lin), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->d_lut_unorm2h, l->unorm2h, sizeof(l->unorm2h), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(c->d_lut_lin2srgb, l->lin2srgb, sizeof(l->lin2srgb), hipMemcpyHostToDevice);
    delete l;
    if (e != hipSuccess) return fail(e, "lookup tables");
    // The working set of an ordinary scene is reserved now (HBM is 288 GB; a context is created once):
    // flatten scratch, scene index, binning lists and frame slot 0's arenas.  The first scene and the
    // first frame then allocate nothing; larger scenes grow the buffers as before.
    if (EnvInt("PM_PREALLOC", 1, 0, 1)) {
        e = c->flatten_cache.Reserve(4096, 65536);
        if (e == hipSuccess) e = hipMalloc(&c->d_chunk_base, (65536 + 1) * sizeof(uint32_t));
        if (e == hipSuccess) c->chunk_base_cap = 65536 + 1;
        if (e == hipSuccess) e = hipMalloc(&c->d_chunk_bbox, (1u << 19) * sizeof(float4));
        if (e == hipSuccess) c->chunk_bbox_cap = 1u << 19;
        if (e == hipSuccess) e = hipMalloc(&c->d_sup_bbox, (1u << 16) * sizeof(float4));
        if (e == hipSuccess) c->sup_bbox_cap = 1u << 16;
        if (e == hipSuccess) e = c->sr_desc.Reserve(65536, 65536);
        if (e == hipSuccess) e = c->sr_list.Reserve(65536, 65536);
        if (e == hipSuccess) e = c->sr_slots.Reserve(65536, 65536);
        if (e == hipSuccess) e = c->sr_desc_whole.Reserve(65536, 65536);
        if (e == hipSuccess) e = c->band_bbox.Reserve(65536, 65536);
        if (e == hipSuccess) e = c->band_item.Reserve(65536, 65536);
        // ... and every frame slot's viewport buffers for anything up to 8192 x 8192 (BASELINE config 5: 256 MB of pixels, 70 MB of queues
        // and per-tile tables) and its arenas, sized for config 5 (2.2 GB of worst-case binning regions, 1.7 GB of tile arena): four slots are
        // 16 GB, 6 % of the HBM, and ~0.4 s of pm_create.  A resize within that allocates nothing, whichever slot the next frame lands on
        // (round 6 first reserved slot 0 only: config 5's first frame was 1.2 ms when it landed there and 85-115 ms -- one hipMalloc of
        // 3.8 GB -- when the frame counter stood elsewhere; PM_PREALLOC_SLOTS / _MPIXELS / _ARENA_MB / _TILE_MB).
#ifdef PM_EMU
        const int arena_mb = 192, tile_mb = 96, slots_dflt = 1;  // (the CPU emulation's "HBM" is the host's memory)
#else
        const int arena_mb = 2304, tile_mb = 1792, slots_dflt = static_cast<int>(kMaxSlots);
#endif
        const size_t n_pre = std::min<size_t>(c->slot.size(), static_cast<size_t>(EnvInt("PM_PREALLOC_SLOTS", slots_dflt, 1, static_cast<int>(kMaxSlots))));
        const size_t px = static_cast<size_t>(EnvInt("PM_PREALLOC_MPIXELS", 64, 0, 4096)) << 20;
        const size_t tables = std::max<size_t>(px / (pm::kTileW * pm::kTileH), 4);
        const uint32_t arena0 = static_cast<uint32_t>(EnvInt("PM_PREALLOC_ARENA_MB", arena_mb, 1, 12288)) << 18;  // dwords
        const uint32_t tile0 = std::max<uint32_t>(static_cast<uint32_t>(EnvInt("PM_PREALLOC_TILE_MB", tile_mb, 1, 16384)) << 16,  // quads
                                                  ((1u << 22) * pm::kCmdQuadsNum) / pm::kCmdQuadsDen);  // (what EnsureArena asks for at least)
        for (size_t si = 0; si < n_pre && e == hipSuccess; ++si) {
            FrameSlot &fs = c->slot[si];
            if (px != 0) {
                e = hipMalloc(&fs.d_fb, px * 4);
                const size_t queue_pre = QueueEntries(tables, tables / pm::kStripTiles);  // (viewports of whole strips, 8192 x 8192 among them)
                if (e == hipSuccess) e = hipMalloc(&fs.d_queue, queue_pre * sizeof(uint4) + 3 * tables * sizeof(uint32_t));
                if (e == hipSuccess) {
                    fs.fb_cap = px * 4;
                    fs.tables_cap = tables;
                    fs.queue_cap = queue_pre;
                }
            }
            if (e == hipSuccess) e = hipMalloc(&fs.d_arena, static_cast<size_t>(arena0) * sizeof(uint32_t));
            if (e == hipSuccess) fs.arena_cap = arena0;
            if (e == hipSuccess && !std::getenv("PM_PTCL_INITIAL_CMDS")) {
                e = fs.ptcl.Reserve(tile0, tile0);
            }
        }
        if (e != hipSuccess) return fail(e, "working-set reservation");
    }
    if (ReserveScene(c, 16u << 20) != PM_OK) {  // 16 MiB like PietRenderer.m:53
        *err = PM_ERR_HIP;
        pm_destroy(c);
        return nullptr;
    }
    // -initWithMetalKitView: builds its pipeline states up front (PietRenderer.m:33-47); here every
    // kernel of the path runs once on a three-point scene, so that the first real scene and frame do
    // not pay for code-object loading (about 1.5 ms spread over a dozen first launches).
    if (EnvInt("PM_WARMUP", 1, 0, 1)) {
        const pm_path wp = {0u, 3u, PM_PATH_FILL | PM_PATH_STROKE, 0x000000ffu, 0x000000ffu, 1.0f};
        pm_path_el we[3] = {};
        we[0].tag = PM_EL_MOVE; we[0].p[0] = 2.0; we[0].p[1] = 2.0;
        we[1].tag = PM_EL_LINE; we[1].p[0] = 12.0; we[1].p[1] = 3.0;
        we[2].tag = PM_EL_CURVE; we[2].p[0] = 12.0; we[2].p[1] = 8.0; we[2].p[2] = 8.0; we[2].p[3] = 12.0; we[2].p[4] = 3.0; we[2].p[5] = 12.0;
        const double ident[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 0.0};
        int rw = pm_resize(c, 40, 24);
        if (rw == PM_OK) rw = pm_flatten_and_encode(c, &wp, 1, we, 3, ident, 1.0f, nullptr, nullptr);
        if (rw == PM_OK) rw = pm_render(c);
        if (rw == PM_OK) rw = pm_sync(c);
        if (rw != PM_OK) {
            *err = rw;
            pm_destroy(c);
            return nullptr;
        }
        // back to a context without scene and viewport (the slots KEEP their buffers: the first real viewport that fits them -- slot
        // 0's are reserved for anything up to 8192 x 8192 -- allocates nothing, AllocSlotViewport)
        InvalidateScene(c);
        c->vp_epoch += 1;
        for (auto &s : c->slot) {
            s.in_flight = false;
            s.needs_check = false;
        }
        c->last_slot = -1;
        c->flatten_cache.resident = false;
        c->flatten_cache.meta_bytes = 0;
        c->width = c->height = c->tiles_x = c->tiles_y = c->strips_x = c->row0 = c->row1 = 0;
        c->frame = 0;
        c->t_flatten_ms = c->t_index_ms = c->t_arena_ms = 0;
        // ... and without the warm-up scene's arena sizes: the first real scene sizes its own (round-3 advisor
        // finding: the floor the three-point scene asked for used to stay in force for every scene after it)
        c->ptcl_want = 0;
        c->arena_cap = 0;
        if (std::getenv("PM_PTCL_INITIAL_CMDS"))  // tests of the overflow path: what pm_sync grew during the warm-up goes too
            for (auto &s : c->slot) s.ptcl.Free();
    }
    *err = PM_OK;
    return c;
}

void pm_destroy(pm_ctx *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)SyncAll(c);
    FreeViewport(c);
    for (auto &s : c->slot) {
        if (s.d_arena) (void)hipFree(s.d_arena);
        s.ptcl.Free();
        if (s.d_row_bbox) (void)hipFree(s.d_row_bbox);  // (the indices live behind the boxes)
        if (s.d_ctr) (void)hipFree(s.d_ctr);
        if (s.h_overflow) (void)hipHostFree(s.h_overflow);
        if (s.ev_done) (void)hipEventDestroy(s.ev_done);
    }
    c->sr_desc.Free();
    c->sr_list.Free();
    c->sr_slots.Free();
    c->sr_desc_whole.Free();
    c->band_bbox.Free();
    c->band_item.Free();
    c->row_base.Free();
    c->idle_sr.Free();
    c->sr_next_one.Free();
    c->flatten_cache.Free();
    if (c->d_scene) (void)hipFree(c->d_scene);
    if (c->d_scene_alt) (void)hipFree(c->d_scene_alt);
    if (c->h_scene) (void)hipHostFree(c->h_scene);
    if (c->d_chunk_base) (void)hipFree(c->d_chunk_base);
    if (c->d_chunk_bbox) (void)hipFree(c->d_chunk_bbox);
    if (c->d_sup_bbox) (void)hipFree(c->d_sup_bbox);
    if (c->d_lut_srgb2lin) (void)hipFree(c->d_lut_srgb2lin);
    if (c->d_lut_unorm2h) (void)hipFree(c->d_lut_unorm2h);
    if (c->d_lut_lin2srgb) (void)hipFree(c->d_lut_lin2srgb);
    for (auto &ev : c->ev)
        if (ev) (void)hipEventDestroy(ev);
    if (c->ev_scene) (void)hipEventDestroy(c->ev_scene);
    if (c->ev_hit) (void)hipEventDestroy(c->ev_hit);
    if (c->d_stage) (void)hipFree(c->d_stage);
    for (int k = 0; k < pm_ctx::kPolySlots; ++k) {
        if (c->ev_poly[k]) (void)hipEventDestroy(c->ev_poly[k]);
        if (c->d_poly[k]) (void)hipFree(c->d_poly[k]);
        if (c->h_poly[k]) (void)hipHostFree(c->h_poly[k]);
    }
    for (hipStream_t q : c->streams) (void)hipStreamDestroy(q);
    delete c;
}

int pm_resize(pm_ctx *c, uint32_t width, uint32_t height) {
    if (!c || width == 0 || height == 0 || width > 65535 || height > 65535) return PM_ERR_INVALID;
    const WallTimer tm;
    PM_TRY(hipSetDevice(c->device));
    const float t_a = tm.ms();
    int r = SyncAll(c);
    if (r != PM_OK) return r;
    if (std::getenv("PM_HOST_TIMING")) std::fprintf(stderr, "pm_resize: setdevice %.3f syncall %.3f ms\n", t_a, tm.ms() - t_a);
    c->width = width;
    c->height = height;
    c->tiles_x = (width + pm::kTileW - 1) / pm::kTileW;   // PietRenderer.m:63-64
    c->tiles_y = (height + pm::kTileH - 1) / pm::kTileH;
    c->strips_x = (c->tiles_x + pm::kStripTiles - 1) / pm::kStripTiles;
    c->row0 = 0;
    c->row1 = c->tiles_y;
    const float t_b = tm.ms();
    r = AllocViewport(c);
    if (std::getenv("PM_HOST_TIMING")) std::fprintf(stderr, "pm_resize: viewport buffers %.3f ms\n", tm.ms() - t_b);
    return r;
}

int pm_set_band(pm_ctx *c, uint32_t tile_row0, uint32_t tile_row1) {
    if (!c || c->tiles_y == 0 || tile_row0 >= tile_row1 || tile_row1 > c->tiles_y) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r = SyncAll(c);
    if (r != PM_OK) return r;
    c->row0 = tile_row0;
    c->row1 = tile_row1;
    return AllocViewport(c);
}

uint8_t *pm_scene_buffer(pm_ctx *c, size_t *cap) {
    if (!c) return nullptr;
    if (cap) *cap = c->scene_cap;
    return c->h_scene;
}

int pm_scene_reserve(pm_ctx *c, size_t cap) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r = SyncAll(c);
    if (r != PM_OK) return r;
    return ReserveScene(c, cap);
}

int pm_upload_scene(pm_ctx *c, size_t bytes) {
    if (!c || bytes > c->scene_cap || bytes < 8) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r = SyncAll(c);  // frames in flight still read the old scene
    if (r != PM_OK) return r;
    InvalidateScene(c);
    c->fb_slots.clear();  // (another scene: its own frames will say which strip rows are heavy -- a view change, pm_reflatten, keeps the report)
    c->plan.fb_applied = false;
    c->replan_wide = false;
    c->plan.reusable = false;
    c->t_flatten_ms = 0;
    // (a context that goes back to host-encoded scenes gives the device flatten's second scene buffer back: round-4 advisor finding)
    if (c->d_scene_alt) {
        (void)hipFree(c->d_scene_alt);
        c->d_scene_alt = nullptr;
        c->dev_scene_alt_cap = 0;
    }
    PM_TRY(hipMemcpyAsync(c->d_scene, c->h_scene, bytes, hipMemcpyHostToDevice, c->stream));
    return SetScene(c, bytes, c->h_scene);  // (stream order: the appended flat group follows the upload)
}

namespace {
int FlattenAndEncode(pm_ctx *c, bool resident, const pm_path *paths, size_t n_paths, const pm_path_el *els, size_t n_els, const pm::DashTable *dash,
                     const double affine[6], float width_scale, size_t *scene_bytes, uint32_t *n_items, bool grouped = false);
}

int pm_flatten_and_encode(pm_ctx *c, const pm_path *paths, size_t n_paths, const pm_path_el *els, size_t n_els,
                          const double affine[6], float width_scale, size_t *scene_bytes, uint32_t *n_items) {
    if (!c || !affine || (n_paths && !paths) || (n_els && !els)) return PM_ERR_INVALID;
    c->fb_slots.clear();  // (new paths: their own frames will say which strip rows are heavy)
    c->plan.fb_applied = false;
    c->replan_wide = false;
    c->plan.reusable = false;  // (new paths: planned afresh, for their own boxes)
    return FlattenAndEncode(c, false, paths, n_paths, els, n_els, nullptr, affine, width_scale, scene_bytes, n_items);
}

int pm_flatten_and_encode_dashed(pm_ctx *c, const pm_path *paths, size_t n_paths, const pm_path_el *els, size_t n_els,
                                 const pm_path_dash *dashes, size_t n_dashes, const float *dash_values, size_t n_dash_values,
                                 const double affine[6], float width_scale, size_t *scene_bytes, uint32_t *n_items) {
    if (n_dashes == 0) return pm_flatten_and_encode(c, paths, n_paths, els, n_els, affine, width_scale, scene_bytes, n_items);
    if (!c || !affine || (n_paths && !paths) || (n_els && !els) || !dashes || (n_dash_values && !dash_values)) return PM_ERR_INVALID;
    c->fb_slots.clear();
    c->plan.fb_applied = false;
    c->replan_wide = false;
    c->plan.reusable = false;
    const pm::DashTable table{dashes, n_dashes, dash_values, n_dash_values};
    return FlattenAndEncode(c, false, paths, n_paths, els, n_els, &table, affine, width_scale, scene_bytes, n_items);
}

namespace {
int FlattenAndEncode(pm_ctx *c, bool resident, const pm_path *paths, size_t n_paths, const pm_path_el *els, size_t n_els, const pm::DashTable *dash,
                     const double affine[6], float width_scale, size_t *scene_bytes, uint32_t *n_items, bool grouped) {
    PM_TRY(hipSetDevice(c->device));
    size_t bytes = 0;
    uint32_t items = 0;
    hipError_t he = hipSuccess;
    const WallTimer timer;
    // The kernels write the OTHER scene buffer: frames in flight keep reading the current one meanwhile (nothing reads
    // the other one: every scene replacement ends with all frames waited for, below).
    auto grow_alt = [&](size_t cap) -> int {
        if (cap <= c->dev_scene_alt_cap && c->d_scene_alt) return PM_OK;
        const int rc = CheckSceneCap(cap);
        if (rc != PM_OK) return rc;
        if (c->d_scene_alt) (void)hipFree(c->d_scene_alt);
        c->d_scene_alt = nullptr;
        c->dev_scene_alt_cap = 0;
        PM_TRY(hipMalloc(&c->d_scene_alt, cap));
        c->dev_scene_alt_cap = cap;
        return PM_OK;
    };
    int r = grow_alt(c->dev_scene_cap);
    if (r == PM_OK)
        r = pm::FlattenEncodeOnDevice(c->stream, &c->flatten_cache, resident, paths, n_paths, els, n_els, dash, affine, width_scale, c->d_scene_alt,
                                      c->dev_scene_alt_cap, &bytes, &items, &he, grouped);
    // (a dash table: the dashes of a scene whose poly-lines did not fit are counted by the call after the one that made room for them)
    for (int attempt = 0; attempt < (c->flatten_cache.n_dashes ? 2 : 1) && r == PM_ERR_CAPACITY && bytes > c->dev_scene_alt_cap; ++attempt) {
        // grow it (the kernels write it; nothing is staged on the host) and retry once.  `bytes` is the exact need (the point count
        // behind it is summed in 64 bits): beyond 4 GiB - 1 grow_alt refuses it; the headroom never makes a need that fits not fit.
        r = grow_alt(std::max<size_t>(bytes, std::min<size_t>(bytes + (bytes >> 3), 0xffffffffull)));
        if (r == PM_OK)
            r = pm::FlattenEncodeOnDevice(c->stream, &c->flatten_cache, resident, paths, n_paths, els, n_els, dash, affine, width_scale, c->d_scene_alt,
                                          c->dev_scene_alt_cap, &bytes, &items, &he, grouped);
    }
    const float flatten_ms = timer.ms();
    {
        // ... and only now the frames in flight are waited for: they read the current scene buffer, and the scene index and
        // binning lists SetScene / the next frame replace.  Whatever happened above, the old scene is gone after this call.
        const int rs = SyncAll(c);
        InvalidateScene(c);
        if (rs != PM_OK) return rs;
    }
    if (r == PM_ERR_HIP) return HipFail(he, "flatten kernels");
    if (r != PM_OK) {
        if (r != PM_ERR_CAPACITY || g_last_error.empty()) SetError("flatten/encode rejected the paths");
        if (r == PM_ERR_CAPACITY && scene_bytes) *scene_bytes = bytes;  // the size the scene would have needed (0: not known)
        return r;
    }
    std::swap(c->d_scene, c->d_scene_alt);
    std::swap(c->dev_scene_cap, c->dev_scene_alt_cap);
    c->t_flatten_ms = flatten_ms;
    r = SetScene(c, bytes, nullptr);
    if (r != PM_OK) return r;
    c->scene_from_paths = true;
    if (scene_bytes) *scene_bytes = bytes;
    if (n_items) *n_items = items;
    return PM_OK;
}
}  // namespace

int pm_reflatten(pm_ctx *c, const double affine[6], float width_scale, size_t *scene_bytes, uint32_t *n_items) {
    if (!c || !affine) return PM_ERR_INVALID;
    if (!c->flatten_cache.resident) {
        SetError("pm_reflatten: no paths resident (pm_flatten_and_encode first)");
        return PM_ERR_INVALID;
    }
    c->replan_wide = true;  // (a view change: the next plan is made to last, EnsureArena)
    return FlattenAndEncode(c, true, nullptr, 0, nullptr, 0, nullptr, affine, width_scale, scene_bytes, n_items);
}

int pm_path_groups(pm_ctx *c, const uint32_t *group_of_path, size_t n_paths) {
    if (!c || !group_of_path) {
        SetError("pm_path_groups: NULL argument");
        return PM_ERR_INVALID;
    }
    if (!c->flatten_cache.resident) {
        SetError("pm_path_groups: no paths resident (pm_flatten_and_encode first)");
        return PM_ERR_INVALID;
    }
    if (n_paths != c->flatten_cache.n_paths) {
        SetError("pm_path_groups: n_paths is " + std::to_string(n_paths) + ", " + std::to_string(c->flatten_cache.n_paths) + " paths are resident");
        return PM_ERR_INVALID;
    }
    PM_TRY(hipSetDevice(c->device));
    hipError_t he = hipSuccess;
    const int r = pm::FlattenSetPathGroups(c->stream, &c->flatten_cache, group_of_path, n_paths, &he);
    if (r == PM_ERR_HIP) return HipFail(he, "pm_path_groups");
    return r;
}

int pm_reflatten_groups(pm_ctx *c, const pm_group_xform *xforms, size_t n_groups, size_t *scene_bytes, uint32_t *n_items) {
    if (!c || !xforms) {
        SetError("pm_reflatten_groups: NULL argument");
        return PM_ERR_INVALID;
    }
    if (!c->flatten_cache.resident) {
        SetError("pm_reflatten_groups: no paths resident (pm_flatten_and_encode first)");
        return PM_ERR_INVALID;
    }
    if (!c->flatten_cache.has_groups) {
        SetError("pm_reflatten_groups: no group map resident (pm_path_groups after pm_flatten_and_encode)");
        return PM_ERR_INVALID;
    }
    if (n_groups == 0 || n_groups <= c->flatten_cache.max_group) {
        SetError("pm_reflatten_groups: " + std::to_string(n_groups) + " transforms for a group map that reaches index " +
                 std::to_string(c->flatten_cache.max_group));
        return PM_ERR_INVALID;
    }
    for (size_t g = 0; g < n_groups; ++g) {
        if (xforms[g].reserved != 0) {
            SetError("pm_reflatten_groups: reserved must be 0 (transform " + std::to_string(g) + ")");
            return PM_ERR_INVALID;
        }
    }
    PM_TRY(hipSetDevice(c->device));
    hipError_t he = hipSuccess;
    // (the one copy of the table, in front of the kernels; a grow-and-retry finds it where it is)
    if (pm::FlattenStageGroupTable(c->stream, &c->flatten_cache, xforms, n_groups, &he) != PM_OK) {
        // (the table of the resident scene may be gone with the failed re-allocation: a grouped scene without its table cannot be
        //  repainted, decision D17 -- whatever happened, the old scene is gone, as after any failed replacement)
        (void)SyncAll(c);
        InvalidateScene(c);
        return HipFail(he, "pm_reflatten_groups");
    }
    c->replan_wide = true;  // (as pm_reflatten: the next plan is made to last, EnsureArena)
    const double unused[6] = {1.0, 0.0, 0.0, 1.0, 0.0, 0.0};
    return FlattenAndEncode(c, true, nullptr, 0, nullptr, 0, nullptr, unused, 1.0f, scene_bytes, n_items, true);
}

// Decision D17: the colours of the resident scene change, nothing else.  No flatten kernel, no read-back, no SetScene, no scene
// index (it is geometry only), and the binning plan in force stays (arena_dirty is left alone): the next frame bins the same boxes
// into the same regions.  The kernels write the OTHER scene buffer, as FlattenAndEncode's do, and the two change places.
int pm_repaint_groups(pm_ctx *c, const pm_group_paint *paints, size_t n_groups) {
    if (!c || !paints) {
        SetError("pm_repaint_groups: NULL argument");
        return PM_ERR_INVALID;
    }
    const pm::FlattenCache &fc = c->flatten_cache;
    if (!fc.resident) {
        SetError("pm_repaint_groups: no paths resident (pm_flatten_and_encode first)");
        return PM_ERR_INVALID;
    }
    if (!fc.has_groups) {
        SetError("pm_repaint_groups: no group map resident (pm_path_groups after pm_flatten_and_encode)");
        return PM_ERR_INVALID;
    }
    if (n_groups == 0 || n_groups <= fc.max_group) {
        SetError("pm_repaint_groups: " + std::to_string(n_groups) + " paints for a group map that reaches index " + std::to_string(fc.max_group));
        return PM_ERR_INVALID;
    }
    for (size_t g = 0; g < n_groups; ++g) {
        if (paints[g].opacity > 255u) {
            SetError("pm_repaint_groups: opacity " + std::to_string(paints[g].opacity) + " is above 255 (paint " + std::to_string(g) + ")");
            return PM_ERR_INVALID;
        }
    }
    if (!c->scene_from_paths || c->scene_bytes < 8 || c->scene_bytes != c->user_scene_bytes || (fc.scene_grouped && !fc.d_xforms)) {
        SetError("pm_repaint_groups: the resident scene did not come from the resident paths (pm_upload_scene since, or the last replacement failed)");
        return PM_ERR_INVALID;
    }
    PM_TRY(hipSetDevice(c->device));
    const WallTimer timer;
    if (c->scene_bytes > c->dev_scene_alt_cap || !c->d_scene_alt) {
        // (the other buffer is the one of two replacements back and may be the smaller one; nothing reads it: every replacement ends
        //  with all frames and hit tests waited for.  Grown once, then never again for scenes of this size.)
        if (c->d_scene_alt) (void)hipFree(c->d_scene_alt);
        c->d_scene_alt = nullptr;
        c->dev_scene_alt_cap = 0;
        PM_TRY(hipMalloc(&c->d_scene_alt, c->dev_scene_cap));
        c->dev_scene_alt_cap = c->dev_scene_cap;
    }
    hipError_t he = hipSuccess;
    const int r = pm::FlattenRepaint(c->stream, &c->flatten_cache, paints, n_groups, c->d_scene, c->d_scene_alt, c->scene_bytes, c->n_items, &he);
    // The two waits of every replacement: the frames and hit tests in flight read the current buffer, and after this call nothing
    // reads the other one -- which the replacement after this one overwrites.
    const int rs = SyncAll(c);
    if (rs != PM_OK || r != PM_OK) {
        InvalidateScene(c);  // (a HIP failure: the paths' colours and the scene may no longer belong together)
        if (rs != PM_OK) return rs;
        return r == PM_ERR_HIP ? HipFail(he, "pm_repaint_groups") : r;
    }
    std::swap(c->d_scene, c->d_scene_alt);
    std::swap(c->dev_scene_cap, c->dev_scene_alt_cap);
    c->meta_colours_stale = true;
    c->last_slot = -1;  // (as after every replacement: no frame of this scene yet, pm_read_pixels has nothing to name)
    c->t_flatten_ms = timer.ms();
    c->t_index_ms = 0;
    return PM_OK;
}

int pm_download_scene(pm_ctx *c, uint8_t *dst, size_t cap, size_t *bytes) {
    if (!c || !dst) return PM_ERR_INVALID;
    if (bytes) *bytes = c->user_scene_bytes;
    if (cap < c->user_scene_bytes) return PM_ERR_CAPACITY;
    PM_TRY(hipSetDevice(c->device));
    PM_TRY(hipMemcpyAsync(dst, c->d_scene, c->user_scene_bytes, hipMemcpyDeviceToHost, c->stream));
    PM_TRY(hipStreamSynchronize(c->stream));
    return PM_OK;
}

int pm_render(pm_ctx *c) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    return Enqueue(c, nullptr, c->fb_stride, nullptr);
}

int pm_render_to(pm_ctx *c, void *dev_framebuffer, size_t stride_bytes, void *hip_stream) {
    if (!c || !dev_framebuffer || (stride_bytes & 3u) || stride_bytes < static_cast<size_t>(c->width) * 4) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    return Enqueue(c, static_cast<uint8_t *>(dev_framebuffer), stride_bytes, hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream);
}

// pm_sync also repairs frames whose command-list arena ran out: pm_bin_kernel marks their tiles
// "no list", the tile kernels skip them, and the frame is left with holes.  EVERY slot that
// carried a frame since the last sync is inspected (up to four frames are in flight, and
// pm_render_to frames each own a caller buffer): the arena grows and each distinct target whose
// most recent frame overflowed is rendered again, oldest first, so that after PM_OK every
// framebuffer handed to this context holds a complete frame.  (A caller that synchronises only
// its own stream never learns of an overflow: pm_sync is the status channel.)
int pm_set_target_format(pm_ctx *c, int fmt) {
    if (!c || (fmt != PM_FMT_RGBA8 && fmt != PM_FMT_BGRA8)) return PM_ERR_INVALID;
    c->target_fmt = fmt;  // (frames already submitted keep the order they were submitted with)
    return PM_OK;
}

int pm_sync(pm_ctx *c) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    auto own_fb = [&](const uint8_t *fb) {
        for (auto &t : c->slot)
            if (fb == t.d_fb) return true;
        return false;
    };
    for (int attempt = 0; attempt < 6; ++attempt) {
        // The frame that defines each target's content: per caller-owned buffer the newest frame
        // submitted since the last sync; of the context's own slot buffers only the last frame's
        // (the one pm_read_pixels / pm_framebuffer_device_ptr name).  Oldest first.
        std::vector<int> latest;
        for (size_t k = 0; k < c->slot.size(); ++k) {
            const int si = static_cast<int>((c->frame + k) % c->slot.size());  // slot c->frame % n holds the oldest frame
            const FrameSlot &s = c->slot[si];
            // (not `in_flight`: every call that waits for the device clears that -- pm_get_stats,
            //  pm_frame_latency, ... -- and a frame with holes must not slip through behind them)
            if (!s.needs_check) continue;
            if (own_fb(s.params.fb)) {
                if (si != c->last_slot) continue;
            } else {
                latest.erase(std::remove_if(latest.begin(), latest.end(), [&](int o) { return c->slot[o].params.fb == s.params.fb; }),
                             latest.end());
            }
            latest.push_back(si);
        }
        int r = SyncAll(c);
        if (r != PM_OK) return r;
        for (auto &t : c->slot) t.needs_check = false;  // (the frames left out of `latest` were superseded on their target)
        std::vector<pm::FrameParams> redo;
        uint64_t want = 0;
        bool gave_up = false;
        // A one-launch frame gave up waiting inside its launch (its workgroups were not all resident, or somebody else's work
        // held the device): the frame has holes, and its slot's hand-over state -- FIFO entries that were pushed and never
        // popped, counters -- is no longer all zero.  EVERY slot whose frame gave up is put back to all zero, also a slot whose
        // frame has since been superseded on its target and needs no second rendering (round-5 advisor: left alone, the next
        // one-launch frame of that slot could pop a stale entry); every frame from now on takes two launches.
        {
            bool repaired = false;
            for (auto &t : c->slot) {
                if (!t.h_overflow || static_cast<volatile uint32_t *>(t.h_overflow)[1] == 0u) continue;
                c->one_launch_broken = true;
                if (t.d_fifo) PM_TRY(hipMemset(t.d_fifo, 0, static_cast<size_t>(pm::kFifos) * t.fifo_cap * sizeof(uint4)));
                if (t.d_ctr) PM_TRY(hipMemset(t.d_ctr, 0, 2 * sizeof(pm::Counters)));
                repaired = true;
            }
            if (repaired) PM_TRY(hipDeviceSynchronize());  // (the frame streams do not wait for the null stream's memsets)
        }
        for (int si : latest) {
            FrameSlot &s = c->slot[si];
            if (static_cast<volatile uint32_t *>(s.h_overflow)[1] != 0u) {  // ... and the frame is rendered again with two launches
                gave_up = true;
                redo.push_back(s.params);
                continue;
            }
            // (the slot's pinned word first: no frame of the slot has run out of arena since it was last cleared -- the usual
            //  case -- and pm_sync costs no copy from the device, 15 us each)
            if (*static_cast<volatile uint32_t *>(s.h_overflow) == 0u) continue;
            uint32_t overflow = 0;
            PM_TRY(hipMemcpy(&overflow, &s.params.ctr_cur->overflow, sizeof(overflow), hipMemcpyDeviceToHost));
            if (!overflow) continue;
            // (every part of the arena has to hold what ITS strip rows asked for: size all by the fullest)
            pm::Counters k;
            PM_TRY(hipMemcpy(&k, s.params.ctr_cur, offsetof(pm::Counters, cls), hipMemcpyDeviceToHost));
            uint64_t top = 0;
            for (uint32_t i = 0; i < pm::kArenaShards; ++i) top = std::max<uint64_t>(top, k.ptcl[i].top);
            top = (top + 2) * pm::kArenaShards;
            want = std::max<uint64_t>(want, std::max<uint64_t>(4ull * s.ptcl.cap, 2ull * top));
            redo.push_back(s.params);
        }
        for (auto &t : c->slot) t.h_overflow[0] = t.h_overflow[1] = 0;  // (nothing is in flight: every frame that raised one has been looked at or superseded)
        if (redo.empty()) return PM_OK;
        want = std::min<uint64_t>(0x7fffffffull, want);
        if (want <= c->ptcl_want && !gave_up) break;
        c->ptcl_want = std::max<uint64_t>(c->ptcl_want, want);  // (every slot grows when it is used next, EnsureSlotBuffers)
        // render the damaged targets again on the context's own streams (a caller's stream may be
        // gone by now; the next pass of this loop waits for them and checks them again)
        for (const pm::FrameParams &p : redo) {
            r = Enqueue(c, own_fb(p.fb) ? nullptr : p.fb, p.fb_stride, nullptr);
            if (r != PM_OK) return r;
        }
    }
    SetError("tile arena overflow (frame needs more than 32 GiB of pieces and command lists)");
    return PM_ERR_CAPACITY;
}

int pm_read_pixels(pm_ctx *c, uint8_t *dst, size_t dst_stride, int fmt) {
    if (!c || !dst || c->last_slot < 0 || dst_stride < static_cast<size_t>(c->width) * 4) return PM_ERR_INVALID;
    const int r = pm_sync(c);
    if (r != PM_OK) return r;
    const FrameSlot *s = &c->slot[c->last_slot];
    const uint32_t rows = std::min(BandRows(c) * pm::kTileH, c->height - c->row0 * pm::kTileH);
    PM_TRY(hipMemcpy2D(dst, dst_stride, s->params.fb, s->params.fb_stride, static_cast<size_t>(c->width) * 4, rows, hipMemcpyDeviceToHost));
    if ((fmt == PM_FMT_BGRA8) != (s->params.fb_bgra != 0)) {  // the frame was stored in the other byte order
        for (uint32_t y = 0; y < rows; ++y) {
            uint8_t *row = dst + static_cast<size_t>(y) * dst_stride;
            for (uint32_t x = 0; x < c->width; ++x) std::swap(row[4 * x], row[4 * x + 2]);
        }
    }
    return PM_OK;
}

void *pm_framebuffer_device_ptr(pm_ctx *c, size_t *stride_bytes, uint32_t *rows) {
    if (!c) return nullptr;
    if (stride_bytes) *stride_bytes = c->fb_stride;
    if (rows) *rows = BandRows(c) * pm::kTileH;
    return c->slot[c->last_slot >= 0 ? c->last_slot : 0].d_fb;
}

void *pm_scene_device_ptr(pm_ctx *c, size_t *bytes) {
    if (!c) return nullptr;
    if (bytes) *bytes = c->user_scene_bytes;
    return c->d_scene;
}

int pm_time_frames(pm_ctx *c, int iters, float *total_ms, float *bin_ms, float *coarse_ms, float *fine_ms, float *clear_ms) {
    if (!c || iters <= 0) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r;
    if ((r = SyncAll(c)) != PM_OK) return r;
    if (total_ms) {
        // pipelined, as pm_render submits them: start on the binning stream, end on the tile stream
        PM_TRY(hipEventRecord(c->ev[0], c->stream));  // everything is idle: fires at once
        for (int i = 0; i < iters; ++i)
            if ((r = Enqueue(c, nullptr, c->fb_stride, nullptr)) != PM_OK) return r;
        for (auto &s : c->slot)  // join: the end event follows the last frame of every stream
            if (s.in_flight && s.frame_stream != c->stream) {
                if (!s.user_stream) PM_TRY(hipEventRecord(s.ev_done, s.frame_stream));
                PM_TRY(hipStreamWaitEvent(c->stream, s.ev_done, 0));
            }
        PM_TRY(hipEventRecord(c->ev[1], c->stream));
        PM_TRY(hipEventSynchronize(c->ev[1]));
        PM_TRY(hipEventElapsedTime(total_ms, c->ev[0], c->ev[1]));
        if ((r = SyncAll(c)) != PM_OK) return r;
    }
    if (bin_ms || coarse_ms || fine_ms || clear_ms) {
        // one kernel at a time on one stream, each launch bracketed by events
        double a1 = 0, a2 = 0, a3 = 0, a4 = 0;
        for (int i = 0; i < iters; ++i) {
            const int si = static_cast<int>(c->frame % c->slot.size());
            FrameSlot *s = &c->slot[si];
            pm::FrameParams p;
            if ((r = BuildParams(c, s, nullptr, c->fb_stride, &p)) != PM_OK) return r;
            // each dispatch carries its own begin / end events: pure kernel durations
            PM_TRY(ResetTileState(c, s, c->stream));
            pm::LaunchBin(p, c->stream, c->ev[0], c->ev[1]);
            if (!c->fused) pm::LaunchCoarse(p, CoarseGrid(c), false, c->stream, c->ev[2], c->ev[3]);
            pm::LaunchFine(p, c->fold_clear && !p.clear_in_bin ? BandRows(c) * c->strips_x : 0u, c->fused, c->stream, c->ev[4], c->ev[5]);
            if (!c->fold_clear && !p.clear_in_bin) pm::LaunchClear(p, BandRows(c) * c->strips_x, c->stream, c->ev[6], c->ev[7]);
            PM_TRY(hipStreamSynchronize(c->stream));
            Submitted(c, si, p, c->stream);
            s->in_flight = false;  // (waited for just above: the next frame is alone too, and is launched as such)
            float t1 = 0, t2 = 0, t3 = 0, t4 = 0;
            PM_TRY(hipEventElapsedTime(&t1, c->ev[0], c->ev[1]));
            if (!c->fused) PM_TRY(hipEventElapsedTime(&t2, c->ev[2], c->ev[3]));
            PM_TRY(hipEventElapsedTime(&t3, c->ev[4], c->ev[5]));
            if (!c->fold_clear && !p.clear_in_bin) PM_TRY(hipEventElapsedTime(&t4, c->ev[6], c->ev[7]));
            a1 += t1;
            a2 += t2;
            a3 += t3;
            a4 += t4;
        }
        if (bin_ms) *bin_ms = static_cast<float>(a1 / iters);
        if (coarse_ms) *coarse_ms = static_cast<float>(a2 / iters);
        if (fine_ms) *fine_ms = static_cast<float>(a3 / iters);
        if (clear_ms) *clear_ms = static_cast<float>(a4 / iters);
    }
    return pm_sync(c);
}

int pm_time_frames_pipelined(pm_ctx *c, int iters, float *total_ms, float *bin_ms, float *coarse_ms, float *fine_ms,
                             float *clear_ms) {
    if (!c || iters <= 0 || iters > 4096) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r;
    if ((r = SyncAll(c)) != PM_OK) return r;
    std::vector<hipEvent_t> tev(static_cast<size_t>(iters) * 8, nullptr);
    hipError_t e = hipSuccess;
    for (auto &v : tev)
        if (e == hipSuccess) e = hipEventCreate(&v);
    r = PM_OK;
    if (e != hipSuccess) r = HipFail(e, "hipEventCreate");
    if (r == PM_OK) e = hipEventRecord(c->ev[0], c->stream);
    // (every frame of the batch as a frame among others is launched: the per-frame decision would fold the
    //  first one's clearing into its tile kernel and leave that frame's clear events unrecorded)
    // ... as Enqueue launches frames behind other frames: clearing in a launch of its own for large viewports, folded into
    // the tile kernel's for small ones (round-3 advisor finding: the batch used to be timed unfolded at every size)
    const int fold_mode = c->fold_clear_mode;
    if (fold_mode == 2) c->fold_clear_mode = BandTiles(c) < 16384u ? 1 : 0;
    const bool folded = c->fold_clear_mode == 1 || c->fold_clear_mode >= 3;  // (no clearing launch of its own: folded into the tile kernel's, or into binning's)
    for (int i = 0; i < iters && r == PM_OK; ++i) r = Enqueue(c, nullptr, c->fb_stride, nullptr, &tev[static_cast<size_t>(i) * 8]);
    c->fold_clear_mode = fold_mode;
    if (r == PM_OK) {
        for (auto &s : c->slot) {
            if (!s.in_flight || s.frame_stream == c->stream) continue;
            if (e == hipSuccess && !s.user_stream) e = hipEventRecord(s.ev_done, s.frame_stream);
            if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, s.ev_done, 0);
        }
        if (e == hipSuccess) e = hipEventRecord(c->ev[1], c->stream);
        if (e == hipSuccess) e = hipEventSynchronize(c->ev[1]);
        if (e == hipSuccess) r = SyncAll(c);
        double acc[4] = {0, 0, 0, 0};  // bin, clear, coarse, fine
        for (int i = 0; i < iters && e == hipSuccess && r == PM_OK; ++i)
            for (int k = 0; k < 4 && e == hipSuccess; ++k) {
                if (k == 1 && folded) continue;  // no separate clear launch
                if (k == 2 && c->fused) continue;       // no separate coarse launch
                float t = 0;
                e = hipEventElapsedTime(&t, tev[static_cast<size_t>(i) * 8 + 2 * k], tev[static_cast<size_t>(i) * 8 + 2 * k + 1]);
                acc[k] += t;
            }
        float tt = 0;
        if (e == hipSuccess) e = hipEventElapsedTime(&tt, c->ev[0], c->ev[1]);
        if (e != hipSuccess) r = HipFail(e, "pipelined timing");
        if (total_ms) *total_ms = tt;
        if (bin_ms) *bin_ms = static_cast<float>(acc[0] / iters);
        if (clear_ms) *clear_ms = static_cast<float>(acc[1] / iters);
        if (coarse_ms) *coarse_ms = static_cast<float>(acc[2] / iters);
        if (fine_ms) *fine_ms = static_cast<float>(acc[3] / iters);
    }
    (void)SyncAll(c);
    for (auto &v : tev)
        if (v) (void)hipEventDestroy(v);
    return r == PM_OK ? pm_sync(c) : r;
}

int pm_frame_latency(pm_ctx *c, int iters, float *median_ms, float *min_ms) {
    if (!c || iters <= 0 || iters > 4096) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r;
    if ((r = SyncAll(c)) != PM_OK) return r;
    std::vector<float> lat;
    for (int i = 0; i < iters; ++i) {
        // One frame exactly as pm_render submits it (three plain launches), nothing else in
        // flight, bracketed by two events on its stream: first kernel begin to last kernel end
        // (SURVEY 8d's t_frame).  Dispatches that carry their own timestamps
        // (pm_debug_frame_timeline) show the same kernels but stretch every gap between them
        // by ~3.5 us, so they are kept for the breakdown only.
        hipStream_t q = c->streams[c->frame % c->streams.size()];
        PM_TRY(hipEventRecord(c->ev[0], q));
        if ((r = Enqueue(c, nullptr, c->fb_stride, nullptr)) != PM_OK) return r;
        PM_TRY(hipEventRecord(c->ev[1], q));
        if ((r = SyncAll(c)) != PM_OK) return r;
        float t = 0;
        PM_TRY(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
        lat.push_back(t);
    }
    std::sort(lat.begin(), lat.end());
    if (median_ms) *median_ms = lat[lat.size() / 2];
    if (min_ms) *min_ms = lat.front();
    return pm_sync(c);
}

int pm_binning_info(pm_ctx *c, uint32_t out[3]) {
    if (!c || !out) return PM_ERR_INVALID;
    out[0] = c->frames_bin_wave;
    out[1] = c->frames_bin_wave_inflight;
    out[2] = c->frames_bin_no_chains;
    return PM_OK;
}

int pm_binning_plan_info(pm_ctx *c, uint32_t out[4]) {
    if (!c || !out) return PM_ERR_INVALID;
    out[0] = c->plan.n_sr_active();
    out[1] = c->plan.n_sr_split;
    out[2] = c->plans_fed_back;
    out[3] = c->plan.fb_applied ? 1u : 0u;
    return PM_OK;
}

int pm_tile_kernel_info(pm_ctx *c, uint32_t *dense_frames) {
    if (!c || !dense_frames) return PM_ERR_INVALID;
    *dense_frames = c->frames_dense_kernel;
    return PM_OK;
}

int pm_one_launch_info(pm_ctx *c, uint32_t *frames, int *applies) {
    if (!c) return PM_ERR_INVALID;
    if (frames) *frames = c->frames_one_launch;
    if (applies) {
        *applies = 0;
        if (c->d_scene && c->tiles_x != 0) {
            const int r = EnsureArena(c);
            if (r != PM_OK) return r;
            *applies = OneLaunchGrid(c) != 0u && !c->one_launch_broken && c->handout != 1 ? 1 : 0;
        }
    }
    return PM_OK;
}

int pm_time_one_launch(pm_ctx *c, int iters, float *kernel_ms) {
    if (!c || iters <= 0 || !kernel_ms) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r;
    if ((r = SyncAll(c)) != PM_OK) return r;
    double acc = 0;
    for (int i = 0; i < iters; ++i) {
        const int si = static_cast<int>(c->frame % c->slot.size());
        FrameSlot *s = &c->slot[si];
        pm::FrameParams p;
        if ((r = BuildParams(c, s, nullptr, c->fb_stride, &p)) != PM_OK) return r;
        const uint32_t grid = OneLaunchGrid(c);
        if (grid == 0u || c->one_launch_broken) return PM_ERR_INVALID;
        if ((r = EnsureFifo(c, s, c->stream)) != PM_OK) return r;
        p.fifo = s->d_fifo;
        p.fifo_cap = s->fifo_cap;
        p.one_launch = 3u;
        PM_TRY(ResetTileState(c, s, c->stream));
        pm::LaunchFrame(p, grid, c->stream, c->ev[0], c->ev[1]);
        PM_TRY(hipStreamSynchronize(c->stream));
        Submitted(c, si, p, c->stream);
        s->in_flight = false;
        float t = 0;
        PM_TRY(hipEventElapsedTime(&t, c->ev[0], c->ev[1]));
        acc += t;
    }
    *kernel_ms = static_cast<float>(acc / iters);
    return pm_sync(c);
}

int pm_debug_time_frame(pm_ctx *c, uint64_t *out, size_t max_wgs, size_t *n_wgs) {
    if (!c || !out) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r;
    if ((r = SyncAll(c)) != PM_OK) return r;
    const int si = static_cast<int>(c->frame % c->slot.size());
    FrameSlot *s = &c->slot[si];
    pm::FrameParams p;
    if ((r = BuildParams(c, s, nullptr, c->fb_stride, &p)) != PM_OK) return r;
    const uint32_t grid = OneLaunchGrid(c);
    if (n_wgs) *n_wgs = grid;
    if (grid == 0u || c->one_launch_broken) return PM_ERR_INVALID;
    if (grid > max_wgs) return PM_ERR_CAPACITY;
    if ((r = EnsureFifo(c, s, c->stream)) != PM_OK) return r;
    unsigned long long *d = nullptr;
    PM_TRY(hipMalloc(&d, static_cast<size_t>(grid) * 32 * sizeof(unsigned long long)));
    p.fifo = s->d_fifo;
    p.fifo_cap = s->fifo_cap;
    p.one_launch = 3u;
    p.dbg_time = d;
    hipError_t e = ResetTileState(c, s, c->stream);
    if (e == hipSuccess) {
        if (c->one_launch_split) {
            p.one_launch = 1u;
            pm::LaunchFrame(p, grid, c->stream);
            p.one_launch = 2u;
        }
        pm::LaunchFrame(p, grid, c->stream);
        e = hipStreamSynchronize(c->stream);
    }
    p.dbg_time = nullptr;
    Submitted(c, si, p, c->stream);
    s->in_flight = false;
    if (e == hipSuccess) e = hipMemcpy(out, d, static_cast<size_t>(grid) * 32 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return HipFail(e, "frame timeline");
    return pm_sync(c);
}

int pm_debug_frame_timeline(pm_ctx *c, int iters, float *out6) {
    if (!c || !out6 || iters <= 0 || iters > 4096) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r;
    if ((r = SyncAll(c)) != PM_OK) return r;
    hipEvent_t tev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (auto &v : tev)
        if (e == hipSuccess) e = hipEventCreate(&v);
    std::vector<float> col[6];
    r = e == hipSuccess ? PM_OK : HipFail(e, "hipEventCreate");
    for (int i = 0; i < iters && r == PM_OK; ++i) {
        r = Enqueue(c, nullptr, c->fb_stride, nullptr, tev);
        if (r == PM_OK) r = SyncAll(c);
        float v[6] = {0, 0, 0, 0, 0, 0};
        bool ok = r == PM_OK && hipEventElapsedTime(&v[0], tev[0], tev[1]) == hipSuccess &&
                  hipEventElapsedTime(&v[4], tev[6], tev[7]) == hipSuccess && hipEventElapsedTime(&v[5], tev[0], tev[7]) == hipSuccess;
        if (ok && c->fused)  // bin, gap, (no coarse launch), fine
            ok = hipEventElapsedTime(&v[1], tev[1], tev[6]) == hipSuccess;
        else if (ok)
            ok = hipEventElapsedTime(&v[1], tev[1], tev[4]) == hipSuccess && hipEventElapsedTime(&v[2], tev[4], tev[5]) == hipSuccess &&
                 hipEventElapsedTime(&v[3], tev[5], tev[6]) == hipSuccess;
        if (ok)
            for (int k = 0; k < 6; ++k) col[k].push_back(v[k]);
    }
    for (auto &v : tev)
        if (v) (void)hipEventDestroy(v);
    if (r != PM_OK) return r;
    if (col[0].empty()) return PM_ERR_HIP;
    for (int k = 0; k < 6; ++k) {
        std::sort(col[k].begin(), col[k].end());
        out6[k] = col[k][col[k].size() / 2];
    }
    return pm_sync(c);
}

int pm_get_stats(pm_ctx *c, pm_stats *out) {
    if (!c || !out) return PM_ERR_INVALID;
    std::memset(out, 0, sizeof(*out));
    PM_TRY(hipSetDevice(c->device));
    int r = SyncAll(c);
    if (r != PM_OK) return r;
    out->tiles_x = c->tiles_x;
    out->tiles_y = c->tiles_y;
    out->band_row0 = c->row0;
    out->band_row1 = c->row1;
    out->n_items = c->n_items;
    out->arena_cap_dwords = c->arena_cap;
    out->scene_bytes = static_cast<uint32_t>(c->user_scene_bytes);
    if (c->last_slot >= 0) {
        pm::Counters k;
        PM_TRY(hipMemcpy(&k, c->slot[c->last_slot].params.ctr_cur, sizeof(k), hipMemcpyDeviceToHost));
        for (uint32_t q = 0; q < pm::kClasses; ++q) {
            for (uint32_t sh = 0; sh < pm::kClassShards; ++sh) {
                out->queued_tiles += k.cls[sh].count[q];
                if (q < 3) out->heavy_tiles += k.cls[sh].count[q];  // (n_heavy_classes)
            }
        }
        out->arena_used_dwords = 0;
        for (uint32_t i = 0; i < pm::kArenaShards; ++i) out->arena_used_dwords += k.ptcl[i].bin_dwords;
        out->ptcl_used_cmds = 0;
        for (uint32_t i = 0; i < pm::kArenaShards; ++i) out->ptcl_used_cmds += k.ptcl[i].top;
        out->overflow = k.overflow;
    }
    return PM_OK;
}

int pm_get_scene_timings(pm_ctx *c, pm_scene_timings *out) {
    if (!c || !out) return PM_ERR_INVALID;
    out->flatten_encode_ms = c->t_flatten_ms;
    out->scene_index_ms = c->t_index_ms;
    out->arena_setup_ms = c->t_arena_ms;
    return PM_OK;
}

int pm_get_binning_plans(pm_ctx *c, uint32_t *plans) {
    if (!c || !plans) return PM_ERR_INVALID;
    *plans = c->plans_made;
    return PM_OK;
}

int pm_fill_coverage(pm_ctx *c, uint32_t item_ix, float *dst, size_t dst_stride_floats) {
    if (!c || !dst || dst_stride_floats < c->width) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r = pm_sync(c);
    if (r != PM_OK) return r;
    if (c->scene_bytes < 8 || item_ix >= c->n_items || c->tiles_x == 0) {
        SetError("pm_fill_coverage: no such item (or no scene / viewport)");
        return PM_ERR_INVALID;
    }
    const uint8_t *meta = c->item_meta.data();  // normal form: {n, 8 + 8n}{boxes}{items}
    const uint8_t *item = meta + 8 + 8ull * c->n_items + 32ull * item_ix;
    uint32_t tag;
    std::memcpy(&tag, item, 4);
    if ((tag & 0xffffu) != pm::kItemFill) {
        SetError("pm_fill_coverage: the item is not a Fill");
        return PM_ERR_INVALID;
    }
    // the item alone as a one-item group behind the resident bytes (its points stay where they are)
    const size_t root = (c->scene_bytes + 7u) & ~static_cast<size_t>(7u);
    uint8_t mini[8 + 8 + 32];
    const uint32_t hdr[2] = {1u, static_cast<uint32_t>(root + 16)};
    std::memcpy(mini, hdr, 8);
    std::memcpy(mini + 8, meta + 8 + 8ull * item_ix, 8);
    std::memcpy(mini + 16, item, 32);
    if (c->meta_colours_stale)  // (a repainted scene: the record with its colour of today)
        PM_TRY(hipMemcpy(mini + 16, c->d_scene + c->dev_items_ix + 32ull * item_ix, 32, hipMemcpyDeviceToHost));
    if (root + sizeof(mini) > c->dev_scene_cap) {
        r = ReserveDevice(c, root + sizeof(mini) + 4096, c->scene_bytes);
        if (r != PM_OK) return r;
    }
    PM_TRY(hipMemcpy(c->d_scene + root, mini, sizeof(mini), hipMemcpyHostToDevice));
    // swap the drawn group for the mini group, render bin + coarse (+ recorded solid colours),
    // run the coverage kernel, put everything back
    std::vector<uint8_t> saved_meta;
    saved_meta.swap(c->item_meta);
    const uint32_t saved_n = c->n_items, saved_bbox = c->dev_bbox_ix, saved_items = c->dev_items_ix;
    c->item_meta.assign(8 + 40, 0);
    const uint32_t mhdr[2] = {1u, 16u};
    std::memcpy(c->item_meta.data(), mhdr, 8);
    std::memcpy(c->item_meta.data() + 8, mini + 8, 40);
    c->n_items = 1;
    c->dev_bbox_ix = static_cast<uint32_t>(root + 8);
    c->dev_items_ix = static_cast<uint32_t>(root + 16);
    c->arena_dirty = true;
    const size_t tiles = static_cast<size_t>(BandRows(c)) * c->tiles_x;
    const size_t rows_px = std::min<size_t>(static_cast<size_t>(BandRows(c)) * pm::kTileH, c->height - c->row0 * pm::kTileH);
    uint32_t *d_counts = nullptr, *d_solid = nullptr;
    float *d_out = nullptr;
    int status = BuildSceneIndex(c);
    hipError_t e = hipSuccess;
    if (status == PM_OK) {
        e = hipMalloc(&d_counts, std::max<size_t>(tiles, 1) * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&d_solid, std::max<size_t>(tiles, 1) * sizeof(uint32_t));
        if (e == hipSuccess) e = hipMalloc(&d_out, static_cast<size_t>(BandRows(c)) * pm::kTileH * c->width * sizeof(float));
        if (e == hipSuccess) e = hipMemset(d_solid, 0, std::max<size_t>(tiles, 1) * sizeof(uint32_t));
    }
    if (status == PM_OK && e == hipSuccess) {
        const int si = static_cast<int>(c->frame % c->slot.size());
        FrameSlot *s = &c->slot[si];
        pm::FrameParams p;
        status = BuildParams(c, s, nullptr, c->fb_stride, &p);
        if (status == PM_OK) {
            p.dbg_counts = d_counts;
            p.dbg_solid = d_solid;
            p.dbg_cmds = nullptr;
            p.dbg_max = 0;
            (void)ResetTileState(c, s, c->stream);
            pm::LaunchBin(p, c->stream);
            pm::LaunchCoarse(p, CoarseGrid(c), true, c->stream);
            pm::LaunchCoverage(p, static_cast<uint32_t>(tiles), d_solid, d_out, c->width, c->stream);
            p.dbg_counts = p.dbg_solid = nullptr;
            Submitted(c, si, p, c->stream);
            e = hipStreamSynchronize(c->stream);
            if (e == hipSuccess)
                e = hipMemcpy2D(dst, dst_stride_floats * sizeof(float), d_out, static_cast<size_t>(c->width) * sizeof(float),
                                static_cast<size_t>(c->width) * sizeof(float), rows_px, hipMemcpyDeviceToHost);
            pm::Counters k;
            if (e == hipSuccess) e = hipMemcpy(&k, p.ctr_cur, sizeof(k), hipMemcpyDeviceToHost);
            if (e == hipSuccess && k.overflow) {
                SetError("pm_fill_coverage: command-list arena overflow");
                status = PM_ERR_CAPACITY;
            }
        }
    }
    if (d_counts) (void)hipFree(d_counts);
    if (d_solid) (void)hipFree(d_solid);
    if (d_out) (void)hipFree(d_out);
    // restore the scene
    c->item_meta.swap(saved_meta);
    c->n_items = saved_n;
    c->dev_bbox_ix = saved_bbox;
    c->dev_items_ix = saved_items;
    c->arena_dirty = true;
    c->last_slot = -1;
    const int rb = BuildSceneIndex(c);
    if (e != hipSuccess) return HipFail(e, "pm_fill_coverage");
    return status != PM_OK ? status : rb;
}

extern "C++" {
// ---- the queries' host scaffold (pm_query_common.h) ---------------------------------------------------------------------------
// (Templates: the block has C++ linkage inside the C interface.)  Every query call is: its check, QueryOrderBefore, its launches with a QueryView, QueryOrderBehind; a host-memory variant stages
// through QueryStaging and ends with a synchronisation of c->stream.
namespace {
constexpr size_t kHitLaunchMax = static_cast<size_t>(1) << 30;  // queries per launch (the kernels index them in 32 bits)
constexpr size_t kHitBatch = static_cast<size_t>(1) << 22;      // pm_hit_test, pm_hit_frame: queries staged on the device at a time (64 MiB)
constexpr size_t kRectBatch = static_cast<size_t>(1) << 20;     // pm_hit_rects, pm_snap, pm_snap_intersections: the same (24 to 60 MiB)
constexpr size_t kStackStageMax = kHitBatch * 16;               // pm_hit_stack, pm_hit_rects_stack: bytes staged at a time -- pm_hit_test's largest batch

static_assert(PM_HIT_SKIP_TRANSPARENT == pm::kHitSkipTransparent && PM_HIT_NONE == pm::kHitNone && PM_SEL_TOUCHES == pm::kSelTouches &&
                  PM_SEL_ENCLOSES == pm::kSelEncloses && PM_POLYGON_MAX_VERTICES == pm::kPolyMaxVertices,
              "pm_query_common.h's and pm_hit_poly.h's constants are the header's");
static_assert(PM_HIT_STOP_AT_OPAQUE == pm::kHitStopAtOpaque && PM_HIT_STACK_MAX == pm::kHitStackMax, "pm_hit_stack.h's constants are the header's");
static_assert(PM_COVERAGE_VISIBLE_ONLY == pm::kCoverageVisibleOnly && sizeof(pm_coverage) == 4 * pm::kCoverageWords, "pm_coverage.h's constants are the header's");
static_assert(PM_SNAP_VERTICES == pm::kSnapVertices && PM_SNAP_EDGES == pm::kSnapEdges && PM_SNAP_KIND_VERTEX == pm::kSnapKindVertex &&
                  PM_SNAP_KIND_EDGE == pm::kSnapKindEdge,
              "pm_snap.h's constants are the header's");
static_assert(PM_SNAP_MAX_NEAR_EDGES == pm::kCrossMaxNear && PM_SNAP_KIND_INTERSECTION == pm::kSnapKindIntersection && PM_SNAP_KIND_TOO_MANY == pm::kSnapKindTooMany,
              "pm_snap_cross.h's constants are the header's");

hipStream_t QueryStream(pm_ctx *c, void *hip_stream) { return hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream; }

int SceneResident(pm_ctx *c) {
    if (!c->d_scene || c->scene_bytes < 8) {  // (what pm_render says: BuildParams)
        SetError("no scene resident (pm_upload_scene / pm_flatten_and_encode first)");
        return PM_ERR_INVALID;
    }
    return PM_OK;
}

int HitCheck(pm_ctx *c, uint32_t flags) {
    if (flags & ~static_cast<uint32_t>(PM_HIT_SKIP_TRANSPARENT)) {
        SetError("pm_hit_test: unknown flag bits");
        return PM_ERR_INVALID;
    }
    return SceneResident(c);
}

// flags of a stack call: PM_HIT_STOP_AT_OPAQUE is theirs alone, the rest is HitCheck's
int StackCheck(pm_ctx *c, uint32_t k, uint32_t flags) {
    if (k == 0 || k > PM_HIT_STACK_MAX) {
        SetError("pm_hit_stack: 1 <= k <= PM_HIT_STACK_MAX");
        return PM_ERR_INVALID;
    }
    return HitCheck(c, flags & ~static_cast<uint32_t>(PM_HIT_STOP_AT_OPAQUE));
}

// What a kernel reads of the context: the scene and the scene index as they are now, and the call's flags
pm::SceneView QueryView(pm_ctx *c, uint32_t flags) {
    pm::SceneView v{};
    v.scene = c->d_scene;
    v.n_items = c->n_items;
    v.items_ix = c->dev_items_ix;
    v.bbox_ix = c->dev_bbox_ix;
    v.chunk_base = c->d_chunk_base;
    v.chunk_bbox = c->d_chunk_bbox;
    v.sup_bbox = c->d_sup_bbox;
    v.flags = flags;
    return v;
}

// The ordering rule of every query, for launches on q.  Before them: q waits for ev_scene unless it is c->stream (the scene's upload
// and index ran there), and for ev_hit if the queries submitted so far went to another stream (ONE event stands for every query
// submitted: when it moves to another stream, that stream first waits for what it stood for) ...
int QueryOrderBefore(pm_ctx *c, hipStream_t q) {
    if (q != c->stream) PM_TRY(hipStreamWaitEvent(q, c->ev_scene, 0));
    if (c->hit_pending && c->hit_stream != q) PM_TRY(hipStreamWaitEvent(q, c->ev_hit, 0));
    return PM_OK;
}
// ... and behind them ev_hit: whatever replaces the scene buffer or the scene index waits for it first (SyncAll)
int QueryOrderBehind(pm_ctx *c, hipStream_t q) {
    PM_TRY(hipGetLastError());
    PM_TRY(hipEventRecord(c->ev_hit, q));
    c->hit_stream = q;
    c->hit_pending = true;
    return PM_OK;
}

// c->d_stage holds `bytes` bytes, laid out by the call that asked.  Grow-only; nothing on c->stream uses the old buffer when it is freed.
hipError_t QueryStaging(pm_ctx *c, size_t bytes) {
    if (bytes <= c->stage_cap) return hipSuccess;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return e;
    if (c->d_stage) (void)hipFree(c->d_stage);
    c->d_stage = nullptr;
    c->stage_cap = 0;
    e = hipMalloc(&c->d_stage, bytes);
    if (e != hipSuccess) return e;
    c->stage_cap = bytes;
    return hipSuccess;
}

// Where a host-memory call's records go: `bytes` per query (host = nullptr: not asked for)
struct QueryOut {
    void *host;
    size_t bytes;
};

// n queries of in_bytes each in host memory, batch_max at a time through the staging buffer, laid out {out0, out1, queries, prefix}:
// the prefix (a call's per-item words) is uploaded once, then batch by batch the queries go up, enqueue(d_in, m, d_out0, d_out1,
// d_prefix) submits the m of them on c->stream, and the records come back.  d_out1 / d_prefix are nullptr if there is none.
template <typename Enqueue>
int QueryBatches(pm_ctx *c, const void *in, size_t in_bytes, size_t n, size_t batch_max, QueryOut out0, QueryOut out1, const void *prefix, size_t prefix_bytes,
                 Enqueue &&enqueue) {
    const size_t batch = std::min(n, batch_max);
    const size_t at_out1 = batch * out0.bytes, at_in = at_out1 + batch * out1.bytes, at_prefix = at_in + batch * in_bytes;
    PM_TRY(QueryStaging(c, at_prefix + prefix_bytes));
    uint8_t *d_out0 = c->d_stage, *d_out1 = out1.host ? c->d_stage + at_out1 : nullptr, *d_in = c->d_stage + at_in;
    uint8_t *d_prefix = prefix_bytes ? c->d_stage + at_prefix : nullptr;
    if (prefix_bytes) PM_TRY(hipMemcpyAsync(d_prefix, prefix, prefix_bytes, hipMemcpyHostToDevice, c->stream));
    for (size_t at = 0; at < n; at += batch) {
        const size_t m = std::min(batch, n - at);
        PM_TRY(hipMemcpyAsync(d_in, static_cast<const uint8_t *>(in) + at * in_bytes, m * in_bytes, hipMemcpyHostToDevice, c->stream));
        const int r = enqueue(d_in, m, d_out0, d_out1, d_prefix);
        if (r != PM_OK) return r;
        PM_TRY(hipMemcpyAsync(static_cast<uint8_t *>(out0.host) + at * out0.bytes, d_out0, m * out0.bytes, hipMemcpyDeviceToHost, c->stream));
        if (d_out1) PM_TRY(hipMemcpyAsync(static_cast<uint8_t *>(out1.host) + at * out1.bytes, d_out1, m * out1.bytes, hipMemcpyDeviceToHost, c->stream));
        PM_TRY(hipStreamSynchronize(c->stream));
    }
    return PM_OK;
}

// What pm_select_rect and pm_select_polygon do once the call's own arguments are checked: a word per item through the staging
// buffer -- enqueue(d_flags) submits on c->stream -- and the two counts
template <typename Enqueue>
int SelectToHost(pm_ctx *c, uint32_t *item_flags, size_t cap, uint32_t *n_touched, uint32_t *n_enclosed, Enqueue &&enqueue) {
    const size_t n = c->n_items;
    if (cap < n) return PM_ERR_CAPACITY;
    if (n != 0 && !item_flags) return PM_ERR_INVALID;
    if (n != 0) {
        PM_TRY(QueryStaging(c, n * 4));
        const int r = enqueue(reinterpret_cast<uint32_t *>(c->d_stage));
        if (r != PM_OK) return r;
        PM_TRY(hipMemcpyAsync(item_flags, c->d_stage, n * 4, hipMemcpyDeviceToHost, c->stream));
        PM_TRY(hipStreamSynchronize(c->stream));
    }
    uint32_t touched = 0, enclosed = 0;
    for (size_t i = 0; i < n; ++i) {
        touched += (item_flags[i] & PM_SEL_TOUCHES) ? 1u : 0u;
        enclosed += (item_flags[i] & PM_SEL_ENCLOSES) ? 1u : 0u;
    }
    if (n_touched) *n_touched = touched;
    if (n_enclosed) *n_enclosed = enclosed;
    return PM_OK;
}

static_assert(sizeof(pm_snap_result) == 32 && offsetof(pm_snap_result, item) == 0 && offsetof(pm_snap_result, kind) == 4 &&
                  offsetof(pm_snap_result, index) == 8 && offsetof(pm_snap_result, t) == 12 && offsetof(pm_snap_result, x) == 16 &&
                  offsetof(pm_snap_result, y) == 20 && offsetof(pm_snap_result, d2) == 24,
              "the record pm_snap_kernel writes");
static_assert(sizeof(pm_snap_cross_result) == 48 && offsetof(pm_snap_cross_result, item) == 0 && offsetof(pm_snap_cross_result, kind) == 4 &&
                  offsetof(pm_snap_cross_result, index) == 8 && offsetof(pm_snap_cross_result, t) == 12 && offsetof(pm_snap_cross_result, x) == 16 &&
                  offsetof(pm_snap_cross_result, y) == 20 && offsetof(pm_snap_cross_result, d2) == 24 && offsetof(pm_snap_cross_result, item2) == 32 &&
                  offsetof(pm_snap_cross_result, index2) == 36 && offsetof(pm_snap_cross_result, u) == 40 && offsetof(pm_snap_cross_result, n_near) == 44,
              "the record pm_cross_kernel writes");

// Everything a snapping call refuses, before anything is enqueued.  name: the call's; allowed: its flag bits; kinds: PM_SNAP_VERTICES |
// PM_SNAP_EDGES if it needs one of them, 0 if it has no such choice
int SnapCheck(pm_ctx *c, const char *name, uint32_t allowed, uint32_t kinds, const void *xyr, size_t n, uint32_t flags, const void *skip_items, size_t n_skip,
              const void *out) {
    auto refuse = [name](const char *why) {
        SetError(std::string(name) + why);
        return PM_ERR_INVALID;
    };
    if (flags & ~allowed) return refuse(": unknown flag bits");
    if (kinds && !(flags & kinds)) return refuse(": PM_SNAP_VERTICES, PM_SNAP_EDGES or both");
    const int r = SceneResident(c);
    if (r != PM_OK) return r;
    if (skip_items ? n_skip < c->n_items : n_skip != 0) return refuse(": skip_items holds one word per item, or is NULL with n_skip == 0");
    if (n != 0 && (!xyr || !out)) return refuse(": a NULL pointer with n != 0");
    return PM_OK;
}
constexpr uint32_t kSnapKinds = PM_SNAP_VERTICES | PM_SNAP_EDGES;

// The launches of either kernel for n queries in device memory, on q: their params differ in the record's size alone
template <typename Params>
int SnapEnqueue(pm_ctx *c, void (*launch)(const Params &, uint32_t, hipStream_t), size_t record, const float *d_xyr, size_t n, uint32_t flags,
                const uint32_t *d_skip, uint8_t *d_out, hipStream_t q) {
    int r = QueryOrderBefore(c, q);
    if (r != PM_OK) return r;
    Params p{};
    p.V = QueryView(c, flags);
    p.skip_items = d_skip;
    for (size_t at = 0; at < n; at += kHitLaunchMax) {
        p.xyr = d_xyr + 3 * at;
        p.out = d_out + record * at;
        p.n = static_cast<uint32_t>(std::min(n - at, kHitLaunchMax));
        launch(p, static_cast<uint32_t>(c->n_cus), q);
    }
    return QueryOrderBehind(c, q);
}

// The host-memory variant of either: {records, queries, skip words} through the staging buffer
template <typename Params>
int SnapToHost(pm_ctx *c, void (*launch)(const Params &, uint32_t, hipStream_t), size_t record, const float *xyr, size_t n, uint32_t flags,
               const uint32_t *skip_items, void *out) {
    return QueryBatches(c, xyr, 12, n, kRectBatch, {out, record}, {nullptr, 0}, skip_items, skip_items ? static_cast<size_t>(c->n_items) * 4 : 0,
                        [&](uint8_t *d_in, size_t m, uint8_t *d_out, uint8_t *, uint8_t *d_skip) {
                            return SnapEnqueue(c, launch, record, reinterpret_cast<float *>(d_in), m, flags, reinterpret_cast<uint32_t *>(d_skip), d_out, c->stream);
                        });
}
}  // namespace
}  // extern "C++"

// ---- point hit testing (pm_hit_kernel, pm_hit_test.h) ----------------------------------------------------------------
namespace {
// The launches for n queries in device memory, on q.  They read the scene buffer and the scene index as they are now.
int HitEnqueue(pm_ctx *c, const float *d_xy, size_t n, uint32_t flags, uint32_t *d_top, uint32_t *d_cnt, hipStream_t q) {
    int r = QueryOrderBefore(c, q);
    if (r != PM_OK) return r;
    pm::HitParams p{};
    p.V = QueryView(c, flags);
    for (size_t at = 0; at < n; at += kHitLaunchMax) {
        p.xy = d_xy + 2 * at;
        p.top_item = d_top + at;
        p.n_hit = d_cnt ? d_cnt + at : nullptr;
        p.n = static_cast<uint32_t>(std::min(n - at, kHitLaunchMax));
        pm::LaunchHitTest(p, static_cast<uint32_t>(c->n_cus), q);
    }
    return QueryOrderBehind(c, q);
}

// What both item-map calls refuse, before anything is enqueued
int HitFrameCheck(pm_ctx *c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t flags, const void *top_item, size_t stride) {
    const int r = HitCheck(c, flags);
    if (r != PM_OK) return r;
    if (static_cast<uint64_t>(x0) + w > 65536u || static_cast<uint64_t>(y0) + h > 65536u) {
        SetError("pm_hit_frame: the rectangle ends beyond pixel 65 535");
        return PM_ERR_INVALID;
    }
    if (stride < w) {
        SetError("pm_hit_frame: stride < w");
        return PM_ERR_INVALID;
    }
    if (w != 0 && h != 0 && !top_item) {
        SetError("pm_hit_frame: top_item is NULL");
        return PM_ERR_INVALID;
    }
    return PM_OK;
}

// The launch for a rectangle of pixels, on q
int HitFrameEnqueue(pm_ctx *c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t flags, uint32_t *d_top, uint32_t *d_cnt, size_t stride,
                    hipStream_t q) {
    int r = QueryOrderBefore(c, q);
    if (r != PM_OK) return r;
    pm::HitFrameParams p{};
    p.V = QueryView(c, flags);
    p.top_item = d_top;
    p.n_hit = d_cnt;
    p.stride = stride;
    p.x0 = x0;
    p.y0 = y0;
    p.w = w;
    p.h = h;
    pm::LaunchHitFrame(p, static_cast<uint32_t>(c->n_cus), q);
    return QueryOrderBehind(c, q);
}
}  // namespace

int pm_hit_test_device(pm_ctx *c, const void *dev_xy, size_t n, uint32_t flags, void *dev_top_item, void *dev_n_hit, void *hip_stream) {
    if (!c || (n != 0 && (!dev_xy || !dev_top_item))) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = HitCheck(c, flags);
    if (r != PM_OK || n == 0) return r;
    return HitEnqueue(c, static_cast<const float *>(dev_xy), n, flags, static_cast<uint32_t *>(dev_top_item), static_cast<uint32_t *>(dev_n_hit),
                      QueryStream(c, hip_stream));
}

int pm_hit_test(pm_ctx *c, const float *xy, size_t n, uint32_t flags, uint32_t *top_item, uint32_t *n_hit) {
    if (!c || (n != 0 && (!xy || !top_item))) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = HitCheck(c, flags);
    if (r != PM_OK || n == 0) return r;
    return QueryBatches(c, xy, 8, n, kHitBatch, {top_item, 4}, {n_hit, 4}, nullptr, 0, [&](uint8_t *d_in, size_t m, uint8_t *d_top, uint8_t *d_cnt, uint8_t *) {
        return HitEnqueue(c, reinterpret_cast<float *>(d_in), m, flags, reinterpret_cast<uint32_t *>(d_top), reinterpret_cast<uint32_t *>(d_cnt), c->stream);
    });
}

// ---- the item map (pm_hit_frame_kernel, pm_hit_frame.h) -----------------------------------------------------------------
int pm_hit_frame_device(pm_ctx *c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t flags, void *dev_top_item, void *dev_n_hit, size_t stride,
                        void *hip_stream) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = HitFrameCheck(c, x0, y0, w, h, flags, dev_top_item, stride);
    if (r != PM_OK || w == 0 || h == 0) return r;
    return HitFrameEnqueue(c, x0, y0, w, h, flags, static_cast<uint32_t *>(dev_top_item), static_cast<uint32_t *>(dev_n_hit), stride, QueryStream(c, hip_stream));
}

int pm_hit_frame(pm_ctx *c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t flags, uint32_t *top_item, uint32_t *n_hit, size_t stride) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r = HitFrameCheck(c, x0, y0, w, h, flags, top_item, stride);
    if (r != PM_OK || w == 0 || h == 0) return r;
    // batches of whole rows, dense on the device (a multiple of the tile's height, so that a batch's tiles are the rectangle's): {top_item, n_hit}
    const size_t rows = std::min<size_t>(h, std::max<size_t>(kHitBatch / w / 16, 1) * 16);
    PM_TRY(QueryStaging(c, rows * w * 8));
    uint32_t *d_top = reinterpret_cast<uint32_t *>(c->d_stage);
    uint32_t *d_cnt = n_hit ? d_top + rows * w : nullptr;
    for (size_t at = 0; at < h; at += rows) {
        const size_t m = std::min<size_t>(rows, h - at);
        r = HitFrameEnqueue(c, x0, y0 + static_cast<uint32_t>(at), w, static_cast<uint32_t>(m), flags, d_top, d_cnt, w, c->stream);
        if (r != PM_OK) return r;
        PM_TRY(hipStreamSynchronize(c->stream));
        PM_TRY(hipMemcpy2D(top_item + at * stride, stride * 4, d_top, static_cast<size_t>(w) * 4, static_cast<size_t>(w) * 4, m, hipMemcpyDeviceToHost));
        if (n_hit) PM_TRY(hipMemcpy2D(n_hit + at * stride, stride * 4, d_cnt, static_cast<size_t>(w) * 4, static_cast<size_t>(w) * 4, m, hipMemcpyDeviceToHost));
    }
    return PM_OK;
}

// ---- coverage counts (pm_item_coverage_kernel, pm_coverage.h; decision D28) ------------------------------------------------------
namespace {
static_assert(sizeof(pm_coverage) == 16 && offsetof(pm_coverage, covered) == 0 && offsetof(pm_coverage, visible) == 4 && offsetof(pm_coverage, top) == 8 &&
                  offsetof(pm_coverage, first_visible) == 12,
              "the record pm_item_coverage_kernel writes");

// What both coverage calls refuse about the flags, the scene and the rectangle, before anything is enqueued
int CoverageCheck(pm_ctx *c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t flags) {
    if (flags & ~static_cast<uint32_t>(PM_HIT_SKIP_TRANSPARENT | PM_COVERAGE_VISIBLE_ONLY)) {
        SetError("pm_item_coverage: unknown flag bits");
        return PM_ERR_INVALID;
    }
    const int r = SceneResident(c);
    if (r != PM_OK) return r;
    if (static_cast<uint64_t>(x0) + w > 65536u || static_cast<uint64_t>(y0) + h > 65536u) {
        SetError("pm_item_coverage: the rectangle ends beyond pixel 65 535");
        return PM_ERR_INVALID;
    }
    if (static_cast<uint64_t>(w) * h > 0xffffffffull) {
        SetError("pm_item_coverage: more than 2^32 - 1 pixels (the counts are 32-bit)");
        return PM_ERR_INVALID;
    }
    return PM_OK;
}

// The launches for a rectangle of pixels, on q: the records' initial value, then the tiles
int CoverageEnqueue(pm_ctx *c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t flags, uint32_t *d_out, hipStream_t q) {
    int r = QueryOrderBefore(c, q);
    if (r != PM_OK) return r;
    pm::CoverageParams p{};
    p.V = QueryView(c, flags);
    p.out = d_out;
    p.x0 = x0;
    p.y0 = y0;
    p.w = w;
    p.h = h;
    pm::LaunchItemCoverage(p, static_cast<uint32_t>(c->n_cus), q);
    return QueryOrderBehind(c, q);
}
}  // namespace

int pm_item_coverage_device(pm_ctx *c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t flags, void *dev_out, size_t cap, void *hip_stream) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = CoverageCheck(c, x0, y0, w, h, flags);
    if (r != PM_OK) return r;
    if (cap < c->n_items) return PM_ERR_CAPACITY;
    if (c->n_items == 0) return PM_OK;
    if (!dev_out || (reinterpret_cast<uintptr_t>(dev_out) & 3u) != 0) {
        SetError("pm_item_coverage_device: dev_out is NULL or not 4-byte aligned");
        return PM_ERR_INVALID;
    }
    return CoverageEnqueue(c, x0, y0, w, h, flags, static_cast<uint32_t *>(dev_out), QueryStream(c, hip_stream));
}

int pm_item_coverage(pm_ctx *c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t flags, pm_coverage *out, size_t cap, uint32_t *n_items) {
    if (!c) return PM_ERR_INVALID;
    if (n_items) *n_items = c->scene_bytes >= 8 ? c->n_items : 0u;
    PM_TRY(hipSetDevice(c->device));
    int r = CoverageCheck(c, x0, y0, w, h, flags);
    if (r != PM_OK) return r;
    const size_t n = c->n_items;
    if (cap < n) return PM_ERR_CAPACITY;
    if (n == 0) return PM_OK;
    if (!out) {
        SetError("pm_item_coverage: out is NULL");
        return PM_ERR_INVALID;
    }
    PM_TRY(QueryStaging(c, n * sizeof(pm_coverage)));
    r = CoverageEnqueue(c, x0, y0, w, h, flags, reinterpret_cast<uint32_t *>(c->d_stage), c->stream);
    if (r != PM_OK) return r;
    PM_TRY(hipMemcpyAsync(out, c->d_stage, n * sizeof(pm_coverage), hipMemcpyDeviceToHost, c->stream));
    PM_TRY(hipStreamSynchronize(c->stream));
    return PM_OK;
}

// ---- rectangle queries (pm_hit_rects_kernel, pm_select_rect_kernel, pm_hit_rect.h; decision D19) ---------------------------
namespace {
int HitRectsEnqueue(pm_ctx *c, const float *d_rects, size_t n, uint32_t flags, uint32_t *d_top, uint32_t *d_cnt, hipStream_t q) {
    int r = QueryOrderBefore(c, q);
    if (r != PM_OK) return r;
    pm::HitRectParams p{};
    p.V = QueryView(c, flags);
    for (size_t at = 0; at < n; at += kHitLaunchMax) {
        p.rects = d_rects + 4 * at;
        p.top_item = d_top + at;
        p.n_hit = d_cnt ? d_cnt + at : nullptr;
        p.n = static_cast<uint32_t>(std::min(n - at, kHitLaunchMax));
        pm::LaunchHitRects(p, static_cast<uint32_t>(c->n_cus), q);
    }
    return QueryOrderBehind(c, q);
}

int SelectRectEnqueue(pm_ctx *c, const float rect[4], uint32_t flags, uint32_t *d_flags, hipStream_t q) {
    int r = QueryOrderBefore(c, q);
    if (r != PM_OK) return r;
    pm::SelectRectParams p{};
    p.V = QueryView(c, flags);
    std::memcpy(p.rect, rect, sizeof(p.rect));
    p.item_flags = d_flags;
    pm::LaunchSelectRect(p, static_cast<uint32_t>(c->n_cus), q);
    return QueryOrderBehind(c, q);
}
}  // namespace

int pm_hit_rects_device(pm_ctx *c, const void *dev_rects, size_t n, uint32_t flags, void *dev_top_item, void *dev_n_hit, void *hip_stream) {
    if (!c || (n != 0 && (!dev_rects || !dev_top_item))) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = HitCheck(c, flags);
    if (r != PM_OK || n == 0) return r;
    return HitRectsEnqueue(c, static_cast<const float *>(dev_rects), n, flags, static_cast<uint32_t *>(dev_top_item), static_cast<uint32_t *>(dev_n_hit),
                           QueryStream(c, hip_stream));
}

int pm_hit_rects(pm_ctx *c, const float *rects, size_t n, uint32_t flags, uint32_t *top_item, uint32_t *n_hit) {
    if (!c || (n != 0 && (!rects || !top_item))) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = HitCheck(c, flags);
    if (r != PM_OK || n == 0) return r;
    return QueryBatches(c, rects, 16, n, kRectBatch, {top_item, 4}, {n_hit, 4}, nullptr, 0, [&](uint8_t *d_in, size_t m, uint8_t *d_top, uint8_t *d_cnt, uint8_t *) {
        return HitRectsEnqueue(c, reinterpret_cast<float *>(d_in), m, flags, reinterpret_cast<uint32_t *>(d_top), reinterpret_cast<uint32_t *>(d_cnt), c->stream);
    });
}

int pm_select_rect_device(pm_ctx *c, const float rect[4], uint32_t flags, void *dev_item_flags, size_t cap, void *hip_stream) {
    if (!c || !rect) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = HitCheck(c, flags);
    if (r != PM_OK) return r;
    if (cap < c->n_items) return PM_ERR_CAPACITY;
    if (c->n_items == 0) return PM_OK;
    if (!dev_item_flags) return PM_ERR_INVALID;
    return SelectRectEnqueue(c, rect, flags, static_cast<uint32_t *>(dev_item_flags), QueryStream(c, hip_stream));
}

int pm_select_rect(pm_ctx *c, const float rect[4], uint32_t flags, uint32_t *item_flags, size_t cap, uint32_t *n_items, uint32_t *n_touched,
                   uint32_t *n_enclosed) {
    if (!c) return PM_ERR_INVALID;
    if (n_items) *n_items = c->scene_bytes >= 8 ? c->n_items : 0u;
    if (!rect) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = HitCheck(c, flags);
    if (r != PM_OK) return r;
    return SelectToHost(c, item_flags, cap, n_touched, n_enclosed, [&](uint32_t *d_flags) { return SelectRectEnqueue(c, rect, flags, d_flags, c->stream); });
}

// ---- hit stacks (pm_hit_stack_kernel, pm_hit_rects_stack_kernel, pm_hit_stack.h; decision D24) ------------------------------
extern "C++" {
namespace {
// The launches of either kernel for n queries of `in_floats` floats in device memory, on q: their params differ in the input's name alone
template <typename Params>
int StackEnqueue(pm_ctx *c, void (*launch)(const Params &, uint32_t, hipStream_t), const float *Params::*in, size_t in_floats, const float *d_in, size_t n,
                 uint32_t k, uint32_t flags, uint32_t *d_items, uint32_t *d_cnt, hipStream_t q) {
    int r = QueryOrderBefore(c, q);
    if (r != PM_OK) return r;
    Params p{};
    p.V = QueryView(c, flags);
    p.k = k;
    for (size_t at = 0; at < n; at += kHitLaunchMax) {
        p.*in = d_in + in_floats * at;
        p.items = d_items + at * k;
        p.n_hit = d_cnt ? d_cnt + at : nullptr;
        p.n = static_cast<uint32_t>(std::min(n - at, kHitLaunchMax));
        launch(p, static_cast<uint32_t>(c->n_cus), q);
    }
    return QueryOrderBehind(c, q);
}

// The host-memory variant of either: {items, counts, queries} through the staging buffer, as many queries to a batch as kStackStageMax holds
template <typename Params>
int StackToHost(pm_ctx *c, void (*launch)(const Params &, uint32_t, hipStream_t), const float *Params::*in, size_t in_floats, const float *h_in, size_t n,
                uint32_t k, uint32_t flags, uint32_t *items, uint32_t *n_hit) {
    const size_t record = static_cast<size_t>(k) * 4;
    return QueryBatches(c, h_in, in_floats * 4, n, kStackStageMax / (record + 4 + in_floats * 4), {items, record}, {n_hit, 4}, nullptr, 0,
                        [&](uint8_t *d_in, size_t m, uint8_t *d_items, uint8_t *d_cnt, uint8_t *) {
                            return StackEnqueue(c, launch, in, in_floats, reinterpret_cast<float *>(d_in), m, k, flags, reinterpret_cast<uint32_t *>(d_items),
                                                reinterpret_cast<uint32_t *>(d_cnt), c->stream);
                        });
}
}  // namespace
}  // extern "C++"

int pm_hit_stack_device(pm_ctx *c, const void *dev_xy, size_t n, uint32_t k, uint32_t flags, void *dev_items, void *dev_n_hit, void *hip_stream) {
    if (!c || (n != 0 && (!dev_xy || !dev_items))) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = StackCheck(c, k, flags);
    if (r != PM_OK || n == 0) return r;
    return StackEnqueue(c, pm::LaunchHitStack, &pm::HitStackParams::xy, 2, static_cast<const float *>(dev_xy), n, k, flags, static_cast<uint32_t *>(dev_items),
                        static_cast<uint32_t *>(dev_n_hit), QueryStream(c, hip_stream));
}

int pm_hit_stack(pm_ctx *c, const float *xy, size_t n, uint32_t k, uint32_t flags, uint32_t *items, uint32_t *n_hit) {
    if (!c || (n != 0 && (!xy || !items))) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = StackCheck(c, k, flags);
    if (r != PM_OK || n == 0) return r;
    return StackToHost(c, pm::LaunchHitStack, &pm::HitStackParams::xy, 2, xy, n, k, flags, items, n_hit);
}

int pm_hit_rects_stack_device(pm_ctx *c, const void *dev_rects, size_t n, uint32_t k, uint32_t flags, void *dev_items, void *dev_n_hit, void *hip_stream) {
    if (!c || (n != 0 && (!dev_rects || !dev_items))) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = StackCheck(c, k, flags);
    if (r != PM_OK || n == 0) return r;
    return StackEnqueue(c, pm::LaunchHitRectsStack, &pm::HitRectStackParams::rects, 4, static_cast<const float *>(dev_rects), n, k, flags,
                        static_cast<uint32_t *>(dev_items), static_cast<uint32_t *>(dev_n_hit), QueryStream(c, hip_stream));
}

int pm_hit_rects_stack(pm_ctx *c, const float *rects, size_t n, uint32_t k, uint32_t flags, uint32_t *items, uint32_t *n_hit) {
    if (!c || (n != 0 && (!rects || !items))) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = StackCheck(c, k, flags);
    if (r != PM_OK || n == 0) return r;
    return StackToHost(c, pm::LaunchHitRectsStack, &pm::HitRectStackParams::rects, 4, rects, n, k, flags, items, n_hit);
}

// ---- polygon queries (pm_select_polygon_kernel, pm_hit_poly.h; decision D20) -------------------------------------------------
namespace {
constexpr size_t kPolyVertBytes = static_cast<size_t>(PM_POLYGON_MAX_VERTICES) * 8;
constexpr size_t kPolyBytes = kPolyVertBytes + PM_POLYGON_MAX_VERTICES / pm::kPolyGroup * 16;   // the vertices, then a box per group of edges

// The ring's buffers, made once at the first polygon query
hipError_t PolyRing(pm_ctx *c) {
    for (int k = 0; k < pm_ctx::kPolySlots; ++k) {
        hipError_t e;
        if (!c->h_poly[k] && (e = hipHostMalloc(reinterpret_cast<void **>(&c->h_poly[k]), kPolyBytes)) != hipSuccess) return e;
        if (!c->d_poly[k] && (e = hipMalloc(reinterpret_cast<void **>(&c->d_poly[k]), kPolyBytes)) != hipSuccess) return e;
        if (!c->ev_poly[k] && (e = hipEventCreateWithFlags(&c->ev_poly[k], hipEventDisableTiming)) != hipSuccess) return e;
    }
    return hipSuccess;
}

// flags of a polygon call: PM_SEL_EVEN_ODD is theirs alone, the rest is HitCheck's
int PolyCheck(pm_ctx *c, const float *xy, size_t m, uint32_t flags) {
    if (!xy || m < 3 || m > PM_POLYGON_MAX_VERTICES) {
        SetError("pm_select_polygon: 3 .. PM_POLYGON_MAX_VERTICES vertices");
        return PM_ERR_INVALID;
    }
    return HitCheck(c, flags & ~static_cast<uint32_t>(PM_SEL_EVEN_ODD));
}

// The launch for a polygon in host memory, on q.  The vertices have left xy when this returns: they are in the slot's pinned
// buffer, which nothing writes again before the event behind this call's kernel has passed.
int SelectPolygonEnqueue(pm_ctx *c, const float *xy, size_t m, uint32_t flags, uint32_t *d_flags, hipStream_t q) {
    constexpr size_t kGroup = pm::kPolyGroup;
    PM_TRY(PolyRing(c));
    const uint32_t slot = c->poly_next;
    c->poly_next = (slot + 1u) % pm_ctx::kPolySlots;
    if (c->poly_used[slot]) PM_TRY(hipEventSynchronize(c->ev_poly[slot]));
    std::memcpy(c->h_poly[slot], xy, m * 8);
    float *gb = c->h_poly[slot] + kPolyVertBytes / 4;
    const size_t n_groups = (m + kGroup - 1) / kGroup;
    for (size_t g = 0; g < n_groups; ++g) {   // the ends of edges g * 16 ..: vertices g * 16 .. one past the group's last, mod m
        float *b = gb + 4 * g;
        b[0] = b[2] = xy[2 * (g * kGroup)];
        b[1] = b[3] = xy[2 * (g * kGroup) + 1];
        for (size_t j = g * kGroup; j <= std::min((g + 1) * kGroup, m); ++j) {
            const float x = xy[2 * (j % m)], y = xy[2 * (j % m) + 1];
            b[0] = std::min(b[0], x);
            b[1] = std::min(b[1], y);
            b[2] = std::max(b[2], x);
            b[3] = std::max(b[3], y);
        }
    }
    pm::HitPolyParams p{};
    p.V = QueryView(c, flags & static_cast<uint32_t>(PM_HIT_SKIP_TRANSPARENT));
    p.verts = c->d_poly[slot];
    p.boxes = c->d_poly[slot] + kPolyVertBytes / 4;
    p.m = static_cast<uint32_t>(m);
    p.even_odd = (flags & PM_SEL_EVEN_ODD) ? 1u : 0u;
    p.valid = 1u;
    p.box[0] = p.box[2] = xy[0];
    p.box[1] = p.box[3] = xy[1];
    for (size_t j = 0; j < m; ++j) {
        const float x = xy[2 * j], y = xy[2 * j + 1];
        if (!std::isfinite(x) || !std::isfinite(y)) p.valid = 0u;
        p.box[0] = std::min(p.box[0], x);
        p.box[1] = std::min(p.box[1], y);
        p.box[2] = std::max(p.box[2], x);
        p.box[3] = std::max(p.box[3], y);
    }
    p.item_flags = d_flags;
    int r = QueryOrderBefore(c, q);
    if (r != PM_OK) return r;
    PM_TRY(hipMemcpyAsync(c->d_poly[slot], c->h_poly[slot], m * 8, hipMemcpyHostToDevice, q));
    PM_TRY(hipMemcpyAsync(c->d_poly[slot] + kPolyVertBytes / 4, gb, n_groups * 16, hipMemcpyHostToDevice, q));
    pm::LaunchSelectPolygon(p, static_cast<uint32_t>(c->n_cus), q);
    r = QueryOrderBehind(c, q);
    if (r != PM_OK) return r;
    PM_TRY(hipEventRecord(c->ev_poly[slot], q));
    c->poly_used[slot] = true;
    return PM_OK;
}
}  // namespace

int pm_select_polygon_device(pm_ctx *c, const float *xy, size_t m, uint32_t flags, void *dev_item_flags, size_t cap, void *hip_stream) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = PolyCheck(c, xy, m, flags);
    if (r != PM_OK) return r;
    if (cap < c->n_items) return PM_ERR_CAPACITY;
    if (c->n_items == 0) return PM_OK;
    if (!dev_item_flags) return PM_ERR_INVALID;
    return SelectPolygonEnqueue(c, xy, m, flags, static_cast<uint32_t *>(dev_item_flags), QueryStream(c, hip_stream));
}

int pm_select_polygon(pm_ctx *c, const float *xy, size_t m, uint32_t flags, uint32_t *item_flags, size_t cap, uint32_t *n_items, uint32_t *n_touched,
                      uint32_t *n_enclosed) {
    if (!c) return PM_ERR_INVALID;
    if (n_items) *n_items = c->scene_bytes >= 8 ? c->n_items : 0u;
    PM_TRY(hipSetDevice(c->device));
    const int r = PolyCheck(c, xy, m, flags);
    if (r != PM_OK) return r;
    return SelectToHost(c, item_flags, cap, n_touched, n_enclosed, [&](uint32_t *d_flags) { return SelectPolygonEnqueue(c, xy, m, flags, d_flags, c->stream); });
}

// ---- snapping (pm_snap_kernel, pm_snap.h; decision D21) and snapping to intersections (pm_cross_kernel, pm_snap_cross.h; D23) ----------
int pm_snap_device(pm_ctx *c, const void *dev_xyr, size_t n, uint32_t flags, const void *dev_skip_items, size_t n_skip, void *dev_out, void *hip_stream) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = SnapCheck(c, "pm_snap", PM_HIT_SKIP_TRANSPARENT | kSnapKinds, kSnapKinds, dev_xyr, n, flags, dev_skip_items, n_skip, dev_out);
    if (r != PM_OK || n == 0) return r;
    return SnapEnqueue(c, pm::LaunchSnap, sizeof(pm_snap_result), static_cast<const float *>(dev_xyr), n, flags, static_cast<const uint32_t *>(dev_skip_items),
                       static_cast<uint8_t *>(dev_out), QueryStream(c, hip_stream));
}

int pm_snap(pm_ctx *c, const float *xyr, size_t n, uint32_t flags, const uint32_t *skip_items, size_t n_skip, pm_snap_result *out) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = SnapCheck(c, "pm_snap", PM_HIT_SKIP_TRANSPARENT | kSnapKinds, kSnapKinds, xyr, n, flags, skip_items, n_skip, out);
    if (r != PM_OK || n == 0) return r;
    return SnapToHost(c, pm::LaunchSnap, sizeof(*out), xyr, n, flags, skip_items, out);
}

int pm_snap_intersections_device(pm_ctx *c, const void *dev_xyr, size_t n, uint32_t flags, const void *dev_skip_items, size_t n_skip, void *dev_out,
                                 void *hip_stream) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = SnapCheck(c, "pm_snap_intersections", PM_HIT_SKIP_TRANSPARENT, 0u, dev_xyr, n, flags, dev_skip_items, n_skip, dev_out);
    if (r != PM_OK || n == 0) return r;
    return SnapEnqueue(c, pm::LaunchCross, sizeof(pm_snap_cross_result), static_cast<const float *>(dev_xyr), n, flags,
                       static_cast<const uint32_t *>(dev_skip_items), static_cast<uint8_t *>(dev_out), QueryStream(c, hip_stream));
}

int pm_snap_intersections(pm_ctx *c, const float *xyr, size_t n, uint32_t flags, const uint32_t *skip_items, size_t n_skip, pm_snap_cross_result *out) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = SnapCheck(c, "pm_snap_intersections", PM_HIT_SKIP_TRANSPARENT, 0u, xyr, n, flags, skip_items, n_skip, out);
    if (r != PM_OK || n == 0) return r;
    return SnapToHost(c, pm::LaunchCross, sizeof(*out), xyr, n, flags, skip_items, out);
}

// ---- bounds (pm_item_bounds_kernel, pm_union_bounds_kernel, pm_bounds.h; decision D22) ---------------------------------------------
namespace {
static_assert(sizeof(pm_bounds) == 32 && sizeof(pm_label_bounds) == 40 && offsetof(pm_label_bounds, n_items) == 32 && offsetof(pm_label_bounds, n_boxed) == 36,
              "the records the bounds kernels write");

// Everything pm_union_bounds / pm_union_bounds_device refuse (HitCheck's part first), before anything is enqueued
int UnionBoundsCheck(pm_ctx *c, uint32_t flags, const void *item_words, size_t n_words, uint32_t word_mask, const void *label_of_item, size_t n_label_words,
                     uint32_t n_labels, const void *out) {
    const int r = HitCheck(c, flags);
    if (r != PM_OK) return r;
    if (n_labels == 0) {
        SetError("pm_union_bounds: n_labels == 0");
        return PM_ERR_INVALID;
    }
    if (item_words && (n_words < c->n_items || word_mask == 0)) {
        SetError("pm_union_bounds: item_words holds one word per item and word_mask selects a bit of them, or item_words is NULL");
        return PM_ERR_INVALID;
    }
    if (label_of_item && n_label_words < c->n_items) {
        SetError("pm_union_bounds: label_of_item holds one label per item, or is NULL");
        return PM_ERR_INVALID;
    }
    if (!out || (reinterpret_cast<uintptr_t>(out) & 7u) != 0) {
        SetError("pm_union_bounds: out is NULL or not 8-byte aligned");
        return PM_ERR_INVALID;
    }
    return PM_OK;
}

int ItemBoundsEnqueue(pm_ctx *c, uint32_t flags, uint8_t *d_out, hipStream_t q) {
    int r = QueryOrderBefore(c, q);
    if (r != PM_OK) return r;
    pm::BoundsParams p{};
    p.V = QueryView(c, flags);
    p.out = d_out;
    pm::LaunchItemBounds(p, static_cast<uint32_t>(c->n_cus), q);
    return QueryOrderBehind(c, q);
}

int UnionBoundsEnqueue(pm_ctx *c, uint32_t flags, const uint32_t *d_words, uint32_t word_mask, const uint32_t *d_labels, uint32_t n_labels, uint8_t *d_out,
                       hipStream_t q) {
    int r = QueryOrderBefore(c, q);
    if (r != PM_OK) return r;
    pm::BoundsParams p{};
    p.V = QueryView(c, flags);
    p.item_words = d_words;
    p.word_mask = word_mask;
    p.label_of_item = d_labels;
    p.n_labels = n_labels;
    p.out = d_out;
    pm::LaunchUnionBounds(p, static_cast<uint32_t>(c->n_cus), q);
    return QueryOrderBehind(c, q);
}
}  // namespace

int pm_item_bounds_device(pm_ctx *c, uint32_t flags, void *dev_out, size_t cap, void *hip_stream) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = HitCheck(c, flags);
    if (r != PM_OK) return r;
    if (cap < c->n_items) return PM_ERR_CAPACITY;
    if (c->n_items == 0) return PM_OK;
    if (!dev_out || (reinterpret_cast<uintptr_t>(dev_out) & 7u) != 0) {
        SetError("pm_item_bounds_device: dev_out is NULL or not 8-byte aligned");
        return PM_ERR_INVALID;
    }
    return ItemBoundsEnqueue(c, flags, static_cast<uint8_t *>(dev_out), QueryStream(c, hip_stream));
}

int pm_item_bounds(pm_ctx *c, uint32_t flags, pm_bounds *out, size_t cap, uint32_t *n_items) {
    if (!c) return PM_ERR_INVALID;
    if (n_items) *n_items = c->scene_bytes >= 8 ? c->n_items : 0u;
    PM_TRY(hipSetDevice(c->device));
    int r = HitCheck(c, flags);
    if (r != PM_OK) return r;
    const size_t n = c->n_items;
    if (cap < n) return PM_ERR_CAPACITY;
    if (n == 0) return PM_OK;
    if (!out) {
        SetError("pm_item_bounds: out is NULL");
        return PM_ERR_INVALID;
    }
    PM_TRY(QueryStaging(c, n * sizeof(pm_bounds)));
    r = ItemBoundsEnqueue(c, flags, c->d_stage, c->stream);
    if (r != PM_OK) return r;
    PM_TRY(hipMemcpyAsync(out, c->d_stage, n * sizeof(pm_bounds), hipMemcpyDeviceToHost, c->stream));
    PM_TRY(hipStreamSynchronize(c->stream));
    return PM_OK;
}

int pm_union_bounds_device(pm_ctx *c, uint32_t flags, const void *dev_item_words, size_t n_words, uint32_t word_mask, const void *dev_label_of_item,
                           size_t n_label_words, uint32_t n_labels, void *dev_out, void *hip_stream) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = UnionBoundsCheck(c, flags, dev_item_words, n_words, word_mask, dev_label_of_item, n_label_words, n_labels, dev_out);
    if (r != PM_OK) return r;
    return UnionBoundsEnqueue(c, flags, static_cast<const uint32_t *>(dev_item_words), word_mask, static_cast<const uint32_t *>(dev_label_of_item), n_labels,
                              static_cast<uint8_t *>(dev_out), QueryStream(c, hip_stream));
}

int pm_union_bounds(pm_ctx *c, uint32_t flags, const uint32_t *item_words, size_t n_words, uint32_t word_mask, const uint32_t *label_of_item,
                    size_t n_label_words, uint32_t n_labels, pm_label_bounds *out) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r = UnionBoundsCheck(c, flags, item_words, n_words, word_mask, label_of_item, n_label_words, n_labels, out);
    if (r != PM_OK) return r;
    // {records, words, labels}
    const size_t n = c->n_items, out_bytes = static_cast<size_t>(n_labels) * sizeof(pm_label_bounds);
    PM_TRY(QueryStaging(c, out_bytes + (item_words ? n * 4 : 0) + (label_of_item ? n * 4 : 0)));
    uint8_t *d_out = c->d_stage;
    uint32_t *d_words = item_words ? reinterpret_cast<uint32_t *>(c->d_stage + out_bytes) : nullptr;
    uint32_t *d_labels = label_of_item ? reinterpret_cast<uint32_t *>(c->d_stage + out_bytes + (item_words ? n * 4 : 0)) : nullptr;
    if (d_words && n) PM_TRY(hipMemcpyAsync(d_words, item_words, n * 4, hipMemcpyHostToDevice, c->stream));
    if (d_labels && n) PM_TRY(hipMemcpyAsync(d_labels, label_of_item, n * 4, hipMemcpyHostToDevice, c->stream));
    r = UnionBoundsEnqueue(c, flags, d_words, word_mask, d_labels, n_labels, d_out, c->stream);
    if (r != PM_OK) return r;
    PM_TRY(hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, c->stream));
    PM_TRY(hipStreamSynchronize(c->stream));
    return PM_OK;
}

// ---- path measurement (pm_measure.h; decision D25) ----------------------------------------------------------------------------------
namespace {
static_assert(PM_MEASURE_NONE == pm::kMeasureNone && PM_MEASURE_OPEN == pm::kMeasureOpen && PM_MEASURE_CLOSED == pm::kMeasureClosed &&
                  PM_MEASURE_FOUND == pm::kMeasureFound && PM_MEASURE_CLAMPED == pm::kMeasureClamped && PM_MEASURE_DEGENERATE == pm::kMeasureDegenerate,
              "pm_measure.h's constants are the header's");
static_assert(sizeof(pm_item_length) == 16 && offsetof(pm_item_length, length) == 0 && offsetof(pm_item_length, n_segments) == 8 &&
                  offsetof(pm_item_length, kind) == 12,
              "the record pm_item_lengths_kernel writes");
static_assert(sizeof(pm_length_query) == 16 && offsetof(pm_length_query, item) == 0 && offsetof(pm_length_query, reserved) == 4 && offsetof(pm_length_query, s) == 8 &&
                  sizeof(pm_edge_query) == 16 && offsetof(pm_edge_query, item) == 0 && offsetof(pm_edge_query, index) == 4 && offsetof(pm_edge_query, t) == 8 &&
                  offsetof(pm_edge_query, reserved) == 12,
              "the queries the measure kernels read");
static_assert(sizeof(pm_length_point) == 32 && offsetof(pm_length_point, item) == 0 && offsetof(pm_length_point, status) == 4 &&
                  offsetof(pm_length_point, index) == 8 && offsetof(pm_length_point, t) == 12 && offsetof(pm_length_point, x) == 16 &&
                  offsetof(pm_length_point, y) == 20 && offsetof(pm_length_point, tx) == 24 && offsetof(pm_length_point, ty) == 28 &&
                  sizeof(pm_length_at) == 16 && offsetof(pm_length_at, s) == 0 && offsetof(pm_length_at, item) == 8 && offsetof(pm_length_at, status) == 12,
              "the records the measure kernels write");

constexpr size_t kMeasureBatch = static_cast<size_t>(1) << 20;   // pm_points_at_length, pm_positions_on_edges: queries staged at a time (32 to 48 MiB)

// Everything the two per-query calls refuse, before anything is enqueued
int MeasureCheck(pm_ctx *c, const char *name, const void *q, size_t n, uint32_t flags, const void *out) {
    const int r = HitCheck(c, flags);
    if (r != PM_OK) return r;
    if (n != 0 && (!q || !out)) {
        SetError(std::string(name) + ": a NULL pointer with n != 0");
        return PM_ERR_INVALID;
    }
    return PM_OK;
}

int MeasureAligned(const char *name, const void *a, const void *b) {
    if (((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 7u) != 0) {
        SetError(std::string(name) + ": a device pointer is not 8-byte aligned");
        return PM_ERR_INVALID;
    }
    return PM_OK;
}

int ItemLengthsEnqueue(pm_ctx *c, uint32_t flags, uint8_t *d_out, hipStream_t q) {
    int r = QueryOrderBefore(c, q);
    if (r != PM_OK) return r;
    pm::MeasureParams p{};
    p.V = QueryView(c, flags);
    p.out = d_out;
    pm::LaunchItemLengths(p, static_cast<uint32_t>(c->n_cus), q);
    return QueryOrderBehind(c, q);
}

// The launches of either per-query kernel for n queries of 16 bytes in device memory, on q
int MeasureEnqueue(pm_ctx *c, void (*launch)(const pm::MeasureParams &, uint32_t, hipStream_t), size_t record, const uint8_t *d_q, size_t n, uint32_t flags,
                   uint8_t *d_out, hipStream_t q) {
    int r = QueryOrderBefore(c, q);
    if (r != PM_OK) return r;
    pm::MeasureParams p{};
    p.V = QueryView(c, flags);
    for (size_t at = 0; at < n; at += kHitLaunchMax) {
        p.q = d_q + 16 * at;
        p.out = d_out + record * at;
        p.n = static_cast<uint32_t>(std::min(n - at, kHitLaunchMax));
        launch(p, static_cast<uint32_t>(c->n_cus), q);
    }
    return QueryOrderBehind(c, q);
}

// The host-memory variant of either: {records, queries} through the staging buffer
int MeasureToHost(pm_ctx *c, void (*launch)(const pm::MeasureParams &, uint32_t, hipStream_t), size_t record, const void *q, size_t n, uint32_t flags, void *out) {
    return QueryBatches(c, q, 16, n, kMeasureBatch, {out, record}, {nullptr, 0}, nullptr, 0, [&](uint8_t *d_in, size_t m, uint8_t *d_out, uint8_t *, uint8_t *) {
        return MeasureEnqueue(c, launch, record, d_in, m, flags, d_out, c->stream);
    });
}
}  // namespace

int pm_item_lengths_device(pm_ctx *c, uint32_t flags, void *dev_out, size_t cap, void *hip_stream) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = HitCheck(c, flags);
    if (r != PM_OK) return r;
    if (cap < c->n_items) return PM_ERR_CAPACITY;
    if (c->n_items == 0) return PM_OK;
    if (!dev_out || (reinterpret_cast<uintptr_t>(dev_out) & 7u) != 0) {
        SetError("pm_item_lengths_device: dev_out is NULL or not 8-byte aligned");
        return PM_ERR_INVALID;
    }
    return ItemLengthsEnqueue(c, flags, static_cast<uint8_t *>(dev_out), QueryStream(c, hip_stream));
}

int pm_item_lengths(pm_ctx *c, uint32_t flags, pm_item_length *out, size_t cap, uint32_t *n_items) {
    if (!c) return PM_ERR_INVALID;
    if (n_items) *n_items = c->scene_bytes >= 8 ? c->n_items : 0u;
    PM_TRY(hipSetDevice(c->device));
    int r = HitCheck(c, flags);
    if (r != PM_OK) return r;
    const size_t n = c->n_items;
    if (cap < n) return PM_ERR_CAPACITY;
    if (n == 0) return PM_OK;
    if (!out) {
        SetError("pm_item_lengths: out is NULL");
        return PM_ERR_INVALID;
    }
    PM_TRY(QueryStaging(c, n * sizeof(pm_item_length)));
    r = ItemLengthsEnqueue(c, flags, c->d_stage, c->stream);
    if (r != PM_OK) return r;
    PM_TRY(hipMemcpyAsync(out, c->d_stage, n * sizeof(pm_item_length), hipMemcpyDeviceToHost, c->stream));
    PM_TRY(hipStreamSynchronize(c->stream));
    return PM_OK;
}

int pm_points_at_length_device(pm_ctx *c, const void *dev_q, size_t n, uint32_t flags, void *dev_out, void *hip_stream) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r = MeasureCheck(c, "pm_points_at_length", dev_q, n, flags, dev_out);
    if (r != PM_OK || n == 0) return r;
    r = MeasureAligned("pm_points_at_length_device", dev_q, dev_out);
    if (r != PM_OK) return r;
    return MeasureEnqueue(c, pm::LaunchPointsAtLength, sizeof(pm_length_point), static_cast<const uint8_t *>(dev_q), n, flags, static_cast<uint8_t *>(dev_out),
                          QueryStream(c, hip_stream));
}

int pm_points_at_length(pm_ctx *c, const pm_length_query *q, size_t n, uint32_t flags, pm_length_point *out) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = MeasureCheck(c, "pm_points_at_length", q, n, flags, out);
    if (r != PM_OK || n == 0) return r;
    for (size_t k = 0; k < n; ++k) {
        if (q[k].reserved != 0u) {
            SetError("pm_points_at_length: a query's reserved word is not 0");
            return PM_ERR_INVALID;
        }
    }
    return MeasureToHost(c, pm::LaunchPointsAtLength, sizeof(*out), q, n, flags, out);
}

int pm_positions_on_edges_device(pm_ctx *c, const void *dev_q, size_t n, uint32_t flags, void *dev_out, void *hip_stream) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r = MeasureCheck(c, "pm_positions_on_edges", dev_q, n, flags, dev_out);
    if (r != PM_OK || n == 0) return r;
    r = MeasureAligned("pm_positions_on_edges_device", dev_q, dev_out);
    if (r != PM_OK) return r;
    return MeasureEnqueue(c, pm::LaunchPositionsOnEdges, sizeof(pm_length_at), static_cast<const uint8_t *>(dev_q), n, flags, static_cast<uint8_t *>(dev_out),
                          QueryStream(c, hip_stream));
}

int pm_positions_on_edges(pm_ctx *c, const pm_edge_query *q, size_t n, uint32_t flags, pm_length_at *out) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = MeasureCheck(c, "pm_positions_on_edges", q, n, flags, out);
    if (r != PM_OK || n == 0) return r;
    for (size_t k = 0; k < n; ++k) {
        if (q[k].reserved != 0u) {
            SetError("pm_positions_on_edges: a query's reserved word is not 0");
            return PM_ERR_INVALID;
        }
    }
    return MeasureToHost(c, pm::LaunchPositionsOnEdges, sizeof(*out), q, n, flags, out);
}

// ---- resampling (pm_resample.h; decision D26) -------------------------------------------------------------------------------------------
namespace {
static_assert(PM_RESAMPLE_STEP == pm::kResampleStep && PM_RESAMPLE_EVEN == pm::kResampleEven && PM_RESAMPLE_MAX_COUNT == pm::kResampleMaxCount &&
                  PM_RESAMPLE_INVALID == pm::kResampleInvalid,
              "pm_resample.h's constants are the header's");
static_assert(sizeof(pm_resample_query) == 32 && offsetof(pm_resample_query, item) == 0 && offsetof(pm_resample_query, mode) == 4 &&
                  offsetof(pm_resample_query, count) == 8 && offsetof(pm_resample_query, first) == 12 && offsetof(pm_resample_query, start) == 16 &&
                  offsetof(pm_resample_query, step) == 24,
              "the request pm_resample_kernel reads");
static_assert(sizeof(pm_resample_info) == 16 && offsetof(pm_resample_info, length) == 0 && offsetof(pm_resample_info, n_unclamped) == 8 &&
                  offsetof(pm_resample_info, kind) == 12,
              "the info pm_resample_kernel writes");
static_assert(PM_RESAMPLE_MAX_COUNT == kMeasureBatch, "a request fits the staging of pm_points_at_length");

// The launches for n requests in device memory, on q
int ResampleEnqueue(pm_ctx *c, const uint8_t *d_q, size_t n, uint32_t flags, uint8_t *d_out, size_t out_cap, uint8_t *d_info, hipStream_t q) {
    int r = QueryOrderBefore(c, q);
    if (r != PM_OK) return r;
    pm::ResampleParams p{};
    p.V = QueryView(c, flags);
    p.out = d_out;
    p.out_cap = out_cap;
    for (size_t at = 0; at < n; at += kHitLaunchMax) {
        p.q = d_q + sizeof(pm_resample_query) * at;
        p.info = d_info + sizeof(pm_resample_info) * at;
        p.n = static_cast<uint32_t>(std::min(n - at, kHitLaunchMax));
        pm::LaunchResample(p, static_cast<uint32_t>(c->n_cus), q);
    }
    return QueryOrderBehind(c, q);
}
}  // namespace

int pm_resample_items_device(pm_ctx *c, const void *dev_q, size_t n, uint32_t flags, void *dev_out, size_t out_cap, void *dev_info, void *hip_stream) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = HitCheck(c, flags);
    if (r != PM_OK || n == 0) return r;
    if (!dev_q || !dev_info || (!dev_out && out_cap != 0)) {
        SetError("pm_resample_items_device: a NULL pointer with n != 0");
        return PM_ERR_INVALID;
    }
    if (((reinterpret_cast<uintptr_t>(dev_q) | reinterpret_cast<uintptr_t>(dev_out) | reinterpret_cast<uintptr_t>(dev_info)) & 7u) != 0) {
        SetError("pm_resample_items_device: a device pointer is not 8-byte aligned");
        return PM_ERR_INVALID;
    }
    return ResampleEnqueue(c, static_cast<const uint8_t *>(dev_q), n, flags, static_cast<uint8_t *>(dev_out), out_cap, static_cast<uint8_t *>(dev_info),
                           QueryStream(c, hip_stream));
}

int pm_resample_items(pm_ctx *c, const pm_resample_query *q, size_t n, uint32_t flags, pm_length_point *out, size_t out_cap, pm_resample_info *info) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r = HitCheck(c, flags);
    if (r != PM_OK || n == 0) return r;
    if (!q || !out || !info) {
        SetError("pm_resample_items: a NULL pointer with n != 0");
        return PM_ERR_INVALID;
    }
    size_t total = 0;
    for (size_t k = 0; k < n; ++k) {
        if (q[k].mode > PM_RESAMPLE_EVEN || q[k].count > PM_RESAMPLE_MAX_COUNT || (q[k].mode == PM_RESAMPLE_EVEN && (q[k].start | q[k].step) != 0)) {
            SetError("pm_resample_items: a request's mode, count, or the start or step of an even request");
            return PM_ERR_INVALID;
        }
        if (q[k].first != total) {   // (a total beyond 2^32 cannot be named by a `first`: refused here)
            SetError("pm_resample_items: a request's first is not the sum of the counts before it");
            return PM_ERR_INVALID;
        }
        total += q[k].count;
    }
    if (total > out_cap || total > kMeasureBatch) return PM_ERR_CAPACITY;
    // the staging buffer: {records, then per batch of requests: infos, requests}
    const size_t batch = std::min(n, kMeasureBatch), at_info = total * sizeof(*out), at_q = at_info + batch * sizeof(*info);
    PM_TRY(QueryStaging(c, at_q + batch * sizeof(*q)));
    for (size_t at = 0; at < n; at += batch) {
        const size_t m = std::min(batch, n - at);
        PM_TRY(hipMemcpyAsync(c->d_stage + at_q, q + at, m * sizeof(*q), hipMemcpyHostToDevice, c->stream));
        r = ResampleEnqueue(c, c->d_stage + at_q, m, flags, c->d_stage, total, c->d_stage + at_info, c->stream);
        if (r != PM_OK) return r;
        PM_TRY(hipMemcpyAsync(info + at, c->d_stage + at_info, m * sizeof(*info), hipMemcpyDeviceToHost, c->stream));
        if (at + m == n && total != 0) PM_TRY(hipMemcpyAsync(out, c->d_stage, total * sizeof(*out), hipMemcpyDeviceToHost, c->stream));
        PM_TRY(hipStreamSynchronize(c->stream));
    }
    return PM_OK;
}

// ---- trimming (pm_trim.h; decision D27) ---------------------------------------------------------------------------------------------------
namespace {
static_assert(PM_TRIM_RANGE == pm::kTrimRange && PM_TRIM_PART == pm::kTrimPart && PM_TRIM_MAX_PARTS == pm::kTrimMaxParts && PM_TRIM_INVALID == pm::kTrimInvalid &&
                  PM_TRIM_MOVE == pm::kTrimMove && PM_TRIM_CUT == pm::kTrimCut && PM_TRIM_TRUNCATED == pm::kTrimTruncated &&
                  PM_TRIM_END_CLAMPED == pm::kTrimEndClamped,
              "pm_trim.h's constants are the header's");
static_assert(sizeof(pm_trim_query) == 32 && offsetof(pm_trim_query, item) == 0 && offsetof(pm_trim_query, mode) == 4 && offsetof(pm_trim_query, first) == 8 &&
                  offsetof(pm_trim_query, cap) == 12 && offsetof(pm_trim_query, s0) == 16 && offsetof(pm_trim_query, s1) == 24,
              "the request pm_trim_kernel reads");
static_assert(sizeof(pm_trim_vertex) == 16 && offsetof(pm_trim_vertex, x) == 0 && offsetof(pm_trim_vertex, y) == 4 && offsetof(pm_trim_vertex, index) == 8 &&
                  offsetof(pm_trim_vertex, flags) == 12,
              "the vertex pm_trim_kernel writes");
static_assert(sizeof(pm_trim_info) == 24 && offsetof(pm_trim_info, length) == 0 && offsetof(pm_trim_info, n_vertices) == 8 && offsetof(pm_trim_info, n_runs) == 12 &&
                  offsetof(pm_trim_info, kind) == 16 && offsetof(pm_trim_info, flags) == 20,
              "the info pm_trim_kernel writes");

// Would the device call the request invalid
bool TrimInvalid(const pm_trim_query &r) {
    if (r.mode == PM_TRIM_RANGE) return r.s0 > r.s1;
    return r.mode != PM_TRIM_PART || r.s1 == 0 || r.s1 > PM_TRIM_MAX_PARTS || r.s0 >= r.s1;
}

// The launches for n requests in device memory, on q
int TrimEnqueue(pm_ctx *c, const uint8_t *d_q, size_t n, uint32_t flags, uint8_t *d_out, size_t out_cap, uint8_t *d_info, hipStream_t q) {
    int r = QueryOrderBefore(c, q);
    if (r != PM_OK) return r;
    pm::TrimParams p{};
    p.V = QueryView(c, flags);
    p.out = d_out;
    p.out_cap = out_cap;
    for (size_t at = 0; at < n; at += kHitLaunchMax) {
        p.q = d_q + sizeof(pm_trim_query) * at;
        p.info = d_info + sizeof(pm_trim_info) * at;
        p.n = static_cast<uint32_t>(std::min(n - at, kHitLaunchMax));
        pm::LaunchTrim(p, static_cast<uint32_t>(c->n_cus), q);
    }
    return QueryOrderBehind(c, q);
}
}  // namespace

int pm_trim_items_device(pm_ctx *c, const void *dev_q, size_t n, uint32_t flags, void *dev_out, size_t out_cap, void *dev_info, void *hip_stream) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = HitCheck(c, flags);
    if (r != PM_OK || n == 0) return r;
    if (!dev_q || !dev_info || (!dev_out && out_cap != 0)) {
        SetError("pm_trim_items_device: a NULL pointer with n != 0");
        return PM_ERR_INVALID;
    }
    if (((reinterpret_cast<uintptr_t>(dev_q) | reinterpret_cast<uintptr_t>(dev_out) | reinterpret_cast<uintptr_t>(dev_info)) & 7u) != 0) {
        SetError("pm_trim_items_device: a device pointer is not 8-byte aligned");
        return PM_ERR_INVALID;
    }
    return TrimEnqueue(c, static_cast<const uint8_t *>(dev_q), n, flags, static_cast<uint8_t *>(dev_out), out_cap, static_cast<uint8_t *>(dev_info),
                       QueryStream(c, hip_stream));
}

int pm_trim_items(pm_ctx *c, const pm_trim_query *q, size_t n, uint32_t flags, pm_trim_vertex *out, size_t out_cap, pm_trim_info *info) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r = HitCheck(c, flags);
    if (r != PM_OK || n == 0) return r;
    if (!q || !info) {
        SetError("pm_trim_items: a NULL pointer with n != 0");
        return PM_ERR_INVALID;
    }
    size_t total = 0;
    for (size_t k = 0; k < n; ++k) {
        if (TrimInvalid(q[k])) {
            SetError("pm_trim_items: a request's mode, a range with s0 > s1, or a part j of m without 1 <= m <= 2^20 and j < m");
            return PM_ERR_INVALID;
        }
        if (q[k].first != total) {   // (a total beyond 2^32 cannot be named by a `first`: refused here)
            SetError("pm_trim_items: a request's first is not the sum of the caps before it");
            return PM_ERR_INVALID;
        }
        total += q[k].cap;
    }
    if (total != 0 && !out) {
        SetError("pm_trim_items: out is NULL with vertices to write");
        return PM_ERR_INVALID;
    }
    if (total > out_cap || total > kMeasureBatch) return PM_ERR_CAPACITY;
    // the staging buffer: {vertices, then per batch of requests: infos, requests}
    const size_t batch = std::min(n, kMeasureBatch), at_info = total * sizeof(*out), at_q = at_info + batch * sizeof(*info);
    PM_TRY(QueryStaging(c, at_q + batch * sizeof(*q)));
    for (size_t at = 0; at < n; at += batch) {
        const size_t m = std::min(batch, n - at);
        PM_TRY(hipMemcpyAsync(c->d_stage + at_q, q + at, m * sizeof(*q), hipMemcpyHostToDevice, c->stream));
        r = TrimEnqueue(c, c->d_stage + at_q, m, flags, c->d_stage, total, c->d_stage + at_info, c->stream);
        if (r != PM_OK) return r;
        PM_TRY(hipMemcpyAsync(info + at, c->d_stage + at_info, m * sizeof(*info), hipMemcpyDeviceToHost, c->stream));
        PM_TRY(hipStreamSynchronize(c->stream));
    }
    if (total == 0) return PM_OK;
    // a piece shorter than its cap leaves rows of its range that the device did not write: those stay the caller's
    bool exact = true;
    for (size_t k = 0; k < n && exact; ++k) exact = info[k].n_vertices >= q[k].cap;
    if (exact) {
        PM_TRY(hipMemcpyAsync(out, c->d_stage, total * sizeof(*out), hipMemcpyDeviceToHost, c->stream));
        PM_TRY(hipStreamSynchronize(c->stream));
        return PM_OK;
    }
    std::vector<pm_trim_vertex> got(total);
    PM_TRY(hipMemcpyAsync(got.data(), c->d_stage, total * sizeof(*out), hipMemcpyDeviceToHost, c->stream));
    PM_TRY(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < n; ++k) {
        const size_t wrote = std::min<size_t>(q[k].cap, info[k].n_vertices);
        if (wrote != 0) std::memcpy(out + q[k].first, got.data() + q[k].first, wrote * sizeof(*out));
    }
    return PM_OK;
}

// ---- item crossings (pm_crossings.h; decision D29) ------------------------------------------------------------------------------------------
namespace {
static_assert(PM_CROSSINGS_TRUNCATED == pm::kCrossingsTruncated && PM_CROSSINGS_TOO_MANY == pm::kCrossingsTooMany && PM_CROSSINGS_MAX_PAIRS == pm::kCrossingsMaxPairs,
              "pm_crossings.h's constants are the header's");
static_assert(sizeof(pm_crossings_query) == 16 && offsetof(pm_crossings_query, item_a) == 0 && offsetof(pm_crossings_query, item_b) == 4 &&
                  offsetof(pm_crossings_query, first) == 8 && offsetof(pm_crossings_query, cap) == 12,
              "the request pm_crossings_kernel reads");
static_assert(sizeof(pm_crossing) == 48 && offsetof(pm_crossing, item_a) == 0 && offsetof(pm_crossing, index_a) == 4 && offsetof(pm_crossing, t) == 8 &&
                  offsetof(pm_crossing, item_b) == 16 && offsetof(pm_crossing, index_b) == 20 && offsetof(pm_crossing, u) == 24 && offsetof(pm_crossing, x) == 32 &&
                  offsetof(pm_crossing, y) == 36 && offsetof(pm_crossing, side) == 40 && sizeof(pm_edge_query) == 16,
              "the record pm_crossings_kernel writes: two pm_edge_query, the point, the side");
static_assert(sizeof(pm_crossings_info) == 16 && offsetof(pm_crossings_info, n_crossings) == 0 && offsetof(pm_crossings_info, flags) == 4 &&
                  offsetof(pm_crossings_info, n_a) == 8 && offsetof(pm_crossings_info, n_b) == 12,
              "the info pm_crossings_kernel writes");

// The launches for n requests in device memory, on q
int CrossingsEnqueue(pm_ctx *c, const uint8_t *d_q, size_t n, uint32_t flags, uint8_t *d_out, size_t out_cap, uint8_t *d_info, hipStream_t q) {
    int r = QueryOrderBefore(c, q);
    if (r != PM_OK) return r;
    pm::CrossingsParams p{};
    p.V = QueryView(c, flags);
    p.out = d_out;
    p.out_cap = out_cap;
    for (size_t at = 0; at < n; at += kHitLaunchMax) {
        p.q = d_q + sizeof(pm_crossings_query) * at;
        p.info = d_info + sizeof(pm_crossings_info) * at;
        p.n = static_cast<uint32_t>(std::min(n - at, kHitLaunchMax));
        pm::LaunchCrossings(p, static_cast<uint32_t>(c->n_cus), q);
    }
    return QueryOrderBehind(c, q);
}
}  // namespace

int pm_item_crossings_device(pm_ctx *c, const void *dev_q, size_t n, uint32_t flags, void *dev_out, size_t out_cap, void *dev_info, void *hip_stream) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    const int r = HitCheck(c, flags);
    if (r != PM_OK || n == 0) return r;
    if (!dev_q || !dev_info || (!dev_out && out_cap != 0)) {
        SetError("pm_item_crossings_device: a NULL pointer with n != 0");
        return PM_ERR_INVALID;
    }
    if (((reinterpret_cast<uintptr_t>(dev_q) | reinterpret_cast<uintptr_t>(dev_out) | reinterpret_cast<uintptr_t>(dev_info)) & 7u) != 0) {
        SetError("pm_item_crossings_device: a device pointer is not 8-byte aligned");
        return PM_ERR_INVALID;
    }
    return CrossingsEnqueue(c, static_cast<const uint8_t *>(dev_q), n, flags, static_cast<uint8_t *>(dev_out), out_cap, static_cast<uint8_t *>(dev_info),
                            QueryStream(c, hip_stream));
}

int pm_item_crossings(pm_ctx *c, const pm_crossings_query *q, size_t n, uint32_t flags, pm_crossing *out, size_t out_cap, pm_crossings_info *info) {
    if (!c) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r = HitCheck(c, flags);
    if (r != PM_OK || n == 0) return r;
    if (!q || !info) {
        SetError("pm_item_crossings: a NULL pointer with n != 0");
        return PM_ERR_INVALID;
    }
    size_t total = 0;
    for (size_t k = 0; k < n; ++k) {
        if (q[k].first != total) {   // (a total beyond 2^32 cannot be named by a `first`: refused here)
            SetError("pm_item_crossings: a request's first is not the sum of the caps before it");
            return PM_ERR_INVALID;
        }
        total += q[k].cap;
    }
    if (total != 0 && !out) {
        SetError("pm_item_crossings: out is NULL with records to write");
        return PM_ERR_INVALID;
    }
    if (total > out_cap || total > kMeasureBatch) return PM_ERR_CAPACITY;
    // the staging buffer: {records, then per batch of requests: infos, requests}
    const size_t batch = std::min(n, kMeasureBatch), at_info = total * sizeof(*out), at_q = at_info + batch * sizeof(*info);
    PM_TRY(QueryStaging(c, at_q + batch * sizeof(*q)));
    for (size_t at = 0; at < n; at += batch) {
        const size_t m = std::min(batch, n - at);
        PM_TRY(hipMemcpyAsync(c->d_stage + at_q, q + at, m * sizeof(*q), hipMemcpyHostToDevice, c->stream));
        r = CrossingsEnqueue(c, c->d_stage + at_q, m, flags, c->d_stage, total, c->d_stage + at_info, c->stream);
        if (r != PM_OK) return r;
        PM_TRY(hipMemcpyAsync(info + at, c->d_stage + at_info, m * sizeof(*info), hipMemcpyDeviceToHost, c->stream));
        PM_TRY(hipStreamSynchronize(c->stream));
    }
    if (total == 0) return PM_OK;
    // an answer shorter than its cap leaves rows of its range that the device did not write: those stay the caller's
    bool exact = true;
    for (size_t k = 0; k < n && exact; ++k) exact = info[k].n_crossings >= q[k].cap;
    if (exact) {
        PM_TRY(hipMemcpyAsync(out, c->d_stage, total * sizeof(*out), hipMemcpyDeviceToHost, c->stream));
        PM_TRY(hipStreamSynchronize(c->stream));
        return PM_OK;
    }
    std::vector<pm_crossing> got(total);
    PM_TRY(hipMemcpyAsync(got.data(), c->d_stage, total * sizeof(*out), hipMemcpyDeviceToHost, c->stream));
    PM_TRY(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < n; ++k) {
        const size_t wrote = std::min<size_t>(q[k].cap, info[k].n_crossings);
        if (wrote != 0) std::memcpy(out + q[k].first, got.data() + q[k].first, wrote * sizeof(*out));
    }
    return PM_OK;
}

int pm_item_paths(pm_ctx *c, uint32_t *path_of_item, size_t cap, uint32_t *n_items) {
    if (!c || !n_items) return PM_ERR_INVALID;
    *n_items = c->scene_bytes >= 8 ? c->n_items : 0u;
    if (c->scene_bytes < 8 || !c->scene_from_paths) {
        SetError("pm_item_paths: the resident scene was not made by pm_flatten_and_encode / pm_reflatten");
        return PM_ERR_INVALID;
    }
    const size_t n = c->n_items;
    if (cap < n) return PM_ERR_CAPACITY;
    if (n == 0) return PM_OK;
    if (!path_of_item) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    // KItems numbers a path's items from path_item_base[p] on (fills first, then strokes): the table is still where the scan left it
    std::vector<uint32_t> base(c->flatten_cache.n_paths);
    hipError_t he = hipSuccess;
    const int r = pm::FlattenPathItemBases(c->stream, &c->flatten_cache, base.data(), &he);
    if (r == PM_ERR_HIP) return HipFail(he, "pm_item_paths");
    if (r != PM_OK) return r;
    for (size_t p = 0; p < base.size(); ++p) {
        const size_t end = p + 1 < base.size() ? base[p + 1] : n;
        if (base[p] > end || end > n) {
            SetError("pm_item_paths: the flatten stage's item table does not match the resident scene");
            return PM_ERR_SCENE;
        }
        for (size_t i = base[p]; i < end; ++i) path_of_item[i] = static_cast<uint32_t>(p);
    }
    return PM_OK;
}

int pm_debug_capture_ptcl(pm_ctx *c, uint32_t max_cmds_per_tile, uint32_t *counts, uint32_t *solid, pm_cmd *cmds) {
    if (!c || !counts || !solid || (max_cmds_per_tile && !cmds)) return PM_ERR_INVALID;
    if (c->last_slot < 0) {
        SetError("pm_debug_capture_ptcl needs a rendered frame");
        return PM_ERR_INVALID;
    }
    PM_TRY(hipSetDevice(c->device));
    int r = pm_sync(c);
    if (r != PM_OK) return r;
    FrameSlot *s = &c->slot[c->last_slot];
    const size_t tiles = static_cast<size_t>(BandRows(c)) * c->tiles_x;
    uint32_t *d_counts = nullptr, *d_solid = nullptr;
    pm::Cmd *d_cmds = nullptr;
    PM_TRY(hipMalloc(&d_counts, std::max<size_t>(tiles, 1) * sizeof(uint32_t)));
    PM_TRY(hipMalloc(&d_solid, std::max<size_t>(tiles, 1) * sizeof(uint32_t)));
    PM_TRY(hipMalloc(&d_cmds, std::max<size_t>(tiles * max_cmds_per_tile, 1) * sizeof(pm::Cmd)));
    // tiles the binning kernel resolved itself never reach the tile kernels: {Bail} + its colour
    std::vector<uint32_t> h_counts(tiles, 1u), h_solid(tiles, 0xffffffffu);
    std::vector<pm::Cmd> h_cmds(tiles * max_cmds_per_tile);
    if (tiles) PM_TRY(hipMemcpy(h_solid.data(), s->d_tile_state, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost));
    for (size_t t = 0; t < tiles && max_cmds_per_tile; ++t) {
        h_cmds[t * max_cmds_per_tile].tag = pm::kCmdBail;
        std::memset(h_cmds[t * max_cmds_per_tile].body, 0, sizeof(h_cmds[0].body));
    }
    int status = PM_OK;
    hipError_t e = hipMemcpy(d_counts, h_counts.data(), tiles * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_solid, h_solid.data(), tiles * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && max_cmds_per_tile) e = hipMemcpy(d_cmds, h_cmds.data(), h_cmds.size() * sizeof(pm::Cmd), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        pm::FrameParams p = s->params;  // same arena / queues / counters as the last frame
        if (p.one_launch != 0u) {
            // the last frame was ONE launch: no queues to replay -- the frame is rendered again (same target, same bytes) by the
            // capture instantiation of that kernel
            c->cap_counts = d_counts;
            c->cap_solid = d_solid;
            c->cap_cmds = d_cmds;
            c->cap_max = max_cmds_per_tile;
            bool own = false;
            for (auto &t : c->slot) own = own || p.fb == t.d_fb;
            status = Enqueue(c, own ? nullptr : p.fb, p.fb_stride, nullptr);
            c->cap_counts = c->cap_solid = nullptr;
            c->cap_cmds = nullptr;
            c->cap_max = 0;
            if (status == PM_OK) status = pm_sync(c);
            if (status == PM_OK && c->slot[c->last_slot].params.dbg_counts == nullptr) {
                SetError("pm_debug_capture_ptcl: the frame could not be rendered again as one launch");
                status = PM_ERR_INVALID;
            }
            if (status != PM_OK) e = hipErrorUnknown;
        } else {
        p.dbg_counts = d_counts;
        p.dbg_solid = d_solid;
        p.dbg_cmds = d_cmds;
        p.dbg_max = max_cmds_per_tile;
        if (c->fused) {
            // the frame path's own kernel, capture switched on (it rebuilds the same lists and renders
            // the same pixels: idempotent); the frame's hand-out counters are spent: deal again
            e = hipMemsetAsync(&p.ctr_cur->ticket, 0, sizeof(p.ctr_cur->ticket), c->stream);
            pm::LaunchFine(p, 0u, true, c->stream);
        } else {
            pm::LaunchCoarse(p, CoarseGrid(c), true, c->stream);  // replays the last frame's queues
        }
        }
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    }
    if (e == hipSuccess) e = hipMemcpy(counts, d_counts, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(solid, d_solid, tiles * sizeof(uint32_t), hipMemcpyDeviceToHost);
    if (e == hipSuccess && max_cmds_per_tile) e = hipMemcpy(cmds, d_cmds, tiles * max_cmds_per_tile * sizeof(pm::Cmd), hipMemcpyDeviceToHost);
    if (e != hipSuccess && status == PM_OK) status = HipFail(e, "ptcl capture");
    (void)hipFree(d_counts);
    (void)hipFree(d_solid);
    (void)hipFree(d_cmds);
    return status;
}

int pm_debug_time_bins(pm_ctx *c, uint64_t *out, size_t max_rows, size_t *n_rows) {
    if (!c || !out) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r = SyncAll(c);
    if (r != PM_OK) return r;
    r = EnsureArena(c);  // (the work list: one row of the timeline per entry, in the list's order)
    if (r != PM_OK) return r;
    const size_t rows = std::max<size_t>(static_cast<size_t>(BandRows(c)) * c->strips_x, c->plan.n_sr_active());
    if (n_rows) *n_rows = rows;
    if (rows > max_rows) return PM_ERR_CAPACITY;
    unsigned long long *d = nullptr;
    PM_TRY(hipMalloc(&d, std::max<size_t>(rows, 1) * 16 * sizeof(unsigned long long)));
    PM_TRY(hipMemset(d, 0, std::max<size_t>(rows, 1) * 16 * sizeof(unsigned long long)));
    const int si = static_cast<int>(c->frame % c->slot.size());
    FrameSlot *s = &c->slot[si];
    pm::FrameParams p;
    r = BuildParams(c, s, nullptr, c->fb_stride, &p);
    if (r == PM_OK) {
        p.dbg_bin = d;
        hipError_t e = ResetTileState(c, s, c->stream);
        pm::LaunchBin(p, c->stream);
        if (!c->fold_clear && !p.clear_in_bin) pm::LaunchClear(p, BandRows(c) * c->strips_x, c->stream);
        if (!c->fused) pm::LaunchCoarse(p, CoarseGrid(c), false, c->stream);
        pm::LaunchFine(p, c->fold_clear && !p.clear_in_bin ? BandRows(c) * c->strips_x : 0u, c->fused, c->stream);
        p.dbg_bin = nullptr;
        Submitted(c, si, p, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e == hipSuccess) e = hipMemcpy(out, d, rows * 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        if (e != hipSuccess) r = HipFail(e, "bin timeline");
    }
    (void)hipFree(d);
    return r;
}

int pm_debug_time_tiles(pm_ctx *c, uint64_t *out, size_t max_slots, size_t *n_slots) {
    if (!c || !out || c->last_slot < 0) return PM_ERR_INVALID;
    PM_TRY(hipSetDevice(c->device));
    int r = pm_sync(c);
    if (r != PM_OK) return r;
    FrameSlot *s = &c->slot[c->last_slot];
    pm::Counters k;
    PM_TRY(hipMemcpy(&k, s->params.ctr_cur, sizeof(k), hipMemcpyDeviceToHost));
    // as pm_fine_kernel decides
    size_t heavy = 0, total = 0;
    for (uint32_t q = 0; q < pm::kClasses; ++q) {
        for (uint32_t sh = 0; sh < pm::kClassShards; ++sh) {
            total += k.cls[sh].count[q];
            if (q < 3) heavy += k.cls[sh].count[q];
        }
    }
    const bool dense = heavy * c->dense_factor >= static_cast<size_t>(s->params.fine_grid) * 4u || c->split_mode == 0;
    const size_t slots = dense ? total : 4 * heavy + (total - heavy);
    if (n_slots) *n_slots = slots;
    if (slots > max_slots) return PM_ERR_CAPACITY;
    unsigned long long *d = nullptr;
    PM_TRY(hipMalloc(&d, std::max<size_t>(slots, 1) * 12 * sizeof(unsigned long long)));
    pm::FrameParams p = s->params;
    p.dbg_time = d;
    // the frame's hand-out counters are spent: deal again
    PM_TRY(hipMemsetAsync(&p.ctr_cur->ticket, 0, sizeof(p.ctr_cur->ticket), c->stream));
    pm::LaunchFine(p, 0u, c->fused, c->stream);  // (the fused kernel rebuilds the same lists: idempotent)
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = hipMemcpy(out, d, slots * 12 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return HipFail(e, "tile timeline");
    return PM_OK;
}

// Drop-in for include/piet_metal.h:3 / src/lib.rs:387-393 (make_test_scene -> make_tiger).
void init_test_scene(uint8_t *buf, ssize_t buf_size) {
    if (!buf || buf_size <= 0) {
        SetError("init_test_scene: bad buffer");
        return;
    }
    int err = PM_OK;
    pm_ctx *c = pm_create(0, &err);
    if (!c) return;
    pm_svg *svg = pm_svg_tiger(0, &err);
    if (svg) {
        const double scale = 8.0;  // src/lib.rs:287
        const double affine[6] = {scale, 0.0, 0.0, scale, 0.0, 0.0};
        size_t bytes = 0;
        uint32_t items = 0;
        err = pm_flatten_and_encode(c, pm_svg_paths(svg), pm_svg_n_paths(svg), pm_svg_els(svg), pm_svg_n_els(svg), affine,
                                    static_cast<float>(scale), &bytes, &items);
        if (err == PM_OK) {
            if (bytes > static_cast<size_t>(buf_size)) SetError("init_test_scene: buffer too small for the Tiger scene");
            else (void)pm_download_scene(c, buf, static_cast<size_t>(buf_size), &bytes);
        }
        pm_svg_free(svg);
    }
    pm_destroy(c);
}

}  // extern "C"
