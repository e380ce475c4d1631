/*
 * piet_metal_amd -- C ABI of the MI355X-native (gfx950) replacement for the
 * compute path of linebender/piet-metal.
 *
 * Every entry point names the reference interface it replaces (paths relative
 * to the piet-metal repository).  No C++/torch types cross this boundary:
 * plain pointers, sizes and status codes only.  Nothing here ever throws or
 * unwinds; the reference's Rust panics / NSLog+nil become negative status codes.
 *
 * One pm_ctx = one GPU + one HIP stream.  A ctx is not thread-safe (the
 * reference renderer is only ever driven from the main thread,
 * TestApp/PietRenderer.m:59).  Multi-GPU = one process and one ctx per GPU,
 * each rendering a band of tile rows (pm_set_band); the bands are gathered by
 * the host layer over RCCL.
 */
#ifndef PIET_METAL_AMD_H
#define PIET_METAL_AMD_H

#include <stddef.h>
#include <stdint.h>
#include <sys/types.h> /* ssize_t */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes --------------------------------------------------------- */
#define PM_OK 0
#define PM_ERR_INVALID (-1)   /* bad argument / encoder misuse (Rust assert!, src/lib.rs:147,152) */
#define PM_ERR_NO_DEVICE (-2) /* no usable gfx950 device: the product has no CPU fallback */
#define PM_ERR_HIP (-3)       /* HIP runtime error (see pm_last_error) */
#define PM_ERR_CAPACITY (-4)  /* scene buffer / arena too small */
#define PM_ERR_SCENE (-5)     /* malformed scene buffer */
#define PM_ERR_PARSE (-6)     /* SVG / path-data syntax error */

/* ---- constants kept from TestApp/PietShaderTypes.h:17-18 -------------------- */
#define PM_TILE_W 16
#define PM_TILE_H 16
/* maxTilesWidth/Height (256) and tileBufSize (4096) of PietShaderTypes.h:27-32 are
 * gone: the tile grid and the per-tile command storage are dynamic. */

/* ==== 1. scene producer ====================================================== */

/* Drop-in for include/piet_metal.h:3 (impl src/lib.rs:387-393): fills `buf`
 * with the Ghostscript Tiger scene at scale 8, flattened ON DEVICE 0 and copied
 * back.  Same signature, no status channel (errors leave buf untouched and are
 * readable through pm_last_error()).
 * PARITY UNPINNED: the bytes equal the in-repo oracle's (oracle/, a restatement of make_tiger +
 * flatten.rs + the kurbo 0.5.6 / roxmltree steps they call), not a buffer produced by the Rust
 * encoder -- none can be produced in this image; the Tiger's 6 arc paths and the current point
 * after `Z` are product-defined. */
void init_test_scene(uint8_t *buf, ssize_t buf_size);

/* Encoder, mirrors `impl Encoder` (src/lib.rs:103-254) method for method.
 * Pure host code: it only writes bytes into the caller's buffer. */
typedef struct pm_encoder pm_encoder;
pm_encoder *pm_encoder_new(uint8_t *buf, size_t cap);                 /* Encoder::new      :104 */
void pm_encoder_free(pm_encoder *e);
size_t pm_encoder_alloc(pm_encoder *e, size_t size);                  /* Encoder::alloc    :114 */
/* Encoder::write_struct :122 (`pub unsafe fn write_struct<T>(&mut self, ix: usize, s: &T)`): copies the
 * `len` bytes of a #[repr(C)] value to offset `ix` of the scene buffer.  The Rust slice index panics
 * past the end; here nothing is written and PM_ERR_CAPACITY is returned (and stays the encoder's status). */
int pm_encoder_write_struct(pm_encoder *e, size_t ix, const void *src, size_t len);
/* Encoder::encode_points :224 (`pub fn encode_points(&mut self, points: &[Point]) -> (usize, Rect)`):
 * allocates n_points (f32, f32) pairs, writes the points rounded to f32 and returns their offset in
 * *points_ix and the f64 bounding box {x0, y0, x1, y1} in bbox.  An empty slice is the reference's
 * .expect("encoded empty points vector") panic: PM_ERR_INVALID. */
int pm_encoder_encode_points(pm_encoder *e, const double *pts_xy, size_t n_points, size_t *points_ix, double bbox[4]);
int pm_encoder_begin_group(pm_encoder *e, size_t n_items);            /* begin_group       :132 */
int pm_encoder_end_group(pm_encoder *e);                              /* end_group         :146 */
int pm_encoder_circle(pm_encoder *e, double cx, double cy, double r); /* circle            :167 */
int pm_encoder_stroke_line(pm_encoder *e, double x0, double y0, double x1, double y1,
                           float width, uint32_t rgba);               /* stroke_line       :177 */
int pm_encoder_fill(pm_encoder *e, const double *pts_xy, size_t n_points,
                    uint32_t rgba);                                   /* fill              :195 */
int pm_encoder_polyline(pm_encoder *e, const double *pts_xy, size_t n_points, uint32_t rgba,
                        float width);                                 /* polyline          :209 */
/* Growth beyond the reference's Encoder, in its own terms:
 *  - PietFill.flags (src/lib.rs:54 "flags", TestApp/SceneEncoder.h:44 "will be used for winding
 *    number rule"): bit 0 selects the even-odd rule, the formula the reference leaves in a
 *    comment (TestApp/PietRender.metal:539-540);
 *  - nested groups (src/lib.rs:148 "when we have nested groups"): pm_encoder_begin_group inside
 *    an open group starts a child group that takes one item slot of its parent (item type 5,
 *    PietGroup {item_type, flags, group_ix}); pm_encoder_end_group closes the innermost group.
 *    A scene with groups renders exactly like the same items inlined in paint order. */
#define PM_FILL_EVEN_ODD 1u
/* Beyond the reference (src/lib.rs:194, "need to deal with subpaths"): ONE Fill item made of
 * n_subpaths closed sub-paths (sub_counts[k] points each, back to back in pts_xy) that share a
 * winding sum -- holes and overlapping contours resolve by fill_flags' rule.  Encoded as PietFill
 * with flags bit 1 (PM_FILL_COMPOUND); every sub-path is followed by a separator entry
 * {x = NaN, y = bits of the index of its first point}, n_points counts both. */
#define PM_FILL_COMPOUND 2u
int pm_encoder_fill_compound(pm_encoder *e, const double *pts_xy, const uint32_t *sub_counts, size_t n_subpaths, uint32_t rgba,
                             uint32_t fill_flags);
/* Beyond the reference (PietRender.metal:488-489, "I should make this shade an ellipse properly"):
 * the ellipse inscribed in the bbox of (cx +- rx, cy +- ry), black like the circle.  Encoded as a
 * Circle item with bit 16 of its item_type word set (the reference reads the tag as a ushort). */
int pm_encoder_ellipse(pm_encoder *e, double cx, double cy, double rx, double ry);
int pm_encoder_fill_rule(pm_encoder *e, const double *pts_xy, size_t n_points, uint32_t rgba,
                         uint32_t fill_flags);
size_t pm_encoder_bytes_used(const pm_encoder *e);                    /* free_space */

/* The reference's two other test scenes (host only, no flattening involved).
 * Return bytes written or a negative status. */
int64_t pm_scene_cardioid(uint8_t *buf, size_t cap);  /* make_cardioid  src/lib.rs:257-270 */
int64_t pm_scene_path_test(uint8_t *buf, size_t cap); /* make_path_test src/lib.rs:273-284 */

/* ==== 2. SVG front-end (replaces roxmltree + kurbo::BezPath::from_svg as used
 *         by make_tiger, src/lib.rs:286-328) ==================================== */

#define PM_EL_MOVE 0
#define PM_EL_LINE 1
#define PM_EL_QUAD 2
#define PM_EL_CURVE 3
#define PM_EL_CLOSE 4

typedef struct {
    uint32_t tag; /* PM_EL_* (kurbo::PathEl) */
    uint32_t pad;
    double p[6];  /* up to three points, x then y */
} pm_path_el;     /* 56 bytes */

#define PM_PATH_FILL 1u
#define PM_PATH_STROKE 2u
#define PM_PATH_EVEN_ODD 4u /* fill-rule="evenodd": the fill item gets PM_FILL_EVEN_ODD */
#define PM_PATH_COMPOUND 8u /* the path's sub-paths become ONE compound Fill item (PM_FILL_COMPOUND): holes work */
/* Stroke styles (beyond the reference, whose strokes are all round-capped, round-joined distance fields; DESIGN.md 2,
 * decision D14).  With PM_PATH_STROKE | PM_PATH_STROKE_OUTLINE every sub-path's stroke is encoded as ONE compound non-zero
 * Fill item -- the stroke's outline, built on the device at the end of the flatten stage -- in the slot of paint order the
 * poly-line item would have had.  The fields below mean something only together with these two bits; without
 * PM_PATH_STROKE_OUTLINE they are ignored and the scene is the poly-line scene, byte for byte.
 *   bits 8-9    cap:  butt 0, round 1, square 2        (3: PM_ERR_INVALID)
 *   bits 10-11  join: miter 0, round 1, bevel 2        (3: PM_ERR_INVALID)
 *   bits 16-31  miter limit as an IEEE binary16 value; 0 = 4.0 (SVG's initial value); a value below 1, NaN or
 *               infinity: PM_ERR_INVALID
 * A sub-path whose last element is PM_EL_CLOSE is closed: a closing segment, a join at every vertex, no caps. */
#define PM_PATH_STROKE_OUTLINE 0x10u
#define PM_STROKE_CAP_BUTT 0u
#define PM_STROKE_CAP_ROUND 1u
#define PM_STROKE_CAP_SQUARE 2u
#define PM_STROKE_JOIN_MITER 0u
#define PM_STROKE_JOIN_ROUND 1u
#define PM_STROKE_JOIN_BEVEL 2u
#define PM_STROKE_CAP_SHIFT 8
#define PM_STROKE_JOIN_SHIFT 10
#define PM_STROKE_MITER_SHIFT 16
/* miter_half = the limit's binary16 bits (0x4400 = 4.0; 0 = the default) */
#define PM_PATH_STROKE_STYLE(cap, join, miter_half)                                                            \
    (PM_PATH_STROKE_OUTLINE | (((uint32_t)(cap) & 3u) << PM_STROKE_CAP_SHIFT) | (((uint32_t)(join) & 3u) << PM_STROKE_JOIN_SHIFT) | \
     (((uint32_t)(miter_half) & 0xffffu) << PM_STROKE_MITER_SHIFT))
#define PM_PATH_STROKE_CAP(flags) (((flags) >> PM_STROKE_CAP_SHIFT) & 3u)
#define PM_PATH_STROKE_JOIN(flags) (((flags) >> PM_STROKE_JOIN_SHIFT) & 3u)
#define PM_PATH_STROKE_MITER_HALF(flags) (((flags) >> PM_STROKE_MITER_SHIFT) & 0xffffu)
#define PM_PATH_STROKE_STYLE_MASK 0xffff0f10u /* every bit above */

typedef struct {
    uint32_t el_begin, el_end; /* element range of this <path> */
    uint32_t flags;            /* PM_PATH_FILL | PM_PATH_STROKE (attribute present) */
    uint32_t fill_rgba;        /* 0xRRGGBBAA, parse_color src/lib.rs:375-385 */
    uint32_t stroke_rgba;
    float stroke_width;        /* user units (NOT yet scaled) */
} pm_path;                     /* 24 bytes */

/* A dash pattern for one path (decision D15): values [first, first + count) of the call's dash_values, alternately
 * dash and gap lengths in user units (scaled by width_scale like stroke widths; an odd count is repeated once), 1 <= count <= 32,
 * every value finite and >= 0; offset: where in the pattern the stroke starts (finite, may be negative). */
typedef struct {
    uint32_t path, first, count;
    float offset;
} pm_path_dash;                /* 16 bytes */

#define PM_SVG_REJECT_ARC_PATHS 1 /* drop any path whose data holds A/a */
#define PM_SVG_FLAT_GRADIENTS 4   /* url(#gradient) paints become ONE colour, the mean of the gradient's stops (the renderer has
                                     no gradients; default: such a paint is `none`, the element is not drawn with it) */
#define PM_SVG_SPEC_DEFAULTS 2    /* SVG's initial `fill: black`, and the sub-paths of a path are filled TOGETHER
                                     (PM_PATH_COMPOUND: holes); default: make_tiger's rules -- only a fill property
                                     (own or inherited) fills (src/lib.rs:299), every sub-path is its own item (:343) */
#define PM_SVG_STROKE_STYLES 8    /* read stroke-linecap / stroke-linejoin / stroke-miterlimit (inherited presentation properties;
                                     initial values butt, miter, 4) and set PM_PATH_STROKE_OUTLINE + the style on every stroked
                                     path; default: they are ignored and every stroke is the reference's round poly-line */
#define PM_SVG_STROKE_DASHES 16   /* needs PM_SVG_STROKE_STYLES (PM_ERR_INVALID without): read stroke-dasharray / stroke-dashoffset
                                     (inherited; none, comma or space lists of lengths, a negative entry means none) into the dash
                                     table pm_svg_dashes / pm_svg_dash_values, scaled by sqrt|det| like widths */

/* Beyond what make_tiger reads (d / fill / stroke / stroke-width of every <path>), pm_svg_parse
 * understands: <g>/<svg> nesting with inherited presentation properties, `transform`
 * (matrix translate scale rotate skewX skewY), `style="..."`, <style> sheets with element / .class /
 * #id selectors (presentation attributes < element < class < id rules < style attribute), opacity / fill-opacity /
 * stroke-opacity (folded into the items' alpha: no group compositing), display: none / visibility, fill-rule (evenodd ->
 * PM_PATH_EVEN_ODD), #rgb / #rrggbb / rgb() rgba() hsl() hsla() / the 147 colour keywords / none, and rect (rounded too),
 * circle, ellipse, line, polyline, polygon as paths; <use> (href / xlink:href, x, y: the referenced
 * element or <symbol>, from anywhere in the document, nested at most 8 deep); <defs> and friends
 * are not drawn where they stand; lengths in px / pt / pc / mm / cm / in and percentages of the outermost
 * viewBox.  Coordinates
 * come out in the root user space; stroke widths are scaled by sqrt|det| of the matrix. */

/* Beyond the reference (src/lib.rs:194, "need to deal with subpaths and also want curves"): the
 * encoder takes a whole kurbo-style path -- what make_tiger's encode_path / encode_path_stroke do
 * (src/lib.rs:342-367) for one BezPath under the identity transform: flatten.rs on the host
 * (tolerance 0.1), then one Fill per sub-path (or ONE compound Fill with PM_FILL_COMPOUND) resp. one
 * poly-line per sub-path with the thin-line rule.  Same bytes as pm_flatten_and_encode on that path. */
int pm_encoder_fill_path(pm_encoder *e, const pm_path_el *els, size_t n_els, uint32_t rgba, uint32_t fill_flags);
int pm_encoder_stroke_path(pm_encoder *e, const pm_path_el *els, size_t n_els, uint32_t rgba, float width);

typedef struct pm_svg pm_svg;
pm_svg *pm_svg_parse(const char *text, size_t len, int flags, int *err);
pm_svg *pm_svg_tiger(int flags, int *err); /* the embedded Ghostscript_Tiger.svg (src/lib.rs:288) */
void pm_svg_free(pm_svg *s);
size_t pm_svg_n_paths(const pm_svg *s);
size_t pm_svg_n_els(const pm_svg *s);
/* The outermost <svg>: returns 1 and fills viewbox = {min-x, min-y, width, height} if it has a valid
 * viewBox (else 0, viewbox zeroed); width / height = its size attributes in px (0: absent, or a
 * percentage).  Path coordinates stay in user space: mapping the viewBox to pixels is the caller's affine. */
int pm_svg_viewbox(const pm_svg *s, double viewbox[4], double *width, double *height);
const pm_path *pm_svg_paths(const pm_svg *s);
const pm_path_el *pm_svg_els(const pm_svg *s);
/* The dash table of the parse (empty without PM_SVG_STROKE_DASHES), as pm_flatten_and_encode_dashed takes it. */
const pm_path_dash *pm_svg_dashes(const pm_svg *s);
size_t pm_svg_n_dashes(const pm_svg *s);
const float *pm_svg_dash_values(const pm_svg *s);
size_t pm_svg_n_dash_values(const pm_svg *s);
/* pm_svg_n_paths entries: for every path the ordinal, among the element children of the outermost <svg>, of the child whose
 * subtree drew it (for a <use>: the child where the <use> stands, not where its target is defined) -- the document's top-level
 * groups, as pm_path_groups takes them (decision D16). */
const uint32_t *pm_svg_path_groups(const pm_svg *s);
uint32_t pm_parse_color(const char *s); /* parse_color src/lib.rs:375-385 */

/* ==== 3. renderer (replaces PietRenderer, TestApp/PietRenderer.{h,m}) ========= */

typedef struct pm_ctx pm_ctx;

/* -initWithMetalKitView: (PietRenderer.m:23-57): device, pipelines, 16 MiB scene
 * buffer.  Returns NULL and sets *err on failure (reference: NSLog + nil). */
pm_ctx *pm_create(int device, int *err);
void pm_destroy(pm_ctx *c);
const char *pm_last_error(void);

/* The ABI this library was built with, as 100 x round + revision: a caller compiled against this header checks
 * pm_abi_version() == PM_ABI_VERSION before it hands structs over (round-5 advisor: pm_scene_timings was 16 bytes in round 4 and is 12
 * again since round 5, and nothing at run time told the two layouts apart).  Libraries before round 6 do not export the symbol. */
#define PM_ABI_VERSION 600u
uint32_t pm_abi_version(void);

/* -mtkView:drawableSizeWillChange: (PietRenderer.m:105-146) minus the scene
 * init: (re)allocates the framebuffer and the dynamic tile grid. */
int pm_resize(pm_ctx *c, uint32_t width, uint32_t height);
/* Render only tile rows [row0,row1) of the viewport (multi-GPU sharding). The
 * framebuffer then holds just that band, row 0 = pixel row row0*16. */
int pm_set_band(pm_ctx *c, uint32_t tile_row0, uint32_t tile_row1);

/* _sceneBuf.contents (PietRenderer.m:52-53, :204): pinned host staging buffer the
 * caller encodes into; pm_upload_scene makes `bytes` of it resident in HBM. */
/* The pointer stays valid until pm_scene_reserve asks for more (or pm_destroy): uploads, device
 * flattening and nested-group scenes grow only the device copy. */
uint8_t *pm_scene_buffer(pm_ctx *c, size_t *cap);
int pm_scene_reserve(pm_ctx *c, size_t cap);
int pm_upload_scene(pm_ctx *c, size_t bytes);
/* flatten.rs moved on-device: flatten + encode make_tiger-style paths directly
 * into the device scene buffer (src/lib.rs:293-327, src/flatten.rs:10-47).
 * affine = kurbo Affine coefficients [a b c d e f]; stroke widths are multiplied
 * by `width_scale` in f32 (src/lib.rs:320).  On return the scene is resident.
 * Paths with PM_PATH_STROKE_OUTLINE get their strokes as outline Fill items (decision D14); *scene_bytes includes the outlines,
 * *n_items and pm_item_paths are what they are without the bit.  On PM_ERR_CAPACITY *scene_bytes is the size the scene would
 * have needed (0: not known).
 * Limits: n_els and n_paths <= 2^26 - 1 (PM_ERR_CAPACITY beyond). */
int pm_flatten_and_encode(pm_ctx *c, const pm_path *paths, size_t n_paths,
                          const pm_path_el *els, size_t n_els, const double affine[6],
                          float width_scale, size_t *scene_bytes, uint32_t *n_items);
/* Animation: flatten + encode the paths of the last pm_flatten_and_encode AGAIN under another
 * affine (they stay resident on the device; nothing is uploaded or allocated).  The reference
 * re-encodes on the CPU when the view changes (PietRenderer.m:90-101, :145); here a view change
 * is four small kernels plus the scene index. */
int pm_reflatten(pm_ctx *c, const double affine[6], float width_scale, size_t *scene_bytes, uint32_t *n_items);
/* Animating objects, not only the camera (decision D16): pm_reflatten with one transform PER GROUP of paths.
 * pm_path_groups assigns every resident path a group index; pm_reflatten_groups flattens path p under
 * xforms[group_of_path[p]]: its affine (kurbo order, binary64) and its width_scale (f32, NOT derived from the matrix on the
 * device: the caller's, as with pm_reflatten).  The scene is, byte for byte, what D1-D15 define when every path takes its own
 * group's two values wherever they appear (subdivision counts, points, widths, the thin-line rule, boxes, outlines, dashes);
 * item order, *n_items, pm_item_paths and the layout do not depend on the table.  A table whose entries are all equal gives
 * pm_reflatten's bytes. */
typedef struct {
    double m[6];
    float width_scale;
    uint32_t reserved; /* 0 */
} pm_group_xform;      /* 56 bytes */
/* group_of_path[n_paths]; n_paths must equal the resident path count (pm_flatten_and_encode[_dashed]).  The map stays resident
 * with the paths: a later pm_flatten_and_encode* forgets it, pm_reflatten ignores and keeps it.  PM_ERR_INVALID: no resident
 * paths, a NULL pointer, another n_paths. */
int pm_path_groups(pm_ctx *c, const uint32_t *group_of_path, size_t n_paths);
/* Same outputs, same PM_ERR_CAPACITY contract and the same grow-and-retry as pm_reflatten; the table is copied before the call
 * returns.  PM_ERR_INVALID: no resident paths or no resident map, a NULL pointer, n_groups == 0 or not above the largest index
 * of the map (a longer table is fine), a non-zero `reserved`. */
int pm_reflatten_groups(pm_ctx *c, const pm_group_xform *xforms, size_t n_groups, size_t *scene_bytes, uint32_t *n_items);
/* Fading and tinting groups of paths (decision D17): one paint per group of the resident map (pm_path_groups).
 * Path p's fill_rgba and stroke_rgba, AS THE LAST pm_flatten_and_encode* GAVE THEM (paints do not accumulate), go through
 * paints[group_of_path[p]], in integers, on the stored sRGB-encoded bytes:
 *     R, G, B:  (c * (255 - k) + t * k + 127) / 255     k = the tint's AA byte, t = the tint's channel
 *     A:        (a * opacity + 127) / 255               round to nearest, no tie (255 is odd); {0, 255} changes nothing
 * The resident scene becomes, byte for byte, the scene D1-D16 define for the painted paths under the transform(s) of the call
 * that made it: only the items' colour words change (the thin-line rule acts on the painted alpha; an outline or dashed item
 * carries the painted, thin-lined stroke colour); length, *n_items, boxes, points, pm_item_paths and paint order stay.  Nothing is
 * flattened, nothing read back, the scene index and the binning plan in force stay (pm_get_binning_plans does not move);
 * pm_get_scene_timings reports the call's host time as flatten_encode_ms and scene_index_ms = 0.  As after every scene
 * replacement, the frames rendered before the call are no longer "the last frame": pm_read_pixels / pm_framebuffer_device_ptr
 * name a frame again once one of the painted scene has been rendered.
 * This is no group compositing: an opacity multiplies every item's own alpha, as the SVG front-end folds `opacity` into the items;
 * overlapping items of a faded group show through each other.
 * The paint stays with the resident paths: a later pm_reflatten / pm_reflatten_groups flattens the painted paths;
 * pm_flatten_and_encode* forgets it; pm_path_groups does not touch it (the colours change with the next paint).
 * PM_ERR_INVALID, nothing changed: a NULL pointer, no resident paths, no resident map, n_groups == 0 or not above the largest
 * index of the map (a longer table is fine), an opacity above 255, a resident scene that did not come from the resident paths
 * (pm_upload_scene since, or the last replacement failed). */
typedef struct {
    uint32_t tint_rgba; /* 0xRRGGBBAA: RR GG BB = the colour mixed in, AA = how much of it (0 none, 255 all) */
    uint32_t opacity;   /* 0..255, multiplies the alpha; above 255: PM_ERR_INVALID */
} pm_group_paint;       /* 8 bytes; identity = {0, 255} */
int pm_repaint_groups(pm_ctx *c, const pm_group_paint *paints, size_t n_groups);
/* pm_flatten_and_encode with a dash table (decision D15): the styled stroke of every path named in `dashes` is cut into dashes
 * on the device.  A dashed stroke stays ONE compound Fill item per sub-path in the poly-line's slot -- *n_items and pm_item_paths
 * do not change -- whose entries are the D14 outlines of its dashes.  `dashes` is strictly ascending by path; PM_ERR_INVALID: an
 * index >= n_paths, a path without PM_PATH_STROKE | PM_PATH_STROKE_OUTLINE, a count of 0 or above 32, a range outside dash_values,
 * a negative or non-finite value, a non-finite offset.  With n_dashes == 0 it is pm_flatten_and_encode.  The table stays resident
 * with the paths: pm_reflatten cuts again under its width_scale; a later pm_flatten_and_encode forgets it.
 * Limits: a segment or a pattern value longer than 65 536 px counts as 65 536 px; on PM_ERR_CAPACITY *scene_bytes counts the
 * dashes only if the scene without outlines fitted (else the undashed outlines: the call that follows learns the rest). */
int pm_flatten_and_encode_dashed(pm_ctx *c, const pm_path *paths, size_t n_paths, const pm_path_el *els, size_t n_els,
                                 const pm_path_dash *dashes, size_t n_dashes, const float *dash_values, size_t n_dash_values,
                                 const double affine[6], float width_scale, size_t *scene_bytes, uint32_t *n_items);
/* Copy the resident scene back (parity checks, init_test_scene): the bytes the caller uploaded or the flatten stage wrote, without
 * the flat form a nested scene gets appended.  With no scene resident -- nothing uploaded yet, or the last replacement failed after
 * it started, a pm_reflatten_groups included -- it is PM_OK with *bytes = 0 and nothing written; pm_render, pm_fill_coverage,
 * pm_item_paths, pm_repaint_groups and every hit-test and rectangle query are PM_ERR_INVALID in that state, pm_get_stats reports n_items = 0, and the resident paths, their group map and
 * their paint stay: pm_reflatten / pm_reflatten_groups bring a scene back, painted as before. */
int pm_download_scene(pm_ctx *c, uint8_t *dst, size_t cap, size_t *bytes);

/* -drawInMTKView: (PietRenderer.m:59-103): enqueue one frame (binning + per-pixel
 * kernels) on the ctx stream; asynchronous like [commandBuffer commit]. */
int pm_render(pm_ctx *c);
/* Same, into a caller-owned device buffer (e.g. a torch tensor) on a caller
 * stream (hipStream_t; NULL = ctx stream).  stride in bytes, multiple of 4. */
int pm_render_to(pm_ctx *c, void *dev_framebuffer, size_t stride_bytes, void *hip_stream);
int pm_sync(pm_ctx *c);

#define PM_FMT_RGBA8 0
#define PM_FMT_BGRA8 1 /* the reference drawable's byte order, PietRenderer.m:29 */
/* Byte order in which pm_render / pm_render_to STORE pixels from now on: PM_FMT_RGBA8 (default) or
 * PM_FMT_BGRA8 = MTLPixelFormatBGRA8Unorm, what the reference's renderKernel writes into
 * (view.colorPixelFormat, PietRenderer.m:29) -- a caller-owned BGRA surface is then filled directly,
 * no swizzle pass.  Same pixels, R and B exchanged. */
int pm_set_target_format(pm_ctx *c, int fmt);
/* Read the (band of the) framebuffer back: height rows of width*4 bytes, in byte order `fmt`
 * (swizzled on the host if the frame was stored in the other order). */
int pm_read_pixels(pm_ctx *c, uint8_t *dst, size_t dst_stride, int fmt);
void *pm_framebuffer_device_ptr(pm_ctx *c, size_t *stride_bytes, uint32_t *rows);
/* The resident scene on the device.  Valid until the scene is next replaced (pm_upload_scene,
 * pm_flatten_and_encode, pm_reflatten): the device flatten writes the NEXT scene into a second buffer while frames
 * in flight still read this one, and the two change places -- a pointer kept across a replacement names the
 * buffer the replacement after that overwrites. */
void *pm_scene_device_ptr(pm_ctx *c, size_t *bytes);

/* Time `iters` frames with HIP events (any pointer may be NULL).
 * total_ms = the whole batch submitted back to back through the frame pipeline, as pm_render
 * does; bin/coarse/fine/clear_ms = average per-launch duration of the frame kernels
 * (pm_bin_kernel, pm_coarse_kernel, pm_fine_kernel; pm_clear_kernel only with PM_FOLD_CLEAR=0,
 * else its work is part of pm_fine_kernel's launch and clear_ms is 0), each ALONE on the GPU: a second pass
 * of `iters` frames serialized on one stream, every launch bracketed by events. */
int pm_time_frames(pm_ctx *c, int iters, float *total_ms, float *bin_ms, float *coarse_ms, float *fine_ms, float *clear_ms);
/* Same, but the per-kernel durations are taken INSIDE the pipelined batch: every launch is
 * bracketed by events on the stream it runs on while frames overlap (iters <= 4096).  These
 * are the durations a kernel trace of pm_render traffic shows. */
int pm_time_frames_pipelined(pm_ctx *c, int iters, float *total_ms, float *bin_ms, float *coarse_ms, float *fine_ms,
                             float *clear_ms);

/* Latency of ONE frame with nothing else in flight: begin of its first kernel to end of its
 * last one, two HIP events on the frame's stream around the plain launches pm_render makes (two
 * by default: pm_bin_kernel, pm_fine_kernel);
 * median and minimum over `iters` frames (SURVEY.md 8d's t_frame; PietRenderer.m has no timing
 * at all). */
int pm_frame_latency(pm_ctx *c, int iters, float *median_ms, float *min_ms);

/* Frames whose tile kernel was the one-wave-per-tile instantiation (six workgroups per CU): what frames get after a frame
 * of the same scene and viewport whose tile kernel found it dense -- long lists enough to occupy every wave (PM_DENSE_KERNEL=0: never). */
int pm_tile_kernel_info(pm_ctx *c, uint32_t *dense_frames);

/* Frames binned with ONE wave per strip row (pm_bin_kernel<.., 1>) since pm_create: out[0] all of them, out[1] those that got it only
 * because they were submitted behind running frames, out[2] of those the ones with a wave for EVERY strip row where the plan chains
 * rows for its own, smaller grid of workgroups (1 280 < strip rows <= 4 096 light ones). */
int pm_binning_info(pm_ctx *c, uint32_t out[3]);

/* The binning plan in force (the host side of tileKernel's dispatch geometry, PietRenderer.m:63-77): out[0] entries of the work list
 * (strip rows some item reaches; a strip row cut in two counts twice), out[1] strip rows cut in two -- the heaviest rows, binned by two
 * workgroups side by side (tiles 0-7 and 8-15) while the resident grid has workgroups to spare --, out[2] plans remade since pm_create
 * from what the frames' binning kernels reported (segment slots per strip row), out[3] 1 if the plan in force was made from such a report. */
int pm_binning_plan_info(pm_ctx *c, uint32_t out[4]);

/* One launch per frame (pm_frame_kernel: the two dispatches of PietRenderer.m:69-88 as roles of one resident
 * grid).  *frames = frames submitted that way since pm_create; *applies = 1 if a frame of the resident scene
 * and viewport, alone on the device, would be (0: two launches -- PM_ONE_LAUNCH=0, more strip rows than resident
 * workgroups, per-tile-row item lists, or a one-launch frame once gave up waiting). */
int pm_one_launch_info(pm_ctx *c, uint32_t *frames, int *applies);
/* Duration of that launch, frame alone, from events carried by the dispatch itself (what a kernel trace shows);
 * average over `iters` frames.  PM_ERR_INVALID when *applies is 0. */
int pm_time_one_launch(pm_ctx *c, int iters, float *kernel_ms);
/* Developer hook: one one-launch frame by its profiling instantiation -- per workgroup 32 x u64 (10 ns clocks and
 * counts, layout at pm_frame_kernel in pm_frame.hip); *n_wgs = the launch's workgroups. */
int pm_debug_time_frame(pm_ctx *c, uint64_t *out, size_t max_wgs, size_t *n_wgs);

/* Developer hook: the lone frame taken apart -- medians over `iters` frames of {pm_bin_kernel,
 * gap, pm_coarse_kernel, gap, pm_fine_kernel, first begin -> last end}, ms, from events attached to
 * the dispatches (which stretch the gaps: a breakdown, not t_frame -- that is pm_frame_latency;
 * needs the default PM_FOLD_CLEAR=1; the coarse entries are 0 in the default fused path). */
int pm_debug_frame_timeline(pm_ctx *c, int iters, float *out6);

typedef struct {
    uint32_t tiles_x, tiles_y;    /* tile grid of the viewport */
    uint32_t band_row0, band_row1;
    uint32_t n_items;             /* scene items */
    uint32_t queued_tiles;        /* tiles handed to the per-tile kernel last frame */
    uint32_t arena_used_dwords;   /* binning arena: dwords of records written last frame */
    uint32_t arena_cap_dwords;
    uint32_t overflow;            /* 1 if the last frame ran out of arena */
    uint32_t scene_bytes;
    uint32_t heavy_tiles;         /* of queued_tiles: scheduled first (long segment streams) */
    uint32_t ptcl_used_cmds;      /* tile arena: 16-byte quads reserved last frame (per-tile pieces + command
                                     lists, a 24-byte command = 1.5 quads), summed over the arena's parts */
} pm_stats;
int pm_get_stats(pm_ctx *c, pm_stats *out); /* synchronises */

/* ==== 4. multi-GPU presentation (new: the reference is single-device, PietRenderer.m:27) =====
 * One process and one pm_ctx per GPU, each rendering a band of tile rows (pm_set_band); the
 * bands meet once, here: a grouped ncclSend/ncclRecv over RCCL (xGMI inside a node) puts every
 * rank's band straight into its rows of the root's final image.  RCCL is bound
 * with dlopen at the first call: the copy the process has mapped already if there is one (a host
 * that also runs torch.distributed keeps ONE RCCL), else librccl.so.1; PM_RCCL_LIB overrides. */
#define PM_COMM_ID_BYTES 128 /* = sizeof(ncclUniqueId) */
typedef struct pm_comm pm_comm;
/* Rank 0 makes the id; the host carries it to the other ranks (file, env, MPI, a torch store). */
int pm_comm_unique_id(uint8_t id[PM_COMM_ID_BYTES]);
/* Collective over all `world` ranks (ncclCommInitRank on the context's device). */
pm_comm *pm_comm_create(pm_ctx *c, const uint8_t id[PM_COMM_ID_BYTES], int rank, int world, int *err);
void pm_comm_destroy(pm_comm *m);
/* What got bound: the path of the shared object ncclCommInitRank came from (lib_path, NUL-terminated,
 * truncated to lib_path_cap) and ncclCommCount of the communicator (*ranks; 0 when m is NULL).  Either
 * output may be NULL.  Loads RCCL like the other calls; not a collective. */
int pm_comm_info(pm_comm *m, char *lib_path, size_t lib_path_cap, int *ranks);
/* Collective.  band_tile_rows = {row0, row1} per rank (2*world entries, what each rank passed to
 * pm_set_band; a rank whose own entry is empty, row0 == row1, sends nothing and may pass any context
 * of the device -- a band gathered in sub-bands, one context each, pipelined under the render).  src_band = this rank's band (NULL: the context's last frame), tightly packed
 * rows of width*4 bytes; dst_image (root only) = the full width*4 x height image.  Asynchronous
 * on hip_stream (NULL: the context's stream); ordered behind the last frame when src_band is NULL.
 * Errors: an argument error (PM_ERR_INVALID for bad rows, strides or a root without dst_image) is
 * returned before anything is posted -- if only SOME ranks fail that way the others wait for them, so
 * tear the communicator down; a root whose own band cannot be placed (overlap, copy failure) still
 * posts its receives, so that the peers' sends complete, and reports the error afterwards. */
int pm_gather(pm_ctx *c, pm_comm *m, const void *src_band, size_t src_stride, const uint32_t *band_tile_rows, int root,
              void *dst_image, size_t dst_stride, void *hip_stream);

/* Host wall-clock cost of the last scene replacement ("flatten+encode timed
 * separately"): the reference does this work once per resize on the CPU (src/lib.rs:286-328,
 * PietRenderer.m:145) and never times it.
 *   flatten_encode_ms  pm_flatten_and_encode: the four flatten kernels incl. their scan
 *                      read-backs and buffer management (0 after pm_upload_scene)
 *   scene_index_ms     header/item read-back, validation, chunk index (pm_index_kernel)
 *   arena_setup_ms     per-(scene, viewport, band) binning-arena sizing on the host, paid by the
 *                      first pm_render after a scene or viewport change */
typedef struct {
    float flatten_encode_ms, scene_index_ms, arena_setup_ms;
} pm_scene_timings; /* 12 bytes, as in round 3: the struct does not grow (a caller built against an older header owns 12 bytes) */
int pm_get_scene_timings(pm_ctx *c, pm_scene_timings *out);
/* Binning plans made since pm_create (strip-row regions sized, lists uploaded): a scene after pm_reflatten keeps the
 * plan in force while every item stays inside the box it was planned with -- one tile wider on each side -- and
 * keeps its segment count.  (Round 4 had this counter as a fourth member of pm_scene_timings; a getter of its own
 * since round 5: ABI note in INTEGRATION.md.) */
int pm_get_binning_plans(pm_ctx *c, uint32_t *plans);

/* Debug/parity hook: re-run the last frame's per-tile kernel with command
 * capture and return every tile's command list in the reference's 24-byte
 * format (TestApp/GenTypes.h:430-495), including the trailing End / the lone
 * Bail.  counts[tiles] and solid[tiles] are per tile (band-relative, row-major);
 * cmds receives max_cmds_per_tile * tiles entries.  Lists longer than
 * max_cmds_per_tile are truncated (count still reports the full length). */
typedef struct {
    uint32_t tag;
    uint32_t body[5];
} pm_cmd;
int pm_debug_capture_ptcl(pm_ctx *c, uint32_t max_cmds_per_tile, uint32_t *counts,
                          uint32_t *solid, pm_cmd *cmds);

/* Winding coverage (alpha before colour) of ONE Fill item of the resident scene over the viewport
 * band, accumulated in f32 instead of the frame path's binary16 (the reference declares
 * signedArea `half`, TestApp/PietRender.metal:472; north star: "coverage within 1 ULP of the f32
 * reference").  The item is binned and encoded alone, exactly as a frame would, then its commands
 * are evaluated per pixel in binary32.  dst = rows of `width` floats, row stride in floats.
 * A validation call: it synchronises and rebuilds the scene index twice. */
int pm_fill_coverage(pm_ctx *c, uint32_t item_ix, float *dst, size_t dst_stride_floats);

/* ==== point hit testing (new: the reference has none; DESIGN.md 2, decision D13, says what "contains" means) ====
 * Independent of pm_resize / pm_set_band / pm_set_target_format (a context with a scene and no viewport answers too);
 * frames in flight are not disturbed. */
#define PM_HIT_NONE 0xffffffffu
#define PM_HIT_SKIP_TRANSPARENT 1u   /* items whose colour has alpha 0 are not hit (Circles are opaque black) */

/* xy = n points {x, y} in scene coordinates (= pixels; the centre of pixel (px, py) is (px + 0.5, py + 0.5)).
 * top_item[k] = index, in flat paint order (what pm_stats.n_items counts: nested groups inlined depth first),
 * of the LAST-painted item that contains point k, or PM_HIT_NONE.  n_hit (may be NULL) = how many items contain it.
 * A point with a non-finite coordinate hits nothing.  n == 0 is PM_OK; unknown flag bits and a context without a
 * resident scene are PM_ERR_INVALID.  Synchronises. */
int pm_hit_test(pm_ctx *c, const float *xy, size_t n, uint32_t flags, uint32_t *top_item, uint32_t *n_hit);

/* Same on device memory (e.g. torch tensors), asynchronous on hip_stream (NULL: the context's stream).  It reads the scene
 * that is resident when it is called: a later scene replacement waits for it before anything it reads is overwritten. */
int pm_hit_test_device(pm_ctx *c, const void *dev_xy, size_t n, uint32_t flags,
                       void *dev_top_item, void *dev_n_hit, void *hip_stream);

/* The item map of a pixel rectangle (decision D18): for pixel (x0 + i, y0 + j), 0 <= i < w, 0 <= j < h, what pm_hit_test answers
 * for the point (x0 + i + 0.5f, y0 + j + 0.5f) -- top_item[j * stride + i] (and n_hit[j * stride + i] if n_hit != NULL), decision
 * D13, same flags.  stride in 32-bit elements, >= w.  Words outside the w x h rectangle are not written.  w == 0 or h == 0 is
 * PM_OK and writes nothing.  PM_ERR_INVALID, before anything is enqueued: unknown flag bits, no resident scene, x0 + w > 65536 or
 * y0 + h > 65536 (the viewport limit; every centre is then exact in f32), stride < w, a NULL top_item when w * h > 0.
 * Needs a scene, no viewport; independent of pm_resize / pm_set_band / pm_set_target_format; frames in flight are not
 * disturbed.  One workgroup per 16 x 16 tile shares the item cull and the segment stream (pm_hit_frame_kernel): the tiling
 * does not show in the result.  Synchronises. */
int pm_hit_frame(pm_ctx *c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t flags,
                 uint32_t *top_item, uint32_t *n_hit, size_t stride);

/* Same on device memory, asynchronous on hip_stream (NULL: the context's stream), ordered as pm_hit_test_device is: it reads
 * the scene that is resident when it is called, and a later scene replacement waits for it. */
int pm_hit_frame_device(pm_ctx *c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t flags,
                        void *dev_top_item, void *dev_n_hit, size_t stride, void *hip_stream);

/* ==== rectangle queries: pick with a tolerance, marquee selection (decision D19) ====
 * A closed rectangle R = {x0, y0, x1, y1} in scene coordinates TOUCHES an item if the item's shape -- edges included, strokes with
 * their width -- has a point in common with R, and ENCLOSES it if all of the shape lies in R.  x0 == x1 and / or y0 == y1 is a
 * valid rectangle (a segment, a point); one with a non-finite value, or with x1 < x0 or y1 < y0, touches and encloses nothing
 * (not an error).  Same flags, same argument rules and same independence of the viewport as pm_hit_test.
 *
 * pm_hit_rects: for each of n rectangles, top_item[k] = the LAST-painted item rectangle k touches, or PM_HIT_NONE; n_hit (may be
 * NULL) = how many it touches.  A pick with tolerance t around (x, y) is the rectangle {x - t, y - t, x + t, y + t}.
 * Synchronises. */
int pm_hit_rects(pm_ctx *c, const float *rects /* n x {x0, y0, x1, y1} */, size_t n, uint32_t flags,
                 uint32_t *top_item, uint32_t *n_hit);
/* Same on device memory, asynchronous on hip_stream (NULL: the context's stream), ordered as pm_hit_test_device is. */
int pm_hit_rects_device(pm_ctx *c, const void *dev_rects, size_t n, uint32_t flags,
                        void *dev_top_item, void *dev_n_hit, void *hip_stream);

#define PM_SEL_TOUCHES 1u
#define PM_SEL_ENCLOSES 2u
/* pm_select_rect: ONE rectangle against every item, occluded ones included: item_flags[i] = PM_SEL_* of item i in flat paint
 * order.  *n_items (may be NULL, like the two counts) is always set; PM_ERR_CAPACITY if cap < n_items, and then nothing else is
 * written.  Words beyond n_items are not written.  Synchronises. */
int pm_select_rect(pm_ctx *c, const float rect[4], uint32_t flags, uint32_t *item_flags, size_t cap,
                   uint32_t *n_items, uint32_t *n_touched, uint32_t *n_enclosed);
/* Same into device memory (the rectangle itself is read from the host before the call returns), asynchronous on hip_stream,
 * ordered as pm_hit_test_device is. */
int pm_select_rect_device(pm_ctx *c, const float rect[4], uint32_t flags, void *dev_item_flags, size_t cap, void *hip_stream);

/* ==== hit stacks: the k topmost items under a point or a pick square (decision D24) ====
 * Select-behind, "the objects under the cursor".  H = the items that contain point q as pm_hit_test means it (pm_hit_stack), or
 * that rectangle q touches as pm_hit_rects means it (pm_hit_rects_stack), PM_HIT_SKIP_TRANSPARENT and invalid queries (a non-finite
 * value, an inverted rectangle: H is empty) included, ordered topmost first: item index descending.  With PM_HIT_STOP_AT_OPAQUE the
 * sequence ends at its first OPAQUE member, which is included: a Circle or ellipse always is, a Line, Fill or Polyline if the alpha
 * byte of its colour is 255 (the stored byte and the geometric containment, not the frame's coverage: an item that covers a pixel
 * partly still ends the stack); if no member is opaque the sequence is all of H.  m = its length.
 * items[q * k + j] = its j-th member for j < min(k, m), PM_HIT_NONE for min(k, m) <= j < k: all k words of every query are written,
 * none beyond n * k.  n_hit[q] (may be NULL) = m, not clipped by k.  With k = 1 and no PM_HIT_STOP_AT_OPAQUE, items and n_hit are
 * pm_hit_test's (pm_hit_rects') top_item and n_hit.  PM_ERR_INVALID, before anything is enqueued: k == 0 or k > PM_HIT_STACK_MAX,
 * flag bits other than these two, a NULL items or input with n > 0, no resident scene.  n == 0 is PM_OK.  Every other call refuses
 * PM_HIT_STOP_AT_OPAQUE as an unknown bit.  Independent of the viewport as pm_hit_test is.  Synchronises. */
#define PM_HIT_STOP_AT_OPAQUE 8u
#define PM_HIT_STACK_MAX 256u
int pm_hit_stack(pm_ctx *c, const float *xy, size_t n, uint32_t k, uint32_t flags, uint32_t *items /* n * k */, uint32_t *n_hit /* n, or NULL */);
int pm_hit_rects_stack(pm_ctx *c, const float *rects /* n x {x0, y0, x1, y1} */, size_t n, uint32_t k, uint32_t flags, uint32_t *items, uint32_t *n_hit);
/* Same on device memory, asynchronous on hip_stream (NULL: the context's stream), ordered as pm_hit_test_device is. */
int pm_hit_stack_device(pm_ctx *c, const void *dev_xy, size_t n, uint32_t k, uint32_t flags, void *dev_items, void *dev_n_hit, void *hip_stream);
int pm_hit_rects_stack_device(pm_ctx *c, const void *dev_rects, size_t n, uint32_t k, uint32_t flags, void *dev_items, void *dev_n_hit, void *hip_stream);

/* ==== coverage counts: covered and visible pixels per item (decision D28) ====
 * "How much of this item can be seen at all": a layer panel's hidden objects, dropping occluded items before export, pixel areas, a
 * pixel to scroll to.  For the pixel rectangle (x0, y0, w, h) let H(p) be the items that contain the centre of pixel p as pm_hit_frame
 * means it (PM_HIT_SKIP_TRANSPARENT included); an item is OPAQUE as pm_hit_stack means it (a Circle or ellipse always, a Line, Fill
 * or Polyline if the alpha byte of its colour is 255).  One record per item i in flat paint order:
 *   covered        pixels p with i in H(p);
 *   visible        pixels with i in H(p) and no opaque j > i in H(p): i is in pm_hit_stack's answer at that centre with
 *                  PM_HIT_STOP_AT_OPAQUE and unbounded k;
 *   top            pixels with i = max H(p): the histogram of pm_hit_frame's top_item;
 *   first_visible  the smallest j * w + i' over the pixels (x0 + i', y0 + j) counted in visible, PM_HIT_NONE if there are none.
 * top <= visible <= covered; the counts add up over disjoint rectangles.  Integer sums and a minimum: the bytes do not depend on the
 * launch.  With PM_COVERAGE_VISIBLE_ONLY, a flag of these two calls alone (every other call refuses it as unknown), covered is DEFINED
 * to equal visible and the walk of a tile may end once all of it lies under opaque items: "which items are hidden", cheaply.
 * Output discipline is pm_item_bounds': *n_items (may be NULL) is always set; PM_ERR_CAPACITY if cap < n_items, and then nothing is
 * written; records beyond n_items are not written.  The call initialises the records it writes: it never accumulates.  w == 0 or
 * h == 0 is PM_OK and writes n_items records {0, 0, 0, PM_HIT_NONE}.  PM_ERR_INVALID, before anything is enqueued: flag bits other
 * than these two, no resident scene, x0 + w > 65536 or y0 + h > 65536, w * h > 2^32 - 1 (the counts are 32-bit), a NULL out with
 * n_items > 0.  Independent of the viewport as pm_hit_frame is; frames in flight are not disturbed.  Synchronises. */
#define PM_COVERAGE_VISIBLE_ONLY 16u
typedef struct { uint32_t covered, visible, top, first_visible; } pm_coverage;   /* 16 bytes */
int pm_item_coverage(pm_ctx *c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t flags, pm_coverage *out, size_t cap,
                     uint32_t *n_items);
/* Same into device memory (4-byte aligned, else PM_ERR_INVALID), asynchronous on hip_stream (NULL: the context's stream), ordered as
 * pm_hit_test_device is. */
int pm_item_coverage_device(pm_ctx *c, uint32_t x0, uint32_t y0, uint32_t w, uint32_t h, uint32_t flags, void *dev_out, size_t cap,
                            void *hip_stream);

/* ==== polygon queries: lasso selection, a marquee in a rotated view (decision D20) ====
 * The query polygon K has m vertices xy = m x {x, y} in scene coordinates, 3 <= m <= PM_POLYGON_MAX_VERTICES (else
 * PM_ERR_INVALID), and closes itself.  K TOUCHES an item if the item's outline reaches K's boundary, a point of the item lies in
 * K, or -- a Fill -- K's first vertex lies in the Fill; it ENCLOSES the item if the outline does not reach the boundary and every
 * point of the item lies in K (strict at the boundary: an item that only reaches an edge of K is touched, not enclosed).  The
 * inside of K is by the non-zero rule, with PM_SEL_EVEN_ODD in flags by the even-odd rule; PM_HIT_SKIP_TRANSPARENT as in
 * pm_select_rect.  Zero area, repeated vertices and self-intersections are valid; a polygon with a non-finite vertex touches and
 * encloses nothing (not an error).  Output discipline, argument rules and independence of the viewport are pm_select_rect's.
 * Synchronises. */
#define PM_POLYGON_MAX_VERTICES 4096u
#define PM_SEL_EVEN_ODD 2u   /* a flag of the polygon calls alone: the rectangle calls reject it */
int pm_select_polygon(pm_ctx *c, const float *xy /* m x {x, y}, host */, size_t m, uint32_t flags,
                      uint32_t *item_flags, size_t cap, uint32_t *n_items, uint32_t *n_touched, uint32_t *n_enclosed);
/* Same into device memory, asynchronous on hip_stream, ordered as pm_hit_test_device is.  The vertices are read from the host
 * before the call returns: every call's kernel sees its own polygon, whatever streams the calls go to.  They wait in one of
 * four staging slots of the context: a fifth call while four are still in flight blocks the host until the oldest of them has
 * run (nothing is allocated per call). */
int pm_select_polygon_device(pm_ctx *c, const float *xy /* host */, size_t m, uint32_t flags,
                             void *dev_item_flags, size_t cap, void *hip_stream);

/* ==== snapping: the nearest vertex or edge to a cursor (decision D21) ====
 * A query is {x, y, r} in scene coordinates; out[k] names the nearest piece of geometry within r of query k's point: the item
 * (flat paint order), PM_SNAP_KIND_VERTEX with the vertex's index in the item and its coordinates, or PM_SNAP_KIND_EDGE with the
 * index of the segment (the entry index of its start), the parameter t in [0, 1] along it and the nearest point {x, y}; d2 is
 * the squared distance in binary64.  Fills, Polylines and Lines offer their finite points and their segments (a Fill's closing
 * segments included), a Circle or an ellipse its centre (vertex 0); a stroke's width plays no part.  Among equal distances the
 * topmost item wins, then the smallest index.  With both PM_SNAP_VERTICES and PM_SNAP_EDGES a vertex within r wins over every
 * edge, a nearer one included.  Nothing within r, a non-finite value or r < 0 (not an error): item = PM_HIT_NONE and every
 * other byte 0.
 * skip_items: NULL with n_skip == 0, or one word per item (n_skip >= n_items): a non-zero word takes that item out of the search
 * -- the words pm_select_rect_device / pm_select_polygon_device wrote can be handed to pm_snap_device as they are.
 * PM_ERR_INVALID, before anything is enqueued: unknown flag bits, neither PM_SNAP_VERTICES nor PM_SNAP_EDGES, no resident scene,
 * a skip_items / n_skip that break the rule above, a NULL xyr or out with n != 0.  n == 0 is PM_OK and writes nothing; records
 * beyond n are not written.  Independent of the viewport as pm_hit_test is; frames in flight are not disturbed.  Synchronises. */
#define PM_SNAP_VERTICES 2u
#define PM_SNAP_EDGES 4u           /* at least one of the two, else PM_ERR_INVALID; PM_HIT_SKIP_TRANSPARENT (1) as in pm_hit_test */
#define PM_SNAP_KIND_VERTEX 1u
#define PM_SNAP_KIND_EDGE 2u
typedef struct { uint32_t item, kind, index; float t; float x, y; double d2; } pm_snap_result;   /* 32 bytes */

int pm_snap(pm_ctx *c, const float *xyr /* n x {x, y, r} */, size_t n, uint32_t flags,
            const uint32_t *skip_items, size_t n_skip, pm_snap_result *out);
/* Same on device memory (dev_out 8-byte aligned), asynchronous on hip_stream (NULL: the context's stream), ordered as
 * pm_hit_rects_device is. */
int pm_snap_device(pm_ctx *c, const void *dev_xyr, size_t n, uint32_t flags,
                   const void *dev_skip_items, size_t n_skip, void *dev_out, void *hip_stream);

/* ==== snapping to intersections: the nearest crossing of two edges (decision D23) ====
 * A query is {x, y, r} as in pm_snap; out[k] names the nearest point within r of query k's point where two edges of the scene
 * cross.  The edges are pm_snap's: a Fill's segments (closing ones included), a Polyline's, a Line's one; Circles and ellipses
 * offer none, a stroke's width plays no part, styled and dashed strokes are the outline Fills they are.  An edge is NEAR iff
 * pm_snap's own distance to it is within r; only pairs of near edges are looked at (a crossing within r lies on two of them).
 * Two edges that share an end point are no pair -- where they meet is a vertex, which pm_snap offers --, nor are parallel,
 * collinear or degenerate ones; an end point ON the other edge (a T-junction) counts.  kind = PM_SNAP_KIND_INTERSECTION:
 * item / index / t name the first edge and the parameter of the crossing along it, item2 / index2 / u the second, {x, y} is the
 * point, d2 its squared distance in binary64.  The first edge is the one of the topmost item, then of the smaller index; among
 * equal distances the pair whose first edge is topmost (then of the smallest index) wins, then the same of the second edge.
 * n_near is the number of near edges.  If it exceeds PM_SNAP_MAX_NEAR_EDGES no pair is looked at: item = PM_HIT_NONE, kind =
 * PM_SNAP_KIND_TOO_MANY, n_near the full count, every other byte 0 -- ask again with a smaller r.  No crossing within r: item =
 * PM_HIT_NONE, n_near the count, every other byte 0.  A non-finite value or r < 0 (not an error): item = PM_HIT_NONE and every
 * other byte 0.
 * flags: PM_HIT_SKIP_TRANSPARENT or 0, any other bit is PM_ERR_INVALID.  skip_items, the other argument rules, the output
 * discipline and the ordering are pm_snap's.  Synchronises. */
#define PM_SNAP_KIND_INTERSECTION 3u
#define PM_SNAP_KIND_TOO_MANY 4u
#define PM_SNAP_MAX_NEAR_EDGES 512u
typedef struct { uint32_t item, kind, index; float t; float x, y; double d2; uint32_t item2, index2; float u; uint32_t n_near; } pm_snap_cross_result;   /* 48 bytes */

int pm_snap_intersections(pm_ctx *c, const float *xyr /* n x {x, y, r} */, size_t n, uint32_t flags,
                          const uint32_t *skip_items, size_t n_skip, pm_snap_cross_result *out);
/* Same on device memory (dev_out 8-byte aligned), asynchronous on hip_stream (NULL: the context's stream), ordered as
 * pm_snap_device is. */
int pm_snap_intersections_device(pm_ctx *c, const void *dev_xyr, size_t n, uint32_t flags,
                                 const void *dev_skip_items, size_t n_skip, void *dev_out, void *hip_stream);

/* ==== bounds: item, selection and group boxes (decision D22) ====
 * The bounds of an item are four binary64 values {x0, y0, x1, y1}: the minimum and maximum of its points (a Fill's non-separator
 * points; a Line's or Polyline's points -+ half its width, the width taken literally; a Circle's centre -+ its radius, an ellipse's
 * -+ rx, ry), a NaN coordinate ignored, an infinity a value like any other.  An item without points, a stroke of NaN width, an
 * ellipse with rx <= 0 or ry <= 0 and an item PM_HIT_SKIP_TRANSPARENT skips have the EMPTY box {+inf, +inf, -inf, -inf}, the
 * identity of the union.  A bound that is a zero is always +0.  A box is BOXED iff x0 <= x1 and y0 <= y1.  For an item of finite
 * points and a finite width >= 0, pm_select_rect reports PM_SEL_ENCLOSES for a rectangle R iff the item is boxed and its box lies in
 * R.  Exact within the coordinate bound of DESIGN.md 9 (|v| <= 3.0e38).
 *
 * pm_item_bounds: one record per item in flat paint order.  Output discipline is pm_select_rect's: *n_items (may be NULL) is always
 * set; PM_ERR_CAPACITY if cap < n_items, and then nothing is written; records beyond n_items are not written.  Synchronises. */
typedef struct { double x0, y0, x1, y1; } pm_bounds;                              /* 32 bytes */
typedef struct { pm_bounds box; uint32_t n_items, n_boxed; } pm_label_bounds;     /* 40 bytes */
int pm_item_bounds(pm_ctx *c, uint32_t flags, pm_bounds *out, size_t cap, uint32_t *n_items);
/* Same into device memory (dev_out 8-byte aligned), asynchronous on hip_stream (NULL: the context's stream), ordered as
 * pm_hit_rects_device is. */
int pm_item_bounds_device(pm_ctx *c, uint32_t flags, void *dev_out, size_t cap, void *hip_stream);

/* pm_union_bounds: out[l], 0 <= l < n_labels, = the union of the bounds of every item that takes part with label l, how many items
 * those are (n_items) and how many of them are boxed (n_boxed).  Item i takes part iff the flags do not skip it, item_words is NULL
 * or item_words[i] & word_mask is non-zero -- the words pm_select_rect_device / pm_select_polygon_device wrote go in as they are,
 * word_mask PM_SEL_TOUCHES, PM_SEL_ENCLOSES or both --, and its label is below n_labels.  label_of_item NULL: every item has label
 * 0 (with n_labels == 1: a selection's box and size in one record).  A label nobody carries gets the empty box and two zeros; all
 * n_labels records are always written.  PM_ERR_INVALID, before anything is enqueued: unknown flag bits (PM_HIT_SKIP_TRANSPARENT is
 * the only one), no resident scene, n_labels == 0, item_words with n_words < n_items or word_mask == 0, label_of_item with
 * n_label_words < n_items, a NULL out.  Independent of the viewport; frames in flight are not disturbed.  Synchronises. */
int pm_union_bounds(pm_ctx *c, uint32_t flags,
                    const uint32_t *item_words, size_t n_words, uint32_t word_mask,
                    const uint32_t *label_of_item, size_t n_label_words, uint32_t n_labels,
                    pm_label_bounds *out);
/* Same on device memory (dev_out 8-byte aligned, else PM_ERR_INVALID), asynchronous on hip_stream, ordered as pm_hit_rects_device
 * is.  The records are their own accumulators: nothing is allocated or staged. */
int pm_union_bounds_device(pm_ctx *c, uint32_t flags,
                           const void *dev_item_words, size_t n_words, uint32_t word_mask,
                           const void *dev_label_of_item, size_t n_label_words, uint32_t n_labels,
                           void *dev_out, void *hip_stream);

/* ==== path measurement: lengths and points at a length (decision D25) ====
 * Lengths are unsigned 64-bit integers in units of 2^-16 px, D15's: a segment's is min(floor(len * 65536 + 0.5), 2^32) of its
 * binary64 length (0 if that is a NaN), an item's the sum over its segments.  The segments of an item are named by their index k
 * as pm_snap names edges: a Line has segment 0, a Polyline k from point k to point k + 1, a Fill every entry that starts a segment,
 * closing ones included, a compound Fill's sub-paths one after another.  A Circle, an ellipse, a Fill of no points, an item
 * PM_HIT_SKIP_TRANSPARENT skips and an item index >= n_items have kind PM_MEASURE_NONE, no segment and length 0.  A styled or
 * dashed stroke is the outline Fill it is; a circle's circumference is not offered.
 *
 * pm_item_lengths: one record {length, n_segments, kind} per item in flat paint order.  Output discipline is pm_item_bounds':
 * *n_items (may be NULL) is always set; PM_ERR_CAPACITY if cap < n_items, and then nothing is written.  Synchronises.
 *
 * pm_points_at_length: out[k] = the point at position q[k].s (any u64) along item q[k].item, on the segment `index` whose
 * [Q, Q + q) holds s (only segments of a length own positions): {x, y} = a + (b - a) * t in binary64, rounded once, t the
 * parameter along the segment, {tx, ty} the unit direction of the segment.  s beyond the item's length T answers with the end of
 * the last segment of a length (t = 1) and PM_MEASURE_CLAMPED iff s > T.  An item of length 0 that has a point answers with its
 * first point, t = 0, direction (0, 0), PM_MEASURE_FOUND | PM_MEASURE_DEGENERATE (and PM_MEASURE_CLAMPED iff s > 0).  An item
 * without a walk or without a point: item = PM_HIT_NONE and every other byte 0.  If the located segment has a non-finite end,
 * item, status and index are as defined and the five floats are unspecified.
 *
 * pm_positions_on_edges: the inverse -- out[k].s = Q_index + min(floor(t * q_index + 0.5), q_index) for the point at parameter t
 * of segment `index` of the item, what pm_snap reports as (item, index, t) for an edge and (item, index, 0) for a vertex of a
 * Polyline or a Line; status PM_MEASURE_FOUND.  An index that names no segment of the item, t outside [0, 1] or a NaN:
 * item = PM_HIT_NONE and every other byte 0.
 *
 * flags: PM_HIT_SKIP_TRANSPARENT or 0.  PM_ERR_INVALID, before anything is enqueued: any other flag bit, no resident scene, a NULL
 * q or out with n != 0, a query whose `reserved` is not 0 (the _device variants cannot look: there such a query answers
 * PM_HIT_NONE).  n == 0 is PM_OK and writes nothing; records beyond n are not written.  Independent of the viewport; frames in
 * flight are not disturbed.  Synchronise. */
#define PM_MEASURE_NONE 0u         /* pm_item_length.kind */
#define PM_MEASURE_OPEN 1u
#define PM_MEASURE_CLOSED 2u
#define PM_MEASURE_FOUND 1u        /* status bits */
#define PM_MEASURE_CLAMPED 2u
#define PM_MEASURE_DEGENERATE 4u
typedef struct { uint64_t length; uint32_t n_segments, kind; } pm_item_length;                             /* 16 bytes */
typedef struct { uint32_t item, reserved; uint64_t s; } pm_length_query;                                   /* 16 bytes */
typedef struct { uint32_t item, status, index; float t; float x, y; float tx, ty; } pm_length_point;       /* 32 bytes */
typedef struct { uint32_t item, index; float t; uint32_t reserved; } pm_edge_query;                        /* 16 bytes */
typedef struct { uint64_t s; uint32_t item, status; } pm_length_at;                                        /* 16 bytes */

int pm_item_lengths(pm_ctx *c, uint32_t flags, pm_item_length *out, size_t cap, uint32_t *n_items);
int pm_points_at_length(pm_ctx *c, const pm_length_query *q, size_t n, uint32_t flags, pm_length_point *out);
int pm_positions_on_edges(pm_ctx *c, const pm_edge_query *q, size_t n, uint32_t flags, pm_length_at *out);
/* Same on device memory (every pointer 8-byte aligned), asynchronous on hip_stream (NULL: the context's stream), ordered as
 * pm_hit_rects_device is.  A pm_snap_result {item, kind, index, t, ...} becomes a pm_edge_query {item, index, t, 0} by moving three
 * of its words, which can be done on the device: no read-back stands between a snap and its position. */
int pm_item_lengths_device(pm_ctx *c, uint32_t flags, void *dev_out, size_t cap, void *hip_stream);
int pm_points_at_length_device(pm_ctx *c, const void *dev_q, size_t n, uint32_t flags, void *dev_out, void *hip_stream);
int pm_positions_on_edges_device(pm_ctx *c, const void *dev_q, size_t n, uint32_t flags, void *dev_out, void *hip_stream);

/* ==== resampling: evenly spaced points along items in one call (decision D26) ====
 * A request names `count` positions s_0 .. s_{count-1} along `item`, u64 in the unit of path measurement, 2^-16 px, and the record
 * out[first + j], j < count, is byte for byte what pm_points_at_length answers for {item, 0, s_j} under the same flags: clamped,
 * degenerate and "none" answers and the unspecified five floats on a segment with a non-finite end included.  Nothing new is said
 * about what a point is; what is new is that the device makes the positions and walks the item once for all of them.
 *
 *   PM_RESAMPLE_STEP  s_j = start + j * step, saturating at 2^64 - 1.  step == 0 is allowed: all positions coincide.
 *   PM_RESAMPLE_EVEN  start and step must be 0.  T is the item's length (pm_item_lengths); m = count - 1 if the item's kind is
 *                     PM_MEASURE_OPEN (the last sample is the end), m = count if it is PM_MEASURE_CLOSED (sample `count` would be
 *                     the start again), and s_j = j * (T div m) + min(j, T mod m) in u64 -- every s_j = 0 where m == 0 and for an
 *                     item without a walk.  Neighbouring gaps differ by at most one unit, and s_m = T exactly.
 *
 * count <= PM_RESAMPLE_MAX_COUNT.  Every request gets a pm_resample_info {length = T, n_unclamped, kind}: kind the item's
 * PM_MEASURE_* kind, n_unclamped how many of the request's `count` positions have an answer that is not "none" and lacks
 * PM_MEASURE_CLAMPED -- in step mode how many markers fit.  It counts positions, whether or not out_cap let their records be written.
 * A request the device cannot answer -- mode > 1, count > PM_RESAMPLE_MAX_COUNT, PM_RESAMPLE_EVEN with a non-zero start or step --
 * writes no point record at all and has the info {0, 0, PM_RESAMPLE_INVALID}.
 *
 * pm_resample_items: the records are packed: q[k].first must be the sum of the counts before it, the total at most out_cap.
 * flags: PM_HIT_SKIP_TRANSPARENT or 0.  PM_ERR_INVALID, before anything is enqueued: any other flag bit, no resident scene, a NULL q,
 * out or info with n != 0, a request the device would call invalid, a wrong `first`.  PM_ERR_CAPACITY, with nothing written: the
 * total exceeds out_cap or 2^20 records (what pm_points_at_length stages at a time).  n == 0 is PM_OK and writes nothing.
 * Independent of the viewport; frames in flight are not disturbed.  Synchronises. */
#define PM_RESAMPLE_STEP 0u            /* pm_resample_query.mode */
#define PM_RESAMPLE_EVEN 1u
#define PM_RESAMPLE_MAX_COUNT 1048576u /* 2^20 */
#define PM_RESAMPLE_INVALID 0xffffffffu /* pm_resample_info.kind of a request that cannot be answered */
typedef struct { uint32_t item, mode, count, first; uint64_t start, step; } pm_resample_query;             /* 32 bytes */
typedef struct { uint64_t length; uint32_t n_unclamped, kind; } pm_resample_info;                          /* 16 bytes */

int pm_resample_items(pm_ctx *c, const pm_resample_query *q, size_t n, uint32_t flags, pm_length_point *out, size_t out_cap, pm_resample_info *info);
/* Same on device memory (every pointer 8-byte aligned), asynchronous on hip_stream (NULL: the context's stream), ordered as
 * pm_hit_rects_device is.  `first` is the caller's: requests may be laid out freely, in any order, with gaps.  No record with
 * first + j >= out_cap is ever written, so a bad `first` cannot reach outside the buffer; ranges that overlap are the caller's
 * business.  The device cannot refuse a request: an invalid one answers as said above. */
int pm_resample_items_device(pm_ctx *c, const void *dev_q, size_t n, uint32_t flags, void *dev_out, size_t out_cap, void *dev_info, void *hip_stream);

/* ==== trimming: the piece of an item between two lengths (decision D27) ====
 * A request names a piece [lo, hi] of `item` in the unit of path measurement, 2^-16 px, and gets the geometry between the two
 * positions: the vertices of the walk's segments that overlap the piece, in the order of the walk, as poly-line runs.  Lengths,
 * segments k, their ends a and b, q_k, Q_k, T and the kind are path measurement's (D25) as they are.
 *
 *   PM_TRIM_RANGE  lo = min(s0, T), hi = min(s1, T); s0 > s1 is invalid.  {0, 2^64 - 1} is the whole item.
 *   PM_TRIM_PART   s0 = j, s1 = m, 1 <= m <= PM_TRIM_MAX_PARTS, j < m: piece j of m even ones, [b_j, b_j+1] with
 *                  b_i = i * (T div m) + min(i, T mod m) -- pm_resample_items' even positions.  The m pieces tile [0, T] exactly.
 *
 * Segment k is covered iff Q_k < hi and Q_k + q_k > lo: an overlap of positive length, or, for q_k == 0, lo < Q_k < hi.  lo >= hi
 * covers nothing (the empty piece).  A covered k has A_k -- a's stored pair if lo <= Q_k, else pm_points_at_length's point at lo --
 * and B_k -- b's stored pair if hi >= Q_k + q_k, else the point at hi.  For every covered k in increasing order A_k is emitted, with
 * PM_TRIM_MOVE, iff k is the first covered segment or A_k differs from the B of the covered segment before (compared as f32 values:
 * -0 equals 0, a NaN nothing); then B_k is emitted.  So a piece is a list of runs without doubled joints, and a run breaks where the
 * walk jumps: between the sub-paths of a compound Fill.  Wrap-around on a closed item is two requests.
 *
 * A vertex is a pm_trim_vertex {x, y, index = k, flags}: PM_TRIM_MOVE starts a run, PM_TRIM_CUT says the vertex is interpolated
 * (on a segment with a non-finite end its x, y are not promised).  Vertex number p of a piece goes to out[first + p] iff p < cap and
 * first + p < out_cap; nothing else of the buffer is touched.  Every request gets a pm_trim_info {length = T, n_vertices, n_runs,
 * kind, flags}: the counts are of the whole piece, whatever was written (cap = 0 is the count pass); flags PM_TRIM_TRUNCATED (some
 * vertex was not written) and PM_TRIM_END_CLAMPED (range mode with s1 > T).  A request the device cannot answer writes no vertex and
 * has an info of zeros with kind PM_TRIM_INVALID.  The length of a piece re-measured from its vertices is not promised to be hi - lo:
 * cut ends are rounded to f32.
 *
 * pm_trim_items: the vertices are packed: q[k].first must be the sum of the caps before it, the total at most out_cap.  flags:
 * PM_HIT_SKIP_TRANSPARENT or 0.  PM_ERR_INVALID, before anything is enqueued: any other flag bit, no resident scene, a NULL q or info
 * with n != 0, a NULL out with a non-zero total, a request the device would call invalid, a wrong `first`.  PM_ERR_CAPACITY, with
 * nothing written: the total exceeds out_cap or 2^20 records.  n == 0 is PM_OK and writes nothing.  Independent of the viewport;
 * frames in flight are not disturbed.  Synchronises. */
#define PM_TRIM_RANGE 0u               /* pm_trim_query.mode */
#define PM_TRIM_PART 1u
#define PM_TRIM_MAX_PARTS 1048576u     /* 2^20 */
#define PM_TRIM_MOVE 1u                /* pm_trim_vertex.flags */
#define PM_TRIM_CUT 2u
#define PM_TRIM_TRUNCATED 1u           /* pm_trim_info.flags */
#define PM_TRIM_END_CLAMPED 2u
#define PM_TRIM_INVALID 0xffffffffu    /* pm_trim_info.kind of a request that cannot be answered */
typedef struct { uint32_t item, mode, first, cap; uint64_t s0, s1; } pm_trim_query;                         /* 32 bytes */
typedef struct { float x, y; uint32_t index, flags; } pm_trim_vertex;                                      /* 16 bytes */
typedef struct { uint64_t length; uint32_t n_vertices, n_runs, kind, flags; } pm_trim_info;                /* 24 bytes */

int pm_trim_items(pm_ctx *c, const pm_trim_query *q, size_t n, uint32_t flags, pm_trim_vertex *out, size_t out_cap, pm_trim_info *info);
/* Same on device memory (every pointer 8-byte aligned), asynchronous on hip_stream (NULL: the context's stream), ordered as
 * pm_hit_rects_device is.  `first` and `cap` are the caller's: pieces may be laid out freely, in any order, with gaps.  No record at
 * or beyond out_cap is ever written; ranges that overlap are the caller's business.  The device cannot refuse a request: an invalid
 * one answers as said above. */
int pm_trim_items_device(pm_ctx *c, const void *dev_q, size_t n, uint32_t flags, void *dev_out, size_t out_cap, void *dev_info, void *hip_stream);

/* ==== item crossings: every point where two items' edges cross (decision D29) ====
 * A request names two items and gets every crossing of an edge of A with an edge of B; item_a == item_b asks for the item's
 * self-crossings, each pair of edges i < j once.  The edges of an item are the segments of path measurement's walk (D25) under D21's
 * names (item, k) with both ends finite; K(item), the size of the range k runs over, is 1 for a Line, the number of points less one
 * for a Polyline, the number of entries (separators included) for a Fill, and 0 for everything without a walk: a Circle or ellipse, a
 * one-point Polyline, an item the flags skip, an index >= the number of items.  No request is invalid.
 *
 * A pair e = (A, i): a -> b, f = (B, j): c -> d is a crossing iff (1) the edges' boxes meet, max(a.x, b.x) >= min(c.x, d.x),
 * max(c.x, d.x) >= min(a.x, b.x) and the same in y, on the stored f32 values; (2) the edges share no end (an end of e equal to an end
 * of f in both f32 coordinates); (3) pm_snap_intersections' arithmetic in binary64, one rounding per operation: r = b - a, s = d - c,
 * den = rx sy - ry sx != 0, w = c - a, t = (wx sy - wy sx) / den, u = (wx ry - wy rx) / den, 0 <= t <= 1 and 0 <= u <= 1.
 * T-junctions count; parallel, collinear and degenerate edges give none.  The point is X = a + r t.
 *
 * The record is a pm_crossing: its first and its second 16 bytes are each a pm_edge_query {item, index, t, 0} that
 * pm_positions_on_edges takes as it is; then x, y (X rounded to f32), side (PM_CROSSING_SIDE_POS if den > 0, PM_CROSSING_SIDE_NEG if
 * den < 0: which way B crosses A) and a zero word.  The crossings of a request are numbered p = 0, 1, ... by (i, j) ascending, and
 * record p goes to out[first + p] iff p < cap and first + p < out_cap; nothing else of the buffer is touched.  Every request gets a
 * pm_crossings_info {n_crossings, flags, n_a = K(A), n_b = K(B)}: n_crossings counts the whole answer, whatever was written (cap = 0
 * is the count pass); flags PM_CROSSINGS_TRUNCATED (some record was not written) and PM_CROSSINGS_TOO_MANY: K(A) * K(B) exceeds
 * PM_CROSSINGS_MAX_PAIRS, no pair was looked at, n_crossings is 0 and nothing is written -- split the item with pm_trim_items.
 * {B, A} answers what {A, B} does with the roles exchanged: the same pairs, t and u exchanged bit for bit, side 1 <-> 2; x and y are
 * computed from the other edge and may differ in the last bit.
 *
 * pm_item_crossings: the records are packed: q[k].first must be the sum of the caps before it, the total at most out_cap.  flags:
 * PM_HIT_SKIP_TRANSPARENT or 0.  PM_ERR_INVALID, before anything is enqueued: any other flag bit, no resident scene, a NULL q or info
 * with n != 0, a NULL out with a non-zero total, a wrong `first`.  PM_ERR_CAPACITY, with nothing written: the total exceeds out_cap or
 * 2^20 records.  n == 0 is PM_OK and writes nothing.  Independent of the viewport; frames in flight are not disturbed.  Synchronises. */
#define PM_CROSSINGS_TRUNCATED 1u          /* pm_crossings_info.flags */
#define PM_CROSSINGS_TOO_MANY 2u
#define PM_CROSSINGS_MAX_PAIRS 268435456u  /* 2^28 */
#define PM_CROSSING_SIDE_POS 1u            /* pm_crossing.side */
#define PM_CROSSING_SIDE_NEG 2u
typedef struct { uint32_t item_a, item_b, first, cap; } pm_crossings_query;                                  /* 16 bytes */
typedef struct { uint32_t item_a, index_a; float t; uint32_t reserved_a;
                 uint32_t item_b, index_b; float u; uint32_t reserved_b;
                 float x, y; uint32_t side, reserved; } pm_crossing;                                         /* 48 bytes */
typedef struct { uint32_t n_crossings, flags, n_a, n_b; } pm_crossings_info;                                 /* 16 bytes */

int pm_item_crossings(pm_ctx *c, const pm_crossings_query *q, size_t n, uint32_t flags, pm_crossing *out, size_t out_cap, pm_crossings_info *info);
/* Same on device memory (every pointer 8-byte aligned), asynchronous on hip_stream (NULL: the context's stream), ordered as
 * pm_hit_rects_device is.  `first` and `cap` are the caller's: answers may be laid out freely, in any order, with gaps.  No record at
 * or beyond out_cap is ever written; ranges that overlap are the caller's business.  A request is one wave's work. */
int pm_item_crossings_device(pm_ctx *c, const void *dev_q, size_t n, uint32_t flags, void *dev_out, size_t out_cap, void *dev_info, void *hip_stream);

/* For a scene made by pm_flatten_and_encode / pm_reflatten: path_of_item[i] = index into the `paths` array that
 * produced item i.  *n_items is always set; PM_ERR_CAPACITY if cap < n_items; PM_ERR_INVALID for a scene that came
 * from pm_upload_scene (or no scene at all). */
int pm_item_paths(pm_ctx *c, uint32_t *path_of_item, size_t cap, uint32_t *n_items);

/* Developer / test hook for the generated layout code (piet_metal_amd/csrc/pm_layout_gen.h, printed by
 * pm_layoutgen from piet_metal_amd/layout/piet_layout.pgpu -- the HIP / C++ target of the reference's
 * piet-gpu-derive generator, piet-gpu-derive/src/lib.rs): every item of `scene`'s root group and
 * every command of `cmds` goes through the generated readers, loaders and writers and must come
 * back byte for byte.  0 = agreement. */
int pm_layout_selfcheck(const uint8_t *scene, size_t scene_len, const pm_cmd *cmds, size_t n_cmds);

/* Developer profiling hook: re-run the last frame's per-tile kernel recording, per queue
 * slot, {start clock, end clock (100 MHz wall clock), tile | quarter << 31,
 * wave << 32 | commands interpreted, ticks in phase A, ticks in phase B (tiles rendered by a
 * whole workgroup), clock when the tile's list was complete (fused kernel; else 0), ticks on
 * the wave's own items, then four words of list-building stages (fused kernel, packed pairs:
 * header | candidates, owners | scan, segments | emission, rounds | records)}.
 * out receives 12 u64 per slot. */
int pm_debug_time_tiles(pm_ctx *c, uint64_t *out, size_t max_slots, size_t *n_slots); /* pm_fine_kernel */
/* Same for pm_bin_kernel: renders one frame recording 12 u64 per strip row {start, item scan done,
 * headers done, segment stream done, record finalised, queues done, chunks streamed, end}. */
int pm_debug_time_bins(pm_ctx *c, uint64_t *out, size_t max_rows, size_t *n_rows);

#ifdef __cplusplus
}
#endif
#endif /* PIET_METAL_AMD_H */
