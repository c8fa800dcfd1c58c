/* libymk_hip.so - C ABI of the MI355X (gfx950) DocumentAnalyzer hot path.
 *
 * The reference (kotaro-kinoshita/yomitoku) is pure Python and has no FFI.  The seam this
 * ABI plugs into is the one its optional ONNX backend already uses: one call per network
 * forward with C-contiguous buffers in and out
 *   sess.run(["output"], {"input": ndarray})   text_detector.py:122-125,
 *                                              text_recognizer.py:248-251,
 *                                              layout_parser.py:252-258,
 *                                              table_structure_recognizer.py:262-268
 * and the `self.model(tensor)` call it stands in for (text_detector.py:127-129 etc.).
 * INTEGRATION.md shows the ctypes stub a yomitoku maintainer would add.
 *
 * Rules
 *   - plain pointers and sizes only; `stream` is a hipStream_t passed as void* (NULL = default);
 *   - pointers named *_dev are device (HBM) addresses owned by the caller; the library owns
 *     weights and workspace, and allocates nothing on the per-call path once a shape was seen;
 *   - every function returns 0 on success, non-zero on failure; ymk_last_error() returns the
 *     message of the calling thread's last failure;
 *   - a model handle may be used from one thread at a time; different handles are independent.
 */
#ifndef YMK_H
#define YMK_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ymk_model ymk_model;

int ymk_version(void);
const char* ymk_last_error(void);
/* number of visible HIP devices, or -1 */
int ymk_device_count(void);

/* ---- model lifecycle (replaces BaseModule.load_model, base.py:80-86) -------------------
 * kind: "dbnet" | "parseq" | "rtdetr".  Weights are handed over tensor by tensor under the
 * reference's state-dict names (host fp32, C-contiguous), scalar hyper-parameters by name,
 * then ymk_model_finalize() folds BatchNorm, repacks panels and uploads to `device`. */
ymk_model* ymk_model_create(const char* kind, int device);
void ymk_model_destroy(ymk_model* m);
/* One parameter may also be set on a finalized model: "conv_split" - how this model's convolutions / linear layers that fill
 * the chip multiply (ymk_conv_split.hip; grid-starved launches, attention and the fused greedy step are exact fp32 always):
 *   16  the default: fp32 operands scaled by powers of two and cut into two fp16 planes (11 + 11 significand bits), three
 *       v_mfma_f32_32x32x16_f16 per product tile, fp32 accumulation - products good to 2^-21, below the fp32 accumulation's
 *       own rounding for K >= 64 (measured: as far from the exact kernel as the exact kernel in another summation order)
 *   0   exact fp32 MFMA (v_mfma_f32_32x32x2_f32, an fmaf chain in k order)
 *   2 / 3   two / three bf16 planes, 3 / 6 MFMAs (2: products to 2^-15 only - evaluation)
 *   -1  follow the process-wide ymk_debug_option("conv_split") if set, else the default.
 * parseq only: "conv_split_encoder" - the same choice for the ViT blocks' linear layers alone (the decoder and the
 * vocabulary head then follow "conv_split").
 *
 * "workspace_reuse" (0 | 1, default 0; any time outside a forward) - how the model lays its activations out in its workspace:
 *   0   the bump arena: every buffer of a forward gets bytes of its own, the workspace is the SUM of a forward's buffers;
 *   1   planned: buffers that are never alive at the same time share bytes.  The dry run that sizes the workspace (at
 *       ymk_model_reserve, or on the host at the head of the first forward of a new shape) records every allocation and the
 *       point where its last user has been enqueued, a deterministic greedy planner (ymk_op_plan_workspace below) turns the
 *       record into one offset per allocation, and forwards replay the table: nothing is searched or allocated inside a
 *       forward, and the four "in_forward" counters of ymk_stat stay where they are.  Outputs are bit-identical to mode 0.
 *   A change drops the cached plans; the next ymk_model_reserve sizes the workspace anew (it may shrink).  An unset parameter
 *   follows ymk_debug_option("workspace_reuse") / the environment variable YMK_WORKSPACE_REUSE (yomitoku_amd/_lib.py).
 *   The stream rule: reuse is sound because all launches of a forward are ordered on ONE stream, the one the call was given.
 *   Buffers touched by anything that stream does not order - the caller after the forward returns, a later ABI call, a host
 *   flag - are never released ("Planned workspaces", has the audit per net).  As in mode 0, consecutive forwards
 *   of one handle must be issued on one stream or be ordered by the caller.
 *   ymk_stat: "workspace_planned_forwards"; "ws_plan_bytes_last" / "ws_bump_bytes_last" / "ws_live_bound_last" = bytes the
 *   last plan (made or replayed) needs / the bump arena needs for the same trace / the largest sum of live bytes at one point
 *   of the trace, which no plan can beat.  ymk_model_workspace_bytes keeps reporting the slab actually held. */
int ymk_model_set_param(ymk_model* m, const char* key, double value);
int ymk_model_set_tensor(ymk_model* m, const char* name, const float* host_data, int ndim, const int64_t* dims);
int ymk_model_finalize(ymk_model* m);
/* Size the model's workspace once for the largest forward the caller will issue, so that forwards within the bound
 * never allocate or free device memory whatever their shape ("allocates nothing on the per-call path" also for calls
 * whose shape changes every time: the pages of a wave differ in size, the mini-batches of text_recognizer.py:158-203
 * differ in rows and width).  dbnet: n images of h x w (either orientation); rtdetr: n images of h x w; parseq: n
 * text lines over all groups of a call, each at most w pixels wide (h ignored). */
int ymk_model_reserve(ymk_model* m, int n, int h, int w, void* stream);
/* The planner of "workspace_reuse" = 1 on a caller-supplied trace; host only, no device.  Allocation k (call order) has
 * sizes[k] bytes, rounded up to 256 here, and is alive from position k until release_pos[k] = the number of allocations
 * made when it was released (> k); negative or >= n = never released.  offsets_out[k]: multiples of 256 such that two
 * allocations alive at the same position never overlap; *peak_out = the slab the plan needs, *live_bound_out = the largest
 * sum of (rounded) sizes alive at one position: live_bound <= peak <= sum of sizes.  Deterministic. */
int ymk_op_plan_workspace(int64_t n, const int64_t* sizes, const int64_t* release_pos, int64_t* offsets_out, int64_t* peak_out,
                          int64_t* live_bound_out);
/* bytes of HBM held by the model's weights / workspace */
int64_t ymk_model_weight_bytes(const ymk_model* m);
int64_t ymk_model_workspace_bytes(const ymk_model* m);

/* ---- DBNet text detector (replaces DBNet.forward, models/dbnet_plus.py:243-246) --------
 * x_dev: fp32 [n][3][h][w] (h, w multiples of 32, as TextDetector.preprocess produces);
 * prob_dev: fp32 [n][1][h][w] = preds["binary"]. */
int ymk_dbnet_forward(ymk_model* m, const float* x_dev, int n, int h, int w, float* prob_dev, void* stream);

/* ---- PARSeq text recogniser (replaces PARSeq.forward, models/parseq.py:159-311) ----------
 * x_dev: fp32 [b][3][32][w] in [-1,1] (w a multiple of the patch width, <= 800: the dynamic-width
 * batches of TextRecognizer._collate, text_recognizer.py:146-156); logits_dev: fp32
 * [b][max_label_length+1][num_tokens-2] (always allocate the full 101 rows); *out_len receives the
 * number of valid rows per sample (101 when refine_iters >= 1, else the AR steps executed),
 * *ar_steps the greedy steps executed before every row held an <eos>.  The call blocks until the AR loop
 * has stopped (the host polls a mapped flag two steps behind the device - the reference's early-stop test,
 * models/parseq.py:245-250) and returns with the refinement pass still queued on the stream.
 *
 * Non-autoregressive mode - the model parameter "decode_ar" = 0 (the reference's `decode_ar: 0`, models/parseq.py:253-262; 1, the
 * default, is the greedy loop above; any other value is refused by ymk_model_finalize): the context is <bos> alone and all
 * max_label_length+1 positions are asked in ONE decoder pass, followed by the refine_iters cloze passes (the first takes the
 * arg-max of that pass over all rows).  The part of the query stream that depends on weights only - up to the cross
 * attention's query projection - is built once by ymk_model_finalize; per call the work starts at the cross attention
 * over each sample's own encoder memory (ymk_op_nar_cross_attention below).  The repetition stop never applies (the
 * reference arms it inside the AR loop only).  *out_len = max_label_length+1 and *ar_steps = 0, for every group.  There is no
 * step loop, no mapped flag, no copy back: in this mode ymk_parseq_forward[_groups] only queues work on the stream and
 * returns without having waited on anything.  (The grouped call hands its row tables to the device through one of 64 slots
 * of pinned memory; it waits - counted in "syncs_in_forward" - only if the copy out of the slot it is about to reuse, issued
 * 64 grouped calls earlier, has still not run.)
 *
 * Retired rows - the model parameter "retire_rows" = 1 (default 0; any other value is refused by ymk_model_finalize): a row
 * leaves the greedy loop after the step whose raw arg-max is ITS <eos>, instead of running until the slowest row of its
 * mini-batch stops: it is no longer embedded, attended, fed forward or multiplied by the vocabulary head.  The refinement
 * masks every context token from a row's first <eos> on, so with the switch on these are what they are with it off: the token
 * ids up to and including each row's first <eos>, the score over them, *out_len and *ar_steps.  What changes: the repetition
 * detector no longer runs on a row behind its <eos>, so logits behind a row's first <eos> carry no repetition cut (the +-30
 * row); and the tokens behind an <eos> enter the max|x| record of the refinement's K|V projection, so refined logits may
 * differ in their last bits (the 2^-21 of the fp16-plane products).  A row the repetition detector stopped is not retired:
 * its arg-maxes stay context of the refinement, as before.  The switch acts where the loop's only products are its tokens:
 * the fused decoder step (decoder width <= 256) with refine_iters >= 1 and the row-max head.  It is accepted and ignored with
 * refine_iters = 0, under ymk_debug_option("parseq_no_rowmax", 1), on the per-operator decoder path of the wider models and
 * with "decode_ar" = 0. */
int ymk_parseq_dims(ymk_model* m, int* num_steps, int* num_classes);
int ymk_parseq_forward(ymk_model* m, const float* x_dev, int b, int w, float* logits_dev, int* out_len, int* ar_steps,
                       void* stream);
/* The same forward over n_groups mini-batches in ONE call (TextRecognizer's per-page mini-batches, of one page or of
 * several: text_recognizer.py:158-203 runs them one after the other).  Group g is its own tensor x_dev[g]
 * ([b[g]][3][32][w[g]], padded to ITS widest crop exactly as _collate does - padding columns are ordinary ViT tokens, so
 * the groups are never re-padded to a common width); x_dev, b, w, out_len, ar_steps are HOST arrays of n_groups
 * entries.  Every layer runs once over the token rows of all groups laid end to end, attention reads per-sample
 * (row offset, length) tables, and one greedy loop serves all rows; logits_dev: [sum b][max_label_length+1][C] in
 * group order.  out_len[g] / ar_steps[g] are what group g's own ymk_parseq_forward call would have returned. */
int ymk_parseq_forward_groups(ymk_model* m, const float* const* x_dev, const int* b, const int* w, int n_groups,
                              float* logits_dev, int* out_len, int* ar_steps, void* stream);
/* what ParseqTokenizer.decode needs from softmax(logits) (parseq_tokenizer.py:79-87) without
 * materialising it: per row the arg-max class id and max probability. rows = b * out_len. */
int ymk_parseq_token_stats(const float* logits_dev, int rows, int num_classes, int* ids_dev, float* probs_dev,
                           void* stream);

/* ---- RT-DETRv2 layout parser / table-structure recogniser (replaces RTDETRv2.forward,
 * models/rtdetr.py:16-21).  x_dev: fp32 [b][3][640][640] in [0,1] (LayoutParser.preprocess,
 * layout_parser.py:195-199); logits_dev: fp32 [b][num_queries][num_classes] = pred_logits;
 * boxes_dev: fp32 [b][num_queries][4] = pred_boxes (cxcywh in [0,1]). */
int ymk_rtdetr_forward(ymk_model* m, const float* x_dev, int b, int h, int w, float* logits_dev, float* boxes_dev,
                       void* stream);

/* ---- fused pre-processing kernels (uint8 BGR page resident in HBM -> network input tensors) ----
 * ymk_det_preprocess: TextDetector.preprocess (text_detector.py:99-107; resize_shortest_edge's
 *   cv2.resize(INTER_AREA) + standardization_image, data/functions.py:196-247).  bgr_dev: uint8
 *   [h][w][3]; x_dev: fp32 [3][oh][ow] (oh, ow from resize_shortest_edge, computed by the caller).
 * ymk_pil_resize_to_chw: LayoutParser / TableStructureRecognizer.preprocess (layout_parser.py:195-199,
 *   table_structure_recognizer.py:169-186): BGR->RGB, PIL bilinear antialiased resize of the crop at
 *   (x0, y0) to oh x ow, ToTensor.  Coefficient tables follow Pillow's precompute_coeffs /
 *   normalize_coeffs_8bpc (bounds: [o][2] = first tap, count; coefs: [o][ksize] 22-bit ints).
 * ymk_crop_batch: ParseqDataset crops (data/dataset.py:105-124): perspective warp, optional 90 deg
 *   rotation, down-scale-only INTER_AREA to the 32 px canvas, ToTensor + Normalize(0.5, 0.5), -1
 *   padding to batch_w.  descs_dev: array of n records of ymk_crop_desc_size() bytes (layout in
 *   yomitoku_amd/csrc/ymk_image.hip: CropDesc); out_dev: fp32 [slots][3][out_h][batch_w]. */
int ymk_det_preprocess(const unsigned char* bgr_dev, int h, int w, int oh, int ow, float* x_dev, void* stream);
int ymk_pil_resize_to_chw(const unsigned char* page_dev, int page_w, int x0, int y0, const int* xbounds_dev,
                          const int* xcoef_dev, int ksize_x, const int* ybounds_dev, const int* ycoef_dev, int ksize_y,
                          int oh, int ow, float* x_dev, void* stream);
/* ymk_pil_resize_batch_to_chw: ymk_pil_resize_to_chw for n crops in one launch (TableStructureRecognizer.preprocess loops over
 *   the table boxes, table_structure_recognizer.py:169-186; here all crops of a forward share a launch).  blob_dev: int32
 *   words - n records of ymk_pil_batch_record_words() words {page address low, high; page width; x0; y0; ksize_x; ksize_y;
 *   word offsets into the blob of xbounds, xcoefs, ybounds, ycoefs; 0}, followed by the tables; x_dev: fp32 [n][3][oh][ow]. */
int ymk_pil_resize_batch_to_chw(const int* blob_dev, int n, int oh, int ow, float* x_dev, void* stream);
int ymk_pil_batch_record_words(void);
int ymk_crop_batch(const unsigned char* page_dev, int page_h, int page_w, const void* descs_dev, int n, int max_warp_w,
                   int max_warp_h, unsigned char* scratch_dev, float* out_dev, int batch_w, int out_h, void* stream);
/* ymk_crop_batch_levels: the same with `source_downscale` (data/dataset.py:26-41,64-79): descriptor.level picks the
 *   pyramid level a crop is cut from.  level_pages: HOST array of n_levels (<= 4) device pointers, level 0 = the page;
 *   a NULL entry (level not built because no quad uses it) aliases the page.
 * ymk_halve_u8c3: one pyramid step, cv2.resize(img, None, fx=0.5, fy=0.5, INTER_AREA) on uint8 [h][w][3];
 *   dst_h / dst_w = round-half-even(h / 2), (w / 2) as cv2 computes them. */
int ymk_crop_batch_levels(const unsigned char* const* level_pages, const int* level_h, const int* level_w, int n_levels,
                          const void* descs_dev, int n, int max_warp_w, int max_warp_h, unsigned char* scratch_dev,
                          float* out_dev, int batch_w, int out_h, void* stream);
int ymk_halve_u8c3(const unsigned char* src_dev, int h, int w, unsigned char* dst_dev, int dst_h, int dst_w, void* stream);
int ymk_crop_desc_size(void);

/* ---- overlay rasteriser for visualize=True (yomitoku_amd/csrc/ymk_overlay.hip; replaces the cv2 / Pillow drawing of
 * utils/visualizer.py on host copies of the page).  DESIGN.md, "Overlay rasteriser", has the drawing rules in full.
 * ymk_draw_overlay: applies n commands IN COMMAND ORDER, in place, to canvas_dev: uint8 [h][w][3], 1 <= h, w <= 16383.  One block
 *   per tile of ymk_overlay_tile() x ymk_overlay_tile() pixels, tiles row-major ((w + tile - 1) / tile per row).  The caller bins
 *   the commands by bounding box: tile_offsets_dev int32 [tiles + 1] (ascending, [0] = 0, [tiles] = n_list), tile_cmds_dev int32
 *   [n_list] = for each tile the indices of the commands that may cover one of its pixels, ascending.  A block stages its list in
 *   LDS ymk_overlay_chunk() records at a time; a tile with an empty list is neither read nor written.  A list entry outside
 *   [0, n), an unknown kind and a glyph byte outside [0, atlas_bytes) draw nothing.  Nothing is allocated and nothing waited for.
 *   cmds_dev: n records of YMK_OVERLAY_CMD_WORDS int32 words (16-byte aligned), all coordinates in [-16383, 16383]:
 *     word 0     kind: YMK_OVERLAY_SEG | _BOX | _GLYPH | _RBOX | _FLUSH, or-ed with YMK_OVERLAY_TO_LAYER or not; a word with any
 *                bit outside 0x1ff set (-1 among them) draws nothing
 *     words 1-3  colour in the canvas's channel order (B, G, R), 0..255
 *     word 4     alpha 0..255 of SEG and BOX (GLYPH takes its alpha from the atlas)
 *     SEG    words 5-9   x0, y0, x1, y1, t     a segment of thickness t with round caps: with d = P1 - P0, L2 = d.d, q = p - P0,
 *                        u = q.d the pixel p is covered iff   L2 == 0 or u <= 0: 4 |q|^2 <= t^2;   u >= L2: 4 |p - P1|^2 <= t^2;
 *                        otherwise 4 (q x d)^2 <= t^2 L2
 *     BOX    words 5-12  ox1, oy1, ox2, oy2, ix1, iy1, ix2, iy2   covered iff inside the outer box and not inside the inner box
 *                        (both inclusive; the inner box is empty when ix1 > ix2 or iy1 > iy2)
 *     GLYPH  words 5-10  x, y, w, h, atlas_offset, pitch   alpha = atlas_dev[atlas_offset + (py - y) * pitch + (px - x)] for
 *                        pixels in [x, x + w) x [y, y + h); atlas_dev: uint8 [atlas_bytes]
 *     RBOX   words 5-9   x1, y1, x2, y2, r     a filled box with round corners: r' = min(r, (x2 - x1) / 2, (y2 - y1) / 2), cx =
 *                        clamp(px, x1 + r', x2 - r'), cy likewise; covered iff inside the box and (px - cx)^2 + (py - cy)^2 <= r'^2
 *     FLUSH  words 5-9   x1, y1, x2, y2, keep255   see "layer"; word 4 is its alpha, the colour words are unused
 *   Blend of a covered pixel, per channel: dst = blend(dst, colour, a) = (colour * a + dst * (255 - a) + 127) / 255 (a = 255
 *   overwrites, 0 leaves).
 *   Layer: every pixel has, for the length of one call, a LAYER next to it: a colour and a coverage cov, both 0 at the start.  A
 *   SEG, BOX, GLYPH or RBOX record with YMK_OVERLAY_TO_LAYER set leaves the canvas alone; where its coverage is a > 0 it paints the
 *   layer: cov == 0: colour = the record's, cov = a; else colour = blend(colour, the record's, a) per channel and cov = blend(cov,
 *   255, a).  FLUSH composites the layer over the canvas, once per pixel however many records painted it: for a pixel inside its
 *   box with cov > 0, e = (cov * alpha + 127) / 255 and dst = blend(dst, layer colour, e) per channel - except, with keep255 != 0,
 *   a channel whose layer colour is exactly 255, which is left alone - and every pixel inside the box gets cov = 0.  Pixels
 *   outside the box keep their layer; a layer never flushed is dropped; a FLUSH with YMK_OVERLAY_TO_LAYER set draws nothing.  The
 *   bounding box of an RBOX and of a FLUSH is its box, and a record directed into the layer has the bounds of its kind.
 * ymk_heatmap_blend: prob_dev fp32 [mh][mw] blended over canvas_dev uint8 [h][w][3] in place, det_visualizer(vis_heatmap=True)
 *   in integers: m = (uint8) trunc(clamp(p, 0, 1) * 255); per axis X = ((2 x + 1) * mw * 1024) / (2 w) - 512 clamped to
 *   [0, (mw - 1) * 1024], taps X >> 10 and min(that + 1, mw - 1), weight X & 1023; v = (sum of the four weighted taps + 2^19)
 *   >> 20; dst = (dst + jet_dev[v][channel] + 1) >> 1 with jet_dev: uint8 [256][3] (B, G, R). */
#define YMK_OVERLAY_CMD_WORDS 16
#define YMK_OVERLAY_SEG 0
#define YMK_OVERLAY_BOX 1
#define YMK_OVERLAY_GLYPH 2
#define YMK_OVERLAY_RBOX 3
#define YMK_OVERLAY_FLUSH 4
#define YMK_OVERLAY_KIND_MASK 0xff
#define YMK_OVERLAY_TO_LAYER 0x100
int ymk_draw_overlay(unsigned char* canvas_dev, int h, int w, const int* cmds_dev, int n, const int* tile_offsets_dev,
                     const int* tile_cmds_dev, int n_list, const unsigned char* atlas_dev, int64_t atlas_bytes, void* stream);
int ymk_heatmap_blend(unsigned char* canvas_dev, int h, int w, const float* prob_dev, int mh, int mw, const unsigned char* jet_dev,
                      void* stream);
int ymk_overlay_tile(void);
int ymk_overlay_chunk(void);

/* ---- a wave of canvases in two calls (DocumentAnalyzer.serve(overlays=True)): text laid out and commands culled on the device.
 * The canvases of a wave - uint8 [h][w][3] each, of differing sizes - lie in ONE device buffer; cmds_dev holds the records of all
 * of them (layout and rules as above), each canvas's commands contiguous and in drawing order.  canvases_dev / table_dev: int64
 * [n_canvases][YMK_OVERLAY_CANVAS_WORDS] = byte offset of the canvas in the buffer, h, w, first command, command count, first
 * tile (the canvases' tiles are numbered one canvas after the other, row-major inside a canvas).  An entry that does not fit
 * (1 <= h, w <= 16383, the bytes inside the buffer, the commands inside [0, n_cmds)) is ignored, never trusted.
 * ymk_overlay_layout: (1) text runs -> GLYPH records.  The host reserves one record per character (kind, colour filled in) and
 *   gives runs_dev: int32 [n_runs][YMK_OVERLAY_RUN_WORDS] = first slot, first code index, count, pen x, pen y, direction (0
 *   horizontal, 1 vertical), vertical step, 0; codes_dev: int32 [n_codes] glyph ids; glyphs_dev: int32 [n_glyphs]
 *   [YMK_OVERLAY_GLYPH_WORDS] = atlas offset, w, h, x offset, y offset, advance.  Character i of a run gets words 5..10 = clamp(pen
 *   + offsets) to [-16383, 16383], w, h, atlas offset, pitch w, with the pen at (pen x + the advances of characters 0..i-1, pen y),
 *   vertical: (pen x, pen y + i * step).  A character whose glyph is empty (w or h 0) or whose id lies outside [0, n_glyphs) gets
 *   kind -1 (draws nothing; it still advances the pen by its advance, 0 for an unknown id).  A run whose slots or codes fall
 *   outside the arrays is skipped.  (2) bounds_dev: int16 [n_cmds][4] = every command's inclusive bounding box x0, y0, x1, y1 (SEG:
 *   the end points' box grown by (t + 1) / 2; BOX: the outer box; RBOX, FLUSH: the box; GLYPH: x .. x + w - 1, y .. y + h - 1;
 *   with or without the layer flag) clipped to its canvas;
 *   (1, 1, 0, 0) - x1 < x0 - for a command that covers none of its canvas.  Commands no canvas entry names are not written.
 * ymk_draw_overlay_pages: ONE launch, a block per tile (total_tiles = the sum over the canvases).  A block finds its canvas in
 *   the table, tests ymk_overlay_cull_pass() bounding boxes of that canvas at a time against its tile, keeps the hits in command
 *   order and applies them as ymk_draw_overlay does; a tile without hits is neither read nor written.  The result equals
 *   ymk_draw_overlay per canvas with the caller's per-tile lists.  No atomics, nothing allocated, nothing waited for. */
#define YMK_OVERLAY_RUN_WORDS 8
#define YMK_OVERLAY_GLYPH_WORDS 6
#define YMK_OVERLAY_CANVAS_WORDS 6
int ymk_overlay_layout(int* cmds_dev, int n_cmds, int16_t* bounds_dev, const int* runs_dev, int n_runs, const int* codes_dev,
                       int n_codes, const int* glyphs_dev, int n_glyphs, const int64_t* canvases_dev, int n_canvases, void* stream);
int ymk_draw_overlay_pages(unsigned char* canvases_dev, int64_t canvas_bytes, const int64_t* table_dev, int n_canvases,
                           int64_t total_tiles, const int* cmds_dev, int n_cmds, const int16_t* bounds_dev,
                           const unsigned char* atlas_dev, int64_t atlas_bytes, void* stream);
int ymk_overlay_cull_pass(void);

/* ---- baseline JPEG encoder for a wave of pages (yomitoku_amd/csrc/ymk_jpeg.hip; DocumentAnalyzer.serve(jpeg=...) and
 * yomitoku_amd/jpeg.py).  DESIGN.md, "JPEG encoder", has the file format and the pixel rules; every stage is integer arithmetic
 * and equals tests/jpeg_ref.py byte for byte.  Pages: uint8 [h][w][3] (B G R; 4:2:0, MCU 16 x 16, six blocks Y0 Y1 Y2 Y3 Cb Cr)
 * or uint8 [h][w] (one component, MCU 8 x 8), rows contiguous, 1 <= h, w <= 16383; a restart interval is one MCU row.
 * Page table: blob_dev, int32 words on the device (16-byte aligned), blob_words of them: n_pages records of
 *   YMK_JPEG_PAGE_WORDS words, then whatever the records point to.
 *     words 0-1   page address, low / high          words 2-4   h, w, channels (1 | 3)
 *     words 5-7   first MCU, first block, first restart interval of the page (the pages' are numbered one after the other)
 *     words 8-9   byte offset of the page's file in out_dev, low / high           word 10  capacity of that file in bytes
 *     word 11-12  BYTE offset in the blob and length of the file's header (ymk_jpeg_header)
 *     word 13     WORD offset in the blob of the page's 128 quantisation values (ymk_jpeg_quant_tables)      word 14  0 (see *_opt)
 *     word 15     the page's mode, 0 = what is said above (see YMK_JPEG_MODE_*)
 *   A record that does not fit (sizes, indices beyond the totals passed, offsets beyond the blob or out_bytes) is ignored, never
 *   trusted: its page gets length -1.
 * Scratch and output are the caller's; ymk_jpeg_scratch_bytes sizes them from HOST arrays h, w, channels: sizes6_out = total
 *   MCUs, blocks, intervals, then the bytes of coef_dev (int16 [blocks][64], 16-byte aligned), of stream_dev (the unstuffed scan:
 *   YMK_JPEG_BLOCK_STREAM_BYTES per block - a block's worst case - big-endian 32-bit words, an interval's words starting at
 *   its first block's) and of intervals_dev (int32 [intervals][2] = bytes, bytes after FF -> FF 00).
 * ymk_jpeg_quant_tables: the 64 luminance, then the 64 chrominance values for `quality` (1..100, IJG rule), zig-zag order; HOST.
 * ymk_jpeg_header: SOI, APP0, DQT, SOF0, DHT, DRI, SOS of such a file into the HOST buffer `out`; returns its length, -1 on error.
 * ymk_jpeg_coefficients: pages -> coef_dev, zig-zag, scan order; one wave per MCU.
 * ymk_jpeg_entropy: coef_dev -> stream_dev + intervals_dev; one wave per interval (bit lengths, wave prefix sum, Huffman bits, pad).
 * ymk_jpeg_compact: lengths_dev int32 [n_pages]: header + stuffed intervals + RSTm + EOI laid out at the page's offset and the
 *   file's length - or -1, and NOT ONE BYTE of the page's output written, when the file would exceed the page's capacity.
 * ymk_jpeg_encode_pages: the three stages in order on `stream`.  Nothing is allocated, nothing waited for. */
#define YMK_JPEG_PAGE_WORDS 16
#define YMK_JPEG_BLOCK_STREAM_BYTES 208
int ymk_jpeg_page_words(void);
int ymk_jpeg_quant_tables(int quality, int* zigzag128_out);
int ymk_jpeg_header(int h, int w, int channels, int quality, unsigned char* out, int capacity);
int ymk_jpeg_scratch_bytes(const int* h, const int* w, const int* channels, int n_pages, int64_t* sizes6_out);
int ymk_jpeg_coefficients(const int* blob_dev, int64_t blob_words, int n_pages, int64_t total_mcus, int16_t* coef_dev,
                          int64_t total_blocks, void* stream);
int ymk_jpeg_entropy(const int* blob_dev, int64_t blob_words, int n_pages, const int16_t* coef_dev, int64_t total_blocks,
                     uint32_t* stream_dev, int64_t stream_bytes, int* intervals_dev, int64_t total_intervals, void* stream);
int ymk_jpeg_compact(const int* blob_dev, int64_t blob_words, int n_pages, const uint32_t* stream_dev, int64_t stream_bytes,
                     int64_t total_blocks, const int* intervals_dev, int64_t total_intervals, unsigned char* out_dev, int64_t out_bytes,
                     int* lengths_dev, void* stream);
int ymk_jpeg_encode_pages(const int* blob_dev, int64_t blob_words, int n_pages, int64_t total_mcus, int64_t total_blocks,
                          int64_t total_intervals, int16_t* coef_dev, uint32_t* stream_dev, int64_t stream_bytes, int* intervals_dev,
                          unsigned char* out_dev, int64_t out_bytes, int* lengths_dev, void* stream);
/* Optimised Huffman tables, opt-in (encode_jpeg_pages(optimize=True), serve(jpeg_optimize=True); tests/jpeg_opt_ref.py is the
 * definition; DESIGN.md, "JPEG encoder", has the rule): the same coefficients coded with tables made for each page, libjpeg's
 * `optimize` rule, byte for byte.  The entries above do what they did; these stand next to them.
 * Page table: as above, except that the header of words 11-12 comes from ymk_jpeg_header_opt - it has no DHT segments - and
 *   word 14 holds the bytes of it that stand before their place (SOI .. SOF0; the rest is DRI, SOS).
 * ymk_jpeg_header_opt: that header into the HOST buffer `out`, *split_out = word 14; returns its length, -1 on error.
 * ymk_jpeg_scratch_bytes_opt: sizes9_out = the six of ymk_jpeg_scratch_bytes with stream_dev at
 *   YMK_JPEG_BLOCK_STREAM_BYTES_OPT per block (a page's own DC code may have 16 bits, Annex K's at most 11: a block's worst case
 *   is 16 + 11 + 63 * 26 = 1665 bits), then the bytes of hist_dev and of tables_dev (each int32 [n_pages][2][256 + 16] =
 *   YMK_JPEG_TABLE_WORDS per page: luminance, chrominance; 256 AC entries, then 16 DC entries) and of dht_dev
 *   (YMK_JPEG_DHT_BYTES per page: an int32 length, then the page's DHT segments, DC 0, AC 0, DC 1, AC 1).  All 4-byte aligned.
 * ymk_jpeg_histogram: hist_dev zeroed on `stream`, then the symbols ymk_jpeg_entropy would emit for coef_dev counted into it;
 *   one wave per interval, integer atomicAdd per page.
 * ymk_jpeg_optimal_tables: hist_dev -> tables_dev (symbol -> code | length << 16, 0: no code) and dht_dev; one workgroup per
 *   page, one wave per table.  Any counts are accepted; a table without a symbol has no code.
 * ymk_jpeg_entropy_opt / ymk_jpeg_compact_opt: the two stages with the pages' tables / DHT records.  An entry of tables_dev with a
 *   length above 16 is ignored, so that no block outgrows its reservation whatever tables_dev holds.
 * ymk_jpeg_encode_pages_opt: the five stages in order on `stream`.  Nothing is allocated, nothing waited for. */
#define YMK_JPEG_BLOCK_STREAM_BYTES_OPT 212
#define YMK_JPEG_TABLE_WORDS 544
#define YMK_JPEG_DHT_BYTES 656
int ymk_jpeg_header_opt(int h, int w, int channels, int quality, unsigned char* out, int capacity, int* split_out);
int ymk_jpeg_scratch_bytes_opt(const int* h, const int* w, const int* channels, int n_pages, int64_t* sizes9_out);
int ymk_jpeg_histogram(const int* blob_dev, int64_t blob_words, int n_pages, const int16_t* coef_dev, int64_t total_blocks,
                       int64_t total_intervals, int* hist_dev, void* stream);
int ymk_jpeg_optimal_tables(const int* blob_dev, int64_t blob_words, int n_pages, const int* hist_dev, uint32_t* tables_dev,
                            unsigned char* dht_dev, void* stream);
int ymk_jpeg_entropy_opt(const int* blob_dev, int64_t blob_words, int n_pages, const int16_t* coef_dev, int64_t total_blocks,
                         const uint32_t* tables_dev, uint32_t* stream_dev, int64_t stream_bytes, int* intervals_dev,
                         int64_t total_intervals, void* stream);
int ymk_jpeg_compact_opt(const int* blob_dev, int64_t blob_words, int n_pages, const uint32_t* stream_dev, int64_t stream_bytes,
                         int64_t total_blocks, const int* intervals_dev, int64_t total_intervals, const unsigned char* dht_dev,
                         unsigned char* out_dev, int64_t out_bytes, int* lengths_dev, void* stream);
int ymk_jpeg_encode_pages_opt(const int* blob_dev, int64_t blob_words, int n_pages, int64_t total_mcus, int64_t total_blocks,
                              int64_t total_intervals, int16_t* coef_dev, int* hist_dev, uint32_t* tables_dev, unsigned char* dht_dev,
                              uint32_t* stream_dev, int64_t stream_bytes, int* intervals_dev, unsigned char* out_dev, int64_t out_bytes,
                              int* lengths_dev, void* stream);
/* Per-page modes, opt-in (encode_jpeg_pages(subsampling=..., grey="auto"), serve(jpeg_subsampling=..., jpeg_grey=...);
 * tests/jpeg_modes_ref.py is the definition).  Word 15 of a page's record:
 *     YMK_JPEG_MODE_420 (0)  a [h][w][3] page as 4:2:0 - today's file - or a [h][w] page as one component; the only mode of a [h][w] page
 *     YMK_JPEG_MODE_422      [h][w][3]: luminance sampling 2 x 1, MCU 16 x 8 pixels, four blocks Y0 Y1 Cb Cr; chroma = the mean of each
 *                            horizontal pair, (a + b + bias) >> 1, bias 0 in even output columns and 1 in odd ones
 *     YMK_JPEG_MODE_444      [h][w][3]: luminance sampling 1 x 1, MCU 8 x 8 pixels, three blocks Y Cb Cr; chroma at full resolution
 *     YMK_JPEG_MODE_GREY     [h][w][3], three interleaved source channels: channel 0 is encoded as the one-component file of the
 *                            [h][w] page it is (MCU 8 x 8, one block), read in place with a pixel stride of 3
 *   Any other value makes the record one that does not fit.  With luminance sampling hs x vs an MCU is 8 hs x 8 vs pixels of
 *   hs vs + 2 blocks, a restart interval one MCU row (at most 2048 MCUs of 3 blocks, 1024 of 4 or of 6), the SOF0 luminance byte
 *   hs << 4 | vs and DRI ceil(w / (8 hs)).  Word 5 and total_mcus count what a wave of ymk_jpeg_coefficients takes: the 16 x 16 pixel
 *   tiles of a [h][w][3] page in every mode (one, two or four MCUs; at 4:2:0 the MCU itself), the 8 x 8 MCUs of a [h][w] page.
 * ymk_jpeg_header_mode / ymk_jpeg_header_opt_mode / ymk_jpeg_scratch_bytes_mode / ymk_jpeg_scratch_bytes_opt_mode: the entries
 *   without _mode for pages of these modes (modes: HOST int [n_pages], null = all 0; sizes[0] = the tiles); mode 0 gives what
 *   those give.
 * ymk_jpeg_pages_grey: diff_dev int32 [n_pages], zeroed on `stream`, then per page the OR over its pixels of (B ^ G) | (B ^ R)
 *   reduced to 0 / 1: 0 = every pixel of the page has B == G == R (the page may be written with YMK_JPEG_MODE_GREY).  blob_dev:
 *   n_pages records of YMK_JPEG_PAGE_WORDS words of which only words 0-4 are read; a record that is not a [h][w][3] page gets -1.
 *   max_pixels: h * w of the largest page (sizes the launch).  16-byte loads where the page's address allows, pixel by pixel
 *   where it does not and behind the last whole 16 pixels.  Nothing is allocated, nothing waited for. */
#define YMK_JPEG_MODE_420 0
#define YMK_JPEG_MODE_422 1
#define YMK_JPEG_MODE_444 2
#define YMK_JPEG_MODE_GREY 4
int ymk_jpeg_header_mode(int h, int w, int channels, int mode, int quality, unsigned char* out, int capacity);
int ymk_jpeg_header_opt_mode(int h, int w, int channels, int mode, int quality, unsigned char* out, int capacity, int* split_out);
int ymk_jpeg_scratch_bytes_mode(const int* h, const int* w, const int* channels, const int* modes, int n_pages, int64_t* sizes6_out);
int ymk_jpeg_scratch_bytes_opt_mode(const int* h, const int* w, const int* channels, const int* modes, int n_pages,
                                    int64_t* sizes9_out);
int ymk_jpeg_pages_grey(const int* blob_dev, int64_t blob_words, int n_pages, int64_t max_pixels, int* diff_dev, void* stream);
/* ymk_pil_resize_u8: Pillow's two-pass 8-bit resample (as ymk_pil_resize_to_chw: 22-bit coefficients, 1 << 21 bias, clip to
 *   uint8 between the passes) for n images in one launch, written as uint8 [oh][ow][C] in the source's channel order.  blob_dev:
 *   n records of YMK_PIL_RESIZE_U8_WORDS int32 words {source address low, high; H; W; C (1 | 3); oh; ow; ksize_x; ksize_y; word
 *   offsets in the blob of xbounds [ow][2], xcoefs [ow][ksize_x], ybounds, ycoefs; destination address low, high; 0}, then the
 *   tables.  A pixel whose taps leave the source, or whose tables leave the blob, is not written.  max_oh, max_ow: the largest
 *   output of the launch. */
#define YMK_PIL_RESIZE_U8_WORDS 16
int ymk_pil_resize_u8_record_words(void);
int ymk_pil_resize_u8(const int* blob_dev, int64_t blob_words, int n, int max_oh, int max_ow, void* stream);
/* ymk_crop_u8: n axis-aligned rectangles of uint8 pages copied into contiguous [ch][cw][C] destinations in one launch
 *   (yomitoku_amd/csrc/ymk_crop.hip; yomitoku_amd/figures.py: the figure crops of serve(figures=...)).  The pages are [H][W][C],
 *   C 1 | 3, contiguous, at any address; a destination is 16-byte aligned.  blob_dev: n records of YMK_CROP_U8_WORDS int32 words
 *   {source address low, high; H; W; C; x0; y0; cw; ch; destination address low, high; index of the crop's first 16-byte
 *   destination chunk in the launch; 0 ...}: a crop has ceil(ch cw C / 16) chunks, the crops' chunks follow one another and
 *   total_chunks is their sum (sizes the launch).  A record that does not fit - a side outside 1..16383, C not 1 | 3,
 *   x0 + cw > W, y0 + ch > H, a negative origin, a misaligned destination, chunks outside 0..total_chunks - is ignored:
 *   nothing is read or written for it.  Exactly ch cw C bytes are written per crop, none behind them; no load leaves
 *   [source, source + H W C).  n == 0 queues nothing.  Nothing is allocated, nothing waited for. */
#define YMK_CROP_U8_WORDS 16
int ymk_crop_u8_record_words(void);
int ymk_crop_u8(const int* blob_dev, int64_t blob_words, int n, int64_t total_chunks, void* stream);

/* ---- Group 4 encoder: CCITT T.6 files of the two-valued pages of a wave, opt-in (yomitoku_amd/csrc/ymk_ccitt.hip;
 * yomitoku_amd/ccitt.py; encode_jpeg_pages(bilevel="auto"), serve(jpeg=..., jpeg_bilevel="auto")).  DESIGN.md, "Two-valued
 * pages"; tests/ccitt_ref.py is the definition, and every stage equals it bit for bit.  A page - uint8 [h][w] or [h][w][3],
 * 1..16383 pixels on a side - is two-valued when every sample is 0 or 255 and, of three channels, B == G == R; 0 is black.
 * Page table (DEVICE, int32 words): n_pages records of YMK_G4_PAGE_WORDS words.
 *     word 0-1   address of the page's pixels (low, high); read by ymk_g4_test_pack only     word 2-4  h, w, channels (1 | 3)
 *     word 5     index of the page's row 0 among the rows of the call: the pages' rows follow one another, sum = total_rows
 *     word 6-7   WORD offset (low, high) in packed_dev of the page's packed rows: h rows of ceil(w / 32) words, 1 = black, the
 *                leftmost pixel of a word in its bit 31, zero bits behind column w
 *     word 8-9   BYTE offset (low, high) of the page's file in out_dev, a multiple of 4     word 10  the file's capacity in bytes
 *     word 11-12 WORD offset (low, high) in slots_dev of row 0's slot; a row's slot has ymk_g4_slot_words(w) words    13  0
 *     word 14-15 not read by these calls (the binariser's: see below); 0 otherwise
 * A record that does not fit the sizes the caller states is taken as absent (flag -1, length -1): nothing outside the stated
 * buffers is touched.  All buffers 8-byte aligned (out_dev 16).
 * ymk_g4_slot_words: ceil((7 w + 32) / 32): no row of w pixels takes more than 7 w + 21 bits (the proof is in ymk_ccitt.hip).
 * ymk_g4_file_capacity: the bytes no file of an h x w page exceeds - h such rows, EOFB, the pad.  HOST, -1 on a bad size.
 * ymk_g4_scratch_bytes: HOST arrays h, w -> sizes5_out = total_rows, then the bytes of packed_dev, slots_dev, rowbits_dev
 *   (uint32 [total_rows]) and rowoff_dev (uint64 [total_rows + n_pages]: page p's h + 1 bit offsets at word-5 + p).
 * ymk_g4_test_pack: flags_dev int32 [n_pages] zeroed on `stream`, then one launch over the pages: flags 0 = two-valued, 1 = not,
 *   -1 = no page; packed_dev = every page's packed rows (whatever its flag).  max_pixels: h w of the largest page.
 * ymk_g4_code_rows: one thread per row codes it against the packed row above (row 0: an all-white row) into its slot - the
 *   codes MSB first in 32-bit words - and its bit count into rowbits_dev.  Reads no flags: the table holds the pages to code.
 *   max_rows: h of the tallest page.
 * ymk_g4_scan: one block per page: rowoff_dev from rowbits_dev; lengths_dev[p] = the file's bytes (rows + EOFB, zero-padded to a
 *   byte), -1 where that exceeds the capacity.
 * ymk_g4_concat: one thread per 32-bit word of every file gathers its bits from the slots; EOFB and the pad behind the rows.
 *   Bytes of out_dev outside the files (and the up to 3 behind a file's end that complete its last word) are not written.
 *   max_capacity: the largest capacity of the table.
 * ymk_g4_encode_pages: rows, scan, concatenate in order on `stream`.  Nothing is allocated, nothing waited for. */
#define YMK_G4_PAGE_WORDS 16
int ymk_g4_page_words(void);
int ymk_g4_slot_words(int w);
int64_t ymk_g4_file_capacity(int h, int w);
int ymk_g4_scratch_bytes(const int* h, const int* w, int n_pages, int64_t* sizes5_out);
int ymk_g4_test_pack(const int* blob_dev, int64_t blob_words, int n_pages, int64_t max_pixels, int* flags_dev, uint32_t* packed_dev,
                     int64_t packed_bytes, void* stream);
int ymk_g4_code_rows(const int* blob_dev, int64_t blob_words, int n_pages, int64_t total_rows, int max_rows, const uint32_t* packed_dev,
                     int64_t packed_bytes, uint32_t* slots_dev, int64_t slot_bytes, int64_t out_bytes, uint32_t* rowbits_dev, void* stream);
int ymk_g4_scan(const int* blob_dev, int64_t blob_words, int n_pages, int64_t total_rows, int64_t packed_bytes, int64_t slot_bytes,
                int64_t out_bytes, const uint32_t* rowbits_dev, uint64_t* rowoff_dev, int* lengths_dev, void* stream);
int ymk_g4_concat(const int* blob_dev, int64_t blob_words, int n_pages, int64_t total_rows, int64_t packed_bytes, const uint32_t* slots_dev,
                  int64_t slot_bytes, const uint64_t* rowoff_dev, const int* lengths_dev, unsigned char* out_dev, int64_t out_bytes,
                  int64_t max_capacity, void* stream);
int ymk_g4_encode_pages(const int* blob_dev, int64_t blob_words, int n_pages, int64_t total_rows, int max_rows, const uint32_t* packed_dev,
                        int64_t packed_bytes, uint32_t* slots_dev, int64_t slot_bytes, uint32_t* rowbits_dev, uint64_t* rowoff_dev,
                        unsigned char* out_dev, int64_t out_bytes, int64_t max_capacity, int* lengths_dev, void* stream);

/* ---- Lossless pages: a zlib stream of the page's PNG-filtered rows in one dynamic-Huffman Deflate block, opt-in
 * (yomitoku_amd/csrc/ymk_flate.hip; yomitoku_amd/flate.py; encode_lossless_pages, encode_jpeg_pages(lossless=...), serve(jpeg=...,
 * jpeg_lossless=...)).  DESIGN.md, "Lossless pages"; tests/flate_ref.py is the definition, and every stage equals it byte for byte.
 *
 * Page table (DEVICE, int32 words): n_pages records of YMK_FLATE_PAGE_WORDS words.
 *     word 0-1   address of the page's pixels (low, high), uint8 H x W x channels, B G R       word 2-4  h, w, channels (1 | 3)
 *     word 5     index: the page's place in hist_dev, tables_dev, head_dev, sizes_dev (0 ... n_index - 1, in the order of 8-9)
 *     word 6-7   BYTE offset (low, high) of the page's filtered bytes in filt_dev; its tokens start at the same uint16 of tokens_dev
 *     word 8-9   the page's first segment in segtok_dev, segadler_dev, segbits_dev (its offsets: off_dev + that + 3 index)
 *     word 10-11 WORD offset of the page's slots in slots_dev      word 12-13 BYTE offset of its file in out_dev, a multiple of 4
 *     word 14    the file's capacity in bytes                      word 15  0, or 1 + the page's place in grey_dev
 * All offsets are those of the page with the channels it arrived with.  grey_dev (ymk_jpeg_pages_grey's answers, or null): a
 * three-channel page whose word there is 0 is coded as ONE channel - fewer segments of the same places, a smaller file.
 * A record that does not fit the sizes the call names is no page: nothing of it is read or written.
 *
 * ymk_flate_file_capacity: the bytes no file of an h x w x channels page exceeds (the proof is in ymk_flate.hip).  HOST, -1 on a
 *   bad size.
 * ymk_flate_scratch_bytes: HOST arrays h, w, channels -> sizes8_out = the segments; then the bytes of filt_dev; tokens_dev; each of
 *   segtok_dev, segadler_dev, segbits_dev; off_dev; slots_dev; each of hist_dev, tables_dev; head_dev.  sizes_dev: int32 [2 n_pages].
 * Every phase takes the table, n_index (the pages the per-page buffers have room for; n_pages <= n_index: a later phase may be
 * given some of the records of an earlier one) and the four sizes its records are checked against: the bytes of filt_dev (tokens_dev
 * has twice as many), the segments, the bytes of slots_dev and of out_dev.
 * ymk_flate_rows: hist_dev zeroed on `stream`, then one wave per row segment: the filtered bytes (a row: its type, then its bytes),
 *   the tokens (uint16: a literal's byte, or 0x8000 | index of the distance << 9 | length - 3), their count, the segment's Adler
 *   sums, and its symbol counts added to hist_dev [index][YMK_FLATE_HIST_WORDS] (286 literal / length symbols, 30 distance symbols).
 * ymk_flate_tables: one wave per page: tables_dev [index][YMK_FLATE_HIST_WORDS] = (code length << 16 | the code, first bit lowest) per
 *   symbol; head_dev [index][YMK_FLATE_HEAD_WORDS]: word 0 the file's bytes (-1: it exceeds the capacity), 1 the channels it is coded
 *   with, 2 the bits of 78 9C and the block's header, 3 the bits of the tail (end-of-block, pad, Adler-32), 4 the Adler-32, 5-6
 *   the tail's bit offset, 8-9 the tail's bits, 10.. the head's bits; sizes_dev [2 index] = word 0, [2 index + 1] = word 1.
 * ymk_flate_code: one wave per segment of every page that has a file: its tokens' bits into its slot, their count into segbits_dev.
 * ymk_flate_scan: one block per page: off_dev from segbits_dev; a page whose counts contradict its head gets -1 in both places.
 * ymk_flate_gather: one thread per 32-bit word of every file; no byte behind a file's end is written.  out_dev 16-byte aligned.
 * ymk_flate_encode_pages: the five in order on `stream`.  Nothing is allocated, nothing waited for. */
#define YMK_FLATE_PAGE_WORDS 16
#define YMK_FLATE_HIST_WORDS 320
#define YMK_FLATE_HEAD_WORDS 160
int ymk_flate_page_words(void);
int64_t ymk_flate_file_capacity(int h, int w, int channels);
int ymk_flate_scratch_bytes(const int* h, const int* w, const int* channels, int n_pages, int64_t* sizes8_out);
int ymk_flate_rows(const int* blob_dev, int64_t blob_words, int n_pages, int n_index, int64_t filt_bytes, int64_t segs, int64_t slot_bytes,
                   int64_t out_bytes, int max_rows, int max_row_segments, const int* grey_dev, unsigned char* filt_dev, uint16_t* tokens_dev,
                   uint32_t* segtok_dev, uint32_t* segadler_dev, int* hist_dev, void* stream);
int ymk_flate_tables(const int* blob_dev, int64_t blob_words, int n_pages, int n_index, int64_t filt_bytes, int64_t segs, int64_t slot_bytes,
                     int64_t out_bytes, const int* grey_dev, const int* hist_dev, const uint32_t* segadler_dev, uint32_t* tables_dev,
                     uint32_t* head_dev, int* sizes_dev, void* stream);
int ymk_flate_code(const int* blob_dev, int64_t blob_words, int n_pages, int n_index, int64_t filt_bytes, int64_t segs, int64_t slot_bytes,
                   int64_t out_bytes, int max_rows, int max_row_segments, const uint16_t* tokens_dev, const uint32_t* segtok_dev,
                   const uint32_t* tables_dev, const uint32_t* head_dev, uint32_t* slots_dev, uint32_t* segbits_dev, void* stream);
int ymk_flate_scan(const int* blob_dev, int64_t blob_words, int n_pages, int n_index, int64_t filt_bytes, int64_t segs, int64_t slot_bytes,
                   int64_t out_bytes, const uint32_t* segbits_dev, uint32_t* head_dev, uint64_t* off_dev, int* sizes_dev, void* stream);
int ymk_flate_gather(const int* blob_dev, int64_t blob_words, int n_pages, int n_index, int64_t filt_bytes, int64_t segs, int64_t slot_bytes,
                     int64_t out_bytes, const uint32_t* slots_dev, const uint32_t* head_dev, const uint64_t* off_dev, unsigned char* out_dev,
                     int64_t max_capacity, void* stream);
int ymk_flate_encode_pages(const int* blob_dev, int64_t blob_words, int n_pages, int n_index, int64_t filt_bytes, int64_t segs,
                           int64_t slot_bytes, int64_t out_bytes, int max_rows, int max_row_segments, const int* grey_dev,
                           unsigned char* filt_dev, uint16_t* tokens_dev, uint32_t* segtok_dev, uint32_t* segadler_dev, uint32_t* segbits_dev,
                           int* hist_dev, uint32_t* tables_dev, uint32_t* head_dev, uint64_t* off_dev, uint32_t* slots_dev,
                           unsigned char* out_dev, int64_t max_capacity, int* sizes_dev, void* stream);

/* ---- Binariser: grey-valued pages of a wave thresholded into the packed rows of the Group 4 encoder, opt-in
 * (yomitoku_amd/csrc/ymk_binarize.hip; yomitoku_amd/ccitt.py; encode_jpeg_pages(bilevel="otsu" | "adaptive"), serve(jpeg=...,
 * jpeg_bilevel=...)).  DESIGN.md, "Thresholded pages"; tests/binarize_ref.py is the definition, and every stage equals it bit
 * for bit.  A page is grey-valued when it has one channel, or three with B == G == R everywhere; p is that value, 1 = black.
 * The page table is the Group 4 encoder's; of it these calls read words 0-4 (pixels, h, w, channels), 6-7 (the packed rows) and
 *     word 14-15 WORD offset (low, high) in sat_dev of the page's summed-area table, h w words (ymk_bin_adaptive_pack only)
 * which the Group 4 calls ignore.  A record that does not fit the sizes the caller states is taken as absent (flag -1, nothing
 * written).  packed_dev, sat_dev 8-byte aligned.  Nothing is allocated, nothing waited for.  ymk_g4_encode_pages codes the rows.
 * ymk_bin_scratch_bytes: HOST arrays h, w -> sizes2_out = the bytes of hist_dev (uint32 [n_pages][256]) and of sat_dev (uint32,
 *   the pages' h w words one behind the other).
 * ymk_bin_test_hist: flags_dev int32 [n_pages] (and hist_dev, where not null) zeroed on `stream`, then one launch over the pages:
 *   flags 0 = grey-valued, 1 = not, -1 = no page; hist_dev[p] = the histogram of the page's first channel.
 * ymk_bin_otsu: one block per page: thresholds_dev[p] = the smallest t in 0..254 with both classes non-empty that maximises
 *   sigma(t) = double(d) * double(d) / double(w0 w1), d = m1 w0 - m0 w1 in int64 (w, m: counts and first moments of the classes
 *   <= t and > t); 0 where no t has both classes.
 * ymk_bin_otsu_pack: packed rows with black iff p <= thresholds_dev[page].
 * ymk_bin_adaptive_pack: three launches: row sums, column sums (a uint32 summed-area table that wraps; window sums are below 2^31
 *   and so exact), then packed rows with black iff p n 20 <= S 17 in 64 bits, n and S the pixel count and the sum of the window
 *   rows [y - r, y + r] x columns [x - r, x + r] clipped to the page, r = max(1, max(h, w) / 16).  max_h, max_w: the largest of
 *   the table. */
int ymk_bin_scratch_bytes(const int* h, const int* w, int n_pages, int64_t* sizes2_out);
int ymk_bin_test_hist(const int* blob_dev, int64_t blob_words, int n_pages, int64_t max_pixels, int* flags_dev, uint32_t* hist_dev,
                      void* stream);
int ymk_bin_otsu(int n_pages, const uint32_t* hist_dev, int* thresholds_dev, void* stream);
int ymk_bin_otsu_pack(const int* blob_dev, int64_t blob_words, int n_pages, int64_t max_pixels, const int* thresholds_dev,
                      uint32_t* packed_dev, int64_t packed_bytes, void* stream);
int ymk_bin_adaptive_pack(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, uint32_t* sat_dev, int64_t sat_bytes,
                          uint32_t* packed_dev, int64_t packed_bytes, void* stream);

/* ---- Page skew: the pages of a wave estimated and turned upright, opt-in (yomitoku_amd/csrc/ymk_deskew.hip;
 * yomitoku_amd/deskew.py; deskew_pages, serve(deskew=True)).  DESIGN.md, "Page skew"; tests/deskew_ref.py is the definition, and
 * every stage equals it bit for bit.  A page is uint8 [h][w] or [h][w][3] (B G R), 1..16383 pixels on a side.
 * Page table (DEVICE, int32 words): n_pages records of YMK_DSK_PAGE_WORDS words, laid out as the Group 4 encoder's.
 *     word 0-1   address of the page's pixels (low, high)     word 2-4  h, w, channels (1 | 3)     word 5, 10, 13  0
 *     word 6-7   WORD offset (low, high) in packed_dev of the page's ink: h rows of ceil(w / 32) words, 1 = ink, the leftmost
 *                pixel of a word in its bit 31, zero bits behind column w
 *     word 8-9   BYTE offset (low, high) in luma_dev of a three-channel page's Y plane, h w bytes, a multiple of 4
 *     word 11-12 address (low, high) of the destination page of ymk_dsk_rotate: same shape, 4-byte aligned, not the page itself
 *     word 14-15 WORD offset (low, high) in sat_dev of the page's summed-area table, h w words (the binariser's)
 * A record that does not fit the sizes the caller states is taken as absent (flag -1, k 0, scores 0, nothing written): nothing
 * outside the stated buffers is touched.  luma_dev, sat_dev, packed_dev, scores_dev, choice_dev 8-byte aligned.  Nothing is
 * allocated, nothing waited for.
 * Angle table (DEVICE for the launches, HOST for ymk_dsk_check_angles): int32 [n_angles][2] = (s_k, c_k) = round(2^14 sin, cos
 *   (k step)), k = -K .. K, n_angles = 2 K + 1 <= 401; s_max the largest |s_k|; dead: k is 0 where |k| < dead.
 * A profile in LDS has 16128 bins.  A page is ESTIMATED when h + 2 m(w) and w + 2 m(h) are at most that, m(n) = ceil((n - 1)
 *   s_max / 2^14): at the default table (5 degrees) every page up to 13700 x 13700.  A larger page gets scores 0, k 0 and flag
 *   0: it is copied, not failed.
 * ymk_dsk_check_angles: HOST: the table is odd, symmetric, 0 < c <= 2^14, s^2 + c^2 = 2^28 to rounding, its middle (0, 2^14);
 *   *s_max_out.
 * ymk_dsk_scratch_bytes: HOST arrays h, w, ch -> sizes5_out = the bytes of luma_dev (three-channel pages' planes, each rounded
 *   up to 16), sat_dev, packed_dev, scores_dev (uint64 [n_pages][n_angles]) and choice_dev; fits_out[p] (may be null) = 1 where
 *   the page is estimated.
 * ymk_dsk_luma: Y = (29 B + 150 G + 77 R + 128) >> 8 of every three-channel page into its plane; a one-channel page is its own.
 *   planes_dev: int32 [n_pages][16], written: the binariser's table of the planes, which ymk_bin_adaptive_pack (unchanged)
 *   takes to write the pages' ink into packed_dev.  max_pixels: h w of the largest page.
 * ymk_dsk_scores: scores_dev zeroed on `stream`, then one block per (page, angle, axis): the profile of the ink along the axis
 *   in LDS - row bin (y c + x s + off) >> 14, column bin (x c - y s + off) >> 14 -, S[page][angle] += sum_b (P[b + 1] - P[b])^2.
 * ymk_dsk_choose: one wave per page.  choice_dev: int32 [n_pages][YMK_DSK_CHOICE_WORDS]: word 0 k - the angle of the largest S,
 *   of equal ones the smallest |k|, then the negative; 0 where |k| < dead or 8 S_k < 9 S_0 -, word 1 the flag (1 estimated, 0
 *   too large, -1 no page), words 2-3 the largest S (uint64), 4-5 S_0, 6-7 zero.
 * ymk_dsk_rotate: reads k from choice_dev; the destination = the page turned by angle k (k = 0: a copy): u = 2 X - (w - 1), v =
 *   2 Y - (h - 1), SX = c u + s v + ((w - 1) << 14), SY = -s u + c v + ((h - 1) << 14), x0 = SX >> 15, fx = (SX >> 7) & 255,
 *   bilinear with weights in 1/256, + 32768 >> 16, a tap outside the page 255.  max_bytes: h w channels of the largest page.
 * ymk_dsk_pages: luma, ymk_bin_adaptive_pack, scores, choose and - `rotate` non-zero - rotate, in order on `stream`. */
#define YMK_DSK_PAGE_WORDS 16
#define YMK_DSK_CHOICE_WORDS 8
int ymk_dsk_page_words(void);
int ymk_dsk_check_angles(const int* table_host, int n_angles, int* s_max_out);
int ymk_dsk_scratch_bytes(const int* h, const int* w, const int* ch, int n_pages, int n_angles, int s_max, int64_t* sizes5_out,
                          int* fits_out);
int ymk_dsk_luma(const int* blob_dev, int64_t blob_words, int n_pages, int64_t max_pixels, unsigned char* luma_dev, int64_t luma_bytes,
                 int64_t packed_bytes, int64_t sat_bytes, int* planes_dev, void* stream);
int ymk_dsk_scores(const int* blob_dev, int64_t blob_words, int n_pages, const uint32_t* packed_dev, int64_t packed_bytes, int64_t sat_bytes,
                   int64_t luma_bytes, const int* table_dev, int n_angles, int s_max, uint64_t* scores_dev, void* stream);
int ymk_dsk_choose(const int* blob_dev, int64_t blob_words, int n_pages, int64_t packed_bytes, int64_t sat_bytes, int64_t luma_bytes,
                   const uint64_t* scores_dev, int n_angles, int s_max, int dead, int* choice_dev, void* stream);
int ymk_dsk_rotate(const int* blob_dev, int64_t blob_words, int n_pages, int64_t max_bytes, const int* table_dev, int n_angles,
                   const int* choice_dev, void* stream);
int ymk_dsk_pages(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, unsigned char* luma_dev, int64_t luma_bytes,
                  uint32_t* sat_dev, int64_t sat_bytes, uint32_t* packed_dev, int64_t packed_bytes, int* planes_dev, const int* table_dev,
                  int n_angles, int s_max, int dead, uint64_t* scores_dev, int* choice_dev, int rotate, void* stream);

/* ---- Layered pages: the pages of a wave separated into an ink mask and two low-resolution pictures, opt-in
 * (yomitoku_amd/csrc/ymk_mrc.hip; yomitoku_amd/mrc.py; separate_pages, encode_jpeg_pages(mrc=...), serve(jpeg=..., jpeg_mrc=...)).
 * DESIGN.md, "Layered pages"; tests/mrc_ref.py is the definition, and every stage equals it bit for bit.  A page is uint8 [h][w]
 * or [h][w][3] (B G R), 1..16383 pixels on a side.  bg_cell, fg_cell: the cells of the two layers, each 1, 2, 4, 8 or 16, one pair
 * per call.  A layer with cell d has a level 0 of H0 x W0 = ceil(h / d) x ceil(w / d) cells; its PYRAMID is the levels 0 .. L one
 * behind the other, level l + 1 of ceil(H_l / 2) x ceil(W_l / 2) cells, the last 1 x 1; a cell is one uint32: byte k the value of
 * channel k (a one-channel page: byte 0), byte 3 whether the cell is known.  Its IMAGE is uint8 [H0][W0][channels].
 * Page table (DEVICE, int32 words): n_pages records of YMK_MRC_PAGE_WORDS words, laid out as the page-skew table, so that
 * ymk_dsk_luma and ymk_bin_adaptive_pack take it unchanged.
 *     word 0-1   address of the page's pixels (low, high)     word 2-4  h, w, channels (1 | 3)     word 10, 13  0
 *     word 5     WORD offset in pyr_dev of the page's pyramids: the foreground's, then the background's
 *     word 6-7   WORD offset (low, high) in packed_dev of the page's ink: h rows of ceil(w / 32) words, 1 = ink, the leftmost
 *                pixel of a word in its bit 31, zero bits behind column w
 *     word 8-9   BYTE offset (low, high) in luma_dev of a three-channel page's Y plane, h w bytes, a multiple of 4
 *     word 11-12 BYTE offset (low, high) in layers_dev of the foreground's image, a multiple of 16; the background's follows at
 *                the next multiple of 16 behind it
 *     word 14-15 WORD offset (low, high) in sat_dev of the page's summed-area table, h w words (the binariser's)
 * A record that does not fit the sizes the caller states is taken as absent (flag -1, nothing written): nothing outside the stated
 * buffers is touched.  luma_dev, sat_dev, packed_dev, pyr_dev 8-byte aligned, layers_dev 16.  Nothing is allocated, nothing
 * waited for.  max_h, max_w: the largest of the table.
 * ymk_mrc_scratch_bytes: HOST arrays h, w, ch -> sizes6_out = the bytes of luma_dev, sat_dev, packed_dev, pyr_dev (fewer than 2^31
 *   words), layers_dev and flags_dev; places_out (may be null): int64 [n_pages][3] = word 5, words 11-12 and the byte offset of
 *   the background's image for pages laid out one behind the other.
 * ymk_mrc_cells: level 0 of both pyramids of every page in one pass over its pixels and its packed ink: the foreground selects
 *   the ink M, the background the pixels outside D = M dilated by the 3 x 3 square, clipped at the page's edge; a cell with N > 0
 *   selected pixels of sum S is known, value (2 S + N) / (2 N) per channel.
 * ymk_mrc_pull: one launch per level: a cell is known iff one of its up to four children is, value (2 sum + k) / (2 k) over its k
 *   known children.
 * ymk_mrc_push: flags_dev int32 [n_pages]: 1 = the top cell of both pyramids is known, 0 = not (no ink, or no paper: the images
 *   are not written), -1 = no page; then the images of the pages with flag 1: a level-0 cell's value, or where it is not known
 *   that of its nearest known ancestor.
 * ymk_mrc_pages: - planes_dev (int32 [n_pages][16], written) not null: ymk_dsk_luma and ymk_bin_adaptive_pack, the ink of the
 *   pages themselves; null: packed_dev holds the caller's ink - then cells, pull and push, in order on `stream`. */
#define YMK_MRC_PAGE_WORDS 16
int ymk_mrc_page_words(void);
int ymk_mrc_scratch_bytes(const int* h, const int* w, const int* ch, int n_pages, int bg_cell, int fg_cell, int64_t* sizes6_out,
                          int64_t* places_out);
int ymk_mrc_cells(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, int bg_cell, int fg_cell,
                  const uint32_t* packed_dev, int64_t packed_bytes, uint32_t* pyr_dev, int64_t pyr_bytes, int64_t layers_bytes, void* stream);
int ymk_mrc_pull(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, int bg_cell, int fg_cell, int64_t packed_bytes,
                 uint32_t* pyr_dev, int64_t pyr_bytes, int64_t layers_bytes, void* stream);
int ymk_mrc_push(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, int bg_cell, int fg_cell, int64_t packed_bytes,
                 const uint32_t* pyr_dev, int64_t pyr_bytes, unsigned char* layers_dev, int64_t layers_bytes, int* flags_dev, void* stream);
int ymk_mrc_pages(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, int bg_cell, int fg_cell,
                  unsigned char* luma_dev, int64_t luma_bytes, uint32_t* sat_dev, int64_t sat_bytes, uint32_t* packed_dev, int64_t packed_bytes,
                  int* planes_dev, uint32_t* pyr_dev, int64_t pyr_bytes, unsigned char* layers_dev, int64_t layers_bytes, int* flags_dev,
                  void* stream);

/* ---- Despeckled pages: connected-component labelling of packed rows, and the removal of every component below a size, opt-in
 * (yomitoku_amd/csrc/ymk_cc.hip; yomitoku_amd/despeckle.py; despeckle_masks, encode_g4_pages(despeckle=...), serve(jpeg=...,
 * jpeg_despeckle=...)).  DESIGN.md, "Despeckled pages"; tests/despeckle_ref.py is the definition, and the rows and the counts
 * equal it exactly.  The page table is the Group 4 encoder's; of it this call reads words 2-3 (h, w), 6-7 (the packed rows, which
 * are rewritten in place: 1 = black, the leftmost pixel of a word in its bit 31; the bits behind column w stay 0 and are pixels
 * of neither colour) and
 *     word 14-15 WORD offset (low, high) in labels_dev and in areas_dev of the page's h w words (where the binariser's
 *                summed-area table would be: ccitt.page_table(tables=True))
 * A record that does not fit the sizes the caller states - the buffers', or max_h, max_w, the largest of the table - is taken as
 * absent: its rows and its scratch are not touched, its counts are 0.  Buffers 4-byte aligned.
 * ymk_cc_scratch_bytes: HOST arrays h, w -> sizes2_out = the bytes of labels_dev and of areas_dev, int32 each: 8 bytes a pixel.
 * ymk_cc_despeckle_pages: counts_dev int32 [n_pages][4] zeroed on `stream`; then, n_black > 0: every 8-connected component of 1
 *   bits with fewer than n_black pixels is cleared, counts [0], [1] += such components, their pixels; then, n_white > 0, on the
 *   result: every 4-connected component of 0 bits with fewer than n_white pixels is set, counts [2], [3] likewise.  A component
 *   that touches the page's edge is no exception.  n_black, n_white: 0..65535, 0 = that colour is left alone (no launch).
 *   Four launches a colour - label the YMK_CC_TILE_W x YMK_CC_TILE_H tiles, merge across their seams, areas, apply -, in order
 *   on `stream`; no kernel waits for another thread's progress (the argument is in ymk_cc.hip).  Nothing is allocated, nothing
 *   waited for.  The result depends on the rows alone, not on timing.
 * ymk_cc_stage: one of a colour's four launches alone - stage 0 label, 1 merge, 2 areas, 3 apply; white: 0 = the black pass, else
 *   the white one; n: that colour's size; counts_dev is added to, not zeroed.  For tools/despeckle_serve_timing.py: the stages of
 *   a colour in order are that colour's pass.
 * Filtered ink (yomitoku_amd/despeckle.py: filter_masks; yomitoku_amd/mrc.py: the ink masks of layered pages with "despeckle" or
 * "blobs"; tests/ink_filter_ref.py is the definition, and the rows and the six counts equal it exactly):
 * ymk_cc_filter_scratch_bytes: sizes3_out = the bytes of labels_dev, areas_dev and boxes_dev (int32; three words a pixel, plane k of
 *   a page at word 3 (words 14-15) + k h w): 20 bytes a pixel in all.
 * ymk_cc_filter_pages: counts_dev int32 [n_pages][6] zeroed on `stream`; the two passes of ymk_cc_despeckle_pages, counts [0]-[3];
 *   then, side > 0, on their result a third, the blob pass: every 8-connected component of 1 bits with area a and bounding box bh x
 *   bw (inclusive extents) is cleared where bh >= side, bw >= side and 256 a >= fill bh bw (in 64 bits), counts [4], [5] += such
 *   components, their pixels.  side: 0 (no blob pass; boxes_dev is not read) or 2..16383; fill: 1..256, in 256ths of the box.  The
 *   blob pass is four launches - label, merge, boxes (every component's exact area and box), apply -; a record that does not fit
 *   boxes_bytes is absent like one that does not fit the labels.  Nothing is allocated, nothing waited for; the result depends on
 *   the rows alone.
 * ymk_cc_filter_stage: one of the blob pass's four launches alone - stage 0 label, 1 merge, 2 boxes, 3 apply; counts_dev
 *   ([n_pages][6]) is added to, not zeroed.  For tools/mrc_filter_timing.py. */
#define YMK_CC_TILE_W 64
#define YMK_CC_TILE_H 16
int ymk_cc_tile_w(void);
int ymk_cc_tile_h(void);
int ymk_cc_scratch_bytes(const int* h, const int* w, int n_pages, int64_t* sizes2_out);
int ymk_cc_despeckle_pages(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, uint32_t* packed_dev,
                           int64_t packed_bytes, int* labels_dev, int64_t labels_bytes, int* areas_dev, int64_t areas_bytes, int n_black,
                           int n_white, int* counts_dev, void* stream);
int ymk_cc_stage(int stage, int white, const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, uint32_t* packed_dev,
                 int64_t packed_bytes, int* labels_dev, int64_t labels_bytes, int* areas_dev, int64_t areas_bytes, int n, int* counts_dev,
                 void* stream);
int ymk_cc_filter_scratch_bytes(const int* h, const int* w, int n_pages, int64_t* sizes3_out);
int ymk_cc_filter_pages(const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, uint32_t* packed_dev,
                        int64_t packed_bytes, int* labels_dev, int64_t labels_bytes, int* areas_dev, int64_t areas_bytes, int* boxes_dev,
                        int64_t boxes_bytes, int n_black, int n_white, int side, int fill, int* counts_dev, void* stream);
int ymk_cc_filter_stage(int stage, const int* blob_dev, int64_t blob_words, int n_pages, int max_h, int max_w, uint32_t* packed_dev,
                        int64_t packed_bytes, int* labels_dev, int64_t labels_bytes, int* areas_dev, int64_t areas_bytes, int* boxes_dev,
                        int64_t boxes_bytes, int side, int fill, int* counts_dev, void* stream);

/* ---- DB post-processing on the host (replaces DBnetPostProcessor.boxes_from_bitmap,
 * postprocessor/dbnet_postporcessor.py:32-82: threshold, border following, min-area rectangles,
 * polygon-mean score, unclip, scaling to the original page).  prob_host: fp32 [h][w] HOST pointer
 * (the map after D2H); quads_out: int16 [capacity][4][2]; scores_out: double [capacity]. */
int ymk_db_postprocess(const float* prob_host, int h, int w, float thresh, float box_thresh, int min_size,
                       int max_candidates, float unclip_ratio, int dest_w, int dest_h, int16_t* quads_out,
                       double* scores_out, int capacity, int* count);

/* ---- table cell detector post-processing on the host (replaces find_holes_as_rects, table_cell_detector.py:116-143:
 * cv2.rectangle / morphologyEx(OPEN, close_ksize x close_ksize box, 3 iterations) / floodFill / findContours(EXTERNAL) /
 * boundingRect).  cell_boxes: int [n][4] (x1, y1, x2, y2) relative to the h x w table crop; rects_out: int [capacity][4],
 * each hole's bounding rectangle grown by `pad`, holes below min_area dropped; HOST pointers. */
int ymk_table_hole_rects(int h, int w, const int* cell_boxes, int n, int pad, int close_ksize, int min_area, int* rects_out,
                         int capacity, int* count);

/* ---- measurement aid for bench.py (not on the product path): between begin/end every launch of
 * the implicit-GEMM convolution kernel is bracketed by HIP events on its own stream; end returns
 * the summed kernel time, the algorithmic FLOPs (2*M*Cout*KH*KW*Cin, unpadded) and launch count.
 * ymk_prof_bytes: algorithmic HBM bytes of the launches since the last begin (input view + weights + output
 * [+ residual], each counted once) - what the PMC traffic of the same launches is compared with. */
int ymk_prof_begin(void);
/* Test / measurement knobs, process-wide (never touched by the product path; defaults in parentheses):
 *   "splitk_force" (-1)  >= 0: that split-K tile shape for every eligible launch      "no_splitk" (0)  1: conv_igemm only
 *   "conv_variant" (0)   alternative conv_igemm schedules for A/B runs (tools/conv_sweep.py): 0-4, 7, 8; any other value is an error
 *   "prof_dump" (0)      1: ymk_prof_end prints one line per launch      "parseq_unfused" (0)  1: per-op PARSeq decoder step at every width
 *   "conv_fast" (27)     bit 0: index shortcut of 1x1 / stride-1 layers, bit 1: residual rows fetched ahead, bit 3: K-tile rows of the
 *                        128 x 64 tile XOR-swizzled instead of padded (48 KB of LDS: three blocks per CU) and that tile for every
 *                        launch with K <= 512, bit 4: accumulators of ragged-Cout launches stored straight from registers;
 *                        bit 2: that direct epilogue for every plain store (A/B runs).  3 = the round-2 kernels.  Every setting
 *                        computes the same bits (tests/test_ops_gpu.py::test_conv_epilogue_variants_are_bit_identical).
 *   "dec_rows" (0)       samples per block of the fused greedy step: 0 = by row count, 1 / 2 / 3 / 4 forced (bit-identical results)
 *   "parseq_no_rowmax" (0)  1: the fused greedy loop writes every step's logits and arg-maxes them from memory (round-2 form);
 *                        0: the vocabulary head's epilogue reduces each 64-column tile to (max, column) and no AR logits exist
 *   "rowmax_tile" (0)    the kernel of that head where 128 x 128 tiles fill the chip: 0 = the A-stationary kernel, one column block
 *                        per block (K <= 192; else the 128 x 64 tile), 6 = 128 x 64 always (rounds 3-5) - the same pair table,
 *                        bit for bit, from each (tests/test_routes_gpu.py).  Any other value is an error and changes nothing
 * GELU: every kernel of the library (the exact-fp32 mode "conv_split" = 0 included, and the greedy decoder step) evaluates
 *   0.5 v (1 + erf(v / sqrt 2)) through one branch-free function (csrc/ymk_common.h gelu_f32: a rational erfc form on v_rcp_f32 /
 *   v_exp_f32) since round 5: absolute error < 5e-7 over the whole line (tests/test_ops_gpu.py), the size of the rounding of
 *   v x a libm-grade erff; the RELATIVE error of the negative tail (|GELU(v)| < 1e-6 beyond v = -5) is not bounded.  Results of
 *   "conv_split" = 0 are therefore not bit-comparable with rounds 1-4, whose kernels called erff.
 *   "conv_split" (-1)    process-wide operand precision of every model whose own "conv_split" parameter is unset, and of
 *                        ymk_op_conv2d: 0 = exact fp32 MFMA, 16 = two fp16 planes, 2 / 3 = bf16 planes (ymk_model_set_param above);
 *                        -1 = unset: models run their default (16), ymk_op_conv2d exact fp32.  Also set for a whole process by
 *                        the environment variable YMK_CONV_SPLIT (yomitoku_amd/_lib.py).
 *   "conv_split_tile" (0) forces one product kernel of that path (tests): 0 = each launch by the routing rule, 1 = the
 *                        register-staged kernel's 128 x 64 tile, 3 = its wide tile for the format (256 x 128 for three bf16
 *                        planes, else 128 x 128 x 16 waves); two fp16 planes only: 21 = the LDS-DMA kernel, 30 = the A-stationary
 *                        kernel ("astat" below).  Accepted: 0, 1, 3, 21, 30; any other value is an error and changes nothing
 *   "gemm_row_limit" (0) > 0: linear layers cut their rows into chunks of at most this many (rounded down to 1024s) - the chunking
 *                        that keeps an A operand view below the 4 GiB a buffer descriptor addresses, forced at test sizes
 *   "astat" (1)          1: chip-filling pointwise layers with K <= 192 and Cout > 64 run on the A-stationary kernel (K = 256 stays on
 *                        the register-staged kernel, where it measured ahead); 0: the round-4 routing (A/B runs).
 *                        "conv_split_tile" 30 forces that kernel for every launch it can run, K <= 256 (tests)
 *   "ar_publish" (1)     how a greedy step of the recogniser tells the host whether rows are still open: 1 = a one-thread launch
 *                        behind the greedy kernel writes the mapped host word (rows store a flag), 0 = the kernel's
 *                        last-arriving block does (rows count: rounds 1-5; A/B runs, tools/stress_call.py)
 *   "parseq_no_ln_fusion" (0)  1: the ViT blocks' LayerNorms as launches of their own (A/B runs, tests); 0: folded into the
 *                        operand load of the q|k|v and fc1 GEMMs wherever the A-stationary kernel takes them
 *   "act_planes" (1)     1: the tensor between a bottleneck's 1 x 1 reduction and its 3 x 3 convolution lives in HBM as the two fp16
 *                        planes the 3 x 3 multiplies with (written by the reduction's epilogue under the bound
 *                        max|x_in| x max row L1 norm + max|bias|, read by LDS-DMA without conversion) wherever both launches
 *                        fill the chip; 0: fp32 activations everywhere (A/B runs)
 *   "parseq_no_mlp_fusion" (0)  1: norm2 -> fc1 -> GELU -> fc2 of the ViT blocks as launches of their own through the [rows][4 D]
 *                        buffer (A/B runs, tests); 0: one launch with the hidden state on chip where the fused kernel runs it
 *   "amax_check" (0)     1: every fp16-split launch whose input came with a max|x| record from its producer ALSO measures the
 *                        input and compares (ymk_amax_check_counters) - the self-check of the record plumbing; 2: also names every
 *                        launch whose record lies BELOW the measured maximum on stderr (serialises the stream) */
int ymk_debug_option(const char* key, int value);
/* Tracing: with YMK_ROCTX=1 in the environment every forward (ymk_dbnet_forward, ymk_parseq_forward[_groups], ymk_rtdetr_forward),
 * ymk_parseq_token_stats, ymk_model_finalize and ymk_model_reserve runs inside a roctx range of its own name
 * (`rocprofv3 --marker-trace --kernel-trace`: which call a kernel belongs to).  The marker library is opened at run time
 * (librocprofiler-sdk-roctx.so, else libroctx64.so); without it, or without the variable, no range is pushed. */
/* Launch counters since the process started, for tests that must know a route was really taken: "astat_launches" (the
 * A-stationary short-K kernel), "ln_fused_launches" (those of them that carried a LayerNorm in their operand load),
 * "planes_written_launches" / "planes_read_launches" (convolutions whose output / input lives in HBM as fp16 planes),
 * "mlp_fused_launches" (ViT MLP halves run as one launch), "rowmax_wide_launches" (row-max heads on anything but the 128 x 64 tile),
 * "nar_forwards" (PARSeq forwards run in the non-autoregressive mode, "decode_ar" = 0).
 * And what a forward must NOT do (round 6): a ymk_*_forward whose workspace the caller sized first (ymk_model_reserve) never
 * allocates or frees device / pinned memory, never builds a weight copy and never waits for a stream - the split weight
 * copies and the max|x| words of the precision a model runs are built by ymk_model_finalize (and by ymk_model_set_param
 * when "conv_split" changes afterwards).  The fallbacks remain for callers of the bare ABI and are counted:
 * "allocs_in_forward" (hipMalloc / hipFree / hipHostMalloc / hipHostFree issued inside a forward), "arena_grows_in_forward"
 * (of those: the workspace grown because no reservation covered the shape), "lazy_panel_builds" (weight copies built on
 * first use: the process-wide precision switched after finalize), "syncs_in_forward" (stream waits those fallbacks made).
 * tests/test_serving_gpu.py holds all four at zero over both entry points of the analyzer. */
int ymk_stat(const char* key, int64_t* value);
/* out4 = {launches checked, records below the true max|x| (a bug), records more than 2^8 above it, largest record / truth
 * exponent distance} since the process started; synchronises the device. */
int ymk_amax_check_counters(int64_t* out4);
int ymk_prof_end(double* conv_ms, double* conv_flop, int64_t* conv_launches);
int ymk_prof_bytes(double* conv_bytes);
/* The launches of the span ymk_prof_end closed last, one row each in launch order: kernel time (ms), algorithmic FLOPs,
 * algorithmic HBM bytes (as above) and the MFMA products the kernel spends per fp32-grade product (0: exact fp32 MFMA,
 * 3: two fp16 or two bf16 planes, 6: three bf16 planes).  *count = how many there are; rows beyond `capacity` are not
 * written (capacity 0 with null arrays asks for the count).  What bench.py prices launch by launch against the closer
 * of the two roofs. */
int ymk_prof_launch_table(double* ms, double* flop, double* bytes, double* mfma_products, int64_t capacity, int64_t* count);

/* ---- single operators (exported for the parity tests; same kernels the models use) -----
 * NHWC fp32 tensors; weight in PyTorch OIHW order on the host. */
int ymk_op_conv2d(const float* x_dev, int n, int h, int w, int c, /* c % 4 == 0, or c == 4 with tap4 */
                  const float* w_host_oihw, int cout, int cin, int kh, int kw, const float* scale_host,
                  const float* bias_host, const float* res_dev, int stride, int pad, int dil, int act, int tap4,
                  float* y_dev, void* stream);
/* ymk_op_conv2d with nothing fixed (tests/test_conv_views_gpu.py): everything conv2d_impl's launch record carries that the
 * entry above pins.  x / res / y address the FIRST channel of a view into a wider NHWC buffer - in_ld / res_ld / out_ld floats
 * between pixels (the caller does the channel offset; Tensor::slice_c in the models); res_ld == 0 broadcasts one residual row
 * to every output pixel; res_post: y = res + act(conv) instead of act(conv + res).  w_host_oihw: [cout][c][kh][kw] (tap4: c == 4,
 * in_ld == 4).  stride_h x stride_w, one pad and one dilation for both axes.  row_group_dev [n*h*w] / group_open_dev (both or
 * neither; plain linear layers only - the launch then goes through the row-major GEMM view and its "gemm_row_limit" chunks):
 * M tiles all of whose rows sit in groups with group_open[g] == 0 keep their old contents.  amax_in_dev (optional): the max|x|
 * record of the input view, AMAX_REC_WORDS = 1024 words (32 lines of 32 words, the value in word 0 of each line);
 * amax_out_dev (optional, zeroed by the caller): receives max|y| of what the launch stored.  Kernels are selected as for
 * ymk_op_conv2d ("conv_split", "conv_split_tile", "splitk_force", "no_splitk", "conv_variant", "conv_fast").  No checks beyond null
 * and sign: the preconditions conv2d_impl enforces are part of what the tests exercise. */
int ymk_op_conv2d_view(const float* x_dev, int n, int h, int w, int c, int in_ld, const float* w_host_oihw, int cout, int kh, int kw,
                       int tap4, const float* scale_host, const float* bias_host, const float* res_dev, int res_ld, int res_post,
                       int stride_h, int stride_w, int pad, int dil, int act, const int* row_group_dev, const int* group_open_dev,
                       const unsigned* amax_in_dev, unsigned* amax_out_dev, float* y_dev, int out_ld, void* stream);
/* A producer convolution (c -> cout1) and the k x k convolution (cout1 -> cout2) that is its only reader, run the way
 * DBNetModel::bottleneck runs them under the fp16-split form (tests/test_conv_planes_gpu.py): where conv_planes_pair_ok accepts
 * the pair ("act_planes" on, both launches fill the chip, no residual on the producer, cout1 % 32 == 0, ...) the intermediate
 * mid_dev [n][h1][w1][cout1] holds fp16 PLANES (per pixel and 32-channel slice 32 high halves, then 32 low halves, scaled by
 * 2^(141 - e), e = the biased exponent of the record clamped to 27 .. 227) and mid_amax_dev (1024 words, zeroed here) the BOUND
 * pl_a max|x| + pl_b; otherwise mid_dev holds fp32 values and the record their measured maximum.  Square strides, contiguous
 * tensors; res1_dev / res2_dev: optional residuals (added before the activation); amax_in_dev: optional record of x (else the
 * producer measures it).  *planes_taken = 0 / 1, *pl_a / *pl_b = the producer's bound constants. */
int ymk_op_conv_planes_pair(const float* x_dev, int n, int h, int w, int c, const unsigned* amax_in_dev, const float* w1_host_oihw,
                            int cout1, int kh1, int kw1, int stride1, int pad1, int dil1, int act1, const float* scale1_host,
                            const float* bias1_host, const float* res1_dev, const float* w2_host_oihw, int cout2, int kh2, int kw2,
                            int stride2, int pad2, int dil2, int act2, const float* scale2_host, const float* bias2_host,
                            const float* res2_dev, float* mid_dev, unsigned* mid_amax_dev, float* y_dev, int* planes_taken,
                            float* pl_a, float* pl_b, void* stream);
/* rows x d LayerNorm (eps as given); attention over contiguous [b][l][heads*hd] q/k/v with optional
 * boolean masks (non-zero = blocked): mask_qk [lq][lk], kpm [b][lk]; use_small selects the masked
 * small-query kernel even without masks (otherwise the fp32-MFMA flash kernel runs). */
/* A 1 x 1 layer with K = c <= 256 through the A-stationary fp16-split kernel (yomitoku_amd/csrc/ymk_conv_astat.hip; the models'
 * short-K pointwise layers run on it since round 5) at ANY row count, where the library's own routing
 * only takes chip-filling launches: y[m][cout] = act(scale * (x'[m][c] . w^T) + bias + res), x' = x - or, with ln_g_host /
 * ln_b_host ([c], host), LayerNorm(x; gamma, beta, ln_eps) folded into the operand load (c = 128 or 192; the input's
 * max|x| record is then the LayerNorm's static output bound, as in the models).  w_host_oc: [cout][c] on the host, x / res / y
 * on the device.  Same arithmetic as the register-staged fp16-split kernel (ymk_op_conv2d under "conv_split" 16 and
 * "conv_split_tile" 3): compared bit for bit in tests/test_conv_astat_gpu.py.  The launch is repeated `reps` times;
 * *kernel_ms = HIP-event time of the last one.  Refuses (error) what the kernel cannot run. */
int ymk_op_conv1x1_astat(const float* x_dev, int m, int c, const float* w_host_oc, int cout, const float* scale_host,
                         const float* bias_host, const float* res_dev, int act, const float* ln_g_host, const float* ln_b_host,
                         float ln_eps, float* y_dev, int reps, float* kernel_ms, void* stream);

/* The MLP half of a ViT block in one launch (yomitoku_amd/csrc/ymk_vit_mlp.hip; what the PARSeq encoder runs per block when a
 * forward fills the chip): y[m][d] = x + fc2(GELU(fc1(LayerNorm(x; gamma, beta, eps)))), fc1 [f][d] + bias [f], fc2 [d][f] + bias
 * [d] (host, nn.Linear layout), x / y on the device.  d = 192, f = 768, m >= 32 641 (256 blocks of 128 rows) - refused (error)
 * otherwise.  Repeated `reps` times IN PLACE on y (timing); *kernel_ms = HIP-event time of the last launch. */
int ymk_op_vit_mlp(const float* x_dev, int m, int d, int f, const float* ln_g_host, const float* ln_b_host, float ln_eps,
                   const float* w1_host_fd, const float* b1_host, const float* w2_host_df, const float* b2_host, float* y_dev, int reps,
                   float* kernel_ms, void* stream);

int ymk_op_layernorm(const float* x_dev, int rows, int d, const float* g_dev, const float* b_dev, float eps,
                     float* y_dev, void* stream);
int ymk_op_attention(const float* q_dev, const float* k_dev, const float* v_dev, float* o_dev, int b, int heads, int lq,
                     int lk, int hd, float scale, const unsigned char* mask_qk_dev, const unsigned char* kpm_dev,
                     int use_small, void* stream);
/* The cross attention of PARSeq's non-autoregressive pass (yomitoku_amd/csrc/ymk_nar_attn.hip): ONE query table q [lq][heads * hd]
 * shared by all b samples; sample i attends its own keys / values - rows i * lk .. of k / v ([rows][heads * hd]), or, with the
 * device tables koff / klen ([b] each, both or neither), rows koff[i] .. koff[i] + klen[i] - 1 (klen >= 1; lk is then unused).
 * o [b][lq][heads * hd] = softmax(scale * q k^T) v per head, fp32 softmax, no masks.  heads <= 8, hd <= 96. */
int ymk_op_nar_cross_attention(const float* q_dev, const float* k_dev, const float* v_dev, float* o_dev, int b, int heads, int lq,
                               int lk, int hd, float scale, const int* koff_dev, const int* klen_dev, void* stream);
/* Two test-only entries that carry what the models' launch sites carry and ymk_op_layernorm / ymk_op_attention /
 * ymk_op_nar_cross_attention pin (tests/test_attention_views_gpu.py).  Neither allocates, synchronises or measures anything: each
 * is one call of the launcher the models call (csrc/ymk_seq.h).
 * layernorm_view: input rows of ldx floats, output rows of ldy floats (both >= d); in_rows_mod > 0 reads input row
 *   m % in_rows_mod - a [in_rows_mod][ldx] table broadcast over the rows.
 * attention_view: kernel 0 = flash_attention, 1 = small_attention, 2 = nar_cross_attention.  q / k / v / o point at the first
 *   column of head 0 inside rows of ldq / ldk / ldv / ldo floats; bs*: batch strides in floats (bsq may be 0 for the small kernel:
 *   one query table for the batch; the nar kernel always has one and takes bsq = 0).  mask_qk [lq][ld_mask] / kpm [b][ld_kpm]
 *   (non-zero = blocked): the small kernel only, and not together with tables.  (qoff, qlen) / (koff, klen): int32 [b] each,
 *   both of a pair or neither - the rows of sample i start at row off[i] of the buffer and number len[i] (>= 1), replacing the
 *   batch strides and lq / lk, which then are the maxima over the batch; the nar kernel takes the key pair only.  amax_*: the
 *   caller's max|x| records of 1024 words bounding q, k and v (any may be null, any two may be the same record): with all
 *   three, scale <= 1 and "conv_split" 16 in force the flash kernel multiplies fp16 planes, otherwise exact fp32. */
int ymk_op_layernorm_view(const float* x_dev, int ldx, int in_rows_mod, int rows, int d, const float* g_dev, const float* b_dev,
                          float eps, float* y_dev, int ldy, void* stream);
int ymk_op_attention_view(int kernel, const float* q_dev, const float* k_dev, const float* v_dev, float* o_dev, int b, int heads, int lq,
                          int lk, int hd, float scale, int ldq, int ldk, int ldv, int ldo, int64_t bsq, int64_t bsk, int64_t bsv,
                          int64_t bso, const unsigned char* mask_qk_dev, int ld_mask, const unsigned char* kpm_dev, int ld_kpm,
                          const int* qoff_dev, const int* qlen_dev, const int* koff_dev, const int* klen_dev,
                          const unsigned* amax_q_dev, const unsigned* amax_k_dev, const unsigned* amax_v_dev, void* stream);
int ymk_op_maxpool3x3s2(const float* x_dev, int n, int h, int w, int c, float* y_dev, void* stream);
int ymk_op_upsample_bilinear(const float* x_dev, int n, int h, int w, int c, int oh, int ow, const float* add_dev,
                             float* y_dev, void* stream);

/* ---- single operators of the RT-DETRv2 decoder (yomitoku_amd/csrc/ymk_det.hip; the launch functions ymk_rtdetr.cpp calls).
 * level_hw: HOST array {h0, w0, h1, w1, h2, w2} of the three token grids; token rows are level-major across the b images:
 * row(i, t) = b * off[l] + i * h[l] * w[l] + (t - off[l]) for token t of level l of image i (off[l]: tokens of the levels
 * before l).  ntok = the sum of h[l] * w[l].
 * topk_tokens: logits [rows][nc] -> idx [b][k]: per image the k tokens of largest max-over-classes logit, in rank order
 *   (descending value, lowest token id among equal values); 1 <= k <= min(2048, ntok).  Allocates the b * ntok key words itself.
 * gather_queries: idx [b][k] (each in [0, ntok), checked) -> content [b][k][d] = om[row(i, idx)], ref [b][k][4] =
 *   sigmoid(bbox[row][:] + anchors[idx][:]) (anchors: [ntok][4]).
 * refine_boxes: out[i] = sigmoid(delta[i] + inverse_sigmoid(ref[i])), inverse_sigmoid clipping at 1e-5, over n floats.
 * mask_rows: out[row(i, t)][:] = valid[t] * in[row(i, t)][:] (valid: [ntok]); d a multiple of 4.
 * deform_sample: multi-scale deformable attention sampling, 8 heads x 32 channels x 3 levels x 4 points: offs [b*k][8][3][4][2],
 *   attw [b*k][8][12] (soft-maxed over the 12), ref [b*k][4] (cx, cy, w, h), value rows of ldv floats (>= 256; the model's
 *   value_dev points inside a [rows][6 * 256] buffer) -> out [b*k][256]. */
int ymk_op_topk_tokens(const float* logits_dev, int b, const int* level_hw, int nc, int k, int* idx_dev, void* stream);
int ymk_op_gather_queries(const float* om_dev, const float* bbox_dev, const float* anchors_dev, const int* idx_dev, int b,
                          const int* level_hw, int k, int d, float* content_dev, float* ref_dev, void* stream);
int ymk_op_refine_boxes(const float* delta_dev, const float* ref_dev, float* out_dev, int64_t n, void* stream);
int ymk_op_mask_rows(const float* in_dev, const float* valid_dev, int b, const int* level_hw, int d, float* out_dev, void* stream);
int ymk_op_deform_sample(const float* offs_dev, const float* attw_dev, const float* ref_dev, const float* value_dev, int ldv, int b,
                         const int* level_hw, int k, float* out_dev, void* stream);
/* NHWC fp32, c a multiple of 4: AvgPool2d(2, 2, 0, ceil_mode=True) -> [n][(h+1)/2][(w+1)/2][c]; nearest x2 -> [n][2h][2w][c] */
int ymk_op_avgpool2x2_ceil(const float* x_dev, int n, int h, int w, int c, float* y_dev, void* stream);
int ymk_op_upsample_nearest2x(const float* x_dev, int n, int h, int w, int c, float* y_dev, void* stream);
/* Test-only entries for the memory-bound kernels between the convolutions and for the max|x| passes, in the forms the models
 * launch them (tests/test_glue_views_gpu.py).  Each is one call of the launch function the models call; none allocates or waits.
 * *_view: the operators above with the caller's pixel strides - x_dev / y_dev / add_dev point at the first channel of the view
 *   inside pixels of in_ld / out_ld / add_ld floats (multiples of 4, >= c; the pointers 16-byte aligned), as Tensor::slice_c makes
 *   them.  The pooling and nearest entries derive the output size; bilinear takes any oh, ow >= 1, add_dev may be null.
 * nchw3_to_nhwc4: x [n][3][h][w] -> y [n][h][w][4], channel 3 zero (the first kernel of every forward).
 * add_bcast: out[r][:] = a[r][:] + b[r % rows_mod][:] over m rows of d floats (d a multiple of 4), contiguous.
 * absmax: one launch of k_absmax with the library's grid rule over `pixels` pixels of c floats at pixel stride ld: atomicMax of
 *   the fp32 bit pattern of max|x| into word 0 of slot_dev, and word 0 of next_dev cleared.
 * amax_merge: word 0 of each of the 32 lines of the record dst_dev = the larger of dst's and src's (1024 words each); a null
 *   record makes it a no-op. */
int ymk_op_maxpool3x3s2_view(const float* x_dev, int n, int h, int w, int c, int in_ld, float* y_dev, int out_ld, void* stream);
int ymk_op_avgpool2x2_ceil_view(const float* x_dev, int n, int h, int w, int c, int in_ld, float* y_dev, int out_ld, void* stream);
int ymk_op_upsample_nearest2x_view(const float* x_dev, int n, int h, int w, int c, int in_ld, float* y_dev, int out_ld, void* stream);
int ymk_op_upsample_bilinear_view(const float* x_dev, int n, int h, int w, int c, int in_ld, int oh, int ow, const float* add_dev,
                                  int add_ld, float* y_dev, int out_ld, void* stream);
int ymk_op_nchw3_to_nhwc4(const float* x_nchw_dev, int n, int h, int w, float* y_dev, void* stream);
int ymk_op_add_bcast(const float* a_dev, const float* b_dev, int rows_mod, int m, int d, float* out_dev, void* stream);
int ymk_op_absmax(const float* x_dev, int64_t pixels, int c, int ld, unsigned* slot_dev, unsigned* next_dev, void* stream);
int ymk_op_amax_merge(unsigned* dst_dev, const unsigned* src_dev, void* stream);

/* ---- single operators of the DBNet++ head (ymk_dbnet.cpp).
 * deconv2x2: act(ConvTranspose2d(cin, cout, 2, stride 2)(x) * scale + bias) through the convolution path's EPI_DECONV2X2
 *   epilogue and the model's panel packing; w_host [cin][cout][2][2], scale / bias [cout] (host, may be null); x [n][h][w][cin],
 *   y [n][2h][2w][cout].  Operand precision as ymk_op_conv2d ("conv_split", "conv_split_tile").
 * deconv2x2_to1_sigmoid: sigmoid(ConvTranspose2d(64, 1, 2, stride 2)(x) + bias); w_host [64][4] (= [64][1][2][2]), x [n][h][w][64],
 *   y [n][2h][2w].
 * dbnet_asf: ScaleChannelSpatialAttention + the per-scale multiply of ScaleFeatureSelection on the ASF conv's output ax
 *   [n][h][w][64] and the concatenated features fuse [n][h][w][256] -> out [n][h][w][256]; w1_host [cmid][64], w2_host [64][cmid]
 *   (channel_wise), sp33_host [9], sp11 (spatial_wise), watt_host [4][64] (attention_wise). */
int ymk_op_deconv2x2(const float* x_dev, int n, int h, int w, int cin, const float* w_host, int cout, const float* scale_host,
                     const float* bias_host, int act, float* y_dev, void* stream);
int ymk_op_deconv2x2_to1_sigmoid(const float* x_dev, int n, int h, int w, const float* w_host, float bias, float* y_dev, void* stream);
int ymk_op_dbnet_asf(const float* ax_dev, const float* fuse_dev, int n, int h, int w, const float* w1_host, const float* w2_host,
                     int cmid, const float* sp33_host, float sp11, const float* watt_host, float* out_dev, void* stream);

/* ---- single operators of the PARSeq greedy decode (yomitoku_amd/csrc/ymk_decstep.hip, ymk_seq.hip; the launch functions
 * ymk_parseq.cpp calls, one launch per call; tests/test_parseq_decstep_gpu.py, tests/test_parseq_greedy_ops_gpu.py).
 * parseq_dec_step: the fused decoder step of position `step` for b samples (k_parseq_dec_step_rows): content row of tok[i][step]
 *   -> norm_c -> K|V appended as row `step` of skv [b][ns][2 d]; query `step` = pos_queries + self attention over rows 0..step,
 *   + cross attention over the sample's memkv rows ([.][2 d]: K then V; sample i owns rows i * l .. i * l + l - 1, or - with the
 *   device tables mem_off / mem_len, both or neither - rows mem_off[i] .. + mem_len[i] - 1, 1 <= mem_len <= l), + MLP, decoder.norm
 *   -> out [b][d].  Host weights in nn.Linear layout ([out][in]): the two in_proj_weight [3 d][d] / in_proj_bias [3 d], the two
 *   out_proj, linear1 [f][d], linear2 [d][f]; they are transposed by the function the model's finalize uses.  ln_host: ten host
 *   vectors [d] - weight, bias of norm_q, norm_c, norm1, norm2, decoder.norm in that order (the norm_q pair may be null: the
 *   step reads it through qsa only).  emb_host [ntok][d], posq_host [ns][d] (pos_queries), qsa_host [ns][d] = the self attention's
 *   query projection of norm_q(pos_queries), as given.  tok [b][ns] (ids in [0, ntok): the kernel trusts them).
 *   prev_not_done (device word, may be null): 0 = a speculative step, nothing is written.  gid [b] / gopen [ns][ng] (both or
 *   neither): row i belongs to mini-batch gid[i]; a row whose gopen[step - 1][gid] is 0 is frozen (neither out nor skv written).
 *   Refuses (error, nothing launched) what parseq_dec_step_supported refuses: d <= 256, d % 4 == 0, heads <= 8, d / heads a
 *   power of two >= 4, f <= 1024, f % 4 == 0, l <= 1024, ns <= 1024.  Rows per block: ymk_debug_option("dec_rows").
 *   Uploads the weights on every call and waits for the stream before it returns.
 * greedy_step: k_greedy_step in the flag form the recogniser runs (open rows STORE 1 into *not_done and gopen[step][gid]; no
 *   mapped host word - the counting form of "ar_publish" 0 is not exported): arg-max of row i of logits (c floats, row stride
 *   ld_b floats; partials = 1: c <= 256 (max, column-as-int-bits) pairs, lowest column among equal maxima) -> raw[i][step]; for
 *   step + 1 < num_steps the next context token tok[i][step + 1] - <eos> instead when the repetition detector (rep_on, periods
 *   1..period_max, a run of min_run_p1 for period 1, min_repeats units otherwise) fires on tok[i][1..step + 1]; state [b][4] =
 *   {has_eos, rep_done, rep_cut (-1 none), retired}.  prev_not_done / gid / gopen as above (a frozen row only gets raw = eos).
 * greedy_step_retire: the same launch with the model parameter "retire_rows" as an argument (0: greedy_step).  1: a row whose
 *   raw arg-max of this step is <eos> gets state[i][3] = 1 and is frozen from the next step on, whatever its mini-batch does:
 *   raw = eos, no token, no repetition-detector advance, no vote in *not_done / gopen.  A row that only the repetition detector
 *   stopped (has_eos set, arg-max not <eos>) is not retired.
 * parseq_dec_step_state: parseq_dec_step with the greedy kernel's state [b][4] (may be null): a row whose state[i][3] != 0 is
 *   treated as a frozen row is (neither out nor skv written; a block of such rows only returns).
 * rowmax_head: the greedy loop's vocabulary head, pairs [m][2 * ceil(cout / 64)] = per 64-column tile (max, column-as-int-bits)
 *   of x [m][k] . w_host[cout][k]^T + bias_host (may be null); k % 4 == 0.  split 0: exact fp32 (64-row tiles); 16: the fp16-split
 *   form with amax_in_dev = the record of x (128-row tiles where the launch fills the chip).  An M tile is skipped (its pairs
 *   keep their contents) when none of its rows is needed: row i is needed when group_open[row_group[i]] != 0 (both or neither;
 *   absent = needed) and row_dead[i * row_dead_ld] == 0 (may be null).  Uploads the weights and waits for the stream.
 * refine_prep: tok2[i][t] = t == 0 ? bos : raw[i][t - 1], kpm[i][t] = an <eos> at or before t in tok2, or t >= gsteps[gid[i]]
 *   (gid / gsteps: both or neither), for t < s_len <= ld_tok; kpm is [b][ld_tok] bytes.
 * rep_cut: for rows with 0 <= state[i][2] < s_len: logits[i][cut][:] = -30, [eos_id] = +30 (logits [b][ld_b], ld_b >= s_len * c).
 * row_argmax: out[r] = first maximal column of row r of logits [rows][c] (torch.argmax; an all -inf row gives 0).
 *   ymk_parseq_token_stats above is the same reduction plus the arg-max's probability.
 * ctx_embed_ln: out[i][pos][:] = LayerNorm(sqrt(d) emb[tok[i][pos]] + (pos > 0 ? posq[pos - 1] : 0); g, b, eps) for pos0 <= pos <
 *   pos0 + npos; tok [b][ld_tok], out [b][out_rows][d]; d <= 1024 (refused otherwise).  All pointers device.
 * init_decode: tok [b][ld_tok] = pad with column 0 = bos, state [b][4] = {0, 0, -1, 0}; ld_tok >= 4.
 * tile_rows: dst [b][rows][d] = src [rows][d] (rows * d a multiple of 4).
 * add_pos_embed: x [b][gh][gw][d] += pos[(r * full_gw + c)][d] in place (gw <= full_gw: the dynamic-width crop), d % 4 == 0. */
int ymk_op_parseq_dec_step(int d, int heads, int f, const float* sa_in_w_host, const float* sa_in_b_host, const float* sa_out_w_host,
                           const float* sa_out_b_host, const float* ca_in_w_host, const float* ca_in_b_host,
                           const float* ca_out_w_host, const float* ca_out_b_host, const float* lin1_w_host, const float* lin1_b_host,
                           const float* lin2_w_host, const float* lin2_b_host, const float* const* ln_host, const float* emb_host,
                           int ntok, const float* posq_host, const float* qsa_host, const int* tok_dev, float* skv_dev,
                           const float* memkv_dev, const int* mem_off_dev, const int* mem_len_dev, const int* prev_not_done_dev,
                           const int* gid_dev, const int* gopen_dev, int ng, int step, int b, int l, int ns, float* out_dev,
                           void* stream);
int ymk_op_greedy_step(const float* logits_dev, int64_t ld_b, int c, int step, int num_steps, int* tok_dev, int* raw_dev, int ld_tok,
                       int* state_dev, int eos_id, int rep_on, int period_max, int min_run_p1, int min_repeats, int* not_done_dev,
                       const int* prev_not_done_dev, const int* gid_dev, int* gopen_dev, int ng, int partials, int b, void* stream);
int ymk_op_greedy_step_retire(const float* logits_dev, int64_t ld_b, int c, int step, int num_steps, int* tok_dev, int* raw_dev,
                              int ld_tok, int* state_dev, int eos_id, int rep_on, int period_max, int min_run_p1, int min_repeats,
                              int* not_done_dev, const int* prev_not_done_dev, const int* gid_dev, int* gopen_dev, int ng, int partials,
                              int retire_rows, int b, void* stream);
int ymk_op_parseq_dec_step_state(int d, int heads, int f, const float* sa_in_w_host, const float* sa_in_b_host,
                                 const float* sa_out_w_host, const float* sa_out_b_host, const float* ca_in_w_host,
                                 const float* ca_in_b_host, const float* ca_out_w_host, const float* ca_out_b_host,
                                 const float* lin1_w_host, const float* lin1_b_host, const float* lin2_w_host, const float* lin2_b_host,
                                 const float* const* ln_host, const float* emb_host, int ntok, const float* posq_host,
                                 const float* qsa_host, const int* tok_dev, float* skv_dev, const float* memkv_dev,
                                 const int* mem_off_dev, const int* mem_len_dev, const int* prev_not_done_dev, const int* gid_dev,
                                 const int* gopen_dev, int ng, const int* state_dev, int step, int b, int l, int ns, float* out_dev,
                                 void* stream);
int ymk_op_rowmax_head(const float* x_dev, int m, int k, const float* w_host, int cout, const float* bias_host, int split,
                       const int* row_group_dev, const int* group_open_dev, const int* row_dead_dev, int row_dead_ld,
                       const unsigned* amax_in_dev, float* pairs_dev, void* stream);
int ymk_op_refine_prep(const int* raw_dev, int ld_tok, int s_len, int bos_id, int eos_id, int* tok2_dev, unsigned char* kpm_dev, int b,
                       const int* gid_dev, const int* gsteps_dev, void* stream);
int ymk_op_rep_cut(float* logits_dev, int64_t ld_b, int c, int s_len, const int* state_dev, int eos_id, int b, void* stream);
int ymk_op_row_argmax(const float* logits_dev, int rows, int c, int* out_dev, void* stream);
int ymk_op_ctx_embed_ln(const int* tok_dev, int ld_tok, int pos0, int npos, const float* emb_dev, const float* posq_dev,
                        const float* g_dev, const float* b_dev, float eps, float* out_dev, int out_rows, int d, int b, void* stream);
int ymk_op_init_decode(int* tok_dev, int ld_tok, int* state_dev, int bos_id, int pad_id, int b, void* stream);
int ymk_op_tile_rows(const float* src_dev, int rows, int d, float* dst_dev, int b, void* stream);
int ymk_op_add_pos_embed(float* x_dev, const float* pos_dev, int b, int gh, int gw, int full_gw, int d, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YMK_H */
