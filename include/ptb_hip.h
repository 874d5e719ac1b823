/*
 * ptb_hip.h -- C ABI of libptb_hip.so: hand-written gfx950 (MI355X / CDNA4) HIP kernels for the
 * pytorch-toolbelt large-image inference hot path (tile merge, TTA de-augment/augment, loss reductions).
 *
 * The reference (BloodAxe/pytorch-toolbelt) is pure Python: it has no FFI / operator registry, so the
 * drop-in boundary is its Python module surface.  Each entry point below replaces the torch
 * op chain of the cited reference function; `pytorch_toolbelt_amd` binds them with ctypes (see INTEGRATION.md
 * for the stub a reference maintainer would add).
 *
 * Conventions
 *   - plain pointers + sizes only; every tensor is contiguous row-major ("NCHW"); device pointers unless marked HOST.
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); nothing synchronises, nothing allocates.
 *   - returns 0 on success, a negative PTB_E* code otherwise; never throws, never aborts.
 *   - float = IEEE fp32.  Arithmetic is not contracted (no FMA fusion) where the reference's result is
 *     reproduced bit-for-bit (tile accumulation, merge division).
 */
#ifndef PTB_HIP_H
#define PTB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PTB_OK 0
#define PTB_EINVAL (-1)      /* bad argument (null pointer, non-positive size, unknown enum) */
#define PTB_EUNSUPPORTED (-2) /* legal for the reference but not implemented natively (caller must raise) */
#define PTB_ELAUNCH (-3)     /* HIP launch failed; see ptb_last_hip_error() */
#define PTB_EBOUNDS (-4)     /* tile rectangle leaves the accumulator */
#define PTB_EHELD (-6)       /* ptb_band_plan_submit_next: the batch lives in memory of a batch a later launch still reads */
#define PTB_EFRESH (-5)      /* first-touch bitmap cannot be honoured for this batch: zero-fill the fresh blocks, then call
                                again with fresh = NULL */

typedef void* ptb_stream_t; /* hipStream_t */

/* View transform code: bit0 = transpose, bit1 = flip source rows, bit2 = flip source cols.
 *   out[i][j] = src[r][c], (r,c) = (j,i) if transpose else (i,j); r -> rows-1-r if bit1; c -> cols-1-c if bit2.
 * The 8 codes are the dihedral group D4 (inference/functional.py:47-132 of the reference). */
#define PTB_VIEW_IDENT 0
#define PTB_VIEW_TRANSPOSE 1
#define PTB_VIEW_FLIPUD 2
#define PTB_VIEW_ROT90_CW 3      /* x[N-1-j][i]   */
#define PTB_VIEW_FLIPLR 4
#define PTB_VIEW_ROT90_CCW 5     /* x[j][N-1-i]   */
#define PTB_VIEW_ROT180 6
#define PTB_VIEW_ANTITRANSPOSE 7 /* x[N-1-j][N-1-i] */

/* Reductions of _deaugment_averaging (inference/tta.py:63-96, inference/functional.py:250-333). */
#define PTB_RED_SUM 0
#define PTB_RED_MEAN 1
#define PTB_RED_GMEAN 2
#define PTB_RED_HMEAN 3
#define PTB_RED_HARMONIC1P 4
#define PTB_RED_LOGODD 5
#define PTB_RED_LOG1P 6

/* element type of the model outputs a `_t` entry point reads (accumulators and results are always fp32) */
#define PTB_F32 0
#define PTB_F16 1
#define PTB_BF16 2
/* further element types of the volumes ptb_volume_split reads (every one widens to fp32 exactly) */
#define PTB_U8 3
#define PTB_I16 4
#define PTB_U16 5
/* or-ed into the `in_dtype` of ptb_deaug_accumulate_t / ptb_accumulate_planned(2) / ptb_merge_band / ptb_band_plan_submit(_rank): the
 * reduced value is rounded to the (fp16 / bf16) source type -- round to nearest even, NaN -> quiet NaN, like torch's `.to(dtype)` --
 * before it is multiplied by the window.  That is what the reference's two calls compute on half-precision model outputs
 * (torch.autocast): `tta.*_image_deaugment(y)` returns a HALF tensor (inference/tta.py:442-467), `integrate_batch` widens it
 * (inference/tiles.py:334-335).  No effect on PTB_F32 sources. */
#define PTB_ROUND_SRC 0x100
/* or-ed into the `in_dtype` of ptb_deaug_reduce_t / ptb_deaug_accumulate_t / ptb_accumulate_planned(2) / ptb_merge_band /
 * ptb_band_plan_submit(_rank): `in` / `batch` / the tile sources point at channels-last memory, [V*B, th, tw, C] -- element (n, c, i, j)
 * at ((n * th + i) * tw + j) * C + c, what a model in torch.channels_last returns -- instead of the planar [V*B, C, th, tw].  The strides
 * keep their meaning (elements between tiles / views: C*th*tw, B*C*th*tw), every output stays planar fp32, and every result has the bits
 * the planar kernels give on the copied batch.  The layout is part of a band plan's per-image configuration (ptb_band_plan_submit_next
 * inherits it): a batch whose layout differs from the image's first batch gets PTB_EUNSUPPORTED with nothing launched, like a dtype
 * change.  With an unknown dtype the result is PTB_EINVAL, as without the flag.
 * The 5-D case: or-ed into the `dtype` of ptb_volume_mirror_reduce, the `in_dtype` of ptb_volume_mirror_accumulate and the `in_dtype` of
 * ptb_volume_plan_submit, `src` / `tiles` / `batch` address [V*B, d, h, w, C] memory -- element (n, c, z, y, x) at
 * (((n * d + z) * h + y) * w + x) * C + c, what a model in torch.channels_last_3d returns.  tile_stride / view_stride keep their meaning (a
 * tile is still one contiguous block of C*d*h*w elements); everything written stays as it is -- the dense result of the source type,
 * the planar fp32 accumulators, the PTB_CROP_* results and layouts -- with the bits the planar kernels give on the copied batch; argument
 * checks keep their order and codes.  The layout is part of a volume plan's per-image configuration, like the dtype.
 * ptb_volume_mirror, a bit copy, refuses the flag (PTB_EINVAL). */
#define PTB_SRC_CHANNELS_LAST 0x200

int ptb_version(void);
/* hipGetErrorString of the last failing HIP call made by this library on this thread ("" if none). */
const char* ptb_last_hip_error(void);
/* Tuning knob for benchmarks/tests: key 0 = chunk rows of the view kernels (16|32|64), 1 = force scalar kernels (0|1),
 * 2 = non-temporal streaming loads in the view kernels (0|1, default 1), 3 = LDS-staged multiscale kernel (0|1, default 1),
 * 4 = workgroups per loss-kernel launch (0 = per-kernel default), 5 = fused focal + statistics forward with 2 pixels per lane
 * (0|1, default 1), 6 = output tile rows of the fused multiscale kernel (16|32|64, default 32),
 * 7 = softmax focal backward that keeps the per-class terms in registers: pixels per lane (0 = off | 2 | 4, default 4),
 * 8 = the fused loss forward prefetches the next pixel group into a second register buffer (0|1, default 0: measured no gain),
 * 9 = XCD-aware tile order of the fused multiscale kernel: strip width in tile columns (0 = row-major order over all XCDs, default 64),
 * 10 = workgroup order of the band plan kernel (A/B): 0 = channels of a work item adjacent (default, fastest), 1 = every XCD a contiguous
 * eighth of the list, 2 = channel-major,
 * 11 = rows per work item of band plans created afterwards (32 | 64, default 64),
 * 12 = fused focal + Dice + Jaccard forward: 0 = lean kernel, 1 = packed-fp32 kernel (default), 2 = packed-fp32 with prefetch,
 * 13 = workgroups of the packed-fp32 forward (default 512), 15 = output tile width of the fused multiscale kernel (64 | 128, default 128),
 * 16 = non-temporal gradient stores in the fused loss backward (0|1, default 1), 17 = XCD-contiguous tile order of the Lovasz radix
 * scatter (0|1, default 1), 18 = one-launch finish of a rank's image in ptb_band_plan_finish_rank (0|1, default 1),
 * 19 = the gradient-binning scatter of the Lovasz training path also evaluates the loss (0|1, default 1; 0: separate lovasz_dot_kernel),
 * 20 = Dice / Jaccard statistics (logits + labels, no ignore) and the default BinaryFocalLoss on label maps run as the statistics-only /
 * focal-only instances of the packed streaming kernel of the fused loss (0|1, default 1; 0: the lean kernels),
 * 21 = the band plan kernel requests the next covering tile before it finishes the current one (0: never, 1: half / bf16 model outputs,
 *      2: fp32 as well; default 2),
 * 22 = (A/B, round 6) odd work items of the band plan kernel issue the loads of their views starting at view V / 2 instead of view 0
 *      (registers, reduction order and bits unchanged; default 0),
 * 23 = the last 8-bit level of the key-only Lovasz forward (ptb_lovasz_fwd_keys) evaluates the loss from every key's final rank and the
 *      foreground count in front of it -- both from the scanned histograms -- instead of scattering the keys a fourth time (0|1, default 1),
 * 25 = the prefetching instances of the band plan kernel (one 1024-thread workgroup per CU) alternate between two sets of LDS tiles for
 *      the transposing views: one barrier per covering tile instead of two (0|1, default 1),
 * 27 = band launches of the identity view (the plain loop without TTA) run one workgroup per work item over ALL channels: the window and
 *      the normaliser are loaded once per pixel instead of once per channel, every covering tile of a channel is requested at once (0|1,
 *      default 1),
 * 28 = fp16 / bf16 d4 launches of a band plan take the PAIRS of each launch group (ptb_band_plan_pairs) as 64 x 128 blocks, whose transposing
 *      views are read in 256-byte rows like the row-preserving ones (0|1, default 1; 0: one 64 x 64 item per workgroup as for every other source).
 * Every setting computes the same values (key 19: bit for bit for segments of up to 2^24 elements -- above that the separate dot kernel's
 * (float)(i + 1) positions round and the two settings may differ in the last bits, the default being the reference's telescoping
 * difference); the keys exist for same-box A/B runs and for tests that compare two code paths bit for bit. */
int ptb_set_tunable(int key, int value);

/* ---- TileMerger.integrate_batch / accumulate_single (inference/tiles.py:310-339) -------------------------------
 * for b in 0..B-1 (in order):  image[:, y:y+th, x:x+tw] += tiles[b] * weight ;  norm[0, y:y+th, x:x+tw] += weight
 * image [C,H,W], norm [H,W], weight [th,tw], tiles [B,C,th,tw]; xs/ys HOST int64[B] (top-left corner of each tile).
 * Overlapping tiles of one batch are handled race-free and in batch order: bit-identical to the sequential loop.
 * First-touch stores (optional): `fresh` is a HOST bitmap owned by the caller, one byte per accumulator block of
 * 64 columns x fresh_rows rows (row-major, ceil(H/fresh_rows) x ceil(W/64)); 1 = the block was never written since the
 * accumulators were (logically) zeroed.  Cells made only of fresh blocks are written with plain stores -- the
 * accumulators then never need a memset and are not read on first touch -- and the library clears the bits it wrote.
 * NULL = plain read-modify-write everywhere.  PTB_EFRESH: see above.
 * norm may be NULL: the normaliser depends only on the crop list and the window, never on the predictions, so a caller
 * can keep the crop list and materialise it later (ptb_norm_accumulate) -- or reuse the one of the previous image. */
int ptb_tile_accumulate(float* image, float* norm, const float* weight, const float* tiles, const int64_t* xs,
                        const int64_t* ys, int B, int C, int th, int tw, int H, int W, uint8_t* fresh, int fresh_rows,
                        ptb_stream_t stream);

/* Planned accumulation (no reference counterpart; the result must equal integrate_batch(...) followed by merge()): the
 * caller knows the complete crop list of the image up front.  `remaining` / `done` are HOST byte maps on the block grid of
 * the first-touch bitmap (64 columns x fresh_rows rows): remaining[b] = planned tiles that have not yet touched block b
 * (initialised by the caller from the crop list), done[b] = the merged value of b has been written.  The call works like
 * ptb_deaug_accumulate (V = 1, views = {PTB_VIEW_IDENT}, PTB_RED_SUM for plain tiles) except that cells whose blocks
 * receive their last planned tile in this launch are written as (sum / norm_full) into `merged` [C,H,W] instead of into
 * `image` -- the separate merge pass disappears for them -- and no norm is accumulated (norm_full [H,W] = the complete,
 * data-independent normaliser in integration order).  The library updates both maps.  One launch group per call:
 * PTB_EUNSUPPORTED (nothing launched) if the batch needs several groups, is not block aligned, or does not fit the plan;
 * PTB_EFRESH as above.  Blocks with done == 0 at the end are merged by ptb_merge_div_masked. */
int ptb_accumulate_planned(float* image, const float* norm_full, float* merged, const float* weight, const void* in, int in_dtype,
                           int V, const int* views, int reduction, const int64_t* xs, const int64_t* ys, int B, int C, int th, int tw,
                           int H, int W, uint8_t* fresh, int fresh_rows, uint8_t* remaining, uint8_t* done, ptb_stream_t stream);
/* ptb_accumulate_planned2 = ptb_accumulate_planned + flags.  PTB_PLANNED_KEEP_SUMS (bit 0): a finalised block also stores its weighted
 * sum in `image` -- the accumulator stays complete and exact whenever it is read (TileMerger.image of a merger that planned itself). */
#define PTB_PLANNED_KEEP_SUMS 1
int ptb_accumulate_planned2(float* image, const float* norm_full, float* merged, const float* weight, const void* in, int in_dtype,
                           int V, const int* views, int reduction, const int64_t* xs, const int64_t* ys, int B, int C, int th, int tw,
                           int H, int W, uint8_t* fresh, int fresh_rows, uint8_t* remaining, uint8_t* done, int flags, ptb_stream_t stream);
/* out[c] = image[c] / norm on the blocks (64 columns x rows rows, row-major grid) whose byte in the DEVICE map `mask` is
 * non-zero; other blocks of `out` are left untouched. */
int ptb_merge_div_masked(const float* image, const float* norm, float* out, int C, int H, int W, const uint8_t* mask, int rows,
                         ptb_stream_t stream);

/* norm[0, y:y+th, x:x+tw] += weight for b in 0..B-1, in order (the norm_mask half of integrate_batch: same race-free cell
 * ownership, same summation order, same optional first-touch bitmap -- a SEPARATE bitmap from the image's). */
int ptb_norm_accumulate(float* norm, const float* weight, const int64_t* xs, const int64_t* ys, int B, int th, int tw, int H,
                        int W, uint8_t* fresh, int fresh_rows, ptb_stream_t stream);

/* Test hook, host only (no device work): the launch plan of the two calls above for one batch.  out: up to `cap`
 * records of 12 ints {launch group, ox, oy, w, h, fresh, chunk_end, ntiles, tile[4] (batch indices, -1 padded)}.
 * Returns the number of cells or a PTB_E* code. */
int ptb_debug_plan(const int64_t* xs, const int64_t* ys, int B, int th, int tw, int H, int W, int chunk_rows,
                   uint8_t* fresh, int fresh_rows, int* out, int cap);

/* ---- TileMerger.merge / merge_ (inference/tiles.py:345-350): out[c] = image[c] / norm (no eps clamp) -----------
 * out may alias image (merge_). */
int ptb_merge_div(const float* image, const float* norm, float* out, int C, int64_t HW, ptb_stream_t stream);
/* Band variant used by the multi-GPU merger (no reference counterpart; must equal the single-device merge):
 * out[c][p] = (image[c][p] + (p < extra_n ? extra[c][p] : 0)) / norm[p] for p in [0,HW), with explicit channel strides
 * (elements) so a row band of a larger accumulator can be merged; extra = the halo strip received from the
 * neighbouring rank (may be NULL with extra_n = 0). */
int ptb_merge_div_ex(const float* image, const float* norm, float* out, int C, int64_t HW, int64_t image_cs, int64_t out_cs,
                     const float* extra, int64_t extra_cs, int64_t extra_n, ptb_stream_t stream);

/* Deferred merge of one horizontal band (rows y0:y1 of the accumulator-sized map, lying between two consecutive tile edges) from
 * ALL the tiles that cover it: == the rows y0:y1 of `merge()` after `integrate_batch(<group>_image_deaugment(batch), crops)` of
 * those n tiles in the given order (inference/tiles.py:321-346 after inference/tta.py:442-467), without an accumulator in
 * HBM.  tile_src HOST array of n DEVICE pointers (view 0 of tile t, [C, th, tw] of in_dtype; view v lies tile_view_stride[t]
 * elements further -- the tiles may belong to different batch tensors), xs / ys HOST tile origins; every tile must cover
 * all rows of the band.  norm_full [H, W] = the complete normaliser, merged [C, H, W].  Returns PTB_EUNSUPPORTED when the
 * band does not fit the fast kernel (alignment, more than 48 tiles, more than 4 tiles over one pixel): the caller then
 * integrates those tiles through the incremental entry points. */
int ptb_merge_band(float* merged, const float* norm_full, const float* weight, const void* const* tile_src,
                   const int64_t* tile_view_stride, int in_dtype, int V, const int* views, int reduction, const int64_t* xs,
                   const int64_t* ys, int n, int C, int th, int tw, int H, int W, int y0, int y1, ptb_stream_t stream);

/* Diagnostic (no reference counterpart): streams `bytes` of device memory through a read-only kernel (16 B per lane, eight
 * non-temporal loads in flight, 8192 workgroups) so that a benchmark can time what this GPU's memory system gives a pure
 * read stream and quote its kernels against that as well as against the 8 TB/s spec.  `sink` = 4 writable device bytes. */
int ptb_read_probe(const void* buf, int64_t bytes, float* sink, ptb_stream_t stream);

/* The same read-only stream over `n` (<= 64) buffers in ONE launch (pointer table in the kernel arguments, a persistent grid of
 * `workgroups` (0: 8192) workgroups walking 32 KiB chunks of the concatenation), so that a pass over the per-batch model outputs
 * of an image pays ramp-up and tail once, like the band kernel it is compared with.  Returns the bytes the launch reads (whole
 * 32 KiB chunks of every buffer) or a negative error code. */
int64_t ptb_read_probe_multi(const void* const* bufs, const int64_t* bytes, int n, float* sink, int workgroups, ptb_stream_t stream);

/* out[i] = sum_s slot_sums[s][i] for the [nslots][n] slotted fp64 sums the loss entry points produce (they zero the slots and
 * the label flag themselves, on the launch stream: callers hand in uninitialised workspaces).  When error_flag (may be NULL) was
 * raised by the forward kernel -- a label outside [0, C) that is not ignore_index, where the reference's F.one_hot raises -- every
 * sum becomes NaN, so the condition can never produce a finite loss, even before the asynchronous host check reports it. */
int ptb_sums_finalize(const double* slot_sums, int nslots, int n, double* out, const int* error_flag, ptb_stream_t stream);

/* ---- Deferred merge of a whole image, planned once (TileMerger(crops=tiler.crops, defer=True)).
 * Replaces the reference's per-batch loop `merger.integrate_batch(<group>_image_deaugment(pred), crops)` + `merger.merge()`
 * (inference/tta.py:442-467, inference/tiles.py:321-346) when the crop list of the image is known up front.
 *
 * ptb_band_plan_create: HOST-side planning from the n tile origins (xs, ys; every tile th x tw, in integration order) of an
 *   H x W merged map with C channels.  The rows between consecutive tile edges are bands; consecutive bands are grouped into
 *   launches of about rows_per_launch rows (at most 224 covering tiles each).  Bands lying completely inside rows
 *   [final_lo, final_hi) are normalised (sum / norm); all others write the UN-normalised weighted sum (multi-GPU merger: rows
 *   whose sums are completed by, or belong to, a neighbouring rank; a single-GPU merger passes 0, H).  cuts [ncuts] (may be
 *   NULL / 0): additional row positions (multiples of 4) that are band edges and launch-group boundaries, so that a caller can
 *   have rows it must hand over early finished by their own launch.  Returns the size in bytes of the device table the plan needs
 *   (>= 0; *out receives the plan), PTB_EUNSUPPORTED when the geometry is off the 4-pixel grid / more than 4 tiles cover a pixel.
 * ptb_band_plan_upload: copies the work-item table into caller-provided device memory (64-byte aligned, the size create
 *   returned; the library never allocates device memory).  Once per plan.
 * ptb_band_plan_info: number of launch groups / bands / work items; last_group_of_tile [n] = the last group that reads tile t
 *   (the caller may release a batch once that group was launched); group_rows [3 * groups] = y0, y1 and the last tile (the
 *   one whose arrival completes it; -1: no tile covers those rows) of every group.
 * ptb_band_plan_submit: takes the B tiles pos .. pos+B-1 of the plan -- `batch` = view 0 of the first tile, tile b at
 *   b * tile_stride elements, view v of a tile view_stride elements further (chunk-major [V*B, C, th, tw] model output:
 *   tile_stride = C*th*tw, view_stride = B*C*th*tw) -- and launches every group whose last tile is now in: the group's rows of
 *   merged [C, H, W] = sum_t w * reduce_v(view_v^-1(tile_t)) / norm_full (integration order per pixel, fp32, no contraction:
 *   bit-identical to the incremental entry points).  The launches of ptb_band_plan_submit / _submit_next / _submit_act do not READ
 *   norm_full: they sum the window values of a pixel's covering tiles in integration order beside the blend, which is how
 *   ptb_norm_accumulate builds that map (same bits; a pixel no tile covers is 0 / 0).  The argument stays part of the call and of the
 *   image's configuration (non-NULL, 16-byte aligned, the same for every batch of an image); ptb_band_plan_submit_rank still reads it.  The batches must stay alive and unmodified until their last group was
 *   launched.  Returns the number of launches (>= 0); PTB_EUNSUPPORTED when `pos` is not the next planned tile or the
 *   configuration (dtype, views, reduction, merged / norm_full / weight pointers) differs from the image's first batch -- nothing
 *   is launched then and the caller integrates incrementally.
 * ptb_band_plan_reset: next image.  ptb_band_plan_state: tiles taken / launches issued for the current image. */
typedef struct ptb_band_plan ptb_band_plan;
int64_t ptb_band_plan_create(const int64_t* xs, const int64_t* ys, int n, int C, int th, int tw, int H, int W, int rows_per_launch,
                             int final_lo, int final_hi, const int64_t* cuts, int ncuts, ptb_band_plan** out);
int ptb_band_plan_upload(ptb_band_plan* plan, void* dev_table, ptb_stream_t stream);
int ptb_band_plan_info(const ptb_band_plan* plan, int* n_groups, int* n_bands, int64_t* n_items, int64_t* last_group_of_tile,
                       int64_t* group_rows);
/* ptb_band_plan_pairs (host only): how launch group `group` of the table is laid out -- first *pair_cnt pairs of vertically adjacent full
 * 64 x 64 items under the same covering tiles (top item, then the one 64 rows below it), then *single_cnt items without a partner;
 * 2 * pair_cnt + single_cnt items in all.  Plans with 32-row items, non-square tiles or items off the 8-pixel grid of their tiles have no pairs. */
int ptb_band_plan_pairs(const ptb_band_plan* plan, int group, int* pair_cnt, int* single_cnt);
int ptb_band_plan_reset(ptb_band_plan* plan);
int ptb_band_plan_state(const ptb_band_plan* plan, int* pos, int* launched);
int ptb_band_plan_submit(ptb_band_plan* plan, int pos, int B, const void* batch, int64_t tile_stride, int64_t view_stride, int in_dtype,
                         int V, const int* views, int reduction, float* merged, const float* norm_full, const float* weight,
                         ptb_stream_t stream);
/* ptb_band_plan_submit_next: the next B planned tiles of an image whose configuration the image's first ptb_band_plan_submit has set
 * (same dtype / views / reduction / merged / norm / weight), `batch` = a contiguous [V * B, C, th, tw] model output -- one integrate_batch
 * of the reference's loop (inference/tiles.py:321-339) as a four-argument host call.  The plan keeps the byte ranges of the batches a later
 * launch group still reads: a batch overlapping one of them is refused with PTB_EHELD before anything is recorded.  Returns the launches
 * issued (>= 0); PTB_EUNSUPPORTED without a configuration or past the plan's last tile; else ptb_band_plan_submit's codes. */
int ptb_band_plan_submit_next(ptb_band_plan* plan, const void* batch, int B, ptb_stream_t stream);
void ptb_band_plan_destroy(ptb_band_plan* plan);

/* Multi-GPU (no reference counterpart; the single-device result of inference/tiles.py:321-346 is the specification).
 * ptb_band_plan_create2 = ptb_band_plan_create + `early`: n_early row ranges [lo, hi) of the plan's rows (ends among the cuts) that a
 * neighbouring rank waits for.  With them launch groups are formed by class: the bands of every early range in one launch of their own
 * (issued as soon as the tiles feeding that range are in), the others in groups of ~rows_per_launch rows that do not break at the cuts.
 * ptb_band_plan_rows_launched: 1 when every group writing rows r0 .. r1-1 has been issued for the current image, else 0.
 * ptb_halo_pack: strided rectangle -> contiguous send buffer, dst[c][r][x] = src[c * chan_stride + r * row_stride + x].
 * ptb_band_plan_submit_rank: ptb_band_plan_submit, then packs every outgoing rectangle (rects: n_sends x {r0, r1, c0, c1}, the plan's
 * rows) whose rows are complete into send_bufs[k] (`packed` [n_sends] in/out, zero at the start of an image) and, when the last one
 * has just been packed, records ready_event (a hipEvent_t; NULL only when n_sends == 0: a communication stream that did not wait
 * for it would send rectangles the pack kernels have not written yet -> PTB_EINVAL) on the stream.  Returns the band launches issued (>= 0).
 * Its launches divide the rows inside [final_lo, final_hi) by norm_full as handed in (a rank may issue its tiles in another order than the
 * image's, in which its map was summed); an image is taken through ptb_band_plan_submit or through this call, not both.
 * ptb_band_plan_finish_rank: the end of a rank's image -- adds the n_recvs received rectangles of partial sums ({r0, r1, c0, c1} in
 * the plan's rows, packed [C][rows][cols] buffers) to `merged` and divides the n_ranges row ranges {r0, r1} that held partial sums by
 * `norm` [H][W] in place (launches only). */
/* The exchange itself over RCCL, bound at run time (dlopen of the process's librccl: no link-time dependency).
 * ptb_rccl_available: 1 when an RCCL library could be bound.  ptb_rccl_unique_id: 128 bytes produced on ONE rank and handed to the
 * others by the job's own channel.  ptb_rccl_comm_init: collective over the nranks processes (HIP current device = the rank's GPU).
 * ptb_halo_exchange: all outgoing (ptb_halo_pack'ed) and incoming rectangles of this rank -- contiguous fp32 buffers, element counts,
 * peer ranks -- as ONE ncclGroup of ncclSend / ncclRecv on `stream` (every pair concurrently, each on its own xGMI link; stream-ordered,
 * returns at once).  PTB_EUNSUPPORTED: no RCCL library; PTB_ELAUNCH: RCCL reported an error (text in ptb_last_hip_error()). */
int ptb_rccl_available(void);
int ptb_rccl_unique_id(void* id128);
int ptb_rccl_comm_init(const void* id128, int nranks, int rank, void** comm);
int ptb_rccl_comm_destroy(void* comm);
int ptb_halo_exchange(void* comm, int n_sends, const float* const* send_bufs, const int64_t* send_counts, const int* send_peers, int n_recvs,
                      float* const* recv_bufs, const int64_t* recv_counts, const int* recv_peers, ptb_stream_t stream);
int64_t ptb_band_plan_create2(const int64_t* xs, const int64_t* ys, int n, int C, int th, int tw, int H, int W, int rows_per_launch,
                              int final_lo, int final_hi, const int64_t* cuts, int ncuts, const int64_t* early, int n_early,
                              ptb_band_plan** out);
/* ptb_band_plan_create3 = ptb_band_plan_create2 + flags.  PTB_PLAN_CLIP_ROWS (bit 0): the plan's rows [0, H) are a window of the image;
 * tiles may hang over its top / bottom (ys < 0, ys + th > H) and only what lies inside is read and merged -- a rank that owns a range
 * of PIXEL rows and holds every tile touching them merges exactly those rows with no exchange (parallel: partition="pixel_rows"). */
#define PTB_PLAN_CLIP_ROWS 1
int64_t ptb_band_plan_create3(const int64_t* xs, const int64_t* ys, int n, int C, int th, int tw, int H, int W, int rows_per_launch,
                              int final_lo, int final_hi, const int64_t* cuts, int ncuts, const int64_t* early, int n_early, int flags,
                              ptb_band_plan** out);
int ptb_band_plan_rows_launched(const ptb_band_plan* plan, int r0, int r1);
int ptb_halo_pack(const float* src, int64_t chan_stride, int64_t row_stride, int C, int rows, int cols, float* dst, ptb_stream_t stream);
int ptb_band_plan_finish_rank(const ptb_band_plan* plan, float* merged, const float* norm, int n_recvs, const int64_t* rects,
                              const float* const* recv_bufs, int n_ranges, const int64_t* ranges, ptb_stream_t stream);
int ptb_band_plan_submit_rank(ptb_band_plan* plan, int pos, int B, const void* batch, int64_t tile_stride, int64_t view_stride, int in_dtype,
                              int V, const int* views, int reduction, float* merged, const float* norm_full, const float* weight,
                              int n_sends, const int64_t* rects, float* const* send_bufs, int* packed, void* ready_event,
                              int* all_packed, ptb_stream_t stream);

/* dst[c][r][x] += src[c][r][x] for a packed src [C, rows, cols] and a rectangle of a larger fp32 accumulator (element
 * strides dst_cs per channel, dst_rs per row): folds a halo rectangle received from another rank into the band
 * accumulator (multi-GPU merger; no reference counterpart). */
int ptb_rect_add(float* dst, const float* src, int C, int rows, int cols, int64_t dst_cs, int64_t dst_rs, ptb_stream_t stream);

/* ---- Loop edges on the device (compositions of reference functions, no single counterpart) ---------
 * ptb_split_tiles_u8 == ImageSlicer.split (inference/tiles.py:177-204, BORDER_CONSTANT only) -> image_to_tensor
 * (utils/torch_utils.py:204-231, HWC->CHW) -> .float() [-> * scale[c] + bias[c]] [-> *_image_augment, tta.py:385-422]:
 * image DEVICE uint8 [IH, IW, IC] contiguous; xs/ys HOST int64[B] = tile origins in IMAGE coordinates (the slicer's
 * bbox_crops: negative / overhanging parts read pad_value); views HOST int[V] (augment view codes; {PTB_VIEW_IDENT} for
 * none); scale/bias HOST float[IC] or both NULL; out DEVICE fp32 [V*B, IC, th, tw] chunk-major.  IC <= 16, V <= 8. */
int ptb_split_tiles_u8(const uint8_t* image, int IH, int IW, int IC, const int64_t* xs, const int64_t* ys, int B, int th, int tw,
                       int V, const int* views, const float* scale, const float* bias, int pad_value, float* out,
                       ptb_stream_t stream);
/* border codes of ptb_split_tiles: OpenCV's cv2.BORDER_* numbers (TRANSPARENT = 5 and ISOLATED = 16 -> PTB_EUNSUPPORTED) */
#define PTB_BORDER_CONSTANT 0     /* iiiiii|abcdefgh|iiiiiii, i = pad_value */
#define PTB_BORDER_REPLICATE 1    /* aaaaaa|abcdefgh|hhhhhhh */
#define PTB_BORDER_REFLECT 2      /* fedcba|abcdefgh|hgfedcb */
#define PTB_BORDER_WRAP 3         /* cdefgh|abcdefgh|abcdefg */
#define PTB_BORDER_REFLECT_101 4  /* gfedcb|abcdefgh|gfedcba */
/* ptb_split_tiles == ptb_split_tiles_u8 for further element types and borders, with the batch written as out_dtype:
 * ImageSlicer.split(image, border, value) (the border pads the WHOLE image, margins of any width; rows and columns map
 * independently, as np.pad does) -> HWC->CHW -> .float() [-> * scale[c] + bias[c]] [-> *_image_augment] [-> .to(out_dtype),
 * round to nearest even].  image DEVICE [IH, IW, IC] contiguous of in_dtype (PTB_U8, PTB_U16, PTB_I16; float sources ->
 * PTB_EUNSUPPORTED); pad_value = the border value already cast to in_dtype (an integer in its range; read for
 * PTB_BORDER_CONSTANT only); out DEVICE [V*B, IC, th, tw] of out_dtype (PTB_F32, PTB_F16, PTB_BF16), chunk-major.  The other
 * arguments are those of ptb_split_tiles_u8.  IC <= 16, V <= 8. */
int ptb_split_tiles(const void* image, int in_dtype, int IH, int IW, int IC, const int64_t* xs, const int64_t* ys, int B, int th,
                    int tw, int V, const int* views, const float* scale, const float* bias, int border, float pad_value,
                    int out_dtype, void* out, ptb_stream_t stream);
/* ptb_merge_crop == TileMerger.merge (tiles.py:345-346) -> np.moveaxis(.., 0, -1) -> .astype(uint8) | argmax
 * -> ImageSlicer.crop_to_orignal_size (tiles.py:271-280; README.md:225-226): window [top, top+OH) x [left, left+OW) of
 * image[C,H,W] / norm[H,W] (norm == NULL: image is already normalised).  layout 0: out [C, OH, OW], 1: out [OH, OW, C].
 * kind = PTB_CROP_F32, PTB_CROP_U8, PTB_CROP_ARGMAX_U8 or PTB_CROP_ARGMAX_I64 (0..3, defined with ptb_volume_merge_crop below;
 * argmax kinds write [OH, OW]); the fp16 / bf16 kinds 4 and 5 -> PTB_EINVAL.  A window outside the accumulator -> PTB_EBOUNDS. */
int ptb_merge_crop(const float* image, const float* norm, int C, int H, int W, int top, int left, int OH, int OW, int layout,
                   int kind, void* out, ptb_stream_t stream);

/* ---- Ensembler (+ ApplySigmoidTo / ApplySoftmaxTo) (inference/ensembling.py:12-123) ---------------
 * out = reduce_t act(inputs[t]) over T model outputs read in place (the reference stacks them first, :111,:117):
 * inputs HOST array of T DEVICE pointers, each [B, C, HW] contiguous fp32; reduction = PTB_RED_*; activation 0: none,
 * 1: sigmoid(x * temperature) (:65), 2: softmax over C of x * temperature (:41).  Summation in list order.  T <= 16. */
int ptb_ensemble_reduce(const float* const* inputs, int T, int reduction, int activation, float temperature, int B, int C,
                        int64_t HW, float* out, ptb_stream_t stream);

/* ---- VolumeMerger.integrate_batch (inference/tiles_3d.py:195-208) -----------------------------------
 * volume [C, D, H, W], norm [D, H, W], weight [d, h, w], tiles [B, C, d, h, w] DEVICE fp32; zs/ys/xs HOST int64[B] = tile
 * origin (roi start) per axis.  For b = 0..B-1 in order: volume[:, roi] += tiles[b] * weight (product rounded, then
 * added); norm[roi] += weight.  Out-of-range rois -> PTB_EBOUNDS.  merge = ptb_merge_div with HW = D*H*W. */
int ptb_volume_accumulate(float* volume, float* norm, const float* weight, const float* tiles, const int64_t* zs, const int64_t* ys,
                          const int64_t* xs, int B, int C, int d, int h, int w, int D, int H, int W, ptb_stream_t stream);

/* ---- Loop edges of the 3-D tiles on the device (VolumeSlicer.split / VolumeMerger.merge + crop; no single counterpart) ----
 * ptb_volume_split == VolumeSlicer.split (inference/tiles_3d.py: np.pad with constant `value`, a copy per tile) -> channels first
 * ([d, h, w, C] -> [C, d, h, w]; a [D, H, W] volume is C = 1) -> np.stack -> .float() [-> * scale[c] + bias[c], product rounded,
 * then the sum] [-> .to(out_dtype), round to nearest even]: volume DEVICE [D, H, W, C] contiguous of in_dtype (PTB_F32, PTB_F16,
 * PTB_BF16, PTB_U8, PTB_I16, PTB_U16); zs/ys/xs HOST int64[B] = tile origins in VOLUME coordinates (the slicer's bbox_crops:
 * voxels outside the volume read pad_value, which the caller has already cast to in_dtype); scale/bias HOST float[C] or both
 * NULL; out DEVICE [B, C, d, h, w] of out_dtype (PTB_F32, PTB_F16, PTB_BF16).  C <= 16 (PTB_EUNSUPPORTED otherwise). */
int ptb_volume_split(const void* volume, int in_dtype, int D, int H, int W, int C, const int64_t* zs, const int64_t* ys,
                     const int64_t* xs, int B, int d, int h, int w, const float* scale, const float* bias, float pad_value,
                     int out_dtype, void* out, ptb_stream_t stream);
/* output kinds of ptb_volume_merge_crop (0..5) and ptb_merge_crop (0..3) */
#define PTB_CROP_F32 0
#define PTB_CROP_U8 1         /* truncating cast (numpy .astype on x86-64: low byte of the int32 truncation, 0 for NaN / out of int32 range) */
#define PTB_CROP_ARGMAX_U8 2  /* argmax over channels: first maximum, NaN counts as maximum; layout ignored */
#define PTB_CROP_ARGMAX_I64 3
#define PTB_CROP_F16 4        /* round to nearest even of the fp32 quotient */
#define PTB_CROP_BF16 5
/* ptb_volume_merge_crop == VolumeMerger.merge (volume / norm_mask, ptb_merge_div: correctly rounded, no eps clamp)
 * -> [(slice(None), z0:z0+OD, y0:y0+OH, x0:x0+OW)] (VolumeSlicer.orignal_image_roi) -> layout -> .to(dtype) | .argmax(0):
 * volume DEVICE fp32 [C, D, H, W], norm DEVICE fp32 [D, H, W]; layout 0: out [C, OD, OH, OW], 1: out [OD, OH, OW, C];
 * kind = PTB_CROP_*; argmax kinds write [OD, OH, OW].  A window outside the accumulator -> PTB_EBOUNDS. */
int ptb_volume_merge_crop(const float* volume, const float* norm, int C, int D, int H, int W, int z0, int y0, int x0, int OD, int OH,
                          int OW, int layout, int kind, void* out, ptb_stream_t stream);

/* ---- Trilinear resampling of a volume before the 3-D loop (ptb_volume_resample.hip) ----
 * F.interpolate(mode="trilinear", align_corners): per axis the float32 scale is n_in / n_out, or with align_corners
 * (n_in - 1) / (n_out - 1) (0 when n_out == 1); src = max(scale * (dst + 0.5f) - 0.5f, 0) or scale * dst; i0 = min((int)src, n_in - 1),
 * i1 = i0 + (i0 < n_in - 1), lambda = src - i0 -- aten's area_pixel_compute_source_index in float32, the taps of ptb_resize_bilinear.
 * The blend runs x, then y, then z: a * (1 - lambda) + b * lambda each, products and sums rounded separately.
 *
 * ptb_volume_resize_trilinear == .float() -> trilinear resize -> .to(out_dtype) of a channel-last volume: volume DEVICE [D, H, W, C]
 * contiguous of in_dtype (PTB_F32, PTB_F16, PTB_BF16, PTB_U8, PTB_I16, PTB_U16 -- what ptb_volume_split reads); out DEVICE
 * [RD, RH, RW, C] of out_dtype (PTB_F32, PTB_F16, PTB_BF16).  PTB_EUNSUPPORTED: C > 16; a row of more than 2^31 - 1 elements; a call whose
 * source window per 64 x 4 x 4 output brick exceeds 2560 elements (down-sampling by about 4 and more) on a volume of more than 2^32 - 1
 * elements -- those launches index the whole volume with 32-bit offsets. */
int ptb_volume_resize_trilinear(const void* volume, int in_dtype, int D, int H, int W, int C, int RD, int RH, int RW, int align_corners,
                                int out_dtype, void* out, ptb_stream_t stream);

/* ---- Mirror test-time augmentation of 3-D tiles (inference/tta_3d.py; no reference counterpart: the spec is the torch expression
 * cat([x.flip(dims_v)]) / stack([y_v.flip(dims_v)]).reduce(0)) -------------------------------------------------------------------
 * A view is a 3-bit mask: bit 0 flips W, bit 1 flips H, bit 2 flips D (view m of [B, C, D, H, W] = x.flip(dims) with dims holding 2
 * if m & 4, 3 if m & 2, 4 if m & 1).  A flip is its own inverse, so de-augmentation uses the same masks.  masks HOST int[nviews],
 * each 0..7; 1 <= nviews <= 8.  Batches are chunk-major: row v * B + b holds view v of tile b.  dtype = PTB_F32, PTB_F16 or
 * PTB_BF16.  Every argument is validated before anything is launched; one [D, H, W] plane of more than 2^31 - 2^21 voxels
 * -> PTB_EUNSUPPORTED.
 * ptb_volume_mirror: in_is_batch = 1: src [B, C, D, H, W] -> dst [V*B, C, D, H, W], dst[v*B + b] = flip_v(src[b]) (augment);
 * in_is_batch = 0: src [V*B, C, D, H, W] -> dst [V, B, C, D, H, W], dst[v, b] = flip_v(src[v*B + b]) (the un-flipped stack).
 * dst has the type of src (a bit copy). */
int ptb_volume_mirror(const void* src, int dtype, void* dst, int nviews, const int* masks, int in_is_batch, int B, int C, int D, int H,
                      int W, ptb_stream_t stream);
/* ptb_volume_mirror_reduce: src [V*B, C, D, H, W] -> dst [B, C, D, H, W] = reduce_v flip_v(src[v*B + b]), reduction = PTB_RED_*
 * (the operations of ptb_deaug_reduce), summed in fp32 in view order; written in the source type (fp16 / bf16: round to nearest
 * even). */
int ptb_volume_mirror_reduce(const void* src, int dtype, void* dst, int nviews, const int* masks, int reduction, int B, int C, int D,
                             int H, int W, ptb_stream_t stream);
/* ptb_volume_mirror_accumulate == ptb_volume_mirror_reduce followed by ptb_volume_accumulate, bit for bit, in one pass per tile:
 * tiles DEVICE [V*B, C, d, h, w] of in_dtype (read natively); volume / norm / weight / zs / ys / xs as for ptb_volume_accumulate.
 * For b = 0..B-1 in order: t = reduce_v flip_v(tiles[v*B + b]) rounded to in_dtype; volume[:, roi] += t * weight (product rounded,
 * then added); norm[roi] += weight.  Out-of-range rois -> PTB_EBOUNDS. */
int ptb_volume_mirror_accumulate(float* volume, float* norm, const float* weight, const void* tiles, int in_dtype, int nviews,
                                 const int* masks, int reduction, const int64_t* zs, const int64_t* ys, const int64_t* xs, int B, int C,
                                 int d, int h, int w, int D, int H, int W, ptb_stream_t stream);
/* ptb_volume_split_mirror == ptb_volume_split followed by ptb_volume_mirror (in_is_batch = 1) over the whole call: out DEVICE
 * [V*B, C, d, h, w] of out_dtype, row v*B + b = view v of tile b.  ptb_volume_split is this with nviews = 1, masks = {0}. */
int ptb_volume_split_mirror(const void* volume, int in_dtype, int D, int H, int W, int C, const int64_t* zs, const int64_t* ys,
                            const int64_t* xs, int B, int d, int h, int w, const float* scale, const float* bias, float pad_value,
                            int nviews, const int* masks, int out_dtype, void* out, ptb_stream_t stream);

/* ---- Deferred slab merge of VolumeMerger(crops=, defer=True): the 3-D blend without accumulators (ptb_volume_bands.hip) ----------
 * The n tile origins (zs, ys, xs; every tile d x h x w, in integration order) are known up front.  Every axis is cut at all tile
 * starts and ends; inside a CELL (product of three intervals) the list of covering tiles is constant.  Cells with one z-interval form
 * a SLAB; once the last tile over a slab is in, one launch reads every covering tile of its voxels, blends in integration order in
 * registers (acc = acc + t * w from +0, n = n + w) and writes acc / n into the result window with the cast / layout / argmax of
 * ptb_volume_merge_crop -- bit for bit ptb_volume_accumulate (or ptb_volume_mirror_accumulate) over all tiles followed by
 * ptb_volume_merge_crop, with no [C + 1, D, H, W] accumulators in memory.
 * ptb_volume_plan_create: HOST-side planning.  window = {z0, y0, x0, OD, OH, OW} of the padded volume, layout / kind as for
 *   ptb_volume_merge_crop.  Work items = (cell x window) cut into boxes; voxels outside the window are never computed; a cell nobody
 *   covers writes 0 / 0.  Returns the bytes of the device table (>= 0; *out receives the plan), PTB_EBOUNDS for a tile or a window
 *   outside the volume, PTB_EUNSUPPORTED when more than 8 tiles cover a voxel (a step below half the tile) or a tile side exceeds 65535.
 * ptb_volume_plan_items: the work-item table for the host, 16 int64 per item: launch group, z0, z1, y0, y1, x0, x1 (the box, in
 *   padded-volume coordinates, inside the window), number of covering tiles, their 8 indices in integration order (-1 beyond).
 *   rows == NULL: returns the number of items; else fills `rows` (capacity in items) and returns it.
 * ptb_volume_plan_info: launch groups (a slab whose tile list exceeds the 224 a launch carries in its kernel arguments is cut into
 *   several groups) in launch order = ascending completing tile; slabs; items; last_group_of_tile [n] (-1: no item reads the tile);
 *   group_info [4 * n_groups] = z0, z1 of the slab, completing tile, items; peak_held_tiles = the most tiles in custody at once when
 *   tiles arrive one by one (a tile is held until the tile completing its last group is in); vec_ok = 1 when w and every x origin are
 *   multiples of 4 (the 16-byte instances serve it if the pointers are aligned too; otherwise one voxel per lane).  Any output may be NULL.
 * ptb_volume_plan_upload: copies the item table into caller-provided device memory (16-byte aligned, the size create returned);
 *   the library never allocates device memory.
 * ptb_volume_plan_submit: takes the B tiles pos .. pos+B-1 -- `batch` = view 0 of the first, tile b at batch + b * tile_stride
 *   elements, view v of a tile view_stride elements further per view; in_dtype PTB_F32 / F16 / BF16 read natively; nviews = 0: plain
 *   tiles, else the mirror masks / reduction of ptb_volume_mirror_accumulate -- and launches every group that is now complete.
 *   weight DEVICE [d, h, w] fp32; out DEVICE, the result window.  Returns the number of launches (>= 0); PTB_EUNSUPPORTED (nothing
 *   recorded or launched) when `pos` is not the next planned tile, the batch runs past the plan, or dtype / views / reduction /
 *   weight / out differ from the image's first batch.  Arguments are validated before anything touches the device.
 * ptb_volume_plan_reset: next image.  ptb_volume_plan_state: tiles taken / groups launched for the current image. */
typedef struct ptb_volume_plan ptb_volume_plan;
int64_t ptb_volume_plan_create(const int64_t* zs, const int64_t* ys, const int64_t* xs, int n, int C, int d, int h, int w, int D, int H,
                               int W, const int64_t* window, int layout, int kind, ptb_volume_plan** out);
int64_t ptb_volume_plan_items(const ptb_volume_plan* plan, int64_t* rows, int64_t capacity);
int ptb_volume_plan_info(const ptb_volume_plan* plan, int* n_groups, int* n_slabs, int64_t* n_items, int64_t* last_group_of_tile,
                         int64_t* group_info, int* peak_held_tiles, int* vec_ok);
int ptb_volume_plan_upload(ptb_volume_plan* plan, void* dev_table, ptb_stream_t stream);
int ptb_volume_plan_reset(ptb_volume_plan* plan);
int ptb_volume_plan_state(const ptb_volume_plan* plan, int* pos, int* launched);
int ptb_volume_plan_submit(ptb_volume_plan* plan, int pos, int B, const void* batch, int64_t tile_stride, int64_t view_stride,
                           int in_dtype, int nviews, const int* masks, int reduction, const float* weight, void* out,
                           ptb_stream_t stream);
void ptb_volume_plan_destroy(ptb_volume_plan* plan);

/* ---- Activations inside the 3-D mirror de-augmentation and tile merges (ptb_volume_activation.hip) --------------------------------
 * A(y) = sigmoid(y * temperature) | softmax over the channels of (y * temperature), evaluated in fp32 on the widened logits of every
 * view of every tile, in registers (ApplySigmoidTo / ApplySoftmaxTo of the reference).  Each entry point takes the arguments of its
 * namesake plus `activation` (PTB_ACT_*) and a finite `temperature`, and means the namesake on the float32 tensor A(y): z = x * t
 * rounded; sigmoid 1 / (1 + exp(-z)); softmax exp(z - max_c z) summed in channel order, times the reciprocal of the sum; then
 * red_pre, the view sum in view order, red_post, tile * weight in integration order.  The reduced value is NOT rounded to a half
 * source type (the source counts as fp32), PTB_ACT_NONE included.  PTB_SRC_CHANNELS_LAST keeps its meaning.  A bad activation code or a
 * non-finite temperature -> PTB_EINVAL; PTB_ACT_SOFTMAX with C > 16 -> PTB_EUNSUPPORTED; both before anything touches the device.
 * ptb_volume_mirror_reduce_act writes dense fp32 [B, C, D, H, W].  ptb_volume_plan_submit_act: activation and temperature belong to
 * the image's configuration, as does the entry point itself (a change -> PTB_EUNSUPPORTED, nothing recorded or launched). */
#define PTB_ACT_NONE 0
#define PTB_ACT_SIGMOID 1
#define PTB_ACT_SOFTMAX 2
int ptb_volume_mirror_reduce_act(const void* src, int dtype, float* dst, int nviews, const int* masks, int reduction, int B, int C, int D,
                                 int H, int W, int activation, float temperature, ptb_stream_t stream);
int ptb_volume_mirror_accumulate_act(float* volume, float* norm, const float* weight, const void* tiles, int in_dtype, int nviews,
                                     const int* masks, int reduction, const int64_t* zs, const int64_t* ys, const int64_t* xs, int B, int C,
                                     int d, int h, int w, int D, int H, int W, int activation, float temperature, ptb_stream_t stream);
int ptb_volume_plan_submit_act(ptb_volume_plan* plan, int pos, int B, const void* batch, int64_t tile_stride, int64_t view_stride,
                               int in_dtype, int nviews, const int* masks, int reduction, const float* weight, void* out, int activation,
                               float temperature, ptb_stream_t stream);

/* ---- {fliplr,flipud,flips,d2,d4}_image_deaugment (inference/tta.py:287-316,344-365,442-467,503-524) -------------
 * in [V*B, C, H, W] (chunk-major: rows [k*B,(k+1)*B) are view k), views HOST int[V] = inverse transform of each chunk.
 * out [B, C, H, W] = reduce_k view_k(in[k*B + b]).  V <= 8.  Transposing views require H == W. */
int ptb_deaug_reduce(const float* in, float* out, int V, const int* views, int reduction, int B, int C, int H, int W,
                     ptb_stream_t stream);

/* Backward of ptb_deaug_reduce for the NON-linear reductions (the TTA functions "respect gradients flow",
 * inference/tta.py:3-4); `in` / `out` are the forward input / output, `views` the forward views.  The linear reductions
 * (sum, mean) are differentiated with ptb_view_transform. */
int ptb_deaug_reduce_bwd(const float* in, const float* out, const float* grad_out, float* grad_in, int V, const int* views,
                         int reduction, int B, int C, int H, int W, ptb_stream_t stream);

/* Half-precision sources: the same as ptb_deaug_reduce / ptb_deaug_accumulate (and ptb_tile_accumulate with V = 1,
 * views = {PTB_VIEW_IDENT}, PTB_RED_SUM) with `in` holding in_dtype elements -- what the reference does with
 * `batch.type_as(self.image)` (inference/tiles.py:334-335) / its dtype-agnostic TTA ops, minus the fp32 copy: fp16 / bf16
 * values are widened in registers (exact), so the result equals the fp32 entry point on in.float() bit for bit.
 * PTB_EUNSUPPORTED (nothing launched) when the shape needs the scalar kernels or a non-default chunk size. */
int ptb_deaug_reduce_t(const void* in, int in_dtype, float* out, int V, const int* views, int reduction, int B, int C, int H,
                       int W, ptb_stream_t stream);
int ptb_deaug_accumulate_t(float* image, float* norm, const float* weight, const void* in, int in_dtype, int V, const int* views,
                           int reduction, const int64_t* xs, const int64_t* ys, int B, int C, int th, int tw, int H, int W,
                           uint8_t* fresh, int fresh_rows, ptb_stream_t stream);

/* ---- Activations inside the 2-D de-augmentation and tile merges (ptb_tile_activation.hip) -------------------------------------------
 * The 2-D twins of the 3-D block above ("Activations inside the 3-D ..."), with its semantics: each entry point takes the arguments of
 * its namesake (ptb_deaug_reduce_t, ptb_deaug_accumulate_t with its first-touch bitmap, ptb_band_plan_submit) plus `activation`
 * (PTB_ACT_*) and a finite `temperature`, and means the namesake on the float32 tensor A(y) = sigmoid(y * temperature) | softmax over
 * the channels of (y * temperature), evaluated per view and pixel in registers on the widened logits: z = x * t rounded; sigmoid
 * 1 / (1 + exp(-z)); softmax exp(z - max_c z) summed in channel order, times the reciprocal of the sum; then red_pre, the view sum in
 * view order, red_post, tile * weight in integration order.  The reduced value is NOT rounded to a half source type (the source
 * counts as fp32; PTB_ROUND_SRC is ignored), PTB_ACT_NONE included; ptb_deaug_reduce_act writes dense fp32 [B, C, H, W].
 * PTB_SRC_CHANNELS_LAST keeps its meaning.  Before anything touches the device: a bad activation code or a non-finite temperature ->
 * PTB_EINVAL; PTB_ACT_SOFTMAX with C > 16 -> PTB_EUNSUPPORTED; a planar source whose shape the vector kernels do not take (tiles off
 * the 4-pixel grid or unaligned: the scalar-kernel shapes of the namesakes) -> PTB_EUNSUPPORTED -- the caller applies A itself and
 * calls the namesake.  A planar source of any dtype is served at every chunk size.  ptb_band_plan_submit_act: the entry point,
 * activation and temperature belong to the image's configuration (a change -> PTB_EUNSUPPORTED, nothing recorded or launched);
 * ptb_band_plan_submit_next declines such an image (PTB_EUNSUPPORTED): every batch of it takes this call. */
int ptb_deaug_reduce_act(const void* in, int in_dtype, float* out, int V, const int* views, int reduction, int B, int C, int H, int W,
                         int activation, float temperature, ptb_stream_t stream);
int ptb_deaug_accumulate_act(float* image, float* norm, const float* weight, const void* in, int in_dtype, int V, const int* views,
                             int reduction, const int64_t* xs, const int64_t* ys, int B, int C, int th, int tw, int H, int W,
                             uint8_t* fresh, int fresh_rows, int activation, float temperature, ptb_stream_t stream);
int ptb_band_plan_submit_act(ptb_band_plan* plan, int pos, int B, const void* batch, int64_t tile_stride, int64_t view_stride,
                             int in_dtype, int V, const int* views, int reduction, float* merged, const float* norm_full,
                             const float* weight, int activation, float temperature, ptb_stream_t stream);

/* ---- reductions over a stack of ANY length, explicit eps (inference/functional.py:247-331; tta.py:63-95) ----------
 * out[i] = post(mean_t pre(src[t, i])) for src [T, n] contiguous fp32: geometric_mean, harmonic_mean(eps), harmonic1p_mean,
 * logodd_mean(eps), log1p_mean, mean, sum along dim 0.  The fused view kernels above take at most 8 planes and the default
 * eps = 1e-6; this entry is `_deaugment_averaging` for tencrop TTA (T = 10), ensembles of more than 8 predictions, and the
 * reductions called with their eps argument.  eps is the Python double: the kernel clamps at (float)eps / (float)(1 - eps).
 * The backward takes the forward output: grad[t, i] = grad_out[i] * post'(out[i]) * pre'(src[t, i]) / T. */
int ptb_stack_reduce(const float* src, int T, int64_t n, int reduction, double eps, float* out, ptb_stream_t stream);
int ptb_stack_reduce_bwd(const float* src, const float* out, const float* grad_out, int T, int64_t n, int reduction, double eps,
                         float* grad, ptb_stream_t stream);

/* ---- per-view transform without reduction ----------------------------------------------------------------------
 * out[k*B + b] = scale * view_k(in[src]) with src = b (in_is_batch = 1: *_image_augment, inference/tta.py:257-284,
 * 319-341,385-422,470-484; in [B,C,H,W]) or src = k*B + b (in_is_batch = 0: de-augment with reduction=None).
 * out [V*B, C, Ho, Wo] where (Ho,Wo) = (W,H) for transposing views (so H == W is required for them). */
int ptb_view_transform(const float* in, float* out, int V, const int* views, int in_is_batch, float scale, int B, int C,
                       int H, int W, ptb_stream_t stream);

/* The same views as pure data movement for elements of ANY type: torch_fliplr ... torch_rot180_transpose, *_image_augment and
 * *_image_deaugment(reduction=None) on integer / boolean / float64 / half tensors and on tensors of more than four dims
 * (inference/functional.py:47-132: x.flip(3), x.flip(2), x.rot90(k, dims=(2, 3)), x.transpose(2, 3) -- index permutations of dims 2
 * and 3 whatever the dtype, dims beyond the fourth ride along with their pixel).  in [planes or V*planes, H, W, run] elements of
 * elem_bytes (1 | 2 | 4 | 8 | 16) bytes, planes = B * C, run = product of the dims beyond the fourth (1 for 4-D tensors);
 * out [V*planes, Ho, Wo, run] with (Ho, Wo) = (W, H) for transposing views -- non-square planes are fine when the views of one call
 * agree on the output shape (all transposing or none; PTB_EINVAL otherwise).  Bit-exact by construction. */
int ptb_view_permute(const void* in, void* out, int V, const int* views, int in_is_batch, int64_t planes, int H, int W,
                     int elem_bytes, int64_t run, ptb_stream_t stream);

/* ---- fused: de-augment + reduce + TileMerger.integrate_batch (tta.py:442-467 feeding tiles.py:321-339) ----------
 * image[:, y:y+th, x:x+tw] += reduce_k view_k(in[k*B+b]) * weight ; norm += weight.  The reduced tile never goes
 * to HBM.  Same tensors as ptb_deaug_reduce (H=th, W=tw) and ptb_tile_accumulate (incl. the first-touch bitmap). */
int ptb_deaug_accumulate(float* image, float* norm, const float* weight, const float* in, int V, const int* views,
                         int reduction, const int64_t* xs, const int64_t* ys, int B, int C, int th, int tw, int H,
                         int W, uint8_t* fresh, int fresh_rows, ptb_stream_t stream);

/* ---- bilinear resize of ms_image_augment / ms_image_deaugment (inference/tta.py:599-621, 645-689) ----------------
 * = torch.nn.functional.interpolate(in, size=(hout,wout), mode="bilinear", align_corners=...) on `planes` = B*C maps. */
int ptb_resize_bilinear(const float* in, float* out, int64_t planes, int hin, int win, int hout, int wout,
                        int align_corners, ptb_stream_t stream);

/* ---- fused ms_image_deaugment (inference/tta.py:645-689): out = reduce_s resize(inputs[s] -> (hout,wout)) -----------
 * inputs: HOST array of n (<= 8) device pointers, map s is [planes, hs[s], ws[s]]; maps that already have the output
 * size are taken as they are (the reference skips F.interpolate for offset 0).  The resized maps never go to HBM. */
int ptb_ms_deaug_reduce(const float* const* inputs, const int* hs, const int* ws, int n, float* out, int64_t planes, int hout,
                        int wout, int align_corners, int reduction, ptb_stream_t stream);
/* Row-strip variant (cfg5 over several GPUs, no collective: every rank reduces its own strip of output rows): computes
 * output rows [out_row0, out_row0 + out_rows) of the hout_full x wout result into out [planes, out_rows, wout].  Map s has
 * hs_full[s] rows in total, of which inputs[s] holds src_rows[s] rows starting at global row src_row0[s] ([planes,
 * src_rows[s], ws[s]]); the strip must contain every source row the 4-tap footprints of the output rows touch
 * (pytorch_toolbelt_amd.parallel.ms_strip_plan computes the ranges).  Same arithmetic as the full call. */
int ptb_ms_deaug_reduce_strip(const float* const* inputs, const int* hs_full, const int* ws, const int* src_row0,
                              const int* src_rows, int n, float* out, int64_t planes, int hout_full, int wout, int out_row0,
                              int out_rows, int align_corners, int reduction, ptb_stream_t stream);

/* Adjoints of the resize entry points ("TTA respects gradient flow", inference/tta.py:3-4; the reference gets them from autograd
 * through F.interpolate).  grad_in / grad_inputs[s] must be ZEROED by the caller: the 4 taps of several output pixels land on
 * the same source pixel and are added with fp32 atomics (summation order, hence the last bit, not deterministic -- as in
 * ATen's upsample_bilinear2d_backward).  ptb_ms_deaug_reduce_bwd: gradient of ptb_ms_deaug_reduce w.r.t. every scale's map;
 * fwd_out = the forward result (needed by the non-linear reductions, may be NULL for sum / mean). */
int ptb_resize_bilinear_bwd(const float* grad_out, float* grad_in, int64_t planes, int hin, int win, int hout, int wout,
                            int align_corners, ptb_stream_t stream);
int ptb_ms_deaug_reduce_bwd(const float* const* inputs, const int* hs, const int* ws, int n, const float* fwd_out, const float* grad_out,
                            float* const* grad_inputs, int64_t planes, int hout, int wout, int align_corners, int reduction,
                            ptb_stream_t stream);

/* F.interpolate(x, size, mode="nearest") for [planes, hin, win] -> [planes, hout, wout] (multiscale TTA with mode="nearest",
 * inference/tta.py:599-621, 645-689): out[p, y, x] = in[p, min(floor(y * hin / hout), hin - 1), min(floor(x * win / wout), win - 1)].
 * backward != 0: `in` is grad_out [planes, hout, wout] and `out` the ZEROED grad_in [planes, hin, win] (atomic adds). */
int ptb_resize_nearest(const float* in, float* out, int64_t planes, int hin, int win, int hout, int wout, int backward,
                       ptb_stream_t stream);

/* The two remaining 4-D modes F.interpolate offers (the reference forwards any `mode`, inference/tta.py:599-621, 645-689), same layout
 * and backward convention as ptb_resize_nearest:
 * "nearest-exact": out[p, y, x] = in[p, min(floor((y + 0.5) * hin / hout), hin - 1), min(floor((x + 0.5) * win / wout), win - 1)];
 * "area" (= adaptive_avg_pool2d): out[p, y, x] = mean of in[p, floor(y hin / hout) : ceil((y + 1) hin / hout),
 *                                                           floor(x win / wout) : ceil((x + 1) win / wout)]. */
int ptb_resize_nearest_exact(const float* in, float* out, int64_t planes, int hin, int win, int hout, int wout, int backward,
                             ptb_stream_t stream);
int ptb_resize_area(const float* in, float* out, int64_t planes, int hin, int win, int hout, int wout, int backward, ptb_stream_t stream);

/* F.interpolate(x, size, mode="bicubic", align_corners) for [planes, hin, win] -> [planes, hout, wout] (multiscale TTA with
 * mode="bicubic"): 4 x 4 taps around floor(src) (src without the clamp at 0 of the linear modes), indices clamped into the image,
 * cubic convolution weights with A = -0.75, rows first (aten UpSampleBicubic2d).  backward != 0: `in` is grad_out
 * [planes, hout, wout], `out` the ZEROED grad_in [planes, hin, win] (atomic adds, like aten's backward). */
int ptb_resize_bicubic(const float* in, float* out, int64_t planes, int hin, int win, int hout, int wout, int align_corners, int backward,
                       ptb_stream_t stream);

/* Multiscale + flip TTA in one pass (BASELINE configs[4]; extension): inputs[s] = the model output for the flip-augmented batch
 * of scale s, [V * B, C, hs[s], ws[s]] chunk-major (view v of plane p at (v * planes + p) * hs * ws; planes = B * C),
 *   out = reduction_s( bilinear_s( inner_reduction_v( view_v^-1( inputs[s][v] ) ) ) )
 * == ms_image_deaugment([<group>_image_deaugment(y_s, inner_reduction) for s], ...) (inference/tta.py:287-316, 344-365, 503-524 then
 * :645-689) without the flip-reduced maps ever reaching HBM.  views[V] = the group's INVERSE view codes (row-preserving only:
 * PTB_VIEW_IDENT / FLIPLR / FLIPUD / ROT180).  Returns PTB_EUNSUPPORTED for transposing views, widths not divisible by 4, or a
 * scale ratio above ~1.3 (source window of a 64 x 64 tile larger than 88 x 96): the caller then composes the two entry points. */
int ptb_ms_flip_deaug_reduce(const float* const* inputs, const int* hs, const int* ws, int n, int V, const int* views,
                             int inner_reduction, float* out, int64_t planes, int hout, int wout, int align_corners, int reduction,
                             ptb_stream_t stream);

/* One rank's rows of the same pass (BASELINE configs[4] over several GPUs: output row strips, no collective): inputs[s] holds rows
 * src_row0[s] .. src_row0[s] + src_rows[s] - 1 of every view plane of scale s ([V * planes, src_rows[s], ws[s]]; hs_full[s] is the full
 * height: the taps are those of the full-size call, so the strips of the result concatenate to it bit for bit); out receives rows
 * out_row0 .. out_row0 + out_rows - 1 of the [planes, hout_full, wout] result.  PTB_EBOUNDS when a strip lacks a source row the taps of
 * those output rows read; views that flip rows do not come in strips (PTB_EUNSUPPORTED). */
int ptb_ms_flip_deaug_reduce_strip(const float* const* inputs, const int* hs_full, const int* ws, const int* src_row0, const int* src_rows,
                                   int n, int V, const int* views, int inner_reduction, float* out, int64_t planes, int hout_full, int wout,
                                   int out_row0, int out_rows, int align_corners, int reduction, ptb_stream_t stream);

/* ================================= segmentation losses (pytorch_toolbelt.losses) =================================
 * logits [B, C, HW] fp32; targets are either labels int64 [B, HW] (one-hot is formed on the fly, never materialised)
 * or dense fp32 [B, C, HW]; exactly one of `labels` / `dense` is non-NULL.  Scalars are accumulated in fp64.
 * flags: */
#define PTB_SEG_FOCAL 1            /* accumulate sigmoid focal sums: sums[0] = sum loss, sums[1] = sum focal_term */
#define PTB_SEG_STATS 2            /* accumulate region statistics: sums[2 + k*C + c], k = 0: I=sum p*t, 1: P=sum p, 2: T=sum t */
#define PTB_SEG_HAS_IGNORE 4       /* ignore_label (labels) / ignore_value (dense) is active */
#define PTB_SEG_HAS_ALPHA 8
#define PTB_SEG_REDUCED 16         /* reduced focal loss with `threshold` */
#define PTB_SEG_MASK_FOCAL_TERM 32 /* normalized focal: ignored elements add 0 to sums[1] (functional.py:90-98) */
#define PTB_SEG_ELEMWISE 64        /* also write the unreduced focal loss to elem_out [B, C, HW] */
#define PTB_SEG_NO_TERM 128       /* the caller will not read sums[1] (no normalized=True): kernels may leave it unset */
/* prob (activation used for the region statistics): */
#define PTB_PROB_SOFTMAX 0         /* log_softmax(dim=1).exp()  (dice.py:68-72 multiclass) */
#define PTB_PROB_SIGMOID 1         /* logsigmoid.exp()          (dice.py:73-75 binary / multilabel) */
#define PTB_PROB_IDENTITY 2        /* from_logits=False: `logits` already holds probabilities */

/* Scalars are accumulated into PTB_SUM_SLOTS interleaved copies (same-address atomics serialise on the device); the
 * caller zeroes the whole buffer and adds the slots: total[k] = sum_s sums[s * n + k]. */
#define PTB_SUM_SLOTS 64

/* One pass over logits+targets for focal_loss_with_logits (losses/functional.py:19-107, sigmoid activation),
 * BinaryFocalLoss (losses/focal.py:77-105) and the sums of soft_dice_score / soft_jaccard_score with dims=(0,2)
 * (losses/functional.py:188-247; DiceLoss losses/dice.py:59-131, JaccardLoss losses/jaccard.py:48-103).
 * sums: double[PTB_SUM_SLOTS][2 + 3*C] (zeroed by this call, like error_flag; reduce with ptb_sums_finalize); error_flag: int, set to 1 when a label is outside [0, C)
 * and not ignore_label (the reference's F.one_hot raises).  class_weights [C] fp32 or NULL. */
int ptb_seg_loss_fwd(const float* logits, const int64_t* labels, const float* dense, const float* class_weights,
                     double* sums, float* elem_out, int* error_flag, int B, int C, int64_t HW, int flags, int prob,
                     float gamma, float alpha, float threshold, int64_t ignore_label, float ignore_value,
                     ptb_stream_t stream);

/* Gradient of the sigmoid focal loss w.r.t. logits: grad[i] = coef[0] * (grad_elem ? grad_elem[i] : 1) * dL_i/dx_i
 * + coef[1] * dF_i/dx_i, coef = DEVICE float[2] (reduction / normalisation factors times the upstream gradient). */
int ptb_focal_bwd(const float* logits, const int64_t* labels, const float* dense, const float* class_weights,
                  const float* coef, const float* grad_elem, float* grad, int B, int C, int64_t HW, int flags,
                  float gamma, float alpha, float threshold, int64_t ignore_label, float ignore_value,
                  ptb_stream_t stream);

/* focal_loss_with_logits(..., activation="softmax", softmax_dim=d) (losses/functional.py:61-107 with :63-64
 * `p = torch.softmax(output, dim=softmax_dim)`): the tensor is passed as the [B, C, HW] view whose C is the softmax dimension.
 * Same flags / sums[0..1] / elem_out / coef / grad_elem contract as ptb_seg_loss_fwd (PTB_SEG_FOCAL) and ptb_focal_bwd, except
 * that `sums` is [PTB_SUM_SLOTS, 2].  class_weights follow dim 1 of the ORIGINAL tensor (functional.py:83-88): cw_mode 0 =
 * none, 1 = indexed by the softmax channel c (cw_n == C), 2 = by (b / cw_div) % cw_n, 3 = by (position / cw_div) % cw_n. */
int ptb_focal_softmax_fwd(const float* logits, const int64_t* labels, const float* dense, const float* class_weights, int cw_mode,
                          int cw_n, int64_t cw_div, double* sums, float* elem_out, int* error_flag, int B, int C, int64_t HW, int flags,
                          float gamma, float alpha, float threshold, int64_t ignore_label, float ignore_value, ptb_stream_t stream);
int ptb_focal_softmax_bwd(const float* logits, const int64_t* labels, const float* dense, const float* class_weights, int cw_mode,
                          int cw_n, int64_t cw_div, const float* coef, const float* grad_elem, float* grad, int B, int C, int64_t HW,
                          int flags, float gamma, float alpha, float threshold, int64_t ignore_label, float ignore_value,
                          ptb_stream_t stream);

/* Gradient of any function of the region statistics w.r.t. logits, given DEVICE arrays gI[C] = dLoss/dI_c and
 * gP[C] = dLoss/dP_c (T does not depend on the logits). */
int ptb_seg_stats_bwd(const float* logits, const int64_t* labels, const float* dense, const float* gI, const float* gP,
                      float* grad, int B, int C, int64_t HW, int flags, int prob, int64_t ignore_label,
                      float ignore_value, ptb_stream_t stream);

/* Both of the above in one pass (backward of a ptb_seg_loss_fwd call with PTB_SEG_FOCAL | PTB_SEG_STATS);
 * PTB_EUNSUPPORTED when the fused kernel does not apply (C > 16, HW % 4 != 0, ...): use the two kernels above. */
int ptb_seg_fused_bwd(const float* logits, const int64_t* labels, const float* dense, const float* class_weights,
                      const float* coef, const float* gI, const float* gP, float* grad, int B, int C, int64_t HW, int flags,
                      int prob, float gamma, float alpha, float threshold, int64_t ignore_label, float ignore_value,
                      ptb_stream_t stream);

/* Scalar tail of DiceLoss (losses/dice.py:112-131), JaccardLoss (losses/jaccard.py:95-113) and their weighted sum with a
 * mean focal loss, together with its derivative, from the slot sums a ptb_seg_loss_fwd call produced:
 *   loss[0] = focal_scale * sum_focal + dice_weight * mean_c dice_loss_c + jaccard_weight * mean_c jaccard_loss_c
 *   score_c = (2 I + smooth) / max(P + T + smooth, eps)  |  (I + smooth) / max(P + T - I + smooth, eps);
 *   loss_c = [T_c > 0] * (log_loss ? -log(max(score_c, eps)) : 1 - score_c); the mean runs over the n_selected classes with
 *   class_mask[c] != 0 (class_mask NULL: all C).  fp32 arithmetic on the fp64 sums rounded to fp32, like the reference.
 * coef DEVICE float[2 + 2C] receives d loss / d (focal loss sum, focal term sum, I[C], P[C]) -- the arrays
 * ptb_focal_bwd / ptb_seg_stats_bwd / ptb_seg_fused_bwd take (after scaling by the upstream gradient).  error_flag (may be NULL): the
 * forward kernel's label flag; when raised the loss is NaN. */
int ptb_region_epilogue(const double* sums, int slots, int C, float focal_scale, float dice_weight, float jaccard_weight,
                        float smooth, float eps, int log_loss, const uint8_t* class_mask, int n_selected, float* loss,
                        float* coef, const int* error_flag, ptb_stream_t stream);

/* The two above in ONE launch (no reference counterpart: losses/dice.py:66-131 and losses/jaccard.py:62-113 are ~40 torch ops): the
 * streaming statistics kernel of ptb_seg_loss_fwd, whose last-arriving workgroup adds up the slot sums, evaluates the scalar tail
 * of ptb_region_epilogue and its derivative, and leaves the workspace zeroed for the next call -- no memset, finalize or epilogue
 * launches.  `workspace`: ptb_region_workspace_bytes(C) bytes of 8-byte aligned DEVICE memory that were ZERO before the first call
 * and are used by one stream at a time; every call leaves them zero.  flags must contain SEG_STATS (2), optionally SEG_FOCAL (1)
 * and the option bits of ptb_seg_loss_fwd (not ELEMWISE).  loss DEVICE float[1], coef DEVICE float[2 + 2C] as for
 * ptb_region_epilogue; error_out (may be NULL): int[1], device OR pinned-host memory, receives the call's label flag (a label
 * outside [0, C) that is not ignore_index also turns the loss into NaN).  Returns PTB_EUNSUPPORTED for an empty input. */
int64_t ptb_region_workspace_bytes(int C);
int ptb_region_loss_fwd(const float* logits, const int64_t* labels, const float* dense, const float* class_weights, void* workspace,
                        int B, int C, int64_t HW, int flags, int prob, float gamma, float alpha, float threshold, int64_t ignore_label,
                        float ignore_value, float focal_scale, float dice_weight, float jaccard_weight, float smooth, float eps,
                        int log_loss, const unsigned char* class_mask, int n_selected, float* loss, float* coef, int* error_out,
                        ptb_stream_t stream);

/* softmax_focal_loss_with_logits / CrossEntropyFocalLoss (losses/functional.py:110-173, losses/focal.py:108-161).
 * sums double[PTB_SUM_SLOTS][2] (zeroed by this call): sum of per-pixel losses, sum of all focal terms; pixel_out [B, HW] optional. */
int ptb_softmax_focal_fwd(const float* logits, const int64_t* labels, const float* class_weights, double* sums,
                          float* pixel_out, int* error_flag, int B, int C, int64_t HW, int reduced, float gamma,
                          float threshold, int64_t ignore_label, ptb_stream_t stream);
int ptb_softmax_focal_bwd(const float* logits, const int64_t* labels, const float* class_weights, const float* coef,
                          const float* grad_pix, float* grad, int B, int C, int64_t HW, int reduced, float gamma,
                          float threshold, int64_t ignore_label, ptb_stream_t stream);

/* ---- Remaining elementwise + reduce losses -------------------------------------------------------
 * kind: 0 SoftBCEWithLogitsLoss (losses/soft_bce.py:29-46; p0 = smooth factor when flags & 2, chan_w / chan_pw = DEVICE
 * per-channel weight / pos_weight [C] or NULL with element channel = (i / HW) % C), 1 balanced BCE (losses/
 * balanced_bce.py:27-40), 2 QualityFocalLoss (losses/quality_focal_loss.py:33-35; p0 = beta), 3 wing_loss (losses/
 * functional.py:260-269; p0 = width, p1 = curvature, p2 = width - width*log(1 + width/curvature)), 4 log_cosh_loss
 * (losses/functional.py:338-341), 5 soft F1 counts of one class (losses/soft_f1.py:22-24, 63-78: p = clamp(sigmoid(x), p0,
 * 1 - p0), or p = x when flags & 2).  flags: 1 = elements whose target == ignore_value contribute 0; 2 = label smoothing.
 * x, t: DEVICE fp32 [n].  sums: DEVICE double [PTB_SUM_SLOTS][4], zeroed by this call, slot-wise partial sums of
 *   kind 0,3,4: {loss};  kind 1: {sum t*logsigmoid(x), sum (1-t)*logsigmoid(-x), #(t == 1), #(t == 0)};  kind 2: {loss, focal};
 *   kind 5: {sum p t, sum p, sum t, #kept} (TP = s0, FP = s1 - s0, FN = s2 - s0); its apply gives d(coef[0] s0 + coef[1] s1)/dx.
 * elem_out (optional, not for kind 1): per-element loss. */
int ptb_pointwise_loss_fwd(int kind, const float* x, const float* t, const float* chan_w, const float* chan_pw, double* sums,
                           float* elem_out, int64_t n, int C, int64_t HW, int flags, float p0, float p1, float p2,
                           float ignore_value, ptb_stream_t stream);
/* out[i] = coef[0] * (grad_elem ? grad_elem[i] : 1) * dloss_i/dx_i (+ coef[1] * dfocal_i/dx_i for kind 2); kind 1: coef =
 * {pos class weight, neg class weight} (each already multiplied by the upstream gradient); emit_loss = 1 (kind 1 only)
 * writes the per-element loss -(coef[0]*t*logsigmoid(x) + coef[1]*(1-t)*logsigmoid(-x)) instead.  coef: DEVICE float[2]. */
int ptb_pointwise_loss_apply(int kind, int emit_loss, const float* x, const float* t, const float* chan_w, const float* chan_pw,
                             const float* coef, const float* grad_elem, float* out, int64_t n, int C, int64_t HW, int flags,
                             float p0, float p1, float p2, float ignore_value, ptb_stream_t stream);
/* SoftCrossEntropyLoss = label_smoothed_nll_loss(log_softmax(x, 1)) (losses/soft_ce.py:24-33, losses/functional.py:280-323):
 * logits [B, C, HW], labels int64 [B, HW]; sums double [PTB_SUM_SLOTS][4]: {sum nll, sum smooth} over non-ignored pixels;
 * pixel_out (optional) [B, HW] = (1-eps)*nll + eps/C*smooth; error_flag set to 1 on a label outside [0, C) that is not ignored.
 * bwd: grad[b,c,i] = coef[0] * (grad_pix ? grad_pix[b,i] : 1) * d pixel_loss / d x[b,c,i]; coef DEVICE float[1]. */
int ptb_soft_ce_fwd(const float* logits, const int64_t* labels, double* sums, float* pixel_out, int* error_flag, int B, int C,
                    int64_t HW, float eps, int has_ignore, int64_t ignore_label, ptb_stream_t stream);
int ptb_soft_ce_bwd(const float* logits, const int64_t* labels, const float* coef, const float* grad_pix, float* grad, int B, int C,
                    int64_t HW, float eps, int has_ignore, int64_t ignore_label, ptb_stream_t stream);

/* BinaryBiTemperedLogisticLoss (losses/bitempered_loss.py:223-284; bi_tempered_logistic_loss :135-180 with the two
 * activations (-x, x) and targets (1-t, t)): x, t DEVICE fp32 [n]; sums double [PTB_SUM_SLOTS][4] {sum of per-element
 * losses}; elem_out optional; iters = normalisation iterations (the reference uses 5); elements whose target equals
 * ignore_value contribute 0.  bwd: grad[i] = coef[0] * (grad_elem ? grad_elem[i] : 1) * dloss_i/dx_i, coef DEVICE float[1]. */
int ptb_bitempered_binary_fwd(const float* x, const float* t, double* sums, float* elem_out, int64_t n, float t1, float t2,
                              float smoothing, int iters, int has_ignore, float ignore_value, ptb_stream_t stream);
int ptb_bitempered_binary_bwd(const float* x, const float* t, const float* coef, const float* grad_elem, float* grad, int64_t n,
                              float t1, float t2, float smoothing, int iters, int has_ignore, float ignore_value,
                              ptb_stream_t stream);

/* bi_tempered_logistic_loss (losses/bitempered_loss.py:135-180) for activations [R, K] (classes last) with DENSE targets [R, K]
 * (one-hot or soft; label smoothing applied inside): out[r] = the unreduced loss of row r.  One wave per row; the tempered softmax's
 * normalisation runs `iters` iterations (the reference's num_iters = 5): fixed point for t2 > 1, bisection for t2 < 1, log-sum-exp
 * for t2 = 1.  backward != 0: grad_loss [R] in, out = d loss / d activations [R, K] (closed form via the escort distribution,
 * :94-104).  t1 = 2 is rejected (the loss formula divides by 2 - t1). */
int ptb_bitempered_rows(const float* activations, const float* onehot, const float* grad_loss, float* out, int64_t R, int K, float t1,
                        float t2, float smoothing, int iters, int backward, ptb_stream_t stream);

/* ---- Lovasz hinge / Lovasz-softmax (losses/lovasz.py:23-184) ---------------------------------------------------
 * mode 0 (softmax): pred = probabilities [B, C, HW], labels int64 [B, HW]; mode 1 (hinge): pred = logits [B, HW],
 * flabels = float 0/1 labels [B, HW], C = 1.  A segment is one (group, class): group = image when per_image else the
 * whole batch; S = groups*C segments of P = (per_image ? HW : B*HW) elements, n = S*P < 2^31.
 * seg_loss[s] (double, zeroed by this call) = dot(relu(errors_sorted), lovasz_grad(fg_sorted)); fg_total[s] = number
 * of foreground pixels (class presence); grad_at_pixel[s*P + i] = Lovasz gradient at the rank of pixel i (for backward;
 * may be NULL when no backward will follow: the scatter of the gradients to pixel order is then skipped).
 * Workspaces are caller-provided device buffers: keys_a/keys_b u32[n] (key = ~kappa, kappa = bits(max(error, +0)) << 1 | fg: the
 * errors in descending order, ties by fg, then by index -- the reference's torch.sort leaves the order of ties open),
 * vals_a/vals_b u32[n] (index << 1 | fg), chunk u32[S*ceil(P/2048)], temp of ptb_lovasz_temp_bytes(P, S) bytes (digit histograms of the
 * hand-written segmented radix sort: four stable 8-bit passes per segment). */
int64_t ptb_lovasz_temp_bytes(int64_t per_segment, int segments);
int ptb_lovasz_fwd(const float* pred, const int64_t* labels, const float* flabels, int B, int C, int64_t HW, int mode,
                   int per_image, int has_ignore, int64_t ignore_label, float ignore_value, uint32_t* keys_a, uint32_t* keys_b,
                   unsigned* vals_a, unsigned* vals_b, unsigned* chunk, unsigned* fg_total,
                   double* seg_loss, float* grad_at_pixel, void* temp, int64_t temp_bytes, ptb_stream_t stream);
/* ptb_lovasz_fwd with the gradient left BINNED instead of scattered to pixel order (16.7 M random 4-byte writes at [4,16,512,512]
 * become one more pass of the sort's scatter): on return keys_b[] holds (index << 1 | fg) and vals_b[] the fp32 gradient bits of the
 * same element, grouped by blocks of 2^r pixels, r = the RETURN VALUE (12..14): the pairs of block b of segment s are at
 * s*P + (b << r) ..., in arbitrary order inside the block.  scratch is unused (may be NULL).  PTB_EUNSUPPORTED when a segment
 * has more than 256 * 2^14 elements (use ptb_lovasz_fwd).  ptb_lovasz_bwd_binned consumes (keys_b, vals_b, r). */
/* ptb_lovasz_fwd_keys: the forward WITHOUT a gradient (evaluation / torch.no_grad()) as a key-only sort -- no (index, fg) value travels
 * with the key: errors <= 0 and ignored pixels share the key of +0 (they contribute relu(e) * grad = 0 wherever they sort among
 * themselves), a positive error's 31 significant bits move up by one and the foreground flag takes the freed bit.  Same seg_loss /
 * fg_total as ptb_lovasz_fwd (the order of equal errors differs, which the loss does not depend on); 4 bytes per element and pass. */
int ptb_lovasz_fwd_keys(const float* pred, const int64_t* labels, const float* flabels, int B, int C, int64_t HW, int mode, int per_image,
                        int has_ignore, int64_t ignore_label, float ignore_value, uint32_t* keys_a, uint32_t* keys_b, unsigned* chunk,
                        unsigned* fg_total, double* seg_loss, void* temp, int64_t temp_bytes, ptb_stream_t stream);
int ptb_lovasz_fwd_binned(const float* pred, const int64_t* labels, const float* flabels, int B, int C, int64_t HW, int mode,
                          int per_image, int has_ignore, int64_t ignore_label, float ignore_value, uint32_t* keys_a, uint32_t* keys_b,
                          unsigned* vals_a, unsigned* vals_b, unsigned* chunk, unsigned* fg_total,
                          double* seg_loss, float* scratch, void* temp, int64_t temp_bytes, ptb_stream_t stream);
int ptb_lovasz_bwd_binned(const float* pred, const int64_t* labels, const float* flabels, const float* coef, const uint32_t* binned_vals,
                          const float* binned_grad, float* grad, int B, int C, int64_t HW, int mode, int per_image, int has_ignore,
                          int64_t ignore_label, float ignore_value, int block_log2, ptb_stream_t stream);
/* ptb_lovasz_bwd_binned with the incoming gradient of the scalar loss as a DEVICE scalar gscale and ptb_lovasz_reduce's coef_out as
 * coef_unit: coefficient of segment s = gscale[0] * coef_unit[s], formed inside the kernel (the rounding of the [S]-sized product the
 * caller would otherwise launch in front of it). */
int ptb_lovasz_bwd_binned2(const float* pred, const int64_t* labels, const float* flabels, const float* coef_unit, const float* gscale,
                           const uint32_t* binned_vals, const float* binned_grad, float* grad, int B, int C, int64_t HW, int mode,
                           int per_image, int has_ignore, int64_t ignore_label, float ignore_value, int block_log2, ptb_stream_t stream);
/* The scalar the modules return from seg_loss / fg_total (losses/lovasz.py:92-108, :110-140): per group the mean of seg_loss over
 * the classes with fg_total > 0 (present_only = 1, classes="present") or over all classes (0; the hinge loss is C = 1), 0 when none
 * is selected; then the mean over the groups.  loss_out = DEVICE float; coef_out = DEVICE float[groups*C] = d(loss)/d(seg_loss). */
int ptb_lovasz_reduce(const double* seg_loss, const unsigned* fg_total, int groups, int C, int present_only, float* loss_out,
                      float* coef_out, ptb_stream_t stream);
/* grad[pred layout] = coef[s] * grad_at_pixel * d(error)/d(pred); coef = DEVICE float[S].  Every element of grad is written. */
int ptb_lovasz_bwd(const float* pred, const int64_t* labels, const float* flabels, const float* coef,
                   const float* grad_at_pixel, float* grad, int B, int C, int64_t HW, int mode, int per_image,
                   int has_ignore, int64_t ignore_label, float ignore_value, ptb_stream_t stream);

/* ---- Run-length codec of masks (utils/rle.py:6-39) --------------------------------------------------------------
 * mask = [B, H, W] contiguous, elem_bytes 1 (bool / uint8), 2, 4 or 8 (signed); N = H*W <= 2^31 - 2 (PTB_EUNSUPPORTED above).
 * labels = HOST int64[K]: one encoding per (slice, label) with foreground mask == label, encoding index e = slice * K + label index;
 * K = 0 (labels may be NULL): one encoding per slice with foreground mask != 0.  With f[p] = fg[p % H][p / H] (column-major, the
 * order of mask.T.flatten()) an encoding lists the maximal runs of f as (start + 1, length) pairs.
 * Two phases around the caller's one D2H read:
 *   ptb_rle_count   counts the run boundaries per (encoding, column, 32-row segment) and scans them (launches of their own; no
 *                   workgroup waits for another); on return (stream order) the first E + 1 int64 of the workspace hold the exclusive
 *                   offsets of the E = B * max(K, 1) encodings in the concatenated output, the last one the total.
 *   ptb_rle_write   out = int64[total]: encoding e is out[enc[e] .. enc[e + 1]).  Same mask, labels and workspace as the count call.
 * workspace = DEVICE buffer of ptb_rle_workspace_bytes(B, K, H, W) bytes (negative: a PTB_E* code), 16-byte aligned. */
int64_t ptb_rle_workspace_bytes(int B, int K, int H, int W);
int ptb_rle_count(const void* mask, int elem_bytes, int B, int H, int W, const int64_t* labels, int K, void* workspace,
                  int64_t workspace_bytes, ptb_stream_t stream);
int ptb_rle_write(const void* mask, int elem_bytes, int B, int H, int W, const int64_t* labels, int K, void* workspace,
                  int64_t workspace_bytes, int64_t* out, int64_t total, ptb_stream_t stream);
/* mask[H, W] (bytes) = 1 where some (start, length) pair of runs (DEVICE int64[2 * pairs], any order, overlapping) covers the pixel,
 * 0 elsewhere.  Runs are clamped to the mask, so unvalidated runs store nothing out of bounds.  workspace = DEVICE buffer of
 * ptb_rle_decode_workspace_bytes(H, W) bytes: the column-major image the runs are filled into before it is transposed. */
int64_t ptb_rle_decode_workspace_bytes(int H, int W);
int ptb_rle_decode(const int64_t* runs, int64_t pairs, int H, int W, uint8_t* mask, void* workspace, int64_t workspace_bytes,
                   ptb_stream_t stream);

/* ---- Confusion matrix of label maps and of logits (no counterpart in the reference) ---------------------------------
 * out = int64[G, K, K], ADDED to: out[g][t][p] += number of positions of group g with target == t and pred == p.  Values compare after
 * widening to int64 (elem_bytes 1 = bool / uint8 unsigned, 2 / 4 / 8 signed).  A position whose target equals ignore_index (when
 * has_ignore) is skipped; any other position whose target or pred lies outside [0, K) is skipped and counted in *invalid (int64,
 * ADDED to; the caller zeroes it).  1 <= K <= 256 (PTB_EUNSUPPORTED above).  The inputs are read where they lie, once per row block
 * (ptb_confusion_plan: 1 for K <= 128, up to 4 at K = 256); there is no workspace -- workgroups count in private 32-bit LDS
 * histograms of lds_bytes <= 64 KiB and flush them with 64-bit integer atomics, so the result is exact and independent of arrival
 * order.  Every launch is one kernel on `stream`; nothing is read back.
 *   ptb_confusion_labels   pred, target = [B, n_per_sample] contiguous; G = B (the pooled matrix of a whole tensor is B = 1).
 *   ptb_confusion_logits   logits = [N, C, S] contiguous in `dtype` (PTB_F32 / PTB_F16 / PTB_BF16), target = [N, S]; C <= 256.
 *                          C >= 2: K = C, pred = argmax over channels (first maximum wins, NaN counts as the maximum: the rule of
 *                          ptb_merge_crop's argmax kinds); C == 1: K = 2, pred = logit > threshold (NaN gives 0).
 *                          per_sample: G = N, else G = 1. */
int ptb_confusion_plan(int K, int* row_blocks, int* lds_bytes);
int ptb_confusion_labels(const void* pred, int pred_elem_bytes, const void* target, int target_elem_bytes, int64_t B, int64_t n_per_sample,
                         int K, int has_ignore, int64_t ignore_index, int64_t* out, int64_t* invalid, ptb_stream_t stream);
int ptb_confusion_logits(const void* logits, int dtype, int64_t N, int C, int64_t S, float threshold, const void* target, int target_elem_bytes,
                         int per_sample, int has_ignore, int64_t ignore_index, int64_t* out, int64_t* invalid, ptb_stream_t stream);

/* ---- Connected components of label maps (no counterpart in the reference) -------------------------------------------
 * labels = [B, D, H, W] contiguous (dims = 2: D == 1), elem_bytes 1 = bool / uint8, 2 / 4 / 8 signed; the B entries are labelled
 * independently in the same launches.  Two neighbouring positions are in one component iff they hold the same value and that value is
 * not `background` (has_background = 0: every value is foreground; a background the element type cannot hold occurs nowhere).
 * connectivity: 4 | 8 (dims = 2), 6 | 26 (dims = 3).  B * D * H * W <= 2^31 - 2 (PTB_EUNSUPPORTED above).  Block-based union-find,
 * every phase a launch of its own on `stream` (tiles in LDS -> seams by atomicMin on a parent map -> flatten -> scan -> rank); no
 * workgroup waits for another one, every loop is capped, nothing is read back, and the result is a function of the input alone.
 *   ptb_cc_plan          host only: tile = {TZ, TY, TX} of phase 1, the tiles and the 1024-position chunks of the call, the levels of
 *                        the scan over chunks + 1 root counts, and the workspace bytes of ptb_cc_label / ptb_cc_remove_small.
 *   ptb_cc_label         cc = int32 like labels: 0 at background, else 1 .. n within each entry, numbered in row-major order of each
 *                        component's first position; count = int64[B] = n, or -1 for an entry in which a step cap was exceeded.
 *   ptb_cc_remove_small  out (like labels; may be labels) = labels with every component of fewer than min_area positions replaced
 *                        by fill; an entry in which a step cap was exceeded is copied unchanged.  No scan, no numbering.
 *   ptb_cc_stats         of ONE entry's cc map and components 1 .. max_components (larger numbers are left out): area =
 *                        int64[max_components]; bbox = int64[max_components, 2 * dims], minima then exclusive maxima in (z,) y, x
 *                        order, all zero where area is 0; value[c] (values_elem_bytes each; both NULL: none) = values at a position
 *                        of component c + 1.  Runs of equal numbers are folded across the wave and the workgroup before the 64-bit
 *                        integer atomics.
 * workspace: DEVICE, 16-byte aligned, at least the plan's bytes (PTB_EINVAL otherwise); cc 16-byte aligned. */
int ptb_cc_plan(int dims, int64_t B, int64_t D, int64_t H, int64_t W, int* tile, int64_t* tiles, int64_t* chunks, int* scan_levels,
                int64_t* label_workspace_bytes, int64_t* remove_workspace_bytes);
int ptb_cc_label(const void* labels, int elem_bytes, int dims, int64_t B, int64_t D, int64_t H, int64_t W, int connectivity, int has_background,
                 int64_t background, int32_t* cc, int64_t* count, void* workspace, int64_t workspace_bytes, ptb_stream_t stream);
int ptb_cc_remove_small(const void* labels, int elem_bytes, int dims, int64_t B, int64_t D, int64_t H, int64_t W, int connectivity,
                        int has_background, int64_t background, int64_t min_area, int64_t fill, void* out, void* workspace,
                        int64_t workspace_bytes, ptb_stream_t stream);
int ptb_cc_stats(const int32_t* cc, int dims, int64_t D, int64_t H, int64_t W, int64_t max_components, const void* values, int values_elem_bytes,
                 int64_t* area, int64_t* bbox, void* value, ptb_stream_t stream);

/* ---- Exact Euclidean distance transform of label maps (no counterpart in the reference) -----------------------------
 * labels = [B, D, H, W] contiguous (dims = 2: D == 1), elem_bytes 1 = bool / uint8, 2 / 4 / 8 signed, read where it lies; the B entries
 * are transformed independently in the same launches.  SITES are the positions distances are measured to: the positions that hold
 * `value` (site_rule PTB_EDT_SITES_EQUAL: value is the background) or that do not hold it (PTB_EDT_SITES_NOT_EQUAL: value is the one
 * foreground class); a value the element type cannot hold occurs nowhere.  out[p] = the Euclidean distance from p to the nearest site
 * of its entry, 0 at sites; an entry without a site gets +inf (int32 form: 2^31 - 1).
 *   spacing       NULL: unit spacing, the passes run on exact int32 squared distances.  Else HOST, three positive finite doubles in
 *                 z, y, x order (z is ignored for dims = 2): float32 maps, every parabola evaluated in double and rounded once per pass.
 *   flags         PTB_EDT_SQUARED: the squared distance.  PTB_EDT_SIGNED: out = d(p -> nearest position that is NOT a site) -
 *                 d(p -> nearest site) (squared: the same sign times d^2): two runs of the passes, the second one with the
 *                 complementary rule, whose last pass subtracts what the first run left in out.
 *   out_kind      PTB_EDT_OUT_F32, or PTB_EDT_OUT_I32 (only with PTB_EDT_SQUARED and spacing == NULL: the exact integers).
 * Passes, each a launch of its own on `stream`: a row pass along W (a wave per row, forward and backward with the last site carried),
 * then one lower-envelope pass (Meijster) along H and, for dims = 3, along D: a lane per line, the envelope's stack in the workspace.
 * No workgroup waits for another one, there are no atomics, every loop is capped by the extent of its axis; nothing is read back and
 * the result is a function of the input alone.  B * D * H * W <= 2^31 - 2 and (dims = 3: D^2 +) H^2 + W^2 <= 2^31 - 2
 * (PTB_EUNSUPPORTED above), so every squared index distance and every intermediate of the envelope is an int32.
 * workspace: DEVICE, 16-byte aligned, ptb_edt_plan's bytes: 12 bytes per position (the 32-bit map of the previous axis + two 32-bit
 * stack words; `out` serves as the other map), + 4 per position for a signed dims = 3 call (the second run must not overwrite out
 * before its last pass), each rounded up to 16.  out 16-byte aligned. */
#define PTB_EDT_SITES_EQUAL 0
#define PTB_EDT_SITES_NOT_EQUAL 1
#define PTB_EDT_SQUARED 1
#define PTB_EDT_SIGNED 2
#define PTB_EDT_OUT_F32 0
#define PTB_EDT_OUT_I32 1
int ptb_edt_plan(int dims, int64_t B, int64_t D, int64_t H, int64_t W, int is_signed, int64_t* workspace_bytes);
int ptb_edt(const void* labels, int elem_bytes, int dims, int64_t B, int64_t D, int64_t H, int64_t W, int site_rule, int64_t value,
            const double* spacing, int flags, void* out, int out_kind, void* workspace, int64_t workspace_bytes, ptb_stream_t stream);

/* ---- Nearest-site feature transform and label expansion (no counterpart in the reference) ----------------------------
 * labels, elem_bytes, dims, B, D, H, W, site_rule, value, spacing: as ptb_edt, with the same limits.  One entry point; `flags` says
 * what it leaves, any combination that asks for something (PTB_EINVAL for none, for an unknown bit, for PTB_NEAREST_MAX_SQ without
 * PTB_NEAREST_GATHER, and when a pointer below is set without its flag or missing with it):
 *   PTB_NEAREST_INDEX    index_out [B, D, H, W] int32: the linear index (z * H + y) * W + x, within the position's own entry, of the
 *                        nearest site; a site gets its own index; -1 everywhere in an entry without a site.  Among the sites at the
 *                        minimum distance the one with the SMALLEST index: every pass prefers the smaller coordinate of its axis on a
 *                        tie and the axes are passed from the fastest to the slowest.  With spacing the maps are float32 (as ptb_edt):
 *                        the rule holds with respect to the stored values, bit for bit wherever they are exact.
 *   PTB_NEAREST_SQUARED  squared_out [B, D, H, W]: the squared distance to that site, int32 with spacing == NULL (2^31 - 1 without a
 *                        site) and float32 otherwise (+inf): the bits of ptb_edt with PTB_EDT_SQUARED on the same arguments.
 *   PTB_NEAREST_GATHER   label expansion.  labels are the markers, site_rule must be PTB_EDT_SITES_NOT_EQUAL and value the background:
 *                        the labelled positions are the sites.  gather_out [B, D, H, W] of elem_bytes: a labelled position keeps its
 *                        value; another one takes the value at its nearest labelled position if (mask == NULL or mask[p] != 0) and
 *                        (without PTB_NEAREST_MAX_SQ, or its squared distance <= max_sq), else `value`.  gather_out must not overlap
 *                        labels.  mask: [B, D, H, W] bytes.
 *   PTB_NEAREST_MAX_SQ   max_sq >= 0 limits the expansion.  spacing == NULL: the kernel compares int32 with (int)max_sq, clipped to
 *                        2^31 - 1 -- pass floor(distance^2); otherwise the float32 squared distance, widened, with max_sq in double.
 * Launches on `stream`: the row pass, a line pass along H and for dims = 3 along D (the passes of ptb_edt, each carrying a second
 * 32-bit map with the site), then for PTB_NEAREST_GATHER one gather kernel.  No workgroup waits for another one, there are no
 * atomics, every loop is capped by the extent of its axis; nothing is read back and the result is a function of the inputs alone.
 * workspace: DEVICE, 16-byte aligned, ptb_nearest_plan's bytes for the same shape and flags.  Per position: 8 (the two 32-bit stack
 * words) + 4 per distance map + 4 per feature map that is not a caller's tensor.  There are two maps of each kind (a pass never reads
 * the map it writes); the one the last pass writes is index_out / squared_out where given, and the last distance map of a dims = 2
 * call does not exist when nobody reads it.  So: INDEX 16 (dims = 3: 20), INDEX | SQUARED 16, GATHER 20 (dims = 3: 24),
 * GATHER | MAX_SQ 24; each map rounded up to 16 bytes.  index_out, squared_out and gather_out 16-byte aligned. */
#define PTB_NEAREST_INDEX 1
#define PTB_NEAREST_SQUARED 2
#define PTB_NEAREST_GATHER 4
#define PTB_NEAREST_MAX_SQ 8
int ptb_nearest_plan(int dims, int64_t B, int64_t D, int64_t H, int64_t W, int flags, int64_t* workspace_bytes);
int ptb_nearest(const void* labels, int elem_bytes, int dims, int64_t B, int64_t D, int64_t H, int64_t W, int site_rule, int64_t value,
                const double* spacing, int flags, int32_t* index_out, void* squared_out, void* gather_out, const void* mask, double max_sq,
                void* workspace, int64_t workspace_bytes, ptb_stream_t stream);

/* ---- Marker-controlled watershed (no counterpart in the reference) ---------------------------------------------------
 * height [B, D, H, W] contiguous of height_dtype (PTB_F32, PTB_F16, PTB_BF16, PTB_U8, PTB_I16: widened to float32 on load, -0 counts as
 * +0), markers [B, D, H, W] of marker_bytes (1 = bool / uint8, 2 / 4 / 8 signed), mask [B, D, H, W] bytes or NULL; dims = 2 (D == 1) or 3;
 * connectivity 4 | 8 (dims = 2), 6 | 26 (dims = 3); B * D * H * W <= 2^31 - 2 (PTB_EUNSUPPORTED above).  All read where they lie.
 * The flooded set M: mask != 0 (all positions without a mask) and height neither NaN nor +inf.  Seeds: the positions of M whose marker
 * is not `background` (a background the element type cannot hold occurs nowhere: every position of M is a seed).  Per entry,
 *   C(p)      the pass height: min over paths of neighbouring positions of M from a seed to p of the max height on the path;
 *   D(p)      the fewest ADMISSIBLE steps (q -> p with C(q) <= C(p)) from a seed to p;
 *   sigma(p)  the smallest linear index (z * H + y) * W + x among the seeds with an admissible path of D(p) steps to p.
 * labels_out [B, D, H, W] of marker_bytes = markers[sigma(p)], and `fill` (the background as the element type holds it) outside M and
 * where no path exists; it must not overlap markers.  `flags`: PTB_WATERSHED_COST -> cost_out float32 = C (+inf where unreached),
 * PTB_WATERSHED_SEED -> seed_out int32 = sigma (-1 where unreached); a pointer without its flag, or a flag without its pointer, is
 * PTB_EINVAL, as an unknown bit is.  The result is a function of the inputs alone.
 * Launches on `stream`: an init kernel, then SWEEPS of the cost kernel until nothing changes, sweeps of the path kernel likewise (the
 * phases cannot be fused), then a gather kernel.  A workgroup relaxes one tile in LDS; only the owning tile writes a position; no
 * workgroup waits for another one, there are no atomic read-modify-writes, every loop is capped.  Sweeps are launched eight at a time;
 * after each batch ONE 4-BYTE WORD IS READ BACK on `stream` and the stream is synchronised -- so the call CANNOT BE CAPTURED into a graph.
 * More than max_sweeps (>= 1) sweeps in a phase, the one that finds nothing to do included -> PTB_ENOTCONVERGED; labels_out is then
 * unwritten.  sweeps_out: HOST, two ints or NULL: the sweeps each phase took (-1: the phase was not reached; with PTB_ENOTCONVERGED the
 * failing phase holds the sweeps it ran).
 * workspace: DEVICE, 16-byte aligned, ptb_watershed_plan's bytes: per position 16 (height key 4, cost key 4, path key 8), per tile
 * (2-D: 64 x 64 positions; 3-D: 8 x 8 x 32) 12, and 16 more; each array rounded up to 16 bytes.  labels_out, cost_out and seed_out
 * 16-byte aligned. */
#define PTB_ENOTCONVERGED (-7) /* ptb_watershed: a phase took more than max_sweeps sweeps */
#define PTB_WATERSHED_COST 1
#define PTB_WATERSHED_SEED 2
int ptb_watershed_plan(int dims, int64_t B, int64_t D, int64_t H, int64_t W, int flags, int64_t* workspace_bytes);
int ptb_watershed(const void* height, int height_dtype, const void* markers, int marker_bytes, const void* mask, int dims, int64_t B, int64_t D,
                  int64_t H, int64_t W, int connectivity, int64_t background, int64_t fill, int flags, int max_sweeps, void* labels_out,
                  float* cost_out, int32_t* seed_out, int32_t* sweeps_out, void* workspace, int64_t workspace_bytes, ptb_stream_t stream);

/* ---- Morphological reconstruction, regional and h-extrema, hole filling (no counterpart in the reference) ------------
 * mask (and, for PTB_RECONSTRUCT_VALUES, seed) [B, D, H, W] contiguous of dtype (PTB_F32, PTB_F16, PTB_BF16, PTB_U8, PTB_I16: widened to
 * float32 on load, -0 counts as +0), domain [B, D, H, W] bytes or NULL; dims = 2 (D == 1) or 3; connectivity 4 | 8 (dims = 2), 6 | 26
 * (dims = 3); B * D * H * W <= 2^31 - 2 (PTB_EUNSUPPORTED above).  All read where they lie.
 * THE DOMAIN: domain != 0 (all positions without one) and mask not NaN.  Positions outside it are nobody's neighbour.  Per entry, R is
 * the least fixed point of R(p) <- max(R(p), min(R(q), mask(p))) over the neighbours q in the domain, from min(start, mask); with
 * erosion = 1 the mirror image (min and max exchanged, from max(start, mask)), computed on complemented keys.  `op` names the start
 * and the result:
 *   PTB_RECONSTRUCT_VALUES     start = seed (a NaN counts as -inf; erosion: +inf).  out of dtype = R; outside the domain the mask's element.
 *   PTB_RECONSTRUCT_EXTREMA    start = mask one step of the ordered 32-bit key down (erosion: up).  out bytes = R < mask (erosion: R > mask):
 *                              the regional maxima (minima); 0 outside the domain.
 *   PTB_RECONSTRUCT_H_EXTREMA  start = float32(mask) - h (erosion: + h), h >= 0 finite; when that has converged, its R becomes the mask
 *                              of a second PTB_RECONSTRUCT_EXTREMA phase.  out bytes as there.
 *   PTB_RECONSTRUCT_FILL       erosion must be 1: start = mask on the faces of the entry, +inf elsewhere.  out of dtype = min(R, top)
 *                              (top: what a domain position that no face reaches holds; the highest value of the caller's type).
 * h must be 0 and top +inf where they have no meaning; seed NULL except for PTB_RECONSTRUCT_VALUES, out != seed.  out may be mask
 * itself but must not overlap it otherwise.  The result is a function of the inputs alone.
 * Launches on `stream`: an init kernel, SWEEPS of the relaxation kernel until nothing changes (h-extrema: a restage kernel and a second
 * run of sweeps), then a gather or a compare kernel.  A workgroup relaxes one tile in LDS; only the owning tile writes a position; no
 * workgroup waits for another one, there are no atomic read-modify-writes, every loop is capped.  Sweeps are launched eight at a time;
 * after each batch ONE 4-BYTE WORD IS READ BACK on `stream` and the stream is synchronised -- so the call CANNOT BE CAPTURED into a graph.
 * More than max_sweeps (>= 1) sweeps in a phase, the one that finds nothing to do included -> PTB_ENOTCONVERGED; out is then unwritten.
 * sweeps_out: HOST, two ints or NULL: the sweeps each phase took (-1: the phase was not reached or does not exist; with
 * PTB_ENOTCONVERGED the failing phase holds the sweeps it ran).
 * workspace: DEVICE, 16-byte aligned, ptb_reconstruct_plan's bytes -- the only place that knows the layout: per position 8 (mask key 4,
 * R 4), per tile (2-D: 64 x 64 positions; 3-D: 8 x 8 x 32) 12, and 16 more; each array rounded up to 16 bytes.  out 16-byte aligned. */
#define PTB_RECONSTRUCT_VALUES 0
#define PTB_RECONSTRUCT_EXTREMA 1
#define PTB_RECONSTRUCT_H_EXTREMA 2
#define PTB_RECONSTRUCT_FILL 3
int ptb_reconstruct_plan(int dims, int64_t B, int64_t D, int64_t H, int64_t W, int op, int64_t* workspace_bytes);
int ptb_reconstruct(const void* seed, const void* mask, int dtype, const void* domain, int dims, int64_t B, int64_t D, int64_t H, int64_t W,
                    int connectivity, int op, int erosion, float h, float top, int max_sweeps, void* out, int32_t* sweeps_out, void* workspace,
                    int64_t workspace_bytes, ptb_stream_t stream);

/* ---- Skeletons by parallel thinning, centreline Dice (no counterpart in the reference) -------------------------------
 * THE NEIGHBOURS of a position P1 = (y, x): P2 (y-1, x), P3 (y-1, x+1), P4 (y, x+1), P5 (y+1, x+1), P6 (y+1, x), P7 (y+1, x-1),
 * P8 (y, x-1), P9 (y-1, x-1); positions outside the entry are background.  One ITERATION is sub-iteration 0, then sub-iteration 1, each
 * synchronous: every decision reads the state from before that sub-iteration.  An object position is deleted in sub-iteration k iff
 *   PTB_THIN_ZHANG (Zhang & Suen 1984)  B = the number of set neighbours, A = the number of i with P_i = 0 and P_i+1 = 1 in the cycle
 *       P2, P3, ..., P9, P2:  2 <= B <= 6 and A == 1 and  k = 0: P2 P4 P6 == 0 and P4 P6 P8 == 0;  k = 1: P2 P4 P8 == 0 and P2 P6 P8 == 0.
 *   PTB_THIN_GUO_HALL (Guo & Hall 1989, as in OpenCV's ximgproc.thinning)
 *       C = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2)),  N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8),
 *       N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9),  N = min(N1, N2),  m = (P6|P7|!P9) & P8 for k = 0, (P2|P3|!P5) & P4 for k = 1:
 *       C == 1 and 2 <= N <= 3 and m == 0.
 * THE SKELETON is the state after the first iteration that deletes nothing; with max_iterations = n >= 0 the state after at most n
 * iterations (0: the object itself).  THE ITERATION COUNT is the number of iterations that deleted something.
 *   ptb_thin_rule   HOST ONLY, no stream, no GPU: the rule on words, as the kernels evaluate it.  Bit i of centre and of nbr[0 .. 8) (the
 *                   words of P2 .. P9) is one position; returns the positions of centre that sub-iteration sub (0 | 1) deletes; 0 for an
 *                   unknown method or sub.
 *   ptb_thin_steps  HOST ONLY: the sub-iterations one launch of the thinning kernel runs (even, <= 32).
 *   ptb_skeleton    labels [B, H, W] contiguous of elem_bytes (1 = bool / uint8, 2 / 4 / 8 signed), read where it lies.  The object:
 *                   PTB_THIN_NOT_EQUAL: labels != value, PTB_THIN_EQUAL: labels == value; a value the element type cannot hold occurs
 *                   nowhere.  B * H * W <= 2^31 - 2 (PTB_EUNSUPPORTED above).  out [B, H, W] bytes, 0 | 1, 16-byte aligned; it must not
 *                   overlap labels.  max_iterations < 0: run to stability under a guard of H + W iterations, beyond which the call returns
 *                   PTB_ENOTCONVERGED with out unwritten (a max_iterations >= H + W counts as < 0).  took: HOST, two ints or NULL: the
 *                   iteration count of the call (of the entry that took longest) and the launches of the thinning kernel that ran.
 *   ptb_centerline_dice   pred, truth [B, H, W] label maps as above, each with its own elem_bytes.  Object k: with PTB_THIN_EQUAL the
 *                   positions that hold class_values[k] (HOST, 1 <= K <= 32 values), with PTB_THIN_NOT_EQUAL (K == 1) those that do not hold
 *                   class_values[0].  With S the skeleton and V the mask of object k in each map, all DEVICE, obj = b * K + k:
 *                     counts [obj][4] int64 = |S_P & V_T|, |S_P|, |S_T & V_P|, |S_T|  (exact; zeroed by the call)
 *                     tprec = counts[0] / counts[1], tsens = counts[2] / counts[3], cldice = 2 tprec tsens / (tprec + tsens): float32 [obj],
 *                     evaluated in float64 in that order and rounded once.  An empty skeleton gives nan in its own ratio; cldice is nan
 *                     when both are empty, 0 when exactly one is or when tprec + tsens == 0.
 *                   2 * K * B * H * W <= 2^31 - 2 (PTB_EUNSUPPORTED above); thinning runs to stability under the guard.
 * STATE: bit planes, 32 positions a word, WW = ceil(W / 32) words a row, bits at columns >= W zero; two planes for ping-pong (a launch
 * reads one and writes the other) and, for ptb_centerline_dice, a third with the untouched masks, over 2 * K * B entries thinned in the
 * same launches.  Launches on `stream`: a pack kernel (per side), LAUNCHES of the thinning kernel -- a workgroup holds a 64 x 64 tile
 * with a halo of ptb_thin_steps() rows and one word in LDS and runs that many sub-iterations there; a tile runs iff it or one of its 8
 * neighbours changed in the launch before --, then an unpack kernel, or a count kernel (popcounts folded per wave, then 64-bit integer
 * atomic adds: exact and order-free) and a one-workgroup finish kernel.  No workgroup waits for another one, every loop is bounded.
 * Launches go eight at a time; after each batch ONE 4-BYTE WORD IS READ BACK on `stream` and the stream is synchronised, and one more
 * word (the iteration count) at the end -- so the calls CANNOT BE CAPTURED into a graph.  The result is a function of the inputs alone.
 * workspace: DEVICE, 16-byte aligned, the plan entry's bytes: 4 * H * WW per plane and entry (2 planes; clDice: 3, over 2 * K * B
 * entries), per tile 12, and 16 more; each array rounded up to 16 bytes. */
#define PTB_THIN_ZHANG 0
#define PTB_THIN_GUO_HALL 1
#define PTB_THIN_EQUAL 0
#define PTB_THIN_NOT_EQUAL 1
uint32_t ptb_thin_rule(int method, int sub, const uint32_t* nbr, uint32_t centre);
int ptb_thin_steps(void);
int ptb_skeleton_plan(int64_t B, int64_t H, int64_t W, int64_t* workspace_bytes);
int ptb_skeleton(const void* labels, int elem_bytes, int64_t B, int64_t H, int64_t W, int object_rule, int64_t value, int method,
                 int64_t max_iterations, void* out, int32_t* took, void* workspace, int64_t workspace_bytes, ptb_stream_t stream);
int ptb_centerline_dice_plan(int64_t B, int64_t H, int64_t W, int K, int64_t* workspace_bytes);
int ptb_centerline_dice(const void* pred, int pred_elem_bytes, const void* truth, int truth_elem_bytes, int64_t B, int64_t H, int64_t W,
                        const int64_t* class_values, int K, int object_rule, int method, int64_t* counts, float* cldice, float* tprec,
                        float* tsens, int32_t* took, void* workspace, int64_t workspace_bytes, ptb_stream_t stream);

/* ---- Surface metrics of two label maps (no counterpart in the reference) ---------------------------------------------
 * pred, truth = [B, D, H, W] contiguous label maps (dims = 2: D == 1), each with its own elem_bytes (1 = bool / uint8, 2 / 4 / 8
 * signed), read where they lie.  Object k of an entry is, with PTB_SURFACE_CLASSES, the positions that hold class_values[k] (HOST, K
 * values) and, with PTB_SURFACE_NOT_BACKGROUND (K == 1), the positions that do not hold class_values[0]; a value the element type
 * cannot hold occurs nowhere.  The SURFACE of an object: its positions with a `connectivity`-neighbour (4 / 8, dims = 3: 6 / 26) that
 * is not in it or lies outside the map.  The directed sample set pred -> truth: the Euclidean distance of every surface position of
 * pred's object to the nearest surface position of truth's object; truth -> pred is the mirror.  Results, obj = b * K + k, all DEVICE:
 *   surface_count [obj][2] int64; directed_hausdorff [obj][2], hausdorff [obj], directed_percentile [obj][2], hausdorff_percentile [obj]
 *   (the percentile of the two sets pooled), mean_surface_distance [obj][2], assd [obj], surface_dice [obj][T]: float32.
 * A direction without samples gives nan; both surfaces empty: nan in the symmetric results; exactly one empty: inf in hausdorff,
 * hausdorff_percentile and assd and 0 in surface_dice.  percentile in [0, 100], interpolated linearly between the order statistics
 * at (n - 1) * percentile / 100; tolerances: HOST, 1 <= T <= 8 values >= 0; spacing: as ptb_edt (NULL: exact int32 squared distances).
 * Per chunk of classes_per_chunk classes: a border kernel per side, ONE ptb_edt over the [chunk * 2 * B] border maps, a sample kernel
 * (maxima, tolerance counts, per-workgroup partial sums in double, first histogram), three more histogram passes of a radix select
 * with a pick kernel after each, and a pass for the upper order statistic; then one finishing kernel.  Stream-ordered, nothing is
 * read back, no workgroup waits for another one, every loop is bounded by the shape; the result is a function of the inputs alone and
 * does not depend on the chunking.
 * ptb_surface_plan: the largest chunk (at most 32 classes) whose workspace stays within max_workspace_bytes and whose transform stays
 * within 2^31 - 2 positions.  min_workspace_bytes (written whenever the shape is supported) is the workspace of one class per chunk;
 * PTB_EINVAL when max_workspace_bytes is below it, PTB_EUNSUPPORTED when 2 * B * D * H * W or the squared extents pass 2^31 - 2.
 * partial_sums_per_map: the workgroups of the sample kernel per map, a function of D * H * W alone.
 * workspace: DEVICE, 16-byte aligned, workspace_bytes as planned (ptb_surface_metrics plans again with workspace_bytes as the cap). */
#define PTB_SURFACE_CLASSES 0
#define PTB_SURFACE_NOT_BACKGROUND 1
int ptb_surface_plan(int dims, int64_t B, int64_t D, int64_t H, int64_t W, int K, int64_t max_workspace_bytes, int* classes_per_chunk,
                     int64_t* workspace_bytes, int64_t* min_workspace_bytes, int* partial_sums_per_map);
int ptb_surface_metrics(const void* pred, int pred_elem_bytes, const void* truth, int truth_elem_bytes, int dims, int64_t B, int64_t D, int64_t H,
                        int64_t W, const int64_t* class_values, int K, int object_rule, int connectivity, const double* spacing, double percentile,
                        const double* tolerances, int T, int64_t* surface_count, float* directed_hausdorff, float* hausdorff,
                        float* directed_percentile, float* hausdorff_percentile, float* mean_surface_distance, float* assd, float* surface_dice,
                        void* workspace, int64_t workspace_bytes, ptb_stream_t stream);

/* ---- Overlap table, IoU matching and panoptic quality of two instance maps (no counterpart in the reference) ---------
 * pred, truth = int32 instance maps of `positions` elements each, contiguous, compared position by position (any shape is one entry),
 * read where they lie (16-byte loads when both bases are 16-byte aligned, element loads otherwise and for the tail).  Ids 1 .. n_pred /
 * 1 .. n_truth are instances; an id <= 0 or above that side's n is background.  1 <= positions <= 2^31 - 2, n_pred, n_truth <=
 * 2^31 - 2, max_pairs <= 2^28 (PTB_EUNSUPPORTED above).  A PAIR is a (pred id, truth id) that occurs at some position, both >= 1.
 *   ptb_inst_plan      host only: the slots of the global table (the power of two >= 2 * max_pairs, at least 2), the workspace bytes
 *                      and the layout of the output block: out_offsets[17] = byte offsets, each a multiple of 16, of
 *                        0 num_pairs int64      1 pred_area int64[n_pred]   2 truth_area int64[n_truth]
 *                        3 pairs int32[rows][2] 4 intersection int64[rows]                       (rows = max_pairs; T >= 1: 0)
 *                        5 pred_match int32[n_pred]  6 truth_match int32[n_truth]  7 pred_iou double[n_pred]  8 truth_iou double[n_truth]
 *                        9 tp  10 fp  11 fn  int64[KK][T];  12 sum_iou  13 sq  14 rq  15 pq  16 ap  double[KK][T]   (KK = max(K, 1))
 *                      T = 0 plans ptb_inst_overlaps (K must be 0), T = 1 .. 16 ptb_inst_match with K classes (0: none; <= 65535).
 *                      workspace = 16 + up16(8 S) + up16(4 S) [key, count] + up16(4 S) [first position] with S slots, plus
 *                        overlaps: W = ceil(positions / 32) bitmap words: up16(4 W) + up16(4 (W + 1)) + up16(8 (W + 1)) + the scan's sums;
 *                        match: (up16(4 x) + up16(8 x)) with x = ceil(n_pred / 1024) * KK * T, + up16(4 ceil(n_pred / 1024) KK)
 *                        + up16(4 ceil(n_truth / 1024) KK).
 *   ptb_inst_overlaps  rows in the order of each pair's FIRST position (row-major); rows past the real count stay zero.
 *   ptb_inst_match     thresholds: HOST, 1 <= T <= 16 increasing doubles in [0.5, 1).  A pair matches at tau iff
 *                      IoU = I / (A_p + A_t - I) > tau (one double division of exact integers) and, with classes (pred_class[n_pred],
 *                      truth_class[n_truth], DEVICE, elem bytes 1 = bool / uint8, 2 / 4 / 8 signed; K >= 1), both classes are equal and
 *                      in 0 .. K - 1.  pred_match / truth_match / pred_iou / truth_iou: the partner at thresholds[0] and its IoU, 0 if
 *                      none.  Present = area > 0 (with classes: and of that class).  tp = matches, fp = present preds - tp, fn =
 *                      present truths - tp, sum_iou = sum of the matched IoUs (partial sums per 1024 predictions from a fixed tree,
 *                      added in block order), sq = sum_iou / tp, rq = tp / (tp + fp / 2 + fn / 2), pq = sum_iou / (tp + fp / 2 + fn / 2),
 *                      ap = tp / (tp + fp + fn); nan where the denominator is 0.
 * num_pairs = the number of distinct pairs, or -1 iff the input has more than max_pairs of them (then every score is nan and the other
 * outputs are unspecified).  The whole output block is zeroed first.  Stream-ordered; nothing is read back; no workgroup waits for
 * another one; every probe loop is capped at its table's slot count; the result is a function of the inputs alone.
 * out, workspace: DEVICE, 16-byte aligned, at least the plan's bytes (PTB_EINVAL otherwise). */
int ptb_inst_plan(int64_t positions, int64_t n_pred, int64_t n_truth, int64_t max_pairs, int T, int64_t K, int64_t* slots, int64_t* workspace_bytes,
                  int64_t* out_offsets, int64_t* out_bytes);
int ptb_inst_overlaps(const int32_t* pred, const int32_t* truth, int64_t positions, int64_t n_pred, int64_t n_truth, int64_t max_pairs, void* out,
                      int64_t out_bytes, void* workspace, int64_t workspace_bytes, ptb_stream_t stream);
int ptb_inst_match(const int32_t* pred, const int32_t* truth, int64_t positions, int64_t n_pred, int64_t n_truth, int64_t max_pairs,
                   const double* thresholds, int T, const void* pred_class, int pred_class_elem_bytes, const void* truth_class,
                   int truth_class_elem_bytes, int64_t K, void* out, int64_t out_bytes, void* workspace, int64_t workspace_bytes, ptb_stream_t stream);

/* ---- Distance-map losses: boundary loss and Hausdorff-DT loss (no counterpart in the reference) ----------------------
 * logits = fp32 [B, C, S], S = (D *) H * W positions; the target is labels int64 [B, S] or dense fp32 [B, C, S] (object: > 0.5), exactly
 * one of them; prob = PTB_PROB_* turns logits into p.  K maps per sample: classes HOST int[K], distinct channels in [0, C), together with
 * class_table DEVICE int[K + C] (the K channels, then for every channel its map or -1); both NULL: K == C, map k is channel k.
 * has_ignore: positions that hold ignore_label (elements of dense equal to ignore_value) belong to no object, add nothing and are not
 * counted.  A MAP is the signed distance ptb_edt leaves for the object as non-sites (> 0 outside, < 0 inside), [B, K, S]:
 * PTB_DLOSS_MAPS_I32_SQUARED (sign * d^2, unit spacing) or PTB_DLOSS_MAPS_F32 (the distance).  An infinite value (+-inf, +-(2^31 - 1): an
 * entry whose object is empty or fills it) counts as 0.
 *   ptb_dloss_plan   host only.  The planes * B * K object maps are transformed in chunks of neighbouring ENTRIES (an entry is one [S] map;
 *                    classes are not contiguous in [R, B, K, S], entries are), one ptb_edt call each: the largest chunk whose ptb_edt
 *                    workspace (signed) stays within max_workspace_bytes and whose positions stay within 2^31 - 2, a multiple of
 *                    4 / gcd(S, 4) unless it is everything (a chunk's output starts 16-byte aligned).  min_workspace_bytes: the smallest
 *                    accepted cap (PTB_EINVAL below it).  partial_slots: the workgroups of ptb_dloss_fwd, B * ceil(S / 1024).
 *   ptb_dloss_masks  one launch writes the uint8 object maps [R, B, K, S]: PTB_DLOSS_PLANE_TRUTH (labels == class_k / dense > 0.5; logits
 *                    may be NULL when it is the only plane) and / or PTB_DLOSS_PLANE_PRED (p_k > 0.5), the truth first.
 *   ptb_dloss_fwd    PTB_DLOSS_BOUNDARY: term = p_k * phi_k.  PTB_DLOSS_HAUSDORFF: term = (p_k - g_k)^2 * (|phi_pred,k|^alpha +
 *                    |phi_truth,k|^alpha), g the 0 / 1 target; alpha == 2 on squared maps takes no root.  pred_maps NULL for the boundary
 *                    loss.  loss[r] = sum of the terms / number of (map, position) elements that are not ignored, over everything
 *                    (per_sample = 0, one result) or per sample (B results); inv_count[r] = 1 / that number.  No atomics: every
 *                    workgroup writes an fp64 sum and an int64 count to its slot of the workspace (16 bytes per slot, 16-byte aligned),
 *                    a second kernel adds the slots of a result in index order.  error_flag DEVICE int: zeroed, then set by a label
 *                    outside [0, C) that is not ignore_label, which also turns the loss into NaN.
 *   ptb_dloss_bwd    grad [B, C, S] = coef[r] * d(sum of the terms) / d logits; coef DEVICE float[1] (float[B] with per_sample):
 *                    upstream gradient times inv_count.  The maps are constants.  Zeros at ignored positions.
 * Stream-ordered, nothing is read back; the grids depend on the shape alone and the result is a function of the inputs alone.  16-byte
 * loads where S % 4 == 0 and the bases are 16-byte aligned (masks: 4), element accesses otherwise.  PTB_EINVAL before any launch for
 * null pointers, K < 1, K > C, a class outside [0, C) or named twice, a misaligned or short workspace, alpha <= 0. */
#define PTB_DLOSS_BOUNDARY 0
#define PTB_DLOSS_HAUSDORFF 1
#define PTB_DLOSS_PLANE_TRUTH 1
#define PTB_DLOSS_PLANE_PRED 2
#define PTB_DLOSS_MAPS_I32_SQUARED 0
#define PTB_DLOSS_MAPS_F32 1
int ptb_dloss_plan(int dims, int64_t B, int64_t D, int64_t H, int64_t W, int K, int planes, int64_t max_workspace_bytes,
                   int64_t* entries_per_chunk, int64_t* workspace_bytes, int64_t* min_workspace_bytes, int64_t* partial_slots);
int ptb_dloss_masks(const float* logits, const int64_t* labels, const float* dense, const int* classes, const int* class_table, int planes,
                    int B, int C, int K, int64_t S, int prob, int has_ignore, int64_t ignore_label, float ignore_value, uint8_t* masks,
                    ptb_stream_t stream);
int ptb_dloss_fwd(int kind, const float* logits, const int64_t* labels, const float* dense, const int* classes, const int* class_table,
                  const void* truth_maps, const void* pred_maps, int maps_kind, int B, int C, int K, int64_t S, int prob, int has_ignore,
                  int64_t ignore_label, float ignore_value, float alpha, int per_sample, void* workspace, int64_t workspace_bytes,
                  float* loss, float* inv_count, int* error_flag, ptb_stream_t stream);
int ptb_dloss_bwd(int kind, const float* logits, const int64_t* labels, const float* dense, const int* classes, const int* class_table,
                  const void* truth_maps, const void* pred_maps, int maps_kind, int B, int C, int K, int64_t S, int prob, int has_ignore,
                  int64_t ignore_label, float ignore_value, float alpha, int per_sample, const float* coef, float* grad,
                  ptb_stream_t stream);

/* ---- Hard-example mining: top-k % and OHEM cross-entropy on a device-side radix select (no counterpart in the reference) ----
 * logits = fp32 [B, C, S]; the target is labels int64 [B, S] (softmax cross-entropy, one ELEMENT per position) or dense fp32 [B, C, S]
 * targets in [0, 1] (sigmoid cross-entropy, one element per (channel, position)), exactly one of them.  The element loss is fp32 and
 * >= +0; elements whose label equals ignore_label (whose target equals ignore_value) are in no set.  A SELECTION SET is every element
 * (per_sample = 0, one result) or the elements of a sample (B results); n its size, counted on the device.
 *   PTB_HARDCE_TOPK  kept = max(1, floor((double)n * k_percent / 100)), 0 < k_percent <= 100
 *   PTB_HARDCE_OHEM  with t0 > 0 and m = min(min_kept, n): kept = (number of losses > t0) if that is at least m, else m
 * and the loss is the mean of the kept largest element losses: (sum of the losses above thr + (kept - gt) * thr) / kept, thr the
 * smallest kept value, gt the number of losses above it.  The eq elements that equal thr by bits share the kept - gt places: weight
 * (kept - gt) / eq each in the gradient.  kept == 0 (an empty set; OHEM with min_kept == 0 and nothing above t0): loss 0, thr +inf.
 *   ptb_hardce_workspace_bytes  host only: the workspace of ptb_hardce_fwd (16-byte aligned), or a negative error code.
 *   ptb_hardce_fwd   writes map (fp32 [B, S] or [B, C, S]: the element losses, all-ones bits where ignored -- the backward reads it),
 *                    loss, threshold, kept, inv_kept (1 / kept, 0 for kept == 0) of every set and select (8 bytes per set: the bits of
 *                    thr and of the tie weight).  error_flag DEVICE int: zeroed, then set by a label outside [0, C) that is not
 *                    ignore_label, which also turns the loss into NaN.
 *   ptb_hardce_bwd   grad [B, C, S] = coef[r] * weight * d(element loss) / d logits, coef DEVICE float[sets]: upstream gradient times
 *                    inv_kept.  The decision is read from the saved map; exact zeros at ignored and unkept elements.
 * Stream-ordered, nothing is read back; the grids depend on the shape alone; histograms and counts are integer atomics, floating-point
 * sums are added in a fixed order, so the result is a function of the inputs alone.  PTB_EINVAL before any launch for null pointers, a
 * shape below 1, an unknown rule, k_percent outside (0, 100], t0 <= 0 or not finite, min_kept < 0, a misaligned or short workspace;
 * PTB_EUNSUPPORTED for a selection set of 2^31 or more elements. */
#define PTB_HARDCE_TOPK 0
#define PTB_HARDCE_OHEM 1
int64_t ptb_hardce_workspace_bytes(int dense, int B, int C, int64_t S, int per_sample);
int ptb_hardce_fwd(const float* logits, const int64_t* labels, const float* dense, int B, int C, int64_t S, int has_ignore,
                   int64_t ignore_label, float ignore_value, int per_sample, int rule, double k_percent, float t0, int64_t min_kept,
                   float* map, void* workspace, int64_t workspace_bytes, float* loss, float* threshold, int64_t* kept, float* inv_kept,
                   void* select, int* error_flag, ptb_stream_t stream);
int ptb_hardce_bwd(const float* logits, const int64_t* labels, const float* dense, const float* map, int B, int C, int64_t S,
                   int per_sample, const float* coef, const void* select, float* grad, ptb_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* PTB_HIP_H */
