/* amt_hip.h -- C ABI of libamt_hip.so: the MI355X (gfx950) implementation of the
 * arcadia-microscopy-tools per-image preprocessing + segmentation + region-props hot path.
 *
 * Nothing native exists upstream: the reference (pure Python) reaches its arithmetic through
 * scikit-image / scipy.ndimage / numpy calls.  Each entry point below therefore cites the
 * REFERENCE CALL SITE it serves (R/ = src/arcadia_microscopy_tools/) and the scikit-image /
 * scipy function whose result it reproduces (SK/ = skimage 0.18.3 source, SP/ = scipy.ndimage).
 * INTEGRATION.md shows the ctypes stubs a maintainer of the reference would add.
 *
 * Conventions
 *   - every image argument is a DEVICE pointer to a batch of `nplanes` C-contiguous (H, W)
 *     planes of the stated element type; planes are independent (one per FOV-channel);
 *   - functions enqueue work on the context's HIP stream and return without synchronising
 *     unless stated; amt_sync() waits for the stream;
 *   - return value: 0 on success, a negative AMT_E* code otherwise; amt_last_error() returns a
 *     thread-local message for the last failure on the calling thread;
 *   - a context is not thread-safe; use one context per host thread (they are cheap), which
 *     makes the library re-entrant for Pipeline(parallel=True) (R/pipeline.py:145-146);
 *   - STREAMS: every amt_* call runs on the stream of the context it is GIVEN -- never on the stream that
 *     produced its operands.  Memory written through context A may be read through context B only after B's
 *     stream has been ordered behind A's: amt_stream_wait(B, A) (everything A was given so far), or
 *     amt_event_record(A, ev) + amt_event_wait(B, ev) (exactly up to the record), or amt_sync(A).  Nothing in the
 *     library checks this (pointers carry no owner); a binding that keeps arrays with their context should refuse
 *     mixed-context calls, as the Python binding does for `out=` (tests/test_gpu_api.py::test_stream_rule_at_the_boundary).
 *     Host memory handed to amt_memcpy_h2d / amt_memcpy_d2h must stay valid until the stream has passed the copy.
 *   - ALIASING: inputs may overlap inputs (amt_subtract(a, a, ...), a RELATE companion that is `labels` itself).  An
 *     output -- every non-const device pointer: results, caller-owned scratch, persistent in/out planes, lists, counts --
 *     must not overlap any other operand of the call, not even in part; the byte range of an operand follows from the
 *     arguments (strides, paddings and rectangles included).  The one exception is a pair an entry point declares IN PLACE
 *     below: it may coincide exactly -- same start, same byte length, same element size -- and every other overlap of that
 *     pair (a plane further, 8 bytes further) is refused too.  A refusal is AMT_EINVAL with a message that names the entry
 *     point and both operands ("... must not alias ..."); it comes before the context is touched and before anything is
 *     reserved or launched, so a refused call has written nothing.  The verdict of a pair never depends on which kernel
 *     the arguments select.  In place today: amt_sub_clip0_f64, amt_add_scalar_f64, amt_rescale (float64 input),
 *     amt_subtract (out with a, with b or with both), amt_clear_border, amt_relabel_sequential, amt_clear_border_relabel and
 *     amt_keep_labels, each `out` with `in`.  The output of amt_contours_emit / amt_borders_emit has a length only the
 *     device knows: its first point is checked.
 */
#ifndef AMT_HIP_H
#define AMT_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AMT_OK 0
#define AMT_EINVAL (-1)   /* bad argument */
#define AMT_EHIP (-2)     /* HIP runtime error */
#define AMT_ENOMEM (-3)   /* device allocation failed */
#define AMT_ENODEV (-4)   /* no usable gfx950 device */
#define AMT_ECAPACITY (-5)/* a caller-provided capacity was too small (see amt_last_error) */

/* element types */
#define AMT_U8 0
#define AMT_U16 1
#define AMT_I32 2
#define AMT_F64 3
#define AMT_I64 4
#define AMT_F32 5

/* scipy.ndimage boundary modes */
#define AMT_MODE_NEAREST 0
#define AMT_MODE_REFLECT 1  /* half-sample symmetric  d c b a | a b c d | d c b a */
#define AMT_MODE_MIRROR 2   /* whole-sample symmetric d c b | a b c d | c b a     */
#define AMT_MODE_CONSTANT 3
#define AMT_MODE_WRAP 4

typedef struct amt_ctx amt_ctx;

/* ---- context, memory, stream ------------------------------------------------------------- */
int amt_device_count(void);
int amt_ctx_create(int device, amt_ctx** out);
/* Share an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); 0 = null stream. */
int amt_ctx_create_on_stream(int device, void* hip_stream, amt_ctx** out);
int amt_ctx_destroy(amt_ctx* ctx);
/* Whether independent kernels inside one call (the watershed's flood classes) run on the context's auxiliary streams
 * (default 1; AMT_FORK=0 changes the default).  Hosts that drive several contexts concurrently switch it off. */
int amt_ctx_set_fork(amt_ctx* ctx, int enable);
/* The context's hipStream_t (e.g. to wrap it in torch.cuda.ExternalStream for an RCCL collective). */
int amt_ctx_stream(amt_ctx* ctx, void** hip_stream);
const char* amt_last_error(void);
const char* amt_version(void);
int amt_device_name(amt_ctx* ctx, char* buf, int buflen);
int amt_malloc(amt_ctx* ctx, size_t bytes, void** dptr);
int amt_free(amt_ctx* ctx, void* dptr);
int amt_memcpy_h2d(amt_ctx* ctx, void* dst, const void* src, size_t bytes); /* async on ctx stream */
int amt_memcpy_d2h(amt_ctx* ctx, void* dst, const void* src, size_t bytes); /* async; amt_sync before reading */
int amt_memcpy_d2d(amt_ctx* ctx, void* dst, const void* src, size_t bytes);
int amt_memset(amt_ctx* ctx, void* dst, int value, size_t bytes);
int amt_sync(amt_ctx* ctx);
/* Diagnostic (AMT_DEBUG_POISON=1): synchronises the stream, then scans the padding behind every scratch buffer of the
 * last call that reserved scratch, and the arena beyond that reservation, for bytes other than the 0xCD the reservation
 * left there.  *slot = -1 when they are clean, when poisoning is off or before the first reservation; else the buffer
 * (in declaration order) whose padding holds the first such byte -- the number of buffers stands for the arena's tail --
 * and *offset = that byte's offset into the arena. */
int amt_debug_scratch_check(amt_ctx* ctx, int* slot, uint64_t* offset);
/* Order `ctx`'s stream after everything enqueued so far on `other`'s stream (same device), without
 * blocking the host: joins batch parts processed on separate streams before a collective. */
int amt_stream_wait(amt_ctx* ctx, amt_ctx* other);
/* Events: amt_event_record marks a point on ctx's stream; amt_event_wait orders what is enqueued next on ANOTHER
 * context's stream after that point (not after everything the recording stream was given later).  Used by the
 * plate's staging ring: a block is rewritten only after the pack kernel that read it (plate.PlateTables). */
int amt_event_create(amt_ctx* ctx, void** event);
int amt_event_record(amt_ctx* ctx, void* event);
int amt_event_wait(amt_ctx* ctx, void* event);
int amt_event_sync(amt_ctx* ctx, void* event); /* host waits for the last record */
int amt_event_destroy(amt_ctx* ctx, void* event);
/* pinned host staging buffers for the FOV feeder */
int amt_host_alloc(size_t bytes, void** hptr);
int amt_host_free(void* hptr);
/* host memcpy with streaming stores, for filling a staging block the DMA engine reads next (thread-safe, no GPU call) */
int amt_host_copy(void* dst, const void* src, size_t bytes);
/* host helpers of the constructor checks and the label upload of SegmentationMask (R/masks.py:169-176: "non-negative",
   "contains no cells"): extrema of an integer array in one call -> out[2] = {min, max}; int64 -> int32 narrowing into a
   staging block with the source extrema from the same pass (minmax may be NULL) */
int amt_host_minmax_int(const void* src, int itemsize, int is_signed, size_t n, int64_t* out);
int amt_host_narrow_i64_i32(int32_t* dst, const int64_t* src, size_t n, int64_t* minmax);
/* HIP-event timing on the context's stream (bench.py roofline: kernel time measured live) */
int amt_timer_create(amt_ctx* ctx, void** timer);
int amt_timer_start(amt_ctx* ctx, void* timer);
int amt_timer_stop(amt_ctx* ctx, void* timer);
int amt_timer_elapsed_ms(amt_ctx* ctx, void* timer, float* ms); /* synchronises on the stop event */
int amt_timer_destroy(amt_ctx* ctx, void* timer);

/* ---- channel access: R/microscopy.py:241-282 (get_channel_intensities) --------------------- */
/* (C,Y,X) stacks are channel-major, so a channel is a pointer offset; ND2 frames are (Y,X,C)
 * interleaved: this de-interleaves nplanes frames into (C,Y,X). */
int amt_deinterleave_u16(amt_ctx* ctx, const uint16_t* yxc, uint16_t* cyx, int nplanes, int H, int W, int C);

/* ---- filters: R/operations.py:91 (difference_of_gaussians), SK/filters/_gaussian.py,
 *      SP/_filters.py:226-236,314-430 (gaussian_filter1d -> correlate1d) ------------------------ */
/* Separable symmetric correlation, axis 0 then axis 1, float64 accumulate in scipy's order
 * (centre tap, then pairs outermost->innermost); `weights` = HOST pointer to 2*radius+1 doubles as
 * scipy builds them (computed by the caller with numpy so that np.exp rounding is shared).
 * in_dtype AMT_U16 (scaled by `scale`, 1/65535 for img_as_float) or AMT_F64 (scale ignored if 1).
 * in_plane_stride = elements between consecutive INPUT planes (0 = H*W); C*H*W filters one channel of
 * every (C,Y,X) field of view of a batch in a single launch.  Output planes are always contiguous.
 * minmax_dev (nullable) receives [min, max] of every OUTPUT plane (2 doubles per plane), folded in while the
 * result is written -- hand it to amt_threshold_value to spare Otsu a full re-read of the image. */
int amt_gaussian(amt_ctx* ctx, const void* in, int in_dtype, double scale, double* out, int nplanes, int H, int W,
                 const double* weights, int radius, int mode, double cval, size_t in_plane_stride,
                 double* minmax_dev);
/* threshold_otsu(gaussian(in)) per plane WITHOUT materialising the float64 image -- the first three calls of the
 * nuclei recipes (ski.filters.gaussian -> ski.filters.threshold_otsu -> `>`; SURVEY.md A.7/A.8, reached through
 * R/pipeline.py:25-45).  uint16 input, fused radii (1..12), aligned rows: ask amt_gaussian_otsu_codes_supported first.
 * Outputs (all caller-owned): minmax_dev[2 n] = range of the smoothed plane, hist_dev[256 n] = np.histogram counts,
 * thr_dev[n] = the Otsu threshold (bit-identical to amt_gaussian + amt_threshold_value), codes[n H W] = uint16 code
 * per pixel with   gaussian(in) > thr  <=>  code > thr_code_dev[plane]   exactly, so amt_threshold_gt /
 * amt_threshold_open_close on (codes, AMT_U16, thr_code_dev) produce the mask of the separate operators.
 * prefix (nullable, caller-owned, n H W words, 16-byte aligned): scratch plane for the single-pass form -- ONE Gaussian
 * pass stores the upper 32 bits of every float64 sample there and a streaming pass derives histogram and codes from
 * them, recomputing exactly the few samples the 32 bits leave undecided (R/pipeline.py:25-45 batches: fewer bytes and
 * no second Gaussian).  Null, scale <= 0 or a negative weight: two Gaussian passes over the input.  The outputs are
 * the same bit for bit either way. */
int amt_gaussian_otsu_codes_supported(int H, int W, int radius, int mode, size_t in_plane_stride);
int amt_gaussian_otsu_codes(amt_ctx* ctx, const uint16_t* in, double scale, int nplanes, int H, int W,
                            const double* weights, int radius, int mode, size_t in_plane_stride, double* minmax_dev,
                            uint32_t* hist_dev, double* thr_dev, double* thr_code_dev, uint16_t* codes,
                            uint32_t* prefix);
/* out = G(w_lo) - G(w_hi) of the same converted input (SK/filters/_gaussian.py:284-290). */
/* One leading axis of an n-D Gaussian (skimage filters EVERY axis of an n-D image, leading axes first,
 * SP/_filters.py:423-427): the array is nplanes x L x inner, the 1-D filter runs along L; out is float64. */
int amt_convolve_axis0(amt_ctx* ctx, const void* in, int in_dtype, double scale, double* out, int nplanes, int L, int inner,
                       const double* weights, int radius, int mode, double cval);
int amt_dog(amt_ctx* ctx, const void* in, int in_dtype, double scale, double* out, int nplanes, int H, int W,
            const double* w_lo, int r_lo, const double* w_hi, int r_hi, int mode, double cval);

/* ---- elementwise (R/operations.py:50,97; SK/exposure/exposure.py:405-428) ------------------- */
/* out = max(in - level[plane], 0)  -- np.clip(dog - background_level, 0, None); out may be in (in place) */
int amt_sub_clip0_f64(amt_ctx* ctx, const double* in, const double* level_dev, double* out, int nplanes, size_t n);
/* rescale_intensity with tuple ranges: clip to [imin,imax]; (x-imin)/(imax-imin)*(omax-omin)+omin.
 * range_dev = nplanes x {imin, imax} doubles on the device.  A float64 `in` may be `out` itself (in place). */
int amt_rescale(amt_ctx* ctx, const void* in, int in_dtype, const double* range_dev, double omin, double omax,
                double* out, int nplanes, size_t n);
int amt_convert_u16_f64(amt_ctx* ctx, const uint16_t* in, double scale, double* out, size_t n);
/* out = in + s (threshold_local subtracts its offset this way, SK/filters/thresholding.py:236); out may be in (in place) */
int amt_add_scalar_f64(amt_ctx* ctx, const double* in, double s, double* out, size_t n);

/* ---- statistics: np.percentile (R/operations.py:47,94), histogram (SK/exposure/exposure.py) -- */
/* One 65536-bin histogram per plane (uint32 counts), bin = pixel value. */
int amt_hist_u16(amt_ctx* ctx, const uint16_t* in, uint32_t* hist, int nplanes, size_t n);
/* One bin per integer value lo .. lo + nbins - 1 of an integer-valued float64 image (scikit-image's histogram of
 * integer images, SK/exposure/exposure.py:63-74, for ranges beyond uint16): hist = nplanes x nbins uint32; values outside
 * the range are not counted.  nbins <= 2^28. */
int amt_hist_range_f64(amt_ctx* ctx, const double* in, double lo, int64_t nbins, uint32_t* hist, int nplanes, size_t n);
/* minmax_dev[plane] = {min, max} */
int amt_minmax_f64(amt_ctx* ctx, const double* in, double* minmax_dev, int nplanes, size_t n);
/* np.histogram(x, bins=nbins, range=(min,max)) counts per plane; edges follow np.linspace.  A constant plane counts in bin
 * nbins / 2: numpy widens its range to (v - 0.5, v + 0.5). */
int amt_hist_f64(amt_ctx* ctx, const double* in, const double* minmax_dev, uint32_t* hist, int nbins, int nplanes,
                 size_t n);
/* np.percentile(x, q) (linear): q_host = nq percentiles in [0,100]; out_dev = nplanes x nq doubles.
 * u16: exact order statistics from the histogram; f64: exact radix select. */
int amt_percentile_u16(amt_ctx* ctx, const uint16_t* in, const double* q_host, int nq, double* out_dev, int nplanes,
                       size_t n);
int amt_percentile_f64(amt_ctx* ctx, const double* in, const double* q_host, int nq, double* out_dev, int nplanes,
                       size_t n);

/* out_dev[plane] = {sum(x <= t), count(x <= t), sum(x > t), count(x > t)} with t = thr_dev[plane]; a fixed
 * reduction tree (bit-reproducible).  Feeds threshold_mean / threshold_li on float images
 * (SK/filters/thresholding.py:830, :642-707). */
int amt_masked_sums_f64(amt_ctx* ctx, const double* in, const double* thr_dev, double* out_dev, int nplanes, size_t n);
/* dst[plane] (h x w) = src[plane][top:top+h, left:left+w]; crop_to_center (R/operations.py:100-132). */
/* dst[plane] ((H + 2 py) x (W + 2 px)) = np.pad(src[plane], ((py, py), (px, px)), mode='edge'): what scikit-image does to
 * the image before an opening / closing with an even-sized footprint (SK/morphology/grey.py:84-127). */
int amt_pad_edge(amt_ctx* ctx, const void* src, void* dst, int elem_size, int nplanes, int H, int W, int py, int px);
int amt_copy_rect(amt_ctx* ctx, const void* src, void* dst, int elem_size, int nplanes, int H, int W, int top,
                  int left, int h, int w);

/* ---- thresholds: R/operations.py:186-216 (apply_threshold), SK/filters/thresholding.py ------- */
#define AMT_THR_OTSU 0
#define AMT_THR_YEN 1
#define AMT_THR_ISODATA 2
#define AMT_THR_TRIANGLE 3
#define AMT_THR_MEAN 4
#define AMT_THR_MINIMUM 5
#define AMT_THR_LI 6
/* Global threshold value per plane (thr_dev[plane], float64 -- for integer images the bin centre).
 * status_dev[plane] != 0 flags "no threshold" (threshold_minimum: fewer/more than two maxima).
 * nbins (float64 input; ignored for uint16): 2..4096, refused outside before anything is written.
 * minmax_dev (nullable, float64 input only) = precomputed [min, max] per plane (amt_gaussian / amt_minmax_f64). */
int amt_threshold_value(amt_ctx* ctx, const void* in, int in_dtype, int method, int nbins, double* thr_dev,
                        int32_t* status_dev, int nplanes, size_t n, const double* minmax_dev);
/* out = in > thr[plane] (uint8 0/1) */
int amt_threshold_gt(amt_ctx* ctx, const void* in, int in_dtype, const double* thr_dev, uint8_t* out, int nplanes,
                     size_t n);
/* Niblack (method 0: m - k*s) / Sauvola (method 1: m*(1 + k*(s/r - 1))) threshold image from the mean m and
 * standard deviation s of the window of window_y rows x window_x columns around each pixel (scikit-image's
 * `window_size`, an odd int or a per-axis tuple), mirror padding
 * (SK/filters/thresholding.py:910-964,1026-1027,1083-1087).  uint16 window sums are exact integers. */
int amt_window_threshold(amt_ctx* ctx, const void* in, int in_dtype, double* thr_image, int nplanes, int H, int W,
                         int window_y, int window_x, int method, double k, double r);
/* The same for ONE n-D image whose window spans every axis, as scikit-image's _mean_std does for stacks
 * (SK/filters/thresholding.py:910-964): nlead axes of lead_shape[] in front of (H, W), one odd window per axis. */
int amt_window_threshold_nd(amt_ctx* ctx, const void* in, int in_dtype, double* thr_image, int nlead,
                            const int* lead_shape, const int* lead_window, int H, int W, int window_y, int window_x,
                            int method, double k, double r);
/* out = in > thr_image (per-pixel thresholds: local / niblack / sauvola) */
int amt_threshold_gt_image(amt_ctx* ctx, const void* in, int in_dtype, const double* thr_image, uint8_t* out,
                           size_t n);

/* ---- morphology: SK/morphology/binary.py, grey.py (ImageOperation callables, north_star) ----- */
/* Footprint = HOST uint8 (fh, fw), odd sizes, anchor at the centre.  op:
 *   AMT_MORPH_ERODE   outside the image counts as `border_value` (skimage: 1);
 *   AMT_MORPH_DILATE  outside the image counts as `border_value` (skimage: 0);
 *   AMT_MORPH_OPEN    fused opening = dilate(erode(x)), AMT_MORPH_CLOSE fused closing = erode(dilate(x)), both with
 *                     skimage's border rules (erosion sees 1, dilation 0): border_value is ignored;
 *   AMT_MORPH_FILL_HOLES  scipy.ndimage.binary_fill_holes(in != 0, structure=footprint) per plane.  `in` is a truth
 *                     value (foreground = byte != 0, on every width and alignment); `out` holds 0 / 1 bytes:
 *                     out[p] = 1 iff in[p] != 0 or p lies in a component of the background that contains no pixel of
 *                     the 1-pixel frame (row 0, row H-1, column 0, column W-1).  Background components are 4-connected
 *                     for the 3 x 3 cross and 8-connected for the 3 x 3 all-ones footprint; any other footprint is
 *                     AMT_EINVAL (for exactly these two, scipy's propagation from outside the image equals the
 *                     component rule).  border_value is ignored.  out must not alias in, nor overlap it in part
 *                     (AMT_EINVAL); nplanes == 0 is
 *                     AMT_OK; H * W < 2^31 - 1 as for amt_label.
 *   AMT_MORPH_REMOVE_SMALL_OBJECTS  skimage.morphology.remove_small_objects(in != 0, min_size=s, connectivity) per
 *                     plane: out[p] = 1 iff in[p] != 0 and the foreground component of p has at least s pixels;
 *   AMT_MORPH_REMOVE_SMALL_HOLES    skimage.morphology.remove_small_holes(in != 0, area_threshold=s, connectivity)
 *                     per plane: out[p] = 1 iff in[p] != 0 or the background component of p has fewer than s pixels --
 *                     unlike AMT_MORPH_FILL_HOLES this includes background components that touch the frame.
 *                     For both: `in` is a truth value (byte != 0) and `out` holds 0 / 1 bytes, as for
 *                     AMT_MORPH_FILL_HOLES; the size s travels in border_value, and s < 1 is AMT_EINVAL (a filter that
 *                     can remove nothing is not an operation).  Components are 4-connected for the 3 x 3 cross
 *                     (scikit-image's connectivity=1) and 8-connected for the 3 x 3 all-ones footprint
 *                     (connectivity=2); any other footprint is AMT_EINVAL.  out must not alias in, nor overlap it in
 *                     part (AMT_EINVAL); nplanes == 0 is AMT_OK; H * W < 2^31 - 1.  Sizes are exact pixel counts
 *                     (integer sums), so two runs give identical bytes.
 *   AMT_MORPH_SKELETONIZE  thinning to centre lines per plane, by Zhang and Suen's 1984 rule (the one
 *                     skimage.morphology.skeletonize cites for 2-D input).  `in` is a truth value per pixel (byte != 0),
 *                     positions outside the image are 0, `out` holds 0 / 1 bytes.  The neighbours of p = (y, x):
 *                       P2 = (y-1, x)    P3 = (y-1, x+1)  P4 = (y, x+1)    P5 = (y+1, x+1)
 *                       P6 = (y+1, x)    P7 = (y+1, x-1)  P8 = (y, x-1)    P9 = (y-1, x-1)
 *                     B(p) is the number of set neighbours; A(p) is the number of i for which P_i = 0 and P_{i+1} = 1 in
 *                     the cyclic order P2, P3, ..., P9, P2.
 *                     First sub-iteration: every set p with 2 <= B <= 6, A = 1, P2 * P4 * P6 = 0 and P4 * P6 * P8 = 0 is
 *                     cleared; all such p are cleared together, judged on the plane as it was before the sub-iteration.
 *                     Second sub-iteration: the same with P2 * P4 * P8 = 0 and P2 * P6 * P8 = 0.
 *                     One iteration is the first sub-iteration followed by the second.  The result is the plane after
 *                     the first iteration that clears nothing, or after max_iter iterations if that comes first;
 *                     max_iter travels in border_value, 0 means no limit, a negative value is AMT_EINVAL.  Each plane of
 *                     a batch has its own count, and a plane that has reached its fixed point stays as it is whatever
 *                     the others need.  The fixed point of the rule is unique for a given input, so the bytes depend on
 *                     no schedule and two runs are identical.  scikit-image applies the rule through a literal 256-entry
 *                     table; parity with that table is unpinned offline (no scikit-image was at hand to compare with):
 *                     the tests pin the rule as stated here, nothing more.
 *                     The footprint names the eight-neighbourhood the rule reads: it must be 3 x 3 all-ones, every
 *                     other footprint (the 3 x 3 cross included) is AMT_EINVAL.  out must not alias in, nor overlap it
 *                     in part (AMT_EINVAL); nplanes == 0 is AMT_OK; H * W < 2^31 - 1.
 *                     THIS OP WAITS FOR THE DEVICE (it waits for the device as the reconstruction ops of amt_rank_filter
 *                     do): the number of launches depends on the data, and the call returns once `out` is complete.
 *                     A workgroup owns a tile of AMT_SKELETON_TILE_ROWS rows x AMT_SKELETON_TILE_WORDS 64-pixel words
 *                     and runs up to AMT_SKELETON_BLOCK_SUBITERS sub-iterations per launch (csrc/amt_morph.hip).
 *                     AMT_DEBUG_SKELETONIZE=1 in the environment prints iterations, launches and syncs to stderr.
 *   AMT_MORPH_NEIGHBOR_CLASSES  one pass: out[p] = 0 where in[p] == 0, else 1 + the number of set neighbours under the
 *                     footprint's non-centre cells.  3 x 3 all-ones gives 1..9 (on a skeleton: 1 isolated, 2 an end,
 *                     3 a path pixel, >= 4 a junction), the 3 x 3 cross gives 1..5; any other footprint is AMT_EINVAL.
 *                     Positions outside the image are 0; border_value is ignored; asynchronous like ops 0..3; out must
 *                     not alias in; nplanes == 0 is AMT_OK; H * W < 2^31 - 1.
 * For ops 7 and 8 the refusals that need no device (footprint, max_iter) come before the context is looked at, as the op
 * range does for every op.
 * Any other op (below 0, above 8) is AMT_EINVAL. */
#define AMT_MORPH_ERODE 0
#define AMT_MORPH_DILATE 1
#define AMT_MORPH_OPEN 2
#define AMT_MORPH_CLOSE 3
#define AMT_MORPH_FILL_HOLES 4
#define AMT_MORPH_REMOVE_SMALL_OBJECTS 5
#define AMT_MORPH_REMOVE_SMALL_HOLES 6
#define AMT_MORPH_SKELETONIZE 7
#define AMT_MORPH_NEIGHBOR_CLASSES 8
#define AMT_SKELETON_TILE_ROWS 64
#define AMT_SKELETON_TILE_WORDS 8
#define AMT_SKELETON_BLOCK_SUBITERS 32
int amt_binary_morph(amt_ctx* ctx, const uint8_t* in, uint8_t* out, int nplanes, int H, int W,
                     const uint8_t* footprint, int fh, int fw, int op, int border_value);
/* Otsu threshold of a float64 image (as amt_threshold_value) that also leaves the byte plane of its 256-bin indices
 * and the threshold's bin, for amt_threshold_open_close. */
int amt_otsu_f64_bins(amt_ctx* ctx, const double* in, const double* minmax_dev, double* thr_dev, double* thr_code_dev,
                      uint8_t* bins, int nplanes, size_t n);
/* out = binary_closing(binary_opening(in > thr[plane])) in one packed chain (the mask chain of BASELINE
 * configs[1]/[2]: R/operations.py:216 followed by SK/morphology/binary.py:82-147).
 * bins, thr_code_dev (both NULL or both given; given requires in_dtype AMT_F64): the outputs of amt_otsu_f64_bins for
 * this image -- the comparison then reads the byte plane of bin indices (1 B/px) and the float64 value only inside
 * the threshold's own bin -- identical masks. */
int amt_threshold_open_close(amt_ctx* ctx, const void* in, int in_dtype, const double* thr_dev, uint8_t* out,
                             int nplanes, int H, int W, const uint8_t* footprint, int fh, int fw, const uint8_t* bins,
                             const double* thr_code_dev);
/* grey erosion / dilation / median over a footprint (uint16 or float64 images), scipy boundary `mode`.
 * op: 0 = erosion (min), 1 = dilation (max, footprint already mirrored by the caller), 2 = median
 * minuend (nullable, != out): out = minuend - rank_filter(in), the last step of ndi.white_tophat (R/ callers reach it
 * through skimage.morphology.white_tophat, SK/morphology/grey.py:425) without a separate subtraction pass; uint16 run
 * footprints subtract inside the filter kernel, everything else filters into `out` and subtracts in place.
 *
 * op 3 .. 6: GREY RECONSTRUCTION (skimage.morphology.reconstruction, and the reconstructions behind
 * skimage.morphology.h_maxima / h_minima), on the operands the filter already has.  Common to the four: dtype AMT_U16 or
 * AMT_F64; the footprint is the 3 x 3 cross (4-connected) or 3 x 3 all-ones (8-connected), anything else is AMT_EINVAL;
 * `mode` is ignored -- nothing propagates from outside the image (scikit-image pads with the neutral value);
 * nplanes == 0 is AMT_OK and writes nothing; H * W < 2^31; `out` aliases neither input (AMT_EINVAL), `in` and `minuend`
 * may be the same buffer; NaN is not supported; -0.0 and +0.0 compare equal, and which of the two is stored where they
 * meet is unspecified.  The refusals that need no device (footprint, NULL mask, h, a minuend with op 6, dtype) come
 * before the context is looked at.
 * THESE OPS WAIT FOR THE DEVICE: the number of passes depends on the data, and the call returns once `out` is complete
 * (every other operator of this header stays asynchronous).
 *   AMT_RANK_RECONSTRUCT_DILATION  `in` = the seed, `minuend` = the MASK (required: NULL is AMT_EINVAL), cval ignored.
 *                     out = R, the least image with R >= seed and R = min(mask, max over the footprint of R); equivalently
 *                     R(p) = max over q of min(seed(q), w(p, q)) with w(p, q) the largest, over footprint-connected paths
 *                     from p to q, of the smallest mask value on the path (ends included).  The fixed point is unique:
 *                     the bytes of `out` depend on no schedule, two runs are identical.  Requires seed <= mask
 *                     everywhere: the first pass counts the violations per plane, and a non-zero count is AMT_EINVAL
 *                     with a message naming the first such plane (as scikit-image raises); `out` is then unspecified.
 *   AMT_RANK_RECONSTRUCT_EROSION   the dual (min <-> max); requires seed >= mask.
 *   AMT_RANK_HMAX_RECONSTRUCT      the mask is `in` itself and the seed is never in memory: AMT_U16 seed(p) =
 *                     max(in(p) - h, 0) with h = cval an integer in 1..65535, AMT_F64 seed(p) = in(p) - h (one rounding)
 *                     with h finite and > 0, else AMT_EINVAL before any launch.  out = R by dilation.  `minuend` keeps its
 *                     meaning out = minuend - R: with minuend == in that is the h-dome.
 *   AMT_RANK_HMIN_RECONSTRUCT      seed = min(in + h, 65535) (AMT_U16) or in + h (AMT_F64); out = R by erosion; a non-NULL
 *                     minuend is AMT_EINVAL.
 * The h-maxima / h-minima MASKS built on ops 5 / 6 (the Python layer's h_maxima / h_minima): uint16 -- a pixel is marked
 * iff residue >= h, with residue = in - R for maxima and R - in for minima (scikit-image's rule; with h an integer it
 * is residue > h - 1, which amt_threshold_gt evaluates); float64 -- a pixel is marked iff R(p) == seed(p) exactly, with
 * seed = fl(in -+ h): the same set in exact arithmetic, and it needs no tolerance (scikit-image subtracts a resolution
 * term that differs between versions).
 * A workgroup owns one tile of AMT_RECONSTRUCT_TILE_H_* x AMT_RECONSTRUCT_TILE_W_* pixels per round (csrc/
 * amt_reconstruct.hip); planes that cross tile seams need several rounds.
 *
 * op 8 and 9: PER-CELL SKELETONS of int32 label planes (op 7 is not an op of this call).  Common to the two: dtype must be
 * AMT_I32; `in` is nplanes x H x W labels, where every non-zero int32 value is a label, negative ones included -- only
 * equality is looked at; the footprint must be 3 x 3 all-ones (it names the eight-neighbourhood, as for
 * AMT_MORPH_SKELETONIZE of amt_binary_morph; every other footprint, the 3 x 3 cross included, is AMT_EINVAL); `minuend`
 * must be NULL and cval is ignored; H * W < 2^31 - 1 and nplanes <= 65535; nplanes == 0 is AMT_OK and writes nothing.
 * The refusals that need no device (dtype, footprint, a negative `mode`, a non-NULL minuend, the plane size) come before
 * the context is looked at.  `out` must not alias `in`, nor overlap it in part (AMT_EINVAL).
 *   AMT_RANK_LABEL_SKELETON  thinning of every label to its centre lines.  The rule is the one of AMT_MORPH_SKELETONIZE
 *                     with one change: for a pixel p with labels[p] = l != 0, P_i = 1 iff the neighbour lies inside the
 *                     image and carries the same label l; a pixel with labels[p] == 0 is never set.  B, A, the two
 *                     sub-iterations, "judged on the plane as it was before the sub-iteration", the iteration count and
 *                     max_iter are word for word those of AMT_MORPH_SKELETONIZE.  By induction over the sub-iterations
 *                     the result is exactly the union of the skeletons each label would get alone in its plane -- a
 *                     pixel of another label looks like background, which is what it would be there -- so touching
 *                     cells get a skeleton each, and there is no limit on a label's size.
 *                     out[p] = labels[p] where p is on the skeleton of its label, 0 elsewhere (an int32 plane like
 *                     `in`).  `mode` carries max_iter: 0 means to the fixed point, a negative value is AMT_EINVAL.
 *                     Each plane of a batch has its own iteration count.  THIS OP WAITS FOR THE DEVICE (it
 *                     waits for the device as the reconstruction ops and AMT_MORPH_SKELETONIZE do); AMT_DEBUG_SKELETONIZE=1
 *                     in the environment prints iterations, launches and syncs to stderr ("amt label_skeleton: ...").
 *                     The kernel is the bit-sliced tile kernel of AMT_MORPH_SKELETONIZE on the mask labels != 0, with four
 *                     constant link bit planes beside it (same label towards E, S, SE, SW): a tile of
 *                     AMT_LABEL_SKELETON_TILE_ROWS rows x AMT_LABEL_SKELETON_TILE_WORDS 64-pixel words and up to
 *                     AMT_LABEL_SKELETON_BLOCK_SUBITERS sub-iterations per launch (csrc/amt_morph.hip).  Parity with
 *                     scikit-image's skeletonize per label, or with CellProfiler's MeasureObjectSkeleton, is
 *                     unpinned offline, as for AMT_MORPH_SKELETONIZE: the tests pin the rule as stated here.
 *   AMT_RANK_LABEL_CENSUS    the census of the same-label pixel graph of a label plane -- any label plane; the Python
 *                     layer feeds it the result of AMT_RANK_LABEL_SKELETON.  `mode` carries max_label (>= 0; 0 writes
 *                     nothing, negative is AMT_EINVAL); `out` is nplanes x max_label x AMT_LCEN_NCOLS INT32, row l - 1 for
 *                     label l.  Values outside 1..max_label own no row; they still differ from every neighbour.  With
 *                     deg(p) the number of the eight neighbours that carry labels[p], the columns of label l:
 *                       AMT_LCEN_PIXELS      pixels carrying l
 *                       AMT_LCEN_ISOLATED    of these, deg == 0
 *                       AMT_LCEN_ENDS        deg == 1
 *                       AMT_LCEN_PATH        deg == 2
 *                       AMT_LCEN_JUNCTIONS   deg >= 3 (the classes of AMT_MORPH_NEIGHBOR_CLASSES minus one, and like them a
 *                                            property of pixels, not of graph nodes)
 *                       AMT_LCEN_ORTH_LINKS  unordered pairs {p, p+(0,1)} and {p, p+(1,0)} with both ends l
 *                       AMT_LCEN_DIAG_LINKS  pairs {p, p+(1,1)} with both ends l and neither p+(0,1) nor p+(1,0) carrying
 *                                            l, and pairs {p, p+(1,-1)} with neither p+(0,-1) nor p+(1,0) carrying l: a
 *                                            diagonal link that an orthogonal pair already bridges is not counted, so a
 *                                            staircase is not measured twice (length = ORTH_LINKS + sqrt(2) * DIAG_LINKS)
 *                     A label absent from its plane gives seven zeros.  The counts are exact integers made without global
 *                     atomics, so two runs give identical bytes.  Asynchronous.  The table must not overlap `in`.
 *
 * op 10 .. 14: Z-STACKS (csrc/amt_zstack.hip).  Common to the five: `in` is nplanes x Z x H x W, stacks back to back and
 * the planes of one stack back to back; `mode` carries Z, 1..65535, anything else is AMT_EINVAL; `dtype` is the dtype of
 * `in`; nplanes == 0 is AMT_OK and writes nothing; `out` must not overlap `in` or `minuend`, not even in part
 * (AMT_EINVAL); H * W < 2^31, and every offset is 64-bit, so Z * H * W of one stack may pass 2^31 elements.  The refusals
 * that need no device (dtype, Z, the footprint, a minuend where none is allowed or a missing one, cval of op 10, the
 * sizes) come before the context is looked at.  The five ops are asynchronous and reserve no scratch.
 *   AMT_RANK_Z_PROJECT      dtype AMT_U8, AMT_U16 or AMT_F64.  cval selects the projection: 0 = max, 1 = min, 2 = mean,
 *                     anything else is AMT_EINVAL.  `out` is nplanes x H x W: max / min in the dtype of `in`, mean in
 *                     FLOAT64.  The integer mean is the exact integer sum over z divided once by Z; the float64 mean is
 *                     the sum taken in the order z = 0, 1, ..., Z - 1 divided once by Z: both equal numpy's
 *                     mean(stack, axis=0) bit for bit (numpy reduces a leading axis plane by plane).  NaN in float64
 *                     input is unsupported.  The footprint is ignored; `minuend` must be NULL.
 *   AMT_RANK_Z_FOCUS_SUMS   dtype AMT_U8 or AMT_U16 (AMT_F64 is AMT_EINVAL: focus is judged on raw data).  `out` is
 *                     nplanes x Z x AMT_ZF_NCOLS 64-bit integers, one row per plane P:
 *                       AMT_ZF_SUM        sum of P
 *                       AMT_ZF_SUMSQ      sum of P^2
 *                       AMT_ZF_LAP_SUMSQ  sum of L^2, L as defined under AMT_RANK_Z_FOCUS_INDEX
 *                       AMT_ZF_BRENNER    sum over x + 2 < W of (P(y, x + 2) - P(y, x))^2
 *                     H * W <= 2^27, else AMT_EINVAL: with uint16 L^2 <= 262140^2 < 2^36, and 2^27 of them still fit 64
 *                     bits.  The sums are integers (workgroup totals added with 64-bit integer atomics), so their bytes
 *                     depend on no order.  The footprint is ignored; `minuend` must be NULL.
 *   AMT_RANK_Z_FOCUS_INDEX  dtype AMT_U8 or AMT_U16.  The footprint must be (2r+1) x (2r+1) with every cell non-zero, r in
 *                     0..AMT_ZSTACK_MAX_RADIUS; anything else is AMT_EINVAL.  `out` is nplanes x H x W UINT16.  With P_z
 *                     plane z of a stack:
 *                       L_z(y, x) = 4 P(y, x) - P(y-1, x) - P(y+1, x) - P(y, x-1) - P(y, x+1), coordinates clamped to the
 *                                   image (edge replication);
 *                       E_z(y, x) = sum of L_z(y+dy, x+dx)^2 over |dy|, |dx| <= r with (y+dy, x+dx) inside the image
 *                                   (outside counts 0);
 *                       out(y, x) = the smallest z at which E_z(y, x) is largest.
 *                     E < 961 * 2^36 < 2^46: the arithmetic is exact 64-bit integers, no float appears, and two runs
 *                     give identical bytes.  `minuend` must be NULL.  This focus rule is this library's own: parity
 *                     with CellProfiler's or ImageJ's stack focusers is unpinned offline.
 *   AMT_RANK_Z_FOCUS_STACK  the operands and the rule of AMT_RANK_Z_FOCUS_INDEX; `out` is nplanes x H x W of the dtype of
 *                     `in` and holds in[index(y, x), y, x].  The index map never reaches memory.
 *   AMT_RANK_Z_TAKE         dtype AMT_U8, AMT_U16 or AMT_F64.  `minuend` is an nplanes x H x W UINT16 index map and is
 *                     required (NULL is AMT_EINVAL).  out(y, x) = in[min(index(y, x), Z - 1), y, x] in the dtype of
 *                     `in`: an index past the stack is clamped, since refusing it would need a wait for the device.
 *                     The footprint is ignored.
 * Ops 12 / 13: a workgroup owns one tile of AMT_ZSTACK_TILE_H x AMT_ZSTACK_TILE_W output pixels and loops over z; each
 * stack is read once plus a halo of r + 1 pixels, and nothing but `out` is written.
 *
 * op 15 .. 18: SPOT DETECTION (csrc/amt_spots.hip).  Common to the four: `in` is nplanes x H x W of `dtype`; nplanes == 0
 * is AMT_OK and writes nothing; H * W < 2^31; `out` must not overlap `in` or `minuend`, not even in part (AMT_EINVAL;
 * buffers that only touch are accepted).  The refusals that need no device (dtype, the footprint, `mode`, a minuend where
 * none is allowed or a missing one, the sizes) come before the context is looked at.  The four ops are asynchronous and
 * use no global float atomics: two runs give identical bytes.  A LIST OF SPOTS of capacity c is nplanes x (c + 1) INT32,
 * per plane: entry 0 the true number of spots, also when it exceeds c; entries 1 .. min(count, c) their raster indices
 * y * W + x, ascending; every later entry -1.
 *   AMT_RANK_LOCAL_MAXIMA   dtype AMT_U16 or AMT_F64.  `out` is nplanes x H x W UINT8, 0 or 1.  The footprint must be
 *                     (2r+1) x (2r+1) with every cell non-zero, r in 1..AMT_SPOT_MAX_RADIUS; `mode` is the border width
 *                     b >= 0; anything else is AMT_EINVAL.  cval is the threshold t; `minuend` is nullable and, when
 *                     given, holds nplanes FLOAT64 thresholds, one per plane, used instead of cval.  The rule is this
 *                     library's own.  Pixel p is marked iff all of these hold:
 *                       in(p) > t;
 *                       in(p) >= in(q) for every q inside the image with Chebyshev distance <= r from p;
 *                       in(p) > in(q), strictly, for those q that precede p in raster order: rows above, and the same
 *                                   row to the left;
 *                       p lies at least b pixels from every image edge.
 *                     The border test is applied last: a plateau whose first pixel lies in the border yields nothing
 *                     there.  Consequences: any two marked pixels are more than r apart (Chebyshev) -- if p and q are
 *                     both marked and within r then in(p) = in(q), and the later one fails the strict test; so a plane
 *                     holds at most ceil(H / (r+1)) * ceil(W / (r+1)) marks; a constant ridge or plateau yields one mark,
 *                     at its first pixel in raster order.  NaN is unsupported; -0.0 equals +0.0.  Parity with
 *                     skimage.feature.peak_local_max on plateaus is unpinned offline (scikit-image thins plateau
 *                     candidates in a second pass); the spacing guarantee is the same.  A workgroup owns one tile of
 *                     AMT_SPOT_TILE_H x AMT_SPOT_TILE_W output pixels with a halo of r in LDS and takes the window
 *                     maximum separably (rows, then columns): a plane is read once plus halo.
 *   AMT_RANK_MASK_LIST      dtype AMT_U8: `in` is any mask, non-zero meaning set.  `mode` is the capacity c >= 1.  The
 *                     footprint is ignored; `minuend` must be NULL.  `out` is the list of the set pixels, capacity c:
 *                     np.flatnonzero per plane, truncated.  The order is the raster order, so the bytes depend on no
 *                     schedule (per-row counts, one exclusive scan per plane, a wave per row placing its entries).
 *   AMT_RANK_SPOT_MEASURE   dtype AMT_U16 or AMT_F64.  `minuend` is a list of spots and is required (NULL is
 *                     AMT_EINVAL); `mode` is its capacity c.  The footprint must be (2k+1) x (2k+1) with every cell
 *                     non-zero, k in 0..AMT_SPOT_MAX_RADIUS.  `out` is nplanes x c x AMT_SPOT_NCOLS FLOAT64.  The row for
 *                     list entry j at (y, x), with a = `in` as float64:
 *                       AMT_SPOT_VALUE     a(y, x)
 *                       AMT_SPOT_DY / _DX  the vertex of the parabola through the three samples along the axis: 0 on the
 *                                          first or last row (column) of the image; otherwise with
 *                                          den = (a- - a0) + (a+ - a0): 0 when den >= 0, else (0.5 * (a- - a+)) / den
 *                                          clamped to [-0.5, 0.5].  The operations run in exactly this order, each rounded
 *                                          once; no multiply feeds an add, so contraction cannot change a bit.
 *                       AMT_SPOT_SUM / _N  sum and count of `in` over |dy|, |dx| <= k, clipped to the image
 *                       AMT_SPOT_RING_SUM / _RING_N  the same over Chebyshev distance k+1 .. k+2, clipped: the local
 *                                          background frame
 *                     uint16 sums are exact integers converted once.  float64 sums run in one fixed order: the window
 *                     (2k+5)^2 is numbered row by row, lane l of a wave adds its elements l, l + 64, ... in that order,
 *                     and the 64 partial sums are combined by a butterfly (distance 32, 16, ... 1).  Rows past
 *                     min(count, c), and rows of -1 entries (or of an index outside the plane), are NaN throughout.
 *   AMT_RANK_TAKE_AT        dtype AMT_U8, AMT_U16, AMT_I32 or AMT_F64.  `minuend` is a list of spots and is required;
 *                     `mode` is its capacity c.  The footprint is ignored.  `out` is nplanes x c of the dtype of `in`:
 *                     out[i][j] = in[i] at list entry j, 0 past the count (labels under spots are taken this way).
 */
#define AMT_RANK_RECONSTRUCT_DILATION 3
#define AMT_RANK_RECONSTRUCT_EROSION  4
#define AMT_RANK_HMAX_RECONSTRUCT     5
#define AMT_RANK_HMIN_RECONSTRUCT     6
#define AMT_RANK_LABEL_SKELETON 8
#define AMT_RANK_LABEL_CENSUS 9
#define AMT_RANK_Z_PROJECT 10
#define AMT_RANK_Z_FOCUS_SUMS 11
#define AMT_RANK_Z_FOCUS_INDEX 12
#define AMT_RANK_Z_FOCUS_STACK 13
#define AMT_RANK_Z_TAKE 14
#define AMT_RANK_LOCAL_MAXIMA 15
#define AMT_RANK_MASK_LIST 16
#define AMT_RANK_SPOT_MEASURE 17
#define AMT_RANK_TAKE_AT 18
#define AMT_SPOT_VALUE 0
#define AMT_SPOT_DY 1
#define AMT_SPOT_DX 2
#define AMT_SPOT_SUM 3
#define AMT_SPOT_N 4
#define AMT_SPOT_RING_SUM 5
#define AMT_SPOT_RING_N 6
#define AMT_SPOT_NCOLS 7
#define AMT_SPOT_TILE_H 64
#define AMT_SPOT_TILE_W 64
#define AMT_SPOT_MAX_RADIUS 15
#define AMT_ZF_SUM 0
#define AMT_ZF_SUMSQ 1
#define AMT_ZF_LAP_SUMSQ 2
#define AMT_ZF_BRENNER 3
#define AMT_ZF_NCOLS 4
#define AMT_ZSTACK_TILE_H 64
#define AMT_ZSTACK_TILE_W 64
#define AMT_ZSTACK_MAX_RADIUS 15
#define AMT_LABEL_SKELETON_TILE_ROWS 64
#define AMT_LABEL_SKELETON_TILE_WORDS 8
#define AMT_LABEL_SKELETON_BLOCK_SUBITERS 32
#define AMT_LCEN_PIXELS 0
#define AMT_LCEN_ISOLATED 1
#define AMT_LCEN_ENDS 2
#define AMT_LCEN_PATH 3
#define AMT_LCEN_JUNCTIONS 4
#define AMT_LCEN_ORTH_LINKS 5
#define AMT_LCEN_DIAG_LINKS 6
#define AMT_LCEN_NCOLS 7
#define AMT_RECONSTRUCT_TILE_H_U16 64
#define AMT_RECONSTRUCT_TILE_W_U16 128
#define AMT_RECONSTRUCT_TILE_H_F64 32
#define AMT_RECONSTRUCT_TILE_W_F64 64
int amt_rank_filter(amt_ctx* ctx, const void* in, void* out, int dtype, int nplanes, int H, int W,
                    const uint8_t* footprint, int fh, int fw, int op, int mode, double cval, const void* minuend);
/* out = a - b (same dtype; white_tophat = image - opening); out may be a, b or both (in place) */
int amt_subtract(amt_ctx* ctx, const void* a, const void* b, void* out, int dtype, size_t n);

/* ---- labelling: R/masks.py:56-65 (clear_border, label, relabel_sequential) ------------------- */
/* Connected components of equal-valued non-zero pixels (uint8 mask or int32 label image),
 * connectivity 1 (4-conn) or 2 (8-conn, skimage default in 2-D); labels 1..K per plane in raster
 * order of each component's first pixel; count_dev[plane] = K. */
int amt_label(amt_ctx* ctx, const void* in, int in_dtype, int32_t* out, int32_t* count_dev, int nplanes, int H, int W,
              int connectivity);
/* amt_label for a uint8 plane batch that is a TRUTH VALUE (foreground = byte != 0; what skimage.measure.label does with
 * a bool array, R/masks.py:63 on a mask): same labels as amt_label on the 0 / 1 image, without the launches that stand by
 * for "other byte values" (planes whose width is a multiple of 16; others take amt_label's path and REQUIRE 0 / 1 bytes). */
int amt_label_mask(amt_ctx* ctx, const uint8_t* mask, int32_t* out, int32_t* count_dev, int nplanes, int H, int W,
                   int connectivity);
/* Same result as amt_label for uint8 masks with at most `capacity` foreground pixels per plane (e.g. the EDT
 * peak markers): foreground is compacted in raster order and labelled on the compact list.  If a plane has
 * more foreground pixels than `capacity`, count_dev[plane] = -1 and that plane's labels are invalid.
 * keep_list, keep_count (both NULL or both given) serve callers that label into the SAME plane batch again and again (a
 * batch driver's marker planes): `out` must be zero except at the pixels listed in
 * keep_list[plane * capacity ...][0 .. keep_count[plane]) -- the state this function leaves behind; start from a
 * zeroed `out` and zeroed keep_count.  Only those pixels are cleared (no full-plane memset), and the lists are replaced
 * by this call's foreground pixels.  Without them `out` is cleared whole. */
int amt_label_sparse(amt_ctx* ctx, const uint8_t* in, int32_t* out, int32_t* count_dev, int nplanes, int H, int W,
                     int connectivity, int capacity, int32_t* keep_list, int32_t* keep_count);
/* skimage.segmentation.clear_border(labels) with buffer_size=0: zero every 8-connected component of
 * equal-valued pixels that touches the 1-px frame; other pixels keep their value.  out may be in (in place). */
int amt_clear_border(amt_ctx* ctx, const int32_t* in, int32_t* out, int nplanes, int H, int W);
/* relabel_sequential: surviving labels -> 1..K in ascending order of the old label; count_dev = K.
 * max_label = upper bound of label values in `in` (any plane).  out may be in (in place). */
int amt_relabel_sequential(amt_ctx* ctx, const int32_t* in, int32_t* out, int32_t* count_dev, int nplanes, size_t n,
                           int max_label);
/* clear_border followed by relabel_sequential (R/masks.py:56,65) in one pass, valid when every label of
 * `in` is a single connected component (outputs of amt_label and amt_watershed_*): a label is removed
 * iff one of its pixels lies on the 1-px frame; survivors -> 1..K in ascending old-label order.
 * nlabels_dev (nullable): the caller vouches that plane p holds exactly the labels 1..nlabels_dev[p] (true for a
 * watershed of a mask from markers numbered 1..K that lie inside the mask); the presence pass is then skipped.
 * out may be in (in place). */
int amt_clear_border_relabel(amt_ctx* ctx, const int32_t* in, int32_t* out, int32_t* count_dev, int nplanes, int H,
                             int W, int max_label, const int32_t* nlabels_dev);
/* np.where(np.isin(labels, keep), labels, 0): keep_dev = nplanes x (max_label+1) uint8 flags; out may be in (in place) */
int amt_keep_labels(amt_ctx* ctx, const int32_t* in, const uint8_t* keep_dev, int32_t* out, int nplanes, size_t n,
                    int max_label);
int amt_cast_i32_i64(amt_ctx* ctx, const int32_t* in, int64_t* out, size_t n);
/* Label planes of other element types: AMT_U8 / AMT_U16 -> AMT_I32 (widened) and AMT_I32 -> AMT_U8 / AMT_U16
 * (narrowed; the caller vouches that the values fit).  Any other pair is refused. */
int amt_cast_labels(amt_ctx* ctx, const void* in, int in_dtype, void* out, int out_dtype, size_t n);
/* skimage.segmentation.expand_labels(label_image, distance) per plane (SK/segmentation/_expand_labels.py:
 * `out[distances <= distance] = label_image[nearest]` on distance_transform_edt(label_image == 0, return_indices=True)).
 * labels = nplanes x H x W non-negative int32; out (another buffer than labels) receives
 *   - the pixel's own label where it has one (0 there when ring != 0, so the annulus comes out of the same pass);
 *   - for a background pixel p with D2(p) <= nmax the label of the nearest labelled pixel, D2 = exact integer squared
 *     Euclidean distance to the nearest labelled pixel; 0 otherwise, and 0 everywhere on a plane without labels.
 * nmax contract: the caller passes nmax = max{n : sqrt(float64(n)) <= distance} (floor(distance^2) corrected by +-1
 * against that very test), so that the integer comparison equals scikit-image's `distances <= distance` for every
 * float distance; nmax < 0 (distance < 0) zeroes the planes, labelled pixels included, as that expression does.
 * Tie rule: when pixels of several labels lie at distance D2(p), the SMALLEST of those labels is written.  scipy's
 * feature transform keeps whichever tied pixel its scan meets first (undocumented); this rule is deterministic and
 * independent of tiling, plane size and batch position.  Untied pixels and the support equal scipy's.
 * Every nmax is exact: searches within 32 rows run from LDS, deeper ones from the packed flags (slower, never wrong). */
int amt_expand_labels(amt_ctx* ctx, const int32_t* labels, int32_t* out, int nplanes, int H, int W, int64_t nmax,
                      int ring);

/* ---- distance transform, markers, watershed (north_star) ------------ */
/* Exact squared Euclidean distance to the nearest zero pixel (int32), and its correctly rounded
 * float64 square root = scipy.ndimage.distance_transform_edt.  Either output may be NULL. */
int amt_edt(amt_ctx* ctx, const uint8_t* mask, int32_t* d2_out, double* edt_out, int nplanes, int H, int W);
/* peaks = (d2 == maximum_filter(d2, (2m+1)^2, constant 0)) & mask & (d2 > 0), border of width m cleared.
 * prev_list, prev_count, prev_status (all NULL, or all given with capacity >= 1; capacity is ignored otherwise):
 * `peaks` is zero except at the pixels listed in prev_list / prev_count (the keep lists amt_label_sparse holds of the
 * previous run's peaks), and only those are cleared -- no full-plane memset.  prev_status = that run's label counts
 * (count_dev of amt_label_sparse): a plane whose count is -1 overflowed its list and is cleared whole.  Start from
 * zeroed planes, zeroed counts and zeroed status. */
int amt_peak_mask(amt_ctx* ctx, const int32_t* d2, const uint8_t* mask, uint8_t* peaks, int nplanes, int H, int W,
                  int min_distance, const int32_t* prev_list, const int32_t* prev_count, int capacity,
                  const int32_t* prev_status);
/* amt_peak_mask followed by amt_label_sparse in one operation, without reading either plane again: the peak search
 * lists the peaks it writes, and one workgroup per plane sorts that list into raster order, joins neighbours
 * (connectivity 1 or 2), numbers the components and writes the markers.  Bit for bit the results of the two calls:
 * `peaks` as the peak mask, and for every plane with at most `capacity` peaks `markers`, count_dev, keep_count and the
 * first keep_count entries of keep_list[plane * capacity ...] (raster order) as the sparse labelling leaves them.  A
 * plane with more peaks reports count_dev = -1 and keep_count = 0 and gets NO markers.
 * keep_list, keep_count (both NULL or both given): with them `peaks`, `markers`, the lists, keep_count and count_dev are
 * the caller's persistent buffers, zeroed once -- count_dev is read as the previous run's status (-1: both planes are
 * cleared whole) before it receives this run's counts, and only the listed pixels are cleared.  Without them both planes
 * are cleared whole.  Lists of up to AMT_PEAK_MARKERS_LDS_TIER peaks are labelled from LDS, longer ones in scratch. */
#define AMT_PEAK_MARKERS_LDS_TIER 4096
int amt_peak_markers(amt_ctx* ctx, const int32_t* d2, const uint8_t* mask, uint8_t* peaks, int32_t* markers,
                     int32_t* count_dev, int nplanes, int H, int W, int min_distance, int connectivity, int capacity,
                     int32_t* keep_list, int32_t* keep_count);
/* Priority flood restricted to `mask` (skimage.segmentation.watershed, no compactness, no watershed line;
 * SURVEY.md A.1).  Priority = (value, insertion age); labels are assigned at push time.
 * `mask` holds 0 / 1 bytes (what a bool array is on the device): scikit-image takes the mask as a truth value, and only
 * amt_watershed_edt_cleared with a marker list, on widths that are a multiple of 16, reads other non-zero bytes that
 * way -- elsewhere differing non-zero byte values would split a region.
 *   amt_watershed_edt : relief = -sqrt(d2) given as the exact integer d2 (bucket queue).  seeds_first = 1 is the
 *                       config-3 recipe (oracle/skops.py:seeded_flood_image): marker pixels are spread first, in
 *                       raster order -- i.e. the relief with every marker pixel lowered to a distinct lowest value;
 *   amt_watershed_f64 : general float64 relief (per-component binary heap).
 * Equal-valued age-0 MARKER pixels: scikit-image orders them by the moves of its single binary heap, which depends
 * on everything else in the image, so such planes cannot be flooded component by component.  tie_policy:
 *   AMT_WS_TIES_EXACT   planes in which two markers of one mask component (with more than one label) tie are
 *                       re-flooded by a sequential emulation of scikit-image's heap: bit-identical, one lane,
 *                       ~seconds per 2048 x 2048 plane.  Untied planes keep the parallel result (also bit-identical).
 *   AMT_WS_TIES_RASTER  ties are broken in raster order (fast; differs from scikit-image in tied planes).
 *   AMT_WS_TIES_REPORT  as RASTER, and ties_dev[plane] = 1 marks every plane whose result may differ.
 * ties_dev (nullable, nplanes ints) receives the per-plane tie flags under every policy.
 * connectivity 1 (4 neighbours) or 2 (8 neighbours, visited N, E, W, S, NW, NE, SW, SE as scikit-image 0.18.3 does;
 * SURVEY.md A.9); connectivity 2 runs the sequential emulation for every plane and requires AMT_WS_TIES_EXACT. */
#define AMT_WS_TIES_EXACT 0
#define AMT_WS_TIES_RASTER 1
#define AMT_WS_TIES_REPORT 2
int amt_watershed_edt(amt_ctx* ctx, const int32_t* d2, const int32_t* markers, const uint8_t* mask, int32_t* out,
                      int nplanes, int H, int W, int seeds_first, int connectivity, int tie_policy, int32_t* ties_dev);
int amt_watershed_f64(amt_ctx* ctx, const double* relief, const int32_t* markers, const uint8_t* mask, int32_t* out,
                      int nplanes, int H, int W, int connectivity, int tie_policy, int32_t* ties_dev);
/* The config-3 tail in one call: amt_watershed_edt(seeds_first = 1, connectivity 1, AMT_WS_TIES_EXACT) followed by
 * amt_clear_border_relabel (R/masks.py:56 + :65 on the watershed of a mask from markers numbered
 * 1..nlabels_dev[plane]; labels that touch the frame are dropped, the rest renumbered 1..count_dev[plane] in ascending
 * order).  Same labels as the two calls, one full-plane write less: the watershed image itself is never materialised --
 * ws_scratch (nplanes x H x W ints) only receives the pixels of flooded components.
 * marker_list, marker_count (both NULL or both given with list_capacity >= 1; list_capacity is ignored otherwise) serve
 * callers that hold the LIST of marker pixels (the keep_list / keep_count amt_label_sparse leaves behind:
 * marker_list[plane * list_capacity ...][0 .. marker_count[plane]) = flat indices of every non-zero pixel of the marker
 * plane): the per-component marker statistics come from the list and the dense statistics pass does not read the
 * marker plane (4 of its 12 bytes per pixel).  A plane whose list is incomplete (count above the capacity) gives
 * undefined labels -- amt_label_sparse reports that plane with count -1.
 * Label boxes.  With a marker list, W % 16 == 0 and 16-byte aligned planes (the path that works from the mask's run
 * tables) the call also leaves the bounding boxes of its final labels with the context.  The per-label entry point --
 * amt_regionprops, amt_regionprops_ext, amt_regionprops_intensity_f64, amt_colocalization, amt_label_bboxes -- that is
 * the DIRECTLY FOLLOWING image operation on the same context and names the same labels_out, nplanes, H, W and max_label
 * takes these boxes and does not read the label planes for them.  Any other operation in between voids them: every
 * entry point that takes device operands, every amt_memcpy_*, amt_memset, amt_malloc, amt_free and amt_sync, and every
 * call through which the context's work becomes visible to another stream or to the host -- amt_stream_wait (on the
 * waiting context AND on the one waited for), amt_event_record, amt_event_wait, amt_event_sync, amt_timer_elapsed_ms.
 * amt_timer_start / amt_timer_stop, amt_last_error, amt_version and amt_device_name do not.  The boxes serve one call,
 * and results are the same either way.  A context on a borrowed stream (amt_ctx_create_on_stream) leaves no boxes: its
 * owner's work runs on that stream between two calls of the library, ordered and unseen.  What remains: between two
 * consecutive calls on a context with its own stream, labels_out can only change through work that races with this
 * call's kernels, or through a caller that takes the raw stream (amt_ctx_stream) and orders or synchronises on it
 * outside the library; such a caller issues any image operation or amt_sync on the context before the per-label call.
 * Every other configuration of the watershed entry points leaves no boxes. */
int amt_watershed_edt_cleared(amt_ctx* ctx, const int32_t* d2, const int32_t* markers, const uint8_t* mask,
                              int32_t* ws_scratch, int32_t* labels_out, int32_t* count_dev, int nplanes, int H, int W,
                              int max_label, const int32_t* nlabels_dev, const int32_t* marker_list,
                              const int32_t* marker_count, int list_capacity);

/* ---- region properties: R/masks.py:286-326 (regionprops_table) ------------------------------- */
/* Morphology columns per label 1..max_label (row = label-1), float64, column order: */
#define AMT_RP_AREA 0
#define AMT_RP_CENTROID_Y 1
#define AMT_RP_CENTROID_X 2
#define AMT_RP_BBOX_Y0 3
#define AMT_RP_BBOX_X0 4
#define AMT_RP_BBOX_Y1 5
#define AMT_RP_BBOX_X1 6
#define AMT_RP_PERIMETER 7
#define AMT_RP_AXIS_MAJOR 8
#define AMT_RP_AXIS_MINOR 9
#define AMT_RP_ECCENTRICITY 10
#define AMT_RP_ORIENTATION 11
#define AMT_RP_AREA_CONVEX 12
#define AMT_RP_SOLIDITY 13
#define AMT_RP_NCOLS 14
/* table_dev (nullable) = nplanes x max_label x AMT_RP_NCOLS doubles.  Labels absent from a plane give area 0.
 * itable_dev (nullable) = intensity columns per label and channel: {mean, max, min, std} (population std, SURVEY.md
 * A.9), nplanes x max_label x C x 4 doubles, from intensity = nplanes x C planes of uint16 (one (C,Y,X) FOV per label
 * plane).  intensity and C >= 1 are given exactly when itable_dev is; at least one table is.  Both tables in one
 * call share the bounding-box pass and the per-label scan: what SegmentationMask.cell_properties needs for a (C,Y,X)
 * field of view (R/masks.py:286-326).
 * This and the other per-label entry points (amt_regionprops_ext, amt_regionprops_intensity_f64, amt_colocalization,
 * amt_label_bboxes) take their bounding boxes from the amt_watershed_edt_cleared call that directly precedes them on
 * the context when it wrote exactly these label planes -- see there for the rule and for what a caller who works on the
 * raw stream owes it; in every other case they read the label planes once for the boxes. */
int amt_regionprops(amt_ctx* ctx, const int32_t* labels, const uint16_t* intensity, int C, double* table_dev,
                    double* itable_dev, int nplanes, int H, int W, int max_label);
/* The same {mean, max, min, std} for float64 intensity images (R/masks.py:178-190, :319-323 accept any 2-D ndarray):
 * two sweeps per label as np.mean / np.std make them; float64 sums, so agreement with numpy is ~1e-15 relative. */
int amt_regionprops_intensity_f64(amt_ctx* ctx, const int32_t* labels, const double* intensity, int C, double* table_dev,
                                  int nplanes, int H, int W, int max_label);
/* Extended region properties (scikit-image 0.25.2 names).  `columns` is an OR of the AMT_RPX_* bits; each bit fills
 * its own columns of the tables below and leaves every other column as it was.
 *   AMT_RPX_EULER_NUMBER       euler_number (8-connected objects, 2x2 configuration counts, Ohser's coefficients)
 *   AMT_RPX_PERIMETER_CROFTON  perimeter_crofton (4 directions; same configuration counts)
 *   AMT_RPX_AREA_FILLED        area_filled (holes = 8-connected components of "not this label" in the bounding box
 *                              that do not touch its edge; other labels inside a hole count)
 *   AMT_RPX_FERET_DIAMETER_MAX feret_diameter_max (from the row extents of the convex image; NaN when the row scratch
 *                              of a plane is exceeded, as for area_convex: the labels' bounding-box heights add up to
 *                              more than H * W, which only labels of several pieces reach.  SegmentationMask measures
 *                              such planes again in groups of labels whose heights fit)
 *   AMT_RPX_CENTROID_LOCAL     centroid_local-0 / -1
 *   AMT_RPX_INERTIA_TENSOR     inertia_tensor-0-0, -0-1, -1-0, -1-1
 *   AMT_RPX_INERTIA_EIGVALS    inertia_tensor_eigvals-0 / -1 (descending)
 *   AMT_RPX_CENTROID_WEIGHTED  centroid_weighted-0 / -1 and centroid_weighted_local-0 / -1 per channel
 * table_dev = nplanes x max_label x AMT_RPX_NCOLS doubles (column order AMT_RPX_COL_*); given exactly when a bit
 * other than AMT_RPX_CENTROID_WEIGHTED is set.  wtable_dev = nplanes x max_label x C x 4 doubles {weighted y, weighted
 * x, weighted local y, weighted local x}, from intensity = nplanes x C planes of element type in_code (AMT_U16:
 * integer sums, exact; AMT_F64: float64 sums); intensity, C >= 1 and wtable_dev are given exactly when
 * AMT_RPX_CENTROID_WEIGHTED is set.  A label with zero total intensity gets NaN weighted centroids; labels absent
 * from a plane get 0 in every column.
 *
 * ---- a label's surroundings: AMT_RPX_NEIGHBORS and AMT_RPX_NEAREST ----
 * CellProfiler's MeasureObjectNeighbors columns.  Both bits fill wtable_dev = nplanes x max_label x C x 4 doubles; the
 * integers among them are exact and held in doubles.
 * AMT_RPX_NEIGHBORS, the contact census: intensity is nplanes x C COMPANION LABEL planes, one (C, Y, X) stack per label
 * plane, in_code == AMT_I32, C >= 1, exactly as for AMT_RPX_RELATE; a companion may be the very buffer `labels` points
 * to, which is the usual call.  Companion values <= 0 are background.  For label l with pixel set P the RING R is the set
 * of in-image pixels q with labels[q] != l that have an 8-neighbour in P (a diagonal contact counts; the plane's border
 * clips the ring), and the neighbour values N of a companion plane B are the multiset {B[q] : q in R, B[q] > 0,
 * B[q] != l}: a label is not its own neighbour.  The four columns are
 *   AMT_RPX_NCOL_COUNT     the number of distinct values in N
 *   AMT_RPX_NCOL_TOUCHING  |N|, the ring pixels held by another object
 *   AMT_RPX_NCOL_RING      |R| (0 when the label fills its plane)
 *   AMT_RPX_NCOL_MAIN      the value with most pixels in N; among equal counts the smallest value wins; 0 when N is
 *                          empty
 * A label absent from its plane gives 0, 0, 0, 0.  Label values outside 1..max_label are never measured, but count as
 * neighbours when positive.  Counts are integer sums: two runs give identical bytes.  Up to AMT_RELATE_LDS_PARTNERS
 * distinct values of N are counted in LDS in one pass over the label's bounding box grown by one pixel; a label with
 * more is still exact, at one pass per value, as for AMT_RPX_RELATE.
 * AMT_RPX_NEAREST, the two nearest labels by centroid: intensity must be NULL, in_code 0 and C == 1.  The centroid of
 * label m is cy = (double)sum_y / (double)area and cx likewise, from integer sums (exact below 2^53 for every plane
 * this ABI accepts).  For label l every other label m of 1..max_label that is present in the plane gets
 * d2 = dy * dy + dx * dx with dy and dx the differences of the centroids, evaluated in that order in float64 without
 * fused multiply-add; the candidates are ordered by (d2, m), so among equal distances the smallest label wins.
 *   AMT_RPX_DCOL_FIRST / AMT_RPX_DCOL_FIRST_DISTANCE    the nearest label and sqrt(d2)
 *   AMT_RPX_DCOL_SECOND / AMT_RPX_DCOL_SECOND_DISTANCE  the next one
 * A first or second neighbour that does not exist gives label 0 and distance NaN; a label absent from its plane gives
 * 0, NaN, 0, NaN.  Label values outside 1..max_label are ignored.  The search compares every pair of labels of a plane
 * (max_label^2 / 2 distances); nothing depends on an order of accumulation: two runs give identical bytes.
 * One call sets at most one of AMT_RPX_CENTROID_WEIGHTED, AMT_RPX_RELATE, AMT_RPX_ROBUST, AMT_RPX_NEIGHBORS and
 * AMT_RPX_NEAREST (they share wtable_dev): more is AMT_EINVAL.  The morphology bits may be combined with either new
 * bit; table_dev is then given and its columns equal those of a call of their own.  AMT_RPX_NEIGHBORS with an in_code
 * other than AMT_I32 or without planes is AMT_EINVAL, and so is AMT_RPX_NEAREST with planes, an in_code other than 0
 * or C != 1.  wtable_dev is given exactly when one of the five bits is set, intensity and C >= 1 exactly when one of
 * the first four is; AMT_I32 planes go with AMT_RPX_RELATE or AMT_RPX_NEIGHBORS.  The accepted mask is
 * AMT_RPX_ALL | AMT_RPX_RELATE | AMT_RPX_ROBUST | AMT_RPX_NEIGHBORS | AMT_RPX_NEAREST.  nplanes == 0 or max_label == 0
 * is AMT_OK and writes nothing; every refusal happens before the first launch.
 *
 * ---- robust intensity statistics per label: AMT_RPX_ROBUST ----
 * With AMT_RPX_ROBUST set, intensity is nplanes x C planes of in_code AMT_U16 or AMT_F64, one (C, Y, X) stack per label
 * plane, C >= 1, and wtable_dev = nplanes x max_label x C x 4 doubles.  For label l with the pixel multiset V of a
 * channel the four columns are
 *   AMT_RPX_QCOL_Q25 / AMT_RPX_QCOL_MEDIAN / AMT_RPX_QCOL_Q75
 *                          np.percentile(V, 25 / 50 / 75), method 'linear': virtual index (n - 1) q / 100 with n = |V|,
 *                          and numpy's lerp between the two neighbouring order statistics, bit for bit
 *   AMT_RPX_QCOL_MAD       np.percentile(|V - median|, 50): the median absolute deviation around the column above, the
 *                          differences taken in float64 (one rounding each); raw, without the factor 1.4826.  It is the
 *                          50th percentile by the rule above, not np.median: for an even count those two differ in the
 *                          last bit on float64 data
 * For AMT_U16 every result is a multiple of 1/4 and exact; the selection runs on integer keys: the values, and
 * |2 v - 2 median| for MAD, counted in AMT_ROBUST_LDS_BINS LDS counters per workgroup over the window [min, max] of the
 * label (a window wider than the table is resolved by one more sweep over the label's box).  The cost per label and
 * channel is at most 5 sweeps over its bounding box, whatever its area (up to the plane's 2^31 - 2 pixels) and values.
 * AMT_F64 selects on order-preserving 64-bit keys, 8 bits per sweep (plain and untuned); images that hold NaN or
 * infinities are not supported, and -0.0 sorts before +0.0.  A label absent from its plane gives four NaNs (numpy on an
 * empty array).  Counts are integer sums: two runs give identical bytes.
 * AMT_RPX_ROBUST together with AMT_RPX_CENTROID_WEIGHTED, AMT_RPX_RELATE, AMT_RPX_NEIGHBORS or AMT_RPX_NEAREST is
 * AMT_EINVAL (they share wtable_dev); the morphology bits may be combined with it, table_dev is then given and its
 * columns equal those of a call of their own.  in_code other than AMT_U16 / AMT_F64 with the bit is AMT_EINVAL.
 * intensity, C >= 1 and wtable_dev are given exactly when one of AMT_RPX_CENTROID_WEIGHTED, AMT_RPX_RELATE,
 * AMT_RPX_ROBUST and AMT_RPX_NEIGHBORS is set (AMT_RPX_NEAREST: wtable_dev alone); the accepted mask is
 * AMT_RPX_ALL | AMT_RPX_RELATE | AMT_RPX_ROBUST | AMT_RPX_NEIGHBORS | AMT_RPX_NEAREST.  nplanes == 0 or max_label == 0
 * is AMT_OK and writes nothing; every refusal happens before the first launch.
 *
 * ---- relating two label images: AMT_RPX_RELATE ----
 * "Measure label image A with label image B as its intensity image": with AMT_RPX_RELATE set, intensity is
 * nplanes x C COMPANION LABEL planes, one (C, Y, X) stack per label plane, in_code == AMT_I32, values 0 (background)
 * to 2^31 - 2, C >= 1; a companion may be the very buffer `labels` points to.  wtable_dev = nplanes x max_label x C x 4
 * doubles.  For label l with pixel set P and companion plane B the four columns are
 *   AMT_RPX_RCOL_PARENT    the non-zero value v that maximises |{p in P : B[p] = v}|; among equal counts the smallest
 *                          v wins; 0 when B is zero on all of P
 *   AMT_RPX_RCOL_OVERLAP   that maximal count (0 without a parent)
 *   AMT_RPX_RCOL_PARTNERS  the number of distinct non-zero values of B on P
 *   AMT_RPX_RCOL_AREA      |P|
 * A label absent from its plane gives 0, 0, 0, 0.  All four are exact integers held in doubles; counts are integer
 * sums, so nothing depends on an order of accumulation and two runs give identical bytes.  Up to
 * AMT_RELATE_LDS_PARTNERS distinct partners of a label are counted in LDS in one pass over its bounding box; a label
 * with more is still exact, at one pass over its box per partner.
 * AMT_RPX_RELATE and AMT_RPX_CENTROID_WEIGHTED in one call is AMT_EINVAL (they share intensity and wtable_dev); the
 * morphology bits may be combined with either.  in_code != AMT_I32 with the bit set is AMT_EINVAL, and so is
 * in_code == AMT_I32 without it (or AMT_RPX_NEIGHBORS, which takes the same planes).  AMT_RPX_ALL stays the
 * scikit-image columns; which of the later bits exclude each other, when intensity, C >= 1 and wtable_dev are given
 * and the accepted mask stand in the blocks above.  nplanes == 0 or max_label == 0 is AMT_OK and writes nothing. */
#define AMT_RPX_EULER_NUMBER (1u << 0)
#define AMT_RPX_PERIMETER_CROFTON (1u << 1)
#define AMT_RPX_AREA_FILLED (1u << 2)
#define AMT_RPX_FERET_DIAMETER_MAX (1u << 3)
#define AMT_RPX_CENTROID_LOCAL (1u << 4)
#define AMT_RPX_INERTIA_TENSOR (1u << 5)
#define AMT_RPX_INERTIA_EIGVALS (1u << 6)
#define AMT_RPX_CENTROID_WEIGHTED (1u << 7)
#define AMT_RPX_ALL 0xffu
#define AMT_RPX_RELATE (1u << 8)
#define AMT_RPX_RCOL_PARENT 0
#define AMT_RPX_RCOL_OVERLAP 1
#define AMT_RPX_RCOL_PARTNERS 2
#define AMT_RPX_RCOL_AREA 3
#define AMT_RELATE_LDS_PARTNERS 128
#define AMT_RPX_ROBUST (1u << 9)
#define AMT_RPX_QCOL_Q25 0
#define AMT_RPX_QCOL_MEDIAN 1
#define AMT_RPX_QCOL_Q75 2
#define AMT_RPX_QCOL_MAD 3
#define AMT_ROBUST_LDS_BINS 1024
#define AMT_RPX_NEIGHBORS (1u << 10)
#define AMT_RPX_NCOL_COUNT 0
#define AMT_RPX_NCOL_TOUCHING 1
#define AMT_RPX_NCOL_RING 2
#define AMT_RPX_NCOL_MAIN 3
#define AMT_RPX_NEAREST (1u << 11)
#define AMT_RPX_DCOL_FIRST 0
#define AMT_RPX_DCOL_FIRST_DISTANCE 1
#define AMT_RPX_DCOL_SECOND 2
#define AMT_RPX_DCOL_SECOND_DISTANCE 3
#define AMT_RPX_COL_EULER_NUMBER 0
#define AMT_RPX_COL_PERIMETER_CROFTON 1
#define AMT_RPX_COL_AREA_FILLED 2
#define AMT_RPX_COL_FERET_DIAMETER_MAX 3
#define AMT_RPX_COL_CENTROID_LOCAL_Y 4
#define AMT_RPX_COL_CENTROID_LOCAL_X 5
#define AMT_RPX_COL_INERTIA_00 6
#define AMT_RPX_COL_INERTIA_01 7
#define AMT_RPX_COL_INERTIA_10 8
#define AMT_RPX_COL_INERTIA_11 9
#define AMT_RPX_COL_EIGVAL_0 10
#define AMT_RPX_COL_EIGVAL_1 11
#define AMT_RPX_NCOLS 12
int amt_regionprops_ext(amt_ctx* ctx, const int32_t* labels, const void* intensity, int in_code, int C,
                        int columns, double* table_dev, double* wtable_dev, int nplanes, int H, int W,
                        int max_label);
int amt_max_i32(amt_ctx* ctx, const int32_t* in, int32_t* max_dev, int nplanes, size_t n);
/* ---- per-label colocalisation of channel pairs ----------------------------------------------------------
 * For one label with pixel set P (n pixels), channels A and B with values a_p, b_p and thresholds tA, tB
 * ("positive" means value > threshold, the comparison amt_threshold_gt makes), the columns are
 *   AMT_COLOC_PEARSON        (n Sum ab - Sum a Sum b) / sqrt((n Sum a^2 - (Sum a)^2) (n Sum b^2 - (Sum b)^2));
 *                            NaN when either channel is constant over P (n = 1 and an absent label included)
 *   AMT_COLOC_OVERLAP        Sum ab / sqrt(Sum a^2 Sum b^2), Manders' overlap coefficient; NaN when that root is 0
 *   AMT_COLOC_M1             Sum a_p[b_p > tB] / Sum a; 0 when Sum a = 0
 *   AMT_COLOC_M2             Sum b_p[a_p > tA] / Sum b; 0 when Sum b = 0
 *   AMT_COLOC_INTERSECTION1  |{a > tA and b > tB}| / |{a > tA}|; 0 when no pixel has a > tA
 *   AMT_COLOC_INTERSECTION2  |{a > tA and b > tB}| / |{b > tB}|; 0 when no pixel has b > tB
 * A label with no pixel in its plane gives NaN, NaN, 0, 0, 0, 0.  These restate the colocalisation functions of
 * skimage.measure (pearson_corr_coeff, manders_overlap_coeff, manders_coloc_coeff, intersection_coeff, scikit-image
 * 0.20 and later) per label; parity with that module is unpinned offline.
 * intensity = nplanes x C planes (C >= 2) of element type in_code, one (C, Y, X) stack per label plane.  AMT_U16: every
 * sum is an exact 64-bit integer and Pearson's differences are taken in 128 bits, so results do not depend on any
 * order of summation, the four quotient columns are correctly rounded and pearson / overlap carry a few roundings.
 * AMT_F64: two sweeps in float64 (means, then centred sums); a channel is constant when its min equals its max over
 * P; NaN or infinite intensities are not supported.  thresholds_dev = nplanes x C doubles on the device;
 * pairs_host = npairs x 2 channel indices (i, j), i != j, in HOST memory: A = channel i, B = channel j.
 * table_dev = nplanes x max_label x npairs x AMT_COLOC_NCOLS doubles.  No atomics: two runs give identical bits. */
#define AMT_COLOC_PEARSON 0
#define AMT_COLOC_OVERLAP 1
#define AMT_COLOC_M1 2
#define AMT_COLOC_M2 3
#define AMT_COLOC_INTERSECTION1 4
#define AMT_COLOC_INTERSECTION2 5
#define AMT_COLOC_NCOLS 6
int amt_colocalization(amt_ctx* ctx, const int32_t* labels, const void* intensity, int in_code, int C,
                       const double* thresholds_dev, const int32_t* pairs_host, int npairs, double* table_dev,
                       int nplanes, int H, int W, int max_label);
/* ---- per-label Haralick texture (grey-level co-occurrence): the AMT_RPX_TEXTURE bit of the extended region properties ----
 * The capability rides on the entry point of the extended region properties, like the relation, the robust statistics
 * and the neighbours: no entry point of its own.  `columns` = AMT_RPX_TEXTURE_COLUMNS(levels, distance, counts), which
 * sets ONE of AMT_RPX_TEXTURE (bit 12: the call writes the feature table) and AMT_RPX_TEXTURE_COUNTS (bit 13: the call
 * writes the raw matrices instead; both bits together are AMT_EINVAL), levels = L in bits 14-20 and distance = d in bits
 * 21-30 (the fields hold 0..127 and 0..1023, so every value outside 2..64 and 1..255 up to there can be stated and is
 * refused); no other bit goes with them (the morphology bits and the other table bits are AMT_EINVAL).  labels = nplanes
 * int32 planes; intensity = nplanes x C planes (C >= 1) of element type in_code (AMT_U16 or AMT_F64), one (C, Y, X) stack
 * per label plane.  With these bits table_dev is an INPUT: the ranges, nplanes x C x 2 doubles {lo, hi} on the device, one
 * pair per (plane, channel) image; it is only read.  wtable_dev is the one output of the call: the features, or with
 * AMT_RPX_TEXTURE_COUNTS the counts (layout below); a caller who wants both calls twice with two buffers of its own,
 * and the features do not depend on whether the counts are taken.
 * AMT_EINVAL for levels outside 2..64, distance outside 1..255, an in_code other than AMT_U16 / AMT_F64, C < 1, a null
 * labels, intensity, table_dev (ranges) or wtable_dev, and for a wtable_dev that overlaps another operand; table_dev
 * counts as an input in this call.
 * QUANTISATION (both element types; uint16 converts to float64 exactly):  v' = min(max(v, lo), hi),
 *   q = min(L - 1, floor((v' - lo) / (hi - lo) * L)),  evaluated in float64 in exactly that order -- subtract, divide,
 * multiply, floor -- without contraction, so numpy reproduces every bin bit for bit.  hi <= lo gives q = 0 everywhere.
 * NaN and infinite intensities or ranges are not supported.
 * CO-OCCURRENCE: for label l with pixel set P, direction a in {0, 45, 90, 135} degrees has the offset (dy, dx) =
 * (0, d), (d, -d), (d, 0), (d, d).  Every unordered pair {p, p + offset} with both ends in P adds 1 to
 * G_a[q(p)][q(p + offset)] and 1 to the transposed entry, so a pair of equal levels adds 2 to a diagonal entry: the
 * symmetric matrix of Haralick (1973) and of skimage.feature.graycomatrix(symmetric=True).  "Both in P" means both carry
 * the value l: connectivity is not considered (two pieces of a label d apart do pair), a pixel of another label or of
 * the background never pairs, and no pixel outside the label's bounding box is read.
 * FEATURES: thirteen columns per (label, channel, direction) from p = G / Sum G, with px(i) = Sum_j p(i, j),
 * p+(k) = Sum_{i + j = k} p (k = 0 .. 2L - 2), p-(k) = Sum_{|i - j| = k} p (k = 0 .. L - 1), mu = Sum i px(i),
 * s2 = Sum (i - mu)^2 px(i), 0 log 0 = 0, logarithms to base 2:
 *   AMT_TEX_ANGULAR_SECOND_MOMENT      Sum p^2
 *   AMT_TEX_CONTRAST                   Sum k^2 p-(k)
 *   AMT_TEX_CORRELATION                Sum (i - mu)(j - mu) p / s2; 1 when exactly one grey level occurs (decided on
 *                                      the integer counts)
 *   AMT_TEX_VARIANCE                   s2
 *   AMT_TEX_INVERSE_DIFFERENCE_MOMENT  Sum p / (1 + (i - j)^2)
 *   AMT_TEX_SUM_AVERAGE                Sum k p+(k)
 *   AMT_TEX_SUM_VARIANCE               Sum (k - sum_average)^2 p+(k)
 *   AMT_TEX_SUM_ENTROPY                -Sum p+ log2 p+
 *   AMT_TEX_ENTROPY                    HXY = -Sum p log2 p
 *   AMT_TEX_DIFFERENCE_VARIANCE        Sum (k - m)^2 p-(k), m = Sum k p-(k)
 *   AMT_TEX_DIFFERENCE_ENTROPY         -Sum p- log2 p-
 *   AMT_TEX_INFO_MEASURE_1             (HXY - HXY1) / HX, HX = -Sum px log2 px, HXY1 = -Sum p(i, j) log2(px(i) px(j));
 *                                      0 when HX = 0
 *   AMT_TEX_INFO_MEASURE_2             sqrt(max(0, 1 - exp(-2 (HXY2 - HXY)))), HXY2 = -Sum px(i) px(j) log2(px(i) px(j))
 * These restate mahotas.features.haralick, the routine behind CellProfiler's MeasureTexture (its sum_average inside
 * sum_variance included); parity with that module is unpinned offline.
 * A direction in which the label has no pair (a single pixel, a one-pixel-wide row in direction 90, d larger than the
 * box) gives thirteen quiet NaNs for that direction only and zero counts; a label absent from its plane gives NaN in all
 * four directions.
 * wtable_dev = nplanes x max_label x C x 4 x AMT_TEX_NCOLS doubles, directions in the order 0, 45, 90, 135; with
 * AMT_RPX_TEXTURE_COUNTS instead nplanes x max_label x C x 4 x levels x levels uint32 behind the same pointer: the raw
 * counts G_a, exact integers.
 * Planes of up to 2^31 - 1 pixels.  Counting is integer and the float64 sums run in one fixed order: two runs give
 * identical bytes; no global atomics.  nplanes == 0 or max_label == 0 writes nothing. */
#define AMT_TEX_ANGULAR_SECOND_MOMENT 0
#define AMT_TEX_CONTRAST 1
#define AMT_TEX_CORRELATION 2
#define AMT_TEX_VARIANCE 3
#define AMT_TEX_INVERSE_DIFFERENCE_MOMENT 4
#define AMT_TEX_SUM_AVERAGE 5
#define AMT_TEX_SUM_VARIANCE 6
#define AMT_TEX_SUM_ENTROPY 7
#define AMT_TEX_ENTROPY 8
#define AMT_TEX_DIFFERENCE_VARIANCE 9
#define AMT_TEX_DIFFERENCE_ENTROPY 10
#define AMT_TEX_INFO_MEASURE_1 11
#define AMT_TEX_INFO_MEASURE_2 12
#define AMT_TEX_NCOLS 13
#define AMT_RPX_TEXTURE (1u << 12)
#define AMT_RPX_TEXTURE_COUNTS (1u << 13)
#define AMT_RPX_TEXTURE_LEVELS_SHIFT 14
#define AMT_RPX_TEXTURE_DISTANCE_SHIFT 21
#define AMT_RPX_TEXTURE_COLUMNS(levels, distance, counts)                                      \
    ((int)(((counts) ? AMT_RPX_TEXTURE_COUNTS : AMT_RPX_TEXTURE) |                             \
           ((unsigned)(levels) << AMT_RPX_TEXTURE_LEVELS_SHIFT) | ((unsigned)(distance) << AMT_RPX_TEXTURE_DISTANCE_SHIFT)))
/* ---- per-label radial intensity distribution and inscribed radii: the AMT_RPX_RADIAL bit of the extended region
 * properties ----
 * How a channel's signal is spread between a label's centre and its rim, and the two radii of the label's shape.  Like
 * texture the capability rides on amt_regionprops_ext.  `columns` = AMT_RPX_RADIAL_COLUMNS(bins): AMT_RPX_RADIAL (bit 31,
 * so the value is negative as an int) and bins = B in the 7-bit field at AMT_RPX_TEXTURE_LEVELS_SHIFT (bits 14-20; the
 * field holds 0..127, so 0 and 17 can be stated and are refused).  With bit 31 set every other bit, bits 21-30 included,
 * must be 0: the morphology bits, the other table bits and both texture bits are AMT_EINVAL.  labels = nplanes int32
 * planes; intensity = nplanes x C planes of element type in_code (AMT_U16 or AMT_F64; other codes are AMT_EINVAL), one
 * (C, Y, X) stack per label plane.  C == 0 with intensity == NULL and wtable_dev == NULL is the geometry-only call
 * (in_code is not looked at); C >= 1 needs both.  table_dev (never NULL) and wtable_dev are both outputs.  AMT_EINVAL
 * for B outside 1..16 and for an output that overlaps another operand.
 * These definitions are our own, after CellProfiler's MeasureObjectIntensityDistribution / MeasureObjectSizeShape;
 * parity with CellProfiler is unpinned offline.  For label l of a plane with pixel set P (n pixels), channel values v_p:
 * DISTANCE TO THE EDGE: d2(p) = the smallest squared Euclidean distance from p to a pixel that does not carry l --
 * background, another label, or any position outside the image: the plane counts as framed with zeros.  So d2 >= 1, and
 * a label cut by the border has its edge there.  Connectivity plays no part: a hole, or a gap between two pieces of l,
 * is outside.  d2 is an exact integer; dmax2 = max over P of d2.
 * RING: ring 0 is the innermost, ring B - 1 the outermost.  b(p) = the largest k in 0..B-1 with
 *   d2(p) * B * B <= dmax2 * (B - k) * (B - k)   in 64-bit integers;
 * in real numbers floor(B * (1 - d / dmax)) with exact ties going outward.  No square root and no float decides a ring.
 * WEDGE: with sy = Sum_P y, sx = Sum_P x, ey = n * y - sy and ex = n * x - sx in int64,
 *   w(p) = (ey > 0) + 2 * (ex > 0) + 4 * (|ey| > |ex|):  eight wedges around the centroid, decided on integers.
 * GEOMETRY ROW per (plane, label): table_dev = nplanes x max_label x AMT_RAD_GEOM_NCOLS doubles,
 *   AMT_RAD_GEOM_MAXIMUM_RADIUS      sqrt((double)dmax2), the radius of the largest inscribed circle
 *   AMT_RAD_GEOM_MEAN_RADIUS         (Sum_P sqrt((double)d2)) / n; the sum is the exact sum of the float64 roots rounded
 *                                    once (Python's math.fsum), so it depends on no order of summation
 *   AMT_RAD_GEOM_RING_COUNT0 + b     n_b, the pixel count of ring b, for b < B; the columns from B to 15 are 0
 * INTENSITY ROWS per (plane, label, channel, ring): wtable_dev = nplanes x max_label x C x B x AMT_RAD_NCOLS doubles.
 * With S_bw the sum of v over the pixels of ring b in wedge w, n_bw their number, S_b = Sum_w S_bw and S = Sum_b S_b:
 *   AMT_RAD_FRAC_AT_D   S_b / S; NaN when S == 0
 *   AMT_RAD_MEAN_FRAC   (S_b / S) / (n_b / n), in that order; NaN when n_b == 0 or S == 0
 *   AMT_RAD_RADIAL_CV   over the wedges w = 0..7 that hold a pixel of ring b, m_w = S_bw / n_bw; mu = the sum of the m_w
 *                       in wedge order divided by their number; var = the sum of (m_w - mu)^2 in wedge order divided by
 *                       their number; the column is sqrt(var) / mu.  NaN when the ring is empty or mu == 0
 * all in float64 without contraction in exactly this order, so that a scalar numpy loop reproduces the bits.
 * AMT_U16: S_bw, S_b and S are exact 64-bit integers, each converted once; every column is then a fixed sequence of
 * correctly rounded operations and does not depend on the order of summation.  AMT_F64: S_bw is summed in the order of
 * the box walk and the wave reductions, S_b over the wedges and S over the rings in ascending order: fixed, so two runs
 * give identical bits; NaN and infinite intensities are not supported.
 * A label absent from its plane gives NaN radii, zero counts and NaN intensity columns.  Every box size gives the exact
 * result: a label whose bounding box has more cells than LDS holds keeps its distances in scratch planes (16 + 32 bits
 * per pixel of the call, always reserved); its row search costs time in proportion to its radius.  Planes of up to
 * 2^31 - 1 pixels.  No global atomics.  nplanes == 0 or max_label == 0 writes nothing. */
#define AMT_RAD_FRAC_AT_D 0
#define AMT_RAD_MEAN_FRAC 1
#define AMT_RAD_RADIAL_CV 2
#define AMT_RAD_NCOLS 3
#define AMT_RAD_MAX_BINS 16
#define AMT_RAD_GEOM_MAXIMUM_RADIUS 0
#define AMT_RAD_GEOM_MEAN_RADIUS 1
#define AMT_RAD_GEOM_RING_COUNT0 2
#define AMT_RAD_GEOM_NCOLS 18
#define AMT_RPX_RADIAL (1u << 31)
#define AMT_RPX_RADIAL_COLUMNS(bins) ((int)(AMT_RPX_RADIAL | ((unsigned)(bins) << AMT_RPX_TEXTURE_LEVELS_SHIFT)))

/* ---- per-plate feature rows (the reference's analogue is the list of cell_properties dicts a
 * user collects per image, R/masks.py:247-328, R/pipeline.py:145-149) ------------------------------------------
 * Compacts the dense tables of B fields of view (table_dev B x K x AMT_RP_NCOLS, itable_dev B x K x C x 4,
 * ncells_dev B int32) into one row per cell, fields of view in order, labels 1..ncells[b] in order:
 *   row = [fov index, label, the AMT_RP_NCOLS morphology columns, C x {mean, max, min, std}]  (16 + 4 C doubles)
 * The fov index of plane b is fov_index_dev[b], or fov_index0 + b when fov_index_dev is NULL.  rows_cap (in rows)
 * must be >= B * K.  *nrows_dev = total rows, or -1 when a field of view holds a count outside [0, K] (its table
 * overflowed).  This block is what a rank contributes to the plate's all-gather: counts first, then rows. */
int amt_pack_plate_rows(amt_ctx* ctx, const double* table_dev, const double* itable_dev, const int32_t* ncells_dev, int B,
                        int K, int C, const int32_t* fov_index_dev, int fov_index0, double* rows_dev, size_t rows_cap,
                        int64_t* nrows_dev);

/* ---- cell outlines: R/masks.py:82-115 (_extract_outlines_skimage), SK/measure/_find_contours.py ------
 * bbox_dev = nplanes x max_label x 4 ints {min row, min col, max row, max col} INCLUSIVE; labels absent from a
 * plane give max < min. */
int amt_label_bboxes(amt_ctx* ctx, const int32_t* labels, int32_t* bbox_dev, int nplanes, int H, int W, int max_label);
/* Marching squares at level 0.5 on the crop of every listed label of ONE label plane (H x W int32), longest
 * contour kept (first among equals), in scikit-image's vertex order.  Two calls with a host step in between
 * (the outline lengths size the output):
 *   boxes_dev   nlab x 5 ints {label, r_lo, c_lo, r_hi, c_hi}: the bounding box padded by one pixel and clamped
 *               to the image, half-open (R/masks.py:99-104)
 *   voff_dev    nlab + 1 offsets into visited_dev, one scratch byte per square ((h-1) x (w-1)) of each crop
 *   info_dev    nlab x 4 ints {points, closed, start square, start segment}; points = 0 for an empty outline
 *   poff_dev    nlab + 1 offsets (in points) into points_dev = (row, col) float64 pairs, image coordinates */
int amt_contours_find(amt_ctx* ctx, const int32_t* labels, int H, int W, int nlab, const int32_t* boxes_dev,
                      const int64_t* voff_dev, uint8_t* visited_dev, size_t visited_bytes, int32_t* info_dev);
int amt_contours_emit(amt_ctx* ctx, const int32_t* labels, int H, int W, int nlab, const int32_t* boxes_dev,
                      const int32_t* info_dev, const int64_t* poff_dev, double* points_dev);

/* Pixel-border outlines, the reference's default extractor (R/masks.py:68-79: cellpose.utils.outlines_list ->
 * cv2.findContours(masks == n, RETR_EXTERNAL, CHAIN_APPROX_NONE), contour with the most points, newest first among
 * equals).  Suzuki-Abe border following on ONE int32 label plane, one walk per outer border.  Parity unpinned: no
 * OpenCV / cellpose offline and no vector in the reference's tests (see oracle/contours.py).
 *   boxes_dev   nlab x 5 ints {label, r_lo, c_lo, r_hi, c_hi}: the TIGHT bounding box, half-open
 *   marks_dev   H x W scratch bytes (cleared by the call)
 *   info_dev    nlab x 3 ints {points, start row, start col} of the selected border
 *   poff_dev    nlab + 1 offsets (in points) into points_dev = (row, col) int32 pairs; a label whose slot is not
 *               exactly its point count is skipped (the host drops borders of fewer than five points) */
int amt_borders_find(amt_ctx* ctx, const int32_t* labels, int H, int W, int nlab, const int32_t* boxes_dev,
                     int8_t* marks_dev, int32_t* info_dev);
int amt_borders_emit(amt_ctx* ctx, const int32_t* labels, int H, int W, int nlab, const int32_t* boxes_dev,
                     const int32_t* info_dev, const int64_t* poff_dev, int32_t* points_dev);

/* ---- Cellpose post-processing: flows + cell probability -> labels (BASELINE configs[4]; the reference reaches it
 * through CellposeModel.eval, R/model.py:206-215, :270-290).  Restated from the published algorithm (cellpose
 * dynamics: follow the flow for niter Euler steps with bilinear sampling, histogram the end points, seeds = 5 x 5
 * maxima with more than 10 pixels, five rounds of 3 x 3 growth over bins with more than 2 pixels, labels by end point,
 * masks above max_size_fraction of the image or below min_size dropped, renumbered in raster order), then the rest of
 * cellpose's compute_masks, as CellposeModel.eval runs it with the parameters the reference hands over
 * (R/model.py:206-215: flow_threshold, default 0.4):
 *   flow_threshold > 0: remove_bad_flow_masks -- the flows are re-derived from the masks (float64 heat diffusion from
 *       each mask's centre, 2 * max(height + width + 2) steps) and a mask whose mean squared difference to dP / 5
 *       exceeds the threshold is dropped;
 *   then fill_holes_and_remove_small_masks: masks below min_size dropped, (fill_holes != 0) the others hole-filled
 *       inside their bounding box, renumbered 1..K in ascending order.
 * flow_threshold == 0 and fill_holes == 0 stops after the first stage.  PARITY UNPINNED: cellpose is not available
 * offline and the reference holds no vector for it (oracle: oracle/cellpose_dynamics.py).
 *   dP = nplanes x 2 x H x W float32 (dY, dX), cellprob = nplanes x H x W float32, labels_out = nplanes x H x W int32,
 *   count_dev[plane] = number of masks, or -1 if the plane produced more than max_seeds seeds.
 *   max_size_fraction is a double: the ceiling is (long long)(H * W * max_size_fraction) in float64, as get_masks takes it. */
int amt_cellpose_masks_ex(amt_ctx* ctx, const float* dP, const float* cellprob, int32_t* labels_out, int32_t* count_dev,
                          int nplanes, int H, int W, float cellprob_threshold, int niter, int min_size,
                          double max_size_fraction, int max_seeds, float flow_threshold, int fill_holes);
/* cellpose.utils.fill_holes_and_remove_small_masks on its own (the last step of amt_cellpose_masks_ex): labels_io =
 * nplanes x H x W int32 carrying labels 1..nlabels_dev[plane] (<= max_label; gaps allowed, larger values are treated as
 * background), in place: labels in ascending order, those with fewer than min_size pixels dropped, (fill_holes != 0)
 * the others hole-filled inside their bounding box -- written over whatever lies in the hole, in sequence, as the
 * package's loop does --, renumbered 1..K; count_dev[plane] = K. */
int amt_fill_holes_remove_small(amt_ctx* ctx, int32_t* labels_io, const int32_t* nlabels_dev, int32_t* count_dev,
                                int nplanes, int H, int W, int max_label, int min_size, int fill_holes);
/* metrics.flow_error of cellpose on its own: labels = nplanes x H x W int32 carrying 1..nlabels_dev[plane] (<= max_label),
 * dP as above; err_out = nplanes x max_label float64 (absent labels 0, the slots above nlabels_dev[plane] included). */
int amt_cellpose_flow_error(amt_ctx* ctx, const int32_t* labels, const float* dP, const int32_t* nlabels_dev,
                            double* err_out, int nplanes, int H, int W, int max_label);

/* ---- channel overlay: R/blending.py:116-226 (create_overlay / overlay_channels) ------------------------
 * out_rgb = H x W x 3 float64 (interleaved).  background and every layer are H x W float64 planes on the device
 * (values outside [0, 1] are clipped, as the reference does).  layers_host = nlayers device pointers;
 * luts_host = nlayers x 256 x 4 float64 RGBA tables (matplotlib's LinearSegmentedColormap table of each layer);
 * opacity_host in [0, 1]; mode_host 0 = ALPHA ("over"), 1 = ADDITIVE.  At most 8 layers per call. */
int amt_overlay(amt_ctx* ctx, const double* background, const double* const* layers_host, int nlayers,
                const double* luts_host, const double* opacity_host, const int32_t* mode_host, double* out_rgb, int H,
                int W);

/* ---- glue of the config-5 flow network (BASELINE configs[4]; R/model.py:211: the network's convolutions run through
 * PyTorch-ROCm) ---- every convolution of Cellpose's residual U-Net is "batch norm -> [ReLU] -> conv" on a sum of up to
 * three terms; one pass prepares its input instead of one framework kernel per operation:
 *   s = (upsample ? x[n,h/2,w/2,c] : x[n,h,w,c]) + y[n,h,w,c] + pre_bias[c];  out = act((s + style[n,c]) * scale[c] + shift[c])
 * x, y (nullable), out, sum_out (nullable: receives s) are bf16 NHWC (channels-last) tensors, style (nullable) float32
 * [N][C], pre_bias (nullable: the biases of the convolutions that produced x and y, run without them), scale / shift
 * float32 [C] (the folded inference-time batch norm); C % 8 == 0. */
int amt_nn_affine_act_bf16(amt_ctx* ctx, const void* x, const void* y, const float* style, const float* pre_bias,
                           const float* scale, const float* shift, void* out, void* sum_out, int N, int H, int W, int C,
                           int relu, int upsample);

/* ---- image normalisation of CellposeModel.eval (R/model.py:206-215 calls eval, whose `normalize=` / `invert=` options
 * map every channel of the image before the network sees it; restated from cellpose 4.0.x transforms.normalize_img /
 * normalize99, PARITY UNPINNED; caller: cellpose_hip.normalize_image) ----
 * Per plane, float32 arithmetic, one correctly rounded operation each:
 *   lo, hi = lohi_dev[plane] = {lo, hi} rounded to float32;  d = hi - lo;
 *   out = d > 1e-3f ? (x - lo) / d : 0;   invert != 0: out = 1 - out
 * in = nplanes x n samples, AMT_U16 / AMT_F32 (exact as float32) or AMT_F64 (rounded once to float32); lohi_dev =
 * nplanes x 2 values on the device, AMT_F64 (the percentiles as amt_percentile_u16 / amt_percentile_f64 leave them: no
 * host round trip between them and this call) or AMT_F32; out = nplanes x n float32, not aliasing in.  At most 65,535
 * planes per call.  16-byte loads and stores when in and out are 16-byte aligned (any n). */
int amt_normalize_planes_f32(amt_ctx* ctx, const void* in, int in_dtype, const void* lohi_dev, int lohi_dtype, int invert,
                             float* out, int nplanes, size_t n);
/* float32 -> float64 (exact): the way of a float32 image into amt_percentile_f64 (cellpose_hip.normalize_image). */
int amt_convert_f32_f64(amt_ctx* ctx, const float* in, double* out, size_t n);

#ifdef __cplusplus
}
#endif
#endif /* AMT_HIP_H */
