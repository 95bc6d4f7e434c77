/*
 * imagekit_hip.h -- C ABI of libimagekit_hip.so, the MI355X-native drop-in for
 * the reference's transform hot path (Shreyas2409/Rust-Image-Transform,
 * crate `imagekit`, module `imagekit::transform`).
 *
 * The reference has no plugin registry: its "operator API" is three free Rust
 * functions (src/transform.rs) called by the /img and /upload handlers
 * (src/lib.rs:175,180,188 and :281,286,294).  Each entry point below names the
 * reference item it replaces.  Plain pointers and sizes only; images are
 * device-resident handles (ik_image) so a decode -> resize -> encode chain
 * keeps pixels in HBM.  All functions are thread-safe; errors are reported as
 * an ik_status plus a thread-local message (ik_last_error), never a panic or
 * abort across the ABI (reference: every failure maps to
 * ImageKitError::TransformError, src/lib.rs:34-52).
 */
#ifndef IMAGEKIT_HIP_H
#define IMAGEKIT_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ImageFormat (reference src/config.rs:11-17): jpeg, webp, avif */
typedef enum { IK_FORMAT_JPEG = 0, IK_FORMAT_WEBP = 1, IK_FORMAT_AVIF = 2 } ik_format;

/* image::imageops::FilterType (image 0.25.8).  The reference always uses
 * Lanczos3 (src/transform.rs:88); the others are extensions. */
typedef enum {
    IK_FILTER_NEAREST = 0,
    IK_FILTER_TRIANGLE = 1,
    IK_FILTER_CATMULLROM = 2,
    IK_FILTER_GAUSSIAN = 3,
    IK_FILTER_LANCZOS3 = 4
} ik_filter;

typedef enum {
    IK_OK = 0,
    IK_ERR_TRANSFORM = 1,   /* ImageKitError::TransformError (decode/encode failure) */
    IK_ERR_INVALID = 2,     /* bad argument (null pointer, zero size, bad enum)    */
    IK_ERR_DEVICE = 3,      /* HIP runtime failure                                  */
    IK_ERR_UNSUPPORTED = 4, /* recognised but not compiled in (e.g. AVIF decode)    */
    IK_ERR_NOMEM = 5
} ik_status;

/* DynamicImage (image 0.25.8): 8-bit, 1..4 interleaved channels
 * (Luma8, LumaA8, Rgb8, Rgba8), pixels resident in device memory. */
typedef struct ik_image ik_image;

/* ---- runtime ---------------------------------------------------------- */
/* ik_init(d >= 0): select HIP device d for the calling thread.
 * ik_init(-1): one process drives every visible GPU (or the list in IK_DEVICES,
 *   e.g. "0,1,2,3"; a device may repeat, "0,0" = two logical devices on GPU 0).
 *   From then on ik_transform / ik_transform_batch / ik_decode called from any
 *   number of threads feed a host work queue: each request goes to the logical
 *   device with the least outstanding cost (ik_request_cost), and runs there on
 *   that device's persistent workers.  The reference's analogue is tokio's
 *   multi-thread runtime calling the transform from every worker
 *   (src/main.rs:20, src/lib.rs:175-191). */
int ik_init(int device);
int ik_init_devices(const int *devices, int n); /* ik_init(-1) with an explicit list */
int ik_device_count(void);
int ik_logical_device_count(void);  /* 0 unless multi-device dispatch is on */
/* per logical device: requests taken, cost completed, cost still outstanding */
int ik_logical_device_stats(uint32_t logical, uint64_t *jobs, uint64_t *cost_done, uint64_t *outstanding);
/* the scheduler's cost of one request, in bytes-equivalent: encoded input +
 * decoded pixels (from the header) + an encoder weight per output pixel */
uint64_t ik_request_cost(const uint8_t *bytes, size_t len, int64_t w, int64_t h, int fmt);
/* the batch placement policy on its own (no device work): n requests with
 * costs[i] over ndev devices already carrying outstanding[d] (may be NULL) ->
 * assign[i]; largest request first to the least-loaded device */
void ik_schedule_plan(const uint64_t *costs, uint32_t n, uint32_t ndev, const uint64_t *outstanding,
                      uint32_t *assign);
/* a batch submit's split over ndev logical devices on its own (no device work):
 * min(ndev, n / min_batch) contiguous parts (at least one) -- part q is requests
 * [part_lo[q], part_lo[q+1]) (part_lo: ndev + 1 entries) -- each placed in turn on
 * the least-loaded device (part_dev[q]); returns the part count.  submit uses it
 * with min_batch = IK_MIN_DEVICE_BATCH (64). */
uint32_t ik_schedule_split(const uint64_t *costs, uint32_t n, uint32_t ndev, const uint64_t *outstanding,
                           uint32_t min_batch, uint32_t *part_lo, uint32_t *part_dev);
/* ik_transform_batch's post-stage routing on its own (no device work): for m decoded
 * requests -- ok[k] (decoded), the image's W, H, C, pitch, device and depth (bytes per
 * sample), the requested w / h (negative = None), fmt and quality -- under a WebP encoder
 * setting (IK_WEBP_*) and a mixed mode (IK_WEBP_MIXED_*): the size each request is coded
 * at (nw, nh; 0 when its resize target cannot be computed), the same-geometry resize
 * group (one launch) and the coder group inside it (one group call) it belongs to, or
 * -1, and its route.  Groups are numbered in launch order.  info[4]: whether the batch
 * makes a mixed exact call, the fewest requests that call takes, the resize group count,
 * the coder group count.  The rules: csrc/ik_post_plan.h. */
typedef enum {
    IK_POST_NONE = 0,             /* the decode failed                                        */
    IK_POST_SINGLE = 1,           /* per-image resize and / or encoder front end              */
    IK_POST_WEBP_MIXED = 2,       /* kept for the batch's one mixed exact WebP call           */
    IK_POST_WEBP_FRONT_GROUP = 3, /* group colour launch, libwebp codes the planes            */
    IK_POST_WEBP_EXACT_GROUP = 4, /* group call of the exact GPU WebP coder                   */
    IK_POST_JPEG_GROUP = 5        /* group call of the GPU JPEG coder                         */
} ik_post_route;
int ik_post_plan(uint32_t m, const int *ok, const uint32_t *W, const uint32_t *H, const uint32_t *C,
                 const uint64_t *pitch, const int *device, const uint32_t *depth, const int64_t *w, const int64_t *h,
                 const int *fmt, const int *quality, int webp_encoder, int mixed_mode, uint32_t *nw, uint32_t *nh,
                 int *resize_group, int *coder_group, int *route, uint32_t *info);
/* How a request's (w, h) becomes pixels (the reference's query parser declares
 * fit=cover|contain, src/transform/params.rs:37-64).  With (tw, th) the request's target
 * -- a missing side computed in f32 with round, each side at least 1:
 *   IK_FIT_CONTAIN  DynamicImage::resize: the largest size of the image's aspect inside
 *                   tw x th (resize_image, src/transform.rs:62-90; ik_resize)
 *   IK_FIT_COVER    DynamicImage::resize_to_fill: the smallest size of the image's aspect
 *                   that covers tw x th -- resize_dimensions(fill), f64 ratio max(tw/W,
 *                   th/H), round, at least 1 -- resampled as ik_resize_exact does and
 *                   cropped to tw x th, centred ((iw - tw) / 2 or (ih - th) / 2, integer
 *                   division) along the axis that overflows.  With one of w / h None there
 *                   is nothing to crop: IK_FIT_CONTAIN.  (image 0.25.8 as recalled; parity
 *                   unpinned)
 *   IK_FIT_EXACT    DynamicImage::resize_exact: tw x th, the aspect not kept
 * Only the kept columns and rows are computed: a cover launch reads the source columns
 * and rows its window needs and writes nw x nh pixels. */
typedef enum { IK_FIT_CONTAIN = 0, IK_FIT_COVER = 1, IK_FIT_EXACT = 2 } ik_fit;
/* ik_post_plan with a fit mode per request (fit NULL: every request IK_FIT_CONTAIN, which
 * is ik_post_plan).  Resize groups share the whole window, so an exact and a cover request
 * of one output size are different groups.  window (may be NULL): six values per request,
 * iw, ih, x0, y0, nw, nh -- it is coded at columns [x0, x0 + nw), rows [y0, y0 + nh) of its
 * image resampled to iw x ih; zeros when that cannot be computed. */
int ik_post_plan_fit(uint32_t m, const int *ok, const uint32_t *W, const uint32_t *H, const uint32_t *C,
                     const uint64_t *pitch, const int *device, const uint32_t *depth, const int64_t *w,
                     const int64_t *h, const int *fit, const int *fmt, const int *quality, int webp_encoder,
                     int mixed_mode, uint32_t *nw, uint32_t *nh, int *resize_group, int *coder_group, int *route,
                     uint32_t *info, uint32_t *window);
/* Orderly teardown: waits for every submitted batch, ends
 * the library's stage threads and worker pools (each releases its HIP streams
 * and arenas), then frees the pooled images, upload areas, resize plans and
 * pinned blocks -- while the HIP runtime is still alive, so that nothing is left
 * to destructors running at process exit.  Call it once before exit (the Python
 * package registers it with atexit; the Rust shim calls it from Drop of its
 * runtime guard).  Images, pipelines and buffers the caller still holds must be
 * freed first; the library may be used again afterwards (ik_init).  Callers
 * still inside the library on other threads return first: every entry point
 * holds the library's lifetime lock shared, teardown takes it exclusively. */
int ik_shutdown(void);
/* ik_shutdown for process exit, when threads of the caller (a server's daemon
 * request threads) may still call in: afterwards every entry point that does
 * device work returns IK_ERR_INVALID ("closed") instead of bringing the library
 * back up.  The Python package registers this one with atexit. */
int ik_close(void);
/* bytes the library holds, by pool (n <= 7 values): [0] device image blocks in
 * use, [1] image blocks kept free for reuse, [2] per-thread device arenas, [3]
 * per-thread pinned arenas, [4] upload areas (device), [5] upload areas (pinned),
 * [6] cached resize plans' device tables */
int ik_memory_stats(uint64_t *out, int n);
size_t ik_last_error(char *buf, size_t cap); /* thread-local message of the last failure */
const char *ik_version(void);

/* ---- image handles ---------------------------------------------------- */
/* ImageBuffer::from_raw: copy a tightly packed host buffer to the device */
int ik_image_from_host(const uint8_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                       ik_image **out);
/* wrap an existing device buffer (not owned; must outlive the handle) */
int ik_image_wrap_device(uint8_t *dev_pixels, uint32_t width, uint32_t height, uint32_t channels,
                         size_t pitch, ik_image **out);
int ik_image_info(const ik_image *img, uint32_t *width, uint32_t *height, uint32_t *channels);
/* 16-bit images (Rgb16 / Rgba16 / L16 / La16 of DynamicImage; 16-bit PNG decodes to
 * them): bytes per sample, 1 or 2; ik_image_to_host writes native-endian u16 for 2.
 * resize_image keeps the depth; encode_image rescales to 8 bits first (to_rgb8). */
int ik_image_depth(const ik_image *img);
int ik_image_from_host16(const uint16_t *pixels, uint32_t width, uint32_t height, uint32_t channels,
                         ik_image **out);
int ik_image_to_host(const ik_image *img, uint8_t *dst, size_t cap); /* tightly packed */
void ik_image_free(ik_image *img);
void ik_buf_free(uint8_t *buf);

/* ---- caller-pinned input memory ------------------------------------------ */
/* Encoded inputs in page-locked host memory are DMAed to the GPU in place (no
 * staging copy): a server reads request bodies into buffers from ik_host_alloc
 * (or registers its own buffer arena once with ik_host_register).  Inputs in
 * ordinary memory work too; they are copied through pinned staging first. */
int ik_host_alloc(size_t bytes, void **out);  /* page-locked, usable by every device */
int ik_host_free(void *p);                     /* only for ik_host_alloc memory */
int ik_host_register(void *p, size_t bytes);   /* page-lock an existing range */
int ik_host_unregister(void *p);               /* the start of a registered range */

/* ---- the three reference functions ------------------------------------ */
/* decode_image (src/transform.rs:27-43): guess_format + load_from_memory_with_format.
 * *fmt_out = IK_FORMAT_* for webp/jpeg/avif, -1 (None) for other formats. */
int ik_decode(const uint8_t *bytes, size_t len, ik_image **out, int *fmt_out);

/* decode_image over n inputs at once (the /img handler under load).  Baseline
 * JPEG scans (with or without restart markers) are entropy-decoded together by
 * the self-synchronising GPU decoder (a few launches for the whole batch) and
 * reconstructed on the GPU; PNG streams go through the batched GPU inflate; lossy
 * WebP files (no animation; with an alpha plane only under
 * ik_set_webp_alpha_decode(IK_WEBP_ALPHA_GPU), which is off by default) are parsed on
 * the host workers and reconstructed together by one set of GPU launches
 * (IK_WEBP_DECODE=auto: when they total 3 MPix; the other WebP kinds by libwebp);
 * inputs of any other kind get
 * ik_decode's verdict.  outs[i] / fmts[i] / status[i] per input (outs[i]
 * NULL on failure; fmts and status may be NULL); returns the first failure or
 * IK_OK. */
int ik_decode_batch(const uint8_t *const *bytes, const size_t *lens, uint32_t n, ik_image **outs,
                    int *fmts, int *status);

/* PNG decoding on the GPU (ik_decode / ik_decode_batch / ik_transform*): streams
 * whose filtered image data is at least min_raw_bytes are inflated and unfiltered
 * on the GPU (parallel DEFLATE over block-start candidates, row-wavefront
 * unfilter), every colour type included (palette, low bit depths, tRNS, 16-bit),
 * interlaced (Adam7) streams too: their seven pass images are unfiltered side by
 * side and gathered into the image by one more kernel; smaller ones and any the
 * GPU finds inconsistent use the host decoder.  -1 = host decoder only.  Default 256 KiB
 * (IK_PNG_GPU_MIN; IK_PNG_GPU=0 = off). */
int ik_set_png_gpu_min(long long min_raw_bytes);
/* the last GPU PNG batch finished on the calling thread's device (n <= 17 values):
 * [0] upload stage host ms (parse, staging copies of unpinned inputs, DMA issue),
 * device ms of [1] the upload (first DMA .. gather + CRC done) [2] decode rounds
 * [3] expand [4] resolve [5] unfilter, [6] kernel stage wall ms, [7] decode rounds,
 * [8] decoder lanes, [9] streams sent to the GPU, [10] PNG streams of the batch the
 * GPU decoded, [11] streams the host decoder took (outside the GPU path, or
 * rejected by it), [12] tokens written by the verified decoder lanes (u16 each),
 * device ms of [13] the block search [14] the gather + CRC pass, [15] kernel stage
 * ms until the block search's candidates were back (waiting for the upload
 * included), [16] 1 if the block search ran beside the previous batch's kernels */
int ik_png_last_timing(double *out, int n);
/* the last batch the calling thread's device ran through its kernel stage
 * (ik_transform_batch*): device ms from HIP events on the kernel stream and the
 * algorithmic bytes of the same launches (n <= 13 values): [0] JPEG entropy
 * decoding ms, [1] entropy-coded bytes read, [2] int16 coefficient bytes written,
 * [3] images, [4] decoder lanes; [5] grouped resize ms, [6] resize bytes (C*W*H
 * in + C*w*h out per image), [7] images resized in groups; [8] batched JPEG
 * encoder ms (coefficients + Huffman), [9] images it coded; the host coder stage
 * (libwebp / libavif on the worker pool): [10] wall ms of the batch, [11] thread
 * CPU ms summed over its requests (core-ms), [12] requests it coded */
int ik_batch_last_timing(double *out, int n);
/* process-wide counts of PNG streams decoded since load: out[0] by the GPU path,
 * out[1] by the host decoder (outside the GPU path, or rejected by it) */
int ik_png_counters(unsigned long long *out);
/* the Adam7 pass table of a w x h image of bits_pp bits per pixel, as the GPU
 * decoder lays an interlaced stream out (no GPU needed): for each non-empty pass,
 * in stream order, 8 values in out (room for 7 x 8; may be NULL): x0, y0, dx, dy,
 * pass width, pass height, row bytes, offset of the pass's first filter byte in
 * the inflated stream; *raw_total (may be NULL) = the inflated length.  Returns
 * the number of non-empty passes. */
int ik_png_adam7_plan(uint32_t w, uint32_t h, int bits_pp, uint64_t *out, uint64_t *raw_total);
/* process-wide counts of WebP streams decoded since load (ik_decode and the batch
 * calls alike): out[0] reconstructed by the GPU decoder, out[1] handed to libwebp on
 * the host (outside the GPU path, handed back by it, or by policy) */
int ik_webp_counters(unsigned long long *out);
/* the last batch with WebP inputs finished on the calling thread's device (n <= 13
 * values): [0] wall ms of the host half (partition 0 + tokens of the lossy files,
 * libwebp for the others, on the worker pool), [1] thread CPU ms of partition 0 +
 * tokens summed over the files (core-ms), [2] staging copies + H2D ms, device ms
 * (HIP events) of [3] reconstruction and loop filter [4] upsampling and colour,
 * [5] images the GPU decoded, [6] images handed to libwebp, [7] macroblock rows
 * launched, [8] the reconstruction grid (the largest of the sub-launches),
 * [9] sub-launches, [10] device ms of the alpha planes' un-filtering, [11] thread CPU
 * ms of reading the alpha planes on the host (core-ms; not part of [1]), [12] images
 * with an alpha plane among [5] */
int ik_webp_last_timing(double *out, int n);
/* Where a lossy WebP file that carries an alpha plane (VP8X with the alpha flag and
 * one ALPH chunk) is decoded.  IK_WEBP_ALPHA_HOST, the default: by libwebp on the
 * host, whatever IK_WEBP_DECODE says.  IK_WEBP_ALPHA_GPU: such a file is a lossy file
 * like any other for the GPU decoder -- under IK_WEBP_DECODE=auto its pixels count
 * toward the 3 MPix thresholds, =gpu forces it there, =host keeps it away; the host
 * reads the plane (raw, or lossless-coded through libwebp), the device undoes its
 * prediction filter and writes RGBA.  Off by default because the plane's entropy
 * decode stays on the host and its un-filtering is one wave per plane: until it is
 * measured faster than libwebp at the sizes auto sends, the default stays.
 * Process-wide; -1 returns to the environment, IK_WEBP_ALPHA_DECODE=host|gpu, which
 * is read per call like IK_WEBP_DECODE. */
typedef enum { IK_WEBP_ALPHA_HOST = 0, IK_WEBP_ALPHA_GPU = 1 } ik_webp_alpha_decode;
int ik_set_webp_alpha_decode(int where);
int ik_get_webp_alpha_decode(void);
/* the host half of that path alone (no GPU needed): the alpha plane of a file the GPU
 * decoder would take, still filtered -- *filter 0 none, 1 horizontal, 2 vertical,
 * 3 gradient; *compression 0 raw, 1 lossless -- w * h bytes into plane (cap: its
 * size).  IK_ERR_UNSUPPORTED for a file the GPU path leaves to libwebp. */
int ik_webp_alpha_plane(const uint8_t *bytes, size_t len, uint8_t *plane, size_t cap, uint32_t *w, uint32_t *h,
                        int *filter, int *compression);
/* the pixel total of a batch's lossy WebP files from which IK_WEBP_DECODE=auto
 * takes the GPU batch path */
unsigned long long ik_webp_gpu_min_batch_pixels(void);
/* the launch plan of a batch of lossy WebP frames (no GPU needed): n frames of
 * mb_w[i] x mb_h[i] macroblocks taking bytes[i] of device memory each.  order[k] is
 * the request placed k-th (largest first: by MB rows, then by MBs, then by index);
 * launch_lo (room for n + 1) lists the first k of each sub-launch and then n: the
 * placed frames are cut where the next would take a sub-launch past cap_bytes, and a
 * frame above the cap is alone in its own; row_start (n + 1 values) is the MB-row
 * ticket of each placed frame's first row, restarting at 0 in each sub-launch, and
 * row_start[n] the MB rows of the last sub-launch.  Returns the sub-launch count
 * (0 for n = 0). */
int ik_webp_batch_plan(const uint32_t *mb_w, const uint32_t *mb_h, const uint64_t *bytes, uint32_t n,
                       uint64_t cap_bytes, uint32_t *order, uint32_t *row_start, uint32_t *launch_lo);
/* process-wide JPEG counters: out[0] = streams whose entropy decoding ran on the
 * GPU (restart intervals or self-synchronising scans), out[1] = on the host */
int ik_jpeg_counters(unsigned long long *out);
/* process-wide counters of the JPEG files of device-resident batches
 * (ik_transform_batch_submit_device): out[0] = taken in place, out[1] = copied back
 * to the host before parsing, out[2] = taken in place but copied back later for the
 * host decoder (these count in out[0] too) */
int ik_jpeg_device_counters(unsigned long long *out);
/* device time (HIP events, ms) of the last marker-walk launch of a device-resident
 * batch, process-wide; 0 before the first */
double ik_jpeg_device_walk_ms(void);
/* Where the baseline JPEG files of a device-resident batch are read from.
 * IK_JPEG_DEVICE_INPLACE, the default: where they lie.  IK_JPEG_DEVICE_COPY: every
 * JPEG is copied back to the host at submit, as before in-place decoding existed
 * (for A/B runs; the outputs are identical).  Process-wide; -1 returns to the
 * environment, IK_JPEG_DEVICE=inplace|copy, which is read per batch. */
typedef enum { IK_JPEG_DEVICE_COPY = 0, IK_JPEG_DEVICE_INPLACE = 1 } ik_jpeg_device;
int ik_set_jpeg_device(int where);
int ik_get_jpeg_device(void);

/* Where a progressive JPEG (SOF2, 8-bit) without restart markers is entropy-decoded.
 * IK_JPEG_PROG_FREE_HOST, the default: on a host core, scan by scan.
 * IK_JPEG_PROG_FREE_GPU: on the GPU, when no scan of the file has a restart interval in
 * force and its entropy-coded bytes, over all scans, come to 4 KiB or more -- the DC and
 * AC first scans through the self-synchronising decoder's launches, together with the
 * batch's baseline files; DC refinement one bit per block; AC refinement, which does not
 * synchronise by itself, as one serial chain per component: one GPU lane per chain, which
 * takes about 1.5 s for a 2000 x 2000 file and about 6 s for a 4096 x 4096 one, in one
 * launch, where a host core decodes the whole file in 67 ms -- the switch is for
 * measurement, not for production.  A file whose first scans overlap, or that refines a
 * band before coding it, stays on the host, which applies scans in file order.  The
 * pixels are the same either way; a file the GPU finds inconsistent goes to the host
 * decoder, which reports the reference's error.  Files in device memory are copied back at submit as before.
 * -1 returns to the environment, IK_JPEG_PROG_FREE=host|gpu, read per file.
 * IK_JPEG_PROG=0 keeps every progressive scan on the host and wins over this switch.
 * ik_jpeg_counters counts a file decoded this way as GPU-decoded. */
typedef enum { IK_JPEG_PROG_FREE_HOST = 0, IK_JPEG_PROG_FREE_GPU = 1 } ik_jpeg_prog_free;
int ik_set_jpeg_prog_free(int where);
int ik_get_jpeg_prog_free(void);
/* Device milliseconds (HIP events) of the last batch that decoded such files on the GPU:
 * out[0] the self-synchronising launches (shared with the batch's baseline files), out[1]
 * the DC refinement launches, out[2] the AC refinement chains.  A development aid
 * (tools/jpeg_prog_bench.py): the three values are process-wide, and decoding threads that
 * run such batches at the same time overwrite each other's. */
int ik_jpeg_prog_free_ms(double *out);
/* The marker walk behind in-place decoding, run on host bytes (no GPU needed; the
 * same code as the kernel's).  skeleton (cap >= IK_JPEG_SKELETON_BYTES) receives SOI
 * and, verbatim and in order, the DQT, DHT, SOFn, DRI, APP0 and APP14 segments and
 * the first SOS header -- itself a JPEG header the parser reads; every other segment
 * is stepped over.  verdict: 0 in place, 1 copy back, 2 malformed (copied back:
 * the host parser words the error).  reason: 0 none, 1 not one SOF0/SOF1 8-bit
 * frame, 2 first scan under 4 KiB, 3 no SOS, 4 skeleton too large, 5 the first SOS
 * names fewer components than the frame, 6 bytes between segments, 7 a segment
 * length past the file's end, 8 no SOI.  entropy_offset: the first scan's first
 * byte (0 when no SOS was reached); eoi_offset: the last FF D9 among the file's
 * last 4 KiB and not before the scan, else len. */
#define IK_JPEG_SKELETON_BYTES 4096
typedef struct {
    int verdict, reason;
    int sof_marker;            /* 0xC0..0xCF, 0 = none */
    uint32_t skeleton_len;
    uint64_t entropy_offset, eoi_offset;
} ik_jpeg_walk_info;
int ik_jpeg_walk_host(const uint8_t *bytes, size_t len, uint8_t *skeleton, size_t cap, ik_jpeg_walk_info *info);

/* resize_image (src/transform.rs:62-90).  w/h < 0 mean None.  Both None returns
 * the input unchanged (*out == img); otherwise a new image (img is not freed:
 * the Rust shim drops its by-value argument).  filter: IK_FILTER_* (Lanczos3 in
 * the reference). */
int ik_resize(ik_image *img, int64_t w, int64_t h, int filter, ik_image **out);
/* The window a W x H image's request (w, h; negative = None, not both) computes under
 * `fit` (ik_fit): out[6] = iw, ih, x0, y0, nw, nh.  Needs no device.  IK_OK, or
 * IK_ERR_INVALID: a dimension, or the fitted / covering size, above u32 (as ik_resize). */
int ik_fit_target(uint32_t W, uint32_t H, int64_t w, int64_t h, int fit, uint32_t *out);
/* ik_resize under a fit mode (ik_fit); IK_FIT_CONTAIN is ik_resize.  8- and 16-bit images. */
int ik_resize_fit(ik_image *img, int64_t w, int64_t h, int fit, int filter, ik_image **out);

/* Resampler arithmetic.  IK_RESIZE_EXACT (default): image 0.25.8's f32 sequence,
 * separately rounded multiply and add per tap -- bit-exact.  IK_RESIZE_FMA: one
 * fused multiply-add per tap -- within +-1 LSB per channel (the north star's
 * tolerance for bilinear/Lanczos), fewer vector instructions.  Process-wide; the
 * default also comes from IK_RESIZE_MODE=exact|fma when first used. */
typedef enum { IK_RESIZE_EXACT = 0, IK_RESIZE_FMA = 1 } ik_resize_mode;
int ik_set_resize_mode(int mode);
int ik_get_resize_mode(void);
/* The resampler kernel a launch of this geometry takes under the current modes
 * (for profiles and benchmarks): "k_resize_periodic" (integer vertical ratios),
 * "k_resize_fused", or "k_vert_naive" (the two-pass fallback); NULL on bad
 * arguments or without a device. */
const char *ik_resize_kernel_name(uint32_t W, uint32_t H, uint32_t C, uint32_t nw, uint32_t nh, int filter);
/* The variant a launch of n images of this geometry takes under the current
 * modes, for tests: out[0..] = slots (A), rows (R), flush (F), weights_in_lds,
 * NS (column strips), NB (bands of the fused plan), per_A, per_R, NBp (bands of
 * the periodic plan; per_A = 0: the geometry is not periodic), Tx, Ty,
 * max_strip_cols, kernel family (0 "k_vert_naive", 1 "k_resize_fused",
 * 2 "k_resize_periodic", for rows W * C bytes apart).  Computed from the geometry
 * alone: needs no device.  The device path caches plans by geometry and fused band
 * height, not by n, while the periodic bands depend on n: where two launch sizes
 * share a band height but not a periodic one (outputs of thousands of rows), a
 * launch may reuse the plan first built, and NBp here is then that of n alone.
 * Fills at most cap values; returns how many there are
 * (IK_RESIZE_PLAN_INFO_LEN), or a negative value on bad arguments. */
#define IK_RESIZE_PLAN_INFO_LEN 13
int ik_resize_plan_info(uint32_t W, uint32_t H, uint32_t C, uint32_t nw, uint32_t nh, int filter, uint32_t n,
                        int32_t *out, int cap);
/* The same values for the launch that computes columns [x0, x0 + nw) and rows
 * [y0, y0 + nh) of the image resampled to iw x ih (ik_resize_window). */
int ik_resize_plan_info_window(uint32_t W, uint32_t H, uint32_t C, uint32_t iw, uint32_t ih, uint32_t x0, uint32_t y0,
                               uint32_t nw, uint32_t nh, int filter, uint32_t n, int32_t *out, int cap);

/* JPEG reconstruction behind decode_image (src/transform.rs:31 -> image 0.25.8
 * -> zune-jpeg 0.4.21, Cargo.lock:3106).  IK_JPEG_RECON_ZUNE (default): zune-jpeg's
 * integer IDCT (stb_image-derived, DC-only shortcut), upsampler and i16 YCbCr->RGB,
 * restated (parity unpinned: no zune-jpeg in this environment).
 * IK_JPEG_RECON_LIBJPEG: libjpeg-turbo's islow IDCT, fancy upsampling and
 * jdcolor.c -- bit-exact with Pillow's decoder.  Entropy decoding is the same in
 * both.  Process-wide; the default also comes from IK_JPEG_RECON=zune|libjpeg. */
typedef enum { IK_JPEG_RECON_LIBJPEG = 0, IK_JPEG_RECON_ZUNE = 1 } ik_jpeg_recon;
int ik_set_jpeg_reconstruction(int mode);
int ik_get_jpeg_reconstruction(void);

/* imageops::resize to exact dimensions (the resampler under resize_image) */
int ik_resize_exact(const ik_image *img, uint32_t nw, uint32_t nh, int filter, ik_image **out);
/* Columns [x0, x0 + nw) and rows [y0, y0 + nh) of ik_resize_exact(img, iw, ih): the same
 * pixels as resizing and then cropping, computed from the window's own weight-table rows
 * and the source columns and rows they read (the primitive under IK_FIT_COVER).  iw x ih
 * equal to the image's size copies the window, as ik_resize_exact copies the image.  A
 * window that is empty or not inside iw x ih: IK_ERR_INVALID. */
int ik_resize_window(const ik_image *img, uint32_t iw, uint32_t ih, uint32_t x0, uint32_t y0, uint32_t nw,
                     uint32_t nh, int filter, ik_image **out);

/* encode_image (src/transform.rs:113-150): quality clamped to [1,100].
 * *out is allocated by the library; release with ik_buf_free. */
int ik_encode(const ik_image *img, int fmt, int quality, uint8_t **out, size_t *out_len);

/* WebP coder behind encode_image (src/transform.rs:129-137); every choice writes the
 * bytes of the reference's webp 0.3.1 -> libwebp WebPEncodeRGB.
 * IK_WEBP_LIBWEBP: libwebp's VP8 coder on host threads over device-made YUV420 planes.
 * IK_WEBP_EXACT: libwebp's own method-4 decisions on the GPU (segment analysis, RD mode
 *   search, token statistics: ik_webp_encode_exact_device) and its bitstream on the
 *   host -- the same files, with the coding off the host cores.
 * IK_WEBP_AUTO (the default): the exact GPU coder for a batch's same-geometry groups
 *   of 32 or more images and pipelines of max_batch >= 32 (its chain of macroblock steps costs
 *   about as much for 64 images as for one), libwebp for smaller groups and lone
 *   images (one host core codes a 512^2 image in ~8 ms, the GPU chain takes ~18).
 * The process default comes from IK_WEBP_ENCODER=auto|exact|libwebp when first used.
 * (Value 1, a non-exact GPU VP8 encoder of earlier rounds, is retired: refused.) */
typedef enum { IK_WEBP_LIBWEBP = 0, IK_WEBP_EXACT = 2, IK_WEBP_AUTO = 3 } ik_webp_encoder;
int ik_set_webp_encoder(int encoder); /* process-wide, for ik_encode / ik_transform */
/* version of the libwebp that codes WebP (WebPGetEncoderVersion, e.g. 0x010600),
 * -1 when none could be loaded.  The codec libraries are explicit dependencies:
 * IK_LIBWEBP=<path> / IK_LIBAVIF=<path> when set, else the system sonames
 * libwebp.so.7 / libavif.so.16 through the dynamic loader (no other search). */
int ik_libwebp_version(void);
/* path of the library that codes fmt (IK_FORMAT_WEBP / IK_FORMAT_AVIF) into buf
 * (NUL-terminated, truncated to cap); returns its length, 0 when none loaded */
size_t ik_codec_library(int fmt, char *buf, size_t cap);
int ik_get_webp_encoder(void);

/* ---- EXIF orientation -------------------------------------------------- */
/* image 0.25.8 offers ImageDecoder::orientation(), Orientation::from_exif and
 * DynamicImage::apply_orientation; the reference's decode_image never calls them
 * (src/transform.rs:27-43), and neither does any entry point above: a file's pixels are
 * decoded as stored.  The calls below are the opt-in equivalent, pixels staying in HBM.
 * With S the stored image, H rows by W columns, orientation o gives out[y][x]:
 *   1 S[y][x]        2 S[y][W-1-x]    3 S[H-1-y][W-1-x]    4 S[H-1-y][x]        (W x H)
 *   5 S[x][y]        6 S[H-1-x][y]    7 S[H-1-x][W-1-y]    8 S[x][W-1-y]        (H x W)
 * (6 turns 90 degrees clockwise, 8 counter-clockwise; the mapping is recalled and pinned
 * to Pillow's ImageOps.exif_transpose) */
/* The file's EXIF Orientation, 1..8: JPEG APP1 before the first SOS, PNG eXIf, WebP
 * (VP8X) EXIF chunk; IFD0 only, tag 0x0112 as one SHORT.  1 when there is none, for any
 * other format, and for a malformed or truncated file: never an error, never a read past
 * len.  Needs no device (csrc/ik_exif.h). */
int ik_exif_orientation(const uint8_t *bytes, size_t len);
/* the `orient` argument of the *_oriented calls: IK_ORIENT_STORED, the pixels as stored
 * (the calls without the argument); IK_ORIENT_AUTO, ik_exif_orientation of the bytes;
 * 1..8, that value whatever the file says (a caller's rotate= parameter).  Anything else
 * is IK_ERR_INVALID. */
typedef enum { IK_ORIENT_AUTO = -1, IK_ORIENT_STORED = 0 /* 1..8: apply that EXIF value */ } ik_orient;
/* DynamicImage::apply_orientation as a new image (orientation 1: a copy); 8- and 16-bit */
int ik_image_orient(const ik_image *img, int orientation /* 1..8 */, ik_image **out);
/* ik_decode, then the turn.  An effective orientation of 1 adds no pass. */
int ik_decode_oriented(const uint8_t *bytes, size_t len, int orient, ik_image **out, int *fmt_out);
/* the edge of the transposing kernel's square tile and the row kernel's strip, in
 * pixels (the sizes at which the kernels' edge handling changes; for tests) */
int ik_orient_tile(void);
int ik_orient_strip(void);

/* ---- background flatten ------------------------------------------------- */
/* encode_image goes through to_rgb8 for JPEG and WebP, which drops the alpha channel: the
 * colours under alpha 0 become visible, and the (non-premultiplying, bit-exact) resampler
 * has already bled them into opaque edges.  The calls below are the opt-in remedy: the
 * decoded image composited onto a constant colour BEFORE the resize, pixels staying in HBM.
 * The image crate has no such call; the arithmetic is this project's own definition
 * (DESIGN section 4).  With the background b per channel given as 0xRRGGBB, a sample c with
 * alpha a, and M = 255 (8-bit) or 65535 (16-bit, where b = b8 * 257):
 *     out = (c*a + b*(M - a) + M/2) / M        (integers, floor division)
 * the integer nearest to the exact quotient (M is odd: no ties); a = 0 gives b, a = M gives c.
 *     Rgba                          -> Rgb
 *     LumaA, colour with R == G == B -> Luma
 *     LumaA, any other colour        -> Rgb (luma replicated, as to_rgb8 replicates it)
 *     Luma, Rgb                      -> as they are: no pass
 * The depth is kept.  Flatten-then-resize equals a premultiplied resample followed by the
 * composite, apart from one rounding of the flattened pixels to integers (the resampler is
 * linear and its weights sum to 1), so no transparent pixel's colour reaches an output. */
#define IK_BG_NONE (-1)
/* the image flattened onto `background` (0x000000..0xFFFFFF) as a new image on the device
 * that holds img; an image without alpha, or IK_BG_NONE, gives a copy.  Any other
 * background is IK_ERR_INVALID. */
int ik_image_flatten(const ik_image *img, int32_t background, ik_image **out);
/* the pixels of a row one workgroup of the flatten kernel takes, and the most rows of
 * workgroups in a launch (further rows are grid-strided): the sizes at which the kernel's
 * edge handling changes; for tests */
int ik_flatten_span(void);
int ik_flatten_row_cap(void);
/* process-wide: out[0] flatten kernel launches, out[1] images flattened by them */
int ik_flatten_counters(unsigned long long out[2]);

/* ---- per-request options ------------------------------------------------ */
/* What the *_opts entry points take for each request, in place of one suffixed entry
 * point per option.  Defaults: IK_FIT_CONTAIN, IK_ORIENT_STORED, IK_BG_NONE; with every
 * request at its defaults (or opts NULL) an *_opts call makes the very calls of the entry
 * point without options.  The order is decode -> orient -> flatten -> resize -> encode: fit,
 * w and h refer to the oriented image, and the background applies whatever the output
 * format (an AVIF request with a background is opaque and carries no alpha plane).
 * opt_size must be the size of a layout this header declares (ik_request_opts, or
 * ik_request_opts2, ik_request_opts3, ik_request_opts4 and ik_request_opts5 below); any other value is IK_ERR_INVALID ("unknown options size")
 * before any device work, which is what lets the struct grow.  A fit outside ik_fit, an orient outside ik_orient / 1..8 and a background
 * that is neither IK_BG_NONE nor 0x000000..0xFFFFFF are IK_ERR_INVALID. */
typedef struct {
    int fit;            /* ik_fit */
    int orient;         /* ik_orient, or 1..8 */
    int32_t background; /* IK_BG_NONE, or 0xRRGGBB */
} ik_request_opts;
/* The second declared layout, 24 bytes: the first one's fields, then blur and unsharpen
 * (below).  The *_opts entry points take `const void *opts` and accept either declared
 * size in opt_size; in a batch the n structs lie opt_size bytes apart.  The new fields at
 * zero (their defaults) make exactly the calls the 12-byte layout makes.  A sigma is 0.0
 * (off) or within [0.0625, IK_BLUR_MAX_SIGMA]; negative, NaN, infinite or out of range is
 * IK_ERR_INVALID, as is a threshold outside 0..65535 and a request with both sigmas set
 * ("blur and sharpen together": one request makes at most one extra pass), all before any
 * device work; in a batch the message names the request.  The order is decode -> orient ->
 * flatten -> resize -> blur or sharpen -> encode: the filter sees the pixels the encoder
 * codes (with w and h both None, the decoded image after orient and flatten). */
typedef struct {
    int fit;                   /* ik_fit */
    int orient;                /* ik_orient, or 1..8 */
    int32_t background;        /* IK_BG_NONE, or 0xRRGGBB */
    float blur_sigma;          /* 0: no blur */
    float sharpen_sigma;       /* 0: no unsharp mask */
    int32_t sharpen_threshold; /* 0..65535, in the sample's own units (8- or 16-bit) */
} ik_request_opts2;

/* ---- blur and unsharpen ---------------------------------------------------- */
/* A Gaussian blur of the caller's sigma and the unsharp mask built on it, pixels staying in
 * HBM.  The project's own definition, modelled on image 0.25.8's
 * imageops::blur and imageops::unsharpen as recalled; parity with the crate is not pinned.
 * It is the resampler's arithmetic at ratio 1.  For an axis of L samples, all in f32:
 *     gaussian(x) = (1 / (sqrtf(2 pi) * sigma)) * expf(-(x * x) / (2 * (sigma * sigma)))
 *     support = 2 * sigma;  for output o:  c = o + 0.5
 *     left = clamp(floorf(c - support), 0, L - 1);  right = clamp(ceilf(c + support), left + 1, L)
 *     w[k] = gaussian((left + k) - (c - 0.5)), summed in order, each divided by the sum
 * Blur: a vertical pass over every sample column (channels independently, alpha included),
 * t = 0 then t = t + (float)S * w[k] for ascending k, product and sum rounded separately,
 * into an f32 image that is neither clamped nor rounded; the same pass horizontally over
 * it; then clamp(t, 0, M) rounded to nearest, halves away from zero (M = 255 or 65535).
 * Unsharpen: with B the blur, d = S - B per sample and out = |d| > threshold ?
 * clamp(S + d, 0, M) : S.  Channels and depth are kept.  The sequence is always this one:
 * IK_RESIZE_FMA does not apply.  sigma <= 0.25 gives one tap of weight 1, the identity. */
#define IK_BLUR_MAX_SIGMA 32.0f
/* the weight table of one axis; needs no device.  *taps receives T, the taps of the widest
 * output.  With left, count and weights all NULL that is all; otherwise left[o] and
 * count[o] for each of the L outputs and weights[o * cap_taps + k], zero from count[o] on,
 * and cap_taps < T is IK_ERR_INVALID (*taps is set).  sigma must lie in
 * [0.0625, IK_BLUR_MAX_SIGMA], L in 1..2^24. */
int ik_blur_axis_plan(uint32_t L, float sigma, int32_t *left, int32_t *count, float *weights, uint32_t cap_taps,
                      uint32_t *taps);
/* the image blurred, or sharpened by the unsharp mask, as a new image on the device that
 * holds img (8- and 16-bit; img is not changed).  sigma as above (0 is IK_ERR_INVALID here),
 * threshold 0..65535: one at or above M never triggers. */
int ik_image_blur(const ik_image *img, float sigma, ik_image **out);
int ik_image_unsharpen(const ik_image *img, float sigma, int32_t threshold, ik_image **out);
/* out[0], out[1]: the columns and rows of the output tile one workgroup of the kernel owns,
 * the sizes at which its edge handling changes; for tests */
int ik_blur_tile(int out[2]);
/* process-wide: out[0] blur kernel launches, out[1] images filtered by them */
int ik_blur_counters(unsigned long long out[2]);

/* ---- watermark overlay ---------------------------------------------------- */
/* One image (a logo, a line of text) composited over another before it is encoded, pixels
 * staying in HBM.  The project's own definition, all integers.  B is
 * the base, W x H, C channels, M = 255 or 65535; O the overlay, wo x ho, any of the
 * channel counts and depths; neither the base's channels nor its depth change, and the
 * overlay is never resized or turned (prepare it once with the calls above).
 *   depth     overlay samples, alpha included, go to the base's depth first: 8 -> 16
 *             v * 257, 16 -> 8 (v + 128) / 257
 *   channels  no alpha: fa = M; a gray overlay is replicated onto a colour base; a colour
 *             overlay on a gray base gives L = (2126 R + 7152 G + 722 B) / 10000 (floor)
 *   opacity   op in 1..255, opM = op or op * 257; a = (fa * opM + M / 2) / M
 *   C 1 or 3  out = (f * a + c * (M - a) + M / 2) / M per colour sample
 *   C 2 or 4  Porter-Duff "over" on straight alpha, ca the base's alpha:
 *             t = ca * (M - a), D = a * M + t, out_a = (D + M / 2) / M; D == 0 leaves the
 *             pixel; else out_c = (f * a * M + c * t + D / 2) / D  (ca = M: the line above)
 *   place     x0 is 0, floor((W - wo) / 2) or W - wo by the gravity (floor towards minus
 *             infinity), then x0 += dx; y0 likewise; |dx|, |dy| <= 2^24.  The window is
 *             the overlay's rectangle clipped to the base; empty: nothing changes and
 *             nothing is launched
 *   tile      the window is the whole base and pixel (x, y) takes
 *             O[(x - x0) mod wo, (y - y0) mod ho], the Euclidean mod */
enum ik_gravity {
    IK_GRAVITY_CENTER = 0,
    IK_GRAVITY_N = 1,
    IK_GRAVITY_S = 2,
    IK_GRAVITY_E = 3,
    IK_GRAVITY_W = 4,
    IK_GRAVITY_NE = 5,
    IK_GRAVITY_NW = 6,
    IK_GRAVITY_SE = 7,
    IK_GRAVITY_SW = 8
};
/* the placement; needs no device.  out[0..3]: the window x, y, w, h in the base (all four 0
 * when it is empty), out[4], out[5]: the overlay's origin x0, y0.  W, H <= 2^24 (0 allowed:
 * an empty window), wo, ho in 1..2^24.  Every other call computes its window through this. */
int ik_overlay_place(uint32_t W, uint32_t H, uint32_t wo, uint32_t ho, int gravity, int32_t dx, int32_t dy, int tile,
                     int32_t out[6]);
/* img under the overlay as a new image on the device that holds img (a device copy, then
 * the kernel in place on it; img is not changed).  opacity 1..255.  An overlay held by
 * another device is copied over for the call. */
int ik_image_overlay(const ik_image *img, const ik_image *overlay, int gravity, int32_t dx, int32_t dy, int opacity,
                     int tile, ik_image **out);
/* the window columns one workgroup of the kernel takes, the size at which its edge handling
 * changes; for tests */
int ik_overlay_span(void);
/* process-wide: out[0] overlay kernel launches, out[1] images composited by them */
int ik_overlay_counters(unsigned long long out[2]);

/* The third declared layout, 56 bytes: ik_request_opts2's 24, then a watermark composited
 * on the pixels the encoder codes: decode -> orient -> flatten -> resize -> blur or sharpen
 * -> overlay -> encode (the mark is not blurred).  overlay NULL means none; the other
 * overlay fields must then be zero, and the call makes exactly the calls of the 24-byte
 * layout.  An unknown gravity, an opacity outside 0..255, a tile outside 0/1, a non-zero
 * reserved and offsets beyond +-2^24 are IK_ERR_INVALID before any device work; in a batch
 * the message names the request.  LIFETIME: the overlay handle is the caller's; it must
 * stay alive (not freed, its pixels not written) until the call returns, and for a
 * submitted ticket until ik_transform_batch_wait has returned for it.  One handle may
 * serve any number of requests and calls at once.  In a batch, members of a resize group
 * that share (handle, gravity, dx, dy, opacity, tile) are composited by one launch. */
typedef struct {
    int fit;                   /* ik_fit */
    int orient;                /* ik_orient, or 1..8 */
    int32_t background;        /* IK_BG_NONE, or 0xRRGGBB */
    float blur_sigma;          /* 0: no blur */
    float sharpen_sigma;       /* 0: no unsharp mask */
    int32_t sharpen_threshold; /* 0..65535 */
    const ik_image *overlay;   /* NULL: no watermark */
    int32_t overlay_gravity;   /* ik_gravity */
    int32_t overlay_dx;        /* added to the gravity's origin, pixels */
    int32_t overlay_dy;
    int32_t overlay_opacity;   /* 0 means 255 (a zeroed struct with only `overlay` set is an
                                  opaque centred mark), else 1..255 */
    int32_t overlay_tile;      /* 0 or 1 */
    int32_t reserved;          /* must be 0 */
} ik_request_opts3;
#ifdef __cplusplus
static_assert(sizeof(ik_request_opts3) == 56, "ik_request_opts3 is 56 bytes");
#else
_Static_assert(sizeof(ik_request_opts3) == 56, "ik_request_opts3 is 56 bytes");
#endif

/* ---- colour adjustments ---------------------------------------------------- */
/* Grayscale, brightness, contrast, saturation, hue, gamma and invert on the pixels' values,
 * pixels staying in HBM.  The project's own definition.  The host turns
 * the six numbers into a PLAN, a colour matrix and a tone table, in f64; the device applies
 * the plan with integers only.  M = 255 or 65535.
 *   matrix  l = (0.2126, 0.7152, 0.0722), L the matrix whose every row is l, I the identity;
 *           s = 1 + saturation / 100;  Sat = L + s (I - L);  t = hue * pi / 180;
 *           Hue = L + cos t (I - L) + sin t S  (SVG hueRotate),
 *           S = [[-l0, -l1, 1 - l2], [0.143, 0.140, -0.283], [-(1 - l0), l1, l2]];
 *           m = Hue Sat;  Q16: off the diagonal q = floor(m * 65536 + 0.5), on it 65536 minus
 *           the row's other two, so every row sums to 65536 and R = G = B stays itself
 *   pixel   C >= 3:  o_i = clamp((q[i][0] R + q[i][1] G + q[i][2] B + 32768) >> 16, 0, M), the
 *           shift arithmetic.  C 1 or 2: the matrix is not applied (it would be the identity)
 *   table   then every colour sample v becomes T[v]:  x = v / M + brightness / 100;
 *           k = ((100 + contrast) / 100)^2;  x = clamp((x - 0.5) k + 0.5, 0, 1);
 *           gamma != 0: x = pow(x, 1 / gamma);  invert: x = 1 - x;  T[v] = floor(x M + 0.5)
 * Alpha is never touched; channels and depth never change.  All six at zero is "no
 * adjustment": nothing is launched.  saturation -100 is grayscale. */
typedef struct {
    int32_t brightness; /* -100..100, 0: none */
    int32_t contrast;   /* -100..100, 0: none */
    int32_t saturation; /* -100..100, 0: none, -100: grayscale */
    int32_t hue;        /* degrees, -360..360, 0: none */
    float gamma;        /* 0.0: none, else 0.1..10.0 */
    int32_t invert;     /* 0 or 1 */
} ik_adjust;
#ifdef __cplusplus
static_assert(sizeof(ik_adjust) == 24, "ik_adjust is 24 bytes");
#else
_Static_assert(sizeof(ik_adjust) == 24, "ik_adjust is 24 bytes");
#endif
/* the plan; needs no device.  depth 1 or 2.  table (or NULL) receives the M + 1 entries of
 * T, matrix (or NULL) the nine Q16 coefficients row by row, *flags (or NULL) bit 0: the
 * matrix is not the identity, bit 1: the table is not the identity.  A field out of range
 * (gamma: NaN, infinite, or neither 0 nor within 0.1..10) is IK_ERR_INVALID.  Every other
 * call builds its plan through this. */
int ik_adjust_plan(const ik_adjust *adj, int depth, uint16_t *table, int32_t matrix[9], int *flags);
/* img adjusted as a new image on the device that holds img (a device copy, then the kernel
 * in place on it; img is not changed).  A plan with flags 0 (all six at zero, a gray image
 * under a matrix alone) gives the copy and launches nothing. */
int ik_image_adjust(const ik_image *img, const ik_adjust *adj, ik_image **out);
/* the pixels of a row one workgroup of the kernel takes, the size at which its edge handling
 * changes; for tests */
int ik_adjust_span(void);
/* process-wide: out[0] adjust kernel launches, out[1] images adjusted by them */
int ik_adjust_counters(unsigned long long out[2]);

/* The fourth declared layout, 80 bytes: ik_request_opts3's 56, then an adjustment of the
 * resized pixels: decode -> orient -> flatten -> resize -> adjust -> blur or sharpen ->
 * overlay -> encode (the mark keeps its colours).  With `adjust` all zero the call makes
 * exactly the calls of the 56-byte layout.  A field out of range is IK_ERR_INVALID before
 * any device work; in a batch the message names the request, and members of a resize group
 * whose 24 adjustment bytes are equal are adjusted by one launch. */
typedef struct {
    int fit;                   /* ik_fit */
    int orient;                /* ik_orient, or 1..8 */
    int32_t background;        /* IK_BG_NONE, or 0xRRGGBB */
    float blur_sigma;          /* 0: no blur */
    float sharpen_sigma;       /* 0: no unsharp mask */
    int32_t sharpen_threshold; /* 0..65535 */
    const ik_image *overlay;   /* NULL: no watermark */
    int32_t overlay_gravity;   /* ik_gravity */
    int32_t overlay_dx;
    int32_t overlay_dy;
    int32_t overlay_opacity;   /* 0 means 255, else 1..255 */
    int32_t overlay_tile;      /* 0 or 1 */
    int32_t reserved;          /* must be 0 */
    ik_adjust adjust;          /* all zero: none */
} ik_request_opts4;
#ifdef __cplusplus
static_assert(sizeof(ik_request_opts4) == 80, "ik_request_opts4 is 80 bytes");
#else
_Static_assert(sizeof(ik_request_opts4) == 80, "ik_request_opts4 is 80 bytes");
#endif

/* ---- pad: the output extended onto a canvas --------------------------------- */
/* The image placed on a larger canvas with a frame around it ("fit=pad", extend,
 * letterbox), pixels staying in HBM.  The project's own definition.
 * Channels and depth never change; nothing is blended; alpha is copied like any other
 * channel.  The image I is W x H, M = 255 or 65535.
 *   canvas  cw = max(W, width), ch = max(H, height): an axis the image already fills is
 *           not padded.  cw == W and ch == H: no pass, no launch.
 *   place   x0 = 0, (cw - W) / 2 (floor) or cw - W by the ik_gravity, y0 likewise; no offsets
 *   sample  canvas pixel (x, y) = I[fy(y - y0), fx(x - x0)], n the axis length, i signed:
 *           IK_PAD_EDGE    clamp(i, 0, n - 1)
 *           IK_PAD_WRAP    i mod n, Euclidean
 *           IK_PAD_MIRROR  j = i mod 2n;  j < n ? j : 2n - 1 - j  (the edge sample repeats;
 *                          the index folds as often as the margin needs)
 *           IK_PAD_COLOR   inside the image its pixel, outside the frame pixel
 *   frame   pixel (colour mode): the colour 0xRRGGBB, each channel b * 257 at 16 bits; C 3 or
 *           4: as it is; C 1 or 2: L = (2126 R + 7152 G + 722 B) / 10000, floor, on the
 *           channels at the image's depth (the overlay's gray rule); the alpha sample, where
 *           the image has one: alpha, * 257 at 16 bits */
enum ik_pad_mode { IK_PAD_NONE = 0, IK_PAD_COLOR = 1, IK_PAD_EDGE = 2, IK_PAD_MIRROR = 3, IK_PAD_WRAP = 4 };
typedef struct {
    int32_t mode;    /* ik_pad_mode; IK_PAD_NONE: no pad, and the other five must be 0 */
    int32_t gravity; /* ik_gravity: where the image lies in the canvas */
    int32_t width;   /* the canvas, 0..2^24.  0: ik_image_pad: the image's side; the _opts */
    int32_t height;  /*   calls: the side of the request's target (w, h), "pad to the box" */
    int32_t color;   /* 0xRRGGBB (colour mode) */
    int32_t alpha;   /* 0..255: the frame's alpha where the image has one (colour mode) */
} ik_pad;
#ifdef __cplusplus
static_assert(sizeof(ik_pad) == 24, "ik_pad is 24 bytes");
#else
_Static_assert(sizeof(ik_pad) == 24, "ik_pad is 24 bytes");
#endif
/* the placement; needs no device.  out: cw, ch, x0, y0.  W, H, width, height within
 * 0..2^24 and a known gravity, else IK_ERR_INVALID.  Every other call places through the
 * rule behind this one. */
int ik_pad_place(uint32_t W, uint32_t H, uint32_t width, uint32_t height, int gravity, int32_t out[4]);
/* img on its canvas as a new image on the device that holds img; 8- and 16-bit.  A pad whose
 * canvas is the image gives a copy and launches nothing.  IK_ERR_INVALID: IK_PAD_NONE or an
 * unknown mode or gravity, a size outside 0..2^24, a colour outside 0..0xFFFFFF, an alpha
 * outside 0..255, an empty image under a larger canvas. */
int ik_image_pad(const ik_image *img, const ik_pad *pad, ik_image **out);
/* the canvas pixels of a row one workgroup of the kernel takes, and the most rows of
 * workgroups of a launch (further rows are grid-strided); for tests */
int ik_pad_span(void);
int ik_pad_row_cap(void);
/* process-wide: out[0] pad kernel launches, out[1] images padded by them */
int ik_pad_counters(unsigned long long out[2]);

/* The fifth declared layout, 104 bytes: ik_request_opts4's 80, then a pad of the finished
 * pixels: decode -> orient -> flatten -> resize -> adjust -> blur or sharpen -> pad ->
 * overlay -> encode.  The frame is neither adjusted nor blurred, and the watermark's gravity
 * sees the canvas.  A pad width or height of 0 is the side of the request's target (tw, th)
 * -- w and h with a missing side computed as the resize computes it -- so IK_FIT_CONTAIN
 * with a zero-size pad returns exactly the box asked for; with w and h both None a zero
 * side is the image's.  With pad.mode IK_PAD_NONE the other five fields must be 0 and the
 * call makes exactly the calls of the 80-byte layout.  A field out of range, or fields set
 * without a mode, is IK_ERR_INVALID before any device work; in a batch the message names
 * the request.  In a batch a resize group's members share their canvas and origin as they
 * share their window (a WebP canvas side above 16383 is judged on the canvas); members whose
 * 24 pad bytes are equal are padded by one launch, and requests that differ only in mode,
 * colour or alpha still share the resize and coder groups. */
typedef struct {
    int fit;                   /* ik_fit */
    int orient;                /* ik_orient, or 1..8 */
    int32_t background;        /* IK_BG_NONE, or 0xRRGGBB */
    float blur_sigma;          /* 0: no blur */
    float sharpen_sigma;       /* 0: no unsharp mask */
    int32_t sharpen_threshold; /* 0..65535 */
    const ik_image *overlay;   /* NULL: no watermark */
    int32_t overlay_gravity;   /* ik_gravity */
    int32_t overlay_dx;
    int32_t overlay_dy;
    int32_t overlay_opacity;   /* 0 means 255, else 1..255 */
    int32_t overlay_tile;      /* 0 or 1 */
    int32_t reserved;          /* must be 0 */
    ik_adjust adjust;          /* all zero: none */
    ik_pad pad;                /* all zero: none */
} ik_request_opts5;
#ifdef __cplusplus
static_assert(sizeof(ik_request_opts5) == 104, "ik_request_opts5 is 104 bytes");
#else
_Static_assert(sizeof(ik_request_opts5) == 104, "ik_request_opts5 is 104 bytes");
#endif

/* ---- fused / batched entry points (pixels stay in HBM) ----------------- */
/* decode -> resize_image -> encode_image in one call (handler src/lib.rs:175-191) */
int ik_transform(const uint8_t *bytes, size_t len, int64_t w, int64_t h, int fmt, int quality,
                 int filter, uint8_t **out, size_t *out_len);
/* ik_transform under a fit mode (ik_fit; IK_FIT_CONTAIN is ik_transform) */
int ik_transform_fit(const uint8_t *bytes, size_t len, int64_t w, int64_t h, int fit, int fmt, int quality,
                     int filter, uint8_t **out, size_t *out_len);
/* ik_transform_fit with the decoded image turned first (orient: ik_orient): fit, w and h
 * refer to the oriented image, as apply_orientation followed by resize would in Rust (the
 * turn is never done after the resize: the resampler's f32 sums would run in another
 * order).  IK_ORIENT_STORED, or an effective orientation of 1, is ik_transform_fit: the
 * same calls, no extra pass.  Scheduled over several devices as ik_transform_fit is. */
int ik_transform_oriented(const uint8_t *bytes, size_t len, int64_t w, int64_t h, int fit, int orient, int fmt,
                          int quality, int filter, uint8_t **out, size_t *out_len);
/* ik_transform with per-request options (ik_request_opts above: fit, orientation and
 * background): decode, turn, flatten onto the background, resize, encode.  opts NULL, or at
 * its defaults, is ik_transform: the same calls.  An image without alpha is not touched by
 * a background: no pass, no copy. */
int ik_transform_opts(const uint8_t *bytes, size_t len, int64_t w, int64_t h, int fmt, int quality, int filter,
                      const void *opts, size_t opt_size, uint8_t **out, size_t *out_len);

/* ik_transform over n requests at once (the /img handler under load, loadtest C4
 * mix): decode_image (one set of GPU launches for the batch's PNG streams, one set
 * of self-synchronising entropy launches for its baseline JPEGs), one resize launch
 * per group of
 * same-geometry requests, encode_image (device front ends; libwebp / libavif on
 * `threads` host threads, 0 = default).  w/h (-1 = None), fmt and quality per
 * request; outs[i] (ik_buf_free) / out_lens[i] / status[i] per request (status
 * may be NULL); returns the first failure or IK_OK.  Equivalent to
 * ik_transform_batch_submit + ik_transform_batch_wait. */
int ik_transform_batch(const uint8_t *const *bytes, const size_t *lens, uint32_t n, const int64_t *w,
                       const int64_t *h, const int *fmt, const int *quality, int filter, int threads,
                       uint8_t **outs, size_t *out_lens, int *status);

/* ik_transform_batch as two calls.  Each device runs batches through four
 * stages on their own threads -- upload (the PNG / JPEG files' DMA, in place when
 * the caller pinned them, then a GPU pass that assembles the zlib streams and
 * checks the IDAT CRCs), decode kernels, post (resize and the encoders' device
 * front ends) and host coders (the device's worker pool) -- so consecutive
 * batches overlap: batch k+1's upload runs under batch k's kernels, batch k's
 * resize beside batch k+1's decode, batch k's libwebp beside both.
 * submit queues the batch and returns at once; wait blocks until its bytes are
 * ready, fills status[] (may be NULL) and returns the first failure, as
 * ik_transform_batch does.  Every array passed to submit -- the inputs included
 * -- must stay valid until wait returns; each ticket is waited for exactly once.
 * With several logical devices (ik_init(-1) / IK_DEVICES) a batch goes whole to
 * the least-loaded device, or in parts of at least IK_MIN_DEVICE_BATCH (64)
 * requests to several.  (The reference's handlers, src/lib.rs:175-191, serving
 * many requests at once.) */
int ik_transform_batch_submit(const uint8_t *const *bytes, const size_t *lens, uint32_t n, const int64_t *w,
                              const int64_t *h, const int *fmt, const int *quality, int filter, int threads,
                              uint8_t **outs, size_t *out_lens, int *status, uint64_t *ticket);
int ik_transform_batch_wait(uint64_t ticket);
/* ik_transform_batch / ik_transform_batch_submit with a fit mode (ik_fit) per request;
 * fit NULL, or all IK_FIT_CONTAIN, is the call without it.  Requests resize in one launch
 * when their whole windows agree.  Wait with ik_transform_batch_wait. */
int ik_transform_batch_fit(const uint8_t *const *bytes, const size_t *lens, uint32_t n, const int64_t *w,
                           const int64_t *h, const int *fit, const int *fmt, const int *quality, int filter,
                           int threads, uint8_t **outs, size_t *out_lens, int *status);
int ik_transform_batch_submit_fit(const uint8_t *const *bytes, const size_t *lens, uint32_t n, const int64_t *w,
                                  const int64_t *h, const int *fit, const int *fmt, const int *quality, int filter,
                                  int threads, uint8_t **outs, size_t *out_lens, int *status, uint64_t *ticket);
/* ... and an orientation (ik_orient) per request; orient NULL, or all IK_ORIENT_STORED, is
 * the _fit call.  IK_ORIENT_AUTO is resolved from the bytes at submit, on the host.  The
 * turn runs in the post stage on the device that holds the decoded image, before the
 * post plan (ik_post_plan_fit), which sees the oriented W, H and pitch: images of one
 * (W, H, C, depth, orientation) are turned by one launch, a lone one by its own, and a
 * request whose effective orientation is 1 is not touched.  Wait with
 * ik_transform_batch_wait.  (ik_transform_batch_submit_device has no oriented form: its
 * in-place JPEG marker walk steps over APP1.) */
int ik_transform_batch_oriented(const uint8_t *const *bytes, const size_t *lens, uint32_t n, const int64_t *w,
                                const int64_t *h, const int *fit, const int *orient, const int *fmt,
                                const int *quality, int filter, int threads, uint8_t **outs, size_t *out_lens,
                                int *status);
int ik_transform_batch_submit_oriented(const uint8_t *const *bytes, const size_t *lens, uint32_t n, const int64_t *w,
                                       const int64_t *h, const int *fit, const int *orient, const int *fmt,
                                       const int *quality, int filter, int threads, uint8_t **outs, size_t *out_lens,
                                       int *status, uint64_t *ticket);

/* ik_transform_batch_submit over request bodies already in device memory (HBM)
 * of one device: dev_bytes[i] are device addresses (hipMalloc / ik_dev_alloc),
 * valid until the wait returns.  The batch runs on the device that holds them.
 * PNG files are walked, gathered, CRC-checked and decoded on the GPU where they
 * lie (no PCIe transfer of the compressed bytes).  Baseline JPEG files (one SOF0 /
 * SOF1 frame, 8 bits, every component in a first scan of 4 KiB or more) are decoded
 * in place too: a marker walk on the GPU brings back only the table and frame
 * segments (a few hundred bytes) and two offsets, the host parser reads those, and
 * the self-synchronising decoder reads the scan from the caller's memory -- nothing
 * at or past dev_bytes[i] + lens[i] is read.  Such a file is copied back later, and
 * alone, when the GPU decoder hands it to the host decoder (further scans, a stray
 * marker, a bad code).  Any other item -- other JPEG kinds, WebP, AVIF, malformed
 * files -- and a PNG the GPU path does not take is copied back to host memory
 * first.  The outputs are the same bytes either way (ik_set_jpeg_device).  Outputs,
 * status and errors as ik_transform_batch_submit; wait with ik_transform_batch_wait.
 * (The reference's handlers receive bodies in host memory, src/lib.rs:175-191;
 * this entry serves callers that already hold them on the device.) */
int ik_transform_batch_submit_device(const uint8_t *const *dev_bytes, const size_t *lens, uint32_t n,
                                     const int64_t *w, const int64_t *h, const int *fmt, const int *quality,
                                     int filter, int threads, uint8_t **outs, size_t *out_lens, int *status,
                                     uint64_t *ticket);

/* The batch calls with per-request options: opts holds n ik_request_opts, n
 * ik_request_opts2, n ik_request_opts3, n ik_request_opts4 or n ik_request_opts5 (or is NULL: every request at its defaults, the call without options),
 * opt_size is the size of that layout.  After a resize group's launch and before its
 * coders, its members that share (blur or unsharpen, sigma, threshold) are filtered by one
 * launch, a lone one by its own; requests that differ only in these settings still share
 * the resize and coder groups.
 * IK_ORIENT_AUTO is resolved from the bytes at submit, on the host.  In the post stage, on
 * the device that holds each decoded image, the turn runs first (as in the _oriented
 * calls), then the flatten, then the unchanged post plan, which sees the flattened C and
 * pitch: images of one (W, H, C, depth, pitch, background) are flattened by one launch, a
 * lone one by its own, and a request whose decoded image has no alpha, or whose background
 * is IK_BG_NONE, is not touched.  Wait with ik_transform_batch_wait. */
int ik_transform_batch_opts(const uint8_t *const *bytes, const size_t *lens, uint32_t n, const int64_t *w,
                            const int64_t *h, const void *opts, size_t opt_size, const int *fmt,
                            const int *quality, int filter, int threads, uint8_t **outs, size_t *out_lens,
                            int *status);
int ik_transform_batch_submit_opts(const uint8_t *const *bytes, const size_t *lens, uint32_t n, const int64_t *w,
                                   const int64_t *h, const void *opts, size_t opt_size, const int *fmt,
                                   const int *quality, int filter, int threads, uint8_t **outs, size_t *out_lens,
                                   int *status, uint64_t *ticket);
/* ik_transform_batch_submit_device with options: fit, background and an explicit
 * orientation 1..8 work as above.  IK_ORIENT_AUTO on any request is IK_ERR_INVALID before
 * anything is queued: the in-place JPEG marker walk steps over APP1, so the file's
 * orientation is not known on the host. */
int ik_transform_batch_submit_device_opts(const uint8_t *const *dev_bytes, const size_t *lens, uint32_t n,
                                          const int64_t *w, const int64_t *h, const void *opts,
                                          size_t opt_size, const int *fmt, const int *quality, int filter,
                                          int threads, uint8_t **outs, size_t *out_lens, int *status,
                                          uint64_t *ticket);

/* A batch of n same-geometry 8-bit images already resident in device memory
 * (image i at dev_src + i*src_image_stride, rows src_pitch bytes apart) ->
 * resize to nw x nh -> encode.  Encoded bytes are written into the caller's
 * host buffer `out` (capacity out_cap) back to back; out_sizes[i] receives each
 * size.  threads = host entropy-coder threads (0 = default).  fmt: any
 * IK_FORMAT_*; JPEG is coded on the GPU, WebP by libwebp (or the GPU VP8
 * encoder) and AVIF by libavif/aom on the host threads, from planes the GPU
 * converted (the encode_image branches, src/transform.rs:121-146). */
typedef struct ik_pipeline ik_pipeline;
int ik_pipeline_create(uint32_t W, uint32_t H, uint32_t C, uint32_t nw, uint32_t nh, int filter,
                       int fmt, int quality, uint32_t max_batch, int threads, ik_pipeline **out);
int ik_pipeline_run(ik_pipeline *p, const uint8_t *dev_src, size_t src_pitch,
                    size_t src_image_stride, uint32_t n, uint8_t *out, size_t out_cap,
                    size_t *out_sizes);
/* Streaming form of ik_pipeline_run: submit enqueues the device stage of a batch
 * (and the copy of what the host stage needs) and returns; collect finishes the
 * oldest submitted batch -- its host entropy stage -- and writes its bytes like
 * ik_pipeline_run (*n_out = its image count).  At most two batches are in flight,
 * so the host stage of batch k overlaps the device stage of batch k+1.  The
 * source frames of a submitted batch must stay valid until it is collected. */
int ik_pipeline_submit(ik_pipeline *p, const uint8_t *dev_src, size_t src_pitch,
                       size_t src_image_stride, uint32_t n);
int ik_pipeline_collect(ik_pipeline *p, uint8_t *out, size_t out_cap, size_t *out_sizes,
                        uint32_t *n_out);
/* WebP encoder of this pipeline (IK_WEBP_*; default: the process default) */
int ik_pipeline_set_webp_encoder(ik_pipeline *p, int encoder);
/* device-only part (resize + colour convert/FDCT [+ GPU VP8]) for n images, no host stage */
int ik_pipeline_run_device(ik_pipeline *p, const uint8_t *dev_src, size_t src_pitch,
                           size_t src_image_stride, uint32_t n);
/* device time (ms) of stage `which` (0 = resize, 1 = colour convert, 2 = GPU VP8
 * wavefront) in the last run, from HIP events on the pipeline's stream;
 * 3 = wall time (ms) of the last collected batch's host entropy stage */
double ik_pipeline_kernel_ms(const ik_pipeline *p, int which);
/* resized pixels of image i of the last run (tightly packed nw*nh*C) */
int ik_pipeline_fetch_resized(ik_pipeline *p, uint32_t i, uint8_t *dst, size_t cap);
void ik_pipeline_destroy(ik_pipeline *p);

/* raw device kernels, for parity tests and the bench (dev_* = device pointers) */
int ik_resize_batch_device(const uint8_t *dev_src, uint32_t W, uint32_t H, uint32_t C,
                           size_t src_pitch, size_t src_image_stride, uint32_t n, uint32_t nw,
                           uint32_t nh, int filter, uint8_t *dev_dst, size_t dst_pitch,
                           size_t dst_image_stride, void *hip_stream);
/* ik_resize_batch_device over a window: image i's columns [x0, x0 + nw) and rows
 * [y0, y0 + nh) of its resize to iw x ih, written as nw x nh pixels at dev_dst +
 * i*dst_image_stride.  Nothing outside those nw*C bytes of nh rows is written, and no
 * source byte is read past the image's last row. */
int ik_resize_window_batch_device(const uint8_t *dev_src, uint32_t W, uint32_t H, uint32_t C, size_t src_pitch,
                                  size_t src_image_stride, uint32_t n, uint32_t iw, uint32_t ih, uint32_t x0,
                                  uint32_t y0, uint32_t nw, uint32_t nh, int filter, uint8_t *dev_dst,
                                  size_t dst_pitch, size_t dst_image_stride, void *hip_stream);
/* apply_orientation over n images of W x H pixels of C samples of `depth` bytes (pixel
 * size C * depth: 1, 2, 3, 4, 6 or 8), image i at dev_src + i*src_image_stride, written at
 * dev_dst + i*dst_image_stride as W x H (orientation 1..4) or H x W (5..8) pixels.
 * Orientation 1 is a pitched device copy.  Nothing outside out_w*C*depth bytes of each of
 * the out_h destination rows is written, and nothing outside W*C*depth bytes of each of
 * the H source rows is read.  Bases, pitches and strides that are all multiples of 4 take
 * the dword path, any others the byte path.  Enqueued on hip_stream (NULL: the calling
 * thread's stream) without waiting.  IK_ERR_INVALID, with nothing launched: orientation
 * outside 1..8, a null pointer, a zero size, C outside 1..4, depth outside 1..2, a pitch
 * below the row bytes, n > 1 with an image stride below rows * pitch, n above 65535, or
 * (5..8) H above 65535 * 64. */
int ik_orient_batch_device(const uint8_t *dev_src, uint32_t W, uint32_t H, uint32_t C, uint32_t depth,
                           size_t src_pitch, size_t src_image_stride, uint32_t n, int orientation,
                           uint8_t *dev_dst, size_t dst_pitch, size_t dst_image_stride, void *hip_stream);
/* the background flatten (above) over n images of W x H pixels of C samples of `depth`
 * bytes, C 4 (Rgba) or 2 (LumaA), image i at dev_src + i*src_image_stride, written at
 * dev_dst + i*dst_image_stride as W x H pixels of out_channels samples: 3 for C = 4; for
 * C = 2, 1 (only when rgb has R == G == B) or 3.  rgb is 0xRRGGBB.  Nothing outside
 * W*out_channels*depth bytes of each of the H destination rows is written, and nothing
 * outside W*C*depth bytes of each of the H source rows is read.  Bases, pitches and strides
 * that are all multiples of 4 take the wide path (16-byte loads, whole-dword stores), for
 * source and destination independently; any others the byte path.  Enqueued on hip_stream
 * (NULL: the calling thread's stream) without waiting.  IK_ERR_INVALID, with nothing
 * launched: C outside {2, 4}, out_channels not allowed for that C and rgb, rgb outside
 * 0x000000..0xFFFFFF, depth outside 1..2, a null pointer, a zero size, a pitch below the row
 * bytes, n > 1 with an image stride below rows * pitch, or n above 65535. */
int ik_flatten_batch_device(const uint8_t *dev_src, uint32_t W, uint32_t H, uint32_t C, uint32_t depth,
                            size_t src_pitch, size_t src_image_stride, uint32_t n, int32_t rgb,
                            uint32_t out_channels, uint8_t *dev_dst, size_t dst_pitch, size_t dst_image_stride,
                            void *hip_stream);
/* blur (sharpen 0) or unsharpen (sharpen 1) over n images of W x H pixels of C = 1..4
 * samples of `depth` bytes, image i at dev_src + i*src_image_stride, written with the same
 * geometry at dev_dst + i*dst_image_stride, in one launch.  Nothing outside W*C*depth bytes
 * of each of the H destination rows is written, and nothing outside W*C*depth bytes of each
 * of the H source rows is read.  Bases, pitches and strides that are all multiples of 4
 * take the wide path (dword loads and stores), for source and destination independently;
 * any others the byte path.  Enqueued on hip_stream (NULL: the calling thread's stream)
 * without waiting; the weight tables of (W, sigma) and (H, sigma) are uploaded once per
 * device and kept.  IK_ERR_INVALID, with nothing launched and nothing written: sigma
 * outside [0.0625, IK_BLUR_MAX_SIGMA] (0 included), sharpen outside 0..1, threshold outside
 * 0..65535, C outside 1..4, depth outside 1..2, a null pointer, a zero size, a pitch below
 * the row bytes, n > 1 with an image stride below rows * pitch, n above 65535, W above 2^24
 * or H above 1048560, or source and destination bytes that overlap. */
int ik_blur_batch_device(const uint8_t *dev_src, uint32_t W, uint32_t H, uint32_t C, uint32_t depth,
                         size_t src_pitch, size_t src_image_stride, uint32_t n, float sigma, int sharpen,
                         int32_t threshold, uint8_t *dev_dst, size_t dst_pitch, size_t dst_image_stride,
                         void *hip_stream);
/* the watermark overlay (above) composited IN PLACE over n base images of W x H pixels of C
 * samples of `depth` bytes, image i at dev_base + i*image_stride, in one launch: one
 * overlay of wo x ho pixels of overlay_channels samples of overlay_depth bytes, one
 * placement and one opacity (1..255) for all of them.  The work is proportional to the
 * window, not to the image.  Nothing outside the window is written, nothing outside
 * W*C*depth bytes of a base row is read, and the overlay is only read.  A base, pitch and
 * stride that are all multiples of 4 take the wide path (whole dwords for the shares of a
 * row that lie inside the window, bytes for its ragged ends); any others the byte path.
 * Enqueued on hip_stream (NULL: the calling thread's stream) without waiting.  An empty
 * window is IK_OK: nothing is launched and the counters do not move.  IK_ERR_INVALID, with
 * nothing launched and nothing written: an unknown gravity, an opacity outside 1..255, a
 * tile outside 0..1, offsets beyond +-2^24, channels outside 1..4, a depth outside 1..2, a
 * null pointer, a zero size, a size above 2^24, a pitch below the row bytes, n > 1 with an
 * image stride below rows * pitch, n above 65535, or base and overlay bytes that overlap. */
int ik_overlay_batch_device(uint8_t *dev_base, uint32_t W, uint32_t H, uint32_t C, uint32_t depth, size_t pitch,
                            size_t image_stride, uint32_t n, const uint8_t *dev_overlay, uint32_t wo, uint32_t ho,
                            uint32_t overlay_channels, uint32_t overlay_depth, size_t overlay_pitch, int gravity,
                            int32_t dx, int32_t dy, int opacity, int tile, void *hip_stream);
/* the colour adjustment (above) applied IN PLACE over n images of W x H pixels of C samples
 * of `depth` bytes, image i at dev + i*image_stride, in one launch.  Nothing outside
 * W*C*depth bytes of each of the H rows is read or written, and alpha bytes keep their
 * values.  A base, pitch and stride that are all multiples of 4 take the wide path (whole
 * dwords; a row's ragged last share moves bytes); any others the byte path.  Enqueued on
 * hip_stream (NULL: the calling thread's stream) without waiting; the tone table of (the 24
 * bytes, depth) is uploaded once per device and kept.  A plan with flags 0 is IK_OK: nothing
 * is launched and the counters do not move.  IK_ERR_INVALID, with nothing launched and
 * nothing written: a field of adj out of range, C outside 1..4, depth outside 1..2, a null
 * pointer, a zero size, a size above 2^24, a pitch below the row bytes, n > 1 with an image
 * stride below rows * pitch, or n above 65535. */
int ik_adjust_batch_device(uint8_t *dev, uint32_t W, uint32_t H, uint32_t C, uint32_t depth, size_t pitch,
                           size_t image_stride, uint32_t n, const ik_adjust *adj, void *hip_stream);
/* the pad (above) of n images of W x H pixels of C samples of `depth` bytes, image i at
 * dev_src + i*src_image_stride, onto canvases of canvas_w x canvas_h pixels at dev_dst +
 * i*dst_image_stride, in one launch; the image lies where ik_pad_place(W, H, canvas_w,
 * canvas_h, pad->gravity) puts it; pad->width and pad->height must be in range like every
 * field of pad, but it is canvas_w and canvas_h that set the canvas.  Every byte
 * of the canvas rows is written, nothing past canvas_w*C*depth bytes of a row is, and no
 * source byte past W*C*depth of a row reaches an output.  The source may lie at any
 * address; dev_dst, dst_pitch and dst_image_stride must be multiples of 4.  Enqueued on
 * hip_stream (NULL: the calling thread's stream) without waiting.  IK_ERR_INVALID, with
 * nothing launched and nothing written: a field of pad out of range or IK_PAD_NONE, C
 * outside 1..4, depth outside 1..2, a null pointer, a zero size, a size above 2^24, a canvas
 * smaller than the image, a pitch below the row bytes, n > 1 with an image stride below
 * rows * pitch, n above 65535, or areas that overlap. */
int ik_pad_batch_device(const uint8_t *dev_src, uint32_t W, uint32_t H, uint32_t C, uint32_t depth,
                        size_t src_pitch, size_t src_image_stride, uint32_t n, const ik_pad *pad,
                        uint32_t canvas_w, uint32_t canvas_h, uint8_t *dev_dst, size_t dst_pitch,
                        size_t dst_image_stride, void *hip_stream);
/* the WebP colour conversion (to_rgb8 + libwebp RGB->YUV420) on the device;
 * dev_yuv receives the Y (w*h), U and V ((w+1)/2 * (h+1)/2) planes back to back */
int ik_webp_yuv420_device(const uint8_t *dev_src, uint32_t w, uint32_t h, uint32_t C,
                          size_t pitch, uint8_t *dev_yuv, void *hip_stream);
/* the AVIF colour conversion (to_rgba8 + ravif's 8-bit BT.601 full-range YCbCr 4:4:4)
 * on the device, for n images of w x h pixels with C channels: image i is read at
 * dev_src + i*img_stride (rows pitch apart) and written at dev_planes +
 * i*plane_img_stride as four planes of w*h bytes each, back to back: Y, U, V, A
 * (A = 255 where the source has no alpha).  dev_transparent receives n ints: the call
 * zeroes them, and flag i is 1 when any alpha of image i is below 255 (the AVIF file
 * then carries an alpha plane).  Nothing past 4*w*h bytes of an image's planes is
 * written.  Enqueued on hip_stream (NULL: the calling thread's stream) without waiting.
 * IK_ERR_INVALID, with nothing written: a null pointer, a zero size, C outside 1..4,
 * n == 0, h or n above 65535, pitch < w*C, or, when n > 1, img_stride < h*pitch or
 * plane_img_stride < 4*w*h. */
int ik_avif_yuv444_device(const uint8_t *dev_src, uint32_t w, uint32_t h, uint32_t C, size_t pitch,
                          size_t img_stride, uint32_t n, uint8_t *dev_planes, size_t plane_img_stride,
                          int *dev_transparent, void *hip_stream);
/* libwebp's method-4 segment analysis on the GPU -- the first stage of
 * encode_image's WebP coder (src/transform.rs:129-137 -> libwebp VP8EncAnalyze +
 * VP8SetSegmentParams), exact: the same segment map and segment header libwebp
 * writes for these planes at this quality.  n images of w x h YUV420 planes in
 * device memory (the ik_webp_yuv420_device layout), image i at dev_yuv +
 * i*yuv_stride.  seg (host) receives n * mb_w * mb_h segment ids, raster order per
 * image; hdr (host) n headers.  Runs on the calling thread's stream and waits. */
typedef struct {
    int32_t num_segments;  /* after libwebp's SimplifySegments (1..4) */
    int32_t update_map;    /* the frame codes a segment map */
    int32_t quant[4];      /* segment quantiser indices (the header's absolute values) */
    int32_t fstrength[4];  /* initial filter levels (libwebp raises them after coding) */
    int32_t base_quant;    /* y_ac_qi */
    int32_t dq_uv_dc, dq_uv_ac;
    int32_t probs[3];      /* segment-tree probabilities */
    int32_t alpha, uv_alpha; /* frame susceptibilities (enc->alpha_, enc->uv_alpha_) */
} ik_vp8_segment_header;
int ik_vp8_analyze_device(const uint8_t *dev_yuv, size_t yuv_stride, uint32_t n, uint32_t w, uint32_t h,
                          float quality, uint8_t *seg, ik_vp8_segment_header *hdr);
/* the exact WebP coder on the GPU: libwebp method 4's segment analysis and macroblock
 * decisions on the device (a wavefront per probability-refresh epoch), the bitstream on
 * the host -- the file WebPEncodeRGB writes for these planes at this quality.  n images
 * of w x h device YUV420 planes (the ik_webp_yuv420_device layout) yuv_stride apart;
 * outs[i] / out_lens[i] receive each file (library-allocated, ik_buf_free).  All or
 * nothing: on a failure no file is left to free and outs / out_lens are not written. */
int ik_webp_encode_exact_device(const uint8_t *dev_yuv, size_t yuv_stride, uint32_t n, uint32_t w, uint32_t h,
                                int quality, uint8_t **outs, size_t *out_lens);
/* the exact WebP coder over images of mixed sizes and qualities, in one set of launches:
 * item i is w x h device YUV420 planes (the ik_webp_yuv420_device layout) at dev_yuv,
 * anywhere in device memory, coded at its own quality (clamped to [1,100]).  Every file is
 * the one ik_webp_encode_exact_device writes for that image alone.  w, h <= 16383 and
 * n <= 65535; a bad item (a zero or oversized side, a null plane) is IK_ERR_INVALID
 * before anything is launched, with outs untouched.  Items that all share one geometry
 * and quality go through the uniform call (one geometry never takes two code paths).
 * outs[i] / out_lens[i] as above, all or nothing: on a failure no file is left to free
 * and outs / out_lens are not written. */
typedef struct {
    const uint8_t *dev_yuv;
    uint32_t w, h;
    int quality;
} ik_webp_exact_item;
int ik_webp_encode_exact_items(const ik_webp_exact_item *items, uint32_t n, uint8_t **outs, size_t *out_lens);
/* the ticket table of that call for n images of w[i] x h[i] pixels (no GPU needed), in
 * the kernel's format: bit 63 = an epoch's statistics fold, bits 48..55 the image's
 * epoch, bits 32..47 the image, bits 0..31 the macroblock (raster index in its image).
 * Each image keeps the single-image order (epochs at libwebp's probability refreshes,
 * macroblocks by diagonal mb_x + 2 mb_y, then the epoch's fold); the images are merged
 * step by step (a step = one diagonal or one fold of an image).  Returns the ticket
 * count and writes the first min(count, cap) tickets to tasks (may be NULL when cap is
 * 0) and the launch's workgroup count to *grid (may be NULL); -1 on a bad argument. */
long long ik_webp_exact_plan(const uint32_t *w, const uint32_t *h, uint32_t n, uint64_t *tasks, size_t cap,
                             uint32_t *grid);
/* where ik_transform_batch codes the WebP requests that form no same-geometry group the
 * uniform exact call takes (encoder IK_WEBP_AUTO or IK_WEBP_EXACT):
 * IK_WEBP_MIXED_HOST (the default): as before -- libwebp on host threads under AUTO, the
 *   exact coder image by image under EXACT;
 * IK_WEBP_MIXED_GPU: when a batch holds enough of them (32, provisional), all of them
 *   through one batched colour launch and one mixed exact call (ik_webp_encode_exact_items'
 *   path); the same files either way.
 * ik_set_webp_mixed(-1) returns to the environment: IK_WEBP_MIXED=host|gpu, read per batch. */
typedef enum { IK_WEBP_MIXED_HOST = 0, IK_WEBP_MIXED_GPU = 1 } ik_webp_mixed;
int ik_set_webp_mixed(int where);
int ik_get_webp_mixed(void);
/* process-wide WebP encode counters: out[0] = images coded by the uniform exact call,
 * out[1] = images coded by the mixed exact call, out[2] = images coded by libwebp on
 * the host, out[3] = mixed exact calls made */
int ik_webp_enc_counters(unsigned long long *out);
/* the JPEG front end (to_rgb8 + RGB->YCbCr + FDCT + quantise) on the device:
 * int16 coefficients, MCU-major, Y/Cb/Cr, natural order */
int ik_jpeg_coeffs_device(const uint8_t *dev_src, uint32_t w, uint32_t h, uint32_t C,
                          size_t pitch, int quality, int16_t *dev_coef, void *hip_stream);
/* the JPEG entropy coder on its own (k_jpeg_huff_enc), for parity tests: baseline
 * Huffman coding of n images of w x h pixels whose int16 coefficients
 * ([mcu][Y,Cb,Cr][64], natural order; the ik_jpeg_coeffs_device layout) lie
 * coef_img_stride int16 units apart in device memory (16-byte aligned, the stride
 * a multiple of 8: IK_ERR_INVALID otherwise).  One launch, the buffers laid out as
 * encode_image's JPEG branch lays them out.  Image i's stuffed scan bytes (no
 * header, no EOI) land in host_out + i * ik_jpeg_enc_capacity(w, h) and their
 * count in host_len[i]; 0xffffffff there is the kernel's "does not fit" answer
 * (twice the unstuffed bytes exceed the capacity), reported as is -- no host
 * coder runs here.  host_out goes to the device before the launch, so bytes
 * the kernel does not write (it stores whole 16-byte words) come back unchanged. */
size_t ik_jpeg_enc_capacity(uint32_t w, uint32_t h);
int ik_jpeg_huffman_device(const int16_t *dev_coef, size_t coef_img_stride, uint32_t n, uint32_t w,
                           uint32_t h, uint8_t *host_out, uint32_t *host_len);
/* process-wide JPEG encode counters: out[0] = images whose scan bytes
 * k_jpeg_huff_enc wrote, out[1] = images the host coder wrote because their
 * stream did not fit the GPU coder's buffer (ik_encode, ik_transform[_batch],
 * ik_pipeline_*) */
int ik_jpeg_enc_counters(unsigned long long *out);

/* device memory helpers (so callers need no HIP headers) */
int ik_dev_alloc(size_t bytes, void **dev_ptr);
int ik_dev_free(void *dev_ptr);
int ik_memcpy_h2d(void *dev_dst, const void *host_src, size_t bytes);
int ik_memcpy_d2h(void *host_dst, const void *dev_src, size_t bytes);
int ik_dev_synchronize(void);

#ifdef __cplusplus
}
#endif
#endif
