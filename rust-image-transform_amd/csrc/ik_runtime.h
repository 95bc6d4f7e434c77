// ik_runtime.h -- host runtime internals of libimagekit_hip.so (not part of the ABI).
#pragma once
#include <array>
#include <condition_variable>
#include <cstdarg>
#include <cstring>
#include <cstdint>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <tuple>
#include <vector>
#include <unordered_map>

#include "ik_internal.h"
#include "ik_post_plan.h"

struct ik_image {
    uint32_t w = 0, h = 0, c = 0;  // c interleaved channels
    uint32_t depth = 1;            // bytes per sample: 1 (8-bit) or 2 (16-bit, native-endian u16)
    size_t pitch = 0;              // bytes between rows on the device (multiple of 256)
    uint8_t* d = nullptr;          // device pixels
    bool owned = true;
    int device = 0;
    size_t block = 0;              // bytes of the pooled allocation behind d (owned images)
};

namespace ik {

// thread-local error message + status (ik_last_error)
int fail(int status, const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);
#define IK_HIP(call)                                    \
    do {                                                \
        hipError_t _e = (call);                         \
        if (_e != hipSuccess) return hip_fail(_e, #call); \
    } while (0)

int current_device();
// make `device` the calling thread's device for the guard's lifetime (an image's
// stages run on the device that holds its pixels)
struct DeviceGuard {
    int prev;
    explicit DeviceGuard(int device);
    ~DeviceGuard();
};

// ---- persistent host workers (ik_pool.cpp) ----
int default_threads();  // IK_THREADS, else min(16, cores)
class Pool {
public:
    Pool(int device, int max_threads);
    // fn(i) for i in [0, n) on up to `threads` threads (the caller included; 0 =
    // default_threads()); returns when every call has returned
    void parallel_for(int n, int threads, const std::function<void(int)>& fn);
    void post(std::function<void()> task);  // run on a worker (device already selected)
    int device() const { return device_; }
    // ik_shutdown: run what is queued, then end and join every worker (each
    // releases its streams and arenas first); the pool takes work again after
    void stop();

private:
    struct Task {
        std::function<void()> fn;
        const void* tag;  // parallel_for helpers: their ForState (withdrawn once it is done)
    };
    void post_tagged(std::function<void()> task, const void* tag);
    void withdraw(const void* tag);
    void ensure(int nthreads);
    void loop();
    int device_, max_threads_;
    int nthreads_ = 0, busy_ = 0;
    bool stop_ = false;
    std::mutex mu_;
    std::condition_variable cv_;
    std::deque<Task> q_;
    std::vector<std::thread> threads_;
};
Pool& device_pool(int device);  // the persistent workers of a physical device
// fn(i) for i in [0, n) on the calling thread's device pool (and the caller)
void parallel_for(int n, int threads, const std::function<void(int)>& fn);

// Figures of the last batch each device's kernel stages ran (ik_batch_last_timing):
// device ms from HIP events on the stage's stream and the algorithmic bytes of the
// same launches.  Two records per device, one per stage: the decode stage's fields
// (kBtJpeg* up to kBtJpegLanes) and the post stage's (resize, JPEG encoder); each is
// reset when its stage starts a batch and summed over that batch's launches.
enum BatchTimingField {
    kBtJpegHuffMs = 0,   // JPEG entropy decoding launches (restart intervals / self-sync)
    kBtJpegScanBytes,    // entropy-coded bytes they read
    kBtJpegCoefBytes,    // int16 coefficients they wrote
    kBtJpegImages,
    kBtJpegLanes,        // decoder lanes (restart intervals or self-sync subsequences)
    kBtResizeMs,         // grouped resize launches
    kBtResizeBytes,      // C*W*H in + C*w*h out per image
    kBtResizeImages,
    kBtJpegEncMs,        // batched JPEG encoder (coefficients + Huffman) launches
    kBtJpegEncImages,
    kBtHostWallMs,       // the host coder stage (libwebp / libavif): wall ms of the batch
    kBtHostCoreMs,       // its thread CPU ms summed over the requests (core-ms)
    kBtHostImages,       // requests it coded
    kBtFields
};
// the host coder stage's record of the batch it just finished (set directly: that
// stage runs on the device's worker pool after the post stage committed)
void batch_timing_host(int device, double wall_ms, double core_ms, double images);
void batch_timing_reset(int device, bool post);
void batch_timing_commit(int device, bool post);  // the stage is done: its fields become the last batch's
void batch_timing_add(int device, int field, double v);
// a pair of events on the calling thread (timing one launch sequence); ms between them
struct EvPair {
    hipEvent_t a = nullptr, b = nullptr;
};
EvPair& thread_events(int which);  // which < 4
float ev_pair_ms(const EvPair& e);
// Who owns which pair (2 and 3: the JPEG and WebP decoders').  kEvResize times
// resize_group's launch and, on a submitting caller's thread, the JPEG marker walk
// (ik_transform_batch_submit_device): each reads its pair right after the stream
// synchronisation that follows its launch, so neither finds the other's events
// pending.  kEvJpegGroup times jpeg_front_group's launches.
constexpr int kEvResize = 0, kEvJpegWalk = kEvResize, kEvJpegGroup = 1;

// A scope in which batch_timing_add records (the decode and post stages of a
// batch set it on their thread); work outside one -- a single-image ik_decode, a
// pool worker's own resize -- adds nothing to ik_batch_last_timing
struct BatchTimingScope {
    bool prev;
    BatchTimingScope();
    ~BatchTimingScope();
};
// record a timing-only event: a failure is ignored (the pair then reads 0 ms) and
// never changes the caller's path
void ev_record(hipEvent_t e, hipStream_t s);

// The library's lifetime against ik_shutdown / ik_close: every public
// entry point holds the lifetime lock shared for its call (ApiGuard; nested calls
// on one thread take it once), shutdown takes it exclusively, so teardown never
// runs under a caller that is still inside the library (e.g. a daemon thread of
// a server during interpreter exit).  Threads the library owns (pool workers,
// stage threads, pipeline workers) are marked internal and never take it:
// shutdown waits for them while it holds the lock.  After ik_close, entry points
// that take it return IK_ERR_INVALID.
struct ApiGuard {
    bool held = false, closed = false;
    ApiGuard();
    ~ApiGuard();
};
void mark_internal_thread();
#define IK_API_ENTER()                                                                        \
    ::ik::ApiGuard ik_api_guard_;                                                             \
    if (ik_api_guard_.closed) return ::ik::fail(IK_ERR_INVALID, "the library is closed (ik_close)")
#define IK_API_ENTER_VOID()          \
    ::ik::ApiGuard ik_api_guard_;    \
    if (ik_api_guard_.closed) return

// Bytes the library holds, by pool (ik_memory_stats): device image blocks in use
// and kept free for reuse, the per-thread device and pinned arenas, the PNG / JPEG
// upload areas (device, pinned), the cached resize plans' device tables
enum MemStat {
    kMemImageLive = 0, kMemImageFree, kMemArenaDev, kMemArenaPinned, kMemUploadDev, kMemUploadPinned,
    kMemPlans, kMemStats
};
void mem_stat(int which, int64_t delta);

// ik_shutdown: stop and join every pool's workers (device and logical pools);
// multi-device dispatch is unconfigured
void pools_shutdown();
// release the calling thread's streams and arenas (synchronised first); a later
// call on this thread creates them again
void release_thread_resources();
void png_shutdown();    // the PNG upload areas (ik_png_decode.cpp)
void plans_shutdown();  // the cached resize plans (ik_plan.cpp)

// multi-device dispatch (ik_init(-1) / IK_DEVICES): logical devices, least outstanding cost
int sched_configure(const int* devices, int n);
bool sched_multi();
int sched_count();
int sched_phys(int logical);
Pool& sched_pool(int logical);
int sched_acquire(uint64_t cost);
// the least-loaded logical device on physical device `phys` (-1: none)
int sched_acquire_on(int phys, uint64_t cost);
void sched_release(int logical, uint64_t cost);
void sched_acquire_batch(const uint64_t* costs, uint32_t n, uint32_t* assign);
void sched_plan(const uint64_t* costs, uint32_t n, uint32_t ndev, const uint64_t* outstanding, uint32_t* assign);
uint32_t sched_split(const uint64_t* costs, uint32_t n, uint32_t nd, uint32_t min_batch, uint64_t* outstanding,
                     uint32_t* lo, uint32_t* dev);
int sched_stats(uint32_t logical, uint64_t* jobs, uint64_t* cost_done, uint64_t* outstanding);
// header-only dimension sniff (PNG IHDR, JPEG SOFn, WebP VP8/VP8L/VP8X); c = bytes per pixel
bool sniff_dims(const uint8_t* b, size_t n, uint32_t& w, uint32_t& h, uint32_t& c);
uint64_t request_cost(const uint8_t* b, size_t n, int64_t w, int64_t h, int fmt);

hipStream_t thread_stream();  // per-thread, per-device non-blocking stream
hipStream_t thread_copy_stream();  // a second one, for uploads that overlap the first's kernels
// a third, at the highest priority, and an event to order it after the first (the
// exact WebP coder's launches; ev may be null); false if it cannot be made
bool thread_prio_stream(hipStream_t* s, hipEvent_t* ev);
// two events (no timing) of the calling thread on its current device, to fork work
// from one of its streams to another and join it back (the PNG unfilter); made on
// first use on that device; false if they cannot be made
bool thread_fork_join_events(hipEvent_t* fork, hipEvent_t* join);
size_t pitch_for(uint32_t w, uint32_t c);
uint8_t* scratch(size_t bytes);  // per-thread device scratch, valid until the next call
// per-thread, per-device grow-only device arenas for batch work (slot 1: JPEG
// batch decode, slot 2: PNG batch decode); valid until the next call with that slot
uint8_t* scratch_slot(int slot, size_t bytes);
uint8_t* pinned_slot(int slot, size_t bytes);  // per-thread grow-only pinned host arenas (slots 0..11)
// Who owns which arena.  Device slots 1, 2, 5 and pinned slots 1, 2, 3, 6 are the JPEG and
// PNG decoders' (ik_jpeg_decode.cpp, ik_png_decode.cpp).
// scratch(): the single-image calls' work area, valid until the thread's next scratch()
constexpr int kScratchDefault = 0;
// copy_h2d_2d / copy_d2h_2d's staging; each copy synchronises the stream before it returns
constexpr int kPinnedStaging = 0;
// a group launch's table of image base pointers, webp_front_group's, resize_group's,
// orient_group's and flatten_group's (which stage it in kPinnedGroupStage as resize_group
// does): all run on one thread and synchronise the stream after the launch that reads the table
constexpr int kScratchPtrTable = 3;
// jpeg_front_group's device work area: quantisation tables, source table, coefficients, Huffman work
constexpr int kScratchJpegGroup = 4;
// encode_device_front's WebP planes, written by the colour kernel; the stream is
// synchronised before the planes are copied out
constexpr int kPinnedWebpPlanes = 4;
// jpeg_front_group's streams, lengths and table staging, and resize_group's pointer-table
// staging: both run on one thread and synchronise the stream before they write the area
constexpr int kPinnedGroupStage = 5;
// ik_transform_batch_submit_device's file heads and JPEG marker-walk records (the caller's
// thread; synchronised before they are read)
constexpr int kPinnedDeviceHeads = 7;
// the exact WebP coder's arenas: its device work area; its constants in, its records out
constexpr int kScratchExact = 8, kPinnedExactIn = 8, kPinnedExactOut = 9;
// the mixed exact call's: same-geometry planes gathered a common stride apart; a batch's
// planes and colour-conversion table (device) and that table's staging (pinned)
constexpr int kScratchExactGather = 10, kScratchMixedPlanes = 11, kPinnedMixedTab = 11;
// the WebP (VP8) decoder's: its device work area and its staged file + headers
constexpr int kScratchVp8d = 9, kPinnedVp8d = 10;
int copy_h2d_2d(uint8_t* dst, size_t dpitch, const uint8_t* src, size_t spitch, size_t width,
                size_t height, hipStream_t s);
int copy_d2h_2d(uint8_t* dst, size_t dpitch, const uint8_t* src, size_t spitch, size_t width,
                size_t height, hipStream_t s);
int alloc_image(uint32_t w, uint32_t h, uint32_t c, ik_image** out, uint32_t depth = 1);

// per-device constant tables (WebP gamma tables)
struct DeviceConsts {
    uint16_t* gamma_to_lin = nullptr;  // [256]
    int* lin_to_gamma = nullptr;       // [33]
    uint32_t* jpeg_huff = nullptr;     // [4][256] standard Huffman tables (k_jpeg_huff_enc)
};
const DeviceConsts* device_consts(int device);
void webp_gamma_tables(uint16_t g2l[256], int l2g[33]);

// host entropy stages (ik_codec.cpp)
int webp_encode_yuv420(const uint8_t* y, const uint8_t* u, const uint8_t* v, int w, int h,
                       float quality, std::vector<uint8_t>& out);
void jpeg_quant_tables(int quality, uint8_t qt[128]);
int avif_encode_yuv444(const uint8_t* planes /* Y, U, V, A */, bool has_alpha, int w, int h, int quality,
                       int speed, std::vector<uint8_t>& out);
void jpeg_write(const int16_t* coef, int w, int h, const uint8_t qt[128], std::vector<uint8_t>& out);
void jpeg_header(int w, int h, const uint8_t qt[128], std::vector<uint8_t>& out);  // SOI .. SOS
void jpeg_huff_u32(uint32_t t[4 * 256]);  // ldc, lac, cdc, cac: code << 8 | size
// which coder wrote an encoded JPEG's scan bytes (ik_jpeg_enc_counters): k_jpeg_huff_enc
// or, for a stream past its buffer, the host coder jpeg_write
void jpeg_enc_count(bool gpu_coded);

// the WebP coder encode_image uses unless ik_set_webp_encoder / IK_WEBP_ENCODER says
// otherwise (ik_webp_gpu.cpp)
constexpr int kDefaultWebpEncoder = IK_WEBP_AUTO;
int default_webp_encoder();
// IK_WEBP_AUTO's and IK_WEBP_MIXED_GPU's thresholds (kAutoExactMinGroup, kAutoMixedMin)
// and the rule that applies them (webp_takes_exact): ik_post_plan.h
// encode_image's quality range, and the bytes of a w x h image's YUV420 planes
inline int clamp_quality(int q) { return q < 1 ? 1 : (q > 100 ? 100 : q); }
inline size_t yuv420_bytes(size_t w, size_t h) { return w * h + 2 * ((w + 1) / 2) * ((h + 1) / 2); }
// the exact coder (ik_vp8x_host.cpp): libwebp's files from n device YUV420 images
int webp_encode_exact(const uint8_t* d_yuv, size_t yuv_stride, int n, int w, int h, int quality,
                      std::vector<std::vector<uint8_t>>& outs);
// the same over images of mixed sizes and qualities (device planes anywhere), in one set
// of launches; items that share one geometry and quality go through webp_encode_exact
struct ExactItem {
    const uint8_t* yuv;
    int w, h, quality;
};
int webp_encode_exact_mixed(const ExactItem* items, int n, std::vector<std::vector<uint8_t>>& outs);
// where a batch's WebP requests outside the uniform groups are coded (ik_set_webp_mixed /
// IK_WEBP_MIXED, read per batch): IK_WEBP_MIXED_HOST or IK_WEBP_MIXED_GPU
int webp_mixed_mode();
// ik_webp_enc_counters: 0 = images by the uniform exact call, 1 = by the mixed exact
// call, 2 = by libwebp on the host, 3 = mixed calls
void webp_enc_count(int which, unsigned long long n);
// its first stages alone (ik_vp8_analyze_device): segment analysis and set-up on the
// device, the segment map and headers into host memory
int vp8_analyze_setup(const uint8_t* d_yuv, size_t yuv_stride, int n, int w, int h, float quality, uint8_t* seg,
                      ik_vp8_segment_header* hdr);

// host decoders (ik_decode.cpp): tightly packed 8-bit pixels
enum class Sniffed { Png, Jpeg, Gif, WebP, Tiff, Bmp, Ico, Hdr, Avif, OpenExr, Qoi, Farbfeld, Pnm, Dds, Unknown };
Sniffed guess_format(const uint8_t* b, size_t n);
const char* format_name(Sniffed f);
// depth (optional): 16-bit streams decode to native-endian u16 samples (*depth = 2);
// without it they are unsupported.  zlib_only: inflate with zlib, not libdeflate (a stream
// the GPU path found corrupt: libdeflate accepts code lengths whose last repeat overruns
// HLIT + HDIST, zlib and the GPU path do not)
int decode_png(const uint8_t* b, size_t n, uint32_t& w, uint32_t& h, uint32_t& c, std::vector<uint8_t>& px,
               uint32_t* depth = nullptr, bool zlib_only = false);
uint32_t png_chunk_crc(const uint8_t* type, const uint8_t* data, size_t len);  // CRC-32 of type + data
// PNG on the GPU (ik_png_decode.cpp + ik_png.hip): inflate + unfilter of n streams
// in one set of launches, straight into new device images; streams the GPU path
// does not cover (or that fail on it) go through decode_png.  Per-stream status
// and message; returns the first failure.
int decode_png_batch(const uint8_t* const* b, const size_t* lens, int n, ik_image** outs, int* status,
                     std::string* msgs);
// decode_png_batch as two stages, so that one batch's upload (PCIe + the GPU
// gather / CRC pass, on the calling thread's copy stream) runs under the previous
// batch's kernels: png_upload_begin parses the streams and issues the upload
// (returns once issued); png_decode_finish, on the kernel stage's thread, runs the
// decode kernels once the upload has landed.  The input arrays stay valid until
// finish returns; every begin is finished exactly once.
struct PngBatchState;
struct PngUpload {
    const uint8_t* const* bytes = nullptr;
    const size_t* lens = nullptr;
    int n = 0;
    std::shared_ptr<PngBatchState> st;
    // dev: bytes[i] are device addresses on the calling thread's device (the
    // caller's files already in HBM), heads[i] a host copy of each file's first 8
    // bytes; the upload then walks the chunks on the GPU and gathers from there
    bool dev = false;
    const uint8_t* const* heads = nullptr;
    // called by png_decode_finish once the batch's decode rounds are done (argument:
    // an event to wait for first, or null): the stage executor launches the next
    // batch's block search there, on the kernel stream before this batch's expand
    // (beside the unfilter instead it doubled the unfilter: profiles/r04k_*)
    std::function<void(hipEvent_t)> on_next_search;
};
int png_upload_begin(const uint8_t* const* b, const size_t* lens, int n, PngUpload& up);
int png_decode_finish(PngUpload& up, ik_image** outs, int* status, std::string* msgs);
// the block search of an issued upload, on stream s (after the upload lands);
// png_decode_finish then only waits for it.  Kernel-stage thread only.
void png_find_prelaunch(PngUpload& up, hipStream_t s);
bool png_find_beside_decode();  // IK_FIND_BESIDE: the next batch's block search beside the decode (experiment)
bool png_upload_landed(const PngUpload& up);  // its upload + gather pass have completed (nothing to wait for)
constexpr int kPngTimingFields = 17;  // ik_png_last_timing
// caller-pinned host memory (ik_host_alloc / ik_host_register): [p, p + n) lies
// inside one such range, so DMAs may read it in place
bool host_pinned(const void* p, size_t n);
bool png_gpu_enabled(size_t raw_bytes);  // IK_PNG_GPU / IK_PNG_GPU_MIN policy
int decode_webp(const uint8_t* b, size_t n, uint32_t& w, uint32_t& h, uint32_t& c, std::vector<uint8_t>& px);
// libwebp's WebPDecodeRGBA of a w x h lossless file, its green channel alone into plane
// (w * h bytes): how the GPU path reads a lossless-coded alpha plane (ik_vp8d_host.cpp).
// false: the decode failed or gave another size.
bool webp_lossless_green(const uint8_t* b, size_t n, uint32_t w, uint32_t h, uint8_t* plane);
// WebP lossy ("VP8 ", no animation; with an alpha plane only under
// IK_WEBP_ALPHA_DECODE=gpu) on the GPU (ik_vp8d_host.cpp + ik_vp8d.hip):
// the host parses the headers and partition 0 and decodes the tokens, the device
// reconstructs, loop-filters and converts to RGB straight into a new device image.
// Returns kVp8dHost (nothing recorded) for files it leaves to decode_webp: other
// WebP kinds, anything its parser finds unusual, data that runs out.
constexpr int kVp8dHost = -1000;
int decode_webp_device(const uint8_t* b, size_t n, ik_image** out);
void webp_count_host_decode();  // a WebP stream handed to decode_webp outside decode_webp_batch (ik_webp_counters)
// decode_image over a batch's n WebP files: the lossy ones the GPU path takes are
// parsed in parallel (partition 0 and the tokens, on up to `threads` threads) and
// reconstructed together -- one staged area, one H2D, one k_vp8d_recon, one
// k_vp8d_alpha where a taken file's alpha plane is filtered and one k_vp8d_rgb launch
// over all of them (sub-launches past IK_VP8D_BATCH_BYTES, default 256 MiB); the rest
// (alpha unless IK_WEBP_ALPHA_DECODE=gpu, lossless, animation, anything handed back, a frame whose
// err word the device set) go to libwebp on the worker that found them.  IK_WEBP_DECODE
// is read per batch: host = libwebp only; gpu = every lossy file takes the batch path
// and a file left to libwebp is an error; auto = the batch path when its lossy files
// total kWebpGpuMinBatchPixels pixels.  outs / status / msgs per file as decode_image
// gives them; returns the first failure.
int decode_webp_batch(const uint8_t* const* b, const size_t* lens, int n, ik_image** outs, int* status,
                      std::string* msgs, int threads);
// IK_WEBP_DECODE (read per call): 0 "host" (libwebp only), 2 "gpu" (every size; a file
// the GPU path leaves to the host is an error instead: the tests' proof that it ran),
// 1 otherwise (auto: the GPU path from 3 MPix, where it is faster than libwebp)
int webp_decode_mode();

// JPEG: host entropy decode + GPU reconstruction straight into a new device image
// (ik_jpeg_decode.cpp + ik_jpeg.hip)
int decode_jpeg_device(const uint8_t* b, size_t n, ik_image** out);
// A batch's JPEG files DMAed to the device by the upload stage (ik_host.cpp
// StageExec), so that the kernel stage's self-synchronising decoder reads their
// scans where they lie instead of copying them in its own time.  The files of the
// batch in one device area (two per device, as the PNG upload areas), DMAed in
// place when the caller pinned them, else through pinned staging; `ev` marks the
// DMAs' end on the upload thread's stream.  Dropping the JpegUpload (after the
// batch's decode returned) frees the area for the next batch.
struct JpegArea;
// A JPEG file of a device-resident batch that is decoded where it lies
// (ik_transform_batch_submit_device; the marker walk, ik_jpeg_walk.h): what came
// back to the host of it.  The file itself stays in the caller's device memory.
struct JpegInPlace {
    const uint8_t* skel = nullptr;  // its skeleton: SOI and the segments the parser reads, host memory
    uint32_t skel_len = 0;
    size_t len = 0;                 // the file's length
    uint64_t ent_off = 0, eoi_off = 0;  // the first scan's bytes: [ent_off, eoi_off) of the file
};
typedef std::unordered_map<const uint8_t*, JpegInPlace> JpegInPlaceMap;  // by the file's device address
struct JpegUpload {
    int n = 0;
    std::unordered_map<const uint8_t*, const uint8_t*> dev;  // host file -> its device copy
    hipEvent_t ev = nullptr;
    std::shared_ptr<JpegArea> area;
    const JpegInPlaceMap* inplace = nullptr;  // device-resident batches: the files taken in place
};
// ik_jpeg_device_counters: 0 taken in place, 1 copied back before parsing, 2 copied back later
void jpeg_device_count(int which, unsigned long long n);
// IK_JPEG_DEVICE / ik_set_jpeg_device: baseline JPEG bodies in device memory are decoded in place
bool jpeg_device_inplace();
// IK_JPEG_PROG_FREE / ik_set_jpeg_prog_free: progressive files without restart markers are
// entropy-decoded on the GPU (off by default: the host decoder takes them; IK_JPEG_PROG=0
// keeps every progressive scan on the host whatever this says)
bool jpeg_prog_free_gpu();
void jpeg_device_walk_ms(float ms);  // the last k_jpeg_walk launch's device time (ik_jpeg_device_walk_ms)
int jpeg_upload_begin(const uint8_t* const* b, const size_t* lens, int n, JpegUpload& up);
void jpeg_shutdown();  // ik_shutdown: the JPEG upload areas
// n streams at once: baseline scans entropy-decoded together by the self-
// synchronising GPU decoder; per-stream status (outs[i] null on failure); returns
// the first failure.  up: the files' device copies (jpeg_upload_begin), or null
int decode_jpeg_batch(const uint8_t* const* b, const size_t* lens, int n, ik_image** outs, int* status,
                      std::string* msgs /* [n] or null: per-stream error message */,
                      const JpegUpload* up = nullptr);

// device-side stage helpers used by ik_encode and the pipeline
int encode_device_image(const uint8_t* dev, uint32_t w, uint32_t h, uint32_t c, size_t pitch,
                        int fmt, int quality, std::vector<uint8_t>& out);
// encode_image in two halves: the device front end (colour conversion, FDCT and
// Huffman coding for JPEG) leaves either the final bytes (done) or the planes the
// host coder takes (WebP YUV420, AVIF YUV444 + alpha); the back end runs that
// host coder (libwebp / libavif) and touches no device
struct EncodePrep {
    int fmt = -1, q = 0;
    uint32_t w = 0, h = 0;
    bool done = false, transparent = false;
    std::vector<uint8_t> planes;
    // or the planes in a shared page-locked block written by a batched colour
    // launch (webp_front_group): no copy into `planes`; the block returns to its
    // pool when the last request holding it is coded
    std::shared_ptr<uint8_t> pin_block;
    const uint8_t* pin_planes = nullptr;
    const uint8_t* plane_data() const { return pin_planes ? pin_planes : planes.data(); }
};
int encode_device_front(const uint8_t* dev, uint32_t w, uint32_t h, uint32_t c, size_t pitch, int fmt, int quality,
                        EncodePrep& p, std::vector<uint8_t>& out);
int encode_image_front(const ik_image* img, int fmt, int quality, EncodePrep& p, std::vector<uint8_t>& out);
int encode_host_back(EncodePrep& p, std::vector<uint8_t>& out);
// A finished JPEG file in out: hdr (SOI .. SOS), len entropy-coded bytes, EOI.  The
// bytes are copied from `stream`, or, when it is null, left for the caller to fill
// (a copy from device memory); returns where they lie in out
uint8_t* jpeg_file(const std::vector<uint8_t>& hdr, const uint8_t* stream, uint32_t len, std::vector<uint8_t>& out);
// The post stage's group calls (ik_encode.cpp), each over n same-geometry 8-bit images
// on one device; a return other than IK_OK leaves every image to the per-image path.
// webp_exact_group: the exact coder's files (outs[i]) for one quality.
// webp_exact_mixed_group: the same over images of any sizes and qualities.
// webp_front_group: the YUV420 planes libwebp codes, in pinned memory (prep[i]).
// jpeg_front_group: the finished JPEG files (out[i]).
int webp_exact_group(const std::vector<ik_image*>& imgs, int quality, std::vector<std::vector<uint8_t>*>& outs);
int webp_exact_mixed_group(const std::vector<ik_image*>& imgs, const std::vector<int>& quality,
                           std::vector<std::vector<uint8_t>*>& outs);
int webp_front_group(const std::vector<ik_image*>& imgs, int quality, std::vector<EncodePrep*>& prep);
int jpeg_front_group(const std::vector<ik_image*>& imgs, int quality, std::vector<std::vector<uint8_t>*>& out);
void encode_shutdown();  // ik_shutdown: their pinned blocks, the per-device constant tables

// resize_image's output size (src/transform.rs:62-90 + DynamicImage::resize; its
// arithmetic: ik_post_plan.h) and a one-launch resize of same-geometry 8-bit images
// (ik_encode.cpp)
int resize_target(uint32_t W, uint32_t H, int64_t w, int64_t h, uint32_t* nw, uint32_t* nh);
int resize_group(const std::vector<ik_image*>& src, const FitWindow& win, int filter, std::vector<ik_image*>& out);
// apply_orientation (2..8) of same-geometry images in one launch (ik_encode.cpp); a return
// other than IK_OK leaves every image to ik_image_orient
int orient_group(const std::vector<ik_image*>& src, int orientation, std::vector<ik_image*>& out);
// the background flatten of same-geometry images with alpha onto one colour in one launch
// (ik_encode.cpp); a return other than IK_OK leaves every image to ik_image_flatten
int flatten_group(const std::vector<ik_image*>& src, uint32_t rgb, std::vector<ik_image*>& out);
// process-wide flatten launches and images flattened (ik_flatten_counters)
void flatten_count(uint64_t launches, uint64_t images);
// one request's blur or unsharpen, after its resize (ik_request_opts2)
struct FilterReq {
    int mode = 0;  // 0: none, 1: blur, 2: unsharpen
    float sigma = 0.0f;
    int32_t threshold = 0;
};
// blur or unsharpen of same-geometry images in one launch (ik_blur_host.cpp); a return other
// than IK_OK leaves every image to ik_image_blur / ik_image_unsharpen
int blur_group(const std::vector<ik_image*>& src, float sigma, bool sharpen, int32_t threshold,
               std::vector<ik_image*>& out);
bool blur_threshold_ok(int32_t t);  // 0..65535
void blur_shutdown();               // ik_shutdown: the cached axis tables (ik_blur_host.cpp)
// one request's watermark, after its blur or unsharpen (ik_request_opts3); the handle is the
// caller's and outlives the call
struct OverlayReq {
    const ik_image* mark = nullptr;  // null: none
    int32_t gravity = 0, dx = 0, dy = 0;
    int32_t opacity = 255;  // 1..255
    int32_t tile = 0;
    // requests whose keys are equal share a launch (overlay_group)
    typedef std::tuple<uintptr_t, int32_t, int32_t, int32_t, int32_t, int32_t> Key;
    Key key() const { return Key((uintptr_t)mark, gravity, dx, dy, opacity, tile); }
};
// IK_OK, or IK_ERR_INVALID with the message set (prefix: "" or "request i: "): the gravity,
// the offsets, the tile flag and an opacity within opacity_lo..255 (ik_overlay_host.cpp)
int overlay_check(int32_t gravity, int32_t dx, int32_t dy, int32_t opacity, int32_t opacity_lo, int32_t tile,
                  const char* prefix);
// the watermark composited in place: onto one image in a launch of its own, or onto
// same-geometry images in one launch; a return other than IK_OK from overlay_group leaves
// every image to overlay_image.  An overlay on another device is copied over for the call.
int overlay_image(ik_image* base, const OverlayReq& r);
int overlay_group(const std::vector<ik_image*>& bases, const OverlayReq& r);
// one request's colour adjustment, after its resize (ik_request_opts4); all zero: none
struct AdjustReq {
    ik_adjust a{};
    bool on() const {
        return a.brightness || a.contrast || a.saturation || a.hue || a.gamma != 0.0f || a.invert;
    }
    // requests whose keys (the 24 bytes) are equal share a launch (adjust_group)
    typedef std::array<uint8_t, sizeof(ik_adjust)> Key;
    Key key() const {
        Key k;
        std::memcpy(k.data(), &a, sizeof a);
        return k;
    }
};
// IK_OK, or IK_ERR_INVALID with the message set (prefix: "" or "request i: "): every field of
// the adjustment within its range (ik_adjust_host.cpp)
int adjust_check(const ik_adjust& a, const char* prefix);
// the adjustment applied in place: to one image in a launch of its own, or to same-geometry
// images in one launch; a return other than IK_OK from adjust_group leaves every image to
// adjust_image.  Both synchronise the stream.
int adjust_image(ik_image* img, const AdjustReq& r);
int adjust_group(const std::vector<ik_image*>& imgs, const AdjustReq& r);
void adjust_shutdown();  // ik_shutdown: the cached plans and their device tables
// one request's pad, after its blur or unsharpen (ik_request_opts5); mode IK_PAD_NONE: none
struct PadReq {
    ik_pad p{};
    bool on() const { return p.mode != IK_PAD_NONE; }
    // requests whose keys (the 24 bytes) are equal share a launch (pad_group)
    typedef std::array<uint8_t, sizeof(ik_pad)> Key;
    Key key() const {
        Key k;
        std::memcpy(k.data(), &p, sizeof p);
        return k;
    }
    // what the post plan routes by
    PostPad geometry() const {
        PostPad g;
        g.on = on();
        g.gravity = p.gravity;
        g.width = (uint32_t)p.width;
        g.height = (uint32_t)p.height;
        return g;
    }
};
// IK_OK, or IK_ERR_INVALID with the message set (prefix: "" or "request i: "): a known mode
// (IK_PAD_NONE only with allow_none, and then with every other field 0) and gravity, sizes
// within 0..2^24, a colour within 0..0xFFFFFF, an alpha within 0..255 (ik_pad_host.cpp)
int pad_check(const ik_pad& p, const char* prefix, bool allow_none);
// an image, or same-geometry images in one launch, placed at g's origin on new canvases of
// g's size (the caller has resolved g: pad_canvas); r gives the mode, the colour and the
// alpha.  A return other than IK_OK from pad_group leaves every image to pad_image.  Both
// synchronise the stream.
int pad_image(const ik_image* img, const PadReq& r, const PadGeom& g, ik_image** out);
int pad_group(const std::vector<ik_image*>& src, const PadReq& r, const PadGeom& g, std::vector<ik_image*>& out);

// One request's options, resolved (ik_post_stage.cpp): what the *_fit, *_oriented and *_opts
// entry points ask for beyond (w, h, fmt, quality), in the order the steps run
struct RequestOps {
    int fit = IK_FIT_CONTAIN;
    int orient = 0;           // effective orientation: 0 = the pixels as stored, 2..8 = turned first
    int32_t bg = IK_BG_NONE;  // or 0xRRGGBB: an image with alpha is flattened onto it after the turn
    AdjustReq adj;            // the colour adjustment of the resized image (all zero: none)
    FilterReq flt;            // the blur or unsharpen after it (mode 0: none)
    PadReq pad;               // the canvas the result is placed on after it (mode 0: none)
    OverlayReq ovl;           // the watermark composited after it (mark null: none)
    bool is_default() const {
        return fit == IK_FIT_CONTAIN && !orient && bg == IK_BG_NONE && !adj.on() && !flt.mode && !pad.on() && !ovl.mark;
    }
};
bool opts_size_ok(size_t opt_size);  // one of the declared ik_request_opts* layouts
// the orientation an `orient` argument (ik_orient) means for these bytes: 0 = none
// (stored order, or an effective 1: no pass), 2..8, or -1 for a bad argument
int effective_orientation(const uint8_t* bytes, size_t len, int orient);
// A batch's options as records, checked request by request: from the *_fit and *_oriented
// calls' arrays (fit, orient; each null: the default) or from an *_opts call's array (opts,
// opt_size apart; null: the defaults).  ops is left empty when every request is at its
// defaults, so such a batch makes the calls of the plain submit.  bytes: the files in host
// memory, or null (device-resident inputs: IK_ORIENT_AUTO cannot be resolved and is refused).
// Returns IK_OK or IK_ERR_INVALID with the message set ("request i: ...").
int request_ops(const int* fit, const int* orient, const void* opts, size_t opt_size, uint32_t n,
                const uint8_t* const* bytes, const size_t* lens, std::vector<RequestOps>& ops);
// the same for a single-request call (fit and orient, or opts when it is not null), in the
// order ik_transform_opts checks; the messages carry no prefix
int single_request_ops(int fit, int orient, const void* opts, size_t opt_size, const uint8_t* bytes, size_t len,
                       RequestOps& r);

// decode_image on the calling thread's device (ik_host.cpp), and the thread's last message
int decode_one(const uint8_t* bytes, size_t len, ik_image** out, int* fmt_out);
std::string last_error_str();
// decode -> orient -> flatten -> resize -> adjust -> filter -> pad -> watermark -> encode of one request, here
int transform_here(const uint8_t* bytes, size_t len, int64_t w, int64_t h, const RequestOps& ops, int fmt, int quality,
                   int filter, uint8_t** out, size_t* out_len);
// a batch part between its stages (ik_host.cpp StageExec): the requests it holds and what
// each stage leaves for the next
struct HostPhase {
    std::vector<uint32_t> idx;
    std::vector<EncodePrep> prep;
    std::vector<std::vector<uint8_t>> bytes_out;
    int threads = 0;
    double t_resize = 0, t_front = 0;
    // the decode stage's results, for the post stage: decoded images, status, message
    std::vector<ik_image*> imgs;
    std::vector<int> ds;
    std::vector<std::string> dm;
};
// the post stage of a batch part (ik_post_stage.cpp); ops: null, or every request's options
void transform_post_phase(const int64_t* w, const int64_t* h, const RequestOps* ops, const int* fmt, const int* quality,
                          int filter, int* st, std::string* errs, HostPhase& hp);

// Per-device phase gates (ik_pool.cpp).  Concurrent batch calls on one device
// take its GPU phases in turn: kGateUpload covers a PNG batch's staging, H2D and
// block search, kGateKernels the decode kernels, kGatePost the resize and the
// encoders' device front ends (so one batch's resize runs beside the next batch's
// decode kernels).  A batch's host phases (libwebp / libavif coding) run outside
// all three, beside the next batch's kernels; its small kernels never queue
// behind another batch's long ones.  gate_pin keeps a gate held across
// gate_leave (a caller that spans several phases).
enum { kGateUpload = 0, kGateKernels = 1, kGatePost = 2 };
void gate_enter(int which);
bool gate_try_enter(int which);  // true if now held (or gates are off)
bool gate_held_any();            // this thread holds one of its device's gates
void gate_leave(int which);
void gate_pin(int which, bool on);

}  // namespace ik
