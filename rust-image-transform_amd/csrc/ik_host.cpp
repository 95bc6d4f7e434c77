// ik_host.cpp -- the C ABI of libimagekit_hip.so (include/imagekit_hip.h).
//
// Mirrors reference src/transform.rs: decode_image (:27-43), resize_image
// (:62-90), encode_image (:113-150) with the error mapping of src/lib.rs:34-52
// (every failure is a status + thread-local message, never a panic).  Pixels
// stay device-resident between the three calls; only compressed bytes cross
// PCIe (plus the small planes/coefficients handed to the host entropy coders).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <map>
#include <tuple>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <deque>

#include "../../include/imagekit_hip.h"
#include "ik_exif.h"
#include "ik_png.h"
#include "ik_runtime.h"
#include "ik_jpeg_walk.h"

namespace ik {

static thread_local std::string t_err;
static thread_local int t_device = -1;

int fail(int status, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    t_err = buf;
    return status;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(IK_ERR_DEVICE, "HIP error %d (%s) in %s", (int)e, hipGetErrorString(e), what);
}

int current_device() {
    if (t_device < 0) {
        int d = 0;
        if (hipGetDevice(&d) != hipSuccess) d = 0;
        t_device = d;
    }
    return t_device;
}

DeviceGuard::DeviceGuard(int device) : prev(current_device()) {
    if (device != prev) {
        t_device = device;
        (void)hipSetDevice(device);
    }
}
DeviceGuard::~DeviceGuard() {
    if (t_device != prev) {
        t_device = prev;
        (void)hipSetDevice(prev);
    }
}

// Per-thread HIP resources: a non-blocking stream per device, pinned staging
// arenas and grow-only device arenas.  Worker threads are persistent (ik_pool.cpp),
// so these live as long as the process; a caller's own thread releases its set
// when it exits.
namespace {
struct Arena {
    uint8_t* p = nullptr;
    size_t cap = 0;
    int device = 0;
};
struct ThreadRes {
    std::map<int, hipStream_t> streams, copy_streams, prio_streams;
    std::map<int, hipEvent_t> prio_events;
    std::map<int, std::array<hipEvent_t, 2>> fork_join;  // per device: an event records only on its own device's streams
    std::map<std::pair<int, int>, Arena> dev;  // (device, slot)
    Arena pinned[12];
    void release() {
        for (auto& kv : streams) (void)hipStreamSynchronize(kv.second);
        for (auto& kv : copy_streams) (void)hipStreamSynchronize(kv.second);
        for (auto& kv : prio_streams) (void)hipStreamSynchronize(kv.second);
        for (auto& kv : dev) {
            if (!kv.second.p) continue;
            (void)hipSetDevice(kv.second.device);
            (void)hipFree(kv.second.p);
            mem_stat(kMemArenaDev, -(int64_t)kv.second.cap);
        }
        for (Arena& a : pinned)
            if (a.p) {
                (void)hipHostFree(a.p);
                mem_stat(kMemArenaPinned, -(int64_t)a.cap);
            }
        for (auto& kv : streams) (void)hipStreamDestroy(kv.second);
        for (auto& kv : copy_streams) (void)hipStreamDestroy(kv.second);
        for (auto& kv : prio_streams) (void)hipStreamDestroy(kv.second);
        for (auto& kv : prio_events) (void)hipEventDestroy(kv.second);
        for (auto& kv : fork_join)
            for (hipEvent_t e : kv.second) (void)hipEventDestroy(e);
        fork_join.clear();
        streams.clear();
        copy_streams.clear();
        prio_streams.clear();
        prio_events.clear();
        dev.clear();
        for (Arena& a : pinned) a = Arena();
    }
    // a caller's own thread that exits releases its set here; workers and stage
    // threads release theirs before they end (ik_shutdown), and after ik_shutdown
    // the process's main thread holds none, so nothing is left to a destructor that
    // runs during process exit
    ~ThreadRes() { release(); }
};
ThreadRes& tres() {
    static thread_local ThreadRes r;
    return r;
}
}  // namespace

void release_thread_resources() { tres().release(); }

namespace {
std::mutex g_bt_mu;
// per device: the batches in the decode and post stages, the last one finished
std::map<int, std::vector<double>> g_bt_dec, g_bt_post, g_bt_last;
bool bt_post_field(int f) { return f >= kBtResizeMs && f < kBtHostWallMs; }
bool bt_host_field(int f) { return f >= kBtHostWallMs; }
thread_local bool t_bt_active = false;  // inside a stage's batch (BatchTimingScope)
// per device (an event records only on its own device's streams); the events are
// left to the runtime: a thread-exit destructor may run at process exit
struct ThreadEvents {
    std::map<int, std::array<EvPair, 4>> p;
};

// the lifetime lock (ApiGuard): shared by callers, exclusive for teardown, and
// writer-preferring -- a waiting teardown holds back new callers, so callers that
// keep calling (a server's request threads) cannot starve it
struct LifeLock {
    std::mutex mu;
    std::condition_variable cv;
    int readers = 0, writers_waiting = 0;
    bool writer = false;
    void lock_shared() {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return !writer && writers_waiting == 0; });
        ++readers;
    }
    void unlock_shared() {
        std::lock_guard<std::mutex> lk(mu);
        if (--readers == 0) cv.notify_all();
    }
    void lock() {
        std::unique_lock<std::mutex> lk(mu);
        ++writers_waiting;
        cv.wait(lk, [&] { return !writer && readers == 0; });
        --writers_waiting;
        writer = true;
    }
    void unlock() {
        std::lock_guard<std::mutex> lk(mu);
        writer = false;
        cv.notify_all();
    }
};
LifeLock g_life;
std::atomic<bool> g_closed{false};
thread_local int t_api_depth = 0;
thread_local bool t_internal = false;
}  // namespace

ApiGuard::ApiGuard() {
    if (t_internal) return;
    if (t_api_depth++ == 0) {
        g_life.lock_shared();
        held = true;
    }
    closed = g_closed.load(std::memory_order_acquire);
}
ApiGuard::~ApiGuard() {
    if (t_internal) return;
    if (--t_api_depth == 0 && held) g_life.unlock_shared();
}
void mark_internal_thread() { t_internal = true; }

namespace {
std::atomic<int64_t> g_mem[kMemStats];
}  // namespace
void mem_stat(int which, int64_t delta) { g_mem[which].fetch_add(delta, std::memory_order_relaxed); }

BatchTimingScope::BatchTimingScope() : prev(t_bt_active) { t_bt_active = true; }
BatchTimingScope::~BatchTimingScope() { t_bt_active = prev; }

void ev_record(hipEvent_t e, hipStream_t s) {
    if (e && hipEventRecord(e, s) != hipSuccess) (void)hipGetLastError();
}

void batch_timing_reset(int device, bool post) {
    std::lock_guard<std::mutex> lk(g_bt_mu);
    (post ? g_bt_post : g_bt_dec)[device].assign(kBtFields, 0.0);
}
void batch_timing_commit(int device, bool post) {
    std::lock_guard<std::mutex> lk(g_bt_mu);
    std::vector<double>& src = (post ? g_bt_post : g_bt_dec)[device];
    std::vector<double>& dst = g_bt_last[device];
    src.resize(kBtFields, 0.0);
    dst.resize(kBtFields, 0.0);
    for (int f = 0; f < kBtFields; ++f)
        if (!bt_host_field(f) && bt_post_field(f) == post) dst[(size_t)f] = src[(size_t)f];
}
void batch_timing_host(int device, double wall_ms, double core_ms, double images) {
    std::lock_guard<std::mutex> lk(g_bt_mu);
    std::vector<double>& dst = g_bt_last[device];
    dst.resize(kBtFields, 0.0);
    dst[kBtHostWallMs] = wall_ms;
    dst[kBtHostCoreMs] = core_ms;
    dst[kBtHostImages] = images;
}
void batch_timing_add(int device, int field, double v) {
    if (!t_bt_active) return;
    std::lock_guard<std::mutex> lk(g_bt_mu);
    std::vector<double>& t = (bt_post_field(field) ? g_bt_post : g_bt_dec)[device];
    if (t.size() < (size_t)kBtFields) t.resize(kBtFields, 0.0);
    t[(size_t)field] += v;
}
EvPair& thread_events(int which) {
    static thread_local ThreadEvents te;
    EvPair& e = te.p[current_device()][which & 3];
    if (!e.a && hipEventCreate(&e.a) != hipSuccess) e.a = nullptr;
    if (!e.b && hipEventCreate(&e.b) != hipSuccess) e.b = nullptr;
    return e;
}
float ev_pair_ms(const EvPair& e) {
    float ms = 0;
    if (!e.a || !e.b || hipEventElapsedTime(&ms, e.a, e.b) != hipSuccess) return 0.f;
    return ms;
}

hipStream_t thread_stream() {
    ThreadRes& r = tres();
    const int d = current_device();
    auto it = r.streams.find(d);
    if (it != r.streams.end()) return it->second;
    (void)hipSetDevice(d);
    hipStream_t s = nullptr;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) return nullptr;
    r.streams[d] = s;
    return s;
}

// The upload stream (PCIe copies of whole batches: 2.25 GB on the bench, ~42 ms)
// at the lowest stream priority: a stream of another priority never shares its
// hardware queue, so no kernel of another stage waits in queue order behind a
// batch's DMA (GPU_MAX_HW_QUEUES is 4: same-priority streams share queues).
hipStream_t thread_copy_stream() {
    ThreadRes& r = tres();
    const int d = current_device();
    auto it = r.copy_streams.find(d);
    if (it != r.copy_streams.end()) return it->second;
    (void)hipSetDevice(d);
    hipStream_t s = nullptr;
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = greatest = 0;
    // (the priority other than the default one: the lowest if it is not the default)
    const int prio = least != 0 ? least : greatest;
    if (getenv("IK_TIMING")) fprintf(stderr, "[streams] priority range %d..%d: upload stream at %d\n", least, greatest, prio);
    if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, prio) != hipSuccess &&
        hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess)
        return nullptr;
    r.copy_streams[d] = s;
    return s;
}

bool thread_prio_stream(hipStream_t* out, hipEvent_t* ev) {
    ThreadRes& r = tres();
    const int d = current_device();
    auto it = r.prio_streams.find(d);
    if (it == r.prio_streams.end()) {
        (void)hipSetDevice(d);
        hipStream_t s = nullptr;
        hipEvent_t e = nullptr;
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = greatest = 0;
        if (hipStreamCreateWithPriority(&s, hipStreamNonBlocking, greatest) != hipSuccess) return false;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) {
            (void)hipStreamDestroy(s);
            return false;
        }
        it = r.prio_streams.emplace(d, s).first;
        r.prio_events[d] = e;
    }
    *out = it->second;
    if (ev) *ev = r.prio_events[d];
    return true;
}

bool thread_fork_join_events(hipEvent_t* fork, hipEvent_t* join) {
    ThreadRes& r = tres();
    const int d = current_device();
    auto it = r.fork_join.find(d);
    if (it == r.fork_join.end()) {
        (void)hipSetDevice(d);
        hipEvent_t f = nullptr, j = nullptr;
        if (hipEventCreateWithFlags(&f, hipEventDisableTiming) != hipSuccess) return false;
        if (hipEventCreateWithFlags(&j, hipEventDisableTiming) != hipSuccess) {
            (void)hipEventDestroy(f);
            return false;
        }
        it = r.fork_join.emplace(d, std::array<hipEvent_t, 2>{f, j}).first;
    }
    *fork = it->second[0];
    *join = it->second[1];
    return true;
}

uint8_t* pinned_slot(int slot, size_t bytes) {
    Arena& a = tres().pinned[slot];
    if (bytes <= a.cap) return a.p;
    if (a.p) {
        (void)hipStreamSynchronize(thread_stream());  // no copy may still read the old buffer
        auto cs = tres().copy_streams.find(current_device());
        if (cs != tres().copy_streams.end()) (void)hipStreamSynchronize(cs->second);
        auto ps = tres().prio_streams.find(current_device());
        if (ps != tres().prio_streams.end()) (void)hipStreamSynchronize(ps->second);
        (void)hipHostFree(a.p);
        mem_stat(kMemArenaPinned, -(int64_t)a.cap);
    }
    a.p = nullptr;
    a.cap = 0;
    size_t want = bytes < (1u << 20) ? (1u << 20) : bytes;
    const hipError_t e = hipHostMalloc((void**)&a.p, want, hipHostMallocDefault);
    if (e != hipSuccess) {
        a.p = nullptr;
        fail(IK_ERR_NOMEM, "hipHostMalloc(%zu bytes): %s", want, hipGetErrorString(e));
        return nullptr;
    }
    a.cap = want;
    mem_stat(kMemArenaPinned, (int64_t)want);
    return a.p;
}

// Caller-pinned ranges (ik_host_alloc / ik_host_register): inputs inside one are
// DMAed in place.  Keyed by start address; the ranges never overlap.
namespace {
struct PinnedRange {
    size_t n = 0;
    bool owned = false;  // ik_host_alloc (hipHostFree) vs ik_host_register (hipHostUnregister)
};
std::mutex g_pin_mu;
std::map<uintptr_t, PinnedRange> g_pins;
}  // namespace

bool host_pinned(const void* p, size_t n) {
    const uintptr_t a = (uintptr_t)p;
    std::lock_guard<std::mutex> lk(g_pin_mu);
    auto it = g_pins.upper_bound(a);
    if (it == g_pins.begin()) return false;
    --it;
    return a >= it->first && a - it->first <= it->second.n && n <= it->second.n - (a - it->first);
}

// Host <-> device copies of pageable memory go through a per-thread pinned
// staging buffer with stream-ordered async copies on the thread's stream.  (A
// synchronous hipMemcpy* from pageable memory is issued on the null stream, and
// a non-blocking stream is not ordered after its DMA.)
static uint8_t* staging(size_t bytes) { return pinned_slot(kPinnedStaging, bytes); }

int copy_h2d_2d(uint8_t* dst, size_t dpitch, const uint8_t* src, size_t spitch, size_t width,
                size_t height, hipStream_t s) {
    const size_t chunk_rows = height ? (size_t)((64u << 20) / (width ? width : 1)) + 1 : 1;
    for (size_t y0 = 0; y0 < height; y0 += chunk_rows) {
        const size_t rows = height - y0 < chunk_rows ? height - y0 : chunk_rows;
        uint8_t* st = staging(rows * width);
        if (!st) return IK_ERR_NOMEM;  // pinned_slot recorded the error
        for (size_t y = 0; y < rows; ++y) std::memcpy(st + y * width, src + (y0 + y) * spitch, width);
        IK_HIP(hipMemcpy2DAsync(dst + y0 * dpitch, dpitch, st, width, width, rows, hipMemcpyHostToDevice, s));
        IK_HIP(hipStreamSynchronize(s));
    }
    return IK_OK;
}

int copy_d2h_2d(uint8_t* dst, size_t dpitch, const uint8_t* src, size_t spitch, size_t width,
                size_t height, hipStream_t s) {
    const size_t chunk_rows = height ? (size_t)((64u << 20) / (width ? width : 1)) + 1 : 1;
    for (size_t y0 = 0; y0 < height; y0 += chunk_rows) {
        const size_t rows = height - y0 < chunk_rows ? height - y0 : chunk_rows;
        uint8_t* st = staging(rows * width);
        if (!st) return IK_ERR_NOMEM;  // pinned_slot recorded the error
        IK_HIP(hipMemcpy2DAsync(st, width, src + y0 * spitch, spitch, width, rows, hipMemcpyDeviceToHost, s));
        IK_HIP(hipStreamSynchronize(s));
        for (size_t y = 0; y < rows; ++y) std::memcpy(dst + (y0 + y) * dpitch, st + y * width, width);
    }
    return IK_OK;
}

// Per-thread, per-device device scratch (grown with hipMalloc; never the
// stream-ordered allocator).  Valid until the next scratch() call on this thread.
uint8_t* scratch_slot(int slot, size_t bytes) {
    const int d = current_device();
    Arena& a = tres().dev[{d, slot}];
    a.device = d;
    if (bytes <= a.cap) return a.p;
    if (a.p) {
        (void)hipStreamSynchronize(thread_stream());
        auto ps = tres().prio_streams.find(d);
        if (ps != tres().prio_streams.end()) (void)hipStreamSynchronize(ps->second);
        (void)hipFree(a.p);
        mem_stat(kMemArenaDev, -(int64_t)a.cap);
    }
    a.p = nullptr;
    a.cap = 0;
    // grow geometrically so a run of slightly larger requests does not re-allocate each time
    size_t want = bytes < (4u << 20) ? (4u << 20) : bytes + bytes / 8;
    (void)hipSetDevice(d);
    if (hipMalloc((void**)&a.p, want) != hipSuccess) return nullptr;
    a.cap = want;
    mem_stat(kMemArenaDev, (int64_t)want);
    return a.p;
}

uint8_t* scratch(size_t bytes) { return scratch_slot(kScratchDefault, bytes); }

size_t pitch_for(uint32_t w, uint32_t c) { return ((size_t)w * c + 255) & ~size_t(255); }

// Device image blocks are recycled per device: hipFree synchronises the whole
// device, which would serialise every thread's stream under request load.  A
// freed block is kept (up to kPoolBytes per device) and handed to the next image
// that fits in it; every API call has synchronised its own stream before it
// returns, so a block is idle when it comes back.
namespace {
// 32 GiB of the 288 GB: two 64-frame 4096^2 batches in flight hold 8 GiB of decoded
// frames; at 4 GiB the pool overflowed every batch, and each hipFree of an
// overflowing block stalled the whole device (and every concurrent batch)
constexpr size_t kPoolBytes = size_t(32) << 30;
struct ImagePool {
    std::mutex mu;
    std::multimap<size_t, uint8_t*> free_blocks;
    size_t held = 0;
};
std::mutex g_ipool_mu;
std::map<int, ImagePool*> g_ipools;
ImagePool& image_pool(int device) {
    std::lock_guard<std::mutex> lk(g_ipool_mu);
    ImagePool*& p = g_ipools[device];
    if (!p) p = new ImagePool();
    return *p;
}
size_t block_size(size_t bytes) {  // 64 KiB granules: images of similar sizes share blocks
    return (bytes + (size_t(64) << 10) - 1) & ~((size_t(64) << 10) - 1);
}
}  // namespace

int alloc_image(uint32_t w, uint32_t h, uint32_t c, ik_image** out, uint32_t depth) {
    auto* img = new ik_image();
    img->w = w; img->h = h; img->c = c; img->depth = depth;
    img->pitch = pitch_for(w, c * depth);
    img->device = current_device();
    (void)hipSetDevice(img->device);
    // + 16 bytes: the fused kernel's 8-byte lane loads may touch the pitch tail
    const size_t need = block_size(img->pitch * (size_t)(h ? h : 1) + 16);
    ImagePool& pool = image_pool(img->device);
    {
        std::lock_guard<std::mutex> lk(pool.mu);
        auto it = pool.free_blocks.lower_bound(need);
        if (it != pool.free_blocks.end() && it->first <= 2 * need) {  // reuse a block at most twice the size
            img->d = it->second;
            img->block = it->first;
            pool.held -= it->first;
            pool.free_blocks.erase(it);
            mem_stat(kMemImageFree, -(int64_t)img->block);
        }
    }
    if (!img->d) {
        hipError_t e = hipMalloc(&img->d, need);
        if (e != hipSuccess) { delete img; return hip_fail(e, "hipMalloc(image)"); }
        img->block = need;
    }
    mem_stat(kMemImageLive, (int64_t)img->block);
    *out = img;
    return IK_OK;
}

namespace {
std::atomic<int> g_resize_mode{-1};  // -1 = not yet read from IK_RESIZE_MODE
}  // namespace

int resize_mode() {
    int m = g_resize_mode.load();
    if (m < 0) {
        const char* e = getenv("IK_RESIZE_MODE");
        m = (e && (!strcmp(e, "fma") || !strcmp(e, "1"))) ? IK_RESIZE_FMA : IK_RESIZE_EXACT;
        int expected = -1;
        g_resize_mode.compare_exchange_strong(expected, m);
        m = g_resize_mode.load();
    }
    return m;
}

namespace {
std::atomic<unsigned long long> g_flatten_launches{0}, g_flatten_images{0};  // ik_flatten_counters
}  // namespace

void flatten_count(uint64_t launches, uint64_t images) {
    g_flatten_launches += launches;
    g_flatten_images += images;
}

}  // namespace ik

using namespace ik;

extern "C" {

const char* ik_version(void) { return "imagekit-hip 0.1.0 (gfx950)"; }

int ik_host_alloc(size_t bytes, void** out) {
    if (!out) return fail(IK_ERR_INVALID, "null pointer");
    *out = nullptr;
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable);
    if (e != hipSuccess) return fail(IK_ERR_NOMEM, "hipHostMalloc(%zu bytes): %s", bytes, hipGetErrorString(e));
    std::lock_guard<std::mutex> lk(g_pin_mu);
    g_pins[(uintptr_t)p] = PinnedRange{bytes, true};
    *out = p;
    return IK_OK;
}

int ik_host_free(void* p) {
    if (!p) return IK_OK;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = g_pins.find((uintptr_t)p);
        if (it == g_pins.end() || !it->second.owned) return fail(IK_ERR_INVALID, "not an ik_host_alloc pointer");
        g_pins.erase(it);
    }
    IK_HIP(hipHostFree(p));
    return IK_OK;
}

int ik_host_register(void* p, size_t bytes) {
    if (!p || !bytes) return fail(IK_ERR_INVALID, "empty range");
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = g_pins.upper_bound((uintptr_t)p + bytes - 1);
        if (it != g_pins.begin()) {
            --it;
            if (it->first + it->second.n > (uintptr_t)p) return fail(IK_ERR_INVALID, "range overlaps a pinned range");
        }
    }
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterPortable);
    if (e != hipSuccess) return fail(IK_ERR_NOMEM, "hipHostRegister(%zu bytes): %s", bytes, hipGetErrorString(e));
    std::lock_guard<std::mutex> lk(g_pin_mu);
    g_pins[(uintptr_t)p] = PinnedRange{bytes, false};
    return IK_OK;
}

int ik_host_unregister(void* p) {
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = g_pins.find((uintptr_t)p);
        if (it == g_pins.end() || it->second.owned) return fail(IK_ERR_INVALID, "not an ik_host_register range");
        g_pins.erase(it);
    }
    IK_HIP(hipHostUnregister(p));
    return IK_OK;
}

size_t ik_last_error(char* buf, size_t cap) {
    const std::string& e = t_err;
    if (buf && cap) {
        size_t n = e.size() < cap - 1 ? e.size() : cap - 1;
        std::memcpy(buf, e.data(), n);
        buf[n] = 0;
    }
    return e.size();
}

int ik_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// How host threads wait for the GPU.  HIP's default (hipDeviceScheduleAuto) spins
// the waiting thread on the CPU; the batch paths have several threads waiting on
// device work at once (stage threads, lane checks) while the host coders (libwebp)
// need every core of the quota, so the library asks for blocking waits
// (hipDeviceScheduleBlockingSync: the thread sleeps until the GPU signals).
// IK_SYNC=spin keeps the spinning.  Applied once per visible device, process-wide.
static void apply_sync_mode(int ndev) {
    static std::once_flag once;
    std::call_once(once, [ndev] {
        const char* e = getenv("IK_SYNC");
        if (e && !strcmp(e, "spin")) return;
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess) cur = 0;
        for (int d = 0; d < ndev; ++d) {
            if (hipSetDevice(d) != hipSuccess) continue;
            const hipError_t r = hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
            if (r != hipSuccess && getenv("IK_TIMING"))
                fprintf(stderr, "[init] device %d: blocking sync not set (%s)\n", d, hipGetErrorString(r));
        }
        (void)hipSetDevice(cur);
    });
}

int ik_init(int device) {
    IK_API_ENTER();
    int n = 0;
    IK_HIP(hipGetDeviceCount(&n));
    apply_sync_mode(n);
    if (device >= n) return fail(IK_ERR_INVALID, "device %d out of range (%d devices)", device, n);
    if (device < 0) {  // every visible GPU (or IK_DEVICES): one process, many devices
        if (int rc = sched_configure(nullptr, 0)) return rc;
        device = sched_phys(0);
    }
    t_device = device;
    IK_HIP(hipSetDevice(current_device()));
    if (!thread_stream()) return fail(IK_ERR_DEVICE, "cannot create HIP stream");
    return IK_OK;
}

int ik_init_devices(const int* devices, int n) {
    IK_API_ENTER();
    if (!devices || n <= 0) return fail(IK_ERR_INVALID, "empty device list");
    if (int rc = sched_configure(devices, n)) return rc;
    return ik_init(sched_phys(0));
}

int ik_logical_device_count(void) { return sched_multi() ? sched_count() : 0; }

int ik_logical_device_stats(uint32_t logical, uint64_t* jobs, uint64_t* cost_done, uint64_t* outstanding) {
    IK_API_ENTER();
    if (!sched_multi()) return fail(IK_ERR_INVALID, "multi-device dispatch is not enabled");
    return sched_stats(logical, jobs, cost_done, outstanding);
}

uint64_t ik_request_cost(const uint8_t* bytes, size_t len, int64_t w, int64_t h, int fmt) {
    return request_cost(bytes, len, w, h, fmt);
}

void ik_schedule_plan(const uint64_t* costs, uint32_t n, uint32_t ndev, const uint64_t* outstanding,
                      uint32_t* assign) {
    if (!costs || !assign || !ndev) return;
    sched_plan(costs, n, ndev, outstanding, assign);
}

int ik_post_plan(uint32_t m, const int* ok, const uint32_t* W, const uint32_t* H, const uint32_t* C,
                 const uint64_t* pitch, const int* device, const uint32_t* depth, const int64_t* w, const int64_t* h,
                 const int* fmt, const int* quality, int webp_encoder, int mixed_mode, uint32_t* nw, uint32_t* nh,
                 int* resize_group, int* coder_group, int* route, uint32_t* info) {
    return ik_post_plan_fit(m, ok, W, H, C, pitch, device, depth, w, h, nullptr, fmt, quality, webp_encoder, mixed_mode,
                            nw, nh, resize_group, coder_group, route, info, nullptr);
}

int ik_post_plan_fit(uint32_t m, const int* ok, const uint32_t* W, const uint32_t* H, const uint32_t* C,
                     const uint64_t* pitch, const int* device, const uint32_t* depth, const int64_t* w,
                     const int64_t* h, const int* fit, const int* fmt, const int* quality, int webp_encoder,
                     int mixed_mode, uint32_t* nw, uint32_t* nh, int* resize_group, int* coder_group, int* route,
                     uint32_t* info, uint32_t* window) {
    if (!ok || !W || !H || !C || !pitch || !device || !depth || !w || !h || !fmt || !quality || !nw || !nh ||
        !resize_group || !coder_group || !route || !info)
        return fail(IK_ERR_INVALID, "null pointer");
    std::vector<PostRequest> rq(m);
    for (uint32_t k = 0; k < m; ++k) {
        rq[k].ok = ok[k] != 0;
        rq[k].W = W[k]; rq[k].H = H[k]; rq[k].C = C[k];
        rq[k].pitch = (size_t)pitch[k]; rq[k].device = device[k]; rq[k].depth = depth[k];
        rq[k].w = w[k]; rq[k].h = h[k]; rq[k].fmt = fmt[k]; rq[k].quality = quality[k];
        if (fit) {
            if (fit[k] < IK_FIT_CONTAIN || fit[k] > IK_FIT_EXACT) return fail(IK_ERR_INVALID, "unknown fit %d", fit[k]);
            rq[k].fit = fit[k];
        }
    }
    const PostPlan P = post_plan(rq.data(), m, webp_encoder, mixed_mode);
    for (uint32_t k = 0; k < m; ++k) {
        const PostPlan::Req& q = P.req[k];
        nw[k] = q.sized ? q.nw : 0;
        nh[k] = q.sized ? q.nh : 0;
        resize_group[k] = q.rgroup;
        coder_group[k] = q.cgroup;
        route[k] = (int)q.route;
        if (window) {
            const FitWindow f = q.sized ? q.win : FitWindow();
            const uint32_t v[6] = {f.iw, f.ih, f.x0, f.y0, f.nw, f.nh};
            std::copy(v, v + 6, window + 6 * (size_t)k);
        }
    }
    info[0] = P.mixed;
    info[1] = (uint32_t)P.mixed_min;
    info[2] = (uint32_t)P.rgroups.size();
    info[3] = (uint32_t)P.cgroups.size();
    return IK_OK;
}

uint32_t ik_schedule_split(const uint64_t* costs, uint32_t n, uint32_t ndev, const uint64_t* outstanding,
                           uint32_t min_batch, uint32_t* part_lo, uint32_t* part_dev) {
    if (!costs || !part_lo || !part_dev || !ndev) return 0;
    std::vector<uint64_t> out(ndev, 0);
    if (outstanding) std::copy(outstanding, outstanding + ndev, out.begin());
    return sched_split(costs, n, ndev, min_batch, out.data(), part_lo, part_dev);
}

int ik_image_from_host(const uint8_t* pixels, uint32_t width, uint32_t height, uint32_t channels,
                       ik_image** out) {
    IK_API_ENTER();
    if (!out || (!pixels && width && height)) return fail(IK_ERR_INVALID, "null pointer");
    if (channels < 1 || channels > 4) return fail(IK_ERR_INVALID, "channels must be 1..4");
    ik_image* img = nullptr;
    int st = alloc_image(width, height, channels, &img);
    if (st) return st;
    if (width && height) {
        const size_t row = (size_t)width * channels;
        int rc = copy_h2d_2d(img->d, img->pitch, pixels, row, row, height, thread_stream());
        if (rc) { ik_image_free(img); return rc; }
    }
    *out = img;
    return IK_OK;
}

int ik_image_from_host16(const uint16_t* pixels, uint32_t width, uint32_t height, uint32_t channels,
                         ik_image** out) {
    IK_API_ENTER();
    if (!out || (!pixels && width && height)) return fail(IK_ERR_INVALID, "null pointer");
    if (channels < 1 || channels > 4) return fail(IK_ERR_INVALID, "channels must be 1..4");
    ik_image* img = nullptr;
    int st = alloc_image(width, height, channels, &img, 2);
    if (st) return st;
    if (width && height) {
        const size_t row = (size_t)width * channels * 2;
        int rc = copy_h2d_2d(img->d, img->pitch, reinterpret_cast<const uint8_t*>(pixels), row, row, height,
                             thread_stream());
        if (rc) { ik_image_free(img); return rc; }
    }
    *out = img;
    return IK_OK;
}

int ik_image_depth(const ik_image* img) { return img ? (int)img->depth : 0; }

int ik_image_wrap_device(uint8_t* dev_pixels, uint32_t width, uint32_t height, uint32_t channels,
                         size_t pitch, ik_image** out) {
    IK_API_ENTER();
    if (!out || !dev_pixels) return fail(IK_ERR_INVALID, "null pointer");
    if (channels < 1 || channels > 4) return fail(IK_ERR_INVALID, "channels must be 1..4");
    if (pitch < (size_t)width * channels) return fail(IK_ERR_INVALID, "pitch smaller than a row");
    auto* img = new ik_image();
    img->w = width; img->h = height; img->c = channels; img->pitch = pitch;
    img->d = dev_pixels; img->owned = false; img->device = current_device();
    *out = img;
    return IK_OK;
}

int ik_image_info(const ik_image* img, uint32_t* w, uint32_t* h, uint32_t* c) {
    if (!img) return fail(IK_ERR_INVALID, "null image");
    if (w) *w = img->w;
    if (h) *h = img->h;
    if (c) *c = img->c;
    return IK_OK;
}

int ik_image_to_host(const ik_image* img, uint8_t* dst, size_t cap) {
    IK_API_ENTER();
    if (!img || !dst) return fail(IK_ERR_INVALID, "null pointer");
    const size_t row = (size_t)img->w * img->c * img->depth;
    if (cap < row * img->h) return fail(IK_ERR_INVALID, "destination too small");
    if (!row || !img->h) return IK_OK;
    DeviceGuard g(img->device);
    return copy_d2h_2d(dst, row, img->d, img->pitch, row, img->h, thread_stream());
}

void ik_image_free(ik_image* img) {
    IK_API_ENTER_VOID();
    if (!img) return;
    if (img->owned && img->d) {
        ImagePool& pool = image_pool(img->device);
        bool kept = false;
        if (img->block) {
            mem_stat(kMemImageLive, -(int64_t)img->block);
            std::lock_guard<std::mutex> lk(pool.mu);
            if (pool.held + img->block <= kPoolBytes) {
                pool.free_blocks.emplace(img->block, img->d);
                pool.held += img->block;
                kept = true;
                mem_stat(kMemImageFree, (int64_t)img->block);
            }
        }
        if (!kept) {
            DeviceGuard g(img->device);
            (void)hipFree(img->d);
        }
    }
    delete img;
}

void ik_buf_free(uint8_t* buf) { free(buf); }

// imageops::resize(image, nw, nh, filter)
int ik_resize_exact(const ik_image* img, uint32_t nw, uint32_t nh, int filter, ik_image** out) {
    IK_API_ENTER();
    if (nw == 0 || nh == 0) return fail(IK_ERR_INVALID, "zero output dimension");
    return ik_resize_window(img, nw, nh, 0, 0, nw, nh, filter, out);
}

// imageops::resize(image, iw, ih, filter) cropped to (x0, y0, nw, nh): only the window
// is computed
int ik_resize_window(const ik_image* img, uint32_t iw, uint32_t ih, uint32_t x0, uint32_t y0, uint32_t nw,
                     uint32_t nh, int filter, ik_image** out) {
    IK_API_ENTER();
    if (!img || !out) return fail(IK_ERR_INVALID, "null pointer");
    if (filter < 0 || filter > 4) return fail(IK_ERR_INVALID, "unknown filter %d", filter);
    if (nw == 0 || nh == 0) return fail(IK_ERR_INVALID, "zero output dimension");
    if ((uint64_t)x0 + nw > iw || (uint64_t)y0 + nh > ih)
        return fail(IK_ERR_INVALID, "window %ux%u at (%u, %u) outside %ux%u", nw, nh, x0, y0, iw, ih);
    if (iw > 0x7FFFFFFFu || ih > 0x7FFFFFFFu) return fail(IK_ERR_INVALID, "dimension overflow");
    DeviceGuard g(img->device);
    ik_image* o = nullptr;
    int st = alloc_image(nw, nh, img->c, &o, img->depth);
    if (st) return st;
    hipStream_t s = thread_stream();
    const size_t orow = (size_t)nw * img->c * img->depth;
    if (img->w == 0 || img->h == 0) {  // "nothing to sample from": blank image
        hipError_t e = hipMemset2DAsync(o->d, o->pitch, 0, orow, nh, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { ik_image_free(o); return hip_fail(e, "blank image"); }
        *out = o;
        return IK_OK;
    }
    if (iw == img->w && ih == img->h) {  // copy instead of resampling
        const uint8_t* from = img->d + (size_t)y0 * img->pitch + (size_t)x0 * img->c * img->depth;
        hipError_t e = hipMemcpy2DAsync(o->d, o->pitch, from, img->pitch, orow, nh, hipMemcpyDeviceToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { ik_image_free(o); return hip_fail(e, "copy image"); }
        *out = o;
        return IK_OK;
    }
    int rc;
    if (img->depth == 2) {  // 16-bit: the two-pass path over u16 samples
        ResizePlan* plan = get_resize_plan_window(current_device(), (int)img->w, (int)img->h, (int)img->c, (int)iw,
                                                  (int)ih, (int)x0, (int)y0, (int)nw, (int)nh, filter, 1);
        float* tmp = plan ? (float*)scratch(sizeof(float) * (size_t)nh * plan->args.tmp_span) : nullptr;
        if (!plan || !tmp) rc = fail(IK_ERR_DEVICE, "cannot set up the 16-bit resize");
        else {
            hipError_t e = launch_resize16(*plan, img->d, img->pitch, o->d, o->pitch, tmp, s);
            rc = e == hipSuccess ? IK_OK : hip_fail(e, "resize (16-bit)");
        }
    } else {
        rc = ik_resize_window_batch_device(img->d, img->w, img->h, img->c, img->pitch, 0, 1, iw, ih, x0, y0, nw, nh,
                                           filter, o->d, o->pitch, 0, s);
    }
    if (rc == IK_OK) {
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = hip_fail(e, "resize");
    }
    if (rc) { ik_image_free(o); return rc; }
    *out = o;
    return IK_OK;
}

}  // extern "C"

namespace ik {

// The output size of src/transform.rs:62-90 + DynamicImage::resize for a w x h
// image and the request's (w, h) options (-1 = None; not both None): the
// arithmetic is resize_target_dims (ik_post_plan.h), shared with the post plan
int resize_target(uint32_t W, uint32_t H, int64_t w, int64_t h, uint32_t* onw, uint32_t* onh) {
    switch (resize_target_dims(W, H, w, h, onw, onh)) {
        case 0: return IK_OK;
        case 1: return fail(IK_ERR_INVALID, "dimension exceeds u32");
        default: return fail(IK_ERR_INVALID, "dimension overflow");
    }
}

}  // namespace ik

extern "C" {

// src/transform.rs:62-90 then DynamicImage::resize (image 0.25.8):
// (nw,nh) == dims -> clone; else resize_dimensions(..., fill=false) (aspect FIT,
// f64, round, max 1) -> imageops::resize.
int ik_resize(ik_image* img, int64_t w, int64_t h, int filter, ik_image** out) {
    IK_API_ENTER();
    return ik_resize_fit(img, w, h, IK_FIT_CONTAIN, filter, out);
}

int ik_fit_target(uint32_t W, uint32_t H, int64_t w, int64_t h, int fit, uint32_t* out) {
    if (!out) return fail(IK_ERR_INVALID, "null pointer");
    if (fit < IK_FIT_CONTAIN || fit > IK_FIT_EXACT) return fail(IK_ERR_INVALID, "unknown fit %d", fit);
    if (w < 0 && h < 0) return fail(IK_ERR_INVALID, "no target: w and h are both None");
    FitWindow f;
    switch (fit_target(W, H, w, h, fit, &f)) {
        case 0: break;
        case 1: return fail(IK_ERR_INVALID, "dimension exceeds u32");
        default: return fail(IK_ERR_INVALID, "dimension overflow");
    }
    out[0] = f.iw; out[1] = f.ih; out[2] = f.x0; out[3] = f.y0; out[4] = f.nw; out[5] = f.nh;
    return IK_OK;
}

// resize_image under a fit mode: CONTAIN is src/transform.rs:62-90 as above; COVER is
// DynamicImage::resize_to_fill and EXACT DynamicImage::resize_exact on the same target
int ik_resize_fit(ik_image* img, int64_t w, int64_t h, int fit, int filter, ik_image** out) {
    IK_API_ENTER();
    if (!img || !out) return fail(IK_ERR_INVALID, "null pointer");
    if (fit < IK_FIT_CONTAIN || fit > IK_FIT_EXACT) return fail(IK_ERR_INVALID, "unknown fit %d", fit);
    if (w < 0 && h < 0) { *out = img; return IK_OK; }
    uint32_t f[6];
    const int st = ik_fit_target(img->w, img->h, w, h, fit, f);
    if (st) return st;
    return ik_resize_window(img, f[0], f[1], f[2], f[3], f[4], f[5], filter, out);
}

int ik_exif_orientation(const uint8_t* bytes, size_t len) { return exif_orientation(bytes, len); }

int ik_orient_tile(void) { return kOrientTile; }
int ik_orient_strip(void) { return kOrientStrip; }

int ik_orient_batch_device(const uint8_t* dev_src, uint32_t W, uint32_t H, uint32_t C, uint32_t depth, size_t src_pitch,
                           size_t src_image_stride, uint32_t n, int orientation, uint8_t* dev_dst, size_t dst_pitch,
                           size_t dst_image_stride, void* hip_stream) {
    IK_API_ENTER();
    if (orientation < 1 || orientation > 8) return fail(IK_ERR_INVALID, "orientation %d outside 1..8", orientation);
    if (!dev_src || !dev_dst) return fail(IK_ERR_INVALID, "null device pointer");
    if (C < 1 || C > 4 || depth < 1 || depth > 2 || !W || !H || !n) return fail(IK_ERR_INVALID, "bad geometry");
    const bool t = orientation >= 5;
    const uint32_t ow = t ? H : W, oh = t ? W : H;
    const size_t px = (size_t)C * depth;
    if (src_pitch < W * px || dst_pitch < ow * px) return fail(IK_ERR_INVALID, "pitch too small");
    if (n > 1 && (src_image_stride < src_pitch * H || dst_image_stride < dst_pitch * oh))
        return fail(IK_ERR_INVALID, "image stride too small");
    if (n > kOrientMaxImages) return fail(IK_ERR_INVALID, "more than %u images", kOrientMaxImages);
    if (t && H > 65535u * kOrientTile) return fail(IK_ERR_INVALID, "image too tall to transpose");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : thread_stream();
    if (orientation == 1) {  // a plain pitched copy
        for (uint32_t i = 0; i < n; ++i)
            IK_HIP(hipMemcpy2DAsync(dev_dst + i * dst_image_stride, dst_pitch, dev_src + i * src_image_stride, src_pitch,
                                    W * px, H, hipMemcpyDeviceToDevice, s));
        return IK_OK;
    }
    const hipError_t e = launch_orient(dev_src, src_pitch, src_image_stride, dev_dst, dst_pitch, dst_image_stride, W, H,
                                       (int)px, orientation, (int)n, s);
    if (e != hipSuccess) return hip_fail(e, "orientation kernel launch");
    return IK_OK;
}

// DynamicImage::apply_orientation: a new image on the device that holds img
int ik_image_orient(const ik_image* img, int orientation, ik_image** out) {
    IK_API_ENTER();
    if (!img || !out) return fail(IK_ERR_INVALID, "null pointer");
    if (orientation < 1 || orientation > 8) return fail(IK_ERR_INVALID, "orientation %d outside 1..8", orientation);
    DeviceGuard g(img->device);
    const bool t = orientation >= 5;
    ik_image* o = nullptr;
    int rc = alloc_image(t ? img->h : img->w, t ? img->w : img->h, img->c, &o, img->depth);
    if (rc) return rc;
    if (img->w && img->h) {
        hipStream_t s = thread_stream();
        rc = ik_orient_batch_device(img->d, img->w, img->h, img->c, img->depth, img->pitch, 0, 1, orientation, o->d,
                                    o->pitch, 0, s);
        if (rc == IK_OK) {
            const hipError_t e = hipStreamSynchronize(s);
            if (e != hipSuccess) rc = hip_fail(e, "orientation");
        }
    }
    if (rc) { ik_image_free(o); return rc; }
    *out = o;
    return IK_OK;
}

int ik_flatten_span(void) { return kFlattenSpan; }
int ik_flatten_row_cap(void) { return kFlattenRowCap; }

int ik_flatten_counters(unsigned long long out[2]) {
    if (!out) return fail(IK_ERR_INVALID, "null pointer");
    out[0] = g_flatten_launches.load();
    out[1] = g_flatten_images.load();
    return IK_OK;
}

int ik_flatten_batch_device(const uint8_t* dev_src, uint32_t W, uint32_t H, uint32_t C, uint32_t depth, size_t src_pitch,
                            size_t src_image_stride, uint32_t n, int32_t rgb, uint32_t out_channels, uint8_t* dev_dst,
                            size_t dst_pitch, size_t dst_image_stride, void* hip_stream) {
    IK_API_ENTER();
    if (rgb < 0 || rgb > 0xFFFFFF) return fail(IK_ERR_INVALID, "background %d outside 0x000000..0xFFFFFF", (int)rgb);
    if (!dev_src || !dev_dst) return fail(IK_ERR_INVALID, "null device pointer");
    if ((C != 2 && C != 4) || depth < 1 || depth > 2 || !W || !H || !n) return fail(IK_ERR_INVALID, "bad geometry");
    // Rgba -> Rgb; LumaA -> Luma (a gray colour only) or Rgb
    if (out_channels != 3 && !(C == 2 && out_channels == 1 && flatten_out_channels(2, (uint32_t)rgb) == 1))
        return fail(IK_ERR_INVALID, "%u channels cannot be flattened to %u onto %06x", C, out_channels, (unsigned)rgb);
    if (src_pitch < (size_t)W * C * depth || dst_pitch < (size_t)W * out_channels * depth)
        return fail(IK_ERR_INVALID, "pitch too small");
    if (n > 1 && (src_image_stride < src_pitch * H || dst_image_stride < dst_pitch * H))
        return fail(IK_ERR_INVALID, "image stride too small");
    if (n > kFlattenMaxImages) return fail(IK_ERR_INVALID, "more than %u images", kFlattenMaxImages);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : thread_stream();
    const hipError_t e = launch_flatten(dev_src, src_pitch, src_image_stride, dev_dst, dst_pitch, dst_image_stride, W, H,
                                        (int)C, (int)out_channels, (int)depth, (uint32_t)rgb, (int)n, s);
    if (e != hipSuccess) return hip_fail(e, "flatten kernel launch");
    flatten_count(1, n);
    return IK_OK;
}

// the image composited onto a background colour: a new image on the device that holds img
// (an image without alpha, or IK_BG_NONE: a copy)
int ik_image_flatten(const ik_image* img, int32_t background, ik_image** out) {
    IK_API_ENTER();
    if (!img || !out) return fail(IK_ERR_INVALID, "null pointer");
    if (background != IK_BG_NONE && (background < 0 || background > 0xFFFFFF))
        return fail(IK_ERR_INVALID, "background %d is neither IK_BG_NONE nor 0x000000..0xFFFFFF", (int)background);
    const bool pass = background != IK_BG_NONE && (img->c == 2 || img->c == 4);
    const uint32_t oc = pass ? flatten_out_channels(img->c, (uint32_t)background) : img->c;
    DeviceGuard g(img->device);
    ik_image* o = nullptr;
    int rc = alloc_image(img->w, img->h, oc, &o, img->depth);
    if (rc) return rc;
    if (img->w && img->h) {
        hipStream_t s = thread_stream();
        rc = pass ? ik_flatten_batch_device(img->d, img->w, img->h, img->c, img->depth, img->pitch, 0, 1, background, oc,
                                            o->d, o->pitch, 0, s)
                  : ik_orient_batch_device(img->d, img->w, img->h, img->c, img->depth, img->pitch, 0, 1, 1, o->d,
                                           o->pitch, 0, s);
        if (rc == IK_OK) {
            const hipError_t e = hipStreamSynchronize(s);
            if (e != hipSuccess) rc = hip_fail(e, "background flatten");
        }
    }
    if (rc) { ik_image_free(o); return rc; }
    *out = o;
    return IK_OK;
}

int ik_encode(const ik_image* img, int fmt, int quality, uint8_t** out, size_t* out_len) {
    IK_API_ENTER();
    if (!img || !out || !out_len) return fail(IK_ERR_INVALID, "null pointer");
    std::vector<uint8_t> bytes;
    EncodePrep prep;
    int st = encode_image_front(img, fmt, quality, prep, bytes);
    if (!st) st = encode_host_back(prep, bytes);
    if (st) return st;
    *out = (uint8_t*)malloc(bytes.size() ? bytes.size() : 1);
    if (!*out) return fail(IK_ERR_NOMEM, "out of host memory");
    std::memcpy(*out, bytes.data(), bytes.size());
    *out_len = bytes.size();
    return IK_OK;
}

}  // extern "C"

namespace ik {

// decode_image: image::guess_format + load_from_memory_with_format; formats the
// reference build compiles in (Cargo.toml:20: jpeg, png, webp; avif = encoder only)
int decode_one(const uint8_t* bytes, size_t len, ik_image** out, int* fmt_out) {
    if (!out) return fail(IK_ERR_INVALID, "null pointer");
    if (!bytes && len) return fail(IK_ERR_INVALID, "null bytes");
    const Sniffed f = guess_format(bytes, len);
    if (f == Sniffed::Unknown) return fail(IK_ERR_TRANSFORM, "The image format could not be determined");
    uint32_t w = 0, h = 0, c = 0;
    // host-decoded pixels: a per-thread buffer (with the PNG decoder's own it
    // trades places, so neither is page-faulted in again per image); released
    // after images over 128 MiB
    thread_local std::vector<uint8_t> px;
    struct Trim {
        ~Trim() { if (px.capacity() > (128u << 20)) std::vector<uint8_t>().swap(px); }
    } trim;
    int st;
    ik_image* img = nullptr;
    switch (f) {
    case Sniffed::Png: {  // GPU inflate + unfilter when the stream allows, else the host decoder
        std::string msg;
        const uint8_t* const bp[1] = {bytes};
        st = decode_png_batch(bp, &len, 1, &img, &st, &msg);
        if (st) return fail(st, "%s", msg.c_str());
        break;
    }
    case Sniffed::Jpeg: st = decode_jpeg_device(bytes, len, &img); break;
    case Sniffed::WebP:  // lossy on the GPU when it covers the file, else libwebp on the host
        st = decode_webp_device(bytes, len, &img);
        if (st == kVp8dHost) {
            if (webp_decode_mode() == 2)
                return fail(IK_ERR_TRANSFORM, "IK_WEBP_DECODE=gpu: the GPU WebP decoder leaves this file to libwebp");
            webp_count_host_decode();
            st = decode_webp(bytes, len, w, h, c, px);
        }
        break;
    default:
        return fail(IK_ERR_TRANSFORM, "The image format %s is not supported", format_name(f));
    }
    if (st) return st;
    if (!img) {
        st = ik_image_from_host(px.data(), w, h, c, &img);
        if (st) return st;
    }
    *out = img;
    if (fmt_out) {
        *fmt_out = f == Sniffed::WebP ? IK_FORMAT_WEBP
                 : f == Sniffed::Jpeg ? IK_FORMAT_JPEG
                 : f == Sniffed::Avif ? IK_FORMAT_AVIF : -1;
    }
    return IK_OK;
}

std::string last_error_str() { return t_err; }

// decode_image over a batch on the calling thread's device; per-item status and
// message (the decoder's own, as TransformError(e.to_string()) carries it).  up:
// the batch's PNG streams' upload, already issued (png_upload_begin), or null
// sniff: null, or a host copy of each item's first bytes (sniff_len(i) of them) when
// bytes holds device addresses for the PNG items and the JPEG items taken in place
// (device-resident inputs: every other item is a host copy already)
static size_t sniff_len(const uint8_t* const* sniff, const uint8_t* const* bytes, const size_t* lens, uint32_t i) {
    return sniff && sniff[i] != bytes[i] ? std::min<size_t>(lens[i], 64) : lens[i];
}

int decode_batch_dev(const uint8_t* const* bytes, const size_t* lens, uint32_t n, ik_image** outs, int* fmts,
                     int* st, std::string* msg, int threads, PngUpload* up = nullptr,
                     const uint8_t* const* sniff = nullptr, const JpegUpload* jup = nullptr) {
    std::vector<const uint8_t*> jb, pb, ph;
    std::vector<size_t> jl, pl;
    std::vector<const uint8_t*> wb;
    std::vector<size_t> wl;
    std::vector<uint32_t> ji, pi, wi, other;
    for (uint32_t i = 0; i < n; ++i) {
        outs[i] = nullptr;
        st[i] = IK_OK;
        if (fmts) fmts[i] = -1;
        if (!bytes[i] && lens[i]) { st[i] = fail(IK_ERR_INVALID, "null bytes"); msg[i] = t_err; continue; }
        const Sniffed f = guess_format(sniff ? sniff[i] : bytes[i], sniff_len(sniff, bytes, lens, i));
        if (f == Sniffed::Jpeg) {
            jb.push_back(bytes[i]);
            jl.push_back(lens[i]);
            ji.push_back(i);
            if (fmts) fmts[i] = IK_FORMAT_JPEG;
        } else if (f == Sniffed::Png) {
            pb.push_back(bytes[i]);
            pl.push_back(lens[i]);
            ph.push_back(sniff ? sniff[i] : bytes[i]);
            pi.push_back(i);
        } else if (f == Sniffed::WebP) {
            wb.push_back(bytes[i]);
            wl.push_back(lens[i]);
            wi.push_back(i);
        } else {
            other.push_back(i);
        }
    }
    if (!pi.empty()) {  // every PNG of the batch through one set of GPU launches
        std::vector<ik_image*> po(pi.size(), nullptr);
        std::vector<int> ps(pi.size(), IK_OK);
        std::vector<std::string> pm(pi.size());
        if (up && up->n == (int)pi.size()) {
            png_decode_finish(*up, po.data(), ps.data(), pm.data());
        } else {
            PngUpload u;
            u.dev = sniff != nullptr;  // (device-resident inputs: the PNG items are device addresses)
            u.heads = ph.data();
            png_upload_begin(pb.data(), pl.data(), (int)pi.size(), u);
            png_decode_finish(u, po.data(), ps.data(), pm.data());
        }
        for (size_t k = 0; k < pi.size(); ++k) {
            outs[pi[k]] = po[k];
            st[pi[k]] = ps[k];
            msg[pi[k]] = pm[k];
        }
    }
    parallel_for((int)other.size(), threads, [&](int k) {  // unknown and unsupported formats: decode_image's verdicts
        const uint32_t i = other[k];
        st[i] = decode_one(bytes[i], lens[i], &outs[i], fmts ? &fmts[i] : nullptr);
        if (st[i]) msg[i] = t_err;
    });
    if (!wi.empty()) {  // the batch's lossy WebP frames through one set of launches, the rest by libwebp
        std::vector<ik_image*> wo(wi.size(), nullptr);
        std::vector<int> ws(wi.size(), IK_OK);
        std::vector<std::string> wm(wi.size());
        decode_webp_batch(wb.data(), wl.data(), (int)wi.size(), wo.data(), ws.data(), wm.data(), threads);
        for (size_t k = 0; k < wi.size(); ++k) {
            outs[wi[k]] = wo[k];
            st[wi[k]] = ws[k];
            msg[wi[k]] = wm[k];
            if (fmts && !ws[k]) fmts[wi[k]] = IK_FORMAT_WEBP;
        }
    }
    if (!ji.empty()) {
        std::vector<ik_image*> jo(ji.size(), nullptr);
        std::vector<int> js(ji.size(), IK_OK);
        std::vector<std::string> jm(ji.size());
        decode_jpeg_batch(jb.data(), jl.data(), (int)ji.size(), jo.data(), js.data(), jm.data(), jup);
        for (size_t k = 0; k < ji.size(); ++k) {
            outs[ji[k]] = jo[k];
            st[ji[k]] = js[k];
            msg[ji[k]] = jm[k];
        }
    }
    int first = IK_OK;
    for (uint32_t i = 0; i < n; ++i)
        if (st[i] && !first) first = st[i];
    return first;
}

}  // namespace ik (reopened for the ABI below)
extern "C" {

int ik_decode(const uint8_t* bytes, size_t len, ik_image** out, int* fmt_out) {
    IK_API_ENTER();
    if (!sched_multi()) return decode_one(bytes, len, out, fmt_out);
    // several devices: the least-loaded one decodes (the image stays there)
    const uint64_t cost = request_cost(bytes, len, -1, -1, IK_FORMAT_JPEG);
    const int ld = sched_acquire(cost);
    int st;
    {
        DeviceGuard g(sched_phys(ld));
        st = decode_one(bytes, len, out, fmt_out);
    }
    sched_release(ld, cost);
    return st;
}

int ik_decode_oriented(const uint8_t* bytes, size_t len, int orient, ik_image** out, int* fmt_out) {
    IK_API_ENTER();
    const int o = effective_orientation(bytes, len, orient);
    if (o < 0) return fail(IK_ERR_INVALID, "unknown orientation %d", orient);
    if (!out) return fail(IK_ERR_INVALID, "null pointer");
    ik_image* img = nullptr;
    int st = ik_decode(bytes, len, &img, fmt_out);
    if (st || !o) {
        if (!st) *out = img;
        return st;
    }
    st = ik_image_orient(img, o, out);
    ik_image_free(img);
    return st;
}

int ik_decode_batch(const uint8_t* const* bytes, const size_t* lens, uint32_t n, ik_image** outs, int* fmts,
                    int* status) {
    IK_API_ENTER();
    if (!bytes || !lens || !outs || !n) return fail(IK_ERR_INVALID, "bad batch");
    std::vector<int> st(n, IK_OK);
    std::vector<std::string> msg(n);
    int first;
    if (sched_multi()) {
        uint64_t cost = 0;
        for (uint32_t i = 0; i < n; ++i) cost += request_cost(bytes[i], lens[i], -1, -1, IK_FORMAT_JPEG);
        const int ld = sched_acquire(cost);
        {
            DeviceGuard g(sched_phys(ld));
            first = decode_batch_dev(bytes, lens, n, outs, fmts, st.data(), msg.data(), 0);
        }
        sched_release(ld, cost);
    } else {
        first = decode_batch_dev(bytes, lens, n, outs, fmts, st.data(), msg.data(), 0);
    }
    uint32_t fi = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (status) status[i] = st[i];
        if (st[i] && fi == 0 && first && st[fi] == IK_OK) fi = i;
    }
    if (first) {
        for (fi = 0; fi < n && !st[fi]; ++fi) {}
        return fail(first, "input %u: %s", fi, msg[fi].c_str());
    }
    return IK_OK;
}

int ik_set_resize_mode(int mode) {
    if (mode != IK_RESIZE_EXACT && mode != IK_RESIZE_FMA) return fail(IK_ERR_INVALID, "bad resize mode %d", mode);
    (void)resize_mode();
    g_resize_mode.store(mode);
    return IK_OK;
}

int ik_get_resize_mode(void) { return resize_mode(); }

}  // extern "C"

namespace ik {

// ---- batched transforms: a four-stage pipeline per device -------------------------
// ik_transform_batch(_submit) -- the handlers of src/lib.rs:175-191 serving many
// requests -- runs each batch through four stages, each on its own threads, so
// that consecutive batches overlap on one device:
//   upload   (one thread per device)  the PNG streams' upload: parse, DMA of the
//            files (in place when the caller pinned them), the GPU gather + CRC
//            pass, and the JPEG files' DMA, on the upload thread's copy stream
//            (png_upload_begin, jpeg_upload_begin)
//   decode   (one thread per device)  the PNG decode kernels once that upload has
//            landed, JPEG entropy decoding and reconstruction, host decoders for
//            the rest (transform_decode_phase)
//   post     (one thread per device)  one resize launch per geometry group, the
//            encoders' device front ends (transform_post_phase), on its own stream:
//            batch k's resize runs beside batch k+1's decode kernels
//   host     (the device's worker pool)  the host coders (libwebp / libavif) and
//            the output buffers (transform_host_phase)
// so batch k+1's PCIe upload runs under batch k's kernels, and batch k's libwebp
// beside both.  With several logical devices (ik_init(-1) / IK_DEVICES) each has
// its own stages; a batch goes whole to the least-loaded device, or is split into
// parts of at least IK_MIN_DEVICE_BATCH (64) requests over several devices -- the
// inflate kernels' time hardly depends on how many frames a launch holds, so
// small parts would only add launches.  (HostPhase, what a batch part carries from stage to
// stage: ik_runtime.h; the post stage: ik_post_stage.cpp.)

// the PNG requests among idx (decode_batch_dev takes the same ones, in the same order)
static void png_items(const uint8_t* const* bytes, const size_t* lens, const uint8_t* const* sniff,
                      const std::vector<uint32_t>& idx, std::vector<const uint8_t*>& pb, std::vector<size_t>& pl,
                      std::vector<const uint8_t*>& ph) {
    pb.clear();
    pl.clear();
    ph.clear();
    for (uint32_t i : idx)
        if ((bytes[i] || !lens[i]) &&
            guess_format(sniff ? sniff[i] : bytes[i], sniff_len(sniff, bytes, lens, i)) == Sniffed::Png) {
            pb.push_back(bytes[i]);
            pl.push_back(lens[i]);
            ph.push_back(sniff ? sniff[i] : bytes[i]);
        }
}

// the JPEG requests among idx, host inputs only (a device-resident batch's JPEG
// items are read where they lie or were copied to the host at submit: no upload)
static void jpeg_items(const uint8_t* const* bytes, const size_t* lens, const std::vector<uint32_t>& idx,
                       std::vector<const uint8_t*>& jb, std::vector<size_t>& jl) {
    jb.clear();
    jl.clear();
    for (uint32_t i : idx)
        if (bytes[i] && guess_format(bytes[i], lens[i]) == Sniffed::Jpeg) {
            jb.push_back(bytes[i]);
            jl.push_back(lens[i]);
        }
}

// Device half, decode stage: decode (GPU where the stream allows; the PNG upload
// already issued when up is given) under the device's kernel gate; the images,
// statuses and messages go to hp.imgs / ds / dm for the post stage
static void transform_decode_phase(const uint8_t* const* bytes, const size_t* lens, HostPhase& hp, PngUpload* up,
                                   const uint8_t* const* sniff = nullptr, const JpegUpload* jup = nullptr) {
    const std::vector<uint32_t>& idx = hp.idx;
    const uint32_t m = (uint32_t)idx.size();
    hp.imgs.assign(m, nullptr);
    hp.ds.assign(m, IK_OK);
    hp.dm.assign(m, std::string());
    if (!m) return;
    std::vector<const uint8_t*> b(m), sn(sniff ? m : 0);
    std::vector<size_t> l(m);
    for (uint32_t k = 0; k < m; ++k) {
        b[k] = bytes[idx[k]];
        l[k] = lens[idx[k]];
        if (sniff) sn[k] = sniff[idx[k]];
    }
    static const bool timing = getenv("IK_TIMING") != nullptr;  // dev: per-stage sums to stderr
    const auto tg0 = std::chrono::steady_clock::now();
    gate_pin(kGateKernels, true);
    const auto tg1 = std::chrono::steady_clock::now();
    batch_timing_reset(current_device(), false);
    BatchTimingScope bts;
    decode_batch_dev(b.data(), l.data(), m, hp.imgs.data(), nullptr, hp.ds.data(), hp.dm.data(), hp.threads, up,
                     sniff ? sn.data() : nullptr, jup);
    batch_timing_commit(current_device(), false);
    gate_pin(kGateKernels, false);
    if (timing)
        fprintf(stderr, "[device_phase] gate wait %.2f ms, decode %.2f ms\n",
                std::chrono::duration<double, std::milli>(tg1 - tg0).count(),
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tg1).count());
}

static void transform_host_phase(uint8_t** outs, size_t* out_lens, int* st, std::string* errs, HostPhase& hp) {
    static const bool timing = getenv("IK_TIMING") != nullptr;
    const std::vector<uint32_t>& idx = hp.idx;
    const uint32_t m = (uint32_t)idx.size();
    std::vector<EncodePrep>& prep = hp.prep;
    std::vector<std::vector<uint8_t>>& bytes_out = hp.bytes_out;
    std::mutex tmu;
    double t_back = 0;
    std::atomic<int64_t> cpu_ns{0};  // thread CPU time of the coders (core budget)
    std::atomic<int> coded{0};
    const auto tw0 = std::chrono::steady_clock::now();
    const double tg = timing ? std::chrono::duration<double, std::milli>(
                                   std::chrono::steady_clock::now().time_since_epoch()).count() : 0.0;
    auto thread_cpu_ns = [] {
        timespec ts{};
        clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
        return (int64_t)ts.tv_sec * 1000000000ll + ts.tv_nsec;
    };
    parallel_for((int)m, hp.threads, [&](int k) {
        const uint32_t i = idx[k];
        if (st[i]) return;
        const auto t0 = std::chrono::steady_clock::now();
        const int64_t c0 = thread_cpu_ns();
        if (!prep[k].done) coded.fetch_add(1);  // a host coder runs (libwebp / libavif)
        int r = encode_host_back(prep[k], bytes_out[k]);
        cpu_ns.fetch_add(thread_cpu_ns() - c0);
        std::vector<uint8_t>().swap(prep[k].planes);
        prep[k].pin_block.reset();  // (the batch's pinned plane block goes back to its pool with the last)
        prep[k].pin_planes = nullptr;
        if (!r) {
            outs[i] = (uint8_t*)malloc(bytes_out[k].size() ? bytes_out[k].size() : 1);
            if (!outs[i]) r = fail(IK_ERR_NOMEM, "out of host memory");
            else {
                std::memcpy(outs[i], bytes_out[k].data(), bytes_out[k].size());
                out_lens[i] = bytes_out[k].size();
            }
        }
        if (timing) {
            std::lock_guard<std::mutex> lk(tmu);
            t_back += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        }
        if (r) { errs[i] = last_error_str(); st[i] = r; }
    });
    batch_timing_host(current_device(),
                      std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count(),
                      (double)cpu_ns.load() * 1e-6, (double)coded.load());
    if (timing)
        fprintf(stderr, "[transform_batch] t=%.1f..%.1f %u requests on device %d: resize %.1f ms, encode front %.1f ms, "
                "host coders %.1f ms (summed)\n", fmod(tg, 1e5), fmod(std::chrono::duration<double, std::milli>(
                std::chrono::steady_clock::now().time_since_epoch()).count(), 1e5), m, current_device(), hp.t_resize,
                hp.t_front, t_back);
}

namespace {

// one submitted batch (a ticket): its parts run on one or more devices
struct Ticket {
    uint32_t n = 0;
    uint8_t** outs = nullptr;
    size_t* out_lens = nullptr;
    int* status = nullptr;
    std::vector<int> st;
    std::vector<std::string> errs;
    std::mutex mu;
    std::condition_variable cv;
    int pending = 0;
    // device-resident inputs (ik_transform_batch_submit_device): the request array
    // the stages read (PNG items and the JPEG items taken in place: the caller's
    // device addresses; others: host copies), the host copies, and each item's
    // sniff bytes
    std::vector<const uint8_t*> eff, sniff;
    std::vector<std::vector<uint8_t>> hcopy;
    std::vector<uint8_t> heads;
    // its baseline JPEG items decoded where they lie: what the marker walk brought
    // back (by device address), and the skeletons' bytes
    JpegInPlaceMap jin;
    std::vector<uint8_t> jskel;
    // each request's options, resolved at submit (request_ops; the watermarks' handles are the
    // caller's, alive until the wait returns); empty when every request is at its defaults
    std::vector<RequestOps> ops;
};

// one device's share of a ticket
struct BatchPart {
    std::shared_ptr<Ticket> t;
    const uint8_t* const* bytes = nullptr;
    const size_t* lens = nullptr;
    const int64_t* w = nullptr;
    const int64_t* h = nullptr;
    const RequestOps* ops = nullptr;  // null: every request at its defaults; else Ticket::ops
    const int* fmt = nullptr;
    const int* quality = nullptr;
    int filter = 0;
    HostPhase hp;
    std::vector<const uint8_t*> pb;  // its PNG inputs (the upload stage's batch)
    std::vector<size_t> pl;
    std::vector<const uint8_t*> ph;  // their first bytes in host memory
    const uint8_t* const* sniff = nullptr;  // device-resident inputs (Ticket::sniff), else null
    PngUpload up;
    std::vector<const uint8_t*> jb;  // its JPEG inputs in host memory
    std::vector<size_t> jl;
    JpegUpload jup;  // their device copies (the upload stage's JPEG DMA)
    int logical = -1;  // logical device (multi-device dispatch), -1 = none
    uint64_t cost = 0;
};

class StageExec {
public:
    StageExec(int device, Pool* host_pool) : dev_(device), pool_(host_pool) {
        for (int k = 0; k < kStages; ++k) th_[k] = std::thread([this, k] { loop(k); });  // live until stop()
    }
    // ik_shutdown: the stages finish what is queued (upload, then decode, then post), then end
    void stop() {
        for (int k = 0; k < kStages; ++k) {
            {
                std::lock_guard<std::mutex> lk(mu_);
                done_[k] = true;
            }
            cv_.notify_all();
            th_[k].join();
        }
    }
    void submit(std::shared_ptr<BatchPart> p) {
        {
            std::lock_guard<std::mutex> lk(mu_);
            q_[0].push_back(std::move(p));
        }
        cv_.notify_all();
    }

private:
    void loop(int stage) {
        mark_internal_thread();  // the library's own thread: no lifetime lock (ApiGuard)
        ik_init(dev_);  // this thread's streams, staging and scratch live on dev_
        for (;;) {
            std::shared_ptr<BatchPart> p;
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return done_[stage] || !q_[stage].empty(); });
                if (q_[stage].empty()) break;  // stopped, nothing left
                p = std::move(q_[stage].front());
                q_[stage].pop_front();
            }
            if (stage == 0) {
                png_items(p->bytes, p->lens, p->sniff, p->hp.idx, p->pb, p->pl, p->ph);
                p->up.dev = p->sniff != nullptr;
                p->up.heads = p->ph.data();
                if (!p->pb.empty()) png_upload_begin(p->pb.data(), p->pl.data(), (int)p->pb.size(), p->up);
                if (!p->sniff) {
                    jpeg_items(p->bytes, p->lens, p->hp.idx, p->jb, p->jl);
                    if (!p->jb.empty()) jpeg_upload_begin(p->jb.data(), p->jl.data(), (int)p->jb.size(), p->jup);
                } else if (!p->t->jin.empty()) {
                    p->jup.inplace = &p->t->jin;  // (no upload: the decoder reads the caller's memory)
                }
                {
                    std::lock_guard<std::mutex> lk(mu_);
                    q_[1].push_back(std::move(p));
                }
                cv_.notify_all();
                continue;
            }
            if (stage == 2) {
                // resize + the encoders' device front ends, beside the next batch's decode
                Ticket& t = *p->t;
                transform_post_phase(p->w, p->h, p->ops, p->fmt, p->quality, p->filter, t.st.data(), t.errs.data(), p->hp);
                pool_->post([p] {
                    Ticket& tk = *p->t;
                    transform_host_phase(tk.outs, tk.out_lens, tk.st.data(), tk.errs.data(), p->hp);
                    p->hp = HostPhase();
                    if (p->logical >= 0) sched_release(p->logical, p->cost);
                    std::lock_guard<std::mutex> lk(tk.mu);
                    if (--tk.pending == 0) tk.cv.notify_all();
                });
                continue;
            }
            // the next queued batch's block search goes out on this stream between
            // this batch's decode rounds and its expand
            p->up.on_next_search = [this](hipEvent_t after) {
                std::shared_ptr<BatchPart> nx;
                {
                    std::lock_guard<std::mutex> lk(mu_);
                    if (!q_[1].empty()) nx = q_[1].front();
                }
                if (!nx || nx->pb.empty()) return;
                // On the kernel stream itself, between this batch's decode rounds and its
                // expand (it covers the host planning there), once the next batch's
                // upload has landed (else its own kernel stage launches it).  Beside
                // expand / resolve / unfilter it only slows them: a stream on another
                // hardware queue measured 63-69 vs 61-62 ms per step (the search took
                // resolve from 3.6 to 13-19 ms; profiles/r03n_find_*.json).
                if (!png_upload_landed(nx->up)) return;
                hipStream_t fs = png_find_beside_decode() ? thread_copy_stream() : thread_stream();
                if (after && hipStreamWaitEvent(fs, after, 0) != hipSuccess) return;
                png_find_prelaunch(nx->up, fs);
            };
            transform_decode_phase(p->bytes, p->lens, p->hp, p->pb.empty() ? nullptr : &p->up, p->sniff, &p->jup);
            p->up = PngUpload();
            p->jup = JpegUpload();  // (the decode has returned: its area is free again)
            {
                std::lock_guard<std::mutex> lk(mu_);
                q_[2].push_back(std::move(p));
            }
            cv_.notify_all();
        }
        release_thread_resources();
    }
    int dev_;
    Pool* pool_;
    std::mutex mu_;
    std::condition_variable cv_;
    static constexpr int kStages = 3;  // upload, decode, post (resize + device front ends)
    std::deque<std::shared_ptr<BatchPart>> q_[kStages];
    bool done_[kStages] = {false, false, false};
    std::thread th_[kStages];
};

std::mutex g_stage_mu;
std::map<int, StageExec*> g_stages;

// the stages of a logical device, or (single-device mode) of physical device
// `phys` (-1: the calling thread's device)
StageExec& stage_exec(int logical, int phys) {
    const int dev = phys >= 0 ? phys : current_device();
    const int key = logical >= 0 ? 1000 + logical : dev;
    std::lock_guard<std::mutex> lk(g_stage_mu);
    StageExec*& e = g_stages[key];
    if (!e) e = logical >= 0 ? new StageExec(sched_phys(logical), &sched_pool(logical))
                             : new StageExec(dev, &device_pool(dev));
    return *e;
}

std::mutex g_async_mu;
std::map<uint64_t, std::shared_ptr<Ticket>> g_async;
uint64_t g_async_next = 1;

}  // namespace

// ik_shutdown's device-memory part: pooled image blocks, the batched colour
// launches' pinned blocks, the per-device constant tables
static void memory_shutdown() {
    {
        std::lock_guard<std::mutex> lk(g_ipool_mu);
        for (auto& kv : g_ipools) {
            std::lock_guard<std::mutex> lk2(kv.second->mu);
            (void)hipSetDevice(kv.first);
            for (auto& b : kv.second->free_blocks) {
                (void)hipFree(b.second);
                mem_stat(kMemImageFree, -(int64_t)b.first);
            }
            kv.second->free_blocks.clear();
            kv.second->held = 0;
        }
    }
    encode_shutdown();
}

// ik_shutdown: wait for every submitted batch, end the stage threads and the
// worker pools (each releases its streams and arenas), then free what the
// library holds, all while the HIP runtime is alive
int shutdown_all(bool close) {
    // exclusive: every caller still inside the library returns first (ApiGuard);
    // nested entry points called from here see depth > 0 and take nothing
    std::unique_lock<LifeLock> life(g_life);
    ++t_api_depth;
    if (close) g_closed.store(true, std::memory_order_release);
    std::vector<std::shared_ptr<Ticket>> ts;
    {
        std::lock_guard<std::mutex> lk(g_async_mu);
        for (auto& kv : g_async) ts.push_back(kv.second);
    }
    for (auto& t : ts) {
        std::unique_lock<std::mutex> lk(t->mu);
        t->cv.wait(lk, [&] { return t->pending == 0; });
    }
    std::vector<StageExec*> st;
    {
        std::lock_guard<std::mutex> lk(g_stage_mu);
        for (auto& kv : g_stages) st.push_back(kv.second);
        g_stages.clear();
    }
    for (StageExec* e : st) {
        e->stop();
        delete e;
    }
    pools_shutdown();
    const int dev = t_device;
    png_shutdown();
    jpeg_shutdown();
    plans_shutdown();
    blur_shutdown();
    adjust_shutdown();
    memory_shutdown();
    release_thread_resources();
    if (dev >= 0) (void)hipSetDevice(dev);
    --t_api_depth;
    return IK_OK;
}

namespace {

int min_device_batch() {
    static const int v = [] {
        const char* e = getenv("IK_MIN_DEVICE_BATCH");
        const int x = e && *e ? atoi(e) : 64;
        return x < 1 ? 1 : x;
    }();
    return v;
}

// the parts of a ticket to the stage executors.  bytes / sniff: the request array
// the stages read (Ticket::eff / sniff for device-resident inputs); phys >= 0:
// the inputs live on that physical device, so the batch goes whole to it
int submit_parts(const std::shared_ptr<Ticket>& t, const uint8_t* const* bytes, const uint8_t* const* sniff,
                 int phys, const size_t* lens, uint32_t n, const int64_t* w, const int64_t* h, const int* fmt,
                 const int* quality, int filter, int threads, uint64_t* ticket) {
    auto make_part = [&](uint32_t lo, uint32_t hi) {
        auto p = std::make_shared<BatchPart>();
        p->t = t;
        p->bytes = bytes; p->lens = lens; p->w = w; p->h = h; p->fmt = fmt; p->quality = quality;
        p->ops = t->ops.empty() ? nullptr : t->ops.data();
        p->sniff = sniff;
        p->filter = filter;
        p->hp.threads = threads;
        for (uint32_t i = lo; i < hi; ++i) p->hp.idx.push_back(i);
        return p;
    };
    auto cost_of = [&](uint32_t i) {
        return request_cost(sniff ? sniff[i] : bytes[i], sniff_len(sniff, bytes, lens, i), w[i], h[i], fmt[i]);
    };
    std::vector<std::shared_ptr<BatchPart>> parts;
    if (!sched_multi()) {
        parts.push_back(make_part(0, n));  // to the stages of `phys` (the inputs' device) or the caller's device
    } else if (phys >= 0) {
        auto p = make_part(0, n);
        for (uint32_t i = 0; i < n; ++i) p->cost += cost_of(i);
        p->logical = sched_acquire_on(phys, p->cost);
        if (p->logical < 0) return fail(IK_ERR_INVALID, "the inputs are on device %d, which serves no logical device", phys);
        parts.push_back(p);
    } else {
        // whole parts of >= IK_MIN_DEVICE_BATCH requests (sched_split's bounds), each to the
        // least-loaded device by the live counters
        const uint32_t nd = (uint32_t)sched_count();
        std::vector<uint64_t> costs(n), out(nd, 0);
        for (uint32_t i = 0; i < n; ++i) costs[i] = cost_of(i);
        std::vector<uint32_t> lo(nd + 1), dev(nd);
        const uint32_t P = sched_split(costs.data(), n, nd, (uint32_t)min_device_batch(), out.data(), lo.data(), dev.data());
        for (uint32_t q = 0; q < P; ++q) {
            auto p = make_part(lo[q], lo[q + 1]);
            for (uint32_t i : p->hp.idx) p->cost += costs[i];
            p->logical = sched_acquire(p->cost);
            parts.push_back(p);
        }
    }
    t->pending = (int)parts.size();
    {
        std::lock_guard<std::mutex> lk(g_async_mu);
        *ticket = g_async_next++;
        g_async[*ticket] = t;
    }
    for (auto& p : parts) {
        const int ld = p->logical;
        stage_exec(ld, ld >= 0 ? -1 : phys).submit(std::move(p));
    }
    return IK_OK;
}

std::shared_ptr<Ticket> new_ticket(uint32_t n, uint8_t** outs, size_t* out_lens, int* status) {
    auto t = std::make_shared<Ticket>();
    t->n = n;
    t->outs = outs;
    t->out_lens = out_lens;
    t->status = status;
    t->st.assign(n, IK_OK);
    t->errs.assign(n, std::string());
    for (uint32_t i = 0; i < n; ++i) { outs[i] = nullptr; out_lens[i] = 0; }
    return t;
}

// device-resident inputs: every one must be device memory of one device (the batch runs there)
int inputs_device(const uint8_t* const* dev_bytes, const size_t* lens, uint32_t n, int* phys_out) {
    int phys = -1;
    for (uint32_t i = 0; i < n; ++i) {
        if (!lens[i]) continue;
        if (!dev_bytes[i]) return fail(IK_ERR_INVALID, "input %u: null bytes", i);
        hipPointerAttribute_t at{};
        if (hipPointerGetAttributes(&at, dev_bytes[i]) != hipSuccess || at.type != hipMemoryTypeDevice) {
            (void)hipGetLastError();
            return fail(IK_ERR_INVALID, "input %u is not device memory", i);
        }
        if (phys < 0) phys = at.device;
        else if (phys != at.device) return fail(IK_ERR_INVALID, "inputs on devices %d and %d", phys, at.device);
    }
    *phys_out = phys < 0 ? current_device() : phys;
    return IK_OK;
}

// device-resident inputs on device phys: what the stages read of them into the ticket
// (Ticket::eff, sniff, hcopy, heads, jin, jskel)
int stage_device_inputs(Ticket* t, const uint8_t* const* dev_bytes, const size_t* lens, uint32_t n, int phys) {
    t->eff.assign(dev_bytes, dev_bytes + n);
    t->sniff.assign(n, nullptr);
    t->hcopy.resize(n);
    t->heads.assign(64 * (size_t)n, 0);
    DeviceGuard g(phys);
    // the first 64 bytes of every file, through pinned memory (the block also
    // holds the JPEG marker walk's table, records and skeleton slots, below)
    const size_t o_files = (64 * (size_t)n + 255) & ~size_t(255);
    const size_t o_jrecs = o_files + 2 * sizeof(uint64_t) * n;
    const size_t o_jskel = (o_jrecs + sizeof(jwalk::Rec) * n + 255) & ~size_t(255);
    uint8_t* pin = pinned_slot(kPinnedDeviceHeads, o_jskel + (size_t)jwalk::kSlot * n);
    void* dp = nullptr;
    if (!pin || hipHostGetDevicePointer(&dp, pin, 0) != hipSuccess || !dp)
        return fail(IK_ERR_NOMEM, "cannot allocate pinned memory for the input headers");
    uint64_t* files = reinterpret_cast<uint64_t*>(pin + o_files);
    for (uint32_t i = 0; i < n; ++i) {
        files[i] = (uint64_t)(uintptr_t)dev_bytes[i];
        files[n + i] = dev_bytes[i] ? lens[i] : 0;
    }
    hipStream_t s = thread_stream();
    const uint64_t* df = reinterpret_cast<const uint64_t*>(reinterpret_cast<uint8_t*>(dp) + o_files);
    IK_HIP(launch_copy_heads(df, df + n, (int)n, reinterpret_cast<uint8_t*>(dp), s));
    IK_HIP(hipStreamSynchronize(s));
    std::memcpy(t->heads.data(), pin, 64 * (size_t)n);
    // The JPEG files: a marker walk on the GPU brings back each one's skeleton
    // (table and frame segments), two offsets and a verdict; those it passes stay
    // where they are, the decoder reads their scans from the caller's memory.
    std::vector<uint32_t> ji;
    for (uint32_t i = 0; i < n; ++i)
        if (dev_bytes[i] && guess_format(t->heads.data() + 64 * (size_t)i, std::min<size_t>(lens[i], 64)) == Sniffed::Jpeg)
            ji.push_back(i);
    const size_t nj = ji.size();
    std::vector<char> in_place(n, 0);
    if (nj && jpeg_device_inplace()) {
        for (size_t k = 0; k < nj; ++k) {  // (the kernel above has finished with the table)
            files[k] = (uint64_t)(uintptr_t)dev_bytes[ji[k]];
            files[nj + k] = lens[ji[k]];
        }
        uint8_t* dpin = reinterpret_cast<uint8_t*>(dp);
        EvPair& ev = thread_events(kEvJpegWalk);
        ev_record(ev.a, s);
        IK_HIP(launch_jpeg_walk(df, df + nj, (int)nj, dpin + o_jskel, dpin + o_jrecs, s));
        ev_record(ev.b, s);
        IK_HIP(hipStreamSynchronize(s));
        jpeg_device_walk_ms(ev_pair_ms(ev));
        const jwalk::Rec* recs = reinterpret_cast<const jwalk::Rec*>(pin + o_jrecs);
        size_t total = 0;
        for (size_t k = 0; k < nj; ++k)
            if (recs[k].verdict == jwalk::kInPlace) total += recs[k].skel_len;
        t->jskel.resize(total);
        size_t o = 0;
        for (size_t k = 0; k < nj; ++k) {
            const jwalk::Rec& r = recs[k];
            const uint32_t i = ji[k];
            if (r.verdict != jwalk::kInPlace) continue;
            auto it = t->jin.find(dev_bytes[i]);
            if (it != t->jin.end()) {  // the same address twice: one record serves both (another length: copied back)
                in_place[i] = it->second.len == lens[i];
                continue;
            }
            JpegInPlace& J = t->jin[dev_bytes[i]];
            std::memcpy(t->jskel.data() + o, pin + o_jskel + (size_t)jwalk::kSlot * k, r.skel_len);
            J.skel = t->jskel.data() + o;
            J.skel_len = r.skel_len;
            J.len = lens[i];
            J.ent_off = r.ent_off;
            J.eoi_off = r.eoi_off;
            o += r.skel_len;
            in_place[i] = 1;
        }
    }
    size_t n_in = 0;
    for (uint32_t i : ji) n_in += in_place[i] ? 1 : 0;
    jpeg_device_count(0, n_in);
    jpeg_device_count(1, nj - n_in);
    // PNG files stay where they are (the upload stage walks and gathers them on
    // the GPU), and so do the JPEG files taken in place; any other item comes
    // back to host memory for its host-side parse
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t* hd = t->heads.data() + 64 * (size_t)i;
        if (!dev_bytes[i] || in_place[i] || guess_format(hd, std::min<size_t>(lens[i], 64)) == Sniffed::Png) {
            t->sniff[i] = dev_bytes[i] ? hd : nullptr;
            continue;
        }
        t->hcopy[i].resize(lens[i]);
        IK_HIP(hipMemcpy(t->hcopy[i].data(), dev_bytes[i], lens[i], hipMemcpyDeviceToHost));
        t->eff[i] = t->sniff[i] = t->hcopy[i].data();
    }
    return IK_OK;
}

// Every batch submit ends here with its requests' options as records (empty: all at their
// defaults).  device: bytes are device addresses; the batch runs where they are, on a logical
// device of that physical device or (single-device mode) on its stages whatever the calling
// thread's device is.
int submit_records(const uint8_t* const* bytes, const size_t* lens, uint32_t n, const int64_t* w, const int64_t* h,
                   std::vector<RequestOps>&& ops, const int* fmt, const int* quality, int filter, int threads,
                   uint8_t** outs, size_t* out_lens, int* status, uint64_t* ticket, bool device) {
    int phys = -1;
    if (device)
        if (int rc = inputs_device(bytes, lens, n, &phys)) return rc;
    auto t = new_ticket(n, outs, out_lens, status);
    t->ops = std::move(ops);
    if (!device) return submit_parts(t, bytes, nullptr, -1, lens, n, w, h, fmt, quality, filter, threads, ticket);
    if (int rc = stage_device_inputs(t.get(), bytes, lens, n, phys)) return rc;
    return submit_parts(t, t->eff.data(), t->sniff.data(), phys, lens, n, w, h, fmt, quality, filter, threads, ticket);
}

// ... and begins here: an entry point's arguments checked in the order the entry points have
// always checked them (the options' size, the arrays, then request by request: request_ops),
// all before a ticket exists or anything is queued.  fit / orient: the *_fit and *_oriented
// calls' arrays; opts, opt_size: the *_opts calls' (the others pass null and any declared size)
int submit_batch(const uint8_t* const* bytes, const size_t* lens, uint32_t n, const int64_t* w, const int64_t* h,
                 const int* fit, const int* orient, const void* opts, size_t opt_size, const int* fmt,
                 const int* quality, int filter, int threads, uint8_t** outs, size_t* out_lens, int* status,
                 uint64_t* ticket, bool device) {
    if (!opts_size_ok(opt_size)) return fail(IK_ERR_INVALID, "unknown options size %zu", opt_size);
    if (!bytes || !lens || !w || !h || !fmt || !quality || !outs || !out_lens || !n || !ticket)
        return fail(IK_ERR_INVALID, "bad batch");
    std::vector<RequestOps> ops;
    // (IK_ORIENT_AUTO is resolved here, on the host: a header walk of a few hundred bytes per file)
    if (int rc = request_ops(fit, orient, opts, opt_size, n, device ? nullptr : bytes, lens, ops)) return rc;
    return submit_records(bytes, lens, n, w, h, std::move(ops), fmt, quality, filter, threads, outs, out_lens, status,
                          ticket, device);
}

}  // namespace
}  // namespace ik

extern "C" {

int ik_transform_batch_submit(const uint8_t* const* bytes, const size_t* lens, uint32_t n, const int64_t* w,
                              const int64_t* h, const int* fmt, const int* quality, int filter, int threads,
                              uint8_t** outs, size_t* out_lens, int* status, uint64_t* ticket) {
    IK_API_ENTER();
    return submit_batch(bytes, lens, n, w, h, nullptr, nullptr, nullptr, sizeof(ik_request_opts), fmt, quality, filter,
                        threads, outs, out_lens, status, ticket, false);
}

int ik_transform_batch_submit_fit(const uint8_t* const* bytes, const size_t* lens, uint32_t n, const int64_t* w,
                                  const int64_t* h, const int* fit, const int* fmt, const int* quality, int filter,
                                  int threads, uint8_t** outs, size_t* out_lens, int* status, uint64_t* ticket) {
    IK_API_ENTER();
    return submit_batch(bytes, lens, n, w, h, fit, nullptr, nullptr, sizeof(ik_request_opts), fmt, quality, filter,
                        threads, outs, out_lens, status, ticket, false);
}

int ik_transform_batch_submit_oriented(const uint8_t* const* bytes, const size_t* lens, uint32_t n, const int64_t* w,
                                       const int64_t* h, const int* fit, const int* orient, const int* fmt,
                                       const int* quality, int filter, int threads, uint8_t** outs, size_t* out_lens,
                                       int* status, uint64_t* ticket) {
    IK_API_ENTER();
    return submit_batch(bytes, lens, n, w, h, fit, orient, nullptr, sizeof(ik_request_opts), fmt, quality, filter,
                        threads, outs, out_lens, status, ticket, false);
}

int ik_transform_batch_submit_opts(const uint8_t* const* bytes, const size_t* lens, uint32_t n, const int64_t* w,
                                   const int64_t* h, const void* opts, size_t opt_size, const int* fmt,
                                   const int* quality, int filter, int threads, uint8_t** outs, size_t* out_lens,
                                   int* status, uint64_t* ticket) {
    IK_API_ENTER();
    return submit_batch(bytes, lens, n, w, h, nullptr, nullptr, opts, opt_size, fmt, quality, filter, threads, outs,
                        out_lens, status, ticket, false);
}

int ik_transform_batch_opts(const uint8_t* const* bytes, const size_t* lens, uint32_t n, const int64_t* w,
                            const int64_t* h, const void* opts, size_t opt_size, const int* fmt,
                            const int* quality, int filter, int threads, uint8_t** outs, size_t* out_lens, int* status) {
    IK_API_ENTER();
    uint64_t ticket = 0;
    if (int rc = ik_transform_batch_submit_opts(bytes, lens, n, w, h, opts, opt_size, fmt, quality, filter, threads, outs,
                                                out_lens, status, &ticket))
        return rc;
    return ik_transform_batch_wait(ticket);
}

int ik_transform_batch_submit_device(const uint8_t* const* dev_bytes, const size_t* lens, uint32_t n,
                                     const int64_t* w, const int64_t* h, const int* fmt, const int* quality,
                                     int filter, int threads, uint8_t** outs, size_t* out_lens, int* status,
                                     uint64_t* ticket) {
    IK_API_ENTER();
    return submit_batch(dev_bytes, lens, n, w, h, nullptr, nullptr, nullptr, sizeof(ik_request_opts), fmt, quality,
                        filter, threads, outs, out_lens, status, ticket, true);
}

int ik_transform_batch_submit_device_opts(const uint8_t* const* dev_bytes, const size_t* lens, uint32_t n,
                                          const int64_t* w, const int64_t* h, const void* opts,
                                          size_t opt_size, const int* fmt, const int* quality, int filter, int threads,
                                          uint8_t** outs, size_t* out_lens, int* status, uint64_t* ticket) {
    IK_API_ENTER();
    return submit_batch(dev_bytes, lens, n, w, h, nullptr, nullptr, opts, opt_size, fmt, quality, filter, threads, outs,
                        out_lens, status, ticket, true);
}

int ik_memory_stats(uint64_t* out, int n) {
    if (!out || n <= 0) return fail(IK_ERR_INVALID, "bad stats buffer");
    for (int i = 0; i < n; ++i) out[i] = i < kMemStats ? (uint64_t)std::max<int64_t>(0, g_mem[i].load()) : 0;
    return IK_OK;
}

int ik_shutdown(void) { return shutdown_all(false); }
int ik_close(void) { return shutdown_all(true); }

int ik_batch_last_timing(double* out, int n) {
    if (!out || n <= 0) return fail(IK_ERR_INVALID, "bad timing buffer");
    const int d = current_device();
    std::lock_guard<std::mutex> lk(g_bt_mu);
    auto it = g_bt_last.find(d);
    for (int i = 0; i < n; ++i) out[i] = it != g_bt_last.end() && i < (int)it->second.size() ? it->second[(size_t)i] : 0.0;
    return IK_OK;
}

int ik_transform_batch_wait(uint64_t ticket) {
    IK_API_ENTER();
    std::shared_ptr<Ticket> t;
    {
        std::lock_guard<std::mutex> lk(g_async_mu);
        auto it = g_async.find(ticket);
        if (it == g_async.end()) return fail(IK_ERR_INVALID, "unknown batch ticket %llu", (unsigned long long)ticket);
        t = it->second;
        g_async.erase(it);
    }
    {
        std::unique_lock<std::mutex> lk(t->mu);
        t->cv.wait(lk, [&] { return t->pending == 0; });
    }
    int first = IK_OK;
    uint32_t first_i = 0;
    for (uint32_t i = 0; i < t->n; ++i) {
        if (t->status) t->status[i] = t->st[i];
        if (t->st[i] && !first) { first = t->st[i]; first_i = i; }
    }
    if (first) return fail(first, "item %u: %s", first_i, t->errs[first_i].c_str());
    return IK_OK;
}

int ik_transform_batch(const uint8_t* const* bytes, const size_t* lens, uint32_t n, const int64_t* w,
                       const int64_t* h, const int* fmt, const int* quality, int filter, int threads, uint8_t** outs,
                       size_t* out_lens, int* status) {
    IK_API_ENTER();
    return ik_transform_batch_fit(bytes, lens, n, w, h, nullptr, fmt, quality, filter, threads, outs, out_lens, status);
}

int ik_transform_batch_fit(const uint8_t* const* bytes, const size_t* lens, uint32_t n, const int64_t* w,
                           const int64_t* h, const int* fit, const int* fmt, const int* quality, int filter,
                           int threads, uint8_t** outs, size_t* out_lens, int* status) {
    IK_API_ENTER();
    uint64_t ticket = 0;
    if (int rc = ik_transform_batch_submit_fit(bytes, lens, n, w, h, fit, fmt, quality, filter, threads, outs, out_lens,
                                               status, &ticket))
        return rc;
    return ik_transform_batch_wait(ticket);
}

int ik_transform_batch_oriented(const uint8_t* const* bytes, const size_t* lens, uint32_t n, const int64_t* w,
                                const int64_t* h, const int* fit, const int* orient, const int* fmt,
                                const int* quality, int filter, int threads, uint8_t** outs, size_t* out_lens,
                                int* status) {
    IK_API_ENTER();
    uint64_t ticket = 0;
    if (int rc = ik_transform_batch_submit_oriented(bytes, lens, n, w, h, fit, orient, fmt, quality, filter, threads,
                                                    outs, out_lens, status, &ticket))
        return rc;
    return ik_transform_batch_wait(ticket);
}

// one request on this device, or (several devices) on the least-loaded one's workers
static int transform_scheduled(const uint8_t* bytes, size_t len, int64_t w, int64_t h, const RequestOps& ops, int fmt,
                               int quality, int filter, uint8_t** out, size_t* out_len) {
    if (!sched_multi()) return transform_here(bytes, len, w, h, ops, fmt, quality, filter, out, out_len);
    // several devices: queue the request to the least-loaded device's workers
    const uint64_t cost = request_cost(bytes, len, w, h, fmt);
    const int ld = sched_acquire(cost);
    std::mutex mu;
    std::condition_variable cv;
    bool done = false;
    int st = IK_OK;
    std::string msg;
    sched_pool(ld).post([&] {
        const int r = transform_here(bytes, len, w, h, ops, fmt, quality, filter, out, out_len);
        std::string m = r ? last_error_str() : std::string();
        std::lock_guard<std::mutex> lk(mu);
        st = r;
        msg.swap(m);
        done = true;
        cv.notify_all();
    });
    {
        std::unique_lock<std::mutex> lk(mu);
        cv.wait(lk, [&] { return done; });
    }
    sched_release(ld, cost);
    if (st) return fail(st, "%s", msg.c_str());
    return IK_OK;
}

// the single-request calls: fit and orient, or opts when it is not null, as one record
static int transform_single(const uint8_t* bytes, size_t len, int64_t w, int64_t h, int fit, int orient, const void* opts,
                            size_t opt_size, int fmt, int quality, int filter, uint8_t** out, size_t* out_len) {
    if (!opts_size_ok(opt_size)) return fail(IK_ERR_INVALID, "unknown options size %zu", opt_size);
    RequestOps ops;
    if (int rc = single_request_ops(fit, orient, opts, opt_size, bytes, len, ops)) return rc;
    return transform_scheduled(bytes, len, w, h, ops, fmt, quality, filter, out, out_len);
}

int ik_transform(const uint8_t* bytes, size_t len, int64_t w, int64_t h, int fmt, int quality,
                 int filter, uint8_t** out, size_t* out_len) {
    IK_API_ENTER();
    return ik_transform_fit(bytes, len, w, h, IK_FIT_CONTAIN, fmt, quality, filter, out, out_len);
}

int ik_transform_fit(const uint8_t* bytes, size_t len, int64_t w, int64_t h, int fit, int fmt, int quality,
                     int filter, uint8_t** out, size_t* out_len) {
    IK_API_ENTER();
    return ik_transform_oriented(bytes, len, w, h, fit, IK_ORIENT_STORED, fmt, quality, filter, out, out_len);
}

int ik_transform_oriented(const uint8_t* bytes, size_t len, int64_t w, int64_t h, int fit, int orient, int fmt,
                          int quality, int filter, uint8_t** out, size_t* out_len) {
    IK_API_ENTER();
    return transform_single(bytes, len, w, h, fit, orient, nullptr, sizeof(ik_request_opts), fmt, quality, filter, out,
                            out_len);
}

int ik_transform_opts(const uint8_t* bytes, size_t len, int64_t w, int64_t h, int fmt, int quality, int filter,
                      const void* opts, size_t opt_size, uint8_t** out, size_t* out_len) {
    IK_API_ENTER();
    return transform_single(bytes, len, w, h, IK_FIT_CONTAIN, IK_ORIENT_STORED, opts, opt_size, fmt, quality, filter, out,
                            out_len);
}

int ik_resize_batch_device(const uint8_t* dev_src, uint32_t W, uint32_t H, uint32_t C,
                           size_t src_pitch, size_t src_image_stride, uint32_t n, uint32_t nw,
                           uint32_t nh, int filter, uint8_t* dev_dst, size_t dst_pitch,
                           size_t dst_image_stride, void* hip_stream) {
    IK_API_ENTER();
    return ik_resize_window_batch_device(dev_src, W, H, C, src_pitch, src_image_stride, n, nw, nh, 0, 0, nw, nh, filter,
                                         dev_dst, dst_pitch, dst_image_stride, hip_stream);
}

int ik_resize_window_batch_device(const uint8_t* dev_src, uint32_t W, uint32_t H, uint32_t C, size_t src_pitch,
                                  size_t src_image_stride, uint32_t n, uint32_t iw, uint32_t ih, uint32_t x0,
                                  uint32_t y0, uint32_t nw, uint32_t nh, int filter, uint8_t* dev_dst,
                                  size_t dst_pitch, size_t dst_image_stride, void* hip_stream) {
    IK_API_ENTER();
    if (!dev_src || !dev_dst) return fail(IK_ERR_INVALID, "null device pointer");
    if (C < 1 || C > 4 || !W || !H || !nw || !nh || !n) return fail(IK_ERR_INVALID, "bad geometry");
    if (!resize_window_ok(iw, ih, x0, y0, nw, nh))
        return fail(IK_ERR_INVALID, "window %ux%u at (%u, %u) outside %ux%u", nw, nh, x0, y0, iw, ih);
    if (filter < 0 || filter > 4) return fail(IK_ERR_INVALID, "unknown filter %d", filter);
    if (src_pitch < (size_t)W * C || dst_pitch < (size_t)nw * C) return fail(IK_ERR_INVALID, "pitch too small");
    if ((src_pitch & 7) || ((uintptr_t)dev_src & 7)) return fail(IK_ERR_INVALID, "source rows must be 8-byte aligned");
    if (C == 4 && (((uintptr_t)dev_dst & 3) || (dst_pitch & 3) || (dst_image_stride & 3)))
        return fail(IK_ERR_INVALID, "RGBA destination rows must be 4-byte aligned");
    if (n > 1 && (src_image_stride < src_pitch * H || dst_image_stride < dst_pitch * nh))
        return fail(IK_ERR_INVALID, "image stride too small");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : thread_stream();
    ResizePlan* plan = get_resize_plan_window(current_device(), (int)W, (int)H, (int)C, (int)iw, (int)ih, (int)x0,
                                              (int)y0, (int)nw, (int)nh, filter, (int)n);
    if (!plan) return fail(IK_ERR_DEVICE, "cannot build resize plan");
    float* tmp = nullptr;
    if (plan->slots == 0 || !resize_fused_fits(src_pitch, H)) {
        tmp = (float*)scratch(sizeof(float) * (size_t)n * nh * plan->args.tmp_span);
        if (!tmp) return fail(IK_ERR_DEVICE, "cannot allocate device scratch");
    }
    hipError_t e = launch_resize(*plan, dev_src, src_pitch, src_image_stride, dev_dst, dst_pitch,
                                 dst_image_stride, (int)n, tmp, s);
    if (e != hipSuccess) return hip_fail(e, "resize kernel launch");
    return IK_OK;
}

const char* ik_resize_kernel_name(uint32_t W, uint32_t H, uint32_t C, uint32_t nw, uint32_t nh, int filter) {
    if (C < 1 || C > 4 || !W || !H || !nw || !nh || filter < 0 || filter > 4) return nullptr;
    ResizePlan* plan = get_resize_plan(current_device(), (int)W, (int)H, (int)C, (int)nw, (int)nh, filter, 1);
    return plan ? resize_kernel_name(*plan, (size_t)W * C) : nullptr;
}

int ik_resize_plan_info(uint32_t W, uint32_t H, uint32_t C, uint32_t nw, uint32_t nh, int filter, uint32_t n,
                        int32_t* out, int cap) {
    return ik_resize_plan_info_window(W, H, C, nw, nh, 0, 0, nw, nh, filter, n, out, cap);
}

int ik_resize_plan_info_window(uint32_t W, uint32_t H, uint32_t C, uint32_t iw, uint32_t ih, uint32_t x0, uint32_t y0,
                               uint32_t nw, uint32_t nh, int filter, uint32_t n, int32_t* out, int cap) {
    if (C < 1 || C > 4 || !W || !H || !nw || !nh || !n || filter < 0 || filter > 4 || !out || cap < 0) return -1;
    if (!resize_window_ok(iw, ih, x0, y0, nw, nh)) return -1;
    ResizeTables t;
    build_resize_tables_window((int)W, (int)H, (int)C, (int)iw, (int)ih, (int)x0, (int)y0, (int)nw, (int)nh, filter,
                               (int)n, t);
    const int32_t v[IK_RESIZE_PLAN_INFO_LEN] = {
        t.slots, t.rows, t.flush, t.weights_in_lds ? 1 : 0, t.NS, t.NB, t.per_A, t.per_R, t.NBp, t.Tx, t.Ty,
        t.max_strip_cols, resize_family_of(t, (size_t)W * C)};
    for (int i = 0; i < IK_RESIZE_PLAN_INFO_LEN && i < cap; ++i) out[i] = v[i];
    return IK_RESIZE_PLAN_INFO_LEN;
}

int ik_webp_yuv420_device(const uint8_t* dev_src, uint32_t w, uint32_t h, uint32_t C, size_t pitch,
                          uint8_t* dev_yuv, void* hip_stream) {
    IK_API_ENTER();
    if (!dev_src || !dev_yuv || !w || !h || C < 1 || C > 4) return fail(IK_ERR_INVALID, "bad arguments");
    const DeviceConsts* dc = device_consts(current_device());
    if (!dc) return fail(IK_ERR_DEVICE, "cannot upload WebP tables");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : thread_stream();
    IK_HIP(launch_webp_yuv420(dev_src, (int)w, (int)h, (int)C, pitch, 0, dev_yuv, 0, 1,
                              dc->gamma_to_lin, dc->lin_to_gamma, s));
    return IK_OK;
}

int ik_avif_yuv444_device(const uint8_t* dev_src, uint32_t w, uint32_t h, uint32_t C, size_t pitch,
                          size_t img_stride, uint32_t n, uint8_t* dev_planes, size_t plane_img_stride,
                          int* dev_transparent, void* hip_stream) {
    IK_API_ENTER();
    if (!dev_src || !dev_planes || !dev_transparent) return fail(IK_ERR_INVALID, "null device pointer");
    if (!w || !h || C < 1 || C > 4 || !n || w > INT32_MAX || h > 65535 || n > 65535)
        return fail(IK_ERR_INVALID, "bad geometry");
    if (pitch < (size_t)w * C) return fail(IK_ERR_INVALID, "pitch too small");
    if (n > 1 && (img_stride < pitch * h || plane_img_stride < 4 * (size_t)w * h))
        return fail(IK_ERR_INVALID, "image stride too small");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : thread_stream();
    IK_HIP(launch_avif_yuv444(dev_src, (int)w, (int)h, (int)C, pitch, img_stride, dev_planes, plane_img_stride,
                              dev_transparent, (int)n, s));
    return IK_OK;
}

int ik_jpeg_coeffs_device(const uint8_t* dev_src, uint32_t w, uint32_t h, uint32_t C, size_t pitch,
                          int quality, int16_t* dev_coef, void* hip_stream) {
    IK_API_ENTER();
    if (!dev_src || !dev_coef || !w || !h || C < 1 || C > 4) return fail(IK_ERR_INVALID, "bad arguments");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : thread_stream();
    uint8_t qt[128];
    jpeg_quant_tables(clamp_quality(quality), qt);
    uint8_t* dq = scratch(128);
    if (!dq) return fail(IK_ERR_DEVICE, "cannot allocate device scratch");
    if (int rc = copy_h2d_2d(dq, 128, qt, 128, 128, 1, s)) return rc;
    IK_HIP(launch_jpeg_coeffs(dev_src, (int)w, (int)h, (int)C, pitch, 0, dq, dev_coef, 0, 1, s));
    IK_HIP(hipStreamSynchronize(s));
    return IK_OK;
}

size_t ik_jpeg_enc_capacity(uint32_t w, uint32_t h) { return jpeg_enc_cap((int)w, (int)h); }

int ik_jpeg_huffman_device(const int16_t* dev_coef, size_t coef_img_stride, uint32_t n, uint32_t w, uint32_t h,
                           uint8_t* host_out, uint32_t* host_len) {
    IK_API_ENTER();
    if (!dev_coef || !host_out || !host_len || !n || !w || !h || w > 65535 || h > 65535)
        return fail(IK_ERR_INVALID, "bad arguments");
    const DeviceConsts* dc = device_consts(current_device());
    if (!dc) return fail(IK_ERR_DEVICE, "cannot upload JPEG tables");
    hipStream_t s = thread_stream();
    if (!s) return fail(IK_ERR_DEVICE, "cannot create HIP stream");
    const JpegEncGeom jg = jpeg_enc_geom(w, h);
    if (n > 1 && coef_img_stride < jg.nmcu * 3 * 64) return fail(IK_ERR_INVALID, "coefficient stride too small");
    // [Huffman work: words + staging][stuffed streams][lengths], as encode_device_front lays them out
    const size_t cap = jg.cap;
    const size_t o_off = jg.work_bytes * n, l_off = o_off + cap * n;
    uint8_t* dw = scratch(l_off + sizeof(uint32_t) * n);
    if (!dw) return fail(IK_ERR_DEVICE, "cannot allocate device scratch");
    const JpegEncArgs a = jg.args(dev_coef, coef_img_stride, dc->jpeg_huff, dw, dw + o_off,
                                  reinterpret_cast<uint32_t*>(dw + l_off));
    // the caller's bytes go up first, so whatever the kernel leaves alone comes back as it was
    if (int rc = copy_h2d_2d(dw + o_off, cap * n, host_out, cap * n, cap * n, 1, s)) return rc;
    const hipError_t e = launch_jpeg_huff_enc(a, (int)n, s);
    if (e == hipErrorInvalidValue)
        return fail(IK_ERR_INVALID, "coefficients must be 16-byte aligned and their stride a multiple of 8");
    if (e != hipSuccess) return hip_fail(e, "jpeg huffman");
    IK_HIP(hipStreamSynchronize(s));
    if (int rc = copy_d2h_2d(reinterpret_cast<uint8_t*>(host_len), 4 * (size_t)n, dw + l_off, 4 * (size_t)n,
                             4 * (size_t)n, 1, s))
        return rc;
    return copy_d2h_2d(host_out, cap * n, dw + o_off, cap * n, cap * n, 1, s);
}

int ik_dev_alloc(size_t bytes, void** dev_ptr) {
    if (!dev_ptr) return fail(IK_ERR_INVALID, "null pointer");
    (void)hipSetDevice(current_device());
    IK_HIP(hipMalloc(dev_ptr, bytes ? bytes : 1));
    return IK_OK;
}
int ik_dev_free(void* p) { IK_HIP(hipFree(p)); return IK_OK; }
int ik_memcpy_h2d(void* d, const void* h, size_t n) {
    IK_API_ENTER();
    IK_HIP(hipDeviceSynchronize());
    return copy_h2d_2d((uint8_t*)d, n, (const uint8_t*)h, n, n, n ? 1 : 0, thread_stream());
}
int ik_memcpy_d2h(void* h, const void* d, size_t n) {
    IK_API_ENTER();
    IK_HIP(hipDeviceSynchronize());
    return copy_d2h_2d((uint8_t*)h, n, (const uint8_t*)d, n, n, n ? 1 : 0, thread_stream());
}
int ik_dev_synchronize(void) { IK_HIP(hipDeviceSynchronize()); return IK_OK; }

}  // extern "C"
