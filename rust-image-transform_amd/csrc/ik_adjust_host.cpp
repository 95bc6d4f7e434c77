// ik_adjust_host.cpp -- the colour adjustment behind the C ABI: the plan (host only, from
// ik_adjust_plan.h), the cached plans and their device tone tables, the checks, the launch
// over a caller's device area, over one image and over a group of same-geometry images, all
// in place.  The kernel is ik_adjust.hip.
#include <atomic>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>

#include "ik_adjust_plan.h"
#include "ik_internal.h"
#include "ik_png.h"
#include "ik_runtime.h"

namespace ik {
namespace {

std::atomic<unsigned long long> g_adjust_launches{0}, g_adjust_images{0};  // ik_adjust_counters

// one plan on a device: the matrix, and the tone table uploaded once and kept for the life
// of the library, as the blur axis tables are (never evicted)
struct AdjustDev {
    int flags = 0;
    int32_t q[9] = {};
    void* tone = nullptr;  // null: the table is the identity
    size_t bytes = 0;
};
std::mutex g_adjust_mu;
std::map<std::tuple<int, AdjustReq::Key, int>, AdjustDev*> g_adjust_plans;  // (device, the 24 bytes, depth)

// the plan of checked parameters on the current device
const AdjustDev* adjust_plan_dev(int device, const ik_adjust& adj, int depth) {
    AdjustReq r;
    r.a = adj;
    const auto key = std::make_tuple(device, r.key(), depth);
    std::lock_guard<std::mutex> lk(g_adjust_mu);
    auto it = g_adjust_plans.find(key);
    if (it != g_adjust_plans.end()) return it->second;
    auto* d = new AdjustDev();
    std::vector<uint16_t> t(depth == 1 ? 256 : 65536);
    if (ik_adjust_plan(&adj, depth, t.data(), d->q, &d->flags) != IK_OK) {
        delete d;
        return nullptr;
    }
    if (d->flags & kAdjustFlagTable) {
        std::vector<uint8_t> blob(depth == 1 ? 256 : 65536 * sizeof(uint16_t));
        if (depth == 1)
            for (int v = 0; v < 256; ++v) blob[v] = (uint8_t)t[v];
        else std::memcpy(blob.data(), t.data(), blob.size());
        d->bytes = blob.size();
        // uploaded on this thread's stream and synchronised there (copy_h2d_2d)
        if (hipMalloc(&d->tone, blob.size()) != hipSuccess ||
            copy_h2d_2d(static_cast<uint8_t*>(d->tone), blob.size(), blob.data(), blob.size(), blob.size(), 1,
                        thread_stream()) != IK_OK) {
            if (d->tone) (void)hipFree(d->tone);
            delete d;
            return nullptr;
        }
        mem_stat(kMemPlans, (int64_t)d->bytes);
    }
    g_adjust_plans[key] = d;
    return d;
}

// the launch on the current device over checked arguments; a plan with nothing to do for
// these channels launches nothing
int adjust_launch(uint8_t* base, size_t pitch, size_t stride, const uint64_t* tab, uint32_t W, uint32_t H, uint32_t C,
                  uint32_t depth, uint32_t n, const ik_adjust& adj, hipStream_t s) {
    if (adjust_is_none(adj)) return IK_OK;
    const AdjustDev* p = adjust_plan_dev(current_device(), adj, (int)depth);
    if (!p) return fail(IK_ERR_DEVICE, "cannot build the adjust plan");
    const bool matrix = (p->flags & kAdjustFlagMatrix) && C >= 3;
    if (!matrix && !p->tone) return IK_OK;
    AdjustArgs a{};
    a.base = base; a.pitch = pitch; a.img_stride = stride; a.tab = tab;
    a.tone = p->tone;
    std::memcpy(a.q, p->q, sizeof a.q);
    a.W = W; a.H = H;
    // (images named by a table are ik_images: pooled hipMalloc blocks, 256-byte pitches)
    a.aligned = tab ? (pitch & 3) == 0 : (((uintptr_t)base | pitch | (n > 1 ? stride : 0)) & 3) == 0;
    const hipError_t e = launch_adjust(a, (int)C, (int)depth, matrix, (int)n, s);
    if (e != hipSuccess) return hip_fail(e, "adjust kernel launch");
    g_adjust_launches += 1;
    g_adjust_images += n;
    return IK_OK;
}

bool image_ok(const ik_image* im) {
    return im->c >= 1 && im->c <= 4 && im->depth >= 1 && im->depth <= 2 && im->w <= kAdjustMaxDim && im->h <= kAdjustMaxDim;
}

}  // namespace

int adjust_check(const ik_adjust& a, const char* prefix) {
    const char* bad = adjust_bad_field(a);
    if (!bad) return IK_OK;
    if (!std::strcmp(bad, "gamma"))
        return fail(IK_ERR_INVALID, "%sadjust gamma %g is neither 0 nor in 0.1..10", prefix, (double)a.gamma);
    const int32_t v = !std::strcmp(bad, "brightness") ? a.brightness
                      : !std::strcmp(bad, "contrast") ? a.contrast
                      : !std::strcmp(bad, "saturation") ? a.saturation
                      : !std::strcmp(bad, "hue")        ? a.hue
                                                        : a.invert;
    return fail(IK_ERR_INVALID, "%sadjust %s %d out of range", prefix, bad, (int)v);
}

void adjust_shutdown() {
    std::lock_guard<std::mutex> lk(g_adjust_mu);
    for (auto& kv : g_adjust_plans) {
        if (kv.second->tone) {
            (void)hipFree(kv.second->tone);
            mem_stat(kMemPlans, -(int64_t)kv.second->bytes);
        }
        delete kv.second;
    }
    g_adjust_plans.clear();
}

// the adjustment applied to one image, in place, in a launch of its own (synchronised)
int adjust_image(ik_image* img, const AdjustReq& r) {
    if (!img) return fail(IK_ERR_INVALID, "null pointer");
    if (int rc = adjust_check(r.a, "")) return rc;
    if (!image_ok(img)) return fail(IK_ERR_INVALID, "bad geometry");
    if (!img->w || !img->h) return IK_OK;
    DeviceGuard g(img->device);
    hipStream_t s = thread_stream();
    int rc = adjust_launch(img->d, img->pitch, 0, nullptr, img->w, img->h, img->c, img->depth, 1, r.a, s);
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = hip_fail(e, "adjust");
    return rc;
}

// the adjustment applied to n images of one geometry (same W, H, C, depth, pitch, device) in
// ONE launch, in place: the kernel reads the bases from a table.  A return other than IK_OK
// leaves every image to adjust_image (the kernel may have run: in that case the stream
// failed and so will that call).
int adjust_group(const std::vector<ik_image*>& imgs, const AdjustReq& r) {
    const size_t n = imgs.size();
    if (!n) return IK_OK;
    const ik_image* b0 = imgs[0];
    if (n > kAdjustMaxImages || !image_ok(b0) || adjust_bad_field(r.a)) return IK_ERR_UNSUPPORTED;
    if (!b0->w || !b0->h) return IK_OK;
    for (const ik_image* im : imgs)
        if ((uintptr_t)im->d & 3) return IK_ERR_UNSUPPORTED;
    DeviceGuard g(b0->device);
    hipStream_t s = thread_stream();
    int rc = IK_OK;
    uint64_t* dtab = reinterpret_cast<uint64_t*>(scratch_slot(kScratchPtrTable, sizeof(uint64_t) * n));
    uint8_t* ht = pinned_slot(kPinnedGroupStage, sizeof(uint64_t) * n);
    void* dht = nullptr;
    if (!dtab) rc = fail(IK_ERR_DEVICE, "cannot allocate device scratch");
    if (!rc && (!ht || hipHostGetDevicePointer(&dht, ht, 0) != hipSuccess || !dht))
        rc = fail(IK_ERR_NOMEM, "cannot map pinned adjust table");
    if (!rc) {
        (void)hipStreamSynchronize(s);  // the previous table is read
        uint64_t* tab = reinterpret_cast<uint64_t*>(ht);
        for (size_t i = 0; i < n; ++i) tab[i] = (uint64_t)(uintptr_t)imgs[i]->d;
        const hipError_t e =
            launch_copy_words(reinterpret_cast<const uint32_t*>(dht), reinterpret_cast<uint32_t*>(dtab), 2 * n, s);
        if (e != hipSuccess) rc = hip_fail(e, "adjust table upload");
    }
    if (!rc) rc = adjust_launch(nullptr, b0->pitch, 0, dtab, b0->w, b0->h, b0->c, b0->depth, (uint32_t)n, r.a, s);
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = hip_fail(e, "adjust (batched)");
    return rc;
}

}  // namespace ik

using namespace ik;

extern "C" {

int ik_adjust_span(void) { return kAdjustSpan; }

int ik_adjust_counters(unsigned long long out[2]) {
    if (!out) return fail(IK_ERR_INVALID, "null pointer");
    out[0] = g_adjust_launches.load();
    out[1] = g_adjust_images.load();
    return IK_OK;
}

int ik_adjust_plan(const ik_adjust* adj, int depth, uint16_t* table, int32_t matrix[9], int* flags) {
    if (!adj) return fail(IK_ERR_INVALID, "null pointer");
    if (depth != 1 && depth != 2) return fail(IK_ERR_INVALID, "depth %d is neither 1 nor 2", depth);
    if (int rc = adjust_check(*adj, "")) return rc;
    int32_t q[9];
    int f = adjust_matrix(*adj, q) ? kAdjustFlagMatrix : 0;
    if (matrix) std::memcpy(matrix, q, sizeof q);
    const bool tone = adj->brightness || adj->contrast || adj->gamma != 0.0f || adj->invert;
    if (table || (flags && tone)) {
        std::vector<uint16_t> own;
        uint16_t* t = table;
        if (!t) {
            own.resize(depth == 1 ? 256 : 65536);
            t = own.data();
        }
        if (adjust_table(*adj, depth, t)) f |= kAdjustFlagTable;
    }
    if (flags) *flags = f;
    return IK_OK;
}

int ik_adjust_batch_device(uint8_t* dev, uint32_t W, uint32_t H, uint32_t C, uint32_t depth, size_t pitch,
                           size_t image_stride, uint32_t n, const ik_adjust* adj, void* hip_stream) {
    IK_API_ENTER();
    if (!adj) return fail(IK_ERR_INVALID, "null pointer");
    if (int rc = adjust_check(*adj, "")) return rc;
    if (!dev) return fail(IK_ERR_INVALID, "null device pointer");
    if (C < 1 || C > 4 || depth < 1 || depth > 2 || !W || !H || !n) return fail(IK_ERR_INVALID, "bad geometry");
    if (W > kAdjustMaxDim || H > kAdjustMaxDim) return fail(IK_ERR_INVALID, "an image of %u x %u pixels", W, H);
    if (pitch < (size_t)W * C * depth) return fail(IK_ERR_INVALID, "pitch too small");
    if (n > 1 && image_stride < pitch * H) return fail(IK_ERR_INVALID, "image stride too small");
    if (n > kAdjustMaxImages) return fail(IK_ERR_INVALID, "more than %u images", kAdjustMaxImages);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : thread_stream();
    return adjust_launch(dev, pitch, image_stride, nullptr, W, H, C, depth, n, *adj, s);
}

int ik_image_adjust(const ik_image* img, const ik_adjust* adj, ik_image** out) {
    IK_API_ENTER();
    if (!img || !adj || !out) return fail(IK_ERR_INVALID, "null pointer");
    if (int rc = adjust_check(*adj, "")) return rc;
    if (!image_ok(img)) return fail(IK_ERR_INVALID, "bad geometry");
    DeviceGuard g(img->device);
    ik_image* o = nullptr;
    int rc = alloc_image(img->w, img->h, img->c, &o, img->depth);
    if (rc) return rc;
    if (img->w && img->h) {
        hipStream_t s = thread_stream();
        const hipError_t e = hipMemcpy2DAsync(o->d, o->pitch, img->d, img->pitch, (size_t)img->w * img->c * img->depth,
                                              img->h, hipMemcpyDeviceToDevice, s);
        if (e != hipSuccess) rc = hip_fail(e, "adjust: copy of the image");
        AdjustReq r;
        r.a = *adj;
        if (!rc) rc = adjust_image(o, r);  // (synchronises the stream)
        else (void)hipStreamSynchronize(s);
    }
    if (rc) { ik_image_free(o); return rc; }
    *out = o;
    return IK_OK;
}

}  // extern "C"
