// ik_blur_host.cpp -- blur and unsharpen behind the C ABI: the cached device tables of an
// axis (ik_blur_plan.h), the launch over a caller's device area, over one image and over
// a group of same-geometry images.  The kernel is ik_blur.hip.
#include <atomic>
#include <cmath>
#include <cstring>
#include <map>
#include <mutex>
#include <tuple>

#include "ik_blur_plan.h"
#include "ik_internal.h"
#include "ik_png.h"
#include "ik_runtime.h"

namespace ik {
namespace {

std::atomic<unsigned long long> g_blur_launches{0}, g_blur_images{0};  // ik_blur_counters

// one axis's tables on a device, kept for the life of the library as the resize plans are
struct BlurAxisDev {
    BlurAxisTab tab{};
    int halo = 0;
    void* dev = nullptr;
    size_t bytes = 0;
};
std::mutex g_blur_mu;
std::map<std::tuple<int, uint32_t, uint32_t>, BlurAxisDev*> g_blur_axes;  // (device, L, sigma's bits)

uint32_t float_bits(float f) {
    uint32_t u;
    std::memcpy(&u, &f, 4);
    return u;
}

const BlurAxisDev* blur_axis(int device, uint32_t L, float sigma) {
    const auto key = std::make_tuple(device, L, float_bits(sigma));
    std::lock_guard<std::mutex> lk(g_blur_mu);
    auto it = g_blur_axes.find(key);
    if (it != g_blur_axes.end()) return it->second;
    BlurAxis a;
    blur_axis_weights((int)L, sigma, a);
    if (a.rl > kBlurMaxR || a.rr > kBlurMaxR) return nullptr;  // (no sigma <= kBlurMaxSigma gets here)
    const size_t o_left = 0, o_cnt = (sizeof(int) * L + 255) & ~size_t(255);
    const size_t o_w = o_cnt + ((sizeof(int) * L + 255) & ~size_t(255));
    std::vector<uint8_t> blob(o_w + sizeof(float) * a.w.size());
    std::memcpy(blob.data() + o_left, a.left.data(), sizeof(int) * L);
    std::memcpy(blob.data() + o_cnt, a.cnt.data(), sizeof(int) * L);
    std::memcpy(blob.data() + o_w, a.w.data(), sizeof(float) * a.w.size());
    auto* d = new BlurAxisDev();
    d->bytes = blob.size();
    // uploaded on this thread's stream and synchronised there (copy_h2d_2d)
    if (hipMalloc(&d->dev, blob.size()) != hipSuccess ||
        copy_h2d_2d(static_cast<uint8_t*>(d->dev), blob.size(), blob.data(), blob.size(), blob.size(), 1,
                    thread_stream()) != IK_OK) {
        if (d->dev) (void)hipFree(d->dev);
        delete d;
        return nullptr;
    }
    mem_stat(kMemPlans, (int64_t)d->bytes);
    const uint8_t* p = static_cast<const uint8_t*>(d->dev);
    d->tab.left = reinterpret_cast<const int*>(p + o_left);
    d->tab.cnt = reinterpret_cast<const int*>(p + o_cnt);
    d->tab.w = reinterpret_cast<const float*>(p + o_w);
    d->tab.T = a.T;
    d->tab.u_lo = a.u_lo; d->tab.u_hi = a.u_hi; d->tab.u_dl = a.u_dl; d->tab.u_cnt = a.u_cnt;
    d->halo = a.rl + a.rr;
    g_blur_axes[key] = d;
    return d;
}

}  // namespace

bool blur_threshold_ok(int32_t t) { return t >= 0 && t <= 65535; }

// ik_shutdown: every cached axis's device tables
void blur_shutdown() {
    std::lock_guard<std::mutex> lk(g_blur_mu);
    for (auto& kv : g_blur_axes) {
        (void)hipFree(kv.second->dev);
        mem_stat(kMemPlans, -(int64_t)kv.second->bytes);
        delete kv.second;
    }
    g_blur_axes.clear();
}

// the launch on the current device; the arguments are the caller's to have checked
int blur_launch(const uint8_t* src, size_t src_pitch, size_t src_stride, uint8_t* dst, size_t dst_pitch,
                size_t dst_stride, uint32_t W, uint32_t H, uint32_t C, uint32_t depth, uint32_t n, float sigma,
                bool sharpen, int32_t threshold, hipStream_t s, const uint64_t* src_tab, const uint64_t* dst_tab) {
    const int dev = current_device();
    const BlurAxisDev* ax = blur_axis(dev, W, sigma);
    const BlurAxisDev* ay = ax ? blur_axis(dev, H, sigma) : nullptr;
    if (!ax || !ay) return fail(IK_ERR_DEVICE, "cannot build blur tables");
    BlurArgs a{};
    a.src = src; a.src_pitch = src_pitch; a.src_img_stride = src_stride;
    a.dst = dst; a.dst_pitch = dst_pitch; a.dst_img_stride = dst_stride;
    a.src_tab = src_tab; a.dst_tab = dst_tab;
    a.W = W; a.H = H; a.C = C;
    a.x = ax->tab; a.y = ay->tab;
    a.halo = ax->halo;
    a.threshold = threshold;
    // (images named by a table are ik_images: pooled hipMalloc blocks, 256-byte pitches)
    a.src_aligned = src_tab ? (src_pitch & 3) == 0 : (((uintptr_t)src | src_pitch | (n > 1 ? src_stride : 0)) & 3) == 0;
    a.dst_aligned = dst_tab ? (dst_pitch & 3) == 0 : (((uintptr_t)dst | dst_pitch | (n > 1 ? dst_stride : 0)) & 3) == 0;
    const hipError_t e = launch_blur(a, (int)depth, sharpen, (int)n, s);
    if (e != hipSuccess) return hip_fail(e, "blur kernel launch");
    g_blur_launches += 1;
    g_blur_images += n;
    return IK_OK;
}

// blur (or unsharpen) over n images of one geometry (same W, H, C, depth, pitch) in ONE
// launch, as flatten_group: new images, the kernel reads the bases from a table.  A return
// other than IK_OK leaves every image to ik_image_blur / ik_image_unsharpen.
int blur_group(const std::vector<ik_image*>& src, float sigma, bool sharpen, int32_t threshold,
               std::vector<ik_image*>& out) {
    const size_t n = src.size();
    out.assign(n, nullptr);
    if (!n) return IK_OK;
    const ik_image* s0 = src[0];
    if (n > kBlurMaxImages || !s0->w || !s0->h || s0->c < 1 || s0->c > 4) return IK_ERR_UNSUPPORTED;
    for (const ik_image* im : src)
        if ((uintptr_t)im->d & 3) return IK_ERR_UNSUPPORTED;
    DeviceGuard g(s0->device);
    std::vector<uint64_t> tab(2 * n);
    for (size_t i = 0; i < n; ++i) {
        const int st = alloc_image(s0->w, s0->h, s0->c, &out[i], s0->depth);
        if (st) {
            for (ik_image*& o : out) { ik_image_free(o); o = nullptr; }
            return st;
        }
        tab[i] = (uint64_t)(uintptr_t)src[i]->d;
        tab[n + i] = (uint64_t)(uintptr_t)out[i]->d;
    }
    hipStream_t s = thread_stream();
    uint64_t* dtab = reinterpret_cast<uint64_t*>(scratch_slot(kScratchPtrTable, sizeof(uint64_t) * 2 * n));
    uint8_t* ht = pinned_slot(kPinnedGroupStage, 16 * n);
    void* dht = nullptr;
    int rc = IK_OK;
    if (!dtab) rc = fail(IK_ERR_DEVICE, "cannot allocate device scratch");
    else if (!ht || hipHostGetDevicePointer(&dht, ht, 0) != hipSuccess || !dht)
        rc = fail(IK_ERR_NOMEM, "cannot map pinned blur table");
    if (!rc) {
        (void)hipStreamSynchronize(s);  // the previous table is read
        std::memcpy(ht, tab.data(), 16 * n);
        const hipError_t e =
            launch_copy_words(reinterpret_cast<const uint32_t*>(dht), reinterpret_cast<uint32_t*>(dtab), 4 * n, s);
        if (e != hipSuccess) rc = hip_fail(e, "blur table upload");
    }
    if (!rc)
        rc = blur_launch(nullptr, s0->pitch, 0, nullptr, out[0]->pitch, 0, s0->w, s0->h, s0->c, s0->depth, (uint32_t)n,
                         sigma, sharpen, threshold, s, dtab, dtab + n);
    if (!rc) {
        const hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = hip_fail(e, sharpen ? "unsharpen (batched)" : "blur (batched)");
    }
    if (rc)
        for (ik_image*& o : out) { ik_image_free(o); o = nullptr; }
    return rc;
}

static int image_filter(const ik_image* img, float sigma, bool sharpen, int32_t threshold, ik_image** out) {
    if (!img || !out) return fail(IK_ERR_INVALID, "null pointer");
    if (!blur_sigma_ok(sigma))
        return fail(IK_ERR_INVALID, "sigma %g outside %g..%g", (double)sigma, (double)kBlurMinSigma, (double)kBlurMaxSigma);
    if (!blur_threshold_ok(threshold)) return fail(IK_ERR_INVALID, "threshold %d outside 0..65535", (int)threshold);
    if (img->c < 1 || img->c > 4 || img->depth < 1 || img->depth > 2) return fail(IK_ERR_INVALID, "bad geometry");
    DeviceGuard g(img->device);
    ik_image* o = nullptr;
    int rc = alloc_image(img->w, img->h, img->c, &o, img->depth);
    if (rc) return rc;
    if (img->w && img->h) {
        hipStream_t s = thread_stream();
        rc = ik_blur_batch_device(img->d, img->w, img->h, img->c, img->depth, img->pitch, 0, 1, sigma, sharpen ? 1 : 0,
                                  threshold, o->d, o->pitch, 0, s);
        if (rc == IK_OK) {
            const hipError_t e = hipStreamSynchronize(s);
            if (e != hipSuccess) rc = hip_fail(e, sharpen ? "unsharpen" : "blur");
        }
    }
    if (rc) { ik_image_free(o); return rc; }
    *out = o;
    return IK_OK;
}

}  // namespace ik

using namespace ik;

extern "C" {

int ik_blur_tile(int out[2]) {
    if (!out) return fail(IK_ERR_INVALID, "null pointer");
    out[0] = kBlurTileW;
    out[1] = kBlurTileH;
    return IK_OK;
}

int ik_blur_counters(unsigned long long out[2]) {
    if (!out) return fail(IK_ERR_INVALID, "null pointer");
    out[0] = g_blur_launches.load();
    out[1] = g_blur_images.load();
    return IK_OK;
}

int ik_blur_axis_plan(uint32_t L, float sigma, int32_t* left, int32_t* count, float* weights, uint32_t cap_taps,
                      uint32_t* taps) {
    if (!taps) return fail(IK_ERR_INVALID, "null pointer");
    if (!L || L > (1u << 24)) return fail(IK_ERR_INVALID, "axis of %u samples", L);
    if (!blur_sigma_ok(sigma))
        return fail(IK_ERR_INVALID, "sigma %g outside %g..%g", (double)sigma, (double)kBlurMinSigma, (double)kBlurMaxSigma);
    BlurAxis a;
    blur_axis_weights((int)L, sigma, a);
    *taps = (uint32_t)a.T;
    if (!left && !count && !weights) return IK_OK;  // the tap count alone
    if (!left || !count || !weights) return fail(IK_ERR_INVALID, "null pointer");
    if (cap_taps < (uint32_t)a.T) return fail(IK_ERR_INVALID, "%d taps do not fit rows of %u", a.T, cap_taps);
    for (uint32_t o = 0; o < L; ++o) {
        left[o] = a.left[o];
        count[o] = a.cnt[o];
        float* row = weights + (size_t)o * cap_taps;
        std::memcpy(row, &a.w[(size_t)o * a.T], sizeof(float) * a.T);
        for (uint32_t k = (uint32_t)a.T; k < cap_taps; ++k) row[k] = 0.0f;
    }
    return IK_OK;
}

int ik_blur_batch_device(const uint8_t* dev_src, uint32_t W, uint32_t H, uint32_t C, uint32_t depth, size_t src_pitch,
                         size_t src_image_stride, uint32_t n, float sigma, int sharpen, int32_t threshold,
                         uint8_t* dev_dst, size_t dst_pitch, size_t dst_image_stride, void* hip_stream) {
    IK_API_ENTER();
    if (!blur_sigma_ok(sigma))
        return fail(IK_ERR_INVALID, "sigma %g outside %g..%g", (double)sigma, (double)kBlurMinSigma, (double)kBlurMaxSigma);
    if (sharpen != 0 && sharpen != 1) return fail(IK_ERR_INVALID, "sharpen %d is neither 0 (blur) nor 1 (unsharpen)", sharpen);
    if (!blur_threshold_ok(threshold)) return fail(IK_ERR_INVALID, "threshold %d outside 0..65535", (int)threshold);
    if (!dev_src || !dev_dst) return fail(IK_ERR_INVALID, "null device pointer");
    if (C < 1 || C > 4 || depth < 1 || depth > 2 || !W || !H || !n) return fail(IK_ERR_INVALID, "bad geometry");
    if (W > (1u << 24) || (H + kBlurTileH - 1) / kBlurTileH > 65535u) return fail(IK_ERR_INVALID, "image too large to blur");
    const size_t row = (size_t)W * C * depth;
    if (src_pitch < row || dst_pitch < row) return fail(IK_ERR_INVALID, "pitch too small");
    if (n > 1 && (src_image_stride < src_pitch * H || dst_image_stride < dst_pitch * H))
        return fail(IK_ERR_INVALID, "image stride too small");
    if (n > kBlurMaxImages) return fail(IK_ERR_INVALID, "more than %u images", kBlurMaxImages);
    // the bytes each side spans, first row's first to last row's last
    const uintptr_t s0 = (uintptr_t)dev_src, d0 = (uintptr_t)dev_dst;
    const uintptr_t s1 = s0 + (size_t)(n - 1) * src_image_stride + (size_t)(H - 1) * src_pitch + row;
    const uintptr_t d1 = d0 + (size_t)(n - 1) * dst_image_stride + (size_t)(H - 1) * dst_pitch + row;
    if (s0 < d1 && d0 < s1) return fail(IK_ERR_INVALID, "source and destination overlap");
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : thread_stream();
    return blur_launch(dev_src, src_pitch, src_image_stride, dev_dst, dst_pitch, dst_image_stride, W, H, C, depth, n, sigma,
                       sharpen != 0, threshold, s, nullptr, nullptr);
}

int ik_image_blur(const ik_image* img, float sigma, ik_image** out) {
    IK_API_ENTER();
    return image_filter(img, sigma, false, 0, out);
}

int ik_image_unsharpen(const ik_image* img, float sigma, int32_t threshold, ik_image** out) {
    IK_API_ENTER();
    return image_filter(img, sigma, true, threshold, out);
}

}  // extern "C"
