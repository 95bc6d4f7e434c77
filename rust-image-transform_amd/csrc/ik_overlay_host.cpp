// ik_overlay_host.cpp -- the watermark overlay behind the C ABI: the placement (host only),
// the checks, the launch over a caller's device area, over one image and over a group of
// same-geometry images, all in place.  The kernel is ik_overlay.hip.
#include <atomic>
#include <cstring>

#include "ik_internal.h"
#include "ik_png.h"
#include "ik_runtime.h"

namespace ik {
namespace {

std::atomic<unsigned long long> g_overlay_launches{0}, g_overlay_images{0};  // ik_overlay_counters

// floor(v / 2) for a v of either sign
int32_t half_floor(int32_t v) { return v >= 0 ? v / 2 : -((-v + 1) / 2); }

// an overlay on the device that holds the bases: the caller's own, or a copy of it for the
// call (freed by the destructor; no cache of such copies is kept)
struct MarkOn {
    const ik_image* use = nullptr;
    ik_image* tmp = nullptr;
    ~MarkOn() { ik_image_free(tmp); }
    // the calling thread's device is `device`
    int bring(const ik_image* mark, int device, hipStream_t s) {
        use = mark;
        if (mark->device == device || !mark->w || !mark->h) return IK_OK;
        if (int rc = alloc_image(mark->w, mark->h, mark->c, &tmp, mark->depth)) return rc;
        IK_HIP(hipMemcpy2DAsync(tmp->d, tmp->pitch, mark->d, mark->pitch, (size_t)mark->w * mark->c * mark->depth, mark->h,
                                hipMemcpyDefault, s));
        use = tmp;
        return IK_OK;
    }
};

// the launch on the current device over checked arguments; an empty window launches nothing
int overlay_launch(uint8_t* base, size_t pitch, size_t stride, const uint64_t* tab, uint32_t W, uint32_t H, uint32_t C,
                   uint32_t depth, uint32_t n, const uint8_t* ov, uint32_t wo, uint32_t ho, uint32_t co, uint32_t od,
                   size_t ov_pitch, const OverlayReq& r, hipStream_t s) {
    int32_t pl[6];
    if (int rc = ik_overlay_place(W, H, wo, ho, r.gravity, r.dx, r.dy, r.tile, pl)) return rc;
    if (!pl[2] || !pl[3]) return IK_OK;
    OverlayArgs a{};
    a.base = base; a.pitch = pitch; a.img_stride = stride; a.tab = tab;
    a.ov = ov; a.ov_pitch = ov_pitch;
    a.wo = (int32_t)wo; a.ho = (int32_t)ho; a.co = (int32_t)co; a.od = (int32_t)od;
    a.wx = pl[0]; a.wy = pl[1]; a.ww = pl[2]; a.wh = pl[3];
    a.x0 = pl[4]; a.y0 = pl[5];
    a.tile = r.tile;
    a.opM = depth == 1 ? (uint32_t)r.opacity : (uint32_t)r.opacity * 257u;
    // (images named by a table are ik_images: pooled hipMalloc blocks, 256-byte pitches)
    a.aligned = tab ? (pitch & 3) == 0 : (((uintptr_t)base | pitch | (n > 1 ? stride : 0)) & 3) == 0;
    a.ov_dword = co == 4 && od == 1 && (((uintptr_t)ov | ov_pitch) & 3) == 0;
    const hipError_t e = launch_overlay(a, (int)C, (int)depth, (int)n, s);
    if (e != hipSuccess) return hip_fail(e, "overlay kernel launch");
    g_overlay_launches += 1;
    g_overlay_images += n;
    return IK_OK;
}

bool image_ok(const ik_image* im) { return im->c >= 1 && im->c <= 4 && im->depth >= 1 && im->depth <= 2; }

}  // namespace

int overlay_check(int32_t gravity, int32_t dx, int32_t dy, int32_t opacity, int32_t opacity_lo, int32_t tile,
                  const char* prefix) {
    if (gravity < IK_GRAVITY_CENTER || gravity > IK_GRAVITY_SW)
        return fail(IK_ERR_INVALID, "%sunknown overlay gravity %d", prefix, (int)gravity);
    if (opacity < opacity_lo || opacity > 255)
        return fail(IK_ERR_INVALID, "%soverlay opacity %d outside %d..255", prefix, (int)opacity, (int)opacity_lo);
    if (tile != 0 && tile != 1) return fail(IK_ERR_INVALID, "%soverlay tile %d is neither 0 nor 1", prefix, (int)tile);
    if (dx < -kOverlayMaxDim || dx > kOverlayMaxDim || dy < -kOverlayMaxDim || dy > kOverlayMaxDim)
        return fail(IK_ERR_INVALID, "%soverlay offset (%d, %d) outside +-%d", prefix, (int)dx, (int)dy, (int)kOverlayMaxDim);
    return IK_OK;
}

// the overlay composited onto one image, in place, in a launch of its own (synchronised)
int overlay_image(ik_image* base, const OverlayReq& r) {
    const ik_image* mark = r.mark;
    if (!base || !mark) return fail(IK_ERR_INVALID, "null pointer");
    if (!image_ok(base) || !image_ok(mark) || !mark->w || !mark->h) return fail(IK_ERR_INVALID, "bad geometry");
    if (!base->w || !base->h) return IK_OK;
    DeviceGuard g(base->device);
    hipStream_t s = thread_stream();
    MarkOn m;
    int rc = m.bring(mark, base->device, s);
    if (!rc)
        rc = overlay_launch(base->d, base->pitch, 0, nullptr, base->w, base->h, base->c, base->depth, 1, m.use->d,
                            m.use->w, m.use->h, m.use->c, m.use->depth, m.use->pitch, r, s);
    const hipError_t e = hipStreamSynchronize(s);  // (also before a copied overlay is freed)
    if (!rc && e != hipSuccess) rc = hip_fail(e, "overlay");
    return rc;
}

// the overlay composited onto n images of one geometry (same W, H, C, depth, pitch,
// device) in ONE launch, in place: the kernel reads the bases from a table.  A return
// other than IK_OK leaves every image to overlay_image (the kernel may have run: in that
// case the stream failed and so will that call).
int overlay_group(const std::vector<ik_image*>& bases, const OverlayReq& r) {
    const size_t n = bases.size();
    if (!n) return IK_OK;
    const ik_image* b0 = bases[0];
    const ik_image* mark = r.mark;
    if (!mark || n > kOverlayMaxImages || !image_ok(b0) || !image_ok(mark) || !mark->w || !mark->h)
        return IK_ERR_UNSUPPORTED;
    if (!b0->w || !b0->h) return IK_OK;
    for (const ik_image* im : bases)
        if ((uintptr_t)im->d & 3) return IK_ERR_UNSUPPORTED;
    DeviceGuard g(b0->device);
    hipStream_t s = thread_stream();
    MarkOn m;
    int rc = m.bring(mark, b0->device, s);
    uint64_t* dtab = reinterpret_cast<uint64_t*>(scratch_slot(kScratchPtrTable, sizeof(uint64_t) * n));
    uint8_t* ht = pinned_slot(kPinnedGroupStage, sizeof(uint64_t) * n);
    void* dht = nullptr;
    if (!rc && !dtab) rc = fail(IK_ERR_DEVICE, "cannot allocate device scratch");
    if (!rc && (!ht || hipHostGetDevicePointer(&dht, ht, 0) != hipSuccess || !dht))
        rc = fail(IK_ERR_NOMEM, "cannot map pinned overlay table");
    if (!rc) {
        (void)hipStreamSynchronize(s);  // the previous table is read
        uint64_t* tab = reinterpret_cast<uint64_t*>(ht);
        for (size_t i = 0; i < n; ++i) tab[i] = (uint64_t)(uintptr_t)bases[i]->d;
        const hipError_t e =
            launch_copy_words(reinterpret_cast<const uint32_t*>(dht), reinterpret_cast<uint32_t*>(dtab), 2 * n, s);
        if (e != hipSuccess) rc = hip_fail(e, "overlay table upload");
    }
    if (!rc)
        rc = overlay_launch(nullptr, b0->pitch, 0, dtab, b0->w, b0->h, b0->c, b0->depth, (uint32_t)n, m.use->d, m.use->w,
                            m.use->h, m.use->c, m.use->depth, m.use->pitch, r, s);
    const hipError_t e = hipStreamSynchronize(s);
    if (!rc && e != hipSuccess) rc = hip_fail(e, "overlay (batched)");
    return rc;
}

}  // namespace ik

using namespace ik;

extern "C" {

int ik_overlay_span(void) { return kOverlaySpan; }

int ik_overlay_counters(unsigned long long out[2]) {
    if (!out) return fail(IK_ERR_INVALID, "null pointer");
    out[0] = g_overlay_launches.load();
    out[1] = g_overlay_images.load();
    return IK_OK;
}

int ik_overlay_place(uint32_t W, uint32_t H, uint32_t wo, uint32_t ho, int gravity, int32_t dx, int32_t dy, int tile,
                     int32_t out[6]) {
    if (!out) return fail(IK_ERR_INVALID, "null pointer");
    if (int rc = overlay_check(gravity, dx, dy, 255, 1, tile, "")) return rc;
    const uint32_t lim = (uint32_t)kOverlayMaxDim;
    if (W > lim || H > lim) return fail(IK_ERR_INVALID, "a base of %u x %u pixels", W, H);
    if (!wo || !ho || wo > lim || ho > lim) return fail(IK_ERR_INVALID, "an overlay of %u x %u pixels", wo, ho);
    // every term is within +-2^24: the sums stay far inside int32
    const int32_t sx = (int32_t)W - (int32_t)wo, sy = (int32_t)H - (int32_t)ho;
    const bool left = gravity == IK_GRAVITY_W || gravity == IK_GRAVITY_NW || gravity == IK_GRAVITY_SW;
    const bool right = gravity == IK_GRAVITY_E || gravity == IK_GRAVITY_NE || gravity == IK_GRAVITY_SE;
    const bool top = gravity == IK_GRAVITY_N || gravity == IK_GRAVITY_NE || gravity == IK_GRAVITY_NW;
    const bool bottom = gravity == IK_GRAVITY_S || gravity == IK_GRAVITY_SE || gravity == IK_GRAVITY_SW;
    const int32_t x0 = (left ? 0 : right ? sx : half_floor(sx)) + dx;
    const int32_t y0 = (top ? 0 : bottom ? sy : half_floor(sy)) + dy;
    int32_t x = 0, y = 0, x1 = (int32_t)W, y1 = (int32_t)H;
    if (!tile) {
        x = x0 > 0 ? x0 : 0;
        y = y0 > 0 ? y0 : 0;
        if (x0 + (int32_t)wo < x1) x1 = x0 + (int32_t)wo;
        if (y0 + (int32_t)ho < y1) y1 = y0 + (int32_t)ho;
    }
    const bool empty = x1 <= x || y1 <= y;
    out[0] = empty ? 0 : x;
    out[1] = empty ? 0 : y;
    out[2] = empty ? 0 : x1 - x;
    out[3] = empty ? 0 : y1 - y;
    out[4] = x0;
    out[5] = y0;
    return IK_OK;
}

int ik_overlay_batch_device(uint8_t* dev_base, uint32_t W, uint32_t H, uint32_t C, uint32_t depth, size_t pitch,
                            size_t image_stride, uint32_t n, const uint8_t* dev_overlay, uint32_t wo, uint32_t ho,
                            uint32_t overlay_channels, uint32_t overlay_depth, size_t overlay_pitch, int gravity,
                            int32_t dx, int32_t dy, int opacity, int tile, void* hip_stream) {
    IK_API_ENTER();
    if (int rc = overlay_check(gravity, dx, dy, opacity, 1, tile, "")) return rc;
    if (!dev_base || !dev_overlay) return fail(IK_ERR_INVALID, "null device pointer");
    if (C < 1 || C > 4 || depth < 1 || depth > 2 || !W || !H || !n) return fail(IK_ERR_INVALID, "bad geometry");
    if (overlay_channels < 1 || overlay_channels > 4 || overlay_depth < 1 || overlay_depth > 2 || !wo || !ho)
        return fail(IK_ERR_INVALID, "bad overlay geometry");
    const size_t row = (size_t)W * C * depth, orow = (size_t)wo * overlay_channels * overlay_depth;
    if (pitch < row || overlay_pitch < orow) return fail(IK_ERR_INVALID, "pitch too small");
    if (n > 1 && image_stride < pitch * H) return fail(IK_ERR_INVALID, "image stride too small");
    if (n > kOverlayMaxImages) return fail(IK_ERR_INVALID, "more than %u images", kOverlayMaxImages);
    // the bytes each side spans, first row's first to last row's last
    const uintptr_t b0 = (uintptr_t)dev_base, o0 = (uintptr_t)dev_overlay;
    const uintptr_t b1 = b0 + (size_t)(n - 1) * image_stride + (size_t)(H - 1) * pitch + row;
    const uintptr_t o1 = o0 + (size_t)(ho - 1) * overlay_pitch + orow;
    if (b0 < o1 && o0 < b1) return fail(IK_ERR_INVALID, "base and overlay overlap");
    OverlayReq r;
    r.gravity = gravity; r.dx = dx; r.dy = dy; r.opacity = opacity; r.tile = tile;
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : thread_stream();
    return overlay_launch(dev_base, pitch, image_stride, nullptr, W, H, C, depth, n, dev_overlay, wo, ho,
                          overlay_channels, overlay_depth, overlay_pitch, r, s);
}

int ik_image_overlay(const ik_image* img, const ik_image* overlay, int gravity, int32_t dx, int32_t dy, int opacity,
                     int tile, ik_image** out) {
    IK_API_ENTER();
    if (!img || !overlay || !out) return fail(IK_ERR_INVALID, "null pointer");
    if (int rc = overlay_check(gravity, dx, dy, opacity, 1, tile, "")) return rc;
    if (!image_ok(img) || !image_ok(overlay) || !overlay->w || !overlay->h) return fail(IK_ERR_INVALID, "bad geometry");
    int32_t pl[6];
    if (int rc = ik_overlay_place(img->w, img->h, overlay->w, overlay->h, gravity, dx, dy, tile, pl)) return rc;
    DeviceGuard g(img->device);
    ik_image* o = nullptr;
    int rc = alloc_image(img->w, img->h, img->c, &o, img->depth);
    if (rc) return rc;
    if (img->w && img->h) {
        const hipError_t e = hipMemcpy2DAsync(o->d, o->pitch, img->d, img->pitch, (size_t)img->w * img->c * img->depth,
                                              img->h, hipMemcpyDeviceToDevice, thread_stream());
        if (e != hipSuccess) rc = hip_fail(e, "overlay: copy of the image");
        OverlayReq r;
        r.mark = overlay; r.gravity = gravity; r.dx = dx; r.dy = dy; r.opacity = opacity; r.tile = tile;
        if (!rc) rc = overlay_image(o, r);  // (synchronises the stream)
    }
    if (rc) { ik_image_free(o); return rc; }
    *out = o;
    return IK_OK;
}

}  // extern "C"
