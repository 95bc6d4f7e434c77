// ik_pad_host.cpp -- the pad behind the C ABI: the checks, the frame pixel, the launch over
// a caller's device areas, over one image and over a group of same-geometry images, each
// onto new canvases.  The placement rule is pad_place (ik_post_plan.h); the kernel is
// ik_pad.hip.
#include <atomic>
#include <cstring>

#include "ik_internal.h"
#include "ik_png.h"
#include "ik_runtime.h"

namespace ik {
namespace {

std::atomic<unsigned long long> g_pad_launches{0}, g_pad_images{0};  // ik_pad_counters

// the frame pixel of colour mode as the px = C * depth bytes it has in memory (DESIGN
// section 4): the colour's channels at the image's depth, their luma on a gray image, the
// alpha where there is one
void frame_pixel(const ik_pad& p, uint32_t C, uint32_t depth, uint8_t px[8]) {
    const uint32_t scale = depth == 1 ? 1u : 257u;
    uint32_t v[4] = {0, 0, 0, 0};
    const uint32_t r = (((uint32_t)p.color >> 16) & 0xFFu) * scale, g = (((uint32_t)p.color >> 8) & 0xFFu) * scale,
                   b = ((uint32_t)p.color & 0xFFu) * scale;
    if (C >= 3) { v[0] = r; v[1] = g; v[2] = b; }
    else v[0] = (2126u * r + 7152u * g + 722u * b) / 10000u;  // (at most 10000 * 65535 < 2^32)
    if (C == 2 || C == 4) v[C - 1] = (uint32_t)p.alpha * scale;
    for (uint32_t c = 0; c < C; ++c) {
        if (depth == 1) px[c] = (uint8_t)v[c];
        else { px[2 * c] = (uint8_t)(v[c] & 0xFFu); px[2 * c + 1] = (uint8_t)(v[c] >> 8); }  // native (little-endian) u16
    }
}

// the launch on the current device over checked arguments: W, H >= 1, a canvas that holds
// the image and differs from it, a destination whose bases, pitch and stride are multiples of 4
int pad_launch(const uint8_t* src, size_t src_pitch, size_t src_stride, uint8_t* dst, size_t dst_pitch, size_t dst_stride,
               uint32_t W, uint32_t H, uint32_t C, uint32_t depth, uint32_t n, const ik_pad& p, const PadGeom& g,
               hipStream_t s, const uint64_t* src_tab, const uint64_t* dst_tab) {
    PadArgs a{};
    a.src = src; a.src_pitch = src_pitch; a.src_img_stride = src_stride;
    a.dst = dst; a.dst_pitch = dst_pitch; a.dst_img_stride = dst_stride;
    a.src_tab = src_tab; a.dst_tab = dst_tab;
    a.W = W; a.H = H; a.cw = g.cw; a.ch = g.ch;
    a.x0 = (int32_t)g.x0; a.y0 = (int32_t)g.y0;
    const uint32_t px = C * depth;
    if (p.mode == IK_PAD_COLOR) {
        uint8_t f[8] = {};
        frame_pixel(p, C, depth, f);
        std::memcpy(a.fpx, f, sizeof f);
        for (uint32_t m = 0; m < 3; ++m) {
            uint8_t q[16];
            for (uint32_t k = 0; k < 16; ++k) q[k] = f[(16 * m + k) % px];
            std::memcpy(a.pat[m], q, sizeof q);
        }
    }
    const hipError_t e = launch_pad(a, (int)px, p.mode, (int)n, s);
    if (e != hipSuccess) return hip_fail(e, "pad kernel launch");
    g_pad_launches += 1;
    g_pad_images += n;
    return IK_OK;
}

bool image_ok(const ik_image* im) {
    return im->c >= 1 && im->c <= 4 && im->depth >= 1 && im->depth <= 2 && im->w <= kPadMaxDim && im->h <= kPadMaxDim;
}
// a resolved canvas that pad_launch can take for a W x H image
int geom_check(uint32_t W, uint32_t H, const PadGeom& g) {
    if (g.cw > kPadMaxDim || g.ch > kPadMaxDim) return fail(IK_ERR_INVALID, "a pad canvas of %u x %u pixels", g.cw, g.ch);
    if (g.cw < W || g.ch < H || g.x0 > g.cw - W || g.y0 > g.ch - H) return fail(IK_ERR_INVALID, "bad pad geometry");
    if (!W || !H) return fail(IK_ERR_INVALID, "an empty image cannot be padded");
    return IK_OK;
}

}  // namespace

int pad_check(const ik_pad& p, const char* prefix, bool allow_none) {
    if (p.mode < IK_PAD_NONE || p.mode > IK_PAD_WRAP || (p.mode == IK_PAD_NONE && !allow_none))
        return fail(IK_ERR_INVALID, "%sunknown pad mode %d", prefix, (int)p.mode);
    if (p.gravity < IK_GRAVITY_CENTER || p.gravity > IK_GRAVITY_SW)
        return fail(IK_ERR_INVALID, "%sunknown pad gravity %d", prefix, (int)p.gravity);
    if (p.width < 0 || p.width > (int32_t)kPadMaxDim || p.height < 0 || p.height > (int32_t)kPadMaxDim)
        return fail(IK_ERR_INVALID, "%spad size %d x %d outside 0..2^24", prefix, (int)p.width, (int)p.height);
    if (p.color < 0 || p.color > 0xFFFFFF)
        return fail(IK_ERR_INVALID, "%spad colour %d outside 0x000000..0xFFFFFF", prefix, (int)p.color);
    if (p.alpha < 0 || p.alpha > 255) return fail(IK_ERR_INVALID, "%spad alpha %d outside 0..255", prefix, (int)p.alpha);
    if (p.mode == IK_PAD_NONE && (p.gravity || p.width || p.height || p.color || p.alpha))
        return fail(IK_ERR_INVALID, "%spad fields set without a mode", prefix);
    return IK_OK;
}

// img at g's origin on a new canvas of g's size, in a launch of its own (synchronised); a
// canvas that is the image: a device copy, no launch
int pad_image(const ik_image* img, const PadReq& r, const PadGeom& g, ik_image** out) {
    if (!img || !out) return fail(IK_ERR_INVALID, "null pointer");
    *out = nullptr;
    if (int rc = pad_check(r.p, "", false)) return rc;
    if (!image_ok(img)) return fail(IK_ERR_INVALID, "bad geometry");
    const bool same = g.cw == img->w && g.ch == img->h;
    if (!same)
        if (int rc = geom_check(img->w, img->h, g)) return rc;
    DeviceGuard dg(img->device);
    ik_image* o = nullptr;
    int rc = alloc_image(g.cw, g.ch, img->c, &o, img->depth);
    if (rc) return rc;
    if (g.cw && g.ch) {
        hipStream_t s = thread_stream();
        rc = same ? ik_orient_batch_device(img->d, img->w, img->h, img->c, img->depth, img->pitch, 0, 1, 1, o->d, o->pitch,
                                           0, s)
                  : pad_launch(img->d, img->pitch, 0, o->d, o->pitch, 0, img->w, img->h, img->c, img->depth, 1, r.p, g, s,
                               nullptr, nullptr);
        const hipError_t e = hipStreamSynchronize(s);
        if (!rc && e != hipSuccess) rc = hip_fail(e, "pad");
    }
    if (rc) { ik_image_free(o); return rc; }
    *out = o;
    return IK_OK;
}

// n images of one geometry (same W, H, C, depth, pitch, device) onto new canvases in ONE
// launch, as blur_group: the kernel reads the bases from a table.  A return other than
// IK_OK leaves every image to pad_image.
int pad_group(const std::vector<ik_image*>& src, const PadReq& r, const PadGeom& g, std::vector<ik_image*>& out) {
    const size_t n = src.size();
    out.assign(n, nullptr);
    if (!n) return IK_OK;
    const ik_image* s0 = src[0];
    if (n > kPadMaxImages || !image_ok(s0) || pad_check(r.p, "", false) || geom_check(s0->w, s0->h, g))
        return IK_ERR_UNSUPPORTED;
    DeviceGuard dg(s0->device);
    std::vector<uint64_t> tab(2 * n);
    for (size_t i = 0; i < n; ++i) {
        const int st = alloc_image(g.cw, g.ch, s0->c, &out[i], s0->depth);
        if (st || ((uintptr_t)out[i]->d & 3)) {
            for (ik_image*& o : out) { ik_image_free(o); o = nullptr; }
            return st ? st : IK_ERR_UNSUPPORTED;
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
        rc = fail(IK_ERR_NOMEM, "cannot map pinned pad table");
    if (!rc) {
        (void)hipStreamSynchronize(s);  // the previous table is read
        std::memcpy(ht, tab.data(), 16 * n);
        const hipError_t e =
            launch_copy_words(reinterpret_cast<const uint32_t*>(dht), reinterpret_cast<uint32_t*>(dtab), 4 * n, s);
        if (e != hipSuccess) rc = hip_fail(e, "pad table upload");
    }
    if (!rc)
        rc = pad_launch(nullptr, s0->pitch, 0, nullptr, out[0]->pitch, 0, s0->w, s0->h, s0->c, s0->depth, (uint32_t)n, r.p,
                        g, s, dtab, dtab + n);
    if (!rc) {
        const hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = hip_fail(e, "pad (batched)");
    }
    if (rc)
        for (ik_image*& o : out) { ik_image_free(o); o = nullptr; }
    return rc;
}

}  // namespace ik

using namespace ik;

extern "C" {

int ik_pad_span(void) { return kPadSpan; }
int ik_pad_row_cap(void) { return kPadRowCap; }

int ik_pad_counters(unsigned long long out[2]) {
    if (!out) return fail(IK_ERR_INVALID, "null pointer");
    out[0] = g_pad_launches.load();
    out[1] = g_pad_images.load();
    return IK_OK;
}

int ik_pad_place(uint32_t W, uint32_t H, uint32_t width, uint32_t height, int gravity, int32_t out[4]) {
    if (!out) return fail(IK_ERR_INVALID, "null pointer");
    if (gravity < IK_GRAVITY_CENTER || gravity > IK_GRAVITY_SW) return fail(IK_ERR_INVALID, "unknown pad gravity %d", gravity);
    if (W > kPadMaxDim || H > kPadMaxDim) return fail(IK_ERR_INVALID, "an image of %u x %u pixels", W, H);
    if (width > kPadMaxDim || height > kPadMaxDim)
        return fail(IK_ERR_INVALID, "pad size %u x %u outside 0..2^24", width, height);
    const PadGeom g = pad_place(W, H, width, height, gravity);
    out[0] = (int32_t)g.cw; out[1] = (int32_t)g.ch; out[2] = (int32_t)g.x0; out[3] = (int32_t)g.y0;
    return IK_OK;
}

int ik_pad_batch_device(const uint8_t* dev_src, uint32_t W, uint32_t H, uint32_t C, uint32_t depth, size_t src_pitch,
                        size_t src_image_stride, uint32_t n, const ik_pad* pad, uint32_t canvas_w, uint32_t canvas_h,
                        uint8_t* dev_dst, size_t dst_pitch, size_t dst_image_stride, void* hip_stream) {
    IK_API_ENTER();
    if (!pad) return fail(IK_ERR_INVALID, "null pointer");
    if (int rc = pad_check(*pad, "", false)) return rc;
    if (!dev_src || !dev_dst) return fail(IK_ERR_INVALID, "null device pointer");
    if (C < 1 || C > 4 || depth < 1 || depth > 2 || !W || !H || !n) return fail(IK_ERR_INVALID, "bad geometry");
    if (W > kPadMaxDim || H > kPadMaxDim) return fail(IK_ERR_INVALID, "an image of %u x %u pixels", W, H);
    if (canvas_w > kPadMaxDim || canvas_h > kPadMaxDim || canvas_w < W || canvas_h < H)
        return fail(IK_ERR_INVALID, "a canvas of %u x %u pixels for an image of %u x %u", canvas_w, canvas_h, W, H);
    const size_t srow = (size_t)W * C * depth, drow = (size_t)canvas_w * C * depth;
    if (src_pitch < srow || dst_pitch < drow) return fail(IK_ERR_INVALID, "pitch too small");
    if (n > 1 && (src_image_stride < src_pitch * H || dst_image_stride < dst_pitch * canvas_h))
        return fail(IK_ERR_INVALID, "image stride too small");
    if (n > kPadMaxImages) return fail(IK_ERR_INVALID, "more than %u images", kPadMaxImages);
    if (((uintptr_t)dev_dst | dst_pitch | (n > 1 ? dst_image_stride : 0)) & 3)
        return fail(IK_ERR_INVALID, "the canvas base, pitch and stride must be multiples of 4");
    // the bytes each side spans, first row's first to last row's last
    const uintptr_t s0 = (uintptr_t)dev_src, d0 = (uintptr_t)dev_dst;
    const uintptr_t s1 = s0 + (size_t)(n - 1) * src_image_stride + (size_t)(H - 1) * src_pitch + srow;
    const uintptr_t d1 = d0 + (size_t)(n - 1) * dst_image_stride + (size_t)(canvas_h - 1) * dst_pitch + drow;
    if (s0 < d1 && d0 < s1) return fail(IK_ERR_INVALID, "source and destination overlap");
    const PadGeom g = pad_place(W, H, canvas_w, canvas_h, pad->gravity);
    hipStream_t s = hip_stream ? (hipStream_t)hip_stream : thread_stream();
    return pad_launch(dev_src, src_pitch, src_image_stride, dev_dst, dst_pitch, dst_image_stride, W, H, C, depth, n, *pad,
                      g, s, nullptr, nullptr);
}

int ik_image_pad(const ik_image* img, const ik_pad* pad, ik_image** out) {
    IK_API_ENTER();
    if (!img || !pad || !out) return fail(IK_ERR_INVALID, "null pointer");
    if (int rc = pad_check(*pad, "", false)) return rc;
    if (!image_ok(img)) return fail(IK_ERR_INVALID, "bad geometry");
    PadReq r;
    r.p = *pad;
    return pad_image(img, r, pad_place(img->w, img->h, (uint32_t)pad->width, (uint32_t)pad->height, pad->gravity), out);
}

}  // extern "C"
