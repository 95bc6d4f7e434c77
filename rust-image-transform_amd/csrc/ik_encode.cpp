// ik_encode.cpp -- encode_image's device front ends and host back end, image by image
// and for a batch's groups (transform_post_phase, ik_host.cpp): the colour-conversion
// launches, the GPU JPEG coder's launches and file assembly, the exact WebP coder's
// group calls, the one-launch resize of a same-geometry group, and the per-device
// constant tables they read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <vector>

#include "../../include/imagekit_hip.h"
#include "ik_png.h"  // launch_copy_words
#include "ik_runtime.h"

namespace ik {

void webp_gamma_tables(uint16_t g2l[256], int l2g[33]) {
    // libwebp picture_csp_enc.c InitGammaTables: kGamma 0.80, kGammaFix 12, kGammaTabFix 7
    const double scale = (double)(1 << 7) / ((1 << 12) - 1);
    const double norm = 1. / 255.;
    for (int v = 0; v <= 255; ++v) g2l[v] = (uint16_t)(pow(norm * v, 0.80) * ((1 << 12) - 1) + .5);
    for (int v = 0; v <= 32; ++v) l2g[v] = (int)(255. * pow(scale * v, 1. / 0.80) + .5);
}

namespace {
std::mutex g_consts_mu;
std::map<int, DeviceConsts*> g_consts;
std::atomic<unsigned long long> g_jpeg_enc_gpu{0}, g_jpeg_enc_host{0};
}  // namespace

void jpeg_enc_count(bool gpu_coded) { (gpu_coded ? g_jpeg_enc_gpu : g_jpeg_enc_host) += 1; }

uint8_t* jpeg_file(const std::vector<uint8_t>& hdr, const uint8_t* stream, uint32_t len, std::vector<uint8_t>& out) {
    out.resize(hdr.size() + len + 2);
    std::memcpy(out.data(), hdr.data(), hdr.size());
    uint8_t* at = out.data() + hdr.size();
    if (stream && len) std::memcpy(at, stream, len);
    at[len] = 0xFF;  // EOI
    at[len + 1] = 0xD9;
    return at;
}

const DeviceConsts* device_consts(int device) {
    std::mutex& mu = g_consts_mu;
    std::map<int, DeviceConsts*>& m = g_consts;
    std::lock_guard<std::mutex> lk(mu);
    auto it = m.find(device);
    if (it != m.end()) return it->second;
    uint16_t g2l[256];
    int l2g[33];
    webp_gamma_tables(g2l, l2g);
    uint32_t hf[4 * 256];
    jpeg_huff_u32(hf);
    auto* dc = new DeviceConsts();
    (void)hipSetDevice(device);
    if (hipMalloc(&dc->gamma_to_lin, sizeof(g2l)) != hipSuccess ||
        hipMalloc(&dc->lin_to_gamma, sizeof(l2g)) != hipSuccess ||
        hipMalloc(&dc->jpeg_huff, sizeof(hf)) != hipSuccess ||
        hipMemcpy(dc->gamma_to_lin, g2l, sizeof(g2l), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dc->lin_to_gamma, l2g, sizeof(l2g), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(dc->jpeg_huff, hf, sizeof(hf), hipMemcpyHostToDevice) != hipSuccess ||
        hipDeviceSynchronize() != hipSuccess) {  // order before non-blocking streams
        delete dc;
        return nullptr;
    }
    m[device] = dc;
    return dc;
}

// Run the device front end of encode_image and hand its output to the host
// entropy stage.  WebP: to_rgb8 + RGB->YUV420 on the GPU, libwebp VP8 coding of
// those planes on the host.  JPEG: to_rgb8 + YCbCr + FDCT + quantise on the GPU,
// baseline Huffman coding on the host.  AVIF: to_rgba8 + YCbCr 4:4:4 on the GPU,
// AV1 coding by libavif/aom on the host.
int encode_device_front(const uint8_t* dev, uint32_t w, uint32_t h, uint32_t c, size_t pitch, int fmt, int quality,
                        EncodePrep& p, std::vector<uint8_t>& out) {
    const int q = clamp_quality(quality);
    p.fmt = fmt;
    p.q = q;
    p.w = w;
    p.h = h;
    p.done = true;  // unless a host coder is left to run (encode_host_back)
    hipStream_t s = thread_stream();
    if (!s) return fail(IK_ERR_DEVICE, "cannot create HIP stream");
    if (fmt == IK_FORMAT_WEBP) {
        if (w > 16383 || h > 16383) return fail(IK_ERR_TRANSFORM, "WebP dimensions %ux%u exceed 16383", w, h);
        const DeviceConsts* dc = device_consts(current_device());
        if (!dc) return fail(IK_ERR_DEVICE, "cannot upload WebP tables");
        const size_t bytes = yuv420_bytes(w, h);
        if (default_webp_encoder() == IK_WEBP_EXACT) {  // (read once: a concurrent switch cannot mix paths)
            uint8_t* dyuv = scratch(bytes);
            if (!dyuv) return fail(IK_ERR_DEVICE, "cannot allocate device scratch");
            hipError_t e = launch_webp_yuv420(dev, (int)w, (int)h, (int)c, pitch, 0, dyuv, 0, 1,
                                              dc->gamma_to_lin, dc->lin_to_gamma, s);
            if (e != hipSuccess) return hip_fail(e, "webp yuv420");
            std::vector<std::vector<uint8_t>> files;
            if (int rc = webp_encode_exact(dyuv, 0, 1, (int)w, (int)h, q, files)) return rc;
            out.swap(files[0]);
            return IK_OK;
        }
        // the colour kernel writes the planes straight into pinned host memory: no
        // copy-engine transfer, which would queue behind another batch's stream upload
        uint8_t* hp = pinned_slot(kPinnedWebpPlanes, bytes);
        void* dhp = nullptr;
        if (!hp || hipHostGetDevicePointer(&dhp, hp, 0) != hipSuccess || !dhp)
            return fail(IK_ERR_NOMEM, "cannot map pinned WebP planes");
        hipError_t e = launch_webp_yuv420(dev, (int)w, (int)h, (int)c, pitch, 0, reinterpret_cast<uint8_t*>(dhp), 0, 1,
                                          dc->gamma_to_lin, dc->lin_to_gamma, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(e, "webp yuv420");
        p.planes.assign(hp, hp + bytes);
        p.done = false;  // libwebp's VP8 coding of the planes: encode_host_back
        return IK_OK;
    }
    if (fmt == IK_FORMAT_JPEG) {
        if (w > 65535 || h > 65535) return fail(IK_ERR_TRANSFORM, "JPEG dimensions %ux%u exceed 65535", w, h);
        uint8_t qt[128];
        jpeg_quant_tables(q, qt);
        const JpegEncGeom jg = jpeg_enc_geom(w, h);
        const size_t cbytes = jg.coef_bytes;
        const DeviceConsts* dc = device_consts(current_device());
        if (!dc) return fail(IK_ERR_DEVICE, "cannot upload JPEG tables");
        // [qtables 256][coefficients][Huffman work: words + staging][stuffed stream][length]
        const size_t c_off = 256, w_off = c_off + (cbytes + 255) / 256 * 256;
        const size_t o_off = w_off + jg.work_bytes, l_off = o_off + jg.cap;
        uint8_t* dq = scratch(l_off + 256);
        if (!dq) return fail(IK_ERR_DEVICE, "cannot allocate device scratch");
        int16_t* dcoef = (int16_t*)(dq + c_off);
        int rc = copy_h2d_2d(dq, 128, qt, 128, 128, 1, s);
        if (rc) return rc;
        hipError_t e = launch_jpeg_coeffs(dev, (int)w, (int)h, (int)c, pitch, 0, dq, dcoef, 0, 1, s);
        if (e != hipSuccess) return hip_fail(e, "jpeg coefficients");
        e = launch_jpeg_huff_enc(jg.args(dcoef, 0, dc->jpeg_huff, dq + w_off, dq + o_off,
                                         reinterpret_cast<uint32_t*>(dq + l_off)), 1, s);
        if (e != hipSuccess) return hip_fail(e, "jpeg huffman");
        uint32_t len = 0;
        rc = copy_d2h_2d(reinterpret_cast<uint8_t*>(&len), 4, dq + l_off, 4, 4, 1, s);
        if (rc) return rc;
        if (len == 0xffffffffu) {  // does not fit the GPU coder's buffer: host coder
            std::vector<int16_t> coef(jg.nmcu * 3 * 64);
            rc = copy_d2h_2d((uint8_t*)coef.data(), cbytes, (const uint8_t*)dcoef, cbytes, cbytes, 1, s);
            if (rc) return rc;
            jpeg_write(coef.data(), (int)w, (int)h, qt, out);
            jpeg_enc_count(false);
            return IK_OK;
        }
        jpeg_enc_count(true);
        std::vector<uint8_t> hdr;
        jpeg_header((int)w, (int)h, qt, hdr);
        uint8_t* at = jpeg_file(hdr, nullptr, len, out);  // the stream comes straight from the device
        return len ? copy_d2h_2d(at, len, dq + o_off, len, len, 1, s) : IK_OK;
    }
    if (fmt == IK_FORMAT_AVIF) {
        // image 0.25.8 AvifEncoder::new_with_speed_quality(out, 4, q) (src/transform.rs:140-145)
        const size_t n = (size_t)w * h;
        uint8_t* dp = scratch(4 * n + 256);
        if (!dp) return fail(IK_ERR_DEVICE, "cannot allocate device scratch");
        int* dflag = reinterpret_cast<int*>(dp + 4 * n + 128 - ((4 * n) & 127));
        hipError_t e = launch_avif_yuv444(dev, (int)w, (int)h, (int)c, pitch, 0, dp, 0, dflag, 1, s);
        if (e != hipSuccess) return hip_fail(e, "avif yuv444");
        p.planes.resize(4 * n);
        int transparent = 0;
        int rc = copy_d2h_2d(p.planes.data(), 4 * n, dp, 4 * n, 4 * n, 1, s);
        if (!rc) rc = copy_d2h_2d(reinterpret_cast<uint8_t*>(&transparent), 4, reinterpret_cast<const uint8_t*>(dflag), 4, 4, 1, s);
        if (rc) return rc;
        p.transparent = transparent != 0;
        p.done = false;  // AV1 coding by libavif: encode_host_back
        return IK_OK;
    }
    return fail(IK_ERR_INVALID, "unknown ImageFormat %d", fmt);
}

int encode_host_back(EncodePrep& p, std::vector<uint8_t>& out) {
    if (p.done) return IK_OK;
    p.done = true;
    if (p.fmt == IK_FORMAT_WEBP) {
        const size_t uvw = (p.w + 1) / 2, uvh = (p.h + 1) / 2;
        const uint8_t* Y = p.plane_data();
        return webp_encode_yuv420(Y, Y + (size_t)p.w * p.h, Y + (size_t)p.w * p.h + uvw * uvh, (int)p.w, (int)p.h,
                                  (float)p.q, out);
    }
    if (p.fmt == IK_FORMAT_AVIF) return avif_encode_yuv444(p.plane_data(), p.transparent, (int)p.w, (int)p.h, p.q, 4, out);
    return fail(IK_ERR_INVALID, "unknown ImageFormat %d", p.fmt);
}

int encode_device_image(const uint8_t* dev, uint32_t w, uint32_t h, uint32_t c, size_t pitch, int fmt, int quality,
                        std::vector<uint8_t>& out) {
    EncodePrep p;
    const int rc = encode_device_front(dev, w, h, c, pitch, fmt, quality, p, out);
    return rc ? rc : encode_host_back(p, out);
}

// the front half of ik_encode on a handle (u16 images are rescaled to u8 first,
// as to_rgb8 / to_rgba8 do)
int encode_image_front(const ik_image* img, int fmt, int quality, EncodePrep& p, std::vector<uint8_t>& out) {
    if (!img) return fail(IK_ERR_INVALID, "null pointer");
    if (img->w == 0 || img->h == 0) return fail(IK_ERR_TRANSFORM, "cannot encode an empty image");
    DeviceGuard g(img->device);
    if (img->depth != 2) return encode_device_front(img->d, img->w, img->h, img->c, img->pitch, fmt, quality, p, out);
    ik_image* u8 = nullptr;
    int st = alloc_image(img->w, img->h, img->c, &u8);
    if (st) return st;
    hipError_t e = launch_u16_to_u8(img->d, img->pitch, u8->d, u8->pitch, (int)(img->w * img->c), (int)img->h,
                                    thread_stream());
    st = e == hipSuccess ? encode_device_front(u8->d, u8->w, u8->h, u8->c, u8->pitch, fmt, quality, p, out)
                         : hip_fail(e, "u16 -> u8");
    if (e == hipSuccess && !st) (void)hipStreamSynchronize(thread_stream());  // u8 is read before it is freed
    ik_image_free(u8);
    return st;
}

// Page-locked blocks shared by the requests of a batched colour launch: a pool of
// free blocks (process-wide); a block goes back when its last holder drops it.
// Best fit (the smallest free block that holds the request, at most twice its
// size, so a small group does not take the block a large one needs), and at most
// kPinnedPoolBytes kept: a block returned past that goes back to the runtime.
namespace {
constexpr size_t kPinnedPoolBytes = size_t(2) << 30;
std::mutex g_pblk_mu;
std::multimap<size_t, uint8_t*> g_pblk_free;  // capacity -> block
size_t g_pblk_held = 0;
}  // namespace
static std::shared_ptr<uint8_t> pinned_block(size_t bytes) {
    uint8_t* p = nullptr;
    size_t cap = 0;
    {
        std::lock_guard<std::mutex> lk(g_pblk_mu);
        auto it = g_pblk_free.lower_bound(bytes);
        if (it != g_pblk_free.end() && it->first <= 2 * bytes) {
            cap = it->first;
            p = it->second;
            g_pblk_held -= cap;
            g_pblk_free.erase(it);
        }
    }
    if (!p) {
        cap = bytes;
        if (hipHostMalloc((void**)&p, cap, hipHostMallocDefault) != hipSuccess) return nullptr;
    }
    return std::shared_ptr<uint8_t>(p, [cap](uint8_t* q) {
        {
            std::lock_guard<std::mutex> lk(g_pblk_mu);
            if (g_pblk_held + cap <= kPinnedPoolBytes) {
                g_pblk_free.emplace(cap, q);
                g_pblk_held += cap;
                return;
            }
        }
        (void)hipHostFree(q);
    });
}

// The exact coder for a same-geometry group (IK_WEBP_EXACT): one batched colour launch
// into device memory, then the whole group through webp_encode_exact -- the files
// are final, no host coder runs.
int webp_exact_group(const std::vector<ik_image*>& imgs, int quality, std::vector<std::vector<uint8_t>*>& outs) {
    const size_t n = imgs.size();
    const ik_image* i0 = imgs[0];
    DeviceGuard g(i0->device);
    const DeviceConsts* dc = device_consts(current_device());
    if (!dc) return fail(IK_ERR_DEVICE, "cannot upload WebP tables");
    const uint32_t w = i0->w, h = i0->h;
    const size_t bytes = yuv420_bytes(w, h);
    const size_t stride = (bytes + 255) & ~size_t(255);
    hipStream_t s = thread_stream();
    uint8_t* dyuv = scratch(stride * n + 16 * n + 256);
    if (!dyuv) return fail(IK_ERR_DEVICE, "cannot allocate device scratch");
    std::vector<uint64_t> htab(n);
    for (size_t i = 0; i < n; ++i) htab[i] = (uint64_t)(uintptr_t)imgs[i]->d;
    uint64_t* dtab = reinterpret_cast<uint64_t*>(dyuv + stride * n);
    hipError_t e = hipMemcpyAsync(dtab, htab.data(), 8 * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = launch_webp_yuv420(nullptr, (int)w, (int)h, (int)i0->c, i0->pitch, 0, dyuv, stride, (int)n,
                               dc->gamma_to_lin, dc->lin_to_gamma, s, dtab);
    if (e != hipSuccess) return hip_fail(e, "webp yuv420 (exact group)");
    std::vector<std::vector<uint8_t>> files;
    const int q = clamp_quality(quality);
    if (int rc = webp_encode_exact(dyuv, stride, (int)n, (int)w, (int)h, q, files)) return rc;
    for (size_t i = 0; i < n; ++i) outs[i]->swap(files[i]);
    return IK_OK;
}

// The exact coder for a batch's WebP requests of mixed sizes and qualities
// (IK_WEBP_MIXED_GPU): one colour launch over a table of the images into device
// memory, then all of them through one webp_encode_exact_mixed call -- the files are
// final, no host coder runs.  8-bit images of at most 16383 x 16383 on one device.
int webp_exact_mixed_group(const std::vector<ik_image*>& imgs, const std::vector<int>& quality,
                           std::vector<std::vector<uint8_t>*>& outs) {
    const size_t n = imgs.size();
    DeviceGuard g(imgs[0]->device);
    const DeviceConsts* dc = device_consts(current_device());
    if (!dc) return fail(IK_ERR_DEVICE, "cannot upload WebP tables");
    hipStream_t s = thread_stream();
    if (!s) return fail(IK_ERR_DEVICE, "cannot create HIP stream");
    std::vector<size_t> at(n);
    size_t total = 0;
    int max_w = 0, max_h = 0;
    for (size_t i = 0; i < n; ++i) {
        const size_t w = imgs[i]->w, h = imgs[i]->h;
        at[i] = total;
        total += (yuv420_bytes(w, h) + 255) & ~size_t(255);
        max_w = std::max(max_w, (int)w);
        max_h = std::max(max_h, (int)h);
    }
    uint8_t* dyuv = scratch_slot(kScratchMixedPlanes, total + sizeof(WebpYuvItem) * n);
    WebpYuvItem* htab = reinterpret_cast<WebpYuvItem*>(pinned_slot(kPinnedMixedTab, sizeof(WebpYuvItem) * n));
    if (!dyuv || !htab) return fail(IK_ERR_DEVICE, "cannot allocate the mixed WebP planes");
    (void)hipStreamSynchronize(s);  // nothing pending reads the pinned table
    std::vector<ExactItem> items(n);
    for (size_t i = 0; i < n; ++i) {
        htab[i] = WebpYuvItem{imgs[i]->d, dyuv + at[i], imgs[i]->pitch, (int32_t)imgs[i]->w, (int32_t)imgs[i]->h,
                              (int32_t)imgs[i]->c, 0};
        items[i] = ExactItem{dyuv + at[i], (int)imgs[i]->w, (int)imgs[i]->h, clamp_quality(quality[i])};
    }
    WebpYuvItem* dtab = reinterpret_cast<WebpYuvItem*>(dyuv + total);
    hipError_t e = hipMemcpyAsync(dtab, htab, sizeof(WebpYuvItem) * n, hipMemcpyHostToDevice, s);
    if (e == hipSuccess)
        e = launch_webp_yuv420_items(dtab, (int)n, max_w, max_h, dc->gamma_to_lin, dc->lin_to_gamma, s);
    if (e != hipSuccess) return hip_fail(e, "webp yuv420 (mixed group)");
    std::vector<std::vector<uint8_t>> files;
    if (int rc = webp_encode_exact_mixed(items.data(), (int)n, files)) return rc;
    for (size_t i = 0; i < n; ++i) outs[i]->swap(files[i]);
    return IK_OK;
}

// encode_image's device front end for n same-geometry 8-bit images going to WebP
// through libwebp: ONE colour-conversion launch over per-image base pointers,
// writing every image's YUV420 planes straight into pinned host memory; prep[i]
// gets the planes for encode_host_back.  Returns IK_ERR_UNSUPPORTED (nothing
// done) when the per-image path applies instead (the GPU VP8 encoder, > 16383).
int webp_front_group(const std::vector<ik_image*>& imgs, int quality, std::vector<EncodePrep*>& prep) {
    const size_t n = imgs.size();
    if (!n) return IK_OK;
    const ik_image* i0 = imgs[0];
    if (i0->w > 16383 || i0->h > 16383 || i0->depth != 1)  // (the caller chose the libwebp coder)
        return IK_ERR_UNSUPPORTED;
    DeviceGuard g(i0->device);
    const DeviceConsts* dc = device_consts(current_device());
    if (!dc) return fail(IK_ERR_DEVICE, "cannot upload WebP tables");
    const uint32_t w = i0->w, h = i0->h;
    const size_t bytes = yuv420_bytes(w, h);
    const size_t stride = (bytes + 255) & ~size_t(255);
    std::shared_ptr<uint8_t> blk = pinned_block(stride * n + 16 * n + 256);
    uint8_t* hp = blk.get();
    void* dhp = nullptr;
    if (!hp || hipHostGetDevicePointer(&dhp, hp, 0) != hipSuccess || !dhp)
        return fail(IK_ERR_NOMEM, "cannot map pinned WebP planes");
    uint64_t* dtab = reinterpret_cast<uint64_t*>(scratch_slot(kScratchPtrTable, sizeof(uint64_t) * n));
    if (!dtab) return fail(IK_ERR_DEVICE, "cannot allocate device scratch");
    hipStream_t s = thread_stream();
    (void)hipStreamSynchronize(s);  // nothing pending reads the pinned area
    uint64_t* htab = reinterpret_cast<uint64_t*>(hp + stride * n);
    for (size_t i = 0; i < n; ++i) htab[i] = (uint64_t)(uintptr_t)imgs[i]->d;
    hipError_t e = launch_copy_words(reinterpret_cast<const uint32_t*>(reinterpret_cast<uint8_t*>(dhp) + stride * n),
                                     reinterpret_cast<uint32_t*>(dtab), 2 * n, s);
    if (e == hipSuccess)
        e = launch_webp_yuv420(nullptr, (int)w, (int)h, (int)i0->c, i0->pitch, 0, reinterpret_cast<uint8_t*>(dhp), stride,
                               (int)n, dc->gamma_to_lin, dc->lin_to_gamma, s, dtab);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return hip_fail(e, "webp yuv420 (batched)");
    const int q = clamp_quality(quality);
    for (size_t i = 0; i < n; ++i) {
        EncodePrep& p = *prep[i];
        p.fmt = IK_FORMAT_WEBP;
        p.q = q;
        p.w = w;
        p.h = h;
        p.pin_block = blk;
        p.pin_planes = hp + stride * i;
        p.done = false;
    }
    return IK_OK;
}

// encode_image's JPEG branch for a group of same-size 8-bit images (one quality),
// batched: one coefficient launch (to_rgb8 + YCbCr + FDCT + quantise) and one
// Huffman launch over all of them, writing the stuffed streams and their lengths
// straight into pinned host memory -- instead of a launch pair and two blocking
// copies per image, which serialised 256 small launches per configs[2] batch.
// Images whose stream does not fit the GPU coder's buffer are coded by the
// single-image path (its host fallback).  out[i] gets the finished JPEG bytes.
int jpeg_front_group(const std::vector<ik_image*>& imgs, int quality, std::vector<std::vector<uint8_t>*>& out) {
    const size_t n = imgs.size();
    if (!n) return IK_OK;
    const ik_image* i0 = imgs[0];
    if (i0->w > 65535 || i0->h > 65535 || i0->depth != 1) return IK_ERR_UNSUPPORTED;
    DeviceGuard g(i0->device);
    const DeviceConsts* dc = device_consts(current_device());
    if (!dc) return fail(IK_ERR_DEVICE, "cannot upload JPEG tables");
    const int q = clamp_quality(quality);
    const uint32_t w = i0->w, h = i0->h;
    uint8_t qt[128];
    jpeg_quant_tables(q, qt);
    std::vector<uint8_t> hdr;
    jpeg_header((int)w, (int)h, qt, hdr);
    const JpegEncGeom jg = jpeg_enc_geom(w, h);
    const size_t cimg = (jg.coef_bytes + 255) & ~size_t(255);  // coefficients per image
    const size_t cap = jg.cap;
    hipStream_t s = thread_stream();
    // sub-batches bound the device and pinned memory (2 cap + coefficients per image)
    constexpr size_t kSub = 64;
    for (size_t b0 = 0; b0 < n; b0 += kSub) {
        const size_t m = std::min(kSub, n - b0);
        // device: [qt 256][src table][coefficients][Huffman work]; pinned: [streams][lengths][qt + table staging]
        const size_t o_tab = 256, o_coef = o_tab + ((sizeof(uint64_t) * m + 255) & ~size_t(255));
        const size_t o_work = o_coef + cimg * m;
        uint8_t* dv = scratch_slot(kScratchJpegGroup, o_work + jg.work_bytes * m);
        const size_t p_len = cap * m, p_stage = p_len + ((sizeof(uint32_t) * m + 255) & ~size_t(255));
        uint8_t* hp = pinned_slot(kPinnedGroupStage, p_stage + 256 + sizeof(uint64_t) * m);
        void* dhp = nullptr;
        if (!dv || !hp || hipHostGetDevicePointer(&dhp, hp, 0) != hipSuccess || !dhp)
            return fail(IK_ERR_NOMEM, "cannot allocate the batched JPEG encoder's buffers");
        uint8_t* dh = reinterpret_cast<uint8_t*>(dhp);
        (void)hipStreamSynchronize(s);  // nothing pending reads the pinned area
        std::memcpy(hp + p_stage, qt, 128);
        uint64_t* htab = reinterpret_cast<uint64_t*>(hp + p_stage + 256);
        for (size_t i = 0; i < m; ++i) htab[i] = (uint64_t)(uintptr_t)imgs[b0 + i]->d;
        EvPair& ev = thread_events(kEvJpegGroup);
        hipError_t e = launch_copy_words(reinterpret_cast<const uint32_t*>(dh + p_stage), reinterpret_cast<uint32_t*>(dv),
                                         32, s);
        if (e == hipSuccess) ev_record(ev.a, s);
        if (e == hipSuccess)
            e = launch_copy_words(reinterpret_cast<const uint32_t*>(dh + p_stage + 256),
                                  reinterpret_cast<uint32_t*>(dv + o_tab), 2 * m, s);
        if (e == hipSuccess)
            e = launch_jpeg_coeffs(nullptr, (int)w, (int)h, (int)i0->c, i0->pitch, 0, dv,
                                   reinterpret_cast<int16_t*>(dv + o_coef), cimg / sizeof(int16_t), (int)m, s,
                                   reinterpret_cast<const uint64_t*>(dv + o_tab));
        if (e == hipSuccess)
            e = launch_jpeg_huff_enc(jg.args(reinterpret_cast<const int16_t*>(dv + o_coef), cimg / sizeof(int16_t),
                                             dc->jpeg_huff, dv + o_work, dh, reinterpret_cast<uint32_t*>(dh + p_len)),
                                     (int)m, s);
        if (e == hipSuccess) ev_record(ev.b, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return hip_fail(e, "jpeg encode (batched)");
        batch_timing_add(current_device(), kBtJpegEncMs, ev_pair_ms(ev));
        batch_timing_add(current_device(), kBtJpegEncImages, (double)m);
        const uint32_t* lens = reinterpret_cast<const uint32_t*>(hp + p_len);
        for (size_t i = 0; i < m; ++i) {
            std::vector<uint8_t>& o = *out[b0 + i];
            if (lens[i] == 0xffffffffu) {  // past the GPU coder's buffer: the single-image path (host coder, counted there)
                EncodePrep pp;
                if (int rc = encode_device_front(imgs[b0 + i]->d, w, h, i0->c, i0->pitch, IK_FORMAT_JPEG, q, pp, o))
                    return rc;
                continue;
            }
            jpeg_enc_count(true);
            jpeg_file(hdr, hp + cap * i, lens[i], o);
        }
    }
    return IK_OK;
}

// imageops::resize over n 8-bit images of one geometry (same W, H, C, pitch) in
// ONE fused launch: the kernel reads each image's base pointer from a table, so
// the images may sit anywhere.  Same arithmetic as ik_resize_window, per image.
// Returns IK_ERR_UNSUPPORTED (nothing allocated) when the geometry needs the
// two-kernel fallback; the caller then resizes image by image.
int resize_group(const std::vector<ik_image*>& src, const FitWindow& win, int filter, std::vector<ik_image*>& out) {
    const size_t n = src.size();
    const uint32_t nw = win.nw, nh = win.nh;
    out.assign(n, nullptr);
    if (!n) return IK_OK;
    const ik_image* s0 = src[0];
    DeviceGuard g(s0->device);
    if (!resize_window_ok(win.iw, win.ih, win.x0, win.y0, win.nw, win.nh)) return IK_ERR_UNSUPPORTED;
    ResizePlan* plan = get_resize_plan_window(current_device(), (int)s0->w, (int)s0->h, (int)s0->c, (int)win.iw,
                                              (int)win.ih, (int)win.x0, (int)win.y0, (int)nw, (int)nh, filter, (int)n);
    if (!plan) return fail(IK_ERR_DEVICE, "cannot build resize plan");
    if (plan->slots == 0 || !resize_fused_fits(s0->pitch, s0->h) || (s0->pitch & 7)) return IK_ERR_UNSUPPORTED;
    std::vector<uint64_t> tab(2 * n);
    for (size_t i = 0; i < n; ++i) {
        const int st = alloc_image(nw, nh, s0->c, &out[i]);
        if (st) {
            for (ik_image*& o : out) { ik_image_free(o); o = nullptr; }
            return st;
        }
        tab[i] = (uint64_t)(uintptr_t)src[i]->d;
        tab[n + i] = (uint64_t)(uintptr_t)out[i]->d;
    }
    hipStream_t s = thread_stream();
    uint64_t* dtab = reinterpret_cast<uint64_t*>(scratch_slot(kScratchPtrTable, sizeof(uint64_t) * 2 * n));
    // the pointer table goes up through a copy kernel reading pinned memory (a
    // copy-engine transfer would queue behind another batch's stream upload)
    uint8_t* ht = pinned_slot(kPinnedGroupStage, 16 * n);
    void* dht = nullptr;
    int rc = IK_OK;
    if (!dtab) rc = fail(IK_ERR_DEVICE, "cannot allocate device scratch");
    else if (!ht || hipHostGetDevicePointer(&dht, ht, 0) != hipSuccess || !dht)
        rc = fail(IK_ERR_NOMEM, "cannot map pinned resize table");
    if (!rc) {
        (void)hipStreamSynchronize(s);  // the previous table is read
        std::memcpy(ht, tab.data(), 16 * n);
        const hipError_t e = launch_copy_words(reinterpret_cast<const uint32_t*>(dht), reinterpret_cast<uint32_t*>(dtab),
                                               4 * n, s);
        if (e != hipSuccess) rc = hip_fail(e, "resize table upload");
    }
    if (!rc) {
        EvPair& ev = thread_events(kEvResize);
        ev_record(ev.a, s);
        hipError_t e = launch_resize(*plan, nullptr, s0->pitch, 0, nullptr, out[0]->pitch, 0, (int)n, nullptr, s, dtab,
                                     dtab + n);
        if (e == hipSuccess) ev_record(ev.b, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = hip_fail(e, "resize (batched)");
        if (!rc) {
            const int d = current_device();
            batch_timing_add(d, kBtResizeMs, ev_pair_ms(ev));
            batch_timing_add(d, kBtResizeBytes, (double)n * s0->c * ((double)s0->w * s0->h + (double)nw * nh));
            batch_timing_add(d, kBtResizeImages, (double)n);
        }
    }
    if (rc)
        for (ik_image*& o : out) { ik_image_free(o); o = nullptr; }
    return rc;
}

// apply_orientation (2..8) over n images of one geometry (same W, H, C, depth, pitch) in
// ONE launch, as resize_group: new images, the kernel reads the bases from a table.
// Returns IK_ERR_UNSUPPORTED (nothing allocated) when a base is not 4-byte aligned (a
// wrapped caller buffer); the caller then turns image by image.
int orient_group(const std::vector<ik_image*>& src, int orientation, std::vector<ik_image*>& out) {
    const size_t n = src.size();
    out.assign(n, nullptr);
    if (!n) return IK_OK;
    const ik_image* s0 = src[0];
    if (n > kOrientMaxImages || !s0->w || !s0->h) return IK_ERR_UNSUPPORTED;
    for (const ik_image* im : src)
        if ((uintptr_t)im->d & 3) return IK_ERR_UNSUPPORTED;
    DeviceGuard g(s0->device);
    const bool t = orientation >= 5;
    std::vector<uint64_t> tab(2 * n);
    for (size_t i = 0; i < n; ++i) {
        const int st = alloc_image(t ? s0->h : s0->w, t ? s0->w : s0->h, s0->c, &out[i], s0->depth);
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
        rc = fail(IK_ERR_NOMEM, "cannot map pinned orientation table");
    if (!rc) {
        (void)hipStreamSynchronize(s);  // the previous table is read
        std::memcpy(ht, tab.data(), 16 * n);
        hipError_t e = launch_copy_words(reinterpret_cast<const uint32_t*>(dht), reinterpret_cast<uint32_t*>(dtab), 4 * n, s);
        if (e == hipSuccess)
            e = launch_orient(nullptr, s0->pitch, 0, nullptr, out[0]->pitch, 0, s0->w, s0->h, (int)(s0->c * s0->depth),
                              orientation, (int)n, s, dtab, dtab + n);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = hip_fail(e, "orientation (batched)");
    }
    if (rc)
        for (ik_image*& o : out) { ik_image_free(o); o = nullptr; }
    return rc;
}

// the background flatten over n images of one geometry (same W, H, C, depth, pitch; C is 2
// or 4) onto one colour in ONE launch, as orient_group: new images of
// flatten_out_channels(C, rgb) channels, the kernel reads the bases from a table.
int flatten_group(const std::vector<ik_image*>& src, uint32_t rgb, std::vector<ik_image*>& out) {
    const size_t n = src.size();
    out.assign(n, nullptr);
    if (!n) return IK_OK;
    const ik_image* s0 = src[0];
    if (n > kFlattenMaxImages || !s0->w || !s0->h || (s0->c != 2 && s0->c != 4)) return IK_ERR_UNSUPPORTED;
    for (const ik_image* im : src)
        if ((uintptr_t)im->d & 3) return IK_ERR_UNSUPPORTED;
    DeviceGuard g(s0->device);
    const uint32_t oc = flatten_out_channels(s0->c, rgb);
    std::vector<uint64_t> tab(2 * n);
    for (size_t i = 0; i < n; ++i) {
        const int st = alloc_image(s0->w, s0->h, oc, &out[i], s0->depth);
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
        rc = fail(IK_ERR_NOMEM, "cannot map pinned flatten table");
    if (!rc) {
        (void)hipStreamSynchronize(s);  // the previous table is read
        std::memcpy(ht, tab.data(), 16 * n);
        hipError_t e = launch_copy_words(reinterpret_cast<const uint32_t*>(dht), reinterpret_cast<uint32_t*>(dtab), 4 * n, s);
        if (e == hipSuccess)
            e = launch_flatten(nullptr, s0->pitch, 0, nullptr, out[0]->pitch, 0, s0->w, s0->h, (int)s0->c, (int)oc,
                               (int)s0->depth, rgb, (int)n, s, dtab, dtab + n);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) rc = hip_fail(e, "background flatten (batched)");
        else flatten_count(1, n);
    }
    if (rc)
        for (ik_image*& o : out) { ik_image_free(o); o = nullptr; }
    return rc;
}

// ik_shutdown: the batched colour launches' pinned blocks, the per-device constant tables
void encode_shutdown() {
    {
        std::lock_guard<std::mutex> lk(g_pblk_mu);
        for (auto& b : g_pblk_free) (void)hipHostFree(b.second);
        g_pblk_free.clear();
        g_pblk_held = 0;
    }
    std::lock_guard<std::mutex> lk(g_consts_mu);
    for (auto& kv : g_consts) {
        (void)hipSetDevice(kv.first);
        (void)hipFree(kv.second->gamma_to_lin);
        (void)hipFree(kv.second->lin_to_gamma);
        (void)hipFree(kv.second->jpeg_huff);
        delete kv.second;
    }
    g_consts.clear();
}

}  // namespace ik

using namespace ik;

extern "C" {

int ik_jpeg_enc_counters(unsigned long long* out) {
    if (!out) return fail(IK_ERR_INVALID, "null pointer");
    out[0] = g_jpeg_enc_gpu.load();
    out[1] = g_jpeg_enc_host.load();
    return IK_OK;
}

}  // extern "C"
