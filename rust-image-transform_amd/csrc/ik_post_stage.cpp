// ik_post_stage.cpp -- what a request's options mean and where they run: the entry points'
// option arguments as one record per request (RequestOps), the batch paths' post stage
// (orient -> flatten -> resize -> adjust -> filter -> pad -> watermark -> the encoders' device front ends) and
// the single-request path through the same steps (transform_here).
#include <hip/hip_runtime.h>

#include <array>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <tuple>

#include "../../include/imagekit_hip.h"
#include "ik_exif.h"
#include "ik_runtime.h"

namespace ik {

// ---- per-request options (ik_request_opts, ik_request_opts2, ik_request_opts3, ik_request_opts4, ik_request_opts5) ----
bool opts_size_ok(size_t opt_size) {
    return opt_size == sizeof(ik_request_opts) || opt_size == sizeof(ik_request_opts2) ||
           opt_size == sizeof(ik_request_opts3) || opt_size == sizeof(ik_request_opts4) ||
           opt_size == sizeof(ik_request_opts5);
}
// request i of an options array whose structs lie opt_size bytes apart, as the largest
// layout (a smaller one's new fields: zero, "off")
static ik_request_opts5 opts_at(const void* opts, size_t opt_size, uint32_t i) {
    ik_request_opts5 o{};
    std::memcpy(&o, static_cast<const uint8_t*>(opts) + (size_t)i * opt_size, opt_size);
    return o;
}
// the blur or unsharpen an options struct asks for.  Returns IK_OK, or IK_ERR_INVALID with
// the message set (prefix: "" or "request i: ")
static int filter_of(const ik_request_opts5& o, const char* prefix, FilterReq& f) {
    f = FilterReq();
    // (written so that a NaN fails)
    const bool bs = o.blur_sigma == 0.0f || (o.blur_sigma >= 0.0625f && o.blur_sigma <= IK_BLUR_MAX_SIGMA);
    const bool ss = o.sharpen_sigma == 0.0f || (o.sharpen_sigma >= 0.0625f && o.sharpen_sigma <= IK_BLUR_MAX_SIGMA);
    if (!bs)
        return fail(IK_ERR_INVALID, "%sblur sigma %g is neither 0 nor in 0.0625..%g", prefix, (double)o.blur_sigma,
                    (double)IK_BLUR_MAX_SIGMA);
    if (!ss)
        return fail(IK_ERR_INVALID, "%ssharpen sigma %g is neither 0 nor in 0.0625..%g", prefix, (double)o.sharpen_sigma,
                    (double)IK_BLUR_MAX_SIGMA);
    if (!blur_threshold_ok(o.sharpen_threshold))
        return fail(IK_ERR_INVALID, "%ssharpen threshold %d outside 0..65535", prefix, (int)o.sharpen_threshold);
    if (o.blur_sigma != 0.0f && o.sharpen_sigma != 0.0f) return fail(IK_ERR_INVALID, "%sblur and sharpen together", prefix);
    if (o.blur_sigma != 0.0f) { f.mode = 1; f.sigma = o.blur_sigma; }
    else if (o.sharpen_sigma != 0.0f) { f.mode = 2; f.sigma = o.sharpen_sigma; f.threshold = o.sharpen_threshold; }
    return IK_OK;
}
// the watermark an options struct asks for (r.mark null: none), checked as filter_of checks
static int overlay_of(const ik_request_opts5& o, const char* prefix, OverlayReq& r) {
    r = OverlayReq();
    if (o.reserved != 0) return fail(IK_ERR_INVALID, "%sreserved options field is %d, not 0", prefix, (int)o.reserved);
    if (int rc = overlay_check(o.overlay_gravity, o.overlay_dx, o.overlay_dy, o.overlay_opacity, 0, o.overlay_tile, prefix))
        return rc;
    if (!o.overlay) {
        if (o.overlay_gravity || o.overlay_dx || o.overlay_dy || o.overlay_opacity || o.overlay_tile)
            return fail(IK_ERR_INVALID, "%soverlay fields set without an overlay", prefix);
        return IK_OK;
    }
    r.mark = o.overlay;
    r.gravity = o.overlay_gravity; r.dx = o.overlay_dx; r.dy = o.overlay_dy;
    r.opacity = o.overlay_opacity ? o.overlay_opacity : 255;
    r.tile = o.overlay_tile;
    return IK_OK;
}
// the colour adjustment an options struct asks for (all zero: none), checked as filter_of checks
static int adjust_of(const ik_request_opts5& o, const char* prefix, AdjustReq& r) {
    r = AdjustReq();
    if (int rc = adjust_check(o.adjust, prefix)) return rc;
    r.a = o.adjust;
    return IK_OK;
}
// the pad an options struct asks for (mode 0: none, and then every field 0), checked as filter_of checks
static int pad_of(const ik_request_opts5& o, const char* prefix, PadReq& r) {
    r = PadReq();
    if (int rc = pad_check(o.pad, prefix, true)) return rc;
    r.p = o.pad;
    return IK_OK;
}
static int background_of(const ik_request_opts5& o, const char* prefix, int32_t& bg) {
    bg = o.background;
    if (bg == IK_BG_NONE || (bg >= 0 && bg <= 0xFFFFFF)) return IK_OK;
    return fail(IK_ERR_INVALID, "%sbackground %d is neither IK_BG_NONE nor 0x000000..0xFFFFFF", prefix, (int)bg);
}

int effective_orientation(const uint8_t* bytes, size_t len, int orient) {
    if (orient < IK_ORIENT_AUTO || orient > 8) return -1;
    const int o = orient == IK_ORIENT_AUTO ? exif_orientation(bytes, len) : orient;
    return o <= 1 ? 0 : o;
}
// the same with its refusal's message.  bytes null (device-resident inputs): the caller has
// refused IK_ORIENT_AUTO.  Only AUTO reads the file: an all-STORED batch stays off the files.
static int orientation_of(int orient, const uint8_t* bytes, size_t len, const char* prefix, int& eff) {
    eff = effective_orientation(bytes, len, orient);
    if (eff < 0) return fail(IK_ERR_INVALID, "%sunknown orientation %d", prefix, orient);
    return IK_OK;
}

int request_ops(const int* fit, const int* orient, const void* opts, size_t opt_size, uint32_t n,
                const uint8_t* const* bytes, const size_t* lens, std::vector<RequestOps>& ops) {
    ops.clear();
    if (!fit && !orient && !opts) return IK_OK;
    ops.assign(n, RequestOps());
    bool any = false;
    for (uint32_t i = 0; i < n; ++i) {
        ik_request_opts5 o{};
        o.background = IK_BG_NONE;
        if (opts) o = opts_at(opts, opt_size, i);
        if (fit) o.fit = fit[i];
        if (orient) o.orient = orient[i];
        char prefix[32];
        snprintf(prefix, sizeof prefix, "request %u: ", i);
        RequestOps& r = ops[i];
        if (o.fit < IK_FIT_CONTAIN || o.fit > IK_FIT_EXACT) return fail(IK_ERR_INVALID, "%sunknown fit %d", prefix, o.fit);
        r.fit = o.fit;
        if (int rc = background_of(o, prefix, r.bg)) return rc;
        if (o.orient == IK_ORIENT_AUTO && !bytes)
            return fail(IK_ERR_INVALID, "%sIK_ORIENT_AUTO cannot be resolved for device-resident inputs", prefix);
        if (int rc = orientation_of(o.orient, bytes ? bytes[i] : nullptr, lens[i], prefix, r.orient)) return rc;
        if (int rc = filter_of(o, prefix, r.flt)) return rc;
        if (int rc = overlay_of(o, prefix, r.ovl)) return rc;
        if (int rc = adjust_of(o, prefix, r.adj)) return rc;
        if (int rc = pad_of(o, prefix, r.pad)) return rc;
        any = any || !r.is_default();
    }
    if (!any) ops.clear();
    return IK_OK;
}

int single_request_ops(int fit, int orient, const void* opts, size_t opt_size, const uint8_t* bytes, size_t len,
                       RequestOps& r) {
    r = RequestOps();
    ik_request_opts5 o{};
    o.fit = fit; o.orient = orient; o.background = IK_BG_NONE;
    if (opts) o = opts_at(opts, opt_size, 0);
    r.fit = o.fit;  // (not checked here: ik_resize_fit refuses an unknown one, after the decode)
    if (int rc = background_of(o, "", r.bg)) return rc;
    if (int rc = filter_of(o, "", r.flt)) return rc;
    if (int rc = overlay_of(o, "", r.ovl)) return rc;
    if (int rc = adjust_of(o, "", r.adj)) return rc;
    if (int rc = pad_of(o, "", r.pad)) return rc;
    return orientation_of(o.orient, bytes, len, "", r.orient);
}

// ---- the steps themselves ----
static int filter_image(ik_image* img, const FilterReq& f, ik_image** out) {
    return f.mode == 2 ? ik_image_unsharpen(img, f.sigma, f.threshold, out) : ik_image_blur(img, f.sigma, out);
}

// resize_image, then the request's colour adjustment (in place), then its blur or unsharpen (the filter sees the pixels the encoder
// will code), then its pad (a new image: the canvas), then its watermark, on one image: what follows the flatten for a single request
// and for a batch's member that no resize group took.  *rs is the image to encode: a new one,
// or, with w and h both None and neither filter nor pad, img itself -- the caller owns img, so the
// watermark in place is still right.  On failure *rs is null and img is all the caller holds.
static int image_tail(ik_image* img, int64_t w, int64_t h, const RequestOps& ops, int filter, ik_image** rs) {
    *rs = nullptr;
    ik_image* cur = nullptr;
    int st = ik_resize_fit(img, w, h, ops.fit, filter, &cur);
    if (st) return st;
    if (ops.adj.on() && (st = adjust_image(cur, ops.adj)) != IK_OK) {
        if (cur != img) ik_image_free(cur);
        return st;
    }
    if (ops.flt.mode) {
        ik_image* fo = nullptr;
        st = filter_image(cur, ops.flt, &fo);
        if (cur != img) ik_image_free(cur);
        if (st) return st;
        cur = fo;
    }
    if (ops.pad.on()) {
        // (w, h and the target refer to img, the image the resize saw)
        const PadGeom g = pad_canvas(ops.pad.geometry(), img->w, img->h, w, h, cur->w, cur->h);
        if (g.cw != cur->w || g.ch != cur->h) {  // (a canvas that is the image: no pass)
            ik_image* po = nullptr;
            st = pad_image(cur, ops.pad, g, &po);
            if (cur != img) ik_image_free(cur);
            if (st) return st;
            cur = po;
        }
    }
    if (ops.ovl.mark && (st = overlay_image(cur, ops.ovl)) != IK_OK) {
        if (cur != img) ik_image_free(cur);
        return st;
    }
    *rs = cur;
    return IK_OK;
}

int transform_here(const uint8_t* bytes, size_t len, int64_t w, int64_t h, const RequestOps& ops, int fmt, int quality,
                   int filter, uint8_t** out, size_t* out_len) {
    ik_image* img = nullptr;
    int st = decode_one(bytes, len, &img, nullptr);
    if (st) return st;
    if (ops.orient) {
        ik_image* turned = nullptr;
        st = ik_image_orient(img, ops.orient, &turned);
        ik_image_free(img);
        if (st) return st;
        img = turned;
    }
    if (ops.bg != IK_BG_NONE && (img->c == 2 || img->c == 4)) {  // (no alpha: no pass, no copy)
        ik_image* flat = nullptr;
        st = ik_image_flatten(img, ops.bg, &flat);
        ik_image_free(img);
        if (st) return st;
        img = flat;
    }
    ik_image* rs = nullptr;
    st = image_tail(img, w, h, ops, filter, &rs);
    if (!st) st = ik_encode(rs, fmt, quality, out, out_len);
    if (rs && rs != img) ik_image_free(rs);
    ik_image_free(img);
    return st;
}

// One "sets" step of the post stage over the images in slot (by member).  sets: the members
// that share the step's key, by key.  A set of two or more goes through one launch, group(k0,
// src, out) with k0 its first member (they all ask for the same); a set of one, or a set whose
// group call did not return IK_OK, goes member by member through each(k, image, &out), and a
// member that fails there gets its status and message.  A member's new image takes its place
// in slot and the old one returns to the pool (a step in place hands back the image it was
// given: nothing moves).  drop_failed: a member that failed loses its image (its slot is
// null); else it keeps the one it had.
template <class Key, class Group, class Each>
static void run_sets(const std::map<Key, std::vector<uint32_t>>& sets, std::vector<ik_image*>& slot, bool drop_failed,
                     std::vector<int>& ds, std::vector<std::string>& dm, Group group, Each each) {
    for (const auto& kv : sets) {
        const std::vector<uint32_t>& ks = kv.second;
        std::vector<ik_image*> src, out(ks.size(), nullptr);
        for (uint32_t k : ks) src.push_back(slot[k]);
        const bool grouped = ks.size() > 1 && group(ks[0], src, out) == IK_OK;
        for (size_t j = 0; j < ks.size(); ++j) {
            const uint32_t k = ks[j];
            if (!grouped) {
                if (int r = each(k, slot[k], &out[j])) {
                    ds[k] = r;
                    dm[k] = last_error_str();
                    if (!drop_failed) continue;
                    out[j] = nullptr;
                }
            }
            if (out[j] == slot[k]) continue;
            ik_image_free(slot[k]);
            slot[k] = out[j];
        }
    }
}

// Device half, post stage: resize, the encoders' device front ends (under the
// post gate, so a batch's resize runs beside the next batch's decode kernels);
// request i's status / message land in st[i] / errs[i]
// ops: null (every request at its defaults), or each request's options
void transform_post_phase(const int64_t* w, const int64_t* h, const RequestOps* ops, const int* fmt, const int* quality,
                          int filter, int* st, std::string* errs, HostPhase& hp) {
    const std::vector<uint32_t>& idx = hp.idx;
    const int threads = hp.threads;
    const uint32_t m = (uint32_t)idx.size();
    if (!m) return;
    std::vector<ik_image*>& imgs = hp.imgs;
    std::vector<int>& ds = hp.ds;
    std::vector<std::string>& dm = hp.dm;
    static const bool timing = getenv("IK_TIMING") != nullptr;
    static const RequestOps defaults;
    auto op = [&](uint32_t k) -> const RequestOps& { return ops ? ops[idx[k]] : defaults; };
    gate_pin(kGatePost, true);
    gate_enter(kGatePost);
    batch_timing_reset(current_device(), true);
    BatchTimingScope bts;
    std::mutex tmu;
    double& t_resize = hp.t_resize;
    double& t_front = hp.t_front;
    hp.prep.assign(m, EncodePrep());
    hp.bytes_out.assign(m, std::vector<uint8_t>());
    std::vector<EncodePrep>& prep = hp.prep;
    std::vector<std::vector<uint8_t>>& bytes_out = hp.bytes_out;
    if (ops) {
        // apply_orientation first, on the device that holds each decoded image: the post plan
        // below sees the oriented W, H and pitch.  Images of one (W, H, C, depth, pitch, device,
        // orientation) go through one launch, a lone one through its own; the stored-order
        // image returns to the pool once it has been turned.
        // Then the background flatten of the images that carry alpha, so that the post plan sees
        // the flattened C and pitch: images of one (W, H, C, depth, pitch, device, colour) go
        // through one launch (the output channels follow from C and the colour), a lone one
        // through its own; an image without alpha, or a request without a background, is not
        // touched.
        typedef std::array<uint64_t, 7> GeomKey;
        auto geom_sets = [&](bool flatten) {
            std::map<GeomKey, std::vector<uint32_t>> sets;
            for (uint32_t k = 0; k < m; ++k) {
                const ik_image* im = imgs[k];
                if (ds[k] || !im) continue;
                const RequestOps& r = op(k);
                if (flatten ? r.bg == IK_BG_NONE || (im->c != 2 && im->c != 4) : !r.orient) continue;
                sets[{im->w, im->h, im->c, im->depth, im->pitch, (uint64_t)im->device,
                      flatten ? (uint64_t)(uint32_t)r.bg : (uint64_t)r.orient}].push_back(k);
            }
            return sets;
        };
        run_sets(geom_sets(false), imgs, true, ds, dm,
                 [&](uint32_t k0, const std::vector<ik_image*>& src, std::vector<ik_image*>& out) {
                     return orient_group(src, op(k0).orient, out);
                 },
                 [&](uint32_t k, ik_image* im, ik_image** out) { return ik_image_orient(im, op(k).orient, out); });
        run_sets(geom_sets(true), imgs, true, ds, dm,
                 [&](uint32_t k0, const std::vector<ik_image*>& src, std::vector<ik_image*>& out) {
                     return flatten_group(src, (uint32_t)op(k0).bg, out);
                 },
                 [&](uint32_t k, ik_image* im, ik_image** out) { return ik_image_flatten(im, op(k).bg, out); });
    }
    // which launch resizes each request and which coder writes its file: ik_post_plan.h
    // (the encoder setting and the mixed mode are read once for the batch)
    std::vector<PostRequest> rq(m);
    for (uint32_t k = 0; k < m; ++k) {
        const uint32_t i = idx[k];
        const ik_image* im = imgs[k];
        rq[k].ok = !ds[k] && im;
        if (rq[k].ok) {
            rq[k].W = im->w; rq[k].H = im->h; rq[k].C = im->c;
            rq[k].pitch = im->pitch; rq[k].device = im->device; rq[k].depth = im->depth;
        }
        rq[k].w = w[i]; rq[k].h = h[i]; rq[k].fmt = fmt[i]; rq[k].quality = quality[i];
        rq[k].fit = op(k).fit;
        rq[k].pad = op(k).pad.geometry();
    }
    const PostPlan plan = post_plan(rq.data(), m, default_webp_encoder(), webp_mixed_mode());
    std::vector<ik_image*> rsz(m, nullptr);   // resized by its group's launch
    std::vector<char> fronted(m, 0);          // encode front end already run by its group's call
    std::vector<ik_image*> kept(m, nullptr);  // resized image kept for the mixed exact call
    const auto tg0 = std::chrono::steady_clock::now();
    for (const PostPlan::ResizeGroup& G : plan.rgroups) {
        std::vector<ik_image*> src, out;
        for (uint32_t k : G.members) src.push_back(imgs[k]);
        if (resize_group(src, G.win, filter, out) != IK_OK) continue;  // its members: image by image below
        for (size_t j = 0; j < out.size(); ++j) rsz[G.members[j]] = out[j];
        if (ops) {
            // the colour adjustment first, in place on the resized images: the members that
            // share the 24 adjustment bytes go through one launch, a lone one or a failed group
            // through launches of their own.  A member whose adjustment fails gets its status
            // and message: its file is dropped, and the later steps pass it by.
            std::map<AdjustReq::Key, std::vector<uint32_t>> adjs;
            for (uint32_t k : G.members)
                if (op(k).adj.on()) adjs[op(k).adj.key()].push_back(k);
            run_sets(adjs, rsz, false, ds, dm,
                     [&](uint32_t k0, const std::vector<ik_image*>& bs, std::vector<ik_image*>& done) {
                         done = bs;
                         return adjust_group(bs, op(k0).adj);
                     },
                     [&](uint32_t k, ik_image* im, ik_image** done) {
                         *done = im;
                         return adjust_image(im, op(k).adj);
                     });
            // blur or unsharpen before the group's coders run: the members that share (mode,
            // sigma, threshold) go through one launch, a lone one through its own, and the
            // unfiltered image returns to the pool.  A member whose filter fails keeps its
            // resized image for the coder groups below (its status is set: its file is dropped).
            std::map<std::tuple<int, uint32_t, int32_t>, std::vector<uint32_t>> filters;
            for (uint32_t k : G.members) {
                const FilterReq& f = op(k).flt;
                if (!f.mode || ds[k]) continue;
                uint32_t sb;
                std::memcpy(&sb, &f.sigma, 4);
                filters[{f.mode, sb, f.threshold}].push_back(k);
            }
            run_sets(filters, rsz, false, ds, dm,
                     [&](uint32_t k0, const std::vector<ik_image*>& fs, std::vector<ik_image*>& fo) {
                         const FilterReq& f = op(k0).flt;
                         return blur_group(fs, f.sigma, f.mode == 2, f.threshold, fo);
                     },
                     [&](uint32_t k, ik_image* im, ik_image** fo) { return filter_image(im, op(k).flt, fo); });
            // then the pad: the group's members share their canvas and origin (the plan's
            // key), those whose 24 pad bytes are equal go through one launch onto new images,
            // a lone one or a failed group through launches of their own, and the unpadded
            // image returns to the pool.  A canvas that is the image: no pass.  A member whose
            // pad fails keeps its image and its status is set (its file is dropped).
            std::map<PadReq::Key, std::vector<uint32_t>> pads;
            if (G.canvas.cw != G.nw || G.canvas.ch != G.nh)
                for (uint32_t k : G.members)
                    if (!ds[k] && op(k).pad.on()) pads[op(k).pad.key()].push_back(k);
            run_sets(pads, rsz, false, ds, dm,
                     [&](uint32_t k0, const std::vector<ik_image*>& ps, std::vector<ik_image*>& po) {
                         return pad_group(ps, op(k0).pad, G.canvas, po);
                     },
                     [&](uint32_t k, ik_image* im, ik_image** po) { return pad_image(im, op(k).pad, G.canvas, po); });
            // then the watermark, in place on the resized (filtered and padded) images: the members
            // that share (overlay handle, gravity, dx, dy, opacity, tile) go through one launch,
            // a lone one or a failed group through launches of their own.  A member whose
            // overlay fails gets its status and message: its file is dropped as above.
            std::map<OverlayReq::Key, std::vector<uint32_t>> marks;
            for (uint32_t k : G.members)
                if (!ds[k] && op(k).ovl.mark) marks[op(k).ovl.key()].push_back(k);
            run_sets(marks, rsz, false, ds, dm,
                     [&](uint32_t k0, const std::vector<ik_image*>& bs, std::vector<ik_image*>& done) {
                         done = bs;
                         return overlay_group(bs, op(k0).ovl);
                     },
                     [&](uint32_t k, ik_image* im, ik_image** done) {
                         *done = im;
                         return overlay_image(im, op(k).ovl);
                     });
        }
        for (uint32_t c = G.cg_lo; c < G.cg_hi; ++c) {
            const PostPlan::CoderGroup& cg = plan.cgroups[c];
            std::vector<ik_image*> im;
            std::vector<EncodePrep*> pp;
            std::vector<std::vector<uint8_t>*> oo;
            bool agree = true;  // (a member whose pad failed still has its unpadded image)
            for (uint32_t k : cg.members) {
                im.push_back(rsz[k]);
                pp.push_back(&prep[k]);
                oo.push_back(&bytes_out[k]);
                agree = agree && rsz[k]->w == G.canvas.cw && rsz[k]->h == G.canvas.ch;
            }
            if (!agree) continue;  // its members: image by image below
            const bool planes = cg.route == PostRoute::WebpFrontGroup;  // libwebp codes them in the host stage
            const int rc = planes                                      ? webp_front_group(im, cg.quality, pp)
                           : cg.route == PostRoute::WebpExactGroup ? webp_exact_group(im, cg.quality, oo)
                                                                       : jpeg_front_group(im, cg.quality, oo);
            if (rc != IK_OK) continue;  // its members: image by image below (Req::solo)
            for (uint32_t k : cg.members) {
                fronted[k] = 1;
                if (planes) continue;
                prep[k].fmt = rq[k].fmt;
                prep[k].done = true;  // the files are final: no host coder
            }
        }
    }
    t_resize += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tg0).count();
    parallel_for((int)m, threads, [&](int k) {
        const uint32_t i = idx[k];
        if (ds[k]) {
            st[i] = ds[k];
            errs[i] = dm[k];
            if (rsz[k]) {  // its group's filter failed after the resize
                ik_image_free(rsz[k]);
                ik_image_free(imgs[k]);
                imgs[k] = nullptr;
                prep[k].done = true;
            }
            return;
        }
        ik_image* rs = rsz[k];
        const auto t0 = std::chrono::steady_clock::now();
        // no group resized it: resized, filtered and marked here
        int r = rs ? IK_OK : image_tail(imgs[k], w[i], h[i], op((uint32_t)k), filter, &rs);
        const auto t1 = std::chrono::steady_clock::now();
        if (!r && !fronted[k] && plan.req[k].solo == PostRoute::WebpMixed) {
            (void)hipStreamSynchronize(thread_stream());  // this thread's resize is done: another's stream reads it
            kept[k] = rs;
        } else if (!r && !fronted[k]) r = encode_image_front(rs, fmt[i], quality[i], prep[k], bytes_out[k]);
        if (timing) {
            const auto t2 = std::chrono::steady_clock::now();
            std::lock_guard<std::mutex> lk(tmu);
            t_resize += std::chrono::duration<double, std::milli>(t1 - t0).count();
            t_front += std::chrono::duration<double, std::milli>(t2 - t1).count();
        }
        if (r) { errs[i] = last_error_str(); st[i] = r; prep[k].done = true; }
        if (rs && rs != imgs[k] && rs != kept[k]) ik_image_free(rs);
        if (imgs[k] != kept[k]) ik_image_free(imgs[k]);
        imgs[k] = nullptr;
    });
    // one colour launch and one mixed exact call for the kept requests; fewer than the
    // minimum of them (the uniform groups took the rest), or a failed call: the existing
    // front end, image by image
    std::vector<uint32_t> ks;
    for (uint32_t k = 0; k < m; ++k)
        if (kept[k]) ks.push_back(k);
    bool coded = false;
    if (ks.size() >= plan.mixed_min) {
        std::vector<ik_image*> im;
        std::vector<int> qs;
        std::vector<std::vector<uint8_t>*> oo;
        for (uint32_t k : ks) { im.push_back(kept[k]); qs.push_back(quality[idx[k]]); oo.push_back(&bytes_out[k]); }
        const auto t0 = std::chrono::steady_clock::now();
        coded = webp_exact_mixed_group(im, qs, oo) == IK_OK;
        t_front += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    }
    parallel_for((int)ks.size(), threads, [&](int j) {
        const uint32_t k = ks[(size_t)j], i = idx[k];
        if (coded) {
            prep[k].fmt = IK_FORMAT_WEBP;
            prep[k].done = true;  // the files are final: no host coder
        } else if (int r = encode_image_front(kept[k], fmt[i], quality[i], prep[k], bytes_out[k])) {
            errs[i] = last_error_str();
            st[i] = r;
            prep[k].done = true;
        }
        ik_image_free(kept[k]);
    });
    batch_timing_commit(current_device(), true);
    gate_pin(kGatePost, false);
    std::vector<ik_image*>().swap(hp.imgs);
    std::vector<int>().swap(hp.ds);
    std::vector<std::string>().swap(hp.dm);
}

}  // namespace ik
