// ik_post_plan.h -- the post stage's routing of a batch (ik_transform_batch): which
// launch resizes each request and which coder writes its file.  Policy only, in sizes
// and counts: plain C++17, no HIP, nothing read from the process (the caller passes the
// WebP encoder setting and the mixed mode, each read once per batch).  The product's
// executor (ik_post_stage.cpp transform_post_phase) walks the plan; ik_post_plan exports it
// for tests/test_post_plan.py.
//
// The rules:
//   resize groups   requests whose decoded images share (W, H, C, pitch, device) and
//                   whose windows (iw, ih, x0, y0, nw, nh; fit_target) agree resize in one
//                   launch (resize_group), when there are at least 2 of them: an exact and a
//                   cover request of one output size are different groups.  Emitted in
//                   ascending key order, members in request order.  A request's pad
//                   (ik_pad) gives it a canvas and an origin (pad_canvas), which are part
//                   of the key as the window is: a group's images leave it with one final
//                   geometry, which is what its coder groups need.  The pad's mode, colour
//                   and alpha are not.
//   coder groups    inside a resize group, its WebP and its JPEG requests of one quality
//                   (at least 2) are coded by one group call.  WebP groups first, then
//                   JPEG, each in ascending quality.
//   the exact rule  a WebP group goes to the exact GPU coder under IK_WEBP_EXACT, or
//                   under IK_WEBP_AUTO from kAutoExactMinGroup (32) frames on
//                   (webp_takes_exact); the rest to libwebp behind one colour launch.
//   the mixed call  under IK_WEBP_MIXED_GPU (and an encoder other than LIBWEBP) a batch
//                   with at least mixed_min 8-bit WebP requests -- kAutoMixedMin (32); 2
//                   under EXACT -- keeps every WebP request that no exact group takes
//                   for one mixed exact call.
//
// Kept as they are, odd as they look:
//   - a request that needs no resize (w = h = None, or a target equal to its size)
//     joins no group, so 32 of them never reach the uniform exact call: WebpMixed or Single
//   - a WebP group with an output dimension (of the canvas, under a pad) above 16383 is routed Single: the per-image
//     front end reports "WebP dimensions ... exceed 16383" for each of its requests
//   - 16-bit images are never grouped and are never mixed candidates
//   - the candidate count behind `mixed` includes requests an exact group then takes, so
//     `mixed` can hold with fewer than mixed_min requests left for the mixed call: the
//     executor counts the survivors again
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <map>
#include <tuple>
#include <vector>

#include "../../include/imagekit_hip.h"

namespace ik {

// IK_WEBP_AUTO: smallest same-geometry group of a batch, and smallest max_batch of a
// pipeline (ik_pipeline.cpp), that the exact GPU coder takes
constexpr size_t kAutoExactMinGroup = 32;
// IK_WEBP_MIXED_GPU: fewest WebP requests of a batch that one mixed exact call takes
// (provisional: the uniform rule's figure, until the two are measured against each
// other -- profiles/webp_mixed_notes.md)
constexpr size_t kAutoMixedMin = 32;
constexpr uint32_t kWebpMaxDim = 16383;

// whether a group, or a pipeline, of `count` same-geometry frames takes the exact GPU
// coder under `encoder` (its chain of macroblock steps costs about the same for 2 frames
// as for 64; a mixed-size stream's small groups code faster on the host threads:
// configs[3]'s loadtest 2,106 vs 1,224 requests/s)
inline bool webp_takes_exact(int encoder, size_t count) {
    return encoder == IK_WEBP_EXACT || (encoder == IK_WEBP_AUTO && count >= kAutoExactMinGroup);
}

// The output size of src/transform.rs:62-90 + DynamicImage::resize for a W x H image
// and the request's (w, h) options (negative = None; not both None).  0, or which limit
// the request broke: 1 a dimension above u32, 2 the fitted size above u32
inline uint32_t f32_as_u32(float v) {
    if (!(v > 0.0f)) return 0;
    if (v >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)v;
}
// the request's target (tw, th): a missing side in f32 with round, each side max(1).
// 1: a dimension above u32
inline int request_target(uint32_t W, uint32_t H, int64_t w, int64_t h, uint32_t* otw, uint32_t* oth) {
    if (w > 0xFFFFFFFFll || h > 0xFFFFFFFFll) return 1;
    uint32_t tw, th;
    if (w >= 0) tw = (uint32_t)w;
    else tw = f32_as_u32(roundf((float)W * ((float)(uint32_t)h / (float)H)));
    if (h >= 0) th = (uint32_t)h;
    else th = f32_as_u32(roundf((float)H * ((float)(uint32_t)w / (float)W)));
    *otw = tw < 1 ? 1 : tw;
    *oth = th < 1 ? 1 : th;
    return 0;
}
// image 0.25.8 resize_dimensions (f64 ratio, round, max 1): aspect fit, or fill.  2: a
// side above u32
inline int resize_dimensions(uint32_t W, uint32_t H, uint32_t tw, uint32_t th, bool fill, uint32_t* onw,
                             uint32_t* onh) {
    const double wr = (double)tw / (double)W, hr = (double)th / (double)H;
    const double r = fill ? (wr > hr ? wr : hr) : (wr < hr ? wr : hr);
    double fw = std::round((double)W * r), fh = std::round((double)H * r);
    if (!(fw < 1.8e19) || !(fh < 1.8e19)) return 2;
    unsigned long long rw = fw < 1 ? 1 : (unsigned long long)fw;
    unsigned long long rh = fh < 1 ? 1 : (unsigned long long)fh;
    if (rw > 0xFFFFFFFFull || rh > 0xFFFFFFFFull) return 2;
    *onw = (uint32_t)rw;
    *onh = (uint32_t)rh;
    return 0;
}
inline int resize_target_dims(uint32_t W, uint32_t H, int64_t w, int64_t h, uint32_t* onw, uint32_t* onh) {
    uint32_t tw, th;
    if (request_target(W, H, w, h, &tw, &th)) return 1;
    uint32_t nw = tw, nh = th;
    if (!(tw == W && th == H) && resize_dimensions(W, H, tw, th, false, &nw, &nh)) return 2;
    *onw = nw;
    *onh = nh;
    return 0;
}

// What a request computes under a fit mode (ik_fit): columns [x0, x0 + nw) and rows
// [y0, y0 + nh) of the image resampled to iw x ih.
//   CONTAIN  DynamicImage::resize: the aspect-fitted size, whole
//   EXACT    DynamicImage::resize_exact: the target, whole
//   COVER    DynamicImage::resize_to_fill (image 0.25.8 as recalled):
//            resize_dimensions(fill) -> resize_exact -> crop, centred along the axis
//            that overflows the target; with one side None there is nothing to crop
// (w, h as resize_target_dims: not both None.)  The same codes.
struct FitWindow {
    uint32_t iw = 0, ih = 0, x0 = 0, y0 = 0, nw = 0, nh = 0;
    bool whole() const { return x0 == 0 && y0 == 0 && nw == iw && nh == ih; }
    bool operator==(const FitWindow& o) const {
        return iw == o.iw && ih == o.ih && x0 == o.x0 && y0 == o.y0 && nw == o.nw && nh == o.nh;
    }
};
inline int fit_target(uint32_t W, uint32_t H, int64_t w, int64_t h, int fit, FitWindow* out) {
    FitWindow f;
    if (fit == IK_FIT_CONTAIN || (fit == IK_FIT_COVER && (w < 0 || h < 0))) {
        if (int rc = resize_target_dims(W, H, w, h, &f.nw, &f.nh)) return rc;
        f.iw = f.nw;
        f.ih = f.nh;
        *out = f;
        return 0;
    }
    uint32_t tw, th;
    if (request_target(W, H, w, h, &tw, &th)) return 1;
    if (fit == IK_FIT_EXACT || W == 0 || H == 0) {  // (an empty image: ik_resize_exact's blank tw x th)
        f.iw = f.nw = tw;
        f.ih = f.nh = th;
        *out = f;
        return 0;
    }
    if (int rc = resize_dimensions(W, H, tw, th, true, &f.iw, &f.ih)) return rc;
    uint32_t cx = 0, cy = 0;
    if ((uint64_t)tw * f.ih > (uint64_t)f.iw * th) cy = f.ih > th ? (f.ih - th) / 2 : 0;
    else cx = f.iw > tw ? (f.iw - tw) / 2 : 0;
    // imageops::crop clamps the rectangle to what is left of the image
    f.x0 = cx < f.iw ? cx : f.iw;
    f.y0 = cy < f.ih ? cy : f.ih;
    f.nw = tw < f.iw - f.x0 ? tw : f.iw - f.x0;
    f.nh = th < f.ih - f.y0 ? th : f.ih - f.y0;
    *out = f;
    return 0;
}

// Where a W x H image lies on its canvas (ik_pad): cw = max(W, width), ch
// = max(H, height), so a width or height of 0 leaves that axis alone; x0 is 0, (cw - W) / 2
// (floor) or cw - W by the gravity, y0 likewise.  The gravity is one of ik_gravity (checked
// by the caller).  Everything that places a pad does it here.
struct PadGeom {
    uint32_t cw = 0, ch = 0, x0 = 0, y0 = 0;
    bool operator==(const PadGeom& o) const { return cw == o.cw && ch == o.ch && x0 == o.x0 && y0 == o.y0; }
};
inline PadGeom pad_place(uint32_t W, uint32_t H, uint32_t width, uint32_t height, int gravity) {
    PadGeom g;
    g.cw = W > width ? W : width;
    g.ch = H > height ? H : height;
    const bool left = gravity == IK_GRAVITY_W || gravity == IK_GRAVITY_NW || gravity == IK_GRAVITY_SW;
    const bool right = gravity == IK_GRAVITY_E || gravity == IK_GRAVITY_NE || gravity == IK_GRAVITY_SE;
    const bool top = gravity == IK_GRAVITY_N || gravity == IK_GRAVITY_NE || gravity == IK_GRAVITY_NW;
    const bool bottom = gravity == IK_GRAVITY_S || gravity == IK_GRAVITY_SE || gravity == IK_GRAVITY_SW;
    g.x0 = left ? 0 : right ? g.cw - W : (g.cw - W) / 2;
    g.y0 = top ? 0 : bottom ? g.ch - H : (g.ch - H) / 2;
    return g;
}
// one request's pad as the plan sees it: its geometry only (mode, colour and alpha do not
// route anything)
struct PostPad {
    bool on = false;
    int gravity = IK_GRAVITY_CENTER;
    uint32_t width = 0, height = 0;  // 0: the side of the request's target
};
// The canvas of a request whose W x H image, asked for as (w, h), came out of the resize as
// nw x nh: a pad side of 0 is the side of the request's target (request_target), or with w
// and h both None the image's own.  No pad: the image is the canvas.
inline PadGeom pad_canvas(const PostPad& p, uint32_t W, uint32_t H, int64_t w, int64_t h, uint32_t nw, uint32_t nh) {
    uint32_t width = p.width, height = p.height;
    if (p.on && !(w < 0 && h < 0) && (!width || !height)) {
        uint32_t tw = 0, th = 0;
        if (request_target(W, H, w, h, &tw, &th) == 0) {  // (it failed: so did the resize)
            if (!width) width = tw;
            if (!height) height = th;
        }
    }
    return p.on ? pad_place(nw, nh, width, height, p.gravity) : pad_place(nw, nh, 0, 0, IK_GRAVITY_NW);
}

enum class PostRoute : int {  // (ik_post_route, as ik_post_plan reports it)
    None = IK_POST_NONE,                       // the decode failed: its status is the request's
    Single = IK_POST_SINGLE,                   // the per-image ik_resize and / or encode_image_front
    WebpMixed = IK_POST_WEBP_MIXED,            // its resized image is kept for the batch's one mixed exact call
    WebpFrontGroup = IK_POST_WEBP_FRONT_GROUP, // its coder group goes to webp_front_group (libwebp codes the planes)
    WebpExactGroup = IK_POST_WEBP_EXACT_GROUP, // its coder group goes to webp_exact_group
    JpegGroup = IK_POST_JPEG_GROUP,            // its coder group goes to jpeg_front_group
};

struct PostRequest {
    bool ok = false;  // decode status 0 and a non-null image
    uint32_t W = 0, H = 0, C = 0;
    size_t pitch = 0;
    int device = 0;
    uint32_t depth = 1;
    int64_t w = -1, h = -1;  // negative: None
    int fmt = 0, quality = 0;
    int fit = IK_FIT_CONTAIN;
    PostPad pad;  // (default: none)
};

struct PostPlan {
    struct Req {
        bool sized = false;    // (nw, nh) is the size its encoder sees (false: the decode or fit_target failed)
        uint32_t nw = 0, nh = 0;
        FitWindow win;         // (sized) what it computes: win.nw x win.nh = nw x nh
        PadGeom canvas;        // (sized) where those pixels lie in the image that is coded: nw x nh at (0, 0) without a pad
        int rgroup = -1, cgroup = -1;
        PostRoute route = PostRoute::None;
        // its route when no group call takes it (it is in no coder group, or its group's
        // resize or coder call failed at run time): Single or WebpMixed
        PostRoute solo = PostRoute::None;
    };
    struct ResizeGroup {
        uint32_t nw = 0, nh = 0;
        FitWindow win;
        PadGeom canvas;                 // its members' final geometry
        std::vector<uint32_t> members;  // request order
        uint32_t cg_lo = 0, cg_hi = 0;  // its coder groups: cgroups[cg_lo, cg_hi)
    };
    struct CoderGroup {
        PostRoute route = PostRoute::None;
        int quality = 0;
        int rgroup = -1;
        std::vector<uint32_t> members;
    };
    bool mixed = false;
    size_t mixed_min = kAutoMixedMin;
    std::vector<Req> req;
    std::vector<ResizeGroup> rgroups;
    std::vector<CoderGroup> cgroups;
};

inline PostPlan post_plan(const PostRequest* rq, uint32_t m, int webp_encoder, int mixed_mode) {
    PostPlan P;
    P.req.resize(m);
    if (webp_encoder == IK_WEBP_EXACT) P.mixed_min = 2;  // any two, as EXACT's uniform groups
    if (mixed_mode == IK_WEBP_MIXED_GPU && webp_encoder != IK_WEBP_LIBWEBP) {
        size_t cand = 0;  // (counted before the exact groups take theirs: see above)
        for (uint32_t k = 0; k < m; ++k) cand += rq[k].ok && rq[k].depth == 1 && rq[k].fmt == IK_FORMAT_WEBP;
        P.mixed = cand >= P.mixed_min;
    }
    // (W, H, C, pitch, device), then the window: iw, ih, x0, y0 and with them (nw, nh), then
    // the canvas and the origin in it (without a pad: nw, nh, 0, 0 for every member)
    typedef std::tuple<uint32_t, uint32_t, uint32_t, size_t, int, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t,
                       uint32_t, uint32_t, uint32_t, uint32_t, uint32_t> GroupKey;
    struct GroupSlot {
        FitWindow win;
        PadGeom canvas;
        std::vector<uint32_t> members;
    };
    std::map<GroupKey, GroupSlot> groups;
    for (uint32_t k = 0; k < m; ++k) {
        const PostRequest& r = rq[k];
        PostPlan::Req& q = P.req[k];
        if (!r.ok) continue;
        q.route = q.solo = PostRoute::Single;
        if (r.w < 0 && r.h < 0) {  // no resize asked for
            q.sized = true;
            q.win.iw = q.win.nw = r.W;
            q.win.ih = q.win.nh = r.H;
        } else {
            q.sized = fit_target(r.W, r.H, r.w, r.h, r.fit, &q.win) == 0;
        }
        q.nw = q.sized ? q.win.nw : 0;
        q.nh = q.sized ? q.win.nh : 0;
        if (!q.sized) continue;  // Single: ik_resize reports it
        q.canvas = pad_canvas(r.pad, r.W, r.H, r.w, r.h, q.nw, q.nh);
        if (P.mixed && r.fmt == IK_FORMAT_WEBP && r.depth == 1 && q.nw >= 1 && q.nh >= 1 && q.canvas.cw <= kWebpMaxDim &&
            q.canvas.ch <= kWebpMaxDim)
            q.route = q.solo = PostRoute::WebpMixed;
        // (never a request that needs no resampling: a whole copy or, under COVER, a crop of one)
        if (r.depth == 1 && !(q.win.iw == r.W && q.win.ih == r.H)) {
            // ordered by (nw, nh) first, as before the windows, then by the rest of the window
            auto& slot = groups[GroupKey(r.W, r.H, r.C, r.pitch, r.device, q.nw, q.nh, q.win.iw, q.win.ih, q.win.x0,
                                         q.win.y0, q.canvas.cw, q.canvas.ch, q.canvas.x0, q.canvas.y0)];
            slot.win = q.win;
            slot.canvas = q.canvas;
            slot.members.push_back(k);
        }
    }
    for (auto& gv : groups) {
        std::vector<uint32_t>& gm = gv.second.members;
        if (gm.size() < 2) continue;
        const int g = (int)P.rgroups.size();
        PostPlan::ResizeGroup G;
        G.win = gv.second.win;
        G.canvas = gv.second.canvas;
        G.nw = G.win.nw;
        G.nh = G.win.nh;
        G.cg_lo = (uint32_t)P.cgroups.size();
        std::map<int, std::vector<uint32_t>> byq, jbyq;
        for (uint32_t k : gm) {
            P.req[k].rgroup = g;
            if (rq[k].fmt == IK_FORMAT_WEBP) byq[rq[k].quality].push_back(k);
            if (rq[k].fmt == IK_FORMAT_JPEG) jbyq[rq[k].quality].push_back(k);
        }
        auto emit = [&](PostRoute route, int quality, std::vector<uint32_t>& members) {
            for (uint32_t k : members) {
                P.req[k].cgroup = (int)P.cgroups.size();
                P.req[k].route = route;
            }
            PostPlan::CoderGroup cg;
            cg.route = route;
            cg.quality = quality;
            cg.rgroup = g;
            cg.members.swap(members);
            P.cgroups.push_back(std::move(cg));
        };
        for (auto& qv : byq) {
            if (qv.second.size() < 2) continue;
            if (G.canvas.cw > kWebpMaxDim || G.canvas.ch > kWebpMaxDim) continue;  // Single, for the per-image error
            if (webp_takes_exact(webp_encoder, qv.second.size())) emit(PostRoute::WebpExactGroup, qv.first, qv.second);
            else if (!P.mixed) emit(PostRoute::WebpFrontGroup, qv.first, qv.second);
        }
        for (auto& qv : jbyq)
            if (qv.second.size() >= 2) emit(PostRoute::JpegGroup, qv.first, qv.second);
        G.cg_hi = (uint32_t)P.cgroups.size();
        G.members.swap(gm);
        P.rgroups.push_back(std::move(G));
    }
    return P;
}

}  // namespace ik
