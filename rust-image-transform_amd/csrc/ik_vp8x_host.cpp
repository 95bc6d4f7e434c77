// ik_vp8x_host.cpp -- the exact WebP coder's host half (encode_image's WebP branch,
// reference src/transform.rs:129-137 -> webp 0.3.1 -> libwebp WebPEncodeRGB): libwebp's
// segment analysis and macroblock decisions run on the GPU (ik_vp8_analysis.hip,
// ik_vp8x.hip); here the epoch/diagonal schedule, the segment set-up, and the
// bitstream: the tokens in RecordTokens order with the final probabilities, libwebp's
// boolean coder, partition 0 (header, segment map, modes), the filter levels libwebp
// raises after coding, and the RIFF container -- the same file WebPEncodeRGB writes
// (tests/test_gpu_vp8x.py; the model is oracle/vp8_modes.c).
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cmath>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "../../include/imagekit_hip.h"
#include "ik_runtime.h"
#include "ik_vp8_gpu.h"
#include "ik_vp8x_gpu.h"

namespace ik {

namespace {

using namespace vp8x;

// ---- libwebp's boolean coder (utils/bit_writer_utils.c) ----
struct BitWriter {
    int32_t range = 255 - 1, value = 0;
    int run = 0, nb_bits = -8;
    std::vector<uint8_t> buf;

    void flush() {
        const int s = 8 + nb_bits;
        const int32_t bits = value >> s;
        value -= bits << s;
        nb_bits -= 8;
        if ((bits & 0xff) != 0xff) {
            if ((bits & 0x100) && !buf.empty()) buf.back()++;  // carry into the bytes written
            for (; run > 0; --run) buf.push_back((bits & 0x100) ? 0x00 : 0xff);
            buf.push_back((uint8_t)(bits & 0xff));
        } else {
            run++;  // 0xff bytes wait: a carry may still come
        }
    }
    int put(int bit, int prob) {
        const int split = (range * prob) >> 8;
        if (bit) {
            value += split + 1;
            range -= split + 1;
        } else {
            range = split;
        }
        if (range < 127) {
            int shift = 0;
            while (((range + 1) << shift) < 128) ++shift;
            range = ((range + 1) << shift) - 1;
            value <<= shift;
            nb_bits += shift;
            if (nb_bits > 0) flush();
        }
        return bit;
    }
    int uniform(int bit) {
        const int split = range >> 1;
        if (bit) {
            value += split + 1;
            range -= split + 1;
        } else {
            range = split;
        }
        if (range < 127) {
            range = ((range + 1) << 1) - 1;
            value <<= 1;
            nb_bits += 1;
            if (nb_bits > 0) flush();
        }
        return bit;
    }
    void bits(uint32_t v, int nb) {
        for (uint32_t mask = 1u << (nb - 1); mask; mask >>= 1) uniform((v & mask) != 0);
    }
    void sbits(int v, int nb) {
        if (!uniform(v != 0)) return;
        if (v < 0) bits(((uint32_t)(-v) << 1) | 1u, nb + 1);
        else bits((uint32_t)v << 1, nb + 1);
    }
    void finish() {
        bits(0, 9 - nb_bits);
        nb_bits = 0;
        flush();
    }
};

void put_le32(uint8_t* p, uint32_t v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
    p[2] = (uint8_t)(v >> 16);
    p[3] = (uint8_t)(v >> 24);
}

// The WebP file of one image from the device's decisions.
void write_file(int w, int h, const XMB* mbs, const uint8_t* probas, const ik_vp8_segment_header& hd,
                const int* max_edge, const XSeg* segs, std::vector<uint8_t>& out) {
    const int mb_w = (w + 15) / 16, mb_h = (h + 15) / 16;
    // the token partition, in RecordTokens order, with the final probabilities
    BitWriter b1;
    {
        std::vector<int> top((size_t)mb_w * 9, 0);
        for (int my = 0; my < mb_h; ++my) {
            int left[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int mx = 0; mx < mb_w; ++mx) {
                record_mb([](uint32_t, int bit) { return bit; }, mbs[my * mb_w + mx], &top[(size_t)mx * 9], left,
                          [&](int bit, uint32_t id) {
                    if (id & 0x4000u) b1.put(bit, (int)(id & 0xffu));
                    else b1.put(bit, probas[id]);
                });
            }
        }
        b1.finish();
    }
    // VP8AdjustFilterStrength: each segment's level at least what its DC-only MBs' largest
    // step needs (kLevelsFromDelta[sharpness 0] is the identity on 0..63)
    int level[4], max_level = 0;
    for (int s = 0; s < 4; ++s) {
        const int delta = (max_edge[s] * segs[s].y2.q[1]) >> 3;
        const int lv = delta < 63 ? delta : 63;
        level[s] = hd.fstrength[s] > lv ? hd.fstrength[s] : lv;
        if (level[s] > max_level) max_level = level[s];
    }
    // partition 0
    BitWriter b0;
    b0.uniform(0);  // colour space
    b0.uniform(0);  // clamping
    if (b0.uniform(hd.num_segments > 1)) {
        b0.uniform(hd.update_map);
        if (b0.uniform(1)) {
            b0.uniform(1);  // absolute values
            for (int s = 0; s < 4; ++s) b0.sbits(hd.quant[s], 7);
            for (int s = 0; s < 4; ++s) b0.sbits(level[s], 6);
        }
        if (hd.update_map)
            for (int s = 0; s < 3; ++s)
                if (b0.uniform(hd.probs[s] != 255)) b0.bits((uint32_t)hd.probs[s], 8);
    }
    b0.uniform(0);  // normal loop filter
    b0.bits((uint32_t)max_level, 6);
    b0.bits(0, 3);  // sharpness
    b0.uniform(0);  // no lf deltas
    b0.bits(0, 2);  // one token partition
    b0.bits((uint32_t)hd.quant[0], 7);
    b0.sbits(0, 4);
    b0.sbits(0, 4);
    b0.sbits(0, 4);
    b0.sbits(hd.dq_uv_dc, 4);
    b0.sbits(hd.dq_uv_ac, 4);
    b0.uniform(0);  // no entropy refresh
    for (int i = 0; i < 1056; ++i)
        if (b0.put(probas[i] != kCoeffProbs0[i], kCoeffUpdateProbs[i])) b0.bits(probas[i], 8);
    b0.uniform(0);  // no skip probability
    for (int i = 0; i < mb_w * mb_h; ++i) {
        const int mx = i % mb_w, my = i / mb_w;
        const XMB& m = mbs[i];
        if (hd.update_map) {
            if (b0.put(m.seg >= 2, hd.probs[0])) b0.put(m.seg & 1, hd.probs[2]);
            else b0.put(m.seg & 1, hd.probs[1]);
        }
        if (b0.put(m.ymode != 4, 145)) {
            const int mode = m.ymode;
            if (b0.put(mode == 1 || mode == 3, 156)) b0.put(mode == 1, 128);
            else b0.put(mode == 2, 163);
        } else {
            for (int k = 0; k < 16; ++k) {
                const int bx = k & 3, by = k >> 2;
                const int top = by ? m.bmodes[k - 4] : (my ? mbs[i - mb_w].bmodes[12 + bx] : 0);
                const int left = bx ? m.bmodes[k - 1] : (mx ? mbs[i - 1].bmodes[by * 4 + 3] : 0);
                const uint8_t* p = kBModeProbs + (top * 10 + left) * 9;
                const int mode = m.bmodes[k];
                if (b0.put(mode != 0, p[0]))
                    if (b0.put(mode != 1, p[1]))
                        if (b0.put(mode != 2, p[2])) {
                            if (!b0.put(mode >= 6, p[3])) {
                                if (b0.put(mode != 3, p[4])) b0.put(mode != 4, p[5]);
                            } else if (b0.put(mode != 6, p[6])) {
                                if (b0.put(mode != 7, p[7])) b0.put(mode != 8, p[8]);
                            }
                        }
            }
        }
        if (b0.put(m.uvmode != 0, 142))
            if (b0.put(m.uvmode != 2, 114)) b0.put(m.uvmode != 3, 183);
    }
    b0.finish();
    // RIFF + VP8 chunk (profile 0: normal filter)
    size_t vp8_size = 10 + b0.buf.size() + b1.buf.size();
    const size_t pad = vp8_size & 1;
    vp8_size += pad;
    const size_t riff_size = 4 + 8 + vp8_size;
    out.assign(8 + riff_size, 0);
    uint8_t* o = out.data();
    std::memcpy(o, "RIFF", 4);
    put_le32(o + 4, (uint32_t)riff_size);
    std::memcpy(o + 8, "WEBPVP8 ", 8);
    put_le32(o + 16, (uint32_t)vp8_size);
    const uint32_t bits = (1u << 4) | ((uint32_t)b0.buf.size() << 5);
    o[20] = (uint8_t)bits;
    o[21] = (uint8_t)(bits >> 8);
    o[22] = (uint8_t)(bits >> 16);
    o[23] = 0x9d;
    o[24] = 0x01;
    o[25] = 0x2a;
    o[26] = (uint8_t)(w & 0xff);
    o[27] = (uint8_t)(w >> 8);
    o[28] = (uint8_t)(h & 0xff);
    o[29] = (uint8_t)(h >> 8);
    std::memcpy(o + 30, b0.buf.data(), b0.buf.size());
    std::memcpy(o + 30 + b0.buf.size(), b1.buf.data(), b1.buf.size());
}

// One geometry's ticket order, as steps: epochs at libwebp's probability refreshes
// (M = max(nmb / 8, 96), bounds M, 2M+1, ...); inside an epoch the MBs by diagonal
// mb_x + 2 mb_y (one counting pass per epoch), then the epoch's fold.  A step is one
// diagonal that holds MBs, or one fold; every dependency of a ticket lies in an earlier
// step.  Tickets carry the epoch and the MB, image 0.
struct GeomSteps {
    std::vector<int> bounds;        // nep + 1 raster bounds of the epochs
    std::vector<uint64_t> tasks;    // the geometry's tickets in order
    std::vector<uint32_t> step_lo;  // steps + 1: each step's first ticket, then the ticket count
};

void build_geometry_steps(int mb_w, int mb_h, GeomSteps& g) {
    const int nmb = mb_w * mb_h;
    const int M = (nmb >> 3) < 96 ? 96 : (nmb >> 3);
    g.bounds.assign(1, 0);
    for (int k = M; k < nmb; k += M + 1) g.bounds.push_back(k);
    g.bounds.push_back(nmb);
    g.tasks.clear();
    g.tasks.reserve((size_t)nmb + g.bounds.size());
    g.step_lo.clear();
    std::vector<int> first, list;
    for (size_t e = 0; e + 1 < g.bounds.size(); ++e) {
        const int k0 = g.bounds[e], k1 = g.bounds[e + 1];
        // (an epoch that starts mid-row holds MBs of smaller diagonals in its next row)
        int d0 = 1 << 30, d1 = -1;
        for (int k = k0; k < k1; ++k) {
            d0 = std::min(d0, k % mb_w + 2 * (k / mb_w));
            d1 = std::max(d1, k % mb_w + 2 * (k / mb_w));
        }
        first.assign((size_t)(d1 - d0 + 2), 0);  // counting sort of the epoch's MBs by diagonal
        for (int k = k0; k < k1; ++k) ++first[(size_t)(k % mb_w + 2 * (k / mb_w) - d0 + 1)];
        for (size_t d = 1; d < first.size(); ++d) first[d] += first[d - 1];
        list.assign((size_t)(k1 - k0), 0);
        std::vector<int> at(first.begin(), first.end() - 1);
        for (int k = k0; k < k1; ++k) list[(size_t)at[(size_t)(k % mb_w + 2 * (k / mb_w) - d0)]++] = k;
        const uint64_t ep = (uint64_t)e << 48;
        for (int d = 0; d <= d1 - d0; ++d) {
            const int a = first[(size_t)d], b = first[(size_t)d + 1];
            if (a == b) continue;  // (a diagonal between an epoch's two rows may hold none of its MBs)
            g.step_lo.push_back((uint32_t)g.tasks.size());
            for (int j = a; j < b; ++j) g.tasks.push_back(ep | (uint32_t)list[(size_t)j]);
        }
        g.step_lo.push_back((uint32_t)g.tasks.size());
        g.tasks.push_back((1ull << 63) | ep);
    }
    g.step_lo.push_back((uint32_t)g.tasks.size());
}

// the steps of a geometry, cached per thread (emptied by begin_schedule when it has
// grown past kGeomCacheMax: references stay valid until the next begin_schedule)
constexpr size_t kGeomCacheMax = 256;
std::map<std::pair<int, int>, GeomSteps>& geometry_cache() {
    static thread_local std::map<std::pair<int, int>, GeomSteps> cache;
    return cache;
}
void begin_schedule() {
    if (geometry_cache().size() > kGeomCacheMax) geometry_cache().clear();
}
const GeomSteps& geometry_steps(int w, int h) {
    const int mb_w = (w + 15) / 16, mb_h = (h + 15) / 16;
    auto it = geometry_cache().find({mb_w, mb_h});
    if (it == geometry_cache().end()) {
        it = geometry_cache().emplace(std::make_pair(mb_w, mb_h), GeomSteps()).first;
        build_geometry_steps(mb_w, mb_h, it->second);
    }
    return it->second;
}

// The call's tickets: the images' steps merged step by step -- step 0 of every image
// (in image order), then step 1 of every image, ...; an image out of steps adds nothing.
// Each image keeps its own order, and a ticket's dependencies (earlier steps of its own
// image) hold smaller tickets, so the lowest unfinished ticket can always run.  Returns
// the widest merged step's ticket count.
int merge_steps(const std::vector<const GeomSteps*>& g, std::vector<uint64_t>& tasks) {
    size_t total = 0;
    for (const GeomSteps* p : g) total += p->tasks.size();
    tasks.clear();
    tasks.reserve(total);
    std::vector<uint32_t> live(g.size());
    for (size_t i = 0; i < g.size(); ++i) live[i] = (uint32_t)i;
    size_t widest = 1;
    for (size_t step = 0; !live.empty(); ++step) {
        const size_t at = tasks.size();
        size_t keep = 0;
        for (uint32_t i : live) {
            const GeomSteps& s = *g[i];
            if (step + 1 >= s.step_lo.size()) continue;  // out of steps
            for (uint32_t t = s.step_lo[step]; t < s.step_lo[step + 1]; ++t) tasks.push_back(s.tasks[t] | ((uint64_t)i << 32));
            live[keep++] = i;
        }
        live.resize(keep);
        widest = std::max(widest, tasks.size() - at);
    }
    return (int)std::min<size_t>(widest, 1u << 30);
}

// resident workgroups: the widest step's tickets (every workgroup more would hold
// LDS and registers that another batch's decode kernels beside the coder lose)
// (IK_VP8X_GRID: a multiple of that, e.g. 0.5 -- dev A/B)
int schedule_grid(int widest, size_t ntasks) {
    static const double mul = getenv("IK_VP8X_GRID") ? atof(getenv("IK_VP8X_GRID")) : 1.0;
    const int want = std::max(1, (int)(std::max(mul, 0.05) * widest));
    return (int)std::min<size_t>(std::min(want, 2048), ntasks);
}

// The uniform call's schedule, cached per thread for its geometry: n images of one
// geometry merged -- tickets in (epoch, diagonal, image) order, each epoch's folds
// after its MBs.
struct XSchedule {
    int w = 0, h = 0, n = 0;
    std::vector<int> bounds;
    std::vector<uint64_t> tasks;
    int grid = 0;
};

const XSchedule& exact_schedule(int w, int h, int n) {
    static thread_local XSchedule sc;
    if (sc.w == w && sc.h == h && sc.n == n) return sc;
    begin_schedule();
    const GeomSteps& g = geometry_steps(w, h);
    sc.bounds = g.bounds;
    const int widest = merge_steps(std::vector<const GeomSteps*>((size_t)n, &g), sc.tasks);
    sc.grid = schedule_grid(widest, sc.tasks.size());
    sc.w = w;
    sc.h = h;
    sc.n = n;
    return sc;
}

// libwebp VP8SetSegmentParams' quantiser for a segment alpha (-127..127) at quality q:
// the pow() is the host's (the same libm call libwebp makes)
void segment_quant_table(float quality, int* qtab) {
    const double amp = 0.9 * 50 / 100. / 128.;  // SNS_TO_DQ, sns 50
    const double Q = quality / 100.;
    const double linear_c = (Q < 0.75) ? Q * (2. / 3.) : 2. * Q - 1.;
    const double c_base = pow(linear_c, 1 / 3.);
    for (int s = -127; s <= 127; ++s) {
        const int v = (int)(127. * (1. - pow(c_base, 1. - amp * s)));
        qtab[s + 127] = v < 0 ? 0 : (v > 127 ? 127 : v);
    }
}

// What a call holds, in the units its arrays are sized by.  The uniform call is the
// mixed one with mb = n * nmb, ep = n * nep, one quantiser table, one geometry's bounds
// and no descriptors.
struct XTotals {
    size_t n, mb, ep;      // images, their macroblocks, their epochs
    size_t quals, bounds;  // 255-entry quantiser tables (distinct qualities), epoch-bound entries
    size_t desc_bytes;     // the descriptor table (the mixed call's)
    size_t tasks;          // tickets
};

// A call's device work area (kScratchExact): one allocation, every field the offset of a
// 256-byte aligned part.  The hand-off words lie first (one memset zeroes them per
// call), the constants last in the order they are staged (one upload).  Without `run`
// (vp8_analyze_setup) the parts only k_vp8x_run uses -- sync, mbs, edges, bounds, desc,
// tasks -- are empty, and an empty part moves no offset after it.
struct WorkArea {
    size_t sync, alpha, uva, kseg, rec, hdr, mbs, edges, seg, segs, lc, pr, st, me, qtab, bounds, desc, tasks;
    size_t sync_bytes, bytes;  // the zeroed part, the whole area
};

WorkArea work_area(const XTotals& t, bool run) {
    WorkArea L{};
    auto part = [&](size_t bytes) { const size_t o = L.bytes; L.bytes += (bytes + 255) & ~(size_t)255; return o; };
    const size_t r = run ? 1 : 0;
    L.sync = part(r * 4 * (4 + t.mb + 2 * t.ep));
    L.sync_bytes = L.bytes;
    L.alpha = part(t.mb), L.uva = part(t.mb * 2), L.kseg = part(t.mb);
    L.rec = part(sizeof(vp8::SegRecord) * t.n), L.hdr = part(sizeof(ik_vp8_segment_header) * t.n);
    L.mbs = part(r * sizeof(XMB) * t.mb), L.edges = part(r * sizeof(XEdge) * t.mb);
    L.seg = part(t.mb), L.segs = part(sizeof(XSeg) * 4 * t.n);
    L.lc = part(2ull * kCostRows * kLevelTab * t.n), L.pr = part(1056ull * t.n), L.st = part(4ull * 1056 * t.n);
    L.me = part(16ull * t.n);
    L.qtab = part(4 * 255 * t.quals), L.bounds = part(r * 4 * t.bounds);
    L.desc = part(r * t.desc_bytes), L.tasks = part(r * 8 * t.tasks);
    return L;
}

// The fields of XArgs and XRun that every call fills alike, from the work area at d
// (r null: the call has no run-only parts; a.mbs and a.edges stay null)
void fill_args(uint8_t* d, const WorkArea& L, const XTotals& t, XArgs& a, XRun* r) {
    a.seg = d + L.seg;
    a.segs = (XSeg*)(d + L.segs);
    a.lc = (uint16_t*)(d + L.lc);
    a.pr = d + L.pr;
    a.stats = (uint32_t*)(d + L.st);
    a.max_edge = (int*)(d + L.me);
    if (!r) return;
    a.mbs = (XMB*)(d + L.mbs);
    a.edges = (XEdge*)(d + L.edges);
    r->tasks = (const uint64_t*)(d + L.tasks);
    r->ntasks = (uint32_t)t.tasks;
    r->bounds = (const int*)(d + L.bounds);
    r->sync = (uint32_t*)(d + L.sync);
    r->done = r->sync + 4;
    r->cnt = r->done + t.mb;
    r->ready = r->cnt + t.ep;
}

// XArgs of n images of one geometry, a common stride apart (the mixed call's come per
// image from its descriptors)
XArgs uniform_args(const uint8_t* d_yuv, size_t yuv_stride, int w, int h) {
    XArgs a{};
    a.yuv = d_yuv;
    a.yuv_stride = yuv_stride;
    a.w = w;
    a.h = h;
    a.mb_w = (w + 15) / 16;
    a.mb_h = (h + 15) / 16;
    return a;
}

// The coder's stream: the thread's highest-priority one, so its launch is dispatched
// ahead of another batch's decode kernels, ordered by an event after the thread's main
// stream, which produced the planes; that main stream itself where there is no other.
int coder_stream(hipStream_t* out) {
    hipStream_t ts = thread_stream();
    if (!ts) return fail(IK_ERR_DEVICE, "cannot create HIP stream");
    hipStream_t s = ts;
    hipEvent_t ev = nullptr;
    if (thread_prio_stream(&s, &ev) && s != ts) {
        IK_HIP(hipEventRecord(ev, ts));
        IK_HIP(hipStreamWaitEvent(s, ev, 0));
    } else {
        s = ts;
    }
    *out = s;
    return IK_OK;
}

// The call's constants through pinned staging in one upload -- a quantiser table per
// quality, the epoch bounds, the descriptors (t.desc_bytes of them, may be none), the
// tickets -- and the hand-off words zeroed, on s.
int upload_constants(uint8_t* d, const WorkArea& L, const XTotals& t, const int* quals, const int* bounds,
                     const XImg* desc, const uint64_t* tasks, hipStream_t s) {
    const size_t const_bytes = L.bytes - L.qtab;
    uint8_t* hc = pinned_slot(kPinnedExactIn, const_bytes);
    if (!hc) return IK_ERR_NOMEM;
    for (size_t k = 0; k < t.quals; ++k) segment_quant_table((float)quals[k], reinterpret_cast<int*>(hc) + 255 * k);
    std::memcpy(hc + (L.bounds - L.qtab), bounds, 4 * t.bounds);
    if (t.desc_bytes) std::memcpy(hc + (L.desc - L.qtab), desc, t.desc_bytes);
    std::memcpy(hc + (L.tasks - L.qtab), tasks, 8 * t.tasks);
    IK_HIP(hipMemcpyAsync(d + L.qtab, hc, const_bytes, hipMemcpyHostToDevice, s));
    IK_HIP(hipMemsetAsync(d + L.sync, 0, L.sync_bytes, s));
    return IK_OK;
}

// Where image i's file comes from: its size and its first record
struct ImgAt {
    int w, h;
    size_t mb0;
};

// After k_vp8x_run: the records back (~830 B per MB), the final probabilities, the
// filter-edge maxima, the headers and the error word; then the files on the host,
// image i's from at(i).
template <class At>
int read_back_and_write(const uint8_t* d, const WorkArea& L, const XTotals& t, hipStream_t s, At at,
                        std::vector<std::vector<uint8_t>>& outs) {
    const int n = (int)t.n;
    const size_t rec_bytes = sizeof(XMB) * t.mb;
    const size_t o_hpr = rec_bytes, o_hme = o_hpr + 1056ull * n, o_hhd = o_hme + 16ull * n;
    const size_t o_herr = o_hhd + sizeof(ik_vp8_segment_header) * n, hbytes = o_herr + 16;
    uint8_t* hp = pinned_slot(kPinnedExactOut, hbytes);
    if (!hp) return IK_ERR_NOMEM;
    IK_HIP(hipMemcpyAsync(hp, d + L.mbs, rec_bytes, hipMemcpyDeviceToHost, s));
    IK_HIP(hipMemcpyAsync(hp + o_hpr, d + L.pr, 1056ull * n, hipMemcpyDeviceToHost, s));
    IK_HIP(hipMemcpyAsync(hp + o_hme, d + L.me, 16ull * n, hipMemcpyDeviceToHost, s));
    IK_HIP(hipMemcpyAsync(hp + o_hhd, d + L.hdr, sizeof(ik_vp8_segment_header) * n, hipMemcpyDeviceToHost, s));
    IK_HIP(hipMemcpyAsync(hp + o_herr, d + L.sync, 8, hipMemcpyDeviceToHost, s));
    IK_HIP(hipStreamSynchronize(s));
    uint32_t err_word = 0;
    std::memcpy(&err_word, hp + o_herr + 4, 4);
    if (err_word) return fail(IK_ERR_DEVICE, "exact WebP coder: a dependency wait timed out on the device");
    const XMB* mbs = reinterpret_cast<const XMB*>(hp);
    const uint8_t* pr = hp + o_hpr;
    const int* me = reinterpret_cast<const int*>(hp + o_hme);
    const ik_vp8_segment_header* hdr = reinterpret_cast<const ik_vp8_segment_header*>(hp + o_hhd);
    outs.resize(n);
    parallel_for(n, n < 16 ? n : 16, [&](int i) {
        XSeg segs[4];
        for (int sg = 0; sg < 4; ++sg) segs[sg] = setup_segment(hdr[i].quant[sg], hdr[i].dq_uv_dc, hdr[i].dq_uv_ac, 50);
        const ImgAt g = at(i);
        write_file(g.w, g.h, mbs + g.mb0, pr + (size_t)1056 * i, hdr[i], me + (size_t)4 * i, segs, outs[i]);
    });
    return IK_OK;
}

}  // namespace

// n images of w x h YUV420 planes on the device (yuv_stride bytes apart) -> the WebP
// files libwebp's WebPEncodeRGB writes at this quality.  Device work on the thread's
// coder stream: segment analysis, set-up, ONE persistent launch for every decision and
// statistics fold, the records back; then the files on the host.
int webp_encode_exact(const uint8_t* d_yuv, size_t yuv_stride, int n, int w, int h, int quality,
                      std::vector<std::vector<uint8_t>>& outs) {
    if (n < 1 || n > 65535 || w < 1 || h < 1 || w > 16383 || h > 16383)
        return fail(IK_ERR_INVALID, "bad WebP shape %dx%d x %d", w, h, n);
    hipStream_t s = nullptr;
    if (int rc = coder_stream(&s)) return rc;
    const XSchedule& sc = exact_schedule(w, h, n);
    XArgs a = uniform_args(d_yuv, yuv_stride, w, h);
    a.use_derr = quality <= 98;  // ERROR_DIFFUSION_QUALITY
    const size_t nmb = (size_t)a.mb_w * a.mb_h, nep = sc.bounds.size() - 1;
    const XTotals t{(size_t)n, nmb * n, nep * n, 1, sc.bounds.size(), 0, sc.tasks.size()};
    const WorkArea L = work_area(t, true);
    uint8_t* d = scratch_slot(kScratchExact, L.bytes);
    if (!d) return fail(IK_ERR_DEVICE, "cannot allocate the exact coder's work area (%zu bytes)", L.bytes);
    if (int rc = upload_constants(d, L, t, &quality, sc.bounds.data(), nullptr, sc.tasks.data(), s)) return rc;
    XRun r{};
    fill_args(d, L, t, a, &r);
    r.nep = (uint32_t)nep;
    // 1. segment analysis (ik_vp8_analysis.hip), 2. set-up, 3. every decision and fold
    IK_HIP(vp8::launch_vp8_analysis(d_yuv, yuv_stride, n, w, h, d + L.alpha, (uint16_t*)(d + L.uva), d + L.kseg,
                                    (vp8::SegRecord*)(d + L.rec), s));
    IK_HIP(launch_vp8x_setup(a, (const vp8::SegRecord*)(d + L.rec), d + L.kseg, (const int*)(d + L.qtab),
                             (ik_vp8_segment_header*)(d + L.hdr), n, s));
    IK_HIP(launch_vp8x_run(a, r, sc.grid, s));
    if (int rc = read_back_and_write(d, L, t, s, [&](int i) { return ImgAt{w, h, nmb * i}; }, outs)) return rc;
    webp_enc_count(0, (unsigned long long)n);
    return IK_OK;
}

// n images of their own sizes and qualities, their planes anywhere in device memory,
// in one set of launches.  Images that all share one geometry and quality go through
// webp_encode_exact itself (gathered first when their planes are unevenly spaced), so a
// geometry never takes two code paths.  For the rest this is webp_encode_exact's driver
// with other totals: the per-MB arrays sized by the sum of the images' MBs, the
// per-epoch ones by the sum of their epochs, a quantiser table per distinct quality, the
// tickets the images' steps merged (merge_steps).  What it alone has is the descriptor
// per image (ik_vp8_gpu.h ImgDesc), which goes up with the constants and gives the
// table-driven kernels each image's planes, geometry and first indices.
int webp_encode_exact_mixed(const ExactItem* items, int n, std::vector<std::vector<uint8_t>>& outs) {
    if (!items || n < 1 || n > 65535) return fail(IK_ERR_INVALID, "bad mixed WebP call of %d images", n);
    bool same = true;
    for (int i = 0; i < n; ++i) {
        const ExactItem& it = items[i];
        if (!it.yuv || it.w < 1 || it.h < 1 || it.w > 16383 || it.h > 16383 || it.quality < 1 || it.quality > 100)
            return fail(IK_ERR_INVALID, "bad WebP item %d: %dx%d at quality %d%s", i, it.w, it.h, it.quality,
                        it.yuv ? "" : ", null planes");
        same = same && it.w == items[0].w && it.h == items[0].h && it.quality == items[0].quality;
    }
    if (same) {
        const int w = items[0].w, h = items[0].h;
        const size_t ysz = yuv420_bytes(w, h);
        // evenly spaced planes as they lie; others gathered a common stride apart
        bool even = n == 1 || (items[1].yuv > items[0].yuv && (size_t)(items[1].yuv - items[0].yuv) >= ysz);
        const size_t step = n > 1 && even ? (size_t)(items[1].yuv - items[0].yuv) : 0;
        for (int i = 2; i < n && even; ++i) even = items[i].yuv == items[0].yuv + step * i;
        if (even) return webp_encode_exact(items[0].yuv, step, n, w, h, items[0].quality, outs);
        hipStream_t ts = thread_stream();
        if (!ts) return fail(IK_ERR_DEVICE, "cannot create HIP stream");
        const size_t stride = (ysz + 255) & ~(size_t)255;
        uint8_t* g = scratch_slot(kScratchExactGather, stride * n);
        if (!g) return fail(IK_ERR_DEVICE, "cannot allocate the gathered planes (%zu bytes)", stride * n);
        for (int i = 0; i < n; ++i) IK_HIP(hipMemcpyAsync(g + stride * i, items[i].yuv, ysz, hipMemcpyDeviceToDevice, ts));
        return webp_encode_exact(g, stride, n, w, h, items[0].quality, outs);
    }
    hipStream_t s = nullptr;
    if (int rc = coder_stream(&s)) return rc;
    // the descriptors, the concatenated epoch bounds, the distinct qualities
    begin_schedule();
    std::vector<const GeomSteps*> geom((size_t)n);
    std::vector<XImg> desc((size_t)n);
    std::vector<int> bounds, quals;
    size_t tot_mb = 0, tot_ep = 0, tot_tasks = 0;
    int max_nmb = 0;
    for (int i = 0; i < n; ++i) {
        const ExactItem& it = items[i];
        const GeomSteps& g = geometry_steps(it.w, it.h);
        geom[(size_t)i] = &g;
        XImg& d = desc[(size_t)i];
        d.yuv = it.yuv;
        d.w = it.w;
        d.h = it.h;
        d.mb_w = (it.w + 15) / 16;
        d.mb_h = (it.h + 15) / 16;
        d.mb0 = (uint32_t)tot_mb;
        d.ep0 = (uint32_t)tot_ep;
        d.bnd0 = (uint32_t)bounds.size();
        d.nep = (uint32_t)g.bounds.size() - 1;
        size_t qi = std::find(quals.begin(), quals.end(), it.quality) - quals.begin();
        if (qi == quals.size()) quals.push_back(it.quality);
        d.qtab = (uint32_t)qi;
        d.use_derr = it.quality <= 98;  // ERROR_DIFFUSION_QUALITY
        bounds.insert(bounds.end(), g.bounds.begin(), g.bounds.end());
        const int nmb = d.mb_w * d.mb_h;
        max_nmb = std::max(max_nmb, nmb);
        tot_mb += (size_t)nmb;
        tot_ep += d.nep;
        tot_tasks += g.tasks.size();
        if (tot_mb > 0x7fffffffu || tot_tasks > 0x7fffffffu)
            return fail(IK_ERR_INVALID, "mixed WebP call of more than 2^31 macroblocks");
    }
    static thread_local std::vector<uint64_t> tasks;
    const int widest = merge_steps(geom, tasks);
    const int grid = schedule_grid(widest, tasks.size());
    const XTotals t{(size_t)n, tot_mb, tot_ep, quals.size(), bounds.size(), sizeof(XImg) * n, tasks.size()};
    const WorkArea L = work_area(t, true);
    uint8_t* d = scratch_slot(kScratchExact, L.bytes);
    if (!d) return fail(IK_ERR_DEVICE, "cannot allocate the exact coder's work area (%zu bytes)", L.bytes);
    if (int rc = upload_constants(d, L, t, quals.data(), bounds.data(), desc.data(), tasks.data(), s)) return rc;
    XArgs a{};  // (planes and geometry: per image, from the descriptors)
    XRun r{};
    fill_args(d, L, t, a, &r);
    const XImg* dimgs = (const XImg*)(d + L.desc);
    IK_HIP(vp8::launch_vp8_analysis_mixed(dimgs, n, max_nmb, d + L.alpha, (uint16_t*)(d + L.uva), d + L.kseg,
                                          (vp8::SegRecord*)(d + L.rec), s));
    IK_HIP(launch_vp8x_setup_mixed(a, dimgs, (const vp8::SegRecord*)(d + L.rec), d + L.kseg, (const int*)(d + L.qtab),
                                   (ik_vp8_segment_header*)(d + L.hdr), n, s));
    IK_HIP(launch_vp8x_run_mixed(a, r, dimgs, grid, s));
    auto at = [&](int i) { return ImgAt{items[i].w, items[i].h, desc[(size_t)i].mb0}; };
    if (int rc = read_back_and_write(d, L, t, s, at, outs)) return rc;
    webp_enc_count(1, (unsigned long long)n);
    webp_enc_count(3, 1);
    return IK_OK;
}

// The exact coder's first two stages alone (ik_vp8_analyze_device): libwebp's segment
// analysis and the segment set-up on the device, the final segment map and headers
// into host memory; on the calling thread's stream, waits.
int vp8_analyze_setup(const uint8_t* d_yuv, size_t yuv_stride, int n, int w, int h, float quality, uint8_t* seg,
                      ik_vp8_segment_header* hdr) {
    hipStream_t s = thread_stream();
    if (!s) return fail(IK_ERR_DEVICE, "cannot create HIP stream");
    XArgs a = uniform_args(d_yuv, yuv_stride, w, h);
    XTotals t{};
    t.n = (size_t)n;
    t.mb = (size_t)a.mb_w * a.mb_h * n;
    t.quals = 1;
    const WorkArea L = work_area(t, false);
    uint8_t* d = scratch_slot(kScratchExact, L.bytes);
    if (!d) return fail(IK_ERR_DEVICE, "cannot allocate the segment analysis' work area (%zu bytes)", L.bytes);
    uint8_t* hc = pinned_slot(kPinnedExactIn, 4 * 255);
    if (!hc) return IK_ERR_NOMEM;
    segment_quant_table(quality, reinterpret_cast<int*>(hc));  // (a float here: staged apart from upload_constants)
    IK_HIP(hipMemcpyAsync(d + L.qtab, hc, 4 * 255, hipMemcpyHostToDevice, s));
    fill_args(d, L, t, a, nullptr);
    IK_HIP(vp8::launch_vp8_analysis(d_yuv, yuv_stride, n, w, h, d + L.alpha, (uint16_t*)(d + L.uva), d + L.kseg,
                                    (vp8::SegRecord*)(d + L.rec), s));
    IK_HIP(launch_vp8x_setup(a, (const vp8::SegRecord*)(d + L.rec), d + L.kseg, (const int*)(d + L.qtab),
                             (ik_vp8_segment_header*)(d + L.hdr), n, s));
    IK_HIP(hipMemcpyAsync(seg, d + L.seg, t.mb, hipMemcpyDeviceToHost, s));
    IK_HIP(hipMemcpyAsync(hdr, d + L.hdr, sizeof(ik_vp8_segment_header) * n, hipMemcpyDeviceToHost, s));
    IK_HIP(hipStreamSynchronize(s));
    return IK_OK;
}

}  // namespace ik

using namespace ik;

// The files as malloc'd C outputs, all or nothing: on an allocation failure nothing is
// left for the caller to free and outs / out_lens are not written.
static int files_to_c_outputs(const std::vector<std::vector<uint8_t>>& files, uint8_t** outs, size_t* out_lens) {
    const size_t n = files.size();
    std::vector<uint8_t*> mem(n, nullptr);
    for (size_t i = 0; i < n; ++i) {
        mem[i] = (uint8_t*)malloc(files[i].size() ? files[i].size() : 1);
        if (!mem[i]) {
            for (size_t j = 0; j < i; ++j) free(mem[j]);
            return fail(IK_ERR_NOMEM, "out of host memory");
        }
        std::memcpy(mem[i], files[i].data(), files[i].size());
    }
    for (size_t i = 0; i < n; ++i) {
        outs[i] = mem[i];
        out_lens[i] = files[i].size();
    }
    return IK_OK;
}

extern "C" int ik_webp_encode_exact_device(const uint8_t* dev_yuv, size_t yuv_stride, uint32_t n, uint32_t w,
                                           uint32_t h, int quality, uint8_t** outs, size_t* out_lens) {
    IK_API_ENTER();
    if (!dev_yuv || !outs || !out_lens) return fail(IK_ERR_INVALID, "null pointer");
    const size_t ysz = yuv420_bytes(w, h);
    if (n > 1 && yuv_stride < ysz) return fail(IK_ERR_INVALID, "image stride %zu under the planes' %zu bytes", yuv_stride, ysz);
    std::vector<std::vector<uint8_t>> files;
    if (int rc = webp_encode_exact(dev_yuv, yuv_stride, (int)n, (int)w, (int)h, clamp_quality(quality), files)) return rc;
    return files_to_c_outputs(files, outs, out_lens);
}

extern "C" int ik_webp_encode_exact_items(const ik_webp_exact_item* items, uint32_t n, uint8_t** outs,
                                          size_t* out_lens) {
    IK_API_ENTER();
    if (!items || !outs || !out_lens) return fail(IK_ERR_INVALID, "null pointer");
    if (n < 1 || n > 65535) return fail(IK_ERR_INVALID, "bad WebP item count %u", n);
    std::vector<ExactItem> it(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (!items[i].dev_yuv || items[i].w < 1 || items[i].h < 1 || items[i].w > 16383 || items[i].h > 16383)
            return fail(IK_ERR_INVALID, "bad WebP item %u: %ux%u%s", i, items[i].w, items[i].h,
                        items[i].dev_yuv ? "" : ", null planes");
        it[i] = ExactItem{items[i].dev_yuv, (int)items[i].w, (int)items[i].h, clamp_quality(items[i].quality)};
    }
    std::vector<std::vector<uint8_t>> files;
    if (int rc = webp_encode_exact_mixed(it.data(), (int)n, files)) return rc;
    return files_to_c_outputs(files, outs, out_lens);
}

extern "C" long long ik_webp_exact_plan(const uint32_t* w, const uint32_t* h, uint32_t n, uint64_t* tasks, size_t cap,
                                        uint32_t* grid) {
    if (!w || !h || n < 1 || n > 65535 || (cap && !tasks)) {
        fail(IK_ERR_INVALID, "bad WebP plan arguments");
        return -1;
    }
    begin_schedule();
    std::vector<const GeomSteps*> geom(n);
    for (uint32_t i = 0; i < n; ++i) {
        if (w[i] < 1 || h[i] < 1 || w[i] > 16383 || h[i] > 16383) {
            fail(IK_ERR_INVALID, "bad WebP plan size %ux%u", w[i], h[i]);
            return -1;
        }
        geom[i] = &geometry_steps((int)w[i], (int)h[i]);
    }
    std::vector<uint64_t> t;
    const int widest = merge_steps(geom, t);
    if (grid) *grid = (uint32_t)schedule_grid(widest, t.size());
    if (cap) std::memcpy(tasks, t.data(), 8 * std::min(cap, t.size()));
    return (long long)t.size();
}
