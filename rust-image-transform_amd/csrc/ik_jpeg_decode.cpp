// ik_jpeg_decode.cpp -- JPEG branch of decode_image (reference src/transform.rs:31 ->
// image 0.25.8 -> zune-jpeg 0.4.21, Cargo.lock:3106), host half.
//
// The host parses the markers and runs the Huffman entropy decoder into a dense
// block-coefficient image (quantised int16, natural order, one plane of 8x8
// blocks per component): baseline sequential (SOF0/SOF1, interleaved or not) and
// progressive (SOF2: DC first/refine, AC first/refine with EOB runs), restart
// intervals, 8-bit, 1 (gray -> L8), 3 (YCbCr -> Rgb8, or RGB for Adobe
// transform 0) or 4 components (CMYK / YCCK -> Rgb8).  Reconstruction --
// dequantise, IDCT, chroma upsampling, colour conversion -- runs on the GPU
// (ik_jpeg.hip) straight into the device image, by default as zune-jpeg 0.4.21
// does it (restated, parity unpinned: no crate sources or outputs here; equal to
// oracle/jpeg_dec.c), or as libjpeg-turbo does (bit-exact with Pillow) --
// ik_set_jpeg_reconstruction.  Arithmetic-coded, lossless, hierarchical and
// 12-bit JPEGs report IK_ERR_UNSUPPORTED.
#include <algorithm>
#include <thread>
#include <memory>
#include <atomic>
#include <cstdlib>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>
#include <array>
#include <mutex>
#include <condition_variable>
#include <map>

#include "../../include/imagekit_hip.h"
#include "ik_png.h"
#include "ik_runtime.h"
#include "ik_jpeg_walk.h"
#include "ik_jsync_plan.h"

namespace ik {
namespace {

const uint8_t kZigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,
                             12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
                             35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51,
                             58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

struct BitReader {
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc = 0;
    int n = 0;
    bool marker_hit = false;
    void fill() {
        while (n <= 56) {
            uint8_t b = 0;
            if (!marker_hit && p < end) {
                b = *p;
                if (b == 0xFF) {
                    const uint8_t nx = p + 1 < end ? p[1] : 0;
                    if (nx == 0x00) { p += 2; }
                    else { marker_hit = true; b = 0; }  // feed zeros past a marker
                } else {
                    ++p;
                }
            }
            acc |= (uint64_t)b << (56 - n);
            n += 8;
        }
    }
    inline int peek(int k) { if (n < k) fill(); return (int)(acc >> (64 - k)); }
    inline void skip(int k) { acc <<= k; n -= k; }
    inline int get(int k) { if (!k) return 0; const int v = peek(k); skip(k); return v; }
    void reset_at_marker() { acc = 0; n = 0; marker_hit = false; }
};

inline int extend(int v, int t) { return v < (1 << (t - 1)) ? v - (1 << t) + 1 : v; }

int decode_symbol(BitReader& br, const HuffTable& t) {
    const int look = br.peek(9);
    const int l = t.look_len[look];
    if (l) { br.skip(l); return t.look_val[look]; }
    int code = br.peek(16);
    for (int len = 10; len <= 16; ++len) {
        const int c = code >> (16 - len);
        if (t.maxcode[len] >= 0 && c <= t.maxcode[len] && c >= t.mincode[len]) {
            br.skip(len);
            return t.vals[t.valptr[len] + c - t.mincode[len]];
        }
    }
    return -1;
}

struct Component {
    int id = 0, h = 1, v = 1, tq = 0, td = 0, ta = 0;
    int bw = 0, bh = 0;    // blocks across/down, padded to whole MCUs
    int dw = 0, dh = 0;    // downsampled width/height (libjpeg downsampled_width/height)
    size_t blk0 = 0;       // first block in the coefficient image
    int pred = 0;
};

const char* const kFmtErr = "Format error decoding Jpeg";

// Baseline scans go to the self-synchronising GPU decoder (ik_jsync.hip) from this
// size up; smaller ones are faster on the host entropy decoder.
constexpr size_t kJsyncMinBytes = 4 << 10;
static_assert(jwalk::kMinScan == kJsyncMinBytes, "the marker walk keeps the same scans on the host decoder");

// Progressive scans with restart intervals on the GPU (k_jpeg_prog);
// IK_JPEG_PROG=0 keeps them on the host entropy decoder.
bool prog_enabled() {
    static const bool on = [] {
        const char* e = getenv("IK_JPEG_PROG");
        return !(e && !strcmp(e, "0"));
    }();
    return on;
}

}  // namespace

std::atomic<int> g_jpeg_prog_free{-1};  // ik_set_jpeg_prog_free; -1: IK_JPEG_PROG_FREE, read per file

// Progressive files without restart markers: IK_JPEG_PROG_FREE=gpu / ik_set_jpeg_prog_free
// sends their scans to the GPU (the Ah = 0 scans through the self-synchronising
// decoder, DC refinement a bit per block, AC refinement a serial chain per
// component); the default keeps them on the host entropy decoder.
bool jpeg_prog_free_gpu() {
    const int m = g_jpeg_prog_free.load();
    if (m >= 0) return m == IK_JPEG_PROG_FREE_GPU;
    const char* e = getenv("IK_JPEG_PROG_FREE");
    return e && !strcmp(e, "gpu");
}

namespace {

struct Decoder {
    const uint8_t* b;
    const uint8_t* end;
    uint16_t qt[4][64] = {};
    HuffTable dc[4], ac[4];
    std::vector<Component> comps;
    int width = 0, height = 0, restart = 0, hmax = 1, vmax = 1, mcux = 0, mcuy = 0;
    bool have_frame = false, progressive = false, adobe = false;
    int adobe_transform = -1;
    std::vector<int16_t> coef;  // [block][64], natural order, quantised (host-decoded scans only)
    size_t nblocks = 0;
    int eobrun = 0;
    // GPU entropy decoding of a baseline scan with restart intervals: the scan is
    // recorded here (segment starts = first byte after each RSTn) instead of decoded
    bool try_gpu = false, deferred = false, need_host = false, scanned = false;
    const uint8_t* gpu_data = nullptr;
    std::vector<unsigned> gpu_segs;
    JpegScanArgs gpu_scan{};
    // progressive scans with restart intervals, recorded for k_jpeg_prog (all of
    // the image's scans, in order: one the GPU cannot take sends the image to the
    // host decoder, or keeps it there from the first scan on)
    struct ProgScan {
        JpegScanArgs a;
        std::vector<unsigned> segs;
        JpegHuffTables tabs;
    };
    std::vector<ProgScan> prog;
    bool prog_host = false;
    // a baseline scan for the self-synchronising GPU decoder (ik_jsync.hip): its
    // entropy-coded bytes (stuffed, with any RSTn markers) and geometry
    bool js = false;
    const uint8_t* js_data = nullptr;
    size_t js_len = 0;
    long long js_nivl = 0;  // restart intervals the frame must have
    // a file decoded where it lies in device memory: b..end is its skeleton (the
    // segments up to the first SOS header), the scan is [ent_off, eoi_off) of the
    // file on the device, and nothing here can be decoded on the host -- whatever the
    // self-synchronising decoder does not take sets need_host (the file is copied back)
    const JpegInPlace* skel = nullptr;
    jsync::Scan js_scan{};  // geometry (device pointers filled at launch)
    // a progressive file without restart markers for the GPU (jpeg_prog_free_gpu):
    // every scan recorded, in file order, with the Huffman tables as they stand at
    // its SOS; pf once the whole file is recorded and large enough (finish)
    struct FreeScan {
        jsync::Scan geom;
        JpegHuffTables tabs;
        const uint8_t* data;  // entropy-coded bytes, up to the marker that ends the scan
        size_t len;
        int comp;             // the (first) component
    };
    std::vector<FreeScan> pf_scans;
    bool pf = false;
    uint64_t pf_first[4] = {};  // per component: the coefficients (zigzag index) an Ah = 0 scan has coded

    void ensure_coef() {
        if (coef.empty()) coef.assign(nblocks * 64, 0);
    }

    int16_t* block(const Component& c, int bx, int by) { return &coef[(c.blk0 + (size_t)by * c.bw + bx) * 64]; }

    int frame(const uint8_t* s, int m) {
        if (have_frame) return fail(IK_ERR_TRANSFORM, "%s: duplicate SOF", kFmtErr);
        if (s[0] != 8) return fail(IK_ERR_UNSUPPORTED, "%d-bit JPEG is not supported", s[0]);
        progressive = m == 0xC2;
        height = (int)s[1] << 8 | s[2];
        width = (int)s[3] << 8 | s[4];
        const int nc = s[5];
        if (!width || !height) return fail(IK_ERR_TRANSFORM, "%s: zero dimension", kFmtErr);
        if (nc != 1 && nc != 3 && nc != 4)
            return fail(IK_ERR_UNSUPPORTED, "JPEG with %d components is not supported", nc);
        // image's default Limits: max_alloc 512 MiB of decoded bytes (L8: 1 per pixel, Rgb8: 3)
        if ((uint64_t)width * height * (nc == 1 ? 1u : 3u) > (512ull << 20))
            return fail(IK_ERR_TRANSFORM, "Limits are exceeded");
        comps.resize(nc);
        for (int i = 0; i < nc; ++i) {
            comps[i].id = s[6 + 3 * i];
            comps[i].h = s[7 + 3 * i] >> 4;
            comps[i].v = s[7 + 3 * i] & 15;
            comps[i].tq = s[8 + 3 * i] & 3;
            if (comps[i].h < 1 || comps[i].h > 4 || comps[i].v < 1 || comps[i].v > 4)
                return fail(IK_ERR_TRANSFORM, "%s: bad sampling factors", kFmtErr);
            hmax = std::max(hmax, comps[i].h);
            vmax = std::max(vmax, comps[i].v);
        }
        for (auto& c : comps)
            if (hmax % c.h || vmax % c.v)
                return fail(IK_ERR_UNSUPPORTED, "fractional JPEG chroma sampling is not supported");
        mcux = (width + 8 * hmax - 1) / (8 * hmax);
        mcuy = (height + 8 * vmax - 1) / (8 * vmax);
        size_t blocks = 0;
        for (auto& c : comps) {
            c.bw = mcux * c.h;
            c.bh = mcuy * c.v;
            c.dw = (width * c.h + hmax - 1) / hmax;
            c.dh = (height * c.v + vmax - 1) / vmax;
            c.blk0 = blocks;
            blocks += (size_t)c.bw * c.bh;
        }
        nblocks = blocks;
        have_frame = true;
        return IK_OK;
    }

    // one block of one scan (ITU T.81 F.2.2 / G.1.2; libjpeg jdhuff.c / jdphuff.c)
    int block_baseline(BitReader& br, Component& c, int16_t* blk) {
        const int t = decode_symbol(br, dc[c.td]);
        if (t < 0 || t > 11) return fail(IK_ERR_TRANSFORM, "%s: bad DC code", kFmtErr);
        c.pred += t ? extend(br.get(t), t) : 0;
        blk[0] = (int16_t)c.pred;
        for (int k = 1; k < 64;) {
            const int rs = decode_symbol(br, ac[c.ta]);
            if (rs < 0) return fail(IK_ERR_TRANSFORM, "%s: bad AC code", kFmtErr);
            const int r = rs >> 4, sz = rs & 15;
            if (!sz) {
                if (r != 15) break;  // EOB
                k += 16;
                continue;
            }
            k += r;
            if (k > 63) return fail(IK_ERR_TRANSFORM, "%s: AC overflow", kFmtErr);
            blk[kZigzag[k]] = (int16_t)extend(br.get(sz), sz);
            ++k;
        }
        return IK_OK;
    }
    int block_dc_first(BitReader& br, Component& c, int16_t* blk, int Al) {
        const int t = decode_symbol(br, dc[c.td]);
        if (t < 0 || t > 11) return fail(IK_ERR_TRANSFORM, "%s: bad DC code", kFmtErr);
        c.pred += t ? extend(br.get(t), t) : 0;
        blk[0] = (int16_t)(c.pred * (1 << Al));
        return IK_OK;
    }
    void block_dc_refine(BitReader& br, int16_t* blk, int Al) {
        if (br.get(1)) blk[0] = (int16_t)(blk[0] | (1 << Al));
    }
    int block_ac_first(BitReader& br, const Component& c, int16_t* blk, int Ss, int Se, int Al) {
        if (eobrun > 0) { --eobrun; return IK_OK; }
        for (int k = Ss; k <= Se; ++k) {
            const int rs = decode_symbol(br, ac[c.ta]);
            if (rs < 0) return fail(IK_ERR_TRANSFORM, "%s: bad AC code", kFmtErr);
            const int r = rs >> 4, sz = rs & 15;
            if (sz) {
                k += r;
                if (k > Se) return fail(IK_ERR_TRANSFORM, "%s: AC overflow", kFmtErr);
                blk[kZigzag[k]] = (int16_t)(extend(br.get(sz), sz) * (1 << Al));
            } else if (r == 15) {
                k += 15;
            } else {
                eobrun = 1 << r;
                if (r) eobrun += br.get(r);
                --eobrun;
                break;
            }
        }
        return IK_OK;
    }
    int block_ac_refine(BitReader& br, const Component& c, int16_t* blk, int Ss, int Se, int Al) {
        const int p1 = 1 << Al, m1 = -1 * (1 << Al);
        auto refine = [&](int16_t* co) {
            if (br.get(1) && (*co & p1) == 0) *co = (int16_t)(*co >= 0 ? *co + p1 : *co + m1);
        };
        int k = Ss;
        if (eobrun == 0) {
            for (; k <= Se; ++k) {
                const int rs = decode_symbol(br, ac[c.ta]);
                if (rs < 0) return fail(IK_ERR_TRANSFORM, "%s: bad AC code", kFmtErr);
                int r = rs >> 4, sz = rs & 15, val = 0;
                if (sz) {
                    if (sz != 1) return fail(IK_ERR_TRANSFORM, "%s: bad AC refinement", kFmtErr);
                    val = br.get(1) ? p1 : m1;
                } else if (r != 15) {
                    eobrun = 1 << r;
                    if (r) eobrun += br.get(r);
                    break;  // the rest of the band goes to the EOB-run pass below
                }
                // skip r zero-history coefficients, refining the nonzero ones passed
                do {
                    int16_t* co = blk + kZigzag[k];
                    if (*co != 0) refine(co);
                    else if (--r < 0) break;
                    ++k;
                } while (k <= Se);
                if (val) {
                    if (k > Se) return fail(IK_ERR_TRANSFORM, "%s: AC overflow", kFmtErr);
                    blk[kZigzag[k]] = (int16_t)val;
                }
            }
        }
        if (eobrun > 0) {
            for (; k <= Se; ++k) {
                int16_t* co = blk + kZigzag[k];
                if (*co != 0) refine(co);
            }
            --eobrun;
        }
        return IK_OK;
    }

    // Record a baseline scan for k_jpeg_huff: find its restart markers (the end of
    // the scan is the first other marker).  False (decode on the host) when the
    // marker count does not match the MCU count.
    bool defer_scan(const std::vector<int>& order, const uint8_t* data, const uint8_t*& next) {
        const bool single = order.size() == 1;
        const Component& c0 = comps[order[0]];
        const int single_bw = (c0.dw + 7) / 8, single_bh = (c0.dh + 7) / 8;
        const long long total_mcu = single ? (long long)single_bw * single_bh : (long long)mcux * mcuy;
        const long long want = (total_mcu + restart - 1) / restart;
        gpu_segs.assign(1, 0u);
        const uint8_t* q = data;
        while (q + 1 < end) {
            if (q[0] != 0xFF) {  // to the next 0xFF (memchr: entropy-coded data holds ~1 in 256 bytes)
                const void* f = std::memchr(q, 0xFF, (size_t)(end - 1 - q));
                if (!f) { q = end - 1; break; }
                q = static_cast<const uint8_t*>(f);
            }
            const uint8_t m = q[1];
            if (m == 0x00) { q += 2; continue; }
            if (m == 0xFF) { ++q; continue; }
            if (m >= 0xD0 && m <= 0xD7) {
                if ((long long)gpu_segs.size() >= want) break;  // a marker past the last interval: let the host judge
                gpu_segs.push_back((unsigned)(q + 2 - data));
                q += 2;
                continue;
            }
            break;
        }
        if ((long long)gpu_segs.size() != want || (size_t)(end - data) > 0xffffffffu) return false;
        JpegScanArgs& a = gpu_scan;
        a = JpegScanArgs{};
        a.size = (long long)(end - data);
        a.n_seg = (int)want;
        a.restart = restart;
        a.total_mcu = total_mcu;
        a.mcux = mcux;
        a.single = single ? 1 : 0;
        a.single_bw = single_bw;
        a.ns = (int)order.size();
        for (int i = 0; i < a.ns; ++i) {
            const Component& c = comps[order[i]];
            a.h[i] = c.h; a.v[i] = c.v; a.bw[i] = c.bw; a.td[i] = c.td; a.ta[i] = c.ta;
            a.blk0[i] = (long long)c.blk0;
        }
        gpu_data = data;
        deferred = true;
        next = q;
        return true;
    }

    // Record a progressive scan with restart intervals for k_jpeg_prog, as
    // defer_scan records a baseline one; a.data holds the scan's offset in the file.
    bool defer_prog(const std::vector<int>& order, int kind, int Ss, int Se, int Al, const uint8_t* data,
                    const uint8_t*& next) {
        const uint8_t* nx = next;
        std::vector<unsigned> keep;
        keep.swap(gpu_segs);
        const bool ok = defer_scan(order, data, nx);
        deferred = false;  // (defer_scan's single-scan record is not used)
        ProgScan ps;
        ps.segs.swap(gpu_segs);
        gpu_segs.swap(keep);
        if (!ok) return false;
        ps.a = gpu_scan;
        ps.a.data = reinterpret_cast<const uint8_t*>((uintptr_t)(data - b));
        ps.a.kind = kind;
        ps.a.Ss = Ss;
        ps.a.Se = Se;
        ps.a.Al = Al;
        tables(ps.tabs);
        prog.push_back(std::move(ps));
        next = nx;
        return true;
    }

    // Record a baseline scan for the self-synchronising GPU decoder: its bytes run
    // to the file's final EOI marker (the GPU's unstuffing flags any other marker
    // inside them, and counts the restart markers against the frame's intervals;
    // either mismatch sends the image to the host decoder, which reports png's --
    // zune-jpeg's -- error).
    // the self-synchronising decoder's geometry of a scan over the components `order`
    bool scan_geom(const std::vector<int>& order, jsync::Scan& a, long long& total_mcu) const {
        jsync::CompGeom cg[4];
        for (size_t i = 0; i < comps.size(); ++i) {
            const Component& c = comps[i];
            cg[i] = jsync::CompGeom{c.h, c.v, c.bw, c.dw, c.dh, c.td, c.ta, (long long)c.blk0};
        }
        return jsync::scan_geom(cg, order.data(), (int)order.size(), mcux, mcuy, a, total_mcu);
    }

    // Record a scan of a progressive file without restart markers: its bytes run to
    // the first marker (fill bytes before it dropped, as the host reader feeds zeros
    // from a marker's first FF on).  False: a scan the GPU path does not take (more
    // blocks per MCU than a lane state holds, or an RSTn inside it).
    bool defer_free(const std::vector<int>& order, int kind, int Ss, int Se, int Al, const uint8_t* data,
                    const uint8_t*& next) {
        // The GPU runs an image's Ah = 0 scans together and its refinements after them,
        // the host decoder every scan in file order.  The two agree when no coefficient
        // is coded by two first scans and every refinement follows the first scan of
        // its whole band (T.81 G.1.1.1.1 asks for as much); any other file is the host's.
        const uint64_t band = (Se == 63 ? ~0ull : (1ull << (Se + 1)) - 1) & ~((1ull << Ss) - 1);
        const bool first = kind == jsync::kDcFirst || kind == jsync::kAcFirst;
        for (int c : order)
            if (first ? (pf_first[c] & band) != 0 : (pf_first[c] & band) != band) return false;
        if (first)
            for (int c : order) pf_first[c] |= band;
        pf_scans.emplace_back();
        FreeScan& fs = pf_scans.back();
        long long total_mcu = 0;
        bool good = scan_geom(order, fs.geom, total_mcu);
        const uint8_t* q = data;
        bool at_marker = false;
        while (good && q + 1 < end) {
            if (q[0] != 0xFF) {
                const void* f = std::memchr(q, 0xFF, (size_t)(end - 1 - q));
                if (!f) break;
                q = static_cast<const uint8_t*>(f);
            }
            const uint8_t m = q[1];
            if (m == 0x00) { q += 2; continue; }
            if (m == 0xFF) { ++q; continue; }
            at_marker = true;
            if (m >= 0xD0 && m <= 0xD7) good = false;
            break;
        }
        if (!good || (size_t)(end - data) > 0xffffffffu) {
            pf_scans.pop_back();
            return false;
        }
        const uint8_t* e = at_marker ? q : end;
        if (at_marker)
            while (e > data && e[-1] == 0xFF) --e;
        fs.geom.kind = kind;
        fs.geom.Ss = Ss;
        fs.geom.Se = Se;
        fs.geom.Al = Al;
        fs.data = data;
        fs.len = (size_t)(e - data);
        fs.comp = order[0];
        tables(fs.tabs);
        next = at_marker ? q : end;
        return true;
    }

    // after parse(): a recorded restart-free progressive file goes to the GPU when its
    // entropy-coded bytes, over all scans, reach the baseline path's threshold
    void finish() {
        if (pf_scans.empty() || need_host) return;
        size_t total = 0;
        for (const FreeScan& f : pf_scans) total += f.len;
        if (total >= kJsyncMinBytes) pf = true;
        else need_host = true;
    }

    bool defer_jsync(const std::vector<int>& order, const uint8_t* data, const uint8_t*& next) {
        jsync::Scan a{};
        long long total_mcu = 0;
        if (!scan_geom(order, a, total_mcu)) return false;
        // the scan's end: the last FF D9 of the file (trailing bytes after EOI are
        // ignored, as the parser ignores them), else the file's end
        const uint8_t* e = end;
        if (!skel)
            for (const uint8_t* q = end - 2; q >= data && q >= end - 4096; --q)
                if (q[0] == 0xFF && q[1] == 0xD9) { e = q; break; }
        // (a file in device memory: the walk made the same search, jwalk::walk_file)
        const size_t len = skel ? (size_t)(skel->eoi_off - skel->ent_off) : (size_t)(e - data);
        if (len < kJsyncMinBytes) return false;
        if (restart) a.ivl_blocks = (long long)restart * a.bpm;
        js_scan = a;
        js_nivl = restart ? (total_mcu + restart - 1) / restart : 1;
        js_data = skel ? nullptr : data;
        js_len = len;
        js = true;
        deferred = true;
        next = e;
        return true;
    }

    void tables(JpegHuffTables& t) const { pack_tables(dc, ac, t); }

    int scan(const uint8_t* s, const uint8_t* se, const uint8_t*& next) {
        if (!have_frame) return fail(IK_ERR_TRANSFORM, "%s: SOS before SOF", kFmtErr);
        const int ns = s[0];
        if (ns < 1 || ns > (int)comps.size() || se - s < 1 + 2 * ns + 3)
            return fail(IK_ERR_TRANSFORM, "%s: bad SOS", kFmtErr);
        std::vector<int> order(ns);
        for (int i = 0; i < ns; ++i) {
            const int cid = s[1 + 2 * i];
            int k = -1;
            for (int j = 0; j < (int)comps.size(); ++j) if (comps[j].id == cid) k = j;
            if (k < 0) return fail(IK_ERR_TRANSFORM, "%s: bad scan component", kFmtErr);
            comps[k].td = s[2 + 2 * i] >> 4;
            comps[k].ta = s[2 + 2 * i] & 15;
            if (comps[k].td > 3 || comps[k].ta > 3) return fail(IK_ERR_TRANSFORM, "%s: bad table id", kFmtErr);
            order[i] = k;
        }
        const int Ss = s[1 + 2 * ns], Se = s[2 + 2 * ns], Ah = s[3 + 2 * ns] >> 4, Al = s[3 + 2 * ns] & 15;
        // kind: 0 baseline, 1 DC first, 2 DC refine, 3 AC first, 4 AC refine
        int kind = 0;
        if (progressive) {
            if (Ss == 0) {
                if (Se != 0) return fail(IK_ERR_TRANSFORM, "%s: bad progressive DC scan", kFmtErr);
                kind = Ah ? 2 : 1;
            } else {
                if (Se < Ss || Se > 63 || ns != 1) return fail(IK_ERR_TRANSFORM, "%s: bad progressive AC scan", kFmtErr);
                kind = Ah ? 4 : 3;
            }
            if (Al > 13) return fail(IK_ERR_TRANSFORM, "%s: bad successive approximation", kFmtErr);
        }
        for (int i = 0; i < ns; ++i) {
            const Component& c = comps[order[i]];
            const bool need_dc = kind == 0 || kind == 1, need_ac = kind == 0 || kind >= 3;
            if ((need_dc && !dc[c.td].present) || (need_ac && !ac[c.ta].present))
                return fail(IK_ERR_TRANSFORM, "%s: missing Huffman table", kFmtErr);
        }
        if (deferred) {  // a second scan: the whole image goes through the host decoder
            need_host = true;
            return IK_OK;
        }
        if (try_gpu && progressive && !skel && !prog_host && prog_enabled()) {
            scanned = true;
            // no restart interval in force at any scan: the file is recorded for the
            // GPU where the switch says so; a scan that cannot be, or a restart
            // interval after recorded scans, sends every scan to the host
            if (!pf_scans.empty() || (restart == 0 && prog.empty() && jpeg_prog_free_gpu())) {
                if (restart == 0 && defer_free(order, kind, Ss, Se, Al, se, next)) return IK_OK;
                if (!pf_scans.empty()) {
                    need_host = true;
                    return IK_OK;
                }
            }
            if (restart > 0 && defer_prog(order, kind, Ss, Se, Al, se, next)) return IK_OK;
            if (!prog.empty()) {  // a later scan the GPU cannot take: all scans on the host
                need_host = true;
                return IK_OK;
            }
            prog_host = true;  // the first scan: this and every later one on the host
        }
        const bool first_scan = !scanned;
        scanned = true;
        if (try_gpu && first_scan && kind == 0 && ns == (int)comps.size() && defer_jsync(order, se, next))
            return IK_OK;
        if (skel) {  // the scan's bytes are not on the host
            need_host = true;
            return IK_OK;
        }
        ensure_coef();
        for (auto& c : comps) c.pred = 0;
        eobrun = 0;
        BitReader br{se, end};
        const bool single = ns == 1;
        const Component& c0 = comps[order[0]];
        const int single_bw = (c0.dw + 7) / 8, single_bh = (c0.dh + 7) / 8;
        const long total_mcu = single ? (long)single_bw * single_bh : (long)mcux * mcuy;
        auto do_block = [&](Component& c, int16_t* blk) -> int {
            switch (kind) {
            case 0: return block_baseline(br, c, blk);
            case 1: return block_dc_first(br, c, blk, Al);
            case 2: block_dc_refine(br, blk, Al); return IK_OK;
            case 3: return block_ac_first(br, c, blk, Ss, Se, Al);
            default: return block_ac_refine(br, c, blk, Ss, Se, Al);
            }
        };
        for (long mcu = 0; mcu < total_mcu; ++mcu) {
            if (restart && mcu > 0 && mcu % restart == 0) {
                // expect RSTn: realign to the marker, reset predictors and EOB run
                const uint8_t* q = br.p;
                while (q + 1 < end && !(q[0] == 0xFF && q[1] >= 0xD0 && q[1] <= 0xD7)) ++q;
                if (q + 1 >= end) return fail(IK_ERR_TRANSFORM, "%s: missing restart marker", kFmtErr);
                br.p = q + 2;
                br.reset_at_marker();
                for (auto& c : comps) c.pred = 0;
                eobrun = 0;
            }
            if (single) {
                Component& c = comps[order[0]];
                const int st = do_block(c, block(c, (int)(mcu % single_bw), (int)(mcu / single_bw)));
                if (st) return st;
                continue;
            }
            const int mx = (int)(mcu % mcux), my = (int)(mcu / mcux);
            for (int oi = 0; oi < ns; ++oi) {
                Component& c = comps[order[oi]];
                for (int by = 0; by < c.v; ++by)
                    for (int bx = 0; bx < c.h; ++bx) {
                        const int st = do_block(c, block(c, mx * c.h + bx, my * c.v + by));
                        if (st) return st;
                    }
            }
        }
        next = br.p;
        return IK_OK;
    }

    int parse() {
        const uint8_t* p = b + 2;
        auto be16 = [](const uint8_t* q) { return (int)q[0] << 8 | q[1]; };
        for (;;) {
            while (p < end && *p != 0xFF) ++p;  // tolerate garbage between segments
            while (p < end && *p == 0xFF) ++p;
            if (p >= end || *p == 0xD9) {
                if (scanned) return IK_OK;  // EOI (or a stream cut after its last scan)
                return fail(IK_ERR_TRANSFORM, "%s: no SOS", kFmtErr);
            }
            const uint8_t m = *p++;
            if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
            if (p + 2 > end) return fail(IK_ERR_TRANSFORM, "%s: truncated", kFmtErr);
            const int len = be16(p);
            if (len < 2 || p + len > end) return fail(IK_ERR_TRANSFORM, "%s: bad segment length", kFmtErr);
            const uint8_t* s = p + 2;
            const uint8_t* se = p + len;
            if (m == 0xDB) {  // DQT
                while (s < se) {
                    const int pq = s[0] >> 4, tq = s[0] & 15;
                    if (tq > 3 || s + 1 + (pq ? 128 : 64) > se) return fail(IK_ERR_TRANSFORM, "%s: bad DQT", kFmtErr);
                    ++s;
                    for (int i = 0; i < 64; ++i) qt[tq][kZigzag[i]] = pq ? (uint16_t)be16(s + 2 * i) : s[i];
                    s += pq ? 128 : 64;
                }
            } else if (m == 0xC4) {  // DHT
                while (s < se) {
                    const int tc = s[0] >> 4, th = s[0] & 15;
                    if (th > 3 || tc > 1 || s + 17 > se) return fail(IK_ERR_TRANSFORM, "%s: bad DHT", kFmtErr);
                    int total = 0;
                    for (int i = 0; i < 16; ++i) total += s[1 + i];
                    if (total > 256 || s + 17 + total > se) return fail(IK_ERR_TRANSFORM, "%s: bad DHT", kFmtErr);
                    if (!build_huff(s + 1, s + 17, total, tc ? ac[th] : dc[th]))
                        return fail(IK_ERR_TRANSFORM, "%s: bad Huffman table", kFmtErr);
                    s += 17 + total;
                }
            } else if (m == 0xDD) {  // DRI
                if (len < 4) return fail(IK_ERR_TRANSFORM, "%s: bad DRI", kFmtErr);
                restart = be16(s);
            } else if (m == 0xEE) {  // APP14 Adobe
                if (len >= 14 && !std::memcmp(s, "Adobe", 5)) { adobe = true; adobe_transform = s[11]; }
            } else if (m == 0xC0 || m == 0xC1 || m == 0xC2) {  // SOF0 / SOF1 / SOF2
                if (len < 8) return fail(IK_ERR_TRANSFORM, "%s: bad SOF", kFmtErr);
                const int st = frame(s, m);
                if (st) return st;
            } else if (m >= 0xC3 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC) {
                return fail(IK_ERR_UNSUPPORTED, "arithmetic / lossless / hierarchical JPEG (SOF%d) is not supported",
                            m - 0xC0);
            } else if (m == 0xDA) {  // SOS: entropy-coded data follows the header
                const uint8_t* next = se;
                const int st = scan(s, se, next);
                if (st) return st;
                if (need_host) return IK_OK;
                p = next;
                continue;
            }
            p += len;
        }
    }
};

}  // namespace

std::atomic<int> g_jpeg_recon{-1};  // -1: not yet read from IK_JPEG_RECON

namespace {

int jpeg_recon() {
    int m = g_jpeg_recon.load();
    if (m < 0) {
        const char* e = getenv("IK_JPEG_RECON");
        m = e && !strcmp(e, "libjpeg") ? IK_JPEG_RECON_LIBJPEG : IK_JPEG_RECON_ZUNE;
        int expected = -1;
        g_jpeg_recon.compare_exchange_strong(expected, m);
        m = g_jpeg_recon.load();
    }
    return m;
}

// reconstruction geometry of a parsed stream; returns the plane bytes it needs
size_t make_geom(const Decoder& d, JpegGeom& g) {
    const int nc = (int)d.comps.size();
    int colorspace = nc == 1 ? 0 : 1;  // gray / YCbCr
    if (nc == 3 && d.adobe && d.adobe_transform == 0) colorspace = 2;  // Adobe RGB-coded
    if (nc == 3 && !d.adobe && d.comps[0].id == 'R' && d.comps[1].id == 'G' && d.comps[2].id == 'B') colorspace = 2;
    if (nc == 4) colorspace = d.adobe && d.adobe_transform == 2 ? 4 : 3;  // YCCK / CMYK
    g = JpegGeom{};
    g.adobe = d.adobe ? 1 : 0;
    g.recon = jpeg_recon();
    g.ncomp = nc;
    g.W = d.width;
    g.H = d.height;
    g.hmax = d.hmax;
    g.vmax = d.vmax;
    g.colorspace = colorspace;
    size_t plane_bytes = 0;
    for (int i = 0; i < nc; ++i) {
        const Component& c = d.comps[i];
        g.h[i] = c.h; g.v[i] = c.v; g.bw[i] = c.bw; g.bh[i] = c.bh; g.dw[i] = c.dw; g.dh[i] = c.dh;
        g.blk0[i] = (long long)c.blk0;
        g.plane0[i] = (long long)plane_bytes;
        plane_bytes += (size_t)c.bw * 8 * c.bh * 8;
    }
    g.nblocks = (long long)d.nblocks;
    return plane_bytes;
}

void qtables(const Decoder& d, uint16_t q[256]) {
    std::memset(q, 0, 256 * sizeof(uint16_t));
    for (int i = 0; i < (int)d.comps.size(); ++i) std::memcpy(&q[i * 64], d.qt[d.comps[i].tq], 64 * sizeof(uint16_t));
}

using jsync::up256;

// process-wide: JPEG streams whose entropy decoding ran on the GPU / on the host
std::atomic<unsigned long long> g_jpeg_gpu_streams{0}, g_jpeg_host_streams{0};
// process-wide: JPEG files of device-resident batches taken in place / copied back
// before parsing / taken in place and copied back later (ik_jpeg_device_counters)
std::atomic<unsigned long long> g_jpeg_dev[3] = {{0}, {0}, {0}};
std::atomic<int> g_jpeg_device{-1};  // ik_set_jpeg_device; -1: IK_JPEG_DEVICE, read per batch
// ik_jpeg_prog_free_ms: the last batch with restart-free progressive files -- device ms of
// the self-synchronising launches, the DC refinement launches, the AC refinement chains
std::atomic<float> g_prog_free_ms[3] = {{0.f}, {0.f}, {0.f}};

}  // namespace

void jpeg_device_count(int which, unsigned long long n) { g_jpeg_dev[which] += n; }
static std::atomic<float> g_jpeg_walk_ms{0.f};
void jpeg_device_walk_ms(float ms) { g_jpeg_walk_ms.store(ms); }

bool jpeg_device_inplace() {
    const int m = g_jpeg_device.load();
    if (m >= 0) return m == IK_JPEG_DEVICE_INPLACE;
    const char* e = getenv("IK_JPEG_DEVICE");
    return !(e && !strcmp(e, "copy"));
}

// ---- the upload stage's JPEG areas (JpegUpload) ------------------------------------
struct JpegArea {
    int device = 0;
    uint8_t* dev = nullptr;
    size_t cap = 0;
    uint8_t* pin = nullptr;  // staging for files the caller did not pin
    size_t pin_cap = 0;
    hipEvent_t ev = nullptr;
    bool busy = false;
};

namespace {
constexpr int kJpegAreas = 2;
struct JpegAreaPool {
    std::mutex mu;
    std::condition_variable cv;
    std::vector<JpegArea*> areas;
};
std::mutex g_jarea_mu;
std::map<int, JpegAreaPool*> g_jarea_pools;
JpegAreaPool& jarea_pool(int device) {
    std::lock_guard<std::mutex> lk(g_jarea_mu);
    JpegAreaPool*& p = g_jarea_pools[device];
    if (!p) p = new JpegAreaPool();
    return *p;
}
// an idle area of the device (waits while the batches ahead hold both), as a
// shared_ptr whose deleter hands it back
std::shared_ptr<JpegArea> jarea_acquire(int device) {
    JpegAreaPool& P = jarea_pool(device);
    std::unique_lock<std::mutex> lk(P.mu);
    JpegArea* got = nullptr;
    while (!got) {
        for (JpegArea* a : P.areas)
            if (!a->busy) { got = a; break; }
        if (!got && (int)P.areas.size() < kJpegAreas) {
            got = new JpegArea();
            got->device = device;
            if (hipEventCreateWithFlags(&got->ev, hipEventDisableTiming) != hipSuccess) got->ev = nullptr;
            P.areas.push_back(got);
        }
        if (!got) P.cv.wait(lk);
    }
    got->busy = true;
    return std::shared_ptr<JpegArea>(got, [](JpegArea* a) {
        JpegAreaPool& Q = jarea_pool(a->device);
        {
            std::lock_guard<std::mutex> l2(Q.mu);
            a->busy = false;
        }
        Q.cv.notify_all();
    });
}
}  // namespace

int jpeg_upload_begin(const uint8_t* const* bytes, const size_t* lens, int n, JpegUpload& up) {
    up = JpegUpload();
    if (n <= 0) return IK_OK;
    std::vector<size_t> off(n), soff(n, (size_t)-1);
    size_t total = 0, stotal = 0;
    for (int i = 0; i < n; ++i) {
        off[i] = total;
        total += up256(lens[i] + 64);
        if (!host_pinned(bytes[i], lens[i])) { soff[i] = stotal; stotal += up256(lens[i]); }
    }
    std::shared_ptr<JpegArea> A = jarea_acquire(current_device());
    if (!A->ev) return IK_OK;  // (no event: the kernel stage copies the scans itself)
    // grow an idle area (nothing pending reads it: it was handed back after its batch's decode)
    if (total > A->cap) {
        if (A->dev) { (void)hipFree(A->dev); mem_stat(kMemUploadDev, -(int64_t)A->cap); }
        A->dev = nullptr;
        A->cap = 0;
        if (hipMalloc((void**)&A->dev, total + total / 8) != hipSuccess) { A->dev = nullptr; return IK_OK; }
        A->cap = total + total / 8;
        mem_stat(kMemUploadDev, (int64_t)A->cap);
    }
    if (stotal > A->pin_cap) {
        if (A->pin) { (void)hipHostFree(A->pin); mem_stat(kMemUploadPinned, -(int64_t)A->pin_cap); }
        A->pin = nullptr;
        A->pin_cap = 0;
        if (hipHostMalloc((void**)&A->pin, stotal + stotal / 8, hipHostMallocDefault) != hipSuccess) {
            A->pin = nullptr;
            return IK_OK;
        }
        A->pin_cap = stotal + stotal / 8;
        mem_stat(kMemUploadPinned, (int64_t)A->pin_cap);
    }
    if (stotal)
        parallel_for(n, 0, [&](int i) {
            if (soff[i] != (size_t)-1) std::memcpy(A->pin + soff[i], bytes[i], lens[i]);
        });
    hipStream_t s = thread_stream();
    hipError_t e = hipSuccess;
    for (int i = 0; i < n && e == hipSuccess; ++i)
        e = hipMemcpyAsync(A->dev + off[i], soff[i] == (size_t)-1 ? bytes[i] : A->pin + soff[i], lens[i],
                           hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipEventRecord(A->ev, s);
    static const bool timing = getenv("IK_TIMING") != nullptr;
    if (timing)
        fprintf(stderr, "[jpeg-upload] %d files, %.1f MB (%.1f MB staged) queued at t=%.1f ms\n", n, total / 1e6, stotal / 1e6,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count() -
                    1e3 * (double)(long long)(std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count() / 1000) * 1000);
    if (e != hipSuccess) {  // the kernel stage copies the scans itself
        (void)hipStreamSynchronize(s);
        return IK_OK;
    }
    for (int i = 0; i < n; ++i) up.dev[bytes[i]] = A->dev + off[i];
    up.n = n;
    up.ev = A->ev;
    up.area = std::move(A);
    return IK_OK;
}

// ik_shutdown: the JPEG upload areas (no batch is in flight)
void jpeg_shutdown() {
    std::vector<JpegAreaPool*> ps;
    {
        std::lock_guard<std::mutex> lk(g_jarea_mu);
        for (auto& kv : g_jarea_pools) ps.push_back(kv.second);
    }
    for (JpegAreaPool* P : ps) {
        std::lock_guard<std::mutex> lk(P->mu);
        for (JpegArea* a : P->areas) {
            (void)hipSetDevice(a->device);
            if (a->dev) { (void)hipFree(a->dev); mem_stat(kMemUploadDev, -(int64_t)a->cap); }
            if (a->pin) { (void)hipHostFree(a->pin); mem_stat(kMemUploadPinned, -(int64_t)a->pin_cap); }
            if (a->ev) (void)hipEventDestroy(a->ev);
            delete a;
        }
        P->areas.clear();
    }
}

namespace {

#ifdef IK_JPEG_DUMP
std::mutex g_jdump_mu;
std::vector<std::array<std::vector<uint8_t>, 7>> g_jdump;  // per image of the last batch
#endif

// The baseline scans of a batch (ds[idx[k]]->js), all through the self-synchronising
// GPU decoder at once (ik_jsync.hip; algorithm ik_jpeg_sync.h):
//   1. layout: every scan's and image's share of one scratch block, one pinned block
//   2. upload: every scan's bytes (DMAed in place when page-locked, else staged),
//      Huffman and quantisation tables, the unstuffing chunk table -- one small copy
//   3. unstuffing on the GPU, then the interval tables come back (a few KB)
//   4. lanes: per image, each interval cut into pieces of lane_bits (host); the
//      refinement scans of the progressive images put into launches and chains
//   5. the sync pass, the fix rounds (one over all lanes, then the settle kernel's
//      per image until no lane changes), bases, the decode pass, the refinement
//      scans -- no host round trip
//   6. counters
//   7. reconstruction of every image (IDCT, upsampling, colour)
// An image the GPU finds inconsistent (a stray marker, a restart count that does
// not match the frame, lanes that never synchronise, a bad code) goes to host_idx:
// the host decoder decides and reports the reference's errors.
// The host's decisions -- scratch layout, lane rules, refinement schedule -- are
// ik_jsync_plan.h's; the steps below add the device pointers, copy and launch.
struct JsyncBatch {
    std::vector<std::unique_ptr<Decoder>>& ds;
    const std::vector<int>& idx;
    ik_image** outs;
    std::vector<int>& st;
    std::vector<int>& host_idx;
    const uint8_t* const* files;
    const JpegUpload* up;
    const int m = (int)idx.size();
    JsyncBatch(std::vector<std::unique_ptr<Decoder>>& ds_, const std::vector<int>& idx_, ik_image** outs_, std::vector<int>& st_,
               std::vector<int>& host_idx_, const uint8_t* const* files_, const JpegUpload* up_)
        : ds(ds_), idx(idx_), outs(outs_), st(st_), host_idx(host_idx_), files(files_), up(up_) {}
    // An item is one scan of one image: a baseline image has one, a progressive file
    // without restart markers (Decoder::pf) one per scan, in file order.
    struct Item {
        int k;                        // the image (index into idx)
        const Decoder::FreeScan* fs;  // null: the baseline scan
        const uint8_t* data;
        const uint8_t* on_dev;        // the scan where it already lies on the device, or null
    };
    std::vector<Item> items;
    std::vector<jsync::ScanIn> sin;
    std::vector<JpegGeom> geom;
    jsync::BatchLayout B;
    int ni = 0;
    hipStream_t s = nullptr;
    uint8_t *dev = nullptr, *hp = nullptr, *hp_dev = nullptr;
    hipError_t e = hipSuccess;
    std::vector<int> ok, hstatus, ivl_lane;
    std::vector<int2> wgs;
    std::vector<jsync::Scan> scans;
    jsync::RefinePlan R;
    long long lanes_used = 0;
    int rounds = 0;  // the settle kernel's most rounds over the batch's scans
    EvPair *ev = nullptr, *ev2 = nullptr;
    const std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    double tm_layout = 0, tm_sync = 0, tm_tables = 0, tm_upwait = -1, t_unstuff = 0;
    const bool timing = [] { static const bool on = getenv("IK_TIMING") != nullptr; return on; }();

    double ms() const { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
    const Decoder& dec(int k) const { return *ds[idx[k]]; }
    template <class T> T* at(const jsync::Region& r) const { return reinterpret_cast<T*>(dev + r.off); }
    void to_host(bool only_ok) {
        for (int k = 0; k < m; ++k)
            if (!only_ok || ok[k]) host_idx.push_back(idx[k]);
    }
    // Small transfers between hp and the device go through a copy kernel on this
    // stream that reads or writes the pinned block directly (ik_png_decode.cpp Xfer):
    // SDMA copies queue behind the next batch's scan upload on the same engine --
    // ~12 ms per transfer with configs[2]'s 683 MB batches in flight.
    hipError_t h2d(uint8_t* d, size_t off, size_t n) {  // hp[off, off + n) -> d
        if (!n) return hipSuccess;
        if (!hp_dev) return hipMemcpyAsync(d, hp + off, n, hipMemcpyHostToDevice, s);
        return launch_copy_words(reinterpret_cast<const uint32_t*>(hp_dev + off), reinterpret_cast<uint32_t*>(d), (n + 3) / 4, s);
    }
    hipError_t d2h(size_t off, const uint8_t* d, size_t n) {  // d -> hp[off, off + n)
        if (!n) return hipSuccess;
        if (!hp_dev) return hipMemcpyAsync(hp + off, d, n, hipMemcpyDeviceToHost, s);
        return launch_copy_words(reinterpret_cast<const uint32_t*>(d), reinterpret_cast<uint32_t*>(hp_dev + off), (n + 3) / 4, s);
    }

    // 1. the items, their layout, the scratch and the pinned block
    bool layout() {
        std::vector<jsync::ImageIn> imgs(m);
        geom.resize(m);
        for (int k = 0; k < m; ++k) {
            const int i = idx[k];
            const Decoder& d = *ds[i];
            auto add = [&](const Decoder::FreeScan* fs, const uint8_t* data, size_t len, long long nivl, const jsync::Scan& g, int comp) {
                // a scan the upload stage already put on the device (JpegUpload) is read
                // where it lies, and so is a file of a device-resident batch: the caller's
                // memory (no byte past the scan is the decoder's to read: the unstuffing
                // kernels' scan_byte stops at scan_len)
                const uint8_t* on_dev = nullptr;
                if (d.skel) on_dev = files[i] + d.skel->ent_off;
                else if (up && up->n) {
                    auto it = up->dev.find(files[i]);
                    if (it != up->dev.end()) on_dev = it->second + (data - files[i]);
                }
                items.push_back(Item{k, fs, data, on_dev});
                sin.push_back(jsync::ScanIn{len, nivl, g.kind, k, comp, on_dev != nullptr, g.total_blocks});
            };
            if (d.pf)
                for (const auto& fs : d.pf_scans) add(&fs, fs.data, fs.len, 1, fs.geom, fs.comp);
            else add(nullptr, d.js_data, d.js_len, d.js_nivl, d.js_scan, 0);
            imgs[k].nblocks = d.nblocks;
            imgs[k].plane_bytes = make_geom(d, geom[k]);
        }
        ni = (int)items.size();
        B = jsync::plan_layout(sin.data(), ni, imgs.data(), m, jsync::DevSizes{sizeof(JsImageDev), sizeof(JpegReconItem), jsync_chunk_scratch_bytes});
        s = thread_stream();
        dev = scratch_slot(1, B.total);
        hp = dev ? pinned_slot(1, B.pin_bytes) : nullptr;
        if (!dev || !hp) { to_host(false); return false; }
        tm_layout = ms();
        (void)hipStreamSynchronize(s);  // the pinned block is free
        if (hipHostGetDevicePointer((void**)&hp_dev, hp, 0) != hipSuccess) hp_dev = nullptr;
        tm_sync = ms();
        return true;
    }

    // 2. one small upload (scan records, chunk table, Huffman and quantisation tables),
    // the scan bytes, and the zeroing; false: no staging memory
    bool upload() {
        JsImageDev* I = reinterpret_cast<JsImageDev*>(hp + B.img.off);
        int2* ch = reinterpret_cast<int2*>(hp + B.chunks.off);
        for (int t = 0; t < ni; ++t) {
            const jsync::ScanLay& L = B.scans[t];
            JsImageDev& J = I[t];
            J = JsImageDev{};
            J.scan = items[t].on_dev ? items[t].on_dev : dev + L.scan.off;
            J.scan_len = (long long)sin[t].len;
            J.out = dev + L.out.off;
            J.ivl = at<long long>(B.ivl) + L.ivl0;
            J.ivl_cap = (int)sin[t].nivl + 1;
            J.chunk0 = L.chunk0;
            J.nchunks = L.nchunks;
            J.totals = at<uint32_t>(B.totals) + 2 * t;
            J.status = at<int>(B.status) + t;
            for (int c = 0; c < L.nchunks; ++c) ch[L.chunk0 + c] = make_int2(t, c);
        }
        parallel_for(ni, 0, [&](int t) {
            JpegHuffTables* T = reinterpret_cast<JpegHuffTables*>(hp + B.scans[t].tab.off);
            if (items[t].fs) std::memcpy(T, &items[t].fs->tabs, sizeof(JpegHuffTables));  // as they stood at the scan's SOS
            else dec(items[t].k).tables(*T);
        });
        parallel_for(m, 0, [&](int k) { qtables(dec(k), reinterpret_cast<uint16_t*>(hp + B.images[k].qt.off)); });
        // the scan bytes: where the upload stage put them (JpegUpload), else DMAed in
        // place from page-locked memory, else through pinned staging
        std::vector<char> in_place(ni, 0);
        std::vector<size_t> st_off(ni, 0);
        size_t st_total = 0;
        for (int t = 0; t < ni; ++t) {
            if (items[t].on_dev) continue;
            in_place[t] = host_pinned(items[t].data, sin[t].len) ? 1 : 0;
            if (!in_place[t]) { st_off[t] = st_total; st_total += up256(sin[t].len); }
        }
        uint8_t* hdata = st_total ? pinned_slot(2, st_total) : nullptr;
        if (st_total && !hdata) { to_host(false); return false; }
        if (st_total)
            parallel_for(ni, 0, [&](int t) {
                if (!in_place[t] && !items[t].on_dev) std::memcpy(hdata + st_off[t], items[t].data, sin[t].len);
            });
        tm_tables = ms();
        const bool wait_up = up && up->n && up->ev;
        if (timing && wait_up) {  // (IK_TIMING: how long the upload stage's DMA still had to run)
            const double tw = ms();
            if (hipEventQuery(up->ev) != hipSuccess) (void)hipEventSynchronize(up->ev);
            tm_upwait = ms() - tw;
        }
        e = h2d(dev, 0, B.upload1.bytes);
        for (int t = 0; t < ni && e == hipSuccess; ++t) {
            if (items[t].on_dev || !sin[t].len) continue;
            e = hipMemcpyAsync(dev + B.scans[t].scan.off, in_place[t] ? items[t].data : hdata + st_off[t], sin[t].len,
                               hipMemcpyHostToDevice, s);
        }
        if (e == hipSuccess && wait_up) e = hipStreamWaitEvent(s, up->ev, 0);
        if (e == hipSuccess) e = hipMemsetAsync(dev + B.readback.off, 0, B.readback.bytes, s);
        // a progressive image's scans each store only what they code: its coefficients start at zero
        for (int k = 0; k < m && e == hipSuccess; ++k)
            if (dec(k).pf) e = hipMemsetAsync(dev + B.images[k].coef.off, 0, B.images[k].coef.bytes, s);
        return true;
    }

    // 3. unstuffing; status, totals and the interval tables back; false: the device failed
    bool unstuff() {
        if (e == hipSuccess)
            e = launch_jsync_unstuff(at<JsImageDev>(B.img), ni, at<const int2>(B.chunks), B.nchunks, at<uint2>(B.counts), s);
        if (e == hipSuccess) e = d2h(0, dev + B.readback.off, B.readback.bytes);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) { (void)hip_fail(e, "jpeg unstuff"); to_host(false); return false; }
        t_unstuff = ms();
        return true;
    }

    // 4. per image, each interval cut into lanes; the images that drop out go to the
    // host; the refinement schedule; all of it into the pinned block.  False: no lanes
    bool lanes() {
        ok.assign(m, 0);
        hstatus.assign(m, 0);
        ivl_lane.assign((size_t)B.nivl_total, 0);
        scans.resize(ni);
        const int* hst = reinterpret_cast<const int*>(hp + B.in_readback(B.status));
        const uint32_t* tot = reinterpret_cast<const uint32_t*>(hp + B.in_readback(B.totals));
        const long long* hivl = reinterpret_cast<const long long*>(hp + B.in_readback(B.ivl));
        for (int k = 0; k < m; ++k) {
            const jsync::ImageLay& IL = B.images[k];
            // An image that drops out here still has Scans the per-scan kernels
            // (k_jsync_settle, k_jsync_seg2: a workgroup / a thread per scan of the
            // batch) load: ones with no lanes -- their tables, and an interval table whose
            // first entry, the lane count of zero intervals, is 0.  (Left zeroed, its
            // null table pointers were read on the device whenever such an image
            // shared a batch with one that decodes.)
            bool good = true;
            for (int t = IL.item0; t < IL.item0 + IL.nitems; ++t) {
                const jsync::ScanLay& L = B.scans[t];
                scans[t] = items[t].fs ? items[t].fs->geom : dec(k).js_scan;
                scans[t].nivl = 0;
                scans[t].lane0 = L.lane0;
                scans[t].ivl_lane = at<const int>(B.ivl_lane) + L.ivl0;
                scans[t].tabs = reinterpret_cast<const JpegHuffTables*>(dev + L.tab.off);
                if (hst[t] || (long long)tot[2 * t + 1] + 1 != sin[t].nivl) { good = false; continue; }  // stray marker / wrong restart count
                if (!jsync::has_lanes(sin[t].kind)) continue;  // (a refinement scan: no lanes, ivl_lane stays 0, 0)
                if (!jsync::split_lanes(hivl + L.ivl0, sin[t].nivl, B.lane_bits, L.lanes_max, ivl_lane.data() + L.ivl0)) good = false;
            }
            if (!good) {
                for (int t = IL.item0; t < IL.item0 + IL.nitems; ++t)
                    for (long long q = 0; q <= sin[t].nivl; ++q) ivl_lane[B.scans[t].ivl0 + q] = 0;
                continue;
            }
            ok[k] = 1;
            for (int t = IL.item0; t < IL.item0 + IL.nitems; ++t) {
                const jsync::ScanLay& L = B.scans[t];
                const int nl = ivl_lane[L.ivl0 + sin[t].nivl];
                lanes_used += nl;
                for (int w = 0; w < nl; w += 256) wgs.push_back(make_int2(t, w));
                jsync::Scan& S = scans[t];
                S.L = B.lane_bits;
                S.words = reinterpret_cast<const uint32_t*>(dev + L.out.off);
                S.ivl = at<const long long>(B.ivl) + L.ivl0;
                S.nivl = (int)sin[t].nivl;
                S.coef = at<int16_t>(IL.coef);
            }
        }
        for (int k = 0; k < m; ++k)
            if (!ok[k]) host_idx.push_back(idx[k]);
        if (wgs.empty()) return false;
        R = jsync::plan_refinement(sin.data(), ni, ok.data());
        static_assert(sizeof(jsync::Chain) == sizeof(int2), "k_jprog_ac_chain reads the chains as int2");
        auto put = [&](const jsync::Region& r, const void* src, size_t bytes) {
            if (bytes) std::memcpy(hp + B.in_upload2(r), src, bytes);
        };
        put(B.scan_tab, scans.data(), sizeof(jsync::Scan) * ni);
        put(B.ivl_lane, ivl_lane.data(), sizeof(int) * B.nivl_total);
        put(B.wgs, wgs.data(), sizeof(int2) * wgs.size());
        put(B.rlist, R.rlist.data(), sizeof(int) * R.rlist.size());
        put(B.chains, R.chains.data(), sizeof(jsync::Chain) * R.chains.size());
        return true;
    }

    // 5. sync, fix rounds, bases, decode; then the refinement scans; status and the
    // settle kernel's rounds back.  False: the device failed
    bool launch() {
        const jsync::Scan* d_scans = at<const jsync::Scan>(B.scan_tab);
        const int2* d_wgs = at<const int2>(B.wgs);
        const int nwg = (int)wgs.size();
        jsync::LaneRec* d_recs = at<jsync::LaneRec>(B.recs);
        int* d_status = at<int>(B.status);
        int* d_changed = at<int>(B.changed);
        const int* d_rlist = at<const int>(B.rlist);
        ev = &thread_events(2);
        ev2 = &thread_events(3);
        e = h2d(dev + B.upload2.off, 0, B.upload2.bytes);
        if (e == hipSuccess) ev_record(ev->a, s);
        if (e == hipSuccess) e = launch_jsync_sync(d_scans, d_wgs, nwg, d_recs, s);
        if (e == hipSuccess) e = hipMemsetAsync(d_changed, 0, sizeof(int), s);
        if (e == hipSuccess) e = launch_jsync_fix(d_scans, ni, d_wgs, nwg, d_recs, d_changed, s);
        if (e == hipSuccess)
            e = launch_jsync_bases_decode(d_scans, ni, d_wgs, nwg, d_recs, at<jsync::LaneBase>(B.bases), dev + B.cs.off, d_status, s);
        if (e == hipSuccess) ev_record(ev->b, s);
        const bool refine = !R.rlist.empty();
        if (refine) {
            int at_scan = 0;
            for (size_t r = 0; r < R.dc_sizes.size() && e == hipSuccess; ++r) {
                e = launch_jprog_dc_refine(d_scans, d_rlist + at_scan, R.dc_sizes[r], R.dc_blocks[r], s);
                at_scan += R.dc_sizes[r];
            }
            if (e == hipSuccess) ev_record(ev2->a, s);
            if (e == hipSuccess)
                e = launch_jprog_ac_chain(d_scans, at<const int2>(B.chains), (int)R.chains.size(), d_rlist, d_status, s);
            if (e == hipSuccess) ev_record(ev2->b, s);
        }
        if (e == hipSuccess) e = d2h(0, reinterpret_cast<const uint8_t*>(d_status), sizeof(int) * ni);
        if (e == hipSuccess) e = d2h(B.pin_changed, reinterpret_cast<const uint8_t*>(d_changed), sizeof(int));
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) {
            (void)hip_fail(e, "jpeg entropy decode");
            to_host(true);
            return false;
        }
        const int* hs = reinterpret_cast<const int*>(hp);
        for (int t = 0; t < ni; ++t) hstatus[items[t].k] |= hs[t];  // any scan's flag sends the image to the host
        std::memcpy(&rounds, hp + B.pin_changed, sizeof(int));
        if (refine) {  // ik_jpeg_prog_free_ms: the last batch's phase A, DC refinement and chain launches
            float dc_ms = 0.f;
            if (!ev->b || !ev2->a || hipEventElapsedTime(&dc_ms, ev->b, ev2->a) != hipSuccess) dc_ms = 0.f;
            g_prog_free_ms[0].store(ev_pair_ms(*ev));
            g_prog_free_ms[1].store(dc_ms);
            g_prog_free_ms[2].store(ev_pair_ms(*ev2));
        }
        return true;
    }

#ifdef IK_JPEG_DUMP  // dev experiment: every image's unstuffed words, lane tables and coefficients (its first scan's)
    void dump() {
        std::lock_guard<std::mutex> lk(g_jdump_mu);
        g_jdump.assign(m, {});
        for (int k = 0; k < m; ++k) {
            if (!ok[k]) continue;
            const int t = B.images[k].item0;
            const jsync::ScanLay& L = B.scans[t];
            const long long nivl = sin[t].nivl;
            const int nl = ivl_lane[L.ivl0 + nivl];
            auto get = [&](int what, const void* src, size_t bytes) {
                g_jdump[k][what].resize(bytes);
                (void)hipMemcpy(g_jdump[k][what].data(), src, bytes, hipMemcpyDeviceToHost);
            };
            get(0, dev + L.out.off, sin[t].len);
            get(1, at<long long>(B.ivl) + L.ivl0, sizeof(long long) * (nivl + 1));
            get(2, at<jsync::LaneRec>(B.recs) + L.lane0, sizeof(jsync::LaneRec) * nl);
            get(3, at<jsync::LaneBase>(B.bases) + L.lane0, sizeof(jsync::LaneBase) * nl);
            get(4, dev + B.images[k].coef.off, B.images[k].coef.bytes);
            g_jdump[k][5].resize(sizeof(int) * (nivl + 1));
            std::memcpy(g_jdump[k][5].data(), ivl_lane.data() + L.ivl0, sizeof(int) * (nivl + 1));
            g_jdump[k][6].resize(sizeof(int) * 2);
            std::memcpy(g_jdump[k][6].data(), &hstatus[k], sizeof(int));
            std::memcpy(g_jdump[k][6].data() + sizeof(int), &rounds, sizeof(int));
        }
    }
#endif

    // 6. ik_batch_last_timing: the decoding launches' time and algorithmic bytes
    void counters() {
        double scan = 0, coef = 0;
        for (int t = 0; t < ni; ++t)
            if (ok[items[t].k]) scan += (double)sin[t].len;
        for (int k = 0; k < m; ++k)
            if (ok[k]) coef += (double)B.images[k].coef.bytes;
        const int d = current_device();
        const bool refine = !R.rlist.empty();
        batch_timing_add(d, kBtJpegHuffMs, ev_pair_ms(*ev) + (refine ? g_prog_free_ms[1].load() + g_prog_free_ms[2].load() : 0.f));
        batch_timing_add(d, kBtJpegScanBytes, scan);
        batch_timing_add(d, kBtJpegCoefBytes, coef);
        batch_timing_add(d, kBtJpegImages, (double)(lanes_used ? std::count(ok.begin(), ok.end(), 1) : 0));
        batch_timing_add(d, kBtJpegLanes, (double)lanes_used);
    }

    // 7. reconstruction, every image in three launches; then each image is counted,
    // or -- the device failed -- handed to the host decoder
    void reconstruct() {
        JpegReconItem* ritems = reinterpret_cast<JpegReconItem*>(hp);
        int mi = 0, max_w = 0, max_h = 0;
        long long max_blocks = 0;
        bool any_fast = false, any_slow = false;
        for (int k = 0; k < m; ++k) {
            if (!ok[k]) continue;
            const int i = idx[k];
            if (hstatus[k]) { host_idx.push_back(i); continue; }
            const Decoder& d = *ds[i];
            JpegGeom g = geom[k];
            g.qt = at<const uint16_t>(B.images[k].qt);
            g.coef = at<const int16_t>(B.images[k].coef);
            g.planes = dev + B.images[k].pl.off;
            ik_image* img = nullptr;
            st[i] = alloc_image((uint32_t)d.width, (uint32_t)d.height, d.comps.size() == 1 ? 1u : 3u, &img);
            if (st[i]) continue;
            outs[i] = img;
            const bool fast = jpeg_zune_fast(g);
            ritems[mi++] = JpegReconItem{g, img->d, img->pitch, fast ? 1 : 0, 0};
            max_blocks = std::max(max_blocks, g.nblocks);
            max_w = std::max(max_w, g.W);
            max_h = std::max(max_h, g.H);
            any_fast = any_fast || fast;
            any_slow = any_slow || !fast;
        }
        e = h2d(dev + B.items.off, 0, sizeof(JpegReconItem) * mi);
        if (e == hipSuccess)
            e = launch_jpeg_reconstruct_batch(at<const JpegReconItem>(B.items), mi, max_blocks, max_w, max_h, any_fast, any_slow, true, s);
        if (e != hipSuccess) (void)hip_fail(e, "jpeg reconstruct");
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        for (int k = 0; k < m; ++k) {
            const int i = idx[k];
            if (!ok[k] || hstatus[k] || !outs[i]) continue;
            if (e != hipSuccess) {  // the device failed: the host decoder takes them
                ik_image_free(outs[i]);
                outs[i] = nullptr;
                st[i] = IK_OK;
                host_idx.push_back(i);
                continue;
            }
            g_jpeg_gpu_streams += 1;
        }
        if (timing)
            fprintf(stderr, "[jsync] %d images, %d scans, %lld lanes, %d fix rounds: layout %.2f, sync %.2f, tables %.2f, upload wait %.2f, "
                    "unstuff %.2f ms, total %.2f ms\n", m, ni, lanes_used, rounds, tm_layout, tm_sync, tm_tables, tm_upwait, t_unstuff, ms());
    }
};

static void jsync_batch(std::vector<std::unique_ptr<Decoder>>& ds, const std::vector<int>& idx, ik_image** outs,
                        std::vector<int>& st, std::vector<int>& host_idx, const uint8_t* const* files,
                        const JpegUpload* up) {
    if (idx.empty()) return;
    JsyncBatch J(ds, idx, outs, st, host_idx, files, up);
    if (!J.layout()) return;   // no memory: every image to the host decoder
    if (!J.upload()) return;   // (the same)
    if (!J.unstuff()) return;  // the device failed: every image to the host decoder
    if (!J.lanes()) return;    // no image left with lanes (those that dropped out are the host's)
    if (!J.launch()) return;   // the device failed: the images that had lanes to the host decoder
#ifdef IK_JPEG_DUMP
    J.dump();
#endif
    J.counters();
    J.reconstruct();
}

// try_gpu: baseline scans go through the self-synchronising GPU decoder (the batch
// path with one image), progressive scans with restart intervals scan by scan
// (k_jpeg_prog); anything else, and any stream the GPU finds inconsistent, goes
// through the host decoder
int decode_jpeg_impl(const uint8_t* bytes, size_t n, ik_image** out, bool try_gpu) {
    static const bool timing = getenv("IK_TIMING") != nullptr;  // dev: phase times to stderr
    auto now = [] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = timing ? now() : 0;
    Decoder d;
    d.b = bytes;
    d.end = bytes + n;
    d.try_gpu = try_gpu;
    int st = d.parse();
    if (st) return st;
    d.finish();
    if (d.need_host) return decode_jpeg_impl(bytes, n, out, false);  // several scans: all on the host
    if (d.js || d.pf) {
        int status = IK_OK;
        std::string msg;
        st = decode_jpeg_batch(&bytes, &n, 1, out, &status, &msg, nullptr);
        if (st && !msg.empty()) return fail(st, "%s", msg.c_str());
        return st;
    }
    const int nc = (int)d.comps.size();
    JpegGeom g;
    const size_t plane_bytes = make_geom(d, g);

    // device scratch: [qtables 4x64 u16][coefficients][planes][progressive scans]
    const size_t qbytes = 256 * sizeof(uint16_t);
    const size_t cbytes = d.nblocks * 64 * sizeof(int16_t);
    std::vector<uint16_t> q(256, 0);
    qtables(d, q.data());
    const double t1 = timing ? now() : 0;
    ik_image* img = nullptr;
    st = alloc_image((uint32_t)d.width, (uint32_t)d.height, nc == 1 ? 1u : 3u, &img);
    if (st) return st;
    const double t2 = timing ? now() : 0;
    const size_t pl_off = qbytes + (cbytes + 255) / 256 * 256;
    const size_t q_off = pl_off + (plane_bytes + 255) / 256 * 256;
    // progressive scans on the GPU: [the file (+ reader slack)][error flag][per scan:
    // tables, interval starts], staged in one host buffer and copied at once
    const bool prog = !d.prog.empty();
    std::vector<uint8_t> pstage;
    std::vector<size_t> ptab_off, pseg_off;
    size_t p_err = 0;
    if (prog) {
        size_t o = up256(n + 1024);
        p_err = o;
        o += 256;
        for (const auto& ps : d.prog) {
            ptab_off.push_back(o);
            o += up256(sizeof(JpegHuffTables));
            pseg_off.push_back(o);
            o += up256(ps.segs.size() * sizeof(unsigned));
        }
        pstage.assign(o, 0);
        std::memcpy(pstage.data(), bytes, n);
        for (size_t k = 0; k < d.prog.size(); ++k) {
            std::memcpy(pstage.data() + ptab_off[k], &d.prog[k].tabs, sizeof(JpegHuffTables));
            std::memcpy(pstage.data() + pseg_off[k], d.prog[k].segs.data(), d.prog[k].segs.size() * sizeof(unsigned));
        }
    }
    uint8_t* dev = scratch(q_off + pstage.size());
    if (!dev) { ik_image_free(img); return fail(IK_ERR_DEVICE, "cannot allocate device scratch"); }
    hipStream_t s = thread_stream();
    st = copy_h2d_2d(dev, qbytes, reinterpret_cast<const uint8_t*>(q.data()), qbytes, qbytes, 1, s);
    if (!st && prog) {
        uint8_t* pb = dev + q_off;
        st = copy_h2d_2d(pb, pstage.size(), pstage.data(), pstage.size(), pstage.size(), 1, s);
        if (!st) {
            hipError_t e = hipMemsetAsync(dev + qbytes, 0, cbytes, s);
            int* d_err = reinterpret_cast<int*>(pb + p_err);
            for (size_t k = 0; k < d.prog.size() && e == hipSuccess; ++k) {
                JpegScanArgs a = d.prog[k].a;
                a.data = pb + (size_t)(uintptr_t)a.data;  // the scan's offset in the file
                a.seg = reinterpret_cast<const unsigned*>(pb + pseg_off[k]);
                a.tabs = reinterpret_cast<const JpegHuffTables*>(pb + ptab_off[k]);
                a.coef = reinterpret_cast<int16_t*>(dev + qbytes);
                a.err = d_err;
                e = launch_jpeg_prog(a, s);
            }
            int err = 0;
            if (e == hipSuccess) e = hipMemcpyAsync(&err, d_err, sizeof(int), hipMemcpyDeviceToHost, s);
            if (e == hipSuccess) e = hipStreamSynchronize(s);
            if (e != hipSuccess) { ik_image_free(img); return hip_fail(e, "jpeg progressive entropy decode"); }
            if (err) {  // a bad code somewhere: the host decoder reports it
                ik_image_free(img);
                return decode_jpeg_impl(bytes, n, out, false);
            }
        }
    } else if (!st && cbytes) {
        st = copy_h2d_2d(dev + qbytes, cbytes, reinterpret_cast<const uint8_t*>(d.coef.data()), cbytes, cbytes, 1, s);
    }
    if (st) { ik_image_free(img); return st; }
    const double t3 = timing ? now() : 0;
    g.qt = reinterpret_cast<const uint16_t*>(dev);
    g.coef = reinterpret_cast<const int16_t*>(dev + qbytes);
    g.planes = dev + pl_off;
    hipError_t e = launch_jpeg_reconstruct(g, img->d, img->pitch, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) { ik_image_free(img); return hip_fail(e, "jpeg reconstruct"); }
    if (timing)
        fprintf(stderr, "[jpeg] %s: parse %.2f alloc %.2f entropy/upload %.2f reconstruct %.2f ms\n",
                prog ? "gpu entropy" : "host entropy", t1 - t0, t2 - t1, t3 - t2, now() - t3);
    (prog ? g_jpeg_gpu_streams : g_jpeg_host_streams) += 1;
    *out = img;
    return IK_OK;
}

}  // namespace

int decode_jpeg_batch(const uint8_t* const* bytes, const size_t* lens, int n, ik_image** outs, int* status,
                      std::string* msgs, const JpegUpload* up) {
    // 1. parse every stream (host threads); baseline scans are deferred to the GPU
    std::vector<std::unique_ptr<Decoder>> ds(n);
    std::vector<int> st(n, IK_OK);
    auto note = [&](int i) {
        if (st[i] && msgs) {
            char buf[512];
            ik_last_error(buf, sizeof(buf));
            msgs[i] = buf;
        }
    };
    static const bool timing = getenv("IK_TIMING") != nullptr;
    const auto tp0 = std::chrono::steady_clock::now();
    // files decoded where they lie in device memory (bytes[i] is a device address):
    // the parser reads the skeleton the marker walk brought back
    std::vector<const JpegInPlace*> inpl(n, nullptr);
    if (up && up->inplace)
        for (int i = 0; i < n; ++i) {
            auto it = up->inplace->find(bytes[i]);
            if (it != up->inplace->end()) inpl[i] = &it->second;
        }
    parallel_for(n, 0, [&](int i) {
        ds[i].reset(new Decoder());
        Decoder& d = *ds[i];
        d.b = inpl[i] ? inpl[i]->skel : bytes[i];
        d.end = inpl[i] ? inpl[i]->skel + inpl[i]->skel_len : bytes[i] + lens[i];
        d.skel = inpl[i];
        d.try_gpu = true;
        st[i] = d.parse();
        if (!st[i]) d.finish();
        if (inpl[i] && (st[i] || !d.js)) {  // not for the GPU after all: the host parser judges the whole file
            st[i] = IK_OK;
            d.need_host = true;
        }
        note(i);
    });
    if (timing)
        fprintf(stderr, "[jpeg-batch] %d streams parsed in %.2f ms\n", n,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp0).count());
    std::vector<int> js_idx, host_idx, prog_idx;
    for (int i = 0; i < n; ++i) {
        outs[i] = nullptr;
        if (st[i]) continue;
        if ((ds[i]->js || ds[i]->pf) && !ds[i]->need_host) js_idx.push_back(i);
        else if (!ds[i]->prog.empty() && !ds[i]->need_host) prog_idx.push_back(i);  // one by one, GPU
        else host_idx.push_back(i);
    }
    // 2. the baseline scans: the self-synchronising GPU decoder over all of them at once
    jsync_batch(ds, js_idx, outs, st, host_idx, bytes, up);
    // 3. everything else: progressive scans with restart intervals on the GPU image by
    // image, the rest (and anything the GPU found inconsistent) with host entropy decoding
    const int nh = (int)host_idx.size();
    host_idx.insert(host_idx.end(), prog_idx.begin(), prog_idx.end());
    // a file taken in place that the host decoder must take: it is copied back now,
    // and only it
    std::vector<std::vector<uint8_t>> back(n);
    for (int k = 0; k < nh; ++k) {
        const int i = host_idx[k];
        if (!inpl[i]) continue;
        back[i].resize(lens[i]);
        const hipError_t e = hipMemcpy(back[i].data(), bytes[i], lens[i], hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            st[i] = hip_fail(e, "jpeg copy back");
            note(i);
            back[i].clear();
        }
        jpeg_device_count(2, 1);
    }
    parallel_for((int)host_idx.size(), 0, [&](int k) {
        const int i = host_idx[k];
        if (inpl[i] && back[i].empty()) return;  // (the copy failed)
        st[i] = decode_jpeg_impl(inpl[i] ? back[i].data() : bytes[i], lens[i], &outs[i], k >= nh);
        note(i);
    });
    int first = IK_OK;
    for (int i = 0; i < n; ++i) {
        if (status) status[i] = st[i];
        if (st[i] && !first) first = st[i];
    }
    return first;
}

int decode_jpeg_device(const uint8_t* bytes, size_t n, ik_image** out) { return decode_jpeg_impl(bytes, n, out, true); }

}  // namespace ik

namespace ik {
int jpeg_recon_mode() { return jpeg_recon(); }
}  // namespace ik

extern "C" {

int ik_set_jpeg_reconstruction(int mode) {
    if (mode != IK_JPEG_RECON_LIBJPEG && mode != IK_JPEG_RECON_ZUNE)
        return ik::fail(IK_ERR_INVALID, "bad JPEG reconstruction mode %d", mode);
    (void)ik::jpeg_recon_mode();
    ik::g_jpeg_recon.store(mode);
    return IK_OK;
}

int ik_get_jpeg_reconstruction(void) { return ik::jpeg_recon_mode(); }

int ik_jpeg_device_counters(unsigned long long* out) {
    if (!out) return ik::fail(IK_ERR_INVALID, "null pointer");
    for (int k = 0; k < 3; ++k) out[k] = ik::g_jpeg_dev[k].load();
    return IK_OK;
}

double ik_jpeg_device_walk_ms(void) { return (double)ik::g_jpeg_walk_ms.load(); }

int ik_set_jpeg_device(int where) {
    if (where < -1 || where > IK_JPEG_DEVICE_INPLACE) return ik::fail(IK_ERR_INVALID, "bad JPEG device mode %d", where);
    ik::g_jpeg_device.store(where);
    return IK_OK;
}

int ik_get_jpeg_device(void) { return ik::jpeg_device_inplace() ? IK_JPEG_DEVICE_INPLACE : IK_JPEG_DEVICE_COPY; }

int ik_set_jpeg_prog_free(int where) {
    if (where < -1 || where > IK_JPEG_PROG_FREE_GPU) return ik::fail(IK_ERR_INVALID, "bad JPEG progressive mode %d", where);
    ik::g_jpeg_prog_free.store(where);
    return IK_OK;
}

int ik_get_jpeg_prog_free(void) { return ik::jpeg_prog_free_gpu() ? IK_JPEG_PROG_FREE_GPU : IK_JPEG_PROG_FREE_HOST; }

int ik_jpeg_prog_free_ms(double* out) {
    if (!out) return ik::fail(IK_ERR_INVALID, "null pointer");
    for (int k = 0; k < 3; ++k) out[k] = (double)ik::g_prog_free_ms[k].load();
    return IK_OK;
}

int ik_jpeg_walk_host(const uint8_t* bytes, size_t len, uint8_t* skeleton, size_t cap, ik_jpeg_walk_info* info) {
    if (!skeleton || !info || (!bytes && len)) return ik::fail(IK_ERR_INVALID, "null pointer");
    if (cap < IK_JPEG_SKELETON_BYTES) return ik::fail(IK_ERR_INVALID, "the skeleton buffer holds %zu bytes, not %d", cap, IK_JPEG_SKELETON_BYTES);
    static_assert(IK_JPEG_SKELETON_BYTES == ik::jwalk::kSlot, "skeleton slot");
    ik::jwalk::Rec r;
    ik::jwalk::HostOps ops;
    ik::jwalk::walk_file(bytes, len, skeleton, r, ops);
    info->verdict = (int)r.verdict;
    info->reason = (int)r.reason;
    info->sof_marker = (int)r.sof;
    info->skeleton_len = r.skel_len;
    info->entropy_offset = r.ent_off;
    info->eoi_offset = r.eoi_off;
    return IK_OK;
}

int ik_jpeg_counters(unsigned long long* out) {
    if (!out) return ik::fail(IK_ERR_INVALID, "null pointer");
    out[0] = ik::g_jpeg_gpu_streams.load();
    out[1] = ik::g_jpeg_host_streams.load();
    return IK_OK;
}

}  // extern "C"

#ifdef IK_JPEG_DUMP
// dev experiment: part `what` of image i of the last self-synchronising batch
// (0 unstuffed bytes, 1 interval bits, 2 lane records, 3 lane bases, 4 coefficients,
// 5 interval lanes, 6 status and fix rounds); returns its size
extern "C" long long ik_dev_jpeg_dump(int i, int what, uint8_t* out, size_t cap) {
    std::lock_guard<std::mutex> lk(ik::g_jdump_mu);
    if (i < 0 || i >= (int)ik::g_jdump.size() || what < 0 || what > 6) return -1;
    const auto& v = ik::g_jdump[i][what];
    if (out) std::memcpy(out, v.data(), std::min(cap, v.size()));
    return (long long)v.size();
}
#endif
