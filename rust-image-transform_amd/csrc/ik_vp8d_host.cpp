// ik_vp8d_host.cpp -- host half of the GPU WebP (VP8 lossy) decoder: decode_image's WebP
// branch (reference src/transform.rs:31 load_from_memory_with_format -> image 0.25.8 ->
// WebP), with the pixels of libwebp's WebPDecodeRGB (tests/test_gpu_webp_decode.py).
//
// The host reads what is serial: the RIFF container, the frame header, partition 0
// (segment / filter / quantiser headers, the coefficient probabilities, every
// macroblock's modes; libwebp vp8_dec.c VP8GetHeaders, ParseIntraMode, quant_dec.c
// VP8ParseQuant, tree_dec.c VP8ParseProba, frame_dec.c PrecomputeFilterStrengths) and
// the token partitions (ParseResiduals), an arithmetic code that is one dependent
// chain per partition (libwebp writes one): a wave decoding it on the scalar unit
// took 776 ms for a 4096^2 frame that libwebp decodes whole in 72 ms on one core.  It
// hands the device each MB's non-zero dequantised coefficients; the device
// reconstructs and loop-filters the frame and converts it to RGB (ik_vp8d.hip).
// Files it does not cover -- lossless (VP8L), alpha, animation, anything its parser
// finds unusual, data that runs out -- go to the host decoder (decode_webp), which
// then gives libwebp's answer, error message included.
//
// Alpha behind a switch (IK_WEBP_ALPHA_DECODE=gpu / ik_set_webp_alpha_decode; off by
// default, so that without it nothing changes and because whether it pays has to be
// measured per size first, profiles/webp_alpha_notes.md): a lossy file with one ALPH
// chunk is the same frame plus an 8-bit plane.  The host reads the plane as the
// encoder filtered it -- raw bytes, or a lossless stream decoded by libwebp itself as
// the VP8L file it would be with a header in front (alpha_plane) -- and the device
// undoes the prediction filter (k_vp8d_alpha) and writes RGBA, WebPDecodeRGBA's pixels
// (tests/test_webp_alpha_host.py, tests/test_gpu_webp_alpha.py).
//
// Two drivers over one launch sequence (run_launch): decode_webp_device, one file of
// one ik_decode call, and decode_webp_batch, the lossy files of a batch call together
// -- their host halves in parallel on the worker pool, then one staged area and one
// pair of launches over all of them, laid out by the plan of ik_vp8d_plan.h.
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <ctime>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/imagekit_hip.h"
#include "ik_runtime.h"
#include "ik_vp8d_gpu.h"
#include "ik_vp8d_plan.h"

namespace ik {

namespace {

using namespace vp8d;

uint32_t le16(const uint8_t* p) { return p[0] | (uint32_t)p[1] << 8; }
uint32_t le24(const uint8_t* p) { return le16(p) | (uint32_t)p[2] << 16; }
uint32_t le32(const uint8_t* p) { return le24(p) | (uint32_t)p[3] << 24; }

// where a file's frame lies: the "VP8 " payload, the canvas size an extended header
// gives (0: none), and the ALPH payload (alen 0: the file has none)
struct Chunks {
    size_t off = 0, len = 0;
    uint32_t cw = 0, ch = 0;
    size_t aoff = 0, alen = 0;
};

// the "VP8 " payload of a simple file, or of an extended one without animation and,
// unless with_alpha, without alpha (libwebp webp_dec.c ParseRIFF / ParseVP8X /
// ParseOptionalChunks / ParseVP8Header).  with_alpha: the alpha flag and exactly one
// ALPH chunk before the frame go together; either without the other, or a second
// chunk, is not taken.  false: leave the file to the host decoder
bool find_vp8(const uint8_t* b, size_t n, bool with_alpha, Chunks& c) {
    c = Chunks();
    if (n < 20 || std::memcmp(b, "RIFF", 4) || std::memcmp(b + 8, "WEBP", 4)) return false;
    const size_t riff = le32(b + 4);
    if (riff < 12 || riff + 8 > n) return false;
    const size_t end = riff + 8;  // (libwebp reads no further than the RIFF size)
    size_t p = 12;
    if (p + 8 > end) return false;
    if (!std::memcmp(b + p, "VP8X", 4)) {
        const size_t sz = le32(b + p + 4);
        if (sz < 10 || p + 8 + sz > end) return false;
        const uint8_t flags = b[p + 8];
        if (flags & 0x02) return false;  // animation
        const bool alpha = flags & 0x10;
        if (alpha && !with_alpha) return false;
        c.cw = 1 + le24(b + p + 12);
        c.ch = 1 + le24(b + p + 15);
        p += 8 + sz + (sz & 1);
        bool have_alph = false;
        for (;;) {
            if (p + 8 > end) return false;
            if (!std::memcmp(b + p, "VP8 ", 4)) break;
            if (!std::memcmp(b + p, "VP8L", 4) || !std::memcmp(b + p, "ANIM", 4) || !std::memcmp(b + p, "ANMF", 4))
                return false;
            const size_t csz = le32(b + p + 4);
            if (!std::memcmp(b + p, "ALPH", 4)) {
                if (!alpha || have_alph || !csz || csz > end - (p + 8)) return false;
                have_alph = true;
                c.aoff = p + 8;
                c.alen = csz;
            }
            if (csz > end - (p + 8)) return false;
            p += 8 + csz + (csz & 1);
        }
        if (alpha != have_alph) return false;
    } else if (std::memcmp(b + p, "VP8 ", 4)) {
        return false;
    }
    c.len = le32(b + p + 4);
    c.off = p + 8;
    return c.len >= 10 && c.off + c.len <= end;
}
// the frame size its header gives (c.len >= 10)
uint32_t frame_w(const uint8_t* b, const Chunks& c) { return le16(b + c.off + 6) & 0x3fff; }
uint32_t frame_h(const uint8_t* b, const Chunks& c) { return le16(b + c.off + 8) & 0x3fff; }

// The filtered alpha plane of an ALPH payload a[0 .. alen) for a w x h frame (libwebp
// alpha_dec.c ALPHInit / ALPHDecode): the header byte -- bits 0-1 the compression (0 raw,
// 1 lossless), 2-3 the filter, 4-5 the pre-processing (which changes nothing on the
// decoding side), 6-7 reserved -- then w * h raw bytes, or a VP8L image stream without
// its 5-byte header whose green channel is the plane.  The stream goes to libwebp as
// the lossless file it would be with that header (VP8LDecodeAlphaHeader enters the same
// DecodeImageStream at the same bit); its entropy code is as serial as the VP8 tokens.
// false: libwebp would refuse it, or it is safer that libwebp decides.
bool alpha_plane(const uint8_t* a, size_t alen, uint32_t w, uint32_t h, std::vector<uint8_t>& plane, int& filter,
                 int& compression) {
    if (alen < 1 || !w || !h) return false;
    compression = a[0] & 3;
    filter = (a[0] >> 2) & 3;
    if (compression > 1 || ((a[0] >> 4) & 3) > 1 || (a[0] >> 6) > 1) return false;
    const size_t px = (size_t)w * h;
    if (compression == 0) {
        if (alen - 1 < px) return false;
        plane.assign(a + 1, a + 1 + px);
        return true;
    }
    const size_t body = alen - 1, chunk = 5 + body;
    const size_t file = 20 + chunk + (chunk & 1);
    uint8_t hd[25] = {'R', 'I', 'F', 'F', 0, 0, 0, 0, 'W', 'E', 'B', 'P', 'V', 'P', '8', 'L'};
    auto put32 = [&](int at, uint32_t v) {
        for (int k = 0; k < 4; ++k) hd[at + k] = (uint8_t)(v >> (8 * k));
    };
    put32(4, (uint32_t)(file - 8));
    put32(16, (uint32_t)chunk);
    hd[20] = 0x2f;  // the VP8L signature, then 14 bits width - 1, 14 bits height - 1, alpha, version 0
    put32(21, (w - 1) | (h - 1) << 14 | 1u << 28);
    std::vector<uint8_t> f(file, 0);
    std::copy(hd, hd + 25, f.begin());
    std::copy(a + 1, a + 1 + body, f.begin() + 25);
    plane.resize(px);
    return webp_lossless_green(f.data(), f.size(), w, h, plane.data());
}

struct Parsed {
    DFrame fr;
    std::vector<DMB> mbs;
};

// frame header + partition 0; false: leave the file to the host decoder
bool parse_vp8(const uint8_t* b, size_t off, size_t len, uint32_t cw, uint32_t ch, Parsed& P) {
    const uint8_t* f = b + off;
    const uint32_t bits = le24(f);
    const int key = !(bits & 1), profile = (bits >> 1) & 7, show = (bits >> 4) & 1;
    const uint32_t part0 = bits >> 5;
    if (!key || profile > 3 || !show) return false;
    if (f[3] != 0x9d || f[4] != 0x01 || f[5] != 0x2a) return false;
    const int w = (int)(le16(f + 6) & 0x3fff), h = (int)(le16(f + 8) & 0x3fff);
    if (!w || !h) return false;
    if (cw && (cw != (uint32_t)w || ch != (uint32_t)h)) return false;
    if (part0 >= len || 10 + (size_t)part0 > len) return false;
    DFrame& fr = P.fr;
    std::memset(&fr, 0, sizeof(fr));
    fr.w = w;
    fr.h = h;
    fr.mb_w = (w + 15) >> 4;
    fr.mb_h = (h + 15) >> 4;
    const HostSrc src{b};
    BitReader br;
    const uint32_t p0 = (uint32_t)(off + 10), p0_end = p0 + part0;
    br_init(br, src, p0, p0_end);
    auto get = [&] { return br_bit(br, src, 0x80); };
    br_value(br, src, 1);  // colour space
    br_value(br, src, 1);  // clamping type

    // segment header (ParseSegmentHeader; the defaults of ResetSegmentHeader)
    int use_segment = get(), update_map = 0, absolute = 1;
    int quantizer[4] = {0, 0, 0, 0}, filter_strength[4] = {0, 0, 0, 0};
    int seg_p[3] = {255, 255, 255};
    if (use_segment) {
        update_map = get();
        if (get()) {
            absolute = get();
            for (int s = 0; s < 4; ++s) quantizer[s] = get() ? br_signed_value(br, src, 7) : 0;
            for (int s = 0; s < 4; ++s) filter_strength[s] = get() ? br_signed_value(br, src, 6) : 0;
        }
        if (update_map)
            for (int s = 0; s < 3; ++s) seg_p[s] = get() ? br_value(br, src, 8) : 255;
    }
    // filter header (ParseFilterHeader)
    const int simple = get(), level = br_value(br, src, 6), sharpness = br_value(br, src, 3);
    const int use_lf_delta = get();
    int ref_lf_delta0 = 0, mode_lf_delta0 = 0;
    if (use_lf_delta && get()) {
        for (int i = 0; i < 4; ++i)
            if (get()) {
                const int v = br_signed_value(br, src, 6);
                if (i == 0) ref_lf_delta0 = v;
            }
        for (int i = 0; i < 4; ++i)
            if (get()) {
                const int v = br_signed_value(br, src, 6);
                if (i == 0) mode_lf_delta0 = v;
            }
    }
    fr.filter_type = level == 0 ? 0 : simple ? 1 : 2;
    if (br.eof) return false;

    // token partitions (ParsePartitions): any clipped or empty one is left to libwebp
    const int last = (1 << br_value(br, src, 2)) - 1;
    fr.num_parts = last + 1;
    {
        const size_t start = off + 10 + part0, pend = off + len;
        if (pend - start < 3 * (size_t)last) return false;
        size_t ps = start + 3 * (size_t)last;
        for (int p = 0; p < last; ++p) {
            const size_t psize = le24(b + start + 3 * p);
            if (psize > pend - ps) return false;
            fr.part_off[p] = (uint32_t)ps;
            fr.part_end[p] = (uint32_t)(ps + psize);
            ps += psize;
        }
        if (ps >= pend) return false;
        fr.part_off[last] = (uint32_t)ps;
        fr.part_end[last] = (uint32_t)pend;
    }

    // quantisers (VP8ParseQuant)
    const int base_q0 = br_value(br, src, 7);
    const int dqy1_dc = get() ? br_signed_value(br, src, 4) : 0;
    const int dqy2_dc = get() ? br_signed_value(br, src, 4) : 0;
    const int dqy2_ac = get() ? br_signed_value(br, src, 4) : 0;
    const int dquv_dc = get() ? br_signed_value(br, src, 4) : 0;
    const int dquv_ac = get() ? br_signed_value(br, src, 4) : 0;
    auto clip = [](int v, int m) { return v < 0 ? 0 : v > m ? m : v; };
    for (int s = 0; s < 4; ++s) {
        int q;
        if (use_segment) {
            q = quantizer[s];
            if (!absolute) q += base_q0;
        } else {
            q = base_q0;  // (every segment: libwebp copies segment 0's matrices)
        }
        DSeg& g = fr.seg[s];
        g.y1[0] = (int16_t)kDcTable[clip(q + dqy1_dc, 127)];
        g.y1[1] = (int16_t)kAcTable[clip(q, 127)];
        g.y2[0] = (int16_t)(kDcTable[clip(q + dqy2_dc, 127)] * 2);
        int y2ac = (kAcTable[clip(q + dqy2_ac, 127)] * 101581) >> 16;
        g.y2[1] = (int16_t)(y2ac < 8 ? 8 : y2ac);
        g.uv[0] = (int16_t)kDcTable[clip(q + dquv_dc, 117)];
        g.uv[1] = (int16_t)kAcTable[clip(q + dquv_ac, 127)];
        // loop-filter strengths (PrecomputeFilterStrengths)
        int base_level = level;
        if (use_segment) {
            base_level = filter_strength[s];
            if (!absolute) base_level += level;
        }
        for (int i4 = 0; i4 <= 1; ++i4) {
            int lv = base_level;
            if (use_lf_delta) {
                lv += ref_lf_delta0;
                if (i4) lv += mode_lf_delta0;
            }
            lv = lv < 0 ? 0 : lv > 63 ? 63 : lv;
            if (lv > 0) {
                int il = lv;
                if (sharpness > 0) {
                    il >>= sharpness > 4 ? 2 : 1;
                    if (il > 9 - sharpness) il = 9 - sharpness;
                }
                if (il < 1) il = 1;
                g.ilevel[i4] = (uint8_t)il;
                g.limit[i4] = (uint8_t)(2 * lv + il);
                g.hev[i4] = (uint8_t)(lv >= 40 ? 2 : lv >= 15 ? 1 : 0);
            } else {
                g.limit[i4] = 0;
            }
        }
    }
    get();  // update_proba (ignored on key frames)
    // coefficient probabilities (VP8ParseProba), rows padded to 16
    for (int i = 0; i < 1056; ++i) {
        const int v = br_bit(br, src, kCoeffUpdateProbs[i]) ? br_value(br, src, 8) : kCoeffProbs0[i];
        fr.proba[(i / 11) * 16 + i % 11] = (uint8_t)v;
    }
    fr.use_skip = get();
    const int skip_p = fr.use_skip ? br_value(br, src, 8) : 0;
    if (br.eof) return false;

    // every MB's modes (ParseIntraMode; left contexts reset per row, top per frame)
    const int nmb = fr.mb_w * fr.mb_h;
    P.mbs.assign(nmb, DMB{});
    std::vector<uint8_t> intra_t(4 * fr.mb_w, B_DC);
    for (int mb_y = 0; mb_y < fr.mb_h; ++mb_y) {
        uint8_t intra_l[4] = {B_DC, B_DC, B_DC, B_DC};
        for (int mb_x = 0; mb_x < fr.mb_w; ++mb_x) {
            DMB& m = P.mbs[(size_t)mb_y * fr.mb_w + mb_x];
            uint8_t* top = intra_t.data() + 4 * mb_x;
            if (update_map)
                m.seg = (uint8_t)(!br_bit(br, src, seg_p[0]) ? br_bit(br, src, seg_p[1])
                                                             : br_bit(br, src, seg_p[2]) + 2);
            if (fr.use_skip) m.skip = (uint8_t)br_bit(br, src, skip_p);
            m.is_i4 = (uint8_t)!br_bit(br, src, 145);
            if (!m.is_i4) {
                const int ymode = br_bit(br, src, 156) ? (br_bit(br, src, 128) ? TM_PRED : H_PRED)
                                                       : (br_bit(br, src, 163) ? V_PRED : DC_PRED);
                m.ymode = (uint8_t)ymode;
                std::memset(top, ymode, 4);
                std::memset(intra_l, ymode, 4);
                std::memset(m.bmodes, ymode, 16);
            } else {
                for (int y = 0; y < 4; ++y) {
                    int ymode = intra_l[y];
                    for (int x = 0; x < 4; ++x) {
                        const uint8_t* pr = kBModeProbs + (top[x] * 10 + ymode) * 9;
                        ymode = !br_bit(br, src, pr[0])   ? B_DC
                              : !br_bit(br, src, pr[1])   ? B_TM
                              : !br_bit(br, src, pr[2])   ? B_VE
                              : !br_bit(br, src, pr[3])   ? (!br_bit(br, src, pr[4])   ? B_HE
                                                             : !br_bit(br, src, pr[5]) ? B_RD
                                                                                       : B_VR)
                              : !br_bit(br, src, pr[6])   ? B_LD
                              : !br_bit(br, src, pr[7])   ? B_VL
                              : !br_bit(br, src, pr[8])   ? B_HD
                                                          : B_HU;
                        top[x] = (uint8_t)ymode;
                        m.bmodes[4 * y + x] = (uint8_t)ymode;
                    }
                    intra_l[y] = (uint8_t)ymode;
                }
            }
            m.uvmode = (uint8_t)(!br_bit(br, src, 142)   ? DC_PRED
                                 : !br_bit(br, src, 114) ? V_PRED
                                 : br_bit(br, src, 183)  ? TM_PRED
                                                         : H_PRED);
        }
        if (br.eof) return false;  // (libwebp: "Premature end-of-partition0 encountered.")
    }
    return true;
}

// ---- the token partitions (vp8_dec.c VP8DecodeMB, ParseResiduals, GetCoeffs,
// GetLargeValue) into each MB's non-zero dequantised coefficients ----
struct Tokens {
    std::vector<uint32_t> coef;   // (value << 16) | position in the MB's 384
    std::vector<uint32_t> at;     // per MB its first entry, then the total
    std::vector<uint8_t> flags;   // per MB: some coefficient is non-zero
};

constexpr uint8_t kCat3[] = {173, 148, 140, 0}, kCat4[] = {176, 155, 140, 135, 0},
                  kCat5[] = {180, 157, 141, 134, 130, 0},
                  kCat6[] = {254, 254, 243, 230, 196, 177, 153, 140, 133, 130, 129, 0};
constexpr const uint8_t* kCat[4] = {kCat3, kCat4, kCat5, kCat6};

struct TokenReader {
    BitReader br;
    HostSrc src;
    const uint8_t* proba;  // DFrame::proba rows
    std::vector<uint32_t>* out;

    int bit(int p) { return br_bit(br, src, p); }
    const uint8_t* row(int type, int b, int ctx) const { return proba + ((type * 8 + b) * 3 + ctx) * 16; }
    int large_value(const uint8_t* p) {
        if (!bit(p[3])) return !bit(p[4]) ? 2 : 3 + bit(p[5]);
        if (!bit(p[6])) {
            if (!bit(p[7])) return 5 + bit(159);
            int v = 7 + 2 * bit(165);
            return v + bit(145);
        }
        const int b1 = bit(p[8]);
        const int b0 = bit(p[9 + b1]);
        const int cat = 2 * b1 + b0;
        int v = 0;
        for (const uint8_t* t = kCat[cat]; *t; ++t) v += v + bit(*t);
        return v + 3 + (8 << cat);
    }
    // one block from position n: its entries at base + zigzag(n); returns the position
    // after its last token, *dc the stored value of position 0
    int coeffs(int type, int ctx, int dq0, int dq1, int n, uint32_t base, int* dc) {
        const uint8_t* p = row(type, band(n), ctx);
        for (; n < 16; ++n) {
            if (!bit(p[0])) return n;
            while (!bit(p[1])) {
                if (++n == 16) return 16;
                p = row(type, band(n), 0);
            }
            int v;
            const uint8_t* next;
            if (!bit(p[2])) {
                v = 1;
                next = row(type, band(n + 1), 1);
            } else {
                v = large_value(p);
                next = row(type, band(n + 1), 2);
            }
            const int16_t q = (int16_t)((bit(0x80) ? -v : v) * (n > 0 ? dq1 : dq0));
            if (n == 0) *dc = q;
            out->push_back((uint32_t)(uint16_t)q << 16 | (base + (uint32_t)zigzag(n)));
            p = next;
        }
        return 16;
    }
};

// contexts packed as libwebp's: bits 0-3 luma columns / rows, 4-5 U, 6-7 V, 8 the Y2 block
bool decode_tokens(const uint8_t* b, const Parsed& P, Tokens& T) {
    const DFrame& fr = P.fr;
    const int mb_w = fr.mb_w, mb_h = fr.mb_h;
    const size_t nmb = (size_t)mb_w * mb_h;
    T.coef.clear();
    T.at.resize(nmb + 1);
    T.flags.resize(nmb);
    std::vector<uint32_t> tnz(mb_w, 0);
    TokenReader R[8];
    for (int p = 0; p < fr.num_parts; ++p) {
        R[p].src = HostSrc{b};
        R[p].proba = fr.proba;
        R[p].out = &T.coef;
        br_init(R[p].br, R[p].src, fr.part_off[p], fr.part_end[p]);
    }
    for (int mb_y = 0; mb_y < mb_h; ++mb_y) {
        TokenReader& t = R[mb_y & (fr.num_parts - 1)];
        uint32_t l = 0;
        for (int mb_x = 0; mb_x < mb_w; ++mb_x) {
            const size_t mb = (size_t)mb_y * mb_w + mb_x;
            const DMB& m = P.mbs[mb];
            T.at[mb] = (uint32_t)T.coef.size();
            uint32_t tc = tnz[mb_x];
            int any = 0;
            if (!(fr.use_skip && m.skip)) {
                const DSeg& q = fr.seg[m.seg];
                int first = 0, ytype = 3;
                if (!m.is_i4) {  // the Y2 block, then its inverse WHT into the blocks' DCs
                    const size_t y2 = T.coef.size();
                    int dcv = 0;
                    const int nz = t.coeffs(1, (int)((tc >> 8) & 1) + (int)((l >> 8) & 1), q.y2[0], q.y2[1], 0, 0, &dcv);
                    const uint32_t bit = nz > 0;
                    tc = (tc & ~0x100u) | bit << 8;
                    l = (l & ~0x100u) | bit << 8;
                    int16_t dc[16] = {0}, out[256];
                    for (size_t k = y2; k < T.coef.size(); ++k) dc[T.coef[k] & 15] = (int16_t)(T.coef[k] >> 16);
                    T.coef.resize(y2);
                    vp8x::itransform_wht(dc, out);
                    for (int k = 0; k < 16; ++k)
                        if (out[16 * k]) {
                            T.coef.push_back((uint32_t)(uint16_t)out[16 * k] << 16 | (uint32_t)(16 * k));
                            any = 1;
                        }
                    first = 1;
                    ytype = 0;
                }
                for (int by = 0; by < 4; ++by) {
                    uint32_t lb = (l >> by) & 1;
                    for (int bx = 0; bx < 4; ++bx) {
                        int dcv = 0;
                        const int nz = t.coeffs(ytype, (int)lb + (int)((tc >> bx) & 1), q.y1[0], q.y1[1], first,
                                                (uint32_t)(4 * by + bx) * 16, &dcv);
                        lb = nz > first;
                        tc = (tc & ~(1u << bx)) | lb << bx;
                        any |= nz > 1 || (first == 0 && dcv != 0);
                    }
                    l = (l & ~(1u << by)) | lb << by;
                }
                for (int c = 0; c < 2; ++c) {
                    const int sh = 4 + 2 * c;
                    for (int by = 0; by < 2; ++by) {
                        uint32_t lb = (l >> (sh + by)) & 1;
                        for (int bx = 0; bx < 2; ++bx) {
                            int dcv = 0;
                            const int nz = t.coeffs(2, (int)lb + (int)((tc >> (sh + bx)) & 1), q.uv[0], q.uv[1], 0,
                                                    (uint32_t)(16 + 4 * c + 2 * by + bx) * 16, &dcv);
                            lb = nz > 0;
                            tc = (tc & ~(1u << (sh + bx))) | lb << (sh + bx);
                            any |= nz > 1 || dcv != 0;
                        }
                        l = (l & ~(1u << (sh + by))) | lb << (sh + by);
                    }
                }
            } else {  // a skipped MB clears the contexts; the Y2 one only for i16
                const uint32_t keep = m.is_i4 ? 0x100u : 0u;
                tc &= keep;
                l &= keep;
            }
            tnz[mb_x] = tc;
            T.flags[mb] = (uint8_t)any;
            if (t.br.eof) return false;  // (libwebp: "Premature end-of-file encountered.")
        }
    }
    T.at[nmb] = (uint32_t)T.coef.size();
    return true;
}

size_t up256(size_t v) { return (v + 255) & ~size_t(255); }

}  // namespace

int webp_decode_mode() {  // IK_WEBP_DECODE: host / gpu (no host fallback: tests) / auto (default)
    const char* e = getenv("IK_WEBP_DECODE");
    if (e && !std::strcmp(e, "host")) return 0;
    if (e && !std::strcmp(e, "gpu")) return 2;
    return 1;
}

// Whether a lossy file with an alpha plane is the GPU path's (IK_WEBP_ALPHA_GPU) or
// libwebp's (IK_WEBP_ALPHA_HOST, the default): ik_set_webp_alpha_decode's value, else
// IK_WEBP_ALPHA_DECODE=host|gpu, read per call as IK_WEBP_DECODE is.  Off by default:
// the alpha plane's entropy decode stays on the host and its un-filtering is one wave
// per plane, so whether the device path wins has to be measured per size first
// (profiles/webp_alpha_notes.md).
std::atomic<int> g_webp_alpha{-1};
int webp_alpha_mode() {
    const int v = g_webp_alpha.load(std::memory_order_relaxed);
    if (v >= 0) return v;
    const char* e = getenv("IK_WEBP_ALPHA_DECODE");
    return e && !std::strcmp(e, "gpu") ? IK_WEBP_ALPHA_GPU : IK_WEBP_ALPHA_HOST;
}

// auto: the device path from this many pixels on.  Measured per frame (decode_image,
// one request; profiles/r06_webp_decode.log): 4096x4096 39.6 ms against libwebp's 62.2,
// 3000x2000 16.9 / 19.5, 2560x1440 11.4 / 12.0, 1920x1080 7.3 / 7.1, 512x512 1.65 / 0.93.
// The host's tokens cost ~1.6 ms per MPix and the reconstruction wavefront
// (mb_w + 2 mb_h) MB steps of ~12-25 us; libwebp ~4 ms per MPix.
constexpr uint64_t kWebpGpuMinPixels = 3000000;

// auto, for a batch (decode_webp_batch): the device path when the batch's lossy files
// total this many pixels.  Starts at the one-frame break-even: that many pixels spread
// over several frames have a shorter critical path than one such frame and share one
// set of launches, so the batch path cannot lose where the one-frame path won
// (profiles/webp_batch_notes.md).
constexpr uint64_t kWebpGpuMinBatchPixels = kWebpGpuMinPixels;

namespace {

std::atomic<unsigned long long> g_webp_gpu{0}, g_webp_host{0};  // ik_webp_counters

// the last batch per device (ik_webp_last_timing)
enum { kWtParseWallMs = 0, kWtParseCoreMs, kWtStageMs, kWtReconMs, kWtRgbMs, kWtGpuImages, kWtHostImages, kWtRows,
       kWtGrid, kWtLaunches, kWtAlphaMs, kWtAlphaCoreMs, kWtAlphaImages, kWtFields };
std::mutex g_wtim_mu;
std::map<int, std::array<double, kWtFields>> g_wtim;

double now_ms() {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
double thread_cpu_ms() {
    timespec ts;
    if (clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts)) return 0;
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}
std::string last_msg() {
    char buf[512];
    ik_last_error(buf, sizeof(buf));
    return buf;
}

// the host half of one accepted file
struct Frame {
    Parsed P;
    Tokens T;
    std::vector<uint8_t> alpha;  // P.fr.channels == 4: the filtered alpha plane, w * h
    size_t bytes() const {
        return P.mbs.capacity() * sizeof(DMB) + (T.coef.capacity() + T.at.capacity()) * 4 + T.flags.capacity() +
               alpha.capacity();
    }
};
// the whole host half of one file: partition 0, the tokens and, with an ALPH chunk
// (c.alen), the filtered alpha plane; false: the file is libwebp's.  *alpha_ms (may be
// null) gets the thread CPU ms of the alpha plane alone.
bool host_half(const uint8_t* b, const Chunks& c, Frame& F, double* alpha_ms) {
    if (!parse_vp8(b, c.off, c.len, c.cw, c.ch, F.P) || !decode_tokens(b, F.P, F.T)) return false;
    DFrame& fr = F.P.fr;
    fr.channels = 3;
    if (!c.alen) return true;
    const double c0 = alpha_ms ? thread_cpu_ms() : 0;
    int filter = 0, compression = 0;
    if (!alpha_plane(b + c.aoff, c.alen, (uint32_t)fr.w, (uint32_t)fr.h, F.alpha, filter, compression)) return false;
    fr.channels = 4;
    fr.alpha_filter = filter;
    if (alpha_ms) *alpha_ms = thread_cpu_ms() - c0;
    return true;
}
constexpr size_t kFrameKeepBytes = 16u << 20;  // host buffers kept between calls up to this much

// One block of memory laid out once: take(bytes) hands out the next 256-byte aligned
// region.  (ik_png_decode.cpp's Carver binds a fixed few named pointers; here the
// regions are per image, so the offsets are kept instead.)
struct Lay {
    size_t cur = 0;
    size_t take(size_t bytes) {
        const size_t o = cur;
        cur += up256(bytes);
        return o;
    }
};
struct FrameLay {
    size_t fr, mb, flags, at, coef, alpha;  // staged: [DFrame][DMB x nmb][flags][entry starts][entries][alpha plane]
    size_t y, u, v, top;                    // device work: the planes, the two top rows
};
void lay_staged(Lay& L, const Frame& F, FrameLay& o) {
    const DFrame& fr = F.P.fr;
    const size_t nmb = (size_t)fr.mb_w * fr.mb_h;
    o.fr = L.take(sizeof(DFrame));
    o.mb = L.take(nmb * sizeof(DMB));
    o.flags = L.take(nmb);
    o.at = L.take((nmb + 1) * 4);
    o.coef = L.take(F.T.coef.size() * 4 + 4);
    o.alpha = fr.channels == 4 ? L.take((size_t)alpha_pitch((uint32_t)fr.w) * fr.h) : 0;
}
void lay_work(Lay& L, const Frame& F, FrameLay& o) {
    const DFrame& fr = F.P.fr;
    o.y = L.take((size_t)fr.mb_w * 16 * fr.mb_h * 16);
    o.u = L.take((size_t)fr.mb_w * 8 * fr.mb_h * 8);
    o.v = L.take((size_t)fr.mb_w * 8 * fr.mb_h * 8);
    o.top = L.take((size_t)2 * fr.mb_w * 32);
}
uint32_t frame_tiles(const DFrame& fr) {
    const uint32_t tr = rgb_tile_rows((uint32_t)fr.w);
    return ((uint32_t)fr.h + tr - 1) / tr;
}
// what a frame adds to a launch's staged + work bytes (the sub-launch cap counts these)
uint64_t frame_launch_bytes(const Frame& F) {
    Lay L;
    FrameLay o;
    lay_staged(L, F, o);
    lay_work(L, F, o);
    return L.cur + sizeof(DImg) + 4 + 4 + (size_t)frame_tiles(F.P.fr) * sizeof(DTile) + 4 * (1 + (size_t)F.P.fr.mb_h);
}

struct LaunchTim {
    double stage_ms = 0, recon_ms = 0, alpha_ms = 0, rgb_ms = 0;
    uint32_t grid = 0;
};

// m parsed frames, in plan order (row_start: m + 1 tickets), through one set of
// launches into new images: one H2D of the staged area
//   [DImg x m][row_start][tiles][the images with a filtered alpha plane] then per frame
//   [DFrame][DMB x nmb][flags][entry starts][entries][alpha plane, rows alpha_pitch(w) apart]
// one memset of the sync words of the work area behind it
//   [ticket, err per image, progress per MB row] then per frame [Y][U][V][top rows]
// the kernels (reconstruction, the alpha filters where a plane has one, colour), the
// err words back, one stream sync.  imgs[k]: the image, or null
// where the device gave the frame up (a row's wait timed out: the device is too busy
// or something is wrong; libwebp decides).  A failure frees every image.
int run_launch(const Frame* const* F, const uint32_t* row_start, int m, ik_image** imgs, int threads, LaunchTim* tim) {
    for (int k = 0; k < m; ++k) imgs[k] = nullptr;
    const uint32_t total_rows = row_start[m];
    uint32_t ntiles = 0;
    for (int k = 0; k < m; ++k) ntiles += frame_tiles(F[k]->P.fr);
    Lay L;
    std::vector<FrameLay> o((size_t)m);
    const size_t o_img = L.take(sizeof(DImg) * (size_t)m);
    const size_t o_rs = L.take(4 * ((size_t)m + 1));
    const size_t o_tiles = L.take(sizeof(DTile) * (size_t)ntiles);
    const size_t o_which = L.take(4 * (size_t)m);
    for (int k = 0; k < m; ++k) lay_staged(L, *F[k], o[k]);
    const size_t stage = L.cur;
    const size_t sync_bytes = 4 * (1 + (size_t)m + total_rows);
    const size_t o_sync = L.take(sync_bytes);
    for (int k = 0; k < m; ++k) lay_work(L, *F[k], o[k]);
    const size_t total = L.cur;

    auto drop = [&] {
        for (int k = 0; k < m; ++k) {
            ik_image_free(imgs[k]);
            imgs[k] = nullptr;
        }
    };
    for (int k = 0; k < m; ++k) {
        const int st = alloc_image((uint32_t)F[k]->P.fr.w, (uint32_t)F[k]->P.fr.h, (uint32_t)F[k]->P.fr.channels, &imgs[k]);
        if (st) {
            drop();
            return st;
        }
    }
    uint8_t* d = scratch_slot(kScratchVp8d, total);
    uint8_t* h = d ? pinned_slot(kPinnedVp8d, stage + up256(4 * (size_t)m)) : nullptr;  // (+ the err words, read back)
    if (!d || !h) {
        drop();
        return d ? IK_ERR_NOMEM : fail(IK_ERR_DEVICE, "cannot allocate the WebP decoder's device work area");
    }
    hipStream_t s = thread_stream();
    (void)hipStreamSynchronize(s);  // (the pinned area may still feed an earlier copy)
    const double t0 = tim ? now_ms() : 0;
    uint32_t* const sync = reinterpret_cast<uint32_t*>(d + o_sync);
    DImg* const himg = reinterpret_cast<DImg*>(h + o_img);
    DTile* const htile = reinterpret_cast<DTile*>(h + o_tiles);
    std::memcpy(h + o_rs, row_start, 4 * ((size_t)m + 1));
    uint32_t prog0 = 0, tile0 = 0, nwhich = 0;
    bool rgba = false;
    uint32_t* const hwhich = reinterpret_cast<uint32_t*>(h + o_which);
    std::vector<uint32_t> first_tile((size_t)m);
    for (int k = 0; k < m; ++k) {
        const DFrame& fr = F[k]->P.fr;
        DImg di{};
        if (fr.channels == 4) {
            rgba = true;
            di.alpha = d + o[k].alpha;
            if (fr.alpha_filter) hwhich[nwhich++] = (uint32_t)k;
        }
        di.fr = reinterpret_cast<const DFrame*>(d + o[k].fr);
        di.mbs = reinterpret_cast<const DMB*>(d + o[k].mb);
        di.flags = d + o[k].flags;
        di.coef_at = reinterpret_cast<const uint32_t*>(d + o[k].at);
        di.coef = reinterpret_cast<const uint32_t*>(d + o[k].coef);
        di.y = d + o[k].y;
        di.u = d + o[k].u;
        di.v = d + o[k].v;
        di.top = d + o[k].top;
        di.out = imgs[k]->d;
        di.ys = (uint32_t)fr.mb_w * 16;
        di.uvs = (uint32_t)fr.mb_w * 8;
        di.out_pitch = (uint32_t)imgs[k]->pitch;
        di.err = sync + 1 + k;
        di.prog = sync + 1 + m + prog0;
        prog0 += (uint32_t)fr.mb_h;
        himg[k] = di;
        first_tile[k] = tile0;
        tile0 += frame_tiles(fr);
    }
    auto fill = [&](int k) {  // frame k's staged records and its tiles
        const Frame& f = *F[k];
        const DFrame& fr = f.P.fr;
        const size_t nmb = (size_t)fr.mb_w * fr.mb_h;
        std::memcpy(h + o[k].fr, &fr, sizeof(DFrame));
        std::memcpy(h + o[k].mb, f.P.mbs.data(), nmb * sizeof(DMB));
        std::memcpy(h + o[k].flags, f.T.flags.data(), nmb);
        std::memcpy(h + o[k].at, f.T.at.data(), (nmb + 1) * 4);
        if (!f.T.coef.empty()) std::memcpy(h + o[k].coef, f.T.coef.data(), f.T.coef.size() * 4);
        if (fr.channels == 4) {  // the plane's rows, alpha_pitch(w) apart
            reinterpret_cast<DFrame*>(h + o[k].fr)->alpha_off = (uint32_t)(o[k].alpha - o[k].fr);
            const size_t w = (size_t)fr.w, ap = alpha_pitch((uint32_t)fr.w);
            for (size_t r = 0; r < (size_t)fr.h; ++r) std::memcpy(h + o[k].alpha + r * ap, f.alpha.data() + r * w, w);
        }
        const uint32_t tr = rgb_tile_rows((uint32_t)fr.w);
        DTile* t = htile + first_tile[k];
        for (uint32_t r = 0; r < (uint32_t)fr.h; r += tr) *t++ = DTile{(uint32_t)k, r, std::min(tr, (uint32_t)fr.h - r)};
    };
    if (m > 1) parallel_for(m, threads, fill);
    else fill(0);

    const DImg* dimg = reinterpret_cast<const DImg*>(d + o_img);
    uint32_t* const herr = reinterpret_cast<uint32_t*>(h + stage);
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};  // after: the alpha kernel, the memset, recon, rgb
    if (tim) {
        const EvPair &p = thread_events(2), &q = thread_events(3);
        ev[0] = p.a, ev[1] = p.b, ev[2] = q.a, ev[3] = q.b;
    }
    hipError_t e = hipMemcpyAsync(d, h, stage, hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(sync, 0, sync_bytes, s);
    if (tim) ev_record(ev[1], s);
    uint32_t grid = 0;
    if (e == hipSuccess)
        e = launch_vp8d_recon(dimg, reinterpret_cast<const uint32_t*>(d + o_rs), m, total_rows, sync, s, &grid);
    if (tim) ev_record(ev[2], s);
    if (e == hipSuccess && nwhich) e = launch_vp8d_alpha(dimg, reinterpret_cast<const uint32_t*>(d + o_which), nwhich, s);
    if (tim) ev_record(ev[0], s);
    if (e == hipSuccess) e = launch_vp8d_rgb(dimg, reinterpret_cast<const DTile*>(d + o_tiles), ntiles, rgba, s);
    if (tim) ev_record(ev[3], s);
    if (e == hipSuccess) e = hipMemcpyAsync(herr, sync + 1, 4 * (size_t)m, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        drop();
        return hip_fail(e, "WebP decode launches");
    }
    if (tim) {
        auto ms = [](hipEvent_t a, hipEvent_t b) {
            float v = 0;
            return a && b && hipEventElapsedTime(&v, a, b) == hipSuccess ? (double)v : 0.0;
        };
        tim->stage_ms += (now_ms() - t0) - ms(ev[1], ev[3]);  // staging copies and the H2D: the wall time less the kernels
        tim->recon_ms += ms(ev[1], ev[2]);
        tim->alpha_ms += ms(ev[2], ev[0]);
        tim->rgb_ms += ms(ev[0], ev[3]);
        tim->grid = std::max(tim->grid, grid);
    }
    for (int k = 0; k < m; ++k)
        if (herr[k]) {
            ik_image_free(imgs[k]);
            imgs[k] = nullptr;
        }
    return IK_OK;
}

void trim_frame(Frame& f) {
    if (f.bytes() > kFrameKeepBytes) f = Frame();
}

// libwebp's decode of one file into a new device image (what decode_image does with
// a WebP file outside the GPU path)
int host_one(const uint8_t* b, size_t n, ik_image** out) {
    thread_local std::vector<uint8_t> px;
    struct Trim {
        ~Trim() { if (px.capacity() > (128u << 20)) std::vector<uint8_t>().swap(px); }
    } trim;
    ++g_webp_host;
    uint32_t w = 0, h = 0, c = 0;
    const int st = decode_webp(b, n, w, h, c, px);
    return st ? st : ik_image_from_host(px.data(), w, h, c, out);
}

int left_to_libwebp() {
    return fail(IK_ERR_TRANSFORM, "IK_WEBP_DECODE=gpu: the GPU WebP decoder leaves this file to libwebp");
}

}  // namespace

void webp_count_host_decode() { ++g_webp_host; }

int decode_webp_device(const uint8_t* b, size_t n, ik_image** out) {
    const int mode = webp_decode_mode();
    if (!mode) return kVp8dHost;
    Chunks c;
    if (!find_vp8(b, n, webp_alpha_mode() == IK_WEBP_ALPHA_GPU, c)) return kVp8dHost;
    if (mode == 1 && (uint64_t)frame_w(b, c) * frame_h(b, c) < kWebpGpuMinPixels) return kVp8dHost;
    thread_local Frame F;  // (per-thread buffers: released after frames over 16 MiB of them)
    struct Trim {
        ~Trim() { trim_frame(F); }
    } trim;
    if (!host_half(b, c, F, nullptr)) return kVp8dHost;
    const Frame* const fp = &F;
    const uint32_t row_start[2] = {0, (uint32_t)F.P.fr.mb_h};
    ik_image* img = nullptr;
    const int st = run_launch(&fp, row_start, 1, &img, 1, nullptr);
    if (st) return st;
    if (!img) return kVp8dHost;
    ++g_webp_gpu;
    *out = img;
    return IK_OK;
}

int decode_webp_batch(const uint8_t* const* b, const size_t* lens, int n, ik_image** outs, int* status,
                      std::string* msgs, int threads) {
    const int mode = webp_decode_mode();
    const double t_begin = now_ms();
    // the files the GPU path would take: a plain lossy frame in the container (with an
    // alpha plane beside it under IK_WEBP_ALPHA_DECODE=gpu)
    struct Cand {
        Chunks c;
        int frame = -1;  // its Frame in the pool, once parsed and accepted: -1 otherwise
        double core_ms = 0, alpha_ms = 0;
    };
    std::vector<Cand> C((size_t)n);
    std::vector<char> take((size_t)n, 0);
    int ncand = 0;
    if (mode) {
        const bool with_alpha = webp_alpha_mode() == IK_WEBP_ALPHA_GPU;
        uint64_t px = 0;
        for (int i = 0; i < n; ++i)
            if (find_vp8(b[i], lens[i], with_alpha, C[i].c)) {
                take[i] = 1;
                ++ncand;
                px += (uint64_t)frame_w(b[i], C[i].c) * frame_h(b[i], C[i].c);
            }
        if (mode == 1 && px < kWebpGpuMinBatchPixels) {
            std::fill(take.begin(), take.end(), 0);
            ncand = 0;
        }
    }
    // the batch's host buffers: kept on the calling thread between batches, released
    // at the batch's end once they hold more than the one-request path would keep
    thread_local std::vector<Frame> pool;
    struct Trim {
        ~Trim() {
            size_t sum = 0;
            for (const Frame& f : pool) sum += f.bytes();
            if (sum > kFrameKeepBytes) std::vector<Frame>().swap(pool);
        }
    } trim;
    if (pool.size() < (size_t)ncand) pool.resize((size_t)ncand);
    for (int i = 0, k = 0; i < n; ++i)
        if (take[i]) C[i].frame = k++;
    Frame* const frames = pool.data();  // (the workers below have pools of their own: this thread's, by address)
    std::atomic<int> host_calls{0};

    // host half, in parallel over the items: partition 0 and the tokens of the taken
    // files; every other file, and any a parser hands back, to libwebp on the same worker
    parallel_for(n, threads, [&](int i) {
        outs[i] = nullptr;
        status[i] = IK_OK;
        if (take[i]) {
            Frame& F = frames[C[i].frame];
            const double c0 = thread_cpu_ms();
            const bool ok = host_half(b[i], C[i].c, F, &C[i].alpha_ms);
            C[i].core_ms = thread_cpu_ms() - c0 - C[i].alpha_ms;
            if (ok) return;
            C[i].frame = -1;
        }
        status[i] = mode == 2 ? left_to_libwebp() : (++host_calls, host_one(b[i], lens[i], &outs[i]));
        if (status[i]) msgs[i] = last_msg();
    });
    std::array<double, kWtFields> W{};
    W[kWtParseWallMs] = now_ms() - t_begin;
    for (int i = 0; i < n; ++i) {
        W[kWtParseCoreMs] += C[i].core_ms;
        W[kWtAlphaCoreMs] += C[i].alpha_ms;
    }

    // the accepted frames: planned (largest first, cut at the cap), then launched
    std::vector<int> acc;  // request index of each accepted frame
    for (int i = 0; i < n; ++i)
        if (C[i].frame >= 0) acc.push_back(i);
    const uint32_t na = (uint32_t)acc.size();
    std::vector<int> retry;  // frames the device gave up
    if (na) {
        uint64_t cap = 256ull << 20;
        if (const char* e = getenv("IK_VP8D_BATCH_BYTES")) {  // dev switch
            const long long v = atoll(e);
            if (v > 0) cap = (uint64_t)v;
        }
        std::vector<uint32_t> mw(na), mh(na), order(na), row_start(na + 1), lo(na + 1);
        std::vector<uint64_t> bytes(na);
        for (uint32_t a = 0; a < na; ++a) {
            const Frame& F = frames[C[acc[a]].frame];
            mw[a] = (uint32_t)F.P.fr.mb_w;
            mh[a] = (uint32_t)F.P.fr.mb_h;
            bytes[a] = frame_launch_bytes(F);
        }
        const int launches = webp_batch_plan(mw.data(), mh.data(), bytes.data(), na, cap, order.data(), row_start.data(),
                                             lo.data());
        LaunchTim tim;
        std::vector<const Frame*> F;
        std::vector<ik_image*> imgs;
        std::vector<uint32_t> rs;
        int failed = IK_OK;  // a failed launch fails its frames and every later launch's
        std::string failed_msg;
        for (int l = 0; l < launches; ++l) {
            const uint32_t k0 = lo[l], m = lo[l + 1] - k0;
            if (!failed) {
                F.resize(m);
                imgs.assign(m, nullptr);
                rs.assign(row_start.begin() + k0, row_start.begin() + k0 + m);
                rs.push_back(rs.back() + mh[order[k0 + m - 1]]);
                for (uint32_t k = 0; k < m; ++k) F[k] = &frames[C[acc[order[k0 + k]]].frame];
                failed = run_launch(F.data(), rs.data(), (int)m, imgs.data(), threads, &tim);
                if (failed) failed_msg = last_msg();
                else W[kWtRows] += rs.back();
            }
            for (uint32_t k = 0; k < m; ++k) {
                const int i = acc[order[k0 + k]];
                if (failed) {
                    status[i] = failed;
                    msgs[i] = failed_msg;
                } else if (imgs[k]) {
                    outs[i] = imgs[k];
                    ++g_webp_gpu;
                    W[kWtGpuImages] += 1;
                    if (F[k]->P.fr.channels == 4) W[kWtAlphaImages] += 1;
                } else {
                    retry.push_back(i);
                }
            }
        }
        W[kWtStageMs] = tim.stage_ms;
        W[kWtReconMs] = tim.recon_ms;
        W[kWtRgbMs] = tim.rgb_ms;
        W[kWtAlphaMs] = tim.alpha_ms;
        W[kWtGrid] = tim.grid;
        W[kWtLaunches] = launches;
    }
    parallel_for((int)retry.size(), threads, [&](int k) {
        const int i = retry[(size_t)k];
        status[i] = mode == 2 ? left_to_libwebp() : (++host_calls, host_one(b[i], lens[i], &outs[i]));
        if (status[i]) msgs[i] = last_msg();
    });
    W[kWtHostImages] = host_calls.load();
    {
        std::lock_guard<std::mutex> lk(g_wtim_mu);
        g_wtim[current_device()] = W;
    }
    if (getenv("IK_TIMING"))  // dev: the batch's phases to stderr
        fprintf(stderr, "vp8d batch of %d: host half %.3f ms (%.3f core-ms) stage+h2d %.3f recon %.3f rgb %.3f ms, %d on the GPU, "
                "%d MB rows, grid %d, %d launches\n", n, W[kWtParseWallMs], W[kWtParseCoreMs], W[kWtStageMs], W[kWtReconMs],
                W[kWtRgbMs], (int)W[kWtGpuImages], (int)W[kWtRows], (int)W[kWtGrid], (int)W[kWtLaunches]);
    int first = IK_OK;
    for (int i = 0; i < n; ++i)
        if (status[i] && !first) first = status[i];
    return first;
}

}  // namespace ik

extern "C" int ik_webp_counters(unsigned long long* out) {
    if (!out) return ik::fail(IK_ERR_INVALID, "null pointer");
    out[0] = ik::g_webp_gpu.load();
    out[1] = ik::g_webp_host.load();
    return IK_OK;
}

extern "C" int ik_webp_last_timing(double* out, int n) {
    if (!out) return ik::fail(IK_ERR_INVALID, "null pointer");
    std::array<double, ik::kWtFields> t{};
    {
        std::lock_guard<std::mutex> lk(ik::g_wtim_mu);
        auto it = ik::g_wtim.find(ik::current_device());
        if (it != ik::g_wtim.end()) t = it->second;
    }
    for (int i = 0; i < n; ++i) out[i] = i < ik::kWtFields ? t[(size_t)i] : 0.0;
    return IK_OK;
}

extern "C" unsigned long long ik_webp_gpu_min_batch_pixels(void) { return ik::kWebpGpuMinBatchPixels; }

extern "C" int ik_set_webp_alpha_decode(int where) {
    if (where != -1 && where != IK_WEBP_ALPHA_HOST && where != IK_WEBP_ALPHA_GPU)
        return ik::fail(IK_ERR_INVALID, "ik_set_webp_alpha_decode: IK_WEBP_ALPHA_HOST, IK_WEBP_ALPHA_GPU or -1");
    ik::g_webp_alpha.store(where, std::memory_order_relaxed);
    return IK_OK;
}
extern "C" int ik_get_webp_alpha_decode(void) { return ik::webp_alpha_mode(); }

extern "C" int ik_webp_alpha_plane(const uint8_t* bytes, size_t len, uint8_t* plane, size_t cap, uint32_t* w, uint32_t* h,
                                   int* filter, int* compression) {
    if (!bytes || !w || !h || !filter || !compression) return ik::fail(IK_ERR_INVALID, "null pointer");
    ik::Chunks c;
    if (!ik::find_vp8(bytes, len, true, c) || !c.alen)
        return ik::fail(IK_ERR_UNSUPPORTED, "not a lossy WebP file with one alpha plane: left to libwebp");
    const uint32_t fw = ik::frame_w(bytes, c), fh = ik::frame_h(bytes, c);
    if (!fw || !fh || fw != c.cw || fh != c.ch)
        return ik::fail(IK_ERR_UNSUPPORTED, "the canvas is not the frame: left to libwebp");
    std::vector<uint8_t> a;
    if (!ik::alpha_plane(bytes + c.aoff, c.alen, fw, fh, a, *filter, *compression))
        return ik::fail(IK_ERR_UNSUPPORTED, "the GPU path leaves this alpha plane to libwebp");
    *w = fw;
    *h = fh;
    if (a.size() > cap || (!plane && !a.empty())) return ik::fail(IK_ERR_INVALID, "the plane needs w * h bytes");
    std::memcpy(plane, a.data(), a.size());
    return IK_OK;
}

extern "C" int ik_webp_batch_plan(const uint32_t* mb_w, const uint32_t* mb_h, const uint64_t* bytes, uint32_t n,
                                  uint64_t cap_bytes, uint32_t* order, uint32_t* row_start, uint32_t* launch_lo) {
    return ik::vp8d::webp_batch_plan(mb_w, mb_h, bytes, n, cap_bytes, order, row_start, launch_lo);
}
