// ik_jsync_plan.h -- the host's share of the self-synchronising JPEG decoder
// (ik_jpeg_sync.h), in offsets and counts: Huffman tables, scan geometry, the lane
// rules, the refinement schedule and the batch's scratch layout.  Plain C++17, no
// HIP: the product's driver (ik_jpeg_decode.cpp jsync_batch) adds the device base
// pointers, and the CPU model (ik_jpeg_model.cpp) runs and exports the same code.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "ik_jpeg_sync.h"

namespace ik {

struct HuffTable {
    bool present = false;
    // canonical decode: maxcode[l], valptr[l], mincode[l]; plus a 9-bit lookahead
    int maxcode[18] = {}, valptr[17] = {}, mincode[17] = {};
    uint8_t vals[256] = {};
    uint8_t look_len[512] = {}, look_val[512] = {};
};

inline bool build_huff(const uint8_t* bits, const uint8_t* vals, int nvals, HuffTable& t) {
    t = HuffTable();
    std::memcpy(t.vals, vals, nvals);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        t.valptr[l] = k;
        t.mincode[l] = code;
        code += bits[l - 1];
        k += bits[l - 1];
        t.maxcode[l] = bits[l - 1] ? code - 1 : -1;
        if (code > (1 << l)) return false;
        code <<= 1;
    }
    t.maxcode[17] = 0x7fffffff;
    // lookahead for codes up to 9 bits
    code = 0;
    k = 0;
    for (int l = 1; l <= 9; ++l) {
        for (int i = 0; i < bits[l - 1]; ++i, ++k, ++code) {
            const int shift = 9 - l;
            for (int f = 0; f < (1 << shift); ++f) {
                t.look_len[(code << shift) | f] = (uint8_t)l;
                t.look_val[(code << shift) | f] = vals[k];
            }
        }
        code <<= 1;
    }
    t.present = true;
    return true;
}

// the kernels' table layout of the 4 DC and 4 AC tables as they stand
inline void pack_tables(const HuffTable* dc, const HuffTable* ac, JpegHuffTables& t) {
    std::memset(&t, 0, sizeof(t));
    for (int k = 0; k < 8; ++k) {
        const HuffTable& h = k < 4 ? dc[k] : ac[k - 4];
        for (int i = 0; i < 512; ++i) t.look[k][i] = (uint16_t)(h.look_len[i] << 8 | h.look_val[i]);
        std::memcpy(t.maxcode[k], h.maxcode, sizeof(h.maxcode));
        std::memcpy(t.valptr[k], h.valptr, sizeof(h.valptr));
        std::memcpy(t.mincode[k], h.mincode, sizeof(h.mincode));
        std::memcpy(t.vals[k], h.vals, sizeof(h.vals));
        int carry = 0;
        for (int l = 1; l <= 16; ++l) {
            if (h.maxcode[l] >= 0) carry = (h.maxcode[l] + 1) << (16 - l);
            t.lj[k][l] = carry;
        }
        if (k < 4) continue;
        for (int i = 0; i < 512; ++i) {  // run/size code and its magnitude bits in one lookup
            const int L = h.look_len[i], rs = h.look_val[i], r = rs >> 4, sz = rs & 15;
            if (!L || !sz || L + sz > 9) continue;
            const int v = (i >> (9 - L - sz)) & ((1 << sz) - 1);
            const int val = v < (1 << (sz - 1)) ? v - (1 << sz) + 1 : v;
            if (val < -128 || val > 127) continue;
            t.fast_ac[k - 4][i] = (int16_t)(val * 256 + r * 16 + L + sz);
        }
    }
}

namespace jsync {

// what a scan's geometry needs of a frame component
struct CompGeom {
    int h, v, bw, dw, dh, td, ta;  // sampling, blocks across (whole MCUs), downsampled size, table ids
    long long blk0;                // first block in the coefficient image
};

// The geometry of a scan over the ns components comps[order[.]] (L, W at their
// defaults, one interval).  False: more blocks per MCU than a lane state holds.
inline bool scan_geom(const CompGeom* comps, const int* order, int ns, int mcux, int mcuy, Scan& a,
                      long long& total_mcu) {
    const bool single = ns == 1;
    a = Scan{};
    int bpm = 0;
    for (int i = 0; i < ns; ++i) {
        const CompGeom& c = comps[order[i]];
        const int nb = single ? 1 : c.h * c.v;
        for (int k = 0; k < nb; ++k) {
            if (bpm >= kMaxBPM) return false;
            a.comp_of[bpm] = i;
            a.bx_of[bpm] = single ? 0 : k % c.h;
            a.by_of[bpm] = single ? 0 : k / c.h;
            ++bpm;
        }
        a.h[i] = c.h; a.v[i] = c.v; a.bw[i] = c.bw; a.td[i] = c.td; a.ta[i] = c.ta;
        a.blk0[i] = c.blk0;
    }
    const CompGeom& c0 = comps[order[0]];
    const int single_bw = (c0.dw + 7) / 8, single_bh = (c0.dh + 7) / 8;
    total_mcu = single ? (long long)single_bw * single_bh : (long long)mcux * mcuy;
    a.bpm = bpm;
    a.mcux = mcux;
    a.single = single ? 1 : 0;
    a.single_bw = single_bw;
    a.total_blocks = total_mcu * bpm;
    a.ivl_blocks = a.total_blocks;
    a.L = kLaneBits;
    a.W = kWarmBits;
    return true;
}

// ---- lane rules ----
// lanes a batch's self-synchronising decoding aims for (about what the chip holds at once)
constexpr long long kJsyncLanes = 512 << 10;

// the refinement kinds take no lanes
inline bool has_lanes(int kind) { return kind == kBaseline || kind == kDcFirst || kind == kAcFirst; }

// Lane length: 1,024 bits, longer for large batches (up to 4,096) while the batch
// still has ~kJsyncLanes lanes -- a longer lane costs the sync pass less warm-up
// per bit and the fix rounds about as many rounds (ik_jpeg_model.cpp on the
// bench's 4096^2 frames: sync + fix work 2.8x the scan at 1,024, 1.7x at 4,096).
// batch_bits: those of every scan that takes lanes.
inline int lane_bits_for(long long batch_bits) {
    return (int)std::min<long long>(4 * kLaneBits, std::max<long long>(1, batch_bits / kJsyncLanes / kLaneBits) * kLaneBits);
}

// Lanes a scan of len stuffed bytes in nivl intervals can need (whole workgroups of
// 256): its at most 8 * len bits cut into lanes, a partial or empty lane per interval.
inline long long lane_capacity(int kind, size_t len, long long nivl, int lane_bits) {
    return has_lanes(kind) ? ((long long)(8 * len) / lane_bits + nivl + 1 + 255) & ~255ll : 0;
}

// ivl[nivl + 1] interval start bits -> ivl_lane[nivl + 1], each interval's first
// lane: pieces of lane_bits, at least one lane per interval.  False (ivl_lane then
// unspecified): a negative interval, or more lanes than capacity.
inline bool split_lanes(const long long* ivl, long long nivl, int lane_bits, long long capacity, int* ivl_lane) {
    ivl_lane[0] = 0;
    for (long long q = 0; q < nivl; ++q) {
        const long long bits = ivl[q + 1] - ivl[q];
        if (bits < 0) return false;
        ivl_lane[q + 1] = ivl_lane[q] + (int)std::max<long long>(1, (bits + lane_bits - 1) / lane_bits);
    }
    return ivl_lane[nivl] <= capacity;
}

// ---- the batch: scans in file order, image by image ----
struct ScanIn {
    size_t len;        // entropy-coded bytes (stuffed)
    long long nivl;    // restart intervals the frame must have
    int kind, image;
    int comp;          // the (first) component
    bool on_device;    // read where it lies: no scratch copy
    long long total_blocks;
};
struct ImageIn {
    size_t nblocks, plane_bytes;
};

// The refinement scans of the progressive images: launch r takes the r-th DC
// refinement scan of every image that has one; a chain per (image, component) takes
// that component's AC refinement scans in file order.  An image not ok gives nothing.
struct Chain {
    int first, count;  // into rlist
};
struct RefinePlan {
    std::vector<int> rlist;           // [DC launch 0 | DC launch 1 | ... | the chains' scans]
    std::vector<int> dc_sizes;        // scans per DC launch
    std::vector<long long> dc_blocks; // the most total_blocks of a launch's scans
    std::vector<Chain> chains;
};
inline RefinePlan plan_refinement(const ScanIn* sc, int ni, const int* image_ok) {
    RefinePlan P;
    std::vector<std::vector<int>> dc_rounds, ac(4);
    std::vector<int> chained;
    for (int t = 0; t < ni;) {
        const int k = sc[t].image;
        size_t r = 0;
        for (auto& v : ac) v.clear();
        for (; t < ni && sc[t].image == k; ++t) {
            if (!image_ok[k]) continue;
            if (sc[t].kind == kDcRefine) {
                if (dc_rounds.size() <= r) { dc_rounds.emplace_back(); P.dc_blocks.push_back(0); }
                dc_rounds[r].push_back(t);
                P.dc_blocks[r] = std::max(P.dc_blocks[r], sc[t].total_blocks);
                ++r;
            } else if (sc[t].kind == kAcRefine) {
                ac[sc[t].comp].push_back(t);
            }
        }
        for (auto& v : ac)
            if (!v.empty()) {
                P.chains.push_back(Chain{(int)chained.size(), (int)v.size()});
                chained.insert(chained.end(), v.begin(), v.end());
            }
    }
    for (auto& v : dc_rounds) {
        P.dc_sizes.push_back((int)v.size());
        P.rlist.insert(P.rlist.end(), v.begin(), v.end());
    }
    for (Chain& c : P.chains) c.first += (int)P.rlist.size();
    P.rlist.insert(P.rlist.end(), chained.begin(), chained.end());
    return P;
}

// ---- the scratch layout ----
inline size_t up256(size_t x) { return (x + 255) / 256 * 256; }
constexpr int kChunkBytes = 4096;  // an unstuffing chunk

// the sizes of what only the device side defines
struct DevSizes {
    size_t image_dev, recon_item;            // sizeof(JsImageDev), sizeof(JpegReconItem)
    size_t (*chunk_scratch)(long long lanes);  // jsync_chunk_scratch_bytes
};

struct Region {
    size_t off = 0, bytes = 0;  // bytes as asked for; the region holds up256(bytes)
    size_t end() const { return off + up256(bytes); }
};
// A scan has its own unstuffed words, table slot, interval table (progressive: one
// interval), chunks and -- the Ah = 0 kinds -- lane range; the coefficients, planes
// and quantisation tables are the image's.
struct ScanLay {
    Region scan, out, tab;  // scan: none (0, 0) when the scan is on the device
    long long lanes_max, lane0;
    int chunk0, nchunks, ivl0;
};
struct ImageLay {
    Region qt, coef, pl;
    int item0, nitems;
};
struct BatchLayout {
    int lane_bits = 0, nchunks = 0, nivl_total = 0;
    long long lanes_max = 0;
    std::vector<ScanLay> scans;
    std::vector<ImageLay> images;
    // in scratch order; then every scan's [scan | out] and every image's [coef | pl]
    Region img, chunks;                         // + tables, qt: the first upload
    Region status, totals, ivl;                 // the read-back after unstuffing
    Region counts;
    Region scan_tab, ivl_lane, wgs, rlist, chains;  // the second upload
    Region changed, recs, bases, cs, items;
    Region upload1, readback, upload2;          // the three groups, each one transfer
    size_t total = 0;
    // the pinned block: the largest group or the reconstruction items, then the
    // entropy launches' read-back [status | changed]
    size_t pin_changed = 0, pin_bytes = 0;
    size_t in_readback(const Region& r) const { return r.off - readback.off; }
    size_t in_upload2(const Region& r) const { return r.off - upload2.off; }
};

inline BatchLayout plan_layout(const ScanIn* sc, int ni, const ImageIn* im, int m, const DevSizes& z) {
    BatchLayout B;
    B.scans.resize(ni);
    B.images.assign(m, ImageLay{});
    size_t o = 0;
    auto take = [&](size_t bytes) { const Region r{o, bytes}; o += up256(bytes); return r; };
    B.img = take(z.image_dev * ni);
    long long batch_bits = 0;
    for (int t = 0; t < ni; ++t)
        if (has_lanes(sc[t].kind)) batch_bits += 8ll * (long long)sc[t].len;
    B.lane_bits = lane_bits_for(batch_bits);
    for (int t = 0; t < ni; ++t) {
        ScanLay& L = B.scans[t];
        ImageLay& I = B.images[sc[t].image];
        if (!I.nitems++) I.item0 = t;
        L.chunk0 = B.nchunks;
        L.nchunks = (int)((sc[t].len + kChunkBytes - 1) / kChunkBytes);
        B.nchunks += L.nchunks;
        L.ivl0 = B.nivl_total;
        B.nivl_total += (int)sc[t].nivl + 1;
        L.lane0 = B.lanes_max;
        L.lanes_max = lane_capacity(sc[t].kind, sc[t].len, sc[t].nivl, B.lane_bits);
        B.lanes_max += L.lanes_max;
    }
    B.chunks = take(8 * (size_t)B.nchunks);  // int2
    for (ScanLay& L : B.scans) L.tab = take(sizeof(JpegHuffTables));
    for (ImageLay& I : B.images) I.qt = take(512);
    B.upload1 = Region{0, o};
    B.status = take(sizeof(int) * ni);
    B.totals = take(sizeof(uint32_t) * 2 * ni);
    B.ivl = take(sizeof(long long) * B.nivl_total);
    B.readback = Region{B.status.off, o - B.status.off};
    B.counts = take(8 * (size_t)B.nchunks);  // uint2
    B.scan_tab = take(sizeof(Scan) * ni);
    B.ivl_lane = take(sizeof(int) * B.nivl_total);
    B.wgs = take(8 * (size_t)(B.lanes_max / 256));  // int2
    B.rlist = take(sizeof(int) * ni);
    B.chains = take(sizeof(Chain) * 4 * m);
    B.upload2 = Region{B.scan_tab.off, o - B.scan_tab.off};
    B.changed = take(256);
    B.recs = take(sizeof(LaneRec) * (size_t)B.lanes_max);
    B.bases = take(sizeof(LaneBase) * (size_t)B.lanes_max);
    B.cs = take(z.chunk_scratch(B.lanes_max));
    B.items = take(z.recon_item * m);
    for (int t = 0; t < ni; ++t) {
        if (!sc[t].on_device) B.scans[t].scan = take(sc[t].len + 64);
        B.scans[t].out = take(sc[t].len + 4 * kPadWords + 8);
    }
    for (int k = 0; k < m; ++k) {
        B.images[k].coef = take(im[k].nblocks * 64 * sizeof(int16_t));
        B.images[k].pl = take(im[k].plane_bytes);
    }
    B.total = o;
    B.pin_changed = up256(sizeof(int) * ni);
    B.pin_bytes = std::max(std::max(B.upload1.bytes, z.recon_item * m + 256), std::max(B.readback.bytes, B.upload2.bytes)) +
                  B.pin_changed + 256;
    return B;
}

}  // namespace jsync
}  // namespace ik
