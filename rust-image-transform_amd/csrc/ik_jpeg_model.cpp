// ik_jpeg_model.cpp -- CPU model of the GPU self-synchronising JPEG entropy decoder
// (TEST INFRASTRUCTURE: built into libik_jpegmodel.so for the CPU test suite, never
// linked into the product).
//
// Runs the algorithm of ik_jpeg.hip's k_jsync_* kernels -- unstuffing, the sync
// pass with its warm-up, the fix rounds, the per-interval bases, the decode pass --
// on the CPU with the same ik_jpeg_sync.h code, and compares the coefficients with
// a plain serial decode of the same scan (interval by interval from its exact
// start), so that the tests can check the parallel machinery on many streams
// without a GPU and report how many lanes the warm-up synchronised.
//
// Shared with the product, not copied: the kernels' per-lane code (ik_jpeg_sync.h)
// and the host's plan (ik_jsync_plan.h) -- Huffman table build and packing, scan
// geometry, lane capacity and split, and, through ikm_jsync_plan, the lane length,
// the scratch layout and the refinement schedule.  The model's own: the marker
// parsers below (test scaffolding) and the serial reference decoders.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ik_jsync_plan.h"

using namespace ik;
using namespace ik::jsync;

namespace {

const uint8_t kZz[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                         41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                         30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// what both parsers below keep of a file: its tables as they stand and its frame
struct Frame {
    HuffTable dc[4], ac[4];
    std::vector<CompGeom> comps;
    int id[4] = {};
    int W = 0, H = 0, hmax = 1, vmax = 1, mcux = 0, mcuy = 0;
    long long nblocks = 0;
    // s: the SOF payload, its sampling factors checked by the caller
    void frame(const uint8_t* s) {
        H = (int)s[1] << 8 | s[2];
        W = (int)s[3] << 8 | s[4];
        comps.assign(s[5], CompGeom{});
        for (size_t i = 0; i < comps.size(); ++i) {
            id[i] = s[6 + 3 * i];
            comps[i].h = s[7 + 3 * i] >> 4;
            comps[i].v = s[7 + 3 * i] & 15;
            hmax = std::max(hmax, comps[i].h);
            vmax = std::max(vmax, comps[i].v);
        }
        mcux = (W + 8 * hmax - 1) / (8 * hmax);
        mcuy = (H + 8 * vmax - 1) / (8 * vmax);
        for (auto& c : comps) {
            c.bw = mcux * c.h;
            c.dw = (W * c.h + hmax - 1) / hmax;
            c.dh = (H * c.v + vmax - 1) / vmax;
            c.blk0 = nblocks;
            nblocks += (long long)c.bw * mcuy * c.v;
        }
    }
};

// a baseline single-scan JPEG, parsed far enough for the entropy decoder
struct Jpeg : Frame {
    int restart = 0;
    std::vector<int> order;
    const uint8_t* scan = nullptr;
    size_t scan_len = 0;
    bool parse(const uint8_t* b, size_t n) {
        size_t p = 2;
        auto be16 = [&](size_t q) { return (int)b[q] << 8 | b[q + 1]; };
        while (p + 4 <= n) {
            if (b[p] != 0xFF) { ++p; continue; }
            const int m = b[p + 1];
            if (m == 0xFF) { ++p; continue; }
            if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7)) { p += 2; continue; }
            const int len = be16(p + 2);
            const uint8_t* s = b + p + 4;
            const uint8_t* se = b + p + 2 + len;
            if (m == 0xC4) {
                while (s < se) {
                    const int tc = s[0] >> 4, th = s[0] & 15;
                    int total = 0;
                    for (int i = 0; i < 16; ++i) total += s[1 + i];
                    if (!build_huff(s + 1, s + 17, total, tc ? ac[th] : dc[th])) return false;
                    s += 17 + total;
                }
            } else if (m == 0xDD) {
                restart = be16(p + 4);
            } else if (m == 0xC0 || m == 0xC1) {
                if (s[5] > 4) return false;
                frame(s);
            } else if (m == 0xC2) {
                return false;  // progressive: not this decoder's
            } else if (m == 0xDA) {
                const int ns = s[0];
                for (int i = 0; i < ns; ++i) {
                    for (int k = 0; k < (int)comps.size(); ++k)
                        if (id[k] == s[1 + 2 * i]) {
                            comps[k].td = s[2 + 2 * i] >> 4;
                            comps[k].ta = s[2 + 2 * i] & 15;
                            order.push_back(k);
                        }
                }
                scan = se;
                // the scan ends at the first marker that is not RSTn (or stuffing)
                size_t q = (size_t)(se - b);
                while (q + 1 < n && !(b[q] == 0xFF && b[q + 1] != 0x00 && b[q + 1] != 0xFF &&
                                      !(b[q + 1] >= 0xD0 && b[q + 1] <= 0xD7)))
                    ++q;
                scan_len = (q + 1 < n ? q : n) - (size_t)(se - b);
                return true;
            }
            p += 2 + len;
        }
        return false;
    }
};

struct Model {
    Jpeg J;
    JpegHuffTables T;
    std::vector<uint32_t> words;
    std::vector<long long> ivl;
    std::vector<int> ivl_lane;
    Scan S{};
    long long total_mcu = 0;

    bool setup() {
        pack_tables(J.dc, J.ac, T);
        const int L = S.L, W = S.W;  // (the caller's)
        if (!scan_geom(J.comps.data(), J.order.data(), (int)J.order.size(), J.mcux, J.mcuy, S, total_mcu)) return false;
        S.L = L;
        S.W = W;
        if (J.restart) S.ivl_blocks = (long long)J.restart * S.bpm;  // as defer_jsync
        // unstuff, byte by byte (the GPU's rule)
        std::vector<uint8_t> out;
        ivl.assign(1, 0);
        const uint8_t* b = J.scan;
        const size_t n = J.scan_len;
        for (size_t i = 0; i < n; ++i) {
            const int prev = i ? b[i - 1] : -1, cur = b[i], next = i + 1 < n ? b[i + 1] : -1;
            if (unstuff_bad(cur, next, i + 1 == n)) return false;
            if (unstuff_rst(cur, next)) ivl.push_back((long long)out.size() * 8);
            if (unstuff_keep(prev, cur, next, i + 1 == n)) out.push_back((uint8_t)cur);
        }
        const long long nbits = (long long)out.size() * 8;
        ivl.push_back(nbits);
        const long long want_ivl = J.restart ? (total_mcu + J.restart - 1) / J.restart : 1;
        if ((long long)ivl.size() - 1 != want_ivl) return false;
        words.assign((out.size() + 3) / 4 + kPadWords, 0u);
        for (size_t i = 0; i < out.size(); ++i) words[i >> 2] |= (uint32_t)out[i] << (24 - 8 * (i & 3));
        ivl_lane.assign(ivl.size(), 0);
        if (!split_lanes(ivl.data(), want_ivl, S.L, lane_capacity(kBaseline, n, want_ivl, S.L), ivl_lane.data())) return false;
        S.words = words.data();
        S.ivl = ivl.data();
        S.nivl = (int)ivl.size() - 1;
        S.ivl_lane = ivl_lane.data();
        S.tabs = &T;
        return true;
    }
};

}  // namespace

namespace {

// what the lane scheme did on one scan
struct LaneStats {
    long long lanes = 0, bad0 = 0, rounds = 0, decoded = 0, redone = 0;
    long long run_blocks = 0;  // AC first: blocks in units of more than one block (EOB runs)
};

// The lane scheme on one scan (S.kind 0, 1 or 3): sync pass, fix rounds, bases, decode
// pass into par (the image's [block][64]).  1 ok, 0 an inconsistency or a bad code,
// -2 the fix rounds did not end.
int lanes_decode(const Scan& S, const JpegHuffTables& T, const std::vector<int>& ivl_lane_v, int16_t* par, LaneStats& st) {
    const int nl = ivl_lane_v.back();
    // lane -> (interval, index)
    std::vector<int> lane_ivl(nl), lane_q(nl);
    for (int k = 0; k < S.nivl; ++k)
        for (int l = ivl_lane_v[k]; l < ivl_lane_v[k + 1]; ++l) { lane_ivl[l] = k; lane_q[l] = l - ivl_lane_v[k]; }
    long long decoded = 0;
    // 1. sync pass
    std::vector<LaneRec> R(nl);
    for (int l = 0; l < nl; ++l) {
        const LaneGeom g = lane_geom(S, lane_ivl[l], lane_q[l]);
        run_lane(S, T, kZz, g, warm_start(S, g), R[l]);
        decoded += R[l].work;
    }
    auto consistent = [&](int l) {
        if (lane_q[l] == 0) return true;
        return R[l - 1].exit != 0 && R[l].start == R[l - 1].exit;
    };
    long long bad0 = 0;
    for (int l = 0; l < nl; ++l) bad0 += !consistent(l);
    // 2. fix rounds (each reads the previous round's records)
    int rounds = 0;
    long long redone = 0;
    for (;;) {
        std::vector<int> todo;
        for (int l = 0; l < nl; ++l)
            if (!consistent(l) && R[l - 1].exit != 0) todo.push_back(l);
        if (todo.empty()) break;
        ++rounds;
        std::vector<LaneRec> prevR = R;
        for (int l : todo) {
            const LaneGeom g = lane_geom(S, lane_ivl[l], lane_q[l]);
            run_lane(S, T, kZz, g, prevR[l - 1].exit, R[l]);
            decoded += R[l].work;
            ++redone;
        }
        if (rounds > nl + 2) return -2;
    }
    st.lanes = nl;
    st.bad0 = bad0;
    st.rounds = rounds;
    st.decoded = decoded;
    st.redone = redone;
    // 3. bases per interval (cut the end padding's blocks), errors
    std::vector<long long> base(nl);
    std::vector<int> cnt(nl);
    std::vector<int> dcb(4 * (size_t)nl);
    bool ok = true;
    for (int k = 0; k < S.nivl && ok; ++k) {
        const long long want = k + 1 < S.nivl ? S.ivl_blocks : S.total_blocks - (long long)k * S.ivl_blocks;
        long long b = 0;
        int dc[4] = {0, 0, 0, 0};
        for (int l = ivl_lane_v[k]; l < ivl_lane_v[k + 1]; ++l) {
            if (!consistent(l)) { ok = false; break; }
            base[l] = (long long)k * S.ivl_blocks + b;
            for (int c = 0; c < 4; ++c) { dcb[4 * l + c] = dc[c]; dc[c] += R[l].dc[c]; }
            long long take = std::min<long long>(R[l].nblk, want - b);
            if (take < 0) take = 0;
            // a bad code within the interval's real blocks is an error
            if (R[l].err && R[l].err - 1 < take) { ok = false; break; }
            cnt[l] = (int)take;
            b += take;
        }
        if (b != want) ok = false;
    }
    // 4. decode pass
    for (int l = 0; l < nl && ok; ++l) {
        if (!cnt[l]) continue;
        Bits br;
        const LaneGeom g = lane_geom(S, lane_ivl[l], lane_q[l]);
        br.init(S.words, st_bit(R[l].start), g.e);
        int j = st_j(R[l].start);
        if (S.kind != kBaseline) {
            LaneBase B{};
            B.block = base[l];
            B.count = cnt[l];
            for (int c = 0; c < 4; ++c) B.dc[c] = dcb[4 * l + c];
            ok = S.kind == kDcFirst ? decode_lane_prog<kDcFirst>(S, T, kZz, br, j, B, par)
                                    : decode_lane_prog<kAcFirst>(S, T, kZz, br, j, B, par);
            if (S.kind == kAcFirst && ok) {  // the blocks its EOB runs cover (a statistic)
                Bits b2;
                b2.init(S.words, st_bit(R[l].start), g.e);
                for (long long i = 0; i < cnt[l];) {
                    const int nb = ac_first_unit<false>(b2, T, kZz, S.ta[0], S.Ss, S.Se, S.Al, (int16_t*)nullptr);
                    if (nb > 1) st.run_blocks += std::min<long long>(nb, cnt[l] - i);
                    i += nb;
                }
            }
            continue;
        }
        int pred[4];
        for (int c = 0; c < 4; ++c) pred[c] = dcb[4 * l + c];
        for (int i = 0; i < cnt[l]; ++i) {
            const long long bi = block_index(S, base[l] + i);
            int16_t* blk = &par[(size_t)bi * 64];
            const int c = S.comp_of[j];
            int diff;
            if (!block<true>(br, T, kZz, S.td[c], S.ta[c], &diff, blk)) { ok = false; break; }
            pred[c] += diff;
            blk[0] = (int16_t)pred[c];
            j = j + 1 == S.bpm ? 0 : j + 1;
        }
    }
    return ok ? 1 : 0;
}

}  // namespace

extern "C" {

// Decode the scan of a baseline JPEG both ways and report:
// stats[0] lanes, [1] lanes inconsistent after the sync pass, [2] fix rounds,
// [3] blocks decoded by the sync pass + fix rounds (incl. warm-up), [4] total
// blocks, [5] 1 if the parallel coefficients equal the serial decode's,
// [6] intervals, [7] lanes re-decoded over all fix rounds, [8] longest fix chain.
// coef_out (may be null): the parallel decode's coefficients ([block][64]).
// Returns 0, or -1 when the stream is not a single-scan baseline JPEG the model takes.
int ikm_jsync_decode(const uint8_t* jpeg, size_t n, int lane_bits, int warm_bits, int16_t* coef_out, size_t coef_cap,
                     long long* stats) {
    Model M;
    M.S.L = lane_bits > 0 ? lane_bits : kLaneBits;
    M.S.W = warm_bits >= 0 ? warm_bits : kWarmBits;
    if (!M.J.parse(jpeg, n) || M.J.order.size() != M.J.comps.size() || !M.setup()) return -1;
    const Scan& S = M.S;
    const JpegHuffTables& T = M.T;
    std::vector<int16_t> par((size_t)M.J.nblocks * 64, 0);
    LaneStats ls;
    const int lrc = lanes_decode(S, T, M.ivl_lane, par.data(), ls);
    if (lrc < 0) return lrc;
    const bool ok = lrc == 1;
    const long long bad0 = ls.bad0, decoded = ls.decoded, redone = ls.redone;
    const int nl = (int)ls.lanes, rounds = (int)ls.rounds;
    // serial reference: every interval from its exact start
    std::vector<int16_t> ser((size_t)M.J.nblocks * 64, 0);
    bool sok = true;
    for (int k = 0; k < S.nivl && sok; ++k) {
        const long long want = k + 1 < S.nivl ? S.ivl_blocks : S.total_blocks - (long long)k * S.ivl_blocks;
        Bits br;
        br.init(S.words, (uint64_t)S.ivl[k], (uint64_t)S.ivl[k + 1]);
        int pred[4] = {0, 0, 0, 0};
        for (long long i = 0; i < want; ++i) {
            const long long b = (long long)k * S.ivl_blocks + i;
            const int j = (int)(b % S.bpm);
            const int c = S.comp_of[j];
            int16_t* blk = &ser[(size_t)block_index(S, b) * 64];
            int diff;
            if (!block<true>(br, T, kZz, S.td[c], S.ta[c], &diff, blk)) { sok = false; break; }
            pred[c] += diff;
            blk[0] = (int16_t)pred[c];
        }
    }
    if (stats) {
        stats[0] = nl;
        stats[1] = bad0;
        stats[2] = rounds;
        stats[3] = decoded;
        stats[4] = S.total_blocks;
        stats[5] = ok && sok && par == ser;
        stats[6] = S.nivl;
        stats[7] = redone;
        stats[8] = M.ivl_lane.back();
    }
    if (coef_out && ok) std::memcpy(coef_out, par.data(), std::min(coef_cap, par.size()) * sizeof(int16_t));
    return ok ? 0 : 1;
}

}  // extern "C"

// ---- progressive files without restart markers ----------------------------------------
namespace {

// one scan of a progressive file, with the Huffman tables as they stand at its SOS
struct PScan {
    std::vector<int> order;   // components, in scan order
    int td[4] = {}, ta[4] = {};
    int Ss = 0, Se = 0, Ah = 0, Al = 0, kind = 0;
    JpegHuffTables T;
    const uint8_t* data = nullptr;
    size_t len = 0;
    std::vector<uint32_t> words;  // unstuffed
    long long nbits = 0;
};

struct ProgFile : Frame {
    std::vector<PScan> scans;

    // false: not a restart-free 8-bit SOF2 file whose scans pass the host parser's checks
    bool parse(const uint8_t* b, size_t n) {
        if (n < 4 || b[0] != 0xFF || b[1] != 0xD8) return false;
        size_t p = 2;
        auto be16 = [&](size_t q) { return (int)b[q] << 8 | b[q + 1]; };
        bool have_frame = false;
        int restart = 0;
        while (p + 4 <= n) {
            if (b[p] != 0xFF) { ++p; continue; }
            const int m = b[p + 1];
            if (m == 0xFF) { ++p; continue; }
            if (m == 0xD9) break;
            if (m == 0xD8 || m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { p += 2; continue; }
            const int len = be16(p + 2);
            if (len < 2 || p + 2 + len > n) return false;
            const uint8_t* s = b + p + 4;
            const uint8_t* se = b + p + 2 + len;
            if (m == 0xC4) {
                while (s < se) {
                    const int tc = s[0] >> 4, th = s[0] & 15;
                    if (th > 3 || tc > 1 || s + 17 > se) return false;
                    int total = 0;
                    for (int i = 0; i < 16; ++i) total += s[1 + i];
                    if (total > 256 || s + 17 + total > se) return false;
                    if (!build_huff(s + 1, s + 17, total, tc ? ac[th] : dc[th])) return false;
                    s += 17 + total;
                }
            } else if (m == 0xDD) {
                restart = be16(p + 4);
            } else if (m == 0xC2) {
                if (have_frame || s[0] != 8) return false;
                const int nc = s[5];
                if (!be16(p + 5) || !be16(p + 7) || (nc != 1 && nc != 3 && nc != 4)) return false;
                for (int i = 0; i < nc; ++i) {
                    const int h = s[7 + 3 * i] >> 4, v = s[7 + 3 * i] & 15;
                    if (h < 1 || h > 4 || v < 1 || v > 4) return false;
                }
                frame(s);
                have_frame = true;
            } else if (m >= 0xC0 && m <= 0xCF && m != 0xC8 && m != 0xCC) {
                return false;  // any other frame type
            } else if (m == 0xDA) {
                if (!have_frame || restart) return false;
                PScan sc;
                const int ns = s[0];
                if (ns < 1 || ns > (int)comps.size() || se - s < 1 + 2 * ns + 3) return false;
                for (int i = 0; i < ns; ++i) {
                    int k = -1;
                    for (int j = 0; j < (int)comps.size(); ++j)
                        if (id[j] == s[1 + 2 * i]) k = j;
                    if (k < 0) return false;
                    sc.td[i] = s[2 + 2 * i] >> 4;
                    sc.ta[i] = s[2 + 2 * i] & 15;
                    if (sc.td[i] > 3 || sc.ta[i] > 3) return false;
                    sc.order.push_back(k);
                }
                sc.Ss = s[1 + 2 * ns];
                sc.Se = s[2 + 2 * ns];
                sc.Ah = s[3 + 2 * ns] >> 4;
                sc.Al = s[3 + 2 * ns] & 15;
                if (sc.Ss == 0) {
                    if (sc.Se != 0) return false;
                    sc.kind = sc.Ah ? kDcRefine : kDcFirst;
                } else {
                    if (sc.Se < sc.Ss || sc.Se > 63 || ns != 1) return false;
                    sc.kind = sc.Ah ? kAcRefine : kAcFirst;
                }
                if (sc.Al > 13) return false;
                for (int i = 0; i < ns; ++i) {
                    if (sc.kind == kDcFirst && !dc[sc.td[i]].present) return false;
                    if (sc.kind >= kAcFirst && !ac[sc.ta[i]].present) return false;
                }
                pack_tables(dc, ac, sc.T);
                // the scan ends at the first marker (an RSTn is a stray one here)
                size_t q = (size_t)(se - b);
                while (q + 1 < n && !(b[q] == 0xFF && b[q + 1] != 0x00 && b[q + 1] != 0xFF)) ++q;
                const bool at_marker = q + 1 < n;
                if (at_marker && b[q + 1] >= 0xD0 && b[q + 1] <= 0xD7) return false;
                size_t e = at_marker ? q : n;
                if (at_marker)
                    while (e > (size_t)(se - b) && b[e - 1] == 0xFF) --e;  // fill bytes before the marker
                sc.data = se;
                sc.len = e - (size_t)(se - b);
                scans.push_back(std::move(sc));
                p = q;
                continue;
            }
            p += 2 + len;
        }
        return have_frame && !scans.empty();
    }
};

// the lane scheme's view of scan sc (as ik_jpeg_decode.cpp defer_free records it)
bool prog_scan_geom(const ProgFile& F, PScan& sc, int L, int W, Scan& S, std::vector<long long>& ivl,
                    std::vector<int>& ivl_lane) {
    std::vector<CompGeom> cg = F.comps;  // with the table ids of this scan's SOS
    for (size_t i = 0; i < sc.order.size(); ++i) { cg[sc.order[i]].td = sc.td[i]; cg[sc.order[i]].ta = sc.ta[i]; }
    long long total_mcu = 0;
    if (!scan_geom(cg.data(), sc.order.data(), (int)sc.order.size(), F.mcux, F.mcuy, S, total_mcu)) return false;
    S.L = L;
    S.W = W;
    S.kind = sc.kind; S.Ss = sc.Ss; S.Se = sc.Se; S.Al = sc.Al;
    // unstuff, byte by byte (the GPU's rule)
    std::vector<uint8_t> out;
    for (size_t i = 0; i < sc.len; ++i) {
        const int prev = i ? sc.data[i - 1] : -1, cur = sc.data[i], next = i + 1 < sc.len ? sc.data[i + 1] : -1;
        if (unstuff_bad(cur, next, i + 1 == sc.len) || unstuff_rst(cur, next)) return false;
        if (unstuff_keep(prev, cur, next, i + 1 == sc.len)) out.push_back((uint8_t)cur);
    }
    sc.nbits = (long long)out.size() * 8;
    sc.words.assign((out.size() + 3) / 4 + kPadWords, 0u);
    for (size_t i = 0; i < out.size(); ++i) sc.words[i >> 2] |= (uint32_t)out[i] << (24 - 8 * (i & 3));
    ivl.assign({0, sc.nbits});
    ivl_lane.assign(2, 0);
    if (!split_lanes(ivl.data(), 1, L, lane_capacity(kDcFirst, sc.len, 1, L), ivl_lane.data())) return false;
    S.words = sc.words.data();
    S.ivl = ivl.data();
    S.nivl = 1;
    S.ivl_lane = ivl_lane.data();
    S.tabs = &sc.T;
    return true;
}

// One scan by the host decoder's rules (ik_jpeg_decode.cpp Decoder::scan: block by
// block in scan order, an EOB run counted down per block, zeros past the data).
bool serial_scan(const Scan& S, const PScan& sc, int16_t* coef) {
    Bits br;
    br.init(S.words, 0, (uint64_t)sc.nbits);
    int pred[4] = {0, 0, 0, 0};
    int eobrun = 0;
    WordReader rd{br, sc.T};
    for (long long b = 0; b < S.total_blocks; ++b) {
        const int j = (int)(b % S.bpm), c = S.comp_of[j];
        int16_t* blk = coef + block_index(S, b) * 64;
        if (sc.kind == kDcFirst) {
            const int t = sym(br, sc.T, S.td[c]);
            if (t < 0 || t > 11) return false;
            pred[c] += t ? extend(getbits(br, t), t) : 0;
            blk[0] = (int16_t)(pred[c] * (1 << sc.Al));
        } else if (sc.kind == kDcRefine) {
            if (getbits(br, 1)) blk[0] = (int16_t)(blk[0] | (1 << sc.Al));
        } else if (sc.kind == kAcFirst) {
            if (eobrun > 0) { --eobrun; continue; }
            for (int k = sc.Ss; k <= sc.Se; ++k) {
                const int rs = sym(br, sc.T, 4 + S.ta[c]);
                if (rs < 0) return false;
                const int r = rs >> 4, sz = rs & 15;
                if (sz) {
                    k += r;
                    if (k > sc.Se) return false;
                    blk[kZz[k]] = (int16_t)(extend(getbits(br, sz), sz) * (1 << sc.Al));
                } else if (r == 15) {
                    k += 15;
                } else {
                    eobrun = (1 << r) + (r ? getbits(br, r) : 0) - 1;
                    break;
                }
            }
        } else {
            if (ac_refine_block(rd, kZz, S.ta[c], blk, sc.Ss, sc.Se, sc.Al, eobrun)) return false;
        }
    }
    return true;
}

}  // namespace

extern "C" {

// Decode a progressive JPEG without restart markers two ways: every scan serially by
// the host decoder's rules, and the Ah = 0 scans by the lane scheme (the Ah > 0 scans
// by the serial rules, DC refinement through dc_refine_bit as k_jprog_dc_refine).
// lane_bits 0: the serial way alone, its coefficients into coef_out.
// stats: [0] lanes over the Ah = 0 scans, [1] lanes inconsistent after the sync pass,
// [2] fix rounds (the most of any scan), [3] blocks over all scans, [4] 1 if the two
// ways agree, [5] scans, [6] Ah = 0 scans, [7] most lanes of a DC-first scan, [8] most
// lanes of an AC-first scan, [9] / [10] lanes and EOB-run-covered blocks of the
// AC-first scan with the most covered blocks per lane.
// Returns 0; -1 for anything but a restart-free 8-bit SOF2 file whose scans pass the
// host parser's checks; 1 when a way met a bad code or an inconsistency.
int ikm_jprog_decode(const uint8_t* jpeg, size_t n, int lane_bits, int warm_bits, int16_t* coef_out, size_t coef_cap,
                     long long* stats) {
    ProgFile F;
    if (!F.parse(jpeg, n)) return -1;
    const bool serial_only = lane_bits == 0;
    const int L = lane_bits > 0 ? lane_bits : kLaneBits, W = warm_bits >= 0 ? warm_bits : kWarmBits;
    std::vector<int16_t> par((size_t)F.nblocks * 64, 0), ser((size_t)F.nblocks * 64, 0);
    long long st[11] = {};
    bool ok = true, sok = true;
    for (PScan& sc : F.scans) {
        Scan S;
        std::vector<long long> ivl;
        std::vector<int> ivl_lane;
        if (!prog_scan_geom(F, sc, L, W, S, ivl, ivl_lane)) return -1;
        st[3] += S.total_blocks;
        st[5] += 1;
        if (sok && !serial_scan(S, sc, ser.data())) sok = false;
        if (serial_only || !ok) continue;
        if (sc.Ah == 0) {
            LaneStats ls;
            const int rc = lanes_decode(S, sc.T, ivl_lane, par.data(), ls);
            if (rc < 0) return rc;
            ok = rc == 1;
            st[0] += ls.lanes;
            st[1] += ls.bad0;
            st[2] = std::max(st[2], ls.rounds);
            st[6] += 1;
            if (sc.kind == kDcFirst) st[7] = std::max(st[7], ls.lanes);
            else {
                st[8] = std::max(st[8], ls.lanes);
                if (ls.run_blocks * std::max<long long>(st[9], 1) >= st[10] * ls.lanes) { st[9] = ls.lanes; st[10] = ls.run_blocks; }
            }
        } else if (sc.kind == kDcRefine) {
            for (long long b = 0; b < S.total_blocks; ++b)
                if (dc_refine_bit(S.words, sc.nbits, b)) par[(size_t)block_index(S, b) * 64] |= (int16_t)(1 << sc.Al);
        } else {
            ok = serial_scan(S, sc, par.data());
        }
    }
    st[4] = !serial_only && ok && sok && par == ser;
    if (stats) std::memcpy(stats, st, sizeof(st));
    const std::vector<int16_t>& outv = serial_only ? ser : par;
    if (coef_out && (serial_only ? sok : ok)) std::memcpy(coef_out, outv.data(), std::min(coef_cap, outv.size()) * sizeof(int16_t));
    return (serial_only ? sok : ok && sok) ? 0 : 1;
}

// The host plan of a batch (ik_jsync_plan.h), from lengths alone.  Per scan, in file order image by
// image: len, nivl, kind, image, comp, on_dev, blocks (total_blocks); per image: img_blocks,
// plane_bytes, img_ok (the images the refinement schedule takes).  ivl_bits (may be null): every
// scan's nivl + 1 interval start bits, at the scan's ivl0 as in the batch's interval table.  The
// device-only records' sizes are stand-ins (a scan record 64, a reconstruction item 256, the bases
// pass's scratch 64 per 64 lanes); no layout rule depends on them.  Out, regions as (offset, bytes held):
//  head[10]         lane_bits, total, pin_bytes, pin_changed, nchunks, nivl_total, lanes_max, DC launches, chains, rlist entries
//  regions[19][2]   BatchLayout's regions in its order, img to items, then the groups upload1, readback, upload2
//  per_scan[ni][11] scan (0, 0: none), out, tab, capacity, lane0, ivl0, chunk0, nchunks;  per_image[m][6] qt, coef, pl
//  ivl_lane[nivl_total], split_ok[ni] (1, 0 refused, -1 a scan without lanes): split_lanes
//  rlist[ni], dc_sizes[ni], dc_blocks[ni], chains[4 m][2]: the refinement schedule
int ikm_jsync_plan(int ni, const long long* len, const long long* nivl, const int* kind, const int* image, const int* comp,
                   const int* on_dev, const long long* blocks, int m, const long long* img_blocks, const long long* plane_bytes,
                   const int* img_ok, const long long* ivl_bits, long long* head, long long* regions, long long* per_scan,
                   long long* per_image, int* ivl_lane, int* split_ok, int* rlist, int* dc_sizes, long long* dc_blocks,
                   int* chains) {
    std::vector<ScanIn> sc(ni);
    std::vector<ImageIn> im(m);
    for (int t = 0; t < ni; ++t)
        sc[t] = ScanIn{(size_t)len[t], nivl[t], kind[t], image[t], comp[t], on_dev[t] != 0, blocks[t]};
    for (int k = 0; k < m; ++k) im[k] = ImageIn{(size_t)img_blocks[k], (size_t)plane_bytes[k]};
    const BatchLayout B = plan_layout(sc.data(), ni, im.data(), m, DevSizes{64, 256, [](long long lanes) { return (size_t)((lanes + 63) / 64) * 64; }});
    const RefinePlan R = plan_refinement(sc.data(), ni, img_ok);
    const long long h[10] = {B.lane_bits, (long long)B.total, (long long)B.pin_bytes, (long long)B.pin_changed, B.nchunks,
                             B.nivl_total, B.lanes_max, (long long)R.dc_sizes.size(), (long long)R.chains.size(), (long long)R.rlist.size()};
    std::memcpy(head, h, sizeof(h));
    auto put = [](long long*& o, const Region& r) { *o++ = (long long)r.off; *o++ = (long long)(r.end() - r.off); };
    for (const Region* r : {&B.img, &B.chunks, &B.status, &B.totals, &B.ivl, &B.counts, &B.scan_tab, &B.ivl_lane, &B.wgs, &B.rlist,
                            &B.chains, &B.changed, &B.recs, &B.bases, &B.cs, &B.items, &B.upload1, &B.readback, &B.upload2})
        put(regions, *r);
    for (int t = 0; t < ni; ++t) {
        const ScanLay& L = B.scans[t];
        put(per_scan, L.scan); put(per_scan, L.out); put(per_scan, L.tab);
        for (long long v : {L.lanes_max, L.lane0, (long long)L.ivl0, (long long)L.chunk0, (long long)L.nchunks}) *per_scan++ = v;
        split_ok[t] = -1;
        if (ivl_bits && has_lanes(kind[t]))
            split_ok[t] = split_lanes(ivl_bits + L.ivl0, nivl[t], B.lane_bits, L.lanes_max, ivl_lane + L.ivl0) ? 1 : 0;
    }
    for (const ImageLay& I : B.images) { put(per_image, I.qt); put(per_image, I.coef); put(per_image, I.pl); }
    std::copy(R.rlist.begin(), R.rlist.end(), rlist);
    std::copy(R.dc_sizes.begin(), R.dc_sizes.end(), dc_sizes);
    std::copy(R.dc_blocks.begin(), R.dc_blocks.end(), dc_blocks);
    for (const Chain& c : R.chains) { *chains++ = c.first; *chains++ = c.count; }
    return 0;
}

}  // extern "C"
