// ik_jpeg_walk.h -- the marker walk over a JPEG file that lies in device memory,
// shared by the GPU kernel (ik_jpeg_walk.hip k_jpeg_walk, one wave per file) and
// the host entry the CPU tests run (ik_jpeg_walk_host, ik_jpeg_decode.cpp).
//
// ik_transform_batch_submit_device decodes baseline JPEG bodies where they lie: the
// self-synchronising decoder (ik_jsync.hip) reads the scan from the caller's
// memory.  What the host parser (ik_jpeg_decode.cpp Decoder::parse) needs of such
// a file is its table and frame segments and two offsets.  The walk hops from
// SOI segment by segment as that parser does (fill FF bytes before a marker are
// skipped; SOI, RSTn and TEM carry no length), copies the segments the parser
// reads -- DQT, DHT, SOFn, DRI, APP0, APP14 and the first SOS header -- verbatim
// and in order into the file's "skeleton" slot, steps over every other segment
// (APPn, COM: EXIF and ICC payloads can be megabytes), and records
//   - the SOF marker,
//   - the offset of the first entropy-coded byte (the end of the first SOS header),
//   - the offset of the file's last FF D9, searched backwards over the window the
//     parser's defer_jsync searches (the last 4 KiB, not before the scan), else
//     the file's length,
//   - a verdict: the file is decoded in place, or copied back to the host (with the
//     reason), or malformed (copied back too: the host parser words the error).
// The skeleton is itself a JPEG header (SOI, the kept segments), so the one host
// parser reads it.  The walk reads no byte at or past the file's length.
#pragma once
#include <stdint.h>

#ifndef IK_HD
#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define IK_HD __host__ __device__ __forceinline__
#else
#define IK_HD inline
#endif
#endif

namespace ik {
namespace jwalk {

// A skeleton slot.  The largest set of segments a baseline file the decoder takes
// needs, each table in a segment of its own (marker 2 + length 2 + payload):
//   SOI                                                        2
//   DQT   4 tables of 16-bit entries: 4 x (4 + 1 + 128)      532
//   DHT   4 DC + 4 AC tables of 256 values: 8 x (4 + 17 + 256)  2,216
//   SOFn  4 components: 4 + 6 + 3 x 4                         22
//   DRI                                                        6
//   APP0  JFIF without a thumbnail                            18
//   APP14 Adobe                                               16
//   SOS   4 components: 4 + 1 + 2 x 4 + 3                     16
// 2,828 bytes; 4 KiB leaves room for repeated tables and a JFXX extension.  A file
// that needs more (a thumbnail in APP0, tables sent many times) is copied back.
constexpr uint32_t kSlot = 4096;
constexpr uint64_t kMinScan = 4096;    // scans under 4 KiB stay on the host decoder (kJsyncMinBytes)
constexpr uint64_t kEoiWindow = 4096;  // defer_jsync looks for the last EOI this far from the end

enum Verdict : uint32_t { kInPlace = 0, kCopyBack = 1, kMalformed = 2 };
enum Reason : uint32_t {
    kNone = 0,
    kNotBaseline = 1,     // not one SOF0 / SOF1 (Huffman, 8 bits) frame before the scan
    kSmallScan = 2,       // the first scan is under the 4 KiB rule
    kNoSos = 3,           // EOI or the end of the file before any SOS
    kSkeletonLarge = 4,   // the kept segments do not fit the slot
    kScanComponents = 5,  // the first SOS names fewer components than the frame
    kGarbage = 6,         // a byte that is not FF where a marker is due (the host parser skips it)
    kBadLength = 7,       // malformed: a segment length under 2 or past the file's end
    kNoSoi = 8,           // malformed: no FF D8 at the start
};

struct Rec {
    uint32_t verdict, reason;
    uint32_t sof;       // the first SOFn marker (0xC0..0xCF), 0 = none
    uint32_t skel_len;  // bytes written to the skeleton slot
    uint64_t ent_off;   // first entropy-coded byte of the first scan (0 = no SOS reached)
    uint64_t eoi_off;   // the file's last FF D9 within the window, else the file's length
};

constexpr uint64_t kNoEoi = ~0ull;

IK_HD bool eoi_at(const uint8_t* f, uint64_t q) { return f[q] == 0xFF && f[q + 1] == 0xD9; }

// The walk of one file.  ops.copy(dst, src, n) copies n bytes (the wave's lanes
// together on the GPU); ops.last_eoi(f, lo, hi) is the largest q in [lo, hi] with
// FF D9 at q, else kNoEoi.  Every lane of a wave runs this with the same values.
template <class Ops>
IK_HD void walk_file(const uint8_t* f, uint64_t n, uint8_t* skel, Rec& r, Ops& ops) {
    r.verdict = kCopyBack;
    r.reason = kNone;
    r.sof = 0;
    r.skel_len = 0;
    r.ent_off = 0;
    r.eoi_off = n;
    if (n < 2 || f[0] != 0xFF || f[1] != 0xD8) {
        r.verdict = kMalformed;
        r.reason = kNoSoi;
        return;
    }
    ops.copy(skel, f, 2);
    uint32_t w = 2;
    uint32_t why = kNone;  // the first reason met to copy the file back
    int ncomp = -1;
    uint64_t p = 2;
    for (;;) {
        if (p < n && f[p] != 0xFF) { why = why ? why : kGarbage; break; }
        while (p < n && f[p] == 0xFF) ++p;
        if (p >= n || f[p] == 0xD9) { why = why ? why : kNoSos; break; }
        const uint32_t m = f[p++];
        if (m == 0xD8 || (m >= 0xD0 && m <= 0xD7) || m == 0x01) continue;
        const uint64_t len = p + 2 <= n ? (uint64_t)f[p] << 8 | f[p + 1] : 0;
        if (len < 2 || len > n - p) {
            r.verdict = kMalformed;
            r.reason = kBadLength;
            r.skel_len = w;
            return;
        }
        const bool sof = m >= 0xC0 && m <= 0xCF && m != 0xC4 && m != 0xC8 && m != 0xCC;
        if (sof) {
            if (r.sof || (m != 0xC0 && m != 0xC1) || len < 8 || f[p + 2] != 8) why = why ? why : kNotBaseline;
            if (!r.sof) {
                r.sof = m;
                if (len >= 8) ncomp = f[p + 7];
            }
        }
        if (sof || m == 0xDB || m == 0xC4 || m == 0xDD || m == 0xE0 || m == 0xEE || m == 0xDA) {
            // FF, the marker and the segment as they lie (the byte before a marker is FF)
            if (len + 2 > kSlot - w) {
                r.reason = kSkeletonLarge;
                r.skel_len = w;
                return;
            }
            ops.copy(skel + w, f + (p - 2), len + 2);
            w += (uint32_t)len + 2;
        }
        p += len;
        if (m == 0xDA) {
            r.ent_off = p;
            if (ncomp < 0) why = why ? why : kNotBaseline;  // SOS before SOF
            else if (len < 3 || f[p - len + 2] != ncomp) why = why ? why : kScanComponents;
            break;
        }
    }
    r.skel_len = w;
    if (r.ent_off) {
        // q from n - 2 down to the scan's start, no further than the window
        const uint64_t lo = n > kEoiWindow && n - kEoiWindow > r.ent_off ? n - kEoiWindow : r.ent_off;
        if (lo + 2 <= n) {
            const uint64_t q = ops.last_eoi(f, lo, n - 2);
            if (q != kNoEoi) r.eoi_off = q;
        }
        if (!why && r.eoi_off - r.ent_off < kMinScan) why = kSmallScan;
    }
    r.reason = why;
    r.verdict = why ? kCopyBack : kInPlace;
}

// the host's operations: one lane
struct HostOps {
    void copy(uint8_t* dst, const uint8_t* src, uint64_t n) {
        for (uint64_t i = 0; i < n; ++i) dst[i] = src[i];
    }
    uint64_t last_eoi(const uint8_t* f, uint64_t lo, uint64_t hi) {
        for (uint64_t q = hi + 1; q-- > lo;)
            if (eoi_at(f, q)) return q;
        return kNoEoi;
    }
};

}  // namespace jwalk
}  // namespace ik
