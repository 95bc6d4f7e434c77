// ik_exif.h -- the EXIF Orientation tag of an encoded file (host only: no HIP, no
// allocation).  What image 0.25.8 offers as ImageDecoder::orientation(): the value a
// caller hands to Orientation::from_exif / DynamicImage::apply_orientation.
//
//   JPEG  the segments before the first SOS; the first APP1 whose payload starts "Exif\0\0"
//   PNG   the chunk list by its length fields (no CRC check); the first eXIf before IEND
//   WebP  inside a VP8X RIFF, the first EXIF chunk (odd sizes padded to even)
//
// The payload is a TIFF header (II / MM, 42, IFD0 offset), with or without an "Exif\0\0"
// prefix in any of the three containers.  IFD0 alone is scanned for tag 0x0112 of type
// SHORT and count 1; no other IFD is followed.  A missing tag, a value outside 1..8,
// another type or count, and any malformed or truncated file give 1: never an error,
// and never a read at or past bytes + len.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

namespace ik {
namespace exif {

inline uint32_t be16(const uint8_t* p) { return (uint32_t)p[0] << 8 | p[1]; }
inline uint32_t be32(const uint8_t* p) { return (uint32_t)p[0] << 24 | (uint32_t)p[1] << 16 | (uint32_t)p[2] << 8 | p[3]; }
inline uint32_t le32(const uint8_t* p) { return (uint32_t)p[3] << 24 | (uint32_t)p[2] << 16 | (uint32_t)p[1] << 8 | p[0]; }

// the Orientation of a TIFF payload of n bytes (1 when there is none)
inline int tiff_orientation(const uint8_t* p, size_t n) {
    if (n >= 6 && !std::memcmp(p, "Exif\0\0", 6)) { p += 6; n -= 6; }
    if (n < 8) return 1;
    bool le;
    if (p[0] == 'I' && p[1] == 'I') le = true;
    else if (p[0] == 'M' && p[1] == 'M') le = false;
    else return 1;
    auto r16 = [&](size_t o) { return le ? (uint32_t)p[o] | (uint32_t)p[o + 1] << 8 : be16(p + o); };
    auto r32 = [&](size_t o) { return le ? le32(p + o) : be32(p + o); };
    if (r16(2) != 42) return 1;
    const size_t ifd = r32(4);
    if (ifd > n || n - ifd < 2) return 1;
    const size_t count = r16(ifd);
    if ((n - ifd - 2) / 12 < count) return 1;  // the entry count points past the payload
    for (size_t e = 0; e < count; ++e) {
        const size_t o = ifd + 2 + 12 * e;
        if (r16(o) != 0x0112) continue;
        if (r16(o + 2) != 3 || r32(o + 4) != 1) return 1;  // not one SHORT
        const uint32_t v = r16(o + 8);
        return v >= 1 && v <= 8 ? (int)v : 1;
    }
    return 1;
}

inline int jpeg_orientation(const uint8_t* b, size_t n) {
    size_t p = 2;  // after SOI
    while (p + 4 <= n) {
        if (b[p] != 0xFF) return 1;
        const uint8_t m = b[p + 1];
        if (m == 0xFF) { ++p; continue; }  // fill byte
        if (m == 0xDA || m == 0xD9) return 1;  // SOS / EOI: no EXIF before the scan
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) { p += 2; continue; }  // no length
        const size_t len = be16(b + p + 2);
        if (len < 2 || len > n - (p + 2)) return 1;
        if (m == 0xE1 && len >= 8 && !std::memcmp(b + p + 4, "Exif\0\0", 6))
            return tiff_orientation(b + p + 4, len - 2);
        p += 2 + len;
    }
    return 1;
}

inline int png_orientation(const uint8_t* b, size_t n) {
    size_t p = 8;  // after the signature
    while (p + 8 <= n) {
        const size_t len = be32(b + p);
        const uint8_t* type = b + p + 4;
        if (!std::memcmp(type, "IEND", 4)) return 1;
        if (len > n - (p + 8)) return 1;
        if (!std::memcmp(type, "eXIf", 4)) return tiff_orientation(b + p + 8, len);
        if (n - (p + 8) - len < 4) return 1;  // the CRC is cut off
        p += 8 + len + 4;
    }
    return 1;
}

inline int webp_orientation(const uint8_t* b, size_t n) {
    if (n < 20 || std::memcmp(b + 12, "VP8X", 4)) return 1;
    // chunks end with the RIFF size or the file, whichever comes first
    const size_t riff_end = (size_t)le32(b + 4) + 8;
    if (riff_end < n) n = riff_end;
    size_t p = 12;
    while (p + 8 <= n) {
        const size_t len = le32(b + p + 4);
        if (len > n - (p + 8)) return 1;
        if (!std::memcmp(b + p, "EXIF", 4)) return tiff_orientation(b + p + 8, len);
        const size_t padded = len + (len & 1);
        if (padded > n - (p + 8)) return 1;
        p += 8 + padded;
    }
    return 1;
}

}  // namespace exif

// 1..8; 1 when the file carries no readable Orientation
inline int exif_orientation(const uint8_t* b, size_t n) {
    if (!b) return 1;
    if (n >= 3 && b[0] == 0xFF && b[1] == 0xD8 && b[2] == 0xFF) return exif::jpeg_orientation(b, n);
    if (n >= 8 && !std::memcmp(b, "\x89PNG\r\n\x1a\n", 8)) return exif::png_orientation(b, n);
    if (n >= 12 && !std::memcmp(b, "RIFF", 4) && !std::memcmp(b + 8, "WEBP", 4)) return exif::webp_orientation(b, n);
    return 1;
}

}  // namespace ik
