// ik_overlay.hip -- composite one overlay image (a watermark) over a window of the base
// images, in place: the project's own definition, all integers.  With M
// the base's sample maximum (255 or 65535), f an overlay colour sample and fa its alpha,
// both brought to the base's depth (8 -> 16: v * 257, 16 -> 8: (v + 128) / 257; no alpha:
// fa = M; a colour overlay on a gray base: (2126 R + 7152 G + 722 B) / 10000), opM the
// opacity at that depth, c a base colour sample and ca the base's alpha:
//
//   a = (fa * opM + M / 2) / M
//   base without alpha:  out = (f * a + c * (M - a) + M / 2) / M          (k_flatten's blend)
//   base with alpha:     t = ca * (M - a);  D = a * M + t;  out_a = (D + M / 2) / M
//                        D == 0: the pixel stays;  else out = (f * a * M + c * t + D / 2) / D
//
// Everything but the last numerator fits u32 (D <= M * M); that numerator is below 2^24 at
// 8 bits and needs u64 at 16 bits, where the division by D is the slow path.  Divisions by
// M, 257 and 10000 are by constants.
//
//   k_overlay<C, DEPTH>   C 1..4, DEPTH 1 or 2 bytes: the base's format, eight variants.
//
// The overlay's format is a wave-uniform run-time switch (it is small and stays in cache).
// A streaming kernel, no LDS.  A row of the base is cut into shares of PPL whole pixels
// that start at multiples of PPL pixels OF THE ROW (not of the window): 16 bytes, or 12
// where a pixel has 3 or 6, so a share starts dword-aligned whenever the bases, pitches
// and strides are multiples of 4 (every ik_image).  One lane owns a share.  A share that
// lies wholly inside the window is loaded and stored as 3 or 4 whole dwords; the window's
// ragged ends, shares that also hold pixels outside it, move only the window's own bytes,
// one by one, so no dword is read-modify-written by two lanes and nothing outside the
// window is written.  Nothing is read outside it either.  A workgroup takes kOverlaySpan
// columns from the first share's start, and 256 / (shares of a span) rows at once where a
// span has fewer than 256 shares; the grid's rows are capped and strided as k_flatten's.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ik_internal.h"

namespace ik {

namespace {

// n dwords at a 4-byte-aligned address (one global_load_dwordx3 / x4: global memory wants
// dword alignment only)
template <int N>
struct __attribute__((packed, aligned(4))) Dwords {
    uint32_t v[N];
};

__device__ __forceinline__ int emod(int v, int n) {
    const int r = v % n;
    return r < 0 ? r + n : r;
}

// the overlay's pixel (ox, row orow) as the base sees it: CC colour samples and the alpha
// at the base's depth
template <int CC, int DEPTH>
__device__ __forceinline__ void fetch(const OverlayArgs& a, const uint8_t* orow, int ox, uint32_t f[3], uint32_t& fa) {
    constexpr uint32_t M = DEPTH == 1 ? 255u : 65535u;
    uint32_t s[4] = {0, 0, 0, 0};
    const uint8_t* p = orow + (size_t)ox * (size_t)(a.co * a.od);
    if (a.od == 1) {
        if (a.ov_dword) {
            const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] = (v >> (8 * k)) & 0xFFu;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < a.co) s[k] = p[k];
        }
        if (DEPTH == 2) {
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] *= 257u;
        }
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < a.co) s[k] = (uint32_t)p[2 * k] | (uint32_t)p[2 * k + 1] << 8;
        if (DEPTH == 1) {
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] = (s[k] + 128u) / 257u;
        }
    }
    fa = a.co == 2 ? s[1] : a.co == 4 ? s[3] : M;
    const bool colour = a.co >= 3;
    if (CC == 3) {
        f[0] = s[0];
        f[1] = colour ? s[1] : s[0];
        f[2] = colour ? s[2] : s[0];
    } else {
        f[0] = colour ? (2126u * s[0] + 7152u * s[1] + 722u * s[2]) / 10000u : s[0];
    }
}

// one base pixel (px: its C samples, in and out) under the overlay's (f, fa)
template <int C, int DEPTH>
__device__ __forceinline__ void composite(uint32_t* px, const uint32_t* f, uint32_t fa, uint32_t opM) {
    constexpr uint32_t M = DEPTH == 1 ? 255u : 65535u;
    constexpr int CC = C <= 2 ? 1 : 3;
    const uint32_t a = (fa * opM + M / 2) / M;
    if (C == 1 || C == 3) {
#pragma unroll
        for (int c = 0; c < CC; ++c) px[c] = (f[c] * a + px[c] * (M - a) + M / 2) / M;
    } else {
        const uint32_t t = px[C - 1] * (M - a);
        const uint32_t D = a * M + t;
        if (D != 0) {
#pragma unroll
            for (int c = 0; c < CC; ++c) {
                if (DEPTH == 1) px[c] = (f[c] * a * M + px[c] * t + D / 2) / D;
                else px[c] = (uint32_t)(((uint64_t)(f[c] * a) * M + (uint64_t)px[c] * t + D / 2) / D);
            }
            px[C - 1] = (D + M / 2) / M;
        }
    }
}

template <int C, int DEPTH>
__global__ __launch_bounds__(256) void k_overlay(OverlayArgs a) {
    constexpr int PX = C * DEPTH;                                                // bytes of a pixel
    constexpr int PPL = PX == 1 ? 16 : PX == 2 ? 8 : (PX == 3 || PX == 4) ? 4 : 2;  // pixels of a share
    constexpr int LB = PPL * PX;                                                 // its bytes: 16 or 12
    constexpr int LW = LB / 4;
    constexpr int SPS = kOverlaySpan / PPL;                                      // shares of a span
    constexpr int RPB = SPS >= 256 ? 1 : 256 / SPS;                              // rows a workgroup takes at once
    constexpr int CC = C <= 2 ? 1 : 3;
    static_assert(LB % 4 == 0 && kOverlaySpan % PPL == 0, "a share is whole dwords, a span whole shares");
    const int img = blockIdx.z;
    uint8_t* base = a.tab ? reinterpret_cast<uint8_t*>(a.tab[img]) : a.base + (size_t)img * a.img_stride;
    const int wx1 = a.wx + a.ww;                                          // one past the window's last column
    const int X0 = a.wx / PPL * PPL + (int)blockIdx.x * kOverlaySpan;     // the workgroup's first column
    for (int yb = (int)blockIdx.y * RPB; yb < a.wh; yb += (int)gridDim.y * RPB) {
        for (int idx = (int)threadIdx.x; idx < SPS * RPB; idx += 256) {
            const int yy = yb + idx / SPS;
            const int xs = X0 + idx % SPS * PPL;  // the share's first column
            if (yy >= a.wh || xs >= wx1) continue;
            const bool whole = xs >= a.wx && xs + PPL <= wx1;
            const bool wide = whole && a.aligned;
            const int y = a.wy + yy;
            uint8_t* p = base + (size_t)y * a.pitch + (size_t)xs * PX;
            const uint8_t* orow = a.ov + (size_t)(a.tile ? emod(y - a.y0, a.ho) : y - a.y0) * a.ov_pitch;
            uint32_t w[LW];
            if (wide) {
                const Dwords<LW> q = *reinterpret_cast<const Dwords<LW>*>(p);
#pragma unroll
                for (int k = 0; k < LW; ++k) w[k] = q.v[k];
            } else {
#pragma unroll
                for (int k = 0; k < LW; ++k) w[k] = 0;
#pragma unroll
                for (int k = 0; k < LB; ++k) {
                    const int x = xs + k / PX;
                    if (x >= a.wx && x < wx1) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
                }
            }
            int ox = a.tile ? emod(xs - a.x0, a.wo) : xs - a.x0;
#pragma unroll
            for (int i = 0; i < PPL; ++i) {
                const int x = xs + i;
                if (x >= a.wx && x < wx1) {
                    uint32_t f[3], fa, px[C];
                    fetch<CC, DEPTH>(a, orow, ox, f, fa);
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const int k = i * C + c;  // the sample
                        px[c] = DEPTH == 1 ? (w[k >> 2] >> (8 * (k & 3))) & 0xFFu : (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
                    }
                    composite<C, DEPTH>(px, f, fa, a.opM);
#pragma unroll
                    for (int c = 0; c < C; ++c) {
                        const int k = i * C + c;
                        if (DEPTH == 1) w[k >> 2] = (w[k >> 2] & ~(0xFFu << (8 * (k & 3)))) | px[c] << (8 * (k & 3));
                        else w[k >> 1] = (w[k >> 1] & ~(0xFFFFu << (16 * (k & 1)))) | px[c] << (16 * (k & 1));
                    }
                }
                ox = ox + 1 == a.wo ? 0 : ox + 1;
            }
            if (wide) {
                Dwords<LW> q;
#pragma unroll
                for (int k = 0; k < LW; ++k) q.v[k] = w[k];
                *reinterpret_cast<Dwords<LW>*>(p) = q;
            } else {
#pragma unroll
                for (int k = 0; k < LB; ++k) {
                    const int x = xs + k / PX;
                    if (x >= a.wx && x < wx1) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
                }
            }
        }
    }
}

template <int C, int DEPTH>
hipError_t launch_variant(const OverlayArgs& a, int n, hipStream_t s) {
    constexpr int PX = C * DEPTH;
    constexpr int PPL = PX == 1 ? 16 : PX == 2 ? 8 : (PX == 3 || PX == 4) ? 4 : 2;
    constexpr int SPS = kOverlaySpan / PPL;
    constexpr int RPB = SPS >= 256 ? 1 : 256 / SPS;
    const uint32_t first = (uint32_t)(a.wx / PPL * PPL);
    const uint32_t gx = ((uint32_t)(a.wx + a.ww) - first + kOverlaySpan - 1) / kOverlaySpan;
    const uint32_t rows = ((uint32_t)a.wh + RPB - 1) / RPB;  // rows of workgroups that cover the window
    // about 8 * kOverlayRowCap workgroups in all, never more than kOverlayRowCap rows of them
    const uint64_t per_row = (uint64_t)gx * (uint64_t)n;
    const uint32_t gy = (uint32_t)std::min<uint64_t>(
        rows, std::min<uint64_t>(kOverlayRowCap, std::max<uint64_t>(1, 8ull * kOverlayRowCap / per_row)));
    hipLaunchKernelGGL((k_overlay<C, DEPTH>), dim3(gx, gy, (unsigned)n), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_overlay(const OverlayArgs& a, int C, int depth, int n, hipStream_t s) {
    if (a.ww <= 0 || a.wh <= 0 || n <= 0) return hipErrorInvalidValue;
    switch (C * 10 + depth) {
        case 11: return launch_variant<1, 1>(a, n, s);
        case 12: return launch_variant<1, 2>(a, n, s);
        case 21: return launch_variant<2, 1>(a, n, s);
        case 22: return launch_variant<2, 2>(a, n, s);
        case 31: return launch_variant<3, 1>(a, n, s);
        case 32: return launch_variant<3, 2>(a, n, s);
        case 41: return launch_variant<4, 1>(a, n, s);
        case 42: return launch_variant<4, 2>(a, n, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ik
