// ik_adjust.hip -- apply a colour adjustment's plan to images in place: the project's own
// definition, all integers on the device.  The host (ik_adjust_plan.h)
// has turned the request into a Q16 colour matrix q and a tone table T.  With M the sample
// maximum (255 or 65535), for a pixel of three or four channels
//
//   o_i = clamp((q[i][0] R + q[i][1] G + q[i][2] B + 32768) >> 16, 0, M)   (arithmetic shift)
//
// then every colour sample v becomes T[v].  Alpha is not touched; a gray pixel (one or two
// channels) skips the matrix, whose rows sum to 65536.  The sums fit i32 at 8 bits (a row's
// sum of |q| stays below 4.6 * 65536) and need i64 at 16 bits, the slow path.
//
//   k_adjust<C, DEPTH, MATRIX, TABLE>   C 1..4, DEPTH 1 or 2 bytes, MATRIX only where C >= 3
//
// A streaming kernel.  A row is cut into shares of PPL whole pixels that start at multiples
// of PPL pixels of the row: 16 bytes, or 12 where a pixel has 3 or 6, so a share starts
// dword-aligned whenever the bases, pitches and strides are multiples of 4 (every
// ik_image).  One lane owns a share.  A whole share is loaded and stored as 3 or 4 whole
// dwords; a row's ragged last share, and every share of an unaligned area, moves its own
// bytes one by one, and there the alpha bytes are not stored at all.  Nothing past
// W * C * DEPTH bytes of a row is read or written.  A workgroup takes kAdjustSpan pixels
// of a row, and 256 / (shares of a span) rows at once where a span has fewer than 256
// shares; the grid's rows are capped and strided as k_flatten's.
//
// The 8-bit table is 256 bytes, staged in LDS once per workgroup and read a byte at a time
// at an address the data chooses (equal dwords broadcast, different dwords of one bank
// serialise).  The 16-bit table, 128 KiB, is gathered from global memory, where it stays in
// L2: the slow path.
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

template <int C, int DEPTH, bool MATRIX, bool TABLE>
__global__ __launch_bounds__(256) void k_adjust(AdjustArgs a) {
    constexpr int PX = C * DEPTH;                                                // bytes of a pixel
    constexpr int PPL = PX == 1 ? 16 : PX == 2 ? 8 : (PX == 3 || PX == 4) ? 4 : 2;  // pixels of a share
    constexpr int LB = PPL * PX;                                                 // its bytes: 16 or 12
    constexpr int LW = LB / 4;
    constexpr int SPS = kAdjustSpan / PPL;                                       // shares of a span
    constexpr int RPB = SPS >= 256 ? 1 : 256 / SPS;                              // rows a workgroup takes at once
    constexpr int CC = C <= 2 ? 1 : 3;                                           // colour samples of a pixel
    constexpr int32_t M = DEPTH == 1 ? 255 : 65535;
    static_assert(LB % 4 == 0 && kAdjustSpan % PPL == 0, "a share is whole dwords, a span whole shares");
    static_assert(!MATRIX || C >= 3, "the matrix needs three colour samples");
    static_assert(MATRIX || TABLE, "nothing to do");
    __shared__ uint32_t lut_w[TABLE && DEPTH == 1 ? 64 : 1];
    if (TABLE && DEPTH == 1) {
        if (threadIdx.x < 64) lut_w[threadIdx.x] = static_cast<const uint32_t*>(a.tone)[threadIdx.x];
        __syncthreads();
    }
    const uint8_t* lut8 = reinterpret_cast<const uint8_t*>(lut_w);
    const uint16_t* lut16 = static_cast<const uint16_t*>(a.tone);
    const int img = blockIdx.z;
    uint8_t* base = a.tab ? reinterpret_cast<uint8_t*>(a.tab[img]) : a.base + (size_t)img * a.img_stride;
    const int W = (int)a.W, H = (int)a.H;
    const int X0 = (int)blockIdx.x * kAdjustSpan;  // the workgroup's first pixel
    for (int yb = (int)blockIdx.y * RPB; yb < H; yb += (int)gridDim.y * RPB) {
        for (int idx = (int)threadIdx.x; idx < SPS * RPB; idx += 256) {
            const int y = yb + idx / SPS;
            const int xs = X0 + idx % SPS * PPL;  // the share's first pixel
            if (y >= H || xs >= W) continue;
            const int cnt = min(PPL, W - xs);     // PPL: a whole share
            const bool wide = cnt == PPL && a.aligned;
            uint8_t* p = base + (size_t)y * a.pitch + (size_t)xs * PX;
            uint32_t w[LW];
            if (wide) {
                const Dwords<LW> d = *reinterpret_cast<const Dwords<LW>*>(p);
#pragma unroll
                for (int k = 0; k < LW; ++k) w[k] = d.v[k];
            } else {
#pragma unroll
                for (int k = 0; k < LW; ++k) w[k] = 0;
#pragma unroll
                for (int k = 0; k < LB; ++k)
                    if (k < cnt * PX) w[k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
            }
            // (a ragged share's missing pixels are zeros: computed, never stored)
#pragma unroll
            for (int i = 0; i < PPL; ++i) {
                int32_t px[CC];
#pragma unroll
                for (int c = 0; c < CC; ++c) {
                    const int k = i * C + c;  // the sample
                    px[c] = (int32_t)(DEPTH == 1 ? (w[k >> 2] >> (8 * (k & 3))) & 0xFFu : (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu);
                }
                if constexpr (MATRIX) {
                    int32_t o[3];
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        int32_t v;
                        if (DEPTH == 1) {
                            v = (a.q[3 * r] * px[0] + a.q[3 * r + 1] * px[1] + a.q[3 * r + 2] * px[2] + 32768) >> 16;
                        } else {
                            const int64_t t = (int64_t)a.q[3 * r] * px[0] + (int64_t)a.q[3 * r + 1] * px[1] +
                                              (int64_t)a.q[3 * r + 2] * px[2] + 32768;
                            v = (int32_t)(t >> 16);
                        }
                        o[r] = min(max(v, 0), M);
                    }
#pragma unroll
                    for (int r = 0; r < 3; ++r) px[r] = o[r];
                }
                if (TABLE) {
#pragma unroll
                    for (int c = 0; c < CC; ++c) px[c] = DEPTH == 1 ? (int32_t)lut8[px[c]] : (int32_t)lut16[px[c]];
                }
#pragma unroll
                for (int c = 0; c < CC; ++c) {
                    const int k = i * C + c;
                    const uint32_t v = (uint32_t)px[c];
                    if (DEPTH == 1) w[k >> 2] = (w[k >> 2] & ~(0xFFu << (8 * (k & 3)))) | v << (8 * (k & 3));
                    else w[k >> 1] = (w[k >> 1] & ~(0xFFFFu << (16 * (k & 1)))) | v << (16 * (k & 1));
                }
            }
            if (wide) {
                Dwords<LW> d;
#pragma unroll
                for (int k = 0; k < LW; ++k) d.v[k] = w[k];
                *reinterpret_cast<Dwords<LW>*>(p) = d;
            } else {
#pragma unroll
                for (int k = 0; k < LB; ++k) {
                    const bool alpha = (C == 2 || C == 4) && k / DEPTH % C == C - 1;
                    if (!alpha && k < cnt * PX) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
                }
            }
        }
    }
}

template <int C, int DEPTH, bool MATRIX, bool TABLE>
hipError_t launch_variant(const AdjustArgs& a, int n, hipStream_t s) {
    constexpr int PX = C * DEPTH;
    constexpr int PPL = PX == 1 ? 16 : PX == 2 ? 8 : (PX == 3 || PX == 4) ? 4 : 2;
    constexpr int SPS = kAdjustSpan / PPL;
    constexpr int RPB = SPS >= 256 ? 1 : 256 / SPS;
    const uint32_t gx = (a.W + kAdjustSpan - 1) / kAdjustSpan;
    const uint32_t rows = (a.H + RPB - 1) / RPB;  // rows of workgroups that cover the image
    // about 8 * kAdjustRowCap workgroups in all, never more than kAdjustRowCap rows of them
    const uint64_t per_row = (uint64_t)gx * (uint64_t)n;
    const uint32_t gy = (uint32_t)std::min<uint64_t>(
        rows, std::min<uint64_t>(kAdjustRowCap, std::max<uint64_t>(1, 8ull * kAdjustRowCap / per_row)));
    hipLaunchKernelGGL((k_adjust<C, DEPTH, MATRIX, TABLE>), dim3(gx, gy, (unsigned)n), dim3(256), 0, s, a);
    return hipGetLastError();
}

template <int C, int DEPTH>
hipError_t launch_colour(const AdjustArgs& a, bool matrix, int n, hipStream_t s) {
    if (matrix && a.tone) return launch_variant<C, DEPTH, true, true>(a, n, s);
    if (matrix) return launch_variant<C, DEPTH, true, false>(a, n, s);
    return launch_variant<C, DEPTH, false, true>(a, n, s);
}

}  // namespace

hipError_t launch_adjust(const AdjustArgs& a, int C, int depth, bool matrix, int n, hipStream_t s) {
    if (!a.W || !a.H || n <= 0 || (uint32_t)n > kAdjustMaxImages || a.W > kAdjustMaxDim || a.H > kAdjustMaxDim)
        return hipErrorInvalidValue;
    if (C <= 2) matrix = false;
    if (!matrix && !a.tone) return hipErrorInvalidValue;
    switch (C * 10 + depth) {
        case 11: return launch_variant<1, 1, false, true>(a, n, s);
        case 12: return launch_variant<1, 2, false, true>(a, n, s);
        case 21: return launch_variant<2, 1, false, true>(a, n, s);
        case 22: return launch_variant<2, 2, false, true>(a, n, s);
        case 31: return launch_colour<3, 1>(a, matrix, n, s);
        case 32: return launch_colour<3, 2>(a, matrix, n, s);
        case 41: return launch_colour<4, 1>(a, matrix, n, s);
        case 42: return launch_colour<4, 2>(a, matrix, n, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ik
