// ik_pad.hip -- extend an image onto a canvas: the project's own definition (DESIGN section
// 4).  The W x H image lies at (x0, y0) of a cw x ch canvas, and canvas pixel (x, y) takes
//
//   I[fy(y - y0), fx(x - x0)]      f by mode, n the axis length, i the signed index:
//     edge    clamp(i, 0, n - 1)
//     wrap    i mod n, Euclidean
//     mirror  j = i mod 2n;  j < n ? j : 2n - 1 - j     (the edge sample repeats)
//     colour  inside the image its pixel, outside the frame pixel (a constant)
//
// Channels and depth never change and nothing is blended, so the kernel moves BYTES: a
// pixel is PX = C * depth bytes (1, 2, 3, 4, 6 or 8) and k_pad<PX, MODE> knows no more of
// the format.
//
// Output-driven, streaming, no LDS.  A canvas row is cut into SHARES of 16 bytes at
// multiples of 16 from the row's start; one lane owns one share.  A workgroup takes one
// canvas row of kPadSpan pixels (kPadSpan * PX bytes, a multiple of 16), its rows are
// grid-strided beyond kPadRowCap, and the row map fy is computed once per workgroup and row
// on the scalar unit, never per sample.  A share is one of three kinds:
//   interior  wholly inside the image's columns (and, colour mode, rows): 16 contiguous
//             source bytes at an ARBITRARY byte address, x0 * PX against the row start.
//             Loaded as the 4 dwords at that address rounded down to a dword, plus the
//             fifth only when the address is not a dword's (each of them holds a byte of
//             the run, so nothing is read that does not share a dword with image bytes),
//             and shifted into place by v_alignbyte_b32: no byte gather.
//   frame     colour mode, wholly outside: the frame pixel's bytes at the share's phase,
//             16 % PX apart from share to share, so three host-made patterns; reads nothing.
//   mixed     everything else (a share the image's edge crosses, every frame share of the
//             other modes, a row's ragged last share): byte by byte through the index map,
//             which costs one modulo per share and is stepped from there.
// Stores: a whole share is one 16-byte store at a dword-aligned address; a row's ragged
// last share stores its whole dwords and then its last 1..3 bytes singly.  Nothing past
// cw * PX bytes of a canvas row is written, and no source byte past W * PX of a row reaches
// an output.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ik_internal.h"

namespace ik {

namespace {

// Pixels are in global memory.  A base read from the table is an integer, and one chosen at
// run time between the table and base + stride loses its address space; with the space
// stated the loads and stores are global_* instructions, not flat_* ones.  Four dwords at
// consecutive 4-byte-aligned addresses become one global_load / global_store_dwordx4 (global
// memory wants dword alignment only).
typedef const __attribute__((address_space(1))) uint8_t* GSrc;
typedef __attribute__((address_space(1))) uint8_t* GDst;
typedef const __attribute__((address_space(1))) uint32_t* GSrc4;
typedef __attribute__((address_space(1))) uint32_t* GDst4;

// the source index of signed index i on an axis of n samples (edge, wrap and mirror)
template <int MODE>
__device__ __forceinline__ uint32_t pad_map(int32_t i, uint32_t n) {
    if (MODE == IK_PAD_EDGE) return (uint32_t)min(max(i, 0), (int32_t)n - 1);
    const int32_t p = MODE == IK_PAD_MIRROR ? 2 * (int32_t)n : (int32_t)n;  // n <= 2^24
    int32_t j = i % p;
    if (j < 0) j += p;
    if (MODE == IK_PAD_MIRROR && j >= (int32_t)n) j = p - 1 - j;
    return (uint32_t)j;
}

template <int PX, int MODE>
__global__ __launch_bounds__(256) void k_pad(PadArgs a) {
    constexpr uint32_t SPANB = (uint32_t)kPadSpan * PX;  // bytes of a canvas row one workgroup takes
    static_assert(SPANB % 16 == 0, "a span holds whole shares");
    const int img = blockIdx.z;
    GSrc src = (GSrc)(a.src_tab ? (uintptr_t)a.src_tab[img] : (uintptr_t)(a.src + img * a.src_img_stride));
    GDst dst = (GDst)(a.dst_tab ? (uintptr_t)a.dst_tab[img] : (uintptr_t)(a.dst + img * a.dst_img_stride));
    const uint32_t CB = a.cw * PX;                    // bytes of a canvas row (cw <= 2^24)
    const uint32_t ib0 = (uint32_t)a.x0 * PX;         // the image's bytes in it: [ib0, ib1)
    const uint32_t ib1 = ib0 + a.W * PX;
    const uint32_t B0 = blockIdx.x * SPANB;           // the span's first byte
    const uint32_t B1 = min(CB, B0 + SPANB);
    for (uint32_t y = blockIdx.y; y < a.ch; y += gridDim.y) {
        // the row map, once per workgroup and row (uniform: scalar registers)
        const int32_t iy = (int32_t)y - a.y0;
        bool in_y = true;
        uint32_t sy;
        if (MODE == IK_PAD_COLOR) {
            in_y = (uint32_t)iy < a.H;
            sy = in_y ? (uint32_t)iy : 0u;
        } else {
            sy = pad_map<MODE>(iy, a.H);
        }
        GSrc srow = src + (size_t)sy * a.src_pitch;
        GDst drow = dst + (size_t)y * a.dst_pitch;
        for (uint32_t b = B0 + threadIdx.x * 16u; b < B1; b += blockDim.x * 16u) {
            const uint32_t nb = min(16u, CB - b);  // 16: a whole share
            uint32_t o[4] = {0, 0, 0, 0};
            if (in_y && b >= ib0 && b + 16u <= ib1) {
                // interior: 16 source bytes at any byte address
                GSrc sp = srow + (b - ib0);
                const uint32_t sh = (uint32_t)(uintptr_t)sp & 3u;
                GSrc ap = sp - sh;
                GSrc4 aw = (GSrc4)ap;
                uint32_t q[5] = {aw[0], aw[1], aw[2], aw[3], 0};
                if (sh) q[4] = aw[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = __builtin_amdgcn_alignbyte(q[k + 1], q[k], sh);
            } else if (MODE == IK_PAD_COLOR && (!in_y || b + 16u <= ib0 || b >= ib1)) {
                // frame: the pattern of this share's phase, (b / 16) % 3 (all three are
                // equal when PX divides 16)
                const uint32_t m = 16 % PX ? (b >> 4) % 3u : 0u;
#pragma unroll
                for (int k = 0; k < 4; ++k) o[k] = m == 0 ? a.pat[0][k] : m == 1 ? a.pat[1][k] : a.pat[2][k];
            } else {
                // mixed: byte by byte; the pixel and the byte in it are stepped from the
                // share's first, the index map from one modulo
                const uint32_t x = b / PX;
                uint32_t j = b - x * PX;
                int32_t i = (int32_t)x - a.x0;
                uint32_t t = 0;  // wrap: the source column; mirror: the index mod 2W
                if (MODE == IK_PAD_WRAP) t = pad_map<IK_PAD_WRAP>(i, a.W);
                if (MODE == IK_PAD_MIRROR) {
                    int32_t r = i % (2 * (int32_t)a.W);
                    t = (uint32_t)(r < 0 ? r + 2 * (int32_t)a.W : r);
                }
                const uint64_t fp = (uint64_t)a.fpx[0] | ((uint64_t)a.fpx[1] << 32);
#pragma unroll
                for (int k = 0; k < 16; ++k) {
                    if ((uint32_t)k < nb) {
                        uint32_t v;
                        if (MODE == IK_PAD_COLOR) {
                            v = (uint32_t)(fp >> (8 * j)) & 0xFFu;
                            if ((uint32_t)i < a.W) v = srow[(size_t)(uint32_t)i * PX + j];  // (in_y holds here)
                        } else {
                            const uint32_t sx = MODE == IK_PAD_EDGE ? pad_map<IK_PAD_EDGE>(i, a.W)
                                                : MODE == IK_PAD_WRAP ? t
                                                                      : (t < a.W ? t : 2 * a.W - 1 - t);
                            v = srow[(size_t)sx * PX + j];
                        }
                        o[k >> 2] |= v << (8 * (k & 3));
                    }
                    if (++j == PX) {
                        j = 0;
                        ++i;
                        if (MODE == IK_PAD_WRAP && ++t == a.W) t = 0;
                        if (MODE == IK_PAD_MIRROR && ++t == 2 * a.W) t = 0;
                    }
                }
            }
            GDst dp = drow + b;
            if (nb == 16u) {
#pragma unroll
                for (int k = 0; k < 4; ++k) ((GDst4)dp)[k] = o[k];
            } else {
                // the row's ragged end: its whole dwords, then its last bytes singly
#pragma unroll
                for (int k = 0; k < 3; ++k)
                    if ((uint32_t)(4 * k + 4) <= nb) ((GDst4)dp)[k] = o[k];
#pragma unroll
                for (int k = 0; k < 15; ++k)
                    if ((uint32_t)k >= (nb & ~3u) && (uint32_t)k < nb) dp[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

template <int PX, int MODE>
hipError_t launch_variant(const PadArgs& a, int n, hipStream_t s) {
    constexpr int SHARES = kPadSpan * PX / 16;  // shares of a full span: 64 * PX
    // a workgroup of whole waves that a full span fills in whole passes
    constexpr int THREADS = SHARES <= 256 ? SHARES : SHARES % 256 == 0 ? 256 : 192;
    static_assert(THREADS % 64 == 0 && SHARES % THREADS == 0, "whole waves, whole passes");
    const uint32_t gx = (a.cw + kPadSpan - 1) / kPadSpan;
    // about 8 * kPadRowCap workgroups in all, never more than kPadRowCap rows of them
    const uint64_t per_row = (uint64_t)gx * (uint64_t)n;
    const uint32_t gy = (uint32_t)std::min<uint64_t>(
        a.ch, std::min<uint64_t>(kPadRowCap, std::max<uint64_t>(1, 8ull * kPadRowCap / per_row)));
    hipLaunchKernelGGL((k_pad<PX, MODE>), dim3(gx, gy, (unsigned)n), dim3(THREADS), 0, s, a);
    return hipGetLastError();
}

template <int MODE>
hipError_t launch_mode(const PadArgs& a, int px, int n, hipStream_t s) {
    switch (px) {
        case 1: return launch_variant<1, MODE>(a, n, s);
        case 2: return launch_variant<2, MODE>(a, n, s);
        case 3: return launch_variant<3, MODE>(a, n, s);
        case 4: return launch_variant<4, MODE>(a, n, s);
        case 6: return launch_variant<6, MODE>(a, n, s);
        case 8: return launch_variant<8, MODE>(a, n, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_pad(const PadArgs& a, int px, int mode, int n, hipStream_t s) {
    switch (mode) {
        case IK_PAD_COLOR: return launch_mode<IK_PAD_COLOR>(a, px, n, s);
        case IK_PAD_EDGE: return launch_mode<IK_PAD_EDGE>(a, px, n, s);
        case IK_PAD_MIRROR: return launch_mode<IK_PAD_MIRROR>(a, px, n, s);
        case IK_PAD_WRAP: return launch_mode<IK_PAD_WRAP>(a, px, n, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ik
