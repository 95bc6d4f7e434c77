// ik_flatten.hip -- composite an image's alpha onto a constant background colour: the
// project's own definition (the image crate has no such call).  With M
// the sample maximum (255, or 65535 at 16 bits where a background channel is b8 * 257),
// c a sample, a its pixel's alpha and b the background channel,
//
//   out = (c * a + b * (M - a) + M / 2) / M      (u32, floor division)
//
// the integer nearest to the exact quotient (M is odd: no ties); a = 0 gives b, a = M
// gives c, and the numerator is at most M * M + M / 2 < 2^32.  The division is by a
// constant, which the compiler turns into an exact multiply-high and shift.
//
//   k_flatten<4, 3, D>  Rgba  -> Rgb
//   k_flatten<2, 1, D>  LumaA -> Luma   (gray background)
//   k_flatten<2, 3, D>  LumaA -> Rgb    (luma replicated, as to_rgb8 replicates it)
//
// A streaming kernel, no LDS: a workgroup takes kFlattenSpan pixels of a row, a lane whole
// pixels worth 16 source bytes (4 RGBA8, 2 RGBA16, 8 LA8, 4 LA16) which it loads at once
// and stores as 2, 3 or 6 whole dwords; consecutive lanes take consecutive pieces.  A
// piece starts at a multiple of kFlattenSpan pixels and a lane's share at a multiple of
// its pixel count, so both sides are dword-aligned whenever the bases, pitches and strides
// are multiples of 4 (every ik_image); a side that is not moves bytes.  What a row's last,
// partial share holds is moved pixel by pixel: nothing is read past W * CIN * D bytes of a
// source row or written past W * COUT * D bytes of a destination row.  The grid is capped
// (at most kFlattenRowCap rows of workgroups, about 2048 workgroups in all) and rows are
// grid-strided.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ik_internal.h"

namespace ik {

namespace {

struct FlattenArgs {
    const uint8_t* src;
    size_t src_pitch, src_img_stride;
    uint8_t* dst;
    size_t dst_pitch, dst_img_stride;
    const uint64_t* src_tab;  // per-image bases (device), or null: src + img * src_img_stride
    const uint64_t* dst_tab;
    uint32_t W, H;
    uint32_t bg[3];                // the background per channel, at the image's depth
    int src_aligned, dst_aligned;  // bases, pitches and strides are multiples of 4
};

// four dwords at a 4-byte-aligned address (one global_load_dwordx4: global memory wants
// dword alignment only)
struct __attribute__((packed, aligned(4))) Dwords4 {
    uint32_t v[4];
};

template <int DEPTH>
__device__ __forceinline__ uint32_t blend(uint32_t c, uint32_t a, uint32_t b) {
    constexpr uint32_t M = DEPTH == 1 ? 255u : 65535u;
    return (c * a + b * (M - a) + M / 2) / M;
}

template <int CIN, int COUT, int DEPTH>
__global__ __launch_bounds__(256) void k_flatten(FlattenArgs a) {
    constexpr int PPL = 16 / (CIN * DEPTH);     // pixels of a lane's 16 source bytes
    constexpr int SPX = CIN * DEPTH;            // bytes of a source pixel
    constexpr int DPX = COUT * DEPTH;           // bytes of a destination pixel
    constexpr int OW = PPL * DPX / 4;           // dwords a lane stores
    constexpr int NS = 16 / DEPTH;              // samples in the 16 bytes
    static_assert(PPL * DPX % 4 == 0, "a lane stores whole dwords");
    const int img = blockIdx.z;
    const uint8_t* src = a.src_tab ? reinterpret_cast<const uint8_t*>(a.src_tab[img]) : a.src + img * a.src_img_stride;
    uint8_t* dst = a.dst_tab ? reinterpret_cast<uint8_t*>(a.dst_tab[img]) : a.dst + img * a.dst_img_stride;
    const uint32_t X0 = blockIdx.x * (uint32_t)kFlattenSpan;               // first pixel of the piece
    const int npx = (int)min((uint32_t)kFlattenSpan, a.W - X0);            // its pixels
    for (uint32_t y = blockIdx.y; y < a.H; y += gridDim.y) {
        const uint8_t* srow = src + (size_t)y * a.src_pitch + (size_t)X0 * SPX;
        uint8_t* drow = dst + (size_t)y * a.dst_pitch + (size_t)X0 * DPX;
        for (int p = (int)threadIdx.x * PPL; p < npx; p += 256 * PPL) {
            const int cnt = min(PPL, npx - p);  // PPL: a whole share
            const uint8_t* sp = srow + (size_t)p * SPX;
            uint8_t* dp = drow + (size_t)p * DPX;
            uint32_t w[4] = {0, 0, 0, 0};
            if (cnt == PPL && a.src_aligned) {
                const Dwords4 q = *reinterpret_cast<const Dwords4*>(sp);
#pragma unroll
                for (int k = 0; k < 4; ++k) w[k] = q.v[k];
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (k < cnt * SPX) w[k >> 2] |= (uint32_t)sp[k] << (8 * (k & 3));
            }
            uint32_t s[NS];  // the samples (native-endian u16 at 16 bits)
#pragma unroll
            for (int k = 0; k < NS; ++k)
                s[k] = DEPTH == 1 ? (w[k >> 2] >> (8 * (k & 3))) & 0xFFu : (w[k >> 1] >> (16 * (k & 1))) & 0xFFFFu;
            uint32_t o[OW];
#pragma unroll
            for (int k = 0; k < OW; ++k) o[k] = 0;
#pragma unroll
            for (int x = 0; x < PPL; ++x) {
                const uint32_t al = s[x * CIN + CIN - 1];
#pragma unroll
                for (int c = 0; c < COUT; ++c) {
                    const uint32_t v = blend<DEPTH>(s[x * CIN + (CIN == 4 ? c : 0)], al, a.bg[c]);
                    const int k = x * COUT + c;  // destination sample
                    if (DEPTH == 1) o[k >> 2] |= v << (8 * (k & 3));
                    else o[k >> 1] |= v << (16 * (k & 1));
                }
            }
            if (cnt == PPL && a.dst_aligned) {
#pragma unroll
                for (int k = 0; k < OW; ++k) reinterpret_cast<uint32_t*>(dp)[k] = o[k];
            } else {
#pragma unroll
                for (int k = 0; k < OW * 4; ++k)
                    if (k < cnt * DPX) dp[k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
            }
        }
    }
}

template <int CIN, int COUT, int DEPTH>
hipError_t launch_variant(const FlattenArgs& a, int n, hipStream_t s) {
    const uint32_t gx = (a.W + kFlattenSpan - 1) / kFlattenSpan;
    // about 8 * kFlattenRowCap workgroups in all, never more than kFlattenRowCap rows of them
    const uint64_t per_row = (uint64_t)gx * (uint64_t)n;
    const uint32_t gy = (uint32_t)std::min<uint64_t>(
        a.H, std::min<uint64_t>(kFlattenRowCap, std::max<uint64_t>(1, 8ull * kFlattenRowCap / per_row)));
    hipLaunchKernelGGL((k_flatten<CIN, COUT, DEPTH>), dim3(gx, gy, (unsigned)n), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_flatten(const uint8_t* src, size_t src_pitch, size_t src_img_stride, uint8_t* dst, size_t dst_pitch,
                          size_t dst_img_stride, uint32_t W, uint32_t H, int cin, int cout, int depth, uint32_t rgb,
                          int n, hipStream_t s, const uint64_t* src_tab, const uint64_t* dst_tab) {
    FlattenArgs a{};
    a.src = src; a.src_pitch = src_pitch; a.src_img_stride = src_img_stride;
    a.dst = dst; a.dst_pitch = dst_pitch; a.dst_img_stride = dst_img_stride;
    a.src_tab = src_tab; a.dst_tab = dst_tab;
    a.W = W; a.H = H;
    for (int c = 0; c < 3; ++c) {
        const uint32_t b8 = (rgb >> (16 - 8 * c)) & 0xFFu;
        a.bg[c] = depth == 1 ? b8 : b8 * 257u;
    }
    // (images named by a table are ik_images: pooled hipMalloc blocks, 256-byte pitches)
    a.src_aligned = src_tab ? (src_pitch & 3) == 0
                            : (((uintptr_t)src | src_pitch | (n > 1 ? src_img_stride : 0)) & 3) == 0;
    a.dst_aligned = dst_tab ? (dst_pitch & 3) == 0
                            : (((uintptr_t)dst | dst_pitch | (n > 1 ? dst_img_stride : 0)) & 3) == 0;
    const int key = cin * 100 + cout * 10 + depth;
    switch (key) {
        case 431: return launch_variant<4, 3, 1>(a, n, s);
        case 432: return launch_variant<4, 3, 2>(a, n, s);
        case 211: return launch_variant<2, 1, 1>(a, n, s);
        case 212: return launch_variant<2, 1, 2>(a, n, s);
        case 231: return launch_variant<2, 3, 1>(a, n, s);
        case 232: return launch_variant<2, 3, 2>(a, n, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ik
