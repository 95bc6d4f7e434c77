// ik_orient.hip -- DynamicImage::apply_orientation on the device: the eight EXIF
// orientations as exact permutations of pixels of 1, 2, 3, 4, 6 or 8 bytes.
//
//   out[y][x] = S[sy][sx]          flip_x  flip_y  transposed
//   2  S[y][W-1-x]                   x
//   3  S[H-1-y][W-1-x]               x       x
//   4  S[H-1-y][x]                           x
//   5  S[x][y]                                        x
//   6  S[H-1-x][y]                           x        x
//   7  S[H-1-x][W-1-y]               x       x        x
//   8  S[x][W-1-y]                   x                x
// (flip_x / flip_y: the source column / row index runs backwards.)
//
// Both kernels move bytes HBM -> LDS -> HBM, reading along source rows and writing along
// destination rows, in dwords wherever the caller's bases and pitches are 4-byte aligned
// (every ik_image is) and in bytes otherwise.  A workgroup's piece starts at a multiple of
// 64 pixels on both sides, so its first byte is dword-aligned for every pixel size; what a
// partial piece leaves over at the right or bottom edge is moved byte by byte: nothing is
// read past W * px bytes of a source row or written past out_w * px of a destination row.
//
// k_orient_rows (2, 3, 4): a wave takes kOrientStrip pixels of one row; the pixel order
// is reversed on the way out of LDS.
// k_orient_transpose (5..8): a workgroup takes a tile of kOrientTile x kOrientTile pixels,
// LDS row j = the source row that becomes destination column DX0 + j.  A destination dword
// is gathered from LDS in granules of gcd(px, 4) bytes: consecutive lanes read consecutive
// LDS rows, so the row pitch is padded by one dword (two for 8-byte pixels, whose lanes
// advance a row every second dword).  By the bank rule of ds_read (bank = dword mod 32
// within a 32-lane half) that leaves 4- and 8-byte pixels conflict-free and the 1-, 2-, 3-
// and 6-byte ones 2-way (a half's 128 output bytes span more than 32 LDS rows there);
// without the padding every lane of a half meets one bank (16- to 32-way).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ik_internal.h"

namespace ik {

namespace {

constexpr int kT = kOrientTile;
constexpr int kStrip = kOrientStrip;

struct OrientArgs {
    const uint8_t* src;
    size_t src_pitch, src_img_stride;
    uint8_t* dst;
    size_t dst_pitch, dst_img_stride;
    const uint64_t* src_tab;  // per-image bases (device), or null: src + img * src_img_stride
    const uint64_t* dst_tab;
    uint32_t W, H;            // the source image
    int flip_x, flip_y;
    int src_aligned, dst_aligned;  // bases, pitches and strides are multiples of 4
};

template <int PX>
struct Px {
    static constexpr int G = PX % 4 == 0 ? 4 : (PX % 2 == 0 ? 2 : 1);  // gather granule, bytes
    static constexpr int LP = kT * PX + (PX == 8 ? 8 : 4);             // padded LDS row pitch of a tile
};

// bytes [off, off + 4) of a destination row piece, gathered from an LDS image in which
// destination pixel x lies at base + x * step (step may be negative)
template <int PX>
__device__ __forceinline__ uint32_t gather_dword(const uint8_t* base, int step, int off) {
    constexpr int G = Px<PX>::G;
    uint32_t v = 0;
#pragma unroll
    for (int g = 0; g < 4; g += G) {
        const int b = off + g, x = b / PX, k = b - x * PX;
        const uint8_t* p = base + x * step + k;
        uint32_t t;
        if (G == 4) t = *reinterpret_cast<const uint32_t*>(p);
        else if (G == 2) t = *reinterpret_cast<const uint16_t*>(p);
        else t = *p;
        v |= t << (8 * g);
    }
    return v;
}

template <int PX>
__global__ __launch_bounds__(256) void k_orient_rows(OrientArgs a) {
    constexpr int SB = kStrip * PX;  // bytes of a full strip
    __shared__ __attribute__((aligned(16))) uint8_t lds[4][SB + 8];
    const int img = blockIdx.z, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint8_t* src = a.src_tab ? reinterpret_cast<const uint8_t*>(a.src_tab[img]) : a.src + img * a.src_img_stride;
    uint8_t* dst = a.dst_tab ? reinterpret_cast<uint8_t*>(a.dst_tab[img]) : a.dst + img * a.dst_img_stride;
    uint8_t* buf = lds[wave];
    const uint32_t DX0 = blockIdx.x * kStrip;                        // destination column of the strip
    const int n = (int)min((uint32_t)kStrip, a.W - DX0);             // its pixels
    const size_t row_bytes = (size_t)a.W * PX;
    const size_t first = (size_t)(a.flip_x ? a.W - DX0 - n : DX0) * PX;  // its first source byte
    const size_t seg_lo = a.src_aligned ? first & ~(size_t)3 : first;
    const int shift = (int)(first - seg_lo), need = shift + n * PX, seg_bytes = n * PX;
    for (uint32_t y0 = blockIdx.y * 4; y0 < a.H; y0 += gridDim.y * 4) {
        const uint32_t y = y0 + wave;
        const bool active = y < a.H;
        if (active) {
            const uint8_t* row = src + (size_t)(a.flip_y ? a.H - 1 - y : y) * a.src_pitch;
            if (a.src_aligned) {
                for (int o = 4 * lane; o < need; o += 256) {
                    const size_t off = seg_lo + o;
                    if (off + 4 <= row_bytes) {
                        *reinterpret_cast<uint32_t*>(buf + o) = *reinterpret_cast<const uint32_t*>(row + off);
                    } else {
                        for (int k = 0; k < 4; ++k)
                            if (off + k < row_bytes) buf[o + k] = row[off + k];
                    }
                }
            } else {
                for (int o = lane; o < need; o += 64) buf[o] = row[seg_lo + o];
            }
        }
        __syncthreads();
        if (active) {
            uint8_t* drow = dst + (size_t)y * a.dst_pitch + (size_t)DX0 * PX;
            const uint8_t* base = buf + shift + (a.flip_x ? (n - 1) * PX : 0);
            const int step = a.flip_x ? -PX : PX;
            if (a.dst_aligned) {
                for (int o = 4 * lane; o < seg_bytes; o += 256) {
                    if (o + 4 <= seg_bytes) {
                        *reinterpret_cast<uint32_t*>(drow + o) = gather_dword<PX>(base, step, o);
                    } else {
                        for (int b = o; b < seg_bytes; ++b) drow[b] = base[(b / PX) * step + b % PX];
                    }
                }
            } else {
                for (int b = lane; b < seg_bytes; b += 64) drow[b] = base[(b / PX) * step + b % PX];
            }
        }
        __syncthreads();
    }
}

template <int PX>
__global__ __launch_bounds__(256) void k_orient_transpose(OrientArgs a) {
    constexpr int LP = Px<PX>::LP, RB = kT * PX;  // LDS row pitch; bytes of a full tile row
    __shared__ __attribute__((aligned(16))) uint8_t tile[kT * LP];
    const int img = blockIdx.z, tid = threadIdx.x;
    const uint8_t* src = a.src_tab ? reinterpret_cast<const uint8_t*>(a.src_tab[img]) : a.src + img * a.src_img_stride;
    uint8_t* dst = a.dst_tab ? reinterpret_cast<uint8_t*>(a.dst_tab[img]) : a.dst + img * a.dst_img_stride;
    const uint32_t X0 = blockIdx.x * kT;   // first source column of the tile
    const uint32_t DX0 = blockIdx.y * kT;  // first destination column: source rows DX0 + j, or H-1 - (DX0 + j)
    const int tw = (int)min((uint32_t)kT, a.W - X0), th = (int)min((uint32_t)kT, a.H - DX0);
    const int row_bytes = tw * PX, seg_bytes = th * PX;
    const uint8_t* s0 = src + (size_t)X0 * PX;
    if (a.src_aligned) {
        for (int idx = tid; idx < kT * (RB / 4); idx += 256) {
            const int j = idx / (RB / 4), o = 4 * (idx - j * (RB / 4));
            if (j >= th) break;
            if (o >= row_bytes) continue;
            const uint8_t* row = s0 + (size_t)(a.flip_y ? a.H - 1 - (DX0 + j) : DX0 + j) * a.src_pitch;
            if (o + 4 <= row_bytes) {
                *reinterpret_cast<uint32_t*>(tile + j * LP + o) = *reinterpret_cast<const uint32_t*>(row + o);
            } else {
                for (int b = o; b < row_bytes; ++b) tile[j * LP + b] = row[b];
            }
        }
    } else {
        for (int idx = tid; idx < kT * RB; idx += 256) {
            const int j = idx / RB, o = idx - j * RB;
            if (j >= th) break;
            if (o >= row_bytes) continue;
            tile[j * LP + o] = s0[(size_t)(a.flip_y ? a.H - 1 - (DX0 + j) : DX0 + j) * a.src_pitch + o];
        }
    }
    __syncthreads();
    // source column X0 + c is destination row X0 + c, or W-1 - (X0 + c); its pixels DX0 .. DX0 + th - 1
    // are LDS rows 0 .. th - 1 at column c
    uint8_t* d0 = dst + (size_t)DX0 * PX;
    if (a.dst_aligned) {
        for (int idx = tid; idx < kT * (RB / 4); idx += 256) {
            const int c = idx / (RB / 4), o = 4 * (idx - c * (RB / 4));
            if (c >= tw) break;
            if (o >= seg_bytes) continue;
            uint8_t* drow = d0 + (size_t)(a.flip_x ? a.W - 1 - (X0 + c) : X0 + c) * a.dst_pitch;
            const uint8_t* col = tile + c * PX;
            if (o + 4 <= seg_bytes) {
                *reinterpret_cast<uint32_t*>(drow + o) = gather_dword<PX>(col, LP, o);
            } else {
                for (int b = o; b < seg_bytes; ++b) drow[b] = col[(b / PX) * LP + b % PX];
            }
        }
    } else {
        for (int idx = tid; idx < kT * RB; idx += 256) {
            const int c = idx / RB, b = idx - c * RB;
            if (c >= tw) break;
            if (b >= seg_bytes) continue;
            d0[(size_t)(a.flip_x ? a.W - 1 - (X0 + c) : X0 + c) * a.dst_pitch + b] = tile[(b / PX) * LP + c * PX + b % PX];
        }
    }
}

template <int PX>
hipError_t launch_px(const OrientArgs& a, bool transposed, int n, hipStream_t s) {
    if (transposed) {
        const dim3 grid((a.W + kT - 1) / kT, (a.H + kT - 1) / kT, (unsigned)n);
        hipLaunchKernelGGL(k_orient_transpose<PX>, grid, dim3(256), 0, s, a);
    } else {
        const uint32_t gy = std::min<uint32_t>((a.H + 3) / 4, 65535u);
        const dim3 grid((a.W + kStrip - 1) / kStrip, gy, (unsigned)n);
        hipLaunchKernelGGL(k_orient_rows<PX>, grid, dim3(256), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_orient(const uint8_t* src, size_t src_pitch, size_t src_img_stride, uint8_t* dst, size_t dst_pitch,
                         size_t dst_img_stride, uint32_t W, uint32_t H, int px, int orientation, int n, hipStream_t s,
                         const uint64_t* src_tab, const uint64_t* dst_tab) {
    OrientArgs a{};
    a.src = src; a.src_pitch = src_pitch; a.src_img_stride = src_img_stride;
    a.dst = dst; a.dst_pitch = dst_pitch; a.dst_img_stride = dst_img_stride;
    a.src_tab = src_tab; a.dst_tab = dst_tab;
    a.W = W; a.H = H;
    a.flip_x = orientation == 2 || orientation == 3 || orientation == 7 || orientation == 8;
    a.flip_y = orientation == 3 || orientation == 4 || orientation == 6 || orientation == 7;
    // (images named by a table are ik_images: pooled hipMalloc blocks, 256-byte pitches)
    a.src_aligned = src_tab ? (src_pitch & 3) == 0
                            : (((uintptr_t)src | src_pitch | (n > 1 ? src_img_stride : 0)) & 3) == 0;
    a.dst_aligned = dst_tab ? (dst_pitch & 3) == 0
                            : (((uintptr_t)dst | dst_pitch | (n > 1 ? dst_img_stride : 0)) & 3) == 0;
    const bool t = orientation >= 5;
    switch (px) {
        case 1: return launch_px<1>(a, t, n, s);
        case 2: return launch_px<2>(a, t, n, s);
        case 3: return launch_px<3>(a, t, n, s);
        case 4: return launch_px<4>(a, t, n, s);
        case 6: return launch_px<6>(a, t, n, s);
        case 8: return launch_px<8>(a, t, n, s);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace ik
