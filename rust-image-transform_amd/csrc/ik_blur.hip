// ik_blur.hip -- Gaussian blur and the unsharp mask built on it: the project's own
// definition, the resampler's arithmetic at ratio 1.  Per channel
// sample, alpha included, with the host-built weights of ik_blur_plan.h:
//
//   vertical    t = 0; for ascending k: t = t + (float)S[left_y + k][b] * w_y[k]     (f32)
//   horizontal  the same over the f32 rows with the column weights, then
//               B = round_half_away(clamp(t, 0, M))          M = 255 or 65535
//   unsharpen   d = S - B;  out = |d| > threshold ? clamp(S + d, 0, M) : S
//
// Each product and each sum is rounded on its own (no contraction in this file), the taps
// run in ascending order, and nothing is rounded or clamped between the passes.
//
//   k_blur<DEPTH, SHARPEN>   DEPTH 1 or 2 bytes per sample, C = 1..4 at run time
//
// One fused launch, the f32 intermediate only in LDS.  A 256-thread workgroup owns a
// kBlurTileW x kBlurTileH output tile.
//   1. Vertical pass.  The tile's columns plus the halo the horizontal taps reach -- the
//      columns [left_x[first], left_x[last] + count_x[last]), which the host tables keep
//      inside the image, so an edge tile has a shorter halo and no clamped duplicates --
//      are filtered down into kBlurTileH LDS rows of floats.  A wave takes a tile row
//      (its weights are wave-uniform: scalar loads), a lane one dword of a source row
//      per tap (4 or 2 samples), consecutive lanes consecutive dwords.  With an
//      unaligned source, and for the dword that straddles the end of a row, a lane
//      loads its samples byte by byte and none past W * C * DEPTH bytes.
//   2. Horizontal pass.  A lane takes one output sample, consecutive lanes consecutive
//      samples of a tile row, so the LDS words they read are consecutive (no bank
//      conflicts for any C).  A tile inside the axis's interior run reads one shared
//      weight vector through scalar loads; any other tile its outputs' own rows.  The
//      unsharp epilogue reads the source sample again.  Results go to an LDS staging row.
//   3. The staging rows leave as whole dwords (a tile starts at a multiple of 4 bytes of
//      its row), or byte by byte for an unaligned destination and a row's last partial
//      dword: nothing past W * C * DEPTH bytes of a destination row is written.
//
// What the halo costs.  The vertical pass filters TW + 2R columns for TW outputs and reads
// count_y source rows for each of the TH tile rows, the overlap between neighbouring rows
// coming from cache: at sigma 1 (R = 2, 5 taps) that is 68 columns x 80 row reads per 64 x
// 16 outputs, 1.06 x the columns; at sigma 32 (R = 64, 129 taps) 192 columns x 2064 row
// reads, 3 x the columns, each of them 129 taps deep.  The LDS is sized by the launch for
// the halo its sigma needs (C = 4: 21 KiB at sigma 1, 53 KiB at sigma 32, which leaves
// three workgroups to a CU).  Large sigmas are paid for in the vertical pass.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "ik_internal.h"

#pragma clang fp contract(off)

namespace ik {

namespace {

// LDS floats of a tile row whose outputs reach `cols` source columns of C samples: up to 3
// samples more where the aligned start reaches back, up to 3 where the last dword reaches
// on; a multiple of 4, so a lane's 4 floats are one 16-byte store
inline int blur_lds_row(int cols, int C) { return (cols * C + 6 + 3) & ~3; }
constexpr int kBlurStageRow = kBlurTileW * 4;  // samples of a staging row

template <typename T>
using cptr = const __attribute__((address_space(4))) T*;
template <typename T>
__device__ __forceinline__ cptr<T> as_const(const T* p) { return (cptr<T>)p; }

// clamp(t, 0, M) then f32::round (half away from zero): the resize kernels' float_nearest
template <int DEPTH>
__device__ __forceinline__ int float_nearest(float t) {
    constexpr float M = DEPTH == 1 ? 255.0f : 65535.0f;
    t = t < 0.0f ? 0.0f : (t > M ? M : t);
    return (int)roundf(t);
}

// one sample (native-endian u16 at DEPTH 2); bytes when the address may be odd
template <int DEPTH>
__device__ __forceinline__ uint32_t load_sample(const uint8_t* p, bool aligned) {
    if (DEPTH == 1) return *p;
    if (aligned) return *reinterpret_cast<const uint16_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8);
}

template <int DEPTH, bool SHARPEN>
__global__ __launch_bounds__(256) void k_blur(BlurArgs a, int lds_row) {
    constexpr int SPW = 4 / DEPTH;  // samples of a dword
    extern __shared__ __attribute__((aligned(16))) float tile[];  // kBlurTileH rows of lds_row floats
    uint8_t* stage = reinterpret_cast<uint8_t*>(tile + kBlurTileH * lds_row);  // then the staging rows
    const int img = blockIdx.z;
    const uint8_t* src = a.src_tab ? reinterpret_cast<const uint8_t*>(a.src_tab[img]) : a.src + img * a.src_img_stride;
    uint8_t* dst = a.dst_tab ? reinterpret_cast<uint8_t*>(a.dst_tab[img]) : a.dst + img * a.dst_img_stride;
    const int C = (int)a.C;
    const int x0 = (int)blockIdx.x * kBlurTileW, y0 = (int)blockIdx.y * kBlurTileH;
    const int tw = min(kBlurTileW, (int)a.W - x0), th = min(kBlurTileH, (int)a.H - y0);
    // the source columns the tile's outputs reach (left and left + count never decrease)
    const int xl = x0 + tw - 1;
    const int cx0 = as_const(a.x.left)[x0], cx1 = as_const(a.x.left)[xl] + as_const(a.x.cnt)[xl];
    const int row_samples = (int)a.W * C;
    const int sa = cx0 * C, se = cx1 * C;                     // their samples [sa, se) of a row
    const int so = a.src_aligned ? sa & ~(SPW - 1) : sa;     // the LDS row starts here: a whole dword
    const int ngroups = (se - so + SPW - 1) / SPW;           // ngroups * SPW <= lds_row (launch_blur sizes it)
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;

    // 1. vertical pass into the tile
    for (int yy = wave; yy < th; yy += 4) {
        const int y = __builtin_amdgcn_readfirstlane(y0 + yy);
        const int ly = as_const(a.y.left)[y], ny = as_const(a.y.cnt)[y];
        cptr<float> wy = as_const(a.y.w) + (size_t)y * a.y.T;
        float* trow = tile + yy * lds_row;
        for (int g = lane; g < ngroups; g += 64) {
            const int s = so + g * SPW;  // the group's first sample
            const uint8_t* p = src + (size_t)ly * a.src_pitch + (size_t)s * DEPTH;
            float t[SPW];
#pragma unroll
            for (int j = 0; j < SPW; ++j) t[j] = 0.0f;
            if (a.src_aligned && s + SPW <= row_samples) {
                for (int k = 0; k < ny; ++k) {
                    const uint32_t v = *reinterpret_cast<const uint32_t*>(p);
                    const float w = wy[k];
#pragma unroll
                    for (int j = 0; j < SPW; ++j) {
                        const float f = (float)(DEPTH == 1 ? (v >> (8 * j)) & 0xFFu : (v >> (16 * j)) & 0xFFFFu);
                        const float prod = f * w;
                        t[j] = t[j] + prod;
                    }
                    p += a.src_pitch;
                }
            } else {
#pragma unroll
                for (int j = 0; j < SPW; ++j) {
                    if (s + j >= row_samples) continue;  // past the row: never read, never used
                    const uint8_t* q = p + j * DEPTH;
                    for (int k = 0; k < ny; ++k) {
                        const float prod = (float)load_sample<DEPTH>(q, a.src_aligned != 0) * wy[k];
                        t[j] = t[j] + prod;
                        q += a.src_pitch;
                    }
                }
            }
            if constexpr (SPW == 4) *reinterpret_cast<float4*>(trow + g * 4) = make_float4(t[0], t[1], t[2], t[3]);
            else *reinterpret_cast<float2*>(trow + g * 2) = make_float2(t[0], t[1]);
        }
    }
    __syncthreads();

    // 2. horizontal pass, clamp and round, the unsharp epilogue; into the staging rows
    const int ns = tw * C;  // samples of a tile row
    const bool uni = x0 >= a.x.u_lo && x0 + tw <= a.x.u_hi;
    for (int i = (int)threadIdx.x; i < th * ns; i += 256) {
        const int yy = i / ns, s = i - yy * ns;
        const int x = s / C, c = s - x * C, xg = x0 + x;
        const float* row = tile + yy * lds_row + (sa - so) + c;
        float t = 0.0f;
        if (uni) {
            const float* q = row + (xg - a.x.u_dl - cx0) * C;
            cptr<float> w = as_const(a.x.w) + (size_t)a.x.u_lo * a.x.T;
            const int nx = a.x.u_cnt;
            for (int k = 0; k < nx; ++k) {
                const float prod = q[k * C] * w[k];
                t = t + prod;
            }
        } else {
            const float* q = row + (a.x.left[xg] - cx0) * C;
            const float* w = a.x.w + (size_t)xg * a.x.T;
            const int nx = a.x.cnt[xg];
            for (int k = 0; k < nx; ++k) {
                const float prod = q[k * C] * w[k];
                t = t + prod;
            }
        }
        int v = float_nearest<DEPTH>(t);
        if (SHARPEN) {
            constexpr int M = DEPTH == 1 ? 255 : 65535;
            const int S = (int)load_sample<DEPTH>(
                src + (size_t)(y0 + yy) * a.src_pitch + ((size_t)xg * C + c) * DEPTH, a.src_aligned != 0);
            const int d = S - v;
            const int sharp = min(max(S + d, 0), M);
            v = (d < 0 ? -d : d) > a.threshold ? sharp : S;
        }
        if (DEPTH == 1) stage[yy * kBlurStageRow + s] = (uint8_t)v;
        else reinterpret_cast<uint16_t*>(stage)[yy * kBlurStageRow + s] = (uint16_t)v;
    }
    __syncthreads();

    // 3. the staging rows out
    const int rb = ns * DEPTH, nd = (rb + 3) >> 2;
    for (int i = (int)threadIdx.x; i < th * nd; i += 256) {
        const int yy = i / nd, d = i - yy * nd;
        uint8_t* dp = dst + (size_t)(y0 + yy) * a.dst_pitch + (size_t)x0 * C * DEPTH + 4 * d;
        const uint8_t* sp = stage + yy * kBlurStageRow * DEPTH + 4 * d;
        if (a.dst_aligned && 4 * d + 4 <= rb) {
            *reinterpret_cast<uint32_t*>(dp) = *reinterpret_cast<const uint32_t*>(sp);
        } else {
#pragma unroll
            for (int b = 0; b < 4; ++b)
                if (4 * d + b < rb) dp[b] = sp[b];
        }
    }
}

template <int DEPTH, bool SHARPEN>
hipError_t launch_variant(const BlurArgs& a, int n, hipStream_t s) {
    const dim3 grid((a.W + kBlurTileW - 1) / kBlurTileW, (a.H + kBlurTileH - 1) / kBlurTileH, (unsigned)n);
    // a tile's outputs reach at most TW + halo columns, and never more than the image has
    const int cols = (int)std::min<uint32_t>(a.W, (uint32_t)(kBlurTileW + a.halo));
    const int lds_row = blur_lds_row(cols, (int)a.C);
    const size_t lds = sizeof(float) * kBlurTileH * lds_row + (size_t)kBlurTileH * kBlurStageRow * DEPTH;
    hipLaunchKernelGGL((k_blur<DEPTH, SHARPEN>), grid, dim3(256), lds, s, a, lds_row);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_blur(const BlurArgs& a, int depth, bool sharpen, int n, hipStream_t s) {
    if (!a.W || !a.H || a.C < 1 || a.C > 4 || n < 1 || (uint32_t)n > kBlurMaxImages) return hipErrorInvalidValue;
    if ((a.H + kBlurTileH - 1) / kBlurTileH > 65535u) return hipErrorInvalidValue;  // grid.y
    if (a.halo < 0 || a.halo > 2 * kBlurMaxR) return hipErrorInvalidValue;          // the LDS tile
    if (depth == 1) return sharpen ? launch_variant<1, true>(a, n, s) : launch_variant<1, false>(a, n, s);
    if (depth == 2) return sharpen ? launch_variant<2, true>(a, n, s) : launch_variant<2, false>(a, n, s);
    return hipErrorInvalidValue;
}

}  // namespace ik
