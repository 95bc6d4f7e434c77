// ik_vp8d_gpu.h -- launchers of the WebP (VP8) decoder's device half (ik_vp8d.hip); the
// host half (container, frame header, partition 0, the token partitions, driver) is
// ik_vp8d_host.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include "ik_vp8d.h"

namespace ik {
namespace vp8d {

// One image of a decode launch (device addresses).  The planes are macroblock-aligned
// (mb_w * 16 by mb_h * 16 luma, half that chroma); top holds the unfiltered bottom rows
// the next MB row predicts from, two MB rows of them (32 bytes per MB: Y 16, U 8, V 8).
struct alignas(16) DImg {
    const DFrame* fr;
    const DMB* mbs;
    const uint32_t* coef;    // the frame's non-zero coefficients: (value << 16) | position in
                             // the MB's 384 (Y 16x16, U 4x16, V 4x16; dequantised, Y2 applied)
    const uint32_t* coef_at; // per MB its first entry; [mb_w * mb_h] = the total
    const uint8_t* flags;    // per MB: 1 = some coefficient is non-zero (libwebp !skip)
    uint8_t *y, *u, *v;
    uint8_t* top;
    uint8_t* out;            // the ik_image's pixels (RGB; RGBA where fr->channels is 4)
    uint32_t ys, uvs;        // plane pitches
    uint32_t out_pitch;
    uint32_t* prog;          // per MB row: MBs done (zeroed per launch)
    uint32_t* err;           // set when a row's wait times out (zeroed per launch)
    uint8_t* alpha;          // fr->channels == 4: the staged alpha plane (alpha_pitch(w) apart, as
                             // filtered by fr->alpha_filter; k_vp8d_alpha un-filters it in place)
};

// One block's work of the colour launch: rows [row0, row0 + rows) of image img
struct DTile {
    uint32_t img, row0, rows;
};
// the rows of a w-wide image that make one tile: about kRgbTilePixels pixels
constexpr uint32_t kRgbTilePixels = 1024;
inline uint32_t rgb_tile_rows(uint32_t w) { return w >= kRgbTilePixels ? 1 : kRgbTilePixels / w; }

// The launch plan beside imgs (the images in plan order: ik_vp8d_plan.h): row_start[k]
// is the ticket of image k's first MB row, row_start[n] the launch's MB rows.
// ticket: zeroed per launch.  The grid is min(rows, 256) for one image and, for
// several, min(rows, the waves the device holds at once: the kernel's occupancy times
// the CU count; kReconBatchGrid if the runtime does not say).  IK_VP8D_GRID (dev
// switch) forces a grid: a number, or "occ" for the batch's.  *grid_used (may be
// null) is the grid.
constexpr uint32_t kReconBatchGrid = 1024;
hipError_t launch_vp8d_recon(const DImg* imgs, const uint32_t* row_start, int n, uint32_t total_rows, uint32_t* ticket,
                             hipStream_t s, uint32_t* grid_used);
// which[0 .. n): the launch's images whose alpha plane has a filter to undo (a wave each)
hipError_t launch_vp8d_alpha(const DImg* imgs, const uint32_t* which, uint32_t n, hipStream_t s);
// rgba: some image of the launch has four channels
hipError_t launch_vp8d_rgb(const DImg* imgs, const DTile* tiles, uint32_t ntiles, bool rgba, hipStream_t s);

}  // namespace vp8d
}  // namespace ik
