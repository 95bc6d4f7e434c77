// ik_internal.h -- shared declarations between the HIP kernels (ik_kernels.hip)
// and the host runtime (ik_*.cpp) of libimagekit_hip.so.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/imagekit_hip.h"
#include "ik_jpeg_sync.h"
#include "ik_resize_plan.h"

namespace ik {

// resize arithmetic (ik_set_resize_mode): IK_RESIZE_EXACT (the reference's f32
// sequence, bit-exact) or IK_RESIZE_FMA (fused multiply-add, within 1 LSB)
int resize_mode();

// kThreads, kStripBytes, kRowWords, ... and the host half of a resize plan: ik_resize_plan.h

// Everything the resize kernels read.  Weight tables follow image 0.25.8
// sample.rs (see ik_plan.cpp); tables live in one device allocation per plan.
struct ResizeArgs {
    const uint8_t* src;
    size_t src_pitch, src_img_stride;
    uint8_t* dst;
    size_t dst_pitch, dst_img_stride;
    int W, H, C, nw, nh, row_bytes;
    const int* ly;     // [nh]   first source row of each output row
    const int* ny;     // [nh]   tap count
    const float* wy;   // [nh*Ty] normalised weights, zero padded
    int Ty;
    const int* lx;     // [nw]
    const int* nx;     // [nw]
    const float* wx;   // [nw*Tx]
    int Tx;
    const int* strips; // [NS*3] (ox0, ox1, first source byte)
    int NS;
    const int* bands;  // [NB*2] (oy0, oy1)
    int NB;
    // fused-kernel step tables.  A band is a sequence of steps; a step brings in
    // up to R new source rows [start, start+count) and scatters them into the A
    // rolling accumulators (acc[d] = output row next+d); `emit` completes row next.
    const int* step_hdr;        // [nsteps][4] (start, count, emit, 0)
    const unsigned long long* step_mask;  // [nsteps] bit j*A+d: row start+j feeds acc[d]
    const float* step_w;        // [nsteps][R][A] the matching weights (0 elsewhere)
    const int* band_step;       // [NB+1] first step of each band
    // periodic sweep (k_resize_periodic): step t brings in source rows
    // R*t + per_base .. +R-1, and output row y takes its taps from steps y .. y+A-1
    const float* per_w;      // [steps][A*R]: per_w[t][e*R + j] = weight of row j of step t in output t-e
    const int* per_bands;    // [NBp*2] (oy0, oy1)
    int per_base, NBp;
    int max_strip_cols;      // max output columns of a strip (LDS table size)
    int max_strip_weights;   // max nox*Tx of a strip (LDS weights size when in LDS)
    int lds_pad;             // zeroed LDS words after the column offsets (ik_resize_plan.h)
    float* tmp;        // naive path only: f32 vertical intermediate [n][nh][tmp_span]
    // naive path: the source samples per row its vertical pass covers, [tmp_col0,
    // tmp_col0 + tmp_span): the columns the plan's outputs read (a whole resize: the row)
    int tmp_col0, tmp_span;
    // fused path, images anywhere in memory: per-image base pointers (device
    // arrays, [n]); null = src + img * src_img_stride / dst + img * dst_img_stride
    const uint64_t* src_tab;
    const uint64_t* dst_tab;
};

// Host-side plan for one (W,H,C,window,filter,band height) geometry.
struct ResizePlan {
    int W = 0, H = 0, C = 0, nw = 0, nh = 0, filter = 0;
    int iw = 0, ih = 0, x0 = 0, y0 = 0;  // the window: ResizeTables (ik_resize_plan.h)
    int slots = 0;        // accumulator slots the fused kernel needs (0 = naive path)
    int rows = 0;         // prefetch depth: max source rows consumed per output row
    bool weights_in_lds = false;
    int flush = 3;        // completed vertical rows staged in LDS per horizontal pass
    int NS = 0, NB = 0;
    int per_A = 0, per_R = 0;  // periodic geometry (k_resize_periodic); 0 = not periodic
    size_t table_bytes = 0;
    void* dev_tables = nullptr;
    ResizeArgs args{};    // pointers into dev_tables; src/dst/tmp filled per launch
};

// ---- launchers (ik_kernels.hip) ----
// The fused kernel addresses one source image through a buffer descriptor with
// 32-bit num_records and row offsets: images over INT32_MAX bytes take the naive
// two-pass path (whose caller must then pass naive_tmp): resize_fused_fits
// (ik_resize_plan.h).
// 16-bit images: the two-pass path over u16 samples (tmp: nh * plan.args.tmp_span floats), and
// the u16 -> u8 rescale of to_rgb8 / to_rgba8
hipError_t launch_resize16(const ResizePlan& plan, const uint8_t* src, size_t src_pitch, uint8_t* dst,
                           size_t dst_pitch, float* tmp, hipStream_t s);
hipError_t launch_u16_to_u8(const uint8_t* src, size_t sp, uint8_t* dst, size_t dp, int row_samples, int rows,
                            hipStream_t s);
hipError_t launch_resize(const ResizePlan& plan, const uint8_t* src, size_t src_pitch,
                         size_t src_img_stride, uint8_t* dst, size_t dst_pitch,
                         size_t dst_img_stride, int n, float* naive_tmp, hipStream_t s,
                         const uint64_t* src_tab = nullptr, const uint64_t* dst_tab = nullptr);
// dynamic LDS bytes of the fused kernel
size_t resize_lds_bytes(const ResizeArgs& a, bool wl, int flush);
// the kernel launch_resize picks for this plan (ik_resize_kernel_name)
const char* resize_kernel_name(const ResizePlan& plan, size_t src_pitch);
// the same choice as a ResizeFamily index, from a host-only plan (ik_resize_plan_info)
int resize_family_of(const ResizeTables& t, size_t src_pitch);
hipError_t launch_webp_yuv420(const uint8_t* src, int w, int h, int C, size_t pitch,
                              size_t img_stride, uint8_t* yuv /* Y, U, V planes per image */,
                              size_t yuv_img_stride, int n, const uint16_t* gamma_to_lin,
                              const int* lin_to_gamma, hipStream_t s,
                              const uint64_t* src_tab = nullptr /* per-image bases instead of img_stride */);
// the same conversion over n images of different sizes in one launch: a device table of
// these (grid.z = image; max_w / max_h: the largest of the table's sizes)
struct WebpYuvItem {
    const uint8_t* src;  // pixels, rows pitch bytes apart
    uint8_t* yuv;        // Y, U, V planes back to back
    size_t pitch;
    int32_t w, h, C, pad;
};
hipError_t launch_webp_yuv420_items(const WebpYuvItem* items, int n, int max_w, int max_h,
                                    const uint16_t* gamma_to_lin, const int* lin_to_gamma, hipStream_t s);
// n images; planes (Y, U, V, A: w*h each) plane_img_stride apart; transparent[n]
// zeroed here, then set to 1 for every image with an alpha < 255
hipError_t launch_avif_yuv444(const uint8_t* src, int w, int h, int C, size_t pitch, size_t img_stride,
                              uint8_t* planes, size_t plane_img_stride, int* transparent, int n, hipStream_t s);
hipError_t launch_jpeg_coeffs(const uint8_t* src, int w, int h, int C, size_t pitch,
                              size_t img_stride, const uint8_t* qtables /*dev, 128 B*/,
                              int16_t* coef, size_t coef_img_stride, int n, hipStream_t s,
                              const uint64_t* src_tab = nullptr /* per-image bases (device), or src + i * img_stride */);

// JPEG reconstruction (ik_jpeg.hip): dequantise + islow IDCT every 8x8 block of
// the coefficient image into per-component sample planes, then fancy-upsample +
// colour-convert into the device image.
struct JpegGeom {
    int ncomp, W, H, hmax, vmax;
    int colorspace;                 // 0 gray, 1 YCbCr, 2 RGB, 3 CMYK, 4 YCCK (4 components -> RGB8)
    int adobe;                      // APP14 Adobe present: CMYK / YCCK samples are stored inverted
    int recon;                      // IK_JPEG_RECON_LIBJPEG / IK_JPEG_RECON_ZUNE (ik_jpeg.hip)
    int h[4], v[4], bw[4], bh[4], dw[4], dh[4];
    long long blk0[4];              // first block of each component in coef
    long long plane0[4];            // byte offset of each component plane (bw*8 x bh*8)
    long long nblocks;
    const uint16_t* qt;             // [component][64] natural order
    const int16_t* coef;            // [block][64] natural order, quantised
    uint8_t* planes;
};
hipError_t launch_jpeg_reconstruct(const JpegGeom& g, uint8_t* dst, size_t dst_pitch, hipStream_t s);
// a batch's reconstructions in three launches (items in device memory)
struct JpegReconItem {
    JpegGeom g;
    uint8_t* dst;
    size_t pitch;
    int fast;  // jpeg_zune_fast(g)
    int pad;
};
hipError_t launch_jpeg_reconstruct_batch(const JpegReconItem* items, int m, long long max_blocks, int max_w, int max_h,
                                         bool any_fast, bool any_slow, bool idct, hipStream_t s);
bool jpeg_zune_fast(const JpegGeom& g);

// Baseline Huffman tables (JpegHuffTables) and the self-synchronising decoder's
// per-lane code are in ik_jpeg_sync.h (shared with its CPU model).
//
// The self-synchronising baseline decoder (ik_jsync.hip), one batch of scans:
// one image's scan as the unstuffing kernels see it
struct JsImageDev {
    const uint8_t* scan;   // the entropy-coded bytes (stuffed, with RSTn markers), device
    long long scan_len;
    uint8_t* out;          // unstuffed bytes as big-endian words (scan_len + 4 kPadWords + 8 bytes)
    long long* ivl;        // interval start bits: ivl_cap entries (intervals + 1)
    int ivl_cap;
    int chunk0, nchunks;   // the image's 4 KiB chunks in the batch's chunk table
    int pad;
    uint32_t* totals;      // [0] bytes kept, [1] restart markers
    int* status;           // bit 0 a stray marker, 1 too many restart markers, 4 inconsistent / missing
                           // blocks, 8 a bad code in the decode pass: the host decoder decides
};
hipError_t launch_jsync_unstuff(JsImageDev* imgs, int nimg, const int2* chunks, int nchunks, uint2* counts,
                                hipStream_t s);
// wgs: (image, first lane of the image) per 256-lane workgroup; every image's lanes
// start on a multiple of 256 (jsync::Scan::lane0)
hipError_t launch_jsync_sync(const jsync::Scan* scans, const int2* wgs, int nwg, jsync::LaneRec* recs, hipStream_t s);
hipError_t launch_jsync_fix(const jsync::Scan* scans, int nimg, const int2* wgs, int nwg, jsync::LaneRec* recs,
                            int* rounds, hipStream_t s);
// bases (segmented prefix sums over each interval's lanes) then the decode pass;
// chunk_scratch: jsync_chunk_scratch_bytes(lanes); status[image]
hipError_t launch_jsync_bases_decode(const jsync::Scan* scans, int nimg, const int2* wgs, int nwg,
                                     const jsync::LaneRec* recs, jsync::LaneBase* bases, void* chunk_scratch,
                                     int* status, hipStream_t s);
size_t jsync_chunk_scratch_bytes(long long lanes);
// Progressive files without restart markers, after their Ah = 0 scans went through
// the launches above (a jsync::Scan per scan): one DC refinement scan of each of n
// images (list: their scans' indices; an image's DC refinements go in file order,
// launch by launch), and every (image, component)'s AC refinement scans in one
// launch (chains: (first, count) into list, file order); status[scan] |= 16 on a bad code
hipError_t launch_jprog_dc_refine(const jsync::Scan* scans, const int* list, int n, long long max_blocks, hipStream_t s);
hipError_t launch_jprog_ac_chain(const jsync::Scan* scans, const int2* chains, int nchains, const int* list, int* status,
                                 hipStream_t s);
// The marker walk over n JPEG files in device memory (ik_jpeg_walk.hip; the walk is
// ik_jpeg_walk.h): skel takes jwalk::kSlot bytes per file, recs a jwalk::Rec each
hipError_t launch_jpeg_walk(const uint64_t* files, const uint64_t* lens, int n, uint8_t* skel, void* recs,
                            hipStream_t s);
struct JpegScanArgs {
    const uint8_t* data;          // the scan's entropy-coded bytes (stuffed, with RST markers)
    long long size;
    const unsigned* seg;          // first byte of each restart interval (n_seg entries)
    int n_seg, restart;           // intervals, MCUs per interval
    long long total_mcu;
    int mcux;                     // MCUs per row (interleaved scans)
    int single, single_bw;        // one-component scan: an MCU is one block, single_bw per row
    int ns;                       // components in the scan, in scan order:
    int h[4], v[4], bw[4], td[4], ta[4];
    long long blk0[4];
    const JpegHuffTables* tabs;
    int16_t* coef;                // [block][64] natural order, pre-zeroed
    int* err;                     // set non-zero on a bad code (the host then redoes the scan)
    int lanes;                    // intervals per 64-lane workgroup (64, or fewer to cut divergence)
    // progressive scans (k_jpeg_prog): 1 DC first, 2 DC refine, 3 AC first, 4 AC refine
    int kind, Ss, Se, Al;
};
// One progressive scan with restart intervals (ik_jpeg.hip k_jpeg_prog): a lane per
// interval, the EOB run and DC predictions reset at each RSTn; the scans of an
// image run in stream order, each refining the coefficients of the ones before.
hipError_t launch_jpeg_prog(const JpegScanArgs& a, hipStream_t s);
int jpeg_lanes_for(long long total_lanes);  // lanes per wave for that many independent decoders

// Baseline Huffman coding of k_jpeg_coeffs' output on the GPU (ik_jpeg_enc.hip),
// the same bytes as ik_codec.cpp's host coder.  Per image: entropy-coded segment
// (stuffed, with pad_byte) in out + i*out_img_stride, its length in out_len[i]
// (0xffffffff: does not fit out_cap -> code it on the host).
struct JpegEncArgs {
    const int16_t* coef;       // [mcu][Y,Cb,Cr][64] natural order per image
    size_t coef_img_stride;    // int16 elements between images
    int nmcu;
    const uint32_t* huff;      // [ldc, lac, cdc, cac][256]: code << 8 | size
    uint8_t* work;             // per image: words_bytes of bit words, then out_cap staging bytes
    size_t work_img_bytes, words_bytes;
    uint8_t* out;              // device or pinned host memory
    size_t out_img_stride, out_cap;
    uint32_t* out_len;
};
hipError_t launch_jpeg_huff_enc(const JpegEncArgs& a, int n, hipStream_t s);
inline size_t jpeg_enc_cap(int w, int h) {  // stuffed-stream capacity per image
    return ((size_t)3 * w * h + 4096 + 15) & ~(size_t)15;
}
// What the two encoder launches need of a w x h image, and the Huffman launch's
// arguments over a caller's buffers (the callers' layouts differ: pointers, no layout)
struct JpegEncGeom {
    size_t nmcu;        // 8 x 8 blocks per component
    size_t coef_bytes;  // the int16 coefficients of one image
    size_t cap;         // stuffed-stream capacity per image
    size_t work_bytes;  // Huffman work per image: cap of bit words, cap of staging
    JpegEncArgs args(const int16_t* coef, size_t coef_img_stride, const uint32_t* huff, uint8_t* work, uint8_t* out,
                     uint32_t* out_len) const {
        JpegEncArgs a{};
        a.coef = coef;
        a.coef_img_stride = coef_img_stride;
        a.nmcu = (int)nmcu;
        a.huff = huff;
        a.work = work;
        a.work_img_bytes = work_bytes;
        a.words_bytes = cap;
        a.out = out;
        a.out_img_stride = cap;
        a.out_cap = cap;
        a.out_len = out_len;
        return a;
    }
};
inline JpegEncGeom jpeg_enc_geom(uint32_t w, uint32_t h) {
    const size_t nmcu = (size_t)((w + 7) / 8) * ((h + 7) / 8), cap = jpeg_enc_cap((int)w, (int)h);
    return JpegEncGeom{nmcu, nmcu * 3 * 64 * sizeof(int16_t), cap, 2 * cap};
}

// ---- EXIF orientation (ik_orient.hip) ----
// apply_orientation over n images of W x H pixels of px = C * depth bytes (1, 2, 3, 4, 6
// or 8): orientation 2..8 (1 is a copy: the callers use hipMemcpy2DAsync).  Transposing
// kinds (5..8) write H x W pixels.  Images i at src + i * src_img_stride, or at
// src_tab[i] / dst_tab[i] (device arrays of 4-byte-aligned bases) when those are given.
constexpr int kOrientTile = 64;    // the transposing kernel's tile edge, pixels
constexpr int kOrientStrip = 256;  // pixels of a row one wave of the row kernel takes
constexpr uint32_t kOrientMaxImages = 65535;  // grid.z
hipError_t launch_orient(const uint8_t* src, size_t src_pitch, size_t src_img_stride, uint8_t* dst, size_t dst_pitch,
                         size_t dst_img_stride, uint32_t W, uint32_t H, int px, int orientation, int n, hipStream_t s,
                         const uint64_t* src_tab = nullptr, const uint64_t* dst_tab = nullptr);

// ---- background flatten (ik_flatten.hip) ----
// alpha composited onto the colour rgb (0xRRGGBB) over n images of W x H pixels of cin
// samples of `depth` bytes: (cin, cout) = (4, 3), (2, 1) or (2, 3); images addressed as
// launch_orient addresses them.
constexpr int kFlattenSpan = 1024;            // pixels of a row one workgroup takes
constexpr int kFlattenRowCap = 256;           // most rows of workgroups in a launch (the rest: grid stride)
constexpr uint32_t kFlattenMaxImages = 65535;  // grid.z
hipError_t launch_flatten(const uint8_t* src, size_t src_pitch, size_t src_img_stride, uint8_t* dst, size_t dst_pitch,
                          size_t dst_img_stride, uint32_t W, uint32_t H, int cin, int cout, int depth, uint32_t rgb,
                          int n, hipStream_t s, const uint64_t* src_tab = nullptr, const uint64_t* dst_tab = nullptr);
// the channels a flatten of a c-channel image onto rgb leaves: Rgba -> 3, LumaA -> 1 for a
// gray colour and 3 for any other, anything without alpha -> c (no pass)
inline uint32_t flatten_out_channels(uint32_t c, uint32_t rgb) {
    if (c == 4) return 3;
    if (c == 2) return ((rgb >> 16) & 0xFF) == ((rgb >> 8) & 0xFF) && ((rgb >> 8) & 0xFF) == (rgb & 0xFF) ? 1 : 3;
    return c;
}

// ---- blur and unsharpen (ik_blur.hip) ----
// a Gaussian blur, or the unsharp mask built on it, over n images of W x H pixels of C
// samples of `depth` bytes, images addressed as launch_orient addresses them.  One axis's
// device tables are those of ik_blur_plan.h: per output left and count, T zero-padded
// weights, and the interior run that shares one weight vector.
constexpr int kBlurTileW = 64;   // output columns of a workgroup's tile
constexpr int kBlurTileH = 16;   // its rows
constexpr int kBlurMaxR = 65;    // most halo columns on a side (sigma 32: 64, one spare for f32 rounding)
constexpr uint32_t kBlurMaxImages = 65535;  // grid.z
struct BlurAxisTab {
    const int* left;
    const int* cnt;
    const float* w;
    int T;
    int u_lo, u_hi, u_dl, u_cnt;  // outputs [u_lo, u_hi): left = o - u_dl, u_cnt taps, the weights of row u_lo
};
struct BlurArgs {
    const uint8_t* src;
    size_t src_pitch, src_img_stride;
    uint8_t* dst;
    size_t dst_pitch, dst_img_stride;
    const uint64_t* src_tab;  // per-image bases (device), or null: src + img * src_img_stride
    const uint64_t* dst_tab;
    uint32_t W, H, C;
    BlurAxisTab x, y;
    int halo;                      // most source columns left plus right of an output's own (<= 2 * kBlurMaxR)
    int threshold;                 // unsharpen: |S - B| above it sharpens
    int src_aligned, dst_aligned;  // bases, pitches and strides are multiples of 4
};
hipError_t launch_blur(const BlurArgs& a, int depth, bool sharpen, int n, hipStream_t s);

// ---- watermark overlay (ik_overlay.hip) ----
// one overlay image composited in place over the window of n same-geometry base images
// (DESIGN section 4): the base of C samples of `depth` bytes, images at base + i *
// img_stride or at tab[i] (a device array of bases).  The overlay's own format (co
// channels of od bytes) is a run-time switch.  The window and the origin are those of
// ik_overlay_place; the launcher's caller has checked them against W x H.
constexpr int kOverlaySpan = 1024;             // window columns one workgroup takes
constexpr int kOverlayRowCap = 256;            // most rows of workgroups in a launch (the rest: grid stride)
constexpr uint32_t kOverlayMaxImages = 65535;  // grid.z
constexpr int32_t kOverlayMaxDim = 1 << 24;    // most pixels on an axis, and the largest |dx|, |dy|
struct OverlayArgs {
    uint8_t* base;
    size_t pitch, img_stride;
    const uint64_t* tab;           // per-image bases (device), or null: base + img * img_stride
    const uint8_t* ov;             // the overlay's pixels
    size_t ov_pitch;
    int32_t wo, ho, co, od;        // its size, channels and bytes per sample
    int32_t wx, wy, ww, wh;        // the window in the base, not empty
    int32_t x0, y0;                // the overlay's origin in the base (may be negative)
    int32_t tile;
    uint32_t opM;                  // the opacity at the base's depth (op, or op * 257)
    int aligned;                   // the bases, the pitch and the stride are multiples of 4
    int ov_dword;                  // the overlay is 4 x 8 bits and its base and pitch are multiples of 4
};
hipError_t launch_overlay(const OverlayArgs& a, int C, int depth, int n, hipStream_t s);

// ---- colour adjustment (ik_adjust.hip) ----
// a plan (ik_adjust_plan.h) applied in place over n same-geometry images of C samples of
// `depth` bytes, images at base + i * img_stride or at tab[i].  matrix:
// q is applied (C >= 3 only); tone: the device table, 256 bytes at depth 1 and 65536
// uint16 at depth 2, or null: no table.  One of the two at least.
constexpr int kAdjustSpan = 1024;             // pixels of a row one workgroup takes
constexpr int kAdjustRowCap = 256;            // most rows of workgroups in a launch (the rest: grid stride)
constexpr uint32_t kAdjustMaxImages = 65535;  // grid.z
constexpr uint32_t kAdjustMaxDim = 1u << 24;  // most pixels on an axis
struct AdjustArgs {
    uint8_t* base;
    size_t pitch, img_stride;
    const uint64_t* tab;  // per-image bases (device), or null: base + img * img_stride
    const void* tone;     // the tone table (device), 4-byte aligned
    int32_t q[9];         // the Q16 matrix, row by row
    uint32_t W, H;
    int aligned;          // the bases, the pitch and the stride are multiples of 4
};
hipError_t launch_adjust(const AdjustArgs& a, int C, int depth, bool matrix, int n, hipStream_t s);

// ---- pad (ik_pad.hip) ----
// n same-geometry images of W x H pixels of px = C * depth bytes (1, 2, 3, 4, 6 or 8) placed
// at (x0, y0) of cw x ch canvases, images addressed as launch_orient
// addresses them.  W, H >= 1; the canvas holds the image; the canvas bases, pitch and stride
// are multiples of 4 (the source's may be anything).
constexpr int kPadSpan = 1024;             // canvas pixels of a row one workgroup takes
constexpr int kPadRowCap = 256;            // most rows of workgroups in a launch (the rest: grid stride)
constexpr uint32_t kPadMaxImages = 65535;  // grid.z
constexpr uint32_t kPadMaxDim = 1u << 24;  // most pixels on an axis of the image and of the canvas
struct PadArgs {
    const uint8_t* src;
    size_t src_pitch, src_img_stride;
    uint8_t* dst;
    size_t dst_pitch, dst_img_stride;
    const uint64_t* src_tab;  // per-image bases (device), or null: src + img * src_img_stride
    const uint64_t* dst_tab;
    uint32_t W, H, cw, ch;
    int32_t x0, y0;      // the image's origin in the canvas, >= 0
    uint32_t fpx[2];     // colour mode: the frame pixel's px bytes
    uint32_t pat[3][4];  // colour mode: the 16 bytes of a frame share at phase (16 * m) % px, m = 0..2
};
hipError_t launch_pad(const PadArgs& a, int px, int mode, int n, hipStream_t s);

// ---- plans (ik_plan.cpp) ----
// axis_weights, required_slots and the tables themselves: ik_resize_plan.h
ResizePlan* get_resize_plan(int device, int W, int H, int C, int nw, int nh, int filter, int n);
// the plan of a window (x0, y0, nw, nh) of the source resampled to iw x ih
ResizePlan* get_resize_plan_window(int device, int W, int H, int C, int iw, int ih, int x0, int y0, int nw, int nh,
                                   int filter, int n);

}  // namespace ik
