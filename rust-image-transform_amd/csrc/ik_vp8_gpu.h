// ik_vp8_gpu.h -- launcher of libwebp's segment analysis on the GPU
// (ik_vp8_analysis.hip), the first stage of the exact WebP coder (ik_vp8x.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "ik_vp8.h"

namespace ik {
namespace vp8 {

// libwebp's segment analysis (ik_vp8_analysis.hip): per image the k-means result
struct SegRecord {
    int32_t centers[4];
    int32_t mid;  // AssignSegments' weighted_average
    int32_t nmb;
    unsigned long long alpha_sum, uv_alpha_sum;  // MBAnalyze's accumulators
};
// n images of w x h YUV420 planes (Vp8Args layout) -> alpha/uva per MB, seg per MB
// (the k-means cluster, before SimplifySegments), rec per image
hipError_t launch_vp8_analysis(const uint8_t* yuv, size_t yuv_stride, int n, int w, int h, uint8_t* alpha,
                               uint16_t* uva, uint8_t* seg, SegRecord* rec, hipStream_t s);

// One image of a mixed call (images of different sizes and qualities in one set of
// launches): where its planes lie, its geometry, and where its parts of the call's
// arrays start.  A table of these goes up with the call's other constants.
struct ImgDesc {
    const uint8_t* yuv;  // Y (w*h), U, V ((w+1)/2 * (h+1)/2): anywhere in device memory
    int32_t w, h, mb_w, mb_h;
    uint32_t mb0;        // first index into the per-MB arrays (sized by the sum of mb_w*mb_h)
    uint32_t ep0;        // first index into the per-epoch arrays cnt / ready
    uint32_t bnd0;       // first index into the concatenated epoch bounds (nep + 1 per image)
    uint32_t nep;        // the image's epochs
    uint32_t qtab;       // which of the call's quantiser tables (one per distinct quality)
    int32_t use_derr;    // chroma error diffusion (quality <= 98)
};
static_assert(sizeof(ImgDesc) == 48, "the descriptor table is uploaded as laid out here");
// the analysis over such a table: grid.y = image, grid.x up to max_nmb with an exit past
// the image's own MB count; alpha / uva / seg start at the image's mb0
hipError_t launch_vp8_analysis_mixed(const ImgDesc* imgs, int n, int max_nmb, uint8_t* alpha, uint16_t* uva,
                                     uint8_t* seg, SegRecord* rec, hipStream_t s);

}  // namespace vp8
}  // namespace ik
