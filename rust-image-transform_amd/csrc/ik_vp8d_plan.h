// ik_vp8d_plan.h -- the launch plan of a batch of lossy WebP frames (decode_webp_batch,
// ik_vp8d_host.cpp; exported as ik_webp_batch_plan).  Host only, no HIP: which request
// is placed k-th, the MB-row ticket each placed image starts at, and where the batch is
// cut into sub-launches.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>

namespace ik {
namespace vp8d {

// n images of mb_w[i] x mb_h[i] macroblocks that take bytes[i] of staged + work memory
// (a frame's staged alpha plane included, so the cap holds for RGBA frames too).
//   order[k]      the request placed k-th: largest first, by MB rows, then by MBs, then
//                 by request index, so a launch's last tickets are short rows
//   launch_lo     the first k of each sub-launch, then n (room for n + 1 values): the
//                 placed images in order, cut where the next one would take a
//                 sub-launch past cap_bytes; an image above the cap is alone in its own
//   row_start[k]  the MB rows placed before image k in its sub-launch (the ticket of its
//                 first row; 0 at each launch_lo), row_start[n] the rows of the last
//                 sub-launch; a sub-launch [lo, hi) that is not the last ends at
//                 row_start[hi - 1] + mb_h[order[hi - 1]]
// Returns the sub-launch count (0 for n = 0).
inline int webp_batch_plan(const uint32_t* mb_w, const uint32_t* mb_h, const uint64_t* bytes, uint32_t n,
                           uint64_t cap_bytes, uint32_t* order, uint32_t* row_start, uint32_t* launch_lo) {
    launch_lo[0] = 0;
    row_start[0] = 0;
    if (!n) return 0;
    std::iota(order, order + n, 0u);
    std::sort(order, order + n, [&](uint32_t a, uint32_t b) {
        if (mb_h[a] != mb_h[b]) return mb_h[a] > mb_h[b];
        const uint64_t ma = (uint64_t)mb_w[a] * mb_h[a], mb = (uint64_t)mb_w[b] * mb_h[b];
        if (ma != mb) return ma > mb;
        return a < b;
    });
    int launches = 0;
    uint64_t used = 0;
    uint32_t rows = 0;
    for (uint32_t k = 0; k < n; ++k) {
        const uint64_t need = bytes[order[k]];
        if (k == 0 || need > cap_bytes - std::min(used, cap_bytes)) {  // (the first image of a launch always fits)
            launch_lo[launches++] = k;
            used = 0;
            rows = 0;
        }
        row_start[k] = rows;
        rows += mb_h[order[k]];
        used += need;
    }
    launch_lo[launches] = n;
    row_start[n] = rows;
    return launches;
}

}  // namespace vp8d
}  // namespace ik
