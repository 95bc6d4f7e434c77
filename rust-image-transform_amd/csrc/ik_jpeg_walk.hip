// ik_jpeg_walk.hip -- gfx950 kernel of the JPEG marker walk over files in device
// memory (ik_transform_batch_submit_device): one wave per file.  The walk itself is
// ik_jpeg_walk.h, shared with the host entry ik_jpeg_walk_host; here the wave's
// lanes hop together (every lane reads the same marker bytes), copy the kept
// segments a byte per lane, and search the last EOI 64 positions at a time.
#include "ik_internal.h"
#include "ik_jpeg_walk.h"

namespace ik {
using namespace jwalk;

namespace {

struct WaveOps {
    int lane;
    __device__ __forceinline__ void copy(uint8_t* dst, const uint8_t* src, uint64_t n) {
        for (uint64_t i = (uint64_t)lane; i < n; i += 64) dst[i] = src[i];
    }
    // positions hi, hi - 1, ... in groups of 64, lane k at hi - k: the first group
    // with a hit holds the answer at its lowest hitting lane
    __device__ __forceinline__ uint64_t last_eoi(const uint8_t* f, uint64_t lo, uint64_t hi) {
        for (uint64_t top = hi;; top -= 64) {
            const bool in = top - lo >= (uint64_t)lane;  // top - lane >= lo
            const bool hit = in && eoi_at(f, top - (uint64_t)lane);
            const unsigned long long mask = __ballot(hit);
            if (mask) return top - (uint64_t)(__ffsll(mask) - 1);
            if (top - lo < 64) return kNoEoi;
        }
    }
};

}  // namespace

// files / lens: the (address, length) table of the batch's JPEG files; skel: a slot
// of kSlot bytes per file; recs: a record per file (both in pinned host memory)
__global__ __launch_bounds__(64) void k_jpeg_walk(const uint64_t* __restrict__ files, const uint64_t* __restrict__ lens,
                                                  uint8_t* __restrict__ skel, Rec* __restrict__ recs) {
    const int f = (int)blockIdx.x;
    WaveOps ops{(int)threadIdx.x};
    Rec r;
    walk_file(reinterpret_cast<const uint8_t*>((uintptr_t)files[f]), lens[f], skel + (size_t)kSlot * f, r, ops);
    if (threadIdx.x == 0) recs[f] = r;
}

hipError_t launch_jpeg_walk(const uint64_t* files, const uint64_t* lens, int n, uint8_t* skel, void* recs,
                            hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_jpeg_walk, dim3((unsigned)n), dim3(64), 0, s, files, lens, skel, reinterpret_cast<Rec*>(recs));
    return hipGetLastError();
}

}  // namespace ik
