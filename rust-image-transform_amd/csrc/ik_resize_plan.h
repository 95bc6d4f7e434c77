// ik_resize_plan.h -- the host half of a resize plan that needs no device: the
// sample.rs weights, the choice of kernel variant (slots, rows, flush, weights in
// LDS or global, periodic or not) and every table the resize kernels read, as
// plain vectors.  build_resize_plan (ik_plan.cpp) uploads them; the CPU model
// (ik_resize_model.cpp, test infrastructure) walks them.  Host code only.
//
// A plan is made for a window (x0, y0, nw, nh) of the source resampled to a virtual
// iw x ih (fit=cover's crop; a whole resize is the full window): the tables hold the
// window's output rows and columns only, indexed from 0, with absolute source
// positions, so the kernels compute and read nothing the crop would discard.
//
// Weights follow image 0.25.8 src/imageops/sample.rs (vertical_sample /
// horizontal_sample, called from reference src/transform.rs:85-89): per output
// index, centre (o + 0.5) * ratio, support * max(ratio, 1), window
// [floor(c - s), ceil(c + s)) clamped, kernel((i - (c - 0.5)) / sratio),
// normalised by the sequential f32 sum (w /= sum).  They are computed once per
// geometry on the host -- with glibc sinf/expf, as rustc's f32::sin/exp are --
// and uploaded, so the device kernels only multiply and add.  Compile with
// -ffp-contract=off: the reference's f32 arithmetic is never contracted.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace ik {

constexpr int kThreads = 256;            // workgroup size (4 wave64s)
constexpr int kBytesPerLane = 8;         // vertical pass: bytes of a source row per lane
constexpr int kStripBytes = kBytesPerLane * kThreads;  // 2048 source bytes per strip
constexpr int kRowWords = kStripBytes + kStripBytes / 8;  // LDS f32 row, +4 words per 32
constexpr int kMaxFlushRows = 4;         // vertical rows staged in LDS per horizontal pass (plan: 2..4)
constexpr int kMaxStripCols = 512;       // output columns per strip (LDS offset/count tables)
constexpr int kMaxStripWeights = 4096;   // horizontal weights per strip kept in LDS (16 KB: an RGB Lanczos3 8x strip's 85 x 48)
// k_resize_periodic's band plan aims at kPerTargetWG workgroups, bands >= kPerMinBand rows
constexpr int kPerTargetWG = 4096, kPerMinBand = 32;

// the (A accumulators, R rows per step) pairs k_resize_periodic is compiled for
#define IK_PERIODIC_INSTANCES(X) X(2, 2) X(2, 4) X(2, 8) X(4, 2) X(4, 4) X(4, 8) X(6, 2) X(6, 4) X(6, 8)

inline bool periodic_instance(int A, int R) {
#define IK_PER_HAS(A_, R_) if (A == A_ && R == R_) return true;
    IK_PERIODIC_INSTANCES(IK_PER_HAS)
#undef IK_PER_HAS
    return false;
}

// dynamic LDS of the fused and periodic kernels, in f32 words:
// [flush rows][strip weights if in LDS][column offsets][lds_pad zero words]
inline size_t resize_lds_words(int flush, bool wl, int max_strip_weights, int max_strip_cols, int lds_pad) {
    return (size_t)flush * kRowWords + (wl ? (size_t)max_strip_weights : 0) + (size_t)max_strip_cols +
           (size_t)lds_pad;
}
// word of strip byte i in an LDS row (4 pad words per 32; the kernels' lds_idx)
inline int resize_lds_idx(int i) { return i + ((i >> 5) << 2); }

namespace rplan {

constexpr float kPi = 3.14159265358979323846264338327950288f;

inline float sinc(float t) {
    const float a = t * kPi;
    if (t == 0.0f) return 1.0f;
    return sinf(a) / a;
}

inline float kernel_eval(int filter, float x) {
    const float ax = fabsf(x);
    switch (filter) {
    case 0: return 1.0f;                                   // box_kernel (Nearest)
    case 1: return ax < 1.0f ? 1.0f - ax : 0.0f;           // triangle_kernel
    case 2: {                                              // catmullrom = bc_cubic_spline(x, 0, 0.5)
        const float b = 0.0f, c = 0.5f;
        float k;
        if (ax < 1.0f) {
            const float a2 = ax * ax, a3 = a2 * ax;
            k = (12.0f - 9.0f * b - 6.0f * c) * a3 + (-18.0f + 12.0f * b + 6.0f * c) * a2 +
                (6.0f - 2.0f * b);
        } else if (ax < 2.0f) {
            const float a2 = ax * ax, a3 = a2 * ax;
            k = (-b - 6.0f * c) * a3 + (6.0f * b + 30.0f * c) * a2 + (-12.0f * b - 48.0f * c) * ax +
                (8.0f * b + 24.0f * c);
        } else {
            k = 0.0f;
        }
        return k / 6.0f;
    }
    case 3: {                                              // gaussian_kernel = gaussian(x, 0.5)
        const float r = 0.5f;
        const float cst = 1.0f / (sqrtf(2.0f * kPi) * r);
        return cst * expf(-(x * x) / (2.0f * (r * r)));
    }
    default:                                               // lanczos3_kernel
        return ax < 3.0f ? sinc(x) * sinc(x / 3.0f) : 0.0f;
    }
}

inline float support_of(int filter) {
    switch (filter) {
    case 0: return 0.0f;
    case 1: return 1.0f;
    case 2: return 2.0f;
    default: return 3.0f;
    }
}

}  // namespace rplan

// sample.rs weights for outputs [o0, o0 + out) of an axis resampled from `in` to
// `virt` samples (the window of a cropped output: O(out) work however large virt
// is); left stays an absolute source position.  Returns the tap count T (row
// stride of w) of those outputs.
inline int axis_weights_window(int in, int virt, int o0, int out, int filter, std::vector<int>& left,
                               std::vector<int>& cnt, std::vector<float>& w) {
    const float ratio = (float)in / (float)virt;
    const float sratio = ratio < 1.0f ? 1.0f : ratio;
    const float src_support = rplan::support_of(filter) * sratio;
    left.assign(out, 0);
    cnt.assign(out, 0);
    std::vector<std::vector<float>> rows(out);
    int T = 1;
    for (int o = 0; o < out; ++o) {
        float c = ((float)(o0 + o) + 0.5f) * ratio;
        long long l = (long long)floorf(c - src_support);
        l = l < 0 ? 0 : (l > in - 1 ? in - 1 : l);
        long long r = (long long)ceilf(c + src_support);
        r = r < l + 1 ? l + 1 : (r > in ? in : r);
        c = c - 0.5f;
        std::vector<float>& ws = rows[o];
        float sum = 0.0f;
        for (long long i = l; i < r; ++i) {
            const float wv = rplan::kernel_eval(filter, ((float)i - c) / sratio);
            ws.push_back(wv);
            sum = sum + wv;
        }
        for (float& wv : ws) wv = wv / sum;
        left[o] = (int)l;
        cnt[o] = (int)(r - l);
        if (cnt[o] > T) T = cnt[o];
    }
    T = (T + 3) & ~3;  // the fused kernel's horizontal pass runs taps in groups
    w.assign((size_t)out * T, 0.0f);
    for (int o = 0; o < out; ++o) std::memcpy(&w[(size_t)o * T], rows[o].data(), sizeof(float) * cnt[o]);
    return T;
}

// sample.rs weights for one whole axis
inline int axis_weights(int in, int out, int filter, std::vector<int>& left, std::vector<int>& cnt,
                        std::vector<float>& w) {
    return axis_weights_window(in, out, 0, out, filter, left, cnt, w);
}

// smallest A with left[r + A] >= left[r] + cnt[r] for every r: no more than A
// output rows are ever open at once in a top-to-bottom sweep
inline int required_slots(const std::vector<int>& left, const std::vector<int>& cnt) {
    const int n = (int)left.size();
    int A = 1;
    for (int r = 0; r < n; ++r) {
        const int end = left[r] + cnt[r];
        while (r + A < n && left[r + A] < end) ++A;
    }
    return A;
}

// Everything build_resize_plan uploads, and the variant the launch picks.
struct ResizeTables {
    int W = 0, H = 0, C = 0, nw = 0, nh = 0, filter = 0, n = 0;
    // the output is columns [x0, x0 + nw) and rows [y0, y0 + nh) of the source resampled
    // to iw x ih (a whole resize: iw = nw, ih = nh, x0 = y0 = 0).  Every table below is
    // indexed by the window's own columns and rows; lx / ly are source positions.
    int iw = 0, ih = 0, x0 = 0, y0 = 0;
    // the source samples per row the window's columns read, [col0, col0 + col_span):
    // what the two-pass kernels' vertical pass covers (a whole resize: 0, W * C)
    int col0 = 0, col_span = 0;
    int slots = 0;        // accumulator slots the fused kernel needs (0 = naive path)
    int rows = 0;         // prefetch depth: max source rows consumed per output row
    bool weights_in_lds = false;
    int flush = 3;        // completed vertical rows staged in LDS per horizontal pass
    int band_h = 0;
    int Tx = 0, Ty = 0;
    std::vector<int> lx, cx, ly, cy;
    std::vector<float> wx, wy;
    std::vector<int> strips;  // [NS*3] (ox0, ox1, first source byte)
    std::vector<int> bands;   // [NB*2] (oy0, oy1)
    std::vector<int> hdr, band_step;           // fused step tables (ResizeArgs)
    std::vector<unsigned long long> smask;
    std::vector<float> sw;
    int per_A = 0, per_R = 0, per_base = 0;    // periodic geometry; per_A = 0: not periodic
    std::vector<float> per_w;
    std::vector<int> per_bands;
    int NS = 0, NB = 0, NBp = 0;
    int max_strip_cols = 0, max_strip_weights = 0;
    int lds_pad = 0;  // zeroed words after the column offsets, so that every padded tap reads inside the launch's LDS
    size_t lds_words() const {
        return resize_lds_words(flush, weights_in_lds, max_strip_weights, max_strip_cols, lds_pad);
    }
};

// First half: weights, variant, strips and the band height (what a plan is cached
// by).  n: images sharing the launch.
inline void resize_plan_head_window(int W, int H, int C, int iw, int ih, int x0, int y0, int nw, int nh, int filter,
                                    int n, ResizeTables& t) {
    t.W = W; t.H = H; t.C = C; t.nw = nw; t.nh = nh; t.filter = filter; t.n = n;
    t.iw = iw; t.ih = ih; t.x0 = x0; t.y0 = y0;
    std::vector<int>&lx = t.lx, &cx = t.cx, &ly = t.ly, &cy = t.cy;
    const int Tx = t.Tx = axis_weights_window(W, iw, x0, nw, filter, lx, cx, t.wx);
    const int Ty = t.Ty = axis_weights_window(H, ih, y0, nh, filter, ly, cy, t.wy);
    int c_lo = W, c_hi = 0;
    for (int ox = 0; ox < nw; ++ox) {
        c_lo = std::min(c_lo, lx[ox]);
        c_hi = std::max(c_hi, lx[ox] + cx[ox]);
    }
    if (nw == iw) { c_lo = 0; c_hi = W; }  // a whole row of outputs: the whole source row, as ever
    t.col0 = c_lo * C;
    t.col_span = (c_hi - c_lo) * C;
    int A = required_slots(ly, cy);
    int slots = A <= 2 ? 2 : A <= 4 ? 4 : A <= 8 ? 8 : A <= 16 ? 16 : 0;

    // prefetch depth: source rows consumed per output row after the first
    int maxblk = 1;
    for (int r = 1; r < nh; ++r) {
        const int b = ly[r] + cy[r] - std::max(ly[r - 1] + cy[r - 1], ly[r]);
        maxblk = std::max(maxblk, b);
    }
    int rows = maxblk <= 4 ? 4 : maxblk <= 8 ? 8 : 16;
    // non-spilling instances: A=4,8 -> R<=8, A=16 -> R=4 (larger blocks
    // take the kernel's chunked path)
    if (slots <= 8 && rows > 8) rows = 8;
    if (slots == 16) rows = 4;
    // column strips: as many output columns as fit kStripBytes source bytes (and,
    // when possible, kMaxStripWeights horizontal weights in LDS)
    bool wl = (long)Tx <= kMaxStripWeights;
    std::vector<int>& strips = t.strips;
    for (int pass = 0; pass < 2 && slots; ++pass) {
        strips.clear();
        bool ok = true;
        for (int ox0 = 0; ox0 < nw;) {
            const int sb = (lx[ox0] * C) & ~127;  // strip rows start on a 128-B line
            int ox1 = ox0;
            while (ox1 < nw && (lx[ox1] + cx[ox1]) * C - sb <= kStripBytes && ox1 - ox0 < kMaxStripCols &&
                   (!wl || (long)(ox1 - ox0 + 1) * Tx <= kMaxStripWeights))
                ++ox1;
            if (ox1 == ox0) { ok = false; break; }  // one output column wider than a strip
            strips.push_back(ox0); strips.push_back(ox1); strips.push_back(sb);
            ox0 = ox1;
        }
        if (!ok) { slots = 0; break; }
        // weights in LDS only when that costs at most ~10% more strips
        if (wl && pass == 0) {
            std::vector<int> keep = strips;
            int ns_wl = (int)strips.size() / 3;
            wl = false;
            strips.clear();
            int ns_gl = 0;
            for (int ox0 = 0; ox0 < nw;) {
                const int sb = (lx[ox0] * C) & ~127;  // strip rows start on a 128-B line
                int ox1 = ox0;
                while (ox1 < nw && (lx[ox1] + cx[ox1]) * C - sb <= kStripBytes && ox1 - ox0 < kMaxStripCols) ++ox1;
                ++ns_gl;
                ox0 = ox1 > ox0 ? ox1 : ox0 + 1;
            }
            if (ns_wl * 10 <= ns_gl * 11) { wl = true; strips = keep; break; }
            continue;  // second pass without the LDS-weights limit
        }
        break;
    }
    const int NS = slots ? (int)strips.size() / 3 : 0;
    // band height depends on how many images share the launch: aim for >= 2048
    // workgroups (8 per CU) without cutting bands below 32 rows
    int band_h = nh;
    if (slots) {
        const long target = 8192;  // measured best on MI355X for 4096^2->512^2 batches (tools/sweep_resize.py)
        long per_img = (target + n - 1) / n;
        long nb = (per_img + NS - 1) / NS;
        if (nb < 1) nb = 1;
        band_h = (int)((nh + nb - 1) / nb);
        // halo rows re-read per band ~ taps - ratio: short filters afford short bands
        const int min_band = Ty <= 20 ? 16 : 32;
        if (band_h < min_band) band_h = min_band;
        band_h = ((band_h + slots - 1) / slots) * slots;
        if (band_h > nh) band_h = nh;
    }
    // flush depth F (vertical rows staged in LDS per horizontal pass): 3 measured
    // best on MI355X for both triangle and lanczos3 8x downscales (deeper costs
    // resident workgroups, shallower runs the barrier-bound horizontal pass more
    // often; tools/sweep_resize.py FLUSH=2,3,4)
    t.flush = 3;
    t.slots = slots; t.rows = rows; t.weights_in_lds = wl; t.NS = NS; t.band_h = band_h;
}

inline void resize_plan_head(int W, int H, int C, int nw, int nh, int filter, int n, ResizeTables& t) {
    resize_plan_head_window(W, H, C, nw, nh, 0, 0, nw, nh, filter, n, t);
}

// Second half: bands, step tables, the periodic tables and the LDS sizes.
inline void resize_plan_tables(ResizeTables& t) {
    const int nh = t.nh, H = t.H, n = t.n, slots = t.slots, rows = t.rows, band_h = t.band_h, Ty = t.Ty, NS = t.NS;
    const std::vector<int>&ly = t.ly, &cy = t.cy;
    const std::vector<float>& wy = t.wy;
    std::vector<int>& bands = t.bands;
    bands.clear();
    for (int y = 0; y < nh; y += band_h) { bands.push_back(y); bands.push_back(y + band_h < nh ? y + band_h : nh); }

    // step tables (see ResizeArgs): per band, output row r needs source rows
    // [max(consumed, ly[r]), ly[r]+cy[r]); cut into steps of <= rows rows, the last
    // step of r emits it.
    std::vector<int>&hdr = t.hdr, &band_step = t.band_step;
    std::vector<unsigned long long>& smask = t.smask;
    std::vector<float>& sw = t.sw;
    hdr.clear(); band_step.clear(); smask.clear(); sw.clear();
    if (slots) {
        for (size_t bi = 0; bi < bands.size(); bi += 2) {
            const int oy0 = bands[bi], oy1 = bands[bi + 1];
            band_step.push_back((int)smask.size());
            int consumed = ly[oy0];
            for (int r = oy0; r < oy1; ++r) {
                const int end = ly[r] + cy[r];
                int st = std::max(consumed, ly[r]);
                do {
                    const int cnt = std::min(rows, std::max(0, end - st));
                    unsigned long long m = 0;
                    std::vector<float> w((size_t)rows * slots, 0.0f);
                    for (int j = 0; j < cnt; ++j)
                        for (int d = 0; d < slots && r + d < oy1; ++d) {
                            const int kk = st + j - ly[r + d];
                            if (kk >= 0 && kk < cy[r + d]) {
                                m |= 1ull << (j * slots + d);
                                w[(size_t)j * slots + d] = wy[(size_t)(r + d) * Ty + kk];
                            }
                        }
                    st += cnt;
                    const int emit = st >= end ? 1 : 0;
                    hdr.push_back(st - cnt); hdr.push_back(cnt); hdr.push_back(emit); hdr.push_back(0);
                    smask.push_back(m);
                    sw.insert(sw.end(), w.begin(), w.end());
                    if (emit) break;
                } while (true);
                consumed = std::max(consumed, end);
            }
            // the kernel runs steps in pairs: pad an odd band with a no-op step
            // (no rows, no taps, no emit; its prefetch re-reads a valid row)
            if ((smask.size() - band_step.back()) & 1) {
                const int last = hdr[hdr.size() - 4];
                hdr.push_back(last); hdr.push_back(0); hdr.push_back(0); hdr.push_back(0);
                smask.push_back(0);
                sw.insert(sw.end(), (size_t)rows * slots, 0.0f);
            }
        }
        band_step.push_back((int)smask.size());
    }

    // Periodic geometry (integer ratio R, every output window inside steps y .. y+A-1
    // of R rows each, step t starting at source row R*t + base): k_resize_periodic
    // sweeps it with A accumulators whose roles rotate at compile time -- no step
    // masks, no accumulator shifts.  Taps outside an output's own window carry weight
    // 0 (+0 added to the sum, so the f32 sequence of the reference is unchanged; the
    // first tap is assigned, not added to 0, which can differ only in the sign of a
    // zero sum and so never in an output byte).  A window keeps the ratio of its
    // virtual height ih; y counts the window's rows, so per_base takes in R * y0.
    int per_A = 0, per_R = 0, per_base = 0;
    std::vector<float>& per_w = t.per_w;
    std::vector<int>& per_bands = t.per_bands;
    per_w.clear(); per_bands.clear();
    if (slots && nh > 0 && t.ih > 0 && H % t.ih == 0) {
        const int R = H / t.ih;
        int lo = 1 << 30, hi = -(1 << 30);
        for (int y = 0; y < nh; ++y) {
            lo = std::min(lo, ly[y] - R * y);
            hi = std::max(hi, ly[y] + cy[y] - R * y);
        }
        const int A = (hi - lo + R - 1) / R;
        if (periodic_instance(A, R)) {
            per_A = A; per_R = R; per_base = lo;
        }
    }
    if (per_A) {
        const int A = per_A, R = per_R, G = A % 2 ? 2 * A : A;  // steps per unrolled group
        // bands: ~kPerTarget workgroups; a band of h rows sweeps h + A - 1 steps,
        // rounded up to whole groups (the extra steps emit nothing)
        long per_img = (kPerTargetWG + n - 1) / n;
        long nb = std::max(1L, (per_img + NS - 1) / NS);
        int h = (int)((nh + nb - 1) / nb);
        h = std::max(h, std::min(nh, kPerMinBand));
        h = ((h + A - 1 + G - 1) / G) * G - (A - 1);  // h + A - 1 a whole number of groups
        if (h < 1) h = std::min(nh, G);
        for (int y = 0; y < nh; y += h) { per_bands.push_back(y); per_bands.push_back(std::min(nh, y + h)); }
        const int nsteps = nh + A - 1 + G;  // the last band's rounding included
        per_w.assign((size_t)nsteps * A * R, 0.0f);
        for (int t2 = 0; t2 < nsteps; ++t2)
            for (int e = 0; e < A; ++e) {
                const int y = t2 - e;
                if (y < 0 || y >= nh) continue;
                for (int j = 0; j < R; ++j) {
                    const int kk = R * t2 + per_base + j - ly[y];
                    if (kk >= 0 && kk < cy[y]) per_w[((size_t)t2 * A + e) * R + j] = wy[(size_t)y * Ty + kk];
                }
            }
    }
    t.per_A = per_A; t.per_R = per_R; t.per_base = per_base;
    t.NB = (int)bands.size() / 2;
    t.NBp = (int)per_bands.size() / 2;
    t.max_strip_cols = 0;
    for (int k = 0; k < NS; ++k) t.max_strip_cols = std::max(t.max_strip_cols, t.strips[3 * k + 1] - t.strips[3 * k]);
    t.max_strip_cols = (t.max_strip_cols + 3) & ~3;
    t.max_strip_weights = (t.max_strip_cols * t.Tx + 3) & ~3;
    // The horizontal pass runs all Tx taps of every column; the zero-weight ones
    // past a column's own count read on past its window: into the next LDS row, or
    // from the last row into the weights and offsets after the rows.  A column with
    // a short window (an image edge) under a long Tx reaches past those too:
    // lds_pad extends the allocation to the furthest word any tap reads (the
    // kernels zero it, with the unused tails of the weights and offsets).
    t.lds_pad = 0;
    long need = 0;
    for (int k = 0; k < NS; ++k) {
        const int sb = t.strips[3 * k + 2];
        for (int ox = t.strips[3 * k]; ox < t.strips[3 * k + 1]; ++ox) {
            long word;
            if (t.C == 3) {
                const int px = t.lx[ox] - sb / 3 + t.Tx - 1;
                word = 3L * px + (px >> 3) + 2;
            } else {
                word = resize_lds_idx(t.lx[ox] * t.C - sb + (t.Tx - 1) * t.C) + t.C - 1;
            }
            need = std::max(need, (long)(t.flush - 1) * kRowWords + word + 1);
        }
    }
    const long nominal = (long)t.lds_words();
    if (need > nominal) t.lds_pad = (int)((need - nominal + 3) & ~3L);
}

inline void build_resize_tables(int W, int H, int C, int nw, int nh, int filter, int n, ResizeTables& t) {
    resize_plan_head(W, H, C, nw, nh, filter, n, t);
    resize_plan_tables(t);
}

inline bool resize_window_ok(long long iw, long long ih, long long x0, long long y0, long long nw, long long nh) {
    return iw >= 1 && ih >= 1 && nw >= 1 && nh >= 1 && x0 >= 0 && y0 >= 0 && x0 + nw <= iw && y0 + nh <= ih &&
           iw <= 0x7FFFFFFFll && ih <= 0x7FFFFFFFll;
}

inline void build_resize_tables_window(int W, int H, int C, int iw, int ih, int x0, int y0, int nw, int nh, int filter,
                                       int n, ResizeTables& t) {
    resize_plan_head_window(W, H, C, iw, ih, x0, y0, nw, nh, filter, n, t);
    resize_plan_tables(t);
}

// The kernel family launch_resize picks (ik_resize_kernel_name): the two-pass
// fallback when the geometry has no fused instance or the image is past the
// buffer descriptor's 32-bit range, else periodic when the plan is and neither
// the FMA mode nor IK_RESIZE_PERIODIC=0 rules it out.
enum ResizeFamily { kFamilyNaive = 0, kFamilyFused = 1, kFamilyPeriodic = 2 };
inline bool resize_fused_fits(size_t src_pitch, size_t H) { return src_pitch * H <= 0x7FFFFFFFull; }
inline int resize_family(int slots, int per_A, int per_R, int flush, size_t src_pitch, size_t H, bool fma,
                         bool periodic_on) {
    if (!(slots > 0 && resize_fused_fits(src_pitch, H))) return kFamilyNaive;
    if (per_A && !fma && flush == 3 && periodic_on && periodic_instance(per_A, per_R)) return kFamilyPeriodic;
    return kFamilyFused;
}

}  // namespace ik
