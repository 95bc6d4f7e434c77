// ik_resize_model.cpp -- CPU model of the GPU resampler (libik_resizemodel.so,
// TEST INFRASTRUCTURE ONLY; not linked into libimagekit_hip.so).
//
// ikm_resize_plan / ikm_resize_table show the host plan of ik_resize_plan.h (the
// one build_resize_plan uploads) to CPU tests.  ikm_resize_run walks those same
// tables in the kernels' order -- workgroup by workgroup (strip, band, image), the
// vertical pass step by step into A accumulators, completed rows into a model of
// the workgroup's LDS with row_put's layouts, the horizontal pass over all Tx
// taps (zero padding included) -- with every product and sum a separate f32
// operation (compile with -ffp-contract=off).  The LDS model starts every
// workgroup as garbage (NaN) and records which words the kernel writes before the
// horizontal pass reads them, so a padded tap that reads a word nobody wrote, or
// one past the launch's dynamic LDS size, is counted (and turns its sum into NaN).
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "ik_resize_plan.h"

using namespace ik;

namespace {

// a window (x0, y0, nw, nh) of the source resampled to iw x ih; whole: (nw, nh, 0, 0, nw, nh)
struct Win {
    int iw, ih, x0, y0, nw, nh;
};

struct Key {
    int v[11];
    bool operator==(const Key& o) const { return std::memcmp(v, o.v, sizeof v) == 0; }
};
thread_local Key g_key = {{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}};
thread_local ResizeTables g_t;

const ResizeTables* plan_for(int W, int H, int C, const Win& w, int filter, int n) {
    if (C < 1 || C > 4 || W < 1 || H < 1 || n < 1 || filter < 0 || filter > 4) return nullptr;
    if (!resize_window_ok(w.iw, w.ih, w.x0, w.y0, w.nw, w.nh)) return nullptr;
    const Key k = {{W, H, C, w.iw, w.ih, w.x0, w.y0, w.nw, w.nh, filter, n}};
    if (!(k == g_key)) {
        g_t = ResizeTables();
        build_resize_tables_window(W, H, C, w.iw, w.ih, w.x0, w.y0, w.nw, w.nh, filter, n, g_t);
        g_key = k;
    }
    return &g_t;
}
const ResizeTables* plan_for(int W, int H, int C, int nw, int nh, int filter, int n) {
    return plan_for(W, H, C, Win{nw, nh, 0, 0, nw, nh}, filter, n);
}

inline int lds_idx(int i) { return i + ((i >> 5) << 2); }

// clamp(t, 0, 255) then f32::round (half away from zero) -> u8, as the kernels'
inline uint8_t float_nearest_u8(float t) {
    t = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);
    return (uint8_t)roundf(t);
}

enum { kStFamily, kStMaxWord, kStLdsWords, kStUnwritten, kStOutside, kStTableOob, kStMaxPutWord, kStCount };

// one workgroup's LDS: [F rows][s_w if WL][s_off], garbage until written
struct Lds {
    std::vector<float> f;
    std::vector<uint8_t> written;
    size_t words = 0;
    void reset(size_t alloc_words, size_t slack) {
        words = alloc_words;
        f.assign(alloc_words + slack, std::numeric_limits<float>::quiet_NaN());
        written.assign(alloc_words + slack, 0);
    }
    void put(size_t i, float v) { f[i] = v; written[i] = 1; }
    void put_int(size_t i, int v) { std::memcpy(&f[i], &v, 4); written[i] = 1; }
    int get_int(size_t i) const { int v; std::memcpy(&v, &f[i], 4); return v; }
};

struct Run {
    const ResizeTables& t;
    const uint8_t* src;
    size_t pitch;
    uint8_t* dst;
    size_t dst_pitch;
    bool fma;
    int64_t* st;
    Lds lds;
    int ox0 = 0, nox = 0, sb = 0;
    size_t sw_at = 0, soff_at = 0;

    // the 8-byte buffer load of lane `lane` at source row `row` (already clamped):
    // bytes past the descriptor's pitch * H records read as 0
    void load_row(int row, float* p /* [kStripBytes] */) const {
        const size_t records = pitch * (size_t)t.H;
        const int row_bytes = t.W * t.C;
        for (int lane = 0; lane < kThreads; ++lane) {
            const int mybyte = sb + kBytesPerLane * lane;
            const size_t voff = mybyte < row_bytes ? (size_t)mybyte : 0;
            for (int i = 0; i < kBytesPerLane; ++i) {
                const size_t a = voff + (size_t)row * pitch + i;
                p[lane * kBytesPerLane + i] = a < records ? (float)src[a] : 0.0f;
            }
        }
    }

    void begin_workgroup(int strip) {
        ox0 = t.strips[3 * strip]; nox = t.strips[3 * strip + 1] - ox0; sb = t.strips[3 * strip + 2];
        const int F = t.flush;
        lds.reset(t.lds_words(), (size_t)kRowWords + 4 * (size_t)t.Tx * 4 + 64);
        sw_at = (size_t)F * kRowWords;
        soff_at = sw_at + (t.weights_in_lds ? (size_t)t.max_strip_weights : 0);
        for (int c = 0; c < nox; ++c)
            lds.put_int(soff_at + c, t.C == 3 ? t.lx[ox0 + c] - sb / 3 : t.lx[ox0 + c] * t.C - sb);
        for (size_t i = 0; i < (size_t)F * kRowWords; ++i) lds.put(i, 0.0f);
        if (t.weights_in_lds) {
            for (int i = 0; i < nox * t.Tx; ++i) lds.put(sw_at + i, t.wx[(size_t)ox0 * t.Tx + i]);
            for (int i = nox * t.Tx; i < t.max_strip_weights; ++i) lds.put(sw_at + i, 0.0f);
        }
        for (int c = nox; c < t.max_strip_cols + t.lds_pad; ++c) lds.put_int(soff_at + c, 0);
    }

    // row_put: lane by lane, row_put_init's index arithmetic
    void row_put(int slot, const float* v /* [kStripBytes] */) {
        const size_t row = (size_t)slot * kRowWords;
        for (int lane = 0; lane < kThreads; ++lane) {
            const int b0 = kBytesPerLane * lane;
            int lo, hi, phi;
            if (t.C == 3) {
                phi = sb % 3;
                const int x0 = b0 + phi;
                lo = x0 + ((x0 * 2731) >> 16);
                hi = lo + (((b0 % 24) == 16 && phi > 0) ? 1 : 0);
            } else {
                phi = -1;
                lo = hi = lds_idx(b0);
            }
            for (int i = 0; i < kBytesPerLane; ++i) {
                int w;
                if (phi <= 0) w = lo + i;
                else if (phi == 1) w = (i < 7 ? lo : hi) + i;
                else w = (i < 6 ? lo : hi) + i;
                if (w > st[kStMaxPutWord]) st[kStMaxPutWord] = w;
                lds.put(row + w, v[b0 + i]);
            }
        }
    }

    float lds_read(size_t w) {
        if ((int64_t)w > st[kStMaxWord]) st[kStMaxWord] = (int64_t)w;
        if (w >= lds.words) ++st[kStOutside];
        else if (!lds.written[w]) ++st[kStUnwritten];
        return lds.f[w];
    }

    void horizontal(int r0, int nrows) {
        const int C = t.C, Tx = t.Tx;
        for (int q = 0; q < nrows; ++q)
            for (int oxl = 0; oxl < nox; ++oxl) {
                const size_t row = (size_t)q * kRowWords;
                const int base = lds.get_int(soff_at + oxl);
                float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
                for (int k = 0; k < Tx; ++k) {
                    const float wk = t.weights_in_lds ? lds_read(sw_at + (size_t)oxl * Tx + k)
                                                      : t.wx[(size_t)(ox0 + oxl) * Tx + k];
                    size_t at;
                    if (C == 3) {
                        const int px = base + k;
                        at = row + 3 * (size_t)px + (size_t)(px >> 3);
                    } else {
                        at = row + (size_t)lds_idx(base + k * C);
                    }
                    for (int c = 0; c < C; ++c) {
                        const float tv = lds_read(at + c);
                        if (fma) {
                            acc[c] = fmaf(tv, wk, acc[c]);
                        } else {
                            const float prod = tv * wk;
                            acc[c] = acc[c] + prod;
                        }
                    }
                }
                uint8_t* o = dst + (size_t)(r0 + q) * dst_pitch + (size_t)(ox0 + oxl) * C;
                for (int c = 0; c < C; ++c) o[c] = float_nearest_u8(acc[c]);
            }
    }

    void fused(int strip, int band) {
        begin_workgroup(strip);
        const int A = t.slots, R = t.rows, F = t.flush, Hm1 = t.H - 1;
        const int oy0 = t.bands[2 * band], oy1 = t.bands[2 * band + 1];
        const int kb = t.band_step[band], ke = t.band_step[band + 1];
        std::vector<float> acc((size_t)A * kStripBytes, 0.0f), p(kStripBytes);
        int next = oy0;
        for (int k = kb; k < ke; ++k) {
            const int hstart = t.hdr[4 * k], hemit = t.hdr[4 * k + 2];
            const unsigned long long m = t.smask[k];
            const float* w = &t.sw[(size_t)k * R * A];
            for (int j = 0; j < R; ++j) {
                if (!((m >> (j * A)) & ((1ull << A) - 1ull))) continue;
                int row = hstart + j;
                row = row < Hm1 ? row : Hm1;
                load_row(row, p.data());
                for (int d = 0; d < A; ++d) {
                    if (!((m >> (j * A + d)) & 1ull)) continue;
                    const float wt = w[j * A + d];
                    float* a = &acc[(size_t)d * kStripBytes];
                    for (int b = 0; b < kStripBytes; ++b) {
                        if (fma) {
                            a[b] = fmaf(p[b], wt, a[b]);
                        } else {
                            const float prod = p[b] * wt;
                            a[b] = a[b] + prod;
                        }
                    }
                }
            }
            if (hemit) {
                if (next >= oy1) { ++st[kStTableOob]; return; }  // more emits than rows
                row_put((next - oy0) % F, acc.data());
                std::memmove(acc.data(), acc.data() + kStripBytes, sizeof(float) * (size_t)(A - 1) * kStripBytes);
                std::fill(acc.begin() + (size_t)(A - 1) * kStripBytes, acc.end(), 0.0f);
                const int nrows = (next - oy0) % F + 1;
                if (nrows == F || next == oy1 - 1) horizontal(next - nrows + 1, nrows);
                ++next;
            }
        }
    }

    void periodic(int strip, int band) {
        begin_workgroup(strip);
        const int A = t.per_A, R = t.per_R, F = t.flush, Hm1 = t.H - 1, G = A % 2 ? 2 * A : A;
        const int oy0 = t.per_bands[2 * band], oy1 = t.per_bands[2 * band + 1], rb = t.per_base;
        std::vector<float> acc((size_t)A * kStripBytes, 0.0f), p(kStripBytes);
        const int t0 = oy0, t1 = t0 + ((oy1 - oy0 + A - 1 + G - 1) / G) * G;
        for (int s = t0; s < t1; ++s) {
            const int U = (s - t0) % A;
            if ((size_t)(s + 1) * A * R > t.per_w.size()) { ++st[kStTableOob]; return; }
            const float* w = &t.per_w[(size_t)s * A * R];
            for (int j = 0; j < R; ++j) {
                int row = R * s + rb + j;
                row = row < 0 ? 0 : (row < Hm1 ? row : Hm1);
                load_row(row, p.data());
                for (int e = 0; e < A; ++e) {
                    const int slot = (U - e + A) % A;  // the output that started e steps ago
                    const float wt = w[e * R + j];
                    float* a = &acc[(size_t)slot * kStripBytes];
                    for (int b = 0; b < kStripBytes; ++b) {
                        const float prod = p[b] * wt;
                        if (e == 0 && j == 0) a[b] = prod;  // its first tap
                        else a[b] = a[b] + prod;
                    }
                }
            }
            const int y = s - (A - 1);
            if (y >= oy0 && y < oy1) {
                row_put((y - oy0) % F, &acc[(size_t)((U + 1) % A) * kStripBytes]);
                const int nrows = (y - oy0) % F + 1;
                if (nrows == F || y == oy1 - 1) horizontal(y - nrows + 1, nrows);
            }
        }
    }

    // k_vert_naive / k_horz_naive: each output's own taps only, the vertical pass over
    // the byte columns [col0, col0 + col_span) of the plan
    void naive() {
        const int rbts = t.col_span, c0 = t.col0;
        std::vector<float> tmp((size_t)t.nh * rbts, std::numeric_limits<float>::quiet_NaN());
        for (int r = 0; r < t.nh; ++r)
            for (int b = 0; b < rbts; ++b) {
                float v = 0.0f;
                for (int k = 0; k < t.cy[r]; ++k) {
                    const size_t at = (size_t)(t.ly[r] + k) * pitch + c0 + b;
                    if (at >= pitch * (size_t)t.H || c0 + b >= t.W * t.C) { ++st[kStTableOob]; continue; }
                    const float prod = (float)src[at] * t.wy[(size_t)r * t.Ty + k];
                    v = v + prod;
                }
                tmp[(size_t)r * rbts + b] = v;
            }
        for (int r = 0; r < t.nh; ++r)
            for (int v = 0; v < t.nw * t.C; ++v) {
                const int ox = v / t.C, c = v - ox * t.C;
                float acc = 0.0f;
                int idx = t.lx[ox] * t.C + c - c0;
                for (int k = 0; k < t.cx[ox]; ++k, idx += t.C) {
                    if (idx < 0 || idx >= rbts) { ++st[kStTableOob]; continue; }
                    const float prod = tmp[(size_t)r * rbts + idx] * t.wx[(size_t)ox * t.Tx + k];
                    acc = acc + prod;
                }
                dst[(size_t)r * dst_pitch + v] = float_nearest_u8(acc);
            }
    }
};

}  // namespace

static int plan_summary(const ResizeTables* t, int32_t* out, int cap);
static long long plan_table(const ResizeTables* t, int which, void* out, long long cap_bytes);
static int plan_run(const ResizeTables* t, const uint8_t* src, long long pitch, long long src_img_stride, int nimg,
             uint8_t* dst, long long dst_pitch, long long dst_img_stride, int fma, int family, long long* stats);

extern "C" {

// the summary of ik_resize_plan_info's first twelve values, then per_base, band_h,
// max_strip_weights, LDS words of the launch, fused steps, per_w steps, lds_pad
int ikm_resize_plan(int W, int H, int C, int nw, int nh, int filter, int n, int32_t* out, int cap) {
    return plan_summary(plan_for(W, H, C, nw, nh, filter, n), out, cap);
}
// the same for a window (x0, y0, nw, nh) of the source resampled to iw x ih
int ikm_resize_plan_window(int W, int H, int C, int iw, int ih, int x0, int y0, int nw, int nh, int filter, int n,
                           int32_t* out, int cap) {
    return plan_summary(plan_for(W, H, C, Win{iw, ih, x0, y0, nw, nh}, filter, n), out, cap);
}
}  // extern "C"

static int plan_summary(const ResizeTables* t, int32_t* out, int cap) {
    if (!t || !out) return -1;
    const int32_t v[19] = {t->slots, t->rows, t->flush, t->weights_in_lds ? 1 : 0, t->NS, t->NB, t->per_A, t->per_R,
                           t->NBp, t->Tx, t->Ty, t->max_strip_cols, t->per_base, t->band_h, t->max_strip_weights,
                           (int32_t)t->lds_words(), (int32_t)t->smask.size(),
                           t->per_A ? (int32_t)(t->per_w.size() / ((size_t)t->per_A * t->per_R)) : 0, t->lds_pad};
    for (int i = 0; i < 19 && i < cap; ++i) out[i] = v[i];
    return 19;
}

// table `which` of that plan: 0 lx, 1 cx, 2 wx, 3 ly, 4 cy, 5 wy, 6 strips, 7 bands,
// 8 step_hdr, 9 step_mask (u64), 10 step_w, 11 band_step, 12 per_w, 13 per_bands.
// Returns its size in bytes; copies it when cap_bytes suffices.
extern "C" {
long long ikm_resize_table(int W, int H, int C, int nw, int nh, int filter, int n, int which, void* out,
                           long long cap_bytes) {
    return plan_table(plan_for(W, H, C, nw, nh, filter, n), which, out, cap_bytes);
}
long long ikm_resize_table_window(int W, int H, int C, int iw, int ih, int x0, int y0, int nw, int nh, int filter,
                                  int n, int which, void* out, long long cap_bytes) {
    return plan_table(plan_for(W, H, C, Win{iw, ih, x0, y0, nw, nh}, filter, n), which, out, cap_bytes);
}
}  // extern "C"

static long long plan_table(const ResizeTables* t, int which, void* out, long long cap_bytes) {
    if (!t) return -1;
    const void* p = nullptr;
    size_t bytes = 0;
#define IKM_TAB(I, V) case I: p = t->V.data(); bytes = t->V.size() * sizeof(t->V[0]); break;
    switch (which) {
        IKM_TAB(0, lx) IKM_TAB(1, cx) IKM_TAB(2, wx) IKM_TAB(3, ly) IKM_TAB(4, cy) IKM_TAB(5, wy) IKM_TAB(6, strips)
        IKM_TAB(7, bands) IKM_TAB(8, hdr) IKM_TAB(9, smask) IKM_TAB(10, sw) IKM_TAB(11, band_step) IKM_TAB(12, per_w)
        IKM_TAB(13, per_bands)
    default: return -1;
    }
#undef IKM_TAB
    if (out && bytes && (long long)bytes <= cap_bytes) std::memcpy(out, p, bytes);
    return (long long)bytes;
}

// nimg images of the plan for (geometry, n) resized on the CPU in the kernels'
// order.  family: -1 what the launch picks in the exact mode (periodic when the
// plan is), 1 k_resize_fused also on a periodic geometry (as the FMA mode and
// IK_RESIZE_PERIODIC=0 do), 0 the two-pass fallback.  fma: one fused multiply-add
// per tap (fused family only).  stats (7 values, may be null): family run, highest
// LDS word the horizontal pass read, LDS words of the launch, reads of words the
// workgroup never wrote, reads past the launch's LDS, table indices out of range,
// highest word row_put wrote within a row.
extern "C" {
int ikm_resize_run(const uint8_t* src, long long pitch, long long src_img_stride, int W, int H, int C, int nw, int nh,
                   int filter, int n, int nimg, uint8_t* dst, long long dst_pitch, long long dst_img_stride, int fma,
                   int family, long long* stats) {
    return plan_run(plan_for(W, H, C, nw, nh, filter, n), src, pitch, src_img_stride, nimg, dst, dst_pitch,
                    dst_img_stride, fma, family, stats);
}
// the same over a window: dst receives nw x nh pixels per image
int ikm_resize_run_window(const uint8_t* src, long long pitch, long long src_img_stride, int W, int H, int C, int iw,
                          int ih, int x0, int y0, int nw, int nh, int filter, int n, int nimg, uint8_t* dst,
                          long long dst_pitch, long long dst_img_stride, int fma, int family, long long* stats) {
    return plan_run(plan_for(W, H, C, Win{iw, ih, x0, y0, nw, nh}, filter, n), src, pitch, src_img_stride, nimg, dst,
                    dst_pitch, dst_img_stride, fma, family, stats);
}
}  // extern "C"

static int plan_run(const ResizeTables* t, const uint8_t* src, long long pitch, long long src_img_stride, int nimg,
             uint8_t* dst, long long dst_pitch, long long dst_img_stride, int fma, int family, long long* stats) {
    if (!t || !src || !dst || pitch < (long long)t->W * t->C || dst_pitch < (long long)t->nw * t->C || nimg < 1)
        return -1;
    int fam = family;
    if (fam < 0) fam = !t->slots ? kFamilyNaive : (t->per_A ? kFamilyPeriodic : kFamilyFused);
    if (fam == kFamilyPeriodic && !t->per_A) return -1;
    if (fam != kFamilyNaive && !t->slots) return -1;
    if (fma && fam == kFamilyPeriodic) return -1;
    int64_t st[kStCount] = {0};
    st[kStFamily] = fam; st[kStMaxWord] = -1; st[kStLdsWords] = (int64_t)t->lds_words(); st[kStMaxPutWord] = -1;
    for (int img = 0; img < nimg; ++img) {
        Run r{*t, src + (size_t)img * src_img_stride, (size_t)pitch, dst + (size_t)img * dst_img_stride,
              (size_t)dst_pitch, fma != 0, st, Lds()};
        if (fam == kFamilyNaive) { r.naive(); continue; }
        const int nb = fam == kFamilyPeriodic ? t->NBp : t->NB;
        for (int band = 0; band < nb; ++band)
            for (int strip = 0; strip < t->NS; ++strip) {
                if (fam == kFamilyPeriodic) r.periodic(strip, band);
                else r.fused(strip, band);
            }
    }
    if (stats)
        for (int i = 0; i < kStCount; ++i) stats[i] = st[i];
    return 0;
}
