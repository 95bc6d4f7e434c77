// ik_blur_plan.h -- the host half of blur and unsharpen: one axis's weight table.
// Needs no device (ik_blur_axis_plan is this function behind the C ABI).
//
// The definition is the project's own, modelled on image 0.25.8's
// imageops::blur as recalled: the resampler's axis_weights (ik_resize_plan.h) at ratio 1
// with a Gaussian of the caller's sigma and a support of 2 * sigma, all in f32, expf from
// the host's libm.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "ik_resize_plan.h"

namespace ik {

constexpr float kBlurMinSigma = 0.0625f;  // below it sigma * sigma and the one-tap case leave f32's comfort
constexpr float kBlurMaxSigma = 32.0f;    // IK_BLUR_MAX_SIGMA: 129 taps, the widest halo the kernel's tile holds

// a sigma a blur can run with (0, "off", is not one); false for NaN
inline bool blur_sigma_ok(float s) { return s >= kBlurMinSigma && s <= kBlurMaxSigma; }

inline float blur_gaussian(float x, float sigma) {
    const float cst = 1.0f / (sqrtf(2.0f * rplan::kPi) * sigma);
    return cst * expf(-(x * x) / (2.0f * (sigma * sigma)));
}

struct BlurAxis {
    int L = 0, T = 1;            // samples; taps of the widest output (row stride of w)
    std::vector<int> left, cnt;  // per output: first source sample, taps
    std::vector<float> w;        // L rows of T weights, zero-padded
    int rl = 0, rr = 0;          // most taps left and right of an output's own sample
    // the interior run [u_lo, u_hi) whose (left - o, cnt, weights) are bit-identical: the
    // kernel reads row u_lo for all of it (u_lo == u_hi: no run)
    int u_lo = 0, u_hi = 0, u_dl = 0, u_cnt = 0;
};

inline void blur_axis_weights(int L, float sigma, BlurAxis& a) {
    const float support = 2.0f * sigma;
    a.L = L;
    a.left.assign(L, 0);
    a.cnt.assign(L, 0);
    std::vector<std::vector<float>> rows(L);
    a.T = 1;
    a.rl = a.rr = 0;
    for (int o = 0; o < L; ++o) {
        float c = (float)o + 0.5f;
        long long l = (long long)floorf(c - support);
        l = l < 0 ? 0 : (l > L - 1 ? L - 1 : l);
        long long r = (long long)ceilf(c + support);
        r = r < l + 1 ? l + 1 : (r > L ? L : r);
        c = c - 0.5f;
        std::vector<float>& ws = rows[o];
        float sum = 0.0f;
        for (long long i = l; i < r; ++i) {
            const float wv = blur_gaussian((float)i - c, sigma);
            ws.push_back(wv);
            sum = sum + wv;
        }
        for (float& wv : ws) wv = wv / sum;
        a.left[o] = (int)l;
        a.cnt[o] = (int)(r - l);
        if (a.cnt[o] > a.T) a.T = a.cnt[o];
        if (o - (int)l > a.rl) a.rl = o - (int)l;
        if ((int)r - 1 - o > a.rr) a.rr = (int)r - 1 - o;
    }
    a.w.assign((size_t)L * a.T, 0.0f);
    for (int o = 0; o < L; ++o) std::memcpy(&a.w[(size_t)o * a.T], rows[o].data(), sizeof(float) * a.cnt[o]);
    // the run around the middle output
    const int m = L / 2;
    auto same = [&](int o) {
        return a.left[o] - o == a.left[m] - m && a.cnt[o] == a.cnt[m] &&
               !std::memcmp(&a.w[(size_t)o * a.T], &a.w[(size_t)m * a.T], sizeof(float) * a.T);
    };
    int lo = m, hi = m + 1;
    while (lo > 0 && same(lo - 1)) --lo;
    while (hi < L && same(hi)) ++hi;
    a.u_lo = lo;
    a.u_hi = hi;
    a.u_dl = m - a.left[m];
    a.u_cnt = a.cnt[m];
}

}  // namespace ik
