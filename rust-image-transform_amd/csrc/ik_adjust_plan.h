// ik_adjust_plan.h -- the host plan of a colour adjustment: the six
// numbers of an ik_adjust as a Q16 colour matrix and a tone table, in f64 with the process's
// cos, sin and pow.  Host only, no device; the operations are written one by one in the
// order tests/adjust_model.py restates them (the host code is built with -ffp-contract=off).
#pragma once

#include <cmath>
#include <cstdint>

#include "../../include/imagekit_hip.h"

namespace ik {

constexpr int kAdjustFlagMatrix = 1;  // the matrix is not the identity
constexpr int kAdjustFlagTable = 2;   // the table is not the identity

// the field out of range, or null: every field is fine (written so that a NaN fails)
inline const char* adjust_bad_field(const ik_adjust& a) {
    if (a.brightness < -100 || a.brightness > 100) return "brightness";
    if (a.contrast < -100 || a.contrast > 100) return "contrast";
    if (a.saturation < -100 || a.saturation > 100) return "saturation";
    if (a.hue < -360 || a.hue > 360) return "hue";
    if (!(a.gamma == 0.0f || (a.gamma >= 0.1f && a.gamma <= 10.0f))) return "gamma";
    if (a.invert != 0 && a.invert != 1) return "invert";
    return nullptr;
}

inline bool adjust_is_none(const ik_adjust& a) {
    return !a.brightness && !a.contrast && !a.saturation && !a.hue && a.gamma == 0.0f && !a.invert;
}

// the nine Q16 coefficients, row by row; returns whether they differ from the identity
inline bool adjust_matrix(const ik_adjust& a, int32_t q[9]) {
    const double l[3] = {0.2126, 0.7152, 0.0722};
    const double S[3][3] = {{-l[0], -l[1], 1.0 - l[2]}, {0.143, 0.140, -0.283}, {-(1.0 - l[0]), l[1], l[2]}};
    const double s = 1.0 + (double)a.saturation / 100.0;
    const double th = (double)a.hue * 3.141592653589793 / 180.0;
    const double c = std::cos(th), sn = std::sin(th);
    double sat[3][3], hue[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double d = (i == j ? 1.0 : 0.0) - l[j];
            sat[i][j] = l[j] + s * d;
            hue[i][j] = (l[j] + c * d) + sn * S[i][j];
        }
    bool changed = false;
    for (int i = 0; i < 3; ++i) {
        int32_t off = 0;
        for (int j = 0; j < 3; ++j) {
            if (i == j) continue;
            const double m = (hue[i][0] * sat[0][j] + hue[i][1] * sat[1][j]) + hue[i][2] * sat[2][j];
            q[3 * i + j] = (int32_t)std::floor(m * 65536.0 + 0.5);
            off += q[3 * i + j];
            changed = changed || q[3 * i + j] != 0;
        }
        q[3 * i + i] = 65536 - off;
    }
    return changed;
}

// the M + 1 entries of the tone table (depth 1: 256, depth 2: 65536); returns whether they
// differ from the identity
inline bool adjust_table(const ik_adjust& a, int depth, uint16_t* t) {
    const int M = depth == 1 ? 255 : 65535;
    const double b = (double)a.brightness / 100.0;
    const double k0 = (double)(100 + a.contrast) / 100.0;
    const double k = k0 * k0;
    const double e = a.gamma != 0.0f ? 1.0 / (double)a.gamma : 0.0;
    bool changed = false;
    for (int v = 0; v <= M; ++v) {
        double x = (double)v / (double)M;
        x = x + b;
        x = (x - 0.5) * k + 0.5;
        x = x < 0.0 ? 0.0 : x > 1.0 ? 1.0 : x;
        if (a.gamma != 0.0f) x = std::pow(x, e);
        if (a.invert) x = 1.0 - x;
        t[v] = (uint16_t)std::floor(x * (double)M + 0.5);
        changed = changed || t[v] != v;
    }
    return changed;
}

}  // namespace ik
