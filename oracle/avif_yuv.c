/*
 * avif_yuv.c -- ORACLE (test infrastructure only, see ik_oracle.h).
 *
 * Restates the colour conversion in front of the reference's AVIF coder
 * (src/transform.rs:138-146 -> image 0.25.8 AvifEncoder -> to_rgba8 -> ravif
 * 0.11.20, 8-bit BT.601 full-range YCbCr 4:4:4 plus the alpha plane), written
 * from the crate's published formula:
 *
 *   const BT601: [f32; 3] = [0.2990, 0.5870, 0.1140];
 *   scale = 255/255 = 1.0, shift = (255.0 * 0.5).round() = 128.0
 *   y  = scale * m[0] * r + scale * m[1] * g + scale * m[2] * b;
 *   cb = (b * scale - y).mul_add(0.5 / (1. - m[2]), shift);
 *   cr = (r * scale - y).mul_add(0.5 / (1. - m[0]), shift);
 *   (y.round() as u8, cb.round() as u8, cr.round() as u8)
 *
 * All f32; the Y sum left to right and never contracted (the Makefile's
 * -ffp-contract=off), f32::round = roundf (half away from zero), `as u8`
 * saturates.  chroma_fma != 0 is the crate as published (mul_add = one rounding);
 * 0 rounds the product and the sum separately, to count what the fusion changes.
 * Parity unpinned: no copy of the crate exists here to compare against
 * (k_avif_yuv444).
 */
#include <math.h>
#include <stdint.h>

#include "ik_oracle.h"

static uint8_t round_u8(float v) {
    v = roundf(v);
    return (uint8_t)(v < 0.f ? 0.f : (v > 255.f ? 255.f : v));
}

void iko_avif_yuv444(const uint8_t *src, uint32_t npix, uint32_t C, int chroma_fma, uint8_t *y,
                     uint8_t *u, uint8_t *v, uint8_t *a, int *transparent) {
    const float m0 = 0.299f, m1 = 0.587f, m2 = 0.114f, scale = 1.f, shift = 128.f;
    const float kb = 0.5f / (1.f - m2), kr = 0.5f / (1.f - m0);
    int translucent = 0;
    for (uint32_t i = 0; i < npix; ++i) {
        uint8_t px[4];
        iko_to_rgba8(src + (size_t)i * C, 1, C, px);
        const float r = (float)px[0], g = (float)px[1], b = (float)px[2];
        const float Y = scale * m0 * r + scale * m1 * g + scale * m2 * b;
        float cb, cr;
        if (chroma_fma) {
            cb = fmaf(b * scale - Y, kb, shift);
            cr = fmaf(r * scale - Y, kr, shift);
        } else {
            const float pb = (b * scale - Y) * kb, pr = (r * scale - Y) * kr;
            cb = pb + shift;
            cr = pr + shift;
        }
        y[i] = round_u8(Y);
        u[i] = round_u8(cb);
        v[i] = round_u8(cr);
        a[i] = px[3];
        translucent |= px[3] != 255;
    }
    *transparent = translucent;
}
