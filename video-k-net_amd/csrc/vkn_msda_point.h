// vkn_msda_point.h — what the forward (vkn_msda.hip) and the backward (vkn_msda_bwd.hip) of the deformable-attention sampling core
// share, so that the two cannot drift apart: the levels' table, the host-side envelope, and the arithmetic of ONE sampling point —
// its pixel coordinates, the test that decides whether it counts, its four clamped corners and its bilinear fractions.
//
// Safety (the headers' contract): a point is tested with the four float comparisons FIRST; a point that fails them has its
// coordinates replaced by 0 before floor / float -> int, its corners are clamped into the level before an address is formed, and
// whatever is loaded for a corner outside is dropped by a select (never multiplied by a zero weight: 0 * inf would be a NaN).
// Every corner index therefore lies inside the level's [H][W] block whatever the offsets hold.
#pragma once
#include "../../include/vkn_msda.h"
#include "vkn_common.h"

namespace msda {

struct Levels {
    int H[VKN_MSDA_MAX_LEVELS], W[VKN_MSDA_MAX_LEVELS], start[VKN_MSDA_MAX_LEVELS];
};

// One point of one level: `ok` = it passes the four comparisons; (xa, ya) .. (xb, yb) its corners, clamped into the level; in1 .. in4
// whether corner (ya, xa), (ya, xb), (yb, xa), (yb, xb) counts (the point is ok AND the corner lies inside); lw, lh the fractions
// towards xb, yb and hw = 1 - lw, hh = 1 - lh.
struct Point {
    bool ok, in1, in2, in3, in4;
    int xa, xb, ya, yb;
    float lw, lh, hw, hh;
};

__device__ __forceinline__ Point point(float rx, float ry, float ox, float oy, int H, int W) {
    const float Hf = (float)H, Wf = (float)W;
    const float x = (rx + ox / Wf) * Wf - 0.5f, y = (ry + oy / Hf) * Hf - 0.5f;
    Point p;
    p.ok = (y > -1.f) && (x > -1.f) && (y < Hf) && (x < Wf);                            // false for a NaN
    const float xs = p.ok ? x : 0.f, ys = p.ok ? y : 0.f;                               // in (-1, W) x (-1, H) from here on
    const float xf = floorf(xs), yf = floorf(ys);
    const int x0 = (int)xf, y0 = (int)yf;                                               // in [-1, W - 1], [-1, H - 1]
    p.lw = xs - xf, p.lh = ys - yf, p.hw = 1.f - p.lw, p.hh = 1.f - p.lh;
    const bool xa_in = x0 >= 0, xb_in = x0 + 1 <= W - 1, ya_in = y0 >= 0, yb_in = y0 + 1 <= H - 1;
    p.xa = x0 < 0 ? 0 : x0, p.xb = x0 + 1 > W - 1 ? W - 1 : x0 + 1;                     // clamped: inside the level in any case
    p.ya = y0 < 0 ? 0 : y0, p.yb = y0 + 1 > H - 1 ? H - 1 : y0 + 1;
    p.in1 = p.ok && ya_in && xa_in, p.in2 = p.ok && ya_in && xb_in, p.in3 = p.ok && yb_in && xa_in, p.in4 = p.ok && yb_in && xb_in;
    return p;
}

__device__ __forceinline__ f32x4 pick(bool keep, const float* p) {
    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    return keep ? v : z;
}

// Host side, before any launch: counts <= 0 / a row stride shorter than its row / an empty level -> VKN_E_ARG, then the envelope of
// include/vkn_msda.h -> VKN_E_SHAPE.  ld_off, ld_logits: the row strides of the offsets (>= 2 M L P) and of the logits (>= M L P), of the
// inputs or of their gradients.  Fills the levels' table and S = sum_l H_l W_l.  `shapes` must not be NULL.
inline int check(const int* shapes, int B, int Q, int M, int D, int L, int P, long long ld_off, long long ld_logits, Levels* lv, long long* S_out) {
    if (B <= 0 || Q <= 0 || M <= 0 || D <= 0 || L <= 0 || P <= 0) return VKN_E_ARG;
    const long long mlp = (long long)M * L * P;
    if (ld_off < 2 * mlp || ld_logits < mlp) return VKN_E_ARG;
    const int nl = L < VKN_MSDA_MAX_LEVELS ? L : VKN_MSDA_MAX_LEVELS;
    for (int l = 0; l < nl; ++l)
        if (shapes[2 * l] <= 0 || shapes[2 * l + 1] <= 0) return VKN_E_ARG;
    if (D != 16 && D != 32 && D != 64) return VKN_E_SHAPE;
    if (((long long)M * D) % 32 != 0 || (long long)M * D > VKN_MSDA_MAX_CHANNELS) return VKN_E_SHAPE;
    if (L > VKN_MSDA_MAX_LEVELS || P > VKN_MSDA_MAX_POINTS) return VKN_E_SHAPE;
    const long long lim = 1ll << 31;
    *lv = Levels{};
    long long S = 0;
    for (int l = 0; l < L; ++l) {
        lv->H[l] = shapes[2 * l];
        lv->W[l] = shapes[2 * l + 1];
        lv->start[l] = (int)S;
        S += (long long)lv->H[l] * lv->W[l];
        if (S * 4 >= lim) return VKN_E_SHAPE;
    }
    const long long C = (long long)M * D, rows = (long long)B * Q;
    if (rows >= lim || (long long)B * S * C * 4 >= lim || rows * C * 4 >= lim || rows * ld_off * 4 >= lim || rows * ld_logits * 4 >= lim ||
        (long long)Q * L * 2 * 4 >= lim)
        return VKN_E_SHAPE;
    *S_out = S;
    return VKN_OK;
}

}  // namespace msda
