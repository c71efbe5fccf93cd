// What the Winograd F(4, 3) kernels (wino3.hip: 16x16 and larger grids, wino3o.hip: 8x8 grids) share: the two transforms, whose order of
// operations is part of the layers' bits, and the hand-over of a wave's accumulators to the inverse transform.  (The tile order, the group
// lookup and the split are those of every conv kernel: device_common.h.  wino.hip's F(4, 5) transforms have one user and live there.)
#pragma once
#include "device_common.h"

namespace p2p {

// BT of F(4, 3) at the points {0, 1, -1, 2, -2, inf}, per channel of a quad: integer coefficients, the order of operations is fixed.
__device__ __forceinline__ void f43_input_transform(const f32x4 (&d)[6], f32x4 (&v)[6])
{
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float d0 = d[0][e], d1 = d[1][e], d2 = d[2][e], d3 = d[3][e], d4 = d[4][e], d5 = d[5][e];
        const float a12 = __builtin_fmaf(-4.f, d2, d4), b12 = __builtin_fmaf(-4.f, d1, d3);
        const float a34 = d4 - d2, b34 = 2.f * (d3 - d1);
        v[0][e] = __builtin_fmaf(4.f, d0, __builtin_fmaf(-5.f, d2, d4));
        v[1][e] = a12 + b12; v[2][e] = a12 - b12;
        v[3][e] = a34 + b34; v[4][e] = a34 - b34;
        v[5][e] = __builtin_fmaf(4.f, d1, __builtin_fmaf(-5.f, d3, d5));
    }
}

// AT of F(4, 3): rows (1 1 1 1 1 0), (0 1 -1 2 -2 0), (0 1 1 4 4 0), (0 1 -1 8 -8 1) -- six position sums to four output columns.
__device__ __forceinline__ void f43_inverse(const f32x4 (&m)[6], f32x4 (&y)[4])
{
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float s12 = m[1][e] + m[2][e], d12 = m[1][e] - m[2][e];
        const float s34 = m[3][e] + m[4][e], d34 = m[3][e] - m[4][e];
        y[0][e] = (m[0][e] + s12) + s34;
        y[1][e] = __builtin_fmaf(2.f, d34, d12);
        y[2][e] = __builtin_fmaf(4.f, s34, s12);
        y[3][e] = __builtin_fmaf(8.f, d34, d12) + m[5][e];
    }
}

// One m-tile of a wave's accumulators (the two 32-channel halves c0, c1 of position j) into an exchange image [position][pair 32][XLD floats].
// C/D layout of the 32x32 MFMA with U as the A operand: row = channel (r & 3) + 8 (r >> 2) + 4 lk of the half, column li = pair.
template <int XLD>
__device__ __forceinline__ void exchange_store(float* X, int j, int li, int lk, const f32x16& c0, const f32x16& c1)
{
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const f32x16& a = c ? c1 : c0;
            const f32x4 v = {a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]};
            *reinterpret_cast<f32x4*>(X + (j * 32 + li) * XLD + c * 32 + 8 * q + 4 * lk) = v;
        }
}

}  // namespace p2p
