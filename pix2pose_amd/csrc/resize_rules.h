// skimage-style bilinear sampling rules shared by every resize on the device (pipeline.hip: the six resizes of est_pose;
// xyz_patch.hip: the training patches): half-pixel centres, floor / ceil taps, numpy-pad 'reflect', skimage's clip=True.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)     // the rules are stated without fused multiply-add; every includer compiles that way

namespace p2p {

struct Tap {
    int i0, i1;
    double d;
};

__device__ inline Tap axis_tap(int o, int n_in, int n_out)
{
    // identity resize (every resize of a 128-px crop): src = o * 1.0 + (0.5 - 0.5) = o exactly -- the same taps and weight without the
    // fp64 division (a quarter of stage2_input_kernel's time at BASELINE.json configs[2])
    if (n_in == n_out) { Tap t; t.i0 = t.i1 = o; t.d = 0.0; return t; }
    const double s = (double)n_in / (double)n_out;
    const double src = (double)o * s + (0.5 * s - 0.5);
    const double lo = floor(src);
    Tap t;
    t.i0 = (int)lo;
    t.i1 = (int)ceil(src);
    t.d = src - lo;
    return t;
}

__device__ inline int reflect_idx(int i, int n)   // numpy-pad 'reflect' (edge sample not repeated)
{
    if (n == 1) return 0;
    const int p = 2 * (n - 1);
    i %= p;
    if (i < 0) i += p;
    return i >= n ? p - i : i;
}

__device__ inline double lerp2(double tl, double tr, double bl, double br, double dr, double dc)
{
    const double top = (1 - dc) * tl + dc * tr;
    const double bot = (1 - dc) * bl + dc * br;
    return (1 - dr) * top + dr * bot;
}

// skimage's clip=True (every version the reference can run on): the warp output is clamped to [min, max] of the warp
// INPUT; in 'constant' mode with cval outside that range, outputs exactly equal to cval are left alone
// (skimage.transform._warps._clip_warp_output).  A no-op unless taps fall outside the image (up-scaling borders) or
// the anti-aliasing filter mixed cval in.
__device__ inline double clip_warp(double v, double lo, double hi, double cval)
{
    if (!(lo <= cval && cval <= hi) && v == cval) return v;
    return v < lo ? lo : (v > hi ? hi : v);
}


// The float32 warp of scikit-image 0.17 / 0.18 (_warp_fast[float32]; derivation at cand_pixel in pipeline.hip)
struct TapF {
    int i0, i1;
    float d;
};

__device__ inline TapF axis_tap_f32(int o, int n_in, int n_out)
{
    if (n_in == n_out) { TapF t; t.i0 = t.i1 = o; t.d = 0.f; return t; }      // ms = 1, mt = 0: src = (float)o exactly
    const double s = (double)n_in / (double)n_out;
    const float ms = (float)s, mt = (float)(s * 0.5 - 0.5);
    const float src = ms * (float)o + mt;            // contraction is off in this file
    const float lo = floorf(src);
    TapF t;
    t.i0 = (int)lo;
    t.i1 = (int)ceilf(src);
    t.d = src - lo;
    return t;
}

__device__ inline float lerp2_f32(float tl, float tr, float bl, float br, float dr, float dc)
{
    const double top = (1.0 - (double)dc) * (double)tl + (double)(dc * tr);
    const double bot = (1.0 - (double)dc) * (double)bl + (double)(dc * br);
    return (float)((1.0 - (double)dr) * top + (double)dr * bot);
}

}  // namespace p2p
