// Device-side definitions every convolution kernel shares: the vector types, the out-of-range load offset, the LDS-only barrier, the
// XCD-aware tile order, the object-group lookup, and the two pieces of arithmetic whose bits must not depend on the kernel that runs them --
// the hi/lo f16 split of an activation and the BatchNorm + activation expression of an epilogue.  A route (streaming, batched, halo, fused
// block, Winograd) that calls these cannot diverge from the others in them.
#pragma once
#include "kernels.h"

namespace p2p {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));

// Byte offset no buffer descriptor of these kernels covers: a raw buffer load at it returns zeros (padding pixels, rows past the batch).
constexpr unsigned OOB = 0xFFFFFFF0u;

// Workgroup barrier for LDS traffic only: __syncthreads() carries a release fence, which on gfx950 is s_waitcnt vmcnt(0) -- every global
// STORE of an epilogue would have to reach L2 before the next exchange pass (and, in a persistent loop, before the next tile) could start.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

// XCD-aware tile order: workgroup b runs on XCD b % 8, and every XCD has its own L2.  The nblk tiles of a sweep are cut into eight
// contiguous runs, one per XCD (the first nblk % 8 runs one tile longer); this is the tile workgroup b takes.  Neighbouring tiles -- which
// share operand rows, a weight panel or a V patch -- then run on one XCD at the same time.  Persistent kernels go on from it in steps of nblk.
__device__ __forceinline__ int xcd_first_tile(int nblk, int b)
{
    const int q = nblk >> 3, r = nblk & 7;
    const int xcd = b & 7, idx = b >> 3;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// Mixed-object batches: the group (object) whose run [grp[g].KEY, grp[g + 1].KEY) holds v; KEY = the member the runs are counted in
// (&IgemmGroup::row0, &IgemmGroup::tile0, &WinoGroup::sample0, &WinoGroup::unit0, &ResBlockGroup::sample0).
template <auto KEY, typename G>
__device__ __forceinline__ int group_of(const G* grp, int n_groups, int v)
{
    int g = 0;
    while (g + 1 < n_groups && grp[g + 1].*KEY <= v) ++g;
    return g;
}

// ---- the split of PREC_F16X3: hi = f16(v) toward zero (v_cvt_pkrtz), lo = f16(v - hi) to nearest (the residual is exact in fp32).
//      The only place an activation is converted: every loader, transform and fused epilogue that writes a split operand calls it.
__device__ __forceinline__ void split4(const f32x4 v, uint2& hi, uint2& lo)
{
    const fp16x2 h01 = __builtin_amdgcn_cvt_pkrtz(v[0], v[1]), h23 = __builtin_amdgcn_cvt_pkrtz(v[2], v[3]);
    fp16x2 l01, l23;
    l01[0] = (__fp16)(v[0] - (float)h01[0]); l01[1] = (__fp16)(v[1] - (float)h01[1]);
    l23[0] = (__fp16)(v[2] - (float)h23[0]); l23[1] = (__fp16)(v[3] - (float)h23[1]);
    hi = make_uint2(__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h23));
    lo = make_uint2(__builtin_bit_cast(unsigned, l01), __builtin_bit_cast(unsigned, l23));
}
// The 3-channel pixels of the first layer (conv1.hip): the fourth half of a record is a constant zero, not a value to convert.
__device__ __forceinline__ void split3(const float (&v)[3], uint2& hi, uint2& lo)
{
    const fp16x2 h01 = __builtin_amdgcn_cvt_pkrtz(v[0], v[1]), h2 = __builtin_amdgcn_cvt_pkrtz(v[2], 0.f);
    fp16x2 l01, l2;
    l01[0] = (__fp16)(v[0] - (float)h01[0]); l01[1] = (__fp16)(v[1] - (float)h01[1]);
    l2[0] = (__fp16)(v[2] - (float)h2[0]); l2[1] = (__fp16)0.f;
    hi = make_uint2(__builtin_bit_cast(unsigned, h01), __builtin_bit_cast(unsigned, h2));
    lo = make_uint2(__builtin_bit_cast(unsigned, l01), __builtin_bit_cast(unsigned, l2));
}

// ---- the epilogue expression: folded BatchNorm fmaf(v, scale, shift), plus the residual where the layer has one (a layer without one on a
//      kernel that serves both adds 0: -0 becomes +0 there, on every route alike), then ReLU (NaN-propagating, kernels.h) or LeakyReLU.
//      range_note* stays with the caller: it belongs to what is stored, and raw split-K partial sums skip both.
//      alpha travels by reference: callers pass the kernel parameter (p.alpha), which is then read on the LeakyReLU path only, where the
//      hand-written epilogues read it; keep it so, the kernels' register counts were checked against this form.
__device__ __forceinline__ float act1(float v, int act, const float& alpha)
{
    if (act == ACT_RELU) v = relu_nan(v);
    else if (act == ACT_LEAKY) v = v > 0.f ? v : v * alpha;
    return v;
}
__device__ __forceinline__ float bn_act1(float v, float sc, float sh, int act, const float& alpha) { return act1(fmaf(v, sc, sh), act, alpha); }
__device__ __forceinline__ float bn_act1(float v, float sc, float sh, float r, int act, const float& alpha) { return act1(fmaf(v, sc, sh) + r, act, alpha); }

__device__ __forceinline__ f32x4 bn4(f32x4 v, const f32x4 sc, const f32x4 sh)       // (alone: the tanh / sigmoid heads)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaf(v[e], sc[e], sh[e]);
    return v;
}
__device__ __forceinline__ f32x4 act4(f32x4 v, int act, const float& alpha)
{
    if (act == ACT_RELU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = relu_nan(v[e]);
    } else if (act == ACT_LEAKY) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * alpha;
    }
    return v;
}
__device__ __forceinline__ f32x4 bn_act4(const f32x4 v, const f32x4 sc, const f32x4 sh, int act, const float& alpha) { return act4(bn4(v, sc, sh), act, alpha); }
__device__ __forceinline__ f32x4 bn_act4(f32x4 v, const f32x4 sc, const f32x4 sh, const f32x4 r, int act, const float& alpha)
{
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = fmaf(v[e], sc[e], sh[e]) + r[e];
    return act4(v, act, alpha);
}

}  // namespace p2p
