// The halo staging the three halo-tiled kernels (igemm_halo.hip, igemm_halo8.hip, igemm_halo_s2.hip) share: where a thread's float4 of the
// halo goes in LDS, and the split + store that puts it there.  What differs per kernel -- the patch geometry, the pixel a float4 comes from --
// stays in its file.
#pragma once
#include "device_common.h"

namespace p2p {

// LDS byte offsets of a thread's HALO_PASSES float4s, two 16-bit values per register; 0xFFFF = this pass is not part of the halo.
template <int HALO_PASSES>
struct HaloDst {
    unsigned d2[(HALO_PASSES + 1) / 2];
    __device__ __forceinline__ void clear()
    {
#pragma unroll
        for (int j = 0; j < (HALO_PASSES + 1) / 2; ++j) d2[j] = 0xFFFFFFFFu;
    }
    __device__ __forceinline__ void set(int j, unsigned dst) { d2[j >> 1] = (j & 1) ? ((d2[j >> 1] & 0x0000FFFFu) | (dst << 16)) : ((d2[j >> 1] & 0xFFFF0000u) | dst); }
    __device__ __forceinline__ unsigned get(int j) const { return (j & 1) ? (d2[j >> 1] >> 16) : (d2[j >> 1] & 0xFFFFu); }
};

// The loaded float4s of a slice into the halo image: record [hi f16 x32 | lo f16 x32 | pad], this thread's quad at `dst` and 64 bytes on.
template <int HALO_PASSES>
__device__ __forceinline__ void halo_store(char* smem, const HaloDst<HALO_PASSES>& h_dst, const f32x4 (&rh)[HALO_PASSES])
{
#pragma unroll
    for (int j = 0; j < HALO_PASSES; ++j) {
        const unsigned dst = h_dst.get(j);
        if (dst == 0xFFFFu) continue;
        uint2 hi, lo;
        split4(rh[j], hi, lo);
        *reinterpret_cast<uint2*>(smem + dst) = hi;
        *reinterpret_cast<uint2*>(smem + dst + 64) = lo;
    }
}

}  // namespace p2p
