// sx_bytes16.hpp -- 16 bytes of an image a lane: one aligned 16-byte load where that is possible, and the bytes classified
// four at a time in their words: equality with a constant and "at least a constant" per byte without carries between the
// bytes, the flag bits of the four words gathered by dot products (gather16; sx_classify.hip does the same for the type
// bits).  170 instructions for the five FASTA classes where a compare and a shift for each byte and class were 340 (round 5).
// The FASTA packer (sx_fasta.hip) and the FASTQ indexer (sx_fastq.hip) name their classes with these.
#pragma once
#include "sx_device.hpp"

namespace sx {

constexpr int kBytes16 = 16;

__device__ __forceinline__ uint32_t eq4(uint32_t w, uint32_t k4) // 0x80 in every byte of w that equals k4's
{
    const uint32_t x = w ^ k4;
    return ~(((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}
__device__ __forceinline__ uint32_t ge4(uint32_t w, uint32_t k4) // 0x80 in every byte of w that is >= k4's (which are < 0x80)
{
    return (w | ((w | 0x80808080u) - k4)) & 0x80808080u;
}
// bit k for byte k of v that equals k4's
__device__ __forceinline__ uint32_t eq16(const uint4 &v, uint32_t k4)
{
    return gather16(eq4(v.x, k4), eq4(v.y, k4), eq4(v.z, k4), eq4(v.w, k4), 7);
}

// The lane's 16 bytes img[i0 .. i0 + 16) in two steps, so that a workgroup can ask for the bytes of several tiles
// before it looks at the first: fetch16 issues the load where one aligned 16-byte load does (everywhere but at the
// image's last bytes, or in an image that does not start on a 16-byte boundary) and says whether it did; where it did
// not, the bytes are read one by one (unpack16: zero from `end` on).
__device__ __forceinline__ bool fetch16(const uint8_t *__restrict__ img, uint64_t i0, uint64_t end, uint4 &v)
{
    if (i0 + kBytes16 <= end && ((uintptr_t)(img + i0) & 15u) == 0) {
        v = *reinterpret_cast<const uint4 *>(img + i0);
        return true;
    }
    return false;
}
__device__ __forceinline__ void unpack16(const uint8_t *__restrict__ img, uint64_t i0, uint64_t end, bool fast, const uint4 &v,
                                         uint32_t (&b)[kBytes16])
{
    if (fast) {
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < kBytes16; ++k) b[k] = (w[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    } else {
#pragma unroll
        for (int k = 0; k < kBytes16; ++k) b[k] = i0 + k < end ? (uint32_t)img[i0 + k] : 0u;
    }
}

} // namespace sx
