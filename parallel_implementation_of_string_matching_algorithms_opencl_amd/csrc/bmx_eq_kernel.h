// bmx_eq_kernel.h -- Myers' Eq words built on the fly from a pattern held in registers, for the kernels whose patterns
// differ per lane (bmx_ed_batch_kernel.h, bmx_index_map_kernel.h).  The pattern lies 32 bytes per 8 registers: byte 8k + j
// of a 32-byte half in byte k of register j.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bmx {

// 32 flags: bit 8k + j = (byte k of p[j] == c), c4 = c in all four bytes.
__host__ __device__ __forceinline__ uint32_t ed_batch_eq32(const uint32_t *p, uint32_t c4)
{
    uint32_t eq = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t x = p[j] ^ c4;
        const uint32_t y = ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x | 0x7f7f7f7fu; // bit 7 of a byte clear: the byte of x is 0
        eq |= ~y >> (7 - j);
    }
    return eq;
}

template <typename W>
__host__ __device__ __forceinline__ W ed_batch_eq(const uint32_t *p, uint32_t c4, W mask)
{
    if (sizeof(W) == 4) return (W)ed_batch_eq32(p, c4) & mask;
    return (W)(((uint64_t)ed_batch_eq32(p + 8, c4) << 32) | ed_batch_eq32(p, c4)) & mask;
}

} // namespace bmx
