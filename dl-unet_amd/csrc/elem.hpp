// elem.hpp — element access shared by the HBM-bound kernels (direct.hip, multiclass.hip): 4 consecutive channels of an
// activation tensor stored as fp32 (16 B) or bf16 (8 B, arithmetic mode 2), read / written as 4 floats, and the grid size of
// a grid-stride launch.
#pragma once
#include "common.hpp"

namespace unet {

typedef float float4_ __attribute__((ext_vector_type(4)));
typedef unsigned short bf16_t;          // storage type of arithmetic mode 2: bf16 bit patterns

// 4 consecutive channels of a tensor stored as T (float: 16 B, bf16: 8 B), as floats
__device__ __forceinline__ float4_ load4(const float *p) { return *(const float4_ *)p; }
__device__ __forceinline__ float4_ load4(const bf16_t *p)
{
    const uint2 w = *(const uint2 *)p;
    return float4_{__builtin_bit_cast(float, w.x << 16), __builtin_bit_cast(float, w.x & 0xffff0000u),
                   __builtin_bit_cast(float, w.y << 16), __builtin_bit_cast(float, w.y & 0xffff0000u)};
}
__device__ __forceinline__ void put1(float *p, float v) { *p = v; }
__device__ __forceinline__ void put1(bf16_t *p, float v) { *p = __builtin_bit_cast(bf16_t, (__bf16)v); }
__device__ __forceinline__ void store4(float *p, float4_ v) { *(float4_ *)p = v; }
__device__ __forceinline__ void store4(bf16_t *p, float4_ v)
{
    uint2 w;
    w.x = (unsigned)__builtin_bit_cast(bf16_t, (__bf16)v[0]) | ((unsigned)__builtin_bit_cast(bf16_t, (__bf16)v[1]) << 16);
    w.y = (unsigned)__builtin_bit_cast(bf16_t, (__bf16)v[2]) | ((unsigned)__builtin_bit_cast(bf16_t, (__bf16)v[3]) << 16);
    *(uint2 *)p = w;
}

static inline int grid_for(size_t total, int per_block = 256, int cap = 8192)
{
    size_t g = (total + per_block - 1) / per_block;
    return (int)(g < 1 ? 1 : (g > (size_t)cap ? cap : g));
}

}  // namespace unet
