// The one fp32 -> bf16 rounding of the training step (train_bf16.hip, train_bf16_act.hip).
#pragma once
#include "yv3_common.h"

namespace {

// fp32 -> bf16 bits, round to nearest even as torch's conversion: NaN -> the canonical quiet NaN 0x7fc0, subnormals rounded (no flush)
__device__ __forceinline__ u16 rne_bf16(float f) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (u16)0x7fc0;
    return (u16)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

}  // namespace
