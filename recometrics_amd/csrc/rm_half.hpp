// rm_half.hpp -- 16-bit floating point as a SOURCE element type: bit patterns in memory, widened exactly to fp32 in registers.
//
// Two kinds of input may arrive in 16 bits under an fp32 call: the caller's score matrix (rm_scores.hpp: ScoreSrc,
// include/recometrics_hip_half.h) and the factor matrices (rm_prep.hpp: FactorSrc, include/recometrics_hip_half_factors.h).
// bf16 is the upper half of an fp32 (a shift / a mask per value, two values per dword); IEEE binary16 goes through the hardware
// conversion (v_cvt_f32_f16: subnormals become fp32 normals; the build sets no flush flag and fp16 denormals are on by default).
// Nothing is ever computed in 16 bits: behind the widening a value is an fp32 value.
#pragma once
#include "rm_device.hpp"

namespace rm {

struct F16Bits { unsigned short b; };
struct BF16Bits { unsigned short b; };
// the two values of a dword, the one at the lower address first
__device__ __forceinline__ float half_lo(F16Bits, unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)w); }
__device__ __forceinline__ float half_hi(F16Bits, unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }
__device__ __forceinline__ float half_lo(BF16Bits, unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float half_hi(BF16Bits, unsigned w) { return __uint_as_float(w & 0xffff0000u); }

} // namespace rm
