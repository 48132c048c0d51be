// rm_kernel_units.hpp -- where the kernels of rm_prep / rm_finalize / rm_noise / rm_scores / rm_rowtopk.hpp are compiled: in the
// kernel units (rm_kernel_units.hip), never in the translation unit that launches them.
//
// Each of the five headers ends with the lists of its templates' instantiations, one per precision (RM_<NAME>_KERNELS_F32 / _F64,
// taking X; rm_scores / rm_rowtopk.hpp also _HALF: fp32 with 16-bit scores in, rm_prep.hpp: with 16-bit factors in), and declares every list `extern template` itself; a kernel unit expands the same list into the definitions, so a
// declaration cannot exist without its definition.  The kernels that are no templates have their bodies under
// RM_PREP_PLAIN_KERNELS / RM_NOISE_PLAIN_KERNELS, which one unit defines; everywhere else they are declarations.  A launch of an
// instantiation that no list names is an undefined symbol when the library is linked (build.py links with --no-undefined).
#pragma once

#define RM_EXTERN_KERNEL(...) extern template __global__ decltype(__VA_ARGS__) __VA_ARGS__;
#define RM_DEFINE_KERNEL(...) template __global__ decltype(__VA_ARGS__) __VA_ARGS__;
