// rm_kernel_units.hip -- the kernels of rm_prep / rm_finalize / rm_noise / rm_scores / rm_rowtopk.hpp, compiled apart from the host
// code that launches them (rm_lib.hip sees them `extern template`, or as declarations, and emits none: rm_kernel_units.hpp).
//
// This file is compiled once per translation unit with -DRM_KERNELS=k, units 3 and 4 once per precision with -DRM_F64=0 / 1
// (recometrics_amd/build.py lists the units; they compile in parallel with the sweeps').  A unit holds nothing but the explicit
// instantiations of its headers' lists and, units 0 and 2, its header's kernels that are no templates.  The cut follows the
// measured compile times (profiles/build_times.txt): k_collect_topk takes more than everything else here together.
//   RM_KERNELS  0  rm_prep.hpp: the plan, operand packing, the positives' scores and the top-K bounds' seeds
//               1  rm_finalize.hpp but k_collect_topk: ranks, AUC, top-K selection, the metrics
//               2  rm_noise.hpp, rm_scores.hpp, rm_rowtopk.hpp: tie noise, the score-matrix entries
//               3  k_collect_topk, lane buffers of 512 and 1024 entries          x fp32 / fp64
//               4  k_collect_topk, lane buffers of 4096 entries                  x fp32 / fp64
//               5  rm_scores.hpp, rm_rowtopk.hpp with 16-bit scores (f16 / bf16 in, fp32 behind the load)
//               6  rm_prep.hpp's readers of raw A / B with 16-bit factors (f16 / bf16 in, fp32 behind the load)
#include <hip/hip_runtime.h>

#if RM_KERNELS == 0
#define RM_PREP_PLAIN_KERNELS
#include "rm_prep.hpp"
#define RM_UNIT_KERNELS(X) RM_PREP_KERNELS_F32(X) RM_PREP_KERNELS_F64(X)
#elif RM_KERNELS == 1
#include "rm_finalize.hpp"
#define RM_UNIT_KERNELS(X) RM_FINALIZE_KERNELS_F32(X) RM_FINALIZE_KERNELS_F64(X)
#elif RM_KERNELS == 2
#define RM_NOISE_PLAIN_KERNELS
#include "rm_noise.hpp"
#include "rm_scores.hpp"
#include "rm_rowtopk.hpp"
#define RM_UNIT_KERNELS(X) RM_NOISE_KERNELS_F32(X) RM_NOISE_KERNELS_F64(X) RM_SCORES_KERNELS_F32(X) RM_SCORES_KERNELS_F64(X) \
                           RM_ROWTOPK_KERNELS_F32(X) RM_ROWTOPK_KERNELS_F64(X)
#elif RM_KERNELS == 3 && !RM_F64
#include "rm_finalize.hpp"
#define RM_UNIT_KERNELS(X) RM_COLLECT_KERNELS_F32(X)
#elif RM_KERNELS == 3
#include "rm_finalize.hpp"
#define RM_UNIT_KERNELS(X) RM_COLLECT_KERNELS_F64(X)
#elif RM_KERNELS == 4 && !RM_F64
#include "rm_finalize.hpp"
#define RM_UNIT_KERNELS(X) RM_COLLECT4096_KERNELS_F32(X)
#elif RM_KERNELS == 4
#include "rm_finalize.hpp"
#define RM_UNIT_KERNELS(X) RM_COLLECT4096_KERNELS_F64(X)
#elif RM_KERNELS == 5
#include "rm_scores.hpp"
#include "rm_rowtopk.hpp"
#define RM_UNIT_KERNELS(X) RM_SCORES_KERNELS_HALF(X) RM_ROWTOPK_KERNELS_HALF(X)
#elif RM_KERNELS == 6
#include "rm_prep.hpp"
#define RM_UNIT_KERNELS(X) RM_PREP_KERNELS_HALF(X)
#else
#error "RM_KERNELS: 0 .. 6"
#endif

namespace rm {
RM_UNIT_KERNELS(RM_DEFINE_KERNEL)
} // namespace rm
