// fp32 sweep, up to 64 factors, LDS lists, three item sub-tiles per step (12 waves per block): the launcher of ONE specialisation
// (RM_SPEC, rm_sweep.hpp k_sweep SPEC); every specialisation is a translation unit of its own so that they compile in parallel.
#include "rm_sweep32_launch.hpp"

#define RM_CAT2(a, b) a##b
#define RM_CAT(a, b) RM_CAT2(a, b)

namespace rm {

int RM_CAT(launch_sweep32_n3_s, RM_SPEC)(bool auc, int NG, dim3 grid, size_t lds, hipStream_t stream, const SweepArgs &sa)
{
    return auc ? launch_small<true, false, LM_LDS, 3, false, RM_SPEC>(NG, grid, lds, stream, sa)
               : launch_small<false, false, LM_LDS, 3, false, RM_SPEC>(NG, grid, lds, stream, sa);
}

} // namespace rm

