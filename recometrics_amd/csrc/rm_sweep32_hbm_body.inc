// fp32 sweep, up to 128 factors, top-K lists in HBM (replace-the-minimum and append buffers): the launcher of ONE specialisation
// (RM_SPEC).
#include "rm_sweep32_launch.hpp"

#define RM_CAT2(a, b) a##b
#define RM_CAT(a, b) RM_CAT2(a, b)

namespace rm {

int RM_CAT(launch_sweep32_hbm_s, RM_SPEC)(bool auc, int lmode, int NG, dim3 grid, size_t lds, hipStream_t stream, const SweepArgs &sa)
{
    if (lmode == LM_HBM)
        return auc ? launch_small<true, false, LM_HBM, 2, true, RM_SPEC>(NG, grid, lds, stream, sa)
                   : launch_small<false, false, LM_HBM, 2, true, RM_SPEC>(NG, grid, lds, stream, sa);
    return auc ? launch_small<true, false, LM_HBM_APPEND, 2, true, RM_SPEC>(NG, grid, lds, stream, sa)
               : launch_small<false, false, LM_HBM_APPEND, 2, true, RM_SPEC>(NG, grid, lds, stream, sa);
}

} // namespace rm

