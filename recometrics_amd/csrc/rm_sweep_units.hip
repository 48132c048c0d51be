// rm_sweep_units.hip -- every instantiation of the two sweep kernels, as rows of one table per precision (rm_launch.hpp).
//
// This file is compiled once per translation unit with -DRM_FAMILY=f -DRM_SPEC=s (recometrics_amd/build.py lists the units; they
// compile in parallel), and once without RM_FAMILY: the table itself -- the walk over the units' rows and the rule that turns a
// request into a key.  A unit instantiates its family's kernels for ONE specialisation of the epilogue's run-time switches
// (k_sweep / k_sweep64 SPEC).  The families:
//   fp32  0  up to 64 factors, LDS lists, three 32-item sub-tiles per step (12 waves per block)      x SPEC 0 / 1 / 2
//         1  up to 128 factors, LDS lists, two sub-tiles                                              x SPEC 0 / 1 / 2
//         2  up to 128 factors, lists in HBM: replace-the-minimum and append buffers                  x SPEC 0 / 1 / 2
//         3  more than 128 factors (256, 512: chunk count at compile time; beyond: at run time, ng 0)   SPEC 0 only
//         4  the score dump, up to 128 factors (beyond: family 3)                                       SPEC 0 only
//   fp64  5  up to 64 factors                                                                         x SPEC 0 / 1
//         6  128, 256, 512 factors and the run-time count                                             x SPEC 0 / 1
// (the fp64 dumps are rows of the SPEC 0 units)
#include <hip/hip_runtime.h>
#include "rm_launch.hpp"

namespace rm {
template <class Args, int FAMILY, int SPEC> SweepRows<Args> unit_rows();       // one explicit specialisation per unit
}

#ifdef RM_FAMILY
#if RM_FAMILY >= 5
#include "rm_sweep64.hpp"
#else
#include "rm_sweep.hpp"
#endif

namespace rm {

#if RM_FAMILY >= 5
typedef Sweep64Args Args;
#else
typedef SweepArgs Args;
#endif

template <int NG, bool AUC, bool DUMP, int LMODE, int NSUB, int SPEC>
static int launch(dim3 grid, size_t lds, hipStream_t stream, const Args &sa)
{
#if RM_FAMILY >= 5
    static_assert(NSUB == 2, "k_sweep64 has two sub-tiles");
    auto kern = k_sweep64<NG, AUC, DUMP, LMODE, SPEC>;
    constexpr int threads = SWEEP_THREADS;
#else
    auto kern = k_sweep<NG, AUC, DUMP, LMODE, NSUB, SPEC>;
    constexpr int threads = 256 * NSUB;
#endif
    hipError_t e = hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(kern, grid, dim3(threads), lds, stream, sa);
    return (int)hipGetLastError();
}

// key and launcher of a row come from the same arguments
#define ROW(NG, AUC, DUMP, LMODE, NSUB, SPEC) {{NG, AUC, DUMP, LMODE, NSUB, SPEC}, launch<NG, AUC, DUMP, LMODE, NSUB, SPEC>}
// factor-group counts of 8: every count up to 64 factors (50 -- the reference notebook's model -- run as 56, not as 64) ...
#define NG_TO_64(...) ROW(2, __VA_ARGS__), ROW(3, __VA_ARGS__), ROW(4, __VA_ARGS__), ROW(5, __VA_ARGS__), ROW(6, __VA_ARGS__), ROW(7, __VA_ARGS__), ROW(8, __VA_ARGS__)
// ... fp32 between 64 and 128 factors: 80, 96 and 100 (implicit-feedback libraries' usual defaults) have kernels of their own
#define NG_TO_128(...) NG_TO_64(__VA_ARGS__), ROW(10, __VA_ARGS__), ROW(12, __VA_ARGS__), ROW(13, __VA_ARGS__), ROW(16, __VA_ARGS__)
#define NG32_LARGE(...) ROW(32, __VA_ARGS__), ROW(64, __VA_ARGS__), ROW(0, __VA_ARGS__)
#define NG64_LARGE(...) ROW(16, __VA_ARGS__), ROW(32, __VA_ARGS__), ROW(64, __VA_ARGS__), ROW(0, __VA_ARGS__)
#define BOTH_AUC(NGS, LMODE, NSUB) NGS(true, false, LMODE, NSUB, RM_SPEC), NGS(false, false, LMODE, NSUB, RM_SPEC)
#define LISTS_OF(NGS, AUC) NGS(AUC, false, LM_LDS, 2, RM_SPEC), NGS(AUC, false, LM_HBM, 2, RM_SPEC), NGS(AUC, false, LM_HBM_APPEND, 2, RM_SPEC)
#define ALL_LISTS(NGS) LISTS_OF(NGS, true), LISTS_OF(NGS, false)
#define DUMP_OF(NGS) NGS(false, true, LM_HBM, 2, 0)

// (a unit's kernels are laid out in its code object in the order of its rows)
static const SweepRow<Args> rows[] = {
#if RM_FAMILY == 0
    BOTH_AUC(NG_TO_64, LM_LDS, 3),
#elif RM_FAMILY == 1
    BOTH_AUC(NG_TO_128, LM_LDS, 2),
#elif RM_FAMILY == 2
    BOTH_AUC(NG_TO_128, LM_HBM, 2), BOTH_AUC(NG_TO_128, LM_HBM_APPEND, 2),
#elif RM_FAMILY == 3
    DUMP_OF(NG32_LARGE), ALL_LISTS(NG32_LARGE),
#elif RM_FAMILY == 4
    DUMP_OF(NG_TO_128),
#elif RM_FAMILY == 5 && RM_SPEC == 0
    DUMP_OF(NG_TO_64), ALL_LISTS(NG_TO_64),
#elif RM_FAMILY == 5
    ALL_LISTS(NG_TO_64),
#elif RM_FAMILY == 6 && RM_SPEC == 0
    DUMP_OF(NG64_LARGE), ALL_LISTS(NG64_LARGE),
#elif RM_FAMILY == 6
    ALL_LISTS(NG64_LARGE),
#endif
};

template <> SweepRows<Args> unit_rows<Args, RM_FAMILY, RM_SPEC>() { return {rows, (int)(sizeof(rows) / sizeof(rows[0]))}; }

} // namespace rm

#else   // ---- the table: the units in one list per precision, and the rule from a request to a key -----------------------------

namespace rm {

template <> SweepRows<SweepArgs> sweep_rows<SweepArgs>(int unit)
{
    switch (unit) {
        case 0: return unit_rows<SweepArgs, 0, 0>();
        case 1: return unit_rows<SweepArgs, 0, 1>();
        case 2: return unit_rows<SweepArgs, 0, 2>();
        case 3: return unit_rows<SweepArgs, 1, 0>();
        case 4: return unit_rows<SweepArgs, 1, 1>();
        case 5: return unit_rows<SweepArgs, 1, 2>();
        case 6: return unit_rows<SweepArgs, 2, 0>();
        case 7: return unit_rows<SweepArgs, 2, 1>();
        case 8: return unit_rows<SweepArgs, 2, 2>();
        case 9: return unit_rows<SweepArgs, 3, 0>();
        case 10: return unit_rows<SweepArgs, 4, 0>();
        default: return {nullptr, 0};
    }
}

template <> SweepRows<Sweep64Args> sweep_rows<Sweep64Args>(int unit)
{
    switch (unit) {
        case 0: return unit_rows<Sweep64Args, 5, 0>();
        case 1: return unit_rows<Sweep64Args, 5, 1>();
        case 2: return unit_rows<Sweep64Args, 6, 0>();
        case 3: return unit_rows<Sweep64Args, 6, 1>();
        default: return {nullptr, 0};
    }
}

// The rule says which variant a request WANTS; whether it exists is the table's answer (find_sweep).  Beyond 512 factors the one
// kernel with a run-time chunk count (ng 0) serves whole chunks only, and only the count the operands were packed for (ngt).
static int template_ng(int ng, int ngt, int chunk) { return ng > 64 && ng % chunk == 0 && ngt == ng ? 0 : ng; }

template <> bool sweep_key<SweepArgs>(int ng, int ngt, bool auc, bool dump, int lmode, int nsub, int spec, SweepKey &key)
{
    if (ng < 2) return false;
    lmode = lmode == LM_LDS || lmode == LM_HBM ? lmode : LM_HBM_APPEND;
    spec = spec == 1 || spec == 2 ? spec : 0;
    if (nsub == 3) {                      // three sub-tiles exist for LDS lists up to 64 factors
        if (dump || lmode != LM_LDS || ng > 8) return false;
        key = {ng, auc, 0, LM_LDS, 3, spec};
        return true;
    }
    if (ng > 16) { ng = template_ng(ng, ngt, 16); spec = 0; }          // (the kernels beyond 128 factors have no specialisations)
    key = dump ? SweepKey{ng, 0, 1, LM_HBM, 2, 0} : SweepKey{ng, auc, 0, lmode, 2, spec};
    return true;
}

template <> bool sweep_key<Sweep64Args>(int ng, int ngt, bool auc, bool dump, int lmode, int, int spec, SweepKey &key)
{
    if (ng < 2) return false;
    lmode = lmode == LM_LDS || lmode == LM_HBM ? lmode : LM_HBM_APPEND;
    ng = template_ng(ng, ngt, 8);
    key = dump ? SweepKey{ng, 0, 1, LM_HBM, 2, 0} : SweepKey{ng, auc, 0, lmode, 2, spec == 1};
    return true;
}

} // namespace rm
#endif
