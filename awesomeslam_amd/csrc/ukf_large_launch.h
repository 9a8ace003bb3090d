// ukf_large_launch.h -- host side of the large-state UKF (ukf_large.h), included by aslam_core.hip: the launch plan (ukf_large_plan() is the ONE
// place that says how many launches a callback is -- the launcher walks it, aslam_get_launch_info and aslam_kernel_info report it), views
// shifted to a trajectory, and the chain launcher (its front end picked by the caller's FrontendVariant).  One stream: the caller's (no stream groups on this path).  The list of the arrays a filter
// owns on this path is for_each_array(UkfLargeView &) in ukf_large.h: to add an array, add the member and one line there.
#pragma once

#include "ekf_large_launch.h"
#include "ukf_large.h"

namespace aslam
{
/// the launches of one callback, in order (NB = NP / 64 block columns)
struct UkfLargePlan
{
        int NB;
        int frontend;  // ukf_large_frontend_kernel                                                             1
        int chol_p;    // NB x large_potrf_inv_tiles + (NB - 1) x large_update_panel(s_only) over the copy of P  2 NB - 1
        int sigma;     // ukf_large_sigma_pose, ukf_large_points                                                 2
        int products;  // ukf_large_wabt: P, S+, Tc                                                              3
        int solve;     // NB x {large_potrf_inv_tiles, large_update_panel} over [S+; Tc; z^T; (Z - Zpred)^T]     2 NB
        int update;    // ukf_large_gain, large_syrk, ukf_large_rank1                                            3
        int launches;  // 4 NB + 8
};

inline UkfLargePlan ukf_large_plan(int NP)
{
        UkfLargePlan p = {};
        p.NB = NP / LB;
        p.frontend = 1;
        p.chol_p = 2 * p.NB - 1;
        p.sigma = 2;
        p.products = 3;
        p.solve = 2 * p.NB;
        p.update = 3;
        p.launches = p.frontend + p.chol_p + p.sigma + p.products + p.solve + p.update;
        return p;
}

/// `nsteps` callbacks of a large-state UKF context: one trajectory (MODE_STEP with sa.traj >= 0) or the whole batch
template <int MODE>
hipError_t launch_ukf_large(LargeHost &h, FrontendVariant fv, const DevView &dv0, const LargeView<double> &lv0, const UkfLargeView &uv0, int *skipped0, int64_t t0,
                            int nsteps, double *poses, int32_t *dims, StepArgs sa, hipStream_t st, StatsView sv0 = {})
{
        const int NP = dv0.NP;
        // the front end of this launch (GATED: the replay seam alone, with its landmark table behind the rest of the LDS)
        const auto frontend = with_variant<false, false, MODE == MODE_REPLAY>(fv, [](auto, auto, auto ga) { return &ukf_large_frontend_kernel<MODE, decltype(ga)::value>; });
        const size_t lds = LargeLds::launch_bytes(NP, fv.gated);
        if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(frontend), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
                return e;
        const LaunchSlice sl = launch_slice<MODE>(sa, dv0.B);
        const size_t first = (size_t)sl.first;
        const int gb = sl.count;
        const DevView dv = shifted_dev(dv0, first, MODE == MODE_REPLAY);
        const LargeView<double> lv = shifted(lv0, first);
        const UkfLargeView uv = shifted(uv0, first, NP);
        int *skip = skipped0 + first;
        const StatsView sv = shifted_stats(sv0, first, nsteps); // statistics to write (large_stats: one launch more per callback), all null for none
        const UkfLargePlan plan = ukf_large_plan(NP);
        const int NB = plan.NB;
        const int ntile = (NP + 127) / 128;
        const int fgroups = (gb + 7) / 8; // ukf_large_wabt and large_syrk deal filters to the 8 XCDs
        h.last_launches = plan.launches + (sv.any() ? 1 : 0);
        h.last_resident = false;
        h.last_syrk_tail = false;
        h.last_groups = 1;
        for (int s = 0; s < nsteps; ++s)
        {
                int count = 0;
                hipLaunchKernelGGL(frontend, dim3(gb), dim3(SMALL_WG), lds, st, dv, lv, uv, t0 + s, s, nsteps, poses, dims, sl.sa, skip);
                count += plan.frontend;
                count += launch_left_looking(dv, lv, NB, gb, skip, st, 1, false); // L = chol(P) in S
                hipLaunchKernelGGL(ukf_large_sigma_pose, dim3(gb), dim3(256), 0, st, dv, lv, uv, skip);
                hipLaunchKernelGGL(ukf_large_points, dim3(NP / 2, gb), dim3(256), 0, st, dv, lv, uv, skip);
                count += plan.sigma;
                for (int mode : {WABT_P, WABT_S, WABT_TC})
                {
                        hipLaunchKernelGGL(ukf_large_wabt, dim3(8 * ukf_wabt_tiles(NP, mode) * fgroups), dim3(256), 0, st, dv, lv, uv, mode, gb, skip);
                        ++count;
                }
                count += launch_left_looking(dv, lv, NB, gb, skip, st, 0, true); // S+ = L L^T, W = Tc L^-T, q = L^-1 z, t = L^-1 (Z - Zpred)
                hipLaunchKernelGGL((ukf_large_gain<MODE>), dim3((NP + 3) / 4, gb), dim3(256), 0, st, dv, lv, uv, s, nsteps, poses, dims, skip);
                hipLaunchKernelGGL(large_syrk<double>, dim3(8 * (ntile * (ntile + 1) / 2) * fgroups), dim3(256), 0, st, dv, lv, gb, skip);
                hipLaunchKernelGGL(ukf_large_rank1, dim3((NP + 3) / 4, gb), dim3(256), 0, st, dv, lv, uv, skip);
                count += plan.update;
                if (count != plan.launches)
                        return hipErrorAssert; // the plan and the launcher disagree: a bug, not a run-time condition
                if (sv.any())
                        hipLaunchKernelGGL(large_stats<double>, dim3(gb), dim3(256), 0, st, dv, lv, s, nsteps, sv, skip);
        }
        return hipGetLastError();
}
} // namespace aslam
