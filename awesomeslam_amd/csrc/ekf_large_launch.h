// ekf_large_launch.h -- host side of the large-state EKF (n > 143, or fp32), included by aslam_core.hip: the environment knobs, the launch
// plan (which of the four kernel chains a callback runs: large_plan() is the ONE place that decides it -- aslam_create, the launcher and
// aslam_kernel_info read its result), views shifted to a group of filters, the chain launcher and the split of a batch into stream groups.
// The default binary32 chain (LargeChain::F32_RESIDENT on the bf16 pipe) solves a tail of <= 3 rows past the last full 64-block as a border
// (large_border(), ekf_large.h): LargePlan::border says so, every group's view carries it to the kernels (LargeView::border), and the X update is
// then launched in front of the syrk.  ASLAM_BORDER=0 is the chain without it.
// Which front-end instantiation a launch takes is a FrontendVariant, passed in by value; with_variant() turns it into template arguments, so
// each family names its kernel template in one expression (to add a variant flag: one member and one line per family).
// The list of the arrays a filter owns is for_each_array(), next to each view's struct (DevView: small_common.h, LargeView: ekf_large.h):
// to add an array, add the member and one line there -- aslam_create, shifted(), aslam_reset and the clear list of restore follow.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "ekf_large.h"
#include "aslam_large16.h"

namespace aslam
{
constexpr int LARGE_GROUPS_MAX = 8;         // capacity of LargeHost's streams; the default number of groups was chosen by measurement (profiles/)
constexpr int CHOL_RESIDENT_MIN_BATCH = 32; // filters in a launch from which a filter per workgroup fills the chip

/// environment knobs (diagnostics / A-B runs; the defaults are what bench.py measures), read once per large-state context in aslam_create
struct LargeKnobs
{
        // replay splits the batch into groups that run the launch chain side by side on separate streams: the latency-bound launches of one
        // group (one-wave diagonal factorisations, the front end, short-K panels) then overlap the GEMMs of the others.
        // ASLAM_LARGE_GROUPS=1..8 (1 = a single stream, for per-kernel profiling); 3: 88 / 88 / 80 of 256 filters -- measured best at the end of
        // round 4 (tools/manual/sweep_groups.sh: 37.4 - 38.0 k filter-steps/s against 36.6 - 36.8 k with 4, 36.5 - 37.1 k with 2)
        int groups = 3;
        // binary32 mode: Cholesky of S as ONE launch with a filter per workgroup (the resident kernels) when the filters of the launch can fill
        // the chip that way (CHOL_RESIDENT_MIN_BATCH), as multi-workgroup launches per block column for few filters.  ASLAM_CHOL_RESIDENT=0/1
        // forces one form
        int chol_resident = -1;
        int right_step = 1;   // binary32 mode below the resident batch: the right-looking one-launch-per-block-column chain (large_right_step); ASLAM_RIGHT_STEP=0: the left-looking chain of rounds 1 - 2 (potrf + panel launches, large_trsm_pipe)
        int bf16_pipe = 3;    // binary32 mode, resident chain: bit 0 the TRSM, bit 1 the Cholesky on the bf16 matrix pipe (large_trsm_bf16, large_chol_bf16: ekf_large_trsm16.h); ASLAM_BF16_PIPE=0: the fp32-MFMA pair (diagnostics: 1 = large_chol_resident writes the planes, 2 = large_trsm_pipe solves)
        int keep_l32 = 0;     // ASLAM_KEEP_L32=1 (tests/manual/large_residuals.py reads L back): large_chol_bf16 also stores the off-diagonal blocks of L in binary32
        int gs_tiles = 0;     // G, S by the row-pair kernel that reads all of P (large_build_GS); ASLAM_GS_TILES=1: from the lower block triangle of P (large_build_GS_tiles) -- bit-identical results, slower, kept for its test
        int border = 1;       // default chain (bf16-pipe Cholesky and TRSM): a tail of <= 3 rows past the last full 64-block is solved as a binary64 border by the X update (large_border, ekf_large.h); ASLAM_BORDER=0: every block row and column through the sweeps, the X update behind the syrk -- kept for its agreement test
        int syrk_tail = 1;    // large_syrk_bf16x3<false>: a last tile row of <= 16 state rows is formed by the idle waves of the diagonal tiles (large_syrk_tail, ekf_large.h); ASLAM_SYRK_TAIL=0: that row as 128x128 tiles of its own -- bit-identical results, kept for its agreement test
        int syrk_running = 0; // diagnostic (ASLAM_SYRK_RUNNING=1): round 2's accumulation order in large_syrk_bf16x3 (profiles/r03_experiments.md)
};

inline LargeKnobs large_knobs_from_env()
{
        LargeKnobs k;
        auto flag = [](const char *name, int &v) { if (const char *e = std::getenv(name)) v = std::atoi(e) != 0; };
        if (const char *e = std::getenv("ASLAM_LARGE_GROUPS"))
                k.groups = std::max(1, std::min(LARGE_GROUPS_MAX, std::atoi(e)));
        if (const char *e = std::getenv("ASLAM_BF16_PIPE"))
                k.bf16_pipe = std::atoi(e) & 3;
        flag("ASLAM_CHOL_RESIDENT", k.chol_resident);
        flag("ASLAM_RIGHT_STEP", k.right_step);
        flag("ASLAM_KEEP_L32", k.keep_l32);
        flag("ASLAM_GS_TILES", k.gs_tiles);
        flag("ASLAM_SYRK_RUNNING", k.syrk_running);
        flag("ASLAM_BORDER", k.border);
        flag("ASLAM_SYRK_TAIL", k.syrk_tail);
        return k;
}

/// the launches of one callback and stream group, in order (NB = NP / 64 block columns); every chain starts with the front end and G, S
enum class LargeChain
{
        F64_LEFT,     // NB x {large_potrf_inv_tiles, large_update_panel over S, G and Y^T}, large_syrk, large_x_update: 4 + 2 NB launches
        F32_RESIDENT, // Cholesky and TRSM as one launch each with the factor resident (bf16 pipe or fp32 MFMA), large_syrk_bf16x3, large_x_update_rows: 6
                      // (LargePlan::border: large_x_update_rows, which then also solves the border, IN FRONT OF the syrk)
        F32_RIGHT,    // large_potrf_inv_tiles(0), NB x large_right_step (factors S and solves the rows of G into Vw together), syrk, X update: 5 + NB
        F32_LEFT      // NB x {large_potrf_inv_tiles, large_update_panel over S}, large_trsm_pipe, syrk, X update: 4 + 2 NB
};

struct LargePlan
{
        LargeChain chain;
        bool chol16, trsm16;         // F32_RESIDENT: large_chol_bf16 for large_chol_resident, large_trsm_bf16 for large_trsm_pipe
        bool border;                 // F32_RESIDENT with chol16 && trsm16: large_border() applies (the kernels decide per filter from its n), the X update runs in front of the syrk
        bool chol_f32out;            // large_chol_bf16 also stores the off-diagonal blocks of L in binary32 (the bf16 TRSM reads L through its planes only)
        bool gs_tiles, syrk_running; // large_build_GS_tiles for large_build_GS; large_syrk_bf16x3<true> for <false>
        bool syrk_tail;              // binary32 chains, large_syrk_bf16x3<false>: large_syrk_tail() applies (the kernel decides per filter from its n)
        int launches;                // kernel launches per callback and stream group
        bool need_Lpl, need_Vw;      // buffers a context of `batch` filters owns besides P, G, S, Hc, Y, Linv
};

/// the plan of a launch over `filters` filters (1 for a step of one trajectory) of a context created for `batch` filters
inline LargePlan large_plan(bool f32, int NP, int batch, int filters, const LargeKnobs &k)
{
        const int NB = NP / LB;
        auto resident = [&k](int nf) { return k.chol_resident >= 0 ? k.chol_resident != 0 : nf >= CHOL_RESIDENT_MIN_BATCH; };
        LargePlan p = {};
        p.gs_tiles = k.gs_tiles != 0;
        p.syrk_running = k.syrk_running != 0;
        p.syrk_tail = f32 && !p.syrk_running && k.syrk_tail != 0;
        p.need_Lpl = f32 && k.bf16_pipe != 0;
        p.need_Vw = f32 && k.right_step && !resident(batch); // (a one-trajectory step on a context that is resident as a whole finds no Vw: F32_LEFT)
        if (!f32)
                p.chain = LargeChain::F64_LEFT, p.launches = 4 + 2 * NB;
        else if (resident(filters))
        {
                p.chain = LargeChain::F32_RESIDENT, p.launches = 6;
                p.chol16 = (k.bf16_pipe & 2) != 0;
                p.trsm16 = (k.bf16_pipe & 1) != 0;
                p.chol_f32out = !p.trsm16 || k.keep_l32;
                p.border = p.chol16 && p.trsm16 && !k.keep_l32 && k.border != 0;
        }
        else if (p.need_Vw)
                p.chain = LargeChain::F32_RIGHT, p.launches = 5 + NB;
        else
                p.chain = LargeChain::F32_LEFT, p.launches = 4 + 2 * NB;
        return p;
}

/// what a large-state context owns on the host side: its knobs, the streams and events of the stream groups, and what its LAST launch really
/// did (aslam_get_launch_info: the tests assert on it, not on the configuration)
struct LargeHost
{
        LargeKnobs knobs;
        hipStream_t aux[LARGE_GROUPS_MAX - 1] = {};
        hipEvent_t ev_fork = nullptr, ev_join[LARGE_GROUPS_MAX - 1] = {};
        int last_groups = 0;        // stream groups that received work (1 = the caller's stream alone; 0 = nothing launched yet)
        int last_launches = 0;      // kernel launches per callback and stream group of that launch (large_stats included)
        bool last_resident = false; // that launch ran LargeChain::F32_RESIDENT
        bool last_syrk_tail = false; // the views of that launch carried the syrk's tail rule (LargeView::syrk_tail; aslam_get_syrk_tail)
};

/// Which instantiation of its front-end family (ekf_small_kernel, ukf_small_kernel, large_frontend_kernel, ukf_large_frontend_kernel) a launch
/// takes: computed ONCE per launch (frontend_variant() in aslam_core.hip, the one rule), passed by value, and read by the launchers and by
/// aslam_kernel_info alike.  To add a variant flag: one member here, one line in the rule and one line per family.
struct FrontendVariant
{
        bool stats;   // a StatsView with something to write: the STATS instantiations of the single-CU kernels (the large chains launch large_stats instead)
        bool sighted; // aslam_sighted_update_enable, EKF contexts alone: SIGHTED (large-state: the front end and large_build_GS, which then also stands in for large_build_GS_tiles)
        bool gated;   // aslam_set_replay_gate with some gate > 0, the replay seam alone: GATED
};

/// f(stats, sighted, gated) with the run-time flags as std::bool_constants, so that a family names its kernel template in one expression.  HAS_*:
/// the flags the family has in this seam; one it has not is std::false_type whatever `v` says, so no instantiation beyond the built ones is formed
template <bool HAS, typename F> auto with_flag(bool on, F &&f)
{
        if constexpr (HAS)
                if (on)
                        return f(std::true_type{});
        return f(std::false_type{});
}
template <bool HAS_STATS, bool HAS_SIGHTED, bool HAS_GATED, typename F> auto with_variant(FrontendVariant v, F &&f)
{
        return with_flag<HAS_STATS>(v.stats, [&](auto st) {
                return with_flag<HAS_SIGHTED>(v.sighted, [&](auto si) { return with_flag<HAS_GATED>(v.gated, [&](auto ga) { return f(st, si, ga); }); });
        });
}

/// which filters a launch covers: one trajectory (MODE_STEP with sa.traj >= 0; the views then start at it, so the kernels get traj = 0) or the
/// whole batch of B (sa.traj < 0 is the batched step)
struct LaunchSlice
{
        int first, count;
        StepArgs sa;
};
template <int MODE> LaunchSlice launch_slice(StepArgs sa, int B)
{
        if (MODE != MODE_STEP || sa.traj < 0)
                return {0, B, sa};
        const int first = sa.traj;
        sa.traj = 0;
        return {first, 1, sa};
}

// the kernels index the filter through blockIdx: a group of filters starting at b gets views whose per-filter arrays (for_each_array next to
// each view's struct) start there.  Arrays the context does not own stay null
struct ShiftBy
{
        size_t b;
        template <typename T> void operator()(T *&p, size_t per, bool) const
        {
                if (p)
                        p += b * per;
        }
};

/// LargeView<T>, UkfLargeView (np: the NP a UKF view does not carry itself).  A DevView has more than its arrays to shift: shifted_dev
template <typename V, typename... NP> V shifted(V v, size_t b, NP... np)
{
        static_assert(!std::is_same<V, DevView>::value && !std::is_same<V, StatsView>::value, "shifted_dev / shifted_stats");
        for_each_array(v, np..., ShiftBy{b});
        return v;
}

/// a DevView: its per-filter arrays, step_in ([3][B]: the stride stays the whole batch) and, in replay, the bound trace ([B][T]-shaped)
inline DevView shifted_dev(DevView d, size_t b, bool trace)
{
        const size_t T_ = (size_t)d.T;
        for_each_array(d, ShiftBy{b});
        d.step_in += b;
        if (trace)
        {
                d.tr_pose += 2 * b * T_;
                d.tr_yaw += b * T_;
                d.tr_twist += 2 * b * T_;
                d.tr_dt += b * T_;
                d.tr_new += b * T_;
                d.tr_nobs += b * T_;
                d.tr_obs += b * T_ * (size_t)d.max_obs * 2;
        }
        return d;
}

/// the per-callback arrays are [B][nsteps]-shaped, the last-callback record [B][2]
inline StatsView shifted_stats(StatsView sv, size_t b, int nsteps)
{
        if (sv.nis)
                sv.nis += b * (size_t)nsteps;
        if (sv.logdet)
                sv.logdet += b * (size_t)nsteps;
        if (sv.pcov)
                sv.pcov += b * (size_t)nsteps * 6;
        if (sv.last)
                sv.last += 2 * b;
        return sv;
}

template <typename T> struct LargeGroup
{
        DevView dv;
        LargeView<T> v;
        int *skip;
        double *poses;
        int32_t *dims;
        int nb;
        hipStream_t st;
        StatsView sv; // statistics asked for with this launch (all null: none, and no large_stats launch)
};

/// The blocked left-looking loop over the NB block columns of a view: the one-wave factorisation of the diagonal block (with its inverse), then
/// the panel launch that eliminates the block column.  s_only = 0: over the stacked [S; G; vector rows] (the factor-and-solve of a callback);
/// s_only = 1: over S alone, where the last block column has nothing below it (last_panel = false).  Returns the launches issued
template <typename T>
int launch_left_looking(const DevView &dv, const LargeView<T> &v, int NB, int gb, int *skip, hipStream_t st, int s_only, bool last_panel)
{
        int count = 0;
        for (int k = 0; k < NB; ++k)
        {
                hipLaunchKernelGGL(large_potrf_inv_tiles<T>, dim3(gb), dim3(256), 0, st, dv, v, k, skip);
                ++count;
                if (k + 1 < NB || last_panel)
                {
                        hipLaunchKernelGGL(large_update_panel<T>, dim3(((s_only ? NB : 2 * NB) - k) / 2, 1, gb), dim3(256), 0, st, dv, v, k, s_only, skip);
                        ++count;
                }
        }
        return count;
}

/// The front-end kernel of a launch (GATED exists for the replay seam alone)
template <typename T, int MODE> auto large_frontend_of(FrontendVariant v)
{
        return with_variant<false, true, MODE == MODE_REPLAY>(
                v, [](auto, auto si, auto ga) { return &large_frontend_kernel<T, MODE, decltype(si)::value, decltype(ga)::value>; });
}

/// callback s of one group: front end + predict, G, S, blocked factorisation of [S; G; Y^T], P -= V V^T, X += V q
template <typename T, int MODE, typename K>
void launch_large_chain(const LargePlan &plan, const LargeGroup<T> &g, K frontend, size_t lds, int64_t t0, int s, int nsteps, StepArgs sa, bool sighted)
{
        const int NP = g.v.NP, NB = NP / LB, gb = g.nb;
        // the front end (`frontend`, `lds`: the caller's large_frontend_of and LargeLds::launch_bytes), then G and S.  The sighted-only
        // update enters in these two launches alone (ASLAM_GS_TILES=1 has no masked form: large_build_GS runs); the gate in the first
        hipLaunchKernelGGL(frontend, dim3(gb), dim3(SMALL_WG), lds, g.st, g.dv, g.v, t0 + s, s, nsteps, g.poses, g.dims, sa, g.skip);
        if (sighted)
                hipLaunchKernelGGL((large_build_GS<T, true>), dim3(1 + (NP / 2 + GS_ROW_PAIRS - 1) / GS_ROW_PAIRS, gb), dim3(256), 0, g.st, g.dv, g.v, g.skip);
        else if (plan.gs_tiles)
                hipLaunchKernelGGL(large_build_GS_tiles<T>, dim3(NB * (NB + 1) / 2, gb), dim3(256), 0, g.st, g.dv, g.v, g.skip);
        else
                hipLaunchKernelGGL(large_build_GS<T>, dim3(1 + (NP / 2 + GS_ROW_PAIRS - 1) / GS_ROW_PAIRS, gb), dim3(256), 0, g.st, g.dv, g.v, g.skip);
        const int ntile = (NP + 127) / 128;
        const dim3 syrk_grid(8 * (ntile * (ntile + 1) / 2) * ((gb + 7) / 8));
        if constexpr (sizeof(T) == 8)
        { // F64_LEFT
                launch_left_looking(g.dv, g.v, NB, gb, g.skip, g.st, 0, true);
                hipLaunchKernelGGL(large_syrk<T>, syrk_grid, dim3(256), 0, g.st, g.dv, g.v, gb, g.skip);
                hipLaunchKernelGGL((large_x_update<T, MODE>), dim3((NP + 3) / 4, gb), dim3(256), 0, g.st, g.dv, g.v, s, nsteps, g.poses, g.dims, g.skip);
                if (g.sv.any())
                        hipLaunchKernelGGL(large_stats<T>, dim3(gb), dim3(256), 0, g.st, g.dv, g.v, s, nsteps, g.sv, g.skip);
        }
        else
        {
                LargeView<T> vv = g.v; // what the consumers of V read
                switch (plan.chain)
                {
                case LargeChain::F32_RESIDENT:
                        if (plan.chol16)
                                launch_chol_bf16(g.dv, g.v, gb, g.skip, g.st, plan.chol_f32out);
                        else
                                hipLaunchKernelGGL(large_chol_resident<LARGE_NB_MAX>, dim3(gb), dim3(256), 0, g.st, g.dv, g.v, g.skip);
                        if (plan.trsm16)
                                launch_trsm_bf16(g.dv, g.v, gb, g.skip, g.st);
                        else
                                hipLaunchKernelGGL(large_trsm_pipe<LARGE_NB_MAX>, dim3(8 * ((gb + 7) / 8) * NB), dim3(256), 0, g.st, g.dv, g.v, gb, g.skip);
                        break;
                case LargeChain::F32_RIGHT:
                        hipLaunchKernelGGL(large_potrf_inv_tiles<T>, dim3(gb), dim3(256), 0, g.st, g.dv, g.v, 0, g.skip);
                        for (int k = 0; k < NB; ++k)
                        {
                                const int M = NB - k - 1;
                                hipLaunchKernelGGL(large_right_step<0>, dim3(M * (M + 1) / 2 + NB * M + NB, 1, gb), dim3(256), 0, g.st, g.dv, g.v, k, g.skip);
                        }
                        vv.G = g.v.Vw; // V is there, row n = q included (large_right_step has solved the rows of G on its way)
                        break;
                default: // F32_LEFT
                        launch_left_looking(g.dv, g.v, NB, gb, g.skip, g.st, 1, false);
                        hipLaunchKernelGGL(large_trsm_pipe<LARGE_NB_MAX>, dim3(8 * ((gb + 7) / 8) * NB), dim3(256), 0, g.st, g.dv, g.v, gb, g.skip);
                }
                // X += V q (+ the diagonal and the pose columns of V V^T in binary64) on the same stream as the syrk; the two write disjoint entries of P,
                // so their order is free.  With the border the X update goes FIRST: it completes V (the columns V2 past the last full 64-block) for the
                // syrk to read.  Without it, behind the syrk as ever.  Round 4 tried the two ways of running it NEXT TO the syrk -- its workgroups inside
                // the syrk launch, and on a side stream of its own -- and both were slower: 2436 us against 1997 + 324 per 256 filters, and 31.7 k
                // against 36.4 k filter-steps/s (profiles/r04_experiments.md section 1)
                auto x_update = [&]() {
                        hipLaunchKernelGGL((large_x_update_rows<MODE>), dim3((NP + XU_WG_ROWS - 1) / XU_WG_ROWS, gb), dim3(XU_THREADS), 0, g.st, g.dv, vv, s, nsteps,
                                           g.poses, g.dims, g.skip);
                };
                if (plan.border)
                        x_update();
                if (plan.syrk_running)
                        hipLaunchKernelGGL((large_syrk_bf16x3<true>), syrk_grid, dim3(256), 0, g.st, g.dv, vv, gb, g.skip);
                else
                        hipLaunchKernelGGL((large_syrk_bf16x3<false>), syrk_grid, dim3(256), 0, g.st, g.dv, vv, gb, g.skip);
                if (!plan.border)
                        x_update();
                if (g.sv.any())
                        hipLaunchKernelGGL(large_stats<T>, dim3(gb), dim3(256), 0, g.st, g.dv, vv, s, nsteps, g.sv, g.skip);
        }
}

/// `nsteps` callbacks of a large-state context: one trajectory (MODE_STEP with sa.traj >= 0) or the whole batch, which from max(32, 8 x groups)
/// filters on is split into stream groups.  The enqueue order (callbacks outermost, groups innermost) is what the rates were measured with.
/// `sv`: statistics to write (one launch more per callback, reported in last_launches), all null for none
template <int MODE, typename T>
hipError_t launch_large(LargeHost &h, FrontendVariant fv, const DevView &dv, const LargeView<T> &lv, int *skipped, int64_t t0, int nsteps, double *poses,
                        int32_t *dims, StepArgs sa, hipStream_t st, StatsView sv = {})
{
        const auto frontend = large_frontend_of<T, MODE>(fv);
        const size_t lds = LargeLds::launch_bytes(dv.NP, fv.gated);
        if (hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(frontend), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds))
                return e;
        const LaunchSlice sl = launch_slice<MODE>(sa, dv.B);
        const int first = sl.first, Bz = sl.count;
        const LargePlan plan = large_plan(sizeof(T) == 4, dv.NP, dv.B, Bz, h.knobs);
        const bool split = Bz >= std::max(32, 8 * h.knobs.groups); // (one group below 32 filters, as with the former default of four groups)
        const int NG = split ? h.knobs.groups : 1;
        const int per = split ? ((Bz + NG - 1) / NG + 7) & ~7 : Bz; // multiples of 8: large_syrk deals filters to the 8 XCDs
        LargeGroup<T> g[LARGE_GROUPS_MAX];
        h.last_launches = plan.launches + (sv.any() ? 1 : 0); // large_stats
        h.last_resident = plan.chain == LargeChain::F32_RESIDENT;
        h.last_syrk_tail = plan.syrk_tail;
        h.last_groups = 0;
        for (int q = 0; q < NG; ++q)
        {
                const int o = std::min(q * per, Bz);
                const size_t b0 = (size_t)(first + o);
                g[q] = {shifted_dev(dv, b0, MODE == MODE_REPLAY), shifted(lv, b0), skipped + b0, poses, dims, std::min(per, Bz - o), q == 0 ? st : h.aux[q - 1], shifted_stats(sv, b0, nsteps)};
                g[q].v.border = plan.border; // (per launch: a one-trajectory step of a resident context runs another chain)
                g[q].v.syrk_tail = plan.syrk_tail;
                if (MODE == MODE_REPLAY && poses)
                        g[q].poses += b0 * (size_t)nsteps * 3;
                if (MODE == MODE_REPLAY && dims)
                        g[q].dims += b0 * (size_t)nsteps;
                h.last_groups += g[q].nb > 0;
        }
        hipError_t e = split ? hipEventRecord(h.ev_fork, st) : hipSuccess;
        for (int q = 1; q < NG && e == hipSuccess; ++q)
                e = hipStreamWaitEvent(h.aux[q - 1], h.ev_fork, 0);
        if (e != hipSuccess)
                return e;
        for (int s = 0; s < nsteps; ++s)
                for (int q = 0; q < NG; ++q)
                        if (g[q].nb > 0)
                                launch_large_chain<T, MODE>(plan, g[q], frontend, lds, t0, s, nsteps, sl.sa, fv.sighted);
        for (int q = 1; q < NG && e == hipSuccess; ++q)
                if ((e = hipEventRecord(h.ev_join[q - 1], h.aux[q - 1])) == hipSuccess)
                        e = hipStreamWaitEvent(st, h.ev_join[q - 1], 0);
        return e != hipSuccess ? e : hipGetLastError();
}
} // namespace aslam
