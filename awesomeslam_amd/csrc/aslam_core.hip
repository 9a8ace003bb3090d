// aslam_core.hip -- libaslam_core.so: context management + C ABI (include/aslam_core.h) over the gfx950 kernels (the launches of the large-state
// paths: ekf_large_launch.h, ukf_large_launch.h).
//
// Build (see Makefile): hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -shared -fPIC
// No CPU fallback exists: without a HIP device every compute entry point returns ASLAM_ERR_HIP.
#include "../../include/aslam_core.h"
#include "../../include/aslam_scan.h"
#include "../../include/aslam_snapshot.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <algorithm>
#include <utility>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include "ekf_small.h"
#include "ekf_large.h"
#include "ekf_large_launch.h"
#include "scan_front.h"
#include "snapshot.h"
#include "prune.h"
#include "merge.h"
#include "join.h"
#include "assoc.h"
#include "joint.h"
#if ASLAM_HAVE_UKF
#include "ukf_small.h"
#include "ukf_large.h"
#include "ukf_large_launch.h"
#endif

using namespace aslam;

static_assert(sizeof(aslam_params) == 80, "aslam_params is part of the C ABI");

namespace
{
thread_local std::string g_err;

int fail(int code, const std::string &msg)
{
        g_err = msg;
        return code;
}

#define HIP_TRY(expr)                                                                                                  \
        do                                                                                                             \
        {                                                                                                              \
                hipError_t e_ = (expr);                                                                                \
                if (e_ != hipSuccess)                                                                                  \
                        return fail(ASLAM_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                 \
        } while (0)
} // namespace

struct aslam_ctx
{
        aslam_config cfg;
        int NT;   // 16-wide tiles per dimension
        int NP;   // padded dimension
        DevView dv;
        std::vector<void *> owned; // hipMalloc'ed blocks (state)
        std::vector<void *> trace_owned;
        hipStream_t last_stream;
        int64_t hbm_bytes;
#if ASLAM_HAVE_UKF
        UkfView ukf = {};
        UkfLargeView ukfl = {}; // large-state UKF (ASLAM_CFG_UKF_LARGE): D, DZ and the small vectors of ukf_large.h
#endif
        // large-state path (n > 143): typed covariance buffers, one launch chain per callback
        bool large = false;
        LargeView<double> lv64 = {};
        LargeView<float> lv32 = {};
        int *skipped = nullptr;
        float *step_in = nullptr; // [3][batch] vx, az, dt of a batched step
        double *largeP = nullptr; // = lv64.P or lv32.P: the covariance is binary64 in both modes
        LargeHost lh; // knobs, streams of the stream groups, what the last launch did (ekf_large_launch.h)
        // aslam_innovation_enable: [batch][2] (nis, logdet) of every filter's last callback, allocated by the first enable; off by default
        double *innov = nullptr;
        bool innov_on = false;
        // aslam_sighted_update_enable: the EKF update takes the rows of the landmarks sighted in the callback alone (dv.sighted); off by default
        bool sighted_on = false;
        // aslam_set_replay_gate: the host copy of dv.gate ([batch] doubles in HBM).  Some gate > 0: the replay seam launches the GATED instantiations
        std::vector<double> gates;
        bool gated() const { return std::any_of(gates.begin(), gates.end(), [](double g) { return g > 0.0; }); }
        // aslam_set_params: the host copy of dv.prm ([batch] records in HBM); aslam_grow and init_state read p0_landmark / p0_pose from it
        std::vector<aslam_params> params;
        aslam_params *params_dev = nullptr;
        // the staging block of the maintenance calls (Staging below): descriptors, reports, staged host arrays, records (grown on demand, not state)
        char *snap_dev = nullptr;
        size_t snap_cap = 0;
        // the pinned host mirror the HOST arguments of the asynchronous maintenance calls pass through on their way to the staging block
        // (stage_host below): free whenever the context is synchronised; blocks it has outgrown wait in stage_old for that moment
        char *stage_pin = nullptr;
        size_t stage_cap = 0, stage_used = 0;
        std::vector<void *> stage_old;
};

namespace
{
template <typename T> int dev_alloc(aslam_ctx *c, T **p, size_t count, std::vector<void *> &pool, bool counted = true)
{
        void *q = nullptr;
        HIP_TRY(hipMalloc(&q, count * sizeof(T)));
        HIP_TRY(hipMemset(q, 0, count * sizeof(T)));
        pool.push_back(q);
        if (counted) // (aslam_get_layout reports state and scratch)
                c->hbm_bytes += (int64_t)(count * sizeof(T));
        *p = static_cast<T *>(q);
        return ASLAM_OK;
}

/// copy a host n x n double matrix into filter `traj`'s P (padded stride NP, converted to the context's dtype)
int upload_P(aslam_ctx *c, int traj, int n, const double *P)
{
        const size_t NP = (size_t)c->NP;
        // (the large path keeps P in binary64 in both modes; fp32 mode: binary32 G, S, L, V and MFMA products)
        std::vector<double> v(NP * NP, 0.0);
        for (int i = 0; i < n; ++i)
                std::memcpy(&v[(size_t)i * NP], P + (size_t)i * n, sizeof(double) * n);
        HIP_TRY(hipMemcpy((c->large ? c->largeP : c->dv.P) + traj * NP * NP, v.data(), sizeof(double) * NP * NP, hipMemcpyHostToDevice));
        return ASLAM_OK;
}

int download_P(aslam_ctx *c, int traj, int n, double *P)
{
        const size_t NP = (size_t)c->NP;
        const double *src = c->large ? c->largeP : c->dv.P;
        HIP_TRY(hipMemcpy2D(P, sizeof(double) * n, src + traj * NP * NP, sizeof(double) * NP, sizeof(double) * n, n, hipMemcpyDeviceToHost));
        return ASLAM_OK;
}

/// new rows of P on growth: zero, with the filter's p0_landmark (UKF_KP_LANDMARK_POSE) on the diagonal (rows n_old .. n_new-1, full padded length)
int grow_P_rows(aslam_ctx *c, int traj, int n_old, int n_new)
{
        const size_t NP = (size_t)c->NP;
        for (int i = n_old; i < n_new; ++i)
        {
                std::vector<double> row(NP, 0.0);
                row[i] = c->params[traj].p0_landmark;
                double *dst = (c->large ? c->largeP : c->dv.P) + traj * NP * NP + (size_t)i * NP;
                HIP_TRY(hipMemcpy(dst, row.data(), sizeof(double) * NP, hipMemcpyHostToDevice));
        }
        return ASLAM_OK;
}

int check_traj(aslam_ctx *c, int traj)
{
        if (!c)
                return fail(ASLAM_ERR_ARG, "null context");
        if (traj < 0 || traj >= c->cfg.batch)
                return fail(ASLAM_ERR_ARG, "trajectory index out of range");
        return ASLAM_OK;
}

int sync_ctx(aslam_ctx *c)
{
        HIP_TRY(hipStreamSynchronize(c->last_stream));
        c->stage_used = 0; // (nothing reads the pinned mirror any more)
        // (hipHostFree may synchronise the whole device, not this context's stream alone: it runs only in the first synchronisation after the
        // mirror has outgrown a block, which a context's first few maintenance calls can cause and its steady state does not)
        for (void *p : c->stage_old)
                (void)hipHostFree(p);
        c->stage_old.clear();
        return ASLAM_OK;
}

/// `bytes` of a HOST argument of a maintenance call to `dst` in the staging block, enqueued on `st`, the call's own stream, through the
/// context's pinned mirror -- not a blocking copy through the null stream: that one waits for whatever unrelated stream shares its hardware
/// queue, and is on no stream the caller can order against.  `src` may go when the call returns.  The context is synchronised when a call
/// begins, so the mirror starts empty; a mirror that has to grow mid-call leaves the old block alive until the next synchronisation.
int stage_host(aslam_ctx *c, void *dst, const void *src, size_t bytes, hipStream_t st)
{
        if (!bytes)
                return ASLAM_OK;
        const size_t need = (bytes + 63) & ~(size_t)63;
        if (c->stage_used + need > c->stage_cap)
        {
                const size_t cap = std::max<size_t>(2 * (c->stage_used + need), 4096);
                void *q = nullptr;
                HIP_TRY(hipHostMalloc(&q, cap, hipHostMallocDefault));
                if (c->stage_pin)
                        c->stage_old.push_back(c->stage_pin);
                c->stage_pin = static_cast<char *>(q), c->stage_cap = cap, c->stage_used = 0;
        }
        char *h = c->stage_pin + c->stage_used;
        c->stage_used += need;
        std::memcpy(h, src, bytes);
        HIP_TRY(hipMemcpyAsync(dst, h, bytes, hipMemcpyHostToDevice, st));
        return ASLAM_OK;
}

/// A call of the launching seams (steps, replay) enters on `st`: on a CHANGE of stream the context's last stream is waited for first, as the
/// maintenance entries wait for it in every call (the contract in include/aslam_core.h: the context orders its own work across a change of
/// stream).  With the stream unchanged this is one comparison: nothing is enqueued, nothing is waited for.
int enter_stream(aslam_ctx *c, hipStream_t st)
{
        if (st != c->last_stream)
        {
                if (int rc = sync_ctx(c); rc != ASLAM_OK)
                        return rc;
                c->last_stream = st;
        }
        return ASLAM_OK;
}

/// the context's typed large-state view (binary32 or binary64 work matrices) handed to f
template <typename F> int with_large_view(aslam_ctx *c, F &&f)
{
        return c->cfg.dtype == ASLAM_F32 ? f(c->lv32) : f(c->lv64);
}

/// P = Identity * p0_pose (*_KP_ROBOT_POSE) on the 3 pose entries of every filter, each from its own record (P zeroed by the caller)
int seed_pose_block(const aslam_ctx *c, double *P, size_t B, size_t NP)
{
        std::vector<double> blk(3 * NP, 0.0);
        for (size_t b = 0; b < B; ++b)
        {
                for (int i = 0; i < 3; ++i)
                        blk[(size_t)i * NP + i] = c->params[b].p0_pose;
                HIP_TRY(hipMemcpy(P + b * NP * NP, blk.data(), sizeof(double) * blk.size(), hipMemcpyHostToDevice));
        }
        return ASLAM_OK;
}

/// the first field of a record that aslam_set_params refuses, or nullptr
const char *bad_param(const aslam_params &p)
{
        const struct
        {
                const char *name;
                double v;
                bool zero_ok;
        } f[] = {{"r_xy", p.r_xy, false},       {"r_yaw", p.r_yaw, false},     {"r_range", p.r_range, false},         {"r_bearing", p.r_bearing, false},
                 {"q_xy", p.q_xy, true},        {"q_yaw", p.q_yaw, true},      {"p0_pose", p.p0_pose, false},         {"p0_landmark", p.p0_landmark, false},
                 {"var_a", p.var_a, false},     {"assoc_dist", (double)p.assoc_dist, false}};
        for (const auto &e : f)
                if (!std::isfinite(e.v) || e.v < 0.0 || (e.v == 0.0 && !e.zero_ok))
                        return e.name;
        return p.promote_count < 1 ? "promote_count" : nullptr;
}

/// whether `p`, an array handed to a for_each_array visitor, is member `m` of the visited view
template <typename P, typename M> bool same_slot(const P &p, const M &m)
{
        return static_cast<const void *>(&p) == static_cast<const void *>(&m);
}

/// elements per filter of the array member `m` of view `v` points to, as the view's for_each_array says (np: the NP a UKF view does not carry)
template <typename V, typename M, typename... NP> size_t per_filter(V v, M V::*m, NP... np)
{
        size_t n = 0;
        for_each_array(v, np..., [&](auto *&p, size_t per, bool) {
                if (same_slot(p, v.*m))
                        n = per;
        });
        return n;
}

/// f(pointer, bytes per filter) for every array of the context that must be zero when a filter starts (the `zero` entries of for_each_array):
/// aslam_reset clears them for the whole batch, snapshot_unpack for the slots it restores -- one list, so the two cannot differ
template <typename F> void for_each_scratch(aslam_ctx *c, F &&f)
{
        auto pick = [&f](auto *&p, size_t per, bool zero) {
                if (zero && p)
                        f(static_cast<void *>(p), per * sizeof(*p));
        };
        if (c->large)
                with_large_view(c, [&](auto &lv) { return for_each_array(lv, pick), 0; });
#if ASLAM_HAVE_UKF
        for_each_array(c->ukf, c->NP, pick);
        for_each_array(c->ukfl, c->NP, pick);
#endif
}

/// The sighting record of filter `traj` when the host changes its dimension from n_old to n_new (aslam_grow, aslam_set_state): new landmarks
/// are growth (last seen now, never sighted), entries at or beyond a lower landmark count become 0
int resize_sightings(aslam_ctx *c, int traj, int n_old, int n_new)
{
        const size_t H = (size_t)c->NP / 2;
        const size_t L_old = (size_t)std::max(0, (n_old - 3) / 2), L_new = (size_t)(n_new - 3) / 2;
        DevView &d = c->dv;
        uint32_t *seen = d.lm_seen + traj * H, *hits = d.lm_hits + traj * H;
        if (L_new > L_old)
        {
                uint32_t clk = 0;
                HIP_TRY(hipMemcpy(&clk, d.clock + traj, sizeof(clk), hipMemcpyDeviceToHost));
                const std::vector<uint32_t> now(L_new - L_old, clk);
                HIP_TRY(hipMemcpy(seen + L_old, now.data(), sizeof(uint32_t) * now.size(), hipMemcpyHostToDevice));
                HIP_TRY(hipMemset(hits + L_old, 0, sizeof(uint32_t) * now.size()));
        }
        else if (L_new < H)
        {
                HIP_TRY(hipMemset(seen + L_new, 0, sizeof(uint32_t) * (H - L_new)));
                HIP_TRY(hipMemset(hits + L_new, 0, sizeof(uint32_t) * (H - L_new)));
        }
        return ASLAM_OK;
}

/// initialize() for the whole batch: ekf.cpp:49-71 / ukf.cpp:49-67
int init_state(aslam_ctx *c)
{
        const size_t B = c->cfg.batch, NP = c->NP;
        DevView &d = c->dv;
        double *P = c->large ? c->largeP : d.P;
        HIP_TRY(hipMemset(d.X, 0, sizeof(double) * B * NP));
        HIP_TRY(hipMemset(d.Z, 0, sizeof(double) * B * NP));
        HIP_TRY(hipMemset(P, 0, sizeof(double) * B * NP * NP));
        HIP_TRY(hipMemset(d.status, 0, sizeof(uint32_t) * B));
        HIP_TRY(hipMemset(d.sens_n, 0, sizeof(int) * B));
        HIP_TRY(hipMemset(d.wait_n, 0, sizeof(int) * B));
        HIP_TRY(hipMemset(d.clock, 0, sizeof(uint32_t) * B));
        HIP_TRY(hipMemset(d.lm_seen, 0, sizeof(uint32_t) * B * (NP / 2)));
        HIP_TRY(hipMemset(d.lm_hits, 0, sizeof(uint32_t) * B * (NP / 2)));
        HIP_TRY(hipMemset(d.sighted, 0, sizeof(uint8_t) * B * (NP / 2)));
        HIP_TRY(hipMemset(d.rejected, 0, sizeof(*d.rejected) * B)); // (the gates stay, like the parameters)
        std::vector<int> n(B, 3), fl(B, FLAG_INIT_X | FLAG_INIT_Z);
        std::vector<double> A(2 * B, 0.0);
        for (size_t b = 0; b < B; ++b)
                A[2 * b] = 1.0; // A = Identity
        HIP_TRY(hipMemcpy(d.n, n.data(), sizeof(int) * B, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d.flags, fl.data(), sizeof(int) * B, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d.A, A.data(), sizeof(double) * 2 * B, hipMemcpyHostToDevice));
        // a reset context is a fresh one: the scratch too (dev_alloc zeroes it; the kernels rely on never-written padding staying zero)
        hipError_t e = hipSuccess;
        for_each_scratch(c, [&](void *p, size_t bytes) {
                if (e == hipSuccess)
                        e = hipMemset(p, 0, B * bytes);
        });
        HIP_TRY(e);
        return seed_pose_block(c, P, B, NP);
}

/// one launch of a single-CU kernel with LDS layout L; `views`: what the kernel takes first (the device view; the UKF's scratch behind it)
template <typename L, typename K, typename... V>
int launch_small(K kern, int grid, hipStream_t st, int64_t t0, int nsteps, double *poses, int32_t *dims, StepArgs sa, StatsView sv, const V &...views)
{
        const size_t lds = L::total;
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(SMALL_WG), lds, st, views..., t0, nsteps, poses, dims, sa, sv);
        HIP_TRY(hipGetLastError());
        return ASLAM_OK;
}

/// f(std::integral_constant<int, NT>) for the tile count of a single-CU context: the small kernels are instantiated for 2, 5 and 9 tiles
template <typename F> auto with_NT(int NT, F &&f)
{
        return NT == 2 ? f(std::integral_constant<int, 2>{}) : NT == 5 ? f(std::integral_constant<int, 5>{}) : f(std::integral_constant<int, 9>{});
}

/// The ONE rule of which front-end instantiation a launch of seam MODE takes (FrontendVariant, ekf_large_launch.h): "gated" exists in the
/// replay seam alone, "sighted" on EKF contexts alone
template <int MODE> FrontendVariant frontend_variant(const aslam_ctx *c, const StatsView &sv)
{
        return {sv.any(), c->cfg.filter == ASLAM_EKF && c->sighted_on, MODE == MODE_REPLAY && c->gated()};
}

/// the flags of a single-CU kernel as the template arguments of its name in aslam_kernel_info, trailing defaults (false) left out as the code writes them
std::string variant_args(std::initializer_list<bool> flags)
{
        std::string s, pending;
        for (const bool f : flags)
                if (pending += f ? ",true" : ",false"; f)
                        s += std::exchange(pending, std::string());
        return s;
}

/// `sv`: the statistics this launch writes (all null: none).  The single-CU kernels have an instantiation of their own for it, the large-state
/// chains one more launch per callback (large_stats); without statistics both run exactly what they ran before.
template <int MODE>
int launch(aslam_ctx *c, int grid, int64_t t0, int nsteps, double *poses, int32_t *dims, StepArgs sa, hipStream_t st, StatsView sv = {})
{
        const FrontendVariant fv = frontend_variant<MODE>(c, sv);
#if ASLAM_HAVE_UKF
        if (c->large && c->cfg.filter == ASLAM_UKF)
        {
                HIP_TRY(launch_ukf_large<MODE>(c->lh, fv, c->dv, c->lv64, c->ukfl, c->skipped, t0, nsteps, poses, dims, sa, st, sv));
                return ASLAM_OK;
        }
#endif
        if (c->large)
                return with_large_view(c, [&](auto &lv) -> int {
                        HIP_TRY(launch_large<MODE>(c->lh, fv, c->dv, lv, c->skipped, t0, nsteps, poses, dims, sa, st, sv));
                        return ASLAM_OK;
                });
        if (c->cfg.filter == ASLAM_EKF)
                return with_NT(c->NT, [&](auto nt) {
                        constexpr int NT = decltype(nt)::value;
                        const auto kern = with_variant<true, true, MODE == MODE_REPLAY>(fv, [](auto stats, auto si, auto ga) {
                                return &ekf_small_kernel<NT, MODE, decltype(stats)::value, decltype(si)::value, decltype(ga)::value>;
                        });
                        return launch_small<SmallLayout<NT>>(kern, grid, st, t0, nsteps, poses, dims, sa, sv, c->dv);
                });
#if ASLAM_HAVE_UKF
        if (c->cfg.filter == ASLAM_UKF)
                return with_NT(c->NT, [&](auto nt) {
                        constexpr int NT = decltype(nt)::value;
                        const auto kern = with_variant<true, false, MODE == MODE_REPLAY>(
                                fv, [](auto stats, auto, auto ga) { return &ukf_small_kernel<NT, MODE, decltype(stats)::value, decltype(ga)::value>; });
                        return launch_small<UkfLayout<NT>>(kern, grid, st, t0, nsteps, poses, dims, sa, sv, c->dv, c->ukf);
                });
#endif
        return fail(ASLAM_ERR_UNSUPPORTED, "no kernel for this filter/size");
}

/// what the per-callback seams and aslam_replay write besides their own outputs: the last-callback record when it is switched on
StatsView innovation_view(const aslam_ctx *c)
{
        return StatsView{nullptr, nullptr, nullptr, c->innov_on ? c->innov : nullptr};
}

/// the record of every filter to NaN ("no callback yet")
int clear_innovation(aslam_ctx *c)
{
        if (!c->innov)
                return ASLAM_OK;
        const std::vector<double> nan(2 * (size_t)c->cfg.batch, std::nan(""));
        HIP_TRY(hipMemcpy(c->innov, nan.data(), sizeof(double) * nan.size(), hipMemcpyHostToDevice));
        return ASLAM_OK;
}

/// at least `bytes` of device staging for a maintenance call (the context is synchronised: nothing reads the old block).  When the block has
/// to grow, the first `keep` bytes of the old one are carried over; with keep = 0 the old block goes before the new one is allocated.
int snap_reserve(aslam_ctx *c, size_t bytes, size_t keep = 0)
{
        if (bytes <= c->snap_cap)
                return ASLAM_OK;
        if (!keep && c->snap_dev)
        {
                (void)hipFree(c->snap_dev);
                c->snap_dev = nullptr, c->snap_cap = 0;
        }
        void *q = nullptr;
        HIP_TRY(hipMalloc(&q, bytes));
        const hipError_t e = keep ? hipMemcpy(q, c->snap_dev, keep, hipMemcpyDeviceToDevice) : hipSuccess;
        if (e != hipSuccess)
        {
                (void)hipFree(q);
                HIP_TRY(e);
        }
        if (c->snap_dev)
                (void)hipFree(c->snap_dev);
        c->snap_dev = static_cast<char *>(q);
        c->snap_cap = bytes;
        return ASLAM_OK;
}

/// The layout of a call's staging in the context's block: sections in the order they are taken, each starting on a 64-byte boundary.  A
/// pointer from at() holds until the next reserve() that has to grow the block.
struct Staging
{
        aslam_ctx *c;
        size_t size = 0;
        size_t take(size_t bytes) { return std::exchange(size, size + (size_t)snap_pad64((int64_t)bytes)); }
        int reserve(size_t keep = 0) const { return snap_reserve(c, size, keep); }
        template <typename T> T *at(size_t off) const { return reinterpret_cast<T *>(c->snap_dev + off); }
};

/// rows a mask must have: the landmarks a filter of this context can hold, (max_landmark_count - 3) / 2 rounded up
int landmark_capacity(const aslam_ctx *c)
{
        return std::max(0, (c->cfg.max_landmark_count - 2) / 2);
}

/// empty, or which of the arguments the per-landmark calls share is refused; `noun`: what the call's array is, "mask" or "into"
std::string bad_mask(const aslam_ctx *c, const void *mask, int ld, int is_device, const char *noun)
{
        if (!c)
                return "null context";
        if (!mask)
                return std::string("null ") + noun;
        if (ld < landmark_capacity(c))
                return "ld is smaller than the context's landmark capacity, (max_landmark_count - 3) / 2 rounded up";
        if (is_device && ((uintptr_t)mask & 15))
                return std::string("a device ") + noun + " must be 16-byte aligned";
        return std::string();
}
} // namespace

extern "C" {

int aslam_abi_version(void)
{
        return ASLAM_ABI_VERSION;
}

const char *aslam_last_error(void)
{
        return g_err.c_str();
}

int aslam_create(const aslam_config *cfg, aslam_ctx **out)
{
        if (!cfg || !out)
                return fail(ASLAM_ERR_ARG, "null argument");
        *out = nullptr;
        if (cfg->filter != ASLAM_EKF && cfg->filter != ASLAM_UKF)
                return fail(ASLAM_ERR_ARG, "filter must be ASLAM_EKF or ASLAM_UKF");
        if (cfg->batch < 1 || cfg->max_landmark_count < 4 || cfg->max_obs < 1 || cfg->max_wait < 1)
                return fail(ASLAM_ERR_ARG, "batch, max_landmark_count, max_obs, max_wait must be positive");
        if (cfg->dtype != ASLAM_F64 && cfg->dtype != ASLAM_F32)
                return fail(ASLAM_ERR_ARG, "dtype must be ASLAM_F64 or ASLAM_F32");
        if (cfg->flags & ~(int32_t)ASLAM_CFG_UKF_LARGE)
                return fail(ASLAM_ERR_ARG, "unknown bit in flags");
        const int n_max = cfg->max_landmark_count - 1; // growth is refused at N >= MAX_LANDMARK_COUNT
        const int need = (n_max + 15) / 16;
        int NT = 0; // the smallest instantiated tile count that holds the state
        for (int cand : {9, 5, 2})
                if (cand >= need)
                        NT = cand;
        const bool large = (NT == 0) || cfg->dtype == ASLAM_F32; // fp32 exists on the multi-workgroup path only
        // rows of G behind the state rows: Y^T (EKF) / z^T and the innovation (UKF); they need room inside the padded dimension
        const int xrows = cfg->filter == ASLAM_UKF ? 2 : 1;
        if (large)
        {
                if (cfg->filter != ASLAM_EKF && (!(cfg->flags & ASLAM_CFG_UKF_LARGE) || cfg->dtype != ASLAM_F64 || !ASLAM_HAVE_UKF))
                        return fail(ASLAM_ERR_UNSUPPORTED, "the UKF is limited to state dimensions up to 143 (single-CU kernels) and fp64; "
                                                           "ASLAM_CFG_UKF_LARGE opts in to the fp64 launch chain beyond that");
                if (n_max + xrows > LARGE_NP_MAX)
                        return fail(ASLAM_ERR_UNSUPPORTED, cfg->filter == ASLAM_EKF ? "state dimension above 1087 is not supported"
                                                                                    : "UKF state dimension above 1085 (max_landmark_count above 1087) is not supported");
                if (cfg->max_obs > LARGE_OBS_CAP || cfg->max_wait > LARGE_WAIT_CAP)
                        return fail(ASLAM_ERR_UNSUPPORTED, "max_obs above 1024 / max_wait above 2048 are not supported");
        }
        else
        {
                if (cfg->max_obs > SMALL_OBS_CAP)
                        return fail(ASLAM_ERR_UNSUPPORTED, "max_obs above 128 is not supported by the single-CU kernels");
                if (cfg->max_wait > SMALL_WAIT_CAP)
                        return fail(ASLAM_ERR_UNSUPPORTED, "max_wait above 512 is not supported by the single-CU kernels");
        }
        HIP_TRY(hipSetDevice(cfg->device));

        aslam_ctx *c = new aslam_ctx();
        c->cfg = *cfg;
        c->large = large;
        c->NT = large ? 0 : NT;
        c->NP = large ? ((n_max + xrows + LB - 1) / LB) * LB : 16 * NT; // the large path needs spare rows (Y^T / z^T and the innovation ride in G)
        c->last_stream = nullptr;
        c->hbm_bytes = 0;
        std::memset(&c->dv, 0, sizeof(c->dv));
        DevView &d = c->dv;
        d.B = cfg->batch;
        d.NP = c->NP;
        d.dim_cap = cfg->max_landmark_count;
        d.max_obs = cfg->max_obs;
        d.max_wait = cfg->max_wait;
        const size_t B = (size_t)cfg->batch;
        int rc = ASLAM_OK;
        auto take = [&](auto *&p, size_t per, bool = false) { // (the one error idiom here: the first failure stops every later allocation)
                if (rc == ASLAM_OK)
                        rc = dev_alloc(c, &p, B * per, c->owned);
        };
        // what a large-state context owns where a single-CU context owns P: `skipped`, the streams of the stream groups, the typed view
        auto take_large = [&]() {
                take(c->skipped, 1);
                c->lh.knobs = large_knobs_from_env();
                for (hipStream_t &q : c->lh.aux)
                        if (hipStreamCreateWithFlags(&q, hipStreamNonBlocking) != hipSuccess)
                                rc = ASLAM_ERR_HIP;
                if (hipEventCreateWithFlags(&c->lh.ev_fork, hipEventDisableTiming) != hipSuccess)
                        rc = ASLAM_ERR_HIP;
                for (hipEvent_t &e : c->lh.ev_join)
                        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess)
                                rc = ASLAM_ERR_HIP;
                with_large_view(c, [&](auto &lv) {
                        const LargePlan plan = large_plan(c->cfg.dtype == ASLAM_F32, c->NP, c->cfg.batch, c->cfg.batch, c->lh.knobs);
                        lv.NP = c->NP;
                        lv.xrows = xrows;
                        for_each_array(lv, [&](auto *&p, size_t per, bool) {
                                const bool unused = (same_slot(p, lv.Lpl) && !plan.need_Lpl) || (same_slot(p, lv.Vw) && !plan.need_Vw);
                                if (!unused)
                                        take(p, per);
                        });
                        c->largeP = lv.P;
                        return 0;
                });
        };
        // Every view's arrays in the order of its for_each_array.  The order of the hipMalloc calls is as it was when the rates in profiles/ were
        // measured (addresses follow from it): the large-state arrays come where P would, step_in ([3][B]) behind A
        for_each_array(d, [&](auto *&p, size_t per, bool) {
                if (large && same_slot(p, d.P))
                        take_large();
                else if (same_slot(p, d.clock) || same_slot(p, d.lm_seen) || same_slot(p, d.lm_hits) || same_slot(p, d.sighted) || same_slot(p, d.gate) ||
                         same_slot(p, d.rejected))
                        rc = rc == ASLAM_OK ? dev_alloc(c, &p, B * per, c->owned, false) : rc; // (bookkeeping, outside the reported bytes)
                else
                        take(p, per);
                if (same_slot(p, d.A))
                        take(c->step_in, 3);
        });
        d.step_in = c->step_in;
        c->params_dev = const_cast<aslam_params *>(d.prm);
        c->params.assign(B, aslam_params ASLAM_PARAMS_DEFAULT_INIT);
        c->gates.assign(B, 0.0); // (dev_alloc zeroes dv.gate: the Euclidean rule)
        if (rc == ASLAM_OK && hipMemcpy(c->params_dev, c->params.data(), sizeof(aslam_params) * B, hipMemcpyHostToDevice) != hipSuccess)
                rc = fail(ASLAM_ERR_HIP, "hipMemcpy of the default parameters failed");
#ifdef ASLAM_STAMPS
        if (rc == ASLAM_OK) // [64 ..): diagnostic builds, last front-end launch, 100 MHz ticks per workgroup
                rc = dev_alloc(c, &d.dbg, 64 + 1024, c->owned);
#endif
#if ASLAM_HAVE_UKF
        if (cfg->filter == ASLAM_UKF)
        { // HBM scratch of the UKF kernels; MP >= 2 n + 5 rounded up to 16 for every n the context takes
                (large ? c->ukfl.MP : c->ukf.MP) = 2 * c->NP + 16;
                if (large)
                        for_each_array(c->ukfl, c->NP, take);
                else
                        for_each_array(c->ukf, c->NP, take);
        }
#else
        if (rc == ASLAM_OK && cfg->filter == ASLAM_UKF)
                rc = fail(ASLAM_ERR_UNSUPPORTED, "library built without the UKF kernels");
#endif
        int scratch = 0; // a view that gains a zero-at-start array may need a larger SnapCtx::clear
        for_each_scratch(c, [&](void *, size_t) { ++scratch; });
        if (rc == ASLAM_OK && scratch > SNAP_CLEAR_MAX)
                rc = fail(ASLAM_ERR_UNSUPPORTED, "more zero-at-start arrays than SnapCtx::clear holds (SNAP_CLEAR_MAX)");
        if (rc == ASLAM_OK)
                rc = init_state(c);
        if (rc != ASLAM_OK)
        {
                std::string keep = g_err;
                aslam_destroy(c);
                g_err = keep;
                return rc;
        }
        *out = c;
        return ASLAM_OK;
}

int aslam_destroy(aslam_ctx *c)
{
        if (!c)
                return ASLAM_OK;
        for (void *p : c->owned)
                (void)hipFree(p);
        for (void *p : c->trace_owned)
                (void)hipFree(p);
        if (c->snap_dev)
                (void)hipFree(c->snap_dev);
        if (c->stage_pin)
                (void)hipHostFree(c->stage_pin);
        for (void *p : c->stage_old)
                (void)hipHostFree(p);
        for (hipStream_t q : c->lh.aux)
                if (q)
                        (void)hipStreamDestroy(q);
        if (c->lh.ev_fork)
                (void)hipEventDestroy(c->lh.ev_fork);
        for (hipEvent_t e : c->lh.ev_join)
                if (e)
                        (void)hipEventDestroy(e);
        delete c;
        return ASLAM_OK;
}

int aslam_reset(aslam_ctx *c)
{
        if (!c)
                return fail(ASLAM_ERR_ARG, "null context");
        int rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        rc = init_state(c);
        return rc != ASLAM_OK ? rc : clear_innovation(c); // (the setting of aslam_innovation_enable and the parameters stay)
}

int aslam_params_default(aslam_params *out)
{
        if (!out)
                return fail(ASLAM_ERR_ARG, "null argument");
        *out = aslam_params ASLAM_PARAMS_DEFAULT_INIT;
        return ASLAM_OK;
}

int aslam_set_params(aslam_ctx *c, int traj, const aslam_params *p)
{
        if (!p)
                return fail(ASLAM_ERR_ARG, "null argument");
        // (the record is judged before the context is looked at: a refused field is reported whatever else is wrong with the call)
        if (const char *bad = bad_param(*p))
                return fail(ASLAM_ERR_ARG, std::string("aslam_params.") + bad +
                                                   (std::string(bad) == "promote_count" ? " must be at least 1"
                                                                                        : (bad[0] == 'q' ? " must be finite and >= 0" : " must be finite and > 0")));
        if (!c)
                return fail(ASLAM_ERR_ARG, "null context");
        if (traj < -1 || traj >= c->cfg.batch)
                return fail(ASLAM_ERR_ARG, "trajectory index out of range (-1 = every filter)");
        int rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        const size_t first = traj < 0 ? 0 : (size_t)traj, count = traj < 0 ? (size_t)c->cfg.batch : 1;
        const std::vector<aslam_params> recs(count, *p);
        HIP_TRY(hipMemcpy(c->params_dev + first, recs.data(), sizeof(aslam_params) * count, hipMemcpyHostToDevice));
        std::copy(recs.begin(), recs.end(), c->params.begin() + first); // (behind the copy: the host copy never disagrees with what the kernels read)
        return ASLAM_OK;
}

int aslam_set_replay_gate(aslam_ctx *c, int traj, double gate)
{
        if (!(gate >= 0.0)) // (a NaN fails the comparison)
                return fail(ASLAM_ERR_ARG, "aslam_set_replay_gate: gate must be 0 (the Euclidean rule) or positive (infinity allowed), not negative or NaN");
        if (!c)
                return fail(ASLAM_ERR_ARG, "aslam_set_replay_gate: null context");
        if (traj < -1 || traj >= c->cfg.batch)
                return fail(ASLAM_ERR_ARG, "aslam_set_replay_gate: traj out of range (-1 = every filter)");
        int rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        const size_t first = traj < 0 ? 0 : (size_t)traj, count = traj < 0 ? (size_t)c->cfg.batch : 1;
        const std::vector<double> g(count, gate);
        HIP_TRY(hipMemcpy(c->dv.gate + first, g.data(), sizeof(double) * count, hipMemcpyHostToDevice));
        std::copy(g.begin(), g.end(), c->gates.begin() + first); // (behind the copy: the host copy never disagrees with what the kernels read)
        return ASLAM_OK;
}

int aslam_get_replay_gate(aslam_ctx *c, int traj, double *gate)
{
        int rc = check_traj(c, traj);
        if (rc != ASLAM_OK)
                return rc;
        if (!gate)
                return fail(ASLAM_ERR_ARG, "aslam_get_replay_gate: null gate");
        if ((rc = sync_ctx(c)) != ASLAM_OK)
                return rc;
        HIP_TRY(hipMemcpy(gate, c->dv.gate + traj, sizeof(double), hipMemcpyDeviceToHost)); // (what the kernels read)
        return ASLAM_OK;
}

int aslam_get_assoc_rejected(aslam_ctx *c, int traj, uint64_t *count)
{
        int rc = check_traj(c, traj);
        if (rc != ASLAM_OK)
                return rc;
        if (!count)
                return fail(ASLAM_ERR_ARG, "aslam_get_assoc_rejected: null count");
        if ((rc = sync_ctx(c)) != ASLAM_OK)
                return rc;
        static_assert(sizeof(*c->dv.rejected) == sizeof(uint64_t), "the counter is 64 bits");
        HIP_TRY(hipMemcpy(count, c->dv.rejected + traj, sizeof(uint64_t), hipMemcpyDeviceToHost));
        return ASLAM_OK;
}

int aslam_get_params(aslam_ctx *c, int traj, aslam_params *p)
{
        int rc = check_traj(c, traj);
        if (rc != ASLAM_OK)
                return rc;
        if (!p)
                return fail(ASLAM_ERR_ARG, "null argument");
        if ((rc = sync_ctx(c)) != ASLAM_OK)
                return rc;
        HIP_TRY(hipMemcpy(p, c->params_dev + traj, sizeof(aslam_params), hipMemcpyDeviceToHost)); // (what the kernels read)
        return ASLAM_OK;
}

int aslam_set_state(aslam_ctx *c, int traj, int n, const double *X, const double *Z, const double *P)
{
        int rc = check_traj(c, traj);
        if (rc != ASLAM_OK)
                return rc;
        if (n < 3 || n >= c->cfg.max_landmark_count || ((n - 3) & 1))
                return fail(ASLAM_ERR_ARG, "n must be 3 + 2k and below max_landmark_count");
        rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        const size_t NP = (size_t)c->NP;
        DevView &d = c->dv;
        const double *src[2] = {X, Z};
        double *dst[2] = {d.X, d.Z};
        for (int i = 0; i < 2; ++i)
                if (src[i])
                {
                        std::vector<double> v(NP, 0.0);
                        std::memcpy(v.data(), src[i], sizeof(double) * n);
                        HIP_TRY(hipMemcpy(dst[i] + traj * NP, v.data(), sizeof(double) * NP, hipMemcpyHostToDevice));
                }
        if (P && (rc = upload_P(c, traj, n, P)) != ASLAM_OK)
                return rc;
        const int fl = 0; // a filter whose state was handed over is past both init flags
        int n_old = 0;
        HIP_TRY(hipMemcpy(&n_old, d.n + traj, sizeof(int), hipMemcpyDeviceToHost));
        if (n != n_old && (rc = resize_sightings(c, traj, n_old, n)) != ASLAM_OK)
                return rc;
        HIP_TRY(hipMemcpy(d.n + traj, &n, sizeof(int), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d.flags + traj, &fl, sizeof(int), hipMemcpyHostToDevice));
        return ASLAM_OK;
}

int aslam_grow(aslam_ctx *c, int traj, int n_new, const double *x_seed, const double *z_seed)
{
        int rc = check_traj(c, traj);
        if (rc != ASLAM_OK)
                return rc;
        rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        DevView &d = c->dv;
        int n_old = 0;
        HIP_TRY(hipMemcpy(&n_old, d.n + traj, sizeof(int), hipMemcpyDeviceToHost));
        if (n_new <= n_old || ((n_new - n_old) & 1) || !x_seed || !z_seed)
                return fail(ASLAM_ERR_ARG, "n_new must exceed the current dimension by an even amount; seeds required");
        if (n_new >= c->cfg.max_landmark_count)
        {
                // ekf.cpp:263-268: warn, keep N, drop the landmarks
                uint32_t st = 0;
                HIP_TRY(hipMemcpy(&st, d.status + traj, sizeof(st), hipMemcpyDeviceToHost));
                st |= ASLAM_ST_GROWTH_REFUSED;
                HIP_TRY(hipMemcpy(d.status + traj, &st, sizeof(st), hipMemcpyHostToDevice));
                return ASLAM_OK;
        }
        const size_t NP = (size_t)c->NP;
        const int k = n_new - n_old;
        HIP_TRY(hipMemcpy(d.X + traj * NP + n_old, x_seed, sizeof(double) * k, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d.Z + traj * NP + n_old, z_seed, sizeof(double) * k, hipMemcpyHostToDevice));
        // conservativeResizeLike(Identity * UKF_KP_LANDMARK_POSE): new rows (new columns of old rows are zero padding already)
        rc = grow_P_rows(c, traj, n_old, n_new);
        if (rc == ASLAM_OK)
                rc = resize_sightings(c, traj, n_old, n_new);
        if (rc != ASLAM_OK)
                return rc;
        HIP_TRY(hipMemcpy(d.n + traj, &n_new, sizeof(int), hipMemcpyHostToDevice));
        return ASLAM_OK;
}

namespace
{
/// one callback of one trajectory: Z (and the EKF's A) to the device, the launch, optional read-back of X (synchronises then)
/// `sighted`: the host's mask of this callback ([n_landmarks], aslam_ekf_step_sighted), or null: under the mode every landmark counts as sighted
int step_one(aslam_ctx *c, int filter, int traj, float vx, float az, float dt, const double *Z, const double *A, double *X_out, void *stream,
             const uint8_t *sighted = nullptr)
{
        int rc = check_traj(c, traj);
        if (rc != ASLAM_OK)
                return rc;
        if (c->cfg.filter != filter)
                return fail(ASLAM_ERR_STATE, filter == ASLAM_EKF ? "context was created for the UKF" : "context was created for the EKF");
        if (!Z)
                return fail(ASLAM_ERR_ARG, "Z is required");
        hipStream_t st = static_cast<hipStream_t>(stream);
        if ((rc = enter_stream(c, st)) != ASLAM_OK) // (before n is read: a growth may still be in flight on the last stream)
                return rc;
        DevView &d = c->dv;
        int n = 0;
        HIP_TRY(hipMemcpyAsync(&n, d.n + traj, sizeof(int), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const size_t NP = (size_t)c->NP;
        HIP_TRY(hipMemcpyAsync(d.Z + traj * NP, Z, sizeof(double) * n, hipMemcpyHostToDevice, st));
        if (A)
                HIP_TRY(hipMemcpyAsync(d.A + 2 * traj, A, 2 * sizeof(double), hipMemcpyHostToDevice, st));
        const size_t nlm = (size_t)(n - 3) / 2;
        if (sighted && nlm)
                HIP_TRY(hipMemcpyAsync(d.sighted + traj * (NP / 2), sighted, nlm, hipMemcpyHostToDevice, st));
        else if (c->sighted_on && filter == ASLAM_EKF && nlm)
                HIP_TRY(hipMemsetAsync(d.sighted + traj * (NP / 2), 1, nlm, st));
        StepArgs sa{traj, vx, az, dt};
        rc = launch<MODE_STEP>(c, 1, 0, 1, nullptr, nullptr, sa, st, innovation_view(c));
        if (rc != ASLAM_OK)
                return rc;
        if (X_out)
        {
                HIP_TRY(hipMemcpyAsync(X_out, d.X + traj * NP, sizeof(double) * n, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
        }
        return ASLAM_OK;
}
} // namespace

int aslam_ekf_step(aslam_ctx *c, int traj, float vx, float az, float dt, const double *Z, double a00, double a10,
                   double *X_out, void *stream)
{
        const double A[2] = {a00, a10};
        return step_one(c, ASLAM_EKF, traj, vx, az, dt, Z, A, X_out, stream);
}

int aslam_ukf_step(aslam_ctx *c, int traj, float vx, float az, float dt, const double *Z, double *X_out, void *stream)
{
        return step_one(c, ASLAM_UKF, traj, vx, az, dt, Z, nullptr, X_out, stream);
}

namespace
{
/// the batched per-callback seam: inputs of all filters to the device (asynchronously, straight from the caller's arrays), one launch
/// chain for the whole batch, optional read-back of X; no synchronisation
/// `sighted` [batch][lds]: as in step_one
int step_batch(aslam_ctx *c, int filter, const float *vx, const float *az, const float *dt, const double *Z, int ldz, const double *a00,
               const double *a10, double *X_out, int ldx, void *stream, const uint8_t *sighted = nullptr, int lds = 0)
{
        if (!c)
                return fail(ASLAM_ERR_ARG, "null context");
        if (c->cfg.filter != filter)
                return fail(ASLAM_ERR_STATE, "context was created for the other filter");
        if (!vx || !az || !dt || !Z || (filter == ASLAM_EKF && (!a00 || !a10)))
                return fail(ASLAM_ERR_ARG, "vx, az, dt, Z (and a00, a10 for the EKF) are required");
        const int B = c->cfg.batch, NP = c->NP;
        if (ldz < 3 || (X_out && ldx < 3))
                return fail(ASLAM_ERR_ARG, "row strides must cover the state");
        hipStream_t st = static_cast<hipStream_t>(stream);
        if (int rc = enter_stream(c, st); rc != ASLAM_OK)
                return rc;
        DevView &d = c->dv;
        HIP_TRY(hipMemcpyAsync(c->step_in, vx, sizeof(float) * B, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(c->step_in + B, az, sizeof(float) * B, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(c->step_in + 2 * (size_t)B, dt, sizeof(float) * B, hipMemcpyHostToDevice, st));
        const size_t wz = sizeof(double) * (size_t)std::min(ldz, NP);
        HIP_TRY(hipMemcpy2DAsync(d.Z, sizeof(double) * NP, Z, sizeof(double) * ldz, wz, B, hipMemcpyHostToDevice, st));
        if (filter == ASLAM_EKF)
        {
                HIP_TRY(hipMemcpy2DAsync(d.A, 2 * sizeof(double), a00, sizeof(double), sizeof(double), B, hipMemcpyHostToDevice, st));
                HIP_TRY(hipMemcpy2DAsync(d.A + 1, 2 * sizeof(double), a10, sizeof(double), sizeof(double), B, hipMemcpyHostToDevice, st));
        }
        if (sighted)
                HIP_TRY(hipMemcpy2DAsync(d.sighted, NP / 2, sighted, lds, (size_t)std::min(lds, NP / 2), B, hipMemcpyHostToDevice, st));
        else if (c->sighted_on && filter == ASLAM_EKF)
                HIP_TRY(hipMemsetAsync(d.sighted, 1, (size_t)B * (NP / 2), st)); // (the kernels read the entries of a filter's own landmarks alone)
        StepArgs sa{-1, 0.f, 0.f, 0.f};
        int rc = launch<MODE_STEP>(c, B, 0, 1, nullptr, nullptr, sa, st, innovation_view(c));
        if (rc != ASLAM_OK)
                return rc;
        if (X_out)
                HIP_TRY(hipMemcpy2DAsync(X_out, sizeof(double) * ldx, d.X, sizeof(double) * NP, sizeof(double) * (size_t)std::min(ldx, NP), B,
                                         hipMemcpyDeviceToHost, st));
        return ASLAM_OK;
}
} // namespace

int aslam_ekf_step_batch(aslam_ctx *c, const float *vx, const float *az, const float *dt, const double *Z, int ldz, const double *a00,
                         const double *a10, double *X_out, int ldx, void *stream)
{
        return step_batch(c, ASLAM_EKF, vx, az, dt, Z, ldz, a00, a10, X_out, ldx, stream);
}

int aslam_ekf_step_sighted(aslam_ctx *c, int traj, float vx, float az, float dt, const double *Z, const uint8_t *sighted, double a00, double a10,
                           double *X_out, void *stream)
{
        if (!sighted)
                return fail(ASLAM_ERR_ARG, "sighted is required");
        const double A[2] = {a00, a10};
        return step_one(c, ASLAM_EKF, traj, vx, az, dt, Z, A, X_out, stream, sighted);
}

int aslam_ekf_step_batch_sighted(aslam_ctx *c, const float *vx, const float *az, const float *dt, const double *Z, int ldz, const uint8_t *sighted,
                                 int ld, const double *a00, const double *a10, double *X_out, int ldx, void *stream)
{
        if (!sighted || ld < 1)
                return fail(ASLAM_ERR_ARG, "sighted with a positive row stride is required");
        return step_batch(c, ASLAM_EKF, vx, az, dt, Z, ldz, a00, a10, X_out, ldx, stream, sighted, ld);
}

int aslam_ukf_step_batch(aslam_ctx *c, const float *vx, const float *az, const float *dt, const double *Z, int ldz, double *X_out, int ldx,
                         void *stream)
{
        return step_batch(c, ASLAM_UKF, vx, az, dt, Z, ldz, nullptr, nullptr, X_out, ldx, stream);
}

int aslam_set_trace(aslam_ctx *c, const aslam_trace *tr)
{
        if (!c || !tr)
                return fail(ASLAM_ERR_ARG, "null argument");
        if (tr->T < 1 || tr->max_obs != c->cfg.max_obs)
                return fail(ASLAM_ERR_ARG, "trace must have T >= 1 and the context's max_obs");
        if (!tr->pose || !tr->yaw || !tr->twist || !tr->dt || !tr->obs_new || !tr->n_obs || !tr->obs)
                return fail(ASLAM_ERR_ARG, "trace arrays must all be given");
        int rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        for (void *p : c->trace_owned)
                (void)hipFree(p);
        c->trace_owned.clear();
        DevView &d = c->dv;
        d.T = tr->T;
        const size_t BT = (size_t)c->cfg.batch * (size_t)tr->T;
        if (tr->is_device)
        {
                d.tr_pose = tr->pose;
                d.tr_yaw = tr->yaw;
                d.tr_twist = tr->twist;
                d.tr_dt = tr->dt;
                d.tr_new = tr->obs_new;
                d.tr_nobs = tr->n_obs;
                d.tr_obs = tr->obs;
                return ASLAM_OK;
        }
        auto up = [&](const void *src, size_t bytes, const void **dst) -> int {
                void *q = nullptr;
                HIP_TRY(hipMalloc(&q, bytes));
                c->trace_owned.push_back(q);
                HIP_TRY(hipMemcpy(q, src, bytes, hipMemcpyHostToDevice));
                *dst = q;
                return ASLAM_OK;
        };
        const void *p = nullptr;
#define UP(field, src, bytes)                                                                                          \
        rc = up(src, bytes, &p);                                                                                       \
        if (rc != ASLAM_OK)                                                                                            \
                return rc;                                                                                             \
        d.field = static_cast<decltype(d.field)>(p);
        UP(tr_pose, tr->pose, BT * 2 * sizeof(double));
        UP(tr_yaw, tr->yaw, BT * sizeof(float));
        UP(tr_twist, tr->twist, BT * 2 * sizeof(double));
        UP(tr_dt, tr->dt, BT * sizeof(float));
        UP(tr_new, tr->obs_new, BT * sizeof(uint8_t));
        UP(tr_nobs, tr->n_obs, BT * sizeof(int32_t));
        UP(tr_obs, tr->obs, BT * (size_t)tr->max_obs * 2 * sizeof(float));
#undef UP
        return ASLAM_OK;
}

int aslam_replay(aslam_ctx *c, int64_t t0, int64_t nsteps, double *poses_out, int32_t *dims_out, void *stream)
{
        return aslam_replay_stats(c, t0, nsteps, poses_out, dims_out, nullptr, nullptr, nullptr, stream);
}

int aslam_replay_stats(aslam_ctx *c, int64_t t0, int64_t nsteps, double *poses_out, int32_t *dims_out, double *nis_out, double *logdet_out,
                       double *pose_cov_out, void *stream)
{
        if (!c)
                return fail(ASLAM_ERR_ARG, "null context");
        if (!c->dv.tr_pose)
                return fail(ASLAM_ERR_STATE, "no trace bound (aslam_set_trace)");
        if (t0 < 0 || nsteps < 1 || t0 + nsteps > c->dv.T || nsteps > 0x7fffffff)
                return fail(ASLAM_ERR_ARG, "step range outside the bound trace");
        hipStream_t st = static_cast<hipStream_t>(stream);
        if (int rc = enter_stream(c, st); rc != ASLAM_OK)
                return rc;
        StepArgs sa{0, 0.f, 0.f, 0.f};
        StatsView sv = innovation_view(c);
        sv.nis = nis_out, sv.logdet = logdet_out, sv.pcov = pose_cov_out;
        return launch<MODE_REPLAY>(c, c->cfg.batch, t0, (int)nsteps, poses_out, dims_out, sa, st, sv);
}

int aslam_innovation_enable(aslam_ctx *c, int on)
{
        if (!c)
                return fail(ASLAM_ERR_ARG, "null context");
        int rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        if (on && !c->innov && (rc = dev_alloc(c, &c->innov, 2 * (size_t)c->cfg.batch, c->owned)) != ASLAM_OK)
                return rc;
        // every switch from off to on starts from NaN: what a callback before the switch left behind is not "the last callback"
        if (on && !c->innov_on && (rc = clear_innovation(c)) != ASLAM_OK)
                return rc;
        c->innov_on = on != 0;
        return ASLAM_OK;
}

int aslam_sighted_update_enable(aslam_ctx *c, int on)
{
        if (!c)
                return fail(ASLAM_ERR_ARG, "null context");
        if (c->cfg.filter != ASLAM_EKF)
                return fail(ASLAM_ERR_UNSUPPORTED, "the sighted-only update exists for the EKF alone: the UKF contexts (either size) have no such mode");
        int rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        c->sighted_on = on != 0;
        return ASLAM_OK;
}

int aslam_get_sighted(aslam_ctx *c, int traj, uint8_t *sighted, int cap, int *n_landmarks)
{
        int n = 0;
        int rc = aslam_get_dim(c, traj, &n); // (checks the arguments and synchronises)
        if (rc != ASLAM_OK)
                return rc;
        const size_t H = (size_t)c->NP / 2;
        const int L = std::max(0, (n - 3) / 2), k = std::min(L, cap);
        if (sighted && cap > 0)
                std::memset(sighted, 0, (size_t)cap);
        if (sighted && k > 0)
                HIP_TRY(hipMemcpy(sighted, c->dv.sighted + traj * H, (size_t)k, hipMemcpyDeviceToHost));
        if (n_landmarks)
                *n_landmarks = L;
        return ASLAM_OK;
}

int aslam_get_innovation(aslam_ctx *c, int traj, double *nis, double *logdet)
{
        int rc = check_traj(c, traj);
        if (rc != ASLAM_OK)
                return rc;
        if (!c->innov_on)
                return fail(ASLAM_ERR_STATE, "the innovation record is off (aslam_innovation_enable)");
        rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        double v[2];
        HIP_TRY(hipMemcpy(v, c->innov + 2 * (size_t)traj, sizeof(v), hipMemcpyDeviceToHost));
        if (nis)
                *nis = v[0];
        if (logdet)
                *logdet = v[1];
        return ASLAM_OK;
}

int aslam_get_dim(aslam_ctx *c, int traj, int *n)
{
        int rc = check_traj(c, traj);
        if (rc != ASLAM_OK)
                return rc;
        if (!n)
                return fail(ASLAM_ERR_ARG, "null output");
        rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        HIP_TRY(hipMemcpy(n, c->dv.n + traj, sizeof(int), hipMemcpyDeviceToHost));
        return ASLAM_OK;
}

int aslam_get_state(aslam_ctx *c, int traj, double *X, double *Z, double *P)
{
        int n = 0;
        int rc = aslam_get_dim(c, traj, &n);
        if (rc != ASLAM_OK)
                return rc;
        const size_t NP = (size_t)c->NP;
        DevView &d = c->dv;
        if (X)
                HIP_TRY(hipMemcpy(X, d.X + traj * NP, sizeof(double) * n, hipMemcpyDeviceToHost));
        if (Z)
                HIP_TRY(hipMemcpy(Z, d.Z + traj * NP, sizeof(double) * n, hipMemcpyDeviceToHost));
        if (P)
                return download_P(c, traj, n, P);
        return ASLAM_OK;
}

int aslam_get_A(aslam_ctx *c, int traj, double *a00, double *a10)
{
        int rc = check_traj(c, traj);
        if (rc != ASLAM_OK)
                return rc;
        rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        double A[2];
        HIP_TRY(hipMemcpy(A, c->dv.A + 2 * traj, sizeof(A), hipMemcpyDeviceToHost));
        if (a00)
                *a00 = A[0];
        if (a10)
                *a10 = A[1];
        return ASLAM_OK;
}

int aslam_get_landmarks(aslam_ctx *c, int traj, double *x, double *y, int *n_landmarks)
{
        int n = 0;
        int rc = aslam_get_dim(c, traj, &n);
        if (rc != ASLAM_OK)
                return rc;
        std::vector<double> X(n);
        HIP_TRY(hipMemcpy(X.data(), c->dv.X + (size_t)traj * c->NP, sizeof(double) * n, hipMemcpyDeviceToHost));
        const int L = (n - 3) / 2;
        for (int i = 0; i < L; ++i)
        {
                if (x)
                        x[i] = X[3 + 2 * i];
                if (y)
                        y[i] = X[4 + 2 * i];
        }
        if (n_landmarks)
                *n_landmarks = L;
        return ASLAM_OK;
}

int aslam_get_wait(aslam_ctx *c, int traj, float *range, float *bearing, uint32_t *count, int cap, int *size)
{
        int rc = check_traj(c, traj);
        if (rc != ASLAM_OK)
                return rc;
        rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        DevView &d = c->dv;
        int wn = 0;
        HIP_TRY(hipMemcpy(&wn, d.wait_n + traj, sizeof(int), hipMemcpyDeviceToHost));
        if (size)
                *size = wn;
        const int k = wn < cap ? wn : cap;
        if (k > 0)
        {
                std::vector<float> rb(2 * (size_t)k);
                std::vector<uint32_t> cn(k);
                HIP_TRY(hipMemcpy(rb.data(), d.wait_rb + (size_t)traj * d.max_wait * 2, sizeof(float) * 2 * k, hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(cn.data(), d.wait_cnt + (size_t)traj * d.max_wait, sizeof(uint32_t) * k, hipMemcpyDeviceToHost));
                for (int i = 0; i < k; ++i)
                {
                        if (range)
                                range[i] = rb[2 * i];
                        if (bearing)
                                bearing[i] = rb[2 * i + 1];
                        if (count)
                                count[i] = cn[i];
                }
        }
        return ASLAM_OK;
}

int aslam_get_status(aslam_ctx *c, int traj, uint32_t *status_bits)
{
        int rc = check_traj(c, traj);
        if (rc != ASLAM_OK)
                return rc;
        if (!status_bits)
                return fail(ASLAM_ERR_ARG, "null output");
        rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        HIP_TRY(hipMemcpy(status_bits, c->dv.status + traj, sizeof(uint32_t), hipMemcpyDeviceToHost));
        return ASLAM_OK;
}

int aslam_get_sightings(aslam_ctx *c, int traj, uint32_t *last_seen, uint32_t *hits, int cap, int *n_landmarks, uint32_t *clock)
{
        int n = 0;
        int rc = aslam_get_dim(c, traj, &n);
        if (rc != ASLAM_OK)
                return rc;
        const DevView &d = c->dv;
        const size_t H = (size_t)c->NP / 2;
        const int L = std::max(0, (n - 3) / 2), k = std::min((int)H, cap); // (beyond L the stored record is zero, and is handed out as it is)
        if (last_seen && k > 0)
                HIP_TRY(hipMemcpy(last_seen, d.lm_seen + traj * H, sizeof(uint32_t) * k, hipMemcpyDeviceToHost));
        if (hits && k > 0)
                HIP_TRY(hipMemcpy(hits, d.lm_hits + traj * H, sizeof(uint32_t) * k, hipMemcpyDeviceToHost));
        if (clock)
                HIP_TRY(hipMemcpy(clock, d.clock + traj, sizeof(uint32_t), hipMemcpyDeviceToHost));
        if (n_landmarks)
                *n_landmarks = L;
        return ASLAM_OK;
}

int aslam_get_layout(aslam_ctx *c, int *padded_dim, int64_t *hbm_bytes)
{
        if (!c)
                return fail(ASLAM_ERR_ARG, "null context");
        if (padded_dim)
                *padded_dim = c->NP;
        if (hbm_bytes)
                *hbm_bytes = c->hbm_bytes;
        return ASLAM_OK;
}

/* ---- include/aslam_snapshot.h ------------------------------------------------------------------------------------- */
namespace
{
/// true where n cannot be the dimension of a filter of this context
bool bad_dimension(const aslam_ctx *c, int n)
{
        return n < 3 || !(n & 1) || n >= c->cfg.max_landmark_count || n > c->NP;
}

/// the descriptor of a record written from slot `slot`: the list sizes clamped to what the slot's lists hold; place_records sets the offset
SnapDesc slot_desc(const aslam_ctx *c, int slot, int n, int sens_n, int wait_n)
{
        return SnapDesc{0, slot, n, std::min(std::max(sens_n, 0), c->dv.max_obs), std::min(std::max(wait_n, 0), c->dv.max_wait), {0, 0}};
}

/// the blob the records of `desc` make, in their order: the offsets into desc; the blob's size and the largest dimension (the pack grid's) back
struct Placed
{
        int64_t total;
        int n_max;
};
Placed place_records(std::vector<SnapDesc> &desc)
{
        Placed p = {64 + snap_pad64(8 * (int64_t)desc.size()), 3};
        for (SnapDesc &d : desc)
        {
                d.off = p.total;
                p.total += snap_pad64(snap_record_bytes(d.n, d.sens_n, d.wait_n));
                p.n_max = std::max(p.n_max, d.n);
        }
        return p;
}

/// n, the init flags and the list sizes of the batch, on the host: one launch, one copy, one synchronisation on `st`; overwrites the staging
int fetch_filter_meta(aslam_ctx *c, hipStream_t st, std::vector<FilterMeta> &meta)
{
        const int B = c->cfg.batch;
        Staging s{c};
        const size_t o_meta = s.take(sizeof(FilterMeta) * B);
        if (int rc = s.reserve(); rc != ASLAM_OK)
                return rc;
        hipLaunchKernelGGL(filter_meta, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, (const int *)c->dv.n, (const int *)c->dv.flags,
                           (const int *)c->dv.sens_n, (const int *)c->dv.wait_n, B, s.at<FilterMeta>(o_meta));
        HIP_TRY(hipGetLastError());
        meta.resize((size_t)B);
        HIP_TRY(hipMemcpyAsync(meta.data(), s.at<FilterMeta>(o_meta), sizeof(FilterMeta) * B, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return ASLAM_OK;
}

/// the mask of the last callback of every slot of `desc` to zero: it indexes landmarks that are gone, have moved, or were never sighted there
int clear_sighted(aslam_ctx *c, const std::vector<SnapDesc> &desc, hipStream_t st)
{
        for (const SnapDesc &d : desc)
                HIP_TRY(hipMemsetAsync(c->dv.sighted + (size_t)d.slot * (c->NP / 2), 0, (size_t)c->NP / 2, st));
        return ASLAM_OK;
}

/// the context side of a pack / unpack launch.  clear[]: the slot-wise scratch aslam_reset zeroes, from the same list (for_each_scratch; at most
/// SNAP_CLEAR_MAX entries in one context: G, S, Vw of the large path, D, DZ, Tc, K of the single-CU UKF, D, DZ of the large-state UKF)
SnapCtx snap_ctx(aslam_ctx *c)
{
        const DevView &d = c->dv;
        SnapCtx s = {};
        s.NP = c->NP, s.max_obs = d.max_obs, s.max_wait = d.max_wait;
        s.X = d.X, s.Z = d.Z, s.P = c->large ? c->largeP : d.P, s.A = d.A;
        s.n = d.n, s.flags = d.flags, s.status = d.status;
        s.sens = d.sens, s.sens_n = d.sens_n, s.wait_rb = d.wait_rb, s.wait_cnt = d.wait_cnt, s.wait_n = d.wait_n;
        s.innov = c->innov;
        int k = 0;
        for_each_scratch(c, [&](void *p, size_t bytes) {
                if (k < SNAP_CLEAR_MAX) // (aslam_create refuses a context with more)
                        s.clear[k] = static_cast<char *>(p), s.clear_bytes[k] = bytes, ++k;
        });
        return s;
}
} // namespace

int64_t aslam_snapshot_record_bytes(int n, int sens_n, int wait_n)
{
        return snap_record_bytes(n, sens_n, wait_n);
}

int aslam_snapshot_check(const void *host_blob, int64_t bytes, int32_t *filter, int32_t *count)
{
        if (!host_blob)
                return fail(ASLAM_ERR_ARG, "null blob");
        const char *b = static_cast<const char *>(host_blob);
        SnapBlobHeader h;
        int64_t table_end = 0;
        if (bytes >= 64)
                std::memcpy(&h, b, 64);
        if (const char *e = snap_check_header(h, bytes, &table_end))
                return fail(ASLAM_ERR_ARG, std::string("snapshot: ") + e);
        for (uint32_t i = 0; i < h.count; ++i)
        {
                uint64_t off;
                std::memcpy(&off, b + 64 + 8 * (size_t)i, 8);
                const char *e = snap_check_offset(off, table_end, h.total_bytes);
                SnapRecHeader r;
                if (!e)
                {
                        std::memcpy(&r, b + off, 64);
                        e = snap_check_record(r, off, h.total_bytes);
                }
                if (e)
                        return fail(ASLAM_ERR_ARG, "snapshot record " + std::to_string(i) + ": " + e);
        }
        if (filter)
                *filter = (int32_t)h.filter;
        if (count)
                *count = (int32_t)h.count;
        return ASLAM_OK;
}

namespace
{
/// the records a snapshot of slots trajs[0 .. count) (null: slot i) holds, described and placed; the context is synchronised
int snap_describe(aslam_ctx *c, const int32_t *trajs, int count, hipStream_t st, std::vector<SnapDesc> &desc, Placed &placed)
{
        std::vector<FilterMeta> meta;
        if (int rc = fetch_filter_meta(c, st, meta); rc != ASLAM_OK)
                return rc;
        for (int i = 0; i < count; ++i)
        {
                const FilterMeta &m = meta[trajs ? trajs[i] : i];
                if (bad_dimension(c, m.n))
                        return fail(ASLAM_ERR_STATE, "a filter of the context has an invalid dimension");
                desc.push_back(slot_desc(c, trajs ? trajs[i] : i, m.n, m.sens_n, m.wait_n));
        }
        placed = place_records(desc);
        return ASLAM_OK;
}

/// the pack launch of a snapshot: records of `desc_dev` (count of them, the largest of dimension n_max) from the slots as they are
void launch_snapshot_pack(aslam_ctx *c, const SnapDesc *desc_dev, int count, const Placed &placed, char *out, hipStream_t st)
{
        hipLaunchKernelGGL(record_pack<SnapshotSrc>, snap_grid((int64_t)placed.n_max * (placed.n_max + 1) / 2, count), dim3(SNAP_WG), 0, st, snap_ctx(c),
                           desc_dev, count, (uint32_t)c->cfg.filter, (uint64_t)placed.total, SnapshotSrc{}, out);
}
} // namespace

int aslam_snapshot(aslam_ctx *c, const int32_t *trajs, int count, void *blob, int64_t cap_bytes, int is_device, int64_t *bytes_needed,
                   void *stream)
{
        if (!c)
                return fail(ASLAM_ERR_ARG, "null context");
        const int B = c->cfg.batch;
        if (!trajs)
                count = B;
        if (count < 1)
                return fail(ASLAM_ERR_ARG, "count must be positive");
        for (int i = 0; trajs && i < count; ++i)
                if (trajs[i] < 0 || trajs[i] >= B)
                        return fail(ASLAM_ERR_ARG, "trajectory index out of range");
        int rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        hipStream_t st = static_cast<hipStream_t>(stream);
        std::vector<SnapDesc> desc;
        Placed placed;
        if ((rc = snap_describe(c, trajs, count, st, desc, placed)) != ASLAM_OK)
                return rc;
        const int64_t total = placed.total;
        if (bytes_needed)
                *bytes_needed = total;
        if (!blob)
                return ASLAM_OK;
        if (cap_bytes < total)
                return fail(ASLAM_ERR_ARG, "blob capacity below the snapshot's size (" + std::to_string(total) + " bytes)");
        if (is_device && ((uintptr_t)blob & 15))
                return fail(ASLAM_ERR_ARG, "a device blob must be 16-byte aligned");
        // staging: descriptors | the records of a host blob
        Staging s{c};
        const size_t o_desc = s.take(sizeof(SnapDesc) * count), o_blob = s.take(is_device ? 0 : (size_t)total);
        if ((rc = s.reserve()) != ASLAM_OK)
                return rc;
        HIP_TRY(hipMemcpy(s.at<SnapDesc>(o_desc), desc.data(), sizeof(SnapDesc) * count, hipMemcpyHostToDevice));
        char *out = is_device ? static_cast<char *>(blob) : s.at<char>(o_blob);
        c->last_stream = st;
        launch_snapshot_pack(c, s.at<SnapDesc>(o_desc), count, placed, out, st);
        HIP_TRY(hipGetLastError());
        if (!is_device)
        {
                HIP_TRY(hipMemcpyAsync(blob, out, (size_t)total, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
        }
        return ASLAM_OK;
}

namespace
{
/// The blob header, the offset table and every record header of a blob, validated, on the host (aslam_restore, aslam_join_maps).  A device
/// blob's come through `st`: the blob header, the offset table, and all record headers through one gather launch -- three small copies, each
/// followed by a synchronisation of `st`; the gather stages at the front of the context's block, which no caller holds data in by then.
int snap_headers(aslam_ctx *c, const void *blob, int64_t bytes, int is_device, hipStream_t st, SnapBlobHeader &h,
                 std::vector<uint64_t> &table, std::vector<SnapRecHeader> &recs)
{
        int rc;
        const char *b = static_cast<const char *>(blob);
        int64_t table_end = 0;
        if (!is_device)
        {
                int32_t cnt = 0;
                if ((rc = aslam_snapshot_check(blob, bytes, nullptr, &cnt)) != ASLAM_OK)
                        return rc;
                std::memcpy(&h, b, 64);
                table.resize(cnt), recs.resize(cnt);
                for (int i = 0; i < cnt; ++i)
                {
                        std::memcpy(&table[i], b + 64 + 8 * (size_t)i, 8);
                        std::memcpy(&recs[i], b + table[i], 64);
                }
                return ASLAM_OK;
        }
        if (bytes >= 64)
        {
                HIP_TRY(hipMemcpyAsync(&h, b, 64, hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
        }
        if (const char *e = snap_check_header(h, bytes, &table_end))
                return fail(ASLAM_ERR_ARG, std::string("snapshot: ") + e);
        const size_t cnt = h.count;
        table.resize(cnt), recs.resize(cnt);
        if (!cnt)
                return ASLAM_OK;
        HIP_TRY(hipMemcpyAsync(table.data(), b + 64, 8 * cnt, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t i = 0; i < cnt; ++i)
                if (const char *e = snap_check_offset(table[i], table_end, h.total_bytes))
                        return fail(ASLAM_ERR_ARG, "snapshot record " + std::to_string(i) + ": " + e);
        // one gather launch through the validated table, one copy
        Staging s{c};
        const size_t o_table = s.take(8 * cnt), o_recs = s.take(64 * cnt);
        if ((rc = s.reserve()) != ASLAM_OK)
                return rc;
        uint64_t *tdev = s.at<uint64_t>(o_table);
        SnapRecHeader *hdev = s.at<SnapRecHeader>(o_recs);
        HIP_TRY(hipMemcpyAsync(tdev, table.data(), 8 * cnt, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(snapshot_gather, dim3((unsigned)((4 * cnt + SNAP_WG - 1) / SNAP_WG)), dim3(SNAP_WG), 0, st, b, tdev, (int)cnt, hdev);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(recs.data(), hdev, 64 * cnt, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t i = 0; i < cnt; ++i)
                if (const char *e = snap_check_record(recs[i], table[i], h.total_bytes))
                        return fail(ASLAM_ERR_ARG, "snapshot record " + std::to_string(i) + ": " + e);
        return ASLAM_OK;
}
} // namespace

int aslam_restore(aslam_ctx *c, const int32_t *records, const int32_t *trajs, int count, const void *blob, int64_t bytes, int is_device,
                  void *stream)
{
        if (!c || !blob)
                return fail(ASLAM_ERR_ARG, "null argument");
        if (count < 1 || count > c->cfg.batch)
                return fail(ASLAM_ERR_ARG, "count must be 1 .. batch (a slot is restored once)");
        if (is_device && ((uintptr_t)blob & 15))
                return fail(ASLAM_ERR_ARG, "a device blob must be 16-byte aligned");
        int rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        hipStream_t st = static_cast<hipStream_t>(stream);

        // ---- the headers, on the host
        SnapBlobHeader h;
        std::vector<uint64_t> table;
        std::vector<SnapRecHeader> recs;
        if ((rc = snap_headers(c, blob, bytes, is_device, st, h, table, recs)) != ASLAM_OK)
                return rc;

        // ---- the request against the context
        if ((int32_t)h.filter != c->cfg.filter)
                return fail(ASLAM_ERR_ARG, "the snapshot holds the other filter kind (EKF / UKF)");
        std::vector<SnapDesc> desc(count);
        std::vector<char> seen(c->cfg.batch, 0);
        for (int i = 0; i < count; ++i)
        {
                const int r = records ? records[i] : i, t = trajs ? trajs[i] : i;
                if (r < 0 || (size_t)r >= recs.size())
                        return fail(ASLAM_ERR_ARG, "record index out of range");
                if (t < 0 || t >= c->cfg.batch)
                        return fail(ASLAM_ERR_ARG, "trajectory index out of range");
                if (seen[t]++)
                        return fail(ASLAM_ERR_ARG, "a slot is named twice");
                const SnapRecHeader &q = recs[r];
                if (q.n >= c->cfg.max_landmark_count)
                        return fail(ASLAM_ERR_UNSUPPORTED, "record " + std::to_string(r) + ": state dimension " + std::to_string(q.n) +
                                                               " does not fit below the context's max_landmark_count");
                if (q.sens_n > c->cfg.max_obs)
                        return fail(ASLAM_ERR_UNSUPPORTED, "record " + std::to_string(r) + ": stored sensor message beyond the context's max_obs");
                if (q.wait_n > c->cfg.max_wait)
                        return fail(ASLAM_ERR_UNSUPPORTED, "record " + std::to_string(r) + ": wait-list beyond the context's max_wait");
                desc[i] = SnapDesc{(int64_t)table[r], t, q.n, q.sens_n, q.wait_n, {0, 0}};
        }

        // ---- one unpack launch; staging: descriptors | a host blob's copy
        Staging s{c};
        const size_t o_desc = s.take(sizeof(SnapDesc) * count), o_blob = s.take(is_device ? 0 : (size_t)h.total_bytes);
        if ((rc = s.reserve()) != ASLAM_OK)
                return rc;
        SnapDesc *ddev = s.at<SnapDesc>(o_desc);
        HIP_TRY(hipMemcpy(ddev, desc.data(), sizeof(SnapDesc) * count, hipMemcpyHostToDevice));
        const char *src = static_cast<const char *>(blob);
        if (!is_device)
        {
                HIP_TRY(hipMemcpy(s.at<char>(o_blob), blob, (size_t)h.total_bytes, hipMemcpyHostToDevice));
                src = s.at<char>(o_blob);
        }
        c->last_stream = st;
        hipLaunchKernelGGL(snapshot_unpack, snap_grid((int64_t)c->NP * c->NP / 2, count), dim3(SNAP_WG), 0, st, snap_ctx(c), ddev, count, src);
        HIP_TRY(hipGetLastError());
        // (format v1 does not carry the sighting record: the restored slots start at clock 0, every landmark at age 0)
        hipLaunchKernelGGL(sight_clear, dim3((unsigned)count), dim3(PRUNE_WAVE), 0, st, ddev, c->NP, c->dv.clock, c->dv.lm_seen, c->dv.lm_hits);
        HIP_TRY(hipGetLastError());
        // (nor the mask of the last callback, nor the count of gated-out observations; the slot's gate stays)
        if ((rc = clear_sighted(c, desc, st)) != ASLAM_OK)
                return rc;
        for (const SnapDesc &d : desc)
                HIP_TRY(hipMemsetAsync(c->dv.rejected + d.slot, 0, sizeof(*c->dv.rejected), st));
        return ASLAM_OK;
}

/* ---- joining maps (join.h) -------------------------------------------------------------------------------------------- */
int aslam_join_maps(aslam_ctx *c, const int32_t *records, const int32_t *trajs, int count, const void *blob, int64_t bytes, int is_device,
                    const aslam_frame *frames, const uint8_t *select, int ld, int32_t *joined_out, void *stream)
{
        static_assert(sizeof(aslam_frame) == 96, "aslam_frame is part of the C ABI");
        const std::string who = "aslam_join_maps: ";
        if (!c || !blob)
                return fail(ASLAM_ERR_ARG, who + "null argument");
        const int B = c->cfg.batch;
        if (count < 1 || count > B)
                return fail(ASLAM_ERR_ARG, who + "count must be 1 .. batch (a slot is joined into once)");
        if (is_device && ((uintptr_t)blob & 15))
                return fail(ASLAM_ERR_ARG, who + "a device blob must be 16-byte aligned");
        int rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        hipStream_t st = static_cast<hipStream_t>(stream);

        // ---- the headers, on the host (the blob's filter kind is not compared: a map is X and P)
        SnapBlobHeader h;
        std::vector<uint64_t> table;
        std::vector<SnapRecHeader> recs;
        if ((rc = snap_headers(c, blob, bytes, is_device, st, h, table, recs)) != ASLAM_OK)
                return rc;

        // ---- the request: indices, slots, the selection and the frames
        struct Entry
        {
                int rec, slot;
                std::vector<int32_t> idx;
        };
        std::vector<Entry> ent(count);
        std::vector<char> seen(B, 0);
        for (int i = 0; i < count; ++i)
        {
                const int r = records ? records[i] : i, t = trajs ? trajs[i] : i;
                if (r < 0 || (size_t)r >= recs.size())
                        return fail(ASLAM_ERR_ARG, who + "records[" + std::to_string(i) + "]: record index out of range");
                if (t < 0 || t >= B)
                        return fail(ASLAM_ERR_ARG, who + "trajs[" + std::to_string(i) + "]: trajectory index out of range");
                if (seen[t]++)
                        return fail(ASLAM_ERR_ARG, who + "trajs[" + std::to_string(i) + "]: a slot is named twice");
                const int L_B = (recs[r].n - 3) / 2;
                if (select && ld < L_B)
                        return fail(ASLAM_ERR_ARG, who + "ld is smaller than the " + std::to_string(L_B) + " landmarks of the record of entry " + std::to_string(i));
                ent[i].rec = r, ent[i].slot = t;
                for (int k = 0; k < L_B; ++k)
                        if (!select || select[(size_t)i * ld + k])
                                ent[i].idx.push_back(k);
                if (!frames)
                        continue;
                const aslam_frame &f = frames[i];
                const std::string fr = who + "frames[" + std::to_string(i) + "]";
                if (!std::isfinite(f.tx) || !std::isfinite(f.ty) || !std::isfinite(f.phi))
                        return fail(ASLAM_ERR_ARG, fr + (!std::isfinite(f.tx) ? ".tx" : !std::isfinite(f.ty) ? ".ty" : ".phi") + " is not finite");
                for (int k = 0; k < 9; ++k)
                        if (!std::isfinite(f.cov[k]))
                                return fail(ASLAM_ERR_ARG, fr + ".cov[" + std::to_string(k) + "] is not finite");
                if (f.cov[1] != f.cov[3] || f.cov[2] != f.cov[6] || f.cov[5] != f.cov[7])
                        return fail(ASLAM_ERR_ARG, fr + ".cov is not exactly symmetric");
                for (int k = 0; k < 9; k += 4)
                        if (f.cov[k] < 0.0)
                                return fail(ASLAM_ERR_ARG, fr + ".cov[" + std::to_string(k) + "] is negative");
        }

        // ---- n, the init flags and the list sizes of the batch: the one copy and the one synchronisation of the call
        const DevView &dv = c->dv;
        std::vector<FilterMeta> meta;
        if ((rc = fetch_filter_meta(c, st, meta)) != ASLAM_OK)
                return rc;
        for (const Entry &e : ent)
        {
                const FilterMeta &m = meta[e.slot];
                if (bad_dimension(c, m.n))
                        return fail(ASLAM_ERR_STATE, who + "filter " + std::to_string(e.slot) + " has an invalid dimension");
                if (m.flags & FLAG_INIT_X)
                        return fail(ASLAM_ERR_STATE, who + "filter " + std::to_string(e.slot) + " has not run a callback yet (init_x is set: the first one "
                                                                                                   "would overwrite X with Z)");
        }
        for (const Entry &e : ent)
                if ((int64_t)meta[e.slot].n + 2 * (int64_t)e.idx.size() >= c->cfg.max_landmark_count)
                        return fail(ASLAM_ERR_UNSUPPORTED, who + "filter " + std::to_string(e.slot) + ": state dimension " + std::to_string(meta[e.slot].n) + " + " +
                                                                   std::to_string(2 * e.idx.size()) + " does not fit below the context's max_landmark_count");

        // ---- the descriptors of the entries that join something (the others leave their slot untouched)
        std::vector<SnapDesc> desc;
        std::vector<JoinDesc> jdesc;
        std::vector<int32_t> idx;
        for (int i = 0; i < count; ++i)
        {
                const Entry &e = ent[i];
                if (joined_out)
                        joined_out[i] = (int32_t)e.idx.size();
                if (e.idx.empty())
                        continue;
                const FilterMeta &m = meta[e.slot];
                desc.push_back(slot_desc(c, e.slot, m.n + 2 * (int)e.idx.size(), m.sens_n, m.wait_n));
                JoinDesc j = {};
                j.src_off = (int64_t)table[e.rec];
                j.n_A = m.n, j.m = (int32_t)e.idx.size(), j.ld_B = recs[e.rec].n + 1, j.idx_off = (int32_t)idx.size();
                j.c = 1.0, j.s = 0.0;
                if (frames)
                {
                        const aslam_frame &f = frames[i];
                        j.c = std::cos(f.phi), j.s = std::sin(f.phi), j.tx = f.tx, j.ty = f.ty;
                        std::copy(f.cov, f.cov + 9, j.cov);
                }
                jdesc.push_back(j);
                idx.insert(idx.end(), e.idx.begin(), e.idx.end());
        }
        const int joined = (int)desc.size();
        if (joined == 0)
                return ASLAM_OK;
        const Placed placed = place_records(desc);

        // ---- staging: descriptors | join descriptors | index lists | a host blob's copy | the records; then pack, unpack, the sighting record
        Staging s{c};
        const size_t o_desc = s.take(sizeof(SnapDesc) * joined), o_jd = s.take(sizeof(JoinDesc) * joined), o_idx = s.take(sizeof(int32_t) * idx.size());
        const size_t o_src = s.take(is_device ? 0 : (size_t)h.total_bytes), o_blob = s.take((size_t)placed.total);
        if ((rc = s.reserve()) != ASLAM_OK)
                return rc;
        const SnapDesc *ddev = s.at<SnapDesc>(o_desc);
        const JoinDesc *jdev = s.at<JoinDesc>(o_jd);
        HIP_TRY(hipMemcpy(s.at<SnapDesc>(o_desc), desc.data(), sizeof(SnapDesc) * joined, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s.at<JoinDesc>(o_jd), jdesc.data(), sizeof(JoinDesc) * joined, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(s.at<int32_t>(o_idx), idx.data(), sizeof(int32_t) * idx.size(), hipMemcpyHostToDevice));
        const char *src = static_cast<const char *>(blob);
        if (!is_device)
        {
                HIP_TRY(hipMemcpy(s.at<char>(o_src), blob, (size_t)h.total_bytes, hipMemcpyHostToDevice));
                src = s.at<char>(o_src);
        }
        char *out = s.at<char>(o_blob);
        const SnapCtx sc = snap_ctx(c);
        c->last_stream = st;
        hipLaunchKernelGGL(join_pack, snap_grid((int64_t)placed.n_max * (placed.n_max + 1) / 2, joined), dim3(SNAP_WG), 0, st, sc, ddev, jdev,
                           (const int32_t *)s.at<int32_t>(o_idx), joined, (uint32_t)c->cfg.filter, (uint64_t)placed.total, src, out);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(snapshot_unpack, snap_grid((int64_t)c->NP * c->NP / 2, joined), dim3(SNAP_WG), 0, st, sc, ddev, joined, (const char *)out);
        HIP_TRY(hipGetLastError());
        // the new landmarks enter the sighting record as aslam_grow enters them; the clock and the old records stay
        hipLaunchKernelGGL(sight_extend, dim3((unsigned)joined), dim3(PRUNE_WAVE), 0, st, ddev, jdev, c->NP, (const uint32_t *)dv.clock, dv.lm_seen,
                           dv.lm_hits);
        HIP_TRY(hipGetLastError());
        // the mask of the last callback, as after aslam_remove_landmarks
        return clear_sighted(c, desc, st);
}

/* ---- removing landmarks (prune.h) ------------------------------------------------------------------------------------ */
int aslam_select_beyond(aslam_ctx *c, const double *max_range, uint8_t *mask_dev, int ld, void *stream)
{
        if (const std::string e = bad_mask(c, mask_dev, ld, 1, "mask"); !e.empty())
                return fail(ASLAM_ERR_ARG, "aslam_select_beyond: " + e);
        if (!max_range)
                return fail(ASLAM_ERR_ARG, "aslam_select_beyond: null max_range");
        const int B = c->cfg.batch;
        std::vector<double> r2((size_t)B);
        for (int b = 0; b < B; ++b)
        {
                if (!std::isfinite(max_range[b]) || max_range[b] <= 0.0)
                        return fail(ASLAM_ERR_ARG, "aslam_select_beyond: max_range[" + std::to_string(b) + "] must be finite and positive");
                r2[b] = max_range[b] * max_range[b];
        }
        int rc = sync_ctx(c);
        if (rc == ASLAM_OK)
                rc = snap_reserve(c, (size_t)snap_pad64(8 * (int64_t)B));
        if (rc != ASLAM_OK)
                return rc;
        hipStream_t st = static_cast<hipStream_t>(stream);
        c->last_stream = st;
        if ((rc = stage_host(c, c->snap_dev, r2.data(), sizeof(double) * B, st)) != ASLAM_OK)
                return rc;
        hipLaunchKernelGGL(prune_select_beyond, dim3((unsigned)B), dim3(PRUNE_WAVE), 0, st, (const double *)c->dv.X, (const int *)c->dv.n, c->NP,
                           reinterpret_cast<const double *>(c->snap_dev), mask_dev, ld);
        HIP_TRY(hipGetLastError());
        return ASLAM_OK;
}

int aslam_select_stale(aslam_ctx *c, const uint32_t *max_age, uint8_t *mask_dev, int ld, void *stream)
{
        if (const std::string e = bad_mask(c, mask_dev, ld, 1, "mask"); !e.empty())
                return fail(ASLAM_ERR_ARG, "aslam_select_stale: " + e);
        if (!max_age)
                return fail(ASLAM_ERR_ARG, "aslam_select_stale: null max_age");
        const int B = c->cfg.batch;
        int rc = sync_ctx(c);
        if (rc == ASLAM_OK)
                rc = snap_reserve(c, (size_t)snap_pad64(4 * (int64_t)B));
        if (rc != ASLAM_OK)
                return rc;
        hipStream_t st = static_cast<hipStream_t>(stream);
        c->last_stream = st;
        if ((rc = stage_host(c, c->snap_dev, max_age, sizeof(uint32_t) * B, st)) != ASLAM_OK)
                return rc;
        hipLaunchKernelGGL(prune_select_stale, dim3((unsigned)B), dim3(PRUNE_WAVE), 0, st, (const uint32_t *)c->dv.clock, (const uint32_t *)c->dv.lm_seen,
                           (const int *)c->dv.n, c->NP, reinterpret_cast<const uint32_t *>(c->snap_dev), mask_dev, ld);
        HIP_TRY(hipGetLastError());
        return ASLAM_OK;
}

namespace
{
/// a mask on the device: a pointer, or (null) the mask at offset `off` of the context's staging block, wherever the block lies by then
struct DevMask
{
        const uint8_t *ptr = nullptr;
        size_t off = 0;
        const uint8_t *get(const Staging &s) const { return ptr ? ptr : s.at<uint8_t>(off); }
};

/// the remove path's own front part of the staging: descriptors | what prune_map reports | the survivor lists.  A caller that launches work
/// on its own sections before remove_landmarks_at takes these too before it reserves, so that the block does not move under that work.
struct RemoveFront
{
        size_t desc, meta, src;
};
RemoveFront remove_front(Staging &s)
{
        const size_t B = (size_t)s.c->cfg.batch;
        return RemoveFront{s.take(sizeof(SnapDesc) * B), s.take(sizeof(PruneMeta) * B), s.take(sizeof(int) * (size_t)s.c->NP * B)};
}

/// aslam_remove_landmarks behind its argument checks and the synchronisation of the context.  `s`: the sections the caller holds in the
/// staging block (aslam_merge_landmarks: its plan, with the mask among them), which survive; this call's sections follow them.  The mask is
/// `host_mask` or, when that is null, `mask`.  meta_out (may be null) receives what prune_map reported: n and n_new of every filter.
int remove_landmarks_at(aslam_ctx *c, Staging s, DevMask mask, const uint8_t *host_mask, int ld, hipStream_t st, std::vector<PruneMeta> *meta_out)
{
        int rc;
        const int B = c->cfg.batch;
        // staging: descriptors | what prune_map reports | the survivor lists | a host mask's copy | the records
        const size_t held = s.size;
        const RemoveFront o = remove_front(s);
        if (host_mask)
                mask = DevMask{nullptr, s.take((size_t)B * ld)};
        if ((rc = s.reserve(held)) != ASLAM_OK)
                return rc;
        if (host_mask)
                HIP_TRY(hipMemcpy(s.at<uint8_t>(mask.off), host_mask, (size_t)B * ld, hipMemcpyHostToDevice));
        c->last_stream = st;
        hipLaunchKernelGGL(prune_map, dim3((unsigned)B), dim3(PRUNE_WAVE), 0, st, mask.get(s), ld, (const int *)c->dv.n, (const int *)c->dv.sens_n,
                           (const int *)c->dv.wait_n, c->NP, s.at<int>(o.src), s.at<PruneMeta>(o.meta));
        HIP_TRY(hipGetLastError());
        // the one copy and the one synchronisation of the call: n, n_new and the list sizes of the batch
        std::vector<PruneMeta> meta((size_t)B);
        HIP_TRY(hipMemcpyAsync(meta.data(), s.at<PruneMeta>(o.meta), sizeof(PruneMeta) * B, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (meta_out)
                *meta_out = meta;
        std::vector<SnapDesc> desc;
        for (int b = 0; b < B; ++b)
        {
                const PruneMeta &m = meta[b];
                if (bad_dimension(c, m.n))
                        return fail(ASLAM_ERR_STATE, "a filter of the context has an invalid dimension");
                if (m.n_new < 3 || !(m.n_new & 1) || m.n_new > m.n)
                        return fail(ASLAM_ERR_STATE, "aslam_remove_landmarks: the survivor count of filter " + std::to_string(b) + " is invalid");
                if (m.n_new == m.n)
                        continue; // loses nothing: not touched at all
                desc.push_back(slot_desc(c, b, m.n_new, m.sens_n, m.wait_n));
        }
        const int count = (int)desc.size();
        if (count == 0)
                return ASLAM_OK;
        const Placed placed = place_records(desc);
        // (the records' size is known only now: the block may move once more, with everything in front of the records; the mask is not read again)
        const size_t o_blob = s.take((size_t)placed.total);
        if ((rc = s.reserve(o_blob)) != ASLAM_OK)
                return rc;
        HIP_TRY(hipMemcpy(s.at<SnapDesc>(o.desc), desc.data(), sizeof(SnapDesc) * count, hipMemcpyHostToDevice));
        const SnapDesc *ddev = s.at<SnapDesc>(o.desc);
        char *blob = s.at<char>(o_blob);
        const SnapCtx sc = snap_ctx(c);
        PruneSrc ps = {};
        ps.src = s.at<int>(o.src); // (s, the slot's list, is set per record)
        hipLaunchKernelGGL(record_pack<PruneSrc>, snap_grid((int64_t)placed.n_max * (placed.n_max + 1) / 2, count), dim3(SNAP_WG), 0, st, sc, ddev, count,
                           (uint32_t)c->cfg.filter, (uint64_t)placed.total, ps, blob);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(snapshot_unpack, snap_grid((int64_t)c->NP * c->NP / 2, count), dim3(SNAP_WG), 0, st, sc, ddev, count, (const char *)blob);
        HIP_TRY(hipGetLastError());
        // the sighting record follows its landmarks; the clock stays (a restore clears both, a prune must not: the kernel is launched here, not in the unpack)
        hipLaunchKernelGGL(sight_compact, dim3((unsigned)B), dim3(PRUNE_WAVE), 0, st, (const int *)s.at<int>(o.src), (const PruneMeta *)s.at<PruneMeta>(o.meta),
                           c->NP, c->dv.lm_seen, c->dv.lm_hits);
        HIP_TRY(hipGetLastError());
        // the mask of the last callback indexes landmarks that have moved: zero in every filter that lost one
        return clear_sighted(c, desc, st);
}
} // namespace

int aslam_remove_landmarks(aslam_ctx *c, const uint8_t *mask, int ld, int is_device, void *stream)
{
        if (const std::string e = bad_mask(c, mask, ld, is_device, "mask"); !e.empty())
                return fail(ASLAM_ERR_ARG, "aslam_remove_landmarks: " + e);
        int rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        return remove_landmarks_at(c, Staging{c}, is_device ? DevMask{mask, 0} : DevMask{}, is_device ? nullptr : mask, ld, static_cast<hipStream_t>(stream),
                                   nullptr);
}

/* ---- merging duplicate landmarks (merge.h) ----------------------------------------------------------------------------- */
namespace
{
/// what the plan stage of a merge leaves behind (the pointers into the staging block hold until the remove path reserves its records)
struct MergePlan
{
        Staging s;     // the call's own sections ...
        size_t o_mask; // ... and the removal mask among them
        hipStream_t st;
        MergeMeta *meta_dev;
        int32_t *pi, *pj, *stop;
        uint8_t *mask;
        double *V, *P;
        std::vector<MergeMeta> meta;
        int ldm, max_count, T; // max_count: pairs of the filter with the most; T: tiles per dimension of the largest filter that merges
};

/// aslam_merge_landmarks up to the first round: the checks, the staging, merge_plan and its report.  No filter is written.
int merge_plan_stage(aslam_ctx *c, const int32_t *into, int ld, int is_device, double noise_var, hipStream_t st, MergePlan &p)
{
        if (const std::string e = bad_mask(c, into, ld, is_device, "into"); !e.empty())
                return fail(ASLAM_ERR_ARG, "aslam_merge_landmarks: " + e);
        if (!std::isfinite(noise_var) || noise_var < 0.0)
                return fail(ASLAM_ERR_ARG, "aslam_merge_landmarks: noise_var must be finite and not negative");
        int rc = sync_ctx(c);
        if (rc != ASLAM_OK)
                return rc;
        const size_t B = (size_t)c->cfg.batch, NP = (size_t)c->NP, ldm = ((size_t)ld + 15) & ~(size_t)15;
        // staging: the plan's report | pairs (i) | pairs (j) | removal mask | stop flags | V | a host array's copy
        Staging s{c};
        const size_t o_meta = s.take(sizeof(MergeMeta) * B), o_pi = s.take(4 * B * ldm), o_pj = s.take(4 * B * ldm);
        p.o_mask = s.take(B * ldm);
        const size_t o_stop = s.take(4 * B), o_V = s.take(8 * B * MERGE_K * NP), o_into = s.take(is_device ? 0 : 4 * B * (size_t)ld);
        p.s = s;
        // (with the remove path's front part behind it: the block does not move while the rounds are in flight)
        remove_front(s);
        if ((rc = s.reserve()) != ASLAM_OK)
                return rc;
        const int32_t *idev = into;
        if (!is_device)
        {
                HIP_TRY(hipMemcpy(s.at<int32_t>(o_into), into, sizeof(int32_t) * B * ld, hipMemcpyHostToDevice));
                idev = s.at<int32_t>(o_into);
        }
        p.st = st, p.ldm = (int)ldm, p.meta_dev = s.at<MergeMeta>(o_meta), p.mask = s.at<uint8_t>(p.o_mask);
        p.pi = s.at<int32_t>(o_pi), p.pj = s.at<int32_t>(o_pj), p.stop = s.at<int32_t>(o_stop);
        p.V = s.at<double>(o_V), p.P = c->large ? c->largeP : c->dv.P;
        c->last_stream = st;
        hipLaunchKernelGGL(merge_plan, dim3((unsigned)B), dim3(PRUNE_WAVE), 0, st, idev, ld, (const int *)c->dv.n, c->NP, p.ldm, p.pi, p.pj, p.mask, p.stop,
                           p.meta_dev);
        HIP_TRY(hipGetLastError());
        // the plan's report, checked before any filter is written: a refused call leaves the context as it was
        p.meta.resize(B);
        HIP_TRY(hipMemcpyAsync(p.meta.data(), p.meta_dev, sizeof(MergeMeta) * B, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        int max_L = p.max_count = 0;
        for (size_t b = 0; b < B; ++b)
        {
                const MergeMeta &m = p.meta[b];
                if (m.bad_j >= 0)
                        return fail(ASLAM_ERR_ARG, "aslam_merge_landmarks: filter " + std::to_string(b) + ", landmark " + std::to_string(m.bad_j) + ": into = " +
                                                       std::to_string(m.bad_i) + " (needs 0 <= into < landmark, and a root that is not merged away itself)");
                p.max_count = std::max(p.max_count, m.count);
                if (m.count > 0)
                        max_L = std::max(max_L, m.L);
        }
        p.T = (3 + 2 * max_L + MERGE_TILE - 1) / MERGE_TILE;
        return ASLAM_OK;
}

/// round r of a planned merge, in its two launches
void launch_merge_gain(aslam_ctx *c, const MergePlan &p, int r, double noise_var)
{
        hipLaunchKernelGGL(merge_gain, dim3((unsigned)c->cfg.batch), dim3(MERGE_WG), 0, p.st, c->dv.X, (const double *)p.P, (const int *)c->dv.n, c->NP, p.ldm,
                           (const int32_t *)p.pi, (const int32_t *)p.pj, (const MergeMeta *)p.meta_dev, r, noise_var, p.V, p.mask, p.stop);
}
void launch_merge_downdate(aslam_ctx *c, const MergePlan &p, int r)
{
        hipLaunchKernelGGL(merge_downdate, dim3((unsigned)(p.T * (p.T + 1) / 2), (unsigned)c->cfg.batch), dim3(MERGE_WG), 0, p.st, p.P, (const int *)c->dv.n,
                           c->NP, (const MergeMeta *)p.meta_dev, r, (const double *)p.V, (const int32_t *)p.stop);
}
} // namespace

int aslam_merge_landmarks(aslam_ctx *c, const int32_t *into, int ld, int is_device, double noise_var, int32_t *merged_out, void *stream)
{
        MergePlan p;
        int rc = merge_plan_stage(c, into, ld, is_device, noise_var, static_cast<hipStream_t>(stream), p);
        if (rc != ASLAM_OK)
                return rc;
        const int B = c->cfg.batch;
        if (merged_out)
                std::fill(merged_out, merged_out + B, 0);
        if (p.max_count == 0)
                return ASLAM_OK;
        for (int r = 0; r * MERGE_ROUND < p.max_count; ++r)
        {
                launch_merge_gain(c, p, r, noise_var);
                HIP_TRY(hipGetLastError());
                launch_merge_downdate(c, p, r);
                HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(merge_sightings, dim3((unsigned)B), dim3(PRUNE_WAVE), 0, p.st, (const uint32_t *)c->dv.clock, c->dv.lm_seen, c->dv.lm_hits, c->NP,
                           p.ldm, (const int32_t *)p.pi, (const int32_t *)p.pj, (const MergeMeta *)p.meta_dev, (const uint8_t *)p.mask);
        HIP_TRY(hipGetLastError());
        // the merged-away landmarks leave through the remove path itself, with the mask the plan wrote (less what a failed pivot took out)
        std::vector<PruneMeta> pm;
        if ((rc = remove_landmarks_at(c, p.s, DevMask{nullptr, p.o_mask}, nullptr, p.ldm, p.st, &pm)) != ASLAM_OK)
                return rc;
        if (merged_out)
                for (int b = 0; b < B; ++b)
                        merged_out[b] = (pm[b].n - pm[b].n_new) / 2;
        return ASLAM_OK;
}

/* diagnostic (tools/merge_rate.py): merge_downdate alone.  The plan and the first round's gain of aslam_merge_landmarks(into_dev), then that
   round's downdate launch `reps` times after three untimed ones, each between two device events on the default stream; ms [reps].  Every
   repetition subtracts again: the filters are left in no state to run on -- restore them. */
int aslam_debug_merge_rate(aslam_ctx *c, const int32_t *into_dev, int ld, double noise_var, int reps, float *ms)
{
        if (!ms || reps < 1)
                return fail(ASLAM_ERR_ARG, "null argument");
        MergePlan p;
        int rc = merge_plan_stage(c, into_dev, ld, 1, noise_var, nullptr, p);
        if (rc != ASLAM_OK || p.max_count == 0)
                return rc;
        launch_merge_gain(c, p, 0, noise_var);
        HIP_TRY(hipGetLastError());
        hipEvent_t e0, e1;
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        for (int k = -3; k < reps; ++k)
        {
                HIP_TRY(hipEventRecord(e0, p.st));
                launch_merge_downdate(c, p, 0);
                HIP_TRY(hipEventRecord(e1, p.st));
                HIP_TRY(hipEventSynchronize(e1));
                float t = 0.f;
                HIP_TRY(hipEventElapsedTime(&t, e0, e1));
                if (k >= 0)
                        ms[k] = t;
        }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        return ASLAM_OK;
}

int aslam_select_duplicates(aslam_ctx *c, const double *gate, const double *max_dist, int32_t *into_dev, int ld, void *stream)
{
        if (const std::string e = bad_mask(c, into_dev, ld, 1, "into"); !e.empty())
                return fail(ASLAM_ERR_ARG, "aslam_select_duplicates: " + e);
        if (!gate || !max_dist)
                return fail(ASLAM_ERR_ARG, "aslam_select_duplicates: null gate or max_dist");
        const int B = c->cfg.batch;
        std::vector<double> par(2 * (size_t)B);
        for (int b = 0; b < B; ++b)
        {
                if (!(gate[b] > 0.0))
                        return fail(ASLAM_ERR_ARG, "aslam_select_duplicates: gate[" + std::to_string(b) + "] must be positive");
                if (!std::isfinite(max_dist[b]) || max_dist[b] <= 0.0)
                        return fail(ASLAM_ERR_ARG, "aslam_select_duplicates: max_dist[" + std::to_string(b) + "] must be finite and positive");
                par[b] = max_dist[b] * max_dist[b];
                par[(size_t)B + b] = gate[b];
        }
        int rc = sync_ctx(c);
        // staging: max_dist^2, gate | every landmark's partner
        Staging s{c};
        const size_t o_par = s.take(sizeof(double) * 2 * B), o_partner = s.take(sizeof(int32_t) * B * ld);
        if (rc == ASLAM_OK)
                rc = s.reserve();
        if (rc != ASLAM_OK)
                return rc;
        hipStream_t st = static_cast<hipStream_t>(stream);
        c->last_stream = st;
        if ((rc = stage_host(c, s.at<double>(o_par), par.data(), sizeof(double) * 2 * B, st)) != ASLAM_OK)
                return rc;
        const double *pd = s.at<double>(o_par);
        int32_t *partner = s.at<int32_t>(o_partner);
        const int wpb = MERGE_WG / PRUNE_WAVE;
        hipLaunchKernelGGL(merge_select, dim3((unsigned)((ld + wpb - 1) / wpb), (unsigned)B), dim3(MERGE_WG), 0, st, (const double *)c->dv.X,
                           (const double *)(c->large ? c->largeP : c->dv.P), (const int *)c->dv.n, c->NP, pd, pd + B, partner, ld);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(merge_resolve, dim3((unsigned)B), dim3(PRUNE_WAVE), 0, st, (const int32_t *)partner, into_dev, ld);
        HIP_TRY(hipGetLastError());
        return ASLAM_OK;
}

/* ---- Mahalanobis-gated data association (assoc.h) ------------------------------------------------------------------------ */
int aslam_gate_observations(aslam_ctx *c, const float *obs, int ldo, int is_device, const int32_t *n_obs, const double *gate, int32_t *assoc_dev,
                            double *mdist_dev, void *stream)
{
        const std::string who = "aslam_gate_observations: ";
        if (!c)
                return fail(ASLAM_ERR_ARG, who + "null context");
        if (!obs)
                return fail(ASLAM_ERR_ARG, who + "null obs");
        if (!n_obs)
                return fail(ASLAM_ERR_ARG, who + "null n_obs");
        if (!gate)
                return fail(ASLAM_ERR_ARG, who + "null gate");
        if (!assoc_dev)
                return fail(ASLAM_ERR_ARG, who + "null assoc_dev");
        if (ldo < 1)
                return fail(ASLAM_ERR_ARG, who + "ldo must be at least 1");
        const int B = c->cfg.batch;
        for (int b = 0; b < B; ++b)
        {
                if (n_obs[b] < 0 || n_obs[b] > ldo)
                        return fail(ASLAM_ERR_ARG, who + "n_obs[" + std::to_string(b) + "] = " + std::to_string(n_obs[b]) + " is outside 0 .. ldo (filter " +
                                                       std::to_string(b) + ")");
                if (!(gate[b] > 0.0))
                        return fail(ASLAM_ERR_ARG, who + "gate[" + std::to_string(b) + "] must be positive (filter " + std::to_string(b) + ")");
        }
        if (is_device && ((uintptr_t)obs & 15))
                return fail(ASLAM_ERR_ARG, who + "a device obs must be 16-byte aligned");
        if ((uintptr_t)assoc_dev & 15)
                return fail(ASLAM_ERR_ARG, who + "assoc_dev must be 16-byte aligned");
        if ((uintptr_t)mdist_dev & 15)
                return fail(ASLAM_ERR_ARG, who + "mdist_dev must be 16-byte aligned");
        int rc = sync_ctx(c);
        // staging: gate | n_obs | a host array's copy
        const size_t obs_bytes = sizeof(float) * 2 * (size_t)B * ldo;
        Staging s{c};
        const size_t o_gate = s.take(sizeof(double) * B), o_n = s.take(sizeof(int32_t) * B), o_obs = s.take(is_device ? 0 : obs_bytes);
        if (rc == ASLAM_OK)
                rc = s.reserve();
        if (rc != ASLAM_OK)
                return rc;
        hipStream_t st = static_cast<hipStream_t>(stream);
        c->last_stream = st;
        if ((rc = stage_host(c, s.at<double>(o_gate), gate, sizeof(double) * B, st)) != ASLAM_OK ||
            (rc = stage_host(c, s.at<int32_t>(o_n), n_obs, sizeof(int32_t) * B, st)) != ASLAM_OK)
                return rc;
        const float *odev = obs;
        if (!is_device)
        {
                if ((rc = stage_host(c, s.at<float>(o_obs), obs, obs_bytes, st)) != ASLAM_OK)
                        return rc;
                odev = s.at<float>(o_obs);
        }
        hipLaunchKernelGGL(assoc_gate, dim3((unsigned)B), dim3(ASSOC_WG), 0, st, (const double *)c->dv.X, (const double *)(c->large ? c->largeP : c->dv.P),
                           (const int *)c->dv.n, c->NP, (const aslam_params *)c->params_dev, odev, ldo, (const int32_t *)s.at<int32_t>(o_n),
                           (const double *)s.at<double>(o_gate), assoc_dev, mdist_dev);
        HIP_TRY(hipGetLastError());
        return ASLAM_OK;
}

/* ---- joint compatibility (joint.h) ------------------------------------------------------------------------------------------ */
namespace
{
/// the regularised lower incomplete gamma function P(a, x), a > 0, x >= 0: the series below a + 1, the continued fraction (modified Lentz) above
double gamma_p(double a, double x)
{
        if (!(x > 0.0))
                return 0.0;
        const double lead = std::exp(-x + a * std::log(x) - std::lgamma(a));
        if (x < a + 1.0)
        {
                double term = 1.0 / a, sum = term;
                for (int k = 1; k < 10000; ++k)
                {
                        term *= x / (a + k);
                        sum += term;
                        if (std::fabs(term) < std::fabs(sum) * 1e-17)
                                break;
                }
                return lead * sum;
        }
        const double tiny = 1e-300;
        double bq = x + 1.0 - a, cq = 1.0 / tiny, dq = 1.0 / bq, h = dq;
        for (int k = 1; k < 10000; ++k)
        {
                const double an = -(double)k * ((double)k - a);
                bq += 2.0;
                dq = an * dq + bq;
                dq = std::fabs(dq) < tiny ? tiny : dq;
                cq = bq + an / cq;
                cq = std::fabs(cq) < tiny ? tiny : cq;
                dq = 1.0 / dq;
                const double del = dq * cq;
                h *= del;
                if (std::fabs(del - 1.0) < 1e-16)
                        break;
        }
        return 1.0 - lead * h;
}

/// whether the byte ranges [p, p + np) and [q, q + nq) share a byte (a null pointer shares none)
bool ranges_overlap(const void *p, size_t np, const void *q, size_t nq)
{
        const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
        return p && q && a < b + nq && b < a + np;
}
} // namespace

int aslam_chi2_point(double prob, int dof, double *out)
{
        const std::string who = "aslam_chi2_point: ";
        if (!out)
                return fail(ASLAM_ERR_ARG, who + "null out");
        if (!(prob > 0.0 && prob < 1.0))
                return fail(ASLAM_ERR_ARG, who + "prob must lie inside (0, 1)");
        if (dof < 1)
                return fail(ASLAM_ERR_ARG, who + "dof must be at least 1");
        const double a = 0.5 * dof;
        double lo = 0.0, hi = 2.0 * a + 10.0; // (x = 2 * the gamma variable)
        for (int k = 0; k < 64 && gamma_p(a, 0.5 * hi) < prob; ++k)
                lo = hi, hi *= 2.0;
        for (int k = 0; k < 200; ++k)
        {
                const double mid = 0.5 * (lo + hi);
                if (!(lo < mid && mid < hi))
                        break;
                (gamma_p(a, 0.5 * mid) < prob ? lo : hi) = mid;
        }
        *out = 0.5 * (lo + hi);
        return ASLAM_OK;
}

int aslam_joint_compat(aslam_ctx *c, const float *obs, int ldo, int is_device, const int32_t *n_obs, const int32_t *cand_dev, const double *gate_tab,
                       int32_t *assoc_dev, double *incr_dev, double *joint_dev, int32_t *count_dev, void *stream)
{
        static_assert(JOINT_MAX_OBS == ASLAM_JC_MAX_OBS, "joint.h and aslam_core.h name one cap");
        const std::string who = "aslam_joint_compat: ";
        if (!c)
                return fail(ASLAM_ERR_ARG, who + "null context");
        const struct
        {
                const char *name;
                const void *p;
                size_t per_filter; // bytes, in units of ldo where `per_obs`
                bool per_obs, device, required;
        } arg[] = {{"obs", obs, sizeof(float) * 2, true, is_device != 0, true},
                   {"n_obs", n_obs, 0, false, false, true},
                   {"cand_dev", cand_dev, sizeof(int32_t), true, true, true},
                   {"assoc_dev", assoc_dev, sizeof(int32_t), true, true, true},
                   {"incr_dev", incr_dev, sizeof(double), true, true, false},
                   {"joint_dev", joint_dev, sizeof(double) * 2, false, true, true},
                   {"count_dev", count_dev, sizeof(int32_t) * 2, false, true, true}};
        for (const auto &a : arg)
                if (a.required && !a.p)
                        return fail(ASLAM_ERR_ARG, who + "null " + a.name);
        if (ldo < 1)
                return fail(ASLAM_ERR_ARG, who + "ldo must be at least 1");
        if (ldo > ASLAM_JC_MAX_OBS)
                return fail(ASLAM_ERR_UNSUPPORTED, who + "ldo = " + std::to_string(ldo) + " is beyond ASLAM_JC_MAX_OBS = " + std::to_string(ASLAM_JC_MAX_OBS));
        const int B = c->cfg.batch;
        for (int b = 0; b < B; ++b)
                if (n_obs[b] < 0 || n_obs[b] > ldo)
                        return fail(ASLAM_ERR_ARG, who + "n_obs[" + std::to_string(b) + "] = " + std::to_string(n_obs[b]) + " is outside 0 .. ldo (filter " +
                                                       std::to_string(b) + ")");
        for (int m = 1; gate_tab && m <= ldo; ++m)
                if (!(gate_tab[m] > 0.0))
                        return fail(ASLAM_ERR_ARG, who + "gate_tab[" + std::to_string(m) + "] must be positive");
        for (const auto &a : arg)
                if (a.device && ((uintptr_t)a.p & 15))
                        return fail(ASLAM_ERR_ARG, who + (&a == &arg[0] ? "a device obs" : a.name) + " must be 16-byte aligned");
        // two device arrays may not share a byte, but for assoc_dev == cand_dev exactly (the chain gate -> joint runs in place)
        auto bytes = [&](const auto &a) { return a.per_filter * (size_t)B * (a.per_obs ? (size_t)ldo : 1); };
        for (const auto &a : arg)
                for (const auto &o : arg)
                        if (&a < &o && a.device && o.device && ranges_overlap(a.p, bytes(a), o.p, bytes(o)) &&
                            !(&a == &arg[2] && &o == &arg[3] && a.p == o.p))
                                return fail(ASLAM_ERR_ARG, who + a.name + " and " + o.name + " overlap");
        int rc = sync_ctx(c);
        // staging: the gate table | n_obs | a host array's copy
        const size_t obs_bytes = sizeof(float) * 2 * (size_t)B * ldo;
        Staging s{c};
        const size_t o_tab = s.take(gate_tab ? sizeof(double) * (ldo + 1) : 0), o_n = s.take(sizeof(int32_t) * B), o_obs = s.take(is_device ? 0 : obs_bytes);
        if (rc == ASLAM_OK)
                rc = s.reserve();
        if (rc != ASLAM_OK)
                return rc;
        hipStream_t st = static_cast<hipStream_t>(stream);
        c->last_stream = st;
        if (gate_tab && (rc = stage_host(c, s.at<double>(o_tab), gate_tab, sizeof(double) * (ldo + 1), st)) != ASLAM_OK)
                return rc;
        if ((rc = stage_host(c, s.at<int32_t>(o_n), n_obs, sizeof(int32_t) * B, st)) != ASLAM_OK)
                return rc;
        const float *odev = obs;
        if (!is_device)
        {
                if ((rc = stage_host(c, s.at<float>(o_obs), obs, obs_bytes, st)) != ASLAM_OK)
                        return rc;
                odev = s.at<float>(o_obs);
        }
        const size_t lds = JointLds{ldo}.bytes();
        HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(joint_compat), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(joint_compat, dim3((unsigned)B), dim3(JOINT_WG), lds, st, (const double *)c->dv.X, (const double *)(c->large ? c->largeP : c->dv.P),
                           (const int *)c->dv.n, c->NP, (const aslam_params *)c->params_dev, odev, ldo, (const int32_t *)s.at<int32_t>(o_n), cand_dev,
                           gate_tab ? (const double *)s.at<double>(o_tab) : nullptr, assoc_dev, incr_dev, joint_dev, count_dev);
        HIP_TRY(hipGetLastError());
        return ASLAM_OK;
}

/* diagnostic (tools/snapshot_rate.py): the pack and the unpack launch of the whole batch and a device-to-device copy of the blob's bytes, each
   between two device events, alternating `reps` times after three untimed rounds.  dev_buf: device memory of at least twice the snapshot's
   size.  ms [3][reps]: pack, unpack, copy.  info[3]: bytes of the blob, of the padded layout unpack writes, of the scratch it clears. */
int aslam_debug_snapshot_rate(aslam_ctx *c, void *dev_buf, int64_t cap_bytes, int reps, float *ms, int64_t *info)
{
        if (!c || !dev_buf || !ms || !info || reps < 1)
                return fail(ASLAM_ERR_ARG, "null argument");
        // the whole batch, described and placed as aslam_snapshot does it (the first pack of the loop below fills the blob the unpacks read)
        const int count = c->cfg.batch;
        std::vector<SnapDesc> hdesc;
        Placed placed = {};
        Staging s{c};
        const size_t o_desc = s.take(sizeof(SnapDesc) * count);
        int rc = sync_ctx(c);
        if (rc == ASLAM_OK)
                rc = snap_describe(c, nullptr, count, nullptr, hdesc, placed);
        const int64_t total = placed.total;
        if (rc == ASLAM_OK && cap_bytes < 2 * total)
                rc = fail(ASLAM_ERR_ARG, "aslam_debug_snapshot_rate needs twice the snapshot's size");
        if (rc == ASLAM_OK)
                rc = s.reserve();
        if (rc != ASLAM_OK)
                return rc;
        const SnapDesc *desc = s.at<SnapDesc>(o_desc);
        HIP_TRY(hipMemcpy(s.at<SnapDesc>(o_desc), hdesc.data(), sizeof(SnapDesc) * count, hipMemcpyHostToDevice));
        const SnapCtx sc = snap_ctx(c);
        char *blob = static_cast<char *>(dev_buf);
        c->last_stream = nullptr;
        auto bytes = [&](auto m) { return per_filter(c->dv, m) * sizeof(*(c->dv.*m)); }; // (P: the large path's has the same shape)
        info[0] = total;
        info[1] = (int64_t)count * (int64_t)(bytes(&DevView::X) + bytes(&DevView::Z) + bytes(&DevView::P) + bytes(&DevView::sens) +
                                             bytes(&DevView::wait_rb) + bytes(&DevView::wait_cnt));
        info[2] = 0;
        for (int k = 0; k < SNAP_CLEAR_MAX; ++k)
                info[2] += sc.clear[k] ? (int64_t)count * (int64_t)sc.clear_bytes[k] : 0;
        hipEvent_t e0, e1;
        HIP_TRY(hipEventCreate(&e0));
        HIP_TRY(hipEventCreate(&e1));
        for (int r = -3; r < reps; ++r)
                for (int what = 0; what < 3; ++what)
                {
                        HIP_TRY(hipEventRecord(e0, nullptr));
                        if (what == 0)
                                launch_snapshot_pack(c, desc, count, placed, blob, nullptr);
                        else if (what == 1)
                                hipLaunchKernelGGL(snapshot_unpack, snap_grid((int64_t)c->NP * c->NP / 2, count), dim3(SNAP_WG), 0, nullptr, sc, desc, count,
                                                   (const char *)blob);
                        else
                                HIP_TRY(hipMemcpyAsync(blob + total, blob, (size_t)total, hipMemcpyDeviceToDevice, nullptr));
                        HIP_TRY(hipEventRecord(e1, nullptr));
                        HIP_TRY(hipEventSynchronize(e1));
                        float t = 0.f;
                        HIP_TRY(hipEventElapsedTime(&t, e0, e1));
                        if (r >= 0)
                                ms[what * reps + r] = t;
                }
        (void)hipEventDestroy(e0);
        (void)hipEventDestroy(e1);
        return ASLAM_OK;
}

/* diagnostic (tests/manual/large_residuals.py): the work matrices of the large path after the last callback, widened to double.
   which: 0 = G (-> V in place) [NP][NP], 1 = S (-> L, lower block triangle) [NP][NP], 2 = Linv [17][64][64], 3 = Y [NP] */
int aslam_debug_large(aslam_ctx *c, int traj, int which, double *out, int64_t cap)
{
        if (check_traj(c, traj) != ASLAM_OK)
                return ASLAM_ERR_ARG;
        if (!c->large || which < 0 || which > 3)
                return fail(ASLAM_ERR_UNSUPPORTED, "aslam_debug_large: large-state contexts only");
        if (sync_ctx(c) != ASLAM_OK)
                return ASLAM_ERR_HIP;
        return with_large_view(c, [&](auto &lv) -> int {
                using V = std::remove_reference_t<decltype(lv)>;
                using T = std::remove_reference_t<decltype(*lv.G)>;
                T *V::*const m = which == 0 ? &V::G : which == 1 ? &V::S : &V::Linv;
                const size_t cnt = which == 3 ? per_filter(lv, &V::Y) : per_filter(lv, m);
                if ((int64_t)cnt > cap)
                        return fail(ASLAM_ERR_ARG, "aslam_debug_large: buffer too small");
                if (which == 3)
                {
                        HIP_TRY(hipMemcpy(out, lv.Y + traj * cnt, cnt * sizeof(double), hipMemcpyDeviceToHost));
                        return ASLAM_OK;
                }
                std::vector<T> tmp(cnt);
                HIP_TRY(hipMemcpy(tmp.data(), lv.*m + traj * cnt, cnt * sizeof(T), hipMemcpyDeviceToHost));
                std::copy(tmp.begin(), tmp.end(), out);
                return ASLAM_OK;
        });
}

#if defined(ASLAM_STAMPS) && ASLAM_HAVE_UKF
/* diagnostic builds only: copy a UKF scratch matrix of filter `traj` to the host. which: 0 D, 1 DZ ([NP][MP]), 2 Tc, 3 K ([NP][NP]) */
int aslam_debug_ukf(aslam_ctx *c, int traj, int which, double *out, int *rows, int *cols)
{
        if (sync_ctx(c) != ASLAM_OK)
                return ASLAM_ERR_HIP;
        double *UkfView::*const m = which == 0 ? &UkfView::D : which == 1 ? &UkfView::DZ : which == 2 ? &UkfView::Tc : &UkfView::K;
        const size_t cnt = per_filter(c->ukf, m, c->NP);
        *rows = c->NP;
        *cols = (int)(cnt / (size_t)c->NP);
        HIP_TRY(hipMemcpy(out, c->ukf.*m + traj * cnt, cnt * sizeof(double), hipMemcpyDeviceToHost));
        return ASLAM_OK;
}
#endif

#ifdef ASLAM_STAMPS
/* diagnostic builds only: per-phase shader-cycle sums of workgroup 0 since the context was created */
int aslam_debug_stamps(aslam_ctx *c, unsigned long long *out12)
{
        if (sync_ctx(c) != ASLAM_OK)
                return ASLAM_ERR_HIP;
        HIP_TRY(hipMemcpy(out12, c->dv.dbg, 12 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        return ASLAM_OK;
}

/* diagnostic builds only: 100 MHz ticks spent inside large_frontend_kernel (workgroup 0) and the number of launches */
int aslam_debug_fe_realtime(aslam_ctx *c, unsigned long long *out2)
{
        if (sync_ctx(c) != ASLAM_OK)
                return ASLAM_ERR_HIP;
        HIP_TRY(hipMemcpy(out2, c->dv.dbg + 56, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        return ASLAM_OK;
}

/* diagnostic builds only: 100 MHz ticks every workgroup (filter) spent inside the last large_frontend_kernel launch */
int aslam_debug_fe_per_filter(aslam_ctx *c, unsigned long long *out, int count)
{
        if (sync_ctx(c) != ASLAM_OK)
                return ASLAM_ERR_HIP;
        HIP_TRY(hipMemcpy(out, c->dv.dbg + 64, (size_t)std::min(count, 1024) * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        return ASLAM_OK;
}

/* diagnostic builds only (-DASLAM_FE_STAMPS): front-end phase cycles, 6 values */
int aslam_debug_fe_stamps(aslam_ctx *c, unsigned long long *out6)
{
        if (sync_ctx(c) != ASLAM_OK)
                return ASLAM_ERR_HIP;
        HIP_TRY(hipMemcpy(out6, c->dv.dbg + 45, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        return ASLAM_OK;
}

/* diagnostic builds only: per-wave busy cycles inside cholesky_forward: [wave][panel, trailing/forward/factor] */
int aslam_debug_wave_busy(aslam_ctx *c, unsigned long long *out24)
{
        if (sync_ctx(c) != ASLAM_OK)
                return ASLAM_ERR_HIP;
        HIP_TRY(hipMemcpy(out24, c->dv.dbg + 16, 24 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        return ASLAM_OK;
}
#endif

/* ---- include/aslam_scan.h ------------------------------------------------------------------------------------------ */
namespace
{
constexpr int MAX_SCAN_DEVICES = 16;
static float *g_scan_tables[MAX_SCAN_DEVICES] = {}; // [2][360]: cos_map, sin_map of LandMarks::initialize (sensor_landmark.cpp:49-56)

static int scan_tables(int device, float **out)
{
        if (device < 0 || device >= MAX_SCAN_DEVICES)
                return fail(ASLAM_ERR_ARG, "device index out of range");
        static std::mutex mu;
        std::lock_guard<std::mutex> lock(mu);
        if (!g_scan_tables[device])
        {
                // the reference fills them with the host libm's binary32 sin / cos of DEG2RAD * float(theta): so does this
                const float DEG2RAD = 0.01745329251f; // config.h:41
                float tab[2 * SCAN_BEAMS];
                for (int t = 0; t < SCAN_BEAMS; ++t)
                {
                        tab[t] = std::cos(DEG2RAD * static_cast<float>(t));
                        tab[SCAN_BEAMS + t] = std::sin(DEG2RAD * static_cast<float>(t));
                }
                float *p = nullptr;
                HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p), sizeof(tab)));
                HIP_TRY(hipMemcpy(p, tab, sizeof(tab), hipMemcpyHostToDevice));
                g_scan_tables[device] = p;
        }
        *out = g_scan_tables[device];
        return ASLAM_OK;
}
} // namespace

int aslam_scan_landmarks(const float *ranges, int64_t count, int is_device, int max_out, float *range_out, float *bearing_out,
                         int32_t *n_out, uint32_t *status_out, int device, void *stream)
{
        if (!ranges || !range_out || !bearing_out || !n_out || !status_out || count < 0 || max_out <= 0)
                return fail(ASLAM_ERR_ARG, "aslam_scan_landmarks: bad argument");
        if (count == 0)
                return ASLAM_OK;
        HIP_TRY(hipSetDevice(device));
        float *tab = nullptr;
        int rc = scan_tables(device, &tab);
        if (rc != ASLAM_OK)
                return rc;
        hipStream_t st = static_cast<hipStream_t>(stream);
        const size_t n = (size_t)count;
        if (is_device)
        {
                hipLaunchKernelGGL(scan_landmarks_kernel, dim3((unsigned)count), dim3(64), 0, st, ranges, tab, tab + SCAN_BEAMS, count, max_out,
                                   range_out, bearing_out, n_out, status_out);
                HIP_TRY(hipGetLastError());
                return ASLAM_OK;
        }
        float *d_in = nullptr, *d_r = nullptr, *d_b = nullptr;
        int32_t *d_n = nullptr;
        uint32_t *d_s = nullptr;
        auto cleanup = [&]() {
                (void)hipFree(d_in), (void)hipFree(d_r), (void)hipFree(d_b), (void)hipFree(d_n), (void)hipFree(d_s);
        };
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&d_in), n * SCAN_BEAMS * sizeof(float));
        if (e == hipSuccess)
                e = hipMalloc(reinterpret_cast<void **>(&d_r), n * max_out * sizeof(float));
        if (e == hipSuccess)
                e = hipMalloc(reinterpret_cast<void **>(&d_b), n * max_out * sizeof(float));
        if (e == hipSuccess)
                e = hipMalloc(reinterpret_cast<void **>(&d_n), n * sizeof(int32_t));
        if (e == hipSuccess)
                e = hipMalloc(reinterpret_cast<void **>(&d_s), n * sizeof(uint32_t));
        if (e == hipSuccess)
                e = hipMemcpyAsync(d_in, ranges, n * SCAN_BEAMS * sizeof(float), hipMemcpyHostToDevice, st);
        if (e == hipSuccess)
                e = hipMemsetAsync(d_r, 0, n * max_out * sizeof(float), st);
        if (e == hipSuccess)
                e = hipMemsetAsync(d_b, 0, n * max_out * sizeof(float), st);
        if (e == hipSuccess)
        {
                hipLaunchKernelGGL(scan_landmarks_kernel, dim3((unsigned)count), dim3(64), 0, st, d_in, tab, tab + SCAN_BEAMS, count, max_out, d_r,
                                   d_b, d_n, d_s);
                e = hipGetLastError();
        }
        if (e == hipSuccess)
                e = hipMemcpyAsync(range_out, d_r, n * max_out * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
                e = hipMemcpyAsync(bearing_out, d_b, n * max_out * sizeof(float), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
                e = hipMemcpyAsync(n_out, d_n, n * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
                e = hipMemcpyAsync(status_out, d_s, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess)
                e = hipStreamSynchronize(st);
        cleanup();
        if (e != hipSuccess)
                return fail(ASLAM_ERR_HIP, std::string("aslam_scan_landmarks: ") + hipGetErrorString(e));
        return ASLAM_OK;
}

int aslam_get_launch_info(aslam_ctx *c, int *stream_groups, int *chol_resident, int *launches_per_callback)
{
        if (!c)
                return fail(ASLAM_ERR_ARG, "null context");
        if (stream_groups)
                *stream_groups = c->large ? c->lh.last_groups : 0;
        if (chol_resident)
                *chol_resident = c->large && c->lh.last_resident;
        if (launches_per_callback)
                *launches_per_callback = c->large ? c->lh.last_launches : 1;
        return ASLAM_OK;
}

int aslam_get_syrk_tail(aslam_ctx *c, int *on)
{
        if (!c || !on)
                return fail(ASLAM_ERR_ARG, "null argument");
        *on = c->large && c->lh.last_syrk_tail;
        return ASLAM_OK;
}

int aslam_kernel_info(aslam_ctx *c, char *name, int name_cap, int *grid, int *block, int *lds_bytes)
{
        if (!c)
                return fail(ASLAM_ERR_ARG, "null context");
        char buf[320];
        std::string nm;
        size_t lds = 0;
        const FrontendVariant fv = frontend_variant<MODE_REPLAY>(c, StatsView{}); // what aslam_replay launches
        if (c->large)
        {
                // the plan of a launch over the whole batch.  The names say which pipe each kernel's products run on (bench.py prices them from
                // this string and looks the chain up in profiles/pmc_traffic.json by it)
                const LargePlan plan = large_plan(c->cfg.dtype == ASLAM_F32, c->NP, c->cfg.batch, c->cfg.batch, c->lh.knobs);
#if ASLAM_HAVE_UKF
                if (c->cfg.filter == ASLAM_UKF)
                        std::snprintf(buf, sizeof(buf), "ukf_large_wabt + large_update_panel<double> + large_syrk<double> (%d-launch chain per callback, 1 stream)",
                                      ukf_large_plan(c->NP).launches);
                else
#endif
                if (plan.chain == LargeChain::F32_RESIDENT) // (the Cholesky, the TRSM and the syrk are named; the X update is launch 5, in front of the syrk, with the border, else launch 6)
                        std::snprintf(buf, sizeof(buf), "%s + %s + large_syrk_bf16x3%s (%d-launch chain per callback, %d stream groups)",
                                      plan.chol16 ? "large_chol_bf16" : "large_chol_resident", plan.trsm16 ? "large_trsm_bf16" : "large_trsm_pipe<17>",
                                      plan.border ? " + border" : "", plan.launches, c->lh.knobs.groups);
                else if (plan.chain == LargeChain::F32_RIGHT)
                        std::snprintf(buf, sizeof(buf), "large_right_step + large_syrk_bf16x3 (%d-launch chain per callback: one right-looking launch per block column)", plan.launches);
                else if (plan.chain == LargeChain::F32_LEFT)
                        std::snprintf(buf, sizeof(buf), "large_trsm_pipe<17> + large_syrk_bf16x3 (%d-launch chain per callback: multi-workgroup Cholesky)", plan.launches);
                else
                        std::snprintf(buf, sizeof(buf), "large_update_panel<double> (%d-launch chain per callback, %d stream groups)", plan.launches, c->lh.knobs.groups);
                // the front end's variant shows as a prefix: the sighted-only update by the G, S kernel it switches, the gate by the front end itself
                nm = std::string(!fv.gated ? "" : c->cfg.filter == ASLAM_EKF ? "large_frontend_kernel<T,gated> + " : "ukf_large_frontend_kernel<gated> + ") +
                     (fv.sighted ? "large_build_GS<T,sighted> + " : "") + buf;
                lds = LargeLds::launch_bytes(c->NP, fv.gated);
        }
        else if (c->cfg.filter == ASLAM_EKF)
        {
                nm = "ekf_small_kernel<" + std::to_string(c->NT) + ",0" + variant_args({fv.stats, fv.sighted, fv.gated}) + ">";
                lds = with_NT(c->NT, [](auto nt) -> size_t { return SmallLayout<decltype(nt)::value>::total; });
        }
#if ASLAM_HAVE_UKF
        else
        {
                nm = "ukf_small_kernel<" + std::to_string(c->NT) + ",0" + variant_args({fv.stats, fv.gated}) + ">";
                lds = with_NT(c->NT, [](auto nt) -> size_t { return UkfLayout<decltype(nt)::value>::total; });
        }
#endif
        if (name && name_cap > 0)
        {
                std::strncpy(name, nm.c_str(), name_cap - 1);
                name[name_cap - 1] = 0;
        }
        if (grid)
                *grid = c->cfg.batch;
        if (block)
                *block = SMALL_WG;
        if (lds_bytes)
                *lds_bytes = (int)lds;
        return ASLAM_OK;
}

} // extern "C"
