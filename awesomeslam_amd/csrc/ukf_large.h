// ukf_large.h -- UKF-SLAM for state dimensions beyond one CU (144 <= n <= 1085), fp64, opt-in (ASLAM_CFG_UKF_LARGE).  One callback
// (UKFSlam::slam, ukf.cpp:260-392) = a chain of launches that use the whole GPU for one filter, `batch` filters side by side through the
// grid as on the large-state EKF path (ekf_large.h), whose buffers (LargeView<double>: P, S, G, Linv, Y) and kernels it shares:
//
//   ukf_large_frontend    cbSensorLandmark + updateZ (+ wait-list, growth: the shared small_frontend code, UKF flavour); the lower block
//                         triangle of P -> S, identity on the padding                                          1 workgroup / filter
//   NB x { large_potrf_inv_tiles, large_update_panel(s_only) }   L = chol(P) in S (ukf.cpp:280; the two augmentation dimensions of Paug are
//                         diagonal, ukf.cpp:274-277: their factor is two scalars, not part of the matrix)
//   ukf_large_sigma_pose  the 2 N + 5 sigma points' poses through f (ukf.cpp:283-297), the predicted mean (ukf.cpp:300-304), the pose
//                         rows of D = XsigPred - Xbar (ukf.cpp:311-313) and of DZ = Zsig - Zpred (ukf.cpp:322-351)      1 workgroup / filter
//   ukf_large_points      the landmark rows of D and DZ: a workgroup per landmark forms its two entries of every sigma point, their
//                         readings h(.), Zpred, and the two vectors that ride through the solve: z = sqrt(-w0) dz_0 and Z - Zpred
//   3 x ukf_large_wabt    A diag(w) B^T over the K = 2 N + 5 sigma points on the f64 MFMA:  P <- D W D^T + Q (ukf.cpp:307-319),
//                         S+ <- DZ W DZ^T + R WITHOUT the i = 0 term (ukf.cpp:342-357), G <- D W DZ^T = Tc (ukf.cpp:360-375)
//   NB x { large_potrf_inv_tiles, large_update_panel }   the EKF's blocked factorisation of the stacked [S+; Tc; z^T; (Z - Zpred)^T]: leaves
//                         W = Tc L^-T in G, q = L^-1 z in row n and t = L^-1 (Z - Zpred) in row n + 1 of G
//   ukf_large_gain        g = W q, X <- Xbar + W t + g (q.t) / (1 - q.q)   (ukf.cpp:378-389 by Sherman-Morrison: DESIGN.md section 4)
//   large_syrk            P <- P - W W^T
//   ukf_large_rank1       P <- P - g g^T / (1 - q.q)      (the rest of K S K^T, ukf.cpp:391: the central weight (1 - N) / 3 is negative)
//
// D and DZ are materialised ([NP][MP] per filter, MP >= 2 N + 5) and the three products are one generic kernel: the simple formulation.
// Every binary32 rounding point of the reference listed in ukf_small.h is kept (weights, sqrt(lambda + N + 2), normalizeAngle on the
// sigma-point headings, on the heading row of D and on the bearing rows of Zpred, DZ and the innovation).
#pragma once

#include "ekf_large.h"

namespace aslam
{
constexpr int UKF_LARGE_XROWS = 2; // z^T and (Z - Zpred)^T ride in rows n, n + 1 of G (LargeView::xrows)

/// HBM scratch of the large-state UKF chain (per context)
struct UkfLargeView
{
        int MP;       // row stride of D / DZ: >= 2 n + 5 rounded up to 16 for every n the context takes
        double *D;    // [B][NP][MP]  XsigPred - Xbar
        double *DZ;   // [B][NP][MP]  Zsig - Zpred
        double *XP;   // [B][3][MP]   propagated sigma-point poses
        double *Xbar; // [B][NP]      predicted mean
        double *sc;   // [B][8]       vx, az, dt of the callback (front end), 1 / (1 - q.q) (ukf_large_gain)
};

/// the per-filter arrays of a UkfLargeView, in allocation order (NP: the context's; see for_each_array(DevView &) in small_common.h).  D and DZ
/// must be zero when a filter starts: the weighted products read their padding columns (ukf_large_wabt)
template <typename F> void for_each_array(UkfLargeView &u, int NP, F &&f)
{
        const size_t np = (size_t)NP, mp = (size_t)u.MP;
        f(u.D, np * mp, true);
        f(u.DZ, np * mp, true);
        f(u.XP, 3 * mp, false);
        f(u.Xbar, np, false);
        f(u.sc, 8, false);
}

/// updateWeights (ukf.h:73-81: binary32 lambda and weight) and w = sqrt(lambda + N + 2) (ukf.cpp:284), as ukf_small.h forms them
struct UkfWeights
{
        int m;                     // 2 N + 5 sigma points
        double w_i, w_0, wsp, wsum; // weights(i >= 1), weights(0), sqrt(lambda + N + 2), sum of the weights
};
__device__ __forceinline__ UkfWeights ukf_weights(int n)
{
        UkfWeights w;
        w.m = 2 * n + 5;
        const float lambda_f = (float)(3.0 - (double)(n + 2));
        const float den_f = (lambda_f + (float)n) + 2.0f;
        w.w_i = (double)(float)(0.5 / (double)den_f);
        w.w_0 = (double)(lambda_f / den_f);
        w.wsp = (double)sqrtf(den_f);
        w.wsum = fma((double)(w.m - 1), w.w_i, w.w_0);
        return w;
}

/// sigma point i -> (column c of Laug, sign); i = 0 is the mean itself (c = -1)
__device__ __forceinline__ void ukf_col_of(int i, int n, int &c, double &sg)
{
        if (i == 0)
                c = -1, sg = 0.0;
        else if (i <= n + 2)
                c = i - 1, sg = 1.0;
        else
                c = i - n - 3, sg = -1.0;
}

/// entry of an augmented sigma point: x +- w l (ukf.cpp:287-288); the centre point is x itself
__device__ __forceinline__ double ukf_xsig(double x, double l, int c, double sg, double wsp)
{
        if (c < 0)
                return x;
        return sg > 0.0 ? x + wsp * l : x - wsp * l;
}

// ------------------------------------------------------------------------------------------------------------------
/// Per-filter front end (one workgroup of SMALL_WG threads per filter, LargeLds::bytes(NP) of dynamic LDS).  `skipped` [B] is set to 1
/// when the callback returned early (no sensor message yet): the rest of the chain then leaves the filter alone.
/// GATED (aslam_set_replay_gate, MODE_REPLAY only; LargeLds::launch_bytes(NP, true) of dynamic LDS): the front end associates by the Mahalanobis gate in the
/// filters whose gate is > 0 (small_frontend); P is read through L2.
template <int MODE, bool GATED = false>
__global__ __launch_bounds__(SMALL_WG) void ukf_large_frontend_kernel(DevView d, LargeView<double> lv, UkfLargeView uv, int64_t t, int s, int nsteps,
                                                                       double *poses_out, int32_t *dims_out, StepArgs sa, int *skipped)
{
        extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
        const int NP = lv.NP;
        const SmallLds L = LargeLds::carve(smem, NP);
        SmallShared &sm = *L.sm;
        const int tid = threadIdx.x;
        const int b = (MODE == MODE_STEP && sa.traj >= 0) ? sa.traj : (int)blockIdx.x; // sa.traj < 0: the batched step, one workgroup per filter
        double *Pg = lv.P + (size_t)b * NP * NP;
        small_enter<MODE, false, GATED>(d, L, b, tid, NP);
        if (MODE == MODE_REPLAY)
        {
                if (small_frontend<false, LARGE_OBS_CAP, LARGE_WAIT_CAP, LARGE_NP_MAX / 2, double, GATED>(d, L, Pg, NP, b, t, s, nsteps, poses_out, dims_out, tid, nullptr,
                                                                                                          GATED ? reinterpret_cast<double *>(smem + LargeLds::gate_table_at(NP)) : nullptr))
                {
                        large_frontend_skip<MODE>(d, L, skipped, b, tid, NP);
                        return;
                }
        }
        else
                small_step_intake(d, sm, sa, b, tid);
        if (tid == 0)
        {
                skipped[b] = 0;
                double *sc = uv.sc + (size_t)b * 8;
                sc[0] = (double)sm.vx, sc[1] = (double)sm.az, sc[2] = (double)sm.dt; // slam()'s binary32 arguments, for ukf_large_sigma_pose
        }
        const int n = sm.n;
        small_store<MODE>(d, L, b, tid, NP); // (starts with a barrier: the rows of P a growth has written are visible below)
        // S <- P on the lower block triangle (full diagonal blocks), identity on rows / columns n .. na - 1: what large_potrf_inv_tiles factors
        const int na = large_blocks(n, lv.xrows) * LB;
        double *Sg = lv.S + (size_t)b * NP * NP;
        typedef double d2 __attribute__((ext_vector_type(2)));
        const int lane = tid & 63, wave = tid >> 6;
        for (int r = wave; r < na; r += SMALL_WG / 64)
        {
                const int cend = LB * (r / LB + 1);
                for (int c = 2 * lane; c < cend; c += 128)
                {
                        d2 v = {0.0, 0.0};
                        if (r < n && c < n)
                                v = *reinterpret_cast<const d2 *>(Pg + (size_t)r * NP + c);
                        if (r >= n || c >= n)
                                v[0] = (r == c) ? 1.0 : 0.0;
                        if (r >= n || c + 1 >= n)
                                v[1] = (r == c + 1) ? 1.0 : 0.0;
                        *reinterpret_cast<d2 *>(Sg + (size_t)r * NP + c) = v;
                }
        }
}

// ------------------------------------------------------------------------------------------------------------------
/// The poses of the 2 N + 5 sigma points through f (only the pose entries go through f: the landmark entries pass unchanged, common.h:49-50),
/// the predicted mean, and the three pose rows of D and DZ with their entries of z and of the innovation.  grid (B), 256 threads.
__global__ __launch_bounds__(256) void ukf_large_sigma_pose(DevView d, LargeView<double> lv, UkfLargeView uv, const int *skipped)
{
        __shared__ double red[3][256];
        const int b = blockIdx.x;
        if (skipped[b])
                return;
        const int n = d.n[b], NP = lv.NP, MP = uv.MP, tid = threadIdx.x;
        const UkfWeights W = ukf_weights(n);
        const int m = W.m, mk = (m + 15) & ~15;
        const double *X = d.X + (size_t)b * NP, *Z = d.Z + (size_t)b * NP;
        const double *Lg = lv.S + (size_t)b * NP * NP; // L = chol(P), lower
        double *G = lv.G + (size_t)b * NP * NP;
        double *XP = uv.XP + (size_t)b * 3 * MP, *Xbar = uv.Xbar + (size_t)b * NP;
        double *Dg = uv.D + (size_t)b * NP * MP, *DZg = uv.DZ + (size_t)b * NP * MP;
        const double *sc = uv.sc + (size_t)b * 8;
        const float vx = (float)sc[0], az = (float)sc[1], dtf = (float)sc[2];
        const double std_a = sqrt(d.prm[b].var_a); // llt of the augmented diagonal, ukf.cpp:276,280
        const double x0 = X[0], x1 = X[1], x2 = X[2];
        double part[3] = {0.0, 0.0, 0.0};
        for (int i = tid; i < mk; i += 256)
        {
                double p0 = 0.0, p1 = 0.0, p2 = 0.0;
                if (i < m)
                {
                        int c;
                        double sg;
                        ukf_col_of(i, n, c, sg);
                        // L is lower triangular: only its columns c < 3 move the pose
                        const double l0 = (c == 0) ? Lg[0] : 0.0;
                        const double l1 = (c >= 0 && c <= 1) ? Lg[(size_t)NP + c] : 0.0;
                        const double l2 = (c >= 0 && c <= 2) ? Lg[2 * (size_t)NP + c] : 0.0;
                        p0 = ukf_xsig(x0, l0, c, sg, W.wsp);
                        p1 = ukf_xsig(x1, l1, c, sg, W.wsp);
                        p2 = ukf_xsig(x2, l2, c, sg, W.wsp);
                        // XsigAug(N, i): 0 +- w * Laug(N, N) on the acceleration-noise column, 0 elsewhere
                        double na = 0.0;
                        if (c == n)
                                na = sg > 0.0 ? 0.0 + W.wsp * std_a : 0.0 - W.wsp * std_a;
                        stateTransition(p0, p1, p2, vx, az, dtf, true, na);
                        p2 = (double)normalizeAngle((float)p2);
                        const double w = (i == 0) ? W.w_0 : W.w_i;
                        part[0] = fma(w, p0, part[0]);
                        part[1] = fma(w, p1, part[1]);
                        part[2] = fma(w, p2, part[2]);
                }
                XP[i] = p0;
                XP[MP + i] = p1;
                XP[2 * MP + i] = p2;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k)
                red[k][tid] = part[k];
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1)
        {
                if (tid < o)
                {
#pragma unroll
                        for (int k = 0; k < 3; ++k)
                                red[k][tid] += red[k][tid + o];
                }
                __syncthreads();
        }
        const double xb[3] = {red[0][0], red[1][0], red[2][0]};
        // predicted mean (ukf.cpp:300-304): the landmark entries are affine in the sigma points, the +- pairs cancel
        for (int k = tid; k < NP; k += 256)
                Xbar[k] = (k < 3) ? xb[k] : (k < n) ? W.wsum * X[k] : 0.0;
        // pose rows: Zsig passes the pose through (common.h:78-90)
        const double zp[3] = {xb[0], xb[1], (double)normalizeAngle((float)xb[2])};
        const double zscale = sqrt(-W.w_0);
        for (int i = tid; i < mk; i += 256)
        {
#pragma unroll
                for (int k = 0; k < 3; ++k)
                {
                        double dv = 0.0, dz = 0.0;
                        if (i < m)
                        {
                                const double p = XP[k * MP + i]; // (this thread's own store)
                                dv = p - xb[k];
                                dz = p - zp[k];
                                if (k == 2)
                                        dv = (double)normalizeAngle((float)dv), dz = (double)normalizeAngle((float)dz);
                        }
                        Dg[(size_t)k * MP + i] = dv;
                        DZg[(size_t)k * MP + i] = dz;
                        if (i == 0)
                        {
                                double zd = Z[k] - zp[k];
                                if (k == 2)
                                        zd = (double)normalizeAngle((float)zd);
                                G[(size_t)n * NP + k] = zscale * dz; // z = sqrt(-w0) dz_0: the rank-one part of S
                                G[(size_t)(n + 1) * NP + k] = zd;    // Z - Zpred (ukf.cpp:381-386)
                        }
                }
        }
}

// ------------------------------------------------------------------------------------------------------------------
/// Landmark rows of D and DZ: workgroup = landmark j (rows ka = 3 + 2 j, kb = ka + 1).  Sigma point i carries X(k) +- w L(k, c_i); its reading
/// is h of those two entries seen from ITS propagated pose.  A sigma point moves the landmark or the pose only if its column of L is c <= kb
/// (L is lower triangular; c < 3 are the pose columns) or the acceleration-noise column c = n: every other one reproduces the centre point's
/// reading bit for bit and takes it without evaluating h again.  grid (NP / 2, B), 256 threads.
__global__ __launch_bounds__(256) void ukf_large_points(DevView d, LargeView<double> lv, UkfLargeView uv, const int *skipped)
{
        __shared__ double red[2][256];
        const int b = blockIdx.y;
        if (skipped[b])
                return;
        const int n = d.n[b], NP = lv.NP, MP = uv.MP, tid = threadIdx.x;
        const int j = blockIdx.x;
        if (j >= (n - 3) / 2)
                return;
        const int ka = 3 + 2 * j, kb = ka + 1;
        const UkfWeights W = ukf_weights(n);
        const int m = W.m, mk = (m + 15) & ~15;
        const double *X = d.X + (size_t)b * NP, *Z = d.Z + (size_t)b * NP;
        const double *La = lv.S + (size_t)b * NP * NP + (size_t)ka * NP, *Lb = La + NP; // rows ka, kb of L = chol(P)
        double *G = lv.G + (size_t)b * NP * NP;
        const double *XP = uv.XP + (size_t)b * 3 * MP, *Xbar = uv.Xbar + (size_t)b * NP;
        double *Da = uv.D + ((size_t)b * NP + ka) * MP, *Db = Da + MP;
        double *DZa = uv.DZ + ((size_t)b * NP + ka) * MP, *DZb = DZa + MP;
        const double xa = X[ka], xb = X[kb], xbar_a = Xbar[ka], xbar_b = Xbar[kb];
        auto hread = [&](double lx, double ly, int i, double &zr, double &zb) {
                const double ddx = lx - XP[i], ddy = ly - XP[MP + i];
                zr = sqrt(ddx * ddx + ddy * ddy);
                zb = atan2(ddy, ddx) - XP[2 * MP + i];
        };
        double z0r, z0b;
        hread(xa, xb, 0, z0r, z0b); // the centre point's reading
        double sr = 0.0, sb = 0.0;
        for (int i = tid; i < mk; i += 256)
        {
                double zr = 0.0, zb = 0.0, da = 0.0, db = 0.0;
                if (i < m)
                {
                        int c;
                        double sg;
                        ukf_col_of(i, n, c, sg);
                        const double la = (c >= 0 && c <= ka) ? La[c] : 0.0; // (c <= ka < n; blocks right of the diagonal block are not L)
                        const double lb = (c >= 0 && c <= kb) ? Lb[c] : 0.0;
                        const double lx = ukf_xsig(xa, la, c, sg, W.wsp), ly = ukf_xsig(xb, lb, c, sg, W.wsp);
                        if (i == 0 || c <= kb || c == n)
                                hread(lx, ly, i, zr, zb);
                        else
                                zr = z0r, zb = z0b;
                        const double w = (i == 0) ? W.w_0 : W.w_i;
                        sr = fma(w, zr, sr);
                        sb = fma(w, zb, sb);
                        da = lx - xbar_a;
                        db = ly - xbar_b;
                }
                Da[i] = da;
                Db[i] = db;
                DZa[i] = zr; // Zsig for now
                DZb[i] = zb;
        }
        red[0][tid] = sr;
        red[1][tid] = sb;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1)
        {
                if (tid < o)
                {
                        red[0][tid] += red[0][tid + o];
                        red[1][tid] += red[1][tid + o];
                }
                __syncthreads();
        }
        // Zpred (ukf.cpp:329-339), DZ = Zsig - Zpred (ukf.cpp:346-351)
        const double zpr = red[0][0], zpb = (double)normalizeAngle((float)red[1][0]);
        const double zscale = sqrt(-W.w_0);
        for (int i = tid; i < m; i += 256)
        {
                const double dr = DZa[i] - zpr, db = (double)normalizeAngle((float)(DZb[i] - zpb)); // (this thread's own stores)
                DZa[i] = dr;
                DZb[i] = db;
                if (i == 0)
                {
                        G[(size_t)n * NP + ka] = zscale * dr;
                        G[(size_t)n * NP + kb] = zscale * db;
                        G[(size_t)(n + 1) * NP + ka] = Z[ka] - zpr;
                        G[(size_t)(n + 1) * NP + kb] = (double)normalizeAngle((float)(Z[kb] - zpb));
                }
        }
}

// ------------------------------------------------------------------------------------------------------------------
/// C = A diag(w) B^T over the K = 2 N + 5 sigma points (rounded up to 16: the padding columns of D / DZ are zero and so are their weights) on the
/// f64 MFMA -- the hot path of the chain, launched three times per callback:
///   WABT_P   A = B = D:   P <- D W D^T + Q                                   lower 128x128 tiles, mirrored on store; P's padding is not touched
///   WABT_S   A = B = DZ:  S <- DZ W DZ^T + R WITHOUT the i = 0 term (= S+)   lower tiles; identity on rows / columns n .. na - 1
///   WABT_TC  A = D, B = DZ: G <- D W DZ^T (= Tc)                             all tiles; zero on the padding, rows n, n + 1 (z^T, the innovation) kept
/// The tile product is large_syrk's, tile128_f64_product (ekf_large.h), over slabs of 16 sigma points, with A scaled by the weights on the way into
/// LDS; a filter's tiles on one XCD.  grid (8 * tiles * ceil(B / 8)), 256 threads.
enum
{
        WABT_P = 0,
        WABT_S = 1,
        WABT_TC = 2
};
__host__ __device__ __forceinline__ int ukf_wabt_tiles(int NP, int mode)
{
        const int ntile = (NP + 127) / 128;
        return mode == WABT_TC ? ntile * ntile : ntile * (ntile + 1) / 2;
}
__global__ __launch_bounds__(256) void ukf_large_wabt(DevView d, LargeView<double> lv, UkfLargeView uv, int mode, int nfilters, const int *skipped)
{
        typedef Mfma<double> MM;
        constexpr int TB = T128, KC = T128_KC;
        __shared__ double As[TB][T128_LD];
        __shared__ double Bs[TB][T128_LD];
        const int ntile = (lv.NP + TB - 1) / TB, ntl = ukf_wabt_tiles(lv.NP, mode);
        const int slot = blockIdx.x >> 3;
        const int b = (slot / ntl) * 8 + (blockIdx.x & 7);
        if (b >= nfilters || skipped[b])
                return;
        const int n = d.n[b], NP = lv.NP, MP = uv.MP;
        const int na = large_blocks(n, lv.xrows) * LB;
        const int tl = slot % ntl;
        int rt, jt;
        if (mode == WABT_TC)
                rt = tl / ntile, jt = tl - rt * ntile;
        else
        {
                const TriIndex tile = tri_index(tl);
                rt = tile.i, jt = tile.j;
        }
        if (rt * TB >= na || jt * TB >= na)
                return;
        const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15;
        const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
        const double *A = (mode == WABT_S ? uv.DZ : uv.D) + (size_t)b * NP * MP;
        const double *Bm = (mode == WABT_P ? uv.D : uv.DZ) + (size_t)b * NP * MP;
        const UkfWeights W = ukf_weights(n);
        const double w_first = (mode == WABT_S) ? 0.0 : W.w_0; // S+ leaves the centre point out
        const int kend = (W.m + KC - 1) / KC * KC;            // <= MP
        // 16-row / 16-column subtiles of this wave's quadrant that hold at least one of the n valid rows / columns; the upper quadrant of a diagonal
        // tile of a symmetric product is the mirror image of its lower one: neither is multiplied
        const bool sym = mode != WABT_TC;
        const bool idle = sym && rt == jt && wc > wr;
        const int nu = idle ? 0 : __builtin_amdgcn_readfirstlane(max(0, min(4, (n - (rt * TB + wr) + 15) >> 4)));
        const int nv = idle ? 0 : __builtin_amdgcn_readfirstlane(max(0, min(4, (n - (jt * TB + wc) + 15) >> 4)));
        typedef double d2 __attribute__((ext_vector_type(2)));
        MM::acc_t acc[4][4];
        // A goes into LDS scaled by the weights of its two sigma points k0, k0 + 1: weights(i) * diff first, as the reference does
        tile128_f64_product(As, Bs, A, Bm, MP, na, rt, jt, kend, nu, nv,
                            [&](double *dst, const d2 &t, int k0) {
                                    const double w0 = (k0 == 0) ? w_first : (k0 < W.m) ? W.w_i : 0.0;
                                    const double w1 = (k0 + 1 < W.m) ? W.w_i : 0.0;
                                    dst[0] = w0 * t[0];
                                    dst[1] = w1 * t[1];
                            },
                            acc);
        if (idle)
                return;
        double *C = (mode == WABT_P ? lv.P : mode == WABT_S ? lv.S : lv.G) + (size_t)b * NP * NP;
        // Q on the pose diagonal of P- (ukf.cpp:66-68), R on the diagonal of S (ukf.cpp:378): this filter's record, read once behind the product loop
        const aslam_params *const prm = d.prm + b;
        double q_xy = 0.0, q_yaw = 0.0, r_xy = 0.0, r_yaw = 0.0, r_range = 0.0, r_bearing = 0.0; // (mode is a kernel argument: each launch loads what it adds)
        if (mode == WABT_P)
                q_xy = prm->q_xy, q_yaw = prm->q_yaw;
        else if (mode == WABT_S)
                r_xy = prm->r_xy, r_yaw = prm->r_yaw, r_range = prm->r_range, r_bearing = prm->r_bearing;
        const bool diagq = sym && rt == jt && wc == wr; // holds (i, j) and (j, i): the lower one is stored to both places
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                {
                        const int col = jt * TB + wc + 16 * v + li;
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                        {
                                const int row = rt * TB + wr + 16 * u + MM::row(lane, r);
                                if (row >= na || col >= na || (diagq && col > row))
                                        continue;
                                const bool valid = row < n && col < n;
                                if (mode == WABT_P)
                                {
                                        if (!valid)
                                                continue; // P's padding stays zero
                                        const double val = acc[u][v][r] + ((row == col && row < 3) ? (row < 2 ? q_xy : q_yaw) : 0.0);
                                        C[(size_t)row * NP + col] = val;
                                        if (row != col) // (the mirror image; a diagonal quadrant stores its lower half to both places)
                                                C[(size_t)col * NP + row] = val;
                                }
                                else if (mode == WABT_S)
                                {
                                        const double val = valid ? acc[u][v][r] + (row == col ? (row < 2 ? r_xy : row == 2 ? r_yaw : (row & 1) ? r_range : r_bearing) : 0.0) : (row == col ? 1.0 : 0.0);
                                        C[(size_t)row * NP + col] = val;
                                        if (diagq && row != col)
                                                C[(size_t)col * NP + row] = val;
                                }
                                else
                                {
                                        if (valid)
                                                C[(size_t)row * NP + col] = acc[u][v][r];
                                        else if (row >= n + UKF_LARGE_XROWS || col >= n)
                                                C[(size_t)row * NP + col] = 0.0; // (rows n, n + 1 below column n: z^T and the innovation, written by the sigma-point kernels)
                                }
                        }
                }
}

// ------------------------------------------------------------------------------------------------------------------
/// After the factorisation of the stacked matrix: W = Tc L^-T in rows 0 .. n-1 of G, q = L^-1 z in row n, t = L^-1 (Z - Zpred) in row n + 1.
///   K Zdiff = Tc S^-1 Zdiff = W t + g (q.t) / (1 - q.q),  g = W q      (S = S+ - z z^T, Sherman-Morrison: DESIGN.md section 4)
/// One wave per state row: X(a) = Xbar(a) + W(a,:) t + g(a) (q.t) / (1 - q.q) (ukf.cpp:389); g -> lv.Y, 1 / (1 - q.q) -> sc[3] for
/// ukf_large_rank1; in replay mode the pose of this callback.  grid (ceil(NP / 4), B), 256 threads.
template <int MODE>
__global__ __launch_bounds__(256) void ukf_large_gain(DevView d, LargeView<double> lv, UkfLargeView uv, int s, int nsteps, double *poses_out,
                                                      int32_t *dims_out, const int *skipped)
{
        const int b = blockIdx.y;
        if (skipped[b])
                return;
        const int n = d.n[b], NP = lv.NP;
        const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (a >= n)
                return;
        const double *vrow = lv.G + ((size_t)b * NP + a) * NP;
        const double *q = lv.G + ((size_t)b * NP + n) * NP, *tt = q + NP;
        typedef double d2 __attribute__((ext_vector_type(2)));
        double g = 0.0, u = 0.0, qq = 0.0, qt = 0.0;
        // 16 bytes per lane and load; column n of all three rows is zero (n is odd: the last pair reaches it)
        for (int j = 2 * lane; j < n; j += 128)
        {
                const d2 v = *reinterpret_cast<const d2 *>(vrow + j), qv = *reinterpret_cast<const d2 *>(q + j), tv = *reinterpret_cast<const d2 *>(tt + j);
#pragma unroll
                for (int e = 0; e < 2; ++e)
                {
                        g = fma(v[e], qv[e], g);
                        u = fma(v[e], tv[e], u);
                        qq = fma(qv[e], qv[e], qq);
                        qt = fma(qv[e], tv[e], qt);
                }
        }
        g = wave_sum_dpp(g), u = wave_sum_dpp(u), qq = wave_sum_dpp(qq), qt = wave_sum_dpp(qt);
        if (lane == 63)
        {
                const double inv_den = 1.0 / (1.0 - qq);
                const double xa = uv.Xbar[(size_t)b * NP + a] + u + g * (qt * inv_den);
                d.X[(size_t)b * NP + a] = xa;
                lv.Y[(size_t)b * NP + a] = g;
                if (a == 0)
                        uv.sc[(size_t)b * 8 + 3] = inv_den;
                if (MODE == MODE_REPLAY)
                {
                        if (a < 3 && poses_out)
                                poses_out[((size_t)b * nsteps + s) * 3 + a] = xa;
                        if (a == 0 && dims_out)
                                dims_out[(size_t)b * nsteps + s] = n;
                }
        }
}

/// P <- P - g g^T / (1 - q.q): what the negative central weight leaves of K S K^T behind large_syrk's W W^T.  One wave per row.
/// grid (ceil(NP / 4), B), 256 threads.
__global__ __launch_bounds__(256) void ukf_large_rank1(DevView d, LargeView<double> lv, UkfLargeView uv, const int *skipped)
{
        const int b = blockIdx.y;
        if (skipped[b])
                return;
        const int n = d.n[b], NP = lv.NP;
        const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (a >= n)
                return;
        const double *g = lv.Y + (size_t)b * NP;
        const double inv_den = uv.sc[(size_t)b * 8 + 3], ga = g[a];
        double *prow = lv.P + ((size_t)b * NP + a) * NP;
        for (int c = lane; c < n; c += 64)
                prow[c] -= (ga * g[c]) * inv_den;
}
} // namespace aslam
