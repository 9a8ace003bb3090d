// ekf_large.h -- EKF-SLAM for state dimensions beyond one CU (144 < n <= 1087; BASELINE configs[3]/[4]: 512 landmarks,
// n = 1027), fp64 or fp32.  One callback = a short chain of launches that use the whole GPU for one filter (and
// `batch` filters side by side through blockIdx.y/z):
//
//   large_frontend   cbSensorLandmark + updateZandA (ekf.cpp:102-213, shared small_frontend code; LDS: LargeLds = sX, sZ + the block of small_common.h), predict
//                    (X <- f(X), P <- A P A^T + Q with A = I + 2 entries, ekf.cpp:295-297), updateH coefficients
//                    (ekf.cpp:117-134), Y = Z - h(X) (ekf.cpp:302-307)                               1 workgroup / filter
//   large_build_GS   G = P H^T (H has <= 5 non-zeros per row, ekf.cpp:301) and S = H G + R (ekf.cpp:300) in one pass
//                    over P; Y^T appended to G as row n
//   17 x { potrf_inv, update_panel }   blocked Cholesky S = L L^T of the STACKED matrix [S; G; Y^T], 64-wide block
//                    columns: a one-wave in-register factorisation of the diagonal block that also yields its inverse,
//                    then ONE MFMA kernel per block column that brings the column up to date with all earlier ones
//                    (left-looking, K = 64 k), eliminates it (X <- X Linv^T, a 64-deep product instead of a triangular
//                    solve) and updates the diagonal blocks below (right-looking).  The same launches that factor S
//                    turn G into V = G L^-T and Y^T into (L^-1 Y)^T, so K = P H^T S^-1 = V L^-1 never needs a
//                    separate triangular solve
//   large_syrk       P <- P - V V^T        ( = (I - K H) P, ekf.cpp:310, since K H P = V V^T for symmetric P ),
//                    128x128 tiles, lower half mirrored, one filter's tiles on one XCD
//   large_x_update   X <- X + V (L^-1 Y)   ( = X + K Y, ekf.cpp:309 )
// The binary32 mode with many filters per launch runs the same steps as SIX launches (ekf_large_launch.h): front end, G and S, large_chol_bf16,
// large_trsm_bf16 (ekf_large_trsm16.h), large_x_update_rows, large_syrk_bf16x3.  There a state of n = n0 + t, n0 a multiple of 64 and t <= 3 -- the
// benchmark's n = 1027 = 16 x 64 + 3 -- is factored and solved over its n0 / 64 full blocks only, and the t x t tail is a BORDER solved in binary64 by
// large_x_update_rows, which for that reason runs in front of the syrk: large_border() below is the one rule every kernel and the launch plan read.
//
// Unlike the single-CU kernel this path does not go through measurement coordinates: in fp32 the H / H^-1 change of
// basis would cost eps * cond(H)^2 per callback; G, S, V are formed directly (2.33 n^3 flops all the same).
// It does use the symmetry of P (P H^T = (H P)^T, K H P = V V^T); the reference's P is symmetric up to rounding.
// Matrices are row-major in HBM with row stride NP (multiple of 64, zero padding); GEMMs run on the 16x16x4 MFMA
// (f64 or f32 inputs), operands staged through LDS.
#pragma once

#include <type_traits>

#include "small_common.h"

namespace aslam
{
constexpr int LB = 64;               // block size of the factorisation = GEMM tile edge
constexpr int LARGE_OBS_CAP = 1024;  // stored sensor message (LDS)
constexpr int LARGE_WAIT_CAP = 2048; // wait-list (LDS)
constexpr int LARGE_NP_MAX = 1088;   // 17 blocks of 64: n <= 1087
constexpr int LARGE_NB_MAX = LARGE_NP_MAX / LB;

template <typename T> struct LargeView // (its arrays, their sizes per filter and which must start zero: for_each_array below, behind LPlanes)
{
        int NP;     // row stride, multiple of LB
        double *P;  // [B][NP][NP]  always binary64 (fp32 mode: only G, S, L, V and the MFMA products are binary32)
        T *G;       // [B][NP][NP]  P H^T, then V; row n carries Y^T, then (L^-1 Y)^T
        T *S;       // [B][NP][NP]  innovation covariance, then L (lower)
        double *Hc; // [B][NP/2][4] h00 h01 h10 h11 per landmark
        double *Y;  // [B][NP]
        T *Linv;    // [B][LARGE_NB_MAX][LB][LB]  inverses of the diagonal blocks of L
        T *Vw;      // [B][NP][NP]  binary32 mode, few-filter chain (large_right_step): V is written HERE, not over G (every block of G is read by many workgroups of a launch); else nullptr
        unsigned short *Lpl; // binary32 mode with the bf16-pipe TRSM: LPlanes::base (bf16 planes of L and of the inverses, written by large_chol_resident), else nullptr
        int xrows;  // vector rows that ride in G behind the n state rows through the factorisation: 1 (EKF: Y^T), 2 (large-state UKF: z^T and the innovation, ukf_large.h)
        int border; // 1: this launch solves a short tail past the last full 64-block as a binary64 border (large_border below; set per launch from LargePlan::border), else 0
        int syrk_tail; // 1: large_syrk_bf16x3<false> forms a last tile row of <= 16 state rows on the idle waves of its diagonal tiles (large_syrk_tail below; LargePlan::syrk_tail), else 0
};

// ---- MFMA traits -------------------------------------------------------------------------------------------------
typedef float f4 __attribute__((ext_vector_type(4)));
template <typename T> struct Mfma;
template <> struct Mfma<double>
{
        typedef d4 acc_t;
        static __device__ __forceinline__ acc_t zero()
        {
                return (acc_t){0.0, 0.0, 0.0, 0.0};
        }
        static __device__ __forceinline__ acc_t mma(double a, double b, acc_t c)
        {
                return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
        }
        // C/D element (row, col) of register r in lane l
        static __device__ __forceinline__ int row(int lane, int r)
        {
                return (lane >> 4) + 4 * r;
        }
};
template <> struct Mfma<float>
{
        typedef f4 acc_t;
        static __device__ __forceinline__ acc_t zero()
        {
                return (acc_t){0.f, 0.f, 0.f, 0.f};
        }
        static __device__ __forceinline__ acc_t mma(float a, float b, acc_t c)
        {
                return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
        }
        static __device__ __forceinline__ int row(int lane, int r)
        {
                return (lane >> 4) * 4 + r;
        }
};

/// acc = A(rows of tile rt, 0 .. kend-1) B(rows of tile jt, 0 .. kend-1)^T: one 128x128 tile of a binary64 product on the 16x16x4 MFMA, the loop of
/// large_syrk (A = B = V) and of ukf_large_wabt (A = D or DZ scaled by the sigma-point weights, ukf_large.h).  256 threads, 4 waves, wave w the
/// 64x64 quadrant (w >> 1, w & 1) as 4x4 MFMA tiles in acc[u][v].  A and B are row-major with row stride ld; slabs of T128_KC columns go through
/// LDS, the next one fetched into registers while the current one is multiplied.  Staging: 8 lanes cover one 128-byte row segment with 16-byte
/// loads, so every wave-level load fetches 8 whole cache lines; 4 passes of 32 rows.  A tile may hang over the na active rows: such rows read row
/// na - 1 instead (the caller never stores their products).  store_a(dst, t, k) puts a thread's pair t = A(row, k .. k+1) at dst in As: the one
/// place where the callers' loops differ.  nu / nv: 16-row / 16-column subtiles of this wave's quadrant to multiply (wave-uniform; 0: the wave only
/// stages).  kend is a multiple of T128_KC.
constexpr int T128 = 128, T128_KC = 16, T128_LD = T128_KC + 2;
template <typename StoreA>
__device__ __forceinline__ void tile128_f64_product(double (&As)[T128][T128_LD], double (&Bs)[T128][T128_LD], const double *A, const double *B, int ld,
                                                    int na, int rt, int jt, int kend, int nu, int nv, StoreA &&store_a, d4 (&acc)[4][4])
{
        typedef Mfma<double> MM;
        typedef double d2 __attribute__((ext_vector_type(2)));
        constexpr int KC = T128_KC;
        const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4;
        const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
        const int lrow = tid >> 3, lc0 = (tid & 7) * 2;
        const double *Ap[4], *Bp[4];
#pragma unroll
        for (int q = 0; q < 4; ++q)
        {
                Ap[q] = A + (size_t)min(rt * T128 + lrow + 32 * q, na - 1) * ld + lc0;
                Bp[q] = B + (size_t)min(jt * T128 + lrow + 32 * q, na - 1) * ld + lc0;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                        acc[u][v] = MM::zero();
        d2 ta[4], tb[4];
        auto fetch = [&](int kc) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                {
                        ta[q] = *reinterpret_cast<const d2 *>(Ap[q] + kc);
                        tb[q] = *reinterpret_cast<const d2 *>(Bp[q] + kc);
                }
        };
        const bool full = (nu == 4 && nv == 4);
        fetch(0);
        for (int kc = 0; kc < kend; kc += KC)
        {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                {
                        store_a(&As[lrow + 32 * q][lc0], ta[q], kc + lc0);
                        *reinterpret_cast<d2 *>(&Bs[lrow + 32 * q][lc0]) = tb[q];
                }
                __syncthreads();
                if (kc + KC < kend)
                        fetch(kc + KC);
                if (full)
                {
#pragma unroll
                        for (int s = 0; s < KC / 4; ++s)
                        {
                                double av[4], bv[4];
#pragma unroll
                                for (int u = 0; u < 4; ++u)
                                {
                                        av[u] = As[wr + 16 * u + li][lg + 4 * s];
                                        bv[u] = Bs[wc + 16 * u + li][lg + 4 * s];
                                }
#pragma unroll
                                for (int u = 0; u < 4; ++u)
#pragma unroll
                                        for (int v = 0; v < 4; ++v)
                                                acc[u][v] = MM::mma(av[u], bv[v], acc[u][v]);
                        }
                }
                else
                {
#pragma unroll
                        for (int u = 0; u < 4; ++u)
                                if (u < nu)
#pragma unroll
                                        for (int v = 0; v < 4; ++v)
                                                if (v < nv)
#pragma unroll
                                                        for (int s = 0; s < KC / 4; ++s)
                                                                acc[u][v] = MM::mma(As[wr + 16 * u + li][lg + 4 * s], Bs[wc + 16 * v + li][lg + 4 * s],
                                                                                    acc[u][v]);
                }
                __syncthreads();
        }
}

/// four floats -> their three bf16 planes, packed two to a register: x = h + m + l up to 2^-25 |x|.  Round to nearest at every level
/// (v_cvt_pk_bf16_f32): with truncated pieces, which all carry the sign of x, the dropped terms of a split product have the sign of the product
/// (large_syrk_bf16x3).
typedef unsigned u2x __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void split_bf16x3(const f4 &x, u2x &h, u2x &m, u2x &l)
{
        typedef float f2 __attribute__((ext_vector_type(2)));
        typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int e = 0; e < 2; ++e)
        {
                const f2 v = {x[2 * e], x[2 * e + 1]};
                const bf2 hh = __builtin_convertvector(v, bf2);
                const f2 r1 = v - __builtin_convertvector(hh, f2);
                const bf2 mm = __builtin_convertvector(r1, bf2);
                const f2 r2 = r1 - __builtin_convertvector(mm, f2);
                const bf2 ll = __builtin_convertvector(r2, bf2);
                h[e] = __builtin_bit_cast(unsigned, hh), m[e] = __builtin_bit_cast(unsigned, mm), l[e] = __builtin_bit_cast(unsigned, ll);
        }
}

/// Planes of L in HBM (binary32 mode; written by the resident Cholesky kernels, streamed by large_trsm_bf16 / large_chol_bf16 --
/// ekf_large_trsm16.h), per filter: Lq [3][NP][NP] bf16, row-major, columns permuted inside every 64-block.  Block (k, j), j < k, holds L(k, j);
/// the DIAGONAL block (k, k) holds the INVERSE of L(k, k) -- the sweeps multiply by it and never read L(k, k) itself -- so that every block of a
/// sweep's sequence  Linv_0; L(1,0), Linv_1; L(2,0), L(2,1), Linv_2; ...  has the same row / plane strides and its address is one multiply-add
/// (the round's first layout kept the inverses behind the planes: 40 scalar instructions and three branches per block to pick the layout).
struct LPlanes
{
        unsigned short *base;
        __host__ __device__ static size_t per_filter(int NP) { return (size_t)3 * NP * NP; }
        __host__ __device__ unsigned short *Lq(int b, int NP) const { return base + (size_t)b * per_filter(NP); }
        /// plane 0 of block (k, j) (row stride NP, plane stride NP * NP)
        __host__ __device__ unsigned short *block(int b, int NP, int k, int j) const { return Lq(b, NP) + (size_t)(64 * k) * NP + 64 * j; }
};
/// the per-filter arrays of a LargeView, in allocation order; G, S and Vw must be zero when a filter starts: the kernels rely on padding they
/// never write (see for_each_array(DevView &) in small_common.h).  Vw and Lpl are null in contexts whose plan does not need them
template <typename T, typename F> void for_each_array(LargeView<T> &v, F &&f)
{
        const size_t np = (size_t)v.NP;
        f(v.P, np * np, false);
        f(v.G, np * np, true);
        f(v.S, np * np, true);
        f(v.Hc, (np / 2) * 4, false);
        f(v.Y, np, false);
        f(v.Linv, (size_t)LARGE_NB_MAX * LB * LB, false);
        f(v.Lpl, LPlanes::per_filter(v.NP), false);
        f(v.Vw, np * np, true);
}

/// position of column c (0 .. 63) of a block inside a permuted plane row: 32 h + 8 g + 4 w + r holds column 32 h + 16 w + 4 g + r
__host__ __device__ __forceinline__ int lplane_pos(int c)
{
        return 32 * (c >> 5) + 8 * ((c >> 2) & 3) + 4 * ((c >> 4) & 1) + (c & 3);
}

/// number of active 64-blocks: the n state rows plus the vector rows that ride in G (LargeView::xrows; the EKF's one row, Y^T, where no view is at hand)
__host__ __device__ __forceinline__ int large_blocks(int n, int xrows = 1)
{
        return (n + xrows + LB - 1) / LB;
}

/// The border rule (binary32 resident chain on the bf16 pipe, LargeView::border).  n = n0 + t with n0 = 64 floor(n / 64): a tail of t <= 3 rows past the
/// last full 64-block (n is odd: t = 1 or 3; n = 1027 = 16 x 64 + 3 is the benchmark's size) would cost a whole block row and block column of the
/// factorisation, of the solve and of the staging of P -= V V^T.  Instead, with S = [S11 S21^T; S21 S22] and G = [G1 G2]:
///     L11 = chol(S11)                       large_chol_bf16 over nbc = n0 / 64 block rows
///     [V1; l] = [G1; S21] L11^-T            large_trsm_bf16 over nbc block columns; S21 rides in rows n+1 .. n+t of G (large_build_GS puts it there)
///     C = S22 - l l^T = L22 L22^T           t x t, binary64: large_x_update_rows, which reads every row of V anyway
///     V2 = (G2 - V1 l^T) L22^-T             large_x_update_rows; stored over G2, row n included
/// so that V = [V1 V2] is the V of the full factorisation up to rounding and every consumer (the syrk, q.q, ln det S) reads it as before.
/// `t` = 0: no border for this n (the whole chain runs over large_blocks(n) blocks, as without the rule).
struct LargeBorder
{
        int t;   // border width: 0 (none), 1 or 3
        int nbc; // block columns the Cholesky factors and the TRSM sweeps: n0 / 64 with a border, else large_blocks(n)
};
__host__ __device__ __forceinline__ LargeBorder large_border(int n, int enabled)
{
        const int n0 = n & ~(LB - 1), t = n - n0;
        const bool on = enabled && n0 >= LB && (t == 1 || t == 3);
        return {on ? t : 0, on ? n0 / LB : large_blocks(n)};
}
constexpr int BORDER_MAX = 3;  // widest border

/// The tail rule of large_syrk_bf16x3 (LargeView::syrk_tail).  rl = (n - 1) / 128 is the last row of 128x128 tiles that holds state rows.  When it holds no
/// more than 16 of them -- ONE 16-row MFMA tile; the benchmark's n = 1027 = 8 x 128 + 3 -- the tiles (rl, jt), jt < rl, would stage 33 slabs of 2 x 128 rows
/// each for two waves' worth of one row tile.  Instead the idle wave of every diagonal tile (jt, jt), jt < rl, whose Bs already holds the planes of column
/// tile jt, forms rows 128 rl .. n-1 x columns 128 jt .. + 127 with its A operand read straight into registers, and the tiles (rl, jt), jt < rl, return at
/// once.  Same operands, same products in the same order, same epilogue arithmetic: bit-identical.  The corner tile (rl, rl) stays as it is.
/// `rows` = 0: no tail for this n (every tile of row rl runs as without the rule).
struct SyrkTail
{
        int rl;   // last tile row with state rows
        int rows; // state rows in it when the rule holds (1 .. 16), else 0
};
__host__ __device__ __forceinline__ SyrkTail large_syrk_tail(int n, int enabled)
{
        const int rl = (n - 1) / 128, t = n - 128 * rl;
        return {rl, enabled && rl >= 1 && t <= 16 ? t : 0};
}
// Rows n+1 .. n+t of G are spare (n + 1 + t <= n0 + 7 < n0 + 64 <= NP; nothing downstream reads them as V: the syrk stores no row >= n, large_stats and
// the X update read row n and rows < n).  Row n+1+k carries row k of S21 in columns < n0 and, in columns n0 + BORDER_SAVE + m, a copy of column n0 + k
// of the rows of G2 every workgroup of the X update needs while their owners overwrite them with V2: m = 0 .. 2 the pose rows, m = 3 row n (Y^T).
constexpr int BORDER_SAVE = 8, BORDER_SAVE_ROWS = 4;
__host__ __device__ __forceinline__ bool border_spare(const LargeBorder &bd, int n, int row, int col) // an entry of G that large_build_GS* must not clear
{
        return bd.t && row > n && row <= n + bd.t && (col < LB * bd.nbc || (col >= LB * bd.nbc + BORDER_SAVE && col < LB * bd.nbc + BORDER_SAVE + BORDER_SAVE_ROWS));
}

// ---- LDS layout of the front-end workgroup (runtime NP): sX, sZ, then the association block of small_common.h with the LARGE_* capacities ----
struct LargeLds
{
        static __host__ __device__ constexpr size_t bytes(int NP) { return assoc_shared_at(8 * (size_t)NP * 2, LARGE_OBS_CAP, LARGE_WAIT_CAP, NP) + sizeof(SmallShared); }
        /// the dynamic LDS of a launch: the GATED front ends keep the gate table of small_frontend behind everything else
        static __host__ __device__ constexpr size_t launch_bytes(int NP, bool gated) { return bytes(NP) + (gated ? 8 * gate_table_doubles(NP) : 0); }
        static __host__ __device__ constexpr size_t gate_table_at(int NP) { return bytes(NP); } // (byte offset of the table in the workgroup's LDS)
        static __device__ __forceinline__ SmallLds carve(unsigned char *smem, int NP)
        {
                SmallLds L = {};
                AssocCarve c = {smem};
                c(L.sX, NP);
                c(L.sZ, NP);
                unsigned char *const p = assoc_carve(L, c.p, LARGE_OBS_CAP, LARGE_WAIT_CAP, NP);
                L.sm = reinterpret_cast<SmallShared *>(smem + (((size_t)(p - smem) + 15) & ~(size_t)15)); // (= assoc_shared_at)
                return L;
        }
};

// ------------------------------------------------------------------------------------------------------------------
/// Per-filter front end + predict (one workgroup of SMALL_WG threads per filter).  `skipped` [B] is set to 1 when the
/// callback returned early (no sensor message yet): the rest of the chain then leaves the filter alone.
/// SIGHTED (aslam_sighted_update_enable): Y is zeroed in the rows of the landmarks this callback did not sight (DevView::sighted, which the front
/// end has just written in replay and the host has copied down for a step); large_build_GS<T, true> does the rest.
/// GATED (aslam_set_replay_gate, MODE_REPLAY only; LargeLds::launch_bytes(NP, true) of dynamic LDS): the front end associates by the Mahalanobis gate in the
/// filters whose gate is > 0 (small_frontend); P is read through L2.
template <typename T, int MODE, bool SIGHTED = false, bool GATED = false>
__global__ __launch_bounds__(SMALL_WG) void large_frontend_kernel(DevView d, LargeView<T> lv, int64_t t, int s, int nsteps,
                                                                   double *poses_out, int32_t *dims_out, StepArgs sa, int *skipped)
{
        extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
        const int NP = lv.NP;
        const SmallLds L = LargeLds::carve(smem, NP);
        SmallShared &sm = *L.sm;
        double *const sX = L.sX, *const sZ = L.sZ;
        const int tid = threadIdx.x;
        const int b = (MODE == MODE_STEP && sa.traj >= 0) ? sa.traj : (int)blockIdx.x; // sa.traj < 0: the batched step, one workgroup per filter
        double *Pg = lv.P + (size_t)b * NP * NP;
        double *Hc = lv.Hc + (size_t)b * (NP / 2) * 4;
        double *Yg = lv.Y + (size_t)b * NP;

#ifdef ASLAM_STAMPS
        unsigned long long stamp_acc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        unsigned long long stamp_last = __builtin_amdgcn_s_memtime();
        const unsigned long long stamp_rt0 = __builtin_amdgcn_s_memrealtime(); // 100 MHz: wall time inside the kernel
#endif
        small_enter<MODE, true, GATED>(d, L, b, tid, NP);
        ASLAM_STAMP(0);
        if (MODE == MODE_REPLAY)
        {
                if (small_frontend<true, LARGE_OBS_CAP, LARGE_WAIT_CAP, LARGE_NP_MAX / 2, double, GATED>(d, L, Pg, NP, b, t, s, nsteps, poses_out, dims_out, tid, nullptr,
                                                                                                         GATED ? reinterpret_cast<double *>(smem + LargeLds::gate_table_at(NP)) : nullptr))
                {
                        large_frontend_skip<MODE>(d, L, skipped, b, tid, NP);
                        return;
                }
        }
        else
                small_step_intake(d, sm, sa, b, tid);
        ASLAM_STAMP(1);
        if (tid == 0)
                skipped[b] = 0;
        const int n = sm.n;
        const int nl = (n - 3) / 2;
        // X <- f(X), ekf.cpp:295-296
        if (tid == 0)
        {
                double p0 = sX[0], p1 = sX[1], p2 = sX[2];
                stateTransition(p0, p1, p2, sm.vx, sm.az, sm.dt, false, 0.0);
                sX[0] = p0;
                sX[1] = p1;
                sX[2] = (double)normalizeAngle((float)p2);
        }
        __syncthreads();
        // updateH coefficients (ekf.cpp:117-134) and Y = Z - h(X) (ekf.cpp:302-307)
        for (int i = tid; i < nl; i += SMALL_WG)
        {
                const double x0 = sX[0], x1 = sX[1];
                const double lx = sX[3 + 2 * i], ly = sX[4 + 2 * i];
                const double ddx = lx - x0, ddy = ly - x1;
                const float hyp = (float)(ddx * ddx + ddy * ddy);
                const float dist = sqrtf(hyp);
                Hc[4 * i + 0] = (-lx + x0) / (double)dist;
                Hc[4 * i + 1] = (-ly + x1) / (double)dist;
                Hc[4 * i + 2] = -(-ly + x1) / (double)hyp;
                Hc[4 * i + 3] = (-lx + x0) / (double)hyp;
                const double hr = sqrt(ddx * ddx + ddy * ddy);
                const double hb = atan2(ddy, ddx) - sX[2];
                Yg[3 + 2 * i] = sZ[3 + 2 * i] - hr;
                Yg[4 + 2 * i] = (double)normalizeAngle((float)(sZ[4 + 2 * i] - hb));
                if constexpr (SIGHTED)
                {
                        if (!d.sighted[(size_t)b * (NP / 2) + i])
                                Yg[3 + 2 * i] = 0.0, Yg[4 + 2 * i] = 0.0;
                }
        }
        if (tid == 0)
        {
                Yg[0] = sZ[0] - sX[0];
                Yg[1] = sZ[1] - sX[1];
                Yg[2] = (double)normalizeAngle((float)(sZ[2] - sX[2]));
        }
        ASLAM_STAMP(2);
        // P <- A P A^T + Q (ekf.cpp:297), A = I except A(0,0), A(1,0): rows 0,1 then columns 0,1
        {
                const double a00 = sm.a00, a10 = sm.a10, q = sm.prm.q_xy, q_yaw = sm.prm.q_yaw; // Q = diag(q_xy, q_xy, q_yaw, 0 ...), ekf.cpp:66-68
                for (int c = tid; c < n; c += SMALL_WG)
                {
                        const double r0 = Pg[c];
                        Pg[c] = a00 * r0;
                        Pg[NP + c] = a10 * r0 + Pg[NP + c];
                }
                __syncthreads();
                for (int r = tid; r < n; r += SMALL_WG)
                {
                        double *row = Pg + (size_t)r * NP;
                        const double c0 = row[0];
                        double v0 = a00 * c0, v1 = a10 * c0 + row[1];
                        if (r == 0)
                                v0 += q;
                        if (r == 1)
                                v1 += q;
                        row[0] = v0;
                        row[1] = v1;
                        if (r == 2)
                                row[2] += q_yaw;
                }
        }
        ASLAM_STAMP(3);
        small_store<MODE>(d, L, b, tid, NP);
        ASLAM_STAMP(4);
#ifdef ASLAM_STAMPS
        if (tid == 0 && blockIdx.x == 0)
        {
                for (int i = 0; i < 12; ++i)
                        d.dbg[i] += stamp_acc[i];
                d.dbg[56] += __builtin_amdgcn_s_memrealtime() - stamp_rt0;
                d.dbg[57] += 1;
        }
        if (tid == 0 && blockIdx.x < 1024)
                d.dbg[64 + blockIdx.x] = __builtin_amdgcn_s_memrealtime() - stamp_rt0; // every workgroup of the last launch (single stream group: the views are not shifted)
#endif
}

// ------------------------------------------------------------------------------------------------------------------
/// G = P H^T (ekf.cpp:301; H has <= 5 non-zeros per row) and S = H G + R (ekf.cpp:300) in one pass over P: a workgroup
/// owns two consecutive rows (a landmark pair, or two padding rows; workgroup 0 the three pose rows), forms their G entries
/// from the P rows it reads, re-forms the three pose rows of G it needs for H G (their P rows stay in L2), and writes G and S
/// without G ever being read back.  Also copies Y^T into row n of G.  Threads run over landmark column pairs.
/// P is binary64 in both modes and the products are formed in binary64; G and S are rounded to T on the way out (in fp32 mode
/// that is the one rounding of G).  Only the lower block triangle of S (with full diagonal blocks) is consumed downstream and written.  grid (1 + ceil((NP / 2) / GS_ROW_PAIRS), B), 256 threads: workgroup 0 the pose rows, the others GS_ROW_PAIRS landmark row pairs each.
constexpr int GS_ROW_PAIRS = 2; // 4: slower (29.1 k against 29.7 k filter-steps/s on one stream), 1: 28.5 k

///
/// SIGHTED (aslam_sighted_update_enable): the update with the rows M = pose rows + rows of the sighted landmarks alone, as the same chain.  For a
/// row u outside M: column u of G is 0, row and column u of S are those of the identity (and Y_u = 0: the front end) -- in binary64, before any
/// rounding, the copies for the border (put_l, save_g2) included.  L then has a unit row there and column u of V is 0: Cholesky, TRSM, border,
/// X update, syrk and large_stats run unchanged, and ln det / NIS come out as those of S_M.  SIGHTED = false is the code it was.
template <typename T, bool SIGHTED = false> __global__ __launch_bounds__(256) void large_build_GS(DevView d, LargeView<T> lv, const int *skipped)
{
        const uint8_t *const sgt = SIGHTED ? d.sighted + (size_t)blockIdx.y * (lv.NP / 2) : nullptr; // [landmark] of this filter
        const int b = blockIdx.y;
        if (skipped[b])
                return;
        const int n = d.n[b], NP = lv.NP;
        const int na = large_blocks(n) * LB;
        const int nl = (n - 3) / 2;
        const double *P = lv.P + (size_t)b * NP * NP;
        T *G = lv.G + (size_t)b * NP * NP;
        T *S = lv.S + (size_t)b * NP * NP;
        const double *Hc = lv.Hc + (size_t)b * (NP / 2) * 4;
        const aslam_params *const prm = d.prm + b; // (wave-uniform: one filter per workgroup)
        const double r_xy = prm->r_xy, r_yaw = prm->r_yaw, r_range = prm->r_range, r_bearing = prm->r_bearing; // diagonal of R by row class (ekf.cpp:65,278)
        const int tid = threadIdx.x;
        const bool pose = (blockIdx.x == 0);
        constexpr int RP = GS_ROW_PAIRS; // landmark row pairs per workgroup: the pose rows of G and the H coefficients of a column pair are formed once for all of them
        const int r0 = pose ? 0 : 3 + 2 * RP * ((int)blockIdx.x - 1); // first row of this workgroup
        if (r0 >= na)
                return;
        // the border (large_border): rows n0 .. n-1 of S (S21 in columns < n0) also go to rows n+1 .. n+t of G, where the TRSM solves them into l, and
        // the entries of G2 the X update needs from other rows than its own are copied next to them
        const LargeBorder bd = large_border(n, lv.border);
        const int n0 = LB * bd.nbc;
        auto put_l = [&](int r, int c, double v) { // S(r, c), a row of S21
                if (bd.t && r >= n0 && c < n0)
                        G[(size_t)(r + bd.t + 1) * NP + c] = (T)v;
        };
        auto save_g2 = [&](int m, int c, T v) { // G(pose row m, c) (m = 3: Y(c)) for c in n0 .. n-1
                if (bd.t && c >= n0 && c < n)
                        G[(size_t)(n + 1 + c - n0) * NP + n0 + BORDER_SAVE + m] = v;
        };
        int nlive = 0; // leading row pairs that are landmarks (rows < n; n is odd, so a pair never straddles n)
        if (!pose)
        {
                for (int rp = 0; rp < RP; ++rp)
                {
                        const int ra = r0 + 2 * rp;
                        if (ra >= na)
                                break;
                        if (ra < n)
                        {
                                nlive = rp + 1;
                                continue;
                        }
                        // padding rows ra, ra+1: G = 0 (row n: Y^T), S = identity
                        for (int rr = ra; rr < min(ra + 2, na); ++rr)
                        {
                                T *grow = G + (size_t)rr * NP, *srow = S + (size_t)rr * NP;
                                const double *Y = lv.Y + (size_t)b * NP;
                                for (int c = tid; c < na; c += 256)
                                {
                                        if (!border_spare(bd, n, rr, c))
                                                grow[c] = (rr == n && c < n) ? (T)Y[c] : (T)0;
                                        if (rr == n)
                                                save_g2(3, c, (T)Y[c]);
                                        srow[c] = (c == rr) ? (T)1 : (T)0;
                                }
                        }
                }
                if (nlive == 0)
                        return;
        }
        // G(a, :) for one row a of P: columns 0..2 copy P, landmark column pair j mixes (t0, t1, t2, ta, tb) with H_j
        const double *p0 = P, *p1 = P + NP, *p2 = P + 2 * (size_t)NP;
        const double t00 = p0[0], t01 = p0[1], t02 = p0[2], t10 = p1[0], t11 = p1[1], t12 = p1[2], t20 = p2[0], t21 = p2[1], t22 = p2[2];
        const double *pa[RP], *pb[RP]; // landmark rows (unused by the pose workgroup)
        double ta0[RP], ta1[RP], ta2[RP], tb0[RP], tb1[RP], tb2[RP], ha0[RP], ha1[RP], hb0[RP], hb1[RP];
#pragma unroll
        for (int rp = 0; rp < RP; ++rp)
        {
                const int ra = min(r0 + 2 * rp, n - 2); // (pairs beyond nlive are never used: keep their addresses valid)
                pa[rp] = P + (size_t)ra * NP, pb[rp] = pa[rp] + NP;
                ta0[rp] = ta1[rp] = ta2[rp] = tb0[rp] = tb1[rp] = tb2[rp] = ha0[rp] = ha1[rp] = hb0[rp] = hb1[rp] = 0.0;
                if (!pose && rp < nlive)
                {
                        ta0[rp] = pa[rp][0], ta1[rp] = pa[rp][1], ta2[rp] = pa[rp][2];
                        tb0[rp] = pb[rp][0], tb1[rp] = pb[rp][1], tb2[rp] = pb[rp][2];
                        const double *hr = Hc + 4 * ((ra - 3) >> 1);
                        ha0[rp] = hr[0], ha1[rp] = hr[1], hb0[rp] = hr[2], hb1[rp] = hr[3]; // H rows ra (range) and ra+1 (bearing)
                }
        }
        bool row_in[RP]; // SIGHTED: rows ra, ra+1 of this pair are in M
#pragma unroll
        for (int rp = 0; rp < RP; ++rp)
        {
                row_in[rp] = true;
                if constexpr (SIGHTED)
                        row_in[rp] = (!pose && rp < nlive) ? sgt[(r0 + 2 * rp - 3) >> 1] != 0 : true;
        }
        auto grow = [](double h00, double h01, double h10, double h11, double t0, double t1, double t2, double ta, double tb, double &ge,
                       double &go) {
                ge = h00 * t0 + h01 * t1 - h00 * ta - h01 * tb;
                go = h10 * t0 + h11 * t1 - t2 - h10 * ta - h11 * tb;
        };
        // S(r, c) = (H G)(r, c) for landmark row r = ra (+1): ha g0 + hb g1 [- g2] - ha ga - hb gb
        auto srow = [](double ha, double hb, bool odd, double g0, double g1, double g2, double ga, double gb) -> double {
                double v = ha * g0 + hb * g1;
                if (odd)
                        v -= g2;
                return v - ha * ga - hb * gb;
        };
        // ---- pose columns 0..2 (G = P there)
        if (tid < 3)
        {
                const int c = tid;
                const double g0 = p0[c], g1 = p1[c], g2 = p2[c];
                if (pose)
                {
                        G[c] = (T)g0, G[NP + c] = (T)g1, G[2 * (size_t)NP + c] = (T)g2;
                        S[c] = (T)(g0 + (c == 0 ? r_xy : 0.0));
                        S[NP + c] = (T)(g1 + (c == 1 ? r_xy : 0.0));
                        S[2 * (size_t)NP + c] = (T)(g2 + (c == 2 ? r_yaw : 0.0));
                }
                else
                {
#pragma unroll
                        for (int rp = 0; rp < RP; ++rp)
                                if (rp < nlive)
                                {
                                        const int ra = r0 + 2 * rp;
                                        const double ga = pa[rp][c], gb = pb[rp][c];
                                        G[(size_t)ra * NP + c] = (T)ga;
                                        G[(size_t)(ra + 1) * NP + c] = (T)gb;
                                        double sa = srow(ha0[rp], ha1[rp], false, g0, g1, g2, ga, gb), sb = srow(hb0[rp], hb1[rp], true, g0, g1, g2, ga, gb);
                                        if (SIGHTED && !row_in[rp])
                                                sa = 0.0, sb = 0.0; // (a pose column of a row outside M)
                                        S[(size_t)ra * NP + c] = (T)sa;
                                        S[(size_t)(ra + 1) * NP + c] = (T)sb;
                                        put_l(ra, c, sa), put_l(ra + 1, c, sb);
                                }
                }
        }
        // Only the lower block triangle of S and its 64x64 diagonal blocks are consumed downstream (the Cholesky kernels): a row of S
        // stops at the end of the diagonal block of its pair's last row -- 2.1 of the 4.7 MB of S per filter are never written.
        // ---- landmark column pairs
        for (int j = tid; j < nl; j += 256)
        {
                const int ce = 3 + 2 * j, co = ce + 1;
                const double h00 = Hc[4 * j], h01 = Hc[4 * j + 1], h10 = Hc[4 * j + 2], h11 = Hc[4 * j + 3];
                double g0e, g0o, g1e, g1o, g2e, g2o;
                grow(h00, h01, h10, h11, t00, t01, t02, p0[ce], p0[co], g0e, g0o);
                grow(h00, h01, h10, h11, t10, t11, t12, p1[ce], p1[co], g1e, g1o);
                grow(h00, h01, h10, h11, t20, t21, t22, p2[ce], p2[co], g2e, g2o);
                bool col_in = true; // SIGHTED: columns ce, co are in M
                if constexpr (SIGHTED)
                {
                        col_in = sgt[j] != 0;
                        if (!col_in)
                                g0e = g0o = g1e = g1o = g2e = g2o = 0.0;
                }
                if (pose)
                {
                        G[ce] = (T)g0e, G[co] = (T)g0o;
                        G[NP + ce] = (T)g1e, G[NP + co] = (T)g1o;
                        G[2 * (size_t)NP + ce] = (T)g2e, G[2 * (size_t)NP + co] = (T)g2o;
                        save_g2(0, ce, (T)g0e), save_g2(0, co, (T)g0o);
                        save_g2(1, ce, (T)g1e), save_g2(1, co, (T)g1o);
                        save_g2(2, ce, (T)g2e), save_g2(2, co, (T)g2o);
                        if (ce < LB)
                        {
                                S[ce] = (T)g0e, S[co] = (T)g0o;
                                S[NP + ce] = (T)g1e, S[NP + co] = (T)g1o;
                                S[2 * (size_t)NP + ce] = (T)g2e, S[2 * (size_t)NP + co] = (T)g2o;
                        }
                }
                else
                {
#pragma unroll
                        for (int rp = 0; rp < RP; ++rp)
                                if (rp < nlive)
                                {
                                        const int ra = r0 + 2 * rp;
                                        double gae, gao, gbe, gbo;
                                        grow(h00, h01, h10, h11, ta0[rp], ta1[rp], ta2[rp], pa[rp][ce], pa[rp][co], gae, gao);
                                        grow(h00, h01, h10, h11, tb0[rp], tb1[rp], tb2[rp], pb[rp][ce], pb[rp][co], gbe, gbo);
                                        if (SIGHTED && !col_in)
                                                gae = gao = gbe = gbo = 0.0;
                                        T *ga = G + (size_t)ra * NP, *gb = ga + NP, *sa = S + (size_t)ra * NP, *sb = sa + NP;
                                        ga[ce] = (T)gae, ga[co] = (T)gao;
                                        gb[ce] = (T)gbe, gb[co] = (T)gbo;
                                        if (ce < LB * ((ra + 1) / LB + 1))
                                        {
                                                double se = srow(ha0[rp], ha1[rp], false, g0e, g1e, g2e, gae, gbe),
                                                       so = srow(ha0[rp], ha1[rp], false, g0o, g1o, g2o, gao, gbo);
                                                double ue = srow(hb0[rp], hb1[rp], true, g0e, g1e, g2e, gae, gbe),
                                                       uo = srow(hb0[rp], hb1[rp], true, g0o, g1o, g2o, gao, gbo);
                                                if (SIGHTED && !(col_in && row_in[rp]))
                                                {
                                                        se = so = ue = uo = 0.0; // rows and columns outside M: those of the identity
                                                        if (ce == ra)
                                                                se = 1.0, uo = 1.0;
                                                }
                                                else
                                                {
                                                if (ce == ra)
                                                        se += r_range; // R on the diagonal: the range row of the pair ...
                                                if (co == ra + 1)
                                                        uo += r_bearing; // ... and its bearing row
                                                }
                                                sa[ce] = (T)se, sa[co] = (T)so;
                                                sb[ce] = (T)ue, sb[co] = (T)uo;
                                                put_l(ra, ce, se), put_l(ra, co, so);
                                                put_l(ra + 1, ce, ue), put_l(ra + 1, co, uo);
                                        }
                                }
                }
        }
        // ---- zero padding columns n .. na-1
        const int nrows = pose ? 3 : 2 * nlive;
        for (int idx = tid; idx < nrows * (na - n); idx += 256)
        {
                const int rr = r0 + idx / (na - n), c = n + idx % (na - n);
                G[(size_t)rr * NP + c] = (T)0;
                S[(size_t)rr * NP + c] = (T)0;
        }
}

// ------------------------------------------------------------------------------------------------------------------
/// The same G and S, bit for bit, from the LOWER BLOCK TRIANGLE of P alone (round 4).  P is symmetric (large_syrk* store the mirror image of every
/// entry they compute, the predict writes rows and columns 0, 1 alike), so the 64x64 block (I, J), J <= I, serves three outputs:
///     G(I, J)  = P(I, :) H^T restricted to the columns of J                       (rows of the block)
///     G(J, I)  = P(J, :) H^T restricted to the columns of I, with P(J, I) = P(I, J)^T   (columns of the block, read transposed from LDS)
///     S(I, J)  = H(I, :) G(:, J) + R                                               (needs G(I +- 1 row, J) and G(0..2, J), kept in binary64 in LDS)
/// large_build_GS read all of P (8.4 MB per filter at n = 1027) to write G and the lower block triangle of S; this reads 4.4 MB: the kernel is
/// HBM-bound, 16.6 -> 12.4 MB per filter and callback.  H couples landmark column pair (c_odd, c_even) = (3 + 2 j, 4 + 2 j) only to the pose and to
/// itself (ekf.cpp:117-134), so an entry needs its own 2-column (2-row) pair -- pairs straddle the 64-blocks, hence the one-element halo around the
/// block -- and the pose columns of its row.  Every expression is evaluated in the order large_build_GS uses (no contraction): G and S come out
/// bit-identical, which tests/test_gpu_large.py::test_tiled_GS_is_bit_identical checks through the diagnostic read-back.
/// grid (NB (NB + 1) / 2, B) with NB = NP / 64, 256 threads; 40 KB of LDS (the block with its halo, 66 x 67 doubles, and the small vectors): four
/// workgroups per CU.  A thread forms, for its entry (r, c), G(r, c) AND the G entry of the other row of r's pair (the halo rows make that possible at
/// the block's edges), so S(r, c) needs nothing from other threads; the first version kept G(I +- 1, J) in LDS in binary64 (76 KB, two workgroups per CU)
/// and indexed by division: 2.0 ms per 256 filters against 0.81 - 0.94 ms for large_build_GS (profiles/r04_experiments.md section 3).
struct GsTilesLds
{
        static constexpr int HB = LB + 2, PLD = HB + 1; // block + halo; row stride 67 doubles: the transposed reads are conflict-free
        double Pt[HB][PLD];          // P(64 I - 1 + r, 64 J - 1 + c)
        double tI[HB][4], tJ[LB][4]; // pose columns P(a, 0..2) of the rows of I (with halo) and of J
        double cI[HB][2], cJ[LB][2]; // (u, v) of H for the rows of I (with halo: the partner rows) and the columns of J: (h00, h01) on odd, (h10, h11) on even indices
        double P3[3][HB], G3[3][LB], P33[3][4]; // P(0..2, 64 J - 1 + c), G(0..2, 64 J + c), P(0..2, 0..2)
};
template <typename T> __global__ __launch_bounds__(256) void large_build_GS_tiles(DevView d, LargeView<T> lv, const int *skipped)
{
        constexpr int HB = GsTilesLds::HB;
        __shared__ GsTilesLds sh;
        auto &Pt = sh.Pt;
        auto &tI = sh.tI;
        auto &tJ = sh.tJ;
        auto &cI = sh.cI;
        auto &cJ = sh.cJ;
        auto &P3 = sh.P3;
        auto &G3 = sh.G3;
        auto &P33 = sh.P33;
        const int b = blockIdx.y;
        if (skipped[b])
                return;
        const int n = d.n[b], NP = lv.NP;
        const int nb = large_blocks(n);
        const int tl = blockIdx.x;
        const TriIndex blk = tri_index(tl);
        const int I = blk.i, J = blk.j;
        if (I >= nb)
                return;
        const double *P = lv.P + (size_t)b * NP * NP;
        T *G = lv.G + (size_t)b * NP * NP;
        T *S = lv.S + (size_t)b * NP * NP;
        const double *Hc = lv.Hc + (size_t)b * (NP / 2) * 4;
        const double *Y = lv.Y + (size_t)b * NP;
        const aslam_params *const prm = d.prm + b; // (wave-uniform: one filter per workgroup)
        const double r_xy = prm->r_xy, r_yaw = prm->r_yaw, r_range = prm->r_range, r_bearing = prm->r_bearing; // diagonal of R by row class (ekf.cpp:65,278)
        const int tid = threadIdx.x;
        const int r0 = LB * I - 1, c0 = LB * J - 1; // global index of halo row / column 0
        const LargeBorder bd = large_border(n, lv.border); // (as large_build_GS: rows of S21 -> rows n+1 .. n+t of G, the copies of G2 next to them)
        const int n0 = LB * bd.nbc;
        auto save_g2 = [&](int m, int c_, T v) {
                if (bd.t && c_ >= n0 && c_ < n)
                        G[(size_t)(n + 1 + c_ - n0) * NP + n0 + BORDER_SAVE + m] = v;
        };
        typedef double d2 __attribute__((ext_vector_type(2)));
        // ---- stage the block: 16-byte loads of the 64 aligned columns (32 lanes per row, 8 rows per pass), then the two halo columns
        {
                const int q = tid & 31, rr = tid >> 5;
#pragma unroll
                for (int ps = 0; ps < (HB + 7) / 8; ++ps)
                {
                        const int r = 8 * ps + rr, gr = r0 + r;
                        if (r < HB)
                        {
                                d2 v = {0.0, 0.0};
                                if (gr >= 0 && gr < NP)
                                        v = *reinterpret_cast<const d2 *>(P + (size_t)gr * NP + LB * J + 2 * q);
                                Pt[r][1 + 2 * q] = v[0], Pt[r][2 + 2 * q] = v[1];
                        }
                }
                if (tid < 2 * HB)
                {
                        const int r = tid >> 1, hc = (tid & 1) ? HB - 1 : 0;
                        const int gr = r0 + r, gc = c0 + hc;
                        Pt[r][hc] = (gr >= 0 && gr < NP && gc >= 0 && gc < NP) ? P[(size_t)gr * NP + gc] : 0.0;
                }
        }
        if (tid < HB)
        {
                const int gr = r0 + tid, gc = c0 + tid;
#pragma unroll
                for (int k = 0; k < 3; ++k)
                {
                        tI[tid][k] = (gr >= 0 && gr < NP) ? P[(size_t)gr * NP + k] : 0.0;
                        P3[k][tid] = (gc >= 0 && gc < NP) ? P[(size_t)k * NP + gc] : 0.0;
                }
                // H coefficients of row gr (the rows of I and their partners)
                double u = 0.0, v = 0.0;
                if (gr >= 3 && gr < n)
                {
                        const double *h = Hc + 4 * ((gr - 3) >> 1);
                        u = (gr & 1) ? h[0] : h[2], v = (gr & 1) ? h[1] : h[3];
                }
                cI[tid][0] = u, cI[tid][1] = v;
        }
        else if (tid >= 128 && tid < 128 + LB)
        {
                const int c = tid - 128, gc = LB * J + c;
#pragma unroll
                for (int k = 0; k < 3; ++k)
                        tJ[c][k] = P[(size_t)gc * NP + k];
                double u = 0.0, v = 0.0;
                if (gc >= 3 && gc < n)
                {
                        const double *h = Hc + 4 * ((gc - 3) >> 1);
                        u = (gc & 1) ? h[0] : h[2], v = (gc & 1) ? h[1] : h[3];
                }
                cJ[c][0] = u, cJ[c][1] = v;
        }
        else if (tid >= 192 && tid < 201)
                P33[(tid - 192) / 3][(tid - 192) % 3] = P[(size_t)((tid - 192) / 3) * NP + (tid - 192) % 3];
        __syncthreads();
        // G(a, c) of ekf.cpp:301 for a landmark column c (3 <= c < n) from the pose entries t0, t1, t2 of row a and the row's entries at the pair of c
        auto gcol = [](bool even, double u, double v, double t0, double t1, double t2, double p_odd, double p_even) -> double {
                return even ? u * t0 + v * t1 - t2 - u * p_odd - v * p_even : u * t0 + v * t1 - u * p_odd - v * p_even;
        };
        const int c = tid & (LB - 1), rq = tid >> 6; // this thread's column of the block, its row inside a pass of four
        const int gc = LB * J + c;
        const bool ceven = !(gc & 1);
        const int co = ceven ? c : c + 1; // halo index of the odd member of column gc's pair (the even one: co + 1)
        const double uJ = cJ[c][0], vJ = cJ[c][1];
        // ---- the pose rows of G over the columns of J (binary64; for S)
        if (rq < 3)
        {
                const int m = rq;
                G3[m][c] = gc >= n ? 0.0 : gc < 3 ? P33[m][gc] : gcol(ceven, uJ, vJ, P33[m][0], P33[m][1], P33[m][2], P3[m][co], P3[m][co + 1]);
        }
        __syncthreads();
        // G of halo row index r (global row r0 + r) at this thread's column, binary64
        auto g_at = [&](int r) -> double {
                const int ga = r0 + r;
                if (ga < 0 || ga > n || gc >= n)
                        return 0.0; // padding (rows beyond n, columns from n on)
                if (ga == n)
                        return Y[gc]; // row n carries Y^T through the solve
                if (gc < 3)
                        return Pt[r][c + 1];
                return gcol(ceven, uJ, vJ, tI[r][0], tI[r][1], tI[r][2], Pt[r][co], Pt[r][co + 1]);
        };
        const double g30 = G3[0][c], g31 = G3[1][c], g32 = G3[2][c];
        // ---- G(I, J) and S(I, J) = H(I, :) G(:, J) + R: entry (r, c) with the G entry of the other row of r's pair
#pragma unroll 4
        for (int ps = 0; ps < LB / 4; ++ps)
        {
                const int r = 4 * ps + rq, gr = LB * I + r; // block row r = halo row r + 1
                const double g = g_at(r + 1);
                if (!border_spare(bd, n, gr, gc))
                        G[(size_t)gr * NP + gc] = (T)g;
                if (gr == n)
                        save_g2(3, gc, (T)g);
                double sv;
                if (gr >= n)
                        sv = (gr == gc) ? 1.0 : 0.0; // padding rows: identity
                else if (gc >= n)
                        sv = 0.0;
                else if (gr < 3)
                        sv = g + (gr == gc ? (gr < 2 ? r_xy : r_yaw) : 0.0);
                else
                {
                        const bool even = !(gr & 1);                    // the bearing row of its landmark
                        const double gp = g_at(even ? r : r + 2);       // the other row of the pair: gr - 1 / gr + 1
                        const double go_ = even ? gp : g, ge_ = even ? g : gp;
                        const double ha = cI[r + 1][0], hb = cI[r + 1][1];
                        double v = ha * g30 + hb * g31;
                        if (even)
                                v -= g32;
                        sv = v - ha * go_ - hb * ge_;
                        if (gr == gc)
                                sv += even ? r_bearing : r_range;
                }
                S[(size_t)gr * NP + gc] = (T)sv;
                if (bd.t && gr >= n0 && gr < n && gc < n0)
                        G[(size_t)(gr + bd.t + 1) * NP + gc] = (T)sv;
        }
        // ---- G(J, I): row cr of J, column a of I, from the block read transposed
        if (I != J)
        {
                const int a = c, gcolx = LB * I + a; // this thread's output column (a landmark column: gcolx >= 64)
                const bool even = !(gcolx & 1);
                const int ao = even ? a : a + 1; // halo ROW index of the odd member of column gcolx's pair
                const double uI = cI[a + 1][0], vI = cI[a + 1][1];
#pragma unroll 4
                for (int ps = 0; ps < LB / 4; ++ps)
                {
                        const int cr = 4 * ps + rq, grow = LB * J + cr;
                        double g;
                        if (grow > n || gcolx >= n)
                                g = 0.0;
                        else if (grow == n)
                                g = Y[gcolx];
                        else
                                g = gcol(even, uI, vI, tJ[cr][0], tJ[cr][1], tJ[cr][2], Pt[ao][cr + 1], Pt[ao + 1][cr + 1]);
                        G[(size_t)grow * NP + gcolx] = (T)g;
                        if (grow < 3)
                                save_g2(grow, gcolx, (T)g);
                }
        }
}

// ------------------------------------------------------------------------------------------------------------------
// (the diagonal blocks: large_potrf_inv_tiles in ekf_large_chol.h)

/// virtual stacked matrix M = [S; G] (2*na rows): row pointer of virtual row vr
template <typename T> __device__ __forceinline__ T *stacked_row(const LargeView<T> &lv, int b, int na, int vr)
{
        const size_t NP = lv.NP;
        return (vr < na) ? lv.S + ((size_t)b * NP + vr) * NP : lv.G + ((size_t)b * NP + (vr - na)) * NP;
}

/// Block column k0 of the stacked matrix M = [S; G; Y^T], for every 64-row block rt below the diagonal block:
///   C  = M(rt, k0) - sum_{k < k0} M(rt, k) L(k0, k)^T      left-looking update, K = 64 k0, MFMA
///   X  = C L(k0,k0)^-T = C Linv^T                           the panel "triangular solve" as a 64-deep MFMA product
///   S(rt, rt) -= X X^T  (blocks of S only)                  the diagonal blocks are kept up to date right-looking, so
///                                                           large_potrf_inv_tiles finds block k0+1 ready when this kernel ends
/// One read-modify-write of every tile per factorisation.  A workgroup takes TWO consecutive 64-row blocks (a 128x64 tile:
/// the block row of L is staged once for both, 128 MFMAs per wave between barriers); the two halves are addressed
/// independently because the pair may straddle the S / G boundary.  4 waves, wave w = rows 32w..32w+31 of the tile as
/// 2x4 MFMA 16x16 tiles.  The next K slab is fetched into registers while the current one is multiplied.
/// grid (ceil((2 nb - k0 - 1) / 2), 1, B) -- or (ceil((nb - k0 - 1) / 2), 1, B) with s_only: the blocks of S alone --, 256 threads.
template <typename T>
__global__ __launch_bounds__(256) void large_update_panel(DevView d, LargeView<T> lv, int k0, int s_only, const int *skipped)
{
        typedef Mfma<T> MM;
        constexpr int KC = (sizeof(T) == 4) ? 64 : 32; // columns staged per round = 256 bytes of a row
        constexpr int LD = KC + (sizeof(T) == 4 ? 8 : 4); // fp32: 18 sixteen-byte slots per row -> conflict-free ds_read_b128 operand reads
        typedef T vec_t __attribute__((ext_vector_type(16 / sizeof(T))));
        constexpr int VW = 16 / sizeof(T);
        static_assert(KC / VW == 16, "16 lanes per staged row");
        __shared__ __attribute__((aligned(16))) T As[2 * LB][LD];
        __shared__ __attribute__((aligned(16))) T Bs[LB][LD];
        const int b = blockIdx.z;
        if (skipped[b])
                return;
        const int n = d.n[b], NP = lv.NP;
        const int nb = large_blocks(n, lv.xrows), na = nb * LB;
        const int rt0 = k0 + 1 + 2 * blockIdx.x; // first virtual 64-row block: S rows below the diagonal block, then all of G
        const int vlim = s_only ? nb : 2 * nb;    // s_only: the rows of G are solved by large_trsm_pipe instead
        if (k0 >= nb || rt0 >= vlim)
                return;
        const bool two = rt0 + 1 < vlim; // the last workgroup may have a single block
        const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4;
        const int half = wave >> 1;            // which 64-row block this wave's rows belong to
        const int rt = rt0 + half;             // its virtual block index
        const bool live = (half == 0) || two;  // wave-uniform
        const int wr = 32 * wave;              // first tile row of the wave
        const T *Brow = lv.S + ((size_t)b * NP + (size_t)k0 * LB) * NP; // block row k0 of L
        typename MM::acc_t acc[2][4];
        auto clear = [&]() {
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int v = 0; v < 4; ++v)
                                acc[u][v] = MM::zero();
        };
        clear();
        // acc += As(rows of this wave) * Bsrc(rows vb .. vb+63)^T over one staged slab
        auto multiply = [&](const T(*Bsrc)[LD], int vb) {
                if constexpr (sizeof(T) == 4)
                {
                        // one 16-byte LDS read per operand row feeds four MFMA steps: lane (li, lg) holds k = 16 c + 4 lg + r for
                        // step r -- a permuted walk over the contraction index, the same for both operands
#pragma unroll
                        for (int c = 0; c < KC / 16; ++c)
                        {
                                f4 av[2], bv[4];
#pragma unroll
                                for (int u = 0; u < 2; ++u)
                                        av[u] = *reinterpret_cast<const f4 *>(&As[wr + 16 * u + li][16 * c + 4 * lg]);
#pragma unroll
                                for (int v = 0; v < 4; ++v)
                                        bv[v] = *reinterpret_cast<const f4 *>(&Bsrc[vb + 16 * v + li][16 * c + 4 * lg]);
#pragma unroll
                                for (int r = 0; r < 4; ++r)
#pragma unroll
                                        for (int u = 0; u < 2; ++u)
#pragma unroll
                                                for (int v = 0; v < 4; ++v)
                                                        acc[u][v] = MM::mma(av[u][r], bv[v][r], acc[u][v]);
                        }
                        return;
                }
#pragma unroll
                for (int s = 0; s < KC / 4; ++s)
                {
                        T av[2], bv[4];
#pragma unroll
                        for (int u = 0; u < 2; ++u)
                                av[u] = As[wr + 16 * u + li][lg + 4 * s];
#pragma unroll
                        for (int v = 0; v < 4; ++v)
                                bv[v] = Bsrc[vb + 16 * v + li][lg + 4 * s];
#pragma unroll
                        for (int u = 0; u < 2; ++u)
#pragma unroll
                                for (int v = 0; v < 4; ++v)
                                        acc[u][v] = MM::mma(av[u], bv[v], acc[u][v]);
                }
        };
        // ---- left-looking update.  Staging: 16 lanes cover the 256-byte row segment of a slab with 16-byte loads.
        const int lrow = tid >> 4, lc0 = (tid & 15) * VW;
        const T *Ap[8], *Bp[4];
#pragma unroll
        for (int q = 0; q < 8; ++q)
        {
                const int r = lrow + 16 * q;                           // tile row 0..127
                const int vr = (rt0 + ((r >> 6) & (two ? 1 : 0))) * LB + (r & 63); // a missing second block re-reads the first
                Ap[q] = stacked_row(lv, b, na, vr) + lc0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
                Bp[q] = Brow + (size_t)(lrow + 16 * q) * NP + lc0;
        vec_t ta[8], tb[4];
        auto fetch = [&](int kc) {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                        ta[q] = *reinterpret_cast<const vec_t *>(Ap[q] + kc);
#pragma unroll
                for (int q = 0; q < 4; ++q)
                        tb[q] = *reinterpret_cast<const vec_t *>(Bp[q] + kc);
        };
        const int Kend = k0 * LB;
        if (Kend > 0)
                fetch(0);
        for (int kc = 0; kc < Kend; kc += KC)
        {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                        *reinterpret_cast<vec_t *>(&As[lrow + 16 * q][lc0]) = ta[q];
#pragma unroll
                for (int q = 0; q < 4; ++q)
                        *reinterpret_cast<vec_t *>(&Bs[lrow + 16 * q][lc0]) = tb[q];
                __syncthreads();
                if (kc + KC < Kend)
                        fetch(kc + KC);
                multiply(Bs, 0);
                __syncthreads();
        }
        // ---- C = M(rt, k0) - acc (kept in registers in the accumulator layout)
        T *Mrow = stacked_row(lv, b, na, (live ? rt : rt0) * LB) + (size_t)(wr & 63) * NP; // first row of this wave
        T *Ctile = Mrow + (size_t)k0 * LB;
        typename MM::acc_t cr[2][4];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v)
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                                cr[u][v][r] = Ctile[(size_t)(16 * u + MM::row(lane, r)) * NP + 16 * v + li] - acc[u][v][r];
        clear();
        // ---- X = C Linv^T, K = 64 in slabs of KC: stage C (from registers) and Linv (row c of Linv = column c of the product)
        const T *Li = lv.Linv + ((size_t)b * LARGE_NB_MAX + k0) * LB * LB;
        auto stage_regs = [&](const typename MM::acc_t(&src)[2][4], int kh) {
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int v = 0; v < 4; ++v)
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                {
                                        const int col = 16 * v + li;
                                        if (col / KC == kh)
                                                As[wr + 16 * u + MM::row(lane, r)][col % KC] = src[u][v][r];
                                }
        };
        for (int kh = 0; kh < LB / KC; ++kh)
        {
                stage_regs(cr, kh);
                for (int idx = tid; idx < LB * KC; idx += 256)
                        Bs[idx / KC][idx % KC] = Li[(idx / KC) * LB + kh * KC + (idx % KC)];
                __syncthreads();
                multiply(Bs, 0);
                __syncthreads();
        }
        if (live)
        {
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int v = 0; v < 4; ++v)
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                        Ctile[(size_t)(16 * u + MM::row(lane, r)) * NP + 16 * v + li] = acc[u][v][r];
        }
        if (rt0 >= nb)
                return; // only blocks of G in this workgroup: done (workgroup-uniform)
        // ---- S(rt, rt) -= X X^T for the blocks of S: this wave's 32 rows of X against the 64 rows of its own block
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                        cr[u][v] = acc[u][v];
        clear();
        for (int kh = 0; kh < LB / KC; ++kh)
        {
                stage_regs(cr, kh);
                __syncthreads();
                multiply(As, 64 * half);
                __syncthreads();
        }
        if (live && rt < nb)
        {
                T *Dtile = Mrow + (size_t)rt * LB;
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                        for (int v = 0; v < 4; ++v)
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                        Dtile[(size_t)(16 * u + MM::row(lane, r)) * NP + 16 * v + li] -= acc[u][v][r];
        }
}

/// P -= V V^T (ekf.cpp:311 in the A-form, V = G after the panel solves) on 128x128 tiles: the kernel is bound by the
/// operand traffic out of L2 (every row tile of V is read once per tile column), so the tile is as large as the
/// accumulators allow: 4 waves, each a 64x64 quadrant = 4x4 MFMA 16x16 tiles (tile128_f64_product above, K = na).  Lower
/// tiles only, mirrored on store.
/// grid (8 * lower tiles * ceil(B/8)), 256 threads.  (A template only because this header is part of two translation units: T is double.)
template <typename T>
__global__ __launch_bounds__(256) void large_syrk(DevView d, LargeView<T> lv, int nfilters, const int *skipped)
{
        static_assert(sizeof(T) == 8, "binary32 products go through large_syrk_bf16x3");
        typedef Mfma<double> MM;
        constexpr int TB = T128;
        __shared__ double As[TB][T128_LD];
        __shared__ double Bs[TB][T128_LD];
        // XCD-aware mapping: consecutive workgroup ids go round-robin to the 8 XCDs, each with its own L2.  All lower tiles of
        // one filter are given ids that are equal mod 8, so the ~45 workgroups that share a filter's V run on one XCD and its
        // row tiles are fetched into that L2 once instead of into all eight.
        const int ntile = (lv.NP + TB - 1) / TB, nlow = ntile * (ntile + 1) / 2;
        const int slot = blockIdx.x >> 3;
        const int b = (slot / nlow) * 8 + (blockIdx.x & 7);
        if (b >= nfilters || skipped[b])
                return;
        const int n = d.n[b], NP = lv.NP;
        const int na = large_blocks(n, lv.xrows) * LB;
        const int tl = slot % nlow;
        const TriIndex tile = tri_index(tl);
        const int rt = tile.i, jt = tile.j;
        if (rt * TB >= na)
                return;
        const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15;
        const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
        const double *G = lv.G + (size_t)b * NP * NP;
        double *P = lv.P + (size_t)b * NP * NP;
        // 16-row / 16-column subtiles of this wave's quadrant that hold at least one of the n valid rows / columns (n = 3 mod 128
        // at full size: the last tile row is almost empty), and the upper quadrant of a diagonal tile is the mirror image of
        // its lower one: neither is multiplied
        const bool idle = (rt == jt && wc > wr);
        const int nu = idle ? 0 : __builtin_amdgcn_readfirstlane(max(0, min(4, (n - (rt * TB + wr) + 15) >> 4)));
        const int nv = idle ? 0 : __builtin_amdgcn_readfirstlane(max(0, min(4, (n - (jt * TB + wc) + 15) >> 4)));
        typedef double d2 __attribute__((ext_vector_type(2)));
        MM::acc_t acc[4][4];
        tile128_f64_product(As, Bs, G, G, NP, na, rt, jt, na, nu, nv, [](double *dst, const d2 &t, int) { *reinterpret_cast<d2 *>(dst) = t; }, acc);
        if (idle)
                return;
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
                                if (row < n && col < n) // keep P's padding clean (row n of G is Y^T, not V)
                                        P[(size_t)row * NP + col] -= acc[u][v][r];
                        }
                        if ((jt < rt || wc < wr) && col < n)
                        {
                                // mirror into the upper triangle
#pragma unroll
                                for (int r = 0; r < 4; ++r)
                                {
                                        const int row = rt * TB + wr + 16 * u + MM::row(lane, r);
                                        if (row < n)
                                                P[(size_t)col * NP + row] -= acc[u][v][r];
                                }
                        }
                }
}

#ifndef ASLAM_XU_ROWS
#define ASLAM_XU_ROWS 8
#endif
constexpr int XU_ROWS = ASLAM_XU_ROWS; // (rows per wave of large_x_update_rows; 4 and 16 measured in round 4: profiles/r04_experiments.md)
#ifndef ASLAM_XU_WAVES
#define ASLAM_XU_WAVES 8
#endif
constexpr int XU_WAVES = ASLAM_XU_WAVES;         // waves per workgroup of large_x_update_rows (4, 8 and 16 measured: profiles/xupdate.md)
constexpr int XU_THREADS = 64 * XU_WAVES;
constexpr int XU_WG_ROWS = XU_WAVES * XU_ROWS;   // rows of V per workgroup
typedef double xu_d2 __attribute__((ext_vector_type(2)));
constexpr int XU_STAGE_THREADS = 256;            // waves 0 .. 3 stage the shared rows of a border and sum its dot products, whatever XU_WAVES is
static_assert(XU_WAVES >= 4 && XU_WAVES <= 16, "large_x_update_rows: 4 staging waves at least, 1024 threads at most");

/// P -= V V^T with the binary32 products formed on the BF16 matrix pipe ("bf16x3"): every float is the exact sum of three bf16 pieces of
/// eight mantissa bits (a = a1 + a2 + a3), and  a b ~= a1 b1 + (a1 b2 + a2 b1) + (a1 b3 + a2 b2 + a3 b1):  six v_mfma_f32_16x16x32_bf16
/// (16x16x32 per instruction, fp32 accumulation, bf16 x bf16 products exact) do the work of eight v_mfma_f32_16x16x4_f32 at twice
/// the rate, and the dropped terms (2^-24 |a b| and below) are smaller than the rounding of a binary32 product chain
/// (tools/ubench/mfma_bf16x3.hip: 6.3e-8 of sum |a b| against 1.5e-7 for an fp32 FMA chain; 294 against 149 T fp32-equivalent FLOP/s).
/// P is stored in binary64 (the update V V^T is small against P in steady state, so rounding the UPDATE to binary32 and accumulating it into
/// an fp64 P costs eps32 |dP| per callback instead of eps32 |P|: tools/fp32_drift_model.py), V in binary32.  Same 128x128 tiling and tile ->
/// workgroup map as large_syrk (4 waves x 4x4 MFMA tiles, lower tiles only, a filter's tiles on one XCD); the K loop stops at the filter's
/// size n (columns n .. of V are zero); the lower tile is read-modify-written in fp64 (16 bytes per lane and access: the products are formed
/// as B x A^T so that a lane holds four consecutive columns of a row) and its NEW value is stored, transposed, into the upper triangle -- no
/// read of the upper triangle, and P stays exactly symmetric.  The slab of V is split into its three bf16 planes by the VALU on the way into LDS (8 bytes per thread, row and plane; unpadded 64-byte rows with XOR-swizzled k-groups),
/// the operand of an MFMA is ONE 16-byte read (row l & 15, k = 8 (l >> 4) .. + 7).
///
/// The X update (large_x_update_rows: X += V q, the diagonal and the pose columns of V V^T in binary64) runs on the same stream: IN FRONT OF this kernel in
/// the default chain (LargePlan::border: it completes V there -- the columns V2 of a filter's border, which this kernel's K loop then reads like any other
/// column), behind it otherwise.  This kernel
/// never touches the entries of P the other one writes (pose columns, pose rows, diagonal), so the order is free and the two COULD run side by side -- round 4 measured both
/// ways (the X update's workgroups inside this launch: 2436 us against 1997 + 324 per 256 filters; on a side stream: 31.7 k against 36.4 k filter-steps/s)
/// and both lose: at this kernel's register footprint the latency-bound X-update workgroups take slots while the matrix pipes idle, and next to it they
/// fight it for L2 (profiles/r04_experiments.md section 1).
///
/// What the chain does around this kernel, then: V arrives in binary32 (the TRSM's output; with a border its last t columns from the X update) and is split
/// by the VALU on the way into LDS -- no kernel of the library writes bf16 planes of V -- and the X update is a launch of its own: launch 5 of the default
/// chain, in front of this one; launch 6, behind it, without the border.
/// RUNNING = false is the default chain's kernel.  RUNNING = true (ASLAM_SYRK_RUNNING=1) is round 2's accumulation order, kept for comparison: every tile
/// takes the general path and the six products of a slab are added straight into the running sum (profiles/r03_experiments.md).
///
/// THE TILE MAP has one exception (large_syrk_tail above; RUNNING = false with LargeView::syrk_tail): a last tile row rl that holds no more than 16 state
/// rows -- the benchmark's rows 1024 .. 1026 -- has no tiles of its own left of the corner.  Tiles (rl, jt), jt < rl, return at once; in diagonal tile
/// (jt, jt) the wave of the upper quadrant, which otherwise only helps to stage, forms those rows x the 128 columns of tile jt from the Bs of its
/// workgroup (`tailw` below) and stores them with the epilogue's arithmetic.  Bit-identical to the tile row (tests/test_gpu_large_syrk_tail.py;
/// profiles/syrk_tail.md).
template <bool RUNNING>
__global__ __launch_bounds__(256, 3) void large_syrk_bf16x3(DevView d, LargeView<float> lv, int nfilters, const int *skipped)
{
        constexpr int TB = 128, KC = 32;
        constexpr int LDB = KC; // bf16 per LDS row: 64 bytes, unpadded; the four 16-byte k-groups of a row are XOR-swizzled with (row & 15) >> 2, which
                                // makes the 16-byte operand reads of 16 rows conflict-free (three workgroups per CU need the 48 KB this leaves)
        typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
        typedef unsigned u4 __attribute__((ext_vector_type(4)));
        typedef unsigned u2 __attribute__((ext_vector_type(2)));
        __shared__ __attribute__((aligned(16))) unsigned short As[3][TB * LDB];
        __shared__ __attribute__((aligned(16))) unsigned short Bs[3][TB * LDB];
        const int ntile = (lv.NP + TB - 1) / TB, nlow = ntile * (ntile + 1) / 2;
        const int slot = blockIdx.x >> 3;
        const int b = (slot / nlow) * 8 + (blockIdx.x & 7);
        if (b >= nfilters || skipped[b])
                return;
        const int n = d.n[b], NP = lv.NP;
        const int na = large_blocks(n) * LB;
        const int tl = slot % nlow;
        int rt = (int)((sqrtf(8.0f * (float)tl + 1.0f) - 1.0f) * 0.5f); // (tri_index() written out: this kernel's register allocation changes with the call)
        while ((rt + 1) * (rt + 2) / 2 <= tl)
                ++rt;
        while (rt * (rt + 1) / 2 > tl)
                --rt;
        const int jt = tl - rt * (rt + 1) / 2;
        if (rt * TB >= n)
                return;
        const SyrkTail tail = large_syrk_tail(n, !RUNNING && lv.syrk_tail);
        if (tail.rows && rt == tail.rl && jt < rt)
                return; // (formed by the idle waves of the diagonal tiles (jt, jt): tailw below)
        const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15, lg = lane >> 4;
        const int wr = (wave >> 1) * 64, wc = (wave & 1) * 64;
        const float *G = lv.G + (size_t)b * NP * NP;
        double *P = lv.P + (size_t)b * NP * NP;
        // staging: 8 lanes cover the 32 columns of a slab row with 16-byte loads; 32 rows per pass
        constexpr int LPR = KC / 4, RPP = 256 / LPR, NPASS = TB / RPP;
        const int lrow = tid / LPR, lc0 = (tid % LPR) * 4;
        const float *Ap[NPASS], *Bp[NPASS];
#pragma unroll
        for (int q = 0; q < NPASS; ++q)
        {
                Ap[q] = G + (size_t)min(rt * TB + lrow + RPP * q, na - 1) * NP + lc0;
                Bp[q] = G + (size_t)min(jt * TB + lrow + RPP * q, na - 1) * NP + lc0;
        }
        f4 acc[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                        acc[u][v] = (f4){0.f, 0.f, 0.f, 0.f};
        f4 ta[NPASS], tb[NPASS];
        auto fetch = [&](int kc) {
#pragma unroll
                for (int q = 0; q < NPASS; ++q)
                {
                        ta[q] = *reinterpret_cast<const f4 *>(Ap[q] + kc);
                        tb[q] = *reinterpret_cast<const f4 *>(Bp[q] + kc);
                }
        };
        // four floats -> their three bf16 planes: x = h + m + l up to 2^-25 |x|.  Round to nearest at every level (v_cvt_pk_bf16_f32): with
        // truncated pieces, which all carry the sign of x, the dropped terms a2 b3 + a3 b2 have the sign of the product, V V^T comes out
        // systematically small and the covariance error grew 1.5x faster than with binary32 MFMAs; rounded, it is 4x smaller than theirs.
        auto stash = [&](unsigned short (&S)[3][TB * LDB], int off, const f4 &x) {
                u2 pk[3];
                split_bf16x3(x, pk[0], pk[1], pk[2]);
#pragma unroll
                for (int p = 0; p < 3; ++p)
                        *reinterpret_cast<u2 *>(&S[p][off]) = pk[p];
        };
        const bool idle = (rt == jt && wc > wr); // upper quadrant of a diagonal tile: the mirror image of its lower one
        // A diagonal quadrant holds (I, J) and (J, I).  With binary32 MFMA products the two sums are bit-identical; here the six partial
        // products of the pair enter them in different orders, so only J <= I is computed and the mirror image is stored from it, element
        // by element inside the 16x16 tiles on the diagonal: P stays exactly symmetric.
        const bool diagq = (rt == jt && wc == wr);
        const int nu = idle ? 0 : __builtin_amdgcn_readfirstlane(max(0, min(4, (n - (rt * TB + wr) + 15) >> 4)));
        const int nv = idle ? 0 : __builtin_amdgcn_readfirstlane(max(0, min(4, (n - (jt * TB + wc) + 15) >> 4)));
        const bool full = !RUNNING && nu == 4 && nv == 4 && !diagq; // wave-uniform: an interior 64x64 quadrant
        const int kend = min(na, (n + KC - 1) / KC * KC); // columns n .. na-1 of V are zero (G = P H^T is zero there and L is the identity)
        const int a_off = (wr + li) * LDB + 8 * (lg ^ (li >> 2)), b_off = (wc + li) * LDB + 8 * (lg ^ (li >> 2)); // swizzled k-group
        const int s_off = lrow * LDB + 8 * ((lc0 >> 3) ^ ((lrow & 15) >> 2)) + (lc0 & 4); // this thread's 8 bytes of a staged row (rows lrow + 32 q: same row & 15)
        // The tail (large_syrk_tail): the idle wave of diagonal tile (jt, jt), jt < rl, forms rows 128 rl .. n-1 x the 128 columns of tile jt.  Bs holds the B
        // operands (what tile (rl, jt) would stage again: column rows 16 v + li, v = 0 .. 7); the A operand, V(128 rl + li, kc + 8 lg .. + 7) for lane (li, lg),
        // comes straight from memory, two 16-byte loads a slab ahead, and is split as stash() splits: no LDS, no barrier.  The eight accumulators are
        // acc[0][0..3], acc[1][0..3].  The wave's other accumulators are dead, and what the path carries from slab to slab lives in them -- acc[3][0..1] the
        // prefetched floats, acc[3][2][0] the bits of the row's byte offset in G -- so that the kernel needs no register more than without the path.
        const bool tailw = idle && tail.rows && rt < tail.rl; // (wave-uniform, like idle; left to the compiler as a divergent condition: made scalar, hipcc spills accumulators inside the K loop)
        f4 &tp0 = acc[3][0], &tp1 = acc[3][1];
        if (tailw) // (rows past the tail: clamped like the staging; MFMA rows do not mix)
                acc[3][2][0] = __builtin_bit_cast(float, 4u * (unsigned)(min(tail.rl * TB + li, na - 1) * NP + 8 * lg));
        auto tail_fetch = [&](int kc) {
                const char *row = reinterpret_cast<const char *>(G + kc) + __builtin_bit_cast(unsigned, acc[3][2][0]);
                tp0 = *reinterpret_cast<const f4 *>(row);
                tp1 = *reinterpret_cast<const f4 *>(row + 16);
        };
        fetch(0);
        if (tailw)
                tail_fetch(0);
        for (int kc = 0; kc < kend; kc += KC)
        {
#pragma unroll
                for (int q = 0; q < NPASS; ++q)
                {
                        stash(As, s_off + RPP * q * LDB, ta[q]);
                        stash(Bs, s_off + RPP * q * LDB, tb[q]);
                }
                __syncthreads();
                if (kc + KC < kend)
                        fetch(kc + KC);
                // two column tiles of the wave's 64x64 at a time: 24 operand registers instead of 48 (three workgroups per CU).
                // B x A^T (see the epilogue), small terms first.  The six products of a slab are summed in a ZERO-INITIALISED temporary and
                // added to the running sum by the VALU once per slab: an MFMA that adds small products to a large accumulator truncates them
                // (four sequential additions per instruction, each losing the addend's low bits: tools/ubench/mfma_rounding.hip), which over
                // 198 MFMAs per element left the DIAGONAL of V V^T (sums of squares) 5.8e-7 too small -- a bias, so the covariance error grew
                // linearly with the callbacks.  With the temporary the bias is 8e-10 and the mean error 9x smaller
                // (tools/ubench/syrk_accum.hip).  Interior tiles (the bulk) take the branch-free path, where the addition of a pair of
                // temporaries is issued behind the MFMAs of the NEXT pair.
#define ASLAM_MM(t, bb, aa, c) t = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, bb), __builtin_bit_cast(bf8, aa), c, 0, 0, 0)
                if (full)
                {
#pragma unroll
                        for (int vh = 0; vh < 4; vh += 2)
                        {
                                u4 bq[2][3];
#pragma unroll
                                for (int v = 0; v < 2; ++v)
#pragma unroll
                                        for (int p = 0; p < 3; ++p)
                                                bq[v][p] = *reinterpret_cast<const u4 *>(&Bs[p][b_off + 16 * (vh + v) * LDB]);
                                f4 pa = {0.f, 0.f, 0.f, 0.f}, pb = {0.f, 0.f, 0.f, 0.f}; // the previous row tile's pair, not yet added
#pragma unroll
                                for (int u = 0; u < 4; ++u)
                                {
                                        u4 ap[3];
#pragma unroll
                                        for (int p = 0; p < 3; ++p)
                                                ap[p] = *reinterpret_cast<const u4 *>(&As[p][a_off + 16 * u * LDB]);
                                        f4 ta, tb;
                                        ASLAM_MM(ta, bq[0][0], ap[2], ((f4){0.f, 0.f, 0.f, 0.f}));
                                        ASLAM_MM(tb, bq[1][0], ap[2], ((f4){0.f, 0.f, 0.f, 0.f}));
                                        ASLAM_MM(ta, bq[0][1], ap[1], ta);
                                        ASLAM_MM(tb, bq[1][1], ap[1], tb);
                                        ASLAM_MM(ta, bq[0][2], ap[0], ta);
                                        ASLAM_MM(tb, bq[1][2], ap[0], tb);
                                        if (u > 0)
                                        {
                                                acc[u - 1][vh] += pa;
                                                acc[u - 1][vh + 1] += pb;
                                        }
                                        ASLAM_MM(ta, bq[0][0], ap[1], ta);
                                        ASLAM_MM(tb, bq[1][0], ap[1], tb);
                                        ASLAM_MM(ta, bq[0][1], ap[0], ta);
                                        ASLAM_MM(tb, bq[1][1], ap[0], tb);
                                        ASLAM_MM(ta, bq[0][0], ap[0], ta);
                                        ASLAM_MM(tb, bq[1][0], ap[0], tb);
                                        pa = ta, pb = tb;
                                        __builtin_amdgcn_sched_barrier(0); // (left alone hipcc hoists every operand read of the slab to its top and spills accumulators)
                                }
                                acc[3][vh] += pa;
                                acc[3][vh + 1] += pb;
                        }
                }
                else if (tailw)
                {
                        // the products of tile (rl, jt), wave by wave: tail rows as the second operand, column rows as the first, the six MFMAs in the
                        // order of the general path below, a zero-initialised temporary per column tile and slab
                        u2x h0, m0, l0, h1, m1, l1;
                        split_bf16x3(tp0, h0, m0, l0);
                        split_bf16x3(tp1, h1, m1, l1);
                        const u4 ap[3] = {(u4){h0[0], h0[1], h1[0], h1[1]}, (u4){m0[0], m0[1], m1[0], m1[1]}, (u4){l0[0], l0[1], l1[0], l1[1]}};
                        if (kc + KC < kend)
                                tail_fetch(kc + KC);
#pragma unroll
                        for (int v = 0; v < 8; ++v)
                        {
                                u4 bq[3];
#pragma unroll
                                for (int p = 0; p < 3; ++p)
                                        bq[p] = *reinterpret_cast<const u4 *>(&Bs[p][b_off + (16 * v - wc) * LDB]);
                                f4 tmp;
                                ASLAM_MM(tmp, bq[0], ap[2], ((f4){0.f, 0.f, 0.f, 0.f}));
                                ASLAM_MM(tmp, bq[1], ap[1], tmp);
                                ASLAM_MM(tmp, bq[2], ap[0], tmp);
                                ASLAM_MM(tmp, bq[0], ap[1], tmp);
                                ASLAM_MM(tmp, bq[1], ap[0], tmp);
                                ASLAM_MM(tmp, bq[0], ap[0], tmp);
                                acc[v >> 2][v & 3] += tmp;
                                __builtin_amdgcn_sched_barrier(0); // (as in the interior path: keep the operand reads of a column tile next to its MFMAs)
                        }
                }
                else
                {
#pragma unroll
                        for (int vh = 0; vh < 4; vh += 2)
                        {
                                u4 bq[2][3];
#pragma unroll
                                for (int v = 0; v < 2; ++v)
#pragma unroll
                                        for (int p = 0; p < 3; ++p)
                                                bq[v][p] = *reinterpret_cast<const u4 *>(&Bs[p][b_off + 16 * (vh + v) * LDB]);
#pragma unroll
                                for (int u = 0; u < 4; ++u)
                                        if (u < nu)
                                        {
                                                u4 ap[3];
#pragma unroll
                                                for (int p = 0; p < 3; ++p)
                                                        ap[p] = *reinterpret_cast<const u4 *>(&As[p][a_off + 16 * u * LDB]);
#pragma unroll
                                                for (int v = 0; v < 2; ++v)
                                                        if (vh + v < nv && !(diagq && vh + v > u))
                                                        {
                                                                f4 tmp;
                                                                if constexpr (RUNNING) // round 2's running accumulator
                                                                {
                                                                        ASLAM_MM(tmp, bq[v][0], ap[2], acc[u][vh + v]);
                                                                        ASLAM_MM(tmp, bq[v][1], ap[1], tmp);
                                                                        ASLAM_MM(tmp, bq[v][2], ap[0], tmp);
                                                                        ASLAM_MM(tmp, bq[v][0], ap[1], tmp);
                                                                        ASLAM_MM(tmp, bq[v][1], ap[0], tmp);
                                                                        ASLAM_MM(tmp, bq[v][0], ap[0], tmp);
                                                                        acc[u][vh + v] = tmp;
                                                                        continue;
                                                                }
                                                                ASLAM_MM(tmp, bq[v][0], ap[2], ((f4){0.f, 0.f, 0.f, 0.f}));
                                                                ASLAM_MM(tmp, bq[v][1], ap[1], tmp);
                                                                ASLAM_MM(tmp, bq[v][2], ap[0], tmp);
                                                                ASLAM_MM(tmp, bq[v][0], ap[1], tmp);
                                                                ASLAM_MM(tmp, bq[v][1], ap[0], tmp);
                                                                ASLAM_MM(tmp, bq[v][0], ap[0], tmp);
                                                                acc[u][vh + v] += tmp;
                                                        }
                                        }
                        }
                }
#undef ASLAM_MM
                __syncthreads();
        }
        if (idle && !tailw)
                return;
        const bool mirror = (jt < rt || wc < wr);
        // The DIAGONAL of V V^T and its three POSE columns (and their mirror image, the pose rows) are formed with binary64 accumulation by the X-update
        // kernel (large_x_update_rows) and are NOT TOUCHED here -- not even read and stored back (a store-back of an old value would tie the order of the two
        // kernels).  Pose columns 0..2 = registers 0..2 of lane group 0 in the first
        // column tile of tile column 0 (posecols below: only its column 3 is updated, by 8-byte accesses); the diagonal is skipped element-wise.
        // The K loop multiplies B x A^T (operands swapped), so a lane's four registers are four consecutive COLUMNS of one row of the
        // lower tile: 32 contiguous bytes, two 16-byte loads and stores per 16x16 tile; the mirror image is the strided side (four
        // 8-byte stores).  With A x B^T (four consecutive rows per lane: four 8-byte loads + stores, 16-byte mirror stores) the
        // epilogue cost 0.66 ms per 256 filters against 0.33 ms (trsm_bench).
        typedef double d2 __attribute__((ext_vector_type(2)));
        // a lane's register quad: P(row, col0 .. col0 + 3) -= a, the new values also to the mirror positions
        auto update4 = [&](int row, int col0, const f4 &a, bool diag16, bool posecols, bool mir) {
                if (diag16 || posecols)
                {
                        // 16x16 tile on the diagonal: the elements J < I, each with its mirror image (J == I: the X update);
                        // columns 0 .. 3: column 3 only
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                                if (col0 + r < row && !(posecols && r < 3) && col0 + r < n)
                                {
                                        double *pe = P + (size_t)row * NP + col0 + r;
                                        const double pn = *pe - (double)a[r];
                                        *pe = pn;
                                        P[(size_t)(col0 + r) * NP + row] = pn;
                                }
                        return;
                }
                double *pp = P + (size_t)row * NP + col0;
                double nv4[4];
                if (col0 + 3 < n)
                {
                        const d2 o0 = *reinterpret_cast<const d2 *>(pp), o1 = *reinterpret_cast<const d2 *>(pp + 2);
                        nv4[0] = o0[0] - (double)a[0], nv4[1] = o0[1] - (double)a[1];
                        nv4[2] = o1[0] - (double)a[2], nv4[3] = o1[1] - (double)a[3];
                        *reinterpret_cast<d2 *>(pp) = (d2){nv4[0], nv4[1]};
                        *reinterpret_cast<d2 *>(pp + 2) = (d2){nv4[2], nv4[3]};
                }
                else
                {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                                if (col0 + r < n)
                                {
                                        nv4[r] = pp[r] - (double)a[r];
                                        pp[r] = nv4[r];
                                }
                }
                if (mir)
                {
#pragma unroll
                        for (int r = 0; r < 4; ++r)
                                if (col0 + r < n)
                                        P[(size_t)(col0 + r) * NP + row] = nv4[r];
                }
        };
        if (tailw)
        {
                // rows 128 rl + li of the tail x column tile jt: what tile (rl, jt) stored (columns < 128 rl < n; pose columns where jt == 0)
                const int row = tail.rl * TB + li;
                if (row < n)
#pragma unroll
                        for (int v = 0; v < 8; ++v)
                                update4(row, jt * TB + 16 * v + 4 * lg, acc[v >> 2][v & 3], false, jt == 0 && lg == 0 && v == 0, true);
                return;
        }
        const bool posecols_lane = (jt == 0 && wc == 0 && lg == 0);
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int v = 0; v < 4; ++v)
                {
                        const int row = rt * TB + wr + 16 * u + li;
                        const int col0 = jt * TB + wc + 16 * v + 4 * lg;
                        if (row >= n || col0 >= n || (diagq && v > u))
                                continue;
                        update4(row, col0, acc[u][v], diagq && v == u, posecols_lane && v == 0 /* this lane's four columns are 0 .. 3 */, mirror || diagq);
                }
}

/// X <- X + V q with q = row n of G = (L^-1 Y)^T; one wave per state row.  grid (ceil(NP/4), B), 256 threads.  In replay
/// mode also writes the pose of this callback.  The binary64 chain's X update; the binary32 chain runs large_x_update_rows below.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void large_x_update(DevView d, LargeView<T> lv, int s, int nsteps, double *poses_out,
                                                      int32_t *dims_out, const int *skipped)
{
        const int b = blockIdx.y;
        if (skipped[b])
                return;
        const int n = d.n[b], NP = lv.NP;
        const int a = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
        if (a >= n)
                return;
        const T *vrow = lv.G + ((size_t)b * NP + a) * NP;
        const T *q = lv.G + ((size_t)b * NP + n) * NP;
        double acc = 0.0;
        // 16 bytes per lane and load (rows are 256-byte aligned: NP is a multiple of 64); columns n .. of both rows are zero
        typedef T vec_t __attribute__((ext_vector_type(16 / sizeof(T))));
        constexpr int VW = 16 / sizeof(T);
        for (int j = VW * lane; j < n; j += 64 * VW)
        {
                const vec_t v = *reinterpret_cast<const vec_t *>(vrow + j), w = *reinterpret_cast<const vec_t *>(q + j);
#pragma unroll
                for (int e = 0; e < VW; ++e)
                        acc = fma((double)v[e], (double)w[e], acc);
        }
        acc = wave_sum_dpp(acc);
        if (lane == 63)
        {
                const double xa = d.X[(size_t)b * NP + a] + acc;
                d.X[(size_t)b * NP + a] = xa;
                if (MODE == MODE_REPLAY)
                {
                        if (a < 3 && poses_out)
                                poses_out[((size_t)b * nsteps + s) * 3 + a] = xa;
                        if (a == 0 && dims_out)
                                dims_out[(size_t)b * nsteps + s] = n;
                }
        }
}
/// binary32 chain: X <- X + V q, and -- in the same pass over row a of V, with binary64 accumulation -- the entries of V V^T that large_syrk_bf16x3
/// leaves out: the DIAGONAL (a sum of squares: every rounding of an fp32 accumulator chain pulls it the same way, and the covariance
/// diagonal is where the error of the fp32 path was largest) and the three POSE columns (the pose block changes by as much as it holds in
/// every callback, Q against the update, so eps32 |dP| is eps32 |P| there), which are subtracted from P: P(a,a), P(a,0..2) and the mirror
/// image P(0..2,a).  Costs four more FMAs per element of a row the kernel reads anyway.  The four rows
/// every row of V is multiplied with -- q and the pose rows of V -- staged ONCE per workgroup in LDS, widened to binary64 (XuStaged: 60 KB with the
/// rows of l), for the XU_ROWS x XU_WAVES rows its waves walk.  With a wave per row and the shared rows read from memory every wave issued 25 loads of 16 bytes per lane for 4 KB of new data: 391 us
/// per 256 filters against 217 us for round 2's single product (profiles/r03_experiments.md).  grid (ceil(NP / XU_WG_ROWS), B), XU_THREADS threads.
///
/// XU_WAVES waves of XU_ROWS rows each share one staging and one border prologue.  Waves 0 .. 3 do the prologue's staging and sums with the strides of a
/// 256-thread workgroup, whatever XU_WAVES is, and a wave's walk over its rows does not depend on it either: every XU_WAVES gives the same bits.  Every
/// wave issues the loads of its first row in front of the workgroup's one barrier.  What the prologue leaves behind (L22^-1, V2 of row n and of the pose
/// rows) is the same in every thread and is moved to scalar registers: the row loop fits 128 vector registers, so that two workgroups of 8 waves (or
/// one of 16) share a CU, four waves per SIMD.  XU_WAVES = 8: 17 workgroups of 64 rows for the 1027 rows of the benchmark; 4, 8 and 16 are measured
/// in profiles/xupdate.md.
///
/// THE BORDER (large_border): for a filter with a tail of t <= 3 rows past its last full 64-block the Cholesky and the TRSM in front of this kernel
/// have covered the n0 = n - t leading columns only, and this kernel -- which runs IN FRONT OF the syrk then -- finishes the factorisation:
///   * every workgroup stages, for the columns < n0, q1 (row n), the pose rows of V1 and the t rows of l (rows n+1 .. n+t of G), and forms from them, in
///     binary64,  C = S22 - l l^T = L22 L22^T,  L22^-1  and  V2 = (G2 - V1 l^T) L22^-T  of row n (q2) and of the pose rows.  Same code, same order in
///     every workgroup (every thread, in fact): all of them hold bit-equal values.  The G2 of those four rows is read from the copies large_build_GS
///     left in the spare rows (BORDER_SAVE), not from the rows themselves, which their owners overwrite with V2 meanwhile; nobody reads another row's
///     columns >= n0.
///   * per row a, t more dot products V1(a) . l_k in the same pass give V2(a), which is stored in binary32 over G2(a) (the K loop of the syrk then reads the
///     border like any other column), and the V2 terms are added to V q, the diagonal and the pose columns.
///     The pass always carries BORDER_MAX = 3 rows of l: with t = 1 two of them are staged as zeros and their dot products and LDS reads are wasted work
///     (n mod 64 = 1 is not the benchmark's case; two more instantiations would remove it).
///   * workgroup 0 of the filter stores q2 into row n, writes L22^-1 into block nbc of Linv (identity outside the t x t corner: large_stats reads the
///     diagonal for ln det S) and raises ASLAM_ST_NOT_PD on a non-positive pivot of C, as the Cholesky does for its blocks.
constexpr int XU_SH_ROWS = 4 + BORDER_MAX;                                      // staged rows: q, pose rows 0 .. 2 of V, l_0 .. l_2
constexpr int XU_NDOT = 4 * BORDER_MAX + BORDER_MAX * (BORDER_MAX + 1) / 2;     // {q, pose rows} . l_k, then the lower triangle of l l^T

/// One staged row in LDS, widened to binary64 ONCE per workgroup (the conversion is exact) instead of once per row of V and element in every wave: of the
/// 8 conversions and 8 FMAs per element of V the row loop keeps one conversion.  Columns 4c, 4c + 1 of the row are h[0][c], columns 4c + 2, 4c + 3 are
/// h[1][c]: a lane owns four consecutive columns and reads them as two 16-byte accesses, each of them dense over the wave (no bank conflict).
struct XuStaged
{
        xu_d2 h[2][LARGE_NP_MAX / 4];
        __device__ __forceinline__ void put(int j, const f4 &r)
        {
                h[0][j >> 2] = (xu_d2){(double)r[0], (double)r[1]};
                h[1][j >> 2] = (xu_d2){(double)r[2], (double)r[3]};
        }
};

__device__ __forceinline__ float readfirstlane_f32(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

/// what a workgroup knows of its filter's border; the same values in every thread
struct XuBorder
{
        double Li[BORDER_MAX][BORDER_MAX]; // L22^-1 (lower triangle; beyond t: the identity)
        float v2[4][BORDER_MAX];           // V2 of row n (q2) and of pose rows 0 .. 2, as stored (beyond t: 0)
        bool ok;                           // every pivot of C was positive
};

/// stages the shared rows (columns < n0 only) and solves the border; contains the workgroup's one barrier.  Staging and sums are the work of threads
/// 0 .. XU_STAGE_THREADS - 1, the 3 x 3 behind the barrier of every thread
__device__ __forceinline__ XuBorder x_update_border(XuStaged *sh, double (*red)[XU_NDOT], const LargeView<float> &lv, int b, int n, const LargeBorder &bd)
{
        constexpr int BM = BORDER_MAX;
        const int NP = lv.NP, tid = threadIdx.x, t = bd.t, n0 = LB * bd.nbc;
        const float *G = lv.G + (size_t)b * NP * NP, *S = lv.S + (size_t)b * NP * NP;
        // S22 and the saved G2 first: their latency hides behind the staging
        float s22[BM][BM], g2[4][BM];
#pragma unroll
        for (int i = 0; i < BM; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j)
                        s22[i][j] = i < t ? S[(size_t)(n0 + i) * NP + n0 + j] : (i == j ? 1.f : 0.f);
#pragma unroll
        for (int k = 0; k < BM; ++k)
#pragma unroll
                for (int m = 0; m < 4; ++m)
                        g2[m][k] = k < t ? G[(size_t)(n + 1 + k) * NP + n0 + BORDER_SAVE + ((m + 3) & 3)] : 0.f; // (here m = 0 is row n, the copies keep it last)
        double dot[XU_NDOT];
#pragma unroll
        for (int i = 0; i < XU_NDOT; ++i)
                dot[i] = 0.0;
        if (tid < XU_STAGE_THREADS) // (wave-uniform)
        {
                for (int j = 4 * tid; j < n0; j += 4 * XU_STAGE_THREADS)
                {
                        f4 r[XU_SH_ROWS];
                        r[0] = *reinterpret_cast<const f4 *>(G + (size_t)n * NP + j);
#pragma unroll
                        for (int m = 0; m < 3; ++m)
                                r[1 + m] = *reinterpret_cast<const f4 *>(G + (size_t)m * NP + j);
#pragma unroll
                        for (int k = 0; k < BM; ++k)
                                r[4 + k] = k < t ? *reinterpret_cast<const f4 *>(G + (size_t)(n + 1 + k) * NP + j) : (f4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int m = 0; m < XU_SH_ROWS; ++m)
                                sh[m].put(j, r[m]);
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                        {
#pragma unroll
                                for (int m = 0; m < 4; ++m)
#pragma unroll
                                        for (int k = 0; k < BM; ++k)
                                                dot[BM * m + k] = fma((double)r[m][e], (double)r[4 + k][e], dot[BM * m + k]);
#pragma unroll
                                for (int i = 0; i < BM; ++i)
#pragma unroll
                                        for (int k = 0; k <= i; ++k)
                                                dot[4 * BM + i * (i + 1) / 2 + k] = fma((double)r[4 + i][e], (double)r[4 + k][e], dot[4 * BM + i * (i + 1) / 2 + k]);
                        }
                }
#pragma unroll
                for (int i = 0; i < XU_NDOT; ++i)
                        dot[i] = wave_sum_dpp(dot[i]);
                if ((tid & 63) == 63)
                {
#pragma unroll
                        for (int i = 0; i < XU_NDOT; ++i)
                                red[tid >> 6][i] = dot[i];
                }
        }
        __syncthreads();
        // (S22 and G2 were loaded from addresses every thread shares: kept as the 18 floats they are while the loads were in flight, scalars from here on)
#pragma unroll
        for (int i = 0; i < BM; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j)
                        s22[i][j] = readfirstlane_f32(s22[i][j]);
#pragma unroll
        for (int k = 0; k < BM; ++k)
#pragma unroll
                for (int m = 0; m < 4; ++m)
                        g2[m][k] = readfirstlane_f32(g2[m][k]);
        static_assert(XU_STAGE_THREADS == 4 * 64, "the sum below is written out for four staging waves");
#pragma unroll
        for (int i = 0; i < XU_NDOT; ++i)
                dot[i] = readfirstlane_f64((red[0][i] + red[1][i]) + (red[2][i] + red[3][i]));
        // C = S22 - l l^T, its Cholesky factor and the inverse of that (rows >= t: the identity)
        XuBorder bx;
        double L[BM][BM];
        bx.ok = true;
#pragma unroll
        for (int j = 0; j < BM; ++j)
        {
                double sjj = (double)s22[j][j] - dot[4 * BM + j * (j + 1) / 2 + j];
#pragma unroll
                for (int k = 0; k < j; ++k)
                        sjj -= L[j][k] * L[j][k];
                bx.ok = bx.ok && sjj > 0.0;
                L[j][j] = sqrt(sjj); // (a non-positive pivot: flagged by workgroup 0 and the NaNs go on into Linv, V2, X and P -- "flag and go on", as chol64::factor_and_invert does for the blocks)
#pragma unroll
                for (int i = j + 1; i < BM; ++i)
                {
                        double sij = (double)s22[i][j] - dot[4 * BM + i * (i + 1) / 2 + j];
#pragma unroll
                        for (int k = 0; k < j; ++k)
                                sij -= L[i][k] * L[j][k];
                        L[i][j] = sij / L[j][j];
                }
        }
        static_assert(BM == 3, "the inverse below is written out for 3 x 3");
        bx.Li[0][0] = 1.0 / L[0][0], bx.Li[1][1] = 1.0 / L[1][1], bx.Li[2][2] = 1.0 / L[2][2];
        bx.Li[1][0] = -(L[1][0] * bx.Li[0][0]) * bx.Li[1][1];
        bx.Li[2][1] = -(L[2][1] * bx.Li[1][1]) * bx.Li[2][2];
        bx.Li[2][0] = -(L[2][0] * bx.Li[0][0] + L[2][1] * bx.Li[1][0]) * bx.Li[2][2];
        bx.Li[0][1] = bx.Li[0][2] = bx.Li[1][2] = 0.0;
        // V2 = (G2 - V1 l^T) L22^-T of row n and of the pose rows
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
                for (int j = 0; j < BM; ++j)
                {
                        double v = 0.0;
#pragma unroll
                        for (int k = 0; k <= j; ++k)
                                v += ((double)g2[m][k] - dot[BM * m + k]) * bx.Li[j][k];
                        bx.v2[m][j] = (float)v;
                }
        return bx;
}

/// passes of 64 lanes x 4 columns over a row: 5 x 256 = 1280 >= LARGE_NP_MAX; with a border the pass stops at n0 <= LARGE_NP_MAX - LB = 4 x 256
template <bool BORDER> constexpr int XU_NPASS = BORDER ? 4 : 5;
static_assert(5 * 256 >= LARGE_NP_MAX && 4 * 256 >= LARGE_NP_MAX - LB, "large_x_update_rows: passes per row");

/// the first row of wave `wave` of workgroup `xb`
__device__ __forceinline__ int x_update_first_row(int xb, int wave) { return (xb * XU_WAVES + wave) * XU_ROWS; }

/// row a of V (of filter matrix G) into registers: 16 bytes per lane and pass.  BORDER: the pass stops at n0 (= jlim); the row's G2 (columns n0 .. n0 + 3:
/// 16 aligned bytes, zero from column n on) rides along with the loads of the row
template <bool BORDER>
__device__ __forceinline__ void x_update_load_row(f4 (&v)[XU_NPASS<BORDER>], f4 &g2, const float *G, int NP, int n, int jlim, int n0, int a)
{
        const int lane = threadIdx.x & 63;
        const float *vr = G + (size_t)min(a, n - 1) * NP;
#pragma unroll
        for (int i = 0; i < XU_NPASS<BORDER>; ++i)
        {
                const int j = 4 * lane + 256 * i;
                v[i] = j < jlim ? *reinterpret_cast<const f4 *>(vr + j) : (f4){0.f, 0.f, 0.f, 0.f}; // (columns n .. of every row of V are zero)
        }
        if constexpr (BORDER)
                g2 = *reinterpret_cast<const f4 *>(vr + n0);
}

/// the XU_ROWS rows of one wave; vn, g2n: the wave's first row, loaded by the caller (x_update_load_row) in front of the workgroup's barrier
template <int MODE, bool BORDER>
__device__ __forceinline__ void x_update_rows_loop(const XuStaged *sh, const XuBorder &bx, const DevView &d, const LargeView<float> &lv, int b, int xb, int n,
                                                   int n0, int s, int nsteps, double *poses_out, int32_t *dims_out, f4 (&vn)[XU_NPASS<BORDER>], f4 &g2n)
{
        const int NP = lv.NP;
        const int tid = threadIdx.x, lane = tid & 63;
        float *G = lv.G + (size_t)b * NP * NP;
        double *P = lv.P + (size_t)b * NP * NP;
        const int a0 = x_update_first_row(xb, __builtin_amdgcn_readfirstlane(tid >> 6));
        constexpr int NPASS = XU_NPASS<BORDER>;
        const int jlim = BORDER ? n0 : n;
        auto load_row = [&](f4 (&v)[NPASS], f4 &g2, int a) { x_update_load_row<BORDER>(v, g2, G, NP, n, jlim, n0, a); };
        // What the prologue left, the same in every thread, as scalars: L22^-1, V2 of row n (q2) and of the pose rows
        double Li[BORDER_MAX][BORDER_MAX];
        float q2[BORDER_MAX], pv[3][BORDER_MAX];
#pragma unroll
        for (int k = 0; k < BORDER_MAX; ++k)
        {
#pragma unroll
                for (int j = 0; j < BORDER_MAX; ++j)
                        Li[k][j] = j <= k ? readfirstlane_f64(bx.Li[k][j]) : 0.0;
                q2[k] = readfirstlane_f32(bx.v2[0][k]);
#pragma unroll
                for (int m = 0; m < 3; ++m)
                        pv[m][k] = readfirstlane_f32(bx.v2[1 + m][k]);
        }
        // the loads of row a + 1 are issued before row a is multiplied: the kernel lives on bytes in flight
#pragma unroll 1
        for (int r = 0; r < XU_ROWS; ++r)
        {
                const int a = a0 + r;
                if (a >= n)
                        break; // wave-uniform
                f4 v[NPASS];
                const f4 g2 = g2n;
#pragma unroll
                for (int i = 0; i < NPASS; ++i)
                        v[i] = vn[i];
                if (r + 1 < XU_ROWS)
                        load_row(vn, g2n, a + 1);
                // The entries of P and X this row updates (nobody else touches them: P(a, 0 .. 2) with the mirror image, P(a, a), X(a)) are fetched NOW and
                // needed behind the sums.  Fetched there, every row of every wave ended in a round trip to memory with nothing else of the wave in
                // flight: 400 -> 343 us per 256 filters (profiles/xupdate.md)
                double *prow = P + (size_t)a * NP;
                double pold[3] = {0.0, 0.0, 0.0}, pdiag = 0.0, xold = 0.0;
                if (lane == 63)
                {
#pragma unroll
                        for (int j = 0; j < 3; ++j)
                                if (j < a)
                                        pold[j] = prow[j];
                        pdiag = prow[a];
                        xold = d.X[(size_t)b * NP + a];
                }
                double acc = 0.0, dd = 0.0, d0 = 0.0, d1 = 0.0, d2 = 0.0, e0 = 0.0, e1 = 0.0, e2 = 0.0;
#pragma unroll
                for (int i = 0; i < NPASS; ++i)
                {
                        const int j = 4 * lane + 256 * i;
                        if (j >= jlim)
                                continue; // (beyond NP nothing was staged)
#pragma unroll
                        for (int h = 0; h < 2; ++h) // columns j, j + 1, then j + 2, j + 3: the order of the sums is that of the columns
                        {
                                const xu_d2 wi = sh[0].h[h][j >> 2], p0 = sh[1].h[h][j >> 2], p1 = sh[2].h[h][j >> 2], p2 = sh[3].h[h][j >> 2];
                                xu_d2 l0 = {0.0, 0.0}, l1 = l0, l2 = l0;
                                if constexpr (BORDER)
                                        l0 = sh[4].h[h][j >> 2], l1 = sh[5].h[h][j >> 2], l2 = sh[6].h[h][j >> 2];
#pragma unroll
                                for (int e = 0; e < 2; ++e)
                                {
                                        const double ve = (double)v[i][2 * h + e];
                                        acc = fma(ve, wi[e], acc);
                                        dd = fma(ve, ve, dd);
                                        d0 = fma(ve, p0[e], d0);
                                        d1 = fma(ve, p1[e], d1);
                                        d2 = fma(ve, p2[e], d2);
                                        if constexpr (BORDER)
                                        {
                                                e0 = fma(ve, l0[e], e0);
                                                e1 = fma(ve, l1[e], e1);
                                                e2 = fma(ve, l2[e], e2);
                                        }
                                }
                        }
                }
                acc = wave_sum_dpp(acc), dd = wave_sum_dpp(dd), d0 = wave_sum_dpp(d0), d1 = wave_sum_dpp(d1), d2 = wave_sum_dpp(d2);
                if constexpr (BORDER)
                        e0 = wave_sum_dpp(e0), e1 = wave_sum_dpp(e1), e2 = wave_sum_dpp(e2);
                if constexpr (BORDER)
                {
                        // q2 and the V2 of the pose rows, pinned in their scalar registers in every pass: they are selected by the row index below (a select
                        // between members of a struct sends the whole struct to scratch memory), and widened to binary64 outside the loop they would
                        // occupy 24 vector registers for all of it
#pragma unroll
                        for (int k = 0; k < BORDER_MAX; ++k)
                        {
                                asm volatile("" : "+s"(q2[k]));
#pragma unroll
                                for (int m = 0; m < 3; ++m)
                                        asm volatile("" : "+s"(pv[m][k]));
                        }
                }
                if (lane == 63)
                {
                        if constexpr (BORDER)
                        {
                                // V2(a) = (G2(a) - V1(a) l^T) L22^-T, rounded to binary32 as it is stored; the pose rows take the values every
                                // workgroup holds (the same expression over another order of summation)
                                const double w0 = (double)g2[0] - e0, w1 = (double)g2[1] - e1, w2 = (double)g2[2] - e2;
                                float x0 = (float)(w0 * Li[0][0]), x1 = (float)(w0 * Li[1][0] + w1 * Li[1][1]),
                                      x2 = (float)(w0 * Li[2][0] + w1 * Li[2][1] + w2 * Li[2][2]);
                                if (a < 3)
                                {
                                        x0 = a == 0 ? pv[0][0] : a == 1 ? pv[1][0] : pv[2][0];
                                        x1 = a == 0 ? pv[0][1] : a == 1 ? pv[1][1] : pv[2][1];
                                        x2 = a == 0 ? pv[0][2] : a == 1 ? pv[1][2] : pv[2][2];
                                }
                                *reinterpret_cast<f4 *>(G + (size_t)a * NP + n0) = (f4){x0, x1, x2, 0.f}; // (x_k = 0 for k >= t: column n .. stay zero)
                                const float xs[BORDER_MAX] = {x0, x1, x2};
#pragma unroll
                                for (int k = 0; k < BORDER_MAX; ++k)
                                {
                                        const double ve = (double)xs[k];
                                        acc = fma(ve, (double)q2[k], acc);
                                        dd = fma(ve, ve, dd);
                                        d0 = fma(ve, (double)pv[0][k], d0);
                                        d1 = fma(ve, (double)pv[1][k], d1);
                                        d2 = fma(ve, (double)pv[2][k], d2);
                                }
                        }
                        const double dp[3] = {d0, d1, d2};
                        // pose columns j < min(a, 3) with their mirror image; the diagonal entry itself
#pragma unroll
                        for (int j = 0; j < 3; ++j)
                                if (j < a)
                                {
                                        const double pn = pold[j] - dp[j];
                                        prow[j] = pn;
                                        P[(size_t)j * NP + a] = pn;
                                }
                        prow[a] = pdiag - dd;
                        const double xa = xold + acc;
                        d.X[(size_t)b * NP + a] = xa;
                        if (MODE == MODE_REPLAY)
                        {
                                if (a < 3 && poses_out)
                                        poses_out[((size_t)b * nsteps + s) * 3 + a] = xa;
                                if (a == 0 && dims_out)
                                        dims_out[(size_t)b * nsteps + s] = n;
                        }
                }
        }
}

/// the body: workgroup `xb` of filter `b` (XU_WG_ROWS rows); sh = XU_SH_ROWS staged rows in LDS, red = 4 x XU_NDOT doubles
template <int MODE>
__device__ __forceinline__ void x_update_rows_body(XuStaged *sh, double (*red)[XU_NDOT], const DevView &d, const LargeView<float> &lv, int b, int xb, int n,
                                                   int s, int nsteps, double *poses_out, int32_t *dims_out)
{
        const int NP = lv.NP;
        const int tid = threadIdx.x;
        if (xb * XU_WG_ROWS >= n)
                return;
        float *G = lv.G + (size_t)b * NP * NP;
        const LargeBorder bd = large_border(n, lv.border);
        const int n0 = LB * bd.nbc;
        const int a0 = x_update_first_row(xb, __builtin_amdgcn_readfirstlane(tid >> 6));
        f4 g20 = {0.f, 0.f, 0.f, 0.f};
        if (bd.t)
        {
                f4 v0[XU_NPASS<true>];
                x_update_load_row<true>(v0, g20, G, NP, n, n0, n0, a0);
                const XuBorder bx = x_update_border(sh, red, lv, b, n, bd);
                if (xb == 0)
                {
                        // row n of V, the border's block of Linv, the status
                        float *Lb = lv.Linv + ((size_t)b * LARGE_NB_MAX + bd.nbc) * LB * LB;
                        for (int e = tid; e < LB * LB; e += XU_THREADS)
                        {
                                const int r = e >> 6, c = e & (LB - 1);
                                double v = r == c ? 1.0 : 0.0;
                                if (r < BORDER_MAX && c <= r)
                                        v = r == 0 ? bx.Li[0][0] : r == 1 ? (c == 0 ? bx.Li[1][0] : bx.Li[1][1]) : (c == 0 ? bx.Li[2][0] : c == 1 ? bx.Li[2][1] : bx.Li[2][2]);
                                Lb[e] = (float)v;
                        }
                        if (tid == 0)
                        {
                                *reinterpret_cast<f4 *>(G + (size_t)n * NP + n0) = (f4){bx.v2[0][0], bx.v2[0][1], bx.v2[0][2], 0.f}; // (columns n .. of every row are zero)
                                if (!bx.ok)
                                        atomicOr(&d.status[b], 4u); // ASLAM_ST_NOT_PD
                        }
                }
                x_update_rows_loop<MODE, true>(sh, bx, d, lv, b, xb, n, n0, s, nsteps, poses_out, dims_out, v0, g20);
        }
        else
        {
                f4 v0[XU_NPASS<false>];
                x_update_load_row<false>(v0, g20, G, NP, n, n, n0, a0);
                for (int j = 4 * tid; j < NP; j += 4 * XU_THREADS)
                {
                        sh[0].put(j, *reinterpret_cast<const f4 *>(G + (size_t)n * NP + j));
                        sh[1].put(j, *reinterpret_cast<const f4 *>(G + j));
                        sh[2].put(j, *reinterpret_cast<const f4 *>(G + NP + j));
                        sh[3].put(j, *reinterpret_cast<const f4 *>(G + 2 * (size_t)NP + j));
                }
                __syncthreads();
                x_update_rows_loop<MODE, false>(sh, XuBorder{}, d, lv, b, xb, n, n0, s, nsteps, poses_out, dims_out, v0, g20);
        }
}

/// grid (ceil(NP / XU_WG_ROWS), B), XU_THREADS threads
template <int MODE>
__global__ __launch_bounds__(XU_THREADS, 4) void large_x_update_rows(DevView d, LargeView<float> lv, int s, int nsteps, double *poses_out, int32_t *dims_out, const int *skipped)
{
        __shared__ __attribute__((aligned(16))) XuStaged sh[XU_SH_ROWS]; // q, pose rows 0 .. 2 of V, the rows of l (border)
        __shared__ double red[4][XU_NDOT];
        const int b = blockIdx.y;
        if (skipped[b])
                return;
        x_update_rows_body<MODE>(sh, red, d, lv, b, (int)blockIdx.x, d.n[b], s, nsteps, poses_out, dims_out);
}

/// The statistics of a callback (StatsView), launched behind the chain only when somebody asks for them: every chain leaves what they need.
///   EKF: row n of G (lv.G as the consumers of V see it) is q = (L^-1 Y)^T:  Y^T S^-1 Y = q.q
///   UKF (lv.xrows == 2): rows n, n + 1 are q = L^-1 z and t = L^-1 (Z - Zpred) for S = S+ - z z^T, S+ = L L^T (ukf_large.h):
///        NIS = t.t + (q.t)^2 / (1 - q.q),   det S = det S+ (1 - q.q)
///   ln det L L^T = -2 sum ln Linv_ii: the inverted diagonal blocks exist in T in every chain (the bf16-pipe Cholesky writes them too)
/// Every entry is widened to binary64 before it is multiplied; the sums are binary64.  grid (B), 256 threads.
template <typename T>
__global__ __launch_bounds__(256) void large_stats(DevView d, LargeView<T> lv, int s, int nsteps, StatsView sv, const int *skipped)
{
        __shared__ double red[4][4];
        const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
        if (skipped[b])
        {
                stats_skip(sv, b, s, nsteps, tid);
                return;
        }
        const int n = d.n[b], NP = lv.NP;
        const bool ukf = lv.xrows == 2;
        const T *q = lv.G + ((size_t)b * NP + n) * NP, *t = q + NP;
        const T *Li = lv.Linv + (size_t)b * LARGE_NB_MAX * LB * LB;
        double tt = 0.0, qq = 0.0, qt = 0.0, ld = 0.0;
        for (int j0 = 0; j0 < NP; j0 += 256) // (the same trip count in every lane: the DPP sums below need the whole wave)
        {
                const int j = j0 + tid;
                const bool in = j < n;
                const int jc = in ? j : 0;
                const double qv = in ? (double)q[jc] : 0.0;
                const double tv = (in && ukf) ? (double)t[jc] : 0.0;
                const double di = in ? (double)Li[(size_t)(jc >> 6) * LB * LB + (jc & (LB - 1)) * (LB + 1)] : 1.0;
                qq = fma(qv, qv, qq);
                qt = fma(qv, tv, qt);
                tt = fma(tv, tv, tt);
                ld += log(di);
        }
        qq = wave_sum_dpp(qq), qt = wave_sum_dpp(qt), tt = wave_sum_dpp(tt), ld = wave_sum_dpp(ld);
        if (lane == 63)
                red[tid >> 6][0] = qq, red[tid >> 6][1] = qt, red[tid >> 6][2] = tt, red[tid >> 6][3] = ld;
        __syncthreads();
        if (tid == 0)
        {
                double r[4];
                for (int k = 0; k < 4; ++k)
                        r[k] = (red[0][k] + red[1][k]) + (red[2][k] + red[3][k]);
                const double den = 1.0 - r[0];
                double nis = ukf ? r[2] + r[1] * r[1] / den : r[0];
                double logdet = ukf ? -2.0 * r[3] + log(fabs(den)) : -2.0 * r[3];
                if (d.status[b] & 4u) // ASLAM_ST_NOT_PD (sticky): no statistics from a factor that does not exist
                        nis = logdet = __builtin_nan("");
                stats_put(sv, b, s, nsteps, nis, logdet);
        }
        if (tid < 6)
        {
                const int r = tid < 1 ? 0 : tid < 3 ? 1 : 2;
                stats_put_pcov(sv, b, s, nsteps, tid, lv.P[(size_t)b * NP * NP + (size_t)r * NP + tid - r * (r + 1) / 2]);
        }
}
} // namespace aslam

#include "ekf_large_trsm.h"
#include "ekf_large_chol.h"
#include "ekf_large_trsm16.h"
