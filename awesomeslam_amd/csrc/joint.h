// joint.h -- aslam_joint_compat (include/aslam_core.h): the joint-compatibility test of a hypothesis of pairings, on the device.
//
// Individual compatibility (assoc.h) decides each pairing alone; the landmarks of a map are correlated through the pose, so pairings that
// each pass can be inconsistent as a set.  This is the sequential compatibility nearest neighbour rule: the candidates cand[j] of the
// observations j = 0 .. n_obs-1, in message order, each tested against the pairings accepted before it.  With A the accepted list, m = |A|:
//     C_A    the stack of H_i P(idx_i, idx_i') H_i'^T over A, + diag(r_range, r_bearing) on the diagonal blocks      (2m x 2m)
//     L_A    its lower Cholesky factor     z_A = L_A^-1 nu_A     D2 = |z_A|^2     logdet = 2 sum log L_A(ii)
// and for candidate j by bordering:
//     c = the cross blocks H_j P(idx_j, idx_i) H_i^T (2 x 2m)      Y = c L_A^-T (forward substitution)      T = C_jj - Y Y^T
//     t00 = sqrt(T00)   t10 = T10 / t00   d = T11 - t10^2   t11 = sqrt(d)
//     w = nu_j - Y z_A   z0 = w0 / t00   z1 = (w1 - t10 z0) / t11   dd = z0^2 + z1^2
// unusable: cand outside [0, L), q not > 0, T00 or d not > 0, dd not finite (a NaN fails every comparison).  Accepted iff
// D2 + dd < gate_tab[m + 1] (no table: every usable candidate); else refused, nothing appended.  Everything is binary64; only lower-triangle
// entries of P are read.  Deterministic, O(m^3), and dependent on the message order: there is no search over alternative candidates.
//
//   joint_compat   one workgroup of 256 threads per filter, dynamic LDS sized from ldo (JointLds).
//                  Phase 0  cand and n_obs into LDS, clamped: a candidate outside [0, L) is never used as an index.  Every read of cand
//                           happens here, before the first write of assoc -- assoc == cand is allowed.
//                  Phase 1  lanes over candidates: H (2 x 5), nu into LDS (gate_jacobian, gate_math.h).
//                  Phase 2  threads over candidate pairs i >= j: 25 entries of P, one 2 x 2 congruence into the packed lower triangle.
//                  Phase 3  wave 0, lanes over the columns of L_A (two per lane at most): the bordering, in place on the triangle.  Column
//                           oriented: once y_p is known every lane subtracts its multiple from its own later columns; the reductions (Y Y^T,
//                           Y z_A) come once per candidate.  Control (m, the candidate, the verdict) is made wave-uniform with readfirstlane;
//                           every whole-wave exchange sits outside lane-dependent branches.
//                  Phase 4  assoc, incr from LDS to HBM.
//
// Every loop is bounded by ldo (validated by the host, at most JOINT_MAX_OBS) or by m <= ldo.  The kernel writes its outputs and nothing else.
#pragma once

#include "gate_math.h"
#include "prune.h"

namespace aslam
{
constexpr int JOINT_WG = 256;
constexpr int JOINT_MAX_OBS = 64; // = ASLAM_JC_MAX_OBS: two columns of L_A per lane of one wave
constexpr int JOINT_LMAX = 542;   // landmarks of the largest state a context accepts (ASSOC_LMAX)

/// the dynamic LDS of joint_compat for a message stride of ldo: doubles first, then the two int arrays
struct JointLds
{
        int ldo;
        __host__ __device__ size_t tri() const { return (size_t)ldo * (2 * ldo + 1); } // (2 ldo)(2 ldo + 1) / 2
        __host__ __device__ size_t doubles() const { return tri() + 10 * (size_t)ldo + 2 * (size_t)ldo + (size_t)ldo + (size_t)ldo + 1; }
        __host__ __device__ size_t bytes() const { return sizeof(double) * doubles() + sizeof(int) * 2 * (size_t)ldo; }
};

/// entry (r, c), r >= c, of the packed lower triangle
__device__ __forceinline__ int joint_tri(int r, int c)
{
        return r * (r + 1) / 2 + c;
}

/// the sum of v over the 64 lanes, the same bits in every lane.  A whole-wave exchange: all lanes active.
__device__ __forceinline__ double joint_wave_sum(double v)
{
        for (int d = 32; d >= 1; d >>= 1)
                v += __shfl_xor(v, d);
        return v;
}

/// One forward-substitution step p of slot S (p = 64 S + src): y_p = c_p / L_pp into the owner's registers, its multiples off every later column
template <int S>
__device__ __forceinline__ void joint_solve_step(const double *tri, int src, int lane, int m2, const int (&col)[2], const double (&diag)[2],
                                                 double (&c0)[2], double (&c1)[2])
{
        const int cp = __builtin_amdgcn_readlane(col[S], src);
        const double lpp = readlane_f64(diag[S], src);
        const double y0 = readlane_f64(c0[S], src) / lpp;
        const double y1 = readlane_f64(c1[S], src) / lpp;
        const int p = 64 * S + src;
#pragma unroll
        for (int s = S; s < 2; ++s)
        {
                const int ci = lane + 64 * s;
                if (ci > p && ci < m2)
                {
                        const double l = tri[joint_tri(col[s], cp)];
                        c0[s] = fma(-l, y0, c0[s]);
                        c1[s] = fma(-l, y1, c1[s]);
                }
                else if (ci == p)
                        c0[s] = y0, c1[s] = y1;
        }
}

/// grid: filters, block: JOINT_WG, dynamic LDS: JointLds{ldo}.bytes().  obs [batch][ldo][2] f32, n_obs [batch], cand [batch][ldo] i32, gate_tab
/// [ldo + 1] or null (evaluate mode); assoc [batch][ldo] i32 (may be cand itself), incr [batch][ldo] f64 or null, joint [batch][2] f64 (D2, log det
/// C_A), count [batch][2] i32 (accepted, refused by the joint test).  (cand and assoc carry no __restrict__: they may be one array.)
__global__ __launch_bounds__(JOINT_WG) void joint_compat(const double *__restrict__ X, const double *__restrict__ P, const int *__restrict__ n, int NP,
                                                         const aslam_params *__restrict__ prm, const float *__restrict__ obs, int ldo,
                                                         const int32_t *__restrict__ n_obs, const int32_t *cand, const double *__restrict__ gate_tab,
                                                         int32_t *assoc, double *__restrict__ incr, double *__restrict__ joint,
                                                         int32_t *__restrict__ count)
{
        extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
        const JointLds lds{ldo};
        double *s_tri = reinterpret_cast<double *>(smem);
        double *s_h = s_tri + lds.tri();   // [ldo][10]
        double *s_nu = s_h + 10 * ldo;     // [ldo][2]
        double *s_incr = s_nu + 2 * ldo;   // [ldo]
        double *s_gate = s_incr + ldo;     // [ldo + 1]
        int *s_k = reinterpret_cast<int *>(s_gate + ldo + 1); // [ldo] the usable candidate, else -1
        int *s_res = s_k + ldo;                               // [ldo] assoc

        const int b = blockIdx.x, tid = threadIdx.x, lane = tid % PRUNE_WAVE;
        const int L = prune_landmarks(n[b], NP, JOINT_LMAX);
        const int no = min(max(n_obs[b], 0), ldo);
        const double *x = X + (size_t)b * NP;
        const double *Pb = P + (size_t)b * NP * NP;
        const double inf = __builtin_inf();

        // Phase 0: the candidates, clamped
        for (int j = tid; j < ldo; j += JOINT_WG)
        {
                const int k = j < no ? cand[(size_t)b * ldo + j] : -1;
                s_k[j] = k >= 0 && k < L ? k : -1;
                s_res[j] = -1;
                s_incr[j] = inf;
        }
        for (int j = tid; j <= ldo; j += JOINT_WG)
                s_gate[j] = gate_tab ? gate_tab[j] : inf;
        __syncthreads();

        // Phase 1: H and nu of every candidate
        for (int j = tid; j < no; j += JOINT_WG)
        {
                const int k = s_k[j];
                if (k < 0)
                        continue;
                const GateJacobian g = gate_jacobian(x[0], x[1], x[2], x[3 + 2 * k], x[4 + 2 * k]);
                if (!(g.q > 0.0))
                {
                        s_k[j] = -1;
                        continue;
                }
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int i = 0; i < 5; ++i)
                                s_h[10 * j + 5 * r + i] = g.h[r][i];
                const float2 o = *reinterpret_cast<const float2 *>(obs + ((size_t)b * ldo + j) * 2);
                s_nu[2 * j] = (double)o.x - g.rh;
                s_nu[2 * j + 1] = remainder((double)o.y - g.bh, GATE_TWO_PI);
        }
        __syncthreads();

        // Phase 2: C(2i.., 2j..) = H_i P(idx_i, idx_j) H_j^T for the candidate pairs i >= j, R added on the diagonal blocks
        const double rr = prm[b].r_range, rb = prm[b].r_bearing;
        for (int p = tid; p < no * no; p += JOINT_WG)
        {
                const int i = p / no, j = p % no;
                if (j > i || s_k[i] < 0 || s_k[j] < 0)
                        continue;
                const int ri[5] = {0, 1, 2, 3 + 2 * s_k[i], 4 + 2 * s_k[i]};
                const int cj[5] = {0, 1, 2, 3 + 2 * s_k[j], 4 + 2 * s_k[j]};
                const double *hi = s_h + 10 * i, *hj = s_h + 10 * j;
                double t[2][5]; // H_i P(idx_i, idx_j)
#pragma unroll
                for (int c = 0; c < 5; ++c)
                {
                        double t0 = 0.0, t1 = 0.0;
#pragma unroll
                        for (int r = 0; r < 5; ++r)
                        {
                                const int hi_r = max(ri[r], cj[c]), lo_c = min(ri[r], cj[c]); // (the lower triangle alone)
                                const double pv = Pb[(size_t)hi_r * NP + lo_c];
                                t0 = fma(hi[r], pv, t0);
                                t1 = fma(hi[5 + r], pv, t1);
                        }
                        t[0][c] = t0, t[1][c] = t1;
                }
                double B00 = 0.0, B01 = 0.0, B10 = 0.0, B11 = 0.0;
#pragma unroll
                for (int c = 0; c < 5; ++c)
                {
                        B00 = fma(t[0][c], hj[c], B00);
                        B01 = fma(t[0][c], hj[5 + c], B01);
                        B10 = fma(t[1][c], hj[c], B10);
                        B11 = fma(t[1][c], hj[5 + c], B11);
                }
                if (i == j)
                {
                        s_tri[joint_tri(2 * i, 2 * i)] = B00 + rr;
                        s_tri[joint_tri(2 * i + 1, 2 * i)] = B10;
                        s_tri[joint_tri(2 * i + 1, 2 * i + 1)] = B11 + rb;
                }
                else
                {
                        s_tri[joint_tri(2 * i, 2 * j)] = B00;
                        s_tri[joint_tri(2 * i, 2 * j + 1)] = B01;
                        s_tri[joint_tri(2 * i + 1, 2 * j)] = B10;
                        s_tri[joint_tri(2 * i + 1, 2 * j + 1)] = B11;
                }
        }
        __syncthreads();

        // Phase 3: the bordering, wave 0.  Lane l owns the columns l and l + 64 of L_A (in accepted order): col = the row / column of the
        // triangle, diag = L_A(col, col), z = z_A(col)
        if (__builtin_amdgcn_readfirstlane(tid / PRUNE_WAVE) == 0)
        {
                int col[2] = {0, 0};
                double diag[2] = {1.0, 1.0}, z[2] = {0.0, 0.0};
                int m = 0, refused = 0;
                double D2 = 0.0, logdet = 0.0;
                for (int j = 0; j < no; ++j)
                {
                        if (__builtin_amdgcn_readfirstlane(s_k[j]) < 0)
                                continue;
                        const int m2 = 2 * m;
                        double c0[2] = {0.0, 0.0}, c1[2] = {0.0, 0.0};
#pragma unroll
                        for (int s = 0; s < 2; ++s)
                                if (lane + 64 * s < m2)
                                {
                                        c0[s] = s_tri[joint_tri(2 * j, col[s])];
                                        c1[s] = s_tri[joint_tri(2 * j + 1, col[s])];
                                }
                        for (int p = 0; p < min(m2, 64); ++p)
                                joint_solve_step<0>(s_tri, p, lane, m2, col, diag, c0, c1);
                        for (int p = 64; p < m2; ++p)
                                joint_solve_step<1>(s_tri, p - 64, lane, m2, col, diag, c0, c1);
                        // (the registers of a lane without a column hold zeros)
                        const double yy00 = joint_wave_sum(c0[0] * c0[0] + c0[1] * c0[1]);
                        const double yy10 = joint_wave_sum(c1[0] * c0[0] + c1[1] * c0[1]);
                        const double yy11 = joint_wave_sum(c1[0] * c1[0] + c1[1] * c1[1]);
                        const double yz0 = joint_wave_sum(c0[0] * z[0] + c0[1] * z[1]);
                        const double yz1 = joint_wave_sum(c1[0] * z[0] + c1[1] * z[1]);
                        const double T00 = s_tri[joint_tri(2 * j, 2 * j)] - yy00;
                        const double T10 = s_tri[joint_tri(2 * j + 1, 2 * j)] - yy10;
                        const double T11 = s_tri[joint_tri(2 * j + 1, 2 * j + 1)] - yy11;
                        const double t00 = sqrt(T00), t10 = T10 / t00;
                        const double d = T11 - t10 * t10;
                        const double t11 = sqrt(d);
                        const double z0 = (s_nu[2 * j] - yz0) / t00;
                        const double z1 = ((s_nu[2 * j + 1] - yz1) - t10 * z0) / t11;
                        const double dd = z0 * z0 + z1 * z1;
                        const bool usable = T00 > 0.0 && d > 0.0 && __builtin_isfinite(dd);
                        // 0 unusable, 1 refused, 2 accepted: the same in every lane (the sums are), made uniform for the control flow
                        const int verdict = __builtin_amdgcn_readfirstlane(!usable ? 0 : D2 + dd < s_gate[m + 1] ? 2 : 1);
                        if (verdict == 0)
                                continue;
                        if (lane == 0)
                                s_incr[j] = dd;
                        if (verdict == 1)
                        {
                                refused += 1;
                                continue;
                        }
#pragma unroll
                        for (int s = 0; s < 2; ++s)
                        {
                                const int ci = lane + 64 * s;
                                if (ci < m2) // the two new rows of L_A: Y | t00; t10 t11
                                {
                                        s_tri[joint_tri(2 * j, col[s])] = c0[s];
                                        s_tri[joint_tri(2 * j + 1, col[s])] = c1[s];
                                }
                                else if (ci == m2)
                                        col[s] = 2 * j, diag[s] = t00, z[s] = z0;
                                else if (ci == m2 + 1)
                                        col[s] = 2 * j + 1, diag[s] = t11, z[s] = z1;
                        }
                        if (lane == 0)
                        {
                                s_tri[joint_tri(2 * j + 1, 2 * j)] = t10;
                                s_res[j] = s_k[j];
                        }
                        __builtin_amdgcn_wave_barrier(); // the same wave reads the new rows back through LDS
                        D2 += dd;
                        logdet += 2.0 * log(t00 * t11);
                        m += 1;
                }
                if (lane == 0)
                {
                        joint[2 * (size_t)b] = D2;
                        joint[2 * (size_t)b + 1] = logdet;
                        count[2 * (size_t)b] = m;
                        count[2 * (size_t)b + 1] = refused;
                }
        }
        __syncthreads();

        // Phase 4
        for (int j = tid; j < ldo; j += JOINT_WG)
        {
                assoc[(size_t)b * ldo + j] = s_res[j];
                if (incr)
                        incr[(size_t)b * ldo + j] = s_incr[j];
        }
}
} // namespace aslam
