// gate_math.h -- the arithmetic of the individual-compatibility gate (assoc.h has the formulas), as the functions assoc_gate
// (aslam_gate_observations) and the gated replay front end (small_frontend<..., GATED>, small_common.h) both call: one text, one rounding
// sequence, so the two decide alike on the same X and P.  Everything is binary64; the library is compiled with -ffp-contract=off, so the only
// fused operations are the fma calls written here.
#pragma once

#include "device_common.h"

namespace aslam
{
constexpr double GATE_TWO_PI = 6.283185307179586; // 2 pi rounded to binary64

/// the per-landmark terms: predicted range and bearing, the entries of S_k = H_k P5 H_k^T + R and its determinant (0 for an invalid landmark)
struct GateLandmark
{
        double rh, bh, s00, s10, s11, det;
};

/// Landmark k (a0 = 3 + 2k) of a filter with pose (px, py, th) and landmark position (lx, ly); rr, rb: the filter's r_range, r_bearing.
/// plow(i, j), i >= j: entry (i, j) of the lower triangle of P.  Invalid (q, s00 or det not > 0; a NaN fails every comparison): det = 0.
template <typename PLOW>
__device__ __forceinline__ GateLandmark gate_landmark(double px, double py, double th, double lx, double ly, int a0, double rr, double rb, PLOW &&plow)
{
        const int a1 = a0 + 1;
        const double dx = lx - px, dy = ly - py;
        const double q = dx * dx + dy * dy;
        const double rh = sqrt(q);
        const double h[2][5] = {{-dx / rh, -dy / rh, 0.0, dx / rh, dy / rh}, {dy / q, -dx / q, -1.0, -dy / q, dx / q}};
        // P5 from the lower triangle: rows and columns 0, 1, 2, a0, a1 (ascending, so row >= column names a lower-triangle entry)
        const int idx[5] = {0, 1, 2, a0, a1};
        double p[5][5];
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
                for (int j = 0; j <= i; ++j)
                        p[i][j] = p[j][i] = plow(idx[i], idx[j]);
        double t[2][5];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int j = 0; j < 5; ++j)
                {
                        double v = 0.0;
#pragma unroll
                        for (int i = 0; i < 5; ++i)
                                v = fma(h[r][i], p[i][j], v);
                        t[r][j] = v;
                }
        double S00 = 0.0, S10 = 0.0, S11 = 0.0;
#pragma unroll
        for (int j = 0; j < 5; ++j)
        {
                S00 = fma(t[0][j], h[0][j], S00);
                S10 = fma(t[1][j], h[0][j], S10);
                S11 = fma(t[1][j], h[1][j], S11);
        }
        const double s00 = S00 + rr, s11 = S11 + rb, s10 = S10;
        const double det = s00 * s11 - s10 * s10;
        const bool valid = q > 0.0 && s00 > 0.0 && det > 0.0;
        return {rh, atan2(dy, dx) - th, s00, s10, s11, valid ? det : 0.0};
}

/// the Jacobian alone, for the joint test (joint.h): H_k (2 x 5 over the columns 0, 1, 2, a0, a1), q and the predicted reading, from the
/// same expressions as gate_landmark (which keeps its own text: the replay seam's bit-for-bit guarantees hang on its rounding sequence)
struct GateJacobian
{
        double h[2][5];
        double q, rh, bh;
};

__device__ __forceinline__ GateJacobian gate_jacobian(double px, double py, double th, double lx, double ly)
{
        const double dx = lx - px, dy = ly - py;
        const double q = dx * dx + dy * dy;
        const double rh = sqrt(q);
        return {{{-dx / rh, -dy / rh, 0.0, dx / rh, dy / rh}, {dy / q, -dx / q, -1.0, -dy / q, dx / q}}, q, rh, atan2(dy, dx) - th};
}

/// m of observation (r, beta) against a landmark's terms (det > 0 is the caller's test)
__device__ __forceinline__ double gate_pair(double r, double beta, double rh, double bh, double s00, double s10, double s11, double det)
{
        const double v0 = r - rh;
        const double v1 = remainder(beta - bh, GATE_TWO_PI);
        return (s11 * v0 * v0 - 2.0 * s10 * v0 * v1 + s00 * v1 * v1) / det;
}

/// One lane's share of an observation's arg-min: landmarks k = lane, lane + 64, ... < L of a table of six arrays with stride `ld`
/// (rh, bh, s00, s10, s11, det).  A NaN m is skipped; k ascends in a lane, so the first of equal minima stays.
__device__ __forceinline__ void gate_scan_lane(const double *tab, int ld, int L, int lane, double r, double beta, double &best, int &bk)
{
        for (int k = lane; k < L; k += 64)
        {
                const double det = tab[5 * ld + k];
                const double m = gate_pair(r, beta, tab[k], tab[ld + k], tab[2 * ld + k], tab[3 * ld + k], tab[4 * ld + k], det);
                if (det > 0.0 && m < best)
                        best = m, bk = k;
        }
}

/// The 64 partial results of a wave into every lane: the smallest m, ties to the smaller landmark index.  A whole-wave exchange: call it
/// with all 64 lanes active, outside every lane-dependent branch.
__device__ __forceinline__ void gate_wave_argmin(double &best, int &bk)
{
        for (int d = 32; d >= 1; d >>= 1)
        {
                const double om = __shfl_xor(best, d);
                const int ok = __shfl_xor(bk, d);
                if (ok >= 0 && (bk < 0 || om < best || (om == best && ok < bk)))
                        best = om, bk = ok;
        }
}
} // namespace aslam
