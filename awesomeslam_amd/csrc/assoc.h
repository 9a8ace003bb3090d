// assoc.h -- aslam_gate_observations (include/aslam_core.h): Mahalanobis-gated data association on the device.
//
// Individual compatibility: the innovation of observation (r, beta) against landmark k of a filter, weighed by S_k = H_k P H_k^T + R and
// compared with a chi-square point.  With a0 = 3 + 2k, a1 = a0 + 1:
//     dx = X[a0] - X[0]   dy = X[a1] - X[1]   q = dx^2 + dy^2   rh = sqrt(q)   bh = atan2(dy, dx) - X[2]
//     H_k (2 x 5 over the columns 0, 1, 2, a0, a1):  range row (-dx/rh, -dy/rh, 0, dx/rh, dy/rh),  bearing row (dy/q, -dx/q, -1, -dy/q, dx/q)
//     S = H_k P5 H_k^T     s00 = S00 + r_range   s11 = S11 + r_bearing   s10 = S10   det = s00 s11 - s10^2
//     v0 = r - rh          v1 = remainder(beta - bh, 2 pi)                m = (s11 v0^2 - 2 s10 v0 v1 + s00 v1^2) / det
// Everything is binary64 (P is, in every context); only lower-triangle entries of P are read.
//
//   assoc_gate   one workgroup per filter.  Phase 1, lanes over landmarks: rh, bh, s00, s10, s11, det of every landmark into LDS (at most 542
//                landmarks x 6 doubles); an invalid landmark (q, s00 or det not > 0; a NaN fails every comparison) is stored with det = 0.
//                Phase 2, a wave per observation, lanes over landmarks, wave-level arg-min with ties to the smaller landmark index.
//
// The kernel writes assoc and mdist and nothing a filter owns.  Every loop is bounded by sizes the host validated (ldo) or that are clamped
// here to what a padded row holds (the landmark count).  The whole-wave exchange sits outside every lane-dependent branch.
#pragma once

#include "gate_math.h"
#include "prune.h"

namespace aslam
{
constexpr int ASSOC_WG = 256;     // 4 waves
constexpr int ASSOC_LMAX = 542;   // landmarks of the largest state a context accepts: (1087 - 3) / 2
constexpr int ASSOC_LPAD = 544;
static_assert(PRUNE_WAVE == 64, "gate_math.h deals landmarks to the 64 lanes of a wave");

/// grid: filters, block: ASSOC_WG.  obs [batch][ldo][2] f32 (range, bearing), n_obs, gate [batch]; assoc [batch][ldo] i32, mdist [batch][ldo]
/// f64 or null.  assoc[b][j] = the valid landmark of smallest m if that m < gate[b], else -1; mdist[b][j] = that smallest m, +inf without a
/// valid landmark; entries j >= n_obs[b] get -1 and +inf.
__global__ __launch_bounds__(ASSOC_WG) void assoc_gate(const double *__restrict__ X, const double *__restrict__ P, const int *__restrict__ n, int NP,
                                                       const aslam_params *__restrict__ prm, const float *__restrict__ obs, int ldo,
                                                       const int32_t *__restrict__ n_obs, const double *__restrict__ gate,
                                                       int32_t *__restrict__ assoc, double *__restrict__ mdist)
{
        __shared__ double s_tab[6 * ASSOC_LPAD]; // rh, bh, s00, s10, s11, det (gate_math.h: the arithmetic is shared with the replay front end)
        const int b = blockIdx.x, tid = threadIdx.x, lane = tid % PRUNE_WAVE;
        const int L = prune_landmarks(n[b], NP, ASSOC_LMAX);
        const double *x = X + (size_t)b * NP;
        const double *Pb = P + (size_t)b * NP * NP;
        const double px = x[0], py = x[1], th = x[2];
        const double rr = prm[b].r_range, rb = prm[b].r_bearing;
        for (int k = tid; k < L; k += ASSOC_WG)
        {
                const int a0 = 3 + 2 * k;
                const GateLandmark g = gate_landmark(px, py, th, x[a0], x[a0 + 1], a0, rr, rb, [&](int i, int j) { return Pb[(size_t)i * NP + j]; });
                s_tab[k] = g.rh;
                s_tab[ASSOC_LPAD + k] = g.bh;
                s_tab[2 * ASSOC_LPAD + k] = g.s00;
                s_tab[3 * ASSOC_LPAD + k] = g.s10;
                s_tab[4 * ASSOC_LPAD + k] = g.s11;
                s_tab[5 * ASSOC_LPAD + k] = g.det;
        }
        __syncthreads();
        const int wave = __builtin_amdgcn_readfirstlane(tid / PRUNE_WAVE);
        const int no = min(max(n_obs[b], 0), ldo);
        const double g = gate[b];
        const double inf = __builtin_inf();
        for (int j = wave; j < ldo; j += ASSOC_WG / PRUNE_WAVE) // (j is the same in every lane of a wave)
        {
                double best = inf;
                int bk = -1;
                if (j < no)
                {
                        const float2 o = *reinterpret_cast<const float2 *>(obs + ((size_t)b * ldo + j) * 2);
                        gate_scan_lane(s_tab, ASSOC_LPAD, L, lane, (double)o.x, (double)o.y, best, bk);
                }
                gate_wave_argmin(best, bk);
                if (lane == 0)
                {
                        assoc[(size_t)b * ldo + j] = best < g ? bk : -1;
                        if (mdist)
                                mdist[(size_t)b * ldo + j] = best;
                }
        }
}
} // namespace aslam
