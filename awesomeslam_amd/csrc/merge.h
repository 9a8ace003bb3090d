// merge.h -- aslam_merge_landmarks / aslam_select_duplicates (include/aslam_core.h): fuse duplicate landmarks of running filters on the device.
//
// One merge takes landmark j into landmark i < j of a filter.  With a = {3 + 2i, 4 + 2i}, c = {3 + 2j, 4 + 2j}:
//     H (2 x n) = +I2 at columns a, -I2 at columns c        d = X[a] - X[c]
//     W = P H^T = P[:, a] - P[:, c]      (by symmetry W^T is the difference of two contiguous rows of P)
//     S = H P H^T + noise_var I2         X <- X - W S^-1 d        P <- P - W S^-1 W^T
// and landmark j is removed; i keeps its index and its Z entries.  The pairs of a filter are taken in ascending j, MERGE_ROUND = 8 per round,
// the k pairs of a round jointly (2k <= 16 constraint rows):
//     S (2k x 2k),  Lc = chol(S),  V = Lc^-1 W^T (2k x n),  y = Lc^-1 d,  X -= V^T y,  P -= V^T V
// Rounds run one after another; a later round reads the P the earlier one left.  Everything is binary64 (P is, in every context).
//
//   merge_plan       validate a row of `into`, list the pairs in ascending j, write the 0/1 removal mask row prune_map will read, report
//   merge_gain       per round: W^T gathered from P, S, its Cholesky factor, V into the staging [B][16][NP] (unused rows zero), X update.
//                    A pivot <= 0 or not finite stops the filter: stop flag, V zeroed, this round's and all later pairs taken out of the mask
//   merge_downdate   P(tile) -= V[:, rows]^T V[:, cols] on the lower-triangle 64 x 64 tiles (v_mfma_f64_16x16x4_f64): reads the lower triangle,
//                    stores each value and its mirror image (P stays exactly symmetric), the diagonal once.  Filters without pairs in the
//                    round are not written
//   merge_sightings  the sighting record of every merged pair fused into its root, before the compaction of aslam_remove_landmarks
//   merge_select     partner[j] = the i < j of smallest Mahalanobis distance inside the gates; merge_resolve turns partners into `into`
//
// No inter-workgroup waits, no spins; every loop is bounded by sizes the host validated (NP, ld) or that merge_plan clamped to them.
#pragma once

#include "prune.h"

namespace aslam
{
constexpr int MERGE_ROUND = 8;             // pairs per round
constexpr int MERGE_K = 2 * MERGE_ROUND;   // constraint rows per round: the K of the downdate
constexpr int MERGE_WG = 256;
constexpr int MERGE_TILE = 64;             // the downdate's tile: 4 waves x (16 x 64)

/// what merge_plan reports per filter, for the one copy to the host
struct MergeMeta
{
        int32_t count; // pairs of the filter
        int32_t bad_j; // -1, or the first landmark whose entry is refused
        int32_t bad_i; // its entry
        int32_t L;     // landmarks of the filter
};

/// grid: filters, block: one wave.  into[b][j] = i merges j into i; -1 keeps j.  Refused: i < -1, i >= j, into[i] != -1.  Entries at or beyond
/// the landmark count are not read.  pi / pj [b][ldm]: the pairs in ascending j; mask [b][ldm]: 1 where j is merged away, 0 elsewhere up to ldm.
__global__ __launch_bounds__(PRUNE_WAVE) void merge_plan(const int32_t *__restrict__ into, int ld, const int *__restrict__ n, int NP, int ldm,
                                                         int32_t *__restrict__ pi, int32_t *__restrict__ pj, uint8_t *__restrict__ mask,
                                                         int32_t *__restrict__ stop, MergeMeta *__restrict__ meta)
{
        const int b = blockIdx.x, lane = threadIdx.x;
        const int L = prune_landmarks(n[b], NP, ld < ldm ? ld : ldm);
        const int32_t *row = into + (size_t)b * ld;
        int32_t *qi = pi + (size_t)b * ldm, *qj = pj + (size_t)b * ldm;
        uint8_t *m = mask + (size_t)b * ldm;
        int count = 0, bad_j = -1, bad_i = 0;
        for (int j0 = 0; j0 < ldm; j0 += PRUNE_WAVE) // (ldm is the same in every lane: all of them reach the ballots)
        {
                const int j = j0 + lane;
                const int i = j < L ? row[j] : -1;
                const bool bad = i != -1 && (i < 0 || i >= j || row[i] != -1); // (row[i] is read only where 0 <= i < j < L)
                const bool pair = i != -1 && !bad;
                const unsigned long long bv = __ballot(bad), pv = __ballot(pair);
                if (bv && bad_j < 0)
                {
                        const int first = __ffsll((long long)bv) - 1;
                        bad_j = j0 + first;
                        bad_i = __shfl(i, first);
                }
                if (pair)
                {
                        const int k = count + __popcll(pv & ((1ull << lane) - 1ull));
                        qi[k] = i;
                        qj[k] = j;
                }
                if (j < ldm)
                        m[j] = pair ? 1 : 0;
                count += __popcll(pv);
        }
        if (lane == 0)
        {
                meta[b] = MergeMeta{count, bad_j, bad_i, L};
                stop[b] = 0;
        }
}

/// grid: filters, block: MERGE_WG; round r.  V [b][MERGE_K][NP] is written whole by every filter that has pairs in the round (rows from 2k on
/// and columns from n on are zero); filters without, or stopped ones, return at once.
__global__ __launch_bounds__(MERGE_WG) void merge_gain(double *__restrict__ X, const double *__restrict__ P, const int *__restrict__ n, int NP, int ldm,
                                                       const int32_t *__restrict__ pi, const int32_t *__restrict__ pj,
                                                       const MergeMeta *__restrict__ meta, int round, double noise_var, double *__restrict__ V,
                                                       uint8_t *__restrict__ mask, int32_t *__restrict__ stop)
{
        __shared__ double S[MERGE_K][MERGE_K + 1];
        __shared__ double y[MERGE_K];
        __shared__ int ra[MERGE_K], rc[MERGE_K];
        __shared__ int failed;
        const int b = blockIdx.x, tid = threadIdx.x;
        const int count = meta[b].count, p0 = round * MERGE_ROUND;
        if (p0 >= count || stop[b])
                return;
        const int k = min(count - p0, MERGE_ROUND), m = 2 * k;
        const int nb = min(max(n[b], 0), NP);
        const int H = NP / 2; // (landmark i holds rows 3 + 2i, 4 + 2i: below NP for i <= H - 3)
        double *x = X + (size_t)b * NP;
        const double *Pb = P + (size_t)b * NP * NP;
        double *Vb = V + (size_t)b * MERGE_K * NP;
        if (tid < MERGE_K)
        {
                const int p = p0 + tid / 2;
                const bool on = tid < m;
                const int i = on ? min(max(pi[(size_t)b * ldm + p], 0), H - 3) : 0, j = on ? min(max(pj[(size_t)b * ldm + p], 0), H - 3) : 0;
                ra[tid] = 3 + 2 * i + (tid & 1);
                rc[tid] = 3 + 2 * j + (tid & 1);
        }
        if (tid == 0)
                failed = 0;
        __syncthreads();
        // W^T: the difference of two rows of P; zero beyond the constraint rows and beyond the state
        for (int e = tid; e < MERGE_K * NP; e += MERGE_WG)
        {
                const int q = e / NP, col = e - q * NP;
                Vb[e] = (q < m && col < nb) ? Pb[(size_t)ra[q] * NP + col] - Pb[(size_t)rc[q] * NP + col] : 0.0;
        }
        __syncthreads(); // (workgroup-scope: the W^T this workgroup stored is what it loads below)
        {
                const int q = tid / MERGE_K, s = tid % MERGE_K; // MERGE_WG == MERGE_K * MERGE_K
                double v = (q == s) ? 1.0 : 0.0;                // identity beyond the constraint rows: the solve leaves zeros there
                if (q < m && s < m)
                {
                        v = Vb[(size_t)q * NP + ra[s]] - Vb[(size_t)q * NP + rc[s]];
                        if (q == s)
                                v += noise_var;
                }
                S[q][s] = v;
                if (tid < MERGE_K)
                        y[tid] = tid < m ? x[ra[tid]] - x[rc[tid]] : 0.0;
        }
        __syncthreads();
        if (tid == 0)
        {
                // Cholesky of the lower triangle in place, then y = Lc^-1 d: 16 x 16 at the most
                for (int c = 0; c < m && !failed; ++c)
                {
                        double piv = S[c][c];
                        for (int t = 0; t < c; ++t)
                                piv = fma(-S[c][t], S[c][t], piv);
                        if (!(piv > 0.0) || !isfinite(piv))
                        {
                                failed = 1;
                                break;
                        }
                        const double l = sqrt(piv);
                        S[c][c] = l;
                        for (int r = c + 1; r < m; ++r)
                        {
                                double v = S[r][c];
                                for (int t = 0; t < c; ++t)
                                        v = fma(-S[r][t], S[c][t], v);
                                S[r][c] = v / l;
                        }
                }
                for (int q = 0; q < m && !failed; ++q)
                {
                        double v = y[q];
                        for (int t = 0; t < q; ++t)
                                v = fma(-S[q][t], y[t], v);
                        y[q] = v / S[q][q];
                }
        }
        __syncthreads();
        if (failed)
        {
                for (int e = tid; e < MERGE_K * NP; e += MERGE_WG)
                        Vb[e] = 0.0;
                for (int p = p0 + tid; p < count; p += MERGE_WG)
                        mask[(size_t)b * ldm + min(max(pj[(size_t)b * ldm + p], 0), ldm - 1)] = 0;
                if (tid == 0)
                        stop[b] = 1;
                return;
        }
        // V = Lc^-1 W^T column by column (forward substitution in registers), X -= V^T y
        for (int col = tid; col < nb; col += MERGE_WG)
        {
                double v[MERGE_K];
#pragma unroll
                for (int q = 0; q < MERGE_K; ++q)
                {
                        double t = Vb[(size_t)q * NP + col];
#pragma unroll
                        for (int s = 0; s < q; ++s)
                                t = fma(-S[q][s], v[s], t);
                        v[q] = t / S[q][q];
                }
                double dx = 0.0;
#pragma unroll
                for (int q = 0; q < MERGE_K; ++q)
                {
                        Vb[(size_t)q * NP + col] = v[q];
                        dx = fma(v[q], y[q], dx);
                }
                x[col] -= dx;
        }
}

/// grid: (lower-triangle tiles of MERGE_TILE x MERGE_TILE, filters), block: MERGE_WG = 4 waves, a wave per 16-row strip of the tile.  Per 16 x 16
/// block 4 issues of v_mfma_f64_16x16x4_f64 (K = MERGE_K), the operands straight from V (16 rows per filter: L2-resident), the accumulator
/// loaded with the lower-triangle entries of P; each new value is stored, and its mirror image row-wise after a transpose through LDS, the
/// diagonal once.  About 12 bytes move per element of P (the lower triangle read, both triangles written) for 32 flops: the kernel waits on
/// memory.  (Measured against a plain-FMA form, a 4 x 4 block per thread with V staged in LDS: profiles/merge.md.)
__global__ __launch_bounds__(MERGE_WG) void merge_downdate(double *__restrict__ P, const int *__restrict__ n, int NP, const MergeMeta *__restrict__ meta,
                                                           int round, const double *__restrict__ V, const int32_t *__restrict__ stop)
{
        __shared__ double tt[MERGE_WG / 64][16][17];
        const int b = blockIdx.y, tid = threadIdx.x;
        if (round * MERGE_ROUND >= meta[b].count || stop[b])
                return;
        const int nb = min(max(n[b], 0), NP);
        const TriIndex tile = tri_index((int)blockIdx.x);
        const int r0 = tile.i * MERGE_TILE, c0 = tile.j * MERGE_TILE;
        if (r0 >= nb)
                return;
        const int wave = tid / 64, lane = tid % 64, li = lane % 16, lg = lane / 16;
        const double *Vb = V + (size_t)b * MERGE_K * NP;
        double *Pb = P + (size_t)b * NP * NP;
        const int rb = r0 + 16 * wave;
        double a[4];
#pragma unroll
        for (int s = 0; s < 4; ++s)
                a[s] = rb + li < NP ? -Vb[(size_t)(lg + 4 * s) * NP + rb + li] : 0.0;
        for (int sc = 0; sc < MERGE_TILE / 16; ++sc) // (the same trip count in every wave: the barriers below are uniform)
        {
                const int cb = c0 + 16 * sc;
                d4 t;
                double bv[4];
#pragma unroll
                for (int s = 0; s < 4; ++s)
                        bv[s] = cb + li < NP ? Vb[(size_t)(lg + 4 * s) * NP + cb + li] : 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r)
                {
                        const int row = rb + lg + 4 * r, col = cb + li;
                        t[r] = (row < nb && col <= row) ? Pb[(size_t)row * NP + col] : 0.0;
                }
#pragma unroll
                for (int s = 0; s < 4; ++s)
                        t = mfma_f64(a[s], bv[s], t);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                {
                        const int row = rb + lg + 4 * r, col = cb + li;
                        if (row < nb && col <= row)
                                Pb[(size_t)row * NP + col] = t[r];
                        tt[wave][lg + 4 * r][li] = t[r];
                }
                __syncthreads();
#pragma unroll
                for (int r = 0; r < 4; ++r)
                {
                        const int row = rb + li, col = cb + lg + 4 * r; // the element whose mirror image this lane stores
                        if (row < nb && col < row)
                                Pb[(size_t)col * NP + row] = tt[wave][li][lg + 4 * r];
                }
                __syncthreads();
        }
}

/// grid: filters, block: one wave; behind the last round, in front of the compaction.  For every pair still in the mask: hits[i] += hits[j],
/// seen[i] = whichever of the two has the smaller age (clock - seen, unsigned 32-bit).  With t = seen - clock - 1 = ~age the smaller age is the
/// larger t: the record goes to t, the pairs fold with atomics (several leaves may share a root; a leaf is never a root), and it comes back.
__global__ __launch_bounds__(PRUNE_WAVE) void merge_sightings(const uint32_t *__restrict__ clock, uint32_t *lm_seen, uint32_t *lm_hits, int NP, int ldm,
                                                              const int32_t *__restrict__ pi, const int32_t *__restrict__ pj,
                                                              const MergeMeta *__restrict__ meta, const uint8_t *__restrict__ mask)
{
        const int b = blockIdx.x, lane = threadIdx.x;
        const MergeMeta mm = meta[b];
        if (mm.count <= 0)
                return;
        const int H = NP / 2;
        const int L = min(max(mm.L, 0), H), count = min(mm.count, ldm);
        uint32_t *seen = lm_seen + (size_t)b * H, *hits = lm_hits + (size_t)b * H;
        const uint32_t off = clock[b] + 1u;
        for (int l = lane; l < L; l += PRUNE_WAVE)
                seen[l] -= off;
        __syncthreads();
        for (int p = lane; p < count; p += PRUNE_WAVE)
        {
                const int i = min(max(pi[(size_t)b * ldm + p], 0), H - 1), j = min(max(pj[(size_t)b * ldm + p], 0), H - 1);
                if (j < ldm && mask[(size_t)b * ldm + j])
                {
                        atomicMax(&seen[i], seen[j]);
                        atomicAdd(&hits[i], hits[j]);
                }
        }
        __syncthreads();
        for (int l = lane; l < L; l += PRUNE_WAVE)
                seen[l] += off;
}

/// The gated distance of the candidate (i, j), i < j, of one filter; binary64, every operation rounded on its own, lower-triangle entries only:
///     dx = X[3+2i] - X[3+2j]    dy = X[4+2i] - X[4+2j]    r2 = dx*dx + dy*dy                       candidate needs r2 <= maxd2
///     s00 = ((P[a0][a0] + P[c0][c0]) - P[c0][a0]) - P[c0][a0]
///     s11 = ((P[a1][a1] + P[c1][c1]) - P[c1][a1]) - P[c1][a1]
///     s10 = ((P[a1][a0] + P[c1][c0]) - P[c1][a0]) - P[c0][a1]
///     det = s00*s11 - s10*s10                                                                      s00 > 0 and det > 0
///     t1 = (s10*dx)*dy    num = (((s11*dx)*dx) - (t1 + t1)) + ((s00*dy)*dy)    m = num / det       m < gate
/// with a0 = 3 + 2i, a1 = a0 + 1, c0 = 3 + 2j, c1 = c0 + 1.  Returns false where a condition fails (a NaN fails every comparison).
__device__ __forceinline__ bool merge_distance(const double *__restrict__ x, const double *__restrict__ Pb, int NP, int i, int j, double maxd2,
                                               double gate, double *m_out)
{
        const int a0 = 3 + 2 * i, a1 = a0 + 1, c0 = 3 + 2 * j, c1 = c0 + 1;
        const double dx = __dsub_rn(x[a0], x[c0]), dy = __dsub_rn(x[a1], x[c1]);
        const double r2 = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy));
        if (!(r2 <= maxd2))
                return false;
        const double *pa0 = Pb + (size_t)a0 * NP, *pa1 = Pb + (size_t)a1 * NP, *pc0 = Pb + (size_t)c0 * NP, *pc1 = Pb + (size_t)c1 * NP;
        const double s00 = __dsub_rn(__dsub_rn(__dadd_rn(pa0[a0], pc0[c0]), pc0[a0]), pc0[a0]);
        const double s11 = __dsub_rn(__dsub_rn(__dadd_rn(pa1[a1], pc1[c1]), pc1[a1]), pc1[a1]);
        const double s10 = __dsub_rn(__dsub_rn(__dadd_rn(pa1[a0], pc1[c0]), pc1[a0]), pc0[a1]);
        const double det = __dsub_rn(__dmul_rn(s00, s11), __dmul_rn(s10, s10));
        if (!(s00 > 0.0) || !(det > 0.0))
                return false;
        const double t1 = __dmul_rn(__dmul_rn(s10, dx), dy);
        const double num = __dadd_rn(__dsub_rn(__dmul_rn(__dmul_rn(s11, dx), dx), __dadd_rn(t1, t1)), __dmul_rn(__dmul_rn(s00, dy), dy));
        const double m = __ddiv_rn(num, det);
        *m_out = m;
        return m < gate;
}

/// grid: (ceil(ld / 4), filters), block: 4 waves; a wave per j, lanes over i < j, wave-level argmin with ties to the smaller i.
/// partner[b][j] = that i, or -1 (no candidate, or j at or beyond the landmark count) up to ld.
__global__ __launch_bounds__(MERGE_WG) void merge_select(const double *__restrict__ X, const double *__restrict__ P, const int *__restrict__ n, int NP,
                                                         const double *__restrict__ maxd2, const double *__restrict__ gate, int32_t *__restrict__ partner,
                                                         int ld)
{
        const int b = blockIdx.y, lane = threadIdx.x % PRUNE_WAVE;
        const int j = blockIdx.x * (MERGE_WG / PRUNE_WAVE) + threadIdx.x / PRUNE_WAVE;
        if (j >= ld)
                return;
        const int L = prune_landmarks(n[b], NP, ld);
        const double *x = X + (size_t)b * NP;
        const double *Pb = P + (size_t)b * NP * NP;
        const double lim = maxd2[b], g = gate[b];
        double best = 0.0;
        int bi = -1;
        if (j < L)
                for (int i = lane; i < j; i += PRUNE_WAVE)
                {
                        double m;
                        if (merge_distance(x, Pb, NP, i, j, lim, g, &m) && (bi < 0 || m < best))
                                best = m, bi = i;
                }
        for (int d = PRUNE_WAVE / 2; d >= 1; d >>= 1)
        {
                const double om = __shfl_xor(best, d);
                const int oi = __shfl_xor(bi, d);
                if (oi >= 0 && (bi < 0 || om < best || (om == best && oi < bi)))
                        best = om, bi = oi;
        }
        if (lane == 0)
                partner[(size_t)b * ld + j] = bi;
}

/// grid: filters, block: one wave.  The conservative rule: into[j] = partner[j] where the partner itself has none, else -1 (a landmark whose
/// partner is about to be merged waits for the next call), so every selected pair is directly gated and no chain is ever written.
__global__ __launch_bounds__(PRUNE_WAVE) void merge_resolve(const int32_t *__restrict__ partner, int32_t *__restrict__ into, int ld)
{
        const int b = blockIdx.x;
        const int32_t *p = partner + (size_t)b * ld;
        for (int j = threadIdx.x; j < ld; j += PRUNE_WAVE)
        {
                const int i = p[j];
                into[(size_t)b * ld + j] = (i >= 0 && i < j && p[i] == -1) ? i : -1;
        }
}
} // namespace aslam
