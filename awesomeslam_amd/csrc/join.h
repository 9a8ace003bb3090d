// join.h -- aslam_join_maps (include/aslam_snapshot.h): put the landmarks of a snapshot record, with their covariance block, behind the state
// of a running filter on the device.
//
//   join_pack      one complete record of snapshot.h per joined filter: the filter's OWN record, X, Z and P extended by the selected landmarks
//                  of the source record, moved into the filter's frame -- what a snapshot would hold had the filter held them
//   sight_extend   the sighting record of every joined filter, extended as aslam_grow extends it (last_seen = clock, hits = 0)
//
// The records then go through snapshot_unpack, unchanged, into their own slots, as the records of prune.h do: the slot becomes a fresh one of
// the larger dimension, and the zero padding, the cleared scratch and every kernel family's layout stay that one piece of code.  The lists
// and headers of the record come from snapshot.h's one writer; join_pack keeps the loop of record_pack as a kernel of its own, since as a
// source of that template it needed more registers and scratch (profiles/record_writer.md).  It takes every size from its descriptors, which the host wrote after validation; it reads nothing of the source record but the X and P
// entries of the selected landmarks (the selected-index list holds indices below the record's landmark count by construction).
#pragma once

#include "prune.h"

namespace aslam
{
/// one joined filter of a launch, next to its SnapDesc (whose n is the NEW dimension n_A + 2m)
struct JoinDesc
{
        int64_t src_off;                // the source record in the source blob
        int32_t n_A, m, ld_B, idx_off;  // the filter's dimension, landmarks joined, row length of the source's P, first entry of its index list
        double c, s, tx, ty;            // cos(phi), sin(phi) as the host took them, t
        double cov[9];                  // covariance of (tx, ty, phi)
};
static_assert(sizeof(JoinDesc) == 128, "16-byte multiples: the descriptors are read as they lie in the staging block");

/// the wrap of device_common.h's normalizeAngle (tools.h:44-50), in binary64
__device__ __forceinline__ double join_wrap(double theta)
{
        constexpr double PI = 3.14159265358979323846, TWO_PI = 2.0 * PI;
        double ret = fmod(theta, TWO_PI);
        ret = ret > PI ? ret - TWO_PI : ret;
        ret = ret < -PI ? ret + TWO_PI : ret;
        return ret;
}

/// the source record of one descriptor: its X and its P (row length ld_B), and the selected landmarks
struct JoinSrc
{
        const double *X, *P;
        const int32_t *idx;
};

/// coordinate i (0: x, 1: y) of selected landmark p in the destination frame: t + R l, left to right
__device__ __forceinline__ double join_point(const JoinDesc &j, const JoinSrc &s, int p, int i)
{
        const int k = s.idx[p];
        const double lx = s.X[3 + 2 * k], ly = s.X[4 + 2 * k];
        return i == 0 ? j.tx + j.c * lx - j.s * ly : j.ty + j.s * lx + j.c * ly;
}

/// entry (a, b), a >= b, of the new diagonal block P' (2m x 2m): block (p, q) = (a / 2, b / 2), p >= q, is R B_pq R^T + G_p cov G_q^T with
/// B_pq read from the LOWER triangle of the source's P (on the diagonal block the entry above the diagonal is the one below it).  The caller
/// mirrors: entry (b, a) is this very value.
__device__ __forceinline__ double join_entry(const JoinDesc &j, const JoinSrc &s, int a, int b)
{
        const int p = a >> 1, i = a & 1, q = b >> 1, k = b & 1;
        const int kp = s.idx[p], kq = s.idx[q];
        const size_t ld = (size_t)j.ld_B;
        const double *r0 = s.P + (size_t)(3 + 2 * kp) * ld + 3 + 2 * kq, *r1 = r0 + ld;
        const double b00 = r0[0], b10 = r1[0], b11 = r1[1], b01 = p == q ? b10 : r0[1];
        // rows i and k of R = [[c, -s], [s, c]]
        const double ri0 = i ? j.s : j.c, ri1 = i ? j.c : -j.s, rk0 = k ? j.s : j.c, rk1 = k ? j.c : -j.s;
        const double t0 = ri0 * b00 + ri1 * b10, t1 = ri0 * b01 + ri1 * b11;
        const double rot = t0 * rk0 + t1 * rk1;
        // row i of G_p = e_i + g_p e_2 and row k of G_q = e_k + g_q e_2, g = (-s lx - c ly, c lx - s ly)
        const double px = s.X[3 + 2 * kp], py = s.X[4 + 2 * kp], qx = s.X[3 + 2 * kq], qy = s.X[4 + 2 * kq];
        const double gp = i ? j.c * px - j.s * py : -j.s * px - j.c * py, gq = k ? j.c * qx - j.s * qy : -j.s * qx - j.c * qy;
        const double uk = j.cov[3 * i + k] + gp * j.cov[6 + k], u2 = j.cov[3 * i + 2] + gp * j.cov[8];
        return rot + (uk + u2 * gq);
}

/// entry (r, col) of the joined filter's P: the old block as it is, +0.0 in both cross blocks, P' behind them; 0.0 in the pad column
__device__ __forceinline__ double join_P(const JoinDesc &j, const JoinSrc &s, const double *__restrict__ Pin, size_t NP, int n, int r, int col)
{
        if (col >= n || (r < j.n_A) != (col < j.n_A))
                return 0.0;
        if (r < j.n_A)
                return Pin[(size_t)r * NP + col];
        const int a = r - j.n_A, b = col - j.n_A;
        return a >= b ? join_entry(j, s, a, b) : join_entry(j, s, b, a);
}

/// The grid and the loop of record_pack (row chunks x records).  d.n of a descriptor is the NEW dimension.  The new columns start at the odd index n_A:
/// a double2 at an even column straddles the old state and the first new landmark, and later two landmarks, so each half has a source of
/// its own (as in PruneSrc); pairs that lie wholly in the old block are moved 16 bytes at a time.
__global__ __launch_bounds__(SNAP_WG) void join_pack(SnapCtx c, const SnapDesc *__restrict__ desc, const JoinDesc *__restrict__ jdesc,
                                                     const int32_t *__restrict__ idx, int count, uint32_t filter, uint64_t total,
                                                     const char *__restrict__ src, char *__restrict__ blob)
{
        const int tid = threadIdx.x;
        const size_t NP = (size_t)c.NP;
        for (int f = blockIdx.y; f < count; f += gridDim.y)
        {
                const SnapDesc d = desc[f];
                const JoinDesc j = jdesc[f];
                const int n = d.n, ld = n + 1, h = ld / 2, nA = j.n_A;
                const size_t slot = (size_t)d.slot;
                JoinSrc s;
                s.X = reinterpret_cast<const double *>(src + j.src_off + 64);
                s.P = s.X + 2 * (size_t)j.ld_B;
                s.idx = idx + j.idx_off;
                char *rec = blob + d.off;
                double2 *Pout = reinterpret_cast<double2 *>(rec + 64 + 16 * (size_t)ld);
                const double *Pin = c.P + slot * NP * NP;
                const int units = n * h;
                for (int i = blockIdx.x * SNAP_WG + tid; i < units; i += gridDim.x * SNAP_WG)
                {
                        const int r = i / h, q = i - r * h;
                        double2 v;
                        if (r < nA && 2 * q + 1 < nA)
                                v = *reinterpret_cast<const double2 *>(Pin + (size_t)r * NP + 2 * q);
                        else
                        {
                                v.x = join_P(j, s, Pin, NP, n, r, 2 * q);
                                v.y = join_P(j, s, Pin, NP, n, r, 2 * q + 1);
                        }
                        Pout[i] = v;
                }
                if (blockIdx.x != 0)
                        continue;
                // workgroup 0 of the record: X, Z, then everything else
                const double *xa = c.X + slot * NP, *za = c.Z + slot * NP;
                const double ax = xa[0], ay = xa[1], ath = xa[2];
                double *Xout = reinterpret_cast<double *>(rec + 64), *Zout = Xout + ld;
                for (int i = tid; i < ld; i += SNAP_WG)
                {
                        double x = 0.0, z = 0.0;
                        if (i < nA)
                                x = xa[i], z = za[i];
                        else if (i < n)
                        {
                                const int p = (i - nA) >> 1;
                                const double dx = join_point(j, s, p, 0) - ax, dy = join_point(j, s, p, 1) - ay;
                                x = join_point(j, s, p, (i - nA) & 1);
                                // the reading the filter's own pose predicts: zero innovation until the landmark is sighted
                                z = (i - nA) & 1 ? join_wrap(atan2(dy, dx) - ath) : sqrt(dx * dx + dy * dy);
                        }
                        Xout[i] = x;
                        Zout[i] = z;
                }
                snap_write_lists_and_headers(c, d, f, count, filter, total, rec, blob);
        }
}

/// grid: joined filters, block: one wave; launched behind the unpack of aslam_join_maps.  The new landmarks enter the record as aslam_grow
/// enters them; the clock and the records of the old landmarks stay (a restore clears both, a join must not: hence a kernel of its own).
__global__ __launch_bounds__(PRUNE_WAVE) void sight_extend(const SnapDesc *__restrict__ desc, const JoinDesc *__restrict__ jdesc, int NP,
                                                           const uint32_t *__restrict__ clock, uint32_t *__restrict__ lm_seen,
                                                           uint32_t *__restrict__ lm_hits)
{
        const size_t slot = (size_t)desc[blockIdx.x].slot;
        const JoinDesc j = jdesc[blockIdx.x];
        const int H = NP / 2;
        const int L_old = min(max((j.n_A - 3) / 2, 0), H), L_new = min(L_old + max(j.m, 0), H);
        const uint32_t clk = clock[slot];
        for (int i = L_old + threadIdx.x; i < L_new; i += PRUNE_WAVE)
                lm_seen[slot * H + i] = clk, lm_hits[slot * H + i] = 0u;
}
} // namespace aslam
