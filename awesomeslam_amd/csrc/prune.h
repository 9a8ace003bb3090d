// prune.h -- aslam_remove_landmarks / aslam_select_beyond (include/aslam_core.h): take landmarks out of running filters on the device.
//
//   prune_select_beyond   mask[b][i] = 1 where landmark i of filter b lies farther than max_range[b] from the filter's own pose
//   prune_map             mask row + n of the filter -> the survivor list src[b][0 .. n_new) (source index of every kept row) and n_new[b]
//   PruneSrc              the source of record_pack (snapshot.h) that gathers X, Z and P through src: one complete record per pruned filter,
//                         what a snapshot would hold had the filter never held the removed landmarks
//
//   prune_select_stale    mask[b][i] = 1 where landmark i of filter b was last sighted more than max_age[b] callbacks ago (the sighting record)
//   sight_compact         the sighting record of every filter that lost something, moved in place through prune_map's survivor list
//   sight_clear           clock and sighting record of restored slots to zero
//
// The records then go through snapshot_unpack, unchanged, into their own slots: a slot whose dimension shrank is made a FRESH one exactly as
// a restored slot is (zero padding, cleared scratch -- see the top of snapshot.h), and no second piece of code has to know what "fresh" means.
// The record's lists and headers are written by snapshot.h's one writer.  record_pack takes every size from its descriptors, which the host
// validated; src holds indices below the padded dimension by construction (prune_map clamps the landmark count it reads to what the row holds).
#pragma once

#include "snapshot.h"

namespace aslam
{
constexpr int PRUNE_WAVE = 64;

/// what prune_map reports per filter, for the one copy to the host: FilterMeta (snapshot.h) with n_new where the flags are, which no prune reads
struct PruneMeta
{
        int32_t n, n_new, sens_n, wait_n;
};

/// landmarks of a filter of dimension n, clamped to what a padded row of NP and a mask row of ld can name
__device__ __forceinline__ int prune_landmarks(int n, int NP, int ld)
{
        int L = (n - 3) / 2;
        const int cap = (NP - 3) / 2;
        L = L > cap ? cap : L;
        L = L > ld ? ld : L;
        return L < 0 ? 0 : L;
}

/// grid: filters, block: one wave.  r2[b] = max_range[b]^2 (binary64, squared on the host).  The two products and the sum are rounded one by one
/// (no FMA), so the comparison is defined bit for bit: dx*dx + dy*dy > r2.
__global__ __launch_bounds__(PRUNE_WAVE) void prune_select_beyond(const double *__restrict__ X, const int *__restrict__ n, int NP,
                                                                  const double *__restrict__ r2, uint8_t *__restrict__ mask, int ld)
{
        const int b = blockIdx.x;
        const double *x = X + (size_t)b * NP;
        const int L = prune_landmarks(n[b], NP, ld);
        const double px = x[0], py = x[1], lim = r2[b];
        uint8_t *row = mask + (size_t)b * ld;
        for (int i = threadIdx.x; i < ld; i += PRUNE_WAVE)
        {
                uint8_t m = 0;
                if (i < L)
                {
                        const double dx = x[3 + 2 * i] - px, dy = x[4 + 2 * i] - py;
                        m = __dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)) > lim ? 1 : 0;
                }
                row[i] = m;
        }
}

/// grid: filters, block: one wave.  Ages are clock - lm_seen in unsigned 32-bit arithmetic (DevView), so a max_age of 0xFFFFFFFF selects nothing.
__global__ __launch_bounds__(PRUNE_WAVE) void prune_select_stale(const uint32_t *__restrict__ clock, const uint32_t *__restrict__ lm_seen,
                                                                 const int *__restrict__ n, int NP, const uint32_t *__restrict__ max_age,
                                                                 uint8_t *__restrict__ mask, int ld)
{
        const int b = blockIdx.x;
        const uint32_t *seen = lm_seen + (size_t)b * (NP / 2);
        const int L = prune_landmarks(n[b], NP, ld);
        const uint32_t clk = clock[b], lim = max_age[b];
        uint8_t *row = mask + (size_t)b * ld;
        for (int i = threadIdx.x; i < ld; i += PRUNE_WAVE)
                row[i] = (i < L && clk - seen[i] > lim) ? 1 : 0;
}

/// grid: filters, block: one wave.  src[b][0 .. n_new): 0, 1, 2, then 3 + 2i, 4 + 2i of every landmark i whose mask entry is 0, in order (ballot
/// and popcount scan over chunks of 64 landmarks).  Mask entries at or beyond the filter's landmark count are not read.
__global__ __launch_bounds__(PRUNE_WAVE) void prune_map(const uint8_t *__restrict__ mask, int ld, const int *__restrict__ n, const int *__restrict__ sens_n,
                                                        const int *__restrict__ wait_n, int NP, int *__restrict__ src, PruneMeta *__restrict__ meta)
{
        const int b = blockIdx.x, lane = threadIdx.x;
        const int nb = n[b];
        const int L = prune_landmarks(nb, NP, ld);
        const uint8_t *row = mask + (size_t)b * ld;
        int *s = src + (size_t)b * NP;
        if (lane < 3)
                s[lane] = lane;
        int kept = 0;
        for (int i0 = 0; i0 < L; i0 += PRUNE_WAVE) // (L is the same in every lane: all of them reach the ballot)
        {
                const int i = i0 + lane;
                const bool keep = i < L && row[i] == 0;
                const unsigned long long votes = __ballot(keep);
                if (keep)
                {
                        const int k = kept + __popcll(votes & ((1ull << lane) - 1ull));
                        s[3 + 2 * k] = 3 + 2 * i;
                        s[4 + 2 * k] = 4 + 2 * i;
                }
                kept += __popcll(votes);
        }
        if (lane == 0)
                meta[b] = PruneMeta{nb, 3 + 2 * kept, sens_n[b], wait_n[b]};
}

/// grid: filters, block: one wave; launched behind the unpack of aslam_remove_landmarks.  meta[b] and src[b] are what prune_map wrote BEFORE the
/// unpack (d.n holds the new dimension by now; the caller's mask is not read again, so it may go when the call returns): a filter that lost
/// nothing is not touched.  Survivor k comes from landmark (src[3 + 2k] - 3) / 2 >= k; chunks of 64 survivors ascend and a chunk's reads precede
/// its writes, so the move is safe in place.  Entries from the new landmark count to the old one become 0; the clock stays.
__global__ __launch_bounds__(PRUNE_WAVE) void sight_compact(const int *__restrict__ src, const PruneMeta *__restrict__ meta, int NP, uint32_t *lm_seen,
                                                            uint32_t *lm_hits)
{
        const int b = blockIdx.x, lane = threadIdx.x;
        const PruneMeta m = meta[b];
        if (m.n_new == m.n)
                return;
        const int H = NP / 2;
        const int L_old = min(max((m.n - 3) / 2, 0), H), L_new = min(max((m.n_new - 3) / 2, 0), L_old);
        const int *s = src + (size_t)b * NP;
        uint32_t *seen = lm_seen + (size_t)b * H, *hits = lm_hits + (size_t)b * H;
        for (int k0 = 0; k0 < L_new; k0 += PRUNE_WAVE)
        {
                const int k = k0 + lane;
                const bool on = k < L_new;
                const int i = on ? min(max((s[3 + 2 * k] - 3) / 2, 0), H - 1) : 0;
                const uint32_t sv = on ? seen[i] : 0u, hv = on ? hits[i] : 0u;
                if (on)
                {
                        seen[k] = sv;
                        hits[k] = hv;
                }
        }
        for (int i = L_new + lane; i < L_old; i += PRUNE_WAVE)
                seen[i] = 0u, hits[i] = 0u;
}

/// grid: records, block: one wave; launched behind the unpack of aslam_restore.  Snapshot format v1 does not carry the record: a restored
/// filter starts with clock 0 and every landmark at age 0.
__global__ __launch_bounds__(PRUNE_WAVE) void sight_clear(const SnapDesc *__restrict__ desc, int NP, uint32_t *__restrict__ clock,
                                                          uint32_t *__restrict__ lm_seen, uint32_t *__restrict__ lm_hits)
{
        const size_t slot = (size_t)desc[blockIdx.x].slot;
        const int H = NP / 2;
        if (threadIdx.x == 0)
                clock[slot] = 0u;
        for (int i = threadIdx.x; i < H; i += PRUNE_WAVE)
                lm_seen[slot * H + i] = 0u, lm_hits[slot * H + i] = 0u;
}

/// The source of record_pack (snapshot.h) for a pruned filter.  d.n of a descriptor is the NEW dimension; src is indexed by the slot.  A double2
/// at an even column straddles two landmarks (column 3 + 2i is odd), so each half has a source of its own: two indexed loads per pair.
struct PruneSrc : SnapshotSrc
{
        const int *src, *s; // prune_map's survivor lists [B][NP], the slot's
        __device__ void begin(const SnapCtx &c, const SnapDesc &d, int f)
        {
                SnapshotSrc::begin(c, d, f);
                s = src + (size_t)d.slot * NP;
        }
        __device__ double2 pair(const double *p, int q) const
        {
                double2 v;
                v.x = p[s[2 * q]];
                v.y = 2 * q + 1 < n ? p[s[2 * q + 1]] : 0.0;
                return v;
        }
        __device__ double2 P(int r, int q) const { return pair(Pin + (size_t)s[r] * NP, q); }
        __device__ double2 XZ(int z, int q) const { return pair(z ? Zin : Xin, q); }
};
} // namespace aslam
