/*
 * aslam_snapshot.h -- snapshot and restore of whole filters (libaslam_core.so): checkpoint, migrate, fork.
 *
 * A snapshot is one self-describing blob that holds EVERYTHING a filter is -- dimension, X, Z, the full P, A, both init flags, the sticky
 * status bits, the stored sensor message and the wait-list with its counts -- so that a filter restored from it continues the run it came
 * from bit for bit (aslam_set_state hands over n, X, Z and P only).  The record does not depend on the context it was taken in: not on the
 * padded row length, not on the kernel family (single-CU or large-state), not on the dtype (P, X and Z are binary64 everywhere).
 *
 * FORMAT, version 1.  Little-endian; every section starts on a 64-byte boundary.
 *
 *   blob header (64 B)    char magic[8] = "ASLSNP01"; u32 version = 1; u32 filter (ASLAM_EKF | ASLAM_UKF); u32 count; u32 reserved;
 *                         u64 total_bytes; zeros to 64
 *   offset table          u64 offset[count] from the start of the blob, zero-padded to a multiple of 64 B
 *   record i at offset[i] record header (64 B):
 *                           i32 n; i32 flags (ASLAM_SNAP_INIT_X | ASLAM_SNAP_INIT_Z); u32 status (ASLAM_ST_*); i32 sens_n; i32 wait_n;
 *                           i32 ld (= n + 1: n is odd, so every row of P is 16-byte aligned); u32 reserved[2]; f64 A[2] (A(0,0), A(1,0));
 *                           zeros to 64
 *                         record body:
 *                           f64 X[ld]; f64 Z[ld]            entry n is zero
 *                           f64 P[n][ld]                    the FULL matrix, row-major, column n of every row zero
 *                           f32 sens[sens_n][2]             range, bearing of the stored sensor message
 *                           f32 wait_rb[wait_n][2]          range, bearing of the wait-list
 *                           u32 wait_cnt[wait_n]
 *                         zeros to the next multiple of 64
 *
 * Records have their exact size (aslam_snapshot_record_bytes): a young filter in a large context is a few hundred bytes.
 * Not part of a record: the bound trace and the replay position (the caller's), the innovation record (restore sets it to NaN for the slots
 * it fills: "no callback yet"), all scratch of the kernels, and the filter's parameters (aslam_params, aslam_core.h): format v1 does not carry
 * them and aslam_restore leaves the destination slot's record alone -- one filter forked into B slots takes B noise models with one
 * aslam_set_params per slot.
 *
 * Status returns and aslam_last_error() as in aslam_core.h.
 */
#ifndef ASLAM_SNAPSHOT_H
#define ASLAM_SNAPSHOT_H

#include "aslam_core.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ASLAM_SNAPSHOT_VERSION 1
#define ASLAM_SNAPSHOT_MAGIC "ASLSNP01"

/* record header `flags` */
enum
{
        ASLAM_SNAP_INIT_X = 1, /* init_x: X is seeded from Z by the next callback (ekf.cpp:84-92) */
        ASLAM_SNAP_INIT_Z = 2  /* init_z: Z's landmark part is still to be seeded */
};

/* exact bytes of one record (header + body, without the padding to the next 64-byte boundary); -1 for an n that is not 3 + 2k or a
 * negative count.  Pure host code: no device needed. */
int64_t aslam_snapshot_record_bytes(int n, int sens_n, int wait_n);

/* Validate a HOST blob of `bytes` bytes: magic, version, filter kind, total_bytes <= bytes, offsets 64-byte aligned and every record inside
 * the blob, n = 3 + 2k, ld = n + 1, counts >= 0, no unknown flag or status bit.  Fills the filter kind and the record count (either may be
 * NULL).  ASLAM_ERR_ARG with a message otherwise.  Pure host code. */
int aslam_snapshot_check(const void *host_blob, int64_t bytes, int32_t *filter, int32_t *count);

/* Filters trajs[0 .. count) of ctx (trajs NULL = the whole batch, 0 .. batch-1, and count is ignored) -> blob.
 * *bytes_needed (may be NULL) always receives the exact size.  blob NULL = size query only; cap_bytes too small = ASLAM_ERR_ARG and
 * nothing is written.  Synchronises the context's last stream, reads the counts of the batch, then enqueues ONE pack launch on `stream`:
 * a device blob (is_device != 0, 16-byte aligned) is complete when `stream` is; a host blob is staged and complete on return. */
int aslam_snapshot(aslam_ctx *ctx, const int32_t *trajs, int count, void *blob, int64_t cap_bytes, int is_device, int64_t *bytes_needed,
                   void *stream);

/* Record records[i] of the blob (NULL = i) -> slot trajs[i] of ctx (NULL = i), i < count.  A record may be named several times (fork), a
 * slot once.  Everything is validated before the context is touched -- what aslam_snapshot_check checks; filter kind equal to the
 * context's (else ASLAM_ERR_ARG); n < max_landmark_count, sens_n <= max_obs, wait_n <= max_wait (else ASLAM_ERR_UNSUPPORTED); indices in
 * range, slots unique (else ASLAM_ERR_ARG) -- and a refused call leaves the context bit for bit as it was.  Synchronises the context's last
 * stream; the headers of a device blob come to the host through `stream` (the blob header, the offset table, and all record headers
 * through one gather launch: three small copies, each followed by a synchronisation of `stream`); then ONE unpack launch is enqueued on `stream`, which becomes the context's last stream.  A device blob must stay valid and
 * unchanged until `stream` has passed the launch; a host blob is copied before the call returns.  A restored slot is exactly what
 * aslam_reset followed by the hand-over would leave: zero padding, cleared scratch.  Contexts of either kernel family, dtype and batch size
 * accept every record that fits. */
int aslam_restore(aslam_ctx *ctx, const int32_t *records, const int32_t *trajs, int count, const void *blob, int64_t bytes, int is_device,
                  void *stream);

/* A rigid 2-D transform with its uncertainty: what takes a point of the source record's frame into the destination filter's frame. */
typedef struct
{
        double tx, ty, phi; /* source frame -> destination frame: p' = t + R(phi) p */
        double cov[9];      /* covariance of (tx, ty, phi), row-major 3 x 3 */
} aslam_frame;              /* 96 bytes */

/* JOIN MAPS: append the landmarks of record records[i] of the blob (NULL = i), with their full covariance block, behind the state of the
 * running filter in slot trajs[i] of ctx (NULL = i), i < count.  records, trajs, count, blob, bytes, is_device and the blob's validation
 * mean what they mean for aslam_restore -- a record may be named several times, a slot once -- except that the blob's filter kind is NOT
 * compared with the context's: a map is X and P, so a UKF record joins into an EKF context and the reverse.
 *
 * Filter A = slot trajs[i] has dimension n_A, the record L_B landmarks.  The selected ones, in ascending source index k_0 < ... < k_{m-1},
 * are those with select[i * ld + k] != 0 (host [count][ld]; entries at or beyond L_B are ignored; ld at least the largest L_B among the named
 * records; select NULL = every landmark of the record).  frames: host [count], NULL = identity with zero covariance.  With c = cos(phi),
 * s = sin(phi) taken once on the host in the call, R = [[c, -s], [s, c]], S = cov and l_p = (X_B[3 + 2 k_p], X_B[4 + 2 k_p]):
 *
 *   x'_p = tx + c lx - s ly          y'_p = ty + s lx + c ly
 *   G_p  = [[1, 0, -s lx - c ly],
 *           [0, 1,  c lx - s ly]]
 *   B_pq = the 2 x 2 block (k_p, k_q) of the record's P, read from its LOWER triangle only (for p = q the upper entry is the lower one: the
 *          source need not be exactly symmetric)
 *   P'_pq = R B_pq R^T + G_p S G_q^T   for p >= q;   P'_qp = (P'_pq)^T, the same bits
 *
 * After the call filter A has dimension n_A + 2m.  X, Z and P at indices below n_A are what they were, bit for bit;
 * X[n_A + 2p .. + 1] = (x'_p, y'_p); the new diagonal block of P is P', exactly symmetric; both cross blocks (old rows x new columns and
 * the mirror) are +0.0 -- the two maps are taken as INDEPENDENT, and ensuring that is the caller's responsibility; the record's pose and its
 * pose-landmark covariances are not used (the marginal of its landmarks).  Z[n_A + 2p .. + 1] is the reading A's own pose predicts for the
 * new landmark: with dx = x'_p - X_A[0], dy = y'_p - X_A[1], sqrt(dx^2 + dy^2) and atan2(dy, dx) - X_A[2], the latter wrapped as the
 * kernels' normalizeAngle wraps (fmod by 2 pi, then one step into [-pi, pi]) -- a joined landmark has zero innovation until it is sighted.
 * All of this arithmetic is binary64, in ASLAM_F32 contexts too.
 * Unchanged: A, both init flags, the status bits, the stored sensor message, the wait-list, the parameters, the sighting clock and the
 * sighting records of the old landmarks (aslam_restore clears those two; a join does not).  The new landmarks enter the sighting record as
 * aslam_grow enters them (last_seen = clock, hits = 0).  The last-callback innovation record and the sighted mask become what they are
 * after aslam_remove_landmarks (NaN; zero).  The slot is a FRESH one of the larger dimension, as a restored slot is.  An entry with m = 0
 * leaves its slot untouched bit for bit, and so does a filter that no entry names.  joined_out (host [count], may be NULL) receives m per
 * entry.
 *
 * Everything is checked before any filter is written; a refused call leaves the context bit for bit as it was:
 *   ASLAM_ERR_ARG          everything aslam_restore refuses about the blob, the indices and slot uniqueness; a select with ld below a named
 *                          record's L_B; a frame with a non-finite field, a cov that is not exactly symmetric, or a negative cov diagonal
 *                          (the message names the argument and the entry)
 *   ASLAM_ERR_STATE        a destination whose init_x flag is still set: its first callback would overwrite X with Z (ekf.cpp:87-91)
 *   ASLAM_ERR_UNSUPPORTED  n_A + 2m >= max_landmark_count for some entry (no status bit is set: this is a host request, not the growth path)
 * The messages of the last two name the filter.
 *
 * Synchronises the context's last stream; the headers of a device blob come to the host as in aslam_restore; n, the flags and the list sizes
 * of the batch come through ONE small device-to-host copy and one synchronisation of `stream`.  Then one pack launch, the unpack launch of
 * aslam_restore and one launch for the sighting record are enqueued on `stream`, which becomes the context's last stream.  No P, of source or
 * destination, crosses to the host.  A device blob must stay valid and unchanged until `stream` has passed the launches; a host blob is
 * copied before the call returns. */
int aslam_join_maps(aslam_ctx *ctx, const int32_t *records, const int32_t *trajs, int count, const void *blob, int64_t bytes, int is_device,
                    const aslam_frame *frames, const uint8_t *select, int ld, int32_t *joined_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* ASLAM_SNAPSHOT_H */
