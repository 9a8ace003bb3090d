/*
 * aslam_core.h -- C ABI of the MI355X-native EKF/UKF-SLAM predict/update core (libaslam_core.so).
 *
 * The reference (iamarkaj/AwesomeSLAM) has no plugin/FFI API: its filter step is the private method
 *     aslam::EKFSlam::slam(vx, az, dt)   awesome_slam/src/ekf/ekf.h:130-131, ekf.cpp:293-311
 *     aslam::UKFSlam::slam(vx, az, dt)   awesome_slam/src/ukf/ukf.h:142-143, ukf.cpp:260-392
 * operating on `Parameters` (ekf.h:56-67, ukf.h:56-82).  This header is the seam a maintainer would cut
 * there: the entry points below replace, one for one, the members of EKFSlam/UKFSlam named beside them.
 * INTEGRATION.md shows the reference-side binding.
 *
 * Conventions: plain C types, caller-owned buffers, `int` status returns (0 = ASLAM_OK, negative =
 * error, text via aslam_last_error()); no exceptions cross the seam.  A context owns all filter state
 * for `batch` independent filters ("trajectories") in HBM; matrices are row-major.  Everything is fp64
 * unless the context was created with ASLAM_F32 (EKF only: the UKF is fp64 at every size -- the single-CU
 * kernels up to N = 143, the ASLAM_CFG_UKF_LARGE launch chain beyond).
 *
 * STREAMS (this header, aslam_snapshot.h and aslam_scan.h).  One HIP stream per call: the `stream` argument
 * is a hipStream_t passed as void*, NULL = the default stream; blocking and non-blocking streams are alike.
 *   - "Asynchronous on `stream`" means: every launch of the call, and every copy of a device input or output,
 *     is enqueued on `stream` (the stream groups of a large-state batch fork from `stream` and join it again
 *     inside the call).  Small host descriptors may be copied down synchronously by the entries that
 *     synchronise inside (below); the entries that do not synchronise copy nothing outside `stream`.  DEVICE inputs -- a bound device trace, a device mask / into / cand / obs / blob / scan array --
 *     are read in stream order, so a producer enqueued on `stream` before the call is in order; DEVICE
 *     outputs are complete for whatever is enqueued on `stream` behind the call, and for the host once
 *     `stream` is synchronised.  No device-wide synchronisation is needed or done.
 *   - The context orders ITS OWN work across a change of stream: a call on another stream than the context's
 *     last one first waits, on the host, for that last stream.  The maintenance entries and the getters
 *     ("synchronises the context first") do so in every call; aslam_*_step, aslam_*_step_batch and
 *     aslam_replay[_stats] only when the stream differs from the last one -- on an unchanged stream they add
 *     nothing, neither a wait nor a launch.  `stream` then becomes the context's last stream.
 *   - Entries that need a number from the device synchronise `stream` INSIDE the call, and say so:
 *     aslam_*_step (the dimension; and X_out), aslam_remove_landmarks, aslam_merge_landmarks,
 *     aslam_join_maps, aslam_snapshot (the counts), aslam_restore and aslam_join_maps of a device blob
 *     (the headers), aslam_scan_landmarks on host arrays.
 *   - The caller's duty: HOST arrays handed to an asynchronous entry (aslam_*_step_batch: inputs and X_out)
 *     stay untouched / unread until the caller has synchronised `stream`; device buffers stay alive until
 *     `stream` has passed the call; a producer or consumer on ANOTHER stream than the call's is the caller's to
 *     order (an event); and a context is not re-entrant -- two host threads on one context need a lock.
 */
#ifndef ASLAM_CORE_H
#define ASLAM_CORE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ASLAM_ABI_VERSION 1

enum
{
        ASLAM_OK = 0,
        ASLAM_ERR_ARG = -1,      /* bad argument */
        ASLAM_ERR_HIP = -2,      /* a HIP runtime call failed (no device, out of memory, launch failure) */
        ASLAM_ERR_UNSUPPORTED = -3, /* configuration outside what the kernels cover */
        ASLAM_ERR_STATE = -4     /* call sequence error (e.g. replay without a trace) */
};

enum
{
        ASLAM_EKF = 0, /* rosrun awesome_slam ekf */
        ASLAM_UKF = 1  /* rosrun awesome_slam ukf */
};

enum
{
        ASLAM_F64 = 0,
        ASLAM_F32 = 1
};

/* per-trajectory status bits, sticky until aslam_reset (aslam_get_status) */
enum
{
        ASLAM_ST_GROWTH_REFUSED = 1, /* updateNewLandmark hit N >= MAX_LANDMARK_COUNT (ekf.cpp:263-268): landmarks dropped */
        ASLAM_ST_WAIT_OVERFLOW = 2,  /* wait-list capacity (max_wait) exceeded: an entry was dropped (deviation!) */
        ASLAM_ST_NOT_PD = 4,         /* a Cholesky pivot was <= 0 (the reference would go on with garbage, ukf.cpp:280) */
        ASLAM_ST_OBS_OVERFLOW = 8,   /* a sensor message had more entries than max_obs */
        ASLAM_ST_INTERNAL = 16       /* an on-chip synchronisation of the large-state kernels timed out (bounded spin instead of a hung GPU):
                                        this filter's state is invalid from that callback on */
};

/* aslam_config.flags */
enum
{
        ASLAM_CFG_UKF_LARGE = 1 /* accept a UKF context beyond the single-CU kernels (144 <= N): fp64 launch chain.
                                   The reference's central weight is (1-N)/3: see DESIGN.md before running long horizons */
};

typedef struct aslam_ctx aslam_ctx;

typedef struct
{
        int32_t filter;             /* ASLAM_EKF | ASLAM_UKF */
        int32_t dtype;              /* ASLAM_F64 | ASLAM_F32 */
        int32_t max_landmark_count; /* config.h:45 MAX_LANDMARK_COUNT (30): growth is refused when the state
                                       DIMENSION N would reach it (ekf.cpp:263).  A run-time field here. */
        int32_t batch;              /* independent filters held by this context */
        int32_t max_obs;            /* capacity of the stored sensor message (sensor_landmark, ekf.h:102) */
        int32_t max_wait;           /* capacity of new_landmark_wait (ekf.h:105); the reference's is unbounded */
        int32_t device;             /* HIP device ordinal */
        int32_t flags;              /* 0 or ASLAM_CFG_* bits; any other bit is ASLAM_ERR_ARG.  ASLAM_CFG_UKF_LARGE: with filter = UKF,
                                       dtype = F64 and a max_landmark_count of 145 .. 1087 a large-state UKF context instead of
                                       ASLAM_ERR_UNSUPPORTED; no effect on smaller UKF contexts and on the EKF */
} aslam_config;

/* A recorded input stream for `batch` filters x T callbacks, already narrowed the way the node's
 * callbacks narrow their messages (cbOdom/updateZandA ekf.cpp:137-142, cbSensorLandmark ekf.cpp:102-114):
 *   pose   [batch][T][2]  f64  msg->pose.pose.position.{x,y}
 *   yaw    [batch][T]     f32  quat2euler(orientation)  (tools.h:62-66; done by the host mirror)
 *   twist  [batch][T][2]  f64  msg->twist.twist.linear.x, angular.z
 *   dt     [batch][T]     f32  delta_time (ekf.cpp:80)
 *   obs_new[batch][T]     u8   1 = a sensor message precedes this odom message
 *   n_obs  [batch][T]     i32
 *   obs    [batch][T][max_obs][2] f32  range, bearing (LaserData, structures.h:85-101)
 * Pointers may be host or device memory (is_device). */
typedef struct
{
        int64_t T;
        int32_t max_obs;
        int32_t is_device;
        const double *pose;
        const float *yaw;
        const double *twist;
        const float *dt;
        const uint8_t *obs_new;
        const int32_t *n_obs;
        const float *obs;
} aslam_trace;

/* ---- life cycle ---------------------------------------------------------------------------------- */
/* EKFSlam()/UKFSlam() + initialize(): ekf.cpp:39-71, ukf.cpp:39-67 (for every filter of the batch) */
int aslam_create(const aslam_config *cfg, aslam_ctx **out);
int aslam_destroy(aslam_ctx *ctx);
/* initialize() again: N = 3, P = p0_pose * I, empty wait-list, init_x = init_z = true; the parameters (aslam_set_params) stay */
int aslam_reset(aslam_ctx *ctx);
const char *aslam_last_error(void);
int aslam_abi_version(void);

/* ---- noise and association parameters, per filter ---------------------------------------------------- */
/* The reference compiles these in (include/awesome_slam/config.h: "changing a filter constant = recompile"); here every filter of a context
 * holds its own record in HBM and every kernel family reads it at launch start.  R and Q stay diagonal, as the reference builds them.
 * UKF_STD_YAW (config.h:55) is NOT a parameter: stateTransitionFunction takes the yaw rate from its `az` argument and never reads
 * point(N+1) (common.h:46-75), so Paug(N+1,N+1) (ukf.cpp:277) cannot reach any result of the filter. */
typedef struct
{
        double r_xy, r_yaw;        /* R(0,0) = R(1,1), R(2,2): the odometry pose "measurement" rows (ekf.cpp:65) */
        double r_range, r_bearing; /* R(3+2i,3+2i), R(4+2i,4+2i) (ekf.cpp:278) */
        double q_xy, q_yaw;        /* Q(0,0) = Q(1,1), Q(2,2) (ekf.cpp:66-68) */
        double p0_pose;            /* P diagonal at initialize() / aslam_reset (ekf.cpp:64) */
        double p0_landmark;        /* new P diagonal on growth (ekf.cpp:277, aslam_grow) */
        double var_a;              /* UKF: Paug(N,N) (ukf.cpp:276); ignored by the EKF */
        float assoc_dist;          /* MIN_DIST_THRESH (config.h:43): landmark association and wait-list match */
        uint32_t promote_count;    /* MIN_LANDMARK_OCC (config.h:44) */
} aslam_params;                    /* 80 bytes */

/* The reference's constants, each the widened binary32 value the reference's own arithmetic sees (config.h declares them `const float`).
 * THE default table: aslam_params_default(), the device kernels' fresh contexts and the host mirror all initialise from it. */
#define ASLAM_PARAMS_DEFAULT_INIT                                                                                                           \
        {                                                                                                                                   \
                (double)0.2f, (double)0.2f, (double)0.2f, (double)0.2f, /* EKF_KR == UKF_KR */                                              \
                (double)0.001f, (double)0.001f,                         /* EKF_KQ == UKF_KQ */                                              \
                (double)0.001f,                                         /* EKF_KP_ROBOT_POSE == UKF_KP_ROBOT_POSE */                        \
                1.0,                                                    /* UKF_KP_LANDMARK_POSE, used by BOTH nodes on growth */            \
                (double)(0.2f * 0.2f),                                  /* UKF_STD_A * UKF_STD_A, a binary32 product */                     \
                0.5f, 10u                                               /* MIN_DIST_THRESH, MIN_LANDMARK_OCC */                             \
        }

int aslam_params_default(aslam_params *out);
/* Set the record of filter `traj` (-1 = every filter of the context); synchronises like the getters.  ASLAM_ERR_ARG, with a message that names
 * the field, unless r_*, p0_*, var_a and assoc_dist are finite and > 0, q_* finite and >= 0 and promote_count >= 1.
 * r_*, q_*, var_a and assoc_dist apply from the next callback (= rewriting the diagonals of the reference's R and Q); p0_landmark to later
 * growths; p0_pose at the next aslam_reset.  promote_count is compared with `==` against the counts as they stand, as the reference compares
 * (ekf.cpp:187-195): set it before the first callback, or entries already past the new value are never promoted.
 * aslam_reset keeps the parameters, as it keeps the innovation setting.  Snapshots (aslam_snapshot.h) do not carry them and aslam_restore
 * leaves the destination's alone: one filter forked into B copies with B noise models is aslam_restore + aslam_set_params.
 * In ASLAM_F32 contexts the parameters stay binary64 and are rounded where the chain rounds S. */
int aslam_set_params(aslam_ctx *ctx, int traj, const aslam_params *params);
int aslam_get_params(aslam_ctx *ctx, int traj, aslam_params *params);

/* ---- the per-callback seam (host keeps association/growth: ekf.cpp:137-290 stay on the host) ------ */
/* Set the device state of one filter: dimension n, X[n], Z[n], P[n*n] row-major (any of them NULL = keep).
 * Used for state hand-over and kernel-level tests.  It clears both init flags and carries neither A nor the stored sensor message, the
 * wait-list or the status bits: aslam_snapshot.h moves a WHOLE filter. */
int aslam_set_state(aslam_ctx *ctx, int traj, int n, const double *X, const double *Z, const double *P);
/* the matrix part of updateNewLandmark (ekf.cpp:271-278 / ukf.cpp:238-245): grow filter `traj` from its
 * current dimension to n_new; new P diagonal = the filter's p0_landmark (UKF_KP_LANDMARK_POSE), new X/Z entries from the seeds
 * (x_seed, z_seed hold n_new - n_old values). */
int aslam_grow(aslam_ctx *ctx, int traj, int n_new, const double *x_seed, const double *z_seed);
/* EKFSlam::slam (ekf.cpp:293-311) for one filter.  Z[n] is param.Z after updateZandA, a00/a10 are
 * param.A(0,0)/A(1,0) (ekf.cpp:210-211).  X_out (n doubles, may be NULL) receives param.X. */
int aslam_ekf_step(aslam_ctx *ctx, int traj, float vx, float az, float dt, const double *Z, double a00,
                   double a10, double *X_out, void *stream);
/* UKFSlam::slam (ukf.cpp:260-392) for one filter. */
int aslam_ukf_step(aslam_ctx *ctx, int traj, float vx, float az, float dt, const double *Z, double *X_out,
                   void *stream);

/* The same seam for ALL `batch` filters of the context at once (B live robots: one launch chain instead of B calls; replaces B x
 * `slam(...)` at ekf.cpp:94 / ukf.cpp:90).  Host arrays: vx, az, dt [batch]; Z [batch][ldz], row b = param.Z of filter b (its first
 * N_b entries are used); a00, a10 [batch] (EKF: param.A(0,0), param.A(1,0)); X_out [batch][ldx] or NULL.
 * ASYNCHRONOUS on `stream`: nothing inside synchronises.  The input arrays must stay untouched and X_out must not be read until
 * the caller has synchronised the stream (use pinned host memory for copies that really overlap). */
int aslam_ekf_step_batch(aslam_ctx *ctx, const float *vx, const float *az, const float *dt, const double *Z, int ldz,
                         const double *a00, const double *a10, double *X_out, int ldx, void *stream);
int aslam_ukf_step_batch(aslam_ctx *ctx, const float *vx, const float *az, const float *dt, const double *Z, int ldz,
                         double *X_out, int ldx, void *stream);
/* The two EKF seams with the mask of the callback: sighted[k] != 0 where the host's association gave landmark k an observation in this
 * callback ([n_landmarks] bytes; the batch form: [batch][ld], row b = filter b, its first (N_b - 3) / 2 entries are used).  Copied down like Z;
 * aslam_get_sighted returns it.  The mask is applied under aslam_sighted_update_enable only; with the mode off these are aslam_ekf_step[_batch]
 * that also record the mask.  Under the mode the plain aslam_ekf_step[_batch] treat EVERY landmark as sighted (they record an all-ones mask):
 * the same update as the _sighted call with all ones, bit for bit. */
int aslam_ekf_step_sighted(aslam_ctx *ctx, int traj, float vx, float az, float dt, const double *Z, const uint8_t *sighted, double a00,
                           double a10, double *X_out, void *stream);
int aslam_ekf_step_batch_sighted(aslam_ctx *ctx, const float *vx, const float *az, const float *dt, const double *Z, int ldz,
                                 const uint8_t *sighted, int ld, const double *a00, const double *a10, double *X_out, int ldx, void *stream);

/* ---- the replay seam (the whole callback, association and growth included, runs on the device) ----- */
/* Bind a trace.  Host pointers are copied to HBM; device pointers are used in place and must stay valid. */
int aslam_set_trace(aslam_ctx *ctx, const aslam_trace *trace);
/* Run callbacks t0 .. t0+nsteps-1 of the bound trace for every filter of the batch: cbSensorLandmark (if
 * obs_new) + cbOdom (updateZ[andA], growth, slam).  Asynchronous on `stream`.  poses_out (device memory,
 * [batch][nsteps][3] f64, may be NULL) receives X(0..2) after each callback; dims_out (device memory,
 * [batch][nsteps] i32, may be NULL) the state dimension N. */
int aslam_replay(aslam_ctx *ctx, int64_t t0, int64_t nsteps, double *poses_out, int32_t *dims_out, void *stream);
/* aslam_replay with the innovation statistics of every callback's slam() and the pose covariance behind it (device memory, f64; any of the
 * three may be NULL, with all three NULL this IS aslam_replay):
 *   nis_out      [batch][nsteps]     y^T S^-1 y, y the wrapped innovation the filter applies (Y, ekf.cpp:302-307; Zdiff, ukf.cpp:381-388) and
 *                                    S the filter's own S -- the UKF's full S, central-weight term included: the signed quadratic form
 *   logdet_out   [batch][nsteps]     ln |det S|
 *   pose_cov_out [batch][nsteps][6]  P(0,0), P(1,0), P(1,1), P(2,0), P(2,1), P(2,2) after the update
 * A callback in which slam() did not run (no sensor message yet, ekf.cpp:84-92) has NaN in all three and pose 0.0; a filter whose
 * ASLAM_ST_NOT_PD bit is set has NaN in nis and logdet.  The large-state paths take one launch more per callback (aslam_get_launch_info)
 * when a statistic is asked for; the filter itself computes bit for bit what it computes without. */
int aslam_replay_stats(aslam_ctx *ctx, int64_t t0, int64_t nsteps, double *poses_out, int32_t *dims_out, double *nis_out,
                       double *logdet_out, double *pose_cov_out, void *stream);
/* Switch the per-filter record of the LAST callback's (nis, logdet) on or off for aslam_*_step, aslam_*_step_batch and aslam_replay (off by
 * default; synchronises).  Switching it on (from off) and aslam_reset clear the record to NaN; aslam_reset keeps the setting. */
int aslam_innovation_enable(aslam_ctx *ctx, int on);
/* the record of filter `traj` (synchronises like the getters below); ASLAM_ERR_STATE when the record is off; NaN before the first callback
 * and after a callback in which slam() did not run */
int aslam_get_innovation(aslam_ctx *ctx, int traj, double *nis, double *logdet);

/* ---- sighted-only update (EKF contexts; off by default) --------------------------------------------------------------------------
   The reference uses every mapped landmark as a measurement in every update, with the stale range / bearing Z keeps for a landmark that was
   not re-observed (ekf.cpp:175-181, 300-310).  With the mode on, a callback updates with the pose rows and the rows of the landmarks SIGHTED in
   it alone: landmark k is sighted iff the association walk of the callback gave it at least one observation (the condition under which
   aslam_get_sightings' hits[k] goes up; a re-walked stored message counts; a landmark promoted in this callback is not sighted).  With
   M = {0, 1, 2} + {3 + 2k, 4 + 2k : k sighted}:  S = H_M P H_M^T + R_M,  K = P H_M^T S^-1,  X += K Y_M,  P = (I - K H_M) P.  Predict, updateH,
   angle wrapping and all bookkeeping are unchanged; a callback with nothing sighted still applies the three pose rows.  aslam_replay[_stats],
   aslam_ekf_step[_batch][_sighted] honour the mode; NIS and ln det S are then those of S_M and Y_M.  Context-wide; synchronises; kept by
   aslam_reset; not carried by snapshots.  ASLAM_ERR_UNSUPPORTED on a UKF context.  A context that never switches it on launches exactly the
   kernels it launched before the mode existed.  (Large-state contexts: ASLAM_GS_TILES=1 is ignored under the mode -- large_build_GS runs.) */
int aslam_sighted_update_enable(aslam_ctx *ctx, int on);
/* The mask the last callback of filter `traj` used (replay: written by the front end every callback, mode on or off; steps: what the call
 * recorded): min(cap, *n_landmarks) entries, the rest of sighted[cap] is zeroed.  aslam_reset, aslam_restore (restored slots) and
 * aslam_remove_landmarks (filters that lost a landmark) zero it.  Synchronises like the getters. */
int aslam_get_sighted(aslam_ctx *ctx, int traj, uint8_t *sighted, int cap, int *n_landmarks);

/* ---- removing landmarks from running filters ------------------------------------------------------- */
/* mask [batch][ld] u8, host or device (is_device; a device mask 16-byte aligned): entry (b, i) != 0 removes landmark i of filter b.
   Survivors keep their order and their values bit for bit (X, Z, rows and columns of P); N drops by 2 per removed landmark.  A, the init
   flags, the status bits (sticky ones included), the stored sensor message, the wait-list, the parameters and the sighting clock stay; the
   sighting records (below) move with their landmarks.  The mask is not read after the call returns.  A filter that loses nothing is not
   touched at all.  Synchronises the context first, then runs on `stream` like aslam_restore.
   ld must be at least the context's landmark capacity, (max_landmark_count - 3) / 2 rounded up; entries at or beyond a filter's landmark
   count are ignored.  One small device-to-host copy (the dimensions) and one synchronisation of `stream` happen inside the call; P never
   leaves the device.  The last-callback innovation record of a pruned filter becomes NaN, as after aslam_restore.
   An observation of a removed landmark no longer associates (nothing is left to associate it with): it goes to the wait-list like the
   sighting of any unknown landmark and is promoted again, as a NEW landmark at the end of the state, after promote_count sightings.  The
   wait-list itself is not edited: as for any sighting, an observation that falls within assoc_dist of an existing entry counts for that
   entry, and an entry whose count has already passed promote_count does not promote a second time (the reference's rule, ekf.cpp:217-253).
   ASLAM_ERR_ARG (the message names the argument) on a null argument, a too small ld or a misaligned device mask; a refused call leaves the
   context unchanged. */
int aslam_remove_landmarks(aslam_ctx *ctx, const uint8_t *mask, int ld, int is_device, void *stream);
/* device mask [batch][ld] <- 1 where landmark i of filter b lies farther than max_range[b] (host array, [batch]) from X(0..1) of its filter,
   0 everywhere else up to ld.  The comparison is dx*dx + dy*dy > max_range[b]^2 in binary64, each operation rounded on its own (no FMA).
   Synchronises the context first, then runs on `stream`.  ASLAM_ERR_ARG as above, and on a max_range that is not finite or is <= 0. */
int aslam_select_beyond(aslam_ctx *ctx, const double *max_range, uint8_t *mask_dev, int ld, void *stream);

/* ---- sighting records: when to remove a landmark --------------------------------------------------- */
/* Every filter keeps a clock and two numbers per landmark, written on the device by the front end of aslam_replay and read by nothing a
   filter computes:
     clock       callbacks of this filter in which updateZandA / updateZ ran (a callback that returns before the first sensor message does
                 not count); the first counted callback has clock 1
     last_seen   clock of the last callback in which the association walk gave landmark i at least one observation -- the callbacks that
                 rewrite Z(3+2i), Z(4+2i); a re-walked stored message counts, as it does for the reference's wait-list counts -- or, before
                 the first such callback, the clock of its promotion
     hits        callbacks in which it was sighted (several observations in one callback are one hit; a fresh landmark has 0)
   The age of a landmark is clock - last_seen in unsigned 32-bit arithmetic, which is right as long as no landmark goes unseen for 2^32
   callbacks.  aslam_reset zeroes everything.  aslam_grow and an aslam_set_state that raises the dimension enter the new landmarks as
   promoted now (last_seen = clock, hits = 0); an aslam_set_state that lowers it zeroes the entries beyond.  aslam_remove_landmarks keeps the
   clock and moves the records with their landmarks.  aslam_restore sets clock and records of the restored slots to 0 (every landmark at age
   0): snapshot format 1 does not carry them.  The per-callback seam (aslam_*_step) runs no association and leaves all of it alone. */
/* last_seen[cap], hits[cap] (either may be NULL), *n_landmarks, *clock of filter traj; synchronises like the getters */
/* (min(cap, padded_dim / 2) entries are written: those at or beyond *n_landmarks are the zeros the record holds there) */
int aslam_get_sightings(aslam_ctx *ctx, int traj, uint32_t *last_seen, uint32_t *hits, int cap, int *n_landmarks, uint32_t *clock);
/* device mask [batch][ld] <- 1 where clock[b] - lm_seen[b][i] > max_age[b] (host array [batch]; 0xFFFFFFFF = never), 0 elsewhere up to ld */
int aslam_select_stale(aslam_ctx *ctx, const uint32_t *max_age, uint8_t *mask_dev, int ld, void *stream);
/* (the mask is aslam_remove_landmarks' and aslam_select_beyond's: the same shape, synchronisation and ASLAM_ERR_ARG refusals) */

/* ---- merging duplicate landmarks: select, fuse, remove ---------------------------------------------- */
/* The reference associates by a fixed Euclidean threshold (assoc_dist); pose drift can push a landmark's re-observation past it, and the
   observation is then promoted as a SECOND landmark at the end of the state.  A merge applies the constraint "these two are the same point"
   and drops one of the pair.  One merge of landmark j into landmark i < j, with a = {3 + 2i, 4 + 2i}, c = {3 + 2j, 4 + 2j}:
       H (2 x n): +I2 at columns a, -I2 at columns c       d = X[a] - X[c]       W = P H^T = P[:, a] - P[:, c]
       S = H P H^T + noise_var I2                          X <- X - W S^-1 d     P <- P - W S^-1 W^T
   then landmark j is removed; i keeps its index and its Z entries.  The pairs of a filter are taken in ascending j, 8 per round, the k pairs
   of a round jointly: S is 2k x 2k, Lc = chol(S), V = Lc^-1 W^T, y = Lc^-1 d, X -= V^T y, P -= V^T V.  Rounds run one after another, a later
   one on the P the earlier one left; several leaves of one root may share a round.  All of it in binary64, in ASLAM_F32 contexts too (P is
   binary64 there), and P stays exactly symmetric.
   into [batch][ld] i32, host or device (is_device; a device array 16-byte aligned): into[b][j] = i merges landmark j of filter b into i, -1
   keeps j.  ld and "entries at or beyond a filter's landmark count are ignored" as for aslam_remove_landmarks.  ASLAM_ERR_ARG, with a message
   that names the filter and the landmark, unless every entry is -1 or has 0 <= i < j and into[b][i] == -1 (no chains: a root is not itself
   merged away), and unless noise_var is finite and >= 0.  A refused call leaves the context unchanged bit for bit: the device's report on
   `into` is checked on the host before any filter is written.
   Synchronises like aslam_remove_landmarks; one more small device-to-host copy (that report) and the synchronisation it needs come in front
   of that call's own.  After the rounds the merged-away landmarks leave through aslam_remove_landmarks' own path (a fresh, compacted slot;
   the sighted mask and the innovation record as after a prune); before it the sighting records fuse: hits[i] += hits[j], last_seen[i] =
   whichever of the two is the younger (age = clock - last_seen, unsigned 32-bit).  A filter that merges nothing is not touched.
   merged_out (host [batch] or NULL): pairs fused and removed per filter.  A filter whose S fails to factor in some round (a pivot <= 0 or
   not finite) keeps the merges of its earlier rounds; that round's and all later pairs are left alone, neither fused nor removed, and no
   status bit is set: the filter is valid. */
int aslam_merge_landmarks(aslam_ctx *ctx, const int32_t *into, int ld, int is_device, double noise_var, int32_t *merged_out, void *stream);
/* device array into_dev [batch][ld] i32 (16-byte aligned, ld as above) <- for every landmark j the i < j to merge it into, or -1; entries from
   the landmark count up to ld are -1.  gate, max_dist: host arrays [batch]; gate > 0 (infinity allowed), max_dist finite and > 0, else
   ASLAM_ERR_ARG.  For a pair i < j, binary64, every operation rounded on its own (no FMA), lower-triangle entries of P only, with
   a0 = 3 + 2i, a1 = a0 + 1, c0 = 3 + 2j, c1 = c0 + 1:
       dx = X[a0] - X[c0]    dy = X[a1] - X[c1]    r2 = dx*dx + dy*dy
       s00 = ((P[a0][a0] + P[c0][c0]) - P[c0][a0]) - P[c0][a0]
       s11 = ((P[a1][a1] + P[c1][c1]) - P[c1][a1]) - P[c1][a1]
       s10 = ((P[a1][a0] + P[c1][c0]) - P[c1][a0]) - P[c0][a1]
       det = s00*s11 - s10*s10
       t1 = (s10*dx)*dy      num = (((s11*dx)*dx) - (t1 + t1)) + ((s00*dy)*dy)      m = num / det
   (i, j) is a candidate iff r2 <= max_dist^2 (squared on the host), s00 > 0, det > 0 and m < gate.  partner[j] = the candidate i of smallest
   m, ties to the smaller i, or -1.  Then into[j] = partner[j] if partner[partner[j]] == -1, else -1 -- the conservative rule: a landmark whose
   partner is itself about to be merged waits for the next call, so every selected pair is directly gated and the array always passes
   aslam_merge_landmarks' validation.  Synchronises the context first, then runs on `stream`. */
int aslam_select_duplicates(aslam_ctx *ctx, const double *gate, const double *max_dist, int32_t *into_dev, int ld, void *stream);

/* ---- Mahalanobis-gated data association -------------------------------------------------------------- */
/* The reference associates an observation with the landmark nearest to it if that is closer than assoc_dist, a fixed Euclidean threshold that
   ignores the covariance.  This call evaluates the individual-compatibility gate where P lives: for every observation of every filter the
   innovation against each landmark, weighed by S_k = H_k P H_k^T + R, against a chi-square point (9.21 is the 99 % point of chi-square with
   2 degrees of freedom).  All arithmetic is binary64, in ASLAM_F32 contexts too; only lower-triangle entries of P are read.
   For filter b with L = (n_b - 3) / 2 landmarks and landmark k, a0 = 3 + 2k, a1 = a0 + 1:
       dx = X[a0] - X[0]    dy = X[a1] - X[1]    q = dx^2 + dy^2    rh = sqrt(q)    bh = atan2(dy, dx) - X[2]
       H_k (2 x 5 over the columns 0, 1, 2, a0, a1):   range row (-dx/rh, -dy/rh, 0, dx/rh, dy/rh),   bearing row (dy/q, -dx/q, -1, -dy/q, dx/q)
       S = H_k P5 H_k^T (P5: the symmetric 5 x 5 of those rows and columns)
       s00 = S00 + r_range    s11 = S11 + r_bearing    s10 = S10    det = s00 s11 - s10^2        (the filter's own aslam_params)
   The landmark is valid iff q > 0, s00 > 0 and det > 0 (a NaN fails every comparison).  For observation j = (r, beta), binary32 widened:
       v0 = r - rh    v1 = remainder(beta - bh, 2 pi) (the IEEE remainder; 2 pi rounded to binary64)
       m = (s11 v0^2 - 2 s10 v0 v1 + s00 v1^2) / det                                              (a NaN m is skipped)
   mdist[b][j] = the smallest m over the valid landmarks, +inf when there is none; assoc[b][j] = the k that attains it if m < gate[b], else
   -1; ties go to the smaller k.  Entries j >= n_obs[b] get -1 and +inf.
   obs [batch][ldo][2] f32 (range, bearing), host or device (is_device; a device array 16-byte aligned); n_obs, gate: host arrays [batch];
   assoc_dev: device [batch][ldo] i32; mdist_dev: device [batch][ldo] f64, or NULL (both 16-byte aligned).  ASLAM_ERR_ARG, with a message that
   names the argument (and the filter, where there is one): a null obs, n_obs, gate or assoc_dev, ldo < 1, an n_obs[b] outside 0 .. ldo, a
   gate[b] that is not > 0 (infinity is allowed), a misaligned device pointer.  A refused call launches nothing.
   Synchronises the context first, then runs on `stream` (one launch, one workgroup per filter); the outputs are complete when the stream
   is.  The call reads X, P, the dimensions and the parameters and writes nothing a filter owns.  It works on every kind of context; for the
   UKF it is this same linearised gate, not the S of the sigma points.  The replay seam (aslam_replay) keeps the Euclidean rule unless
   aslam_set_replay_gate switches this gate on there. */
int aslam_gate_observations(aslam_ctx *ctx, const float *obs, int ldo, int is_device, const int32_t *n_obs, const double *gate, int32_t *assoc_dev,
                            double *mdist_dev, void *stream);

/* ---- joint compatibility of a hypothesis of pairings --------------------------------------------------- */
/* The gate above decides each pairing alone.  The landmarks of a map are correlated through the pose, so pairings that each pass it can be
   inconsistent as a set.  This call tests a hypothesis jointly, where P lives: the sequential compatibility nearest neighbour rule (Neira &
   Tardos 2001 without the branch and bound).  Evaluated at the X and P the last callback left, all binary64, lower-triangle entries of P only
   (entry (r, c) is read as P[max(r,c)][min(r,c)]).
   The observations j = 0 .. n_obs[b]-1 are taken in message order, each with its candidate landmark cand[b][j] (normally the assoc_dev output of
   aslam_gate_observations).  A candidate k is usable iff 0 <= k < L_b and q > 0; dx, dy, q, rh, bh and H_k are the gate's, and
   nu_j = (r - rh, remainder(beta - bh, 2 pi)).  With A the ordered list of the pairings accepted so far, m = |A|:
       C_A = the stack of H_i P(idx_i, idx_i') H_i'^T, + diag(r_range, r_bearing) of the filter's own aslam_params on the diagonal blocks
       L_A = its lower Cholesky factor (2m x 2m)     z_A = L_A^-1 nu_A     D2 = |z_A|^2     logdet = 2 sum log L_A(ii)
   and for a usable candidate j, by bordering:
       c (2 x 2m) = the cross blocks H_j P(idx_j, idx_i) H_i^T, i in A       Y = c L_A^-T (forward substitution)       T = C_jj - Y Y^T
       t00 = sqrt(T00)    t10 = T10 / t00    d = T11 - t10^2    t11 = sqrt(d)
       w = nu_j - Y z_A   z0 = w0 / t00      z1 = (w1 - t10 z0) / t11      dd_j = z0^2 + z1^2
   The candidate becomes unusable if T00 is not > 0, d is not > 0 or dd_j is not finite (a NaN fails every comparison).  It is accepted iff
   D2 + dd_j < gate_tab[m + 1]: the two rows (Y | t00; t10 t11) join L_A, z0 and z1 join z_A, D2 += dd_j, logdet += 2 log(t00 t11), m += 1.
   Otherwise it is refused by the joint test: nothing is appended, the refused counter goes up by one.  Two observations with one candidate may
   both be accepted (R keeps C positive definite).  With gate_tab == NULL (evaluate mode) every usable candidate is accepted: the call reports
   D2, log det C and the increments of the given hypothesis.  The rule is deterministic, O(m^3), and DEPENDS ON THE MESSAGE ORDER; there is no
   search over alternative candidates.
   obs, ldo, is_device, n_obs: as for aslam_gate_observations, ldo <= ASLAM_JC_MAX_OBS.  cand_dev: device [batch][ldo] i32.  gate_tab: host
   [ldo + 1] f64 or NULL; gate_tab[m] bounds D2 of m pairings (the chi-square point of 2m degrees of freedom: aslam_chi2_point), entry 0 is
   ignored, one table serves the batch.  assoc_dev: device [batch][ldo] i32, the candidate where accepted, else -1, -1 from n_obs[b] on;
   assoc_dev == cand_dev exactly is allowed (the chain gate -> joint runs in place), every other overlap of two device arrays is refused.
   incr_dev: device [batch][ldo] f64 or NULL: dd_j of every usable candidate, accepted or refused, +inf for an unusable or absent candidate and
   from n_obs[b] on.  joint_dev: device [batch][2] f64 (D2, log det C_A; 0, 0 for an empty hypothesis).  count_dev: device [batch][2] i32
   (accepted, refused by the joint test).  Every device pointer 16-byte aligned.
   ASLAM_ERR_ARG, with a message that names the argument (and the filter, where there is one): a null obs, n_obs, cand_dev, assoc_dev,
   joint_dev or count_dev, ldo < 1, an n_obs[b] outside 0 .. ldo, a gate_tab[m], m >= 1, that is not > 0 (infinity is allowed), a misaligned
   or partially overlapping device pointer.  ASLAM_ERR_UNSUPPORTED: ldo > ASLAM_JC_MAX_OBS.  A refused call launches nothing.
   Synchronises the context first, then runs on `stream` (one launch, one workgroup per filter), so a cand_dev written by
   aslam_gate_observations on the same stream is in order.  Works on every kind of context (for the UKF it is this linearised test); writes
   nothing a filter owns. */
#define ASLAM_JC_MAX_OBS 64
int aslam_joint_compat(aslam_ctx *ctx, const float *obs, int ldo, int is_device, const int32_t *n_obs, const int32_t *cand_dev, const double *gate_tab,
                       int32_t *assoc_dev, double *incr_dev, double *joint_dev, int32_t *count_dev, void *stream);
/* host only: *out = the `prob` quantile of chi-square with `dof` degrees of freedom (bisection on the regularised incomplete gamma function).
   ASLAM_ERR_ARG for a null out, prob outside (0, 1) or dof < 1. */
int aslam_chi2_point(double prob, int dof, double *out);

/* The same gate inside the replay seam (aslam_replay[_stats]): per filter, off by default.  A callback of a filter whose gate is > 0, that
   starts with landmarks (n0 > 3) and has a non-empty stored message, associates as follows.  The evaluation point is the X and P the previous
   callback left (the motion of this odometry period is not added); bearings are normalised first, as ever.  For every observation j, m against
   every landmark k < (n0 - 3) / 2 exactly as aslam_gate_observations defines it (the same device functions compute both), arg-min with ties to
   the smaller k.
       accepted (m_min < gate):  Z(3+2k), Z(4+2k) take the observation (of several accepted observations of one landmark the last in message order);
                                 k is sighted (mask, last_seen, hits: one hit per callback)
       dropped  (not accepted, but the reference's own nearest-landmark distance is below assoc_dist):  neither a match nor wait-list evidence;
                                 the filter's rejected counter goes up by one
       otherwise:                the observation goes through the wait-list, which is unchanged and stays Euclidean
   Landmarks promoted in a callback are gated from the next one on.  n0 == 3, an empty message and every filter whose gate is 0 take the
   Euclidean rule, bit for bit what they compute without this call; a context in which no gate is > 0 launches exactly the kernels it launched
   before (aslam_kernel_info names the gated instantiation while one is in use; the gate adds no launch).  Everything behind association is
   untouched, and the gate composes with aslam_replay_stats and aslam_sighted_update_enable.  All four kernel families take it, the single-CU
   UKF included.  Not part of it: joint compatibility, a gate on the wait-list.  aslam_*_step* run no association and are unaffected.
   aslam_set_replay_gate: gate of filter traj (-1 = all); 0 = the Euclidean rule (default), > 0 (infinity allowed) = gated.  ASLAM_ERR_ARG,
   naming the argument, on a NaN or negative gate or a bad traj; a refused call changes nothing.  aslam_reset keeps the gates, like the
   parameters; snapshots do not carry them, and aslam_restore, prune, merge and join leave them alone.  The counter is zeroed by aslam_reset and,
   for the restored slots, by aslam_restore; prune, merge and join leave it alone.  All three synchronise the context first. */
int aslam_set_replay_gate(aslam_ctx *ctx, int traj, double gate);
int aslam_get_replay_gate(aslam_ctx *ctx, int traj, double *gate);
int aslam_get_assoc_rejected(aslam_ctx *ctx, int traj, uint64_t *count);

/* ---- read-back (synchronises the context's last stream) ------------------------------------------- */
int aslam_get_dim(aslam_ctx *ctx, int traj, int *n);
/* X[n], Z[n], P[n*n] row-major; any may be NULL */
int aslam_get_state(aslam_ctx *ctx, int traj, double *X, double *Z, double *P);
int aslam_get_A(aslam_ctx *ctx, int traj, double *a00, double *a10);
/* convertToLandmarkMsg (common.h:93-108): x[i] = X(3+2i), y[i] = X(4+2i); returns the count in *n_landmarks */
int aslam_get_landmarks(aslam_ctx *ctx, int traj, double *x, double *y, int *n_landmarks);
/* wait-list: up to `cap` entries of (range, bearing, count); *size = entries held */
int aslam_get_wait(aslam_ctx *ctx, int traj, float *range, float *bearing, uint32_t *count, int cap, int *size);
int aslam_get_status(aslam_ctx *ctx, int traj, uint32_t *status_bits);
/* padded row length of the device layout (multiple of 16) and bytes of HBM held by the filters' state and scratch, for reporting (the
   sighting records, 4 + 4 * padded_dim bytes per filter, are not in the count) */
int aslam_get_layout(aslam_ctx *ctx, int *padded_dim, int64_t *hbm_bytes);
/* name + launch geometry of the kernel aslam_replay uses for this context (for profiles / bench reports) */
int aslam_kernel_info(aslam_ctx *ctx, char *name, int name_cap, int *grid, int *block, int *lds_bytes);
/* what the LAST aslam_replay / aslam_*_step[_batch] of this context really launched (large-state path; the single-CU kernels report
 * 0, 0, 1): stream groups the batch was split into (1 = the caller's stream alone), whether the Cholesky of S ran as the one-launch
 * resident kernel, kernel launches per callback and group.  Lets a test assert that it exercised the launch shape it means to. */
int aslam_get_launch_info(aslam_ctx *ctx, int *stream_groups, int *chol_resident, int *launches_per_callback);
/* whether the LAST launch of this context handed large_syrk_bf16x3 the tail rule (a last tile row of <= 16 state rows formed on the idle waves
 * of the diagonal tiles; the kernel applies it per filter from its dimension).  0 with ASLAM_SYRK_TAIL=0, ASLAM_SYRK_RUNNING=1, in binary64 and
 * on the single-CU kernels. */
int aslam_get_syrk_tail(aslam_ctx *ctx, int *on);

#ifdef __cplusplus
}
#endif
#endif /* ASLAM_CORE_H */
