"""Tuning the noise model: one recorded run, many parameter sets, one replay.

sweep() puts the same trajectory on every filter of one context, gives every filter its own aslam_params record (Core.set_params) and runs the
whole trace once with the innovation statistics switched on (Core.replay_stats).  The candidates are then ranked by what the statistics say:
the summed Gaussian log-likelihood of the innovations, the mean normalised innovation squared per degree of freedom (1 for a consistent filter)
and, when the trace carries ground truth, the mean pose NEES (3 for a consistent filter).  Plumbing only: every number comes out of the kernels.
"""
import numpy as np

from . import consistency
from .core import CFG_UKF_LARGE, F64, Core, Params


def sweep(kind, trajectory, candidates, max_landmark_count, dtype=F64, truth=None, device=0, gates=None):
    """Replay `trajectory` once per candidate, all candidates in one launch.

    kind                'ekf' or 'ukf'
    trajectory          a trace.Trace (its trajectory 0 is used) or a trace.Trajectory
    candidates          parameter sets: core.Params objects or dicts of overrides of the defaults (Core.set_params)
    max_landmark_count  as for Core
    truth               [T, 3] ground-truth poses; default: the trace's own, when it has one
    gates               one association gate per candidate (Core.set_replay_gate: 0 = the Euclidean rule, > 0 = the Mahalanobis gate), so that a
                        gate can be ranked like a noise model; None: the Euclidean rule everywhere, and the result is what it was without the argument

    Returns a list with one dict per candidate, in the order given:
        params          the record the filter ran with (dict)
        log_likelihood  sum over the callbacks in which slam() ran of consistency.log_likelihood(nis, logdet, dim)
        nis_per_dim     mean over those callbacks of nis / dim
        callbacks       how many there were
        N               the final state dimension
        status          the filter's ASLAM_ST_* bits (0 = nothing happened)
        pose_nees       mean consistency.pose_nees over those callbacks (None without ground truth)
    and, with `gates`:
        gate            the gate the filter ran with
        rejected        observations the gate dropped (Core.assoc_rejected)

    A larger log-likelihood is a better account of the recorded innovations.  UKF caveat: the UKF's S is the reference's signed form -- the
    central weight (1 - N) / 3 is negative, so S may be indefinite; nis is then a signed quadratic form and ln |det S| is not the normaliser of
    a density: for the UKF the figures are returned as they are and log_likelihood is a score without that meaning.
    """
    import torch

    from . import trace as tg

    if isinstance(trajectory, tg.Trajectory):
        tj = trajectory
        trajectory = tg.Trace(tj.odom[None], tj.dt[None], tj.obs_new[None], tj.n_obs[None], tj.obs[None],
                              np.zeros((1, 0, 2)) if tj.landmarks is None else np.asarray(tj.landmarks)[None], None if tj.truth is None else tj.truth[None], tj.warmup)
    B = len(candidates)
    if B < 1:
        raise ValueError("no candidates")
    if gates is not None and len(gates) != B:
        raise ValueError("`gates` holds one gate per candidate")
    tr = trajectory.select([0] * B)
    T = tr.T
    if truth is None and tr.truth is not None:
        truth = tr.truth[0]
    large = max_landmark_count > 145 or dtype != F64  # beyond the single-CU kernels (state dimension <= 144)
    with torch.cuda.device(device):
        core = Core(kind, max_landmark_count, batch=B, max_obs=tr.max_obs, max_wait=2048 if large else 512, device=device, dtype=dtype,
                    flags=CFG_UKF_LARGE if kind == "ukf" and large else 0)
        try:
            for b, cand in enumerate(candidates):
                core.set_params(cand, b)
            if gates is not None:
                for b, g in enumerate(gates):
                    core.set_replay_gate(g, b)
            core.reset()  # p0_pose applies at initialize(): every candidate runs under its own record from the first callback on
            core.set_trace(tr)
            dev = torch.device("cuda", device)
            poses = torch.zeros((B, T, 3), dtype=torch.float64, device=dev)
            dims = torch.zeros((B, T), dtype=torch.int32, device=dev)
            nis, logdet = (torch.zeros((B, T), dtype=torch.float64, device=dev) for _ in range(2))
            pcov = torch.zeros((B, T, 6), dtype=torch.float64, device=dev)
            core.replay_stats(0, T, poses.data_ptr(), dims.data_ptr(), nis.data_ptr(), logdet.data_ptr(), pcov.data_ptr())
            torch.cuda.synchronize(dev)
            poses, dims, nis, logdet, pcov = (a.cpu().numpy() for a in (poses, dims, nis, logdet, pcov))
            out = []
            for b in range(B):
                ran = ~np.isnan(pcov[b]).any(axis=1)  # slam() ran (nis alone is also NaN behind a failed factorisation)
                ll = consistency.log_likelihood(nis[b][ran], logdet[b][ran], dims[b][ran])
                nees = None
                if truth is not None and ran.any():
                    nees = float(np.nanmean(consistency.pose_nees(poses[b][ran], pcov[b][ran], np.asarray(truth)[:T][ran])))
                out.append(dict(params=Params.as_dict(core.params(b)), log_likelihood=float(ll.sum()),
                                nis_per_dim=float((nis[b][ran] / dims[b][ran]).mean()) if ran.any() else float("nan"), callbacks=int(ran.sum()),
                                N=core.dim(b), status=core.status(b), pose_nees=nees))
                if gates is not None:
                    out[-1].update(gate=core.replay_gate(b), rejected=core.assoc_rejected(b))
            return out
        finally:
            core.close()
