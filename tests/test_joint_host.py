"""Joint compatibility, without a GPU: the ABI is there, aslam_chi2_point (host arithmetic) gives the chi-square points, and the test-side
reference (joint_ref.py) is what it claims to be -- its bordering form is the dense nu^T (H P H^T + R)^-1 nu, a single pairing is the
individual gate's m, its binary64 and long-double evaluations decide alike on the inputs the GPU test uses with the margins that test relies
on, and the crafted cases give the outputs they were crafted for."""
import os
import re

import numpy as np
import pytest

import assoc_ref as ar
import joint_ref as jr
import merge_ref as mr
from awesomeslam_amd import core

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHI2_99 = {2: 9.2103, 4: 13.2767, 6: 16.8119, 128: 168.1332}
# (N, n_obs) of the GPU test -> accepted by the sequential test at 0.99 on the candidates of gate_ref at 9.21; nothing is refused
ACCEPTED = {(3, 4): 0, (5, 5): 4, (17, 5): 4, (131, 9): 8, (133, 64): 57, (17, 0): 0, (5, 1): 1, (141, 16): 14, (163, 16): 15, (1027, 24): 21}


def test_abi_declares_and_exports_the_calls(built):
    hdr = open(os.path.join(ROOT, "include", "aslam_core.h")).read()
    code = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S))
    assert ("int aslam_joint_compat(aslam_ctx *ctx, const float *obs, int ldo, int is_device, const int32_t *n_obs, const int32_t *cand_dev, "
            "const double *gate_tab, int32_t *assoc_dev, double *incr_dev, double *joint_dev, int32_t *count_dev, void *stream);") in code
    assert "int aslam_chi2_point(double prob, int dof, double *out);" in code and "#define ASLAM_JC_MAX_OBS 64" in hdr
    assert {"aslam_joint_compat", "aslam_chi2_point"} <= set(core.CORE_SYMBOLS)
    assert {"aslam_node_set_joint_prob", "aslam_node_joint_rejected"} <= set(core.NODE_SYMBOLS)
    node_hdr = open(os.path.join(ROOT, "awesomeslam_amd", "csrc", "host", "aslam_node.h")).read()
    for name in ("aslam_node_set_joint_prob", "aslam_node_joint_rejected"):
        assert name + "(" in node_hdr and hasattr(core.node_lib(), name)
    lib = core.core_lib()
    rc = lib.aslam_joint_compat(None, None, 4, 0, None, None, None, None, None, None, None, None)
    assert rc == -1 and b"aslam_joint_compat" in lib.aslam_last_error() and b"context" in lib.aslam_last_error()
    assert lib.aslam_abi_version() == 1


def test_chi2_points(built):
    for dof, want in CHI2_99.items():
        assert abs(core.chi2_point(0.99, dof) - want) <= 1e-4, dof
    assert abs(core.chi2_point(0.5, 2) - 2 * np.log(2)) <= 1e-12  # (2 dof: the exponential distribution, the median in closed form)
    assert abs(core.chi2_point(0.95, 1) - 3.841458820694124) <= 1e-9
    for prob, dof in ((0.0, 2), (1.0, 2), (-0.1, 2), (float("nan"), 2), (0.5, 0), (0.5, -3)):
        with pytest.raises(core.AslamError, match="aslam_chi2_point: .*(prob|dof)"):
            core.chi2_point(prob, dof)
    assert core.core_lib().aslam_chi2_point(0.5, 2, None) == -1


def test_chi2_points_against_scipy(built):
    stats = pytest.importorskip("scipy.stats")
    for prob in (0.01, 0.5, 0.9, 0.99, 0.999999):
        for dof in (1, 2, 3, 4, 10, 64, 128, 129):
            want = stats.chi2.ppf(prob, dof)
            assert abs(core.chi2_point(prob, dof) - want) <= 1e-10 * max(want, 1), (prob, dof)


def test_joint_gates_increase(built):
    tab = core.joint_gates(0.99, 64)
    assert tab.shape == (65,) and tab.dtype == np.float64 and tab[0] == 0.0
    assert (np.diff(tab) > 0).all()
    assert abs(tab[1] - CHI2_99[2]) <= 1e-4 and abs(tab[64] - CHI2_99[128]) <= 1e-4
    assert abs(core.joint_gates(0.5, 1)[1] - 1.3863) <= 1e-4


def shape_case(N, n_obs):
    X, P = mr.synthetic(N, [])
    obs = ar.observations(X, n_obs, 100 + N)
    cand, _ = ar.gate_ref(X, P, obs, gate=ar.GATE, dtype=np.longdouble)
    return X, P, obs, cand


@pytest.mark.parametrize("N,n_obs", [(5, 5), (17, 5), (131, 9), (163, 16)])
def test_the_bordering_form_is_the_dense_form(N, n_obs, built):
    """one hypothesis (the long-double decisions), two evaluations, in both precisions.  Long double: equal to 1e-15 relative, three decimal
    orders below what binary64 resolves.  Binary64: within 1000 x 2^-52 -- the spread of two legitimate orders on these well-conditioned inputs
    (the GPU test takes its bar from this very difference, per input)"""
    X, P, obs, cand = shape_case(N, n_obs)
    tab = core.joint_gates(0.99, n_obs)
    ld = jr.sequential(X, P, obs, cand, gate_tab=tab, dtype=np.longdouble)
    for dtype, tol in ((np.longdouble, 1e-15), (np.float64, 1000 * jr.EPS)):
        b = jr.sequential(X, P, obs, cand, gate_tab=tab, dtype=dtype, follow=ld.verdicts)
        D2, logdet, incr = jr.dense(X, P, obs, cand, ld, dtype=dtype)
        errs = (jr.err_of(b.D2, D2), jr.err_of(b.logdet, logdet, signed=True), jr.err_of(b.incr, incr))
        print(f"joint reference N={N} n_obs={n_obs} {dtype.__name__}: bordering vs dense D2 {errs[0]:.2e} logdet {errs[1]:.2e} incr {errs[2]:.2e}")
        assert max(errs) <= tol
    # the upper triangle of P is never read
    junk = P + np.triu(np.full_like(P, 7.0), 1)
    again = jr.sequential(X, junk, obs, cand, gate_tab=tab, dtype=np.longdouble)
    assert again.D2 == ld.D2 and np.array_equal(again.incr, ld.incr) and np.array_equal(again.assoc, ld.assoc)


@pytest.mark.parametrize("N,n_obs", [(5, 5), (17, 5), (131, 9)])
def test_one_pairing_is_the_individual_gate(N, n_obs):
    X, P, obs, cand = shape_case(N, n_obs)
    for dtype in (np.float64, np.longdouble):
        _, m = ar.gate_ref(X, P, obs, gate=np.inf, dtype=dtype)
        k, _ = ar.gate_ref(X, P, obs, gate=np.inf, dtype=dtype)
        for j in range(n_obs):
            r = jr.sequential(X, P, obs[j:j + 1], k[j:j + 1], dtype=dtype)  # evaluate mode
            assert r.accepted == 1 and r.assoc[0] == k[j] and r.D2 == r.incr[0]
            assert abs(r.D2 - m[j]) <= 64 * jr.EPS * max(m[j], 1)  # (2 x 2 by Cholesky against the closed form: a few roundings each)


@pytest.mark.parametrize("N,n_obs", list(ACCEPTED))
def test_binary64_and_long_double_decide_alike(N, n_obs, built):
    X, P, obs, cand = shape_case(N, n_obs)
    tab = core.joint_gates(0.99, max(n_obs, 1))
    b64 = jr.sequential(X, P, obs, cand, gate_tab=tab)
    ld = jr.sequential(X, P, obs, cand, gate_tab=tab, dtype=np.longdouble)
    g, t = jr.margins(X, P, obs, cand, gate_tab=tab)
    spread = jr.err_of(b64.D2, ld.D2)
    print(f"joint reference N={N} n_obs={n_obs}: accepted {ld.accepted} refused {ld.refused} D2 {float(ld.D2):.4f} decision margin {g:.2g} "
          f"pivot margin {t:.2g} binary64 vs long double {spread:.2e}")
    assert b64.verdicts == ld.verdicts and np.array_equal(b64.assoc, ld.assoc)
    assert (ld.accepted, ld.refused) == (ACCEPTED[(N, n_obs)], 0)
    assert g > 1e-6 and t > 1e-9
    assert spread <= 16 * jr.EPS  # (1.25e-15 at the most here; a few dozen roundings on well-conditioned inputs, with room for another libm)


@pytest.mark.parametrize("name", list(jr.crafted()))
def test_crafted_cases(name, built):
    c = jr.crafted()[name]
    tab = None if c["prob"] is None else core.joint_gates(c["prob"], max(len(c["obs"]), 1))
    for dtype in (np.float64, np.longdouble):
        r = jr.sequential(c["X"], c["P"], c["obs"], c["cand"], c["r"], c["r"], tab, dtype)
        if c["assoc"] is not None:
            assert r.assoc.tolist() == c["assoc"] and (r.accepted, r.refused) == (c["accepted"], c["refused"])
        assert np.isposinf(r.incr).astype(int).tolist() == c["inf"]
    g, t = jr.margins(c["X"], c["P"], c["obs"], c["cand"], c["r"], c["r"], tab)
    assert g > 1e-6 and t > 1e-9
    if name == "common-shift":
        ic, m = ar.gate_ref(c["X"], c["P"], c["obs"], c["r"], c["r"], ar.GATE, np.longdouble)
        assert ic.tolist() == [0, 1, 2, 3, 4] and 1.86 <= m.min() and m.max() <= 3.27  # each pairing passes alone
        assert abs(r.D2 - 8.939) < 1e-3 and abs(g - 0.34) < 0.01
        assert np.allclose(np.asarray(r.incr, np.float64), [1.86, 184.6, 6.84, 0.239, 695.7], rtol=2e-3)
    if name == "common-shift-reordered":
        first = jr.crafted()["common-shift"]
        back = [c["cand"].index(k) for k in range(5)]  # the verdicts in the first message's order
        assert [r.assoc[j] >= 0 for j in back] != [a >= 0 for a in first["assoc"]]  # the order of the message decides
    if name == "one-observation":
        _, m = ar.gate_ref(c["X"], c["P"], c["obs"], c["r"], c["r"], np.inf, np.longdouble)
        assert abs(r.D2 - m[0]) <= 64 * jr.EPS * max(m[0], 1)


def test_the_cap_case_has_64_usable_candidates(built):
    X, P, obs, cand = jr.cap64()
    assert len(set(cand.tolist())) == 64 and obs.shape == (64, 2)
    tab = core.joint_gates(0.99, 64)
    ld = jr.sequential(X, P, obs, cand, gate_tab=tab, dtype=np.longdouble)
    assert ld.verdicts.count("unusable") == 0 and ld.accepted + ld.refused == 64
    g, t = jr.margins(X, P, obs, cand, gate_tab=tab)
    assert g > 1e-6 and t > 1e-9
