"""The float64 model of the minibatch tail (tests/lstsq_tail.py) against the
oracle's own path, get_nearplane_gradients -> update_nearplane ->
precondition_nearplane_gradients, and against hand-computed 2x2 systems: the
GPU tests (tests/test_lstsq_tail_gpu.py) rest on this model, so the model
itself is pinned here, without a GPU."""
import numpy as np
import pytest

import lstsq_tail as lt


def _rc(rng, *shape):
    return (rng.standard_normal(shape) +
            1j * rng.standard_normal(shape)).astype(np.complex64)


@pytest.fixture(scope="module")
def minibatch():
    """16^2 window, 2 modes, one eigen probe on the first, 12 positions: the
    oracle's gradients, eigen update and step lengths of one minibatch."""
    from oracle import operators as ops
    from oracle import solvers as osol
    rng = np.random.default_rng(16)
    pw = det = 16
    S, N, num_batch = 2, 12, 2
    HW = pw + 14
    scan = (rng.random((N, 2)) * 11 + 1.25).astype(np.float32)
    psi_true = ((0.75 + 0.25 * rng.random((1, HW, HW))) * np.exp(
        1j * np.pi * (rng.random((1, HW, HW)) - 0.5))).astype(np.complex64)
    w = osol.gaussian_probe(pw, rin=0.6)
    probe = np.stack([w * np.exp(1j * np.pi * rng.random((pw, pw))) / (m + 1)
                      for m in range(S)])[None, None].astype(np.complex64)
    ep = _rc(rng, 1, 1, 1, pw, pw)
    ep = (ep / osol.mnorm(ep)).astype(np.complex64)
    ew = np.zeros((N, 2, S), np.float32)
    ew[:, 0] = 1
    ew[:, 1, 0] = 0.05 * rng.standard_normal(N)
    far = ops.ptycho_fwd(osol.get_varying_probe(probe, ep, ew), scan,
                         psi_true, det)
    data = np.sum(np.abs(far)**2, axis=(1, 2)).astype(np.float32)
    psi0 = (psi_true * (1 + 0.1 * rng.standard_normal(psi_true.shape))
            ).astype(np.complex64)
    probe0 = (probe * (1 + 0.05 * rng.standard_normal(probe.shape))).astype(
        np.complex64)
    o = osol.get_nearplane_gradients(
        data, psi0, scan, probe0, ep, ew, 0, N, num_batch=num_batch,
        detector_shape=det, measured_pixels=np.ones((det, det), dtype=bool))
    ep_o, ew_o = osol.update_nearplane(dict(o), probe0, ep.copy(), ew.copy(),
                                       0, N, num_batch=num_batch)
    pre = osol.psi_preconditioner(psi0, probe0, scan)
    precond, bo, bp = osol.precondition_nearplane_gradients(
        o["chi"], scan, o["unique_probe"], probe0, o["object_upd_sum"],
        o["m_probe_update"], pre, o["patches"], 0, N)
    bo, bp = float(np.ravel(bo)[0]), float(np.ravel(bp)[0])
    return dict(
        N=N, pw=pw, num_batch=num_batch, bo=bo, bp=bp, ep_o=ep_o[0, 0, 0],
        ew_o=ew_o, probe_o=probe0[0, 0] + bp * o["m_probe_update"][0, 0],
        cost_o=float(np.mean(o["costs"])),
        G=ops.patch_fwd(precond[0], scan, patch_width=pw),
        O=o["patches"][:, 0, 0], chi0=o["chi"][:, 0, 0],
        Pn=o["unique_probe"][:, 0, 0], mpu=o["m_probe_update"][0, 0],
        probe=probe0[0, 0], E=ep[0, 0, 0], weights=ew,
        norm=float(np.sum(np.square(ew[:, 1, 0].astype(np.float64)))),
        costs=np.ravel(o["costs"]),
        eps=float(np.float32(1e-9) / (pw * pw)) * pw * pw)


def _disagreements(got, mb):
    rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
    return dict(beta_object=rel(got["steps"][2], np.float64(mb["bo"])),
                beta_probe=rel(got["steps"][3], np.float64(mb["bp"])),
                cost=rel(got["steps"][4], np.float64(mb["cost_o"])),
                probe=rel(got["probe"], mb["probe_o"]),
                eigen_probe=rel(got["E"], mb["ep_o"]),
                eigen_weights=rel(got["weights"], mb["ew_o"]))


# 4 x the larger of the two forms' disagreements with the oracle measured on
# this problem (see test_model_reproduces_the_oracle_minibatch)
ORACLE_BAR = dict(beta_object=4 * 5.55e-8, beta_probe=4 * 5.35e-8,
                  cost=4 * 9.34e-9, probe=4 * 5.23e-8, eigen_probe=4 * 8.00e-8,
                  eigen_weights=4 * 2.81e-8)


@pytest.mark.parametrize("form", ["packed", "fused"])
def test_model_reproduces_the_oracle_minibatch(minibatch, form):
    """packed_tail and fused_tail, fed the oracle's own chi, patches,
    m_probe_update and preconditioned update, give the oracle's step lengths,
    updated probe, eigen probe and eigen weights.  The oracle keeps complex64 /
    float32 arrays between its float64 sums, so the two part at float32
    rounding.  Measured max|model - oracle| / max|oracle| (packed ; fused):
      beta_object    5.50e-08 ; 5.55e-08     beta_probe     5.35e-08 ; 5.26e-08
      mean cost      9.34e-09 ; 9.34e-09     probe          5.23e-08 ; 5.23e-08
      eigen probe    8.00e-08 ; 8.00e-08     eigen weights  2.81e-08 ; 2.81e-08
    The bar of each quantity is 4 x the larger of its two figures."""
    mb = minibatch
    kw = dict(eps=mb["eps"], count=float(mb["N"]), num_batch=mb["num_batch"],
              recover_psi=True, recover_probe=True)
    probe, mpu = mb["probe"], mb["mpu"]  # (S, pw, pw)
    combined = np.zeros_like(probe)
    if form == "packed":
        stats = lt.step_stats(mb["G"], mb["O"], mb["chi0"], probe[0],
                              mb["Pn"], mpu[0])
        got = lt.packed_tail(stats, mb["costs"], mb["O"], mb["chi0"], mpu,
                             mb["E"], mb["weights"], mb["norm"], probe,
                             combined, **kw)
    else:
        got = lt.fused_tail(mb["G"], mb["O"], mb["chi0"], mpu, mb["E"],
                            mb["weights"], mb["norm"], probe, combined,
                            mb["costs"], **kw)
    d = _disagreements(got, mb)
    print(form, {k: f"{v:.2e}" for k, v in d.items()})
    np.testing.assert_allclose(got["combined"],
                               (got["probe"] - probe) / mb["num_batch"],
                               rtol=0, atol=1e-12)
    for name, v in d.items():
        assert v <= ORACLE_BAR[name], (name, v, ORACLE_BAR[name])


def test_fused_form_equals_packed_form(minibatch):
    """The two compositions are the same mathematics in another order: in
    float64 they agree to rounding on every output."""
    mb = minibatch
    kw = dict(eps=mb["eps"], count=float(mb["N"]), num_batch=mb["num_batch"],
              recover_psi=True, recover_probe=True)
    probe, mpu = mb["probe"], mb["mpu"]
    f = lt.fused_tail(mb["G"], mb["O"], mb["chi0"], mpu, mb["E"],
                      mb["weights"], mb["norm"], probe, None, mb["costs"],
                      **kw)
    p = lt.packed_tail(f["stats"], mb["costs"], mb["O"], mb["chi0"], mpu,
                       mb["E"], mb["weights"], mb["norm"], probe, None, **kw)
    for name in ("steps", "probe", "weights", "E", "update", "sums3", "tail3",
                 "sums5", "nacc"):
        np.testing.assert_allclose(f[name], p[name], rtol=1e-11, atol=1e-13,
                                   err_msg=name)
    np.testing.assert_allclose(
        f["eigen_proj"], lt.eigen_proj(mb["O"], mb["chi0"], mpu[0],
                                       mb["E"]), rtol=1e-10, atol=1e-12)


# Two 2x2 systems worked by hand (eps = 0, sums = 0, so A1 = s0 and A4 = s1):
#  row 0: A1 = 2, A4 = 3, A2 = 1,  b = (1, 4): det = 5,
#         x1 = -(1 * 4 - 3 * 1) / 5 = -0.2 (clamped), x2 = (2 * 4 - 1) / 5 = 1.4
#  row 1: A1 = 2, A4 = 3, A2 = i,  b = (5, 5): det = 6 - 1 = 5,
#         x1 = -conj(5 i - 15) / 5 = 3 + i,  x2 = conj(10 + 5 i) / 5 = 2 - i
HAND = np.array([[2, 3, 1, 0, 1, 4, 0, 1],
                 [2, 3, 0, 1, 5, 5, 0, 1]], dtype=np.float32)
ZERO = np.zeros(3)


def test_solve_both_directions_by_hand_and_the_clamp():
    x1, x2 = lt.solve(HAND, 0.0, ZERO, 2.0, True, True)
    np.testing.assert_allclose(x1, [-0.2, 3 + 1j], rtol=1e-15)
    np.testing.assert_allclose(x2, [1.4, 2 - 1j], rtol=1e-15)
    so, sp = lt.step_lengths(HAND, 0.0, ZERO, 2.0, True, True)
    np.testing.assert_allclose(so, [0.0, 2.7], rtol=1e-15)  # -0.2 clamped
    np.testing.assert_allclose(sp, [1.26, 1.8], rtol=1e-15)
    out = lt.step_solve(HAND, 0.0, np.array([0, 0, 7.0]), 2.0, True, True)
    np.testing.assert_allclose(out, [2.7, 3.06, 1.35, 1.53, 3.5], rtol=1e-15)
    # a negative solution in the other direction as well: b -> -b
    neg = HAND.copy()
    neg[:, 4:6] *= -1
    so, sp = lt.step_lengths(neg, 0.0, ZERO, 2.0, True, True)
    np.testing.assert_allclose(so, [0.18, 0.0], rtol=1e-15)
    np.testing.assert_allclose(sp, [0.0, 0.0], rtol=0)


def test_solve_object_only_by_hand():
    """recover_psi alone: x1 = b1 / A1, x2 = 0, with the batch-mean term:
    sums = { 4, 6 } over count 2 -> A1 = 2 + 0.5 * 4 / 2 = 3."""
    sums = lt.step_sums(HAND, None, 0.0)
    np.testing.assert_allclose(sums, [4, 6, 0], rtol=1e-15)
    out = lt.step_solve(HAND, 0.0, sums, 2.0, True, False)
    np.testing.assert_allclose(out, [0.9 * (1 / 3 + 5 / 3), 0, 0.9, 0, 0],
                               rtol=1e-15)


def test_solve_probe_only_by_hand():
    """recover_probe alone: x2 = b2 / A4, A4 = 3 + 0.5 * 6 / 2 = 4.5; a `count`
    over all ranks (4) larger than the local rows: A4 = 3 + 0.5 * 6 / 4."""
    sums = lt.step_sums(HAND, [1.0, 2.0], 0.0)
    np.testing.assert_allclose(sums, [4, 6, 3], rtol=1e-15)
    out = lt.step_solve(HAND, 0.0, sums, 2.0, False, True)
    np.testing.assert_allclose(out, [0, 0.9 * 9 / 4.5, 0, 0.9, 1.5],
                               rtol=1e-15)
    out = lt.step_solve(HAND, 0.0, sums, 4.0, False, True)
    np.testing.assert_allclose(out, [0, 0.9 * 9 / 3.75, 0, 0.9 * 9 / 3.75 / 4,
                                     0.75], rtol=1e-15)
    # neither direction: nothing moves
    np.testing.assert_array_equal(
        lt.step_solve(HAND, 0.0, sums, 2.0, False, False)[:4], 0)


def test_eigen_normalise_is_the_expanded_quadratic():
    """The direct normalisation against the closed form the kernels use,
    |E + k u|^2 = |E|^2 + 2 k Re(conj(E) u) + k^2 |u|^2, and unit mean norm."""
    rng = np.random.default_rng(3)
    E, u = _rc(rng, 16, 16), _rc(rng, 16, 16) * 40
    count, beta = 12.0, 0.1
    E1, esum = lt.eigen_normalise(E, u, count, beta)
    uu, ee, eu = lt.norm_sums(E, u)
    k = beta / np.sqrt(uu / count**2 / E.size) / count
    inv = 1 / np.sqrt((ee + 2 * k * eu + k * k * uu) / E.size)
    np.testing.assert_allclose(E1, (E.astype(np.complex128) + k * u) * inv,
                               rtol=1e-12)
    np.testing.assert_allclose(esum, E.size, rtol=1e-12)


def test_single_precision_switch_restores_float64():
    s = np.abs(np.random.default_rng(0).standard_normal((5, 8))) + 0.5
    sums = lt.step_sums(s, None, 1e-9)
    err = lt.float32_error(lt.step_solve, s, 1e-9, sums, 5.0, True, True)
    assert 0 < err < 1e-5
    assert lt.step_solve(s, 1e-9, sums, 5.0, True, True).dtype == np.float64
    assert lt.scalar_bar(0.0) == 1e-6 and lt.scalar_bar(1e-6) == 8e-6
