"""What rpie's position correction rests on, checked without a GPU: the NumPy
composition the GPU tests compare against (tests/rpie_positions.py) is the
oracle's rpie when positions are off; the sums over all modes follow from the
object projection; and the method corrects positions on the small problems
the GPU tests scale up."""
import copy

import numpy as np
import pytest

import rpie_positions as rp
from oracle import operators as ops
from oracle import position as opos
from oracle import solvers as osol


def _small(depth, eigen, seed=3, det=16, S=2, N=6):
    rng = np.random.default_rng(seed)
    ij = np.stack(np.meshgrid(np.arange(3), np.arange(2), indexing="ij"),
                  -1).reshape(-1, 2)[:N]
    scan = (3 + 3.0 * ij + rng.random((N, 2))).astype(np.float32)
    HW = det + 14
    psi = rp.smooth_object(rng, depth, HW, sigma=1.0)
    w = osol.gaussian_probe(det, rin=0.6)
    probe = np.stack([w * np.exp(1j * np.pi * rng.random((det, det))) / (m + 1)
                      for m in range(S)])[None, None].astype(np.complex64)
    propagator = None
    if depth > 1:
        propagator = ops.fresnel_spectrum_propagator(
            (det, det), (2e-6, 2e-6), 1e-6, 1e-10)
    data = ops.intensity_from_farplane(
        ops.ptycho_fwd(probe, scan, psi, det, propagator=propagator)).astype(
            np.float32)
    ep = ew = None
    if eigen:
        ep = (0.1 * (rng.random((1, 1, 1, det, det)) - 0.5 + 1j *
                     (rng.random((1, 1, 1, det, det)) - 0.5))).astype(
                         np.complex64)
        ew = np.ones((N, 2, S), dtype=np.float32)
        ew[:, 1] = 0.05 * rng.standard_normal((N, S)).astype(np.float32)
    psi0 = np.full_like(psi, 0.5)
    psi0[1:] = 1.0
    probe0 = (probe * (1 + 0.05 * rng.standard_normal(probe.shape))).astype(
        np.complex64)
    state = dict(psi=psi0, probe=probe0, scan=scan, costs=[], eigen_probe=ep,
                 eigen_weights=ew)
    return state, data, propagator


@pytest.mark.parametrize("depth,eigen,model,method", [
    (1, False, "gaussian", "compact"), (1, True, "gaussian", "compact"),
    (1, False, "poisson", "per minibatch"), (2, False, "gaussian", "compact"),
    (3, False, "poisson", "compact")])
def test_composition_without_positions_is_the_oracle(depth, eigen, model,
                                                     method):
    """Two epochs, bit for bit: every array of the state and the costs."""
    state, data, propagator = _small(depth, eigen)
    if model == "poisson":
        data = np.round(data * (2000.0 / data.max())).astype(np.float32)
    det = data.shape[-1]
    batches = np.array_split(np.arange(len(data)), 2)
    kw = dict(detector_shape=det, alpha=1.0, batch_method=method,
              force_orthogonality=True, propagator=propagator,
              noise_model=model)
    want = osol.iterate(copy.deepcopy(state), data, batches, 2, solver="rpie",
                        rng=np.random.default_rng(5), **kw)
    got = rp.iterate(copy.deepcopy(state), data, batches, 2,
                     rng=np.random.default_rng(5), **kw)
    assert got["costs"] == want["costs"]
    for key in ("psi", "probe", "scan", "eigen_probe", "eigen_weights"):
        if want[key] is None:
            assert got[key] is None
        else:
            assert np.array_equal(got[key], want[key], equal_nan=True), key


@pytest.mark.parametrize("pw,S", [(6, 1), (20, 3), (64, 2)])
def test_sums_over_modes_from_the_object_projection(pw, S):
    """sum_s Re(conj(g P_s) chi_s) = Re(conj(g) objproj) and
    sum_s |g P_s|^2 = |g|^2 sum_s |P_s|^2 on the central window."""
    rng = np.random.default_rng(pw + S)
    N = 5
    rc = lambda *s: (rng.random(s) - 0.5 + 1j * (rng.random(s) - 0.5)).astype(
        np.complex64)
    patches, chi, probe = rc(N, pw, pw), rc(N, 1, S, pw, pw), rc(N, 1, S, pw, pw)
    num = np.zeros((N, 2), np.float32)
    den = np.zeros((N, 2), np.float32)
    for m in range(S):
        a, b = opos.position_update_terms(patches[:, None, None], probe, chi,
                                          m)
        num += a
        den += b
    objproj = np.sum(np.conj(probe) * chi, axis=(1, 2))
    inten = np.sum(np.abs(probe)**2, axis=(1, 2))
    crop = pw // 4
    c = slice(crop, pw - crop)
    for k, g in enumerate(opos.gaussian_gradient(patches)):
        np.testing.assert_allclose(
            np.sum(np.real(np.conj(g) * objproj)[:, c, c], axis=(-2, -1)),
            num[:, k], rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(
            np.sum((np.abs(g)**2 * inten)[:, c, c], axis=(-2, -1)),
            den[:, k], rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("depth,grid,recover_probe", [(1, 7, True),
                                                       (1, 7, False),
                                                       (2, 6, False)])
def test_composition_corrects_positions(depth, grid, recover_probe):
    """32^2 tiles, 2 modes, pitch 4 px, +-0.7 px jitter, the object started
    from the truth, alpha = 1, 2 compact minibatches: the mean position error
    falls with each of the first 4 epochs; without correction it stays."""
    det = 32
    propagator = None
    if depth > 1:
        propagator = ops.fresnel_spectrum_propagator(
            (det, det), (2e-6, 2e-6), 1e-6, 1e-10)
    true, psi, probe, data, rng = rp.grid_problem(
        det, 2, grid, depth=depth, propagator=propagator)
    scan0 = (true + rp.jitter(rng, true.shape)).astype(np.float32)
    batches = np.array_split(np.arange(len(true)), 2)
    kw = dict(detector_shape=det, alpha=1.0, batch_method="compact",
              propagator=propagator, recover_probe=recover_probe,
              rng=np.random.default_rng(2))
    for correct in (True, False):
        state = dict(psi=psi.copy(), probe=probe.copy(), scan=scan0.copy(),
                     costs=[], eigen_probe=None, eigen_weights=None)
        if correct:
            state["position"] = rp.position_state(scan0)
        errors = [rp.position_error(state["scan"], true)]
        state = rp.iterate(
            state, data, batches, 4, after_epoch=lambda s: errors.append(
                rp.position_error(s["scan"], true)), **kw)
        if correct:
            assert all(b < a for a, b in zip(errors, errors[1:])), errors
        else:
            assert errors[-1] == errors[0]
