"""The float64 model of the prime-factor entries (tests/pfa_model.py) against
np.fft and the oracle; no GPU.  What test_pfa_entries_gpu.py holds the kernels
to is pinned here: the two sub-tile layouts, the stage contracts, the five
probe forms, the bilinear gather, and the input conditions of the GPU cases."""
import numpy as np
import pytest

import pfa_cases as pc
import pfa_model as pm
from util import OP_MAXABS, OP_NORMWISE, assert_close, relerr

DETS = [96, 160, 224, 192, 1024, 2048]
TIGHT = 1e-12


def _small(det):
    """(pw, nscan, S): an odd padding difference where the size allows it."""
    return {96: (95, 5, 3), 160: (127, 4, 2), 224: (100, 4, 2), 192: (192, 3, 2),
            1024: (1000, 2, 1), 2048: (2001, 1, 1)}[det]


@pytest.mark.parametrize("det", DETS)
def test_layout_maps(det):
    """Sub-tile n1, element n2 holds coordinate (M n1 + p n2) mod det (n1 + 4
    n2 at 1024 / 2048); both maps are permutations; to / from are inverses."""
    g = pm.Geom(det)
    assert g.p * g.M == det
    rng = np.random.default_rng(det)
    t = rng.random((2, det, det))
    s = pm.tile_to_subtiles(t, g)
    assert s.shape == (2, g.p, g.p, g.M, g.M)
    n1y, n1x, n2y, n2x = g.p - 1, 1, g.M - 3, 5
    if g.ct:
        y, x = n1y + 4 * n2y, n1x + 4 * n2x
        assert g.freq[2, 7] == 7 + g.M * 2
    else:
        y, x = (g.M * n1y + g.p * n2y) % det, (g.M * n1x + g.p * n2x) % det
    assert s[1, n1y, n1x, n2y, n2x] == t[1, y, x]
    np.testing.assert_array_equal(pm.subtiles_to_tile(s, g), t)
    np.testing.assert_array_equal(
        pm.subtiles_to_far(pm.far_to_subtiles(t, g), g), t)


@pytest.mark.parametrize("det", DETS)
def test_forward_composition_is_fft2(det):
    """gather -> sub-tile FFT -> combine's far plane = fwd_scale x
    fft2(pad(patch x probe)) at the mapped frequencies."""
    pw, nscan, S = _small(det)
    psi = pc.random_object(pw, det)
    scan = pc.positions(pw, nscan, first=2)
    pr = pc.probe_case("eigen", nscan, S, pw, det + 1, C=2, Sm=1)
    sub, patches = pm.fwd_gather(psi, scan, pr["probes"], det)
    fwd_scale = 0.37
    F = pm.far_plane(pm.subtile_fft(sub), det, fwd_scale)
    want = fwd_scale * np.fft.fft2(pm.pad_tile(patches[:, None] * pr["probes"], det))
    assert relerr(F, want) <= TIGHT
    # ... and the inputs of the combine cases invert that map
    back = pm.far_plane(pm.subtiles_from_far(want, det, fwd_scale).astype(
        np.complex128), det, fwd_scale)
    assert relerr(back, want) <= 1e-6  # (rounded to complex64 on the way)


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("det", DETS)
def test_backward_composition_is_ifft2(det, model):
    """combine -> inverse sub-tile FFT -> products = the direct chain
    ifft2(F x factor), cropped, with its products."""
    pw, nscan, S = _small(det)
    c = pm.combine_case(det, nscan, S, seed=det + model)
    pm.check_combine_case(c)
    sub_hat = c["sub"].astype(np.complex128)
    nm = int(c["mask"].sum())
    out, costs, F, I = pm.combine_gradient(sub_hat, c["data_nan"], c["mask"], det,
                                           c["fwd_scale"], model, 0.9, nm)
    rng = np.random.default_rng(det)
    patches = pc.rc(rng, nscan, pw, pw)
    pr = pc.probe_case("unique", nscan, S, pw, det + 3, Sm=1)
    mpu0 = pc.rc(rng, S, pw, pw)
    inv_scale, scale = 1.0 / det, 0.25
    objproj, chi0, mpu, chi = pm.inv_products(
        pm.subtile_fft(out, inverse=True), patches, pr["probes"], det, inv_scale,
        scale, mpu0)
    ms = c["mask"] != 0
    term, gg = pm.cost_terms(I, np.where(ms, c["data_nan"], 0).astype(np.float64),
                             model)
    factor = np.where(ms, gg, 0.9 - 1.0)
    want_chi = pm.crop_tile(
        inv_scale * det * det * np.fft.ifft2(F * factor[:, None]), pw)
    assert relerr(chi, want_chi) <= TIGHT
    assert relerr(objproj, np.sum(np.conj(pr["probes"]) * want_chi, 1)) <= TIGHT
    assert relerr(chi0, want_chi[:, 0]) <= TIGHT
    assert relerr(mpu, mpu0 + scale * np.sum(
        np.conj(patches)[:, None] * want_chi, 0)) <= TIGHT
    assert relerr(costs, np.sum(term[:, ms], -1) / nm) <= TIGHT


@pytest.mark.parametrize("form", pm.FORMS)
def test_probe_forms(form):
    """The five forms against the oracle's get_varying_probe."""
    from oracle.solvers import get_varying_probe
    nscan, S, pw = 3, 3, 6
    pr = pc.probe_case(form, nscan, S, pw, 11, C=2, Sm=2)
    got = pr["probes"]
    assert got.shape == (nscan, S, pw, pw)
    if form == "shared":
        want = np.broadcast_to(pr["probe"], got.shape)
    elif form == "per_scan":
        want = pr["probe"]
    elif form == "unique":
        want = pr["weights"][:, 0, :, None, None] * pr["probe"][None]
        want[:, :2] = pr["unique"]
    else:
        want = get_varying_probe(
            pr["probe"][None, None],
            None if pr["eigen"] is None else pr["eigen"][None],
            pr["weights"])[:, 0]
    assert_close(got, want, what=form)


def test_gather_is_the_oracles():
    """patches_of against oracle patch_fwd on positions inside, on the last
    legal corner, one row past it and over every side."""
    from oracle.operators import patch_fwd
    pw = 7
    psi = pc.random_object(pw, 3)
    scan = pc.positions(pw, 18)
    H, W = psi.shape
    assert np.any(np.floor(scan[:, 0]) == H - pw) and np.any(scan == -0.5)
    assert np.any((np.floor(scan[:, 0]) == H - pw - 1) &
                  (np.floor(scan[:, 1]) == W - pw - 1))
    assert np.any((np.floor(scan[:, 1]) == W - pw) & (scan[:, 0] >= 0) &
                  (np.floor(scan[:, 0]) < H - pw - 1))
    for lo, hi in ((0, 0), (1, 0), (0, 1)):  # over each side, by the floor
        assert np.any(np.floor(scan[:, lo]) < 0)
        assert np.any(np.floor(scan[:, lo]) + pw > (H, W)[lo])
    got = pm.patches_of(psi, scan, pw)
    want = patch_fwd(psi, scan, patch_width=pw)
    assert_close(got, want, what="patches")
    whole = np.all(scan == np.floor(scan), axis=1)
    assert whole.sum() >= 4
    np.testing.assert_array_equal(got[whole].astype(np.complex64), want[whole])
    assert np.all(got[5, 0] == 0) and np.any(got[5, 1] != 0)  # (-0.5, ..): row -1


@pytest.mark.parametrize("noise", ["gaussian", "poisson"])
def test_chain_is_the_oracles_gradient(noise):
    """96 / 64 with eigen probes and a mask: the whole model chain against
    oracle.solvers.get_nearplane_gradients (the poisson step length pinned to
    1: start 1, weight 0 -- the entries leave it to their caller)."""
    from oracle.solvers import get_nearplane_gradients
    det, pw, nscan, S = 96, 64, 5, 3
    model = ("gaussian", "poisson").index(noise)
    rng = np.random.default_rng(5)
    H, W = pc.object_shape(pw)
    psi = ((0.75 + 0.25 * rng.random((H, W))) * np.exp(
        1j * (rng.random((H, W)) - 0.5))).astype(np.complex64)
    scan = (rng.random((nscan, 2)) * 7 + 0.5).astype(np.float32)
    pr = pc.probe_case("eigen", nscan, S, pw, 8, C=2, Sm=2)
    mask = rng.random((det, det)) >= 0.15
    fwd_scale = inv_scale = 1.0 / det
    sub, patches = pm.fwd_gather(psi, scan, pr["probes"], det)
    sub_hat = pm.subtile_fft(sub)
    I0 = np.sum(np.abs(pm.far_plane(sub_hat, det, fwd_scale))**2, axis=1)
    data = (I0 * rng.uniform(0.5, 1.5, I0.shape)).astype(np.float32)
    nm, us, nb = int(mask.sum()), 0.9, 4
    out, costs, F, I = pm.combine_gradient(sub_hat, data, mask, det, fwd_scale,
                                           model, us, nm)
    objproj, chi0, mpu, chi = pm.inv_products(
        pm.subtile_fft(out, inverse=True), patches, pr["probes"], det, inv_scale,
        1.0 / nb)
    o = get_nearplane_gradients(
        data, psi[None], scan, pr["probe"][None, None], pr["eigen"][None],
        pr["weights"], 0, nscan, num_batch=nb, detector_shape=det,
        measured_pixels=mask, noise_model=noise, unmeasured_pixels_scaling=us,
        step_length_start=1.0, step_length_weight=0.0)
    assert_close(chi, o["chi"][:, 0], what="chi")
    assert_close(patches, o["patches"][:, 0, 0], what="patches")
    assert_close(mpu, o["m_probe_update"][0, 0], what="m_probe_update")
    assert_close(np.sum(np.abs(F)**2, 1), o["intensity"], what="intensity")
    np.testing.assert_allclose(costs, np.ravel(o["costs"]), rtol=1e-4)
    # objproj is what the oracle scatters: conj(unique_probe) x chi over modes
    assert_close(objproj, np.sum(np.conj(o["unique_probe"][:, 0]) * o["chi"][:, 0],
                                 axis=1), what="objproj")


@pytest.mark.parametrize("det,S,nscan", pc.COMBINE)
def test_combine_case_conditions(det, S, nscan):
    """The GPU combine cases: min I >= 0.25 on every measured pixel, counts
    non-negative with exact zeros on >= 1 % of the measured pixels."""
    pc.combine_case(det, S, nscan)
