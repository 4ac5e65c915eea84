"""The NumPy composition of cgrad with position correction
(tests/cgrad_positions.py), checked without a GPU: with positions off it IS
`cgrad_models.cgrad`, with positions on it corrects them; and the `alpha`
option that damps the position step."""
import inspect

import numpy as np
import pytest

import cgrad_models as cm
import cgrad_positions as cp
import rpie_positions as rp


def _grid():
    true, psi, probe, data, rng = rp.grid_problem(32, 2, 7)
    scan0 = (true + rp.jitter(rng, true.shape)).astype(np.float32)
    return true, scan0, psi, probe, data


@pytest.mark.parametrize("model,masked", [("gaussian", False),
                                          ("poisson", True)])
def test_positions_off_is_cgrad_models_bit_for_bit(model, masked):
    """Two epochs, two minibatches: every state array and the costs."""
    det = 32
    true, scan0, psi, probe, data = _grid()
    mask = cm.detector_mask(det) if masked else None
    psi0 = (0.8 * psi + 0.1).astype(np.complex64)
    batches = np.array_split(np.arange(len(true)), 2)
    new = lambda: dict(psi=psi0.copy(), probe=probe.copy(), scan=scan0.copy(),
                       costs=[])
    want, got = new(), new()
    for _ in range(2):
        want = cm.cgrad(want, data, batches, detector_shape=det, model=model,
                        mask=mask, cg_iter=2)
    got = cp.iterate(got, data, batches, 2, detector_shape=det, model=model,
                     mask=mask, cg_iter=2)
    assert got["costs"] == want["costs"]
    for key in ("psi", "probe", "scan"):
        assert np.array_equal(got[key], want[key]), key
    assert not np.array_equal(got["psi"], psi0)
    # an update_start beyond the run is positions off, too
    late = new()
    late["position"] = rp.position_state(scan0, update_start=5)
    late = cp.iterate(late, data, batches, 2, detector_shape=det, model=model,
                      mask=mask, cg_iter=2, rng=np.random.default_rng(0))
    assert late["costs"] == want["costs"]
    assert np.array_equal(late["psi"], want["psi"])
    assert np.array_equal(late["scan"], scan0)


# (model of the CG, model whose direction feeds the sums, cg_iter, probe CG)
CASES = [("gaussian", None, 1, True), ("gaussian", None, 2, False),
         ("gaussian", None, 4, True), ("gaussian", "poisson", 2, True),
         ("poisson", None, 1, False), ("poisson", None, 2, True),
         ("poisson", None, 4, False)]


@pytest.mark.parametrize("model,terms_model,cg_iter,recover_probe", CASES)
def test_composition_corrects_positions(model, terms_model, cg_iter,
                                        recover_probe):
    """7 x 7 positions at pitch 4 px, 32^2, 2 modes, +-0.7 px jitter, the
    object started from the truth, alpha = 1, two minibatches: after three
    epochs the mean position error (common shift removed) is below one third
    of its initial value (0.313 px); without correction it is unchanged."""
    det = 32
    true, scan0, psi, probe, data = _grid()
    batches = np.array_split(np.arange(len(true)), 2)
    first = rp.position_error(scan0, true)
    errors = []
    state = dict(psi=psi.copy(), probe=probe.copy(), scan=scan0.copy(),
                 costs=[], position=rp.position_state(scan0))
    state = cp.iterate(
        state, data, batches, 3, detector_shape=det, model=model,
        terms_model=terms_model, cg_iter=cg_iter, alpha=1.0,
        recover_probe=recover_probe, rng=np.random.default_rng(2),
        after_epoch=lambda s: errors.append(rp.position_error(s["scan"],
                                                              true)))
    print(f"{model} (sums: {terms_model or model}), cg_iter {cg_iter}, probe "
          f"{recover_probe}: {first:.4f} ->", ["%.4f" % e for e in errors])
    assert errors[-1] < first / 3
    still = dict(psi=psi.copy(), probe=probe.copy(), scan=scan0.copy(),
                 costs=[])
    still = cp.iterate(still, data, batches, 3, detector_shape=det,
                       model=model, cg_iter=cg_iter,
                       recover_probe=recover_probe)
    assert rp.position_error(still["scan"], true) == first


def test_half_the_poisson_direction_is_the_gaussian_one_near_the_solution():
    """1 - d/I = (1 - sqrt(d/I)) (1 + sqrt(d/I)): with I within 1 % of d the
    two directions agree to first order in the error."""
    det = 32
    true, scan0, psi, probe, data = _grid()
    near = (psi * 1.005).astype(np.complex64)
    s, d = true[:6], data[:6]
    g = cp.descent_direction("gaussian", d, near, s, probe, det)
    p = cp.descent_direction("poisson", d, near, s, probe, det)
    assert np.linalg.norm(p - g) < 2e-2 * np.linalg.norm(g)


def test_alpha_option():
    import tike_amd.ptycho as tp
    assert tp.CgradOptions().alpha == 0.05
    assert tp.CgradOptions().alpha == tp.RpieOptions().alpha
    # a new LAST field: what positional arguments mean is unchanged
    names = list(inspect.signature(tp.CgradOptions).parameters)
    assert names == ["num_batch", "batch_method", "rescale_method",
                     "rescale_period", "num_iter", "convergence_window",
                     "time_limit", "cg_iter", "step_length", "alpha"]
    o = tp.CgradOptions(3, "compact", "mean_of_abs_object", 10, 2, 0, np.inf,
                        4, 1.0)
    assert (o.num_batch, o.batch_method, o.cg_iter, o.step_length,
            o.alpha) == (3, "compact", 4, 1.0, 0.05)
    o = tp.CgradOptions(batch_method="compact", cg_iter=4, step_length=1.0)
    assert (o.batch_method, o.cg_iter, o.step_length) == ("compact", 4, 1.0)
