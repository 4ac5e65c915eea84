"""cgrad over the noise models on the measured pixels, without a GPU: the
NumPy composition's gradient is a true gradient of its cost, and the mask
rule of _check_data_shape."""
import numpy as np
import pytest

import cgrad_models as cm


def _problem(rng, det=16, pw=16, S=2, N=4):
    HW = 32
    scan = (2 + rng.random((N, 2)) * (HW - pw - 4)).astype(np.float64)
    psi = (0.8 + 0.2 * rng.random((1, HW, HW))) * np.exp(
        1j * (rng.random((1, HW, HW)) - 0.5))
    probe = (rng.random((1, 1, S, pw, pw)) - 0.5
             + 1j * (rng.random((1, 1, S, pw, pw)) - 0.5))
    return scan, psi, probe


@pytest.mark.parametrize("model", ["gaussian", "poisson"])
@pytest.mark.parametrize("variable", ["psi", "probe"])
def test_composition_gradient_is_a_true_gradient(model, variable):
    """Central differences of the masked cost along random directions v are
    one fixed positive multiple of Re<g, v>."""
    rng = np.random.default_rng(3 if model == "gaussian" else 4)
    det = 16
    scan, psi, probe = _problem(rng, det=det)
    mask = cm.detector_mask(det)
    assert 0 < mask.sum() < mask.size
    from oracle import operators as ops
    far = ops.ptycho_fwd(probe, scan, psi * 1.1, det)
    data = ops.intensity_from_farplane(far).astype(np.float64) * 1.3
    data[:, ~mask] = np.nan
    if variable == "psi":
        x = psi
        f = lambda x: cm.cost(model, data, x, scan, probe, det, mask)
        g = cm.grad_psi(model, data, x, scan, probe, det, mask)
    else:
        x = probe
        f = lambda x: cm.cost(model, data, psi, scan, x, det, mask)
        g = cm.grad_probe(model, data, psi, scan, x, det, mask)
    assert np.all(np.isfinite(g))
    ratios = []
    for _ in range(5):
        v = rng.standard_normal(x.shape) + 1j * rng.standard_normal(x.shape)
        h = 1e-3 * np.linalg.norm(x) / np.linalg.norm(v)
        fd = (f(x + h * v) - f(x - h * v)) / (2 * h)
        ratios.append(fd / np.real(np.vdot(g, v)))
    ratios = np.array(ratios)
    assert np.all(ratios > 0), ratios
    spread = (ratios.max() - ratios.min()) / ratios.mean()
    assert spread < 1e-2, ratios


def _params(tp, mask):
    pw = 16
    return tp.PtychoParameters(
        probe=np.ones((1, 1, 1, pw, pw), np.complex64),
        psi=np.ones((1, 48, 48), np.complex64),
        scan=np.full((3, 2), 4.0, np.float32),
        algorithm_options=tp.CgradOptions(),
        exitwave_options=tp.ExitWaveOptions(measured_pixels=mask))


def test_check_data_shape_cgrad_all_measured_default_passes():
    import tike_amd.ptycho as tp
    from tike_amd.ptycho.ptycho import _check_data_shape
    data = np.ones((3, 32, 32), np.float32)
    p = tp.PtychoParameters(
        probe=np.ones((1, 1, 1, 16, 16), np.complex64),
        psi=np.ones((1, 48, 48), np.complex64),
        scan=np.full((3, 2), 4.0, np.float32),
        algorithm_options=tp.CgradOptions())
    # the default mask is probe-shaped and all True: every pixel measured
    assert p.exitwave_options.measured_pixels.shape[-1] != 32
    assert np.all(p.exitwave_options.measured_pixels)
    _check_data_shape(data, p)
    # a (16, 16) all-True mask given explicitly means the same
    _check_data_shape(data, _params(tp, np.ones((16, 16), bool)))
    # a data-shaped mask with unmeasured pixels is a mask
    _check_data_shape(data, _params(tp, cm.detector_mask(32)))


def test_check_data_shape_cgrad_rejects_a_mask_of_the_wrong_shape():
    import tike_amd.ptycho as tp
    from tike_amd.ptycho.ptycho import _check_data_shape
    data = np.ones((3, 32, 32), np.float32)
    mask = np.ones((16, 16), bool)
    mask[3, 4] = False
    with pytest.raises(ValueError, match="measured_pixels"):
        _check_data_shape(data, _params(tp, mask))
