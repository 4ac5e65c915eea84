"""NumPy composition of cgrad over a noise model on the measured pixels:
conjugate gradient (oracle.solvers.conjugate_gradient / line_search) on the
mean over positions of each pattern's mean cost over its measured pixels, with
the gradient Ptycho.adj(<model>_grad(...)) on measured pixels and 0 elsewhere.
Unmeasured counts (NaN here) are selected away, never multiplied."""
import numpy as np

from oracle import operators as ops
from oracle import solvers as osol

_TERMS = {
    "gaussian": lambda d, i: (np.sqrt(i) - np.sqrt(d))**2,
    "poisson": lambda d, i: i - d * np.log(i + 1e-9),
}
_FACTORS = {
    "gaussian": lambda d, i: 1 - np.sqrt(d) / (np.sqrt(i) + 1e-9),
    "poisson": lambda d, i: 1 - d / (i + 1e-9),
}


def _select(mask, values):
    if mask is None:
        return values
    with np.errstate(invalid="ignore"):
        return np.where(mask, values, 0)


def cost_each(model, data, intensity, mask=None):
    """Per-pattern mean of the model's terms over the measured pixels."""
    n = intensity.shape[-1] * intensity.shape[-2] if mask is None else mask.sum()
    # (float64: the poisson terms carry a large offset, sum(d - d log d), that
    # float32 sums would round the comparisons of the line search on)
    with np.errstate(invalid="ignore"):
        terms = _TERMS[model](np.asarray(data, np.float64),
                              np.asarray(intensity, np.float64))
    return _select(mask, terms).sum(axis=(-2, -1)) / n


def cost(model, data, psi, scan, probe, det, mask=None):
    far = ops.ptycho_fwd(probe, scan, psi, det)
    return float(np.mean(cost_each(model, data, ops.intensity_from_farplane(far),
                                   mask)))


def farplane_factor(model, data, far, mask=None):
    inten = ops.intensity_from_farplane(far)
    with np.errstate(invalid="ignore"):
        f = _select(mask, _FACTORS[model](data, inten))
    return far * f[..., None, None, :, :]


def grad_psi(model, data, psi, scan, probe, det, mask=None):
    far = ops.ptycho_fwd(probe, scan, psi, det)
    g = farplane_factor(model, data, far, mask).astype(far.dtype)
    uprobe = np.broadcast_to(probe, (len(scan), *probe.shape[1:]))
    return ops.ptycho_adj(g, uprobe, scan, psi)[0]


def grad_probe(model, data, psi, scan, probe, det, mask=None):
    far = ops.ptycho_fwd(probe, scan, psi, det)
    g = farplane_factor(model, data, far, mask).astype(far.dtype)
    uprobe = np.broadcast_to(probe, (len(scan), *probe.shape[1:]))
    return np.sum(ops.ptycho_adj(g, uprobe, scan, psi)[1], axis=0,
                  keepdims=True)


def cgrad(state, data, batches, *, detector_shape, model, mask=None,
          cg_iter=2, step_length=1.0, recover_probe=True):
    """One epoch: object then probe, `cg_iter` CG iterations each (as
    oracle.solvers.cgrad, over `model` on the measured pixels)."""
    det = detector_shape
    psi, probe, scan = state["psi"], state["probe"], state["scan"]
    batch_cost = []
    for b in batches:
        lo, hi = int(b[0]), int(b[0]) + len(b)
        d, s = data[lo:hi].astype(np.float32), scan[lo:hi]
        psi, c = osol.conjugate_gradient(
            psi, lambda p: cost(model, d, p, s, probe, det, mask),
            lambda p: grad_psi(model, d, p, s, probe, det, mask),
            num_iter=cg_iter, step_length=step_length)
        if recover_probe:
            probe, c = osol.conjugate_gradient(
                probe, lambda q: cost(model, d, psi, s, q, det, mask),
                lambda q: grad_probe(model, d, psi, s, q, det, mask),
                num_iter=cg_iter, step_length=step_length)
        batch_cost.append(c)
    state["costs"].append([float(np.mean(batch_cost))])
    state["psi"], state["probe"] = psi, probe
    return state


def detector_mask(det):
    """A beamstop disc at the zero frequency (corner-centred layout), a dead
    row and a dead column: True = measured."""
    f = np.fft.fftfreq(det) * det
    r2 = f[:, None]**2 + f[None, :]**2
    mask = r2 > (det / 24.0)**2
    mask[det // 3, :] = False
    mask[:, (2 * det) // 5] = False
    return mask
