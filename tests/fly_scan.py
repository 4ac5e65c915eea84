"""float64 NumPy model of fly-scan ptychography: `fly` consecutive scan
positions expose one frame.

    I_f = sum_{j < fly} sum_{m < S} |far[f * fly + j, m]|^2
    cost = mean over frames of each frame's mean over its measured pixels of
           (sqrt(I) - sqrt(d))^2 (gaussian) or I - d log(I + 1e-9) (poisson)
    far-plane gradient of position (f, j), mode m:
           far * (1 - sqrt(d_f) / (sqrt(I_f) + 1e-9))   (gaussian)
           far * (1 - d_f / (I_f + 1e-9))               (poisson)
    object / probe gradient: the adjoint operator of that far-plane gradient

and a cgrad epoch over it (conjugate gradient with Dai-Yuan directions and
the backtracking search of oracle.solvers, which also records how clearly
every comparison of the search was decided).  The operator is composed from
oracle.operators' patch gather / scatter (bilinear weights in float32, as
everywhere) with complex128 transforms.  Unmeasured counts (NaN in the tests)
are selected away, never multiplied.  With fly == 1 every function is
tests/cgrad_models.py's."""
import numpy as np
import scipy.fft

from oracle import operators as ops

import cgrad_models as cm

_TERMS = cm._TERMS
_FACTORS = cm._FACTORS


# ------------------------------------------------------------- the operator
def fwd(probe, scan, psi, det):
    """(N, 1, S, det, det) complex128."""
    near = ops.convolution_fwd(np.asarray(psi[0], np.complex128), scan,
                               np.asarray(probe[..., 0, :, :, :],
                                          np.complex128), det)
    return scipy.fft.fft2(near, axes=(-2, -1), norm="ortho")[..., None, :, :, :]


def adj(far, probe, scan, psi):
    """(psi_adj (1, H, W), probe_adj (N, 1, S, pw, pw)) complex128."""
    near = scipy.fft.ifft2(far, axes=(-2, -1), norm="ortho")[..., 0, :, :, :]
    p = np.asarray(probe[..., 0, :, :, :], np.complex128)
    p = np.broadcast_to(p, (len(scan), *p.shape[-3:]))
    psi = np.asarray(psi, np.complex128)
    psi_adj = ops.convolution_adj(near, scan, p, psi.shape[-2], psi.shape[-1])
    probe_adj = ops.convolution_adj_probe(near, scan, psi[0], p.shape[-1])
    return psi_adj[None], probe_adj[..., None, :, :, :]


# ------------------------------------------------- intensity, cost, gradient
def frame_intensity(far, fly):
    """(F, det, det) from far (F * fly, 1, S, det, det)."""
    far = np.asarray(far)
    N, det = far.shape[0], far.shape[-1]
    power = (far.real.astype(np.float64)**2 + far.imag.astype(np.float64)**2)
    return power.reshape(N // fly, -1, det, det).sum(axis=1)


def _select(mask, values):
    if mask is None:
        return values
    with np.errstate(invalid="ignore"):
        return np.where(mask, values, 0)


def cost_each(model, data, intensity, mask=None):
    """Per-frame mean of the model's terms over the measured pixels."""
    n = intensity.shape[-1] * intensity.shape[-2] if mask is None else mask.sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        terms = _TERMS[model](np.asarray(data, np.float64),
                              np.asarray(intensity, np.float64))
    return _select(mask, terms).sum(axis=(-2, -1)) / n


def farplane_gradient(model, data, far, fly, mask=None):
    """The far-plane gradient, 0 at unmeasured pixels; data and intensity
    repeated over the positions and modes of a frame."""
    inten = frame_intensity(far, fly)
    with np.errstate(invalid="ignore", divide="ignore"):
        f = _select(mask, _FACTORS[model](np.asarray(data, np.float64), inten))
    return far * np.repeat(f, fly, axis=0)[:, None, None, :, :]


def simulate(det, probe, scan, psi, fly):
    return frame_intensity(fwd(probe, scan, psi, det), fly)


def cost(model, data, psi, scan, probe, det, fly, mask=None):
    inten = frame_intensity(fwd(probe, scan, psi, det), fly)
    return float(np.mean(cost_each(model, data, inten, mask)))


def grad_psi(model, data, psi, scan, probe, det, fly, mask=None):
    g = farplane_gradient(model, data, fwd(probe, scan, psi, det), fly, mask)
    return adj(g, probe, scan, psi)[0]


def grad_probe(model, data, psi, scan, probe, det, fly, mask=None):
    g = farplane_gradient(model, data, fwd(probe, scan, psi, det), fly, mask)
    return np.sum(adj(g, probe, scan, psi)[1], axis=0, keepdims=True)


# --------------------------------------------------------------- the solver
def _direction(grad1, grad0=None, dir_=None):
    if dir_ is None:
        return -grad1
    return (-grad1 + dir_ * np.linalg.norm(grad1.ravel())**2 /
            (np.sum(dir_.conj() * (grad1 - grad0)) + 1e-32))


def _line_search(f, x, d, step, margins, fx=None):
    """oracle.solvers.line_search; every comparison `f(x + step d) <= f(x)`
    leaves |f(x + step d) - f(x)| / |f(x)| in `margins`."""
    fx = f(x) if fx is None else fx
    while True:
        # (the product rounds x and the step to float32 between iterations)
        xsd = (x + np.float32(step) * d).astype(np.complex64).astype(
            np.complex128)
        fxsd = f(xsd)
        margins.append(abs(fxsd - fx) / abs(fx))
        if fxsd <= fx:
            return step, fxsd, xsd
        step *= 0.5
        if step < 1e-32:
            return 0, fx, x


def conjugate_gradient(x, cost_function, grad, num_iter, step_length,
                       margins):
    dir_ = grad0 = fx = None
    for i in range(num_iter):
        grad1 = grad(x)
        dir_ = _direction(grad1) if i == 0 else _direction(grad1, grad0, dir_)
        grad0 = grad1
        step_length, fx, x = _line_search(cost_function, x, dir_, step_length,
                                          margins, fx)
    return x, fx


def cgrad(state, data, batches, *, detector_shape, fly, model, mask=None,
          cg_iter=2, step_length=1.0, recover_probe=True):
    """One epoch: per minibatch of POSITIONS (whole frames), object then
    probe, `cg_iter` CG iterations each.  state["margins"] collects the
    relative margin of every line-search comparison."""
    det = detector_shape
    psi = np.asarray(state["psi"], np.complex128)
    probe = np.asarray(state["probe"], np.complex128)
    scan = state["scan"]
    margins = state.setdefault("margins", [])
    batch_cost = []
    for b in batches:
        lo, hi = int(b[0]), int(b[0]) + len(b)
        assert lo % fly == 0 and hi % fly == 0
        d, s = data[lo // fly:hi // fly], scan[lo:hi]
        psi, c = conjugate_gradient(
            psi, lambda p: cost(model, d, p, s, probe, det, fly, mask),
            lambda p: grad_psi(model, d, p, s, probe, det, fly, mask),
            cg_iter, step_length, margins)
        if recover_probe:
            probe, c = conjugate_gradient(
                probe, lambda q: cost(model, d, psi, s, q, det, fly, mask),
                lambda q: grad_probe(model, d, psi, s, q, det, fly, mask),
                cg_iter, step_length, margins)
        batch_cost.append(c)
    state["costs"].append([float(np.mean(batch_cost))])
    state["psi"], state["probe"] = psi, probe
    return state


# ------------------------------------------------------------- the problems
FIXTURE = dict(obj=96, pw=32, det=32, S=2, fly=3, nframe=12, seed=3, amp=1.0,
               mix=0.3, dim=0.5)
"""The problem of tests/golden/fly_scan.npz."""

SOLVER_CASES = {
    # name: problem; seeds chosen so that every comparison of the float64
    # line searches, over both epochs and every (model, mask, probe) variant,
    # is decided by a relative margin >= MIN_MARGIN
    # (test_fly_scan_cpu.py asserts it)
    "fixture": FIXTURE,
    "fused64": dict(obj=112, pw=64, det=64, S=1, fly=3, nframe=6, seed=1,
                    amp=1.0, mix=0.3, dim=0.6),
}
SOLVER_VARIANTS = [(model, use_mask, recover_probe)
                   for model in ("gaussian", "poisson")
                   for use_mask in (False, True)
                   for recover_probe in (False, True)]
MIN_MARGIN = 1e-3


def window(pw, rin=0.6):
    r = np.hypot(*np.meshgrid(np.linspace(-1, 1, pw), np.linspace(-1, 1, pw)))
    return np.exp(-(r / rin)**2 / 2)


def problem(obj, pw, det, S, fly, nframe, seed, amp=4.0, mix=0.8,
            dim=1.0):
    """A seeded fly-scan problem: frames on a grid, the `fly` positions of a
    frame along a short line (the stage moves while the detector integrates).
    Returns dict(scan (F * fly, 2) f32, psi (1, obj, obj) c64 the true object,
    probe (1, 1, S, pw, pw) c64, data (F, det, det) f32, psi0 the first
    iterate)."""
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(nframe)))
    room = obj - pw - 4  # corner coordinates in [2, obj - pw - 2)
    pitch = (room - 2.0 * fly) / max(side - 1, 1)
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side),
                              indexing="ij"), -1).reshape(-1, 2)[:nframe]
    start = 2 + pitch * ij + 0.9 * rng.random((nframe, 2))
    along = np.arange(fly)[None, :, None] * np.array([0.35, 1.7])[None, None]
    scan = (start[:, None, :] + along).reshape(-1, 2).astype(np.float32)
    assert scan.min() >= 1 and np.floor(scan).max() <= obj - pw - 1
    psi = ((0.75 + 0.25 * rng.random((1, obj, obj))) * np.exp(
        1j * np.pi * (rng.random((1, obj, obj)) - 0.5))).astype(np.complex64)
    w = window(pw)
    probe = np.stack([
        amp * w * np.exp(1j * np.pi * rng.random((pw, pw))) / (m + 1)
        for m in range(S)
    ])[None, None].astype(np.complex64)
    data = simulate(det, probe, scan, psi, fly).astype(np.float32)
    psi0 = (mix * psi + (1 - mix) * 0.5).astype(np.complex64)
    probe0 = (dim * probe).astype(np.complex64)
    return dict(scan=scan, psi=psi, probe=probe, data=data, psi0=psi0,
                probe0=probe0)


def block_mask(det):
    """A block of unmeasured pixels, a dead row and a dead column."""
    mask = np.ones((det, det), dtype=bool)
    mask[det // 4:det // 4 + max(2, det // 8), det // 2:det // 2 + det // 4] = False
    mask[det // 3, :] = False
    mask[:, (2 * det) // 5] = False
    return mask


def masked(data, mask):
    """The counts with NaN where nothing was measured."""
    out = np.array(data, dtype=np.float32, copy=True)
    out[:, ~mask] = np.nan
    return out


def run_model(case, model, use_mask, recover_probe, epochs=2, cg_iter=2):
    """The float64 cgrad on a named SOLVER_CASES problem, one minibatch.
    Returns (state, problem, mask)."""
    kw = SOLVER_CASES[case]
    P = problem(**kw)
    mask = block_mask(kw["det"]) if use_mask else None
    data = masked(P["data"], mask) if use_mask else P["data"]
    N = len(P["scan"])
    state = dict(psi=P["psi0"].copy(), probe=P["probe0"].copy(),
                 scan=P["scan"], costs=[])
    for _ in range(epochs):
        state = cgrad(state, data, [np.arange(N)], detector_shape=kw["det"],
                      fly=kw["fly"], model=model, mask=mask, cg_iter=cg_iter,
                      recover_probe=recover_probe)
    return state, dict(P, data=data), mask
