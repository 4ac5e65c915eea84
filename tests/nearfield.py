"""float64 NumPy model of near-field (Fresnel, holographic) ptychography.

The detector sits a finite distance behind the sample, probe window =
detector, and the wave on the detector is one Fresnel step of the exit wave:

    w[n, s] = IFFT2(H . FFT2(patch_n(psi) x probe_s))     (norm: the operator's)
    I_f     = sum_{j < fly} sum_{s < S} |w[f * fly + j, s]|^2

H (det, det) complex, in FFT order, used as given.  Costs and the gradient
factor are those of tests/fly_scan.py (a frame's cost is the mean of the
model's term over its measured pixels; unmeasured counts, NaN in the tests, are
selected away); the gradient goes through the EXACT adjoint
IFFT2(conj(H) . FFT2(.)) and the adjoint of the gather.  Built on the gather /
scatter of tests/fly_scan.py (oracle.operators, bilinear weights in float32)
and, for the scan gradient, on tests/autograd_model.py.

`pass1` / `pass2` restate the two-pass decomposition of the column transform
(csrc/fft_engine2.h) on one (det, det) plane, so that the entry
`tike_nearfield_plane_gradient` can be held to the model for a GIVEN hand-off:
its input is the input of an inverse pass 2, its output that of a forward
pass 1."""
import functools

import numpy as np
import scipy.fft

from oracle import operators as ops

import fly_scan as fs

MODELS = ("gaussian", "poisson")


# ------------------------------------------------------------- the operator
def propagate(x, H, adjoint=False, norm="ortho"):
    """IFFT2(H . FFT2(x)) over the last two axes, conj(H) for the adjoint."""
    H = np.asarray(H, np.complex128)
    X = scipy.fft.fft2(np.asarray(x, np.complex128), axes=(-2, -1), norm=norm)
    return scipy.fft.ifft2(X * (H.conj() if adjoint else H), axes=(-2, -1),
                           norm=norm)


def exit_waves(probe, scan, psi, det):
    """(N, S, det, det) complex128: patch x probe, probe window = detector."""
    assert probe.shape[-1] == det, (probe.shape, det)
    return ops.convolution_fwd(np.asarray(psi[0], np.complex128), scan,
                               np.asarray(probe[..., 0, :, :, :],
                                          np.complex128), det)


def fwd(probe, scan, psi, det, H):
    """The detector-plane waves (N, 1, S, det, det) complex128."""
    return propagate(exit_waves(probe, scan, psi, det), H)[..., None, :, :, :]


def adj(w, probe, scan, psi, H, want=(True, True)):
    """(psi_adj (1, H, W), probe_adj (N, 1, S, pw, pw)) complex128: the exact
    adjoint of `fwd` in the object and in the probe (None where not wanted)."""
    near = propagate(np.asarray(w)[..., 0, :, :, :], H, adjoint=True)
    p = np.asarray(probe[..., 0, :, :, :], np.complex128)
    p = np.broadcast_to(p, (len(scan), *p.shape[-3:]))
    psi = np.asarray(psi, np.complex128)
    psi_adj = probe_adj = None
    if want[0]:
        psi_adj = ops.convolution_adj(near, scan, p, psi.shape[-2],
                                      psi.shape[-1])[None]
    if want[1]:
        probe_adj = ops.convolution_adj_probe(near, scan, psi[0], p.shape[-1])[
            ..., None, :, :, :]
    return psi_adj, probe_adj


# ------------------------------------------------- intensity, cost, gradient
def simulate(det, probe, scan, psi, fly, H):
    return fs.frame_intensity(fwd(probe, scan, psi, det, H), fly)


def cost(model, data, psi, scan, probe, det, fly, H, mask=None):
    inten = simulate(det, probe, scan, psi, fly, H)
    return float(np.mean(fs.cost_each(model, data, inten, mask)))


def plane_gradient(model, data, psi, scan, probe, det, fly, H, mask=None):
    return fs.farplane_gradient(model, data, fwd(probe, scan, psi, det, H),
                                fly, mask)


def grad_psi(model, data, psi, scan, probe, det, fly, H, mask=None):
    g = plane_gradient(model, data, psi, scan, probe, det, fly, H, mask)
    return adj(g, probe, scan, psi, H, (True, False))[0]


def grad_probe(model, data, psi, scan, probe, det, fly, H, mask=None):
    g = plane_gradient(model, data, psi, scan, probe, det, fly, H, mask)
    return np.sum(adj(g, probe, scan, psi, H, (False, True))[1], axis=0,
                  keepdims=True)


def objproj(model, data, psi, scan, probe, det, fly, H, mask=None):
    """(N, det, det): sum_s conj(probe_s) x the adjoint-propagated plane
    gradient -- what the adjoint of the gather, and the scan gradient, take."""
    g = plane_gradient(model, data, psi, scan, probe, det, fly, H, mask)
    near = propagate(g[..., 0, :, :, :], H, adjoint=True)
    p = np.asarray(probe[0, 0], np.complex128)
    return (p.conj()[None] * near).sum(axis=1)


def autograd_gradients(model, data, psi, scan, probe, det, fly, H, mask=None):
    """dict(psi, probe, scan) of mean_f cost_f as `torch.autograd` defines
    them for complex leaves (2 x the conjugate Wirtinger derivative; the scan's
    is the plain real derivative), the costs normalised by the measured pixels
    and the frames."""
    import torch

    import autograd_model as am
    nframe = len(scan) // fly
    n = det * det if mask is None else int(mask.sum())
    k = 2.0 / (n * nframe)
    proj = objproj(model, data, psi, scan, probe, det, fly, H, mask)
    gs, A = am.scan_gradient(torch.from_numpy(proj),
                             torch.from_numpy(np.asarray(psi, np.complex128)),
                             torch.from_numpy(np.asarray(scan, np.float32)).to(
                                 torch.float64))
    return dict(
        psi=k * grad_psi(model, data, psi, scan, probe, det, fly, H, mask),
        probe=k * grad_probe(model, data, psi, scan, probe, det, fly, H, mask),
        scan=k * gs.numpy(), A=k * A.numpy())


# ------------------------------------------ the two passes of fft_engine2.h
def pass1(x, inverse=False):
    """Pass 1 of the (unnormalised) two-pass transform of (..., N, N) planes:
    row transforms, for every r < N / 16 a length-16 transform over the rows
    {r + (N / 16) y2}, the twiddle w_N^(r k1), stored at the rows 16 r + k1."""
    x = np.asarray(x, np.complex128)
    N = x.shape[-1]
    RB = N // 16
    f = scipy.fft.ifft if inverse else scipy.fft.fft
    kw = dict(norm="forward") if inverse else {}
    X = f(x, axis=-1, **kw)
    X = X.reshape(*x.shape[:-2], 16, RB, N)  # [y2, r, column]
    Y = f(X, axis=-3, **kw)  # [k1, r, column]
    sign = 2j if inverse else -2j
    tw = np.exp(sign * np.pi * np.outer(np.arange(16), np.arange(RB)) / N)
    Y = Y * tw[:, :, None]
    return np.swapaxes(Y, -3, -2).reshape(x.shape)  # row 16 r + k1


def pass2(y, inverse=False):
    """Pass 2: for every k1 < 16 a length-(N / 16) transform over the rows
    {16 r + k1}, stored at the rows {k1 + 16 k2}.  pass2(pass1(x)) is the
    unnormalised transform of x."""
    y = np.asarray(y, np.complex128)
    N = y.shape[-1]
    RB = N // 16
    Y = y.reshape(*y.shape[:-2], RB, 16, N)  # [r, k1, column]
    f = scipy.fft.ifft if inverse else scipy.fft.fft
    kw = dict(norm="forward") if inverse else {}
    return f(Y, axis=-3, **kw).reshape(y.shape)  # [k2, k1] = row k1 + 16 k2


def entry(work, data, model, fly, S, mask=None, upstream=None, inv_scale=1.0,
          scale=1.0):
    """What `tike_nearfield_plane_gradient` makes of a hand-off `work`
    (nframe * fly, S, det, det): dict(w, intensity, costs, g, out)."""
    work = np.asarray(work, np.complex128)
    det = work.shape[-1]
    nframe = work.shape[0] // fly
    w = inv_scale * pass2(work, inverse=True)
    inten = fs.frame_intensity(w[:, None], fly)
    n = det * det if mask is None else int(mask.sum())
    up = np.ones(nframe) if upstream is None else np.asarray(upstream,
                                                             np.float64)
    costs = fs.cost_each(model, data, inten, mask)
    with np.errstate(invalid="ignore", divide="ignore"):
        lp = fs._select(mask, fs._FACTORS[model](np.asarray(data, np.float64),
                                                 inten))
    g = scale * up[:, None, None] / n * lp
    gw = w * np.repeat(g, fly, axis=0)[:, None]
    return dict(w=w, intensity=inten, costs=costs, g=g, out=pass1(gw))


# --------------------------------------------------------------- the solver
def cgrad(state, data, batches, *, detector_shape, fly, model, H, mask=None,
          cg_iter=2, step_length=1.0, recover_probe=False):
    """One cgrad epoch (tests/fly_scan.py's, with this module's cost and
    gradients).  state["margins"] collects the relative margin of every
    line-search comparison, state["costs"] the epoch's mean cost."""
    det = detector_shape
    psi = np.asarray(state["psi"], np.complex128)
    probe = np.asarray(state["probe"], np.complex128)
    scan = state["scan"]
    margins = state.setdefault("margins", [])
    batch_cost = []
    for b in batches:
        lo, hi = int(b[0]), int(b[0]) + len(b)
        assert lo % fly == 0 and hi % fly == 0
        sc, d = scan[lo:hi], data[lo // fly:hi // fly]
        psi, c = fs.conjugate_gradient(
            psi,
            lambda x: cost(model, d, x, sc, probe, det, fly, H, mask),
            lambda x: grad_psi(model, d, x, sc, probe, det, fly, H, mask),
            cg_iter, step_length, margins)
        if recover_probe:
            probe, c = fs.conjugate_gradient(
                probe,
                lambda x: cost(model, d, psi, sc, x, det, fly, H, mask),
                lambda x: grad_probe(model, d, psi, sc, x, det, fly, H, mask),
                cg_iter, step_length, margins)
        batch_cost.append(c)
    state["costs"].append([float(np.mean(batch_cost))])
    state["psi"], state["probe"] = psi, probe
    return state


# ------------------------------------------------------------- test problems
def propagator(det, nyquist_phase=3 * np.pi):
    """A paraxial Fresnel propagator in FFT order, complex64: the phase
    -nyquist_phase (fy^2 + fx^2) / (1/2)^2 / 2 with f in cycles per pixel, i.e.
    nyquist_phase / 2 per axis at Nyquist."""
    f = np.fft.fftfreq(det)
    q = (f[:, None]**2 + f[None, :]**2) / 0.25
    return np.exp(-0.5j * nyquist_phase * q).astype(np.complex64)


def smooth(shape, rng, sigma):
    """A smooth real field of unit maximum (white noise, Gaussian low-pass)."""
    from scipy.ndimage import gaussian_filter
    x = gaussian_filter(rng.standard_normal(shape), sigma, mode="wrap")
    return x / np.abs(x).max()


def problem(det, S, fly, nframe, seed, step=3.0, phase=0.3):
    """A well-conditioned near-field problem, as a real frame is: a probe of
    amplitude near 1 with a smooth random phase filling the frame (the modes
    behind the first weaker), a weak-phase object, positions with fractions.
    dict(psi (1, H, W), probe (1, 1, S, det, det), scan (nframe * fly, 2),
    H (det, det)) in float32 / complex64."""
    rng = np.random.default_rng(seed)
    N = nframe * fly
    side = int(np.ceil(np.sqrt(N)))
    span = int(np.ceil(step * side)) + 4
    Hh = det + span + 2
    psi = np.exp(1j * phase * smooth((Hh, Hh), rng, 3.0)) * (
        1 - 0.05 * np.abs(smooth((Hh, Hh), rng, 4.0)))
    probe = np.empty((1, 1, S, det, det), np.complex128)
    for s in range(S):
        amp = (1 + 0.1 * smooth((det, det), rng, 4.0)) * (0.5**s)
        probe[0, 0, s] = amp * np.exp(2j * smooth((det, det), rng, 6.0))
    idx = np.arange(N)
    scan = np.stack([1.3 + step * (idx // side), 1.7 + step * (idx % side)],
                    axis=1) + rng.uniform(0, 0.9, (N, 2))
    return dict(psi=psi[None].astype(np.complex64),
                probe=probe.astype(np.complex64),
                scan=scan.astype(np.float32), H=propagator(det))


SOLVER = dict(det=128, S=2, nframe={1: 64, 2: 32}, seed=11)
"""The problem of the solver tests: 64 positions at 128^2, two modes."""


def solver_problem(fly):
    """`problem` with its frames, the first iterate (a flat object, the probe
    dimmed by a tenth) and a module-gap mask."""
    P = problem(SOLVER["det"], SOLVER["S"], fly, SOLVER["nframe"][fly],
                SOLVER["seed"] + fly, step=5.0)
    det = SOLVER["det"]
    data = simulate(det, P["probe"], P["scan"], P["psi"], fly,
                    P["H"]).astype(np.float32)
    mask = np.ones((det, det), bool)
    mask[det // 2 - 1:det // 2 + 1, :] = False
    return dict(P, data=fs.masked(data, mask), mask=mask,
                psi0=np.ones_like(P["psi"]),
                probe0=(0.9 * P["probe"]).astype(np.complex64))


STEP_LENGTH = 1.0 / 32
"""The first step of the solver tests' line searches: the float64 searches
accept it or its half, so a run costs few evaluations of the model."""


@functools.lru_cache(maxsize=None)
def run_model(fly, epochs=2, cg_iter=2, model="gaussian"):
    """Two epochs of the float64 cgrad on `solver_problem(fly)`, one
    minibatch, the object recovered (the probe's gradient is held to the model
    by the route tests): (state, problem).  Computed once."""
    P = solver_problem(fly)
    N = len(P["scan"])
    state = dict(psi=P["psi0"].copy(), probe=P["probe0"].copy(),
                 scan=P["scan"], costs=[])
    for _ in range(epochs):
        state = cgrad(state, P["data"], [np.arange(N)],
                      detector_shape=SOLVER["det"], fly=fly, model=model,
                      H=P["H"], mask=P["mask"], cg_iter=cg_iter,
                      step_length=STEP_LENGTH, recover_probe=False)
    return state, P
