"""float64 NumPy model of detector binning: the far plane is `B` times finer
than the measured pixels, and a measured pixel is the incoherent sum over its
B x B far-plane pixels (and, as in tests/fly_scan.py, over the `fly` positions
of its frame and the modes).  det: far-plane width, w = det // B: data width.
In the stored (FFT-shifted) layout

    I[f, U, V] = sum_{u, v < B} sum_{j < fly} sum_{m < S}
                 |far[f * fly + j, m, U * B + u, V * B + v]|^2
    cost[f]    = mean over the measured (U, V) of the noise model's term
    far-plane gradient: far * factor(I, d)[U, V] on every pixel of bin (U, V),
                        0 on unmeasured bins

The terms, the factors, the operator, the conjugate gradient and its line
search are those of tests/fly_scan.py; with B == 1 every function here is
that module's."""
import numpy as np

import fly_scan as fs

_TERMS = fs._TERMS
_FACTORS = fs._FACTORS


def block_sum(a, B):
    """(..., det, det) -> (..., det // B, det // B): sums over B x B blocks."""
    a = np.asarray(a)
    det = a.shape[-1]
    w = det // B
    assert w * B == det and a.shape[-2] == det
    return a.reshape(*a.shape[:-2], w, B, w, B).sum(axis=(-3, -1))


def spread(a, B):
    """(..., w, w) -> (..., w * B, w * B): a bin's value on its B x B pixels."""
    return np.repeat(np.repeat(np.asarray(a), B, axis=-2), B, axis=-1)


def frame_intensity(far, fly, B):
    """(F, w, w) float64 from far (F * fly, 1, S, det, det)."""
    return block_sum(fs.frame_intensity(far, fly), B)


cost_each = fs.cost_each
"""Per-frame mean of the model's terms over the measured DATA pixels."""


def _factor(model, data, inten, mask):
    with np.errstate(invalid="ignore", divide="ignore"):
        return fs._select(mask, _FACTORS[model](np.asarray(data, np.float64),
                                                inten))


def farplane_gradient(model, data, far, fly, B, mask=None):
    """The far-plane gradient: the factor of a bin on each of its pixels, 0
    on unmeasured bins; data (F, w, w), mask (w, w)."""
    f = _factor(model, data, frame_intensity(far, fly, B), mask)
    return far * np.repeat(spread(f, B), fly, axis=0)[:, None, None, :, :]


def cost_factor_table(model, data, far, fly, B, mask=None, upstream=None):
    """(F, det, det): upstream_f * factor / num_measured, replicated over every
    bin's pixels, 0 on unmeasured bins."""
    inten = frame_intensity(far, fly, B)
    n = inten.shape[-1] * inten.shape[-2] if mask is None else mask.sum()
    f = _factor(model, data, inten, mask)
    if upstream is not None:
        f = f * np.asarray(upstream, np.float64)[:, None, None]
    return spread(f / n, B)


def simulate(det, probe, scan, psi, fly, B):
    return frame_intensity(fs.fwd(probe, scan, psi, det), fly, B)


def cost(model, data, psi, scan, probe, det, fly, B, mask=None):
    inten = frame_intensity(fs.fwd(probe, scan, psi, det), fly, B)
    return float(np.mean(cost_each(model, data, inten, mask)))


def grad_psi(model, data, psi, scan, probe, det, fly, B, mask=None):
    g = farplane_gradient(model, data, fs.fwd(probe, scan, psi, det), fly, B,
                          mask)
    return fs.adj(g, probe, scan, psi)[0]


def grad_probe(model, data, psi, scan, probe, det, fly, B, mask=None):
    g = farplane_gradient(model, data, fs.fwd(probe, scan, psi, det), fly, B,
                          mask)
    return np.sum(fs.adj(g, probe, scan, psi)[1], axis=0, keepdims=True)


def cgrad(state, data, batches, *, detector_shape, fly, binning, model,
          mask=None, cg_iter=2, step_length=1.0, recover_probe=True):
    """fly_scan.cgrad with the binned cost and gradients: one epoch."""
    det, B = detector_shape, binning
    psi = np.asarray(state["psi"], np.complex128)
    probe = np.asarray(state["probe"], np.complex128)
    scan = state["scan"]
    margins = state.setdefault("margins", [])
    batch_cost = []
    for b in batches:
        lo, hi = int(b[0]), int(b[0]) + len(b)
        assert lo % fly == 0 and hi % fly == 0
        d, s = data[lo // fly:hi // fly], scan[lo:hi]
        psi, c = fs.conjugate_gradient(
            psi, lambda p: cost(model, d, p, s, probe, det, fly, B, mask),
            lambda p: grad_psi(model, d, p, s, probe, det, fly, B, mask),
            cg_iter, step_length, margins)
        if recover_probe:
            probe, c = fs.conjugate_gradient(
                probe, lambda q: cost(model, d, psi, s, q, det, fly, B, mask),
                lambda q: grad_probe(model, d, psi, s, q, det, fly, B, mask),
                cg_iter, step_length, margins)
        batch_cost.append(c)
    state["costs"].append([float(np.mean(batch_cost))])
    state["psi"], state["probe"] = psi, probe
    return state


# ------------------------------------------------------------- the problems
SOLVER = dict(obj=72, pw=32, det=32, S=2, B=2, side=6, seed=2, amp=1.0,
              mix=0.3, dim=0.5)
"""The reconstruction problem of the GPU test: a 6 x 6 scan, a 32^2 far plane
under 16^2 counts, a probe window as wide as the far plane -- twice the data
width, what `binning` exists for."""
SOLVER_FLY = (1, 2)
MIN_MARGIN = fs.MIN_MARGIN


def problem(fly, obj, pw, det, S, B, side, seed, amp, mix, dim):
    """A seeded problem on a side x side grid of positions, row by row; with
    fly > 1 consecutive positions of a row expose one frame.  Returns what
    fly_scan.problem returns, data (side^2 // fly, det // B, det // B)."""
    rng = np.random.default_rng(seed)
    assert (side * side) % fly == 0 and side % fly == 0
    room = obj - pw - 4
    pitch = (room - 1.0) / (side - 1)
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side),
                              indexing="ij"), -1).reshape(-1, 2)
    scan = (2 + pitch * ij + 0.9 * rng.random((side * side, 2))).astype(
        np.float32)
    assert scan.min() >= 1 and np.floor(scan).max() <= obj - pw - 1
    psi = ((0.75 + 0.25 * rng.random((1, obj, obj))) * np.exp(
        1j * np.pi * (rng.random((1, obj, obj)) - 0.5))).astype(np.complex64)
    w = fs.window(pw)
    probe = np.stack([
        amp * w * np.exp(1j * np.pi * rng.random((pw, pw))) / (m + 1)
        for m in range(S)
    ])[None, None].astype(np.complex64)
    data = simulate(det, probe, scan, psi, fly, B).astype(np.float32)
    psi0 = (mix * psi + (1 - mix) * 0.5).astype(np.complex64)
    probe0 = (dim * probe).astype(np.complex64)
    return dict(scan=scan, psi=psi, probe=probe, data=data, psi0=psi0,
                probe0=probe0)


_RUNS = {}


def run_model(fly, model, epochs=2, cg_iter=2):
    """The float64 cgrad on the SOLVER problem with the block mask at data
    resolution, one minibatch, the probe recovered: (state, problem, mask).
    Computed once per (fly, model) and shared; nobody writes into it."""
    key = (fly, model, epochs, cg_iter)
    if key not in _RUNS:
        kw = SOLVER
        P = problem(fly, **kw)
        mask = fs.block_mask(kw["det"] // kw["B"])
        data = fs.masked(P["data"], mask)
        N = len(P["scan"])
        state = dict(psi=P["psi0"].copy(), probe=P["probe0"].copy(),
                     scan=P["scan"], costs=[])
        for _ in range(epochs):
            state = cgrad(state, data, [np.arange(N)],
                          detector_shape=kw["det"], fly=fly,
                          binning=kw["B"], model=model, mask=mask,
                          cg_iter=cg_iter)
        _RUNS[key] = (state, dict(P, data=data), mask)
    return _RUNS[key]
