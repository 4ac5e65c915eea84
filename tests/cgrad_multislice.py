"""float64 NumPy model of cgrad on an object of several slices.

    beam_0[n, s]  = P_s
    e_d[n, s]     = patch_n(O_d) beam_d[n, s]
    beam_{d+1}    = Fr(e_d) = IFFT2(FFT2(e_d) Hprop)          (d < D - 1)
    far[n, s]     = FFT2(e_{D-1}[n, s]),   I_n = sum_s |far[n, s]|^2
    cost          = mean over positions of each pattern's mean over its
                    measured pixels of the gaussian / Poisson term
                    (tests/cgrad_models.py)

and the EXACT gradient, the adjoint through every slice:

    g_{D-1} = IFFT2(far factor)      (factor: cgrad_models._FACTORS on the
                                      measured pixels, 0 elsewhere)
    d = D-1 ... 0:  dO_d = sum_n patch_adj_n(sum_s conj(beam_d[n, s]) g_d[n, s])
                    w    = conj(patch_n(O_d)) g_d
                    g_{d-1} = Fr^H(w)  (d > 0),   dP_s = sum_n w[n, s]  (d = 0)

with NO division by the number of slices (the reference's Multislice.adj
divides the object part by D; the solver must not).  complex128 throughout:
the patch gather / scatter of oracle.operators keeps the dtype (bilinear
weights in float32, as everywhere); the transforms are numpy.fft's
(oracle.operators' round to complex64).  Unmeasured counts (NaN in the tests)
are selected away, never multiplied.  The conjugate gradient and its line
search are tests/fly_scan.py's: every comparison of a search leaves its
relative margin behind."""
import numpy as np

from oracle import operators as ops

import cgrad_models as cm
import fly_scan as fs

_TERMS = cm._TERMS
_FACTORS = cm._FACTORS

PIXEL = 1e-8  # 10 nm
WAVELENGTH = 1e-10
DISTANCE = 2e-6


def propagator(pw):
    """The Fresnel propagator between two slices, FFT order, the complex64
    values the operator holds, as complex128."""
    return ops.fresnel_spectrum_propagator(
        (pw, pw), (pw * PIXEL, pw * PIXEL), DISTANCE,
        WAVELENGTH).astype(np.complex128)


def _fft2(x):
    return np.fft.fft2(x, axes=(-2, -1), norm="ortho")


def _ifft2(x):
    return np.fft.ifft2(x, axes=(-2, -1), norm="ortho")


def fresnel(x, H):
    return _ifft2(_fft2(x) * H)


def fresnel_adj(x, H):
    return _ifft2(_fft2(x) * np.conj(H))


def _shared(probe):
    """(1, S, pw, pw) complex128 from (1, 1, S, pw, pw)."""
    return np.asarray(probe, np.complex128)[..., 0, :, :, :]


# ------------------------------------------------------------- the operator
def incident(probe, scan, psi, H):
    """The probes incident on every slice: [(1|N, S, pw, pw)] * D."""
    psi = np.asarray(psi, np.complex128)
    beams = [_shared(probe)]
    for d in range(len(psi) - 1):
        beams.append(fresnel(ops.convolution_fwd(psi[d], scan, beams[d]), H))
    return beams


def fwd(probe, scan, psi, H):
    """far (N, S, det, det) complex128 and the incident probes."""
    psi = np.asarray(psi, np.complex128)
    beams = incident(probe, scan, psi, H)
    return _fft2(ops.convolution_fwd(psi[-1], scan, beams[-1])), beams


def step_back(g, scan, layer, beam):
    """One slice of the way back: (sum_s conj(beam) g  (N, pw, pw),
    conj(patch(layer)) g  (N, S, pw, pw))."""
    N = len(scan)
    beam = np.broadcast_to(beam, (N, *beam.shape[-3:]))
    objproj = np.sum(np.conj(beam) * g, axis=-3)
    w = ops.convolution_adj_probe(g, scan, np.asarray(layer, np.complex128),
                                  g.shape[-1])
    return objproj, w


def adj(far, beams, scan, psi, H):
    """The adjoint of `fwd` at the far-plane array `far`: (psi_adj (D, H, W),
    probe_adj (1, 1, S, pw, pw) summed over the positions)."""
    psi = np.asarray(psi, np.complex128)
    N, D = len(scan), len(psi)
    g = _ifft2(far)
    psi_adj = np.zeros_like(psi)
    for d in range(D - 1, -1, -1):
        beam = np.broadcast_to(beams[d], (N, *beams[d].shape[-3:]))
        psi_adj[d] = ops.convolution_adj(g, scan, beam, psi.shape[-2],
                                         psi.shape[-1])
        w = ops.convolution_adj_probe(g, scan, psi[d], g.shape[-1])
        if d > 0:
            g = fresnel_adj(w, H)
    return psi_adj, np.sum(w, axis=0)[None, None]


# ------------------------------------------------- intensity, cost, gradient
def intensity(far):
    return np.sum(far.real**2 + far.imag**2, axis=-3)


def simulate(probe, scan, psi, H):
    return intensity(fwd(probe, scan, psi, H)[0])


def cost(model, data, psi, scan, probe, H, mask=None):
    inten = intensity(fwd(probe, scan, psi, H)[0])
    return float(np.mean(cm.cost_each(model, data, inten, mask)))


def farplane_gradient(model, data, far, mask=None):
    with np.errstate(invalid="ignore", divide="ignore"):
        f = cm._select(mask, _FACTORS[model](np.asarray(data, np.float64),
                                             intensity(far)))
    return far * f[:, None]


def gradients(model, data, psi, scan, probe, H, mask=None):
    """(d cost / d psi (D, H, W), d cost / d probe (1, 1, S, pw, pw)), both
    unnormalised: cost' = 2 / (N n_measured) Re <gradient, direction>."""
    far, beams = fwd(probe, scan, psi, H)
    return adj(farplane_gradient(model, data, far, mask), beams, scan, psi, H)


def grad_psi(*args, **kw):
    return gradients(*args, **kw)[0]


def grad_probe(*args, **kw):
    return gradients(*args, **kw)[1]


# --------------------------------------------------------------- the solver
def cgrad(state, data, batches, *, H, model, mask=None, cg_iter=2,
          step_length=1.0, recover_probe=True):
    """One epoch: per minibatch, one CG over all slices, then one over the
    probe, `cg_iter` iterations each.  state["margins"] collects the relative
    margin of every line-search comparison."""
    psi = np.asarray(state["psi"], np.complex128)
    probe = np.asarray(state["probe"], np.complex128)
    scan = state["scan"]
    margins = state.setdefault("margins", [])
    batch_cost = []
    for b in batches:
        lo, hi = int(b[0]), int(b[0]) + len(b)
        d, s = data[lo:hi], scan[lo:hi]
        psi, c = fs.conjugate_gradient(
            psi, lambda p: cost(model, d, p, s, probe, H, mask),
            lambda p: grad_psi(model, d, p, s, probe, H, mask), cg_iter,
            step_length, margins)
        if recover_probe:
            probe, c = fs.conjugate_gradient(
                probe, lambda q: cost(model, d, psi, s, q, H, mask),
                lambda q: grad_probe(model, d, psi, s, q, H, mask), cg_iter,
                step_length, margins)
        batch_cost.append(c)
    state["costs"].append([float(np.mean(batch_cost))])
    state["psi"], state["probe"] = psi, probe
    return state


# ------------------------------------------------------------- the problems
SOLVER_CASES = {
    # name: problem; seeds chosen so that every comparison of the float64
    # line searches, over both epochs and every (model, mask, probe) variant,
    # is decided by a relative margin >= fly_scan.MIN_MARGIN
    # (test_cgrad_multislice_cpu.py asserts it).  The probe amplitudes at 32^2
    # put the mean count near e, where the Poisson term d - d log d of a
    # solved pattern vanishes: the cost is then mostly what the solver
    # changes, and a comparison is not decided in the fourth digit of an offset
    "general32_d2": dict(obj=72, pw=32, S=2, D=2, N=9, seed=3, amp=1.6),
    "general32_d3": dict(obj=72, pw=32, S=2, D=3, N=9, seed=1, amp=1.9),
    "fused128_d2": dict(obj=200, pw=128, S=2, D=2, N=12, seed=1),
}
SOLVER_VARIANTS = fs.SOLVER_VARIANTS
MIN_MARGIN = fs.MIN_MARGIN


def positions(obj, pw, N, rng):
    """N fractional positions on a jittered grid; the first sits at the first
    allowed corner (floor = 1), the last at the last allowed one (floor =
    obj - pw - 1)."""
    side = int(np.ceil(np.sqrt(N)))
    room = obj - pw - 2  # floors in [1, obj - pw - 1]
    pitch = (room - 1.0) / max(side - 1, 1)
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"),
                  -1).reshape(-1, 2)[:N]
    scan = 1 + pitch * ij + 0.9 * rng.random((N, 2))
    scan[0] = 1 + 0.9 * rng.random(2)
    scan[-1] = obj - pw - 1 + 0.9 * rng.random(2)
    scan = scan.astype(np.float32)
    assert np.floor(scan).min() == 1 and np.floor(scan).max() == obj - pw - 1
    return scan


def problem(obj, pw, S, D, N, seed, amp=1.0, mix=0.3, dim=0.6):
    """A seeded multislice problem.  Returns dict(scan (N, 2) f32, psi
    (D, obj, obj) c64 the true slices -- mutually different, about 0.3 rad of
    phase noise each --, probe (1, 1, S, pw, pw) c64, H the propagator, data
    (N, pw, pw) f32, psi0 / probe0 the first iterates)."""
    rng = np.random.default_rng(seed)
    scan = positions(obj, pw, N, rng)
    psi = ((0.8 + 0.2 * rng.random((D, obj, obj))) * np.exp(
        0.3j * rng.standard_normal((D, obj, obj)))).astype(np.complex64)
    w = fs.window(pw)
    probe = np.stack([
        amp * w * np.exp(1j * np.pi * rng.random((pw, pw))) / (m + 1)
        for m in range(S)
    ])[None, None].astype(np.complex64)
    H = propagator(pw)
    data = simulate(probe, scan, psi, H).astype(np.float32)
    psi0 = (mix * psi + (1 - mix) * 0.9).astype(np.complex64)
    probe0 = (dim * probe).astype(np.complex64)
    return dict(scan=scan, psi=psi, probe=probe, H=H, data=data, psi0=psi0,
                probe0=probe0)


_RUNS = {}


def run_model(case, model, use_mask, recover_probe, epochs=2, cg_iter=2):
    """The float64 cgrad on a named SOLVER_CASES problem, one minibatch;
    computed once per argument list.  Returns (state, problem, mask)."""
    key = (case, model, use_mask, recover_probe, epochs, cg_iter)
    if key not in _RUNS:
        kw = SOLVER_CASES[case]
        P = problem(**kw)
        mask = fs.block_mask(kw["pw"]) if use_mask else None
        data = fs.masked(P["data"], mask) if use_mask else P["data"]
        N = len(P["scan"])
        state = dict(psi=P["psi0"].copy(), probe=P["probe0"].copy(),
                     scan=P["scan"], costs=[])
        for _ in range(epochs):
            state = cgrad(state, data, [np.arange(N)], H=P["H"], model=model,
                          mask=mask, cg_iter=cg_iter,
                          recover_probe=recover_probe)
        _RUNS[key] = (state, dict(P, data=data), mask)
    return _RUNS[key]
