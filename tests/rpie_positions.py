"""rpie with position correction in NumPy, composed from the oracle: the
forward model, the adjoints and `rpie_update` of oracle.operators /
oracle.solvers, the shift estimate of oracle.position summed over the probe
modes, `update_position` and the affine regularisation.  Shared by
test_rpie_positions_cpu.py (which pins it to `oracle.solvers.rpie`) and
test_rpie_positions_gpu.py (which holds the solver to it)."""
import numpy as np

from oracle import operators as ops
from oracle import position as opos
from oracle import solvers as osol


def minibatch(data, psi, scan, probe, eigen_probe, eigen_weights, lo, hi,
              psi_num, *, detector_shape, measured_pixels, propagator=None,
              noise_model="gaussian", unmeasured_pixels_scaling=1.0,
              recover_psi=True, recover_probe=True, step_length_start=0.5,
              step_length_usemodes="all_modes", step_length_weight=0.5,
              want_terms=False):
    """One minibatch [lo, hi) of rpie: costs, numerators, eigen weights, and
    (want_terms) numerator / denominator of the shift estimates (n, 2)."""
    pw, S, D = probe.shape[-1], probe.shape[-3], psi.shape[0]
    n = hi - lo
    pad = (detector_shape - pw) // 2
    sc = scan[lo:hi]
    beam = osol.get_varying_probe(
        probe, eigen_probe, None if eigen_weights is None else
        eigen_weights[lo:hi])
    if beam.shape[0] == 1 and n > 1:
        beam = np.broadcast_to(beam, (n, *beam.shape[1:])).copy()
    if D == 1:
        far = ops.ptycho_fwd(beam, sc, psi, detector_shape, "ortho")
        incident = beam[None, :, 0]
    else:
        far, incident = ops.ptycho_fwd_intermediate(beam, sc, psi, propagator,
                                                    "ortho")
    inten = np.sum(np.square(np.abs(far)), axis=tuple(range(1, far.ndim - 2)))
    d = data[lo:hi].astype(np.float32)
    costs = getattr(ops, f"{noise_model}_each_pattern")(
        d[:, measured_pixels][:, None, :],
        inten[:, measured_pixels][:, None, :])
    if noise_model == "poisson":
        with np.errstate(invalid="ignore", divide="ignore"):
            xi = (1 - d / inten)[:, None, None, ...]
            grad_cost = far * xi
            step = np.full((far.shape[0], 1, far.shape[2], 1, 1),
                           np.float32(step_length_start), dtype=np.float32)
            if step_length_usemodes == "dominant_mode":
                step = osol.poisson_steplength_dominant_mode(
                    xi, inten, d, measured_pixels, step, step_length_weight)
            else:
                step = osol.poisson_steplength_all_modes(
                    xi, np.square(np.abs(far)), inten, d, measured_pixels,
                    step, step_length_weight)
            far[..., measured_pixels] = (-step * grad_cost)[...,
                                                            measured_pixels]
    else:
        far[..., measured_pixels] = -ops.gaussian_grad(
            d, far, inten)[..., measured_pixels]
    far[..., np.logical_not(measured_pixels)] *= np.float32(
        unmeasured_pixels_scaling - 1.0)
    chi = np.ascontiguousarray(
        ops.propagation_adj(far, "ortho")[..., pad:pad + pw, pad:pad + pw])
    probe_num = np.zeros((D, *probe.shape), dtype=probe.dtype)
    if recover_psi:
        for t in range(D - 1, -1, -1):
            g = (np.conj(incident[t][:, None]) * chi / S).reshape(n * S, pw, pw)
            psi_num[t] = ops.patch_adj(patches=g, images=psi_num[t],
                                       positions=sc, nrepeat=S)
            o_t = ops.patch_fwd(psi[t], sc,
                                patch_width=pw)[..., None, None, :, :]
            probe_num[t] += np.sum(np.conj(o_t) * chi, axis=-5, keepdims=True)
            if t == 0:
                break
            chi = ops.fresnel_adj(chi, propagator, "ortho")
    o_0 = ops.patch_fwd(psi[0], sc, patch_width=pw)[..., None, None, :, :]
    terms = None
    if want_terms:
        # chi has reached the first slice; every mode contributes
        terms = [np.zeros((n, 2), np.float32), np.zeros((n, 2), np.float32)]
        for m in range(S):
            a, b = opos.position_update_terms(o_0, incident[0][:, None], chi,
                                              m)
            terms[0] += a
            terms[1] += b
    if recover_probe and eigen_weights is not None:
        op0 = o_0 * probe[..., 0:1, :, :]
        a = np.sum(np.real(np.conj(op0) * chi[..., 0:1, :, :]), axis=(-1, -2))
        b = np.sum(np.abs(op0)**2, axis=(-1, -2))
        eigen_weights[lo:hi, 0:1, 0:1] += 0.1 * (a / b)
    return costs, psi_num, probe_num, eigen_weights, terms


def epoch(state, data, batches, *, epoch, detector_shape, alpha=0.05,
          batch_method="compact", measured_pixels=None, rng=None,
          recover_psi=True, recover_probe=True, probe_update_start=0,
          propagator=None, **kw):
    """One epoch of rpie; with state["position"] set, one position update
    after its last minibatch (every minibatch sees the old positions)."""
    nb = len(batches)
    if measured_pixels is None:
        measured_pixels = np.ones((detector_shape, detector_shape), dtype=bool)
    recover_probe = recover_probe and epoch >= probe_update_start
    order = (range(nb) if batch_method == "compact" else
             (rng or np.random.default_rng()).permutation(nb))
    pos = state.get("position")
    N = len(state["scan"])
    num, den = np.zeros((N, 2), np.float32), np.zeros((N, 2), np.float32)
    psi_num = probe_num = None
    batch_cost = np.empty(nb, dtype=np.float32)
    upd = dict(alpha=alpha, recover_psi=recover_psi,
               recover_probe=recover_probe)
    for b in order:
        lo = int(batches[b][0])
        hi = lo + len(batches[b])
        if psi_num is None:
            psi_num = np.zeros_like(state["psi"])
        costs, psi_num, probe_num, state["eigen_weights"], terms = minibatch(
            data, state["psi"], state["scan"], state["probe"],
            state.get("eigen_probe"), state.get("eigen_weights"), lo, hi,
            psi_num, detector_shape=detector_shape,
            measured_pixels=measured_pixels, propagator=propagator,
            recover_psi=recover_psi, recover_probe=recover_probe,
            want_terms=pos is not None, **kw)
        if terms is not None:
            num[lo:hi], den[lo:hi] = terms
        batch_cost[b] = np.mean(costs)
        if batch_method != "compact":
            state = osol.rpie_update(state, psi_num, probe_num, **upd)
            psi_num = probe_num = None
    state["costs"].append([float(batch_cost.mean())])
    if pos is not None:
        state["scan"] = opos.update_position(state["scan"], pos, num, den,
                                             alpha=alpha, epoch=epoch)
    if batch_method == "compact":
        state = osol.rpie_update(
            state, psi_num, probe_num,
            errors=[float(x[0]) for x in state["costs"][-3:]], **upd)
    if state.get("eigen_weights") is not None:
        w = state["eigen_weights"]
        state["eigen_weights"] = (w / osol.mnorm(
            w, axis=-3, keepdims=True)).astype(np.float32)
    return state


def iterate(state, data, batches, num_iter, *, detector_shape,
            force_orthogonality=False, rescale_period=10, after_epoch=None,
            **kw):
    """The epoch driver around `epoch`: probe constraints, preconditioners,
    the solver, the ambiguity rescale, the affine regularisation."""
    for _ in range(num_iter):
        e = len(state["costs"])
        if kw.get("recover_probe", True) and e >= kw.get(
                "probe_update_start", 0):
            if force_orthogonality:
                state["probe"], _ = osol.orthogonalize_eig(state["probe"])
            if state.get("eigen_probe") is not None:
                state["eigen_probe"], state["eigen_weights"] = (
                    osol.constrain_variable_probe(state["eigen_probe"],
                                                  state["eigen_weights"]))
        state["psi_precond"] = osol.psi_preconditioner(
            state["psi"], state["probe"], state["scan"],
            propagator=kw.get("propagator"))
        state["probe_precond"] = osol.probe_preconditioner(
            state["psi"], state["probe"], state["scan"])
        state = epoch(state, data, batches, epoch=e,
                      detector_shape=detector_shape, **kw)
        if len(state["costs"]) % rescale_period == 0:
            state["psi"], state["probe"] = osol.remove_object_ambiguity(
                state["psi"], state["probe"], state["psi_precond"])
        if state.get("position") is not None:
            state["scan"] = opos.affine_position_regularization(
                state["scan"], state["position"],
                kw.get("rng") or np.random.default_rng()).astype(np.float32)
        if after_epoch is not None:
            after_epoch(state)
    return state


def position_state(scan, **options):
    """The oracle's form of PositionOptions(scan, **options)."""
    return dict(initial_scan=scan.copy(),
                momentum=np.zeros((len(scan), 4), dtype=np.float32), **options)


def jitter(rng, shape, amplitude=0.7):
    """Uniform errors in [-amplitude, amplitude) px, their mean removed."""
    e = ((rng.random(shape) - 0.5) * 2 * amplitude).astype(np.float32)
    return e - e.mean(axis=0)


def position_error(scan, true):
    """Mean absolute position error, a common shift removed."""
    return float(np.abs((scan - scan.mean(0)) - (true - true.mean(0))).mean())


def smooth_object(rng, depth, HW, sigma=1.5):
    """A random object with structure a few pixels wide (gradients carry
    position information), amplitude 0.75 ... 1, phase within +-pi/2."""
    from scipy.ndimage import gaussian_filter
    raw = ((0.75 + 0.25 * rng.random((depth, HW, HW))) * np.exp(
        1j * np.pi * (rng.random((depth, HW, HW)) - 0.5)))
    return (gaussian_filter(raw.real, (0, sigma, sigma)) +
            1j * gaussian_filter(raw.imag, (0, sigma, sigma))).astype(
                np.complex64)


def grid_problem(det, S, grid, *, pitch=4.0, seed=0, depth=1, propagator=None):
    """grid x grid positions at `pitch` px, a smooth object of `depth` slices,
    S probe modes filling the detector: (true scan, object, probe, data)."""
    rng = np.random.default_rng(seed)
    ij = np.stack(np.meshgrid(np.arange(grid), np.arange(grid),
                              indexing="ij"), -1).reshape(-1, 2)
    true = (6 + pitch * ij + rng.random((grid * grid, 2))).astype(np.float32)
    HW = int(true.max()) + det + 8
    psi = smooth_object(rng, depth, HW)
    w = osol.gaussian_probe(det, rin=0.6)
    probe = np.stack([w * np.exp(1j * np.pi * rng.random((det, det))) / (m + 1)
                      for m in range(S)])[None, None].astype(np.complex64)
    data = ops.intensity_from_farplane(
        ops.ptycho_fwd(probe, true, psi, det, propagator=propagator)).astype(
            np.float32)
    return true, psi, probe, data, rng
