"""cgrad with position correction in NumPy, composed from the oracle and
tests/cgrad_models.py: per minibatch the shift estimate of
oracle.position.position_update_terms summed over the probe modes, at the
incoming iterate and the old positions, with chi = cgrad's own near-plane
descent direction (-adj(gaussian_grad), -1/2 adj(poisson_grad), 0 at the
unmeasured pixels); then the minibatch's CG (`cgrad_models.cgrad`); after the
last minibatch one `oracle.position.update_position`.  Shared by
test_cgrad_positions_cpu.py (which pins it to `cgrad_models.cgrad`) and
test_cgrad_positions_gpu.py (which holds the solver to it)."""
import numpy as np

import cgrad_models as cm
from oracle import operators as ops
from oracle import position as opos
from oracle import solvers as osol

POISSON_STEP = 0.5


def descent_direction(model, data, psi, scan, probe, det, mask=None):
    """chi (n, 1, S, pw, pw): minus the near-plane gradient of the model's
    cost on the measured pixels, times 1/2 under the Poisson model."""
    pw = probe.shape[-1]
    pad = (det - pw) // 2
    far = ops.ptycho_fwd(probe, scan, psi, det)
    g = cm.farplane_factor(model, data, far, mask).astype(far.dtype)
    chi = -ops.propagation_adj(g, "ortho")[..., pad:pad + pw, pad:pad + pw]
    if model == "poisson":
        chi = np.float32(POISSON_STEP) * chi
    return np.ascontiguousarray(chi)


def shift_terms(model, data, psi, scan, probe, det, mask=None):
    """numerator, denominator (n, 2) of the shift estimates, all modes."""
    n, S, pw = len(scan), probe.shape[-3], probe.shape[-1]
    chi = descent_direction(model, data, psi, scan, probe, det, mask)
    patches = ops.patch_fwd(psi[0], scan, patch_width=pw)[:, None, None]
    beam = np.broadcast_to(probe, (n, *probe.shape[1:]))
    num = np.zeros((n, 2), np.float32)
    den = np.zeros((n, 2), np.float32)
    for m in range(S):
        a, b = opos.position_update_terms(patches, beam, chi, m)
        num += a
        den += b
    return num, den


def epoch(state, data, batches, *, epoch, detector_shape, model, mask=None,
          cg_iter=2, step_length=1.0, alpha=0.05, recover_psi=True,
          recover_probe=True, terms_model=None):
    """One epoch of cgrad; with state["position"] set (and the epoch at or
    past its update_start) one position update after the last minibatch.
    terms_model: the model whose direction feeds the sums, if not `model`."""
    det = detector_shape
    pos = state.get("position")
    correct = pos is not None and epoch >= pos.get("update_start", 0)
    N = len(state["scan"])
    num, den = np.zeros((N, 2), np.float32), np.zeros((N, 2), np.float32)
    batch_cost = []
    for b in batches:
        lo, hi = int(b[0]), int(b[0]) + len(b)
        d, s = data[lo:hi].astype(np.float32), state["scan"][lo:hi]
        if correct:
            num[lo:hi], den[lo:hi] = shift_terms(
                terms_model or model, d, state["psi"], s, state["probe"], det, mask)
        if recover_psi:
            state = cm.cgrad(state, data, [b], detector_shape=det, model=model,
                             mask=mask, cg_iter=cg_iter,
                             step_length=step_length,
                             recover_probe=recover_probe)
            batch_cost.append(state["costs"].pop()[0])
            continue
        psi, probe = state["psi"], state["probe"]
        c = cm.cost(model, d, psi, s, probe, det, mask)
        if recover_probe:
            probe, c = osol.conjugate_gradient(
                probe, lambda q: cm.cost(model, d, psi, s, q, det, mask),
                lambda q: cm.grad_probe(model, d, psi, s, q, det, mask),
                num_iter=cg_iter, step_length=step_length)
            state["probe"] = probe
        batch_cost.append(c)
    state["costs"].append([float(np.mean(batch_cost))])
    if correct:
        state["scan"] = opos.update_position(
            state["scan"], pos, num, den, alpha=alpha,
            epoch=epoch).astype(np.float32)
    return state


def iterate(state, data, batches, num_iter, *, rng=None, after_epoch=None,
            **kw):
    """The epoch driver: `epoch`, then the affine regularisation of the
    positions (cgrad runs with the probe constraints off and reads no
    preconditioner)."""
    for _ in range(num_iter):
        state = epoch(state, data, batches, epoch=len(state["costs"]), **kw)
        if state.get("position") is not None:
            state["scan"] = opos.affine_position_regularization(
                state["scan"], state["position"],
                rng or np.random.default_rng()).astype(np.float32)
        if after_epoch is not None:
            after_epoch(state)
    return state


# ------------------------------------------------------------ test problems
def problem(det, pw, S, N, seed, *, masked=False, u16=False, pitch=7.0,
            margin=24):
    """N positions on a grid at `pitch` px with `margin` px of object around
    them (corrected positions move), a smooth object (its gradients carry the
    position information), S probe modes in a pw window, noise-free data on a
    det x det detector.  masked: NaN counts at the unmeasured pixels of
    `cgrad_models.detector_mask`; u16: whole counts up to 20000 as uint16
    (which cannot hold NaN: the mask alone says what is measured).  Returns
    (true scan, object, probe, data, mask or None, generator)."""
    from rpie_positions import smooth_object
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(N)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side),
                              indexing="ij"), -1).reshape(-1, 2)[:N]
    true = (margin // 2 + pitch * ij + rng.random((N, 2))).astype(np.float32)
    HW = int(pitch * (side - 1)) + pw + margin + 2
    psi = smooth_object(rng, 1, HW)
    w = osol.gaussian_probe(pw, rin=0.6)
    probe = np.stack([w * np.exp(1j * np.pi * rng.random((pw, pw))) / (m + 1)
                      for m in range(S)])[None, None].astype(np.complex64)
    data = ops.intensity_from_farplane(
        ops.ptycho_fwd(probe, true, psi, det)).astype(np.float32)
    mask = cm.detector_mask(det) if masked else None
    if u16:
        data = np.round(data * (20000.0 / data.max())).astype(np.uint16)
    elif masked:
        data[:, ~mask] = np.nan
    return true, psi, probe, data, mask, rng


def start(psi_true):
    """The first iterate of the epoch comparisons: near the solution, where
    the one-mode poisson problems are well conditioned (see
    test_cgrad_models_gpu._start)."""
    return (0.8 * psi_true + 0.1).astype(np.complex64)


# ------------------------------------------- the C entry, called directly
def entry_run(psi, scan, probe, data, mask, model, *, positions=True,
              with_acc=True, with_num=True):
    """One call of tike_lstsq_chunk_gradients_positions (positions=False:
    of tike_lstsq_chunk_gradients) on the whole problem as one chunk, every
    output as a NumPy array (None where it was not asked for)."""
    import torch
    import tike_amd._arrays as A
    from tike_amd._lib import check, lib
    from tike_amd.operators.propagation import fft_scales
    from tike_amd.ptycho.position import gaussian_derivative_taps
    dev = torch.device("cuda", torch.cuda.current_device())
    N, S, det = len(scan), probe.shape[-3], probe.shape[-1]
    H, W = psi.shape[-2:]
    u16 = data.dtype == np.uint16
    t = dict(psi=A.to_device(psi), scan=A.to_device(scan),
             probe=A.to_device(probe), data=A.data_to_device(data),
             mask=None if mask is None else A.to_device(mask.astype(np.uint8)))
    c64 = lambda *s: torch.empty(*s, dtype=torch.complex64, device=dev)
    f32 = lambda *s: torch.full(s, float("nan"), dtype=torch.float32,
                                device=dev)
    scratch, work = c64(N, 1, S, det, det), c64(N, 1, S, det, det)
    gscale = f32(2 * N, det, det)
    patches, objproj = c64(N, det, det), c64(N, det, det)
    costs = f32(N)
    mpu = torch.zeros(1, 1, S, det, det, dtype=torch.complex64, device=dev)
    acc = torch.zeros(2, H, W, device=dev) if with_acc else None
    # (NaN: the entry overwrites the sums, it does not accumulate)
    num, den = (f32(N, 2), f32(N, 2)) if with_num else (None, None)
    inten = f32(det, det)
    taps, r = gaussian_derivative_taps(0.333)
    fwd_scale, inv_scale = fft_scales(det, "ortho")
    nmeasured = det * det if mask is None else int(mask.sum())
    args = (A.ptr(t["psi"]), A.ptr(t["scan"]), A.ptr(t["probe"]), None, None,
            0, 0, A.ptr(t["data"]), int(u16), A.ptr(t["mask"]),
            {"gaussian": 0, "poisson": 1}[model], 1.0, nmeasured,
            A.ptr(scratch), A.ptr(work), A.ptr(gscale), A.ptr(patches),
            A.ptr(costs), A.ptr(objproj) if positions or with_acc else None,
            None, A.ptr(mpu), 1.0, A.ptr(acc), N, S, det, H, W, fwd_scale,
            inv_scale)
    if positions:
        check(lib.tike_lstsq_chunk_gradients_positions(
            *args, taps.ctypes.data, r, A.ptr(inten), A.ptr(num), A.ptr(den),
            A.stream_ptr()), "chunk gradients + position sums")
    else:
        check(lib.tike_lstsq_chunk_gradients(*args, A.stream_ptr()),
              "chunk gradients")
    host = lambda x: None if x is None else x.cpu().numpy()
    return dict(costs=host(costs), mpu=host(mpu), acc=host(acc),
                num=host(num), den=host(den))
