"""The difference map (Thibault et al., Science 321 (2008) 379;
Ultramicroscopy 109 (2009) 338).  The reference snapshot has no such solver;
this docstring and the float64 model of the tests (tests/dm_model.py) define
it.

Unlike `lstsq_grad`, `rpie` and `cgrad` it keeps STATE from one epoch to the
next besides the object and the probe: one exit wave per position and mode,
``waves (N, S, pw, pw)`` complex64, in the rank's local position order.  With
``O_n`` the bilinear patch of the object at position n, ``P_s`` the shared
probe and ``a = DmOptions.relaxation``, one epoch is

1. the exit-wave step, for every position, with the object and the probe of
   the epoch's start::

       r     = (1 + a) P_s O_n - a waves              tike_dm_reflect
       R     = scale FFT2(pad(r))
       I_n   = sum_s |R|^2
       G     = R (sqrt(d_n) / (sqrt(I_n) + 1e-9) - 1)   measured pixels
             = (unmeasured_pixels_scaling - 1) R        elsewhere
                                                      tike_farplane_gradient
       chi   = IFFT2(G) inv_scale
       waves <- (1 - a) waves + a P_s O_n + crop(chi)   tike_dm_update

   that is ``waves + P_F(r) - P O`` with ``P_F`` the modulus projection;

2. ``overlap_iter`` alternations of::

       O   <- (c_O O + sum_n scatter(sum_s conj(P_s) waves))
              / (c_O + sum_n scatter(sum_s |P_s|^2))
       P_s <- (c_P P_s + sum_n conj(O_n) waves) / (c_P + sum_n |O_n|^2)

   with ``c = inertia * max(denominator)``; the object line only with
   ``object_options``, the probe line (which sees the new object) only with
   ``probe_options`` and from ``update_start`` on.  The sums come from
   `tike_lstsq_gradients` on the waves, `tike_scatter_patches`,
   `tike_psi_preconditioner` and `tike_probe_preconditioner`, and are
   all-reduced over the ranks.

The minibatches only partition the work: the result does not depend on
``num_batch`` beyond the order of the sums.

Where the waves live.  They are solver state, kept in a cache on the operator
(as `GradientPlan` and the workspaces of `lstsq._workspace` are), keyed on
``(N, S, pw)``, and start as ``waves = P O`` at the first epoch and whenever
that key changes.  They are NOT part of `PtychoParameters`: a new
`Reconstruction` -- also one that resumes from a result -- starts again from
``waves = P O``.  They take ``N S pw^2 8`` bytes of device memory.

The cost.  ``algorithm_options.costs`` receives the mean over the positions of
all ranks of ``mean_{measured pixels} (sqrt(I_n) - sqrt(d_n))^2``: the Fourier
error of the REFLECTED estimate r, as PtyPy reports it for its difference map.
It is not the model cost of ``O P``, which `lstsq_grad`, `rpie` and `cgrad`
report -- for that see `tike_amd.operators.Ptycho.cost`.  The two agree where
the waves equal ``P O`` (the first epoch).

Routes of the middle of the exit-wave step (`FUSED`, `TIKE_DM_FUSED`):
far-plane-free at 256^2 / 512^2 with probe window = detector, at most 8 modes
(4 at 512^2) and resident data -- `tike_fft2_pass1` ->
`tike_fwd_grad_ifft2_pass1` -> `tike_fft2_pass2_inplace`, the far plane never
stored, as on rpie's route; everything else stores it: `tike_fft2` ->
`tike_farplane_gradient` -> `tike_fft2`, any shape `tike_fft2` takes.
"""
import logging
import math

import torch

from ... import _tuning
from ... import _arrays as A
from ..._lib import check, lib
from ...operators.propagation import fft_scales
from . import lstsq as L

logger = logging.getLogger(__name__)

FUSED = _tuning.dm_fused
"""256^2 / 512^2, probe window = detector, resident data: the far-plane-free
route of the exit-wave step.  False: the stored route, which remains the path
of every other shape; tests set it to compare the two."""

MAX_MODES = 16  # of `tike_lstsq_gradients`, which forms the overlap sums


def refuse(parameters, fly=1):
    """What the difference map cannot be combined with, by name, and the
    option values it cannot run with.  Reads shapes and options only: it is
    called before any device work (`Reconstruction`, and `dm` itself)."""
    o = parameters.algorithm_options
    D = parameters.psi.shape[0]
    S = parameters.probe.shape[-3]
    refusals = (
        (fly > 1, f"fly={fly} with dm: fly-scan data (several scan positions "
         "per diffraction pattern) is reconstructed by cgrad only"),
        (parameters.exitwave_options is not None
         and parameters.exitwave_options.noise_model == "poisson",
         "dm with the Poisson noise model: the modulus projection of the "
         "difference map is the amplitude (gaussian) model's; a Poisson "
         "projection is not implemented"),
        (parameters.eigen_probe is not None
         or parameters.eigen_weights is not None,
         "dm does not support eigen probes: the probe update of the "
         "difference map is written for one shared probe"),
        (D > 1, f"dm with several slices (psi.shape[0] = {D}): a multislice "
         "difference map is not implemented"),
        (parameters.position_options is not None,
         "dm with position_options: position correction is not implemented "
         "for dm"),
        (getattr(parameters.object_options, "use_adaptive_moment", False),
         "dm with object_options.use_adaptive_moment: the object update of "
         "the difference map is a projection, not a gradient step"),
        (getattr(parameters.probe_options, "use_adaptive_moment", False),
         "dm with probe_options.use_adaptive_moment: the probe update of "
         "the difference map is a projection, not a gradient step"),
        (S > MAX_MODES, f"dm with {S} probe modes: the overlap sums are "
         f"formed for at most {MAX_MODES}"),
    )
    for applies, message in refusals:
        if applies:
            raise NotImplementedError(message)
    values = (
        (o.relaxation > 0 and math.isfinite(o.relaxation),
         f"DmOptions.relaxation = {o.relaxation!r}: expected a finite number "
         "> 0"),
        (int(o.overlap_iter) == o.overlap_iter and o.overlap_iter >= 1,
         f"DmOptions.overlap_iter = {o.overlap_iter!r}: expected an integer "
         ">= 1"),
        (o.object_inertia >= 0,
         f"DmOptions.object_inertia = {o.object_inertia!r}: expected a number "
         ">= 0"),
        (o.probe_inertia >= 0,
         f"DmOptions.probe_inertia = {o.probe_inertia!r}: expected a number "
         ">= 0"),
    )
    for holds, complaint in values:
        if not holds:
            raise ValueError(complaint)


def fused_route(op, S, pw, data):
    """True where the exit-wave step runs without a stored far plane."""
    det = op.detector_shape
    return bool(FUSED and det in (256, 512) and L.fused_gradients(S, pw, det)
                and isinstance(data, torch.Tensor))


def _waves(op, N, S, pw, device):
    """(the cached waves of this operator, True when they are new and so
    stand for P O)."""
    key = (N, S, pw)
    cached = getattr(op, "_tike_amd_dm_waves", None)
    if (cached is not None and cached[0] == key
            and cached[1].device == device):
        return cached[1], False
    waves = torch.empty((N, S, pw, pw), dtype=torch.complex64, device=device)
    op._tike_amd_dm_waves = (key, waves)
    return waves, True


def exit_wave_step(op, data, psi, scan, probe, waves, fresh, lo, hi, costs,
                   *, relaxation, exitwave_options):
    """Step 1 of the module docstring for the positions [lo, hi), chunk by
    chunk: `waves[lo:hi]` updated in place, `costs[lo:hi]` written.  fresh:
    the waves are not initialised yet and stand for P O."""
    dev = psi.device
    S, pw = probe.shape[-3], probe.shape[-1]
    det = op.detector_shape
    H, W = psi.shape[-2:]
    st = A.stream_ptr()
    fwd_scale, inv_scale = fft_scales(det, op.norm)
    nmeasured, mask_u8 = L.mask_info(exitwave_options, det)
    unmeasured = float(exitwave_options.unmeasured_pixels_scaling)
    fused = fused_route(op, S, pw, data)
    chunk = L.chunk_positions(S, det)
    nmax = max(1, min(chunk, hi - lo))
    ws = L._workspace(op)
    near = ws.get("dm_near", (nmax, S, det, det), torch.complex64, dev)
    mid = (ws.get("dm_mid", (nmax, S, det, det), torch.complex64, dev)
           if fused else None)
    for clo in range(lo, hi, chunk):
        chi_hi = min(hi, clo + chunk)
        n = chi_hi - clo
        sc = scan[clo:chi_hi]
        wv = waves[clo:chi_hi]
        if fresh:
            # the waves of the chunk written as P O (probe window = plane);
            # the reflection below then needs no wave: r = P O
            check(
                lib.tike_dm_reflect(A.ptr(psi[0]), A.ptr(sc), A.ptr(probe),
                                    None, A.ptr(wv), relaxation, n, S, pw,
                                    pw, H, W, st), "dm: waves = P O")
        check(
            lib.tike_dm_reflect(A.ptr(psi[0]), A.ptr(sc), A.ptr(probe),
                                None if fresh else A.ptr(wv), A.ptr(near),
                                relaxation, n, S, pw, det, H, W, st),
            "dm: reflection")
        if fused:
            check(lib.tike_fft2_pass1(A.ptr(near), A.ptr(mid), n * S, det, 0,
                                      st), "dm: forward pass 1")
            check(
                lib.tike_fwd_grad_ifft2_pass1(
                    A.ptr(mid), A.ptr(data[clo:chi_hi]),
                    int(data.dtype == torch.uint16), A.ptr(mask_u8),
                    A.ptr(costs[clo:chi_hi]), A.ptr(near), n, S, det,
                    fwd_scale, 0, unmeasured, nmeasured, st),
                "dm: far field + projection + inverse pass 1")
            check(
                lib.tike_fft2_pass2_inplace(A.ptr(near), n * S, det, 1,
                                            inv_scale, st),
                "dm: inverse pass 2")
        else:
            check(lib.tike_fft2(A.ptr(near), A.ptr(near), n * S, det, 0,
                                fwd_scale, st), "dm: forward transform")
            check(
                lib.tike_farplane_gradient(
                    A.ptr(near), A.ptr(A.data_f32(data, clo, chi_hi)),
                    A.ptr(mask_u8), None, A.ptr(costs[clo:chi_hi]), n, S,
                    det, 0, 1, unmeasured, nmeasured, st),
                "dm: modulus projection")
            check(lib.tike_fft2(A.ptr(near), A.ptr(near), n * S, det, 1,
                                inv_scale, st), "dm: inverse transform")
        check(
            lib.tike_dm_update(A.ptr(wv), A.ptr(near), A.ptr(psi[0]),
                               A.ptr(sc), A.ptr(probe), relaxation, None, n,
                               S, pw, det, H, W, st), "dm: wave update")


def _object_update(op, psi, scan, probe, waves, comm, inertia):
    """The object line of step 2."""
    dev = psi.device
    N, S, pw = waves.shape[:3]
    H, W = psi.shape[-2:]
    st = A.stream_ptr()
    chunk = L.chunk_positions(S, pw)
    ws = L._workspace(op)
    objproj = ws.get("dm_objproj", (max(1, min(chunk, N)), pw, pw),
                     torch.complex64, dev)
    acc = torch.zeros((2, H, W), dtype=torch.float32, device=dev)
    den = torch.zeros((H, W), dtype=torch.float32, device=dev)
    for lo in range(0, N, chunk):
        n = min(chunk, N - lo)
        sc = scan[lo:lo + n]
        check(
            lib.tike_lstsq_gradients(A.ptr(waves[lo:lo + n]), A.ptr(sc),
                                     A.ptr(psi[0]), A.ptr(probe), None, None,
                                     0, 0, None, None, None, A.ptr(objproj),
                                     n, S, pw, H, W, st),
            "dm: sum_s conj(P_s) waves")
        check(
            lib.tike_scatter_patches(A.ptr(objproj), A.ptr(sc), A.ptr(acc), n,
                                     pw, H, W, st), "dm: object numerator")
    amp = torch.sum(torch.square(probe.abs()), dim=-3)[0, 0].contiguous()
    if N:
        check(
            lib.tike_psi_preconditioner(A.ptr(amp), A.ptr(scan), A.ptr(den),
                                        N, pw, H, W, st),
            "dm: object denominator")
    if comm.collective:
        comm.Allreduce(acc, den)
    c = inertia * den.max()
    return ((c * psi + torch.complex(acc[0], acc[1])) / (c + den)).contiguous()


def _probe_update(op, psi, scan, probe, waves, comm, inertia):
    """The probe line of step 2."""
    dev = psi.device
    N, S, pw = waves.shape[:3]
    H, W = psi.shape[-2:]
    st = A.stream_ptr()
    chunk = L.chunk_positions(S, pw)
    num = torch.zeros((S, pw, pw), dtype=torch.complex64, device=dev)
    den = torch.zeros((pw, pw), dtype=torch.complex64, device=dev)
    for lo in range(0, N, chunk):
        n = min(chunk, N - lo)
        check(
            lib.tike_lstsq_gradients(A.ptr(waves[lo:lo + n]),
                                     A.ptr(scan[lo:lo + n]), A.ptr(psi[0]),
                                     A.ptr(probe), None, None, 0, 0, None,
                                     None, A.ptr(num), None, n, S, pw, H, W,
                                     st), "dm: probe numerator")
    if N:
        check(
            lib.tike_probe_preconditioner(A.ptr(scan), A.ptr(psi[0]),
                                          A.ptr(den), N, pw, H, W, st),
            "dm: probe denominator")
    if comm.collective:
        comm.Allreduce(num, den)
    den = den.real
    c = inertia * den.max()
    return ((c * probe + num) / (c + den)).contiguous()


def dm(parameters, data, batches, comm, *, op, epoch):
    """Advance psi / probe, and the waves kept on `op`, by one epoch of the
    difference map (module docstring).  The epoch's entry of
    `algorithm_options.costs` is the Fourier error of the reflected estimate,
    not the model cost of O P (see `tike_amd.operators.Ptycho.cost`).  The
    waves are not part of `parameters`: a new `Reconstruction` starts again
    from waves = P O."""
    refuse(parameters, int(getattr(op, "fly", 1)))
    o = parameters.algorithm_options
    psi, probe, scan = parameters.psi, parameters.probe, parameters.scan
    exitwave_options = parameters.exitwave_options
    probe = probe.contiguous()
    recover_psi = parameters.object_options is not None
    recover_probe = (parameters.probe_options is not None
                     and epoch >= parameters.probe_options.update_start)
    dev = psi.device
    N = scan.shape[0]
    S, pw = probe.shape[-3], probe.shape[-1]
    relaxation = float(o.relaxation)
    waves, fresh = _waves(op, N, S, pw, dev)
    costs = torch.zeros(max(N, 1), dtype=torch.float32, device=dev)
    if hasattr(data, "hint"):  # patterns streamed from pinned host memory
        data.hint([(int(b[0]), int(b[0]) + len(b)) for b in batches
                   if len(b)])
    count = 0.0
    for n, batch in enumerate(batches):
        lo = int(batch[0]) if len(batch) else 0
        hi = lo + len(batch)
        comm.minibatch = int(n)
        count += L.global_count(comm, op, lo, hi)
        exit_wave_step(op, data, psi, scan, probe, waves, fresh, lo, hi,
                       costs, relaxation=relaxation,
                       exitwave_options=exitwave_options)
    total = comm.Allreduce_scalars([costs[:N].sum(dtype=torch.float64)], dev)
    for _ in range(int(o.overlap_iter)):
        if recover_psi:
            psi = _object_update(op, psi, scan, probe, waves, comm,
                                 float(o.object_inertia))
        if recover_probe:
            probe = _probe_update(op, psi, scan, probe, waves, comm,
                                  float(o.probe_inertia))
    # one device->host scalar per epoch, as the other solvers read theirs
    o.costs.append([float(total[0].item()) / count])
    parameters.psi, parameters.probe = psi, probe
    return parameters
