"""Conjugate-gradient ptychography solver.

The reference snapshot ships no ptychography ``cgrad``; it is
composed here, as BASELINE's configs ask, from the reference's own pieces:
``tike.opt.conjugate_gradient`` (opt.py:312-380: Dai-Yuan direction,
backtracking line search), the cost ``Ptycho.cost(..., model=...)``
(ptycho.py:193-204) and its gradient ``Ptycho.adj(<model>_grad(...))``
(objective.py:31-44, :90-104) on the measured pixels (``lstsq.py:448-452``
selects them), following the multi-GPU pattern of lamino/solvers/cgrad.py:58-92:
the cost and the gradient are summed over ranks, every rank then takes the same
step.

Position correction (``position_options``) is composed the same way, from what
the other two solvers do: per minibatch, before its first CG step and at the
old positions, the least-squares shift estimate of every position summed over
all probe modes (``lstsq.all_mode_position_sums``, rpie's estimator; with one
mode lstsq.py:545-579) with chi = cgrad's own near-plane descent direction,
-adj(gaussian_grad) or -1/2 adj(poisson_grad), 0 at unmeasured pixels; after
the last minibatch one ``lstsq._update_position`` with ``alpha`` of the
algorithm options, the allowed-positions test of rpie, and only then the new
``parameters.scan``.  The sums need the object projection alone, which the
gradient pass of the object writes anyway (``_PositionTerms``).

One epoch loop (``cgrad()``) serves three routes, each behind
``_Minibatch``.  Per minibatch and per recovered variable (the object, then
the probe, then -- where the detector has one -- the root of its fitted
table) it runs one conjugate-gradient call -- on the device where the
minibatch offers that and the search succeeds (``_cg_on_device``), else
``_host_cg``, the ONE ``opt.conjugate_gradient`` of this module -- and, when
no variable is recovered, one cost-only evaluation.

* plain (``_CostPlan`` + ``_cost_and_grad``): one pattern per position, a
  single slice, a far-field detector as fine as the data.  The only route
  with device line searches, graph capture and position sums.
* whole frames (``data`` holds one frame per ``fly`` consecutive positions,
  reference ptycho.py:95-125; also ``fly`` = 1 whenever the operator's
  ``detector`` -- ``operators.detector``, no reference counterpart -- is not
  the plain far field): the mean over FRAMES of each frame's mean cost over
  its measured pixels, the intensity of a frame being the sum over its
  positions and modes.  Every line search is decided on the host.  What the
  detector does is the one thing that differs, chunk by chunk:

  - far field, binned (a far plane B times finer than the patterns; the mask
    and the pixel count are at data resolution), with a background b = a * a
    per pixel, or blurred by K = a^2 / sum a^2: ``_fly_cost_and_grad`` --
    forward, ``detector.farplane_step``, adjoint.  A background or a blur
    that is fitted adds a THIRD conjugate-gradient call per minibatch, on a
    (real), after the object's and the probe's: the intensity depends on
    neither, so that call stores the minibatch's intensities once and every
    gradient and line-search trial is one launch of the ``State``'s
    ``cost_and_grad`` (``ptycho/background.py``, ``ptycho/blur.py``) -- no
    forward operator, no transform.
  - near field (every pattern is |IFFT2(H FFT2(patch x probe))|^2, probe
    window = detector, H a fixed propagator): ``_nearfield_cost_and_grad``,
    whose middle on the 128^2 / 256^2 route is one launch,
    ``tike_nearfield_plane_gradient`` -- the detector-plane wave never exists
    in memory.
* objects of several slices (``psi.shape[0] > 1``, probe window = detector):
  the same cost on the far field behind the last slice, e_d = patch(O_d) x
  beam_d, beam_{d+1} = Fresnel(e_d), and its EXACT gradient -- the adjoint
  taken back through every slice, conj(patch) x wave between two transforms
  (``tike_slice_step_back``), WITHOUT the division by the number of slices
  that ``Multislice.adj`` keeps from the reference
  (``_multislice_cost_and_grad``; the route, the chunk, the workspace
  buffers, the forward of a chunk and the fused walk back are the functions
  of ``_multislice.py``, which ``tike_amd.autograd`` calls as well, with what
  differs between the two as arguments).  One conjugate gradient moves all
  slices at once, then one the probe; the cost is not linear in the far plane
  along an object direction any more: every line search is decided on the
  host.
"""
import logging
from typing import NamedTuple, Optional

import numpy as np
import torch

from ... import _tuning
from ... import _arrays as A
from ... import opt
from ..._lib import check, lib
from ...operators import detector as D
from ...operators import nearfield as NF
from ...operators.propagation import fft_scales
from ..exitwave import ExitWaveOptions
from ..position import gaussian_derivative_taps
from . import _multislice as M
from . import lstsq as L
from ._plan import MODELS
from .lstsq import (SPLIT_FORWARD_SIZES, _get_nearplane_gradients,
                    _update_position, _workspace, chunk_positions,
                    fused_gradients, global_count, mask_info, minibatch_key)
from .rpie import _positions_flag, _raise_unless_allowed


logger = logging.getLogger(__name__)

_ALL_MEASURED = {}


class _CostModel(NamedTuple):
    """What cgrad minimises (`_cost_model`; unpacks as the 4-tuple it was)."""
    options: ExitWaveOptions  # what the gradient passes read
    model: int  # MODELS
    nmeasured: int  # measured pixels per pattern
    mask: Optional[torch.Tensor]  # uint8 (det, det); None: every pixel


def _cost_model(exitwave_options, det):
    """The `_CostModel` of the caller's exit-wave options.  A mask whose
    pixels are all measured means every pixel, whatever its shape (the
    probe-shaped default); one with unmeasured pixels must be (det, det) --
    mask_info raises otherwise.  The exit-wave relaxations of lstsq / rpie
    (unmeasured_pixels_scaling, step_length_*) are no part of a cost and are
    not read."""
    eo = exitwave_options
    if eo.noise_model not in MODELS:
        raise ValueError(f"unknown noise model {eo.noise_model!r}")
    model = MODELS[eo.noise_model]
    if mask_info(eo)[1] is None:
        key = (det, eo.noise_model)
        if key not in _ALL_MEASURED:
            _ALL_MEASURED[key] = ExitWaveOptions(
                measured_pixels=np.ones((det, det), dtype=bool),
                noise_model=eo.noise_model)
        return _CostModel(_ALL_MEASURED[key], model, det * det, None)
    nmeasured, mask_u8 = mask_info(eo, det)
    return _CostModel(eo, model, nmeasured, mask_u8)


POISSON_POSITION_STEP = 0.5
"""chi of the shift estimate under the Poisson model is this times cgrad's
descent direction: 1 - d/I = (1 - sqrt(d/I)) (1 + sqrt(d/I)) ~ 2 (1 - sqrt(d/I))
near the solution, so half the Poisson direction is the gaussian exit-wave
difference there (it is also the reference's first Poisson step,
exitwave.py `step_length_start`; the option itself is not read, as
CgradOptions documents).  The numerator is linear in chi: applied to it once
per epoch."""


def _gradient_buffer(psi, probe, want_psi, want_probe, planar=None):
    """The ONE zeroed float32 buffer in which an evaluation sums MINUS its
    gradients -- the object's first, then the probe's, so that one
    `comm.Allreduce` sums both over the ranks -- and its views: (buffer,
    object view or None, probe view or None).  Views are complex64, shaped
    like psi and probe; planar: the shape, (..., 2, H, W), of a float32 object
    view instead (the accumulators of the grouped scatter)."""
    n_obj = 2 * psi.numel() if want_psi else 0
    n_prb = 2 * probe.numel() if want_probe else 0
    grads = torch.zeros(n_obj + n_prb, dtype=torch.float32, device=psi.device)
    obj = prb = None
    if want_psi:
        obj = (grads[:n_obj].view(planar) if planar else
               torch.view_as_complex(grads[:n_obj].view(*psi.shape, 2)))
    if want_probe:
        prb = torch.view_as_complex(grads[n_obj:].view(*probe.shape, 2))
    return grads, obj, prb


class _PositionTerms:
    """(numerator, denominator) of the shift estimates of this rank's
    positions, (N, 2) each, and which minibatch still owes its rows: the sums
    are taken by the FIRST gradient evaluation of a minibatch -- at the
    incoming iterate -- and by no later one (`take`)."""

    def __init__(self, scan):
        self.numerator = torch.zeros_like(scan)
        self.denominator = torch.zeros_like(scan)
        self.pending = False

    def take(self):
        """The two arrays if this minibatch's sums are still to be taken
        (they count as taken from here on), else None."""
        if not self.pending:
            return None
        self.pending = False
        return self.numerator, self.denominator


class _CostPlan:
    """Everything a line-search probe (cost only) of one minibatch needs that
    does not change between probes: workspaces, chunk bounds, raw pointers of
    the scan / data / cost slices.  A probe is then two C-ABI calls per chunk
    and one reduction -- at BASELINE configs[0] (256 positions of 128^2) the
    Python between the launches was most of the epoch."""

    def __init__(self, op, data, psi, scan, probe, lo, hi, cm):
        det, dev = op.detector_shape, psi.device
        S, pw, (H, W) = probe.shape[-3], probe.shape[-1], psi.shape[-2:]
        self.model, self.nmeasured = cm.model, cm.nmeasured
        N = hi - lo
        ws = _workspace(op)
        self.split = det in SPLIT_FORWARD_SIZES
        chunk = chunk_positions(S, det, self.split)
        self.far = ws.get("far", (min(chunk, max(N, 1)), 1, S, det, det),
                          torch.complex64, dev)
        # detector sizes p x 2^k (round 6): the prime-factor launches of the
        # gradient pipeline with nothing but the costs stored -- sub-tile
        # transforms + the p x p combine, no far plane in natural order
        self.pfa = (not self.split and L.PFA_ROUTE and L.GENERAL_FUSED
                    and L.pfa_gradients(S, pw, det))
        self.pfa_lds = bool(self.pfa and L.PFA_SUBTILES_IN_LDS
                            and lib.tike_pfa_fwd_subtiles_supported(S, pw, det))
        if self.pfa_lds:
            self.aux = ws.get("pfa_probe", (S, det, det), torch.complex64, dev)
        elif self.pfa:
            self.aux = ws.get("mid", tuple(self.far.shape), torch.complex64,
                              dev)
        self.costs = ws.get("costs", (max(N, 1),), torch.float32, dev)[:N]
        self.fwd_scale = fft_scales(det, op.norm)[0]
        self.dims = (S, pw, det, H, W)
        self.u16 = int(data.dtype == torch.uint16)
        # resident data that the cost kernel of this size reads as it is
        direct = isinstance(data, torch.Tensor) and (
            self.split or data.dtype == torch.float32)
        self.pmask = A.ptr(cm.mask)
        self.lo = lo
        self.chunks = []
        for clo in range(lo, hi, chunk):
            chi = min(hi, clo + chunk)
            self.chunks.append(
                (clo, chi, scan[clo:chi], data[clo:chi] if direct else None,
                 self.costs[clo - lo:chi - lo]))

    def run(self, data, psi, probe):
        S, pw, det, H, W = self.dims
        st = A.stream_ptr()
        ppsi, pprobe, pfar = A.ptr(psi), A.ptr(probe), A.ptr(self.far)
        mask, model, nmeasured = self.pmask, self.model, self.nmeasured
        for clo, chi, sc, d, cost in self.chunks:
            n = chi - clo
            if d is None:  # streamed from the host, or 16-bit counts at 128^2
                d = data[clo:chi] if self.split else A.data_f32(data, clo, chi)
            if self.split:
                check(
                    lib.tike_fwd_pass1(ppsi, sc.data_ptr(), pprobe, 0, None,
                                       None, None, 0, 0, pfar, None, n, S, pw,
                                       det, H, W, st), "cgrad forward pass 1")
                check(
                    lib.tike_fwd_gradient_scale(
                        pfar, d.data_ptr(), self.u16, mask, None, None,
                        cost.data_ptr(), None, n, S, det, self.fwd_scale,
                        model, 1.0, nmeasured, st),
                    "cgrad forward pass 2 + cost")
            elif self.pfa:
                if self.pfa_lds:
                    check(
                        lib.tike_pfa_fwd_subtiles(
                            ppsi, sc.data_ptr(), pprobe, None, None, 0, 0,
                            A.ptr(self.aux), pfar, None, n, S, pw, det, H, W,
                            st), "cgrad forward (sub-tiles in LDS)")
                else:
                    check(
                        lib.tike_pfa_fwd_gather(
                            ppsi, sc.data_ptr(), pprobe, 0, None, None, None,
                            0, 0, A.ptr(self.aux), None, n, S, pw, det, H, W,
                            st), "cgrad forward (prime-factor gather)")
                    check(lib.tike_pfa_fft2(A.ptr(self.aux), pfar, n * S, det,
                                            0, st), "cgrad sub-tile transforms")
                check(
                    lib.tike_pfa_combine_gradient(
                        pfar, d.data_ptr(), mask, cost.data_ptr(), n, S, det,
                        self.fwd_scale, model, 1.0, nmeasured, 0, st),
                    "cgrad cost (p x p combine)")
            else:
                check(
                    lib.tike_ptycho_fwd(ppsi, sc.data_ptr(), pprobe, 0, None,
                                        None, 0, 0, pfar, n, S, pw, det, H, W,
                                        self.fwd_scale, 0, st), "cgrad forward")
                check(
                    lib.tike_farplane_gradient(pfar, d.data_ptr(), mask, None,
                                               cost.data_ptr(), n, S, det,
                                               model, 0, 1.0, nmeasured, st),
                    "cgrad cost")
        return self.costs

    def supports_gradients(self):
        """The far-plane-free sizes and 128^2 (float32 data), probe window =
        detector: the gradient of a chunk is ONE C-ABI call
        (tike_lstsq_chunk_gradients)."""
        S, pw, det, _, _ = self.dims
        return ((self.split or (det == 128 and not self.u16)) and pw == det
                and fused_gradients(S, pw, det)
                and all(c[3] is not None for c in self.chunks))

    def gradients(self, op, comm, psi, probe, want_psi, want_probe,
                  position_terms=None):
        """(costs, -d cost / d psi or None, -d cost / d probe or None), the
        sums over the positions of all ranks -- what _get_nearplane_gradients
        returns for this case, without its per-call set-up.  position_terms:
        (numerator, denominator) of all local positions; the rows of this
        minibatch are filled chunk by chunk from the projection of the chunk
        (tike_lstsq_chunk_gradients_positions), which is then formed whether
        or not the object gradient is wanted."""
        S, pw, det, H, W = self.dims
        dev = psi.device
        ws = _workspace(op)
        n_max = self.far.shape[0]
        mid = ws.get("mid", tuple(self.far.shape), torch.complex64, dev)
        # (128^2 keeps the far plane: factor table + intensity table)
        gscale = ws.get("gscale", ((2 if det == 128 else 1) * n_max, det, det),
                        torch.float32, dev)
        N = self.costs.shape[0]
        patches = ws.get("patches", (max(N, 1), pw, pw), torch.complex64, dev)
        objproj = ws.get("objproj", (n_max, pw, pw), torch.complex64, dev)
        grads, acc, mpu = _gradient_buffer(psi, probe, want_psi, want_probe,
                                           planar=(2, H, W))
        _, inv_scale = fft_scales(det, op.norm)
        st = A.stream_ptr()
        lo = self.lo
        if position_terms:
            taps, taps_r = gaussian_derivative_taps(sigma=0.333)
            inten = ws.get("probe_intensity", (pw, pw), torch.float32, dev)
        for clo, chi, sc, d, cost in self.chunks:
            n = chi - clo
            args = (A.ptr(psi), sc.data_ptr(), A.ptr(probe), None, None, 0, 0,
                    d.data_ptr(), self.u16, self.pmask, self.model, 1.0,
                    self.nmeasured, A.ptr(self.far), A.ptr(mid), A.ptr(gscale),
                    A.ptr(patches[clo - lo:chi - lo]), cost.data_ptr(),
                    A.ptr(objproj) if want_psi or position_terms else None,
                    None, A.ptr(mpu), 1.0, A.ptr(acc), n, S, det, H, W,
                    self.fwd_scale, inv_scale)
            if position_terms:
                check(
                    lib.tike_lstsq_chunk_gradients_positions(
                        *args, taps.ctypes.data, taps_r, A.ptr(inten),
                        A.ptr(position_terms[0][clo:chi]),
                        A.ptr(position_terms[1][clo:chi]), st),
                    "cgrad gradients + position shift sums")
            else:
                check(lib.tike_lstsq_chunk_gradients(*args, st),
                      "cgrad gradients")
        if comm.collective and grads.numel():
            comm.Allreduce(grads)
        return self.costs, acc, mpu


def _cost_and_grad(op, comm, data, psi, scan, probe, lo, hi, *, want_psi,
                   want_probe, want_grad, cm, read_cost=True, plan=None,
                   position_terms=None):
    """Global cost (mean over all positions of each pattern's mean over its
    measured pixels, the noise model of `cm`, _cost_model) of the minibatch
    [lo, hi) and, optionally, d cost / d psi and d cost / d probe
    (unnormalised adjoints).

    The gradient is the one lstsq_grad forms (the same kernels, whatever the
    detector size); a line-search probe (cost only) at 256^2 / 512^2 is the
    split forward of that pipeline with nothing but the costs stored.
    position_terms (with want_grad): (numerator, denominator) of the shift
    estimates, rows [lo, hi) filled by this gradient pass."""
    if want_grad and plan is not None and plan.supports_gradients():
        costs, acc, mpu = plan.gradients(op, comm, psi, probe, want_psi,
                                         want_probe, position_terms)
    elif want_grad:
        g = _get_nearplane_gradients(
            data, psi, scan, probe, None, None, lo, hi, comm, num_batch=1,
            exitwave_options=cm.options, op=op, recover_psi=want_psi,
            recover_probe=want_probe, need_chi0=False, plain=True,
            all_mode_position_terms=position_terms)
        costs, acc, mpu = g["costs"], g.get("object_acc"), g.get(
            "m_probe_update")
    else:
        plan = plan or _CostPlan(op, data, psi, scan, probe, lo, hi, cm)
        costs = plan.run(data, psi, probe)
    # the accumulators hold MINUS the gradients
    gpsi = (-torch.complex(acc[0], acc[1])[None]
            if want_grad and want_psi else None)
    gprobe = -mpu if want_grad and want_probe else None
    total = costs.sum(dtype=torch.float64)  # device scalar (this rank)
    if read_cost:
        return _finish_cost(total, comm, op, lo, hi), gpsi, gprobe
    return total, gpsi, gprobe


def _finish_cost(total, comm, op, lo, hi, fly=1):
    """Mean cost over the positions -- fly scans: the FRAMES -- of ALL ranks,
    on the host: one (all-)reduction and one read-back."""
    if comm.collective:
        total = comm.Allreduce_scalars([total], total.device)[0]
    return float(total.item()) / (global_count(comm, op, lo, hi) / fly)


DEVICE_LINE_SEARCH = True
"""Tests set this to False to run opt.conjugate_gradient with the host-side
line search (one read-back per trial) everywhere."""

PLAIN_ROUTE = True
"""Tests set this to False to send plain minibatches the whole-frames way."""

LINE_SEARCH_SLOTS = (8, 4)
"""Step lengths enqueued ahead per line search to begin with: first CG
iteration of a call (it starts from `step_length`), later iterations (they
start from the length accepted last).  A reconstruction then learns what its
searches need (`_SlotPolicy`)."""

MAX_SLOTS = 30  # tike_cgrad_line_search's limit: step_length / 2^29

LINEAR_LINE_SEARCH = True
"""The far plane is linear in the variable a search moves along, so ONE forward
pass of the direction and one pass over two hand-offs give the costs of 16
step lengths at once (tike_cgrad_line_search_linear): same candidates, same
acceptance rule, results equal to the trial-by-trial search up to float32
rounding, for about half the work (c2: 1.1 ms of trials per search -> 0.6 ms).
False: the trial-by-trial device search (tike_cgrad_line_search)."""

LINEAR_STEPS = 16  # TK_LS_STEPS x TK_LS_PASSES of csrc/cgrad_search.hip


class _SlotPolicy:
    """How many trial step lengths to enqueue ahead, per variable (object,
    probe) and kind of search (first of a call, later ones), learnt from the
    trials the previous calls of this reconstruction needed: one more than the
    largest number seen; a count that has been two or more too generous for
    eight calls in a row shrinks by one.  A skipped slot costs about 20 us, a
    search that runs out of slots costs the whole CG call again -- so a
    problem whose steps shrink below step_length / 2^7 pays for that once,
    not in every call of every epoch (round-3 advisor finding).  Counts change
    rarely, which keeps the captured launch sequences (`_CgGraph`) valid."""

    # calls of a variable that skip the all-at-once search after it has found
    # none of its 16 step lengths acceptable (doubled per repeated failure)
    LINEAR_PAUSE = 16

    def __init__(self):
        self.slots = {v: list(LINE_SEARCH_SLOTS) for v in (0, 1)}
        self.generous = {v: [0, 0] for v in (0, 1)}
        self.linear_skip = {0: 0, 1: 0}
        self.linear_pause = {0: self.LINEAR_PAUSE, 1: self.LINEAR_PAUSE}

    def linear_allowed(self, variable):
        """The all-at-once search keeps no steps below step / 2^15: a problem
        that needs them would run it, throw it away and repeat the whole CG
        call trial by trial -- in every call (round-4 advisor finding).  After
        a failure the variable goes straight to the trial-by-trial search for
        a while, then the all-at-once search gets another try."""
        if self.linear_skip[variable] > 0:
            self.linear_skip[variable] -= 1
            return False
        return True

    def linear_result(self, variable, ok):
        if ok:
            self.linear_pause[variable] = self.LINEAR_PAUSE
        else:
            self.linear_skip[variable] = self.linear_pause[variable]
            self.linear_pause[variable] = min(1024,
                                              2 * self.linear_pause[variable])

    def get(self, variable):
        return tuple(self.slots[variable])

    def learn(self, variable, trials_per_search):
        """trials_per_search: trials each search of a successful call made."""
        seen = (trials_per_search[0], max(trials_per_search[1:], default=1))
        for kind in (0, 1):
            want = max(min(MAX_SLOTS, int(seen[kind]) + 1),
                       LINE_SEARCH_SLOTS[kind])
            have = self.slots[variable][kind]
            if want > have:
                self.slots[variable][kind] = want
                self.generous[variable][kind] = 0
            elif want <= have - 2:
                self.generous[variable][kind] += 1
                if self.generous[variable][kind] >= 8:
                    self.slots[variable][kind] = have - 1
                    self.generous[variable][kind] = 0
            else:
                self.generous[variable][kind] = 0

    def widen(self, variable):
        """After a search ran out of slots: every slot the entry allows."""
        self.slots[variable] = [MAX_SLOTS, MAX_SLOTS]
        self.generous[variable] = [0, 0]


def _slot_policy(op):
    policy = getattr(op, "_cgrad_slot_policy", None)
    if policy is None:
        policy = op._cgrad_slot_policy = _SlotPolicy()
    return policy


def _cg_enqueue(plan, op, comm, x, other, variable, num_iter, step_init,
                count, data, scan, lo, hi, slots, bufs, linear=False,
                positions=None):
    """Enqueue one conjugate-gradient call -- opt.conjugate_gradient
    (opt.py:312-380: Dai-Yuan directions, backtracking line search) for the
    object (variable 0) or the probe (variable 1) with every line search
    decided on the device (tike_cgrad_line_search): per iteration the gradient
    pass, the direction (tike_cgrad_direction) and up to `slots` cost-only
    trials, no host round trip, nothing but launches (so the whole call can be
    captured as a graph).  step_init: device double[5] {0, step_length, 0, 0,
    0}; bufs: two iterates' worth of scratch.  Returns (the last iterate,
    device double[5 + num_iter]: the search state { fx, step, done, trials,
    failures } followed by the running total of trials after every search).
    positions: the `_PositionTerms` of the epoch; the first gradient pass
    takes the minibatch's sums if they are still owed."""
    dev = x.device
    S, pw, det, H, W = plan.dims
    N = hi - lo
    # carried from search to search on the device (the step accepted last is
    # the first one tried next, opt.py:366-371)
    out = torch.zeros(5 + num_iter, dtype=torch.float64, device=dev)
    state = out[:5]
    state.copy_(step_init)
    skip = torch.zeros(1, dtype=torch.int32, device=dev)
    scan_ptr = scan[lo:hi].data_ptr()
    data_ptr = data[lo:hi].data_ptr()
    st_ptr = A.stream_ptr()
    # gradient and direction of the previous iteration, and the four sums of
    # tike_cgrad_direction: one entry per iteration instead of a dozen torch
    # launches (negation, two reductions, the Dai-Yuan update, the cost at x)
    gradient, d = torch.empty_like(x), torch.empty_like(x)
    sums = torch.empty(4, dtype=torch.float64, device=dev)
    if linear:
        ws = _workspace(op)
        far_b = ws.get("far_b", tuple(plan.far.shape), torch.complex64, dev)
        costs_k = ws.get("costs_k", ((LINEAR_STEPS + 1) * max(N, 1) + 1,),
                         torch.float32, dev)
        # one chunk: the gradient pass leaves the forward hand-off of x (at
        # 128^2 its far plane) in plan.far, which the search reads as it is
        a_valid = int(len(plan.chunks) == 1)
        row_sums = torch.zeros(LINEAR_STEPS + 1, dtype=torch.float64,
                               device=dev)
    for i in range(num_iter):
        a, b = (x, other) if variable == 0 else (other, x)  # psi, probe
        costs, acc, mpu = plan.gradients(
            op, comm, a, b, variable == 0, variable == 1,
            positions.take() if positions is not None and i == 0 else None)
        check(
            lib.tike_cgrad_direction(
                A.ptr(acc) if variable == 0 else None,
                None if variable == 0 else A.ptr(mpu), A.ptr(gradient),
                A.ptr(d), x.numel(), int(i == 0), A.ptr(costs),
                costs.numel(), count, A.ptr(state), A.ptr(sums), st_ptr),
            "cgrad direction")
        xs = bufs[i % 2]
        if linear:
            # one rank: the whole search in one call; several: the cost sums of
            # each pass are all-reduced between the pass and its decision
            for stage in ((1, 2, 3, 4) if comm.collective else (0,)):
                check(
                    lib.tike_cgrad_line_search_linear_masked(
                        variable, A.ptr(x), A.ptr(d), A.ptr(xs), A.ptr(other),
                        scan_ptr, data_ptr, plan.u16, A.ptr(plan.far), a_valid,
                        A.ptr(far_b), A.ptr(costs_k), N, plan.far.shape[0], S,
                        det, H, W, plan.fwd_scale, count, A.ptr(state), stage,
                        A.ptr(row_sums), plan.pmask, plan.model,
                        plan.nmeasured, st_ptr),
                    "cgrad line search (all steps at once)")
                if stage in (1, 3):
                    comm.Allreduce_f64(row_sums)
        else:
            check(
                lib.tike_cgrad_line_search_masked(
                    variable, A.ptr(x), A.ptr(d), A.ptr(xs), A.ptr(other),
                    scan_ptr, data_ptr, plan.u16, A.ptr(plan.far),
                    A.ptr(plan.costs), N, plan.far.shape[0], S, det, H, W,
                    plan.fwd_scale, count, A.ptr(state), A.ptr(skip),
                    slots[0 if i == 0 else 1], plan.pmask, plan.model,
                    plan.nmeasured, st_ptr),
                "cgrad line search")
        out[5 + i].copy_(state[3])
        x = xs
    return x, out


def _cg_result(x, out):
    """Read a call's state back (the ONE host synchronisation of a call):
    (x, mean cost, trials made by every search), or None when a search ran
    out of slots."""
    final = out.cpu().numpy()
    if final[4] != 0:
        return None
    return x, float(final[0]), np.diff(final[5:], prepend=0.0)


def _step_init(step_length, dev):
    return torch.from_numpy(
        np.array([0.0, float(step_length), 0.0, 0.0, 0.0])).to(dev)


def _cg_device(plan, op, comm, psi, probe, variable, num_iter, step_length,
               count, data, scan, lo, hi, slots=LINE_SEARCH_SLOTS,
               linear=False, positions=None):
    """`_cg_enqueue` launched eagerly + its read-back.  Returns (x, mean
    cost, trials made by every search), or None when a search ran out of its
    slots -- the caller then repeats the call with more slots or with the
    host-side search, which has no limit."""
    x = psi if variable == 0 else probe
    other = probe if variable == 0 else psi
    bufs = [torch.empty_like(x), torch.empty_like(x)]
    return _cg_result(*_cg_enqueue(
        plan, op, comm, x, other, variable, num_iter,
        _step_init(step_length, x.device), count, data, scan, lo, hi, slots,
        bufs, linear=linear, positions=positions))


USE_GRAPHS = _tuning.cgrad_graphs
"""A conjugate-gradient call is a fixed sequence of ~10 launches per trial
slot whose only data-dependent control flow lives on the device (the `skip`
word), so it can be captured once and replayed as a HIP graph from its second
occurrence on (`_CgGraph`).  MEASURED SLOWER on ROCm 7.2 / gfx950 and therefore
OFF unless TIKE_CGRAD_GRAPHS=1: BASELINE configs[0] (256 positions, every
launch shorter than its own issue) 73.4 k patterns/s launched one by one,
35.7 k replayed -- a replay of ~270 nodes costs ~6 us per node on the GPU
side, more than eager launches that the host issues ahead; c2 67.8 k vs 66.6 k
(profiles/r04_experiments.md).  Kept as an option and under test."""

MAX_GRAPHS = 64


class _CgGraph:
    """The captured launch sequence of one `_cg_enqueue` call.  Inputs are
    copied into static buffers, the graph is replayed, the result is cloned
    out (the buffers belong to the graph)."""

    def __init__(self, enqueue, x, other, step_length):
        self.x = torch.empty_like(x)
        self.other = torch.empty_like(other)
        self.bufs = [torch.empty_like(x), torch.empty_like(x)]
        self.init = _step_init(step_length, x.device)
        self.graph = torch.cuda.CUDAGraph()
        torch.cuda.synchronize()
        with torch.cuda.graph(self.graph):
            self.result, self.out = enqueue(self.x, self.other, self.init,
                                            self.bufs)

    def __call__(self, x, other):
        self.x.copy_(x)
        self.other.copy_(other)
        self.graph.replay()
        return self.result.clone(), self.out


def _every_rank(comm, op, lo, hi, mine):
    """True when `mine` holds on every rank (asked once per minibatch and
    reconstruction: minibatch sizes and data placement are static)."""
    cache = op.__dict__.setdefault("_tike_amd_every_rank", {})
    key = minibatch_key(comm, lo, hi)
    if key not in cache:
        cache[key] = comm.Allreduce_count(int(bool(mine))) == comm.size
    return cache[key]


def _cg_on_device(plan, op, comm, psi, probe, variable, o, count, data, scan,
                  lo, hi, positions=None):
    """One CG call on the device with the slot counts this reconstruction has
    learnt, replayed from a graph once the same call has been seen before; a
    call whose search runs out of slots is repeated once with every slot the
    entry allows before the host-side search takes over.  Returns (x, cost)
    or None.  positions: see `_cg_enqueue` (never with USE_GRAPHS: a replayed
    graph would write the sums of the epoch it was captured in)."""
    policy = _slot_policy(op)
    x = psi if variable == 0 else probe
    other = probe if variable == 0 else psi
    if LINEAR_LINE_SEARCH and not USE_GRAPHS:
        # (the policy is fed by results every rank sees alike -- the staged
        # search decides on all-reduced sums -- so the ranks stay in step)
        r = None
        if policy.linear_allowed(variable):
            r = _cg_device(plan, op, comm, psi, probe, variable, o.cg_iter,
                           o.step_length, count, data, scan, lo, hi,
                           linear=True, positions=positions)
            policy.linear_result(variable, r is not None)
        if r is not None:
            return r[0], r[1]
        if comm.collective:
            return None  # (the host-side search sums its costs over the ranks)
        # a search found none of its 16 step lengths acceptable (steps below
        # step / 2^15): the trial-by-trial search below reaches 2^-29
        policy.widen(variable)
    graphs = getattr(op, "_cgrad_graphs", None)
    if graphs is None:
        graphs = op._cgrad_graphs = {}
    for attempt in range(2):
        slots = policy.get(variable)

        def enqueue(x_, other_, init, bufs):
            return _cg_enqueue(plan, op, comm, x_, other_, variable,
                               o.cg_iter, init, count, data, scan, lo, hi,
                               slots, bufs)

        key = (variable, lo, hi, slots, tuple(x.shape), tuple(other.shape),
               o.cg_iter, float(o.step_length), float(count),
               plan.far.data_ptr(), plan.costs.data_ptr(), scan.data_ptr(),
               data.data_ptr())
        seen = graphs.get(key) if USE_GRAPHS else "eager"
        if seen is False:  # second occurrence: capture
            try:
                seen = graphs[key] = _CgGraph(enqueue, x, other, o.step_length)
            except Exception as e:  # noqa: BLE001 -- capture is an optimisation
                logger.warning("cgrad: graph capture failed (%s); this call "
                               "stays eager", e)
                seen = graphs[key] = "eager"
        if seen is None or seen == "eager":
            # first occurrence: eager (it also warms every lazily created
            # table and workspace a capture must not allocate)
            if seen is None:
                if len(graphs) >= MAX_GRAPHS:
                    graphs.clear()
                graphs[key] = False
            r = _cg_device(plan, op, comm, psi, probe, variable, o.cg_iter,
                           o.step_length, count, data, scan, lo, hi,
                           slots=slots, positions=positions)
        else:
            r = _cg_result(*seen(x, other))
        if r is not None:
            policy.learn(variable, r[2])
            return r[0], r[1]
        if slots == (MAX_SLOTS, MAX_SLOTS):
            break
        policy.widen(variable)
    return None


def _fly_of(op, data, scan):
    """Positions per frame, from the arrays a rank holds (the caller has
    validated divisibility); a rank without a frame takes the context's."""
    if data.shape[0] == 0:
        return int(getattr(op, "fly", 1))
    return scan.shape[0] // data.shape[0]


_REFUSALS = (
    # (the kind of minibatch, what it cannot be combined with, message), the
    # most specific wording first
    ("binning", "positions", "binning={binning} with position_options: "
     "position correction of binned data is not implemented"),
    ("binning", "eigen", "binning={binning} with eigen probes: a varying "
     "probe per position of binned data is not implemented"),
    ("binning", "slices", "binning={binning} with several slices "
     "(psi.shape[0] = {D}): multislice reconstruction of binned data is not "
     "implemented"),
    ("fly", "positions", "fly={fly} with position_options: position "
     "correction of fly-scan data is not implemented"),
    ("fly", "eigen", "fly={fly} with eigen probes: a varying probe per "
     "position of fly-scan data is not implemented"),
    ("fly", "slices", "fly={fly} with several slices (psi.shape[0] = {D}): "
     "multislice fly-scan reconstruction is not implemented"),
    ("slices", "positions", "cgrad with several slices (psi.shape[0] = {D}) "
     "and position_options: position correction of a multislice object is "
     "not implemented for cgrad"),
    ("slices", "eigen", "cgrad with several slices (psi.shape[0] = {D}) and "
     "eigen probes: a varying probe per position is not implemented for "
     "cgrad"),
    ("any", "eigen", "cgrad does not support eigen probes"),
)


def _refuse(parameters, fly, kinds=("binning", "fly", "slices", "any"),
            binning=1):
    """NotImplementedError for the first row of `_REFUSALS` that applies."""
    D = parameters.psi.shape[0]
    has = dict(any=True, fly=fly > 1, binning=binning > 1, slices=D > 1,
               positions=parameters.position_options is not None,
               eigen=(parameters.eigen_probe is not None
                      or parameters.eigen_weights is not None))
    for kind, other, message in _REFUSALS:
        if kind in kinds and has[kind] and has[other]:
            raise NotImplementedError(
                message.format(fly=fly, binning=binning, D=D))


def _refuse_fly(parameters, fly):
    """What a fly-scan reconstruction cannot be combined with."""
    _refuse(parameters, fly, ("fly",))


def _refuse_binning(parameters, binning):
    """What a reconstruction of binned data cannot be combined with."""
    _refuse(parameters, 1, ("binning",), binning)


def _refuse_multislice(parameters):
    """What a multislice object cannot be combined with (fly scans: above)."""
    _refuse(parameters, 1, ("slices",))


def _fly_adjoint(op, far, probe, scan, psi, want_psi, want_probe):
    """Ptycho.adj of a chunk's far plane (a workspace: overwritten):
    (psi_adj (1, H, W) or None, probe_adj summed over the positions
    (1, 1, S, pw, pw) or None)."""
    N, S = scan.shape[0], probe.shape[-3]
    pw, det = op.probe_shape, op.detector_shape
    H, W = psi.shape[-2:]
    dev = psi.device
    if op.fused_adjoint_shapes(S):
        psi_adj, probe_adj = op.adj_device(far, probe, scan, psi)
        return (psi_adj if want_psi else None,
                probe_adj.sum(dim=0, keepdim=True) if want_probe else None)
    st = A.stream_ptr()
    chi = far if pw == det else torch.empty(
        (N, 1, S, pw, pw), dtype=torch.complex64, device=dev)
    check(
        lib.tike_ifft2_crop(A.ptr(far), A.ptr(far), A.ptr(chi), N * S, det, pw,
                            fft_scales(det, op.norm)[1], st),
        "cgrad fly adjoint (ifft2)")
    psi_adj = probe_adj = None
    if want_psi:
        psi_adj = torch.zeros_like(psi)
        check(
            lib.tike_conv_adj(A.ptr(chi), A.ptr(scan), A.ptr(probe), 0,
                              A.ptr(psi_adj), N, S, pw, pw, H, W, st),
            "cgrad fly adjoint (object)")
    if want_probe:
        each = torch.empty((N, 1, S, pw, pw), dtype=torch.complex64,
                           device=dev)
        check(
            lib.tike_conv_adj_probe(A.ptr(chi), A.ptr(scan), A.ptr(psi),
                                    A.ptr(each), N, S, pw, pw, H, W, st),
            "cgrad fly adjoint (probe)")
        probe_adj = each.sum(dim=0, keepdim=True)
    return psi_adj, probe_adj


def _whole_frames(op, probe, lo, hi, fly):
    """(chunk, nmax) of an evaluation over the positions [lo, hi), whole
    frames: positions per chunk (whole frames), the most a chunk holds."""
    assert lo % fly == 0 and hi % fly == 0, (lo, hi, fly)
    chunk = max(1, chunk_positions(probe.shape[-3], op.detector_shape)
                // fly) * fly
    return chunk, min(chunk, max(hi - lo, 1))


def _frame_costs(op, nframe, dev):
    """The workspace's costs of the frames of an evaluation."""
    return _workspace(op).get("costs", (max(nframe, 1),), torch.float32,
                              dev)[:nframe]


def _fly_cost_and_grad(op, comm, data, psi, scan, probe, lo, hi, fly, *,
                       want_psi, want_probe, want_grad, cm,
                       detector=D.Detector(), stored=None):
    """(sum of this rank's per-frame costs, a device scalar; d cost / d psi or
    None; d cost / d probe or None -- unnormalised adjoints summed over the
    ranks) of the positions [lo, hi), whole frames: the data rows
    [lo / fly, hi / fly).  Per chunk of whole frames: the forward operator,
    the far-plane step of `detector`, a far-field kind
    (`detector.farplane_step`; costs only for a line-search probe: the far
    plane is read once and not written) and, for a gradient, the adjoint of
    the far plane it left.  stored (frames, det, det) float32 (background and
    blur, cost only): receives the frames' intensities without the background
    or the blur."""
    dev = psi.device
    S, det = probe.shape[-3], op.detector_shape
    chunk, nmax = _whole_frames(op, probe, lo, hi, fly)
    far_all = _workspace(op).get("far", (nmax, 1, S, det, det),
                                 torch.complex64, dev)
    costs = _frame_costs(op, (hi - lo) // fly, dev)
    grads, gpsi, gprobe = _gradient_buffer(
        psi, probe, want_grad and want_psi, want_grad and want_probe)
    work = D.workspaces(detector, _workspace(op), dev, max(nmax // fly, 1),
                        det, cm)
    for clo in range(lo, hi, chunk):
        chi = min(hi, clo + chunk)
        sc = scan[clo:chi]
        far = far_all[:chi - clo]
        op.fwd_device(probe, sc, psi, out=far)
        frames = slice((clo - lo) // fly, (chi - lo) // fly)
        D.farplane_step(
            op, detector, far, A.counts(data[clo // fly:chi // fly]), fly, cm,
            costs=costs[frames], want_grad=want_grad,
            intensity=None if stored is None else stored[frames], work=work)
        if want_grad:
            # the far plane now holds MINUS the gradient
            a, b = _fly_adjoint(op, far, probe, sc, psi, want_psi, want_probe)
            if gpsi is not None:
                gpsi -= a
            if gprobe is not None:
                gprobe -= b
    if comm.collective and grads.numel():
        comm.Allreduce(grads)
    return costs.sum(dtype=torch.float64), gpsi, gprobe


def _nearfield_cost_and_grad(op, comm, data, psi, scan, probe, lo, hi, fly, *,
                             want_psi, want_probe, want_grad, cm, H):
    """(sum of the per-frame costs, a device scalar; d cost / d psi or None;
    d cost / d probe or None -- unnormalised adjoints, as `_fly_cost_and_grad`
    returns them) of the positions [lo, hi), whole frames, with the detector in
    the NEAR field: every frame is |IFFT2(H FFT2(patch x probe))|^2 summed over
    its positions and modes, H (det, det) the operator's `nearfield`
    (ptycho/nearfield.py; operators/nearfield.py has the three routes).  Per
    chunk of whole frames, on the fused route: tike_fwd_pass1 ->
    tike_fresnel_colpass(H) -> tike_nearfield_plane_gradient (a cost-only
    evaluation, a line-search probe, stops here with out = NULL: nothing
    plane-sized is written) -> tike_fresnel_colpass(conj H) ->
    tike_ifft2_pass2_products -> tike_scatter_patches: about 8 crossings of
    the planes per gradient evaluation.  upstream = num_measured and scale =
    -1 (the blur route's convention): the wave carries MINUS the unnormalised
    gradient."""
    dev = psi.device
    S, det = probe.shape[-3], op.detector_shape
    Hh, W = psi.shape[-2:]
    ws = _workspace(op)
    how = NF.route(op.probe_shape, det, S)
    fused = how != "general"
    chunk, nmax = _whole_frames(op, probe, lo, hi, fly)
    bufs = NF.buffers(ws, dev, nmax, S, det, fly, how)
    costs = _frame_costs(op, (hi - lo) // fly, dev)
    want_psi, want_probe = want_grad and want_psi, want_grad and want_probe
    # (fused: the planar accumulator of the grouped scatter)
    grads, gpsi, gprobe = _gradient_buffer(
        psi, probe, want_psi, want_probe,
        planar=(1, 2, Hh, W) if fused else None)
    unit = D.upstream_unit(ws, "nearfield_upstream", max(nmax // fly, 1), dev,
                           cm.nmeasured)
    if fused and want_grad:
        objproj = ws.get("nearfield_objproj", (nmax, det, det),
                         torch.complex64, dev)
    inv_scale = fft_scales(det, op.norm)[1]
    st = A.stream_ptr()
    for clo in range(lo, hi, chunk):
        chi = min(hi, clo + chunk)
        sc = scan[clo:chi]
        n = chi - clo
        d = A.counts(data[clo // fly:chi // fly])
        wave, finished = NF.wave_and_back(
            op, psi, sc, probe, H, d, fly, how, bufs, model=cm.model,
            measured=cm.mask, num_measured=cm.nmeasured,
            upstream=unit[:n // fly], scale=-1.0,
            costs=costs[(clo - lo) // fly:(chi - lo) // fly],
            want_back=want_grad, unnormalised=True)
        if not want_grad:
            continue
        if not finished:
            # inverse pass 2 + object projection + probe product, as for the
            # first slice of a multislice walk back
            check(
                lib.tike_ifft2_pass2_products(
                    A.ptr(wave), A.ptr(psi[0]), A.ptr(sc), A.ptr(probe), 0,
                    A.ptr(objproj), A.ptr(gprobe), 1.0, None, 0, n, S, det,
                    Hh, W, inv_scale, st),
                "nearfield cgrad: inverse pass 2 + both products")
            if gpsi is not None:
                check(
                    lib.tike_scatter_patches(A.ptr(objproj), A.ptr(sc),
                                             A.ptr(gpsi[0]), n, det, Hh, W,
                                             st),
                    "nearfield cgrad: object gradient")
            continue
        conv = op.diffraction.diffraction
        if gpsi is not None:
            # (Convolution.adj adds into the array it is given)
            conv.adj(nearplane=wave, scan=sc, probe=probe[0], psi=gpsi[0])
        if gprobe is not None:
            gprobe += conv.adj_probe(nearplane=wave, scan=sc,
                                     psi=psi[0]).sum(dim=0)[None, None]
    if comm.collective and grads.numel():
        comm.Allreduce(grads)
    # the accumulators hold MINUS the gradients
    if gpsi is not None:
        gpsi = -torch.complex(gpsi[:, 0], gpsi[:, 1]) if fused else -gpsi
    return (costs.sum(dtype=torch.float64), gpsi,
            -gprobe if gprobe is not None else None)


MULTISLICE_FUSED = _tuning.cgrad_multislice_fused
"""128^2, 256^2 or 512^2 tiles, probe window = detector, at most 8 modes: a
multislice gradient runs on the two-pass kernels.  False: the general route
(Convolution / FresnelSpectProp / the transforms slice by slice), which is
also the route of every other shape."""

MULTISLICE_STEP_BACK_FUSED = _tuning.cgrad_multislice_step_back
"""The step back through a slice as ONE launch (`tike_slice_step_back`; 128^2
and 256^2).  False, and always at 512^2: `tike_ifft2_pass2_products(keep_chi)`
-> `tike_conv_adj_probe` -> `tike_fft2_pass1`."""


def _multislice_chunk_fused(op, psi, sc, probe, d32, costs, cm, want_grad,
                            acc, pacc, bufs):
    """One chunk on the fused kernels (module docstring; csrc/multislice.hip):
    the far plane and the walk back of `_multislice.py` around the cost
    kernel.  acc (D, 2, H, W) float32 or None and pacc (S, pw, pw) complex64
    or None receive MINUS the gradients of the chunk."""
    n, S, det = sc.shape[0], probe.shape[-3], op.detector_shape
    far, mid, beams, objproj = bufs
    st = A.stream_ptr()
    far = M.fused_far(op, psi, sc, probe, far, beams, "multislice cgrad")
    check(
        lib.tike_farplane_gradient(A.ptr(far), A.ptr(d32), A.ptr(cm.mask),
                                   None, A.ptr(costs), n, S, det, cm.model,
                                   int(want_grad), 1.0, cm.nmeasured, st),
        "multislice cgrad: cost + far-plane gradient")
    if not want_grad:
        return
    # the far plane holds MINUS the gradient, 0 at unmeasured pixels
    mid = mid[0, :n]
    check(lib.tike_fft2_pass1(A.ptr(far), A.ptr(mid), n * S, det, 1, st),
          "multislice cgrad: inverse pass 1")
    # (no object gradient wanted: the one launch forms no projection)
    inv_scale = fft_scales(det, op.norm)[1]
    M.fused_step_back(op, psi, sc, probe, far, mid, beams[:, :n],
                      objproj[:, :n], acc, pacc, first_scale=inv_scale,
                      scale=inv_scale, want_proj=acc is not None,
                      one_launch=MULTISLICE_STEP_BACK_FUSED,
                      label="multislice cgrad")


def _multislice_chunk_general(op, psi, sc, probe, d32, costs, cm, want_grad,
                              gpsi, gprobe):
    """One chunk through the general operators, any probe window = detector
    size.  gpsi (D, H, W) / gprobe (1, 1, S, pw, pw) complex64 or None
    receive MINUS the gradients of the chunk."""
    D = psi.shape[0]
    n, S, det = sc.shape[0], probe.shape[-3], op.detector_shape
    conv, fresnel = op.diffraction.diffraction, op.diffraction.propagation
    far, beams = M.general_far(op, psi, sc, probe)
    check(
        lib.tike_farplane_gradient(A.ptr(far), A.ptr(d32), A.ptr(cm.mask),
                                   None, A.ptr(costs), n, S, det, cm.model,
                                   int(want_grad), 1.0, cm.nmeasured,
                                   A.stream_ptr()),
        "multislice cgrad: cost + far-plane gradient")
    if not want_grad:
        return
    wave = op.propagation.adj(far, overwrite=True)
    for d in range(D - 1, -1, -1):
        if gpsi is not None:
            # (Convolution.adj adds into the array it is given)
            conv.adj(nearplane=wave, scan=sc, probe=beams[d], psi=gpsi[d])
        if d == 0 and gprobe is None:
            break
        wave = conv.adj_probe(nearplane=wave, scan=sc, psi=psi[d])
        if d > 0:
            wave = fresnel.adj(wave, overwrite=True)
        else:
            gprobe += wave.sum(dim=0)[None, None]


def _multislice_chunk(op, psi, probe):
    """Positions per chunk of `_multislice_cost_and_grad`.  Fused route: far +
    mid + D - 1 sets of incident probes within HALF the HBM that is free right
    now, as rpie's fused multislice chunks are sized (asked once per
    minibatch: every evaluation of its line searches then splits alike)."""
    return M.chunk_positions(
        op, psi.device, probe.shape[-3], psi.shape[0] + 1,
        M.fused_route(op, probe, MULTISLICE_FUSED))


def _multislice_cost_and_grad(op, comm, data, psi, scan, probe, lo, hi, *,
                              want_psi, want_probe, want_grad, cm, chunk=None):
    """(sum of this rank's per-pattern costs, a device scalar; d cost / d psi
    (D, H, W) or None; d cost / d probe or None -- unnormalised adjoints
    summed over the ranks, as `_cost_and_grad` returns them) of the positions
    [lo, hi) for an object of several slices: the exact adjoint through every
    slice, no division by the number of slices.  Chunk by chunk (`chunk`
    positions each; None: `_multislice_chunk`); a line-search probe (want_grad
    False) stops behind the cost."""
    op.diffraction._check_slices(psi)
    dev, D, S = psi.device, psi.shape[0], probe.shape[-3]
    N = hi - lo
    ws = _workspace(op)
    fused = M.fused_route(op, probe, MULTISLICE_FUSED)
    want_psi, want_probe = want_grad and want_psi, want_grad and want_probe
    if chunk is None:
        chunk = _multislice_chunk(op, psi, probe)
    if fused:
        bufs = M.fused_buffers(op, dev, D, S, max(1, min(chunk, N)))
    costs = ws.get("costs", (max(N, 1),), torch.float32, dev)[:N]
    # (fused: the planar accumulators of the grouped scatter)
    grads, gpsi, gprobe = _gradient_buffer(
        psi, probe, want_psi, want_probe,
        planar=(D, 2, *psi.shape[-2:]) if fused else None)
    for clo in range(lo, hi, chunk):
        chi = min(hi, clo + chunk)
        sc = scan[clo:chi]
        d32 = A.data_f32(data, clo, chi)
        c = costs[clo - lo:chi - lo]
        if fused:
            _multislice_chunk_fused(
                op, psi, sc, probe, d32, c, cm, want_grad, gpsi,
                gprobe[0, 0] if gprobe is not None else None, bufs)
        else:
            _multislice_chunk_general(op, psi, sc, probe, d32, c, cm,
                                      want_grad, gpsi, gprobe)
    if comm.collective and grads.numel():
        comm.Allreduce(grads)
    # the accumulators hold MINUS the gradients
    if gpsi is not None:
        gpsi = -torch.complex(gpsi[:, 0], gpsi[:, 1]) if fused else -gpsi
    return (costs.sum(dtype=torch.float64), gpsi,
            -gprobe if gprobe is not None else None)


class _Minibatch:
    """The cost of the positions [lo, hi) of this rank -- all that the epoch
    loop and `_host_cg` know of a minibatch, whichever of the kinds (module
    docstring) it is.

    evaluate(psi, probe, variable, want_grad, position_terms=None, a=None) ->
        (this rank's cost sum, a device float64 scalar; with want_grad MINUS
        d cost / d variable -- the unnormalised adjoint, summed over the ranks
        -- else None).  variable: 0 the object, 1 the probe, 2 the root a of
        the detector's fitted table (minibatches with a `state` only; `a` is
        then the point of evaluation, psi and probe those of the block's
        start), None cost only.
        position_terms: plain minibatches only, see `_cost_and_grad`.
    start(psi, probe, variable) -> where the conjugate gradient of `variable`
        starts.
    finish(total) -> the mean cost over all ranks, a host float: the one
        read-back of an evaluation.
    on_device: line searches may be decided on the device (`_cg_on_device`,
        which wants `plan` and `count`): plain minibatches only.

    detector: the `operators.detector.Detector` of the reconstruction; state:
    the `State` of ptycho/background.py or ptycho/blur.py, whose `value` then
    stands in the detector's, or None.

    Every rank builds every minibatch and makes every collective, whatever
    its share."""

    on_device = False

    def __init__(self, op, comm, data, psi, scan, probe, lo, hi, cm, fly,
                 detector=D.Detector(), state=None):
        self.where = (op, comm, data), scan, (lo, hi)
        self.detector, self.state = detector, state
        self.stored = None  # the intensities of the third block
        self.finish = lambda total: _finish_cost(total, comm, op, lo, hi, fly)
        if psi.shape[0] > 1:  # (every evaluation splits into the same chunks)
            self.run = _multislice_cost_and_grad
            self.how = dict(cm=cm, chunk=_multislice_chunk(op, psi, probe))
        elif fly > 1 or detector.kind != "far" or not PLAIN_ROUTE:
            if lo % fly or hi % fly:
                raise ValueError(
                    f"minibatch [{lo}, {hi}) does not hold whole frames of "
                    f"fly={fly} positions")
            global_count(comm, op, lo, hi)  # (all-reduced ahead of the passes)
            self.run = (_nearfield_cost_and_grad
                        if detector.kind == "nearfield" else _fly_cost_and_grad)
            self.how = dict(cm=cm, fly=fly)
        else:
            self.plan = _CostPlan(op, data, psi, scan, probe, lo, hi, cm)
            self.run = _cost_and_grad
            self.how = dict(cm=cm, read_cost=False, plan=self.plan)
            # line searches decided on the device: one rank, HBM-resident
            # data, the far-plane-free sizes and 128^2
            # (several ranks: the all-at-once search, whose cost sums are
            # all-reduced between its cost passes and its decisions -- every
            # rank must take the same route, so every rank must hold positions)
            self.on_device = (DEVICE_LINE_SEARCH and hi > lo
                              and isinstance(data, torch.Tensor)
                              and self.plan.supports_gradients())
            if comm.collective:
                self.on_device = (LINEAR_LINE_SEARCH and not USE_GRAPHS
                                  and _every_rank(comm, op, lo, hi,
                                                  self.on_device))
            self.count = global_count(comm, op, lo, hi)

    def start(self, psi, probe, variable):
        return (psi, probe, getattr(self.state, "a", None))[variable]

    def evaluate(self, psi, probe, variable, want_grad, position_terms=None,
                 a=None):
        (op, comm, data), scan, (lo, hi) = self.where
        how = self.how if position_terms is None else dict(
            self.how, position_terms=position_terms)
        if self.run is _nearfield_cost_and_grad:
            how = dict(how, H=self.detector.value)
        elif self.run is _fly_cost_and_grad:
            how = dict(how, detector=self.detector if self.state is None else
                       self.detector._replace(value=self.state.value))
        if variable == 2:
            fly = how["fly"]
            if self.stored is None:
                # the intensities at the block's object and probe, once: they
                # depend on neither the background nor the kernel
                nframe = (hi - lo) // fly
                self.stored = _workspace(op).get(
                    "background_intensity",
                    (max(nframe, 1), op.detector_shape, op.detector_shape),
                    torch.float32, psi.device)[:nframe]
                self.run(op, comm, data, psi, scan, probe, lo, hi,
                         want_psi=False, want_probe=False, want_grad=False,
                         stored=self.stored, **how)
            return self.state.cost_and_grad(
                op, A.counts(data[lo // fly:hi // fly]), self.stored, a,
                how["cm"], want_grad)
        r = self.run(op, comm, data, psi, scan, probe, lo, hi,
                     want_psi=variable == 0, want_probe=variable == 1,
                     want_grad=want_grad, **how)
        return r[0], None if variable is None else r[1 + variable]


def _host_cg(minibatch, psi, probe, variable, o, positions=None):
    """`opt.conjugate_gradient` on the object (variable 0), the probe (1) or
    the root of the detector's fitted table (2: real float32, the `a` of the
    minibatch's `state`) of one minibatch, every line search decided on the host:
    (x, mean cost).
    positions: the `_PositionTerms` of the epoch; the first gradient pass
    takes the minibatch's sums if they are still owed.

    A gradient pass forms the cost of its argument as well: it is kept ON THE
    DEVICE and read back only if the line search asks for the cost of that
    very array (opt.line_search does, for its starting point) -- which then
    costs neither a forward pass nor, for the other gradient evaluations, a
    host synchronisation."""
    last = [None, None]  # the array of the last gradient pass, its cost sum

    def run(x, want_grad):
        return minibatch.evaluate(
            x if variable == 0 else psi, x if variable == 1 else probe,
            variable, want_grad,
            positions.take() if want_grad and positions is not None else None,
            **(dict(a=x) if variable == 2 else {}))

    def cost(x):
        return minibatch.finish(last[1] if x is last[0] else run(x, False)[0])

    def grad(x):
        last[1], g = run(x, True)
        last[0] = x
        return [g]

    return opt.conjugate_gradient(
        torch, x=minibatch.start(psi, probe, variable),
        cost_function=cost, grad=grad,
        dir_multi=lambda x: x[0], num_iter=o.cg_iter,
        step_length=o.step_length)


def cgrad(parameters, data, batches, comm, *, op, epoch):
    """One epoch: for every minibatch, `cg_iter` CG iterations on psi, then
    (when probe recovery is on) on the probe and then (with a background that
    is fitted) on the root of the background; with position_options, one
    position update after the last minibatch (every minibatch of the epoch
    saw the old positions, as in lstsq_grad and rpie)."""
    o = parameters.algorithm_options
    fly = _fly_of(op, data, parameters.scan)
    # what `Reconstruction` set; an operator of another maker: the far field
    detector = getattr(op, "detector", D.Detector())
    third = getattr(op, "detector_state", None)
    _refuse(parameters, fly, binning=detector.binning)
    recover = (parameters.object_options is not None,
               parameters.probe_options is not None
               and epoch >= parameters.probe_options.update_start,
               third is not None and bool(third.options.update)
               and epoch >= third.options.update_start)
    psi, probe, scan = parameters.psi, parameters.probe, parameters.scan
    # (the mask and the pixel count are at data resolution)
    cm = _cost_model(parameters.exitwave_options,
                     detector.width(op.detector_shape))
    position_options = parameters.position_options  # (plain minibatches only)
    positions = None
    if position_options is not None:
        if position_options.use_position_regularization and epoch > 0:
            # the affine pull that followed the last epoch moved the positions
            # after they were tested (as rpie does at its entry)
            _raise_unless_allowed(
                float(_positions_flag(scan, psi, probe, comm)), scan, psi,
                probe)
        if epoch >= position_options.update_start:
            positions = _PositionTerms(scan)
    batch_cost = []
    for batch_index, b in enumerate(batches):
        lo = int(b[0]) if len(b) else 0
        hi = lo + len(b)
        comm.minibatch = batch_index
        mb = _Minibatch(op, comm, data, psi, scan, probe, lo, hi, cm, fly,
                        detector, third)
        if positions is not None:
            positions.pending = True
            # the object's first gradient pass writes the projection the sums
            # need; without one (object not recovered, no CG iteration, or a
            # CG call replayed from a graph) one extra gradient pass of the
            # minibatch, nothing accumulated: every rank decides alike
            if not (recover[0] and o.cg_iter >= 1
                    and not (mb.on_device and USE_GRAPHS)):
                mb.evaluate(psi, probe, None, True, positions.take())
        cost = None
        # CG on the object, then on the probe, then on the background's root
        for variable in (0, 1, 2):
            if not recover[variable]:
                continue
            owed = positions if variable == 0 else None
            r = None
            if mb.on_device:
                r = _cg_on_device(mb.plan, op, comm, psi, probe, variable, o,
                                  mb.count, data, scan, lo, hi,
                                  positions=owed)
            if r is None:
                r = _host_cg(mb, psi, probe, variable, o, owed)
            x, cost = r
            if variable == 2:
                third.set(x)
                continue
            psi, probe = (x, probe) if variable == 0 else (psi, x)
        if cost is None:  # no variable recovered: the cost alone
            cost = mb.finish(mb.evaluate(psi, probe, None, False)[0])
        batch_cost.append(cost)
    o.costs.append([float(np.mean(batch_cost))])  # (host floats, all of them)
    if positions is not None:
        # the minibatches above all used the old positions
        numerator = positions.numerator
        if cm.model == MODELS["poisson"]:
            numerator = POISSON_POSITION_STEP * numerator
        scan = _update_position(scan, position_options, numerator,
                                positions.denominator, comm, alpha=o.alpha,
                                epoch=epoch)
        # ... and the new ones must not reach a kernel unless every patch
        # stays inside the object
        _raise_unless_allowed(float(_positions_flag(scan, psi, probe, comm)),
                              scan, psi, probe)
        parameters.scan = scan
    parameters.psi, parameters.probe = psi, probe
    return parameters
