"""A differentiable intensity model for ``torch.autograd`` over the HIP
operators.

``intensity(operator, psi, probe, scan, fly=...)`` returns the diffraction
intensities of `Ptycho._compute_intensity` as a tensor that takes part in
PyTorch's autograd graph: any loss written in PyTorch gets exact gradients
with respect to the object, the probe AND the scan positions, fly scans
included.  No solver is involved; the solvers keep their hand-written adjoints
and their refusals.

Backward, in PyTorch's convention (a complex leaf's ``.grad`` is
dL/dRe + i dL/dIm), with g = dL/dI (FRAME, det, det) and f(n) the frame that
position n exposes:

    G[n,s]        = 2 g[f(n)] far[n,s]
    chi[n,s]      = crop_pw(F^H G[n,s])          F = the operator's transform
    probe.grad[s] = sum_n conj(patch_n) chi[n,s]
    objproj[n]    = sum_s conj(probe_s) chi[n,s]
    psi.grad      = scatter_n(objproj[n])        adjoint of the bilinear gather
    scan.grad[n]  = sum_px Re((Dy_n, Dx_n) conj(objproj[n]))

F^H is the unscaled inverse transform times the FORWARD scale of the
operator's `norm` (for "ortho" that is the operator's inverse; for "backward"
and "forward" the operator's inverse is F^-1, not F^H, and would be wrong by
det^2).  Dy, Dx: the derivative of the bilinear patch with the integer part
of the position held fixed (`tike_scan_gradient`, include/tike_amd.h).

Per chunk of whole frames (`chunk_positions`), recomputing the forward -- at
most one chunk of far plane is ever resident:

    tike_ptycho_fwd -> tike_ifft2_crop_scaled (128, 256, 512: g applied while
    the inverse loads; other sizes tike_farplane_scale + tike_ifft2_crop) ->
    tike_lstsq_gradients -> tike_scatter_patches -> tike_scan_gradient

No torch arithmetic on that path: views, allocation and the final
planar-to-complex conversion of the object gradient only.

``intensity(..., eigen_probe=E, eigen_weights=w)`` is the same with the
varying probe of the reference's `get_varying_probe` (probe.py:272-303), E
(1, C, M, pw, pw), w (N, C + 1, S), weights per POSITION (any `fly`):

    P[n,s] = w[n,0,s] probe[s] + sum_c w[n,c+1,s] E[c,s]    s < M
    P[n,s] = w[n,0,s] probe[s]                               s >= M

Backward, with chi as above (far from P) and q[n,s] = conj(patch_n) chi[n,s]:

    probe.grad[s]      = sum_n w[n,0,s]   q[n,s]
    E.grad[c,s]        = sum_n w[n,c+1,s] q[n,s]                   s < M
    w.grad[n,0,s]      = sum_px Re(conj(probe[s]) q[n,s])
    w.grad[n,c+1,s]    = sum_px Re(conj(E[c,s])   q[n,s])          s < M; 0 else
    objproj[n]         = sum_s conj(P[n,s]) chi[n,s]   -> psi.grad, scan.grad

all five from ONE pass over chi, `tike_eigen_probe_gradients` in the place of
`tike_lstsq_gradients`; the other launches are unchanged, and without
eigen_weights nothing changes at all.

``multislice_intensity(operator, psi, probe, scan, fly=...)`` is the same for
an object of D slices (probe window = detector): e_d = patch_n(O_d) beam_d,
beam_0 = the probe, beam_{d+1} = Fresnel(e_d), far = F e_{D-1}.  Backward, the
exact adjoint through every slice with no division by D:

    G[n,s]       = 2 g[f(n)] far[n,s]
    w_{D-1}      = F^H G
    objproj_d[n] = sum_s conj(beam_d[n,s]) w_d[n,s]
    psi.grad[d]  = scatter_n(objproj_d[n])
    w_{d-1}      = Fresnel^H(conj(patch_n(O_d)) w_d)   F^-1 conj(H) F: the
                                                       same for every `norm`
    probe.grad   = sum_n conj(patch_n(O_0)) w_0
    scan.grad[n] = sum_d sum_px Re((Dy_n,d, Dx_n,d) conj(objproj_d[n]))

Per chunk of whole frames, the forward recomputed, on the route `cgrad` takes
for the shape (`fused_slices`; its `MULTISLICE_FUSED` and
`MULTISLICE_STEP_BACK_FUSED` are honoured) and through cgrad's own code: the
route, the chunk, the `ms_*` buffers, the forward of a chunk and the fused
step back are the functions of ptycho/solvers/_multislice.py, called with
F^H's scale and a projection plane per slice:

* fused (128^2, 256^2, 512^2, at most 8 modes): `fused_forward` ->
  tike_fft2_pass2_inplace -> tike_ifft2_pass1_scaled (g applied while inverse
  pass 1 loads; the factor 2 and the forward scale ride on the pass 2 behind
  it) -> per slice tike_slice_step_back (512^2, or the lever off:
  tike_ifft2_pass2_products(keep_chi) -> tike_conv_adj_probe ->
  tike_fft2_pass1) -> tike_scatter_patches -> tike_fresnel_colpass(adjoint);
  slice 0: tike_ifft2_pass2_products with the probe gradient;
* general (any other probe window = detector, at most MAX_MODES modes):
  Convolution / FresnelSpectProp / tike_fft2 slice by slice,
  tike_farplane_scale for g, tike_lstsq_gradients for every slice's objproj;

then ONE tike_scan_gradient_slices over the D objproj planes of the chunk.
Only what `needs_input_grad` asks for is launched.

Forward mode.  ``intensity_jvp(operator, psi, probe, scan, d_psi=, d_probe=,
d_scan=, fly=...)`` returns (I, dI = J v) for tangents d_psi (1, H, W), d_probe
(1, 1, S, pw, pw) and d_scan (N, 2) -- one slice, the shared probe, any `fly`,
the operator's `norm`; Dy, Dx as above (`tike_scan_gradient`: the integer part
of the position held fixed, a tap outside the object zero):

    dpatch_n   = patch_n(d_psi) + d_scan[n,0] Dy_n(psi) + d_scan[n,1] Dx_n(psi)
    dwave[n,s] = dpatch_n probe[s] + patch_n(psi) d_probe[s]
    dfar[n,s]  = F pad(dwave[n,s])                F with its forward scale
    dI[f]      = sum_{n in frame f} sum_s 2 Re(conj(far[n,s]) dfar[n,s])

Per chunk of whole frames -- half of `chunk_positions`: the far plane and its
tangent are both resident --

    tike_ptycho_fwd -> tike_conv_fwd_tangent -> tike_fft2 (in place, forward
    scale) -> tike_intensity_tangent (dI, and I with the bits of
    tike_intensity)

and with no tangent at all only the primal launches.  `intensity` on
``torch.autograd.forward_ad`` dual tensors (any subset of psi, probe, scan)
returns a dual whose tangent is this dI: `_Intensity.jvp` runs the same chunk
loop (`_jvp_chunks`, the one loop of the one-slice forms: with eigen weights
it launches tike_eigen_wave_tangent, as below).  The eigen-probe form and
`multislice_intensity` have no forward-mode
RULE: under `forward_ad` they keep torch's own refusal ("you must implement
the jvp function"); their forward mode is a function each,
`eigen_intensity_jvp` and `multislice_intensity_jvp` below.
``gauss_newton_product`` composes the two modes: J^T (weight * J v) by
`intensity_jvp` and then the backward above.

Forward mode, several slices.  ``multislice_intensity_jvp(operator, psi, probe,
scan, d_psi=, d_probe=, d_scan=, fly=...)`` returns (I, dI = J v) of
`multislice_intensity` for tangents d_psi (D, H, W), d_probe (1, 1, S, pw, pw)
and d_scan (N, 2); the Fresnel step is linear, so the tangent of a beam is the
Fresnel step of the tangent of the exit wave in front of it:

    beam_0 = probe                      dbeam_0 = d_probe
    dpatch_{n,d} = patch_n(d_psi[d]) + d_scan[n,0] Dy_n(psi[d])
                                     + d_scan[n,1] Dx_n(psi[d])
    e_d  = patch_n(psi[d]) beam_d
    de_d = dpatch_{n,d} beam_d + patch_n(psi[d]) dbeam_d
    beam_{d+1} = Fresnel(e_d)           dbeam_{d+1} = Fresnel(de_d)
    far = F e_{D-1}    dfar = F de_{D-1}
    dI[f] = sum_{n in frame f} sum_s 2 Re(conj(far) dfar)

Per chunk of whole frames -- the far plane, the D - 1 sets of incident beams
and ONE tangent set are resident, one set more than the forward holds --

    the primal as `multislice_intensity` runs it (`_SlicesForward`, the one
    forward of a chunk, over `fused_far` or `general_far` of
    ptycho/solvers/_multislice.py, cgrad's own: I has its bits;
    both leave the beam incident on every slice) -> per slice
    tike_slice_wave_tangent, de_d written over dbeam_d in
    place (slice 0: the shared probe and d_probe), and between two slices the
    Fresnel step of the tangent (fused route: tike_fft2_pass1 ->
    tike_fresnel_colpass -> tike_fft2_pass2_inplace with the scale of
    `fused_far`, measured faster; general route: tike_fresnel_spect_prop in
    place) -> tike_fft2 (in place, forward scale) -> tike_intensity_tangent

with no torch arithmetic; no tangent at all: only the primal launches.  One
slice goes through the chunk loop of `intensity_jvp`.  There is still no
forward-mode RULE for `_MultisliceIntensity`: dual tensors stay refused, the
function is the interface.  ``multislice_gauss_newton_product`` is
`gauss_newton_product` for this model: the JVP without the primal intensity,
then the backward of `multislice_intensity` with weight * dI upstream.

Forward mode, eigen probes.  ``eigen_intensity_jvp(operator, psi, probe, scan,
eigen_probe=, eigen_weights=, d_psi=, d_probe=, d_scan=, d_eigen_probe=,
d_eigen_weights=, fly=...)`` returns (I, dI = J v) of `intensity(...,
eigen_probe=, eigen_weights=)` for tangents of all five inputs (d_eigen_probe
(1, C, M, pw, pw), d_eigen_weights (N, C + 1, S); eigen_probe=None is C = 0):
the varying probe is linear in the planes and in the weights, so with P as
above

    dP[n,s]    = w[n,0,s] d_probe[s] + d_w[n,0,s] probe[s]
               + sum_c (w[n,c+1,s] d_E[c,s] + d_w[n,c+1,s] E[c,s])    s < M
                 (the first two terms alone for s >= M)
    dpatch_n   = patch_n(d_psi) + d_scan[n,0] Dy_n(psi) + d_scan[n,1] Dx_n(psi)
    dwave[n,s] = dpatch_n P[n,s] + patch_n(psi) dP[n,s]
    dfar[n,s]  = F pad(dwave[n,s])
    dI[f]      = sum_{n in frame f} sum_s 2 Re(conj(far[n,s]) dfar[n,s])

Per chunk of whole frames -- half of `chunk_positions`, as above --

    tike_ptycho_fwd (with the eigen probes: I has the bits of `intensity`) ->
    tike_eigen_wave_tangent (P and dP built in registers, never stored;
    d_scan and d_eigen_weights sliced to the chunk) -> tike_fft2 (in place,
    forward scale) -> tike_intensity_tangent

with no torch arithmetic; no tangent at all: only the primal launches.  There
is no forward-mode rule for `_EigenIntensity` either: the function is the
interface.  ``eigen_gauss_newton_product`` is `gauss_newton_product` for this
model over the five inputs: the JVP without the primal intensity, then the
backward of the eigen form with weight * dI upstream.

The noise-model cost.  ``cost(operator, data, psi, probe, scan, model=,
measured_pixels=, eigen_probe=, eigen_weights=, fly=...)`` returns the
per-frame costs of `Ptycho.cost`'s two noise models on the measured pixels,
differentiable with respect to every input of the form it dispatches to
(several slices, eigen probes, or plain):

    gaussian: cost_f = mean_p (sqrt(I) - sqrt(d))^2,  l' = 1 - sqrt(d) / (sqrt(I) + 1e-9)
    poisson:  cost_f = mean_p I - d log(I + 1e-9),    l' = 1 - d / (I + 1e-9)

Forward, per chunk of whole frames: the form's forward (`_one_slice_far` or
`_SlicesForward`, as everywhere in this module) -> tike_cost_factor (costs).
Backward, per chunk: the forward again -> tike_cost_factor (the chunk's table
upstream_f l' / num_measured, 0 under the mask) -> the form's backward chain
from the point where it reads the table (`_Back.run`, `_fused_back`,
`_general_back`: shared with the three backwards above, which hand them
``g[lo // fly:hi // fly]``).  ``cost_jvp`` runs the form's
forward-mode chunk loop with tike_cost_curvature in the place of
tike_intensity_tangent: (costs, dcosts = sum_p l' dI / num_measured).
``cost_gauss_newton_product`` is J^T diag(upstream_f c / (num_measured
(I + floor))) J v, c = 1/2 (gaussian) or 1 (poisson): for one slice ONE chunk
loop with the far plane resident --

    the forward-mode launches of the form -> tike_cost_curvature (the chunk's
    table) -> `_Back.run` on the SAME far plane (the scaled inverse writes
    into the tangent's far plane)

-- and for several slices the forward-mode chunks (the table over all frames)
followed by the backward of `multislice_intensity`.  No tensor of
N // fly * det * det elements exists in `cost`, `cost_jvp` or the one-slice
product.  ``cost(..., binning=B)`` is the same cost with the far plane B times
finer than the counts (a measured pixel the sum over its B x B far-plane
pixels): tike_binned_cost_factor in the place of tike_cost_factor, its table
at far-plane resolution with a bin's value on each of its pixels, the chain
behind it unchanged; `cost_jvp` and `cost_gauss_newton_product` refuse
binning > 1 by name.  ``cost(..., blur=K)`` is the same cost at K (*) I, the
cyclic convolution of each frame's intensity with a (k, k) kernel (partial
coherence, a detector's point-spread function): per chunk tike_intensity stores
the intensities and tike_blur_cost_factor, in the place of tike_cost_factor,
writes costs or the table K (star) (g mask l' / num_measured), the chain behind
it unchanged; K.grad is the sum of the chunks' tike_blur_kernel_sums; `cost_jvp`
and `cost_gauss_newton_product` take no blur.  ``cost(..., nearfield=H)`` puts
the detector in the near field, I = |IFFT2(H FFT2(patch x probe))|^2 with probe
window = detector (one slice, the shared probe): a Function of its own,
`_NearfieldCost`, over `operators.nearfield.wave_and_back` -- forward
tike_fwd_pass1 -> tike_fresnel_colpass -> tike_nearfield_plane_gradient with
out = NULL, backward the same chunk with grad_output for the upstream, the
adjoint Fresnel step and the tail of `_Back` (tike_lstsq_gradients,
tike_scatter_patches, tike_scan_gradient); H takes no gradient; `cost_jvp` and
`cost_gauss_newton_product` take no nearfield.

The entries share their bodies: the three `*_jvp` functions are `_jvp`, the
three `*_gauss_newton_product` functions `_gauss_newton`, over `_checked_jvp`
(the refusals), `_apply` (the form's `Function`) and `_jvp_loop` (its
forward-mode chunk loop), each of which tells the forms apart by the inputs
(psi, probe, scan, eigen_probe, eigen_weights) it is handed.
"""
import importlib

import torch
from torch.autograd.function import once_differentiable

from . import _arrays as A
from ._lib import check, lib
from .operators import detector as _D
from .operators.multislice import Multislice
from .operators.propagation import fft_scales
from .ptycho.solvers import _multislice

MAX_MODES = 16
"""Probe modes `tike_lstsq_gradients` takes (TK_MAX_MODES)."""

MAX_EIGEN_PLANES = 16
"""Eigen planes C * M (eigen probes x the modes that own them)
`tike_eigen_probe_gradients` takes."""

_SCALED_INVERSE_SIZES = (128, 256, 512)
"""Detector sizes of `tike_ifft2_crop_scaled`."""


def _checked(operator, psi, probe, scan, fly, check_positions,
             name="intensity", slices=False, eigen_probe=None,
             eigen_weights=None):
    """Every refusal, in an order that needs no device until the last one.
    slices: `multislice_intensity` -- any number of slices, whose shapes
    `Multislice.check_slice_shapes` judges.  eigen_probe, eigen_weights: the
    varying probe of `intensity`."""
    depth = "D" if slices else "1"
    if eigen_probe is not None and eigen_weights is None:
        raise ValueError(
            f"{name}: eigen_probe without eigen_weights (the weights say how "
            "much of every eigen probe a position sees)")
    given = [("psi", psi, torch.complex64), ("probe", probe, torch.complex64),
             ("scan", scan, torch.float32)]
    if eigen_probe is not None:
        given.append(("eigen_probe", eigen_probe, torch.complex64))
    if eigen_weights is not None:
        given.append(("eigen_weights", eigen_weights, torch.float32))
    for what, x, dtype in given:
        if not isinstance(x, torch.Tensor):
            raise TypeError(
                f"{name}: {what} must be a torch device tensor, not "
                f"{type(x).__name__} (host arrays take part in no autograd "
                "graph)")
        if x.dtype != dtype:
            raise TypeError(f"{name}: {what} must be {dtype}, not {x.dtype}")
    if (psi.ndim != 3 or probe.ndim != 5 or scan.ndim != 2
            or scan.shape[1] != 2 or (slices and psi.shape[0] < 1)):
        raise ValueError(
            f"{name}: psi ({depth}, H, W), probe (1, 1, S, pw, pw) and scan "
            f"(N, 2) expected; got {tuple(psi.shape)}, {tuple(probe.shape)}, "
            f"{tuple(scan.shape)}")
    if psi.shape[0] > 1 and not slices:
        raise NotImplementedError(
            f"intensity with several slices (psi.shape[0] = {psi.shape[0]}): "
            "multislice_intensity is the differentiable model of a "
            "multislice object")
    if probe.shape[0] != 1:
        raise NotImplementedError(
            f"{name} with a probe per position (probe.shape[0] = "
            f"{probe.shape[0]}): a probe tensor per position is not "
            "implemented; intensity(..., eigen_probe=, eigen_weights=) is the "
            "varying probe of shared probe + weighted eigen probes")
    pw, det = operator.probe_shape, operator.detector_shape
    if probe.shape[1] != 1 or tuple(probe.shape[-2:]) != (pw, pw):
        raise ValueError(
            f"{name}: probe must be (1, 1, S, {pw}, {pw}) for this "
            f"operator, not {tuple(probe.shape)}")
    if tuple(psi.shape[-2:]) != (operator.nz, operator.n):
        raise ValueError(
            f"{name}: psi must be ({depth}, {operator.nz}, {operator.n}) for "
            f"this operator, not {tuple(psi.shape)}")
    Multislice.check_slice_shapes(psi.shape[0], det, pw)
    fly = int(fly)
    if fly < 1 or scan.shape[0] % fly:
        raise ValueError(
            f"{scan.shape[0]} scan positions are not a multiple of fly={fly}")
    if probe.shape[2] > MAX_MODES:
        raise ValueError(
            f"{name}: {probe.shape[2]} probe modes; the gradient kernels "
            f"take at most {MAX_MODES}")
    if eigen_weights is not None:
        N, S = scan.shape[0], probe.shape[2]
        if eigen_weights.ndim != 3 or (eigen_probe is not None
                                       and eigen_probe.ndim != 5):
            raise ValueError(
                f"{name}: eigen_weights (N, C + 1, S) and eigen_probe "
                f"(1, C, M, pw, pw) expected; got "
                f"{tuple(eigen_weights.shape)}"
                + ("" if eigen_probe is None else
                   f", {tuple(eigen_probe.shape)}"))
        C, M = (0, 0) if eigen_probe is None else eigen_probe.shape[1:3]
        if eigen_probe is not None and (
                eigen_probe.shape[0] != 1 or C < 1 or not 1 <= M <= S
                or tuple(eigen_probe.shape[-2:]) != (pw, pw)):
            raise ValueError(
                f"{name}: eigen_probe must be (1, C, M, {pw}, {pw}) with "
                f"C >= 1 and 1 <= M <= S = {S} for this probe, not "
                f"{tuple(eigen_probe.shape)}")
        if tuple(eigen_weights.shape) != (N, C + 1, S):
            raise ValueError(
                f"{name}: eigen_weights must be (N, C + 1, S) = ({N}, "
                f"{C + 1}, {S}) for these positions, eigen probes and modes, "
                f"not {tuple(eigen_weights.shape)}")
        if C * M > MAX_EIGEN_PLANES:
            raise ValueError(
                f"{name}: {C} eigen probes on {M} modes are {C * M} planes; "
                f"the gradient kernel takes at most {MAX_EIGEN_PLANES}")
    if check_positions and scan.shape[0]:
        # (the fused scatter drops what falls outside the object)
        from .ptycho.position import check_allowed_positions
        check_allowed_positions(scan, psi, probe.shape)
    for what, x, _ in given:
        if x.device.type != "cuda":
            raise TypeError(
                f"{name}: {what} lives on {x.device}; tike_amd runs on the "
                "GPU only and there is no CPU fallback")
    return fly


def _chunk_rows(op, probe, fly, halve=False):
    """Positions per chunk of the one-slice forms, whole frames.  halve: the
    far plane and its tangent are both resident."""
    from .ptycho.solvers.lstsq import chunk_positions
    chunk = chunk_positions(probe.shape[2], op.detector_shape)
    return max(1, chunk // (2 if halve else 1) // fly) * fly


def _one_slice_far(op, psi, probe, scan, eigen, weights, lo, hi, out):
    """The far plane of the positions lo ... hi - 1 of a one-slice form in
    out[:hi - lo]: tike_ptycho_fwd, with the eigen operands unless weights is
    None."""
    far = out[:hi - lo]
    if weights is None:
        op.fwd_device(probe, scan[lo:hi], psi, out=far)
    else:
        op.fwd_device(probe, scan[lo:hi], psi, eigen, weights[lo:hi], out=far)
    return far


class _Back:
    """The backward chain of the one-slice forms behind the far plane, shared
    by `_Intensity.backward`, `_EigenIntensity.backward`, the backward of
    `cost` and the resident `cost_gauss_newton_product`: the buffers of a
    chunk of at most `rows` positions, the accumulated gradients, and per
    chunk the launches from the point where the upstream table is read.
    weights (with eigen or None: C = 0) selects the eigen form, which swaps
    tike_lstsq_gradients for tike_eigen_probe_gradients.  want: (psi, probe,
    scan, eigen_probe, eigen_weights).  resident: the caller brings the far
    plane and a second buffer of its size to `run`; none is allocated here."""

    def __init__(self, op, fly, psi, probe, scan, want, rows, eigen=None,
                 weights=None, resident=False):
        from .ptycho.solvers.lstsq import _workspace
        (self.want_psi, self.want_probe, self.want_scan, want_eigen,
         want_weights) = want
        self.op, self.fly = op, fly
        self.psi, self.probe, self.scan = psi, probe, scan
        self.eigen, self.weights = eigen, weights
        self.want_eigen = bool(want_eigen) and eigen is not None
        self.want_weights = bool(want_weights) and weights is not None
        S = probe.shape[2]
        C, M = eigen.shape[1:3] if eigen is not None else (0, 0)
        pw, det = op.probe_shape, op.detector_shape
        H, W = psi.shape[-2:]
        dev = psi.device
        # F^H = the unscaled inverse x the forward scale; the 2 of G goes along
        self.scale = 2.0 * fft_scales(det, op.norm)[0]
        self.scaled_inverse = det in _SCALED_INVERSE_SIZES
        self.acc = (torch.zeros((2, H, W), dtype=torch.float32, device=dev)
                    if self.want_psi else None)
        self.gprobe = torch.zeros_like(probe) if self.want_probe else None
        self.geigen = torch.zeros_like(eigen) if self.want_eigen else None
        self.gweights = (torch.empty_like(weights) if self.want_weights
                         else None)
        self.gscan = torch.empty_like(scan) if self.want_scan else None
        self.far_all = None if resident else torch.empty(
            (rows, 1, S, det, det), dtype=torch.complex64, device=dev)
        # (the scaled inverse must not work in place; the plain one may: None)
        self.mid_all = (torch.empty((rows, 1, S, det, det),
                                    dtype=torch.complex64, device=dev)
                        if self.scaled_inverse and not resident else None)
        self.chi_all = None if pw == det else torch.empty(
            (rows, 1, S, pw, pw), dtype=torch.complex64, device=dev)
        self.need_proj = self.want_psi or self.want_scan
        self.objproj_all = (torch.empty((rows, pw, pw), dtype=torch.complex64,
                                        device=dev)
                            if self.need_proj else None)
        # the pixel tiles' partial weight sums (include/tike_amd.h): float64
        self.work = (_workspace(op).get(
            "eigen_gradients_work",
            (-(-pw * pw // 256), max(rows, 1), S + C * M), torch.float64, dev)
                     if self.want_weights else None)

    def forward(self, lo, hi):
        """The far plane of the positions lo ... hi - 1 in the chunk's own
        buffer."""
        return _one_slice_far(self.op, self.psi, self.probe, self.scan,
                              self.eigen, self.weights, lo, hi, self.far_all)

    def run(self, lo, hi, far, table, spare=None):
        """The chain behind `far` (n, 1, S, det, det), which it may overwrite,
        with table (n // fly, det, det) = dL/dI of the chunk's frames.  spare:
        a buffer of far's shape for the scaled inverse to write to (resident
        callers)."""
        op, fly, st = self.op, self.fly, A.stream_ptr()
        psi, probe = self.psi, self.probe
        n, S = hi - lo, probe.shape[2]
        pw, det = op.probe_shape, op.detector_shape
        H, W = psi.shape[-2:]
        sc = self.scan[lo:hi]
        if self.scaled_inverse:
            mid = spare if self.mid_all is None else self.mid_all[:n]
        else:
            mid = far
        chi = mid if self.chi_all is None else self.chi_all[:n]
        if self.scaled_inverse:
            # S * fly planes share a frame's table
            check(
                lib.tike_ifft2_crop_scaled(A.ptr(far), A.ptr(table), S * fly,
                                           A.ptr(mid), A.ptr(chi), n * S, det,
                                           pw, self.scale, st),
                "intensity backward (scaled ifft2 + crop)")
        else:
            check(
                lib.tike_farplane_scale(A.ptr(far), A.ptr(table), n // fly,
                                        S * fly, det * det, 2.0, st),
                "intensity backward (upstream gradient)")
            check(
                lib.tike_ifft2_crop(A.ptr(far), A.ptr(mid), A.ptr(chi), n * S,
                                    det, pw, 0.5 * self.scale, st),
                "intensity backward (ifft2 + crop)")
        objproj = self.objproj_all[:n] if self.need_proj else None
        if self.weights is None:
            check(
                lib.tike_lstsq_gradients(A.ptr(chi), A.ptr(sc), A.ptr(psi),
                                         A.ptr(probe), None, None, 0, 0, None,
                                         None, A.ptr(self.gprobe),
                                         A.ptr(objproj), n, S, pw, H, W, st),
                "intensity backward (probe gradient + object projection)")
        else:
            eigen = self.eigen
            C, M = eigen.shape[1:3] if eigen is not None else (0, 0)
            check(
                lib.tike_eigen_probe_gradients(
                    A.ptr(chi), A.ptr(sc), A.ptr(psi), A.ptr(probe),
                    A.ptr(eigen), A.ptr(self.weights[lo:hi]), C, M,
                    A.ptr(self.gprobe), A.ptr(self.geigen),
                    A.ptr(self.gweights[lo:hi]) if self.want_weights else None,
                    A.ptr(objproj), A.ptr(self.work), n, S, pw, H, W, st),
                "intensity backward (probe, eigen probe and weight gradients "
                "+ object projection)")
        if self.want_psi:
            check(
                lib.tike_scatter_patches(A.ptr(objproj), A.ptr(sc),
                                         A.ptr(self.acc), n, pw, H, W, st),
                "intensity backward (object gradient)")
        if self.want_scan:
            check(
                lib.tike_scan_gradient(A.ptr(objproj), A.ptr(sc), A.ptr(psi),
                                       A.ptr(self.gscan[lo:hi]), n, pw, H, W,
                                       st),
                "intensity backward (scan gradient)")

    def result(self):
        """(psi, probe, scan, eigen_probe, eigen_weights) gradients, None
        where not wanted."""
        gpsi = (torch.complex(self.acc[0], self.acc[1])[None]
                if self.want_psi else None)
        return gpsi, self.gprobe, self.gscan, self.geigen, self.gweights


def _backward_chunks(op, fly, psi, probe, scan, want, table_of, eigen=None,
                     weights=None):
    """The backward of the one-slice forms: per chunk of whole frames the
    recomputed forward, the upstream table of the chunk -- table_of(lo, hi,
    far), frames lo // fly ... hi // fly - 1 -- and the chain of `_Back`."""
    N = scan.shape[0]
    chunk = _chunk_rows(op, probe, fly)
    back = _Back(op, fly, psi, probe, scan, want, min(chunk, N), eigen,
                 weights)
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        far = back.forward(lo, hi)
        back.run(lo, hi, far, table_of(lo, hi, far))
    return back.result()


def _one_slice_forward(ctx, operator, fly, psi, probe, scan, eigen_probe=None,
                       eigen_weights=None):
    """The forward of `_Intensity` and `_EigenIntensity`: (the inputs that are
    not None, detached and contiguous, saved for backward in the order psi,
    probe, scan, eigen_weights, eigen_probe; the intensity)."""
    from .ptycho.ptycho import _intensity_chunks
    psi, probe, scan, eigen_weights, eigen_probe = (
        None if x is None else x.detach().contiguous()
        for x in (psi, probe, scan, eigen_weights, eigen_probe))
    saved = tuple(x for x in (psi, probe, scan, eigen_weights, eigen_probe)
                  if x is not None)
    ctx.operator, ctx.fly = operator, fly
    ctx.save_for_backward(*saved)
    A.current_device()  # (hands the library its deterministic-mode scratch)
    det = operator.detector_shape
    if scan.shape[0] == 0:
        return saved, torch.empty((0, det, det), dtype=torch.float32,
                                  device=psi.device)
    # chunked; the far plane of a chunk dies with the chunk
    frames = [inten for _, _, inten in _intensity_chunks(
        operator, psi, scan, probe, eigen_probe, eigen_weights, fly=fly)]
    return saved, frames[0] if len(frames) == 1 else torch.cat(frames)


class _Intensity(torch.autograd.Function):

    @staticmethod
    def forward(ctx, psi, probe, scan, operator, fly):
        saved, inten = _one_slice_forward(ctx, operator, fly, psi, probe, scan)
        ctx.save_for_forward(*saved)
        return inten

    @staticmethod
    def jvp(ctx, d_psi, d_probe, d_scan, _operator, _fly):
        """The tangent of the intensity under `torch.autograd.forward_ad`.
        torch hands an input that is no dual tensor a tangent of zeros, not
        None (None only when materialising is off), and `forward` cannot see
        which inputs are dual.  Its terms add exact zeros -- the bits of a
        None tangent -- but the gather then reads all three tangents: with
        scan alone dual, `tike_conv_fwd_tangent` takes about a quarter longer
        than under `intensity_jvp(d_scan=...)` (profiles/autograd_jvp.md)."""
        psi, probe, scan = ctx.saved_tensors
        tangents = [None if t is None else t.detach().contiguous()
                    for t in (d_psi, d_probe, d_scan)]
        return _jvp_chunks(ctx.operator, (psi, probe, scan, None, None),
                           tangents + [None, None], ctx.fly, primal=False)[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        psi, probe, scan = ctx.saved_tensors
        fly = ctx.fly
        g = g.to(torch.float32).contiguous()
        want = tuple(ctx.needs_input_grad[:3]) + (False, False)
        grads = _backward_chunks(
            ctx.operator, fly, psi, probe, scan, want,
            lambda lo, hi, far: g[lo // fly:hi // fly])
        return grads[0], grads[1], grads[2], None, None


class _EigenIntensity(torch.autograd.Function):
    """`_Intensity` with the varying probe of eigen_probe (or None: C = 0) and
    eigen_weights; the backward swaps tike_lstsq_gradients for
    tike_eigen_probe_gradients."""

    @staticmethod
    def forward(ctx, psi, probe, scan, eigen_probe, eigen_weights, operator,
                fly):
        ctx.eigen = eigen_probe is not None
        return _one_slice_forward(ctx, operator, fly, psi, probe, scan,
                                  eigen_probe, eigen_weights)[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        psi, probe, scan, weights = ctx.saved_tensors[:4]
        eigen = ctx.saved_tensors[4] if ctx.eigen else None
        fly = ctx.fly
        g = g.to(torch.float32).contiguous()
        grads = _backward_chunks(
            ctx.operator, fly, psi, probe, scan,
            tuple(ctx.needs_input_grad[:5]),
            lambda lo, hi, far: g[lo // fly:hi // fly], eigen, weights)
        return grads + (None, None)


def intensity(operator, psi, probe, scan, *, eigen_probe=None,
              eigen_weights=None, fly=1, check_positions=True):
    """Diffraction intensities (N // fly, det, det) float32 of an entered
    `tike_amd.operators.Ptycho`, differentiable with respect to whichever of
    psi (1, H, W) complex64, probe (1, 1, S, pw, pw) complex64, scan (N, 2)
    float32, eigen_probe (1, C, M, pw, pw) complex64 and eigen_weights
    (N, C + 1, S) float32 -- device tensors -- requires a gradient.  Frame f
    is the sum over the positions f * fly ... f * fly + fly - 1 and over the
    modes: the values of ``operator._compute_intensity(..., fly=fly)``; the
    operator's `norm` is honoured.  Once differentiable.  Without
    eigen_weights it also has a forward-mode rule: on
    `torch.autograd.forward_ad` dual tensors (any of psi, probe, scan) the
    result is a dual with the tangent of `intensity_jvp` (torch gives the
    inputs that are not dual a tangent of zeros, so all three tangents are
    gathered: where only some inputs vary, `intensity_jvp` with the others
    left None is the faster call).  The eigen-probe
    form below and `multislice_intensity` have none: under `forward_ad` they
    raise torch's "you must implement the jvp function" (their forward mode
    is a function each: `eigen_intensity_jvp`, `multislice_intensity_jvp`).

    With eigen_weights the probe varies from position to position (not from
    frame to frame: any `fly`), as `get_varying_probe` has it: position n sees
    w[n, 0, s] probe[s] + sum_c w[n, c + 1, s] eigen_probe[c, s] in the first
    M <= S modes and w[n, 0, s] probe[s] in the others.  eigen_probe=None with
    eigen_weights (N, 1, S) is C = 0: an intensity scale per position and
    mode.  Without eigen_weights the call launches what it always launched.

    Raises NotImplementedError for several slices or a probe TENSOR per
    position, TypeError for host arrays or other dtypes, ValueError when N is
    no multiple of `fly`, for more than `MAX_MODES` modes, for eigen_probe
    without eigen_weights, for eigen shapes that do not fit probe and scan,
    for more than `MAX_EIGEN_PLANES` eigen planes C * M and -- with
    check_positions, the default -- for positions that
    `check_allowed_positions` refuses: the object gradient's scatter drops
    what falls outside the object.  check_positions costs a read-back of the
    positions per call.
    """
    fly = _checked(operator, psi, probe, scan, fly, check_positions,
                   eigen_probe=eigen_probe, eigen_weights=eigen_weights)
    if eigen_weights is None:
        return _Intensity.apply(psi, probe, scan, operator, fly)
    return _EigenIntensity.apply(psi, probe, scan, eigen_probe, eigen_weights,
                                 operator, fly)


# -------------------------------------------------------------- forward mode
def _tangent_sink(inten, tangent, fly, what):
    """What the forward-mode chunk loops do with a chunk's far plane and its
    tangent unless told otherwise: tike_intensity_tangent into the frames'
    rows of `tangent` (and of `inten` unless None)."""

    def sink(lo, hi, far, dfar):
        # the S * fly planes of a frame are adjacent
        P = far.shape[-3] * fly
        check(
            lib.tike_intensity_tangent(
                A.ptr(far), A.ptr(dfar),
                None if inten is None else A.ptr(inten[lo // fly:]),
                A.ptr(tangent[lo // fly:]), (hi - lo) // fly, P,
                far.shape[-1] * far.shape[-2], A.stream_ptr()),
            f"{what} (tangent intensity)")

    return sink


def _jvp_outputs(op, psi, scan, fly, primal, sink):
    """(I or None, dI) to fill, or (None, None) where a sink takes the far
    planes."""
    if sink is not None:
        return None, None
    det, frames = op.detector_shape, scan.shape[0] // fly
    return (torch.empty((frames, det, det), dtype=torch.float32,
                        device=psi.device) if primal else None,
            torch.empty((frames, det, det), dtype=torch.float32,
                        device=psi.device))


def _jvp_chunks(op, primals, tangents, fly, primal=True, sink=None):
    """(I or None, dI): the forward-mode chunk loop of the one-slice forms
    (`intensity_jvp`, `_Intensity.jvp`, `eigen_intensity_jvp`) on contiguous
    device tensors: primals (psi, probe, scan, eigen, weights) and their five
    tangents, at least one of which is not None.  weights None: the plain
    form, tike_conv_fwd_tangent; otherwise (eigen, d_eigen: None for C = 0)
    tike_eigen_wave_tangent.  sink(lo, hi, far, dfar): called per chunk in the
    place of tike_intensity_tangent (`cost_jvp`, `cost_gauss_newton_product`;
    both far planes are its to overwrite); then (None, None) is returned and
    no frame-sized tensor exists."""
    psi, probe, scan, eigen, weights = primals
    d_psi, d_probe, d_scan, d_eigen, d_weights = tangents
    # (the form's public function, for `check`)
    what = "intensity_jvp" if weights is None else "eigen_intensity_jvp"
    N, S = scan.shape[0], probe.shape[2]
    pw, det = op.probe_shape, op.detector_shape
    H, W = psi.shape[-2:]
    A.current_device()  # (hands the library its deterministic-mode scratch)
    st = A.stream_ptr()
    inten, tangent = _jvp_outputs(op, psi, scan, fly, primal, sink)
    if N == 0:
        return inten, tangent
    if sink is None:
        sink = _tangent_sink(inten, tangent, fly, what)
    # the far plane and its tangent are both resident; whole frames
    chunk = _chunk_rows(op, probe, fly, halve=True)
    far_all = torch.empty((min(chunk, N), 1, S, det, det),
                          dtype=torch.complex64, device=psi.device)
    dfar_all = torch.empty_like(far_all)
    fwd_scale = fft_scales(det, op.norm)[0]
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        n = hi - lo
        sc = scan[lo:hi]
        dsc = None if d_scan is None else A.ptr(d_scan[lo:hi])
        far = _one_slice_far(op, psi, probe, scan, eigen, weights, lo, hi,
                             far_all)
        dfar = dfar_all[:n]
        if weights is None:
            check(
                lib.tike_conv_fwd_tangent(
                    A.ptr(psi), A.ptr(d_psi), A.ptr(sc), dsc, A.ptr(probe),
                    A.ptr(d_probe), A.ptr(dfar), n, S, pw, det, H, W, st),
                f"{what} (tangent exit waves)")
        else:
            C, M = (0, 0) if eigen is None else eigen.shape[1:3]
            check(
                lib.tike_eigen_wave_tangent(
                    A.ptr(psi), A.ptr(d_psi), A.ptr(sc), dsc, A.ptr(probe),
                    A.ptr(d_probe), A.ptr(eigen), A.ptr(d_eigen),
                    A.ptr(weights[lo:hi]),
                    None if d_weights is None else A.ptr(d_weights[lo:hi]), C,
                    M, A.ptr(dfar), n, S, pw, det, H, W, st),
                f"{what} (tangent exit waves)")
        check(lib.tike_fft2(A.ptr(dfar), A.ptr(dfar), n * S, det, 0,
                            fwd_scale, st), f"{what} (tangent far plane)")
        sink(lo, hi, far, dfar)
    return inten, tangent


def _jvp_loop(op, primals, tangents, fly, primal=True, sink=None):
    """The forward-mode chunk loop of the form that the primals (psi, probe,
    scan, eigen, weights) have: several slices or one."""
    if primals[0].shape[0] > 1:
        return _multislice_jvp_chunks(op, *primals[:3], *tangents[:3], fly,
                                      primal, sink)
    return _jvp_chunks(op, primals, tangents, fly, primal, sink)


def _apply(primals, operator, fly):
    """The `Function` of the form that the primals (psi, probe, scan, eigen,
    weights) have."""
    if primals[4] is not None:
        return _EigenIntensity.apply(*primals, operator, fly)
    function = _MultisliceIntensity if primals[0].shape[0] > 1 else _Intensity
    return function.apply(*primals[:3], operator, fly)


def _checked_tangents(name, given):
    """A tangent matches its primal in type, dtype, shape and device: {what:
    the tangent detached and contiguous} for the (what, primal, tangent) of
    `given` whose tangent is not None."""
    out = {}
    for what, x, t in given:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor):
            raise TypeError(
                f"{name}: d_{what} must be a torch device tensor, not "
                f"{type(t).__name__}")
        if t.dtype != x.dtype:
            raise TypeError(
                f"{name}: d_{what} must be {x.dtype} as {what} is, not "
                f"{t.dtype}")
        if t.shape != x.shape:
            raise ValueError(
                f"{name}: d_{what} must have the shape of {what}, "
                f"{tuple(x.shape)}, not {tuple(t.shape)}")
        if t.device != x.device:
            raise ValueError(
                f"{name}: d_{what} lives on {t.device}, {what} on {x.device}")
        out[what] = t.detach().contiguous()
    return out


def _checked_jvp(name, operator, primals, tangents, fly, check_positions,
                 slices=False, eigen=False):
    """Every refusal of the forward-mode entries that needs no device, the
    tangents' among them, before `_checked` asks for device tensors: (fly, the
    five tangents).  primals: (psi, probe, scan, eigen_probe, eigen_weights);
    eigen: the eigen form, which must have eigen_weights; the other forms
    look at the first three of either."""
    psi, probe, scan, eigen_probe, eigen_weights = primals
    given = list(zip(_EIGEN_WRT, primals, tangents))
    if not eigen:
        given, eigen_probe, eigen_weights = given[:3], None, None
    elif eigen_probe is None:
        if tangents[3] is not None:
            raise ValueError(
                f"{name}: d_eigen_probe without eigen_probe (there is no "
                "eigen probe it could be the tangent of)")
        del given[3]
    checked = None
    if all(isinstance(x, torch.Tensor) for _, x, _ in given):
        # (host arrays: `_checked` below names them)
        checked = _checked_tangents(name, given)
    if eigen and eigen_weights is None:
        raise TypeError(
            f"{name}: eigen_weights is required (without them `intensity_jvp` "
            "is the forward mode of the model)")
    fly = _checked(operator, psi, probe, scan, fly, check_positions, name=name,
                   slices=slices, eigen_probe=eigen_probe,
                   eigen_weights=eigen_weights)
    return fly, [checked.get(k) for k in _EIGEN_WRT]


def _jvp(name, operator, primals, tangents, fly, check_positions, **form):
    """The body of the three `*_jvp` functions on (psi, probe, scan,
    eigen_probe, eigen_weights) and their tangents; form: `slices` or `eigen`
    of `_checked_jvp`."""
    fly, tangents = _checked_jvp(name, operator, primals, tangents, fly,
                                 check_positions, **form)
    primals = [None if x is None else x.detach().contiguous()
               for x in primals]
    if all(t is None for t in tangents):
        with torch.no_grad():
            inten = _apply(primals, operator, fly)
        return inten, torch.zeros_like(inten)
    return _jvp_loop(operator, primals, tangents, fly)


def _gauss_newton(name, names, operator, primals, tangents, weight, fly, wrt,
                  check_positions, **form):
    """The body of the three `*_gauss_newton_product` functions: the
    forward-mode loop of the form without the primal intensity, then its
    `Function` with weight * dI upstream.  names: the inputs of the form;
    form: as in `_jvp`."""
    wrt = _checked_product(name, operator, primals, weight, fly, wrt, names)
    fly, tangents = _checked_jvp(name, operator, primals, tangents, fly,
                                 check_positions, **form)
    leaves = [None if x is None else
              x.detach().contiguous().requires_grad_(k in wrt)
              for k, x in zip(_EIGEN_WRT, primals)]
    by_name = dict(zip(_EIGEN_WRT, leaves))
    if all(t is None for t in tangents):
        return tuple(torch.zeros_like(by_name[k]) for k in wrt)
    tangent = _jvp_loop(operator,
                        [None if x is None else x.detach() for x in leaves],
                        tangents, fly, primal=False)[1]
    if weight is not None:
        tangent = tangent * weight.detach()
    with torch.enable_grad():
        inten = _apply(leaves, operator, fly)
        return torch.autograd.grad(inten, [by_name[k] for k in wrt],
                                   grad_outputs=tangent)


def intensity_jvp(operator, psi, probe, scan, *, d_psi=None, d_probe=None,
                  d_scan=None, fly=1, check_positions=True):
    """(I, dI): the intensities of `intensity(operator, psi, probe, scan,
    fly=fly)` -- the same bits -- and their directional derivative J v along
    the tangents d_psi (1, H, W) complex64, d_probe (1, 1, S, pw, pw)
    complex64 and d_scan (N, 2) float32, each None (zero) or a device tensor
    of its primal's shape, dtype and device.  Both (N // fly, det, det)
    float32, outside any autograd graph.  The derivative with respect to the
    positions is that of `scan.grad`: the integer part of a position is held
    fixed.  One slice and the shared probe only: eigen probes are no parameter
    of this function, and several slices are `multislice_intensity_jvp`'s.
    With no tangent dI is zeros and only the primal launches.

    Raises what `intensity` raises (NotImplementedError for several slices or
    a probe per position, TypeError, ValueError), and TypeError / ValueError
    for a tangent that does not match its primal, before any launch.
    """
    return _jvp("intensity_jvp", operator, (psi, probe, scan, None, None),
                (d_psi, d_probe, d_scan, None, None), fly, check_positions)


_WRT = ("psi", "probe", "scan")


def _frames(scan, fly):
    """N // fly, or None where `_checked` is about to refuse scan or fly."""
    try:
        fly = int(fly)
    except (TypeError, ValueError):
        return None
    if (not isinstance(scan, torch.Tensor) or scan.ndim != 2 or fly < 1
            or scan.shape[0] % fly):
        return None
    return scan.shape[0] // fly


def gauss_newton_product(operator, psi, probe, scan, *, d_psi=None,
                         d_probe=None, d_scan=None, weight=None, fly=1,
                         wrt=_WRT, check_positions=True):
    """J^T (weight * J v): the Gauss-Newton (weight=None) or Fisher (weight =
    1 / I for Poisson counts) matrix of the intensity model applied to the
    tangents v = (d_psi, d_probe, d_scan) of `intensity_jvp`.  Returns a tuple
    with one tensor per name in `wrt` (any of "psi", "probe", "scan", in that
    order of `wrt`), each in the `.grad` convention of `intensity` (a complex
    input's part is d/dRe + i d/dIm).  weight: (N // fly, det, det) float32
    device tensor or None.

    Composed of `intensity_jvp` and the backward of `intensity` with
    weight * dI for the upstream gradient -- one forward more than a fused
    chain would take; only what `wrt` names is launched in the backward.

    Raises what `intensity_jvp` raises, ValueError for names in `wrt` other
    than the three (or none, or one twice), TypeError / ValueError for a
    weight of another type, dtype, shape or device.
    """
    return _gauss_newton("gauss_newton_product", _WRT, operator,
                         (psi, probe, scan, None, None),
                         (d_psi, d_probe, d_scan, None, None), weight, fly,
                         wrt, check_positions)


def _checked_frame_tensor(name, what, x, operator, psi, scan, fly, planes):
    """The refusals of a float32 tensor with a row per frame: `weight`
    (N // fly, det, det) with planes, `upstream` (N // fly,) without."""
    if not isinstance(x, torch.Tensor):
        raise TypeError(
            f"{name}: {what} must be a torch device tensor, not "
            f"{type(x).__name__}")
    if x.dtype != torch.float32:
        raise TypeError(
            f"{name}: {what} must be torch.float32, not {x.dtype}")
    frames = _frames(scan, fly)
    det = operator.detector_shape
    shape = (frames,) + ((det, det) if planes else ())
    if frames is not None and tuple(x.shape) != shape:
        raise ValueError(
            f"{name}: {what} must be "
            f"{'(N // fly, det, det)' if planes else '(N // fly,)'} = "
            f"{shape}, not {tuple(x.shape)}")
    if isinstance(psi, torch.Tensor) and x.device != psi.device:
        raise ValueError(
            f"{name}: {what} lives on {x.device}, psi on {psi.device}")


def _checked_product(name, operator, primals, weight, fly, wrt, names):
    """The `wrt` and `weight` refusals of the Gauss-Newton products; wrt as a
    tuple.  primals: (psi, probe, scan, eigen_probe, eigen_weights); names:
    what `wrt` may name."""
    wrt = tuple(wrt)
    if not wrt or len(set(wrt)) != len(wrt) or any(w not in names
                                                   for w in wrt):
        raise ValueError(
            f"{name}: wrt must name some of {names}, each once; got {wrt}")
    if weight is not None:
        _checked_frame_tensor(name, "weight", weight, operator, primals[0],
                              primals[2], fly, planes=True)
    if "eigen_probe" in wrt and primals[3] is None:
        raise ValueError(
            f'{name}: "eigen_probe" in wrt with eigen_probe=None (there is no '
            "eigen probe to differentiate with respect to)")
    return wrt


# ------------------------------------------------------------ several slices
PASS1_TAKES_TABLE = True
"""Fused route: the upstream gradient is applied by `tike_ifft2_pass1_scaled`
while inverse pass 1 loads the far plane (its hand-off is that of
`tike_fft2_pass1(inverse)`: the same pass-1 engine behind another load).
False: `tike_farplane_scale` + `tike_fft2_pass1`, two launches and one more
trip of the far plane through memory; the tests compare the two."""


def _cgrad():
    """cgrad's MODULE, whose levers `MULTISLICE_FUSED` and
    `MULTISLICE_STEP_BACK_FUSED` choose the route.  Through `importlib`
    because the solvers package exports the solver FUNCTION under the
    module's name (`from .ptycho.solvers import cgrad` is the function), and
    looked up where a lever is read, not once at import: tests and tools set
    the levers on the module between calls."""
    return importlib.import_module(__package__ + ".ptycho.solvers.cgrad")


class _SlicesForward:
    """The forward of `multislice_intensity` chunk by chunk, for its four
    users (the forward, the backward, the forward mode, the cost): the route,
    the chunk of whole frames (`extra`: sets of (S, det, det) per position a
    user holds besides; sized as `cgrad` sizes its multislice chunks), on the
    fused route the workspace buffers, and per chunk the far plane and the
    beams -- all from `ptycho/solvers/_multislice.py`, which cgrad walks too.
    Iterating yields (lo, hi, far (n, S, det, det), beams) with beams[d]
    (n, S, pw, pw) the beam incident on slice d >= 1.  On the general route
    far and beams are fresh tensors that the iteration does not hold on to:
    they live as long as the caller keeps them."""

    def __init__(self, op, fly, psi, probe, scan, extra=0):
        self.op, self.psi, self.probe, self.scan = op, psi, probe, scan
        D, S = psi.shape[0], probe.shape[2]
        self.fused = _multislice.fused_route(op, probe,
                                             _cgrad().MULTISLICE_FUSED)
        # fused route: far + mid + D - 1 sets of incident probes + the D
        # objproj planes (D / S of a set, rounded up) + `extra` sets
        chunk = _multislice.chunk_positions(
            op, psi.device, S, D + 1 + -(-D // S) + extra, self.fused)
        self.chunk = max(1, chunk // fly) * fly
        self.nmax = min(self.chunk, scan.shape[0])
        if self.fused:
            self.far_all, mid, self.beams_all, self.objproj = (
                _multislice.fused_buffers(op, psi.device, D, S,
                                          max(self.nmax, 1), nproj=D))
            self.mid = mid[0]

    def tangent(self):
        """(nmax, S, det, det) for the forward mode's tangent: of the
        workspace on the fused route."""
        from .ptycho.solvers.lstsq import _workspace
        S, det = self.probe.shape[2], self.op.detector_shape
        if self.fused:
            return _workspace(self.op).get(
                "ms_tangent", (self.nmax, S, det, det), torch.complex64,
                self.psi.device)
        return torch.empty((self.nmax, S, det, det), dtype=torch.complex64,
                           device=self.psi.device)

    def __iter__(self):
        op, psi, probe, N = self.op, self.psi, self.probe, self.scan.shape[0]
        for lo in range(0, N, self.chunk):
            hi = min(N, lo + self.chunk)
            sc = self.scan[lo:hi]
            if self.fused:
                far = _multislice.fused_far(op, psi, sc, probe, self.far_all,
                                            self.beams_all,
                                            "multislice_intensity")
                yield lo, hi, far, [probe[0]] + [
                    b[:hi - lo] for b in self.beams_all[:psi.shape[0] - 1]]
            else:
                yield (lo, hi) + _multislice.general_far(op, psi, sc, probe)


def _fused_back(op, psi, sc, probe, far, beams, table, fly, mid, objproj, want,
                acc, gprobe):
    """One chunk of the backward on the two-pass kernels behind the far plane
    and the incident beams of `_SlicesForward`: the upstream gradient `table`
    applied with pass 1 of F^H, then the walk back that cgrad takes
    (`_multislice.fused_step_back`).  Leaves objproj_d in objproj[d, :n] when
    the object or the positions want it."""
    want_psi, want_probe, want_scan = want
    n, S, det = sc.shape[0], probe.shape[-3], op.detector_shape
    st = A.stream_ptr()
    fwd_scale, inv_scale = fft_scales(det, op.norm)
    mid = mid[:n]
    if PASS1_TAKES_TABLE:
        # S * fly planes share a frame's table
        check(
            lib.tike_ifft2_pass1_scaled(A.ptr(far), A.ptr(table), None, None,
                                        S * fly, A.ptr(mid), n * S, det, st),
            "multislice_intensity backward (upstream gradient + inverse "
            "pass 1)")
    else:
        check(
            lib.tike_farplane_scale(A.ptr(far), A.ptr(table), n // fly,
                                    S * fly, det * det, 1.0, st),
            "multislice_intensity backward (upstream gradient)")
        check(lib.tike_fft2_pass1(A.ptr(far), A.ptr(mid), n * S, det, 1, st),
              "multislice_intensity backward (inverse pass 1)")
    # the pass 2 behind it finishes F^H: the FORWARD scale, and the 2 of G
    _multislice.fused_step_back(
        op, psi, sc, probe, far, mid, beams[1:], objproj[:, :n], acc, gprobe,
        first_scale=2.0 * fwd_scale, scale=inv_scale,
        want_proj=want_psi or want_scan,
        one_launch=_cgrad().MULTISLICE_STEP_BACK_FUSED,
        label="multislice_intensity backward")


def _general_back(op, psi, sc, probe, far, beams, table, fly, objproj, want,
                  acc, gprobe):
    """One chunk of the backward through the general operators behind the far
    plane and the incident beams of `_SlicesForward`, as cgrad's
    `_multislice_chunk_general` walks back; table: the upstream table of the
    chunk's frames; objproj (D, nmax, pw, pw) or None."""
    want_psi, want_probe, want_scan = want
    D, (H, W) = psi.shape[0], psi.shape[-2:]
    n, S, det = sc.shape[0], probe.shape[-3], op.detector_shape
    conv, fresnel = op.diffraction.diffraction, op.diffraction.propagation
    need_proj = want_psi or want_scan
    st = A.stream_ptr()
    check(
        lib.tike_farplane_scale(A.ptr(far), A.ptr(table), n // fly, S * fly,
                                det * det, 2.0, st),
        "multislice_intensity backward (upstream gradient)")
    # F^H: the unscaled inverse x the FORWARD scale, in place
    check(
        lib.tike_fft2(A.ptr(far), A.ptr(far), n * S, det, 1,
                      fft_scales(det, op.norm)[0], st),
        "multislice_intensity backward (F^H)")
    wave = far
    for d in range(D - 1, 0, -1):
        if need_proj:
            # the incident probes as the varying probe of all S modes: every
            # mode is read from `unique_probe`, the other probe operands are
            # placeholders that are never dereferenced for a mode below S
            check(
                lib.tike_lstsq_gradients(
                    A.ptr(wave), A.ptr(sc), A.ptr(psi[d]), A.ptr(beams[d]),
                    A.ptr(beams[d]), A.ptr(sc), 0, S, A.ptr(beams[d]), None,
                    None, A.ptr(objproj[d, :n]), n, S, det, H, W, st),
                "multislice_intensity backward (object projection of a "
                "slice)")
        if want_psi:
            check(
                lib.tike_scatter_patches(A.ptr(objproj[d, :n]), A.ptr(sc),
                                         A.ptr(acc[d]), n, det, H, W, st),
                "multislice_intensity backward (object gradient of a slice)")
        wave = fresnel.adj(conv.adj_probe(nearplane=wave, scan=sc, psi=psi[d]),
                           overwrite=True)
    check(
        lib.tike_lstsq_gradients(A.ptr(wave), A.ptr(sc), A.ptr(psi[0]),
                                 A.ptr(probe), None, None, 0, 0, None, None,
                                 A.ptr(gprobe),
                                 A.ptr(objproj[0, :n]) if need_proj else None,
                                 n, S, det, H, W, st),
        "multislice_intensity backward (first slice: both products)")
    if want_psi:
        check(
            lib.tike_scatter_patches(A.ptr(objproj[0, :n]), A.ptr(sc),
                                     A.ptr(acc[0]), n, det, H, W, st),
            "multislice_intensity backward (object gradient of the first "
            "slice)")


class _MultisliceIntensity(torch.autograd.Function):

    @staticmethod
    def forward(ctx, psi, probe, scan, operator, fly):
        psi, probe, scan = (x.detach().contiguous() for x in (psi, probe, scan))
        ctx.operator, ctx.fly = operator, fly
        ctx.save_for_backward(psi, probe, scan)
        A.current_device()  # (hands the library its deterministic-mode scratch)
        op = operator
        N, S, det = scan.shape[0], probe.shape[2], op.detector_shape
        inten = torch.empty((N // fly, det, det), dtype=torch.float32,
                            device=psi.device)
        if N == 0:
            return inten
        for lo, hi, far, beams in _SlicesForward(op, fly, psi, probe, scan):
            del beams  # (general route: only the far plane is kept)
            # the S * fly planes of a frame are adjacent
            check(
                lib.tike_intensity(A.ptr(far), A.ptr(inten[lo // fly:]),
                                   (hi - lo) // fly, S * fly, det * det,
                                   A.stream_ptr()),
                "multislice_intensity")
        return inten

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        psi, probe, scan = ctx.saved_tensors
        fly = ctx.fly
        g = g.to(torch.float32).contiguous()
        grads = _multislice_backward_chunks(
            ctx.operator, fly, psi, probe, scan,
            tuple(ctx.needs_input_grad[:3]),
            lambda lo, hi, far: g[lo // fly:hi // fly])
        return grads + (None, None)


def _multislice_backward_chunks(op, fly, psi, probe, scan, want, table_of):
    """The backward of `multislice_intensity`, shared with the backward of
    `cost`: per chunk of whole frames `_fused_back` or `_general_back` with
    the upstream table table_of(lo, hi, far) of the chunk's frames, then the
    scan gradient over the D objproj planes.  (psi, probe, scan) gradients."""
    want_psi, want_probe, want_scan = want
    D, (H, W) = psi.shape[0], psi.shape[-2:]
    pw = op.probe_shape
    dev = psi.device
    acc = (torch.zeros((D, 2, H, W), dtype=torch.float32, device=dev)
           if want_psi else None)
    gprobe = torch.zeros_like(probe) if want_probe else None
    gscan = torch.empty_like(scan) if want_scan else None
    forward = _SlicesForward(op, fly, psi, probe, scan)
    nmax = forward.nmax
    if forward.fused:
        objproj = forward.objproj
    else:
        objproj = (torch.empty((D, nmax, pw, pw), dtype=torch.complex64,
                               device=dev)
                   if want_psi or want_scan else None)
    for lo, hi, far, beams in forward:
        sc = scan[lo:hi]
        table = table_of(lo, hi, far)
        if forward.fused:
            _fused_back(op, psi, sc, probe, far, beams, table, fly,
                        forward.mid, objproj, want, acc, gprobe)
        else:
            _general_back(op, psi, sc, probe, far, beams, table, fly, objproj,
                          want, acc, gprobe)
        # (general route: fresh tensors, gone before the next chunk's are made)
        del far, beams
        if want_scan:
            check(
                lib.tike_scan_gradient_slices(
                    A.ptr(objproj), nmax * pw * pw, A.ptr(sc), A.ptr(psi),
                    A.ptr(gscan[lo:hi]), hi - lo, D, pw, H, W,
                    A.stream_ptr()),
                "multislice_intensity backward (scan gradient)")
    gpsi = torch.complex(acc[:, 0], acc[:, 1]) if want_psi else None
    return gpsi, gprobe, gscan


def multislice_intensity(operator, psi, probe, scan, *, fly=1,
                         check_positions=True):
    """`intensity` for an object of D >= 1 slices: the diffraction intensities
    (N // fly, det, det) float32 behind the last slice of psi (D, H, W)
    complex64 -- e_d = patch_n(psi[d]) x beam_d, beam_0 = the probe,
    beam_{d+1} = the operator's Fresnel step of e_d, far = F e_{D-1} -- summed
    over the modes and the `fly` positions of a frame, differentiable with
    respect to whichever of psi, probe (1, 1, S, pw, pw) complex64 and scan
    (N, 2) float32 -- device tensors -- requires a gradient.  psi.grad is
    (D, H, W): the exact gradient of every slice, not divided by D.  The
    operator is an entered `tike_amd.operators.Ptycho` with probe_shape ==
    detector_shape and its optics set (probe_wavelength, probe_FOV_lengths,
    multislice_propagation_distance); its `norm` is honoured.  One slice goes
    through `intensity` itself.  Once differentiable.

    Raises TypeError for host arrays or other dtypes, ValueError for other
    ranks or shapes, for several slices with probe_shape != detector_shape,
    when N is no multiple of `fly`, for more than `MAX_MODES` modes (more than
    8 at 128^2, 256^2 and 512^2 take the general route) and -- with
    check_positions -- for positions that `check_allowed_positions` refuses,
    NotImplementedError for a probe per position.
    """
    fly = _checked(operator, psi, probe, scan, fly, check_positions,
                   name="multislice_intensity", slices=True)
    if psi.shape[0] == 1:
        return _Intensity.apply(psi, probe, scan, operator, fly)
    return _MultisliceIntensity.apply(psi, probe, scan, operator, fly)


# --------------------------------------------- forward mode, several slices
TANGENT_FRESNEL_TWO_PASS = True
"""Fused route: the Fresnel step of the tangent between two slices by
`tike_fft2_pass1` -> `tike_fresnel_colpass` -> `tike_fft2_pass2_inplace` (the
scale of `_multislice.fused_far`, the `ms_mid` workspace for the hand-off)
instead of `tike_fresnel_spect_prop` in place: 0.68 - 0.77 of its time at 256^2 and 128^2
(profiles/autograd_multislice_jvp.md).  The general route has the one launch
only; the tests compare the two."""

FIRST_SLICE_BY_CONV_TANGENT = False
"""Slice 0 (shared probe, shared d_probe) by `tike_conv_fwd_tangent` at
det == pw instead of `tike_slice_wave_tangent`: the two are timed against each
other in profiles/autograd_multislice_jvp.md; the tests compare them."""


def _multislice_jvp_chunks(op, psi, probe, scan, d_psi, d_probe, d_scan, fly,
                           primal=True, sink=None):
    """(I or None, dI): the chunk loop of `multislice_intensity_jvp` for
    D > 1 slices on contiguous device tensors; at least one tangent is not
    None.  sink: as in `_jvp_chunks`."""
    D, (H, W) = psi.shape[0], psi.shape[-2:]
    N, S, det = scan.shape[0], probe.shape[2], op.detector_shape
    A.current_device()  # (hands the library its deterministic-mode scratch)
    st = A.stream_ptr()
    inten, tangent = _jvp_outputs(op, psi, scan, fly, primal, sink)
    if N == 0:
        return inten, tangent
    if sink is None:
        sink = _tangent_sink(inten, tangent, fly, "multislice_intensity_jvp")
    # one set more than the forward: the tangent (the general route keeps the
    # forward's chunk, which bounds a launch, not the memory)
    forward = _SlicesForward(op, fly, psi, probe, scan, extra=1)
    fused = forward.fused
    fresnel = op.diffraction.propagation
    fwd_scale, inv_scale = fft_scales(det, op.norm)
    dwave_all = forward.tangent()
    if fused:
        mid = forward.mid
        prop = fresnel._propagator((det, det), psi.device)
    for lo, hi, far, beams in forward:
        n = hi - lo
        sc = scan[lo:hi]
        dsc = None if d_scan is None else d_scan[lo:hi]
        dwave = dwave_all[:n]
        for d in range(D):
            dslice = None if d_psi is None else d_psi[d]
            if d == 0 and FIRST_SLICE_BY_CONV_TANGENT:
                check(
                    lib.tike_conv_fwd_tangent(
                        A.ptr(psi[0]), A.ptr(dslice), A.ptr(sc), A.ptr(dsc),
                        A.ptr(probe), A.ptr(d_probe), A.ptr(dwave), n, S, det,
                        det, H, W, st),
                    "multislice_intensity_jvp (tangent exit waves of the "
                    "first slice)")
                continue
            if d == 0:
                beam, per_scan = probe, 0
                dbeam, dper_scan = d_probe, 0
            else:
                if fused and TANGENT_FRESNEL_TWO_PASS:
                    check(lib.tike_fft2_pass1(A.ptr(dwave), A.ptr(mid), n * S,
                                              det, 0, st),
                          "multislice_intensity_jvp (Fresnel step of the "
                          "tangent: pass 1)")
                    check(
                        lib.tike_fresnel_colpass(A.ptr(mid), A.ptr(prop), 0,
                                                 A.ptr(dwave), n * S, det,
                                                 fwd_scale * inv_scale, st),
                        "multislice_intensity_jvp (Fresnel step of the "
                        "tangent: column passes)")
                    check(lib.tike_fft2_pass2_inplace(A.ptr(dwave), n * S, det,
                                                      1, 1.0, st),
                          "multislice_intensity_jvp (Fresnel step of the "
                          "tangent: pass 2)")
                else:
                    dwave = fresnel.fwd(dwave, overwrite=True)
                beam, per_scan, dbeam, dper_scan = beams[d], 1, dwave, 1
            # (de_d goes over dbeam_d where that is per position)
            check(
                lib.tike_slice_wave_tangent(
                    A.ptr(psi[d]), A.ptr(dslice), A.ptr(sc), A.ptr(dsc),
                    A.ptr(beam), per_scan, A.ptr(dbeam), dper_scan,
                    A.ptr(dwave), n, S, det, H, W, st),
                "multislice_intensity_jvp (tangent exit waves of a slice)")
        check(lib.tike_fft2(A.ptr(dwave), A.ptr(dwave), n * S, det, 0,
                            fwd_scale, st),
              "multislice_intensity_jvp (tangent far plane)")
        sink(lo, hi, far, dwave)
    return inten, tangent


def multislice_intensity_jvp(operator, psi, probe, scan, *, d_psi=None,
                             d_probe=None, d_scan=None, fly=1,
                             check_positions=True):
    """(I, dI): the intensities of `multislice_intensity(operator, psi, probe,
    scan, fly=fly)` -- the same bits -- and their directional derivative J v
    along the tangents d_psi (D, H, W) complex64, d_probe (1, 1, S, pw, pw)
    complex64 and d_scan (N, 2) float32, each None (zero) or a device tensor
    of its primal's shape, dtype and device.  Both (N // fly, det, det)
    float32, outside any autograd graph.  The operator is what
    `multislice_intensity` wants: entered, probe window = detector, its optics
    set.  The derivative with respect to the positions is that of `scan.grad`:
    the integer part of a position is held fixed and a tap outside the object
    counts as zero.  With no tangent dI is zeros and only the primal launches;
    one slice returns the bits of `intensity_jvp`.  This function is the
    forward mode of the model: `multislice_intensity` itself has no rule for
    `torch.autograd.forward_ad` dual tensors and keeps torch's refusal there.

    Raises what `multislice_intensity` raises (TypeError, ValueError,
    NotImplementedError for a probe per position), and TypeError / ValueError
    for a tangent that does not match its primal -- a (1, H, W) tangent of a
    (D, H, W) object among them --, before any launch.
    """
    return _jvp("multislice_intensity_jvp", operator,
                (psi, probe, scan, None, None),
                (d_psi, d_probe, d_scan, None, None), fly, check_positions,
                slices=True)


def multislice_gauss_newton_product(operator, psi, probe, scan, *, d_psi=None,
                                    d_probe=None, d_scan=None, weight=None,
                                    fly=1, wrt=_WRT, check_positions=True):
    """`gauss_newton_product` for `multislice_intensity`: J^T (weight * J v)
    for the tangents v = (d_psi (D, H, W), d_probe, d_scan) of
    `multislice_intensity_jvp`, one tensor per name in `wrt` (any of "psi",
    "probe", "scan", in that order of `wrt`) in the `.grad` convention of
    `multislice_intensity`: the object part is (D, H, W), every slice's exact
    part, not divided by D.  weight: (N // fly, det, det) float32 device tensor
    or None.

    Composed of the JVP with the primal intensity not written and the backward
    of `multislice_intensity` with weight * dI for the upstream gradient; only
    what `wrt` names is launched in the backward.  No dual tensors: see
    `multislice_intensity_jvp`.

    Raises what `multislice_intensity_jvp` raises, ValueError for names in
    `wrt` other than the three (or none, or one twice), TypeError / ValueError
    for a weight of another type, dtype, shape or device.
    """
    return _gauss_newton("multislice_gauss_newton_product", _WRT, operator,
                         (psi, probe, scan, None, None),
                         (d_psi, d_probe, d_scan, None, None), weight, fly,
                         wrt, check_positions, slices=True)


# ------------------------------------------------ forward mode, eigen probes
def eigen_intensity_jvp(operator, psi, probe, scan, *, eigen_probe=None,
                        eigen_weights, d_psi=None, d_probe=None, d_scan=None,
                        d_eigen_probe=None, d_eigen_weights=None, fly=1,
                        check_positions=True):
    """(I, dI): the intensities of `intensity(operator, psi, probe, scan,
    eigen_probe=eigen_probe, eigen_weights=eigen_weights, fly=fly)` -- the
    same bits -- and their directional derivative J v along the tangents
    d_psi (1, H, W) complex64, d_probe (1, 1, S, pw, pw) complex64, d_scan
    (N, 2) float32, d_eigen_probe (1, C, M, pw, pw) complex64 and
    d_eigen_weights (N, C + 1, S) float32, each None (zero) or a device tensor
    of its primal's shape, dtype and device.  Both (N // fly, det, det)
    float32, outside any autograd graph.  eigen_weights is required;
    eigen_probe=None with eigen_weights (N, 1, S) is C = 0.  Rows c + 1 of the
    weights and of their tangent count for nothing in the modes s >= M.  The
    derivative with respect to the positions is that of `scan.grad`: the
    integer part of a position is held fixed.  With no tangent dI is zeros and
    only the primal launches.  This function is the forward mode of the eigen
    form: `intensity(..., eigen_weights=)` itself has no rule for
    `torch.autograd.forward_ad` dual tensors and keeps torch's refusal there.

    Raises what `intensity` raises for the eigen form (NotImplementedError,
    TypeError, ValueError), TypeError without eigen_weights, ValueError for
    d_eigen_probe without eigen_probe, and TypeError / ValueError for a
    tangent that does not match its primal, before any launch.
    """
    return _jvp("eigen_intensity_jvp", operator,
                (psi, probe, scan, eigen_probe, eigen_weights),
                (d_psi, d_probe, d_scan, d_eigen_probe, d_eigen_weights), fly,
                check_positions, eigen=True)


_EIGEN_WRT = ("psi", "probe", "scan", "eigen_probe", "eigen_weights")


def eigen_gauss_newton_product(operator, psi, probe, scan, *, eigen_probe=None,
                               eigen_weights, d_psi=None, d_probe=None,
                               d_scan=None, d_eigen_probe=None,
                               d_eigen_weights=None, weight=None, fly=1,
                               wrt=_EIGEN_WRT, check_positions=True):
    """`gauss_newton_product` for the eigen form of `intensity`:
    J^T (weight * J v) for the tangents v of `eigen_intensity_jvp`, one tensor
    per name in `wrt` (any of "psi", "probe", "scan", "eigen_probe",
    "eigen_weights", in that order of `wrt`) in the `.grad` convention of
    `intensity` (a complex input's part is d/dRe + i d/dIm; the weights' part
    is exactly 0 in rows c + 1 of the modes s >= M).  weight: (N // fly, det,
    det) float32 device tensor or None.

    Composed of the JVP with the primal intensity not written and the backward
    of `intensity(..., eigen_probe=, eigen_weights=)` with weight * dI for the
    upstream gradient; only what `wrt` names is launched in the backward.  No
    dual tensors: see `eigen_intensity_jvp`.

    Raises what `eigen_intensity_jvp` raises, ValueError for names in `wrt`
    other than the five (or none, or one twice) or for "eigen_probe" in `wrt`
    with eigen_probe=None, TypeError / ValueError for a weight of another
    type, dtype, shape or device.
    """
    return _gauss_newton(
        "eigen_gauss_newton_product", _EIGEN_WRT, operator,
        (psi, probe, scan, eigen_probe, eigen_weights),
        (d_psi, d_probe, d_scan, d_eigen_probe, d_eigen_weights), weight, fly,
        wrt, check_positions, eigen=True)


# ------------------------------------------------- the noise-model cost
_MODELS = {"gaussian": 0, "poisson": 1}
"""The noise models of `Ptycho.cost` and their number in the C ABI."""

COST_FLOOR = 1e-9
"""The project's guard (`1e-9` in the factors of both models): the default
`floor` of `cost_gauss_newton_product`."""


def _checked_cost(name, operator, data, measured_pixels, model, psi, probe,
                  scan, eigen_probe, eigen_weights, fly, check_positions,
                  checked, binning=1):
    """Every refusal of the cost functions, none of which needs a device until
    the last: (fly, whatever `checked` returns besides, counts, mask or None,
    num_measured, the model's number).  checked(slices): the form's own
    `_checked*` call, which returns fly or (fly, tangents).  binning = B: the
    counts and the mask are (det // B, det // B), num_measured counts data
    pixels."""
    if (isinstance(binning, bool) or not isinstance(binning, int)
            or binning < 1):
        raise ValueError(
            f"{name}: binning={binning!r}: expected an integer >= 1")
    if operator.detector_shape % binning:
        raise ValueError(
            f"{name}: binning={binning} does not divide the far-plane width "
            f"{operator.detector_shape}")
    if not isinstance(data, torch.Tensor):
        raise TypeError(
            f"{name}: data must be a torch device tensor, not "
            f"{type(data).__name__}")
    if data.dtype not in (torch.float32, torch.uint16):
        raise TypeError(
            f"{name}: data must be torch.float32 or torch.uint16, not "
            f"{data.dtype}")
    det = operator.detector_shape // binning  # (the data width)
    frames = _frames(scan, fly)
    if data.ndim != 3 or tuple(data.shape[1:]) != (det, det) or (
            frames is not None and data.shape[0] != frames):
        raise ValueError(
            f"{name}: data must be (N // fly, det, det) = "
            f"({'?' if frames is None else frames}, {det}, {det}), not "
            f"{tuple(data.shape)}"
            + ("" if binning == 1 else f" (binning={binning})"))
    mask, num_measured = None, det * det
    if measured_pixels is not None:
        mask = measured_pixels
        if not isinstance(mask, torch.Tensor):
            raise TypeError(
                f"{name}: measured_pixels must be a torch device tensor, not "
                f"{type(mask).__name__}")
        if mask.dtype not in (torch.bool, torch.uint8):
            raise TypeError(
                f"{name}: measured_pixels must be torch.bool or torch.uint8, "
                f"not {mask.dtype}")
        if tuple(mask.shape) != (det, det):
            raise ValueError(
                f"{name}: measured_pixels must be ({det}, {det}), not "
                f"{tuple(mask.shape)}")
        num_measured = int((mask != 0).sum())
        if num_measured == 0:
            raise ValueError(
                f"{name}: measured_pixels measures no pixel (the cost is a "
                "mean over the measured pixels)")
    if model not in _MODELS:
        raise ValueError(
            f"{name}: unknown noise model {model!r}; one of "
            f"{tuple(_MODELS)}")
    slices = isinstance(psi, torch.Tensor) and psi.ndim == 3 and psi.shape[0] > 1
    if slices and (eigen_weights is not None or eigen_probe is not None):
        raise NotImplementedError(
            f"{name}: several slices (psi.shape[0] = {psi.shape[0]}) with "
            "eigen probes: multislice_intensity has no varying probe")
    out = checked(slices)
    for what, x in (("data", data), ("measured_pixels", mask)):
        if x is not None and x.device.type != "cuda":
            raise TypeError(
                f"{name}: {what} lives on {x.device}; tike_amd runs on the "
                "GPU only and there is no CPU fallback")
    if mask is not None:
        mask = (mask != 0).to(torch.uint8).contiguous()
    return out, data.detach().contiguous(), mask, num_measured, _MODELS[model]


class _Counts:
    """The counts, the mask and the noise model of one call, and the two
    entries on a chunk's far plane."""

    def __init__(self, data, mask, num_measured, model, fly,
                 detector=_D.Detector()):
        self.data, self.mask, self.nm = data, mask, num_measured
        self.model, self.fly = model, fly
        # (`operators.detector`; b or K detached: the factors are taken at
        # I + b, at K (*) I)
        self.detector = detector
        self._stored = None  # the stored intensities of the chunk in hand
        self.u16 = int(data.dtype == torch.uint16)

    def _intensity(self, far, nf):
        """The stored intensities (nf, det, det) of a chunk's far plane
        (tike_intensity: one read of the far plane), in a buffer that is
        reused from chunk to chunk (one stream)."""
        det = far.shape[-1]
        if self._stored is None or self._stored.shape[0] < nf:
            self._stored = torch.empty((nf, det, det), dtype=torch.float32,
                                       device=far.device)
        inten = self._stored[:nf]
        check(
            lib.tike_intensity(A.ptr(far), A.ptr(inten), nf,
                               far.shape[-3] * self.fly, det * det,
                               A.stream_ptr()), "cost (tike_intensity)")
        return inten

    def kernel_sums(self, lo, hi, upstream, ksum):
        """Adds d (sum_f upstream_f cost_f) / d blur of the frames of the
        positions lo ... hi - 1 to ksum (k, k) float64: tike_blur_kernel_sums
        on the intensities `factor` has just stored for this chunk."""
        fly = self.fly
        flo, nf = lo // fly, (hi - lo) // fly
        K = self.detector.value
        k, det = K.shape[-1], self._stored.shape[-1]
        n = lib.tike_blur_kernel_sums_partials(det, k)
        partials = torch.empty(n, dtype=torch.float64, device=ksum.device)
        kgrad = torch.empty((k, k), dtype=torch.float64, device=ksum.device)
        check(
            lib.tike_blur_kernel_sums(
                A.ptr(self._stored[:nf]), A.ptr(K), k,
                A.ptr(self.data[flo:]), self.u16, A.ptr(self.mask),
                None if upstream is None else A.ptr(upstream[flo:]),
                A.ptr(partials), A.ptr(kgrad), nf, det, self.model, self.nm,
                A.stream_ptr()), "cost (tike_blur_kernel_sums)")
        ksum.add_(kgrad)

    def factor(self, lo, hi, far, upstream, costs, table):
        """The detector's `tike_*_cost_factor` (`detector.cost_factor`) on the
        frames of the positions lo ... hi - 1: counts and mask at data
        resolution, the table at the far plane's; with a blur on the chunk's
        stored intensities (tike_intensity)."""
        fly = self.fly
        flo, nf = lo // fly, (hi - lo) // fly
        _D.cost_factor(
            self.detector, far,
            self._intensity(far, nf) if self.detector.kind == "blur" else None,
            A.ptr(self.data[flo:]), self.u16, self.mask,
            None if upstream is None else A.ptr(upstream[flo:]),
            None if costs is None else A.ptr(costs[flo:]), table, nf, fly,
            self.model, self.nm)

    def curvature(self, lo, hi, far, dfar, upstream, costs, dcosts, table,
                  floor=COST_FLOOR):
        """tike_cost_curvature on the frames of the positions lo ... hi - 1."""
        fly = self.fly
        flo, nf = lo // fly, (hi - lo) // fly
        check(
            lib.tike_cost_curvature(
                A.ptr(far), A.ptr(dfar),
                # (the curvature itself does not read the counts)
                None if costs is None and dcosts is None else
                A.ptr(self.data[flo:]), self.u16, A.ptr(self.mask),
                None if upstream is None else A.ptr(upstream[flo:]),
                None if costs is None else A.ptr(costs[flo:]),
                None if dcosts is None else A.ptr(dcosts[flo:]),
                A.ptr(table), nf, far.shape[-3] * fly,
                far.shape[-1] * far.shape[-2], self.model, float(floor),
                self.nm, A.stream_ptr()),
            "cost (tike_cost_curvature)")


def _cost_far_chunks(op, fly, psi, probe, scan, eigen, weights):
    """(lo, hi, far plane of the positions lo ... hi - 1) per chunk of whole
    frames, by the form's forward."""
    N, S, det = scan.shape[0], probe.shape[2], op.detector_shape
    if N == 0:
        return
    if psi.shape[0] > 1:
        for lo, hi, far, beams in _SlicesForward(op, fly, psi, probe, scan):
            del beams  # (general route: only the far plane is kept)
            yield lo, hi, far
        return
    chunk = _chunk_rows(op, probe, fly)
    far_all = torch.empty((min(chunk, N), 1, S, det, det),
                          dtype=torch.complex64, device=psi.device)
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        yield lo, hi, _one_slice_far(op, psi, probe, scan, eigen, weights, lo,
                                     hi, far_all)


def _cost_forward(op, counts, psi, probe, scan, eigen, weights):
    """(frames,) costs: per chunk the form's forward and tike_cost_factor."""
    fly = counts.fly
    A.current_device()  # (hands the library its deterministic-mode scratch)
    costs = torch.empty(scan.shape[0] // fly, dtype=torch.float32,
                        device=psi.device)
    for lo, hi, far in _cost_far_chunks(op, fly, psi, probe, scan, eigen,
                                        weights):
        counts.factor(lo, hi, far, None, costs, None)
    return costs


class _Cost(torch.autograd.Function):
    """The per-frame cost of every form of the model.  The backward is the
    form's own backward whose upstream table of a chunk comes from
    tike_cost_factor on the chunk's recomputed far plane."""

    @staticmethod
    def forward(ctx, psi, probe, scan, eigen_probe, eigen_weights, operator,
                counts, background, blur):
        # (background, blur: `counts` holds them detached; here for their
        # gradients)
        psi, probe, scan = (x.detach().contiguous() for x in (psi, probe, scan))
        eigen = (None if eigen_probe is None else
                 eigen_probe.detach().contiguous())
        weights = (None if eigen_weights is None else
                   eigen_weights.detach().contiguous())
        ctx.operator, ctx.counts = operator, counts
        ctx.have = (eigen is not None, weights is not None)
        ctx.save_for_backward(psi, probe, scan,
                              *(x for x in (eigen, weights) if x is not None))
        return _cost_forward(operator, counts, psi, probe, scan, eigen,
                             weights)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        psi, probe, scan = ctx.saved_tensors[:3]
        rest = list(ctx.saved_tensors[3:])
        eigen = rest.pop(0) if ctx.have[0] else None
        weights = rest.pop(0) if ctx.have[1] else None
        op, counts = ctx.operator, ctx.counts
        fly, det = counts.fly, op.detector_shape
        g = g.to(torch.float32).contiguous()
        A.current_device()  # (hands the library its deterministic-mode scratch)
        tables = {}
        kind = counts.detector.kind
        want_b = kind == "background" and ctx.needs_input_grad[7]
        # d cost_f / d b = d cost_f / d I: the sum of the table over the
        # frames, chunk by chunk in float64, rounded once
        bsum = (torch.zeros((det, det), dtype=torch.float64,
                            device=psi.device) if want_b else None)
        # d (sum_f g_f cost_f) / d K: the chunks' kgrad, float64, rounded once
        want_k = kind == "blur" and ctx.needs_input_grad[8]
        ksum = (torch.zeros(tuple(counts.detector.value.shape),
                            dtype=torch.float64,
                            device=psi.device) if want_k else None)

        def table_of(lo, hi, far):
            # one chunk of table, reused: the chain reads it before the next
            # chunk's entry writes it (one stream)
            nf = (hi - lo) // fly
            if "t" not in tables or tables["t"].shape[0] < nf:
                tables["t"] = torch.empty((nf, det, det), dtype=torch.float32,
                                          device=psi.device)
            table = tables["t"][:nf]
            counts.factor(lo, hi, far, g, None, table)
            if want_b:
                bsum.add_(table.sum(dim=0, dtype=torch.float64))
            if want_k:
                counts.kernel_sums(lo, hi, g, ksum)
            return table

        def gb():
            return (bsum.to(torch.float32) if want_b else None,
                    ksum.to(torch.float32) if want_k else None)

        want = tuple(ctx.needs_input_grad[:5])
        if (want_b or want_k) and not any(want):
            # the background or the kernel alone: no chain behind the tables
            for lo, hi, far in _cost_far_chunks(op, fly, psi, probe, scan,
                                                eigen, weights):
                if want_b:
                    table_of(lo, hi, far)
                else:  # (the kernel's sums need the intensities, no table)
                    counts._intensity(far, (hi - lo) // fly)
                    counts.kernel_sums(lo, hi, g, ksum)
            return (None,) * 7 + gb()
        if psi.shape[0] > 1:
            grads = _multislice_backward_chunks(op, fly, psi, probe, scan,
                                                want[:3], table_of)
            return grads + (None, None, None, None) + gb()
        grads = _backward_chunks(op, fly, psi, probe, scan, want, table_of,
                                 eigen, weights)
        return grads + (None, None) + gb()


def _nearfield_chunks(op, counts, psi, probe, scan, H, visit):
    """Per chunk of whole frames of the near-field form: visit(lo, hi, sc, d,
    how, bufs), how / bufs those of `operators.nearfield.wave_and_back`."""
    from .operators import nearfield as NF
    from .ptycho.solvers.lstsq import _workspace
    fly, N = counts.fly, scan.shape[0]
    S, det = probe.shape[2], op.detector_shape
    how = NF.route(op.probe_shape, det, S)
    chunk = _chunk_rows(op, probe, fly)
    bufs = NF.buffers(_workspace(op), psi.device, max(min(chunk, N), 1), S,
                      det, fly, how)
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        visit(lo, hi, scan[lo:hi], counts.data[lo // fly:hi // fly], how, bufs)


class _NearfieldCost(torch.autograd.Function):
    """The per-frame cost with the detector in the near field
    (`operators.nearfield`): one slice, the shared probe.  Forward: the chain
    with out = NULL.  Backward: the chunk again with grad_output for the
    upstream, the adjoint Fresnel step, its inverse finished to chi
    (tike_fft2_pass2_inplace on the fused routes), then the tail of `_Back`:
    tike_lstsq_gradients, tike_scatter_patches, tike_scan_gradient."""

    @staticmethod
    def forward(ctx, psi, probe, scan, operator, counts, H):
        from .operators import nearfield as NF
        psi, probe, scan = (x.detach().contiguous() for x in (psi, probe, scan))
        ctx.operator, ctx.counts, ctx.H = operator, counts, H
        ctx.save_for_backward(psi, probe, scan)
        A.current_device()
        costs = torch.empty(scan.shape[0] // counts.fly, dtype=torch.float32,
                            device=psi.device)

        def visit(lo, hi, sc, d, how, bufs):
            fly = counts.fly
            NF.wave_and_back(operator, psi, sc, probe, H, d, fly, how, bufs,
                             model=counts.model, measured=counts.mask,
                             num_measured=counts.nm,
                             costs=costs[lo // fly:hi // fly])

        _nearfield_chunks(operator, counts, psi, probe, scan, H, visit)
        return costs

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from .operators import nearfield as NF
        psi, probe, scan = ctx.saved_tensors
        op, counts, H = ctx.operator, ctx.counts, ctx.H
        fly, det, S = counts.fly, op.detector_shape, probe.shape[2]
        Hh, W = psi.shape[-2:]
        g = g.to(torch.float32).contiguous()
        A.current_device()
        want_psi, want_probe, want_scan = ctx.needs_input_grad[:3]
        dev = psi.device
        acc = (torch.zeros((2, Hh, W), dtype=torch.float32, device=dev)
               if want_psi else None)
        gprobe = torch.zeros_like(probe) if want_probe else None
        gscan = torch.empty_like(scan) if want_scan else None
        need_proj = want_psi or want_scan
        proj = {}
        inv_scale = fft_scales(det, op.norm)[1]

        def visit(lo, hi, sc, d, how, bufs):
            n, st = hi - lo, A.stream_ptr()
            # the 2 of torch's gradient of a real function of a complex leaf
            chi, finished = NF.wave_and_back(
                op, psi, sc, probe, H, d, fly, how, bufs, model=counts.model,
                measured=counts.mask, num_measured=counts.nm,
                upstream=g[lo // fly:hi // fly], scale=2.0, want_back=True)
            if not finished:
                check(
                    lib.tike_fft2_pass2_inplace(A.ptr(chi), n * S, det, 1,
                                                inv_scale, st),
                    "nearfield cost backward (inverse pass 2)")
            objproj = None
            if need_proj:
                if "p" not in proj or proj["p"].shape[0] < n:
                    proj["p"] = torch.empty((n, det, det),
                                            dtype=torch.complex64, device=dev)
                objproj = proj["p"][:n]
            check(
                lib.tike_lstsq_gradients(A.ptr(chi), A.ptr(sc), A.ptr(psi),
                                         A.ptr(probe), None, None, 0, 0, None,
                                         None, A.ptr(gprobe), A.ptr(objproj),
                                         n, S, det, Hh, W, st),
                "nearfield cost backward (probe gradient + object projection)")
            if want_psi:
                check(
                    lib.tike_scatter_patches(A.ptr(objproj), A.ptr(sc),
                                             A.ptr(acc), n, det, Hh, W, st),
                    "nearfield cost backward (object gradient)")
            if want_scan:
                check(
                    lib.tike_scan_gradient(A.ptr(objproj), A.ptr(sc),
                                           A.ptr(psi), A.ptr(gscan[lo:hi]), n,
                                           det, Hh, W, st),
                    "nearfield cost backward (scan gradient)")

        _nearfield_chunks(op, counts, psi, probe, scan, H, visit)
        gpsi = torch.complex(acc[0], acc[1])[None] if want_psi else None
        return gpsi, gprobe, gscan, None, None, None


def cost(operator, data, psi, probe, scan, *, model="gaussian",
         measured_pixels=None, eigen_probe=None, eigen_weights=None, fly=1,
         binning=1, check_positions=True, background=None, blur=None,
         nearfield=None):
    """The per-frame cost (N // fly,) float32 of the model's intensity against
    the counts `data` (N // fly, det, det) float32 or uint16 under the
    project's noise models -- "gaussian": mean of (sqrt(I) - sqrt(d))^2,
    "poisson": mean of I - d log(I + 1e-9) -- over the measured pixels
    (measured_pixels (det, det) bool or uint8, None: all), differentiable once
    with respect to whichever of psi, probe, scan, eigen_probe and
    eigen_weights requires a gradient.  ``cost(...).mean()`` is
    ``Ptycho.cost(data, psi, scan, probe, model=, fly=)`` for one slice and
    the shared probe.  psi (D, H, W) with D > 1 is the model of
    `multislice_intensity`, eigen_weights that of `intensity(...,
    eigen_probe=, eigen_weights=)`, otherwise `intensity`.

    The gradient factors are the solvers': 1 - sqrt(d) / (sqrt(I) + 1e-9) and
    1 - d / (I + 1e-9), finite at I = 0; a count under the mask may be NaN: it
    is selected away.  Forward, per chunk of whole frames: the form's forward,
    then tike_cost_factor (costs).  Backward, per chunk: the forward again,
    tike_cost_factor with grad_output for the upstream (the chunk's table),
    and the form's backward chain from the point where it reads the table.  No
    tensor of N // fly * det * det elements exists at any time.

    binning = B > 1 (B divides det): the far plane is B times finer than the
    counts -- data (N // fly, det // B, det // B), measured_pixels
    (det // B, det // B), a measured pixel the sum of the model's intensity
    over its B x B far-plane pixels -- for every form; ``cost(...).mean()`` is
    ``Ptycho.cost(..., binning=B)``.  tike_binned_cost_factor stands in the
    place of tike_cost_factor and writes the chunk's table at far-plane
    resolution, a bin's value replicated over its pixels, so the backward
    chain is unchanged; no binned or unbinned intensity of all frames exists.

    background: a (det, det) float32 device tensor b, the incoherent
    background of ptycho.BackgroundOptions in the stored layout of the
    counts: the costs and every gradient above are taken at I + b
    (tike_background_cost_factor in the place of tike_cost_factor), and b may
    require a gradient itself: d cost_f / d b = d cost_f / d I, so b.grad is
    the sum of the chunks' tables over their frames (float64, rounded once);
    no tensor of N // fly * det * det elements exists for it either.  A value
    under the mask may be NaN.  NotImplementedError with binning > 1.

    blur: a (k, k) float32 device tensor K, k in {3, 5, 7}, used as given (the
    caller keeps it non-negative with sum 1): the costs and every gradient
    above are taken at K (*) I, the convolution of each frame's intensity with
    K, cyclic over the (det, det) plane in the stored layout of the counts
    (the physical convolution with the detector's opposite edges joined) --
    partial spatial coherence, a detector's point-spread function.  Per chunk
    the intensities are stored once (tike_intensity) and
    tike_blur_cost_factor, in the place of tike_cost_factor, writes the costs
    or the table K (star) (g mask l' / num_measured); the backward chain is
    unchanged, so this holds for every form of the model.  K may require a
    gradient: the sum of the chunks' tike_blur_kernel_sums, float64, rounded
    once.  NotImplementedError with binning > 1 or with a background.

    nearfield: a (det, det) complex64 device tensor H in FFT order, used as
    given (it takes no gradient): the detector sits in the near field, probe
    window = detector, and the intensity is |IFFT2(H FFT2(patch x probe))|^2
    summed over the modes and the `fly` positions of a frame
    (ptycho.NearFieldOptions; data and measured_pixels in the natural layout of
    the detector).  One slice, the shared probe; exact gradients with respect
    to psi, probe and scan.  At 128^2 and 256^2 the forward is tike_fwd_pass1
    -> tike_fresnel_colpass -> tike_nearfield_plane_gradient with out = NULL:
    the detector-plane wave never exists in memory.  ``cost(...).mean()`` is
    ``Ptycho.cost(..., nearfield=H)``.  NotImplementedError with eigen probes,
    several slices, binning > 1, a background, a blur, or an H that requires a
    gradient; `cost_jvp` and `cost_gauss_newton_product` take no nearfield.

    Raises what the form's intensity raises, ValueError for a binning that is
    no integer >= 1 or does not divide the far-plane width, TypeError / ValueError for data
    or measured_pixels of another type, dtype or shape, ValueError for a mask
    that measures nothing or an unknown model, NotImplementedError for several
    slices with eigen probes.  measured_pixels costs a read-back per call.
    """
    name = "cost"

    def checked(slices):
        return _checked(operator, psi, probe, scan, fly, check_positions,
                        name=name, slices=slices, eigen_probe=eigen_probe,
                        eigen_weights=eigen_weights)

    fly, data, mask, nm, model = _checked_cost(
        name, operator, data, measured_pixels, model, psi, probe, scan,
        eigen_probe, eigen_weights, fly, check_positions, checked, binning)
    if nearfield is not None:
        H = _checked_nearfield(name, operator, nearfield, psi, eigen_probe,
                               eigen_weights, binning, background, blur)
        return _NearfieldCost.apply(psi, probe, scan, operator,
                                    _Counts(data, mask, nm, model, fly), H)
    detector = _D.far_field(binning)
    if background is not None:
        detector = _D.Detector("background", 1, _checked_background(
            name, operator, background, binning))
    if blur is not None:
        detector = _D.Detector("blur", 1, _checked_blur(
            name, operator, blur, binning, background))
    return _Cost.apply(psi, probe, scan, eigen_probe, eigen_weights, operator,
                       _Counts(data, mask, nm, model, fly, detector),
                       background, blur)


def _checked_nearfield(name, operator, nearfield, psi, eigen_probe,
                       eigen_weights, binning, background, blur):
    """The propagator of `cost` on the device, after its refusals."""
    det = operator.detector_shape
    _D.refuse("nearfield", _D.entry(name), binning=binning,
              background=background is not None, blur=blur is not None,
              slices=psi.shape[0], eigen=(eigen_probe is not None
                                          or eigen_weights is not None),
              window=operator.probe_shape, det=det)
    return _D.device_value(name, "nearfield", nearfield, det)


def _checked_background(name, operator, background, binning):
    """The background of `cost`, detached and contiguous, after its
    refusals."""
    _D.refuse("background", _D.entry(name), binning=binning)
    return _D.device_value(name, "background", background,
                           operator.detector_shape)


def _checked_blur(name, operator, blur, binning, background):
    """The blur kernel of `cost`, detached and contiguous, after its
    refusals."""
    _D.refuse("blur", _D.entry(name), binning=binning,
              background=background is not None)
    return _D.device_value(name, "blur", blur, operator.detector_shape)


def _refuse_binned_curvature(name, binning):
    """`cost_jvp` and `cost_gauss_newton_product` on a binned far plane."""
    if binning != 1:
        raise NotImplementedError(
            f"{name} with binning={binning!r}: the forward-mode derivative "
            "and the Gauss-Newton product of the cost are not implemented "
            "for a binned far plane; `cost` is")


def _cost_tangents(name, operator, data, measured_pixels, model, psi, probe,
                   scan, eigen_probe, eigen_weights, d_psi, d_probe, d_scan,
                   d_eigen_probe, d_eigen_weights, fly, check_positions):
    """The checks of `cost_jvp` and `cost_gauss_newton_product`: (counts, the
    five primals detached and contiguous, the five tangents)."""
    if eigen_weights is None and (d_eigen_probe is not None
                                  or d_eigen_weights is not None):
        raise ValueError(
            f"{name}: d_eigen_probe or d_eigen_weights without eigen_weights")

    def checked(slices):
        return _checked_jvp(
            name, operator, (psi, probe, scan, eigen_probe, eigen_weights),
            (d_psi, d_probe, d_scan, d_eigen_probe, d_eigen_weights), fly,
            check_positions, slices=slices, eigen=eigen_weights is not None)

    (fly, tangents), data, mask, nm, model = _checked_cost(
        name, operator, data, measured_pixels, model, psi, probe, scan,
        eigen_probe, eigen_weights, fly, check_positions, checked)
    primals = [None if x is None else x.detach().contiguous()
               for x in (psi, probe, scan, eigen_probe, eigen_weights)]
    return _Counts(data, mask, nm, model, fly), primals, list(tangents)


def cost_jvp(operator, data, psi, probe, scan, *, model="gaussian",
             measured_pixels=None, eigen_probe=None, eigen_weights=None,
             d_psi=None, d_probe=None, d_scan=None, d_eigen_probe=None,
             d_eigen_weights=None, fly=1, binning=1, check_positions=True):
    """(costs, dcosts), both (N // fly,) float32 outside any autograd graph:
    the costs of `cost` -- the same bits -- and their directional derivative
    along the tangents of the form's `*_jvp` function (each None or of its
    primal's shape): the exact slope of a line search.  The form's
    forward-mode chunk loop with tike_cost_curvature in the place of
    tike_intensity_tangent: neither I nor dI is stored.  With no tangent
    dcosts is zeros and only the primal launches.

    Raises what `cost` and the form's `*_jvp` function raise, and
    NotImplementedError for binning > 1 (there is no curvature entry for a
    binned far plane).
    """
    _refuse_binned_curvature("cost_jvp", binning)
    counts, primals, tangents = _cost_tangents(
        "cost_jvp", operator, data, measured_pixels, model, psi, probe, scan,
        eigen_probe, eigen_weights, d_psi, d_probe, d_scan, d_eigen_probe,
        d_eigen_weights, fly, check_positions)
    fly = counts.fly
    if all(t is None for t in tangents):
        costs = _cost_forward(operator, counts, *primals)
        return costs, torch.zeros_like(costs)
    costs = torch.empty(primals[2].shape[0] // fly, dtype=torch.float32,
                        device=primals[0].device)
    dcosts = torch.empty_like(costs)
    _jvp_loop(
        operator, primals, tangents, fly, primal=False,
        sink=lambda lo, hi, far, dfar: counts.curvature(
            lo, hi, far, dfar, None, costs, dcosts, None))
    return costs, dcosts


def cost_gauss_newton_product(operator, data, psi, probe, scan, *,
                              model="gaussian", measured_pixels=None,
                              eigen_probe=None, eigen_weights=None, d_psi=None,
                              d_probe=None, d_scan=None, d_eigen_probe=None,
                              d_eigen_weights=None, upstream=None,
                              floor=COST_FLOOR, fly=1, wrt=None, binning=1,
                              check_positions=True):
    """J^T diag(upstream_f c / (num_measured (I + floor))) J v on the measured
    pixels: the Gauss-Newton matrix of sum_f upstream_f cost_f applied to the
    tangents v of `cost_jvp` -- c = 1/2 for "gaussian" (the curvature
    1 / (2 I) of the amplitude residual), 1 for "poisson" (the Fisher
    information 1 / I).  One tensor per name in `wrt` (default: every input
    of the form; the names and the order of the form's `*_gauss_newton_product`),
    in the `.grad` convention of `cost`.  upstream: (N // fly,) float32 device
    tensor or None (ones); floor >= 0, the project's 1e-9 by default.  `data`
    only names dtype and shape here: the curvature does not depend on the
    counts.

    One slice (with or without eigen probes): ONE chunk loop with the far
    plane resident -- the form's forward-mode launches, tike_cost_curvature
    (the chunk's table), then the backward chain of the form on the SAME far
    plane: no third forward, no I, dI or weight over all frames.  Several
    slices: composed -- the forward-mode chunks with tike_cost_curvature write
    the (N // fly, det, det) table, then the backward of
    `multislice_intensity` runs with it.  Only what `wrt` names is launched
    behind the table.

    Raises what `cost_jvp` raises, ValueError for names in `wrt` the form does
    not have (or none, or one twice), for a negative or non-finite floor,
    TypeError / ValueError for an upstream of another type, dtype, shape or
    device, NotImplementedError for binning > 1.
    """
    name = "cost_gauss_newton_product"
    _refuse_binned_curvature(name, binning)
    names = _EIGEN_WRT if eigen_weights is not None else _WRT
    wrt = _checked_product(
        name, operator, (psi, probe, scan, eigen_probe, eigen_weights), None,
        fly, names if wrt is None else wrt, names)
    floor = float(floor)
    if not (floor >= 0.0 and floor != float("inf")):
        raise ValueError(f"{name}: floor must be finite and >= 0, not {floor}")
    if upstream is not None:
        _checked_frame_tensor(name, "upstream", upstream, operator, psi, scan,
                              fly, planes=False)
        upstream = upstream.detach().contiguous()
    counts, primals, tangents = _cost_tangents(
        name, operator, data, measured_pixels, model, psi, probe, scan,
        eigen_probe, eigen_weights, d_psi, d_probe, d_scan, d_eigen_probe,
        d_eigen_weights, fly, check_positions)
    fly = counts.fly
    psi, probe, scan, eigen, weights = primals
    by_name = dict(zip(_EIGEN_WRT, primals))
    if all(t is None for t in tangents) or scan.shape[0] == 0:
        return tuple(torch.zeros_like(by_name[k]) for k in wrt)
    op, det, dev = operator, operator.detector_shape, psi.device
    want = tuple(k in wrt for k in _EIGEN_WRT)
    if psi.shape[0] > 1:
        table = torch.empty((scan.shape[0] // fly, det, det),
                            dtype=torch.float32, device=dev)
        _jvp_loop(
            op, primals, tangents, fly, primal=False,
            sink=lambda lo, hi, far, dfar: counts.curvature(
                lo, hi, far, dfar, upstream, None, None,
                table[lo // fly:hi // fly], floor))
        grads = _multislice_backward_chunks(
            op, fly, psi, probe, scan, want[:3],
            lambda lo, hi, far: table[lo // fly:hi // fly]) + (None, None)
    else:
        rows = min(_chunk_rows(op, probe, fly, halve=True), scan.shape[0])
        back = _Back(op, fly, psi, probe, scan, want, rows, eigen, weights,
                     resident=True)
        table_all = torch.empty((rows // fly, det, det), dtype=torch.float32,
                                device=dev)

        def sink(lo, hi, far, dfar):
            table = table_all[:(hi - lo) // fly]
            counts.curvature(lo, hi, far, dfar, upstream, None, None, table,
                             floor)
            # (the tangent far plane is dead behind the table: the scaled
            # inverse writes there)
            back.run(lo, hi, far, table, spare=dfar)

        _jvp_loop(op, primals, tangents, fly, primal=False, sink=sink)
        grads = back.result()
    return tuple(dict(zip(_EIGEN_WRT, grads))[k] for k in wrt)
