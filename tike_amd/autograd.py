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
"""
import torch
from torch.autograd.function import once_differentiable

from . import _arrays as A
from ._lib import check, lib
from .operators.propagation import fft_scales

MAX_MODES = 16
"""Probe modes `tike_lstsq_gradients` takes (TK_MAX_MODES)."""

_SCALED_INVERSE_SIZES = (128, 256, 512)
"""Detector sizes of `tike_ifft2_crop_scaled`."""


def _checked(operator, psi, probe, scan, fly, check_positions):
    """Every refusal, in an order that needs no device until the last one."""
    for name, x, dtype in (("psi", psi, torch.complex64),
                           ("probe", probe, torch.complex64),
                           ("scan", scan, torch.float32)):
        if not isinstance(x, torch.Tensor):
            raise TypeError(
                f"intensity: {name} must be a torch device tensor, not "
                f"{type(x).__name__} (host arrays take part in no autograd "
                "graph)")
        if x.dtype != dtype:
            raise TypeError(f"intensity: {name} must be {dtype}, not {x.dtype}")
    if psi.ndim != 3 or probe.ndim != 5 or scan.ndim != 2 or scan.shape[1] != 2:
        raise ValueError(
            "intensity: psi (1, H, W), probe (1, 1, S, pw, pw) and scan "
            f"(N, 2) expected; got {tuple(psi.shape)}, {tuple(probe.shape)}, "
            f"{tuple(scan.shape)}")
    if psi.shape[0] > 1:
        raise NotImplementedError(
            f"intensity with several slices (psi.shape[0] = {psi.shape[0]}): "
            "a differentiable multislice model is not implemented")
    if probe.shape[0] != 1:
        raise NotImplementedError(
            f"intensity with a probe per position (probe.shape[0] = "
            f"{probe.shape[0]}): varying and eigen probes are not implemented")
    pw, det = operator.probe_shape, operator.detector_shape
    if probe.shape[1] != 1 or tuple(probe.shape[-2:]) != (pw, pw):
        raise ValueError(
            f"intensity: probe must be (1, 1, S, {pw}, {pw}) for this "
            f"operator, not {tuple(probe.shape)}")
    if tuple(psi.shape[-2:]) != (operator.nz, operator.n):
        raise ValueError(
            f"intensity: psi must be (1, {operator.nz}, {operator.n}) for "
            f"this operator, not {tuple(psi.shape)}")
    fly = int(fly)
    if fly < 1 or scan.shape[0] % fly:
        raise ValueError(
            f"{scan.shape[0]} scan positions are not a multiple of fly={fly}")
    if probe.shape[2] > MAX_MODES:
        raise ValueError(
            f"intensity: {probe.shape[2]} probe modes; the gradient kernels "
            f"take at most {MAX_MODES}")
    if check_positions and scan.shape[0]:
        # (the fused scatter drops what falls outside the object)
        from .ptycho.position import check_allowed_positions
        check_allowed_positions(scan, psi, probe.shape)
    for name, x in (("psi", psi), ("probe", probe), ("scan", scan)):
        if x.device.type != "cuda":
            raise TypeError(
                f"intensity: {name} lives on {x.device}; tike_amd runs on the "
                "GPU only and there is no CPU fallback")
    return fly


class _Intensity(torch.autograd.Function):

    @staticmethod
    def forward(ctx, psi, probe, scan, operator, fly):
        from .ptycho.ptycho import _intensity_chunks
        psi, probe, scan = (x.detach().contiguous() for x in (psi, probe, scan))
        ctx.operator, ctx.fly = operator, fly
        ctx.save_for_backward(psi, probe, scan)
        A.current_device()  # (hands the library its deterministic-mode scratch)
        det = operator.detector_shape
        if scan.shape[0] == 0:
            return torch.empty((0, det, det), dtype=torch.float32,
                               device=psi.device)
        # chunked; the far plane of a chunk dies with the chunk
        frames = [inten for _, _, inten in _intensity_chunks(
            operator, psi, scan, probe, fly=fly)]
        return frames[0] if len(frames) == 1 else torch.cat(frames)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        from .ptycho.solvers.lstsq import chunk_positions
        psi, probe, scan = ctx.saved_tensors
        op, fly = ctx.operator, ctx.fly
        want_psi, want_probe, want_scan = ctx.needs_input_grad[:3]
        N, S = scan.shape[0], probe.shape[2]
        pw, det = op.probe_shape, op.detector_shape
        H, W = psi.shape[-2:]
        dev = psi.device
        g = g.to(torch.float32).contiguous()
        st = A.stream_ptr()
        # F^H = the unscaled inverse x the forward scale; the 2 of G goes along
        scale = 2.0 * fft_scales(det, op.norm)[0]
        scaled_inverse = det in _SCALED_INVERSE_SIZES
        acc = (torch.zeros((2, H, W), dtype=torch.float32, device=dev)
               if want_psi else None)
        gprobe = (torch.zeros_like(probe) if want_probe else None)
        gscan = (torch.empty_like(scan) if want_scan else None)
        chunk = max(1, chunk_positions(S, det) // fly) * fly  # whole frames
        rows = min(chunk, N)
        far_all = torch.empty((rows, 1, S, det, det), dtype=torch.complex64,
                              device=dev)
        # (the scaled inverse must not work in place; the plain one may)
        mid_all = torch.empty_like(far_all) if scaled_inverse else far_all
        chi_all = mid_all if pw == det else torch.empty(
            (rows, 1, S, pw, pw), dtype=torch.complex64, device=dev)
        need_proj = want_psi or want_scan
        objproj_all = (torch.empty((rows, pw, pw), dtype=torch.complex64,
                                   device=dev) if need_proj else None)
        for lo in range(0, N, chunk):
            hi = min(N, lo + chunk)
            n = hi - lo
            sc = scan[lo:hi]
            far, mid, chi = far_all[:n], mid_all[:n], chi_all[:n]
            table = g[lo // fly:hi // fly]
            op.fwd_device(probe, sc, psi, out=far)
            if scaled_inverse:
                # S * fly planes share a frame's table
                check(
                    lib.tike_ifft2_crop_scaled(A.ptr(far), A.ptr(table),
                                               S * fly, A.ptr(mid), A.ptr(chi),
                                               n * S, det, pw, scale, st),
                    "intensity backward (scaled ifft2 + crop)")
            else:
                check(
                    lib.tike_farplane_scale(A.ptr(far), A.ptr(table), n // fly,
                                            S * fly, det * det, 2.0, st),
                    "intensity backward (upstream gradient)")
                check(
                    lib.tike_ifft2_crop(A.ptr(far), A.ptr(mid), A.ptr(chi),
                                        n * S, det, pw, 0.5 * scale, st),
                    "intensity backward (ifft2 + crop)")
            objproj = objproj_all[:n] if need_proj else None
            check(
                lib.tike_lstsq_gradients(A.ptr(chi), A.ptr(sc), A.ptr(psi),
                                         A.ptr(probe), None, None, 0, 0, None,
                                         None, A.ptr(gprobe), A.ptr(objproj),
                                         n, S, pw, H, W, st),
                "intensity backward (probe gradient + object projection)")
            if want_psi:
                check(
                    lib.tike_scatter_patches(A.ptr(objproj), A.ptr(sc),
                                             A.ptr(acc), n, pw, H, W, st),
                    "intensity backward (object gradient)")
            if want_scan:
                check(
                    lib.tike_scan_gradient(A.ptr(objproj), A.ptr(sc),
                                           A.ptr(psi), A.ptr(gscan[lo:hi]), n,
                                           pw, H, W, st),
                    "intensity backward (scan gradient)")
        gpsi = torch.complex(acc[0], acc[1])[None] if want_psi else None
        return gpsi, gprobe, gscan, None, None


def intensity(operator, psi, probe, scan, *, fly=1, check_positions=True):
    """Diffraction intensities (N // fly, det, det) float32 of an entered
    `tike_amd.operators.Ptycho`, differentiable with respect to whichever of
    psi (1, H, W) complex64, probe (1, 1, S, pw, pw) complex64 and scan (N, 2)
    float32 -- device tensors -- requires a gradient.  Frame f is the sum over
    the positions f * fly ... f * fly + fly - 1 and over the modes: the values
    of ``operator._compute_intensity(..., fly=fly)``; the operator's `norm` is
    honoured.  Once differentiable.

    Raises NotImplementedError for several slices or a probe per position
    (there are no eigen probes either), TypeError for host arrays or other
    dtypes, ValueError when N is no multiple of `fly`, for more than
    `MAX_MODES` modes and -- with check_positions, the default -- for positions
    that `check_allowed_positions` refuses: the object gradient's scatter
    drops what falls outside the object.  check_positions costs a read-back of
    the positions per call.
    """
    fly = _checked(operator, psi, probe, scan, fly, check_positions)
    return _Intensity.apply(psi, probe, scan, operator, fly)
