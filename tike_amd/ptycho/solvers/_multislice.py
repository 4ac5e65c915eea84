"""The walk through an object of several slices that `cgrad` and
`tike_amd.autograd` share: e_d = patch(O_d) x beam_d, beam_{d+1} =
Fresnel(e_d), far = F e_{D-1}, and the EXACT adjoint back through every slice
(no division by the number of slices).  One copy of the route decision, the
chunk sizing, the `ms_*` workspace buffers, the forward of a chunk on either
route and the step back on the two-pass kernels; what the two users do
differently comes in as arguments.  rpie's fused path takes its chunk and its
buffers from here too; its walk back is the reference's per-slice numerator,
not this adjoint, and stays in rpie.py.

The step back on the GENERAL route is not here, on purpose: cgrad walks back
through `Convolution.adj` into a complex gradient, autograd through
`tike_lstsq_gradients` and the planar scatter -- different launches with
different bits.  It stays `cgrad._multislice_chunk_general` and
`autograd._general_back`.

`label` names the caller in every error of a launch issued here.
"""
import torch

from ... import _arrays as A
from ..._lib import check, lib
from ...operators.multislice import (chunk_within_hbm, fused_forward,
                                     fused_slices)
from ...operators.propagation import fft_scales
from . import lstsq as L


def fused_route(op, probe, lever):
    """True: the two-pass kernels (128^2, 256^2 or 512^2 tiles, probe window =
    detector, at most 8 modes) with the caller's lever on; False: the general
    operators slice by slice."""
    return bool(lever and fused_slices(probe.shape[-1], op.detector_shape,
                                       probe.shape[-3]))


def chunk_positions(op, device, S, planes, fused=True):
    """Positions per chunk.  Fused route: `planes` complex64 sets of
    (S, det, det) per position within HALF the HBM that is free right now
    (`chunk_within_hbm`); the general route and `CHUNK_POSITIONS_OVERRIDE`:
    `lstsq.chunk_positions`."""
    det = op.detector_shape
    if L.CHUNK_POSITIONS_OVERRIDE or not fused:
        return L.chunk_positions(S, det)
    return chunk_within_hbm(L._workspace(op), device, planes, S, det)


def fused_buffers(op, device, D, S, nmax, nback=1, nproj=1):
    """(far (nmax, S, det, det), mid (nback, nmax, ...), beams (D - 1, nmax,
    ...), objproj (nproj, nmax, det, det)) of the operator's workspace: what a
    chunk of at most nmax positions holds on the fused route."""
    ws, det, c64 = L._workspace(op), op.detector_shape, torch.complex64
    return (ws.get("ms_far", (nmax, S, det, det), c64, device),
            ws.get("ms_mid", (nback, nmax, S, det, det), c64, device),
            ws.get("ms_beams", (max(D - 1, 1), nmax, S, det, det), c64,
                   device),
            ws.get("ms_objproj", (nproj, nmax, det, det), c64, device))


def fused_far(op, psi, sc, probe, far, beams, label):
    """The far plane of a chunk in `far[:n]` (returned), the probes incident
    on the slices behind the first in `beams[:, :n]`: `fused_forward` ->
    tike_fft2_pass2_inplace."""
    n, S, det = sc.shape[0], probe.shape[-3], op.detector_shape
    fwd_scale, inv_scale = fft_scales(det, op.norm)
    prop = op.diffraction.propagation._propagator((det, det), psi.device)
    fused_forward(psi, sc, probe, 0, far[:n], beams, prop,
                  fwd_scale * inv_scale)
    check(
        lib.tike_fft2_pass2_inplace(A.ptr(far), n * S, det, 0, fwd_scale,
                                    A.stream_ptr()), f"{label}: far field")
    return far[:n]


def general_far(op, psi, sc, probe):
    """(far (n, S, det, det), [the probe incident on every slice]) through
    the general operators, any probe window = detector size."""
    conv, fresnel = op.diffraction.diffraction, op.diffraction.propagation
    beams = [probe[0]]  # (1, S, pw, pw), then (n, S, pw, pw)
    for d in range(psi.shape[0]):
        wave = conv.fwd(psi=psi[d], scan=sc, probe=beams[d])
        if d + 1 < psi.shape[0]:
            beams.append(fresnel.fwd(wave, overwrite=True))
    return op.propagation.fwd(wave, overwrite=True), beams


def fused_step_back(op, psi, sc, probe, far, mid, beams, objproj, acc, pacc, *,
                    first_scale, scale, want_proj, one_launch, label):
    """From `mid` (n, S, det, det) holding pass 1 of the last transform's
    inverse to both products of slice 0, per slice behind the first:
    tike_slice_step_back (one_launch; 128^2 and 256^2 only), else
    tike_ifft2_pass2_products(keep_chi) -> tike_conv_adj_probe ->
    tike_fft2_pass1; -> tike_scatter_patches -> tike_fresnel_colpass(adjoint).
    `far` is scratch; beams[d - 1] (n, S, det, det), the probe incident on
    slice d >= 1, is overwritten.  first_scale rides on the first pass 2 of the
    walk, scale on the later ones.  objproj (1 | D, n, det, det): one plane
    reused or one per slice, left holding sum_s conj(beam_d) w_d; the one
    launch writes it only if want_proj, the other launches always.  acc
    (D, 2, H, W) float32 or None, pacc (S, det, det) complex64 or None: they
    receive the products of the object and of the probe."""
    D, (H, W) = psi.shape[0], psi.shape[-2:]
    n, S, det = sc.shape[0], probe.shape[-3], op.detector_shape
    st = A.stream_ptr()
    fwd_scale = fft_scales(det, op.norm)[0]
    prop = op.diffraction.propagation._propagator((det, det), psi.device)
    one_launch = one_launch and det in (128, 256)
    assert len(objproj) in (1, D), (len(objproj), D)
    for d in range(D - 1, 0, -1):
        beam = beams[d - 1]
        proj = objproj[d] if len(objproj) > 1 else objproj[0]
        if one_launch:
            # (no projection wanted: none formed, the beams unread)
            check(
                lib.tike_slice_step_back(A.ptr(mid), A.ptr(psi[d]), A.ptr(sc),
                                         A.ptr(beam),
                                         A.ptr(proj) if want_proj else None,
                                         A.ptr(far), n, S, det, H, W,
                                         first_scale, st),
                f"{label}: step back through a slice")
        else:
            check(
                lib.tike_ifft2_pass2_products(
                    A.ptr(mid), A.ptr(psi[d]), A.ptr(sc), A.ptr(beam), 1,
                    A.ptr(proj), None, 1.0, None, 1, n, S, det, H, W,
                    first_scale, st),
                f"{label}: inverse pass 2 + object projection")
            # (the beam is dead from here on: it takes conj(patch) x wave)
            check(
                lib.tike_conv_adj_probe(A.ptr(mid), A.ptr(sc), A.ptr(psi[d]),
                                        A.ptr(beam), n, S, det, det, H, W, st),
                f"{label}: conj(patch) x wave")
            check(lib.tike_fft2_pass1(A.ptr(beam), A.ptr(far), n * S, det, 0,
                                      st), f"{label}: step back, pass 1")
        if acc is not None:
            check(
                lib.tike_scatter_patches(A.ptr(proj), A.ptr(sc), A.ptr(acc[d]),
                                         n, det, H, W, st),
                f"{label}: object gradient of a slice")
        check(
            lib.tike_fresnel_colpass(A.ptr(far), A.ptr(prop), 1, A.ptr(mid),
                                     n * S, det, fwd_scale, st),
            f"{label}: adjoint Fresnel step, column passes")
        first_scale = scale
    check(
        lib.tike_ifft2_pass2_products(
            A.ptr(mid), A.ptr(psi[0]), A.ptr(sc), A.ptr(probe), 0,
            A.ptr(objproj[0]), A.ptr(pacc), 1.0, None, 0, n, S, det, H, W,
            first_scale, st),
        f"{label}: first slice, inverse pass 2 + both products")
    if acc is not None:
        check(
            lib.tike_scatter_patches(A.ptr(objproj[0]), A.ptr(sc),
                                     A.ptr(acc[0]), n, det, H, W, st),
            f"{label}: object gradient of the first slice")
