"""Float64 model of `tike_amd.autograd.multislice_intensity` (test
infrastructure), on tests/autograd_model.py (the bilinear gather, its taps, the
scan gradient of one slice) and tests/cgrad_multislice.py (the optics and the
Fresnel propagator between two slices).

    beam_0[n, s] = P_s
    e_d[n, s]    = patch_n(O_d) beam_d[n, s]
    beam_{d+1}   = IFFT2(FFT2(e_d) Hprop)              (the same for every norm)
    far[n, s]    = F e_{D-1}[n, s]                     (the operator's norm)
    I[f]         = sum over the fly positions of frame f and the modes |far|^2

`intensity` is differentiable by torch.autograd; `hand_gradients` restates the
backward the HIP route implements with no autograd, in the precision of its
inputs (complex128 for the bars, complex64 for the float32 restatement that
fixes the scan bar), and returns the absolute-term sums
A_n = sum_d sum_px (|Dy|, |Dx|) |objproj_d| the scan bars are stated in.
"""
import numpy as np
import torch

import autograd_model as am
from cgrad_multislice import DISTANCE, PIXEL, WAVELENGTH, propagator

C128, F64 = am.C128, am.F64


def optics(pw):
    """The keyword arguments that give `tike_amd.operators.Ptycho` the
    propagator of `propagator(pw)`."""
    return dict(probe_wavelength=WAVELENGTH,
                probe_FOV_lengths=(pw * PIXEL, pw * PIXEL),
                multislice_propagation_distance=DISTANCE)


def as_model(psi, probe, scan, single=False):
    """Host arrays -> (psi, probe, scan, Hprop) tensors: complex128 / float64
    holding the float32 values, or -- single -- complex64 / float32."""
    c, f = (torch.complex64, torch.float32) if single else (C128, F64)
    pw = probe.shape[-1]
    return (torch.from_numpy(np.asarray(psi)).to(c),
            torch.from_numpy(np.asarray(probe)).to(c),
            torch.from_numpy(np.asarray(scan, dtype=np.float32)).to(f),
            torch.from_numpy(propagator(pw)).to(c))


def _fft2(x):
    return torch.fft.fft2(x, norm="ortho")


def _ifft2(x):
    return torch.fft.ifft2(x, norm="ortho")


def _forward(psi, probe, scan, Hprop, norm):
    """(far (N, S, pw, pw), [patch_n(O_d)], [beam_d])."""
    pw = probe.shape[-1]
    beams, patches = [probe[0, 0][None]], []
    for d in range(psi.shape[0]):
        patches.append(am.patches(psi[d:d + 1], scan, pw))
        wave = patches[d][:, None] * beams[d]
        if d + 1 < psi.shape[0]:
            beams.append(_ifft2(_fft2(wave) * Hprop))
    return torch.fft.fft2(wave, norm=norm), patches, beams


def intensity(psi, probe, scan, Hprop, fly=1, norm="ortho"):
    """(N // fly, pw, pw) real; differentiable by torch.autograd."""
    far = _forward(psi, probe, scan, Hprop, norm)[0]
    each = (far.real**2 + far.imag**2).sum(dim=1)
    return each.reshape(scan.shape[0] // fly, fly, *each.shape[-2:]).sum(dim=1)


def autograd_gradients(psi, probe, scan, Hprop, g, fly=1, norm="ortho"):
    """(intensity, psi.grad (D, H, W), probe.grad, scan.grad) of
    sum(g * intensity) by torch.autograd on the model."""
    psi, probe, scan = (x.detach().clone().requires_grad_(True)
                        for x in (psi, probe, scan))
    inten = intensity(psi, probe, scan, Hprop, fly, norm)
    (inten * g).sum().backward()
    return inten.detach(), psi.grad, probe.grad, scan.grad


def _scatter(objproj, scan, H, W):
    """The adjoint of the bilinear gather of one slice: (H, W)."""
    pw = objproj.shape[-1]
    corner = torch.floor(scan)
    frac = scan - corner
    fy, fx = frac[:, 0, None, None], frac[:, 1, None, None]
    r = torch.arange(pw)
    yy = (corner[:, 0].long()[:, None, None] + r[None, :, None]).expand(
        -1, pw, pw)
    xx = (corner[:, 1].long()[:, None, None] + r[None, None, :]).expand(
        -1, pw, pw)
    out = torch.zeros((H, W), dtype=objproj.dtype)
    for dy, dx, w in ((0, 0, (1 - fx) * (1 - fy)), (0, 1, fx * (1 - fy)),
                      (1, 0, (1 - fx) * fy), (1, 1, fx * fy)):
        out.index_put_((yy + dy, xx + dx), w * objproj, accumulate=True)
    return out


def hand_gradients(psi, probe, scan, Hprop, g, fly=1, norm="ortho"):
    """The backward of `multislice_intensity`, no autograd, in the precision
    of the inputs: dict(psi (D, H, W), probe, scan (N, 2), A (N, 2), objproj
    (D, N, pw, pw)); scan and A are accumulated in float64 from the terms of
    that precision (as the kernel does)."""
    with torch.no_grad():
        D, (H, W) = psi.shape[0], psi.shape[-2:]
        pw = probe.shape[-1]
        far, patches, beams = _forward(psi, probe, scan, Hprop, norm)
        G = 2 * g.repeat_interleave(fly, dim=0)[:, None] * far
        # F^H: the unscaled inverse times the FORWARD scale
        w = torch.fft.ifft2(G, norm="forward") * am.forward_scale(pw, norm)
        gpsi = torch.zeros_like(psi)
        objproj = []
        gscan = torch.zeros((scan.shape[0], 2), dtype=F64)
        absum = torch.zeros((scan.shape[0], 2), dtype=F64)
        for d in range(D - 1, -1, -1):
            q = (beams[d].conj() * w).sum(dim=1)
            objproj.insert(0, q)
            gpsi[d] = _scatter(q, scan, H, W)
            gs, a = _scan_terms(q, psi[d:d + 1], scan)
            gscan += gs
            absum += a
            w = patches[d].conj()[:, None] * w
            if d > 0:
                w = _ifft2(_fft2(w) * Hprop.conj())
        gprobe = w.sum(dim=0)[None, None]
    return dict(psi=gpsi, probe=gprobe, scan=gscan, A=absum,
                objproj=torch.stack(objproj))


def _scan_terms(q, layer, scan):
    """autograd_model.scan_gradient with the terms formed in the precision of
    the inputs and summed in float64."""
    pw = q.shape[-1]
    (o00, o01, o10, o11), fy, fx = am._taps(layer, scan, pw)
    dy = (1 - fx) * (o10 - o00) + fx * (o11 - o01)
    dx = (1 - fy) * (o01 - o00) + fy * (o11 - o10)
    term = lambda t: (t * q.conj()).real.to(F64).sum(dim=(1, 2))
    absterm = lambda t: (t.abs() * q.abs()).to(F64).sum(dim=(1, 2))
    return (torch.stack([term(dy), term(dx)], dim=1),
            torch.stack([absterm(dy), absterm(dx)], dim=1))


# ------------------------------------------------------- the end-to-end cases
# (N, S, pw, obj, D, fly): general 32 and 64; fused 128 (fly, then the S = 8
# limit), 256, and 512 with its three-launch step back
END_TO_END_CASES = [(6, 2, 32, 72, 2, 1), (8, 2, 64, 104, 3, 2),
                    (6, 2, 128, 170, 2, 2), (4, 8, 128, 170, 3, 1),
                    (4, 2, 256, 300, 3, 2), (2, 1, 512, 560, 2, 1)]

SCAN_BAR = 1e-6
"""|err| <= SCAN_BAR * A_n for scan.grad end to end: the single-slice bar,
which holds while the float32 restatement of `hand_gradients` stays within
1e-7 A_n of the float64 one (test_autograd_multislice_cpu.py asserts that;
profiles/autograd_multislice.md has the figures)."""


def rc(rng, *s):
    return (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(
        np.complex64)


def case(N, S, pw, obj, D, fly, norm="ortho"):
    """Host inputs of an end-to-end case: D random slices near 1 (a thick
    sample transmits: O = 1 + 0.2 x complex white noise), S random modes, positions over the
    whole allowed range, a random signed upstream gradient."""
    rng = np.random.default_rng(N + 3 * S + 5 * pw + 7 * D)
    psi = (1 + 0.2 * rc(rng, D, obj, obj)).astype(np.complex64)
    probe = rc(rng, 1, 1, S, pw, pw)
    scan = (1 + rng.random((N, 2)) * (obj - pw - 1)).astype(np.float32)
    g = rng.standard_normal((N // fly, pw, pw)).astype(np.float32)
    return dict(psi=psi, probe=probe, scan=scan, g=g, fly=fly, norm=norm)


def case_model(c, single=False):
    """The model's intensity and hand gradients of `case(...)`, host arrays:
    dict(intensity, grad_psi, grad_probe, grad_scan, grad_A)."""
    m = as_model(c["psi"], c["probe"], c["scan"], single)
    g = torch.from_numpy(c["g"]).to(m[2].dtype)
    with torch.no_grad():
        inten = intensity(*m, c["fly"], c["norm"]).numpy()
    hand = hand_gradients(*m, g, c["fly"], c["norm"])
    return dict(intensity=inten, **{
        "grad_" + k: v.numpy() for k, v in hand.items() if k != "objproj"})


# ----------------------------------------------------------- position recovery
def problem(pw=32, H=96, fly=2, side=14, step=4, seed=0):
    """`autograd_model.problem` with a second slice from
    `cgrad_multislice.problem`'s recipe (amplitude 0.8 ... 1, about 0.3 rad of
    phase noise), data from the true positions through both slices.  Host
    arrays: dict(psi (2, H, H), probe, scan_true, scan_start, data, det,
    fly)."""
    p = am.problem(pw=pw, H=H, fly=fly, side=side, step=step, seed=seed)
    rng = np.random.default_rng(seed + 1000)
    second = ((0.8 + 0.2 * rng.random((1, H, H))) * np.exp(
        0.3j * rng.standard_normal((1, H, H)))).astype(np.complex64)
    psi = np.concatenate([p["psi"], second])
    with torch.no_grad():
        data = intensity(*as_model(psi, p["probe"], p["scan_true"]),
                         fly).numpy()
    return dict(p, psi=psi, data=data.astype(np.float32))


RECOVERY = dict(seed=49, steps=80, lr=0.05)
"""Seed and Adam steps of the position-recovery tests, chosen on the float64
model: with them the model ALONE brings the RMS position error to 0.43 of its
start (test_autograd_multislice_cpu.py asserts <= 0.5).  The second slice is
white phase noise, whose bilinear patch changes character with the fraction of
the position, so the positions alone settle in local minima: of the seeds
0 ... 69 tried at 120 steps, most end between 0.5 and 0.65 of their start, two
below 0.5 (48: 0.495; 49: 0.42), and more steps change nothing."""


def recover_on_model(p):
    """Adam on the positions alone on the float64 model: (final, costs)."""
    psi, probe, _, Hprop = as_model(p["psi"], p["probe"], p["scan_true"])
    data = torch.from_numpy(p["data"]).to(F64)
    start = torch.from_numpy(p["scan_start"]).to(F64)
    return am.recover(
        lambda s: am.amplitude_loss(
            intensity(psi, probe, s, Hprop, p["fly"]), data), start,
        steps=RECOVERY["steps"], lr=RECOVERY["lr"])
