"""Float64 model of the forward-mode derivative of `tike_amd.autograd.intensity`
(test infrastructure), on `autograd_model._taps`, `patches` and `farplane`:

    dpatch_n   = patch_n(d_psi) + d_scan[n,0] Dy_n(psi) + d_scan[n,1] Dx_n(psi)
    dwave[n,s] = dpatch_n probe[s] + patch_n(psi) d_probe[s]
    dfar[n,s]  = F pad(dwave[n,s])
    dI[f]      = sum_{n in frame f} sum_s 2 Re(conj(far[n,s]) dfar[n,s])

`hand_jvp` is that in float64 (`tangent_nearplane`: its first two lines, padded),
`hand_jvp_float32` the same formulas in float32 / complex64 on the CPU -- what
float32 alone costs --, `inner` the real inner product of the `.grad`
convention, `gauss_newton` the damped Gauss-Newton iteration on the positions
that the CPU and the GPU tests run, and `case` seeded inputs and tangents.
"""
import numpy as np
import torch

import autograd_model as am


def case(N, S, pw, det, H, W, fly, seed=0):
    """Host arrays: psi, probe, scan (fractions in [0.05, 0.95]: a finite
    difference crosses no integer) and the tangents d_psi, d_probe, d_scan of
    their shapes and dtypes."""
    rng = np.random.default_rng(seed + 7 * det + N)
    rc = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)
                     ).astype(np.complex64)
    scan = np.stack([rng.integers(1, H - pw - 1, N) + 0.05 + 0.9 * rng.random(N),
                     rng.integers(1, W - pw - 1, N) + 0.05 + 0.9 * rng.random(N)],
                    1).astype(np.float32)
    return dict(psi=rc(1, H, W), probe=rc(1, 1, S, pw, pw), scan=scan,
                d_psi=rc(1, H, W), d_probe=rc(1, 1, S, pw, pw),
                d_scan=rng.standard_normal((N, 2)).astype(np.float32))


def as_model(c, names=("d_psi", "d_probe", "d_scan")):
    """(psi, probe, scan) and {name: tangent} of `case` as float64 tensors; the
    tangents not in `names` are None."""
    conv = lambda a: torch.from_numpy(a).to(
        am.C128 if np.iscomplexobj(a) else am.F64)
    primal = am.as_model(c["psi"], c["probe"], c["scan"])
    return primal, {k: conv(c[k]) if k in names else None
                    for k in ("d_psi", "d_probe", "d_scan")}


def _tangent_wave(psi, probe, scan, d_psi, d_probe, d_scan):
    """dwave (N, S, pw, pw) in the dtype of psi."""
    pw = probe.shape[-1]
    (o00, o01, o10, o11), fy, fx = am._taps(psi, scan, pw)
    dpatch = torch.zeros_like(o00)
    if d_psi is not None:
        dpatch = dpatch + am.patches(d_psi, scan, pw)
    if d_scan is not None:
        dy = (1 - fx) * (o10 - o00) + fx * (o11 - o01)
        dx = (1 - fy) * (o01 - o00) + fy * (o11 - o10)
        dpatch = (dpatch + d_scan[:, 0, None, None] * dy
                  + d_scan[:, 1, None, None] * dx)
    dwave = dpatch[:, None] * probe[0, 0][None]
    if d_probe is not None:
        dwave = dwave + am.patches(psi, scan, pw)[:, None] * d_probe[0, 0][None]
    return dwave


def _padded(wave, det):
    pw = wave.shape[-1]
    pad = (det - pw) // 2
    near = torch.zeros(wave.shape[:2] + (det, det), dtype=wave.dtype)
    near[:, :, pad:pad + pw, pad:pad + pw] = wave
    return near


def tangent_nearplane(psi, probe, scan, det, d_psi=None, d_probe=None,
                      d_scan=None):
    """pad(dwave) (N, S, det, det) complex128: what `tike_conv_fwd_tangent`
    writes."""
    with torch.no_grad():
        return _padded(_tangent_wave(psi, probe, scan, d_psi, d_probe, d_scan),
                       det)


def hand_jvp(psi, probe, scan, det, d_psi=None, d_probe=None, d_scan=None,
             fly=1, norm="ortho"):
    """(I, dI) float64 (N // fly, det, det), no autograd."""
    with torch.no_grad():
        N = scan.shape[0]
        far = am.farplane(psi, probe, scan, det, norm)
        dfar = torch.fft.fft2(
            tangent_nearplane(psi, probe, scan, det, d_psi, d_probe, d_scan),
            norm=norm)
        frames = lambda x: x.sum(dim=1).reshape(N // fly, fly, det,
                                                det).sum(dim=1)
        return (frames(far.real**2 + far.imag**2),
                frames(2 * (far.conj() * dfar).real))


def hand_jvp_float32(psi, probe, scan, det, d_psi=None, d_probe=None,
                     d_scan=None, fly=1, norm="ortho"):
    """`hand_jvp` with every array complex64 / float32 (float64 model tensors
    in, rounded first): the same formulas at the kernels' precision."""
    low = lambda x: None if x is None else x.to(
        torch.complex64 if x.is_complex() else torch.float32)
    psi, probe, scan, d_psi, d_probe, d_scan = map(
        low, (psi, probe, scan, d_psi, d_probe, d_scan))
    with torch.no_grad():
        N, pw = scan.shape[0], probe.shape[-1]
        wave = am.patches(psi, scan, pw)[:, None] * probe[0, 0][None]
        far = torch.fft.fft2(_padded(wave, det), norm=norm)
        dfar = torch.fft.fft2(_padded(_tangent_wave(
            psi, probe, scan, d_psi, d_probe, d_scan), det), norm=norm)
        frames = lambda x: x.sum(dim=1).reshape(N // fly, fly, det,
                                                det).sum(dim=1)
        return (frames(far.real**2 + far.imag**2),
                frames(2 * (far.real * dfar.real + far.imag * dfar.imag)))


def inner(a, b):
    """The real inner product sum(Re a Re b + Im a Im b) in float64 on the
    host: the pairing under which a `.grad` is the gradient."""
    a, b = (np.asarray(x.detach().cpu() if isinstance(x, torch.Tensor) else x)
            for x in (a, b))
    if np.iscomplexobj(a) or np.iscomplexobj(b):
        a, b = a.astype(np.complex128), b.astype(np.complex128)
        return float((a.real * b.real + a.imag * b.imag).sum())
    return float((a.astype(np.float64) * b.astype(np.float64)).sum())


# --------------------------------------------------- Gauss-Newton on positions
def gauss_newton(forward, jv, jtu, data, start, steps=4, cg_iters=20,
                 damping=1e-3):
    """Levenberg-Marquardt on the positions alone with r = I - data:
    `steps` times solve (J^T J + lam) delta = -J^T r by at most `cg_iters`
    conjugate-gradient iterations from zero, lam = damping * mean|J^T J 1|, and
    step by delta.  forward(scan) -> I, jv(scan, v) -> J v, jtu(scan, u) ->
    J^T u; tensors of one dtype and device.  Returns ([positions after every
    step, host arrays], [cost 0.5 |r|^2 before every step and after the
    last])."""
    dot = lambda a, b: float((a.double() * b.double()).sum())
    scan = start.detach().clone()
    after, costs = [], []
    for _ in range(steps):
        r = forward(scan) - data
        costs.append(0.5 * dot(r, r))
        hess = lambda v: jtu(scan, jv(scan, v))
        lam = damping * float(hess(torch.ones_like(scan)).abs().mean())
        b = -jtu(scan, r)
        delta = torch.zeros_like(scan)
        res, p = b.clone(), b.clone()
        rs0 = rs = dot(res, res)
        for _ in range(cg_iters):
            if rs <= 1e-24 * rs0:
                break
            hp = hess(p) + lam * p
            alpha = rs / dot(p, hp)
            delta = delta + alpha * p
            res = res - alpha * hp
            rs_new = dot(res, res)
            p = res + (rs_new / rs) * p
            rs = rs_new
        scan = scan + delta
        after.append(scan.detach().cpu().numpy().copy())
    r = forward(scan) - data
    costs.append(0.5 * dot(r, r))
    return after, costs
