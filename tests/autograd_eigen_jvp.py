"""Float64 model of the forward-mode derivative of
`tike_amd.autograd.intensity` with eigen probes (test infrastructure), on
`autograd_eigen.varying_probe` / `farplane`, `autograd_model._taps` /
`patches` and `autograd_jvp._padded` / `inner`:

    P[n,s]  = w[n,0,s] probe[s] + sum_c w[n,c+1,s] E[c,s]            (s < M)
    dP[n,s] = w[n,0,s] d_probe[s] + d_w[n,0,s] probe[s]
            + sum_c (w[n,c+1,s] d_E[c,s] + d_w[n,c+1,s] E[c,s])      (s < M)
    dpatch_n   = patch_n(d_psi) + d_scan[n,0] Dy_n(psi) + d_scan[n,1] Dx_n(psi)
    dwave[n,s] = dpatch_n P[n,s] + patch_n(psi) dP[n,s]
    dfar[n,s]  = F pad(dwave[n,s])
    dI[f]      = sum_{n in frame f} sum_s 2 Re(conj(far[n,s]) dfar[n,s])

The varying probe is linear in (probe, E) and in w, so dP is
`varying_probe(d_probe, d_E, w) + varying_probe(probe, E, d_w)`.
`hand_jvp` is that in float64 (`tangent_nearplane`: the lines up to dwave,
padded), `hand_jvp_float32` the same formulas in float32 / complex64 on the
CPU -- what float32 alone costs --, `case` seeded inputs with five tangents,
and `joint_gauss_newton` the damped Gauss-Newton iteration on (positions,
eigen weights) jointly that the CPU and the GPU tests run: the CG of
`autograd_jvp.gauss_newton` on a tuple of tensors.
"""
import functools

import numpy as np
import torch

import autograd_eigen as ae
import autograd_jvp as aj
import autograd_model as am

TANGENT_NAMES = ("d_psi", "d_probe", "d_scan", "d_eigen", "d_weights")
# each tangent alone, all five, and (for the entry) none
TANGENTS = [(k,) for k in TANGENT_NAMES] + [TANGENT_NAMES]


def _tangent_wave(psi, probe, scan, eigen, weights, d_psi, d_probe, d_scan,
                  d_eigen, d_weights):
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
    dwave = dpatch[:, None] * ae.varying_probe(probe, eigen, weights)
    dP = None
    if d_probe is not None or (d_eigen is not None and eigen is not None):
        zero = lambda x: None if x is None else torch.zeros_like(x)
        dP = ae.varying_probe(
            zero(probe) if d_probe is None else d_probe,
            zero(eigen) if d_eigen is None else d_eigen, weights)
    if d_weights is not None:
        other = ae.varying_probe(probe, eigen, d_weights)
        dP = other if dP is None else dP + other
    if dP is not None:
        dwave = dwave + am.patches(psi, scan, pw)[:, None] * dP
    return dwave


def tangent_nearplane(psi, probe, scan, eigen, weights, det, d_psi=None,
                      d_probe=None, d_scan=None, d_eigen=None, d_weights=None):
    """pad(dwave) (N, S, det, det) complex128: what `tike_eigen_wave_tangent`
    writes."""
    with torch.no_grad():
        return aj._padded(_tangent_wave(psi, probe, scan, eigen, weights,
                                        d_psi, d_probe, d_scan, d_eigen,
                                        d_weights), det)


def _frames(x, N, fly, det):
    return x.sum(dim=1).reshape(N // fly, fly, det, det).sum(dim=1)


def hand_jvp(psi, probe, scan, eigen, weights, det, d_psi=None, d_probe=None,
             d_scan=None, d_eigen=None, d_weights=None, fly=1, norm="ortho"):
    """(I, dI) float64 (N // fly, det, det), no autograd."""
    with torch.no_grad():
        N = scan.shape[0]
        far = ae.farplane(psi, probe, scan, eigen, weights, det, norm)
        dfar = torch.fft.fft2(
            tangent_nearplane(psi, probe, scan, eigen, weights, det, d_psi,
                              d_probe, d_scan, d_eigen, d_weights), norm=norm)
        return (_frames(far.real**2 + far.imag**2, N, fly, det),
                _frames(2 * (far.conj() * dfar).real, N, fly, det))


def hand_jvp_float32(psi, probe, scan, eigen, weights, det, d_psi=None,
                     d_probe=None, d_scan=None, d_eigen=None, d_weights=None,
                     fly=1, norm="ortho"):
    """`hand_jvp` with every array complex64 / float32 (float64 model tensors
    in, rounded first): the same formulas at the kernels' precision."""
    low = lambda x: None if x is None else x.to(
        torch.complex64 if x.is_complex() else torch.float32)
    (psi, probe, scan, eigen, weights, d_psi, d_probe, d_scan, d_eigen,
     d_weights) = map(low, (psi, probe, scan, eigen, weights, d_psi, d_probe,
                            d_scan, d_eigen, d_weights))
    with torch.no_grad():
        N = scan.shape[0]
        far = ae.farplane(psi, probe, scan, eigen, weights, det, norm)
        dfar = torch.fft.fft2(aj._padded(_tangent_wave(
            psi, probe, scan, eigen, weights, d_psi, d_probe, d_scan, d_eigen,
            d_weights), det), norm=norm)
        assert far.dtype == dfar.dtype == torch.complex64
        return (_frames(far.real**2 + far.imag**2, N, fly, det),
                _frames(2 * (far.real * dfar.real + far.imag * dfar.imag), N,
                        fly, det))


# ------------------------------------------------------------------ the inputs
def tangents(c, seed):
    """Seeded host tangents of the five inputs of an `autograd_eigen.inputs`
    case (d_eigen None for C = 0): complex normal for the object and the
    probe, 0.3 x complex normal for the eigen probes, normal for the positions
    and 0.5 normal for the weights."""
    rng = np.random.default_rng(seed)
    return dict(
        d_psi=ae.rc(rng, *c["psi"].shape), d_probe=ae.rc(rng, *c["probe"].shape),
        d_scan=rng.standard_normal(c["scan"].shape).astype(np.float32),
        d_eigen=None if c["eigen"] is None else (
            0.3 * ae.rc(rng, *c["eigen"].shape)).astype(np.complex64),
        d_weights=(0.5 * rng.standard_normal(c["weights"].shape)).astype(
            np.float32))


def model_tangents(c, names=TANGENT_NAMES):
    """{name: float64 tensor or None} of a case's tangents; those not in
    `names` (and d_eigen for C = 0) are None."""
    return {k: ae.t128(c[k]) if k in names else None for k in TANGENT_NAMES}


@functools.lru_cache(maxsize=None)
def case(N, S, M, C, pw, det, H, fly, norm="ortho"):
    """`autograd_eigen.case` (inputs, the model's intensity) with the five
    seeded tangents, a random signed u (N // fly, det, det) and the model's
    dI along all five -- computed once, shared, left unchanged."""
    c = dict(ae.case(N, S, M, C, pw, det, H, fly, norm))
    c.update(tangents(c, seed=17 + N + 3 * S + 5 * det))
    c["u"] = np.random.default_rng(23 + N + det).standard_normal(
        (N // fly, det, det)).astype(np.float32)
    inten, tangent = hand_jvp(*ae.model_of(c), det, fly=fly, norm=norm,
                              **model_tangents(c))
    assert np.array_equal(inten.numpy(), c["intensity"])
    c["tangent"] = tangent.numpy()
    return c


# ----------------------------------- Gauss-Newton on positions and weights
def joint_gauss_newton(forward, jv, jtu, data, start, steps=4, cg_iters=20,
                       damping=1e-3):
    """Levenberg-Marquardt on a TUPLE of parameter tensors x = (scan, weights)
    with r = I - data: `steps` times solve (J^T J + D) delta = -J^T r by at
    most `cg_iters` conjugate-gradient iterations from zero and step by delta.
    D damps every parameter group by its own lam_k = damping * mean|(J^T J 1)_k|
    (the groups have different units: one lam for both would leave the group
    of the smaller curvature to the damping alone).  forward(x) -> I,
    jv(x, v) -> J v, jtu(x, u) -> J^T u as a tuple like x; tensors of one
    dtype and device.  The inner products are float64 sums over all groups.
    Returns ([x after every step, tuples of host arrays], [cost 0.5 |r|^2
    before every step and after the last])."""
    one = lambda a, b: float((a.double() * b.double()).sum())
    dot = lambda a, b: sum(one(x, y) for x, y in zip(a, b))
    axpy = lambda a, x, y: tuple(a * p + q for p, q in zip(x, y))
    x = tuple(t.detach().clone() for t in start)
    after, costs = [], []
    for _ in range(steps):
        r = forward(x) - data
        costs.append(0.5 * one(r, r))
        hess = lambda v: jtu(x, jv(x, v))
        lam = tuple(damping * float(h.abs().mean())
                    for h in hess(tuple(torch.ones_like(t) for t in x)))
        b = tuple(-g for g in jtu(x, r))
        delta = tuple(torch.zeros_like(t) for t in x)
        res, p = tuple(t.clone() for t in b), tuple(t.clone() for t in b)
        rs0 = rs = dot(res, res)
        for _ in range(cg_iters):
            if rs <= 1e-24 * rs0:
                break
            hp = tuple(h + l * q for h, l, q in zip(hess(p), lam, p))
            alpha = rs / dot(p, hp)
            delta = axpy(alpha, p, delta)
            res = axpy(-alpha, hp, res)
            rs_new = dot(res, res)
            p = axpy(rs_new / rs, p, res)
            rs = rs_new
        x = tuple(t + d for t, d in zip(x, delta))
        after.append(tuple(t.detach().cpu().numpy().copy() for t in x))
    r = forward(x) - data
    costs.append(0.5 * one(r, r))
    return after, costs


@functools.lru_cache(maxsize=None)
def recovery_problem():
    """`autograd_eigen.problem()` with fly = 1 data: the same object, probe,
    eigen probe, positions and weights, every position exposing its own frame.
    At the problem's own fly = 2 the joint problem is degenerate in the
    float64 model itself: the eigen probe is the probe times the column
    coordinate -- to first order a sideways shift of the probe, which the
    intensity cannot tell from a shift of the position --, and with two
    positions and two weights behind every frame four steps bring the cost
    down by 300 while the positions go from 0.243 px to 0.217 px only (and,
    with the groups preconditioned, AWAY to 0.40 px at a lower cost still).
    With a frame per position ten steps reach 0.11 px and go on falling.
    Computed once, shared, left unchanged."""
    p = dict(ae.problem())
    p["fly"] = 1
    with torch.no_grad():
        p["data"] = ae.intensity(
            ae.t128(p["psi"]), ae.t128(p["probe"]), ae.t128(p["scan_true"]),
            ae.t128(p["eigen"]), ae.t128(p["weights_true"]), p["det"],
            1).numpy().astype(np.float32)
    return p


JOINT_RECOVERY = dict(
    # after four steps of `joint_recovery_model(recovery_problem())`:
    # position RMS (px) and weights RMS, float64 and float32 on the CPU
    rms64=0.16285397267094412, rms32=0.16285409994929811,
    wrms64=0.010376283963667009, wrms32=0.01037634465724134)
"""The figures test_autograd_eigen_jvp_cpu.py reproduces and the GPU test is
bounded by: the float64 result plus twice the deviation of the float32 run
from it (`joint_recovery_bounds`)."""


def joint_recovery_bounds():
    """(position RMS, weights RMS) the GPU run may end at: what the float64
    model reaches, plus the deviation of the float32 restatement from it,
    doubled."""
    j = JOINT_RECOVERY
    return (j["rms64"] + 2 * abs(j["rms32"] - j["rms64"]),
            j["wrms64"] + 2 * abs(j["wrms32"] - j["wrms64"]))


def joint_recovery_model(p, single=False):
    """The joint iteration on the CPU model of the recovery problem `p`
    (`recovery_problem()`): J v by `hand_jvp` and J^T u by
    `autograd_eigen.hand_gradients` in float64, or -- single -- by
    `hand_jvp_float32` and `hand_gradients(single=True)`, with float32
    parameters and residuals.  Returns (after, costs) of
    `joint_gauss_newton`."""
    det, fly = p["det"], p["fly"]
    psi, probe, eigen = (ae.t128(p[k]) for k in ("psi", "probe", "eigen"))
    ft = torch.float32 if single else am.F64
    data = torch.from_numpy(p["data"]).to(ft)
    start = (torch.from_numpy(p["scan_start"]).to(ft),
             torch.from_numpy(p["weights_start"]).to(ft))
    run = hand_jvp_float32 if single else hand_jvp
    wide = lambda t: t.to(am.F64)

    def forward(x):
        return run(psi, probe, wide(x[0]), eigen, wide(x[1]), det,
                   fly=fly)[0].to(ft)

    def jv(x, v):
        return run(psi, probe, wide(x[0]), eigen, wide(x[1]), det,
                   d_scan=wide(v[0]), d_weights=wide(v[1]), fly=fly)[1].to(ft)

    def jtu(x, u):
        g = ae.hand_gradients(psi, probe, wide(x[0]), eigen, wide(x[1]), det,
                              wide(u), fly, single=single)
        return g["scan"].to(ft), g["weights"].to(ft)

    return joint_gauss_newton(forward, jv, jtu, data, start)
