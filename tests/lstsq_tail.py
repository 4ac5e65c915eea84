"""A float64 / complex128 model of the lstsq_grad minibatch tail, entry by
entry: the 2x2 step-length solves, the probe update, the eigen-probe update and
the eigen weights (everything between a minibatch's gradients and the next
forward pass).  NumPy only.  Each function restates ONE entry of
include/tike_amd.h from that header's formulas and the reference lines it cites
(lstsq.py:136-205, 297-364, 605-761; probe.py:362-476) -- not from the kernels:
the solves are written in complex form, the eigen probe is normalised the
direct way (two norms, no expanded quadratic), and sums are plain `np.sum`.
tests/test_lstsq_tail_cpu.py pins this model against oracle/solvers.py;
tests/test_lstsq_tail_gpu.py holds every HIP entry of the tail to it.

Shapes: stats (B, 8) and sums5 (B, 5) as the header lays them out; patches
O, chi0, G (B, pw, pw); probe, mpu (S, pw, pw); E (pw, pw); weights
(B, C + 1, S).  Nothing is modified in place: every function returns new
arrays."""
import contextlib

import numpy as np

F8 = np.float64
C16 = np.complex128


def f8(x):
    return np.asarray(x, dtype=F8)


def c16(x):
    return np.asarray(x, dtype=C16)


def mnorm(x):
    """sqrt(mean |x|^2) (linalg.py:12-18)."""
    x = c16(x)
    return np.sqrt(np.mean((x * np.conj(x)).real))


def _tot(a):
    return a.reshape(a.shape[0], -1).sum(axis=1)


# ------------------------------------------------------------ the 2x2 solves
def step_sums(stats, costs, eps):
    """tike_lstsq_step_sums: { sum (A1 + eps), sum (A4 + eps), sum costs }
    (costs None: 0) over the rows of stats."""
    stats = f8(stats).reshape(-1, 8)
    return np.array([np.sum(stats[:, 0] + eps), np.sum(stats[:, 1] + eps),
                     0.0 if costs is None else np.sum(f8(costs))], dtype=F8)


def solve(stats, eps, sums, count, recover_psi, recover_probe):
    """The per-position solutions (x1, x2) of lstsq.py:666-700, complex as the
    reference forms them; `sums` and `count` span all ranks."""
    stats = f8(stats).reshape(-1, 8)
    sums = f8(sums)
    A1 = stats[:, 0] + eps + 0.5 * sums[0] / count
    A4 = stats[:, 1] + eps + 0.5 * sums[1] / count
    b1, b2 = stats[:, 4], stats[:, 5]
    x1 = np.zeros(len(stats), dtype=C16)
    x2 = np.zeros(len(stats), dtype=C16)
    if recover_psi and recover_probe:
        A2 = stats[:, 2] + 1j * stats[:, 3]
        A3 = np.conj(A2)
        det = A1 * A4 - A2 * A3
        x1 = -np.conj(A2 * b2 - A4 * b1) / det
        x2 = np.conj(A1 * b2 - A3 * b1) / det
    elif recover_psi:
        x1 = (b1 / A1).astype(C16)
    elif recover_probe:
        x2 = (b2 / A4).astype(C16)
    return x1, x2


def step_lengths(stats, eps, sums, count, recover_psi, recover_probe):
    """0.9 max(0, Re x) per position, both directions (lstsq.py:702-718)."""
    x1, x2 = solve(stats, eps, sums, count, recover_psi, recover_probe)
    return 0.9 * np.maximum(0.0, x1.real), 0.9 * np.maximum(0.0, x2.real)


def step_solve(stats, eps, sums, count, recover_psi, recover_probe):
    """tike_lstsq_step_solve: { sum step_o, sum step_p, beta_o, beta_p, mean
    cost } with the sums over the local rows and the means over `count`."""
    so, sp = step_lengths(stats, eps, sums, count, recover_psi, recover_probe)
    so, sp = np.sum(so), np.sum(sp)
    return np.array([so, sp, so / count, sp / count, f8(sums)[2] / count],
                    dtype=F8)


# ------------------------------------------------- object and probe updates
def object_update_precond(acc_planar, precond, pmax, alpha):
    """tike_object_update_precond (lstsq.py:605-616): (upd_sum, upd_precond)
    from the planar accumulator (2, npix); `combined` gains acc_planar."""
    acc = f8(acc_planar)
    g = acc[0] + 1j * acc[1]
    den = np.sqrt(np.square((1.0 - alpha) * c16(precond).real) +
                  np.square(alpha * float(pmax)))
    return g, g / den


def probe_update(probe, combined, mpu, beta, inv_num_batch):
    """tike_probe_update (lstsq.py:177-181): (probe, combined) afterwards."""
    d = float(beta) * c16(mpu)
    return (c16(probe) + d,
            None if combined is None else c16(combined) + d * inv_num_batch)


# --------------------------------------------------- eigen-probe bookkeeping
def eigen_weights0(weights, stats, m):
    """tike_eigen_weights0 (lstsq.py:721-738, probe.py:417-424): the weights
    with [n][0][m] += 0.1 stats6 / stats7, and norms[c - 1] = sum_n
    weights[n][c][m]^2."""
    w = f8(weights).copy()
    stats = f8(stats).reshape(-1, 8)
    w[:, 0, m] += 0.1 * stats[:, 6] / stats[:, 7]
    return w, np.sum(np.square(w[:, 1:, m]), axis=0)


def eigen_proj_mean(first, weights_c, norm, P):
    """tike_eigen_proj_mean (probe.py:429-433): the mean over pixels of
    (Re(conj(R) E) + w) / norm."""
    return (f8(first) / P + f8(weights_c)) / float(norm)


def eigen_normalise(E, update, count, beta):
    """tike_eigen_normalise (probe.py:440-448): (E', sum |E'|^2)."""
    u = c16(update) / count
    E = c16(E) + beta * u / mnorm(u)
    E = E / mnorm(E)
    return E, np.sum(np.abs(E)**2)


def eigen_dsum(sums5, P):
    """tike_eigen_dsum: sum_n sums5[n][2] / P."""
    return np.sum(f8(sums5).reshape(-1, 5)[:, 2] / P)


def eigen_weights(sums5, P, dsum, count, weights_c, esum=None):
    """tike_eigen_weights (probe.py:450-476, lstsq.py:740-761): (weights_c
    afterwards, projection coefficients or None)."""
    s = f8(sums5).reshape(-1, 5)
    w = f8(weights_c) + (s[:, 1] / P) / (s[:, 2] / P + 0.1 * dsum / count)
    coefs = None if esum is None else (s[:, 3] + 1j * s[:, 4]) / float(esum)
    return w, coefs


# ------------------------------------------------- the per-position passes
def residual(patches, chi0, mpu0):
    """R_n = conj(O_n) chi_n,0 - m_probe_update_0 (lstsq.py:318-322)."""
    return np.conj(c16(patches)) * c16(chi0) - c16(mpu0)


def eigen_proj(patches, chi0, mpu0, E):
    """sum_p Re(conj(R_n) E): the eigen_proj of tike_lstsq_step_stats."""
    return _tot((np.conj(residual(patches, chi0, mpu0)) * c16(E)).real)


def q_of(patches, chi0, E):
    """q[n] = sum_p Re(conj(O_n) chi_n,0 conj(E))."""
    return _tot((np.conj(c16(patches)) * c16(chi0) * np.conj(c16(E))).real)


def eigen_proj_from_q(q, mpu0, E):
    """eigen_proj[n] = q[n] - sum_p Re(mpu_0 conj(E_0))."""
    return f8(q) - np.sum((c16(mpu0) * np.conj(c16(E))).real)


def pixel_update1(update, patches, chi0, mpu0, eigen_proj, weights_c, norm):
    """tike_eigen_pixel_update1: update + sum_n R_n pm[n], pm formed from
    eigen_proj (probe.py:429-436, before the mean over positions)."""
    R = residual(patches, chi0, mpu0)
    P = R.shape[-1] * R.shape[-2]
    pm = eigen_proj_mean(eigen_proj, weights_c, norm, P)
    return c16(update) + np.sum(R * pm[:, None, None], axis=0)


def step_stats(G, O, chi0, P0, Pn, mpu0):
    """tike_lstsq_step_stats (lstsq.py:641-694, 721-738): G_n the patches of
    the preconditioned object update, Pn (B, pw, pw) the varying probe of
    mode 0 (or P0 broadcast)."""
    G, O, chi0 = c16(G), c16(O), c16(chi0)
    dOP = G * c16(Pn)
    dPO = c16(mpu0) * O
    OP = O * c16(P0)
    a2 = _tot(dOP * np.conj(dPO))
    return np.stack([_tot(np.abs(dOP)**2), _tot(np.abs(dPO)**2), a2.real,
                     a2.imag, _tot((np.conj(dOP) * chi0).real),
                     _tot((np.conj(dPO) * chi0).real),
                     _tot((np.conj(OP) * chi0).real), _tot(np.abs(OP)**2)], 1)


def position_sums5(O, chi0, mpu0, E):
    """tike_eigen_position_sums (probe.py:437-469): { sum Re(conj(R) E),
    sum Re(chi0 conj(O E)), sum |O E|^2, Re / Im sum R conj(E) }."""
    O, chi0, E = c16(O), c16(chi0), c16(E)
    R = residual(O, chi0, mpu0)
    phi = O * E
    re = _tot(R * np.conj(E))
    return np.stack([_tot((np.conj(R) * E).real),
                     _tot((chi0 * np.conj(phi)).real), _tot(np.abs(phi)**2),
                     re.real, re.imag], 1)


def norm_sums(E, update):
    """nacc = { sum |update|^2, sum |E|^2, sum Re(conj(E) update) }."""
    E, u = c16(E), c16(update)
    return np.array([np.sum(np.abs(u)**2), np.sum(np.abs(E)**2),
                     np.sum((np.conj(E) * u).real)], dtype=F8)


# ------------------------------------------------------------ compositions
def tail_mid(E, update, beta_eigen, stats, eps, sums3, count, recover_psi,
             recover_probe):
    """tike_lstsq_tail_mid: dict(tail=(sum step_o, sum step_p), nacc, E)."""
    out = dict(tail=step_solve(stats, eps, sums3, count, recover_psi,
                               recover_probe)[:2], nacc=None, E=None)
    if E is not None:
        out["nacc"] = norm_sums(E, update)
        out["E"] = eigen_normalise(E, update, count, beta_eigen)[0]
    return out


def tail_solve1(E, update, beta_eigen, stats, costs, sums5, eps, count,
                recover_psi, recover_probe):
    """tike_lstsq_tail_solve1: dict(E, sums3, tail3)."""
    sums3 = step_sums(stats, costs, eps)
    tail = step_solve(stats, eps, sums3, count, recover_psi, recover_probe)
    E1 = eigen_normalise(E, update, count, beta_eigen)[0]
    return dict(E=E1, sums3=sums3,
                tail3=np.array([tail[0], tail[1],
                                eigen_dsum(sums5, E1.size)], dtype=F8))


def tail_finish(tail3, sums3, count, probe, combined, mpu, inv_num_batch,
                weights, m, stats, sums5, npix):
    """tike_lstsq_tail_finish: dict(steps, probe, combined, weights)."""
    tail3, sums3 = f8(tail3), f8(sums3)
    steps = np.array([tail3[0], tail3[1], tail3[0] / count, tail3[1] / count,
                      sums3[2] / count], dtype=F8)
    out = dict(steps=steps, probe=None, combined=None, weights=None)
    if probe is not None:
        out["probe"], out["combined"] = probe_update(probe, combined, mpu,
                                                     steps[3], inv_num_batch)
    if weights is not None:
        w, _ = eigen_weights0(weights, stats, m)
        if sums5 is not None:
            w[:, 1, m], _ = eigen_weights(sums5, npix, tail3[2], count,
                                          w[:, 1, m])
        out["weights"] = w
    return out


def packed_tail(stats, costs, O, chi0, mpu, E, weights, norm, probe, combined,
                *, eps, count, num_batch, recover_psi, recover_probe, m=0):
    """The packed form (_packed_tail) of one rank holding the whole minibatch:
    step statistics given, then tike_eigen_pixel_update1 (or
    tike_lstsq_step_sums), tike_lstsq_tail_mid, tike_eigen_position_sums1,
    tike_lstsq_tail_finish.  E None: no eigen probe; weights None: none kept."""
    beta_eigen = min(0.1, 1.0 / num_batch)
    sums3 = step_sums(stats, costs, eps)
    update = sums5 = None
    tail3 = np.zeros(3, dtype=F8)
    if E is not None:
        mpu0 = c16(mpu)[m]
        update = pixel_update1(np.zeros(np.shape(E), dtype=C16), O, chi0, mpu0,
                               eigen_proj(O, chi0, mpu0, E),
                               f8(weights)[:, 1, m], norm)
    mid = tail_mid(E, update, beta_eigen, stats, eps, sums3, count,
                   recover_psi, recover_probe)
    tail3[:2] = mid["tail"]
    if E is not None:
        sums5 = position_sums5(O, chi0, mpu0, mid["E"])
        tail3[2] = eigen_dsum(sums5, mid["E"].size)
    fin = tail_finish(tail3, sums3, count, probe if recover_probe else None,
                      combined, mpu, 1.0 / num_batch, weights, m, stats, sums5,
                      None if E is None else mid["E"].size)
    return dict(fin, E=mid["E"], update=update, sums3=sums3, tail3=tail3,
                sums5=sums5, nacc=mid["nacc"])


def fused_tail(G, O, chi0, mpu, E, weights, norm, probe, combined, costs, *,
               eps, count, num_batch, recover_psi, recover_probe, m=0):
    """The fused form (_fused_tail): q from pass 2, tike_eigen_pixel_update1q,
    tike_lstsq_step_stats_eigen1 (statistics with the OLD eigen probe in the
    varying probe, sums5 against the new one), tike_lstsq_tail_solve1,
    tike_lstsq_tail_finish."""
    beta_eigen = min(0.1, 1.0 / num_batch)
    mpu0, P0, w = c16(mpu)[m], c16(probe)[m], f8(weights)
    eproj = eigen_proj_from_q(q_of(O, chi0, E), mpu0, E)
    update = pixel_update1(np.zeros(np.shape(E), dtype=C16), O, chi0, mpu0,
                           eproj, w[:, 1, m], norm)
    nacc = norm_sums(E, update)
    E1 = eigen_normalise(E, update, count, beta_eigen)[0]
    Pn = w[:, 0, m, None, None] * P0 + w[:, 1, m, None, None] * c16(E)
    stats = step_stats(G, O, chi0, P0, Pn, mpu0)
    sums5 = position_sums5(O, chi0, mpu0, E1)
    s1 = tail_solve1(E, update, beta_eigen, stats, costs, sums5, eps, count,
                     recover_psi, recover_probe)
    fin = tail_finish(s1["tail3"], s1["sums3"], count,
                      probe if recover_probe else None, combined, mpu,
                      1.0 / num_batch, weights, m, stats, sums5, E1.size)
    return dict(fin, E=s1["E"], update=update, sums3=s1["sums3"],
                tail3=s1["tail3"], sums5=sums5, nacc=nacc, stats=stats,
                eigen_proj=eproj)


# --------------------------------------------- float32 restatements (bars)
@contextlib.contextmanager
def single_precision():
    """Inside: every function of this module evaluates the same formulas in
    float32 / complex64 -- the restatement the scalar bars are measured
    with."""
    global F8, C16
    F8, C16 = np.float32, np.complex64
    try:
        yield
    finally:
        F8, C16 = np.float64, np.complex128


def rel_max(got, want):
    """max |got - want| / max |want|: arrays whose elements share a scale."""
    got, want = np.asarray(got, C16_), np.asarray(want, C16_)
    assert got.shape == want.shape, (got.shape, want.shape)
    if want.size == 0:
        return 0.0
    den = np.abs(want).max()
    err = np.abs(got - want).max()
    if not np.isfinite(err):
        return np.inf
    return float(err / den) if den > 0 else (0.0 if err == 0 else np.inf)


def rel_each(got, want):
    """max over the elements of |got - want| / |want| (an element that must be
    zero must be zero): short lists of sums, each with a scale of its own."""
    got, want = np.asarray(got, C16_), np.asarray(want, C16_)
    assert got.shape == want.shape, (got.shape, want.shape)
    return max([rel_max(g, w) for g, w in zip(got.ravel(), want.ravel())],
               default=0.0)


C16_ = np.complex128


def float32_error(fn, *args, metric=rel_max, pick=None, **kwargs):
    """The metric between fn evaluated in float32 and in float64 on the same
    inputs, the largest over every array fn returns (or over pick(result);
    tuples and dicts are walked, None skipped): what a correct float32
    implementation of the formula may be off by on these inputs."""
    want = fn(*args, **kwargs)
    with single_precision():
        got = fn(*args, **kwargs)
    if pick is not None:
        got, want = pick(got), pick(want)
    return max([metric(g, w) for g, w in zip(_leaves(got), _leaves(want))],
               default=0.0)


def _leaves(x):
    if x is None:
        return []
    if isinstance(x, dict):
        return [l for k in sorted(x) for l in _leaves(x[k])]
    if isinstance(x, (tuple, list)):
        return [l for v in x for l in _leaves(v)]
    return [x]


def scalar_bar(measured):
    """The bar of the scalar arithmetic: 8 x the float32 restatement's own
    error on the same inputs (the margin covers another summation order over
    up to 1000 terms), and not below 1e-6."""
    return max(8.0 * float(measured), 1e-6)
