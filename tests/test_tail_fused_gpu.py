"""The fused minibatch tail (one rank, one eigen probe: pass 2 leaves the
per-position part of the eigen projection, the step statistics and the eigen
position sums are one pass) against the staged packed tail it replaces."""
import numpy as np
import pytest

from util import assert_close

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tp():
    import tike_amd.ptycho as m
    return m


def _headline_problem(tp, det, S, N, seed, pitch=7.0, margin=8):
    """A small problem of the c3 kind: S modes and one eigen probe on the
    first mode, positions on a jittered raster inside the object."""
    import tike_amd.random
    rng = np.random.default_rng(seed)
    pw = det
    side = int(np.ceil(np.sqrt(N)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side),
                              indexing="ij"), -1).reshape(-1, 2)[:N]
    scan = (2 + pitch * ij + rng.random((N, 2))).astype(np.float32)
    HW = int(pitch * (side - 1)) + pw + margin
    psi_true = ((0.75 + 0.25 * rng.random((1, HW, HW))) * np.exp(
        1j * np.pi * (rng.random((1, HW, HW)) - 0.5))).astype(np.complex64)
    w = tp.gaussian(pw, rin=0.6)
    probe = np.stack([w * np.exp(1j * np.pi * rng.random((pw, pw))) / (m + 1)
                      for m in range(S)])[None, None].astype(np.complex64)
    np.random.seed(seed)
    tike_amd.random.randomizer_np = np.random.default_rng(seed + 1)
    ep, ew = tp.init_varying_probe(scan, probe, num_eigen_probes=2,
                                   probes_with_modes=1)
    ew[:, 1, 0] = 0.05 * rng.standard_normal(N).astype(np.float32)
    data = tp.simulate(det, probe, scan, psi_true, eigen_probe=ep,
                       eigen_weights=ew)
    probe0 = (probe * (1 + 0.05 * rng.standard_normal(probe.shape))).astype(
        np.complex64)
    return scan, psi_true, probe0, ep, ew, data


def _epoch(tp, problem, det, num_batch, fused, monkeypatch):
    """One lstsq epoch (the bench's update rule); the route the tail took."""
    import tike_amd.random
    from tike_amd.ptycho.solvers import lstsq as L
    scan, psi_true, probe0, ep, ew, data = problem
    N = len(scan)
    monkeypatch.setattr(L, "FUSED_TAIL", fused)
    taken = []
    real = L._fused_tail
    monkeypatch.setattr(L, "_fused_tail",
                        lambda *a, **k: (taken.append(1), real(*a, **k))[1])
    params = tp.PtychoParameters(
        probe=probe0.copy(), psi=np.full_like(psi_true, 0.5),
        scan=scan.copy(), eigen_probe=ep.copy(), eigen_weights=ew.copy(),
        algorithm_options=tp.LstsqOptions(num_batch=num_batch, num_iter=1,
                                          batch_method="wobbly_center"),
        probe_options=tp.ProbeOptions(force_orthogonality=True),
        object_options=tp.ObjectOptions(),
        exitwave_options=tp.ExitWaveOptions(
            measured_pixels=np.ones((det, det), dtype=bool)))
    tike_amd.random.randomizer_np = np.random.default_rng(11)
    with tp.Reconstruction(data, params, order=np.arange(N),
                           batches=np.array_split(np.arange(N), num_batch),
                           spatial_sort=True) as ctx:
        ctx.iterate(1)
        got = ctx.get_result()
    return got, len(taken)


@pytest.mark.parametrize("det,S,N,num_batch", [
    (256, 8, 20, 2),   # the c3 shape: 8 modes + one eigen probe
    (256, 8, 21, 2),   # an odd minibatch: its last position takes the fallback
    (128, 8, 18, 2),
    (256, 4, 13, 1),
    (128, 8, 300, 1),  # above 256 positions: a second round of every
                       # one-workgroup loop over the minibatch
])
def test_fused_tail_equals_staged_tail(tp, det, S, N, num_batch, monkeypatch):
    problem = _headline_problem(tp, det, S, N, seed=det + S + N)
    staged, n_staged = _epoch(tp, problem, det, num_batch, False, monkeypatch)
    fused, n_fused = _epoch(tp, problem, det, num_batch, True, monkeypatch)
    assert n_staged == 0 and n_fused in (0, num_batch)
    if det == 256 or N > 256:  # the fused pass 2 of the c3 route
        assert n_fused == num_batch
    np.testing.assert_allclose(np.array(fused.algorithm_options.costs),
                               np.array(staged.algorithm_options.costs),
                               rtol=1e-5)
    for name in ("psi", "probe", "eigen_probe", "eigen_weights"):
        assert_close(getattr(fused, name), getattr(staged, name),
                     normwise=1e-5, maxabs=1e-4, what=name)


def test_fused_tail_minibatch_quantities(tp, monkeypatch):
    """The first minibatch: eigen_proj, the updated eigen probe and weights,
    and both step lengths of the two tails from the same gradients."""
    import torch
    from tike_amd.ptycho.solvers import lstsq as L
    det, S, N = 256, 8, 24
    problem = _headline_problem(tp, det, S, N, seed=5)
    seen = {}

    def spy(fused):
        real_packed = L._packed_tail

        def wrapped(g, psi, scan, probe, eigen_probe, eigen_weights, *a, **k):
            out = real_packed(g, psi, scan, probe, eigen_probe, eigen_weights,
                              *a, **k)
            if "first" not in seen.setdefault(fused, {}):
                lo, hi = a[1], a[2]
                torch.cuda.synchronize()
                seen[fused] = dict(
                    first=True,
                    eproj=g["eigen_proj"].clone().cpu().numpy(),
                    E=eigen_probe.clone().cpu().numpy(),
                    w=eigen_weights[lo:hi].clone().cpu().numpy(),
                    steps=k["steps_row"].clone().cpu().numpy())
            return out
        return wrapped

    for fused in (False, True):
        monkeypatch.setattr(L, "_packed_tail", spy(fused))
        _epoch(tp, problem, det, 1, fused, monkeypatch)
    a, b = seen[False], seen[True]
    for name in ("eproj", "E", "w", "steps"):
        assert_close(b[name], a[name], normwise=1e-5, maxabs=1e-4, what=name)
