"""One launch past 4 GiB of far plane, and past 65 536 positions, on every
route of the lstsq minibatch, the fused operators, the transforms and the
launches that put a position count into gridDim.y -- checked POSITION BY
POSITION against the float64 model of tests/large_launch.py.

The batch is a base problem of n0 distinct positions repeated R times on the
device (large_launch.py explains why a wrapped index cannot hide in it); the
host model only ever sees the n0 base positions, and the comparison is reduced
on the device in slabs.  No chunk override: every case asserts that the plan
it ran put the whole batch into one launch.

Bars (those of `_minibatch_vs_oracle`, test_solvers_gpu.py): patches
OP_NORMWISE, chi0 and the gradients 2e-5 normwise, costs COST_RTOL -- per
position for the per-position outputs; for the accumulated outputs the same
bar plus the float32 accumulation bound (additions into the entry) x 2^-24 x
sum |terms| from the float64 model."""
import contextlib
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import large_launch as ll
from util import COST_RTOL, OP_NORMWISE

pytestmark = pytest.mark.gpu

GRAD_BAR = 2e-5
ROUTES_RUN = set()
REPORT = []  # (test, seconds, need in GiB): printed by the closing test


# ------------------------------------------------------------------ helpers
def _need_or_skip(need_bytes, what):
    """Skip only when the card cannot hold 1.25 x the case's need."""
    import torch
    free = torch.cuda.mem_get_info()[0]
    print(f"{what}: needs {need_bytes / 2**30:.2f} GiB, "
          f"{free / 2**30:.1f} GiB free")
    if free < 1.25 * need_bytes:
        pytest.skip(f"{what}: {need_bytes / 2**30:.2f} GiB needed x 1.25, "
                    f"{free / 2**30:.2f} GiB free")


@contextlib.contextmanager
def _measured(name, need_bytes):
    import torch
    t0 = time.perf_counter()
    try:
        yield
    finally:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        REPORT.append((name, time.perf_counter() - t0, need_bytes / 2**30))
        print(f"{name}: {REPORT[-1][1]:.2f} s")


@contextlib.contextmanager
def _switches(module, **values):
    saved = {k: getattr(module, k) for k in values}
    for k, v in values.items():
        setattr(module, k, v)
    try:
        yield
    finally:
        for k, v in saved.items():
            setattr(module, k, v)


class _Sizes:
    """Stands in for the workspace: records what `GradientPlan.buffers` would
    allocate (shapes only, on the meta device)."""

    def __init__(self):
        self.bytes = {}

    def get(self, name, shape, dtype, device):
        import torch
        t = torch.empty(tuple(shape), dtype=dtype, device="meta")
        self.bytes[name] = max(self.bytes.get(name, 0),
                               t.numel() * t.element_size())
        return t


def _rep(a, R, dtype=None):
    """Host array (n0, ...) -> device tensor (R * n0, ...), repeated on the
    device."""
    import tike_amd._arrays as A
    t = A.to_device(a, dtype)
    return t.repeat(R, *([1] * (t.ndim - 1))).contiguous()


def _check_positions(got, want, n0, bar, what, fails):
    err, k, i = ll.worst(ll.position_errors(got, want, n0), n0)
    print(f"  {what}: worst per-position error {err:.3e} (bar {bar:.1e}) at "
          f"position {k} (base {i})")
    if not err <= bar:
        fails.append(f"{what}: {err:.3e} > {bar:.1e} at position {k}")
    return err


def _check_costs(got, want, n0, rtol, fails, what="costs"):
    import torch
    w = torch.from_numpy(np.asarray(want, np.float64)).to(got.device)
    rel = (got.to(torch.float64).reshape(-1, n0) - w).abs() / w.abs()
    err, k, i = ll.worst(rel.reshape(-1), n0)
    print(f"  {what}: worst per-position relative error {err:.3e} "
          f"(bar {rtol:.1e}) at position {k} (base {i})")
    if not err <= rtol:
        fails.append(f"{what}: {err:.3e} > {rtol:.1e} at position {k}")


def _check_accumulated(got, want, abs_terms, additions, bar, what, fails):
    bound = ll.accumulation_bound(abs_terms, additions)
    diff, ref, b = ll.accumulated_error(got, want, bound)
    depth = float(np.max(additions))
    print(f"  {what}: ||got - want|| / ||want|| = {diff / ref:.3e} (bar "
          f"{bar:.1e} + accumulation bound {b / ref:.3e}, depth {depth:.0f})")
    if not diff <= bar * ref + b:
        fails.append(f"{what}: {diff / ref:.3e} > {bar:.1e} + {b / ref:.3e}")
    excess = ll.entrywise_excess(got, want, bound, bar)
    print(f"  {what}: worst entry at {excess:.3e} of (bar x max|want| + its "
          f"own accumulation bound)")
    if not excess <= 1.0:
        fails.append(f"{what}: an entry at {excess:.3e} of its tolerance")


POLICY_MAX_POSITIONS = 1 << 22  # chunk_positions: 8 GiB of 16^2 far planes


def _grid_limit(unit=1):
    """The count just past which a wrapper takes a second slice: the device's
    gridDim.y limit as the library read it (`tike_max_grid_dim_y`) x `unit`
    positions per grid row.  Where the device reports a limit that no batch
    the chunk policy admits can reach, the launches are in range as they
    stand and the cases keep 65 536 rows."""
    from tike_amd._lib import lib
    limit = int(lib.tike_max_grid_dim_y())
    assert limit > 0, "hipDeviceAttributeMaxGridDimY could not be read"
    print(f"hipDeviceAttributeMaxGridDimY = {limit}")
    if limit * unit >= POLICY_MAX_POSITIONS:
        print("  ... beyond every admitted batch: no launch is ever sliced")
        return (1 << 16) * unit, ()
    return limit * unit, (limit,)


# ---------------------------------------------- one chunk of the minibatch
@functools.lru_cache(maxsize=None)
def _base_and_model(det, S, n0, u16_mask, noise):
    b = ll.base_problem(det, S, n0, seed=3 * det + S)
    mask = np.ones((det, det), dtype=bool)
    data = data_in = b["data"]
    if u16_mask:
        # uint16 counts + a mask whose unmeasured pixels hold garbage, as
        # test_resident_gradient_kernel_vs_oracle_beyond_one_wave builds them
        mask = np.random.default_rng(9).random((det, det)) > 0.1
        data = np.round(data * (20000.0 / data.max())).astype(np.uint16)
        data_in = data.copy()
        data_in[:, ~mask] = 65535  # never read: the mask selects
    m = ll.chunk_model(b["psi"], b["scan"], b["probe"], b["eigen"],
                       b["weights"], data.astype(np.float32), mask, det,
                       noise_model=noise)
    return b, mask, data_in, m


def _run_chunk_case(case):
    import torch
    import tike_amd._arrays as A
    import tike_amd.ptycho as tp
    from tike_amd import _lib
    from tike_amd.communicators import Comm
    from tike_amd.operators import Ptycho
    from tike_amd.ptycho.solvers import lstsq as L
    from tike_amd.ptycho.solvers._plan import GradientPlan

    det, S, n0, N = case["det"], case["S"], case["n0"], case["N"]
    counts = ()
    if case["axis"] == "count":  # just past the limit the device reports
        limit, counts = _grid_limit()
        N = ll.positions_for(1, n0, limit)
    R = N // n0
    noise = case.get("noise_model", "gaussian")
    want_route, expect = case["route"], dict(case.get("expect", {}))
    if _lib.DETERMINISTIC and noise == "poisson" and want_route == "no_farplane":
        # ordered sums: the per-mode steps come from a stored far plane
        # (_plan.py, `handoff_steps`), which is the split_kept route
        want_route, expect = "split_kept", {}
    strides, tiles = ll.case_strides(case)
    ll.assert_no_aliasing(strides, tiles, n0, counts)
    b, mask, data_in, m = _base_and_model(det, S, n0,
                                          bool(case.get("u16_mask")), noise)
    pw = b["pw"]
    HW = b["psi"].shape[-1]
    eo = tp.ExitWaveOptions(measured_pixels=mask, noise_model=noise)
    positions = bool(case.get("positions"))
    fails = []
    with _switches(L, **case.get("switches", {})), Ptycho(
            probe_shape=pw, detector_shape=det, nz=HW, n=HW) as op:
        assert not L.CHUNK_POSITIONS_OVERRIDE
        _, mask_u8 = L.mask_info(eo, det)
        plan = GradientPlan.for_(op, S, pw, det, eo, mask_u8, eigen_modes=1,
                                 num_eigen=1)
        assert plan.route == want_route, (plan.route, want_route)
        assert plan.chunk >= N, (plan.chunk, N)
        for k, v in expect.items():
            assert bool(getattr(plan, k)) == v, (k, getattr(plan, k))
        sizes = _Sizes()
        plan.buffers(sizes, N, torch.device("cuda"), varying=1,
                     want_patches=True)
        far_bytes = sizes.bytes["far"]
        assert far_bytes == N * strides["far / mid"], far_bytes
        if case["axis"] == "bytes":
            assert N * S * det * det * 8 > 1 << 32
        need = (sum(sizes.bytes.values()) + N * strides["data"] * 3 +
                4 * ll.SLAB_BYTES + (1 << 28))
        _need_or_skip(need, case["name"])
        with _measured(case["name"], need):
            out = d = data_d = pos_terms = None
            try:
                d = dict(psi=A.to_device(b["psi"]),
                         probe=A.to_device(b["probe"]),
                         ep=A.to_device(b["eigen"]),
                         scan=_rep(b["scan"], R), ew=_rep(b["weights"], R))
                if data_in.dtype == np.uint16:
                    # (torch repeats 16-bit signed, not unsigned, integers)
                    data_d = A.data_to_device(data_in).view(
                        torch.int16).repeat(R, 1, 1).view(torch.uint16)
                else:
                    data_d = _rep(data_in, R, np.float32)
                if positions:
                    pos_terms = (torch.full((N, 2), float("nan"),
                                            device=d["scan"].device),
                                 torch.full((N, 2), float("nan"),
                                            device=d["scan"].device))
                out = L._get_nearplane_gradients(
                    data_d, d["psi"], d["scan"], d["probe"], d["ep"], d["ew"],
                    0, N, Comm(), num_batch=1, exitwave_options=eo, op=op,
                    recover_psi=True, recover_probe=True,
                    position_terms=pos_terms)
                torch.cuda.synchronize()
                ROUTES_RUN.add(plan.route)
                print(f"{case['name']}: N = {N}, route {plan.route}, far "
                      f"plane {far_bytes / 2**30:.3f} GiB, launches "
                      f"{plan.launches}")
                _check_positions(out["patches"], m["patches"], n0,
                                 OP_NORMWISE, "patches", fails)
                chi0 = out["chi0"]
                if chi0.ndim == 5:  # one chunk of a route that stores chi
                    assert chi0.shape[2] == out["chi_modes"]
                    chi0 = chi0[:N, 0, 0]
                _check_positions(chi0, m["chi0"], n0, GRAD_BAR, "chi0", fails)
                _check_costs(out["costs"], m["costs"], n0, COST_RTOL, fails)
                # every position adds 4 bilinear taps to a pixel it covers;
                # the probe gradient is one sum over the N positions
                _check_accumulated(
                    L.object_upd_sum(out)[0], R * m["object_upd_sum"],
                    R * m["object_abs"], R * m["object_terms"], GRAD_BAR,
                    "object_upd_sum", fails)
                _check_accumulated(
                    out["m_probe_update"][0, 0], R * m["m_probe_update"],
                    R * m["m_probe_abs"], np.full(m["m_probe_abs"].shape, N),
                    GRAD_BAR, "m_probe_update", fails)
                if positions:
                    # (`_minibatch_vs_oracle`: rtol 2e-3, atol 1e-4 max|num|)
                    for t, key in zip(pos_terms, ("position_numerator",
                                                  "position_denominator")):
                        w = torch.from_numpy(m[key]).to(t.device)
                        assert bool(torch.isfinite(t).all()), key
                        err = (t.to(torch.float64).reshape(R, n0, 2) - w).abs()
                        tol = 2e-3 * w.abs() + (
                            1e-4 * float(np.abs(m[key]).max())
                            if key.endswith("numerator") else 0.0)
                        worst = float((err / tol).max())
                        print(f"  {key}: worst error / tolerance {worst:.3e}")
                        if not worst <= 1.0:
                            fails.append(f"{key}: {worst:.3e} x tolerance")
            finally:
                del out, d, data_d, pos_terms
                op.__dict__.pop("_tike_amd_workspace", None)
    assert not fails, fails


@pytest.mark.parametrize("case", ll.CHUNK_CASES,
                         ids=[c["name"] for c in ll.CHUNK_CASES])
def test_one_launch_of_the_minibatch_chunk(case):
    """`_get_nearplane_gradients` with no chunk override on a batch whose far
    plane spans more than 4 GiB (or more than 65 536 positions): the plan's
    route and chunk say one launch covered it; every position meets the
    bars."""
    from tike_amd import _lib
    if case.get("deterministic"):
        # the switch is a process-wide one, set at start-up: the case without
        # it once more in a child, as the other GPU modules switch it
        if _lib.DETERMINISTIC:
            return  # this is the child (or the whole suite under the switch)
        env = dict(os.environ, TIKE_DETERMINISTIC="1")
        twin = case["name"][:-len("-deterministic")]
        out = subprocess.run(
            [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu",
             "-p", "no:cacheprovider", f"{os.path.abspath(__file__)}::"
             f"test_one_launch_of_the_minibatch_chunk[{twin}]"],
            capture_output=True, text=True, env=env, timeout=600)
        print(out.stdout[-3000:])
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
        assert " passed" in out.stdout and "failed" not in out.stdout
        assert "skipped" not in out.stdout
        return
    _run_chunk_case(case)


# ------------------------------------------------------------ the operators
def _operator_problem(det, S, n0, seed):
    b = ll.base_problem(det, S, n0, seed=seed, eigen=False)
    rng = np.random.default_rng(seed + 1)
    far = (rng.standard_normal((n0, 1, S, det, det)) + 1j * rng.standard_normal(
        (n0, 1, S, det, det))).astype(np.complex64)
    return b, far


def test_forward_operator_in_one_batch_past_4_gib():
    """`fwd_device(sub_batch=-1)`: 1030 positions x 8 modes x 256^2 in one
    batch, every position's far plane against the model."""
    import torch
    import tike_amd._arrays as A
    from tike_amd.operators import Ptycho
    det, S, n0 = 256, 8, ll.N0_BYTES
    N = ll.positions_for(S * det * det * 8, n0, ll.FOUR_GIB)
    ll.assert_no_aliasing({"far": 8 * S * det * det, "scan": 8}, (1, S), n0)
    b, _ = _operator_problem(det, S, n0, seed=21)
    want = ll.ptycho_fwd(b["probe"], b["scan"], b["psi"][0], det)[:, None]
    need = N * S * det * det * 8 + 4 * ll.SLAB_BYTES
    _need_or_skip(need, "fwd 256x8")
    HW = b["psi"].shape[-1]
    with _measured("fwd-256x8", need), Ptycho(
            probe_shape=det, detector_shape=det, nz=HW, n=HW) as op:
        out = scan = None
        try:
            scan = _rep(b["scan"], N // n0)
            out = torch.full((N, 1, S, det, det), float("nan"),
                             dtype=torch.complex64, device=scan.device)
            assert out.numel() * 8 > 1 << 32
            op.fwd_device(A.to_device(b["probe"]), scan, A.to_device(b["psi"]),
                          out=out, sub_batch=-1)
            fails = []
            _check_positions(out, want, n0, OP_NORMWISE, "farplane", fails)
            assert not fails, fails
        finally:
            del out, scan


@pytest.mark.parametrize("gib", [4, 16])
def test_adjoint_operator_in_one_batch(gib):
    """`adj_device` (no chunking at all): just over 4 GiB of far plane, and
    just over 16 GiB -- past 2^31 complex elements.  probe_adj position by
    position; psi_adj = R x the base sum, within the accumulation bound."""
    import torch
    import tike_amd._arrays as A
    from tike_amd.operators import Ptycho
    det, S, n0 = 256, 8, ll.N0_BYTES
    span = S * det * det * 8
    N = ll.positions_for(span, n0, gib << 30)
    R = N // n0
    ll.assert_no_aliasing({"far / probe_adj": span, "objproj": 8 * det * det,
                           "scan": 8}, (1, S), n0)
    b, far = _operator_problem(det, S, n0, seed=22)
    bprobe = np.broadcast_to(b["probe"][0], (n0, S, det, det))
    psi_adj, probe_adj = ll.ptycho_adj(far[:, 0], bprobe, b["scan"],
                                       b["psi"][0])
    # (the object projection the kernel scatters: one term per bilinear tap)
    objproj = np.sum(np.conj(bprobe.astype(np.complex128)) * ll.ifft2(
        far[:, 0]), 1)
    _, mag, cnt = ll.scatter(objproj, b["scan"], *b["psi"].shape[-2:])
    need = 2 * N * span + N * det * det * 8 + 4 * ll.SLAB_BYTES
    _need_or_skip(need, f"adjoint {gib} GiB")
    HW = b["psi"].shape[-1]
    with _measured(f"adj-256x8-{gib}GiB", need), Ptycho(
            probe_shape=det, detector_shape=det, nz=HW, n=HW) as op:
        far_d = scan = got_psi = got_probe = None
        try:
            scan = _rep(b["scan"], R)
            far_d = _rep(far, R)
            assert far_d.numel() * 8 > gib << 30
            got_probe = torch.full((N, 1, S, det, det), float("nan"),
                                   dtype=torch.complex64, device=scan.device)
            psi_d = A.to_device(b["psi"])
            got_psi = torch.full_like(psi_d, float("nan"))
            op.adj_device(far_d, A.to_device(b["probe"]), scan, psi_d,
                          psi_adj=got_psi, probe_adj=got_probe)
            fails = []
            _check_positions(got_probe, probe_adj[:, None], n0, OP_NORMWISE,
                             "probe_adj", fails)
            _check_accumulated(got_psi[0], R * psi_adj, R * mag, R * cnt,
                               OP_NORMWISE, "psi_adj", fails)
            assert not fails, fails
        finally:
            del far_d, scan, got_psi, got_probe


@pytest.mark.parametrize("n,entry", [(256, "tike_fft2"),
                                     (300, "tike_fft2_general")])
def test_transforms_past_4_gib(n, entry):
    """ntile tiles of n x n just over 4 GiB in one call, forward, out of
    place: every tile against numpy's float64 transform."""
    import torch
    import tike_amd._arrays as A
    from tike_amd._lib import check, lib
    n0 = ll.N0_BYTES
    ntile = ll.positions_for(8 * n * n, n0, ll.FOUR_GIB)
    ll.assert_no_aliasing({"tiles": 8 * n * n}, (1,), n0)
    assert ntile * n < 1 << 31  # the documented bound of the general engine
    rng = np.random.default_rng(n)
    x = (rng.standard_normal((n0, n, n)) + 1j * rng.standard_normal(
        (n0, n, n))).astype(np.complex64)
    want = ll.fft2(x)
    need = 2 * ntile * n * n * 8 + 4 * ll.SLAB_BYTES
    _need_or_skip(need, entry)
    with _measured(f"{entry}-{n}", need):
        xin = out = None
        try:
            xin = _rep(x, ntile // n0)
            out = torch.full_like(xin, float("nan"))
            args = (A.ptr(xin), A.ptr(out), ntile, n, 0, 1.0 / n)
            if entry == "tike_fft2":
                check(lib.tike_fft2(*args, A.stream_ptr()), entry)
            else:
                check(lib.tike_fft2_general(*args, 0, 0, A.stream_ptr()), entry)
            fails = []
            _check_positions(out, want, n0, OP_NORMWISE, entry, fails)
            assert not fails, fails
        finally:
            del xin, out


# --------------------------- launches with a position count in gridDim.y
def _count_problem(det, S, n0, seed):
    rng = np.random.default_rng(seed)
    far = (rng.standard_normal((n0, S, det, det)) + 1j * rng.standard_normal(
        (n0, S, det, det))).astype(np.complex64)
    inten = (np.abs(far.astype(np.complex128)) ** 2).sum(1)
    data = (inten * (1 + 0.2 * rng.standard_normal(inten.shape)) ** 2).astype(
        np.float32)
    mask = rng.random((det, det)) > 0.1
    return far, inten, data, mask


def _factor(inten, data, mask, model, unmeasured):
    dm = np.where(mask, data.astype(np.float64), 0.0)
    if model == 0:
        term = (np.sqrt(inten) - np.sqrt(dm)) ** 2
        g = -(1 - np.sqrt(dm) / (np.sqrt(inten) + 1e-9))
    else:
        term = inten - dm * np.log(inten + 1e-9)
        g = -(1 - dm / (inten + 1e-9))
    costs = np.where(mask, term, 0.0).sum((-2, -1)) / mask.sum()
    return np.where(mask, g, unmeasured - 1.0), costs


@pytest.mark.parametrize("model", [0, 1])
def test_farplane_gradient_past_65536_positions(model):
    """`tike_farplane_gradient`, direct, 16^2 x 2 modes: positions in
    gridDim.y beyond the device's limit.  Outputs prefilled with NaN."""
    import torch
    import tike_amd._arrays as A
    from tike_amd._lib import check, lib
    det, S, n0 = 16, 2, ll.N0_COUNT
    limit, counts = _grid_limit()
    N = ll.positions_for(1, n0, limit)
    ll.assert_no_aliasing({"far": 8 * S * det * det, "data": 4 * det * det,
                           "costs": 4}, (1, S), n0, counts)
    far, _, data, mask = _count_problem(det, S, n0, seed=31 + model)
    inten = (np.abs(far.astype(np.complex128)) ** 2).sum(1)
    g, costs = _factor(inten, data, mask, model, 0.9)
    need = N * det * det * (8 * S + 8) + 4 * ll.SLAB_BYTES
    _need_or_skip(need, "tike_farplane_gradient")
    with _measured(f"tike_farplane_gradient-model{model}", need):
        R = N // n0
        far_d = data_d = inten_d = costs_d = None
        try:
            far_d, data_d = _rep(far, R), _rep(data, R)
            data_d[:, torch.from_numpy(~mask).to(data_d.device)] = float("nan")
            inten_d = torch.full((N, det, det), float("nan"),
                                 device=far_d.device)
            costs_d = torch.full((N,), float("nan"), device=far_d.device)
            mask_d = A.to_device(mask.astype(np.uint8))
            check(lib.tike_farplane_gradient(
                A.ptr(far_d), A.ptr(data_d), A.ptr(mask_d), A.ptr(inten_d),
                A.ptr(costs_d), N, S, det, model, 1, 0.9, int(mask.sum()),
                A.stream_ptr()), "tike_farplane_gradient")
            fails = []
            _check_positions(far_d, far * g[:, None], n0, OP_NORMWISE,
                             "farplane x factor", fails)
            _check_positions(inten_d, inten, n0, OP_NORMWISE, "intensity",
                             fails)
            _check_costs(costs_d, costs, n0, COST_RTOL, fails)
            assert not fails, fails
        finally:
            del far_d, data_d, inten_d, costs_d


@pytest.mark.parametrize("model", [0, 1])
def test_gradient_scale_past_65536_positions(model):
    """`tike_gradient_scale` (the pos_major route's factor), direct."""
    import torch
    import tike_amd._arrays as A
    from tike_amd._lib import check, lib
    det, n0 = 16, ll.N0_COUNT
    limit, counts = _grid_limit()
    N = ll.positions_for(1, n0, limit)
    ll.assert_no_aliasing({"intensity / data / gscale": 4 * det * det,
                           "costs": 4}, (1,), n0, counts)
    _, inten, data, mask = _count_problem(det, 2, n0, seed=41 + model)
    inten = inten.astype(np.float32)
    g, costs = _factor(inten.astype(np.float64), data, mask, model, 0.9)
    need = N * det * det * 12 + 4 * ll.SLAB_BYTES
    _need_or_skip(need, "tike_gradient_scale")
    with _measured(f"tike_gradient_scale-model{model}", need):
        R = N // n0
        inten_d = data_d = g_d = costs_d = None
        try:
            inten_d, data_d = _rep(inten, R), _rep(data, R)
            g_d = torch.full((N, det, det), float("nan"),
                             device=inten_d.device)
            costs_d = torch.full((N,), float("nan"), device=inten_d.device)
            mask_d = A.to_device(mask.astype(np.uint8))
            check(lib.tike_gradient_scale(
                A.ptr(inten_d), A.ptr(data_d), A.ptr(mask_d), A.ptr(g_d),
                A.ptr(costs_d), N, det, model, 0.9, int(mask.sum()),
                A.stream_ptr()), "tike_gradient_scale")
            fails = []
            _check_positions(g_d, g, n0, OP_NORMWISE, "gscale", fails)
            _check_costs(costs_d, costs, n0, COST_RTOL, fails)
            assert not fails, fails
        finally:
            del inten_d, data_d, g_d, costs_d


def test_scale_modes_past_65536_tiles():
    """`tike_scale_modes`, 16^2 x 8 modes: nscan x S tiles in gridDim.y just
    over the limit."""
    import tike_amd._arrays as A
    from tike_amd._lib import check, lib
    det, S, n0 = 16, 8, ll.N0_COUNT
    limit, counts = _grid_limit()
    N = ll.positions_for(S, n0, limit)  # spans counted in tiles
    assert N * S >= limit + n0 * S and N % n0 == 0
    ll.assert_no_aliasing({"far": 8 * S * det * det, "steps": 4 * S}, (1, S),
                          n0, counts)
    far, _, _, mask = _count_problem(det, S, n0, seed=51)
    steps = (0.5 + np.random.default_rng(52).random((n0, S))).astype(np.float32)
    want = far * np.where(mask, steps[:, :, None, None].astype(np.float64), 1.0)
    need = N * S * det * det * 8 + 4 * ll.SLAB_BYTES
    _need_or_skip(need, "tike_scale_modes")
    with _measured("tike_scale_modes", need):
        R = N // n0
        far_d = steps_d = None
        try:
            far_d, steps_d = _rep(far, R), _rep(steps, R)
            mask_d = A.to_device(mask.astype(np.uint8))
            check(lib.tike_scale_modes(A.ptr(far_d), A.ptr(steps_d),
                                       A.ptr(mask_d), N * S, det,
                                       A.stream_ptr()), "tike_scale_modes")
            fails = []
            _check_positions(far_d, want, n0, OP_NORMWISE, "farplane x steps",
                             fails)
            assert not fails, fails
        finally:
            del far_d, steps_d


def test_scatter_and_preconditioner_past_the_group_limit():
    """`tike_scatter_patches`, `tike_psi_preconditioner` and
    `tike_scatter_amplitudes` put groups of 8 positions into gridDim.y: more
    than 8 x the device's limit of positions of 16^2, so that each takes a
    second slice.  The positions of that slice scan a band of the image that
    nothing else touches, and those pixels are held to the tight bar on their
    own (three terms per tap: a dropped launch, or a slice that read its
    patches or positions from the wrong place, cannot hide under the sum of
    half a million); the band of the first slice equals the base sums x the
    number of times every base position occurs in it, within its
    accumulation bound.  Outside the deterministic switch the case runs once
    more in a child under it, on the ordered kernels."""
    import torch
    import tike_amd._arrays as A
    from tike_amd import _lib
    from tike_amd._lib import check, lib
    pw, n0, W, band = 16, ll.N0_COUNT, 40, 40
    H = 2 * band
    span, counts = _grid_limit(unit=8)  # positions of the first slice
    N = ll.positions_for(1, n0, span) + 2 * n0
    R = N // n0
    ll.assert_no_aliasing({"objproj": 8 * pw * pw, "amp": 4 * pw * pw,
                           "scan": 8}, (1, 8), n0, counts)
    rng = np.random.default_rng(61)
    scan = (1 + (band - pw - 3) * rng.random((n0, 2))).astype(np.float32)
    proj = (rng.standard_normal((n0, pw, pw)) + 1j * rng.standard_normal(
        (n0, pw, pw))).astype(np.complex64)
    amp = rng.random((pw, pw)).astype(np.float32)
    amps = rng.random((n0, pw, pw)).astype(np.float32)
    # how often base position i occurs in the first slice and behind it
    total = np.full(n0, R)
    first = span // n0 + (np.arange(n0) < span % n0)
    later = total - first
    assert later.sum() == N - span and 2 * n0 <= later.sum() <= 4 * n0

    def expected(values):
        """(want, bound) over the whole image: the first slice's band above,
        the later positions' band below (float32 positions, as the device
        forms them)."""
        want = np.zeros((H, W), np.complex128)
        bound = np.zeros((H, W))
        for times, shift in ((first, 0), (later, band)):
            mags, cnts = np.zeros((H, W)), np.zeros((H, W))
            for i in range(n0):
                at = scan[i:i + 1] + np.array([shift, 0], np.float32)
                img, mag, cnt = ll.scatter(values[i:i + 1], at, H, W)
                want += times[i] * img
                mags += times[i] * mag
                cnts += times[i] * cnt
            bound += ll.accumulation_bound(mags, cnts)
        return want, bound

    need = N * pw * pw * 12 + 4 * ll.SLAB_BYTES
    _need_or_skip(need, "scatter")
    with _measured("scatter+preconditioner+amplitudes", need):
        scan_d = proj_d = amps_d = None
        try:
            scan_d, proj_d, amps_d = _rep(scan, R), _rep(proj, R), _rep(amps, R)
            scan_d[span:, 0] += band  # the later slices: the band below
            dev = scan_d.device
            acc = torch.zeros((2, H, W), dtype=torch.float32, device=dev)
            pre = torch.zeros((H, W), dtype=torch.float32, device=dev)
            ill = torch.zeros((H, W), dtype=torch.float32, device=dev)
            st = A.stream_ptr()
            check(lib.tike_scatter_patches(A.ptr(proj_d), A.ptr(scan_d),
                                           A.ptr(acc), N, pw, H, W, st),
                  "tike_scatter_patches")
            check(lib.tike_psi_preconditioner(A.ptr(A.to_device(amp)),
                                              A.ptr(scan_d), A.ptr(pre), N,
                                              pw, H, W, st),
                  "tike_psi_preconditioner")
            check(lib.tike_scatter_amplitudes(A.ptr(amps_d), A.ptr(scan_d),
                                              A.ptr(ill), N, pw, H, W, st),
                  "tike_scatter_amplitudes")
            fails = []
            for what, got, values in (
                    ("tike_scatter_patches", torch.complex(acc[0], acc[1]),
                     proj),
                    ("tike_psi_preconditioner", pre,
                     np.broadcast_to(amp, (n0, pw, pw))),
                    ("tike_scatter_amplitudes", ill, amps)):
                want, bound = expected(values.astype(np.complex128))
                if not got.is_complex():
                    want = want.real
                # the two bands on their own: each with the bar relative to
                # ITS largest entry
                for name, rows in (("first slice", slice(0, band)),
                                   ("later slices", slice(band, H))):
                    excess = ll.entrywise_excess(
                        got[rows].contiguous(), want[rows], bound[rows],
                        OP_NORMWISE)
                    print(f"  {what}, {name}: worst entry at {excess:.3e} of "
                          f"(1e-5 x max|want| + its accumulation bound "
                          f"<= {bound[rows].max():.2e})")
                    assert np.abs(want[rows]).max() > 0
                    if not excess <= 1.0:
                        fails.append(f"{what}, {name}: {excess:.3e}")
            assert not fails, fails
        finally:
            del scan_d, proj_d, amps_d
    if not _lib.DETERMINISTIC:
        env = dict(os.environ, TIKE_DETERMINISTIC="1")
        out = subprocess.run(
            [sys.executable, "-m", "pytest", "-x", "-q", "-s", "-m", "gpu",
             "-p", "no:cacheprovider", f"{os.path.abspath(__file__)}::"
             "test_scatter_and_preconditioner_past_the_group_limit"],
            capture_output=True, text=True, env=env, timeout=600)
        print(out.stdout[-3000:])
        assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
        assert " passed" in out.stdout and "skipped" not in out.stdout


# ------------------------------------------------------ the minibatch tail
def _check_rows(got, want, n0, what, fails):
    """Per-position sums over pixels, entry by entry, with the bars of
    test_lstsq_tail_gpu.py's `check_sums`: rtol 2e-4, atol 2e-5 max|want|."""
    import torch
    w = torch.from_numpy(np.asarray(want, np.float64)).to(got.device)
    assert bool(torch.isfinite(got).all()), f"{what}: an entry was not written"
    err = (got.to(torch.float64).reshape(-1, *w.shape) - w).abs()
    tol = 2e-4 * w.abs() + 2e-5 * float(np.abs(want).max())
    ratio = (err / tol).reshape(err.shape[0], -1).amax(1)
    worst, k = float(ratio.max()), int(ratio.argmax())
    print(f"  {what}: worst error / tolerance {worst:.3e} (replica {k})")
    if not worst <= 1.0:
        fails.append(f"{what}: {worst:.3e} x tolerance in replica {k}")


def test_minibatch_tail_entries_past_4_gib():
    """`tike_lstsq_step_stats`, `tike_eigen_position_sums`,
    `tike_position_sums`, `tike_probe_grad` and `tike_scatter_patches`, direct,
    on (N, 256, 256) patches and chi just over 4 GiB each (N = 8195), against
    tests/lstsq_tail.py's float64 functions on the base positions (and R x
    the base sums for the two accumulations)."""
    import torch
    import lstsq_tail as lt
    import tike_amd._arrays as A
    from tike_amd._lib import check, lib
    from tike_amd.ptycho.position import gaussian_derivative_taps
    pw, S, n0 = 256, 1, ll.N0_BYTES
    N = ll.positions_for(8 * pw * pw, n0, ll.FOUR_GIB)
    R = N // n0
    ll.assert_no_aliasing({"patches / chi": 8 * pw * pw, "stats": 32,
                           "sums5": 20, "scan": 8, "weights": 8 * S}, (1,), n0)
    rng = np.random.default_rng(71)
    rc = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)
                     ).astype(np.complex64)
    HW = pw + 24
    scan = (1 + 21 * rng.random((n0, 2))).astype(np.float32)
    psi, gobj = rc(HW, HW), rc(HW, HW)
    probe, mpu, E = rc(S, pw, pw), rc(S, pw, pw), rc(pw, pw)
    chi = rc(n0, 1, pw, pw)
    w = (1 + 0.3 * rng.standard_normal((n0, 2, S))).astype(np.float32)
    O = ll.patches_of(psi, scan, pw).astype(np.complex64)  # as stored
    G = ll.patches_of(gobj, scan, pw)
    Pn = (w[:, 0, 0, None, None] * probe[0].astype(np.complex128) +
          w[:, 1, 0, None, None] * E.astype(np.complex128))
    stats = lt.step_stats(G, O, chi[:, 0], probe[0], Pn, mpu[0])
    eproj = lt.eigen_proj(O, chi[:, 0], mpu[0], E)
    sums5 = lt.position_sums5(O, chi[:, 0], mpu[0], E)
    num, den = ll.position_terms(O.astype(np.complex128), Pn,
                                 chi[:, 0].astype(np.complex128))
    terms = np.conj(ll.patches_of(psi, scan, pw)) * chi[:, 0]
    img, mag, cnt = ll.scatter(chi[:, 0], scan, HW, HW)
    need = 3 * N * 8 * pw * pw + 4 * ll.SLAB_BYTES
    _need_or_skip(need, "minibatch tail")
    with _measured("minibatch-tail-256", need):
        O_d = chi_d = patches_out = None
        try:
            st = A.stream_ptr()
            dev = lambda x: A.to_device(np.ascontiguousarray(x))
            scan_d, w_d = _rep(scan, R), _rep(w, R)
            O_d, chi_d = _rep(O, R), _rep(chi, R)
            assert O_d.numel() * 8 > 1 << 32
            psi_d, gobj_d, probe_d, mpu_d, E_d = map(
                dev, (psi, gobj, probe, mpu, E))
            nan = lambda *s: torch.full(s, float("nan"), device=O_d.device)
            fails = []
            stats_d, eproj_d = nan(N, 8), nan(N)
            check(lib.tike_lstsq_step_stats(
                A.ptr(chi_d), A.ptr(scan_d), A.ptr(psi_d), A.ptr(gobj_d),
                A.ptr(probe_d), A.ptr(E_d), A.ptr(w_d), 1, 1, None,
                A.ptr(mpu_d), A.ptr(O_d), A.ptr(stats_d), N, S, 1, pw, HW, HW,
                A.ptr(E_d), A.ptr(eproj_d), st), "tike_lstsq_step_stats")
            _check_rows(stats_d, stats, n0, "step stats", fails)
            _check_rows(eproj_d, eproj, n0, "eigen_proj", fails)
            sums_d = nan(N, 5)
            check(lib.tike_eigen_position_sums(
                A.ptr(O_d), A.ptr(chi_d), A.ptr(mpu_d), A.ptr(E_d), None, 1, 1,
                0, A.ptr(sums_d), N, pw, 1, st), "tike_eigen_position_sums")
            _check_rows(sums_d, sums5, n0, "eigen position sums", fails)
            taps, radius = gaussian_derivative_taps(sigma=0.333)
            num_d, den_d = nan(N, 2), nan(N, 2)
            check(lib.tike_position_sums(
                A.ptr(O_d), A.ptr(chi_d), 1, A.ptr(probe_d), A.ptr(E_d),
                A.ptr(w_d), 1, 1, taps.ctypes.data, radius, A.ptr(num_d),
                A.ptr(den_d), N, S, pw, st), "tike_position_sums")
            _check_rows(num_d, num, n0, "position numerator", fails)
            _check_rows(den_d, den, n0, "position denominator", fails)
            # the two accumulations: R x the base sums
            del O_d
            O_d = None
            patches_out = torch.full((N, pw, pw), float("nan"),
                                     dtype=torch.complex64,
                                     device=chi_d.device)
            grad = torch.zeros((S, pw, pw), dtype=torch.complex64,
                               device=chi_d.device)
            check(lib.tike_probe_grad(
                A.ptr(chi_d), A.ptr(scan_d), A.ptr(psi_d), A.ptr(patches_out),
                A.ptr(grad), N, S, pw, HW, HW, st), "tike_probe_grad")
            _check_positions(patches_out, ll.patches_of(psi, scan, pw), n0,
                             OP_NORMWISE, "patches of tike_probe_grad", fails)
            _check_accumulated(grad[0], R * terms.sum(0),
                               R * np.abs(terms).sum(0),
                               np.full((pw, pw), N), GRAD_BAR,
                               "tike_probe_grad", fails)
            acc = torch.zeros((2, HW, HW), dtype=torch.float32,
                              device=chi_d.device)
            check(lib.tike_scatter_patches(A.ptr(chi_d), A.ptr(scan_d),
                                           A.ptr(acc), N, pw, HW, HW, st),
                  "tike_scatter_patches")
            _check_accumulated(torch.complex(acc[0], acc[1]), R * img,
                               R * mag, R * cnt, GRAD_BAR,
                               "tike_scatter_patches", fails)
            # ... and once more with chi ZERO below the 2^32-byte boundary:
            # the sums are then those of the positions behind it alone, at
            # the tight bar -- a read that wrapped there would find zeros
            first = (1 << 32) // (8 * pw * pw)
            tail = np.arange(first, N) % n0
            assert 0 < len(tail) <= 2 * n0  # (base indices, with repeats)
            chi_d[:first] = 0
            grad.zero_()
            acc.zero_()
            check(lib.tike_probe_grad(
                A.ptr(chi_d), A.ptr(scan_d), A.ptr(psi_d), None, A.ptr(grad),
                N, S, pw, HW, HW, st), "tike_probe_grad")
            check(lib.tike_scatter_patches(A.ptr(chi_d), A.ptr(scan_d),
                                           A.ptr(acc), N, pw, HW, HW, st),
                  "tike_scatter_patches")
            # (adding an exact zero does not round: the depth is the tail's)
            _check_accumulated(grad[0], terms[tail].sum(0),
                               np.abs(terms[tail]).sum(0),
                               np.full((pw, pw), len(tail)), GRAD_BAR,
                               "tike_probe_grad, positions past 2^32 bytes",
                               fails)
            timg, tmag, tcnt = ll.scatter(chi[tail, 0], scan[tail], HW, HW)
            _check_accumulated(torch.complex(acc[0], acc[1]), timg, tmag, tcnt,
                               GRAD_BAR,
                               "tike_scatter_patches, positions past 2^32 "
                               "bytes", fails)
            assert not fails, fails
        finally:
            del O_d, chi_d, patches_out


# ------------------------------------------------------------- fly scans
@pytest.mark.parametrize("model", ["gaussian", "poisson"])
def test_fly_farplane_gradient_past_4_gib(model):
    """`tike_fly_farplane_gradient` at fly 4 x 8 modes x 128^2: 1030 frames of
    32 far planes each, just over 4 GiB, uint16 counts and a mask; every
    frame against tests/fly_scan.py's float64 functions, with the bars of
    test_fly_scan_gpu.py (OP_NORMWISE for gradient, intensity and costs)."""
    import torch
    import fly_scan as fs
    import tike_amd._arrays as A
    from tike_amd.operators import Ptycho
    det, S, fly, n0, UMS = 128, 8, 4, ll.N0_BYTES, 0.75
    frame_bytes = 8 * fly * S * det * det
    nframe = ll.positions_for(frame_bytes, n0, ll.FOUR_GIB)
    R = nframe // n0
    ll.assert_no_aliasing({"far (a frame)": frame_bytes,
                           "far (a position)": frame_bytes // fly,
                           "data": 2 * det * det, "intensity": 4 * det * det,
                           "costs": 4}, (1, fly, fly * S), n0)
    rng = np.random.default_rng(81)
    far = (rng.standard_normal((n0 * fly, 1, S, det, det)) +
           1j * rng.standard_normal((n0 * fly, 1, S, det, det))).astype(
               np.complex64)
    counts = rng.poisson(2.0 * fly * S, (n0, det, det)).astype(np.uint16)
    mask = fs.block_mask(det)
    d = counts.astype(np.float64)
    inten = fs.frame_intensity(far, fly)
    cost_want = fs.cost_each(model, d, inten, mask)
    expect = np.where(mask, -fs.farplane_gradient(
        model, fs.masked(d, mask), far, fly, mask), (UMS - 1.0) * far)
    junk = counts.copy()
    junk[:, ~mask] = 65535  # counts that must not be read
    need = nframe * (frame_bytes + 6 * det * det) + 4 * ll.SLAB_BYTES
    _need_or_skip(need, "tike_fly_farplane_gradient")
    with _measured(f"tike_fly_farplane_gradient-{model}", need), Ptycho(
            probe_shape=det, detector_shape=det, nz=det + 8, n=det + 8) as op:
        far_d = data_d = out_i = None
        try:
            far_d = _rep(far, R)
            assert far_d.numel() * 8 > 1 << 32
            data_d = torch.from_numpy(junk.view(np.int16)).to(
                far_d.device).repeat(R, 1, 1).view(torch.uint16)
            out_i = torch.full((nframe, det, det), float("nan"),
                               device=far_d.device)
            costs = torch.full((nframe,), float("nan"), device=far_d.device)
            op.fly_farplane_gradient(
                far_d, data_d, fly, model=("gaussian", "poisson").index(model),
                measured=A.to_device(mask.astype(np.uint8)),
                num_measured=int(mask.sum()), intensity=out_i, costs=costs,
                apply_gradient=True, unmeasured_scaling=UMS)
            fails = []
            # (a "position" of the comparison is a frame: fly x S planes)
            _check_positions(far_d.reshape(nframe, fly, S, det, det),
                             expect.reshape(n0, fly, S, det, det), n0,
                             OP_NORMWISE, "far-plane gradient", fails)
            _check_positions(out_i, inten, n0, OP_NORMWISE, "intensity", fails)
            _check_costs(costs, cost_want, n0, OP_NORMWISE, fails)
            assert not fails, fails
        finally:
            del far_d, data_d, out_i


# ------------------------------------------------- position refinement (pd)
def test_position_pd_sums_on_three_stacked_far_planes_past_4_gib():
    """`tike_position_pd_sums` on ONE stacked array [F(scan); F(scan + dx);
    F(scan + dy)] as `position_pd_shifts` lays it out, each third just over
    4 GiB (1030 positions x 8 modes x 256^2), uint16 counts; against
    tests/position_pd.py's `sums_f64`.  The bar of test_position_pd_gpu.py
    (every column OP_NORMWISE normwise over the positions) is applied to
    every replica of the base positions on its own: a sum of one position
    may cancel, so a single entry has no relative bar of its own, but one
    entry read from a neighbour moves its replica's column far beyond it."""
    import torch
    import position_pd as pp
    import tike_amd._arrays as A
    from tike_amd._lib import check, lib
    det, S, n0, inv_dx = 256, 8, ll.N0_BYTES, -1.0
    npix = det * det
    N = ll.positions_for(8 * S * npix, n0, ll.FOUR_GIB)
    R = N // n0
    ll.assert_no_aliasing({"far": 8 * S * npix, "data": 2 * npix, "sums": 20,
                           "costs": 4}, (1, S), n0)
    rng = np.random.default_rng(91)
    f0 = (rng.standard_normal((n0, S, npix)) + 1j * rng.standard_normal(
        (n0, S, npix))).astype(np.complex64)
    fx, fy = ((f0 * (1 + 0.05 * (rng.standard_normal(f0.shape) + 1j *
                                 rng.standard_normal(f0.shape)))).astype(
                                     np.complex64) for _ in range(2))
    data = rng.poisson(2.0 * S, (n0, npix)).astype(np.uint16)
    want_sums, want_costs = pp.sums_f64(f0, fx, fy, data, inv_dx)
    need = 3 * N * 8 * S * npix + N * 2 * npix + (1 << 28)
    _need_or_skip(need, "tike_position_pd_sums")
    with _measured("tike_position_pd_sums", need):
        far = None
        try:
            far = torch.empty((3 * N, 1, S, det, det), dtype=torch.complex64,
                              device="cuda")
            assert far[:N].numel() * 8 > 1 << 32
            for k, f in enumerate((f0, fx, fy)):  # (broadcast: no temporary)
                far[k * N:(k + 1) * N].view(R, n0, 1, S, det, det).copy_(
                    A.to_device(f).reshape(1, n0, 1, S, det, det).expand(
                        R, n0, 1, S, det, det))
            data_d = torch.from_numpy(data.view(np.int16)).to(
                far.device).repeat(R, 1).view(torch.uint16)
            sums = torch.full((N, 5), float("nan"), device=far.device)
            costs = torch.full((N,), float("nan"), device=far.device)
            check(lib.tike_position_pd_sums(
                A.ptr(far[:N]), A.ptr(far[N:2 * N]), A.ptr(far[2 * N:]),
                A.ptr(data_d), 1, inv_dx, A.ptr(sums), A.ptr(costs), N, S,
                npix, A.stream_ptr()), "tike_position_pd_sums")
            assert bool(torch.isfinite(sums).all() & torch.isfinite(costs).all())
            got = torch.cat([sums, costs[:, None]], 1).to(
                torch.float64).reshape(R, n0, 6)
            want = torch.from_numpy(np.concatenate(
                [want_sums, want_costs[:, None]], 1)).to(far.device)
            miss = (torch.linalg.vector_norm(got - want, dim=1) /
                    torch.linalg.vector_norm(want, dim=0))  # (R, 6)
            worst = miss.amax(0).cpu().numpy()
            for name, e in zip(("aa", "ab", "bb", "ar", "br", "costs"), worst):
                print(f"  sum {name}: worst replica normwise {e:.3e} "
                      f"(bar {OP_NORMWISE:.1e})")
            assert (worst <= OP_NORMWISE).all(), worst
        finally:
            del far


# ----------------------------------------------- cgrad's device line search
@pytest.mark.parametrize("det", [128, 256])
def test_cgrad_line_search_all_steps_at_once(det):
    """`tike_cgrad_line_search_linear_masked`, the search that prices all 16
    step lengths from two hand-offs, with ONE chunk.  128^2: more positions
    than gridDim.y holds (its costs launch puts the chunk's positions
    there).  256^2 x 1: steps x N x det^2 x 8 just over 4 GiB.  The cost rows
    of x and of the 16 step lengths (stages 1 and 3), every position against
    float64 costs of F(x) + s F(d) (the far plane is linear in the object),
    gaussian model, COST_RTOL."""
    import torch
    import cgrad_models as cm
    import tike_amd._arrays as A
    from tike_amd._lib import check, lib
    from tike_amd.operators.propagation import fft_scales
    S, step, counts = 1, 0.5, ()
    if det == 128:
        n0 = ll.N0_COUNT
        limit, counts = _grid_limit()
        N = ll.positions_for(1, n0, limit)
    else:
        n0 = ll.N0_BYTES
        N = ll.positions_for(16 * det * det * 8, n0, ll.FOUR_GIB)
        assert 16 * N * det * det * 8 > 1 << 32
    R = N // n0
    ll.assert_no_aliasing({"far_a / far_b": 8 * S * det * det,
                           "all steps of a position": 16 * 8 * det * det,
                           "data": 4 * det * det, "scan": 8, "cost rows": 4},
                          (1, 16), n0, counts)
    b = ll.base_problem(det, S, n0, seed=101, eigen=False)
    rng = np.random.default_rng(102)
    psi = b["psi"][0]
    d = (0.1 * (rng.standard_normal(psi.shape) + 1j * rng.standard_normal(
        psi.shape))).astype(np.complex64)
    fa = ll.ptycho_fwd(b["probe"], b["scan"], psi, det)
    fb = ll.ptycho_fwd(b["probe"], b["scan"], d, det)
    d64 = b["data"].astype(np.float64)
    want = np.stack([cm.cost_each("gaussian", d64, np.sum(
        np.abs(fa + s * fb) ** 2, axis=1)) for s in
                     [0.0] + [step * 2.0 ** -k for k in range(16)]])  # (17, n0)
    need = N * det * det * (2 * 8 * S + 4) + (1 << 28)
    _need_or_skip(need, "cgrad line search")
    with _measured(f"tike_cgrad_line_search_linear-{det}", need):
        far_a = far_b = data_d = None
        try:
            dev = lambda x: A.to_device(np.ascontiguousarray(x))
            scan_d, data_d = _rep(b["scan"], R), _rep(b["data"], R)
            far_a = torch.empty((N, 1, S, det, det), dtype=torch.complex64,
                                device=scan_d.device)
            far_b = torch.empty_like(far_a)
            costs_k = torch.full((17 * N + 1,), float("nan"),
                                 device=scan_d.device)
            state = torch.tensor([0.0, step, 0.0, 0.0, 0.0],
                                 dtype=torch.float64, device=scan_d.device)
            sums = torch.zeros(17, dtype=torch.float64, device=scan_d.device)
            psi_d, d_d, probe_d = dev(psi), dev(d), dev(b["probe"][0, 0])
            xs = torch.zeros_like(psi_d)
            H, W = psi.shape
            for stage in (1, 3):  # first pass: x and 8 steps; second: 8 more
                if stage == 3:
                    state[1] = step / 256
                check(lib.tike_cgrad_line_search_linear_masked(
                    0, A.ptr(psi_d), A.ptr(d_d), A.ptr(xs), A.ptr(probe_d),
                    A.ptr(scan_d), A.ptr(data_d), 0, A.ptr(far_a), 0,
                    A.ptr(far_b), A.ptr(costs_k), N, N, S, det, H, W,
                    fft_scales(det, "ortho")[0], float(N), A.ptr(state), stage,
                    A.ptr(sums), None, 0, det * det, A.stream_ptr()),
                    "tike_cgrad_line_search_linear_masked")
            rows = costs_k[:17 * N].reshape(17, N)
            assert bool(torch.isfinite(rows).all()), "a cost was not written"
            fails = []
            for k in range(17):
                _check_costs(rows[k], want[k], n0, COST_RTOL, fails,
                             what=f"cost row {k}")
            assert not fails, fails
        finally:
            del far_a, far_b, data_d


# ------------------------------------------- Propagation at the line limit
def test_propagation_at_the_general_engines_line_limit():
    """`Propagation.fwd` on a batch of the smallest tiles the shape-general
    engine takes, with ntile x n just over 2^31 -- what `tk_fft2_general`
    refuses in one call.  Either the caller splits and every tile is right,
    or `ValueError` is raised by name; `out` is never handed back unwritten
    (it is prefilled: the input, overwritten in place)."""
    import torch
    from tike_amd._lib import lib
    from tike_amd.operators import Propagation
    n = next(k for k in (3, 5, 6, 7) if lib.tike_fft2_supported(k))
    n0 = ll.N0_BYTES
    ntile = ll.positions_for(n, n0, 1 << 31)  # spans counted in lines
    assert ntile * n >= 1 << 31
    ll.assert_no_aliasing({"tiles": 8 * n * n, "lines": 8 * n}, (1, n), n0,
                          (1 << 31,))
    rng = np.random.default_rng(111)
    x = (rng.standard_normal((n0, n, n)) + 1j * rng.standard_normal(
        (n0, n, n))).astype(np.complex64)
    want = ll.fft2(x)
    need = ntile * n * n * 8 + 4 * ll.SLAB_BYTES
    _need_or_skip(need, "Propagation.fwd")
    with _measured(f"Propagation.fwd-{n}x{n}", need):
        x_d = out = None
        try:
            x_d = _rep(x, ntile // n0)
            with Propagation(detector_shape=n) as op:
                try:
                    out = op.fwd(x_d, overwrite=True)
                except ValueError as e:
                    print(f"  {ntile} tiles of {n} x {n}: ValueError({e})")
                    return
            fails = []
            _check_positions(out, want, n0, OP_NORMWISE, "every tile", fails)
            assert not fails, fails
        finally:
            del x_d, out


# ------------------------------------------------ rpie, an object of slices
def test_rpie_two_slices_fused_with_its_free_memory_chunk():
    """`_gradients_multislice_fused` at 256^2 x 8 modes, two slices, 1030
    positions, with the chunk it sizes from the free memory: the chunk's
    array of inverse passes (one per slice) spans more than 4 GiB in one
    launch.  Costs and chi0 of every position, both numerators of both
    slices = R x the base sums within the accumulation bound."""
    import importlib
    import torch
    import tike_amd._arrays as A
    import tike_amd.ptycho as tp
    from tike_amd.communicators import Comm
    from tike_amd.operators import Ptycho
    from tike_amd.ptycho.solvers import lstsq as L
    Rp = importlib.import_module("tike_amd.ptycho.solvers.rpie")
    det, S, D, n0 = 256, 8, 2, ll.N0_BYTES
    N = ll.positions_for(S * det * det * 8, n0, ll.FOUR_GIB)
    R = N // n0
    ll.assert_no_aliasing({"far / beams": 8 * S * det * det,
                           "objproj / chi0": 8 * det * det,
                           "data": 4 * det * det, "scan": 8, "costs": 4},
                          (1, S), n0)
    b = ll.base_problem(det, S, n0, seed=121, eigen=False)
    rng = np.random.default_rng(122)
    psi = np.concatenate([b["psi"], (1 + 0.1 * (rng.standard_normal(
        b["psi"].shape) + 1j * rng.standard_normal(b["psi"].shape))).astype(
            np.complex64)])
    HW = psi.shape[-1]
    eo = tp.ExitWaveOptions(measured_pixels=np.ones((det, det), dtype=bool))
    need = 5 * N * S * det * det * 8 + N * det * det * 12 + 4 * ll.SLAB_BYTES
    _need_or_skip(need, "rpie, two slices")
    with _measured("rpie-2-slices-256x8", need), Ptycho(
            probe_shape=det, detector_shape=det, nz=HW, n=HW,
            probe_wavelength=1e-10, probe_FOV_lengths=(2e-6, 2e-6),
            multislice_propagation_distance=1e-6) as op:
        data_d = costs = chi0 = None
        try:
            assert not L.CHUNK_POSITIONS_OVERRIDE and Rp.FUSED_MULTISLICE
            psi_d = A.to_device(psi)
            prop = op.diffraction.propagation._propagator(
                (det, det), psi_d.device).cpu().numpy()
            m = ll.multislice_rpie_model(psi, b["scan"], b["probe"][0, 0],
                                         b["data"], prop)
            scan_d, data_d = _rep(b["scan"], R), _rep(b["data"], R)
            probe_d = A.to_device(b["probe"])
            psi_num = torch.zeros_like(psi_d)
            probe_num = torch.zeros((D, *probe_d.shape), dtype=probe_d.dtype,
                                    device=psi_d.device)
            costs, chi0, _ = Rp._gradients_multislice_fused(
                data_d, psi_d, scan_d, probe_d, None, None, 0, N, Comm(),
                psi_num, probe_num, op=op, exitwave_options=eo)
            torch.cuda.synchronize()
            ws = L._workspace(op).buffers
            per = S * det * det
            chunk = ws["ms_far"].numel() // per
            span = ws["ms_mid"].numel() * 8
            print(f"  chunk of {chunk} positions; its inverse passes span "
                  f"{span / 2**30:.2f} GiB, its hand-off "
                  f"{ws['ms_far'].numel() * 8 / 2**30:.2f} GiB")
            assert span > 1 << 32 and chunk * per * 8 >= 1 << 32, (chunk, span)
            fails = []
            _check_costs(costs, m["costs"], n0, COST_RTOL, fails)
            _check_positions(chi0, m["chi0"], n0, GRAD_BAR, "chi0", fails)
            for t in range(D):
                _check_accumulated(
                    psi_num[t], R * m["psi_num"][t], R * m["psi_abs"][t],
                    R * m["psi_terms"][t], GRAD_BAR, f"psi_num[{t}]", fails)
                _check_accumulated(
                    probe_num[t, 0, 0], R * m["probe_num"][t],
                    R * m["probe_abs"][t],
                    np.full(m["probe_abs"][t].shape, N), GRAD_BAR,
                    f"probe_num[{t}]", fails)
            assert not fails, fails
        finally:
            del data_d, costs, chi0
            op.__dict__.pop("_tike_amd_workspace", None)


# ------------------------------------------------------------- the closing
def test_every_route_ran_in_one_launch():
    """Every value `GradientPlan.route` takes was exercised above (under the
    deterministic switch poisson at 256^2 keeps its far plane: split_kept
    runs twice there); the wall time and the need of every case."""
    total = 0.0
    for name, seconds, gib in REPORT:
        total += seconds
        print(f"{name:48s} {seconds:7.2f} s  {gib:7.2f} GiB")
    print(f"{'total':48s} {total:7.2f} s")
    assert ROUTES_RUN == set(ll.ROUTES), sorted(set(ll.ROUTES) - ROUTES_RUN)
