"""cgrad over the gaussian / poisson cost on the measured pixels: the product
against the NumPy composition (tests/cgrad_models.py) on every gradient route,
the three line searches against each other, the masked line-search entries
directly, data variants, two ranks and deterministic mode."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cgrad_models as cm
from util import assert_close

pytestmark = pytest.mark.gpu

MODES = [("gaussian", True), ("poisson", False), ("poisson", True)]


@pytest.fixture(scope="module")
def tp():
    import tike_amd.ptycho as m
    return m


def _problem(tp, det, pw, S, N, seed, mask):
    rng = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(N)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side),
                              indexing="ij"), -1).reshape(-1, 2)[:N]
    scan = (2 + 7.0 * ij + rng.random((N, 2))).astype(np.float32)
    HW = 7 * (side - 1) + pw + 8
    psi_true = ((0.75 + 0.25 * rng.random((1, HW, HW))) * np.exp(
        1j * np.pi * (rng.random((1, HW, HW)) - 0.5))).astype(np.complex64)
    w = tp.gaussian(pw, rin=0.6)
    probe = np.stack([w * np.exp(1j * np.pi * rng.random((pw, pw))) / (m + 1)
                      for m in range(S)])[None, None].astype(np.complex64)
    data = tp.simulate(det, probe, scan, psi_true).astype(np.float32)
    if mask is not None:
        data[:, ~mask] = np.nan
    return scan, psi_true, probe, data


def _start(psi_true):
    """The first iterate: close enough to the solution that the one-mode
    poisson problems are well conditioned.  Their far fields have dark
    speckles, and where I ~ 0 < d the factor d / (I + 1e-9) is huge: from
    0.5 psi_true + 0.25, a 1e-6 relative change of the counts moves the
    NumPy composition's own probe by up to 4e-2 after two epochs (100^2 with
    an 80^2 probe; 256^2 + mask 2e-3, 384^2 4e-3) -- float32 rounding then
    decides the result.  From 0.8 psi_true + 0.1 the same change moves it by
    at most 7e-5 on every shape here."""
    return (0.8 * psi_true + 0.1).astype(np.complex64)


def _run(tp, data, scan, psi0, probe, model, mask, *, epochs=2, cg_iter=2,
         step=1.0, num_gpu=0, **kw):
    N = len(scan)
    eo = (tp.ExitWaveOptions(measured_pixels=mask, noise_model=model)
          if mask is not None else
          tp.ExitWaveOptions(measured_pixels=np.ones(probe.shape[-2:], bool),
                             noise_model=model))
    params = tp.PtychoParameters(
        probe=probe.copy(), psi=psi0.copy(), scan=scan.copy(),
        algorithm_options=tp.CgradOptions(num_batch=1, cg_iter=cg_iter,
                                          num_iter=epochs, step_length=step,
                                          batch_method="contiguous"),
        probe_options=tp.ProbeOptions(init_rescale_from_measurements=False),
        object_options=tp.ObjectOptions(), exitwave_options=eo)
    if num_gpu != 0:
        return tp.reconstruct(data, params, num_gpu=num_gpu)
    with tp.Reconstruction(data, params, order=np.arange(N),
                           batches=[np.arange(N)], **kw) as ctx:
        ctx.iterate(epochs)
        return ctx.get_result()


@pytest.mark.parametrize("model,masked", MODES)
@pytest.mark.parametrize("det,pw,S,N", [
    (256, 256, 1, 6), (256, 256, 2, 5), (512, 512, 2, 3), (128, 128, 1, 8),
    (384, 384, 1, 3), (100, 80, 1, 6), (256, 192, 2, 4)])
def test_cgrad_models_vs_composition(tp, model, masked, det, pw, S, N):
    """Every gradient route (256^2 resident, 512^2 split, 128^2 whole tile,
    prime-factor, unfused, pw < det) under gaussian+mask, poisson and
    poisson+mask, NaN counts at the unmeasured pixels."""
    mask = cm.detector_mask(det) if masked else None
    scan, psi_true, probe, data = _problem(tp, det, pw, S, N, det + N, mask)
    psi0 = _start(psi_true)
    got = _run(tp, data, scan, psi0, probe, model, mask)
    state = dict(psi=psi0.copy(), probe=probe.copy(), scan=scan.copy(),
                 costs=[])
    for _ in range(2):
        state = cm.cgrad(state, data, [np.arange(N)], detector_shape=det,
                         model=model, mask=mask, cg_iter=2)
    assert np.all(np.isfinite(got.psi)) and np.all(np.isfinite(got.probe))
    np.testing.assert_allclose(np.array(got.algorithm_options.costs),
                               np.array(state["costs"]), rtol=2e-3)
    assert_close(got.psi, state["psi"], normwise=2e-3, maxabs=2e-2, what="psi")
    assert_close(got.probe, state["probe"], normwise=2e-3, maxabs=2e-2,
                 what="probe")


def _searches(tp, monkeypatch, data, scan, psi0, probe, model, mask, **kw):
    import importlib
    C = importlib.import_module("tike_amd.ptycho.solvers.cgrad")
    monkeypatch.setattr(C, "USE_GRAPHS", False)
    used = []
    real = C._cg_device

    def spy(*a, **k):
        r = real(*a, **k)
        used.append((bool(k.get("linear")), r is not None))
        return r

    monkeypatch.setattr(C, "_cg_device", spy)
    out = {}
    for name, linear, on_device in (("linear", True, True),
                                    ("trials", False, True),
                                    ("host", False, False)):
        monkeypatch.setattr(C, "LINEAR_LINE_SEARCH", linear)
        monkeypatch.setattr(C, "DEVICE_LINE_SEARCH", on_device)
        del used[:]
        out[name] = _run(tp, data, scan, psi0, probe, model, mask, **kw)
        out[name + "_used"] = list(used)
    return out


@pytest.mark.parametrize("det,S,N", [(128, 1, 8), (256, 2, 6), (512, 1, 3)])
def test_cgrad_poisson_mask_searches_agree(tp, monkeypatch, det, S, N):
    mask = cm.detector_mask(det)
    scan, psi_true, probe, data = _problem(tp, det, det, S, N, det + 1, mask)
    r = _searches(tp, monkeypatch, data, scan, _start(psi_true),
                  probe, "poisson", mask)
    assert r["linear_used"] and all(u == (True, True)
                                    for u in r["linear_used"]), r
    assert r["trials_used"] and all(not lin and ok
                                    for lin, ok in r["trials_used"]), r
    assert not r["host_used"]
    for b in ("trials", "host"):
        np.testing.assert_allclose(
            np.array(r["linear"].algorithm_options.costs),
            np.array(r[b].algorithm_options.costs), rtol=2e-5)
        assert_close(r["linear"].psi, r[b].psi, normwise=2e-5, maxabs=2e-4,
                     what="psi " + b)
        assert_close(r["linear"].probe, r[b].probe, normwise=2e-5,
                     maxabs=2e-4, what="probe " + b)


def test_cgrad_poisson_nearly_converged_linear_search_still_steps(
        tp, monkeypatch):
    """Close to the solution the poisson totals carry a large offset; the
    all-at-once search forms each candidate as a difference from x, so it
    still takes a step whenever the float64 search finds one."""
    import importlib
    C = importlib.import_module("tike_amd.ptycho.solvers.cgrad")
    monkeypatch.setattr(C, "USE_GRAPHS", False)
    det, N = 256, 6
    mask = cm.detector_mask(det)
    scan, psi_true, probe, data = _problem(tp, det, det, 1, N, 11, mask)
    rng = np.random.default_rng(5)
    psi0 = (psi_true * (1 + 3e-4 * (rng.random(psi_true.shape) - 0.5))
            ).astype(np.complex64)
    used = []
    real = C._cg_device

    def spy(*a, **k):
        r = real(*a, **k)
        used.append((bool(k.get("linear")), r is not None))
        return r

    monkeypatch.setattr(C, "_cg_device", spy)
    got = _run(tp, data, scan, psi0, probe, "poisson", mask, epochs=1,
               cg_iter=1)
    # the float64 search along the same direction (the composition's)
    d64 = data.astype(np.float64)
    s = scan
    p64 = probe.astype(np.complex128)
    f = lambda x: float(np.mean(cm.cost_each(
        "poisson", d64, np.sum(np.abs(cm.ops.ptycho_fwd(
            p64, s, x, det).astype(np.complex128))**2, axis=(1, 2)), mask)))
    g = cm.grad_psi("poisson", d64, psi0, s, probe, det, mask)
    x0 = psi0.astype(np.complex128)
    f0 = f(x0)
    accepts = [f(x0 - 2.0**-k * g) < f0 for k in range(16)]
    # the problem is one where the float64 search decreases the cost ...
    assert any(accepts), "precondition: the float64 search finds a step"
    # ... and the product's all-at-once search, on its own gradient, takes a
    # step too -- one that lowers the float64 cost
    assert used and used[0] == (True, True), used
    assert not np.array_equal(got.psi, psi0), "the linear search took no step"
    assert f(got.psi.astype(np.complex128)) < f0


def _entry_problem(tp, det, S, N, model, seed=2):
    import torch
    mask = cm.detector_mask(det)
    scan, psi_true, probe, data = _problem(tp, det, det, S, N, seed, mask)
    psi = (psi_true * 0.9).astype(np.complex64)
    # a search direction: the model's descent direction, scaled so that the
    # longest step moves psi by about 10 %
    g = cm.grad_psi(("gaussian", "poisson")[model], data, psi, scan, probe,
                    det, mask)
    d = (-0.2 * np.linalg.norm(psi) / np.linalg.norm(g) * g).astype(
        np.complex64)
    dev = "cuda"
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(mask=mask, scan=scan, probe=probe, data=data, psi=psi, d=d,
                t=dict(psi=T(psi), d=T(d), xs=T(np.zeros_like(psi)),
                       probe=T(probe[0, 0]), scan=T(scan), data=T(data),
                       mask=T(mask.astype(np.uint8))))


def _linear_call(P, det, S, N, model, stage, state, sums, masked=True,
                 old=False):
    import torch
    import tike_amd._arrays as A
    from tike_amd._lib import check, lib
    from tike_amd.operators.propagation import fft_scales
    t = P["t"]
    H, W = P["psi"].shape[-2:]
    if "far_a" not in P:
        P["far_a"] = torch.empty((N, 1, S, det, det), dtype=torch.complex64,
                                 device="cuda")
        P["far_b"] = torch.empty_like(P["far_a"])
        P["costs_k"] = torch.zeros(17 * N + 1, dtype=torch.float32,
                                   device="cuda")
    args = (0, A.ptr(t["psi"]), A.ptr(t["d"]), A.ptr(t["xs"]),
            A.ptr(t["probe"]), A.ptr(t["scan"]), A.ptr(t["data"]), 0,
            A.ptr(P["far_a"]), 0, A.ptr(P["far_b"]), A.ptr(P["costs_k"]), N,
            N, S, det, H, W, fft_scales(det, "ortho")[0], float(N),
            A.ptr(state), stage, A.ptr(sums))
    if old:
        check(lib.tike_cgrad_line_search_linear(*args, A.stream_ptr()), "old")
    else:
        nm = int(P["mask"].sum()) if masked else det * det
        check(lib.tike_cgrad_line_search_linear_masked(
            *args, A.ptr(t["mask"]) if masked else None, model, nm,
            A.stream_ptr()), "new")


@pytest.mark.parametrize("model", [0, 1])
@pytest.mark.parametrize("det", [128, 256])
def test_linear_masked_entry_row_sums_vs_numpy(tp, model, det):
    """The 17 row sums of one search (stage 1: x and 8 steps; stage 3: 8
    more) against float64 NumPy costs of x + s d; poisson rows 1..16 are
    differences from x."""
    import torch
    S, N = 1, 3
    P = _entry_problem(tp, det, S, N, model)
    step = 0.5
    state = torch.tensor([0.0, step, 0.0, 0.0, 0.0], dtype=torch.float64,
                         device="cuda")
    sums = torch.zeros(17, dtype=torch.float64, device="cuda")
    _linear_call(P, det, S, N, model, 1, state, sums)
    rows = sums.cpu().numpy().copy()
    state[1] = step / 256
    _linear_call(P, det, S, N, model, 3, state, sums)
    rows[9:] = sums.cpu().numpy()[9:]
    name = ("gaussian", "poisson")[model]
    d64 = P["data"].astype(np.float64)
    p64 = P["probe"].astype(np.complex128)

    # the far plane is linear in the object: F(x + s d) = A + s B, formed in
    # float64 from the two forward passes (a float32 forward of x + s d
    # would round away the small differences of the short steps)
    fa = cm.ops.ptycho_fwd(p64, P["scan"], P["psi"], det).astype(np.complex128)
    fb = cm.ops.ptycho_fwd(p64, P["scan"], P["d"], det).astype(np.complex128)

    def costs(s_):
        inten = np.sum(np.abs(fa + s_ * fb)**2, axis=(1, 2))
        return cm.cost_each(name, d64, inten, P["mask"])

    c0 = costs(0.0)
    want = [c0.sum()]
    for k in range(16):
        ck = costs(step * 2.0**-k)
        want.append((ck - c0).sum() if model else ck.sum())
    want = np.array(want)
    # every row against its own magnitude (poisson rows 1..16 are the
    # differences from x, down to 1e-6 of the plain total in row 0 at the
    # short steps), with an absolute floor of 2e-10 of that total: three
    # orders below the float32 rounding of a plain total, which is what the
    # difference form is for.  (Below ~1e-4 of the total the float32 sums of
    # sign-mixed per-pixel differences limit the rows to ~1e-10 of it.)
    floor = 2e-10 * abs(want[0])
    err = np.abs(rows - want)
    assert np.all(err < 1e-5 * np.abs(want) + floor), (err / np.abs(want), want)


@pytest.mark.parametrize("det", [128, 256])
def test_old_linear_entry_equals_new_with_null_mask(tp, det):
    import torch
    S, N = 1, 3
    P = _entry_problem(tp, det, S, N, 0)
    rows = []
    for old in (True, False):
        state = torch.tensor([0.0, 0.5, 0.0, 0.0, 0.0], dtype=torch.float64,
                             device="cuda")
        sums = torch.zeros(17, dtype=torch.float64, device="cuda")
        P["t"]["data"] = torch.nan_to_num(P["t"]["data"], nan=1.0)
        _linear_call(P, det, S, N, 0, 1, state, sums, masked=False, old=old)
        rows.append(sums.cpu().numpy())
    # (the per-pattern rows are float atomics: equal up to their order)
    np.testing.assert_allclose(rows[0], rows[1], rtol=1e-6)


def test_cgrad_explicit_all_true_mask_equals_default(tp):
    det, N = 256, 5
    scan, psi_true, probe, data = _problem(tp, det, det, 2, N, 9, None)
    psi0 = _start(psi_true)
    a = _run(tp, data, scan, psi0, probe, "gaussian", None)
    b = _run(tp, data, scan, psi0, probe, "gaussian", np.ones((det, det), bool))
    np.testing.assert_allclose(np.array(a.algorithm_options.costs),
                               np.array(b.algorithm_options.costs), rtol=1e-6)
    assert_close(a.psi, b.psi, normwise=1e-6, maxabs=1e-5, what="psi")


def test_cgrad_poisson_mask_u16_and_host_data(tp):
    det, N = 256, 6
    mask = cm.detector_mask(det)
    scan, psi_true, probe, data = _problem(tp, det, det, 1, N, 13, None)
    counts = np.rint(np.minimum(data, 60000)).astype(np.uint16)
    psi0 = _start(psi_true)
    f32 = np.where(mask, counts.astype(np.float32), np.nan).astype(np.float32)
    a = _run(tp, counts, scan, psi0, probe, "poisson", mask)
    b = _run(tp, f32, scan, psi0, probe, "poisson", mask)
    c = _run(tp, f32, scan, psi0, probe, "poisson", mask, data_on_host=True)
    for x, y, tol in ((a, b, 1e-4), (b, c, 1e-6)):
        np.testing.assert_allclose(np.array(x.algorithm_options.costs),
                                   np.array(y.algorithm_options.costs),
                                   rtol=tol)
    assert_close(a.psi, b.psi, normwise=1e-4, maxabs=1e-3, what="u16 psi")
    assert_close(b.psi, c.psi, normwise=1e-6, maxabs=1e-5, what="host psi")


def test_cgrad_poisson_mask_two_ranks_match_one(tp, monkeypatch):
    det, N = 256, 8
    mask = cm.detector_mask(det)
    scan, psi_true, probe, data = _problem(tp, det, det, 1, N, 17, mask)
    psi0 = _start(psi_true)
    one = _run(tp, data, scan, psi0, probe, "poisson", mask, num_gpu=None)
    monkeypatch.setenv("TIKE_AMD_OVERSUBSCRIBE", "1")
    two = _run(tp, data, scan, psi0, probe, "poisson", mask, num_gpu=2)
    np.testing.assert_allclose(np.array(two.algorithm_options.costs),
                               np.array(one.algorithm_options.costs),
                               rtol=1e-3)
    assert_close(two.psi, one.psi, normwise=1e-3, maxabs=1e-2, what="psi")
    assert_close(two.probe, one.probe, normwise=1e-3, maxabs=1e-2,
                 what="probe")


def test_cgrad_poisson_mask_deterministic_children_bit_identical(tmp_path):
    child = os.path.join(os.path.dirname(__file__), "_cgrad_models_child.py")
    env = dict(os.environ, TIKE_DETERMINISTIC="1")
    outs = []
    for k in range(2):
        out = tmp_path / f"run{k}.npz"
        subprocess.run([sys.executable, child, str(out)], env=env, check=True,
                       timeout=300)
        outs.append(np.load(out))
    for key in outs[0].files:
        np.testing.assert_array_equal(outs[0][key], outs[1][key], err_msg=key)
