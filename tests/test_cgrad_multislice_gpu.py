"""Multislice cgrad on the GPU: `tike_slice_step_back` against the float64
model (tests/cgrad_multislice.py), the gradient of a whole chunk on both
routes, the solver against the model's cgrad, and the host plumbing (host-kept
data, 16-bit counts, the periodic rescale, two ranks)."""
import importlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cgrad_multislice as ms
import fly_scan as fs
from util import COST_RTOL, OP_NORMWISE, SOLVER_NORMWISE, relerr

pytestmark = pytest.mark.gpu

NEVER = 1 << 30


@pytest.fixture(scope="module")
def tp():
    import tike_amd.ptycho as m
    return m


# ------------------------------------------------------------------ the kernel
KERNEL_CASES = [(3, 1, 128), (2, 3, 128), (3, 2, 256), (2, 8, 256)]
# (512^2 is not built: the entry answers TIKE_ERR_UNSUPPORTED there)


def _kernel_case(nscan, S, det):
    """Random inputs and the model's two outputs.  The positions: the first
    allowed corner (three positions), the last allowed corner -- both take the
    vector gather -- and the corner one pixel past it, floor = H - det, whose
    trailing bilinear taps leave the image: the clamped gather."""
    rng = np.random.default_rng(det + S)
    H = W = det + 37
    c = lambda *shape: (rng.standard_normal(shape)
                        + 1j * rng.standard_normal(shape)).astype(np.complex64)
    G, beam, psi = c(nscan, S, det, det), c(nscan, S, det, det), c(H, W)
    scan = np.array([[1.3, 1.6], [H - det - 1 + 0.4, W - det - 1 + 0.7],
                     [H - det + 0.25, W - det + 0.5]], np.float32)[-nscan:]
    Hp = ms.propagator(det)
    g = ms._ifft2(G.astype(np.complex128))
    objproj, w = ms.step_back(g, scan, psi, beam.astype(np.complex128))
    return G, beam, psi, scan, Hp, objproj, ms.fresnel_adj(w, Hp)


def _step_back(G, beam, psi, scan, Hp):
    """The kernel fed as the issue asks: work = inverse pass 1 of G; returns
    (objproj, Fr^H(conj(patch) g) finished by the adjoint column passes and an
    inverse pass 2, and the device arrays for the checks of the caller)."""
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    from tike_amd.operators.propagation import fft_scales
    dev = torch.device("cuda")
    nscan, S, det = G.shape[0], G.shape[1], G.shape[-1]
    H, W = psi.shape
    fwd_scale, inv_scale = fft_scales(det, "ortho")
    st = A.stream_ptr()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    d = dict(G=t(G), beam=t(beam), psi=t(psi), scan=t(scan),
             prop=t(Hp.astype(np.complex64)))
    d["work"] = torch.empty_like(d["G"])
    check(lib.tike_fft2_pass1(A.ptr(d["G"]), A.ptr(d["work"]), nscan * S, det,
                              1, st), "inverse pass 1")
    keep = {k: d[k].clone() for k in ("work", "beam", "psi")}
    d["objproj"] = torch.full((nscan, det, det), 7.0, dtype=torch.complex64,
                              device=dev)
    d["far1"] = torch.full_like(d["G"], 7.0)
    check(lib.tike_slice_step_back(
        A.ptr(d["work"]), A.ptr(d["psi"]), A.ptr(d["scan"]), A.ptr(d["beam"]),
        A.ptr(d["objproj"]), A.ptr(d["far1"]), nscan, S, det, H, W, inv_scale,
        st), "tike_slice_step_back")
    for k, v in keep.items():
        assert torch.equal(torch.view_as_real(v), torch.view_as_real(d[k])), k
    back = torch.empty_like(d["G"])
    check(lib.tike_fresnel_colpass(A.ptr(d["far1"]), A.ptr(d["prop"]), 1,
                                   A.ptr(back), nscan * S, det, fwd_scale, st),
          "adjoint column passes")
    check(lib.tike_fft2_pass2_inplace(A.ptr(back), nscan * S, det, 1,
                                      inv_scale, st), "inverse pass 2")
    return d, back


@pytest.mark.parametrize("nscan,S,det", KERNEL_CASES)
def test_kernel_vs_float64_model(nscan, S, det):
    import torch
    G, beam, psi, scan, Hp, want_proj, want_back = _kernel_case(nscan, S, det)
    d, back = _step_back(G, beam, psi, scan, Hp)
    again, back2 = _step_back(G, beam, psi, scan, Hp)
    for a, b in ((d["objproj"], again["objproj"]), (d["far1"], again["far1"]),
                 (back, back2)):
        assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))
    # without a projection (objproj NULL, the beams unread): the same wave
    from tike_amd import _arrays as A
    from tike_amd._lib import check, lib
    far1 = torch.full_like(d["far1"], 7.0)
    H, W = psi.shape
    check(lib.tike_slice_step_back(
        A.ptr(d["work"]), A.ptr(d["psi"]), A.ptr(d["scan"]), None, None,
        A.ptr(far1), nscan, S, det, H, W, 1.0 / det, A.stream_ptr()),
        "tike_slice_step_back without objproj")
    assert torch.equal(torch.view_as_real(far1), torch.view_as_real(d["far1"]))
    got_proj, got_back = d["objproj"].cpu().numpy(), back.cpu().numpy()
    assert np.all(np.isfinite(got_proj)) and np.all(np.isfinite(got_back))
    e_proj, e_back = relerr(got_proj, want_proj), relerr(got_back, want_back)
    worst = max(relerr(got_back[n], want_back[n]) for n in range(nscan))
    print(f"{(nscan, S, det)}: objproj {e_proj:.2e}, step back {e_back:.2e} "
          f"(worst position {worst:.2e})")
    assert e_proj <= OP_NORMWISE
    assert e_back <= OP_NORMWISE and worst <= OP_NORMWISE


def test_kernel_without_positions_and_bad_arguments():
    import torch

    from tike_amd import _arrays as A
    from tike_amd._lib import ERR_ARG, ERR_UNSUPPORTED, lib
    dev = torch.device("cuda")
    det, S = 128, 1
    z = lambda *shape: torch.full(shape, 3.0, dtype=torch.complex64, device=dev)
    work, beam, far1 = z(1, S, det, det), z(1, S, det, det), z(1, S, det, det)
    objproj, psi = z(1, det, det), z(det + 8, det + 8)
    scan = torch.full((1, 2), 2.5, device=dev)
    st = A.stream_ptr()
    fn = lib.tike_slice_step_back
    ok = [A.ptr(work), A.ptr(psi), A.ptr(scan), A.ptr(beam), A.ptr(objproj),
          A.ptr(far1), 1, S, det, det + 8, det + 8, 1.0, st]

    def call(**change):
        args = list(ok)
        for k, v in change.items():
            args[int(k[1:])] = v
        return fn(*args)

    assert call(a6=0) == 0
    torch.cuda.synchronize()
    assert bool((objproj == 3).all()) and bool((far1 == 3).all())
    for i in (0, 1, 2, 3, 5):  # (objproj alone may be NULL)
        assert call(**{f"a{i}": None}) == ERR_ARG
    assert call(a7=0) == ERR_ARG
    assert call(a7=9) == ERR_UNSUPPORTED
    assert call(a8=64) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((objproj == 3).all()) and bool((far1 == 3).all())


# ------------------------------------------------- the gradient of a chunk
def parameters(tp, P, model, mask, recover_probe, epochs=2, cg_iter=2,
               num_batch=1, **options):
    pw = P["probe"].shape[-1]
    eo = tp.ExitWaveOptions(
        measured_pixels=mask if mask is not None else np.ones((pw, pw), bool),
        noise_model=model)
    optics = dict(probe_wavelength=ms.WAVELENGTH,
                  probe_FOV_lengths=(pw * ms.PIXEL, pw * ms.PIXEL))
    return tp.PtychoParameters(
        probe=P["probe0"].copy(), psi=P["psi0"].copy(), scan=P["scan"].copy(),
        algorithm_options=tp.CgradOptions(num_batch=num_batch, cg_iter=cg_iter,
                                          num_iter=epochs, step_length=1.0,
                                          batch_method="contiguous",
                                          **options),
        # (the optics travel in ProbeOptions: a probe that is not recovered
        # keeps them and starts updating at an epoch that never comes)
        probe_options=tp.ProbeOptions(
            init_rescale_from_measurements=False,
            update_start=0 if recover_probe else NEVER, **optics),
        object_options=tp.ObjectOptions(
            multislice_propagation_distance=ms.DISTANCE),
        exitwave_options=eo)


GRADIENT_CASES = {
    # name: (problem, fused route?)
    "general32": (dict(obj=72, pw=32, S=2, D=2, N=5, seed=5), False),
    "general64": (dict(obj=104, pw=64, S=2, D=3, N=4, seed=6), False),
    "fused128": (dict(obj=170, pw=128, S=2, D=2, N=5, seed=7), True),
    "fused256": (dict(obj=300, pw=256, S=2, D=3, N=4, seed=8), True),
}
_WANT = {}


def _gradient_want(name, model, use_mask):
    """The model's cost and gradients of a GRADIENT_CASES problem at its
    first iterates, on integer counts; computed once."""
    key = (name, model, use_mask)
    if key not in _WANT:
        if name not in _WANT:
            P = ms.problem(**GRADIENT_CASES[name][0])
            # integer counts, the same values as float32 and as uint16
            P["counts"] = np.round(40 * P["data"] / P["data"].mean()).astype(
                np.uint16)
            _WANT[name] = P
        P = _WANT[name]
        pw = P["probe"].shape[-1]
        mask = fs.block_mask(pw) if use_mask else None
        d = P["counts"].astype(np.float64)
        c = ms.cost(model, d, P["psi0"], P["scan"], P["probe0"], P["H"], mask)
        _WANT[key] = (c, *ms.gradients(model, d, P["psi0"], P["scan"],
                                       P["probe0"], P["H"], mask))
    return _WANT[name], _WANT[key]


@pytest.mark.parametrize("name", sorted(GRADIENT_CASES))
def test_chunk_gradient_vs_float64_model(tp, name, monkeypatch):
    """Both models, with and without the mask, float32 and uint16 counts:
    cost to COST_RTOL, object and probe gradient to OP_NORMWISE; a chunk
    override that splits the positions into two chunks agrees to 1e-6."""
    import torch

    C = importlib.import_module("tike_amd.ptycho.solvers.cgrad")
    from tike_amd.ptycho.solvers import lstsq as L
    _, fused = GRADIENT_CASES[name]
    P, _ = _gradient_want(name, "gaussian", False)
    N, pw = len(P["scan"]), P["probe"].shape[-1]
    mask_h = fs.block_mask(pw)
    for model in ("gaussian", "poisson"):
        for use_mask in (False, True):
            _, (c_want, gpsi_want, gprobe_want) = _gradient_want(
                name, model, use_mask)
            mask = mask_h if use_mask else None
            for u16 in (False, True):
                counts = P["counts"].copy()
                if u16 and use_mask:
                    counts[:, ~mask_h] = 65535  # counts that must not be read
                data = counts if u16 else (
                    fs.masked(counts.astype(np.float32), mask_h)
                    if use_mask else counts.astype(np.float32))
                params = parameters(tp, P, model, mask, True)
                with tp.Reconstruction(data, params, order=np.arange(N),
                                       batches=[np.arange(N)],
                                       spatial_sort=False) as ctx:
                    assert ctx.data.dtype == (torch.uint16 if u16 else
                                              torch.float32)
                    p = ctx.parameters
                    cm = C._cost_model(p.exitwave_options, pw)
                    from tike_amd.operators.multislice import fused_slices
                    assert fused_slices(pw, pw, p.probe.shape[-3]) == fused
                    runs = []
                    for chunk in (None, (N + 1) // 2):
                        monkeypatch.setattr(L, "CHUNK_POSITIONS_OVERRIDE",
                                            chunk)
                        total, gpsi, gprobe = C._multislice_cost_and_grad(
                            ctx.operator, ctx.comm, ctx.data, p.psi, p.scan,
                            p.probe, 0, N, want_psi=True, want_probe=True,
                            want_grad=True, cm=cm)
                        cost_only = C._multislice_cost_and_grad(
                            ctx.operator, ctx.comm, ctx.data, p.psi, p.scan,
                            p.probe, 0, N, want_psi=False, want_probe=False,
                            want_grad=False, cm=cm)
                        assert cost_only[1] is None and cost_only[2] is None
                        runs.append((float(total) / N, gpsi.cpu().numpy(),
                                     gprobe.cpu().numpy(),
                                     float(cost_only[0]) / N))
                    monkeypatch.setattr(L, "CHUNK_POSITIONS_OVERRIDE", None)
                (c, gpsi, gprobe, c_probe), split = runs
                tag = (name, model, use_mask, u16)
                print(tag, f"cost {abs(c - c_want) / abs(c_want):.2e} object "
                      f"{relerr(gpsi, gpsi_want):.2e} probe "
                      f"{relerr(gprobe, gprobe_want):.2e}; two chunks: object "
                      f"{relerr(split[1], gpsi):.2e} probe "
                      f"{relerr(split[2], gprobe):.2e}")
                assert gpsi.shape == P["psi0"].shape
                assert gprobe.shape == P["probe0"].shape
                assert abs(c - c_want) <= COST_RTOL * abs(c_want), tag
                assert abs(c_probe - c_want) <= COST_RTOL * abs(c_want), tag
                assert relerr(gpsi, gpsi_want) <= OP_NORMWISE, tag
                assert relerr(gprobe, gprobe_want) <= OP_NORMWISE, tag
                for d in range(gpsi.shape[0]):  # every slice on its own
                    assert relerr(gpsi[d], gpsi_want[d]) <= OP_NORMWISE, tag
                assert abs(split[0] - c) <= 1e-6 * abs(c), tag
                assert relerr(split[1], gpsi) <= 1e-6, tag
                assert relerr(split[2], gprobe) <= 1e-6, tag


def test_step_back_lever_and_general_route_agree_at_128(tp, monkeypatch):
    """The one-launch step back, the three launches it replaces and the
    general operators form the same gradient (1e-4: three float32 routes)."""
    C = importlib.import_module("tike_amd.ptycho.solvers.cgrad")
    P, _ = _gradient_want("fused128", "poisson", True)
    N, pw = len(P["scan"]), P["probe"].shape[-1]
    mask = fs.block_mask(pw)
    data = fs.masked(P["counts"].astype(np.float32), mask)
    out = []
    with tp.Reconstruction(data, parameters(tp, P, "poisson", mask, True),
                           order=np.arange(N), batches=[np.arange(N)],
                           spatial_sort=False) as ctx:
        p = ctx.parameters
        cm = C._cost_model(p.exitwave_options, pw)
        for fused, one_launch in ((True, True), (True, False), (False, True)):
            monkeypatch.setattr(C, "MULTISLICE_FUSED", fused)
            monkeypatch.setattr(C, "MULTISLICE_STEP_BACK_FUSED", one_launch)
            total, gpsi, gprobe = C._multislice_cost_and_grad(
                ctx.operator, ctx.comm, ctx.data, p.psi, p.scan, p.probe, 0,
                N, want_psi=True, want_probe=True, want_grad=True, cm=cm)
            out.append((float(total), gpsi.cpu().numpy(),
                        gprobe.cpu().numpy()))
    for other in out[1:]:
        print(f"cost {abs(other[0] - out[0][0]) / abs(out[0][0]):.2e} object "
              f"{relerr(other[1], out[0][1]):.2e} probe "
              f"{relerr(other[2], out[0][2]):.2e}")
        assert abs(other[0] - out[0][0]) <= 1e-4 * abs(out[0][0])
        assert relerr(other[1], out[0][1]) <= 1e-4
        assert relerr(other[2], out[0][2]) <= 1e-4


# ------------------------------------------------------------------ the solver
def _reconstruct(tp, P, model, mask, recover_probe, epochs=2, **kw):
    N = len(P["scan"])
    params = parameters(tp, P, model, mask, recover_probe, epochs=epochs)
    with tp.Reconstruction(P["data"], params, order=np.arange(N),
                           batches=[np.arange(N)], **kw) as ctx:
        ctx.iterate(epochs)
        return ctx.get_result()


@pytest.mark.parametrize("model,use_mask,recover_probe", ms.SOLVER_VARIANTS)
@pytest.mark.parametrize("case", sorted(ms.SOLVER_CASES))
def test_cgrad_multislice_vs_float64_model(tp, case, model, use_mask,
                                           recover_probe):
    """Two epochs of reconstruct-as-a-context with CgradOptions(cg_iter=2);
    every line-search decision of the model is clear
    (test_cgrad_multislice_cpu.py)."""
    state, P, mask = ms.run_model(case, model, use_mask, recover_probe)
    assert min(state["margins"]) >= ms.MIN_MARGIN
    got = _reconstruct(tp, P, model, mask, recover_probe)
    costs = np.array(got.algorithm_options.costs)
    print(case, model, use_mask, recover_probe,
          f"psi {relerr(got.psi, state['psi']):.2e} probe "
          f"{relerr(got.probe, state['probe']):.2e} costs",
          np.ravel(costs), "vs", np.ravel(state["costs"]))
    assert got.psi.shape == P["psi0"].shape
    np.testing.assert_allclose(costs, np.array(state["costs"]),
                               rtol=SOLVER_NORMWISE)
    assert relerr(got.psi, state["psi"]) <= SOLVER_NORMWISE
    assert relerr(got.probe, state["probe"]) <= SOLVER_NORMWISE
    if not recover_probe:
        assert np.array_equal(got.probe, P["probe0"])
    assert np.array_equal(got.scan, P["scan"])


def test_reconstruct_entry(tp):
    """`reconstruct()` itself takes the two-slice object."""
    case = "general32_d2"
    state, P, mask = ms.run_model(case, "gaussian", True, True)
    N = len(P["scan"])
    got = tp.reconstruct(P["data"], parameters(tp, P, "gaussian", mask, True),
                         order=np.arange(N), batches=[np.arange(N)])
    assert relerr(got.psi, state["psi"]) <= SOLVER_NORMWISE
    assert relerr(got.probe, state["probe"]) <= SOLVER_NORMWISE


@pytest.mark.parametrize("model", ["gaussian", "poisson"])
def test_costs_do_not_increase(tp, model):
    _, P, mask = ms.run_model("general32_d3", model, True, True)
    r = _reconstruct(tp, P, model, mask, True, epochs=4)
    costs = np.ravel(r.algorithm_options.costs)
    print(model, "costs", costs)
    assert len(costs) == 4 and np.all(np.diff(costs) <= 0)


def test_fused_and_general_route_agree_at_128(tp, monkeypatch):
    C = importlib.import_module("tike_amd.ptycho.solvers.cgrad")
    _, P, mask = ms.run_model("fused128_d2", "gaussian", True, True)
    a = _reconstruct(tp, P, "gaussian", mask, True)
    monkeypatch.setattr(C, "MULTISLICE_FUSED", False)
    b = _reconstruct(tp, P, "gaussian", mask, True)
    print(f"psi {relerr(b.psi, a.psi):.2e} probe {relerr(b.probe, a.probe):.2e}")
    assert relerr(b.psi, a.psi) <= 1e-4 and relerr(b.probe, a.probe) <= 1e-4
    np.testing.assert_allclose(b.algorithm_options.costs,
                               a.algorithm_options.costs, rtol=1e-4)


# ---------------------------------------------------------------- the plumbing
def test_data_on_host_equals_resident(tp):
    _, P, mask = ms.run_model("general32_d2", "gaussian", True, True)
    a = _reconstruct(tp, P, "gaussian", mask, True)
    b = _reconstruct(tp, P, "gaussian", mask, True, data_on_host=True)
    assert relerr(b.psi, a.psi) <= 1e-6 and relerr(b.probe, a.probe) <= 1e-6
    np.testing.assert_allclose(b.algorithm_options.costs,
                               a.algorithm_options.costs, rtol=1e-6)


def test_16_bit_counts_stay_16_bit(tp):
    import torch
    P = ms.problem(**ms.SOLVER_CASES["general32_d2"])
    counts = np.round(30 * P["data"]).astype(np.uint16)
    N = len(P["scan"])
    for kw in ({}, dict(data_on_host=True)):
        with tp.Reconstruction(counts, parameters(tp, P, "poisson", None, True),
                               order=np.arange(N), batches=[np.arange(N)],
                               **kw) as ctx:
            assert ctx.data.dtype == torch.uint16
            ctx.iterate(1)
            assert ctx.data.dtype == torch.uint16
            assert np.isfinite(ctx.get_result().algorithm_options.costs[-1][0])


def test_end_of_epoch_steps_take_several_slices(tp):
    """The periodic rescale (it refreshes the object preconditioner of every
    slice the epoch before) and the default object constraints: three epochs
    with a rescale after the second; costs keep falling."""
    _, P, mask = ms.run_model("general32_d3", "gaussian", False, True)
    N = len(P["scan"])
    params = parameters(tp, P, "gaussian", None, True, rescale_period=2)
    with tp.Reconstruction(P["data"], params, order=np.arange(N),
                           batches=[np.arange(N)]) as ctx:
        ctx.iterate(3)
        r = ctx.get_result()
    costs = np.ravel(r.algorithm_options.costs)
    print("costs", costs)
    assert r.psi.shape == P["psi0"].shape and np.all(np.isfinite(r.psi))
    assert np.all(np.isfinite(r.probe)) and np.all(np.isfinite(costs))
    assert r.object_options.preconditioner is not None
    assert np.all(np.diff(costs) < 0)


@pytest.mark.parametrize("D", [2, 3])
def test_rescale_leaves_the_cost_as_it_is(tp, D):
    """Removing the object / probe scale ambiguity under cgrad divides every
    slice by the norm and gives the probe the norm once per slice: the exit
    wave, and with it the cost, is unchanged (float32: 1e-5).  The
    single-slice rule (the probe takes the norm once) changes it."""
    from tike_amd.ptycho.object import remove_object_ambiguity
    from tike_amd.ptycho.ptycho import _apply_object_constraints
    from tike_amd.ptycho.solvers import update_preconditioners
    C = importlib.import_module("tike_amd.ptycho.solvers.cgrad")
    case = f"general32_d{D}"
    _, P, _ = ms.run_model(case, "gaussian", False, True)
    N = len(P["scan"])
    params = parameters(tp, P, "gaussian", None, True, rescale_period=1)
    with tp.Reconstruction(P["data"], params, order=np.arange(N),
                           batches=[np.arange(N)]) as ctx:
        p = ctx.parameters
        cm = C._cost_model(p.exitwave_options, P["probe"].shape[-1])

        def cost(psi, probe):
            return float(C._multislice_cost_and_grad(
                ctx.operator, ctx.comm, ctx.data, psi, p.scan, probe, 0, N,
                want_psi=False, want_probe=False, want_grad=False,
                cm=cm)[0]) / N

        before = cost(p.psi, p.probe)
        p = update_preconditioners(comm=ctx.comm, parameters=p,
                                   operator=ctx.operator, probe=False)
        pre = p.object_options.preconditioner
        psi0, probe0 = p.psi.clone(), p.probe.clone()
        # (one epoch on record: the rescale of period 1 is due)
        p.algorithm_options.costs.append([before])
        p = _apply_object_constraints(p)
        scale = float((psi0.abs().mean() / p.psi.abs().mean()))
        after = cost(p.psi, p.probe)
        wrong = cost(*remove_object_ambiguity(psi0, probe0, pre))
    print(f"D={D}: object divided by {scale:.4f}; cost {before:.6e} -> "
          f"{after:.6e}; with the probe scaled once {wrong:.6e}")
    assert abs(scale - 1) > 0.05  # the rescale did something
    assert abs(after - before) <= 1e-5 * abs(before)
    assert abs(wrong - before) > 1e-2 * abs(before)


# ------------------------------------------------------------------- two ranks
def _ranks(tmp_path, world):
    """Fresh child processes, one per rank (gloo, one GPU)."""
    here = os.path.dirname(os.path.abspath(__file__))
    store = tmp_path / f"store_{world}"
    outs = [str(tmp_path / f"out_{world}_{rank}.npz") for rank in range(world)]
    procs = [subprocess.Popen(
        [sys.executable, os.path.join(here, "_cgrad_multislice_child.py"),
         str(rank), str(world), str(store), outs[rank]],
        stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        for rank in range(world)]
    for proc in procs:
        out, err = proc.communicate(timeout=600)
        assert proc.returncode == 0, out[-2000:] + err[-4000:]
    return [np.load(o) for o in outs]


def test_two_ranks_match_one_rank(tmp_path):
    one, = _ranks(tmp_path, 1)
    two = _ranks(tmp_path, 2)
    assert list(one["shares"]) == [1, 8]
    assert list(two[0]["shares"]) == [1, 4]
    assert list(two[1]["shares"]) == [0, 4]  # an empty share
    for r in two:
        print(f"two ranks: psi {relerr(r['psi'], one['psi']):.2e} probe "
              f"{relerr(r['probe'], one['probe']):.2e}")
        assert relerr(r["psi"], one["psi"]) <= 1e-4
        assert relerr(r["probe"], one["probe"]) <= 1e-4
        np.testing.assert_allclose(r["costs"], one["costs"], rtol=1e-4)
        assert np.array_equal(r["scan"], one["scan"])
        assert np.array_equal(r["psi"], two[0]["psi"])
        assert np.array_equal(r["probe"], two[0]["probe"])
