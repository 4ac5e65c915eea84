#!/usr/bin/env python3
"""Launch for launch, bit for bit: the host-code counterpart of
tools/kernel_identity.py for `tike_amd.autograd` and for the solver code that
shares its multislice walk (not a test):

    python tools/launch_trace.py OUT.json [GROUP]   # in each of two trees
    python tools/launch_trace.py --compare A.json B.json

The first form starts a fresh child process under TIKE_DETERMINISTIC=1 that
wraps every `tike_*` function of `_lib._PROTOTYPES` on the loaded library and
runs every public function of `tike_amd.autograd` on the smallest shapes of
the test helpers that take every branch -- one chunk and three chunks
(`CHUNK_POSITIONS_OVERRIDE = 5`), the fused multislice shape also with each
lever flipped -- and then `solver_scenarios`: cgrad's multislice cost and
gradient, rpie's near-plane gradients of an object of slices and one
minibatch of lstsq's unfused route, each on the smallest shapes that take every
branch, and `detector_scenarios`: fly scans, binning, a background, a blur
and the near field through cgrad, `simulate`, the operator's cost and
`autograd.cost`.  GROUP ("autograd", "solver" or "detector") runs that group
alone.  Per scenario OUT.json holds the launches (the entry, null /
non-null for each pointer, the value of every other argument), the SHA-256 of
each output tensor (the solver scenarios run twice in the process: an output
whose bits differ between the two runs -- `tike_conv_adj` sums by float atomics
in either mode -- is recorded as "unstable" with its norm and one projection,
which `--compare` holds to UNSTABLE_RTOL) and the peak of
`torch.cuda.max_memory_allocated` above what was resident.  `--compare`
prints the first difference per scenario and exits non-zero on any.  A tree
without a built library borrows one through TIKE_AMD_LIB."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
LEVERS = (("autograd", "PASS1_TAKES_TABLE"),
          ("autograd", "TANGENT_FRESNEL_TWO_PASS"),
          ("autograd", "FIRST_SLICE_BY_CONV_TANGENT"),
          ("cgrad", "MULTISLICE_FUSED"), ("cgrad", "MULTISLICE_STEP_BACK_FUSED"))


UNSTABLE_RTOL = 1e-5
"""An output that is not bit-stable (float atomics) is held to this times its
norm, in the norm and in one fixed projection: float32 sums of some dozens of
terms in another order differ by a few 1e-7 of the norm."""


def same_output(u, v):
    if isinstance(u, list) and isinstance(v, list):
        bound = UNSTABLE_RTOL * max(u[1], v[1])
        return all(abs(p - q) <= bound for p, q in zip(u[1:], v[1:]))
    return u == v


def compare(a, b):
    a, b = (json.load(open(p)) for p in (a, b))
    bad = 0
    for key in sorted(set(a) | set(b)):
        x, y = a.get(key), b.get(key)
        if x and y and len(x["hashes"]) == len(y["hashes"]) and all(
                map(same_output, x["hashes"], y["hashes"])):
            y = dict(y, hashes=x["hashes"])
        if x == y:
            continue
        bad += 1
        if x is None or y is None:
            print(f"{key}: only in {'B' if x is None else 'A'}")
            continue
        for what in ("launches", "hashes", "peak"):
            u, v = x[what], y[what]
            if u != v and isinstance(u, list):
                k = next((k for k, (p, q) in enumerate(zip(u, v)) if p != q),
                         min(len(u), len(v)))
                u, v = (f"#{k} of {len(w)}: {w[k] if k < len(w) else 'end'}"
                        for w in (u, v))
            if u != v:
                print(f"{key}: {what}: A {u} | B {v}")
    print(f"{len(a)} scenarios in A, {len(b)} in B, {bad} differ")
    return int(bad > 0)


def solver_scenarios(record, C, L, dev):
    """The solver code that shares the multislice walk and the stored
    far-plane gradient stage, through names both trees have: cgrad's
    `_multislice_cost_and_grad`, rpie's `_get_nearplane_gradients` on objects
    of slices, and a minibatch of lstsq's unfused route.  The outputs hashed
    include what the calls write in place."""
    import importlib

    import cgrad_multislice as ms
    import fly_scan as fs
    import numpy as np
    import test_solvers_gpu as ts
    import torch

    import tike_amd._arrays as A
    import tike_amd.ptycho as tp
    from tike_amd.communicators import Comm
    from tike_amd.operators import Ptycho
    R = importlib.import_module("tike_amd.ptycho.solvers.rpie")
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    N = 7
    problems = {}

    def problem(pw, D):
        """(device psi0, scan, probe0, integer counts; operator keywords)"""
        if (pw, D) not in problems:
            obj = {32: 72, 128: 170, 256: 300}[pw]
            P = ms.problem(obj=obj, pw=pw, S=2, D=D, N=N, seed=pw + D)
            counts = np.round(40 * P["data"] / P["data"].mean()).astype(
                np.float32)
            problems[pw, D] = (
                [to(P[k]) for k in ("psi0", "scan", "probe0")] + [to(counts)],
                dict(probe_shape=pw, detector_shape=pw, nz=obj, n=obj,
                     probe_wavelength=ms.WAVELENGTH,
                     probe_FOV_lengths=(pw * ms.PIXEL, pw * ms.PIXEL),
                     multislice_propagation_distance=ms.DISTANCE))
        return problems[pw, D]

    def exitwave(model, pw):
        # gaussian on every pixel, poisson with a mask
        mask = fs.block_mask(pw) if model == "poisson" else np.ones(
            (pw, pw), dtype=bool)
        return tp.ExitWaveOptions(measured_pixels=mask, noise_model=model)

    def given(tensors):
        return [t for t in tensors if t is not None]

    wants = ((False, False, False), (True, True, True), (True, True, False),
             (True, False, True))  # want_grad, want_psi, want_probe

    def cgrad(label, pw, D, levers):
        (psi, scan, probe, counts), keywords = problem(pw, D)
        for model in ("gaussian", "poisson"):
            cm = C._cost_model(exitwave(model, pw), pw)
            for chunks in (0, 5):
                L.CHUNK_POSITIONS_OVERRIDE = chunks
                for grad, want_psi, want_probe in wants:
                    with Ptycho(**keywords) as op:
                        record(
                            f"cgrad {label} D={D} {model} chunk {chunks} "
                            f"grad={grad} psi={want_psi} probe={want_probe} "
                            f"{levers}",
                            lambda: given(C._multislice_cost_and_grad(
                                op, Comm(), counts, psi, scan, probe, 0, N,
                                want_psi=want_psi, want_probe=want_probe,
                                want_grad=grad, cm=cm)))
        L.CHUNK_POSITIONS_OVERRIDE = 0

    for D in (2, 3):
        for one_launch in (True, False):
            C.MULTISLICE_STEP_BACK_FUSED = one_launch
            cgrad("fused 128", 128, D, f"step back fused={one_launch}")
        C.MULTISLICE_STEP_BACK_FUSED = True
    cgrad("general 32", 32, 3, "")
    C.MULTISLICE_FUSED = False
    cgrad("general 128", 128, 3, "MULTISLICE_FUSED=False")
    C.MULTISLICE_FUSED = True

    def rpie(pw, model, recover_psi):
        (psi, scan, probe, counts), keywords = problem(pw, 2)
        eo = exitwave(model, pw)
        for chunks in (0, 5):
            L.CHUNK_POSITIONS_OVERRIDE = chunks

            def run():
                psi_num = torch.zeros_like(psi)
                terms = ((torch.zeros_like(scan), torch.zeros_like(scan))
                         if recover_psi else None)
                cost, probe_num = R._get_nearplane_gradients(
                    counts, psi, scan, probe, None, None, 0, N, Comm(),
                    psi_num, op=op, exitwave_options=eo,
                    recover_psi=recover_psi, recover_probe=True,
                    position_terms=terms)
                return [cost, probe_num, psi_num] + list(terms or ())

            with Ptycho(**keywords) as op:
                record(f"rpie {pw} D=2 {model} chunk {chunks} "
                       f"recover_psi={recover_psi}", run)
        L.CHUNK_POSITIONS_OVERRIDE = 0

    for pw, model in ((128, "gaussian"), (128, "poisson"), (256, "gaussian")):
        rpie(pw, model, True)  # (256^2 gaussian: the one-launch last slice)
    for model in ("gaussian", "poisson"):
        for recover_psi in (True, False):
            rpie(32, model, recover_psi)

    # lstsq's unfused route: the levers, the shape and the options of
    # test_general_shape_launches_equal_the_unfused_kernels, both models
    det, pw, S, n = 96, 64, 3, 9
    scan, psi, probe, ep, ew, data = ts._headline_problem(
        tp, det, S, n, seed=11, eigen=True, pw=pw)
    mask = np.random.default_rng(3).random((det, det)) > 0.1
    data = data.copy()
    data[:, ~mask] = np.nan
    scan, psi, probe, ep, ew = (A.to_device(x) for x in (scan, psi, probe, ep,
                                                        ew))
    data = A.to_device(data, np.float32)
    saved = L.GENERAL_FUSED, L.PFA_ROUTE
    L.GENERAL_FUSED = L.PFA_ROUTE = False
    for model in ("gaussian", "poisson"):
        eo = tp.ExitWaveOptions(measured_pixels=mask, noise_model=model,
                                unmeasured_pixels_scaling=0.9)

        def run():
            out = L._get_nearplane_gradients(
                data, psi, scan, probe, ep, ew, 0, n, Comm(), num_batch=2,
                exitwave_options=eo, op=op, recover_psi=True,
                recover_probe=True)
            return [L.object_upd_sum(out), out["m_probe_update"], out["chi0"],
                    out["costs"]]

        with Ptycho(probe_shape=pw, detector_shape=det, nz=psi.shape[-1],
                    n=psi.shape[-1]) as op:
            launched = [x[0] for x in record(f"lstsq unfused {model}",
                                             run)["launches"]]
        assert "tike_farplane_gradient" in launched and (
            "tike_poisson_steps" in launched) == (model == "poisson"), launched
    L.GENERAL_FUSED, L.PFA_ROUTE = saved


def detector_scenarios(record, L, dev):
    """What lies between the sample and the counts -- fly scans, binning, a
    background, a blur, the near field -- through names both trees have:
    `tp.reconstruct` (one epoch of cgrad, cg_iter 2), `tp.simulate`,
    `Ptycho.cost`, `Ptycho._compute_intensity`, `autograd.cost` and its
    backward, on the smallest problems of the test helpers; and one plain
    128^2 cgrad call."""
    import background as bg
    import binned as bn
    import blur as bl
    import fly_scan as fs
    import nearfield as nf
    import numpy as np
    import torch

    import tike_amd.operators as ops
    import tike_amd.ptycho as tp
    from tike_amd import autograd as ag
    from tike_amd.operators import nearfield as NF
    to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    host = lambda xs: [torch.from_numpy(np.ascontiguousarray(x)) for x in xs]

    def problems():
        """(label, problem, det, fly, keywords of reconstruct with the first
        guess of the third block (update -> keywords), keywords of the
        operator's and simulate's entries, the third block's name or None)"""
        none = lambda update: {}
        P = fs.problem(obj=96, pw=32, det=32, S=2, fly=2, nframe=12, seed=3,
                       amp=1.0, mix=0.3, dim=0.5)
        yield "fly2", P, 32, 2, none, {}, None
        for fly in bn.SOLVER_FLY:
            yield (f"binned fly{fly}", bn.problem(fly, **bn.SOLVER), 32, fly,
                   lambda update: dict(binning=bn.SOLVER["B"]),
                   dict(binning=bn.SOLVER["B"]), None)
        for case in ("fly1", "fly2"):
            fly = bl.SOLVER_CASES[case]["fly"]
            P = bg.solver_problem(case)
            yield (f"background {case}", P, 32, fly,
                   lambda update, P=P: dict(
                       background_options=tp.BackgroundOptions(
                           P["b0"].copy(), update=update)),
                   dict(background=P["background"]), "background")
            P = bl.solver_problem(case)
            yield (f"blur {case}", P, 32, fly,
                   lambda update, P=P: dict(blur_options=tp.BlurOptions(
                       P["k0"].copy(), update=update)),
                   dict(blur=P["kernel"]), "blur")
        for fly in (1, 2):
            P = nf.solver_problem(fly)
            yield (f"nearfield128 fly{fly}", P, 128, fly,
                   lambda update, P=P: dict(
                       nearfield_options=tp.NearFieldOptions(P["H"].copy())),
                   dict(nearfield=P["H"]), None)
        P = nf.problem(32, 2, 2, 6, seed=5)
        P.update(data=nf.simulate(32, P["probe"], P["scan"], P["psi"], 2,
                                  P["H"]).astype(np.float32),
                 psi0=np.ones_like(P["psi"]),
                 probe0=(0.9 * P["probe"]).astype(np.complex64))
        yield ("nearfield32 fly2", P, 32, 2,
               lambda update, P=P: dict(
                   nearfield_options=tp.NearFieldOptions(P["H"].copy())),
               dict(nearfield=P["H"]), None)

    def parameters(P, model, mask, recover_probe):
        return tp.PtychoParameters(
            probe=P["probe0"].copy(), psi=P["psi0"].copy(),
            scan=P["scan"].copy(),
            algorithm_options=tp.CgradOptions(
                num_batch=1, cg_iter=2, num_iter=1, step_length=1.0,
                batch_method="contiguous"),
            probe_options=tp.ProbeOptions(init_rescale_from_measurements=False)
            if recover_probe else None,
            object_options=tp.ObjectOptions(),
            exitwave_options=tp.ExitWaveOptions(measured_pixels=mask,
                                                noise_model=model))

    def solve(label, P, fly, options, third):
        """One epoch, over minibatches, noise models, chunks and what is
        recovered; uint16 counts once."""
        N, w = len(P["scan"]), P["data"].shape[-1]
        every, measured = np.ones((w, w), bool), np.nan_to_num(P["data"])
        noise = [("gaussian", every, measured),
                 ("poisson", fs.block_mask(w),
                  fs.masked(measured, fs.block_mask(w))),
                 ("gaussian u16", every,
                  np.round(measured).astype(np.uint16))]
        recover = [(False, None), (True, None)]
        if third:
            recover = [(p, u) for p, _ in recover for u in (True, False)]
        for nbatch in (1, 2):
            n = N // nbatch
            assert n % fly == 0, (label, n, fly)
            batches = [np.arange(i * n, (i + 1) * n) for i in range(nbatch)]
            # a full chunk of whole frames, then a partial one
            for chunk in (0, (n // fly // 2 + 1) * fly):
                L.CHUNK_POSITIONS_OVERRIDE = chunk
                for model, mask, data in noise:
                    for probe, update in recover:
                        if "u16" in model and (nbatch, probe) != (1, True):
                            continue

                        def run():
                            kw = options(update)
                            got = tp.reconstruct(
                                data, parameters(P, model.split()[0], mask,
                                                 probe),
                                fly=fly, order=np.arange(N), batches=batches,
                                **kw)
                            fitted = [getattr(o, dict(
                                background="background", blur="kernel")[third])
                                      for o in kw.values()] if third else []
                            return host([got.psi, got.probe, np.asarray(
                                got.algorithm_options.costs)] + fitted)

                        record(f"cgrad {label} batches {nbatch} chunk {chunk} "
                               f"{model} probe={probe} update={update}", run)
        L.CHUNK_POSITIONS_OVERRIDE = 0

    def entries(label, P, det, fly, kw):
        """simulate, the operator's two entries and autograd.cost."""
        pw = P["probe"].shape[-1]
        record(f"simulate {label}", lambda: host([tp.simulate(
            det, P["probe"], P["scan"], P["psi"], fly=fly, **kw)]))
        dkw = {k: (v if isinstance(v, int) else to(v)) for k, v in kw.items()}
        x = dict(psi=to(P["psi0"]), probe=to(P["probe0"]), scan=to(P["scan"]))
        w = P["data"].shape[-1]
        mask = fs.block_mask(w)
        counts = {"gaussian": (to(np.nan_to_num(P["data"])), None),
                  "poisson": (to(np.round(np.nan_to_num(P["data"])).astype(
                      np.uint16)), to(mask))}
        fitted = [k for k in ("background", "blur") if k in kw]
        with ops.Ptycho(det, pw, nz=P["psi"].shape[-2],
                        n=P["psi"].shape[-1]) as op:
            record(f"intensity {label}", lambda: list(op._compute_intensity(
                None, x["psi"], x["scan"], x["probe"], fly=fly, **dkw)))
            for model, (data, m) in counts.items():
                record(f"Ptycho.cost {label} {model}", lambda: [op.cost(
                    data, x["psi"], x["scan"], x["probe"], model=model,
                    fly=fly, **dkw)])
                up = to(np.random.default_rng(1).random(
                    data.shape[0]).astype(np.float32) + 0.5)
                for chunk in (0, (len(P["scan"]) // fly // 2 + 1) * fly):
                    L.CHUNK_POSITIONS_OVERRIDE = chunk
                    for names in (("psi", "probe", "scan") + tuple(fitted),
                                  tuple(fitted)):
                        if not names:
                            continue

                        def run():
                            leaves = {k: v.clone().requires_grad_(k in names)
                                      for k, v in {**x, **dkw}.items()
                                      if isinstance(v, torch.Tensor)}
                            out = ag.cost(
                                op, data, leaves["psi"], leaves["probe"],
                                leaves["scan"], model=model,
                                measured_pixels=m, fly=fly,
                                **{k: leaves.get(k, v)
                                   for k, v in dkw.items()})
                            return (out,) + torch.autograd.grad(
                                out, [leaves[k] for k in names],
                                grad_outputs=up)

                        record(f"autograd.cost {label} {model} chunk {chunk} "
                               f"wrt {','.join(names)}", run)
                L.CHUNK_POSITIONS_OVERRIDE = 0

    for label, P, det, fly, options, kw, third in problems():
        solve(label, P, fly, options, third)
        entries(label, P, det, fly, kw)
        if label.startswith("nearfield128"):
            NF.FUSED = False
            solve(label + " FUSED=False", P, fly, options, third)
            entries(label + " FUSED=False", P, det, fly, kw)
            NF.FUSED = True
    # the plain route, untouched
    P = fs.problem(obj=170, pw=128, det=128, S=2, fly=1, nframe=8, seed=1,
                   amp=1.0, mix=0.3, dim=0.5)
    solve("plain128", P, 1, lambda update: {}, None)


def child(out, only=None):
    import importlib

    import autograd_cost
    import autograd_eigen as ae
    import autograd_multislice as ams
    import numpy as np
    import test_autograd_gpu as tg
    import test_autograd_multislice_gpu as tm
    import torch
    import torch.autograd.forward_ad as fwAD

    import tike_amd.operators as ops
    from tike_amd import _lib, autograd as ag
    from tike_amd.ptycho.solvers import lstsq
    modules = dict(autograd=ag, cgrad=importlib.import_module(
        "tike_amd.ptycho.solvers.cgrad"))
    dev, trace, results = torch.device("cuda"), [], {}

    def wrap(name, fn, kinds):
        def call(*args):
            trace.append([name] + [
                int(bool(getattr(a, "value", a))) if k is ctypes.c_void_p else
                a for a, k in zip(args, kinds)])
            return fn(*args)
        return call

    for name, kinds in _lib._PROTOTYPES.items():
        setattr(_lib.lib, name, wrap(name, getattr(_lib.lib, name), kinds))

    def digests(outs):
        outs = [outs] if isinstance(outs, torch.Tensor) else list(outs)
        return [hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()
                for t in outs], outs

    def gist(t):
        """["unstable", norm, one fixed projection] of a tensor in float64:
        what `--compare` holds to UNSTABLE_RTOL x the norm."""
        v = t.detach().cpu().numpy().reshape(-1)
        v = v.view(v.real.dtype).astype(np.float64)
        return ["unstable", float(np.linalg.norm(v)),
                float(v @ np.cos(0.37 * np.arange(v.size)))]

    def record(key, fn, twice=False, strict=True):
        """twice: the call is made again and an output whose bits differ
        between the two is recorded as "unstable" with its `gist`, not by its
        hash (sums by float atomics in either mode: `tike_conv_adj`).  strict
        False: launches that differ between the two calls (what a process
        sets up once) are recorded as they are, those of the second call
        under "again", and `--compare` holds both trees to both."""
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before, trace[:] = torch.cuda.memory_allocated(), []
        outs = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        launches, (hashes, outs) = list(trace), digests(outs)
        if twice:
            trace[:] = []
            again = digests(fn())[0]
            assert trace == launches or not strict, key
            extra = {} if trace == launches else dict(again=list(trace))
            hashes = [a if a == b else gist(t)
                      for a, b, t in zip(hashes, again, outs)]
        results[key] = dict(launches=launches, peak=peak, hashes=hashes)
        results[key].update(extra if twice else {})
        return results[key]

    def shapes():
        """(label, operator keywords, host inputs by name, fly, functions)"""
        plain = (ag.intensity, ag.intensity_jvp, ag.gauss_newton_product)
        for N, S, pw, det, H, W, fly in (tg.CONFIG, tg.END_TO_END_CASES[6][:5]
                                         + tg.END_TO_END_CASES[6][4:]):
            c = ae.inputs(N, S, 0, 0, pw, H, W, seed=N + det)
            yield (f"plain{det}", dict(probe_shape=pw, detector_shape=det, nz=H,
                                       n=W),
                   {k: c[k] for k in ag._WRT}, fly, plain)
        eigen = (ag.intensity, ag.eigen_intensity_jvp,
                 ag.eigen_gauss_newton_product)
        for N, S, M, C, pw, det, H, fly in (ae.END_TO_END_CASES[0],
                                            ae.END_TO_END_CASES_MORE[1]):
            c = ae.inputs(N, S, M, C, pw, H, H, seed=N + det)
            c["eigen_probe"], c["eigen_weights"] = c["eigen"], c["weights"]
            yield (f"eigen{C}", dict(probe_shape=pw, detector_shape=det, nz=H,
                                     n=H),
                   {k: c[k] for k in ag._EIGEN_WRT if c[k] is not None}, fly,
                   eigen)
        slices = (ag.multislice_intensity, ag.multislice_intensity_jvp,
                  ag.multislice_gauss_newton_product)
        for label, (N, S, pw, obj, D, fly) in (
                ("general", tm.GENERAL), ("fused", tm.FUSED),
                ("fused3", ams.END_TO_END_CASES[3])):
            c = ams.case(N, S, pw, obj, D, fly)
            yield (label, dict(probe_shape=pw, detector_shape=pw, nz=obj, n=obj,
                               **ams.optics(pw)),
                   {k: c[k] for k in ag._WRT}, fly, slices)

    def scenarios(label, keywords, host, fly, functions):
        forward, jvp, product = functions
        det, frames = keywords["detector_shape"], host["scan"].shape[0] // fly
        rng = np.random.default_rng(frames + det)
        to = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        x = {k: to(v) for k, v in host.items()}
        d = {"d_" + k: to((rng.standard_normal(v.shape) + (
            1j * rng.standard_normal(v.shape) if np.iscomplexobj(v) else 0)
        ).astype(v.dtype)) for k, v in host.items()}
        g = to(rng.standard_normal((frames, det, det)).astype(np.float32))
        g2, up = g * g, to(rng.random(frames).astype(np.float32) + 0.5)
        counts = rng.poisson(20.0, (frames, det, det))
        args = [x[k] for k in ag._WRT]
        kw = dict(fly=fly, **{k: v for k, v in x.items() if k not in ag._WRT})
        dscan = dict(d_scan=d["d_scan"])

        def backward(model, names):
            leaves = {k: v.clone().requires_grad_(k in names)
                      for k, v in x.items()}
            out = model(*(leaves[k] for k in ag._WRT), fly=fly, **{
                k: leaves[k] for k in kw if k != "fly"})
            return (out,) + torch.autograd.grad(
                out, [leaves[k] for k in names],
                grad_outputs=g if out.ndim == 3 else up)

        def dual():
            with fwAD.dual_level():
                out = ag.intensity(op, *(fwAD.make_dual(x[k], d["d_" + k])
                                         for k in ag._WRT), fly=fly)
                return fwAD.unpack_dual(out)

        with ops.Ptycho(**keywords) as op:
            f = lambda fn: (lambda *a, **k: fn(op, *a, **k))
            calls = {
                "backward": lambda: backward(f(forward), tuple(x)),
                "backward scan": lambda: backward(f(forward), ("scan",)),
                "jvp": lambda: jvp(op, *args, **kw, **d),
                "jvp scan": lambda: jvp(op, *args, **kw, **dscan),
                "product": lambda: product(op, *args, **kw, **d, weight=g2,
                                           wrt=tuple(x)),
                "product scan": lambda: product(op, *args, **kw, **d,
                                                wrt=("scan",))}
            if "eigen_weights" not in x and host["psi"].shape[0] == 1:
                calls["dual"] = dual
            for model, data, mask in (
                    ("gaussian", to(counts.astype(np.float32)), None),
                    ("poisson", to(counts.astype(np.uint16)),
                     to(autograd_cost.module_gap_mask(det)))):
                ck = dict(kw, model=model, measured_pixels=mask)
                cost = lambda *a, ck=ck, data=data, **k: ag.cost(
                    op, data, *a, **{**ck, **k})
                calls.update({
                    f"cost {model}": lambda cost=cost: backward(cost,
                                                                tuple(x)),
                    f"cost_jvp {model}": lambda ck=ck, data=data: ag.cost_jvp(
                        op, data, *args, **ck, **d),
                    f"cost product {model}": lambda ck=ck, data=data:
                    ag.cost_gauss_newton_product(op, data, *args, **ck, **d,
                                                 upstream=up, wrt=tuple(x))})
            for key, fn in calls.items():
                record(f"{label}: {key}", fn)

    for shape in shapes() if only in (None, "autograd") else ():
        for chunks in (0, 5):
            lstsq.CHUNK_POSITIONS_OVERRIDE = chunks
            scenarios(f"{shape[0]} chunk {chunks}", *shape[1:])
        lstsq.CHUNK_POSITIONS_OVERRIDE = 0
        for module, lever in LEVERS if shape[0] == "fused" else ():
            value = getattr(modules[module], lever)
            setattr(modules[module], lever, not value)
            scenarios(f"fused {lever}={not value}", *shape[1:])
            setattr(modules[module], lever, value)
    twice = lambda key, fn: record(key, fn, twice=True)  # noqa: E731
    if only in (None, "solver"):
        solver_scenarios(twice, modules["cgrad"], lstsq, dev)
    if only in (None, "detector"):
        from tike_amd import _arrays
        _arrays.current_device()  # (once per process: tike_set_deterministic)
        # (what is not bit-stable is the atomics' of the general adjoint, at
        # det 32 and with the near field's FUSED off: the other 128^2
        # scenarios are held to their bits)
        detector_scenarios(
            lambda key, fn: record(
                key, fn, strict=False,
                twice="128" not in key or "FUSED=False" in key), lstsq, dev)
        differ = [k for k, r in results.items() if "again" in r]
        print(f"{len(differ)} scenarios whose second call launches otherwise",
              differ[:5])
    with open(out, "w") as fh:
        json.dump(results, fh, default=str)
    unstable = [k for k, r in results.items()
                if any(isinstance(h, list) for h in r["hashes"])]
    launches = sum(len(r["launches"]) for r in results.values())
    print(f"{len(results)} scenarios, {launches} launches, {len(unstable)} "
          f"with an unstable output -> {out}")


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:4]))
    if sys.argv[1] == "--child":
        sys.exit(child(*sys.argv[2:4]))
    # a fresh process: the library reads TIKE_DETERMINISTIC when it is loaded
    sys.exit(subprocess.run(
        [sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:3],
        env=dict(os.environ, TIKE_DETERMINISTIC="1"), timeout=900).returncode)
