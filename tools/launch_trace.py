#!/usr/bin/env python3
"""Launch for launch, bit for bit: the host-code counterpart of
tools/kernel_identity.py for `tike_amd.autograd` (not a test):

    python tools/launch_trace.py OUT.json           # in each of two trees
    python tools/launch_trace.py --compare A.json B.json

The first form starts a fresh child process under TIKE_DETERMINISTIC=1 that
wraps every `tike_*` function of `_lib._PROTOTYPES` on the loaded library and
runs every public function of `tike_amd.autograd` on the smallest shapes of
the test helpers that take every branch -- one chunk and three chunks
(`CHUNK_POSITIONS_OVERRIDE = 5`), the fused multislice shape also with each
lever flipped.  Per scenario OUT.json holds the launches (the entry, null /
non-null for each pointer, the value of every other argument), the SHA-256 of
each output tensor and the peak of `torch.cuda.max_memory_allocated` above
what was resident.  `--compare` prints the first difference per scenario and
exits non-zero on any.  A tree without a built library borrows one through
TIKE_AMD_LIB."""
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


def compare(a, b):
    a, b = (json.load(open(p)) for p in (a, b))
    bad = 0
    for key in sorted(set(a) | set(b)):
        x, y = a.get(key), b.get(key)
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


def child(out):
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

    def record(key, fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before, trace[:] = torch.cuda.memory_allocated(), []
        outs = fn()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        outs = [outs] if isinstance(outs, torch.Tensor) else list(outs)
        results[key] = dict(launches=list(trace), peak=peak, hashes=[
            hashlib.sha256(t.detach().cpu().numpy().tobytes()).hexdigest()
            for t in outs])

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

    for shape in shapes():
        for chunks in (0, 5):
            lstsq.CHUNK_POSITIONS_OVERRIDE = chunks
            scenarios(f"{shape[0]} chunk {chunks}", *shape[1:])
        lstsq.CHUNK_POSITIONS_OVERRIDE = 0
        for module, lever in LEVERS if shape[0] == "fused" else ():
            value = getattr(modules[module], lever)
            setattr(modules[module], lever, not value)
            scenarios(f"fused {lever}={not value}", *shape[1:])
            setattr(modules[module], lever, value)
    with open(out, "w") as fh:
        json.dump(results, fh, default=str)
    print(f"{len(results)} scenarios -> {out}")


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(*sys.argv[2:4]))
    if sys.argv[1] == "--child":
        sys.exit(child(sys.argv[2]))
    # a fresh process: the library reads TIKE_DETERMINISTIC when it is loaded
    sys.exit(subprocess.run(
        [sys.executable, os.path.abspath(__file__), "--child", sys.argv[1]],
        env=dict(os.environ, TIKE_DETERMINISTIC="1"), timeout=900).returncode)
