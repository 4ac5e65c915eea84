"""The runners of tests/test_overlap_sums_gpu.py -- one case of
tests/overlap_sums.py through the entries by raw pointers, every output held
to the model's bound -- and, run as a program, the child process of
test_deterministic_forms: the reduced table under tike_set_deterministic
(process-wide, hence a fresh process), each case twice from the same start,
then the gather with a scratch buffer too small for the partial sums (the
one-chunk fall-back of probe_chunk).  Prints one JSON line and switches the
mode off again."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, HERE)
import numpy as np  # noqa: E402

import overlap_sums as om  # noqa: E402
from devbuf import Dev  # noqa: E402


def _api():
    import tike_amd._arrays as A
    from tike_amd._lib import lib
    return A, lib


def _held(x):
    """A read-only input on the device (it must come back bit for bit)."""
    return None if x is None else Dev(x.shape, cplx=np.iscomplexobj(x), init=x)


def _ptr(d):
    return None if d is None else d.ptr()


def _digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def run_gather(name, outputs=None):
    """tike_lstsq_gradients with the case's output set (or `outputs`),
    tike_probe_grad with the patches -- without them too where the case asks
    for m_probe_update alone -- and tike_probe_preconditioner.  Returns
    ({(entry, output): worst error / bound}, digest of every output, whether
    every input came back bit for bit)."""
    A, lib = _api()
    I = om.gather_inputs(name)
    c, H, W = I["case"], I["H"], I["W"]
    N, S, pw = c.nscan, c.S, c.pw
    R = om.gather_reference(name)
    keys = ("chi", "scan", "psi", "probe", "eigen", "weights", "unique")
    d = {k: _held(I[k]) for k in keys}
    st = A.stream_ptr()
    ratios, got_all = {}, []

    def outputs_of(which):
        return dict(
            patches=Dev((N, pw, pw), cplx=True) if "patches" in which else None,
            m_probe_update=Dev((S, pw, pw), cplx=True, init=I["mpu0"])
            if "m_probe_update" in which else None,
            objproj=Dev((N, pw, pw), cplx=True) if "objproj" in which else None)

    def judge(entry, o):
        for k, buf in o.items():
            if buf is None:
                continue
            prev = I["mpu0"] if k == "m_probe_update" else None
            got = buf.get()
            got_all.append(got)
            key = (entry, k)
            ratios[key] = max(ratios.get(key, 0.0), om.ratio(
                got, R[k], om.gather_bound(name, k, prev)[0], prev))

    which = om.OUTPUTS[outputs or c.outputs]
    o = outputs_of(which)
    rc = lib.tike_lstsq_gradients(
        d["chi"].ptr(), d["scan"].ptr(), d["psi"].ptr(), d["probe"].ptr(),
        _ptr(d["eigen"]), _ptr(d["weights"]), c.C, c.Sm, _ptr(d["unique"]),
        _ptr(o["patches"]), _ptr(o["m_probe_update"]), _ptr(o["objproj"]), N, S,
        pw, H, W, st)
    assert rc == 0, ("tike_lstsq_gradients", rc)
    judge("tike_lstsq_gradients", o)
    forms = [("patches", "m_probe_update")]
    if which == ("m_probe_update",):
        forms.append(("m_probe_update",))
    for form in forms:
        o = outputs_of(form)
        rc = lib.tike_probe_grad(d["chi"].ptr(), d["scan"].ptr(), d["psi"].ptr(),
                                 _ptr(o["patches"]), o["m_probe_update"].ptr(),
                                 N, S, pw, H, W, st)
        assert rc == 0, ("tike_probe_grad", rc)
        judge("tike_probe_grad", o)
    pre = Dev((pw, pw), cplx=True, init=I["pre0"])
    rc = lib.tike_probe_preconditioner(d["scan"].ptr(), d["psi"].ptr(), pre.ptr(),
                                       N, pw, H, W, st)
    assert rc == 0, ("tike_probe_preconditioner", rc)
    got = pre.get()
    got_all.append(got)
    # the imaginary part is not the entry's: bit for bit as it was
    assert np.array_equal(got.imag.copy().view(np.uint32),
                          I["pre0"].imag.copy().view(np.uint32))
    prev = I["pre0"].real.astype(np.float64)
    ratios[("tike_probe_preconditioner", "out")] = om.ratio(
        got.real.copy(), R["probe_preconditioner"],
        om.gather_bound(name, "probe_preconditioner", prev)[0], prev)
    intact = all(b.untouched() for b in d.values() if b is not None)
    return ratios, _digest(got_all), intact


def run_scatter(name):
    """The three scatter entries on a case, each into an image that already
    holds values.  Returns as run_gather, keyed (entry, "image")."""
    A, lib = _api()
    I = om.scatter_inputs(name)
    c = I["case"]
    scan = _held(I["scan"])
    st = A.stream_ptr()
    ratios, got_all, held = {}, [], [scan]
    for entry in om.SCATTER_ENTRIES:
        values, prev = om.scatter_values(I, entry)
        v = _held(values)
        held.append(v)
        if entry == "tike_scatter_patches":  # planar: real plane, imaginary plane
            img = Dev((2, c.H, c.W), init=np.stack([prev.real, prev.imag]))
        else:
            img = Dev((c.H, c.W), init=prev)
        rc = getattr(lib, entry)(v.ptr(), scan.ptr(), img.ptr(), c.nscan, c.pw,
                                 c.H, c.W, st)
        assert rc == 0, (entry, rc)
        got = img.get()
        got_all.append(got)
        if entry == "tike_scatter_patches":
            got = (got[0] + 1j * got[1]).astype(np.complex64)
        ratios[(entry, "image")] = om.ratio(
            got, om.scatter_reference(name, entry),
            om.scatter_bound(name, entry)[0], prev)
    return ratios, _digest(got_all), all(b.untouched() for b in held)


def _flat(ratios):
    return {"{} {}".format(*k): v for k, v in ratios.items()}


def main():
    _, lib = _api()
    out = dict(cases={}, identical=True, intact=True)
    floats = 1 << 22
    scratch = Dev(floats, init=np.zeros(floats, np.float32))
    assert lib.tike_set_deterministic(1, scratch.ptr(), 4 * floats) == 0
    try:
        for run, names in ((run_gather, om.DET_GATHER), (run_scatter, om.DET_SCATTER)):
            for name in names:
                kw = dict(outputs="all") if run is run_gather else {}
                first, second = run(name, **kw), run(name, **kw)
                out["cases"][name] = _flat(first[0])
                out["identical"] = out["identical"] and first[1] == second[1]
                out["intact"] = out["intact"] and first[2] and second[2]
        scratch.get()  # (the guard behind the scratch buffer)
        # partial sums of nine chunks do not fit: one chunk, one contributor
        name = om.DET_GATHER[-1]
        assert om.num_chunks(om.gather_inputs(name)["case"].nscan) > 1
        small = Dev(16, init=np.zeros(16, np.float32))
        assert lib.tike_set_deterministic(1, small.ptr(), 4 * 16) == 0
        first, second = run_gather(name, "all"), run_gather(name, "all")
        small.get()
        out["cases"]["small scratch " + name] = _flat(first[0])
        out["identical"] = out["identical"] and first[1] == second[1]
        out["intact"] = out["intact"] and first[2] and second[2]
    finally:
        lib.tike_set_deterministic(0, None, 0)
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
