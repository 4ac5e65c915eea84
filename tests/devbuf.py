"""Device buffers for tests that call a C entry by raw pointers: every buffer a
kernel may write carries GUARD floats of a known PATTERN behind its logical
end, which must come back intact; an output starts as NaN, an in-place or
accumulated array from the contents given."""
import numpy as np

GUARD = 64
PATTERN = (np.arange(GUARD, dtype=np.float32) * 0.5 - 1234.0)


def _arrays():
    import tike_amd._arrays as A
    return A


class Dev:
    """Device buffer of float32 or complex64 with GUARD floats of PATTERN behind
    its logical end; NaN unless `init` gives its contents."""

    def __init__(self, shape, cplx=False, init=None):
        self.shape, self.cplx = tuple(np.atleast_1d(shape)), cplx
        self.n = int(np.prod(self.shape)) * (2 if cplx else 1)
        host = np.full(self.n + GUARD, np.nan, np.float32)
        if init is not None:
            a = np.ascontiguousarray(
                np.broadcast_to(init, self.shape),
                dtype=np.complex64 if cplx else np.float32)
            host[:self.n] = a.view(np.float32).ravel()
        host[self.n:] = PATTERN
        self.start = host[:self.n].copy()
        self.flat = _arrays().to_device(host)

    def ptr(self):
        return self.flat.data_ptr()

    def get(self):
        host = self.flat.cpu().numpy()
        np.testing.assert_array_equal(host[self.n:], PATTERN,
                                      err_msg="written past the end")
        a = host[:self.n].copy()
        return (a.view(np.complex64) if self.cplx else a).reshape(self.shape)

    def untouched(self):
        """Guard intact and every bit of the contents as it started."""
        got = self.get().view(np.float32).ravel()
        return np.array_equal(got.view(np.uint32), self.start.view(np.uint32))


def dev(x):
    return None if x is None else _arrays().to_device(np.ascontiguousarray(x))


def dptr(t):
    return None if t is None else t.data_ptr()
