"""Child process of test_three_chunks_in_deterministic_mode
(test_autograd_cost_gpu.py): the one-chunk and the three-chunk run of `cost`,
`cost_jvp` and `cost_gauss_newton_product` on the plain chunk case, compared
here; prints one JSON line {output: 0.0 where the bits agree, else the
normwise difference}.  The parent starts it under TIKE_DETERMINISTIC=1."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from test_autograd_cost_gpu import (CHUNK_CASES, _chunked_outputs,  # noqa: E402
                                    _compare_chunked)


def main():
    import tike_amd._lib as L
    assert L.DETERMINISTIC
    kind, shape = CHUNK_CASES[0]
    whole = _chunked_outputs(kind, shape, 0)
    cut = _chunked_outputs(kind, shape, 4)
    print(json.dumps(_compare_chunked(whole, cut)))


if __name__ == "__main__":
    main()
