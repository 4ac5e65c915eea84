"""ctypes binding of the C ABI declared in include/tike_amd.h.

The shared library is built in-tree (``tike_amd/csrc/libtike_amd.so``) by
``tike_amd/csrc/Makefile`` (``__graft_entry__.build()``).  There is no CPU
fallback: if the library is missing, importing this module raises.

The argument types of every entry are read from the header, once, at import
(``parse_header``): the header is the only place a signature is written down.
"""
import ctypes
import os
import re

# PyTorch-ROCm bundles its own HIP runtime (torch/lib/libamdhip64.so).  It must
# be loaded BEFORE libtike_amd.so so that both bind to the same runtime: with
# the opposite order the process holds two runtimes and every launch from
# this library fails with hipErrorNoDevice (100).
import torch  # noqa: F401  (load order matters, see above)

_HERE = os.path.dirname(os.path.abspath(__file__))
# TIKE_AMD_LIB: alternative build of the same library (A/B tuning runs)
LIB_PATH = os.environ.get("TIKE_AMD_LIB") or os.path.join(
    _HERE, "csrc", "libtike_amd.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "tike_amd.h")

_SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long,
            "float": ctypes.c_float, "double": ctypes.c_double}
# [const] BASE [*...] [const] [name]; BASE is one word, or `unsigned` and one
_PARAMETER = re.compile(
    r"(?:const\s+)?((?:unsigned\s+)?\w+)\s*(\**)\s*(?:const\b\s*)?(?:\w+)?")


def _argtype(name, position, text):
    """The ctypes class of one parameter.  A spelling outside the rules is
    refused, never guessed: ctypes would truncate or reinterpret the value
    without a word."""
    m = _PARAMETER.fullmatch(text)
    base, stars = m.groups() if m else (None, None)
    if stars == "" and base in _SCALARS:
        return _SCALARS[base]
    if stars == "*":
        return ctypes.c_void_p
    if stars == "**" and base == "void":
        return ctypes.POINTER(ctypes.c_void_p)
    raise ImportError(
        f"include/tike_amd.h: {name}, parameter {position}: no ctypes type "
        f"for `{text}`")


def parse_header(text):
    """(constants, entries) of the text of a header: every `#define TIKE_*`
    with an integer value by name, and for every declaration
    `RET tike_name(PARAMS);`, in order, name -> (RET, [ctypes class, ...])."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants = {name: int(value) for name, value in re.findall(
        r"^[ \t]*#[ \t]*define[ \t]+(TIKE_\w+)[ \t]+(-?\d+)[ \t]*$", text,
        flags=re.M)}
    entries = {}
    for ret, name, params in re.findall(
            r"^[ \t]*(\w[\w \t*]*?)\s*\b(tike_\w+)\s*\((.*?)\)\s*;", text,
            flags=re.M | re.S):
        if name in entries:
            raise ImportError(f"include/tike_amd.h declares {name} twice")
        params = [" ".join(p.split()) for p in params.split(",")]
        if params in ([""], ["void"]):
            params = []
        entries[name] = (" ".join(ret.split()), [
            _argtype(name, k, p) for k, p in enumerate(params, 1)])
    if len(entries) != len(re.findall(r"\btike_\w+\s*\(", text)):
        raise ImportError(
            "include/tike_amd.h: a `tike_name(` that is no declaration "
            "`RET tike_name(PARAMS);` at the start of a line")
    return constants, entries


def read_header():
    """parse_header of include/tike_amd.h (one read of the file)."""
    if not os.path.isfile(HEADER_PATH):
        raise ImportError(
            f"{HEADER_PATH} not found: the binding reads every prototype from "
            "the header; `include/` travels with the package.")
    with open(HEADER_PATH) as f:
        return parse_header(f.read())


_CONSTANTS, _ENTRIES = read_header()

# the header version this package's call sites were written against
ABI_VERSION = 25
try:
    ERR_ARG = _CONSTANTS["TIKE_ERR_ARG"]
    ERR_UNSUPPORTED = _CONSTANTS["TIKE_ERR_UNSUPPORTED"]
    ERR_COMM = _CONSTANTS["TIKE_ERR_COMM"]
    COMM_ID_BYTES = _CONSTANTS["TIKE_COMM_ID_BYTES"]
except KeyError as e:
    raise ImportError(f"{HEADER_PATH} does not define {e.args[0]}") from e

if not os.path.isfile(LIB_PATH):
    raise ImportError(
        f"{LIB_PATH} not found: build the HIP library first "
        "(`make -C tike_amd/csrc` or `python -c 'import __graft_entry__ as g; "
        "g.build()'`). tike_amd has no CPU fallback.")

lib = ctypes.CDLL(LIB_PATH)

# name -> argtypes of every entry that returns int (tike_build_id does not),
# in the header's order
_PROTOTYPES = {name: args for name, (ret, args) in _ENTRIES.items()
               if ret == "int"}


def build_id():
    """sha256 of the sources the loaded library was built from
    (`tike_build_id`; '' for a library older than round 6)."""
    try:
        fn = lib.tike_build_id
    except AttributeError:
        return ""
    fn.restype = ctypes.c_char_p
    fn.argtypes = []
    return fn().decode()


def declared_symbols():
    """Names of every `int tike_*` entry declared in include/tike_amd.h."""
    return sorted(_PROTOTYPES)


for _name, _args in _PROTOTYPES.items():
    try:
        _fn = getattr(lib, _name)
    except AttributeError as e:
        raise ImportError(
            f"{LIB_PATH} does not export {_name}: it was built from another "
            "include/tike_amd.h; rebuild it (`make -C tike_amd/csrc`).") from e
    _fn.argtypes = _args
    _fn.restype = ctypes.c_int


def _check_abi_version():
    """Refuse a library built from another header: its entries would take
    this package's positional arguments for something else."""
    got = lib.tike_abi_version()
    header = _CONSTANTS.get("TIKE_ABI_VERSION")
    if got != ABI_VERSION or header != ABI_VERSION:
        raise ImportError(
            f"{LIB_PATH} reports ABI version {got}, include/tike_amd.h "
            f"{'?' if header is None else header}, this binding expects "
            f"{ABI_VERSION}: rebuild the library (`make -C tike_amd/csrc`).")


_check_abi_version()


def check(rc, what=""):
    """Translate a C-ABI return code into the reference's error behaviour."""
    if rc == 0:
        return
    if rc == ERR_ARG:
        raise ValueError(f"{what}: incompatible shapes / arguments")
    if rc == ERR_UNSUPPORTED:
        raise ValueError(f"{what}: unsupported size for the HIP path")
    if rc >= ERR_COMM:
        raise RuntimeError(f"{what}: RCCL error {rc - ERR_COMM}")
    raise RuntimeError(f"{what}: HIP error {rc}")


# TIKE_DETERMINISTIC=1: fixed-order sums instead of float atomics (bit-identical
# iterates from run to run; include/tike_amd.h `tike_set_deterministic`).  The
# scratch buffer the library needs is allocated here, on the device in use
# when the first tensor goes to the GPU (tike_amd._arrays.current_device).
DETERMINISTIC = os.environ.get("TIKE_DETERMINISTIC", "0") == "1"
DETERMINISTIC_SCRATCH_MIB = int(os.environ.get("TIKE_DETERMINISTIC_MIB", "256"))
_det_scratch = None


def ensure_deterministic():
    """Hand the library its scratch buffer (no-op unless TIKE_DETERMINISTIC=1).
    The buffer lives on ONE device -- the library's pointer is process-wide --
    and its users are ordered by ONE stream: when the current device is no
    longer the buffer's (torch.cuda.set_device, a second Reconstruction on
    another GPU) the buffer is re-allocated there and registered again, after
    the work in flight on the old one has finished.  Two devices driven
    concurrently from one process are not supported in this mode (one process
    per GPU is the design)."""
    global _det_scratch
    if not DETERMINISTIC:
        return
    current = torch.cuda.current_device()
    if _det_scratch is not None and _det_scratch.device.index == current:
        return
    if _det_scratch is not None:
        torch.cuda.synchronize(_det_scratch.device)
    _det_scratch = torch.empty(DETERMINISTIC_SCRATCH_MIB << 20,
                               dtype=torch.uint8,
                               device=torch.device("cuda", current))
    check(lib.tike_set_deterministic(1, _det_scratch.data_ptr(),
                                     _det_scratch.numel()),
          "tike_set_deterministic")
