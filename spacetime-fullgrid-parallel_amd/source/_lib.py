"""ctypes binding of libstk.so (include/stk.h) and the torch plumbing around it.

PyTorch is used for device memory, streams and torch.distributed only; every
arithmetic kernel of the hot path is a hand-written HIP kernel in libstk.
There is NO CPU fallback: if the library is missing, or a tensor does not live
on a GPU, the call raises.
"""
import ctypes
import os

import numpy as np
import torch

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(os.path.dirname(_HERE), 'libstk.so')
HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(_HERE)), 'include', 'stk.h')


class StkError(RuntimeError):
    pass


# callbacks of stk_pcg_solve (include/stk.h); how a callback receives its arguments is this side's choice
OPERATOR_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p)
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.c_int32)
CALLBACKS = {'stk_operator_fn': OPERATOR_FN, 'stk_allreduce_fn': ALLREDUCE_FN}

# the header's structs under the names the package uses
STRUCT_NAMES = {'stk_ell_pattern': 'EllPattern', 'stk_kron_ell_term': 'KronEllTerm', 'stk_pack_pattern': 'PackPattern',
                'stk_kron_pack_term': 'KronPackTerm', 'stk_comm_msg': 'CommMsg', 'stk_ell_rows': 'EllRows',
                'stk_csr_host': 'CsrHost', 'stk_mg_level': 'MGLevel'}

_SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'double': ctypes.c_double}


def bind(text):
    """The binding that header text states, as _header.parse reads it: (struct classes by C name,
    {function: (restype, argtypes)}, constants).  include/stk.h is the only statement of the ABI."""
    header = _header.parse(text)
    structs = {}

    def ctype(t):
        if t.stars == 0:
            return CALLBACKS.get(t.base, ctypes.c_void_p) if t.base in header.callbacks else _SCALARS[t.base]
        if t.stars == 1 and t.base == 'char' and t.const[0]:
            return ctypes.c_char_p
        if t.stars == 1 and t.base in structs:
            return ctypes.POINTER(structs[t.base])
        if t.stars == 2 and t.base in header.handles:  # the out-parameter of a *_create
            return ctypes.POINTER(ctypes.c_void_p)
        return ctypes.c_void_p

    for name, fields in header.structs:
        structs[name] = type(STRUCT_NAMES.get(name, name), (ctypes.Structure,),
                             {'_fields_': [(f, ctype(t)) for f, t in fields]})
    prototypes = {f.name: (ctype(f.ret), [ctype(p.type) for p in f.params]) for f in header.functions}
    return structs, prototypes, header.constants


def _bind_header():
    try:
        with open(HEADER_PATH) as f:
            return bind(f.read())
    except (OSError, _header.HeaderError) as e:
        raise StkError('cannot bind libstk from %s: %s' % (HEADER_PATH, e)) from e


_structs, prototypes, _constants = _bind_header()
globals().update({cls.__name__: cls for cls in _structs.values()})  # EllPattern, ..., MGLevel
globals().update(_constants)  # STK_TRANSFER_MAX_A, ...
EXPORTED_SYMBOLS = sorted(prototypes)

_lib = None


def lib():
    """The loaded library.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise StkError(
                'libstk.so not found at %s: build it with '
                '`python -c "import __graft_entry__ as g; g.build()"` or '
                '`make -C spacetime-fullgrid-parallel_amd/csrc`. '
                'There is no CPU fallback.' % LIB_PATH)
        _lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in prototypes.items():
            fn = getattr(_lib, name)
            fn.restype = res
            fn.argtypes = args
    return _lib


def check(rc):
    if rc != 0:
        raise StkError(lib().stk_last_error().decode())


def stream():
    if not torch.cuda.is_available():
        raise StkError('libstk kernels need a GPU (none visible); there is no '
                       'CPU fallback')
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """Device pointer of a tensor (None -> NULL).  Refuses host tensors and
    tensors of another GPU than this process's (a kernel of this rank's stream
    over another rank's memory is a peer access at best, a fault at worst)."""
    if t is None:
        return None
    if not t.is_cuda:
        raise StkError('libstk kernels need device tensors; got a %s tensor '
                       '(no GPU visible? there is no CPU fallback)' % t.device)
    if _process_device is not None and t.device.index != _process_device:
        raise StkError('tensor lives on cuda:%d but this process computes on '
                       'cuda:%d' % (t.device.index, _process_device))
    return t.data_ptr()


# The GPU of this process, fixed ONCE (comm.init_from_env, or the first use):
# torch.cuda.current_device() is thread-local and a new thread starts on device
# 0, so plans built in worker threads (heateq_mpi.py, multigrid.py) would
# otherwise be uploaded to cuda:0 on every rank.
_process_device = None


def set_process_device(index):
    """Pins the device of this process (one process per GPU)."""
    global _process_device
    _process_device = int(index)
    if torch.cuda.is_available():
        torch.cuda.set_device(_process_device)


def compute_device():
    """Device the slab of this process lives on -- the same answer in every
    thread."""
    global _process_device
    if _process_device is None:
        if not torch.cuda.is_available():
            return torch.device('cpu')
        _process_device = torch.cuda.current_device()
    return torch.device('cuda', _process_device)


def in_device_context(fn):
    """Wraps a worker-thread body so that the thread's current device (what
    hipMalloc and torch.cuda.current_stream() see) is the process's."""
    def run(*args, **kw):
        dev = compute_device()
        if dev.type != 'cuda':
            return fn(*args, **kw)
        with torch.cuda.device(dev):
            return fn(*args, **kw)
    return run


from .host_malloc import give_back, host_heap_for_setup, keep_to_the_heap  # noqa: E402,F401


def to_dev(array, dtype=None):
    """Uploads a NumPy array (used for CSR arrays and small tables)."""
    t = torch.from_numpy(np.ascontiguousarray(array))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(compute_device())


def transpose(src, rows, cols, ld_src, dst, ld_dst, zero_to=0, src_off=0, dst_off=0):
    """dst[c, r] = src[r, c] on the device (stk_transpose); offsets in doubles."""
    check(lib().stk_transpose(stream(), rows, cols, ptr(src) + 8 * src_off, ld_src,
                              ptr(dst) + 8 * dst_off, ld_dst, zero_to))


def copy_block(src, rows, cols, ld_src, dst, ld_dst, src_off=0, dst_off=0):
    """dst[r, c] = src[r, c] between two leading dimensions (stk_copy_block)."""
    if rows and cols:
        check(lib().stk_copy_block(stream(), rows, cols, ptr(src) + 8 * src_off, ld_src,
                                   ptr(dst) + 8 * dst_off, ld_dst))


class DeviceCSR:
    """A CSR matrix resident on the device: int32 pattern + float64 values
    (reference source/mpi_shared_mem.py:46-48 fixes the same dtypes)."""
    def __init__(self, mat):
        import scipy.sparse as sp
        mat = sp.csr_matrix(mat)
        mat.sort_indices()
        self.shape = mat.shape
        self.nnz = mat.nnz
        self.indptr = to_dev(mat.indptr.astype(np.int32))
        self.indices = to_dev(mat.indices.astype(np.int32))
        self.data = to_dev(mat.data.astype(np.float64))
