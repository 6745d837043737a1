"""ctypes binding of libturbogp.so (the C-ABI in include/turbogp.h).

The optimisation path has no CPU fallback: if the library is missing or cannot be loaded this module
raises ``TurboGPLibraryError`` on first use, and every native class in this package is unusable.
The one thing that works without a GPU is the RELOAD path (a pickled model queried where no HIP device
is visible): ``NativeGP(DEVICE_HOST)`` -- a handle of the library's host backend -- and, where not even
the ROCm runtime is installed, the host-only build ``libturbogp_host.so`` (``load()`` says which).
"""
import ctypes
import importlib.util
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

# Hardware queues.  The HIP runtime deals a process's streams round-robin onto GPU_MAX_HW_QUEUES hardware queues
# (default 4) and two streams on one queue run one after the other: with the library's three shared streams per
# device plus the private streams of a threaded hyper-parameter fit (three per factory) a second live factory
# doubled the time of a fit (N = 500: 11.6 -> 19.3 ms; 11.8 with eight queues).  The runtime
# reads the variable ONCE, when it initialises (the first HIP call of the process: here tgp_create, or torch's own
# first CUDA call if that came earlier -- then this default is too late and the process keeps four queues unless
# the variable was exported before Python started).  An explicit setting in the environment always wins.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
# TGP_LIBRARY points at another build of the same library (kernel experiments)
LIB_PATH = os.environ.get("TGP_LIBRARY") or os.path.join(_HERE, "csrc", "libturbogp.so")

OK, NOT_PD, BAD_ARG, HIP_ERROR, NOT_FITTED, NO_MEMORY, NO_DEVICE = 0, 1, 2, 3, 4, 5, 6
DEVICE_HOST = -1     # tgp_create(TGP_DEVICE_HOST): the reload path without a GPU (include/turbogp.h)
F64, F32, F32X3, F32H2 = 0, 1, 2, 3
KERNELS = {"rbf": 0, "matern12": 1, "matern32": 2, "matern52": 3}
ACQ_NONE, ACQ_UCB, ACQ_PI, ACQ_EI, ACQ_SIGMA, ACQ_MES = 0, 1, 2, 3, 4, 5
BUF_K, BUF_L, BUF_LINV, BUF_ALPHA = 0, 1, 2, 3
BATCH_KB, BATCH_CL = 0, 1    # tgp_sweep_batch strategies: Kriging Believer, Constant Liar
SIDE_GE, SIDE_LE, SIDE_COST = 0, 1, 2    # tgp_side kinds: value >= level, value <= level, the log of a cost
SIDE_KINDS = {"ge": SIDE_GE, "le": SIDE_LE, "cost": SIDE_COST}
EHVI_MAX_FRONT = 256    # TGP_EHVI_MAX_FRONT: most points of a front (tgp_ehvi_set_front)

# every symbol include/turbogp.h declares
SYMBOLS = (
    "tgp_create", "tgp_destroy", "tgp_last_error", "tgp_version", "tgp_fit", "tgp_fit_grad", "tgp_loo", "tgp_fit_loo_grad", "tgp_fit_optimise", "tgp_fit_lbfgsb", "tgp_set_private_stream",
    "tgp_set_overlap", "tgp_tuning", "tgp_mt19937_uniform_columns", "tgp_set_candidates_mt19937", "tgp_stream_status", "tgp_workers_acquire", "tgp_workers_release",
    "tgp_fit_append", "tgp_export_state", "tgp_import_state", "tgp_export_factor_dev", "tgp_import_factor_dev", "tgp_debug_read",
    "tgp_set_candidates", "tgp_set_candidates_dev", "tgp_gen_candidates", "tgp_gen_candidates_lhs", "tgp_lhs_design",
    "tgp_read_candidates", "tgp_get_candidate",
    "tgp_sweep", "tgp_sweep_batch", "tgp_sweep_batch_mc", "tgp_ts_draw", "tgp_ts_sweep", "tgp_ts_eval", "tgp_ts_read", "tgp_mes_set_maxima", "tgp_mes_draw", "tgp_predict_cov", "tgp_sample_joint", "tgp_sweep_topk", "tgp_set_winner_out", "tgp_winner_wait", "tgp_acq_grad", "tgp_acq_refine", "tgp_acq_lbfgsb",
    "tgp_evaluate", "tgp_predict_batch", "tgp_predict", "tgp_profile_enable", "tgp_profile_read", "tgp_profile_reset",
    "tgp_sweep_geometry", "tgp_last_timings", "tgp_hyper_sample", "tgp_sweep_integrated", "tgp_kg_set_points", "tgp_sweep_kg",
    "tgp_kg_grad", "tgp_kg_lbfgsb", "tgp_sweep_weighted", "tgp_weighted_grad", "tgp_weighted_lbfgsb",
    "tgp_ehvi_set_front", "tgp_sweep_ehvi", "tgp_ehvi_grad", "tgp_ehvi_lbfgsb",
    "tgp_fit_input_grad", "tgp_warp_points", "tgp_warp_inverse", "tgp_warp_candidates", "tgp_warp_read_raw", "tgp_fit_warp_grad",
    "tgp_fit_warp_lbfgsb",
    "tgp_multi_create", "tgp_multi_destroy", "tgp_multi_last_error", "tgp_multi_size", "tgp_multi_handle",
    "tgp_multi_fit", "tgp_multi_set_candidates", "tgp_multi_gen_candidates", "tgp_multi_sweep",
)


class TurboGPLibraryError(RuntimeError):
    """libturbogp.so is missing / not loadable / reported a HIP failure."""


class NoDeviceError(TurboGPLibraryError):
    """tgp_create found no HIP device (TGP_NO_DEVICE)."""


_lib = None


class Factor(ctypes.Structure):
    """``tgp_factor`` (include/turbogp.h): what a sweep needs of a fit, as device pointers"""
    _fields_ = [("N", ctypes.c_int64), ("D", ctypes.c_int64), ("Np", ctypes.c_int64), ("Dp", ctypes.c_int64),
                ("fit_gen", ctypes.c_int64), ("kernel", ctypes.c_int32), ("normalize_y", ctypes.c_int32),
                ("small_path", ctypes.c_int32), ("reserved", ctypes.c_int32),
                ("constant", ctypes.c_double), ("noise", ctypes.c_double), ("jitter", ctypes.c_double),
                ("y_mean", ctypes.c_double), ("y_std", ctypes.c_double), ("lml", ctypes.c_double), ("sumlog", ctypes.c_double),
                ("Xs", ctypes.c_void_p), ("ls", ctypes.c_void_p), ("alpha", ctypes.c_void_p), ("Linv", ctypes.c_void_p)]


class Side(ctypes.Structure):
    """``tgp_side`` (include/turbogp.h): a side model of the weighted acquisition -- its handle, kind and level"""
    _fields_ = [("g", ctypes.c_void_p), ("kind", ctypes.c_int32), ("reserved", ctypes.c_int32), ("level", ctypes.c_double)]


_dp = ctypes.POINTER(ctypes.c_double)
_i64p = ctypes.POINTER(ctypes.c_int64)
_vp = ctypes.c_void_p


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.

    PyTorch's ROCm wheels bundle their own ``libamdhip64.so`` (SONAME ``libamdhip64.so.7``, the
    same as /opt/rocm's).  If ``torch`` is imported first, libturbogp.so's dependency resolves
    to that already-loaded copy and all is well; if libturbogp.so comes first it pulls in
    /opt/rocm's copy and a later ``import torch`` loads a SECOND runtime, which then finds "No
    HIP GPUs" -- and device pointers of one runtime are unknown to the other
    (``tgp_set_candidates_dev`` checks them).  So when PyTorch is installed, bind to its copy
    up front, without importing torch.  ``TGP_HIP_RUNTIME=system`` keeps /opt/rocm's."""
    if os.environ.get("TGP_HIP_RUNTIME", "") == "system" or "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    path = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(path):
        try:
            ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass   # libturbogp.so then binds to the system runtime as linked


HOST_LIB_PATH = os.path.join(_HERE, "csrc", "libturbogp_host.so")
HOST_ONLY = False     # True once load() had to settle for libturbogp_host.so (no ROCm runtime on this machine)
LOAD_ERROR = None     # why libturbogp.so itself could not be loaded, when HOST_ONLY (the dlopen message)


def _argtypes():
    c = ctypes
    fit = [_vp, _dp, c.c_int64, c.c_int64, _dp, c.c_int, c.c_double, _dp, c.c_int64, c.c_double, c.c_double,
           c.c_int, _dp, _dp, _dp]
    return {
        "tgp_last_error": [_vp],
        "tgp_create": [c.c_int, c.c_int, c.POINTER(_vp)],
        "tgp_destroy": [_vp],
        "tgp_fit": fit,
        "tgp_fit_grad": fit + [_dp],
        "tgp_loo": [_vp, _dp, _dp, _dp, _dp],
        "tgp_fit_loo_grad": fit + [_dp, _dp],
        "tgp_fit_input_grad": fit + [_dp, _dp],
        "tgp_warp_points": [_vp, _dp, c.c_int64, c.c_int64, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp],
        "tgp_warp_inverse": [_vp, _dp, c.c_int64, c.c_int64, _dp, _dp, _dp, _dp, _dp],
        "tgp_warp_candidates": [_vp, _dp, _dp, _dp, _dp],
        "tgp_warp_read_raw": [_vp, c.c_int64, c.c_int64, _dp],
        "tgp_fit_warp_grad": fit[:12] + [_dp, _dp, _dp, _dp] + fit[12:] + [_dp],
        "tgp_fit_warp_lbfgsb": [_vp, _dp, c.c_int64, c.c_int64, _dp, c.c_int, _dp, _dp, _dp, c.c_int64, c.c_int64, _dp, _dp,
                                c.c_double, c.c_double, c.c_int, c.c_int64, _dp, _dp, _i64p, _i64p],
        "tgp_fit_append": fit + [c.POINTER(c.c_int)],
        "tgp_fit_optimise": [_vp, _dp, c.c_int64, c.c_int64, _dp, c.c_int, _dp, c.c_int64, c.c_int64, _dp, _dp,
                             c.c_double, c.c_int, c.c_int64, _dp, _dp, _i64p, _i64p],
        "tgp_fit_lbfgsb": [_vp, _dp, c.c_int64, c.c_int64, _dp, c.c_int, _dp, c.c_int64, c.c_int64, _dp, _dp,
                           c.c_double, c.c_int, c.c_int64, _dp, _dp, _i64p, _i64p],
        "tgp_hyper_sample": [_vp, _dp, c.c_int64, c.c_int64, _dp, c.c_int, _dp, c.c_int64, _dp, _dp, c.c_double, c.c_int,
                             c.c_int64, c.c_int64, c.c_int64, _dp, c.c_uint64, _dp, _dp, _i64p, _i64p],
        "tgp_sweep_integrated": [_vp, _dp, c.c_int64, c.c_int64, _dp, c.c_int, _dp, c.c_int64, c.c_int64, c.c_double, c.c_int,
                                 c.c_int, c.c_double, c.c_double, c.c_double, _dp, _dp, _dp, _dp, _i64p, _i64p],
        "tgp_export_state": [_vp, _vp, c.c_int64, _i64p],
        "tgp_import_state": [_vp, _vp, c.c_int64, _dp],
        "tgp_export_factor_dev": [_vp, c.POINTER(Factor)],
        "tgp_import_factor_dev": [_vp, c.POINTER(Factor), c.c_int64, c.c_int64],
        "tgp_debug_read": [_vp, c.c_int, _dp],
        "tgp_set_candidates": [_vp, _dp, c.c_int64],
        "tgp_set_candidates_dev": [_vp, _vp, c.c_int64],
        "tgp_gen_candidates": [_vp, c.c_uint64, c.c_uint64, c.c_int64, _dp, _dp],
        "tgp_gen_candidates_lhs": [_vp, c.c_uint64, c.c_uint64, c.c_int64, c.c_uint64, _dp, _dp],
        "tgp_lhs_design": [_vp, c.c_uint64, c.c_uint64, c.c_int64, c.c_uint64, c.c_int64, _dp, _dp, _dp],
        "tgp_read_candidates": [_vp, c.c_int64, c.c_int64, _dp],
        "tgp_get_candidate": [_vp, c.c_int64, _dp],
        "tgp_sweep": [_vp, c.c_int, c.c_double, c.c_double, c.c_double, _dp, _dp, _dp, _dp, _i64p, _i64p],
        "tgp_sweep_topk": [_vp, c.c_int, c.c_double, c.c_double, c.c_double, c.c_int64, _dp, _i64p, _i64p],
        "tgp_sweep_batch": [_vp, c.c_int64, c.c_int, c.c_double, _dp, c.c_int64, c.c_int, c.c_double, c.c_double,
                            c.c_double, _i64p, _dp, _dp, _dp, _dp, _dp, _i64p],
        "tgp_sweep_batch_mc": [_vp, c.c_int64, c.c_int64, c.c_uint64, _dp, _dp, c.c_int64, c.c_int, c.c_double, c.c_double,
                               c.c_double, _i64p, _dp, _dp, _dp, _dp, _dp, _dp, _i64p],
        "tgp_ts_draw": [_vp, c.c_uint64, c.c_int64, c.c_int64],
        "tgp_ts_sweep": [_vp, c.c_double, c.c_int, _i64p, _dp, _dp, _dp],
        "tgp_ts_eval": [_vp, _dp, c.c_int64, _dp, _dp],
        "tgp_ts_read": [_vp, _dp, _dp, _dp, _dp],
        "tgp_mes_set_maxima": [_vp, _dp, c.c_int64],
        "tgp_mes_draw": [_vp, c.c_uint64, c.c_int64, c.c_int64, c.c_double, c.c_double, _dp],
        "tgp_kg_set_points": [_vp, _dp, c.c_int64, _dp],
        "tgp_sweep_kg": [_vp, c.c_double, _dp, _dp, _dp, _dp, _dp, _i64p, _i64p],
        "tgp_kg_grad": [_vp, _dp, c.c_int64, c.c_double, _dp, _dp],
        "tgp_kg_lbfgsb": [_vp, _dp, c.c_int64, _dp, _dp, c.c_double, c.c_int64, _dp, _dp, _i64p, _i64p],
        "tgp_sweep_weighted": [_vp, c.POINTER(Side), c.c_int64, c.c_int, c.c_double, c.c_double, c.c_double, _dp, _dp, _dp, _dp,
                               _dp, _dp, _dp, _dp, _i64p, _i64p],
        "tgp_weighted_grad": [_vp, c.POINTER(Side), c.c_int64, _dp, c.c_int64, c.c_int, c.c_double, c.c_double, c.c_double,
                              _dp, _dp],
        "tgp_weighted_lbfgsb": [_vp, c.POINTER(Side), c.c_int64, _dp, c.c_int64, _dp, _dp, c.c_int, c.c_double, c.c_double,
                                c.c_double, c.c_int64, _dp, _dp, _i64p, _i64p],
        "tgp_ehvi_set_front": [_vp, _dp, c.c_int64, c.c_double, c.c_double, _dp, _i64p, _dp, _dp],
        "tgp_sweep_ehvi": [_vp, _vp, _dp, _dp, _dp, _dp, _dp, _dp, _i64p, _i64p],
        "tgp_ehvi_grad": [_vp, _vp, _dp, c.c_int64, _dp, _dp],
        "tgp_ehvi_lbfgsb": [_vp, _vp, _dp, c.c_int64, _dp, _dp, c.c_int64, _dp, _dp, _i64p, _i64p],
        "tgp_predict_cov": [_vp, _dp, c.c_int64, c.c_int, _dp, _dp, _i64p],
        "tgp_sample_joint": [_vp, _dp, c.c_int64, c.c_int64, c.c_int, c.c_double, c.c_uint64, _dp, _dp, _dp, _dp],
        "tgp_acq_refine": [_vp, _dp, c.c_int64, _dp, _dp, c.c_int, c.c_double, c.c_double, c.c_double,
                           c.c_int64, _dp, _dp, _i64p, _i64p],
        "tgp_acq_lbfgsb": [_vp, _dp, c.c_int64, _dp, _dp, c.c_int, c.c_double, c.c_double, c.c_double,
                           c.c_int64, _dp, _dp, _i64p, _i64p],
        "tgp_set_winner_out": [_vp, _vp, c.c_int64],
        "tgp_winner_wait": [_vp, _vp],
        "tgp_stream_status": [_vp, c.POINTER(c.c_int)],
        "tgp_acq_grad": [_vp, _dp, c.c_int64, c.c_int, c.c_double, c.c_double, c.c_double, _dp, _dp],
        "tgp_evaluate": [_vp, _dp, c.c_int64, c.c_int, c.c_double, c.c_double, c.c_double, _dp, _dp, _dp,
                         _dp, _i64p, _i64p],
        "tgp_predict_batch": [_vp, c.c_int64, _i64p, c.c_int64, c.POINTER(_vp), c.POINTER(_vp), c.c_int, _dp, _dp,
                              _dp, _dp, c.c_int, _dp, c.c_int64, _dp, _dp, _dp, _i64p],
        "tgp_predict": [_vp, _dp, c.c_int64, _dp, _dp],
        "tgp_profile_enable": [_vp, c.c_int],
        "tgp_set_private_stream": [_vp, c.c_int],
        "tgp_set_overlap": [_vp, c.c_int],
        "tgp_workers_acquire": [_vp, c.c_int, c.POINTER(_vp)],
        "tgp_workers_release": [_vp],
        "tgp_tuning": [c.c_char_p, c.c_int64],
        "tgp_mt19937_uniform_columns": [_vp, c.POINTER(c.c_int32), c.c_int64, c.c_int64, _dp, _dp, _dp],
        "tgp_set_candidates_mt19937": [_vp, _vp, c.POINTER(c.c_int32), c.c_int64, c.c_int64, c.c_int64, _dp, _dp],
        "tgp_profile_read": [_vp, _i64p, _dp, _i64p, _dp, _dp, _dp],
        "tgp_profile_reset": [_vp],
        "tgp_sweep_geometry": [_vp, _i64p, _i64p],
        "tgp_last_timings": [_vp, _dp, c.c_int64],
        "tgp_multi_last_error": [_vp],
        "tgp_multi_create": [c.c_int, c.POINTER(c.c_int), c.c_int, c.POINTER(_vp)],
        "tgp_multi_destroy": [_vp],
        "tgp_multi_size": [_vp],
        "tgp_multi_handle": [_vp, c.c_int, c.POINTER(_vp)],
        "tgp_multi_fit": [_vp] + fit[1:],
        "tgp_multi_set_candidates": [_vp, _dp, c.c_int64],
        "tgp_multi_gen_candidates": [_vp, c.c_uint64, c.c_int64, _dp, _dp],
        "tgp_multi_sweep": [_vp, c.c_int, c.c_double, c.c_double, c.c_double, _dp, _i64p, _dp, _dp],
    }


class _Unavailable:
    """stands in for a GPU-only entry of the host-only library: calling it says what is missing"""

    def __init__(self, name):
        self.name = name

    def __call__(self, *a):
        raise TurboGPLibraryError("%s needs the GPU build of libturbogp.so; this process loaded the host-only "
                                  "library (%s), which serves reloaded models only" % (self.name, HOST_LIB_PATH))


def load():
    """Load the library once and declare argument types.  Raises loudly when absent.

    Where libturbogp.so cannot be LOADED -- a machine without the ROCm runtime it links, e.g. the laptop
    that plots a recorder -- the host-only build libturbogp_host.so (same C-ABI names, TGP_DEVICE_HOST
    handles only) is taken instead and ``HOST_ONLY`` is set: reloaded models predict, everything
    else raises."""
    global _lib, HOST_ONLY, LOAD_ERROR
    if _lib is not None:
        return _lib
    if os.environ.get("TGP_LIBRARY") and not os.path.exists(LIB_PATH):
        # an explicit path that does not exist is a mistake, never a reason to settle for the host-only build
        raise TurboGPLibraryError("TGP_LIBRARY=%s does not exist" % LIB_PATH)
    if not os.path.exists(LIB_PATH) and not os.path.exists(HOST_LIB_PATH):
        raise TurboGPLibraryError(
            "libturbogp.so not found at %s -- build it with `python -c 'import __graft_entry__ as g; "
            "g.build()'` or `make -C turbo_amd/csrc`. There is no CPU fallback." % LIB_PATH)
    lib = None
    err = None
    if os.path.exists(LIB_PATH):
        _share_hip_runtime_with_torch()
        try:
            lib = ctypes.CDLL(LIB_PATH)
        except OSError as e:
            err = e
    if lib is None:
        if not os.path.exists(HOST_LIB_PATH):
            raise TurboGPLibraryError("cannot load %s: %s" % (LIB_PATH, err)) from err
        try:
            lib = ctypes.CDLL(HOST_LIB_PATH)
        except OSError as e:
            raise TurboGPLibraryError("cannot load %s (%s) nor %s (%s)" % (LIB_PATH, err, HOST_LIB_PATH, e)) from e
    lib.tgp_version.restype = ctypes.c_char_p
    HOST_ONLY = b"host-only" in lib.tgp_version()
    if HOST_ONLY:
        LOAD_ERROR = ("%s: %s" % (LIB_PATH, err)) if err is not None else "%s is not there" % LIB_PATH
    for name, args in _argtypes().items():
        if not hasattr(lib, name):
            if not HOST_ONLY:
                raise TurboGPLibraryError("%s does not export %s" % (LIB_PATH, name))
            setattr(lib, name, _Unavailable(name))
            continue
        fn = getattr(lib, name)
        fn.argtypes = args
        fn.restype = (ctypes.c_char_p if name in ("tgp_last_error", "tgp_multi_last_error")
                      else ctypes.c_int64 if name == "tgp_tuning" else ctypes.c_int)
    _lib = lib
    return lib


class _Workers:
    def __init__(self, gp, n):
        self.gp, self.n = gp, n

    def __enter__(self):
        arr = (_vp * self.n)()
        self.gp._check(self.gp.lib.tgp_workers_acquire(self.gp._h, self.n, arr))
        # the pool's mutex is this thread's from here: whatever goes wrong before the block is entered (a failed
        # allocation, a KeyboardInterrupt) must give it back, or every later hyper-parameter fit on the device blocks
        try:
            self.views = [NativeGP._borrowed(self.gp.lib, _vp(arr[i]), self.gp.device) for i in range(self.n)]
        except BaseException:
            self.gp.lib.tgp_workers_release(self.gp._h)
            raise
        return self.views

    def __exit__(self, *exc):
        # the handles go back to the pool: the views handed out must not outlive the block (the library may destroy the
        # workers with the device's last ordinary handle, and another thread's fit may be using them by then)
        for w in getattr(self, "views", []):
            w._h = None
        self.views = []
        rc = self.gp.lib.tgp_workers_release(self.gp._h)
        if rc != OK and exc[0] is None:
            self.gp._check(rc)
        return False


class _GlobalRngLock:
    """NumPy's own lock around its global generator -- every draw of ``np.random`` takes it -- held while the library reads
    the state, continues the stream and writes the state back: another thread's draw then waits, exactly as it would
    behind one of NumPy's own long draws, instead of landing between the read and the write-back and being lost."""

    def __enter__(self):
        try:
            self.lock = np.random.mtrand._rand._bit_generator.lock
            self.lock.acquire()
        except Exception:
            self.lock = None
        return self

    def __exit__(self, *exc):
        if self.lock is not None:
            self.lock.release()
        return False


def numpy_global_uniform_columns(num_points, lows, highs):
    """``np.hstack([np.random.uniform(lo, hi, size=(num_points, 1)) for lo, hi in zip(lows, highs)])`` -- the reference's
    ``random_selector`` (turbo/modules/naive_selectors.py:39-46) -- computed by ``tgp_mt19937_uniform_columns``: NumPy's
    GLOBAL legacy RNG is read (``np.random.get_state``), its MT19937 stream continued in C++ and the state written back,
    so the numbers AND every later draw from ``np.random`` are the ones NumPy itself would have produced, bit for bit
    (tests/test_host_draw.py).  Returns None where that cannot be promised (another bit generator behind the global
    RNG, bounds whose range is not finite, a library without the entry): the caller then asks NumPy."""
    lo = np.asarray(lows, dtype=np.float64).reshape(-1)
    hi = np.asarray(highs, dtype=np.float64).reshape(-1)
    if num_points < 1 or lo.size < 1 or lo.shape != hi.shape:
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        if not np.all(np.isfinite(hi - lo)):
            return None   # (NumPy raises for a range that is not finite: let it)
    try:
        lib = load()
        entry = lib.tgp_mt19937_uniform_columns
    except Exception:
        return None
    if isinstance(entry, _Unavailable):
        return None
    out = np.empty((int(num_points), lo.size), dtype=np.float64)
    lo, hi = _f64c(lo), _f64c(hi)
    with _GlobalRngLock():
        st = np.random.get_state()
        if not isinstance(st, tuple) or st[0] != "MT19937" or len(st) != 5:
            return None
        key = np.array(st[1], dtype=np.uint32, order="C", copy=True)
        pos = ctypes.c_int32(int(st[2]))
        rc = entry(key.ctypes.data_as(_vp), ctypes.byref(pos), int(num_points), lo.size, _ptr(lo), _ptr(hi), _ptr(out))
        if rc != OK:
            return None       # (nothing was written back: NumPy's state is untouched)
        np.random.set_state((st[0], key, int(pos.value), st[3], st[4]))
    return out


def tuning():
    """every TGP_* switch of the library with the value in force in this process (``tgp_tuning``):
    {name: (value, description)}"""
    lib = load()
    n = lib.tgp_tuning(None, 0)
    buf = ctypes.create_string_buffer(int(n))
    lib.tgp_tuning(buf, n)
    out = {}
    for line in buf.value.decode().splitlines():
        kv, _, doc = line.partition("\t# ")
        k, _, v = kv.partition("=")
        out[k] = (v, doc)
    return out


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _f64c(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _bounds(lo, hi, D=None):
    """the box as two contiguous float64 vectors; with D, one entry per dimension or an AssertionError"""
    lo, hi = _f64c(lo).reshape(-1), _f64c(hi).reshape(-1)
    assert D is None or lo.shape == hi.shape == (D,), "bounds must have one entry per dimension"
    return lo, hi


def _pending(pending, D):
    """the pending points of a batch selection as (Xp (P, D) or None, P); nothing pending: (None, 0)"""
    Xp = None if pending is None else _f64c(np.atleast_2d(pending))
    if Xp is None or Xp.size == 0:
        return None, 0
    assert Xp.ndim == 2 and Xp.shape[1] == D, "pending points must be (P, %d)" % D
    return Xp, Xp.shape[0]


class _SweepOut:
    """what tgp_sweep / tgp_evaluate / tgp_sweep_integrated write: the (M,) vectors asked for and the winner"""

    def __init__(self, M, want_mu, want_sigma, want_acq):
        self.mu = np.empty(M) if want_mu else None
        self.sg = np.empty(M) if want_sigma else None
        self.aq = np.empty(M) if want_acq else None
        self.bv, self.bi, self.nc = ctypes.c_double(float("nan")), ctypes.c_int64(-1), ctypes.c_int64(0)

    def args(self):
        return (_ptr(self.mu), _ptr(self.sg), _ptr(self.aq), ctypes.byref(self.bv), ctypes.byref(self.bi),
                ctypes.byref(self.nc))

    def result(self, **extra):
        return dict(mu=self.mu, sigma=self.sg, acq=self.aq, best_val=self.bv.value, best_idx=self.bi.value,
                    n_clamped=self.nc.value, **extra)


class NativeGP:
    """One GPU context (tgp_handle).  Thin, stateful, not thread-safe per handle.
    ``device=DEVICE_HOST`` makes a host context instead (``self.host``): fit / predict / acquisition of
    a reloaded model without a GPU, nothing else."""
    ts_S = ts_F = 0    # shape of the last Thompson draw (ts_draw)
    fit_gen = 0        # counts the calls that left another fit in the handle (what a draw or MES maxima belong to)

    def __init__(self, device=0, dtype="f64"):
        self._h = None
        self.lib = load()
        assert dtype in ("f64", "f32", "f32x3", "f32h2"), "dtype must be 'f64', 'f32', 'f32x3' or 'f32h2'"
        self.dtype = dtype
        self.device = int(device)
        self.host = self.device == DEVICE_HOST
        h = _vp()
        rc = self.lib.tgp_create(self.device, {"f64": F64, "f32": F32, "f32x3": F32X3, "f32h2": F32H2}[dtype], ctypes.byref(h))
        if rc == NO_DEVICE:
            raise NoDeviceError(self.lib.tgp_last_error(None).decode())
        if rc != OK:
            raise TurboGPLibraryError(self.lib.tgp_last_error(None).decode())
        self._h = h
        self._cand_keepalive = None
        self._winner_keepalive = None
        self.gen_key = None      # what the resident batch IS when the GPU generated it: (kind, seed, first, M, total, lo, hi)
        if not self.host:
            self._warn_if_streams_serialised()

    _stream_warned = set()       # devices the warning below was given for (once per process and device)

    def stream_status(self):
        """``tgp_stream_status``: {'background_overlaps', 'third_overlaps'} (1 / 0 / -1 = not probed) and
        'gpu_max_hw_queues' as the environment has it (0: unset)"""
        v = (ctypes.c_int * 3)()
        self._check(self.lib.tgp_stream_status(self._h, v))
        return dict(background_overlaps=int(v[0]), third_overlaps=int(v[1]), gpu_max_hw_queues=int(v[2]))

    def _warn_if_streams_serialised(self):
        if self.device in NativeGP._stream_warned or not hasattr(self.lib, "tgp_stream_status"):
            return
        try:
            st = self.stream_status()
        except Exception:       # (a library without the entry: TGP_LIBRARY pointing at an older build)
            return
        if st["background_overlaps"] == 0 or st["third_overlaps"] == 0:
            NativeGP._stream_warned.add(self.device)
            import warnings
            what = []
            if st["background_overlaps"] == 0:
                what.append("the fit's background stream runs on the main stream's hardware queue: the inverse factor "
                            "follows the Cholesky instead of running beside it (large fits take about twice as long)")
            if st["third_overlaps"] == 0:
                what.append("there is no third stream: tgp_set_overlap / CandidateSweep(prefetch_next=True) is a no-op")
            warnings.warn("turbo_amd: the library's streams on device %d probed as SERIALISED (%s).  The HIP runtime deals "
                          "streams onto GPU_MAX_HW_QUEUES hardware queues (4 by default) and reads the variable once, at its "
                          "first call in the process: turbo_amd sets 8 at import, which is too late when another library "
                          "(torch.cuda) initialised HIP first -- GPU_MAX_HW_QUEUES is %s here.  Export GPU_MAX_HW_QUEUES=8 "
                          "before starting Python, or import turbo_amd and create its first context before touching "
                          "torch.cuda." % (self.device, "; ".join(what),
                                          st["gpu_max_hw_queues"] if st["gpu_max_hw_queues"] else "unset"), RuntimeWarning)

    def close(self):
        if getattr(self, "_h", None) is not None:
            if getattr(self, "_owned", True):
                self.lib.tgp_destroy(self._h)
            self._h = None

    @classmethod
    def _borrowed(cls, lib, handle, device):
        """a view of a handle the library owns (a pooled worker): every call works, close() does not destroy"""
        w = cls.__new__(cls)
        w._h, w.lib, w.dtype, w.device, w.host = handle, lib, "f64", int(device), False
        w._cand_keepalive = w._winner_keepalive = None
        w.gen_key = None
        w._owned = False
        return w

    def workers(self, n):
        """``tgp_workers_acquire``: a context manager yielding n worker handles of this handle's device (each on a
        private stream), the device's pool locked for this thread until the block ends"""
        return _Workers(self, int(n))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc == OK:
            return
        msg = self.lib.tgp_last_error(self._h).decode()
        if rc == NOT_PD:
            # same exception type (and advice) as sklearn/gaussian_process/_gpr.py:348-358
            raise np.linalg.LinAlgError(
                "The kernel is not returning a positive definite matrix. Try gradually "
                "increasing the 'alpha' parameter of the surrogate. (%s)" % msg)
        if rc == BAD_ARG:
            raise ValueError(msg)
        if rc == NOT_FITTED:
            raise RuntimeError(msg)
        if rc == NO_MEMORY:
            raise MemoryError(msg)
        raise TurboGPLibraryError(msg)

    def _fit_args(self, X, y, kind, constant, length_scale, noise, jitter, normalize_y):
        """what tgp_fit, tgp_fit_append, tgp_fit_grad and tgp_fit_loo_grad share: (X, number of length scales, their
        common argument list, the (lml, y_mean, y_std) doubles it points at)"""
        X = _f64c(X)
        y = _f64c(y).reshape(-1)
        assert X.ndim == 2 and X.shape[0] == y.shape[0], "X must be (N, D) and y (N,)"
        ls = _f64c(np.atleast_1d(length_scale))
        out = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        return X, ls.shape[0], (self._h, _ptr(X), X.shape[0], X.shape[1], _ptr(y), KERNELS[kind], float(constant),
                                _ptr(ls), ls.shape[0], float(noise), float(jitter), 1 if normalize_y else 0,
                                *map(ctypes.byref, out)), out

    def fit(self, X, y, kind, constant, length_scale, noise, jitter, normalize_y, append=False):
        """full fit, or (append=True) a one-row extension of the resident factor when X is the
        resident training set plus one row; ``self.appended`` tells which path ran"""
        X, _, args, (lml, ym, ys) = self._fit_args(X, y, kind, constant, length_scale, noise, jitter, normalize_y)
        self.appended = False
        if append:
            flag = ctypes.c_int(0)
            self._check(self.lib.tgp_fit_append(*args, ctypes.byref(flag)))
            self.appended = bool(flag.value)
        else:
            self._check(self.lib.tgp_fit(*args))
        self.fit_gen += 1
        self.N, self.D = X.shape
        return lml.value, ym.value, ys.value

    def fit_grad(self, X, y, kind, constant, length_scale, noise, jitter, normalize_y):
        """fit + d LML / d log(theta): returns (lml, grad [c, ls..., noise])"""
        X, n_ls, args, (lml, _, _) = self._fit_args(X, y, kind, constant, length_scale, noise, jitter, normalize_y)
        grad = np.zeros(2 + n_ls)
        self.fit_gen += 1
        self._check(self.lib.tgp_fit_grad(*args, _ptr(grad)))
        self.N, self.D = X.shape
        return lml.value, grad

    def loo(self):
        """``tgp_loo``: closed-form leave-one-out cross-validation of the fitted model.  Returns a dict with ``resid``
        (y_i - mu_-i, raw units), ``sigma`` (the held-out observation's deviation, raw units, noise and jitter
        included), ``lpd`` (log predictive densities, normalised units) and ``loo`` (their sum)"""
        n = int(self.N)
        resid, sigma, lpd = np.zeros(n), np.zeros(n), np.zeros(n)
        loo = ctypes.c_double()
        self._check(self.lib.tgp_loo(self._h, _ptr(resid), _ptr(sigma), _ptr(lpd), ctypes.byref(loo)))
        return dict(resid=resid, sigma=sigma, lpd=lpd, loo=loo.value)

    def fit_loo_grad(self, X, y, kind, constant, length_scale, noise, jitter, normalize_y):
        """fit + the leave-one-out score and d L_LOO / d log(theta): returns (lml, loo, grad [c, ls..., noise])"""
        X, n_ls, args, (lml, _, _) = self._fit_args(X, y, kind, constant, length_scale, noise, jitter, normalize_y)
        loo = ctypes.c_double()
        grad = np.zeros(2 + n_ls)
        self.fit_gen += 1
        self._check(self.lib.tgp_fit_loo_grad(*args, ctypes.byref(loo), _ptr(grad)))
        self.N, self.D = X.shape
        return lml.value, loo.value, grad

    def fit_input_grad(self, X, y, kind, constant, length_scale, noise, jitter, normalize_y, want_dX=True):
        """``tgp_fit_input_grad``: fit + d LML / d log(theta) on the blocked route + d LML / d X (N, D) in raw X units:
        returns (lml, grad [c, ls..., noise], dX); ``want_dX=False``: dX is None and the call is ``fit_grad`` on that route"""
        X, n_ls, args, (lml, _, _) = self._fit_args(X, y, kind, constant, length_scale, noise, jitter, normalize_y)
        grad = np.zeros(2 + n_ls)
        dX = np.zeros(X.shape) if want_dX else None
        self.fit_gen += 1
        self._check(self.lib.tgp_fit_input_grad(*args, _ptr(grad), _ptr(dX)))
        self.N, self.D = X.shape
        return lml.value, grad, dX

    @staticmethod
    def _warp_box(lo, hi, a, b, D):
        lo, hi = _bounds(lo, hi, D)
        a, b = _bounds(np.broadcast_to(np.asarray(a, dtype=np.float64), (D,)), np.broadcast_to(np.asarray(b, dtype=np.float64), (D,)), D)
        return lo, hi, a, b

    def warp_points(self, X, lo, hi, a, b, derivatives=False):
        """``tgp_warp_points``: the Kumaraswamy warp w (m, D) of the points X (m, D) in the box lo / hi with shapes a, b (D
        each, or scalars); ``derivatives=True``: (w, dw/du, dw/da, dw/db).  Needs no fitted model; a host handle
        computes it on the host"""
        X = _f64c(np.atleast_2d(X))
        lo, hi, a, b = self._warp_box(lo, hi, a, b, X.shape[1])
        out = [np.empty(X.shape) for _ in range(4 if derivatives else 1)]
        ptrs = [_ptr(o) for o in out] + [None] * (4 - len(out))
        self._check(self.lib.tgp_warp_points(self._h, _ptr(X), X.shape[0], X.shape[1], _ptr(lo), _ptr(hi), _ptr(a), _ptr(b), *ptrs))
        return tuple(out) if derivatives else out[0]

    def warp_inverse(self, W, lo, hi, a, b):
        """``tgp_warp_inverse``: the raw points x (m, D) whose warp is W (m, D), in closed form on the host"""
        W = _f64c(np.atleast_2d(W))
        lo, hi, a, b = self._warp_box(lo, hi, a, b, W.shape[1])
        out = np.empty(W.shape)
        self._check(self.lib.tgp_warp_inverse(self._h, _ptr(W), W.shape[0], W.shape[1], _ptr(lo), _ptr(hi), _ptr(a), _ptr(b), _ptr(out)))
        return out

    def warp_candidates(self, lo, hi, a, b):
        """``tgp_warp_candidates``: the RESIDENT batch through the warp on the device; the warped rows become the resident
        batch (a borrowed buffer is not written to), the raw rows stay readable through ``warp_read_raw`` until another
        batch is made resident.  Called again without a new batch it warps the raw rows with the new shapes"""
        lo, hi, a, b = self._warp_box(lo, hi, a, b, self.D)
        self._check(self.lib.tgp_warp_candidates(self._h, _ptr(lo), _ptr(hi), _ptr(a), _ptr(b)))

    def warp_read_raw(self, first=0, count=None):
        """``tgp_warp_read_raw``: rows [first, first + count) of the batch as it was before ``warp_candidates``"""
        count = int(self.M) - int(first) if count is None else int(count)
        out = np.empty((max(count, 0), self.D))
        self._check(self.lib.tgp_warp_read_raw(self._h, int(first), count, _ptr(out)))
        return out

    def fit_warp_grad(self, X, y, kind, constant, length_scale, noise, jitter, normalize_y, lo, hi, a, b):
        """``tgp_fit_warp_grad``: fit on w(X) + the gradient of the LML in log(constant, length scale(s), noise, a (D), b (D));
        returns (lml, grad (2 + n_ls + 2 D,)).  The handle is left fitted on w(X)"""
        X, n_ls, args, (lml, _, _) = self._fit_args(X, y, kind, constant, length_scale, noise, jitter, normalize_y)
        lo, hi, a, b = self._warp_box(lo, hi, a, b, X.shape[1])
        grad = np.zeros(2 + n_ls + 2 * X.shape[1])
        self.fit_gen += 1
        self._check(self.lib.tgp_fit_warp_grad(*args[:12], _ptr(lo), _ptr(hi), _ptr(a), _ptr(b), *args[12:], _ptr(grad)))
        self.N, self.D = X.shape
        return lml.value, grad

    def fit_warp_optimise(self, X, y, kind, lo, hi, theta0, n_ls, log_bounds, jitter, normalize_y, prior_sigma=0.0, max_iter=500):
        """``tgp_fit_warp_lbfgsb``: ``fit_optimise(lbfgsb=True)`` over theta' = log(constant, length scale(s), noise, a (D),
        b (D)) in the box lo / hi: every row of theta0 (S, P') is optimised inside log_bounds (P', 2), P' = 2 + n_ls + 2 D;
        ``prior_sigma > 0`` adds theta^2 / (2 prior_sigma^2) over the free warp entries.  Returns (theta (S, P'), the
        minimised objective (S,), status (S,), evaluations)"""
        X = _f64c(X)
        y = _f64c(y).reshape(-1)
        D = X.shape[1]
        lo, hi = _bounds(lo, hi, D)
        theta0 = _f64c(np.atleast_2d(theta0))
        S, P = theta0.shape
        assert P == 2 + n_ls + 2 * D, "theta0 must be (S, 2 + n_ls + 2 D)"
        lb = _f64c(np.asarray(log_bounds, dtype=np.float64).reshape(P, 2))
        blo, bhi = _f64c(lb[:, 0]), _f64c(lb[:, 1])
        theta, f = np.empty((S, P)), np.empty(S)
        st = np.empty(S, dtype=np.int64)
        ev = ctypes.c_int64(0)
        self.fit_gen += 1
        self._check(self.lib.tgp_fit_warp_lbfgsb(
            self._h, _ptr(X), X.shape[0], D, _ptr(y), KERNELS[kind], _ptr(lo), _ptr(hi), _ptr(theta0), S, int(n_ls), _ptr(blo),
            _ptr(bhi), float(prior_sigma), float(jitter), 1 if normalize_y else 0, int(max_iter), _ptr(theta), _ptr(f),
            st.ctypes.data_as(_i64p), ctypes.byref(ev)))
        return theta, f, st, ev.value

    def set_private_stream(self, on=True):
        """submit this handle's work to a stream of its own (handles of a device share one by default),
        so calls on several handles from several threads overlap on the GPU"""
        self._check(self.lib.tgp_set_private_stream(self._h, 1 if on else 0))

    def set_overlap(self, mode=2):
        """``tgp_set_overlap``: the next fits start the sweep of the RESIDENT candidate batch inside themselves
        (1: candidate scaling + the first cross-kernel, 2: + the contraction's early row tiles; 0: off).
        Results are bit-identical to the serial schedule."""
        self._check(self.lib.tgp_set_overlap(self._h, int(mode)))

    def fit_optimise(self, X, y, kind, theta0, n_ls, log_bounds, jitter, normalize_y, max_iter=500, lbfgsb=False):
        """the hyper-parameter fit inside the library: every row of theta0 (S, 2 + n_ls) = log(constant, length
        scale(s), noise) is optimised inside log_bounds (2 + n_ls, 2); returns (theta (S, P), -lml (S,), status (S,),
        evaluations).  ``lbfgsb=True`` = ``tgp_fit_lbfgsb``: SciPy's L-BFGS-B restated in the library, the iterates
        scikit-learn's fit walks, at every size; False = ``tgp_fit_optimise``: one launch with a projected L-BFGS for
        N <= 128, ``tgp_fit_lbfgsb`` above."""
        X = _f64c(X)
        y = _f64c(y).reshape(-1)
        theta0 = _f64c(np.atleast_2d(theta0))
        S, P = theta0.shape
        assert P == 2 + n_ls, "theta0 must be (S, 2 + n_ls)"
        lb = _f64c(np.asarray(log_bounds, dtype=np.float64).reshape(P, 2))
        lo, hi = _f64c(lb[:, 0]), _f64c(lb[:, 1])
        theta = np.empty((S, P))
        f = np.empty(S)
        st = np.empty(S, dtype=np.int64)
        ev = ctypes.c_int64(0)
        entry = self.lib.tgp_fit_lbfgsb if lbfgsb else self.lib.tgp_fit_optimise
        self.fit_gen += 1
        self._check(entry(
            self._h, _ptr(X), X.shape[0], X.shape[1], _ptr(y), KERNELS[kind], _ptr(theta0), S, int(n_ls),
            _ptr(lo), _ptr(hi), float(jitter), 1 if normalize_y else 0, int(max_iter), _ptr(theta), _ptr(f),
            st.ctypes.data_as(_i64p), ctypes.byref(ev)))
        return theta, f, st, ev.value

    def hyper_sample(self, X, y, kind, theta0, n_ls, log_bounds, jitter, normalize_y, n_samples=8, burn=20, thin=5,
                     width=None, seed=0):
        """``tgp_hyper_sample``: S slice-sampling draws of theta = log(constant, length scale(s), noise) from
        exp(LML) on the box log_bounds (2 + n_ls, 2), started at theta0.  Returns (thetas (S, P), lml (S,),
        evaluations, not_pd).  The handle is left fitted at the last evaluation -- not a model to use."""
        X = _f64c(X)
        y = _f64c(y).reshape(-1)
        assert X.ndim == 2 and X.shape[0] == y.shape[0], "X must be (N, D) and y (N,)"
        theta0 = _f64c(theta0).reshape(-1)
        P = 2 + int(n_ls)
        assert theta0.shape == (P,), "theta0 must be (2 + n_ls,)"
        lb = _f64c(np.asarray(log_bounds, dtype=np.float64).reshape(P, 2))
        lo, hi = _f64c(lb[:, 0]), _f64c(lb[:, 1])
        w = None if width is None else _f64c(np.broadcast_to(np.asarray(width, dtype=np.float64), (P,)))
        S = int(n_samples)
        theta = np.empty((max(S, 0), P))
        lml = np.empty(max(S, 0))
        ev, npd = ctypes.c_int64(0), ctypes.c_int64(0)
        self.fit_gen += 1
        self._check(self.lib.tgp_hyper_sample(
            self._h, _ptr(X), X.shape[0], X.shape[1], _ptr(y), KERNELS[kind], _ptr(theta0), int(n_ls), _ptr(lo), _ptr(hi),
            float(jitter), 1 if normalize_y else 0, S, int(burn), int(thin), _ptr(w), int(seed) & 0xFFFFFFFFFFFFFFFF,
            _ptr(theta), _ptr(lml), ctypes.byref(ev), ctypes.byref(npd)))
        self.N, self.D = X.shape
        return theta, lml, ev.value, npd.value

    def sweep_integrated(self, X, y, kind, thetas, n_ls, jitter, normalize_y, acq=ACQ_NONE, sf=1.0, incumbent=0.0,
                         param=0.0, want_mu=False, want_sigma=False, want_acq=False):
        """``tgp_sweep_integrated``: the acquisition averaged over the hyper-parameter samples thetas (S, 2 + n_ls) on
        the resident candidates, and the mixture's moments; a dict like ``sweep``'s.  The handle ends fitted at the
        last sample."""
        X = _f64c(X)
        y = _f64c(y).reshape(-1)
        thetas = _f64c(np.atleast_2d(thetas))
        assert thetas.shape[1] == 2 + int(n_ls), "thetas must be (S, 2 + n_ls)"
        out = _SweepOut(getattr(self, "M", 0), want_mu, want_sigma, want_acq)
        self.fit_gen += 1
        self._check(self.lib.tgp_sweep_integrated(
            self._h, _ptr(X), X.shape[0], X.shape[1], _ptr(y), KERNELS[kind], _ptr(thetas), thetas.shape[0], int(n_ls),
            float(jitter), 1 if normalize_y else 0, int(acq), float(sf), float(incumbent), float(param), *out.args()))
        self.N, self.D = X.shape
        return out.result()

    def export_state(self):
        """bytes that define the fitted model (theta, X, y) -- see tgp_export_state"""
        need = ctypes.c_int64(0)
        self._check(self.lib.tgp_export_state(self._h, None, 0, ctypes.byref(need)))
        buf = ctypes.create_string_buffer(need.value)
        self._check(self.lib.tgp_export_state(self._h, ctypes.cast(buf, _vp), need.value, ctypes.byref(need)))
        return buf.raw

    def import_state(self, blob):
        """rebuild the model of `export_state` on this handle (runs the fit); returns the LML"""
        blob = bytes(blob)
        lml = ctypes.c_double(0.0)
        buf = ctypes.create_string_buffer(blob, len(blob))
        self.fit_gen += 1
        self._check(self.lib.tgp_import_state(self._h, ctypes.cast(buf, _vp), len(blob), ctypes.byref(lml)))
        n, d = np.frombuffer(blob, dtype=np.int64, count=2, offset=8)
        self.N, self.D = int(n), int(d)
        return lml.value

    def export_factor(self):
        """``tgp_export_factor_dev``: a ``Factor`` of device pointers into THIS handle's buffers (valid until its next
        fit / import / close) -- what another handle, or another rank after a broadcast, needs to sweep with this fit"""
        f = Factor()
        self._check(self.lib.tgp_export_factor_dev(self._h, ctypes.byref(f)))
        return f

    def import_factor(self, factor, row0=0, rows=None):
        """``tgp_import_factor_dev``: receive rows [row0, row0 + rows) of a factor (all of it by default); rows arrive in
        order, the handle is fitted when the last one is in.  Returns True once the factor is complete."""
        rows = int(factor.Np - row0) if rows is None else int(rows)
        self.fit_gen += 1
        self._check(self.lib.tgp_import_factor_dev(self._h, ctypes.byref(factor), int(row0), rows))
        self.N, self.D = int(factor.N), int(factor.D)
        return row0 + rows == factor.Np

    def debug_read(self, which):
        N = self.N
        out = np.empty(N if which == BUF_ALPHA else (N, N), dtype=np.float64)
        self._check(self.lib.tgp_debug_read(self._h, which, _ptr(out)))
        return out

    def _batch_is(self, M, keepalive=None, gen_key=None):
        """the resident batch changed: its row count, what keeps a caller's device memory alive, and -- when the GPU
        generated it -- what it IS (``generate``'s key; None: not a generated batch, so nothing to find again)"""
        self.M = int(M)
        self._cand_keepalive = keepalive
        self.gen_key = gen_key

    def set_candidates(self, Xc):
        Xc = _f64c(Xc)
        assert Xc.ndim == 2 and Xc.shape[1] == self.D, "candidates must be (M, %d)" % self.D
        self._check(self.lib.tgp_set_candidates(self._h, _ptr(Xc), Xc.shape[0]))
        self._batch_is(Xc.shape[0])

    def set_candidates_numpy_stream(self, M, lo, hi, first=0, count=None):
        """make resident the batch ``np.hstack([np.random.uniform(l, h, size=(M, 1)) for l, h in zip(lo, hi)])`` -- the
        reference's ``random_selector`` draw (turbo/modules/naive_selectors.py:39-46) -- WITHOUT forming it on the host:
        NumPy's global MT19937 stream is continued in the library, the GPU forms the doubles
        (``tgp_set_candidates_mt19937``), and ``np.random`` is left where its own calls would have left it.  Returns
        False -- nothing drawn, nothing changed -- where that cannot be promised (a host handle, another bit generator
        behind the global RNG, a range that is not finite): the caller draws with NumPy then.

        ``first`` / ``count``: keep only rows [first, first + count) of that M-row batch resident -- a rank's shard of ONE
        batch -- while ``np.random`` still ends behind the whole batch (the other rows' numbers are passed over)."""
        lo, hi = _bounds(lo, hi)
        count = int(M) - int(first) if count is None else int(count)
        if getattr(self, "host", False) or HOST_ONLY or lo.shape != (self.D,) or hi.shape != (self.D,) or int(M) < 1:
            return False
        if first < 0 or count < 1 or first + count > int(M):
            return False
        with np.errstate(over="ignore", invalid="ignore"):
            if not np.all(np.isfinite(hi - lo)):
                return False
        with _GlobalRngLock():
            st = np.random.get_state()
            if not isinstance(st, tuple) or st[0] != "MT19937" or len(st) != 5:
                return False
            key = np.array(st[1], dtype=np.uint32, order="C", copy=True)
            pos = ctypes.c_int32(int(st[2]))
            self._check(self.lib.tgp_set_candidates_mt19937(self._h, key.ctypes.data_as(_vp), ctypes.byref(pos), int(M), int(first), count,
                                                            _ptr(lo), _ptr(hi)))
            np.random.set_state((st[0], key, int(pos.value), st[3], st[4]))
        self._batch_is(count)
        return True

    def set_candidates_dev(self, dev_ptr, M, keepalive=None):
        self._check(self.lib.tgp_set_candidates_dev(self._h, _vp(int(dev_ptr)), int(M)))
        self._batch_is(M, keepalive=keepalive)

    def generate(self, seed, first, M, lo, hi, lhs_total=None, reuse=False):
        """The resident batch drawn ON the GPU, uniform or (``lhs_total`` given) rows first .. + M of an lhs_total-point
        Latin hypercube: the one place that says what such a batch IS (``gen_key``) and how it is drawn.  ``reuse=True``
        leaves a batch alone that is this very one already (the previous call prefetched it).  Returns whether it drew."""
        lo, hi = _bounds(lo, hi, self.D)
        lhs = lhs_total is not None
        key = ("lhs" if lhs else "uniform", int(seed), int(first), int(M), int(lhs_total) if lhs else None,
               lo.tobytes(), hi.tobytes())
        if reuse and self.gen_key == key:
            return False
        if lhs:
            self._check(self.lib.tgp_gen_candidates_lhs(self._h, int(seed), int(first), int(M), int(lhs_total), _ptr(lo), _ptr(hi)))
        else:
            self._check(self.lib.tgp_gen_candidates(self._h, int(seed), int(first), int(M), _ptr(lo), _ptr(hi)))
        self._batch_is(M, gen_key=key)
        return True

    def gen_candidates(self, seed, first_candidate, M, lo, hi):
        """M uniform candidates in [lo, hi) drawn on the GPU (Philox-4x32-10 stream `seed`)"""
        self.generate(seed, first_candidate, M, lo, hi)

    def gen_candidates_lhs(self, seed, first_sample, M, n_total, lo, hi):
        """rows first_sample .. + M of an n_total-point Latin hypercube design drawn on the GPU become the resident batch"""
        self.generate(seed, first_sample, M, lo, hi, lhs_total=n_total)

    def lhs_design(self, seed, first_sample, M, n_total, lo, hi):
        """(M, D) rows of an n_total-point Latin hypercube design, drawn on the GPU, as a host array
        (no fitted model needed)"""
        lo, hi = _bounds(lo, hi)
        assert lo.shape == hi.shape and lo.ndim == 1
        out = np.empty((int(M), lo.shape[0]))
        self.gen_key = None      # the design overwrites the handle's own batch: a generated batch is no longer resident
        self._check(self.lib.tgp_lhs_design(self._h, int(seed), int(first_sample), int(M), int(n_total),
                                            lo.shape[0], _ptr(lo), _ptr(hi), _ptr(out)))
        return out

    def read_candidates(self, first=0, count=None):
        count = self.M - first if count is None else count
        out = np.empty((int(count), self.D))
        self._check(self.lib.tgp_read_candidates(self._h, int(first), int(count), _ptr(out)))
        return out

    def get_candidate(self, idx):
        out = np.empty(self.D, dtype=np.float64)
        self._check(self.lib.tgp_get_candidate(self._h, int(idx), _ptr(out)))
        return out

    def sweep(self, acq=ACQ_NONE, sf=1.0, incumbent=0.0, param=0.0, want_mu=False,
              want_sigma=False, want_acq=False):
        out = _SweepOut(self.M, want_mu, want_sigma, want_acq)
        self._check(self.lib.tgp_sweep(self._h, acq, float(sf), float(incumbent), float(param), *out.args()))
        return out.result(sweep_ms=self.profile_read()['last_sweep_ms'])

    def sweep_batch(self, q, strategy=BATCH_KB, lie=0.0, pending=None, acq=ACQ_EI, sf=1.0, incumbent=0.0, param=0.0,
                    want_posterior=False):
        """``tgp_sweep_batch``: q resident candidates chosen greedily under Kriging Believer / Constant Liar, conditioned
        on the pending points (P, D) first.  Returns a dict: idx (q,), val (q,), x (q, D), fantasies (P + q,) pending
        first, mu / sigma (M,) after all P + q points (want_posterior) or None, n_clamped"""
        q = int(q)
        Xp, P = _pending(pending, self.D)
        idx = np.empty(max(q, 1), dtype=np.int64)
        val = np.empty(max(q, 1))
        x = np.empty((max(q, 1), self.D))
        fant = np.empty(max(P + q, 1))
        mu = np.empty(self.M) if want_posterior else None
        sg = np.empty(self.M) if want_posterior else None
        nc = ctypes.c_int64(0)
        self._check(self.lib.tgp_sweep_batch(self._h, q, int(strategy), float(lie), _ptr(Xp), P, int(acq), float(sf),
                                             float(incumbent), float(param), idx.ctypes.data_as(_i64p), _ptr(val),
                                             _ptr(x), _ptr(fant), _ptr(mu), _ptr(sg), ctypes.byref(nc)))
        return dict(idx=idx[:q], val=val[:q], x=x[:q], fantasies=fant[:P + q], mu=mu, sigma=sg, n_clamped=nc.value,
                    sweep_ms=self.profile_read()['last_sweep_ms'])

    def sweep_batch_mc(self, q, n_sim=16, seed=0, eps=None, pending=None, acq=ACQ_EI, sf=1.0, incumbent=0.0, param=0.0,
                       want_acq=False, want_sigma=False):
        """``tgp_sweep_batch_mc``: q resident candidates chosen greedily by the Monte Carlo strategy -- the average of the
        acquisition over ``n_sim`` <= 64 simulated outcomes of the pending (P, D) and the selected points.  ``eps`` None:
        the normals come from the Philox stream of ``seed``; else (n_sim, P + q) standard normals used as they are.
        Returns a dict: idx (q,), val (q,), x (q, D), fantasies (n_sim, P + q) pending first, eps (n_sim, P + q), acq
        (q, M) every step's averaged acquisition (want_acq) or None, sigma (M,) after all points (want_sigma) or None,
        n_clamped"""
        q, S = int(q), int(n_sim)
        Xp, P = _pending(pending, self.D)
        J, Sa = max(P + q, 1), max(S, 1)
        if eps is not None:
            eps = _f64c(np.asarray(eps, dtype=np.float64))
            assert eps.shape == (S, P + q), "eps must be (n_sim, P + q) = (%d, %d)" % (S, P + q)
        idx = np.empty(max(q, 1), dtype=np.int64)
        val = np.empty(max(q, 1))
        x = np.empty((max(q, 1), self.D))
        fant = np.empty((Sa, J))
        eo = np.empty((Sa, J))
        aq = np.empty((max(q, 1), self.M)) if want_acq else None
        sg = np.empty(self.M) if want_sigma else None
        nc = ctypes.c_int64(0)
        self._check(self.lib.tgp_sweep_batch_mc(self._h, q, S, int(seed) % (1 << 64), _ptr(eps), _ptr(Xp), P, int(acq),
                                                float(sf), float(incumbent), float(param), idx.ctypes.data_as(_i64p),
                                                _ptr(val), _ptr(x), _ptr(fant), _ptr(eo), _ptr(aq), _ptr(sg),
                                                ctypes.byref(nc)))
        return dict(idx=idx[:q], val=val[:q], x=x[:q], fantasies=fant, eps=eo, acq=aq, sigma=sg, n_clamped=nc.value,
                    sweep_ms=self.profile_read()['last_sweep_ms'])

    def ts_draw(self, seed, S=1, F=2048):
        """``tgp_ts_draw``: S <= 64 posterior sample paths of the fitted model with F random Fourier features (a multiple
        of 64 in [64, 16384]), kept in the handle until the next draw or fit"""
        self._check(self.lib.tgp_ts_draw(self._h, int(seed) % (1 << 64), int(S), int(F)))
        self.ts_S, self.ts_F = int(S), int(F)

    def ts_sweep(self, sf=1.0, distinct=False, want_f=False):
        """``tgp_ts_sweep``: per drawn sample the arg-max of sf * raw value over the resident candidates (distinct: sample
        s skips the rows of samples < s).  Returns a dict: idx (S,), val (S,) raw sampled values, x (S, D), f (M, S) raw
        values (want_f) or None"""
        S = self.ts_S
        idx = np.empty(S, dtype=np.int64)
        val = np.empty(S)
        x = np.empty((S, self.D))
        f = np.empty((self.M, S)) if want_f else None
        self._check(self.lib.tgp_ts_sweep(self._h, float(sf), 1 if distinct else 0, idx.ctypes.data_as(_i64p), _ptr(val),
                                          _ptr(x), _ptr(f)))
        return dict(idx=idx, val=val, x=x, f=f, sweep_ms=self.profile_read()['last_sweep_ms'])

    def ts_eval(self, Xq, want_grad=False):
        """``tgp_ts_eval``: the drawn paths at m <= 4096 points; returns f (m, S) raw values and grad (m, S, D) or None"""
        Xq = _f64c(np.atleast_2d(Xq))
        assert Xq.ndim == 2 and Xq.shape[1] == self.D, "points must be (m, %d)" % self.D
        m, S = Xq.shape[0], self.ts_S
        f = np.empty((m, S))
        g = np.empty((m, S, self.D)) if want_grad else None
        self._check(self.lib.tgp_ts_eval(self._h, _ptr(Xq), m, _ptr(f), _ptr(g)))
        return f, g

    def ts_read(self):
        """``tgp_ts_read``: the draw itself -- omega (F, D) in scaled coordinates, b (F,), W (S, F), eps (S, N)"""
        S, F = self.ts_S, self.ts_F
        om, b, W, eps = np.empty((F, self.D)), np.empty(F), np.empty((S, F)), np.empty((S, self.N))
        self._check(self.lib.tgp_ts_read(self._h, _ptr(om), _ptr(b), _ptr(W), _ptr(eps)))
        return dict(omega=om, b=b, W=W, eps=eps)

    def mes_set_maxima(self, ystar):
        """``tgp_mes_set_maxima``: the 1 <= S <= 64 finite raw values of the optimum that ``ACQ_MES`` averages over; they
        belong to the resident fit (any later fit, append or import drops them).  Works on host handles too."""
        ys = _f64c(np.asarray(ystar, dtype=np.float64).reshape(-1))
        self._check(self.lib.tgp_mes_set_maxima(self._h, _ptr(ys), ys.shape[0]))

    def mes_draw(self, seed, S=8, F=2048, sf=1.0, incumbent=float("nan")):
        """``tgp_mes_draw``: S maxima of posterior sample paths over the resident candidates (a Thompson draw of F
        features and its non-distinct sweep), none worse than ``incumbent`` (NaN: no such step), stored as the handle's
        maxima on the device; returns them (S,).  The Thompson draw stays in the handle."""
        out = np.empty(max(int(S), 1))
        self._check(self.lib.tgp_mes_draw(self._h, int(seed) % (1 << 64), int(S), int(F), float(sf), float(incumbent),
                                          _ptr(out)))
        self.ts_S, self.ts_F = int(S), int(F)
        return out[:int(S)]

    def kg_set_points(self, Xa):
        """``tgp_kg_set_points``: the 1 <= A <= 256 finite discretisation points Xa (A, D) of the knowledge gradient; they
        belong to the resident fit (any later fit, append or import drops them).  Returns the raw posterior mean at
        them (A,).  GPU handles only."""
        Xa = _f64c(np.atleast_2d(Xa))
        assert Xa.ndim == 2 and Xa.shape[1] == self.D, "points must be (A, %d)" % self.D
        mu = np.empty(max(Xa.shape[0], 1))
        self._check(self.lib.tgp_kg_set_points(self._h, _ptr(Xa), Xa.shape[0], _ptr(mu)))
        self.kg_A = Xa.shape[0]
        return mu[:Xa.shape[0]]

    def sweep_kg(self, sf=1.0, want_kg=False, want_mu=False, want_sigma=False, want_cov=False):
        """``tgp_sweep_kg``: the knowledge gradient of every resident candidate against the stored points, float64
        behind the predict-only sweep.  Returns ``sweep``'s dict (``acq`` is the knowledge gradient (M,)) plus ``kg``
        (the same array), ``cov`` (M, A) -- the raw latent covariance between candidate i and point j -- or None, and
        ``kg_ms`` (``tgp_last_timings`` slot 20)."""
        M = getattr(self, "M", 0)
        out = _SweepOut(M, want_mu, want_sigma, want_kg)
        cov = np.empty((M, getattr(self, "kg_A", 0))) if want_cov else None
        self._check(self.lib.tgp_sweep_kg(self._h, float(sf), _ptr(out.aq), _ptr(out.mu), _ptr(out.sg), _ptr(cov),
                                          ctypes.byref(out.bv), ctypes.byref(out.bi), ctypes.byref(out.nc)))
        v = np.zeros(21)
        self._check(self.lib.tgp_last_timings(self._h, _ptr(v), 21))
        return out.result(kg=out.aq, cov=cov, kg_ms=float(v[20]))

    def kg_grad(self, Xq, sf=1.0):
        """``tgp_kg_grad``: the knowledge gradient (m,) -- ``sweep_kg``'s value for the same point -- and its gradient
        (m, D) at m <= 4096 points, against the stored points; float64 whatever the handle's dtype"""
        Xq = _f64c(np.atleast_2d(Xq))
        assert Xq.ndim == 2 and Xq.shape[1] == self.D, "points must be (m, %d)" % self.D
        val = np.empty(Xq.shape[0])
        grad = np.empty(Xq.shape)
        self._check(self.lib.tgp_kg_grad(self._h, _ptr(Xq), Xq.shape[0], float(sf), _ptr(val), _ptr(grad)))
        return val, grad

    def kg_lbfgsb(self, X0, lo, hi, sf=1.0, max_iter=15000):
        """``tgp_kg_lbfgsb``: ``acq_refine(lbfgsb=True)`` with the knowledge gradient as the objective -- L-BFGS-B from
        every start in lock-step, one batched ``tgp_kg_grad`` per round; returns (x (R, D), values (R,), status (R,),
        evaluations)"""
        X0 = _f64c(np.atleast_2d(X0))
        assert X0.ndim == 2 and X0.shape[1] == self.D, "start points must be (R, %d)" % self.D
        lo, hi = _bounds(lo, hi, self.D)
        R = X0.shape[0]
        x = np.empty((R, self.D))
        v = np.empty(R)
        st = np.empty(R, dtype=np.int64)
        its = ctypes.c_int64(0)
        self._check(self.lib.tgp_kg_lbfgsb(self._h, _ptr(X0), R, _ptr(lo), _ptr(hi), float(sf), int(max_iter), _ptr(x), _ptr(v),
                                           st.ctypes.data_as(_i64p), ctypes.byref(its)))
        return x, v, st, its.value

    @staticmethod
    def _sides(sides):
        """``[(NativeGP, kind, level), ...]`` as a ``tgp_side`` array (None when empty) and its length; kind: SIDE_GE /
        SIDE_LE / SIDE_COST or 'ge' / 'le' / 'cost'"""
        sides = list(sides or ())
        if not sides:
            return None, 0
        arr = (Side * len(sides))()
        for k, (g, kind, level) in enumerate(sides):
            arr[k].g = g._h if isinstance(g._h, int) or g._h is None else g._h.value
            arr[k].kind = SIDE_KINDS[kind] if isinstance(kind, str) else int(kind)
            arr[k].level = float(level)
        return arr, len(sides)

    @staticmethod
    def _resident_rows_are(g, M):
        """does handle g hold exactly M resident rows?  (tgp_read_candidates answers TGP_BAD_ARG past the batch)"""
        row = np.empty(max(int(getattr(g, 'D', 0)), 1))
        return M >= 1 and g.lib.tgp_read_candidates(g._h, M - 1, 1, _ptr(row)) == OK and \
            g.lib.tgp_read_candidates(g._h, M, 1, _ptr(row)) != OK

    def sweep_weighted(self, sides, acq=ACQ_EI, sf=1.0, incumbent=0.0, param=0.0, want_mu=False, want_sigma=False,
                       want_acq=False, want_logw=False, want_value=False, want_sides=False):
        """``tgp_sweep_weighted``: the resident batch scored under this (the objective's) model and the side models
        ``sides = [(NativeGP, kind, level), ...]`` -- value = acq * prod_k f_k (EI / PI) or sum_k log f_k (ACQ_NONE) --
        and its arg-max.  Every side's resident batch becomes its own copy of this handle's rows.  ``acq`` (M,) is the
        unweighted acquisition; ``want_sides``: ``side_mu`` / ``side_sigma`` (K, M)."""
        arr, K = self._sides(sides)
        out = _SweepOut(self.M, want_mu, want_sigma, want_acq)
        logw = np.empty(self.M) if want_logw else None
        value = np.empty(self.M) if want_value else None
        smu = np.empty((K, self.M)) if want_sides else None
        ssg = np.empty((K, self.M)) if want_sides else None
        try:
            self._check(self.lib.tgp_sweep_weighted(self._h, arr, K, int(acq), float(sf), float(incumbent), float(param), _ptr(out.mu),
                                                    _ptr(out.sg), _ptr(out.aq), _ptr(logw), _ptr(value), _ptr(smu), _ptr(ssg),
                                                    ctypes.byref(out.bv), ctypes.byref(out.bi), ctypes.byref(out.nc)))
        except Exception:
            # a side the call reached before it failed owns a copy of these rows already: its row count is asked of the
            # library (a probe of row M - 1 and of row M), so that a later sweep's (M,) outputs have the library's size
            for g, _, _ in (sides or ()):
                if isinstance(g, NativeGP) and g is not self and g._h is not None and not g.host and self._resident_rows_are(g, self.M):
                    g._batch_is(self.M)
            raise
        for g, _, _ in (sides or ()):
            g._batch_is(self.M)       # the side owns a copy of these rows now: nothing of a caller's to keep alive
        return out.result(logw=logw, value=value, side_mu=smu, side_sigma=ssg)

    def weighted_grad(self, Xq, sides, acq=ACQ_EI, sf=1.0, incumbent=0.0, param=0.0):
        """``tgp_weighted_grad``: the weighted value (m,) -- ``sweep_weighted``'s formula -- and its gradient (m, D) at
        m <= 4096 points; float64 whatever the handles' dtypes"""
        Xq = _f64c(np.atleast_2d(Xq))
        assert Xq.ndim == 2 and Xq.shape[1] == self.D, "points must be (m, %d)" % self.D
        arr, K = self._sides(sides)
        val = np.empty(Xq.shape[0])
        grad = np.empty(Xq.shape)
        self._check(self.lib.tgp_weighted_grad(self._h, arr, K, _ptr(Xq), Xq.shape[0], int(acq), float(sf), float(incumbent),
                                               float(param), _ptr(val), _ptr(grad)))
        return val, grad

    def weighted_lbfgsb(self, X0, lo, hi, sides, acq=ACQ_EI, sf=1.0, incumbent=0.0, param=0.0, max_iter=15000):
        """``tgp_weighted_lbfgsb``: ``acq_refine(lbfgsb=True)`` with the weighted value as the objective -- L-BFGS-B from
        every start in lock-step, one batched ``tgp_weighted_grad`` per round; returns (x (R, D), values (R,), status
        (R,), evaluations)"""
        X0 = _f64c(np.atleast_2d(X0))
        assert X0.ndim == 2 and X0.shape[1] == self.D, "start points must be (R, %d)" % self.D
        lo, hi = _bounds(lo, hi, self.D)
        arr, K = self._sides(sides)
        R = X0.shape[0]
        x = np.empty((R, self.D))
        v = np.empty(R)
        st = np.empty(R, dtype=np.int64)
        its = ctypes.c_int64(0)
        self._check(self.lib.tgp_weighted_lbfgsb(self._h, arr, K, _ptr(X0), R, _ptr(lo), _ptr(hi), int(acq), float(sf),
                                                 float(incumbent), float(param), int(max_iter), _ptr(x), _ptr(v),
                                                 st.ctypes.data_as(_i64p), ctypes.byref(its)))
        return x, v, st, its.value

    def ehvi_set_front(self, Y, ref, sf=(1.0, 1.0)):
        """``tgp_ehvi_set_front``: the Pareto front of the observed pairs ``Y`` (n, 2) over the reference point ``ref``
        (2,), raw units, under the directions ``sf`` (+1 maximise, -1 minimise), kept on this (objective 1's) handle
        until the next call.  Returns (front (P, 2) raw units, sorted by the oriented first objective ascending;
        hypervolume).  Needs no fitted model."""
        Y = _f64c(Y).reshape(-1, 2)
        ref = _f64c(ref).reshape(-1)
        assert ref.shape == (2,), "ref must have 2 entries"
        P = ctypes.c_int64(0)
        hv = ctypes.c_double(0.0)
        front = np.empty((EHVI_MAX_FRONT, 2))
        self._check(self.lib.tgp_ehvi_set_front(self._h, _ptr(Y) if Y.shape[0] else None, Y.shape[0], float(sf[0]), float(sf[1]),
                                                _ptr(ref), ctypes.byref(P), _ptr(front), ctypes.byref(hv)))
        return front[:P.value].copy(), hv.value

    @staticmethod
    def _handle_of(g):
        return g._h if isinstance(g._h, int) or g._h is None else g._h.value

    def sweep_ehvi(self, g, want_mu=False, want_sigma=False, want_second=False, want_value=False):
        """``tgp_sweep_ehvi``: the resident batch scored by the two-objective expected hypervolume improvement under
        this (objective 1's) model and ``g`` (objective 2's, a NativeGP) over the front of ``ehvi_set_front``, and its
        arg-max.  ``g``'s resident batch becomes its own copy of this handle's rows.  ``want_second``: ``mu2`` /
        ``sigma2`` (M,); ``want_value``: ``value`` (M,)."""
        out = _SweepOut(self.M, want_mu, want_sigma, False)
        mu2 = np.empty(self.M) if want_second else None
        sg2 = np.empty(self.M) if want_second else None
        value = np.empty(self.M) if want_value else None
        try:
            self._check(self.lib.tgp_sweep_ehvi(self._h, self._handle_of(g), _ptr(out.mu), _ptr(out.sg), _ptr(mu2), _ptr(sg2),
                                                _ptr(value), ctypes.byref(out.bv), ctypes.byref(out.bi), ctypes.byref(out.nc)))
        except Exception:
            # (as sweep_weighted: a second objective the call reached before it failed owns a copy of these rows already)
            if isinstance(g, NativeGP) and g is not self and g._h is not None and not g.host and self._resident_rows_are(g, self.M):
                g._batch_is(self.M)
            raise
        g._batch_is(self.M)           # g owns a copy of these rows now: nothing of a caller's to keep alive
        return out.result(mu2=mu2, sigma2=sg2, value=value)

    def ehvi_grad(self, Xq, g):
        """``tgp_ehvi_grad``: the value (m,) -- ``sweep_ehvi``'s formula -- and its gradient (m, D) at m <= 4096 points;
        float64 whatever the handles' dtypes"""
        Xq = _f64c(np.atleast_2d(Xq))
        assert Xq.ndim == 2 and Xq.shape[1] == self.D, "points must be (m, %d)" % self.D
        val = np.empty(Xq.shape[0])
        grad = np.empty(Xq.shape)
        self._check(self.lib.tgp_ehvi_grad(self._h, self._handle_of(g), _ptr(Xq), Xq.shape[0], _ptr(val), _ptr(grad)))
        return val, grad

    def ehvi_lbfgsb(self, X0, lo, hi, g, max_iter=15000):
        """``tgp_ehvi_lbfgsb``: ``acq_refine(lbfgsb=True)`` with the expected hypervolume improvement as the objective --
        L-BFGS-B from every start in lock-step, one batched ``tgp_ehvi_grad`` per round; returns (x (R, D), values (R,),
        status (R,), evaluations)"""
        X0 = _f64c(np.atleast_2d(X0))
        assert X0.ndim == 2 and X0.shape[1] == self.D, "start points must be (R, %d)" % self.D
        lo, hi = _bounds(lo, hi, self.D)
        R = X0.shape[0]
        x = np.empty((R, self.D))
        v = np.empty(R)
        st = np.empty(R, dtype=np.int64)
        its = ctypes.c_int64(0)
        self._check(self.lib.tgp_ehvi_lbfgsb(self._h, self._handle_of(g), _ptr(X0), R, _ptr(lo), _ptr(hi), int(max_iter), _ptr(x),
                                             _ptr(v), st.ctypes.data_as(_i64p), ctypes.byref(its)))
        return x, v, st, its.value

    def predict_cov(self, Xq, latent=False):
        """``tgp_predict_cov``: the joint posterior over m <= 4096 points -- mu (m,), cov (m, m) in raw units (symmetric
        bit for bit; the noise on the diagonal unless ``latent``) and the number of negative diagonal entries (not
        clamped, as sklearn's ``predict(return_cov=True)`` does not).  Works on host handles too."""
        Xq = _f64c(np.atleast_2d(Xq))
        assert Xq.ndim == 2 and Xq.shape[1] == self.D, "points must be (m, %d)" % self.D
        m = Xq.shape[0]
        mu, cov = np.empty(max(m, 1)), np.empty((max(m, 1), max(m, 1)))
        neg = ctypes.c_int64(0)
        self._check(self.lib.tgp_predict_cov(self._h, _ptr(Xq), m, 1 if latent else 0, _ptr(mu), _ptr(cov), ctypes.byref(neg)))
        return mu, cov, neg.value

    def sample_joint(self, Xq, n_samples=1, seed=0, eps=None, latent=False, nugget=1e-10):
        """``tgp_sample_joint``: ``n_samples`` <= 4096 exact joint samples at m <= 4096 points, y = mu + y_std Lc eps with
        Lc the Cholesky factor of the joint covariance + ``nugget`` I.  ``eps`` None: the normals come from the Philox
        stream of ``seed`` (GPU handles only); else (n_samples, m) standard normals used as they are.  Returns a dict:
        y (n_samples, m), eps (n_samples, m), mu (m,).  ``numpy.linalg.LinAlgError`` when a pivot fails."""
        Xq = _f64c(np.atleast_2d(Xq))
        assert Xq.ndim == 2 and Xq.shape[1] == self.D, "points must be (m, %d)" % self.D
        m, S = Xq.shape[0], int(n_samples)
        if eps is not None:
            eps = _f64c(np.asarray(eps, dtype=np.float64))
            assert eps.shape == (S, m), "eps must be (n_samples, m) = (%d, %d)" % (S, m)
        y, eo, mu = np.empty((max(S, 1), max(m, 1))), np.empty((max(S, 1), max(m, 1))), np.empty(max(m, 1))
        self._check(self.lib.tgp_sample_joint(self._h, _ptr(Xq), m, S, 1 if latent else 0, float(nugget), int(seed) % (1 << 64),
                                              _ptr(eps), _ptr(y), _ptr(eo), _ptr(mu)))
        return dict(y=y, eps=eo, mu=mu)

    def sweep_topk(self, k, acq, sf=1.0, incumbent=0.0, param=0.0):
        """the k best resident candidates: (indices (k,), values (k,)), best first"""
        vals = np.empty(int(k))
        idxs = np.empty(int(k), dtype=np.int64)
        nc = ctypes.c_int64(0)
        self._check(self.lib.tgp_sweep_topk(self._h, acq, float(sf), float(incumbent), float(param), int(k),
                                            _ptr(vals), idxs.ctypes.data_as(_i64p), ctypes.byref(nc)))
        return idxs, vals

    def acq_refine(self, X0, lo, hi, acq, sf=1.0, incumbent=0.0, param=0.0, max_iter=200, lbfgsb=False):
        """refine R start points together, maximising the acquisition: ``tgp_acq_refine`` (a projected L-BFGS on the
        GPU) or, ``lbfgsb=True``, ``tgp_acq_lbfgsb`` (L-BFGS-B itself in the library, SciPy's walk per restart, one
        batched evaluation per round); returns (x (R, D), values (R,), status (R,), evaluations)"""
        X0 = _f64c(np.atleast_2d(X0))
        assert X0.ndim == 2 and X0.shape[1] == self.D, "start points must be (R, %d)" % self.D
        lo, hi = _bounds(lo, hi, self.D)
        R = X0.shape[0]
        x = np.empty((R, self.D))
        v = np.empty(R)
        st = np.empty(R, dtype=np.int64)
        its = ctypes.c_int64(0)
        entry = self.lib.tgp_acq_lbfgsb if lbfgsb else self.lib.tgp_acq_refine
        self._check(entry(self._h, _ptr(X0), R, _ptr(lo), _ptr(hi), acq, float(sf),
                          float(incumbent), float(param), int(max_iter), _ptr(x), _ptr(v),
                          st.ctypes.data_as(_i64p), ctypes.byref(its)))
        return x, v, st, its.value

    def set_winner_out(self, dev_ptr, global_offset=0, keepalive=None):
        """attach (or, with None, detach) the (D + 2,) float64 device record every sweep packs its
        winner [value, global index, row] into -- the input of the sharded arg-max's all-gather"""
        self._check(self.lib.tgp_set_winner_out(self._h, _vp(int(dev_ptr)) if dev_ptr else None,
                                                int(global_offset)))
        self._winner_keepalive = keepalive

    def winner_wait(self, stream=None):
        """``tgp_winner_wait``: make a stream of the caller (``torch.cuda.current_stream().cuda_stream`` -- an integer --
        or None for the default stream) wait for the winner record of the last sweep: the explicit ordering between the
        library's stream, which packs the record, and the stream RCCL reads it on"""
        self._check(self.lib.tgp_winner_wait(self._h, _vp(int(stream)) if stream else None))

    def evaluate(self, Xc, acq=ACQ_NONE, sf=1.0, incumbent=0.0, param=0.0, want_mu=False,
                 want_sigma=False, want_acq=False):
        """set_candidates + sweep in ONE call (tgp_evaluate); same result dict as ``sweep``"""
        Xc = _f64c(Xc)
        assert Xc.ndim == 2 and Xc.shape[1] == self.D, "candidates must be (M, %d)" % self.D
        out = _SweepOut(Xc.shape[0], want_mu, want_sigma, want_acq)
        self._check(self.lib.tgp_evaluate(self._h, _ptr(Xc), Xc.shape[0], acq, float(sf), float(incumbent), float(param),
                                          *out.args()))
        self._batch_is(Xc.shape[0])
        return out.result(sweep_ms=self.profile_read()['last_sweep_ms'])

    def predict_batch(self, models, Xc, want_sigma=True):
        """T stored models (N <= 256, same kernel kind / D / normalize_y) x one batch of points in one
        call.  ``models``: list of dicts with X (N, D), y (N,), kind, constant, length_scale, noise,
        jitter, normalize_y.  Returns (mu (T, M), sigma (T, M) or None, lml (T,), n_clamped)."""
        T = len(models)
        Xc = _f64c(np.atleast_2d(Xc))
        D = Xc.shape[1]
        kind, norm = models[0]['kind'], bool(models[0]['normalize_y'])
        Xs = [_f64c(m['X']) for m in models]
        ys = [_f64c(m['y']).reshape(-1) for m in models]
        for m, X, y in zip(models, Xs, ys):
            assert m['kind'] == kind and bool(m['normalize_y']) == norm, "one kernel kind / normalisation per batch"
            assert X.ndim == 2 and X.shape[1] == D and X.shape[0] == y.shape[0]
        Ns = np.array([X.shape[0] for X in Xs], dtype=np.int64)
        ls = np.vstack([np.broadcast_to(np.asarray(m['length_scale'], dtype=np.float64), (D,)) for m in models])
        ls = _f64c(ls)
        cs = _f64c([m['constant'] for m in models])
        ns = _f64c([m['noise'] for m in models])
        js = _f64c([m['jitter'] for m in models])
        xp = (_vp * T)(*[X.ctypes.data for X in Xs])
        yp = (_vp * T)(*[y.ctypes.data for y in ys])
        M = Xc.shape[0]
        mu = np.empty((T, M))
        sg = np.empty((T, M)) if want_sigma else None
        lml = np.empty(T)
        nc = ctypes.c_int64(0)
        self._check(self.lib.tgp_predict_batch(self._h, T, Ns.ctypes.data_as(_i64p), D, xp, yp, KERNELS[kind],
                                               _ptr(cs), _ptr(ls), _ptr(ns), _ptr(js), 1 if norm else 0,
                                               _ptr(Xc), M, _ptr(mu), _ptr(sg), _ptr(lml), ctypes.byref(nc)))
        return mu, sg, lml, nc.value

    def acq_grad(self, Xq, acq=ACQ_NONE, sf=1.0, incumbent=0.0, param=0.0):
        """acquisition value (m,) and gradient (m, D) at a small batch of points"""
        Xq = _f64c(np.atleast_2d(Xq))
        assert Xq.ndim == 2 and Xq.shape[1] == self.D, "points must be (m, %d)" % self.D
        val = np.empty(Xq.shape[0])
        grad = np.empty(Xq.shape)
        self._check(self.lib.tgp_acq_grad(self._h, _ptr(Xq), Xq.shape[0], acq, float(sf), float(incumbent),
                                          float(param), _ptr(val), _ptr(grad)))
        return val, grad

    def profile_enable(self, on=True):
        self._check(self.lib.tgp_profile_enable(self._h, 1 if on else 0))

    def profile_reset(self):
        self._check(self.lib.tgp_profile_reset(self._h))

    def profile_read(self):
        tl, kl = ctypes.c_int64(), ctypes.c_int64()
        tm, km, fm, sm = (ctypes.c_double() for _ in range(4))
        self._check(self.lib.tgp_profile_read(self._h, ctypes.byref(tl), ctypes.byref(tm),
                                              ctypes.byref(kl), ctypes.byref(km),
                                              ctypes.byref(fm), ctypes.byref(sm)))
        return dict(trmm_launches=tl.value, trmm_ms=tm.value, kstar_launches=kl.value,
                    kstar_ms=km.value, last_fit_ms=fm.value, last_sweep_ms=sm.value)

    def last_timings(self):
        """device times (ms) of the last calls: fit, sweep, and the three stages of the LML gradient"""
        v = np.zeros(12)
        self._check(self.lib.tgp_last_timings(self._h, _ptr(v), 12))
        return dict(fit_ms=v[0], sweep_ms=v[1], grad_kinv_ms=v[2], grad_pairwise_ms=v[3], grad_ard_ms=v[4],
                    trmm_flops=v[5], sweep_f64=int(v[6]), small_fit_phases_us=[float(x) for x in v[7:12]])

    def last_prune(self):
        """what the last ``sweep`` did about pruning (``tgp_last_timings`` slots 12-14): state -1 = not eligible (outputs
        asked for, another acquisition or dtype, N <= 256, TGP_SWEEP_PRUNE=0), -2 = gated off (the noise is too small
        for the contraction's rounding), 0 = the pruned schedule ran, 1 = too many survivors: every candidate was
        contracted; lb_set / survivors = candidates of its two exact sets; screen = survivors of the matrix-core screen
        in front of the bound pass (slot 16), -1 where it does not apply (f64, Matern, TGP_PRUNE_SCREEN=0, not pruned);
        screen_arith = that screen's arithmetic (slot 18): 0 none, 1 f32, 2 fp16 planes (TGP_SCREEN_ARITH)"""
        v = np.zeros(19)
        self._check(self.lib.tgp_last_timings(self._h, _ptr(v), 19))
        return dict(state=int(v[12]), lb_set=int(v[13]), survivors=int(v[14]), screen=int(v[16]), screen_arith=int(v[18]))

    def last_prune_spec(self):
        """the speculative round of the last ``sweep``'s pruned schedule (``tgp_last_timings`` slot 21, TGP_PRUNE_SPEC):
        0 = not tried, 1 = hit (the runner-ups contracted beside the lb set covered every survivor: one exact round),
        2 = miss (the survivors' round ran as well).  ``last_prune()`` reads the same either way."""
        v = np.zeros(22)
        self._check(self.lib.tgp_last_timings(self._h, _ptr(v), 22))
        return int(v[21])

    def sweep_geometry(self):
        ch, npad = ctypes.c_int64(), ctypes.c_int64()
        self._check(self.lib.tgp_sweep_geometry(self._h, ctypes.byref(ch), ctypes.byref(npad)))
        return ch.value, npad.value
