"""Raw C ABI of the resident streaming fit (mps2qc_fit_brickwork_resident of include/mps2qc_hip.h) for the tests."""
import ctypes as C

import numpy as np

RESIDENT_OUTPUTS = ("opt_gates", "final_gates", "loss_history", "best_val", "n_iter", "last_envs", "last_overlap")
OPTIMISER = (3e-3, 0.9, 0.999, 1e-8)


def bit_reversed(n):
    """rev with little_endian[rev] = site0_msb (and back: the map is an involution)."""
    return np.array([int(format(i, f"0{n}b")[::-1], 2) for i in range(1 << n)])


def resident_raw_fit(n, sites, target, init, steps, only=RESIDENT_OUTPUTS, frozen=False, tol=1e-30, param_tol=0.0, opts=None,
                     shared=None):
    """One resident fit through the raw ABI with the optimiser 3e-3, 0.9, 0.999, 1e-8.  ``target``: a numpy array or a
    CUDA torch tensor (passed by data_ptr()); ``opts``: None (a NULL pointer) or a dict with any of target_on_device,
    target_little_endian, check_every, use_graph laid over the library's defaults; ``only``: the outputs that get a
    pointer, every other one is NULL.  Returns (rc, the arrays asked for, steps_enqueued)."""
    from tensorrl_qas_amd import _lib
    lib = _lib.load_mps2qc()
    sites = np.ascontiguousarray(sites, np.int32)
    init = np.ascontiguousarray(init, np.complex128)
    B, G = init.shape[0], len(sites)
    if isinstance(target, np.ndarray):
        target = np.ascontiguousarray(target, np.complex128)
        tptr = C.c_void_p(target.ctypes.data)
    else:
        tptr = C.c_void_p(target.data_ptr())
    shared = target.ndim == 1 if shared is None else shared
    out = dict(opt_gates=np.zeros_like(init), final_gates=np.zeros_like(init), loss_history=np.zeros((B, steps)),
               best_val=np.zeros(B), n_iter=np.zeros(B, np.int32), last_envs=np.zeros_like(init),
               last_overlap=np.zeros(B, np.complex128))
    ptr = {k: (v.ctypes.data_as(_lib.c_i32p if k == "n_iter" else _lib.c_f64p) if k in only else None) for k, v in out.items()}
    o = None
    if opts is not None:
        o = _lib.ResidentOpts()
        assert lib.mps2qc_resident_default_opts(C.byref(o)) == 0
        for k, v in opts.items():
            setattr(o, k, v)
    enq = C.c_int32(-1)
    rc = lib.mps2qc_fit_brickwork_resident(
        0, n, G, sites.ctypes.data_as(_lib.c_i32p), B, tptr, int(shared), init.ctypes.data_as(_lib.c_f64p), *OPTIMISER,
        int(frozen), steps, tol, param_tol, C.byref(o) if o is not None else None,
        *(ptr[k] for k in RESIDENT_OUTPUTS), None, C.byref(enq))
    return rc, {k: v for k, v in out.items() if k in only}, enq.value


def same_bits(a, b):
    """Every output of two runs is bit for bit the same."""
    assert set(a) == set(b)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
