"""ctypes binding of libfbstab_hip.so (the C-ABI in include/fbstab_hip.h).

This is plumbing for the Python tests and ``bench.py``: it passes raw pointers
(numpy host arrays or torch CUDA tensors) to the C entry points and adds no
computation of its own.  There is no fallback: if the shared library is missing
or no HIP device is usable, construction raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("FBSTAB_HIP_LIB", os.path.join(_HERE, "libfbstab_hip.so"))

MPC_SEQ = ("Q", "R", "S", "q", "r", "A", "B", "c", "E", "L", "d", "x0")
DENSE_ARR = ("H", "f", "G", "h", "A", "b")

HOST_POINTERS = 0
DEVICE_POINTERS = 1
ASYNC = 2
KEEP_MATRICES = 4

EXIT_FLAGS = {0: "SUCCESS", 1: "DIVERGENCE", 2: "MAXITERATIONS", 3: "PRIMAL_INFEASIBLE",
              4: "DUAL_INFEASIBLE", 5: "PRIMAL_DUAL_INFEASIBLE", 6: "SATURATE_ERROR"}


class Options(C.Structure):
    """fbstab_options_t (include/fbstab_types.h) == AlgorithmParameters
    (fbstab/fbstab_algorithm.h:48-82)."""
    _fields_ = [(n, C.c_double) for n in (
        "sigma0", "sigma_max", "sigma_min", "alpha", "beta", "eta", "delta",
        "gamma", "abs_tol", "rel_tol", "stall_tol", "infeas_tol",
        "inner_tol_max", "inner_tol_min")] + [(n, C.c_int) for n in (
            "max_newton_iters", "max_prox_iters", "max_inner_iters",
            "max_linesearch_iters", "check_feasibility",
            "nonmonotone_linesearch", "display_level", "reserved")]


def DefaultOptions(**kw) -> Options:
    """FBstabMpc::DefaultOptions / FBstabDense::DefaultOptions
    (fbstab_algorithm-impl.h:33-59); display is FINAL there, the batch path
    never prints so the field is carried but unused."""
    o = Options(1e-8, 1e-6, 1e-12, 0.95, 0.75, 1e-8, 0.2, 0.1, 1e-6, 1e-12, 1e-10,
                1e-8, 1e-2, 1e-12, 200, 30, 50, 20, 1, 1, 1, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def ReliableOptions(**kw) -> Options:
    """ReliableOptions (fbstab_algorithm-impl.h:61-74)."""
    o = DefaultOptions(sigma0=1e-4, sigma_max=1e-2, sigma_min=1e-10, beta=0.9,
                       abs_tol=1e-4, rel_tol=1e-6, max_linesearch_iters=40,
                       max_newton_iters=500, max_prox_iters=100,
                       nonmonotone_linesearch=0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


OUT_DTYPE = np.dtype([("eflag", np.int32), ("pad_", np.int32),
                      ("residual", np.float64), ("newton_iters", np.int32),
                      ("prox_iters", np.int32), ("solve_time", np.float64),
                      ("initial_residual", np.float64)])
assert OUT_DTYPE.itemsize == 40


class _MpcBatch(C.Structure):
    _fields_ = [("base", C.c_void_p * 12), ("stride", C.c_longlong * 12)]


class _DenseBatch(C.Structure):
    _fields_ = [("base", C.c_void_p * 6), ("stride", C.c_longlong * 6)]


class _VarBatch(C.Structure):
    _fields_ = [("base", C.c_void_p * 4), ("stride", C.c_longlong * 4)]


class _MpcGradBatch(C.Structure):
    _fields_ = [("base", C.c_void_p * 12), ("stride", C.c_longlong * 12)]


class _DenseGradBatch(C.Structure):
    _fields_ = [("base", C.c_void_p * 6), ("stride", C.c_longlong * 6)]


class _DenseOutBatch(C.Structure):
    """fbstab_dense_out_batch_t: where fbstab_hip_mpc_condense_batch writes H, f, A, b (the G and h slots unused)."""
    _fields_ = [("base", C.c_void_p * 6), ("stride", C.c_longlong * 6)]


class _MultiVarBatch(C.Structure):
    """fbstab_multi_var_batch_t: nrhs vectors (z, l, v) per QP."""
    _fields_ = [("base", C.c_void_p * 3), ("stride", C.c_longlong * 3), ("rhs_stride", C.c_longlong * 3)]


class _Plant(C.Structure):
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("stride_A", C.c_longlong), ("stride_B", C.c_longlong)]


class _SweepLog(C.Structure):
    _fields_ = [("z", C.c_void_p), ("l", C.c_void_p), ("v", C.c_void_p), ("x0", C.c_void_p), ("eflag", C.c_void_p)]


class _CondensedMap(C.Structure):
    """fbstab_condensed_map_t: M = [F; G], f_c(0), b_c(0) and their strides."""
    _fields_ = [("M", C.c_void_p), ("f0", C.c_void_p), ("b0", C.c_void_p), ("stride_M", C.c_longlong),
                ("stride_f0", C.c_longlong), ("stride_b0", C.c_longlong)]


class _CondensedSweepLog(C.Structure):
    """fbstab_condensed_sweep_log_t."""
    _fields_ = [("u", C.c_void_p), ("x", C.c_void_p), ("U", C.c_void_p), ("v", C.c_void_p), ("eflag", C.c_void_p),
                ("newton", C.c_void_p)]


class _CondensedRefs(C.Structure):
    """fbstab_condensed_refs_t: per-step q, r, c, d - base, doubles between steps, doubles between trajectories."""
    _fields_ = [("base", C.c_void_p * 4), ("step", C.c_longlong * 4), ("stride", C.c_longlong * 4)]


class _CondensedRefGrad(C.Structure):
    """fbstab_condensed_ref_grad_t: where the per-step gradients of q, r, c, d go."""
    _fields_ = [("base", C.c_void_p * 4), ("step", C.c_longlong * 4), ("stride", C.c_longlong * 4)]


class _CondensedRefImages(C.Structure):
    """fbstab_condensed_ref_images_t: f0_k, b0_k and their steps and strides."""
    _fields_ = [("f0", C.c_void_p), ("b0", C.c_void_p), ("step_f0", C.c_longlong), ("step_b0", C.c_longlong),
                ("stride_f0", C.c_longlong), ("stride_b0", C.c_longlong)]


class _CondensedSweepDir(C.Structure):
    """fbstab_condensed_sweep_dir_t: the directions of x0, of the disturbances and of the images f0_k, b0_k."""
    _fields_ = [("dx0", C.c_void_p), ("stride_dx0", C.c_longlong), ("dw", C.c_void_p), ("df0", C.c_void_p),
                ("db0", C.c_void_p), ("step_df0", C.c_longlong), ("step_db0", C.c_longlong),
                ("stride_df0", C.c_longlong), ("stride_db0", C.c_longlong)]


class _SweepScenario(C.Structure):
    """fbstab_sweep_scenario_t: the disturbances (device pointer or NULL) and the shift flag."""
    _fields_ = [("w", C.c_void_p), ("shift", C.c_int)]


_libs: Dict[str, C.CDLL] = {}
_torch = None  # the torch module, once load_library has imported it (device arrays need a loaded library anyway)
_current = LIB_PATH  # the library new solver objects bind to (see `library`)


def current_library_path() -> str:
    """Path of the library new solver objects bind to (what bench.py hashes as "this build")."""
    return _current


class library:
    """``with hip_api.library(path):`` - solver objects created inside bind to ANOTHER build of the
    same sources at ``path`` (the tests compare a pattern-initialised build with the product
    library, tests/helpers.py: VARIANT_LIBS); both libraries can be in use in one process."""

    def __init__(self, path: str):
        self.path = path

    def __enter__(self):
        global _current
        self.prev, _current = _current, self.path
        return load_library()

    def __exit__(self, *exc):
        global _current
        _current = self.prev
        return False


def load_library() -> C.CDLL:
    """Load libfbstab_hip.so; raises (never falls back) when it is absent."""
    LIB_PATH = _current
    if LIB_PATH in _libs:
        return _libs[LIB_PATH]
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `make -C fbstab_amd/csrc` "
            "(__graft_entry__.build()); fbstab_amd has no CPU fallback")
    # torch (device memory / streams / torch.distributed plumbing) bundles its
    # own HIP runtime: import it first so this process ends up with ONE
    # libamdhip64 (loading ours first makes torch see "No HIP GPUs").
    global _torch
    try:
        import torch
        _torch = torch
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    lib.fbstab_hip_last_error.restype = C.c_char_p
    for kind in ("mpc", "dense"):
        getattr(lib, f"fbstab_hip_{kind}_last_kernel_ms").restype = C.c_double
        getattr(lib, f"fbstab_hip_{kind}_last_kernel_ms").argtypes = [C.c_void_p]
        getattr(lib, f"fbstab_hip_{kind}_destroy").argtypes = [C.c_void_p]
        getattr(lib, f"fbstab_hip_{kind}_set_options").argtypes = [C.c_void_p, C.c_void_p]
        getattr(lib, f"fbstab_hip_{kind}_get_options").argtypes = [C.c_void_p, C.c_void_p]
        getattr(lib, f"fbstab_hip_{kind}_solve_batch").argtypes = [
            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        getattr(lib, f"fbstab_hip_{kind}_solve_batch_final").argtypes = [
            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        getattr(lib, f"fbstab_hip_{kind}_query").argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        getattr(lib, f"fbstab_hip_{kind}_solve_traced").argtypes = [
            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.fbstab_hip_mpc_kernel_name.restype = C.c_char_p
    lib.fbstab_hip_mpc_kernel_name.argtypes = [C.c_void_p]
    if hasattr(lib, "fbstab_hip_mpc_adjoint_batch"):  # (absent from a build of an earlier round loaded for an A/B)
        lib.fbstab_hip_mpc_adjoint_batch.argtypes = [
            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(lib, "fbstab_hip_mpc_adjoint_kernel_name"):  # (absent from an earlier build loaded for an A/B)
        lib.fbstab_hip_mpc_adjoint_kernel_name.restype = C.c_char_p
        lib.fbstab_hip_mpc_adjoint_kernel_name.argtypes = [C.c_void_p]
    if hasattr(lib, "fbstab_hip_dense_adjoint_batch"):  # (absent from a build of an earlier round loaded for an A/B)
        lib.fbstab_hip_dense_adjoint_batch.argtypes = [
            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
            C.c_void_p, C.c_int, C.c_void_p]
    for kind in ("mpc", "dense"):  # (absent from a build of an earlier round loaded for an A/B)
        if hasattr(lib, f"fbstab_hip_{kind}_adjoint_batch_reduced"):
            getattr(lib, f"fbstab_hip_{kind}_adjoint_batch_reduced").argtypes = [
                C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    for kind in ("mpc", "dense"):  # (absent from a build of an earlier round loaded for an A/B)
        if hasattr(lib, f"fbstab_hip_{kind}_tangent_batch"):
            getattr(lib, f"fbstab_hip_{kind}_tangent_batch").argtypes = [
                C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(lib, "fbstab_hip_mpc_kkt_solve_batch"):  # (absent from an earlier build loaded for an A/B)
        lib.fbstab_hip_mpc_kkt_solve_batch.argtypes = [
            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
            C.c_int, C.c_void_p]
        lib.fbstab_hip_mpc_x0_sensitivity_batch.argtypes = [
            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_longlong,
            C.c_void_p, C.c_int, C.c_void_p]
    if hasattr(lib, "fbstab_hip_dense_kkt_solve_batch"):  # (absent from an earlier build loaded for an A/B)
        lib.fbstab_hip_dense_kkt_solve_batch.argtypes = [
            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
            C.c_int, C.c_void_p]
        lib.fbstab_hip_dense_jacobian_batch.argtypes = [
            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int,
            C.c_void_p]
    if hasattr(lib, "fbstab_hip_mpc_condense_batch"):  # (absent from an earlier build loaded for an A/B)
        lib.fbstab_hip_mpc_condensed_sizes.argtypes = [C.c_int] * 4 + [C.c_void_p] * 3
        lib.fbstab_hip_mpc_condense_batch.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                      C.c_void_p]
        lib.fbstab_hip_mpc_expand_batch.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                    C.c_void_p]
    if hasattr(lib, "fbstab_hip_mpc_condensed_adjoint_batch"):  # (absent from an earlier build loaded for an A/B)
        lib.fbstab_hip_mpc_condensed_adjoint_batch.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 4 + [
            C.c_double] + [C.c_void_p] * 5
    if hasattr(lib, "fbstab_hip_mpc_condensed_tangent_batch"):  # (absent from an earlier build loaded for an A/B)
        lib.fbstab_hip_mpc_condensed_tangent_batch.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 4 + [
            C.c_double] + [C.c_void_p] * 5
    if hasattr(lib, "fbstab_hip_mpc_condensed_multi_sizes"):  # (absent from an earlier build loaded for an A/B)
        lib.fbstab_hip_mpc_condensed_multi_sizes.argtypes = [C.c_int] * 6 + [C.c_void_p] * 3
        lib.fbstab_hip_mpc_condensed_kkt_solve_batch.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3 + [
            C.c_int, C.c_void_p, C.c_double, C.c_void_p, C.c_int] + [C.c_void_p] * 3
        lib.fbstab_hip_mpc_condensed_x0_sensitivity_batch.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3 + [
            C.c_double, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int] + [C.c_void_p] * 3
    if hasattr(lib, "fbstab_hip_mpc_condensed_receding_sweep"):  # (absent from an earlier build loaded for an A/B)
        lib.fbstab_hip_mpc_condensed_sweep_sizes.argtypes = [C.c_int] * 6 + [C.c_void_p] * 3
        lib.fbstab_hip_mpc_condensed_x0_map_batch.argtypes = [C.c_int] * 5 + [C.c_void_p, C.c_void_p, C.c_longlong,
                                                              C.c_int, C.c_void_p]
        lib.fbstab_hip_mpc_condensed_receding_sweep.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 6 + [
            C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    if hasattr(lib, "fbstab_hip_mpc_condensed_receding_sweep_adjoint"):  # (absent from an earlier build loaded for an A/B)
        lib.fbstab_hip_mpc_condensed_sweep_adjoint_sizes.argtypes = [C.c_int] * 6 + [C.c_void_p] * 4
        lib.fbstab_hip_mpc_condensed_receding_sweep_adjoint.argtypes = [C.c_void_p] + [C.c_int] * 5 + [
            C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_double] + [C.c_void_p] * 5 + [
            C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    if hasattr(lib, "fbstab_hip_mpc_condensed_tracking_sweep"):  # (absent from an earlier build loaded for an A/B)
        lib.fbstab_hip_mpc_condensed_reference_sizes.argtypes = [C.c_int] * 6 + [C.c_void_p] * 2
        lib.fbstab_hip_mpc_condensed_reference_images_batch.argtypes = [C.c_int] * 6 + [C.c_void_p] * 3 + [
            C.c_int, C.c_int, C.c_void_p]
        lib.fbstab_hip_mpc_condensed_tracking_sweep.argtypes = [C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 6 + [
            C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.fbstab_hip_mpc_condensed_tracking_sweep_adjoint.argtypes = [C.c_void_p] + [C.c_int] * 5 + [
            C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 3 + [C.c_double] + [C.c_void_p] * 3 + [
            C.c_int] + [C.c_void_p] * 3 + [C.c_int, C.c_void_p, C.c_void_p]
    if hasattr(lib, "fbstab_hip_mpc_condensed_receding_sweep_tangent"):  # (absent from an earlier build loaded for an A/B)
        lib.fbstab_hip_mpc_condensed_sweep_tangent_sizes.argtypes = [C.c_int] * 6 + [C.c_void_p] * 3
        lib.fbstab_hip_mpc_condensed_receding_sweep_tangent.argtypes = [C.c_void_p] + [C.c_int] * 5 + [
            C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 2 + [C.c_double] + [C.c_void_p] * 3 + [
            C.c_int, C.c_void_p, C.c_void_p]
    if hasattr(lib, "fbstab_hip_mpc_refined_steps"):  # (absent from a round-4 build loaded for an A/B: FBSTAB_HIP_LIB)
        lib.fbstab_hip_mpc_refined_steps.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(lib, "fbstab_hip_mpc_queue_order"):  # (absent from an earlier build loaded for an A/B)
        lib.fbstab_hip_mpc_queue_order.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.fbstab_hip_mpc_receding_sweep.argtypes = [
        C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "fbstab_hip_mpc_receding_sweep_logged"):  # (absent from an earlier build loaded for an A/B)
        lib.fbstab_hip_mpc_receding_sweep_logged.argtypes = lib.fbstab_hip_mpc_receding_sweep.argtypes + [C.c_void_p]
        lib.fbstab_hip_mpc_receding_sweep_adjoint.argtypes = [
            C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
            C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.fbstab_hip_mpc_sweep_adjoint_kernel_name.restype = C.c_char_p
        lib.fbstab_hip_mpc_sweep_adjoint_kernel_name.argtypes = [C.c_void_p]
    if hasattr(lib, "fbstab_hip_mpc_receding_sweep_scenario"):  # (absent from an earlier build loaded for an A/B)
        lib.fbstab_hip_mpc_receding_sweep_scenario.argtypes = lib.fbstab_hip_mpc_receding_sweep.argtypes + [
            C.c_void_p, C.c_void_p]
    lib.fbstab_hip_shard_group_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.fbstab_hip_shard_group_destroy.argtypes = [C.c_void_p]
    lib.fbstab_hip_shard_group_stats.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    for name in ("fbstab_hip_mpc_solve_batch_sharded", "fbstab_hip_dense_solve_batch_sharded"):
        getattr(lib, name).argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_void_p]
    lib.fbstab_hip_mpc_receding_sweep_sharded.argtypes = [C.c_void_p] * 7 + [C.c_int, C.c_int, C.c_void_p, C.c_int,
                                                          C.c_void_p, C.c_void_p]
    lib.fbstab_hip_mpc_create.argtypes = [C.c_int] * 6 + [C.c_void_p]
    if hasattr(lib, "fbstab_hip_mpc_create_in_flight"):  # (absent from a build of an earlier round loaded for an A/B)
        lib.fbstab_hip_mpc_create_in_flight.argtypes = [C.c_int] * 7 + [C.c_void_p]
    lib.fbstab_hip_dense_create.argtypes = [C.c_int] * 5 + [C.c_void_p]
    lib.fbstab_hip_dense_set_factorisation.argtypes = [C.c_void_p, C.c_int, C.c_int]
    lib.fbstab_hip_dense_get_factorisation.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    _libs[LIB_PATH] = lib
    return lib


EXPORTED_SYMBOLS = (
    "fbstab_hip_last_error", "fbstab_hip_device_count",
    "fbstab_hip_mpc_create", "fbstab_hip_mpc_destroy", "fbstab_hip_mpc_set_options",
    "fbstab_hip_mpc_get_options", "fbstab_hip_mpc_solve_batch", "fbstab_hip_mpc_solve_batch_final",
    "fbstab_hip_mpc_solve_traced", "fbstab_hip_mpc_receding_sweep",
    "fbstab_hip_mpc_last_kernel_ms", "fbstab_hip_mpc_query", "fbstab_hip_mpc_kernel_name",
    "fbstab_hip_mpc_refined_steps", "fbstab_hip_mpc_queue_order", "fbstab_hip_mpc_create_in_flight",
    "fbstab_hip_mpc_debug_newton", "fbstab_hip_mpc_adjoint_batch", "fbstab_hip_mpc_adjoint_kernel_name",
    "fbstab_hip_mpc_adjoint_batch_reduced", "fbstab_hip_mpc_tangent_batch", "fbstab_hip_debug_stamps",
    "fbstab_hip_mpc_receding_sweep_logged", "fbstab_hip_mpc_receding_sweep_adjoint",
    "fbstab_hip_mpc_sweep_adjoint_kernel_name", "fbstab_hip_mpc_receding_sweep_scenario",
    "fbstab_hip_mpc_kkt_solve_batch", "fbstab_hip_mpc_x0_sensitivity_batch",
    "fbstab_hip_mpc_condensed_sizes", "fbstab_hip_mpc_condense_batch", "fbstab_hip_mpc_expand_batch",
    "fbstab_hip_mpc_condensed_adjoint_batch", "fbstab_hip_mpc_condensed_tangent_batch",
    "fbstab_hip_mpc_condensed_multi_sizes", "fbstab_hip_mpc_condensed_kkt_solve_batch",
    "fbstab_hip_mpc_condensed_x0_sensitivity_batch",
    "fbstab_hip_mpc_condensed_sweep_sizes", "fbstab_hip_mpc_condensed_x0_map_batch",
    "fbstab_hip_mpc_condensed_receding_sweep",
    "fbstab_hip_mpc_condensed_sweep_adjoint_sizes", "fbstab_hip_mpc_condensed_receding_sweep_adjoint",
    "fbstab_hip_mpc_condensed_reference_sizes", "fbstab_hip_mpc_condensed_reference_images_batch",
    "fbstab_hip_mpc_condensed_tracking_sweep", "fbstab_hip_mpc_condensed_tracking_sweep_adjoint",
    "fbstab_hip_mpc_condensed_sweep_tangent_sizes", "fbstab_hip_mpc_condensed_receding_sweep_tangent",
    "fbstab_hip_dense_kkt_solve_batch", "fbstab_hip_dense_jacobian_batch",
    "fbstab_hip_dense_create", "fbstab_hip_dense_destroy", "fbstab_hip_dense_set_options",
    "fbstab_hip_dense_get_options", "fbstab_hip_dense_solve_batch", "fbstab_hip_dense_solve_batch_final",
    "fbstab_hip_dense_solve_traced", "fbstab_hip_dense_adjoint_batch",
    "fbstab_hip_dense_adjoint_batch_reduced", "fbstab_hip_dense_tangent_batch",
    "fbstab_hip_dense_debug_newton", "fbstab_hip_dense_last_kernel_ms", "fbstab_hip_dense_query",
    "fbstab_hip_dense_set_factorisation", "fbstab_hip_dense_get_factorisation",
    "fbstab_hip_shard_group_create", "fbstab_hip_shard_group_destroy", "fbstab_hip_shard_group_stats",
    "fbstab_hip_mpc_solve_batch_sharded", "fbstab_hip_mpc_receding_sweep_sharded",
    "fbstab_hip_dense_solve_batch_sharded")


class FBstabHipError(RuntimeError):
    """Mirrors the std::runtime_error the reference throws (fbstab_mpc.cc:62-65,
    fbstab_mpc.h:229-242, ...)."""


def _check(lib, rc):
    if rc != 0:
        raise FBstabHipError(f"[{rc}] {lib.fbstab_hip_last_error().decode()}")


def _is_torch(a) -> bool:
    return type(a).__module__.startswith("torch")


def _shared_stride(a, st: int, B: int) -> int:
    """Batch stride of a problem array in a batch of ``B``: a ``(1, len)`` array beside B > 1 QPs is shared by all
    of them (stride 0, include/fbstab_hip.h)."""
    assert a.shape[0] == B or a.shape[0] == 1, (a.shape, B)
    return 0 if (a.shape[0] == 1 and B > 1) else st


def _ptr_stride(a, length: int):
    """(pointer, batch stride in doubles, is_device) of a (batch, length) array."""
    if _is_torch(a):
        import torch
        assert a.dtype == torch.float64 and a.dim() == 2 and a.shape[1] == length, \
            (a.shape, length)
        assert a.stride(1) == 1 or length <= 1
        return a.data_ptr(), (a.stride(0) if a.shape[0] > 1 else length), a.is_cuda
    assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.ndim == 2 \
        and a.shape[1] == length, (getattr(a, "shape", None), length)
    assert a.strides[1] == 8 or length <= 1
    return a.ctypes.data, (a.strides[0] // 8 if a.shape[0] > 1 else length), False


def _fill_block(block, names, lens, arrays, B, dev_flags, optional=False, shared=True):
    """Fills a batch, direction or gradient block (``base[i]``, ``stride[i]`` per name) from a dict of ``(rows, len)``
    arrays and returns ``B``.  A slot of length 0 is NULL with stride 0.  ``optional``: so is an absent name or None
    (otherwise the name is required).  ``shared``: a ``(1, len)`` array beside B > 1 QPs is shared by all of them,
    stride 0 (otherwise the array's own row stride stands, and B = None takes the rows of the first array).  The
    device flag of every array read goes to ``dev_flags``."""
    for i, (k, n) in enumerate(zip(names, lens)):
        a = None if n == 0 else (arrays.get(k) if optional else arrays[k])
        if a is None:
            assert n == 0 or optional, f"{k} is required"
            block.base[i], block.stride[i] = None, 0
            continue
        p, st, d = _ptr_stride(a, n)
        if B is None:
            B = a.shape[0]
        block.base[i], block.stride[i] = p, (_shared_stride(a, st, B) if shared else st)
        dev_flags.append(d)
    return B


def _fill_vars(arrs, var_lens, B, dev_flags, optional=False, vb=None):
    """A _VarBatch of the ``(B, n)`` arrays ``arrs`` (z, l, v[, y] or seeds, adjoints, ...); a vector of length 0 is
    NULL.  Every other slot is required, except that with ``optional`` the slots behind the first may be None.
    B = None: rows are not compared (the root block of a sharded call)."""
    vb = _VarBatch() if vb is None else vb
    for i, (a, n) in enumerate(zip(arrs, var_lens)):
        if a is None or n == 0:
            assert n == 0 or (optional and i > 0), "z, l, v and gz are required"
            vb.base[i], vb.stride[i] = None, 0
            continue
        p, st, d = _ptr_stride(a, n)
        assert B is None or a.shape[0] == B
        vb.base[i], vb.stride[i] = p, st
        dev_flags.append(d)
    return vb


def _fill_multi(arrs, var_lens, B, K, dev_flags, optional=False, first_required=True):
    """A _MultiVarBatch of the ``(B, K, n)`` arrays ``arrs`` (seeds or steps of K right-hand sides per QP); a
    ``(K, n)`` array is one block shared by the batch (stride 0).  None is a NULL slot (``optional``; the first
    slot only without ``first_required``)."""
    mb = _MultiVarBatch()
    for i, (a, n) in enumerate(zip(arrs, var_lens)):
        if a is None:
            assert optional and (i > 0 or not first_required), "gz is required"
            mb.base[i], mb.stride[i], mb.rhs_stride[i] = None, 0, 0
            continue
        tor = _is_torch(a)
        assert a.dtype == (_torch.float64 if tor else np.float64), a.dtype
        shape = tuple(a.shape)
        assert shape == (B, K, n) or shape == (K, n), (shape, (B, K, n))
        st = tuple(a.stride()) if tor else tuple(t // 8 for t in a.strides)
        assert st[-1] == 1 or n <= 1
        mb.base[i] = a.data_ptr() if tor else a.ctypes.data
        mb.stride[i] = (st[0] if B > 1 else K * n) if len(shape) == 3 else 0
        mb.rhs_stride[i] = st[-2] if K > 1 else n
        dev_flags.append(a.is_cuda if tor else False)
    return mb


class _Host:
    """Allocators for what a host-pointer call returns (numpy)."""
    on_dev = False

    @staticmethod
    def zeros(like, shape, dtype="f8"):
        return np.zeros(shape, dtype=dtype)

    @staticmethod
    def out(like, B):
        return np.zeros(B, dtype=OUT_DTYPE)

    @staticmethod
    def ptr(a):
        return a.ctypes.data


class _Device:
    """... and a device-pointer call (torch tensors on the device of ``like``)."""
    on_dev = True

    @staticmethod
    def zeros(like, shape, dtype="f8"):
        return _torch.zeros(shape, dtype={"f8": _torch.float64, "i4": _torch.int32}[dtype], device=like.device)

    @staticmethod
    def out(like, B):
        return _torch.zeros((B, 40), dtype=_torch.uint8, device=like.device)

    @staticmethod
    def ptr(a):
        return a.data_ptr()


def _placement(dev_flags, like, stream=0, async_=False, keep_matrices=False):
    """Host or device?  From the device flags collected while the call's blocks were filled: ``(where, flags,
    stream)`` - ``where`` is _Host or _Device, whose ``zeros`` / ``out`` / ``ptr`` make status, SolverOut records and
    zero arrays where the data lives; ``flags`` the flags word of the C call; ``stream`` the caller's, or for device
    arrays torch's current stream: the arrays were produced there (0 is the null stream, which the handle's own
    blocking stream is ordered with)."""
    on_dev = all(dev_flags)
    assert on_dev or not any(dev_flags), "mix of host and device arrays"
    if not on_dev:
        return _Host, HOST_POINTERS, stream
    if not stream:
        stream = _torch.cuda.current_stream(like.device).cuda_stream
    return _Device, DEVICE_POINTERS | (ASYNC if async_ else 0) | (KEEP_MATRICES if keep_matrices else 0), stream


class _SolverBase:
    _kind = ""

    def __init__(self):
        self._h = C.c_void_p()
        self._lib = load_library()

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            getattr(self._lib, f"fbstab_hip_{self._kind}_destroy")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def UpdateOptions(self, options: Options):
        _check(self._lib, getattr(self._lib, f"fbstab_hip_{self._kind}_set_options")(
            self._h, C.byref(options)))

    def CurrentOptions(self) -> Options:
        o = Options()
        _check(self._lib, getattr(self._lib, f"fbstab_hip_{self._kind}_get_options")(
            self._h, C.byref(o)))
        return o

    def last_kernel_ms(self) -> float:
        return float(getattr(self._lib, f"fbstab_hip_{self._kind}_last_kernel_ms")(self._h))

    def query(self) -> Dict[str, int]:
        sb, lds, wg, th = C.c_longlong(), C.c_int(), C.c_int(), C.c_int()
        _check(self._lib, getattr(self._lib, f"fbstab_hip_{self._kind}_query")(
            self._h, C.byref(sb), C.byref(lds), C.byref(wg), C.byref(th)))
        return dict(scratch_bytes=sb.value, lds_bytes=lds.value, workgroups=wg.value,
                    threads=th.value)

    def _solve(self, batch_struct, names: Sequence[str], lens: Sequence[int], arrays,
               var_lens, z, l, v, y, out, stream, async_, keep_matrices=False, norms=False):
        dev_flags = []
        B = z.shape[0]
        _fill_block(batch_struct, names, lens, arrays, B, dev_flags)
        vb = _fill_vars((z, l, v, y), var_lens, B, dev_flags)
        where, flags, stream = _placement(dev_flags, z, stream, async_, keep_matrices)
        if out is None:
            out = where.out(z, B)
        out_ptr = where.ptr(out)
        if norms:
            # fbstab_hip_*_solve_batch_final: (B, 4) |rz| |rl| |rv| tolerance, living where out lives
            nrm = where.zeros(z, (B, 4))
            nptr = where.ptr(nrm)
            rc = getattr(self._lib, f"fbstab_hip_{self._kind}_solve_batch_final")(
                self._h, B, C.byref(batch_struct), C.byref(vb), out_ptr, C.c_void_p(nptr), flags,
                C.c_void_p(stream) if stream else None)
            _check(self._lib, rc)
            return out, nrm
        rc = getattr(self._lib, f"fbstab_hip_{self._kind}_solve_batch")(
            self._h, B, C.byref(batch_struct), C.byref(vb), out_ptr, flags,
            C.c_void_p(stream) if stream else None)
        _check(self._lib, rc)
        return out

    def _adjoint(self, fn, batch_struct, grad_struct, names: Sequence[str], lens: Sequence[int], data,
                 z, l, v, gz, gl, gv, sigma, want, adj, stream, async_, reduce=(), out=None):
        """fbstab_hip_*_adjoint_batch (``fn``) behind ``Adjoint``; an array of length 0 is a NULL slot.  With names
        in ``reduce`` the call goes to fbstab_hip_*_adjoint_batch_reduced, those slots with stride 0."""
        reduce = tuple(reduce)
        want = tuple(names if want is None else want) + tuple(k for k in reduce if want is not None and k not in want)
        unknown = (set(want) | set(reduce)) - set(names)
        assert not unknown, unknown
        if reduce:
            fn = getattr(self._lib, f"fbstab_hip_{self._kind}_adjoint_batch_reduced")
        dev_flags = []
        B = z.shape[0]
        _fill_block(batch_struct, names, lens, data, B, dev_flags)
        var_lens = (self.nz, self.nl, self.nv)
        xb = _fill_vars((z, l, v), var_lens, B, dev_flags)
        sb = _fill_vars((gz, gl, gv), var_lens, B, dev_flags, optional=True)
        where, flags, stream = _placement(dev_flags, z, stream, async_)
        on_dev = where.on_dev
        status = where.zeros(z, B, "i4")
        # a name in `reduce` gets ONE array, the sum over the batch: stride 0 whatever B is
        res = {k: where.zeros(z, (1 if k in reduce else B, n)) for k, n in zip(names, lens) if k in reduce or k in want}
        _fill_block(grad_struct, names, lens, res, B, [], optional=True)
        for k in reduce:
            grad_struct.stride[names.index(k)] = 0
        ab = None
        if adj:
            for k, n in zip(("dz", "dl", "dv"), var_lens):
                res[k] = where.zeros(z, (B, n))
            ab = _fill_vars((res["dz"], res["dl"], res["dv"]), var_lens, B, [])
        args = [self._h, B, C.byref(batch_struct), C.byref(xb), C.byref(sb), C.c_double(sigma), C.byref(grad_struct),
                C.byref(ab) if ab is not None else None,
                C.c_void_p(where.ptr(status))]
        if reduce:
            # the SolverOut records of the solve, living where status lives (None: no QP is left out for its eflag)
            if out is not None:
                assert _is_torch(out) == on_dev and out.shape[0] == B, "out lives where the arrays live"
                args.append(C.c_void_p(where.ptr(out)))
            else:
                args.append(None)
        else:
            assert out is None, "out= takes part in a reduced call only"
        _check(self._lib, fn(*args, flags, C.c_void_p(stream) if stream else None))
        res["status"] = status
        return res


def _tangent(self, batch_struct, dir_struct, names, lens, data, z, l, v, ddata, sigma, rhs, stream, async_):
    """fbstab_hip_*_tangent_batch behind ``Tangent``; an array of length 0, an absent name and None are NULL
    slots of ``ddata``, a ``(1, len)`` direction beside B > 1 QPs has stride 0."""
    unknown = set(ddata) - set(names)
    assert not unknown, unknown
    dev_flags = []
    B = z.shape[0]
    _fill_block(batch_struct, names, lens, data, B, dev_flags)
    _fill_block(dir_struct, names, lens, ddata, B, dev_flags, optional=True)
    var_lens = (self.nz, self.nl, self.nv)
    xb = _fill_vars((z, l, v), var_lens, B, dev_flags)
    where, flags, stream = _placement(dev_flags, z, stream, async_)
    if where.on_dev:
        zeros = lambda n: where.zeros(z, (B, n))
    else:
        zeros = lambda n: np.zeros((max(B, 1), n))[:B]   # (an empty batch keeps the strides of a row)
    status = where.zeros(z, B, "i4")
    res = {k: zeros(n) for k, n in zip(("dz", "dl", "dv"), var_lens)}
    db = _fill_vars((res["dz"], res["dl"], res["dv"]), var_lens, B, [])
    rb = None
    if rhs:
        res.update({k: zeros(n) for k, n in zip(("gz", "gl", "gv"), var_lens)})
        rb = _fill_vars((res["gz"], res["gl"], res["gv"]), var_lens, B, [])
    fn = getattr(self._lib, f"fbstab_hip_{self._kind}_tangent_batch")
    _check(self._lib, fn(self._h, B, C.byref(batch_struct), C.byref(xb), C.byref(dir_struct), C.c_double(sigma),
                         C.byref(db), C.byref(rb) if rb is not None else None,
                         C.c_void_p(where.ptr(status)), flags, C.c_void_p(stream) if stream else None))
    res["status"] = status
    return res


def _multi_call(self, batch_struct, names, lens, fn, data, z, l, v, K, seeds, head, sigma, want, gain_shape, stream,
                async_):
    """The many-right-hand-side calls behind ``KktSolve``, ``X0Sensitivity`` and ``Jacobian``: ``fn(handle, B, data, x,
    *head, sigma, step, [gain, gain_stride,] status, flags, stream)``.  ``seeds``: (gz, gl, gv), which travel with K at
    the head (fbstab_hip_*_kkt_solve_batch), or None (the seeds are generated in the kernel).  ``gain_shape``: None,
    or the ``(cols, rows)`` of the column-major per-QP block the call takes behind ``step`` - allocated where ``want``
    names ``"gain"``, NULL otherwise.  A vector of length 0 - the l slots with nl == 0 - travels as a NULL slot."""
    dev_flags = []
    B = z.shape[0]
    _fill_block(batch_struct, names, lens, data, B, dev_flags)
    var_lens = (self.nz, self.nl, self.nv)
    xb = _fill_vars((z, l, v), var_lens, B, dev_flags)
    live = lambda arrs: tuple(None if n == 0 else a for a, n in zip(arrs, var_lens))
    if seeds is not None:
        head = (K, C.byref(_fill_multi(live(seeds), var_lens, B, K, dev_flags, optional=True))) + tuple(head)
    where, flags, stream = _placement(dev_flags, z, stream, async_)
    status = where.zeros(z, B, "i4")
    if where.on_dev:
        zeros = lambda *shape: where.zeros(z, (B,) + shape)
    else:
        zeros = lambda *shape: np.zeros((max(B, 1),) + shape)[:B]   # (an empty batch keeps the strides of a row)
    res = {k: zeros(K, n) for k, n in zip(("dz", "dl", "dv"), var_lens) if k in want}
    ob = _fill_multi(live(tuple(res.get(k) for k in ("dz", "dl", "dv"))), var_lens, B, K, [], optional=True,
                     first_required=False) if res else None
    gain = gain_shape is not None and "gain" in want
    extra = ()
    if gain_shape is not None:
        if gain:
            res["gain"] = zeros(*gain_shape)
        extra = (C.c_void_p(where.ptr(res["gain"])) if gain else None, gain_shape[0] * gain_shape[1])
    _check(self._lib, fn(self._h, B, C.byref(batch_struct), C.byref(xb), *head, C.c_double(sigma),
                         C.byref(ob) if ob is not None else None, *extra, C.c_void_p(where.ptr(status)), flags,
                         C.c_void_p(stream) if stream else None))
    if gain:
        res["gain"] = res["gain"].transpose(1, 2) if where.on_dev else res["gain"].transpose(0, 2, 1)
    res["status"] = status
    return res


def _solve_traced(self, batch_struct, names, lens, arrays, var_lens, z, l, v, y, capacity):
    """fbstab_hip_*_solve_traced for ONE QP in (1, n) numpy arrays.  Returns
    ``(out, records)``; records is ``(n, 8)``: kind, i0, i1, v0..v4
    (fbstab_trace_record_t, include/fbstab_types.h)."""
    dev_flags = []
    B = _fill_block(batch_struct, names, lens, arrays, None, dev_flags, shared=False)
    vb = _fill_vars((z, l, v, y), var_lens, 1, dev_flags)
    assert B == 1 and not any(dev_flags)
    out = np.zeros(1, dtype=OUT_DTYPE)
    rec = np.zeros((capacity, 8))
    count = C.c_int(0)
    rc = getattr(self._lib, f"fbstab_hip_{self._kind}_solve_traced")(
        self._h, C.byref(batch_struct), C.byref(vb), out.ctypes.data, rec.ctypes.data, capacity,
        C.byref(count))
    _check(self._lib, rc)
    return out, rec[:min(count.value, capacity)].copy()


def _debug_newton(self, batch_struct, names, lens, data, z, l, v, zb, lb, vb):
    """fbstab_hip_*_debug_newton behind ``debug_newton``: ONE QP, whatever shape its numpy arrays have."""
    lib = self._lib
    fn = getattr(lib, f"fbstab_hip_{self._kind}_debug_newton")
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    row = lambda a: np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(1, -1))
    nz, nl, nv = self.nz, self.nl, self.nv
    rows = {k: row(data[k]) for k, n in zip(names, lens) if n > 0}
    _fill_block(batch_struct, names, lens, rows, 1, [])
    xs = (row(z), row(l), row(v), np.zeros((1, nv)))
    vb_ = _fill_vars(xs, (nz, nl, nv, nv), 1, [])
    io = np.zeros(3 * nz + 3 * nl + 2 * nv + 1)
    io[:nz + nl + nv] = np.concatenate([np.ravel(zb), np.ravel(lb), np.ravel(vb)])
    _check(lib, fn(self._h, C.byref(batch_struct), C.byref(vb_), io.ctypes.data))
    out, o = {}, 0
    for n, sz in zip(("dz", "dl", "dv", "adz", "wz", "wl", "rz", "rl"), (nz, nl, nv, nv, nz, nl, nz, nl)):
        out[n] = io[o:o + sz].copy()
        o += sz
    out["ok"] = bool(io[o] > 0.5)
    return out


def out_to_numpy(out) -> np.ndarray:
    """SolverOut records (numpy structured array) from a solve's ``out``."""
    if _is_torch(out):
        return np.frombuffer(out.cpu().numpy().tobytes(), dtype=OUT_DTYPE).copy()
    return out


class FBstabMpcBatch(_SolverBase):
    """Batched counterpart of ``fbstab::FBstabMpc`` (fbstab/fbstab_mpc.h:56-243):
    ``FBstabMpcBatch(N, nx, nu, nc, max_batch)`` allocates the device workspace
    (the reference constructor allocates the CPU workspace, fbstab_mpc.cc:61-89)
    and ``Solve`` solves a batch in the reference data layout."""
    _kind = "mpc"

    def __init__(self, N: int, nx: int, nu: int, nc: int, max_batch: int = 1,
                 device: int = 0, handles_in_flight: int = 1):
        """handles_in_flight: how many such solvers the caller keeps busy on the device at the same time
        (fbstab_hip_mpc_create_in_flight: each then takes its share of the resident workgroups).  The share
        counts the launches that can really overlap, min(handles_in_flight, hardware queues of the process):
        ceil(2 x resident / that) workgroups per CU, at most half the grid for handles_in_flight >= 2 - on the
        BASELINE shape one per CU for eight in flight on eight queues, two per CU (0.87 GB of scratch per
        handle) on HIP's default of four queues or for four in flight.  The queue count is GPU_MAX_HW_QUEUES as
        the environment holds it when the handle is created (read only; unset = 4); FBSTAB_HIP_WGS_PER_CU
        forces a share.  ``query()`` reports the workgroups and scratch bytes the handle got."""
        super().__init__()
        if hasattr(self._lib, "fbstab_hip_mpc_create_in_flight"):
            _check(self._lib, self._lib.fbstab_hip_mpc_create_in_flight(
                N, nx, nu, nc, max_batch, device, handles_in_flight, C.byref(self._h)))
        else:  # (a build of an earlier round, loaded for an A/B)
            _check(self._lib, self._lib.fbstab_hip_mpc_create(N, nx, nu, nc, max_batch, device, C.byref(self._h)))
        self.N, self.nx, self.nu, self.nc = N, nx, nu, nc
        self.max_batch = max_batch
        self.nz, self.nl, self.nv = (N + 1) * (nx + nu), (N + 1) * nx, (N + 1) * nc
        self.seq_len = [(N + 1) * nx * nx, (N + 1) * nu * nu, (N + 1) * nu * nx,
                        (N + 1) * nx, (N + 1) * nu, N * nx * nx, N * nx * nu, N * nx,
                        (N + 1) * nc * nx, (N + 1) * nc * nu, (N + 1) * nc, nx]

    def kernel_name(self) -> str:
        return self._lib.fbstab_hip_mpc_kernel_name(self._h).decode()

    def adjoint_kernel_name(self) -> str:
        """The kernel the next Adjoint call launches (fbstab_hip_mpc_adjoint_kernel_name)."""
        if not hasattr(self._lib, "fbstab_hip_mpc_adjoint_kernel_name"):
            # (an earlier build loaded for an A/B: its one-row record instances ran their own adjoint, every other
            # handle the flat-vector one)
            kn = self.kernel_name()
            return kn.replace("r16_kernel", "r16_adjoint_kernel") if kn.startswith("fbstab_mpc_r16_kernel<12,4,") \
                else "fbstab_mpc_adjoint_kernel<64>"
        return self._lib.fbstab_hip_mpc_adjoint_kernel_name(self._h).decode()

    def refined_steps(self) -> int:
        """Newton steps of the last call that were refined (fbstab_hip_mpc_refined_steps)."""
        n = C.c_longlong(-1)
        _check(self._lib, self._lib.fbstab_hip_mpc_refined_steps(self._h, C.byref(n)))
        return int(n.value)

    def queue_order(self) -> np.ndarray:
        """The order in which the next batch solve of the same size hands out its queue tickets: the QP indices
        of the last packed batch solve by descending Newton count (fbstab_hip_mpc_queue_order); empty where the
        handle holds none."""
        order = np.zeros(self.max_batch, dtype=np.int32)
        n = C.c_int(0)
        _check(self._lib, self._lib.fbstab_hip_mpc_queue_order(self._h, order.ctypes.data, order.size, C.byref(n)))
        return order[:n.value].copy()

    def Solve(self, data: Dict[str, object], z, l, v, y, out=None, stream: int = 0,
              async_: bool = False, keep_matrices: bool = False):
        """``data``: dict of the 12 sequences, each ``(batch, len)`` float64
        (all numpy, or all torch CUDA tensors); ``z,l,v``: initial guess,
        overwritten with the solution, ``y`` overwritten (fbstab_mpc.h:181-195).
        ``keep_matrices``: FBSTAB_HIP_KEEP_MATRICES (receding horizon: only
        q, r, c, d, x0 and the guess changed since the previous flagged call)."""
        return self._solve(_MpcBatch(), MPC_SEQ, self.seq_len, data,
                           (self.nz, self.nl, self.nv, self.nv), z, l, v, y, out,
                           stream, async_, keep_matrices)

    def SolveFinal(self, data, z, l, v, y, out=None, stream: int = 0, async_: bool = False):
        """Solve followed by the numbers of the reference's Display::FINAL summary
        (fbstab_hip_mpc_solve_batch_final): returns ``(out, norms)``, norms ``(batch, 4)``
        = |rz|, |rl|, |rv|, tolerance at the returned point."""
        return self._solve(_MpcBatch(), MPC_SEQ, self.seq_len, data,
                           (self.nz, self.nl, self.nv, self.nv), z, l, v, y, out, stream, async_, norms=True)

    def SolveTraced(self, data, z, l, v, y, capacity: int = 4096):
        """One QP (``(1, n)`` numpy arrays) with the reference's per-iteration
        display returned as records (fbstab_hip_mpc_solve_traced)."""
        return _solve_traced(self, _MpcBatch(), MPC_SEQ, self.seq_len, data,
                             (self.nz, self.nl, self.nv, self.nv), z, l, v, y, capacity)

    def sweep_adjoint_kernel_name(self) -> str:
        """What the next RecedingSweepAdjoint call launches (fbstab_hip_mpc_sweep_adjoint_kernel_name)."""
        return self._lib.fbstab_hip_mpc_sweep_adjoint_kernel_name(self._h).decode()

    @staticmethod
    def _plant(A, B, dev):
        """(struct, tensors to keep alive): the column-major images of one plant shared by all trajectories, from
        ``(nx, nx)`` / ``(nx, nu)`` row-major numpy arrays or torch tensors."""
        import torch
        img = lambda M: (M.detach().to(dev, torch.float64).t() if _is_torch(M)
                         else torch.from_numpy(np.ascontiguousarray(np.asarray(M, dtype=np.float64))).to(dev).t()
                         ).contiguous().reshape(-1)
        Ad, Bd = img(A), img(B)
        return _Plant(Ad.data_ptr(), Bd.data_ptr(), 0, 0), (Ad, Bd)

    def RecedingSweep(self, data, z, l, v, y, A, B, steps: int, retire: bool = True,
                      log_inputs: bool = False, stream: int = 0, log: bool = False, w=None, shift: bool = False):
        """fbstab_hip_mpc_receding_sweep: ``steps`` warm-started closed-loop steps on
        the device (torch CUDA tensors; ``data["x0"]`` is advanced in place, ``z, l,
        v, y`` hold the last solution).  ``A``/``B``: the simulation model as
        ``(nx, nx)``/``(nx, nu)`` numpy arrays shared by all trajectories.  Returns
        ``dict(out, stats, kernel_ms[, u])`` with ``stats`` a structured array per
        step (newton_sum, success, retired_total, newton_max).  ``log=True``
        (fbstab_hip_mpc_receding_sweep_logged) adds what RecedingSweepAdjoint needs, per step: ``z_log, l_log,
        v_log`` ``(steps, batch, n)`` - the point the step returned -, ``x_log`` ``(steps, batch, nx)`` - the state
        it was solved for - and ``eflag_log`` ``(steps, batch)`` int32, -1 once a trajectory is retired.
        ``w``: ``(steps, batch, nx)`` float64 CUDA tensor of disturbances, x_(k+1) = A x_k + B u_k + w_k (a parked
        trajectory stays at the origin); ``shift=True``: the point a step returned is moved one stage towards the
        present before it is the next step's guess (stage N keeps its values; not behind the last step) - fewer
        Newton steps on time-invariant horizons, MORE on random time-varying ones (include/fbstab_hip.h).  Either
        one makes the call fbstab_hip_mpc_receding_sweep_scenario; with neither it is exactly the call above."""
        b, dev_flags = _MpcBatch(), []
        B_ = _fill_block(b, MPC_SEQ, self.seq_len, data, None, dev_flags, shared=False)
        vb = _fill_vars((z, l, v, y), (self.nz, self.nl, self.nv, self.nv), B_, dev_flags)
        assert all(dev_flags), "device tensors only"
        where, _, stream = _placement(dev_flags, z, stream)
        dev = z.device
        plant, plant_keep = self._plant(A, B, dev)   # column-major images
        out = where.out(z, B_)
        stats = np.zeros((steps, 4), dtype=np.uint64)
        kms = np.zeros(steps, dtype=np.float32)
        u = where.zeros(z, (steps, B_, self.nu)) if log_inputs else None
        args = [self._h, B_, C.byref(b), C.byref(vb), out.data_ptr(), C.byref(plant), steps, 1 if retire else 0,
                u.data_ptr() if u is not None else None, stats.ctypes.data, kms.ctypes.data,
                C.c_void_p(stream) if stream else None]
        logs = {}
        lg = None
        if log:
            for k, n in (("z_log", self.nz), ("l_log", self.nl), ("v_log", self.nv), ("x_log", self.nx)):
                logs[k] = where.zeros(z, (steps, B_, n))
            logs["eflag_log"] = where.zeros(z, (steps, B_), "i4")
            lg = _SweepLog(*[logs[k].data_ptr() for k in ("z_log", "l_log", "v_log", "x_log", "eflag_log")])
        if w is not None or shift:
            import torch
            if w is not None:
                assert _is_torch(w) and w.is_cuda and w.dtype == torch.float64 and \
                    tuple(w.shape) == (steps, B_, self.nx), "w: a (steps, batch, nx) float64 CUDA tensor"
                w = w.detach().contiguous()
            sc = _SweepScenario(w.data_ptr() if w is not None else None, 1 if shift else 0)
            _check(self._lib, self._lib.fbstab_hip_mpc_receding_sweep_scenario(
                *args, C.byref(lg) if lg is not None else None, C.byref(sc)))
        elif log:
            _check(self._lib, self._lib.fbstab_hip_mpc_receding_sweep_logged(*args, C.byref(lg)))
        else:
            _check(self._lib, self._lib.fbstab_hip_mpc_receding_sweep(*args))
        st = np.zeros(steps, dtype=[("newton_sum", np.int64), ("success", np.int64),
                                    ("retired_total", np.int64), ("newton_max", np.int64)])
        for j, n in enumerate(st.dtype.names):
            st[n] = stats[:, j].astype(np.int64)
        r = dict(out=out, stats=st, kernel_ms=kms)
        if u is not None:
            r["u"] = u
        r.update(logs)
        return r

    def RecedingSweepAdjoint(self, data, A, B, steps: int, log, gu=None, gx=None, retire: bool = True,
                             sigma: float = 0.0, want: Optional[Sequence[str]] = None, mu: bool = False,
                             stream: int = 0) -> Dict[str, object]:
        """Reverse mode through a logged sweep (fbstab_hip_mpc_receding_sweep_adjoint): ``log`` is what
        ``RecedingSweep(..., log=True)`` returned (its ``z_log, l_log, v_log, eflag_log``), ``gu`` ``(steps, batch,
        nu)`` = dL/du_k and ``gx`` ``(steps, batch, nx)`` = dL/dx_(k+1) the seeds (None: zero), ``A``/``B`` the plant
        as in ``RecedingSweep`` (numpy or torch).  Torch CUDA tensors only.  Returns a dict with dL/d(sequence),
        ``(batch, len)``, for every name of ``want`` (default: all 12 of MPC_SEQ; ``"x0"`` is dL/dx_0 of the
        trajectory, every other one the sum over the steps), ``"status"`` (``(batch,)`` int32: steps whose
        factorisation failed) and, with ``mu=True``, ``"mu"`` ``(steps, batch, nx)``: the costates from which the
        plant's own gradients follow, ``A_bar = einsum("kbi,kbj->ij", mu, x_log)`` and ``B_bar`` likewise with u.
        ``data["x0"]`` is not read."""
        import torch
        want = tuple(MPC_SEQ if want is None else want)
        assert not set(want) - set(MPC_SEQ), want
        zl = log["z_log"]
        dev, B_ = zl.device, zl.shape[1]
        assert zl.is_cuda and zl.shape == (steps, B_, self.nz), "the log of RecedingSweep(..., log=True) on the device"
        b, dev_flags = _MpcBatch(), []
        # (the x0 slot stays NULL: it is not read)
        _fill_block(b, MPC_SEQ[:-1], self.seq_len[:-1], data, B_, dev_flags)
        assert all(dev_flags), "device tensors only"
        where, _, stream = _placement(dev_flags, zl, stream)
        keep = []

        def arr(a, shape, dt):
            if a is None:
                return None
            assert a.is_cuda and a.dtype == dt and tuple(a.shape) == shape, (tuple(a.shape), shape)
            a = a.contiguous()
            keep.append(a)
            return a.data_ptr()

        lg = _SweepLog(arr(log["z_log"], (steps, B_, self.nz), torch.float64),
                       arr(log["l_log"], (steps, B_, self.nl), torch.float64),
                       arr(log["v_log"], (steps, B_, self.nv), torch.float64), None,
                       arr(log["eflag_log"], (steps, B_), torch.int32))
        plant, plant_keep = self._plant(A, B, dev)
        res = {k: where.zeros(zl, (B_, n)) for k, n in zip(MPC_SEQ, self.seq_len) if k in want}
        g = _MpcGradBatch()
        _fill_block(g, MPC_SEQ, self.seq_len, res, B_, [], optional=True, shared=False)
        status = where.zeros(zl, B_, "i4")
        mu_log = where.zeros(zl, (steps, B_, self.nx)) if mu else None
        _check(self._lib, self._lib.fbstab_hip_mpc_receding_sweep_adjoint(
            self._h, B_, C.byref(b), C.byref(plant), steps, 1 if retire else 0, C.byref(lg),
            arr(gu, (steps, B_, self.nu), torch.float64), arr(gx, (steps, B_, self.nx), torch.float64),
            C.c_double(sigma), C.byref(g), mu_log.data_ptr() if mu else None, status.data_ptr(),
            C.c_void_p(stream) if stream else None))
        del plant_keep
        res["status"] = status
        if mu:
            res["mu"] = mu_log
        return res


    def debug_newton(self, data, z, l, v, zb, lb, vb):
        """Tests only: one Newton step of the device path at (x, xbar,
        sigma0, alpha of the current options) for ONE QP (numpy arrays).
        Returns dict(dz, dl, dv, adz, wz, wl, rz, rl, ok)."""
        return _debug_newton(self, _MpcBatch(), MPC_SEQ, self.seq_len, data, z, l, v, zb, lb, vb)

    def Adjoint(self, data: Dict[str, object], z, l, v, gz, gl=None, gv=None, sigma: float = 0.0,
                want: Optional[Sequence[str]] = None, adj: bool = False, stream: int = 0,
                async_: bool = False, reduce: Sequence[str] = (), out=None) -> Dict[str, object]:
        """Reverse-mode derivative of the solution map (fbstab_hip_mpc_adjoint_batch): for a loss L with
        seeds ``gz, gl, gv`` = dL/d(z, l, v) at the returned point ``(z, l, v)`` (``(batch, n)`` arrays, all numpy
        or all torch CUDA tensors, like ``Solve``), returns a dict with dL/d(sequence) for every name of ``want``
        (default: all 12 of MPC_SEQ, each ``(batch, len)``), ``"status"`` (``(batch,)`` int32: 0, or 1 where
        the factorisation failed and the gradients are zero) and, with ``adj=True``, ``"dz", "dl", "dv"``.
        ``gl``/``gv`` None: zero seeds.  ``sigma <= 0``: 1e-8.
        ``reduce``: names whose gradient comes back as ONE ``(1, len)`` array, the sum over the batch (for data
        shared by the batch; fbstab_hip_mpc_adjoint_batch_reduced), leaving out QPs whose status is 1 and, with
        ``out`` (the records ``Solve`` returned), QPs whose solve did not end in SUCCESS.  A ``(1, len)`` array in
        ``data`` beside a batch of more than one QP is shared by all of them."""
        return self._adjoint(self._lib.fbstab_hip_mpc_adjoint_batch, _MpcBatch(), _MpcGradBatch(), MPC_SEQ,
                             self.seq_len, data, z, l, v, gz, gl, gv, sigma, want, adj, stream, async_, reduce, out)

    def Tangent(self, data: Dict[str, object], z, l, v, ddata: Dict[str, object], sigma: float = 0.0,
                rhs: bool = False, stream: int = 0, async_: bool = False) -> Dict[str, object]:
        """Forward-mode derivative of the solution map (fbstab_hip_mpc_tangent_batch): the first-order change
        ``dz, dl, dv`` (``(batch, n)``) of the solutions at the returned point ``(z, l, v)`` for the perturbation
        ``ddata`` of the problem data: a dict name -> ``(batch, len)`` direction, or ``(1, len)`` for one direction
        shared by the batch; absent names and None are zero perturbations.  dQ and dR enter through their symmetric
        part.  All numpy or all torch CUDA tensors, like ``Adjoint``.  Returns a dict with ``"dz", "dl", "dv"``,
        ``"status"`` (``(batch,)`` int32: 1 where the factorisation failed and the tangent is zero) and, with
        ``rhs=True``, the seeds ``"gz", "gl", "gv"`` of the tangent system.  ``sigma <= 0``: 1e-8."""
        return _tangent(self, _MpcBatch(), _MpcBatch(), MPC_SEQ, self.seq_len, data, z, l, v, ddata, sigma, rhs,
                        stream, async_)

    def KktSolve(self, data: Dict[str, object], z, l, v, gz, gl=None, gv=None, sigma: float = 0.0, stream: int = 0,
                 async_: bool = False) -> Dict[str, object]:
        """Several right-hand sides on ONE factorisation per QP (fbstab_hip_mpc_kkt_solve_batch): ``gz`` of shape
        ``(batch, K, nz)``, or ``(K, nz)`` for one block of K seeds shared by the batch; ``gl``, ``gv`` the same
        (None: zero).  Returns a dict with ``dz (batch, K, nz)``, ``dl``, ``dv`` - slot k what ``Adjoint(...,
        adj=True)`` returns for seed k - and ``status`` (``(batch,)`` int32: 1 where the factorisation failed and
        every right-hand side's step is zero).  All numpy or all torch CUDA tensors, like ``Adjoint``.
        ``sigma <= 0``: 1e-8."""
        assert len(gz.shape) in (2, 3), gz.shape
        return _multi_call(self, _MpcBatch(), MPC_SEQ, self.seq_len, self._lib.fbstab_hip_mpc_kkt_solve_batch, data,
                           z, l, v, gz.shape[-2], (gz, gl, gv), (), sigma, ("dz", "dl", "dv"), None, stream, async_)

    def X0Sensitivity(self, data: Dict[str, object], z, l, v, sigma: float = 0.0,
                      want: Sequence[str] = ("dz", "gain"), stream: int = 0, async_: bool = False) -> Dict[str, object]:
        """The solutions' sensitivity to the initial state on ONE factorisation per QP
        (fbstab_hip_mpc_x0_sensitivity_batch): those of ``want`` among ``dz (batch, nx, nz)``, ``dl``, ``dv`` - row j
        what ``Tangent`` returns for the direction x0 = e_j - and ``gain (batch, nu, nx)`` = du0/dx0, the local
        feedback law, plus ``status``.  All numpy or all torch CUDA tensors, like ``Adjoint``."""
        unknown = set(want) - {"dz", "dl", "dv", "gain"}
        assert not unknown, unknown
        return _multi_call(self, _MpcBatch(), MPC_SEQ, self.seq_len, self._lib.fbstab_hip_mpc_x0_sensitivity_batch,
                           data, z, l, v, self.nx, None, (), sigma, want, (self.nx, self.nu), stream, async_)


class FBstabDenseBatch(_SolverBase):
    """Batched counterpart of ``fbstab::FBstabDense`` (fbstab/fbstab_dense.h:50-194)."""
    _kind = "dense"

    def __init__(self, nz: int, nl: int, nv: int, max_batch: int = 1, device: int = 0):
        super().__init__()
        _check(self._lib, self._lib.fbstab_hip_dense_create(
            nz, nl, nv, max_batch, device, C.byref(self._h)))
        self.nz, self.nl, self.nv = nz, nl, nv
        self.arr_len = [nz * nz, nz, nl * nz, nl, nv * nz, nv]

    def Solve(self, data: Dict[str, object], z, l, v, y, out=None, stream: int = 0,
              async_: bool = False):
        return self._solve(_DenseBatch(), DENSE_ARR, self.arr_len, data,
                           (self.nz, self.nl, self.nv, self.nv), z, l, v, y, out,
                           stream, async_)

    ORDER_AUTO, ORDER_PIVOTED, ORDER_NATURAL = 0, 1, 2

    def SetFactorisation(self, order: int = 0, spread_bits: int = 0):
        """fbstab_hip_dense_set_factorisation: elimination order of the LDL' of the KKT
        matrix (dense_cholesky_solver.cc:70-79); ``spread_bits`` 0 keeps the current value."""
        _check(self._lib, self._lib.fbstab_hip_dense_set_factorisation(self._h, order, spread_bits))

    def Factorisation(self) -> Dict[str, int]:
        """Settings in force and the number of Newton steps of the last batch that went to
        the pivoted factorisation behind a natural-order attempt (-1: does not apply)."""
        o, b, n = C.c_int(), C.c_int(), C.c_longlong()
        _check(self._lib, self._lib.fbstab_hip_dense_get_factorisation(
            self._h, C.byref(o), C.byref(b), C.byref(n)))
        return dict(order=o.value, spread_bits=b.value, pivoted_steps=n.value)

    def SolveFinal(self, data, z, l, v, y, out=None, stream: int = 0, async_: bool = False):
        """As FBstabMpcBatch.SolveFinal (fbstab_hip_dense_solve_batch_final)."""
        return self._solve(_DenseBatch(), DENSE_ARR, self.arr_len, data,
                           (self.nz, self.nl, self.nv, self.nv), z, l, v, y, out, stream, async_, norms=True)

    def debug_newton(self, data, z, l, v, zb, lb, vb):
        """Tests only: one Newton step of the dense device path at (x, xbar, sigma0,
        alpha of the current options) for ONE QP (numpy arrays).  Returns
        dict(dz, dl, dv, adz, wz, wl, rz, rl, ok)."""
        return _debug_newton(self, _DenseBatch(), DENSE_ARR, self.arr_len, data, z, l, v, zb, lb, vb)

    def SolveTraced(self, data, z, l, v, y, capacity: int = 4096):
        """One QP (``(1, n)`` numpy arrays) with the reference's per-iteration
        display returned as records (fbstab_hip_dense_solve_traced)."""
        return _solve_traced(self, _DenseBatch(), DENSE_ARR, self.arr_len, data,
                             (self.nz, self.nl, self.nv, self.nv), z, l, v, y, capacity)

    def Adjoint(self, data: Dict[str, object], z, l, v, gz, gl=None, gv=None, sigma: float = 0.0,
                want: Optional[Sequence[str]] = None, adj: bool = False, stream: int = 0,
                async_: bool = False, reduce: Sequence[str] = (), out=None) -> Dict[str, object]:
        """Reverse-mode derivative of the dense solution map (fbstab_hip_dense_adjoint_batch): for a loss L with
        seeds ``gz, gl, gv`` = dL/d(z, l, v) at the returned point ``(z, l, v)`` (``(batch, n)`` arrays, all numpy
        or all torch CUDA tensors, like ``Solve``), returns a dict with dL/d(array) for every name of ``want``
        (default: all six of DENSE_ARR, each ``(batch, len)``, the matrices column-major like the inputs),
        ``"status"`` (``(batch,)`` int32: 0, or 1 where the factorisation failed and the gradients are zero) and,
        with ``adj=True``, ``"dz", "dl", "dv"``.  ``gl``/``gv`` None: zero seeds.  ``sigma <= 0``: 1e-8.  With
        ``nl == 0`` the G, h and l arrays are ``(batch, 0)`` (or None on input).  ``reduce``, ``out`` and shared
        ``(1, len)`` inputs: as FBstabMpcBatch.Adjoint (fbstab_hip_dense_adjoint_batch_reduced)."""
        return self._adjoint(self._lib.fbstab_hip_dense_adjoint_batch, _DenseBatch(), _DenseGradBatch(), DENSE_ARR,
                             self.arr_len, data, z, l, v, gz, gl, gv, sigma, want, adj, stream, async_, reduce, out)

    def Tangent(self, data: Dict[str, object], z, l, v, ddata: Dict[str, object], sigma: float = 0.0,
                rhs: bool = False, stream: int = 0, async_: bool = False) -> Dict[str, object]:
        """Forward-mode derivative of the dense solution map (fbstab_hip_dense_tangent_batch): as
        FBstabMpcBatch.Tangent, ``ddata`` naming directions of H, f, G, h, A, b (the matrices column-major like the
        inputs, dH through its symmetric part).  With ``nl == 0`` the G, h and l arrays are ``(batch, 0)``."""
        return _tangent(self, _DenseBatch(), _DenseBatch(), DENSE_ARR, self.arr_len, data, z, l, v, ddata, sigma,
                        rhs, stream, async_)

    WRT = {"f": DENSE_ARR.index("f"), "h": DENSE_ARR.index("h"), "b": DENSE_ARR.index("b")}   # FBSTAB_DENSE_f, _h, _b

    def KktSolve(self, data: Dict[str, object], z, l, v, gz, gl=None, gv=None, sigma: float = 0.0, stream: int = 0,
                 async_: bool = False) -> Dict[str, object]:
        """Several right-hand sides on ONE factorisation per QP (fbstab_hip_dense_kkt_solve_batch): ``gz`` of shape
        ``(batch, K, nz)``, or ``(K, nz)`` for one block of K seeds shared by the batch; ``gl``, ``gv`` the same
        (None: zero).  Returns a dict with ``dz (batch, K, nz)``, ``dl``, ``dv`` - slot k the step ``Adjoint(...,
        adj=True)`` solves for seed k - and ``status`` (``(batch,)`` int32: 1 where the factorisation failed and
        every right-hand side's step is zero).  All numpy or all torch CUDA tensors, like ``Adjoint``.
        ``sigma <= 0``: 1e-8.  With ``nl == 0`` ``gl`` is None or ``(batch, K, 0)``."""
        assert len(gz.shape) in (2, 3), gz.shape
        return _multi_call(self, _DenseBatch(), DENSE_ARR, self.arr_len, self._lib.fbstab_hip_dense_kkt_solve_batch,
                           data, z, l, v, gz.shape[-2], (gz, gl, gv), (), sigma, ("dz", "dl", "dv"), None, stream,
                           async_)

    def Jacobian(self, data: Dict[str, object], z, l, v, wrt: str = "b", want: Sequence[str] = ("dz",),
                 sigma: float = 0.0, stream: int = 0, async_: bool = False) -> Dict[str, object]:
        """The solutions' sensitivity to one of the arrays ``f``, ``h``, ``b`` on ONE factorisation per QP
        (fbstab_hip_dense_jacobian_batch): those of ``want`` among ``dz (batch, nrhs, nz)``, ``dl``, ``dv`` with
        nrhs the array's length - row k what ``Tangent`` returns for the perturbation e_k of ``wrt`` - plus
        ``status``.  The slots not in ``want`` are neither allocated nor written: ``want=("dz",)`` with ``wrt="b"``
        is dz/db alone.  All numpy or all torch CUDA tensors, like ``Adjoint``."""
        unknown = set(want) - {"dz", "dl", "dv"}
        assert not unknown and len(want) > 0, want
        assert wrt in self.WRT, wrt
        K = {"f": self.nz, "h": self.nl, "b": self.nv}[wrt]
        return _multi_call(self, _DenseBatch(), DENSE_ARR, self.arr_len, self._lib.fbstab_hip_dense_jacobian_batch,
                           data, z, l, v, K, None, (self.WRT[wrt],), sigma, want, None, stream, async_)


class ShardGroup:
    """fbstab_hip_shard_group_*: the GPUs of one node driven by ONE process; shard d of a
    batch lives on ``devices[d]`` and is solved by ``solvers[d]`` (a solver created on
    that device); the results are gathered to ``devices[root]`` in one RCCL operation
    (fbstab_hip_*_solve_batch_sharded).  Arrays are torch CUDA tensors."""

    def __init__(self, devices: Sequence[int]):
        self._lib = load_library()
        self._g = C.c_void_p()
        self.devices = list(devices)
        arr = (C.c_int * len(self.devices))(*self.devices)
        _check(self._lib, self._lib.fbstab_hip_shard_group_create(len(self.devices), arr, C.byref(self._g)))

    def close(self):
        if getattr(self, "_g", None) and self._g.value:
            self._lib.fbstab_hip_shard_group_destroy(self._g)
            self._g = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def stats(self) -> Dict[str, int]:
        a, b = C.c_longlong(), C.c_longlong()
        _check(self._lib, self._lib.fbstab_hip_shard_group_stats(self._g, C.byref(a), C.byref(b)))
        return dict(gathers=a.value, rccl_ops=b.value)

    def _shards(self, solvers, names, lens, data, xs, outs):
        n = len(self.devices)
        assert len(solvers) == len(data) == len(xs) == len(outs) == n
        kind = solvers[0]._kind
        bs = ((_MpcBatch if kind == "mpc" else _DenseBatch) * n)()
        vs = (_VarBatch * n)()
        counts = (C.c_int * n)()
        hs = (C.c_void_p * n)(*[s._h.value for s in solvers])
        op = (C.c_void_p * n)()
        var_lens = (solvers[0].nz, solvers[0].nl, solvers[0].nv, solvers[0].nv)
        for d in range(n):
            dev_flags = []
            counts[d] = _fill_block(bs[d], names, lens, data[d], None, dev_flags, shared=False)
            _fill_vars(xs[d], var_lens, counts[d], dev_flags, vb=vs[d])
            assert all(dev_flags)
            op[d] = outs[d].data_ptr()
        return kind, bs, vs, counts, hs, op, var_lens

    def Solve(self, solvers, data, xs, outs, root: int, root_x, root_out):
        """``data[d]``: dict of shard d's arrays, ``xs[d] = (z, l, v, y)``, ``outs[d]``: ``(B_d, 40)``
        uint8, all on ``devices[d]``; ``root_x = (z, l, v, y)`` and ``root_out`` hold the whole batch
        on ``devices[root]``."""
        names, lens = (MPC_SEQ, solvers[0].seq_len) if solvers[0]._kind == "mpc" else (DENSE_ARR, solvers[0].arr_len)
        kind, bs, vs, counts, hs, op, var_lens = self._shards(solvers, names, lens, data, xs, outs)
        dev_flags = []
        rv = _fill_vars(root_x, var_lens, None, dev_flags)
        assert all(dev_flags)
        _check(self._lib, getattr(self._lib, f"fbstab_hip_{kind}_solve_batch_sharded")(
            self._g, hs, counts, bs, vs, op, root, C.byref(rv), C.c_void_p(root_out.data_ptr())))

    def RecedingSweep(self, solvers, data, xs, outs, A, B, steps: int, retire: bool, u_logs, root: int, root_u_log):
        """fbstab_hip_mpc_receding_sweep_sharded; ``A``/``B``: one plant (numpy) for all trajectories;
        ``u_logs[d]``: ``(steps, B_d, nu)`` on devices[d]; ``root_u_log``: the shards' logs one after the
        other on devices[root].  Returns the per-step statistics summed over the shards."""
        import torch
        kind, bs, vs, counts, hs, op, _ = self._shards(solvers, MPC_SEQ, solvers[0].seq_len, data, xs, outs)
        n = len(self.devices)
        plants = (_Plant * n)()
        keep = []
        for d in range(n):
            dev = xs[d][0].device
            Ad = torch.from_numpy(np.asfortranarray(np.asarray(A, dtype=np.float64)).T.copy().reshape(-1)).to(dev)
            Bd = torch.from_numpy(np.asfortranarray(np.asarray(B, dtype=np.float64)).T.copy().reshape(-1)).to(dev)
            keep += [Ad, Bd]
            plants[d] = _Plant(Ad.data_ptr(), Bd.data_ptr(), 0, 0)
        ul = (C.c_void_p * n)(*[u.data_ptr() for u in u_logs])
        stats = np.zeros((steps, 4), dtype=np.uint64)
        _check(self._lib, self._lib.fbstab_hip_mpc_receding_sweep_sharded(
            self._g, hs, counts, bs, vs, op, plants, steps, 1 if retire else 0, ul, root,
            C.c_void_p(root_u_log.data_ptr()), stats.ctypes.data))
        return stats

