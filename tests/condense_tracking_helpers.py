"""TEST INFRASTRUCTURE ONLY: what tests/test_condense_tracking_cpu.py and tests/test_gpu_condense_tracking.py share -
the per-step references q_k, r_k, c_k, d_k of the closed-loop set-ups of tests/condense_sweep_helpers.py, the problem
of a step, the reference closed loop on them (a ReferenceCondenser per step), and the host build of
fbstab_amd/csrc/fb_condense_refs.h (tests/hostsim/condense_refs.cc)."""
import ctypes as C
import functools

import numpy as np

from tests import condense_helpers as ch
from tests import condense_sweep_helpers as sh
from tests import hostsim
from tools import fixtures as fx

LD = ch.LD
STEPS = sh.STEPS          # forward
ADJOINT_STEPS = 6         # reverse: the first six steps of the same references
REF_NAMES = ("q", "r", "c", "d")
LOOP_FIXTURES = ("double_integrator", "small", "four_wave", "tiny")
# which trajectory retires at which step on these references (unshifted and shifted alike), by the oracle
RETIRES = {"tiny": {1: 4}, "small": {2: 4, 4: 4}, "four_wave": {}, "double_integrator": {2: 0}}


@functools.lru_cache(maxsize=None)
def references(name):
    """name -> ``(STEPS, batch, len)`` for q, r, c, d of ``sh.setup(name)``: q and r move by a tenth of their size,
    c by a hundredth, and d only loosens the constraints (d_k = d - 0.05 |g|).  Built once; the tests leave them
    unchanged."""
    p = sh.setup(name)[0]
    rng = np.random.default_rng(31)
    ref = {}
    for k in REF_NAMES:                                  # (drawn in this order)
        a = p.arrays[k]
        g = rng.standard_normal((STEPS,) + a.shape)
        if k in ("q", "r"):
            ref[k] = a + 0.1 * g * (1 + np.abs(a))
        elif k == "c":
            ref[k] = a + 0.01 * g * (1 + np.abs(a))
        else:
            ref[k] = a - 0.05 * np.abs(g)
        ref[k] = np.ascontiguousarray(ref[k])
    return ref


def with_arrays(p, **arrays):
    """``p`` with some arrays replaced; the others are shared, not copied."""
    m = fx.MpcProblem(*p.sizes())
    m.arrays = dict(p.arrays)
    for k, a in arrays.items():
        m.arrays[k] = np.ascontiguousarray(a, dtype=np.float64)
    return m


@functools.lru_cache(maxsize=None)
def problem_at(name, k, names=REF_NAMES):
    """The problem of step ``k``: ``sh.setup(name)``'s with step k of the references ``names``."""
    ref = references(name)
    return with_arrays(sh.setup(name)[0], **{n: ref[n][k] for n in names})


@functools.lru_cache(maxsize=None)
def condenser_at(name, k):
    return sh.ReferenceCondenser(problem_at(name, k))


@functools.lru_cache(maxsize=None)
def oracle_loop(name, shift=False, variant="plain", retire=True, steps=STEPS):
    """sh.oracle_loop on the tracked problem: step k solves the condensed QP of ``problem_at(name, k)``."""
    from oracle.oracle_py import Oracle
    p, A, B, w = sh.setup(name)
    orc = Oracle(fma=(variant == "fma"))
    at = [0]

    def solve(x, U, v):
        k = at[0]
        at[0] += 1
        rc = condenser_at(name, k)
        d = rc.problem(x)
        if variant == "affine":
            aff = rc.affine()
            d.arrays["f"] = np.stack([f0 + F @ x[q] for q, (f0, F, _, _) in enumerate(aff)])
            d.arrays["b"] = np.stack([b0 + G @ x[q] for q, (_, _, b0, G) in enumerate(aff)])
        z, _, vo, _, out = orc.solve_dense(d, x0guess=(U, np.zeros((p.batch, 0)), v), raise_on_error=False)
        return z, vo, out
    return sh.condensed_closed_loop(solve, p, A, B, steps, w=w[:steps], shift=shift, retire=retire)


# ---- the device logic on one host thread -----------------------------------------------------------------------
class HostRefs:
    """condense_reference_vectors of fb_condense_refs.h with Ctx<1> (hostsim/condense_refs.cc), the groups of R
    steps walked as the kernel's grid walks them."""

    def __init__(self):
        self.lib = C.CDLL(hostsim.build("libhostsim_condense_refs.so", "condense_refs.cc",
                                        ("fb_common.h", "fb_batch.h", "fb_condense_plan.h", "fb_condense.h",
                                         "fb_condense_refs.h")))
        self.lib.hostsim_condense_refs.restype = C.c_longlong
        self.lib.hostsim_condense_refs.argtypes = [C.c_int] * 4 + [C.c_void_p] * 3 + [C.c_int, C.c_int, C.c_void_p,
                                                                                    C.c_longlong, C.c_void_p,
                                                                                    C.c_longlong]

    def images(self, p, q, seqs, steps, R, pad=0):
        """(f0 (steps, nzc), b0 (steps, nv)) of trajectory ``q`` of ``p``'s model.  ``seqs``: for q, r, c, d a pair
        (flat float64 array, doubles between steps) - step k reads from ``array[k * step:]``.  ``pad``: doubles
        between two images, which must come back NaN."""
        N, nx, nu, nc = p.sizes()
        nzc, nv = (N + 1) * nu, p.nv
        keep = [np.ascontiguousarray(p.arrays[k][q], dtype=np.float64) for k in ch.MPC_NAMES]
        for i in (3, 4, 7, 10, 11):                       # q, r, c, d and x0 are not read
            keep[i] = None
        data = (C.c_void_p * 12)(*[None if a is None else a.ctypes.data for a in keep])
        arrs = [np.ascontiguousarray(seqs[k][0], dtype=np.float64) for k in REF_NAMES]
        ref = (C.c_void_p * 4)(*[a.ctypes.data for a in arrs])
        step = (C.c_longlong * 4)(*[seqs[k][1] for k in REF_NAMES])
        f0, b0 = np.full((steps, nzc + pad), np.nan), np.full((steps, nv + pad), np.nan)
        lds = self.lib.hostsim_condense_refs(N, nx, nu, nc, data, ref, step, steps, R, f0.ctypes.data, nzc + pad,
                                             b0.ctypes.data, nv + pad)
        assert lds > 0, "the words behind the workgroup's LDS were written"
        assert np.isnan(f0[:, nzc:]).all() and np.isnan(b0[:, nv:]).all()
        self.lds_doubles = lds
        return f0[:, :nzc], b0[:, :nv]


def packed(ref, q, steps):
    """The references of trajectory ``q`` as ``HostRefs.images`` takes them: (steps, len) flat, step = len."""
    return {k: (np.ascontiguousarray(ref[k][:steps, q]).reshape(-1), ref[k].shape[2]) for k in REF_NAMES}
