"""TEST INFRASTRUCTURE ONLY: what tests/test_condense_cpu.py and tests/test_gpu_condense.py share - the fixtures,
the extended-precision reference of the condensing maps, the acceptance rule and the host build of
fbstab_amd/csrc/fb_condense.h (tests/hostsim/condense.cc)."""
import ctypes as C
import functools

import numpy as np

from tests import hostsim
from tests.helpers import mpc_explicit
from tools import fixtures as fx

LD = np.longdouble
MPC_NAMES = ("Q", "R", "S", "q", "r", "A", "B", "c", "E", "L", "d", "x0")
MATRIX_NAMES = ("Q", "R", "S", "A", "B", "E", "L")
BATCH = 5

# (name, (N, nx, nu, nc) or None for the named generators, seed)
SHAPES = (("tiny", (1, 1, 1, 1), 11), ("small", (3, 5, 2, 3), 12), ("odd33", (2, 33, 3, 1), 13),
          ("flat", (6, 30, 3, 5), 14), ("four_wave", (8, 6, 8, 4), 15), ("double_integrator", None, 16),
          ("servo_motor", None, 17))
SHAPE_NAMES = tuple(s[0] for s in SHAPES)


@functools.lru_cache(maxsize=None)
def problem(name):
    """The fixture of that name, a batch of BATCH QPs (built once; the tests leave it unchanged)."""
    _, sizes, seed = next(s for s in SHAPES if s[0] == name)
    rng = np.random.default_rng(seed)
    if sizes is not None:
        p = fx.random_ltv_mpc(rng, BATCH, *sizes)
        # (the seeded defects of test_condense_cpu.py would prove nothing on zero S or c)
        assert np.abs(p.arrays["S"]).max() > 0 and np.abs(p.arrays["c"]).max() > 0
        return p
    g = fx.OcpGenerator()
    getattr(g, {"double_integrator": "DoubleIntegrator", "servo_motor": "ServoMotor"}[name])()
    p = g.GetFBstabInput()
    p.arrays = {k: np.ascontiguousarray(np.repeat(a, BATCH, axis=0)) for k, a in p.arrays.items()}
    # the same model from BATCH initial states (QP 0: the generator's own), near enough to stay feasible
    p.arrays["x0"][1:] += {"double_integrator": 0.05, "servo_motor": 0.005}[name] * rng.standard_normal((BATCH - 1, p.nx))
    return p


# ---- the reference: the elimination of mpc_explicit's matrices in np.longdouble ---------------------------------
def _explicit(p, q, absolute):
    m = [np.asarray(a, dtype=LD) for a in mpc_explicit(p, q)]
    return [np.abs(a) for a in m] if absolute else m


def _rollout(p, G, h, absolute):
    """z = T U + t from G z = h: G's x columns are block bidiagonal with -I on the diagonal, so the rows of stage
    i give x_i by forward substitution (no factorisation).  ``absolute``: every term enters with a plus sign."""
    N, nx, nu, nc = p.sizes()
    ns = nx + nu
    T = np.zeros((p.nz, (N + 1) * nu), dtype=LD)
    t = np.zeros(p.nz, dtype=LD)
    for i in range(N + 1):
        o = i * ns
        T[o + nx:o + ns, i * nu:(i + 1) * nu] = np.eye(nu, dtype=LD)
        rows = slice(i * nx, (i + 1) * nx)
        if i == 0:
            t[:nx] = h[rows] if absolute else -h[rows]
        else:
            Gp = G[rows, o - ns:o]
            T[o:o + nx] = Gp @ T[o - ns:o]
            t[o:o + nx] = Gp @ t[o - ns:o] + (h[rows] if absolute else -h[rows])
    return T, t


def _condense(p, q, absolute):
    H, f, G, h, A, b = _explicit(p, q, absolute)
    T, t = _rollout(p, G, h, absolute)
    At = A @ t
    return dict(H=T.T @ H @ T, f=T.T @ (H @ t + f), A=A @ T, b=(b + At) if absolute else (b - At))


def condense_reference(p, q):
    """H_c (nz_c x nz_c), f_c, A_c (nv x nz_c), b_c of QP ``q`` as 2-D / 1-D longdouble arrays."""
    return _condense(p, q, False)


def rule_factor(p):
    """c 2^-52 with c = 2 (N + 2)(nx + nu + nc + 2): the chain length times the widest inner product, doubled."""
    N, nx, nu, nc = p.sizes()
    return LD(2 * (N + 2) * (nx + nu + nc + 2)) * LD(2.0) ** -52


def condense_bound(p, q):
    """The acceptance rule, componentwise: the same formulas on the entrywise absolute values of all data (minus
    signs made plus) times ``rule_factor`` - a first-order worst-case rounding bound."""
    return {k: a * rule_factor(p) for k, a in _condense(p, q, True).items()}


def _expand(p, q, U, v, y, absolute):
    N, nx, nu, nc = p.sizes()
    ns = nx + nu
    H, f, G, h, A, b = _explicit(p, q, absolute)
    T, t = _rollout(p, G, h, absolute)
    U, v = (np.asarray(a, dtype=LD) for a in (U, v))
    if absolute:
        U, v = np.abs(U), np.abs(v)
    z = T @ U + t
    g = H @ z + f + A.T @ v
    l = np.zeros(p.nl, dtype=LD)
    for i in range(N, -1, -1):
        o = i * ns
        l[i * nx:(i + 1) * nx] = g[o:o + nx]
        if i < N:
            l[i * nx:(i + 1) * nx] += G[(i + 1) * nx:(i + 2) * nx, o:o + nx].T @ l[(i + 1) * nx:(i + 2) * nx]
    return z, l


def expand_reference(p, q, U, v, y):
    """(z, l, v, y) of the MPC QP from the condensed point: states by forward substitution, costates from the x
    rows of Hz + f + G'l + A'v = 0, in longdouble; v and y pass through."""
    z, l = _expand(p, q, U, v, y, False)
    return z, l, np.asarray(v), np.asarray(y)


def expand_bound(p, q, U, v, y):
    """The rule for (z, l): the same formulas on absolute values, times ``rule_factor``."""
    z, l = _expand(p, q, U, v, y, True)
    return z * rule_factor(p), l * rule_factor(p)


def assert_condition(p, q):
    """The rule is applied only where it is not vacuous: max(bound) <= 1e-5 max|reference| for every array."""
    ref, bound = condense_reference(p, q), condense_bound(p, q)
    for k in ref:
        assert bound[k].max() <= 1e-5 * np.abs(ref[k]).max(), (k, float(bound[k].max()), float(np.abs(ref[k]).max()))
    return ref, bound


def images(res, p):
    """The flat column-major images of a result dict as the reference's 2-D / 1-D arrays."""
    nzc, nv = (p.N + 1) * p.nu, p.nv
    return dict(H=np.asarray(res["H"]).reshape(nzc, nzc).T, f=np.asarray(res["f"]).reshape(-1),
                A=np.asarray(res["A"]).reshape(nzc, nv).T, b=np.asarray(res["b"]).reshape(-1))


def rule_violations(got, ref, bound, names=("H", "f", "A", "b")):
    """Names of the arrays of ``got`` (as ``images`` returns them) that miss the rule somewhere."""
    return [k for k in names if not (np.abs(got[k].astype(LD) - ref[k]) <= bound[k]).all()]


def worst_ratio(got, ref, bound, names=("H", "f", "A", "b")):
    """max |got - ref| / bound over the arrays (entries with a zero bound: exact or inf)."""
    w = 0.0
    for k in names:
        err = np.abs(got[k].astype(LD) - ref[k])
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(bound[k] > 0, err / np.where(bound[k] > 0, bound[k], 1), np.where(err > 0, np.inf, 0))
        w = max(w, float(r.max()))
    return w


# ---- the device logic on one host thread -----------------------------------------------------------------------
class HostCondense:
    """condense_matrices / condense_vectors / condense_expand of fb_condense.h with Ctx<1> (hostsim/condense.cc)."""
    MATRICES, VECTORS, ALL = 1, 2, 3

    def __init__(self):
        self.lib = C.CDLL(hostsim.build("libhostsim_condense.so", "condense.cc",
                                        ("fb_common.h", "fb_batch.h", "fb_condense_plan.h", "fb_condense.h")))
        self.lib.hostsim_condense.argtypes = [C.c_int] * 4 + [C.c_void_p, C.c_int] + [C.c_void_p] * 4
        self.lib.hostsim_expand.argtypes = [C.c_int] * 4 + [C.c_void_p] * 8

    @staticmethod
    def _data(p, q):
        keep = [np.ascontiguousarray(p.arrays[k][q], dtype=np.float64) for k in MPC_NAMES]
        return keep, (C.c_void_p * 12)(*[a.ctypes.data for a in keep])

    def condense(self, p, q, what=3):
        """dict H, f, A, b (flat, column-major) of QP ``q``; what ``what`` does not select stays NaN."""
        nzc, nv = (p.N + 1) * p.nu, p.nv
        res = dict(H=np.full(nzc * nzc, np.nan), f=np.full(nzc, np.nan), A=np.full(nv * nzc, np.nan),
                   b=np.full(nv, np.nan))
        keep, data = self._data(p, q)
        self.lib.hostsim_condense(*p.sizes(), data, what, *(res[k].ctypes.data for k in ("H", "f", "A", "b")))
        return res

    def expand(self, p, q, U, v, y):
        keep, data = self._data(p, q)
        U, v, y = (np.ascontiguousarray(a, dtype=np.float64) for a in (U, v, y))
        z, l, vo, yo = (np.full(n, np.nan) for n in (p.nz, p.nl, p.nv, p.nv))
        self.lib.hostsim_expand(*p.sizes(), data, U.ctypes.data, v.ctypes.data, y.ctypes.data, z.ctypes.data,
                                l.ctypes.data, vo.ctypes.data, yo.ctypes.data)
        return z, l, vo, yo


def condensed_problem(p, arrays=None):
    """The dense problem ((N + 1) nu, 0, nv) of every QP of ``p``: from ``arrays`` (dict of (batch, len) images), or
    from the reference rounded to double."""
    nzc = (p.N + 1) * p.nu
    d = fx.DenseProblem(nzc, 0, p.nv)
    if arrays is None:
        refs = [condense_reference(p, q) for q in range(p.batch)]
        arrays = dict(H=np.stack([r["H"].astype(np.float64).T.reshape(-1) for r in refs]),
                      f=np.stack([r["f"].astype(np.float64) for r in refs]),
                      A=np.stack([r["A"].astype(np.float64).T.reshape(-1) for r in refs]),
                      b=np.stack([r["b"].astype(np.float64) for r in refs]))
    d.arrays = dict(H=np.ascontiguousarray(arrays["H"]), f=np.ascontiguousarray(arrays["f"]),
                    G=np.zeros((p.batch, 0)), h=np.zeros((p.batch, 0)), A=np.ascontiguousarray(arrays["A"]),
                    b=np.ascontiguousarray(arrays["b"]))
    return d


def u_of(p, z):
    """The u blocks of z, (batch, (N + 1) nu)."""
    N, nx, nu, nc = p.sizes()
    return np.ascontiguousarray(np.asarray(z).reshape(-1, N + 1, nx + nu)[:, :, nx:].reshape(-1, (N + 1) * nu))
