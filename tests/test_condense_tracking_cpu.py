"""Per-step references on the condensed MPC route without a GPU (fbstab_hip_mpc_condensed_reference_images_batch,
fbstab_hip_mpc_condensed_tracking_sweep, fbstab_hip_mpc_condensed_tracking_sweep_adjoint): the one new device function
(fb_condense_refs.h) compiled for one host thread against the host build of condense_vectors, bit for bit, and against
the extended-precision reference; the host stage (fb_condense_stage.h) under a stand-alone driver with host lambdas in
the kernels' place, plain and under the address and undefined-behaviour sanitizers; the reference closed loop on the
test references; and the argument checks of the C-ABI, which run before any device call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import condense_helpers as ch
from tests import condense_sweep_helpers as sh
from tests import condense_tracking_helpers as th
from tests.test_host_stage import CSRC, HOSTSIM

LD = ch.LD
REF_STEPS = 5          # 5 = 2 * 2 + 1 = 3 + 2: the last group is partial for R = 2 and R = 3
DEVICE_FIXTURES = ("tiny", "small", "odd33", "flat")


@pytest.fixture(scope="module")
def host():
    return th.HostRefs()


@pytest.fixture(scope="module")
def host_vectors():
    return ch.HostCondense()


def _step_problem(name, k, names=th.REF_NAMES):
    """The problem of step k with x0 = 0."""
    p = th.problem_at(name, k, names)
    return th.with_arrays(p, x0=np.zeros_like(p.arrays["x0"]))


# ---- 1. the device function under Ctx<1> -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", DEVICE_FIXTURES)
def test_images_are_bitwise_the_vectors_kernel_at_x0_zero_and_meet_the_rule(host, host_vectors, name):
    p = sh.setup(name)[0]
    ref = th.references(name)
    for q in (0, p.batch - 1):
        want = [host_vectors.condense(_step_problem(name, k), q, host_vectors.VECTORS) for k in range(REF_STEPS)]
        for R in (1, 2, 3):
            f0, b0 = host.images(p, q, th.packed(ref, q, REF_STEPS), REF_STEPS, R, pad=3)
            for k in range(REF_STEPS):
                assert f0[k].tobytes() == want[k]["f"].tobytes(), (name, q, R, k)
                assert b0[k].tobytes() == want[k]["b"].tobytes(), (name, q, R, k)
        for k in range(REF_STEPS):
            pk = _step_problem(name, k)
            r, bound = ch.condense_reference(pk, q), ch.condense_bound(pk, q)
            got = dict(f=f0[k], b=b0[k])
            print(name, q, k, "worst error / bound:", ch.worst_ratio(got, r, bound, names=("f", "b")))
            assert ch.rule_violations(got, r, bound, names=("f", "b")) == []


def test_lds_of_a_workgroup_is_what_the_header_states(host):
    p = sh.setup("small")[0]
    N, nx, nu, nc = p.sizes()
    e = lambda n: n + (n & 1)
    ldx, ldc, ldu = nx | 1, nc | 1, nu | 1
    window = 2 * e(ldx * nx) + e(ldx * nu) + e(ldc * nx) + e(ldu * nx) + e(ldc * nu) + e(ldu * nu)
    for R in (1, 3):
        host.images(p, 0, th.packed(th.references("small"), 0, REF_STEPS), REF_STEPS, R)
        assert host.lds_doubles == window + R * (e((N + 1) * nx) + 2 * e(nx))


def test_a_slot_without_a_reference_reads_the_sequence_of_the_data(host, host_vectors):
    name = "small"
    p = sh.setup(name)[0]
    ref = th.references(name)
    q = 1
    seqs = th.packed(ref, q, REF_STEPS)
    for k in ("r", "c"):                                   # (what the host stage hands over for a NULL slot: step 0)
        seqs[k] = (p.arrays[k][q], 0)
    f0, b0 = host.images(p, q, seqs, REF_STEPS, 2)
    for k in range(REF_STEPS):
        want = host_vectors.condense(_step_problem(name, k, ("q", "d")), q, host_vectors.VECTORS)
        assert f0[k].tobytes() == want["f"].tobytes() and b0[k].tobytes() == want["b"].tobytes(), k


def test_one_reference_for_the_batch_and_a_sliding_window(host, host_vectors):
    name = "small"
    p = sh.setup(name)[0]
    N, nx, nu, nc = p.sizes()
    ref = th.references(name)
    # stride 0: every trajectory reads trajectory 0's rows, with its own model
    shared = th.packed(ref, 0, REF_STEPS)
    for q in (0, 2):
        f0, b0 = host.images(p, q, shared, REF_STEPS, 3)
        for k in range(REF_STEPS):
            pk = th.with_arrays(_step_problem(name, k), **{n: np.repeat(ref[n][k, :1], p.batch, axis=0) for n in th.REF_NAMES})
            want = host_vectors.condense(pk, q, host_vectors.VECTORS)
            assert f0[k].tobytes() == want["f"].tobytes() and b0[k].tobytes() == want["b"].tobytes(), (q, k)
    # a window of (N + 1) nx doubles that slides by nx over one long reference for q
    rng = np.random.default_rng(7)
    long_q = rng.standard_normal((REF_STEPS + N + 1) * nx)
    seqs = th.packed(ref, 1, REF_STEPS)
    seqs["q"] = (long_q, nx)
    f0, b0 = host.images(p, 1, seqs, REF_STEPS, 2)
    for k in range(REF_STEPS):
        qk = p.arrays["q"].copy()
        qk[1] = long_q[k * nx:k * nx + (N + 1) * nx]       # the packed copy
        want = host_vectors.condense(th.with_arrays(_step_problem(name, k), q=qk), 1, host_vectors.VECTORS)
        assert f0[k].tobytes() == want["f"].tobytes() and b0[k].tobytes() == want["b"].tobytes(), k


@pytest.mark.parametrize("defect", ["q_of_the_next_step", "c_dropped"])
def test_the_rule_catches_seeded_defects(host, defect):
    caught = []
    for name in DEVICE_FIXTURES:
        p = sh.setup(name)[0]
        ref = th.references(name)
        seqs = th.packed(ref, 0, REF_STEPS + 1)
        if defect == "q_of_the_next_step":
            seqs["q"] = (seqs["q"][0][ref["q"].shape[2]:], seqs["q"][1])
        else:
            seqs["c"] = (np.zeros_like(seqs["c"][0]), seqs["c"][1])
        f0, b0 = host.images(p, 0, seqs, REF_STEPS, 2)
        good_f0, good_b0 = host.images(p, 0, th.packed(ref, 0, REF_STEPS), REF_STEPS, 2)
        for k in range(REF_STEPS):
            pk = _step_problem(name, k)
            r, bound = ch.condense_reference(pk, 0), ch.condense_bound(pk, 0)
            assert ch.rule_violations(dict(f=good_f0[k], b=good_b0[k]), r, bound, names=("f", "b")) == []
            if ch.rule_violations(dict(f=f0[k], b=b0[k]), r, bound, names=("f", "b")):
                caught.append((name, k))
    print(defect, "caught on", caught)
    assert {n for n, _ in caught} == set(DEVICE_FIXTURES), caught


# ---- 2. the host stage -------------------------------------------------------------------------------------------------
GROUPS = ("images", "sweep", "adjoint", "refusals", "no_refs")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    """-> run(group) -> (exit status, output), as tests/test_condense_stage.py builds its driver.  `sanitized`: built
    with -fsanitize=address,undefined; a finding ends it with a non-zero status."""
    d = tmp_path_factory.mktemp("condense_tracking_stage_" + request.param)
    exe = str(d / "condense_tracking_stage_driver")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", *extra,
                           "-I" + os.path.join(HOSTSIM, "runtime_shim"), "-I" + CSRC, "-o", exe,
                           os.path.join(HOSTSIM, "condense_tracking_stage_driver.cc")])

    def run(group):
        r = subprocess.run([exe, group], capture_output=True, text=True)
        return r.returncode, r.stdout + r.stderr
    return run


@pytest.mark.parametrize("group", GROUPS)
def test_every_launch_of_a_tracked_call_receives_the_pointers_of_its_step(driver, group):
    status, output = driver(group)
    assert status == 0 and output == "", output[-4000:]


def test_the_driver_knows_its_groups(driver):
    assert driver("no such group")[0] == 2


# ---- 3. the reference closed loop ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", th.LOOP_FIXTURES)
def test_reference_loop_on_the_references_retires_as_the_table_says(name):
    p = sh.setup(name)[0]
    for shift in (False, True):
        ref = th.oracle_loop(name, shift=shift)
        assert sh.retirement(ref["eflag"]) == th.RETIRES[name], (name, shift, sh.retirement(ref["eflag"]))
        live = (ref["eflag"] == 0).all(axis=0)
        assert live.sum() >= 3, live
        # the references matter: u moves from the untracked loop's
        g = sh.gap(ref["u"][:, live], sh.oracle_loop(name, shift=shift)["u"][:, live])
        print(name, shift, "gap to the untracked loop:", g)
        assert g >= 0.05, g


# ---- 4. the C-ABI without a GPU ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from fbstab_amd import hip_api
    return hip_api.load_library()


def _lds_bytes(N, nx, nu, nc, R):
    """The formula include/fbstab_hip.h states."""
    e = lambda n: n + (n & 1)
    ldx, ldc, ldu = nx | 1, nc | 1, nu | 1
    window = 2 * e(ldx * nx) + e(ldx * nu) + e(ldc * nx) + e(ldu * nx) + e(ldc * nu) + e(ldu * nu)
    return 8 * (window + R * (e((N + 1) * nx) + 2 * e(nx)))


def _rule(N, nx, nu, nc, steps):
    R = max(1, min(256 // nx, steps))
    while R > 1 and _lds_bytes(N, nx, nu, nc, R) > 80 * 1024:
        R -= 1
    return R


def test_condensed_reference_sizes(lib):
    for N, nx, nu, nc, steps in [(1, 1, 1, 1, 12), (3, 5, 2, 3, 12), (2, 33, 3, 1, 5), (10, 40, 3, 6, 50),
                                 (10, 60, 4, 6, 50), (30, 40, 3, 6, 50), (3, 5, 2, 3, 1)]:
        used, lds = C.c_int(-1), C.c_longlong(-1)
        assert lib.fbstab_hip_mpc_condensed_reference_sizes(N, nx, nu, nc, steps, 0, C.byref(used), C.byref(lds)) == 0
        R = _rule(N, nx, nu, nc, steps)
        assert (used.value, lds.value) == (R, _lds_bytes(N, nx, nu, nc, R)), (N, nx, nu, nc, steps)
        assert lds.value <= 80 * 1024 or R == 1
        assert lib.fbstab_hip_mpc_condensed_reference_sizes(N, nx, nu, nc, steps, 2, C.byref(used), C.byref(lds)) == 0
        assert (used.value, lds.value) == (min(2, steps), _lds_bytes(N, nx, nu, nc, min(2, steps)))
    used, lds = C.c_int(-1), C.c_longlong(-1)
    assert _lds_bytes(10, 40, 3, 6, 40) > 160 * 1024
    assert lib.fbstab_hip_mpc_condensed_reference_sizes(10, 40, 3, 6, 50, 40, C.byref(used), C.byref(lds)) == 3
    assert (used.value, lds.value) == (0, 0) and b"LDS" in lib.fbstab_hip_last_error()
    assert lib.fbstab_hip_mpc_condensed_reference_sizes(3, 5, 2, 3, 0, 0, None, None) == 1
    assert lib.fbstab_hip_mpc_condensed_reference_sizes(3, 5, 2, 3, 4, -1, None, None) == 1
    assert lib.fbstab_hip_mpc_condensed_reference_sizes(3, 0, 2, 3, 4, 0, None, None) == 1
    assert lib.fbstab_hip_mpc_condensed_reference_sizes(3, 5, 2, 3, 4, 0, None, None) == 0   # (null outputs are allowed)


def test_the_images_call_refuses_bad_arguments_before_any_device_call(lib):
    from fbstab_amd import hip_api
    N, nx, nu, nc, batch, steps = 2, 3, 2, 2, 2, 3
    n1 = N + 1
    lens = [n1 * nx * nx, n1 * nu * nu, n1 * nu * nx, n1 * nx, n1 * nu, N * nx * nx, N * nx * nu, N * nx,
            n1 * nc * nx, n1 * nc * nu, n1 * nc, nx]
    buf = np.zeros(4096)

    def call(breaker=None, batch=batch, steps=steps):
        data = hip_api._MpcBatch()
        for i, n in enumerate(lens):
            data.base[i], data.stride[i] = buf.ctypes.data, n
        refs = hip_api._CondensedRefs()
        for i, n in enumerate((n1 * nx, n1 * nu, N * nx, n1 * nc)):
            refs.base[i], refs.step[i], refs.stride[i] = buf.ctypes.data, 2 * n, n
        im = hip_api._CondensedRefImages(buf.ctypes.data, buf.ctypes.data, 2 * n1 * nu, 2 * n1 * nc, n1 * nu, n1 * nc)
        a = dict(data=data, refs=refs, im=im, rpg=0)
        if breaker:
            breaker(a)
        rc = lib.fbstab_hip_mpc_condensed_reference_images_batch(
            N, nx, nu, nc, batch, steps, C.byref(a["data"]), C.byref(a["refs"]) if a["refs"] is not None else None,
            C.byref(a["im"]) if a["im"] is not None else None, a["rpg"], 0, None)
        return rc, lib.fbstab_hip_last_error().decode()

    bad = {
        "negative_step": lambda a: a["refs"].step.__setitem__(0, -1),
        "negative_stride": lambda a: a["refs"].stride.__setitem__(3, -1),
        "short_stride": lambda a: a["refs"].stride.__setitem__(1, n1 * nu - 1),
        "null_images": lambda a: a.__setitem__("im", None),
        "null_f0": lambda a: setattr(a["im"], "f0", None),
        "short_output_step": lambda a: setattr(a["im"], "step_b0", n1 * nc - 1),
        "short_output_stride": lambda a: setattr(a["im"], "stride_f0", 0),
        "negative_refs_per_group": lambda a: a.__setitem__("rpg", -1),
        "null_data_pointer": lambda a: a["data"].base.__setitem__(0, None),
    }
    for name, breaker in bad.items():
        rc, msg = call(breaker)
        assert rc == 1 and msg, (name, rc, msg)
    assert call(steps=-1)[0] == 1
    # nothing to do is OK with or without a device; stride 0 and overlapping windows are allowed
    assert call(batch=0)[0] == 0 and call(steps=0)[0] == 0
    assert call(lambda a: a.__setitem__("refs", None), batch=0)[0] == 0
    ok = lambda a: (a["refs"].stride.__setitem__(0, 0), a["refs"].step.__setitem__(0, nx))
    assert call(ok, batch=0)[0] == 0
    if lib.fbstab_hip_device_count() == 0:
        rc, msg = call(ok)
        assert rc == 2 and "device" in msg, (rc, msg)
