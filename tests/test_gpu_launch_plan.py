"""What a created handle reports (fbstab_hip_*_query) against the sizing rules of fbstab_amd/csrc/fb_launch_plan.h as
tests/launch_plan_rules.py restates them: handle creation only, no solve.  (tests/test_launch_plan.py checks the
header itself, as tables on the CPU.)"""
import pytest

from tests.launch_plan_rules import dense_rule, mpc_rule

KNOBS = ("GENERIC", "FLAT_ADJOINT", "LDS_PAD_BYTES", "WGS_PER_CU", "MAX_WORKGROUPS", "DENSE_THREADS", "DENSE_ORDER",
         "DENSE_SPREAD_BITS", "DENSE_STICKY", "DENSE_ACT_BITS")
MAX_BATCH = (3, 4096)
CAPS = (None, "2")

# (id, kind, sizes, FBSTAB_HIP_GENERIC, runs on a record kernel, QPs per workgroup)
SHAPES = [
    ("one-row record", "mpc", (2, 2, 1, 2), None, True, 4),
    ("row-pair record", "mpc", (2, 13, 4, 4), None, True, 2),
    ("flat-vector", "mpc", (2, 2, 1, 2), "1", False, 1),
    ("dense, one wavefront", "dense", (4, 1, 4), None, False, 1),
    ("dense, four wavefronts", "dense", (70, 0, 8), None, False, 1),
]


def handle_rows(shape, monkeypatch_env):
    """-> {(max_batch, cap): (query, names)} of the four handles of a shape; monkeypatch_env(name, value or None)
    sets or unsets a variable.  The uncapped max_batch = 4096 handle comes first."""
    from fbstab_amd import hip_api
    _, kind, sizes, generic, _, _ = shape
    monkeypatch_env("FBSTAB_HIP_GENERIC", generic)
    rows = {}
    for maxb in sorted(MAX_BATCH, reverse=True):
        for cap in CAPS:
            monkeypatch_env("FBSTAB_HIP_MAX_WORKGROUPS", cap)
            if kind == "mpc":
                s = hip_api.FBstabMpcBatch(*sizes, max_batch=maxb)
                names = (s.kernel_name(), s.adjoint_kernel_name(), s.sweep_adjoint_kernel_name())
            else:
                s = hip_api.FBstabDenseBatch(*sizes, max_batch=maxb)
                names = ()
            rows[(maxb, cap)] = (s.query(), names)
            s.close()
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_a_created_handle_reports_the_workgroups_and_scratch_of_the_rule(shape, monkeypatch):
    import torch
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    for knob in KNOBS:
        monkeypatch.delenv("FBSTAB_HIP_" + knob, raising=False)

    def env(name, value):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, value)

    _, kind, sizes, _, record, qps = shape
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    rows = handle_rows(shape, env)
    # the occupancy query's answer, as the handle that has the device to itself and batches to fill it reports it
    q = rows[(4096, None)][0]
    assert q["workgroups"] % cus == 0 and q["workgroups"] < 4096, q
    resident = q["workgroups"] // cus
    assert q["scratch_bytes"] % (q["workgroups"] * qps) == 0, q
    per_slot = q["scratch_bytes"] // (q["workgroups"] * qps)  # bytes of scratch per QP slot: the shape's, not the grid's
    if kind == "mpc":
        # (the table above says which handles run on a record kernel: the flat-vector kernel has one name)
        assert (rows[(4096, None)][1][0] != "fbstab_mpc_kernel<64>") == record, rows[(4096, None)][1]
        assert per_slot > 0
    assert per_slot % 8 == 0
    for (maxb, cap), (q, names) in rows.items():
        if kind == "mpc":
            # (one handle in flight: the hardware queues of the process do not enter)
            want = mpc_rule(cus, resident, 1, 4, record, qps, maxb, per_slot // 8, None, cap)
        else:
            want = dense_rule(cus, resident, maxb, per_slot // 8, None, cap)
        print("%s max_batch %d FBSTAB_HIP_MAX_WORKGROUPS %s: CUs %d, resident %d: %r %r (rule: %r)"
              % (shape[0], maxb, cap, cus, resident, q, names, want))
        assert q["workgroups"] == want[0], (maxb, cap, q, want)
        assert q["scratch_bytes"] == want[1], (maxb, cap, q, want)
        assert q["scratch_bytes"] % (q["workgroups"] * qps) == 0, (maxb, cap, q)
        assert q["scratch_bytes"] // (q["workgroups"] * qps) == per_slot, (maxb, cap, q, per_slot)
