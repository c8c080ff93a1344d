"""The record adjoint of all five record instances in the library the tests load: ten kernels (padded and exact)
inside the register budget the build gates on, and the export that names the kernel a handle's next adjoint call
launches."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INSTANCES = ("<12, 4, 20,", "<12, 4, 32,", "<18, 5, 10,", "<24, 8, 16,", "<24, 8, 32,")


def test_every_record_instance_has_its_adjoint_kernels_inside_the_register_budget():
    """tools/check_vgpr_budget.py --max 496 on the adjoint kernels, as the Makefile runs it on every rec_*.o (no
    --warn-only: the <24,8,*> adjoints call none of the refinement sweeps that put their solve kernels over):
    five instances, padded and exact, none over the budget."""
    from fbstab_amd import hip_api
    hip_api.load_library()
    lib = hip_api.current_library_path()
    tool = os.path.join(ROOT, "tools", "check_vgpr_budget.py")
    r = subprocess.run([sys.executable, tool, "--max", "496", "--only", "fbstab_mpc_r16_adjoint_kernel", lib],
                       capture_output=True, text=True)
    rows = [l for l in r.stdout.splitlines() if "fbstab_mpc_r16_adjoint_kernel<" in l]
    assert len(rows) >= 10, r.stdout[-800:] + r.stderr[-500:]
    for inst in INSTANCES:
        assert sum(inst in l for l in rows) == 2, (inst, rows)
    for l in rows:
        assert "over the budget" not in l, l
        assert int(l.split("->")[1].split()[0]) <= 496, l
    assert r.returncode == 0, r.stdout[-800:]


def test_the_adjoint_kernel_name_is_exported_bound_and_declared():
    from fbstab_amd import hip_api
    sym = "fbstab_hip_mpc_adjoint_kernel_name"
    assert sym in hip_api.EXPORTED_SYMBOLS
    assert hasattr(hip_api.load_library(), sym)
    assert hasattr(hip_api.FBstabMpcBatch, "adjoint_kernel_name")
    with open(os.path.join(ROOT, "include", "fbstab_hip.h")) as f:
        text = f.read()
    assert "const char* %s(fbstab_mpc_handle_t handle);" % sym in text
