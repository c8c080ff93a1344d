"""The host staging of the C-ABI (fbstab_amd/csrc/fb_host_stage.h: SolverBase, the stages, the *_run templates, the
stride rules that take a handle's lengths; fb_sweep_stage.h: the closed-loop sweeps and their adjoint) on the CPU: the header compiles with the host compiler over a heap-backed
<hip/hip_runtime.h> (tests/hostsim/runtime_shim), and tests/hostsim/stage_driver.cc runs it with host lambdas in the
kernels' place - plain, and once more under the address and undefined-behaviour sanitizers, where device memory is
the heap and a copy that overruns a staging buffer by one double ends the driver.  The driver holds the expected
placements, restated from include/fbstab_hip.h; a group that fails prints its findings and exits non-zero, one that
passes prints nothing.  What a created handle does with the same calls on a GPU is tests/test_gpu_placement.py's."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fbstab_amd", "csrc")
HOSTSIM = os.path.join(ROOT, "tests", "hostsim")

GROUPS = ("solve", "solve_device_pointers", "adjoint", "tangent", "multi", "multi_run", "sweep", "sweep_adjoint", "probe",
          "refusals", "leaks")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    """-> run(group) -> (exit status, output).  `sanitized`: the same driver built with
    -fsanitize=address,undefined; a finding ends it with a non-zero status."""
    d = tmp_path_factory.mktemp("host_stage_" + request.param)
    exe = str(d / "stage_driver")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", *extra,
                           "-I" + os.path.join(HOSTSIM, "runtime_shim"), "-I" + CSRC, "-o", exe,
                           os.path.join(HOSTSIM, "stage_driver.cc")])

    def run(group):
        r = subprocess.run([exe, group], capture_output=True, text=True)
        return r.returncode, r.stdout + r.stderr
    return run


@pytest.mark.parametrize("group", GROUPS)
def test_the_staging_puts_every_double_where_the_header_says_and_nowhere_else(driver, group):
    status, output = driver(group)
    assert status == 0 and output == "", output[-4000:]


def test_the_driver_knows_its_groups(driver):
    assert driver("no such group")[0] == 2


def _include_closure(path, seen):
    for inc in re.findall(r'^#include "([^"]+)"', open(path).read(), re.M):
        p = os.path.normpath(os.path.join(os.path.dirname(path), inc))
        if p not in seen:
            seen.add(p)
            _include_closure(p, seen)
    return seen


def test_no_kernel_header_is_in_the_closure_of_the_staging_header():
    closure = {os.path.relpath(p, ROOT) for p in _include_closure(os.path.join(CSRC, "fb_host_stage.h"), set())}
    assert closure == {"include/fbstab_hip.h", "include/fbstab_types.h", "fbstab_amd/csrc/fb_grad_reduce_plan.h",
                       "fbstab_amd/csrc/fb_launch_plan.h", "fbstab_amd/csrc/fb_in_flight.h"}, closure
    text = open(os.path.join(CSRC, "fb_host_stage.h")).read()
    assert "__global__" not in text and "hipLaunchKernelGGL" not in text
    # ... and the sweeps' staging header adds fb_host_stage.h to that closure, and nothing else
    sweep = {os.path.relpath(p, ROOT) for p in _include_closure(os.path.join(CSRC, "fb_sweep_stage.h"), set())}
    assert sweep == closure | {"fbstab_amd/csrc/fb_host_stage.h"}, sweep
    text = open(os.path.join(CSRC, "fb_sweep_stage.h")).read()
    assert "__global__" not in text and "hipLaunchKernelGGL" not in text
