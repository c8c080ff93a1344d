"""The host side of the condensed MPC route (fbstab_amd/csrc/fb_condense_stage.h over fb_condense_plan.h: the argument
checks, the blocks as the kernels take them, the callers' work arrays, the order of the launches) on the CPU: the
header compiles with the host compiler over the heap-backed <hip/hip_runtime.h> of tests/hostsim/runtime_shim, and
tests/hostsim/condense_stage_driver.cc runs it with host lambdas in the place of the kernels and of the dense handle -
plain, and once more under the address and undefined-behaviour sanitizers, where a work array that is carved one
double too long, or a stride that should not have been read, ends the driver.  A group that fails prints its findings
and exits non-zero, one that passes prints nothing.  What the kernels compute behind the same calls is
tests/test_gpu_condense*.py's; asynchrony and copy direction are not shown here (runtime_shim)."""
import os
import subprocess

import pytest

from tests.test_host_stage import CSRC, HOSTSIM, ROOT, _include_closure

GROUPS = ("placement", "carve", "sequence", "refusals")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    """-> run(group) -> (exit status, output).  `sanitized`: the same driver built with
    -fsanitize=address,undefined; a finding ends it with a non-zero status."""
    d = tmp_path_factory.mktemp("condense_stage_" + request.param)
    exe = str(d / "condense_stage_driver")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", *extra,
                           "-I" + os.path.join(HOSTSIM, "runtime_shim"), "-I" + CSRC, "-o", exe,
                           os.path.join(HOSTSIM, "condense_stage_driver.cc")])

    def run(group):
        r = subprocess.run([exe, group], capture_output=True, text=True)
        return r.returncode, r.stdout + r.stderr
    return run


@pytest.mark.parametrize("group", GROUPS)
def test_the_condensed_stage_checks_places_carves_and_queues_as_the_header_says(driver, group):
    status, output = driver(group)
    assert status == 0 and output == "", output[-4000:]


def test_the_driver_knows_its_groups(driver):
    assert driver("no such group")[0] == 2


def test_the_stage_reaches_no_kernel_header_and_the_plan_only_the_public_one():
    closure = {os.path.relpath(p, ROOT) for p in _include_closure(os.path.join(CSRC, "fb_condense_stage.h"), set())}
    assert closure == {"include/fbstab_hip.h", "include/fbstab_types.h", "fbstab_amd/csrc/fb_condense_plan.h",
                       "fbstab_amd/csrc/fb_host_stage.h", "fbstab_amd/csrc/fb_grad_reduce_plan.h",
                       "fbstab_amd/csrc/fb_launch_plan.h", "fbstab_amd/csrc/fb_in_flight.h"}, closure
    for name in ("fb_condense_stage.h", "fb_condense_plan.h"):
        text = open(os.path.join(CSRC, name)).read()
        assert "__global__" not in text and "hipLaunchKernelGGL" not in text and "FB_DEV" not in text, name
    plan = {os.path.relpath(p, ROOT) for p in _include_closure(os.path.join(CSRC, "fb_condense_plan.h"), set())}
    assert plan == {"include/fbstab_hip.h", "include/fbstab_types.h"}, plan
