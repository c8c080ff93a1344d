"""The grid a handle takes when it shares the device (fbstab_amd/csrc/fb_in_flight.h, behind
fbstab_hip_mpc_create_in_flight): the rule as a table on the CPU - the header compiles with the host compiler
alone -, and on the GPU what fbstab_hip_mpc_query reports against the same rule, with bitwise equal outputs
whatever share a handle got (a QP's bits do not depend on the row, wavefront or workgroup that solves it:
DESIGN.md 4.1)."""
import os
import subprocess

import numpy as np
import pytest

from tools import fixtures as fx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fbstab_amd", "csrc")

RESIDENT = (1, 2, 3, 4, 8)
HANDLES = tuple(range(1, 65))
QUEUES = (1, 2, 4, 8, 32)

DRIVER = r'''
#include <cstdio>
#include "fb_in_flight.h"
int main(int argc, char** argv) {
  if (argc > 1) { std::printf("%d\n", fbk::hw_queues_hint_from(argv[1][0] == '-' && !argv[1][1] ? nullptr : argv[1])); return 0; }
  const int res[] = {1, 2, 3, 4, 8}, hwq[] = {1, 2, 4, 8, 32};
  for (int r : res) for (int h = 1; h <= 64; h++) for (int q : hwq)
    std::printf("%d %d %d %d\n", r, h, q, fbk::in_flight_wgs_per_cu(r, h, q));
  return 0;
}
'''


def share_rule(resident, handles_in_flight, hw_queues):
    """The rule, restated: launches that can be resident side by side x grid = twice the resident slots; a
    handle that shares the device keeps at most half the grid; one handle alone keeps all of it."""
    if handles_in_flight == 1:
        return resident
    concurrent = min(handles_in_flight, hw_queues)
    share = -(-2 * resident // concurrent)
    share = max(1, min(share, resident))
    return min(share, max(1, resident // 2))


def hw_queues_hint(text):
    """GPU_MAX_HW_QUEUES as the library reads it: a decimal in 1..32, anything else is HIP's default of 4."""
    import re
    if text is None or not re.fullmatch(r"\s*[+-]?[0-9]+", text):
        return 4
    v = int(text)
    return v if 1 <= v <= 32 else 4


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("in_flight")
    src = d / "share_table.cc"
    src.write_text(DRIVER)
    exe = str(d / "share_table")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I" + CSRC, "-o", exe, str(src)])
    return exe


@pytest.fixture(scope="module")
def table(driver):
    out = subprocess.run([driver], capture_output=True, text=True, check=True).stdout
    t = {}
    for line in out.splitlines():
        r, h, q, w = (int(x) for x in line.split())
        t[(r, h, q)] = w
    assert len(t) == len(RESIDENT) * len(HANDLES) * len(QUEUES)
    return t


def test_the_rows_the_header_documents(table):
    """resident = 4, the BASELINE shape: (handles_in_flight, hw_queues) -> workgroups per CU."""
    assert table[(4, 8, 8)] == 1    # unchanged: eight launches of 256 workgroups
    assert table[(4, 8, 4)] == 2    # four launches can overlap: 4 x 512
    assert table[(4, 4, 4)] == 2 and table[(4, 4, 8)] == 2 and table[(4, 4, 32)] == 2
    for q in QUEUES:
        assert table[(4, 2, q)] == 2
        assert table[(4, 1, q)] == 4


def test_bounds_and_monotonicity_over_the_whole_table(table):
    for (r, h, q), w in table.items():
        assert w == share_rule(r, h, q), (r, h, q, w)
        assert 1 <= w <= r, (r, h, q, w)
        if h >= 2 and r >= 2:
            assert 2 * w <= r, (r, h, q, w)
        if h == 1:
            assert w == r
    # monotone non-increasing in the launches that can overlap: more of them never means a larger grid each
    for r in RESIDENT:
        by_c = {}
        for h in HANDLES:
            for q in QUEUES:
                by_c.setdefault(min(h, q), []).append(table[(r, h, q)])
        cs = sorted(by_c)
        for a, b in zip(cs, cs[1:]):
            assert min(by_c[a]) >= max(by_c[b]), (r, a, b, by_c[a], by_c[b])


@pytest.mark.parametrize("text, want", [("-", 4), ("4", 4), ("8", 8), ("1", 1), ("32", 32), ("33", 4), ("0", 4),
                                        ("-3", 4), ("eight", 4), ("8x", 4), ("", 4), ("16", 16)])
def test_the_queue_hint_accepts_1_to_32_and_falls_back_to_hips_default(driver, text, want):
    """("-" stands for unset.)"""
    assert int(subprocess.run([driver, text], capture_output=True, text=True, check=True).stdout) == want
    assert hw_queues_hint(None if text == "-" else text) == want


def test_the_library_reads_the_queue_hint_and_touches_no_other_runtime_variable():
    """The share rule's queue count is read, never written: no setenv / putenv / unsetenv in the native sources,
    and GPU_MAX_HW_QUEUES is the only variable of the HIP runtime they name."""
    import re
    names = set()
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".h", ".hip")):
            continue
        text = open(os.path.join(CSRC, f)).read()
        assert not re.search(r"\b(setenv|putenv|unsetenv)\s*\(", text), f
        names.update(re.findall(r'getenv\(\s*"([^"]+)"', text))
    assert "GPU_MAX_HW_QUEUES" in names
    assert all(n.startswith("FBSTAB_HIP_") for n in names - {"GPU_MAX_HW_QUEUES"}), names


@pytest.mark.gpu
def test_a_handles_grid_follows_the_rule_and_its_share_leaves_the_bits_alone(monkeypatch):
    """B = 2048 of the BASELINE workload through handles created for 1, 4 and 8 in flight: `workgroups` is
    CUs x the rule at the ambient GPU_MAX_HW_QUEUES (capped by max_batch: a record kernel never takes more
    workgroups than QPs), and z, l, v, y and the SolverOut fields are bitwise equal across the three."""
    import torch
    from fbstab_amd import hip_api
    assert hip_api.load_library().fbstab_hip_device_count() >= 1
    for knob in ("FBSTAB_HIP_WGS_PER_CU", "FBSTAB_HIP_MAX_WORKGROUPS", "FBSTAB_HIP_GENERIC", "FBSTAB_HIP_LDS_PAD_BYTES"):
        monkeypatch.delenv(knob, raising=False)
    hwq = hw_queues_hint(os.environ.get("GPU_MAX_HW_QUEUES"))
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 2048
    p = fx.synthetic_mpc_batch(B)
    data = {k: np.ascontiguousarray(a) for k, a in p.arrays.items()}
    res, resident = {}, None
    for k in (1, 4, 8):
        s = hip_api.FBstabMpcBatch(*p.sizes(), max_batch=B, handles_in_flight=k)
        q = s.query()
        if k == 1:
            # the occupancy query's answer, as the handle that has the device to itself reports it
            assert q["workgroups"] % cus == 0 and q["workgroups"] < B
            resident = q["workgroups"] // cus
        want = min(B, cus * share_rule(resident, k, hwq))
        print("handles_in_flight %d: GPU_MAX_HW_QUEUES hint %d, resident %d, CUs %d: workgroups %d (rule: %d), scratch %d bytes"
              % (k, hwq, resident, cus, q["workgroups"], want, q["scratch_bytes"]))
        assert q["workgroups"] == want, (k, hwq, resident, q)
        z = np.zeros((B, p.nz)); l = np.zeros((B, p.nl)); v = np.zeros((B, p.nv)); y = np.zeros((B, p.nv))
        out = s.Solve(data, z, l, v, y)
        res[k] = (z, l, v, y, out)
        s.close()
    assert (res[1][4]["eflag"] == 0).all()
    for k in (4, 8):
        for name, a, b in zip("zlvy", res[1][:4], res[k][:4]):
            assert np.array_equal(a, b), (k, name)
        for f in ("eflag", "residual", "newton_iters", "prox_iters"):
            assert np.array_equal(res[1][4][f], res[k][4][f]), (k, f)
