"""How a handle is sized and how its launches are shaped (fbstab_amd/csrc/fb_launch_plan.h, behind both create
functions and every launch site of the C-ABI unit): the header compiles with the host compiler alone, and a driver
prints its answers for whole tables of inputs - plain and once more under the address and undefined-behaviour
sanitizers - which are compared with the rules as they are restated here, from their description and not from the
header's code.  tests/test_gpu_launch_plan.py holds what a created handle reports against the same restatement."""
import itertools
import os
import subprocess

import pytest

from tests.launch_plan_rules import (batch_grid_rule, dense_rule, mpc_per_cu, mpc_rule, one_launch_sweep_rule,
                                     positive_knob, slots_hold_rule)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fbstab_amd", "csrc")

# One row of input per line on stdin, one row of answers per line on stdout ("-": an unset variable).
DRIVER = r'''
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "fb_launch_plan.h"
namespace {
const char* text_of(const std::string& s) { return s == "-" ? nullptr : s.c_str(); }
fbk::CreateKnobs knobs_of(const std::string& wgs, const std::string& cap) {
  fbk::CreateKnobText t;
  t.wgs_per_cu = text_of(wgs);
  t.max_workgroups = text_of(cap);
  return fbk::create_knobs_from(t);
}
}  // namespace
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind, wgs, cap;
    in >> kind;
    if (kind == "mpc") {
      int cus, occ, hif, hwq, record, qps, maxb;
      long long ws;
      in >> cus >> occ >> hif >> hwq >> record >> qps >> maxb >> ws >> wgs >> cap;
      const fbk::LaunchPlan p = fbk::mpc_plan(cus, occ, hif, hwq, record != 0, qps, maxb, ws, knobs_of(wgs, cap));
      std::printf("%d %lld\n", p.workgroups, p.scratch_bytes);
    } else if (kind == "dense") {
      int cus, occ, maxb, wave, kglobal;
      long long ws, kv;
      in >> cus >> occ >> maxb >> wave >> ws >> kglobal >> kv >> wgs >> cap;
      const fbk::LaunchPlan p = fbk::dense_plan(cus, occ, maxb, wave != 0, ws, kglobal != 0, kv, knobs_of(wgs, cap));
      std::printf("%d %lld\n", p.workgroups, p.scratch_bytes);
    } else if (kind == "launch") {
      int w, per_wg, batch;
      long long nz;
      in >> w >> per_wg >> batch >> nz;
      const int grid = fbk::batch_grid(batch, w, per_wg);
      std::printf("%d %d %d %d %d %zu", grid, fbk::keep_grid(batch, per_wg), fbk::dense_grid(batch, w),
                  (int)fbk::slots_hold(batch, w, per_wg), (int)fbk::record_spreads(batch, grid),
                  fbk::sweep_seed_bytes(nz, w, per_wg));
      const int steps[] = {0, 1, 0xfffe, 0xffff};
      for (int record = 0; record < 2; record++)
        for (int st : steps)
          for (int per_step = 0; per_step < 2; per_step++)
            std::printf(" %d", (int)fbk::sweep_in_one_launch(record != 0, batch, w, per_wg, st, per_step != 0));
      std::printf("\n");
    } else if (kind == "knob") {  // knob <index> followed by "-" (unset) or "=<text>"
      int index;
      std::string rest;
      in >> index >> rest;
      const std::string value = rest.size() > 1 ? rest.substr(1) : "";
      const char* text = rest == "-" ? nullptr : value.c_str();
      fbk::CreateKnobText t;
      const char** slot[] = {&t.generic, &t.flat_adjoint, &t.lds_pad_bytes, &t.wgs_per_cu, &t.max_workgroups,
                             &t.dense_threads, &t.dense_order, &t.dense_spread_bits, &t.dense_sticky,
                             &t.dense_act_bits};
      if (index < 10) *slot[index] = text;
      const fbk::CreateKnobs k = fbk::create_knobs_from(t);
      std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d\n", (int)k.generic, k.flat_adjoint, k.lds_pad_bytes,
                  k.wgs_per_cu, k.max_workgroups, k.dense_threads, fbk::dense_threads_choice(k, 4, 1),
                  fbk::dense_threads_choice(k, 70, 0), k.dense_order, k.dense_spread_bits, k.dense_sticky,
                  k.dense_act_bits, (int)fbk::sweep_per_step_from(index == 10 ? text : nullptr),
                  (int)fbk::sweep_adjoint_per_step_from(index == 11 ? text : nullptr));
    } else {
      return 2;
    }
  }
  return 0;
}
'''


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def driver(request, tmp_path_factory):
    """-> run(rows) -> the driver's answer lines.  `sanitized`: the same driver built with
    -fsanitize=address,undefined; a finding ends it with a non-zero status."""
    d = tmp_path_factory.mktemp("launch_plan_" + request.param)
    src = d / "plan_table.cc"
    src.write_text(DRIVER)
    exe = str(d / "plan_table")
    extra = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if request.param == "sanitized" else []
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", *extra, "-I" + CSRC, "-o", exe,
                           str(src)])

    def run(rows):
        r = subprocess.run([exe], input="".join(row + "\n" for row in rows), capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-2000:]
        out = r.stdout.splitlines()
        assert len(out) == len(rows)
        return out
    return run


# ---- creation -----------------------------------------------------------------------------------------------------

CUS = (1, 4, 256)
OCCUPANCY = (0, 1, 2, 4, 8, 9)  # (0 and 9: outside the 1..8 the rule counts with)
HANDLES = (1, 2, 8)
QUEUES = (1, 4, 8)
QPS = (1, 2, 4)
WGS_PER_CU = (None, "0", "2", "x")
MAX_WORKGROUPS = (None, "0", "1", "2")
WS_DOUBLES = 1237  # (odd: a factor that went missing shows)


def batches_around(w):
    """max_batch: the small ones, and the ones around the uncapped grid w and four times it."""
    return sorted({b for b in (1, 2, 3, 4, 5, w - 1, w, w + 1, 4 * w, 4 * w + 1) if b >= 1})


def tok(text):
    return "-" if text is None else text


def test_mpc_handles_get_the_workgroups_and_scratch_of_the_rule(driver):
    rows, want = [], []
    for cus, occ, hif, hwq, qps, record, wgs, cap in itertools.product(CUS, OCCUPANCY, HANDLES, QUEUES, QPS, (0, 1),
                                                                        WGS_PER_CU, MAX_WORKGROUPS):
        for maxb in batches_around(cus * mpc_per_cu(occ, hif, hwq, wgs)):
            rows.append("mpc %d %d %d %d %d %d %d %d %s %s" % (cus, occ, hif, hwq, record, qps, maxb, WS_DOUBLES,
                                                               tok(wgs), tok(cap)))
            want.append(mpc_rule(cus, occ, hif, hwq, record, qps, maxb, WS_DOUBLES, wgs, cap))
    got = [tuple(int(x) for x in line.split()) for line in driver(rows)]
    for row, g, w in zip(rows, got, want):
        assert g == w, (row, g, w)
        # a handle never keeps more workgroups than its max_batch can use, and scratch for every slot of them
        assert 1 <= g[0] and g[1] % (g[0] * int(row.split()[6])) == 0, (row, g)


def test_dense_handles_get_the_workgroups_and_scratch_of_the_rule(driver):
    rows, want = [], []
    scratch = (("1 %d 0 0" % WS_DOUBLES, WS_DOUBLES), ("0 0 1 %d" % (3 * WS_DOUBLES), 3 * WS_DOUBLES),
               ("0 %d 0 %d" % (WS_DOUBLES, WS_DOUBLES), 0))  # wave; K in global scratch; everything in LDS
    for cus, occ, wgs, cap in itertools.product(CUS, OCCUPANCY, WGS_PER_CU, MAX_WORKGROUPS):
        for maxb in batches_around(cus * (positive_knob(wgs) or min(max(occ, 1), 8))):
            for args, per_wg_doubles in scratch:
                rows.append("dense %d %d %d %s %s %s" % (cus, occ, maxb, args, tok(wgs), tok(cap)))
                want.append(dense_rule(cus, occ, maxb, per_wg_doubles, wgs, cap))
    got = [tuple(int(x) for x in line.split()) for line in driver(rows)]
    for row, g, w in zip(rows, got, want):
        assert g == w, (row, g, w)
        assert 1 <= g[0] <= int(row.split()[3]), (row, g)


# ---- launches -----------------------------------------------------------------------------------------------------

def test_every_launch_gets_the_grid_of_the_rule_and_the_device_spreads_when_the_host_does(driver):
    nz = 7
    cases = [(w, p, b) for w in (1, 2, 3, 8) for p in (1, 2, 4) for b in range(0, 4 * w * p + 2)]
    out = driver(["launch %d %d %d %d" % (w, p, b, nz) for w, p, b in cases])
    for (w, p, b), line in zip(cases, out):
        grid, keep, dense, holds, spreads, seed, *one_launch = (int(x) for x in line.split())
        assert grid == batch_grid_rule(b, w, p), (w, p, b, grid)
        assert keep == -(-b // p), (w, p, b, keep)
        assert dense == min(b, w), (w, p, b, dense)
        assert bool(holds) == slots_hold_rule(b, w, p), (w, p, b, holds)
        assert seed == 8 * nz * w * p, (w, p, b, seed)
        want = [one_launch_sweep_rule(record, b, w, p, steps, per_step)
                for record in (0, 1) for steps in (0, 1, 0xfffe, 0xffff) for per_step in (0, 1)]
        assert [bool(x) for x in one_launch] == want, (w, p, b, one_launch)
        if b >= 1:
            assert 1 <= grid <= max(1, w), (w, p, b, grid)
        if not b <= w:  # packed: every QP of the batch, or every slot of the handle, is served at once
            assert grid * p >= min(b, w * p), (w, p, b, grid)
        # R16Queue::fetch (fb_record_kernel.h) spreads when batch <= gridDim.x: exactly when the host rule did
        assert bool(spreads) == (b <= grid), (w, p, b)
        assert bool(spreads) == (b <= w), (w, p, b, grid)
        # a KEEP launch has a slot for every QP exactly where the handle's slots hold the batch
        if holds:
            assert keep <= w, (w, p, b, keep)


# ---- knobs --------------------------------------------------------------------------------------------------------

UNSET = None
COMMON = (UNSET, "", "0", "1", "-1", "2x", "abc")
# the driver's columns, and what they hold with nothing set
COLUMNS = ("generic", "flat_adjoint", "lds_pad_bytes", "wgs_per_cu", "max_workgroups", "dense_threads",
           "threads_choice_small", "threads_choice_large", "dense_order", "dense_spread_bits", "dense_sticky",
           "dense_act_bits", "sweep_per_step", "sweep_adjoint_per_step")
DEFAULTS = dict(zip(COLUMNS, (0, -1, 0, 0, 0, 0, 0, 0, -1, 0, -1, -1, 0, 0)))
AUTO, PIVOTED, NATURAL = 0, 1, 2  # (include/fbstab_hip.h: FBSTAB_HIP_DENSE_ORDER_*)
# (variable, its index in the driver, the columns it moves, {text: their values}) - what today's expressions give
KNOBS = [
    ("GENERIC", 0, ("generic",),
     {UNSET: 0, "": 0, "0": 0, "1": 1, "-1": 0, "2x": 1, "abc": 0}),
    ("FLAT_ADJOINT", 1, ("flat_adjoint",),
     {UNSET: -1, "": -1, "0": 0, "1": 1, "-1": 0, "2x": 1, "abc": 0}),
    ("LDS_PAD_BYTES", 2, ("lds_pad_bytes",),
     {UNSET: 0, "": 0, "0": 0, "1": 0, "-1": 0, "2x": 0, "abc": 0, "17": 16, "16": 16, "4111": 4096}),
    ("WGS_PER_CU", 3, ("wgs_per_cu",),
     {UNSET: 0, "": 0, "0": 0, "1": 1, "-1": 0, "2x": 2, "abc": 0}),
    ("MAX_WORKGROUPS", 4, ("max_workgroups",),
     {UNSET: 0, "": 0, "0": 0, "1": 1, "-1": 0, "2x": 2, "abc": 0}),
    # (the number; what a handle of nz + nl = 5 makes of it; what one of nz + nl = 70 does)
    ("DENSE_THREADS", 5, ("dense_threads", "threads_choice_small", "threads_choice_large"),
     {UNSET: (0, 0, 0), "": (0, 0, 0), "0": (0, 0, 0), "1": (1, 0, 0), "-1": (-1, 0, 0), "2x": (2, 0, 0),
      "abc": (0, 0, 0), "256": (256, 256, 256), "64": (64, 64, 0), "128": (128, 0, 0)}),
    ("DENSE_ORDER", 6, ("dense_order",),
     {UNSET: -1, "": -1, "0": -1, "1": -1, "-1": -1, "2x": -1, "abc": -1, "auto": AUTO, "natural": NATURAL,
      "pivoted": PIVOTED, "Auto": -1}),
    ("DENSE_SPREAD_BITS", 7, ("dense_spread_bits",),
     {UNSET: 0, "": 0, "0": 0, "1": 1, "-1": 0, "2x": 2, "abc": 0}),
    ("DENSE_STICKY", 8, ("dense_sticky",),
     {UNSET: -1, "": 0, "0": 0, "1": 1, "-1": 1, "2x": 1, "abc": 0}),
    ("DENSE_ACT_BITS", 9, ("dense_act_bits",),
     {UNSET: -1, "": 0, "0": 0, "1": 1, "-1": -1, "2x": 2, "abc": 0, "999": 999, "1000": -1}),
    ("SWEEP_PER_STEP", 10, ("sweep_per_step",),
     {UNSET: 0, "": 0, "0": 0, "1": 1, "-1": 1, "2x": 1, "abc": 0}),
    ("SWEEP_ADJOINT_PER_STEP", 11, ("sweep_adjoint_per_step",),
     {UNSET: 0, "": 0, "0": 0, "1": 1, "-1": 1, "2x": 1, "abc": 0}),
]


@pytest.mark.parametrize("name, index, moved, table", KNOBS, ids=[k[0] for k in KNOBS])
def test_every_knob_parses_as_it_always_did_and_moves_nothing_else(driver, name, index, moved, table):
    assert set(COMMON) <= set(table), name
    texts = list(table)
    out = driver(["knob %d %s" % (index, "-" if t is UNSET else "=" + t) for t in texts])
    for t, line in zip(texts, out):
        got = dict(zip(COLUMNS, (int(x) for x in line.split())))
        values = table[t] if isinstance(table[t], tuple) else (table[t],)
        assert got == {**DEFAULTS, **dict(zip(moved, values))}, (name, t, got)


def test_every_knob_of_the_c_abi_unit_is_read_in_the_header_and_has_a_row_above():
    """fbstab_hip.hip reads no variable itself; fb_launch_plan.h reads the ones of the table, each in one place."""
    import re
    assert "getenv" not in open(os.path.join(CSRC, "fbstab_hip.hip")).read()
    names = re.findall(r'getenv\(\s*"([^"]+)"', open(os.path.join(CSRC, "fb_launch_plan.h")).read())
    assert sorted(names) == sorted("FBSTAB_HIP_" + k[0] for k in KNOBS)
