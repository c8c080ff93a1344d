"""When a record handle hands its queue tickets out longest-first (fbstab_amd/csrc/fb_queue_order_plan.h, behind
fbstab_hip_mpc_solve_batch and fbstab_hip_mpc_queue_order): the rule as a table on the CPU - the header compiles
with the host compiler alone, and the spread it asks about is fb_launch_plan.h's -, the parse of
FBSTAB_HIP_QUEUE_ORDER, and the places the sources read it."""
import itertools
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fbstab_amd", "csrc")

# One row of input per line on stdin, one row of answers per line on stdout.
DRIVER = r'''
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "fb_launch_plan.h"
#include "fb_queue_order_plan.h"
int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream in(line);
    std::string kind;
    in >> kind;
    if (kind == "rule") {
      int knob, record, batch, workgroups, per_wg, order_batch;
      in >> knob >> record >> batch >> workgroups >> per_wg >> order_batch;
      const bool spread = fbk::record_spreads(batch, fbk::batch_grid(batch, workgroups, per_wg));
      const bool sorts = fbk::queue_order_sorts(knob != 0, record != 0, spread, batch);
      std::printf("%d %d %d\n", (int)sorts,
                  (int)fbk::queue_order_applies(knob != 0, record != 0, spread, batch, order_batch),
                  fbk::queue_order_batch_after(sorts, batch, order_batch));
    } else if (kind == "knob") {  // "-" (unset) or "=<text>"
      std::string rest;
      in >> rest;
      const std::string value = rest.size() > 1 ? rest.substr(1) : "";
      const char* text = rest == "-" ? nullptr : value.c_str();
      std::printf("%d\n", (int)fbk::queue_order_knob_from(text));
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
    d = tmp_path_factory.mktemp("queue_order_" + request.param)
    src = d / "order_table.cc"
    src.write_text(DRIVER)
    exe = str(d / "order_table")
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


def rule(knob, record, batch, workgroups, order_batch):
    """The rule, restated: a packed batch solve of a record instance on a handle with the knob on sorts its counts
    behind it, and uses the stored order where that was made for its batch
    size; nothing else touches the stored order."""
    sorts = bool(knob and record and batch > workgroups and batch >= 1)
    return sorts, sorts and order_batch == batch, batch if sorts else order_batch


WORKGROUPS = (1, 2, 256, 1024)
PER_WG = (1, 2, 4)


def _batches(w):
    return sorted({1, 2, w - 1, w, w + 1, 2 * w, 4 * w, 4 * w + 1, 8192, 65535, 65536, 1 << 20} - {0})


def test_the_order_is_kept_and_used_by_the_rule_over_the_whole_table(driver):
    rows, want = [], []
    for knob, record, w, per_wg in itertools.product((0, 1), (0, 1), WORKGROUPS, PER_WG):
        for batch in _batches(w):
            for order_batch in (-1, batch, batch + 5, 8192):
                rows.append("rule %d %d %d %d %d %d" % (knob, record, batch, w, per_wg, order_batch))
                want.append(rule(knob, record, batch, w, order_batch))
    for row, line, (sorts, applies, after) in zip(rows, driver(rows), want):
        assert [int(x) for x in line.split()] == [int(sorts), int(applies), after], row


def test_the_rows_the_header_documents(driver):
    """A handle of 1024 workgroups of four rows, the knob on.  (rule knob record batch workgroups per_wg order_batch)"""
    ask = lambda *a: [int(x) for x in driver(["rule " + " ".join(map(str, a))])[0].split()]
    assert ask(1, 1, 8192, 1024, 4, -1) == [1, 0, 8192]       # the first solve: index order, installs its order
    assert ask(1, 1, 8192, 1024, 4, 8192) == [1, 1, 8192]     # the next one of the same size: ordered
    assert ask(1, 1, 8187, 1024, 4, 8192) == [1, 0, 8187]     # another size: not by the old order, installs its own
    assert ask(1, 1, 1024, 1024, 4, 8192) == [0, 0, 8192]     # spread: neither uses nor changes it ...
    assert ask(1, 1, 1025, 1024, 4, 1025) == [1, 1, 1025]     # ... one QP past the grid: packed, ordered
    assert ask(1, 0, 8192, 1024, 4, 8192) == [0, 0, 8192]     # KEEP solves, sweeps, adjoints, probes, flat-vector kernels
    assert ask(0, 1, 8192, 1024, 4, -1) == [0, 0, -1]         # FBSTAB_HIP_QUEUE_ORDER=0
    assert ask(1, 1, 1 << 20, 1024, 4, 1 << 20) == [1, 1, 1 << 20]


# what today's expression gives: on unless the text is a number that is 0 (atoi: text that is no number reads as 0;
# empty counts as unset)
KNOB = {None: 1, "": 1, "0": 0, "1": 1, "-1": 1, "2x": 1, "abc": 0, "00": 0, "0x": 0, "8": 1}


def test_the_knob_is_on_unless_it_holds_a_zero(driver):
    texts = list(KNOB)
    out = driver(["knob %s" % ("-" if t is None else "=" + t) for t in texts])
    for t, line in zip(texts, out):
        assert int(line) == KNOB[t], t


def test_the_variable_is_read_in_one_place_and_once_per_handle():
    """getenv of FBSTAB_HIP_QUEUE_ORDER stands once, in fb_queue_order_plan.h (fbstab_hip.hip calls getenv nowhere),
    and the C-ABI unit asks for it in one place, where it creates an MPC handle."""
    hits = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".h", ".hip")):
            n = len(re.findall(r'getenv\(\s*"FBSTAB_HIP_QUEUE_ORDER"', open(os.path.join(CSRC, f)).read()))
            if n:
                hits[f] = n
    assert hits == {"fb_queue_order_plan.h": 1}
    unit = open(os.path.join(CSRC, "fbstab_hip.hip")).read()
    assert "getenv" not in unit and unit.count("queue_order_knob()") == 1
    create = unit[unit.index("int fbstab_hip_mpc_create_in_flight("):unit.index("int fbstab_hip_mpc_destroy(")]
    assert "fbk::queue_order_knob()" in create
