"""CPU test of tools/line_search_lengths.py, the model behind kCoopLineSearchTrials (fb_algorithm.h)."""
import numpy as np
import pytest

from tools import fixtures as fx
from tools import line_search_lengths as lsl
from oracle.oracle_py import default_options


def test_the_tool_counts_passes_as_the_trace_does(oracle):
    """tools/line_search_lengths.py: passes per step at K lengths per pass = sum of ceil(f / K) over the steps of
    the trace / steps, with f formed here from the records themselves."""
    p = fx.synthetic_mpc_batch(64)
    o = default_options()
    fails = []
    for b in range(p.batch):
        one = fx.MpcProblem(*p.sizes())
        one.arrays = {k: np.ascontiguousarray(a[b:b + 1]) for k, a in p.arrays.items()}
        out, rec = oracle.solve_display(one, opts=o, trace_cap=1 << 16)[4::2]
        steps = [r for r in rec if r[0] == 3 and r[1] >= 1]   # FBSTAB_TRACE_DETAILED_LINE after a step
        assert len(steps) == int(out["newton_iters"][0])
        for r in steps:
            f = 0
            t = 1.0
            while t != r[3]:   # t = beta^f by the solver's own chain of products
                t *= o.beta
                f += 1
                assert f <= o.max_linesearch_iters
            fails.append(f)
    got = lsl.fails_of_problem(oracle, p)
    assert got.tolist() == fails
    for k in lsl.KS:
        want = sum(-(-f // k) for f in fails) / float(len(fails))
        assert lsl.passes_per_step(got, k) == pytest.approx(want, rel=1e-15)
    assert lsl.passes(got, 4) > lsl.passes(got, 8) > lsl.passes(got, 12)
