"""The sizing and launch-shape rules of fbstab_amd/csrc/fb_launch_plan.h, restated from their description (DESIGN.md
4.6, the header's comments) and not from the header's code: tests/test_launch_plan.py checks the header against
them as tables on the CPU, tests/test_gpu_launch_plan.py what created handles report."""
import re


def knob_number(text):
    """C's atoi on the texts these tests use: optional sign and leading digits, anything else 0."""
    m = re.match(r"\s*([+-]?[0-9]+)", text or "")
    return int(m.group(1)) if m else 0


def positive_knob(text):
    """WGS_PER_CU and MAX_WORKGROUPS: a positive number applies, everything else is as good as unset."""
    return max(knob_number(text), 0)


def share_rule(resident, handles_in_flight, hw_queues):
    """tests/test_in_flight_share.py's restatement of fb_in_flight.h."""
    if handles_in_flight == 1:
        return resident
    share = -(-2 * resident // min(handles_in_flight, hw_queues))
    return min(max(1, min(share, resident)), max(1, resident // 2))


def mpc_per_cu(occupancy, handles_in_flight, hw_queues, wgs_per_cu):
    per_cu = share_rule(min(max(occupancy, 1), 8), handles_in_flight, hw_queues)
    return positive_knob(wgs_per_cu) or per_cu


def mpc_rule(cus, occupancy, handles_in_flight, hw_queues, record, qps_per_wg, max_batch, ws_doubles,
             wgs_per_cu=None, max_workgroups=None):
    """-> (workgroups, scratch_bytes) of an MPC handle."""
    workgroups = cus * mpc_per_cu(occupancy, handles_in_flight, hw_queues, wgs_per_cu)
    need = max_batch if record else -(-max_batch // qps_per_wg)
    workgroups = min(workgroups, need)
    if positive_knob(max_workgroups):
        workgroups = min(workgroups, positive_knob(max_workgroups))
    return workgroups, ws_doubles * 8 * workgroups * qps_per_wg


def dense_rule(cus, occupancy, max_batch, per_wg_doubles, wgs_per_cu=None, max_workgroups=None):
    """-> (workgroups, scratch_bytes) of a dense handle; per_wg_doubles: the wave layout's ws_doubles, k_doubles +
    v_doubles where K lives in global scratch, 0 otherwise.  (The occupancy is the query's answer held to 1..8, as
    for the MPC handles: both come from the same query.)"""
    per_cu = positive_knob(wgs_per_cu) or min(max(occupancy, 1), 8)
    workgroups = min(cus * per_cu, max_batch)
    if positive_knob(max_workgroups):
        workgroups = min(workgroups, positive_knob(max_workgroups))
    return workgroups, 8 * per_wg_doubles * workgroups


def batch_grid_rule(batch, workgroups, per_wg):
    """A batch of no more QPs than workgroups is spread, one QP per workgroup; a larger one is packed per_wg to a
    workgroup, on no more workgroups than the handle has."""
    return batch if batch <= workgroups else min(-(-batch // per_wg), workgroups)


def slots_hold_rule(batch, workgroups, qps_per_wg):
    return batch <= workgroups * qps_per_wg


def one_launch_sweep_rule(record, batch, workgroups, qps_per_wg, steps, per_step):
    return bool(record) and slots_hold_rule(batch, workgroups, qps_per_wg) and steps < 0xffff and not per_step
