// The grid a handle takes when it shares the device with other handles: the rule behind
// fbstab_hip_mpc_create_in_flight, as pure host functions (no HIP types: tests/test_in_flight_share.py compiles
// this header with the host compiler alone).
//
// A batch launch is a persistent grid that pulls QPs from a queue.  Alone on the device it wants every resident
// workgroup slot (`resident` per CU, the occupancy query's answer: four on the BASELINE shape, one wavefront per
// SIMD).  With several launches in flight the best measured geometry is launches x grid = TWICE the resident
// slots: the workgroups that do not fit wait, and take the SIMDs a launch frees when it runs into its tail (a
// few slow QPs, up to 73 Newton steps against a mean of 19).  Eight launches of one workgroup per CU on eight
// hardware queues are that geometry (LABNOTES R5.3, Part II "The tail").
//
// What can be resident side by side is not the number of handles but the number of LAUNCHES the runtime lets
// overlap: streams that share a hardware queue run their kernels one after the other.  So the rule counts
//     concurrent = min(handles_in_flight, hw_queues)
//     share      = ceil(2 * resident / concurrent),  clamped to [1, resident]
// and a handle that shares the device at all (handles_in_flight >= 2) keeps at most half the grid and half the
// scratch memory: share <= max(1, resident / 2).  handles_in_flight = 1 keeps `resident`.
//
//   resident = 4:   handles_in_flight  hw_queues  workgroups per CU   wavefronts wanted, all launches
//                          8               8              1                 8 x 256 = 2048
//                          8               4              2                 4 x 512 = 2048
//                          4             >= 4             2                 4 x 512 = 2048
//                          2              any             2                 2 x 512 = 1024
//                          1              any             4                     1024
//
// `hw_queues` is a HINT about how many of the caller's streams can run side by side: what the HIP runtime of
// this process was told (GPU_MAX_HW_QUEUES; HIP's own default is 4).  The library only reads it - it never sets,
// unsets or exports an environment variable, and reads no other variable of the runtime.  A caller whose streams
// share queues for other reasons (more streams than handles, other work on the device) can force a share with
// FBSTAB_HIP_WGS_PER_CU.
#pragma once
#include <cstdlib>

namespace fbk {

constexpr int kHipDefaultHwQueues = 4;
constexpr int kMaxHwQueuesHint = 32;

// workgroups per CU of one handle's launches
inline int in_flight_wgs_per_cu(int resident, int handles_in_flight, int hw_queues) {
  if (resident < 1) resident = 1;
  if (handles_in_flight <= 1) return resident;
  if (hw_queues < 1) hw_queues = 1;
  const int concurrent = handles_in_flight < hw_queues ? handles_in_flight : hw_queues;
  int share = (2 * resident + concurrent - 1) / concurrent;
  const int half = resident / 2 > 1 ? resident / 2 : 1;
  if (share > half) share = half;
  if (share > resident) share = resident;
  if (share < 1) share = 1;
  return share;
}

// the value of GPU_MAX_HW_QUEUES as text (nullptr: unset) -> the hint; 1..32, anything else is HIP's default
inline int hw_queues_hint_from(const char* text) {
  if (!text || !*text) return kHipDefaultHwQueues;
  char* end = nullptr;
  const long v = strtol(text, &end, 10);
  if (end == text || *end != '\0' || v < 1 || v > kMaxHwQueuesHint) return kHipDefaultHwQueues;
  return (int)v;
}

inline int hw_queues_hint() { return hw_queues_hint_from(getenv("GPU_MAX_HW_QUEUES")); }

}  // namespace fbk
