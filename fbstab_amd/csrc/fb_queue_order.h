// The queue order of a record handle (fb_queue_order_plan.h has the rule and the reasons): behind a packed batch
// solve, ONE workgroup sorts the QP indices of the batch by the Newton counts the solve has just written,
// descending, and the next solve of the same batch hands them out in that order (R16Queue::fetch,
// fb_record_kernel.h).
//
// A counting sort on newton_iters clamped to [0, 255], stable by index inside a count, with no atomic anywhere:
// the same counts give the same order.  The four wavefronts of the workgroup take the four quarters of the batch
// (chunks, in index order) and walk them in tiles of 64.  Sweep 1 counts the chunk's population of every bin.  The
// prefix runs over the bins from 255 down and, inside a bin, over the chunks upwards, and gives every chunk the
// place of its first index of every count.  Sweep 2 places: a lane's index goes to the running place of its bin
// plus the number of lower lanes of the tile with the same count, and the running place moves on by the tile's
// population of the bin.  Both sweeps find the populations by ballot, one distinct count of the tile at a time, so
// every index is written exactly once and the places of a bin ascend with the index.
//
// What the kernel may cost is set by what runs beside it.  The record launches of the other streams of a caller
// with several handles in flight hold every SIMD at 496 of 512 registers and - four workgroups of 40,128 bytes, 32
// granules of 1280 each - ALL of a CU's LDS for as long as they run, and a kernel that does not fit into the rest
// waits for a workgroup of theirs to end, with the next solve of its stream queued behind it (LABNOTES R6.3; R7.1:
// a first version with 2 KB of LDS took 185 us alone and 12 ms in flight).  Hence four wavefronts (one per SIMD) of
// at most 16 registers and NO LDS: a chunk's 256 counters live in four registers of its wavefront (bin k in lane
// k mod 64 of register k / 64, read and written by the wavefront's scalar side), and the chunks meet once, through
// 4 x 256 ints of global memory behind the order.
#pragma once
#include "fb_common.h"
#include "fb_queue_order_plan.h"

namespace fbk {

constexpr int kQueueOrderThreads = 256;
constexpr int kQueueOrderChunks = kQueueOrderThreads / 64;
constexpr int kQueueOrderBins = 256;
constexpr int kQueueOrderRegs = kQueueOrderBins / 64;
// ints of the handle's order buffer: the order, and the chunks' counters behind it
inline size_t queue_order_ints(int max_batch) { return (size_t)max_batch + kQueueOrderChunks * kQueueOrderBins; }

// the sort key of QP i, and -1 for a lane beyond its chunk (no bin: it matches no count of the tile)
__device__ __forceinline__ int queue_order_key(const fbstab_solver_out_t* out, int i, int end) {
  if (i >= end) return -1;
  const int n = out[i].newton_iters;
  return n < 0 ? 0 : n > kQueueOrderBins - 1 ? kQueueOrderBins - 1 : n;
}

// counter of bin k (wavefront-uniform) += n / its value, in every lane
__device__ __forceinline__ void queue_order_add(int (&cnt)[kQueueOrderRegs], int k, int n, int lane) {
#pragma unroll
  for (int r = 0; r < kQueueOrderRegs; r++) cnt[r] += (r == (k >> 6) && lane == (k & 63)) ? n : 0;
}
__device__ __forceinline__ int queue_order_get(const int (&cnt)[kQueueOrderRegs], int k) {
  int at = 0;
#pragma unroll
  for (int r = 0; r < kQueueOrderRegs; r++) {
    const int v = __builtin_amdgcn_readlane(cnt[r], k & 63);
    at = r == (k >> 6) ? v : at;
  }
  return at;
}

// out: the SolverOut block of the solve that has just run on this stream; order: [batch] ints, all written;
// hist: [kQueueOrderChunks][kQueueOrderBins] ints of scratch (queue_order_ints).
// (amdgpu_num_vgpr counts in units of two registers here, as FB_R16_REG_CAP of fb_record_kernel.h does: 8 = 16.)
__global__ __launch_bounds__(kQueueOrderThreads) __attribute__((amdgpu_num_vgpr(8))) void fbstab_mpc_queue_order_kernel(const fbstab_solver_out_t* out,
                                                                                    int batch, int* order, int* hist) {
  if (batch < 1) return;
  // (the chunk is the wavefront's, and so are its bounds: scalar registers)
  const int lane = threadIdx.x & 63, chunk = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int len = (batch + kQueueOrderChunks - 1) / kQueueOrderChunks;
  const int begin = chunk * len < batch ? chunk * len : batch, end = begin + len < batch ? begin + len : batch;
  int cnt[kQueueOrderRegs] = {0, 0, 0, 0};

  // sweep 1: the chunk's population of every bin
  for (int base = begin; base < end; base += 64) {
    const int key = queue_order_key(out, base + lane, end);
    unsigned long long todo = __ballot(key >= 0);
    while (todo != 0ull) {
      const int k = __builtin_amdgcn_readlane(key, __ffsll((long long)todo) - 1);
      const unsigned long long same = __ballot(key == k);
      queue_order_add(cnt, k, __popcll(same), lane);
      todo &= ~same;
    }
  }
#pragma unroll
  for (int r = 0; r < kQueueOrderRegs; r++) hist[(unsigned)(chunk * kQueueOrderBins + r * 64 + lane)] = cnt[r];
  __syncthreads();  // (the chunks' counters are read by the other wavefronts of the workgroup)

  // prefix: the lane that holds bin k = 64 r + lane sums what stands in front of this chunk's indices of count k -
  // every index of a higher count (registers above r, and the higher lanes of register r), and the lower chunks'
  // indices of count k
  int above = 0;
#pragma nounroll
  for (int r = kQueueOrderRegs - 1; r >= 0; r--) {  // (rolled, like the loops inside: the kernel has 16 registers)
    int total = 0, lower = 0;
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (int c = 0; c < kQueueOrderChunks; c++) {
      // (a volatile load: one at a time, so that the loop stays as it is written - two registers, not eight)
      const int n = static_cast<const volatile int*>(hist)[(unsigned)(c * kQueueOrderBins + r * 64 + lane)];
      total += n;
      lower += c < chunk ? n : 0;
    }
    int from = total;  // sum over this lane and the higher ones
#pragma nounroll
    for (int d = 1; d < 64; d <<= 1) {
      const int v = __shfl_down(from, d, 64);
      from += lane + d < 64 ? v : 0;
    }
    const int place = above + from - total + lower;
#pragma unroll
    for (int q = 0; q < kQueueOrderRegs; q++) cnt[q] = q == r ? place : cnt[q];
    above += __builtin_amdgcn_readlane(from, 0);
  }

  // sweep 2: every index to its place.  (The keys are read a second time: were `out` to change in between - it
  // does not, the stream orders its writers - a place could leave the batch, so the store checks it.)
  for (int base = begin; base < end; base += 64) {
    const int key = queue_order_key(out, base + lane, end);
    unsigned long long todo = __ballot(key >= 0);
    while (todo != 0ull) {
      const int k = __builtin_amdgcn_readlane(key, __ffsll((long long)todo) - 1);
      const unsigned long long same = __ballot(key == k);
      const int at = queue_order_get(cnt, k);
      if (key == k) {
        const int place =
            at + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(same >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)same, 0u));
        if (place >= 0 && place < batch) order[place] = base + lane;
      }
      queue_order_add(cnt, k, __popcll(same), lane);
      todo &= ~same;
    }
  }
}

}  // namespace fbk
