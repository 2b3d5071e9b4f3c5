// request_schedule.h -- the counted wait of the block kernels' prologues, as plain constexpr functions (no HIP types: a host
// program can include this header; tests/test_request_schedule_cpu.py does, and checks every instantiated queue depth).
//
// Prologue of c3k2_fused_body / head_fused_body / conv_pair_kernel on the LDS-DMA path: a wave issues, in program order,
//   [patch LDS-DMA pieces] [per-channel constants] [the first min(D, total) blocks of its weight queue]
// and then needs the patch and the constants, not the weights. Vector-memory loads of one wave return in issue order, so
// `s_waitcnt vmcnt(N)` with N = the number of load INSTRUCTIONS issued after the last constant load waits for exactly the
// first two groups and leaves the whole weight queue in flight across the barrier.
#pragma once

namespace unina {
namespace sched {

constexpr int kVmcntMax = 63;   // s_waitcnt vmcnt is a 6-bit field on gfx9

// load instructions per weight block of a wave: one 16-byte load per lane and KiB (EltH / EltI8: 1 KiB; EltS: the 2-KiB (hi | lo) pair)
constexpr int loads_per_block(int wblk_bytes) { return wblk_bytes / 1024; }

// weight blocks the prologue requests: the queue depth, or the wave's whole sequence when that is shorter
constexpr int prologue_blocks(int depth, int total_blocks) { return depth < total_blocks ? depth : total_blocks; }

// N of the prologue's counted wait
constexpr int prologue_wait(int depth, int total_blocks, int wblk_bytes) {
  return prologue_blocks(depth, total_blocks) * loads_per_block(wblk_bytes);
}

constexpr bool prologue_wait_fits(int depth, int total_blocks, int wblk_bytes) {
  return prologue_wait(depth, total_blocks, wblk_bytes) <= kVmcntMax;
}

}  // namespace sched
}  // namespace unina
