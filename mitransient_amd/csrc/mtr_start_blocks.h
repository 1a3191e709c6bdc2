// mtr_start_blocks.h — the PATH-START TABLE of k_fused's lean flat-walk kernels (mtr_kernels.hip: START BLOCKS) as index and size
// arithmetic.  No HIP include: tests/host_start_blocks.cpp compiles it alone (tests/test_start_blocks.py), the library sweeps it
// through mtr_test_start_blocks.
//
// A wave of such a kernel takes the sample indices of a work ticket in BLOCKS of 64 consecutive ones and computes the 64 path starts
// of a block in one full-width pass (path_begin), one record per entry, into its own 64 records of a table in global memory; a lane
// whose path has ended takes the next entry of its wave's block and reads that record.  Nothing is shared between waves:
//   record (workgroup g, wave w, entry e)     at ((g * waves + w) * 64 + e) * 48 bytes
//   record                                    ray origin (3 words), direction (3), tmax, PCG32 state (2), increment (2), one unused
// One table per launch slot (the context rotates kStartSlots of them with its ticket counters), all in ONE allocation (below).
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define MTR_SB_HD __host__ __device__ constexpr
#else
#define MTR_SB_HD constexpr
#endif

namespace mtr {

constexpr uint32_t kStartBlock = 64;            // entries of a block: the lanes of a wave
constexpr uint32_t kStartRecBytes = 48;         // three 16-byte words per record
constexpr uint32_t kStartSlots = 16;            // tables of a context (mtr_api.hip: d_ticket's rotation)
constexpr uint32_t kStartFresh = 2u * kStartBlock;     // "entries handed out" of a block that is assigned but not computed yet (ticket entry)

// blocks of a ticket of n_lanes samples, and the entries of the last one (the others hold kStartBlock)
MTR_SB_HD uint32_t start_blocks(uint32_t n_lanes) { return n_lanes / kStartBlock + (n_lanes % kStartBlock ? 1u : 0u); }
MTR_SB_HD uint32_t start_last_entries(uint32_t n_lanes) { return n_lanes ? n_lanes - kStartBlock * (start_blocks(n_lanes) - 1u) : 0u; }
// entries of the block that starts at sample index `base` (a multiple of kStartBlock; 0 at or beyond the ticket's end)
MTR_SB_HD uint32_t start_block_entries(uint32_t n_lanes, uint32_t base) { return base >= n_lanes ? 0u : (n_lanes - base < kStartBlock ? n_lanes - base : kStartBlock); }
// what the context allocates per launch slot and the kernel indexes: the same functions
MTR_SB_HD size_t start_table_bytes(uint32_t grid, uint32_t waves) { return (size_t)grid * waves * kStartBlock * kStartRecBytes; }
MTR_SB_HD size_t start_rec_off(uint32_t wg, uint32_t waves, uint32_t wave, uint32_t entry) { return (((size_t)wg * waves + wave) * kStartBlock + entry) * kStartRecBytes; }
// The context's kStartSlots tables share one allocation.  Their STRIDE is a function of the allocation alone, never of a launch: two
// launches in flight with different grids (two streams) then use disjoint tables whatever their sizes.  The context allocates
// start_alloc_bytes(largest table so far) and re-allocates — after draining — only when a launch's table exceeds the stride.
MTR_SB_HD size_t start_alloc_bytes(size_t table_bytes) { return ((table_bytes + 15u) & ~(size_t)15u) * kStartSlots; }
MTR_SB_HD size_t start_slot_stride(size_t alloc_bytes) { return (alloc_bytes / kStartSlots) & ~(size_t)15u; }
MTR_SB_HD size_t start_slot_off(size_t stride, uint32_t slot) { return stride * slot; }

} // namespace mtr
