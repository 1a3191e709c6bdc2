// mtr_splat_plan.h — the PLAN of the partition path of mtr_splat_add (mtr_splat.hip) as host arithmetic: whether a call can
// be partitioned, how the pixel index is split into two digits, and where each region of the workspace lies.  No HIP
// include: tests/host_splat_plan.cpp compiles it alone and sweeps it over every film size (tests/test_splat_plan.py).
// splat_partition_supported, splat_partition_scratch_bytes and launch_splat_partitioned read the plan and nothing else.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mtr {

constexpr uint32_t kSplatPlanMaxDigits = 2048;        // LDS counters per tile (11 bits per half: films up to 2^22 pixels)
constexpr uint32_t kSplatPlanScanBlock = 4096;        // entries of the run-start table one workgroup scans (k_part_scan_lo)
constexpr uint64_t kSplatPlanMaxPixels = 1ull << 22;

struct SplatPlan {
    bool supported;                 // the partition path can take this call (else: the f32 atomics)
    uint32_t bits_pix;              // bits of a pixel id; the record key is pixel | bin << bits_pix
    uint32_t bits_lo, n_lo, n_hi;   // low digit = pixel & (n_lo - 1), high digit = pixel >> bits_lo < n_hi
    // byte offsets into the workspace
    size_t rec_a, rec_b;            // [n] 16-byte records each
    size_t hist_hi;                 // u32 [kSplatPlanMaxDigits]
    size_t base_hi;                 // u32 [kSplatPlanMaxDigits + 16]
    size_t starts;                  // u32 [npix + 16]
    size_t cur_lo;                  // u32 [npix + 16]
    size_t block_sums;              // u32 [n_scan]
    uint32_t n_scan;                // workgroups of the run-start scan = block sums written
    size_t total_bytes;             // what the caller allocates
};

inline SplatPlan splat_partition_plan(uint32_t width, uint32_t height, uint32_t bins, uint32_t n_freq, uint64_t n)
{
    SplatPlan p{};
    const uint64_t npix = (uint64_t)width * height;
    p.total_bytes = 2 * (size_t)n * 16u + (2 * (size_t)kSplatPlanMaxDigits + 2 * (size_t)npix + (size_t)npix / kSplatPlanScanBlock + 128) * 4u;
    if (npix < 2 || npix > (1ull << 31)) return p;          // (no digits to speak of / past 32-bit pixel ids: never supported)
    p.bits_pix = 1; while ((1ull << p.bits_pix) < npix) ++p.bits_pix;
    // (an 8 + 10 bit split — fewer cursors for the first scatter's same-address claims, 64-byte runs in the second — measured
    // the same as 9 + 9: 12.3 against 12.4 ms for 2^28; the claims are not what bounds the scatters)
    p.bits_lo = p.bits_pix / 2u;
    p.n_lo = 1u << p.bits_lo;
    p.n_hi = (uint32_t)((npix - 1u) >> p.bits_lo) + 1u;
    size_t o = 0;
    p.rec_a = o; o += (size_t)n * 16u;
    p.rec_b = o; o += (size_t)n * 16u;
    p.hist_hi = o; o += (size_t)kSplatPlanMaxDigits * 4u;
    p.base_hi = o; o += ((size_t)kSplatPlanMaxDigits + 16u) * 4u;
    p.starts = o; o += ((size_t)npix + 16u) * 4u;
    p.cur_lo = o; o += ((size_t)npix + 16u) * 4u;
    p.block_sums = o;
    p.n_scan = (uint32_t)((npix + 1u + kSplatPlanScanBlock - 1u) / kSplatPlanScanBlock);            // <= 1025 (films up to 2^22 pixels)
    // (record key = pixel | bin << bits_pix in 32 bits; LDS counters for either half)
    if (n_freq || n == 0 || n >= 0xffffffffull || npix > kSplatPlanMaxPixels) return p;
    uint32_t bits_bin = 1; while ((1ull << bits_bin) < bins) ++bits_bin;
    if (p.bits_pix + bits_bin > 32u) return p;
    // the record key pixel | bin << bits_pix shares its value space with the sentinel kDropped = 0xffffffff: when both counts are
    // exact powers of two that fill the 32 bits, the last pixel's last bin WOULD be that key and its contribution would vanish
    if (p.bits_pix + bits_bin == 32u && (((uint64_t)(bins - 1u) << p.bits_pix) | (npix - 1u)) == 0xffffffffull) return p;
    p.supported = (size_t)bins * 12u <= 150u * 1024u;             // the row must fit LDS
    return p;
}

} // namespace mtr
