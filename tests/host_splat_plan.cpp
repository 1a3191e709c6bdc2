// TEST-ONLY C wrapper of mitransient_amd/csrc/mtr_splat_plan.h (the host arithmetic of mtr_splat_add's partition path),
// built by tests/test_splat_plan.py with g++ alone: one plan, and a sweep over a range of pixel counts that checks in C++
// what the kernels of mtr_splat.hip need from the plan and hands back a summary.
#include <cstdint>

#include "../mitransient_amd/csrc/mtr_splat_plan.h"

extern "C" {

struct hsp_plan_out {
    uint64_t supported, bits_pix, bits_lo, n_lo, n_hi;
    uint64_t rec_a, rec_b, hist_hi, base_hi, starts, cur_lo, block_sums;
    uint64_t n_scan, total_bytes;
};

void hsp_plan(uint32_t width, uint32_t height, uint32_t bins, uint32_t n_freq, uint64_t n, hsp_plan_out *o)
{
    const mtr::SplatPlan p = mtr::splat_partition_plan(width, height, bins, n_freq, n);
    o->supported = p.supported ? 1u : 0u;
    o->bits_pix = p.bits_pix; o->bits_lo = p.bits_lo; o->n_lo = p.n_lo; o->n_hi = p.n_hi;
    o->rec_a = p.rec_a; o->rec_b = p.rec_b; o->hist_hi = p.hist_hi; o->base_hi = p.base_hi;
    o->starts = p.starts; o->cur_lo = p.cur_lo; o->block_sums = p.block_sums;
    o->n_scan = p.n_scan; o->total_bytes = p.total_bytes;
}

// the first pixel count (0: none) at which each property fails, and the extremes over the range
struct hsp_sweep_out {
    uint64_t checked;
    uint64_t bad_supported;      // not supported (bins and n are chosen so that every film of the range should be)
    uint64_t bad_digits;         // n_lo > 2048, n_hi > 2048, n_lo != 1 << bits_lo, or n_hi * n_lo < npix, or (n_hi - 1) * n_lo >= npix
    uint64_t bad_bits;           // 1 << bits_pix < npix, or 1 << (bits_pix - 1) >= npix (npix > 2)
    uint64_t bad_layout;         // a region overlaps the next, leaves total_bytes, or is misaligned
    uint64_t bad_scan;           // n_scan blocks of 4096 do not cover npix + 1 entries, or more block sums than reserved slots
    uint64_t max_n_lo, max_n_hi, max_n_scan;
    uint64_t min_spare_words;    // smallest (total_bytes - end of the block sums) / 4
    uint64_t max_spare_words;
};

void hsp_sweep(uint64_t npix_first, uint64_t npix_last, uint32_t bins, uint64_t n, hsp_sweep_out *o)
{
    *o = hsp_sweep_out{};
    o->min_spare_words = ~0ull;
    auto flag = [](uint64_t &slot, uint64_t npix) { if (!slot) slot = npix; };
    for (uint64_t npix = npix_first; npix <= npix_last; ++npix) {
        const mtr::SplatPlan p = mtr::splat_partition_plan((uint32_t)npix, 1u, bins, 0u, n);
        ++o->checked;
        if (!p.supported) flag(o->bad_supported, npix);
        if (p.n_lo > 2048u || p.n_hi > 2048u || p.n_lo != (1ull << p.bits_lo) || (uint64_t)p.n_hi * p.n_lo < npix
            || (uint64_t)(p.n_hi - 1u) * p.n_lo >= npix)
            flag(o->bad_digits, npix);
        if ((1ull << p.bits_pix) < npix || (npix > 2 && (1ull << (p.bits_pix - 1u)) >= npix)) flag(o->bad_bits, npix);
        // what the kernels and the two memsets of launch_splat_partitioned touch, in bytes, in the order of the layout
        const uint64_t begin[7] = {p.rec_a, p.rec_b, p.hist_hi, p.base_hi, p.starts, p.cur_lo, p.block_sums};
        const uint64_t bytes[7] = {n * 16u, n * 16u, 2048u * 4u /* memset */, ((uint64_t)p.n_hi + 1u) * 4u, (npix + 16u) * 4u /* memset */,
                                   npix * 4u, (uint64_t)p.n_scan * 4u};
        const uint64_t align[7] = {16u, 16u, 4u, 4u, 4u, 4u, 4u};
        bool ok = p.rec_a == 0u;
        for (int k = 0; k < 7; ++k) {
            const uint64_t end = begin[k] + bytes[k];
            ok = ok && begin[k] % align[k] == 0u && end <= (k < 6 ? begin[k + 1] : (uint64_t)p.total_bytes);
        }
        if (!ok) flag(o->bad_layout, npix);
        // the pixel cursors are addressed as cur_lo + (hi << bits_lo) + digit, digit < n_lo: the last bucket's claims of EMPTY
        // digits are skipped (count 0), so only digits of real pixels are touched — nothing to reserve past npix
        const uint64_t slots = ((uint64_t)p.total_bytes - p.block_sums) / 4u;
        if ((uint64_t)p.n_scan * 4096u < npix + 1u || p.n_scan > slots) flag(o->bad_scan, npix);
        if (p.n_lo > o->max_n_lo) o->max_n_lo = p.n_lo;
        if (p.n_hi > o->max_n_hi) o->max_n_hi = p.n_hi;
        if (p.n_scan > o->max_n_scan) o->max_n_scan = p.n_scan;
        const uint64_t spare = slots >= p.n_scan ? slots - p.n_scan : 0u;
        if (spare < o->min_spare_words) o->min_spare_words = spare;
        if (spare > o->max_spare_words) o->max_spare_words = spare;
    }
}

} // extern "C"
