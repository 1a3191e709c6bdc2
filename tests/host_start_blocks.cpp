// TEST-ONLY program over mitransient_amd/csrc/mtr_start_blocks.h (block, size and offset arithmetic of the path-start table of
// k_fused's lean flat-walk kernels), built by tests/test_start_blocks.py with g++ alone under AddressSanitizer and UBSan: every
// wave of a grid writes its 64 records into a table of exactly start_table_bytes bytes — a record that left the table, or two that
// shared a byte, is a sanitizer report or a count below — and every ticket length is cut into blocks.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../mitransient_amd/csrc/mtr_start_blocks.h"

int main()
{
    using namespace mtr;
    const uint32_t waves = 4;
    for (uint32_t grid : { 1u, 2u, 3u, 7u, 64u, 255u, 1024u }) {
        const size_t bytes = start_table_bytes(grid, waves);
        std::vector<unsigned char> tab(bytes, 0);
        for (uint32_t wg = 0; wg < grid; ++wg) for (uint32_t w = 0; w < waves; ++w) for (uint32_t e = 0; e < kStartBlock; ++e) {
            unsigned char *rec = tab.data() + start_rec_off(wg, waves, w, e);
            for (uint32_t b = 0; b < kStartRecBytes; ++b) { if (rec[b]) { printf("overlap at grid %u wg %u wave %u entry %u\n", grid, wg, w, e); return 1; } rec[b] = 1; }
        }
        for (size_t b = 0; b < bytes; ++b) if (!tab[b]) { printf("byte %zu of grid %u belongs to no record\n", b, grid); return 1; }
        // the context's slots: stride from the allocation; a table of this grid in every slot stays inside the allocation and its slot
        const size_t cap = start_alloc_bytes(bytes), stride = start_slot_stride(cap);
        for (uint32_t s = 0; s < kStartSlots; ++s)
            if (stride < bytes || start_slot_off(stride, s) + bytes > cap || (s && start_slot_off(stride, s - 1u) + bytes > start_slot_off(stride, s))) { printf("slot %u of grid %u\n", s, grid); return 1; }
    }
    for (uint32_t n = 1; n <= 65537u; ++n) {
        const uint32_t nb = start_blocks(n);
        uint64_t sum = 0;
        for (uint32_t b = 0; b < nb; ++b) sum += start_block_entries(n, b * kStartBlock);
        if (sum != n || start_last_entries(n) != start_block_entries(n, (nb - 1u) * kStartBlock) || start_block_entries(n, nb * kStartBlock)) { printf("blocks of %u\n", n); return 1; }
    }
    printf("ok\n");
    return 0;
}
