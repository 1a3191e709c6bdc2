// TEST-ONLY C wrapper of mitransient_amd/csrc/mtr_flat_prims.h (index and size arithmetic of the child-ordered primitive table of
// k_fused's lean flat-walk kernels), built by tests/test_flat_prims.py with g++ alone: one top level (n_quads rectangles, n_boxes
// boxes) laid out byte by byte as the kernel stages it and as flat_prim_fetch reads it, and what went wrong handed back as counts.
// With -DHFP_MAIN it is a stand-alone program that sweeps every top level itself (the form a sanitizer build runs).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../mitransient_amd/csrc/mtr_flat_prims.h"

extern "C" {

struct hfp_out {
    uint64_t entries, bytes;
    uint64_t live;              // entries the walk can read: k < n_quads, (b, f) with b < n_boxes
    uint64_t collisions;        // bytes two entries (staged ones: every entry below `entries`) both own
    uint64_t out_of_bounds;     // entries with a byte at or past `bytes`
    uint64_t misaligned;        // records off a 16-byte boundary, first-slot words off a 4-byte one
    uint64_t unstaged;          // live entries that are not among the staged ones
    uint64_t slack;             // bytes - the last owned byte - 1
};

void hfp_check(uint32_t n_quads, uint32_t n_boxes, hfp_out *o)
{
    using namespace mtr;
    *o = hfp_out{};
    o->entries = flat_prim_entries(n_boxes);
    o->bytes = flat_prim_bytes(n_boxes);
    std::vector<uint8_t> owner(o->bytes + 4096u, 0);      // (room past the end: an overrun is counted, not performed)
    uint64_t last = 0;
    auto own = [&](uint32_t off, uint32_t len, uint32_t align) {
        if (off % align) ++o->misaligned;
        if ((uint64_t)off + len > o->bytes) ++o->out_of_bounds;
        for (uint32_t k = 0; k < len && off + k < owner.size(); ++k) {
            if (owner[off + k]) ++o->collisions;
            owner[off + k] = 1;
            if (off + k > last) last = off + k;
        }
    };
    // what the kernel stages: every entry below flat_prim_entries (dead rectangle entries are zero-filled)
    for (uint32_t e = 0; e < o->entries; ++e) {
        own(flat_prim_rec_off(e), kFlatPrimRecBytes, 16u);
        own(flat_prim_first_off(n_boxes, e), 4u, 4u);
    }
    // what the walk reads
    for (uint32_t k = 0; k < n_quads; ++k) {
        ++o->live;
        if (flat_prim_quad_entry(k) >= o->entries) ++o->unstaged;
    }
    std::vector<uint8_t> seen(o->entries + 64u, 0);
    for (uint32_t k = 0; k < n_quads; ++k) seen[flat_prim_quad_entry(k)] = 1;
    for (uint32_t b = 0; b < n_boxes; ++b)
        for (uint32_t f = 0; f < kFlatPrimFaces; ++f) {
            const uint32_t e = flat_prim_face_entry(b, f);
            ++o->live;
            if (e >= o->entries) { ++o->unstaged; continue; }
            if (seen[e]) ++o->collisions;           // two live primitives on one entry
            seen[e] = 1;
            if (e != kFlatPrimQuads + (kFlatPrimFaces * b + f)) ++o->unstaged;      // (the walk adds box_select's bit index to the rectangles' eight)
        }
    o->slack = o->bytes - last - 1u;
}

} // extern "C"

#ifdef HFP_MAIN
int main()
{
    int bad = 0;
    for (uint32_t nq = 0; nq <= 8u; ++nq)
        for (uint32_t nb = 0; nb <= 4u; ++nb) {
            hfp_out o;
            hfp_check(nq, nb, &o);
            const bool ok = !o.collisions && !o.out_of_bounds && !o.misaligned && !o.unstaged && o.live == nq + 6u * nb &&
                            o.bytes == ((84u * (8u + 6u * nb) + 15u) & ~15u) && o.slack < 16u;
            if (!ok) { printf("n_quads %u n_boxes %u: FAILED\n", nq, nb); ++bad; }
        }
    printf("%s\n", bad ? "failed" : "ok");
    return bad ? 1 : 0;
}
#endif
