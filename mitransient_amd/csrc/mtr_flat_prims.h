// mtr_flat_prims.h — the CHILD-ORDERED PRIMITIVE TABLE of k_fused's lean flat-walk kernels (mtr_core.h: flat_walk_device,
// mtr_kernels.hip: the staging and fused_plan) as index and size arithmetic.  No HIP include: tests/host_flat_prims.cpp compiles it
// alone and sweeps it over every top level a FlatTop can describe (tests/test_flat_prims.py).
//
// The table is a COPY, per workgroup, of the intersection records the flat walk tests, ordered by what the walk holds in a register
// when it wants one — the child index of the root's slab stage, the face bit of box_select — so that a record's address no longer
// has to be loaded (WNode::ref[k]) before the record is:
//   entry k, k < 8                 the TriPair of the rectangle that is child k of the root (filled for k < n_quads)
//   entry 8 + 6 b + f              the TriPair of face f of box b (b < n_boxes <= 4)
// The records (80 B each, 16-byte aligned) come first, then one word per entry: the `first` slot the primitive tests report as
// Hit::prim, which they derived from the reference before.  The table lies directly IN FRONT of the staged tree, so its address
// follows from the tree's and the header's box count: no pointer of its own rides through the persistent loop.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define MTR_FP_HD __host__ __device__ constexpr
#else
#define MTR_FP_HD constexpr
#endif

namespace mtr {

constexpr uint32_t kFlatPrimQuads = 8;          // entries reserved for the root's children (kWide)
constexpr uint32_t kFlatPrimFaces = 6;          // entries per box
constexpr uint32_t kFlatPrimRecBytes = 80;      // sizeof(TriPair)
constexpr uint32_t kFlatPrimEntryBytes = kFlatPrimRecBytes + 4u;

MTR_FP_HD uint32_t flat_prim_entries(uint32_t n_boxes) { return kFlatPrimQuads + kFlatPrimFaces * n_boxes; }
MTR_FP_HD uint32_t flat_prim_quad_entry(uint32_t k) { return k; }
// (box_select's bit 6 b + f IS the entry, less the rectangles' eight)
MTR_FP_HD uint32_t flat_prim_face_entry(uint32_t b, uint32_t f) { return kFlatPrimQuads + kFlatPrimFaces * b + f; }
// byte offsets from the table's first byte
MTR_FP_HD uint32_t flat_prim_rec_off(uint32_t entry) { return kFlatPrimRecBytes * entry; }
MTR_FP_HD uint32_t flat_prim_first_off(uint32_t n_boxes, uint32_t entry) { return kFlatPrimRecBytes * flat_prim_entries(n_boxes) + 4u * entry; }
// what fused_plan reserves and the kernel carves: the same function
MTR_FP_HD uint32_t flat_prim_bytes(uint32_t n_boxes) { return (kFlatPrimEntryBytes * flat_prim_entries(n_boxes) + 15u) & ~15u; }

} // namespace mtr
