// TEST-ONLY C wrapper of mitransient_amd/csrc/mtr_grad_reduce.h (the word-to-segment rule of k_grad_reduce), built by
// tests/test_grad_reduce.py with g++ alone.
#include <cstdint>

#include "../mitransient_amd/csrc/mtr_grad_reduce.h"

extern "C" {

// the segment and the offset of word i of a row whose segments hold n0, n1, n2 words
uint32_t hgr_segment(uint32_t n0, uint32_t n1, uint32_t n2, uint32_t i, uint32_t *offset)
{
    const uint32_t n[mtr::kGradSegments] = { n0, n1, n2 };
    return mtr::grad_reduce_segment(n, i, offset);
}

}
