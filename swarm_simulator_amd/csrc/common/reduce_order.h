// reduce_order.h -- the ORDER OF OPERATIONS of a workgroup-wide reduction of the batch QP (kernels/qp_base.inc: wave_red, block_reduce,
// block_reduce_n), stated once for the kernel and for the host restatement of tests/qp_glue/glue_main.cpp.
//
// A floating-point sum depends on the order of its additions, and the interior-point iterates follow the last bit of gap, the residual
// norms and the step lengths.  block_reduce_n reduces K values behind ONE pair of barriers; per value it must give block_reduce's bits, i.e.
// the same tree:
//   inside a wavefront  four steps inside each row of 16 lanes -- lane l combines with lane partner(step, l); after the fourth every lane
//                       of a row holds the row's result --, then (row 0 o row 1) o (row 2 o row 3);
//   across wavefronts   left to right over the wavefronts' results: ((w0 o w1) o w2) o ...
// What block_reduce_n adds is only WHERE the partial results wait between the two barriers: the reduction scratch has SLOTS doubles, value q
// of a chunk keeps its wavefronts' results in slots [q * waves, (q + 1) * waves), so a chunk holds SLOTS / waves values and K values
// take ceil(K / chunk) pairs of barriers.
#pragma once

#if defined(__HIPCC__)
#define RED_RULE __host__ __device__ inline __attribute__((always_inline))
#else
#define RED_RULE inline
#endif

namespace red_order {

constexpr int SLOTS = 16;    // doubles of reduction scratch (the first 16 of the kernel's dynamic LDS)
constexpr int ROW_STEPS = 4;
// DPP controls of the four steps: quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror
constexpr int DPP_CTRL[ROW_STEPS] = {0xB1, 0x4E, 0x141, 0x140};
// the lane whose value lane `lane` reads in step `step`
RED_RULE constexpr int partner(int step, int lane) {
    return step == 0 ? (lane ^ 1) : step == 1 ? (lane ^ 2) : step == 2 ? ((lane & ~7) | (7 - (lane & 7))) : ((lane & ~15) | (15 - (lane & 15)));
}
RED_RULE constexpr int chunk(int waves) { return SLOTS / waves; }                              // values per pair of barriers
RED_RULE constexpr int slot(int q_in_chunk, int wave, int waves) { return q_in_chunk * waves + wave; }  // where (value, wavefront) waits

}  // namespace red_order
