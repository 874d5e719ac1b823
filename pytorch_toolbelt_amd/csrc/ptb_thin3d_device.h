// The deletion rule of 3-D thinning (ptb_skeleton3d.hip, utils/skeleton.py with dims=3): "simple and not an end point" of one 26-bit
// neighbourhood code.  Written once, for the kernel and for the host entry ptb_thin3d_rule, which the CPU suite checks against a model
// that labels the 3 x 3 x 3 cube.  THE DEFINITION (Bertrand & Malandain 1994 for "simple"; the sub-field order is this library's):
//   Positions are (z, y, x); positions outside the entry are background.  The object is 26-connected, the background 6-connected.
//   N26(p), N18(p), N6(p): the usual punctured neighbourhoods of p.
//   p is SIMPLE iff the object positions of N26(p) form exactly one 26-connected component, and the background positions of N18(p) that
//     a 6-path within N18(p) joins to a background member of N6(p) form exactly one 6-connected component (so there is such a member;
//     a background position of N18(p) that no such path reaches does not count).
//   p is an END POINT iff it has exactly one object position in N26(p).  A position with none is not simple: it stays.
//   The SUBFIELD of p is (z & 1) * 4 + (y & 1) * 2 + (x & 1), coordinates within the entry: two positions of one subfield are never
//     26-adjacent.
//   One ITERATION is six DIRECTION PASSES in the order z-1, z+1, y-1, y+1, x-1, x+1.  A pass first marks its CANDIDATES from the state at
//     its start -- the object positions whose neighbour in the pass's direction is background -- and then runs eight SUB-STEPS,
//     subfield 0 to 7: sub-step f deletes every candidate of subfield f that is simple and no end point in the state before that
//     sub-step.  (Marking once per pass keeps a pass from peeling two layers.)  The decisions of a sub-step cannot see each other, so a
//     sub-step equals deleting simple points one at a time: topology is kept by construction, no order or tie rule enters the result.
//   THE SKELETON is the state after the first iteration that deletes nothing (max_iterations = n: after at most n; 0: the object), THE
//     ITERATION COUNT the number of iterations that deleted something.
// THE CODE.  The 3 x 3 x 3 cube around p as 27 bits, bit n = (dz + 1) * 9 + (dy + 1) * 3 + (dx + 1), so p is bit 13; the 26-bit code
// is the cube without bit 13 (the bits above it one place lower).
// THE FLOODS.  No adjacency table and nothing in memory: inside the cube, "26-adjacent or equal" is a dilation by one place along x, then
// y, then z, and "6-adjacent or equal" the union of the six single shifts -- shifts by 1, 3 and 9 bits with the cube's faces masked so
// that nothing wraps into the next row or slab.  A flood grows from the lowest set bit (reach = dilate(reach) & set) until it stops; the
// trips are capped by the size of the set.  One component <=> the flood reaches the whole set.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptb {

constexpr uint32_t T3_CUBE = 0x7FFFFFFu, T3_CENTRE = 1u << 13;
constexpr uint32_t T3_X0 = 0x1249249u, T3_X2 = T3_X0 << 2;                     // the faces dx = -1 and dx = +1
constexpr uint32_t T3_Y0 = 0x7u | 0x7u << 9 | 0x7u << 18, T3_Y2 = T3_Y0 << 6;  // ... dy = -1, dy = +1
constexpr uint32_t T3_TO_X2 = T3_CUBE & ~T3_X0, T3_TO_X0 = T3_CUBE & ~T3_X2;   // where a shift by +1 / -1 place along x may land: inside the cube, not wrapped into the next row
constexpr uint32_t T3_TO_Y2 = T3_CUBE & ~T3_Y0, T3_TO_Y0 = T3_CUBE & ~T3_Y2;   // ... along y: not wrapped into the next slab
constexpr uint32_t T3_N6 = 1u << 4 | 1u << 10 | 1u << 12 | 1u << 14 | 1u << 16 | 1u << 22;
constexpr uint32_t T3_CORNERS = 1u << 0 | 1u << 2 | 1u << 6 | 1u << 8 | 1u << 18 | 1u << 20 | 1u << 24 | 1u << 26;
constexpr uint32_t T3_N18 = T3_CUBE & ~T3_CORNERS & ~T3_CENTRE;
static_assert(__builtin_popcount(T3_X0) == 9 && __builtin_popcount(T3_Y0) == 9 && __builtin_popcount(T3_N18) == 18 && (T3_N6 & ~T3_N18) == 0u &&
              (T3_X2 | T3_Y2) <= T3_CUBE, "the faces, N18 and N6 of the 27-bit cube");

// the 27-bit cube of a 26-bit code, and back
__host__ __device__ inline uint32_t thin3d_cube(uint32_t code26) { return (code26 & 0x1FFFu) | (code26 >> 13 & 0x1FFFu) << 14; }
__host__ __device__ inline uint32_t thin3d_code(uint32_t cube) { return (cube & 0x1FFFu) | (cube >> 14 & 0x1FFFu) << 13; }

// every cube position within Chebyshev distance 1 of a position of r
__host__ __device__ inline uint32_t thin3d_dilate26(uint32_t r) {
    r |= (r << 1 & T3_TO_X2) | (r >> 1 & T3_TO_X0);
    r |= (r << 3 & T3_TO_Y2) | (r >> 3 & T3_TO_Y0);
    return (r | r << 9 | r >> 9) & T3_CUBE;
}
// ... that shares a face with, or is, a position of r
__host__ __device__ inline uint32_t thin3d_dilate6(uint32_t r) {
    return (r | (r << 1 & T3_TO_X2) | (r >> 1 & T3_TO_X0) | (r << 3 & T3_TO_Y2) | (r >> 3 & T3_TO_Y0) | r << 9 | r >> 9) & T3_CUBE;
}

// THE RULE: is the position with this 26-bit neighbourhood code simple and not an end point?  (The only evaluation of the definition
// in the library's native code.)
__host__ __device__ inline bool thin3d_deletable(uint32_t code26) {
    const uint32_t obj = thin3d_cube(code26);
    if ((obj & (obj - 1u)) == 0u) return false;                                // no neighbour: not simple; one: an end point
    uint32_t reach = obj & (0u - obj);
#pragma unroll 1
    for (int i = 0; i < 26; ++i) {                                             // (a trip that grows adds a position: fewer than 26 of them)
        const uint32_t grown = thin3d_dilate26(reach) & obj;
        if (grown == reach) break;
        reach = grown;
    }
    if (reach != obj) return false;
    const uint32_t bg = T3_N18 & ~obj, faces = bg & T3_N6;
    if (!faces) return false;
    reach = faces & (0u - faces);
#pragma unroll 1
    for (int i = 0; i < 18; ++i) {
        const uint32_t grown = thin3d_dilate6(reach) & bg;
        if (grown == reach) break;
        reach = grown;
    }
    return (faces & ~reach) == 0u;
}

}  // namespace ptb
