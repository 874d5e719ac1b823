// The deletion rule of parallel thinning (ptb_skeleton.hip, utils/skeleton.py) on WORDS: bit i of every word is one position, so one
// evaluation decides 32 positions.  Written once, for the kernels and for the host entry ptb_thin_rule, which the CPU suite checks
// against the formulae on all 256 neighbourhoods.
// THE NEIGHBOURS of a position P1 = (y, x), in the order of the array nbr[8]:
//     P2 (y-1, x)   P3 (y-1, x+1)   P4 (y, x+1)   P5 (y+1, x+1)   P6 (y+1, x)   P7 (y+1, x-1)   P8 (y, x-1)   P9 (y-1, x-1)
// Positions outside the entry are background.  One ITERATION is sub-iteration 0, then sub-iteration 1; each is synchronous (every
// decision reads the state from before it).  An object position is deleted in sub-iteration k iff
//   ZHANG (Zhang & Suen 1984): with B the number of set neighbours and A the number of i with P_i = 0 and P_i+1 = 1 in the cycle
//     P2, P3, ..., P9, P2:   2 <= B <= 6 and A == 1 and
//     k = 0: P2 P4 P6 == 0 and P4 P6 P8 == 0;      k = 1: P2 P4 P8 == 0 and P2 P6 P8 == 0.
//   GUO_HALL (Guo & Hall 1989, as in OpenCV's ximgproc.thinning): with
//     C  = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2)),
//     N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8),   N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9),   N = min(N1, N2),
//     m  = (P6|P7|!P9) & P8 for k = 0,   (P2|P3|!P5) & P4 for k = 1:   C == 1 and 2 <= N <= 3 and m == 0.
// The counts are bit-sliced: adders over words give the bits of B, N1 and N2 for 32 positions at once, "exactly one of" gives A == 1
// and C == 1.  No table, no per-position branch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ptb {

enum { THIN_ZHANG = 0, THIN_GUO_HALL = 1 };     // PTB_THIN_*

struct ThinSum {                // one bit of a sum and its carry
    uint32_t s, c;
};
__host__ __device__ inline ThinSum thin_add(uint32_t a, uint32_t b) { return {a ^ b, a & b}; }
__host__ __device__ inline ThinSum thin_add(uint32_t a, uint32_t b, uint32_t c) { return {a ^ b ^ c, (a & b) | (c & (a ^ b))}; }

// where exactly one of the words t[0 .. n) is set
template <int n>
__host__ __device__ inline uint32_t thin_exactly_one(const uint32_t (&t)[n]) {
    uint32_t ones = 0u, more = 0u;
#pragma unroll
    for (int i = 0; i < n; ++i) {
        more |= ones & t[i];
        ones |= t[i];
    }
    return ones & ~more;
}

// the sum of four one-bit words: bit 1 | bit 2 in `two_up` (the sum is >= 2), bit 2 in `four` (it is 4)
__host__ __device__ inline void thin_sum4(uint32_t a, uint32_t b, uint32_t c, uint32_t d, uint32_t& two_up, uint32_t& four) {
    const ThinSum x = thin_add(a, b, c), y = thin_add(x.s, d);
    two_up = x.c | y.c;
    four = x.c & y.c;
}

// The positions of `centre` that sub-iteration `sub` (0 | 1) of METHOD deletes: nbr[0 .. 8) = the words of P2 .. P9.
template <int METHOD>
__host__ __device__ inline uint32_t thin_rule(int sub, const uint32_t (&nbr)[8], uint32_t centre) {
    const uint32_t P2 = nbr[0], P3 = nbr[1], P4 = nbr[2], P5 = nbr[3], P6 = nbr[4], P7 = nbr[5], P8 = nbr[6], P9 = nbr[7];
    if (METHOD == THIN_ZHANG) {
        // B = b0 + 2 b1 + 4 b2 + 8 b3: three adders of weight 1, two of weight 2, one of weight 4
        const ThinSum s1 = thin_add(P2, P3, P4), s2 = thin_add(P5, P6, P7), s3 = thin_add(P8, P9);
        const ThinSum w1 = thin_add(s1.s, s2.s, s3.s);
        const ThinSum t1 = thin_add(s1.c, s2.c, s3.c), t2 = thin_add(t1.s, w1.c);
        const uint32_t b0 = w1.s, b1 = t2.s, b2 = t1.c ^ t2.c, b3 = t1.c & t2.c;
        const uint32_t b_ok = (b1 | b2 | b3) & ~b3 & ~(b2 & b1 & b0);                     // 2 <= B, B != 8, B != 7
        const uint32_t t[8] = {~P2 & P3, ~P3 & P4, ~P4 & P5, ~P5 & P6, ~P6 & P7, ~P7 & P8, ~P8 & P9, ~P9 & P2};
        const uint32_t side = sub == 0 ? ~(P2 & P4 & P6) & ~(P4 & P6 & P8) : ~(P2 & P4 & P8) & ~(P2 & P6 & P8);
        return centre & b_ok & thin_exactly_one(t) & side;
    } else {
        const uint32_t q[4] = {~P2 & (P3 | P4), ~P4 & (P5 | P6), ~P6 & (P7 | P8), ~P8 & (P9 | P2)};
        uint32_t up1, four1, up2, four2;
        thin_sum4(P9 | P2, P3 | P4, P5 | P6, P7 | P8, up1, four1);
        thin_sum4(P2 | P3, P4 | P5, P6 | P7, P8 | P9, up2, four2);
        const uint32_t n_ok = up1 & up2 & ~(four1 & four2);                               // min(N1, N2) >= 2, and not both 4
        const uint32_t m = sub == 0 ? (P6 | P7 | ~P9) & P8 : (P2 | P3 | ~P5) & P4;
        return centre & thin_exactly_one(q) & n_ok & ~m;
    }
}

// the words of the eight neighbours of the positions of `c`, from the 3 x 3 words around it: (ul u ur / l c r / dl d dr)
__host__ __device__ inline void thin_neighbours(uint32_t ul, uint32_t u, uint32_t ur, uint32_t l, uint32_t c, uint32_t r, uint32_t dl, uint32_t d, uint32_t dr,
                                                uint32_t (&nbr)[8]) {
    nbr[0] = u;                                 // bit i of a word is column 32 w + i: the column to the right is one bit up
    nbr[1] = (u >> 1) | (ur << 31);
    nbr[2] = (c >> 1) | (r << 31);
    nbr[3] = (d >> 1) | (dr << 31);
    nbr[4] = d;
    nbr[5] = (d << 1) | (dl >> 31);
    nbr[6] = (c << 1) | (l >> 31);
    nbr[7] = (u << 1) | (ul >> 31);
}

}  // namespace ptb
