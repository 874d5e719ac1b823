// The soft skeleton and the soft-clDice training loss with its gradient (losses/cldice.py, utils/softskel.py; the reference has no
// counterpart; Shit et al., CVPR 2021).  The definitions stand in include/ptb_hip.h: E = the minimum over a position and its 4 edge
// neighbours, D = the maximum over the 3 x 3 window, positions outside the plane never take part; v_0 = x, v_j+1 = E(v_j), o_j = D(v_j+1),
// delta_j = relu(v_j - o_j), S_j = S_j-1 + relu(delta_j - S_j-1 delta_j), softskel_k = S_k.  A value depends on x within R = k + 2.
// THE STENCIL IS BLOCKED IN TIME IN LDS.  A workgroup owns a square tile and holds it with a halo as a PLANE: rows of LP floats with a ring
// of one cell around; a cell outside the image, and the ring, holds +inf.  +inf is "takes no part": E leaves such a cell at +inf (so it
// stays one through every stage) and reads its neighbours only at a finite centre -- the ring keeps every read inside the plane without a
// coordinate test --, a minimum ignores it, and D reads it as -inf.  A wrong value at the rim of the halo travels one cell per E or D,
// so with a halo of R the owned cells are exact after the k + 1 stages.  The halo of an instance is its largest R whatever k the call
// names: the geometry is a compile-time constant, k only bounds the stage loop.
//   1. ss_fwd_kernel   a workgroup per (class, batch entry, 32 x 32 tile).  Activation on load (a softmax reads the C logits of a cell),
//                      then the stages on two rolling planes -- v_j and v_j+1; o_j is evaluated where it is used -- with S in the registers
//                      of the lane that owns the position (4 a lane).  The same again for the target plane.  Writes ST [B, K, S] and the
//                      four sums of the tile in float64 to ITS OWN slot; the soft_skeleton instance writes S alone.
//   2. ss_finish_kernel  one workgroup adds the slots of every class in index order, evaluates the scalar tail and the coefficients
//                      a = dloss/d sum(SP g), b = dloss/d sum(SP), c = dloss/d sum(ST p), each already divided by K.
//   3. ss_bwd_kernel   THE EXACT ADJOINT IN GATHER FORM, no atomics.  The upstream on SP is w = a g + b.  Per position, descending in j:
//                        m_j = [delta_j - S_j-1 delta_j > 0],  g_delta_j = m_j gS_j (1 - S_j-1),  gS_j-1 = gS_j (1 - m_j delta_j),
//                        direct_j = [v_j > o_j] g_delta_j,  go_j = -direct_j,
//                        gv_j+1 = direct_j+1 + D^T(go_j) + E^T(gv_j+2)   (both selections over v_j+1),   gv_0 = direct_0 + E^T(gv_1).
//                      A window passes its adjoint to the ONE position it selects: the first in row-major window order among equal
//                      values (E: up, left, centre, right, down).  D^T and E^T are evaluated at the RECEIVING position p: every cell q
//                      keeps the index its two windows select in a byte plane, and p adds the adjoint of each neighbour q whose byte
//                      names p.  The tile recomputes the forward on the tile + 2 R and carries adjoints on the tile + R.  LDS plan, a
//                      constant number of planes: the probabilities, two rolling v, go, gv and the selection bytes; stage j recomputes
//                      v_j, v_j+1 and S_j-1 from the probabilities (j + 1 erosions: O(k^2) cheap LDS steps); gS and direct_j+1 stay in the
//                      registers of the lane that owns the cell.  Writes dloss/dp + c ST for its interior, [B, K, S].
//   4. ss_act_bwd_kernel  a streaming pass over those planes: the activation's Jacobian (a softmax needs all C probabilities of a
//                      position), times the upstream scalar read on the device; writes grad [B, C, S], zeros in unselected channels of a
//                      sigmoid / identity.
// Every sum is added in a fixed order and the grids depend on the shape and k alone: a second run gives the same bits.  No workgroup waits
// for another one; every loop is bounded by k, C, K or a plane.  THE CAP: 1 <= iterations <= 8, from the backward's LDS plan -- instances
// (tile side, largest R): (32, 5) for k <= 3, (24, 7) for k <= 5, (16, 10) for k <= 8, each under 53 KiB so that three workgroups share a CU.
#include <algorithm>
#include <cmath>

#include "ptb_common.h"
#include "ptb_dispatch.h"
#include "ptb_logits4.h"
#include "ptb_softskel_host.h"

namespace ptb {

constexpr int SS_THREADS = 256;
constexpr int SS_FWD_TILE = 32;
#define SS_INF __builtin_inff()

struct SsArgs {
    const float* x;             // [B, C, S] logits / probabilities (soft_skeleton: [N, 1, S] planes)
    const long long* labels;    // [B, S], or NULL ...
    const float* dense;         // ... and [B, C, S]
    float* st;                  // [B, K, S] soft skeleton of the target (soft_skeleton: of x)
    double* slots;              // [K][B * tiles][4]
    const float* coef;          // [K][3] a, b, c
    float* dp;                  // [B, K, S] dloss / dp
    int cls[SS_MAX_CLASSES];    // the channel of selected class k
    int B, C, K, H, W, act, k;
    unsigned tiles, ntx;
};

// ---------------------------------------------------------------------------------------------------------- the values of a cell
// the plane of a tile at (ty0, tx0) with a halo of HALO cells and the ring: the values of the image, +inf elsewhere
template <int LP, int HALO, bool TARGET>
__device__ __forceinline__ void ss_load(const SsArgs& a, float* dst, size_t b, int ch, int ty0, int tx0) {
#pragma unroll 1
    for (int c = (int)threadIdx.x; c < LP * LP; c += SS_THREADS) {
        const int r = c / LP, q = c - r * LP;
        const int gy = ty0 - HALO - 1 + r, gx = tx0 - HALO - 1 + q;
        float v = SS_INF;
        if (r >= 1 && r <= LP - 2 && q >= 1 && q <= LP - 2 && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
            const size_t S = (size_t)a.H * (size_t)a.W, pos = (size_t)gy * (size_t)a.W + (size_t)gx;
            v = TARGET ? target(a.labels, a.dense, b, ch, a.C, S, pos) : prob(a.x + b * (size_t)a.C * S + pos, ch, a.C, S, a.act);
        }
        dst[c] = v;
    }
}

// ---------------------------------------------------------------------------------------------------------- E and D on a plane
template <int LP>
__device__ __forceinline__ void ss_erode(const float* s, float* d) {
#pragma unroll 2
    for (int c = (int)threadIdx.x; c < LP * LP; c += SS_THREADS) {
        float m = s[c];
        if (m < SS_INF) m = fminf(fminf(fminf(s[c - LP], s[c - 1]), fminf(s[c + 1], s[c + LP])), m);
        d[c] = m;
    }
}

// the window index E selects at a finite cell: up, left, centre, right, down; the first among equal values
template <int LP>
__device__ __forceinline__ int ss_erode_select(const float* s, int c) {
    float m = s[c - LP];
    int at = 0;
    if (s[c - 1] < m) { m = s[c - 1]; at = 1; }
    if (s[c] < m) { m = s[c]; at = 2; }
    if (s[c + 1] < m) { m = s[c + 1]; at = 3; }
    if (s[c + LP] < m) at = 4;
    return at;
}

// D at a finite cell, and the row-major window index it selects (the first among equal values)
template <int LP>
__device__ __forceinline__ float ss_dilate(const float* s, int c, int& at) {
    float m = -SS_INF;
    at = 4;
#pragma unroll
    for (int n = 0; n < 9; ++n) {
        const float v = s[c + (n / 3 - 1) * LP + (n % 3 - 1)];
        if (v < SS_INF && v > m) { m = v; at = n; }
    }
    return m;
}

// E's window in its order: up, left, centre, right, down
template <int L>
__device__ __forceinline__ constexpr int ss_cross(int n) { return n == 0 ? -L : n == 1 ? -1 : n == 2 ? 0 : n == 3 ? 1 : L; }

__device__ __forceinline__ const float* ss_plane(const float* X, const float* P1, const float* P2, int i) { return i == 0 ? X : (i & 1) ? P1 : P2; }

// Stages 0 .. n - 1 for the cells cf[] a lane owns: S = S_n-1 (0 for n == 0).  v_0 = X, v_i alternates between P1 and P2 (P2 may be X: the
// forward kernel rolls over two planes).  Entered and left with every write to the planes visible to the workgroup.
template <int LP, int PER>
__device__ __forceinline__ void ss_stages(const float* X, float* P1, float* P2, int n, const int (&cf)[PER], unsigned active, float (&S)[PER]) {
#pragma unroll
    for (int u = 0; u < PER; ++u) S[u] = 0.0f;
#pragma unroll 1
    for (int i = 0; i < n; ++i) {
        const float* src = ss_plane(X, P1, P2, i);
        float* dst = const_cast<float*>(ss_plane(X, P1, P2, i + 1));
        ss_erode<LP>(src, dst);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            if (!(active >> u & 1u)) continue;
            int at;
            const float diff = src[cf[u]] - ss_dilate<LP>(dst, cf[u], at);
            const float d = diff > 0.0f ? diff : 0.0f;
            const float t = d - S[u] * d;
            S[u] += t > 0.0f ? t : 0.0f;
        }
        __syncthreads();
    }
}

__device__ __forceinline__ void ss_place(const SsArgs& a, unsigned& k, unsigned& b, int& ty0, int& tx0, int T) {
    const unsigned t = blockIdx.x % a.tiles, kb = blockIdx.x / a.tiles;
    b = kb % (unsigned)a.B;
    k = kb / (unsigned)a.B;
    ty0 = (int)(t / a.ntx) * T;
    tx0 = (int)(t % a.ntx) * T;
}

// ---------------------------------------------------------------------------------------------------------- forward
// LAUNCHED WITH EXACTLY SS_THREADS THREADS over K * B * tiles workgroups
template <int R, bool LOSS>
__global__ __launch_bounds__(SS_THREADS) void ss_fwd_kernel(const SsArgs a) {
    constexpr int T = SS_FWD_TILE, LP = T + 2 * R + 2, PER = T * T / SS_THREADS;
    __shared__ float P[2][LP * LP];
    __shared__ double wsum[SS_THREADS / 64][4];                              // (block_sums, ptb_logits4.h)
    unsigned k, b;
    int ty0, tx0;
    ss_place(a, k, b, ty0, tx0, T);
    const int ch = a.cls[k];
    const size_t S = (size_t)a.H * (size_t)a.W;
    int cf[PER];
    size_t pos[PER];
    unsigned active = 0u;
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int i = (int)threadIdx.x + u * SS_THREADS, iy = i / T, ix = i % T;
        cf[u] = (iy + R + 1) * LP + ix + R + 1;
        pos[u] = (size_t)(ty0 + iy) * (size_t)a.W + (size_t)(tx0 + ix);
        if (ty0 + iy < a.H && tx0 + ix < a.W) active |= 1u << u;
    }
    float own[LOSS ? 2 : 1][PER], skel[LOSS ? 2 : 1][PER];
#pragma unroll
    for (int side = 0; side < (LOSS ? 2 : 1); ++side) {
        if (side == 0) ss_load<LP, R, false>(a, P[0], b, ch, ty0, tx0);
        else ss_load<LP, R, true>(a, P[0], b, ch, ty0, tx0);
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PER; ++u) own[side][u] = P[0][cf[u]];
        ss_stages<LP, PER>(P[0], P[1], P[0], a.k + 1, cf, active, skel[side]);
    }
    if constexpr (!LOSS) {
#pragma unroll
        for (int u = 0; u < PER; ++u)
            if (active >> u & 1u) a.st[(size_t)b * S + pos[u]] = skel[0][u];
    } else {
        double s[4] = {0.0, 0.0, 0.0, 0.0};                                    // sum SP g, sum SP, sum ST p, sum ST
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            if (!(active >> u & 1u)) continue;
            a.st[((size_t)b * a.K + k) * S + pos[u]] = skel[1][u];
            s[0] += (double)(skel[0][u] * own[1][u]);
            s[1] += (double)skel[0][u];
            s[2] += (double)(skel[1][u] * own[0][u]);
            s[3] += (double)skel[1][u];
        }
        const double r = block_sums(s, wsum);
        if (threadIdx.x < 4) a.slots[(size_t)blockIdx.x * 4 + threadIdx.x] = r;
    }
}

// one workgroup: per class the slots in index order (a lane per run of neighbouring slots, then a fixed tree over the lanes), the tail, a / b / c
__global__ __launch_bounds__(SS_THREADS) void ss_finish_kernel(const double* slots, unsigned per_class, int K, float smooth, float* loss, float* coef) {
    __shared__ double part[4][SS_THREADS];
    const unsigned run = (per_class + SS_THREADS - 1) / SS_THREADS;
    const unsigned lo = min(threadIdx.x * run, per_class), hi = min(lo + run, per_class);
    double total = 0.0;
#pragma unroll 1
    for (int k = 0; k < K; ++k) {
        const double* s = slots + (size_t)k * per_class * 4;
        double r[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 1
        for (unsigned i = lo; i < hi; ++i) {
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q] += s[(size_t)i * 4 + q];
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) part[q][threadIdx.x] = r[q];
        __syncthreads();
#pragma unroll 1
        for (int half = SS_THREADS / 2; half > 0; half >>= 1) {                // a fixed tree over the lanes: lane i takes lane i + half
            if ((int)threadIdx.x < half) {
#pragma unroll
                for (int q = 0; q < 4; ++q) part[q][threadIdx.x] += part[q][threadIdx.x + half];
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) r[q] = part[q][0];
            const double sm = (double)smooth, inv_k = 1.0 / (double)K;
            const double tp = (r[0] + sm) / (r[1] + sm), ts = (r[2] + sm) / (r[3] + sm), den = tp + ts;
            double l = 1.0, da = 0.0, db = 0.0, dc = 0.0;
            if (den != 0.0) {
                l = 1.0 - 2.0 * tp * ts / den;
                const double dtp = -2.0 * ts * ts / (den * den), dts = -2.0 * tp * tp / (den * den);
                da = dtp / (r[1] + sm);
                db = -dtp * tp / (r[1] + sm);
                dc = dts / (r[3] + sm);
            }
            total += l;
            coef[k * 3 + 0] = (float)(da * inv_k);
            coef[k * 3 + 1] = (float)(db * inv_k);
            coef[k * 3 + 2] = (float)(dc * inv_k);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (float)(total / (double)K);
}

// ---------------------------------------------------------------------------------------------------------- backward
template <int T_, int R_>
struct SsBwd {
    static constexpr int T = T_, R = R_;
    static constexpr int LP = T + 4 * R + 2;        // the forward planes: the tile + 2 R and the ring
    static constexpr int LA = T + 2 * R + 2;        // the adjoint planes: the tile + R and a ring of zeros
    static constexpr int PER = (LA * LA + SS_THREADS - 1) / SS_THREADS;
    static constexpr int LDS_BYTES = 3 * LP * LP * 4 + LA * LA * 9;
    static_assert(LDS_BYTES <= 160 * 1024 / 3, "three workgroups a CU");
    static_assert(PER <= 8, "a lane's cells are a bit mask and a handful of registers");
};

// LAUNCHED WITH EXACTLY SS_THREADS THREADS over K * B * tiles workgroups (tiles of side G::T); a.k + 2 <= G::R
template <class G>
__global__ __launch_bounds__(SS_THREADS) void ss_bwd_kernel(const SsArgs a) {
    constexpr int T = G::T, R = G::R, LP = G::LP, LA = G::LA, PER = G::PER;
    __shared__ float X[LP * LP], P1[LP * LP], P2[LP * LP];
    __shared__ float Go[LA * LA], Gv[LA * LA];
    __shared__ unsigned char Sel[LA * LA];          // bits 0-3: the index D selects at the cell, bits 4-7: the one E selects; 0xFF: none
    unsigned k, b;
    int ty0, tx0;
    ss_place(a, k, b, ty0, tx0, T);
    const int ch = a.cls[k];
    const size_t S = (size_t)a.H * (size_t)a.W;
    const float ca = a.coef[k * 3 + 0], cb = a.coef[k * 3 + 1], cc = a.coef[k * 3 + 2];

    ss_load<LP, 2 * R, false>(a, X, b, ch, ty0, tx0);
#pragma unroll 1
    for (int c = (int)threadIdx.x; c < LA * LA; c += SS_THREADS) {
        Go[c] = 0.0f;
        Gv[c] = 0.0f;
        Sel[c] = 0xFFu;
    }
    int cf[PER], cg[PER];
    size_t pos[PER];
    unsigned active = 0u, inner = 0u;               // the cell lies in the image; ... and in the tile
    float gS[PER], prev[PER];                       // gS_j; direct_j+1
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        const int c = (int)threadIdx.x + u * SS_THREADS, ra = c / LA, qa = c - ra * LA;
        const int gy = ty0 - R - 1 + ra, gx = tx0 - R - 1 + qa;
        cg[u] = c < LA * LA ? c : 0;
        cf[u] = c < LA * LA ? (ra + R) * LP + qa + R : 0;
        pos[u] = 0;
        gS[u] = prev[u] = 0.0f;
        if (c < LA * LA && ra >= 1 && ra <= LA - 2 && qa >= 1 && qa <= LA - 2 && gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) {
            active |= 1u << u;
            pos[u] = (size_t)gy * (size_t)a.W + (size_t)gx;
            if (gy >= ty0 && gy < ty0 + T && gx >= tx0 && gx < tx0 + T) inner |= 1u << u;
            gS[u] = ca * target(a.labels, a.dense, b, ch, a.C, S, pos[u]) + cb;                     // w = a g + b
        }
    }
    __syncthreads();

#pragma unroll 1
    for (int j = a.k; j >= 0; --j) {
        float Sp[PER];                                                         // S_j-1
        ss_stages<LP, PER>(X, P1, P2, j, cf, active, Sp);
        const float* src = ss_plane(X, P1, P2, j);
        float* dst = const_cast<float*>(ss_plane(X, P1, P2, j + 1));
        ss_erode<LP>(src, dst);
        __syncthreads();
        float now[PER];                                                        // direct_j
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            now[u] = 0.0f;
            if (!(active >> u & 1u)) continue;
            int at;
            const float diff = src[cf[u]] - ss_dilate<LP>(dst, cf[u], at);
            const bool over = diff > 0.0f;
            const float d = over ? diff : 0.0f;
            const bool m = d - Sp[u] * d > 0.0f;
            const float gd = m ? gS[u] * (1.0f - Sp[u]) : 0.0f;
            if (m) gS[u] = gS[u] * (1.0f - d);
            now[u] = over ? gd : 0.0f;
            Go[cg[u]] = -now[u];
            Sel[cg[u]] = (unsigned char)(at | ss_erode_select<LP>(dst, cf[u]) << 4);
        }
        __syncthreads();
        float gv[PER];                                                         // gv_j+1 = direct_j+1 + D^T(go_j) + E^T(gv_j+2)
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            gv[u] = prev[u];
            prev[u] = now[u];
            if (!(active >> u & 1u)) continue;
            const int c = cg[u];
#pragma unroll
            for (int n = 0; n < 9; ++n) {
                const int q = c + (n / 3 - 1) * LA + (n % 3 - 1);
                if ((Sel[q] & 15u) == (unsigned)(8 - n)) gv[u] += Go[q];
            }
#pragma unroll
            for (int n = 0; n < 5; ++n) {
                const int q = c + ss_cross<LA>(n);
                if ((unsigned)(Sel[q] >> 4) == (unsigned)(4 - n)) gv[u] += Gv[q];
            }
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < PER; ++u)
            if (active >> u & 1u) Gv[cg[u]] = gv[u];
    }
    // gv_0 = direct_0 + E^T(gv_1), the selection over v_0
#pragma unroll
    for (int u = 0; u < PER; ++u)
        if (active >> u & 1u) Sel[cg[u]] = (unsigned char)(15 | ss_erode_select<LP>(X, cf[u]) << 4);
    __syncthreads();
#pragma unroll
    for (int u = 0; u < PER; ++u) {
        if (!(inner >> u & 1u)) continue;
        float g = prev[u];
#pragma unroll
        for (int n = 0; n < 5; ++n) {
            const int q = cg[u] + ss_cross<LA>(n);
            if ((unsigned)(Sel[q] >> 4) == (unsigned)(4 - n)) g += Gv[q];
        }
        const size_t at = ((size_t)b * a.K + k) * S + pos[u];
        a.dp[at] = g + cc * a.st[at];
    }
}

struct SsActArgs {
    const float* x;             // [B, C, S]
    const float* dp;            // [B, K, S]
    const float* upstream;      // [1]
    float* grad;                // [B, C, S]
    int cls[SS_MAX_CLASSES];
    size_t S, total;            // total = B * S
    int C, K, act;
};

__global__ __launch_bounds__(SS_THREADS) void ss_act_bwd_kernel(const SsActArgs a) {
    const size_t i = (size_t)blockIdx.x * SS_THREADS + threadIdx.x;
    if (i >= a.total) return;
    const size_t b = i / a.S, pos = i - b * a.S;
    const float up = *a.upstream;
    const float* x0 = a.x + b * (size_t)a.C * a.S + pos;
    const float* d0 = a.dp + b * (size_t)a.K * a.S + pos;
    float* g0 = a.grad + b * (size_t)a.C * a.S + pos;
    float m = 0.0f, s = 1.0f, dot = 0.0f;
    if (a.act == PTB_PROB_SOFTMAX) {                                           // grad_c = p_c (d_c - sum_j p_j d_j)
        m = x0[0];
#pragma unroll 1
        for (int c = 1; c < a.C; ++c) m = fmaxf(m, x0[(size_t)c * a.S]);
        s = 0.0f;
#pragma unroll 1
        for (int c = 0; c < a.C; ++c) s += expf(x0[(size_t)c * a.S] - m);
#pragma unroll 1
        for (int k = 0; k < a.K; ++k) dot += expf(x0[(size_t)a.cls[k] * a.S] - m) / s * d0[(size_t)k * a.S];
    }
#pragma unroll 1
    for (int c = 0; c < a.C; ++c) {
        float d = 0.0f;
        bool selected = false;
#pragma unroll 1
        for (int k = 0; k < a.K; ++k)
            if (a.cls[k] == c) {
                d = d0[(size_t)k * a.S];
                selected = true;
            }
        const float v = x0[(size_t)c * a.S];
        float g;
        if (a.act == PTB_PROB_SOFTMAX) g = expf(v - m) / s * (d - dot);
        else if (!selected) g = 0.0f;
        else if (a.act == PTB_PROB_SIGMOID) {
            const float p = 1.0f / (1.0f + expf(-v));
            g = p * (1.0f - p) * d;
        } else g = d;
        g0[(size_t)c * a.S] = up * g;
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
static long long ss_tiles(long long H, long long W, int T) { return ((H + T - 1) / T) * ((W + T - 1) / T); }

static int ss_bwd_tile(int k) { return k <= 3 ? 32 : k <= 5 ? 24 : 16; }

// the shape part of the arguments; the grid of a launch with tiles of side T
static int ss_problem(int64_t B, int C, int K, int64_t H, int64_t W, int iterations, int T, SsArgs& a) {
    if (B < 1 || C < 1 || K < 1 || H < 1 || W < 1 || iterations < 1) return PTB_EINVAL;
    if (iterations > SS_CAP || K > SS_MAX_CLASSES) return PTB_EUNSUPPORTED;
    if (H > MAX_POS || W > MAX_POS || H * W > MAX_POS || B > MAX_POS) return PTB_EUNSUPPORTED;
    const long long tiles = ss_tiles(H, W, T);
    if (tiles > MAX_POS / ((long long)K * B)) return PTB_EUNSUPPORTED;
    a.B = (int)B; a.C = C; a.K = K; a.H = (int)H; a.W = (int)W; a.k = iterations;
    a.tiles = (unsigned)tiles; a.ntx = (unsigned)((W + T - 1) / T);
    return PTB_OK;
}

// ptb_softskel_host.h: the rank-agnostic kernels for the volume unit
void ss_launch_finish(const double* slots, unsigned per_class, int K, float smooth, float* loss, float* coef, hipStream_t stream) {
    hipLaunchKernelGGL(ss_finish_kernel, dim3(1), dim3(SS_THREADS), 0, stream, slots, per_class, K, smooth, loss, coef);
}

int ss_launch_act_bwd(const float* x, const float* dp, const float* upstream, float* grad, const int* cls, int K, int C, int prob, size_t B, size_t S,
                      hipStream_t stream) {
    const size_t positions = B * S, blocks = (positions + SS_THREADS - 1) / SS_THREADS;        // the streaming pass: a lane a position
    if (blocks > 0x7fffffffULL) return PTB_EUNSUPPORTED;
    SsActArgs g{};
    g.x = x; g.dp = dp; g.upstream = upstream; g.grad = grad;
    for (int k = 0; k < K; ++k) g.cls[k] = cls[k];
    g.S = S; g.total = positions; g.C = C; g.K = K; g.act = prob;
    hipLaunchKernelGGL(ss_act_bwd_kernel, dim3((unsigned)blocks), dim3(SS_THREADS), 0, stream, g);
    return PTB_OK;
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_softskel_cap(void) { return SS_CAP; }

extern "C" int ptb_soft_skeleton(const float* x, int64_t N, int64_t H, int64_t W, int iterations, float* out, ptb_stream_t stream) {
    if (!x || !out) return PTB_EINVAL;
    SsArgs a{};
    if (int rc = ss_problem(N, 1, 1, H, W, iterations, SS_FWD_TILE, a)) return rc;
    a.x = x; a.st = out; a.act = PTB_PROB_IDENTITY;
    with_at_most<5, 10>(iterations + 2, [&](auto r) {
        hipLaunchKernelGGL((ss_fwd_kernel<r(), false>), dim3((unsigned)N * a.tiles), dim3(SS_THREADS), 0, (hipStream_t)stream, a);
    });
    return check_launch();
}

extern "C" int64_t ptb_soft_cldice_slots(int64_t B, int K, int64_t H, int64_t W) {
    SsArgs a{};
    if (int rc = ss_problem(B, 1, K, H, W, 1, SS_FWD_TILE, a)) return rc;
    return (int64_t)K * B * a.tiles;
}

extern "C" int ptb_soft_cldice_fwd(const float* x, const int64_t* labels, const float* dense, int64_t B, int C, int64_t H, int64_t W, const int* classes,
                                   int K, int prob, int iterations, float smooth, float* st, void* workspace, int64_t workspace_bytes, float* loss,
                                   float* coef, ptb_stream_t stream) {
    if (!x || (labels != nullptr) == (dense != nullptr) || !st || !workspace || !loss || !coef || ss_bad_prob(prob)) return PTB_EINVAL;
    if (!(smooth >= 0.0f) || !std::isfinite(smooth)) return PTB_EINVAL;
    SsArgs a{};
    if (int rc = ss_classes(classes, C, K, a.cls)) return rc;
    if (int rc = ss_problem(B, C, K, H, W, iterations, SS_FWD_TILE, a)) return rc;
    const long long slots = (long long)K * B * a.tiles;
    if (!aligned16(workspace) || workspace_bytes < 32 * slots) return PTB_EINVAL;
    a.x = x; a.labels = reinterpret_cast<const long long*>(labels); a.dense = dense; a.st = st; a.act = prob;
    a.slots = reinterpret_cast<double*>(workspace);
    hipStream_t s = (hipStream_t)stream;
    with_at_most<5, 10>(iterations + 2, [&](auto r) {
        hipLaunchKernelGGL((ss_fwd_kernel<r(), true>), dim3((unsigned)slots), dim3(SS_THREADS), 0, s, a);
    });
    ss_launch_finish(a.slots, (unsigned)(B * a.tiles), K, smooth, loss, coef, s);
    return check_launch();
}

extern "C" int ptb_soft_cldice_bwd(const float* x, const int64_t* labels, const float* dense, int64_t B, int C, int64_t H, int64_t W, const int* classes,
                                   int K, int prob, int iterations, const float* st, const float* coef, const float* upstream, float* dp, float* grad,
                                   ptb_stream_t stream) {
    if (!x || (labels != nullptr) == (dense != nullptr) || !st || !coef || !upstream || !dp || !grad || ss_bad_prob(prob)) return PTB_EINVAL;
    SsArgs a{};
    if (int rc = ss_classes(classes, C, K, a.cls)) return rc;
    const int T = ss_bwd_tile(iterations);
    if (int rc = ss_problem(B, C, K, H, W, iterations, T, a)) return rc;
    a.x = x; a.labels = reinterpret_cast<const long long*>(labels); a.dense = dense; a.st = const_cast<float*>(st); a.act = prob;
    a.coef = coef; a.dp = dp;
    if (((size_t)B * (size_t)H * (size_t)W + SS_THREADS - 1) / SS_THREADS > 0x7fffffffULL) return PTB_EUNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)((long long)K * B * a.tiles));
    if (T == 32) hipLaunchKernelGGL((ss_bwd_kernel<SsBwd<32, 5>>), grid, dim3(SS_THREADS), 0, s, a);
    else if (T == 24) hipLaunchKernelGGL((ss_bwd_kernel<SsBwd<24, 7>>), grid, dim3(SS_THREADS), 0, s, a);
    else hipLaunchKernelGGL((ss_bwd_kernel<SsBwd<16, 10>>), grid, dim3(SS_THREADS), 0, s, a);
    ss_launch_act_bwd(x, dp, upstream, grad, a.cls, K, C, prob, (size_t)B, (size_t)H * (size_t)W, s);
    return check_launch();
}
