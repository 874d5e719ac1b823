// The soft skeleton and the soft-clDice loss of VOLUMES (losses/cldice.py and utils/softskel.py with dims=3).  The definitions stand in
// include/ptb_hip.h: E = the minimum over a position and its 6 face neighbours, D = the maximum over the 3 x 3 x 3 window, positions outside
// the volume never take part; the chain v_j+1 = E(v_j), o_j = D(v_j+1), delta_j = relu(v_j - o_j), S_j = S_j-1 + relu(delta_j - S_j-1 delta_j)
// is the one of ptb_softskel.hip.
// ONE LAUNCH PER STAGE, NOT A STENCIL BLOCKED IN TIME.  Blocking all k + 1 stages needs a halo of k + 2 on every side, and in three axes under
// a fifth of a tile would be useful; a stage alone needs a halo of 2 (E on the tile + 1, D of that on the tile), and a pass through HBM per stage
// is cheap at the sizes of volume patches.  A workgroup of 256 lanes owns a tile of (TZ, TY, TX) = (8, 8, 32) positions; a lane owns one (y, x)
// column of it and walks it in z.  A cell outside the volume holds +inf, which is "takes no part": E leaves it, a minimum ignores it, D reads it
// as absent.  No block needs a ring: E is evaluated on the tile + 1 only and reads the tile + 2, D on the tile only and reads the tile + 1.
//   1. ss3_stage_kernel<FIRST, LAST, SAVE>   a workgroup per (side: prediction | target, class, batch entry, tile).  Loads v_j on the tile + 2
//                      (FIRST: the activation of the logits -- a softmax reads the C logits of a cell -- or the target; else the fp32 level
//                      the launch before wrote), E into a second block on the tile + 1, then the column walk: the in-plane 3 x 3 maxima of
//                      v_j+1 for the planes z - 1, z, z + 1 roll through three registers (9 LDS reads a cell for D, not 27); delta_j, then
//                      S_j = f(S_j-1) read and written at the lane's own position alone, and v_j+1 of the tile.  SAVE (prediction side, a
//                      gradient is wanted): v_j+1 and delta_j go to level j of two stores [k + 1][B, K, S]; otherwise two v planes ping-pong.
//                      LAST: the four sums in float64 -- the prediction side sum SP g and sum SP, the target side sum ST p and sum ST --, a
//                      column in z order, a fixed tree in the wave, the waves in order, to the workgroup's OWN slot [K][B tiles][4].
//   2. ss_finish_kernel (ptb_softskel.hip) the loss and coef [K][3] = a, b, c.
//   3. ss3_direct_kernel   pointwise, a lane a position and class: rebuilds S_-1 .. S_k-1 from delta_0 .. delta_k in registers (the S recursion
//                      is pointwise in the deltas: no S level is stored), descends from gS_k = a g + b:
//                        m_j = [delta_j - S_j-1 delta_j > 0],  g_delta_j = m_j gS_j (1 - S_j-1),  gS_j-1 = m_j ? gS_j (1 - delta_j) : gS_j,
//                        direct_j = [delta_j > 0] g_delta_j, written over delta_j.
//   4. ss3_gather_kernel<FINAL>   THE EXACT ADJOINT IN GATHER FORM, no atomics, one launch per j = k .. 0:
//                        gv_j+1 = direct_j+1 + D^T(-direct_j) + E^T(gv_j+2)   (both selections over v_j+1; direct_k+1 = gv_k+2 = 0).
//                      Loads v_j+1 on the tile + 2, -direct_j and gv_j+2 on the tile + 1; every cell q of the tile + 1 writes one selection byte
//                      (bits 0-4: the index D selects at q, 0 .. 26, dz then dy then dx ascending; bits 5-7: the one E selects, in the order
//                      z-1, y-1, x-1, centre, x+1, y+1, z+1; the first among equal values; 0xFF outside the volume); a receiving cell p of the
//                      tile adds the adjoint of each neighbour whose byte names p.  gv ping-pongs between two planes.  FINAL: gv_0 = direct_0
//                      + E^T(gv_1) over v_0 -- the activation on load, so the probabilities are never stored --, no D term; writes
//                      dp = gv_0 + c ST.
//   5. ss_act_bwd_kernel (ptb_softskel.hip) with S = D H W.
// Every sum is added in a fixed order and the grids depend on the shape and k alone: a second run gives the same bits.  No workgroup waits
// for another one; every loop is bounded by k, C, K or a tile.
#include <cmath>

#include "ptb_common.h"
#include "ptb_dispatch.h"
#include "ptb_logits4.h"
#include "ptb_softskel_host.h"

namespace ptb {

constexpr int SS3_THREADS = 256;
constexpr int TZ = 8, TY = 8, TX = 32;           // the tile; TY * TX lanes, one column each
constexpr int AZ = TZ + 4, AY = TY + 4, AX = TX + 4, AN = AZ * AY * AX;        // the block on the tile + 2
constexpr int BZ = TZ + 2, BY = TY + 2, BX = TX + 2, BN = BZ * BY * BX;        // the block on the tile + 1
static_assert(TY * TX == SS3_THREADS, "a lane a column");
constexpr int SS3_STAGE_LDS = (AN + BN) * 4 + 4 * 2 * 8;
constexpr int SS3_GATHER_LDS = (AN + 2 * BN) * 4 + BN;
static_assert(SS3_STAGE_LDS == 34400 && SS3_STAGE_LDS <= 160 * 1024 / 4, "ss3_stage_kernel: 34400 bytes (34336 without sums), four workgroups a CU");
static_assert(SS3_GATHER_LDS == 51336 && SS3_GATHER_LDS <= 160 * 1024 / 3, "ss3_gather_kernel: 51336 bytes, three workgroups a CU");
#define SS3_INF __builtin_inff()

struct Ss3Shape {
    int B, C, K, D, H, W, act;
    unsigned tiles, ntx, nty;                    // tiles of a volume; along x, along y
    int cls[SS_MAX_CLASSES];                     // the channel of selected class k
};

struct Ss3Args {
    Ss3Shape s;
    const float* x;             // [B, C, S] logits / probabilities (soft_skeleton: [N, 1, S] volumes)
    const long long* labels;    // [B, S], or NULL ...
    const float* dense;         // ... and [B, C, S]
    const float *vin0, *vin1;   // v_j [B, K, S] of the prediction / target side (not FIRST)
    float *vout0, *vout1;       // v_j+1 (not LAST; the prediction side under SAVE writes vsave instead)
    float *S0, *S1;             // S [B, K, S] of the two sides, read and written in place
    float *vsave, *dsave;       // level j of the two stores (SAVE)
    double* slots;              // [K][B * tiles][4], or NULL: no sums (soft_skeleton)
};

struct Ss3GatherArgs {
    Ss3Shape s;
    const float* x;             // FINAL: the logits, v_0 is their activation
    const float* v;             // v_j+1 [B, K, S]
    const float* go;            // direct_j (its negative is the adjoint of o_j)
    const float* gvin;          // gv_j+2, or NULL: zeros
    const float* own;           // direct_j+1 (FINAL: direct_0), or NULL: zeros
    float* gvout;               // gv_j+1
    const float* st;            // FINAL: ST, coef and dp = gv_0 + c ST
    const float* coef;
    float* dp;
};

// where a workgroup stands: side, class, batch entry, the origin of its tile
struct Ss3Place {
    unsigned side, k, b;
    int z0, y0, x0;
};

__device__ __forceinline__ Ss3Place ss3_place(const Ss3Shape& s) {
    Ss3Place p;
    const unsigned t = blockIdx.x % s.tiles, skb = blockIdx.x / s.tiles;
    p.b = skb % (unsigned)s.B;
    const unsigned sk = skb / (unsigned)s.B;
    p.k = sk % (unsigned)s.K;
    p.side = sk / (unsigned)s.K;
    const unsigned tzy = t / s.ntx;
    p.x0 = (int)(t % s.ntx) * TX;
    p.y0 = (int)(tzy % s.nty) * TY;
    p.z0 = (int)(tzy / s.nty) * TZ;
    return p;
}

// cell c of a block of (NY, NX) rows whose origin lies HALO cells before the tile's: its position in the volume, or false outside
template <int NY, int NX, int HALO>
__device__ __forceinline__ bool ss3_cell(const Ss3Shape& s, const Ss3Place& p, int c, size_t& pos) {
    const int z = c / (NY * NX), r = c - z * (NY * NX), y = r / NX, x = r - y * NX;
    const int gz = p.z0 - HALO + z, gy = p.y0 - HALO + y, gx = p.x0 - HALO + x;
    if (gz < 0 || gz >= s.D || gy < 0 || gy >= s.H || gx < 0 || gx >= s.W) return false;
    pos = ((size_t)gz * (size_t)s.H + (size_t)gy) * (size_t)s.W + (size_t)gx;
    return true;
}

// cell c of the tile + 1 block -> the same cell of the tile + 2 block
__device__ __forceinline__ int ss3_b_to_a(int c) {
    const int z = c / (BY * BX), r = c - z * (BY * BX), y = r / BX, x = r - y * BX;
    return ((z + 1) * AY + y + 1) * AX + x + 1;
}

// E's window in its order: z-1, y-1, x-1, centre, x+1, y+1, z+1, as offsets in a block of (NY, NX) rows
template <int NY, int NX>
__device__ __forceinline__ constexpr int ss3_cross(int n) {
    return n == 0 ? -NY * NX : n == 1 ? -NX : n == 2 ? -1 : n == 3 ? 0 : n == 4 ? 1 : n == 5 ? NX : NY * NX;
}

// D's window, dz then dy then dx ascending
template <int NY, int NX>
__device__ __forceinline__ constexpr int ss3_cube(int n) { return (n / 9 - 1) * NY * NX + (n / 3 % 3 - 1) * NX + (n % 3 - 1); }

// the maximum of the in-plane 3 x 3 window of the tile + 1 block around cell c; -inf where no cell of it lies in the volume
__device__ __forceinline__ float ss3_plane_max(const float* Bv, int c) {
    float m = -SS3_INF;
#pragma unroll
    for (int n = 0; n < 9; ++n) {
        const float v = Bv[c + (n / 3 - 1) * BX + (n % 3 - 1)];
        if (v < SS3_INF) m = fmaxf(m, v);
    }
    return m;
}

// ---------------------------------------------------------------------------------------------------------- a stage
// LAUNCHED WITH EXACTLY SS3_THREADS THREADS over sides * K * B * tiles workgroups
template <bool FIRST, bool LAST, bool SAVE>
__global__ __launch_bounds__(SS3_THREADS) void ss3_stage_kernel(const Ss3Args a) {
    __shared__ float A[AN];                         // v_j on the tile + 2
    __shared__ float Bv[BN];                        // v_j+1 on the tile + 1
    __shared__ double wsum[SS3_THREADS / 64][2];    // (block_sums, ptb_logits4.h)
    const Ss3Shape& s = a.s;
    const Ss3Place p = ss3_place(s);
    const bool is_target = p.side != 0u;
    const int ch = s.cls[p.k];
    const size_t S = (size_t)s.D * (size_t)s.H * (size_t)s.W, base = ((size_t)p.b * s.K + p.k) * S;
    const float* vin = is_target ? a.vin1 : a.vin0;
#pragma unroll 1
    for (int c = (int)threadIdx.x; c < AN; c += SS3_THREADS) {
        size_t pos;
        float v = SS3_INF;
        if (ss3_cell<AY, AX, 2>(s, p, c, pos)) {
            if constexpr (FIRST) v = is_target ? target(a.labels, a.dense, p.b, ch, s.C, S, pos) : prob(a.x + (size_t)p.b * s.C * S + pos, ch, s.C, S, s.act);
            else v = vin[base + pos];
        }
        A[c] = v;
    }
    __syncthreads();
#pragma unroll 2
    for (int c = (int)threadIdx.x; c < BN; c += SS3_THREADS) {
        const int ca = ss3_b_to_a(c);
        float m = A[ca];
        if (m < SS3_INF) {
#pragma unroll
            for (int n = 0; n < 7; ++n)
                if (n != 3) m = fminf(m, A[ca + ss3_cross<AY, AX>(n)]);
        }
        Bv[c] = m;
    }
    __syncthreads();

    const int ly = (int)threadIdx.x / TX, lx = (int)threadIdx.x % TX;
    const bool column = p.y0 + ly < s.H && p.x0 + lx < s.W;
    const bool save = SAVE && !is_target;
    float* Sp = is_target ? a.S1 : a.S0;
    float* vout = is_target ? a.vout1 : a.vout0;
    const size_t at0 = base + ((size_t)p.z0 * (size_t)s.H + (size_t)(p.y0 + ly)) * (size_t)s.W + (size_t)(p.x0 + lx), plane = (size_t)s.H * (size_t)s.W;
    const int cb0 = (ly + 1) * BX + lx + 1;         // the column in plane 0 of the tile + 1 block
    double sums[2] = {0.0, 0.0};                    // prediction: sum SP g, sum SP; target: sum ST p, sum ST
    float m0 = ss3_plane_max(Bv, cb0), m1 = ss3_plane_max(Bv, cb0 + BY * BX);
#pragma unroll
    for (int z = 0; z < TZ; ++z) {
        const float m2 = ss3_plane_max(Bv, cb0 + (z + 2) * BY * BX);
        if (column && p.z0 + z < s.D) {
            const size_t at = at0 + (size_t)z * plane;
            const float diff = A[((z + 2) * AY + ly + 2) * AX + lx + 2] - fmaxf(fmaxf(m0, m1), m2);
            const float d = diff > 0.0f ? diff : 0.0f;
            float skel = 0.0f;
            if constexpr (!FIRST) skel = Sp[at];
            const float t = d - skel * d;
            skel += t > 0.0f ? t : 0.0f;
            Sp[at] = skel;
            const float vn = Bv[cb0 + (z + 1) * BY * BX];
            if (save) {
                a.vsave[at] = vn;
                a.dsave[at] = d;
            } else if (!LAST) vout[at] = vn;
            if constexpr (LAST) {
                if (a.slots) {
                    const size_t pos = at - base;
                    const float other = is_target ? prob(a.x + (size_t)p.b * s.C * S + pos, ch, s.C, S, s.act) : target(a.labels, a.dense, p.b, ch, s.C, S, pos);
                    sums[0] += (double)(skel * other);
                    sums[1] += (double)skel;
                }
            }
        }
        m0 = m1;
        m1 = m2;
    }
    if constexpr (LAST) {
        if (!a.slots) return;                       // (uniform: a kernel argument)
        const double r = block_sums(sums, wsum);
        if (threadIdx.x < 2) {
            const size_t slot = ((size_t)p.k * s.B + p.b) * s.tiles + blockIdx.x % s.tiles;
            a.slots[slot * 4 + (is_target ? 2 : 0) + threadIdx.x] = r;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------- backward
struct Ss3DirectArgs {
    const long long* labels;
    const float* dense;
    const float* coef;          // [K][3]
    float* dstore;              // [k + 1][B, K, S]: delta_j in, direct_j out
    size_t S, total;            // total = B * K * S
    int C, K, k;
    int cls[SS_MAX_CLASSES];
};

__global__ __launch_bounds__(SS3_THREADS) void ss3_direct_kernel(const Ss3DirectArgs a) {
    const size_t i = (size_t)blockIdx.x * SS3_THREADS + threadIdx.x;
    if (i >= a.total) return;
    const size_t bk = i / a.S, pos = i - bk * a.S, b = bk / (size_t)a.K;
    const int k = (int)(bk - b * (size_t)a.K), ch = a.cls[k];
    const float g = target(a.labels, a.dense, b, ch, a.C, a.S, pos);
    float d[SS_CAP + 1], below[SS_CAP + 1];       // delta_j; S_j-1
    float skel = 0.0f;
#pragma unroll
    for (int j = 0; j <= SS_CAP; ++j) {
        d[j] = below[j] = 0.0f;
        if (j <= a.k) {
            d[j] = a.dstore[(size_t)j * a.total + i];
            below[j] = skel;
            const float t = d[j] - skel * d[j];
            skel += t > 0.0f ? t : 0.0f;
        }
    }
    float gS = a.coef[k * 3 + 0] * g + a.coef[k * 3 + 1];                      // w = a g + b
#pragma unroll
    for (int j = SS_CAP; j >= 0; --j) {
        if (j <= a.k) {
            const bool m = d[j] - below[j] * d[j] > 0.0f;
            const float gd = m ? gS * (1.0f - below[j]) : 0.0f;
            if (m) gS = gS * (1.0f - d[j]);
            a.dstore[(size_t)j * a.total + i] = d[j] > 0.0f ? gd : 0.0f;
        }
    }
}

// LAUNCHED WITH EXACTLY SS3_THREADS THREADS over K * B * tiles workgroups (one side)
template <bool FINAL>
__global__ __launch_bounds__(SS3_THREADS) void ss3_gather_kernel(const Ss3GatherArgs a) {
    __shared__ float V[AN];                         // v_j+1 on the tile + 2
    __shared__ float Go[BN], Gv[BN];                // -direct_j and gv_j+2 on the tile + 1, zeros outside the volume
    __shared__ unsigned char Sel[BN];
    const Ss3Shape& s = a.s;
    const Ss3Place p = ss3_place(s);
    const int ch = s.cls[p.k];
    const size_t S = (size_t)s.D * (size_t)s.H * (size_t)s.W, base = ((size_t)p.b * s.K + p.k) * S;
#pragma unroll 1
    for (int c = (int)threadIdx.x; c < AN; c += SS3_THREADS) {
        size_t pos;
        float v = SS3_INF;
        if (ss3_cell<AY, AX, 2>(s, p, c, pos)) v = FINAL ? prob(a.x + (size_t)p.b * s.C * S + pos, ch, s.C, S, s.act) : a.v[base + pos];
        V[c] = v;
    }
#pragma unroll 1
    for (int c = (int)threadIdx.x; c < BN; c += SS3_THREADS) {
        size_t pos;
        float go = 0.0f, gv = 0.0f;
        if (ss3_cell<BY, BX, 1>(s, p, c, pos)) {
            if constexpr (!FINAL) go = -a.go[base + pos];
            if (a.gvin) gv = a.gvin[base + pos];
        }
        Go[c] = go;
        Gv[c] = gv;
    }
    __syncthreads();
#pragma unroll 1
    for (int c = (int)threadIdx.x; c < BN; c += SS3_THREADS) {
        const int ca = ss3_b_to_a(c);
        unsigned sel = 0xFFu;
        if (V[ca] < SS3_INF) {
            float m = V[ca + ss3_cross<AY, AX>(0)];                            // E: the first minimum in its order
            unsigned e = 0u;
#pragma unroll
            for (int n = 1; n < 7; ++n) {
                const float v = V[ca + ss3_cross<AY, AX>(n)];
                if (v < m) { m = v; e = (unsigned)n; }
            }
            unsigned dsel = 31u;
            if constexpr (!FINAL) {                                            // D: the first maximum among the cells of the volume
                m = -SS3_INF;
#pragma unroll
                for (int n = 0; n < 27; ++n) {
                    const float v = V[ca + ss3_cube<AY, AX>(n)];
                    if (v < SS3_INF && v > m) { m = v; dsel = (unsigned)n; }
                }
            }
            sel = dsel | e << 5;
        }
        Sel[c] = (unsigned char)sel;
    }
    __syncthreads();

    const int ly = (int)threadIdx.x / TX, lx = (int)threadIdx.x % TX;
    if (!(p.y0 + ly < s.H && p.x0 + lx < s.W)) return;
    const size_t at0 = base + ((size_t)p.z0 * (size_t)s.H + (size_t)(p.y0 + ly)) * (size_t)s.W + (size_t)(p.x0 + lx), plane = (size_t)s.H * (size_t)s.W;
    float cc = 0.0f;
    if constexpr (FINAL) cc = a.coef[p.k * 3 + 2];
#pragma unroll 1
    for (int z = 0; z < TZ; ++z) {
        if (p.z0 + z >= s.D) break;
        const size_t at = at0 + (size_t)z * plane;
        const int cb = ((z + 1) * BY + ly + 1) * BX + lx + 1;
        float g = a.own ? a.own[at] : 0.0f;
        if constexpr (!FINAL) {
#pragma unroll
            for (int n = 0; n < 27; ++n) {                                     // the neighbour at window offset n names p by the opposite offset
                const int q = cb + ss3_cube<BY, BX>(n);
                if ((Sel[q] & 31u) == (unsigned)(26 - n)) g += Go[q];
            }
        }
#pragma unroll
        for (int n = 0; n < 7; ++n) {
            const int q = cb + ss3_cross<BY, BX>(n);
            if ((unsigned)(Sel[q] >> 5) == (unsigned)(6 - n)) g += Gv[q];
        }
        if constexpr (FINAL) a.dp[at] = g + cc * a.st[at];
        else a.gvout[at] = g;
    }
}

// ---------------------------------------------------------------------------------------------------------- host side
// the shape part of the arguments; PTB_EUNSUPPORTED above the caps and where a grid of `sides` sides does not fit
static int ss3_problem(int64_t B, int C, int K, int64_t D, int64_t H, int64_t W, int iterations, int sides, Ss3Shape& s) {
    if (C < 1 || K < 1 || iterations < 1) return PTB_EINVAL;
    if (int rc = check_shape(3, B, D, H, W)) return rc;
    if (iterations > SS_CAP || K > SS_MAX_CLASSES) return PTB_EUNSUPPORTED;
    const long long ntx = (W + TX - 1) / TX, nty = (H + TY - 1) / TY, ntz = (D + TZ - 1) / TZ, tiles = ntx * nty * ntz;
    if (tiles > MAX_POS / ((long long)sides * K * B)) return PTB_EUNSUPPORTED;
    if (((long long)B * K * D * H * W + SS3_THREADS - 1) / SS3_THREADS > MAX_POS) return PTB_EUNSUPPORTED;      // the pointwise grids: a lane a position and class
    s.B = (int)B; s.C = C; s.K = K; s.D = (int)D; s.H = (int)H; s.W = (int)W;
    s.tiles = (unsigned)tiles; s.ntx = (unsigned)ntx; s.nty = (unsigned)nty;
    return PTB_OK;
}

// The workspace of the loss, in bytes from its start: the slots, then float planes of P = B K S each -- the prediction's S (the backward: dp),
// two rolling planes of the target (the backward: gv), then two rolling planes of the prediction, or with keep_grad the two level stores.
struct Ss3Plan {
    size_t P, slots_bytes, total_bytes;
    float* plane(void* ws, size_t i) const { return reinterpret_cast<float*>(static_cast<char*>(ws) + slots_bytes) + i * P; }
};

static Ss3Plan ss3_plan(const Ss3Shape& s, int iterations, bool keep_grad) {
    Ss3Plan pl;
    pl.P = (size_t)s.B * (size_t)s.K * (size_t)s.D * (size_t)s.H * (size_t)s.W;
    pl.slots_bytes = 32 * (size_t)s.K * (size_t)s.B * (size_t)s.tiles;
    pl.total_bytes = pl.slots_bytes + 4 * pl.P * (3 + (keep_grad ? 2 * ((size_t)iterations + 1) : 2));
    return pl;
}

// the k + 1 stage launches; `sides` workgroup sides
static void ss3_stages(Ss3Args a, int iterations, int sides, bool keep, float* roll0[2], float* roll1[2], float* vstore, float* dstore, size_t P, hipStream_t stream) {
    const dim3 grid((unsigned)((long long)sides * a.s.K * a.s.B * a.s.tiles)), block(SS3_THREADS);
    for (int j = 0; j <= iterations; ++j) {
        a.vin0 = keep ? (j ? vstore + (size_t)(j - 1) * P : nullptr) : roll0[(j + 1) & 1];
        a.vout0 = roll0[j & 1];
        a.vin1 = roll1[(j + 1) & 1];
        a.vout1 = roll1[j & 1];
        a.vsave = keep ? vstore + (size_t)j * P : nullptr;
        a.dsave = keep ? dstore + (size_t)j * P : nullptr;
        with_bool(keep, [&](auto sv) {
            if (j == 0) hipLaunchKernelGGL((ss3_stage_kernel<true, false, sv()>), grid, block, 0, stream, a);
            else if (j < iterations) hipLaunchKernelGGL((ss3_stage_kernel<false, false, sv()>), grid, block, 0, stream, a);
            else hipLaunchKernelGGL((ss3_stage_kernel<false, true, sv()>), grid, block, 0, stream, a);
        });
    }
}

}  // namespace ptb

using namespace ptb;

extern "C" int ptb_soft_skeleton_3d(const float* x, int64_t N, int64_t D, int64_t H, int64_t W, int iterations, float* out, void* workspace,
                                    int64_t workspace_bytes, ptb_stream_t stream) {
    if (!x || !out || !workspace) return PTB_EINVAL;
    Ss3Args a{};
    if (int rc = ss3_problem(N, 1, 1, D, H, W, iterations, 1, a.s)) return rc;
    const size_t P = (size_t)N * (size_t)D * (size_t)H * (size_t)W;
    if (workspace_bytes < 0 || (size_t)workspace_bytes < 8 * P || (reinterpret_cast<uintptr_t>(workspace) & 3u)) return PTB_EINVAL;
    a.s.act = PTB_PROB_IDENTITY;
    a.x = x; a.S0 = out;
    float* roll[2] = {static_cast<float*>(workspace), static_cast<float*>(workspace) + P};
    ss3_stages(a, iterations, 1, false, roll, roll, nullptr, nullptr, P, (hipStream_t)stream);
    return check_launch();
}

extern "C" int64_t ptb_soft_cldice_3d_workspace(int64_t B, int K, int64_t D, int64_t H, int64_t W, int iterations, int keep_grad) {
    Ss3Shape s{};
    if (int rc = ss3_problem(B, 1, K, D, H, W, iterations, 2, s)) return rc;
    return (int64_t)ss3_plan(s, iterations, keep_grad != 0).total_bytes;
}

extern "C" int ptb_soft_cldice_3d_fwd(const float* x, const int64_t* labels, const float* dense, int64_t B, int C, int64_t D, int64_t H, int64_t W,
                                      const int* classes, int K, int prob, int iterations, float smooth, int keep_grad, float* st, void* workspace,
                                      int64_t workspace_bytes, float* loss, float* coef, ptb_stream_t stream) {
    if (!x || (labels != nullptr) == (dense != nullptr) || !st || !workspace || !loss || !coef || ss_bad_prob(prob)) return PTB_EINVAL;
    if (!(smooth >= 0.0f) || !std::isfinite(smooth)) return PTB_EINVAL;
    Ss3Args a{};
    if (int rc = ss_classes(classes, C, K, a.s.cls)) return rc;
    if (int rc = ss3_problem(B, C, K, D, H, W, iterations, 2, a.s)) return rc;
    const bool keep = keep_grad != 0;
    const Ss3Plan pl = ss3_plan(a.s, iterations, keep);
    if (!aligned16(workspace) || workspace_bytes < 0 || (size_t)workspace_bytes < pl.total_bytes) return PTB_EINVAL;
    a.s.act = prob;
    a.x = x; a.labels = reinterpret_cast<const long long*>(labels); a.dense = dense;
    a.slots = reinterpret_cast<double*>(workspace);
    a.S0 = pl.plane(workspace, 0); a.S1 = st;
    float* roll1[2] = {pl.plane(workspace, 1), pl.plane(workspace, 2)};
    float* roll0[2] = {keep ? nullptr : pl.plane(workspace, 3), keep ? nullptr : pl.plane(workspace, 4)};
    float* vstore = keep ? pl.plane(workspace, 3) : nullptr;
    float* dstore = keep ? pl.plane(workspace, 3 + (size_t)iterations + 1) : nullptr;
    hipStream_t s = (hipStream_t)stream;
    ss3_stages(a, iterations, 2, keep, roll0, roll1, vstore, dstore, pl.P, s);
    ss_launch_finish(a.slots, (unsigned)(B * a.s.tiles), K, smooth, loss, coef, s);
    return check_launch();
}

extern "C" int ptb_soft_cldice_3d_bwd(const float* x, const int64_t* labels, const float* dense, int64_t B, int C, int64_t D, int64_t H, int64_t W,
                                      const int* classes, int K, int prob, int iterations, const float* st, const float* coef, const float* upstream,
                                      void* workspace, int64_t workspace_bytes, float* grad, ptb_stream_t stream) {
    if (!x || (labels != nullptr) == (dense != nullptr) || !st || !coef || !upstream || !workspace || !grad || ss_bad_prob(prob)) return PTB_EINVAL;
    Ss3GatherArgs a{};
    if (int rc = ss_classes(classes, C, K, a.s.cls)) return rc;
    if (int rc = ss3_problem(B, C, K, D, H, W, iterations, 1, a.s)) return rc;
    const Ss3Plan pl = ss3_plan(a.s, iterations, true);
    if (!aligned16(workspace) || workspace_bytes < 0 || (size_t)workspace_bytes < pl.total_bytes) return PTB_EINVAL;
    a.s.act = prob;
    const size_t P = pl.P, S = (size_t)D * (size_t)H * (size_t)W;
    float* dp = pl.plane(workspace, 0);
    float* gv[2] = {pl.plane(workspace, 1), pl.plane(workspace, 2)};
    const float* vstore = pl.plane(workspace, 3);
    float* dstore = pl.plane(workspace, 3 + (size_t)iterations + 1);
    hipStream_t s = (hipStream_t)stream;

    Ss3DirectArgs d{};
    d.labels = reinterpret_cast<const long long*>(labels); d.dense = dense; d.coef = coef; d.dstore = dstore;
    d.S = S; d.total = P; d.C = C; d.K = K; d.k = iterations;
    for (int k = 0; k < K; ++k) d.cls[k] = a.s.cls[k];
    hipLaunchKernelGGL(ss3_direct_kernel, dim3((unsigned)((P + SS3_THREADS - 1) / SS3_THREADS)), dim3(SS3_THREADS), 0, s, d);

    const dim3 grid((unsigned)((long long)K * B * a.s.tiles)), block(SS3_THREADS);
    for (int j = iterations; j >= 0; --j) {                                    // gv_j+1 into plane j & 1, from gv_j+2 in the other one
        a.v = vstore + (size_t)j * P;
        a.go = dstore + (size_t)j * P;
        a.own = j < iterations ? dstore + (size_t)(j + 1) * P : nullptr;
        a.gvin = j < iterations ? gv[(j + 1) & 1] : nullptr;
        a.gvout = gv[j & 1];
        hipLaunchKernelGGL((ss3_gather_kernel<false>), grid, block, 0, s, a);
    }
    a.x = x; a.v = nullptr; a.go = nullptr; a.own = dstore; a.gvin = gv[0]; a.gvout = nullptr;
    a.st = st; a.coef = coef; a.dp = dp;
    hipLaunchKernelGGL((ss3_gather_kernel<true>), grid, block, 0, s, a);
    if (int rc = ss_launch_act_bwd(x, dp, upstream, grad, a.s.cls, K, C, prob, (size_t)B, S, s)) return rc;
    return check_launch();
}
