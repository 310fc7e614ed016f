// s2act.hip — gfx950 (CDNA4) kernels for the eSCN/UMA S2 grid activation
// (distmlip_amd/uma_ops.py s2_act), lmax = 2, fp32 operands and fp32
// accumulation on v_mfma_f32_16x16x4_f32:
//
//   k_s2_act<false>   out[n,s,c] = sum_g from_g[s,g] silu(sum_t to_g[g,t] x[n,t,c])
//   k_s2_act<true>    f = to_g x,  q[g] = sum_s from_g[s,g] go[n,s,c],
//                     dx[n,t,c] = sum_g to_g[g,t] silu'(f) q
//
// x, out, go, dx are [N, 9, C]; to_g [G, 9] and from_g [9, G] are the matrices
// of uma_model.s2_grid.  The [N, C, G] grid tensor of the torch composition
// (62 GB at N = 238k, C = 128, G = 512) never exists: a grid value lives in
// one register between two matrix instructions.  The reverse recomputes f and
// saves nothing.
//
// Work split.  The (node, channel) pairs are the columns of one flat
// [9, N.C] problem; a column block is 16 consecutive channels of one node
// (C % 32 == 0, so a block never straddles nodes).  A wave owns NB = 2
// consecutive column blocks (32 consecutive channels of one node) and walks
// the whole grid in tiles of 16 points.  A block of 256 threads is four such
// waves, S2_COLS = 128 columns (one node at C = 128, two at 64, four at 32);
// the waves share nothing, there is no LDS and no barrier.  Across the grid
// loop a wave keeps, per column block, the nine coefficients of x as three B
// fragments (K = 9 padded to 12; the reverse go as well) and four 16x16
// accumulators (rows 9..15 of the padded output side stay zero).
//
// Chaining the two contractions without a transpose.  The expansion is
// computed transposed, D[g, c] = sum_t to_g[g0+g, t] x[t, c], as three
// 16x16x4 steps with A[i = lane%16][k = lane/16] = to_g[g0 + i][4j + k] and
// B[k][c = lane%16] = x[4j + k][c].  Its accumulator leaves lane L with
// channel L%16 and, in register r, grid point g0 + 4(L/16) + r.  That is
// already a B operand of the contraction (B[k = L/16][c = L%16]) for the
// K-slice {g0 + 4k + r, k = 0..3}: step r of the contraction multiplies
// register r by A[s = lane%16][k = lane/16] = from_g[s][g0 + 4k + r], which is
// component r of ONE float4 load from_g[s][g0 + 4k .. +3].  Step r has an
// accumulator of its own: four chains over the tiles, added pairwise at the
// end.  (One chain over all 512 points, G/4 dependent steps, was 8x as far
// from fp64 as the rocBLAS GEMM of the torch path; four chains are 1.1x.)
// The order of the sum over g is fixed and there are no atomics, so a launch
// repeats bit for bit.  The reverse is the same chain
// with two expansions (f from x through to_g, q from go through from_g^T:
// A[g = lane%16][k] = from_g[4j + k][g0 + g]) and to_g^T on the way back
// (A[t = lane%16][k] = to_g[g0 + 4k + r][t]).
// Instructions of different column blocks are interleaved (block index
// innermost), so back-to-back MFMAs never depend on each other.
//
// Grid matrices.  DECISION: streamed, in fragment order, from L2/L1 straight
// into registers; nothing is staged in LDS.  With NB = 2 one set of A
// fragments (forward 3 dwords + 1 float4 per lane, reverse 10 dwords) feeds 14
// (20) MFMAs, i.e. under 2 KB of cache traffic per ~450 matrix-pipe cycles of
// a SIMD, a quarter of what the L1 delivers, and the fragments of tile i+1 are
// requested before the arithmetic of tile i.  The matrices are 36 KB at
// G = 512 and 144 KB at G = 2048 (L2 resident either way); an LDS copy would
// have capped occupancy at G = 512 and would not fit at G = 2048, while this
// form is the same kernel for every G % 32 == 0.  Padding lanes (t, s >= 9)
// load nothing and feed zeros.
//
// silu / silu' are the exact sigmoid and SiLU of kernels.hip (the 14/15-VALU
// short sequences with the wave-uniform fall-back to expf and the IEEE
// division outside |x| <= 87), copied below; one range test covers the 16
// grid values a lane holds per tile.  silu'(f) = sg (1 + f (1 - sg)).
//
// Cost per 16x16 (grid x column) block: forward 7 MFMAs of 8 passes = 224
// matrix-pipe cycles beside 4 x 15 VALU = 240 issue cycles; reverse 10 MFMAs
// = 320 beside about 4 x 20 VALU.  Both pipes are loaded about equally; HBM
// traffic (2 N.9.C.4 bytes forward, 3 N.9.C.4 reverse) is far from binding.
// Measured at N = 238k, C = 128, G = 512 (tests/perf_s2_act.py): 13.1 ms
// forward, 18.6 ms reverse, i.e. 42% of the fp32 matrix peak counting the
// padded MFMAs and 43-45% of the VALU issue rate counting the silu alone:
// the two pipes overlap only in part.  NB = 4 halves the fragment traffic but
// needs 156 / 201 registers (3 / 2 waves per SIMD); not measured.
//
// Resources (hipcc -O3 --offload-arch=gfx950,
// -Rpass-analysis=kernel-resource-usage), no LDS:
//   kernel            VGPR  AGPR  SGPR  scratch  waves/SIMD
//   k_s2_act<fwd>       50    40    32        0           5
//   k_s2_act<bwd>       69    44    32        0           4
// No spill in either kernel, in or outside the grid loop.
//
// The Makefile compiles this file with the packed fp32 VALU forms
// (v_pk_{add,mul,fma}_f32) switched off.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/distmlip_hip.h"

void dm_set_last_error(const char* msg);      // kernels.hip

namespace {

typedef __attribute__((ext_vector_type(4))) float f32x4;

constexpr int BLOCK = 256;
constexpr int NB = 2;                  // 16-column blocks per wave
constexpr int S2_COLS = (BLOCK / 64) * NB * 16;   // columns per block

// ---- exact sigmoid / SiLU, as in kernels.hip ------------------------------
__device__ __forceinline__ float sigf_ref(float x) {
    return 1.0f / (1.0f + expf(-x));
}
__device__ __forceinline__ float siluf_ref(float x) {
    return x / (1.0f + expf(-x));
}

constexpr float ACT_FAST_MAX = 87.0f;

// 1 + expf(-x) for |x| <= ACT_FAST_MAX, in libm's operation order
__device__ __forceinline__ float act_one_plus_exp_neg(float x) {
#pragma clang fp contract(off)
    const float c = -0x1.715476p+0f, cc = -0x1.4ae0bep-26f;  // -log2(e), hi + lo
    const float ph = x * c;
    const float n = __builtin_rintf(ph);
    const float pl = __builtin_fmaf(x, cc, __builtin_fmaf(x, c, -ph));
    const float a = (ph - n) + pl;
    return 1.0f + __builtin_ldexpf(__builtin_amdgcn_exp2f(a), (int)n);
}

template <int N>
__device__ __forceinline__ bool act_wave_in_range(const float (&x)[N]) {
    bool outside = false;
#pragma unroll
    for (int i = 0; i < N; ++i)
        outside |= !(__builtin_fabsf(x[i]) <= ACT_FAST_MAX);
    return __builtin_amdgcn_ballot_w64(outside) == 0;
}

__device__ __forceinline__ float sigf_fast(float x) {
    const float y = act_one_plus_exp_neg(x);
    const float r = __builtin_amdgcn_rcpf(y);
    return __builtin_fmaf(__builtin_fmaf(-y, r, 1.0f), r, r);
}

__device__ __forceinline__ float siluf_fast(float x) {
#pragma clang fp contract(off)
    const float y = act_one_plus_exp_neg(x);
    const float r = __builtin_amdgcn_rcpf(y);
    const float q = x * r;
    // y q - x, negated in the last fma: keeps the sign of a zero x
    return __builtin_fmaf(-__builtin_fmaf(y, q, -x), r, q);
}

// y = silu(x) (!BWD) or y = silu'(x) q (BWD) for the N values of a lane: one
// range test and one wave-uniform branch for all of them
template <bool BWD, bool FAST, int N>
__device__ __forceinline__ void act_sel(const float (&x)[N],
                                        const float (&q)[N], float (&y)[N]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if constexpr (!BWD) {
            y[i] = FAST ? siluf_fast(x[i]) : siluf_ref(x[i]);
        } else {
            const float sg = FAST ? sigf_fast(x[i]) : sigf_ref(x[i]);
            y[i] = q[i] * (sg * (1.0f + x[i] * (1.0f - sg)));
        }
    }
}

template <bool BWD, int N>
__device__ __forceinline__ void act_n(const float (&x)[N], const float (&q)[N],
                                      float (&y)[N]) {
    if (__builtin_expect(act_wave_in_range(x), 1))
        act_sel<BWD, true>(x, q, y);
    else
        act_sel<BWD, false>(x, q, y);
}

// ---- A fragments of one 16-point grid tile --------------------------------
template <bool BWD>
struct Frag {
    float to[3];        // expansion of x:  to_g[g0 + lc][4j + lk]
    f32x4 back;         // fwd contraction: from_g[lc][g0 + 4lk + r]
                        // bwd contraction: to_g[g0 + 4lk + r][lc]
    float ft[BWD ? 3 : 1];   // bwd expansion of go: from_g[4j + lk][g0 + lc]
};

template <bool BWD>
__device__ __forceinline__ void load_frag(Frag<BWD>& a,
                                          const float* __restrict__ to_g,
                                          const float* __restrict__ from_g,
                                          int G, int g0, int lc, int lk) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int t = 4 * j + lk;
        a.to[j] = t < 9 ? to_g[(g0 + lc) * 9 + t] : 0.0f;
        if constexpr (BWD) a.ft[j] = t < 9 ? from_g[t * G + g0 + lc] : 0.0f;
    }
    a.back = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    if (lc < 9) {
        if constexpr (!BWD) {
            a.back = *(const f32x4*)(from_g + lc * G + g0 + 4 * lk);
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                a.back[r] = to_g[(g0 + 4 * lk + r) * 9 + lc];
        }
    }
}

// ncols = N.C.  x / go / out rows of column `col`: n = col / C, c = col % C,
// element (n.9 + t).C + c.
template <bool BWD>
__global__ void __launch_bounds__(BLOCK)
k_s2_act(const float* __restrict__ go, const float* __restrict__ x,
         const float* __restrict__ to_g, const float* __restrict__ from_g,
         float* __restrict__ out, int64_t ncols, int C, int G) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int lc = lane & 15, lk = lane >> 4;
    const int64_t col0 = ((int64_t)blockIdx.x * (BLOCK / 64) + w) * (NB * 16);
    if (col0 >= ncols) return;            // whole wave; there is no barrier

    // per column block: validity (ncols is a multiple of 32, so a block is
    // whole or absent) and the 64-bit offset of (row 0, this lane's channel)
    bool valid[NB];
    int64_t off[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int64_t col = col0 + 16 * b;
        valid[b] = col < ncols;
        const int64_t n = col / C;
        off[b] = n * 9 * C + (col - n * C) + lc;
    }

    // B fragments of the expansions: rows t = 4j + lk (zero for t >= 9)
    float xb[NB][3], gb[BWD ? NB : 1][3];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const int t = 4 * j + lk;
            const bool ok = valid[b] && t < 9;
            xb[b][j] = ok ? x[off[b] + (int64_t)t * C] : 0.0f;
            if constexpr (BWD) gb[b][j] = ok ? go[off[b] + (int64_t)t * C] : 0.0f;
        }

    // one accumulator per contraction step r: four chains of G/16 steps
    // instead of one of G/4, added pairwise at the end (a sequential fp32
    // sum over 512 grid points measured 8x the error of the rocBLAS GEMM)
    f32x4 acc[NB][4];
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[b][r] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int ntile = G / 16;
    Frag<BWD> cur, nxt;
    load_frag<BWD>(cur, to_g, from_g, G, 0, lc, lk);
#pragma unroll 1
    for (int it = 0; it < ntile; ++it) {
        // the last tile prefetches tile 0 again: in bounds, and unused
        load_frag<BWD>(nxt, to_g, from_g, G, it + 1 < ntile ? 16 * (it + 1) : 0,
                       lc, lk);

        f32x4 f[NB], q[BWD ? NB : 1];
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            f[b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if constexpr (BWD) q[b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                f[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(cur.to[j], xb[b][j],
                                                            f[b], 0, 0, 0);
                if constexpr (BWD)
                    q[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        cur.ft[j], gb[b][j], q[b], 0, 0, 0);
            }

        float fv[NB * 4], qv[NB * 4], yv[NB * 4];
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                fv[b * 4 + r] = f[b][r];
                qv[b * 4 + r] = BWD ? q[BWD ? b : 0][r] : 0.0f;
            }
        act_n<BWD>(fv, qv, yv);

#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int b = 0; b < NB; ++b)
                acc[b][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    cur.back[r], yv[b * 4 + r], acc[b][r], 0, 0, 0);
        cur = nxt;
    }

    // accumulator: lane holds channel lc, register r holds row 4 lk + r
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const f32x4 sum = (acc[b][0] + acc[b][1]) + (acc[b][2] + acc[b][3]);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int s = 4 * lk + r;
            if (valid[b] && s < 9) out[off[b] + (int64_t)s * C] = sum[r];
        }
    }
}

template <bool BWD>
int launch_s2(const float* go, const float* x, const float* to_g,
              const float* from_g, float* out, int64_t N, int32_t C, int32_t G,
              hipStream_t s) {
    if (N < 0 || C <= 0 || C % 32 != 0 || G <= 0 || G % 32 != 0) {
        dm_set_last_error("dm_s2_act: C and G must be positive multiples of 32");
        return -1;
    }
    if (N == 0) return 0;
    if (((uintptr_t)go | (uintptr_t)x | (uintptr_t)to_g | (uintptr_t)from_g |
         (uintptr_t)out) & 15) {
        dm_set_last_error("dm_s2_act: pointers must be 16-byte aligned");
        return -1;
    }
    const int64_t ncols = N * C;
    const int64_t nb = (ncols + S2_COLS - 1) / S2_COLS;
    if (nb > INT32_MAX) {
        dm_set_last_error("dm_s2_act: too many nodes for one launch");
        return -1;
    }
    k_s2_act<BWD><<<dim3((unsigned)nb), BLOCK, 0, s>>>(go, x, to_g, from_g, out,
                                                       ncols, C, G);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dm_set_last_error(hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

}  // namespace

extern "C" {

int dm_s2_act_fwd_f32(const float* x, const float* to_g, const float* from_g,
                      float* out, int64_t N, int32_t C, int32_t G,
                      uint64_t stream) {
    return launch_s2<false>(nullptr, x, to_g, from_g, out, N, C, G,
                            (hipStream_t)stream);
}

int dm_s2_act_bwd_f32(const float* go, const float* x, const float* to_g,
                      const float* from_g, float* dx, int64_t N, int32_t C,
                      int32_t G, uint64_t stream) {
    return launch_s2<true>(go, x, to_g, from_g, dx, N, C, G,
                           (hipStream_t)stream);
}

}  // extern "C"
