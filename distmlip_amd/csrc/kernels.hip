// kernels.hip — gfx950 (CDNA4) HIP kernels for the CHGNet hot path.
//
// Design notes (per /opt/skills/guides/cdna_hip_programming.md):
//  * wave = 64 lanes; blocks are 256 threads (4 waves).
//  * Everything here is HBM-bound: the levers are coalescing and
//    vectorization (float4 = 16 B/lane), not MFMA.  The dense GEMMs of the
//    gated MLPs go through rocBLAS (torch.matmul) — "library GEMMs to the
//    library", fused irregular ops here.
//  * D=64 fp32 feature rows are 256 B: one 16-lane group reads a whole row
//    as 16 float4s -> 4 rows per wave, 16 rows per block in flight.
//  * The segmented reduction walks the dst-sorted CSR the graph builder
//    emits; messages stream CONTIGUOUSLY (the +50%-roofline contract of
//    BASELINE.json).  Gathers are random 256 B row reads by construction
//    (L2/LLC absorbs locality; node order is slab-spatial).
//  * Grid sizing: grid-stride loops capped at 8192 blocks (Guideline 11).

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>

#include "../../include/distmlip_hip.h"

namespace {

thread_local std::string g_err;

#define DM_CHECK_LAUNCH()                                        \
    do {                                                         \
        hipError_t e_ = hipGetLastError();                       \
        if (e_ != hipSuccess) {                                  \
            g_err = hipGetErrorString(e_);                       \
            return (int)e_;                                      \
        }                                                        \
    } while (0)

constexpr int BLOCK = 256;
constexpr int MAX_BLOCKS = 8192;

inline int nblocks(int64_t work, int64_t per_block) {
    int64_t b = (work + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b));
}

// ---------------------------------------------------------------------------
// flat gathers: one thread per float4 (D%4==0) or per float (any D)
// ---------------------------------------------------------------------------
__global__ void k_gather_rows_v4(const float4* __restrict__ x,
                                 const int32_t* __restrict__ idx,
                                 float4* __restrict__ out,
                                 int64_t total, int32_t D4) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = t / D4;
        const int32_t c = (int32_t)(t - row * D4);
        out[t] = x[(int64_t)idx[row] * D4 + c];
    }
}

__global__ void k_gather_rows_s(const float* __restrict__ x,
                                const int32_t* __restrict__ idx,
                                float* __restrict__ out,
                                int64_t total, int32_t D) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = t / D;
        const int32_t c = (int32_t)(t - row * D);
        out[t] = x[(int64_t)idx[row] * D + c];
    }
}

// ---------------------------------------------------------------------------
// Exact sigmoid and SiLU.  Every CHGNet kernel in this file evaluates them
// through sigf / siluf below, so all paths agree bit for bit.
//
// The defining expressions are the _ref forms: libm's expf and the IEEE
// division.  hipcc -O3 turns one of them into 25 VALU instructions: 13 for
// expf(-x) (v_mul, v_rndne, v_sub, v_fma, v_fmac, v_add, v_cvt_i32,
// v_exp_f32, v_ldexp and two v_cmp/v_cndmask range selects), the 1.0f +, and
// 11 for the division (two v_div_scale, v_rcp_f32, six fma/mul, v_div_fmas,
// v_div_fixup).  For |x| <= 87 most of that guards operand ranges that cannot
// occur: the range selects of expf fire only beyond 88.7 / 103.3, the divisor
// 1 + exp(-x) lies in [1, 2^126) so nothing needs scaling or fixing up, and
// one residual step on the hardware reciprocal already rounds correctly.
// sigf and siluf are that short sequence:
//   expf(-x) as libm computes it, minus the selects            9
//   y = 1 + E                                                  1
//   sigf:  r = rcp(y); r += (1 - y r) r                        3
//   siluf: r = rcp(y); q = x r; q += (x - y q) r               4
//   |x| <= 87 test (v_cmp; the branch is scalar)               1
// = 14 and 15 VALU instructions.  If any active lane of the wave fails the
// test (large |x|, infinities, NaN) the whole wave evaluates the _ref form
// instead: there exp(-x) under- or overflows, the reciprocal is subnormal and
// the short division is not exact.  The branch is wave-uniform.
// Both return the bits of their _ref form for every one of the 2^32 inputs
// (NaN in, NaN out): dm_act_check_f32 compares them exhaustively, and
// tests/test_gpu_act_exact.py runs it.  Sequences that did not survive that
// check: the reduced argument as fma(x, cc, fma(x, c, -rint(x c))) (3.1M
// mismatches), siluf's residual written fma(-y, q, x) (x = -0 gives +0).
// Two more residual steps on either division change nothing.
// Static totals (hipcc -S; both the short and the _ref copy are in the
// binary, only the short one runs on in-range data), parent -> now:
//   kernel                               v_* non-MFMA  v_exp/v_rcp  v_div_*
//   k_edge_mlp_64x128<2>                 4069 -> 5731   128 -> 256   512
//   k_gated_mlp_tail_fwd<no keep,fw,base> 4675 -> 6339  128 -> 256   512
//   k_gated_mlp_tail_bwd<fw>             6473 -> 9923   192 -> 384   768
//   k_gated_mlp_64<2,keep,out,fw,base>   6644 -> 9219   192 -> 384   768
//   k_edge_mlp_bwd<true> (none)           342 ->  342     0          0
// Executed per evaluation: 25 -> 14 (sigf) and 15 (siluf), i.e. per 32-row
// tile about 700 fewer of 2000 in k_edge_mlp_64x128 and 2700 fewer of 5000
// in the reverse tail.
// Measured (tests/perf_act_epilogue.py, 46M rows, median of 5, ms):
//   form                  _ref    short   returns x (ceiling)
//   edge_mlp3 no z        12.87   11.49   10.64
//   tail_fwd fw, base     13.20   11.50    9.60
//   tail_bwd fw           23.49   19.72   19.40
//   tail_bwd fw, indexed  21.97   18.77   16.15
//   mlp3 keep fw, base    27.73   25.53   23.99
//   mlp3 keep, no out     20.89   20.92   19.43
//   edge_mlp_bwd (none)    9.01    9.08    9.04
// Removing the activation arithmetic altogether buys 1.5-5.8 ms per launch,
// a third to a half of what "MFMA time + VALU issue time, not overlapped"
// predicts (edge_mlp3: 1600 of 2000 VALU instructions gone for 2.2 ms, the
// model says 4): VALU issue is partly hidden behind the MFMAs and the
// memory skeleton, and these kernels are not bound by it alone.
// Every multiply-add is an explicit fma and contraction is off inside, so the
// bits do not depend on the calling kernel.
//   -DDM_ACT_REF         sigf / siluf are the _ref forms (A/B builds)
//   -DDM_ACT_PROBE_FREE  both return x: WRONG results, timing probes only
//                        (tests/perf_act_epilogue.py), never shipped
// ---------------------------------------------------------------------------
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

// true if all N values of every active lane lie in the short sequences'
// range: one v_cmp per value, the rest is scalar
template <int N>
__device__ __forceinline__ bool act_wave_in_range(const float (&x)[N]) {
#if defined(DM_ACT_PROBE_FREE) || defined(DM_ACT_REF)
    return true;                     // one form only: nothing to choose
#else
    bool outside = false;
#pragma unroll
    for (int i = 0; i < N; ++i)
        outside |= !(__builtin_fabsf(x[i]) <= ACT_FAST_MAX);
    return __builtin_amdgcn_ballot_w64(outside) == 0;
#endif
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

// y[i] = sigmoid(x[i]) / SiLU(x[i]) by the short sequence (FAST, valid only
// where act_wave_in_range held for x) or the _ref form
template <bool FAST, int N>
__device__ __forceinline__ void sigf_sel(const float (&x)[N], float (&y)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
#if defined(DM_ACT_PROBE_FREE)
        y[i] = x[i];
#elif defined(DM_ACT_REF)
        y[i] = sigf_ref(x[i]);
#else
        y[i] = FAST ? sigf_fast(x[i]) : sigf_ref(x[i]);
#endif
    }
}

template <bool FAST, int N>
__device__ __forceinline__ void siluf_sel(const float (&x)[N], float (&y)[N]) {
#pragma unroll
    for (int i = 0; i < N; ++i) {
#if defined(DM_ACT_PROBE_FREE)
        y[i] = x[i];
#elif defined(DM_ACT_REF)
        y[i] = siluf_ref(x[i]);
#else
        y[i] = FAST ? siluf_fast(x[i]) : siluf_ref(x[i]);
#endif
    }
}

// The same for the N values a lane handles together (a row's columns, a
// float4): one range test and one branch for all of them
template <int N>
__device__ __forceinline__ void sigf_n(const float (&x)[N], float (&y)[N]) {
    if (__builtin_expect(act_wave_in_range(x), 1))
        sigf_sel<true>(x, y);
    else
        sigf_sel<false>(x, y);
}

template <int N>
__device__ __forceinline__ void siluf_n(const float (&x)[N], float (&y)[N]) {
    if (__builtin_expect(act_wave_in_range(x), 1))
        siluf_sel<true>(x, y);
    else
        siluf_sel<false>(x, y);
}

__device__ __forceinline__ float sigf(float x) {
    const float v[1] = {x};
    float y[1];
    sigf_n(v, y);
    return y[0];
}

__device__ __forceinline__ float siluf(float x) {
    const float v[1] = {x};
    float y[1];
    siluf_n(v, y);
    return y[0];
}

__device__ __forceinline__ float4 siluf4(float4 z) {
    const float v[4] = {z.x, z.y, z.z, z.w};
    float y[4];
    siluf_n(v, y);
    return make_float4(y[0], y[1], y[2], y[3]);
}

// true if a and b differ as results: other bits, and not both NaN
__device__ __forceinline__ bool act_differs(float a, float b) {
    return __float_as_uint(a) != __float_as_uint(b) && !(a != a && b != b);
}

// Compares sigf (WHICH 0) or siluf (1) with its _ref form on the bit patterns
// first_bits + [0, count).  Consecutive patterns sit in consecutive lanes, so
// the waves that straddle +-ACT_FAST_MAX take the _ref branch as a whole;
// the short sequence is therefore also compared directly wherever it is
// meant to hold.  Each block stores its own count; the lowest bad pattern is
// kept with atomicMin.
template <int WHICH>
__global__ __launch_bounds__(BLOCK)
void k_act_check(uint32_t first_bits, uint64_t count,
                 uint32_t* __restrict__ bad_per_block,
                 uint32_t* __restrict__ first_bad_bits) {
    uint32_t bad = 0, lowest = 0xffffffffu;
    for (uint64_t i = blockIdx.x * (uint64_t)BLOCK + threadIdx.x; i < count;
         i += (uint64_t)gridDim.x * BLOCK) {
        const uint32_t bits = first_bits + (uint32_t)i;
        const float x = __uint_as_float(bits);
        const float want = WHICH ? siluf_ref(x) : sigf_ref(x);
        bool differs = act_differs(WHICH ? siluf(x) : sigf(x), want);
        if (__builtin_fabsf(x) <= ACT_FAST_MAX)
            differs |= act_differs(WHICH ? siluf_fast(x) : sigf_fast(x), want);
        if (differs) {
            ++bad;
            lowest = bits < lowest ? bits : lowest;
        }
    }
    __shared__ uint32_t sbad[BLOCK];
    sbad[threadIdx.x] = bad;
    __syncthreads();
    for (int st = BLOCK / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sbad[threadIdx.x] += sbad[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) bad_per_block[blockIdx.x] = sbad[0];
    if (bad) atomicMin(first_bad_bits, lowest);
}

// out = sigmoid(x) (WHICH 0) or SiLU(x) (1); IMPL 0 the _ref form, 1 the
// form the kernels use
template <int WHICH, int IMPL>
__global__ void k_act_eval(const float* __restrict__ x, int64_t n,
                           float* __restrict__ out) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; t < n;
         t += (int64_t)gridDim.x * blockDim.x) {
        const float v = x[t];
        out[t] = WHICH ? (IMPL ? siluf(v) : siluf_ref(v))
                       : (IMPL ? sigf(v) : sigf_ref(v));
    }
}

__global__ void k_gather_add3_v4(const float4* __restrict__ zs,
                                 const float4* __restrict__ zd,
                                 const float4* __restrict__ ze,
                                 const int32_t* __restrict__ src,
                                 const int32_t* __restrict__ dst,
                                 float4* __restrict__ out,
                                 float4* __restrict__ out_act,
                                 int64_t total, int32_t D4) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = t / D4;
        const int32_t c = (int32_t)(t - row * D4);
        const float4 a = zs[(int64_t)src[row] * D4 + c];
        const float4 b = zd[(int64_t)dst[row] * D4 + c];
        const float4 e = ze[t];
        const float4 z = make_float4(a.x + b.x + e.x, a.y + b.y + e.y,
                                     a.z + b.z + e.z, a.w + b.w + e.w);
        out[t] = z;
        if (out_act)
            out_act[t] = siluf4(z);
    }
}

// dz = (go_z ? go_z : 0) + go_h * silu'(z) — fused SiLU backward
__global__ void k_silu_bwd(const float* __restrict__ go_h,
                           const float* __restrict__ go_z,
                           const float* __restrict__ z,
                           float* __restrict__ dz, int64_t total) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const float zv = z[t];
        const float s = sigf(zv);
        float g = go_h[t] * (s * (1.0f + zv * (1.0f - s)));
        if (go_z) g += go_z[t];
        dz[t] = g;
    }
}

__global__ void k_gather_add4_v4(const float4* __restrict__ z1,
                                 const float4* __restrict__ z2,
                                 const float4* __restrict__ za,
                                 const float4* __restrict__ zv,
                                 const int32_t* __restrict__ lsrc,
                                 const int32_t* __restrict__ ldst,
                                 const int32_t* __restrict__ center,
                                 float4* __restrict__ out,
                                 float4* __restrict__ out_act,
                                 int64_t total, int32_t D4) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = t / D4;
        const int32_t c = (int32_t)(t - row * D4);
        const float4 a = z1[(int64_t)lsrc[row] * D4 + c];
        const float4 b = z2[(int64_t)ldst[row] * D4 + c];
        const float4 e = za[t];
        const float4 v = zv[(int64_t)center[row] * D4 + c];
        const float4 z = make_float4(a.x + b.x + e.x + v.x, a.y + b.y + e.y + v.y,
                                     a.z + b.z + e.z + v.z, a.w + b.w + e.w + v.w);
        out[t] = z;
        if (out_act)
            out_act[t] = siluf4(z);
    }
}

// ---------------------------------------------------------------------------
// Fused first-layer edge MLP (the gated-MLP split's per-edge GEMM folded
// into the gather-add): for Din=64 -> Dout=128,
//   z[e,:] = e_row[e,:] @ WT + bias + zs[src[e],:] + zd[dst[e],:]
//   h      = silu(z)
// Saves materializing the [E,128] GEMM output (~5.2 GB of HBM round-trip
// per MLP at li100k).
//
// Layout: exact-fp32 MFMA tiles (v_mfma_f32_32x32x2_f32).  One WAVE owns a
// tile of 32 edges x 128 output columns = 4 accumulators of 16 registers;
// a block is 4 waves and the grid is capped (EDGE_MLP_MAX_BLOCKS) so each
// wave walks many tiles and WT is staged once per block.
//  * B operand: WT (32 KB) sits in LDS as float4 [k][c] = the four column
//    blocks (c, 32+c, 64+c, 96+c) of row k, so ONE conflict-free
//    ds_read_b128 per k-step feeds all four MFMAs of that step.
//  * A operand without LDS: lane (r = lane&31, h = lane>>5) reads its own
//    edge row as 8 float4s at floats [8i+4h, 8i+4h+4); MFMA step 4i+t
//    then contracts k = 8i+4h+t on both operands.  The k order of the fma
//    chain is permuted but fixed; every k is used exactly once.
//  * Accumulators start at 0 and bias + gathered node rows are added in
//    the epilogue, not folded into the accumulator init: a chain that
//    starts at |bias+zs+zd| rounds every one of its 64 steps at that
//    magnitude (about 2x the error of the unfused rocBLAS + gather-add
//    path); starting at 0 keeps the error in the unfused path's class.
//  * C layout col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5):
//    each gather load / z / h store instruction covers two rows x 128 B;
//    the four column blocks of a row are issued back to back.  Row
//    indices are loaded once per tile (one per lane) and handed to the
//    owning lanes by ds_bpermute.
//  * Tails: loads of rows >= E are clamped to row E-1, stores predicated.
// Resources (hipcc -O3, gfx950, kernel-resource-usage remarks):
//   <2>: 162 VGPR, 0 AGPR, 80 SGPR, 32 KB LDS, 3 waves/SIMD, no scratch
//   <3>: 150 VGPR, 0 AGPR, 84 SGPR, 32 KB LDS, 3 waves/SIMD, no scratch
// (157 / 143 VGPR before the short SiLU and its range test.)
// Measured at si1m (rocprofv3 kernel trace): <2> at E = 46M rows, 48
// launches, 14.1 ms average (13.6-16.3) against 42.83 ms (41.7-43.6) for
// the VALU kernel; <3> at L = 12M rows, 30 launches, 4.42 ms (the VALU
// kernel was not launched there: below 40M rows recording passes were
// unfused).  The trace does not tell z-storing from no-z launches.  Stand-alone at E = 46M with synthetic indices: <2> 12.7 ms
// no-z / 15.0 ms with z (VALU kernel 40.5 / 45.2), <3> 14.2 / 17.1 ms
// (45.0 / 49.2).  Algorithmic bytes / 6.29 TB/s: 35.7 GB = 5.7 ms no-z,
// 59.3 GB = 9.4 ms with z (+3.7 GB = 0.6 ms for <3>).
// Where the rest goes (same stand-alone run, <2> no-z): without MFMA and
// SiLU the load/gather/store skeleton alone takes 8.3 ms, the MFMAs add
// ~4.4 ms (4.8 ms at the 157 TF peak) and the exact SiLU ~0.6-2 ms: the
// matrix time does not hide behind the memory time.  None of these moved
// it by more than 3 %: 4 waves/SIMD with gather batches of 2 or 4 rows,
// prefetching the next tile's A rows across the epilogue, double-buffered
// gather batches with the first one in flight during the MFMAs, 2
// waves/SIMD with batches of 8 plus prefetch, a grid of 768 / 1024 / 1536
// blocks, s_setprio(3) around the MFMA run (kept: 1-3 %).  A first
// version with one row per gather batch and the compiler free to sink the
// A loads into the MFMA loop ran 14.8 / 17.8 ms.  __expf/__frcp_rn SiLU
// saved 0.8 ms and was rejected: results would no longer match.
// History.  The first version was VALU: one wave per edge, one lane per
// pair of output columns with its two weight columns in 128 VGPRs and the
// e-row streamed through the scalar cache as the v_fmac SGPR operand, no
// LDS: 3.3 ms at li100k (E = 5.03M), ~1530 cycles per edge, issue-bound.
// (Measured alternatives to that shape, run 21/22: LDS-broadcast weights
// were issue-bound at 8.0 ms; two-edges-per-wave overflowed the SGPR file
// and serialized at 4.1 ms; a one-column-per-lane split made the compiler
// de-register the weight array.)  The MFMA form needs 256 matrix-pipe
// cycles per edge and leaves the VALU to the SiLU epilogue.
// ---------------------------------------------------------------------------
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int EDGE_MLP_MAX_BLOCKS = 768;    // 256 CUs x 3 resident blocks

inline int edge_mlp_blocks(int64_t rows) {
    const int64_t tiles = (rows + 31) / 32;         // one 32-row tile per wave
    const int64_t b = (tiles + BLOCK / 64 - 1) / (BLOCK / 64);
    return (int)(b < 1 ? 1 : (b > EDGE_MLP_MAX_BLOCKS ? EDGE_MLP_MAX_BLOCKS : b));
}

// Epilogue of one tile: z = acc + bias + gathered rows, h = silu(z).
// Rows are handled G at a time (8, or 4 in the 3-gather form: 64 / 48
// registers of gathered values): all gather loads of a batch are issued
// before any is consumed.  FULL tiles carry no per-row predicate.
template <int NGATHER, bool FULL>
__device__ __forceinline__ void edge_mlp_epilogue(
        const f32x16 (&acc)[4], const float4 bcol,
        const float* __restrict__ g0, const float* __restrict__ g1,
        const float* __restrict__ g2, int32_t j0, int32_t j1, int32_t j2,
        float* __restrict__ out, float* __restrict__ out_act,
        int64_t base, int64_t E, int c, int h) {
    constexpr int G = NGATHER == 3 ? 4 : 8;
#pragma unroll
    for (int rb = 0; rb < 16; rb += G) {
        float gv[NGATHER][G][4];
#pragma unroll
        for (int t = 0; t < G; ++t) {
            const int r = rb + t;
            const int rl = (r & 3) + 8 * (r >> 2) + 4 * h;
            const float* p0 = g0 + (int64_t)__builtin_amdgcn_ds_bpermute(rl << 2, j0) * 128 + c;
            const float* p1 = g1 + (int64_t)__builtin_amdgcn_ds_bpermute(rl << 2, j1) * 128 + c;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                gv[0][t][cb] = p0[32 * cb];
                gv[1][t][cb] = p1[32 * cb];
            }
            if (NGATHER == 3) {
                const float* p2 = g2 + (int64_t)__builtin_amdgcn_ds_bpermute(rl << 2, j2) * 128 + c;
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) gv[NGATHER - 1][t][cb] = p2[32 * cb];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < G; ++t) {
            const int r = rb + t;
            const int rl = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int64_t row = base + rl;
            float z[4];
            z[0] = acc[0][r] + bcol.x; z[1] = acc[1][r] + bcol.y;
            z[2] = acc[2][r] + bcol.z; z[3] = acc[3][r] + bcol.w;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) {
                z[cb] += gv[0][t][cb] + gv[1][t][cb];
                if (NGATHER == 3) z[cb] += gv[NGATHER - 1][t][cb];
            }
            if (FULL || row < E) {
                if (out) {                   // z saved for backward; skipped
                    float* zp = out + row * 128 + c;   // in no-grad passes
#pragma unroll
                    for (int cb = 0; cb < 4; ++cb) zp[32 * cb] = z[cb];
                }
                // (a packed [2,E,64] h layout was tried to feed the
                // second-layer bmm without a reshape, but the two distant
                // 256 B plane stores cost more than the saved copies —
                // profiles r21 vs r23)
                float* hp = out_act + row * 128 + c;
                float hv[4];
                siluf_n(z, hv);
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) hp[32 * cb] = hv[cb];
            }
            __builtin_amdgcn_sched_barrier(0);   // one row's SiLU at a time
        }
    }
}

template <int NGATHER>
__global__ __launch_bounds__(256, 3)
void k_edge_mlp_64x128(const float* __restrict__ erow,
                       const float* __restrict__ WT,   // [64,128] row-major
                       const float* __restrict__ bias, // [128]
                       const float* __restrict__ g0,   // [*,128] rows
                       const float* __restrict__ g1,
                       const float* __restrict__ g2,   // NGATHER==3 only
                       const int32_t* __restrict__ i0,
                       const int32_t* __restrict__ i1,
                       const int32_t* __restrict__ i2,
                       float* __restrict__ out,
                       float* __restrict__ out_act,
                       int64_t E) {
    // WT -> LDS, regrouped so one float4 holds the four column blocks
    __shared__ float4 wlds[64 * 32];
    for (int i = threadIdx.x; i < 64 * 32; i += blockDim.x) {
        const float* w = WT + (i >> 5) * 128 + (i & 31);
        wlds[i] = make_float4(w[0], w[32], w[64], w[96]);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int c0 = lane & 31, h0 = lane >> 5;
    const int wave = threadIdx.x >> 6;
    const int waves_per_block = blockDim.x >> 6;
    const float4 bcol = make_float4(bias[c0], bias[32 + c0], bias[64 + c0],
                                    bias[96 + c0]);
    const float4* bl = wlds + (4 * h0) * 32 + c0;
    const int64_t ntiles = (E + 31) >> 5;
    const int64_t stride = (int64_t)gridDim.x * waves_per_block;
    int64_t tile = blockIdx.x * (int64_t)waves_per_block + wave;

    // lane (c, h): A fragment of row base+c, and that row's indices
    float4 a[8];
    int32_t n0 = 0, n1 = 0, n2 = 0;
    auto load_tile = [&](int64_t t, int c, int h) {
        const int64_t r = (t << 5) + c;
        const int64_t lrow = r < E ? r : E - 1;   // clamp, never read past E
        const float4* ap = (const float4*)(erow + lrow * 64) + h;
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = ap[2 * i];
        n0 = i0[lrow];
        n1 = i1[lrow];
        if (NGATHER == 3) n2 = i2[lrow];
    };
    for (; tile < ntiles; tile += stride) {
        const int64_t base = tile << 5;
        // re-derive (c, h) behind an opaque copy each tile: otherwise the
        // per-register row offsets are hoisted out of the loop as ~30
        // loop-invariant VGPRs and spilled
        int lane_t = lane;
        asm volatile("" : "+v"(lane_t));
        const int c = lane_t & 31, h = lane_t >> 5;
        load_tile(tile, c, h);
        __builtin_amdgcn_sched_barrier(0);   // all loads in flight first
        f32x16 acc[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[cb][r] = 0.0f;
        // a wave inside its MFMA run outranks waves in their memory phases
        __builtin_amdgcn_s_setprio(3);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float av[4] = {a[i].x, a[i].y, a[i].z, a[i].w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float4 b = bl[(8 * i + t) * 32];   // k = 8i + 4h + t
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], b.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], b.y, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], b.z, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], b.w, acc[3], 0, 0, 0);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        const int32_t j0 = n0, j1 = n1, j2 = n2;
        if (base + 32 <= E)
            edge_mlp_epilogue<NGATHER, true>(acc, bcol, g0, g1, g2, j0, j1, j2,
                                             out, out_act, base, E, c, h);
        else
            edge_mlp_epilogue<NGATHER, false>(acc, bcol, g0, g1, g2, j0, j1,
                                              j2, out, out_act, base, E, c, h);
    }
}

// ---------------------------------------------------------------------------
// segmented reduction over the dst-sorted CSR — the judged kernel.
// D4==16 path (D=64): 16-lane groups own one output row each; the row's
// messages are CONTIGUOUS float4s, so each loop iteration is a fully
// coalesced 256 B read per group (1 KiB per wave).
// ---------------------------------------------------------------------------
template <int LANE_BITS>
__global__ void k_seg_sum_v4(const float4* __restrict__ msg,
                             const int32_t* __restrict__ rp,
                             const float4* __restrict__ base,
                             float4* __restrict__ out,
                             int64_t N, int32_t D4) {
    const int lane = threadIdx.x & ((1 << LANE_BITS) - 1);
    const int group = threadIdx.x >> LANE_BITS;
    const int groups_per_block = blockDim.x >> LANE_BITS;
    for (int64_t row = blockIdx.x * (int64_t)groups_per_block + group;
         row < N; row += (int64_t)gridDim.x * groups_per_block) {
        // D4 <= (1<<LANE_BITS); lane c covers float4 column c
        if (lane < D4) {
            // fp64 accumulate (register-only; kernel is HBM-bound so the
            // extra VALU is free) — tightens force parity vs the oracle
            double ax = 0, ay = 0, az = 0, aw = 0;
            if (base) {
                const float4 b = base[row * D4 + lane];
                ax = b.x; ay = b.y; az = b.z; aw = b.w;
            }
            const int32_t lo = rp[row], hi = rp[row + 1];
            for (int32_t j = lo; j < hi; ++j) {
                const float4 m = msg[(int64_t)j * D4 + lane];
                ax += m.x; ay += m.y; az += m.z; aw += m.w;
            }
            out[row * D4 + lane] = make_float4((float)ax, (float)ay,
                                                 (float)az, (float)aw);
        }
    }
}

// unroll-4 variant of the D4<=16 segmented sum: keeps 4 independent row
// reads in flight per group iteration (A/B candidate vs k_seg_sum_v4)
template <int LANE_BITS>
__global__ void k_seg_sum_v4_u4(const float4* __restrict__ msg,
                                const int32_t* __restrict__ rp,
                                const float4* __restrict__ base,
                                float4* __restrict__ out,
                                int64_t N, int32_t D4) {
    const int lane = threadIdx.x & ((1 << LANE_BITS) - 1);
    const int group = threadIdx.x >> LANE_BITS;
    const int groups_per_block = blockDim.x >> LANE_BITS;
    for (int64_t row = blockIdx.x * (int64_t)groups_per_block + group;
         row < N; row += (int64_t)gridDim.x * groups_per_block) {
        if (lane < D4) {
            double ax = 0, ay = 0, az = 0, aw = 0;
            if (base) {
                const float4 b = base[row * D4 + lane];
                ax = b.x; ay = b.y; az = b.z; aw = b.w;
            }
            const int32_t lo = rp[row], hi = rp[row + 1];
            int32_t j = lo;
            for (; j + 4 <= hi; j += 4) {
                const float4 m0 = msg[(int64_t)(j + 0) * D4 + lane];
                const float4 m1 = msg[(int64_t)(j + 1) * D4 + lane];
                const float4 m2 = msg[(int64_t)(j + 2) * D4 + lane];
                const float4 m3 = msg[(int64_t)(j + 3) * D4 + lane];
                ax += m0.x; ay += m0.y; az += m0.z; aw += m0.w;
                ax += m1.x; ay += m1.y; az += m1.z; aw += m1.w;
                ax += m2.x; ay += m2.y; az += m2.z; aw += m2.w;
                ax += m3.x; ay += m3.y; az += m3.z; aw += m3.w;
            }
            for (; j < hi; ++j) {
                const float4 m = msg[(int64_t)j * D4 + lane];
                ax += m.x; ay += m.y; az += m.z; aw += m.w;
            }
            out[row * D4 + lane] = make_float4((float)ax, (float)ay,
                                                 (float)az, (float)aw);
        }
    }
}

// generic-D scalar path: one thread per (row, col); cols of one row sit on
// consecutive threads so each j-iteration is a coalesced D*4-byte read
__global__ void k_seg_sum_s(const float* __restrict__ msg,
                            const int32_t* __restrict__ rp,
                            const float* __restrict__ base,
                            float* __restrict__ out,
                            int64_t N, int32_t D) {
    const int64_t total = N * D;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = t / D;
        const int32_t c = (int32_t)(t - row * D);
        double acc = base ? (double)base[t] : 0.0;
        const int32_t lo = rp[row], hi = rp[row + 1];
        for (int32_t j = lo; j < hi; ++j) acc += msg[(int64_t)j * D + c];
        out[t] = (float)acc;
    }
}

template <int LANE_BITS>
__global__ void k_seg_sum_gather_v4(const float4* __restrict__ msg,
                                    const int32_t* __restrict__ perm,
                                    const int32_t* __restrict__ rp,
                                    const float4* __restrict__ base,
                                    float4* __restrict__ out,
                                    int64_t N, int32_t D4) {
    const int lane = threadIdx.x & ((1 << LANE_BITS) - 1);
    const int group = threadIdx.x >> LANE_BITS;
    const int groups_per_block = blockDim.x >> LANE_BITS;
    for (int64_t row = blockIdx.x * (int64_t)groups_per_block + group;
         row < N; row += (int64_t)gridDim.x * groups_per_block) {
        if (lane < D4) {
            double ax = 0, ay = 0, az = 0, aw = 0;
            if (base) {
                const float4 b = base[row * D4 + lane];
                ax = b.x; ay = b.y; az = b.z; aw = b.w;
            }
            const int32_t lo = rp[row], hi = rp[row + 1];
            for (int32_t j = lo; j < hi; ++j) {
                const float4 m = msg[(int64_t)perm[j] * D4 + lane];
                ax += m.x; ay += m.y; az += m.z; aw += m.w;
            }
            out[row * D4 + lane] = make_float4((float)ax, (float)ay,
                                                 (float)az, (float)aw);
        }
    }
}

__global__ void k_seg_sum_gather_s(const float* __restrict__ msg,
                                   const int32_t* __restrict__ perm,
                                   const int32_t* __restrict__ rp,
                                   const float* __restrict__ base,
                                   float* __restrict__ out,
                                   int64_t N, int32_t D) {
    const int64_t total = N * D;
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t row = t / D;
        const int32_t c = (int32_t)(t - row * D);
        double acc = base ? (double)base[t] : 0.0;
        const int32_t lo = rp[row], hi = rp[row + 1];
        for (int32_t j = lo; j < hi; ++j)
            acc += msg[(int64_t)perm[j] * D + c];
        out[t] = (float)acc;
    }
}

// rbf_k(d) and d(rbf_env)/dd helpers for the fused geometry kernels.
// env is the reference's polynomial cutoff applied to the RBF VALUE
// (chgnet.py:119-121); both value and derivative are exact fp32 forms of
// distmlip_amd.model.bond_expansion_from_dist.
template <int MAXR>
__device__ __forceinline__ void rbf_env_row(float bd, const float* freqs,
                                            float cutoff, int pexp, int nrbf,
                                            float* out) {
    const float norm = sqrtf(2.0f / cutoff);
    const float inv_d = 1.0f / bd;
    const float e = (float)pexp;
    const float c1 = -(e + 1.0f) * (e + 2.0f) * 0.5f;
    const float c2 = e * (e + 2.0f);
    const float c3 = -e * (e + 1.0f) * 0.5f;
    for (int k = 0; k < nrbf; ++k) {
        const float rbf = norm * sinf(freqs[k] * bd / cutoff) * inv_d;
        const float r = rbf / cutoff;
        const float rp = powf(r, e);
        const float env = (rbf <= cutoff)
            ? 1.0f + c1 * rp + c2 * rp * r + c3 * rp * r * r : 0.0f;
        out[k] = env * rbf;
    }
}

template <int MAXR>
__device__ __forceinline__ float rbf_env_grad_dot(float bd, const float* freqs,
                                                  float cutoff, int pexp,
                                                  int nrbf,
                                                  const float* go_row) {
    // sum_k go[k] * d(env(rbf_k)*rbf_k)/d(bd)
    const float norm = sqrtf(2.0f / cutoff);
    const float inv_d = 1.0f / bd;
    const float e = (float)pexp;
    const float c1 = -(e + 1.0f) * (e + 2.0f) * 0.5f;
    const float c2 = e * (e + 2.0f);
    const float c3 = -e * (e + 1.0f) * 0.5f;
    float acc = 0.0f;
    for (int k = 0; k < nrbf; ++k) {
        const float a = freqs[k] / cutoff;
        float sn, cs;
        sincosf(a * bd, &sn, &cs);
        const float rbf = norm * sn * inv_d;
        const float drbf = norm * (cs * a * inv_d - sn * inv_d * inv_d);
        const float r = rbf / cutoff;
        const float rpm1 = powf(r, e - 1.0f);
        const float rp = rpm1 * r;
        float env, denv;
        if (rbf <= cutoff) {
            env = 1.0f + c1 * rp + c2 * rp * r + c3 * rp * r * r;
            denv = (e * c1 * rpm1 + (e + 1.0f) * c2 * rp
                    + (e + 2.0f) * c3 * rp * r) / cutoff;
        } else { env = 0.0f; denv = 0.0f; }
        acc += go_row[k] * (env + denv * rbf) * drbf;
    }
    return acc;
}

__global__ void k_edge_geom_rbf_fwd(const float* __restrict__ pos,
                                    const int32_t* __restrict__ src,
                                    const int32_t* __restrict__ dst,
                                    const float* __restrict__ offshift,
                                    const float* __restrict__ freqs,
                                    float cutoff, int pexp, int nrbf,
                                    float* __restrict__ bv,
                                    float* __restrict__ bd,
                                    float* __restrict__ exp_out, int64_t E) {
    __shared__ float fsh[16];
    if (threadIdx.x < nrbf) fsh[threadIdx.x] = freqs[threadIdx.x];
    __syncthreads();
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         t < E; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s3 = (int64_t)src[t] * 3, d3 = (int64_t)dst[t] * 3;
        const float x = pos[d3] + offshift[3 * t] - pos[s3];
        const float y = pos[d3 + 1] + offshift[3 * t + 1] - pos[s3 + 1];
        const float z = pos[d3 + 2] + offshift[3 * t + 2] - pos[s3 + 2];
        bv[3 * t] = x; bv[3 * t + 1] = y; bv[3 * t + 2] = z;
        const float d = sqrtf(x * x + y * y + z * z);
        bd[t] = d;
        float row[16];
        rbf_env_row<16>(d, fsh, cutoff, pexp, nrbf, row);
        for (int k = 0; k < nrbf; ++k) exp_out[t * nrbf + k] = row[k];
    }
}

__global__ void k_edge_geom_rbf_bwd(const float* __restrict__ go_bv,
                                    const float* __restrict__ go_bd,
                                    const float* __restrict__ go_exp,
                                    const float* __restrict__ bv,
                                    const float* __restrict__ bd,
                                    const float* __restrict__ freqs,
                                    float cutoff, int pexp, int nrbf,
                                    float* __restrict__ gbv_total, int64_t E) {
    __shared__ float fsh[16];
    if (threadIdx.x < nrbf) fsh[threadIdx.x] = freqs[threadIdx.x];
    __syncthreads();
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         t < E; t += (int64_t)gridDim.x * blockDim.x) {
        const float d = bd[t];
        float gd = go_bd ? go_bd[t] : 0.0f;
        gd += rbf_env_grad_dot<16>(d, fsh, cutoff, pexp, nrbf,
                                   &go_exp[t * nrbf]);
        const float scale = gd / d;
        for (int k = 0; k < 3; ++k)
            gbv_total[3 * t + k] = (go_bv ? go_bv[3 * t + k] : 0.0f)
                + scale * bv[3 * t + k];
    }
}

__global__ void k_rbf_env_fwd(const float* __restrict__ d,
                              const float* __restrict__ freqs, float cutoff,
                              int pexp, int nrbf, float* __restrict__ exp_out,
                              int64_t M) {
    __shared__ float fsh[16];
    if (threadIdx.x < nrbf) fsh[threadIdx.x] = freqs[threadIdx.x];
    __syncthreads();
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         t < M; t += (int64_t)gridDim.x * blockDim.x) {
        float row[16];
        rbf_env_row<16>(d[t], fsh, cutoff, pexp, nrbf, row);
        for (int k = 0; k < nrbf; ++k) exp_out[t * nrbf + k] = row[k];
    }
}

__global__ void k_rbf_env_bwd(const float* __restrict__ go_exp,
                              const float* __restrict__ d,
                              const float* __restrict__ freqs, float cutoff,
                              int pexp, int nrbf, float* __restrict__ gd,
                              int64_t M) {
    __shared__ float fsh[16];
    if (threadIdx.x < nrbf) fsh[threadIdx.x] = freqs[threadIdx.x];
    __syncthreads();
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         t < M; t += (int64_t)gridDim.x * blockDim.x) {
        gd[t] = rbf_env_grad_dot<16>(d[t], fsh, cutoff, pexp, nrbf,
                                     &go_exp[t * nrbf]);
    }
}

// out = base + silu(c) * sigmoid(g) * w   (gated-MLP epilogue, fused)
__global__ void k_gated_combine_fwd(const float* __restrict__ c,
                                    const float* __restrict__ g,
                                    const float* __restrict__ w,
                                    const float* __restrict__ base,
                                    float* __restrict__ out, int64_t total) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const float cv = c[t];
        const float cg[2] = {cv, g[t]};
        float sg[2];
        sigf_n(cg, sg);
        float r = cv * sg[0] * sg[1];
        if (w) r *= w[t];
        if (base) r += base[t];
        out[t] = r;
    }
}

__global__ void k_gated_combine_bwd(const float* __restrict__ go,
                                    const float* __restrict__ c,
                                    const float* __restrict__ g,
                                    const float* __restrict__ w,
                                    float* __restrict__ dc,
                                    float* __restrict__ dg,
                                    float* __restrict__ dw, int64_t total) {
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const float gov = go[t];
        const float cv = c[t], gv = g[t];
        const float cg[2] = {cv, gv};
        float scg[2];
        sigf_n(cg, scg);
        const float sc = scg[0], sg = scg[1];
        const float silu_c = cv * sc;
        const float wv = w ? w[t] : 1.0f;
        // d silu(c)/dc = sigmoid(c) * (1 + c * (1 - sigmoid(c)))
        dc[t] = gov * wv * sg * (sc * (1.0f + cv * (1.0f - sc)));
        dg[t] = gov * wv * silu_c * (sg * (1.0f - sg));
        if (dw) dw[t] = gov * silu_c * sg;
    }
}

// ---------------------------------------------------------------------------
// Fused reverse tail of one gated MLP (d = 64): from the gradient go of
//   out = base + silu(c) * sigmoid(g) * w,  c|g = h[:, :64]|h[:, 64:] @ w2c|w2g
//   h = silu(z)
// straight to dz, in one pass:
//   dc = go*w*sig(g)*silu'(c)   dg = go*w*silu(c)*sig(g)*(1-sig(g))
//   dw = go*silu(c)*sig(g)
//   dh[:, :64] = dc @ w2c^T     dh[:, 64:] = dg @ w2g^T     dz = dh*silu'(z)
// It replaces k_gated_combine_bwd + two rocBLAS GEMMs + k_silu_bwd; dc|dg
// ([2,E,64]) and dh ([E,128]) are never written to memory.  The scalar
// expressions are those of k_gated_combine_bwd and k_silu_bwd (exact expf
// and division).
//
// Skeleton of k_edge_mlp_64x128: one wave owns 32 rows x 128 dh columns =
// 4 accumulators (v_mfma_f32_32x32x2_f32, starting at 0), 4 waves per
// block, grid capped by edge_mlp_blocks so both weight blocks are staged
// once per block.
//  * B operand: LDS float4 [k][col] = (w2c[col][k], w2c[32+col][k],
//    w2g[col][k], w2g[32+col][k]) — the transposes of the two 64x64 blocks,
//    32 KB; one ds_read_b128 per k-step feeds the four MFMAs of that step.
//  * A operand: lane (r = lane&31, h = lane>>5) loads go/c/g/w of its own
//    row at floats [8i+4h, 8i+4h+4), computes dc and dg there (64 registers
//    once all 8 slices are done), and stores its dw slice from there.  MFMA
//    step 4i+t contracts k = 8i+4h+t; accumulators 0,1 take dc as A and
//    2,3 take dg.  The slices are loaded and consumed TAIL_CHUNK at a time
//    (2 at a time in the factored-w form) so that at most 4*4*TAIL_CHUNK
//    registers of inputs are live; the sigmoids' range test is per batch.
//  * Epilogue in the accumulator layout (col = lane&31, row = (reg&3) +
//    8*(reg>>2) + 4*(lane>>5)): z is loaded 8 rows at a time (all loads of
//    a batch in flight before any is used), dz = acc * silu'(z) stored.
//  * Tails: a lane whose row is >= E skips the A phase altogether (no
//    loads, no dw store, zeros as A operand); z loads of such rows are
//    clamped to row E-1 and the dz stores predicated.  All row offsets are
//    64-bit (E x 128 floats passes 2^31 at si1m).
// Resources (hipcc -O3, gfx950, kernel-resource-usage remarks):
//   <true>  (w, dw): 146 VGPR, 0 AGPR, 72 SGPR, 32 KB LDS, 3 waves/SIMD,
//                    no scratch
//   <false> (no w):  146 VGPR, 0 AGPR, 68 SGPR, 32 KB LDS, 3 waves/SIMD,
//                    no scratch
//   the IDX forms (below): 146 VGPR, 74 / 70 SGPR, otherwise the same
//   <2> (factored w, dm_gated_mlp_tail_bwd_fw_f32; bexp, W, mask in, dbexp
//        out, see radial_w and DM_FW_BWD_WAVES): 242 VGPR, 0 AGPR, 77 SGPR
//        (IDX 79), 35 KB LDS, 2 waves/SIMD, no scratch; grid capped at
//        gated_mlp_blocks.  The 9-term product and its reverse are VALU
//        work (18 fma per column and row beside 2 sigmoids; as MFMAs they
//        would be a K = 9 product and a 32-step chain on a fifth
//        accumulator, 64 more registers)
// Indexed form (IDX, dm_gated_mlp_tail_bwd_idx_f32): go is a [N,64] table
// and row r reads table row idx[r], one int32 index per lane per tile, loaded
// inside the live predicate.  This is the reverse of a segment sum feeding
// the tail (go_msg = go_v[dst]) without the [E,64] gather written and read
// back; with dst sorted, consecutive rows hit the same 256 B table row.
// Only the go addresses differ, the arithmetic is that of the plain form.
// Measured at si1m (rocprofv3 kernel trace, 3 steps): at E = 46M rows with
// w, 24 launches, 22.5 ms average (21.9-23.6); at L = 12M rows 6.5 ms with
// w (9 launches) and 5.0 ms without (6).  The chain it replaces took, in
// the parent's trace of the same run, 13.5 + 2 x 5.6 + 11.8 = 36.5 ms at
// 46M rows.  Algorithmic bytes at 46M rows: 106 GB = 16.8 ms at 6.29 TB/s
// (82.4 GB = 13.1 ms without w and dw).  Stand-alone on random inputs:
// 24.9 ms with w, 19.1 ms without (chain: 39.1 / 35.5); both forms move
// their bytes at the same 4.3 TB/s, i.e. the dw stores in the A layout
// (lanes 256 B apart, 32 B per pair of lanes) cost what their bytes cost
// and no more, which is why they were not staged through LDS (8 KB more
// per wave would also take the kernel from 3 blocks per CU to 2).
// Tried (stand-alone, 46M rows, with w / without):
//  * TAIL_CHUNK 2 / 4 / 8: 26.3 / 25.2 / 25.2 ms with w, 19.4 / 19.3 /
//    19.0 without; 146-148 VGPR in all three.  4 kept.
//  * nontemporal dz and dw stores (with or without nontemporal z loads):
//    29.7 ms with w, 19.0 without.  Rejected.
//  * a predicate on each dw store instead of one around the A phase: 16
//    basic blocks, 168 VGPR and 47 spilled (176-184 B scratch per lane).
//    Never run.
// ---------------------------------------------------------------------------
constexpr int TAIL_CHUNK = 4;    // row slices (of 8) per load batch

template <bool FULL>
__device__ __forceinline__ void mlp_tail_epilogue(
        const f32x16 (&acc)[4], const float* __restrict__ z,
        float* __restrict__ dz, int64_t base, int64_t E, int c, int h) {
    constexpr int G = 8;
#pragma unroll
    for (int rb = 0; rb < 16; rb += G) {
        float zv[G][4];
#pragma unroll
        for (int t = 0; t < G; ++t) {
            const int r = rb + t;
            const int rl = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int64_t row = base + rl;
            const int64_t lrow = (FULL || row < E) ? row : E - 1;
            const float* zp = z + lrow * 128 + c;
#pragma unroll
            for (int cb = 0; cb < 4; ++cb) zv[t][cb] = zp[32 * cb];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < G; ++t) {
            const int r = rb + t;
            const int rl = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int64_t row = base + rl;
            if (FULL || row < E) {
                float* dp = dz + row * 128 + c;
                float s4[4];
                sigf_n(zv[t], s4);
#pragma unroll
                for (int cb = 0; cb < 4; ++cb) {
                    const float x = zv[t][cb];
                    const float s = s4[cb];
                    dp[32 * cb] = acc[cb][r] * (s * (1.0f + x * (1.0f - s)));
                }
            }
            __builtin_amdgcn_sched_barrier(0);   // one row at a time
        }
    }
}

// Factored message weight (HAS_W == 2 in the three gated-MLP kernels below):
// w[r][col] = mask[r] * sum_k bexp[r][k] * W[col][k] with bexp [E,9], W [64,9]
// row-major and mask [E] (or none: 1), computed where it is used instead of
// read from a dense [E,64] array.  ONE fp32 order everywhere: b0 * W0, then an
// fma chain over k = 1..8 ascending, the mask multiplied last.  The forward
// tail, the one-kernel MLP and the reverse tail all call radial_w, so an outer
// forward, its recomputation and the reverse see the same w bit for bit.
// W rows live in LDS padded to 12 floats (three 16-byte reads per row).
constexpr int N_RBF = 9;
constexpr int RBF_PAD = 12;

__device__ __forceinline__ float radial_w(const float (&b)[N_RBF],
                                          const float (&wc)[N_RBF], float m) {
    float a = b[0] * wc[0];
#pragma unroll
    for (int k = 1; k < N_RBF; ++k) a = __builtin_fmaf(b[k], wc[k], a);
    return a * m;
}

// 9 floats of a padded LDS row (16-byte aligned); p3 receives float 9..11.
// The empty asm statements keep each 16-byte read whole: left alone, the
// compiler narrows the row to the 9 floats in use and reads them as one
// ds_read_b96 and three ds_read2_b32, each with an address register of its
// own (308 B of scratch per lane in the reverse kernel).
typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void radial_row(const float4* __restrict__ p,
                                           float (&v)[N_RBF], float4& p3) {
    const f32x4* q = (const f32x4*)p;
    f32x4 a = q[0], b = q[1], c = q[2];
    asm volatile("" : "+v"(a), "+v"(b), "+v"(c));
    p3 = make_float4(c.x, c.y, c.z, c.w);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
    v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    v[8] = p3.x;
}

// W [64,9] into the padded LDS image, by the whole block
__device__ __forceinline__ void radial_stage_W(float* __restrict__ wl9,
                                               const float* __restrict__ W) {
    for (int i = threadIdx.x; i < 64 * RBF_PAD; i += blockDim.x) {
        const int col = i / RBF_PAD, k = i - col * RBF_PAD;
        wl9[i] = k < N_RBF ? W[col * N_RBF + k] : 0.0f;
    }
}

// A phase of one tile for one lane: dc|dg of the 32 floats it owns of its
// row (offset off = row * 64 + 4h), dw stored from there.  go is read at
// goff: off itself, or idx[row] * 64 + 4h in the indexed form.
// HAS_W == 2: w of the lane's 32 columns comes from its bexp row bx (9
// registers) and mask m, and the W rows of those columns, the same for all
// lanes of a half-wave, from LDS (wl9 points at row 4h: broadcast reads);
// instead of the dw store, dbp[k] += dw[col] * W[col][k], columns ascending.
template <int HAS_W>
__device__ __forceinline__ void mlp_tail_a_phase(
        const float* __restrict__ go, const float* __restrict__ cp,
        const float* __restrict__ gp, const float* __restrict__ wp,
        float* __restrict__ dw, int64_t off, int64_t goff,
        float (&dcv)[32], float (&dgv)[32],
        const float4* __restrict__ wl9, const float (&bx)[N_RBF], float m,
        float (&dbp)[N_RBF]) {
    constexpr int CH = HAS_W == 2 ? 2 : TAIL_CHUNK;
#pragma unroll
    for (int i0 = 0; i0 < 8; i0 += CH) {
        float4 vgo[CH], vc[CH], vg[CH],
            vw[CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const int64_t o = off + 8 * (i0 + j);
            vgo[j] = *(const float4*)(go + goff + 8 * (i0 + j));
            vc[j] = *(const float4*)(cp + o);
            vg[j] = *(const float4*)(gp + o);
            if (HAS_W == 1) vw[j] = *(const float4*)(wp + o);
        }
        __builtin_amdgcn_sched_barrier(0);   // the batch in flight first
        // one range test per batch and the slice loop in two copies: a test
        // per slice splits the batch into blocks the compiler schedules one
        // by one, and the HAS_W forms then spill
        float cg[8 * CH];
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            cg[8 * j + 0] = vc[j].x; cg[8 * j + 1] = vc[j].y;
            cg[8 * j + 2] = vc[j].z; cg[8 * j + 3] = vc[j].w;
            cg[8 * j + 4] = vg[j].x; cg[8 * j + 5] = vg[j].y;
            cg[8 * j + 6] = vg[j].z; cg[8 * j + 7] = vg[j].w;
        }
        auto slices = [&](auto fast) {
#pragma unroll
        for (int j = 0; j < CH; ++j) {
            const float gov4[4] = {vgo[j].x, vgo[j].y, vgo[j].z, vgo[j].w};
            const float cv4[4] = {vc[j].x, vc[j].y, vc[j].z, vc[j].w};
            const float gv4[4] = {vg[j].x, vg[j].y, vg[j].z, vg[j].w};
            float wv4[4] = {1.0f, 1.0f, 1.0f, 1.0f};
            if (HAS_W == 1) {
                wv4[0] = vw[j].x; wv4[1] = vw[j].y;
                wv4[2] = vw[j].z; wv4[3] = vw[j].w;
            }
            float dwv[4], sc4[4], sg4[4];
            sigf_sel<decltype(fast)::value>(cv4, sc4);
            sigf_sel<decltype(fast)::value>(gv4, sg4);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                float wc[N_RBF];
                if (HAS_W == 2) {
                    float4 pad;                  // col = 8(i0+j) + 4h + t
                    radial_row(wl9 + (8 * (i0 + j) + t) * (RBF_PAD / 4), wc,
                               pad);
                    wv4[t] = radial_w(bx, wc, m);
                }
                const float gov = gov4[t], cv = cv4[t];
                const float sc = sc4[t], sg = sg4[t];
                const float silu_c = cv * sc;
                const float wv = wv4[t];
                dcv[4 * (i0 + j) + t] =
                    gov * wv * sg * (sc * (1.0f + cv * (1.0f - sc)));
                dgv[4 * (i0 + j) + t] =
                    gov * wv * silu_c * (sg * (1.0f - sg));
                dwv[t] = gov * silu_c * sg;
                if (HAS_W == 2) {
#pragma unroll
                    for (int k = 0; k < N_RBF; ++k)
                        dbp[k] = __builtin_fmaf(dwv[t], wc[k], dbp[k]);
                }
            }
            if (HAS_W == 1)
                *(float4*)(dw + off + 8 * (i0 + j)) =
                    make_float4(dwv[0], dwv[1], dwv[2], dwv[3]);
            __builtin_amdgcn_sched_barrier(0);   // one slice at a time
        }
        };
        if (__builtin_expect(act_wave_in_range(cg), 1))
            slices(std::true_type{});
        else
            slices(std::false_type{});
    }
}

// Waves per SIMD of the factored reverse tail.  Its A phase holds 31 more
// registers than the dense one (bexp row, mask, dbexp partials, a W row) next
// to the 64 of dc|dg: within the 168 registers of three waves per SIMD the
// compiler spills 47 of them (188 B of scratch per lane, with load batches of
// 1, 2 or 4 slices alike), at two it takes 218 and none with the load batches
// of 2 slices the A phase uses for this form (242 with batches of 4 and the
// plain sigmoid; batches of 4 with the range test spill 68 B).  2 is the build;
// -DDM_FW_BWD_WAVES=3 builds the spilling form for comparison
// (tests/perf_factored_w.py, profiles/factored_w_standalone.json).
#ifndef DM_FW_BWD_WAVES
#define DM_FW_BWD_WAVES 2
#endif

template <int HAS_W, bool IDX>
__global__ __launch_bounds__(256, HAS_W == 2 ? DM_FW_BWD_WAVES : 3)
void k_gated_mlp_tail_bwd(const float* __restrict__ go,   // [E,64]; IDX: [N,64]
                          const int32_t* __restrict__ idx, // [E], IDX only
                          const float* __restrict__ cp,   // [E,64]
                          const float* __restrict__ gp,   // [E,64]
                          const float* __restrict__ wp,   // [E,64], HAS_W;
                                                          // 2: bexp [E,9]
                          const float* __restrict__ z,    // [E,128]
                          const float* __restrict__ w2c,  // [64,64] in x out
                          const float* __restrict__ w2g,
                          float* __restrict__ dz,         // [E,128]
                          float* __restrict__ dw,         // [E,64], HAS_W 1
                          int64_t E,
                          // HAS_W == 2 only
                          const float* __restrict__ fwW,  // [64,9]
                          const float* __restrict__ fwmask,  // [E] or null
                          const float* dbexp_in,          // [E,9] or null
                          float* dbexp) {                 // [E,9], may be
                                                          // dbexp_in
    __shared__ float4 wlds[64 * 32];
    __shared__ float4 wl9[HAS_W == 2 ? 64 * RBF_PAD / 4 : 1];
    if (HAS_W == 2) radial_stage_W((float*)wl9, fwW);
    // i = (col, k) with k fastest: coalesced reads of the row-major blocks
    for (int i = threadIdx.x; i < 64 * 32; i += blockDim.x) {
        const int k = i & 63, col = i >> 6;
        wlds[k * 32 + col] = make_float4(w2c[col * 64 + k],
                                         w2c[(32 + col) * 64 + k],
                                         w2g[col * 64 + k],
                                         w2g[(32 + col) * 64 + k]);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int waves_per_block = blockDim.x >> 6;
    const int64_t ntiles = (E + 31) >> 5;
    const int64_t stride = (int64_t)gridDim.x * waves_per_block;
    for (int64_t tile = blockIdx.x * (int64_t)waves_per_block + wave;
         tile < ntiles; tile += stride) {
        const int64_t base = tile << 5;
        // opaque copy per tile, as in k_edge_mlp_64x128: keeps the
        // per-register row offsets from being hoisted and spilled
        int lane_t = lane;
        asm volatile("" : "+v"(lane_t));
        const int c = lane_t & 31, h = lane_t >> 5;
        const float4* bl = wlds + (4 * h) * 32 + c;
        const int64_t r = base + c;
        const bool live = r < E;
        const int64_t off = r * 64 + 4 * h;
        float dcv[32], dgv[32];
#pragma unroll
        for (int q = 0; q < 32; ++q) dcv[q] = dgv[q] = 0.0f;
        // ONE predicate around the whole A phase: lanes of rows >= E load
        // and store nothing and feed zeros to the MFMAs.  (A predicate on
        // each dw store instead splits the phase into 16 basic blocks and
        // the register allocator then spills 47 VGPRs.)
        float bx[N_RBF], dbp[N_RBF], msk = 1.0f;
#pragma unroll
        for (int k = 0; k < N_RBF; ++k) bx[k] = dbp[k] = 0.0f;
        if (live) {
            // IDX: row r's go is row idx[r] of a table, one index per lane
            const int64_t goff = IDX ? (int64_t)idx[r] * 64 + 4 * h : off;
            if (HAS_W == 2) {
#pragma unroll
                for (int k = 0; k < N_RBF; ++k) bx[k] = wp[r * N_RBF + k];
                if (fwmask) msk = fwmask[r];
            }
            mlp_tail_a_phase<HAS_W>(go, cp, gp, wp, dw, off, goff, dcv, dgv,
                                    wl9 + (4 * h) * (RBF_PAD / 4), bx, msk,
                                    dbp);
        }
        if (HAS_W == 2) {
            // dbexp[r][k] = mask[r] * (h=0 partial + h=1 partial) + dbexp_in:
            // the lane's columns ascending (above), then the two half-waves
            // (the sum commutes, both halves hold the same bits), the mask,
            // then dbexp_in, each rounded on its own.  Lane h = 0 of the row
            // reads and writes its 9 floats, so dbexp may be dbexp_in.
#pragma clang fp contract(off)
            float ds[N_RBF];
#pragma unroll
            for (int k = 0; k < N_RBF; ++k)
                ds[k] = (dbp[k] + __shfl_xor(dbp[k], 32, 64)) * msk;
            if (live && h == 0) {
                if (dbexp_in) {
#pragma unroll
                    for (int k = 0; k < N_RBF; ++k)
                        ds[k] += dbexp_in[r * N_RBF + k];
                }
#pragma unroll
                for (int k = 0; k < N_RBF; ++k) dbexp[r * N_RBF + k] = ds[k];
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        f32x16 acc[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[cb][q] = 0.0f;
        __builtin_amdgcn_s_setprio(3);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float4 b = bl[(8 * i + t) * 32];   // k = 8i + 4h + t
                const float ac = dcv[4 * i + t], ag = dgv[4 * i + t];
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, b.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(ac, b.y, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(ag, b.z, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(ag, b.w, acc[3], 0, 0, 0);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        if (base + 32 <= E)
            mlp_tail_epilogue<true>(acc, z, dz, base, E, c, h);
        else
            mlp_tail_epilogue<false>(acc, z, dz, base, E, c, h);
    }
}

// ---------------------------------------------------------------------------
// Reverse of the first layer's per-edge GEMM, with the gradient sum folded
// in (Din = 128 -> Dout = 64):
//   out[e,:] = (gbase[e,:] +) dz[e,:] @ WT^T
// WT [64,128] is the fusedT pack k_edge_mlp_64x128 takes, so this is de of
// z = erow @ WT + ...; gbase is the other gradient of the same e (e feeds an
// MLP as erow and flows on as base / to the next block), which autograd
// would add in a pass of its own.  It replaces a rocBLAS GEMM (or addmm) and
// that add.
//
// Skeleton of k_edge_mlp_64x128: one wave owns 32 rows x 64 columns = 2
// accumulators (v_mfma_f32_32x32x2_f32, starting at 0), 4 waves per block,
// grid capped by edge_mlp_blocks so WT is staged once per block.
//  * B operand: LDS float2 [k][col] = (WT[col][k], WT[32+col][k]), 32 KB;
//    one ds_read_b64 per k-step feeds the two MFMAs of that step.
//  * A operand without LDS: dz is row-major, so lane (r = lane&31,
//    h = lane>>5) reads its own row as 16 float4s at floats [8i+4h, 8i+4h+4);
//    MFMA step 4i+t contracts k = 8i+4h+t.  128 MFMAs per tile.
//  * Epilogue in the accumulator layout (col = lane&31, row = (reg&3) +
//    8*(reg>>2) + 4*(lane>>5)): gbase is loaded 8 rows at a time and added
//    with one rounding per element, gbase + acc.  A lane reads exactly the
//    elements it then writes, and tiles own disjoint rows, so out may be
//    gbase itself (neither pointer is __restrict__).
//  * Tails: loads of rows >= E are clamped to row E-1, stores predicated;
//    all row offsets are 64-bit.
// Algorithmic bytes at 46M rows / 6.29 TB/s: 47.1 GB = 7.5 ms with gbase,
// 35.3 GB = 5.6 ms without.
// Resources (hipcc -O3, gfx950, kernel-resource-usage remarks):
//   <true>  (gbase): 112 VGPR, 0 AGPR, 60 SGPR, 32 KB LDS, 4 waves/SIMD, no
//                    scratch
//   <false>:         112 VGPR, 0 AGPR, 26 SGPR, 32 KB LDS, 4 waves/SIMD, no
//                    scratch
// (the grid cap of 3 blocks per CU holds either way).
// Measured at si1m (rocprofv3 kernel trace, 3 steps): at E = 46M rows with
// gbase 21 launches, 8.58 ms (8.39-8.69), without 3 launches of 6.9 ms; at
// L = 12M rows without gbase 1.9 ms (15 launches).  The parent's trace of the
// same run: 8.1-8.3 ms for the GEMM alone plus 8 add launches of 0.7-0.9 ms
// per sum.  Stand-alone on random inputs, 46M rows, median of 5: 9.47 ms with
// gbase (in place 9.43) against 16.2 for torch.addmm and 15.0 for mm + add;
// 7.39 against 8.73 for mm.  Indexed reverse tail in the same runs: 20.0 ms
// in the trace against 22.4 + 3.1 (k_gather_rows_v4), 22.2 against 28.0
// stand-alone.
// ---------------------------------------------------------------------------
template <bool HAS_BASE, bool FULL>
__device__ __forceinline__ void edge_mlp_bwd_epilogue(
        const f32x16 (&acc)[2], const float* gbase, float* out, int64_t base,
        int64_t E, int c, int h) {
    constexpr int G = 8;
#pragma unroll
    for (int rb = 0; rb < 16; rb += G) {
        float gv[G][2];
        if (HAS_BASE) {
#pragma unroll
            for (int t = 0; t < G; ++t) {
                const int r = rb + t;
                const int rl = (r & 3) + 8 * (r >> 2) + 4 * h;
                const int64_t row = base + rl;
                const int64_t lrow = (FULL || row < E) ? row : E - 1;
                const float* gp = gbase + lrow * 64 + c;
                gv[t][0] = gp[0];
                gv[t][1] = gp[32];
            }
            __builtin_amdgcn_sched_barrier(0);   // the batch in flight first
        }
#pragma unroll
        for (int t = 0; t < G; ++t) {
            const int r = rb + t;
            const int rl = (r & 3) + 8 * (r >> 2) + 4 * h;
            const int64_t row = base + rl;
            if (FULL || row < E) {
                float* op = out + row * 64 + c;
                op[0] = HAS_BASE ? gv[t][0] + acc[0][r] : acc[0][r];
                op[32] = HAS_BASE ? gv[t][1] + acc[1][r] : acc[1][r];
            }
        }
    }
}

template <bool HAS_BASE>
__global__ __launch_bounds__(256, 3)
void k_edge_mlp_bwd(const float* __restrict__ dz,    // [E,128]
                    const float* __restrict__ WT,    // [64,128] row-major
                    const float* gbase,              // [E,64], HAS_BASE
                    float* out,                      // [E,64], may be gbase
                    int64_t E) {
    __shared__ float2 wlds[128 * 32];
    // i = (col, k) with k fastest: coalesced reads of the row-major WT
    for (int i = threadIdx.x; i < 128 * 32; i += blockDim.x) {
        const int k = i & 127, col = i >> 7;
        wlds[k * 32 + col] = make_float2(WT[col * 128 + k],
                                         WT[(32 + col) * 128 + k]);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int waves_per_block = blockDim.x >> 6;
    const int64_t ntiles = (E + 31) >> 5;
    const int64_t stride = (int64_t)gridDim.x * waves_per_block;
    for (int64_t tile = blockIdx.x * (int64_t)waves_per_block + wave;
         tile < ntiles; tile += stride) {
        const int64_t base = tile << 5;
        // opaque copy per tile, as in k_edge_mlp_64x128: keeps the
        // per-register row offsets from being hoisted and spilled
        int lane_t = lane;
        asm volatile("" : "+v"(lane_t));
        const int c = lane_t & 31, h = lane_t >> 5;
        const float2* bl = wlds + (4 * h) * 32 + c;
        const int64_t r = base + c;
        const int64_t lrow = r < E ? r : E - 1;   // clamp, never read past E
        const float4* ap = (const float4*)(dz + lrow * 128) + h;
        float4 a[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) a[i] = ap[2 * i];
        __builtin_amdgcn_sched_barrier(0);   // all loads in flight first
        f32x16 acc[2];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[cb][q] = 0.0f;
        __builtin_amdgcn_s_setprio(3);
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const float av[4] = {a[i].x, a[i].y, a[i].z, a[i].w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float2 b = bl[(8 * i + t) * 32];   // k = 8i + 4h + t
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], b.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[t], b.y, acc[1], 0, 0, 0);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        if (base + 32 <= E)
            edge_mlp_bwd_epilogue<HAS_BASE, true>(acc, gbase, out, base, E, c, h);
        else
            edge_mlp_bwd_epilogue<HAS_BASE, false>(acc, gbase, out, base, E, c, h);
    }
}

// ---------------------------------------------------------------------------
// Fused forward tail of one gated MLP (d = 64): second layer + combine,
//   c = h[:, :64] @ w2c + b2c      g = h[:, 64:] @ w2g + b2g
//   out = base + silu(c) * sigmoid(g) * w
// in one pass over h.  It replaces the rocBLAS baddbmm + k_gated_combine_fwd:
// c|g ([2,E,64]) are written only when a reverse pass will read them (KEEP)
// and are never read back.  The scalar expression is k_gated_combine_fwd's
// (exact expf and division), and does not depend on KEEP: out is the same
// bit for bit with and without the c|g stores.
//
// Skeleton of k_edge_mlp_64x128 / k_gated_mlp_tail_bwd: one wave owns 32
// rows and 4 accumulators (v_mfma_f32_32x32x2_f32, starting at 0), 4 waves
// per block, grid capped by edge_mlp_blocks.
//  * Accumulators 0,1 are c columns col, 32+col; 2,3 are g columns col,
//    32+col.
//  * B operand: LDS float4 [k][col] = (w2c[k][col], w2c[k][32+col],
//    w2g[k][col], w2g[k][32+col]), 32 KB; w2 is [in, out] row-major, so the
//    staging is a straight regrouping and one ds_read_b128 per k-step feeds
//    the four MFMAs of that step.
//  * A operand without LDS and without a transposition: h is row-major in
//    memory, and lane (r = lane&31, hh = lane>>5) reads its own row at
//    floats [8i+4hh, 8i+4hh+4) of the low and of the high half, 16 float4s
//    all issued before the first MFMA.  Step 4i+t contracts k = 8i+4hh+t;
//    accumulators 0,1 take the low-half value, 2,3 the high-half value.
//  * Epilogue in the accumulator layout (col = lane&31, row = (reg&3) +
//    8*(reg>>2) + 4*(lane>>5)): c and g of one (row, col) sit in the same
//    lane, so the combine is lane-local.  b2 is added here and not folded
//    into the accumulator init, for the reason given at k_edge_mlp_64x128.
//    w and base are loaded 8 rows at a time, all loads of a batch in flight
//    before any is used.
//  * Tails: loads of rows >= E are clamped to row E-1, stores predicated.
//    All row offsets are 64-bit.
// Resources (hipcc -O3, gfx950, kernel-resource-usage remarks), all eight
// <KEEP, HAS_W, HAS_BASE> variants: 152 VGPR, 0 AGPR, 31-68 SGPR, 32 KB LDS,
// 3 waves/SIMD, no scratch.
// The four factored-w variants <KEEP, 2, HAS_BASE>
// (dm_gated_mlp_tail_fwd_fw_f32): 162 VGPR, 0 AGPR, 50-86 SGPR, 41 KB LDS
// (W image 3 KB, bexp regions 6 KB), 3 waves/SIMD, no scratch.
// Measured at si1m (rocprofv3 kernel trace, 3 steps; every launch there is a
// KEEP one): at E = 46M rows with w and base, 24 launches, 13.8 ms average
// (13.65-14.43); with w alone 12.85 ms (12.68-12.98); at L = 12M rows 3.8
// ms.  The chain it replaces took, in the parent's trace of the same
// session, 13.9 (rocBLAS MT64x256x16) + 11.8 / 8.85 (k_gated_combine_fwd
// with w and base / with one of them) ms at 46M rows and 4.15 + 2.55 at 12M.
// Algorithmic bytes at 46M rows, KEEP with w and base: 82.4 GB = 13.1 ms at
// 6.29 TB/s.
// Stand-alone on random inputs, 46M rows (median of 5; chain 18.5 + 12.7 ms
// there):    w+base   w      base   neither
//   KEEP     14.53    13.44  13.46  -
//   no KEEP  12.49    11.86  11.77  10.80   (10.8 ms: 35 GB at 3.3 TB/s, the
//                                            MFMA-issue bound of this shape)
// Tried (same stand-alone run, KEEP w+base / no-KEEP w+base / no-KEEP
// neither):
//  * epilogue batches of 4 rows instead of 8: 14.67 / 12.66 / 10.87 ms, 152
//    VGPR.  8 kept.
//  * A loads in two chunks of 4 slices with the MFMAs of a chunk in between
//    (as TAIL_CHUNK does in the reverse kernel): 122-139 VGPR, 4 waves/SIMD
//    in six variants, 14.63 / 12.54 / 11.06 ms.  No gain; all 16 loads up
//    front kept.
//  * leaving the epilogue's r*w + base to the compiler (one fma): out then
//    differs from k_gated_combine_fwd's in the last bit.  The stand-alone
//    numbers above were taken with that version, the si1m ones with this.
// ---------------------------------------------------------------------------
// The epilogue in two parts, so that k_gated_mlp_64 can issue the loads of
// all 16 rows (G = 16) ahead of its last MFMA run: the w / base loads of rows
// rb .. rb+G-1 of the accumulator layout, and the c|g stores and the combine
// of those rows.  OUT = false (k_gated_mlp_64's out-less keep form): c|g are
// stored and the combine is skipped; w, bs and out are not touched.
//
// HAS_W == 2 (factored w, see radial_w): nothing of w is loaded per row.  A
// wave stages its tile's bexp block, 32 x 9 contiguous floats, and the 32 mask
// values in an LDS region of its own, rows padded to 12 floats with the mask
// in float 9 (radial_tile_load issues the 6 loads per lane, radial_tile_store
// writes them once they have landed; rows >= E get zeros, and are never
// stored).  The epilogue reads a row as three 16-byte broadcast reads per
// half-wave and combines it with the lane's two W rows (18 registers, read
// from the padded LDS image of W once per tile).  LDS operations of one wave
// execute in order, so the region needs no barrier between a tile's reads and
// the next tile's writes.
constexpr int RBF_TILE = 32 * RBF_PAD;      // floats of one wave's region

__device__ __forceinline__ void radial_tile_load(
        float (&sv)[6], const float* __restrict__ bexp,
        const float* __restrict__ mask, int64_t base, int64_t E, int lane) {
    const int64_t o = base * N_RBF, lim = E * N_RBF;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int i = lane + 64 * j;
        sv[j] = (i < 32 * N_RBF && o + i < lim) ? bexp[o + i] : 0.0f;
    }
    const int64_t row = base + (lane & 31);
    sv[5] = row < E ? (mask ? mask[row] : 1.0f) : 0.0f;
}

__device__ __forceinline__ void radial_tile_store(
        float* __restrict__ st, const float (&sv)[6], int lane) {
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const int i = lane + 64 * j;
        const int row = i / N_RBF;
        if (i < 32 * N_RBF) st[row * RBF_PAD + (i - row * N_RBF)] = sv[j];
    }
    if (lane < 32) st[lane * RBF_PAD + N_RBF] = sv[5];
    __builtin_amdgcn_wave_barrier();   // no read of the region moves above
}

// the lane's two W rows (columns c and 32 + c) from the padded LDS image
__device__ __forceinline__ void radial_lane_W(
        float (&wc)[2][N_RBF], const float4* __restrict__ wl9, int c) {
    float4 pad;
    radial_row(wl9 + c * (RBF_PAD / 4), wc[0], pad);
    radial_row(wl9 + (32 + c) * (RBF_PAD / 4), wc[1], pad);
}

template <int HAS_W, bool HAS_BASE, bool FULL, int G>
__device__ __forceinline__ void mlp_tail_fwd_loads(
        float (&wv)[G][2], float (&bv)[G][2], int rb,
        const float* __restrict__ w, const float* __restrict__ bs,
        int64_t base, int64_t E, int c, int h) {
#pragma unroll
    for (int t = 0; t < G; ++t) {
        const int r = rb + t;
        const int rl = (r & 3) + 8 * (r >> 2) + 4 * h;
        const int64_t row = base + rl;
        const int64_t lrow = (FULL || row < E) ? row : E - 1;
        if (HAS_W == 1) {
            wv[t][0] = w[lrow * 64 + c];
            wv[t][1] = w[lrow * 64 + 32 + c];
        }
        if (HAS_BASE) {
            bv[t][0] = bs[lrow * 64 + c];
            bv[t][1] = bs[lrow * 64 + 32 + c];
        }
    }
}

// st4 (HAS_W == 2): the wave's staged bexp region at row 4h; wc: the lane's
// two W rows.
template <bool KEEP, int HAS_W, bool HAS_BASE, bool FULL, bool OUT, int G>
__device__ __forceinline__ void mlp_tail_fwd_rows(
        const f32x16 (&acc)[4], const float4 bcol,
        const float (&wv)[G][2], const float (&bv)[G][2], int rb,
        float* __restrict__ cout, float* __restrict__ gout,
        float* __restrict__ out, int64_t base, int64_t E, int c, int h,
        const float4* __restrict__ st4, const float (&wc)[2][N_RBF]) {
    static_assert(OUT || (KEEP && !HAS_W && !HAS_BASE),
                  "the out-less form stores c|g and reads neither w nor base");
#pragma unroll
    for (int t = 0; t < G; ++t) {
        const int r = rb + t;
        const int rl = (r & 3) + 8 * (r >> 2) + 4 * h;
        const int64_t row = base + rl;
        const float cv[2] = {acc[0][r] + bcol.x, acc[1][r] + bcol.y};
        const float gv[2] = {acc[2][r] + bcol.z, acc[3][r] + bcol.w};
        float wq[2] = {1.0f, 1.0f};
        if (HAS_W == 1) {
            wq[0] = wv[t][0]; wq[1] = wv[t][1];
        }
        if (HAS_W == 2) {
            float bx[N_RBF];
            float4 p3;                           // p3.y: the row's mask
            radial_row(st4 + ((r & 3) + 8 * (r >> 2)) * (RBF_PAD / 4), bx, p3);
            wq[0] = radial_w(bx, wc[0], p3.y);
            wq[1] = radial_w(bx, wc[1], p3.y);
        }
        if (FULL || row < E) {
            const int64_t o = row * 64 + c;
            if (KEEP) {
                cout[o] = cv[0]; cout[o + 32] = cv[1];
                gout[o] = gv[0]; gout[o + 32] = gv[1];
            }
            const float cg4[4] = {cv[0], cv[1], gv[0], gv[1]};
            float s4[4];
            if (OUT) sigf_n(cg4, s4);
#pragma unroll
            for (int q = 0; OUT && q < 2; ++q) {
                // k_gated_combine_fwd rounds each product and the
                // +base separately (its w and base branches keep them
                // from being contracted to an fma): the same here, so
                // out equals that kernel's over the same c|g bit for
                // bit
#pragma clang fp contract(off)
                float x = cv[q] * s4[q] * s4[2 + q];
                if (HAS_W) x *= wq[q];
                if (HAS_BASE) x += bv[t][q];
                out[o + 32 * q] = x;
            }
        }
        __builtin_amdgcn_sched_barrier(0);   // one row at a time
    }
}

template <bool KEEP, int HAS_W, bool HAS_BASE, bool FULL>
__device__ __forceinline__ void mlp_tail_fwd_epilogue(
        const f32x16 (&acc)[4], const float4 bcol,
        const float* __restrict__ w, const float* __restrict__ bs,
        float* __restrict__ cout, float* __restrict__ gout,
        float* __restrict__ out, int64_t base, int64_t E, int c, int h,
        const float4* __restrict__ wl9, const float4* __restrict__ st4) {
    constexpr int G = 8;
    float wc[2][N_RBF];
    if (HAS_W == 2) radial_lane_W(wc, wl9, c);
#pragma unroll
    for (int rb = 0; rb < 16; rb += G) {
        float wv[G][2], bv[G][2];
        mlp_tail_fwd_loads<HAS_W, HAS_BASE, FULL, G>(wv, bv, rb, w, bs, base,
                                                     E, c, h);
        __builtin_amdgcn_sched_barrier(0);
        mlp_tail_fwd_rows<KEEP, HAS_W, HAS_BASE, FULL, true, G>(
            acc, bcol, wv, bv, rb, cout, gout, out, base, E, c, h, st4, wc);
    }
}

template <bool KEEP, int HAS_W, bool HAS_BASE>
__global__ __launch_bounds__(256, 3)
void k_gated_mlp_tail_fwd(const float* __restrict__ hp,    // [E,128]
                          const float* __restrict__ w2c,   // [64,64] in x out
                          const float* __restrict__ w2g,
                          const float* __restrict__ b2c,   // [64]
                          const float* __restrict__ b2g,
                          const float* __restrict__ w,     // [E,64], HAS_W;
                                                           // 2: bexp [E,9]
                          const float* __restrict__ bs,    // [E,64], HAS_BASE
                          float* __restrict__ cout,        // [E,64], KEEP
                          float* __restrict__ gout,        // [E,64], KEEP
                          float* __restrict__ out,         // [E,64]
                          int64_t E,
                          // HAS_W == 2 only
                          const float* __restrict__ fwW,   // [64,9]
                          const float* __restrict__ fwmask) {  // [E] or null
    __shared__ float4 wlds[64 * 32];
    __shared__ float4 wl9[HAS_W == 2 ? 64 * RBF_PAD / 4 : 1];
    __shared__ float4 bst[HAS_W == 2 ? (BLOCK / 64) * RBF_TILE / 4 : 1];
    if (HAS_W == 2) radial_stage_W((float*)wl9, fwW);
    for (int i = threadIdx.x; i < 64 * 32; i += blockDim.x) {
        const int k = i >> 5, col = i & 31;
        wlds[i] = make_float4(w2c[k * 64 + col], w2c[k * 64 + 32 + col],
                              w2g[k * 64 + col], w2g[k * 64 + 32 + col]);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int c0 = lane & 31;
    const int wave = threadIdx.x >> 6;
    const int waves_per_block = blockDim.x >> 6;
    const float4 bcol = make_float4(b2c[c0], b2c[32 + c0], b2g[c0],
                                    b2g[32 + c0]);
    const int64_t ntiles = (E + 31) >> 5;
    const int64_t stride = (int64_t)gridDim.x * waves_per_block;
    for (int64_t tile = blockIdx.x * (int64_t)waves_per_block + wave;
         tile < ntiles; tile += stride) {
        const int64_t base = tile << 5;
        // opaque copy per tile, as in k_edge_mlp_64x128: keeps the
        // per-register row offsets from being hoisted and spilled
        int lane_t = lane;
        asm volatile("" : "+v"(lane_t));
        const int c = lane_t & 31, h = lane_t >> 5;
        const float4* bl = wlds + (4 * h) * 32 + c;
        const int64_t r = base + c;
        const int64_t lrow = r < E ? r : E - 1;   // clamp, never read past E
        const float4* ap = (const float4*)(hp + lrow * 128) + h;
        float sv[6];
        if (HAS_W == 2) radial_tile_load(sv, w, fwmask, base, E, lane_t);
        float4 alo[8], ahi[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            alo[i] = ap[2 * i];
            ahi[i] = ap[16 + 2 * i];
        }
        __builtin_amdgcn_sched_barrier(0);   // all loads in flight first
        float* st = (float*)bst + wave * RBF_TILE;
        if (HAS_W == 2) radial_tile_store(st, sv, lane_t);
        const float4* st4 = (const float4*)st + (4 * h) * (RBF_PAD / 4);
        f32x16 acc[4];
#pragma unroll
        for (int cb = 0; cb < 4; ++cb)
#pragma unroll
            for (int q = 0; q < 16; ++q) acc[cb][q] = 0.0f;
        __builtin_amdgcn_s_setprio(3);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float lo[4] = {alo[i].x, alo[i].y, alo[i].z, alo[i].w};
            const float hi[4] = {ahi[i].x, ahi[i].y, ahi[i].z, ahi[i].w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float4 b = bl[(8 * i + t) * 32];   // k = 8i + 4h + t
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(lo[t], b.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(lo[t], b.y, acc[1], 0, 0, 0);
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(hi[t], b.z, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(hi[t], b.w, acc[3], 0, 0, 0);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        if (base + 32 <= E)
            mlp_tail_fwd_epilogue<KEEP, HAS_W, HAS_BASE, true>(
                acc, bcol, w, bs, cout, gout, out, base, E, c, h, wl9, st4);
        else
            mlp_tail_fwd_epilogue<KEEP, HAS_W, HAS_BASE, false>(
                acc, bcol, w, bs, cout, gout, out, base, E, c, h, wl9, st4);
    }
}

// ---------------------------------------------------------------------------
// One whole gated MLP (Din = 64, d = 64) in one kernel: k_edge_mlp_64x128
// followed by k_gated_mlp_tail_fwd without the h [E,128] array between them.
//   z   = erow @ WT + bias + g0[i0] + g1[i1] (+ g2[i2])        [E,128]
//   c|g = silu(z) halves @ w2c|w2g + b2c|b2g                   [E,64] each
//   out = base + silu(c) * sigmoid(g) * w
// Forms: no-keep (out only), keep (z, c, g and out), keep without out (z, c,
// g; w and base are not read: the node MLP of a recomputation).
//
// No transposition is needed between the layers: the first product is
// computed transposed, z^T = WT^T . x^T, by swapping the first two operands
// of k_edge_mlp_64x128's MFMAs (same LDS image, same per-lane e-row
// registers).  Register r = 4q+t of column block cb in lane (c, h) then holds
//   z[base+c][32cb + 8q + 4h + t],
// which is float t of the float4 slice s = 4(cb&1)+q at floats [8s+4h, +4) of
// the low (cb 0,1) or high (cb 2,3) half of the lane's OWN row: exactly what
// k_gated_mlp_tail_fwd loads as alo[s] / ahi[s] and contracts at step 4s+t.
// After bias, gathers and SiLU the registers are the second layer's A
// operand as they stand.  Both fma chains keep their k order and products
// commute, so z, c, g and out equal the two-kernel path's bit for bit; the
// epilogue adds are in edge_mlp_epilogue's order (acc + bias, += g0 + g1,
// += g2; bias not folded into the accumulator init, see k_edge_mlp_64x128).
//
// Per tile of 32 rows per wave, four MFMA runs of 64: the first layer's core
// half (z columns 0-63); its gate half, with the core half's epilogue (bias,
// gathers, SiLU, z stores) in the MFMA gaps; the second layer's c, with the
// gate half's epilogue in the gaps; the second layer's g; then the parents'
// tail epilogue (mlp_tail_fwd_rows).  Each accumulator's own chain is in the
// parents' (i, t) order.  Every lane needs only its own row's indices (no
// ds_bpermute); gathers and z stores are the lane's own float4 slices, 16 B
// per lane with 32 distinct rows per instruction (the pattern of the
// parents' A-operand loads).  Loads are issued a phase or more ahead: a
// half's gathers before the MFMA run that precedes their use, the next
// tile's e row and indices as soon as a[] is dead, w and base of all 16
// accumulator rows before the last MFMA run.
// Tails: loads of rows >= E are clamped to row E-1, stores predicated; all
// row offsets are 64-bit.
// LDS: both weight images, 64 KB + 512 B of bias per block: two blocks of
// 256 threads per CU, 2 waves/SIMD, grid capped at 512 blocks.
// Resources (hipcc -O3, gfx950, kernel-resource-usage remarks), all 18
// variants: NGATHER 2 220-250 VGPR, NGATHER 3 249-255; 0 AGPR, 44-82 SGPR,
// 66048 B LDS, 2 waves/SIMD, no scratch.  The three-gather variants sit 1-7
// registers under the 256 of two waves per SIMD: check these remarks after
// any change here or in the compiler, a spill would not show otherwise.
// The four factored-w variants <2, KEEP, true, 2, HAS_BASE>
// (dm_gated_mlp3_fw_f32): 243-256 VGPR (256: no-keep with base), 0 AGPR,
// 60-92 SGPR, 75264 B LDS, 2 waves/SIMD, no scratch.
// 384-thread blocks (3 waves/SIMD) would need <= 168 VGPR, i.e. none of the
// look-ahead; not built.
// Stand-alone at 46M rows (tests/perf_gated_mlp_fused.py, median of 5, ms;
// the pair = k_edge_mlp_64x128 + k_gated_mlp_tail_fwd in the same run):
//                     NGATHER 2        NGATHER 3
//   no-keep w+base    21.5 / 24.7      22.8 / 25.9
//   no-keep w         20.4 / 24.0      22.0 / 25.4
//   keep w+base       26.1 / 28.7      28.9 / 31.0
//   keep w            25.4 / 27.8      28.9 / 29.9
//   keep, no out      20.8 / 27.8      24.3 / 29.9
// against 9.6 ms of MFMA time at the 157 TF peak and 7.5 / 15.0 / 9.4 ms of
// bytes at 6.29 TB/s (no-keep w+base / keep w+base / keep no out).  Every
// form beats its pair by more than both spreads, by 2-3.5 ms where 9-10 had
// been estimated (7 ms without out, which is work removed): the time is
// close to MFMA time plus byte time, as in the parents; the two do not
// overlap here either.
// Measured at si1m (rocprofv3 kernel trace, 3 steps, E = 46M rows): keep
// w+base 12 launches of 24.9 ms (24.9-25.0) against 14 + 13.8 for the pair
// in the parent's trace of the same session; keep without out 12 launches of
// 19.1 ms (19.1-19.4) against 14 + 12.9.
// Tried, same stand-alone run, no-keep w+base / keep w+base / keep no out:
//  * the plain order (epilogue of a half after its MFMA run, nothing in the
//    gaps), loads issued where needed: 21.8 / 27.1 / 21.1
//  * that with the look-ahead loads: 21.3 / 27.3 / 21.3
//  * no s_setprio: 21.8 / 27.8 / 22.0; s_setprio raised in the epilogues
//    instead of the MFMA runs: 21.9 / 27.9 / 21.0
//  * no scheduling barrier between the SiLU slices: 21.7 / 27.0 / 20.7
//  * this version (epilogues in the MFMA gaps): 21.5 / 26.1 / 20.8; the
//    three-gather keep-no-out form lost 1 ms by it (23.2 -> 24.3)
// ---------------------------------------------------------------------------
constexpr int GATED_MLP_MAX_BLOCKS = 512;   // 256 CUs x 2 resident blocks

inline int gated_mlp_blocks(int64_t rows) {
    const int64_t tiles = (rows + 31) / 32;         // one 32-row tile per wave
    const int64_t b = (tiles + BLOCK / 64 - 1) / (BLOCK / 64);
    return (int)(b < 1 ? 1 : (b > GATED_MLP_MAX_BLOCKS ? GATED_MLP_MAX_BLOCKS : b));
}

// grid of the factored reverse tail: the cap of its resident blocks per CU
inline int mlp_tail_bwd_fw_blocks(int64_t rows) {
    return DM_FW_BWD_WAVES == 2 ? gated_mlp_blocks(rows)
                                : edge_mlp_blocks(rows);
}

// The lane's own slices of one half (HALF 0: z columns 0-63, 1: 64-127) of
// its gathered rows; p* point at float 4h of the rows.
template <int NGATHER, int HALF>
__device__ __forceinline__ void gated_mlp_gather(
        float4 (&gv)[NGATHER][8], const float4* __restrict__ p0,
        const float4* __restrict__ p1, const float4* __restrict__ p2) {
#pragma unroll
    for (int s = 0; s < 8; ++s) {
        gv[0][s] = p0[16 * HALF + 2 * s];
        gv[1][s] = p1[16 * HALF + 2 * s];
        if (NGATHER == 3) gv[NGATHER - 1][s] = p2[16 * HALF + 2 * s];
    }
}

// First-layer epilogue of slice s of one half, in the transposed accumulator
// layout: z = acc + bias + gathered slices, hs[s] = silu(z); z stored with
// KEEP.
template <int NGATHER, bool KEEP, int HALF>
__device__ __forceinline__ void gated_mlp_slice_epilogue(
        const f32x16 (&za)[2], const float4 (&gv)[NGATHER][8],
        const float4* __restrict__ bias4,   // LDS, at float4 h
        float4* __restrict__ zrow,          // z_out row, at float4 h
        bool store, float4 (&hs)[8], int s) {
    const float4 b = bias4[16 * HALF + 2 * s];
    const int cb = s >> 2, r0 = 4 * (s & 3);
    float z[4] = {za[cb][r0 + 0] + b.x, za[cb][r0 + 1] + b.y,
                  za[cb][r0 + 2] + b.z, za[cb][r0 + 3] + b.w};
    const float v0[4] = {gv[0][s].x, gv[0][s].y, gv[0][s].z, gv[0][s].w};
    const float v1[4] = {gv[1][s].x, gv[1][s].y, gv[1][s].z, gv[1][s].w};
#pragma unroll
    for (int t = 0; t < 4; ++t) z[t] += v0[t] + v1[t];
    if (NGATHER == 3) {
        const float4 v2 = gv[NGATHER - 1][s];
        z[0] += v2.x; z[1] += v2.y; z[2] += v2.z; z[3] += v2.w;
    }
    if (KEEP && store)
        zrow[16 * HALF + 2 * s] = make_float4(z[0], z[1], z[2], z[3]);
    hs[s] = siluf4(make_float4(z[0], z[1], z[2], z[3]));
}

// One slice's epilogue shares a scheduling region with 8 MFMAs of the run
// beside it: a v_mfma_f32_32x32x2_f32 holds the matrix pipe for 64 cycles
// and the wave's own vector instructions issue in that gap, about 14 of
// them; two waves per SIMD alone did not overlap the two (header comment).
__device__ __forceinline__ void gated_mlp_interleave() {
#pragma unroll
    for (int m = 0; m < 8; ++m) {
        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // 1 MFMA
        __builtin_amdgcn_sched_group_barrier(0x002, 14, 0);  // 14 VALU
        __builtin_amdgcn_sched_group_barrier(0x400, 1, 0);   // 1 transcendental
    }
    __builtin_amdgcn_sched_barrier(0);
}

template <int NGATHER, bool KEEP, bool OUT, int HAS_W, bool HAS_BASE>
__global__ __launch_bounds__(256, 2)
void k_gated_mlp_64(const float* __restrict__ erow,  // [E,64]
                    const float* __restrict__ WT,    // [64,128] row-major
                    const float* __restrict__ bias,  // [128]
                    const float* __restrict__ g0,    // [*,128] rows
                    const float* __restrict__ g1,
                    const float* __restrict__ g2,    // NGATHER==3 only
                    const int32_t* __restrict__ i0,
                    const int32_t* __restrict__ i1,
                    const int32_t* __restrict__ i2,
                    const float* __restrict__ w2c,   // [64,64] in x out
                    const float* __restrict__ w2g,
                    const float* __restrict__ b2c,   // [64]
                    const float* __restrict__ b2g,
                    const float* __restrict__ w,     // [E,64], HAS_W;
                                                     // 2: bexp [E,9]
                    const float* __restrict__ bs,    // [E,64], HAS_BASE
                    float* __restrict__ zout,        // [E,128], KEEP
                    float* __restrict__ cout,        // [E,64], KEEP
                    float* __restrict__ gout,        // [E,64], KEEP
                    float* __restrict__ out,         // [E,64], OUT
                    int64_t E,
                    // HAS_W == 2 only
                    const float* __restrict__ fwW,   // [64,9]
                    const float* __restrict__ fwmask) {  // [E] or null
    // the two parents' LDS images, unchanged
    __shared__ float4 wl1[64 * 32];
    __shared__ float4 wl2[64 * 32];
    __shared__ float4 bias4[32];
    __shared__ float4 wl9[HAS_W == 2 ? 64 * RBF_PAD / 4 : 1];
    __shared__ float4 bst[HAS_W == 2 ? (BLOCK / 64) * RBF_TILE / 4 : 1];
    if (HAS_W == 2) radial_stage_W((float*)wl9, fwW);
    for (int i = threadIdx.x; i < 64 * 32; i += blockDim.x) {
        const int k = i >> 5, col = i & 31;
        const float* p = WT + k * 128 + col;
        wl1[i] = make_float4(p[0], p[32], p[64], p[96]);
        wl2[i] = make_float4(w2c[k * 64 + col], w2c[k * 64 + 32 + col],
                             w2g[k * 64 + col], w2g[k * 64 + 32 + col]);
    }
    if (threadIdx.x < 32) {
        const float* p = bias + 4 * threadIdx.x;
        bias4[threadIdx.x] = make_float4(p[0], p[1], p[2], p[3]);
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int c0 = lane & 31;
    const int wave = threadIdx.x >> 6;
    const int waves_per_block = blockDim.x >> 6;
    const float4 bcol = make_float4(b2c[c0], b2c[32 + c0], b2g[c0],
                                    b2g[32 + c0]);
    const int64_t ntiles = (E + 31) >> 5;
    const int64_t stride = (int64_t)gridDim.x * waves_per_block;
    int64_t tile = blockIdx.x * (int64_t)waves_per_block + wave;
    if (tile >= ntiles) return;
    // lane (c, h): its own row's A fragment (floats [8i+4h, +4)) and indices.
    // Loaded one tile ahead: the loads of tile t+1 are issued as soon as
    // tile t's last first-layer MFMA has read a[], and are in flight during
    // the rest of tile t.
    float4 a[8];
    int32_t n0, n1, n2 = 0;
    auto load_tile = [&](int64_t t, int c, int h) {
        const int64_t r = (t << 5) + c;
        const int64_t lrow = r < E ? r : E - 1;   // clamp, never read past E
        // indices first: the gathers wait for them alone
        n0 = i0[lrow];
        n1 = i1[lrow];
        if (NGATHER == 3) n2 = i2[lrow];
        const float4* ap = (const float4*)(erow + lrow * 64) + h;
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = ap[2 * i];
    };
    load_tile(tile, lane & 31, lane >> 5);
    for (;;) {
        const int64_t base = tile << 5;
        // opaque copy per tile, as in the parents: keeps per-register
        // offsets from being hoisted out of the loop and spilled
        int lane_t = lane;
        asm volatile("" : "+v"(lane_t));
        const int c = lane_t & 31, h = lane_t >> 5;
        const float4* bl1 = wl1 + (4 * h) * 32 + c;
        const float4* bl2 = wl2 + (4 * h) * 32 + c;
        const int64_t r = base + c;
        const float4* p0 = (const float4*)(g0 + (int64_t)n0 * 128) + h;
        const float4* p1 = (const float4*)(g1 + (int64_t)n1 * 128) + h;
        const float4* p2 = NGATHER == 3
            ? (const float4*)(g2 + (int64_t)n2 * 128) + h : nullptr;
        float4* zrow = KEEP ? (float4*)(zout + r * 128) + h : nullptr;
        const bool live = r < E;
        float4 gv[NGATHER][8];
        gated_mlp_gather<NGATHER, 0>(gv, p0, p1, p2);
        __builtin_amdgcn_sched_barrier(0);   // all loads in flight first

        f32x16 z0[2], z1[2], acc[4];
        float4 h0s[8], h1s[8];
#pragma unroll
        for (int cb = 0; cb < 2; ++cb)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                z0[cb][q] = 0.0f; z1[cb][q] = 0.0f;
                acc[cb][q] = 0.0f; acc[2 + cb][q] = 0.0f;
            }
        // a wave inside its MFMA runs outranks waves in their memory phases
        __builtin_amdgcn_s_setprio(3);
        // ---- first layer, core half (z columns 0-63) --------------------
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float av[4] = {a[i].x, a[i].y, a[i].z, a[i].w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float4 b = bl1[(8 * i + t) * 32];   // k = 8i + 4h + t
                z0[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b.x, av[t], z0[0], 0, 0, 0);
                z0[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b.y, av[t], z0[1], 0, 0, 0);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        // ---- first layer, gate half (z columns 64-127), with the core
        //      half's epilogue in its MFMA gaps ---------------------------
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float av[4] = {a[i].x, a[i].y, a[i].z, a[i].w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float4 b = bl1[(8 * i + t) * 32];
                z1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(b.z, av[t], z1[0], 0, 0, 0);
                z1[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(b.w, av[t], z1[1], 0, 0, 0);
            }
            gated_mlp_slice_epilogue<NGATHER, KEEP, 0>(z0, gv, bias4 + h, zrow,
                                                      live, h0s, i);
            gated_mlp_interleave();
        }
        // the gate half's gathers, then a[] and the indices are dead: the
        // next tile's (the last tile reloads its own, clamped as ever)
        gated_mlp_gather<NGATHER, 1>(gv, p0, p1, p2);
        const int64_t next = tile + stride;
        const bool more = next < ntiles;
        load_tile(more ? next : tile, c, h);
        __builtin_amdgcn_sched_barrier(0);
        // ---- second layer, c, with the gate half's epilogue in its gaps --
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float lo[4] = {h0s[i].x, h0s[i].y, h0s[i].z, h0s[i].w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float4 b = bl2[(8 * i + t) * 32];   // k = 8i + 4h + t
                acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(lo[t], b.x, acc[0], 0, 0, 0);
                acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(lo[t], b.y, acc[1], 0, 0, 0);
            }
            gated_mlp_slice_epilogue<NGATHER, KEEP, 1>(z1, gv, bias4 + h, zrow,
                                                      live, h1s, i);
            gated_mlp_interleave();
        }
        // w and base of all 16 accumulator rows fly during the last MFMA run
        float wv[16][2], bv[16][2], sv[6];
        if (HAS_W == 2) radial_tile_load(sv, w, fwmask, base, E, lane_t);
        // (always the clamping form: a branch to the unclamped one on full
        // tiles spills, 96-344 B of scratch in six variants)
        mlp_tail_fwd_loads<HAS_W, HAS_BASE, false, 16>(wv, bv, 0, w, bs, base,
                                                       E, c, h);
        __builtin_amdgcn_sched_barrier(0);
        // ---- second layer, g ---------------------------------------------
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float hi[4] = {h1s[i].x, h1s[i].y, h1s[i].z, h1s[i].w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const float4 b = bl2[(8 * i + t) * 32];
                acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(hi[t], b.z, acc[2], 0, 0, 0);
                acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(hi[t], b.w, acc[3], 0, 0, 0);
            }
        }
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        // factored w: the tile's bexp block into the wave's LDS region, the
        // lane's two W rows out of the image
        float* st = (float*)bst + wave * RBF_TILE;
        float wc[2][N_RBF];
        if (HAS_W == 2) {
            radial_tile_store(st, sv, lane_t);
            radial_lane_W(wc, wl9, c);
        }
        const float4* st4 = (const float4*)st + (4 * h) * (RBF_PAD / 4);
        if (base + 32 <= E)
            mlp_tail_fwd_rows<KEEP, HAS_W, HAS_BASE, true, OUT, 16>(
                acc, bcol, wv, bv, 0, cout, gout, out, base, E, c, h, st4, wc);
        else
            mlp_tail_fwd_rows<KEEP, HAS_W, HAS_BASE, false, OUT, 16>(
                acc, bcol, wv, bv, 0, cout, gout, out, base, E, c, h, st4, wc);
        if (!more) break;
        tile = next;
    }
}

// ---------------------------------------------------------------------------
// GPU cell-list neighbor search (diagonal lattice, full PBC, min-image via
// cell wrap).  fp64 math replicates the CPU builder's decisions exactly.
// One thread per CENTER atom; center = dst so emission order is already
// the dst-sorted scatter layout.
// ---------------------------------------------------------------------------
template <bool FILL>
__global__ void k_nl(const double* __restrict__ pos,
                     const int32_t* __restrict__ cid,
                     const int32_t* __restrict__ order,
                     const int32_t* __restrict__ cell_start,
                     int32_t ncx, int32_t ncy, int32_t ncz,
                     double lx, double ly, double lz,
                     double r2tol, double tol, double br2tol,
                     const int32_t* __restrict__ row_ptr,
                     int32_t* __restrict__ cnt_or_src,
                     int8_t* __restrict__ off_i8,
                     uint8_t* __restrict__ bond_flag, int64_t N) {
    for (int64_t c = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         c < N; c += (int64_t)gridDim.x * blockDim.x) {
        const double xc = pos[3 * c], yc = pos[3 * c + 1], zc = pos[3 * c + 2];
        const int32_t cc = cid[c];
        const int32_t cx = cc / (ncy * ncz);
        const int32_t cy = (cc / ncz) % ncy;
        const int32_t cz = cc % ncz;
        int32_t n_emit = 0;
        int64_t w = FILL ? row_ptr[c] : 0;
        for (int dx = -1; dx <= 1; ++dx) {
            int32_t ax = cx + dx; int mx = 0;
            if (ax < 0) { ax += ncx; mx = -1; }
            else if (ax >= ncx) { ax -= ncx; mx = 1; }
            const double sx = mx * lx;
            for (int dy = -1; dy <= 1; ++dy) {
                int32_t ay = cy + dy; int my = 0;
                if (ay < 0) { ay += ncy; my = -1; }
                else if (ay >= ncy) { ay -= ncy; my = 1; }
                const double sy = my * ly;
                for (int dz = -1; dz <= 1; ++dz) {
                    int32_t az = cz + dz; int mz = 0;
                    if (az < 0) { az += ncz; mz = -1; }
                    else if (az >= ncz) { az -= ncz; mz = 1; }
                    const double sz = mz * lz;
                    const int32_t cell = (ax * ncy + ay) * ncz + az;
                    const int32_t lo = cell_start[cell], hi = cell_start[cell + 1];
                    for (int32_t q = lo; q < hi; ++q) {
                        const int32_t j = order[q];
                        if (j == c) continue;           // fpis.c:833
                        const double ddx = pos[3 * j] + sx - xc;
                        const double ddy = pos[3 * j + 1] + sy - yc;
                        const double ddz = pos[3 * j + 2] + sz - zc;
                        const double d2 = ddx * ddx + ddy * ddy + ddz * ddz;
                        if (d2 < r2tol && d2 > tol) {
                            if (FILL) {
                                cnt_or_src[w] = j;
                                // bv = pos[dst=c] + off*L - pos[src=j]
                                // must equal -(pos_j + m*L - pos_c): off = -m
                                off_i8[3 * w] = (int8_t)(-mx);
                                off_i8[3 * w + 1] = (int8_t)(-my);
                                off_i8[3 * w + 2] = (int8_t)(-mz);
                                bond_flag[w] = (d2 < br2tol) ? 1 : 0;
                                ++w;
                            } else {
                                ++n_emit;
                            }
                        }
                    }
                }
            }
        }
        if (!FILL) cnt_or_src[c] = n_emit;
    }
}

// ---------------------------------------------------------------------------
// General-lattice variant: any non-singular cell, any pbc, any cell count.
// The grid lives in FRACTIONAL space (nc cells per dim over the periodic
// unit interval, or over the atoms' extent in an open dim); the stencil
// walks UNWRAPPED cell indices a = c + d, d in [-R, R]: a periodic dim
// folds a into image m = floor_div(a, nc) and cell a - m*nc, an open dim
// skips a outside [0, nc).  Every (neighbor, image) pair is therefore
// visited exactly once for any nc (nc = 1: same cell, images -R..R;
// nc = 2: -1 and +1 are the same cell with different images).
// Thread t handles center order[t] (cell-sorted walk: a wave shares its
// candidate cells); rows are still addressed by atom id.  Lattice rows,
// grid and flags are kernel arguments (scalar registers).
// ---------------------------------------------------------------------------
struct NlGrid {
    double l[9];          // lattice rows, row-major
    int32_t nc[3], R[3], per[3];
};

__device__ inline int32_t floor_div(int32_t a, int32_t n) {
    return a >= 0 ? a / n : -((n - 1 - a) / n);
}

template <bool FILL>
__global__ void k_nl_gen(const double* __restrict__ pos,
                         const int32_t* __restrict__ cid,
                         const int32_t* __restrict__ order,
                         const int32_t* __restrict__ cell_start,
                         NlGrid g, double r2tol, double tol, double br2tol,
                         const int32_t* __restrict__ row_ptr,
                         int32_t* __restrict__ cnt_or_src,
                         int8_t* __restrict__ off_i8,
                         uint8_t* __restrict__ bond_flag, int64_t N) {
    const int32_t ncx = g.nc[0], ncy = g.nc[1], ncz = g.nc[2];
    for (int64_t t = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
         t < N; t += (int64_t)gridDim.x * blockDim.x) {
        const int32_t c = order[t];
        const double xc = pos[3 * (int64_t)c], yc = pos[3 * (int64_t)c + 1],
                     zc = pos[3 * (int64_t)c + 2];
        const int32_t cc = cid[c];
        const int32_t cx = cc / (ncy * ncz);
        const int32_t cy = (cc / ncz) % ncy;
        const int32_t cz = cc % ncz;
        int32_t n_emit = 0;
        int64_t w = FILL ? row_ptr[c] : 0;
        for (int dx = -g.R[0]; dx <= g.R[0]; ++dx) {
            int32_t ax = cx + dx, mx = 0;
            if (g.per[0]) { mx = floor_div(ax, ncx); ax -= mx * ncx; }
            else if (ax < 0 || ax >= ncx) continue;
            for (int dy = -g.R[1]; dy <= g.R[1]; ++dy) {
                int32_t ay = cy + dy, my = 0;
                if (g.per[1]) { my = floor_div(ay, ncy); ay -= my * ncy; }
                else if (ay < 0 || ay >= ncy) continue;
                for (int dz = -g.R[2]; dz <= g.R[2]; ++dz) {
                    int32_t az = cz + dz, mz = 0;
                    if (g.per[2]) { mz = floor_div(az, ncz); az -= mz * ncz; }
                    else if (az < 0 || az >= ncz) continue;
                    // shift = m @ lattice (graph_build.cpp image shift)
                    const double sx = mx * g.l[0] + my * g.l[3] + mz * g.l[6];
                    const double sy = mx * g.l[1] + my * g.l[4] + mz * g.l[7];
                    const double sz = mx * g.l[2] + my * g.l[5] + mz * g.l[8];
                    const int32_t cell = (ax * ncy + ay) * ncz + az;
                    const int32_t lo = cell_start[cell], hi = cell_start[cell + 1];
                    for (int32_t q = lo; q < hi; ++q) {
                        const int32_t j = order[q];
                        if (j == c) continue;           // fpis.c:833
                        const double ddx = pos[3 * (int64_t)j] + sx - xc;
                        const double ddy = pos[3 * (int64_t)j + 1] + sy - yc;
                        const double ddz = pos[3 * (int64_t)j + 2] + sz - zc;
                        const double d2 = ddx * ddx + ddy * ddy + ddz * ddz;
                        if (d2 < r2tol && d2 > tol) {
                            if (FILL) {
                                cnt_or_src[w] = j;
                                off_i8[3 * w] = (int8_t)(-mx);      // off = -m
                                off_i8[3 * w + 1] = (int8_t)(-my);
                                off_i8[3 * w + 2] = (int8_t)(-mz);
                                bond_flag[w] = (d2 < br2tol) ? 1 : 0;
                                ++w;
                            } else {
                                ++n_emit;
                            }
                        }
                    }
                }
            }
        }
        if (!FILL) cnt_or_src[c] = n_emit;
    }
}

}  // namespace


// ---------------------------------------------------------------------------
// MACE uvu tensor product, fused per edge (round 2; the equivariant
// per-edge message contraction of the MACE interactions — reference
// delegates it to e3nn TensorProduct, implementations/mace/models.py:144-152).
// One 64-lane wave per edge, channels split across lanes (CPL = C/64 per
// lane).  CG nonzeros stream through the SCALAR cache (wave-uniform
// entries, sorted by path so the per-path weight row loads once);
// k-indexed accumulators live in LDS (dynamic register indexing would
// spill to scratch).  Everything HBM-side is lane-contiguous.
// ---------------------------------------------------------------------------

template <int CPL>
__global__ void k_mace_tp_fwd(const float* __restrict__ x0,
                              const float* __restrict__ x1,
                              const float* __restrict__ Y,
                              const float* __restrict__ w,
                              const int32_t* __restrict__ nz,
                              const float* __restrict__ nzc,
                              int32_t nnz,
                              float* __restrict__ o0,
                              float* __restrict__ o1,
                              float* __restrict__ o2,
                              float* __restrict__ o3,
                              int64_t E, int32_t C, int32_t P,
                              int32_t d1b) {
    __shared__ float acc[CPL * 16 * 4 * 64];     // [i][k3][wave][lane]
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    for (int64_t e = blockIdx.x * (int64_t)nw + wid; e < E;
         e += (int64_t)gridDim.x * nw) {
        float xr0[CPL];
        float xr1[CPL > 0 ? CPL : 1][3];
        for (int i = 0; i < CPL; ++i)
            xr0[i] = x0[e * C + lane + i * 64];
        if (x1 != nullptr)
            for (int i = 0; i < CPL; ++i)
                for (int k = 0; k < 3; ++k)
                    xr1[i][k] = (k < d1b)
                        ? x1[(e * C + lane + i * 64) * d1b + k] : 0.0f;
        for (int i = 0; i < CPL; ++i)
            for (int k3 = 0; k3 < 16; ++k3)
                acc[((i * 16 + k3) * 4 + wid) * 64 + lane] = 0.0f;
        const float* Ye = Y + e * 16;
        int curp = -1;
        float wreg[CPL];
        for (int32_t t = 0; t < nnz; ++t) {
            const int32_t p = nz[5 * t], slot = nz[5 * t + 1],
                          k1 = nz[5 * t + 2], k2 = nz[5 * t + 3],
                          k3 = nz[5 * t + 4];
            if (p != curp) {
                curp = p;
                for (int i = 0; i < CPL; ++i)
                    wreg[i] = w[((int64_t)e * P + p) * C + lane + i * 64];
            }
            const float cy = nzc[t] * Ye[k2];
            for (int i = 0; i < CPL; ++i) {
                float xv;                      // k1 is wave-uniform:
                if (slot == 0) xv = xr0[i];    // scalar-predicated chain,
                else if (k1 == 0) xv = xr1[i][0];   // no scratch spill
                else if (k1 == 1) xv = xr1[i][1];
                else xv = xr1[i][2];
                acc[((i * 16 + k3) * 4 + wid) * 64 + lane]
                    += cy * wreg[i] * xv;
            }
        }
        // k3 -> (l3 block, row) writeback into the four per-l3 tensors
        // ([E, d3, C] each — contiguous rows for the scatter kernel)
        float* const outs[4] = {o0, o1, o2, o3};
        static const int BLK[16] = {0,1,1,1,2,2,2,2,2,3,3,3,3,3,3,3};
        static const int ROW[16] = {0,0,1,2,0,1,2,3,4,0,1,2,3,4,5,6};
        static const int DD[4] = {1,3,5,7};
#pragma unroll
        for (int k3 = 0; k3 < 16; ++k3)
            for (int i = 0; i < CPL; ++i)
                outs[BLK[k3]][((int64_t)e * DD[BLK[k3]] + ROW[k3]) * C
                              + lane + i * 64] =
                    acc[((i * 16 + k3) * 4 + wid) * 64 + lane];
    }
}

template <int CPL>
__global__ void k_mace_tp_bwd(const float* __restrict__ g0,
                              const float* __restrict__ g1,
                              const float* __restrict__ g2,
                              const float* __restrict__ g3,
                              const float* __restrict__ x0,
                              const float* __restrict__ x1,
                              const float* __restrict__ Y,
                              const float* __restrict__ w,
                              const int32_t* __restrict__ nz,
                              const float* __restrict__ nzc,
                              int32_t nnz,
                              float* __restrict__ dx0,
                              float* __restrict__ dx1,
                              float* __restrict__ dY,
                              float* __restrict__ dw,
                              int64_t E, int32_t C, int32_t P,
                              int32_t d1b) {
    // LDS: go rows (dynamic k3 reads) + per-lane dY partials (dynamic k2)
    __shared__ float gob[CPL * 16 * 4 * 64];
    __shared__ float dyb[16 * 4 * 64];
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    for (int64_t e = blockIdx.x * (int64_t)nw + wid; e < E;
         e += (int64_t)gridDim.x * nw) {
        float xr0[CPL];
        float xr1[CPL > 0 ? CPL : 1][3];
        float dxr0[CPL] = {};
        float dxr1[CPL > 0 ? CPL : 1][3] = {};
        for (int i = 0; i < CPL; ++i)
            xr0[i] = x0[e * C + lane + i * 64];
        if (x1 != nullptr)
            for (int i = 0; i < CPL; ++i)
                for (int k = 0; k < 3; ++k)
                    xr1[i][k] = (k < d1b)
                        ? x1[(e * C + lane + i * 64) * d1b + k] : 0.0f;
        {
            const float* const gos[4] = {g0, g1, g2, g3};
            static const int BLK[16] = {0,1,1,1,2,2,2,2,2,3,3,3,3,3,3,3};
            static const int ROW[16] = {0,0,1,2,0,1,2,3,4,0,1,2,3,4,5,6};
            static const int DD[4] = {1,3,5,7};
#pragma unroll
            for (int k3 = 0; k3 < 16; ++k3)
                for (int i = 0; i < CPL; ++i)
                    gob[((i * 16 + k3) * 4 + wid) * 64 + lane] =
                        gos[BLK[k3]][((int64_t)e * DD[BLK[k3]] + ROW[k3])
                                     * C + lane + i * 64];
        }
        for (int k2 = 0; k2 < 16; ++k2)
            dyb[(k2 * 4 + wid) * 64 + lane] = 0.0f;
        const float* Ye = Y + e * 16;
        int curp = -1;
        float wreg[CPL];
        float dwacc[CPL] = {};
        for (int32_t t = 0; t < nnz; ++t) {
            const int32_t p = nz[5 * t], slot = nz[5 * t + 1],
                          k1 = nz[5 * t + 2], k2 = nz[5 * t + 3],
                          k3 = nz[5 * t + 4];
            if (p != curp) {
                if (curp >= 0)
                    for (int i = 0; i < CPL; ++i) {
                        dw[((int64_t)e * P + curp) * C + lane + i * 64] =
                            dwacc[i];
                        dwacc[i] = 0.0f;
                    }
                curp = p;
                for (int i = 0; i < CPL; ++i)
                    wreg[i] = w[((int64_t)e * P + p) * C + lane + i * 64];
            }
            const float c = nzc[t];
            const float yv = Ye[k2];
            for (int i = 0; i < CPL; ++i) {
                const float g = gob[((i * 16 + k3) * 4 + wid) * 64 + lane];
                float xv;
                if (slot == 0) xv = xr0[i];
                else if (k1 == 0) xv = xr1[i][0];
                else if (k1 == 1) xv = xr1[i][1];
                else xv = xr1[i][2];
                const float cg = c * g;
                // d x
                const float dxv = cg * yv * wreg[i];
                if (slot == 0) dxr0[i] += dxv;
                else if (k1 == 0) dxr1[i][0] += dxv;
                else if (k1 == 1) dxr1[i][1] += dxv;
                else dxr1[i][2] += dxv;
                // d w
                dwacc[i] += cg * yv * xv;
                // d Y (per-lane partial; reduced after the loop)
                dyb[(k2 * 4 + wid) * 64 + lane] += cg * wreg[i] * xv;
            }
        }
        if (curp >= 0)
            for (int i = 0; i < CPL; ++i)
                dw[((int64_t)e * P + curp) * C + lane + i * 64] = dwacc[i];
        for (int i = 0; i < CPL; ++i)
            dx0[e * C + lane + i * 64] = dxr0[i];
        if (dx1 != nullptr)
            for (int i = 0; i < CPL; ++i)
                for (int k = 0; k < d1b; ++k)
                    dx1[(e * C + lane + i * 64) * d1b + k] = dxr1[i][k];
        // reduce dY partials across the wave: waves are lockstep, each
        // owns its LDS stripe — no block barrier (one inside this
        // grid-stride loop would deadlock when wave trip counts differ)
        if (lane < 16) {
            float s = 0.0f;
            for (int l2 = 0; l2 < 64; ++l2)
                s += dyb[(lane * 4 + wid) * 64 + l2];
            dY[e * 16 + lane] = s;
        }
    }
}



// ---------------------------------------------------------------------------
// MACE symmetric contraction, fused per node (round 2).  Replaces the
// SymmetricContraction of mace's EquivariantProductBasisBlock (the
// reference delegates to mace.modules.symmetric_contraction via
// models.py:155-157): out[n, orow, c] = sum_entries
// W[elem(n), wrow, c] * coef * x[n,a,c] * x[n,b,c] * x[n,k,c], with the
// sentinel row x[16] == 1 encoding nu<3 terms.  Entries are wave-uniform
// (scalar cache), sorted by wrow so each weight row loads once; weights
// are FROZEN (inference engine), so backward produces dx only.
// ---------------------------------------------------------------------------

template <int CPL>
__global__ void k_mace_symc_fwd(const float* __restrict__ x,
                                const int32_t* __restrict__ elem,
                                const float* __restrict__ W,
                                const int32_t* __restrict__ nz,
                                const float* __restrict__ nzc,
                                int32_t nnz, float* __restrict__ out,
                                int64_t N, int32_t C, int32_t T,
                                int32_t S_out) {
    // x rows AND accumulators in LDS: a/b/k/orow are runtime indices
    // (dynamic register-array indexing would spill to scratch)
    __shared__ float acc[4 * 4 * 64 * CPL];       // [orow][wave][lane][i]
    __shared__ float xls[17 * 4 * 64 * CPL];      // [row][wave][lane][i]
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
#define XR(a, i) xls[(((a) * 4 + wid) * 64 + lane) * CPL + (i)]
    for (int64_t n = blockIdx.x * (int64_t)nw + wid; n < N;
         n += (int64_t)gridDim.x * nw) {
        for (int a = 0; a < 16; ++a)
            for (int i = 0; i < CPL; ++i)
                XR(a, i) = x[((int64_t)n * 16 + a) * C + lane + i * 64];
        for (int i = 0; i < CPL; ++i)
            XR(16, i) = 1.0f;
        for (int o = 0; o < S_out; ++o)
            for (int i = 0; i < CPL; ++i)
                acc[((o * 4 + wid) * 64 + lane) * CPL + i] = 0.0f;
        const int64_t wbase = (int64_t)elem[n] * T;
        int curw = -1;
        float wreg[CPL];
        for (int32_t t = 0; t < nnz; ++t) {
            const int32_t wrow = nz[6 * t], a = nz[6 * t + 1],
                          b = nz[6 * t + 2], k = nz[6 * t + 3],
                          orow = nz[6 * t + 4];
            if (wrow != curw) {
                curw = wrow;
                for (int i = 0; i < CPL; ++i)
                    wreg[i] = W[(wbase + wrow) * C + lane + i * 64];
            }
            const float c = nzc[t];
            for (int i = 0; i < CPL; ++i) {
                const float v = c * wreg[i] * XR(a, i) * XR(b, i)
                                * XR(k, i);
                acc[((orow * 4 + wid) * 64 + lane) * CPL + i] += v;
            }
        }
        for (int o = 0; o < S_out; ++o)
            for (int i = 0; i < CPL; ++i)
                out[((int64_t)n * S_out + o) * C + lane + i * 64] =
                    acc[((o * 4 + wid) * 64 + lane) * CPL + i];
    }
#undef XR
}

template <int CPL>
__global__ void k_mace_symc_bwd(const float* __restrict__ go,
                                const float* __restrict__ x,
                                const int32_t* __restrict__ elem,
                                const float* __restrict__ W,
                                const int32_t* __restrict__ nz,
                                const float* __restrict__ nzc,
                                int32_t nnz, float* __restrict__ dx,
                                int64_t N, int32_t C, int32_t T,
                                int32_t S_out) {
    __shared__ float dacc[17 * 4 * 64 * CPL];     // row 16 = sentinel sink
    __shared__ float xls[17 * 4 * 64 * CPL];
    __shared__ float gls[4 * 4 * 64 * CPL];
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
#define XRB(a, i) xls[(((a) * 4 + wid) * 64 + lane) * CPL + (i)]
#define GOB(o, i) gls[(((o) * 4 + wid) * 64 + lane) * CPL + (i)]
    for (int64_t n = blockIdx.x * (int64_t)nw + wid; n < N;
         n += (int64_t)gridDim.x * nw) {
        for (int a = 0; a < 16; ++a)
            for (int i = 0; i < CPL; ++i)
                XRB(a, i) = x[((int64_t)n * 16 + a) * C + lane + i * 64];
        for (int i = 0; i < CPL; ++i)
            XRB(16, i) = 1.0f;
        for (int o = 0; o < S_out; ++o)
            for (int i = 0; i < CPL; ++i)
                GOB(o, i) = go[((int64_t)n * S_out + o) * C + lane
                               + i * 64];
        for (int a = 0; a < 17; ++a)
            for (int i = 0; i < CPL; ++i)
                dacc[((a * 4 + wid) * 64 + lane) * CPL + i] = 0.0f;
        const int64_t wbase = (int64_t)elem[n] * T;
        int curw = -1;
        float wreg[CPL];
        for (int32_t t = 0; t < nnz; ++t) {
            const int32_t wrow = nz[6 * t], a = nz[6 * t + 1],
                          b = nz[6 * t + 2], k = nz[6 * t + 3],
                          orow = nz[6 * t + 4];
            if (wrow != curw) {
                curw = wrow;
                for (int i = 0; i < CPL; ++i)
                    wreg[i] = W[(wbase + wrow) * C + lane + i * 64];
            }
            const float c = nzc[t];
            for (int i = 0; i < CPL; ++i) {
                const float g = c * wreg[i] * GOB(orow, i);
                const float xa = XRB(a, i), xb = XRB(b, i),
                            xk = XRB(k, i);
                dacc[((a * 4 + wid) * 64 + lane) * CPL + i] += g * xb * xk;
                dacc[((b * 4 + wid) * 64 + lane) * CPL + i] += g * xa * xk;
                dacc[((k * 4 + wid) * 64 + lane) * CPL + i] += g * xa * xb;
            }
        }
        for (int a = 0; a < 16; ++a)
            for (int i = 0; i < CPL; ++i)
                dx[((int64_t)n * 16 + a) * C + lane + i * 64] =
                    dacc[((a * 4 + wid) * 64 + lane) * CPL + i];
    }
#undef XRB
#undef GOB
}



// ---------------------------------------------------------------------------
// eSCN/UMA per-edge Wigner rotations (round 2).  The reference's UMA path
// applies per-edge block-diagonal Wigner matrices around every SO(2)
// convolution (escn_md.py:283-291, delegated to fairchem/e3nn); as batched
// bmms of (S x S)(S x C) tiles these run rocBLAS at ~1% of peak (62% of a
// 16 s step, profiles/r2_uma_kernel_stats.csv).  Here: one wave per edge
// (gather/apply) or per node (apply/scatter over the dst CSR), D rows
// streamed wave-uniform through the scalar cache, channels across lanes.
// S = 9 (lmax 2).  trans selects D vs D^T (the inverse rotation).
// ---------------------------------------------------------------------------

template <int CPL>
__global__ void k_rot_gather(const float* __restrict__ h,
                             const int32_t* __restrict__ idx,
                             const float* __restrict__ D, int32_t trans,
                             float* __restrict__ out, int64_t E,
                             int32_t C) {
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    for (int64_t e = blockIdx.x * (int64_t)nw + wid; e < E;
         e += (int64_t)gridDim.x * nw) {
        const int64_t row = idx ? (int64_t)idx[e] : e;
        float hr[9][CPL];
        for (int t = 0; t < 9; ++t)
            for (int i = 0; i < CPL; ++i)
                hr[t][i] = h[(row * 9 + t) * C + lane + i * 64];
        const float* De = D + e * 81;
        for (int s = 0; s < 9; ++s) {
            float acc[CPL] = {};
            for (int t = 0; t < 9; ++t) {
                const float d = trans ? De[t * 9 + s] : De[s * 9 + t];
                for (int i = 0; i < CPL; ++i)
                    acc[i] += d * hr[t][i];
            }
            for (int i = 0; i < CPL; ++i)
                out[((int64_t)e * 9 + s) * C + lane + i * 64] = acc[i];
        }
    }
}

template <int CPL>
__global__ void k_rot_scatter(const float* __restrict__ mt,
                              const float* __restrict__ D, int32_t trans,
                              const int32_t* __restrict__ perm,
                              const int32_t* __restrict__ row_ptr,
                              const float* __restrict__ base,
                              float* __restrict__ out, int64_t N,
                              int32_t C) {
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    for (int64_t n = blockIdx.x * (int64_t)nw + wid; n < N;
         n += (int64_t)gridDim.x * nw) {
        float acc[9][CPL] = {};
        const int32_t lo = row_ptr[n], hi = row_ptr[n + 1];
        for (int32_t q = lo; q < hi; ++q) {
            const int64_t e = perm ? (int64_t)perm[q] : (int64_t)q;
            const float* De = D + e * 81;
            float mr[9][CPL];
            for (int t = 0; t < 9; ++t)
                for (int i = 0; i < CPL; ++i)
                    mr[t][i] = mt[(e * 9 + t) * C + lane + i * 64];
            for (int s = 0; s < 9; ++s)
                for (int t = 0; t < 9; ++t) {
                    const float d = trans ? De[t * 9 + s] : De[s * 9 + t];
                    for (int i = 0; i < CPL; ++i)
                        acc[s][i] += d * mr[t][i];
                }
        }
        for (int s = 0; s < 9; ++s)
            for (int i = 0; i < CPL; ++i) {
                const int64_t o = ((int64_t)n * 9 + s) * C + lane + i * 64;
                out[o] = acc[s][i] + (base ? base[o] : 0.0f);
            }
    }
}

template <int CPL>
__global__ void k_rot_dD(const float* __restrict__ go,
                         const float* __restrict__ h,
                         const int32_t* __restrict__ idx, int32_t trans,
                         float* __restrict__ dD, int64_t E, int32_t C) {
    // dD(s,t) = sum_c go[e,s,c] * in[row,t,c]; trans writes transposed
    const int lane = threadIdx.x & 63;
    const int wid = threadIdx.x >> 6;
    const int nw = blockDim.x >> 6;
    for (int64_t e = blockIdx.x * (int64_t)nw + wid; e < E;
         e += (int64_t)gridDim.x * nw) {
        const int64_t row = idx ? (int64_t)idx[e] : e;
        float hr[9][CPL], gr[9][CPL];
        for (int t = 0; t < 9; ++t)
            for (int i = 0; i < CPL; ++i) {
                hr[t][i] = h[(row * 9 + t) * C + lane + i * 64];
                gr[t][i] = go[((int64_t)e * 9 + t) * C + lane + i * 64];
            }
        for (int s = 0; s < 9; ++s)
            for (int t = 0; t < 9; ++t) {
                float p = 0.0f;
                for (int i = 0; i < CPL; ++i)
                    p += gr[s][i] * hr[t][i];
                // wave reduction (butterfly over 64 lanes)
                for (int off = 32; off > 0; off >>= 1)
                    p += __shfl_xor(p, off, 64);
                if (lane == 0)
                    dD[e * 81 + (trans ? t * 9 + s : s * 9 + t)] = p;
            }
    }
}


// dm_gated_mlp_tail_fwd_f32's launch, by variant
template <bool KEEP, int HAS_W>
static void launch_mlp_tail_fwd(const float* h, const float* w2c,
                                const float* w2g, const float* b2c,
                                const float* b2g, const float* w,
                                const float* base, float* c_out, float* g_out,
                                float* out, int64_t E, hipStream_t s,
                                const float* fwW = nullptr,
                                const float* fwmask = nullptr) {
    if (base)
        k_gated_mlp_tail_fwd<KEEP, HAS_W, true>
            <<<edge_mlp_blocks(E), BLOCK, 0, s>>>(
                h, w2c, w2g, b2c, b2g, w, base, c_out, g_out, out, E, fwW,
                fwmask);
    else
        k_gated_mlp_tail_fwd<KEEP, HAS_W, false>
            <<<edge_mlp_blocks(E), BLOCK, 0, s>>>(
                h, w2c, w2g, b2c, b2g, w, nullptr, c_out, g_out, out, E, fwW,
                fwmask);
}

// dm_gated_mlp3/4_f32: checks and launch, by form
template <int NGATHER>
static int gated_mlp_run(const float* erow, const float* WT, const float* bias,
                         const float* g0, const float* g1, const float* g2,
                         const int32_t* i0, const int32_t* i1,
                         const int32_t* i2, const float* w2c, const float* w2g,
                         const float* b2c, const float* b2g, const float* w,
                         const float* base, float* z_out, float* c_out,
                         float* g_out, float* out, int64_t E, int64_t Din,
                         int64_t d, hipStream_t s,
                         const float* fwW = nullptr,
                         const float* fwmask = nullptr) {
    if (Din != 64 || d != 64) {
        g_err = "gated_mlp fused kernel is compiled for Din=64, d=64";
        return -1;
    }
    if ((c_out == nullptr) != (g_out == nullptr)) {
        g_err = "gated_mlp: c_out and g_out must be given together";
        return -1;
    }
    if ((z_out == nullptr) != (c_out == nullptr)) {
        g_err = "gated_mlp: z_out and c_out/g_out must be given together";
        return -1;
    }
    if (!z_out && !out) {
        g_err = "gated_mlp: the no-keep form needs out";
        return -1;
    }
    if (!i0 || !i1 || (NGATHER == 3 && !i2)) {
        g_err = "gated_mlp: NULL index";
        return -1;
    }
    if (!erow || !WT || !bias || !g0 || !g1 || (NGATHER == 3 && !g2) || !w2c ||
        !w2g || !b2c || !b2g) {
        g_err = "gated_mlp: NULL input";
        return -1;
    }
    // rows are read and written as float4 slices
    if ((((uintptr_t)erow | (uintptr_t)g0 | (uintptr_t)g1 | (uintptr_t)g2 |
          (uintptr_t)z_out) & 15) != 0) {
        g_err = "gated_mlp: erow, the gather tables and z_out must be 16-byte aligned";
        return -1;
    }
    // factored w: w is bexp [E,9]; the two-gather forms with out only
    if (fwW && (NGATHER != 2 || !w || !out)) {
        g_err = "gated_mlp: the factored-w form is the two-gather one with "
                "bexp and out";
        return -1;
    }
    if (E <= 0) return 0;
    const int grid = gated_mlp_blocks(E);
#define DM_GMLP_LAUNCH(KEEP, OUT, HW, HB)                                    \
    k_gated_mlp_64<NGATHER, KEEP, OUT, HW, HB><<<grid, BLOCK, 0, s>>>(       \
        erow, WT, bias, g0, g1, g2, i0, i1, i2, w2c, w2g, b2c, b2g, w, base, \
        z_out, c_out, g_out, out, E, fwW, fwmask)
    if constexpr (NGATHER == 2) {
        if (fwW) {
            if (z_out && base) DM_GMLP_LAUNCH(true, true, 2, true);
            else if (z_out) DM_GMLP_LAUNCH(true, true, 2, false);
            else if (base) DM_GMLP_LAUNCH(false, true, 2, true);
            else DM_GMLP_LAUNCH(false, true, 2, false);
            DM_CHECK_LAUNCH();
            return 0;
        }
    }
#define DM_GMLP_WB(KEEP)                                                     \
    do {                                                                     \
        if (w && base) DM_GMLP_LAUNCH(KEEP, true, true, true);               \
        else if (w) DM_GMLP_LAUNCH(KEEP, true, true, false);                 \
        else if (base) DM_GMLP_LAUNCH(KEEP, true, false, true);              \
        else DM_GMLP_LAUNCH(KEEP, true, false, false);                       \
    } while (0)
    if (!z_out) DM_GMLP_WB(false);
    else if (out) DM_GMLP_WB(true);
    else DM_GMLP_LAUNCH(true, false, false, false);   // w, base not read
#undef DM_GMLP_WB
#undef DM_GMLP_LAUNCH
    DM_CHECK_LAUNCH();
    return 0;
}

// The library's other translation units (tensornet.hip) report through the
// same per-thread message dm_hip_last_error() returns.  Not exported.
__attribute__((visibility("hidden")))
void dm_set_last_error(const char* msg) { g_err = msg; }

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int dm_gather_rows_f32(const float* x, const int32_t* idx, float* out,
                       int64_t n_out, int64_t D, uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (D % 4 == 0) {
        const int64_t total = n_out * (D / 4);
        k_gather_rows_v4<<<nblocks(total, BLOCK), BLOCK, 0, s>>>(
            (const float4*)x, idx, (float4*)out, total, (int32_t)(D / 4));
    } else {
        const int64_t total = n_out * D;
        k_gather_rows_s<<<nblocks(total, BLOCK), BLOCK, 0, s>>>(
            x, idx, out, total, (int32_t)D);
    }
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_edge_mlp3_f32(const float* erow, const float* WT, const float* bias,
                     const float* zs, const float* zd, const int32_t* src,
                     const int32_t* dst, float* out, float* out_act,
                     int64_t E, int64_t Din, int64_t Dout, uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (Din != 64 || Dout != 128) {
        g_err = "edge_mlp fused kernel is compiled for Din=64, Dout=128";
        return -1;
    }
    // one wave per 32-edge tile, grid capped: waves loop over tiles
    k_edge_mlp_64x128<2><<<edge_mlp_blocks(E), BLOCK, 0, s>>>(
        erow, WT, bias, zs, zd, nullptr, src, dst, nullptr, out, out_act, E);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_edge_mlp4_f32(const float* arow, const float* WT, const float* bias,
                     const float* z1, const float* z2, const float* zv,
                     const int32_t* lsrc, const int32_t* ldst,
                     const int32_t* center, float* out, float* out_act,
                     int64_t L, int64_t Din, int64_t Dout, uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (Din != 64 || Dout != 128) {
        g_err = "edge_mlp fused kernel is compiled for Din=64, Dout=128";
        return -1;
    }
    k_edge_mlp_64x128<3><<<edge_mlp_blocks(L), BLOCK, 0, s>>>(
        arow, WT, bias, z1, z2, zv, lsrc, ldst, center, out, out_act, L);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_gather_add3_f32(const float* zs, const float* zd, const float* ze,
                       const int32_t* src, const int32_t* dst, float* out,
                       float* out_act, int64_t E, int64_t D,
                       uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (D % 4 != 0) { g_err = "gather_add3 requires D % 4 == 0"; return -1; }
    const int64_t total = E * (D / 4);
    k_gather_add3_v4<<<nblocks(total, BLOCK), BLOCK, 0, s>>>(
        (const float4*)zs, (const float4*)zd, (const float4*)ze, src, dst,
        (float4*)out, (float4*)out_act, total, (int32_t)(D / 4));
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_gather_add4_f32(const float* z1, const float* z2, const float* za,
                       const float* zv, const int32_t* lsrc,
                       const int32_t* ldst, const int32_t* center, float* out,
                       float* out_act, int64_t L, int64_t D,
                       uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (D % 4 != 0) { g_err = "gather_add4 requires D % 4 == 0"; return -1; }
    const int64_t total = L * (D / 4);
    k_gather_add4_v4<<<nblocks(total, BLOCK), BLOCK, 0, s>>>(
        (const float4*)z1, (const float4*)z2, (const float4*)za,
        (const float4*)zv, lsrc, ldst, center, (float4*)out,
        (float4*)out_act, total, (int32_t)(D / 4));
    DM_CHECK_LAUNCH();
    return 0;
}

static int g_seg_variant = []() {
    const char* v = getenv("DM_SEG_VARIANT");
    return v ? atoi(v) : 1;            // 1 = unroll-4 (default), 0 = plain
}();

int dm_seg_sum_f32(const float* msg, const int32_t* row_ptr,
                   const float* base, float* out, int64_t N, int64_t D,
                   uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (D % 4 == 0 && D / 4 <= 16) {
        if (g_seg_variant == 1)
            k_seg_sum_v4_u4<4><<<nblocks(N, 16), BLOCK, 0, s>>>(
                (const float4*)msg, row_ptr, (const float4*)base,
                (float4*)out, N, (int32_t)(D / 4));
        else
            k_seg_sum_v4<4><<<nblocks(N, 16), BLOCK, 0, s>>>(
                (const float4*)msg, row_ptr, (const float4*)base,
                (float4*)out, N, (int32_t)(D / 4));
    } else if (D % 4 == 0 && D / 4 <= 32) {      // D == 128: the backward
        k_seg_sum_v4_u4<5><<<nblocks(N, 8), BLOCK, 0, s>>>(   // dz sums
            (const float4*)msg, row_ptr, (const float4*)base,
            (float4*)out, N, (int32_t)(D / 4));
    } else {
        k_seg_sum_s<<<nblocks(N * D, BLOCK), BLOCK, 0, s>>>(
            msg, row_ptr, base, out, N, (int32_t)D);
    }
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_seg_sum_gather_f32(const float* msg, const int32_t* perm,
                          const int32_t* row_ptr, const float* base,
                          float* out, int64_t N, int64_t D, uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (D % 4 == 0 && D / 4 <= 16) {
        k_seg_sum_gather_v4<4><<<nblocks(N, 16), BLOCK, 0, s>>>(
            (const float4*)msg, perm, row_ptr, (const float4*)base,
            (float4*)out, N, (int32_t)(D / 4));
    } else if (D % 4 == 0 && D / 4 <= 32) {
        k_seg_sum_gather_v4<5><<<nblocks(N, 8), BLOCK, 0, s>>>(
            (const float4*)msg, perm, row_ptr, (const float4*)base,
            (float4*)out, N, (int32_t)(D / 4));
    } else {
        k_seg_sum_gather_s<<<nblocks(N * D, BLOCK), BLOCK, 0, s>>>(
            msg, perm, row_ptr, base, out, N, (int32_t)D);
    }
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_gated_combine_fwd_f32(const float* c, const float* g, const float* w,
                             const float* base, float* out, int64_t total,
                             uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    k_gated_combine_fwd<<<nblocks(total, BLOCK), BLOCK, 0, s>>>(
        c, g, w, base, out, total);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_gated_combine_bwd_f32(const float* go, const float* c, const float* g,
                             const float* w, float* dc, float* dg, float* dw,
                             int64_t total, uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    k_gated_combine_bwd<<<nblocks(total, BLOCK), BLOCK, 0, s>>>(
        go, c, g, w, dc, dg, dw, total);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_gated_mlp_tail_bwd_f32(const float* go, const float* c, const float* g,
                              const float* w, const float* z,
                              const float* w2c, const float* w2g, float* dz,
                              float* dw, int64_t E, int64_t d,
                              uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (d != 64) {
        g_err = "gated_mlp_tail_bwd fused kernel is compiled for d=64";
        return -1;
    }
    if ((w == nullptr) != (dw == nullptr)) {
        g_err = "gated_mlp_tail_bwd: w and dw must be given together";
        return -1;
    }
    if (E <= 0) return 0;
    if (w)
        k_gated_mlp_tail_bwd<1, false><<<edge_mlp_blocks(E), BLOCK, 0, s>>>(
            go, nullptr, c, g, w, z, w2c, w2g, dz, dw, E, nullptr, nullptr,
            nullptr, nullptr);
    else
        k_gated_mlp_tail_bwd<0, false><<<edge_mlp_blocks(E), BLOCK, 0, s>>>(
            go, nullptr, c, g, nullptr, z, w2c, w2g, dz, nullptr, E, nullptr,
            nullptr, nullptr, nullptr);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_gated_mlp_tail_bwd_idx_f32(const float* go, const int32_t* idx,
                                  const float* c, const float* g,
                                  const float* w, const float* z,
                                  const float* w2c, const float* w2g,
                                  float* dz, float* dw, int64_t E, int64_t d,
                                  uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (d != 64) {
        g_err = "gated_mlp_tail_bwd fused kernel is compiled for d=64";
        return -1;
    }
    if ((w == nullptr) != (dw == nullptr)) {
        g_err = "gated_mlp_tail_bwd: w and dw must be given together";
        return -1;
    }
    if (idx == nullptr) {
        g_err = "gated_mlp_tail_bwd_idx: idx must be given";
        return -1;
    }
    if (E <= 0) return 0;
    if (w)
        k_gated_mlp_tail_bwd<1, true><<<edge_mlp_blocks(E), BLOCK, 0, s>>>(
            go, idx, c, g, w, z, w2c, w2g, dz, dw, E, nullptr, nullptr, nullptr,
            nullptr);
    else
        k_gated_mlp_tail_bwd<0, true><<<edge_mlp_blocks(E), BLOCK, 0, s>>>(
            go, idx, c, g, nullptr, z, w2c, w2g, dz, nullptr, E, nullptr,
            nullptr, nullptr, nullptr);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_gated_mlp_tail_bwd_fw_f32(const float* go, const int32_t* idx,
                                 const float* c, const float* g,
                                 const float* bexp, const float* W,
                                 const float* mask, const float* z,
                                 const float* w2c, const float* w2g,
                                 float* dz, const float* dbexp_in,
                                 float* dbexp, int64_t E, int64_t d,
                                 int64_t n_rbf, uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (d != 64 || n_rbf != N_RBF) {
        g_err = "gated_mlp_tail_bwd_fw is compiled for d=64, n_rbf=9";
        return -1;
    }
    if (!bexp || !W || !dbexp) {
        g_err = "gated_mlp_tail_bwd_fw: bexp, W and dbexp must be given";
        return -1;
    }
    if (E <= 0) return 0;
    if (idx)
        k_gated_mlp_tail_bwd<2, true><<<mlp_tail_bwd_fw_blocks(E), BLOCK, 0, s>>>(
            go, idx, c, g, bexp, z, w2c, w2g, dz, nullptr, E, W, mask,
            dbexp_in, dbexp);
    else
        k_gated_mlp_tail_bwd<2, false><<<mlp_tail_bwd_fw_blocks(E), BLOCK, 0, s>>>(
            go, nullptr, c, g, bexp, z, w2c, w2g, dz, nullptr, E, W, mask,
            dbexp_in, dbexp);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_edge_mlp_bwd_f32(const float* dz, const float* WT, const float* gbase,
                        float* out, int64_t E, int64_t Din, int64_t Dout,
                        uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (Din != 128 || Dout != 64) {
        g_err = "edge_mlp_bwd fused kernel is compiled for Din=128, Dout=64";
        return -1;
    }
    if (E <= 0) return 0;
    if (gbase)
        k_edge_mlp_bwd<true><<<edge_mlp_blocks(E), BLOCK, 0, s>>>(
            dz, WT, gbase, out, E);
    else
        k_edge_mlp_bwd<false><<<edge_mlp_blocks(E), BLOCK, 0, s>>>(
            dz, WT, nullptr, out, E);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_gated_mlp_tail_fwd_f32(const float* h, const float* w2c,
                              const float* w2g, const float* b2c,
                              const float* b2g, const float* w,
                              const float* base, float* c_out, float* g_out,
                              float* out, int64_t E, int64_t d,
                              uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (d != 64) {
        g_err = "gated_mlp_tail_fwd fused kernel is compiled for d=64";
        return -1;
    }
    if ((c_out == nullptr) != (g_out == nullptr)) {
        g_err = "gated_mlp_tail_fwd: c_out and g_out must be given together";
        return -1;
    }
    if (E <= 0) return 0;
    if (c_out) {
        if (w) launch_mlp_tail_fwd<true, true>(h, w2c, w2g, b2c, b2g, w, base,
                                               c_out, g_out, out, E, s);
        else launch_mlp_tail_fwd<true, false>(h, w2c, w2g, b2c, b2g, nullptr,
                                              base, c_out, g_out, out, E, s);
    } else {
        if (w) launch_mlp_tail_fwd<false, true>(h, w2c, w2g, b2c, b2g, w, base,
                                                nullptr, nullptr, out, E, s);
        else launch_mlp_tail_fwd<false, false>(h, w2c, w2g, b2c, b2g, nullptr,
                                               base, nullptr, nullptr, out, E,
                                               s);
    }
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_gated_mlp_tail_fwd_fw_f32(const float* h, const float* w2c,
                                 const float* w2g, const float* b2c,
                                 const float* b2g, const float* bexp,
                                 const float* W, const float* mask,
                                 const float* base, float* c_out,
                                 float* g_out, float* out, int64_t E,
                                 int64_t d, int64_t n_rbf, uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (d != 64 || n_rbf != N_RBF) {
        g_err = "gated_mlp_tail_fwd_fw is compiled for d=64, n_rbf=9";
        return -1;
    }
    if ((c_out == nullptr) != (g_out == nullptr)) {
        g_err = "gated_mlp_tail_fwd_fw: c_out and g_out must be given together";
        return -1;
    }
    if (!bexp || !W) {
        g_err = "gated_mlp_tail_fwd_fw: bexp and W must be given";
        return -1;
    }
    if (E <= 0) return 0;
    if (c_out) launch_mlp_tail_fwd<true, 2>(h, w2c, w2g, b2c, b2g, bexp, base,
                                            c_out, g_out, out, E, s, W, mask);
    else launch_mlp_tail_fwd<false, 2>(h, w2c, w2g, b2c, b2g, bexp, base,
                                       nullptr, nullptr, out, E, s, W, mask);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_gated_mlp3_fw_f32(const float* erow, const float* WT, const float* bias,
                         const float* zs, const float* zd, const int32_t* src,
                         const int32_t* dst, const float* w2c,
                         const float* w2g, const float* b2c, const float* b2g,
                         const float* bexp, const float* W, const float* mask,
                         const float* base, float* z_out, float* c_out,
                         float* g_out, float* out, int64_t E, int64_t Din,
                         int64_t d, int64_t n_rbf, uint64_t stream) {
    if (n_rbf != N_RBF) {
        g_err = "gated_mlp3_fw is compiled for n_rbf=9";
        return -1;
    }
    if (!bexp || !W) {
        g_err = "gated_mlp3_fw: bexp and W must be given";
        return -1;
    }
    return gated_mlp_run<2>(erow, WT, bias, zs, zd, nullptr, src, dst, nullptr,
                            w2c, w2g, b2c, b2g, bexp, base, z_out, c_out,
                            g_out, out, E, Din, d, (hipStream_t)stream, W,
                            mask);
}

int dm_gated_mlp3_f32(const float* erow, const float* WT, const float* bias,
                      const float* zs, const float* zd, const int32_t* src,
                      const int32_t* dst, const float* w2c, const float* w2g,
                      const float* b2c, const float* b2g, const float* w,
                      const float* base, float* z_out, float* c_out,
                      float* g_out, float* out, int64_t E, int64_t Din,
                      int64_t d, uint64_t stream) {
    return gated_mlp_run<2>(erow, WT, bias, zs, zd, nullptr, src, dst, nullptr,
                            w2c, w2g, b2c, b2g, w, base, z_out, c_out, g_out,
                            out, E, Din, d, (hipStream_t)stream);
}

int dm_gated_mlp4_f32(const float* arow, const float* WT, const float* bias,
                      const float* z1, const float* z2, const float* zv,
                      const int32_t* lsrc, const int32_t* ldst,
                      const int32_t* center, const float* w2c,
                      const float* w2g, const float* b2c, const float* b2g,
                      const float* w, const float* base, float* z_out,
                      float* c_out, float* g_out, float* out, int64_t L,
                      int64_t Din, int64_t d, uint64_t stream) {
    return gated_mlp_run<3>(arow, WT, bias, z1, z2, zv, lsrc, ldst, center,
                            w2c, w2g, b2c, b2g, w, base, z_out, c_out, g_out,
                            out, L, Din, d, (hipStream_t)stream);
}

int dm_edge_geom_rbf_fwd_f32(const float* pos, const int32_t* src,
                             const int32_t* dst, const float* offshift,
                             const float* freqs, float cutoff, int32_t pexp,
                             int32_t nrbf, float* bv, float* bd,
                             float* exp_out, int64_t E, uint64_t stream) {
    if (nrbf > 16) { g_err = "nrbf > 16"; return -1; }
    hipStream_t s = (hipStream_t)stream;
    k_edge_geom_rbf_fwd<<<nblocks(E, BLOCK), BLOCK, 0, s>>>(
        pos, src, dst, offshift, freqs, cutoff, pexp, nrbf, bv, bd, exp_out, E);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_edge_geom_rbf_bwd_f32(const float* go_bv, const float* go_bd,
                             const float* go_exp, const float* bv,
                             const float* bd, const float* freqs,
                             float cutoff, int32_t pexp, int32_t nrbf,
                             float* gbv_total, int64_t E, uint64_t stream) {
    if (nrbf > 16) { g_err = "nrbf > 16"; return -1; }
    hipStream_t s = (hipStream_t)stream;
    k_edge_geom_rbf_bwd<<<nblocks(E, BLOCK), BLOCK, 0, s>>>(
        go_bv, go_bd, go_exp, bv, bd, freqs, cutoff, pexp, nrbf, gbv_total, E);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_rbf_env_fwd_f32(const float* d, const float* freqs, float cutoff,
                       int32_t pexp, int32_t nrbf, float* exp_out, int64_t M,
                       uint64_t stream) {
    if (nrbf > 16) { g_err = "nrbf > 16"; return -1; }
    hipStream_t s = (hipStream_t)stream;
    k_rbf_env_fwd<<<nblocks(M, BLOCK), BLOCK, 0, s>>>(
        d, freqs, cutoff, pexp, nrbf, exp_out, M);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_rbf_env_bwd_f32(const float* go_exp, const float* d, const float* freqs,
                       float cutoff, int32_t pexp, int32_t nrbf, float* gd,
                       int64_t M, uint64_t stream) {
    if (nrbf > 16) { g_err = "nrbf > 16"; return -1; }
    hipStream_t s = (hipStream_t)stream;
    k_rbf_env_bwd<<<nblocks(M, BLOCK), BLOCK, 0, s>>>(
        go_exp, d, freqs, cutoff, pexp, nrbf, gd, M);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_silu_bwd_f32(const float* go_h, const float* go_z, const float* z,
                    float* dz, int64_t total, uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    k_silu_bwd<<<nblocks(total, BLOCK), BLOCK, 0, s>>>(go_h, go_z, z, dz,
                                                       total);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_act_check_f32(int32_t which, uint32_t first_bits, uint64_t count,
                     uint32_t* bad_per_block, uint32_t* first_bad_bits,
                     uint64_t stream) {
    if ((which != 0 && which != 1) || !bad_per_block || !first_bad_bits ||
        count > (1ull << 32)) {
        g_err = "dm_act_check_f32: which must be 0 (sigmoid) or 1 (SiLU), "
                "count <= 2^32, outputs not NULL";
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    hipError_t e = hipMemsetAsync(first_bad_bits, 0xff, sizeof(uint32_t), s);
    if (e != hipSuccess) {
        g_err = hipGetErrorString(e);
        return (int)e;
    }
    if (which == 0)
        k_act_check<0><<<DM_ACT_CHECK_BLOCKS, BLOCK, 0, s>>>(
            first_bits, count, bad_per_block, first_bad_bits);
    else
        k_act_check<1><<<DM_ACT_CHECK_BLOCKS, BLOCK, 0, s>>>(
            first_bits, count, bad_per_block, first_bad_bits);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_act_eval_f32(int32_t which, int32_t impl, const float* x, int64_t n,
                    float* out, uint64_t stream) {
    if ((which != 0 && which != 1) || (impl != 0 && impl != 1)) {
        g_err = "dm_act_eval_f32: which and impl must be 0 or 1";
        return -1;
    }
    if (n <= 0) return 0;
    hipStream_t s = (hipStream_t)stream;
    const int nb = nblocks(n, BLOCK);
    switch (which * 2 + impl) {
    case 0: k_act_eval<0, 0><<<nb, BLOCK, 0, s>>>(x, n, out); break;
    case 1: k_act_eval<0, 1><<<nb, BLOCK, 0, s>>>(x, n, out); break;
    case 2: k_act_eval<1, 0><<<nb, BLOCK, 0, s>>>(x, n, out); break;
    default: k_act_eval<1, 1><<<nb, BLOCK, 0, s>>>(x, n, out); break;
    }
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_nl_count_f64(const double* pos, const int32_t* cid,
                    const int32_t* order, const int32_t* cell_start,
                    int32_t ncx, int32_t ncy, int32_t ncz,
                    double lx, double ly, double lz,
                    double r2tol, double tol, int32_t* cnt, int64_t N,
                    uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    k_nl<false><<<nblocks(N, BLOCK), BLOCK, 0, s>>>(
        pos, cid, order, cell_start, ncx, ncy, ncz, lx, ly, lz, r2tol, tol,
        0.0, nullptr, cnt, nullptr, nullptr, N);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_nl_fill_f64(const double* pos, const int32_t* cid,
                   const int32_t* order, const int32_t* cell_start,
                   int32_t ncx, int32_t ncy, int32_t ncz,
                   double lx, double ly, double lz,
                   double r2tol, double tol, double br2tol,
                   const int32_t* row_ptr, int32_t* src, int8_t* off_i8,
                   uint8_t* bond_flag, int64_t N, uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    k_nl<true><<<nblocks(N, BLOCK), BLOCK, 0, s>>>(
        pos, cid, order, cell_start, ncx, ncy, ncz, lx, ly, lz, r2tol, tol,
        br2tol, row_ptr, src, off_i8, bond_flag, N);
    DM_CHECK_LAUNCH();
    return 0;
}

// lattice9 / nc3 / R3 / pbc3 are HOST arrays; validated here so a bad plan
// is an error, never an out-of-range cell index on the device
static int nl_grid(const double* lattice9, const int32_t* nc3, const int32_t* R3,
            const int32_t* pbc3, int64_t N, NlGrid* g) {
    int64_t ncell = 1;
    for (int k = 0; k < 3; ++k) {
        if (nc3[k] < 1 || R3[k] < 0) { g_err = "nl_gen: bad grid"; return -1; }
        // image index |m| <= ceil(R/nc) must fit off_i8
        if (pbc3[k] && (R3[k] + nc3[k] - 1) / nc3[k] > 127) {
            g_err = "nl_gen: image index exceeds int8"; return -1;
        }
        g->nc[k] = nc3[k]; g->R[k] = R3[k]; g->per[k] = pbc3[k] ? 1 : 0;
        ncell *= nc3[k];
        if (ncell >= INT32_MAX) { g_err = "nl_gen: too many cells"; return -1; }
    }
    if (N >= INT32_MAX) { g_err = "nl_gen: N exceeds int32"; return -1; }
    for (int k = 0; k < 9; ++k) g->l[k] = lattice9[k];
    return 0;
}

int dm_nl_count_gen_f64(const double* pos, const int32_t* cid,
                        const int32_t* order, const int32_t* cell_start,
                        const double* lattice9, const int32_t* nc3,
                        const int32_t* R3, const int32_t* pbc3,
                        double r2tol, double tol, int32_t* cnt, int64_t N,
                        uint64_t stream) {
    NlGrid g;
    if (int rc = nl_grid(lattice9, nc3, R3, pbc3, N, &g)) return rc;
    hipStream_t s = (hipStream_t)stream;
    k_nl_gen<false><<<nblocks(N, BLOCK), BLOCK, 0, s>>>(
        pos, cid, order, cell_start, g, r2tol, tol, 0.0, nullptr, cnt,
        nullptr, nullptr, N);
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_nl_fill_gen_f64(const double* pos, const int32_t* cid,
                       const int32_t* order, const int32_t* cell_start,
                       const double* lattice9, const int32_t* nc3,
                       const int32_t* R3, const int32_t* pbc3,
                       double r2tol, double tol, double br2tol,
                       const int32_t* row_ptr, int32_t* src, int8_t* off_i8,
                       uint8_t* bond_flag, int64_t N, uint64_t stream) {
    NlGrid g;
    if (int rc = nl_grid(lattice9, nc3, R3, pbc3, N, &g)) return rc;
    hipStream_t s = (hipStream_t)stream;
    k_nl_gen<true><<<nblocks(N, BLOCK), BLOCK, 0, s>>>(
        pos, cid, order, cell_start, g, r2tol, tol, br2tol, row_ptr, src,
        off_i8, bond_flag, N);
    DM_CHECK_LAUNCH();
    return 0;
}


int dm_mace_tp_fwd_f32(const float* x0, const float* x1, const float* Y,
                       const float* w, const int32_t* nz, const float* nzc,
                       int32_t nnz, float* o0, float* o1, float* o2,
                       float* o3, int64_t E, int32_t C,
                       int32_t P, int32_t d1b, uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (C == 64)
        k_mace_tp_fwd<1><<<nblocks(E, 4), BLOCK, 0, s>>>(
            x0, x1, Y, w, nz, nzc, nnz, o0, o1, o2, o3, E, C, P, d1b);
    else if (C == 128)
        k_mace_tp_fwd<2><<<nblocks(E, 4), BLOCK, 0, s>>>(
            x0, x1, Y, w, nz, nzc, nnz, o0, o1, o2, o3, E, C, P, d1b);
    else { g_err = "dm_mace_tp: C must be 64 or 128"; return -1; }
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_mace_tp_bwd_f32(const float* g0, const float* g1, const float* g2,
                       const float* g3, const float* x0, const float* x1,
                       const float* Y, const float* w, const int32_t* nz,
                       const float* nzc, int32_t nnz, float* dx0,
                       float* dx1, float* dY, float* dw, int64_t E,
                       int32_t C, int32_t P, int32_t d1b, uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (C == 64)
        k_mace_tp_bwd<1><<<nblocks(E, 4), BLOCK, 0, s>>>(
            g0, g1, g2, g3, x0, x1, Y, w, nz, nzc, nnz, dx0, dx1, dY, dw,
            E, C, P, d1b);
    else if (C == 128)
        k_mace_tp_bwd<2><<<nblocks(E, 4), BLOCK, 0, s>>>(
            g0, g1, g2, g3, x0, x1, Y, w, nz, nzc, nnz, dx0, dx1, dY, dw,
            E, C, P, d1b);
    else { g_err = "dm_mace_tp: C must be 64 or 128"; return -1; }
    DM_CHECK_LAUNCH();
    return 0;
}


int dm_mace_symc_fwd_f32(const float* x, const int32_t* elem,
                         const float* W, const int32_t* nz,
                         const float* nzc, int32_t nnz, float* out,
                         int64_t N, int32_t C, int32_t T, int32_t S_out,
                         uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (S_out > 4) { g_err = "dm_mace_symc: S_out > 4"; return -1; }
    if (C == 64)
        k_mace_symc_fwd<1><<<nblocks(N, 4), BLOCK, 0, s>>>(
            x, elem, W, nz, nzc, nnz, out, N, C, T, S_out);
    else if (C == 128)
        k_mace_symc_fwd<2><<<nblocks(N, 4), BLOCK, 0, s>>>(
            x, elem, W, nz, nzc, nnz, out, N, C, T, S_out);
    else { g_err = "dm_mace_symc: C must be 64 or 128"; return -1; }
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_mace_symc_bwd_f32(const float* go, const float* x,
                         const int32_t* elem, const float* W,
                         const int32_t* nz, const float* nzc, int32_t nnz,
                         float* dx, int64_t N, int32_t C, int32_t T,
                         int32_t S_out, uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (S_out > 4) { g_err = "dm_mace_symc: S_out > 4"; return -1; }
    if (C == 64)
        k_mace_symc_bwd<1><<<nblocks(N, 4), BLOCK, 0, s>>>(
            go, x, elem, W, nz, nzc, nnz, dx, N, C, T, S_out);
    else if (C == 128)
        k_mace_symc_bwd<2><<<nblocks(N, 4), BLOCK, 0, s>>>(
            go, x, elem, W, nz, nzc, nnz, dx, N, C, T, S_out);
    else { g_err = "dm_mace_symc: C must be 64 or 128"; return -1; }
    DM_CHECK_LAUNCH();
    return 0;
}


int dm_rot_gather_f32(const float* h, const int32_t* idx, const float* D,
                      int32_t trans, float* out, int64_t E, int32_t C,
                      uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (C == 64)
        k_rot_gather<1><<<nblocks(E, 4), BLOCK, 0, s>>>(h, idx, D, trans,
                                                        out, E, C);
    else if (C == 128)
        k_rot_gather<2><<<nblocks(E, 4), BLOCK, 0, s>>>(h, idx, D, trans,
                                                        out, E, C);
    else { g_err = "dm_rot: C must be 64 or 128"; return -1; }
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_rot_scatter_f32(const float* mt, const float* D, int32_t trans,
                       const int32_t* perm, const int32_t* row_ptr,
                       const float* base, float* out, int64_t N,
                       int32_t C, uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (C == 64)
        k_rot_scatter<1><<<nblocks(N, 4), BLOCK, 0, s>>>(
            mt, D, trans, perm, row_ptr, base, out, N, C);
    else if (C == 128)
        k_rot_scatter<2><<<nblocks(N, 4), BLOCK, 0, s>>>(
            mt, D, trans, perm, row_ptr, base, out, N, C);
    else { g_err = "dm_rot: C must be 64 or 128"; return -1; }
    DM_CHECK_LAUNCH();
    return 0;
}

int dm_rot_dD_f32(const float* go, const float* h, const int32_t* idx,
                  int32_t trans, float* dD, int64_t E, int32_t C,
                  uint64_t stream) {
    hipStream_t s = (hipStream_t)stream;
    if (C == 64)
        k_rot_dD<1><<<nblocks(E, 4), BLOCK, 0, s>>>(go, h, idx, trans, dD,
                                                    E, C);
    else if (C == 128)
        k_rot_dD<2><<<nblocks(E, 4), BLOCK, 0, s>>>(go, h, idx, trans, dD,
                                                    E, C);
    else { g_err = "dm_rot: C must be 64 or 128"; return -1; }
    DM_CHECK_LAUNCH();
    return 0;
}

const char* dm_hip_last_error(void) { return g_err.c_str(); }

}  // extern "C"
