// so2.hip — gfx950 (CDNA4) kernels for the eSCN/UMA SO(2) convolution in the
// z-aligned edge frame (distmlip_amd/uma_ops.py so2_conv), lmax = 2,
// C in {64, 128}, bf16 operands on v_mfma_f32_32x32x16_bf16 with fp32
// accumulation:
//
//   k_so2<C, false>   mt[e] = gate_m . (W_m x_m[e]),  x = xs || xd
//   k_so2<C, true>    u = W_m^T bf16(go_m);  dxs, dxd = gate_m . u;
//                     dgate[e, m] = sum u . bf16(x)
//
// x, go and the weights are rounded to bf16 (round to nearest even, the
// rounding of torch's .bfloat16()); every product is accumulated in fp32 and
// the gate is applied in fp32 in the epilogue.  Rows per m (uma_model
// m_indices(2)): m=0 {0,2,6}; m=1 plus {3,7} minus {1,5}; m=2 plus {8}
// minus {4}.  For m > 0, with Br = Wr^T, Bi = Wi^T as [K, N],
//     op = xp.Br - xm.Bi,   om = xp.Bi + xm.Br:
// two A fragments (xp, xm) and two B fragments (Br, Bi) feed four MFMAs; the
// minus is a packed sign-bit flip of the xm fragment.  The reverse is the
// same form over go with Br' = Wr, Bi' = -Wi restricted to one side's input
// columns (the negation is exact in bf16 and done at pack time).
//
// Work split.  A block of 256 threads owns T = 64 edges and walks the three
// m-groups.  Within a group the accumulators of the block cover the group's
// whole output width (3C, 4C, 2C forward), so every x element is fetched
// from HBM and converted once and every output is stored once.  Wave w owns
// the 32-channel slice wn = w % (C/32) of EVERY output row of the group, and
// (C = 64 only) the 32-edge half wm = w / 2; at C = 128 a wave covers all 64
// edges as two M tiles.  The m=1 group is the largest: 8 accumulator tiles
// of 16 registers = 128 per lane at C = 128.  Accumulator layout of a tile:
// lane holds channel lane%32, register r holds edge (r&3) + 8(r>>2) +
// 4(lane>>5): a store of one register is two 128-byte rows.
//
// A operand.  K is walked in stages of one (row, side) slab of KC = 64
// channels: all threads load the stage's fp32 x as float4 (both parts for
// m > 0), round to bf16 and write it to LDS as [part][edge][64] with rows
// padded to 144 bytes (conflict-free 16-byte fragment reads: lane%32 = edge,
// k = 8(lane>>5) + 0..7).  Two LDS buffers; the loads of stage n+1 are issued
// into registers before the MFMAs of stage n, so one barrier per stage.
//
// B operand.  The host packs each group's [K, N] matrices in fragment order
// [kstep][r|i][ntile][lane][8 bf16]: one B fragment is a 1 KB contiguous
// 16-byte-per-lane load.  DEVIATION from streaming the weights through LDS:
// with the split above a wave's B fragments (its own channel slice) are used
// by no other wave of the block at C = 128 (by one other at C = 64), so
// staging them in LDS would add a write, a barrier and a read to every
// fragment without saving an L2 read; they are loaded from L2 straight into
// registers instead.  The block reads the whole pack once per tile (38 C^2
// bf16 = 1.24 MB at C = 128, L2 resident), 19 KB per edge beside the 13.8 KB
// per edge of HBM traffic.
//
// Reverse.  The output width doubles (both sides), so it runs per side:
// blockIdx.y picks the side, each block has the accumulator budget of the
// forward, and the go tile is read once per side.
// dgate follows from <go, W x> = <W^T go, x>: in the epilogue each lane
// multiplies u by bf16(x) read in the accumulator layout, sums over its
// tiles, then a fixed-order reduction: xor-shuffles over the 32 lanes of a
// half wave, one LDS slot per (channel slice, edge), and thread e sums the
// slots in slice order.  The two sides leave one partial each, [2, E, 3],
// which the caller adds.  No atomics.
//
// Tail tiles feed zeros to the MFMA for rows >= E and predicate every global
// access on row < E.  Row offsets are 64-bit (E.9.C exceeds 2^31 at scale).
//
// Resources (hipcc -O3 --offload-arch=gfx950,
// -Rpass-analysis=kernel-resource-usage), 37,888 B LDS per block, occupancy
// 2 waves per SIMD (__launch_bounds__(256, 2): 256 registers) for all four:
//   k_so2<64,  fwd>   192 VGPR, no spill
//   k_so2<128, fwd>   256 VGPR, no VGPR spill (2 SGPRs spilled to a VGPR)
//   k_so2<64,  bwd>   204 VGPR, no spill
//   k_so2<128, bwd>   256 VGPR, 3 VGPRs spilled (16 B of scratch per lane:
//                     kernel-long values stored once at entry and reloaded
//                     in the epilogue, not in the MFMA loop), 9 SGPRs
// The k-step loop is unrolled by two, not four: the full unroll hoists the B
// loads of all four steps and spills tens of registers at C = 128.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/distmlip_hip.h"

void dm_set_last_error(const char* msg);      // kernels.hip

namespace {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

constexpr int BLOCK = 256;
constexpr int T = 64;                 // edges per block
constexpr int KC = 64;                // channels per stage
constexpr int LDA = KC * 2 + 16;      // bytes per LDS row (padded)
constexpr int PART = T * LDA;         // bytes per part of a stage
constexpr int NLD = T * (KC / 4) / BLOCK;   // float4 per thread, part, stage

__device__ __forceinline__ uint32_t pack2(float a, float b) {
    bf16x2 v = {(__bf16)a, (__bf16)b};
    return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ float round_bf16(float a) {
    return (float)(__bf16)a;
}

// elements of the packed image of group M with NSLAB K-slabs of C
template <int C>
constexpr int64_t pack_elems(int M, bool bwd) {
    const int nl = 3 - M;
    return (int64_t)(bwd ? nl : 2 * nl) * C * nl * C * (M == 0 ? 1 : 2);
}
template <int C>
constexpr int64_t pack_offset(int M, bool bwd) {
    int64_t o = 0;
    for (int m = 0; m < M; ++m) o += pack_elems<C>(m, bwd);
    return o;
}

struct Smem {
    unsigned char a[2][2][PART];      // [buffer][part][edge][LDA]
    float red[4][T];                  // dgate partials per channel slice
};

// One m-group of one 64-edge tile.  Every pointer is already advanced to the
// tile's first edge (64-bit, uniform), so the per-lane offsets are 32-bit;
// nv = the number of valid edges of the tile.  a0/a1: the A sources by side
// (forward xs, xd; reverse go, go).  wp: the group's packed B image.  out: forward mt,
// reverse dx of this side.  xside, dgate: reverse only, this side's x and
// its dgate partial.
template <int C, bool BWD, int M>
__device__ __forceinline__ void so2_group(
        const float* __restrict__ a0, const float* __restrict__ a1,
        const u32x4* __restrict__ wp, const float* __restrict__ gate,
        float* __restrict__ out, const float* __restrict__ xside,
        float* __restrict__ dgate, int nv, Smem& sm) {
    constexpr int WN = C / 32, WM = 4 / WN, MT = 2 / WM;
    constexpr int NL = 3 - M, NP = M == 0 ? 1 : 2;
    constexpr int NSLAB = BWD ? NL : 2 * NL;
    constexpr int HPS = C / KC;                  // stages per slab
    constexpr int NSTAGE = NSLAB * HPS;
    constexpr int NT = NL * WN;                  // 32-wide tiles of N

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int wn = w % WN, wm = w / WN;
    const int lc = lane & 31, lh = lane >> 5;
    const int sc4 = tid & 15, se = tid >> 4;     // staging: float4 col, edge

    f32x16 acc[MT][NP][NL];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int j = 0; j < NL; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[mt][p][j][r] = 0.0f;

    float4 st[NP][NLD];
    auto load_stage = [&](int n) {
        const int q = n / HPS, h = n - q * HPS;
        const int j = BWD ? q : q >> 1;
        const float* __restrict__ src = (!BWD && (q & 1)) ? a1 : a0;
        const int l = M + j;
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int row = l * l + l + (p ? -M : M);
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                const int e = se + 16 * i;
                st[p][i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (e < nv)
                    st[p][i] = *(const float4*)(src + (e * 9 + row) * C +
                                                h * KC + sc4 * 4);
            }
        }
    };
    auto write_stage = [&](int buf) {
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int i = 0; i < NLD; ++i) {
                u32x2 v = {pack2(st[p][i].x, st[p][i].y),
                           pack2(st[p][i].z, st[p][i].w)};
                *(u32x2*)(sm.a[buf][p] + (se + 16 * i) * LDA + sc4 * 8) = v;
            }
    };

    load_stage(0);
    write_stage(0);
    __syncthreads();
#pragma unroll 1
    for (int n = 0; n < NSTAGE; ++n) {
        const int buf = n & 1;
        if (n + 1 < NSTAGE) load_stage(n + 1);
#pragma unroll 2
        for (int ks = 0; ks < KC / 16; ++ks) {
            const int kstep = n * (KC / 16) + ks;
            u32x4 b[NP][NL];
#pragma unroll
            for (int ri = 0; ri < NP; ++ri)
#pragma unroll
                for (int j = 0; j < NL; ++j)
                    b[ri][j] = wp[((kstep * NP + ri) * NT + j * WN + wn) * 64 +
                                  lane];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                const int el = wm * (WM == 2 ? 32 : 0) + mt * 32 + lc;
                const int ao = el * LDA + ks * 32 + lh * 16;
                const u32x4 ap = *(const u32x4*)(sm.a[buf][0] + ao);
                if constexpr (M == 0) {
#pragma unroll
                    for (int j = 0; j < NL; ++j)
                        acc[mt][0][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                            __builtin_bit_cast(bf16x8, ap),
                            __builtin_bit_cast(bf16x8, b[0][j]),
                            acc[mt][0][j], 0, 0, 0);
                } else {
                    const u32x4 am = *(const u32x4*)(sm.a[buf][1] + ao);
                    const u32x4 an = am ^ 0x80008000u;      // -xm, packed
#pragma unroll
                    for (int j = 0; j < NL; ++j) {
                        const bf16x8 br = __builtin_bit_cast(bf16x8, b[0][j]);
                        const bf16x8 bi = __builtin_bit_cast(bf16x8, b[NP - 1][j]);
                        acc[mt][0][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                            __builtin_bit_cast(bf16x8, ap), br, acc[mt][0][j],
                            0, 0, 0);
                        acc[mt][NP - 1][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                            __builtin_bit_cast(bf16x8, ap), bi,
                            acc[mt][NP - 1][j], 0, 0, 0);
                        acc[mt][0][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                            __builtin_bit_cast(bf16x8, an), bi, acc[mt][0][j],
                            0, 0, 0);
                        acc[mt][NP - 1][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                            __builtin_bit_cast(bf16x8, am), br,
                            acc[mt][NP - 1][j], 0, 0, 0);
                    }
                }
            }
        }
        if (n + 1 < NSTAGE) write_stage(buf ^ 1);
        __syncthreads();
    }

    // epilogue: gate in fp32; reverse also u . bf16(x) for dgate.  One
    // accumulator tile at a time (16 loads in flight), so the x loads of the
    // whole group are not hoisted into registers at once.
    const int ch = wn * 32 + lc;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int elb = wm * (WM == 2 ? 32 : 0) + mt * 32 + 4 * lh;
        float dg[16], g[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int e = elb + (r & 3) + 8 * (r >> 2);
            // reverse: registers are short, the gate is re-read per tile
            g[r] = (!BWD && e < nv) ? gate[e * 3 + M] : 0.0f;
            dg[r] = 0.0f;
        }
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                const int l = M + j;
                const int row = l * l + l + (p ? -M : M);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (BWD) {
#pragma unroll
                    for (int rb = 0; rb < 16; rb += 8) {
                        float xv[8];
#pragma unroll
                        for (int t = 0; t < 8; ++t) {
                            const int r = rb + t;
                            const int e = elb + (r & 3) + 8 * (r >> 2);
                            xv[t] = e < nv ? xside[(e * 9 + row) * C + ch]
                                           : 0.0f;
                        }
#pragma unroll
                        for (int t = 0; t < 8; ++t)
                            dg[rb + t] += acc[mt][p][j][rb + t] *
                                          round_bf16(xv[t]);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int e = elb + (r & 3) + 8 * (r >> 2);
                    if (e < nv)
                        out[(e * 9 + row) * C + ch] =
                            (BWD ? gate[e * 3 + M] : g[r]) * acc[mt][p][j][r];
                }
            }
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (BWD) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
#pragma unroll
                for (int s = 16; s >= 1; s >>= 1)
                    dg[r] += __shfl_xor(dg[r], s, 64);
                if (lc == 0)
                    sm.red[wn][wm * (WM == 2 ? 32 : 0) + mt * 32 + (r & 3) +
                               8 * (r >> 2) + 4 * lh] = dg[r];
            }
        }
    }
    if constexpr (BWD) {
        __syncthreads();
        if (tid < nv) {
            float d = 0.0f;
#pragma unroll
            for (int s = 0; s < WN; ++s) d += sm.red[s][tid];
            dgate[tid * 3 + M] = d;
        }
        __syncthreads();
    }
}

template <int C, bool BWD>
__global__ void __launch_bounds__(BLOCK, 2)
k_so2(const float* __restrict__ xs, const float* __restrict__ xd,
      const float* __restrict__ go, const float* __restrict__ gate,
      const uint16_t* __restrict__ wpack, float* __restrict__ o0,
      float* __restrict__ o1, float* __restrict__ dgate, int64_t E) {
    __shared__ __attribute__((aligned(16))) Smem sm;
    const int64_t e0 = (int64_t)blockIdx.x * T;
    const int nv = E - e0 < T ? (int)(E - e0) : T;
    const int64_t xo = e0 * 9 * C;            // 64-bit: E.9.C exceeds 2^31
    gate += e0 * 3;
    if constexpr (!BWD) {
        so2_group<C, false, 0>(xs + xo, xd + xo,
            (const u32x4*)(wpack + pack_offset<C>(0, false)), gate, o0 + xo,
            nullptr, nullptr, nv, sm);
        so2_group<C, false, 1>(xs + xo, xd + xo,
            (const u32x4*)(wpack + pack_offset<C>(1, false)), gate, o0 + xo,
            nullptr, nullptr, nv, sm);
        so2_group<C, false, 2>(xs + xo, xd + xo,
            (const u32x4*)(wpack + pack_offset<C>(2, false)), gate, o0 + xo,
            nullptr, nullptr, nv, sm);
    } else {
        // one side per block (blockIdx.y): the accumulator budget of the
        // forward; dgate leaves as one partial per side, [2, E, 3]
        const int side = blockIdx.y;
        go += xo;
        dgate += ((int64_t)side * E + e0) * 3;
        const float* __restrict__ x = (side ? xd : xs) + xo;
        float* __restrict__ dx = (side ? o1 : o0) + xo;
        const uint16_t* __restrict__ ws =
            wpack + side * pack_offset<C>(3, true);
        so2_group<C, true, 0>(go, go,
            (const u32x4*)(ws + pack_offset<C>(0, true)), gate, dx, x, dgate,
            nv, sm);
        so2_group<C, true, 1>(go, go,
            (const u32x4*)(ws + pack_offset<C>(1, true)), gate, dx, x, dgate,
            nv, sm);
        so2_group<C, true, 2>(go, go,
            (const u32x4*)(ws + pack_offset<C>(2, true)), gate, dx, x, dgate,
            nv, sm);
    }
}

template <bool BWD>
int launch_so2(const float* xs, const float* xd, const float* go,
               const float* gate, const uint16_t* wpack, float* o0, float* o1,
               float* dgate, int64_t E, int32_t C, hipStream_t s) {
    if (C != 64 && C != 128) {
        dm_set_last_error("dm_so2_conv: C must be 64 or 128");
        return -1;
    }
    if (E <= 0) return 0;
    const int64_t nb = (E + T - 1) / T;
    if (nb > INT32_MAX) {
        dm_set_last_error("dm_so2_conv: too many edges for one launch");
        return -1;
    }
    if (((uintptr_t)xs | (uintptr_t)xd | (uintptr_t)go | (uintptr_t)wpack) &
        15) {
        dm_set_last_error("dm_so2_conv: pointers must be 16-byte aligned");
        return -1;
    }
    const dim3 grid((unsigned)nb, BWD ? 2 : 1);
    if (C == 64)
        k_so2<64, BWD><<<grid, BLOCK, 0, s>>>(xs, xd, go, gate, wpack, o0,
                                                  o1, dgate, E);
    else
        k_so2<128, BWD><<<grid, BLOCK, 0, s>>>(xs, xd, go, gate, wpack, o0,
                                                   o1, dgate, E);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dm_set_last_error(hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

}  // namespace

extern "C" {

int dm_so2_conv_fwd_bf16(const float* xs, const float* xd, const float* gate,
                         const uint16_t* wpack, float* mt, int64_t E,
                         int32_t C, uint64_t stream) {
    return launch_so2<false>(xs, xd, nullptr, gate, wpack, mt, nullptr,
                             nullptr, E, C, (hipStream_t)stream);
}

int dm_so2_conv_bwd_bf16(const float* go, const float* xs, const float* xd,
                         const float* gate, const uint16_t* wpack_t,
                         float* dxs, float* dxd, float* dgate2, int64_t E,
                         int32_t C, uint64_t stream) {
    return launch_so2<true>(xs, xd, go, gate, wpack_t, dxs, dxd, dgate2, E, C,
                            (hipStream_t)stream);
}

}  // extern "C"
