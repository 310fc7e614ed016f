// mace_conv.hip — gfx950 (CDNA4) kernels for the MACE interaction's
// convolution: gather, uvu tensor product and dst sum in one pass.
//
//     M[i, o3+k3, c] = sum_{e -> i} sum_p w[e,p,c] * sum_{k1}
//                      x[src[e], o1+k1, c] * yc[e, (p,k1,k3)]
//     yc[e, t]       = sum_k2 K[t, k2] * Y[e, k2]
//
// over the paths p = (l1, l2, l3) of the interaction, with K [T,16] the
// coupling rows the caller builds: row t = (p, k1, k3) holds CG_p[k1, :, k3]
// at the columns of p's l2 block.  Written op by op this is a gather to
// [E, R, C], a per-edge product that writes sixteen rows of C floats per
// edge, and four segment sums that read them back.  The kernels here form
// no per-edge array but their inputs (Y, w) and outputs (dY, dw).
//
// Layouts: node rows l-major, xs [N, R, C] (row 0 is l = 0, rows 1..3 the
// l = 1 components; R = 1 or 4), M and G [N, 16, C] with row l3*l3 + m3,
// w [E, P, C], Y [E, 16].
//
// Mapping: one wave per (node, 64-channel block), lane = channel, as in
// tensornet.hip.  Every global access of a wave is one coalesced 256 B row;
// edge and node indices are wave-uniform.  The node's accumulators live in
// registers and its CSR row is walked in order: no atomics, and every
// launch gives the same bits.
//
// Static structure.  l_max = 3 leaves two path lists, the 4 paths of an
// l = 0 sender (T = 16) and the 10 paths of an l = 0, 1 sender (T = 88).
// The kernels are templated on which one applies, so (p, k1, k3) of every t
// is a compile-time constant and every accumulator a fixed register; only
// the CG values are run-time data.  Lane j owns the K rows
// t = rev6(j) and rev6(j) + 64, kept in LDS for the block (rev6 = the six lane bits
// reversed, the order the wave reduction below ends in).  Per edge these two
// lanes' dot products with Y[e] (scalar loads) give yc[t], which goes to the
// wave's own LDS stripe; all lanes read the stripe back as broadcast
// ds_read_b128s and run the unrolled products.  A stripe belongs to one
// wave, so the grid-stride loop has no block barrier.
//
// Reverse, dst CSR (bwd_edge): G[n] stays in registers for the row; per edge
//     dw[e,p,c] = sum_{k1,k3} yc[t] x[k1] g[k3]
//     D[t]      = sum_c w[p] x[k1] g[k3]          (a sum over channels)
//     dY[e,k2]  = sum_t K[t,k2] D[t]
// The T channel sums are taken together: a butterfly in which each step
// halves the number of values a lane holds (lane pairs split the values
// between them, one shuffle and one add per value pair), so T sums cost
// about T shuffles, not 6 T, and D[t] ends in the lane that holds K row t.
// The sixteen dY terms go through the same butterfly.  With C > 64 each
// channel block writes its own [E,16] slice of dYp and the caller adds them.
//
// Reverse, src CSR (bwd_node): for node s and its out-edges e = src_perm[j]
//     dxs[s,k1,c] = sum_e sum_{p,k3} w[e,p,c] yc[e,t] G[dst[e],k3,c]

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <type_traits>

#include "../../include/distmlip_hip.h"

void dm_set_last_error(const char* msg);      // kernels.hip

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int MAX_BLOCKS = 8192;

inline int nblocks(int64_t work, int64_t per_block) {
    int64_t b = (work + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b));
}

// The path list of a sender with l = 0..LS and its flat index t = (p, k1, k3)
// (path-major, then k1, then k3): the order of mace_model.tp_paths and of the
// caller's K rows.
struct PathTab {
    int P, T;
    int l1[10], l2[10], l3[10];
    int tp[88], tk1[88], tk3[88];
};

constexpr PathTab make_tab(int ls) {
    PathTab t{};
    int n = 0, nt = 0;
    for (int l1 = 0; l1 <= ls; ++l1)
        for (int l2 = 0; l2 <= 3; ++l2)
            for (int l3 = 0; l3 <= 3; ++l3) {
                const int lo = l1 > l2 ? l1 - l2 : l2 - l1;
                if ((l1 + l2 + l3) % 2 != 0 || l3 < lo || l3 > l1 + l2)
                    continue;
                t.l1[n] = l1; t.l2[n] = l2; t.l3[n] = l3;
                for (int k1 = 0; k1 < 2 * l1 + 1; ++k1)
                    for (int k3 = 0; k3 < 2 * l3 + 1; ++k3) {
                        t.tp[nt] = n; t.tk1[nt] = k1; t.tk3[nt] = k3;
                        ++nt;
                    }
                ++n;
            }
    t.P = n; t.T = nt;
    return t;
}

template <int LS> inline constexpr PathTab TAB = make_tab(LS);
static_assert(TAB<0>.P == 4 && TAB<0>.T == 16, "l = 0 sender");
static_assert(TAB<1>.P == 10 && TAB<1>.T == 88, "l = 0, 1 sender");

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) {
        f(std::integral_constant<int, I>{});
        static_for<I + 1, N>(f);
    }
}

// LDS traffic of one wave is executed in order; this keeps the compiler from
// moving a stripe's reads across its writes.
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The K rows of a lane, t = rev6(lane) and rev6(lane) + 64, kept in LDS for
// the block (row lane and row 64 + lane, zero where t >= T).  Rows are 20
// floats apart, so the b128 reads of sixteen neighbouring lanes fall on
// sixteen different bank quads.
template <int LS>
struct KRows {
    static constexpr int T = TAB<LS>.T;
    static constexpr int NS = T > 64 ? 2 : 1;
    static constexpr int KS = 20;
    static constexpr int FLOATS = NS * 64 * KS;
    const float4* row;
    int t0;

    // every thread of the block calls this once, before the work loop
    __device__ __forceinline__ void init(float* kl,
                                         const float* __restrict__ K,
                                         int lane) {
        for (int i = threadIdx.x; i < NS * 64 * 16; i += BLOCK) {
            const int j = i >> 4, k = i & 15;
            const int t = (int)(__brev((unsigned)(j & 63)) >> 26) + (j & 64);
            kl[j * KS + k] = t < T ? K[t * 16 + k] : 0.0f;
        }
        __syncthreads();
        t0 = (int)(__brev((unsigned)lane) >> 26);
        row = reinterpret_cast<const float4*>(kl + lane * KS);
    }

    __device__ __forceinline__ void get(float (&a)[16], int slot) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 v = row[slot * (64 * KS / 4) + i];
            a[4 * i] = v.x; a[4 * i + 1] = v.y;
            a[4 * i + 2] = v.z; a[4 * i + 3] = v.w;
        }
    }

    // yc[t] = K[t,:] . Y[e,:] into the wave's stripe
    __device__ __forceinline__ void put_yc(float* stripe,
                                           const float* __restrict__ y) const {
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            float a[16], acc = 0.0f;
            get(a, s);
#pragma unroll
            for (int k = 0; k < 16; ++k) acc = fmaf(a[k], y[k], acc);
            if (t0 + 64 * s < T) stripe[t0 + 64 * s] = acc;
        }
    }
};

// acc[o3+k3] += (w[p] * x[o1+k1]) * yc[t] over all t, yc from the stripe
template <int LS>
__device__ __forceinline__ void conv_accum(
        float (&acc)[16], const float (&x)[LS ? 4 : 1],
        const float (&w)[TAB<LS>.P], const float* stripe) {
    constexpr int P = TAB<LS>.P, T = TAB<LS>.T;
    float wx[P][3];
    static_for<0, P>([&](auto pc) {
        constexpr int p = decltype(pc)::value;
        constexpr int l1 = TAB<LS>.l1[p];
#pragma unroll
        for (int k1 = 0; k1 < 2 * l1 + 1; ++k1)
            wx[p][k1] = w[p] * x[l1 * l1 + k1];
    });
    const float4* s4 = reinterpret_cast<const float4*>(stripe);
    static_for<0, T / 4>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const float4 v4 = s4[i];
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
        static_for<0, 4>([&](auto jc) {
            constexpr int t = 4 * i + decltype(jc)::value;
            constexpr int p = TAB<LS>.tp[t];
            constexpr int l3 = TAB<LS>.l3[p];
            constexpr int r = l3 * l3 + TAB<LS>.tk3[t];
            acc[r] = fmaf(wx[p][TAB<LS>.tk1[t]], v[t & 3], acc[r]);
        });
    });
}

// dx[o1+k1] += (w[p] * g[o3+k3]) * yc[t] over all t
template <int LS>
__device__ __forceinline__ void conv_accum_t(
        float (&dx)[LS ? 4 : 1], const float (&g)[16],
        const float (&w)[TAB<LS>.P], const float* stripe) {
    constexpr int P = TAB<LS>.P, T = TAB<LS>.T;
    float wg[P][7];
    static_for<0, P>([&](auto pc) {
        constexpr int p = decltype(pc)::value;
        constexpr int l3 = TAB<LS>.l3[p];
#pragma unroll
        for (int k3 = 0; k3 < 2 * l3 + 1; ++k3)
            wg[p][k3] = w[p] * g[l3 * l3 + k3];
    });
    const float4* s4 = reinterpret_cast<const float4*>(stripe);
    static_for<0, T / 4>([&](auto ic) {
        constexpr int i = decltype(ic)::value;
        const float4 v4 = s4[i];
        const float v[4] = {v4.x, v4.y, v4.z, v4.w};
        static_for<0, 4>([&](auto jc) {
            constexpr int t = 4 * i + decltype(jc)::value;
            constexpr int p = TAB<LS>.tp[t];
            constexpr int l1 = TAB<LS>.l1[p];
            constexpr int r = l1 * l1 + TAB<LS>.tk1[t];
            dx[r] = fmaf(wg[p][TAB<LS>.tk3[t]], v[t & 3], dx[r]);
        });
    });
}

// out[n,:,c] over the CSR row of n, e = PERM ? perm[p] : p:
//   forward (TR = false): out = M [N,16,C], A = xs, idx = src, the dst CSR
//   reverse (TR = true):  out = dxs [N,R,C], A = G, idx = dst, the src CSR
template <int LS, bool TR, int UNROLL>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(4)))
void k_mace_conv(
        const float* __restrict__ A, const float* __restrict__ tp_w,
        const float* __restrict__ Y, const float* __restrict__ K,
        const int32_t* __restrict__ idx, const int32_t* __restrict__ perm,
        const int32_t* __restrict__ row_ptr, float* __restrict__ out,
        int64_t N, int32_t C) {
    constexpr int P = TAB<LS>.P, T = TAB<LS>.T, R = LS ? 4 : 1;
    constexpr int RA = TR ? 16 : R;      // rows read per edge
    constexpr int RO = TR ? R : 16;      // rows written per node
    __shared__ __attribute__((aligned(16))) float lds[WAVES][UNROLL][T];
    __shared__ __attribute__((aligned(16))) float kl[KRows<LS>::FLOATS];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    KRows<LS> kr;
    kr.init(kl, K, lane);
    const int32_t CB = C >> 6;
    const int64_t work = N * CB;
    const int64_t CA = RA * (int64_t)C, CP = P * (int64_t)C;
    for (int64_t wk = (int64_t)blockIdx.x * WAVES + wid; wk < work;
         wk += (int64_t)gridDim.x * WAVES) {
        const int64_t n = wk / CB;
        const int32_t c = (int32_t)(wk - n * CB) * 64 + lane;
        const int32_t p0 = row_ptr[n], p1 = row_ptr[n + 1];
        float acc[RO];
#pragma unroll
        for (int r = 0; r < RO; ++r) acc[r] = 0.0f;
        int32_t p = p0;
        for (; p + UNROLL <= p1; p += UNROLL) {
            float a[UNROLL][RA], w[UNROLL][P];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int32_t e = TR ? perm[p + u] : p + u;
                const float* ap = A + (int64_t)idx[e] * CA + c;
                const float* wp = tp_w + (int64_t)e * CP + c;
#pragma unroll
                for (int k = 0; k < P; ++k) w[u][k] = wp[(int64_t)k * C];
#pragma unroll
                for (int r = 0; r < RA; ++r) a[u][r] = ap[(int64_t)r * C];
                kr.put_yc(lds[wid][u], Y + (int64_t)e * 16);
            }
            wave_lds_sync();
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                if constexpr (TR)
                    conv_accum_t<LS>(acc, a[u], w[u], lds[wid][u]);
                else
                    conv_accum<LS>(acc, a[u], w[u], lds[wid][u]);
            }
            wave_lds_sync();
        }
        for (; p < p1; ++p) {
            float a[RA], w[P];
            const int32_t e = TR ? perm[p] : p;
            const float* ap = A + (int64_t)idx[e] * CA + c;
            const float* wp = tp_w + (int64_t)e * CP + c;
#pragma unroll
            for (int k = 0; k < P; ++k) w[k] = wp[(int64_t)k * C];
#pragma unroll
            for (int r = 0; r < RA; ++r) a[r] = ap[(int64_t)r * C];
            kr.put_yc(lds[wid][0], Y + (int64_t)e * 16);
            wave_lds_sync();
            if constexpr (TR)
                conv_accum_t<LS>(acc, a, w, lds[wid][0]);
            else
                conv_accum<LS>(acc, a, w, lds[wid][0]);
            wave_lds_sync();
        }
        float* op = out + n * (RO * (int64_t)C) + c;
#pragma unroll
        for (int r = 0; r < RO; ++r) op[(int64_t)r * C] = acc[r];
    }
}

// One butterfly step on a value pair: the lane whose MASK bit is clear keeps
// x, the other keeps y, and each adds its partner's copy of what it keeps.
__device__ __forceinline__ float bfly_pair(float x, float y, int mask,
                                           bool hi) {
    const float keep = hi ? y : x, send = hi ? x : y;
    return keep + __shfl_xor(send, mask, 64);
}

// The remaining steps MASK, MASK/2, .., 1 on v[0..NV): each halves NV
// (an odd count is padded with a zero) until one value is left, which the
// last steps sum plainly.  With all six steps halving, lane j ends with the
// wave sums of the values rev6(j) + 64 s in v[s].
template <int NV, int MASK, int NMAX>
__device__ __forceinline__ void bfly_rest(float (&v)[NMAX], int lane) {
    if constexpr (MASK >= 1) {
        if constexpr (NV > 1) {
            constexpr int H = (NV + 1) / 2;
            const bool hi = (lane & MASK) != 0;
#pragma unroll
            for (int i = 0; i < H; ++i)
                v[i] = bfly_pair(v[2 * i],
                                 2 * i + 1 < NV ? v[2 * i + 1] : 0.0f,
                                 MASK, hi);
            bfly_rest<H, MASK / 2>(v, lane);
        } else {
            v[0] += __shfl_xor(v[0], MASK, 64);
            bfly_rest<1, MASK / 2>(v, lane);
        }
    }
}

template <int LS>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(4)))
void k_mace_conv_bwd_edge(
        const float* __restrict__ G, const float* __restrict__ xs,
        const float* __restrict__ tp_w, const float* __restrict__ Y,
        const float* __restrict__ K, const int32_t* __restrict__ src,
        const int32_t* __restrict__ row_ptr, float* __restrict__ dw,
        float* __restrict__ dYp, int64_t N, int64_t E, int32_t C) {
    constexpr int P = TAB<LS>.P, T = TAB<LS>.T, R = LS ? 4 : 1;
    constexpr int T8 = T / 8;
    __shared__ __attribute__((aligned(16))) float lds[WAVES][T];
    __shared__ __attribute__((aligned(16))) float kl[KRows<LS>::FLOATS];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const bool b5 = (lane & 32) != 0, b4 = (lane & 16) != 0,
               b3 = (lane & 8) != 0;
    KRows<LS> kr;
    kr.init(kl, K, lane);
    const int32_t CB = C >> 6;
    const int64_t work = N * CB;
    const int64_t C16 = 16 * (int64_t)C, CR = R * (int64_t)C,
                  CP = P * (int64_t)C;
    for (int64_t wk = (int64_t)blockIdx.x * WAVES + wid; wk < work;
         wk += (int64_t)gridDim.x * WAVES) {
        const int64_t n = wk / CB;
        const int32_t cb = (int32_t)(wk - n * CB);
        const int32_t c = cb * 64 + lane;
        const int32_t p0 = row_ptr[n], p1 = row_ptr[n + 1];
        if (p0 == p1) continue;
        float g[16];
        const float* gp = G + n * C16 + c;
#pragma unroll
        for (int r = 0; r < 16; ++r) g[r] = gp[(int64_t)r * C];
        for (int32_t e = p0; e < p1; ++e) {
            float x[R], w[P], dwv[P], v[T8];
            const float* xp = xs + (int64_t)src[e] * CR + c;
            const float* wp = tp_w + (int64_t)e * CP + c;
#pragma unroll
            for (int k = 0; k < P; ++k) { w[k] = wp[(int64_t)k * C]; dwv[k] = 0.0f; }
#pragma unroll
            for (int r = 0; r < R; ++r) x[r] = xp[(int64_t)r * C];
            kr.put_yc(lds[wid], Y + (int64_t)e * 16);
            wave_lds_sync();
            const float4* s4 = reinterpret_cast<const float4*>(lds[wid]);
            // eight t at a time: dw, the terms of D, and the first three
            // butterfly steps on them
            static_for<0, T8>([&](auto ic) {
                constexpr int i = decltype(ic)::value;
                const float4 ya = s4[2 * i], yb = s4[2 * i + 1];
                const float yc[8] = {ya.x, ya.y, ya.z, ya.w,
                                     yb.x, yb.y, yb.z, yb.w};
                float q[8];
                static_for<0, 8>([&](auto jc) {
                    constexpr int j = decltype(jc)::value;
                    constexpr int t = 8 * i + j;
                    constexpr int pp = TAB<LS>.tp[t];
                    constexpr int l1 = TAB<LS>.l1[pp], l3 = TAB<LS>.l3[pp];
                    const float xg = x[l1 * l1 + TAB<LS>.tk1[t]]
                                     * g[l3 * l3 + TAB<LS>.tk3[t]];
                    dwv[pp] = fmaf(yc[j], xg, dwv[pp]);
                    q[j] = w[pp] * xg;
                });
                const float lo = bfly_pair(bfly_pair(q[0], q[1], 32, b5),
                                           bfly_pair(q[2], q[3], 32, b5),
                                           16, b4);
                const float hi = bfly_pair(bfly_pair(q[4], q[5], 32, b5),
                                           bfly_pair(q[6], q[7], 32, b5),
                                           16, b4);
                v[i] = bfly_pair(lo, hi, 8, b3);
            });
            wave_lds_sync();
            float* dp = dw + (int64_t)e * CP + c;
#pragma unroll
            for (int k = 0; k < P; ++k) dp[(int64_t)k * C] = dwv[k];
            bfly_rest<T8, 4>(v, lane);
            // v[0], v[1] = D[t0], D[t0 + 64]: this lane's K rows
            float dy[16];
            kr.get(dy, 0);
#pragma unroll
            for (int k = 0; k < 16; ++k) dy[k] *= v[0];
            if constexpr (T > 64) {
                float kb[16];
                kr.get(kb, 1);
#pragma unroll
                for (int k = 0; k < 16; ++k) dy[k] = fmaf(kb[k], v[1], dy[k]);
            }
            bfly_rest<16, 32>(dy, lane);
            if ((lane & 3) == 0)
                dYp[((int64_t)cb * E + e) * 16 + (kr.t0 & 15)] = dy[0];
        }
    }
}

// ---------------------------------------------------------------------------
// The same three passes with the radial MLP's last layer inside:
//     w[e,p,c] = sum_j h[e,j] Wr[p C + c, j],      h [E,64], Wr [P C, 64]
// is formed per tile of ETILE = 16 edges and per path on
// v_mfma_f32_16x16x4_f32 and never reaches global memory; neither does dw,
// which bwd_edge multiplies by Wr on the same instruction into
//     dh[e,j] = sum_{p,c} dw[e,p,c] Wr[p C + c, j].
//
// A wave still owns one (node, 64-channel block) and walks its CSR row, now
// sixteen edges at a time.  Per tile it loads the sixteen h rows once as the
// A operand (lane = (edge i, k-quarter q), 16 registers) and writes the
// sixteen yc rows to its stripe.  Then per path: four 16x16 tiles over
// K = 64 (16 MFMAs each) give w[16 edges][64 channels], dropped into the
// wave's [16][WS] LDS stripe and read back with lane = channel; the products
// of that path's t run per edge as in the kernels above, with the
// accumulators in registers.  The sender (or G) rows a path needs are
// re-read per path: they stay in the caches, and holding sixteen edges of
// them would take 64 to 256 registers.
//
// The B operand comes from global memory: a channel block's slice of Wr is
// P x 16 KB, all of a CU's LDS at P = 10, while the whole matrix is 320 KB
// and stays in L2.  The caller packs it once so every load is one coalesced
// float4 per lane:
//     Wa[p][cb][nt][g][q][j][i] = Wr[p C + 64 cb + 16 nt + j, 16 q + 4 g + i]
//     Wb[p][cb][jt][g][q][n][i] = Wr[p C + 64 cb + 16 q + 4 g + i, 16 jt + n]
// (Wa for w, Wb for dh).  MFMA step s = 4 g + i multiplies the k = 16 q + s
// of the four lane quarters: the K order is permuted the same way on both
// operands, which a dot product does not see.
//
// bwd_edge keeps G[n] in registers.  Per (edge, path) it overwrites the
// lane's w in the stripe by its dw, takes the channel sums D[t] of the
// path's t with the butterfly (lane j ends with value rev6(j)) and stores
// them in the wave's D stripe.  After the dw of a path is complete the
// stripe is the A operand of the dh tile, accumulated over the paths in 16
// registers and written once per tile to this channel block's dhp slice.
// After the last path lane (u, k2 quad) takes dY[e_u, k2] = sum_t K[t,k2]
// D[u][t] from LDS.  A partial tile repeats its last edge in the unused
// rows, which are computed and never stored.
// ---------------------------------------------------------------------------

constexpr int ETILE = 16;
constexpr int RH = 64;                  // width of h
constexpr int WS = 68;                  // stripe row: b128 reads of 16 rows spread over the banks

typedef float f32x4 __attribute__((ext_vector_type(4)));

// first t of path p
template <int LS>
constexpr int path_t0(int p) {
    int t = 0;
    while (TAB<LS>.tp[t] != p) ++t;
    return t;
}

// number of t of path p
template <int LS>
constexpr int path_nt(int p) {
    return (2 * TAB<LS>.l1[p] + 1) * (2 * TAB<LS>.l3[p] + 1);
}

// 16 consecutive floats of a row, as this lane's share of an A operand
__device__ __forceinline__ void load16(float (&a)[16], const float* p) {
    const float4* p4 = reinterpret_cast<const float4*>(p);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 v = p4[g];
        a[4 * g] = v.x; a[4 * g + 1] = v.y; a[4 * g + 2] = v.z;
        a[4 * g + 3] = v.w;
    }
}

// stripe[16][WS] = A[16 x 64] * the packed slice at wa (4 column tiles)
__device__ __forceinline__ void w_tile(const float (&a)[16],
                                       const float4* __restrict__ wa,
                                       float* stripe, int lane) {
    const int q = lane >> 4, j = lane & 15;
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        float4 b[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) b[g] = wa[(nt * 4 + g) * 64 + lane];
        f32x4 d = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            d = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * g], b[g].x, d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * g + 1], b[g].y, d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * g + 2], b[g].z, d, 0, 0, 0);
            d = __builtin_amdgcn_mfma_f32_16x16x4f32(a[4 * g + 3], b[g].w, d, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
            stripe[(4 * q + r) * WS + nt * 16 + j] = d[r];
    }
}

// forward (TR = false) and bwd_node (TR = true) of k_mace_conv, w from h
template <int LS, bool TR>
__global__ __launch_bounds__(BLOCK)
void k_mace_conv_rad(
        const float* __restrict__ A, const float* __restrict__ h,
        const float4* __restrict__ Wa, const float* __restrict__ Y,
        const float* __restrict__ K, const int32_t* __restrict__ idx,
        const int32_t* __restrict__ perm, const int32_t* __restrict__ row_ptr,
        float* __restrict__ out, int64_t N, int32_t C) {
    constexpr int P = TAB<LS>.P, T = TAB<LS>.T, R = LS ? 4 : 1;
    constexpr int RA = TR ? 16 : R, RO = TR ? R : 16;
    __shared__ __attribute__((aligned(16))) float ws[WAVES][ETILE * WS];
    __shared__ __attribute__((aligned(16))) float ycs[WAVES][ETILE * T];
    __shared__ __attribute__((aligned(16))) float kl[KRows<LS>::FLOATS];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    KRows<LS> kr;
    kr.init(kl, K, lane);
    float* stripe = ws[wid];
    float* ycw = ycs[wid];
    const int32_t CB = C >> 6;
    const int64_t work = N * CB;
    const int64_t CA = RA * (int64_t)C;
    for (int64_t wk = (int64_t)blockIdx.x * WAVES + wid; wk < work;
         wk += (int64_t)gridDim.x * WAVES) {
        const int64_t n = wk / CB;
        const int32_t cb = (int32_t)(wk - n * CB);
        const int32_t c = cb * 64 + lane;
        const int32_t p0 = row_ptr[n], p1 = row_ptr[n + 1];
        float acc[RO];
#pragma unroll
        for (int r = 0; r < RO; ++r) acc[r] = 0.0f;
        for (int32_t pt = p0; pt < p1; pt += ETILE) {
            const int nv = p1 - pt < ETILE ? p1 - pt : ETILE;
            float ha[16];
            {
                const int32_t pp = pt + (lane & 15) < p1 ? pt + (lane & 15)
                                                         : p1 - 1;
                const int32_t e = TR ? perm[pp] : pp;
                load16(ha, h + (int64_t)e * RH + (lane >> 4) * 16);
            }
            for (int u = 0; u < nv; ++u) {
                const int32_t e = TR ? perm[pt + u] : pt + u;
                kr.put_yc(ycw + u * T, Y + (int64_t)e * 16);
            }
            // a real loop over the paths: unrolled, the scheduler hoists
            // every path's B loads to the top and spills
#pragma unroll 1
            for (int pr = 0; pr < P; ++pr) {
              w_tile(ha, Wa + ((int64_t)pr * CB + cb) * 1024, stripe, lane);
              wave_lds_sync();
              static_for<0, P>([&](auto pc) {
                constexpr int p = decltype(pc)::value;
                if (pr != p) return;
                constexpr int l1 = TAB<LS>.l1[p], l3 = TAB<LS>.l3[p];
                constexpr int d1 = 2 * l1 + 1, d3 = 2 * l3 + 1;
                constexpr int tb = path_t0<LS>(p);
                constexpr int la = TR ? l3 : l1, da = TR ? d3 : d1;
#pragma unroll 2
                for (int u = 0; u < nv; ++u) {
                    const int32_t e = TR ? perm[pt + u] : pt + u;
                    const float* ap = A + (int64_t)idx[e] * CA
                                      + (int64_t)(la * la) * C + c;
                    float a[da];
#pragma unroll
                    for (int r = 0; r < da; ++r) a[r] = ap[(int64_t)r * C];
                    const float w = stripe[u * WS + lane];
                    const float* yc = ycw + u * T + tb;
                    if constexpr (TR) {
#pragma unroll
                        for (int k3 = 0; k3 < d3; ++k3) {
                            const float wg = w * a[k3];
#pragma unroll
                            for (int k1 = 0; k1 < d1; ++k1)
                                acc[l1 * l1 + k1] = fmaf(
                                    wg, yc[k1 * d3 + k3], acc[l1 * l1 + k1]);
                        }
                    } else {
#pragma unroll
                        for (int k1 = 0; k1 < d1; ++k1) {
                            const float wx = w * a[k1];
#pragma unroll
                            for (int k3 = 0; k3 < d3; ++k3)
                                acc[l3 * l3 + k3] = fmaf(
                                    wx, yc[k1 * d3 + k3], acc[l3 * l3 + k3]);
                        }
                    }
                }
              });
              wave_lds_sync();
            }
        }
        float* op = out + n * (RO * (int64_t)C) + c;
#pragma unroll
        for (int r = 0; r < RO; ++r) op[(int64_t)r * C] = acc[r];
    }
}

template <int LS>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(2)))
void k_mace_conv_rad_bwd_edge(
        const float* __restrict__ G, const float* __restrict__ xs,
        const float* __restrict__ h, const float4* __restrict__ Wa,
        const float4* __restrict__ Wb, const float* __restrict__ Y,
        const float* __restrict__ K, const int32_t* __restrict__ src,
        const int32_t* __restrict__ row_ptr, float* __restrict__ dhp,
        float* __restrict__ dYp, int64_t N, int64_t E, int32_t C) {
    constexpr int P = TAB<LS>.P, T = TAB<LS>.T, R = LS ? 4 : 1;
    constexpr int DS = T + 1;           // odd: 16 rows on 16 banks
    __shared__ __attribute__((aligned(16))) float ws[WAVES][ETILE * WS];
    __shared__ __attribute__((aligned(16))) float ycs[WAVES][ETILE * T];
    __shared__ __attribute__((aligned(16))) float dss[WAVES][ETILE * DS];
    __shared__ __attribute__((aligned(16))) float kl[KRows<LS>::FLOATS];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    KRows<LS> kr;
    kr.init(kl, K, lane);
    float* stripe = ws[wid];
    float* ycw = ycs[wid];
    float* dsw = dss[wid];
    const int q = lane >> 4, j = lane & 15;
    const int32_t CB = C >> 6;
    const int64_t work = N * CB;
    const int64_t C16 = 16 * (int64_t)C, CR = R * (int64_t)C;
    for (int64_t wk = (int64_t)blockIdx.x * WAVES + wid; wk < work;
         wk += (int64_t)gridDim.x * WAVES) {
        const int64_t n = wk / CB;
        const int32_t cb = (int32_t)(wk - n * CB);
        const int32_t c = cb * 64 + lane;
        const int32_t p0 = row_ptr[n], p1 = row_ptr[n + 1];
        if (p0 == p1) continue;
        float g[16];
        const float* gp = G + n * C16 + c;
#pragma unroll
        for (int r = 0; r < 16; ++r) g[r] = gp[(int64_t)r * C];
        for (int32_t pt = p0; pt < p1; pt += ETILE) {
            const int nv = p1 - pt < ETILE ? p1 - pt : ETILE;
            float ha[16];
            {
                const int32_t e = pt + j < p1 ? pt + j : p1 - 1;
                load16(ha, h + (int64_t)e * RH + q * 16);
            }
            for (int u = 0; u < nv; ++u)
                kr.put_yc(ycw + u * T, Y + (int64_t)(pt + u) * 16);
            f32x4 dh[4];
#pragma unroll
            for (int jt = 0; jt < 4; ++jt)
                dh[jt] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 1
            for (int pr = 0; pr < P; ++pr) {
              w_tile(ha, Wa + ((int64_t)pr * CB + cb) * 1024, stripe, lane);
              wave_lds_sync();
              static_for<0, P>([&](auto pc) {
                constexpr int p = decltype(pc)::value;
                if (pr != p) return;
                constexpr int l1 = TAB<LS>.l1[p], l3 = TAB<LS>.l3[p];
                constexpr int d1 = 2 * l1 + 1, d3 = 2 * l3 + 1;
                constexpr int tb = path_t0<LS>(p), NV = d1 * d3;
                for (int u = 0; u < nv; ++u) {
                    const float* xp = xs + (int64_t)src[pt + u] * CR
                                      + (int64_t)(l1 * l1) * C + c;
                    float x[d1], v[NV];
#pragma unroll
                    for (int k1 = 0; k1 < d1; ++k1) x[k1] = xp[(int64_t)k1 * C];
                    const float w = stripe[u * WS + lane];
                    const float* yc = ycw + u * T + tb;
                    float dwv = 0.0f;
#pragma unroll
                    for (int k1 = 0; k1 < d1; ++k1)
#pragma unroll
                        for (int k3 = 0; k3 < d3; ++k3) {
                            const float xg = x[k1] * g[l3 * l3 + k3];
                            dwv = fmaf(yc[k1 * d3 + k3], xg, dwv);
                            v[k1 * d3 + k3] = w * xg;
                        }
                    stripe[u * WS + lane] = dwv;
                    bfly_rest<NV, 32>(v, lane);
                    if (kr.t0 < NV) dsw[u * DS + tb + kr.t0] = v[0];
                }
              });
              wave_lds_sync();
              {
                // dh += dw[16 edges x 64 channels] * Wr slice
                float da[16];
                load16(da, stripe + j * WS + q * 16);
                const float4* wb = Wb + ((int64_t)pr * CB + cb) * 1024;
#pragma unroll
                for (int jt = 0; jt < 4; ++jt) {
                    float4 b[4];
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq)
                        b[gq] = wb[(jt * 4 + gq) * 64 + lane];
#pragma unroll
                    for (int gq = 0; gq < 4; ++gq) {
                        dh[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            da[4 * gq], b[gq].x, dh[jt], 0, 0, 0);
                        dh[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            da[4 * gq + 1], b[gq].y, dh[jt], 0, 0, 0);
                        dh[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            da[4 * gq + 2], b[gq].z, dh[jt], 0, 0, 0);
                        dh[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                            da[4 * gq + 3], b[gq].w, dh[jt], 0, 0, 0);
                    }
                }
              }
              wave_lds_sync();
            }
            // dh rows 4 q + r, columns 16 jt + j
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (4 * q + r < nv) {
                    float* dp = dhp + ((int64_t)cb * E + pt + 4 * q + r) * RH + j;
#pragma unroll
                    for (int jt = 0; jt < 4; ++jt) dp[jt * 16] = dh[jt][r];
                }
            // dY[e_u, 4 kq ..] = sum_t K[t, 4 kq ..] D[u][t]
            {
                const int u = lane >> 2, kq = lane & 3;
                float4 dy = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
                for (int t = 0; t < T; ++t) {
                    const int row = (t & 64)      // as KRows::init places it
                        + (int)(__brev((unsigned)(t & 63)) >> 26);
                    const float4 k4 = reinterpret_cast<const float4*>(
                        kl + row * KRows<LS>::KS)[kq];
                    const float d = dsw[u * DS + t];
                    dy.x = fmaf(k4.x, d, dy.x); dy.y = fmaf(k4.y, d, dy.y);
                    dy.z = fmaf(k4.z, d, dy.z); dy.w = fmaf(k4.w, d, dy.w);
                }
                if (u < nv)
                    reinterpret_cast<float4*>(
                        dYp + ((int64_t)cb * E + pt + u) * 16)[kq] = dy;
            }
            wave_lds_sync();
        }
    }
}

int conv_check(int64_t N, int32_t C, int32_t ls, const char* name) {
    if (N < 0 || C <= 0 || C % 64 != 0 || (ls != 0 && ls != 1)) {
        char buf[128];
        snprintf(buf, sizeof buf,
                 "%s: C must be a positive multiple of 64 and ls 0 or 1",
                 name);
        dm_set_last_error(buf);
        return -1;
    }
    return 0;
}

int rad_check(int64_t N, int32_t C, int32_t H, int32_t ls, const char* name) {
    if (H != RH) {
        char buf[128];
        snprintf(buf, sizeof buf, "%s: H must be %d", name, RH);
        dm_set_last_error(buf);
        return -1;
    }
    return conv_check(N, C, ls, name);
}

int conv_launched() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dm_set_last_error(hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

}  // namespace

extern "C" {

int dm_mace_conv_fwd_f32(const float* xs, const float* tp_w, const float* Y,
                         const float* K, const int32_t* src,
                         const int32_t* row_ptr, float* M, int64_t N,
                         int32_t C, int32_t ls, uint64_t stream) {
    if (int rc = conv_check(N, C, ls, "dm_mace_conv_fwd_f32")) return rc;
    if (N == 0) return 0;
    const int nb = nblocks(N * (C / 64), WAVES);
    hipStream_t s = (hipStream_t)stream;
    if (ls == 0)
        k_mace_conv<0, false, 4><<<nb, BLOCK, 0, s>>>(
            xs, tp_w, Y, K, src, nullptr, row_ptr, M, N, C);
    else
        k_mace_conv<1, false, 2><<<nb, BLOCK, 0, s>>>(
            xs, tp_w, Y, K, src, nullptr, row_ptr, M, N, C);
    return conv_launched();
}

int dm_mace_conv_bwd_edge_f32(const float* G, const float* xs,
                              const float* tp_w, const float* Y,
                              const float* K, const int32_t* src,
                              const int32_t* row_ptr, float* dw, float* dYp,
                              int64_t N, int64_t E, int32_t C, int32_t ls,
                              uint64_t stream) {
    if (int rc = conv_check(N, C, ls, "dm_mace_conv_bwd_edge_f32")) return rc;
    if (N == 0 || E == 0) return 0;
    const int nb = nblocks(N * (C / 64), WAVES);
    hipStream_t s = (hipStream_t)stream;
    if (ls == 0)
        k_mace_conv_bwd_edge<0><<<nb, BLOCK, 0, s>>>(
            G, xs, tp_w, Y, K, src, row_ptr, dw, dYp, N, E, C);
    else
        k_mace_conv_bwd_edge<1><<<nb, BLOCK, 0, s>>>(
            G, xs, tp_w, Y, K, src, row_ptr, dw, dYp, N, E, C);
    return conv_launched();
}

int dm_mace_conv_bwd_node_f32(const float* G, const float* tp_w,
                              const float* Y, const float* K,
                              const int32_t* dst, const int32_t* src_perm,
                              const int32_t* src_row_ptr, float* dxs,
                              int64_t N, int32_t C, int32_t ls,
                              uint64_t stream) {
    if (int rc = conv_check(N, C, ls, "dm_mace_conv_bwd_node_f32")) return rc;
    if (N == 0) return 0;
    const int nb = nblocks(N * (C / 64), WAVES);
    hipStream_t s = (hipStream_t)stream;
    if (ls == 0)
        k_mace_conv<0, true, 2><<<nb, BLOCK, 0, s>>>(
            G, tp_w, Y, K, dst, src_perm, src_row_ptr, dxs, N, C);
    else
        k_mace_conv<1, true, 1><<<nb, BLOCK, 0, s>>>(
            G, tp_w, Y, K, dst, src_perm, src_row_ptr, dxs, N, C);
    return conv_launched();
}

int dm_mace_conv_rad_fwd_f32(const float* xs, const float* h, const float* Wa,
                             const float* Y, const float* K,
                             const int32_t* src, const int32_t* row_ptr,
                             float* M, int64_t N, int32_t C, int32_t H,
                             int32_t ls, uint64_t stream) {
    if (int rc = rad_check(N, C, H, ls, "dm_mace_conv_rad_fwd_f32")) return rc;
    if (N == 0) return 0;
    const int nb = nblocks(N * (C / 64), WAVES);
    hipStream_t s = (hipStream_t)stream;
    const float4* wa = reinterpret_cast<const float4*>(Wa);
    if (ls == 0)
        k_mace_conv_rad<0, false><<<nb, BLOCK, 0, s>>>(
            xs, h, wa, Y, K, src, nullptr, row_ptr, M, N, C);
    else
        k_mace_conv_rad<1, false><<<nb, BLOCK, 0, s>>>(
            xs, h, wa, Y, K, src, nullptr, row_ptr, M, N, C);
    return conv_launched();
}

int dm_mace_conv_rad_bwd_edge_f32(const float* G, const float* xs,
                                  const float* h, const float* Wa,
                                  const float* Wb, const float* Y,
                                  const float* K, const int32_t* src,
                                  const int32_t* row_ptr, float* dhp,
                                  float* dYp, int64_t N, int64_t E, int32_t C,
                                  int32_t H, int32_t ls, uint64_t stream) {
    if (int rc = rad_check(N, C, H, ls, "dm_mace_conv_rad_bwd_edge_f32"))
        return rc;
    if (N == 0 || E == 0) return 0;
    const int nb = nblocks(N * (C / 64), WAVES);
    hipStream_t s = (hipStream_t)stream;
    const float4* wa = reinterpret_cast<const float4*>(Wa);
    const float4* wb = reinterpret_cast<const float4*>(Wb);
    if (ls == 0)
        k_mace_conv_rad_bwd_edge<0><<<nb, BLOCK, 0, s>>>(
            G, xs, h, wa, wb, Y, K, src, row_ptr, dhp, dYp, N, E, C);
    else
        k_mace_conv_rad_bwd_edge<1><<<nb, BLOCK, 0, s>>>(
            G, xs, h, wa, wb, Y, K, src, row_ptr, dhp, dYp, N, E, C);
    return conv_launched();
}

int dm_mace_conv_rad_bwd_node_f32(const float* G, const float* h,
                                  const float* Wa, const float* Y,
                                  const float* K, const int32_t* dst,
                                  const int32_t* src_perm,
                                  const int32_t* src_row_ptr, float* dxs,
                                  int64_t N, int32_t C, int32_t H, int32_t ls,
                                  uint64_t stream) {
    if (int rc = rad_check(N, C, H, ls, "dm_mace_conv_rad_bwd_node_f32"))
        return rc;
    if (N == 0) return 0;
    const int nb = nblocks(N * (C / 64), WAVES);
    hipStream_t s = (hipStream_t)stream;
    const float4* wa = reinterpret_cast<const float4*>(Wa);
    if (ls == 0)
        k_mace_conv_rad<0, true><<<nb, BLOCK, 0, s>>>(
            G, h, wa, Y, K, dst, src_perm, src_row_ptr, dxs, N, C);
    else
        k_mace_conv_rad<1, true><<<nb, BLOCK, 0, s>>>(
            G, h, wa, Y, K, dst, src_perm, src_row_ptr, dxs, N, C);
    return conv_launched();
}

}  // extern "C"
