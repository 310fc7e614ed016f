// mace_symc.hip — gfx950 (CDNA4) kernels for the MACE symmetric contraction,
// evaluated through its coupling trees (so3.symmetric_basis_trees).
//
// Per node n with element e = elem[n], per channel c, x[16] the l-major rows
// of xs [N,16,C]:
//
//     q_{l1,l2,L}[mL] = sum_{a,b} CG(l1,l2,L)[a,b,mL] x[l1,a] x[l2,b]   (stage 1)
//     v_{L,l3,lo}[mL] = sum_{trees t = (l1,l2,L,l3) of lo} W[e,wrow(t),c] q_t[mL]
//     out[lo,mo]     += sum_{mL,k} CG(L,l3,lo)[mL,k,mo] v[mL] x[l3,k]   (stage 2)
//
// The same polynomial written out flat (k_mace_symc_* in kernels.hip) is a
// list of four-factor terms w x x x, 2953 of them for the first layer; here
// every term is a two-factor product, about 1300 stage-1 and 160 stage-2 terms.
//
// One form for every correlation order.  Row 16 of x is the constant 1.  A
// nu = 2 tree (l1, l2) of lo is a tree with L = lo whose second coupling is
// the identity against row 16; the nu = 1 tree (lo,) is one whose stage 1 is
// x[lo,m] * 1.  So the nu <= 2 trees of one lo form one more group, and the
// multiplications by 1 are exact.
//
// Mapping: one wave per (node, 64-channel block), lane = channel, grid-stride
// over N * C/64, as in mace_conv.hip.  Every global access of a wave is one
// coalesced 256 B row.  Any C % 64 == 0 is served.
//
// Tables.  The caller builds one int32 table (mace_ops._symc_tree_tables) from
// so3.real_cg and the tree lists; the kernels hold no tree list of their own.
// Only maxima are compile-time: 16 x rows, 2L+1 <= 9, S_out <= 4.  Every
// table read is wave-uniform and goes through the scalar cache.
//
//     header [16]   n_groups, then the int32 offsets of the four sections
//                   below and of nz
//     groups [G,8]  tree_beg, tree_end, and three [beg,end) ranges of segs:
//                   stage 2 by out row, by mL, by x row
//     trees  [.,2]  wrow, pair
//     pairs  [.,12] row pointers [10] of the pair's stage-1 entries by mL,
//                   and the [beg,end) range of its transposed segs
//     segs   [.,4]  dst, nz_beg, nz_end, 0
//     nz     [.,2]  p | q << 8, and the coefficient's bits
//
// A seg is a sum  sum_j coef_j A[p_j] B[q_j]  whose destination row dst is
// fixed, so it accumulates in one register; which LDS rows A and B are
// depends on the use (below).  A pair (l1,l2,L) is stored once and
// recomputed per tree that uses it: holding every pair's q and every group's
// v live would need 100 to 170 values per lane.
//
// Schedule, forward.  Per group (L, l3, lo): v[9] = 0 in registers; per tree,
// load its weight row and run the pair's nine mL rows (A = B = x),
// v[mL] += w q; store v to the wave's LDS stripe; run the group's stage-2
// segs by out row (A = v, B = x) into the four out accumulators, which stay
// in registers.
//
// Schedule, reverse (dx only: the weights are frozen).  Same group order.  Per
// group, recompute v as above; dv[mL] = sum CG3 g[mo] x[k] from the segs by mL
// (A = g, B = x); dx[l3,k] += sum CG3 g[mo] v[mL] from the segs by x row
// (A = g, B = v); per tree, the pair's transposed segs (A = dv, B = x) give
//     dx[r] += w * sum coef dv[mL] x[s]
// with both (r,s) = (a,b) and (b,a) of every stage-1 entry listed, entries
// whose r is row 16 left out.  dx is sixteen LDS rows, written once per node:
// no atomics, and every launch gives the same bits.
//
// Where values live.  x, v, g, dv, dx are rows of the wave's own LDS stripe
// (their index is run-time), 64 consecutive floats each, so no access has a
// bank conflict.  A lane reads only what it wrote itself, so there is no
// barrier or fence anywhere: none inside the grid-stride loop, where a block
// barrier would deadlock when wave trip counts differ (see k_mace_tp_bwd).
//
// Matrix instructions do not fit.  The weights differ per channel and per
// element and the couplings act on the m index of a single channel: there is
// no contraction over channels or nodes to tile on MFMA.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/distmlip_hip.h"

void dm_set_last_error(const char* msg);      // kernels.hip

namespace {

constexpr int BLOCK = 128;
constexpr int WAVES = BLOCK / 64;
constexpr int MAX_BLOCKS = 16384;
constexpr int XR = 17;                 // x rows, row 16 == 1
constexpr int VR = 9;                  // 2L+1 <= 9
constexpr int OR = 4;                  // S_out <= 4
constexpr int FWD_ROWS = XR + VR;
constexpr int BWD_ROWS = XR + VR + OR + VR + 16;

inline int nblocks(int64_t work, int64_t per_block) {
    int64_t b = (work + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b));
}

struct Tab {
    int ng;
    const int32_t* groups;
    const int32_t* trees;
    const int32_t* pairs;
    const int32_t* segs;
    const int2* nz;
};

__device__ __forceinline__ Tab open_tab(const int32_t* __restrict__ tab) {
    Tab t;
    t.ng = tab[0];
    t.groups = tab + tab[1];
    t.trees = tab + tab[2];
    t.pairs = tab + tab[3];
    t.segs = tab + tab[4];
    t.nz = reinterpret_cast<const int2*>(tab + tab[5]);
    return t;
}

// sum_j coef_j A[p_j] B[q_j] over entries [beg, end); A and B are the lane's
// columns of two LDS row blocks
__device__ __forceinline__ float seg_dot(const int2* __restrict__ nz, int beg,
                                         int end, const float* A,
                                         const float* B) {
    float acc = 0.0f;
#pragma unroll 4
    for (int j = beg; j < end; ++j) {
        const int2 e = nz[j];
        acc = fmaf(__int_as_float(e.y) * A[(e.x & 255) * 64],
                   B[(e.x >> 8) * 64], acc);
    }
    return acc;
}

// v[mL] = sum_{trees of the group} w_t q_t[mL]; Wn is the lane's column of the
// node's weight rows
__device__ __forceinline__ void group_v(const Tab& t, const int32_t* grp,
                                        const float* __restrict__ Wn,
                                        int32_t C, const float* X,
                                        float (&v)[VR]) {
#pragma unroll
    for (int m = 0; m < VR; ++m) v[m] = 0.0f;
    for (int tr = grp[0]; tr < grp[1]; ++tr) {
        const float w = Wn[(int64_t)t.trees[2 * tr] * C];
        const int32_t* rp = t.pairs + 12 * t.trees[2 * tr + 1];
#pragma unroll
        for (int m = 0; m < VR; ++m)
            v[m] = fmaf(w, seg_dot(t.nz, rp[m], rp[m + 1], X, X), v[m]);
    }
}

__global__ __launch_bounds__(BLOCK) void k_mace_symc_tree_fwd(
        const float* __restrict__ x, const int32_t* __restrict__ elem,
        const float* __restrict__ W, const int32_t* __restrict__ tab,
        float* __restrict__ out, int64_t N, int32_t C, int32_t T,
        int32_t S_out) {
    __shared__ float lds[WAVES * FWD_ROWS * 64];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* X = lds + wid * (FWD_ROWS * 64) + lane;
    float* V = X + XR * 64;
    const Tab t = open_tab(tab);
    const int32_t CB = C / 64;
    X[16 * 64] = 1.0f;
    for (int64_t wk = blockIdx.x * (int64_t)WAVES + wid; wk < N * CB;
         wk += (int64_t)gridDim.x * WAVES) {
        const int64_t n = wk / CB;
        const int64_t col = (wk - n * CB) * 64 + lane;
        const float* xn = x + n * 16 * C + col;
#pragma unroll
        for (int a = 0; a < 16; ++a) X[a * 64] = xn[(int64_t)a * C];
        const float* Wn = W + (int64_t)elem[n] * T * C + col;
        float o[OR] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int g = 0; g < t.ng; ++g) {
            const int32_t* grp = t.groups + 8 * g;
            float v[VR];
            group_v(t, grp, Wn, C, X, v);
#pragma unroll
            for (int m = 0; m < VR; ++m) V[m * 64] = v[m];
            for (int sg = grp[2]; sg < grp[3]; ++sg) {
                const int32_t* seg = t.segs + 4 * sg;
                const float acc = seg_dot(t.nz, seg[1], seg[2], V, X);
                const int r = seg[0];
#pragma unroll
                for (int i = 0; i < OR; ++i) o[i] += r == i ? acc : 0.0f;
            }
        }
#pragma unroll
        for (int i = 0; i < OR; ++i)
            if (i < S_out) out[(n * S_out + i) * C + col] = o[i];
    }
}

__global__ __launch_bounds__(BLOCK) void k_mace_symc_tree_bwd(
        const float* __restrict__ go, const float* __restrict__ x,
        const int32_t* __restrict__ elem, const float* __restrict__ W,
        const int32_t* __restrict__ tab, float* __restrict__ dx, int64_t N,
        int32_t C, int32_t T, int32_t S_out) {
    __shared__ float lds[WAVES * BWD_ROWS * 64];
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float* X = lds + wid * (BWD_ROWS * 64) + lane;
    float* V = X + XR * 64;
    float* G = V + VR * 64;
    float* DV = G + OR * 64;
    float* DX = DV + VR * 64;
    const Tab t = open_tab(tab);
    const int32_t CB = C / 64;
    X[16 * 64] = 1.0f;
    for (int64_t wk = blockIdx.x * (int64_t)WAVES + wid; wk < N * CB;
         wk += (int64_t)gridDim.x * WAVES) {
        const int64_t n = wk / CB;
        const int64_t col = (wk - n * CB) * 64 + lane;
        const float* xn = x + n * 16 * C + col;
#pragma unroll
        for (int a = 0; a < 16; ++a) {
            X[a * 64] = xn[(int64_t)a * C];
            DX[a * 64] = 0.0f;
        }
#pragma unroll
        for (int i = 0; i < OR; ++i)
            G[i * 64] = i < S_out ? go[(n * S_out + i) * C + col] : 0.0f;
        const float* Wn = W + (int64_t)elem[n] * T * C + col;
        for (int g = 0; g < t.ng; ++g) {
            const int32_t* grp = t.groups + 8 * g;
            float v[VR];
            group_v(t, grp, Wn, C, X, v);
#pragma unroll
            for (int m = 0; m < VR; ++m) {
                V[m * 64] = v[m];
                DV[m * 64] = 0.0f;
            }
            for (int sg = grp[4]; sg < grp[5]; ++sg) {
                const int32_t* seg = t.segs + 4 * sg;
                DV[seg[0] * 64] = seg_dot(t.nz, seg[1], seg[2], G, X);
            }
            for (int sg = grp[6]; sg < grp[7]; ++sg) {
                const int32_t* seg = t.segs + 4 * sg;
                DX[seg[0] * 64] += seg_dot(t.nz, seg[1], seg[2], G, V);
            }
            for (int tr = grp[0]; tr < grp[1]; ++tr) {
                const float w = Wn[(int64_t)t.trees[2 * tr] * C];
                const int32_t* rp = t.pairs + 12 * t.trees[2 * tr + 1];
                for (int sg = rp[10]; sg < rp[11]; ++sg) {
                    const int32_t* seg = t.segs + 4 * sg;
                    DX[seg[0] * 64] = fmaf(
                        w, seg_dot(t.nz, seg[1], seg[2], DV, X),
                        DX[seg[0] * 64]);
                }
            }
        }
        float* dn = dx + n * 16 * C + col;
#pragma unroll
        for (int a = 0; a < 16; ++a) dn[(int64_t)a * C] = DX[a * 64];
    }
}

int tree_check(int64_t N, int32_t C, int32_t T, int32_t S_out,
               const char* name) {
    if (N < 0 || C <= 0 || C % 64 != 0 || T <= 0 || S_out < 1 ||
        S_out > OR) {
        char buf[128];
        snprintf(buf, sizeof buf,
                 "%s: C must be a positive multiple of 64 and S_out 1..4",
                 name);
        dm_set_last_error(buf);
        return -1;
    }
    return 0;
}

int tree_launched() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dm_set_last_error(hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

}  // namespace

extern "C" {

int dm_mace_symc_tree_fwd_f32(const float* x, const int32_t* elem,
                              const float* W, const int32_t* tab, float* out,
                              int64_t N, int32_t C, int32_t T, int32_t S_out,
                              uint64_t stream) {
    if (int rc = tree_check(N, C, T, S_out, "dm_mace_symc_tree_fwd_f32"))
        return rc;
    if (N == 0) return 0;
    k_mace_symc_tree_fwd<<<nblocks(N * (C / 64), WAVES), BLOCK, 0,
                           (hipStream_t)stream>>>(x, elem, W, tab, out, N, C,
                                                  T, S_out);
    return tree_launched();
}

int dm_mace_symc_tree_bwd_f32(const float* go, const float* x,
                              const int32_t* elem, const float* W,
                              const int32_t* tab, float* dx, int64_t N,
                              int32_t C, int32_t T, int32_t S_out,
                              uint64_t stream) {
    if (int rc = tree_check(N, C, T, S_out, "dm_mace_symc_tree_bwd_f32"))
        return rc;
    if (N == 0) return 0;
    k_mace_symc_tree_bwd<<<nblocks(N * (C / 64), WAVES), BLOCK, 0,
                           (hipStream_t)stream>>>(go, x, elem, W, tab, dx, N,
                                                  C, T, S_out);
    return tree_launched();
}

}  // extern "C"
