// tensornet.hip — gfx950 (CDNA4) kernels for the TensorNet message pass.
//
// TensorNet's node state is one 3x3 tensor per channel, stored
// component-major: X[n, 3a+b, c], nine rows of C floats per node.  An
// interaction layer sums, at every node i, the sender tensors decomposed
// into their isotropic / antisymmetric / symmetric-traceless parts
// (I, A, S), each part scaled by a per-edge per-channel radial weight
// f[e, k, c]:
//
//     M[i,:,c] = sum_{e -> i} sum_k f[e,k,c] * P_k(Y[src[e],:,c])
//
// Written op by op that is a gather to [E, 9, C], a scale and a segment sum:
// 2304 B per edge and per tensor at C = 64, written and read back, in the
// forward and again in the reverse.  The kernels here never form an
// [E, 9, C] array.
//
// Mapping: one wave per (node, 64-channel block), lane = channel.  The nine
// accumulators of a lane live in registers; every global access of a wave is
// one coalesced 256 B row (three rows of f and nine rows of Y per edge); the
// edge's source node is wave-uniform and comes through the scalar cache.
// Edges are taken four at a time: 48 independent row loads in flight per
// wave at 16 waves per CU (<= 128 VGPRs), enough to cover an HBM miss on
// random 2304 B rows.
// Each row is summed by one wave in CSR order: no atomics, and the result is
// the same bit for bit on every run.
//
// The projections are self-adjoint under the Frobenius product, so the
// reverse pass uses the same three forms:
//     df[e,k,c] = < G[dst(e),:,c], P_k(Y[src[e],:,c]) >       (dst CSR)
//     dY[j,:,c] = sum_{e in out(j)} sum_k f[e,k,c] P_k(G[dst[e],:,c])
//                                                (src permutation CSR)
// and dY is the forward kernel run over the other CSR.

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "../../include/distmlip_hip.h"

void dm_set_last_error(const char* msg);      // kernels.hip

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int MAX_BLOCKS = 8192;
constexpr int UNROLL = 4;

inline int nblocks(int64_t work, int64_t per_block) {
    int64_t b = (work + per_block - 1) / per_block;
    return (int)(b < 1 ? 1 : (b > MAX_BLOCKS ? MAX_BLOCKS : b));
}

// a + b + c with the rounding errors of both additions added back in
// (Knuth's TwoSum): the result is accurate relative to |a + b + c| itself,
// not to |a| + |b| + |c|, so a trace whose terms cancel keeps its digits.
__device__ __forceinline__ float sum3(float a, float b, float c) {
    const float s1 = a + b, b1 = s1 - a;
    const float e1 = (a - (s1 - b1)) + (b - b1);
    const float s2 = s1 + c, b2 = s2 - s1;
    const float e2 = (s1 - (s2 - b2)) + (c - b2);
    return s2 + (e1 + e2);
}

// The diagonal of the I and S parts of t: tr/3 and t_aa - tr/3, the latter
// as (2 t_aa - t_bb - t_cc)/3 so that it too is accurate relative to itself.
__device__ __forceinline__ void tn_diag(const float (&t)[9], float& tr3,
                                        float (&sd)[3]) {
    constexpr float third = 1.0f / 3.0f;
    tr3 = sum3(t[0], t[4], t[8]) * third;
    sd[0] = sum3(2.0f * t[0], -t[4], -t[8]) * third;
    sd[1] = sum3(2.0f * t[4], -t[0], -t[8]) * third;
    sd[2] = sum3(2.0f * t[8], -t[0], -t[4]) * third;
}

// acc += sum_k w[k] * P_k(t), t a 3x3 tensor in row order 3a+b.
//   I = tr(t)/3 * 1,  A = (t - t^T)/2,  S = (t + t^T)/2 - I
// Every part is formed first, accurately relative to itself, and then
// scaled, so each product's rounding error is relative to
// |w_k| * |P_k(t)|, never to a cancelled sum.
__device__ __forceinline__ void tn_accum(float (&acc)[9], const float (&t)[9],
                                         const float (&w)[3]) {
    float tr3, sd[3];
    tn_diag(t, tr3, sd);
    acc[0] = fmaf(w[0], tr3, fmaf(w[2], sd[0], acc[0]));
    acc[4] = fmaf(w[0], tr3, fmaf(w[2], sd[1], acc[4]));
    acc[8] = fmaf(w[0], tr3, fmaf(w[2], sd[2], acc[8]));
    const float a01 = 0.5f * (t[1] - t[3]), s01 = 0.5f * (t[1] + t[3]);
    const float a02 = 0.5f * (t[2] - t[6]), s02 = 0.5f * (t[2] + t[6]);
    const float a12 = 0.5f * (t[5] - t[7]), s12 = 0.5f * (t[5] + t[7]);
    acc[1] = fmaf(w[1], a01, fmaf(w[2], s01, acc[1]));
    acc[3] = fmaf(-w[1], a01, fmaf(w[2], s01, acc[3]));
    acc[2] = fmaf(w[1], a02, fmaf(w[2], s02, acc[2]));
    acc[6] = fmaf(-w[1], a02, fmaf(w[2], s02, acc[6]));
    acc[5] = fmaf(w[1], a12, fmaf(w[2], s12, acc[5]));
    acc[7] = fmaf(-w[1], a12, fmaf(w[2], s12, acc[7]));
}

// out[n,:,c] = sum over the CSR row of n of sum_k f[e,k,c] P_k(T[idx[e],:,c])
// with e = perm ? perm[p] : p for p in [row_ptr[n], row_ptr[n+1]).
//   forward: T = Y, idx = src, perm = null, the dst CSR
//   reverse: T = G, idx = dst, perm = src_perm, the src CSR
template <bool PERM>
__global__ __launch_bounds__(BLOCK) void k_tn_msg(
        const float* __restrict__ T, const float* __restrict__ f,
        const int32_t* __restrict__ idx, const int32_t* __restrict__ perm,
        const int32_t* __restrict__ row_ptr, float* __restrict__ out,
        int64_t N, int32_t C) {
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int32_t CB = C >> 6;
    const int64_t work = N * CB;
    const int64_t C9 = 9 * (int64_t)C, C3 = 3 * (int64_t)C;
    for (int64_t w = (int64_t)blockIdx.x * WAVES + wid; w < work;
         w += (int64_t)gridDim.x * WAVES) {
        const int64_t n = w / CB;
        const int32_t c = (int32_t)(w - n * CB) * 64 + lane;
        const int32_t p0 = row_ptr[n], p1 = row_ptr[n + 1];
        float acc[9];
#pragma unroll
        for (int r = 0; r < 9; ++r) acc[r] = 0.0f;
        int32_t p = p0;
        for (; p + UNROLL <= p1; p += UNROLL) {
            float t[UNROLL][9], wk[UNROLL][3];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const int32_t e = PERM ? perm[p + u] : p + u;
                const float* tp = T + (int64_t)idx[e] * C9 + c;
                const float* fp = f + (int64_t)e * C3 + c;
#pragma unroll
                for (int k = 0; k < 3; ++k) wk[u][k] = fp[(int64_t)k * C];
#pragma unroll
                for (int r = 0; r < 9; ++r) t[u][r] = tp[(int64_t)r * C];
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) tn_accum(acc, t[u], wk[u]);
        }
        for (; p < p1; ++p) {
            float t[9], wk[3];
            const int32_t e = PERM ? perm[p] : p;
            const float* tp = T + (int64_t)idx[e] * C9 + c;
            const float* fp = f + (int64_t)e * C3 + c;
#pragma unroll
            for (int k = 0; k < 3; ++k) wk[k] = fp[(int64_t)k * C];
#pragma unroll
            for (int r = 0; r < 9; ++r) t[r] = tp[(int64_t)r * C];
            tn_accum(acc, t, wk);
        }
        float* op = out + n * C9 + c;
#pragma unroll
        for (int r = 0; r < 9; ++r) op[(int64_t)r * C] = acc[r];
    }
}

// df[e,k,c] = < G[n,:,c], P_k(Y[src[e],:,c]) > for the in-edges e of node n.
// The node's G row is read once and kept as the ten sums the three inner
// products need.
__device__ __forceinline__ void tn_edge_dots(const float (&t)[9], float gtr,
                                             const float (&gd)[3],
                                             const float (&gs)[3],
                                             const float (&gdiag)[3],
                                             float (&d)[3]) {
    float tr3, sd[3];
    tn_diag(t, tr3, sd);
    d[0] = gtr * tr3;
    const float a01 = 0.5f * (t[1] - t[3]), s01 = 0.5f * (t[1] + t[3]);
    const float a02 = 0.5f * (t[2] - t[6]), s02 = 0.5f * (t[2] + t[6]);
    const float a12 = 0.5f * (t[5] - t[7]), s12 = 0.5f * (t[5] + t[7]);
    d[1] = fmaf(gd[0], a01, fmaf(gd[1], a02, gd[2] * a12));
    float s = gdiag[0] * sd[0];
    s = fmaf(gdiag[1], sd[1], s);
    s = fmaf(gdiag[2], sd[2], s);
    s = fmaf(gs[0], s01, s);
    s = fmaf(gs[1], s02, s);
    d[2] = fmaf(gs[2], s12, s);
}

__global__ __launch_bounds__(BLOCK) void k_tn_msg_bwd_edge(
        const float* __restrict__ G, const float* __restrict__ Y,
        const int32_t* __restrict__ src, const int32_t* __restrict__ row_ptr,
        float* __restrict__ df, int64_t N, int32_t C) {
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int32_t CB = C >> 6;
    const int64_t work = N * CB;
    const int64_t C9 = 9 * (int64_t)C, C3 = 3 * (int64_t)C;
    for (int64_t w = (int64_t)blockIdx.x * WAVES + wid; w < work;
         w += (int64_t)gridDim.x * WAVES) {
        const int64_t n = w / CB;
        const int32_t c = (int32_t)(w - n * CB) * 64 + lane;
        const int32_t p0 = row_ptr[n], p1 = row_ptr[n + 1];
        if (p0 == p1) continue;
        float g[9];
        const float* gp = G + n * C9 + c;
#pragma unroll
        for (int r = 0; r < 9; ++r) g[r] = gp[(int64_t)r * C];
        const float gtr = g[0] + g[4] + g[8];
        const float gd[3] = {g[1] - g[3], g[2] - g[6], g[5] - g[7]};
        const float gs[3] = {g[1] + g[3], g[2] + g[6], g[5] + g[7]};
        const float gdiag[3] = {g[0], g[4], g[8]};
        int32_t p = p0;
        for (; p + UNROLL <= p1; p += UNROLL) {
            float t[UNROLL][9];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const float* tp = Y + (int64_t)src[p + u] * C9 + c;
#pragma unroll
                for (int r = 0; r < 9; ++r) t[u][r] = tp[(int64_t)r * C];
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                float d[3];
                tn_edge_dots(t[u], gtr, gd, gs, gdiag, d);
                float* dp = df + (int64_t)(p + u) * C3 + c;
#pragma unroll
                for (int k = 0; k < 3; ++k) dp[(int64_t)k * C] = d[k];
            }
        }
        for (; p < p1; ++p) {
            float t[9], d[3];
            const float* tp = Y + (int64_t)src[p] * C9 + c;
#pragma unroll
            for (int r = 0; r < 9; ++r) t[r] = tp[(int64_t)r * C];
            tn_edge_dots(t, gtr, gd, gs, gdiag, d);
            float* dp = df + (int64_t)p * C3 + c;
#pragma unroll
            for (int k = 0; k < 3; ++k) dp[(int64_t)k * C] = d[k];
        }
    }
}

int tn_check(int64_t N, int32_t C, const char* name) {
    if (N < 0 || C <= 0 || C % 64 != 0) {
        char buf[96];
        snprintf(buf, sizeof buf, "%s: C must be a positive multiple of 64",
                 name);
        dm_set_last_error(buf);
        return -1;
    }
    return 0;
}

int tn_launched() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dm_set_last_error(hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

}  // namespace

extern "C" {

int dm_tn_msg_fwd_f32(const float* Y, const float* f, const int32_t* src,
                      const int32_t* row_ptr, float* M, int64_t N, int32_t C,
                      uint64_t stream) {
    if (int rc = tn_check(N, C, "dm_tn_msg_fwd_f32")) return rc;
    if (N == 0) return 0;
    k_tn_msg<false><<<nblocks(N * (C / 64), WAVES), BLOCK, 0,
                      (hipStream_t)stream>>>(Y, f, src, nullptr, row_ptr, M,
                                             N, C);
    return tn_launched();
}

int dm_tn_msg_bwd_edge_f32(const float* G, const float* Y, const int32_t* src,
                           const int32_t* row_ptr, float* df, int64_t N,
                           int32_t C, uint64_t stream) {
    if (int rc = tn_check(N, C, "dm_tn_msg_bwd_edge_f32")) return rc;
    if (N == 0) return 0;
    k_tn_msg_bwd_edge<<<nblocks(N * (C / 64), WAVES), BLOCK, 0,
                        (hipStream_t)stream>>>(G, Y, src, row_ptr, df, N, C);
    return tn_launched();
}

int dm_tn_msg_bwd_node_f32(const float* G, const float* f, const int32_t* dst,
                           const int32_t* src_perm,
                           const int32_t* src_row_ptr, float* dY, int64_t N,
                           int32_t C, uint64_t stream) {
    if (int rc = tn_check(N, C, "dm_tn_msg_bwd_node_f32")) return rc;
    if (N == 0) return 0;
    k_tn_msg<true><<<nblocks(N * (C / 64), WAVES), BLOCK, 0,
                     (hipStream_t)stream>>>(G, f, dst, src_perm, src_row_ptr,
                                            dY, N, C);
    return tn_launched();
}

}  // extern "C"
