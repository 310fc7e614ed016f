// md.hip — gfx950 (CDNA4) kernels for the native MD / relaxation driver
// (distmlip_amd/md.py): the integrator state update and its reductions.
//
// The state is fp64 throughout: wrapped fractional coordinates frac [N,3],
// cartesian velocities vel [N,3], inverse masses inv_mass [N].  Forces come
// as the engines' fp32 (or fp64 from an fp64 source).  One thread owns one
// atom, 256 threads per block.  Two kernels cover every integrator of the
// driver:
//
//   k_md_kick_drift   v = a v + b F/m, drift (plain or the Langevin "AOA"
//                     middle of BAOAB), cartesian -> fractional, periodic
//                     wrap into [0,1).  116 B per atom: frac and vel read
//                     and written (96), the fp32 force (12), inv_mass (8);
//                     the Langevin form reads 24 B of noise on top.
//   k_md_kick_reduce  v += b F/m and five sums in the same pass:
//                     sum m v^2, sum F.v, sum |F|^2, sum |v|^2, max |F_i|^2.
//                     68 B per atom with the kick, 44 B as a pure reduction
//                     (b == 0 leaves vel unwritten).
//
// Both are HBM streams far below the force step's cost; what they buy is one
// launch instead of a chain of elementwise ones, no [N,3] temporaries, a
// reduction tree that is fixed (wave shuffles, LDS across the four waves, one
// plain store per block, then one single-block pass over the per-block
// partials in index order: no atomics, bit-identical from run to run), and
// the periodic wrap in one place.
//
// Every expression is evaluated op by op (no fused multiply-add): the fp64
// torch composition in distmlip_amd/md_ops.py performs the same operations
// in the same order, and the two agree to the bit per atom.
//
// The wrap: on a periodic dim f -= floor(f), which rounds to exactly 1.0 for
// a tiny negative f (-1e-17 - floor(-1e-17) = 1 - 1e-17 -> 1.0); a result
// >= 1.0 therefore becomes 0.0, the same point on the circle.  The graph
// builder's contract is frac in [0,1) on periodic dims.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/distmlip_hip.h"

#pragma clang fp contract(off)

void dm_set_last_error(const char* msg);      // kernels.hip

namespace {

constexpr int BLOCK = 256;
constexpr int WAVES = BLOCK / 64;
constexpr int NRED = 5;           // m v^2, F.v, |F|^2, |v|^2, max |F_i|^2

// inverse lattice rows (frac = cart @ Linv) and periodic flags, by value
struct MdCell {
    double li[9];
    int32_t per[3];
};

__device__ __forceinline__ double wrap01(double f) {
    f = f - floor(f);
    return f >= 1.0 ? 0.0 : f;
}

template <bool LANGEVIN, typename FT>
__global__ void __launch_bounds__(BLOCK)
k_md_kick_drift(double* __restrict__ frac, double* __restrict__ vel,
                const FT* __restrict__ force,
                const double* __restrict__ inv_mass,
                const double* __restrict__ xi, double a, double b, double h,
                double c1, double c2, MdCell cell, int64_t N) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= N) return;
    const double im = inv_mass ? inv_mass[i] : 1.0;
    const double t = inv_mass ? b * im : b;
    double v[3], dr[3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
        v[k] = a * vel[3 * i + k] + t * (double)force[3 * i + k];
    if (LANGEVIN) {
        const double hh = 0.5 * h;
        const double s = inv_mass ? c2 * sqrt(im) : c2;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double d1 = hh * v[k];
            v[k] = c1 * v[k] + s * xi[3 * i + k];
            dr[k] = d1 + hh * v[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) dr[k] = h * v[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        vel[3 * i + k] = v[k];
        const double df = (dr[0] * cell.li[k] + dr[1] * cell.li[3 + k])
                          + dr[2] * cell.li[6 + k];
        const double f = frac[3 * i + k] + df;
        frac[3 * i + k] = cell.per[k] ? wrap01(f) : f;
    }
}

// Fixed tree over the block: 64-lane shuffle halving, then the four wave
// results through LDS, added in wave order by thread 0.  Valid in thread 0.
// fmax drops a NaN operand, so for a NaN force the max slot stays finite
// where torch's .max() in the composition returns NaN; the |F|^2 sum next to
// it is NaN in both, and that is what the driver tests for non-finite input.
__device__ __forceinline__ void block_reduce(double (&r)[NRED],
                                             double (*lds)[NRED]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < NRED - 1; ++q) r[q] = r[q] + __shfl_down(r[q], off, 64);
        r[NRED - 1] = fmax(r[NRED - 1], __shfl_down(r[NRED - 1], off, 64));
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int q = 0; q < NRED; ++q) lds[wave][q] = r[q];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NRED; ++q) r[q] = lds[0][q];
        for (int w = 1; w < WAVES; ++w) {
#pragma unroll
            for (int q = 0; q < NRED - 1; ++q) r[q] = r[q] + lds[w][q];
            r[NRED - 1] = fmax(r[NRED - 1], lds[w][NRED - 1]);
        }
    }
}

// partials is [NRED, nb] (nb = gridDim.x): one row per quantity
template <bool KICK, typename FT>
__global__ void __launch_bounds__(BLOCK)
k_md_kick_reduce(double* __restrict__ vel, const FT* __restrict__ force,
                 const double* __restrict__ inv_mass, double b,
                 double* __restrict__ partials, int64_t N) {
    __shared__ double lds[WAVES][NRED];
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    double r[NRED] = {0.0, 0.0, 0.0, 0.0, 0.0};
    if (i < N) {
        const double im = inv_mass ? inv_mass[i] : 1.0;
        double v[3], f[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v[k] = vel[3 * i + k];
            f[k] = (double)force[3 * i + k];
        }
        if (KICK) {
            const double t = inv_mass ? b * im : b;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v[k] = v[k] + t * f[k];
                vel[3 * i + k] = v[k];
            }
        }
        const double v2 = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
        r[0] = inv_mass ? v2 / im : v2;
        r[1] = (f[0] * v[0] + f[1] * v[1]) + f[2] * v[2];
        r[2] = (f[0] * f[0] + f[1] * f[1]) + f[2] * f[2];
        r[3] = v2;
        r[4] = r[2];
    }
    block_reduce(r, lds);
    if (threadIdx.x == 0) {
        const int64_t nb = gridDim.x;
#pragma unroll
        for (int q = 0; q < NRED; ++q) partials[q * nb + blockIdx.x] = r[q];
    }
}

// One block: thread t adds partials t, t + 256, ... in that order, then the
// same block tree.  out is [NRED].
__global__ void __launch_bounds__(BLOCK)
k_md_reduce_final(const double* __restrict__ partials, double* __restrict__ out,
                  int64_t nb) {
    __shared__ double lds[WAVES][NRED];
    double r[NRED] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t j = threadIdx.x; j < nb; j += BLOCK) {
#pragma unroll
        for (int q = 0; q < NRED - 1; ++q) r[q] = r[q] + partials[q * nb + j];
        r[NRED - 1] = fmax(r[NRED - 1], partials[(NRED - 1) * nb + j]);
    }
    block_reduce(r, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < NRED; ++q) out[q] = r[q];
    }
}

int md_check(int64_t N, const char* msg_n) {
    // one block per 256 atoms on a 1-D grid
    if (N < 0 || N >= INT32_MAX) { dm_set_last_error(msg_n); return -1; }
    return 0;
}

int md_launched() {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        dm_set_last_error(hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

inline int md_blocks(int64_t N) { return (int)((N + BLOCK - 1) / BLOCK); }

}  // namespace

extern "C" {

int dm_md_kick_drift_f64(double* frac, double* vel, const void* force,
                         int32_t force_f64, const double* inv_mass,
                         const double* xi, double a, double b, double h,
                         double c1, double c2, const double* linv9,
                         const int32_t* pbc3, int64_t N, uint64_t stream) {
    if (int rc = md_check(N, "dm_md_kick_drift_f64: N out of range")) return rc;
    if (N == 0) return 0;
    if (!frac || !vel || !force || !linv9 || !pbc3) {
        dm_set_last_error("dm_md_kick_drift_f64: null argument");
        return -1;
    }
    MdCell cell;
    for (int k = 0; k < 9; ++k) cell.li[k] = linv9[k];
    for (int k = 0; k < 3; ++k) cell.per[k] = pbc3[k] ? 1 : 0;
    hipStream_t s = (hipStream_t)stream;
    const int nb = md_blocks(N);
#define DM_MD_KD(L, FT)                                                      \
    k_md_kick_drift<L, FT><<<nb, BLOCK, 0, s>>>(                             \
        frac, vel, (const FT*)force, inv_mass, xi, a, b, h, c1, c2, cell, N)
    if (xi) {
        if (force_f64) DM_MD_KD(true, double); else DM_MD_KD(true, float);
    } else {
        if (force_f64) DM_MD_KD(false, double); else DM_MD_KD(false, float);
    }
#undef DM_MD_KD
    return md_launched();
}

int dm_md_kick_reduce_f64(double* vel, const void* force, int32_t force_f64,
                          const double* inv_mass, double b, double* partials,
                          double* out5, int64_t N, uint64_t stream) {
    if (int rc = md_check(N, "dm_md_kick_reduce_f64: N out of range")) return rc;
    if (!out5 || (N > 0 && (!vel || !force || !partials))) {
        dm_set_last_error("dm_md_kick_reduce_f64: null argument");
        return -1;
    }
    hipStream_t s = (hipStream_t)stream;
    const int nb = md_blocks(N);
    if (nb > 0) {
#define DM_MD_KR(K, FT)                                                      \
    k_md_kick_reduce<K, FT><<<nb, BLOCK, 0, s>>>(                            \
        vel, (const FT*)force, inv_mass, b, partials, N)
        if (b != 0.0) {
            if (force_f64) DM_MD_KR(true, double); else DM_MD_KR(true, float);
        } else {
            if (force_f64) DM_MD_KR(false, double); else DM_MD_KR(false, float);
        }
#undef DM_MD_KR
    }
    k_md_reduce_final<<<1, BLOCK, 0, s>>>(partials, out5, (int64_t)nb);
    return md_launched();
}

}  // extern "C"
