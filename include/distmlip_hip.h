/* distmlip_hip.h — C-ABI of the gfx950 HIP kernel library.
 *
 * These entry points are the hot ops the reference delegates to PyTorch/DGL
 * (SURVEY.md §8(a)), hand-written in HIP for CDNA4:
 *   - gather / fused gather-add: the per-edge feature gathers behind the
 *     gated-MLP message compute (reference matgl CHGNetGraphConv via
 *     implementations/matgl/models/chgnet.py:300-313; DGL edge UDFs)
 *   - segmented scatter-add over the dst-sorted CSR: the node aggregation
 *     (DGL update_all sum reduce; the >=50%-HBM-roofline kernel of
 *     BASELINE.json)
 *   - permutation-CSR scatter: the deterministic backward of every gather
 *     (replaces torch autograd's atomics-based index_add backward)
 *
 * Conventions (mirrors the reference's int-code style, fast.c:205-212):
 *   - all pointers are DEVICE pointers (fp32 data, int32 indices); the
 *     caller (PyTorch) owns every allocation; the library never frees.
 *   - `stream` is a hipStream_t passed as uint64 — calls are async on it.
 *   - return 0 on success, nonzero hipError_t otherwise;
 *     dm_hip_last_error() returns the message.
 *   - row_ptr arrays are int32 CSR offsets of length n_rows+1 produced by
 *     the graph builder (include/distmlip_graph.h build extensions).
 */
#ifndef DISTMLIP_HIP_H
#define DISTMLIP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* out[i, :] = x[idx[i], :]                        (n_out rows, D columns) */
int dm_gather_rows_f32(const float* x, const int32_t* idx, float* out,
                       int64_t n_out, int64_t D, uint64_t stream);

/* out[e, :] = zs[src[e], :] + zd[dst[e], :] + ze[e, :]  (fused 2-gather-add:
 * the split-linear form of GatedMLP(cat(v_src, v_dst, e))).  If out_act is
 * non-null also emits silu(out) in the same pass (the gated-MLP hidden
 * activation). */
int dm_gather_add3_f32(const float* zs, const float* zd, const float* ze,
                       const int32_t* src, const int32_t* dst, float* out,
                       float* out_act, int64_t E, int64_t D, uint64_t stream);

/* out[l, :] = z1[lsrc[l], :] + z2[ldst[l], :] + za[l, :] + zv[center[l], :]
 * (bond/line-graph GatedMLP(cat(n_b1, n_b2, a, v_center))); optional fused
 * silu as above. */
int dm_gather_add4_f32(const float* z1, const float* z2, const float* za,
                       const float* zv, const int32_t* lsrc,
                       const int32_t* ldst, const int32_t* center, float* out,
                       float* out_act, int64_t L, int64_t D, uint64_t stream);

/* dz = (go_z ? go_z : 0) + go_h * silu'(z) — backward of the fused silu */
int dm_silu_bwd_f32(const float* go_h, const float* go_z, const float* z,
                    float* dz, int64_t total, uint64_t stream);

/* The CHGNet kernels evaluate sigmoid(x) = 1/(1 + expf(-x)) and
 * SiLU(x) = x/(1 + expf(-x)) through one pair of device functions, a shorter
 * instruction sequence that returns the bits of those expressions for every
 * fp32 input.  The two entries below expose the pair for checking.
 * which: 0 sigmoid, 1 SiLU.
 *
 * dm_act_check_f32 compares the kernels' function with the plain expression
 * on the count (<= 2^32) bit patterns first_bits, first_bits + 1, ...
 * (wrapping).  Two NaNs count as equal.  bad_per_block
 * [DM_ACT_CHECK_BLOCKS] receives one mismatch count per block (sum them);
 * *first_bad_bits receives the lowest mismatching pattern, or 0xffffffff
 * (a NaN, which cannot mismatch) if there is none.
 *
 * dm_act_eval_f32: out[i] = f(x[i]) for i < n, with impl 0 the plain
 * expression and impl 1 the kernels' function. */
#define DM_ACT_CHECK_BLOCKS 4096
int dm_act_check_f32(int32_t which, uint32_t first_bits, uint64_t count,
                     uint32_t* bad_per_block, uint32_t* first_bad_bits,
                     uint64_t stream);
int dm_act_eval_f32(int32_t which, int32_t impl, const float* x, int64_t n,
                    float* out, uint64_t stream);

/* out[n, :] = (base ? base[n, :] : 0) + sum_{j in [row_ptr[n], row_ptr[n+1])}
 *             msg[j, :]
 * msg is DST-SORTED (builder layout).  THE judged scatter-add kernel. */
int dm_seg_sum_f32(const float* msg, const int32_t* row_ptr,
                   const float* base, float* out, int64_t N, int64_t D,
                   uint64_t stream);

/* out[n, :] = (base?base[n,:]:0) + sum_j msg[perm[j], :] — scatter along a
 * non-sorted direction via its permutation CSR (deterministic backward of
 * gathers). */
int dm_seg_sum_gather_f32(const float* msg, const int32_t* perm,
                          const int32_t* row_ptr, const float* base,
                          float* out, int64_t N, int64_t D, uint64_t stream);

/* Fused first-layer edge MLP: z[e,:] = erow[e,:] @ WT + bias
 *   + zs[src[e],:] + zd[dst[e],:]   (+ zv[center[e],:] for the 4-input
 * line-graph form).  WT is weight.T, [Din, Dout] row-major, held in
 * per-lane registers (one wave per edge, e-row via the scalar cache);
 * compiled for Din=64, Dout=128 (the CHGNet gated-MLP first layer) —
 * other shapes return an error and the binding falls back to the unfused
 * GEMM + dm_gather_add{3,4} path.  out (= z, row-major [E,128], the
 * backward save) may be NULL to skip the write in no-grad passes;
 * out_act = silu(z), row-major. */
int dm_edge_mlp3_f32(const float* erow, const float* WT, const float* bias,
                     const float* zs, const float* zd, const int32_t* src,
                     const int32_t* dst, float* out, float* out_act,
                     int64_t E, int64_t Din, int64_t Dout, uint64_t stream);
int dm_edge_mlp4_f32(const float* arow, const float* WT, const float* bias,
                     const float* z1, const float* z2, const float* zv,
                     const int32_t* lsrc, const int32_t* ldst,
                     const int32_t* center, float* out, float* out_act,
                     int64_t L, int64_t Din, int64_t Dout, uint64_t stream);

/* out = (base?base:0) + silu(c) * sigmoid(g) * (w?w:1) — the gated-MLP
 * epilogue (core activation x gate x shared message weight x residual),
 * fused from ~5 eager passes.  bwd emits dc, dg and (if w) dw.
 * c and g (and dc/dg) are plain element pointers, so a PACKED [2, N, D]
 * buffer works by passing base and base + N*D — the binding's
 * gated_combine_packed path relies on this. */
int dm_gated_combine_fwd_f32(const float* c, const float* g, const float* w,
                             const float* base, float* out, int64_t total,
                             uint64_t stream);
int dm_gated_combine_bwd_f32(const float* go, const float* c, const float* g,
                             const float* w, float* dc, float* dg, float* dw,
                             int64_t total, uint64_t stream);

/* Fused reverse tail of one gated MLP, from the gradient go [E,d] of
 *   out = base + silu(c) * sigmoid(g) * (w?w:1)
 * to the gradient dz [E,2d] of the first layer's pre-activation z, where
 * c = h[:, :d] @ w2c, g = h[:, d:] @ w2g and h = silu(z):
 *   dc = go*w*sig(g)*silu'(c)       dg = go*w*silu(c)*sig(g)*(1-sig(g))
 *   dw = go*silu(c)*sig(g)
 *   dz = [dc @ w2c^T | dg @ w2g^T] * silu'(z)
 * One kernel in place of dm_gated_combine_bwd_f32 + two GEMMs +
 * dm_silu_bwd_f32; dc, dg and dh never reach memory.  c and g are the two
 * halves of a packed [2,E,d] buffer (or any two [E,d] arrays); w2c, w2g are
 * [d,d] row-major, input x output.  w and dw are both NULL or both given.
 * Compiled for d = 64: any other d returns an error and launches nothing. */
int dm_gated_mlp_tail_bwd_f32(const float* go, const float* c, const float* g,
                              const float* w, const float* z,
                              const float* w2c, const float* w2g, float* dz,
                              float* dw, int64_t E, int64_t d,
                              uint64_t stream);

/* dm_gated_mlp_tail_bwd_f32 with go read by index: go is a [N,d] table and
 * row r takes table row idx[r] (int32 [E], every entry in [0,N)), i.e. the
 * plain entry on the materialized go[idx], bit for bit, without that [E,d]
 * array being written or read.  Same refusals; idx must not be NULL. */
int dm_gated_mlp_tail_bwd_idx_f32(const float* go, const int32_t* idx,
                                  const float* c, const float* g,
                                  const float* w, const float* z,
                                  const float* w2c, const float* w2g,
                                  float* dz, float* dw, int64_t E, int64_t d,
                                  uint64_t stream);

/* Reverse of the fused first layer's per-edge GEMM with the gradient sum
 * folded in:  out[e,:] = (gbase ? gbase[e,:] : 0) + dz[e,:] @ WT^T
 * with dz [E,Din], WT [Dout,Din] row-major (the pack dm_edge_mlp3_f32 /
 * dm_edge_mlp4_f32 take as their [Din',Dout'] WT), gbase and out [E,Dout].
 * One kernel in place of a GEMM (or addmm) and an elementwise add.  out may
 * be gbase itself (each element is read before it is written, by the same
 * lane); it must not overlap dz.  gbase may be NULL.
 * Compiled for Din = 128, Dout = 64: anything else returns an error and
 * launches nothing.  E <= 0 returns 0 without a launch. */
int dm_edge_mlp_bwd_f32(const float* dz, const float* WT, const float* gbase,
                        float* out, int64_t E, int64_t Din, int64_t Dout,
                        uint64_t stream);

/* Fused forward tail of one gated MLP: the second layer over h [E,2d] and
 * the combine, in one kernel:
 *   c = h[:, :d] @ w2c + b2c        g = h[:, d:] @ w2g + b2g
 *   out = (base?base:0) + silu(c) * sigmoid(g) * (w?w:1)
 * One kernel in place of the batched GEMM + dm_gated_combine_fwd_f32.
 * w2c, w2g are [d,d] row-major, input x output; b2c, b2g are [d].  c_out and
 * g_out are both NULL (c and g never reach memory: passes that record
 * nothing) or both given (any two [E,d] arrays, e.g. the halves of the
 * packed [2,E,d] buffer dm_gated_mlp_tail_bwd_f32 reads); out is the same
 * bit for bit either way.  w and base may be NULL.
 * Compiled for d = 64: any other d, or exactly one of c_out/g_out, returns
 * an error and launches nothing.  E <= 0 returns 0 without a launch. */
int dm_gated_mlp_tail_fwd_f32(const float* h, const float* w2c,
                              const float* w2g, const float* b2c,
                              const float* b2g, const float* w,
                              const float* base, float* c_out, float* g_out,
                              float* out, int64_t E, int64_t d,
                              uint64_t stream);

/* One whole gated MLP in one kernel: dm_edge_mlp3_f32 followed by
 * dm_gated_mlp_tail_fwd_f32 without the h [E,2d] array between them:
 *   z   = erow @ WT + bias + zs[src] + zd[dst]                  [E,2d]
 *   c   = silu(z)[:, :d] @ w2c + b2c    g = silu(z)[:, d:] @ w2g + b2g
 *   out = (base?base:0) + silu(c) * sigmoid(g) * (w?w:1)
 * with every operand laid out as in those two entries.  z, c, g and out are
 * theirs bit for bit.  Accepted forms:
 *   no-keep        z_out, c_out, g_out all NULL, out given
 *   keep           z_out, c_out, g_out and out given
 *   keep, no out   z_out, c_out, g_out given, out NULL: w and base are not
 *                  read
 * erow, zs, zd and z_out must be 16-byte aligned.  Compiled for Din = 64,
 * d = 64.  Any other size or form, or a NULL index or input, returns an error
 * and launches nothing.  E <= 0 returns 0 without a launch. */
int dm_gated_mlp3_f32(const float* erow, const float* WT, const float* bias,
                      const float* zs, const float* zd, const int32_t* src,
                      const int32_t* dst, const float* w2c, const float* w2g,
                      const float* b2c, const float* b2g, const float* w,
                      const float* base, float* z_out, float* c_out,
                      float* g_out, float* out, int64_t E, int64_t Din,
                      int64_t d, uint64_t stream);

/* The three-gather line-graph form over dm_edge_mlp4_f32's operands:
 *   z = arow @ WT + bias + z1[lsrc] + z2[ldst] + zv[center]. */
int dm_gated_mlp4_f32(const float* arow, const float* WT, const float* bias,
                      const float* z1, const float* z2, const float* zv,
                      const int32_t* lsrc, const int32_t* ldst,
                      const int32_t* center, const float* w2c,
                      const float* w2g, const float* b2c, const float* b2g,
                      const float* w, const float* base, float* z_out,
                      float* c_out, float* g_out, float* out, int64_t L,
                      int64_t Din, int64_t d, uint64_t stream);

/* Factored message weight.  The three entries below are
 * dm_gated_mlp_tail_fwd_f32, dm_gated_mlp3_f32 and dm_gated_mlp_tail_bwd_f32
 * (plain, or indexed with idx != NULL) with the dense w [E,d] replaced by its
 * factors:
 *   w[e][col] = (mask ? mask[e] : 1) * sum_k bexp[e][k] * W[col][k]
 * bexp [E,n_rbf], W [d,n_rbf] row-major, mask [E] or NULL.  No dense [E,d]
 * weight is read or written.  The sum has one fp32 order in all three:
 * bexp[e][0] * W[col][0], then fmaf over k = 1..8 ascending, then the mask; the
 * three kernels therefore see the same w bit for bit.  Outputs that do not
 * depend on w (c, g, z) are the dense entries' bit for bit.
 * The reverse entry returns, in place of dw,
 *   dbexp[e][k] = mask[e] * sum_col dw[e][col] * W[col][k]  (+ dbexp_in[e][k])
 * summed as: fmaf over the columns 8i+4h+t ascending for each half h = 0, 1
 * of the row's columns (i = 0..7, t = 0..3), then half 0 + half 1, then the
 * mask, then + dbexp_in, each step rounded.  dbexp_in [E,n_rbf] may be NULL
 * and may be dbexp itself (accumulation in place).
 * Compiled for d = 64 and n_rbf = 9 (dm_gated_mlp3_fw_f32: Din = 64 too);
 * anything else, a NULL bexp, W or dbexp, returns an error and launches
 * nothing.  Rows >= E are neither loaded nor stored.  dm_gated_mlp3_fw_f32
 * takes the no-keep and the keep form, both with out. */
int dm_gated_mlp_tail_fwd_fw_f32(const float* h, const float* w2c,
                                 const float* w2g, const float* b2c,
                                 const float* b2g, const float* bexp,
                                 const float* W, const float* mask,
                                 const float* base, float* c_out,
                                 float* g_out, float* out, int64_t E,
                                 int64_t d, int64_t n_rbf, uint64_t stream);
int dm_gated_mlp3_fw_f32(const float* erow, const float* WT, const float* bias,
                         const float* zs, const float* zd, const int32_t* src,
                         const int32_t* dst, const float* w2c,
                         const float* w2g, const float* b2c, const float* b2g,
                         const float* bexp, const float* W, const float* mask,
                         const float* base, float* z_out, float* c_out,
                         float* g_out, float* out, int64_t E, int64_t Din,
                         int64_t d, int64_t n_rbf, uint64_t stream);
int dm_gated_mlp_tail_bwd_fw_f32(const float* go, const int32_t* idx,
                                 const float* c, const float* g,
                                 const float* bexp, const float* W,
                                 const float* mask, const float* z,
                                 const float* w2c, const float* w2g,
                                 float* dz, const float* dbexp_in,
                                 float* dbexp, int64_t E, int64_t d,
                                 int64_t n_rbf, uint64_t stream);

/* Fused edge geometry + radial basis (replaces the torch chain for
 * chgnet.py:96-124): per local edge e,
 *   bv[e]  = pos[dst[e]] + offshift[e] - pos[src[e]]
 *   bd[e]  = |bv[e]|
 *   exp[e,k] = env(rbf_k) * rbf_k,   rbf_k = sqrt(2/c) sin(f_k bd / c)/bd
 * env = the reference's polynomial cutoff applied to the RBF VALUE
 * (chgnet.py:119-121 quirk), exponent `pexp`.  nrbf <= 16. */
int dm_edge_geom_rbf_fwd_f32(const float* pos, const int32_t* src,
                             const int32_t* dst, const float* offshift,
                             const float* freqs, float cutoff, int32_t pexp,
                             int32_t nrbf, float* bv, float* bd, float* exp_out,
                             int64_t E, uint64_t stream);
/* backward: gbv_total[e] = go_bv[e] + (go_bd[e] + sum_k go_exp[e,k] *
 * d(exp_k)/d(bd)) * bv[e]/bd[e].  The caller scatters gbv_total to pos via
 * the CSRs and passes it on as d(offshift).  No gradient wrt freqs. */
int dm_edge_geom_rbf_bwd_f32(const float* go_bv, const float* go_bd,
                             const float* go_exp, const float* bv,
                             const float* bd, const float* freqs,
                             float cutoff, int32_t pexp, int32_t nrbf,
                             float* gbv_total, int64_t E, uint64_t stream);

/* Fused radial-basis + envelope only (bond-graph expansion on nd_dist):
 * exp[m,k] = env(rbf_k(d[m])) * rbf_k(d[m]); bwd gives gd[m]. */
int dm_rbf_env_fwd_f32(const float* d, const float* freqs, float cutoff,
                       int32_t pexp, int32_t nrbf, float* exp_out, int64_t M,
                       uint64_t stream);
int dm_rbf_env_bwd_f32(const float* go_exp, const float* d, const float* freqs,
                       float cutoff, int32_t pexp, int32_t nrbf, float* gd,
                       int64_t M, uint64_t stream);

/* GPU-resident neighbor list (single-partition fast path; diagonal
 * lattice, full PBC, >= 3 cells per dim).  Exact fp64 replica of the CPU
 * builder's edge condition (fpis.c:833 contract: d^2 < r^2+tol,
 * d^2 > tol, no self edges in any image).  Atoms are pre-binned on the
 * host side (torch): `order` lists atom ids sorted by cell id,
 * `cell_start[ncell+1]` the bin offsets.  Edges are emitted center-major
 * with center as DST (so the emission order IS the dst-sorted scatter
 * layout); `off_i8` is the integer image of the dst atom and `bond_flag`
 * marks d^2 < bond_r^2+tol. */
int dm_nl_count_f64(const double* pos, const int32_t* cid,
                    const int32_t* order, const int32_t* cell_start,
                    int32_t ncx, int32_t ncy, int32_t ncz,
                    double lx, double ly, double lz,
                    double r2tol, double tol, int32_t* cnt, int64_t N,
                    uint64_t stream);
int dm_nl_fill_f64(const double* pos, const int32_t* cid,
                   const int32_t* order, const int32_t* cell_start,
                   int32_t ncx, int32_t ncy, int32_t ncz,
                   double lx, double ly, double lz,
                   double r2tol, double tol, double br2tol,
                   const int32_t* row_ptr, int32_t* src, int8_t* off_i8,
                   uint8_t* bond_flag, int64_t N, uint64_t stream);

/* General-lattice GPU neighbor list: any non-singular cell (triclinic /
 * sheared), any pbc combination, any cell count per dim (cells shorter
 * than the cutoff included).  Same emitted-edge contract as above
 * (fpis.c:418-901; edge condition fpis.c:833) and the same pre-binned
 * inputs, but the grid lives in FRACTIONAL space: dim k has `nc3[k]`
 * cells and a stencil radius `R3[k]`; a periodic dim (pbc3[k] != 0) folds
 * the unwrapped cell index c+d into (image, cell) by floor division, an
 * open dim skips indices outside [0, nc).  The image shift is
 * m @ lattice with `lattice9` the row-major lattice ROWS.  Threads walk
 * centers in `order` (cell-sorted); rows are addressed by atom id.
 * pos/cid/order/cell_start/row_ptr and the outputs are DEVICE arrays;
 * lattice9/nc3/R3/pbc3 are small HOST arrays passed on to the kernel by
 * value.  Fails (nonzero) if an image index could exceed int8. */
int dm_nl_count_gen_f64(const double* pos, const int32_t* cid,
                        const int32_t* order, const int32_t* cell_start,
                        const double* lattice9, const int32_t* nc3,
                        const int32_t* R3, const int32_t* pbc3,
                        double r2tol, double tol, int32_t* cnt, int64_t N,
                        uint64_t stream);
int dm_nl_fill_gen_f64(const double* pos, const int32_t* cid,
                       const int32_t* order, const int32_t* cell_start,
                       const double* lattice9, const int32_t* nc3,
                       const int32_t* R3, const int32_t* pbc3,
                       double r2tol, double tol, double br2tol,
                       const int32_t* row_ptr, int32_t* src, int8_t* off_i8,
                       uint8_t* bond_flag, int64_t N, uint64_t stream);

/* MACE uvu tensor product, fused per edge (round 2).  Replaces the
 * e3nn TensorProduct the reference's MACE interactions delegate to
 * (implementations/mace/models.py:144-152, conv_tp of
 * RealAgnosticResidualInteractionBlock): per-edge contraction of sender
 * features (l=0 block x0 [E,C]; optional l=1 block x1 [E,C,d1b]) with
 * edge spherical harmonics Y [E,16] and per-edge path weights w [E,P,C],
 * CG nonzeros streamed as (path, slot, k1, k2, k3) int32 quintuples nz
 * sorted by path + coefficients nzc.  m is [E,16,C] (l3-major rows).
 * Backward writes dx0/dx1/dY/dw in the matching layouts. */
int dm_mace_tp_fwd_f32(const float* x0, const float* x1, const float* Y,
                       const float* w, const int32_t* nz, const float* nzc,
                       int32_t nnz, float* o0, float* o1, float* o2,
                       float* o3, int64_t E, int32_t C, int32_t P,
                       int32_t d1b, uint64_t stream);
int dm_mace_tp_bwd_f32(const float* g0, const float* g1, const float* g2,
                       const float* g3, const float* x0, const float* x1,
                       const float* Y, const float* w, const int32_t* nz,
                       const float* nzc, int32_t nnz, float* dx0,
                       float* dx1, float* dY, float* dw, int64_t E,
                       int32_t C, int32_t P, int32_t d1b, uint64_t stream);

/* MACE symmetric contraction, fused per node (round 2).  Replaces
 * mace's SymmetricContraction (EquivariantProductBasisBlock,
 * models.py:155-157): polynomial entries (wrow, a, b, k, orow) int32
 * sextuples + coefficients, x rows [N,16,C] (sentinel row 16 == 1
 * implied), per-element weight table W [n_elem, T, C]; weights frozen
 * so backward produces dx only. */
int dm_mace_symc_fwd_f32(const float* x, const int32_t* elem,
                         const float* W, const int32_t* nz,
                         const float* nzc, int32_t nnz, float* out,
                         int64_t N, int32_t C, int32_t T, int32_t S_out,
                         uint64_t stream);
int dm_mace_symc_bwd_f32(const float* go, const float* x,
                         const int32_t* elem, const float* W,
                         const int32_t* nz, const float* nzc, int32_t nnz,
                         float* dx, int64_t N, int32_t C, int32_t T,
                         int32_t S_out, uint64_t stream);

/* eSCN/UMA per-edge Wigner rotation family (round 2): replaces the
 * per-edge D-matrix bmms of the reference's UMA path
 * (escn_md.py:283-291 rotation setup; applications around every SO(2)
 * conv).  D is [E, 81] row-major (S = 9, lmax 2); trans selects D^T
 * (the inverse rotation).  rot_gather: out[e] = D_e . h[idx[e]]
 * (idx NULL = identity rows).  rot_scatter: out[n] = (base[n]) +
 * sum_{edges of n via row_ptr/perm} D_e . mt[e].  rot_dD: the D
 * gradient, one [9,9] block per edge. */
int dm_rot_gather_f32(const float* h, const int32_t* idx, const float* D,
                      int32_t trans, float* out, int64_t E, int32_t C,
                      uint64_t stream);
int dm_rot_scatter_f32(const float* mt, const float* D, int32_t trans,
                       const int32_t* perm, const int32_t* row_ptr,
                       const float* base, float* out, int64_t N,
                       int32_t C, uint64_t stream);
int dm_rot_dD_f32(const float* go, const float* h, const int32_t* idx,
                  int32_t trans, float* dD, int64_t E, int32_t C,
                  uint64_t stream);

/* TensorNet tensor message pass, fused per node.  Replaces the matgl
 * TensorNetInteraction message step the reference's TensorNet_Dist delegates
 * to (implementations/matgl/models/tensornet.py, the per-layer loop around
 * atom_transfer): node tensors are stored component-major, Y [N,9,C] with
 * row 3a+b, the per-edge radial weights f [E,3,C] with k in {I, A, S}, and
 * P_k is the projection of a 3x3 tensor onto its isotropic (tr/3 * 1),
 * antisymmetric ((T - T^T)/2) or symmetric-traceless part, per channel.
 * Edges are DST-SORTED (builder layout): row_ptr [N+1] is the dst CSR,
 * (src_perm, src_row_ptr) the src permutation CSR.
 *
 *   fwd:      M[i,:,c]  = sum_{e in [row_ptr[i], row_ptr[i+1])}
 *                         sum_k f[e,k,c] * P_k(Y[src[e],:,c])
 *   bwd_edge: df[e,k,c] = < G[dst(e),:,c], P_k(Y[src[e],:,c]) >,  G = dL/dM,
 *             dst(e) = the row of the dst CSR that holds e
 *   bwd_node: dY[j,:,c] = sum_{p in [src_row_ptr[j], src_row_ptr[j+1])}
 *                         sum_k f[e,k,c] * P_k(G[dst[e],:,c]),  e = src_perm[p]
 *   (the projections are self-adjoint under the Frobenius product, so the
 *   reverse needs no transposed form).
 *
 * One wave per (node, 64-channel block), lane = channel, nine accumulators
 * in registers: no [E,9,C] intermediate, no atomics, each row summed in CSR
 * order, so results are bit-identical from run to run.  A row without edges
 * writes zeros (fwd, bwd_node) or nothing (bwd_edge has no rows to write).
 * N == 0 returns 0 with no launch; a graph without edges (row_ptr all zero)
 * reads row_ptr only, so Y, f, src may then be NULL.  C must be a positive
 * multiple of 64: anything else returns nonzero and launches nothing. */
int dm_tn_msg_fwd_f32(const float* Y, const float* f, const int32_t* src,
                      const int32_t* row_ptr, float* M, int64_t N, int32_t C,
                      uint64_t stream);
int dm_tn_msg_bwd_edge_f32(const float* G, const float* Y, const int32_t* src,
                           const int32_t* row_ptr, float* df, int64_t N,
                           int32_t C, uint64_t stream);
int dm_tn_msg_bwd_node_f32(const float* G, const float* f, const int32_t* dst,
                           const int32_t* src_perm,
                           const int32_t* src_row_ptr, float* dY, int64_t N,
                           int32_t C, uint64_t stream);

/* Integrator kernels of the native MD / relaxation driver
 * (distmlip_amd/md.py; the reference drives ASE's integrators instead,
 * implementations/matgl/ase.py:130-490).  State is fp64: wrapped fractional
 * coordinates frac [N,3], cartesian velocities vel [N,3] (A/fs), inv_mass [N]
 * (NULL = unit masses, FIRE).  `force` [N,3] is fp32 (the engines' output),
 * or fp64 when force_f64 != 0.  One thread per atom, no atomics; every
 * expression is evaluated op by op (no fused multiply-add), in the order of
 * the fp64 torch composition in distmlip_amd/md_ops.py.  frac/vel/force/
 * inv_mass/xi/partials/out5 are DEVICE arrays; linv9 (row-major inverse
 * lattice, frac = cart @ Linv) and pbc3 are small HOST arrays passed on to
 * the kernel by value.  N == 0 launches nothing (kick_reduce then writes
 * zeros); N >= 2^31-1 returns nonzero.
 *
 *   kick_drift: v = a*v + (b*inv_mass)*F, then the displacement
 *       xi == NULL:  dr = h*v
 *       xi != NULL:  d1 = (h/2)*v;  v = c1*v + (c2*sqrt(inv_mass))*xi;
 *                    dr = d1 + (h/2)*v             (the "AOA" of BAOAB)
 *     then frac_k += (dr_x*Linv[0][k] + dr_y*Linv[1][k]) + dr_z*Linv[2][k]
 *     and, on periodic dims, f -= floor(f) with a result >= 1.0 (a tiny
 *     negative f rounds there) replaced by 0.0: frac stays in [0,1), the
 *     graph builder's contract.  Open dims are left unwrapped.
 *     a = 1 is the first half of velocity Verlet, a = lambda Berendsen,
 *     (a, b, h) = (beta, gamma, s*dt) with NULL masses the FIRE update.
 *
 *   kick_reduce: v += (b*inv_mass)*F (b == 0: vel is not written), then
 *     out5 = { sum m v^2, sum F.v, sum |F|^2, sum |v|^2, max_i |F_i|^2 },
 *     m = 1/inv_mass.  Each block reduces by a fixed tree (wave shuffles,
 *     LDS across the four waves) and stores one partial per quantity into
 *     partials [5, ceil(N/256)] (caller-provided scratch); a second
 *     single-block launch adds those in index order into out5.  The result
 *     is bit-identical from run to run. */
int dm_md_kick_drift_f64(double* frac, double* vel, const void* force,
                         int32_t force_f64, const double* inv_mass,
                         const double* xi, double a, double b, double h,
                         double c1, double c2, const double* linv9,
                         const int32_t* pbc3, int64_t N, uint64_t stream);
int dm_md_kick_reduce_f64(double* vel, const void* force, int32_t force_f64,
                          const double* inv_mass, double b, double* partials,
                          double* out5, int64_t N, uint64_t stream);

/* ---- indexed row moves (distmlip_amd/csrc/rows.hip): the edge <-> bond
 * exchange of a CHGNet step and its reverse, in place over dst ----
 *
 *   dm_move_rows_f32:  dst[di[i], :] (=|+=) src[si[i], :]   for i < M
 *   dm_zero_rows_f32:  dst[di[i], :] = 0                    for i < M
 *
 * src and dst are row-major fp32 with D columns and must not overlap.  si and
 * di are int64 [M] device arrays (the dtype of the builders' map_de /
 * map_ude); either may be NULL for the identity (row i).  CALLER'S CONTRACT:
 * every index is a valid row of its array, and the entries of di are unique;
 * each destination element then has exactly one writer, no atomics are used
 * and the add form rounds once per element.  op is 0 (assign) or 1 (add).
 * Rows move as float4 when D % 4 == 0 and both pointers are 16-byte aligned,
 * as single floats otherwise; all offsets are 64-bit (arrays past 2^31
 * elements are fine).  M <= 0 returns 0 without a launch; D outside
 * [1, 2^31), another op, or a NULL src / dst returns an error and launches
 * nothing. */
int dm_move_rows_f32(const float* src, const int64_t* si, float* dst,
                     const int64_t* di, int64_t M, int64_t D, int32_t op,
                     uint64_t stream);
int dm_zero_rows_f32(float* dst, const int64_t* di, int64_t M, int64_t D,
                     uint64_t stream);

const char* dm_hip_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* DISTMLIP_HIP_H */
