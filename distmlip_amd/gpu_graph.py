"""GPU-resident graph construction: cell-list neighbor
search on the GPU (fp64, exact replica of the CPU builder's edge
condition) + bond/line graph assembly with torch GPU primitives.  Removes
the per-step CPU rebuild + H2D of graph arrays.

Two neighbor-list kernels share the pipeline (dispatch: `fast_scope`):

  * fast path (`dm_nl_*_f64`): diagonal lattice, full PBC, >= 3 cells of
    >= cutoff per dim — every BASELINE workload;
  * general path (`dm_nl_*_gen_f64`): any non-singular lattice (triclinic,
    sheared), any pbc combination, any box size, cells shorter than the
    cutoff included.  The grid lives in fractional space (`cell_plan`).

Scope guard (`supported`): False — the engines then fall back to the
native CPU builder — only for a singular lattice, a cell so short that an
image index would leave the int8 range of `off_i8`, a periodic fractional
coordinate outside [0, 1) (wrapped coordinates are the builder contract),
or an N / expected E beyond int32.
"""
from __future__ import annotations

import ctypes
from ctypes import POINTER, c_double, c_int32, c_int64, c_uint64

import numpy as np
import torch


class GpuPD:
    """PartitionData-compatible index bundle, built on-device."""

    @property
    def line_src_csr(self):
        return (self.line_src_perm, self.line_src_row_ptr)

    @property
    def line_dst_csr(self):
        return (None, self.line_row_ptr)


INT32_MAX = 2 ** 31 - 1
# cell_start stays O(N) for a sparse, huge box
MAX_CELLS_PER_ATOM = 8
MIN_CELL_CAP = 4096


def fast_scope(lattice, pbc, cutoff: float) -> bool:
    """Dispatch predicate: True routes to the diagonal `dm_nl_*_f64`
    kernels (diagonal lattice, full PBC, >= 3 cells of >= cutoff per
    dim), False to the general `dm_nl_*_gen_f64` pair."""
    lat = np.asarray(lattice)
    if not np.allclose(lat, np.diag(np.diag(lat)), atol=1e-12):
        return False
    if not all(int(x) for x in pbc):
        return False
    d = np.diag(lat)
    return bool((d // cutoff >= 3).all())


def cell_heights(lattice) -> np.ndarray:
    """h_k = 1 / |column k of L^-1|: perpendicular height of the cell
    along lattice vector k (|d frac_k| <= |d cart| / h_k)."""
    inv = np.linalg.inv(np.asarray(lattice, dtype=np.float64))
    return 1.0 / np.linalg.norm(inv, axis=0)


def cell_plan(lattice, pbc, frac, cutoff: float, tol: float = 1e-8,
              max_cells=None):
    """Fractional-space cell grid of the general neighbor list (pure
    numpy).  Returns (nc, R, origin, span), int64[3] / int64[3] /
    float64[3] / float64[3].

    Dim k spans [origin_k, origin_k + span_k] in fractional coordinates:
    the unit interval if periodic, the atoms' extent if open.  With
    rc = sqrt(cutoff^2 + tol) and h_k the perpendicular cell height,
    nc_k = max(1, floor(span_k h_k / rc)) cells of perpendicular width
    w_k = span_k h_k / nc_k, and the stencil reaches
    R_k = ceil(rc / w_k) cells (1 whenever the dim holds a full cutoff).
    An edge has |d frac_k| <= d / h_k < rc / h_k <= R_k cells, so the
    unwrapped cells of its end points differ by at most R_k.  `max_cells`
    caps prod(nc) by shrinking nc (bigger cells: R stays valid)."""
    pbc = [bool(int(x)) for x in pbc]
    frac = np.asarray(frac, dtype=np.float64).reshape(-1, 3)
    h = cell_heights(lattice)
    rc = float(np.sqrt(cutoff * cutoff + tol))
    origin = np.zeros(3)
    span = np.ones(3)
    for k in range(3):
        if not pbc[k] and len(frac):
            lo, hi = float(frac[:, k].min()), float(frac[:, k].max())
            origin[k], span[k] = lo, hi - lo
    nc = np.ones(3, dtype=np.int64)
    R = np.zeros(3, dtype=np.int64)
    for k in range(3):
        ext = span[k] * h[k]
        nc[k] = max(1, int(np.floor(ext / rc)))
        if ext > 0.0:
            R[k] = int(np.ceil(rc / (ext / nc[k])))
        if not pbc[k]:
            R[k] = min(R[k], nc[k] - 1)     # cells outside [0, nc) are skipped
    if max_cells is not None:
        while int(nc.prod()) > max_cells:
            f = (max_cells / float(nc.prod())) ** (1.0 / 3.0)
            new = np.maximum(1, np.floor(nc * f).astype(np.int64))
            if (new == nc).all():
                new[int(np.argmax(nc))] -= 1
            nc = new
        for k in range(3):
            if not pbc[k]:
                R[k] = min(R[k], nc[k] - 1)
    return nc, R, origin, span


def cell_index(frac, nc, origin, span) -> np.ndarray:
    """int64[N,3] cell of each atom under a `cell_plan` grid — the numpy
    twin of the binning `build` does on the device."""
    frac = np.asarray(frac, dtype=np.float64).reshape(-1, 3)
    out = np.empty(frac.shape, dtype=np.int64)
    for k in range(3):
        scale = nc[k] / span[k] if span[k] > 0.0 else 0.0
        out[:, k] = np.clip(np.floor((frac[:, k] - origin[k]) * scale),
                            0, nc[k] - 1).astype(np.int64)
    return out


def _cell_cap(n_atoms: int) -> int:
    return max(MIN_CELL_CAP, MAX_CELLS_PER_ATOM * int(n_atoms))


def supported(structure, cutoff: float, tol: float = 1e-8,
              frac=None) -> bool:
    """True when the GPU builder handles `structure`; see the module
    docstring for the fallback conditions.  `frac` overrides
    structure.frac_coords (the coordinates the build will bin)."""
    lat = np.asarray(structure.lattice, dtype=np.float64)
    pbc = [bool(int(x)) for x in structure.pbc]
    if fast_scope(lat, pbc, cutoff):         # the fast path's own guard
        return True
    # singular lattice: the CPU builder's guard (graph_build.cpp)
    if lat.shape != (3, 3) or not np.isfinite(lat).all() \
            or abs(np.linalg.det(lat)) < 1e-12:
        return False
    frac = np.asarray(structure.frac_coords if frac is None else frac,
                      dtype=np.float64)
    N = len(frac)
    if N == 0 or N >= INT32_MAX or not np.isfinite(frac).all():
        return False
    for k in range(3):
        if pbc[k] and (frac[:, k].min() < 0.0 or frac[:, k].max() >= 1.0):
            return False
    nc, R, _, span = cell_plan(lat, pbc, frac, cutoff, tol)
    # image index: |m_k| <= ceil(R_k / nc_k) must fit off_i8
    for k in range(3):
        if pbc[k] and -(-int(R[k]) // int(nc[k])) > 127:
            return False
    # expected E = N * density * cutoff sphere; an open dim thinner than
    # the sphere counts as 2 rc thick (the sphere sticks out of the slab)
    h = cell_heights(lat)
    rc = float(np.sqrt(cutoff * cutoff + tol))
    vol = abs(np.linalg.det(lat))
    for k in range(3):
        if not pbc[k]:
            vol *= max(span[k], 2.0 * rc / h[k])
    e_est = N * (N / vol) * (4.0 / 3.0) * np.pi * rc ** 3
    return bool(2.0 * e_est < INT32_MAX)


def engages(structure, cutoff: float, mode: str, tol: float = 1e-8,
            frac=None) -> bool:
    """The engines' `gpu_build` switch: "auto" — anything supported();
    "fast" — only the diagonal fast-path scope (the pre-general-lattice
    behaviour); "off" — never."""
    if mode == "auto":
        return supported(structure, cutoff, tol, frac=frac)
    if mode == "fast":
        return fast_scope(structure.lattice, structure.pbc, cutoff)
    if mode == "off":
        return False
    raise ValueError(f"gpu_build must be 'auto', 'fast' or 'off', "
                     f"got {mode!r}")


def _csr_of(idx_sorted_key: torch.Tensor, n_rows: int, device):
    rp = torch.zeros(n_rows + 1, dtype=torch.int64, device=device)
    rp[1:] = torch.bincount(idx_sorted_key, minlength=n_rows)
    return torch.cumsum(rp, 0).to(torch.int32)


WALL_EPSILON = 1e-10


def compute_walls_home(frac_np, lattice_np, P, cutoff, bond_cutoff,
                       use_bond_graph):
    """Replicates graph_build.cpp:compute_walls / Walls::which exactly
    (fp64 expression order preserved): returns (dim, walls[P-1],
    home[N]) as numpy.  Global by construction — every rank computes the
    same walls (the cross-rank halo alignment requirement)."""
    frac = np.asarray(frac_np, dtype=np.float64)
    lat = np.asarray(lattice_np, dtype=np.float64)
    if P <= 1:
        return 0, np.zeros(0), np.zeros(len(frac), dtype=np.int32)
    # reference quirk: partition dim from cart = L . frac (lattice rows
    # dotted with frac — the TRANSPOSE of cart = frac @ L)
    c = frac @ lat.T
    ext = c.max(0) - c.min(0)
    dim = int(np.argmax(ext))
    x = frac[:, dim]
    fmin, fmax = float(x.min()), float(x.max())
    flen = fmax - fmin
    walls = np.array([i * (flen / P) + WALL_EPSILON + fmin
                      for i in range(1, P)], dtype=np.float64)
    while True:
        hit = False
        for wi in range(P - 1):
            if (x == walls[wi]).any():
                print("Collision b/w atom and partition wall, moving wall.",
                      flush=True)
                walls[wi] += WALL_EPSILON
                hit = True
        if not hit:
            break
    # width check norm: lattice COLUMN dim (graph_build.cpp lv[] indices —
    # consistent with the transposed-cart quirk above)
    vnorm = float(np.linalg.norm(lat[:, dim]))
    width = float(walls[0]) * vnorm
    if use_bond_graph and width <= 2 * (cutoff + bond_cutoff):
        raise RuntimeError(
            f"Partition walls are too close together: width {width} <= "
            f"2*(cutoff+bond_cutoff)")
    if not use_bond_graph and width <= 2 * cutoff:
        raise RuntimeError(
            f"Partition walls are too close together: width {width} <= "
            f"2*cutoff")
    home = np.searchsorted(walls, x, side="left").astype(np.int32)
    return dim, walls, home


def assemble_partition(src, dst, off_i8, bond_flag, home, P, rank,
                       use_bond_graph, n_atoms):
    """Device-agnostic torch restatement of
    graph_build.cpp:build_partitions for ONE partition, from the global
    edge arrays in builder emission order.

    Bit-equality contract: fed the native builder's global arrays
    (py_index_1/2, offsets, within flags) it reproduces the native
    FOCUSED build's outputs exactly (tests/test_gpu_partition_seam.py);
    fed the GPU NL's arrays (same per-dst rows, pinned by
    test_gpu_graph_matches_cpu_builder) it is rank-invariant, which is
    what the cross-rank halo slices rely on.

    Returns a GpuPD carrying markers / line_markers / global_ids /
    n_owned in addition to the PartitionData fields."""
    dev = src.device
    E = src.shape[0]
    src64, dst64 = src.long(), dst.long()
    home_t = torch.as_tensor(home, dtype=torch.long, device=dev)

    # to_part: src of any cross-partition edge goes to dst's partition
    # (utils.c:1189-1253; conflicts impossible under the width check)
    hs, hd = home_t[src64], home_t[dst64]
    cross = hs != hd
    to_part = torch.full((n_atoms,), -1, dtype=torch.long, device=dev)
    to_part[src64[cross]] = hd[cross]

    # regions [pure | to_0.. | from_0..], each ascending by global id
    # (utils.c:1102-1154 packed order == ascending id — the rank-invariant
    # halo-slice alignment property)
    ids = torch.arange(n_atoms, dtype=torch.long, device=dev)
    p = rank
    is_home = home_t == p
    pure_m = is_home & (to_part == -1)
    markers = [0]
    gl = [ids[pure_m]]
    acc = int(pure_m.sum())
    for q in range(P):
        markers.append(acc)
        if q != p:
            t = ids[is_home & (to_part == q)]
            gl.append(t)
            acc += len(t)
    n_owned = acc
    for q in range(P):
        markers.append(acc)
        if q != p:
            t = ids[(home_t == q) & (to_part == p)]
            gl.append(t)
            acc += len(t)
    markers.append(acc)          # total (the dist.py:234-249 append)
    global_ids = torch.cat(gl)
    Nn = int(global_ids.numel())

    g2l = torch.full((n_atoms,), -1, dtype=torch.long, device=dev)
    g2l[global_ids] = torch.arange(Nn, dtype=torch.long, device=dev)

    # local edges: owner = home[dst] (utils.c:206), global order, then
    # STABLE sort by dst_local -> dst-sorted scatter layout
    eown_m = hd == p
    eidx = torch.nonzero(eown_m, as_tuple=False).squeeze(1)
    dl = g2l[dst64[eidx]]
    sl = g2l[src64[eidx]]
    perm = torch.argsort(dl, stable=True)
    pd = GpuPD()
    pd.device = dev
    pd.n_atoms = Nn
    pd.n_owned = n_owned
    pd.src = sl[perm].to(torch.int32)
    pd.dst = dl[perm].to(torch.int32)
    pd.row_ptr = _csr_of(dl[perm], Nn, dev)
    sperm = torch.argsort(sl[perm], stable=True)
    pd.src_perm = sperm.to(torch.int32)
    pd.src_row_ptr = _csr_of(sl[perm][sperm], Nn, dev)
    pd.off_i8 = off_i8[eidx][perm].contiguous()
    edge_gids = eidx[perm]
    pd.markers = np.asarray(markers, dtype=np.int64)
    pd.global_ids = global_ids.cpu().numpy()
    pd.line_markers = None

    if not use_bond_graph:
        pd.n_bonds = 0
        return pd

    g2l_edge = torch.full((E,), -1, dtype=torch.long, device=dev)
    g2l_edge[edge_gids] = torch.arange(len(edge_gids), dtype=torch.long,
                                       device=dev)

    # BDE classification over within edges in ascending order
    # (utils.c:497-653): from (ghost bonds), to, pure
    w_e = torch.nonzero(bond_flag.to(torch.bool), as_tuple=False).squeeze(1)
    wd, ws = dst64[w_e], src64[w_e]
    known = g2l[wd] != -1
    w_e, wd, ws = w_e[known], wd[known], ws[known]
    tp_d = to_part[wd]
    hm_d = home_t[wd]
    m_from = tp_d == p
    m_to = (~m_from) & (tp_d != -1)
    m_pure = (~m_from) & (tp_d == -1) & (hm_d == p)

    bde_parts = [w_e[m_pure]]
    needs_parts = [torch.ones(int(m_pure.sum()), dtype=torch.bool,
                              device=dev)]
    line_markers = [0]
    acc = int(m_pure.sum())
    for q in range(P):
        line_markers.append(acc)
        if q != p:
            t = w_e[m_to & (tp_d == q)]
            bde_parts.append(t)
            needs_parts.append(torch.ones(len(t), dtype=torch.bool,
                                          device=dev))
            acc += len(t)
    n_owned_bonds = acc
    for q in range(P):
        line_markers.append(acc)
        if q != p:
            t = w_e[m_from & (hm_d == q)]
            bde_parts.append(t)
            needs_parts.append(torch.zeros(len(t), dtype=torch.bool,
                                           device=dev))
            acc += len(t)
    line_markers.append(acc)     # total (dist.py:234-249 append)
    bde_e = torch.cat(bde_parts)               # global edge id per BDE
    needs = torch.cat(needs_parts)
    B = int(bde_e.numel())
    b_src_a = src64[bde_e]                     # global atom ids
    b_dst_a = dst64[bde_e]

    pd.n_bonds = B
    pd.line_markers = np.asarray(line_markers, dtype=np.int64)
    pd.map_de = g2l_edge[bde_e[:n_owned_bonds]]
    pd.map_ude = torch.arange(n_owned_bonds, dtype=torch.long, device=dev)
    pd.n_owned_bonds = n_owned_bonds

    # adjacency: BDEs grouped by src atom, stable (counting sort)
    srt = torch.argsort(b_src_a, stable=True)
    ssrc = b_src_a[srt]
    grp_start = torch.searchsorted(
        ssrc, torch.arange(n_atoms + 1, dtype=torch.long, device=dev))
    grp_cnt = grp_start[1:] - grp_start[:-1]

    # line edges: b1 -> b2 for b2 in group(dst_a(b1)), keep needs(b2) and
    # dst_a(b2) != src_a(b1) (utils.c:702-751); candidate order = group
    # order == CPU fill order, so expansion+filter == count+fill
    l_counts = grp_cnt[b_dst_a]
    Lc = int(l_counts.sum().item())
    e1 = torch.repeat_interleave(
        torch.arange(B, dtype=torch.long, device=dev), l_counts)
    csum = torch.cumsum(l_counts, 0) - l_counts
    offs = torch.arange(Lc, dtype=torch.long, device=dev) \
        - torch.repeat_interleave(csum, l_counts)
    e2 = srt[torch.repeat_interleave(grp_start[b_dst_a], l_counts) + offs]
    keep = needs[e2] & (b_dst_a[e2] != b_src_a[e1])
    e1, e2 = e1[keep], e2[keep]
    center = g2l[b_src_a[e2]]

    lsort = torch.argsort(e2, stable=True)
    l_src64, l_dst64, center64 = e1[lsort], e2[lsort], center[lsort]
    pd.l_src = l_src64.to(torch.int32)
    pd.l_dst = l_dst64.to(torch.int32)
    pd.center = center64.to(torch.int32)
    pd.line_row_ptr = _csr_of(l_dst64, B, dev)
    lsp = torch.argsort(l_src64, stable=True)
    pd.line_src_perm = lsp.to(torch.int32)
    pd.line_src_row_ptr = _csr_of(l_src64[lsp], B, dev)
    cp = torch.argsort(center64, stable=True)
    pd.center_perm = cp.to(torch.int32)
    pd.center_row_ptr = _csr_of(center64[cp], Nn, dev)
    return pd


def build_partition(structure, P, rank, cutoff, bond_cutoff, tol,
                    use_bond_graph, device, frac_override=None):
    """GPU SPMD slab build: full-box GPU neighbor list (cheap — 18.5 ms at
    1M atoms) + on-device partition assembly for THIS rank.  Replaces the
    per-rank focused CPU build (0.39-0.47 s at 1M/8) on the SPMD path for
    diagonal-lattice full-PBC structures."""
    full = build(structure, cutoff, bond_cutoff, tol,
                 use_bond_graph=False, device=device,
                 frac_override=frac_override, _want_bond_flag=True)
    frac_np = frac_override if frac_override is not None \
        else structure.frac_coords
    _, _, home = compute_walls_home(frac_np, structure.lattice, P, cutoff,
                                    bond_cutoff, use_bond_graph)
    return assemble_partition(full.src, full.dst, full.off_i8,
                              full.bond_flag, home, P, rank,
                              use_bond_graph, structure.num_atoms)


def build(structure, cutoff, bond_cutoff, tol, use_bond_graph, device,
          frac_override=None, _want_bond_flag=False):
    """Returns a GpuPD (or raises if unsupported — callers guard with
    supported())."""
    from distmlip_amd.ops import hip_lib, _check

    lib = hip_lib()
    dev = torch.device(device)
    lat33 = np.ascontiguousarray(structure.lattice, dtype=np.float64)
    pbc = [int(bool(int(x))) for x in structure.pbc]
    fast = fast_scope(lat33, pbc, cutoff)
    frac_np = frac_override if frac_override is not None \
        else structure.frac_coords
    frac = torch.tensor(np.asarray(frac_np), dtype=torch.float64, device=dev)
    N = frac.shape[0]
    if fast:
        lx, ly, lz = (float(x) for x in np.diag(lat33))
        pos = frac * torch.tensor([lx, ly, lz], dtype=torch.float64,
                                  device=dev)
        nc = [max(3, int(d // cutoff)) for d in (lx, ly, lz)]
        cxyz = [(frac[:, k] * nc[k]).long().clamp_(0, nc[k] - 1)
                for k in range(3)]
    else:
        if abs(np.linalg.det(lat33)) < 1e-12:
            raise RuntimeError("gpu_graph.build: singular lattice")
        # cart = frac @ lattice in the CPU builder's term order
        # (graph_build.cpp: u*row0 + v*row1 + w*row2)
        lat_t = torch.tensor(lat33, dtype=torch.float64, device=dev)
        pos = (frac[:, 0:1] * lat_t[0] + frac[:, 1:2] * lat_t[1]
               + frac[:, 2:3] * lat_t[2])
        nc_np, R_np, origin, span = cell_plan(
            lat33, pbc, frac_np, cutoff, tol, max_cells=_cell_cap(N))
        nc = [int(x) for x in nc_np]
        # bin in fractional space; atoms outside the planned extent (only
        # possible off-contract) are clamped into the edge cells
        cxyz = []
        for k in range(3):
            scale = nc[k] / span[k] if span[k] > 0.0 else 0.0
            cxyz.append(torch.floor((frac[:, k] - float(origin[k])) * scale)
                        .long().clamp_(0, nc[k] - 1))
        lat9 = (c_double * 9)(*lat33.reshape(-1).tolist())
        nc3 = (c_int32 * 3)(*nc)
        R3 = (c_int32 * 3)(*[int(x) for x in R_np])
        pbc3 = (c_int32 * 3)(*pbc)
    pos = pos.contiguous()
    ncx, ncy, ncz = nc
    cid = ((cxyz[0] * ncy + cxyz[1]) * ncz + cxyz[2]).to(torch.int32)
    order64 = torch.argsort(cid, stable=True)
    order = order64.to(torch.int32)
    sorted_cid = cid[order64]
    cell_start = torch.searchsorted(
        sorted_cid, torch.arange(ncx * ncy * ncz + 1, device=dev,
                                 dtype=torch.int32)).to(torch.int32)

    def fp(t):
        return ctypes.cast(t.data_ptr(), POINTER(c_double))

    def ip(t):
        return ctypes.cast(t.data_ptr(), POINTER(c_int32))

    stream = c_uint64(torch.cuda.current_stream().cuda_stream)
    cnt = torch.empty(N, dtype=torch.int32, device=dev)
    r2tol = cutoff * cutoff + tol
    if fast:
        _check(lib.dm_nl_count_f64(
            fp(pos), ip(cid), ip(order), ip(cell_start), ncx, ncy, ncz,
            c_double(lx), c_double(ly), c_double(lz), c_double(r2tol),
            c_double(tol), ip(cnt), c_int64(N), stream), "dm_nl_count_f64")
    else:
        _check(lib.dm_nl_count_gen_f64(
            fp(pos), ip(cid), ip(order), ip(cell_start), lat9, nc3, R3,
            pbc3, c_double(r2tol), c_double(tol), ip(cnt), c_int64(N),
            stream), "dm_nl_count_gen_f64")

    row_ptr64 = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    row_ptr64[1:] = torch.cumsum(cnt.long(), 0)
    E = int(row_ptr64[-1].item())
    if E > INT32_MAX:
        raise RuntimeError(f"gpu_graph.build: {E} edges exceed int32")
    row_ptr = row_ptr64.to(torch.int32)

    src = torch.empty(E, dtype=torch.int32, device=dev)
    off_i8 = torch.empty(E, 3, dtype=torch.int8, device=dev)
    bond_flag = torch.empty(E, dtype=torch.uint8, device=dev)
    br2tol = bond_cutoff * bond_cutoff + tol
    off_p = ctypes.cast(off_i8.data_ptr(), POINTER(ctypes.c_int8))
    flag_p = ctypes.cast(bond_flag.data_ptr(), POINTER(ctypes.c_uint8))
    if fast:
        _check(lib.dm_nl_fill_f64(
            fp(pos), ip(cid), ip(order), ip(cell_start), ncx, ncy, ncz,
            c_double(lx), c_double(ly), c_double(lz), c_double(r2tol),
            c_double(tol), c_double(br2tol), ip(row_ptr), ip(src),
            off_p, flag_p, c_int64(N), stream), "dm_nl_fill_f64")
    else:
        _check(lib.dm_nl_fill_gen_f64(
            fp(pos), ip(cid), ip(order), ip(cell_start), lat9, nc3, R3,
            pbc3, c_double(r2tol), c_double(tol), c_double(br2tol),
            ip(row_ptr), ip(src), off_p, flag_p, c_int64(N), stream),
            "dm_nl_fill_gen_f64")

    dst = torch.repeat_interleave(
        torch.arange(N, device=dev, dtype=torch.int32), cnt.long())

    pd = GpuPD()
    pd.device = dev
    pd.n_atoms = N
    pd.n_owned = N
    pd.src = src
    pd.dst = dst
    pd.row_ptr = row_ptr
    sperm64 = torch.argsort(src.long(), stable=True)
    pd.src_perm = sperm64.to(torch.int32)
    pd.src_row_ptr = _csr_of(src.long(), N, dev)
    pd.off_i8 = off_i8

    if use_bond_graph:
        eids_b = torch.nonzero(bond_flag, as_tuple=False).squeeze(1)
        B = int(eids_b.numel())
        b_src = src.long()[eids_b]
        b_dst = dst.long()[eids_b]
        # bonds grouped by src atom (adjacency, utils.c:702-751 semantics)
        srt = torch.argsort(b_src, stable=True)
        ssrc = b_src[srt]
        grp_start = torch.searchsorted(ssrc, torch.arange(N + 1, device=dev))
        grp_cnt = grp_start[1:] - grp_start[:-1]
        l_counts = grp_cnt[b_dst]
        L = int(l_counts.sum().item())
        e1 = torch.repeat_interleave(torch.arange(B, device=dev), l_counts)
        csum = torch.cumsum(l_counts, 0) - l_counts
        offs = torch.arange(L, device=dev) - torch.repeat_interleave(csum, l_counts)
        e2 = srt[torch.repeat_interleave(grp_start[b_dst], l_counts) + offs]
        keep = b_dst[e2] != b_src[e1]          # backtrack skip utils.c:727
        e1, e2 = e1[keep], e2[keep]
        center = b_src[e2]                      # utils.c:733 (local = global)
        # l_dst-sorted line layout + CSRs
        lsort = torch.argsort(e2, stable=True)
        l_src64, l_dst64, center64 = e1[lsort], e2[lsort], center[lsort]
        pd.n_bonds = B
        pd.l_src = l_src64.to(torch.int32)
        pd.l_dst = l_dst64.to(torch.int32)
        pd.center = center64.to(torch.int32)
        pd.line_row_ptr = _csr_of(l_dst64, B, dev)
        lsp = torch.argsort(l_src64, stable=True)
        pd.line_src_perm = lsp.to(torch.int32)
        pd.line_src_row_ptr = _csr_of(l_src64, B, dev)
        cp = torch.argsort(center64, stable=True)
        pd.center_perm = cp.to(torch.int32)
        pd.center_row_ptr = _csr_of(center64, N, dev)
        pd.map_de = eids_b
        pd.map_ude = torch.arange(B, device=dev)
    else:
        pd.n_bonds = 0
    if _want_bond_flag:
        pd.bond_flag = bond_flag
    return pd
