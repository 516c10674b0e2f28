// Set-up and tear-down of a context: fsi_create / fsi_create_tuned as a sequence of stages, fsi_destroy.
#include "fsi_host.hpp"

using namespace fsi;
using namespace fsi::host;

namespace {
const int TET_EDGES[6][2] = {{2, 3}, {1, 3}, {1, 2}, {0, 3}, {0, 2}, {0, 1}};      // UFC edge -> local vertices

// What one stage of fsi_create_tuned hands to the next: host vectors that are gone once the context stands.
struct Setup {
  std::vector<int64_t> gptr, rowptr;         // node graph on node ids (number_nodes .. build_node_graph); [ndof + 1] of the matrix
  std::vector<int32_t> gadj, prow_rank;      // ...; [V] rank of the node of pressure position q
  std::vector<int32_t> cell_dofs, cell_rank, cell_prow, tet_vertices;
  std::vector<uint16_t> enbr, epnbr;
  std::vector<int32_t> snode, sidx, sb_col;  // ranks of the solid nodes, ascending; [N2] rank -> compact solid index or -1
  std::vector<int64_t> sb_ptr;               // sb_ptr / sb_col: block-CSR pattern of the solid block on the compact numbering
};

// FsiTuning -> the context's fields (the kernels and the solver read those)
static void apply_tuning(FsiCtx* ctx, const FsiTuning& t) {
  ctx->tune = t;
  ctx->kry_fp32_policy = t.krylov_fp32; ctx->prod.policy32 = t.operator_fp32; ctx->schur_fp32 = t.schur_fp32 != 0;
  ctx->sweeps_fp32 = t.sweeps_fp32; ctx->solid_fp32 = t.solid_fp32;
  ctx->fused_sweeps = t.fused_sweeps != 0; ctx->sweeps_fp16 = ctx->fused_sweeps && t.sweeps_fp16 != 0;
  ctx->coloured = t.node_order == 2;
  ctx->newton_forcing = t.newton_forcing; ctx->newton_forcing_late = t.newton_forcing_late; ctx->newton_late_factor = t.newton_late_factor;
  ctx->f32_cycle_floor = t.f32_cycle_floor; ctx->f32_verdict_skip_rtol = t.f32_verdict_skip_rtol;
  ctx->orth_floor32 = t.orth_floor32; ctx->orth_floor64 = t.orth_floor64; ctx->gcr_escape = t.gcr_escape; ctx->gcr_reorth = t.gcr_reorth;
  ctx->prec_streams = t.prec_streams; ctx->cheb4 = t.cheb4; ctx->coarse_power = t.coarse_power; ctx->solid_mg = t.solid_mg; ctx->dd_mg = t.dd_mg;
  ctx->solid_block_jacobi = t.solid_block_jacobi; ctx->solid_fused = t.solid_fused;
  ctx->cheb_its_s = t.its_solid; ctx->cheb_its_f = t.its_fluid; ctx->cheb_its_p = t.its_schur; ctx->cheb_its_d = t.its_disp;
  ctx->cheb_kappa_s = t.kappa_solid; ctx->cheb_kappa_f = t.kappa_fluid; ctx->cheb_kappa_p = t.kappa_schur; ctx->cheb_kappa_d = t.kappa_disp;
  ctx->solid_coarse_exact = t.solid_coarse_exact;
  ctx->newton_adaptive = t.newton_adaptive;
  ctx->sbmg_pre = t.sbmg_pre; ctx->sbmg_post = t.sbmg_post; ctx->sbmg_cits = t.sbmg_cits; ctx->sbmg_alpha = t.sbmg_alpha; ctx->sbmg_ckappa = t.sbmg_ckappa;
  ctx->mg_pre = t.mg_pre; ctx->mg_post = t.mg_post; ctx->mg_cits = t.mg_cits; ctx->mg_alpha = t.mg_alpha; ctx->mg_ckappa = t.mg_ckappa;
}

// produces: the context's tuning (checked, applied); refuses a bad mesh description or bad parameters
static int check_inputs(FsiCtx* ctx, const FsiMeshDesc* mesh, const FsiParams* prm, int device, const FsiTuning* tuning) {
  FsiTuning t;
  fsi_tuning_defaults(&t);
  if (tuning) {      // a caller built against a shorter struct: its fields, the defaults for the rest
    const size_t n = std::min<size_t>(sizeof(FsiTuning), tuning->struct_size > 0 ? (size_t)tuning->struct_size : sizeof(FsiTuning));
    std::memcpy(&t, tuning, n);
    t.struct_size = (int32_t)sizeof(FsiTuning);
  }
  if (t.its_schur <= 0 || t.its_disp <= 0 || t.its_fluid <= 0 || t.its_solid <= 0 || t.krylov_capacity < 8 || t.krylov_fp32 < 0 || t.krylov_fp32 > 2 ||
      (t.jacobian_waves != 1 && t.jacobian_waves != 2) || !(t.newton_forcing >= 0.0)) {
    ctx->err = "fsi_create: FsiTuning out of range (sweep counts must be positive, krylov_capacity >= 8, krylov_fp32 in 0..2, jacobian_waves 1 | 2)";
    return FSI_ERR_INVALID;
  }
  apply_tuning(ctx, t);
  ctx->device = device;
  const int64_t V = mesh->num_vertices, N2 = mesh->num_nodes, C = mesh->num_cells;
  if (V <= 0 || N2 < V || C <= 0 || !mesh->coords || !mesh->tet_nodes || !mesh->cell_kind || !mesh->cell_region) {
    ctx->err = "fsi_create: empty or inconsistent mesh description";
    return FSI_ERR_INVALID;
  }
  if (prm->num_fluid_regions > MAX_REGIONS || prm->num_solid_regions > MAX_REGIONS || !(prm->dt > 0.0)) {
    ctx->err = "fsi_create: bad parameters (dt <= 0 or too many regions)";
    return FSI_ERR_INVALID;
  }
  if (6 * N2 + V >= (int64_t)2147483647) { ctx->err = "fsi_create: more than 2^31 dofs"; return FSI_ERR_INVALID; }
  for (int64_t c = 0; c < C; ++c) {
    const int kind = mesh->cell_kind[c], reg = mesh->cell_region[c];
    if (kind < 0 || kind > 1 || reg < 0 || reg >= (kind == 0 ? prm->num_fluid_regions : prm->num_solid_regions)) {
      ctx->err = "fsi_create: cell with a bad kind/region marker";
      return FSI_ERR_INVALID;
    }
    for (int a = 0; a < 10; ++a) {
      const int32_t nd = mesh->tet_nodes[10 * c + a];
      if (nd < 0 || nd >= N2 || (a < 4 && nd >= V)) { ctx->err = "fsi_create: node id out of range"; return FSI_ERR_INVALID; }
    }
  }
  for (int r = 0; r < prm->num_solid_regions; ++r)
    if (prm->solid_models && (prm->solid_models[r] < 0 || prm->solid_models[r] > 1)) { ctx->err = "fsi_create: material model must be 0 (StVenantKirchoff) or 1 (MooneyRivlin)"; return FSI_ERR_INVALID; }
  return FSI_OK;
}

// produces: the two streams, the ev_* events, the element tables in constant memory
static int open_device(FsiCtx* ctx, int device) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device) { ctx->err = "fsi_create: no such HIP device"; return FSI_ERR_DEVICE; }
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipStreamCreate(&ctx->stream));
  HIPCHK(hipStreamCreate(&ctx->stream2));
  for (hipEvent_t* e : {&ctx->ev_split, &ctx->ev_solid, &ctx->ev_b}) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
  HIPCHK(hipEventCreate(&ctx->ev0));
  HIPCHK(hipEventCreate(&ctx->ev1));
  HIPCHK(upload_tables());
  return FSI_OK;
}

// produces: sizes, scheme, material properties and the host copy of the mesh
static void copy_problem(FsiCtx* ctx, const FsiMeshDesc* mesh, const FsiParams* prm) {
  const int64_t V = mesh->num_vertices, N2 = mesh->num_nodes, C = mesh->num_cells;
  ctx->V = V; ctx->N2 = N2; ctx->C = C; ctx->ndof = 6 * N2 + V;
  if (ctx->tune.mg_post <= 0) {
    // "by size" (the default): what a fine displacement sweep costs is a launch's latency in a small context and its bytes in a large
    // one, what it saves in outer iterations is the same - seven sweeps after the coarse correction win 2 - 15 % up to 630 k tets in
    // both storage modes, five win 3 - 6 % from 1.12 M tets on in the mixed mode (profiles/r05_param_scan_final_tree.txt)
    ctx->tune.mg_post = N2 < 1100000 ? 7 : 5;
    ctx->mg_post = ctx->tune.mg_post;
  }
  ctx->scheme = Scheme{prm->dt, prm->theta, 1.0 - prm->theta, prm->delta, prm->laplace_alpha};
  ctx->nfluid = prm->num_fluid_regions;
  ctx->nsolid = prm->num_solid_regions;
  for (int r = 0; r < MAX_REGIONS; ++r) { ctx->fluid[r] = FluidProps{1.0, 1.0}; ctx->solid[r] = SolidProps{1.0, 1.0, 1.0, 0, 0.0, 0.0, 0.0}; }
  for (int r = 0; r < ctx->nfluid; ++r) ctx->fluid[r] = FluidProps{prm->fluid_props[2 * r], prm->fluid_props[2 * r + 1]};
  for (int r = 0; r < ctx->nsolid; ++r)
    ctx->solid[r] = SolidProps{prm->solid_props[6 * r], prm->solid_props[6 * r + 1], prm->solid_props[6 * r + 2],
                               prm->solid_models ? prm->solid_models[r] : 0, prm->solid_props[6 * r + 3],
                               prm->solid_props[6 * r + 4], prm->solid_props[6 * r + 5]};
  ctx->h_coords.assign(mesh->coords, mesh->coords + 3 * V);
  ctx->h_tet_nodes.assign(mesh->tet_nodes, mesh->tet_nodes + 10 * C);
}

// produces: h_rank2node, h_node2rank, h_prank, prow_rank, levels (owner or Morton order, optionally multicoloured); the graph on node ids
static int number_nodes(FsiCtx* ctx, const FsiMeshDesc* mesh, Setup& s) {
  const int64_t V = ctx->V, N2 = ctx->N2, C = ctx->C;
  const int32_t* tn = ctx->h_tet_nodes.data();
  std::vector<int64_t>& gptr = s.gptr;
  std::vector<int32_t>&gadj = s.gadj, &prow_rank = s.prow_rank;
  // ---- base ordering: every vertex followed by the edge nodes it owns (= edges whose lower vertex it is) ------
  std::vector<int32_t> owner(N2, -1), other(N2, 0);
  for (int32_t v = 0; v < V; ++v) owner[v] = v;
  for (int64_t c = 0; c < C; ++c)
    for (int e = 0; e < 6; ++e) {
      const int32_t a = tn[10 * c + TET_EDGES[e][0]], b = tn[10 * c + TET_EDGES[e][1]], nd = tn[10 * c + 4 + e];
      owner[nd] = std::min(a, b);
      other[nd] = std::max(a, b);
    }
  for (int64_t i = 0; i < N2; ++i)
    if (owner[i] < 0) { ctx->err = "fsi_create: P2 node that belongs to no cell"; return FSI_ERR_INVALID; }
  std::vector<int32_t> base(N2);
  std::iota(base.begin(), base.end(), 0);
  std::sort(base.begin(), base.end(), [&](int32_t x, int32_t y) {
    if (owner[x] != owner[y]) return owner[x] < owner[y];
    const bool ex = x >= V, ey = y >= V;
    if (ex != ey) return !ex;
    if (other[x] != other[y]) return other[x] < other[y];
    return x < y;
  });
  // default numbering: P2 nodes along a Morton (Z-order) curve through their coordinates - spatially compact runs of
  // consecutive nodes are what the gathers of every SpMV, the element scatters and the LDS tiles live on
  if (ctx->tune.node_order == 0) {      // mesh / multicolour order keep `base`
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300};
    for (int64_t v = 0; v < V; ++v)
      for (int i = 0; i < 3; ++i) { lo[i] = std::min(lo[i], mesh->coords[3 * v + i]); hi[i] = std::max(hi[i], mesh->coords[3 * v + i]); }
    double span = 0.0;
    for (int i = 0; i < 3; ++i) span = std::max(span, hi[i] - lo[i]);
    if (!(span > 0.0)) span = 1.0;
    auto spread = [](uint64_t x) {          // 21 bits -> every third bit
      x &= 0x1fffff;
      x = (x | x << 32) & 0x1f00000000ffffull;
      x = (x | x << 16) & 0x1f0000ff0000ffull;
      x = (x | x << 8) & 0x100f00f00f00f00full;
      x = (x | x << 4) & 0x10c30c30c30c30c3ull;
      x = (x | x << 2) & 0x1249249249249249ull;
      return x;
    };
    std::vector<uint64_t> code(N2);
    for (int64_t nd = 0; nd < N2; ++nd) {
      uint64_t c = 0;
      for (int i = 0; i < 3; ++i) {
        const double x = nd < V ? mesh->coords[3 * nd + i]
                                : 0.5 * (mesh->coords[3 * (int64_t)owner[nd] + i] + mesh->coords[3 * (int64_t)other[nd] + i]);
        const uint64_t q = (uint64_t)std::min(2097151.0, std::max(0.0, (x - lo[i]) / span * 2097151.0));
        c |= spread(q) << i;
      }
      code[nd] = c;
    }
    std::sort(base.begin(), base.end(), [&](int32_t a, int32_t b) { return code[a] != code[b] ? code[a] < code[b] : a < b; });
  }

  // ---- node graph (node ids), sorted unique pairs ---------------------------------------------------------------
  std::vector<uint64_t> pairs;
  pairs.reserve((size_t)C * 100);
  for (int64_t c = 0; c < C; ++c)
    for (int a = 0; a < 10; ++a)
      for (int b = 0; b < 10; ++b)
        pairs.push_back(((uint64_t)(uint32_t)tn[10 * c + a] << 32) | (uint32_t)tn[10 * c + b]);
  std::sort(pairs.begin(), pairs.end());
  pairs.erase(std::unique(pairs.begin(), pairs.end()), pairs.end());
  gptr.assign(N2 + 1, 0);
  gadj.resize(pairs.size());
  for (size_t i = 0; i < pairs.size(); ++i) {
    gptr[(pairs[i] >> 32) + 1] += 1;
    gadj[i] = (int32_t)(pairs[i] & 0xffffffffu);
  }
  for (int64_t r = 0; r < N2; ++r) gptr[r + 1] += gptr[r];
  std::vector<uint64_t>().swap(pairs);

  // ---- greedy multicolouring of the node graph (base order): nodes of one colour share no element -----------------
  // (only the ILU(0) paths need it; the default Chebyshev-based preconditioner keeps the mesh's own node order, whose
  //  locality is what the gathers of every SpMV live on.  FSI_ORDER=colour selects the multicolour ordering.)
  std::vector<int32_t> color(N2, ctx->coloured ? -1 : 0);
  if (!ctx->coloured) ctx->ncolors = 1;
  if (ctx->coloured) {
    std::vector<int32_t> mark(1024, -1);
    for (int64_t r = 0; r < N2; ++r) {
      const int32_t nd = base[r];
      for (int64_t k = gptr[nd]; k < gptr[nd + 1]; ++k) {
        const int32_t c = color[gadj[k]];
        if (c >= 0) {
          if ((size_t)c >= mark.size()) mark.resize(2 * c + 2, -1);
          mark[c] = nd;
        }
      }
      int32_t c = 0;
      while ((size_t)c < mark.size() && mark[c] == nd) ++c;
      if ((size_t)c >= mark.size()) mark.resize(2 * c + 2, -1);
      color[nd] = c;
      ctx->ncolors = std::max(ctx->ncolors, c + 1);
    }
  }
  ctx->h_rank2node = base;
  std::stable_sort(ctx->h_rank2node.begin(), ctx->h_rank2node.end(), [&](int32_t x, int32_t y) { return color[x] < color[y]; });
  ctx->h_node2rank.resize(N2);
  for (int64_t r = 0; r < N2; ++r) ctx->h_node2rank[ctx->h_rank2node[r]] = (int32_t)r;
  // pressure block: vertices in the same (colour, base) order
  ctx->h_prank.assign(V, 0);
  prow_rank.resize(V);
  int32_t q = 0;
  for (int64_t r = 0; r < N2; ++r) {
    const int32_t nd = ctx->h_rank2node[r];
    if (nd < V) { ctx->h_prank[nd] = q; prow_rank[q] = (int32_t)r; ++q; }
  }
  // levels: one per colour for the d/v rows (6 rows per node), then one per colour for the pressure rows
  std::vector<int64_t> ncount(ctx->ncolors, 0), vcount(ctx->ncolors, 0);
  for (int64_t nd = 0; nd < N2; ++nd) { ncount[color[nd]] += 1; if (nd < V) vcount[color[nd]] += 1; }
  int64_t r0 = 0;
  for (int c = 0; c < ctx->ncolors; ++c) { ctx->levels.push_back(Level{6 * r0, ncount[c], 6}); r0 += ncount[c]; }
  int64_t q0 = 0;
  for (int c = 0; c < ctx->ncolors; ++c) { ctx->levels.push_back(Level{6 * N2 + q0, vcount[c], 1}); q0 += vcount[c]; }
  return FSI_OK;
}

// produces: h_nadj*, h_padj* (final ranks), the monolithic matrix' rowptr and nnz; refuses rows beyond the row buffers
static int build_node_graph(FsiCtx* ctx, Setup& s) {
  const int64_t V = ctx->V, N2 = ctx->N2;
  const std::vector<int32_t>&rk = ctx->h_node2rank, &prow_rank = s.prow_rank;
  std::vector<int64_t>&gptr = s.gptr, &rowptr = s.rowptr;
  std::vector<int32_t>& gadj = s.gadj;
  // adjacency in final ranks (ascending) and pressure neighbours as positions in the pressure block (ascending)
  ctx->h_nadj_ptr.assign(N2 + 1, 0);
  ctx->h_nadj.resize(gadj.size());
  ctx->h_padj_ptr.assign(N2 + 1, 0);
  ctx->h_padj.clear();
  int64_t o = 0;
  std::vector<int32_t> tmpv;
  for (int64_t r = 0; r < N2; ++r) {
    const int32_t nd = ctx->h_rank2node[r];
    const int64_t o0 = o;
    tmpv.clear();
    for (int64_t k = gptr[nd]; k < gptr[nd + 1]; ++k) {
      ctx->h_nadj[o++] = rk[gadj[k]];
      if (gadj[k] < V) tmpv.push_back(ctx->h_prank[gadj[k]]);
    }
    std::sort(ctx->h_nadj.begin() + o0, ctx->h_nadj.begin() + o);
    std::sort(tmpv.begin(), tmpv.end());
    ctx->h_padj.insert(ctx->h_padj.end(), tmpv.begin(), tmpv.end());
    ctx->h_nadj_ptr[r + 1] = o;
    ctx->h_padj_ptr[r + 1] = (int64_t)ctx->h_padj.size();
  }
  std::vector<int64_t>().swap(gptr);
  std::vector<int32_t>().swap(gadj);
  for (int64_t r = 0; r < N2; ++r) {
    const int64_t deg = ctx->h_nadj_ptr[r + 1] - ctx->h_nadj_ptr[r];
    if (deg >= 65536 / 6 || 6 * deg + (ctx->h_padj_ptr[r + 1] - ctx->h_padj_ptr[r]) > 1024) {
      ctx->err = "fsi_create: node with too many neighbours for the row buffers (max 1024 entries per row)";
      return FSI_ERR_INVALID;
    }
  }

  // ---- CSR row pointers ------------------------------------------------------------------------------------
  rowptr.assign(ctx->ndof + 1, 0);
  for (int64_t r = 0; r < N2; ++r) {
    const int64_t len = 6 * (ctx->h_nadj_ptr[r + 1] - ctx->h_nadj_ptr[r]) + (ctx->h_padj_ptr[r + 1] - ctx->h_padj_ptr[r]);
    for (int t = 0; t < 6; ++t) rowptr[6 * r + t + 1] = len;
  }
  for (int64_t q = 0; q < V; ++q) {
    const int32_t r = prow_rank[q];
    rowptr[6 * N2 + q + 1] = 6 * (ctx->h_nadj_ptr[r + 1] - ctx->h_nadj_ptr[r]) + (ctx->h_padj_ptr[r + 1] - ctx->h_padj_ptr[r]);
  }
  for (int64_t i = 0; i < ctx->ndof; ++i) rowptr[i + 1] += rowptr[i];
  ctx->nnz = rowptr[ctx->ndof];
  return FSI_OK;
}

// produces: cell_dofs, cell_rank, cell_prow, enbr, epnbr, tet_vertices
static void build_element_tables(FsiCtx* ctx, Setup& s) {
  const int64_t N2 = ctx->N2, C = ctx->C;
  const int32_t* tn = ctx->h_tet_nodes.data(); const std::vector<int32_t>& rk = ctx->h_node2rank;
  std::vector<int32_t>&cell_dofs = s.cell_dofs, &cell_rank = s.cell_rank, &tet_vertices = s.tet_vertices, &cell_prow = s.cell_prow;
  std::vector<uint16_t>&enbr = s.enbr, &epnbr = s.epnbr;
  cell_dofs.resize((size_t)C * NLOC); cell_rank.resize((size_t)C * 10); tet_vertices.resize((size_t)C * 4); cell_prow.resize((size_t)C * 4);
  enbr.resize((size_t)C * 100); epnbr.resize((size_t)C * 40);
  for (int64_t c = 0; c < C; ++c) {
    for (int a = 0; a < 10; ++a) {
      const int32_t ra = rk[tn[10 * c + a]];
      cell_rank[10 * c + a] = ra;
      for (int cmp = 0; cmp < 3; ++cmp) {
        cell_dofs[c * NLOC + cmp * 10 + a] = 6 * ra + cmp;
        cell_dofs[c * NLOC + 30 + cmp * 10 + a] = 6 * ra + 3 + cmp;
      }
      const int32_t* lo = ctx->h_nadj.data() + ctx->h_nadj_ptr[ra];
      const int32_t* hi = ctx->h_nadj.data() + ctx->h_nadj_ptr[ra + 1];
      for (int b = 0; b < 10; ++b)
        enbr[c * 100 + a * 10 + b] = (uint16_t)(std::lower_bound(lo, hi, rk[tn[10 * c + b]]) - lo);
      const int32_t* plo = ctx->h_padj.data() + ctx->h_padj_ptr[ra];
      const int32_t* phi = ctx->h_padj.data() + ctx->h_padj_ptr[ra + 1];
      for (int b = 0; b < 4; ++b)
        epnbr[c * 40 + a * 4 + b] = (uint16_t)(std::lower_bound(plo, phi, ctx->h_prank[tn[10 * c + b]]) - plo);
    }
    for (int a = 0; a < 4; ++a) {
      cell_dofs[c * NLOC + 60 + a] = (int32_t)(6 * N2 + ctx->h_prank[tn[10 * c + a]]);
      cell_prow[4 * c + a] = cell_dofs[c * NLOC + 60 + a];
      tet_vertices[4 * c + a] = tn[10 * c + a];
    }
  }
}

// produces: col_cells, h_col_ptr, ncellcol - the assembly colouring: greedy, balanced (the least used admissible colour), at most 128 colours
static int colour_cells(FsiCtx* ctx, const Setup& s) {
  const int64_t N2 = ctx->N2, C = ctx->C;
  const std::vector<int32_t>& cell_rank = s.cell_rank;
  constexpr int MAXCOL = 128;
  std::vector<uint64_t> used((size_t)N2 * 2, 0);
  std::vector<uint8_t> colour((size_t)C);
  std::vector<int64_t> count;
  bool ok = true;
  for (int64_t c = 0; c < C && ok; ++c) {
    uint64_t m0 = 0, m1 = 0;
    for (int a = 0; a < 10; ++a) { m0 |= used[2 * (size_t)cell_rank[10 * c + a]]; m1 |= used[2 * (size_t)cell_rank[10 * c + a] + 1]; }
    int best = -1;
    for (int k = 0; k < (int)count.size(); ++k) {
      const bool taken = k < 64 ? (m0 >> k) & 1 : (m1 >> (k - 64)) & 1;
      if (!taken && (best < 0 || count[k] < count[best])) best = k;
    }
    if (best < 0) {
      if ((int)count.size() == MAXCOL) { ok = false; break; }
      best = (int)count.size();
      count.push_back(0);
    }
    colour[c] = (uint8_t)best;
    count[best] += 1;
    for (int a = 0; a < 10; ++a) {
      if (best < 64) used[2 * (size_t)cell_rank[10 * c + a]] |= 1ull << best;
      else used[2 * (size_t)cell_rank[10 * c + a] + 1] |= 1ull << (best - 64);
    }
  }
  if (ok) {
    const int nc = (int)count.size();
    ctx->h_col_ptr.assign(nc + 1, 0);
    for (int k = 0; k < nc; ++k) ctx->h_col_ptr[k + 1] = ctx->h_col_ptr[k] + count[k];
    std::vector<int64_t> fill(ctx->h_col_ptr.begin(), ctx->h_col_ptr.end() - 1);
    std::vector<int32_t> cells((size_t)C);
    for (int64_t c = 0; c < C; ++c) cells[fill[colour[c]]++] = (int32_t)c;
    FSICHK(upload(ctx, ctx->col_cells, cells));
    ctx->ncellcol = nc;
  }   // more than 128 cells around one node: the unordered single launch stays (ncellcol = 0)
  return FSI_OK;
}

// produces: inc*, pinc*, Re - the incidences of the residual gather: per node rank / pressure row the (cell, local index) pairs, cells ascending
static int residual_incidences(FsiCtx* ctx, const Setup& s) {
  const int64_t V = ctx->V, N2 = ctx->N2, C = ctx->C;
  const std::vector<int32_t>&cell_rank = s.cell_rank, &cell_prow = s.cell_prow;
  if (C < (int64_t)1 << 27) {
    std::vector<int64_t> iptr((size_t)N2 + 1, 0), pptr((size_t)V + 1, 0);
    for (int64_t c = 0; c < C; ++c) {
      for (int a = 0; a < 10; ++a) iptr[(size_t)cell_rank[10 * c + a] + 1] += 1;
      for (int a = 0; a < 4; ++a) pptr[(size_t)(cell_prow[4 * c + a] - 6 * N2) + 1] += 1;
    }
    for (int64_t r = 0; r < N2; ++r) iptr[r + 1] += iptr[r];
    for (int64_t q = 0; q < V; ++q) pptr[q + 1] += pptr[q];
    std::vector<int32_t> inc((size_t)10 * C), pinc((size_t)4 * C);
    std::vector<int64_t> ifill(iptr.begin(), iptr.end() - 1), pfill(pptr.begin(), pptr.end() - 1);
    for (int64_t c = 0; c < C; ++c) {
      for (int a = 0; a < 10; ++a) inc[ifill[cell_rank[10 * c + a]]++] = (int32_t)(16 * c + a);
      for (int a = 0; a < 4; ++a) pinc[pfill[cell_prow[4 * c + a] - 6 * N2]++] = (int32_t)(16 * c + a);
    }
    FSICHK(upload(ctx, ctx->inc_ptr, iptr));
    FSICHK(upload(ctx, ctx->pinc_ptr, pptr));
    FSICHK(upload(ctx, ctx->inc, inc));
    FSICHK(upload(ctx, ctx->pinc, pinc));
    HIPCHK(ctx->Re.alloc((size_t)C * NLOC));
  }
  return FSI_OK;
}

// produces: the numbering, element tables, node graph and matrix structure on the device (cols, diagpos, geom), the work vectors
static int upload_structure(FsiCtx* ctx, const FsiMeshDesc* mesh, const Setup& s) {
  const int64_t V = ctx->V, N2 = ctx->N2, C = ctx->C;
  const std::vector<int32_t>& rk = ctx->h_node2rank;
  ctx->h_user2solver.resize(ctx->ndof);
  std::vector<int32_t> solver2user(ctx->ndof);
  for (int64_t nd = 0; nd < N2; ++nd)
    for (int cmp = 0; cmp < 3; ++cmp) {
      ctx->h_user2solver[3 * nd + cmp] = 6 * rk[nd] + cmp;
      ctx->h_user2solver[3 * N2 + 3 * nd + cmp] = 6 * rk[nd] + 3 + cmp;
    }
  for (int64_t v = 0; v < V; ++v) ctx->h_user2solver[6 * N2 + v] = (int32_t)(6 * N2 + ctx->h_prank[v]);
  for (int64_t i = 0; i < ctx->ndof; ++i) solver2user[ctx->h_user2solver[i]] = (int32_t)i;

  // ---- upload ------------------------------------------------------------------------------------------------
  FSICHK(upload(ctx, ctx->user2solver, ctx->h_user2solver));
  FSICHK(upload(ctx, ctx->solver2user, solver2user));
  FSICHK(upload(ctx, ctx->cell_dofs, s.cell_dofs));
  FSICHK(upload(ctx, ctx->cell_rank, s.cell_rank));
  FSICHK(upload(ctx, ctx->cell_prow, s.cell_prow));
  FSICHK(upload(ctx, ctx->enbr, s.enbr));
  FSICHK(upload(ctx, ctx->epnbr, s.epnbr));
  FSICHK(upload(ctx, ctx->cell_kind, std::vector<int32_t>(mesh->cell_kind, mesh->cell_kind + C)));
  FSICHK(upload(ctx, ctx->cell_region, std::vector<int32_t>(mesh->cell_region, mesh->cell_region + C)));
  FSICHK(upload(ctx, ctx->nadj_ptr, ctx->h_nadj_ptr));
  FSICHK(upload(ctx, ctx->nadj, ctx->h_nadj));
  FSICHK(upload(ctx, ctx->padj_ptr, ctx->h_padj_ptr));
  FSICHK(upload(ctx, ctx->padj, ctx->h_padj));
  FSICHK(upload(ctx, ctx->rowptr, s.rowptr));
  HIPCHK(ctx->cols.alloc(ctx->nnz));
  HIPCHK(ctx->diagpos.alloc(ctx->ndof));
  FSICHK(upload(ctx, ctx->vrank, s.prow_rank));
  {
    DevBuf<int32_t> d_tv;
    DevBuf<double> d_coords;
    FSICHK(upload(ctx, d_tv, s.tet_vertices));
    FSICHK(upload(ctx, d_coords, ctx->h_coords));
    HIPCHK(ctx->geom.alloc((size_t)C * 10));
    launch_expand_cols(ctx->stream, N2, V, ctx->nadj_ptr.p, ctx->nadj.p, ctx->padj_ptr.p, ctx->padj.p, ctx->vrank.p,
                       ctx->rowptr.p, ctx->cols.p, ctx->diagpos.p);
    launch_geometry(ctx->stream, C, d_coords.p, d_tv.p, ctx->geom.p);
    HIPCHK(hipStreamSynchronize(ctx->stream));
  }
  const int64_t n = ctx->ndof;
  DevBuf<double>* vecs[] = {&ctx->U, &ctx->U1, &ctx->F, &ctx->b, &ctx->du, &ctx->bs, &ctx->tmp1, &ctx->tmp2, &ctx->tmp3,
                            &ctx->tmp4, &ctx->tmp5, &ctx->tmp6, &ctx->tmp7, &ctx->rowscale};
  for (auto* v : vecs) {
    HIPCHK(v->alloc(n));
    HIPCHK(hipMemsetAsync(v->p, 0, n * sizeof(double), ctx->stream));
  }
  HIPCHK(ctx->A_pre.alloc(ctx->nnz));
  HIPCHK(ctx->A.alloc(ctx->nnz));
  return FSI_OK;
}

// produces: node_solid, the masks, the compact solid block three times (ss_* CSR, sb_* block-CSR, fs_* coupling rows), the sampling events
static int build_solid_blocks(FsiCtx* ctx, const FsiMeshDesc* mesh, Setup& s) {
  const int64_t N2 = ctx->N2, C = ctx->C;
  const int32_t* tn = ctx->h_tet_nodes.data(); const std::vector<int32_t>& rk = ctx->h_node2rank;
  std::vector<int32_t>&snode = s.snode, &sidx = s.sidx, &sb_col = s.sb_col;
  std::vector<int64_t>& sb_ptr = s.sb_ptr;
  std::vector<int32_t> node_solid(N2, 0);
  for (int64_t c = 0; c < C; ++c)
    if (mesh->cell_kind[c] == 1)
      for (int a = 0; a < 10; ++a) node_solid[rk[tn[10 * c + a]]] = 1;
  FSICHK(upload(ctx, ctx->node_solid, node_solid));
  std::vector<double> ms(3 * N2), mf(3 * N2);
  for (int64_t r = 0; r < N2; ++r)
    for (int i = 0; i < 3; ++i) { ms[3 * r + i] = node_solid[r] ? 1.0 : 0.0; mf[3 * r + i] = node_solid[r] ? 0.0 : 1.0; }
  sidx.assign(N2, -1);
  for (int64_t r = 0; r < N2; ++r)
    if (node_solid[r]) { sidx[r] = (int32_t)snode.size(); snode.push_back((int32_t)r); }
  const int64_t nS = (int64_t)snode.size();
  ctx->nS = nS;
  std::vector<int64_t> ss_rowptr(3 * nS + 1, 0), ss_diagpos(3 * nS, 0), ss_src;
  std::vector<int32_t> ss_cols;
  for (int64_t i = 0; i < nS; ++i) {
    const int64_t r = snode[i], a = ctx->h_nadj_ptr[r], deg = ctx->h_nadj_ptr[r + 1] - a;
    for (int c = 0; c < 3; ++c) {
      const int64_t row0 = 9 * a + 3 * c * deg;            // start of row 3r+c in the 3x3-blocked structure
      for (int64_t k = 0; k < deg; ++k) {
        const int32_t si = sidx[ctx->h_nadj[a + k]];
        if (si < 0) continue;
        for (int j = 0; j < 3; ++j) {
          if (si == i && j == c) ss_diagpos[3 * i + c] = (int64_t)ss_cols.size();
          ss_cols.push_back(3 * si + j);
          ss_src.push_back(row0 + 3 * k + j);
        }
      }
      ss_rowptr[3 * i + c + 1] = (int64_t)ss_cols.size();
    }
  }
  {   // block-CSR structure of the same block
    std::vector<int64_t> sb_src;
    std::vector<int32_t> sb_row, sb_stride(nS);
    sb_ptr.assign(nS + 1, 0);
    for (int64_t i = 0; i < nS; ++i) {
      const int64_t r = snode[i], a = ctx->h_nadj_ptr[r], deg = ctx->h_nadj_ptr[r + 1] - a;
      sb_stride[i] = (int32_t)(3 * deg);
      for (int64_t k = 0; k < deg; ++k) {
        const int32_t si = sidx[ctx->h_nadj[a + k]];
        if (si < 0) continue;
        sb_col.push_back(si);
        sb_row.push_back((int32_t)i);
        sb_src.push_back(9 * a + 3 * k);
      }
      sb_ptr[i + 1] = (int64_t)sb_col.size();
    }
    ctx->sb_nblocks = (int64_t)sb_col.size();
    FSICHK(upload(ctx, ctx->sb_ptr, sb_ptr));
    FSICHK(upload(ctx, ctx->sb_src, sb_src));
    FSICHK(upload(ctx, ctx->sb_col, sb_col));
    FSICHK(upload(ctx, ctx->sb_row, sb_row));
    FSICHK(upload(ctx, ctx->sb_stride, sb_stride));
    HIPCHK(ctx->sb_vals.alloc(9 * sb_col.size()));
    HIPCHK(ctx->sb_dinv.alloc(4 * nS));
    HIPCHK(ctx->sb_binv12.alloc(12 * nS));
    HIPCHK(ctx->sb_binv9.alloc(9 * nS));
  }
  {   // rows of fluid-interior nodes that see solid columns: the only rows the solid predictor changes in the fluid rhs
    std::vector<int32_t> fs_rows, fs_col;
    std::vector<int64_t> fs_ptr(1, 0), fs_src;
    for (int64_t r = 0; r < N2; ++r) {
      if (node_solid[r]) continue;
      const int64_t a = ctx->h_nadj_ptr[r], deg = ctx->h_nadj_ptr[r + 1] - a;
      bool any = false;
      for (int64_t k = 0; k < deg && !any; ++k) any = node_solid[ctx->h_nadj[a + k]] != 0;
      if (!any) continue;
      for (int c = 0; c < 3; ++c) {
        const int64_t row0 = 9 * a + 3 * c * deg;
        for (int64_t k = 0; k < deg; ++k) {
          const int32_t nb = ctx->h_nadj[a + k];
          if (!node_solid[nb]) continue;
          for (int j = 0; j < 3; ++j) { fs_col.push_back(3 * nb + j); fs_src.push_back(row0 + 3 * k + j); }
        }
        fs_rows.push_back((int32_t)(3 * r + c));
        fs_ptr.push_back((int64_t)fs_col.size());
      }
    }
    ctx->nfs = (int64_t)fs_rows.size();
    FSICHK(upload(ctx, ctx->fs_rows, fs_rows));
    FSICHK(upload(ctx, ctx->fs_ptr, fs_ptr));
    FSICHK(upload(ctx, ctx->fs_col, fs_col));
    FSICHK(upload(ctx, ctx->fs_src, fs_src));
  }
  FSICHK(upload(ctx, ctx->snode, snode));
  FSICHK(upload(ctx, ctx->ss_rowptr, ss_rowptr));
  FSICHK(upload(ctx, ctx->ss_diagpos, ss_diagpos));
  FSICHK(upload(ctx, ctx->ss_cols, ss_cols));
  FSICHK(upload(ctx, ctx->ss_src, ss_src));
  HIPCHK(ctx->ss_vals.alloc(ss_cols.size()));
  for (SweepSamples* s : {&ctx->smp_ss, &ctx->smp_db, &ctx->smp_sc, &ctx->smp_sch}) HIPCHK(s->create());
  FSICHK(upload(ctx, ctx->mask_s, ms));
  FSICHK(upload(ctx, ctx->mask_f, mf));
  return FSI_OK;
}

// produces: rowptr_pv / rowptr_pp / cols_pp, the 3x3-blocked and the v-p / p-v structures, the value arrays of the node-pair copies
static int build_pressure_blocks(FsiCtx* ctx, const Setup& s) {
  const int64_t V = ctx->V, N2 = ctx->N2;
  const int64_t nadj_total = ctx->h_nadj_ptr[N2], padj_total = ctx->h_padj_ptr[N2];
  std::vector<int64_t> rowptr_pv(V + 1, 0), rowptr_pp(V + 1, 0), diagpos_pp(V, 0);
  for (int64_t q = 0; q < V; ++q) {
    const int32_t r = s.prow_rank[q];
    rowptr_pv[q + 1] = rowptr_pv[q] + 3 * (ctx->h_nadj_ptr[r + 1] - ctx->h_nadj_ptr[r]);
    rowptr_pp[q + 1] = rowptr_pp[q] + (ctx->h_padj_ptr[r + 1] - ctx->h_padj_ptr[r]);
  }
  std::vector<int32_t> cols_pp(rowptr_pp[V]);
  for (int64_t q = 0; q < V; ++q) {
    const int32_t r = s.prow_rank[q];
    const int64_t a = ctx->h_padj_ptr[r], len = ctx->h_padj_ptr[r + 1] - a;
    bool found = false;
    for (int64_t k = 0; k < len; ++k) {
      cols_pp[rowptr_pp[q] + k] = ctx->h_padj[a + k];
      if (ctx->h_padj[a + k] == q) { diagpos_pp[q] = rowptr_pp[q] + k; found = true; }
    }
    if (!found) { ctx->err = "fsi_create: vertex missing from its own neighbour list"; return FSI_ERR_INVALID; }
  }
  FSICHK(upload(ctx, ctx->rowptr_pv, rowptr_pv));
  FSICHK(upload(ctx, ctx->rowptr_pp, rowptr_pp));
  FSICHK(upload(ctx, ctx->diagpos_pp, diagpos_pp));
  FSICHK(upload(ctx, ctx->cols_pp, cols_pp));
  HIPCHK(ctx->rowptr3.alloc(3 * N2 + 1));
  HIPCHK(ctx->diagpos3.alloc(3 * N2));
  HIPCHK(ctx->cols3.alloc(9 * nadj_total));
  HIPCHK(ctx->rowptr_vp.alloc(3 * N2 + 1));
  HIPCHK(ctx->cols_vp.alloc(3 * padj_total));
  HIPCHK(ctx->cols_pv.alloc(rowptr_pv[V]));
  launch_block_structure(ctx->stream, N2, V, ctx->nadj_ptr.p, ctx->nadj.p, ctx->padj_ptr.p, ctx->padj.p, ctx->vrank.p,
                         ctx->rowptr3.p, ctx->cols3.p, ctx->diagpos3.p, ctx->rowptr_vp.p, ctx->cols_vp.p,
                         ctx->rowptr_pv.p, ctx->cols_pv.p);
  HIPCHK(hipGetLastError());
  HIPCHK(ctx->Adv.alloc(9 * nadj_total));
  HIPCHK(ctx->dd_db.alloc(3 * nadj_total));
  HIPCHK(ctx->vv_db.alloc(3 * nadj_total));
  HIPCHK(ctx->adv_db.alloc(3 * nadj_total));
  HIPCHK(ctx->dd_db32.alloc(3 * nadj_total));
  HIPCHK(ctx->vv_db32.alloc(3 * nadj_total));
  HIPCHK(ctx->dd_dinv32.alloc(4 * N2));
  HIPCHK(ctx->dd_chat.alloc(nadj_total));
  HIPCHK(ctx->dd_rowflag.alloc(3 * N2));
  return FSI_OK;
}

// LDS tiles of a graph: per tile of `rows_per_tile` consecutive rows the sorted distinct columns (ulist, tile t at uptr[t] .. uptr[t + 1])
// and per entry its column's 16-bit index in that list (ploc).  Not ok: a tile has more than `limit` columns; max_nu is of the tiles before it.
struct Tiles { bool ok = true; int max_nu = 0; std::vector<int64_t> uptr; std::vector<int32_t> ulist; std::vector<uint16_t> ploc; };
static Tiles build_tiles(const std::vector<int64_t>& ptr, const std::vector<int32_t>& col, int64_t nrows, int rows_per_tile, int64_t limit) {
  Tiles t;
  const int64_t ntiles = (nrows + rows_per_tile - 1) / rows_per_tile;
  t.uptr.assign(ntiles + 1, 0); t.ploc.resize(ptr[nrows]);
  std::vector<int32_t> tmpu;
  for (int64_t k = 0; k < ntiles; ++k) {
    const int64_t r0 = k * rows_per_tile, r1 = std::min<int64_t>(nrows, r0 + rows_per_tile);
    const int64_t e0 = ptr[r0], e1 = ptr[r1];
    tmpu.assign(col.begin() + e0, col.begin() + e1);
    std::sort(tmpu.begin(), tmpu.end());
    tmpu.erase(std::unique(tmpu.begin(), tmpu.end()), tmpu.end());
    if ((int64_t)tmpu.size() > limit) { t.ok = false; break; }
    t.max_nu = std::max<int>(t.max_nu, (int)tmpu.size());
    for (int64_t e = e0; e < e1; ++e)
      t.ploc[e] = (uint16_t)(std::lower_bound(tmpu.begin(), tmpu.end(), col[e]) - tmpu.begin());
    t.ulist.insert(t.ulist.end(), tmpu.begin(), tmpu.end());
    t.uptr[k + 1] = (int64_t)t.ulist.size();
  }
  return t;
}

// produces: tile_uptr / tile_ulist / tile_ploc - the LDS tiles of the node graph (tiled = false: a tile too large, or switched off)
static int build_node_tiles(FsiCtx* ctx) {
  // nodes per tile (FsiTuning.tile_nodes; 0 = 256): 128 makes no difference at 140 k tets (49.7 against 49.9 ms per step) and
  // costs 1.5 % at 1.12 M tets (round 4 scan, profiles/r04_tile_scan.txt)
  const int TN = (ctx->tune.tile_nodes == 128 || ctx->tune.tile_nodes == 256) ? ctx->tune.tile_nodes : 256;
  ctx->tile_nodes = TN;
  if (ctx->tune.tiles == 0) return FSI_OK;
  const Tiles t = build_tiles(ctx->h_nadj_ptr, ctx->h_nadj, ctx->N2, TN, tile_limit());
  ctx->tiled = t.ok;
  ctx->tile_max_nu = t.max_nu;
  if (!t.ok) return FSI_OK;
  FSICHK(upload(ctx, ctx->tile_uptr, t.uptr));
  FSICHK(upload(ctx, ctx->tile_ulist, t.ulist));
  FSICHK(upload(ctx, ctx->tile_ploc, t.ploc));
  if (getenv("FSI_DEBUG_PRECOND")) {
    const int64_t ntiles = (int64_t)t.uptr.size() - 1;
    std::vector<int> sorted_nu(ntiles);
    for (int64_t k = 0; k < ntiles; ++k) sorted_nu[k] = (int)(t.uptr[k + 1] - t.uptr[k]);
    std::sort(sorted_nu.begin(), sorted_nu.end());
    fprintf(stderr, "[precond] tiles: %lld, distinct neighbours median %d, 90%% %d, max %d\n", (long long)ntiles,
            sorted_nu[(size_t)(ntiles / 2)], sorted_nu[(size_t)((ntiles - 1) * 9 / 10)], ctx->tile_max_nu);
  }
  return FSI_OK;
}

// P2 -> P1 hierarchy on one numbering of `nf` fine nodes.  from[2 i], from[2 i + 1]: the two fine nodes that fine node i interpolates
// between - i itself twice: a vertex, which is a coarse node; negative: an end outside the numbering.  fptr / fcol: the fine graph.
// Coarse nodes = the vertices in fine order (cfine); par / pw [nf][2]: parents and weights (vertex 1, 0; edge node 1/2, 1/2); chptr /
// child / chw: their transpose; cptr / ccol: the coarse graph.  Not ok when an end of an edge node is missing or is no vertex.
struct Hierarchy { bool ok = false; int64_t nc = 0; std::vector<int32_t> par, child, ccol, cfine; std::vector<float> pw, chw; std::vector<int64_t> chptr, cptr; };
static Hierarchy build_hierarchy(int64_t nf, const std::vector<int32_t>& from, const std::vector<int64_t>& fptr, const std::vector<int32_t>& fcol) {
  Hierarchy h;
  auto& [ok, nc, par, child, ccol, cfine, pw, chw, chptr, cptr] = h;
  std::vector<int32_t> cidx(nf, -1);
  for (int64_t i = 0; i < nf; ++i)
    if (from[2 * i] == i) { cidx[i] = (int32_t)cfine.size(); cfine.push_back((int32_t)i); }
  nc = (int64_t)cfine.size();
  par.resize(2 * (size_t)nf); pw.resize(2 * (size_t)nf); chptr.assign(nc + 1, 0);
  for (int64_t i = 0; i < nf; ++i) {
    if (cidx[i] >= 0) { par[2 * i] = par[2 * i + 1] = cidx[i]; pw[2 * i] = 1.f; pw[2 * i + 1] = 0.f; chptr[cidx[i] + 1] += 1; }
    else {
      const int32_t a = from[2 * i], b = from[2 * i + 1];
      if (a < 0 || b < 0 || cidx[a] < 0 || cidx[b] < 0) return h;
      par[2 * i] = cidx[a]; par[2 * i + 1] = cidx[b];
      pw[2 * i] = pw[2 * i + 1] = 0.5f;
      chptr[par[2 * i] + 1] += 1; chptr[par[2 * i + 1] + 1] += 1;
    }
  }
  for (int64_t i = 0; i < nc; ++i) chptr[i + 1] += chptr[i];
  child.resize(chptr[nc]); chw.resize(chptr[nc]);
  std::vector<int64_t> fill(chptr.begin(), chptr.end() - 1);
  for (int64_t i = 0; i < nf; ++i)
    for (int k = 0; k < 2; ++k)
      if (pw[2 * i + k] != 0.f) { const int64_t pos = fill[par[2 * i + k]]++; child[pos] = (int32_t)i; chw[pos] = pw[2 * i + k]; }
  cptr.assign(nc + 1, 0);
  for (int64_t I = 0; I < nc; ++I) {
    const int64_t i = cfine[I];
    for (int64_t e = fptr[i]; e < fptr[i + 1]; ++e)
      if (cidx[fcol[e]] >= 0) ccol.push_back(cidx[fcol[e]]);      // ascending: fine indices ascend, cidx is monotone
    cptr[I + 1] = (int64_t)ccol.size();
  }
  ok = true;
  return h;
}

// produces: the P2 -> P1 hierarchies of the displacement block (mg_*) and of the solid block on its compact numbering (sbmg_*, bcr)
static int build_hierarchies(FsiCtx* ctx, const Setup& s) {
  const int64_t V = ctx->V, N2 = ctx->N2, C = ctx->C, nS = ctx->nS;
  const int32_t* tn = ctx->h_tet_nodes.data(); const std::vector<int32_t>& rk = ctx->h_node2rank;
  std::vector<float> ones(4 * N2, 1.0f);
  for (int64_t i = 0; i < N2; ++i) ones[4 * i + 3] = 0.0f;
  FSICHK(upload(ctx, ctx->ones32, ones));
  std::vector<int32_t> from(2 * (size_t)N2, -1);      // by rank: the ranks of an edge node's end vertices (from the last cell that holds the edge), a vertex' own rank
  for (int64_t r = 0; r < N2; ++r)
    if (ctx->h_rank2node[r] < V) from[2 * r] = from[2 * r + 1] = (int32_t)r;
  for (int64_t c = 0; c < C; ++c)
    for (int e = 0; e < 6; ++e) {
      const int64_t r = rk[tn[10 * c + 4 + e]];
      from[2 * r] = rk[tn[10 * c + TET_EDGES[e][0]]];
      from[2 * r + 1] = rk[tn[10 * c + TET_EDGES[e][1]]];
    }
  const Hierarchy h = build_hierarchy(N2, from, ctx->h_nadj_ptr, ctx->h_nadj);
  if (!h.ok || h.nc != V) { ctx->dd_mg = 0; return FSI_OK; }      // one-level sweeps; the solid level is not attempted
  const int64_t nc = h.nc;
  ctx->mg_nc = nc;
  ctx->mg_cnnz = (int64_t)h.ccol.size();
  FSICHK(upload(ctx, ctx->mg_par, h.par));     FSICHK(upload(ctx, ctx->mg_pw, h.pw));
  FSICHK(upload(ctx, ctx->mg_chptr, h.chptr)); FSICHK(upload(ctx, ctx->mg_child, h.child)); FSICHK(upload(ctx, ctx->mg_chw, h.chw));
  FSICHK(upload(ctx, ctx->mg_cptr, h.cptr));   FSICHK(upload(ctx, ctx->mg_ccol, h.ccol));   FSICHK(upload(ctx, ctx->mg_cfine, h.cfine));
  HIPCHK(ctx->mg_Ac.alloc(ctx->mg_cnnz));
  HIPCHK(ctx->mg_cc.alloc(ctx->mg_cnnz));
  HIPCHK(ctx->mg_d0.alloc(N2));
  HIPCHK(ctx->mg_dcinv4.alloc(4 * nc));
  HIPCHK(ctx->mg_cflag.alloc(3 * nc));
  HIPCHK(ctx->mg_work.alloc(5 * 4 * nc));
  std::vector<float> cones(4 * (size_t)nc, 1.0f);
  for (int64_t i = 0; i < nc; ++i) cones[4 * i + 3] = 0.0f;
  FSICHK(upload(ctx, ctx->mg_cones, cones));
  if (!ctx->solid_mg || nS == 0) return FSI_OK;
  std::vector<int32_t> sfrom(2 * (size_t)nS);         // the same by compact solid index (-1: an end vertex outside the solid set)
  for (int64_t i = 0; i < nS; ++i)
    for (int k = 0; k < 2; ++k) sfrom[2 * i + k] = s.sidx[from[2 * (size_t)s.snode[i] + k]];
  const Hierarchy sh = build_hierarchy(nS, sfrom, s.sb_ptr, s.sb_col);
  if (!sh.ok || sh.nc == 0) { ctx->solid_mg = 0; return FSI_OK; }
  const int64_t nsc = sh.nc;
  ctx->sbmg_nc = nsc;
  ctx->sbmg_nblk = (int64_t)sh.ccol.size();
  FSICHK(upload(ctx, ctx->sbmg_par, sh.par));     FSICHK(upload(ctx, ctx->sbmg_pw, sh.pw));
  FSICHK(upload(ctx, ctx->sbmg_chptr, sh.chptr)); FSICHK(upload(ctx, ctx->sbmg_child, sh.child)); FSICHK(upload(ctx, ctx->sbmg_chw, sh.chw));
  FSICHK(upload(ctx, ctx->sbmg_cptr, sh.cptr));   FSICHK(upload(ctx, ctx->sbmg_ccol, sh.ccol));   FSICHK(upload(ctx, ctx->sbmg_cfine, sh.cfine));
  HIPCHK(ctx->sbmg_cvals.alloc(9 * sh.ccol.size()));
  HIPCHK(ctx->sbmg_cbinv12.alloc(12 * nsc));
  HIPCHK(ctx->sbmg_flag.alloc(nS));
  HIPCHK(ctx->sbmg_cflag.alloc(nsc));
  HIPCHK(ctx->sbmg_work.alloc(5 * 4 * nsc));
  if (ctx->solid_coarse_exact) FSICHK(bcr_plan(ctx, nsc, sh.cptr, sh.ccol, nullptr));     // (leaves ctx->bcr null when the level does not suit it)
  return FSI_OK;
}

// produces: the value arrays of the field blocks; s_* - the explicit Schur complement's pattern (vertices that share a velocity
// node's element neighbourhood) and its tiles
static int build_schur_pattern(FsiCtx* ctx, const Setup& s) {
  const int64_t V = ctx->V, N2 = ctx->N2, nadj_total = ctx->h_nadj_ptr[N2], padj_total = ctx->h_padj_ptr[N2];
  HIPCHK(ctx->vvf_dinv32.alloc(4 * N2));
  HIPCHK(ctx->Avp.alloc(3 * padj_total));
  HIPCHK(ctx->Apv.alloc(ctx->cols_pv.n));
  HIPCHK(ctx->App.alloc(ctx->cols_pp.n));
  for (SubMat* M : {&ctx->Mdd, &ctx->Mvv}) {
    M->n = 3 * N2; M->nnz = 9 * nadj_total;
    M->rowptr = ctx->rowptr3.p; M->cols = ctx->cols3.p; M->diagpos = ctx->diagpos3.p;
    HIPCHK(M->vals.alloc(M->nnz));
  }
  std::vector<int64_t> s_rowptr(V + 1, 0), s_diagpos(V, 0);
  std::vector<int32_t> s_cols, mark(V, -1), row;
  s_cols.reserve((size_t)V * 64);
  for (int64_t q = 0; q < V; ++q) {
    const int32_t r = s.prow_rank[q];
    row.clear();
    for (int64_t kb = ctx->h_nadj_ptr[r]; kb < ctx->h_nadj_ptr[r + 1]; ++kb) {
      const int32_t b = ctx->h_nadj[kb];
      for (int64_t t = ctx->h_padj_ptr[b]; t < ctx->h_padj_ptr[b + 1]; ++t) {
        const int32_t u = ctx->h_padj[t];
        if (mark[u] != (int32_t)q) { mark[u] = (int32_t)q; row.push_back(u); }
      }
    }
    std::sort(row.begin(), row.end());
    for (size_t t = 0; t < row.size(); ++t)
      if (row[t] == (int32_t)q) s_diagpos[q] = (int64_t)s_cols.size() + (int64_t)t;
    s_cols.insert(s_cols.end(), row.begin(), row.end());
    s_rowptr[q + 1] = (int64_t)s_cols.size();
  }
  FSICHK(upload(ctx, ctx->s_rowptr, s_rowptr));
  FSICHK(upload(ctx, ctx->s_diagpos, s_diagpos));
  FSICHK(upload(ctx, ctx->s_cols, s_cols));
  HIPCHK(ctx->s_vals.alloc(s_cols.size()));
  // rows per tile (FsiTuning.schur_tile_rows; 0 = 64).  A sweep is a chain of dependent steps per workgroup (stage the tile's
  // distinct columns, 32 rows per pass, update) and the data is on die, so shorter chains in more workgroups win: round 4
  // scan, ms per preconditioner application with 64 / 128 / 256 rows: 1.10 / 1.13 / 1.28 at 140 k tets (24 k rows: 94 tiles
  // of 256 rows are fewer than the chip has CUs), 3.97 / 4.02 / 3.99 at 1.12 M tets (profiles/r04_tile_scan.txt)
  const int want = ctx->tune.schur_tile_rows;
  const int TR = (want == 32 || want == 64 || want == 128 || want == 256) ? want : 64;
  ctx->schur_tile = TR;
  const Tiles t = build_tiles(s_rowptr, s_cols, V, TR, 7000);          // 56 KB of LDS as doubles
  ctx->schur_tiled = t.ok && V > 0;
  ctx->s_tile_max_nu = t.max_nu;
  if (ctx->schur_tiled) {
    FSICHK(upload(ctx, ctx->s_tile_uptr, t.uptr));
    FSICHK(upload(ctx, ctx->s_tile_ulist, t.ulist));
    FSICHK(upload(ctx, ctx->s_ploc, t.ploc));
  }
  HIPCHK(ctx->blk.alloc((size_t)20 * 3 * N2 + 16));
  return FSI_OK;
}

// produces: the Krylov store, sized from `free_b` bytes of free device memory (the recycled directions are what 288 GB of HBM are used for)
static int size_krylov_store(FsiCtx* ctx, size_t free_b) {
  const int64_t n = ctx->ndof;
  ctx->debug_gcr = getenv("FSI_DEBUG_GCR") != nullptr;
  ctx->debug_prec_apply = (getenv("FSI_DEBUG_PRECOND") && atoi(getenv("FSI_DEBUG_PRECOND")) >= 2) ? 12 : 0;
  ctx->ldq = (n + 3) & ~(int64_t)3;
  ctx->ldz = (n + 1) & ~(int64_t)1;
  const double per_dir = (double)ctx->ldz * 8.0 + (double)ctx->ldq * (ctx->kry_fp32_policy == 1 ? 4.0 : 8.0);
  int64_t cap = (int64_t)((double)free_b * 0.5 / per_dir);
  // 600 kept directions (round 2: 400): a Jacobian's life of 20 steps makes ~380 early in a run and ~550 once the ramp is up
  // (4.6 Newton iterations per step); a full store rotates, and the 100-step run is 5 % faster without that (12.0 against
  // 11.4 Newton-it/s); the 20-step bench does not notice.  Half of the free HBM remains the upper limit.
  cap = std::max<int64_t>(8, std::min<int64_t>(cap, ctx->tune.krylov_capacity));
  ctx->kry.init(cap);
  HIPCHK(ctx->KZ.alloc((size_t)cap * ctx->ldz));
  HIPCHK(ctx->KQ.alloc((size_t)cap * ctx->ldq * (ctx->kry_fp32_policy == 1 ? 4 : 8)));      // FP64-sized unless FP32 is forced
  HIPCHK(ctx->hcoef.alloc(gcr_coef_len(cap)));
  if (ctx->kry_fp32_policy != 0) { HIPCHK(ctx->KQh.alloc((size_t)GCR_WINDOW * ctx->ldq)); HIPCHK(ctx->hcoef_hot.alloc(gcr_coef_len(GCR_WINDOW))); }
  HIPCHK(ctx->gcr_out.alloc(8));
  HIPCHK(ctx->gcr_y.alloc(cap));
  HIPCHK(ctx->gcr_cn.alloc((size_t)GCR_FLUSH_BATCH * cap));
  HIPCHK(ctx->gcr_slots.alloc(GCR_FLUSH_BATCH));
  HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&ctx->gcr_host), GcrStaging{cap}.size() * sizeof(double), hipHostMallocDefault));
  gcr_reset(ctx);
  HIPCHK(ctx->scratch.alloc(std::max<size_t>(24576, (size_t)(cap + 2) * 256 + 16)));
  return FSI_OK;
}

}  // namespace

FsiCtx::~FsiCtx() {
  if (gcr_host) (void)hipHostFree(gcr_host);
  rccl_destroy(this);
  bcr_free(this);
  auto drop = [](hipEvent_t* e, int n) { for (int k = 0; k < n; ++k) if (e[k]) (void)hipEventDestroy(e[k]); };
  for (SweepSamples* s : {&smp_ss, &smp_db, &smp_sc, &smp_sch}) s->destroy();
  for (PhaseTimer* t : {&t_res, &t_jac, &t_fac, &t_spmv, &t_prec, &t_ortho, &t_flush, &t_kry}) { drop(t->e0, PhaseTimer::RING); drop(t->e1, PhaseTimer::RING); }
  for (hipEvent_t* e : {&ev0, &ev1, &ev_split, &ev_solid, &ev_b}) drop(e, 1);
  if (stream2) (void)hipStreamDestroy(stream2);
  if (stream) (void)hipStreamDestroy(stream);
}

extern "C" {

int fsi_destroy(FsiCtx* ctx) {
  if (!ctx) return FSI_OK;
  (void)hipSetDevice(ctx->device);
  (void)hipDeviceSynchronize();
  delete ctx;
  return FSI_OK;
}

int fsi_create(const FsiMeshDesc* mesh, const FsiParams* prm, int device, FsiCtx** out) {
  FsiTuning t;
  fsi_tuning_from_env(&t);        // defaults + the FSI_<NAME> overrides of the environment (csrc/fsi_tuning.hip)
  return fsi_create_tuned(mesh, prm, device, &t, out);
}

int fsi_create_tuned(const FsiMeshDesc* mesh, const FsiParams* prm, int device, const FsiTuning* tuning, FsiCtx** out) {
  if (!mesh || !prm || !out) return FSI_ERR_INVALID;
  *out = nullptr;
  FsiCtx* ctx = new FsiCtx();
  *out = ctx;   // returned even on failure so that fsi_last_error() can be read; caller destroys it
  Setup s;
  FSICHK(check_inputs(ctx, mesh, prm, device, tuning));
  FSICHK(open_device(ctx, device));
  copy_problem(ctx, mesh, prm);
  FSICHK(number_nodes(ctx, mesh, s));
  FSICHK(build_node_graph(ctx, s));
  build_element_tables(ctx, s);
  if (!ctx->tune.assembly_atomic) {      // reproducible assembly: coloured Jacobian launches, residual summed per dof in cell order
    FSICHK(colour_cells(ctx, s));
    FSICHK(residual_incidences(ctx, s));
  }
  FSICHK(upload_structure(ctx, mesh, s));
  FSICHK(build_solid_blocks(ctx, mesh, s));
  FSICHK(build_pressure_blocks(ctx, s));
  FSICHK(build_node_tiles(ctx));
  FSICHK(build_hierarchies(ctx, s));
  FSICHK(build_schur_pattern(ctx, s));
  HIPCHK(hipMemsetAsync(ctx->A_pre.p, 0, ctx->nnz * sizeof(double), ctx->stream));
  HIPCHK(ctx->iflags.alloc(FsiCtx::IFLAG_BCMASK + ctx->ndof));
  // Krylov space: sized from free memory, after every other allocation
  size_t free_b = 0, total_b = 0;
  HIPCHK(hipMemGetInfo(&free_b, &total_b));
  ctx->kry_fp32 = ctx->kry_fp32_policy == 1;
  if (ctx->prod.policy32 && ctx->kry_fp32_policy != 0) {
    FSICHK(ctx->prod.layout(ctx, s.rowptr));      // the FP32 copy of the monolithic operator
    HIPCHK(hipMemGetInfo(&free_b, &total_b));
  }
  FSICHK(size_krylov_store(ctx, free_b));
  HIPCHK(hipStreamSynchronize(ctx->stream));
  return FSI_OK;
}

}  // extern "C"
