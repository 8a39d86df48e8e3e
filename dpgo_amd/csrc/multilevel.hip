// multilevel.hip -- the multilevel preconditioner: hierarchy set-up and V-cycle launches (stands in for src/PoseGraph.cpp:598-613, src/QuadraticProblem.cpp:56-69).
#include "host.h"

namespace dpgo_host {

// ---------------------------------------------------------------------------------------------------------
// Multilevel preconditioner: hierarchy setup (symbolic on the host once per block pattern, numeric on the device
// for every new set of Q values) and the per-iteration launches.  DESIGN.md section 5.
int ml_tile(int b, int split) { return (64 / (b * split)) * kWaves; }
// tiles of the additive preconditioner's layout (4 lane groups per pose, one tile = one aggregate per workgroup)
int additive_tile(const dpgo_problem_s* p) { return ml_tile(p->b, 4); }
int ml_level_split(int n) { return n < 40000 ? 4 : 1; }

// Aggregate sizes per coarsening.  Every k must divide the workgroup tile of its level (fused restriction); the
// coarsest operator is a dense inverse of at most kMlDense unknowns (Infinity-Cache resident), kMlDenseMax if that is
// what it takes to get there in one coarsening; otherwise one more level.
constexpr int kMlDense = 3200, kMlDenseMax = 6400;
// Two-level hierarchies use GRAPH aggregates (a single negative entry -S: breadth-first-grown aggregates of at most S
// poses, grow_aggregates) whenever one coarsening with S <= kMlGraphMax reaches a dense level of about 2 500
// unknowns: compact aggregates need 40-60 % of the Hessian-vector products that index runs of the same size need
// (DESIGN.md section 5), and the dense level can then be small.  DPGO_ML_GRAPH=0: index runs as before.
constexpr int kMlGraphMax = 512, kMlGraphUnknownsPerPose = 1600;
int ml_default_graph_size(int n, int b) {
  if (options().ml_graph == 0) return 0;
  if (options().ml_graph_size >= 2) return options().ml_graph_size;  // experiments: force the size
  const long long S = std::max<long long>(4, ((long long)n * b + kMlGraphUnknownsPerPose - 1) / kMlGraphUnknownsPerPose);
  return S <= kMlGraphMax ? (int)S : 0;
}
// Blocks whose plain greedy growth would use aggregates of >= kMlMergeFrom poses (n (d+1) >= ~100 000 unknowns: >= 25 600
// poses in 3-D) grow them to S = ceil(n (d+1) / 2 200) instead and MERGE the growth's fragments up to 3 S / 2
// (merge_small_aggregates): the aggregates come out uniform (mean ~ S instead of ~0.55 S with a tail of fragments), the
// same coarse-space quality needs a quarter fewer of them -- 100k poses: 546 aggregates / 70 products to |rgrad| < 1e-2
// against 732 / 77, a dense level of 38 MB instead of 69 MB; 25k: 536 / 87 against 589 / 93 (oracle, round 4).  Round 5:
// from a plain growth size of 12 on (n (d+1) > ~17 600 unknowns: >= 4 400 poses in 3-D) -- torus3D 38 -> 35 products
// (exact factor: 22; S = 6 / cap 9: 29 with 814 aggregates, S = 4 / cap 6: 28 with 1 215 aggregates = a dense level of 4 860
// unknowns, 189 MB, whose stream costs what the ten products save), 6 250-pose grid 50 -> 42, 12 500-pose slab 140 -> ~105
// (oracle, tools/balanced_aggregates_experiment.py ... vcycle).  Smaller blocks keep the plain growth (sphere2500: 364 aggregates / 32 products against 417 / 49 merged;
// their hierarchies are what the committed vectors pin).
constexpr int kMlMergeFrom = 12, kMlMergedUnknownsPerPose = 2200;
std::vector<int> ml_default_ks(int n, int b, int split0) {
  if (const int S = ml_default_graph_size(n, b)) {
    const bool forced = options().ml_graph_size >= 2;
    if (!forced && S >= kMlMergeFrom) {
      const int Sm = (int)(((long long)n * b + kMlMergedUnknownsPerPose - 1) / kMlMergedUnknownsPerPose);
      const int cap = Sm + Sm / 2;
      if (cap <= kMlGraphMax) return std::vector<int>{-Sm, -cap};
    }
    return std::vector<int>{-S};
  }
  std::vector<int> ks;
  int cur = n, split = split0;
  for (int guard = 0; guard < 16; ++guard) {
    const int P = ml_tile(b, split);
    int pick = 0;
    for (int limit : {kMlDense, kMlDenseMax}) {
      for (int k = 4; k <= P && !pick; ++k)
        if (P % k == 0 && (long long)((cur + k - 1) / k) * b <= limit) pick = k;
      if (pick) break;
    }
    if (pick) {
      ks.push_back(pick);
      return ks;
    }
    int k = 2;
    for (int c = 2; c <= 8; ++c)
      if (P % c == 0) k = c;
    ks.push_back(k);
    cur = (cur + k - 1) / k;
    split = ml_level_split(cur);
  }
  return ks;
}

void ml_free(dpgo_problem_s* p) {
  p->ml_additive_layout = false;
  p->ml.clear();
  p->dense = dpgo_problem_s::DenseLevel();
  p->ml_symbolic = p->ml_ready = false;
  p->ml_ops32_ready = false;
}

// Symbolic setup: level sizes, block patterns of the Galerkin operators, buffers.  The aggregates, patterns and tables are
// aggregation.h's (plain C++ over index vectors); this function decodes the shape, sizes the buffers, starts the jobs that
// overlap, calls those functions and uploads what they return.
// ks_in: aggregate sizes per coarsening; {-S}: two levels, graph aggregates of at most S poses; {-S, -cap}: the same with
// the fragments of the greedy growth merged up to `cap` poses (HierarchySpec).  perm_tile > 0 (graph aggregates): also
// build the (aggregate, slot) -> pose table of the additive preconditioner's persistent layout with that many slots per
// aggregate.
int ml_symbolic_setup(dpgo_problem_s* p, const std::vector<int>& ks_in, int perm_tile) {
  // DPGO_SETUP_TIMING=1: host section times on stderr (where the once-per-pattern cost of the hierarchy goes)
  const bool timing = options().setup_timing != 0;
  auto t_last = std::chrono::steady_clock::now();
  const auto t_first = t_last;
  auto lap = [&](const char* what) {
    if (!timing) return;
    const auto t = std::chrono::steady_clock::now();
    std::fprintf(stderr, "dpgo_hip: symbolic set-up: %-44s %7.3f ms\n", what, 1e3 * std::chrono::duration<double>(t - t_last).count());
    t_last = t;
  };
  ml_free(p);
  lap("previous hierarchy freed");
  if (!p->has_pattern()) return fail(DPGO_ERR_STATE, "multilevel: Q's block pattern is not set");
  HierarchySpec spec;
  std::string why;
  if (!spec.decode(ks_in, &why)) return fail(DPGO_ERR_INVALID, "multilevel: " + why);
  const std::vector<int>& ks = spec.ks;
  const int b = p->b, bb = b * b;
  const size_t nt = p->T;  // doubles per node
  Pattern P = p->h_pattern;  // the current level's operator; every coarsening replaces it by the next level's
  int cur = p->n;
  p->ml.resize(ks.size() + 1);
  for (size_t l = 0; l <= ks.size(); ++l) {
    auto& L = p->ml[l];
    L.n = cur;
    L.split = (l == 0) ? p->split : ml_level_split(cur);
    L.k = (l < ks.size()) ? ks[l] : 0;
    if (l == 0 && spec.graph) {
      Aggregates agg;
      // the level-0 buffers whose sizes are known up front are allocated by a helper thread while the aggregates grow
      int alloc_rc = DPGO_OK;
      std::string alloc_msg;  // (the helper's error text is thread-local to the helper)
      const int dev_ = p->device;
      const int nthreads = setup_threads();
      JobGuard alloc_job{TaskPool::get().submit(1, [&, dev_](int) {
        alloc_rc = [&]() -> int {
          HIPC(hipSetDevice(dev_));
          CHK(L.tbuf.alloc(nt * cur));
          CHK(L.res1.alloc(nt * cur));
          CHK(L.Pb.alloc((size_t)cur * bb));
          CHK(L.x1.alloc(nt * cur));
          CHK(L.x.alloc(nt * cur));
          return DPGO_OK;
        }();
        if (alloc_rc != DPGO_OK) alloc_msg = g_err;
      }, nthreads)};
      if (p->add_plan_known && p->add_agg.S == L.k && p->add_agg.cap == spec.cap && (int)p->add_agg.agg.lab.size() == cur) {
        agg = p->add_agg.agg;  // (the additive plan of this pattern was found with exactly these aggregates)
      } else {
        agg = grow_aggregates(P, L.k, ml_growth_chunks(cur));
        lap("greedy growth of the aggregates");
        if (spec.cap) merge_small_aggregates(P, L.k, spec.cap, ml_growth_chunks(cur), agg);
        lap("merge of the growth's fragments");
      }
      const int na = agg.count();
      L.graph = true;
      L.merge_cap = spec.cap;
      // the patterns that follow from the labels -- A P (rows in parallel) and the dense level's operator (aggregates in
      // parallel) -- are built by worker threads while this one uploads the labels and builds the run and tile tables
      Pattern AP, C;
      JobGuard pattern_job{TaskPool::get().submit(2, [&](int which) {
        if (which == 0)
          AP = ap_pattern(P, agg);
        else
          C = coarse_pattern(P, agg, nthreads / 2);
      }, nthreads)};
      CHK(upload(L.lab, agg.lab.data(), agg.lab.size(), p->stream));
      CHK(upload(L.agg_ptr, agg.ptr.data(), agg.ptr.size(), p->stream));
      CHK(upload(L.agg_mem, agg.mem.data(), agg.mem.size(), p->stream));
      CHK(upload(L.parent, agg.parent.data(), agg.parent.size(), p->stream));
      CHK(upload(L.pslot, agg.pslot.data(), agg.pslot.size(), p->stream));
      const std::vector<int32_t> mpos = member_positions(agg);
      CHK(upload(L.mem_pos, mpos.data(), mpos.size(), p->stream));
      lap("labels, members, trees uploaded");
      std::vector<int32_t> seg_info, seg_ptr, tperm;
      L.nseg = run_table(agg.lab, na, 64 / (b * L.split), seg_info, seg_ptr);
      CHK(upload(L.seg_info, seg_info.data(), seg_info.size(), p->stream));
      CHK(upload(L.seg_ptr, seg_ptr.data(), seg_ptr.size(), p->stream));
      // the layout of the additive preconditioner's persistent kernel: aggregate = workgroup tile of `perm_tile` slots
      if (!perm_tile && !spec.cap && L.k == additive_tile(p)) perm_tile = L.k;
      if (perm_tile) {
        if (std::max(L.k, spec.cap) > perm_tile) return fail(DPGO_ERR_INVALID, "multilevel: aggregates larger than the tile");
        tperm = tile_table(agg, perm_tile);
        CHK(upload(L.tile_perm, tperm.data(), tperm.size(), p->stream));
        L.perm_tile = perm_tile;
      }
      lap("run table, tile table");
      TaskPool::get().wait(pattern_job.job);
      lap("patterns of A P and of the dense level joined");
      CHK(upload_bsr(L.AP, cur, na, (int)AP.colidx.size(), b, AP.rowptr.data(), AP.colidx.data(), nullptr, p->stream));
      lap("A P allocated, pattern uploaded");
      TaskPool::get().wait(alloc_job.job);
      if (alloc_rc != DPGO_OK) return fail(alloc_rc, "level-0 buffers: " + alloc_msg);
      lap("level-0 vectors joined");
      HIPC(hipStreamSynchronize(p->stream));  // the host vectors go out of scope
      lap("stream synchronised");
      P = std::move(C);
      cur = na;
      continue;
    }
    if (L.k) {
      if (L.k < 2 || ml_tile(b, L.split) % L.k)
        return fail(DPGO_ERR_INVALID, "multilevel: aggregate size must divide the workgroup tile of its level (" +
                                          std::to_string(ml_tile(b, L.split)) + " nodes)");
    }
    if (l > 0) {
      CHK(upload_bsr(L.A, cur, cur, (int)P.colidx.size(), b, P.rowptr.data(), P.colidx.data(), nullptr, p->stream));
      const std::vector<int32_t> srow = slot_rows(P);
      CHK(upload(L.slot_row, srow.data(), srow.size(), p->stream));
      HIPC(hipStreamSynchronize(p->stream));  // srow goes out of scope at the end of this block
      CHK(L.r.alloc(nt * cur));
      if (!L.k) CHK(L.x.alloc(nt * cur));  // dense level: its solution, read by the level above
    }
    if (L.k) {  // index runs of k nodes: the same two patterns from their labels
      const Aggregates runs = Aggregates::index_runs(cur, L.k);
      if (l == 0) {
        const Pattern AP = ap_pattern(P, runs);
        CHK(upload_bsr(L.AP, cur, runs.count(), (int)AP.colidx.size(), b, AP.rowptr.data(), AP.colidx.data(), nullptr, p->stream));
        CHK(L.res1.alloc(nt * cur));
      }
      if (l > 0) CHK(L.dinv.alloc((size_t)cur * bb));
      CHK(L.Pb.alloc((size_t)cur * bb));
      CHK(L.x1.alloc(nt * cur));
      CHK(L.x.alloc(nt * cur));
      P = coarse_pattern(P, runs, setup_threads());
      cur = runs.count();
    }
  }
  const int N = cur * b;
  if (N > 16384) return fail(DPGO_ERR_INVALID, "multilevel: dense coarsest operator too large (" + std::to_string(N) +
                                                   " unknowns): use more levels / larger aggregates");
  p->dense.lda = ((N + kNB - 1) / kNB) * kNB;
  // + 8 rows: the apply kernel reads (and discards) the rows of a ghost node behind a ragged last node group
  CHK(p->dense.inv.alloc((size_t)p->dense.lda * (p->dense.lda + 8)));
  CHK(p->dense.inv32.alloc((size_t)p->dense.lda * (p->dense.lda + 8)));
  if (p->ml.size() == 2) {  // two levels: the packed lower triangle and the bookkeeping of k_dense_sym_apply
    const int nT = p->dense.lda / kNB;
    std::vector<DenseChunk> chunks;
    std::vector<int> first;
    dense_chunk_table(nT, options().dense_chunk > 0 ? options().dense_chunk : kDenseChunk, chunks, first);  // (tuning knob)
    p->dense.nchunks = (int)chunks.size();
    CHK(upload(p->dense.chunks, chunks.data(), chunks.size(), p->stream));
    CHK(upload(p->dense.chunk_first, first.data(), first.size(), p->stream));
    CHK(p->dense.packed.alloc((size_t)nT * (nT + 1) / 2 * kNB * kNB));
    CHK(p->dense.pd.alloc((size_t)p->dense.nchunks * kNB * p->r));
    CHK(p->dense.pt.alloc((size_t)nT * p->dense.lda * p->r));
    HIPC(hipStreamSynchronize(p->stream));  // the host vectors go out of scope
  }
  CHK(p->dense.W.alloc((size_t)p->dense.lda * kNB));
  CHK(p->dense.Rx.alloc((size_t)p->dense.lda * kNB));
  HIPC(hipStreamSynchronize(p->stream));
  lap("coarser levels, dense level allocated");
  if (timing)
    std::fprintf(stderr, "dpgo_hip: symbolic set-up: %-44s %7.3f ms\n", "total",
                 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t_first).count());
  p->ml_symbolic = true;
  return DPGO_OK;
}

int flat_grid(size_t items) {
  size_t g = (items + kBlock - 1) / kBlock;
  if (g < 1) g = 1;
  return g < (size_t)kMaxGrid ? (int)g : kMaxGrid;
}

bool gj_use_mfma() {
  return options().gj_mfma != 0;
}

// In-place inverse of the dense SPD lda x lda array M (lda a multiple of 64); W, Rx: lda x 64 panels.
// (Round 6, both measured at 2 184 unknowns = 35 block steps and NOT kept: a look-ahead schedule -- the tiles of block row /
// column kb + 1 first, the rest of the rank-64 update in one launch with the next panel, W / Rx double-buffered, bitwise the
// same result -- 2.80 ms against 2.65 ms: the panel's latency-bound pivot loop runs slower beside 600 update workgroups than
// the launch it saves; the 64 x 64 pivot block by four block steps of 16 pivots -- one wavefront inverting the 16 x 16 block
// with wave barriers only, rank-16 updates on 4 x 4 register tiles, reciprocal by v_rcp_f64 + two Newton steps -- 2.96 ms:
// a pivot's dependent chain (LDS line, reciprocal, quad shuffle, LDS write, barrier) costs the same 0.7 us in a wavefront as
// in a workgroup.)
int dense_spd_inverse(hipStream_t s, double* M, int lda, double* W, double* Rx, bool mfma) {
  const int nt = lda / kNB;
  for (int kb = 0; kb < nt; ++kb) {
    launch(k_sweep_panel, nt, 0, s, M, lda, kb, W, Rx);
    launch(mfma ? k_sweep_update<true> : k_sweep_update<false>, dim3(nt, nt), 0, s, M, lda, kb, W, Rx);
  }
  launch(k_sweep_finish, dim3(nt, nt), 0, s, M, lda);
  HIPC(hipGetLastError());
  return DPGO_OK;
}

template <int D>
int ml_numeric_setup_d(dpgo_problem_s* p) {
  const int nl = (int)p->ml.size();
  long long stride = 1;
  for (int l = 0; l + 1 < nl; ++l) {
    auto& L = p->ml[l];
    auto& C = p->ml[l + 1];
    const long long span = stride * L.k;
    // (the wave-parallel set-up kernels: one wave per aggregate / per coarse slot)
    auto wave_grid = [](int items) { return std::max(1, std::min(kMaxGrid, (items + kWaves - 1) / kWaves)); };
    if (L.graph)
      launch(k_ml_build_P_tree_wave<D>, wave_grid(C.n), 0, p->stream, p->Q.dev(), L.agg_ptr, L.agg_mem, L.parent, L.pslot,
             L.mem_pos, L.Pb, C.n);
    else
      launch(k_ml_build_P<D>, flat_grid(C.n), 0, p->stream, p->Q.dev(), p->n, (int)stride, (int)span, L.Pb, C.n);
    const BsrDev A = (l == 0) ? p->Q.dev() : L.A.dev();
    const bool have_ap = l == 0 && L.AP.vals;
    if (have_ap)  // A P first: the Galerkin operator of a two-level hierarchy is its restriction
      launch(k_ml_build_AP<D>, flat_grid(L.n), 0, p->stream, p->Q.dev(), p->ml_shift, L.Pb, L.agg(), L.n, L.AP.dev(),
             L.AP.vals);
    if (have_ap)
      launch(k_ml_galerkin_ap<D>, wave_grid(C.A.nnzb), 0, p->stream, L.AP.dev(), L.Pb, L.agg(), L.agg_ptr, L.agg_mem, L.n,
             C.slot_row, C.A.colidx, C.A.vals, C.A.nnzb);
    else
      launch(k_ml_galerkin<D>, flat_grid(C.A.nnzb), 0, p->stream, A, (l == 0) ? p->ml_shift : 0.0, L.Pb, L.agg(), L.agg_ptr,
             L.agg_mem, L.n, C.slot_row, C.A.colidx, C.A.vals, C.A.nnzb);
    if (C.k)  // smoother of the next level (level 0 uses the handle's block-Jacobi factors)
      launch(k_build_dinv<D>, flat_grid(C.n), 0, p->stream, C.A.dev(), 0.0, C.dinv, C.n);
    stride = span;
  }
  HIPC(hipGetLastError());
  auto& Lc = p->ml.back();
  const int lda = p->dense.lda, N = Lc.n * p->b;
  HIPC(hipMemsetAsync(p->dense.inv, 0, sizeof(double) * (size_t)lda * (lda + 8), p->stream));
  launch(k_dense_pad_identity, 1, 0, p->stream, p->dense.inv, lda, N);
  launch(k_ml_dense_assemble<D>, flat_grid(Lc.A.nnzb), 0, p->stream, Lc.A.dev(), Lc.slot_row, p->dense.inv, lda, Lc.A.nnzb);
  HIPC(hipGetLastError());
  CHK(dense_spd_inverse(p->stream, p->dense.inv, lda, p->dense.W, p->dense.Rx, gj_use_mfma()));
  if (p->dense.packed) {
    const int nT = lda / kNB;
    launch(k_dense_pack_lower, dim3(nT, nT), 0, p->stream, p->dense.inv, lda, p->dense.packed);
    HIPC(hipGetLastError());
  }
  {  // the fp32 storage of the inverse: what the cycle streams when the dense level is kept in fp32 -- by request
     // (ml_coarse_bits == 32: the fp64 array then keeps the SAME rounded values, so that what dpgo_problem_multilevel_get
     // returns is what the cycle applies) or together with the rest of the cycle's storage (coarse32_active: the fp64
     // array stays exact, the cycle applies its rounding)
    const size_t total = (size_t)lda * (lda + 8);
    if (p->ml_coarse_bits == 32)
      launch(k_dense_round_f32, flat_grid(total), 0, p->stream, p->dense.inv, p->dense.inv32, total);
    else
      launch(k_copy_f32, flat_grid(total), 0, p->stream, p->dense.inv, p->dense.inv32, total);
    HIPC(hipGetLastError());
  }
  return DPGO_OK;
}

// Numeric setup for the CURRENT values of Q (device only; redone after every re-weighting).
int ml_numeric_setup(dpgo_problem_s* p) {
  if (!p->ml_symbolic) return fail(DPGO_ERR_STATE, "multilevel: symbolic setup missing");
  CHK(build_dinv(p, p->ml_shift));
  if (p->d == 2)
    CHK(ml_numeric_setup_d<2>(p));
  else
    CHK(ml_numeric_setup_d<3>(p));
  p->ml_ready = true;
  p->ml_ops32_ready = false;  // (the fp32 copies of A P and the prolongation follow at the next solve that streams them)
  return DPGO_OK;
}

// The hierarchy's shape in the form ml_symbolic_setup takes it.
std::vector<int> ml_current_ks(const dpgo_problem_s* p) {
  std::vector<int> ks;
  for (size_t l = 0; l + 1 < p->ml.size(); ++l) ks.push_back(p->ml[l].graph ? -p->ml[l].k : p->ml[l].k);
  if (p->ml.size() == 2 && p->ml[0].graph && p->ml[0].merge_cap) ks.push_back(-p->ml[0].merge_cap);
  return ks;
}

// Layout of the additive preconditioner inside the one-launch solve (k_rtr_persist<..., ADD>): ONE aggregate per workgroup,
// at most kPersistMax = 256 of them.  Host only, once per block pattern:
//   1. graph aggregates of at most one 4-lane-group tile (16 poses in 3-D), plain greedy growth, while there are <= 256
//      (blocks up to ~3 500 poses: the lowest-latency layout);
//   2. else one pose per (d+1) lanes (tile = 64 poses in 3-D): graph aggregates grown to S poses, fragments merged up to
//      min(tile, 3 S / 2), with the smallest S (from ceil(n / 230) in steps of an eighth) that leaves <= 256 aggregates
//      (12 500-pose slab: S = 55, 230 aggregates; 6 250-pose grid: S = 28, 221) -- blocks up to ~14 000 poses;
//   3. without graph aggregates (DPGO_ML_GRAPH=0): index runs of one tile;
//   4. opt-in (additive_tiles(p) == 2), none of the above fits: graph aggregates of the workgroup's TWO tiles (128 poses in
//      3-D, 168 in 2-D), grown and merged as in 2 with tile = 2 P1 -- blocks up to ~28 000 poses -- if the instance's
//      LDS holds that many aggregates' coarse rows (additive_lds_fits).
int additive_tiles(const dpgo_problem_s* p) {
  const int t = p->add_tiles ? p->add_tiles : options().additive_tiles;
  return t == 2 ? 2 : 1;
}
const dpgo_problem_s::AddPlan& additive_plan(dpgo_problem_s* p) {
  if (p->add_plan_known) return p->add_plan;
  p->add_plan = dpgo_problem_s::AddPlan();
  p->add_plan_known = true;
  auto& A = p->add_agg;
  A = dpgo_problem_s::AggCache();
  if (p->split != 4 || !p->has_pattern()) return p->add_plan;
  const int P4 = ml_tile(p->b, 4), P1 = ml_tile(p->b, 1), P2 = 2 * P1, n = p->n;
  const bool graph_ok = options().ml_graph != 0;
  const Pattern& Q = p->h_pattern;
  const int chunks = ml_growth_chunks(n);
  // the plan of the graph aggregates in A (cases 1, 2, 4)
  auto found = [&](int split, int tile, int na) -> const dpgo_problem_s::AddPlan& {
    p->add_plan = dpgo_problem_s::AddPlan{split, tile, A.S, A.cap, na, true};
    return p->add_plan;
  };
  // the search for at most `want` merged aggregates starts where nine tenths of them hold the block (256: ceil(n / 230))
  auto first_size = [&](int want) { return std::max(8, (n + (want * 9) / 10 - 1) / ((want * 9) / 10)); };
  if (graph_ok) {
    if ((long long)n <= (long long)kPersistMax * P4) {
      A.agg = grow_aggregates(Q, P4, chunks);
      A.S = P4, A.cap = 0;
      if (A.agg.count() <= kPersistMax) return found(4, P4, A.agg.count());
    }
    if ((long long)n <= (long long)kPersistMax * P1) {
      // A handle that is solved next to other handles of the device (dpgo_optimize_device_many: persist_share > 1 when the
      // plan is first asked for) aims at HALF the chip -- every aggregate is a workgroup that owns a CU for the whole solve,
      // so two such solves run side by side instead of taking turns; the product count is a weak function of the aggregate
      // size, the time of an iteration is not a function of how full the tiles are.
      const int want = (p->persist_share > 1 && (long long)n * 10 <= (long long)(kPersistMax / 2) * P1 * 8) ? kPersistMax / 2 : kPersistMax;
      int na = search_merged_aggregates(Q, first_size(want), P1, want, chunks, A.agg, &A.S, &A.cap);
      if (!na && want < kPersistMax)  // (no growth size reaches half the chip: the whole-chip plan)
        na = search_merged_aggregates(Q, first_size(kPersistMax), P1, kPersistMax, chunks, A.agg, &A.S, &A.cap);
      if (na) return found(1, P1, na);
    }
    A = dpgo_problem_s::AggCache();
  }
  if ((n + P4 - 1) / P4 <= kPersistMax)
    p->add_plan = dpgo_problem_s::AddPlan{4, P4, P4, 0, (n + P4 - 1) / P4, false};
  else if ((n + P1 - 1) / P1 <= kPersistMax)
    p->add_plan = dpgo_problem_s::AddPlan{1, P1, P1, 0, (n + P1 - 1) / P1, false};
  if (!p->add_plan.split && graph_ok && additive_tiles(p) == 2 && (long long)n <= (long long)kPersistMax * P2) {
    const int na = search_merged_aggregates(Q, first_size(kPersistMax), P2, kPersistMax, chunks, A.agg, &A.S, &A.cap);
    // (static + coarse-row LDS beyond the CU's: no plan)
    if (na && additive_lds_fits(p, 1, 2, na)) return found(1, P2, na);
    A = dpgo_problem_s::AggCache();
  }
  return p->add_plan;
}

// lane groups per pose of the additive layout the CURRENT two-level hierarchy fits (0: none)
int additive_split_of(const dpgo_problem_s* p) {
  if (!p->ml_symbolic || p->ml.size() != 2 || p->split != 4 || p->ml[1].n > kPersistMax) return 0;
  const auto& L = p->ml[0];
  const int P4 = ml_tile(p->b, 4), P1 = ml_tile(p->b, 1);
  const int tile = L.graph ? (L.tile_perm ? L.perm_tile : 0) : L.k;
  return tile == P4 ? 4 : (tile == P1 || (tile == 2 * P1 && L.graph && additive_tiles(p) == 2) ? 1 : 0);
}
// workgroup tiles per aggregate of that layout (1 or 2)
int additive_mt_of(const dpgo_problem_s* p) {
  return additive_split_of(p) == 1 && p->ml[0].perm_tile == 2 * ml_tile(p->b, 1) ? 2 : 1;
}

// Make the hierarchy match the handle's Q (lazily, like the reference's constructPreconditioner inside the first
// PreConditioner call, src/PoseGraph.cpp:582-586).
int ml_ensure(dpgo_problem_s* p, double shift, bool additive) {
  // the additive preconditioner needs ONE aggregate per workgroup tile of its persistent layout (two levels); a hierarchy
  // the caller set up explicitly is kept if it has that shape, the default one is replaced by the handle's plan
  // (additive_plan) and put back when the V-cycle is asked for again
  if (additive && !additive_split_of(p)) {
    const auto& plan = additive_plan(p);
    if (!plan.split) return fail(DPGO_ERR_UNSUPPORTED, "additive preconditioner: the block does not fit 256 aggregates of one workgroup tile" +
                                                           std::string(additive_tiles(p) == 2 ? " or two" : ""));
    std::vector<int> ks{plan.graph ? -plan.S : plan.S};
    if (plan.graph && plan.cap) ks.push_back(-plan.cap);
    CHK(ml_symbolic_setup(p, ks, plan.graph ? plan.tile : 0));
    if (!additive_split_of(p)) return fail(DPGO_ERR_STATE, "additive preconditioner: hierarchy does not match its plan");
    p->ml_additive_layout = true;
    p->ml_user_ks = false;
  } else if (!additive && p->ml_additive_layout && !p->ml_user_ks) {
    CHK(ml_symbolic_setup(p, ml_default_ks(p->n, p->b, p->split)));
    p->ml_additive_layout = false;
  }
  // level 0 smooths with the handle's shared block-Jacobi factors: a block-Jacobi solve with another shift in between
  // has overwritten them, so they are re-derived for THIS shift even when the hierarchy itself is current (no-op otherwise)
  if (p->ml_ready && p->ml_shift == shift) return build_dinv(p, shift);
  if (!p->ml_symbolic) CHK(ml_symbolic_setup(p, ml_default_ks(p->n, p->b, p->split)));
  p->ml_shift = shift;
  return ml_numeric_setup(p);
}

// The fp32 operator copies of the cycle (dpgo_problem_s::ml_operator_bits): (re)built from the fp64 originals whenever those
// changed -- after the hierarchy's numeric set-up, after the symmetric copy of Q was refreshed -- by the first solve that
// wants them (call after resolve_tcg_storage and ml_ensure; never inside a recorded iteration).
int ml_ops32_ensure(dpgo_problem_s* p) {
  if (!p->ml_ops32_wanted() || p->ml_ops32_ready) return DPGO_OK;
  auto& L0 = p->ml[0];
  const size_t bb = (size_t)p->b * p->b;
  const size_t nu = (size_t)p->sym.nu * bb, nap = (size_t)L0.AP.nnzb * bb, npb = (size_t)L0.n * bb;
  if (!p->sym.uvalsT32) CHK(p->sym.uvalsT32.alloc(nu));
  if (!L0.AP32) CHK(L0.AP32.alloc(nap));
  if (!L0.Pb32) CHK(L0.Pb32.alloc(npb));
  if (!L0.x1f) CHK(L0.x1f.alloc((size_t)L0.n * p->T));
  if (!L0.res1f) CHK(L0.res1f.alloc((size_t)L0.n * p->T));
  auto copy = [&](const double* in, float* out, size_t total) {
    launch(k_copy_f32, flat_grid(total), 0, p->stream, in, out, total);
  };
  copy(p->sym.uvalsT, p->sym.uvalsT32, nu);
  copy(L0.AP.vals, L0.AP32, nap);
  copy(L0.Pb, L0.Pb32, npb);
  HIPC(hipGetLastError());
  p->ml_ops32_ready = true;
  return DPGO_OK;
}

// Dense level + prolongation.  Large coarsest levels: two nodes per workgroup (halves the right-hand-side loads per
// matrix byte); balanced rounds: every workgroup takes the same number of node groups (a ragged last round would leave
// most of the chip idle while the dense inverse streams).
int persist_capacity(int device);  // (two resident slots per CU; below)
// f(Int<NODES>{}, a value of the storage type) for the k_ml_coarse_prolong<D, R, NODES, MT> instances that are compiled:
// 4 / 2 / 1 nodes per workgroup in float and double, 3 in double only
template <class F>
int dispatch_coarse(int nodes, bool f32, F&& f) {
  if (nodes == 4) return f32 ? f(Int<4>{}, float{}) : f(Int<4>{}, double{});
  if (nodes == 3) return f(Int<3>{}, double{});
  if (nodes == 2) return f32 ? f(Int<2>{}, float{}) : f(Int<2>{}, double{});
  return f32 ? f(Int<1>{}, float{}) : f(Int<1>{}, double{});
}
int launch_coarse_prolong(dpgo_problem_s* p, const dpgo_problem_s::MlLevel& L, const dpgo_problem_s::MlLevel& C,
                          const DevState* gate, double* xc_out) {
  const bool f32 = p->coarse32_active();
  // nodes per workgroup (the right-hand side is read once per workgroup): 732 nodes: 1 -> 2: 19.7 -> 17.1 us, 4: 18.1;
  // three (fp64 storage) where that brings the level down to one workgroup per CU in one round: 546 nodes: 2 -> 3:
  // 273 -> 182 workgroups, 13.2 -> 11.6 us, the 100k bench step 4.45 -> 4.33 ms
  const int cus = persist_capacity(p->device) / 2;
  int nodes = C.n >= 512 ? 2 : 1;
  if (nodes == 2 && !f32 && (C.n + 1) / 2 > cus && (C.n + 2) / 3 <= cus) nodes = 3;
  if (const int v = options().coarse_nodes)  // tuning knob
    nodes = (v == 4 || v == 2 || (v == 3 && !f32)) ? v : 1;
  const int groups = (C.n + nodes - 1) / nodes;
  int cap = kMaxGrid;
  if (options().coarse_grid > 0) cap = options().coarse_grid;  // tuning knob
  const int rounds = (groups + cap - 1) / cap;
  const int gc = std::max(1, (groups + rounds - 1) / rounds);
  // non-temporal loads of the inverse whenever the loop's working set does not fit the Infinity Cache (kernel comment)
  int hint = p->beyond_cache();
  if (options().coarse_nt >= 0) hint = options().coarse_nt != 0;  // tuning knob
  CHK(dispatch_dr(p->d, p->r, [&](auto Dc, auto Rc) {
    constexpr int D = decltype(Dc)::value, R = decltype(Rc)::value;
    return dispatch_coarse(nodes, f32, [&](auto Nc, auto mt) {
      using MT = decltype(mt);  // (the inverse and, in the same buffer, the right-hand side are stored in this type)
      const MT* inv;
      if constexpr (std::is_same_v<MT, float>) inv = p->dense.inv32; else inv = p->dense.inv;
      return launch(k_ml_coarse_prolong<D, R, decltype(Nc)::value, MT>, gc, 0, p->stream, inv, p->dense.lda,
                    reinterpret_cast<const MT*>(C.r.get()), L.x1, L.Pb, L.k, L.x, gate, L.n, C.n, xc_out, hint);
    });
  }));
  HIPC(hipGetLastError());
  return DPGO_OK;
}

// Dense level from the packed lower triangle: xc = A_c^-1 rc into C.x (two launches: partial products, fixed-order sums)
int launch_dense_sym(dpgo_problem_s* p, const dpgo_problem_s::MlLevel& C, const DevState* gate) {
  const int N = C.n * p->b, nT = p->dense.lda / kNB;
  auto go = [&](auto Rc) {
    constexpr int R = decltype(Rc)::value;
    launch(k_dense_sym_apply<R>, p->dense.nchunks, 0, p->stream, p->dense.packed, p->dense.chunks, C.r, N, p->dense.lda,
           p->dense.pd, p->dense.pt, gate);
    return launch(k_dense_sym_finish<R>, dim3(nT, 4), 0, p->stream, p->dense.pd, p->dense.pt, p->dense.chunk_first, nT, N,
                  p->dense.lda, C.x, gate);
  };
  switch (p->r) {  // (these two kernels know r alone)
    case 2: CHK(go(Int<2>{})); break;
    case 3: CHK(go(Int<3>{})); break;
    case 4: CHK(go(Int<4>{})); break;
    case 5: CHK(go(Int<5>{})); break;
    case 6: CHK(go(Int<6>{})); break;
    default: return fail(DPGO_ERR_UNSUPPORTED, "unsupported r");
  }
  HIPC(hipGetLastError());
  return DPGO_OK;
}

// f(kernel, Q in the storage it reads, pre-smoothed iterate, prolongation blocks, where the residual is kept) for the level-0
// restriction: the cycle's fp32 copies (operators and vectors, or -- A/B, DPGO_ML_VECTOR_BITS=64 -- operators only), else the
// symmetric copy of Q when the tCG-step kernel reads it, else Q at the handle's split
template <int D, int R, class F>
int dispatch_restrict0(const dpgo_problem_s* p, F&& f) {
  auto& L = p->ml[0];
  double* res_out = p->ml_use_ap() ? L.res1.get() : nullptr;
  if (p->ml_vec32_active()) return f(k_ml_restrict<D, R, 1, BsrSymDev32, float, float>, p->sym.dev32(), L.x1f, L.Pb32, L.res1f);
  if (p->ml_ops32_active()) return f(k_ml_restrict<D, R, 1, BsrSymDev32, float, double>, p->sym.dev32(), L.x1, L.Pb32, res_out);
  if (p->tcg_sym) return f(k_ml_restrict<D, R, 1, BsrSymDev>, p->sym.dev(), L.x1, L.Pb, res_out);
  return dispatch_split(p->split, [&](auto Sc) { return f(k_ml_restrict<D, R, decltype(Sc)::value>, p->Q.dev(), L.x1, L.Pb, res_out); });
}

// Level-0 restriction of the cycle: rc = P^T (r - A x1) into ml[1].r (+ the residual itself for k_ml_post_ap).  Graph
// aggregates: the restriction kernel adds P_i^T res_i up over every run of same-aggregate poses inside a wave's chunk and
// writes one partial sum per run, k_ml_agg_sum adds an aggregate's partial sums up.
int launch_ml_restrict0(dpgo_problem_s* p, const double* r, const DevState* gate, int g0, bool stop_check) {
  auto& L = p->ml[0];
  auto& C = p->ml[1];
  // inside the tCG loop (not after its first update): tCG's residual test one kernel early (TcgStopCheck, multilevel.h);
  // the <r,r> partial sums are the ones k_tcg_update has just left in region B, one per workgroup of ITS grid
  TcgStopCheck stop;
  if (stop_check && gate) {
    CHK(sums_ready(p->pB));
    stop.state = const_cast<DevState*>(gate);
    stop.pin = p->pB.in();
    stop.nb = p->pB.count();
    stop.hflag = p->hflag;
    stop.gen = p->gen;
  }
  float* rc32 = (C.k == 0 && p->coarse32_active()) ? reinterpret_cast<float*>(C.r.get()) : nullptr;
  const double* dnext = C.k ? C.dinv : nullptr;
  CHK(dispatch_dr(p->d, p->r, [&](auto Dc, auto Rc) {
    constexpr int D = decltype(Dc)::value, R = decltype(Rc)::value;
    return dispatch_restrict0<D, R>(p, [&](auto kernel, const auto& A, const auto& x1, const auto& Pb, const auto& res_out) {
      return launch(kernel, g0, 0, p->stream, A, x1, r, Pb, p->ml_shift, L.k, C.r, rc32, dnext, p->ml_omega, C.x1, gate, L.n,
                    res_out, L.tbuf, L.seg_info, stop);
    });
  }));
  if (L.graph)
    CHK(dispatch_dr(p->d, p->r, [&](auto D, auto R) {
      return launch(k_ml_agg_sum<D, R>, std::min(C.n, kMaxGrid), 0, p->stream, L.tbuf, L.seg_ptr, C.n, C.r, rc32, gate);
    }));
  HIPC(hipGetLastError());
  return DPGO_OK;
}

// f(kernel, A P, kept residual, prolongation blocks) for the level-0 post-smoothing through A P: the fp32 copies (and beside
// them the fp32 or the fp64 residual) at one pose per D+1 lanes, the fp64 originals at the handle's split
template <int D, int R, class F>
int dispatch_post_ap(const dpgo_problem_s* p, F&& f) {
  auto& L0 = p->ml[0];
  if (p->ml_ops32_active()) {
    const BsrDev32 ap32{L0.AP.rowptr, L0.AP.colidx, L0.AP32};
    if (p->ml_vec32_active()) return f(k_ml_post_ap<D, R, 1, float, float>, ap32, L0.res1f, L0.Pb32);
    return f(k_ml_post_ap<D, R, 1, float, double>, ap32, L0.res1, L0.Pb32);
  }
  return dispatch_split(p->split, [&](auto Sc) { return f(k_ml_post_ap<D, R, decltype(Sc)::value>, L0.AP.dev(), L0.res1, L0.Pb); });
}

// Level-0 post-smoothing, the cycle's last launch: z = proj_X(M^-1 r), partial sums <r,r>, <z,r> into `sums` (may be NULL:
// none).  A two-level hierarchy goes through A P and the coarse solution (k_ml_post_ap), any other through Q (k_ml_post).
int launch_ml_post0(dpgo_problem_s* p, const double* Xdev, const double* r, double* z, Partials* sums, const DevState* gate) {
  const int g0 = p->grid_post();
  double* pout = nullptr;
  if (sums) CHK(sums_out(*sums, g0, &pout));
  if (p->ml_use_ap()) {
    CHK(dispatch_dr(p->d, p->r, [&](auto Dc, auto Rc) {
      constexpr int D = decltype(Dc)::value, R = decltype(Rc)::value;
      return dispatch_post_ap<D, R>(p, [&](auto kernel, const auto& AP, const auto& res1, const auto& Pb) {
        return launch(kernel, g0, 0, p->stream, AP, Xdev, r, res1, p->ml[1].x, Pb, p->ml[0].agg(), p->dinv, p->ml_omega, z,
                      pout, gate, p->n);
      });
    }));
  } else {
    CHK(dispatch_drs(p->d, p->r, p->ml[0].split, [&](auto D, auto R, auto SPLIT) {
      auto go = [&](auto kernel, const auto& Q) {  // level 0 reads Q: the symmetric copy when the tCG-step kernel does
        return launch(kernel, g0, 0, p->stream, Q, Xdev, p->ml[0].x, r, p->dinv, p->ml_omega, p->ml_shift, z, pout, gate, p->n);
      };
      return p->tcg_sym ? go(k_ml_post<D, R, 1, BsrSymDev>, p->sym.dev()) : go(k_ml_post<D, R, SPLIT>, p->Q.dev());
    }));
  }
  HIPC(hipGetLastError());
  return DPGO_OK;
}

// The launches of one cycle after the pre-smoothing step of level 0 (x1 = w Dinv r is in ml[0].x1):
// z = proj_X(M^-1 r); partial sums <r,r>, <z,r> into `sums` (may be NULL).  `gate`: state record for early exit.
int launch_ml_tail(dpgo_problem_s* p, const double* Xdev, const double* r, double* z, Partials* sums,
                   const DevState* gate, bool stop_check) {
  const int nl = (int)p->ml.size();
  // the dense level reads its right-hand side in the precision its inverse is stored in (same buffer)
  auto rc32_of = [&](const dpgo_problem_s::MlLevel& C) {
    return (C.k == 0 && p->coarse32_active()) ? reinterpret_cast<float*>(C.r.get()) : nullptr;
  };
  auto A_of = [&](int l) { return l == 0 ? p->Q.dev() : p->ml[l].A.dev(); };
  auto r_of = [&](int l) { return l == 0 ? r : (const double*)p->ml[l].r; };
  auto grid_of = [&](const dpgo_problem_s::MlLevel& L) {  // (of a level below 0)
    return std::min(kMaxGrid, pose_tiles(L.n, p->b, L.split));
  };
  const bool ap = p->ml_use_ap();  // two levels: the residual after pre-smoothing is kept, the dense level hands over xc
  CHK(launch_ml_restrict0(p, r, gate, p->grid_restrict(), stop_check));
  for (int l = 1; l + 1 < nl; ++l) {  // down
    auto& L = p->ml[l];
    auto& C = p->ml[l + 1];
    CHK(dispatch_drs(p->d, p->r, L.split, [&](auto D, auto R, auto SPLIT) {
      return launch(k_ml_restrict<D, R, SPLIT>, grid_of(L), 0, p->stream, A_of(l), L.x1, r_of(l), L.Pb, 0.0, L.k, C.r, rc32_of(C),
                    C.k ? C.dinv : nullptr, p->ml_omega, C.x1, gate, L.n, nullptr, nullptr, nullptr, TcgStopCheck());
    }));
  }
  {  // dense level (+ prolongation unless the level above does it itself)
    auto& L = p->ml[nl - 2];
    auto& C = p->ml[nl - 1];
    if (p->ml_use_dense_sym())
      CHK(launch_dense_sym(p, C, gate));
    else
      CHK(launch_coarse_prolong(p, L, C, gate, ap ? C.x : nullptr));
  }
  for (int l = nl - 2; l >= 1; --l) {  // up (two levels: nothing between the dense level and level 0)
    auto& L = p->ml[l];
    auto& F = p->ml[l - 1];
    CHK(dispatch_drs(p->d, p->r, L.split, [&](auto D, auto R, auto SPLIT) {
      return launch(k_ml_post_mid<D, R, SPLIT>, grid_of(L), 0, p->stream, L.A.dev(), L.x, L.r, L.dinv, p->ml_omega, F.x1, F.Pb,
                    F.k, F.x, F.n, gate, L.n);
    }));
  }
  return launch_ml_post0(p, Xdev, r, z, sums, gate);
}

// Stand-alone application z = proj_X(M^-1 v) (QuadraticProblem::PreConditioner outside the tCG loop).
int launch_ml_apply(dpgo_problem_s* p, const double* Xdev, const double* v, double* z) {
  CHK(dispatch_dr(p->d, p->r, [&](auto D, auto R) {
    return launch(k_ml_presmooth<D, R>, p->grid(), 0, p->stream, v, p->dinv, p->ml_omega, p->ml[0].x1, nullptr, p->n);
  }));
  HIPC(hipGetLastError());
  // (outside the tCG loop the cycle reads the fp64 originals: its pre-smoothed iterate was written in fp64 just above)
  p->ml_ops32_suspend = true;
  const int rc = launch_ml_tail(p, Xdev, v, z, nullptr, nullptr);
  p->ml_ops32_suspend = false;
  return rc;
}

}  // namespace dpgo_host

extern "C" {


int dpgo_multilevel_default_ks(int n, int d, int* ks, int* nks) {
  if (n <= 0 || d < 2 || d > 3 || !nks) return fail(DPGO_ERR_INVALID, "bad arguments");
  int split = (n < 40000) ? 4 : 1;
  if (const int v = options().split)
    if (v == 1 || v == 2 || v == 4) split = v;
  const std::vector<int> v = ml_default_ks(n, d + 1, split);
  if (ks)
    for (size_t l = 0; l < v.size() && (int)l < *nks; ++l) ks[l] = v[l];
  *nks = (int)v.size();
  return DPGO_OK;
}


int dpgo_multilevel_graph_aggregates(int n, const int32_t* rowptr, const int32_t* colidx, int max_size, int32_t* label,
                                     int32_t* parent, int* n_aggregates) {
  if (n <= 0 || !rowptr || !colidx || max_size < 2 || !label) return fail(DPGO_ERR_INVALID, "bad arguments");
  const Pattern P{{rowptr, rowptr + n + 1}, {colidx, colidx + rowptr[n]}};
  for (int32_t c : P.colidx)
    if (c < 0 || c >= n) return fail(DPGO_ERR_INVALID, "block column out of range");
  const Aggregates agg = grow_aggregates(P, max_size, ml_growth_chunks(n));
  std::copy(agg.lab.begin(), agg.lab.end(), label);
  if (parent) std::copy(agg.parent.begin(), agg.parent.end(), parent);
  if (n_aggregates) *n_aggregates = agg.count();
  return DPGO_OK;
}


int dpgo_multilevel_merged_aggregates(int n, const int32_t* rowptr, const int32_t* colidx, int max_size, int merge_cap,
                                      int32_t* label, int32_t* parent, int* n_aggregates) {
  if (n <= 0 || !rowptr || !colidx || max_size < 2 || merge_cap < max_size || !label) return fail(DPGO_ERR_INVALID, "bad arguments");
  const Pattern P{{rowptr, rowptr + n + 1}, {colidx, colidx + rowptr[n]}};
  for (int32_t c : P.colidx)
    if (c < 0 || c >= n) return fail(DPGO_ERR_INVALID, "block column out of range");
  Aggregates agg = grow_aggregates(P, max_size, ml_growth_chunks(n));
  const int na = merge_small_aggregates(P, max_size, merge_cap, ml_growth_chunks(n), agg);
  std::copy(agg.lab.begin(), agg.lab.end(), label);
  if (parent) std::copy(agg.parent.begin(), agg.parent.end(), parent);
  if (n_aggregates) *n_aggregates = na;
  return DPGO_OK;
}


int dpgo_problem_additive_plan(dpgo_problem_t p, int* lane_groups, int* tile, int* growth, int* merge_cap, int* aggregates,
                               int* graph) {
  if (!p) return fail(DPGO_ERR_INVALID, "null handle");
  if (!p->has_pattern()) return fail(DPGO_ERR_STATE, "Q's block pattern is not set");
  const auto& plan = additive_plan(p);
  if (lane_groups) *lane_groups = plan.split;
  if (tile) *tile = plan.tile;
  if (growth) *growth = plan.S;
  if (merge_cap) *merge_cap = plan.cap;
  if (aggregates) *aggregates = plan.na;
  if (graph) *graph = plan.graph ? 1 : 0;
  return DPGO_OK;
}


int dpgo_problem_additive_tiles(dpgo_problem_t p, int* tiles) {
  if (!p || !tiles) return fail(DPGO_ERR_INVALID, "null handle / pointer");
  if (*tiles < 0 || *tiles > 2) return fail(DPGO_ERR_INVALID, "additive tiles: 1 or 2 (0 queries)");
  if (*tiles > 0 && *tiles != additive_tiles(p)) {
    p->add_tiles = *tiles;
    p->add_plan_known = false;  // (the plan and the hierarchy built for it follow the new value at the next solve)
    p->add_agg = dpgo_problem_s::AggCache();
    if (p->ml_additive_layout && !p->ml_user_ks) ml_free(p);
  }
  *tiles = additive_tiles(p);
  return DPGO_OK;
}


int dpgo_problem_setup_multilevel(dpgo_problem_t p, int nks, const int* ks, double omega, double shift) {
  CHK(check_ready(p));
  if (nks < 0 || nks > 8 || (nks > 0 && !ks) || !(omega > 0.0) || !(shift >= 0.0))
    return fail(DPGO_ERR_INVALID, "bad multilevel arguments");
  std::vector<int> v = nks > 0 ? std::vector<int>(ks, ks + nks) : ml_default_ks(p->n, p->b, p->split);
  const bool same = p->ml_symbolic && ml_current_ks(p) == v;
  if (!same) {
    // graph aggregates with merged fragments that fit a workgroup tile of the one-launch solve also get that layout's
    // (aggregate, slot) table, so that an explicit hierarchy of this shape serves precond = additive as well
    int perm_tile = 0;
    if (v.size() == 2 && v[0] < 0 && v[1] < 0 && p->split == 4)
      perm_tile = -v[1] <= ml_tile(p->b, 4) ? ml_tile(p->b, 4) : (-v[1] <= ml_tile(p->b, 1) ? ml_tile(p->b, 1) : 0);
    if (!perm_tile && v.size() == 2 && v[0] < 0 && v[1] < 0 && p->split == 4 && additive_tiles(p) == 2 && -v[1] <= 2 * ml_tile(p->b, 1))
      perm_tile = 2 * ml_tile(p->b, 1);  // (the two-tile layout, opt-in)
    CHK(ml_symbolic_setup(p, v, perm_tile));
  }
  p->ml_user_ks = nks > 0;
  p->ml_additive_layout = false;
  p->ml_omega = omega;
  p->ml_shift = shift;
  CHK(ml_numeric_setup(p));
  HIPC(hipStreamSynchronize(p->stream));
  return DPGO_OK;
}


int dpgo_problem_multilevel_path(dpgo_problem_t p, int* flags) {
  if (!p || !flags) return fail(DPGO_ERR_INVALID, "null handle / pointer");
  if (!p->ml_symbolic) return fail(DPGO_ERR_STATE, "multilevel hierarchy not set up");
  *flags = (p->ml_use_ap() ? DPGO_ML_PATH_AP : 0) | (p->ml_use_dense_sym() ? DPGO_ML_PATH_PACKED_DENSE : 0);
  return DPGO_OK;
}


int dpgo_problem_multilevel_coarse_bits(dpgo_problem_t p, int* bits) {
  if (!p || !bits) return fail(DPGO_ERR_INVALID, "null handle / pointer");
  if (*bits < 0) {
    *bits = p->ml_coarse_bits;
    return DPGO_OK;
  }
  if (*bits != 32 && *bits != 64) return fail(DPGO_ERR_INVALID, "the coarsest inverse is stored in 32 or 64 bits");
  if (*bits != p->ml_coarse_bits) {
    p->ml_coarse_bits = *bits;
    p->ml_ready = false;  // the stored inverse is rebuilt at the next use
  }
  return DPGO_OK;
}


int dpgo_problem_multilevel_operator_bits(dpgo_problem_t p, int* bits, int* active) {
  if (!p || !bits) return fail(DPGO_ERR_INVALID, "null handle / pointer");
  if (*bits >= 0) {
    if (*bits != 32 && *bits != 64) return fail(DPGO_ERR_INVALID, "the cycle's operator copies are stored in 32 or 64 bits");
    p->ml_operator_bits = *bits;
  }
  *bits = p->ml_operator_bits;
  // (what the last solve's cycle streamed: 1 operator copies, 2 the cycle's internal vectors, 4 the dense level -- in fp32)
  if (active) *active = (p->ml_ops32_active() ? 1 : 0) | (p->ml_vec32_active() ? 2 : 0) | (p->coarse32_active() ? 4 : 0);
  return DPGO_OK;
}

int dpgo_problem_multilevel_info(dpgo_problem_t p, int* nlevels, int* sizes, int* ks, int* nnzb) {
  if (!p) return fail(DPGO_ERR_INVALID, "null handle");
  if (!p->ml_symbolic) return fail(DPGO_ERR_STATE, "multilevel hierarchy not set up");
  const int cap = nlevels ? *nlevels : 0;
  for (int l = 0; l < (int)p->ml.size() && l < cap; ++l) {
    if (sizes) sizes[l] = p->ml[l].n;
    if (ks) ks[l] = p->ml[l].graph ? -p->ml[l].k : p->ml[l].k;  // negative: graph aggregates of at most that many poses
    // (graph aggregates whose fragments were merged: the LAST level's entry, otherwise 0, carries -merge bound)
    if (ks && l > 0 && l + 1 == (int)p->ml.size() && p->ml[0].graph && p->ml[0].merge_cap) ks[l] = -p->ml[0].merge_cap;
    if (nnzb) nnzb[l] = (l == 0) ? p->Q.nnzb : p->ml[l].A.nnzb;
  }
  if (nlevels) *nlevels = (int)p->ml.size();
  return DPGO_OK;
}


int dpgo_problem_multilevel_get(dpgo_problem_t p, int level, int what, void* out_host) {
  CHK(check_ready(p));
  if (!p->ml_ready) return fail(DPGO_ERR_STATE, "multilevel hierarchy not built");
  if (!out_host || level < 0 || level >= (int)p->ml.size()) return fail(DPGO_ERR_INVALID, "bad level / null pointer");
  auto& L = p->ml[level];
  const int bb = p->b * p->b;
  const void* src = nullptr;
  size_t bytes = 0;
  switch (what) {
    case DPGO_ML_P_BLOCKS:
      src = L.Pb, bytes = sizeof(double) * (size_t)L.n * bb;
      break;
    case DPGO_ML_A_ROWPTR:
      src = L.A.rowptr, bytes = sizeof(int32_t) * ((size_t)L.n + 1);
      break;
    case DPGO_ML_A_COLIDX:
      src = L.A.colidx, bytes = sizeof(int32_t) * (size_t)L.A.nnzb;
      break;
    case DPGO_ML_A_VALUES:
      src = L.A.vals, bytes = sizeof(double) * (size_t)L.A.nnzb * bb;
      break;
    case DPGO_ML_AGG_LABELS:
      src = L.graph ? L.lab : nullptr, bytes = sizeof(int32_t) * (size_t)L.n;
      break;
    case DPGO_ML_AP_NNZB: {
      if (!L.AP.vals) return fail(DPGO_ERR_INVALID, "this level does not hold that item");
      *static_cast<int32_t*>(out_host) = L.AP.nnzb;
      return DPGO_OK;
    }
    case DPGO_ML_RESTRICT_PARTIALS: {
      if (!L.graph) return fail(DPGO_ERR_INVALID, "this level does not hold that item");
      *static_cast<int32_t*>(out_host) = L.nseg;
      return DPGO_OK;
    }
    case DPGO_ML_DENSE_INVERSE: {
      if (level + 1 != (int)p->ml.size()) return fail(DPGO_ERR_INVALID, "the dense inverse belongs to the last level");
      const int N = L.n * p->b;  // the N x N corner of the padded lda x lda array
      HIPC(hipMemcpy2DAsync(out_host, sizeof(double) * N, p->dense.inv, sizeof(double) * p->dense.lda, sizeof(double) * N, N,
                            hipMemcpyDeviceToHost, p->stream));
      HIPC(hipStreamSynchronize(p->stream));
      return DPGO_OK;
    }
    default:
      return fail(DPGO_ERR_INVALID, "unknown item");
  }
  if (!src) return fail(DPGO_ERR_INVALID, "this level does not hold that item");
  HIPC(hipMemcpyAsync(out_host, src, bytes, hipMemcpyDeviceToHost, p->stream));
  HIPC(hipStreamSynchronize(p->stream));
  return DPGO_OK;
}


int dpgo_dense_spd_inverse(int N, const double* A_host, double* Ainv_host, int device, int use_mfma) {
  if (N <= 0 || N > 16384 || !A_host || !Ainv_host) return fail(DPGO_ERR_INVALID, "bad arguments");
  int cnt = 0;
  CHK(dpgo_device_count(&cnt));
  if (cnt <= 0) return fail(DPGO_ERR_HIP, "no HIP device (this library has no CPU fallback)");
  if (device < 0 || device >= cnt) return fail(DPGO_ERR_INVALID, "device index out of range");
  HIPC(hipSetDevice(device));
  const int lda = ((N + kNB - 1) / kNB) * kNB;
  DevBuf<double> M, W, Rx;
  CHK(M.alloc((size_t)lda * lda));
  CHK(W.alloc((size_t)lda * kNB));
  CHK(Rx.alloc((size_t)lda * kNB));
  HIPC(hipMemset(M, 0, sizeof(double) * (size_t)lda * lda));
  HIPC(hipMemcpy2D(M, sizeof(double) * lda, A_host, sizeof(double) * N, sizeof(double) * N, N, hipMemcpyHostToDevice));
  launch(k_dense_pad_identity, 1, 0, nullptr, M, lda, N);
  CHK(dense_spd_inverse(nullptr, M, lda, W, Rx, use_mfma != 0));
  HIPC(hipMemcpy2D(Ainv_host, sizeof(double) * N, M, sizeof(double) * lda, sizeof(double) * N, N, hipMemcpyDeviceToHost));
  return DPGO_OK;
}
#ifdef DPGO_TIMELINE
int dpgo_debug_timeline_cycle(long long* out /* [2][3][64]: restriction, post-smoothing */) {
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tl_restrict), sizeof(long long) * 3 * 64));
  HIPC(hipMemcpyFromSymbol(out + 3 * 64, HIP_SYMBOL(g_tl_post), sizeof(long long) * 3 * 64));
  return DPGO_OK;
}
#endif

}  // extern "C"
