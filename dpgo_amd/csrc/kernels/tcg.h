// kernels/tcg.h -- the two kernels of the tCG loop (fused Hessian step and residual / iterate update): shared scalar prologues,
// the generic-layout kernels (odd tile size) and the span kernels (even tile size: every 3-D case).
// What the kernels share exists once, as force-inlined helpers (each kernel keeps its own load placement):
//   entry         tcg_idle, tcg_publish                          early-exit test; thread 0 of workgroup 0 stores the state and publishes
//   tile          TileGeo, tile_geo                              p0 / valid / i / okp / ok of a wave's share of a pose tile (span layout)
//   Hessian step  tcg_ring_slots, hess_stage, hess_project,      DEF ring slots; X, z to LDS; S-correction (s_correct_col, common.h: shared
//                 hess_direction_update                          with k_hess) + projection; delta / H delta update and <delta, H delta>
//   update        tcg_step_span, tcg_step_col                    eta += c delta (unless DEF), r += c H delta, for c = alpha and c = tau
//                 (the z tail is span_from_lds, common.h: fp64 or fp32 destination)
// Part of kernels.h (included inside namespace dpgo, in this order: common.h, problem.h, tcg.h, persist.h, multilevel.h, dense.h, manifold.h, rtr.h, agent.h, init.h).
#pragma once

// ================================================================ K7b + K1/K3/K2 fused: one tCG step
// One launch per tCG iteration:
//  (i)   prologue = the scalar half of the direction update (ROPTLIB tCG_TR): convergence test
//        |r| <= |r0| min(|r0|^theta, kappa), beta = z_r'/z_r, e_Pd / d_Pd recurrences, from the
//        <r,r>, <z,r> partials of k_tcg_update (first = 1: norm_r0, z_r, d_Pd initialisation);
//  (ii)  Hz = proj_X( z Q - z_rot S ): the block-SpMM gathers the preconditioned residual z;
//  (iii) row-local, in place:  delta <- beta*delta - z,   H delta <- beta*(H delta) - Hz
//        (H is linear on the tangent space, so this equals H applied to the new delta; it lets the
//        direction update ride in the SpMM epilogue instead of costing a second gather or a separate
//        kernel: 3 -> 2 launches per tCG iteration), and the <delta, H delta> partial.
// The oracle has the same option (hess_recurrence) for trajectory-level parity tests.
// ---------------------------------------------------------------- tCG scalar prologues (shared)
// Direction-update scalars (ROPTLIB tCG_TR): returns false when this launch has nothing left to do.
__device__ __forceinline__ bool tcg_hess_prologue(DevState& st, const double* __restrict__ pin, int nb_in, int first,
                                                  double* red, double& beta, const PartialRaw<2>* early = nullptr) {
  double pr[2];
  if (early)
    partials_finish<2>(*early, pr, red);
  else
    load_partials<2>(pin, nb_in, pr, red);
  const double r_r = pr[0], z_r_new = pr[1];
  beta = 0.0;
  if (first) {
    st.norm_r0 = sqrt(r_r);
    st.z_r = z_r_new;
    st.d_Pd = z_r_new;
    st.e_Pd = 0.0;
    if (st.max_inner <= 0) {
      st.tcg_done = 1;
      return false;
    }
    return true;
  }
  const double norm_r = sqrt(r_r);
  const double pw = (st.theta == 1.0) ? st.norm_r0 : pow(st.norm_r0, st.theta);  // theta = 1 (reference default)
  if (st.tcg_j >= st.min_inner && norm_r <= st.norm_r0 * (pw < st.kappa ? pw : st.kappa)) {
    st.tcg_status = (st.kappa < pw) ? TCG_LCON : TCG_SCON;
    st.tcg_done = 1;
    return false;
  }
  beta = z_r_new / st.z_r;
  st.e_Pd = beta * (st.e_Pd + st.alpha * st.d_Pd);
  st.d_Pd = z_r_new + beta * beta * st.d_Pd;
  st.z_r = z_r_new;
  st.tcg_j += 1;
  if (st.tcg_j >= st.max_inner) {
    st.tcg_done = 1;
    st.tcg_status = TCG_MAXITER;
    return false;
  }
  return true;
}

// Step-length scalars: mode 0 = normal step, 1 = boundary step (eta += tau*delta, stop), 2 = initialisation.
__device__ __forceinline__ int tcg_update_prologue(DevState& st, const double* __restrict__ pin, int nb_in, int first,
                                                   double* red, double& alpha, double& tau,
                                                   const PartialRaw<1>* early = nullptr) {
  alpha = 0.0;
  tau = 0.0;
  if (first) {
    st.tcg_done = 0;
    st.tcg_j = 0;
    st.tcg_status = TCG_MAXITER;
    st.e_Pe = 0.0;
    st.e_Pd = 0.0;
    return 2;
  }
  double dh[1];
  if (early)
    partials_finish<1>(*early, dh, red);
  else
    load_partials<1>(pin, nb_in, dh, red);
  const double d_Hd = dh[0];
  alpha = st.z_r / d_Hd;
  const double e_Pe_new = st.e_Pe + 2.0 * alpha * st.e_Pd + alpha * alpha * st.d_Pd;
  st.n_hess += 1;
  st.alpha = alpha;
  const double D2 = st.Delta * st.Delta;
  if (d_Hd <= 0.0 || e_Pe_new >= D2) {
    tau = (-st.e_Pd + sqrt(st.e_Pd * st.e_Pd + st.d_Pd * (D2 - st.e_Pe))) / st.d_Pd;
    st.tcg_status = (d_Hd < 0.0) ? TCG_NEGCURV : TCG_EXCREGION;
    st.tcg_done = 1;
    return 1;
  }
  st.e_Pe = e_Pe_new;
  return 0;
}

// ---------------------------------------------------------------- kept directions (DEF = 1)
// Nothing inside a tCG run reads the iterate eta: the trust-region norms come from the scalar recurrences above and the rho
// test reads eta once, in k_retract.  A solve whose direction ring fits (host: tcg_dirs_ensure) therefore keeps the
// directions instead of summing them every iteration:
//  * the Hessian-step kernels read delta_{k-1} from slot k-1 of the ring and write delta_k to slot k (`delta` is the ring,
//    a slot is n * T doubles), k = the iteration index the prologue has just computed (0 with `first`, else st.tcg_j): the
//    same bytes as the in-place update, and a launch that exits early touches nothing.  k < max_inner <= slots of the ring;
//  * the update kernels load neither delta nor eta and store no eta; the thread that stores the state record also stores
//    this iteration's step length (alpha, or tau on the boundary step) and the number of steps so far into `coef`:
//    coef[0] = count (0 from the initialisation), coef[1 + j] = step length of iteration j;
//  * k_retract folds eta = fma(c_{K-1}, delta_{K-1}, ... fma(c_0, delta_0, +0)) while it loads its tile: the same fused
//    multiply-adds in the same order on the same operands as the running sum, so every bit of eta is the same.
template <int DEF>
__device__ __forceinline__ void tcg_store_coef(double* __restrict__ coef, const DevState& st, int mode, double alpha, double tau) {
  if constexpr (DEF) {
    if (mode == 2) {
      coef[0] = 0.0;
    } else {
      coef[1 + st.tcg_j] = (mode == 1) ? tau : alpha;
      coef[0] = (double)(st.tcg_j + 1);
    }
  }
}
// The ring slots a Hessian step reads and writes, from the iteration index the prologue has just computed: slot k of the
// ring receives delta_k, slot k - 1 holds delta_{k-1} (a slot is n * T doubles).  DEF = 0: both are `delta`, updated in place.
template <int DEF, int T>
__device__ __forceinline__ void tcg_ring_slots(double* delta, int first, int tcg_j, int n, const double*& din, double*& dout) {
  dout = delta;
  if constexpr (DEF) dout = delta + (size_t)(first ? 0 : tcg_j) * ((size_t)n * T);
  din = (DEF && !first) ? dout - (size_t)n * T : dout;
}

// ---------------------------------------------------------------- entry: early exit, state record and progress word
// A launch has nothing to do once the outer iteration has stopped or the tCG run is over (`done_counts` = false: the update
// kernel's initialisation launch, first = 1, starts a run whatever the record says about the last one).
__device__ __forceinline__ bool tcg_idle(const DevState& st, bool done_counts = true) {
  return st.rtr_stop || (done_counts && st.tcg_done);
}
// One thread of the launch stores the state record and publishes the progress word; `between` runs between the two (the
// update kernels store the step length there, tcg_store_coef).
struct TcgNothing {
  __device__ __forceinline__ void operator()() const {}
};
template <class F = TcgNothing>
__device__ __forceinline__ void tcg_publish(DevState* sout, const DevState& st, unsigned long long* hflag, unsigned gen,
                                            F between = F()) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    store_state(sout, st);
    between();
    publish_progress(hflag, gen, st);
  }
}

// ---------------------------------------------------------------- span layout: a wave's share of a pose tile
// p0 = its first pose, valid = entries of its span that exist (ragged last tile), i = this lane's pose, okp = the pose exists,
// ok = ... and this lane group is the one that owns it (SPLIT > 1: group 0).
struct TileGeo {
  int p0, valid, i;
  bool okp, ok;
};
template <class GEO>
__device__ __forceinline__ TileGeo tile_geo(int tile, int n, const LaneId& L) {
  TileGeo t;
  t.p0 = tile * GEO::P + L.wave * GEO::G;
  const int npose = (n - t.p0) < GEO::G ? (n - t.p0) : GEO::G;
  t.valid = npose > 0 ? npose * GEO::T : 0;
  t.i = t.p0 + L.g;
  t.okp = (L.g < GEO::G) && (t.i < n);
  t.ok = t.okp && (L.s == 0);
  return t;
}

// ---------------------------------------------------------------- Hessian-step tile phases (span and symmetric kernels)
// Own-tile X and z pieces to the wave's LDS tiles.
template <int NIT>
__device__ __forceinline__ void hess_stage(double* ys, double* vs, const dbl2 (&xv)[NIT], const dbl2 (&zv)[NIT], int valid,
                                           int lane) {
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int pc = lane + 64 * it;
    if (2 * pc < valid) {
      reinterpret_cast<dbl2*>(ys)[pc] = xv[it];
      reinterpret_cast<dbl2*>(vs)[pc] = zv[it];
    }
  }
}
// h = column c of z Q (the gather's result) -> os = proj_X(h - z_rot S); hs is the tile in between.  Runs between two
// wave_sync() of the caller (vs staged before it, os read after it).
template <int D, int R>
__device__ __forceinline__ void hess_project(const double* ys, const double* vs, double* hs, double* os,
                                             const double (&srow)[D], const LaneId& L, bool ok, double (&h)[R]) {
  constexpr int T = Geo<D, R>::T;
  if (ok) {
    if (L.c < D) s_correct_col<D, R>(vs + L.g * T, srow, h);
    store_col<R>(hs + L.g * T + L.c * R, h);
  }
  wave_sync();
  if (ok) {
    double hz[R], sdummy[D];
    proj_col<D, R>(ys + L.g * T, hs + L.g * T, L.c, h, hz, sdummy);
    store_col<R>(os + L.g * T + L.c * R, hz);
  }
}
// z of piece `it`: from the registers that staged it (k_tcg_hess_span) or re-read from its LDS tile (k_tcg_hess_sym).
template <int NIT>
__device__ __forceinline__ dbl2 hess_z_piece(const dbl2 (&zv)[NIT], int it, int) { return zv[it]; }
__device__ __forceinline__ dbl2 hess_z_piece(const double* vs, int, int pc) { return reinterpret_cast<const dbl2*>(vs)[pc]; }
// Row-local direction update in span layout: delta <- beta delta - z, H delta <- beta H delta - Hz (Hz from os), stored to
// dtile / htile (the wave's spans of the output slot and of H delta), and the <delta, H delta> partial.
template <int NTS, int NIT, class Z>
__device__ __forceinline__ void hess_direction_update(double* dtile, double* htile, const double* os, const Z& z,
                                                      const dbl2 (&dv)[NIT], const dbl2 (&hv)[NIT], double beta, int first,
                                                      int valid, int lane, double& part) {
  dbl2* d2 = reinterpret_cast<dbl2*>(dtile);
  dbl2* h2 = reinterpret_cast<dbl2*>(htile);
#pragma unroll
  for (int it = 0; it < NIT; ++it) {
    const int pc = lane + 64 * it;
    if (2 * pc < valid) {
      const dbl2 hzv = reinterpret_cast<const dbl2*>(os)[pc];
      const dbl2 zl = hess_z_piece(z, it, pc);
      dbl2 dn, hn;
      if (first) {
        dn.x = -zl.x;
        dn.y = -zl.y;
        hn.x = -hzv.x;
        hn.y = -hzv.y;
      } else {
        dn.x = fma(beta, dv[it].x, -zl.x);
        dn.y = fma(beta, dv[it].y, -zl.y);
        hn.x = fma(beta, hv[it].x, -hzv.x);
        hn.y = fma(beta, hv[it].y, -hzv.y);
      }
      st_stream<NTS>(d2 + pc, dn);
      st_stream<NTS>(h2 + pc, hn);
      part = fma(dn.x, hn.x, part);
      part = fma(dn.y, hn.y, part);
    }
  }
}

// ---------------------------------------------------------------- update-kernel recurrences
// eta += c delta (not with DEF: the directions are kept and eta is formed once, in k_retract) and r += c H delta, for the
// regular step (c = alpha) and the boundary step (c = tau).  Span layout: one piece, eta stored, r left to the caller.
template <int DEF>
__device__ __forceinline__ void tcg_step_span(double c, const dbl2& ev, const dbl2& dv, const dbl2& hv, dbl2* eta_pc, dbl2& rr) {
  if constexpr (!DEF) {
    dbl2 e = ev;
    e.x = fma(c, dv.x, e.x);
    e.y = fma(c, dv.y, e.y);
    *eta_pc = e;
  }
  rr.x = fma(c, hv.x, rr.x);
  rr.y = fma(c, hv.y, rr.y);
}
// Column layout: loads included (eta, delta, H delta, r at this lane's column), eta stored, r left to the caller.
template <int R, int DEF>
__device__ __forceinline__ void tcg_step_col(double c, double* eta_c, const double* delta_c, const double* Hd_c,
                                             const double* r_c, double (&rr)[R]) {
  double hd[R];
  if constexpr (!DEF) {
    double e[R], dl[R];
    load_col<R>(eta_c, e);
    load_col<R>(delta_c, dl);
#pragma unroll
    for (int a = 0; a < R; ++a) e[a] = fma(c, dl[a], e[a]);
    store_col<R>(eta_c, e);
  }
  load_col<R>(Hd_c, hd);
  load_col<R>(r_c, rr);
#pragma unroll
  for (int a = 0; a < R; ++a) rr[a] = fma(c, hd[a], rr[a]);
}

template <int D, int R, int SPLIT, int DEF = 0>
__global__ __launch_bounds__(kBlock, DPGO_LB_HESS) void k_tcg_hess(BsrDev Q, const double* __restrict__ X,
                                                     const double* __restrict__ S, const double* __restrict__ z,
                                                     double* __restrict__ delta, double* __restrict__ Hd,
                                                     const double* __restrict__ pin, int nb_in,
                                                     double* __restrict__ pout, const DevState* __restrict__ sin,
                                                     DevState* __restrict__ sout, int first, int n,
                                                     unsigned long long* hflag, unsigned gen) {
  // generic layout (odd tile size: the 2-D cases with odd r); even tile sizes run k_tcg_hess_span
  using GEO = Geo<D, R, SPLIT>;
  __shared__ __attribute__((aligned(16))) double sm[kWaves][3][GEO::G][GEO::T];
  __shared__ double red[kWaves * kNP];
  DevState st;
  load_state(st, sin);
  gen = state_gen(st, gen);
  if (tcg_idle(st)) {
    tcg_publish(sout, st, hflag, gen);
    return;
  }
  double beta;
  const bool go = tcg_hess_prologue(st, pin, nb_in, first, red, beta);
  tcg_publish(sout, st, hflag, gen);
  if (!go) return;
  const double* din;
  double* dout;
  tcg_ring_slots<DEF, GEO::T>(delta, first, st.tcg_j, n, din, dout);

  const LaneId L = lane_id<D, SPLIT>();
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  double part[1] = {0.0};
  const TileIter ti_ = tile_iter(ntiles);
  for (int tile = ti_.first; tile < ti_.last; tile += ti_.step) {
    const int i = tile * GEO::P + L.wave * GEO::G + L.g;
    const bool okp = (L.g < GEO::G) && (i < n);
    const bool ok = okp && (L.s == 0);
    double h[R], zc[R], x[R];
    const size_t off = (size_t)i * GEO::T + L.c * R;
    double* ys = ok ? &sm[L.wave][0][L.g][0] : nullptr;
    double* vs = ok ? &sm[L.wave][1][L.g][0] : nullptr;
    double* hs = ok ? &sm[L.wave][2][L.g][0] : nullptr;
    // issue the epilogue's loads first: they overlap the gather's index -> tile latency chain
    double srow[D], dl[R], hd[R];
    if (ok) {
      load_col<R>(X + off, x);
      load_col<R>(z + off, zc);
      if (L.c < D) {
#pragma unroll
        for (int a = 0; a < D; ++a) srow[a] = S[(size_t)i * D * D + L.c * D + a];
      }
      if (!first) {
        load_col<R>(din + off, dl);
        load_col<R>(Hd + off, hd);
      }
    }
    spmm_col<D, R, SPLIT>(Q.rowptr, Q.colidx, Q.vals, z, i, L.s, L.c, okp, h);
    if (ok) {
      store_col<R>(ys + L.c * R, x);
      store_col<R>(vs + L.c * R, zc);
    }
    wave_sync();
    if (ok) {
      if (L.c < D) s_correct_col<D, R>(vs, srow, h);
      store_col<R>(hs + L.c * R, h);
    }
    wave_sync();
    if (ok) {
      double hz[R], s[D];
      proj_col<D, R>(ys, hs, L.c, h, hz, s);
      if (first) {
#pragma unroll
        for (int a = 0; a < R; ++a) {
          dl[a] = -zc[a];
          hd[a] = -hz[a];
        }
      } else {
#pragma unroll
        for (int a = 0; a < R; ++a) {
          dl[a] = fma(beta, dl[a], -zc[a]);
          hd[a] = fma(beta, hd[a], -hz[a]);
        }
      }
#pragma unroll
      for (int a = 0; a < R; ++a) part[0] = fma(dl[a], hd[a], part[0]);
      store_col<R>(dout + off, dl);
      store_col<R>(Hd + off, hd);
    }
    wave_sync();
  }
  store_partials<1>(part, pout, red);
}

// ================================================================ span kernels (pose tile size even: all 3-D cases)
// Same arithmetic as k_tcg_hess / k_tcg_update; the differences are purely about memory:
//  * own-tile vectors move as lane-linear 16-byte pieces (Span<>), element-wise recurrences run in span layout;
//  * the FIRST tile's global loads (row pointer, column indices, vector pieces) are issued before the scalar
//    prologue (state record + partial-sum reduction), so the two dependent-latency chains overlap -- this is
//    what matters for small blocks (multi-GPU strong scaling), where a kernel is a chain of ~15 memory latencies.
template <int D, int R, int SPLIT, int NTS = 0, int DEF = 0>
__global__ __launch_bounds__(kBlock) void k_tcg_hess_span(BsrDev Q, const double* __restrict__ X,
                                                          const double* __restrict__ S, const double* __restrict__ z,
                                                          double* __restrict__ delta, double* __restrict__ Hd,
                                                          const double* __restrict__ pin, int nb_in,
                                                          double* __restrict__ pout, const DevState* __restrict__ sin,
                                                          DevState* __restrict__ sout, int first, int n,
                                                          unsigned long long* hflag, unsigned gen) {
  using GEO = Geo<D, R, SPLIT>;
  using SPN = Span<D, R, SPLIT>;
  __shared__ __attribute__((aligned(16))) double sm[kWaves][4][GEO::G][GEO::T];
  __shared__ double red[kWaves * kNP];
  const LaneId L = lane_id<D, SPLIT>();
  const int lane = threadIdx.x & 63;
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  const TileIter ti_ = tile_iter(ntiles);
  double* ys = &sm[L.wave][0][0][0];
  double* vs = &sm[L.wave][1][0][0];
  double* hs = &sm[L.wave][2][0][0];
  double* os = &sm[L.wave][3][0][0];

  // ---- per-tile prefetch state
  RowIdx ri;
  dbl2 xv[SPN::NIT], zv[SPN::NIT], dv[SPN::NIT], hv[SPN::NIT];
  double srow[D];
  TileGeo tg{};
  // (DEF: the ring slots this launch reads and writes follow from the prologue: the first tile's piece of delta_{k-1} is
  // requested behind it -- an early-exit launch must not touch the ring, its tcg_j may equal the number of slots)
  const double* din = DEF ? nullptr : delta;
  double* dout = delta;
  auto prefetch = [&](int tile) {
    tg = tile_geo<GEO>(tile, n, L);
    ri = row_idx_load<D, SPLIT>(Q.rowptr, Q.colidx, tg.i, L.s, L.c, tg.okp);
    const size_t base = (size_t)tg.p0 * GEO::T;
    const dbl2* X2 = reinterpret_cast<const dbl2*>(X + base);
    const dbl2* z2 = reinterpret_cast<const dbl2*>(z + base);
    const dbl2* h2 = reinterpret_cast<const dbl2*>(Hd + base);
#pragma unroll
    for (int it = 0; it < SPN::NIT; ++it) {
      const int pc = lane + 64 * it;
      if (2 * pc < tg.valid) {
        xv[it] = ld_stream<NTS>(X2 + pc);
        zv[it] = z2[pc];
        if (!first) {
          if (!DEF || din) dv[it] = ld_stream<NTS>(reinterpret_cast<const dbl2*>(din + base) + pc);
          hv[it] = ld_stream<NTS>(h2 + pc);
        }
      }
    }
    if (tg.ok && L.c < D) {
#pragma unroll
      for (int a = 0; a < D; ++a) srow[a] = ld_stream<NTS>(S + (size_t)tg.i * D * D + L.c * D + a);
    }
  };
  // ---- everything the prologue needs is requested before the first wait: state record (scalar loads), the
  // previous kernel's partial sums (small blocks only: the registers would cost the big-block kernel an
  // occupancy step), then the first tile.  A small-block launch is a chain of dependent memory round trips
  // (rocprof: 9.4 us for 2500 poses); this takes two of them off the chain.
  DPGO_TL_DECL;
  DPGO_STAMP(0, 0);
  DevState st;
  load_state(st, sin);
  gen = state_gen(st, gen);
  [[maybe_unused]] PartialRaw<2> praw;
  if constexpr (SPLIT > 1) partials_issue<2>(pin, nb_in, praw);
  int tile = ti_.first;
  bool have = tile < ti_.last;
  if (have) prefetch(tile);

  DPGO_STAMP(0, 1);
  // ---- scalar prologue
  if (tcg_idle(st)) {
    tcg_publish(sout, st, hflag, gen);
    return;
  }
  double beta;
  const bool go = tcg_hess_prologue(st, pin, nb_in, first, red, beta, (SPLIT > 1) ? &praw : nullptr);
  tcg_publish(sout, st, hflag, gen);
  if (!go) return;
  DPGO_STAMP(0, 2);
  tcg_ring_slots<DEF, GEO::T>(delta, first, st.tcg_j, n, din, dout);
  if constexpr (DEF) {
    if (!first && have) {
      const dbl2* d2 = reinterpret_cast<const dbl2*>(din + (size_t)tg.p0 * GEO::T);
#pragma unroll
      for (int it = 0; it < SPN::NIT; ++it) {
        const int pc = lane + 64 * it;
        if (2 * pc < tg.valid) dv[it] = ld_stream<NTS>(d2 + pc);
      }
    }
  }

  double part[1] = {0.0};
  while (have) {
    hess_stage(ys, vs, xv, zv, tg.valid, lane);
    DPGO_STAMP(0, 3);
    double h[R];
    spmm_col_pre<D, R, SPLIT>(ri, Q.colidx, Q.vals, z, L.s, L.c, h);
    wave_sync();
    DPGO_STAMP(0, 4);
    hess_project<D, R>(ys, vs, hs, os, srow, L, tg.ok, h);
    wave_sync();
    hess_direction_update<NTS>(dout + (size_t)tg.p0 * GEO::T, Hd + (size_t)tg.p0 * GEO::T, os, zv, dv, hv, beta, first,
                               tg.valid, lane, part[0]);
    wave_sync();
    DPGO_STAMP(0, 5);
    tile += ti_.step;
    have = tile < ti_.last;
    if (have) prefetch(tile);
  }
  store_partials<1>(part, pout, red);
  DPGO_STAMP(0, 6);
  DPGO_COMMIT(0);
}

// k_tcg_hess_span on the symmetric storage of Q (spmm_sym_pre, common.h): big blocks only (one pose per D+1 lanes).  The
// own-tile pieces of delta / H delta are requested after the gather instead of one tile ahead and z is re-read from LDS
// (registers).  The gather keeps the loads of DPGO_HESS_BATCH blocks in flight per wave, which costs the third wave per SIMD
// (217 VGPRs) and still wins: 2 waves x 4 blocks in flight against 3 x 1 (39.7 -> 37.3 us).  In-kernel timeline of a tile
// (tools/timeline_tiles.py, profiles/r05_v4_timeline_tiles.txt): ~8 us, of which the gather's two round trips 3 us and the
// epilogue behind it 4 us.  Tried on top and measured neutral, i.e. the launch is bound by what the memory system
// delivers to 512 resident workgroups, not by one wave's chain of round trips: delta / H delta requested in front of the
// gather (37.4..37.7 us), a three-stage pipeline over the tiles (row extents two tiles ahead, indices + own X, z, S one tile
// ahead: tile 7 us, launch 37.4..38.0 us), the previous kernel's partial sums requested in front of the first tile.
template <int D, int R, int NTS, int DEF = 0>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(DPGO_SYM_WAVES, DPGO_SYM_WAVES))) void k_tcg_hess_sym(BsrSymDev Q, const double* __restrict__ X,
                                                          const double* __restrict__ S, const double* __restrict__ z,
                                                          double* __restrict__ delta, double* __restrict__ Hd,
                                                          const double* __restrict__ pin, int nb_in,
                                                          double* __restrict__ pout, const DevState* __restrict__ sin,
                                                          DevState* __restrict__ sout, int first, int n,
                                                          unsigned long long* hflag, unsigned gen) {
  constexpr int SPLIT = 1;
  using GEO = Geo<D, R, SPLIT>;
  using SPN = Span<D, R, SPLIT>;
  __shared__ __attribute__((aligned(16))) double sm[kWaves][4][GEO::G][GEO::T];
  __shared__ double red[kWaves * kNP];
  const LaneId L = lane_id<D, SPLIT>();
  const int lane = threadIdx.x & 63;
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  const TileIter ti_ = tile_iter(ntiles);
  double* ys = &sm[L.wave][0][0][0];
  double* vs = &sm[L.wave][1][0][0];
  double* hs = &sm[L.wave][2][0][0];
  double* os = &sm[L.wave][3][0][0];

  // ---- per-tile prefetch state
  SymIdx si;
  dbl2 xv[SPN::NIT], zv[SPN::NIT];
  double srow[D];
  TileGeo tg{};
  auto prefetch = [&](int tk) {
    tg = tile_geo<GEO>(tile_of(Q, tk), n, L);  // (the walk over the tiles: BsrSymDevT::tord)
    si = sym_idx_load<D>(Q, tg.i, L.c, tg.okp);
    const size_t base = (size_t)tg.p0 * GEO::T;
    const dbl2* X2 = reinterpret_cast<const dbl2*>(X + base);
    const dbl2* z2 = reinterpret_cast<const dbl2*>(z + base);
#pragma unroll
    for (int it = 0; it < SPN::NIT; ++it) {
      const int pc = lane + 64 * it;
      if (2 * pc < tg.valid) {
        xv[it] = ld_stream<NTS>(X2 + pc);
        zv[it] = z2[pc];
      }
    }
    if (tg.ok && L.c < D) {
#pragma unroll
      for (int a = 0; a < D; ++a) srow[a] = ld_stream<NTS>(S + (size_t)tg.i * D * D + L.c * D + a);
    }
  };
  // ---- everything the prologue needs is requested before the first wait: state record (scalar loads), the
  // previous kernel's partial sums (small blocks only: the registers would cost the big-block kernel an
  // occupancy step), then the first tile.  A small-block launch is a chain of dependent memory round trips
  // (rocprof: 9.4 us for 2500 poses); this takes two of them off the chain.
  DPGO_TL_DECL;
  DPGO_TL_TILES_DECL;
  DPGO_STAMP(0, 0);
  DevState st;
  load_state(st, sin);
  gen = state_gen(st, gen);
  [[maybe_unused]] PartialRaw<2> praw;
  int tile = ti_.first;
  bool have = tile < ti_.last;
  if (have) prefetch(tile);

  DPGO_STAMP(0, 1);
  // ---- scalar prologue
  if (tcg_idle(st)) {
    tcg_publish(sout, st, hflag, gen);
    return;
  }
  double beta;
  const bool go = tcg_hess_prologue(st, pin, nb_in, first, red, beta, (SPLIT > 1) ? &praw : nullptr);
  tcg_publish(sout, st, hflag, gen);
  if (!go) return;
  const double* din;
  double* dout;
  tcg_ring_slots<DEF, GEO::T>(delta, first, st.tcg_j, n, din, dout);
  DPGO_STAMP(0, 2);
  DPGO_STAMP_ENTRY;
  DPGO_STAMP_AT(1);

  double part[1] = {0.0};
  while (have) {
    DPGO_STAMP_TILE(0);
    hess_stage(ys, vs, xv, zv, tg.valid, lane);
    DPGO_STAMP(0, 3);
    DPGO_STAMP_TILE(1);
    double h[R];
    spmm_sym_pre<D, R, DPGO_HESS_BATCH>(si, Q, z, L.c, h);
    DPGO_TL_USE(h[0]);
    DPGO_STAMP_TILE(2);
    // delta, H delta of the own tile: requested after the gather (its accumulators need the registers), consumed after
    // the projection
    dbl2 dv[SPN::NIT], hv[SPN::NIT];
    if (!first) {
      const size_t base = (size_t)tg.p0 * GEO::T;
      const dbl2* d2 = reinterpret_cast<const dbl2*>(din + base);
      const dbl2* h2 = reinterpret_cast<const dbl2*>(Hd + base);
#pragma unroll
      for (int it = 0; it < SPN::NIT; ++it) {
        const int pc = lane + 64 * it;
        if (2 * pc < tg.valid) {
          dv[it] = ld_stream<NTS>(d2 + pc);
          hv[it] = ld_stream<NTS>(h2 + pc);
        }
      }
    }
    wave_sync();
    DPGO_STAMP(0, 4);
    DPGO_STAMP_TILE(3);
    hess_project<D, R>(ys, vs, hs, os, srow, L, tg.ok, h);
    wave_sync();
    DPGO_STAMP_TILE(4);
    hess_direction_update<NTS>(dout + (size_t)tg.p0 * GEO::T, Hd + (size_t)tg.p0 * GEO::T, os, vs, dv, hv, beta, first,
                               tg.valid, lane, part[0]);
    wave_sync();
    DPGO_STAMP(0, 5);
    tile += ti_.step;
    have = tile < ti_.last;
    if (have) prefetch(tile);
    DPGO_STAMP_TILE(5);
    DPGO_TILE_NEXT;
  }
  store_partials<1>(part, pout, red);
  DPGO_STAMP(0, 6);
  DPGO_STAMP_AT(2);
  DPGO_COMMIT(0);
}

#ifndef DPGO_UPDATE_WAVES
#define DPGO_UPDATE_WAVES 0  // waves per SIMD k_tcg_update_span is compiled for (0: the compiler's choice -- 203 VGPRs = 2 waves)
#endif
// ML = 1: the launch is known to be in multilevel mode (ml_omega > 0: z receives the unprojected pre-smoothing step, the
// iterate is not read) -- the instance the 100k loop launches: without the iterate's pieces and the projection it fits
// DPGO_UPDATE_WAVES_ML waves per SIMD.  ML = 0: the mode is the runtime argument (block-Jacobi / no preconditioner / either).
#ifndef DPGO_UPDATE_WAVES_ML
#define DPGO_UPDATE_WAVES_ML 3
#endif
// DEF = 1 (kept directions, see above k_tcg_hess): delta and eta are not touched (null), the step length goes to `coef`.
// (3, 5): the multilevel instance drops from 147 to 119 VGPRs; it stays at DPGO_UPDATE_WAVES_ML waves -- a fourth workgroup
// per CU does not fit the LDS (4 x 41 088 bytes), and the grid, hence the order of the partial sums, is the reference's.
// PIPE = 1 (DPGO_UPDATE_PIPE, the default; 0 = the reference order, same bits): the next tile is requested while this one is
// still being finished, see request_next below.  It costs the registers of a second tile's geometry and block-Jacobi row
// and whatever the compiler then keeps live: (3, 5) DEF = 1 goes from 119 to 157 VGPRs, still three waves, no scratch.  The
// instances that do not hold their occupancy that way have no PIPE = 1 form (kUpdatePipe: the launch picks PIPE = 0):
//  * ML = 1, DEF = 0 at 20 and more doubles per pose, (3, 5) and (3, 6): four piece sets (eta, delta, H delta, r) in flight
//    need 168 VGPRs and 180 / 232 bytes of scratch per lane; up to 16 doubles per pose it fits (115-164 VGPRs);
//  * every ML = 0 instance: (3, 5) goes from 209 VGPRs to 256 + 20 AGPRs (2 -> 1 wave), (3, 3) DEF = 1 from 4 waves to 2.
template <int D, int R, int DEF>
constexpr int kUpdatePipe = (DEF || Geo<D, R>::T <= 16) ? 1 : 0;
template <int D, int R, int ML = 0, int DEF = 0, int PIPE = 0>
__global__ __launch_bounds__(kBlock)
    __attribute__((amdgpu_waves_per_eu(ML ? DPGO_UPDATE_WAVES_ML : (DPGO_UPDATE_WAVES ? DPGO_UPDATE_WAVES : 1),
                                       ML ? DPGO_UPDATE_WAVES_ML : (DPGO_UPDATE_WAVES ? DPGO_UPDATE_WAVES : 8))))
void k_tcg_update_span(const double* __restrict__ X, const double* __restrict__ g,
                                                            const double* __restrict__ dinv,
                                                            const double* __restrict__ delta,
                                                            const double* __restrict__ Hd, double* __restrict__ eta,
                                                            double* __restrict__ r, double* __restrict__ z,
                                                            const double* __restrict__ pin, int nb_in,
                                                            double* __restrict__ pout, const DevState* __restrict__ sin,
                                                            DevState* __restrict__ sout, int first, int n,
                                                            unsigned long long* hflag, unsigned gen,
                                                            double ml_omega, double* __restrict__ coef,
                                                            float* __restrict__ z32 = nullptr) {
  // ml_omega > 0 (fused multilevel preconditioner): z receives the pre-smoothing step w Dinv r, unprojected -- into z32
  // instead, rounded to fp32, when the cycle keeps its internal vectors in that storage (kernel-uniform)
  using GEO = Geo<D, R>;
  using SPN = Span<D, R, 1>;
  __shared__ __attribute__((aligned(16))) double sm[kWaves][4][GEO::G][GEO::T];
  __shared__ double red[kWaves * kNP];
  const LaneId L = lane_id<D>();
  const int lane = threadIdx.x & 63;
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  const TileIter ti_ = tile_iter(ntiles);
  double* ys = &sm[L.wave][0][0][0];
  double* rs = &sm[L.wave][1][0][0];
  double* zs = &sm[L.wave][2][0][0];
  double* os = &sm[L.wave][3][0][0];

  const bool ml_mode = ML ? true : (ml_omega > 0.0);  // (ML: compile-time)
  dbl2 xv[SPN::NIT], ev[SPN::NIT], dv[SPN::NIT], hv[SPN::NIT], rv[SPN::NIT];
  double drow[GEO::B];
  TileGeo tg{};  // (one lane group per pose: okp is the whole test)
  // (PIPE: the geometry and the block-Jacobi row of the tile in flight, beside the ones of the tile being finished)
  [[maybe_unused]] double drow_n[GEO::B];
  [[maybe_unused]] TileGeo tg_n{};
  auto request = [&](int tile, TileGeo& t, double (&drow_)[GEO::B]) {
    t = tile_geo<GEO>(tile, n, L);
    const size_t base = (size_t)t.p0 * GEO::T;
    const dbl2* X2 = reinterpret_cast<const dbl2*>(X + base);
    const dbl2* g2 = reinterpret_cast<const dbl2*>(g + base);
    [[maybe_unused]] const dbl2* e2 = reinterpret_cast<const dbl2*>(eta + base);
    [[maybe_unused]] const dbl2* d2 = reinterpret_cast<const dbl2*>(delta + base);
    const dbl2* h2 = reinterpret_cast<const dbl2*>(Hd + base);
    const dbl2* r2 = reinterpret_cast<const dbl2*>(r + base);
#pragma unroll
    for (int it = 0; it < SPN::NIT; ++it) {
      const int pc = lane + 64 * it;
      if (2 * pc < t.valid) {
        // (the iterate is only needed by the tangent projection of the block-Jacobi / unpreconditioned z; the multilevel
        // pre-smoothing step x1 = w Dinv r is not projected: 16 MB less per launch at 100k poses)
        if (!ml_mode) xv[it] = X2[pc];
        if (first) {
          rv[it] = g2[pc];
        } else {
          if constexpr (!DEF) {
            ev[it] = e2[pc];
            dv[it] = d2[pc];
          }
          hv[it] = h2[pc];
          rv[it] = r2[pc];
        }
      }
    }
    if (t.okp && dinv) {
#pragma unroll
      for (int k = 0; k < GEO::B; ++k) drow_[k] = dinv[(size_t)t.i * GEO::BB + L.c * GEO::B + k];
    }
  };
  auto prefetch = [&](int tile) { request(tile, tg, drow); };
  // PIPE = 1: the next tile is requested as soon as the piece registers of this one are consumed -- behind the first
  // per-piece loop, which is the last reader of xv / ev / dv / hv / rv -- so its round trip runs under the block-Jacobi
  // step, the LDS passes and the stores of z instead of starting behind them.  The pieces it loads are other addresses
  // than the ones just stored; the arithmetic, its order and every store are those of PIPE = 0 (DPGO_UPDATE_PIPE=0).
  auto request_next = [&](int& tile, bool& have) {
    if constexpr (PIPE) {
      tile += ti_.step;
      have = tile < ti_.last;
      if (have) request(tile, tg_n, drow_n);
    }
  };
  DPGO_TL_DECL;
  DPGO_STAMP(1, 0);
  // state record and partial sums are requested before the first tile (see k_tcg_hess_span)
  DevState st;
  load_state(st, sin);
  gen = state_gen(st, gen);
  PartialRaw<1> praw;
  partials_issue<1>(pin, nb_in, praw);
  int tile = ti_.first;
  bool have = tile < ti_.last;
  if (have) prefetch(tile);

  if (tcg_idle(st, !first)) {
    tcg_publish(sout, st, hflag, gen);
    return;
  }
  double alpha, tau;
  const int mode = tcg_update_prologue(st, pin, nb_in, first, red, alpha, tau, &praw);
  tcg_publish(sout, st, hflag, gen, [&] { tcg_store_coef<DEF>(coef, st, mode, alpha, tau); });

  DPGO_STAMP(1, 2);
  double part[2] = {0.0, 0.0};
  while (have) {
    const size_t base = (size_t)tg.p0 * GEO::T;
    [[maybe_unused]] dbl2* eta2 = reinterpret_cast<dbl2*>(eta + base);
    if (mode == 1) {  // workgroup-uniform: eta += tau * delta, then tCG stops
      // (r += tau * H delta with it: r = g + H eta holds at every exit of tCG, which is what the rho test reads, k_retract)
      dbl2* r2 = reinterpret_cast<dbl2*>(r + base);
#pragma unroll
      for (int it = 0; it < SPN::NIT; ++it) {
        const int pc = lane + 64 * it;
        if (2 * pc < tg.valid) {
          dbl2 rr = rv[it];
          tcg_step_span<DEF>(tau, ev[it], dv[it], hv[it], eta2 + pc, rr);
          r2[pc] = rr;
        }
      }
      request_next(tile, have);
    } else {
      dbl2* r2 = reinterpret_cast<dbl2*>(r + base);
#pragma unroll
      for (int it = 0; it < SPN::NIT; ++it) {
        const int pc = lane + 64 * it;
        if (2 * pc < tg.valid) {
          if (!ml_mode) reinterpret_cast<dbl2*>(ys)[pc] = xv[it];
          dbl2 rr = rv[it];
          if (mode == 2) {
            if constexpr (!DEF) {
              dbl2 zero;
              zero.x = 0.0;
              zero.y = 0.0;
              eta2[pc] = zero;
            }
          } else {
            tcg_step_span<DEF>(alpha, ev[it], dv[it], hv[it], eta2 + pc, rr);
          }
          r2[pc] = rr;
          reinterpret_cast<dbl2*>(rs)[pc] = rr;
          part[0] = fma(rr.x, rr.x, part[0]);
          part[0] = fma(rr.y, rr.y, part[0]);
        }
      }
      request_next(tile, have);
      wave_sync();
      double zz[R];
      if (tg.okp) {
        const double* rt = rs + L.g * GEO::T;
        if (dinv) {
          jacobi_col<D, R>(rt, drow, zz);
        } else {
#pragma unroll
          for (int a = 0; a < R; ++a) zz[a] = rt[L.c * R + a];
        }
        store_col<R>(zs + L.g * GEO::T + L.c * R, zz);
      }
      wave_sync();
      if (tg.okp) {
        double out[R], sdummy[D];
        if (ml_mode) {
#pragma unroll
          for (int a = 0; a < R; ++a) out[a] = ml_omega * zz[a];
        } else {
          proj_col<D, R>(ys + L.g * GEO::T, zs + L.g * GEO::T, L.c, zz, out, sdummy);
        }
        const double* rt = rs + L.g * GEO::T + L.c * R;
#pragma unroll
        for (int a = 0; a < R; ++a) part[1] = fma(out[a], rt[a], part[1]);
        store_col<R>(os + L.g * GEO::T + L.c * R, out);
      }
      wave_sync();
      if (z32)
        span_from_lds<D, R>(z32 + base, os, tg.valid);
      else
        span_from_lds<D, R>(z + base, os, tg.valid);
      wave_sync();
    }
    DPGO_STAMP(1, 5);
    if constexpr (PIPE) {
      if (have) {
        tg = tg_n;
#pragma unroll
        for (int k = 0; k < GEO::B; ++k) drow[k] = drow_n[k];
      }
    } else {
      tile += ti_.step;
      have = tile < ti_.last;
      if (have) prefetch(tile);
    }
  }
  if (mode != 1) store_partials<2>(part, pout, red);
  DPGO_STAMP(1, 6);
  DPGO_COMMIT(1);
}

// ================================================================ K7a: tCG residual / iterate update
// ROPTLIB SolversTR::tCG_TR, first half of one inner iteration (and, with first = 1, its
// initialisation r = g, eta = 0, z = P(r)):
//   d_Hd (from k_hess partials) -> alpha, e_Pe';  boundary / negative curvature -> eta += tau*delta, r += tau*Hd, stop
//   else eta += alpha*delta; r += alpha*Hd; z = P(r);  partials: [0] <r,r>  [1] <z,r>
template <int D, int R, int DEF = 0>
__global__ __launch_bounds__(kBlock, DPGO_LB_UPDATE) void k_tcg_update(const double* __restrict__ X, const double* __restrict__ g,
                                                       const double* __restrict__ dinv,
                                                       const double* __restrict__ delta,
                                                       const double* __restrict__ Hd, double* __restrict__ eta,
                                                       double* __restrict__ r, double* __restrict__ z,
                                                       const double* __restrict__ pin, int nb_in,
                                                       double* __restrict__ pout, const DevState* __restrict__ sin,
                                                       DevState* __restrict__ sout, int first, int n,
                                                       unsigned long long* hflag, unsigned gen, double ml_omega,
                                                       double* __restrict__ coef) {
  // generic layout (odd tile size); even tile sizes run k_tcg_update_span
  using GEO = Geo<D, R>;
  __shared__ __attribute__((aligned(16))) double sm[kWaves][3][GEO::G][GEO::T];
  __shared__ double red[kWaves * kNP];
  DevState st;
  load_state(st, sin);
  gen = state_gen(st, gen);
  if (tcg_idle(st, !first)) {
    tcg_publish(sout, st, hflag, gen);
    return;
  }
  double alpha, tau;
  const int mode = tcg_update_prologue(st, pin, nb_in, first, red, alpha, tau);  // 0: step, 1: boundary step, 2: init
  tcg_publish(sout, st, hflag, gen, [&] { tcg_store_coef<DEF>(coef, st, mode, alpha, tau); });

  const LaneId L = lane_id<D>();
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  double part[2] = {0.0, 0.0};
  const TileIter ti_ = tile_iter(ntiles);
  for (int tile = ti_.first; tile < ti_.last; tile += ti_.step) {
    const int i = tile * GEO::P + L.wave * GEO::G + L.g;
    const bool ok = (L.g < GEO::G) && (i < n);
    const size_t off = (size_t)i * GEO::T + L.c * R;
    if (mode == 1) {  // workgroup-uniform
      if (ok) {
        // (r += tau * H delta with it: r = g + H eta holds at every exit of tCG, which is what the rho test reads)
        double rr[R];
        tcg_step_col<R, DEF>(tau, eta + off, delta + off, Hd + off, r + off, rr);
        store_col<R>(r + off, rr);
      }
      continue;
    }
    double* ys = ok ? &sm[L.wave][0][L.g][0] : nullptr;
    double* rs = ok ? &sm[L.wave][1][L.g][0] : nullptr;
    double* zs = ok ? &sm[L.wave][2][L.g][0] : nullptr;
    double rr[R], x[R], zz[R], drow[GEO::B];
    if (ok) {
      // all of this pose's loads are issued back to back (independent addresses)
      load_col<R>(X + off, x);
      if (dinv) {
#pragma unroll
        for (int k = 0; k < GEO::B; ++k) drow[k] = dinv[(size_t)i * GEO::BB + L.c * GEO::B + k];
      }
      if (mode == 2) {
        load_col<R>(g + off, rr);
        if constexpr (!DEF) {
          double e[R];
#pragma unroll
          for (int a = 0; a < R; ++a) e[a] = 0.0;
          store_col<R>(eta + off, e);
        }
      } else {
        tcg_step_col<R, DEF>(alpha, eta + off, delta + off, Hd + off, r + off, rr);
      }
      store_col<R>(r + off, rr);
#pragma unroll
      for (int a = 0; a < R; ++a) part[0] = fma(rr[a], rr[a], part[0]);
      store_col<R>(ys + L.c * R, x);
      store_col<R>(rs + L.c * R, rr);
    }
    wave_sync();
    if (ok) {
      if (dinv) {
        jacobi_col<D, R>(rs, drow, zz);
      } else {
#pragma unroll
        for (int a = 0; a < R; ++a) zz[a] = rr[a];
      }
      store_col<R>(zs + L.c * R, zz);
    }
    wave_sync();
    if (ok) {
      double out[R], s[D];
      if (ml_omega > 0.0) {
#pragma unroll
        for (int a = 0; a < R; ++a) out[a] = ml_omega * zz[a];
      } else {
        proj_col<D, R>(ys, zs, L.c, zz, out, s);
      }
#pragma unroll
      for (int a = 0; a < R; ++a) part[1] = fma(out[a], rr[a], part[1]);
      store_col<R>(z + off, out);
    }
    wave_sync();
  }
  if (mode != 1) store_partials<2>(part, pout, red);
}
