// solve.hip -- QuadraticOptimizer::optimize on the device (src/QuadraticOptimizer.cpp, ROPTLIB RTRNewton / tCG_TR): tCG launches, the one-launch solve, preconditioner selection.
#include "host.h"

namespace dpgo_host {

// f(kernel) for the update-kernel instance this handle's state selects:
//   even pose tile size (span kernels)   ML    DEF (a solve that keeps its directions)   PIPE
//     block-Jacobi / no preconditioner   0     dirs_on                                   0
//     multilevel mode (ml_omega > 0)     1     dirs_on                                   pipe ? kUpdatePipe<D, R, DEF> : 0
//   odd pose tile size: the generic kernel, k_tcg_update<D, R, DEF>
// ML = 1 is its own instance (3 waves per SIMD).  PIPE: DPGO_UPDATE_PIPE=0 selects the instances that request the next tile
// behind the last store (same bits, kernels/tcg.h); only the multilevel instances that hold their three waves with a tile in
// flight have a PIPE = 1 form (kUpdatePipe), and only a launch in which a workgroup can hold a second tile has one to request
// early: with a tile per workgroup -- every block up to the resident count, sphere2500's 40 tiles -- the reference-order
// instance runs.
template <int D, int R, class F>
int dispatch_tcg_update_mode(const dpgo_problem_s* p, bool ml_mode, F&& f) {
  const bool def = p->dirs_on;
  if constexpr (Span<D, R, 1>::kOk) {
    if (!ml_mode) return def ? f(k_tcg_update_span<D, R, 0, 1, 0>) : f(k_tcg_update_span<D, R, 0, 0, 0>);
    const bool pipe = options().update_pipe != 0 && pose_tiles(p->n, p->b) > p->grid_u(ml_mode);
    if (def) return pipe ? f(k_tcg_update_span<D, R, 1, 1, kUpdatePipe<D, R, 1>>) : f(k_tcg_update_span<D, R, 1, 1, 0>);
    return pipe ? f(k_tcg_update_span<D, R, 1, 0, kUpdatePipe<D, R, 0>>) : f(k_tcg_update_span<D, R, 1, 0, 0>);
  } else {
    return def ? f(k_tcg_update<D, R, 1>) : f(k_tcg_update<D, R>);
  }
}

int launch_tcg_update(dpgo_problem_s* p, const double* dinv, int first, double* z_out,
                      double ml_omega) {
  const bool ml_mode = ml_omega > 0.0;
  const int g = p->grid_u(ml_mode);
  // <delta, H delta> of the last Hessian step from region A (with `first` the kernel sums nothing: no test), <r,r>, <z,r> to B
  if (!first) CHK(sums_ready(p->pA));
  double* pb = nullptr;
  CHK(sums_out(p->pB, g, &pb));
  double* zt = z_out ? z_out : p->z;
  // (the pre-smoothed iterate of a cycle that keeps its internal vectors in fp32 goes to that buffer instead)
  float* z32 = (ml_omega > 0.0 && !p->ml.empty() && z_out == p->ml[0].x1 && p->ml_vec32_active()) ? p->ml[0].x1f : nullptr;
  CHK(dispatch_dr(p->d, p->r, [&](auto Dc, auto Rc) {
    constexpr int D = decltype(Dc)::value, R = decltype(Rc)::value;
    // (odd tile size: the generic kernel has no fp32 output -- resolve_tcg_storage keeps such blocks off the symmetric
    // storage, hence off the cycle's fp32 vectors; a state that says otherwise is refused instead of dropping z32)
    if (!Span<D, R, 1>::kOk && z32) return fail(DPGO_ERR_STATE, "fp32 cycle vectors need the span kernels (even pose tile size)");
    // (a solve that keeps its directions: the deferred instances get neither delta nor eta, only the step-length array)
    const bool def = p->dirs_on;
    return dispatch_tcg_update_mode<D, R>(p, ml_mode, [&](auto kernel) {
      auto go = [&](auto... z32_arg) {
        return launch(kernel, g, 0, p->stream, p->x1, p->g1, dinv, def ? nullptr : p->delta.get(), p->Hd,
                      def ? nullptr : p->eta.get(), p->rr, zt, p->pA.in(), p->pA.count(), pb, p->state.in(),
                      p->state.out(), first, p->n, p->hflag, p->gen, ml_omega, def ? p->dirs_coef.get() : nullptr,
                      z32_arg...);
      };
      // (the span kernels end in the fp32 output, the generic one has none)
      if constexpr (Span<D, R, 1>::kOk) return go(z32);
      else return go();
    });
  }));
  HIPC(hipGetLastError());
  p->state.advance();
  return DPGO_OK;
}

// fused direction update + Riemannian Hessian-vector product (one tCG step)
// the tCG-step kernel: span variant whenever the pose tile size is even (all 3-D cases)
// f(kernel, Q in the storage that kernel reads) for the instance this handle's state selects
// (DEF: the instances of a solve that keeps its directions -- their `delta` is the direction ring, kernels/tcg.h)
template <int D, int R, int DEF, class F>
int dispatch_tcg_hess_mode(const dpgo_problem_s* p, F&& f) {
  if constexpr (Span<D, R, 1>::kOk) {
    if (p->tcg_sym) return f(p->stream_nt ? k_tcg_hess_sym<D, R, 1, DEF> : k_tcg_hess_sym<D, R, 0, DEF>, p->sym.dev());
    if (p->stream_nt && p->split == 1) return f(k_tcg_hess_span<D, R, 1, 1, DEF>, p->Q.dev());
    return dispatch_split(p->split, [&](auto Sc) { return f(k_tcg_hess_span<D, R, decltype(Sc)::value, 0, DEF>, p->Q.dev()); });
  } else {
    return dispatch_split(p->split, [&](auto Sc) { return f(k_tcg_hess<D, R, decltype(Sc)::value, DEF>, p->Q.dev()); });
  }
}
template <int D, int R, class F>
int dispatch_tcg_hess(const dpgo_problem_s* p, F&& f) {
  return p->dirs_on ? dispatch_tcg_hess_mode<D, R, 1>(p, f) : dispatch_tcg_hess_mode<D, R, 0>(p, f);
}

int launch_tcg_hess_with(dpgo_problem_s* p, const DevState* sin, DevState* sout, int first, unsigned long long* hflag,
                         unsigned gen) {  // (the state slots and the progress word of the caller's choice: kernel probes)
  if (p->dirs_on && !p->dirs) return fail(DPGO_ERR_STATE, "deferred tCG launch without a direction ring");
  double* dl = p->dirs_on ? p->dirs.get() : p->delta.get();
  // <r,r>, <z,r> from region B (the update kernel's or, in the V-cycle, the level-0 post-smoothing's), <delta, H delta> to A
  CHK(sums_ready(p->pB));
  const int g = p->grid_s();
  double* pa = nullptr;
  CHK(sums_out(p->pA, g, &pa));
  CHK(dispatch_dr(p->d, p->r, [&](auto Dc, auto Rc) {
    constexpr int D = decltype(Dc)::value, R = decltype(Rc)::value;
    return dispatch_tcg_hess<D, R>(p, [&](auto kernel, const auto& Q) {
      return launch(kernel, g, 0, p->stream, Q, p->x1, p->S1, p->z, dl, p->Hd, p->pB.in(), p->pB.count(), pa, sin, sout,
                    first, p->n, hflag, gen);
    });
  }));
  HIPC(hipGetLastError());
  return DPGO_OK;
}
int launch_tcg_hess(dpgo_problem_s* p, int first) {
  CHK(launch_tcg_hess_with(p, p->state.in(), p->state.out(), first, p->hflag, p->gen));
  p->state.advance();
  return DPGO_OK;
}

// the pose tile size is even: the span kernels (and with them the symmetric storage) exist for this pair
static bool span_ok(int d, int r) {
  bool ok = false;
  (void)dispatch_dr(d, r, [&](auto Dc, auto Rc) {
    ok = Span<decltype(Dc)::value, decltype(Rc)::value, 1>::kOk;
    return DPGO_OK;
  });
  return ok;
}

// which storage of Q the tCG-step kernel of the coming launches reads (Q does not change inside a solve)
int resolve_tcg_storage(dpgo_problem_s* p) {
  p->tcg_sym = false;
  p->stream_nt = p->want_stream_nt();
  if (!span_ok(p->d, p->r) || !p->sym_wanted()) return DPGO_OK;
  bool usable = false;
  CHK(sym_ensure(p, &usable));
  p->tcg_sym = usable;
  return DPGO_OK;
}

// Whether the coming multi-launch RTR solve keeps tCG's directions (kernels/tcg.h, DEF) -- decided here, once per solve:
// yes when DPGO_TCG_DIRS is not 0 and a ring of max(1, max_inner) pose vectors fits DPGO_TCG_DIRS_MAX_MB and the device
// (the state record's max_inner is the solve's RTR_tCG_iterations and the last slot a run writes is max_inner - 1, so the
// ring holds every slot a kernel can address).  The ring and its step lengths are allocated on first use and grown when a
// solve has a larger budget; a ring that cannot be allocated leaves the handle without one and the solve on p->delta / p->eta.
// may_alloc = false (the kernel probes, which address slots 0 and 1): deferred only on the ring a solve has left.
int tcg_dirs_ensure(dpgo_problem_s* p, int max_inner, bool may_alloc) {
  p->dirs_on = false;
  if (options().tcg_dirs == 0) return DPGO_OK;
  const int slots = std::max(1, max_inner);
  const size_t slot = (size_t)p->n * p->T;
  if ((double)slots * (double)slot * sizeof(double) > (double)std::max(0, options().tcg_dirs_max_mb) * 1048576.0) return DPGO_OK;
  if (slots > p->dirs_cap || !p->dirs || !p->dirs_coef) {
    if (!may_alloc) return DPGO_OK;
    p->dirs = DevBuf<double>();  // (released first: the old and the new ring never exist side by side)
    p->dirs_coef = DevBuf<double>();
    p->dirs_cap = 0;
    if (p->dirs.alloc((size_t)slots * slot) != DPGO_OK || p->dirs_coef.alloc((size_t)slots + 1) != DPGO_OK) {
      (void)hipGetLastError();  // (out of memory is not an error of the solve)
      p->dirs = DevBuf<double>();
      p->dirs_coef = DevBuf<double>();
      return DPGO_OK;
    }
    HIPC(hipMemsetAsync(p->dirs_coef, 0, sizeof(double) * ((size_t)slots + 1), p->stream));
    p->dirs_cap = slots;
  }
  p->dirs_on = true;
  return DPGO_OK;
}

// ---------------------------------------------------------------------------------------------------------
// One-launch solve (kernels/persist.h, k_rtr_persist): one launch runs QuadraticOptimizer::optimize whole.
//
// Residency.  Every workgroup of such a launch waits for all the others, so all of them must be resident at once.  The
// grid is therefore sized against a per-device count of resident slots shared by all handles of the process (one slot =
// one 256-thread workgroup; capacity = two per CU: every variant of the kernel is compiled for two workgroups per CU
// -- registers, LDS --, whatever else runs), reserved for the duration of the solve.  A handle that cannot reserve runs the
// multi-launch scheme.  Other processes are not covered: every in-kernel spin is bounded, a time-out poisons the state
// record (rtr_stop = kPersistPoison) and leaves the caller's iterate untouched; the solve then runs on the multi-launch
// scheme (one_launch_collect).
constexpr int kMaxDevices = 64;
std::atomic<int> g_warnings{0};  // warnings printed to stderr so far (dpgo_warning_count)
std::atomic<int> g_persist_used[kMaxDevices];
std::atomic<int> g_persist_cap[kMaxDevices];  // 0 = not yet queried

int persist_capacity(int device) {
  int cap = g_persist_cap[device % kMaxDevices].load();
  if (cap == 0) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0) cus = 1;
    cap = 2 * cus;
    g_persist_cap[device % kMaxDevices].store(cap);
  }
  return cap;
}
bool persist_reserve(dpgo_problem_s* p, int slots, int limit) {
  auto& used = g_persist_used[p->device % kMaxDevices];
  int cur = used.load();
  while (cur + slots <= limit)
    if (used.compare_exchange_weak(cur, cur + slots)) {
      p->persist_reserved = slots;
      return true;
    }
  return false;
}
void persist_release(dpgo_problem_s* p) {
  if (p->persist_reserved > 0) g_persist_used[p->device % kMaxDevices].fetch_sub(p->persist_reserved);
  p->persist_reserved = 0;
}

// Geometry of a launch: lane groups per pose (SPLIT), tiles per workgroup (MT), workgroups.  The smallest-latency layout
// whose grid fits the handle's share of the resident slots: 4 lane groups per pose (short gather chains) while the tiles
// fit, otherwise one pose per (d+1) lanes, with up to 2 tiles per workgroup.
bool additive_available(dpgo_problem_s* p) {
  return p->persist && !p->persist_failed_once && additive_plan(p).split != 0;
}
// f(Int<SPLIT>{}, Int<MT>{}, additive as std::bool_constant) for the k_rtr_persist<D, R, SPLIT, MT, ADD> layout of a launch:
// the seven that are compiled -- additive (4, 1), (1, 2), (1, 1); plain (4, 1), (4, 2), (1, 1), (1, 2) -- and the only place that
// turns (lane groups per pose, tiles per workgroup, additive) into one of them
template <class F>
int dispatch_persist(int split, int mt, bool additive, F&& f) {
  if (additive) {
    if (split == 4) return f(Int<4>{}, Int<1>{}, std::true_type{});
    return mt == 2 ? f(Int<1>{}, Int<2>{}, std::true_type{}) : f(Int<1>{}, Int<1>{}, std::true_type{});
  }
  if (split == 4) return mt == 1 ? f(Int<4>{}, Int<1>{}, std::false_type{}) : f(Int<4>{}, Int<2>{}, std::false_type{});
  return mt == 1 ? f(Int<1>{}, Int<1>{}, std::false_type{}) : f(Int<1>{}, Int<2>{}, std::false_type{});
}
// LDS of one workgroup (gfx950: 160 KiB per CU; every persistent instance runs one workgroup per CU)
constexpr size_t kPersistLds = 160 * 1024;
// hipFuncAttributeMaxDynamicSharedMemorySize of a kernel instance as last raised, per device: one counter per instance
template <auto Kernel>
std::atomic<int> g_dynamic_lds_set[kMaxDevices];
// The additive instance of this layout fits one CU with `na` aggregates: its static LDS (as compiled for the handle's
// (d, r)) plus the (d+1) rows of A_c^-1 per workgroup, (d+1)^2 na doubles.  With two tiles per workgroup the static part
// grows with (d+1) r; an instance the compiler could not place is refused here, not at the launch.
bool additive_lds_fits(const dpgo_problem_s* p, int split, int mt, int na) {
  hipFuncAttributes a{};
  const int rc = dispatch_dr(p->d, p->r, [&](auto Dc, auto Rc) {
    return dispatch_persist(split, mt, true, [&](auto Sc, auto Mc, auto Ac) {
      HIPC(hipFuncGetAttributes(&a, reinterpret_cast<const void*>(
                                        &k_rtr_persist<decltype(Dc)::value, decltype(Rc)::value, decltype(Sc)::value,
                                                       decltype(Mc)::value, decltype(Ac)::value>)));
      return DPGO_OK;
    });
  });
  return rc == DPGO_OK && a.sharedSizeBytes + sizeof(double) * (size_t)p->b * p->b * na <= kPersistLds;
}
// `free_slots`: what may be reserved.  Alone on the device (share = 1): the lowest-latency layout that fits (4 lane groups
// per pose while the tiles fit, then one pose per (d+1) lanes).  Sharing the device with `share` concurrently solved
// agents: the lowest-latency layout of which `share` copies fit side by side; if there is none, the most compact one
// (the solves then take turns).
PersistGeo persist_geometry(const dpgo_problem_s* p, int free_slots, int share, bool additive) {
  if (additive) {  // fixed by the hierarchy (after ml_ensure); one workgroup per CU (the rows of the coarse inverse live in its LDS)
    const int sp = additive_split_of(p);
    if (!sp) return PersistGeo();
    PersistGeo g{sp, additive_mt_of(p), p->ml[1].n, 0};
    if (g.mt == 2 && !additive_lds_fits(p, sp, g.mt, g.wgs)) return PersistGeo();  // (the V-cycle runs instead)
    g.slots = g.wgs * persist_slots_per_wg(sp, 1, true);
    if (g.wgs > kPersistMax || g.slots > free_slots) return PersistGeo();
    return g;
  }
  const int env_split = options().persist_split, env_mt = options().persist_mt;
  const int cand[4][2] = {{4, 1}, {4, 2}, {1, 1}, {1, 2}};
  PersistGeo compact;
  for (auto& c : cand) {
    if (env_split && c[0] != env_split) continue;
    if (env_mt && c[1] != env_mt) continue;
    const int wgs = (pose_tiles(p->n, p->b, c[0]) + c[1] - 1) / c[1];
    const int slots = wgs * persist_slots_per_wg(c[0], c[1]);
    if (wgs > kPersistMax || slots > free_slots) continue;
    const PersistGeo g{c[0], c[1], wgs, slots};
    if ((long long)slots * std::max(1, share) <= free_slots) return g;  // everybody fits at once
    if (compact.wgs == 0 || slots < compact.slots) compact = g;
  }
  return compact;
}

// Enqueues the persistent launch of a WHOLE solve (k_rtr_persist; no host wait).  *used = false: not launched (no geometry
// / no free slots) -- the caller runs the multi-launch scheme.
int launch_rtr_persistent(dpgo_problem_s* p, const dpgo_ropt_params* prm, const double* dinv, bool* used, bool additive) {
  *used = false;
  p->gen += 1;
  if (p->persist_stream_ordered) {
    // dpgo_optimize_device_begin: the caller enqueues this handle's solves and everything between them on ONE stream, so
    // no two of its one-launch solves are ever resident together -- nothing to reserve (a reservation could only be
    // released by the collecting call, long after the kernel has left the chip)
    const PersistGeo g = persist_geometry(p, persist_capacity(p->device), 1, additive);
    if (g.wgs <= 0) return DPGO_OK;
    p->persist_split = g.split;
    p->persist_mt = g.mt;
    p->persist_wgs = g.wgs;
    p->persist_add = additive;
  } else if (p->persist_reserved == 0) {
    // Alone on the device: what is free now, first come first served.  Sharing it with other concurrently solved agents:
    // the most compact layout, at most 4/5 of the slots in use at once (a CU that holds a persistent workgroup has no
    // registers left for anything else, and every agent's other kernels -- gradient, retraction, rho test -- need
    // somewhere to run: packing the chip full made a 16-agent sweep slower), and a solve that finds no room WAITS for
    // another one to finish (a solve is well under a millisecond) instead of taking the slow path.
    const int cap = persist_capacity(p->device);
    auto& used = g_persist_used[p->device % kMaxDevices];
    PersistGeo g;
    if (p->persist_share <= 1) {
      g = persist_geometry(p, cap - used.load(), 1, additive);
      if (g.wgs <= 0 || !persist_reserve(p, g.slots, cap)) return DPGO_OK;
    } else {
      // (the additive form's grid is fixed by its hierarchy -- one workgroup per aggregate, up to the whole chip: such solves
      // take turns)
      const int limit = additive ? cap : cap - cap / 5;
      g = persist_geometry(p, limit, p->persist_share, additive);
      if (g.wgs <= 0) return DPGO_OK;
      const auto t0 = std::chrono::steady_clock::now();
      while (!persist_reserve(p, g.slots, limit)) {
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() > 0.05) return DPGO_OK;
        std::this_thread::yield();
      }
    }
    p->persist_split = g.split;
    p->persist_mt = g.mt;
    p->persist_wgs = g.wgs;
    p->persist_add = additive;
  }
  // (the granules' epochs are salted per launch, so what earlier launches left in the table never matches; the table is
  // cleared before a salt can repeat -- every 2047 generations of this handle -- and at creation)
  // (the control block: every field but `error` is assigned by the launch, and `error` is zero unless a launch of this
  // handle timed out -- cleared at creation and behind such a launch only, not by a fill kernel in front of every solve)
  if (p->pctrl_dirty) {
    HIPC(hipMemsetAsync(p->pctrl, 0, sizeof(PersistCtrl), p->stream));
    p->pctrl_dirty = false;
  }
  if (p->gen - p->gran_cleared_at >= 0x7ffu) {  // (the multi-launch scheme advances `gen` too: count, do not test bits)
    HIPC(hipMemsetAsync(p->pgran, 0, sizeof(unsigned long long) * kGranWords, p->stream));
    p->gran_cleared_at = p->gen;
  }
  const unsigned salt = ((p->gen & 0x7ffu) + 1u) << 20;  // never 0; the in-launch step counter fills the low 20 bits
  // granule sweeps of the in-kernel all-reduce: wait before the first one (a granule needs ~1 us to cross the chip and
  // the slowest of more workgroups arrives later; sweeping earlier only loads the fabric: sphere2500 11.9 -> 7.9 us per
  // iteration, 12.5k slab 15.3 -> 12.1), back off between sweeps.  DPGO_POLL_FIRST / DPGO_POLL_SLEEP override.
  const int env_first = options().poll_first, env_sleep = options().poll_sleep;
  // (whole-solve kernel, run r4j, us per product at first = 16 / 24 / 32 / 44 / 56: sphere2500, 157 workgroups of 4 lane
  // groups per pose, 7.3 / 6.5 / 7.0 / 7.6 / 8.3; 6 250 poses, 196 workgroups of the same layout with two tiles, 10.9 / 9.9 /
  // 9.9 / 10.5 / 11.1; 12.5k slab, one pose per (d+1) lanes, 12.0 / 10.9 / 10.7 / 10.5 / 10.4)
  const int first = env_first >= 0 ? std::min(255, env_first)
                                   : (p->persist_split == 4 ? (p->persist_wgs <= 160 ? kPollFirstSleep : 30) : 32);
  // (one pose per (d+1) lanes: 44 until round 6; with the phases that round shortened -- own tiles from LDS, 16-byte cells --
  // the sweep over 12 / 20 / 28 / 36 / 44 / 52 has its best at 28-36: slab additive 17.1 / 15.7 / 14.6 / 14.7 / 15.0 / 15.3,
  // block-Jacobi 10.5 / 9.9 / 9.6 / 9.6 / 9.7 / 9.7, torus3D additive 17.1 / 15.5 / 15.0 / 14.8 / 15.2 / 15.7 us per product;
  // tools/r6/poll_first_sweep.sh)
  const int between = env_sleep >= 0 ? std::min(255, env_sleep) : kPollSleep;
  // (a reduction that also carries the additive preconditioner's payload -- 2 (d+1) r more granules per participant --
  // completes later: its first sweep waits longer; 0 in the argument = as the plain one)
  const int env_first_pay = options().poll_first_pay;
  const int first_pay = env_first_pay >= 0 ? std::min(255, env_first_pay) : kPollFirstPaySleep;
  const int poll = (first_pay << 16) | (first << 8) | between;

  AddDev add{};
  size_t lds = 0;
  if (additive) {
    auto& L0 = p->ml[0];
    auto& C = p->ml[1];
    add = AddDev{L0.Pb, p->dense.inv, p->dense.lda, C.n, C.r, 1.0, L0.graph ? L0.tile_perm : nullptr,
                 L0.graph ? L0.lab : nullptr, L0.graph ? L0.mem_pos : nullptr, L0.graph ? L0.agg_ptr : nullptr};
    lds = sizeof(double) * (size_t)p->b * C.n * p->b;  // (d+1) rows of the inverse
  }
  const RtrArgs ra{prm->gradnorm_tol, prm->RTR_initial_radius, 5.0 * prm->RTR_initial_radius, prm->RTR_tCG_iterations,
                   prm->RTR_iterations, prm->accept_tiny_decrease};
  const double* Glin = p->has_G ? p->G : nullptr;
  // (static + dynamic LDS of the additive instances can exceed 64 KB: the launch attribute is raised to the largest size
  // any handle of the process has asked of that instantiation on that device)
  CHK(dispatch_dr(p->d, p->r, [&](auto Dc, auto Rc) {
    constexpr int D = decltype(Dc)::value, R = decltype(Rc)::value;
    return dispatch_persist(p->persist_split, p->persist_mt, additive, [&](auto Sc, auto Mc, auto Ac) {
      constexpr auto kernel = &k_rtr_persist<D, R, decltype(Sc)::value, decltype(Mc)::value, decltype(Ac)::value>;
      if (lds > 0) {  // the attribute belongs to the instance and the device: only ever raised
        auto& set = g_dynamic_lds_set<kernel>[p->device % kMaxDevices];
        if ((int)lds > set.load()) {
          HIPC(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
          int cur = set.load();
          while (cur < (int)lds && !set.compare_exchange_weak(cur, (int)lds)) {}
        }
      }
      return launch(kernel, p->persist_wgs, lds, p->stream, p->Q.dev(), p->x1, Glin, dinv, p->x2, p->eta, p->z, p->pgran, salt,
                    p->state.slot(0), p->pctrl, p->n, p->hflag, p->gen, poll, ra, add);
    });
  }));
  {  // the iterate reaches the caller's X only if the launch completed on every participant (k_persist_commit)
    const size_t count = (size_t)p->n * p->T;
    const int grid = (int)std::min<size_t>(1024, (count + kBlock - 1) / kBlock);
    // (rewind: slot 0 is the record the solve leaves; the commit kernel also writes it and the control block into the
    // host-coherent copies the caller reads after synchronising)
    launch(k_persist_commit, grid, 0, p->stream, p->state.rewind(), p->pctrl, p->x2, p->x1, count, p->hstate, p->hctrl);
  }
  HIPC(hipGetLastError());
  *used = true;
  return DPGO_OK;
}

void persist_report(dpgo_problem_s* p) {  // (hctrl has been read back with the state record)
  if (!options().persist_verbose) return;
  const double it = std::max<double>(1.0, (double)p->hctrl->ticks[4]);
  std::fprintf(stderr,
               "dpgo_hip: persistent tCG: %u workgroups (%d lane groups per pose, %d tiles each)%s, %u iterations; per "
               "iteration (us): Hessian phase %.2f, all-reduce %.2f, update phase %.2f, all-reduce %.2f; per solve (us): "
               "set-up + initial statistics %.1f, first updates %.1f, retraction / trial point / rho test %.1f\n",
               p->hctrl->members, p->persist_split, p->persist_mt, p->hctrl->error ? " TIMED OUT" : "", p->hctrl->iters,
               0.01 * (double)p->hctrl->ticks[0] / it, 0.01 * (double)p->hctrl->ticks[1] / it,
               0.01 * (double)p->hctrl->ticks[2] / it, 0.01 * (double)p->hctrl->ticks[3] / it,
               0.01 * (double)p->hctrl->ticks[5], 0.01 * (double)p->hctrl->ticks[6], 0.01 * (double)p->hctrl->ticks[7]);
}

// One ROPTLIB SolversTR::Run outer iteration: tCG + retraction + rho test.  State stays on the device; the host
// feeds tCG-step kernels just-in-time (or polls the state every `tcg_poll_interval` inner iterations).
int rtr_outer_iteration(dpgo_problem_s* p, const dpgo_ropt_params* prm, const double* dinv, Counters& cnt,
                        bool poll_at_end) {
  p->gen += 1;
  const bool add = prm->precond == DPGO_PRECOND_ADDITIVE;
  // (additive: where the persistent kernel cannot run -- no free slots, an earlier time-out -- the V-cycle on the same
  // two-level hierarchy takes over)
  const bool ml = prm->precond == DPGO_PRECOND_MULTILEVEL || add;
  if (add) cnt.vcycle_for_additive = true;
  // multilevel: the update kernel writes the pre-smoothing step of level 0 instead of the block-Jacobi z; the cycle's
  // last kernel produces z and the partial sums <r,r>, <z,r>
  auto update = [&](int first) -> int {
    if (ml) {
      CHK(launch_tcg_update(p, dinv, first, p->ml[0].x1, p->ml_omega));
      const bool early_stop = options().ml_early_stop != 0;
      return launch_ml_tail(p, p->x1, p->rr, p->z, &p->pB, p->state.in(), early_stop && !first);
    }
    return launch_tcg_update(p, dinv, first);
  };
  CHK(update(1));
  p->feed.runs += 1;
  const int max_inner = prm->RTR_tCG_iterations;
  auto step = [&](int j) -> int {
    if (j == 0) p->feed.runs_fed += 1;
    p->feed.steps += 1;
    CHK(launch_tcg_hess(p, j == 0 ? 1 : 0));
    return update(0);
  };
  if (max_inner <= 0) CHK(launch_tcg_hess(p, 1));  // only finalises the tCG state (eta = 0)
  bool done = false;
  if (prm->tcg_poll_interval > 0) {
    // polling mode: enqueue `poll` iterations, then synchronise and read the state back
    const int poll = prm->tcg_poll_interval;
    int j = 0;
    while (j < max_inner) {
      const int chunk = (max_inner - j) < poll ? (max_inner - j) : poll;
      for (int c = 0; c < chunk; ++c) CHK(step(j + c));
      j += chunk;
      CHK(poll_state(p));
      if (p->hstate->tcg_done || p->hstate->rtr_stop) {
        done = true;
        break;
      }
    }
  } else {
    // just-in-time feed: stay kAhead iterations ahead of the progress word the device publishes into
    // host-coherent memory; no synchronisation, no copy, at most kAhead wasted (early-exit) iterations
    // a multilevel iteration is 5+ launches: waste fewer of them after tCG stops.  (2 is the minimum: iteration j's count
    // is published by the prologue of iteration j+1's Hessian-step kernel, so one iteration ahead never sees progress --
    // tried in round 4, the watchdog fires.)
    int kAhead = ml ? 2 : 4;
    if (options().tcg_ahead > 0) kAhead = std::max(2, options().tcg_ahead);  // tuning knob (>= 2, see above)
    // The two-level V-cycle with the restriction's stop check (DPGO_ML_EARLY_STOP, the default) is fed on TICKETS instead:
    // the device says whether an iteration will run before the host enqueues it.
    //  * step 0 waits for this run's generation in the word: the opening update's prologue publishes it, with rtr_stop when
    //    the previous outer iteration met the stop test -- such a run costs its opening launches and nothing else; otherwise
    //    step 0 is enqueued while the opening cycle runs;
    //  * step s + 1 waits for the go ticket of iteration s (kProgressGo, common.h), which the restriction of step s publishes
    //    once its residual test has not held: the rest of that restriction, the aggregate sum, the dense level and the
    //    post-smoothing are still queued then, so the queue does not run dry, and a run that ends in iteration s has nothing
    //    of iteration s + 1 behind it.
    // Every wait is for a launch that is already enqueued and that completes without the host (each publishes the ticket,
    // tcg_done or rtr_stop), so a wait ends whatever other streams do.  The shrink loop, deeper hierarchies and every other
    // preconditioner keep the rule above.
    const bool tickets = ml && !poll_at_end && options().ml_early_stop != 0 && p->ml.size() == 2;
    int enq = 0;
    unsigned long long last_w = ~0ull;
    auto t_progress = std::chrono::steady_clock::now();
    while (true) {
      const unsigned long long w = __atomic_load_n(p->hflag.get(), __ATOMIC_ACQUIRE);
      const bool current = (unsigned)(w >> 32) == p->gen;
      int dev_j = 0;
      if (current) {
        dev_j = (int)((w >> 8) & 0xFFFFFFu);
        if (w & (kProgressDone | kProgressRtrStop)) {
          done = true;
          if (w & kProgressRtrStop) p->saw_rtr_stop = true;
          break;
        }
      }
      if (enq >= max_inner) break;
      // the watchdog measures time WITHOUT progress (a word of this run that changes), not time since the loop started
      const unsigned long long w_run = current ? w : 0ull;
      if (w_run != last_w) {
        last_w = w_run;
        t_progress = std::chrono::steady_clock::now();
      }
      const bool feed = tickets ? (current && (enq == 0 || ((w & kProgressGo) && dev_j >= enq - 1))) : (enq < dev_j + kAhead);
      if (feed) {
        CHK(step(enq));
        enq += 1;
      } else {
        __builtin_ia32_pause();
        if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_progress).count() > 60.0) {
          HIPC(hipStreamSynchronize(p->stream));  // surfaces a device fault instead of spinning forever
          return fail(DPGO_ERR_HIP, "tCG progress word did not advance for 60 s");
        }
      }
    }
  }
  if (!done) CHK(launch_tcg_hess(p, 0));  // max_inner iterations enqueued, not (yet known to be) finished: last prologue
  if (p->saw_rtr_stop) return DPGO_OK;  // the previous outer iteration already met the stop test
  // rho test: <eta, H eta> and <eta, g1> from tCG's own residual, r = g1 + H eta at every exit of tCG (k_tcg_update; nothing
  // between tCG and here writes r: the cycle only reads it), summed by the retraction from the eta it loads anyway.
  // DPGO_RHO_EXACT=1: from a fresh H eta instead, one more pass over Q (the reference path of the tests).
  const bool rho_exact = options().rho_exact != 0;
  // (a solve that kept its directions: the retraction forms eta from them, and leaves it in p->eta for the exact tail)
  CHK(launch_retract(p, p->x1, p->eta, 1.0, p->x2, p->state.in(), rho_exact ? nullptr : p->rr.get(),
                     rho_exact ? nullptr : p->g1.get(), p->dirs_on));
  CHK(launch_grad(p, p->x2, p->g2, p->S2, nullptr, p->state.in(), p->tcg_sym && outer_sym_enabled()));
  cnt.spmm += 1;
  if (rho_exact) {
    CHK(launch_hess(p, p->x1, p->S1, p->eta, p->g1, p->Hd, p->state.in(), 0, p->tcg_sym && outer_sym_enabled()));
    cnt.spmm += 1;
  }
  CHK(launch_rtr_update(p));  // (exchanges the roles of g1 / g2 and S1 / S2)
  if (poll_at_end) CHK(poll_state(p));
  return DPGO_OK;
}

// DPGO_PRECOND_AUTO after a solve: what the next one runs (dpgo_hip.h).  `used` = the preconditioner the solve resolved to,
// `products` = its Hessian-vector products.
//   * a block without coupling to other agents never hands back (its cheap early calls end on the trust-region boundary
//     after a few products whatever the preconditioner, and the switch back and forth cost the 100k grid 37.6 against
//     29.3 ms);
//   * a coupled block the additive one-launch solve cannot hold: hysteresis on the share of the tCG budget a solve used
//     (the V-cycle is ~3x a block-Jacobi iteration: it pays when the budget binds);
//   * a coupled block the additive solve CAN hold (<= ~14 000 poses): the cost rule.  Q is constant across RBCD sweeps, so
//     the hierarchy is paid once: when the block-Jacobi solves since the last change of Q have cost as much as one set-up
//     (kAutoSetupUnits: 2.8-3.0 ms against 9.9-10.6 us per block-Jacobi product on 6 250 / 12 500 poses), the next solve
//     runs additive on trial; it stays while its products x the additive unit cost (19 us) stay below the reference
//     block-Jacobi solve's x the block-Jacobi unit cost, and hands back otherwise (the hierarchy is kept: the next trial
//     is free but waits twice as long).
//     The unit costs are those of a solve that has the device to itself.  A handle solved NEXT TO others of the device
//     (dpgo_optimize_device_many, persist_share > 1) is charged for the part of the chip its launch blocks instead: the
//     additive form owns one CU per aggregate (up to the whole chip: such solves take turns), block-Jacobi's compact
//     layout a quarter to a half of it, so there a product costs [us] x max(resident slots / slots in use at once, 1 / share)
//     x share -- the same figure as alone whenever every concurrently solved handle fits at once.
// (round 6: an additive iteration is two chip-wide reductions, as a block-Jacobi one -- 11.0 against 9.6 us on a 12 500-pose
// slab, 8.7 against 6.6 on sphere2500; it was 15.7 / 10.6 with three: 18 units)
constexpr int kAutoUnitsJacobi = 10, kAutoUnitsAdditive = 13, kAutoSetupUnits = 2800, kAutoMinProducts = 6;
// (the two-tile additive layout, dpgo_problem_additive_tiles = 2, has a unit of its own, not reported by
// dpgo_auto_rule_constants: 10 x the ratio of the two in-kernel iterations on the same 25 000-pose rank share of
// grid:50x50x20 -- additive on two tiles 33.8 us (the instance spills), block-Jacobi on two tiles 15.4 us;
// profiles/two_tile_additive.txt)
constexpr int kAutoUnitsAdditive2 = 22;
int auto_units_jacobi(dpgo_problem_s* p) {
  const int share = std::max(1, p->persist_share);
  if (share == 1 || !p->persist) return kAutoUnitsJacobi;
  const int cap = persist_capacity(p->device), limit = cap - cap / 5;  // (what launch_rtr_persistent lets such solves use)
  const PersistGeo g = persist_geometry(p, limit, share, false);
  if (g.wgs <= 0) return kAutoUnitsJacobi;
  const double part = std::max((double)g.slots / limit, 1.0 / share);
  // (two tiles per workgroup cost 1.25x per product with 4 lane groups per pose; with one pose per (d+1) lanes -- the
  // 12 500-pose slabs -- that variant keeps 512 registers and spills: measured under sharing 22 us per product against
  // 9.4 alone, i.e. two such solves side by side gain nothing over one after the other: 2.1x.  Round 6, loop-back sweeps
  // 8 x 12 500: forced block-Jacobi 3.81 ms, forced additive 3.05 ms, the rule with 1.25x here 3.72 ms -- a mix.)
  const double two_tiles = g.mt == 2 ? (g.split == 1 ? 2.1 : 1.25) : 1.0;
  return std::max(1, (int)std::lround(kAutoUnitsJacobi * two_tiles * part * share));
}
int auto_units_additive(dpgo_problem_s* p) {  // (after additive_available(p): the plan exists)
  const int share = std::max(1, p->persist_share);
  const int units = p->add_plan.tile == 2 * ml_tile(p->b, 1) ? kAutoUnitsAdditive2 : kAutoUnitsAdditive;
  if (share == 1) return units;
  const int cap = persist_capacity(p->device);
  const double part = std::max((double)(p->add_plan.na * persist_slots_per_wg(p->add_plan.split, 1, true)) / cap, 1.0 / share);
  return std::max(1, (int)std::lround(units * part * share));
}
void auto_update(dpgo_problem_s* p, const dpgo_ropt_params* prm, int used, int products) {
  const int budget = std::max(1, prm->RTR_iterations) * std::max(1, prm->RTR_tCG_iterations);
  const bool coupled = p->has_G || p->C.nnzb > 0;
  auto& a = p->auto_cost;
  a.last_used = used;
  a.last_products = products;
  if (!coupled) {
    if (!p->auto_ml && 2 * products >= budget) p->auto_ml = true;
    return;
  }
  const bool cost_rule = options().auto_cost_rule != 0;
  if (!p->auto_ml) {  // the solve ran block-Jacobi
    a.state = 0;
    a.uj = auto_units_jacobi(p);
    a.jac_units += (long long)kAutoUnitsJacobi * products;  // (the set-up is wall time: paid back in solo units)
    const bool binds = 2 * products >= budget;
    const bool paid = cost_rule && products >= kAutoMinProducts && a.jac_units >= ((long long)kAutoSetupUnits << a.backoff);
    if (binds || paid) {
      // (the plan -- host aggregation, once per block pattern -- is only looked for when the rule wants it)
      const bool add = cost_rule && !p->ml_user_ks && additive_available(p);
      if (add) a.ua = auto_units_additive(p);
      // a trial that cannot win is not run: even at kAutoMinProducts the additive solve would cost more than this one did
      const bool hopeless = add && !binds && (long long)a.ua * kAutoMinProducts >= (long long)a.uj * products;
      if (hopeless) {
        a.jac_units = 0;
        a.backoff = std::min(a.backoff + 1, 6);
      } else if (binds || add) {
        p->auto_ml = true;
        if (add) {
          a.state = 1;
          a.ref = products;
          a.switches += 1;
        }
      }
    }
    return;
  }
  if (a.state == 0) {  // a multilevel choice outside the cost rule (V-cycle blocks, dpgo_problem_auto_state): budget hysteresis
    if (10 * products <= budget) p->auto_ml = false;
    return;
  }
  a.ua = auto_units_additive(p);
  // on trial: strictly cheaper than the reference solve; once accepted: handed back only when 15 % dearer (the two are
  // within a few per cent of each other on interior blocks of a chain partition -- no flapping)
  const long long cost = (long long)a.ua * products * 100, ref = (long long)a.uj * a.ref * (a.state == 2 ? 115 : 100);
  if (cost < ref) {
    a.state = 2;
  } else {  // no cheaper than block-Jacobi on this block in this phase of the run: hand back, try again later
    p->auto_ml = false;
    a.state = 0;
    a.jac_units = 0;
    a.backoff = std::min(a.backoff + 1, 6);
  }
}

// A solve is planned (plan_solve), then either enqueued as ONE launch (one_launch_enqueue) and collected
// (one_launch_collect) -- by the same call, or by dpgo_optimize_device_end for what ..._begin enqueued -- or run on the
// multi-launch scheme (multi_launch_solve), which is also what follows a one-launch solve that timed out.
// X is in p->x1 on entry and on exit.  src/QuadraticOptimizer.cpp:26-48.

// Everything a solve decides before its first launch: the preconditioner (and its factors), the storage of Q the tCG-step
// kernel reads, whether the one-launch kernel may run.
int plan_solve(dpgo_problem_s* p, const dpgo_ropt_params* prm, SolvePlan* plan) {
  plan->t0 = std::chrono::steady_clock::now();
  if (p->hctrl) std::memset(p->hctrl, 0, sizeof(PersistCtrl));
  p->dirs_on = false;  // (the one-launch solve keeps its vectors on chip)
  plan->prm = *prm;    // DPGO_PRECOND_AUTO -> what this handle currently runs
  plan->is_auto = prm->precond == DPGO_PRECOND_AUTO;
  if (plan->is_auto) {
    p->auto_decide();
    // (the multilevel choice: the additive form wherever its persistent kernel runs)
    plan->prm.precond = (p->auto_ml && prm->method == DPGO_METHOD_RTR)
                            ? ((additive_available(p) && !p->ml_user_ks) ? DPGO_PRECOND_ADDITIVE : DPGO_PRECOND_MULTILEVEL)
                            : DPGO_PRECOND_BLOCK_JACOBI;
  }
  prm = &plan->prm;
  plan->dinv = nullptr;
  if (prm->precond == DPGO_PRECOND_BLOCK_JACOBI) {
    CHK(build_dinv(p, prm->precond_shift));
    plan->dinv = p->dinv;
  } else if (prm->precond == DPGO_PRECOND_MULTILEVEL) {
    // built lazily for the current Q, like the reference's factor (src/PoseGraph.cpp:582-586)
    CHK(ml_ensure(p, prm->precond_shift));
    plan->dinv = p->dinv;  // the smoother's block-Jacobi factors (same shift)
  } else if (prm->precond == DPGO_PRECOND_ADDITIVE) {
    if (prm->method != DPGO_METHOD_RTR) return fail(DPGO_ERR_UNSUPPORTED, "the additive preconditioner exists inside the tCG loop only");
    if (!additive_split_of(p) && !additive_plan(p).split)
      return fail(DPGO_ERR_UNSUPPORTED, "additive preconditioner: block too large (at most 256 aggregates of one workgroup tile, " +
                                            std::to_string(ml_tile(p->b, 1)) + " poses" +
                                            (additive_tiles(p) == 2 ? ", or of two" : "; dpgo_problem_additive_tiles: two") + ")");
    CHK(ml_ensure(p, prm->precond_shift, /*additive=*/true));
    plan->dinv = p->dinv;
  } else if (prm->precond != DPGO_PRECOND_NONE) {
    return fail(DPGO_ERR_INVALID, "unknown preconditioner");
  }
  p->loop_extra_bytes = 0;
  if (prm->precond == DPGO_PRECOND_MULTILEVEL && !p->ml.empty()) {
    const size_t nd = (size_t)p->dense.lda;
    size_t bytes = nd * nd * (size_t)(p->ml_coarse_bits / 8) / (p->ml_use_dense_sym() ? 2 : 1);
    const auto& L0 = p->ml[0];
    bytes += (size_t)L0.AP.nnzb * (sizeof(double) * p->b * p->b + sizeof(int32_t)) + sizeof(double) * (size_t)p->n * p->b * p->b;
    bytes += 3 * p->vec_bytes();
    p->loop_extra_bytes = bytes;
  }
  CHK(resolve_tcg_storage(p));
  if (prm->precond == DPGO_PRECOND_MULTILEVEL) CHK(ml_ops32_ensure(p));  // (opt-in fp32 operator copies of the cycle)
  // ---- blocks in the latency regime: the whole solve is ONE persistent launch (k_rtr_persist) and one read-back.  The
  // single-iteration radius-shrink mode (:80-99) and the polling mode keep the multi-launch scheme.
  // (the in-kernel all-reduce tags its granules with salt | step, the step counter in the low 20 bits: a solve whose
  // parameters allow more reductions than that -- at most 3 per tCG iteration + 4 per outer iteration + 1 -- keeps the
  // multi-launch scheme)
  const bool epochs_fit = (long long)std::max(1, prm->RTR_iterations) * (3LL * std::max(0, prm->RTR_tCG_iterations) + 4) + 1 < (1LL << 20);
  plan->one_launch = prm->method == DPGO_METHOD_RTR && prm->RTR_iterations != 1 && prm->tcg_poll_interval <= 0 && p->persist &&
                     epochs_fit && !p->persist_failed_once &&
                     (prm->precond == DPGO_PRECOND_ADDITIVE || prm->precond == DPGO_PRECOND_BLOCK_JACOBI ||
                      prm->precond == DPGO_PRECOND_NONE);
  return DPGO_OK;
}

// *used = false: not launched (no geometry / no free slots) -- the caller runs the multi-launch scheme
int one_launch_enqueue(dpgo_problem_s* p, const SolvePlan& plan, bool* used) {
  return launch_rtr_persistent(p, &plan.prm, plan.dinv, used, plan.prm.precond == DPGO_PRECOND_ADDITIVE);
}

// Waits for an enqueued one-launch solve.  *ok = false: it timed out (the launch's workgroups were not all resident: another
// process on the device) -- the caller's iterate is untouched, this handle stops using the kernel and the caller runs the
// solve on the multi-launch scheme.
int one_launch_collect(dpgo_problem_s* p, const SolvePlan& plan, dpgo_ropt_result* res, bool* ok) {
  *ok = false;
  std::memset(res, 0, sizeof(*res));
  res->tCGStatus = DPGO_TCG_MAXITER;
  // (no read-back commands: k_persist_commit has written the state record and the control block into hstate / hctrl)
  HIPC(hipStreamSynchronize(p->stream));
  persist_report(p);
  // (k_persist_commit, which ran behind the solve, saw the same two words: with a poisoned record OR a raised time-out
  // flag -- some participant gave up, however late -- the caller's iterate has not been touched)
  if (p->hstate->rtr_stop == kPersistPoison || p->hctrl->error) {
    p->persist_failed_once = true;
    p->pctrl_dirty = true;
    persist_release(p);
    if (options().persist_verbose)
      std::fprintf(stderr, "dpgo_hip: persistent solve timed out; this handle continues with the multi-launch scheme\n");
    return DPGO_OK;
  }
  const DevState& h = *p->hstate;
  res->fInit = h.fInit;
  res->gradNormInit = h.gnInit;
  res->fOpt = h.f1;
  res->gradNormOpt = h.ngf;
  res->tCGStatus = h.outer_iter > 0 ? h.tcg_status : DPGO_TCG_MAXITER;
  res->rtr_iterations = h.outer_iter;
  res->rtr_accepted = h.n_accept;
  res->latest_step_accepted = h.accepted_last;
  res->tcg_iterations = h.n_hess;
  p->feed = dpgo_problem_s::FeedCounts();  // (nothing is fed: the launch runs the loop itself)
  p->feed.products = h.n_hess;
  res->precond_used = plan.prm.precond;
  res->spmm_count = 1 + 2 * h.outer_iter + h.n_hess;
  if (plan.is_auto) auto_update(p, &plan.prm, plan.prm.precond, h.n_hess);
  res->success = 1;  // :44
  res->elapsedMs = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - plan.t0).count();
  *ok = true;
  return DPGO_OK;
}

int multi_launch_solve(dpgo_problem_s* p, const SolvePlan& plan, dpgo_ropt_result* res) {
  const dpgo_ropt_params* prm = &plan.prm;
  const double* dinv = plan.dinv;
  Counters cnt;
  std::memset(res, 0, sizeof(*res));
  res->tCGStatus = DPGO_TCG_MAXITER;
  p->feed = dpgo_problem_s::FeedCounts();
  // whether this solve's tCG runs keep their directions (every launch follows it)
  p->dirs_on = false;
  if (prm->method == DPGO_METHOD_RTR) CHK(tcg_dirs_ensure(p, prm->RTR_tCG_iterations));
  // statistics before optimisation (:28-29) -- one fused pass: f, rgrad, S
  CHK(launch_grad(p, p->x1, p->g1, p->S1, nullptr, nullptr, prm->method == DPGO_METHOD_RTR && p->tcg_sym && outer_sym_enabled()));
  cnt.spmm += 1;
  CHK(launch_rtr_begin(p, prm->gradnorm_tol, prm->RTR_initial_radius, 5.0 * prm->RTR_initial_radius,
                       prm->RTR_tCG_iterations, prm->accept_tiny_decrease));
  // The initial statistics are read back together with the final ones when the solve is fed just-in-time (one
  // synchronisation per call instead of two): an iterate that already meets the tolerance (:57-59) makes the first tCG
  // launch publish rtr_stop, which ends the loop below before anything is changed.
  const bool deferred = prm->method == DPGO_METHOD_RTR && prm->RTR_iterations != 1 && prm->tcg_poll_interval <= 0;
  if (!deferred) {
    CHK(poll_state(p));
    res->fInit = p->hstate->fInit;
    res->gradNormInit = p->hstate->gnInit;
  } else {
    p->hstate->rtr_stop = 0;
  }
  int n_hess_total = 0;
  int shrink_tries = 0;

  if (prm->method == DPGO_METHOD_RTR) {
    // trustRegion(): src/QuadraticOptimizer.cpp:50-108
    if (!p->hstate->rtr_stop) {  // :57-59 early-out
      if (prm->RTR_iterations == 1) {  // :80-99 shrink the radius until the step is accepted
        double radius = prm->RTR_initial_radius;
        int total_steps = 0;
        while (true) {
          shrink_tries += 1;
          p->hstate->Delta = radius;
          p->hstate->Delta_max = radius;
          p->hstate->outer_iter = 0;
          CHK(push_state(p));
          p->saw_rtr_stop = false;
          CHK(rtr_outer_iteration(p, prm, dinv, cnt, true));
          if (p->hstate->accepted_last) break;
          if (total_steps > 10) break;  // "Too many RTR rejections. Returning initial guess." (x1 untouched)
          radius /= 4.0;
          total_steps++;
        }
      } else {
        const bool polling = prm->tcg_poll_interval > 0;
        p->saw_rtr_stop = false;
        for (int it = 0; it < prm->RTR_iterations; ++it) {
          CHK(rtr_outer_iteration(p, prm, dinv, cnt, polling));
          if (polling ? (p->hstate->rtr_stop != 0) : p->saw_rtr_stop) break;
          const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - plan.t0).count();
          if (prm->time_bound_s > 0 && el > prm->time_bound_s) break;  // Solver.TimeBound (:78)
        }
        CHK(poll_state(p));
        if (deferred) {
          res->fInit = p->hstate->fInit;
          res->gradNormInit = p->hstate->gnInit;
        }
      }
      res->tCGStatus = p->hstate->tcg_status;
      res->rtr_iterations = (prm->RTR_iterations == 1) ? shrink_tries : p->hstate->outer_iter;
      res->rtr_accepted = p->hstate->n_accept;
      res->latest_step_accepted = p->hstate->accepted_last;
      n_hess_total = p->hstate->n_hess;
    }
    res->fOpt = p->hstate->f1;
    res->gradNormOpt = p->hstate->ngf;
  } else if (prm->method == DPGO_METHOD_RGD) {
    // gradientDescent(): src/QuadraticOptimizer.cpp:110-137 (one fixed-step preconditioned step)
    const double* step = p->g1;
    if (prm->RGD_use_preconditioner) {
      if (prm->precond == DPGO_PRECOND_MULTILEVEL)
        CHK(launch_ml_apply(p, p->x1, p->g1, p->z));
      else
        CHK(launch_precond(p, p->x1, p->g1, dinv, p->z));
      step = p->z;
    }
    CHK(launch_retract(p, p->x1, step, -prm->RGD_stepsize, p->x2, nullptr));
    HIPC(hipMemcpyAsync(p->x1, p->x2, p->vec_bytes(), hipMemcpyDeviceToDevice, p->stream));
    CHK(launch_grad(p, p->x1, p->g1, p->S1, nullptr));
    cnt.spmm += 1;
    CHK(launch_rtr_begin(p, prm->gradnorm_tol, prm->RTR_initial_radius, 5.0 * prm->RTR_initial_radius,
                         prm->RTR_tCG_iterations, prm->accept_tiny_decrease));
    CHK(poll_state(p));
    res->fOpt = p->hstate->f1;
    res->gradNormOpt = p->hstate->ngf;
  } else {
    return fail(DPGO_ERR_INVALID, "unknown method");
  }
  res->tcg_iterations = n_hess_total;
  p->feed.products = n_hess_total;
  res->precond_used = (prm->precond == DPGO_PRECOND_ADDITIVE && cnt.vcycle_for_additive) ? DPGO_PRECOND_MULTILEVEL : prm->precond;
  if (plan.is_auto && prm->method == DPGO_METHOD_RTR) auto_update(p, prm, res->precond_used, n_hess_total);
  res->spmm_count = cnt.spmm + n_hess_total;
  res->success = 1;  // :44 (set unconditionally after a solve)
  res->elapsedMs = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - plan.t0).count();
  return DPGO_OK;
}

// The whole solve, synchronously.
int run_optimize(dpgo_problem_s* p, const dpgo_ropt_params* prm, dpgo_ropt_result* res) {
  struct SlotGuard {  // the resident-slot reservation of the persistent kernel lives as long as the solve
    dpgo_problem_s* p;
    ~SlotGuard() { persist_release(p); }
  } slot_guard{p};
  SolvePlan plan;
  bool used = false, ok = false;
  CHK(plan_solve(p, prm, &plan));
  if (plan.one_launch) CHK(one_launch_enqueue(p, plan, &used));
  if (used) CHK(one_launch_collect(p, plan, res, &ok));
  return ok ? DPGO_OK : multi_launch_solve(p, plan, res);
}

int BorrowedIterate::begin(dpgo_problem_s* p, double* X_dev) {
  if (!aligned8(X_dev)) return fail(DPGO_ERR_INVALID, "iterate not 8-byte aligned");
  // the caller's buffer IS the iterate for the duration of the solve (no copies in or out): accepted steps are written
  // into it by k_rtr_update, rejected ones leave it untouched -- unless it is not 16-byte aligned (the tCG and cycle
  // kernels read the iterate in 16-byte pieces): then the solve runs on the handle's own x1, copied in here and out when
  // the solve has ended -- stream-ordered, as the solve itself
  own_x1 = p->x1;
  staged = aligned16(X_dev) ? nullptr : X_dev;
  if (staged) HIPC(hipMemcpyAsync(own_x1, staged, p->vec_bytes(), hipMemcpyDeviceToDevice, p->stream));
  else p->x1 = X_dev;
  return DPGO_OK;
}
int BorrowedIterate::end(dpgo_problem_s* p, int rc) {
  p->x1 = own_x1;
  if (rc == DPGO_OK && staged) HIPC(hipMemcpyAsync(staged, own_x1, p->vec_bytes(), hipMemcpyDeviceToDevice, p->stream));
  return rc;
}

// The two kernels of the tCG loop run as persistent grids: one workgroup per resident slot (occupancy x CUs).
// More workgroups than slots only add prologues (state record + partial-sum reduction) and a ragged second
// round: 100k poses, same box: caps 1024/1024 -> 70.7 us per tCG iteration, 512/768 (= the resident counts of
// k_tcg_update / k_tcg_hess at 203 / 164 VGPRs) -> 64.7 us.  The other kernels keep the family's cap.
template <class K>
int resident_blocks(K kernel, int* out) {
  int per_cu = 0;
  HIPC(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kBlock, 0));
  int dev = 0, cus = 0;
  HIPC(hipGetDevice(&dev));
  HIPC(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
  *out = std::max(1, std::min(kPartialCap, per_cu * cus));
  return DPGO_OK;
}
template <class K>
int lower_to_resident(K kernel, int* cap) {  // *cap = min(*cap, resident count of `kernel`)
  int c = 0;
  CHK(resident_blocks(kernel, &c));
  *cap = std::min(*cap, c);
  return DPGO_OK;
}
int tune_launch_caps(dpgo_problem_s* p) {
  // Which instance each cap is read from -- not always the one a launch then picks; the grids were measured with these:
  CHK(dispatch_dr(p->d, p->r, [&](auto Dc, auto Rc) {
    constexpr int D = decltype(Dc)::value, R = decltype(Rc)::value;
    if constexpr (Span<D, R, 1>::kOk) {
      // (the reference-order instances, PIPE = 0: the grids do not follow DPGO_UPDATE_PIPE; both orders have these counts)
      CHK(resident_blocks(k_tcg_update_span<D, R, 0, 0, 0>, &p->cap_u));
      CHK(resident_blocks(k_tcg_update_span<D, R, 1, 0, 0>, &p->cap_u_ml));
      // cap_hs: the non-temporal instance <D, R, 1>, also when <D, R, 0> runs
      CHK(resident_blocks(k_tcg_hess_sym<D, R, 1>, &p->cap_hs));
    } else {
      CHK(resident_blocks(k_tcg_update<D, R>, &p->cap_u));
      p->cap_u_ml = p->cap_u;  // (one kernel for both modes)
    }
    CHK(dispatch_split(p->split, [&](auto Sc) {
      constexpr int S = decltype(Sc)::value;
      // cap_h: the span kernel's default-NTS instance of this split, also when the non-temporal <D, R, 1, 1> runs
      if constexpr (Span<D, R, 1>::kOk)
        CHK(resident_blocks(k_tcg_hess_span<D, R, S>, &p->cap_h));
      else
        CHK(resident_blocks(k_tcg_hess<D, R, S>, &p->cap_h));
      // cap_restrict / cap_post: the plain-storage fp64 instance of this split ...
      CHK(resident_blocks(k_ml_restrict<D, R, S, BsrDev>, &p->cap_restrict));
      CHK(resident_blocks(k_ml_post_ap<D, R, S>, &p->cap_post));
      return DPGO_OK;
    }));
    if (p->split != 4 && p->split != 2) {
      // ... and at one pose per D+1 lanes only, the smallest count over the variants a cycle may launch (symmetric storage,
      // fp32 copies) -- a grid sized for a variant with more resident workgroups than the launched one leaves part of it
      // waiting for a slot
      CHK(lower_to_resident(k_ml_restrict<D, R, 1, BsrSymDev, double, double>, &p->cap_restrict));
      CHK(lower_to_resident(k_ml_restrict<D, R, 1, BsrSymDev32, float, float>, &p->cap_restrict));
      CHK(lower_to_resident(k_ml_restrict<D, R, 1, BsrSymDev32, float, double>, &p->cap_restrict));
      CHK(lower_to_resident(k_ml_post_ap<D, R, 1, float, float>, &p->cap_post));
      CHK(lower_to_resident(k_ml_post_ap<D, R, 1, float, double>, &p->cap_post));
    }
    // cap_spmm_sym: the non-temporal instance, also when <D, R, 0> runs; cap_outer_sym: the smaller of k_grad's and k_hess's
    p->cap_spmm_sym = p->cap_outer_sym = kMaxGrid;
    CHK(lower_to_resident(k_spmm_sym<D, R, 1>, &p->cap_spmm_sym));
    CHK(lower_to_resident(k_grad<D, R, 1, BsrSymDev>, &p->cap_outer_sym));
    CHK(lower_to_resident(k_hess<D, R, 1, BsrSymDev>, &p->cap_outer_sym));
    return DPGO_OK;
  }));
  if (options().grid_ml > 0) p->cap_restrict = p->cap_post = std::min(kPartialCap, options().grid_ml);
  // tuning knobs (any value up to the partial-sum capacity is valid)
  if (options().grid_update > 0) p->cap_u = p->cap_u_ml = std::min(kPartialCap, options().grid_update);
  if (options().grid_hess > 0) p->cap_h = std::min(kPartialCap, options().grid_hess);
  if (options().grid_hess_sym > 0) p->cap_hs = std::min(kPartialCap, options().grid_hess_sym);
  if (options().grid_outer_sym > 0) p->cap_outer_sym = std::min(kPartialCap, options().grid_outer_sym);
  if (options().grid_spmm_sym > 0) p->cap_spmm_sym = std::min(4096, options().grid_spmm_sym);
  return DPGO_OK;
}

// One-launch solve: on by size -- every block the kernel can hold (two 64-pose tiles on each of 256 workgroups: 32 768 poses
// in 3-D; measured per Hessian-vector product against the multi-launch scheme: 625 poses 6.6 / 13.7 us, sphere2500 6.5 /
// 15.4, 6 250 9.9 / 17.2, 12.5k slab 10.5 / 19.7, 25k 18.7 / 26.5).  DPGO_PERSIST_MAX_POSES lowers the limit, DPGO_PERSIST=0/1
// overrides.
int tune_persist(dpgo_problem_s* p) {
  const int max_poses = options().persist_max_poses > 0 ? options().persist_max_poses : 1 << 30;
  const bool fits = persist_geometry(p, persist_capacity(p->device)).wgs > 0;
  bool on = fits && p->n <= max_poses;
  if (options().persist >= 0) on = fits && options().persist != 0;
  p->persist = on;
  return DPGO_OK;
}

}  // namespace dpgo_host

extern "C" {


int dpgo_problem_auto_state(dpgo_problem_t p, int* use_multilevel) {
  if (!p || !use_multilevel) return fail(DPGO_ERR_INVALID, "null pointer");
  if (*use_multilevel >= 0) {
    p->auto_ml = *use_multilevel != 0;
    p->auto_decided = true;
    p->auto_cost = dpgo_problem_s::AutoCost();  // (a choice made from outside is followed by the budget hysteresis)
  } else {
    if (*use_multilevel == -2) p->auto_decided = false;  // back to the decision a fresh handle takes for this problem
    p->auto_decide();
  }
  *use_multilevel = p->auto_ml ? 1 : 0;
  return DPGO_OK;
}


int dpgo_problem_auto_info(dpgo_problem_t p, int* state, long long* jacobi_units, int* reference_products, int* switches,
                           int* backoff, int* units_jacobi, int* units_additive) {
  if (!p) return fail(DPGO_ERR_INVALID, "null handle");
  const auto& a = p->auto_cost;
  if (units_jacobi) *units_jacobi = a.uj;
  if (units_additive) *units_additive = a.ua;
  if (state) *state = a.state;
  if (jacobi_units) *jacobi_units = a.jac_units;
  if (reference_products) *reference_products = a.ref;
  if (switches) *switches = a.switches;
  if (backoff) *backoff = a.backoff;
  return DPGO_OK;
}


int dpgo_auto_rule_constants(int* units_jacobi, int* units_additive, int* setup_units, int* min_products) {
  if (units_jacobi) *units_jacobi = kAutoUnitsJacobi;
  if (units_additive) *units_additive = kAutoUnitsAdditive;
  if (setup_units) *setup_units = kAutoSetupUnits;
  if (min_products) *min_products = kAutoMinProducts;
  return DPGO_OK;
}


int dpgo_optimize(dpgo_problem_t p, const dpgo_ropt_params* params, const double* X0, double* Xopt,
                  dpgo_ropt_result* result) {
  CHK(check_ready(p));
  if (!params || !X0 || !Xopt || !result) return fail(DPGO_ERR_INVALID, "null pointer");
  CHK(h2d(p, p->x1, X0));
  CHK(run_optimize(p, params, result));
  return d2h(p, Xopt, p->x1);
}


int dpgo_optimize_device(dpgo_problem_t p, const dpgo_ropt_params* params, double* X_dev, dpgo_ropt_result* result) {
  CHK(check_ready(p));
  if (!params || !X_dev || !result) return fail(DPGO_ERR_INVALID, "null pointer");
  if (!aligned8(X_dev)) return fail(DPGO_ERR_INVALID, "X_dev not 8-byte aligned");
  BorrowedIterate x;
  CHK(x.begin(p, X_dev));
  CHK(x.end(p, run_optimize(p, params, result)));
  HIPC(hipStreamSynchronize(p->stream));
  return DPGO_OK;
}


int dpgo_warning_count(void) { return g_warnings.load(); }

// Enqueue only: a one-launch solve is left in flight with its commit kernel (pd.launched; dpgo_optimize_device_end collects
// it), any other solve runs to completion right here, into pd.result.
static int begin_solve(dpgo_problem_s* p, const dpgo_ropt_params* prm, dpgo_problem_s::Pending& pd) {
  CHK(plan_solve(p, prm, &pd.plan));
  if (pd.plan.one_launch) CHK(one_launch_enqueue(p, pd.plan, &pd.launched));
  return pd.launched ? DPGO_OK : multi_launch_solve(p, pd.plan, &pd.result);
}

int dpgo_optimize_device_begin(dpgo_problem_t p, const dpgo_ropt_params* params, double* X_dev,
                               const double* nbr_tiles_dev) {
  CHK(check_ready(p));
  if (!params || !X_dev) return fail(DPGO_ERR_INVALID, "null pointer");
  if (!aligned8(X_dev)) return fail(DPGO_ERR_INVALID, "X_dev not 8-byte aligned");
  if (p->pending.active) return fail(DPGO_ERR_STATE, "a solve of this handle is already in flight (dpgo_optimize_device_end)");
  if (nbr_tiles_dev) CHK(refresh_G(p, nbr_tiles_dev));  // (first, on the same stream)
  auto& pd = p->pending;
  pd = dpgo_problem_s::Pending();
  CHK(pd.x.begin(p, X_dev));
  p->persist_stream_ordered = true;
  const int rc = begin_solve(p, params, pd);
  p->persist_stream_ordered = false;
  if (rc != DPGO_OK || !pd.launched) {  // failed, or the solve is not a one-launch solve and has run to completion
    CHK(pd.x.end(p, rc));
    if (pd.x.staged) HIPC(hipStreamSynchronize(p->stream));
  }
  pd.active = true;
  return DPGO_OK;
}


int dpgo_optimize_device_end(dpgo_problem_t p, dpgo_ropt_result* result) {
  if (!p || !result) return fail(DPGO_ERR_INVALID, "null pointer");
  CHK(set_device(p));
  auto& pd = p->pending;
  if (!pd.active) return fail(DPGO_ERR_STATE, "no solve in flight (dpgo_optimize_device_begin)");
  pd.active = false;
  if (!pd.launched) {
    *result = pd.result;
    return DPGO_OK;
  }
  pd.launched = false;
  bool ok = false;
  int rc = one_launch_collect(p, pd.plan, result, &ok);
  if (rc == DPGO_OK && !ok) rc = multi_launch_solve(p, pd.plan, result);  // (after a time-out, as the synchronous call)
  // (no resident slots to release: launch_rtr_persistent reserves none for a stream-ordered solve, and none were held going in)
  CHK(pd.x.end(p, rc));
  HIPC(hipStreamSynchronize(p->stream));
  return DPGO_OK;
}


// ---- several agents of one process updated concurrently (same-colour agents of a parallel RBCD sweep) ----
namespace {
// Host threads that feed the just-in-time tCG loops of several handles at once: one worker per concurrently solved handle,
// created on first use and kept (a solve is a few milliseconds; creating threads per sweep would show).
class FeedPool {
 public:
  static FeedPool& get() {
    static FeedPool* pool = new FeedPool();  // never destroyed: workers may outlive static destructors
    return *pool;
  }
  // runs job(0..count-1): job(0) on the calling thread, the others on workers; returns when all are done
  void run(int count, const std::function<void(int)>& job) {
    std::unique_lock<std::mutex> call(call_mu_);  // one batch at a time
    {
      std::lock_guard<std::mutex> lk(mu_);
      while ((int)workers_.size() < count - 1) {
        const int id = (int)workers_.size();
        workers_.emplace_back([this, id] { loop(id); });
        workers_.back().detach();
      }
      job_ = &job;
      count_ = count;
      pending_ = count - 1;
      epoch_ += 1;
    }
    cv_.notify_all();
    job(0);
    std::unique_lock<std::mutex> lk(mu_);
    done_.wait(lk, [this] { return pending_ == 0; });
    job_ = nullptr;
  }

 private:
  void loop(int id) {
    unsigned long long seen = 0;
    while (true) {
      const std::function<void(int)>* job = nullptr;
      {
        std::unique_lock<std::mutex> lk(mu_);
        cv_.wait(lk, [&] { return epoch_ != seen; });
        seen = epoch_;
        if (id + 1 < count_) job = job_;
      }
      if (job) {
        (*job)(id + 1);
        std::lock_guard<std::mutex> lk(mu_);
        if (--pending_ == 0) done_.notify_all();
      }
    }
  }
  std::mutex call_mu_, mu_;
  std::condition_variable cv_, done_;
  std::vector<std::thread> workers_;
  const std::function<void(int)>* job_ = nullptr;
  int count_ = 0, pending_ = 0;
  unsigned long long epoch_ = 0;
};

// Runs body(k) for every handle on its OWN stream, ordered after `after_stream`; the handles' previous streams are
// restored afterwards.  Returns the first failure (its message becomes this thread's dpgo_last_error).
static int run_many(int count, const dpgo_problem_t* handles, void* after_stream, const std::function<int(int)>& body) {
  if (count <= 0) return DPGO_OK;
  if (!handles) return fail(DPGO_ERR_INVALID, "null handle array");
  for (int k = 0; k < count; ++k) {
    CHK(check_ready(handles[k]));
    if (handles[k]->device != handles[0]->device) return fail(DPGO_ERR_INVALID, "handles on different devices");
    for (int q = 0; q < k; ++q)
      if (handles[q] == handles[k]) return fail(DPGO_ERR_INVALID, "a handle appears twice");
  }
  {  // ROCm maps a process's HIP streams onto 4 hardware queues by default: more concurrently solved handles than that
     // still complete, but queue behind each other -- say so once instead of silently serialising
    static std::atomic<bool> warned{false};
    const int queues = 4;
    if (count > queues && !warned.exchange(true)) {
      g_warnings.fetch_add(1);
      std::fprintf(stderr,
                   "dpgo_hip: warning: %d handles are solved concurrently but the HIP runtime maps their streams onto %d "
                   "hardware queues: they partly serialise\n",
                   count, queues);
    }
  }
  std::vector<hipStream_t> prev(count);
  for (int k = 0; k < count; ++k) prev[k] = handles[k]->stream;  // (all of them first: restored below whatever fails)
  hipEvent_t ev = nullptr;
  HIPC(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, (hipStream_t)after_stream);
  for (int k = 0; k < count && e == hipSuccess; ++k) {
    if (prev[k] != handles[k]->own_stream) e = hipStreamSynchronize(prev[k]);  // earlier work of the handle itself
    handles[k]->stream = handles[k]->own_stream;
    handles[k]->persist_share = count;  // persistent tCG launches: prefer the layout with the fewest resident slots
    if (e == hipSuccess) e = hipStreamWaitEvent(handles[k]->own_stream, ev, 0);
  }
  std::vector<int> rc(count, DPGO_OK);
  std::vector<std::string> msg(count);
  if (e == hipSuccess) {
    FeedPool::get().run(count, [&](int k) {
      int r = (hipSetDevice(handles[k]->device) == hipSuccess) ? body(k) : fail(DPGO_ERR_HIP, "hipSetDevice failed");
      if (r == DPGO_OK && hipStreamSynchronize(handles[k]->stream) != hipSuccess)
        r = fail(DPGO_ERR_HIP, "hipStreamSynchronize failed");
      rc[k] = r;
      if (r != DPGO_OK) msg[k] = g_err;  // thread-local message of the worker
    });
  }
  for (int k = 0; k < count; ++k) {
    handles[k]->stream = prev[k];
    handles[k]->persist_share = 1;
  }
  (void)hipEventDestroy(ev);
  if (e != hipSuccess) return fail(DPGO_ERR_HIP, std::string("stream ordering of the concurrent update: ") + hipGetErrorString(e));
  for (int k = 0; k < count; ++k)
    if (rc[k] != DPGO_OK) return fail(rc[k], "handle " + std::to_string(k) + ": " + msg[k]);
  return DPGO_OK;
}
}  // namespace


int dpgo_optimize_device_many(int count, const dpgo_problem_t* handles, const dpgo_ropt_params* params,
                              double* const* X_dev, const double* const* nbr_tiles_dev, void* after_stream,
                              dpgo_ropt_result* results) {
  if (count <= 0) return DPGO_OK;
  if (!params || !X_dev || !results) return fail(DPGO_ERR_INVALID, "null pointer");
  for (int k = 0; k < count; ++k) {
    if (!X_dev[k]) return fail(DPGO_ERR_INVALID, "null iterate");
    if (!aligned8(X_dev[k])) return fail(DPGO_ERR_INVALID, "iterate not 8-byte aligned");
  }
  return run_many(count, handles, after_stream, [&](int k) -> int {
    dpgo_problem_s* p = handles[k];
    if (nbr_tiles_dev && nbr_tiles_dev[k]) CHK(refresh_G(p, nbr_tiles_dev[k]));
    BorrowedIterate x;
    CHK(x.begin(p, X_dev[k]));
    return x.end(p, run_optimize(p, params, &results[k]));
  });
}


int dpgo_problem_eval_terms_device_many(int count, const dpgo_problem_t* handles, const double* const* X_dev,
                                        const double* const* nbr_tiles_dev, void* after_stream, double* terms) {
  if (count <= 0) return DPGO_OK;
  if (!X_dev || !terms) return fail(DPGO_ERR_INVALID, "null pointer");
  for (int k = 0; k < count; ++k)
    if (!X_dev[k]) return fail(DPGO_ERR_INVALID, "null iterate");
  return run_many(count, handles, after_stream, [&](int k) -> int {
    dpgo_problem_s* p = handles[k];
    if (nbr_tiles_dev && nbr_tiles_dev[k]) CHK(refresh_G(p, nbr_tiles_dev[k]));
    CHK(eval_state(p, X_dev[k]));
    terms[3 * k + 0] = p->hstate->xqx;
    terms[3 * k + 1] = p->hstate->xg;
    terms[3 * k + 2] = p->hstate->ngf * p->hstate->ngf;
    return DPGO_OK;
  });
}


#ifdef DPGO_TIMELINE
int dpgo_debug_timeline(long long* out /* [2][16] */) {
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_timeline), sizeof(long long) * 32));
  return DPGO_OK;
}
int dpgo_debug_timeline_tiles(long long* out /* [3][64] */) {
  HIPC(hipDeviceSynchronize());
  HIPC(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_tl_tiles), sizeof(long long) * 3 * 64));
  return DPGO_OK;
}
#endif


int dpgo_problem_persistent_info(dpgo_problem_t p, int* enabled, int* workgroups, int* last_members, int* last_iterations,
                                 int* last_layout) {
  if (!p) return fail(DPGO_ERR_INVALID, "null handle");
  if (enabled) *enabled = (p->persist && !p->persist_failed_once) ? 1 : 0;
  if (workgroups) *workgroups = p->persist_wgs;
  if (last_members) *last_members = p->hctrl ? (int)p->hctrl->members : 0;
  if (last_iterations) *last_iterations = p->hctrl ? (int)p->hctrl->iters : 0;
  if (last_layout) *last_layout = (p->hctrl && p->hctrl->members) ? p->persist_split * 16 + p->persist_mt : 0;
  return DPGO_OK;
}


int dpgo_problem_persistent_phases(dpgo_problem_t p, double us_per_iteration[4], int* iterations) {
  if (!p || !us_per_iteration) return fail(DPGO_ERR_INVALID, "null handle / pointer");
  const double it = p->hctrl ? (double)p->hctrl->ticks[4] : 0.0;
  for (int k = 0; k < 4; ++k)  // (100 MHz wall-clock ticks of participant 0, summed over the iterations after the first)
    us_per_iteration[k] = (p->hctrl && it > 0.0 && p->hctrl->members) ? 0.01 * (double)p->hctrl->ticks[k] / it : 0.0;
  if (iterations) *iterations = (p->hctrl && p->hctrl->members) ? (int)p->hctrl->iters : 0;
  return DPGO_OK;
}


int dpgo_problem_feed_counters(dpgo_problem_t p, long long counts[4]) {
  if (!p || !counts) return fail(DPGO_ERR_INVALID, "null handle / pointer");
  counts[0] = p->feed.steps;
  counts[1] = p->feed.runs;
  counts[2] = p->feed.runs_fed;
  counts[3] = p->feed.products;
  return DPGO_OK;
}


int dpgo_problem_set_persistent(dpgo_problem_t p, int enable) {
  if (!p) return fail(DPGO_ERR_INVALID, "null handle");
  if (enable && persist_geometry(p, persist_capacity(p->device)).wgs <= 0)
    return fail(DPGO_ERR_UNSUPPORTED, "block too large for the persistent tCG kernel (at most 2 tiles on each of 256 workgroups)");
  p->persist = enable != 0;
  if (enable) p->persist_failed_once = false;
  return DPGO_OK;
}


int dpgo_problem_tcg_kernel_info(dpgo_problem_t p, int* symmetric, int* split, int* stream_nt) {
  CHK(check_ready(p));
  CHK(resolve_tcg_storage(p));
  if (symmetric) *symmetric = p->tcg_sym ? 1 : 0;
  if (split) *split = p->tcg_sym ? 1 : p->split;
  if (stream_nt) *stream_nt = (p->stream_nt && (p->tcg_sym || p->split == 1)) ? 1 : 0;
  return DPGO_OK;
}


int dpgo_problem_tcg_directions_info(dpgo_problem_t p, int* deferred, int* slots) {
  if (!p) return fail(DPGO_ERR_INVALID, "null handle");
  if (deferred) *deferred = p->dirs_on ? 1 : 0;
  if (slots) *slots = p->dirs ? p->dirs_cap : 0;
  return DPGO_OK;
}

}  // extern "C"
