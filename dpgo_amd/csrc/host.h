// host.h -- what the translation units of libdpgo_hip.so share: error reporting, the typed helpers that choose a kernel
// instance (dispatch_dr, dispatch_split, dispatch_drs) and launch it (launch), the tile count of a pose grid (pose_tiles), the problem
// handle (struct dpgo_problem_s: device buffers, hierarchy, solver state of one PoseGraph) and the declarations of the
// host-side helpers each unit defines.
//   problem.hip     handle lifecycle, Q / G upload, symmetric storage, QuadraticProblem evaluations (k_spmm, k_grad, k_hess ...)
//   multilevel.hip  hierarchy set-up (symbolic on the host, numeric on the device) and the V-cycle's launches
//   solve.hip       QuadraticOptimizer::optimize: tCG launches, the one-launch solve, RTR outer loop, preconditioner
//                   selection (DPGO_PRECOND_AUTO), concurrent / begin-end solves
//   agents.hip      GNC re-weighting, initial guesses, manifold operations, public-pose exchange plans
//   align.hip       frame alignment of agents that start in their own frames: candidates, robust average, lift
//   bench_probes.hip  kernel timing probes used by bench.py
//   certify.hip     certificate of global optimality (LOBPCG on C(X) = Q - Lambda(X)) and the staircase escape
// Host compiler only, no HIP (each has a stand-alone test program under tests/cxx or is included by one):
//   handoff.h        the partial-sum regions and the state slots one launch leaves for the next
//   options.h        the DPGO_* switches: one table, read from the environment once
//   taskpool.h       the set-up code's worker threads (TaskPool), setup_threads, parallel_ranges, pattern_by_ranges
//   aggregation.h / aggregation.cpp  the hierarchy's set-up over index vectors: aggregates (growth, merge, index runs),
//                    block patterns of A P and of the next level, run / tile / chunk tables, the additive layout's search
//   cert_dense.h / cert_dense.cpp    the certificate's host algebra on the r x r Gram blocks: small factorizations, block
//                    assembly, the coefficient matrices and decisions of every step of the eigen-solver
#pragma once
#include "kernels.h"
#include "handoff.h"
#include "options.h"
#include "taskpool.h"
#include "aggregation.h"
#include "cert_dense.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <memory>
#include <pthread.h>
#include <sched.h>
#include <mutex>
#include <thread>
#include <type_traits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../include/dpgo_hip.h"

using namespace dpgo;

namespace dpgo_host {


inline thread_local std::string g_err;

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIPC(expr)                                                                              \
  do {                                                                                          \
    hipError_t e_ = (expr);                                                                     \
    if (e_ != hipSuccess)                                                                       \
      return fail(DPGO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_) + " (" + __FILE__ + \
                                    ":" + std::to_string(__LINE__) + ")");                      \
  } while (0)

#define CHK(expr)                \
  do {                           \
    int rc_ = (expr);            \
    if (rc_ != DPGO_OK) return rc_; \
  } while (0)

// (d, r) pairs with compiled kernels
#define DPGO_FOR_DR(M) M(2, 2) M(2, 3) M(2, 4) M(2, 5) M(3, 3) M(3, 4) M(3, 5) M(3, 6)

inline bool supported(int d, int r) {
#define M(dd, rr) \
  if (d == dd && r == rr) return true;
  DPGO_FOR_DR(M)
#undef M
  return false;
}

// ---- choosing and launching a kernel instance ----
// Run-time values that select a template instance reach the code as types: Int<V> for a number, a value of the type
// itself (float{}, double{}) for a storage type.  A dispatch_* helper calls a generic lambda with them and returns what the
// lambda returns (a DPGO_* code); the call of the lambda is always inlined, so a launch function compiles to the straight
// code a switch would give.  An Int<V> converts to its number at compile time, so a lambda that takes
// (auto D, auto R) writes k_retract<D, R>; only a lambda NESTED in it cannot (it would capture D by reference): a body that
// nests takes (auto Dc, auto Rc) and starts with
//   constexpr int D = decltype(Dc)::value, R = decltype(Rc)::value;
template <int V>
using Int = std::integral_constant<int, V>;

// f(Int<D>{}, Int<R>{}) for the pair of DPGO_FOR_DR that equals (d, r)
template <class F>
__attribute__((always_inline)) inline int dispatch_dr(int d, int r, F&& f) {
#define M(dd, rr) \
  if (d == dd && r == rr) [[clang::always_inline]] return f(Int<dd>{}, Int<rr>{});
  DPGO_FOR_DR(M)
#undef M
  return fail(DPGO_ERR_UNSUPPORTED, "unsupported (d, r)");
}
// f(Int<SPLIT>{}) for the lane groups per pose of a <D, R, SPLIT> kernel: 4, 2, anything else is 1
template <class F>
__attribute__((always_inline)) inline int dispatch_split(int split, F&& f) {
  [[clang::always_inline]] return split == 4 ? f(Int<4>{}) : split == 2 ? f(Int<2>{}) : f(Int<1>{});
}

// both at once: f(Int<D>{}, Int<R>{}, Int<SPLIT>{})
template <class F>
__attribute__((always_inline)) inline int dispatch_drs(int d, int r, int split, F&& f) {
  return dispatch_dr(d, r, [&](auto D, auto R) { return dispatch_split(split, [&](auto S) { return f(D, R, S); }); });
}

// The one place a kernel is launched.  The parameter types are the kernel's own and every argument is converted to its
// parameter's type here: nullptr needs no cast, a DevBuf<T> no .get(), and an argument of the wrong type or a wrong number
// of them is an error at the call.  Workgroups of kBlock threads unless launch_wg says otherwise.  Nothing is checked
// at run time: the launch function's HIPC(hipGetLastError()) does that once for all its launches, and the DPGO_OK returned
// only lets a selector's lambda end in `return launch(...)`.
template <class... KArgs, class... Args>
inline int launch_wg(void (*kernel)(KArgs...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, Args&&... args) {
  static_assert(sizeof...(KArgs) == sizeof...(Args), "launch: as many arguments as the kernel has parameters");
  hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, static_cast<KArgs>(std::forward<Args>(args))...);
  return DPGO_OK;
}
template <class... KArgs, class... Args>
inline int launch(void (*kernel)(KArgs...), dim3 grid, size_t lds_bytes, hipStream_t stream, Args&&... args) {
  return launch_wg(kernel, grid, dim3(kBlock), lds_bytes, stream, std::forward<Args>(args)...);
}

// workgroups that hold n poses at (64 / (b * split)) * kWaves poses each (b = d + 1 lanes per lane group), at least one
inline int pose_tiles(int n, int b, int split = 1) {
  const int P = (64 / (b * split)) * kWaves;
  return std::max(1, (n + P - 1) / P);
}

// Caller pointers (include/dpgo_hip.h, "Alignment"): any 8-byte-aligned address is valid; the kernels that move own-tile
// spans in 16-byte pieces (dbl2, span_from_lds) run on 16-byte-aligned buffers only
inline bool aligned8(const void* q) { return ((uintptr_t)q & 7) == 0; }
inline bool aligned16(const void* q) { return ((uintptr_t)q & 15) == 0; }

// ---- the library's own device and pinned memory ----
// Every buffer the library keeps is a DevBuf (hipMalloc) or a PinBuf (hipHostMalloc): move-only, released by the destructor,
// so a struct that gains a buffer needs no second edit anywhere and an early return leaks nothing.  Assigning an empty value
// releases (`S = SymQ()`); the conversion to T* lets code that only reads the pointer -- launch arguments, `p->dirs + slot`,
// `if (!p->Q.vals)` -- look as it did with raw pointers.  These two types are the only callers of hipMalloc / hipFree /
// hipHostMalloc / hipHostFree (dpgo_device_malloc / dpgo_device_free hand memory to the caller and are not counted).
// g_live_*: what all of them hold at the moment (dpgo_debug_live_allocations).
inline std::atomic<long long> g_live_buffers{0}, g_live_bytes{0};

template <class T, bool kPinned>
class OwnedBuf {
 public:
  OwnedBuf() = default;
  OwnedBuf(OwnedBuf&& o) noexcept : p_(std::exchange(o.p_, nullptr)), bytes_(std::exchange(o.bytes_, 0)) {}
  OwnedBuf& operator=(OwnedBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      bytes_ = std::exchange(o.bytes_, 0);
    }
    return *this;
  }
  ~OwnedBuf() { reset(); }
  // `count` elements (flags: hipHostMalloc's, pinned memory only); what the buffer held before is released first
  int alloc(size_t count, unsigned flags = hipHostMallocDefault) {
    reset();
    const size_t bytes = sizeof(T) * count;
    if constexpr (kPinned)
      HIPC(hipHostMalloc(&p_, bytes, flags));
    else
      HIPC(hipMalloc(&p_, bytes));
    if (!p_) return DPGO_OK;  // (a request for zero bytes)
    bytes_ = bytes;
    g_live_buffers.fetch_add(1, std::memory_order_relaxed);
    g_live_bytes.fetch_add((long long)bytes, std::memory_order_relaxed);
    return DPGO_OK;
  }
  void reset() {
    if (!p_) return;
    if constexpr (kPinned)
      (void)hipHostFree(p_);
    else
      (void)hipFree(p_);
    g_live_buffers.fetch_sub(1, std::memory_order_relaxed);
    g_live_bytes.fetch_sub((long long)bytes_, std::memory_order_relaxed);
    p_ = nullptr;
    bytes_ = 0;
  }
  T* get() const { return p_; }
  operator T*() const { return p_; }
  T* operator->() const { return p_; }

 private:
  T* p_ = nullptr;
  size_t bytes_ = 0;
};
template <class T>
using DevBuf = OwnedBuf<T, false>;
template <class T>
using PinBuf = OwnedBuf<T, true>;

// at least one element (an empty edge list, an empty block row); copies `count` of them on `s`
template <class T>
inline int upload(DevBuf<T>& dst, const T* src, size_t count, hipStream_t s) {
  CHK(dst.alloc(count > 0 ? count : 1));
  if (count > 0) HIPC(hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyHostToDevice, s));
  return DPGO_OK;
}

// the handle's own stream: declared in front of the buffers, so destroyed after them
struct OwnedStream {
  hipStream_t s = nullptr;
  OwnedStream() = default;
  OwnedStream(const OwnedStream&) = delete;
  OwnedStream& operator=(const OwnedStream&) = delete;
  ~OwnedStream() {
    if (s) (void)hipStreamDestroy(s);
  }
  operator hipStream_t() const { return s; }
};

struct Bsr {
  int nrows = 0, ncols = 0, nnzb = 0;
  DevBuf<int32_t> rowptr, colidx;
  DevBuf<double> vals;
  BsrDev dev() const { return BsrDev{rowptr, colidx, vals}; }
};

// What a solve has decided before its first launch (plan_solve, solve.hip): kept by a begin / end solve between the calls.
struct SolvePlan {
  dpgo_ropt_params prm{};  // the caller's, DPGO_PRECOND_AUTO resolved to what the handle currently runs
  bool is_auto = false;    // (the caller asked for DPGO_PRECOND_AUTO: the solve reports to auto_update)
  const double* dinv = nullptr;  // borrowed: the handle's block-Jacobi factors, or none
  std::chrono::steady_clock::time_point t0;
  bool one_launch = false;  // eligible for the one-launch solve (k_rtr_persist)
};

// The caller's device iterate as the handle's x1 for the duration of a solve (solve.hip).  Borrows, owns nothing.
struct BorrowedIterate {
  double* own_x1 = nullptr;  // the handle's x1, put back by end()
  double* staged = nullptr;  // the caller's iterate when it is not 16-byte aligned: the solve runs on own_x1
  int begin(dpgo_problem_s* p, double* X_dev);
  int end(dpgo_problem_s* p, int rc);  // rc: what the solve returned; copies out after a successful solve only
};

// The handle's partial-sum regions (handoff.h; DESIGN.md section 4 says who writes and who reads each).  sums_out: for the
// launch that writes R on `grid` workgroups; sums_ready: in front of a launch whose kernel sums R.
using Partials = PartialRegion<kPartialCap>;
inline int sums_out(Partials& R, int grid, double** ptr) {
  *ptr = R.out(grid);
  return *ptr ? DPGO_OK : fail(DPGO_ERR_STATE, "partial sums: the writing launch's grid is outside 1 .. kPartialCap");
}
inline int sums_ready(const Partials& R) {
  return R.is_written() ? DPGO_OK : fail(DPGO_ERR_STATE, "partial sums: read before any launch of this handle wrote them");
}

}  // namespace dpgo_host
using namespace dpgo_host;

struct dpgo_problem_s {
  int r = 0, d = 0, n = 0, b = 0, T = 0;
  int device = 0;
  OwnedStream own_stream;  // (first: the buffers below are released before the stream is destroyed)
  hipStream_t stream = nullptr;
  Bsr Q;
  Bsr C;  // inter-agent coupling (rectangular), for G
  DevBuf<double> G0, G;
  bool has_G = false;
  bool g0_nonzero = false;  // the constant term G0 of the coupling holds a non-zero entry (priors)
  DevBuf<double> dinv;
  double dinv_shift = -1.0;
  // work vectors
  DevBuf<double> x1_buf, x2, g1, g2, eta, delta, Hd, rr, z, S1, S2;
  // the iterate the kernels run on: x1_buf, or -- borrowed for the duration of a device solve -- the caller's buffer
  double* x1 = nullptr;
  // tCG's kept directions (kernels/tcg.h, DEF): a ring of dirs_cap pose vectors and the step lengths that go with them
  // (dirs_coef: count, then one per slot).  Allocated by the first multi-launch RTR solve that runs deferred, grown when a
  // later solve has a larger tCG budget (tcg_dirs_ensure).  dirs_on: the mode of the current / last such solve, decided
  // once per solve on the host; every launch of the solve follows it.
  DevBuf<double> dirs, dirs_coef;
  int dirs_cap = 0;
  bool dirs_on = false;
  // multilevel (aggregation multigrid) preconditioner: levels[0] = the pose level ... levels.back() = the dense level
  struct MlLevel {
    int n = 0;      // nodes
    int k = 0;      // aggregate size towards the next level (0 on the dense level)
    int split = 1;  // lane groups per node of this level's SpMM-family kernels
    Bsr A;          // level >= 1: Galerkin operator (level 0: Q + shift I, never formed)
    DevBuf<int32_t> slot_row;  // level >= 1: block row of every slot of A
    DevBuf<double> dinv, Pb;  // smoother factors; prolongation blocks towards level + 1
    DevBuf<double> r, x1, x;  // restricted residual, pre-smoothed iterate, corrected iterate
    // level 0 of a two-level hierarchy: AP = (Q + shift I) P (block rows = poses, block columns = level-1 nodes) and the
    // residual after pre-smoothing, so that the post-smoothing kernel gathers from the SMALL coarse vector:
    // r - A (x1 + P xc) = (r - A x1) - (A P) xc
    Bsr AP;
    DevBuf<double> res1;
    // level 0 of a two-level hierarchy with GRAPH aggregates (grow_aggregates, aggregation.h): label of every pose, members of every
    // aggregate in discovery order, the spanning tree the prolongation is composed along, P_i^T res_i of every pose
    bool graph = false;
    DevBuf<int32_t> lab, agg_ptr, agg_mem, parent, pslot;
    DevBuf<int32_t> mem_pos;  // position of every pose in agg_mem (k_ml_build_P_tree_wave)
    // restriction of graph aggregates: inside the G consecutive poses a wave of k_ml_restrict owns, every RUN of poses with
    // the same aggregate is added up in the wave and leaves ONE partial sum; seg_info[i] = slot * 32 + length for the first
    // pose of a run (-1 otherwise), slots ordered by aggregate, seg_ptr[a] .. seg_ptr[a+1] = the partial sums of aggregate a
    DevBuf<int32_t> seg_info, seg_ptr;
    int nseg = 0;  // partial sums per restriction
    DevBuf<int32_t> tile_perm;  // aggregates of at most one persistent tile: pose of every (aggregate, slot), -1 = empty
    int perm_tile = 0;             // slots per aggregate in tile_perm
    int merge_cap = 0;             // graph aggregates: fragments merged up to this many poses (0: plain greedy growth)
    DevBuf<double> tbuf;
    DevBuf<float> Pb32, AP32;  // fp32 copies of Pb and of A P's values (level 0, ml_operator_bits == 32)
    DevBuf<float> x1f, res1f;  // ... and the cycle-internal vectors of level 0 in that storage: the
                                             // pre-smoothed iterate (k_tcg_update -> k_ml_restrict), the kept residual
                                             // (k_ml_restrict -> k_ml_post_ap)
    AggMap agg() const { return AggMap{graph ? lab : nullptr, k}; }
  };
  std::vector<MlLevel> ml;
  Pattern h_pattern;  // host copy of Q's block pattern (symbolic setup of the hierarchy)
  bool has_pattern() const { return h_pattern.n() == n; }
  bool ml_symbolic = false, ml_ready = false, ml_user_ks = false;
  bool ml_additive_layout = false;  // the hierarchy is the one the additive preconditioner needs (one aggregate per workgroup tile)
  // layout of the additive preconditioner's one-launch solve for this block pattern (additive_plan): lane groups per pose
  // (0: the block does not fit), slots per workgroup tile = aggregate, growth size and merge bound of the graph aggregates
  // (graph = false: index runs of `tile` poses), number of aggregates = workgroups
  struct AddPlan {
    int split = 0, tile = 0, S = 0, cap = 0, na = 0;
    bool graph = true;
  } add_plan;
  bool add_plan_known = false;
  // workgroup tiles one aggregate of the additive layout may take: 1, or 2 for blocks no one-tile plan holds
  // (dpgo_problem_additive_tiles; 0 = DPGO_ADDITIVE_TILES)
  int add_tiles = 0;
  // the aggregation the plan was found with (host arrays), reused by the symbolic setup that follows: growing and merging
  // the aggregates of a 12 500-pose block is 1.4 ms of host time
  struct AggCache {
    Aggregates agg;
    int S = 0, cap = 0;
  } add_agg;
  double ml_omega = 0.7, ml_shift = 1e-1;
  // the dense level of the hierarchy: what lives and dies with it (ml_free assigns an empty one)
  struct DenseLevel {
    DevBuf<double> inv;   // inverse of the coarsest operator, row-major, leading dimension lda
    DevBuf<float> inv32;  // its fp32 storage (what the cycle streams when ml_coarse_bits == 32)
    // lower block triangle of the (exactly symmetric) inverse, packed 64 x 64 tiles: what a two-level cycle streams in 64-bit
    // mode (k_dense_sym_apply: half the bytes); chunk table, partial-sum buffers
    DevBuf<double> packed, pd, pt;
    DevBuf<DenseChunk> chunks;
    DevBuf<int> chunk_first;
    int nchunks = 0;
    int lda = 0;
    DevBuf<double> W, Rx;  // Gauss-Jordan panels (setup only)
  } dense;
  bool ml_use_dense_sym() const {
    const int env = options().ml_dense_sym;
    if (!ml_use_ap() || ml_coarse_bits != 64 || !dense.packed || env == 0) return false;
    return env == 1 || dense.lda >= 3072;  // below, the row-streaming kernel (one launch, cache-resident inverse) is as fast
  }
  int ml_coarse_bits = 64;  // 32: opt-in (dpgo_problem_multilevel_coarse_bits)
  // Storage precision of the OPERATOR COPIES the V-cycle streams on level 0 of an HBM-bound block (symmetric storage, two
  // levels): Q's values in the restriction's residual r - A x1, the values of A P in the post-smoothing, the prolongation
  // blocks in both -- 32: fp32 copies beside the fp64 originals (the Hessian step, the set-up and every product and sum
  // stay fp64; the cycle is a preconditioner) -- and, with them, the two vectors that live INSIDE a cycle: the
  // pre-smoothed iterate x1 and the kept residual res1 (written once, read once per application).  DEFAULT since round 5 (100k poses: restriction 34.1 -> 29.2 us, post-smoothing
  // 25.7 -> 23.9 us, 152 -> 148 us per product, same product counts; 64 restores the fp64 originals).  ml_ops32_ready: the
  // copies hold the current values.
  int ml_operator_bits = 32;
  bool ml_ops32_ready = false;
  bool ml_ops32_suspend = false;  // set around a stand-alone application of the cycle (its pre-smoothing kernel writes fp64)
  bool ml_ops32_wanted() const { return ml_operator_bits == 32 && tcg_sym && split == 1 && ml_use_ap() && sym.uvalsT != nullptr; }
  bool ml_ops32_active() const { return !ml_ops32_suspend && ml_ops32_wanted() && ml_ops32_ready; }
  bool ml_vec32_active() const { return ml_ops32_active() && options().ml_vector_bits != 64; }  // (x1 / res1 in fp32 too)
  // the dense level (the inverse of the coarsest operator and the restricted residual it multiplies) streamed in fp32: by
  // request per handle (ml_coarse_bits == 32) or, with the rest of the cycle's fp32 storage, by DPGO_ML_DENSE_BITS=32 --
  // unless the level runs on the packed-triangle matrix-core kernels, which exist in fp64 only.  NOT the default: at 100k
  // poses the dense kernel itself gets faster (11.8 -> 9.3 us), the loop does not (136.0 against 135.6 us per product, three
  // interleaved pairs: the 19 MB it frees in the Infinity Cache change nothing the other kernels notice).
  bool coarse32_active() const {
    return ml_coarse_bits == 32 || (ml_vec32_active() && !ml_use_dense_sym() && options().ml_dense_bits == 32);
  }
  // DPGO_PRECOND_AUTO: the multilevel cycle is currently selected.  Decided afresh at the first "auto" use after every
  // change of Q (a function of the problem only, so repeated runs reproduce): multilevel for a block without coupling
  // to other agents -- there the tCG budget, not the trust-region boundary, ends the local solves --, block-Jacobi
  // for a block of a multi-agent problem; then hysteresis on the share of the tCG budget each solve used.
  bool auto_ml = false, auto_decided = false;
  // The cost rule of a COUPLED block the additive one-launch solve can hold (dpgo_hip.h, DPGO_PRECOND_AUTO): Q -- and with it
  // the hierarchy -- is constant across RBCD sweeps, so the set-up is paid once; everything is counted in units of a tenth of
  // a block-Jacobi product (kAutoUnits*), a function of the solves' product counts only, so that repeated runs reproduce.
  struct AutoCost {
    long long jac_units = 0;  // block-Jacobi work since Q last changed (or since the last hand-back)
    int ref = 0;              // products of the block-Jacobi solve the additive form is measured against
    int state = 0;            // 0 block-Jacobi, 1 additive on trial (its first solve), 2 additive
    int backoff = 0;          // hand-backs so far: the next trial waits for 2^backoff set-ups' worth of block-Jacobi work
    int switches = 0;         // block-Jacobi -> additive transitions since Q last changed
    int last_used = -1, last_products = 0;  // the last auto solve, as the rule saw it
    int uj = 10, ua = 18;     // unit costs of a block-Jacobi / an additive product the rule last used (auto_units_*)
  } auto_cost;
  void auto_decide() {
    if (!auto_decided) {
      auto_ml = !(has_G || C.nnzb > 0);
      auto_decided = true;
      auto_cost = AutoCost();
    }
  }
  // two-level hierarchies: level-0 post-smoothing through A P and the coarse solution (k_ml_post_ap); DPGO_ML_AP=0 disables
  bool ml_use_ap() const {
    const bool off = options().ml_ap == 0;
    return ml.size() == 2 && ml[0].AP.vals != nullptr && (!off || ml[0].graph);  // (graph aggregates exist in this form only)
  }
  // symmetric copy of Q for the plain SpMM on Infinity-Cache-cold blocks (k_spmm_sym): upper blocks transposed + lower references
  struct SymQ {
    int nu = 0, nl = 0;
    DevBuf<int32_t> urow, ucol, usrc, lrow, lcol, lslot, lsrc;
    DevBuf<double> uvalsT;
    DevBuf<float> uvalsT32;  // fp32 copy of the values (the cycle's level-0 restriction, ml_operator_bits == 32)
    DevBuf<int32_t> tord;  // walk over the workgroup tiles (BsrSymDevT::tord; NULL: index order)
    DevBuf<int> flag;  // device: set by k_sym_check when a lower block is not the transpose of its upper one
    bool symbolic = false;     // pattern arrays belong to the current block pattern
    bool pattern_ok = false;   // the pattern is structurally symmetric
    bool ready = false;        // uvalsT holds the current values and they passed the symmetry check
    bool values_ok = false;
    BsrSymDev dev() const { return BsrSymDev{urow, ucol, uvalsT, lrow, lcol, lslot, tord}; }
    BsrSymDev32 dev32() const { return BsrSymDev32{urow, ucol, uvalsT32, lrow, lcol, lslot, tord}; }
  } sym;
  int spmm_variant = DPGO_SPMM_AUTO;
  bool tcg_sym = false;  // the fused tCG-step kernel reads the symmetric copy (resolved before a solve / a kernel probe)
  int cap_hs = kMaxGrid; // launch cap of k_tcg_hess_sym
  bool sym_wanted() const {
    if (spmm_variant == DPGO_SPMM_PLAIN || split != 1) return false;
    if (spmm_variant == DPGO_SPMM_SYMMETRIC) return true;
    // AUTO: when the tCG loop's working set (Q and eight pose vectors) no longer fits the 256 MB Infinity Cache, i.e. when
    // Q's bytes come from HBM: there the half-size storage wins (k_tcg_hess 45.5 against 49.4 us, plain product 28.4 against
    // 36.6 us at 100k poses with cold operands), while on cache-resident operands the fused kernels gain nothing
    // (DESIGN.md section 3).  DPGO_SPMM_SYMMETRIC=0/1 in the environment overrides.
    if (options().spmm_symmetric >= 0) return options().spmm_symmetric != 0;
    return beyond_cache();
  }
  // what the tCG loop streams besides Q and the pose vectors (the multilevel cycle's dense inverse, A P, prolongation):
  // set by the solve that last chose a preconditioner
  size_t loop_extra_bytes = 0;
  // non-temporal single-use operands: when the launch is fed from HBM (same size rule as the symmetric storage)
  bool want_stream_nt() const {
    return options().stream_nt >= 0 ? options().stream_nt != 0 : beyond_cache();
  }
  bool beyond_cache() const {
    return sizeof(double) * ((size_t)Q.nnzb * b * b + 8 * (size_t)n * T) + sizeof(int32_t) * (size_t)Q.nnzb + loop_extra_bytes >
           ((size_t)256 << 20);
  }
  // persistent whole-chip tCG kernel (blocks in the latency regime, block-Jacobi / no preconditioner): kernels/persist.h
  bool persist = false;      // enabled for this handle (by size; DPGO_PERSIST=0/1, dpgo_problem_set_persistent)
  int persist_share = 1;     // agents solved concurrently on this device (> 1: the most compact layout is preferred)
  int persist_wgs = 0, persist_split = 0, persist_mt = 0;  // geometry of the current / last launch
  int persist_reserved = 0;  // resident-slot reservation held by the running solve
  bool persist_failed_once = false;
  bool stream_nt = false;  // single-use operands of the tCG-step kernel move non-temporally (ld_stream, common.h)
  bool persist_add = false;  // the reservation is for the additive-preconditioner variant
  bool persist_stream_ordered = false;  // set for the duration of a begin / end solve (see launch_rtr_persistent)
  // a solve enqueued by dpgo_optimize_device_begin and not yet collected by ..._end
  struct Pending {
    bool active = false;    // begin has been called
    bool launched = false;  // the one-launch solve is in flight (else: the solve already ran, `result` holds its outcome)
    SolvePlan plan;         // of the solve in flight: what one_launch_collect and a fallback after a time-out go by
    BorrowedIterate x;      // the caller's iterate, returned by the call that ends the solve
    dpgo_ropt_result result{};
  } pending;
  DevBuf<PersistCtrl> pctrl;
  bool pctrl_dirty = true;  // the control block has to be cleared in front of the next one-launch solve (creation, after a time-out)
  DevBuf<unsigned long long> pgran;  // granule table of the in-kernel all-reduce (kGranWords 8-byte words)
  unsigned gran_cleared_at = 0;         // value of `gen` when the table was last cleared
  PinBuf<PersistCtrl> hctrl;
  DevBuf<double> partial_mem;  // the four regions below, kPartialCap * kNP doubles each
  Partials pE, pA, pB, pH;
  DevBuf<DevState> state_mem;  // the two slots of `state`
  StateSlots<DevState> state;
  PinBuf<DevState> hstate;
  PinBuf<unsigned long long> hflag;  // host-coherent: host-coherent: device-published tCG progress word
  unsigned gen = 0;
  bool saw_rtr_stop = false;  // set from the progress word in just-in-time mode
  // what the last solve's tCG feed enqueued (dpgo_problem_feed_counters; host counts only): tCG steps (Hessian step + update
  // [+ cycle]) enqueued, tCG runs started, runs that were fed at least one step, Hessian-vector products executed
  struct FeedCounts {
    long long steps = 0, runs = 0, runs_fed = 0, products = 0;
  } feed;
  // re-weightable edges (GNC): registered, replaced and dropped together (assigning an empty one releases them)
  struct GncEdges {
    int em = 0;
    DevBuf<int32_t> e_p1, e_p2, c_ptr, c_edge;
    DevBuf<double> e_R, e_t, e_kappa, e_tau, e_w, e_rsq, q_base;
    DevBuf<uint8_t> e_fixed, c_kind, e_role;
    DevBuf<int32_t> e_slot;
    // contributions of shared re-weightable edges to the coupling matrix C
    DevBuf<int32_t> g_ptr, g_edge;
    DevBuf<uint8_t> g_kind;
    DevBuf<double> c_base;
    int n_shared_edges = 0;
    // k_edge_robust's per-workgroup records and k_edge_robust_finish's result (allocated by the first re-weighting)
    DevBuf<RobustPartial> r_partial;
    DevBuf<RobustStatsDev> r_stats;
    EdgeDev dev() const {
      return EdgeDev{e_p1, e_p2, e_R, e_t, e_kappa, e_tau, e_fixed, e_role, e_slot, e_w, e_rsq, em};
    }
  } gnc;
  size_t vec_bytes() const { return (size_t)n * T * sizeof(double); }
  int grid() const { return std::min(pose_tiles(n, b), cap_u); }
  int cap_u = kMaxGrid, cap_h = kMaxGrid;  // launch caps of the streaming / SpMM kernel families
  // k_tcg_update_span's multilevel-mode instance (no iterate, no projection: 143 VGPRs = 3 waves per SIMD) has its own cap
  int cap_u_ml = kMaxGrid;
  int grid_u(bool ml_mode) const { return std::min(pose_tiles(n, b), ml_mode ? cap_u_ml : cap_u); }
  int split = 1;  // lane groups per pose in the SpMM kernels (latency layout for small blocks)
  // SpMM kernels (k_spmm, k_grad, k_hess, k_tcg_hess)
  int grid_s() const { return std::min(pose_tiles(n, b, split), tcg_sym ? cap_hs : cap_h); }
  // level-0 restriction / post-smoothing of the multilevel cycle: their own resident-slot counts (lighter kernels than
  // k_tcg_hess: with 4 instead of 3 waves per SIMD the 1 563 tiles of the 100k block take 2 rounds instead of 3)
  int cap_restrict = kMaxGrid, cap_post = kMaxGrid;
  int grid_restrict() const { return std::min(pose_tiles(n, b, split), cap_restrict); }
  int grid_post() const { return std::min(pose_tiles(n, b, split), cap_post); }
  // the outer iteration's kernels on the symmetric storage (k_grad, k_hess: 110-114 VGPRs = 4 waves per SIMD) have their own
  // cap -- grid_s() is sized for the tCG-step kernel's 2 waves per SIMD
  int cap_outer_sym = kMaxGrid;
  int grid_outer_sym() const { return std::min(pose_tiles(n, b), cap_outer_sym); }
  int cap_spmm_sym = kMaxGrid;  // launch cap of k_spmm_sym (resident count of the compiled kernel)
  int grid_spmm_sym() const { return std::min(pose_tiles(n, b), cap_spmm_sym); }
  // plain k_spmm: no partial sums, higher occupancy than the fused tCG kernel
  int grid_spmm() const { return std::min(pose_tiles(n, b, split), kMaxGrid); }
  int grid_flat() const {  // elementwise kernels
    size_t total = (size_t)n * T;
    size_t g = (total + kBlock - 1) / kBlock;
    if (g < 1) g = 1;
    return g < (size_t)kMaxGrid ? (int)g : kMaxGrid;
  }
};

namespace dpgo_host {

struct Counters {
  int spmm = 0;
  bool vcycle_for_additive = false;  // an outer iteration of an "additive" solve ran the V-cycle instead
};

struct PersistGeo {
  int split = 0, mt = 0, wgs = 0, slots = 0;
};

// ---- problem.hip
int set_device(dpgo_problem_s* p);
int upload_bsr(Bsr& m, int nrows, int ncols, int nnzb, int b, const int32_t* rowptr, const int32_t* colidx,
               const double* vals, hipStream_t s);
int validate_bsr(int nrows, int ncols, int nnzb, const int32_t* rowptr, const int32_t* colidx, bool need_diag);
int build_dinv(dpgo_problem_s* p, double shift);
int poll_state(dpgo_problem_s* p);
int push_state(dpgo_problem_s* p);
void sym_free(dpgo_problem_s* p);
int launch_spmm_view(dpgo_problem_s* p, const BsrDev& M, const double* V, const double* Gadd, double* OUT, int rows, int g,
                     bool stream_nt = false);
int sym_symbolic_setup(dpgo_problem_s* p);
int sym_ensure(dpgo_problem_s* p, bool* usable);
int launch_spmm_sym(dpgo_problem_s* p, const BsrSymDev& M, const double* V, const double* Gadd, double* OUT);
int launch_spmm(dpgo_problem_s* p, const Bsr& M, const double* V, const double* Gadd, double* OUT, int nrows = -1,
                bool plain_only = false);
bool outer_sym_enabled();
int launch_grad(dpgo_problem_s* p, const double* X, double* RG, double* S, double* EG,
                const DevState* st = nullptr, bool sym = false);
int launch_hess(dpgo_problem_s* p, const double* X, const double* S, const double* V, const double* Gdot,
                double* HV, const DevState* st, int check_tcg, bool sym = false);
int launch_retract(dpgo_problem_s* p, const double* X, const double* eta, double scale, double* X2,
                   const DevState* st, const double* rho_r = nullptr, const double* rho_g = nullptr, bool from_dirs = false);
int launch_rtr_update(dpgo_problem_s* p);
int launch_precond(dpgo_problem_s* p, const double* X, const double* V, const double* dinv, double* Z);
int launch_rtr_begin(dpgo_problem_s* p, double tol, double Delta0, double Dmax, int max_inner, int tiny);
int eval_state(dpgo_problem_s* p, const double* X, double* S = nullptr, bool sym = false);
int refresh_G(dpgo_problem_s* p, const double* nbr_tiles);
int check_ready(dpgo_problem_s* p);
int h2d(dpgo_problem_s* p, double* dst, const double* src);
int d2h(dpgo_problem_s* p, double* dst, const double* src);

// ---- multilevel.hip
int ml_tile(int b, int split);
int additive_tile(const dpgo_problem_s* p);
int ml_level_split(int n);
int ml_default_graph_size(int n, int b);
std::vector<int> ml_default_ks(int n, int b, int split0);
void ml_free(dpgo_problem_s* p);
int ml_symbolic_setup(dpgo_problem_s* p, const std::vector<int>& ks_in, int perm_tile = 0);
int flat_grid(size_t items);
bool gj_use_mfma();
int dense_spd_inverse(hipStream_t s, double* M, int lda, double* W, double* Rx, bool mfma);
int ml_numeric_setup(dpgo_problem_s* p);
std::vector<int> ml_current_ks(const dpgo_problem_s* p);
const dpgo_problem_s::AddPlan& additive_plan(dpgo_problem_s* p);
int additive_split_of(const dpgo_problem_s* p);
int additive_tiles(const dpgo_problem_s* p);
int additive_mt_of(const dpgo_problem_s* p);
int ml_ensure(dpgo_problem_s* p, double shift, bool additive = false);
int ml_ops32_ensure(dpgo_problem_s* p);
int persist_capacity(int device);  // (two resident slots per CU; below)
int launch_coarse_prolong(dpgo_problem_s* p, const dpgo_problem_s::MlLevel& L, const dpgo_problem_s::MlLevel& C,
                          const DevState* gate, double* xc_out = nullptr);
int launch_dense_sym(dpgo_problem_s* p, const dpgo_problem_s::MlLevel& C, const DevState* gate);
int launch_ml_restrict0(dpgo_problem_s* p, const double* r, const DevState* gate, int g0, bool stop_check = false);
int launch_ml_post0(dpgo_problem_s* p, const double* Xdev, const double* r, double* z, Partials* sums, const DevState* gate);
int launch_ml_tail(dpgo_problem_s* p, const double* Xdev, const double* r, double* z, Partials* sums,
                   const DevState* gate, bool stop_check = false);
int launch_ml_apply(dpgo_problem_s* p, const double* Xdev, const double* v, double* z);

// ---- solve.hip
int launch_tcg_update(dpgo_problem_s* p, const double* dinv, int first, double* z_out = nullptr,
                      double ml_omega = 0.0);
int launch_tcg_hess(dpgo_problem_s* p, int first);
int launch_tcg_hess_with(dpgo_problem_s* p, const DevState* sin, DevState* sout, int first, unsigned long long* hflag,
                         unsigned gen);
int resolve_tcg_storage(dpgo_problem_s* p);
int tcg_dirs_ensure(dpgo_problem_s* p, int max_inner, bool may_alloc = true);
int persist_capacity(int device);
bool persist_reserve(dpgo_problem_s* p, int slots, int limit);
void persist_release(dpgo_problem_s* p);
bool additive_available(dpgo_problem_s* p);
PersistGeo persist_geometry(const dpgo_problem_s* p, int free_slots, int share = 1, bool additive = false);
bool additive_lds_fits(const dpgo_problem_s* p, int split, int mt, int na);
int launch_rtr_persistent(dpgo_problem_s* p, const dpgo_ropt_params* prm, const double* dinv, bool* used, bool additive);
void persist_report(dpgo_problem_s* p);
int rtr_outer_iteration(dpgo_problem_s* p, const dpgo_ropt_params* prm, const double* dinv, Counters& cnt,
                        bool poll_at_end);
int auto_units_jacobi(dpgo_problem_s* p);
int auto_units_additive(dpgo_problem_s* p);
void auto_update(dpgo_problem_s* p, const dpgo_ropt_params* prm, int used, int products);
int plan_solve(dpgo_problem_s* p, const dpgo_ropt_params* prm, SolvePlan* plan);
int one_launch_enqueue(dpgo_problem_s* p, const SolvePlan& plan, bool* used);
int one_launch_collect(dpgo_problem_s* p, const SolvePlan& plan, dpgo_ropt_result* res, bool* ok);
int multi_launch_solve(dpgo_problem_s* p, const SolvePlan& plan, dpgo_ropt_result* res);
int run_optimize(dpgo_problem_s* p, const dpgo_ropt_params* prm, dpgo_ropt_result* res);
int tune_launch_caps(dpgo_problem_s* p);
int tune_persist(dpgo_problem_s* p);

// ---- agents.hip
int rebuild_vals(dpgo_problem_s* p, int nnzb, const int32_t* cptr, const int32_t* cedge, const uint8_t* ckind,
                 const double* base, double sign, double* out);
int rebuild_Q_from_weights(dpgo_problem_s* p, const double* base, double sign, double* out);
int rebuild_C_from_weights(dpgo_problem_s* p, const double* base, double sign, double* out);
int refresh_after_weights(dpgo_problem_s* p);

}  // namespace dpgo_host
