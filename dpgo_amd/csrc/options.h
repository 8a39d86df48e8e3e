// options.h -- every tuning / A-B switch of the library in one table, read from the environment once.  Includes nothing
// from HIP: host.h includes it for the library, the host-only units (aggregation.cpp) and their stand-alone test programs
// include it directly.
#pragma once

#include <cstdlib>
#include <string>

namespace dpgo_host {

// Every tuning / A-B switch of the library in ONE place: read from the environment once (first use; dpgo_options_reload
// reads again), printed by dpgo_describe_options / dpgo_problem_describe.  -1 (or 0 where noted) = not set: the size rules
// decide.  The kernel-selecting ones are exercised by tests/test_parity_gpu.py::test_kernel_selecting_switches_*.
//        field              variable                  unset  meaning
#define DPGO_OPTIONS(X)                                                                                                  \
  X(split,             "DPGO_SPLIT",              0,  "lane groups per pose of the SpMM-family kernels: 1, 2, 4 (0: by size)")       \
  X(spmm_symmetric,    "DPGO_SPMM_SYMMETRIC",    -1,  "symmetric storage of Q for blocks beyond the Infinity Cache: 0 / 1")          \
  X(stream_nt,         "DPGO_STREAM_NT",         -1,  "non-temporal single-use operands in the tCG-step kernels: 0 / 1")             \
  X(outer_sym,         "DPGO_OUTER_SYM",          1,  "outer RTR iteration (k_grad / k_hess) reads the symmetric copy when tCG does") \
  X(rho_exact,         "DPGO_RHO_EXACT",          0,  "rho test from a fresh H eta (k_hess, one more pass over Q) instead of tCG's residual: reference path") \
  X(tcg_dirs,          "DPGO_TCG_DIRS",           1,  "multi-launch tCG keeps its directions and k_retract sums eta once (0: eta += alpha delta every iteration: reference path)") \
  X(tcg_dirs_max_mb,   "DPGO_TCG_DIRS_MAX_MB", 4096,  "largest direction ring (RTR_tCG_iterations pose vectors) a solve may hold; beyond it the solve runs the reference path") \
  X(update_pipe,       "DPGO_UPDATE_PIPE",        1,  "k_tcg_update_span requests its next tile behind the first per-piece loop (0: behind the tile's last store: reference order)") \
  X(tile_walk,         "DPGO_TILE_WALK",          1,  "symmetric-storage kernels walk each XCD's tiles breadth-first over the tile graph (0: index order)") \
  X(tcg_ahead,         "DPGO_TCG_AHEAD",          0,  "iterations the just-in-time feed stays ahead (0: 2 multilevel / 4 otherwise)") \
  X(grid_update,       "DPGO_GRID_UPDATE",        0,  "launch cap of k_tcg_update (0: resident count)")                              \
  X(grid_hess,         "DPGO_GRID_HESS",          0,  "launch cap of k_tcg_hess (0: resident count)")                                \
  X(grid_hess_sym,     "DPGO_GRID_HESS_SYM",      0,  "launch cap of k_tcg_hess_sym (0: resident count)")                            \
  X(grid_retract,      "DPGO_GRID_RETRACT",       0,  "launch cap of k_retract (0: 1024)")                                           \
  X(grid_outer_sym,    "DPGO_GRID_OUTER_SYM",     0,  "launch cap of k_grad / k_hess on the symmetric storage (0: resident count)")  \
  X(grid_spmm_sym,     "DPGO_GRID_SPMM_SYM",      0,  "launch cap of k_spmm_sym (0: resident count, at most 1024)")                  \
  X(grid_ml,           "DPGO_GRID_ML",            0,  "launch cap of the level-0 restriction / post-smoothing (0: resident count)")  \
  X(grid_edges,        "DPGO_GRID_EDGES",         0,  "launch cap of k_edge_robust, GNC and robust re-weighting alike (0: 1024)")    \
  X(persist,           "DPGO_PERSIST",           -1,  "one-launch solve (k_rtr_persist) off / on whatever the size: 0 / 1")          \
  X(persist_max_poses, "DPGO_PERSIST_MAX_POSES",  0,  "largest block the one-launch solve takes (0: every block it can hold)")       \
  X(persist_split,     "DPGO_PERSIST_SPLIT",      0,  "lane groups per pose of the one-launch solve: 1, 4 (0: by size)")             \
  X(persist_mt,        "DPGO_PERSIST_MT",         0,  "tiles per workgroup of the one-launch solve: 1, 2 (0: by size)")              \
  X(additive_tiles,    "DPGO_ADDITIVE_TILES",     1,  "workgroup tiles per aggregate of the additive one-launch solve: 1, 2 (opt-in: blocks up to ~28 000 poses)") \
  X(poll_first,        "DPGO_POLL_FIRST",        -1,  "s_sleep units before the first sweep of the in-kernel all-reduce")            \
  X(poll_sleep,        "DPGO_POLL_SLEEP",        -1,  "s_sleep units between sweeps of the in-kernel all-reduce")                    \
  X(poll_first_pay,    "DPGO_POLL_FIRST_PAY",    -1,  "the same before the first sweep of a reduction that carries a payload")       \
  X(persist_verbose,   "DPGO_PERSIST_VERBOSE",    0,  "per-solve phase report of the one-launch solve on stderr")                    \
  X(setup_timing,      "DPGO_SETUP_TIMING",       0,  "section times of the hierarchy's symbolic set-up on stderr")                  \
  X(setup_threads,     "DPGO_SETUP_THREADS",      0,  "host threads of the hierarchy's symbolic set-up (0: min(8, cores); 1: serial)") \
  X(setup_pin,         "DPGO_SETUP_PIN",          1,  "set-up worker threads placed in the CPU group of the thread that first used them") \
  X(auto_cost_rule,    "DPGO_AUTO_COST_RULE",     1,  "DPGO_PRECOND_AUTO on coupled blocks: cost rule (0: tCG-budget hysteresis only)") \
  X(ml_graph,          "DPGO_ML_GRAPH",           1,  "graph aggregates in the default hierarchy (0: index runs)")                   \
  X(ml_graph_size,     "DPGO_ML_GRAPH_SIZE",      0,  "growth size of the default graph aggregates (0: by size)")                    \
  X(ml_growth_chunks,  "DPGO_ML_GROWTH_CHUNKS",   0,  "index ranges the graph aggregates grow and merge in (0: 8 from 65 536 poses, else 1)") \
  X(ml_ap,             "DPGO_ML_AP",              1,  "two-level post-smoothing through A P (0: gather through Q; index runs only)") \
  X(ml_dense_sym,      "DPGO_ML_DENSE_SYM",      -1,  "dense level from the packed lower triangle on the matrix cores: 0 / 1")       \
  X(ml_early_stop,     "DPGO_ML_EARLY_STOP",      1,  "tCG's residual test in the restriction kernel, one kernel early")             \
  X(ml_operator_bits,  "DPGO_ML_OPERATOR_BITS",   0,  "level-0 operator copies of the cycle on HBM-bound blocks: 32 / 64 (0: 32)")   \
  X(ml_vector_bits,    "DPGO_ML_VECTOR_BITS",     0,  "cycle-internal vectors (pre-smoothed iterate, kept residual) beside fp32 operator copies: 32 / 64 (0: 32)") \
  X(ml_dense_bits,     "DPGO_ML_DENSE_BITS",      0,  "dense level beside fp32 cycle vectors: 32 / 64 (0: 64 -- fp32 measured neutral)") \
  X(gj_mfma,           "DPGO_GJ_MFMA",            1,  "rank-64 updates of the dense inverse on the fp64 matrix cores")               \
  X(dense_chunk,       "DPGO_DENSE_CHUNK",        0,  "tiles per workgroup of k_dense_sym_apply (0: default)")                       \
  X(coarse_nodes,      "DPGO_COARSE_NODES",       0,  "nodes per workgroup of k_ml_coarse_prolong: 1-4 (0: by size)")                \
  X(coarse_grid,       "DPGO_COARSE_GRID",        0,  "launch cap of k_ml_coarse_prolong (0: default)")                              \
  X(coarse_nt,         "DPGO_COARSE_NT",         -1,  "non-temporal loads of the dense inverse: 0 / 1")
struct Options {
#define X(field, var, unset, text) int field = unset;
  DPGO_OPTIONS(X)
#undef X
};
inline Options& options_storage() {
  static Options o;
  return o;
}
inline void options_read(Options& o) {
  o = Options();
#define X(field, var, unset, text) \
  if (const char* e_ = std::getenv(var)) o.field = (*e_ == 0) ? 1 : std::atoi(e_);
  DPGO_OPTIONS(X)
#undef X
}
inline const Options& options() {
  static const bool once = (options_read(options_storage()), true);
  (void)once;
  return options_storage();
}
inline std::string options_describe() {
  const Options& o = options();
  std::string s;
#define X(field, var, unset, text) s += std::string(var) + "=" + std::to_string(o.field) + (o.field == (unset) ? "" : " [set]") + "  # " + text + "\n";
  DPGO_OPTIONS(X)
#undef X
  return s;
}

}  // namespace dpgo_host
