// aggregation.h -- the host side of the hierarchy's symbolic set-up as plain C++ over index vectors: aggregates (greedy
// growth, fragment merge, index runs), the block patterns that follow from them, the run / tile / chunk tables the kernels
// read, the decoding of a hierarchy's shape and the search for the additive layout's aggregates.  Host compiler only:
// nothing from HIP, no kernel header, no problem handle -- the kernels' constants (tile sizes, kDenseChunk ...) arrive as
// arguments.  multilevel.hip sizes buffers, starts jobs, calls these and uploads; tests/cxx/test_aggregation.cpp calls
// them alone.  DESIGN.md section 5.
#pragma once

#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

namespace dpgo_host {

// block pattern of a square block-sparse matrix (block rows with sorted block columns)
struct Pattern {
  std::vector<int32_t> rowptr, colidx;
  int n() const { return (int)rowptr.size() - 1; }
};

// lab = aggregate of every node, mem / ptr = the aggregates' members, parent / pslot = the breadth-first tree of graph
// aggregates (parent of every non-root node, slot of block (parent, node) in the pattern; -1 / 0 for a root)
struct Aggregates {
  std::vector<int32_t> lab, ptr, mem, parent, pslot;
  int count() const { return (int)ptr.size() - 1; }
  // runs of k consecutive indices (the last one ragged): lab[i] = i / k, members in index order, no tree
  static Aggregates index_runs(int n, int k);
};

// Large blocks grow (and merge) their aggregates independently inside `chunks` contiguous index ranges -- [n c / chunks,
// n (c + 1) / chunks): a seed's search does not leave its range, a fragment joins a neighbour of its own range -- one host
// thread each; the ranges' aggregates are numbered one range after the other.  This is the RULE (restated in the oracle:
// amg_growth_chunks / the lo, hi arguments of amg_graph_aggregates and amg_merge_small_aggregates), not a schedule: the
// result does not depend on the number of threads that execute it.  100k poses: growth + merge 3.7 -> 0.6 ms.
int ml_growth_chunks(int n);

// Graph aggregates of at most S nodes, grown greedily: seeds in index order; a seed's aggregate takes unassigned nodes in
// breadth-first order (queue; a node's neighbours in the order of its block row) until it holds S; mem / ptr = members in
// discovery order.  Restated in oracle/dpgo_oracle.py (amg_graph_aggregates).
Aggregates grow_aggregates(const Pattern& P, int S, int chunks);
// The merge: the greedy growth leaves fragments (pockets between full aggregates); where an aggregate is a WORKGROUP of the
// one-launch solve (additive preconditioner) every fragment costs a whole workgroup.  Passes over the aggregates in index
// order until nothing changes: an aggregate of at most S / 2 nodes joins the neighbouring aggregate (one it shares a block
// with) it has the most blocks in common with among those that still have room (sizes add up to at most `cap`; ties: the
// lower index).  Afterwards the aggregates are renumbered in the order of their smallest member and every aggregate's
// breadth-first tree is rebuilt from that member (neighbours in block-row order).  Aggregates that are not grow_aggregates'
// output for the same `chunks` (numbered range after range, none across a range boundary) are merged as ONE range.
// Returns the number of aggregates.  Restated in the oracle (amg_merge_small_aggregates).
int merge_small_aggregates(const Pattern& P, int S, int cap, int chunks, Aggregates& agg);
// Growth to S and merge up to min(tile, 3 S / 2) for S = S_first, then in steps of an eighth (at least 2) while S <= tile,
// until at most `want` aggregates are left: their number, with *S / *cap what they were made with; 0 if no size gets there
// (agg then holds the last attempt).
int search_merged_aggregates(const Pattern& P, int S_first, int tile, int want, int chunks, Aggregates& agg, int* S, int* cap);

// Pattern of A P: row i holds the sorted, distinct aggregates of its block columns (P.n() rows).  Rows in parallel.
Pattern ap_pattern(const Pattern& P, const Aggregates& agg);
// Pattern of the next level's operator: row a holds the sorted, distinct aggregates of the block columns of the rows of a's
// members.  Aggregates in parallel, on at most `threads` threads.
Pattern coarse_pattern(const Pattern& P, const Aggregates& agg, int threads);

// Runs of equal labels inside chunks of G consecutive poses (what one wave of the level-0 kernels adds up before it
// writes): seg_info[first pose of a run] = 32 * slot + length (-1 elsewhere), the slots ordered by aggregate and, inside
// an aggregate, by pose (a counting sort over the runs), seg_ptr = the aggregates' slot ranges.  Returns the run count.
int run_table(const std::vector<int32_t>& lab, int na, int G, std::vector<int32_t>& seg_info, std::vector<int32_t>& seg_ptr);
// the additive preconditioner's persistent layout, aggregate = workgroup tile of `tile` slots: pose of every
// (aggregate, slot), members in their order, -1 = empty
std::vector<int32_t> tile_table(const Aggregates& agg, int tile);
// position of every node in agg.mem
std::vector<int32_t> member_positions(const Aggregates& agg);
// block row of every slot of the pattern
std::vector<int32_t> slot_rows(const Pattern& P);
// The packed lower block triangle of nT x nT tiles cut into chunks of at most `chunk` consecutive tiles of one block row
// (one workgroup of k_dense_sym_apply each): chunks = {I, J0, count, 0} row after row, first[I] = block row I's first
// chunk, first[nT] = their number.  Chunk: the kernels' DenseChunk (four ints).
template <class Chunk>
void dense_chunk_table(int nT, int chunk, std::vector<Chunk>& chunks, std::vector<int>& first) {
  chunks.clear();
  first.assign(nT + 1, 0);
  for (int I = 0; I < nT; ++I) {
    first[I] = (int)chunks.size();
    for (int J0 = 0; J0 <= I; J0 += chunk) chunks.push_back(Chunk{I, J0, std::min(chunk, I + 1 - J0), 0});
  }
  first[nT] = (int)chunks.size();
}

// A hierarchy's shape, decoded from the list the C API takes: aggregate sizes per coarsening; {-S}: two levels, graph
// aggregates of at most S poses; {-S, -cap}: the same with the fragments of the greedy growth merged up to `cap` poses.
// (ml_current_ks, multilevel.hip, is the encoder.)
struct HierarchySpec {
  bool graph = false;
  int S = 0, cap = 0;   // graph aggregates: growth size, merge bound (0: plain growth)
  std::vector<int> ks;  // aggregate size per coarsening (graph: {S})
  bool decode(const std::vector<int>& ks_in, std::string* err);  // false: *err says what is wrong with ks_in
};

}  // namespace dpgo_host
