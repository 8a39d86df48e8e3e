// aggregation.cpp -- aggregates, block patterns and tables of the hierarchy's symbolic set-up (aggregation.h).  Host
// compiler only.
#include "aggregation.h"
#include "taskpool.h"

#include <chrono>
#include <cstdio>

namespace dpgo_host {

Aggregates Aggregates::index_runs(int n, int k) {
  Aggregates R;
  const int na = (n + k - 1) / k;
  R.lab.resize(n);
  R.mem.resize(n);
  for (int i = 0; i < n; ++i) R.lab[i] = i / k, R.mem[i] = i;
  R.ptr.resize(na + 1);
  for (int a = 0; a <= na; ++a) R.ptr[a] = std::min(n, a * k);
  return R;
}

int ml_growth_chunks(int n) {
  const int forced = options().ml_growth_chunks;
  if (forced > 0) return std::max(1, std::min(forced, std::max(1, n / 64)));
  return n >= 65536 ? 8 : 1;
}
namespace {
// one index range's aggregates: members and their number (ids local to the range, from 0)
struct Part {
  std::vector<int32_t> ptr, mem;
  int na = 0;
};
// growth inside [lo, hi): agg.lab (ids local to the range), agg.parent, agg.pslot written at the range's indices; the
// members go to the range's part
int grow_range(const Pattern& P, int lo, int hi, int S, Aggregates& agg, Part& part) {
  const auto &rowptr = P.rowptr, &colidx = P.colidx;
  auto &lab = agg.lab, &parent = agg.parent, &pslot = agg.pslot, &ptr = part.ptr, &mem = part.mem;
  mem.clear();
  mem.reserve(hi - lo);
  ptr.assign(1, 0);
  int na = 0;
  for (int s = lo; s < hi; ++s) {
    if (lab[s] >= 0) continue;
    const size_t first = mem.size();
    lab[s] = na;
    mem.push_back(s);
    for (size_t head = first; head < mem.size() && (int)(mem.size() - first) < S; ++head) {
      const int u = mem[head];
      for (int t = rowptr[u]; t < rowptr[u + 1] && (int)(mem.size() - first) < S; ++t) {
        const int v = colidx[t];
        if (v < lo || v >= hi || lab[v] >= 0) continue;
        lab[v] = na;
        parent[v] = u;
        pslot[v] = t;
        mem.push_back(v);
      }
    }
    ptr.push_back((int32_t)mem.size());
    ++na;
  }
  return na;
}

// merge inside [lo, hi) (agg.lab: ids local to the range); in place; returns the number of aggregates of the range
int merge_range(const Pattern& P, int lo, int hi, int S, int cap, Aggregates& agg, Part& part) {
  const auto &rowptr = P.rowptr, &colidx = P.colidx;
  auto &lab = agg.lab, &parent = agg.parent, &pslot = agg.pslot, &ptr = part.ptr, &mem = part.mem;
  const int na = (int)ptr.size() - 1;
  const int n = hi - lo;
  std::vector<std::vector<int32_t>> members(na);
  for (int a = 0; a < na; ++a) members[a].assign(mem.begin() + ptr[a], mem.begin() + ptr[a + 1]);
  std::vector<int> cnt(na, 0);
  std::vector<int> touched;
  for (bool changed = true; changed;) {
    changed = false;
    for (int a = 0; a < na; ++a) {
      if (members[a].empty() || 2 * (int)members[a].size() > S) continue;
      touched.clear();
      for (int i : members[a])
        for (int t = rowptr[i]; t < rowptr[i + 1]; ++t) {
          const int v = colidx[t];
          if (v < lo || v >= hi) continue;
          const int c = lab[v];
          if (c == a) continue;
          if (cnt[c]++ == 0) touched.push_back(c);
        }
      std::sort(touched.begin(), touched.end());
      int best = -1, best_n = 0;
      for (int c : touched) {
        if ((int)(members[c].size() + members[a].size()) <= cap && cnt[c] > best_n) best = c, best_n = cnt[c];
        cnt[c] = 0;
      }
      if (best >= 0) {
        members[best].insert(members[best].end(), members[a].begin(), members[a].end());
        for (int i : members[a]) lab[i] = best;
        members[a].clear();
        changed = true;
      }
    }
  }
  // Members of the surviving aggregates in index order (one counting pass over the poses instead of a sort per aggregate),
  // `grew` = absorbed at least one other aggregate.
  std::vector<char> grew(na, 0);
  for (int a = 0; a < na; ++a)
    if (!members[a].empty() && (int)members[a].size() != ptr[a + 1] - ptr[a]) grew[a] = 1;
  std::vector<int32_t> first_member(na, -1);
  for (int i = hi - 1; i >= lo; --i) first_member[lab[i]] = i;
  std::vector<int> alive;
  for (int a = 0; a < na; ++a)
    if (!members[a].empty()) alive.push_back(a);
  std::sort(alive.begin(), alive.end(), [&](int x, int y) { return first_member[x] < first_member[y]; });
  std::vector<int32_t> sorted_mem, sorted_ptr(na + 1, 0);
  {  // only the aggregates that grew need their members sorted (the roots of the search below)
    for (int a = 0; a < na; ++a) sorted_ptr[a + 1] = sorted_ptr[a] + (grew[a] ? (int32_t)members[a].size() : 0);
    sorted_mem.resize(sorted_ptr[na]);
    std::vector<int32_t> fill(sorted_ptr.begin(), sorted_ptr.end() - 1);
    for (int i = lo; i < hi; ++i)
      if (grew[lab[i]]) sorted_mem[fill[lab[i]]++] = i;
  }
  std::vector<int32_t> new_lab(n, -1), new_mem;  // (new_lab indexed by pose - lo)
  std::vector<int32_t> old_parent(parent.begin() + lo, parent.begin() + hi), old_pslot(pslot.begin() + lo, pslot.begin() + hi);
  std::fill(parent.begin() + lo, parent.begin() + hi, -1);
  std::fill(pslot.begin() + lo, pslot.begin() + hi, 0);
  new_mem.reserve(n);
  std::vector<int32_t> new_ptr(1, 0);
  for (size_t k = 0; k < alive.size(); ++k) {
    const int a = alive[k];
    if (!grew[a]) {
      // untouched by the merge: the growth's own search started from the aggregate's smallest member (seeds are taken in
      // index order) and claimed exactly these poses in exactly the order the search below would -- keep its tree
      for (int m = ptr[a]; m < ptr[a + 1]; ++m) {
        const int v = mem[m];
        new_lab[v - lo] = (int32_t)k;
        parent[v] = old_parent[v - lo];
        pslot[v] = old_pslot[v - lo];
        new_mem.push_back(v);
      }
      new_ptr.push_back((int32_t)new_mem.size());
      continue;
    }
    // (a merged aggregate is connected by construction, so the search from its smallest member reaches everything; should
    // the pattern not be symmetric, the members it misses become further roots in index order)
    for (int q = sorted_ptr[a]; q < sorted_ptr[a + 1]; ++q) {
      const int root = sorted_mem[q];
      if (new_lab[root - lo] >= 0) continue;
      size_t head = new_mem.size();
      new_lab[root - lo] = (int32_t)k;
      new_mem.push_back(root);
      for (; head < new_mem.size(); ++head) {
        const int u = new_mem[head];
        for (int t = rowptr[u]; t < rowptr[u + 1]; ++t) {
          const int v = colidx[t];
          if (v < lo || v >= hi || lab[v] != a || new_lab[v - lo] >= 0) continue;
          new_lab[v - lo] = (int32_t)k;
          parent[v] = u;
          pslot[v] = t;
          new_mem.push_back(v);
        }
      }
    }
    new_ptr.push_back((int32_t)new_mem.size());
  }
  mem.swap(new_mem);
  ptr.swap(new_ptr);
  std::copy(new_lab.begin(), new_lab.end(), lab.begin() + lo);
  return (int)alive.size();
}

// growth (do_grow) and / or merge (cap > 0) inside the index ranges, the ranges' aggregates joined one after the other
int grow_and_merge(const Pattern& P, int S, int cap, bool do_grow, int chunks, Aggregates& agg) {
  const int n = P.n();
  auto &lab = agg.lab, &ptr = agg.ptr, &mem = agg.mem;
  chunks = std::max(1, std::min(chunks, std::max(1, n)));
  if (do_grow) {
    lab.assign(n, -1);
    agg.parent.assign(n, -1);
    agg.pslot.assign(n, 0);
  }
  std::vector<Part> parts(chunks);
  auto bound = [&](int c) { return (int)((long long)n * c / chunks); };
  if (!do_grow) {
    // the caller's aggregates (grow_aggregates' output: numbered range after range, none across a range boundary) are
    // split by range, ids local to the range; anything else is merged as ONE range
    const int na_in = (int)ptr.size() - 1;
    std::vector<int> first_agg(chunks + 1, na_in);
    bool split_ok = chunks > 1;
    if (split_ok) {
      int c = 0;
      first_agg[0] = 0;
      for (int a = 0; a < na_in && split_ok; ++a) {
        if (ptr[a + 1] <= ptr[a]) { split_ok = false; break; }
        int lo_m = n, hi_m = -1;
        for (int m = ptr[a]; m < ptr[a + 1]; ++m) lo_m = std::min(lo_m, (int)mem[m]), hi_m = std::max(hi_m, (int)mem[m]);
        while (c + 1 < chunks && lo_m >= bound(c + 1)) first_agg[++c] = a;
        if (lo_m < bound(c) || hi_m >= bound(c + 1)) split_ok = false;
      }
      while (c + 1 < chunks) first_agg[++c] = na_in;
      first_agg[chunks] = na_in;
    }
    if (!split_ok) {
      chunks = 1;
      parts.resize(1);
      parts[0].ptr = ptr;
      parts[0].mem = mem;
      parts[0].na = na_in;
    } else {
      for (int c = 0; c < chunks; ++c) {
        const int a0 = first_agg[c], a1 = first_agg[c + 1];
        Part& part = parts[c];
        part.na = a1 - a0;
        part.ptr.assign(1, 0);
        for (int a = a0; a < a1; ++a) part.ptr.push_back(ptr[a + 1] - ptr[a0]);
        part.mem.assign(mem.begin() + ptr[a0], mem.begin() + ptr[a1]);
        if (a0 > 0)
          for (int i = bound(c); i < bound(c + 1); ++i) lab[i] -= a0;
      }
    }
  }
  const bool timing_ = options().setup_timing > 1;
  const auto tA = std::chrono::steady_clock::now();
  std::vector<double> tch(chunks, 0.0);
  parallel_ranges(chunks, std::min(chunks, setup_threads()), [&](int, int c0, int c1) {
    for (int c = c0; c < c1; ++c) {
      const auto t0 = std::chrono::steady_clock::now();
      Part& part = parts[c];
      const int lo = bound(c), hi = bound(c + 1);
      if (do_grow) part.na = grow_range(P, lo, hi, S, agg, part);
      if (cap > 0) part.na = merge_range(P, lo, hi, S, cap, agg, part);
      tch[c] = 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    }
  });
  const auto tB = std::chrono::steady_clock::now();
  // the ranges' aggregates one after the other
  std::vector<int> agg_off(chunks + 1, 0);
  std::vector<size_t> mem_off(chunks + 1, 0);
  for (int c = 0; c < chunks; ++c) agg_off[c + 1] = agg_off[c] + parts[c].na, mem_off[c + 1] = mem_off[c] + parts[c].mem.size();
  const int na = agg_off[chunks];
  mem.resize(mem_off[chunks]);
  ptr.assign((size_t)na + 1, 0);
  parallel_ranges(chunks, std::min(chunks, setup_threads()), [&](int, int c0, int c1) {
    for (int c = c0; c < c1; ++c) {
      const Part& part = parts[c];
      if (agg_off[c] > 0)
        for (int i = bound(c); i < bound(c + 1); ++i) lab[i] += agg_off[c];
      for (int a = 0; a < part.na; ++a) ptr[(size_t)agg_off[c] + a + 1] = (int32_t)(mem_off[c] + part.ptr[a + 1]);
      if (!part.mem.empty()) std::memcpy(mem.data() + mem_off[c], part.mem.data(), sizeof(int32_t) * part.mem.size());
    }
  });
  if (timing_) {
    std::fprintf(stderr, "dpgo_hip: grow / merge (%d ranges): parallel section %.3f ms, join %.3f ms; per range:", chunks,
                 1e3 * std::chrono::duration<double>(tB - tA).count(),
                 1e3 * std::chrono::duration<double>(std::chrono::steady_clock::now() - tB).count());
    for (double t : tch) std::fprintf(stderr, " %.3f", t);
    std::fprintf(stderr, "\n");
  }
  return na;
}
}  // namespace

Aggregates grow_aggregates(const Pattern& P, int S, int chunks) {
  Aggregates agg;
  grow_and_merge(P, S, 0, true, chunks, agg);
  return agg;
}
int merge_small_aggregates(const Pattern& P, int S, int cap, int chunks, Aggregates& agg) {
  return grow_and_merge(P, S, cap, false, chunks, agg);
}
int search_merged_aggregates(const Pattern& P, int S_first, int tile, int want, int chunks, Aggregates& agg, int* S_out, int* cap_out) {
  for (int S = S_first; S <= tile; S += std::max(2, S / 8)) {
    const int cap = std::min(tile, S + S / 2);
    grow_and_merge(P, S, 0, true, chunks, agg);
    const int na = grow_and_merge(P, S, cap, false, chunks, agg);
    if (na <= want) {
      *S_out = S, *cap_out = cap;
      return na;
    }
  }
  return 0;
}

// (Inserting into the sorted row instead of sort + unique was measured: no gain, the labels' gather is what it costs.)
Pattern ap_pattern(const Pattern& P, const Aggregates& agg) {
  const auto &rowptr = P.rowptr, &colidx = P.colidx, &lab = agg.lab;
  Pattern AP;
  pattern_by_ranges(P.n(), setup_threads(), 1024, colidx.size(), [&](int, int i, std::vector<int32_t>& out) {
    const size_t first = out.size();
    for (int t = rowptr[i]; t < rowptr[i + 1]; ++t) out.push_back(lab[colidx[t]]);
    std::sort(out.begin() + first, out.end());
    out.erase(std::unique(out.begin() + first, out.end()), out.end());
  }, AP.rowptr, AP.colidx);
  return AP;
}

Pattern coarse_pattern(const Pattern& P, const Aggregates& agg, int threads) {
  const auto &rowptr = P.rowptr, &colidx = P.colidx, &lab = agg.lab, &ptr = agg.ptr, &mem = agg.mem;
  const int na = agg.count();
  const int chunks = std::max(1, std::min(std::max(1, threads), na / 16 + 1));
  std::vector<std::vector<int32_t>> marks(chunks);  // per range: the last aggregate that listed a column
  Pattern C;
  pattern_by_ranges(na, chunks, 16, colidx.size() / 8, [&](int c, int a, std::vector<int32_t>& out) {
    auto& mark = marks[c];
    if (mark.empty()) mark.assign(na, -1);
    const size_t first = out.size();
    for (int m = ptr[a]; m < ptr[a + 1]; ++m) {
      const int i = mem[m];
      for (int t = rowptr[i]; t < rowptr[i + 1]; ++t) {
        const int cl = lab[colidx[t]];
        if (mark[cl] != a) {
          mark[cl] = a;
          out.push_back(cl);
        }
      }
    }
    std::sort(out.begin() + first, out.end());
  }, C.rowptr, C.colidx);
  return C;
}

int run_table(const std::vector<int32_t>& lab, int na, int G, std::vector<int32_t>& seg_info, std::vector<int32_t>& seg_ptr) {
  const int n = (int)lab.size();
  seg_info.assign(n, -1);
  seg_ptr.assign(na + 1, 0);
  int nruns = 0;
  for (int i = 0; i < n;) {
    int j = i + 1;
    while (j < n && j % G != 0 && lab[j] == lab[i]) ++j;
    seg_info[i] = j - i;  // (length for now)
    seg_ptr[lab[i] + 1] += 1;
    ++nruns;
    i = j;
  }
  for (int a = 0; a < na; ++a) seg_ptr[a + 1] += seg_ptr[a];
  std::vector<int32_t> next(seg_ptr.begin(), seg_ptr.end() - 1);
  for (int i = 0; i < n;) {
    const int len = seg_info[i];
    seg_info[i] = len + 32 * next[lab[i]]++;
    i += len;
  }
  return nruns;
}

std::vector<int32_t> tile_table(const Aggregates& agg, int tile) {
  const int na = agg.count();
  std::vector<int32_t> tperm((size_t)na * tile, -1);
  for (int a = 0; a < na; ++a)
    for (int m = agg.ptr[a]; m < agg.ptr[a + 1]; ++m) tperm[(size_t)a * tile + (m - agg.ptr[a])] = agg.mem[m];
  return tperm;
}

std::vector<int32_t> member_positions(const Aggregates& agg) {
  std::vector<int32_t> mpos(agg.mem.size());
  for (size_t m = 0; m < agg.mem.size(); ++m) mpos[agg.mem[m]] = (int32_t)m;
  return mpos;
}

std::vector<int32_t> slot_rows(const Pattern& P) {
  std::vector<int32_t> srow(P.colidx.size());
  for (int i = 0; i < P.n(); ++i)
    for (int t = P.rowptr[i]; t < P.rowptr[i + 1]; ++t) srow[t] = i;
  return srow;
}

bool HierarchySpec::decode(const std::vector<int>& ks_in, std::string* err) {
  const bool merged = ks_in.size() == 2 && ks_in[0] < 0 && ks_in[1] < 0;
  graph = (ks_in.size() == 1 && ks_in[0] < 0) || merged;
  ks = ks_in;
  if (merged) ks.pop_back();
  if (graph) ks[0] = -ks_in[0];
  S = graph ? ks[0] : 0;
  cap = merged ? -ks_in[1] : 0;
  if (merged && cap < S) return *err = "the merge bound is at least the growth size", false;
  for (int k : ks)
    if (k < 0) return *err = "graph aggregates (a negative size) make a two-level hierarchy", false;
  if (graph && S < 2) return *err = "graph aggregates hold at least 2 poses", false;
  return true;
}

}  // namespace dpgo_host
