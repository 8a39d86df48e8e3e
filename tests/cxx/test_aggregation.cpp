// The hierarchy's set-up over index vectors (dpgo_amd/csrc/aggregation.h, taskpool.h, options.h), with the host compiler and
// no library: aggregates (growth, merge, index runs), the two block patterns against a brute-force construction, the run /
// tile / chunk tables, the additive layout's search and the decoding of a hierarchy's shape -- everything at 1, 3 and 8
// set-up threads with bitwise equal results.  The same program is what runs under the address and thread sanitizers.
#include "aggregation.h"
#include "taskpool.h"

#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

using namespace dpgo_host;

static int failures = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      if (failures < 40) std::printf("aggregation: line %d: %s\n", __LINE__, #cond); \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

typedef std::vector<int32_t> Vec;
typedef std::vector<std::set<int>> Adj;  // row -> block columns

static Pattern pattern_of(const Adj& adj) {
  Pattern P;
  P.rowptr.assign(1, 0);
  for (const auto& row : adj) {
    P.colidx.insert(P.colidx.end(), row.begin(), row.end());
    P.rowptr.push_back((int32_t)P.colidx.size());
  }
  return P;
}
static Adj chain(int n) {
  Adj adj(n);
  for (int i = 0; i < n; ++i) {
    adj[i].insert(i);
    if (i > 0) adj[i].insert(i - 1);
    if (i + 1 < n) adj[i].insert(i + 1);
  }
  return adj;
}
static Adj grid(int nx, int ny, int nz) {
  Adj adj(nx * ny * nz);
  auto id = [&](int x, int y, int z) { return (z * ny + y) * nx + x; };
  for (int z = 0; z < nz; ++z)
    for (int y = 0; y < ny; ++y)
      for (int x = 0; x < nx; ++x) {
        auto& row = adj[id(x, y, z)];
        row.insert(id(x, y, z));
        if (x > 0) row.insert(id(x - 1, y, z));
        if (x + 1 < nx) row.insert(id(x + 1, y, z));
        if (y > 0) row.insert(id(x, y - 1, z));
        if (y + 1 < ny) row.insert(id(x, y + 1, z));
        if (z > 0) row.insert(id(x, y, z - 1));
        if (z + 1 < nz) row.insert(id(x, y, z + 1));
      }
  return adj;
}

// Everything the issue of a set of aggregates must satisfy.  max_size: S after the growth, cap after the merge; chunks: the
// index ranges they were made in; one_root: the pattern is symmetric, so every aggregate is one tree.
static void check_aggregates(const Pattern& P, const Aggregates& g, int max_size, int chunks, bool one_root) {
  const int n = P.n(), na = g.count();
  EXPECT((int)g.lab.size() == n && (int)g.mem.size() == n && (int)g.parent.size() == n && (int)g.pslot.size() == n);
  EXPECT(na >= 1 && g.ptr[0] == 0 && g.ptr[na] == n);
  if (failures) return;
  std::vector<char> seen(n, 0);
  chunks = std::max(1, std::min(chunks, n));
  int range = 0;  // of the previous aggregate: ids ascend range after range
  for (int a = 0; a < na; ++a) {
    EXPECT(g.ptr[a + 1] > g.ptr[a] && g.ptr[a + 1] - g.ptr[a] <= max_size);
    int roots = 0;
    const int first = g.mem[g.ptr[a]];
    int c = 0;
    while (c + 1 < chunks && first >= (int)((long long)n * (c + 1) / chunks)) ++c;
    EXPECT(c >= range);
    range = c;
    for (int m = g.ptr[a]; m < g.ptr[a + 1]; ++m) {
      const int v = g.mem[m];
      EXPECT(v >= 0 && v < n && !seen[v] && g.lab[v] == a);
      if (v < 0 || v >= n) return;
      seen[v] = 1;
      EXPECT(v >= (int)((long long)n * c / chunks) && v < (int)((long long)n * (c + 1) / chunks));  // inside the range
      const int u = g.parent[v];
      if (u < 0) {
        ++roots;
        continue;
      }
      EXPECT(u < n && g.lab[u] == a);
      EXPECT(g.pslot[v] >= P.rowptr[u] && g.pslot[v] < P.rowptr[u + 1] && P.colidx[g.pslot[v]] == v);
    }
    EXPECT(g.parent[first] < 0 && roots >= 1 && (!one_root || roots == 1));
  }
  for (int v = 0; v < n; ++v) EXPECT(seen[v]);
}

static void check_patterns(const Pattern& P, const Aggregates& g, int threads) {
  const int n = P.n(), na = g.count();
  Adj ap(n), co(na);
  for (int i = 0; i < n; ++i)
    for (int t = P.rowptr[i]; t < P.rowptr[i + 1]; ++t) {
      ap[i].insert(g.lab[P.colidx[t]]);
      co[g.lab[i]].insert(g.lab[P.colidx[t]]);
    }
  const Pattern AP = ap_pattern(P, g), want_ap = pattern_of(ap);
  EXPECT(AP.rowptr == want_ap.rowptr && AP.colidx == want_ap.colidx);
  const Pattern C = coarse_pattern(P, g, threads), want_c = pattern_of(co);
  EXPECT(C.rowptr == want_c.rowptr && C.colidx == want_c.colidx);
}

static void check_run_table(const Vec& lab, int na, int G) {
  const int n = (int)lab.size();
  Vec info, ptr;
  const int nruns = run_table(lab, na, G, info, ptr);
  EXPECT((int)info.size() == n && (int)ptr.size() == na + 1 && ptr[0] == 0 && nruns == ptr[na]);
  if (failures) return;
  Vec rebuilt(n, -1), next(ptr.begin(), ptr.end() - 1);
  for (int i = 0; i < n;) {
    EXPECT(info[i] >= 0);
    if (info[i] < 0) return;
    const int slot = info[i] / 32, len = info[i] % 32;
    EXPECT(len >= 1 && i + len <= n && i / G == (i + len - 1) / G);  // no run crosses a multiple of G
    int a = 0;
    while (a + 1 < na && ptr[a + 1] <= slot) ++a;
    EXPECT(slot >= ptr[a] && slot < ptr[a + 1]);
    EXPECT(slot == next[a]);  // an aggregate's slots: contiguous from seg_ptr[a], in pose order
    ++next[a];
    for (int j = i; j < i + len && j < n; ++j) {
      rebuilt[j] = a;
      if (j > i) EXPECT(info[j] == -1);
    }
    if (len < 1) return;
    i += len;
  }
  EXPECT(rebuilt == lab);
  for (int a = 0; a < na; ++a) EXPECT(next[a] == ptr[a + 1]);
}

static void check_tile_table(const Aggregates& g, int tile) {
  const Vec tp = tile_table(g, tile);
  EXPECT((int)tp.size() == g.count() * tile);
  if (failures) return;
  for (int a = 0; a < g.count(); ++a)
    for (int s = 0; s < tile; ++s) {
      const int m = g.ptr[a] + s;
      EXPECT(tp[(size_t)a * tile + s] == (m < g.ptr[a + 1] ? g.mem[m] : -1));
    }
}

struct Chunk {
  int I, J0, cnt, pad;
};
static void check_dense_chunks(int nT, int chunk) {
  std::vector<Chunk> chunks;
  std::vector<int> first;
  dense_chunk_table(nT, chunk, chunks, first);
  EXPECT((int)first.size() == nT + 1 && first[nT] == (int)chunks.size());
  std::vector<int> cover((size_t)nT * nT, 0);
  for (const Chunk& c : chunks) {
    EXPECT(c.I >= 0 && c.I < nT && c.J0 >= 0 && c.cnt >= 1 && c.cnt <= chunk && c.J0 + c.cnt <= c.I + 1 && c.pad == 0);
    if (c.I < 0 || c.I >= nT || c.J0 < 0 || c.J0 + c.cnt > nT) return;
    for (int J = c.J0; J < c.J0 + c.cnt; ++J) cover[(size_t)c.I * nT + J] += 1;
  }
  for (int I = 0; I < nT; ++I) {
    for (int J = 0; J < nT; ++J) EXPECT(cover[(size_t)I * nT + J] == (J <= I ? 1 : 0));
    EXPECT(chunks[first[I]].I == I && chunks[first[I]].J0 == 0 && (first[I] == 0 || chunks[first[I] - 1].I == I - 1));
  }
}

static void append(Vec& blob, const Vec& v) {
  blob.push_back((int32_t)v.size());
  blob.insert(blob.end(), v.begin(), v.end());
}
static void append(Vec& blob, const Aggregates& g) {
  for (const Vec* v : {&g.lab, &g.ptr, &g.mem, &g.parent, &g.pslot}) append(blob, *v);
}
static void append(Vec& blob, const Pattern& P) {
  append(blob, P.rowptr);
  append(blob, P.colidx);
}

// growth (checked), merge (checked), both patterns against brute force, run and tile tables; everything into `blob`
static void grow_merge_case(const Pattern& P, int S, int cap, int chunks, bool symmetric, Vec& blob) {
  const int threads = setup_threads();
  Aggregates g = grow_aggregates(P, S, chunks);
  check_aggregates(P, g, S, chunks, symmetric);
  check_patterns(P, g, threads);
  append(blob, g);
  if (cap) {
    const int na = merge_small_aggregates(P, S, cap, chunks, g);
    EXPECT(na == g.count());
    check_aggregates(P, g, cap, chunks, symmetric);
    check_patterns(P, g, threads);
    append(blob, g);
  }
  append(blob, ap_pattern(P, g));
  append(blob, coarse_pattern(P, g, threads));
  append(blob, coarse_pattern(P, g, std::max(1, threads / 2)));
  for (int G : {16, 21, 4, 5}) {  // 64 / (b * split) for b = 4, 3 and split = 1, 4
    check_run_table(g.lab, g.count(), G);
    Vec info, ptr;
    blob.push_back(run_table(g.lab, g.count(), G, info, ptr));
    append(blob, info);
    append(blob, ptr);
  }
  check_tile_table(g, std::max(S, cap));
  check_tile_table(g, std::max(S, cap) + 3);
  append(blob, tile_table(g, std::max(S, cap)));
  const Vec mpos = member_positions(g);
  for (int m = 0; m < P.n(); ++m) EXPECT(mpos[g.mem[m]] == m);
  append(blob, mpos);
}

// every case once, at the current DPGO_SETUP_THREADS; returns all the arrays it produced
static Vec all_cases() {
  Vec blob;
  {  // one node
    const Pattern P = pattern_of(chain(1));
    grow_merge_case(P, 2, 3, 1, true, blob);
    grow_merge_case(P, 2, 0, 3, true, blob);  // (more ranges than nodes)
  }
  {  // two nodes, one aggregate: node 1 hangs on node 0 through slot (0, 1)
    const Pattern P = pattern_of(chain(2));
    const Aggregates g = grow_aggregates(P, 2, 1);
    EXPECT(g.count() == 1 && g.lab == Vec({0, 0}) && g.mem == Vec({0, 1}) && g.parent == Vec({-1, 0}) && g.pslot[1] == 1);
    grow_merge_case(P, 2, 2, 1, true, blob);
  }
  // 130 nodes in 3 ranges: boundaries at 43 / 86
  grow_merge_case(pattern_of(chain(130)), 4, 6, 3, true, blob);
  {  // 5 x 5 x 4 grid
    const Pattern P = pattern_of(grid(5, 5, 4));
    grow_merge_case(P, 7, 10, 1, true, blob);
    grow_merge_case(P, 7, 10, 3, true, blob);
  }
  {  // large enough for several row ranges of A P (1 024 rows each) and of the next level's pattern (16 aggregates each)
    const Pattern P = pattern_of(grid(40, 40, 4));
    grow_merge_case(P, 7, 10, 3, true, blob);
    grow_merge_case(P, 16, 0, 8, true, blob);
  }
  {  // the set-up's overlap: both patterns as one job of two items (each a parallel section of its own) while this thread
     // builds the tables, joined by wait() -- and a second job left to its guard
    const Pattern P = pattern_of(grid(40, 40, 4));
    const Aggregates g = grow_aggregates(P, 7, 3);
    const int threads = setup_threads();
    Pattern AP, C;
    Vec info, ptr, tiles;
    int side = 0;
    {
      JobGuard side_job{TaskPool::get().submit(1, [&](int) { side = 1; }, threads)};
      JobGuard job{TaskPool::get().submit(2, [&](int which) {
        if (which == 0)
          AP = ap_pattern(P, g);
        else
          C = coarse_pattern(P, g, threads / 2);
      }, threads)};
      run_table(g.lab, g.count(), 16, info, ptr);
      tiles = tile_table(g, 7);
      TaskPool::get().wait(job.job);
      const Pattern AP1 = ap_pattern(P, g), C1 = coarse_pattern(P, g, threads);
      EXPECT(AP.rowptr == AP1.rowptr && AP.colidx == AP1.colidx && C.rowptr == C1.rowptr && C.colidx == C1.colidx);
    }
    EXPECT(side == 1);
    append(blob, AP);
    append(blob, C);
  }
  {  // a node whose row holds only its diagonal: an aggregate of its own, before and after the merge
    Adj adj = chain(10);
    adj[4] = {4};
    adj[3].erase(4);
    adj[5].erase(4);
    const Pattern P = pattern_of(adj);
    Aggregates g = grow_aggregates(P, 4, 1);
    EXPECT(g.ptr[g.lab[4] + 1] - g.ptr[g.lab[4]] == 1);
    merge_small_aggregates(P, 4, 6, 1, g);
    EXPECT(g.ptr[g.lab[4] + 1] - g.ptr[g.lab[4]] == 1 && g.parent[4] == -1);
    grow_merge_case(P, 4, 6, 1, true, blob);
  }
  {  // block (2, 1) without (1, 2): {2} joins {0, 1} through its own row, the search from 0 cannot reach it -- a second root
    Adj adj(3);
    adj[0] = {0, 1};
    adj[1] = {0, 1};
    adj[2] = {1, 2};
    const Pattern P = pattern_of(adj);
    Aggregates g = grow_aggregates(P, 2, 1);
    EXPECT(g.count() == 2 && g.lab == Vec({0, 0, 1}));
    EXPECT(merge_small_aggregates(P, 2, 3, 1, g) == 1);
    EXPECT(g.lab == Vec({0, 0, 0}) && g.mem == Vec({0, 1, 2}) && g.parent == Vec({-1, 0, -1}));
    grow_merge_case(P, 2, 3, 1, false, blob);
  }
  {  // index runs: 23 nodes in runs of 4, the last one of 3; no tree; the same pattern functions
    const Aggregates r = Aggregates::index_runs(23, 4);
    EXPECT(r.count() == 6 && r.ptr == Vec({0, 4, 8, 12, 16, 20, 23}) && r.parent.empty() && r.pslot.empty());
    for (int i = 0; i < 23; ++i) EXPECT(r.lab[i] == i / 4 && r.mem[i] == i);
    check_patterns(pattern_of(chain(23)), r, setup_threads());
    for (int G : {16, 21, 4, 5}) check_run_table(r.lab, r.count(), G);
    check_tile_table(r, 4);
    const Pattern P = pattern_of(grid(40, 40, 4));  // (several row ranges)
    const Aggregates r8 = Aggregates::index_runs(P.n(), 8), r5 = Aggregates::index_runs(P.n(), 5);
    check_patterns(P, r8, setup_threads());
    check_patterns(P, r5, setup_threads());
    append(blob, ap_pattern(P, r5));
    append(blob, coarse_pattern(P, r5, setup_threads()));
    const Vec srow = slot_rows(P);
    for (int i = 0; i < P.n(); ++i)
      for (int t = P.rowptr[i]; t < P.rowptr[i + 1]; ++t) EXPECT(srow[t] == i);
  }
  {  // the search: growth sizes 4, 6, 8 ... 16 on the 5 x 5 x 4 grid; at S = 4 / cap 6 there are at least ceil(100 / 6) = 17
     // aggregates, so it has to step at least once to get to 12
    const Pattern P = pattern_of(grid(5, 5, 4));
    const int tile = 16, want = 12;
    Aggregates g;
    int S = 0, cap = 0;
    const int na = search_merged_aggregates(P, 4, tile, want, 1, g, &S, &cap);
    EXPECT(na > 0 && na <= want && na == g.count() && S > 4 && S <= tile && (S - 4) % 2 == 0 && cap == std::min(tile, S + S / 2));
    if (na > 0) {
      Aggregates h = grow_aggregates(P, S, 1);
      EXPECT(merge_small_aggregates(P, S, cap, 1, h) == na);
      EXPECT(h.lab == g.lab && h.ptr == g.ptr && h.mem == g.mem && h.parent == g.parent && h.pslot == g.pslot);
      for (int s = 4; s < S; s += std::max(2, s / 8)) {  // every earlier size of the schedule leaves more than `want`
        Aggregates e = grow_aggregates(P, s, 1);
        EXPECT(merge_small_aggregates(P, s, std::min(tile, s + s / 2), 1, e) > want);
        if (s + std::max(2, s / 8) > S) EXPECT(s + std::max(2, s / 8) == S);  // (S is on the schedule)
      }
      append(blob, g);
    }
    for (int w = 6; w <= 20; ++w) {  // every target: the search agrees with the schedule walked by hand
      int S_hand = 0, na_hand = 0;
      for (int s = 4; s <= tile && !S_hand; s += std::max(2, s / 8)) {
        Aggregates e = grow_aggregates(P, s, 1);
        na_hand = merge_small_aggregates(P, s, std::min(tile, s + s / 2), 1, e);
        if (na_hand <= w) S_hand = s;
      }
      int Sw = 0, capw = 0;
      const int naw = search_merged_aggregates(P, 4, tile, w, 1, g, &Sw, &capw);
      EXPECT(Sw == S_hand && naw == (S_hand ? na_hand : 0) && capw == (S_hand ? std::min(tile, S_hand + S_hand / 2) : 0));
    }
    int S2 = -1, cap2 = -1;
    EXPECT(search_merged_aggregates(P, 4, tile, 1, 1, g, &S2, &cap2) == 0 && S2 == -1 && cap2 == -1);  // 100 nodes, 16 at most each
  }
  return blob;
}

int main() {
  for (int nT : {1, 3, 50})
    for (int chunk : {1, 2})  // 2 = kDenseChunk (kernels/dense.h)
      check_dense_chunks(nT, chunk);
  {  // a hierarchy's shape
    std::string err;
    HierarchySpec s;
    EXPECT(!s.decode({-4, 8}, &err) && !err.empty());
    EXPECT(!s.decode({-1}, &err));
    EXPECT(!s.decode({-8, -4}, &err));
    EXPECT(s.decode({-8}, &err) && s.graph && s.S == 8 && s.cap == 0 && s.ks == std::vector<int>({8}));
    EXPECT(s.decode({-8, -12}, &err) && s.graph && s.S == 8 && s.cap == 12 && s.ks == std::vector<int>({8}));
    EXPECT(s.decode({4, 8}, &err) && !s.graph && s.S == 0 && s.cap == 0 && s.ks == std::vector<int>({4, 8}));
  }
  Vec first;
  for (const char* threads : {"1", "3", "8"}) {
    setenv("DPGO_SETUP_THREADS", threads, 1);
    options_read(options_storage());
    EXPECT(setup_threads() == std::atoi(threads));
    const Vec blob = all_cases();
    if (first.empty()) first = blob;
    EXPECT(!blob.empty() && blob == first);  // bitwise the same at every thread count
  }
  if (failures) return 1;
  std::printf("aggregation: ok\n");
  return 0;
}
