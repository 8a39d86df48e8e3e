// kernels/certify.h -- certificate of global optimality of the rank-r relaxation: products with the certificate matrix
// C(X) = Q - Lambda(X), the Gram blocks and linear combinations of the block eigen-solver (certify.hip), the
// preconditioner without tangent projection, the lift of an iterate to rank r + 1 along a witness.
// Part of kernels.h (included inside namespace dpgo, after init.h).
//
// An "r-row block" is one pose-tile vector [n, d+1, r]: r vectors of R^{(d+1)n} at once (row a of the block = element a of
// every column).  The eigen-solver works on blocks of the handle's own rank, so the compiled (D, R) instances are reused.
// Every reduction is a per-workgroup partial written in a fixed order and summed by k_cert_reduce in a fixed order: no
// float atomics, bitwise reproducible run to run.
#pragma once

constexpr int kCertMaxBlocks = 8;  // r-row blocks one Gram / combination pass reads
constexpr int kCertMaxOut = 4;     // outputs of one combination pass
constexpr int kCertMaxPairs = 16;  // Gram blocks of one pass
constexpr int kCertCols = 64;      // columns per LDS chunk of k_cert_gram

struct CertIn {
  const double* b[kCertMaxBlocks];
};
struct CertOut {
  double* b[kCertMaxOut];
};
struct CertPairs {
  int8_t x[kCertMaxPairs], y[kCertMaxPairs];
};

// ================================================================ CW = W Q - W_rot Lambda(X)   (no tangent projection)
// Lambda's top-left D x D block of pose i is S_i = sym(Y_i^T (XQ)_rot,i), cached by k_grad at X; its last row and column
// are zero.  k_hess without proj_X.  partials: the R x R block W CW^T of this workgroup, row-major, at
// partials[blockIdx.x * R * R].
template <int D, int R, int SPLIT, class MAT = BsrDev>
__global__ __launch_bounds__(kBlock) void k_cert_apply(MAT Q, const double* __restrict__ S, const double* __restrict__ W,
                                                       double* __restrict__ CW, double* __restrict__ partials, int n) {
  using GEO = Geo<D, R, SPLIT>;
  __shared__ double sm[kWaves][GEO::G][GEO::T];
  __shared__ double red[kWaves * R * R];
  const LaneId L = lane_id<D, SPLIT>();
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  double part[R * R];
#pragma unroll
  for (int k = 0; k < R * R; ++k) part[k] = 0.0;
  const TileIter ti_ = tile_iter(ntiles);
  for (int tk = ti_.first; tk < ti_.last; tk += ti_.step) {
    const int tile = tile_of(Q, tk);
    const int i = tile * GEO::P + L.wave * GEO::G + L.g;
    const bool okp = (L.g < GEO::G) && (i < n);
    const bool ok = okp && (L.s == 0);
    double h[R], w[R];
    const size_t off = (size_t)i * GEO::T + L.c * R;
    double* ws = ok ? &sm[L.wave][L.g][0] : nullptr;
    q_gather<D, R, SPLIT>(Q, W, i, L.s, L.c, okp, h);
    if (ok) {
      load_col<R>(W + off, w);
      store_col<R>(ws + L.c * R, w);
    }
    wave_sync();
    if (ok) {
      if (L.c < D) {
        // h[:,c] -= sum_a W[:,a] * S[a][c]   (S symmetric: row c of S_i)
#pragma unroll
        for (int a = 0; a < D; ++a) {
          const double sac = S[(size_t)i * D * D + L.c * D + a];
#pragma unroll
          for (int k = 0; k < R; ++k) h[k] = fma(-ws[a * R + k], sac, h[k]);
        }
      }
#pragma unroll
      for (int a = 0; a < R; ++a)
#pragma unroll
        for (int b = 0; b < R; ++b) part[a * R + b] = fma(w[a], h[b], part[a * R + b]);
      store_col<R>(CW + off, h);
    }
    wave_sync();
  }
  block_allreduce<R * R>(part, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < R * R; ++k) partials[(size_t)blockIdx.x * R * R + k] = part[k];
  }
}

// ================================================================ the same product for a TEAM of agents, one launch
// The team's pose vectors are one allocation of N = sum n_a tiles; member a owns the slice [first, first + n) in its own
// internal pose order.  Rows of member a of W C(X):  W_a Q_aa + sum_b W_b Q_ba - W_a,rot Lambda_a, with Q_aa the member's
// own Q (it already carries the diagonal terms of the shared edges), Q_ba its coupling matrix C -- column slot k of C is
// team tile nbr_pose[k], read straight from W: no neighbour buffer, no pack, no exchange -- and Lambda_a the S that k_grad
// cached with the member's G current.  The host's tile table maps every workgroup tile to (member, first local pose): a
// tile lies inside ONE member (a member's last tile is ragged), so everything that selects a matrix is uniform per
// workgroup.  One pose per D+1 lanes; the own-row gather, the coupling blocks in slot order, the S correction: a fixed
// summation order, bitwise reproducible for any grid.  partials as k_cert_apply.
struct CertMember {
  BsrDev Q;                 // n x n block rows of the member
  BsrDev C;                 // n block rows, column slots into nbr_pose
  const int32_t* nbr_pose;  // team tile of every column slot of C
  const double* S;          // the member's Lambda blocks [n, D, D]
  int first, n;
};
struct CertTile {
  int member, p0;  // first local pose of the tile
};
template <int D, int R>
__global__ __launch_bounds__(kBlock) void k_cert_apply_team(const CertMember* __restrict__ members,
                                                            const CertTile* __restrict__ tiles, int ntiles,
                                                            const double* __restrict__ W, double* __restrict__ CW,
                                                            double* __restrict__ partials) {
  using GEO = Geo<D, R, 1>;
  constexpr int B = GEO::B, T = GEO::T, BB = GEO::BB;
  __shared__ double sm[kWaves][GEO::G][GEO::T];
  __shared__ double red[kWaves * R * R];
  const LaneId L = lane_id<D, 1>();
  double part[R * R];
#pragma unroll
  for (int k = 0; k < R * R; ++k) part[k] = 0.0;
  const TileIter ti_ = tile_iter(ntiles);
  for (int tk = ti_.first; tk < ti_.last; tk += ti_.step) {
    const int mi = tiles[tk].member, p0 = tiles[tk].p0;
    const BsrDev Q = members[mi].Q, Cm = members[mi].C;
    const int32_t* __restrict__ nbr = members[mi].nbr_pose;
    const double* __restrict__ S = members[mi].S;
    const int first = members[mi].first, n = members[mi].n;
    const int il = p0 + L.wave * GEO::G + L.g;  // the member's pose
    const bool ok = (L.g < GEO::G) && (il < n);
    const int i = first + il;                   // the team's tile
    double h[R], w[R];
    const size_t off = (size_t)i * T + L.c * R;
    double* ws = ok ? &sm[L.wave][L.g][0] : nullptr;
    q_gather<D, R, 1>(Q, W + (size_t)first * T, il, 0, L.c, ok, h);
    if (ok) {
      // coupling blocks of the row: the other members' tiles, through nbr_pose (spmm_col's arithmetic)
      const int t1 = Cm.rowptr[il + 1];
      for (int t = Cm.rowptr[il]; t < t1; ++t) {
        const double* __restrict__ q = Cm.vals + (size_t)t * BB + L.c * B;
        const double* __restrict__ x = W + (size_t)nbr[Cm.colidx[t]] * T;
        double qk[B];
#pragma unroll
        for (int kk = 0; kk < B; ++kk) qk[kk] = q[kk];
#pragma unroll
        for (int kk = 0; kk < B; ++kk) {
#pragma unroll
          for (int a = 0; a < R; ++a) h[a] = fma(x[kk * R + a], qk[kk], h[a]);
        }
      }
      load_col<R>(W + off, w);
      store_col<R>(ws + L.c * R, w);
    }
    wave_sync();
    if (ok) {
      if (L.c < D) {
#pragma unroll
        for (int a = 0; a < D; ++a) {
          const double sac = S[(size_t)il * D * D + L.c * D + a];
#pragma unroll
          for (int k = 0; k < R; ++k) h[k] = fma(-ws[a * R + k], sac, h[k]);
        }
      }
#pragma unroll
      for (int a = 0; a < R; ++a)
#pragma unroll
        for (int b = 0; b < R; ++b) part[a * R + b] = fma(w[a], h[b], part[a * R + b]);
      store_col<R>(CW + off, h);
    }
    wave_sync();
  }
  block_allreduce<R * R>(part, red);
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < R * R; ++k) partials[(size_t)blockIdx.x * R * R + k] = part[k];
  }
}

// out[k] = X[idx[k]] for pose tiles of T doubles: the neighbour tiles of a member, taken from the team's iterate
static __global__ __launch_bounds__(kBlock) void k_cert_gather_tiles(const double* __restrict__ X,
                                                                     const int32_t* __restrict__ idx, int T, int count,
                                                                     double* __restrict__ out) {
  const size_t total = (size_t)count * T;
  for (size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (size_t)gridDim.x * kBlock) {
    const size_t k = e / T;
    out[e] = X[(size_t)idx[k] * T + (e - k * T)];
  }
}

// ================================================================ Gram blocks  G_p = B_x(p) B_y(p)^T  (R x R each)
// One streaming pass over up to NB blocks: chunks of kCertCols columns of every block are staged in LDS (each chunk of a
// block is one contiguous span of kCertCols * R doubles), then every thread owns whole entries (pair, a, b) of the
// result and sums over the chunk's columns.  partials[blockIdx.x * E + e], E = npairs * R * R.
template <int D, int R, int NB>
__global__ __launch_bounds__(kBlock) void k_cert_gram(CertIn in, int nb, CertPairs pr, int npairs,
                                                      double* __restrict__ partials, int n) {
  static_assert(NB <= kCertMaxBlocks, "too many blocks");
  constexpr int CH = kCertCols * R;
  constexpr int EPT = (kCertMaxPairs * R * R + kBlock - 1) / kBlock;  // entries per thread
  __shared__ double lds[NB][CH];
  const int E = npairs * R * R;
  const size_t total = (size_t)n * (D + 1) * R;
  const size_t nchunks = ((size_t)n * (D + 1) + kCertCols - 1) / kCertCols;
  double acc[EPT];
  int ex[EPT], ey[EPT];
#pragma unroll
  for (int t = 0; t < EPT; ++t) {
    acc[t] = 0.0;
    const int e = threadIdx.x + t * kBlock;
    const int p = e / (R * R), ab = e - p * R * R;
    const bool ok = e < E;
    ex[t] = ok ? (int)pr.x[p] * CH + ab / R : -1;  // offset of (block, row a) in lds
    ey[t] = ok ? (int)pr.y[p] * CH + ab % R : -1;
  }
  for (size_t ch = blockIdx.x; ch < nchunks; ch += gridDim.x) {
    const size_t base = ch * CH;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (j < nb) {
        const double* src = in.b[j];
        for (int e = threadIdx.x; e < CH; e += kBlock) lds[j][e] = (base + e < total) ? src[base + e] : 0.0;
      }
    }
    __syncthreads();
    const double* l0 = &lds[0][0];
#pragma unroll
    for (int t = 0; t < EPT; ++t) {
      if (ex[t] >= 0) {
        double s = acc[t];
        for (int c = 0; c < kCertCols; ++c) s = fma(l0[ex[t] + c * R], l0[ey[t] + c * R], s);
        acc[t] = s;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < EPT; ++t) {
    const int e = threadIdx.x + t * kBlock;
    if (e < E) partials[(size_t)blockIdx.x * E + e] = acc[t];
  }
}

// fixed-order sum of per-workgroup partials: out[e] = sum_{w < nwg} partials[w * E + e]
static __global__ __launch_bounds__(kBlock) void k_cert_reduce(const double* __restrict__ partials, int nwg, int E,
                                                        double* __restrict__ out) {
  for (int e = blockIdx.x * kBlock + threadIdx.x; e < E; e += gridDim.x * kBlock) {
    double s = 0.0;
    for (int w = 0; w < nwg; ++w) s += partials[(size_t)w * E + e];
    out[e] = s;
  }
}

// ================================================================ per-pose linear combinations
// out_k = sum_j M_jk^T B_j   (r x r coefficients, r-row blocks): column-wise, out_k[col][b] = sum_j sum_a M[k][j][a][b]
// B_j[col][a].  M: device, [nout][nb][R][R].  One thread per column reads its column of every input before it writes: an output may be one of the inputs.
template <int D, int R, int NB>
__global__ __launch_bounds__(kBlock) void k_cert_combine(CertIn in, int nb, CertOut out, int nout,
                                                         const double* __restrict__ M, int n) {
  static_assert(NB <= kCertMaxBlocks, "too many blocks");
  const size_t ncol = (size_t)n * (D + 1);
  for (size_t col = (size_t)blockIdx.x * kBlock + threadIdx.x; col < ncol; col += (size_t)gridDim.x * kBlock) {
    double v[NB][R];
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      if (j < nb) {
        load_col<R>(in.b[j] + col * R, v[j]);
      } else {
#pragma unroll
        for (int a = 0; a < R; ++a) v[j][a] = 0.0;
      }
    }
    for (int k = 0; k < nout; ++k) {
      double o[R];
#pragma unroll
      for (int b = 0; b < R; ++b) o[b] = 0.0;
      const double* Mk = M + (size_t)k * nb * R * R;
#pragma unroll
      for (int j = 0; j < NB; ++j) {
        if (j < nb) {
#pragma unroll
          for (int a = 0; a < R; ++a)
#pragma unroll
            for (int b = 0; b < R; ++b) o[b] = fma(Mk[(j * R + a) * R + b], v[j][a], o[b]);
        }
      }
      store_col<R>(out.b[k] + col * R, o);
    }
  }
}

// ================================================================ block-Jacobi without tangent projection: Z = V Dinv
template <int D, int R>
__global__ __launch_bounds__(kBlock) void k_cert_jacobi(const double* __restrict__ V, const double* __restrict__ dinv,
                                                        double* __restrict__ Z, int n) {
  using GEO = Geo<D, R>;
  __shared__ double sm[kWaves][GEO::G][GEO::T];
  const LaneId L = lane_id<D>();
  const int ntiles = (n + GEO::P - 1) / GEO::P;
  const TileIter ti_ = tile_iter(ntiles);
  for (int tile = ti_.first; tile < ti_.last; tile += ti_.step) {
    const int i = tile * GEO::P + L.wave * GEO::G + L.g;
    const bool ok = (L.g < GEO::G) && (i < n);
    const size_t off = (size_t)i * GEO::T + L.c * R;
    double* vs = ok ? &sm[L.wave][L.g][0] : nullptr;
    if (ok) {
      double v[R];
      load_col<R>(V + off, v);
      store_col<R>(vs + L.c * R, v);
    }
    wave_sync();
    if (ok) {
      double z[R];
      jacobi_col<D, R>(vs, dinv + (size_t)i * GEO::BB + L.c * GEO::B, z);
      store_col<R>(Z + off, z);
    }
    wave_sync();
  }
}

// ================================================================ set-up pieces
// seeded start block: a hash of (seed, element index) mapped to [-1, 1) -- independent of the launch geometry
template <int D, int R>
__global__ __launch_bounds__(kBlock) void k_cert_random(unsigned long long seed, double* __restrict__ W, int n) {
  const size_t total = (size_t)n * (D + 1) * R;
  for (size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (size_t)gridDim.x * kBlock) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(e + 1);  // splitmix64
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    W[e] = (double)(z >> 11) * (2.0 / 9007199254740992.0) - 1.0;
  }
}

// the translation indicator t = (0_D, 1) of every pose in row 0 of a block (rows 1 .. R-1 zero)
template <int D, int R>
__global__ __launch_bounds__(kBlock) void k_cert_indicator(double* __restrict__ W, int n) {
  const size_t total = (size_t)n * (D + 1) * R;
  for (size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (size_t)gridDim.x * kBlock) {
    const size_t col = e / R;
    W[e] = ((e % R) == 0 && (col % (D + 1)) == D) ? 1.0 : 0.0;
  }
}

// scale = max_i max diag(Q_ii): per-workgroup maxima (one thread per pose), the host takes the max of those
template <int D>
__global__ __launch_bounds__(kBlock) void k_cert_scale(BsrDev Q, double* __restrict__ out, int n) {
  constexpr int B = D + 1;
  __shared__ double red[kBlock];
  const int i = blockIdx.x * kBlock + threadIdx.x;
  double m = 0.0;
  if (i < n) {
    for (int t = Q.rowptr[i]; t < Q.rowptr[i + 1]; ++t) {
      if (Q.colidx[t] == i) {
#pragma unroll
        for (int k = 0; k < B; ++k) m = fmax(m, Q.vals[(size_t)t * B * B + k * B + k]);
      }
    }
  }
  red[threadIdx.x] = m;
  __syncthreads();
  for (int s = kBlock / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s) red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + s]);
    __syncthreads();
  }
  if (threadIdx.x == 0) out[blockIdx.x] = red[0];
}

// ================================================================ lift to rank R + 1 along a witness
// Xl = [X; alpha v^T]: [n, D+1, R] -> [n, D+1, R+1], v = (D+1) n doubles in pose-major order (one tile column per entry).
// k_retract<D, R+1> then maps Xl onto the manifold.
template <int D, int R>
__global__ __launch_bounds__(kBlock) void k_cert_lift(const double* __restrict__ X, const double* __restrict__ v,
                                                      double alpha, double* __restrict__ Xl, int n) {
  const size_t ncol = (size_t)n * (D + 1);
  for (size_t col = (size_t)blockIdx.x * kBlock + threadIdx.x; col < ncol; col += (size_t)gridDim.x * kBlock) {
#pragma unroll
    for (int a = 0; a < R; ++a) Xl[col * (R + 1) + a] = X[col * R + a];
    Xl[col * (R + 1) + R] = alpha * v[col];
  }
}
