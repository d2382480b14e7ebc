// G = U^T U of the global stage: weighted tile bases and compacted rows, the dense form (pmd_gram_u, R <= frames), the
// block-sparse form and its product with a right matrix (pmd_gram_blocks, pmd_gram_apply, R > frames), and the CSR
// assembly of the sparse spatial matrix.  Everything here is hand-written; the tile-pair and tile x background sums are
// written once and stored by a dense and a block kernel each.
#include "pmd_internal.h"
#include <algorithm>

// ---------------------------------------------------------------- weighted tile bases ------
// Uw[tile][c][q] = Ut[tile][c][q] * w[q] / cumw[pix[tile][q]] for c < ranks[tile], else 0
// (decomposition.py:812-816, :847-853).
__global__ void weight_tiles_kernel(const float* __restrict__ Ut, long tile_stride, int ld, const int* __restrict__ pix,
                                    int d, const float* __restrict__ w, const float* __restrict__ cumw,
                                    const int* __restrict__ ranks, float* __restrict__ Uw) {
  const int tile = blockIdx.y;
  const int rk = ranks[tile];
  // every one of the 64 x ld entries is written: the padding feeds MFMA operands (0 * x must be 0)
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < PMD_RPAD * ld; i += gridDim.x * blockDim.x) {
    const int c = i / ld, q = i - c * ld;
    float v = 0.f;
    if (c < rk && q < d) v = Ut[(long)tile * tile_stride + (long)c * ld + q] * w[q] / cumw[pix[(long)tile * d + q]];
    Uw[(long)tile * tile_stride + (long)c * ld + q] = v;
  }
}

extern "C" int pmd_weight_tiles(pmd_ctx* ctx, const float* Ut, int dpad, const int* pix, int d, const float* w,
                                const float* cumw, const int* ranks, float* Uw, int n_tiles) {
  CTX_CHECK(ctx);
  pmd_prof_scope prof__(ctx, "weight_tiles");
  for (int t0 = 0; t0 < n_tiles; t0 += 32768) {
    const int tn = (n_tiles - t0 < 32768) ? n_tiles - t0 : 32768;
    hipLaunchKernelGGL(weight_tiles_kernel, dim3(32, tn), dim3(256), 0, ctx->stream, Ut + (long)t0 * 64 * dpad,
                       64L * dpad, dpad, pix + (long)t0 * d, d, w, cumw, ranks + t0, Uw + (long)t0 * 64 * dpad);
    PMD_LAUNCH_CHECK(ctx, "weight_tiles_kernel");
  }
  return PMD_OK;
}

// Z[col_off[tile] + c][t] = Out[tile][c][t], c < ranks[tile]
__global__ void compact_rows_kernel(const float* __restrict__ Out, long tile_stride, long ldo,
                                    const int* __restrict__ col_off, const int* __restrict__ ranks, int T,
                                    float* __restrict__ Z, long ldz) {
  const int tile = blockIdx.y;
  const int rk = ranks[tile];
  const long off = col_off[tile];
  for (int c = 0; c < rk; ++c)
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < T; t += gridDim.x * blockDim.x)
      Z[(off + c) * ldz + t] = Out[(long)tile * tile_stride + (long)c * ldo + t];
}

extern "C" int pmd_compact_rows(pmd_ctx* ctx, const float* Out, long ldo, const int* col_off, const int* ranks, int T,
                                float* Z, long ldz, int n_tiles) {
  CTX_CHECK(ctx);
  const long tile_stride = 64L * ldo;
  pmd_prof_scope prof__(ctx, "compact_rows");
  for (int t0 = 0; t0 < n_tiles; t0 += 32768) {
    const int tn = (n_tiles - t0 < 32768) ? n_tiles - t0 : 32768;
    hipLaunchKernelGGL(compact_rows_kernel, dim3(16, tn), dim3(256), 0, ctx->stream, Out + (long)t0 * tile_stride,
                       tile_stride, ldo, col_off + t0, ranks + t0, T, Z, ldz);
    PMD_LAUNCH_CHECK(ctx, "compact_rows_kernel");
  }
  return PMD_OK;
}

// ---------------------------------------------------------------- G = U^T U ----------------
// pairs[p] = (tile a, tile b, i0, i1, j0, j1): overlap rectangle in FOV coordinates.  origins[tile] = (k, j).
// acc[a][b] = sum over the rectangle of tile a's component 4 ti + a times tile b's component 4 tj + b (pa, pb: the tiles'
// rows of Uw; oa, ob: their origins; ti, tj = threadIdx.x / 16, % 16), in fp64, 64 pixels at a time through LDS.  All zero
// when a rank is zero.
__device__ __forceinline__ void gram_pair_accumulate(const float* pa, const float* pb, int ra, int rb, int dpad, int b1,
                                                     const int* rect, const int* oa, const int* ob, int ti, int tj, double (&acc)[4][4]) {
  __shared__ float ua[64][65];
  __shared__ float ub[64][65];
  const int i0 = rect[0], i1 = rect[1], j0 = rect[2], j1 = rect[3];
  const int ka = oa[0], ja = oa[1], kb = ob[0], jb = ob[1];
  const int h = i1 - i0, npix = h * (j1 - j0);
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = 0.0;
  if (ra == 0 || rb == 0) return;
  for (int p0 = 0; p0 < npix; p0 += 64) {
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
      const int c = i >> 6, pl = i & 63;
      const int p = p0 + pl;
      float va = 0.f, vb = 0.f;
      if (p < npix) {
        const int jj = p / h, ii = p - jj * h;
        const int gi = i0 + ii, gj = j0 + jj;
        if (c < ra) va = pa[(long)c * dpad + (gi - ka) + b1 * (gj - ja)];
        if (c < rb) vb = pb[(long)c * dpad + (gi - kb) + b1 * (gj - jb)];
      }
      ua[c][pl] = va;
      ub[c][pl] = vb;
    }
    __syncthreads();
#pragma unroll 4
    for (int pl = 0; pl < 64; ++pl) {
      double av[4], bv[4];
#pragma unroll
      for (int a = 0; a < 4; ++a) { av[a] = (double)ua[4 * ti + a][pl]; bv[a] = (double)ub[4 * tj + a][pl]; }
#pragma unroll
      for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) acc[a][b] = fma(av[a], bv[b], acc[a][b]);
    }
    __syncthreads();
  }
}

// Dense form: writes G[off_a + c][off_b + c'] and its transpose.
__global__ __launch_bounds__(256) void gram_pairs_kernel(const float* __restrict__ Uw, int dpad, int b1,
                                                         const int* __restrict__ pairs, const int* __restrict__ origins,
                                                         const int* __restrict__ col_off, const int* __restrict__ ranks,
                                                         float* __restrict__ G, long ldg) {
  const int* pr = pairs + (long)blockIdx.x * 6;
  const int ta = pr[0], tb = pr[1];
  const int ra = ranks[ta], rb = ranks[tb];
  if (ra == 0 || rb == 0) return;
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;   // this thread's 4 x 4 entries of the 64 x 64 block
  double acc[4][4];
  gram_pair_accumulate(Uw + (long)ta * 64 * dpad, Uw + (long)tb * 64 * dpad, ra, rb, dpad, b1, pr + 2, origins + 2 * ta,
                       origins + 2 * tb, ti, tj, acc);
  const long oa = col_off[ta], ob = col_off[tb];
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int c = 4 * ti + a, cp = 4 * tj + b;
      if (c < ra && cp < rb) {
        const float v = (float)acc[a][b];
        G[(oa + c) * ldg + ob + cp] = v;
        G[(ob + cp) * ldg + oa + c] = v;
      }
    }
}

// tile x background: sum_q Uw[tile][c][q] * basis[pix[tile][q]][k] in fp64 (urow: row c of the tile, pixt: its pixel
// list, kstride: columns per pixel of the basis)
__device__ __forceinline__ float gram_bg_dot(const float* __restrict__ urow, const int* __restrict__ pixt, int d,
                                             const float* __restrict__ basis, int kstride, int k) {
  double s = 0.0;
  for (int q = 0; q < d; ++q) s += (double)urow[q] * (double)basis[(long)pixt[q] * kstride + k];
  return (float)s;
}

// Dense form: G[off + c][Rt + k] and its transpose.
__global__ __launch_bounds__(256) void gram_bg_kernel(const float* __restrict__ Uw, int dpad, int d,
                                                      const int* __restrict__ pix, const float* __restrict__ basis,
                                                      int K, const int* __restrict__ col_off,
                                                      const int* __restrict__ ranks, int Rt, float* __restrict__ G,
                                                      long ldg) {
  const int tile = blockIdx.x;
  const int rk = ranks[tile];
  const long off = col_off[tile];
  for (int i = threadIdx.x; i < rk * K; i += 256) {
    const int c = i / K, k = i - c * K;
    const float v = gram_bg_dot(Uw + (long)tile * 64 * dpad + (long)c * dpad, pix + (long)tile * d, d, basis, K, k);
    G[(off + c) * ldg + Rt + k] = v;
    G[(long)(Rt + k) * ldg + off + c] = v;
  }
}

// background x background, one workgroup per entry, into the K rows Gstrip (columns Rt ... Rt + K) that hold the
// background's rows of G: the strip of the block form, or rows Rt ... of the dense G
__global__ __launch_bounds__(256) void gram_bgbg_strip_kernel(const float* __restrict__ basis, long D, int K, int Rt,
                                                              float* __restrict__ Gstrip, long ldgs) {
  __shared__ double red[256];
  const int k1 = blockIdx.x, k2 = blockIdx.y;
  if (k2 < k1) return;
  double s = 0.0;
  for (long c = threadIdx.x; c < D; c += 256) s += (double)basis[c * K + k1] * (double)basis[c * K + k2];
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    Gstrip[(long)k1 * ldgs + Rt + k2] = (float)red[0];
    Gstrip[(long)k2 * ldgs + Rt + k1] = (float)red[0];
  }
}

extern "C" int pmd_gram_u(pmd_ctx* ctx, const float* Uw, int dpad, int b1, int b2, const int* pix, const int* pairs,
                          int n_pairs, const int* origins, const int* col_off, const int* ranks, int n_tiles, int Rt,
                          const float* basis, long D, int K, float* G, long ldg) {
  CTX_CHECK(ctx);
  pmd_prof_scope prof__(ctx, "gram_u");
  const long R = Rt + K;
  PMD_HIP(ctx, hipMemsetAsync(G, 0, (size_t)R * ldg * sizeof(float), ctx->stream));
  if (n_pairs > 0) {
    hipLaunchKernelGGL(gram_pairs_kernel, dim3(n_pairs), dim3(256), 0, ctx->stream, Uw, dpad, b1, pairs, origins,
                       col_off, ranks, G, ldg);
    PMD_LAUNCH_CHECK(ctx, "gram_pairs_kernel");
  }
  if (K > 0) {
    hipLaunchKernelGGL(gram_bg_kernel, dim3(n_tiles), dim3(256), 0, ctx->stream, Uw, dpad, b1 * b2, pix, basis, K,
                       col_off, ranks, Rt, G, ldg);
    PMD_LAUNCH_CHECK(ctx, "gram_bg_kernel");
    hipLaunchKernelGGL(gram_bgbg_strip_kernel, dim3(K, K), dim3(256), 0, ctx->stream, basis, D, K, Rt, G + (long)Rt * ldg, ldg);
    PMD_LAUNCH_CHECK(ctx, "gram_bgbg_strip_kernel");
  }
  return PMD_OK;
}

// =============================================================================================
// Block-sparse form of G = U^T U (used when the right matrix is not the identity, i.e. R > frames:
// decomposition.py:976-981).  G is never densified: tile pairs give 64x64 blocks, the background
// columns give one 64x64 block per tile plus a dense K x Rc strip.
// =============================================================================================

// Gblk[p][c][c'] = sum over the overlap of pair p of Uw[a][c][.] * Uw[b][c'][.]   (a <= b), zero beyond the ranks
__global__ __launch_bounds__(256) void gram_pair_blocks_kernel(const float* __restrict__ Uw, int dpad, int b1,
                                                               const int* __restrict__ pairs,
                                                               const int* __restrict__ origins,
                                                               const int* __restrict__ ranks,
                                                               float* __restrict__ Gblk) {
  const int* pr = pairs + (long)blockIdx.x * 6;
  const int ta = pr[0], tb = pr[1];
  const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;   // this thread's 4 x 4 entries of the 64 x 64 block
  double acc[4][4];
  gram_pair_accumulate(Uw + (long)ta * 64 * dpad, Uw + (long)tb * 64 * dpad, ranks[ta], ranks[tb], dpad, b1, pr + 2,
                       origins + 2 * ta, origins + 2 * tb, ti, tj, acc);
  float* g = Gblk + (long)blockIdx.x * 4096;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) g[(4 * ti + a) * 64 + 4 * tj + b] = (float)acc[a][b];
}

// Gbg[tile][c][k] = sum_q Uw[tile][c][q] * basis[pix[q]][k]; also scattered into the dense strip
// Gstrip[k][off + c] (K x ldgs).
__global__ __launch_bounds__(256) void gram_bg_blocks_kernel(const float* __restrict__ Uw, int dpad, int d,
                                                             const int* __restrict__ pix,
                                                             const float* __restrict__ basis, int K,
                                                             const int* __restrict__ col_off,
                                                             const int* __restrict__ ranks, float* __restrict__ Gbg,
                                                             float* __restrict__ Gstrip, long ldgs, int kstride) {
  const int tile = blockIdx.x;
  const int rk = ranks[tile];
  const long off = col_off[tile];
  for (int i = threadIdx.x; i < 64 * 64; i += 256) {
    const int c = i >> 6, k = i & 63;
    float v = 0.f;
    if (c < rk && k < K) {
      v = gram_bg_dot(Uw + (long)tile * 64 * dpad + (long)c * dpad, pix + (long)tile * d, d, basis, kstride, k);
      Gstrip[(long)k * ldgs + off + c] = v;
    }
    Gbg[(long)tile * 4096 + i] = v;
  }
}

// GM[off_a + c][x] = sum over neighbour blocks (b, c') of G_ab[c][c'] * M[off_b + c'][x]
// nbr_ptr[a] .. nbr_ptr[a+1]: entries (row offset of the block's M rows, rows in the block,
// block index into Gblk/Gbg, flags: bit0 = use the transposed block, bit1 = background block).
template <int NOUT>
__global__ __launch_bounds__(256) void gram_apply_kernel(const float* __restrict__ Gblk, const float* __restrict__ Gbg,
                                                         const int* __restrict__ nbr_ptr, const int* __restrict__ nbr,
                                                         const int* __restrict__ col_off, const int* __restrict__ ranks,
                                                         const float* __restrict__ M, long ldm, int ncols,
                                                         float* __restrict__ GM, long ldgm) {
  __shared__ float g[64][NOUT + 1];  // g[c'][c]
  const int a = blockIdx.y;
  const int ra = ranks[a];
  if (ra == 0) return;
  const int x = blockIdx.x * 256 + threadIdx.x;
  // fp32 accumulation over the few hundred terms of a block row: the product feeds fp32 GEMMs
  // (the reference rounds its float64 U^T U v to float32 at decomposition.py:982)
  float acc[NOUT];
#pragma unroll
  for (int c = 0; c < NOUT; ++c) acc[c] = 0.f;
  for (int e = nbr_ptr[a]; e < nbr_ptr[a + 1]; ++e) {
    const int row0 = nbr[4 * e], rb = nbr[4 * e + 1], blk = nbr[4 * e + 2], flags = nbr[4 * e + 3];
    const float* src = (flags & 2) ? Gbg + (long)blk * 4096 : Gblk + (long)blk * 4096;
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * NOUT; i += 256) {
      const int cp = i / NOUT, c = i - cp * NOUT;
      // stored block is [row-tile comp][col-tile comp]; transposed flag: this tile is the column tile
      g[cp][c] = src[(flags & 1) ? cp * 64 + c : c * 64 + cp];
    }
    __syncthreads();
    // eight rows of M in flight per thread (unconditional loads on clamped indices), FMAs only for the
    // 8-column groups below this tile's rank
    const long xc = (x < ncols) ? x : ncols - 1;
    for (int cp0 = 0; cp0 < rb; cp0 += 8) {
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = M[(long)(row0 + ((cp0 + u < rb) ? cp0 + u : rb - 1)) * ldm + xc];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        if (cp0 + u < rb) {
#pragma unroll
          for (int c0 = 0; c0 < NOUT; c0 += 8) {
            if (c0 < ra) {
#pragma unroll
              for (int c = c0; c < c0 + 8; ++c) acc[c] = fmaf(g[cp0 + u][c], v[u], acc[c]);
            }
          }
        }
      }
    }
  }
  if (x < ncols) {
    const long off = col_off[a];
#pragma unroll
    for (int c = 0; c < NOUT; ++c)
      if (c < ra) GM[(off + c) * ldgm + x] = acc[c];
  }
}

// The same product on the fp32 MFMA path: a workgroup owns tile a x 256 columns (a wave 64 of them).  Per neighbour
// block the (rank-masked) G block goes through LDS as the A operand (m = component of tile a, k = component of the
// neighbour), a lane's float4 of M row cp0 + k is the B operand of four N tiles at once (N tile s = columns
// 4 n + s: the permutation is undone by the float4 store of the four accumulators).  16 x CT x 4 accumulators.
typedef float ga_f32x4 __attribute__((ext_vector_type(4)));
constexpr int GA_LD = 80;  // g[cp][c] row length: 80 = 16 mod 64, the four k rows of a fragment hit disjoint banks

template <int CT>
__global__ __launch_bounds__(256) void gram_apply_mfma_kernel(const float* __restrict__ Gblk, const float* __restrict__ Gbg,
                                                              const int* __restrict__ nbr_ptr, const int* __restrict__ nbr,
                                                              const int* __restrict__ col_off, const int* __restrict__ ranks,
                                                              const float* __restrict__ M, long ldm, int ncols,
                                                              float* __restrict__ GM, long ldgm) {
  __shared__ float g[64][GA_LD];
  const int a = blockIdx.y;
  const int ra = ranks[a];
  if (ra == 0) return;
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (uniform, and known to be)
  const int n16 = lane & 15, kk = lane >> 4;
  const int x0 = blockIdx.x * 256 + wave * 64 + 4 * n16;
  const long xc = (x0 + 3 < ldm) ? x0 : 0;  // idle lanes read valid columns; their results are not stored
  ga_f32x4 acc[CT][4];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int sx = 0; sx < 4; ++sx) acc[ct][sx] = (ga_f32x4){0.f, 0.f, 0.f, 0.f};
  for (int e = nbr_ptr[a]; e < nbr_ptr[a + 1]; ++e) {
    const int row0 = nbr[4 * e], rb = nbr[4 * e + 1], blk = nbr[4 * e + 2], flags = nbr[4 * e + 3];
    const float* src = (flags & 2) ? Gbg + (long)blk * 4096 : Gblk + (long)blk * 4096;
    __syncthreads();
    // (only the part the MFMAs below read: cp < round_up(rb, 16), c < round_up(ra, 16); consecutive threads read
    // consecutive addresses of the stored block in either orientation)
    const int cpn = (rb + 15) & ~15, cn = (ra + 15) & ~15;
    if (flags & 1) {
      for (int i = threadIdx.x; i < cpn * cn; i += 256) {
        const int cp = i / cn, c = i - cp * cn;
        const float v = src[cp * 64 + c];
        g[cp][c] = (cp < rb && c < ra) ? v : 0.f;  // masked: rows / columns beyond the ranks hold other tiles' data
      }
    } else {
      for (int i = threadIdx.x; i < cpn * cn; i += 256) {
        const int c = i / cpn, cp = i - c * cpn;
        const float v = src[c * 64 + cp];
        g[cp][c] = (cp < rb && c < ra) ? v : 0.f;
      }
    }
    __syncthreads();
    // 16 rows of M (four k steps) per batch, all four loads in flight at once, unconditional (rows clamped into the
    // block; the masked G makes their contribution zero)
    const float* mp = M + (long)row0 * ldm + xc;
    for (int cp0 = 0; cp0 < rb; cp0 += 16) {
      ga_f32x4 b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) b[u] = *reinterpret_cast<const ga_f32x4*>(mp + (long)min(cp0 + 4 * u + kk, rb - 1) * ldm);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        if (cp0 + 4 * u < rb) {  // workgroup-uniform
#pragma unroll
          for (int ct = 0; ct < CT; ++ct) {
            if (16 * ct < ra) {  // workgroup-uniform: component tiles beyond this tile's rank are skipped
              const float av = g[cp0 + 4 * u + kk][16 * ct + n16];
#pragma unroll
              for (int sx = 0; sx < 4; ++sx) acc[ct][sx] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, b[u][sx], acc[ct][sx], 0, 0, 0);
            }
          }
        }
      }
    }
  }
  if (x0 >= ncols) return;
  const long off = col_off[a];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = 16 * ct + 4 * kk + i;
      if (c >= ra) continue;
      float* o = GM + (off + c) * ldgm + x0;
      if (x0 + 3 < ncols) {
        *reinterpret_cast<ga_f32x4*>(o) = (ga_f32x4){acc[ct][0][i], acc[ct][1][i], acc[ct][2][i], acc[ct][3][i]};
      } else {
        for (int sx = 0; sx < 4 && x0 + sx < ncols; ++sx) o[sx] = acc[ct][sx][i];
      }
    }
}

// blocks: Gblk [n_pairs][64][64], Gbg [n_tiles][64][64], Gstrip [K][ldgs] (ldgs >= Rt + K)
extern "C" int pmd_gram_blocks(pmd_ctx* ctx, const float* Uw, int dpad, int b1, int b2, const int* pix,
                               const int* pairs, int n_pairs, const int* origins, const int* col_off, const int* ranks,
                               int n_tiles, int Rt, const float* basis, long D, int K, float* Gblk, float* Gbg,
                               float* Gstrip, long ldgs) {
  CTX_CHECK(ctx);
  pmd_prof_scope prof__(ctx, "gram_blocks");
  if (n_pairs > 0) {
    hipLaunchKernelGGL(gram_pair_blocks_kernel, dim3(n_pairs), dim3(256), 0, ctx->stream, Uw, dpad, b1, pairs, origins,
                       ranks, Gblk);
    PMD_LAUNCH_CHECK(ctx, "gram_pair_blocks_kernel");
  }
  if (K > 0) {
    PMD_HIP(ctx, hipMemsetAsync(Gstrip, 0, (size_t)K * ldgs * sizeof(float), ctx->stream));
    // Gbg: [K block of 64][tile][64][64] (one block of 64 background columns per launch)
    for (int k0 = 0; k0 < K; k0 += 64) {
      const int kc = (K - k0 < 64) ? K - k0 : 64;
      hipLaunchKernelGGL(gram_bg_blocks_kernel, dim3(n_tiles), dim3(256), 0, ctx->stream, Uw, dpad, b1 * b2, pix, basis + k0, kc,
                         col_off, ranks, Gbg + (long)(k0 / 64) * n_tiles * 4096, Gstrip + (long)k0 * ldgs, ldgs, K);
      PMD_LAUNCH_CHECK(ctx, "gram_bg_blocks_kernel");
    }
    hipLaunchKernelGGL(gram_bgbg_strip_kernel, dim3(K, K), dim3(256), 0, ctx->stream, basis, D, K, Rt, Gstrip, ldgs);
    PMD_LAUNCH_CHECK(ctx, "gram_bgbg_strip_kernel");
  }
  return PMD_OK;
}

// GM = G M for the block-sparse G (rows of the K background columns via one small GEMM).
extern "C" int pmd_gram_apply(pmd_ctx* ctx, const float* Gblk, const float* Gbg, const float* Gstrip, long ldgs,
                              const int* nbr_ptr, const int* nbr, const int* col_off, const int* ranks, int n_tiles,
                              int Rt, int K, int max_rank, const float* M, long ldm, int ncols, float* GM, long ldgm) {
  CTX_CHECK(ctx);
  {
    pmd_prof_scope prof__(ctx, "gram_apply");
    dim3 grid((ncols + 255) / 256, n_tiles);
    const bool mfma_ok = ctx->routes.gram_apply_mfma && ldm % 4 == 0 && ldgm % 4 == 0 && ((uintptr_t)M & 15) == 0 &&
                         ((uintptr_t)GM & 15) == 0 && max_rank <= 64;
    if (mfma_ok) {
      const int ct = (max_rank + 15) / 16;
#define GA_LAUNCH(CT_)                                                                                                   \
  hipLaunchKernelGGL(gram_apply_mfma_kernel<CT_>, grid, dim3(256), 0, ctx->stream, Gblk, Gbg, nbr_ptr, nbr, col_off, ranks, \
                     M, ldm, ncols, GM, ldgm)
      if (ct <= 1) GA_LAUNCH(1);
      else if (ct == 2) GA_LAUNCH(2);
      else if (ct == 3) GA_LAUNCH(3);
      else GA_LAUNCH(4);
#undef GA_LAUNCH
    } else if (max_rank <= 16)
      hipLaunchKernelGGL(gram_apply_kernel<16>, grid, dim3(256), 0, ctx->stream, Gblk, Gbg, nbr_ptr, nbr, col_off, ranks,
                         M, ldm, ncols, GM, ldgm);
    else if (max_rank <= 32)
      hipLaunchKernelGGL(gram_apply_kernel<32>, grid, dim3(256), 0, ctx->stream, Gblk, Gbg, nbr_ptr, nbr, col_off, ranks,
                         M, ldm, ncols, GM, ldgm);
    else
      hipLaunchKernelGGL(gram_apply_kernel<64>, grid, dim3(256), 0, ctx->stream, Gblk, Gbg, nbr_ptr, nbr, col_off, ranks,
                         M, ldm, ncols, GM, ldgm);
    PMD_LAUNCH_CHECK(ctx, "gram_apply_kernel");
  }
  if (K > 0) RUN(pmd_gemm_rm(ctx, 0, 0, K, ncols, Rt + K, 1.f, Gstrip, ldgs, M, ldm, 0.f, GM + (long)Rt * ldgm, ldgm));
  return PMD_OK;
}

// =============================================================================================
// CSR assembly of the sparse spatial matrix on the device (decomposition.py:812-853, :929-930):
// row p (output pixel order) holds, for every covering tile in tile order, rank_t entries
// (float64(U) * w) * (1/cumw), then the K background entries.  cover1[i][0..3] / cover2[j][0..3]
// list the indices of the tile-row / tile-column origins covering FOV row i / column j (-1 pads).
// =============================================================================================
__device__ __forceinline__ void csr_pixel(long p, int d1, int d2, int order_f, int* i, int* j) {
  if (order_f) { *j = (int)(p / d1); *i = (int)(p - (long)(*j) * d1); }
  else { *i = (int)(p / d2); *j = (int)(p - (long)(*i) * d2); }
}

__global__ void csr_count_kernel(int d1, int d2, int order_f, const int* __restrict__ cover1,
                                 const int* __restrict__ cover2, int n2, const int* __restrict__ ranks, int K,
                                 long* __restrict__ row_nnz) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (long)d1 * d2) return;
  int i, j;
  csr_pixel(p, d1, d2, order_f, &i, &j);
  long n = K;
  for (int a = 0; a < 4; ++a) {
    const int ki = cover1[4 * i + a];
    if (ki < 0) continue;
    for (int b = 0; b < 4; ++b) {
      const int ji = cover2[4 * j + b];
      if (ji >= 0) n += ranks[ki * n2 + ji];
    }
  }
  row_nnz[p] = n;
}

__global__ void csr_fill_kernel(int d1, int d2, int order_f, int b1, const int* __restrict__ cover1,
                                const int* __restrict__ cover2, const int* __restrict__ orig1,
                                const int* __restrict__ orig2, int n2, const int* __restrict__ ranks,
                                const int* __restrict__ col_off, const float* __restrict__ Ut, int dpad,
                                const float* __restrict__ w, const double* __restrict__ inv_cumw,
                                const float* __restrict__ basis, int K, int Rt, const long* __restrict__ indptr,
                                double* __restrict__ data, int* __restrict__ indices, int* __restrict__ zero_count, int rpad) {
  const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (long)d1 * d2) return;
  int i, j;
  csr_pixel(p, d1, d2, order_f, &i, &j);
  long pos = indptr[p];
  const double inv = inv_cumw[(long)i * d2 + j];
  int zeros = 0;
  for (int a = 0; a < 4; ++a) {
    const int ki = cover1[4 * i + a];
    if (ki < 0) continue;
    for (int b = 0; b < 4; ++b) {
      const int ji = cover2[4 * j + b];
      if (ji < 0) continue;
      const int tile = ki * n2 + ji;
      const int q = (i - orig1[ki]) + b1 * (j - orig2[ji]);
      const double wq = (double)w[q];
      const int rk = ranks[tile];
      const int off = col_off[tile];
      for (int c = 0; c < rk; ++c) {
        const double v = ((double)Ut[(long)tile * rpad * dpad + (long)c * dpad + q] * wq) * inv;
        zeros += (v == 0.0);
        data[pos] = v;
        indices[pos] = off + c;
        ++pos;
      }
    }
  }
  for (int k = 0; k < K; ++k) {
    const double v = (double)basis[((long)i * d2 + j) * K + k];
    zeros += (v == 0.0);
    data[pos] = v;
    indices[pos] = Rt + k;
    ++pos;
  }
  if (zeros) atomicAdd(zero_count, zeros);
}

extern "C" int pmd_csr_count(pmd_ctx* ctx, int d1, int d2, int order_f, const int* cover1, const int* cover2, int n2,
                             const int* ranks, int K, long* row_nnz) {
  CTX_CHECK(ctx);
  pmd_prof_scope prof__(ctx, "csr_assembly");
  const long D = (long)d1 * d2;
  hipLaunchKernelGGL(csr_count_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, ctx->stream, d1, d2, order_f,
                     cover1, cover2, n2, ranks, K, row_nnz);
  PMD_LAUNCH_CHECK(ctx, "csr_count_kernel");
  return PMD_OK;
}

extern "C" int pmd_csr_fill(pmd_ctx* ctx, int d1, int d2, int order_f, int b1, const int* cover1, const int* cover2,
                            const int* orig1, const int* orig2, int n2, const int* ranks, const int* col_off,
                            const float* Ut, int dpad, const float* w, const double* inv_cumw, const float* basis,
                            int K, int Rt, const long* indptr, double* data, int* indices, int* zero_count, int rpad) {
  CTX_CHECK(ctx);
  if (rpad < 64 || rpad % 64) return pmd_fail(ctx, PMD_ERR_ARG, "pmd_csr_fill", "rpad must be a positive multiple of 64");
  pmd_prof_scope prof__(ctx, "csr_assembly");
  const long D = (long)d1 * d2;
  PMD_HIP(ctx, hipMemsetAsync(zero_count, 0, sizeof(int), ctx->stream));
  hipLaunchKernelGGL(csr_fill_kernel, dim3((unsigned)((D + 255) / 256)), dim3(256), 0, ctx->stream, d1, d2, order_f, b1,
                     cover1, cover2, orig1, orig2, n2, ranks, col_off, Ut, dpad, w, inv_cumw, basis, K, Rt, indptr, data,
                     indices, zero_count, rpad);
  PMD_LAUNCH_CHECK(ctx, "csr_fill_kernel");
  return PMD_OK;
}
