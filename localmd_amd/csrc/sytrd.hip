// Dense symmetric eigensolver for the global stage (decomposition.py:984, :1090, :1129: the
// jnp.linalg.svd(..., hermitian=True) calls on min(R, frames)-sized Gram matrices).
//
//   A = Q T Q^T   blocked Householder tridiagonalisation, hand-written (this file)
//   T = Z L Z^T   rocSOLVER sstedc (divide and conquer)
//   E = Q Z       rocSOLVER sormtr
//
// The tridiagonalisation is the memory-bound part: every column needs y = A_trailing v over the
// not-yet-reduced block.  rocSOLVER's ssytrd reads the full square for it and spends five
// launches per column (~0.55 s at n = 10^4); here the product reads only one triangle (each
// element a_cr feeds y_c and y_r), and a column costs two launches:
//   sytrd_advance : finish w of the previous column from the partial sums, apply the panel's
//                   rank-2 corrections to the next column, partial norms for its reflector
//   sytrd_symv    : reflector scalars, triangle matrix-vector product tiles, panel dot products
// followed per 64-column panel by one rank-2k update of the trailing block (rocBLAS ssyr2k).
// All partial sums are combined in a fixed order: results are run-to-run reproducible.
//
// Conventions = LAPACK ssytrd('L') on the column-major view of the buffer.  In memory terms:
// row c of the buffer holds A(r, c) for r >= c at offset r ("memory-upper" triangle is the one
// that is read); reflector j is v = [1, A[j][j+2..n)] acting on positions j+1..n-1, tau[j].
#include "pmd_internal.h"
#include <rocsolver/rocsolver.h>
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#define PMD_BLAS(ctx, call)                                                     \
  do {                                                                          \
    rocblas_status s__ = (call);                                                \
    if (s__ != rocblas_status_success) return pmd_fail(ctx, PMD_ERR_BLAS, #call, rocblas_status_to_string(s__)); \
  } while (0)

namespace {

constexpr int NB = 64;      // panel width
constexpr int BR = 64;      // rows of one symv tile
constexpr int CW = 512;     // positions of one symv tile: 2 x 256 (4 row quarters of 16 rows, two workgroups per CU);
                            // measured at n = 10^4: 334 ms (1024 = 4 x 256, 2 row halves of 32 rows), 303 ms (512), 320 ms (256)
constexpr int DCH = 256;    // positions per dot-product workgroup

struct sytrd_bufs {
  float* W;     // NB x ldw: w vectors of the current panel
  long ldw;
  float* RP;    // [chunk q][row c]: row partial sums of the symv tiles
  float* CP;    // [row block b][position r]: column partial sums
  long ldp;
  float* SP;    // per tile workgroup: partial v^T A v
  float* DP;    // [dot chunk][2][NB]: partial W_k^T v, V_k^T v
  double* NP;   // per advance workgroup: partial sum of squares
  float* scal;  // beta, tau, scale of the current reflector
  int cw;       // tile width (positions) of the symv launches: CW
};

__device__ __forceinline__ int tile_r0(int cs, int b) { return (cs + b * BR) & ~3; }
__device__ __forceinline__ int tile_nq(int n, int cs, int b, int cw) { return (n - tile_r0(cs, b) + cw - 1) / cw; }

// deterministic sum over the workgroup (nthreads <= 512); every thread gets the result
template <typename T>
__device__ __forceinline__ T block_sum(T val, T* s_red, int nthreads) {
  const int tid = threadIdx.x;
  __syncthreads();
  s_red[tid] = val;
  __syncthreads();
  for (int o = 256; o > 0; o >>= 1) {
    if (tid < o && tid + o < nthreads) s_red[tid] += s_red[tid + o];
    __syncthreads();
  }
  return s_red[0];
}

// sum of p[idx * stride] for idx = first, first + step, ... < count, in that order; the first U loads
// are issued together (straight-line code, so that independent batches of one kernel overlap)
template <int U>
__device__ __forceinline__ float batch_sum(const float* __restrict__ p, long stride, int first, int step, int count) {
  float acc = 0.f;
  {
    float t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = first + u * step;
      t[u] = p[(long)((idx < count) ? idx : 0) * stride];  // unconditional load: no branch, no wait between loads
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc += (first + u * step < count) ? t[u] : 0.f;
  }
  for (int base = first + U * step; base < count; base += U * step) {
    float t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + u * step;
      t[u] = p[(long)((idx < count) ? idx : 0) * stride];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc += (base + u * step < count) ? t[u] : 0.f;
  }
  return acc;
}

// batch_sum in two halves, so that the first batches of several sums can be issued back to back before anything
// waits (a sum's continuation loop is control flow: loads that follow it in program order would otherwise start
// one memory round trip later).  batch_finish adds in exactly the order of batch_sum.
// (addresses: wave-uniform base pointer + 32-bit byte offset per lane - one add, one compare and one select per load
// instead of a 64-bit multiply-add: with ~130 loads per thread the address arithmetic was most of this kernel)
template <int U>
__device__ __forceinline__ void batch_issue(const float* __restrict__ base, unsigned elem_off, unsigned stride, int first, int step,
                                            int count, float* t) {
  const char* bp = reinterpret_cast<const char*>(base);
  const unsigned off0 = elem_off * 4u;                              // idx = 0 (always valid to read)
  const unsigned offf = off0 + (unsigned)first * stride * 4u;       // idx = first
  const unsigned inc = (unsigned)step * stride * 4u;
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const unsigned off = (first + u * step < count) ? offf + (unsigned)u * inc : off0;
    t[u] = *reinterpret_cast<const float*>(bp + off);
  }
}
template <int U>
__device__ __forceinline__ float batch_finish(const float* __restrict__ p, long stride, int first, int step, int count,
                                              const float* t0) {
  float acc = 0.f;
#pragma unroll
  for (int u = 0; u < U; ++u) acc += (first + u * step < count) ? t0[u] : 0.f;
  for (int base = first + U * step; base < count; base += U * step) {
    float t[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int idx = base + u * step;
      t[u] = p[(long)((idx < count) ? idx : 0) * stride];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) acc += (base + u * step < count) ? t[u] : 0.f;
  }
  return acc;
}

// ------------------------------------------------------------------------------------------
// FIN: finish w of column jp = j - 1 (slatrd steps after the symv):
//        w_pre = A v - V (W^T v) - W (V^T v);  w = tau w_pre - (tau^2/2)(w_pre^T v) v
// UPD: column j of the panel gets the rank-2 corrections of the i = j - j0 earlier panel columns.
// Always (unless FIN && !UPD): d[j] and the partial norms of A[j][j+2..n).
// One workgroup = 64 positions r = j + 64 blockIdx.x + lane; wave `part` of waves 0..3 sums every
// fourth partial of those positions, so that all loads of a thread are in flight at once.  Lanes
// 0..3 of wave 4 do the same for position j: w_jp[j] is a scalar every workgroup needs, and it
// comes out bit-identical to what the owner of that position stores.
// ------------------------------------------------------------------------------------------
constexpr int APOS = 64;

#ifdef PMD_SYMV_TRACE
// Debug build only (PMD_EXTRA_FLAGS=-DPMD_SYMV_TRACE): wall-clock stamps (100 MHz) of the phases of every workgroup
// of the symv launch of column PMD_SYMV_TRACE_J, read back with pmdk_symv_trace (scripts/symv_trace.py).
#ifndef PMD_SYMV_TRACE_J
#define PMD_SYMV_TRACE_J 32
#endif
__device__ unsigned long long g_symv_trace[4096 * 8];
#define TRACE_STAMP(slot)                                                                     \
  do {                                                                                        \
    if (j == PMD_SYMV_TRACE_J && threadIdx.x == 0 && wg < 4096) g_symv_trace[wg * 8 + (slot)] = wall_clock64(); \
  } while (0)
__device__ unsigned long long g_adv_trace[1024 * 8];
#define ADV_STAMP(slot)                                                                       \
  do {                                                                                        \
    if (FIN && UPD && j == PMD_SYMV_TRACE_J && threadIdx.x == 0 && blockIdx.x < 1024) g_adv_trace[blockIdx.x * 8 + (slot)] = wall_clock64(); \
  } while (0)
#define ADV2_STAMP(slot)                                                                      \
  do {                                                                                        \
    if (UPD && j == PMD_SYMV_TRACE_J && threadIdx.x == 0 && blockIdx.x < 1024) g_adv_trace[blockIdx.x * 8 + (slot)] = wall_clock64(); \
  } while (0)
#else
#define TRACE_STAMP(slot) do {} while (0)
#define ADV_STAMP(slot) do {} while (0)
#define ADV2_STAMP(slot) do {} while (0)
#endif


template <bool FIN, bool UPD>
__global__ __launch_bounds__(320) void sytrd_advance_kernel(float* __restrict__ A, long ld, int n, int j, int j0,
                                                            sytrd_bufs B, int nsp, float* __restrict__ d) {
  __shared__ float s_dW[NB], s_dV[NB], s_Wj[NB], s_Vj[NB];
  __shared__ float s_y[4][APOS + 1], s_u[4][APOS + 1];
  __shared__ float s_red[8];
  __shared__ float s_sp[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform, and known to be)
  const int jp = j - 1;
  const int ip = jp - j0;  // earlier panel columns seen by column jp
  int part = wave, slot = lane, r = j + blockIdx.x * APOS + lane;
  if (wave == 4) {
    part = lane & 3;
    slot = APOS;
    r = (FIN && UPD && lane < 4) ? j : n;
  }
  const bool live = r < n;
  if (!live) r = n - 1;  // idle lanes run the same loads on a valid position and store nothing
  const bool combiner = live && part == 0;          // wave 0, and lane 0 of wave 4
  const bool owner = live && wave == 0;             // stores results of position r
  float tau = 0.f, scale = 0.f, alpha = 0.f;
  float ypart = 0.f, upart = 0.f, xv = 0.f;
  float vkv[16], wkv[16];
  // every load below is unconditional (clamped index + select): the compiler turns a guarded load into a
  // branch with a full wait behind it, which serialises the ~80 independent loads of a thread
  ADV_STAMP(0);
  const float xj = A[(long)j * ld + r];
  if (FIN) {
    // every load of this phase is issued here, back to back, before anything is summed
    const int cs = j;  // first row of the symv launch of column jp
    const int nbk = (n - cs + BR - 1) / BR;
    const int bc = (r - cs) / BR;
    const int nq = tile_nq(n, cs, bc, B.cw);
    int bmax = bc;
    if (bc + 1 < nbk && tile_r0(cs, bc + 1) <= r) bmax = bc + 1;
    const int ndch = (n - j + DCH - 1) / DCH;  // dot chunks of the symv launch of column jp (cs = j)
    const int kd = tid & (NB - 1), whichd = (tid >> 6) & 1;
    const int kcd = (kd < ip) ? kd : 0;
    const float* dp = B.DP + (long)whichd * NB + kcd;
    float t_rp[10], t_cp[40], t_dp[40], t_sp[4];
    batch_issue<10>(B.RP, (unsigned)r, (unsigned)B.ldp, part, 4, nq, t_rp);
    batch_issue<40>(B.CP, (unsigned)r, (unsigned)B.ldp, part, 4, bmax + 1, t_cp);
    xv = A[(long)jp * ld + r];
    {
      const char* vb = reinterpret_cast<const char*>(A + (long)j0 * ld);  // panel rows: uniform base + small offsets
      const char* wb = reinterpret_cast<const char*>(B.W);
      const unsigned r4 = (unsigned)r * 4u, ldb = (unsigned)ld * 4u, ldwb = (unsigned)B.ldw * 4u;
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int k = part + 4 * t;
        const unsigned kc = (k < ip) ? (unsigned)k : 0u;
        vkv[t] = *reinterpret_cast<const float*>(vb + (kc * ldb + r4));
        wkv[t] = *reinterpret_cast<const float*>(wb + (kc * ldwb + r4));
      }
    }
    batch_issue<40>(B.DP, (unsigned)(whichd * NB + kcd), 2u * NB, 0, 1, ndch, t_dp);
    const float* sidep = (whichd == 0) ? B.W + (long)kcd * B.ldw + j : A + (long)(j0 + kcd) * ld + j;
    const float sidev = *sidep;
    batch_issue<4>(B.SP, 0u, 1u, tid, 320, nsp, t_sp);
    tau = B.scal[1];
    scale = B.scal[2];
    ADV_STAMP(6);
    ypart = batch_finish<10>(B.RP + r, B.ldp, part, 4, nq, t_rp) + batch_finish<40>(B.CP + r, B.ldp, part, 4, bmax + 1, t_cp);
    {
      float acc = batch_finish<40>(dp, 2 * NB, 0, 1, ndch, t_dp);
      if (kd >= ip) acc = 0.f;
      const float side = UPD ? sidev : 0.f;
      if (tid < NB) {
        s_dW[kd] = acc;
        s_Wj[kd] = side;
      } else if (tid < 2 * NB) {
        s_dV[kd] = acc;
        s_Vj[kd] = side;
      }
    }
    ADV_STAMP(1);
    float part_sp = batch_finish<4>(B.SP, 1, tid, 320, nsp, t_sp);
    ADV_STAMP(2);
    for (int o = 32; o > 0; o >>= 1) part_sp += __shfl_xor(part_sp, o);
    if (lane == 0) s_red[wave] = part_sp;
    __syncthreads();
    ADV_STAMP(3);
    const float vav = ((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) + s_red[4];
    float cross = 0.f;
    for (int k = 0; k < ip; ++k) cross += s_dV[k] * s_dW[k];
    const float vtw = vav - 2.f * cross;
    alpha = -0.5f * tau * tau * vtw;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const int k = part + 4 * t;
      if (k < ip) {
        ypart -= vkv[t] * s_dW[k] + wkv[t] * s_dV[k];
        if (UPD) upart += vkv[t] * s_Wj[k] + wkv[t] * s_Vj[k];
      }
    }
    if (live) {
      s_y[part][slot] = ypart;
      if (UPD) s_u[part][slot] = upart;
    }
    __syncthreads();
  }
  ADV_STAMP(4);
  float w = 0.f, v = 0.f, u = 0.f;
  if (FIN && combiner) {
    const float y = (s_y[0][slot] + s_y[1][slot]) + (s_y[2][slot] + s_y[3][slot]);
    if (UPD) u = (s_u[0][slot] + s_u[1][slot]) + (s_u[2][slot] + s_u[3][slot]);
    v = (r == j) ? 1.f : xv * scale;
    w = tau * y + alpha * v;
    if (owner) {
      B.W[(long)ip * B.ldw + r] = w;
      A[(long)jp * ld + r] = v;
    } else {
      s_sp[0] = w;
    }
  }
  if (FIN && !UPD) return;
  if (FIN && UPD) __syncthreads();
  if (wave != 0) return;
  double sq = 0.0;
  if (owner) {
    float x = xj;
    if (UPD) {
      x -= u + (v * s_sp[0] + w);
      A[(long)j * ld + r] = x;
    }
    if (r == j) d[j] = x;
    if (r >= j + 2) sq = (double)x * (double)x;
  }
  for (int o = 32; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
  if (lane == 0) B.NP[blockIdx.x] = sq;
  ADV_STAMP(5);
}

// ------------------------------------------------------------------------------------------
// The same step with the loads spread over more SIMDs (phase trace, scripts/symv_trace.py: with 64 positions x
// 4 parts per workgroup a thread issues ~130 loads and the kernel is bound by instruction issue, 2.8 us before
// the last load is out).  Here a workgroup owns 32 positions, eight parts sum every eighth partial (waves 0..3,
// two parts each), wave 4 computes the scalars every position needs (w_jp[j], v^T w) with one partial per lane,
// waves 5 and 6 sum the panel dot products.  FIN is implied (a previous column exists).  Fixed summation order.
// ------------------------------------------------------------------------------------------
constexpr int APOS2 = 32, NPART2 = 8;

__device__ __forceinline__ float wave_tree_sum(float v) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <bool UPD>
__global__ __launch_bounds__(448) void sytrd_advance2_kernel(float* __restrict__ A, long ld, int n, int j, int j0,
                                                             sytrd_bufs B, int nsp, float* __restrict__ d) {
  __shared__ float s_dW[NB], s_dV[NB], s_Wj[NB], s_Vj[NB];
  __shared__ float s_y[NPART2][APOS2 + 1], s_u[NPART2][APOS2 + 1];
  __shared__ float s_red[8];
  __shared__ float s_bc[2];  // alpha, w_jp[j]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int jp = j - 1;
  const int ip = jp - j0;  // earlier panel columns seen by column jp
  const int cs = j;        // first row of the symv launch of column jp
  const int nbk = (n - cs + BR - 1) / BR;
  ADV2_STAMP(0);
  float t_sp[4];
  batch_issue<4>(B.SP, 0u, 1u, tid, 448, nsp, t_sp);
  const float tau = B.scal[1], scale = B.scal[2];

  // ---- role-specific loads (wave-uniform branches, straight-line loads inside)
  const int part = wave * 2 + (lane >> 5), pl = lane & 31;
  int r = j + blockIdx.x * APOS2 + pl;
  const bool live = wave < 4 && r < n;
  if (r >= n) r = n - 1;
  float t_rp[3], t_cp[20], vkv[8], wkv[8], t_dp[40];
  float xv = 0.f, xj = 0.f, sidev = 0.f, rp_j = 0.f, cp_j = 0.f;
  int nq = 0, bmax = 0, nq_j = 0;
  if (wave < 4) {
    const int bc = (r - cs) / BR;
    nq = tile_nq(n, cs, bc, B.cw);
    bmax = bc;
    if (bc + 1 < nbk && tile_r0(cs, bc + 1) <= r) bmax = bc + 1;
    batch_issue<3>(B.RP, (unsigned)r, (unsigned)B.ldp, part, NPART2, nq, t_rp);
    batch_issue<20>(B.CP, (unsigned)r, (unsigned)B.ldp, part, NPART2, bmax + 1, t_cp);
    const char* vb = reinterpret_cast<const char*>(A + (long)j0 * ld);
    const char* wb = reinterpret_cast<const char*>(B.W);
    const unsigned r4 = (unsigned)r * 4u, ldb = (unsigned)ld * 4u, ldwb = (unsigned)B.ldw * 4u;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int k = part + NPART2 * t;
      const unsigned kc = (k < ip) ? (unsigned)k : 0u;
      vkv[t] = *reinterpret_cast<const float*>(vb + (kc * ldb + r4));
      wkv[t] = *reinterpret_cast<const float*>(wb + (kc * ldwb + r4));
    }
    xv = A[(long)jp * ld + r];
    xj = A[(long)j * ld + r];
  } else if (wave == 4) {
    // position j: its partial sums are the row chunks of row block 0 and that block's column partial
    nq_j = tile_nq(n, cs, 0, B.cw);
    rp_j = B.RP[(long)((lane < nq_j) ? lane : 0) * B.ldp + j];
    cp_j = B.CP[j];
  } else {
    const int which = wave - 5;
    const int kc = (lane < ip) ? lane : 0;
    const int ndch = (n - j + DCH - 1) / DCH;  // dot chunks of the symv launch of column jp
    batch_issue<40>(B.DP, (unsigned)(which * NB + kc), 2u * NB, 0, 1, ndch, t_dp);
    if (UPD) sidev = (which == 0) ? B.W[(long)kc * B.ldw + j] : A[(long)(j0 + kc) * ld + j];
    float acc = batch_finish<40>(B.DP + which * NB + kc, 2 * NB, 0, 1, ndch, t_dp);
    if (lane >= ip) acc = 0.f;
    if (which == 0) {
      s_dW[lane] = acc;
      s_Wj[lane] = sidev;
    } else {
      s_dV[lane] = acc;
      s_Vj[lane] = sidev;
    }
  }
  ADV2_STAMP(6);
  float ypart = 0.f, upart = 0.f;
  if (wave < 4)
    ypart = batch_finish<3>(B.RP + r, B.ldp, part, NPART2, nq, t_rp) + batch_finish<20>(B.CP + r, B.ldp, part, NPART2, bmax + 1, t_cp);
  ADV2_STAMP(1);
  float part_sp = batch_finish<4>(B.SP, 1, tid, 448, nsp, t_sp);
  ADV2_STAMP(2);
  part_sp = wave_tree_sum(part_sp);
  if (lane == 0) s_red[wave] = part_sp;
  __syncthreads();
  ADV2_STAMP(3);

  if (wave < 4) {
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int k = part + NPART2 * t;
      if (k < ip) {
        ypart -= vkv[t] * s_dW[k] + wkv[t] * s_dV[k];
        if (UPD) upart += vkv[t] * s_Wj[k] + wkv[t] * s_Vj[k];
      }
    }
    s_y[part][pl] = ypart;
    if (UPD) s_u[part][pl] = upart;
  } else if (wave == 4) {
    const float vav = (((s_red[0] + s_red[1]) + (s_red[2] + s_red[3])) + ((s_red[4] + s_red[5]) + s_red[6]));
    const bool kin = lane < ip;
    const float cross = wave_tree_sum(kin ? s_dV[lane] * s_dW[lane] : 0.f);
    const float alpha = -0.5f * tau * tau * (vav - 2.f * cross);
    float yj = ((lane < nq_j) ? rp_j : 0.f) + ((lane == 0) ? cp_j : 0.f);
    if (UPD && kin) yj -= s_Vj[lane] * s_dW[lane] + s_Wj[lane] * s_dV[lane];
    yj = wave_tree_sum(yj);  // (only the update of column j uses it: UPD)
    if (lane == 0) {
      s_bc[0] = alpha;
      s_bc[1] = tau * yj + alpha;  // v[j] = 1
    }
  }
  __syncthreads();
  ADV2_STAMP(4);
  if (tid >= APOS2) return;
  // ---- combine the eight parts of position r (wave 0, lanes 0..31)
  float w = 0.f, v = 0.f, u = 0.f;
  if (live) {
    const float y = ((s_y[0][pl] + s_y[1][pl]) + (s_y[2][pl] + s_y[3][pl])) + ((s_y[4][pl] + s_y[5][pl]) + (s_y[6][pl] + s_y[7][pl]));
    if (UPD) u = ((s_u[0][pl] + s_u[1][pl]) + (s_u[2][pl] + s_u[3][pl])) + ((s_u[4][pl] + s_u[5][pl]) + (s_u[6][pl] + s_u[7][pl]));
    v = (r == j) ? 1.f : xv * scale;
    w = tau * y + s_bc[0] * v;
    B.W[(long)ip * B.ldw + r] = w;
    A[(long)jp * ld + r] = v;
  }
  if (!UPD) return;
  double sq = 0.0;
  if (live) {
    const float x = xj - (u + (v * s_bc[1] + w));
    A[(long)j * ld + r] = x;
    if (r == j) d[j] = x;
    if (r >= j + 2) sq = (double)x * (double)x;
  }
  for (int o = 16; o > 0; o >>= 1) sq += __shfl_xor(sq, o);
  if (lane == 0) B.NP[blockIdx.x] = sq;
  ADV2_STAMP(5);
}

// ------------------------------------------------------------------------------------------
// Column j: reflector scalars from the partial norms (every workgroup, same order), then
//   tiles (b, q): rows c in [cs + 64 b, +64), positions [r0(b) + 1024 q, +1024), cs = j + 1:
//       RP[q][c]  = sum_{r in tile, r >= c} A[c][r] v[r]
//       CP[b][r]  = sum_{c in tile, c <  r} A[c][r] v[c]
//   dot workgroups: W_k^T v and V_k^T v over 256 positions for the k < j - j0 panel columns.
// ------------------------------------------------------------------------------------------

template <int CWT>
__global__ __launch_bounds__(512, CWT == 1024 ? 2 : 4) void sytrd_symv_kernel(const float* __restrict__ A, long ld, int n, int j, int j0,
                                                         sytrd_bufs B, int n_np, int npairs, int nbk,
                                                         float* __restrict__ e, float* __restrict__ tau_out) {
  constexpr int NPG = CWT / 256;   // position groups (256 positions = 64 lanes x float4 each)
  constexpr int NRG = 8 / NPG;     // row groups
  constexpr int RPW = BR / NRG;    // rows per wave: 32 or 16, all in flight at once
  constexpr int LOGR = (RPW == 32) ? 5 : (RPW == 16) ? 4 : 3;
#ifdef PMD_SYMV_TRACE
  if (j == PMD_SYMV_TRACE_J && threadIdx.x == 0) {
    const int wg_ = blockIdx.y * gridDim.x + blockIdx.x;
    if (wg_ < 4096) g_symv_trace[wg_ * 8 + 6] = wall_clock64();
  }
#endif
  __shared__ float s_v[BR];
  __shared__ float s_row[NPG][BR];
  __shared__ float s_col[NPG][NRG - 1][64][4];
  __shared__ float s_red[8];
  __shared__ float s_sc[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // (uniform, and known to be)
  const int wc = wave % NPG, rh = wave / NPG;  // position group and row group of this wave
  const int cs = j + 1;
  const float* xr = A + (long)j * ld;
  const int wg = blockIdx.y * gridDim.x + blockIdx.x;
  const bool is_dot = (int)blockIdx.y >= npairs;
  TRACE_STAMP(0);
  // ---- which tile: row blocks are paired (p, nbk-1-p) so that every grid row has about the same work
  int b = blockIdx.y, q = blockIdx.x;
  bool valid = !is_dot;
  if (valid) {
    const int nq_b = tile_nq(n, cs, b, CWT);
    if (q >= nq_b) {
      const int b2 = nbk - 1 - b;
      q -= nq_b;
      if (b2 == b || q >= tile_nq(n, cs, b2, CWT)) valid = false;
      b = b2;
    }
  }
  if (!valid && !is_dot) {
    if (tid == 0) B.SP[wg] = 0.f;
    return;
  }
  const int cb = is_dot ? cs : cs + b * BR;
  const int rows = min(BR, n - cb);
  const int r0 = tile_r0(cs, is_dot ? 0 : b);
  const int pos = r0 + (is_dot ? 0 : q) * CWT + wc * 256 + lane * 4;
  const int n4 = (n + 3) & ~3;
  const bool ok = pos < n4;
  // Every load of the tile is issued before anything waits: one memory round trip per workgroup.  The
  // loads are unconditional (clamped row / position, results masked later): a guarded load becomes a
  // branch with a full wait behind it.  Rows >= rows repeat the last row and meet v = 0.
  // wave 0 first asks for the partial norms and the pivot of the reflector (written by the previous launch): its
  // scalar chain then runs while the tile streams in, instead of starting one round trip after the tile arrived
  double np_pre[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
  float a0_pre = 0.f;
  if (wave == 0) {
#pragma unroll
    for (int u = 0; u < 5; ++u) {
      const int t = lane + 64 * u;
      np_pre[u] = B.NP[(t < n_np) ? t : 0];
    }
    a0_pre = xr[cs];
  }
  TRACE_STAMP(7);
  float4 a[RPW];
  float v4[4];
  {
    const int posc = ok ? pos : r0;
    const float* ap = A + (long)cb * ld + posc;
#pragma unroll
    for (int uu = 0; uu < RPW; ++uu) a[uu] = *reinterpret_cast<const float4*>(ap + (long)min(rh * RPW + uu, rows - 1) * ld);
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      const int r = pos + t;
      const bool in = r < n && r > cs;
      v4[t] = xr[in ? r : cs];
      if (!in) v4[t] = 0.f;
    }
    if (tid < BR) {
      const int c = cb + tid;
      const bool in = c < n && c > cs;
      const float xc = xr[in ? c : cs];
      s_v[tid] = in ? xc : 0.f;
    }
  }
  TRACE_STAMP(1);
  if (wave == 0) {
    // reflector scalars: fixed-order tree over the partial norms, every lane of wave 0 holds the result
    double xn = 0.0;
#pragma unroll
    for (int u = 0; u < 5; ++u) xn += (lane + 64 * u < n_np) ? np_pre[u] : 0.0;
    for (int t = lane + 320; t < n_np; t += 64) xn += B.NP[t];
    for (int o = 32; o > 0; o >>= 1) xn += __shfl_xor(xn, o);
    const float a0 = a0_pre;
    float beta = a0, tau = 0.f, scale = 0.f;
    if (xn > 0.0) {
      const double nr = sqrt((double)a0 * (double)a0 + xn);
      const double bt = (a0 >= 0.f) ? -nr : nr;
      beta = (float)bt;
      tau = (float)((bt - (double)a0) / bt);
      scale = (float)(1.0 / ((double)a0 - bt));
    }
    if (lane == 0) {
      s_sc[0] = beta;
      s_sc[1] = tau;
      s_sc[2] = scale;
      if (blockIdx.x == 0 && blockIdx.y == 0) {
        e[j] = beta;
        tau_out[j] = tau;
        B.scal[0] = beta;
        B.scal[1] = tau;
        B.scal[2] = scale;
      }
    }
  }
  __syncthreads();
  TRACE_STAMP(2);
  const float scale = s_sc[2];

  if (is_dot) {
    // ---- panel dot products
    const int i = j - j0;
    const int dchunk = ((int)blockIdx.y - npairs) * gridDim.x + blockIdx.x;
    const int base = cs + dchunk * DCH;
    if (base >= n || i == 0) return;
    float vv[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int r = base + g * 64 + lane;
      const float xg = xr[min(r, n - 1)];
      vv[g] = (r < n) ? ((r == cs) ? 1.f : xg * scale) : 0.f;
    }
    for (int k = wave; k < i; k += 8) {
      float aw = 0.f, av = 0.f;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int r = min(base + g * 64 + lane, n - 1);  // beyond n: vv = 0
        aw += B.W[(long)k * B.ldw + r] * vv[g];
        av += A[(long)(j0 + k) * ld + r] * vv[g];
      }
      for (int o = 32; o > 0; o >>= 1) {
        aw += __shfl_xor(aw, o);
        av += __shfl_xor(av, o);
      }
      if (lane == 0) {
        B.DP[((long)dchunk * 2 + 0) * NB + k] = aw;
        B.DP[((long)dchunk * 2 + 1) * NB + k] = av;
      }
    }
    return;
  }
  // v = x * scale, v[cs] = 1
#pragma unroll
  for (int t = 0; t < 4; ++t) v4[t] = (pos + t == cs) ? 1.f : v4[t] * scale;
  if (tid < BR) s_v[tid] = (cb + tid == cs) ? 1.f : s_v[tid] * scale;
  __syncthreads();

  const bool edge = (q == 0) || (r0 + (q + 1) * CWT > n);
  float col[4] = {0.f, 0.f, 0.f, 0.f};
  float pr[RPW];
  if (edge) {
#pragma unroll
    for (int uu = 0; uu < RPW; ++uu) {
      const int c = cb + rh * RPW + uu;
      const float vc = s_v[rh * RPW + uu];
      // row part uses r >= c, column part r > c; nothing beyond n
      const float m0 = (pos + 0 < n) ? a[uu].x : 0.f, m1 = (pos + 1 < n) ? a[uu].y : 0.f,
                  m2 = (pos + 2 < n) ? a[uu].z : 0.f, m3 = (pos + 3 < n) ? a[uu].w : 0.f;
      pr[uu] = (((pos + 0 >= c) ? m0 * v4[0] : 0.f) + ((pos + 1 >= c) ? m1 * v4[1] : 0.f)) +
               (((pos + 2 >= c) ? m2 * v4[2] : 0.f) + ((pos + 3 >= c) ? m3 * v4[3] : 0.f));
      col[0] += (pos + 0 > c) ? m0 * vc : 0.f;
      col[1] += (pos + 1 > c) ? m1 * vc : 0.f;
      col[2] += (pos + 2 > c) ? m2 * vc : 0.f;
      col[3] += (pos + 3 > c) ? m3 * vc : 0.f;
    }
  } else {
#pragma unroll
    for (int uu = 0; uu < RPW; ++uu) {
      const float vc = s_v[rh * RPW + uu];
      pr[uu] = (a[uu].x * v4[0] + a[uu].y * v4[1]) + (a[uu].z * v4[2] + a[uu].w * v4[3]);
      col[0] += a[uu].x * vc;
      col[1] += a[uu].y * vc;
      col[2] += a[uu].z * vc;
      col[3] += a[uu].w * vc;
    }
  }
#ifdef PMD_SYMV_TRACE
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#endif
  TRACE_STAMP(3);
  // RPW row sums across the 64 lanes: halve the number of values per lane at every exchange; after LOGR
  // exchanges a lane holds one row (index = its top LOGR lane bits), the remaining lane bits are plain adds
#pragma unroll
  for (int s = 0; s < LOGR; ++s) {
    const int off = 32 >> s, half = (RPW / 2) >> s;
    const bool upper = (lane & off) != 0;
#pragma unroll
    for (int t = 0; t < half; ++t) {
      const float send = upper ? pr[t] : pr[t + half];
      const float keep = upper ? pr[t + half] : pr[t];
      pr[t] = keep + __shfl_xor(send, off);
    }
  }
#pragma unroll
  for (int off = 32 >> LOGR; off > 0; off >>= 1) pr[0] += __shfl_xor(pr[0], off);
  if ((lane & ((64 >> LOGR) - 1)) == 0) s_row[wc][rh * RPW + (lane >> (6 - LOGR))] = pr[0];
  if (rh > 0) {
#pragma unroll
    for (int t = 0; t < 4; ++t) s_col[wc][rh - 1][lane][t] = col[t];
  }
  __syncthreads();
  TRACE_STAMP(4);
  float spart = 0.f;
  if (tid < rows) {
    float rs = s_row[0][tid];
#pragma unroll
    for (int g = 1; g < NPG; ++g) rs += s_row[g][tid];
    B.RP[(long)q * B.ldp + cb + tid] = rs;
    spart = s_v[tid] * rs;
  }
  if (rh == 0) {
#pragma unroll
    for (int g = 0; g < NRG - 1; ++g)
#pragma unroll
      for (int t = 0; t < 4; ++t) col[t] += s_col[wc][g][lane][t];
    spart += (v4[0] * col[0] + v4[1] * col[1]) + (v4[2] * col[2] + v4[3] * col[3]);
    if (ok) *reinterpret_cast<float4*>(B.CP + (long)b * B.ldp + pos) = make_float4(col[0], col[1], col[2], col[3]);
  }
  for (int o = 32; o > 0; o >>= 1) spart += __shfl_xor(spart, o);
  if (lane == 0) s_red[wave] = spart;
  __syncthreads();
  if (tid == 0) {
    float tot = 0.f;
    for (int t = 0; t < 8; ++t) tot += s_red[t];
    B.SP[wg] = tot;
  }
  TRACE_STAMP(5);
}

// Panel update of the trailing block (slatrd's A22 -= V W^T + W V^T) on the triangle that is read:
//   T[c][r] -= sum_k V_k[c] W_k[r] + W_k[c] V_k[r],   ts <= c <= r < n,  k < nbc <= 64.
// One workgroup = one 64 x 64 tile (I <= J); wave w owns rows 16 w .. 16 w + 15 of it in four 16 x 16 fp32 MFMA
// accumulators; rocBLAS' ssyr2k spends several launches per call on this.  The panel operands are staged through LDS:
// the workgroup copies the 64 x 64 blocks of V and W it needs (row side and column side, two halves of 32 panel rows,
// coalesced 256-byte rows) into LDS once and every wave reads its MFMA fragments from there (fragments loaded straight
// from the panels cost ten 4-byte loads per eight MFMAs, the column side fetched by all four waves: 2.5 x the L2 traffic).
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void sytrd_rank2k_lds_kernel(float* __restrict__ A, long lda, int n, int ts, int j0, int nbc,
                                                               const float* __restrict__ W, long ldw) {
  constexpr int LS = 68;
  __shared__ float sv_c[32][LS], sw_c[32][LS], sv_r[32][LS], sw_r[32][LS];   // [panel row][position]: row side (c), column side (r)
  const int I = blockIdx.y, J = blockIdx.x;
  if (J < I) return;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane((int)(tid >> 6));
  const int n16 = lane & 15, kk = lane >> 4;
  const int cb = ts + 64 * I, r0 = ts + 64 * J;
  const int c0 = cb + 16 * wave;
  const float* V = A + (long)j0 * lda;
  f32x4 acc[4];
#pragma unroll
  for (int jn = 0; jn < 4; ++jn) acc[jn] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int lp = tid & 63, lk = tid >> 6;   // loader: position lp, panel rows lk, lk + 4, ...
  const int pc = min(cb + lp, n - 1), pr = min(r0 + lp, n - 1);
  for (int h = 0; h < 2; ++h) {
    if (h) __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int k = 32 * h + lk + 4 * u;
      const bool in = k < nbc;
      const long kc = in ? k : 0;   // unconditional loads on a valid row, masked below
      const float v1 = V[kc * lda + pc], w1 = W[kc * ldw + pc], v2 = V[kc * lda + pr], w2 = W[kc * ldw + pr];
      sv_c[lk + 4 * u][lp] = in ? v1 : 0.f;
      sw_c[lk + 4 * u][lp] = in ? w1 : 0.f;
      sv_r[lk + 4 * u][lp] = in ? v2 : 0.f;
      sw_r[lk + 4 * u][lp] = in ? w2 : 0.f;
    }
    __syncthreads();
    if (c0 < n) {
#pragma unroll
      for (int k0 = 0; k0 < 32; k0 += 4) {
        const int k = k0 + kk;
        const float a1 = sv_c[k][16 * wave + n16], a2 = sw_c[k][16 * wave + n16];
#pragma unroll
        for (int jn = 0; jn < 4; ++jn) {
          const float b1 = sw_r[k][16 * jn + n16], b2 = sv_r[k][16 * jn + n16];
          acc[jn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[jn], 0, 0, 0);
          acc[jn] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, b2, acc[jn], 0, 0, 0);
        }
      }
    }
  }
  if (c0 >= n) return;
#pragma unroll
  for (int jn = 0; jn < 4; ++jn) {
    const int col = r0 + 16 * jn + n16;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int row = c0 + 4 * kk + i;
      if (row < n && col < n && col >= row) A[(long)row * lda + col] -= acc[jn][i];
    }
  }
}

__global__ void copy_rows_kernel(const float* __restrict__ src, long lds_, float* __restrict__ dst, long ldd, int n) {
  const int row = blockIdx.y;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x)
    dst[(long)row * ldd + c] = src[(long)row * lds_ + c];
}

// Vb[k][r - p0] = reflector k0 + k at position r (0 before its unit entry, 1 at k0 + k + 1); a reflector
// with tau = 0 is the identity and becomes a zero row
__global__ void extract_v_kernel(const float* __restrict__ A, long lda, const float* __restrict__ tau, int k0, int p0,
                                 int np, float* __restrict__ Vb, long ldv, int off) {
  const int k = blockIdx.y;
  const int unit = k0 + k + off;       // off = 1: tridiagonalisation of this file; off = 64: band reduction of sytrd2.hip
  const bool dead = tau[k0 + k] == 0.f;
  for (int rr = blockIdx.x * blockDim.x + threadIdx.x; rr < np; rr += gridDim.x * blockDim.x) {
    const int r = p0 + rr;
    float v = 0.f;
    if (!dead && r >= unit) v = (r == unit) ? 1.f : A[(long)(k0 + k) * lda + r];
    Vb[(long)k * ldv + rr] = v;
  }
}

// S = Vb Vb^T (row-major kb x kb) -> T^{-1} = striu(S) + diag(1 / tau) in place
__global__ void tinv_kernel(float* __restrict__ S, int kb, const float* __restrict__ tau, int k0) {
  const int i = blockIdx.x;
  for (int jj = threadIdx.x; jj < kb; jj += blockDim.x) {
    float v = S[(long)i * kb + jj];
    if (jj < i) v = 0.f;
    if (jj == i) {
      const float t = tau[k0 + i];
      v = (t == 0.f) ? 1.f : 1.f / t;
    }
    S[(long)i * kb + jj] = v;
  }
}

}  // namespace

// Z <- Q Z for the Q of pmd_sytrd_impl (reflectors in A, tau): memory row m of Z is one vector over the
// positions.  Blocks of QB reflectors in compact WY form, Q_blk = I - V T V^T with
// T^{-1} = striu(V^T V) + diag(1/tau), applied last block first:  Z -= ((Z V) T^T) V^T.
// Three GEMMs and one triangular solve per block (rocSOLVER's sormtr works in 64-column steps at ~20 TFLOP/s).
constexpr int QB = 1024;

static size_t pmd_apply_q_workspace_bytes_impl(int n) {
  return ((size_t)QB * n + (size_t)QB * QB + (size_t)n * QB) * sizeof(float) + 4096;
}

// off: distance of a reflector's unit entry below the diagonal (reflector c = [1 at position c + off, A[c][c + off + 1 ..)])
static int pmd_apply_q_off_impl(pmd_ctx* ctx, int n, const float* A, long lda, const float* tau, float* Z, long ldz,
                                void* ws, size_t ws_bytes, int off) {
  pmd_prof_scope prof__(ctx, "apply_q");
  if (n < off + 1) return PMD_OK;
  pmd_arena ar(ws, ws_bytes);
  float* Vb = ar.take_n<float>((size_t)QB * n);
  float* S = ar.take_n<float>((size_t)QB * QB);
  float* Y = ar.take_n<float>((size_t)n * QB);
  if (ar.overflow) return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_apply_q", "workspace too small");
  const int nref = n - off;
  const float one = 1.f;
  for (int k0 = (nref - 1) / QB * QB; k0 >= 0; k0 -= QB) {
    const int kb = std::min(QB, nref - k0);
    const int p0 = k0 + off, np = n - p0;
    hipLaunchKernelGGL(extract_v_kernel, dim3((np + 255) / 256, kb), dim3(256), 0, ctx->stream, A, lda, tau, k0, p0, np, Vb, (long)np, off);
    PMD_LAUNCH_CHECK(ctx, "extract_v_kernel");
    int rc = pmd_gemm_rm(ctx, 0, 1, kb, kb, np, 1.f, Vb, np, Vb, np, 0.f, S, kb);
    if (rc != PMD_OK) return rc;
    hipLaunchKernelGGL(tinv_kernel, dim3(kb), dim3(256), 0, ctx->stream, S, kb, tau, k0);
    PMD_LAUNCH_CHECK(ctx, "tinv_kernel");
    rc = pmd_gemm_rm(ctx, 0, 1, n, kb, np, 1.f, Z + p0, ldz, Vb, np, 0.f, Y, kb);  // Y = Z V
    if (rc != PMD_OK) return rc;
    // X = Y T^T  <=>  T^{-1} X^T = Y^T: the row-major upper triangular T^{-1} is a column-major lower one, transposed
    PMD_BLAS(ctx, rocblas_strsm(ctx->blas, rocblas_side_left, rocblas_fill_lower, rocblas_operation_transpose,
                                rocblas_diagonal_non_unit, kb, n, &one, S, kb, Y, kb));
    rc = pmd_gemm_rm(ctx, 0, 0, n, np, kb, -1.f, Y, kb, Vb, np, 1.f, Z + p0, ldz);  // Z -= X V^T
    if (rc != PMD_OK) return rc;
  }
  return PMD_OK;
}

static int pmd_apply_q_impl(pmd_ctx* ctx, int n, const float* A, long lda, const float* tau, float* Z, long ldz, void* ws,
                     size_t ws_bytes) {
  return pmd_apply_q_off_impl(ctx, n, A, lda, tau, Z, ldz, ws, ws_bytes, 1);
}

// ---------------------------------------------------------------------------------------------
static size_t pmd_sytrd_workspace_bytes_impl(int n) {
  const size_t n4 = (size_t)pmd_round_up(n, 4);
  const size_t nq = (size_t)(n / 256 + 2), nbk = (size_t)(n / BR + 2);
  size_t b = 0;
  b += NB * n4 * sizeof(float) + 256;                 // W
  b += nq * n4 * sizeof(float) + 256;                 // RP
  b += nbk * n4 * sizeof(float) + 256;                // CP
  b += (nq + 2) * (nbk + 2) * sizeof(float) + 256;    // SP
  b += (size_t)(n / DCH + 2) * 2 * NB * sizeof(float) + 256;  // DP
  b += (size_t)(n / 32 + 2) * sizeof(double) + 256;  // NP (one per advance workgroup: 32 positions)
  b += 4096;
  return b;
}

// Tridiagonalise the symmetric matrix held in A (memory-upper triangle read, see the header comment).
// d[n], e[n-1], tau[n-1] on the device.  lda % 4 == 0, lda >= round_up(n, 4), A 16-byte aligned.
static int pmd_sytrd_impl(pmd_ctx* ctx, int n, float* A, long lda, float* d, float* e, float* tau, void* ws, size_t ws_bytes) {
  pmd_prof_scope prof__(ctx, "sytrd");
  if (n < 1) return PMD_OK;
  const long n4 = pmd_round_up(n, 4);
  if (lda % 4 != 0 || lda < n4 || ((uintptr_t)A & 15)) return pmd_fail(ctx, PMD_ERR_ARG, "pmd_sytrd", "lda must be a multiple of 4, >= round_up(n,4), A 16-byte aligned");
  pmd_arena ar(ws, ws_bytes);
  sytrd_bufs B;
  const size_t nqmax = (size_t)(n / 256 + 2), nbkmax = (size_t)(n / BR + 2);
  B.ldw = n4;
  B.ldp = n4;
  B.W = ar.take_n<float>(NB * (size_t)n4);
  B.RP = ar.take_n<float>(nqmax * n4);
  B.CP = ar.take_n<float>(nbkmax * n4);
  B.SP = ar.take_n<float>((nqmax + 2) * (nbkmax + 2));
  B.DP = ar.take_n<float>((size_t)(n / DCH + 2) * 2 * NB);
  B.NP = ar.take_n<double>((size_t)(n / 32 + 2));
  B.scal = ar.take_n<float>(16);
  if (ar.overflow) return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_sytrd", "workspace too small");
  hipStream_t st = ctx->stream;

  B.cw = CW;
  const bool use_rocblas_syr2k = ctx->routes.syr2k_rocblas;
  const bool adv_old = ctx->routes.sytrd_advance_old;   // 64 positions x 4 parts per workgroup
  const float one = 1.f, minus1 = -1.f;
  int nsp = 0;
  for (int j0 = 0; j0 < n - 1; j0 += NB) {
    const int nbc = std::min(NB, n - 1 - j0);
    for (int i = 0; i < nbc; ++i) {
      const int j = j0 + i;
      int ga = (n - j + APOS - 1) / APOS;  // workgroups of the advance launch = partial norms the symv sums
      if (i == 0) {
        hipLaunchKernelGGL((sytrd_advance_kernel<false, false>), dim3(ga), dim3(320), 0, st, A, lda, n, j, j0, B, nsp, d);
      } else if (adv_old) {
        hipLaunchKernelGGL((sytrd_advance_kernel<true, true>), dim3(ga), dim3(320), 0, st, A, lda, n, j, j0, B, nsp, d);
      } else {
        ga = (n - j + APOS2 - 1) / APOS2;
        hipLaunchKernelGGL((sytrd_advance2_kernel<true>), dim3(ga), dim3(448), 0, st, A, lda, n, j, j0, B, nsp, d);
      }
      const int cs = j + 1;
      const int nbk = (n - cs + BR - 1) / BR;
      const int npairs = (nbk + 1) / 2;
      auto r0 = [&](int b) { return (cs + b * BR) & ~3; };
      auto nq = [&](int b) { return (n - r0(b) + CW - 1) / CW; };
      int nqx = 1;
      for (int p = 0; p < npairs; ++p) nqx = std::max(nqx, nq(p) + ((nbk - 1 - p != p) ? nq(nbk - 1 - p) : 0));
      const int ndch = (i > 0) ? (n - cs + DCH - 1) / DCH : 0;
      const int drows = (ndch + nqx - 1) / nqx;
      {
        // with profiling on, every 64th column's product is timed on its own (bench.py: roofline of this kernel)
        pmd_prof_scope sample__((ctx->profile && (j & 63) == 32) ? ctx : nullptr, "sytrd_symv_sample");
        hipLaunchKernelGGL(sytrd_symv_kernel<CW>, dim3(nqx, npairs + drows), dim3(512), 0, st, A, lda, n, j, j0, B, ga, npairs, nbk, e, tau);
      }
      nsp = nqx * npairs;
    }
    PMD_LAUNCH_CHECK(ctx, "sytrd panel");
    const int ts = j0 + nbc;
    if (adv_old)
      hipLaunchKernelGGL((sytrd_advance_kernel<true, false>), dim3((n - ts + APOS - 1) / APOS), dim3(320), 0, st, A, lda, n, ts, j0, B, nsp, d);
    else
      hipLaunchKernelGGL((sytrd_advance2_kernel<false>), dim3((n - ts + APOS2 - 1) / APOS2), dim3(448), 0, st, A, lda, n, ts, j0, B, nsp, d);
    PMD_LAUNCH_CHECK(ctx, "sytrd_advance_kernel");
    if (use_rocblas_syr2k) {
      PMD_BLAS(ctx, rocblas_ssyr2k(ctx->blas, rocblas_fill_lower, rocblas_operation_none, n - ts, nbc, &minus1,
                                   A + (long)j0 * lda + ts, (rocblas_int)lda, B.W + ts, (rocblas_int)B.ldw, &one,
                                   A + (long)ts * lda + ts, (rocblas_int)lda));
    } else {
      const int nt = (n - ts + 63) / 64;
      hipLaunchKernelGGL(sytrd_rank2k_lds_kernel, dim3(nt, nt), dim3(256), 0, st, A, lda, n, ts, j0, nbc, B.W, B.ldw);
      PMD_LAUNCH_CHECK(ctx, "sytrd_rank2k_lds_kernel");
    }
  }
  hipLaunchKernelGGL((sytrd_advance_kernel<false, false>), dim3(1), dim3(320), 0, st, A, lda, n, n - 1, n - 1, B, 0, d);
  PMD_LAUNCH_CHECK(ctx, "sytrd_advance_kernel");
  return PMD_OK;
}

// rocSOLVER's own tridiagonalisation with the same conventions (tests, small matrices)
static int pmd_sytrd_rocsolver(pmd_ctx* ctx, int n, float* A, long lda, float* d, float* e, float* tau) {
  pmd_prof_scope prof__(ctx, "rocsolver_ssytrd");
  PMD_BLAS(ctx, rocsolver_ssytrd(ctx->blas, rocblas_fill_lower, n, A, (rocblas_int)lda, d, e, tau));
  return PMD_OK;
}

// Library-owned scratch of the eigensolver (grown on demand, released with the context)
static int ctx_scratch(pmd_ctx* ctx, size_t bytes, void** out) {
  if (ctx->scratch_bytes < bytes) {
    PMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    ctx->scratch = nullptr;
    ctx->scratch_bytes = 0;
    PMD_HIP(ctx, hipMalloc(&ctx->scratch, bytes));
    ctx->scratch_bytes = bytes;
  }
  *out = ctx->scratch;
  return PMD_OK;
}

// Tridiagonalisation alone (tests and probes): impl 0 = rocSOLVER ssytrd('L'), 1 = this file.
extern "C" int pmdk_sytrd(pmd_ctx* ctx, int n, float* A, long lda, float* d, float* e, float* tau, int impl) {
  CTX_CHECK(ctx);
  if (impl == 0) return pmd_sytrd_rocsolver(ctx, n, A, lda, d, e, tau);
  const size_t tb = pmd_sytrd_workspace_bytes_impl(n);
  void* scratch = nullptr;
  int rc = ctx_scratch(ctx, tb, &scratch);
  if (rc != PMD_OK) return rc;
  return pmd_sytrd_impl(ctx, n, A, lda, d, e, tau, scratch, tb);
}

// Two-stage path (sytrd2.hip): A = Q1 B Q1^T (band), B = Q2 T Q2^T (tridiagonal), sstedc, E = Q1 (Q2 Z).  *done = 0 and A
// untouched when a panel of stage 1 was numerically rank deficient.
static int pmd_syevd_two_stage(pmd_ctx* ctx, int n, float* A, long lda, float* w, int* info, int* done) {
  *done = 0;
  const size_t b1 = pmd_sy2sb_workspace_bytes_impl(n), b2 = pmd_sb2st_workspace_bytes_impl(n);
  const size_t bq = pmd_apply_q_workspace_bytes_impl(n);
  const size_t zb = (size_t)n * n * sizeof(float), ab = (size_t)n * lda * sizeof(float);
  void* scratch = nullptr;
  int rc = ctx_scratch(ctx, zb + ab + std::max(b1, bq) + b2 + 4 * (size_t)n * sizeof(float) + 16384, &scratch);
  if (rc != PMD_OK) return rc;
  pmd_arena ar(scratch, ctx->scratch_bytes);
  float* Z = ar.take_n<float>((size_t)n * n);
  float* W = ar.take_n<float>((size_t)n * lda);     // working copy: stage 1 overwrites it with the band and the reflectors
  float* e = ar.take_n<float>(n);
  float* tau1 = ar.take_n<float>(n);
  void* w1 = ar.take(std::max(b1, bq));
  void* w2 = ar.take(b2);
  if (ar.overflow) return pmd_fail(ctx, PMD_ERR_WORKSPACE, "pmd_syevd_two_stage", "scratch too small");
  PMD_HIP(ctx, hipMemcpyAsync(W, A, ab, hipMemcpyDeviceToDevice, ctx->stream));
  int flag = 0;
  rc = pmd_sy2sb_impl(ctx, n, W, lda, tau1, &flag, w1, b1);
  if (rc != PMD_OK) return rc;
  if (flag) return PMD_OK;
  float *V2 = nullptr, *tau2 = nullptr;
  rc = pmd_sb2st_impl(ctx, n, W, lda, w, e, &V2, &tau2, w2, b2);
  if (rc != PMD_OK) return rc;
  {
    pmd_prof_scope prof__(ctx, "rocsolver_sstedc");
    rocblas_status st = rocsolver_sstedc(ctx->blas, rocblas_evect_tridiagonal, n, w, e, Z, n, info);
    if (st != rocblas_status_success) return pmd_fail(ctx, PMD_ERR_BLAS, "rocsolver_sstedc", rocblas_status_to_string(st));
  }
  rc = pmd_sb2st_apply_q2_impl(ctx, n, V2, tau2, Z, n, n);
  if (rc != PMD_OK) return rc;
  rc = pmd_apply_q_off_impl(ctx, n, W, lda, tau1, Z, n, w1, bq, 64);
  if (rc != PMD_OK) return rc;
  hipLaunchKernelGGL(copy_rows_kernel, dim3(8, n), dim3(256), 0, ctx->stream, Z, (long)n, A, lda, n);
  PMD_LAUNCH_CHECK(ctx, "copy_rows_kernel");
  *done = 1;
  return PMD_OK;
}

namespace {
__global__ void widen_kernel(const float* __restrict__ src, long lds_, double* __restrict__ dst, long ldd, int n) {
  const int r = blockIdx.y;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) dst[(long)r * ldd + c] = (double)src[(long)r * lds_ + c];
}
__global__ void narrow_kernel(const double* __restrict__ src, long lds_, float* __restrict__ dst, long ldd, int n) {
  const int r = blockIdx.y;
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) dst[(long)r * ldd + c] = (float)src[(long)r * lds_ + c];
}
// Eigenvalues computed in double -> fp32, with the magnitude of a numerically null one floored at eps32 * max |lambda|.
// The reference diagonalises in fp32 (jnp.linalg.svd(hermitian=True) = LAPACK ssyevd on CPU): a null direction comes out of
// it with |lambda| ~ eps32 lambda_max, never with the 1e-11 lambda_max a double-precision solver can return for the same
// fp32 matrix - and the reference's rule keeps every non-zero |lambda| and scales its direction by 1 / sqrt(|lambda|)
// (decomposition.py:984-996).  Without the floor the double-precision paths amplify such a direction 100x more than the
// reference's arithmetic can (seeded fuzz, round 3: fit 7.2 / 20.9 where float64 gives 0.7 / 1.1).  Exact zeros stay zero.
__global__ void narrow_eigenvalues_kernel(const double* __restrict__ src, float* __restrict__ dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double lmax = fmax(fabs(src[0]), fabs(src[n - 1]));     // ascending order
  const double floor_ = 1.1920929e-07 * lmax;
  const double v = src[i];
  dst[i] = (float)((v != 0.0 && fabs(v) < floor_) ? copysign(floor_, v) : v);
}
}  // namespace

// Small orders in double precision (rocSOLVER dsyevd on a widened copy, results rounded to fp32): what NumPy does for
// float32 input, and the policy of the tile stage (Gram matrices diagonalised in fp64) carried up to the global stage
// where it costs a few milliseconds.  The fp32 divide-and-conquer class loses two digits against QR-iteration / MRRR
// solvers on the graded Gram spectra of this pipeline (profiles/r02_fuzz_wide.txt); in fp64 that is below fp32 rounding.
static int syevd_f64(pmd_ctx* ctx, int n, float* A, long lda, float* w, int* info) {
  pmd_prof_scope prof__(ctx, "rocsolver_dsyevd");
  void* scratch = nullptr;
  int rc = ctx_scratch(ctx, ((size_t)n * n + 2 * (size_t)n) * sizeof(double) + 4096, &scratch);
  if (rc != PMD_OK) return rc;
  pmd_arena ar(scratch, ctx->scratch_bytes);
  double* Ad = ar.take_n<double>((size_t)n * n);
  double* wd = ar.take_n<double>(n);
  double* ed = ar.take_n<double>(n);
  hipLaunchKernelGGL(widen_kernel, dim3((n + 255) / 256, n), dim3(256), 0, ctx->stream, A, lda, Ad, (long)n, n);
  PMD_LAUNCH_CHECK(ctx, "widen_kernel");
  PMD_BLAS(ctx, rocsolver_dsyevd(ctx->blas, rocblas_evect_original, rocblas_fill_lower, n, Ad, n, wd, ed, info));
  hipLaunchKernelGGL(narrow_kernel, dim3((n + 255) / 256, n), dim3(256), 0, ctx->stream, Ad, (long)n, A, lda, n);
  hipLaunchKernelGGL(narrow_eigenvalues_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, wd, w, n);
  PMD_LAUNCH_CHECK(ctx, "narrow_kernel");
  return PMD_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// fp64 refinement of an fp32 eigendecomposition (Ogita & Aishima, "Iterative refinement for symmetric eigenvalue
// decomposition", Japan J. Indust. Appl. Math. 35, 2018).  The fp32 solvers (own tridiagonalisation + sstedc, rocSOLVER
// ssyevd) return vectors with an error of ~c eps32 lambda_1 / |lambda_i - lambda_j| per pair: 5e-4 on Vt rows whose
// singular values differ by 2 % (measured: 128 x 128 x 10^4 movie, order 2027), where NumPy - LAPACK in double on the
// same fp32 matrix - is exact to 1e-6.  With X the computed vectors (columns), in double:
//     G = X^T X,  S = X^T A X,  lambda~_i = S_ii / G_ii,  R = I - G,
//     E_ij = (S_ij + lambda~_j R_ij) / (lambda~_j - lambda~_i)   if |lambda~_i - lambda~_j| > delta,   else R_ij / 2,
//     X <- X + X E
// converges quadratically for the pairs outside clusters (delta = 1e-5 max |lambda|: what fp32 cannot separate stays the
// fp32 solver's choice, orthonormalised).  7 n^3 fp64 flops per step on the fp64 matrix cores: 1.5 ms per step at
// n = 2000, 12 ms at 4096; applied between SYEVD_F64_MAX (up to it the whole problem runs in double) and
// SYEVD_REFINE_MAX (beyond it the cost reaches the solver's own).
// ---------------------------------------------------------------------------------------------------------------
constexpr int SYEVD_F64_MAX = 512;
constexpr int SYEVD_REFINE_MAX = 4096;
constexpr int SYEVD_REFINE_STEPS = 2;
namespace {
__global__ void refine_lambda_kernel(const double* __restrict__ S, const double* __restrict__ G, int n, double* __restrict__ lam) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) lam[i] = S[(long)i * n + i] / G[(long)i * n + i];
}
// S (column-major, ld n) <- E; lmax = max |lambda~| is taken from the ends of the ascending spectrum
__global__ void refine_e_kernel(double* __restrict__ S, const double* __restrict__ G, const double* __restrict__ lam, int n) {
  const int j = blockIdx.y;                                    // column
  const double lj = lam[j];
  const double lmax = fmax(fabs(lam[0]), fabs(lam[n - 1]));
  const double delta = 1e-5 * lmax;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const long k = (long)j * n + i;
    const double r = (i == j ? 1.0 : 0.0) - G[k];
    const double dl = lj - lam[i];
    S[k] = (i != j && fabs(dl) > delta) ? (S[k] + lj * r) / dl : 0.5 * r;
  }
}
__global__ void narrow_vec_kernel(const double* __restrict__ src, float* __restrict__ dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = (float)src[i];
}
// The Rayleigh quotients of refined vectors need not ascend where the fp32 solver's did (inside a cluster, a repeated
// eigenvalue or a null space they differ by rounding only): rank[i] = place of lam[i] in ascending order, ties by index
// (counting, n <= SYEVD_REFINE_MAX), sorted[rank[i]] = lam[i].
__global__ void refine_rank_kernel(const double* __restrict__ lam, int n, int* __restrict__ rank, double* __restrict__ sorted) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double li = lam[i];
  int r = 0;
  for (int j = 0; j < n; ++j) {
    const double lj = lam[j];
    r += (lj < li || (lj == li && j < i)) ? 1 : 0;
  }
  rank[i] = r;
  sorted[r] = li;
}
// narrow_kernel with vector r leaving as memory row rank[r]
__global__ void narrow_ranked_kernel(const double* __restrict__ src, long lds_, const int* __restrict__ rank, float* __restrict__ dst,
                                     long ldd, int n) {
  const int r = blockIdx.y;
  const long ro = rank[r];
  for (int c = blockIdx.x * blockDim.x + threadIdx.x; c < n; c += gridDim.x * blockDim.x) dst[ro * ldd + c] = (float)src[(long)r * lds_ + c];
}
}  // namespace

int pmd_ctx_scratch2(pmd_ctx* ctx, size_t bytes, void** out) {
  if (ctx->scratch2_bytes < bytes) {
    PMD_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->scratch2) (void)hipFree(ctx->scratch2);
    ctx->scratch2 = nullptr;
    ctx->scratch2_bytes = 0;
    PMD_HIP(ctx, hipMalloc(&ctx->scratch2, bytes));
    ctx->scratch2_bytes = bytes;
  }
  *out = ctx->scratch2;
  return PMD_OK;
}

static int refine_steps_for(int n) { return (n > SYEVD_F64_MAX && n <= SYEVD_REFINE_MAX) ? SYEVD_REFINE_STEPS : 0; }

// Ad: widened copy of the input matrix (column-major lower triangle valid), taken BEFORE the fp32 solver overwrote A;
// A (memory row j = eigenvector j) and w are refined in place and leave in ascending order of the refined eigenvalues.
// ws: 5 n^2 + n doubles behind Ad.
static int syevd_refine(pmd_ctx* ctx, int n, const double* Ad, float* A, long lda, float* w, double* ws, int steps) {
  pmd_prof_scope prof__(ctx, "syevd_refine_f64");
  const size_t nn = (size_t)n * n;
  double* X = ws;
  double* AX = X + nn;
  double* S = AX + nn;
  double* G = S + nn;
  double* Xn = G + nn;
  double* lam = Xn + nn;
  const double one = 1.0, zero = 0.0;
  hipLaunchKernelGGL(widen_kernel, dim3((n + 255) / 256, n), dim3(256), 0, ctx->stream, A, lda, X, (long)n, n);
  PMD_LAUNCH_CHECK(ctx, "widen_kernel");
  for (int it = 0; it < steps; ++it) {
    PMD_BLAS(ctx, rocblas_dsymm(ctx->blas, rocblas_side_left, rocblas_fill_lower, n, n, &one, Ad, n, X, n, &zero, AX, n));
    PMD_BLAS(ctx, rocblas_dgemm(ctx->blas, rocblas_operation_transpose, rocblas_operation_none, n, n, n, &one, X, n, AX, n, &zero, S, n));
    PMD_BLAS(ctx, rocblas_dgemm(ctx->blas, rocblas_operation_transpose, rocblas_operation_none, n, n, n, &one, X, n, X, n, &zero, G, n));
    hipLaunchKernelGGL(refine_lambda_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, S, G, n, lam);
    hipLaunchKernelGGL(refine_e_kernel, dim3(8, n), dim3(256), 0, ctx->stream, S, G, lam, n);
    PMD_LAUNCH_CHECK(ctx, "refine_e_kernel");
    PMD_HIP(ctx, hipMemcpyAsync(Xn, X, nn * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    PMD_BLAS(ctx, rocblas_dgemm(ctx->blas, rocblas_operation_none, rocblas_operation_none, n, n, n, &one, X, n, S, n, &one, Xn, n));
    double* t = X; X = Xn; Xn = t;
  }
  // ascending order is the contract (and where narrow_eigenvalues_kernel finds max |lambda|); Xn is free by now
  double* sorted = Xn;
  int* rank = reinterpret_cast<int*>(Xn + n);
  hipLaunchKernelGGL(refine_rank_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, lam, n, rank, sorted);
  hipLaunchKernelGGL(narrow_ranked_kernel, dim3((n + 255) / 256, n), dim3(256), 0, ctx->stream, X, (long)n, rank, A, lda, n);
  hipLaunchKernelGGL(narrow_eigenvalues_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, sorted, w, n);
  PMD_LAUNCH_CHECK(ctx, "narrow_ranked_kernel");
  return PMD_OK;
}

static int pmd_syevd_f32(pmd_ctx* ctx, int n, float* A, long lda, float* w, float* work, int* info);

// Symmetric eigendecomposition, ascending eigenvalues; on exit memory row j of A is eigenvector j.
// Only the row-major upper triangle of A (= column-major lower) is read.  work: n floats, info: device int.
int pmd_syevd(pmd_ctx* ctx, int n, float* A, long lda, float* w, float* work, int* info) {
  const int steps = ctx->routes.syevd != PMD_SYEVD_F64 ? refine_steps_for(n) : 0;
  if (steps == 0) return pmd_syevd_f32(ctx, n, A, lda, w, work, info);
  void* s2 = nullptr;
  int rc0 = pmd_ctx_scratch2(ctx, (6 * (size_t)n * n + (size_t)n) * sizeof(double) + 4096, &s2);
  if (rc0 != PMD_OK) return rc0;
  double* Ad = static_cast<double*>(s2);
  hipLaunchKernelGGL(widen_kernel, dim3((n + 255) / 256, n), dim3(256), 0, ctx->stream, A, lda, Ad, (long)n, n);
  PMD_LAUNCH_CHECK(ctx, "widen_kernel");
  rc0 = pmd_syevd_f32(ctx, n, A, lda, w, work, info);
  if (rc0 != PMD_OK) return rc0;
  return syevd_refine(ctx, n, Ad, A, lda, w, Ad + (size_t)n * n, steps);
}

extern "C" int pmdk_syevd(pmd_ctx* ctx, int n, float* A, long lda, float* w, float* work, int* info) {
  CTX_CHECK(ctx);
  return pmd_syevd(ctx, n, A, lda, w, work, info);
}

static int pmd_syevd_f32(pmd_ctx* ctx, int n, float* A, long lda, float* w, float* work, int* info) {
  const int mode = ctx->routes.syevd;
  const bool force_lib = mode == PMD_SYEVD_ROCSOLVER;
  const bool force_own = mode == PMD_SYEVD_OWN;
  if (n >= 1 && (mode == PMD_SYEVD_F64 || (mode == PMD_SYEVD_AUTO && n <= SYEVD_F64_MAX))) return syevd_f64(ctx, n, A, lda, w, info);
  const bool own = !force_lib && (force_own || n >= 192) && n >= 3 && lda % 4 == 0 && lda >= pmd_round_up(n, 4) && !((uintptr_t)A & 15);
  if (!own) {
    pmd_prof_scope prof__(ctx, "rocsolver_ssyevd");
    PMD_BLAS(ctx, rocsolver_ssyevd(ctx->blas, rocblas_evect_original, rocblas_fill_lower, n, A, (rocblas_int)lda, w, work, info));
    return PMD_OK;
  }
  const bool two_stage = mode == PMD_SYEVD_TWOSTAGE && n >= 256;
  if (two_stage) {
    int done = 0;
    const int rc2 = pmd_syevd_two_stage(ctx, n, A, lda, w, info, &done);
    if (rc2 != PMD_OK) return rc2;
    if (done) return PMD_OK;     // else: a rank-deficient panel; A is untouched, the one-stage path below takes over
  }
  const size_t tb = std::max(pmd_sytrd_workspace_bytes_impl(n), pmd_apply_q_workspace_bytes_impl(n));
  const size_t zb = (size_t)n * n * sizeof(float);
  void* scratch = nullptr;
  int rc = ctx_scratch(ctx, tb + zb + 2 * (size_t)n * sizeof(float) + 4096, &scratch);
  if (rc != PMD_OK) return rc;
  pmd_arena ar(scratch, ctx->scratch_bytes);
  float* Z = ar.take_n<float>((size_t)n * n);
  float* e = ar.take_n<float>(n);
  float* tau = ar.take_n<float>(n);
  void* tws = ar.take(tb);
  rc = pmd_sytrd_impl(ctx, n, A, lda, w, e, tau, tws, tb);
  if (rc != PMD_OK) return rc;
  {
    pmd_prof_scope prof__(ctx, "rocsolver_sstedc");
    PMD_BLAS(ctx, rocsolver_sstedc(ctx->blas, rocblas_evect_tridiagonal, n, w, e, Z, n, info));
  }
  if (ctx->routes.apply_q_rocsolver) {
    pmd_prof_scope prof__(ctx, "rocsolver_sormtr");
    PMD_BLAS(ctx, rocsolver_sormtr(ctx->blas, rocblas_side_left, rocblas_fill_lower, rocblas_operation_none, n, n, A,
                                   (rocblas_int)lda, tau, Z, n));
  } else {
    rc = pmd_apply_q_impl(ctx, n, A, lda, tau, Z, n, tws, tb);
    if (rc != PMD_OK) return rc;
  }
  hipLaunchKernelGGL(copy_rows_kernel, dim3(8, n), dim3(256), 0, ctx->stream, Z, (long)n, A, lda, n);
  PMD_LAUNCH_CHECK(ctx, "copy_rows_kernel");
  return PMD_OK;
}

#ifdef PMD_SYMV_TRACE
extern "C" int pmdk_adv_trace(unsigned long long* host_out, int count) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_adv_trace), sizeof(unsigned long long) * (size_t)count, 0, hipMemcpyDeviceToHost);
}
extern "C" int pmdk_symv_trace(unsigned long long* host_out, int count) {
  return (int)hipMemcpyFromSymbol(host_out, HIP_SYMBOL(g_symv_trace), sizeof(unsigned long long) * (size_t)count, 0, hipMemcpyDeviceToHost);
}
#endif
