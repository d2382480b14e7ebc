// OASIS spike inference of ROI traces for an AR(2) model with real roots (localmd_amd/deconvolve.py, p = 2; Friedrich,
// Zhou & Paninski 2017, Alg. 3, in its online "push, then merge while violated" form): minimise
// 1/2 |c + b - y|^2 + lam sum_t s_t over s_t = c_t - g1 c_{t-1} - g2 c_{t-2} >= 0 by greedy pooling.  A pool is a
// spike-free stretch c[t0 + j] = h_j v + g2 h_{j-1} w' (h the impulse response, v its first value, w' the last value of
// the pool underneath); with N = sum_j h_j y'[t0 + j] and M = sum_j h_{j-1} y'[t0 + j] kept per pool, the identity
// h_{m+j} = h_m h_j + g2 h_{m-1} h_{j-1} makes a merge O(1), so the mapping of oasis.hip carries over: one lane per
// problem, 64 problems per wave, one wave per workgroup.  Contraction is off, every fp32 operation is rounded on its own
// and divisions are IEEE, so tests/oasis2_ref.py reproduces every output bit for bit; the exact sequence of operations is
// stated in include/pmd_hip.h.
//
// oasis_ar2_kernel    the lanes of a wave step t in lockstep.  Forward pass: the load of y[t + 1] is issued before frame
//                     t is worked on; the top pool (v, w, N, M, t0) and the pool under it (with gw = g2 w' of the pool
//                     below it and the three entries of H that its length selects) stay in registers, everything below
//                     lies on the lane's stack in the workspace.  A push stores the pool that leaves the registers; a
//                     merge reloads the pool that enters them and the w of the pool below that one.  Only the merge loop
//                     diverges.  The length of a pool is not stored: it is the distance to the next pool's first frame.
//                     Fill pass: t ascends again, a lane walks its stack from the bottom and writes c and s of frame t
//                     (coalesced over the problems), and adds the squared residual to its fp64 chain.  The kernel never
//                     forms a power or a sum of squares: it indexes the three table rows of its trace.
//
// Workspace: problem p = 64 q + lane of a wave of m = min(64, n_prob - 64 q) problems has its pool d at element
// 64 q T + d m + lane of five arrays (v, w, N, M: float, t0: int) of n_prob T elements each; a sixth array of that size
// is spare, 24 bytes per pool.  Lanes at the same depth share cache lines.  A lane only ever reads what it wrote itself,
// in program order: there are no atomics, no LDS, no barrier, and no wave waits for another.
#include "pmd_common.h"
#include "../../include/pmd_hip.h"

namespace {

__global__ __launch_bounds__(64) void oasis_ar2_kernel(const float* __restrict__ Y, long ldy, int T, long n_prob,
                                                        const int* __restrict__ col, const float* __restrict__ par,
                                                        const int* __restrict__ tab_row, const float* __restrict__ tab,
                                                        long ldtab, float* __restrict__ C, long ldc,
                                                        float* __restrict__ S, long lds, double* __restrict__ rss,
                                                        int* __restrict__ n_pools, float* __restrict__ st_v,
                                                        float* __restrict__ st_w, float* __restrict__ st_n,
                                                        float* __restrict__ st_m, int* __restrict__ st_t0) {
#pragma clang fp contract(off)
  const long p = (long)blockIdx.x * 64 + threadIdx.x;
  if (p >= n_prob) return;
  const float g1 = par[5 * p], g2 = par[5 * p + 1], lam = par[5 * p + 2], s_min = par[5 * p + 3], b = par[5 * p + 4];
  const float* __restrict__ y = Y + col[p];
  const float* __restrict__ H = tab + (long)tab_row[p] * ldtab;      // H[i] = h_{i-1}
  const float* __restrict__ HH = H + ldtab;
  const float* __restrict__ HK = HH + ldtab;
  const long rest = n_prob - (long)blockIdx.x * 64;
  const long m = rest < 64 ? rest : 64;                          // problems of this wave
  const long base = (long)blockIdx.x * T * 64 + threadIdx.x;     // pool d of this lane: base + m d
  const float one_g1 = 1.f - g1;
  const float one_g = one_g1 - g2;
  const float mu = lam * one_g;
  const float mu1 = lam * one_g1;

  // ---- forward pass: pools 0 .. depth - 3 on the stack, pool depth - 2 in (pv, pw, pn, pm, pt) with pgw = g2 w of the
  // pool below it and (ph1, ph0, phm) = h_l, h_{l-1}, h_{l-2} of its length l; the top in (v, w, n, mm, t0)
  int depth = 0;
  float v = 0.f, w = 0.f, n = 0.f, mm = 0.f;
  float pv = 0.f, pw = 0.f, pn = 0.f, pm = 0.f, pgw = 0.f, ph1 = 0.f, ph0 = 0.f, phm = 0.f;
  int t0 = 0, pt = 0;
  float y_next = y[0];
  for (int t = 0; t < T; ++t) {
    const float yt = y_next;
    if (t + 1 < T) y_next = y[(long)(t + 1) * ldy];
    if (depth >= 2) {                  // the pool under the top leaves the registers
      const long a = base + m * (depth - 2);
      st_v[a] = pv, st_w[a] = pw, st_n[a] = pn, st_m[a] = pm, st_t0[a] = pt;
    }
    if (depth >= 1) {
      const float below = depth >= 2 ? pw : 0.f;
      pgw = g2 * below;
      pv = v, pw = w, pn = n, pm = mm, pt = t0;
      const long l = t - t0;           // the length of the pool that is now under the top, >= 1
      ph1 = H[l + 1], ph0 = H[l], phm = H[l - 1];
    }
    const float yb = yt - b;
    const float x = yb - (t < T - 2 ? mu : (t == T - 2 ? mu1 : lam));
    const float xv = depth == 0 ? (x > 0.f ? x : 0.f) : x;      // the bottom pool's value is clipped, its sum N is not
    v = xv, w = xv, n = x, mm = 0.f, t0 = t;
    ++depth;
    // Every iteration pops one pool and the loop stops at depth 1.  At frame t the stack holds at most t + 1 pools, so
    // at most t iterations run: `room` carries that bound, the loop ends whatever the data are (a NaN never compares
    // true, so it never merges), and it waits for nobody.
    for (int room = t; room > 0; --room) {
      if (depth < 2) break;
      const float e1 = ph1 * pv;
      const float e2 = ph0 * pgw;
      const float pred = e1 + e2;
      const float lim = pred + s_min;
      if (!(v < lim)) break;
      const float gm = g2 * mm;
      const float a1 = ph1 * n;
      const float a2 = ph0 * gm;
      const float an = a1 + a2;
      const float b1 = ph0 * n;
      const float b2 = phm * gm;
      const float bm = b1 + b2;
      n = pn + an, mm = pm + bm, t0 = pt;
      --depth;
      const long l = t + 1 - t0;       // the merged length, >= 2
      const float k1 = pgw * HK[l];
      const float num = n - k1;
      v = num / HH[l];
      if (depth == 1) v = v > 0.f ? v : 0.f;
      const float w1 = H[l] * v;
      const float w2 = H[l - 1] * pgw;
      w = w1 + w2;
      if (depth >= 2) {                // the pool that enters the registers, and the w of the pool below it
        const long a = base + m * (depth - 2);
        pv = st_v[a], pw = st_w[a], pn = st_n[a], pm = st_m[a], pt = st_t0[a];
        const float below = depth >= 3 ? st_w[a - m] : 0.f;
        pgw = g2 * below;
        const long pl = t0 - pt;
        ph1 = H[pl + 1], ph0 = H[pl], phm = H[pl - 1];
      }
    }
  }
  if (depth >= 2) {
    const long a = base + m * (depth - 2);
    st_v[a] = pv, st_w[a] = pw, st_t0[a] = pt;
  }
  {
    const long a = base + m * (depth - 1);
    st_v[a] = v, st_w[a] = w, st_t0[a] = t0;
  }
  if (n_pools) n_pools[p] = depth;
  if (!C && !S && !rss) return;

  // ---- fill pass: pool k is (vk, gw, start) with gw = g2 w of pool k - 1, the next one begins at frame `next`
  int k = -1, next = 0, start = 0;
  float vk = 0.f, wk = 0.f, gw = 0.f, c1 = 0.f, c2 = 0.f;
  double acc = 0.0;
  float y_cur = y[0];
  for (int t = 0; t < T; ++t) {
    const float yt = y_cur;
    if (t + 1 < T) y_cur = y[(long)(t + 1) * ldy];
    const bool first = t == next;
    if (first) {
      ++k;
      const float below = k >= 1 ? wk : 0.f;
      gw = g2 * below;
      vk = st_v[base + m * k], wk = st_w[base + m * k];
      start = t;
      next = k + 1 < depth ? st_t0[base + m * (k + 1)] : T;
    }
    const long j = t - start;
    const float f1 = H[j + 1] * vk;
    const float f2 = H[j] * gw;
    const float c = f1 + f2;
    float s = 0.f;
    if (first && k >= 1) {
      const float x1 = g1 * c1;
      float d = c - x1;
      if (t >= 2) {
        const float x2 = g2 * c2;
        d = d - x2;
      }
      s = d > 0.f ? d : 0.f;
    }
    c2 = c1, c1 = c;
    if (C) C[(long)t * ldc + p] = c;
    if (S) S[(long)t * lds + p] = s;
    const float cb = c + b;
    const float r = yt - cb;
    acc = acc + (double)r * (double)r;
  }
  if (rss) rss[p] = acc;
}

}  // namespace

extern "C" {

int pmd_oasis_ar2(pmd_ctx* ctx, const float* Y, long ldy, long T, long n_prob, const int* col, const float* par,
                  const int* tab_row, const float* tab, long ldtab, float* C, long ldc, float* S, long lds, double* rss,
                  int* n_pools, void* ws, size_t ws_bytes) {
  CTX_CHECK(ctx);
  const char* what = "pmd_oasis_ar2";
  if (T < 1 || T >= 0x7fffffffL || n_prob < 1 || ldy < 1 || ldtab < T + 2)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (1 <= T < 2^31 - 1, n_prob >= 1, ldy >= 1, ldtab >= T + 2)");
  if ((C && ldc < n_prob) || (S && lds < n_prob))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "ldc or lds smaller than n_prob");
  if (!Y || !col || !par || !tab || !tab_row) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (!C && !S && !rss && !n_pools) return pmd_fail(ctx, PMD_ERR_ARG, what, "no output requested");
  const long blocks = (n_prob + 63) / 64;
  if (blocks > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many problems in one call");
  const size_t pools = (size_t)n_prob * (size_t)T;
  if (!ws || ws_bytes < (size_t)24 * pools)
    return pmd_fail(ctx, PMD_ERR_WORKSPACE, what, "workspace smaller than 24 T n_prob bytes");
  pmd_prof_scope prof__(ctx, "oasis_ar2");
  float* st_v = (float*)ws;
  float* st_w = st_v + pools;
  float* st_n = st_w + pools;
  float* st_m = st_n + pools;
  int* st_t0 = (int*)(st_m + pools);       // the sixth array of `pools` words is spare
  hipLaunchKernelGGL(oasis_ar2_kernel, dim3((unsigned)blocks), dim3(64), 0, ctx->stream, Y, ldy, (int)T, n_prob, col, par,
                     tab_row, tab, ldtab, C, ldc, S, lds, rss, n_pools, st_v, st_w, st_n, st_m, st_t0);
  PMD_LAUNCH_CHECK(ctx, "oasis_ar2_kernel");
  return PMD_OK;
}

}  // extern "C"
