// OASIS spike inference of ROI traces for an AR(1) model (localmd_amd/deconvolve.py; Friedrich, Zhou & Paninski 2017,
// Alg. 1): minimise 1/2 |c + b - y|^2 + lam sum_t s_t over s_t = c_t - g c_{t-1} >= 0 by pool-adjacent-violators.  The
// solve is sequential along time and independent across problems (a trace with one candidate penalty), so the mapping is
// breadth: one lane per problem, 64 problems per wave, one wave per workgroup.  Contraction is off, every fp32 operation
// is rounded on its own and divisions are IEEE, so tests/oasis_ref.py reproduces every output bit for bit; the exact
// sequence of operations is stated in include/pmd_hip.h.
//
// oasis_ar1_kernel    the lanes of a wave step t in lockstep.  Forward pass: the load of y[t + 1] is issued before frame
//                     t is worked on; the top pool (v, w, t0) and the pool under it (with the power pw[l] that its
//                     length selects) stay in registers, everything below lies on the lane's stack in the workspace.  A
//                     push stores the pool that leaves the registers; a merge reloads the pool that enters them.  Only
//                     the merge loop diverges.  The length of a pool is not stored: it is the distance to the next
//                     pool's first frame.  Fill pass: t ascends again, a lane walks its stack from the bottom and
//                     writes c and s of frame t (coalesced over the problems), and adds the squared residual to its
//                     fp64 chain.  The kernel never forms a power of g: it indexes the table row of its trace.
//
// Workspace: problem p = 64 q + lane of a wave of m = min(64, n_prob - 64 q) problems has its pool d at element
// 64 q T + d m + lane of three arrays (v, w: float, t0: int) of n_prob T elements each, 12 bytes per pool, so that lanes
// at the same depth share cache lines.  A lane only ever reads what it wrote itself, in program order: there are no
// atomics, no LDS, no barrier, and no wave waits for another.
#include "pmd_common.h"
#include "../../include/pmd_hip.h"

namespace {

__global__ __launch_bounds__(64) void oasis_ar1_kernel(const float* __restrict__ Y, long ldy, int T, long n_prob,
                                                        const int* __restrict__ col, const float* __restrict__ par,
                                                        const int* __restrict__ pw_row, const float* __restrict__ pw,
                                                        long ldpw, float* __restrict__ C, long ldc,
                                                        float* __restrict__ S, long lds, double* __restrict__ rss,
                                                        int* __restrict__ n_pools, float* __restrict__ st_v,
                                                        float* __restrict__ st_w, int* __restrict__ st_t0) {
#pragma clang fp contract(off)
  const long p = (long)blockIdx.x * 64 + threadIdx.x;
  if (p >= n_prob) return;
  const float g = par[4 * p], lam = par[4 * p + 1], s_min = par[4 * p + 2], b = par[4 * p + 3];
  const float* __restrict__ y = Y + col[p];
  const float* __restrict__ tab = pw + (long)pw_row[p] * ldpw;
  const long rest = n_prob - (long)blockIdx.x * 64;
  const long m = rest < 64 ? rest : 64;                          // problems of this wave
  const long base = (long)blockIdx.x * T * 64 + threadIdx.x;     // pool d of this lane: base + m d
  const float one_g = 1.f - g;
  const float mu = lam * one_g;

  // ---- forward pass: pools 0 .. depth - 3 on the stack, pool depth - 2 in (pv, pwt, pt, pp), the top in (v, w, t0)
  int depth = 0;
  float v = 0.f, w = 0.f, pv = 0.f, pwt = 0.f, pp = 0.f;
  int t0 = 0, pt = 0;
  float y_next = y[0];
  for (int t = 0; t < T; ++t) {
    const float yt = y_next;
    if (t + 1 < T) y_next = y[(long)(t + 1) * ldy];
    if (depth >= 2) {                  // the pool under the top leaves the registers
      const long a = base + m * (depth - 2);
      st_v[a] = pv, st_w[a] = pwt, st_t0[a] = pt;
    }
    if (depth >= 1) {
      pv = v, pwt = w, pt = t0;
      pp = tab[t - t0];                // the length of the pool that is now under the top
    }
    const float yb = yt - b;
    v = yb - (t < T - 1 ? mu : lam), w = 1.f, t0 = t;
    ++depth;
    // Every iteration pops one pool and the loop stops at depth 1.  At frame t the stack holds at most t + 1 pools, so
    // at most t iterations run: `room` carries that bound, the loop ends whatever the data are (a NaN never compares
    // true, so it never merges), and it waits for nobody.
    for (int room = t; room > 0; --room) {
      if (depth < 2) break;
      const float lim = pv * pp;
      if (!(v < lim + s_min)) break;
      const float a1 = pwt * pv;
      const float pw_i = pp * w;
      const float a2 = pw_i * v;
      const float num = a1 + a2;
      const float p2 = pp * pp;
      const float d2 = p2 * w;
      const float den = pwt + d2;
      v = num / den, w = den, t0 = pt;
      --depth;
      if (depth >= 2) {                // the pool that enters the registers
        const long a = base + m * (depth - 2);
        pv = st_v[a], pwt = st_w[a], pt = st_t0[a];
        pp = tab[t0 - pt];
      }
    }
  }
  if (depth >= 2) {
    const long a = base + m * (depth - 2);
    st_v[a] = pv, st_t0[a] = pt;
  }
  st_v[base + m * (depth - 1)] = v, st_t0[base + m * (depth - 1)] = t0;
  if (n_pools) n_pools[p] = depth;
  if (!C && !S && !rss) return;

  // ---- fill pass: pool k is (vp, start), the next one begins at frame `next`
  int k = -1, next = 0, start = 0;
  float vp = 0.f, c_prev = 0.f;
  double acc = 0.0;
  float y_cur = y[0];
  for (int t = 0; t < T; ++t) {
    const float yt = y_cur;
    if (t + 1 < T) y_cur = y[(long)(t + 1) * ldy];
    const bool first = t == next;
    if (first) {
      ++k;
      const float vk = st_v[base + m * k];
      vp = vk > 0.f ? vk : 0.f;
      start = t;
      next = k + 1 < depth ? st_t0[base + m * (k + 1)] : T;
    }
    const float c = vp * tab[t - start];
    float s = 0.f;
    if (first && k >= 1) {
      const float gc = g * c_prev;
      const float d = c - gc;
      s = d > 0.f ? d : 0.f;
    }
    c_prev = c;
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

size_t pmd_oasis_ar1_workspace_bytes(long T, long n_prob) {
  if (T < 1 || n_prob < 1) return 0;
  return (size_t)12 * (size_t)n_prob * (size_t)T;
}

int pmd_oasis_ar1(pmd_ctx* ctx, const float* Y, long ldy, long T, long n_prob, const int* col, const float* par,
                  const int* pw_row, const float* pw, long ldpw, float* C, long ldc, float* S, long lds, double* rss,
                  int* n_pools, void* ws, size_t ws_bytes) {
  CTX_CHECK(ctx);
  const char* what = "pmd_oasis_ar1";
  if (T < 1 || T >= 0x7fffffffL || n_prob < 1 || ldy < 1 || ldpw < T + 1)
    return pmd_fail(ctx, PMD_ERR_ARG, what, "bad scalar argument (1 <= T < 2^31 - 1, n_prob >= 1, ldy >= 1, ldpw >= T + 1)");
  if ((C && ldc < n_prob) || (S && lds < n_prob))
    return pmd_fail(ctx, PMD_ERR_ARG, what, "ldc or lds smaller than n_prob");
  if (!Y || !col || !par || !pw || !pw_row) return pmd_fail(ctx, PMD_ERR_ARG, what, "null pointer");
  if (!C && !S && !rss && !n_pools) return pmd_fail(ctx, PMD_ERR_ARG, what, "no output requested");
  const long blocks = (n_prob + 63) / 64;
  if (blocks > 0x7fffffffL) return pmd_fail(ctx, PMD_ERR_ARG, what, "too many problems in one call");
  if (!ws || ws_bytes < pmd_oasis_ar1_workspace_bytes(T, n_prob))
    return pmd_fail(ctx, PMD_ERR_WORKSPACE, what, "workspace smaller than pmd_oasis_ar1_workspace_bytes(T, n_prob)");
  pmd_prof_scope prof__(ctx, "oasis_ar1");
  const size_t pools = (size_t)n_prob * (size_t)T;
  float* st_v = (float*)ws;
  float* st_w = st_v + pools;
  int* st_t0 = (int*)(st_w + pools);
  hipLaunchKernelGGL(oasis_ar1_kernel, dim3((unsigned)blocks), dim3(64), 0, ctx->stream, Y, ldy, (int)T, n_prob, col, par,
                     pw_row, pw, ldpw, C, ldc, S, lds, rss, n_pools, st_v, st_w, st_t0);
  PMD_LAUNCH_CHECK(ctx, "oasis_ar1_kernel");
  return PMD_OK;
}

}  // extern "C"
